// The two layouts the pairs calls and the feature banks share, each stated once.  Plain host code: no HIP header, so that a CPU
// program can include it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/akaze_hip.h"

namespace akz {
inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }  // the parts of one buffer start on 256 bytes

// Feature sets placed in one block of memory: rows (64 bytes each) | x | y (| src), every part on 256 bytes; set k's rows and the x / y
// of its first n_descriptors keypoints -- the only ones a match can name -- start at row set_row[k].  c->mp_in, its pinned image
// c->mp_pin_in and a bank's `dev` are such blocks.
struct SetsBlock {
    std::vector<uint64_t> set_row;  // one per set; 0 for a set that is not placed
    uint64_t rows = 0;              // of all placed sets
    size_t b_rows = 0, b_xy = 0;    // bytes of the rows and of x (y and src: as x), for at least one row
    uint8_t* d_rows = nullptr;
    float *d_kx = nullptr, *d_ky = nullptr;
    uint32_t* d_src = nullptr;  // a budgeted bank's source indices; null without

    // the sets `order` names, one behind the other in that order
    void place(const akz_feature_set* sets, uint64_t n_sets, const std::vector<uint64_t>& order) {
        set_row.assign((size_t)n_sets, 0);
        rows = 0;
        for (uint64_t k : order) {
            set_row[(size_t)k] = rows;
            rows += sets[k].n_descriptors;
        }
        const uint64_t rows1 = std::max<uint64_t>(rows, 1);
        b_rows = up256((size_t)rows1 * 64), b_xy = up256((size_t)rows1 * 4);
    }
    size_t bytes(bool with_src) const { return b_rows + (with_src ? 3 : 2) * b_xy; }
    void bind(void* base, bool with_src) {
        d_rows = (uint8_t*)base;
        d_kx = (float*)(d_rows + b_rows), d_ky = (float*)(d_rows + b_rows + b_xy);
        d_src = with_src ? (uint32_t*)(d_rows + b_rows + 2 * b_xy) : nullptr;
    }
};
inline std::vector<uint64_t> index_order(uint64_t n_sets) {  // every set, as a bank places them
    std::vector<uint64_t> order((size_t)n_sets);
    for (uint64_t k = 0; k < n_sets; ++k) order[(size_t)k] = k;
    return order;
}

// The kept block of a RANSAC pairs call (c->mp_keep and its pinned image c->mp_pin_out): a head of kept counts | models | found |
// accepted fits | trials run | poses | points (3 floats per kept record, where want_points), then the kept lists.  The caller sets the
// five byte counts (0: the field is absent, and its pointer is the next field's) and want_points, pairs_keep the rest.
struct PairsHead {
    uint64_t* cnt;
    float* model;
    int32_t* found;
    uint32_t *fits, *trials;
    akz_pose* pose;
    float* points;
    akz_match* keep;
    size_t bytes;  // of the head
};
struct PairsKeep {
    size_t b_model, b_found, b_fits, b_trials;
    size_t b_pose = 0;
    bool want_points = false;
    size_t b_cnt = 0, b_points = 0;
    uint64_t n_keep = 0;
    PairsHead d{};  // on the device
};
inline PairsHead pairs_head(void* base, const PairsKeep& k) {  // base null: the size alone
    size_t off = 0;
    auto part = [&](size_t bytes) {
        char* p = base ? (char*)base + off : nullptr;
        off += bytes;
        return p;
    };
    PairsHead h{};
    h.cnt = (uint64_t*)part(k.b_cnt);
    h.model = (float*)part(k.b_model);
    h.found = (int32_t*)part(k.b_found);
    h.fits = (uint32_t*)part(k.b_fits);  // fits | trials | poses stay together: the seeded call zeroes [fits, points) with one memset
    h.trials = (uint32_t*)part(k.b_trials);
    h.pose = (akz_pose*)part(k.b_pose);
    h.points = (float*)part(k.b_points);
    h.keep = (akz_match*)part(0);
    h.bytes = off;
    return h;
}
}  // namespace akz
