// Cross-checked matching (additions; include/akaze_hip.h): cross(A, B) keeps a record of descriptor_match(A, B) only
// if descriptor_match(B, A) holds the record that points back.  akz_descriptor_match_cross_host is the statement -- two plain
// scans of feature_matching.rs:23-94 and a lookup.  On the GPU both directions come from the matcher -- one pass over the
// distances on the FP4 kernel (akz::match_sets_at with the opposite direction, pairs_scans with `cross`), two scans on the other
// matcher kernels and for rows of 62..64 bytes -- and launch::pair(s)_cross_filter rewrites the forward list in place.
// akz_match_features_seeded_cross_pairs is the seeded pairs call (akz_match_seeded_api.cpp) with that list in front of RANSAC.
#include <algorithm>
#include <cstring>
#include <vector>

#include "akz_ctx.hpp"
#include "akz_match_rule.hpp"

namespace {

// descriptor_match (feature_matching.rs:37-81) on the host: the ungated scan of akz_match_rule.hpp
std::vector<akz_match> host_scan(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint32_t thr, double ratio2) {
    std::vector<akz_match> out;
    akz::host_match_scan(d0, n0, d1, n1, desc_bytes, thr, ratio2, [](uint64_t, uint64_t) { return true; },
                         [&](const akz_match& m) { out.push_back(m); });
    return out;
}

bool host_args_ok(const char* name, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, const akz_match* out,
                  const uint64_t* n_out) {
    if (!n_out || desc_bytes == 0 || desc_bytes > 64 || (n0 && (!d0 || !out)) || (n1 && !d1)) {
        set_error(std::string(name) + "bad arguments (desc_bytes must be 1..64)");
        return false;
    }
    return true;
}

}  // namespace

extern "C" {

int akz_descriptor_match_cross_host(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes,
                                    uint64_t distance_threshold, double lowes_ratio, akz_match* out, uint64_t* n_out) {
    if (!host_args_ok("descriptor_match_cross_host: ", d0, n0, d1, n1, desc_bytes, out, n_out)) return AKZ_ERR_INVALID_ARG;
    const uint32_t thr = akz::clamp_threshold(distance_threshold);
    const double ratio2 = lowes_ratio * lowes_ratio;
    const std::vector<akz_match> fwd = host_scan(d0, n0, d1, n1, desc_bytes, thr, ratio2);
    const std::vector<akz_match> rev = host_scan(d1, n1, d0, n0, desc_bytes, thr, ratio2);
    std::vector<uint64_t> back((size_t)n1, ~0ull);  // row of B -> the row of A its reverse record names
    for (const akz_match& r : rev) back[(size_t)r.index_0] = r.index_1;
    uint64_t cnt = 0;
    for (const akz_match& m : fwd)
        if (back[(size_t)m.index_1] == m.index_0) out[cnt++] = m;
    *n_out = cnt;
    return AKZ_OK;
}

int akz_descriptor_match_cross_device(akz_ctx* c, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1,
                                      uint64_t distance_threshold, double lowes_ratio, akz_match* d_out, uint64_t* d_n_out) {
    AKZ_TRY(bind(c, true, false));
    if (!d_out || !d_n_out || (n0 && !d_d0) || (n1 && !d_d1) || n0 > 0x7fffffffull || n1 > 0x7fffffffull) {
        set_error("descriptor_match_cross: bad arguments");
        return AKZ_ERR_INVALID_ARG;
    }
    hipStream_t st = c->stream;
    if (n0 == 0 || n1 == 0) {  // an empty set on either side: the result is empty
        AKZ_HIP_TRY(hipMemsetAsync(d_n_out, 0, sizeof(uint64_t), st));
        return AKZ_OK;
    }
    const size_t b_rev = up256((size_t)n1 * sizeof(akz_match));
    AKZ_TRY(ensure(c, c->cx_rev, b_rev + 256));
    akz_match* d_rev = (akz_match*)c->cx_rev.p;
    uint64_t* d_rcnt = (uint64_t*)((char*)c->cx_rev.p + b_rev);
    const uint64_t first = 0;
    AKZ_TRY(akz::match_sets_at(c, d_d0, n0, d_d1, &first, &n1, 1, distance_threshold, lowes_ratio, d_out, d_n_out, d_rev, d_rcnt));
    launch::pair_cross_filter(st, launch::CrossJobHost{0, 0, 0, 0, (uint32_t)n0, (uint32_t)n1}, d_out, d_n_out, d_rev, d_rcnt);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

int akz_descriptor_match_cross(akz_ctx* c, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes,
                               uint64_t distance_threshold, double lowes_ratio, akz_match* out, uint64_t* n_out) {
    AKZ_TRY(bind(c, true, false));
    if (!host_args_ok("descriptor_match_cross: ", d0, n0, d1, n1, desc_bytes, out, n_out)) return AKZ_ERR_INVALID_ARG;
    if (n0 > 0x7fffffffull || n1 > 0x7fffffffull) {
        set_error("descriptor_match_cross: too many rows");
        return AKZ_ERR_INVALID_ARG;
    }
    *n_out = 0;
    if (n0 == 0 || n1 == 0) return AKZ_OK;
    // both sets as 64-byte rows in one block (A, then B); the lists and their counts beside them
    hipStream_t st = c->stream;
    std::vector<uint8_t> rows((size_t)(n0 + n1) * 64, 0);
    for (uint64_t i = 0; i < n0; ++i) std::memcpy(&rows[(size_t)i * 64], d0 + i * desc_bytes, (size_t)desc_bytes);
    for (uint64_t i = 0; i < n1; ++i) std::memcpy(&rows[(size_t)(n0 + i) * 64], d1 + i * desc_bytes, (size_t)desc_bytes);
    const size_t b_fwd = up256((size_t)n0 * sizeof(akz_match)), b_rev = up256((size_t)n1 * sizeof(akz_match));
    AKZ_TRY(ensure(c, c->match_a, rows.size()));
    AKZ_TRY(ensure(c, c->match_out, b_fwd + 256));
    AKZ_TRY(ensure(c, c->cx_rev, b_rev + 256));
    uint8_t* d_rows = (uint8_t*)c->match_a.p;
    akz_match* d_fwd = (akz_match*)c->match_out.p;
    uint64_t* d_cnt = (uint64_t*)((char*)c->match_out.p + b_fwd);
    akz_match* d_rev = (akz_match*)c->cx_rev.p;
    uint64_t* d_rcnt = (uint64_t*)((char*)c->cx_rev.p + b_rev);
    AKZ_HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice, st));
    akz_feature_set sets[2] = {{nullptr, 0, nullptr, n0}, {nullptr, 0, nullptr, n1}};  // (pairs_scans reads the row counts alone)
    const uint64_t pair[2] = {0, 1};
    // (pairs_scans reads c, sets, n_sets, pairs, n_pairs and desc_bytes of the call, set_row and d_rows of the block)
    SetsBlock block;
    block.place(sets, 2, {0, 1});
    block.d_rows = d_rows;
    std::vector<launch::PairJobHost> tab;
    std::vector<launch::CrossJobHost> xtab;
    AKZ_TRY(pairs_scans({"", c, sets, 2, pair, 1, desc_bytes, nullptr, nullptr, nullptr}, lowes_ratio, block, d_fwd, d_cnt, tab, d_rev, d_rcnt, &xtab, distance_threshold));
    launch::pair_cross_filter(st, xtab[0], d_fwd, d_cnt, d_rev, d_rcnt);
    AKZ_HIP_TRY(hipGetLastError());
    uint64_t cnt = 0;
    AKZ_HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    if (cnt) {
        AKZ_HIP_TRY(hipMemcpyAsync(out, d_fwd, (size_t)cnt * sizeof(akz_match), hipMemcpyDeviceToHost, st));
        AKZ_HIP_TRY(hipStreamSynchronize(st));
    }
    *n_out = cnt;
    return AKZ_OK;
}

int akz_debug_match_tile_rows(uint32_t* rows) {  // include/akaze_hip_debug.h
    if (!rows) return AKZ_ERR_INVALID_ARG;
    *rows = launch::match_mfma_tile_rows();
    return AKZ_OK;
}
int akz_debug_match_seed_rows(uint32_t n0, uint32_t* rows) {  // include/akaze_hip_debug.h
    if (!rows) return AKZ_ERR_INVALID_ARG;
    *rows = launch::match_cols_seed_rows(n0);
    return AKZ_OK;
}

int akz_match_features_seeded_cross_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                          uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out, uint64_t* n_out, float* model,
                                          int* found, uint32_t* iterations, uint64_t* trials_run) {
    return match_seeded_pairs_impl({"match_features_seeded_cross_pairs: ", c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr}, true,
                                   options, model, found, iterations, trials_run);
}

}  // extern "C"
