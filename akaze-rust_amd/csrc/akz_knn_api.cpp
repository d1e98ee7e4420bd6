// k-nearest-neighbour descriptor matching (additions; include/akaze_hip.h): knn(A, B, k, threshold) gives every row of
// A its k nearest rows of B below the threshold, ordered by (distance, index), with their distances.
// akz_descriptor_match_knn_host is the statement -- a popcount scan with a sorted insertion.  On the GPU the distances come from
// the FP4 matrix instruction (akz_knn.hip: k_knn_fp4<K> over launch::unpack_pair's images, k_knn_merge<K> over the partial lists).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "akz_ctx.hpp"
#include "akz_match_rule.hpp"

namespace {

constexpr uint64_t kNoRow = ~0ull;

bool knn_args_ok(const char* name, const void* d0, uint64_t n0, const void* d1, uint64_t n1, uint64_t desc_bytes, uint64_t k, const void* out,
                 const void* counts) {
    if (k == 0 || k > AKZ_KNN_MAX_K) {
        set_error(std::string(name) + "k must be 1.." + std::to_string(AKZ_KNN_MAX_K));
        return false;
    }
    if (desc_bytes == 0 || desc_bytes > 64 || !out || !counts || (n0 && !d0) || (n1 && !d1) || n0 > 0x7fffffffull || n1 > 0x7fffffffull) {
        set_error(std::string(name) + "bad arguments (desc_bytes must be 1..64, at most 2^31 - 1 rows a side)");
        return false;
    }
    return true;
}

// scan, merge and records of n0 x n1 64-byte rows on the device, enqueued on c->stream
int knn_enqueue(akz_ctx* c, const uint8_t* d_d0, uint32_t n0, const uint8_t* d_d1, uint32_t n1, uint32_t k, uint64_t distance_threshold,
                akz_match* d_out, uint32_t* d_counts) {
    const uint32_t thr = akz::clamp_threshold(distance_threshold);
    const uint32_t chunks = launch::knn_chunks(n0, n1, c->settings.dbg_knn_chunks);
    const uint32_t q_rows = launch::match_mfma_rows(n0, true), t_rows = launch::match_mfma_rows(n1, false);
    AKZ_TRY(ensure(c, c->kn_part, launch::knn_part_bytes(n0, chunks, k)));
    if (n1) {  // (the matcher's own images: like every user of them, on c->stream only)
        AKZ_TRY(ensure(c, c->ms[0].q8, (size_t)q_rows * 512));
        AKZ_TRY(ensure(c, c->ms[0].t8, (size_t)t_rows * 512));
        AKZ_TRY(ensure(c, c->ms[0].pop, ((size_t)2 * q_rows + t_rows) * sizeof(uint32_t)));
        uint32_t* qpop = (uint32_t*)c->ms[0].pop.p;
        uint32_t* tpop = qpop + 2 * (size_t)q_rows;
        launch::unpack_pair(c->stream, d_d0, n0, q_rows, (uint8_t*)c->ms[0].q8.p, qpop, nullptr, thr, d_d1, n1, t_rows, (uint8_t*)c->ms[0].t8.p, tpop,
                            true);
    }
    if (!launch::knn(c->stream, (const uint8_t*)c->ms[0].q8.p, n0, (const uint8_t*)c->ms[0].t8.p, n1, thr, chunks, k, (uint32_t*)c->kn_part.p, d_out,
                     d_counts)) {
        set_error("descriptor_match_knn: the kernel was built for another tile of the matcher");
        return AKZ_ERR_UNSUPPORTED;
    }
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

}  // namespace

extern "C" {

int akz_descriptor_match_knn_host(const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint64_t k,
                                  uint64_t distance_threshold, akz_match* out, uint32_t* counts) {
    if (!knn_args_ok("descriptor_match_knn_host: ", d0, n0, d1, n1, desc_bytes, k, out, counts)) return AKZ_ERR_INVALID_ARG;
    const uint32_t thr = akz::clamp_threshold(distance_threshold);
    for (uint64_t i = 0; i < n0; ++i) {
        const uint8_t* a = d0 + i * desc_bytes;
        uint32_t kd[AKZ_KNN_MAX_K];
        uint64_t kj[AKZ_KNN_MAX_K];
        uint32_t cnt = 0;
        for (uint64_t j = 0; j < n1; ++j) {
            const uint32_t d = akz::hamming_bytes(a, d1 + j * desc_bytes, desc_bytes);
            // rows come in ascending j: among equal distances the earlier row stays in front, and a full list takes d only below its worst
            if (d >= thr || (cnt == k && d >= kd[cnt - 1])) continue;
            uint32_t at = cnt < k ? cnt++ : cnt - 1;
            for (; at > 0 && kd[at - 1] > d; --at) {
                kd[at] = kd[at - 1];
                kj[at] = kj[at - 1];
            }
            kd[at] = d;
            kj[at] = j;
        }
        for (uint64_t r = 0; r < k; ++r)
            out[i * k + r] = r < cnt ? akz_match{i, kj[r], (double)kd[r]} : akz_match{i, kNoRow, std::numeric_limits<double>::infinity()};
        counts[i] = cnt;
    }
    return AKZ_OK;
}

int akz_descriptor_match_knn_device(akz_ctx* c, const uint8_t* d_d0, uint64_t n0, const uint8_t* d_d1, uint64_t n1, uint64_t k,
                                    uint64_t distance_threshold, akz_match* d_out, uint32_t* d_counts) {
    AKZ_TRY(bind(c, true, false));
    if (!knn_args_ok("descriptor_match_knn_device: ", d_d0, n0, d_d1, n1, 61, k, d_out, d_counts)) return AKZ_ERR_INVALID_ARG;
    if (n0 == 0) return AKZ_OK;
    return knn_enqueue(c, d_d0, (uint32_t)n0, d_d1, (uint32_t)n1, (uint32_t)k, distance_threshold, d_out, d_counts);
}

int akz_descriptor_match_knn(akz_ctx* c, const uint8_t* d0, uint64_t n0, const uint8_t* d1, uint64_t n1, uint64_t desc_bytes, uint64_t k,
                             uint64_t distance_threshold, akz_match* out, uint32_t* counts) {
    AKZ_TRY(bind(c, true, false));
    if (!knn_args_ok("descriptor_match_knn: ", d0, n0, d1, n1, desc_bytes, k, out, counts)) return AKZ_ERR_INVALID_ARG;
    if (desc_bytes > 61) {
        set_error("descriptor_match_knn: rows of 62..64 bytes are not supported on the GPU (the FP4 image carries 488 columns)");
        return AKZ_ERR_UNSUPPORTED;
    }
    if (n0 == 0) return AKZ_OK;
    // both sets as 64-byte rows in one block (A, then B), the records and the counts behind them
    hipStream_t st = c->stream;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    std::vector<uint8_t> rows((size_t)(n0 + n1) * 64, 0);
    for (uint64_t i = 0; i < n0; ++i) std::memcpy(&rows[(size_t)i * 64], d0 + i * desc_bytes, (size_t)desc_bytes);
    for (uint64_t i = 0; i < n1; ++i) std::memcpy(&rows[(size_t)(n0 + i) * 64], d1 + i * desc_bytes, (size_t)desc_bytes);
    const size_t b_rows = up(rows.size()), b_out = up((size_t)n0 * k * sizeof(akz_match)), b_cnt = up((size_t)n0 * sizeof(uint32_t));
    AKZ_TRY(ensure(c, c->kn_io, b_rows + b_out + b_cnt));
    uint8_t* d_rows = (uint8_t*)c->kn_io.p;
    akz_match* d_out = (akz_match*)(d_rows + b_rows);
    uint32_t* d_cnt = (uint32_t*)(d_rows + b_rows + b_out);
    AKZ_HIP_TRY(hipMemcpyAsync(d_rows, rows.data(), rows.size(), hipMemcpyHostToDevice, st));
    AKZ_TRY(knn_enqueue(c, d_rows, (uint32_t)n0, d_rows + (size_t)n0 * 64, (uint32_t)n1, (uint32_t)k, distance_threshold, d_out, d_cnt));
    AKZ_HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n0 * k * sizeof(akz_match), hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipMemcpyAsync(counts, d_cnt, (size_t)n0 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    return AKZ_OK;
}

int akz_debug_set_knn_chunks(akz_ctx* c, uint32_t chunks) {  // include/akaze_hip_debug.h
    AKZ_TRY(bind(c));
    c->settings.dbg_knn_chunks = chunks;
    push_settings(c);
    return AKZ_OK;
}

}  // extern "C"
