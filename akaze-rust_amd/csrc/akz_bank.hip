// k_bank_gather: the 64-byte descriptor rows of many extraction results into the one row buffer of a feature bank
// (akz_bank_api.cpp), ONE launch whatever the number of results and images.  k_bank_select, below it: the same for a bank under a
// keypoint budget, where every destination row names its source row through the budget's index list.
//
// The host hands over a table of segments {source rows, row count, first destination row}, one per image of every result in
// bank order, so that dst_row0 never decreases and segment s + 1 starts where segment s ends; an image without keypoints is a
// segment of 0 rows that shares its dst_row0 with the next one.  The destination decides the work: workgroup b owns the
// kRowsPerWg destination rows from b * kRowsPerWg on, whichever segments they fall into -- no atomics, no tickets, nothing that
// depends on the order workgroups are dispatched in.  It finds the segment of its first row by a bisection of the table (read
// directly: 24 bytes per image, uniform over the workgroup); a lane then steps forward from there to the segment of its own row,
// which is the LAST one whose dst_row0 is not beyond the row -- empty segments are stepped over and cost nothing else.
//
// Access shape.  Four lanes per row, 16 bytes each: one 16-byte load, one 16-byte store, a wave covers 1 KiB of consecutive
// destination bytes.  Bytes of a row at or beyond desc_bytes are stored as zero whatever the source holds (the scans' contract
// for a row is "rest zero"); a lane whose 16 bytes lie wholly beyond desc_bytes does not load.  Sources and the destination
// are 16-byte aligned (rows of 64 bytes in blocks the runtime allocated).  Every offset is 64-bit.  No LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "akz_internal.hpp"

namespace akz {
namespace {

constexpr int BT = 256;                      // lanes per workgroup: 64 rows per pass
constexpr uint32_t kPasses = 4;              // passes of a workgroup
constexpr uint32_t kRowsPerWg = BT / 4 * kPasses;

__global__ __launch_bounds__(BT) void k_bank_gather(const launch::BankSeg* __restrict__ tab, uint32_t n_seg, uint64_t total_rows,
                                                    uint32_t desc_bytes, uint8_t* __restrict__ dst) {
    const uint64_t row0 = (uint64_t)blockIdx.x * kRowsPerWg;
    uint32_t lo = 0, hi = n_seg;  // tab[0].dst_row0 == 0: the last segment that starts at or in front of row0 lies in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tab[mid].dst_row0 <= row0) lo = mid;
        else hi = mid;
    }
    uint32_t s = lo;
    const uint32_t q = threadIdx.x & 3;
    uint32_t keep[4];  // which bytes of the lane's four words lie in front of desc_bytes
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t base = 16 * q + 4 * w, n = desc_bytes > base ? min(desc_bytes - base, 4u) : 0u;
        keep[w] = n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
    }
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        const uint64_t r = row0 + (uint64_t)pass * (BT / 4) + (threadIdx.x >> 2);
        if (r >= total_rows) return;
        while (s + 1 < n_seg && tab[s + 1].dst_row0 <= r) ++s;
        const launch::BankSeg seg = tab[s];
        const uint64_t i = r - seg.dst_row0;
        if (i >= seg.n_rows) continue;  // (a table that leaves a gap: nothing is read for rows no segment covers)
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (keep[0]) v = *reinterpret_cast<const uint4*>(seg.src_rows + i * 64 + 16 * q);
        v.x &= keep[0], v.y &= keep[1], v.z &= keep[2], v.w &= keep[3];
        *reinterpret_cast<uint4*>(dst + r * 64 + 16 * q) = v;
    }
}

// k_bank_select: the same shape for a bank under a keypoint budget -- destination row r is row t = r - dst_row0 of set s, and
// the row it receives is the one the budget's index list names, i = idx[idx_off + t].  The table is bisected and stepped over as
// above.  What differs from the plain gather is the source side: the four lanes of a row still read 64 consecutive bytes, but
// consecutive rows of a wave come from ascending, NOT contiguous addresses, and the address hangs on a load of its own.  So a
// lane first fetches the indices of all its kPasses rows, then issues all its row loads, then stores: the kPasses dependent
// chains run side by side.  Lane 0 of a row's four also carries x, y and the source index to the bank.  The indices are
// trusted: they come from launch::budget, or from akz_debug_bank_select, which checks them.
__global__ __launch_bounds__(BT) void k_bank_select(const launch::BankSel* __restrict__ tab, uint32_t n_set, uint64_t total_rows,
                                                    uint32_t desc_bytes, const uint32_t* __restrict__ idx, const float* __restrict__ sx,
                                                    const float* __restrict__ sy, uint8_t* __restrict__ dst, float* __restrict__ dx,
                                                    float* __restrict__ dy, uint32_t* __restrict__ dst_src) {
    const uint64_t row0 = (uint64_t)blockIdx.x * kRowsPerWg;
    uint32_t lo = 0, hi = n_set;  // tab[0].dst_row0 == 0: the last set that starts at or in front of row0 lies in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tab[mid].dst_row0 <= row0) lo = mid;
        else hi = mid;
    }
    uint32_t s = lo;
    const uint32_t q = threadIdx.x & 3;
    uint32_t keep[4];  // which bytes of the lane's four words lie in front of desc_bytes
#pragma unroll
    for (uint32_t w = 0; w < 4; ++w) {
        const uint32_t base = 16 * q + 4 * w, n = desc_bytes > base ? min(desc_bytes - base, 4u) : 0u;
        keep[w] = n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
    }
    bool live[kPasses];
    uint32_t i[kPasses];
    const uint8_t* src[kPasses];
    uint64_t xy[kPasses];
#pragma unroll
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        const uint64_t r = row0 + (uint64_t)pass * (BT / 4) + (threadIdx.x >> 2);
        live[pass] = r < total_rows;
        i[pass] = 0;
        src[pass] = nullptr;
        xy[pass] = 0;
        if (!live[pass]) continue;
        while (s + 1 < n_set && tab[s + 1].dst_row0 <= r) ++s;
        const launch::BankSel set = tab[s];
        const uint64_t t = r - set.dst_row0;
        live[pass] = t < set.keep;  // (a table that leaves a gap: nothing is read for rows no set covers)
        if (!live[pass]) continue;
        i[pass] = idx[set.idx_off + t];
        src[pass] = set.src_rows;
        xy[pass] = set.src_base;
    }
    uint4 v[kPasses];
    float x[kPasses], y[kPasses];
#pragma unroll
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        v[pass] = make_uint4(0u, 0u, 0u, 0u);
        x[pass] = y[pass] = 0.0f;
        if (!live[pass]) continue;
        if (keep[0]) v[pass] = *reinterpret_cast<const uint4*>(src[pass] + (uint64_t)i[pass] * 64 + 16 * q);
        if (q == 0) x[pass] = sx[xy[pass] + i[pass]], y[pass] = sy[xy[pass] + i[pass]];
    }
#pragma unroll
    for (uint32_t pass = 0; pass < kPasses; ++pass) {
        if (!live[pass]) continue;
        const uint64_t r = row0 + (uint64_t)pass * (BT / 4) + (threadIdx.x >> 2);
        uint4 o = v[pass];
        o.x &= keep[0], o.y &= keep[1], o.z &= keep[2], o.w &= keep[3];
        *reinterpret_cast<uint4*>(dst + r * 64 + 16 * q) = o;
        if (q == 0) dx[r] = x[pass], dy[r] = y[pass], dst_src[r] = i[pass];
    }
}

}  // namespace

namespace launch {
void bank_select(hipStream_t s, const BankSel* d_tab, uint32_t n_set, uint64_t total_rows, uint32_t desc_bytes, const uint32_t* d_idx,
                 const float* d_sx, const float* d_sy, uint8_t* d_dst, float* d_dx, float* d_dy, uint32_t* d_dst_src) {
    if (!n_set || !total_rows) return;
    const uint64_t wgs = (total_rows + kRowsPerWg - 1) / kRowsPerWg;
    hipLaunchKernelGGL(k_bank_select, dim3((uint32_t)wgs), dim3(BT), 0, s, d_tab, n_set, total_rows, desc_bytes, d_idx, d_sx, d_sy, d_dst,
                       d_dx, d_dy, d_dst_src);
}
void bank_gather(hipStream_t s, const BankSeg* d_tab, uint32_t n_seg, uint64_t total_rows, uint32_t desc_bytes, uint8_t* d_dst) {
    if (!n_seg || !total_rows) return;
    const uint64_t wgs = (total_rows + kRowsPerWg - 1) / kRowsPerWg;
    hipLaunchKernelGGL(k_bank_gather, dim3((uint32_t)wgs), dim3(BT), 0, s, d_tab, n_seg, total_rows, desc_bytes, d_dst);
}
}  // namespace launch
}  // namespace akz
