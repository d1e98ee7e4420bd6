// The keypoint budget on the device (include/akaze_hip.h: AKZ_BUDGET_*; akz_budget_api.cpp holds the host statement):
//   k_budget_init        radius2 := +inf, rank := 0
//   k_budget_walk<RANK>  the all-pairs tile walk: <false> the suppression radius of every keypoint, <true> its place in the order
//   k_budget_compact     per set, the indices with rank < keep, ascending
// Every float operation is one f32 operation of the statement (the build never contracts and keeps subnormals); minimum and count
// depend on no order, so the atomics that merge the partial results of a keypoint's train chunks give the statement's bits.
#include <hip/hip_runtime.h>

#include "akz_internal.hpp"

namespace akz {
namespace {

using launch::BudgetBlock;
using launch::BudgetSet;

constexpr unsigned WT = 256;       // threads of a walk workgroup: four waves of 64
constexpr unsigned QPL = 4;        // queries per lane, in registers
constexpr unsigned QT = WT * QPL;  // queries per workgroup
constexpr unsigned TT = WT;        // train keypoints per LDS stage: every thread stages one
constexpr unsigned CT = 1024;      // threads of a compaction workgroup

constexpr unsigned kInfBits = 0x7f800000u;

__global__ void __launch_bounds__(256) k_budget_init(float* __restrict__ radius2, unsigned* __restrict__ rank, unsigned total) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < total) {
        radius2[i] = __uint_as_float(kInfBits);
        rank[i] = 0u;
    }
}

// One workgroup: QT queries of one set, QPL per lane in registers (query q0 + k * WT + thread), against the set's keypoints
// [t0, t1), staged TT at a time through LDS as 16-byte records that every lane reads at the same address (a broadcast).
//   RANK = false  query (x, y, r | min), train (x, y, fl(robust * r)):  min = min(min, d2) where r_i < fl(robust * r_j)
//   RANK = true   query (radius2, r, index | count), train the same three: count += j stands before i in
//                 (radius2 descending, r descending, index ascending)
// A stage's tail beyond t1 holds records that change nothing (a train response of -inf dominates nobody; a radius of -1 is below
// every radius2 >= 0), so the inner loop runs without bounds.  Queries beyond the set compute and store nothing.
template <bool RANK>
__global__ void __launch_bounds__(WT) k_budget_walk(const BudgetSet* __restrict__ sets, const BudgetBlock* __restrict__ blocks,
                                                    const float* __restrict__ gx, const float* __restrict__ gy,
                                                    const float* __restrict__ gr, float robust, float* radius2, unsigned* rank) {
    __shared__ float4 s_t[TT];
    const BudgetBlock b = blocks[blockIdx.x];
    const BudgetSet s = sets[b.set];
    const unsigned tid = threadIdx.x;
    float qa[QPL], qb[QPL], qr[QPL], qm[QPL];  // RANK: (radius2, r, -, -), else (x, y, r, the minimum so far)
    unsigned qi[QPL], qc[QPL];                 // the query's index in its set; RANK: the keypoints found before it so far
    bool live[QPL];
#pragma unroll
    for (unsigned k = 0; k < QPL; ++k) {
        const unsigned q = b.q0 + k * WT + tid;
        live[k] = q < s.n;
        qi[k] = q;
        qc[k] = 0u;
        qm[k] = __uint_as_float(kInfBits);
        qa[k] = qb[k] = qr[k] = 0.0f;
        if (live[k]) {
            qa[k] = RANK ? radius2[s.base + q] : gx[s.base + q];
            qb[k] = RANK ? gr[s.base + q] : gy[s.base + q];
            if (!RANK) qr[k] = gr[s.base + q];
        }
    }

    for (unsigned t = b.t0; t < b.t1; t += TT) {
        const unsigned j = t + tid;
        float4 rec;
        if (j < b.t1) {
            if (RANK) rec = make_float4(radius2[s.base + j], gr[s.base + j], __uint_as_float(j), 0.0f);
            else rec = make_float4(gx[s.base + j], gy[s.base + j], robust * gr[s.base + j], 0.0f);
        } else {
            rec = RANK ? make_float4(-1.0f, 0.0f, __uint_as_float(0xffffffffu), 0.0f) : make_float4(0.0f, 0.0f, -__uint_as_float(kInfBits), 0.0f);
        }
        __syncthreads();  // the stage before has been read by every wave
        s_t[tid] = rec;
        __syncthreads();
        const unsigned cnt = min(TT, b.t1 - t);
        const unsigned lim = (cnt + 3u) & ~3u;
#pragma unroll 4
        for (unsigned u = 0; u < lim; ++u) {
            const float4 tr = s_t[u];
#pragma unroll
            for (unsigned k = 0; k < QPL; ++k) {
                if (RANK) {
                    const unsigned tj = __float_as_uint(tr.z);
                    const bool ahead = tr.x > qa[k] || (tr.x == qa[k] && (tr.y > qb[k] || (tr.y == qb[k] && tj < qi[k])));
                    qc[k] += ahead ? 1u : 0u;
                } else {
                    const float dx = qa[k] - tr.x, dy = qb[k] - tr.y;
                    const float xx = dx * dx, yy = dy * dy;
                    const float d2 = xx + yy;
                    qm[k] = (qr[k] < tr.z && d2 < qm[k]) ? d2 : qm[k];
                }
            }
        }
    }
#pragma unroll
    for (unsigned k = 0; k < QPL; ++k) {
        if (!live[k]) continue;
        if (RANK) {
            if (qc[k]) atomicAdd(rank + s.base + qi[k], qc[k]);
        } else {
            // d2 >= +0 and never NaN for finite inputs: the bits of such floats order as the values do
            if (__float_as_uint(qm[k]) != kInfBits) atomicMin((unsigned*)radius2 + s.base + qi[k], __float_as_uint(qm[k]));
        }
    }
}

// One workgroup per set: the indices i with rank_i < keep in ascending order to idx + out_off, by ballot and a prefix over the waves,
// CT keypoints a round.  The order is total, so exactly `keep` indices qualify.
__global__ void __launch_bounds__(CT) k_budget_compact(const BudgetSet* __restrict__ sets, const unsigned* __restrict__ rank,
                                                       unsigned* __restrict__ idx) {
    __shared__ unsigned s_cnt[CT / 64];
    const BudgetSet s = sets[blockIdx.x];
    if (s.keep == 0) return;  // (the same for the whole workgroup)
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned kept = 0;  // (the same value in every thread)
    for (unsigned start = 0; start < s.n; start += CT) {
        const unsigned i = start + threadIdx.x;
        const bool keep = i < s.n && rank[s.base + i] < s.keep;
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_cnt[wave] = (unsigned)__popcll(bal);
        __syncthreads();
        unsigned below = 0, total = 0;
#pragma unroll
        for (unsigned w = 0; w < CT / 64; ++w) {
            const unsigned c = s_cnt[w];
            total += c;
            below += w < wave ? c : 0u;
        }
        const unsigned at = kept + below + (unsigned)__popcll(bal & ((1ull << lane) - 1ull));
        if (keep && at < s.keep) idx[s.out_off + at] = i;  // (at < keep always; the bound keeps a set's list inside its room)
        kept += total;
        __syncthreads();  // the counts are read before the next round writes them
    }
}

}  // namespace

namespace launch {

uint32_t budget_query_tile() { return QT; }
uint32_t budget_train_tile() { return TT; }

void budget(hipStream_t st, bool spread, float robust, const float* d_x, const float* d_y, const float* d_r, uint32_t total,
            const BudgetSet* d_sets, uint32_t n_sets, const BudgetBlock* d_blocks, uint32_t n_blocks, float* d_radius2, uint32_t* d_rank,
            uint32_t* d_idx) {
    if (total == 0 || n_sets == 0) return;
    hipLaunchKernelGGL(k_budget_init, dim3((total + 255u) / 256u), dim3(256), 0, st, d_radius2, d_rank, total);
    if (n_blocks) {
        if (spread)
            hipLaunchKernelGGL(k_budget_walk<false>, dim3(n_blocks), dim3(WT), 0, st, d_sets, d_blocks, d_x, d_y, d_r, robust, d_radius2,
                               d_rank);
        hipLaunchKernelGGL(k_budget_walk<true>, dim3(n_blocks), dim3(WT), 0, st, d_sets, d_blocks, d_x, d_y, d_r, robust, d_radius2, d_rank);
    }
    hipLaunchKernelGGL(k_budget_compact, dim3(n_sets), dim3(CT), 0, st, d_sets, d_rank, d_idx);
}

}  // namespace launch
}  // namespace akz
