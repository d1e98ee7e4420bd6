// The cross-check of two match lists on the device (include/akaze_hip.h: cross(A, B); akz_cross_api.cpp):
//   k_pairs_cross_filter      per pair, the forward list rewritten in place to the records whose reverse record points back
#include <hip/hip_runtime.h>

#include <algorithm>

#include "akz_internal.hpp"

namespace akz {
namespace {

using CrossJob = launch::CrossJobHost;

constexpr unsigned CT = 256;  // four waves of 64

// One workgroup per pair.  fwd = descriptor_match(A, B) (ascending index_0 in A), rev = descriptor_match(B, A) (ascending index_0
// in B, each row of B at most once): forward record m survives iff rev holds r with r.index_0 == m.index_1 and r.index_1 ==
// m.index_0 -- a binary search for m.index_1.  The survivors are compacted in order by ballot and prefix over the four waves.
// In place: a round reads its 256 records into registers, meets at a barrier and only then writes, to places at or below the
// ones it read -- so a write never reaches a record that is still to be read, and no other workgroup touches this list.
// Counts above the room of a list (fwd_cap, rev_cap) are cut to it.
__global__ void __launch_bounds__(CT) k_pairs_cross_filter(const CrossJob* __restrict__ tab, CrossJob one, akz_match* fwd_base,
                                                           unsigned long long* fwd_cnt, const akz_match* __restrict__ rev_base,
                                                           const unsigned long long* __restrict__ rev_cnt) {
    __shared__ unsigned s_cnt[CT / 64];
    const CrossJob j = tab ? tab[blockIdx.x] : one;
    akz_match* fwd = fwd_base + j.fwd_off;
    const akz_match* rev = rev_base + j.rev_off;
    const unsigned long long n = min(fwd_cnt[j.fwd_cnt_idx], (unsigned long long)j.fwd_cap);
    const unsigned long long m = min(rev_cnt[j.rev_cnt_idx], (unsigned long long)j.rev_cap);
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long kept = 0;  // (the same value in every thread)
    for (unsigned long long start = 0; start < n; start += CT) {
        const unsigned long long i = start + threadIdx.x;
        akz_match rec;
        rec.index_0 = rec.index_1 = 0;
        rec.distance = 0.0;
        bool keep = false;
        if (i < n) {
            rec = fwd[i];
            unsigned long long lo = 0, hi = m;  // the first reverse record with index_0 >= rec.index_1
            while (lo < hi) {
                const unsigned long long mid = lo + (hi - lo) / 2;
                if (rev[mid].index_0 < rec.index_1) lo = mid + 1;
                else hi = mid;
            }
            if (lo < m) {
                const akz_match r = rev[lo];
                keep = r.index_0 == rec.index_1 && r.index_1 == rec.index_0;
            }
        }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_cnt[wave] = (unsigned)__popcll(bal);
        __syncthreads();  // every record of the round is in registers, every wave's count in LDS
        unsigned below = 0, total = 0;
#pragma unroll
        for (unsigned w = 0; w < CT / 64; ++w) {
            const unsigned c = s_cnt[w];
            total += c;
            below += w < wave ? c : 0u;
        }
        if (keep) fwd[kept + below + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = rec;
        kept += total;
        __syncthreads();  // the counts are read before the next round writes them
    }
    __syncthreads();  // (an empty list: every thread has read the count before it is written)
    if (threadIdx.x == 0) fwd_cnt[j.fwd_cnt_idx] = kept;
}

}  // namespace

namespace launch {

void pairs_cross_filter(hipStream_t s, const CrossJobHost* d_tab, uint32_t n_pairs, akz_match* d_fwd, uint64_t* d_fwd_cnt,
                        const akz_match* d_rev, const uint64_t* d_rev_cnt) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_pairs_cross_filter, dim3(n_pairs), dim3(CT), 0, s, d_tab, CrossJobHost{}, d_fwd, (unsigned long long*)d_fwd_cnt, d_rev,
                       (const unsigned long long*)d_rev_cnt);
}
void pair_cross_filter(hipStream_t s, const CrossJobHost& job, akz_match* d_fwd, uint64_t* d_fwd_cnt, const akz_match* d_rev,
                       const uint64_t* d_rev_cnt) {
    hipLaunchKernelGGL(k_pairs_cross_filter, dim3(1), dim3(CT), 0, s, (const CrossJobHost*)nullptr, job, d_fwd, (unsigned long long*)d_fwd_cnt,
                       d_rev, (const unsigned long long*)d_rev_cnt);
}

}  // namespace launch
}  // namespace akz
