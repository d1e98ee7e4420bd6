// k-nearest-neighbour descriptor matching on the matrix cores (include/akaze_hip.h: knn(A, B, k, threshold); akz_knn_api.cpp;
// DESIGN.md 8):
//   k_knn_fp4<K>     per workgroup 512 queries against one chunk of the train set: every lane's K smallest keys
//   k_knn_merge<K>   per query the k smallest keys over all partial lists -> records, padding slots and counts
//
// The scan is the FP4 tile walk of akz_fp4_scan.hpp in its one-direction form (two tiles per barrier), as under k_match_fp4
// (akz_match.hip), with a sorted list as the visitor's state: the walk hands every lane the sixteen accumulators
// 488 - 2 hamming of its query to rows j0 + lane_row(i) of a 32-row sub-tile, ascending train index inside a lane.
//
// Keys.  A lane keeps K keys (d << 22 | row - first row of the chunk), ascending, in K registers: the order of keys is the
// order of (d, j), a chunk holds at most 2^22 rows (launch::knn_chunks sees to it) and d <= 488 < 2^9.  All K start at the
// sentinel threshold << 22 (threshold <= 489 here: the host clips it), which no key with d < threshold reaches, so `below the
// threshold` needs no test of its own.  A lane's rows arrive in ascending j, so a new row enters the list iff its distance is
// strictly below the worst kept distance: the fast path is one maximum over the 16 accumulators against 488 - 2 worst, as the
// top-2 scan compares against `second`; the slow path offers every accumulator above that limit to an unrolled compare-exchange
// chain (list[r], x = min, max -- static register indices only).  A key that does not belong falls out of the chain's end, so
// a stale limit costs time, never correctness.
//
// Partial lists.  The two lanes of a column hold disjoint rows, the chunks disjoint row ranges, and keys are totally ordered,
// so merging is order-free: every lane writes its list, part[((chunk * 2 + h) * K + slot) * n0 + query] (consecutive queries on
// consecutive lanes), and k_knn_merge<K> takes the K smallest of a query's 2 * chunks lists as 64-bit keys (d << 32 | j).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "akz_fp4_scan.hpp"
#include "akz_internal.hpp"

namespace akz {
namespace {

constexpr unsigned kRowBits = 22;  // key = d << kRowBits | row inside the chunk
constexpr unsigned kRowMask = (1u << kRowBits) - 1u;

// first tile of chunk c of `chunks` over `tiles` tiles: balanced, no chunk empty while chunks <= tiles
__host__ __device__ inline unsigned knn_chunk_tile(unsigned c, unsigned chunks, unsigned tiles) {
    return (unsigned)((unsigned long long)c * tiles / chunks);
}

// The walk's visitor: a lane's K smallest keys of the chunk that starts at tile t_begin.
template <int K>
struct KnnList : fp4::Visitor {
    unsigned list[K];
    float limf;  // accumulator of the worst kept distance: only rows ABOVE it enter
    unsigned t_begin;

    __device__ __forceinline__ void sub_tile(const v16f& acc, unsigned j0, int, int) {
        float topf = acc[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) topf = fmaxf(topf, acc[i]);
        if (topf > limf) {  // one of the lane's 16 rows is nearer than its worst kept one
            const unsigned jb = j0 - t_begin * fp4::TR;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (acc[i] > limf) {
                    unsigned x = ((unsigned)((fp4::kBits - (int)acc[i]) >> 1) << kRowBits) | (jb + fp4::lane_row(i));
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const unsigned lo = min(list[k], x);
                        x = max(list[k], x);
                        list[k] = lo;
                    }
                    limf = (float)(fp4::kBits - 2 * (int)(list[K - 1] >> kRowBits));
                }
            }
        }
    }
};

// blockIdx.x: 512 queries; blockIdx.y: a chunk of the train tiles.  q4 / t4: the FP4 images, rows padded to whole workgroups /
// whole tiles with zero rows; threshold <= 489.
template <int K>
__global__ void __launch_bounds__(fp4::NT) k_knn_fp4(const uint8_t* __restrict__ q4, unsigned n0, const uint8_t* __restrict__ t4, unsigned n1,
                                                     unsigned threshold, unsigned* __restrict__ part) {
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned r = lane & 31u, h = lane >> 5;
    const unsigned q = blockIdx.x * fp4::QB + wave * 32u + r;
    const fp4::Queries bq = fp4::load_queries(q4, q, h);
    KnnList<K> v;
#pragma unroll
    for (int k = 0; k < K; ++k) v.list[k] = threshold << kRowBits;
    v.limf = (float)(fp4::kBits - 2 * (int)threshold);
    const unsigned tiles_total = (n1 + fp4::TR - 1) / fp4::TR;
    v.t_begin = knn_chunk_tile(blockIdx.y, gridDim.y, tiles_total);
    fp4::walk<fp4::kStepOneWay, 1>(bq, t4, fp4::Chunk{v.t_begin, knn_chunk_tile(blockIdx.y + 1, gridDim.y, tiles_total), 0u, n1}, v);
    if (q < n0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[((size_t)(blockIdx.y * 2u + h) * K + k) * n0 + q] = v.list[k];
    }
}

// One thread per query: the K smallest keys over its 2 * chunks partial lists (none for an empty train set), then the k records
// of the query -- {query, row, distance}, and {query, ~0, +infinity} in the slots beyond its count -- and the count.
template <int K>
__global__ void __launch_bounds__(256) k_knn_merge(const unsigned* __restrict__ part, unsigned n0, unsigned chunks, unsigned tiles,
                                                   unsigned threshold, unsigned k_out, akz_match* __restrict__ out,
                                                   unsigned* __restrict__ counts) {
    const unsigned q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n0) return;
    unsigned long long best[K];
#pragma unroll
    for (int k = 0; k < K; ++k) best[k] = ~0ull;
    // (a list's K loads are issued together, and the loads of the next lists do not wait for this one's chains: a key enters a
    //  chain only below the worst kept one, which after the first lists is rare)
#pragma unroll 4
    for (unsigned l = 0; l < 2u * chunks; ++l) {
        const unsigned long long row0 = (unsigned long long)knn_chunk_tile(l >> 1, chunks, tiles) * fp4::TR;
        unsigned key[K];
#pragma unroll
        for (int s = 0; s < K; ++s) key[s] = part[((size_t)l * K + s) * n0 + q];
#pragma unroll
        for (int s = 0; s < K; ++s) {
            const unsigned d = key[s] >> kRowBits;
            unsigned long long x = ((unsigned long long)d << 32) | (row0 + (key[s] & kRowMask));
            if (d < threshold && x < best[K - 1]) {  // (the sentinel and nothing else has d == threshold)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const unsigned long long lo = best[k] < x ? best[k] : x;
                    x = best[k] < x ? x : best[k];
                    best[k] = lo;
                }
            }
        }
    }
    unsigned cnt = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if ((unsigned)k < k_out) {
            const bool live = best[k] != ~0ull;
            akz_match m;
            m.index_0 = q;
            m.index_1 = live ? (best[k] & 0xffffffffull) : ~0ull;
            m.distance = live ? (double)(unsigned)(best[k] >> 32) : __builtin_inf();
            out[(size_t)q * k_out + k] = m;
            cnt += live ? 1u : 0u;
        }
    }
    counts[q] = cnt;
}

template <int K>
void knn_launch(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, uint32_t n1, uint32_t thr, uint32_t chunks, uint32_t k,
                uint32_t* d_part, akz_match* d_out, uint32_t* d_counts) {
    const uint32_t tiles = (n1 + fp4::TR - 1) / fp4::TR;
    if (n1) hipLaunchKernelGGL((k_knn_fp4<K>), dim3((n0 + fp4::QB - 1) / fp4::QB, chunks), dim3(fp4::NT), 0, s, q4, n0, t4, n1, thr, d_part);
    hipLaunchKernelGGL((k_knn_merge<K>), dim3((n0 + 255) / 256), dim3(256), 0, s, d_part, n0, n1 ? chunks : 0u, tiles, thr, k, d_out, d_counts);
}

}  // namespace

namespace launch {

uint32_t knn_list_len(uint32_t k) { return k <= 1 ? 1u : k <= 2 ? 2u : k <= 4 ? 4u : 8u; }
uint32_t knn_chunks(uint32_t n0, uint32_t n1, uint32_t forced) {
    const uint32_t tiles = (std::max<uint32_t>(n1, 1) + fp4::TR - 1) / fp4::TR;
    const uint32_t most = (1u << kRowBits) / fp4::TR;  // tiles of a chunk whose rows fit a key
    return std::max(match_mfma_chunks(n0, n1, forced), (tiles + most - 1) / most);
}
size_t knn_part_bytes(uint32_t n0, uint32_t chunks, uint32_t k) { return (size_t)2 * chunks * knn_list_len(k) * std::max<uint32_t>(n0, 1) * sizeof(uint32_t); }
bool knn(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, uint32_t n1, uint32_t threshold, uint32_t chunks, uint32_t k,
         uint32_t* d_part, akz_match* d_out, uint32_t* d_counts) {
    if (k == 0 || k > 8 || chunks == 0) return false;
    if (n0 == 0) return true;
    const uint32_t thr = std::min<uint32_t>(threshold, (uint32_t)fp4::kBits + 1u);
    switch (knn_list_len(k)) {
        case 1: knn_launch<1>(s, q4, n0, t4, n1, thr, chunks, k, d_part, d_out, d_counts); break;
        case 2: knn_launch<2>(s, q4, n0, t4, n1, thr, chunks, k, d_part, d_out, d_counts); break;
        case 4: knn_launch<4>(s, q4, n0, t4, n1, thr, chunks, k, d_part, d_out, d_counts); break;
        default: knn_launch<8>(s, q4, n0, t4, n1, thr, chunks, k, d_part, d_out, d_counts); break;
    }
    return true;
}

}  // namespace launch
}  // namespace akz
