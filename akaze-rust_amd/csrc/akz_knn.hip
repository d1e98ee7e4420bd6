// k-nearest-neighbour descriptor matching on the matrix cores (include/akaze_hip.h: knn(A, B, k, threshold); akz_knn_api.cpp;
// DESIGN.md 8):
//   k_knn_fp4<K>     per workgroup 512 queries against one chunk of the train set: every lane's K smallest keys
//   k_knn_merge<K>   per query the k smallest keys over all partial lists -> records, padding slots and counts
//
// The scan is the one-direction form of k_match_fp4 (akz_match.hip) with the top-2 state replaced by a sorted list: operands
// are the FP4 +-1 images of launch::unpack_pair(fp4) -- 256 bytes per row, <a', b'> = 488 - 2 hamming(a, b), exact in the f32
// accumulators --, 1024 threads = 16 waves, a wave owns 32 queries as the resident B operand, the workgroup walks its chunk
// in LDS tiles of 128 train rows, two tiles per barrier.  The 32 x 32 result has its column (query) on the lane and rows
// (i & 3) + 8 (i >> 2) + 4 h (h = lane >> 5) in register i: ascending train index inside a lane.
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

#include "akz_internal.hpp"

namespace akz {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int KN_NT = 1024;               // threads per workgroup: 16 waves of 32 queries
constexpr int KN_QB = (KN_NT / 64) * 32;  // queries per workgroup
constexpr int KN_SUB = 4;                 // 32-row matrix tiles per LDS tile
constexpr int KN_TR = 32 * KN_SUB;        // train rows per LDS tile (= launch::match_mfma_tile_rows(), checked at launch)
constexpr int KN_ROW = 256;               // bytes per unpacked row
constexpr int KN_PITCH = KN_ROW + 16;     // LDS row pitch: the 16-byte operand reads of 16 consecutive rows fall into different banks
constexpr int KN_STEP = 2;                // tiles per barrier
constexpr int kBits = 488;                // columns that carry +-1 (61 bytes)
constexpr float kPadAcc = -1.0e30f;       // accumulator given to the padding rows of a partial tile (a real one is >= -488)
constexpr unsigned kRowBits = 22;         // key = d << kRowBits | row inside the chunk
constexpr unsigned kRowMask = (1u << kRowBits) - 1u;

// first tile of chunk c of `chunks` over `tiles` tiles: balanced, no chunk empty while chunks <= tiles
__host__ __device__ inline unsigned knn_chunk_tile(unsigned c, unsigned chunks, unsigned tiles) {
    return (unsigned)((unsigned long long)c * tiles / chunks);
}

// blockIdx.x: 512 queries; blockIdx.y: a chunk of the train tiles.  q4 / t4: the FP4 images, rows padded to whole workgroups /
// whole tiles with zero rows; threshold <= 489.
template <int K>
__global__ void __launch_bounds__(KN_NT) k_knn_fp4(const uint8_t* __restrict__ q4, unsigned n0, const uint8_t* __restrict__ t4, unsigned n1,
                                                   unsigned threshold, unsigned* __restrict__ part) {
    constexpr int SUBS = KN_SUB * KN_STEP;
    __shared__ __attribute__((aligned(16))) uint8_t s_tile[2][KN_STEP * KN_TR * KN_PITCH];
    const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const unsigned r = lane & 31u, h = lane >> 5;
    const unsigned q_first = blockIdx.x * KN_QB + wave * 32u;
    auto op = [](v4i x) { return v8i{x.x, x.y, x.z, x.w, 0, 0, 0, 0}; };  // FP4 operands occupy the first four registers

    v4i bq[8];  // B operands: the wave's queries, eight K-steps of 64 columns, resident for the whole chunk
    {
        const uint8_t* row = q4 + (size_t)(q_first + r) * KN_ROW + 16 * h;
#pragma unroll
        for (int s = 0; s < 8; ++s) bq[s] = *reinterpret_cast<const v4i*>(row + 32 * s);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" : "+v"(bq[s]));  // (the waits for these loads stay out of the tile loop)
    unsigned list[K];
#pragma unroll
    for (int k = 0; k < K; ++k) list[k] = threshold << kRowBits;
    float limf = (float)(kBits - 2 * (int)threshold);  // accumulator of the worst kept distance: only rows ABOVE it enter

    const unsigned tiles_total = (n1 + KN_TR - 1) / KN_TR;
    const unsigned t_begin = knn_chunk_tile(blockIdx.y, gridDim.y, tiles_total), t_end = knn_chunk_tile(blockIdx.y + 1, gridDim.y, tiles_total);
    // staging: the next step's tiles arrive in 64-row parts (1024 sixteen-byte pieces, one per thread) through one register
    // stage: part p requested before chain 2 p, handed to the other LDS buffer after chain 2 p + 1 has been issued
    const unsigned st_src = (tid >> 4) * KN_ROW + (tid & 15u) * 16u, st_dst = (tid >> 4) * KN_PITCH + (tid & 15u) * 16u;
    uint4 stage;
    auto fetch = [&](unsigned tile, int p) { stage = *reinterpret_cast<const uint4*>(t4 + ((size_t)tile * KN_TR + 64u * p) * KN_ROW + st_src); };
    auto commit = [&](int buf, int p) { *reinterpret_cast<uint4*>(&s_tile[buf][64 * p * KN_PITCH + st_dst]) = stage; };
    if (t_begin < t_end) {
#pragma unroll
        for (int p = 0; p < 2 * KN_STEP; ++p) {
            if (p < 2 * (int)min((unsigned)KN_STEP, t_end - t_begin)) {
                fetch(t_begin, p);
                commit(0, p);
            }
        }
    }
    __syncthreads();
    for (unsigned tile = t_begin; tile < t_end; tile += KN_STEP) {
        const int buf = (int)(((tile - t_begin) / KN_STEP) & 1u);
        const unsigned to = tile + KN_STEP;                                            // the step staged during this one
        const unsigned here = min((unsigned)KN_STEP, t_end - tile);                    // tiles of this step
        const unsigned next = to < t_end ? min((unsigned)KN_STEP, t_end - to) : 0u;    // ... and of the one being staged
#pragma unroll
        for (int sub = 0; sub < SUBS; ++sub) {
            if (sub >= KN_SUB && (unsigned)sub >= KN_SUB * here) break;  // (uniform: the last step of a chunk may be short)
            const bool more = (unsigned)(sub >> 1) < 2u * next;          // part sub / 2 of the next step exists
            const bool partial = (tile + (sub / KN_SUB) + 1) * KN_TR > n1;  // uniform: only the last tile of the set
            if (more && (sub & 1) == 0) fetch(to, sub >> 1);  // in flight under the two chains below
            v16f acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
            const uint8_t* arow = &s_tile[buf][(32 * sub + r) * KN_PITCH + 16 * h];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const v4i a = *reinterpret_cast<const v4i*>(arow + 32 * s);
                acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(op(a), op(bq[s]), acc, 4, 4, 0, 127, 0, 127);
            }
            // three operand reads in flight ahead of the matrix instructions that consume them (as in k_match_fp4)
            __builtin_amdgcn_sched_group_barrier(0x100, 3, 0);
#pragma unroll
            for (int s = 0; s < 8 - 3; ++s) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 3, 0);
            if ((sub & 1) == 1 && more) commit(buf ^ 1, sub >> 1);  // before the accumulators are looked at
            const unsigned j0 = tile * KN_TR + 32 * sub + 4 * h;     // the lane's first row of the sub-tile
            if (partial) {  // padding rows never match
#pragma unroll
                for (int i = 0; i < 16; ++i)
                    if (j0 + (unsigned)((i & 3) + 8 * (i >> 2)) >= n1) acc[i] = kPadAcc;
            }
            float topf = acc[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) topf = fmaxf(topf, acc[i]);
            if (topf > limf) {  // one of the lane's 16 rows is nearer than its worst kept one
                const unsigned jb = j0 - t_begin * KN_TR;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    if (acc[i] > limf) {
                        unsigned x = ((unsigned)((kBits - (int)acc[i]) >> 1) << kRowBits) | (jb + (unsigned)((i & 3) + 8 * (i >> 2)));
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            const unsigned lo = min(list[k], x);
                            x = max(list[k], x);
                            list[k] = lo;
                        }
                        limf = (float)(kBits - 2 * (int)(list[K - 1] >> kRowBits));
                    }
                }
            }
        }
        __syncthreads();
    }
    const unsigned q = q_first + r;
    if (q < n0) {
#pragma unroll
        for (int k = 0; k < K; ++k) part[((size_t)(blockIdx.y * 2u + h) * K + k) * n0 + q] = list[k];
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
        const unsigned long long row0 = (unsigned long long)knn_chunk_tile(l >> 1, chunks, tiles) * KN_TR;
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
    const uint32_t tiles = (n1 + KN_TR - 1) / KN_TR;
    if (n1) hipLaunchKernelGGL((k_knn_fp4<K>), dim3((n0 + KN_QB - 1) / KN_QB, chunks), dim3(KN_NT), 0, s, q4, n0, t4, n1, thr, d_part);
    hipLaunchKernelGGL((k_knn_merge<K>), dim3((n0 + 255) / 256), dim3(256), 0, s, d_part, n0, n1 ? chunks : 0u, tiles, thr, k, d_out, d_counts);
}

}  // namespace

namespace launch {

uint32_t knn_list_len(uint32_t k) { return k <= 1 ? 1u : k <= 2 ? 2u : k <= 4 ? 4u : 8u; }
uint32_t knn_chunks(uint32_t n0, uint32_t n1, uint32_t forced) {
    const uint32_t tiles = (std::max<uint32_t>(n1, 1) + KN_TR - 1) / KN_TR;
    const uint32_t most = (1u << kRowBits) / KN_TR;  // tiles of a chunk whose rows fit a key
    return std::max(match_mfma_chunks(n0, n1, forced), (tiles + most - 1) / most);
}
size_t knn_part_bytes(uint32_t n0, uint32_t chunks, uint32_t k) { return (size_t)2 * chunks * knn_list_len(k) * std::max<uint32_t>(n0, 1) * sizeof(uint32_t); }
bool knn(hipStream_t s, const uint8_t* q4, uint32_t n0, const uint8_t* t4, uint32_t n1, uint32_t threshold, uint32_t chunks, uint32_t k,
         uint32_t* d_part, akz_match* d_out, uint32_t* d_counts) {
    if (match_mfma_tile_rows() != (uint32_t)KN_TR || match_mfma_query_block() != (uint32_t)KN_QB || k == 0 || k > 8 || chunks == 0) return false;
    if (n0 == 0) return true;
    const uint32_t thr = std::min<uint32_t>(threshold, (uint32_t)kBits + 1u);
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
