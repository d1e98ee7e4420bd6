// Guided matching: the Hamming scan of descriptor_match (feature_matching.rs:37-81) in which a train row competes for a
// query only if it lies within `radius` pixels of where a known model sends that query -- the transferred point of a
// homography (kind 0: transfer_disc / transfer_near, i.e. homography_inlier, akz_homography.hpp) or the epipolar line of a
// fundamental matrix (kind 1: epipolar_line / epipolar_near, akz_fmatrix.hpp).  Minimum, second minimum and the lowest row
// among equal minima are those of the gated rows only.
//
// GATE FIRST, then popcount the survivors.  The gate is selective -- a 3-pixel band around an epipolar line keeps about
// 1 % of a 1080p frame's keypoints, a 3-pixel disc a few rows out of thousands -- so nearly all of the distances a
// matrix-core scan would form are thrown away, and the gate itself (7 vector operations per element for a line, 9 for a
// disc) costs about as much per element as that scan's whole share of a matrix instruction.  So: one query per lane (its 64
// descriptor bytes in 16 registers, its four gate constants in 4), the train rows of a chunk staged through LDS 256 at a
// time with their x | y beside them; a lane evaluates the gate on the row's coordinates (one LDS broadcast read) and only
// where some lane of the wave passes does the wave read the row's 64 bytes (four broadcast reads) and count bits.  All 64
// bytes are compared (rows shorter than that arrive zero-padded), so 62..64-byte descriptors need no second form.
// A lane walks its rows in ascending order: the reference's strict '<' update applies as it stands.  Records, chunking and
// the merge / compaction are those of k_match (akz_kernels.hip): a row that fails the gate is a row that is not there.
//
// One launch serves many pairs: workgroup -> (pair, block of 256 queries, chunk of the pair's train rows) through a
// per-pair table; the models are read from device memory (9 floats per pair), so a composite call feeds them from its
// pick / filter kernel without a host round trip, and `found` (optional) switches pairs without a model off.
#include <hip/hip_runtime.h>

#include "akz_homography.hpp"
#include "akz_internal.hpp"
#include "akz_match_rule.hpp"

namespace akz {
namespace {

constexpr int GT = 256;  // threads per workgroup = queries per block = train rows per LDS tile

struct GuidedPair {  // = launch::GuidedPairHost
    unsigned long long rec_off;  // first record of the pair: rec[rec_off + chunk * n0 + query]
    unsigned q_row0, n0;         // the query set: first row of the uploaded block, rows
    unsigned t_row0, n1;         // the train set
    unsigned wg0;                // first workgroup of the pair (ascending; pairs without rows are not in the table)
    unsigned chunks, chunk_rows, model;  // model: index into models / found
};

template <int KIND>
struct Gate;
template <>
struct Gate<0> {
    TransferDisc t;
    __device__ __forceinline__ Gate(const float (&m)[9], float x0, float y0, float radius) : t(transfer_disc(m, x0, y0, radius)) {}
    __device__ __forceinline__ bool pass(float x1, float y1) const { return transfer_near(t, x1, y1); }
};
template <>
struct Gate<1> {
    EpipolarLine e;
    __device__ __forceinline__ Gate(const float (&m)[9], float x0, float y0, float radius) : e(epipolar_line(m, x0, y0, radius)) {}
    __device__ __forceinline__ bool pass(float x1, float y1) const { return epipolar_near(e, x1, y1); }
};

template <int KIND>
__global__ void __launch_bounds__(GT) k_match_guided(const uint4* __restrict__ rows, const float* __restrict__ kx,
                                                     const float* __restrict__ ky, const GuidedPair* __restrict__ tab,
                                                     unsigned n_tab, const float* __restrict__ models,
                                                     const int* __restrict__ found, float radius, unsigned threshold,
                                                     MatchRec* __restrict__ out) {
    __shared__ uint4 s_tile[GT * 4];
    __shared__ float2 s_xy[GT];
    // the pair of this workgroup: the last table entry that starts at or before it (uniform)
    unsigned lo = 0, hi = n_tab - 1;
    while (lo < hi) {
        const unsigned mid = (lo + hi + 1) >> 1;
        if (tab[mid].wg0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const GuidedPair gp = tab[lo];
    const unsigned local = blockIdx.x - gp.wg0, qb = local / gp.chunks, ch = local - qb * gp.chunks;
    const unsigned i = qb * GT + threadIdx.x;
    const bool live = i < gp.n0;
    const size_t qrow = (size_t)gp.q_row0 + (live ? i : gp.n0 - 1);  // (n0 >= 1 for every table entry)
    uint4 q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = rows[qrow * 4 + k];
    float m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = models[(size_t)gp.model * 9 + k];
    const Gate<KIND> gate(m, kx[qrow], ky[qrow], radius);
    const bool on = found == nullptr || found[gp.model] != 0;  // (uniform) a pair without a model: records of an empty scan
    NearestTwo best = NearestTwo::start(threshold);
    const unsigned begin = on ? min(gp.n1, ch * gp.chunk_rows) : gp.n1, end = min(gp.n1, begin + gp.chunk_rows);
    auto feed = [&](unsigned r, unsigned base) {  // a row inside the gate: its distance, then the reference's update rule
        unsigned d = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 t = s_tile[r * 4 + k];
            d += __popc(q[k].x ^ t.x);
            d += __popc(q[k].y ^ t.y);
            d += __popc(q[k].z ^ t.z);
            d += __popc(q[k].w ^ t.w);
        }
        best.feed(d, base + r);
    };
    for (unsigned base = begin; base < end; base += GT) {
        const unsigned nrows = min((unsigned)GT, end - base);
        __syncthreads();
        for (unsigned e = threadIdx.x; e < nrows * 4; e += GT) s_tile[e] = rows[((size_t)gp.t_row0 + base) * 4 + e];
        if (threadIdx.x < nrows) s_xy[threadIdx.x] = make_float2(kx[(size_t)gp.t_row0 + base + threadIdx.x], ky[(size_t)gp.t_row0 + base + threadIdx.x]);
        __syncthreads();
        // four rows' coordinates and gates at a time (independent LDS reads and compares), then the survivors in row order
        unsigned r = 0;
        for (; r + 4 <= nrows; r += 4) {
            bool pass[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float2 p = s_xy[r + k];
                pass[k] = gate.pass(p.x, p.y);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (pass[k]) feed(r + k, base);
        }
        for (; r < nrows; ++r) {
            const float2 p = s_xy[r];
            if (gate.pass(p.x, p.y)) feed(r, base);
        }
    }
    if (live) out[gp.rec_off + (size_t)ch * gp.n0 + i] = best.record();
}

}  // namespace

namespace launch {

static_assert(sizeof(GuidedPairHost) == sizeof(GuidedPair), "the device reads the host's pair records");

uint32_t match_guided_block() { return GT; }
void match_guided(hipStream_t s, int kind, const uint8_t* d_rows, const float* d_kx, const float* d_ky, const GuidedPairHost* d_tab,
                  uint32_t n_tab, uint32_t n_workgroups, const float* d_models, const int32_t* d_found, float radius,
                  uint32_t threshold, MatchRec* d_rec) {
    if (n_tab == 0 || n_workgroups == 0) return;
    const uint4* rows = reinterpret_cast<const uint4*>(d_rows);
    const GuidedPair* tab = reinterpret_cast<const GuidedPair*>(d_tab);
    if (kind == 0)
        hipLaunchKernelGGL(k_match_guided<0>, dim3(n_workgroups), dim3(GT), 0, s, rows, d_kx, d_ky, tab, n_tab, d_models, d_found, radius,
                           threshold, d_rec);
    else
        hipLaunchKernelGGL(k_match_guided<1>, dim3(n_workgroups), dim3(GT), 0, s, rows, d_kx, d_ky, tab, n_tab, d_models, d_found, radius,
                           threshold, d_rec);
}

}  // namespace launch
}  // namespace akz
