// The pose stage of akz_match_features_seeded_pose_pairs: after k_pairs_pick_filter and k_refit have left every pair's model,
// found flag and kept list on the device, k_pairs_pose runs the statement of akz_pose.hpp on the KEPT list -- the same source as
// akz_recover_pose_host, the same bits -- and rewrites the kept list and its count in place.
#include "akz_pose.hpp"
#include "akz_ransac_device.hpp"

namespace akz {
namespace {

using PairJob = launch::PairJobHost;

// Per pair (a workgroup of 256, grid-stride): nothing for a pair without a model (its pose was zeroed by the call).  Thread 0
// decomposes E in LDS (three rows: a lone chain of rotations that four lanes would not shorten) and broadcasts the candidates;
// every thread walks the kept list in strides of 256 with four integer counters, which go through an integer tree in LDS -- no
// float is ever summed across lanes, so the counts are exact whatever the order.  With a winner the list is compacted in place in
// match order: in a step every thread holds its own record before the step's first barrier and writes at or below its own
// place behind it, so no record is overwritten before it is read.  The points, where asked, follow from the compacted list.
__global__ void __launch_bounds__(kGroup) k_pairs_pose(const PairJob* __restrict__ pairs, unsigned n_pairs, const akz_camera* __restrict__ cameras,
                                                       const float* __restrict__ kx, const float* __restrict__ ky, const float* __restrict__ models,
                                                       const int* __restrict__ found, akz_match* keep, unsigned long long* __restrict__ keep_cnt,
                                                       akz_pose* __restrict__ poses, float* __restrict__ points) {
    __shared__ double s_m[3 * 9];
    __shared__ PoseCandidates s_pc;
    __shared__ float s_sigma[3];
    __shared__ int s_ok;
    __shared__ unsigned s_cnt[4 * kGroup];
    __shared__ unsigned s_wsum[kGroup / 64];
    const unsigned tid = threadIdx.x;
    for (unsigned p = blockIdx.x; p < n_pairs; p += gridDim.x) {
        if (found[p] == 0) continue;  // (the same for the whole workgroup)
        const PairJob pj = pairs[p];
        const unsigned long long n = keep_cnt[p];
        const akz_camera k0 = cameras[2 * (size_t)p], k1 = cameras[2 * (size_t)p + 1];
        if (tid == 0) {
            LdsMat m{s_m};
            float f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = models[(size_t)p * 9 + k];
            PoseCandidates pc;
            float sigma[3];
            const bool ok = pose_decompose(m, f, k0, k1, pc, sigma);
            s_ok = ok ? 1 : 0;
            if (ok) s_pc = pc;
#pragma unroll
            for (int k = 0; k < 3; ++k) s_sigma[k] = sigma[k];
        }
        __syncthreads();
        const bool ok = s_ok != 0;
        PoseCandidates pc;
        if (ok) pc = s_pc;
        akz_match* list = keep + pj.keep_off;
        const float *x0 = kx + pj.kp0_off, *y0 = ky + pj.kp0_off, *x1 = kx + pj.kp1_off, *y1 = ky + pj.kp1_off;
        unsigned cnt[4] = {0u, 0u, 0u, 0u};
        if (ok)
            for (unsigned long long i = tid; i < n; i += kGroup) {
                const akz_match mt = list[i];
                double a[3], b[3];
                pose_rays(x0[mt.index_0], y0[mt.index_0], x1[mt.index_1], y1[mt.index_1], k0, k1, a, b);
                const unsigned bits = pose_front(pc, a, b);
#pragma unroll
                for (int k = 0; k < 4; ++k) cnt[k] += (bits >> k) & 1u;
            }
#pragma unroll
        for (int k = 0; k < 4; ++k) s_cnt[k * kGroup + tid] = cnt[k];
        __syncthreads();
        for (unsigned s = kGroup / 2; s > 0; s >>= 1) {
            if (tid < s) {
#pragma unroll
                for (int k = 0; k < 4; ++k) s_cnt[k * kGroup + tid] += s_cnt[k * kGroup + tid + s];
            }
            __syncthreads();
        }
        const uint32_t in_front[4] = {s_cnt[0], s_cnt[kGroup], s_cnt[2 * kGroup], s_cnt[3 * kGroup]};
        uint32_t winner = 0;
        const bool posed = ok && pose_winner(in_front, winner);
        if (tid == 0) {
            const float sigma[3] = {s_sigma[0], s_sigma[1], s_sigma[2]};
            akz_pose res;
            pose_result(ok, pc, sigma, in_front, res);
            poses[p] = res;
        }
        if (posed) {
            unsigned long long written = 0;
            for (unsigned long long base = 0; base < n; base += kGroup) {
                const unsigned long long i = base + tid;
                akz_match mt = {0, 0, 0.0};
                bool kept = false;
                if (i < n) {
                    mt = list[i];
                    double a[3], b[3];
                    pose_rays(x0[mt.index_0], y0[mt.index_0], x1[mt.index_1], y1[mt.index_1], k0, k1, a, b);
                    kept = ((pose_front(pc, a, b) >> winner) & 1u) != 0u;
                }
                compact_kept(kept, &mt, list, written, s_wsum, tid);
            }
            if (tid == 0) keep_cnt[p] = written;
            if (points) {  // (compact_kept ends on a barrier: the workgroup's stores to the list are visible to it)
                double r[9], ts[3];
                pose_of_candidate(pc, winner, r, ts);
                float* out = points + 3 * pj.keep_off;
                for (unsigned long long i = tid; i < written; i += kGroup) {
                    const akz_match mt = list[i];
                    double a[3], b[3];
                    float x[3];
                    pose_rays(x0[mt.index_0], y0[mt.index_0], x1[mt.index_1], y1[mt.index_1], k0, k1, a, b);
                    pose_point(r, ts, a, b, x);
                    out[3 * i] = x[0];
                    out[3 * i + 1] = x[1];
                    out[3 * i + 2] = x[2];
                }
            }
        }
        __syncthreads();  // (s_ok, s_pc, s_cnt: the next pair's)
    }
}

}  // namespace

namespace launch {
void pairs_pose(hipStream_t s, const PairJobHost* d_pairs, uint32_t n_pairs, const akz_camera* d_cameras, const float* d_kx, const float* d_ky,
                const float* d_f, const int32_t* d_found, void* d_keep, uint64_t* d_keep_cnt, akz_pose* d_poses, float* d_points) {
    if (n_pairs == 0) return;
    hipLaunchKernelGGL(k_pairs_pose, dim3(std::min<uint32_t>(n_pairs, 8192)), dim3(kGroup), 0, s, d_pairs, n_pairs, d_cameras, d_kx, d_ky, d_f, d_found,
                       (akz_match*)d_keep, (unsigned long long*)d_keep_cnt, d_poses, d_points);
}
}  // namespace launch
}  // namespace akz
