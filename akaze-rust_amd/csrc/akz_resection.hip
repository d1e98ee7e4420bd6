// The seeded resection RANSAC on the GPU (akz_resection_seeded_problems; the statement: akz_resection.hpp, included here as the
// host includes it -- the same source, the same bits).  The round kernel has the shape of k_seeded_round (akz_ransac_kernels.hip)
// over problems of five planes X | Y | Z | u | v and models of 15 floats; k_seeded_update<15> follows it: the winner and the stopping
// rule of every model of the family.  The refit is refit_loop<ResectionRefit> of akz_ransac_device.hpp, the loop of every model.
//   k_resection_round<NW>   a round of 128 trials of every problem that still runs
//   k_resection_finish      per problem: found, the refit loop, the kept indices, the pose
#include "akz_ransac_device.hpp"
#include "akz_ransac_seeded.hpp"
#include "akz_resection.hpp"

namespace akz {
namespace {

using ResJob = launch::ResJobHost;
using ResMat = LdsMatT<kResRows>;

constexpr int MF = kResModelFloats;
constexpr int TPW = 16;  // trials per wave
constexpr int TW = 64;
constexpr unsigned WPR = AKZ_RANSAC_ROUND / TPW;  // workgroups per problem and round

struct Planes {
    const float *X, *Y, *Z, *u, *v;
};
__device__ inline Planes planes_of(const float* planes, unsigned long long stride, unsigned long long off) {
    const float* X = planes + off;
    return Planes{X, X + stride, X + 2 * stride, X + 3 * stride, X + 4 * stride};
}

// The four lanes of a trial form its sums as FundamentalNormalisedDev::rows does: lane j takes elements j and j + 4 of the sample
// (sum8_part; lanes 2 and 3 have no second element: + 0.0, as resection_from_6 has it) and quad_join leaves the host's bits on all
// four, so centroids and scales agree without an exchange through memory.  Lane 0 writes M.  side: c[0 .. 4], s2, s3.
__device__ __forceinline__ bool trial_rows(ResMat m, double* side, int sub, const unsigned* smp, const Planes& pl, const ResCamera& cam) {
    const bool two = sub < 2;
    const unsigned ja = smp[sub], jb = smp[two ? sub + 4 : sub];
    const float aX = pl.X[ja], aY = pl.Y[ja], aZ = pl.Z[ja], au = pl.u[ja], av = pl.v[ja];
    const float bX = pl.X[jb], bY = pl.Y[jb], bZ = pl.Z[jb], bu = pl.u[jb], bv = pl.v[jb];
    double c[kResSums1];
    {
        double a[kResSums1], b[kResSums1];
        res_terms1(aX, aY, aZ, au, av, cam, a);
        res_terms1(bX, bY, bZ, bu, bv, cam, b);
#pragma unroll
        for (int k = 0; k < kResSums1; ++k) c[k] = sum8_part(a[k], two ? b[k] : 0.0);
        quad_join(c);
#pragma unroll
        for (int k = 0; k < kResSums1; ++k) c[k] = c[k] / 6.0;
    }
    double s2 = 0.0, s3 = 0.0;
    {
        double a[2], b[2], d[2];
        res_terms2(aX, aY, aZ, au, av, cam, c, a);
        res_terms2(bX, bY, bZ, bu, bv, cam, c, b);
        d[0] = sum8_part(a[0], two ? b[0] : 0.0);
        d[1] = sum8_part(a[1], two ? b[1] : 0.0);
        quad_join(d);
        if (!refit_scale(d[0], 6.0, s2) || !res_scale3(d[1], 6.0, s3)) return false;  // (the same bits on all four lanes)
    }
    double sums[kResSums3];
    {
        double b[kResSums3];
        res_terms3(aX, aY, aZ, au, av, cam, c, s2, s3, sums);
        res_terms3(bX, bY, bZ, bu, bv, cam, c, s2, s3, b);
#pragma unroll
        for (int k = 0; k < kResSums3; ++k) sums[k] = sum8_part(sums[k], two ? b[k] : 0.0);
        quad_join(sums);
    }
    if (sub == 0) {
        res_normal_matrix(m, sums);
#pragma unroll
        for (int k = 0; k < kResSums1; ++k) side[k] = c[k];
        side[5] = s2;
        side[6] = s3;
    }
    return true;
}
__device__ inline bool trial_model(ResMat m, const double* side, float epsilon, float (&f)[MF]) {
    const double c[kResSums1] = {side[0], side[1], side[2], side[3], side[4]};
    return res_model_from_rotated(m, 6.0, epsilon, c, side[5], side[6], f);
}

// One round of every problem that still runs, in the shape of k_seeded_round: workgroup 8 p + w has trials 128 round + 16 w .. + 16
// of problem p, FOUR lanes per trial and sixteen trials per wave.  The twelve-row sweep has 21 levels of up to six disjoint
// pairs; four lanes take the five widest levels in two passes (26 rotation slots a sweep for sixteen trials), eight lanes would
// take every level in one (21 slots for eight trials): a wave's rotations cost the same however many lanes rotate, so four lanes
// do 1.6 times the trials per slot, they keep the quad exchange and the ballot masks of the other models, and only a lone
// problem's latency -- 26 against 21 -- pays.  The trial's 12 x 12 f64 matrix is 1 152 B of LDS (18 KiB a workgroup).  Each trial
// draws its own sample (seeded_sample<6>) on its first lane.  Then the whole workgroup counts each of its trials (NW - 1 helper
// waves join when there are few problems; counts are integers: the same for every NW).  Models and counts go to slot
// (trial mod 128) of the problem's ring; no model: the count -1.
template <int NW>
__global__ void __launch_bounds__(TW * NW) k_resection_round(const ResJob* __restrict__ jobs, const unsigned* __restrict__ done,
                                                             unsigned long long k1, unsigned long long stream_base, unsigned round,
                                                             unsigned max_trials, const float* __restrict__ planes, unsigned long long stride,
                                                             float epsilon_model, float epsilon_inlier, float* __restrict__ ring_mdl,
                                                             int* __restrict__ ring_inl) {
    __shared__ double s_m[TPW][kResRows * kResRows];
    __shared__ double s_side[TPW][8];
    __shared__ float s_f[TPW][MF];
    __shared__ unsigned s_smp[TPW][8];
    __shared__ int s_ok[TPW];
    __shared__ int s_cnt[TPW];
    const int tid = (int)threadIdx.x, lane = tid & (TW - 1), tw = lane >> 2, sub = lane & 3;
    const unsigned p = blockIdx.x / WPR, slot0 = (blockIdx.x % WPR) * TPW, t0 = round * AKZ_RANSAC_ROUND + slot0;
    if (done[p] != 0u || t0 >= max_trials) return;  // (the same for the whole workgroup)
    const unsigned here = min((unsigned)TPW, max_trials - t0);  // trials of this workgroup
    const ResJob pj = jobs[p];
    const unsigned n = pj.n;
    const ResCamera cam{pj.fx, pj.fy, pj.cx, pj.cy};
    const Planes pl = planes_of(planes, stride, pj.off);
    float* mdl = ring_mdl + (size_t)p * AKZ_RANSAC_ROUND * MF;
    int* inl = ring_inl + (size_t)p * AKZ_RANSAC_ROUND;
    const unsigned long long ks = seeded_stream_key(k1, stream_base + p);  // (uniform: the problem's stream)
    if (NW == 1 || tid < TW) {  // the models: the first wave
        const bool valid = (unsigned)tw < here;
        ResMat m{s_m[tw]};
        if (valid && sub == 0) {
            unsigned smp[kResK];
            seeded_sample<kResK>(ks, (unsigned long long)t0 + (unsigned)tw, n, smp);
#pragma unroll
            for (int i = 0; i < kResK; ++i) s_smp[tw][i] = smp[i];
        }
        wave_sync();
        bool usable = false;
        if (valid) usable = trial_rows(m, s_side[tw], sub, s_smp[tw], pl, cam);
        wave_sync();
        bool active = usable;
        for (int sweep = 0; sweep < 60; ++sweep) {
            if (__ballot(active) == 0ull) break;
            const bool rotated = jacobi_sweep_levels<kResRows, kResRows>(m, sub, active);
            if (((__ballot(rotated) >> (4 * tw)) & 0xfull) == 0ull) active = false;  // this trial's first sweep without a rotation
        }
        if (valid && sub == 0) {
            float f[MF];
            const bool ok = usable && trial_model(m, s_side[tw], epsilon_model, f);
            const unsigned slot = slot0 + (unsigned)tw;
            s_ok[tw] = ok ? 1 : 0;
            if (NW > 1) s_cnt[tw] = 0;
            if (ok) {
#pragma unroll
                for (int k = 0; k < MF; ++k) {
                    s_f[tw][k] = f[k];
                    mdl[slot * MF + k] = f[k];
                }
            } else {
                inl[slot] = -1;
            }
        }
    }
    if (NW == 1) wave_sync();
    else __syncthreads();
    for (unsigned u = 0; u < here; ++u) {
        if (!s_ok[u]) continue;
        float f[MF];
#pragma unroll
        for (int k = 0; k < MF; ++k) f[k] = s_f[u][k];
        int cnt = 0;
        for (unsigned i = (unsigned)tid; i < n; i += TW * NW)
            cnt += res_inlier(f, cam, pl.X[i], pl.Y[i], pl.Z[i], pl.u[i], pl.v[i], epsilon_inlier) ? 1 : 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        if (NW == 1) {
            if (lane == 0) inl[slot0 + u] = cnt;
        } else if (lane == 0) {
            atomicAdd(&s_cnt[u], cnt);
        }
    }
    if (NW > 1) {
        __syncthreads();
        if ((unsigned)tid < here && s_ok[tid]) inl[slot0 + (unsigned)tid] = s_cnt[tid];
    }
}

// one problem's correspondences, camera and count (the view of ResectionRefit), and the table that yields it
struct ResView : Planes {
    ResCamera cam;
    unsigned n;
};
struct ResTable {
    const ResJob* jobs;
    const float* planes;
    unsigned long long stride;
    __device__ ResView view(unsigned p) const {
        const ResJob pj = jobs[p];
        return ResView{planes_of(planes, stride, pj.off), ResCamera{pj.fx, pj.fy, pj.cx, pj.cy}, pj.n};
    }
};

// After the last round, per problem (a workgroup of 256, grid-stride): found = its best count > 0; with a winner and
// max_iterations > 0 refit_loop<ResectionRefit> (lane sums of 5, 2, then 40); then the kept indices under the final model compacted
// in order, their count, the accepted fits and the pose.  found = 0: no index, a pose of zeros.
__global__ void __launch_bounds__(kGroup) k_resection_finish(ResTable table, unsigned n_problems, const float* __restrict__ best_mdl,
                                                             const int* __restrict__ best_inl, float epsilon_model, float epsilon_inlier,
                                                             unsigned max_iterations, unsigned* __restrict__ kept_out,
                                                             unsigned* __restrict__ n_kept, unsigned* __restrict__ fits,
                                                             akz_resection* __restrict__ poses) {
    static_assert(sizeof(akz_resection) == (MF + 1) * 4, "r | t | sigma | found");
    __shared__ unsigned s_wsum[kGroup / 64];
    const unsigned tid = threadIdx.x;
    for (unsigned p = blockIdx.x; p < n_problems; p += gridDim.x) {
        const ResView q = table.view(p);
        const bool found = best_inl[p] > 0;  // (the same for the whole workgroup)
        float h[MF];
#pragma unroll
        for (int k = 0; k < MF; ++k) h[k] = found ? best_mdl[(size_t)p * MF + k] : 0.0f;
        unsigned done = 0;
        if (found && max_iterations > 0) done = refit_loop<ResectionRefit>(q, h, epsilon_model, epsilon_inlier, max_iterations, s_wsum, tid);
        const unsigned long long off = table.jobs[p].off;
        unsigned long long written = 0;
        if (found)
            for (unsigned base = 0; base < q.n; base += kGroup) {
                const unsigned i = base + tid;
                const bool kept = i < q.n && ResectionRefit::inlier(h, q, i, epsilon_inlier);
                const unsigned long long at = compact_slot(kept, written, s_wsum, tid);
                if (kept) kept_out[off + at] = i;
            }
        if (tid == 0) {
            n_kept[p] = (unsigned)written;
            fits[p] = done;
            akz_resection out;
#pragma unroll
            for (int k = 0; k < 9; ++k) out.r[k] = h[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                out.t[k] = h[9 + k];
                out.sigma[k] = h[12 + k];
            }
            out.found = found ? 1 : 0;
            poses[p] = out;
        }
        __syncthreads();  // (refit_loop's LDS, s_wsum: the next problem's)
    }
}

}  // namespace

namespace launch {
void resection_round(hipStream_t s, const ResJobHost* d_jobs, uint32_t n_problems, const uint32_t* d_done, uint64_t k1, uint64_t stream_base,
                     uint32_t round, uint32_t max_trials, const float* d_planes, uint64_t stride, float epsilon_model, float epsilon_inlier,
                     float* d_ring_mdl, int32_t* d_ring_inl) {
    if (n_problems == 0) return;
    // helper waves below 64 problems (512 workgroups: half the chip's SIMDs), as seeded_round has them
    const uint32_t blocks = n_problems * WPR;
    const bool helpers = blocks < 512;
    auto k = helpers ? k_resection_round<4> : k_resection_round<1>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(TW * (helpers ? 4 : 1)), 0, s, d_jobs, d_done, (unsigned long long)k1, (unsigned long long)stream_base,
                       round, max_trials, d_planes, (unsigned long long)stride, epsilon_model, epsilon_inlier, d_ring_mdl, d_ring_inl);
}
void resection_finish(hipStream_t s, const ResJobHost* d_jobs, uint32_t n_problems, const float* d_planes, uint64_t stride,
                      const float* d_best_mdl, const int32_t* d_best_inl, float epsilon_model, float epsilon_inlier, uint32_t max_iterations,
                      uint32_t* d_kept, uint32_t* d_n_kept, uint32_t* d_fits, akz_resection* d_poses) {
    if (n_problems == 0) return;
    hipLaunchKernelGGL(k_resection_finish, dim3(std::min<uint32_t>(n_problems, 8192)), dim3(kGroup), 0, s, ResTable{d_jobs, d_planes, stride},
                       n_problems, d_best_mdl, d_best_inl, epsilon_model, epsilon_inlier, max_iterations, d_kept, d_n_kept, d_fits, d_poses);
}
}  // namespace launch
}  // namespace akz
