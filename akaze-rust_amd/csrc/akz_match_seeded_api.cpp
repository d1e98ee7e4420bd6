// akz_match_features_seeded_pairs and, with the cross-check in front, akz_match_features_seeded_cross_pairs (additions;
// include/akaze_hip.h): match_features over many pairs with the seeded
// RANSAC of akz_ransac_seeded.hpp -- the trial kernel draws its own samples, the stopping rule runs per pair on the device, and
// the calling thread's random source is never touched.  The call is pairs_front and pairs_tail (akz_match_api.cpp) around what is its
// own: the host's table need[pair][round of the window] (seeded_need, the one function the host statement calls too),
// filled and uploaded one window at a time -- its cost follows the rounds that are launched, not max_trials --; rounds of
// launch::seeded_round + launch::seeded_update, enqueued without a host synchronisation in windows of kWindow rounds -- after a window the host reads the count of pairs still running and stops launching at 0, which cannot change
// a result: a round of a finished pair leaves at once.  The tail picks over the pairs' best slots as one trial per pair, and the
// head of its read-back also carries trials_run.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "akz_ctx.hpp"
#include "akz_ransac_seeded.hpp"

namespace akz {
int seeded_refuse_options(const char* name, const akz_ransac_options* opt);  // akz_ransac_seeded.cpp
}
using namespace akz;

// cross: every pair's raw list is cross(A, B) (akz_match_features_seeded_cross_pairs, akz_cross_api.cpp) -- pairs_scans also
// writes the opposite direction and launch::pairs_cross_filter rewrites d_raw / d_cnt before anything reads them; clear, the call
// enqueues what it always did.  pose: akz_match_features_seeded_pose_pairs (akz_pose_api.cpp, which has refused what that call refuses) --
// the pairs' cameras ride behind done | need, the head carries the poses (zeroed with the fits and the trial counts) and the points, and
// the tail runs launch::pairs_pose; null, nothing of it is allocated or enqueued.  q.bank: the sets lie in a feature bank (akz_bank_api.cpp) --
// the front opens on its block and uploads no set; everything else is the same code over the same table.
int match_seeded_pairs_impl(const PairsCall& q, bool cross, const akz_ransac_options* options, float* model, int* found, uint32_t* iterations,
                            uint64_t* trials_run, const SeededPose* pose) {
    constexpr uint32_t kWindow = 8;  // rounds enqueued between two looks at the pairs still running
    const char* name = q.name;
    akz_ctx* c = q.c;
    const uint64_t n_pairs = q.n_pairs;
    AKZ_TRY(seeded_refuse_options(name, options));
    const akz_ransac_options& opt = *options;
    if (opt.guided && !(opt.guided_radius >= 0.0f && std::isfinite(opt.guided_radius))) {
        set_error(std::string(name) + "guided_radius must be finite and >= 0");
        return AKZ_ERR_INVALID_ARG;
    }
    if (n_pairs >= (1ull << 28)) {  // (a round is 8 workgroups per pair in one launch)
        set_error(std::string(name) + "n_pairs must be < 1 << 28");
        return AKZ_ERR_INVALID_ARG;
    }
    if (n_pairs == 0) return AKZ_OK;
    // (the normalised kind: a fundamental matrix too -- K = 8, the refit's rank rule for both stages, the epipolar band when guiding)
    const bool normalised = opt.model_kind == AKZ_RANSAC_FUNDAMENTAL_NORMALISED;
    const bool fundamental = opt.model_kind == AKZ_GUIDED_FUNDAMENTAL || normalised;
    const launch::RansacModel kind = normalised    ? launch::RansacModel::FundamentalNormalised
                                     : fundamental ? launch::RansacModel::Fundamental
                                                   : launch::RansacModel::Homography;
    const int guided_kind = fundamental ? AKZ_GUIDED_FUNDAMENTAL : AKZ_GUIDED_HOMOGRAPHY;
    const uint64_t K = fundamental ? 8 : 4;
    const float epsilon_model = normalised ? AKZ_FUNDAMENTAL_REFIT_EPSILON : fundamental ? 0.05f : AKZ_HOMOGRAPHY_EPSILON_MODEL;
    const float refit_epsilon = fundamental ? AKZ_FUNDAMENTAL_REFIT_EPSILON : AKZ_HOMOGRAPHY_EPSILON_MODEL;
    const uint32_t max_trials = (uint32_t)opt.max_trials, n_rounds = (max_trials + AKZ_RANSAC_ROUND - 1) / AKZ_RANSAC_ROUND;
    const bool stopping = opt.confidence > 0.0;
    const size_t b_done = up256((size_t)n_pairs * 4);
    const size_t b_need = stopping ? up256((size_t)n_pairs * kWindow * 4) : 0;  // one window of rounds per pair
    const size_t b_cam = pose ? up256((size_t)n_pairs * 2 * sizeof(akz_camera)) : 0;
    PairsFront f;  // behind the pair table: done | need | cameras, on the device and (+ 256 for the count of pairs still running, in front of the cameras) in pinned memory
    AKZ_TRY(pairs_front(q, opt.lowes_ratio, opt.guided != 0, cross, b_done + b_need + b_cam, b_done + b_need + 256 + b_cam, f));
    hipStream_t st = c->stream;
    // the rounds' state: every pair's best model and count, its ring of a round's models and counts, the running counts per round
    const size_t b_bm = up256((size_t)n_pairs * 36), b_bi = up256((size_t)n_pairs * 4);
    const size_t b_rm = up256((size_t)n_pairs * AKZ_RANSAC_ROUND * 36), b_ri = up256((size_t)n_pairs * AKZ_RANSAC_ROUND * 4);
    const size_t b_run = up256((size_t)std::max<uint32_t>(n_rounds, 1) * 4);
    AKZ_TRY(ensure(c, c->mp_trials, b_bm + b_bi + b_rm + b_ri + b_run));
    uint32_t* d_done = (uint32_t*)f.d_own;
    uint32_t* d_need = stopping ? (uint32_t*)(f.d_own + b_done) : nullptr;
    float* d_bm = (float*)c->mp_trials.p;
    int32_t* d_bi = (int32_t*)((char*)c->mp_trials.p + b_bm);
    float* d_rm = (float*)((char*)c->mp_trials.p + b_bm + b_bi);
    int32_t* d_ri = (int32_t*)((char*)c->mp_trials.p + b_bm + b_bi + b_rm);
    uint32_t* d_run = (uint32_t*)((char*)c->mp_trials.p + b_bm + b_bi + b_rm + b_ri);
    uint32_t* h_done = (uint32_t*)f.h_own;  // | need, as on the device
    uint32_t* h_run = (uint32_t*)(f.h_own + b_done + b_need);
    AKZ_HIP_TRY(hipMemsetAsync(d_bm, 0, b_bm + b_bi, st));  // no winner yet: count 0, the zero model
    AKZ_HIP_TRY(hipMemsetAsync(d_run, 0, b_run, st));
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[2], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    // per pair: one "trial" for the pick (its best slot), the place of its kept list, done from the start with fewer than K
    // matches or no trials, and the stopping table
    const double t_need0 = now_ms();
    uint64_t n_keep = 0, n_running = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        launch::PairJobHost& j = f.tab[(size_t)p];
        const uint64_t n = f.h_cnt[j.cnt_idx];
        const bool runs = n >= K && max_trials > 0;
        j.trial_off = p;
        j.n_trials = runs ? 1 : 0;
        j.keep_off = n_keep;
        n_keep += n;
        h_done[p] = runs ? 0u : 1u;
        n_running += runs ? 1 : 0;
    }
    // need[pair][k] for rounds first .. first + kWindow of the pairs that run: filled when the window is about to be launched
    uint32_t* h_need = h_done + b_done / 4;
    auto fill_need = [&](uint32_t first) {
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const uint64_t n = f.h_cnt[f.tab[(size_t)p].cnt_idx];
            for (uint32_t k = 0; k < kWindow; ++k) {
                const uint64_t T = std::min<uint64_t>(max_trials, ((uint64_t)first + k + 1) * AKZ_RANSAC_ROUND);
                h_need[(size_t)p * kWindow + k] = h_done[p] == 0u && first + k < n_rounds ? (uint32_t)seeded_need(n, (int)K, T, opt.confidence) : 0u;
            }
        }
    };
    if (stopping) fill_need(0);
    double t_need = now_ms() - t_need0;
    PairsKeep keep{up256((size_t)n_pairs * 36), up256((size_t)n_pairs * 4), up256((size_t)n_pairs * 4), up256((size_t)n_pairs * 4)};
    if (pose) keep.b_pose = up256((size_t)n_pairs * sizeof(akz_pose)), keep.want_points = pose->points != nullptr;
    AKZ_TRY(pairs_keep(c, f, n_keep, keep));
    AKZ_TRY(pairs_table_upload(c, f));
    AKZ_HIP_TRY(hipMemcpyAsync(d_done, h_done, b_done + b_need, hipMemcpyHostToDevice, st));
    akz_camera* d_cam = (akz_camera*)(f.d_own + b_done + b_need);
    if (pose) {
        akz_camera* h_cam = (akz_camera*)(f.h_own + b_done + b_need + 256);
        for (uint64_t p = 0; p < n_pairs; ++p) h_cam[2 * p] = pose->cameras[q.pairs[2 * p]], h_cam[2 * p + 1] = pose->cameras[q.pairs[2 * p + 1]];
        AKZ_HIP_TRY(hipMemcpyAsync(d_cam, h_cam, (size_t)n_pairs * 2 * sizeof(akz_camera), hipMemcpyHostToDevice, st));
    }
    AKZ_HIP_TRY(hipMemsetAsync(keep.d.fits, 0, (char*)keep.d.points - (char*)keep.d.fits, st));  // fits | trials | poses (no pose where the stage leaves at once)
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
    const uint64_t k1 = seeded_seed_key(opt.seed[0], opt.seed[1]);
    for (uint32_t r = 0; r < n_rounds && n_running; ++r) {
        launch::seeded_round(st, kind, f.d_tab, (uint32_t)n_pairs, d_done, k1, opt.stream_base, r, max_trials, f.d_cnt, f.d_pts, f.cap1, epsilon_model,
                             opt.epsilon_inliers, d_rm, d_ri);
        launch::seeded_update(st, (uint32_t)n_pairs, r, max_trials, d_need, kWindow, r % kWindow, d_rm, d_ri, d_done, d_bi, d_bm, keep.d.trials, d_run);
        AKZ_HIP_TRY(hipGetLastError());
        if (stopping && (r + 1) % kWindow == 0 && r + 1 < n_rounds) {  // (without the rule every pair runs to max_trials)
            AKZ_HIP_TRY(hipMemcpyAsync(h_run, d_run + r, 4, hipMemcpyDeviceToHost, st));
            AKZ_HIP_TRY(hipStreamSynchronize(st));
            n_running = *h_run;
            if (n_running) {  // the next window's table (the stream is idle: the pinned table is free to rewrite)
                const double t0 = now_ms();
                fill_need(r + 1);
                t_need += now_ms() - t0;
                AKZ_HIP_TRY(hipMemcpyAsync(d_need, h_need, b_need, hipMemcpyHostToDevice, st));
            }
        }
    }
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[4], st));
    const RefineStage refine{opt.refine_iterations, nullptr};
    const GuidedStage guided{opt.guided_radius, opt.guided_lowes_ratio};
    const PoseStage stage{d_cam, pose ? pose->poses : nullptr, pose ? pose->points : nullptr};
    return pairs_tail(q, f, keep, kind, d_bm, d_bi, opt.epsilon_inliers, opt.refine_iterations > 0 ? &refine : nullptr, refit_epsilon,
                      opt.guided ? &guided : nullptr, guided_kind, t_need, model, found, iterations, trials_run, pose ? &stage : nullptr);
}

extern "C" int akz_match_features_seeded_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                               uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out, uint64_t* n_out,
                                               float* model, int* found, uint32_t* iterations, uint64_t* trials_run) {
    return match_seeded_pairs_impl({"match_features_seeded_pairs: ", c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr}, false, options,
                                   model, found, iterations, trials_run);
}
