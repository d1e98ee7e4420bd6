// akz_match_features_seeded_pairs and, with the cross-check in front, akz_match_features_seeded_cross_pairs (additions;
// include/akaze_hip.h): match_features over many pairs with the seeded
// RANSAC of akz_ransac_seeded.hpp -- the trial kernel draws its own samples, the stopping rule runs per pair on the device, and
// the calling thread's random source is never touched.  The call is pairs_front and pairs_tail (akz_match_api.cpp) around the rounds.
// The rounds are seeded_rounds_device, the driver of every seeded call (the resection's too, akz_resection_api.cpp): the host's table
// need[entry][round of the window] (seeded_need, the one function the host statement calls too), filled and uploaded one window at a
// time -- its cost follows the rounds that are launched, not max_trials --; rounds of the caller's launch + launch::seeded_update,
// enqueued without a host synchronisation in windows of kWindow rounds -- after a window the host reads the count of entries still
// running and stops launching at 0, which cannot change a result: a round of a finished entry leaves at once.  The tail picks over
// the pairs' best slots as one trial per pair, and the head of its read-back also carries trials_run.
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

SeededState::SeededState(uint64_t n_, uint32_t model_floats_, const akz_ransac_options& opt)
    : n(n_), model_floats(model_floats_), max_trials((uint32_t)opt.max_trials), n_rounds((max_trials + AKZ_RANSAC_ROUND - 1) / AKZ_RANSAC_ROUND),
      confidence(opt.confidence) {
    const size_t np = (size_t)n;
    b_bm = up256(np * model_floats * 4), b_bi = up256(np * 4), b_rm = up256(np * AKZ_RANSAC_ROUND * model_floats * 4);
    b_ri = up256(np * AKZ_RANSAC_ROUND * 4), b_run = up256((size_t)std::max<uint32_t>(n_rounds, 1) * 4);
    b_done = up256(np * 4), b_need = stopping() ? up256(np * kWindow * 4) : 0;
}
void SeededState::place(void* d_state) {
    char* d = (char*)d_state;
    d_bm = (float*)d, d_bi = (int32_t*)(d + b_bm), d_rm = (float*)(d + b_bm + b_bi), d_ri = (int32_t*)(d + b_bm + b_bi + b_rm);
    d_run = (uint32_t*)(d + b_bm + b_bi + b_rm + b_ri);
}
void SeededState::tables(void* d_done_need, void* h_done_need, void* h_word) {
    d_done = (uint32_t*)d_done_need, h_done = (uint32_t*)h_done_need, h_run = (uint32_t*)h_word;
    h_need = h_done + b_done / 4;  // (as on the device)
    if (stopping()) d_need = d_done + b_done / 4;
}
int SeededState::clear(hipStream_t st) const {
    AKZ_HIP_TRY(hipMemsetAsync(d_bm, 0, b_bm + b_bi, st));  // no winner yet: count 0, the zero model
    AKZ_HIP_TRY(hipMemsetAsync(d_run, 0, b_run, st));
    return AKZ_OK;
}

int seeded_rounds_device(hipStream_t st, SeededState& s, int K, uint64_t n_running, const std::function<uint64_t(uint64_t)>& n_of,
                  const std::function<int()>& upload, const std::function<void(uint32_t)>& round, double* t_need) {
    constexpr uint32_t kWindow = SeededState::kWindow;
    // need[entry][k] for rounds first .. first + kWindow of the entries that run: filled when the window is about to be launched
    // (K as a constant: the bisection's product unrolls -- 20 ns a call, on a table of thousands of entries per window)
    auto need = [&](uint64_t n, uint64_t T) { return K == 4 ? seeded_need(n, 4, T, s.confidence) : K == 6 ? seeded_need(n, 6, T, s.confidence) : seeded_need(n, 8, T, s.confidence); };
    auto fill_need = [&](uint32_t first) {
        const double t0 = now_ms();
        for (uint64_t p = 0; p < s.n; ++p) {
            const uint64_t n = n_of(p);
            for (uint32_t k = 0; k < kWindow; ++k) {
                const uint64_t T = std::min<uint64_t>(s.max_trials, ((uint64_t)first + k + 1) * AKZ_RANSAC_ROUND);
                s.h_need[(size_t)p * kWindow + k] = s.h_done[p] == 0u && first + k < s.n_rounds ? (uint32_t)need(n, T) : 0u;
            }
        }
        if (t_need) *t_need += now_ms() - t0;
    };
    if (s.stopping()) fill_need(0);
    AKZ_TRY(upload());
    for (uint32_t r = 0; r < s.n_rounds && n_running; ++r) {
        round(r);
        launch::seeded_update(st, (uint32_t)s.n, r, s.max_trials, s.d_need, kWindow, r % kWindow, s.d_rm, s.d_ri, s.d_done, s.d_bi, s.d_bm, s.d_trials,
                              s.d_run, s.model_floats);
        AKZ_HIP_TRY(hipGetLastError());
        if (s.stopping() && (r + 1) % kWindow == 0 && r + 1 < s.n_rounds) {  // (without the rule every entry runs to max_trials)
            AKZ_HIP_TRY(hipMemcpyAsync(s.h_run, s.d_run + r, 4, hipMemcpyDeviceToHost, st));
            AKZ_HIP_TRY(hipStreamSynchronize(st));
            n_running = *s.h_run;
            if (n_running) {  // the next window's table (the stream is idle: the pinned table is free to rewrite)
                fill_need(r + 1);
                AKZ_HIP_TRY(hipMemcpyAsync(s.d_need, s.h_need, s.b_need, hipMemcpyHostToDevice, st));
            }
        }
    }
    return AKZ_OK;
}

// cross: every pair's raw list is cross(A, B) (akz_match_features_seeded_cross_pairs, akz_cross_api.cpp) -- pairs_scans also
// writes the opposite direction and launch::pairs_cross_filter rewrites d_raw / d_cnt before anything reads them; clear, the call
// enqueues what it always did.  pose: akz_match_features_seeded_pose_pairs (akz_pose_api.cpp, which has refused what that call refuses) --
// the pairs' cameras ride behind done | need, the head carries the poses (zeroed with the fits and the trial counts) and the points, and
// the tail runs launch::pairs_pose; null, nothing of it is allocated or enqueued.  q.bank: the sets lie in a feature bank (akz_bank_api.cpp) --
// the front opens on its block and uploads no set; everything else is the same code over the same table.
int match_seeded_pairs_impl(const PairsCall& q, bool cross, const akz_ransac_options* options, float* model, int* found, uint32_t* iterations,
                            uint64_t* trials_run, const SeededPose* pose) {
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
    SeededState s(n_pairs, 9, opt);
    const uint32_t max_trials = s.max_trials;
    const size_t b_done = s.b_done, b_need = s.b_need;  // (need: one window of rounds per pair)
    const size_t b_cam = pose ? up256((size_t)n_pairs * 2 * sizeof(akz_camera)) : 0;
    PairsFront f;  // behind the pair table: done | need | cameras, on the device and (+ 256 for the count of pairs still running, in front of the cameras) in pinned memory
    AKZ_TRY(pairs_front(q, opt.lowes_ratio, opt.guided != 0, cross, b_done + b_need + b_cam, b_done + b_need + 256 + b_cam, f));
    hipStream_t st = c->stream;
    AKZ_TRY(ensure(c, c->mp_trials, s.bytes()));
    s.place(c->mp_trials.p);
    s.tables(f.d_own, f.h_own, f.h_own + b_done + b_need);
    AKZ_TRY(s.clear(st));
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[2], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    // per pair: one "trial" for the pick (its best slot), the place of its kept list, done from the start with fewer than K
    // matches or no trials; the stopping table is the rounds'
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
        s.h_done[p] = runs ? 0u : 1u;
        n_running += runs ? 1 : 0;
    }
    double t_need = now_ms() - t_need0;
    PairsKeep keep{up256((size_t)n_pairs * 36), up256((size_t)n_pairs * 4), up256((size_t)n_pairs * 4), up256((size_t)n_pairs * 4)};
    if (pose) keep.b_pose = up256((size_t)n_pairs * sizeof(akz_pose)), keep.want_points = pose->points != nullptr;
    akz_camera* d_cam = (akz_camera*)(f.d_own + b_done + b_need);
    const uint64_t k1 = seeded_seed_key(opt.seed[0], opt.seed[1]);
    AKZ_TRY(seeded_rounds_device(
        st, s, (int)K, n_running, [&](uint64_t p) { return f.h_cnt[f.tab[(size_t)p].cnt_idx]; },
        [&]() -> int {
            AKZ_TRY(pairs_keep(c, f, n_keep, keep));
            s.d_trials = keep.d.trials;
            AKZ_TRY(pairs_table_upload(c, f));
            AKZ_HIP_TRY(hipMemcpyAsync(s.d_done, s.h_done, b_done + b_need, hipMemcpyHostToDevice, st));
            if (pose) {
                akz_camera* h_cam = (akz_camera*)(f.h_own + b_done + b_need + 256);
                for (uint64_t p = 0; p < n_pairs; ++p) h_cam[2 * p] = pose->cameras[q.pairs[2 * p]], h_cam[2 * p + 1] = pose->cameras[q.pairs[2 * p + 1]];
                AKZ_HIP_TRY(hipMemcpyAsync(d_cam, h_cam, (size_t)n_pairs * 2 * sizeof(akz_camera), hipMemcpyHostToDevice, st));
            }
            AKZ_HIP_TRY(hipMemsetAsync(keep.d.fits, 0, (char*)keep.d.points - (char*)keep.d.fits, st));  // fits | trials | poses (no pose where the stage leaves at once)
            if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
            return AKZ_OK;
        },
        [&](uint32_t r) {
            launch::seeded_round(st, kind, f.d_tab, (uint32_t)n_pairs, s.d_done, k1, opt.stream_base, r, max_trials, f.d_cnt, f.d_pts, f.cap1,
                                 epsilon_model, opt.epsilon_inliers, s.d_rm, s.d_ri);
        },
        &t_need));
    if (f.timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[4], st));
    const RefineStage refine{opt.refine_iterations, nullptr};
    const GuidedStage guided{opt.guided_radius, opt.guided_lowes_ratio};
    const PoseStage stage{d_cam, pose ? pose->poses : nullptr, pose ? pose->points : nullptr};
    return pairs_tail(q, f, keep, kind, s.d_bm, s.d_bi, opt.epsilon_inliers, opt.refine_iterations > 0 ? &refine : nullptr, refit_epsilon,
                      opt.guided ? &guided : nullptr, guided_kind, t_need, model, found, iterations, trials_run, pose ? &stage : nullptr);
}

extern "C" int akz_match_features_seeded_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                               uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out, uint64_t* n_out,
                                               float* model, int* found, uint32_t* iterations, uint64_t* trials_run) {
    return match_seeded_pairs_impl({"match_features_seeded_pairs: ", c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, nullptr}, false, options,
                                   model, found, iterations, trials_run);
}
