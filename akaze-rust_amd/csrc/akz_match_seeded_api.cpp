// akz_match_features_seeded_pairs and, with the cross-check in front, akz_match_features_seeded_cross_pairs (additions;
// include/akaze_hip.h): match_features over many pairs with the seeded
// RANSAC of akz_ransac_seeded.hpp -- the trial kernel draws its own samples, the stopping rule runs per pair on the device, and
// the calling thread's random source is never touched.  Stages, all on the context's stream: upload, scans, k_pair_points and the
// ONE read-back of the match counts as in match_pairs_impl (akz_match_api.cpp: pairs_validate, pairs_place, pairs_upload,
// pairs_scans); the host's table need[pair][round of the window] (seeded_need, the one function the host statement calls too),
// filled and uploaded one window at a time -- its cost follows the rounds that are launched, not max_trials --; rounds of
// launch::seeded_round + launch::seeded_update, enqueued without a host synchronisation in windows of kWindow rounds -- after a window the host reads the count of pairs still running and stops launching at 0, which cannot change
// a result: a round of a finished pair leaves at once --; launch::pairs_pick_filter over the pairs' best slots as one trial per
// pair; launch::model_refit and the guided stage as in match_pairs_impl; ONE read-back whose head also carries trials_run.
// The guided stage, the span read-back and the copy-out below restate the tail of match_pairs_impl with one more head field: a
// fix to either is to be carried to the other.
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
// enqueues what it always did.
int match_seeded_pairs_impl(const char* name, bool cross, akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs,
                            uint64_t n_pairs, uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out, uint64_t* n_out,
                            float* model, int* found, uint32_t* iterations, uint64_t* trials_run) {
    constexpr uint32_t kWindow = 8;  // rounds enqueued between two looks at the pairs still running
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
    std::vector<uint8_t> seen;
    uint64_t cap = 0;
    AKZ_TRY(pairs_validate(name, c, sets, n_sets, pairs, n_pairs, desc_bytes, out, n_out, seen, cap));
    if (opt.guided) AKZ_TRY(guided_limits(name, sets, pairs, n_pairs, seen));
    AKZ_TRY(bind(c, true, false));
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
    const bool timed = c->mp_split_on;
    if (timed)
        for (hipEvent_t& e : c->mp_split_ev)
            if (!e) AKZ_HIP_TRY(hipEventCreate(&e));
    hipStream_t st = c->stream;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    std::vector<uint64_t> set_row, used;
    const uint64_t rows = pairs_place(sets, n_sets, pairs, n_pairs, seen, set_row, used);
    const uint64_t rows1 = std::max<uint64_t>(rows, 1), cap1 = std::max<uint64_t>(cap, 1);
    const size_t b_rows = up((size_t)rows1 * 64), b_xy = up((size_t)rows1 * 4);
    const size_t b_raw = up((size_t)cap1 * sizeof(akz_match)), b_cnt = up((size_t)n_pairs * 8), b_pts = (size_t)cap1 * 16;
    const size_t b_tab = up((size_t)n_pairs * sizeof(launch::PairJobHost)), b_done = up((size_t)n_pairs * 4);
    const size_t b_need = stopping ? up((size_t)n_pairs * kWindow * 4) : 0;  // one window of rounds per pair
    // the rounds' state: every pair's best model and count, its ring of a round's models and counts, the running counts per round
    const size_t b_bm = up((size_t)n_pairs * 36), b_bi = up((size_t)n_pairs * 4);
    const size_t b_rm = up((size_t)n_pairs * AKZ_RANSAC_ROUND * 36), b_ri = up((size_t)n_pairs * AKZ_RANSAC_ROUND * 4);
    const size_t b_run = up((size_t)std::max<uint32_t>(n_rounds, 1) * 4);
    AKZ_TRY(ensure(c, c->mp_in, b_rows + 2 * b_xy));
    AKZ_TRY(ensure(c, c->mp_raw, b_raw + b_cnt + b_pts));
    AKZ_TRY(ensure(c, c->mp_tab, b_tab + b_done + b_need));
    AKZ_TRY(ensure(c, c->mp_trials, b_bm + b_bi + b_rm + b_ri + b_run));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_in, b_rows + 2 * b_xy));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_tab, b_tab + b_cnt + b_done + b_need + 256));
    uint8_t* d_rows = (uint8_t*)c->mp_in.p;
    float *d_kx = (float*)(d_rows + b_rows), *d_ky = (float*)(d_rows + b_rows + b_xy);
    akz_match* d_raw = (akz_match*)c->mp_raw.p;
    uint64_t* d_cnt = (uint64_t*)((char*)c->mp_raw.p + b_raw);
    float* d_pts = (float*)((char*)c->mp_raw.p + b_raw + b_cnt);
    launch::PairJobHost* d_tab = (launch::PairJobHost*)c->mp_tab.p;
    uint32_t* d_done = (uint32_t*)((char*)c->mp_tab.p + b_tab);
    uint32_t* d_need = stopping ? (uint32_t*)((char*)c->mp_tab.p + b_tab + b_done) : nullptr;
    float* d_bm = (float*)c->mp_trials.p;
    int32_t* d_bi = (int32_t*)((char*)c->mp_trials.p + b_bm);
    float* d_rm = (float*)((char*)c->mp_trials.p + b_bm + b_bi);
    int32_t* d_ri = (int32_t*)((char*)c->mp_trials.p + b_bm + b_bi + b_rm);
    uint32_t* d_run = (uint32_t*)((char*)c->mp_trials.p + b_bm + b_bi + b_rm + b_ri);
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[0], st));
    AKZ_TRY(pairs_upload(c, sets, used, set_row, rows, desc_bytes, b_rows, b_xy));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[1], st));
    std::vector<launch::PairJobHost> tab;
    if (cross) {  // the reverse lists (room: every pair's second set), their counts and the filter's records
        uint64_t cap_rev = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) cap_rev += sets[pairs[2 * p + 1]].n_descriptors;
        const size_t b_rev = up((size_t)std::max<uint64_t>(cap_rev, 1) * sizeof(akz_match)), b_xtab = up((size_t)n_pairs * sizeof(launch::CrossJobHost));
        AKZ_TRY(ensure(c, c->cx_rev, b_rev + b_cnt + b_xtab));
        AKZ_TRY(ensure_pinned(c, c->cx_pin_tab, b_xtab));
        akz_match* d_rev = (akz_match*)c->cx_rev.p;
        uint64_t* d_rcnt = (uint64_t*)((char*)c->cx_rev.p + b_rev);
        launch::CrossJobHost* d_xtab = (launch::CrossJobHost*)((char*)c->cx_rev.p + b_rev + b_cnt);
        std::vector<launch::CrossJobHost> xtab;
        AKZ_TRY(pairs_scans(c, sets, n_sets, pairs, n_pairs, desc_bytes, opt.lowes_ratio, set_row, d_rows, d_raw, d_cnt, tab, d_rev, d_rcnt, &xtab));
        std::memcpy(c->cx_pin_tab.p, xtab.data(), (size_t)n_pairs * sizeof(launch::CrossJobHost));
        AKZ_HIP_TRY(hipMemcpyAsync(d_xtab, c->cx_pin_tab.p, (size_t)n_pairs * sizeof(launch::CrossJobHost), hipMemcpyHostToDevice, st));
        launch::pairs_cross_filter(st, d_xtab, (uint32_t)n_pairs, d_raw, d_cnt, d_rev, d_rcnt);
        AKZ_HIP_TRY(hipGetLastError());
    } else {
        AKZ_TRY(pairs_scans(c, sets, n_sets, pairs, n_pairs, desc_bytes, opt.lowes_ratio, set_row, d_rows, d_raw, d_cnt, tab));
    }
    launch::PairJobHost* h_tab = (launch::PairJobHost*)c->mp_pin_tab.p;
    uint64_t* h_cnt = (uint64_t*)((char*)c->mp_pin_tab.p + b_tab);
    uint32_t* h_done = (uint32_t*)((char*)c->mp_pin_tab.p + b_tab + b_cnt);  // | need, as on the device
    uint32_t* h_run = (uint32_t*)((char*)c->mp_pin_tab.p + b_tab + b_cnt + b_done + b_need);
    std::memcpy(h_tab, tab.data(), (size_t)n_pairs * sizeof(launch::PairJobHost));
    AKZ_HIP_TRY(hipMemcpyAsync(d_tab, h_tab, (size_t)n_pairs * sizeof(launch::PairJobHost), hipMemcpyHostToDevice, st));
    launch::pair_points(st, d_tab, (uint32_t)n_pairs, d_raw, d_cnt, d_kx, d_ky, d_pts, cap1);
    AKZ_HIP_TRY(hipGetLastError());
    AKZ_HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    AKZ_HIP_TRY(hipMemsetAsync(d_bm, 0, b_bm + b_bi, st));  // no winner yet: count 0, the zero model
    AKZ_HIP_TRY(hipMemsetAsync(d_run, 0, b_run, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[2], st));
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    // per pair: one "trial" for the pick (its best slot), the place of its kept list, done from the start with fewer than K
    // matches or no trials, and the stopping table
    const double t_need0 = now_ms();
    uint64_t n_keep = 0, n_running = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        launch::PairJobHost& j = tab[(size_t)p];
        const uint64_t n = h_cnt[j.cnt_idx];
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
            const uint64_t n = h_cnt[tab[(size_t)p].cnt_idx];
            for (uint32_t k = 0; k < kWindow; ++k) {
                const uint64_t T = std::min<uint64_t>(max_trials, ((uint64_t)first + k + 1) * AKZ_RANSAC_ROUND);
                h_need[(size_t)p * kWindow + k] = h_done[p] == 0u && first + k < n_rounds ? (uint32_t)seeded_need(n, (int)K, T, opt.confidence) : 0u;
            }
        }
    };
    if (stopping) fill_need(0);
    double t_need = now_ms() - t_need0;
    // the head of the read-back: kept counts | models | found | accepted fits | trials run, then the kept lists
    const size_t b_hm = up((size_t)n_pairs * 36), b_hf = up((size_t)n_pairs * 4), b_it = up((size_t)n_pairs * 4), b_tr = up((size_t)n_pairs * 4);
    const size_t b_head = b_cnt + b_hm + b_hf + b_it + b_tr;
    const size_t b_keep = b_head + (size_t)std::max<uint64_t>(n_keep, 1) * sizeof(akz_match);
    AKZ_TRY(ensure(c, c->mp_keep, b_keep));
    AKZ_TRY(ensure_pinned(c, c->mp_pin_out, b_keep));
    uint64_t* d_kcnt = (uint64_t*)c->mp_keep.p;
    float* d_hm = (float*)((char*)c->mp_keep.p + b_cnt);
    int32_t* d_hf = (int32_t*)((char*)c->mp_keep.p + b_cnt + b_hm);
    uint32_t* d_it = (uint32_t*)((char*)c->mp_keep.p + b_cnt + b_hm + b_hf);
    uint32_t* d_tr = (uint32_t*)((char*)c->mp_keep.p + b_cnt + b_hm + b_hf + b_it);
    akz_match* d_keep = (akz_match*)((char*)c->mp_keep.p + b_head);
    std::memcpy(h_tab, tab.data(), (size_t)n_pairs * sizeof(launch::PairJobHost));
    AKZ_HIP_TRY(hipMemcpyAsync(d_tab, h_tab, (size_t)n_pairs * sizeof(launch::PairJobHost), hipMemcpyHostToDevice, st));
    AKZ_HIP_TRY(hipMemcpyAsync(d_done, h_done, b_done + b_need, hipMemcpyHostToDevice, st));
    AKZ_HIP_TRY(hipMemsetAsync(d_it, 0, b_it + b_tr, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[3], st));
    const uint64_t k1 = seeded_seed_key(opt.seed[0], opt.seed[1]);
    for (uint32_t r = 0; r < n_rounds && n_running; ++r) {
        launch::seeded_round(st, kind, d_tab, (uint32_t)n_pairs, d_done, k1, opt.stream_base, r, max_trials, d_cnt, d_pts, cap1, epsilon_model,
                             opt.epsilon_inliers, d_rm, d_ri);
        launch::seeded_update(st, (uint32_t)n_pairs, r, max_trials, d_need, kWindow, r % kWindow, d_rm, d_ri, d_done, d_bi, d_bm, d_tr, d_run);
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
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[4], st));
    launch::pairs_pick_filter(st, kind, d_tab, (uint32_t)n_pairs, d_raw, d_cnt, d_pts, cap1, d_bm, d_bi, opt.epsilon_inliers, d_keep, d_kcnt, d_hm,
                              d_hf);
    AKZ_HIP_TRY(hipGetLastError());
    if (opt.refine_iterations > 0) {
        launch::model_refit(st, kind, d_tab, (uint32_t)n_pairs, d_raw, d_cnt, d_pts, cap1, refit_epsilon, opt.epsilon_inliers,
                            opt.refine_iterations, d_keep, d_kcnt, d_hm, d_hf, d_it);
        AKZ_HIP_TRY(hipGetLastError());
    }
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[5], st));
    AKZ_HIP_TRY(hipMemcpyAsync(c->mp_pin_out.p, c->mp_keep.p, b_head + (size_t)n_keep * sizeof(akz_match), hipMemcpyDeviceToHost, st));
    if (timed) AKZ_HIP_TRY(hipEventRecord(c->mp_split_ev[6], st));
    // the guided stage, as in match_pairs_impl: every pair scanned again with the model on the device
    akz_match* d_gout = nullptr;
    if (opt.guided) {
        AKZ_TRY(ensure(c, c->gd_out, b_cnt + (size_t)cap1 * sizeof(akz_match)));
        AKZ_TRY(ensure_pinned(c, c->gd_pin_cnt, b_cnt));
        uint64_t* d_gcnt = (uint64_t*)c->gd_out.p;
        d_gout = (akz_match*)((char*)c->gd_out.p + b_cnt);
        std::vector<GuidedPairSpec> spec((size_t)n_pairs);
        uint64_t off = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            const uint64_t a = pairs[2 * p], b = pairs[2 * p + 1];
            spec[(size_t)p] = GuidedPairSpec{set_row[(size_t)a], sets[a].n_descriptors, set_row[(size_t)b], sets[b].n_descriptors, off};
            off += sets[a].n_descriptors;
        }
        AKZ_TRY(guided_enqueue(c, spec, d_rows, d_kx, d_ky, guided_kind, d_hm, d_hf, opt.guided_radius, 10000, opt.guided_lowes_ratio, d_gout,
                               d_gcnt));
        AKZ_HIP_TRY(hipMemcpyAsync(c->gd_pin_cnt.p, d_gcnt, (size_t)n_pairs * 8, hipMemcpyDeviceToHost, st));
    }
    AKZ_HIP_TRY(hipStreamSynchronize(st));
    const char* head = (const char*)c->mp_pin_out.p;
    const uint64_t* h_kcnt = (const uint64_t*)head;
    const float* h_hm = (const float*)(head + b_cnt);
    const int32_t* h_hf = (const int32_t*)(head + b_cnt + b_hm);
    const uint32_t* h_it = (const uint32_t*)(head + b_cnt + b_hm + b_hf);
    const uint32_t* h_tr = (const uint32_t*)(head + b_cnt + b_hm + b_hf + b_it);
    const akz_match* h_keep = (const akz_match*)(head + b_head);
    const uint64_t* h_gcnt = opt.guided ? (const uint64_t*)c->gd_pin_cnt.p : nullptr;
    const akz_match* h_gout = nullptr;
    if (opt.guided) {  // the guided lists of the pairs with a model: ONE read-back of the span they occupy
        uint64_t span = 0, off = 0;
        for (uint64_t p = 0; p < n_pairs; ++p) {
            if (h_hf[p] && h_gcnt[p]) span = off + h_gcnt[p];
            off += sets[pairs[2 * p]].n_descriptors;
        }
        if (span) {
            AKZ_TRY(ensure_pinned(c, c->gd_pin_out, (size_t)span * sizeof(akz_match)));
            AKZ_HIP_TRY(hipMemcpyAsync(c->gd_pin_out.p, d_gout, (size_t)span * sizeof(akz_match), hipMemcpyDeviceToHost, st));
            AKZ_HIP_TRY(hipStreamSynchronize(st));
            h_gout = (const akz_match*)c->gd_pin_out.p;
        }
    }
    uint64_t at = 0;
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (opt.guided && h_hf[p] != 0) {  // found: the guided list replaces the filtered one
            const uint64_t g = h_gcnt[p];
            if (g) std::memcpy(out + at, h_gout + at, (size_t)g * sizeof(akz_match));
            n_out[p] = g;
        } else {
            const uint64_t k = h_kcnt[p];
            if (k) std::memcpy(out + at, h_keep + tab[(size_t)p].keep_off, (size_t)k * sizeof(akz_match));
            n_out[p] = k;
        }
        at += sets[pairs[2 * p]].n_descriptors;
    }
    if (model) std::memcpy(model, h_hm, (size_t)n_pairs * 36);
    for (uint64_t p = 0; p < n_pairs; ++p) {
        if (found) found[p] = h_hf[p];
        if (iterations) iterations[p] = h_it[p];
        if (trials_run) trials_run[p] = h_tr[p];
    }
    if (timed) {  // akz_debug_match_pairs_split: [2] is the host's stopping table here, [3] the rounds
        float ms[6] = {};
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[0], c->mp_split_ev[0], c->mp_split_ev[1]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[1], c->mp_split_ev[1], c->mp_split_ev[2]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[3], c->mp_split_ev[3], c->mp_split_ev[4]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[4], c->mp_split_ev[4], c->mp_split_ev[5]));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms[5], c->mp_split_ev[5], c->mp_split_ev[6]));
        for (int k = 0; k < 6; ++k) c->mp_split_ms[k] = ms[k];
        c->mp_split_ms[2] = t_need;
    }
    return AKZ_OK;
}

extern "C" int akz_match_features_seeded_pairs(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const uint64_t* pairs, uint64_t n_pairs,
                                               uint64_t desc_bytes, const akz_ransac_options* options, akz_match* out, uint64_t* n_out,
                                               float* model, int* found, uint32_t* iterations, uint64_t* trials_run) {
    return match_seeded_pairs_impl("match_features_seeded_pairs: ", false, c, sets, n_sets, pairs, n_pairs, desc_bytes, options, out, n_out, model,
                                   found, iterations, trials_run);
}
