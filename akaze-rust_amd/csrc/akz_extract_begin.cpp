// C ABI of libakaze_hip.so, part 3a: the begin half of extract_features -- scale space, detectors, NMS candidates, all enqueued
// without a host synchronisation.  extract_begin opens the job, fills a BeginRoute (which kernel every level takes, where the
// chain forks: decided once) and runs the stages below over one BeginState in the order the route gives.
#include "akz_extract.hpp"

namespace {
enum class Prep : uint8_t {
    Tiled,       // k_prep -- unless the level's planes came with k_head (level 1) or rode on the previous level's last k_fed_own
    Stream,      // k_prep_stream
    LevelMarch,  // k_level_march: preparation and the first n1 diffusion steps in one launch
    Resident     // covered by the resident tail's one launch (from res_first on)
};
enum class Det : uint8_t {  // detector_family's 0 split in two, 4 and 5
    Fallback,  // 0, no fused form: k_deriv1 + k_deriv2 + k_nms, which borrow context scratch planes
    NmsFused,  // 0, but the kernel size has the fused derivative + NMS form
    TiledSet,  // 4: levels of one sigma_size grouped into one launch
    March      // 5
};
// The schedule of one begin half, filled once by begin_route before anything is enqueued.  Two things are only known while
// enqueueing and are NOT here: whether k_head took level 0 (BeginState::head_fused, reported by head_impl) and whether a level's
// preparation rode on the previous level's last diffusion launch (BeginState::prepared, reported by fed_impl).
struct BeginRoute {
    bool big = false;           // the job takes the batch path (column marches, forked coarse chain, resident tail)
    int pre_on = 0;             // level 0 runs ahead on: 0 nothing (the context's stream), 2 the copy stream, 1 a stream of its own
    bool level1_clone = false;  // level 1 continues level 0's octave: k_head can leave its Lsmooth and the Scharr pair
    size_t res_first = 0;       // first level of the resident tail (L: none)
    size_t fork_level = 0;      // first level of the coarse chain (L: no fork)
    size_t oct1 = 0;            // first level past the first octave (fork_level if there is none on the main stream)
    bool own_kernels = true;    // no level of the coarse chain takes Det::Fallback (else the join is on the main stream)
    struct Level {
        Prep prep = Prep::Tiled;
        uint32_t n1 = 0, rem = 0;  // LevelMarch: diffusion steps inside k_level_march / left to k_fed_own
        bool fold_half = false;    // LevelMarch: the 2x2 mean of a new octave is formed inside the level kernel
        bool may_ride = false;     // Tiled: the previous level's last k_fed_own launch may write this level's Lsmooth and Lflow
        Det det = Det::Fallback;
    };
    std::vector<Level> lv;
};

// No HIP call, nothing mutated.  What the job decided comes as `f` (its stream is not looked at) and `big`; of the context only
// settings that no job overrides are read.
BeginRoute begin_route(const akz_ctx* c, const JobForm& f, const std::vector<LevelPlan>& plan, const akz_config& cfg, uint32_t w, uint32_t h,
                       uint32_t n, uint32_t flags, bool input_ready, bool big) {
    const size_t L = plan.size();
    BeginRoute rt;
    rt.big = big;
    rt.lv.resize(L);
    const int pre_mode = c->settings.sched[SCHED_EARLY_STREAM] == 0 ? c->pre_mode : c->settings.sched[SCHED_EARLY_STREAM] == 1 ? 2 : c->settings.sched[SCHED_EARLY_STREAM] == 2 ? 1 : 0;  // (1: a stream of its own, measurement only)
    if ((input_ready || (flags & AKZ_INPUT_READY)) && pre_mode != 0 && c->settings.profiling < 2 && f.prep_mode == 2 && big &&
        launch::blur5_march_supported(w, h, (uint32_t)gaussian_kernel_size((float)cfg.base_scale_offset)) &&
        launch::contrast_march_supported(w, h, (uint32_t)gaussian_kernel_size(1.0f), (uint32_t)cfg.contrast_factor_num_bins))
        rt.pre_on = pre_mode;
    rt.level1_clone = L > 1 && plan[1].octave == plan[0].octave && plan[1].w == w && plan[1].h == h;
    // Fork.  From octave `fork_octave` on the levels are small: their launches (diffusion, preparation, detectors) do not
    // fill the chip and are bound by launch-to-launch latency -- about 1 ms of the step for 8 % of its pixels.  That
    // chain moves to a second stream when octave fork_octave - 1 is finished, and the main stream goes straight to the
    // detectors of the fine octaves (bandwidth-bound, 2.2 ms): the two run side by side and join before the candidate
    // list is read.  (Running two BIG kernels side by side is a loss -- see extract_begin -- so the fork is at octave 2.)
    const int fork_octave = c->settings.sched[SCHED_FORK_OCTAVE] > 0 ? c->settings.sched[SCHED_FORK_OCTAVE] : 2;  // (forking at octave 3 instead, octave 2 on the main stream: -4 %; sched[SCHED_FORK_OCTAVE]: measurement)
    // (a lone 1080p frame is a chain of dependent launches either way and only pays for the two events: measured
    // 0.596 -> 0.625 ms per streamed frame; batch-path jobs (gates::kBigPxSync / kBigPxAsync) fork)
    // Resident tail: from the first level whose image fits one compute unit, ALL remaining levels (preparation and
    // every diffusion step, across octaves) are one launch with one workgroup per image (akz_resident.hip).
    // One workgroup advances an image by one diffusion step in ~2 us whatever the batch size, so a lone frame, whose
    // launch chain is bound by latency, keeps the separate launches (octave 3 of a 1080p frame: 0.11 ms as 12 launches
    // against 0.32 ms resident); a batch that forks its coarse chain onto the second stream hides that latency under
    // the fine detectors and gains what the 17 small launches cost those detectors (5.9 -> 5.3 ms per 32-frame step).
    rt.res_first = L;
    if (c->settings.fed_mode == 2 && (f.prep_mode == 3 || (f.prep_mode == 2 && big))) {
        size_t f = 1;
        while (f < L && !launch::octave_resident_supported(plan[f].w, plan[f].h)) ++f;
        f = std::max(f, L > (size_t)launch::kResidentMaxLevels ? L - (size_t)launch::kResidentMaxLevels : (size_t)1);
        size_t steps = 0;
        bool ok = true;
        for (size_t l = L; l-- > f;) {
            if (plan[l].tau.empty()) ok = false;
            steps += plan[l].tau.size();
            if (steps > (size_t)launch::kResidentMaxSteps) {  // keep the tail that fits
                steps -= plan[l].tau.size();
                f = l + 1;
                break;
            }
        }
        if (ok && f < L) rt.res_first = f;
    }
    // (full stage profiling attributes time to stages: it keeps everything on one stream)
    rt.fork_level = L;
    if (fork_octave > 0 && c->settings.profiling < 2 && big)
        for (size_t i = 1; i < L && rt.fork_level == L; ++i)
            if ((int)plan[i].octave >= fork_octave) rt.fork_level = i;
    // small frames in a large batch: the resident tail may start before octave 2 -- the chain then forks where the tail
    // starts (run_levels stops at the resident launch, which covers every level behind it: a fork behind that point
    // would run those levels a second time as separate launches)
    if (rt.fork_level < L && rt.res_first < rt.fork_level) rt.fork_level = rt.res_first;
    rt.oct1 = 1;
    while (rt.oct1 < rt.fork_level && plan[rt.oct1].octave == plan[0].octave) ++rt.oct1;

    for (size_t l = 0; l < L; ++l) {
        const LevelPlan& lv = plan[l];
        BeginRoute::Level& q = rt.lv[l];
        const int fam = detector_family(c, f, lv.det_sigma, lv.w, lv.h, n, border_margin(lv, cfg));
        q.det = fam == 5 ? Det::March : fam == 4 ? Det::TiledSet : launch::detector_nms_fused_supported(lv.det_sigma) ? Det::NmsFused : Det::Fallback;
        if (l >= rt.fork_level && q.det == Det::Fallback) rt.own_kernels = false;
        if (l == 0) continue;
        const LevelPlan& pv = plan[l - 1];
        const bool half = lv.octave > pv.octave;
        const uint64_t lpx = (uint64_t)lv.w * lv.h * n;
        if (l >= rt.res_first) {
            q.prep = Prep::Resident;
        } else if (!lv.tau.empty() && c->settings.fed_mode == 2 && launch::level_march_supported(lv.w, lv.h) &&
                   (f.prep_mode == 3 || (f.prep_mode == 2 && lpx >= gates::kLevelMarchPx))) {
            q.prep = Prep::LevelMarch;
            q.n1 = std::min<uint32_t>((uint32_t)lv.tau.size(), 4u);
            q.rem = (uint32_t)lv.tau.size() - q.n1;
            // a new octave: the 2x2 mean of the previous Lt is formed inside the level kernel where the widths allow it
            // (one launch and one plane round trip less per octave), materialised first otherwise
            q.fold_half = half && launch::level_march_half_supported(lv.w, lv.h, pv.w, pv.h, q.n1);
        } else if (f.prep_mode != 0 && launch::prep_stream_supported(lv.w, lv.h) &&
                   (f.prep_mode == 1 || (f.prep_mode >= 2 && !half && lpx >= c->settings.stream_min_px))) {
            // measured on MI355X: the streaming kernel is ~2x faster for cloned levels of a batch (a single
            // frame is launch-latency bound and stays on the tiled kernel); for the first
            // level of an octave (2x2 mean of a 4x larger input) the two are equal, the tiled one stays
            q.prep = Prep::Stream;
        }
        // The next level of the octave starts from this level's final Lt: where it would take the tiled preparation
        // (k_prep), the last diffusion launch of this level writes its Lsmooth and Lflow as well -- one dependent launch
        // less per level of a lone frame's chain (sched[SCHED_PREP_OWN_LAUNCH] = 1: a launch of its own, as before)
        q.may_ride = c->settings.sched[SCHED_PREP_OWN_LAUNCH] == 0 && c->settings.fed_mode == 2 && lv.octave == pv.octave && q.prep == Prep::Tiled;
    }
    return rt;
}

struct BeginState {
    akz_ctx* c;
    akz_result* r;
    const BeginRoute& rt;
    uint32_t n;
    bool keep_all;
    JobForm form;    // what the job decided; form.stream is the caller's stream
    JobForm chain;   // ... as the level chain enqueues: form, or with the coarse stream behind the fork
    uint64_t seq;    // published (c->begin_seq) when this job's fed_ev has been recorded
    // One append list for the whole batch (image id stored per candidate): a single D2H later.
    Candidate* d_cand;
    uint32_t* d_count;
    uint32_t cap;
    std::vector<float> g1;        // Lsmooth taps (lib.rs:95)
    std::vector<char> det_done;   // sched[SCHED_DET_BEHIND_LEVEL]: the level's detector was enqueued behind its level kernel already
    std::vector<char> prepared;   // level l's Lsmooth and Lflow have been written by the last diffusion launch of level l - 1 (k_fed_own's epilogue)
    bool head_fused = false;      // k_head took level 0
    float* P(size_t l, int p) const { return r->planes[l][p]; }
    size_t L() const { return r->plan.size(); }
};

// derivatives, Ldet and extrema candidates of level l in one launch on stream `on`; false when the
// level's kernel size has no fused form (then the multi-kernel fallback runs, see detectors)
bool detector_one_pass(BeginState& b, size_t l, hipStream_t on) {
    akz_ctx* c = b.c;
    const LevelPlan& lv = b.r->plan[l];
    const float thr = (float)b.r->cfg.detector_threshold, bm = border_margin(lv, b.r->cfg);
    if (c->settings.profiling) {
        c->prof.det_launches += 1;
        c->prof.det_px += (uint64_t)lv.w * lv.h * b.n;
    }
    const Det det = b.rt.lv[l].det;
    if (det != Det::March && det != Det::NmsFused) return false;
    StageTimer st(c, AKZ_ST_DETECTOR, on);
    if (det == Det::March) st.kernel(AKZ_KR_DETECTOR_MARCH, lv.det_sigma, lv.w, lv.h, b.n, 1, (uint64_t)lv.w * lv.h * b.n);
    (det == Det::March ? launch::detector_march : launch::detector_nms_fused)(
        on, b.P(l, AKZ_LSMOOTH), lv.det_sigma, b.P(l, AKZ_LX), b.P(l, AKZ_LY), b.P(l, AKZ_LXX), b.P(l, AKZ_LYY), b.P(l, AKZ_LXY),
        b.P(l, AKZ_LDET), lv.w, lv.h, b.n, (uint32_t)l, thr, bm, b.d_cand, b.cap, b.d_count);
    return true;
}
// sched[SCHED_DET_BEHIND_LEVEL] (measurement, profiles/r06_interleave.txt): the detector of a fine level right behind the kernel that wrote its
// Lsmooth instead of after the whole fine chain -- does the detector then find (part of) the plane in the Infinity Cache?
void interleave_detector(BeginState& b, size_t l) {
    if (b.c->settings.sched[SCHED_DET_BEHIND_LEVEL] && l < b.rt.fork_level && !b.det_done[l] && b.rt.lv[l].det == Det::March && detector_one_pass(b, l, b.chain.stream)) b.det_done[l] = 1;
}

// ---- level 0: Lt0 = gaussian_blur(img, base_scale_offset); contrast factor (lib.rs:56-69) ----
// Running ahead.  These two stages need nothing but the frames, and the contrast passes are bound by arithmetic, not
// by bandwidth: when the frames are known to be complete -- the caller says so (AKZ_INPUT_READY) or this library
// uploaded them itself (akz_extract_begin_host_*: `input_ready` is the upload's event) -- a large batch enqueues them
// on the context's copy stream, which does NOT wait for what the context's stream still has to do for the batch before,
// and the context's stream picks up behind them.  They then run under the previous batch's detectors instead of in front
// of this batch's first level: 0.3-0.4 ms less on the critical path of a 5 ms step (+3.7 %, 5 x 80 steps each way).
// (place_streams: on the context's stream instead when the copy stream could not be given a hardware queue and
// a pipe of its own.)
// The contrast scratch (c->small) is shared by the jobs of a context: a job's early stages wait for the level-0 stages
// of the job before, on whichever stream those ran (pre_done).  Only with the march kernels (they use no other
// context scratch).
template <typename T>
int level0(BeginState& b, const T* d_imgs, hipEvent_t input_ready) {
    akz_ctx* c = b.c;
    akz_result* r = b.r;
    const akz_config& cfg = r->cfg;
    const uint32_t w = r->w, h = r->h, n = b.n;
    const bool early = b.rt.pre_on != 0;
    JobForm f = b.form;  // (on the early stream where the job runs ahead)
    if (early) {
        Stream& ps = b.rt.pre_on == 2 ? c->copy : c->pre;
        AKZ_TRY(ps.ensure());
        if (input_ready) AKZ_HIP_TRY(hipStreamWaitEvent(ps, input_ready, 0));
        if (c->pre_done) AKZ_HIP_TRY(hipStreamWaitEvent(ps, c->pre_done, 0));
        // however early the caller begins this batch, its first two stages start when the batch before goes from its
        // (VALU-bound) diffusion launches to its (bandwidth-bound) detectors: that is what they are meant to run under
        if (c->settings.sched[SCHED_EARLY_HOLD] && b.seq > 1)
            AKZ_HIP_TRY(hipStreamWaitEvent(ps, (c->settings.sched[SCHED_EARLY_HOLD] == 2 ? c->pre_ev : c->fed_ev)[(b.seq - 1) % akz_ctx::kFedRing], 0));
        f.stream = ps;
    }
    // the job's candidate counter is cleared on the stream of its first stage (every detector launch comes behind that):
    // by that stage's kernel itself where it is k_head, by a fill otherwise
    // (a small job: both stages in two launches -- akz_ops.cpp: head_impl; level 1, where it continues the octave, finds its Lsmooth
    // written -- the contrast factor's blur of Lt0 is the same image -- and the Scharr pair of it in level 0's Lx / Ly planes)
    AKZ_TRY(head_impl<T>(c, f, d_imgs, b.P(0, AKZ_LT), b.rt.level1_clone ? b.P(1, AKZ_LSMOOTH) : nullptr, b.P(0, AKZ_LX), b.P(0, AKZ_LY), w, h, n,
                         (float)cfg.base_scale_offset, cfg.contrast_percentile, 1.0, cfg.contrast_factor_num_bins, r->d_k, &b.head_fused, b.d_count));
    if (!b.head_fused) {
        AKZ_HIP_TRY(hipMemsetAsync(b.d_count, 0, sizeof(uint32_t), f.stream));
        {
            StageTimer st(c, AKZ_ST_BLUR0, f.stream);
            AKZ_TRY(gaussian_blur_impl<T>(c, f, d_imgs, b.P(0, AKZ_LT), w, h, n, (float)cfg.base_scale_offset));
        }
        {
            StageTimer st(c, AKZ_ST_CONTRAST, f.stream);
            AKZ_TRY(contrast_impl(c, f, b.P(0, AKZ_LSMOOTH), w, h, n, cfg.contrast_percentile, 1.0, cfg.contrast_factor_num_bins, r->d_k));
        }
    }
    // every job marks the end of its level-0 stages (the last use of the context's contrast scratch): a later job that
    // runs ahead waits for exactly that, whichever stream it was recorded on
    AKZ_TRY(c->pre_done.ensure());
    AKZ_HIP_TRY(hipEventRecord(c->pre_done, f.stream));
    if (early) AKZ_HIP_TRY(hipStreamWaitEvent(b.form.stream, c->pre_done, 0));
    return AKZ_OK;
}

// all levels from i on (preparation and every diffusion step, across octaves) in one launch
int resident_tail(BeginState& b, size_t i) {
    akz_ctx* c = b.c;
    const std::vector<LevelPlan>& plan = b.r->plan;
    const size_t L = b.L();
    std::vector<launch::ResidentLevel> rl;
    std::vector<std::vector<float>> ht(L);
    uint64_t px_steps = 0;
    for (size_t l = i; l < L; ++l) {
        for (double t : plan[l].tau) ht[l].push_back(0.5f * (float)t);
        rl.push_back(launch::ResidentLevel{b.P(l, AKZ_LT), b.P(l, AKZ_LSMOOTH), b.P(l, AKZ_LFLOW), b.keep_all ? b.P(l, AKZ_LSTEP) : nullptr,
                                           plan[l].w, plan[l].h, plan[l].octave > plan[l - 1].octave,
                                           (uint32_t)plan[l].tau.size(), ht[l].data(), plan[l].octave});
        px_steps += (uint64_t)plan[l].w * plan[l].h * b.n * plan[l].tau.size();
    }
    StageTimer st(c, AKZ_ST_FED, b.chain.stream);
    st.kernel(AKZ_KR_OCTAVE_RESIDENT, (uint32_t)rl.size(), plan[i].w, plan[i].h, b.n, 1, 0, px_steps);
    launch::octave_resident(b.chain.stream, b.P(i - 1, AKZ_LT), plan[i - 1].w, plan[i - 1].h, b.n, rl.data(), (uint32_t)rl.size(), b.g1.data(), b.r->d_k);
    if (c->settings.profiling) {
        c->prof.fed_launches += 1;
        c->prof.fed_px_steps += px_steps;
    }
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

// Large launches of levels that diffuse: preparation and the first (up to four) diffusion steps in ONE launch of
// k_level_march (akz_march.hip) — Lt is read once for both, 4 B read + 12 (+4) B written per pixel instead of
// 12 + 12 (+4); a new octave's 2x2 mean is materialised first.  Remaining steps follow in k_fed_own launches.
// (from 4 Mpx per launch -- the third octave of a 32-frame 1080p batch -- on: one launch less per level in the
// coarse chain that runs next to the fine detectors, +1.0 % throughput, measured 4 x 80 steps each way)
int level_by_march(BeginState& b, size_t i, float* A, float* B) {
    akz_ctx* c = b.c;
    const LevelPlan &lv = b.r->plan[i], &pv = b.r->plan[i - 1];
    const BeginRoute::Level& q = b.rt.lv[i];
    const uint32_t n = b.n, n1 = q.n1, rem = q.rem;
    const bool half = lv.octave > pv.octave;
    const uint32_t rest = rem ? fed_num_launches(c, rem, lv.w, lv.h, n) : 0;
    float* d1 = fed_dst(rest + 1, 1, A, B);
    const float* level_in = b.P(i - 1, AKZ_LT);
    if (half && !q.fold_half) {
        StageTimer st(c, AKZ_ST_PREP, b.chain.stream);
        float* hb = d1 == A ? B : A;
        launch::half_size(b.chain.stream, b.P(i - 1, AKZ_LT), hb, pv.w, pv.h, n);
        level_in = hb;
    }
    float ht[4];
    for (uint32_t j = 0; j < n1; ++j) ht[j] = 0.5f * (float)lv.tau[j];
    {
        StageTimer st(c, AKZ_ST_FED, b.chain.stream);
        st.kernel(AKZ_KR_LEVEL_MARCH, n1 | (q.fold_half ? 16u : 0u) | ((rem == 0 && b.keep_all) ? 32u : 0u), lv.w, lv.h, n, 1,
                  (uint64_t)lv.w * lv.h * n, (uint64_t)lv.w * lv.h * n * n1);
        launch::level_march(b.chain.stream, level_in, b.P(i, AKZ_LSMOOTH), b.P(i, AKZ_LFLOW), d1,
                            (rem == 0 && b.keep_all) ? b.P(i, AKZ_LSTEP) : nullptr, lv.w, lv.h, n, b.g1.data(), b.r->d_k,
                            lv.octave, ht, n1, q.fold_half ? pv.w : 0u, q.fold_half ? pv.h : 0u);
        if (c->settings.profiling) {
            c->prof.fed_launches += 1;
            c->prof.fed_px_steps += (uint64_t)lv.w * lv.h * n * n1;
            c->prof.fused_px += (uint64_t)lv.w * lv.h * n;
        }
    }
    if (rem) {  // (a span of its own: the rows of akz_debug_kernel_rows tell the two kernels apart)
        StageTimer st(c, AKZ_ST_FED, b.chain.stream);
        st.kernel(AKZ_KR_FED_OWN, rem, lv.w, lv.h, n, rest, 0, (uint64_t)lv.w * lv.h * n * rem);
        AKZ_TRY(fed_impl(c, b.chain, d1, A, B, b.P(i, AKZ_LFLOW), b.keep_all ? b.P(i, AKZ_LSTEP) : nullptr, lv.w, lv.h, n, lv.tau.data() + n1, rem));
    }
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

// A level as separate launches: its preparation (unless it came with k_head or rode on the level before), then its diffusion.
// (Preparation + the first eight diffusion steps as ONE tiled launch -- k_prep and k_fed_own fused, tile + halo 8 + 2 --
// was built and measured in round 3: 20 us per launch at best against 6-8 + 8-10 for the pair (the preparation then runs
// on the whole diffusion region, 2.3 x the tile); a lone 1080p frame 0.59 -> 0.86 ms, batches -1 ... -4 %.  Removed.)
int level_by_launches(BeginState& b, size_t i, float* A, float* B) {
    akz_ctx* c = b.c;
    const LevelPlan &lv = b.r->plan[i], &pv = b.r->plan[i - 1];
    const uint32_t n = b.n, n_tau = (uint32_t)lv.tau.size();
    const bool half = lv.octave > pv.octave;
    // FED input: the previous level's final Lt (clone, lib.rs:92, no copy needed) or its 2x2 mean
    // (lib.rs:82) materialised by k_prep into a buffer the first FED launch does not write.
    const float* fed_in = b.P(i - 1, AKZ_LT);
    float* half_buf = nullptr;
    if (half) {
        const uint32_t launches = fed_num_launches(c, n_tau, lv.w, lv.h, n);
        half_buf = launches == 0 ? A : (fed_dst(launches, 1, A, B) == A ? B : A);
        fed_in = half_buf;
    }
    if (i == 1 && b.head_fused && b.rt.level1_clone) {  // Lsmooth is k_head's; Lflow = pm_g2 of the Scharr pair k_head left in level 0's Lx / Ly
        StageTimer st(c, AKZ_ST_PREP, b.chain.stream);
        launch::flow_from_pair(b.chain.stream, b.P(0, AKZ_LX), b.P(0, AKZ_LY), b.P(1, AKZ_LFLOW), lv.w, lv.h, n, b.r->d_k, lv.octave);
    } else if (!b.prepared[i]) {
        StageTimer st(c, AKZ_ST_PREP, b.chain.stream);
        (b.rt.lv[i].prep == Prep::Stream ? launch::prep_stream : launch::prep_fused)(
            b.chain.stream, b.P(i - 1, AKZ_LT), half, half_buf, b.P(i, AKZ_LSMOOTH), b.P(i, AKZ_LFLOW), lv.w, lv.h, pv.w, pv.h, n, b.g1.data(), b.r->d_k, lv.octave);
    }
    if (b.keep_all && n_tau == 0) AKZ_HIP_TRY(hipMemsetAsync(b.P(i, AKZ_LSTEP), 0, plane_bytes(lv.w, lv.h, n), b.chain.stream));
    launch::FedNextPrep np{};
    const bool ride = i + 1 < b.L() && b.rt.lv[i + 1].may_ride;
    if (ride) np = launch::FedNextPrep{b.P(i + 1, AKZ_LSMOOTH), b.P(i + 1, AKZ_LFLOW), b.g1.data(), b.r->d_k, b.r->plan[i + 1].octave};
    bool rode = false;
    StageTimer st(c, AKZ_ST_FED, b.chain.stream);
    st.kernel(AKZ_KR_FED_OWN, n_tau, lv.w, lv.h, n, fed_num_launches(c, n_tau, lv.w, lv.h, n), 0, (uint64_t)lv.w * lv.h * n * n_tau);
    AKZ_TRY(fed_impl(c, b.chain, fed_in, A, B, b.P(i, AKZ_LFLOW), b.keep_all ? b.P(i, AKZ_LSTEP) : nullptr, lv.w, lv.h, n, lv.tau.data(), n_tau,
                     ride ? &np : nullptr, &rode));
    b.prepared[i + 1] = rode ? 1 : 0;
    return AKZ_OK;
}

// ---- levels [lo, hi) of the chain (lib.rs:78-119) on b.chain.stream ----
int run_levels(BeginState& b, size_t lo, size_t hi) {
    akz_ctx* c = b.c;
    const std::vector<LevelPlan>& plan = b.r->plan;
    for (size_t i = lo; i < hi; ++i) {
        if (i >= 2) interleave_detector(b, i - 1);  // (level i - 1 is complete; its Lsmooth was written one launch group ago)
        if (i == b.rt.res_first) return resident_tail(b, i);
        float* A = b.P(i, AKZ_LT);
        const bool on_coarse = i >= b.rt.fork_level;  // the coarse chain has its own ping-pong plane (it outlives the batch's join)
        if (on_coarse) AKZ_TRY(ensure(c, c->scratch_coarse, plane_bytes(plan[b.rt.fork_level].w, plan[b.rt.fork_level].h, b.n)));
        float* B = (float*)(on_coarse ? c->scratch_coarse.p : c->scratch[5].p);
        AKZ_TRY(b.rt.lv[i].prep == Prep::LevelMarch ? level_by_march(b, i, A, B) : level_by_launches(b, i, A, B));
    }
    return AKZ_OK;
}

// One launch per chunk of up to `maxn` levels of a set (levels of one sigma_size); the kernel row carries the shape of the chunk's
// first level (the largest, in a march set).
using DetSetLaunch = void (*)(hipStream_t, uint32_t, const launch::DetLevelDesc*, uint32_t, uint32_t, float, Candidate*, uint32_t, uint32_t*);
void detector_set(BeginState& b, hipStream_t on, DetSetLaunch go, uint32_t maxn, uint32_t kind, uint32_t sigma, const std::vector<launch::DetLevelDesc>& v) {
    akz_ctx* c = b.c;
    for (size_t i = 0; i < v.size(); i += maxn) {
        const uint32_t cnt = (uint32_t)std::min<size_t>(maxn, v.size() - i);
        StageTimer st(c, AKZ_ST_DETECTOR, on);
        if (c->settings.profiling) {
            c->prof.det_launches += 1;
            uint64_t set_px = 0;
            for (size_t j = i; j < i + cnt; ++j) set_px += (uint64_t)v[j].w * v[j].h * b.n;
            c->prof.det_px += set_px;
            st.kernel(kind, sigma, v[i].w, v[i].h, b.n, 1, set_px);
        }
        go(on, sigma, v.data() + i, cnt, b.n, (float)b.r->cfg.detector_threshold, b.d_cand, b.cap, b.d_count);
    }
}

// ---- detectors: levels [lo, hi) on f.stream ----
// The detector of level l needs only Lsmooth_l; its launches follow the whole diffusion chain on the same stream (running them on
// a side stream next to the diffusion was +3 % with the round-1 kernels and is -15 % with the column march, which
// saturates the store path on its own; with only the half-resolution octave's detectors on the side stream it is
// still -5 %: removed).
// levels whose detector is the one-kernel tiled form are grouped by sigma_size: one launch per group
// Column-march levels are grouped the same way (sigma_size and the width's parity, which the kernel is compiled for; the kept planes and
// the extrema test are the job's): one launch per set of up to launch::detector_march_set_max() levels, largest first, when
// sched[SCHED_DET_SETS] asks for it (kDetSetsByDefault: DESIGN.md 4; sched[SCHED_DET_SETS] = 1: one launch per level, 2 / 11 .. 14: sets)
constexpr bool kDetSetsByDefault = true;
int detectors(BeginState& b, size_t lo, size_t hi, const JobForm& f) {
    akz_ctx* c = b.c;
    const akz_config& cfg = b.r->cfg;
    const uint32_t n = b.n;
    const hipStream_t on = f.stream;
    std::map<uint32_t, std::vector<launch::DetLevelDesc>> sets;
    std::map<std::pair<uint32_t, uint32_t>, std::vector<launch::DetLevelDesc>> march_sets;
    const bool by_sets = c->settings.sched[SCHED_DET_SETS] == 0 ? kDetSetsByDefault : c->settings.sched[SCHED_DET_SETS] != 1;
    for (size_t l = lo; l < hi; ++l) {
        if (b.det_done[l]) continue;  // (sched[SCHED_DET_BEHIND_LEVEL]: enqueued behind its level kernel already)
        const LevelPlan& lv = b.r->plan[l];
        const float thr = (float)cfg.detector_threshold, bm = border_margin(lv, cfg);
        const Det det = b.rt.lv[l].det;
        if ((by_sets && det == Det::March) || det == Det::TiledSet) {
            (det == Det::March ? march_sets[{lv.det_sigma, lv.w & 1u}] : sets[lv.det_sigma])
                .push_back(launch::DetLevelDesc{b.P(l, AKZ_LSMOOTH), b.P(l, AKZ_LX), b.P(l, AKZ_LY), b.P(l, AKZ_LXX), b.P(l, AKZ_LYY), b.P(l, AKZ_LXY),
                                                b.P(l, AKZ_LDET), lv.w, lv.h, (uint32_t)l, bm});
            continue;
        }
        if (detector_one_pass(b, l, on)) continue;
        {
            StageTimer st(c, AKZ_ST_DETECTOR, on);
            AKZ_TRY(detector_impl(c, f, b.P(l, AKZ_LSMOOTH), lv.det_sigma, b.P(l, AKZ_LX), b.P(l, AKZ_LY), b.P(l, AKZ_LXX),
                                  b.P(l, AKZ_LYY), b.P(l, AKZ_LXY), b.P(l, AKZ_LDET), lv.w, lv.h, n));
        }
        StageTimer st(c, AKZ_ST_NMS, on);
        launch::nms(on, b.P(l, AKZ_LDET), lv.w, lv.h, n, (uint64_t)lv.w * lv.h, (uint32_t)l, thr, bm, b.d_cand, b.cap, b.d_count);
    }
    for (auto& kv : march_sets) {
        std::vector<launch::DetLevelDesc>& v = kv.second;
        std::stable_sort(v.begin(), v.end(), [](const launch::DetLevelDesc& x, const launch::DetLevelDesc& y) { return (uint64_t)x.w * x.h > (uint64_t)y.w * y.h; });
        detector_set(b, on, launch::detector_march_set, launch::detector_march_set_max(), AKZ_KR_DETECTOR_MARCH, kv.first.first, v);
    }
    for (auto& kv : sets)  // (plan order)
        detector_set(b, on, launch::detector_tiled_set, launch::detector_tiled_set_max(), AKZ_KR_DETECTOR_TILED, kv.first, kv.second);
    return AKZ_OK;
}

// The coarse chain (levels from fork_level on, then their detectors) runs on the second stream; the main stream
// takes the fine detectors.  The JOIN is on the coarse stream: it waits for the fine detectors and records the
// batch's completion, and the main stream goes straight on to the next batch.  (Joined on the main stream, that
// stream sat idle for 0.35-0.5 ms per 32-frame step: next to the bandwidth-bound fine detectors the coarse
// chain's small launches are starved -- HBM latency grows several-fold -- and finish well after them.  Now that
// tail runs under the next batch's level-0 kernels; the chain has its own diffusion scratch, and the chains of
// consecutive batches follow each other on one stream.)
// *done_on: the stream behind whose work the batch's candidate list is complete
int fork_and_join(BeginState& b, hipStream_t* done_on) {
    akz_ctx* c = b.c;
    const hipStream_t s = b.form.stream;
    AKZ_TRY(c->coarse.ensure());
    Event fine_done = StageTimer::get(c);
    AKZ_HIP_TRY(hipEventRecord(fine_done, s));
    AKZ_HIP_TRY(hipStreamWaitEvent(c->coarse, fine_done, 0));
    ev_put(c, std::move(fine_done));
    // (holding the chain back until the full-resolution detectors, or all fine detectors, have finished: -2 ... -5 %)
    // The fine detectors are ENQUEUED first: the coarse chain is dozens of small launches, and a caller that is not
    // ahead of the chip -- one synchronous call on a 4K pair -- kept the main stream idle for the 0.19 ms it took to
    // enqueue them (the two streams run side by side either way).
    AKZ_TRY(detectors(b, 0, b.rt.fork_level, b.form));
    b.chain.stream = c->coarse;
    AKZ_TRY(run_levels(b, b.rt.fork_level, b.L()));
    AKZ_TRY(detectors(b, b.rt.fork_level, b.L(), b.chain));
    Event ev = StageTimer::get(c);
    if (b.rt.own_kernels) {
        AKZ_HIP_TRY(hipEventRecord(ev, s));
        AKZ_HIP_TRY(hipStreamWaitEvent(c->coarse, ev, 0));
        *done_on = c->coarse;
    } else {  // the multi-kernel detector fallback borrows context scratch planes: then join on the main stream
        AKZ_HIP_TRY(hipEventRecord(ev, c->coarse));
        AKZ_HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    }
    ev_put(c, std::move(ev));
    return AKZ_OK;
}

// the slab of a begin half: per level Lt, Lsmooth, Lx, Ly, Ldet, Lflow, and with AKZ_KEEP_ALL_PLANES the rest
std::vector<std::pair<uint32_t, int>> begin_planes(size_t L, bool keep_all) {
    static const int kOrder[10] = {AKZ_LT, AKZ_LSMOOTH, AKZ_LX, AKZ_LY, AKZ_LDET, AKZ_LFLOW, AKZ_LXX, AKZ_LYY, AKZ_LXY, AKZ_LSTEP};
    std::vector<std::pair<uint32_t, int>> want;
    for (uint32_t l = 0; l < L; ++l)
        for (int k = 0; k < (keep_all ? 10 : 6); ++k) {
            const int p = kOrder[k];
            // level 0: Lsmooth is a clone of Lt (lib.rs:58) -> alias; it has no Lflow / Lstep
            if (l > 0 || (p != AKZ_LSMOOTH && p != AKZ_LFLOW && p != AKZ_LSTEP)) want.emplace_back(l, p);
        }
    return want;
}
}  // namespace

int mask_enqueue(akz_ctx* c, hipStream_t s, const akz_result* r, const MaskSpec& m, int slot, uint32_t cap, uint32_t* d_count) {
    const uint32_t L = (uint32_t)r->plan.size();
    uint32_t lw[kMaxLevels], lh[kMaxLevels], lo[kMaxLevels];
    for (uint32_t l = 0; l < L && l < (uint32_t)kMaxLevels; ++l) lw[l] = r->plan[l].w, lh[l] = r->plan[l].h, lo[l] = r->plan[l].octave;
    StageTimer st(c, AKZ_ST_NMS, s);
    st.kernel(AKZ_KR_MASK_CANDIDATES, m.frame_stride ? r->n : 1u, r->w, r->h, r->n, 1, cap);
    launch::mask_candidates(s, (const Candidate*)c->cand_slot[slot].p, (Candidate*)c->cand_mask_slot[slot].p, cap, d_count, m.d, m.row_pitch,
                            m.frame_stride, lw, lh, lo, L, r->n);
    AKZ_HIP_TRY(hipGetLastError());
    return AKZ_OK;
}

// open -> route -> level 0 -> fine levels -> pre_ev / fed_ev -> fork or not -> nms_done
template <typename T>
int extract_begin(akz_ctx* c, const T* d_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfgp, uint32_t flags, akz_job** out,
                  int want_slot, hipEvent_t input_ready, bool sync_call, const MaskSpec* mask) {
    if (!out) return AKZ_ERR_INVALID_ARG;
    *out = nullptr;
    AKZ_TRY(bind(c, true, c && c->is_lane));  // (a lane's finish half shares the lane's one stream: begin waits for it)
    const uint64_t big_px = sync_call ? c->settings.big_px_sync : c->settings.big_px_async;  // (akz_gates.hpp)
    if (!d_imgs || !cfgp || n == 0) {
        set_error("extract: null image/config or empty batch");
        return AKZ_ERR_INVALID_ARG;
    }
    JobOpening o;
    o.drain_side = true;
    AKZ_TRY(job_open(c, "extract_begin", want_slot, w, h, n, flags, *cfgp, o));
    akz_job* job = o.job.get();
    akz_result* r = job->r.get();
    r->big_px = big_px;  // (the finish half may run on another thread while the next job is begun with another gate)
    const size_t L = r->plan.size();
    const bool keep_all = (flags & AKZ_KEEP_ALL_PLANES) != 0;
    const hipStream_t s = c->stream;
    AKZ_TRY(job_layout(o, begin_planes(L, keep_all)));

    job->t_begin_ms = now_ms();
    uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)n * std::max<uint32_t>(c->cand_cap_hint.load(), 16u),
                                                0x7fffffffull / sizeof(Candidate));
    // A job like the one before it (same shape) whose list was short gets a list no longer than the one-launch sort takes
    // (launch::sort_small_capacity): should this image have more candidates after all, the overflow path of the finish half
    // redoes the extrema with room for them.
    {
        const uint32_t last = c->last_total_cands.load();
        if (c->last_cand_shape.load() == shape_key(w, h, n) && last > 0 && (uint64_t)last * 5 / 4 + 64 <= launch::sort_small_capacity())
            cap = std::min(cap, launch::sort_small_capacity());
    }
    AKZ_TRY(ensure(c, c->cand_slot[o.slot], (size_t)cap * sizeof(Candidate)));
    AKZ_TRY(ensure(c, c->count_slot[o.slot], 256));
    if (mask) AKZ_TRY(ensure(c, c->cand_mask_slot[o.slot], (size_t)cap * sizeof(Candidate)));
    for (Event& e : c->fed_ev) AKZ_TRY(e.ensure());
    for (Event& e : c->pre_ev) AKZ_TRY(e.ensure());
    const uint64_t seq = c->begin_seq.load() + 1;  // published when this job's event has been recorded
    // Jobs below gates::kTiledPrepPx take the TILED preparation family whatever their launches' sizes -- k_blur, k_contrast_max /
    // _hist, k_prep riding on the previous level's last k_fed_own launch, no resident tail: since that epilogue exists the
    // chain of few-microsecond launches beats the streaming kernels and k_level_march up to ~11 Mpx per job (akz_gates.hpp: kTiledPrepPx; profiles/
    // r06_lone_libm.txt: 2-6 x 1080p, 4-8 x 720p, lone 2-5 Mpx frames 3-9 % faster per call, 0-9 % as a stream).  Only the
    // automatic mode 2 is overridden.  A batch-path job marches from its own size on (JobForm::march_min_px).
    const uint64_t job_px = (uint64_t)w * h * n;
    const bool big = job_px >= big_px;
    const bool tiled_family = c->settings.prep_mode == 2 && c->settings.sched[SCHED_PREP_OWN_LAUNCH] == 0 && job_px < gates::kTiledPrepPx;
    const JobForm form{s, tiled_family ? 0 : c->settings.prep_mode, big ? std::min<uint64_t>(gates::kMarchPx, job_px) : gates::kMarchPx};
    if (big && !c->placed) AKZ_TRY(place_streams(c));
    const BeginRoute rt = begin_route(c, form, r->plan, r->cfg, w, h, n, flags, input_ready != nullptr, big);
    BeginState b{c, r, rt, n, keep_all, form, form, seq, (Candidate*)c->cand_slot[o.slot].p, (uint32_t*)c->count_slot[o.slot].p, cap,
                 {}, std::vector<char>(L, 0), std::vector<char>(L + 1, 0)};

    AKZ_TRY(level0<T>(b, d_imgs, input_ready));
    // ---- levels 1..L-1 ----
    AKZ_TRY(ensure(c, c->scratch[5], plane_bytes(w, h, n)));
    b.g1 = gaussian_kernel(1.0f, gaussian_kernel_size(1.0f));
    // (A small job's first-octave detectors on a second stream, under the remaining octaves' chain of small launches, was built
    // and measured three times in round 6.  With the persistent detector launches: lone 1080p call 0.795 / 0.799 ms with /
    // without, 720p 0.634 / 0.620 -- persistent workgroups hold their compute units until the launch ends and the chain's
    // launches wait for places.  With one tile per workgroup on a lowest-priority stream the two do run side by side -- under
    // rocprofv3 the begin chain ends 40 us earlier -- but unprofiled, where the chain's launches follow each other without the
    // profiler's gaps, there is nothing to fill: 0.745-0.751 / 0.749-0.750 ms, 720p 0.588 / 0.576.  On a stream with a CU mask
    // (hipExtStreamCreateWithCUMask: 64 / 128 / 192 of the 256 compute units): 0.730 / 0.690 / 0.670 against 0.682 without, a
    // stream of frames 0.57 / 0.54 / 0.514 against 0.519, 720p 0.54 against 0.53.  Not kept.)
    // the fine levels (all levels when the batch does not fork) on the main stream
    AKZ_TRY(run_levels(b, 1, rt.oct1));
    AKZ_HIP_TRY(hipEventRecord(c->pre_ev[seq % akz_ctx::kFedRing], s));
    AKZ_TRY(run_levels(b, rt.oct1, rt.fork_level));
    // The keypoint kernels of the batch that is finished next (orientation, M-LDB: gather-bound, on the auxiliary
    // stream) wait for this point: next to the VALU-bound diffusion launches they cost more than next to the
    // bandwidth-bound detector launches that follow, and the diffusion launches stay individually timeable.
    AKZ_HIP_TRY(hipEventRecord(c->fed_ev[seq % akz_ctx::kFedRing], s));
    c->begin_seq.store(seq);

    hipStream_t done_on = s;
    if (rt.fork_level < L) AKZ_TRY(fork_and_join(b, &done_on));
    else AKZ_TRY(detectors(b, 0, L, form));
    AKZ_HIP_TRY(hipGetLastError());
    // The detection mask: the list every consumer reads -- the three sorts, k_relations, k_select, the speculative fetches, the host's
    // selection -- is what the mask keeps of it, made behind the last detector and in front of the job's event.  (The mask may be the
    // output of work queued earlier on the caller's stream: this point lies far behind the frames' own wait.)
    if (mask) {
        AKZ_TRY(mask_enqueue(c, done_on, r, *mask, o.slot, cap, b.d_count));
        job->mask = *mask;
    }
    job->nms_done = StageTimer::get(c);
    AKZ_HIP_TRY(hipEventRecord(job->nms_done, done_on));
    job->done_stream = done_on;
    job->seq = seq;
    *out = o.keep(cap);
    return AKZ_OK;
}
template int extract_begin<uint8_t>(akz_ctx*, const uint8_t*, uint32_t, uint32_t, uint32_t, const akz_config*, uint32_t, akz_job**, int, hipEvent_t, bool, const MaskSpec*);
template int extract_begin<float>(akz_ctx*, const float*, uint32_t, uint32_t, uint32_t, const akz_config*, uint32_t, akz_job**, int, hipEvent_t, bool, const MaskSpec*);
