// C ABI of libakaze_hip.so, part 3: extract_features -- the C entry points over the two halves (akz_extract_begin.cpp,
// akz_extract_finish.cpp), caller-provided evolutions, lanes and the finisher thread, gate calibration, the graph probe.
#include "akz_extract.hpp"

static int extract_finish(akz_job* jobp, akz_result** out) {
    if (!jobp || !out) return AKZ_ERR_INVALID_ARG;
    *out = nullptr;
    int rc;
    if (jobp->fin) {  // finished (or being finished) by its lane's thread
        job_wait(jobp);
        rc = jobp->rc;
        *out = jobp->out;
        if (rc != AKZ_OK) set_error(jobp->err);
    } else {
        rc = extract_finish_body(jobp, out);
    }
    delete jobp;
    return rc;
}
static void finisher_loop(akz_ctx* c, Finisher* f) {
    (void)hipSetDevice(c->device);
    for (;;) {
        akz_job* j = nullptr;
        {
            std::unique_lock<std::mutex> lk(f->m);
            f->wake.wait(lk, [&] { return f->quit || !f->queue.empty(); });
            if (f->queue.empty()) return;  // quit is only set with nothing in flight
            j = f->queue.front();
            f->queue.erase(f->queue.begin());
        }
        akz_result* res = nullptr;
        int rc;
        try {
            rc = extract_finish_body(j, &res);
        } catch (const std::exception& e) {  // (allocation failure on this thread must not take the process down)
            set_error(std::string("extract_finish: ") + e.what());
            rc = AKZ_ERR_NO_MEMORY;
            res = nullptr;
        }
        std::string err = rc != AKZ_OK ? get_error() : std::string();
        {
            std::lock_guard<std::mutex> lk(f->m);
            j->rc = rc;
            j->out = res;
            j->err.swap(err);
            j->finished = true;
            --f->in_flight;
        }
        f->done.notify_all();
    }
}
static void finisher_post(akz_ctx* lane, akz_job* j) {
    if (!lane->fin) {
        lane->fin.reset(new Finisher);
        Finisher* f = lane->fin.get();
        f->th = std::thread([lane, f] { finisher_loop(lane, f); });
    }
    Finisher* f = lane->fin.get();
    {
        std::lock_guard<std::mutex> lk(f->m);
        j->fin = lane->fin;
        f->queue.push_back(j);
        ++f->in_flight;
    }
    f->wake.notify_one();
}

// `pub mod ops` on CALLER-PROVIDED evolutions (ops::scale_space_extrema::detect_keypoints, scale_space_extrema.rs:199-203,
// and ops::descriptors::extract_descriptors, descriptors.rs:14-27, take a `Vec<EvolutionStep>` that the caller may have
// built or modified itself): the host planes of one image are uploaded into a result's slab, the extrema pass runs on
// the uploaded Ldet planes and the usual finish half (host keypoint logic, orientation, descriptors) follows.
static int extract_from_planes(akz_ctx* c, uint32_t w, uint32_t h, const akz_config* cfgp, const float* const* planes,
                               uint64_t n_levels, uint32_t flags, akz_result** out) {
    if (!out) return AKZ_ERR_INVALID_ARG;
    *out = nullptr;
    AKZ_TRY(bind(c));
    if (!cfgp || !planes) {
        set_error("extract_from_planes: null config / plane table");
        return AKZ_ERR_INVALID_ARG;
    }
    JobOpening o;
    AKZ_TRY(job_open(c, "extract_from_planes", -1, w, h, 1, (flags & ~(uint32_t)AKZ_NO_DETECT) | AKZ_KEEP_ALL_PLANES, *cfgp, o));
    akz_job* job = o.job.get();
    akz_result* r = job->r.get();
    const std::vector<LevelPlan>& plan = r->plan;
    const size_t L = plan.size();
    if (n_levels != L) {
        set_error("extract_from_planes: the number of evolutions does not match allocate_evolutions(width, height, options)");
        return AKZ_ERR_INVALID_ARG;
    }
    const bool detect = !(flags & AKZ_NO_DETECT);
    for (size_t l = 0; l < L; ++l)
        for (int p : {(int)AKZ_LT, (int)AKZ_LX, (int)AKZ_LY, (int)AKZ_LDET})
            if (!planes[l * 10 + p] && (detect || p != AKZ_LDET)) {
                set_error("extract_from_planes: Lt, Lx, Ly (and Ldet for detection) of every evolution are required");
                return AKZ_ERR_INVALID_ARG;
            }
    hipStream_t s = c->stream;
    std::vector<std::pair<uint32_t, int>> wanted;
    for (uint32_t l = 0; l < L; ++l)
        for (int p = 0; p < 10; ++p)
            if (planes[l * 10 + p]) wanted.emplace_back(l, p);
    AKZ_TRY(job_layout(o, wanted));
    job->t_begin_ms = now_ms();
    AKZ_HIP_TRY(hipMemsetAsync(r->d_k, 0, sizeof(double), s));  // the contrast factor is not part of the inputs
    for (size_t l = 0; l < L; ++l)
        for (int p = 0; p < 10; ++p)
            if (planes[l * 10 + p] && r->planes[l][p] && !(l == 0 && p == AKZ_LSMOOTH && r->planes[0][AKZ_LSMOOTH] == r->planes[0][AKZ_LT]))
                AKZ_HIP_TRY(hipMemcpyAsync(r->planes[l][p], planes[l * 10 + p], plane_bytes(plan[l].w, plan[l].h, 1),
                                           hipMemcpyHostToDevice, s));
    AKZ_HIP_TRY(hipStreamSynchronize(s));  // the caller's planes are pageable host memory: complete before returning
    const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)std::max<uint32_t>(c->cand_cap_hint.load(), 16u), 0x7fffffffull / sizeof(Candidate));
    AKZ_TRY(ensure(c, c->cand_slot[o.slot], (size_t)cap * sizeof(Candidate)));
    AKZ_TRY(ensure(c, c->count_slot[o.slot], 256));
    uint32_t* d_count = (uint32_t*)c->count_slot[o.slot].p;
    AKZ_HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), s));
    if (detect)
        for (size_t l = 0; l < L; ++l)
            launch::nms(s, r->planes[l][AKZ_LDET], plan[l].w, plan[l].h, 1, (uint64_t)plan[l].w * plan[l].h, (uint32_t)l,
                        (float)r->cfg.detector_threshold, border_margin(plan[l], r->cfg), (Candidate*)c->cand_slot[o.slot].p, cap,
                        d_count);
    AKZ_HIP_TRY(hipGetLastError());
    job->nms_done = StageTimer::get(c);
    AKZ_HIP_TRY(hipEventRecord(job->nms_done, s));
    return extract_finish(o.keep(cap), out);
}

template <typename T>
static int extract_impl(akz_ctx* c, const T* d_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfgp,
                        uint32_t flags, akz_result** out, const MaskSpec* mask = nullptr) {
    if (!out) return AKZ_ERR_INVALID_ARG;
    *out = nullptr;
    akz_job* job = nullptr;
    AKZ_TRY(extract_begin<T>(c, d_imgs, w, h, n, cfgp, flags, &job, -1, nullptr, /*sync_call=*/true, mask));
    return extract_finish(job, out);
}

template <typename T>
static int extract_host(akz_ctx* c, const T* img, uint32_t w, uint32_t h, const akz_config* cfg, uint32_t flags,
                        akz_result** out, const uint8_t* host_mask = nullptr) {
    AKZ_TRY(bind(c));
    if (!img || w == 0 || h == 0) {
        set_error("extract: null or empty image");
        return AKZ_ERR_INVALID_ARG;
    }
    const size_t bytes = (size_t)w * h * sizeof(T);
    AKZ_TRY(ensure(c, c->scratch[4], bytes));
    MaskSpec mask;
    if (host_mask) {  // w * h bytes, tight: uploaded behind the frame; the call is synchronous, so the one buffer serves
        AKZ_TRY(ensure(c, c->mask_up, (size_t)w * h));
        AKZ_HIP_TRY(hipMemcpyAsync(c->mask_up.p, host_mask, (size_t)w * h, hipMemcpyHostToDevice, c->stream));
        mask = MaskSpec{(const uint8_t*)c->mask_up.p, w, 0};
    }
    AKZ_HIP_TRY(hipMemcpyAsync(c->scratch[4].p, img, bytes, hipMemcpyHostToDevice, c->stream));
    // the frame is consumed by level 0 on the same stream before anything else touches scratch[4]
    return extract_impl<T>(c, (const T*)c->scratch[4].p, w, h, 1, cfg, flags, out, host_mask ? &mask : nullptr);
}

extern "C" {

int akz_extract_gray_u8(akz_ctx* c, const uint8_t* img, uint32_t w, uint32_t h, const akz_config* cfg, uint32_t flags,
                        akz_result** out) {
    return extract_host<uint8_t>(c, img, w, h, cfg, flags, out);
}
int akz_extract_gray_u8_masked(akz_ctx* c, const uint8_t* img, const uint8_t* mask, uint32_t w, uint32_t h, const akz_config* cfg, uint32_t flags,
                               akz_result** out) {
    if (out) *out = nullptr;
    if (!mask) {
        set_error("akz_extract_gray_u8_masked: null mask");
        return AKZ_ERR_INVALID_ARG;
    }
    return extract_host<uint8_t>(c, img, w, h, cfg, flags, out, mask);
}
int akz_extract_gray_f32(akz_ctx* c, const float* img, uint32_t w, uint32_t h, const akz_config* cfg, uint32_t flags,
                         akz_result** out) {
    return extract_host<float>(c, img, w, h, cfg, flags, out);
}
int akz_extract_device_u8(akz_ctx* c, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                          const akz_config* cfg, uint32_t flags, akz_result** out) {
    return extract_impl<uint8_t>(c, d_imgs, w, h, n, cfg, flags, out);
}
int akz_extract_device_f32(akz_ctx* c, const float* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                           const akz_config* cfg, uint32_t flags, akz_result** out) {
    return extract_impl<float>(c, d_imgs, w, h, n, cfg, flags, out);
}

// lanes = 1 (default): every job runs on the context's own stream.  lanes = k > 1: jobs below gates::kLanePx are dealt to k child
// contexts in turn (larger jobs fill the chip on their own and stay on the context).  A job's result belongs to the
// lane it ran on; nothing else changes for the caller (same begin / finish / result calls, bit-identical results).
int akz_ctx_set_lanes(akz_ctx* c, uint32_t lanes) {
    AKZ_TRY(bind(c));
    if (lanes < 1 || lanes > 8) return AKZ_ERR_INVALID_ARG;
    const size_t want = lanes == 1 ? 0 : lanes;
    // a lane that goes away must have no extraction in flight: its job would be finished on destroyed streams
    for (size_t i = want; i < c->lanes.size(); ++i) {
        for (int k = 0; k < akz_ctx::kSlots; ++k)
            if (c->lanes[i]->slot_busy[k]) {
                set_error("akz_ctx_set_lanes: a lane that would be removed has an extraction in flight (finish or abandon it first)");
                return AKZ_ERR_INVALID_ARG;
            }
    }
    while (c->lanes.size() > want) {
        AKZ_TRY(akz_ctx_destroy(c->lanes.back()));
        c->lanes.pop_back();
    }
    while (c->lanes.size() < want) {
        Stream st;  // (the lane's own)
        AKZ_TRY(st.ensure());
        akz_ctx* l = nullptr;
        AKZ_TRY(akz_ctx_create(c->device, nullptr, &l));
        l->stream = std::move(st);
        l->is_lane = true;
        l->cand_cap_hint = c->cand_cap_hint.load();
        c->lanes.push_back(l);
    }
    push_settings(c);
    c->next_lane = 0;
    return place_lanes(c);
}
// on != 0: the finish half of every job that is dealt to a lane starts on the lane's own thread as soon as the job has
// been begun; akz_extract_finish waits for it and hands the result over (bit-identical; errors of the finish half are
// reported there as before).  Jobs that stay on the context itself (no lanes, or batch-path jobs) are not affected.
int akz_ctx_set_eager_finish(akz_ctx* c, int on) {
    AKZ_TRY(bind(c));
    c->eager_finish = on != 0;
    return AKZ_OK;
}
// `frames`: imgs are device frames in that layout (u8), converted to luma into the job's staging buffer.  sync_call: the
// begin half of a synchronous call -- on the context itself, finished by the caller right away (extract_impl's form).
static int extract_begin_dispatch(akz_ctx* c, const void* imgs, bool is_u8, uint32_t w, uint32_t h, uint32_t n,
                                  const akz_config* cfg, uint32_t flags, akz_job** out, bool on_host = false,
                                  const FrameSpec* frames = nullptr, bool sync_call = false, const MaskSpec* mask = nullptr) {
    akz_ctx* on = c;
    if (!sync_call && c && !c->lanes.empty() && (uint64_t)w * h * n < c->settings.lane_px) {
        AKZ_TRY(bind(c, false));
        on = c->lanes[c->next_lane++ % c->lanes.size()];
        // the lane starts when the caller's stream has reached this point (its inputs are complete)
        AKZ_TRY(c->lane_in.ensure());
        AKZ_HIP_TRY(hipEventRecord(c->lane_in, c->stream));
        AKZ_HIP_TRY(hipStreamWaitEvent(on->stream, c->lane_in, 0));
    }
    int slot = -1;
    const void* d_imgs = imgs;
    hipEvent_t ready = nullptr;  // frames this library put into the staging buffer on the copy stream: complete behind that event
    if (on_host || frames) {
        // Frames in host memory, or device frames in a layout of the caller's: they go into the staging buffer of the job
        // slot this extraction will hold (exclusive until its finish or abandon, so jobs in flight never share one).
        // Host frames are uploaded on the context's copy stream; only this job's kernels wait for the copy, so it runs
        // under whatever the main stream is doing for the batch before.  Device frames are converted to luma
        // (k_frame_luma): with AKZ_INPUT_READY on the copy stream in exactly that shape; without it they may be the
        // output of work queued earlier on the caller's stream, so the conversion goes on the job's main stream (a lane's:
        // behind the lane_in wait above) and no event is handed down.
        if (out) *out = nullptr;
        AKZ_TRY(bind(on, true, on->is_lane));
        if (!imgs || w == 0 || h == 0 || n == 0) {
            set_error("extract_begin_host: null or empty frames");
            return AKZ_ERR_INVALID_ARG;
        }
        slot = free_slot(on);
        if (slot < 0) {
            set_error("extract_begin: too many extractions in flight on this context (finish one first)");
            return AKZ_ERR_INVALID_ARG;
        }
        const size_t bytes = (size_t)w * h * n * (is_u8 ? 1 : sizeof(float));
        AKZ_TRY(ensure(on, on->stage[slot], bytes));
        const bool on_copy = on_host || (flags & AKZ_INPUT_READY);
        if (on_copy) {
            AKZ_TRY(on->copy.ensure());
            AKZ_TRY(on->staged[slot].ensure());
        }
        if (on_host) AKZ_HIP_TRY(hipMemcpyAsync(on->stage[slot].p, imgs, bytes, hipMemcpyHostToDevice, on->copy));
        else AKZ_TRY(frames_enqueue(on, on_copy ? on->copy.h : on->stream.h, (const uint8_t*)imgs, *frames, n, (uint8_t*)on->stage[slot].p));
        if (on_copy) {
            AKZ_HIP_TRY(hipEventRecord(on->staged[slot], on->copy));
            AKZ_HIP_TRY(hipStreamWaitEvent(on->stream, on->staged[slot], 0));
            ready = on->staged[slot].h;
        }
        if (frames) flags &= ~(uint32_t)AKZ_INPUT_READY;  // (the promise was about the caller's frames; the luma frames are complete behind `ready`)
        d_imgs = on->stage[slot].p;
    }
    // (a mask travels with the job: on a lane its filter runs on the lane's stream, behind the lane_in wait above)
    const int rc = is_u8 ? extract_begin<uint8_t>(on, (const uint8_t*)d_imgs, w, h, n, cfg, flags, out, slot, ready, sync_call, mask)
                         : extract_begin<float>(on, (const float*)d_imgs, w, h, n, cfg, flags, out, slot, ready, sync_call, mask);
    // a job dealt to a lane is always finished by the lane's own thread (lanes whose jobs wait for the caller's finish call
    // measured SLOWER than no lanes: the chains overlap on the chip but the finish halves queue on one host thread)
    if (rc == AKZ_OK && !sync_call && (c->eager_finish || on != c)) finisher_post(on, *out);
    return rc;
}
}  // extern "C"
// akz_extract_device_frames / akz_extract_begin_device_frames (akz_frames_api.cpp, which has checked the layout)
int extract_begin_frames(akz_ctx* c, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, const akz_config* cfg, uint32_t flags, akz_job** out,
                         const MaskSpec* mask) {
    if (fs.packed_gray()) return extract_begin_dispatch(c, d_src, true, fs.w, fs.h, n, cfg, flags, out, false, nullptr, false, mask);  // already what the extraction takes
    return extract_begin_dispatch(c, d_src, true, fs.w, fs.h, n, cfg, flags, out, false, &fs, false, mask);
}
int extract_frames(akz_ctx* c, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, const akz_config* cfg, uint32_t flags, akz_result** out,
                   const MaskSpec* mask) {
    if (fs.packed_gray()) return extract_impl<uint8_t>(c, d_src, fs.w, fs.h, n, cfg, flags, out, mask);
    akz_job* job = nullptr;
    AKZ_TRY(extract_begin_dispatch(c, d_src, true, fs.w, fs.h, n, cfg, flags & ~(uint32_t)AKZ_INPUT_READY, &job, false, &fs, /*sync_call=*/true, mask));
    return extract_finish(job, out);
}
extern "C" {
int akz_extract_begin_host_u8(akz_ctx* c, const uint8_t* h_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfg,
                              uint32_t flags, akz_job** out) {
    return extract_begin_dispatch(c, h_imgs, true, w, h, n, cfg, flags, out, true);
}
int akz_extract_begin_host_f32(akz_ctx* c, const float* h_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfg,
                               uint32_t flags, akz_job** out) {
    return extract_begin_dispatch(c, h_imgs, false, w, h, n, cfg, flags, out, true);
}
int akz_extract_begin_device_u8(akz_ctx* c, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                                const akz_config* cfg, uint32_t flags, akz_job** out) {
    return extract_begin_dispatch(c, d_imgs, true, w, h, n, cfg, flags, out);
}
int akz_extract_begin_device_f32(akz_ctx* c, const float* d_imgs, uint32_t w, uint32_t h, uint32_t n,
                                 const akz_config* cfg, uint32_t flags, akz_job** out) {
    return extract_begin_dispatch(c, d_imgs, false, w, h, n, cfg, flags, out);
}
int akz_extract_finish(akz_job* job, akz_result** out) { return extract_finish(job, out); }

// The job gates from timings on this machine (akaze_hip_debug.h).  Five lone frames; each through the synchronous call and
// through the begin / finish interface with two jobs in flight, with the batch path forced off (gate above every size) and
// on (gate 0); medians of kReps.  A gate = the smallest size from which the batch path wins at that size and every larger one.
int akz_ctx_calibrate_gates(akz_ctx* c, uint64_t* sync_px, uint64_t* async_px, double* ms_out) {
    AKZ_TRY(bind(c));
    static const uint32_t kShapes[5][2] = {{1280, 720}, {1600, 900}, {1920, 1080}, {2688, 1512}, {3840, 2160}};  // (0.9 .. 8.3 Mpx: both sides of the gates)
    constexpr int kReps = 5;
    akz_config cfg;
    akz_config_default(&cfg);
    const uint64_t keep_sync = c->settings.big_px_sync, keep_async = c->settings.big_px_async;
    struct Restore {
        akz_ctx* c;
        uint64_t s, a;
        bool armed = true;
        ~Restore() { if (armed) { c->settings.big_px_sync = s; c->settings.big_px_async = a; } }
    } restore{c, keep_sync, keep_async};
    double ms[5][4];
    auto median = [](std::vector<double>& v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    for (int si = 0; si < 5; ++si) {
        const uint32_t w = kShapes[si][0], h = kShapes[si][1];
        std::vector<uint8_t> frame((size_t)w * h);
        AKZ_TRY(akz_synth_frame_u8(frame.data(), w, h, 0, 0, 0));
        void* d = nullptr;
        AKZ_TRY(akz_device_malloc(c, frame.size(), &d));
        struct Free { akz_ctx* c; void* d; ~Free() { (void)akz_device_free(c, d); } } fr{c, d};
        AKZ_TRY(akz_memcpy_h2d(c, d, frame.data(), frame.size()));
        for (int path = 0; path < 2; ++path) {
            c->settings.big_px_sync = c->settings.big_px_async = path ? 0 : ~0ull;
            // synchronous call
            std::vector<double> t;
            for (int r = 0; r < kReps + 1; ++r) {
                akz_result* res = nullptr;
                const double t0 = now_ms();
                AKZ_TRY(akz_extract_device_u8(c, (const uint8_t*)d, w, h, 1, &cfg, AKZ_NO_HOST_DESCRIPTORS, &res));
                if (r) t.push_back(now_ms() - t0);  // (the first call of a shape allocates)
                akz_result_free(res);
            }
            ms[si][path] = median(t);
            // begin / finish with two jobs in flight: time per frame in steady state
            t.clear();
            akz_job* jobs[2] = {nullptr, nullptr};
            AKZ_TRY(akz_extract_begin_device_u8(c, (const uint8_t*)d, w, h, 1, &cfg, AKZ_NO_HOST_DESCRIPTORS | AKZ_INPUT_READY, &jobs[0]));
            double last = now_ms();
            for (int r = 0; r < 2 * kReps + 2; ++r) {
                akz_job* next = nullptr;
                int st = akz_extract_begin_device_u8(c, (const uint8_t*)d, w, h, 1, &cfg, AKZ_NO_HOST_DESCRIPTORS | AKZ_INPUT_READY, &next);
                akz_result* res = nullptr;
                if (st == AKZ_OK) st = akz_extract_finish(jobs[0], &res);
                else (void)akz_job_abandon(jobs[0]);
                if (st != AKZ_OK) {
                    if (next) (void)akz_job_abandon(next);
                    return st;
                }
                akz_result_free(res);
                jobs[0] = next;
                const double now = now_ms();
                if (r >= 2) t.push_back(now - last);
                last = now;
            }
            akz_result* res = nullptr;
            AKZ_TRY(akz_extract_finish(jobs[0], &res));
            akz_result_free(res);
            ms[si][2 + path] = median(t);
        }
    }
    auto gate = [&](int lone, int batch) -> uint64_t {
        int first = 5;  // smallest index from which the batch path wins everywhere above
        for (int si = 4; si >= 0 && ms[si][batch] < ms[si][lone]; --si) first = si;
        return first == 5 ? (uint64_t)kShapes[4][0] * kShapes[4][1] + 1 : (uint64_t)kShapes[first][0] * kShapes[first][1];
    };
    restore.armed = false;
    c->settings.big_px_sync = gate(0, 1);
    c->settings.big_px_async = gate(2, 3);
    push_settings(c);
    if (sync_px) *sync_px = c->settings.big_px_sync;
    if (async_px) *async_px = c->settings.big_px_async;
    if (ms_out)
        for (int si = 0; si < 5; ++si)
            for (int k = 0; k < 4; ++k) ms_out[si * 4 + k] = ms[si][k];
    return AKZ_OK;
}
// Measurement hook (bench.py `single_frame.graph`): is a lone frame's begin phase — a chain of ~45 dependent
// launches — shorter as ONE hipGraph launch?  The begin phase of (d_imgs, w, h, n, cfg) is stream-captured into a
// graph (same kernels, same buffers), then `reps` graph launches and `reps` plain enqueues of the same chain are
// timed from an idle stream with HIP events.  Results of the captured chain are discarded.
int akz_ctx_graph_probe(akz_ctx* c, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfg,
                        uint32_t flags, uint32_t reps, double* ms_graph, double* ms_plain, uint64_t* graph_nodes) {
    AKZ_TRY(bind(c));
    if (!d_imgs || !cfg || !ms_graph || !ms_plain || reps == 0) return AKZ_ERR_INVALID_ARG;
    if ((uint64_t)w * h * n >= c->settings.big_px_async) {  // such a batch forks its coarse chain and completes on that stream: not one capture
        set_error("akz_ctx_graph_probe: jobs that take the batch path fork onto a second stream and cannot be captured from one");
        return AKZ_ERR_INVALID_ARG;
    }
    const int prof = c->settings.profiling;
    c->settings.profiling = 0;
    struct Restore { akz_ctx* c; int p; ~Restore() { c->settings.profiling = p; } } restore{c, prof};
    // 1. warm: every buffer the chain uses exists afterwards (no allocation may happen while capturing)
    for (int i = 0; i < 2; ++i) {
        akz_result* r = nullptr;
        AKZ_TRY(extract_impl<uint8_t>(c, d_imgs, w, h, n, cfg, flags, &r));
        result_delete(r);
    }
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    Event e0, e1;
    AKZ_TRY(e0.ensure(hipEventDefault));
    AKZ_TRY(e1.ensure(hipEventDefault));
    // 2. plain chain, from an idle stream each time
    double plain = 0.0;
    for (uint32_t i = 0; i < reps; ++i) {
        akz_job* job = nullptr;
        AKZ_HIP_TRY(hipEventRecord(e0, c->stream));
        AKZ_TRY(extract_begin<uint8_t>(c, d_imgs, w, h, n, cfg, flags, &job));
        AKZ_HIP_TRY(hipEventRecord(e1, c->stream));
        AKZ_HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        AKZ_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        plain += ms;
        job_destroy(job);
    }
    // 3. the same chain as a graph
    akz_job* cap = nullptr;
    AKZ_HIP_TRY(hipStreamBeginCapture(c->stream, hipStreamCaptureModeRelaxed));
    const int st = extract_begin<uint8_t>(c, d_imgs, w, h, n, cfg, flags, &cap);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(c->stream, &graph);
    if (st != AKZ_OK || ce != hipSuccess || !graph) {
        if (cap) job_destroy(cap);
        if (st == AKZ_OK) set_error(std::string("stream capture of the begin phase failed: ") + hipGetErrorString(ce));
        return st != AKZ_OK ? st : AKZ_ERR_HIP;
    }
    size_t nodes = 0;
    (void)hipGraphGetNodes(graph, nullptr, &nodes);
    if (graph_nodes) *graph_nodes = nodes;
    hipGraphExec_t exec = nullptr;
    AKZ_HIP_TRY(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));
    AKZ_HIP_TRY(hipGraphLaunch(exec, c->stream));  // warm
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    double gms = 0.0;
    for (uint32_t i = 0; i < reps; ++i) {
        AKZ_HIP_TRY(hipEventRecord(e0, c->stream));
        AKZ_HIP_TRY(hipGraphLaunch(exec, c->stream));
        AKZ_HIP_TRY(hipEventRecord(e1, c->stream));
        AKZ_HIP_TRY(hipEventSynchronize(e1));
        float ms = 0.0f;
        AKZ_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        gms += ms;
    }
    (void)hipGraphExecDestroy(exec);
    (void)hipGraphDestroy(graph);
    job_destroy(cap);
    *ms_graph = gms / reps;
    *ms_plain = plain / reps;
    return AKZ_OK;
}

int akz_extract_from_planes(akz_ctx* c, uint32_t w, uint32_t h, const akz_config* cfg, const float* const* planes,
                            uint64_t n_levels, uint32_t flags, akz_result** out) {
    return extract_from_planes(c, w, h, cfg, planes, n_levels, flags, out);
}
int akz_job_abandon(akz_job* job) {
    if (!job) return AKZ_OK;
    job_wait(job);
    const akz_result* r = job->out ? job->out : job->r.get();
    if (r) (void)hipSetDevice(r->ctx->device);
    job_destroy(job);
    return AKZ_OK;
}

}  // extern "C"
