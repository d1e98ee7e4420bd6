// C ABI of libakaze_hip.so, part 3c: the slab pool, the lifetime of results and jobs, the akz_result_* accessors and the
// downloads of planes and whole pyramids.
#include "akz_extract.hpp"

int slab_acquire(akz_ctx* c, size_t bytes, void** p, size_t* got) {
    bytes = align_up(std::max<size_t>(bytes, 256), 256);
    std::lock_guard<std::mutex> lk(c->slab_m);
    DevBuf b;  // (the block leaves as a raw pointer: a result holds it until slab_release, or until it is freed behind a dead context)
    for (size_t i = 0; i < c->slab_pool.size() && !b.p; ++i)
        if (c->slab_pool[i].bytes >= bytes && c->slab_pool[i].bytes <= bytes + bytes / 4 + 65536) {
            b = std::move(c->slab_pool[i]);
            c->slab_pool.erase(c->slab_pool.begin() + (long)i);
        }
    if (!b.p) {
        bytes += bytes / 8;  // head-room so that the next, slightly larger request can reuse the block
        AKZ_HIP_TRY(b.acquire(bytes, false));
        AKZ_HIP_TRY(alloc_fill(c, b.p, bytes));
    }
    *got = b.bytes;
    *p = b.detach();
    return AKZ_OK;
}
void slab_release(akz_ctx* c, void* p, size_t bytes) {
    std::lock_guard<std::mutex> lk(c->slab_m);
    if (c->slab_pool.size() >= 8) {
        (void)sync_all_streams(c);
        c->slab_pool.erase(c->slab_pool.begin());
    }
    c->slab_pool.push_back(DevBuf::adopt(p, bytes));
}

static void result_release_device(akz_result* r) {
    if (r->ctx && r->ctx->dead) {  // the pools went away with the context: hand the blocks back to the runtime
        (void)DevBuf::adopt(r->slab, r->slab_bytes).release();
        (void)DevBuf::adopt(r->d_desc64, r->desc_block_bytes).release();
    } else {
        if (r->slab) slab_release(r->ctx, r->slab, r->slab_bytes);
        if (r->d_desc64) slab_release(r->ctx, r->d_desc64, r->desc_block_bytes);
    }
    r->slab = nullptr;
    r->d_desc64 = nullptr;
}
// Every akz_result is deleted through here: a result may outlive akz_ctx_destroy (a caller that frees in the
// "wrong" order); the context struct itself is then released with its last result.
void result_delete(akz_result* r) {
    if (!r) return;
    akz_ctx* c = r->ctx;
    result_release_device(r);
    delete r;
    if (c && --c->live_results == 0 && c->dead) delete c;
}
void ResultDeleter::operator()(akz_result* r) const { result_delete(r); }
// a job that will not produce a result hands back what it holds on its context (the shell itself is deleted by the caller)
void job_release(akz_job* j) {
    akz_ctx* c = j->r ? j->r->ctx : nullptr;
    if (!c) return;
    // the streams the begin half enqueues on (a forked batch completes on the coarse stream); the finish half's is not one of them
    (void)sync_all_streams(c, kSyncMain | kSyncSide);
    if (j->slot >= 0) c->slot_busy[j->slot] = false;
    j->slot = -1;
    ev_put(c, std::move(j->nms_done));
    result_release_device(j->r.get());
}
// the outcome of an eagerly finished job, once its lane's thread is through with it
void job_wait(akz_job* j) {
    if (!j->fin) return;
    std::unique_lock<std::mutex> lk(j->fin->m);
    j->fin->done.wait(lk, [&] { return j->finished; });
}
void job_destroy(akz_job* j) {
    if (!j) return;
    if (j->fin) {
        job_wait(j);
        if (j->out) result_delete(j->out);
    } else {
        job_release(j);
    }
    delete j;
}

int free_slot(const akz_ctx* c, int want) {
    for (int i = 0; i < akz_ctx::kSlots && want < 0; ++i)
        if (!c->slot_busy[i]) want = i;
    return want >= 0 && !c->slot_busy[want] ? want : -1;
}
int job_open(akz_ctx* c, const char* who, int want_slot, uint32_t w, uint32_t h, uint32_t n, uint32_t flags, const akz_config& cfg, JobOpening& o) {
    o.slot = free_slot(c, want_slot);
    if (o.slot < 0) {
        set_error(std::string(who) + ": too many extractions in flight on this context (finish one first)");
        return AKZ_ERR_INVALID_ARG;
    }
    o.job.reset(new akz_job);
    o.job->in_hand = c->in_hand;
    o.job->alone_at_begin = o.job->in_hand->fetch_add(1) == 0;
    o.job->r.reset(new akz_result);
    akz_result* r = o.job->r.get();
    r->ctx = c;
    ++c->live_results;
    r->cfg = cfg;
    r->w = w; r->h = h; r->n = n; r->flags = flags;
    return build_plan(w, h, r->cfg, r->plan);
}
int job_layout(JobOpening& o, const std::vector<std::pair<uint32_t, int>>& wanted) {
    akz_result* r = o.job->r.get();
    std::memset(r->planes, 0, sizeof(r->planes));
    size_t off = 0;
    std::vector<size_t> at;
    for (const auto& lp : wanted) {
        at.push_back(off);
        off += align_up(plane_bytes(r->plan[lp.first].w, r->plan[lp.first].h, r->n), 256);
    }
    const size_t k_off = off;
    off += align_up((size_t)r->n * sizeof(double), 256);
    AKZ_TRY(slab_acquire(r->ctx, off, &r->slab, &r->slab_bytes));
    o.laid_out = true;
    for (size_t i = 0; i < wanted.size(); ++i) r->planes[wanted[i].first][wanted[i].second] = (float*)((char*)r->slab + at[i]);
    if (!r->planes[0][AKZ_LSMOOTH]) r->planes[0][AKZ_LSMOOTH] = r->planes[0][AKZ_LT];  // level 0: Lsmooth is a clone of Lt (lib.rs:58) -> alias
    r->d_k = (double*)((char*)r->slab + k_off);
    return AKZ_OK;
}
JobOpening::~JobOpening() {  // return the device blocks to the pool on any early error exit
    if (!laid_out || !job) return;
    // (the main stream is not waited for: the pool hands a block out again to work that is enqueued behind it)
    if (drain_side) (void)sync_all_streams(job->r->ctx, kSyncSide);
    result_release_device(job->r.get());
}
akz_job* JobOpening::keep(uint32_t cap) {
    job->slot = slot;
    job->cap = cap;
    job->r->ctx->slot_busy[slot] = true;
    laid_out = false;
    return job.release();
}

extern "C" {

int akz_result_free(akz_result* r) {
    if (!r) return AKZ_OK;
    (void)hipSetDevice(r->ctx->device);
    result_delete(r);
    return AKZ_OK;
}
int akz_result_num_images(const akz_result* r, uint64_t* n) {
    if (!r || !n) return AKZ_ERR_INVALID_ARG;
    *n = r->n;
    return AKZ_OK;
}
static int check_img(const akz_result* r, uint64_t img) {
    if (!r || img >= r->n) {
        set_error("null result or image index out of range");
        return AKZ_ERR_INVALID_ARG;
    }
    return AKZ_OK;
}
int akz_result_counts(const akz_result* r, uint64_t img, uint64_t* n_levels, uint64_t* n_keypoints,
                      uint64_t* desc_bytes) {
    AKZ_TRY(check_img(r, img));
    if (n_levels) *n_levels = r->plan.size();
    if (n_keypoints) *n_keypoints = r->kps[(size_t)img].size();
    if (desc_bytes) *desc_bytes = ((6 + 36 + 120) * r->cfg.descriptor_channels + 7) / 8;
    return AKZ_OK;
}
int akz_result_keypoints(const akz_result* r, uint64_t img, akz_keypoint* out) {
    AKZ_TRY(check_img(r, img));
    const auto& k = r->kps[(size_t)img];
    if (!k.empty()) {
        if (!out) return AKZ_ERR_INVALID_ARG;
        std::memcpy(out, k.data(), k.size() * sizeof(akz_keypoint));
    }
    return AKZ_OK;
}
int akz_result_descriptors(const akz_result* r, uint64_t img, uint8_t* out) {
    AKZ_TRY(check_img(r, img));
    if (r->flags & AKZ_NO_HOST_DESCRIPTORS) {
        set_error("descriptors were kept on the device (AKZ_NO_HOST_DESCRIPTORS)");
        return AKZ_ERR_INVALID_ARG;
    }
    const size_t nk = r->kps[(size_t)img].size();
    if (nk) {
        if (!out) return AKZ_ERR_INVALID_ARG;
        const size_t nb = ((6 + 36 + 120) * r->cfg.descriptor_channels + 7) / 8;
        const uint8_t* rows = r->rows64.data() + r->desc_off[(size_t)img] * 64;
        for (size_t i = 0; i < nk; ++i) std::memcpy(out + i * nb, rows + i * 64, nb);
    }
    return AKZ_OK;
}
// ops::scale_space_extrema::compute_main_orientation (scale_space_extrema.rs:207-329) and
// ops::descriptors::extract_descriptors (descriptors.rs:14-35) for CALLER-SUPPLIED keypoints of image `img`, on the
// pyramid the result retains: what the reference's two public ops do when they are handed a keypoint list that did
// not come out of detect_keypoints (re-description, externally detected points).
int akz_result_describe_keypoints(const akz_result* r, uint64_t img, akz_keypoint* kps, uint64_t n_kp,
                                  int compute_orientation, uint8_t* descriptors) {
    AKZ_TRY(check_img(r, img));
    akz_ctx* c = r->ctx;
    AKZ_TRY(bind(c));
    if (n_kp == 0) return AKZ_OK;
    if (!kps || !descriptors) {
        set_error("akz_result_describe_keypoints: null argument");
        return AKZ_ERR_INVALID_ARG;
    }
    const size_t L = r->plan.size();
    const LevelTable tab = level_table(r);
    AKZ_TRY(ensure_aux(c));
    hipStream_t s = c->aux;
    // The descriptor takes its ratio from the KEYPOINT's octave (descriptors.rs:51), the orientation from the octave of the
    // keypoint's LEVEL (scale_space_extrema.rs:279).  The detector's keypoints carry their level's octave; a caller's need not:
    // the orientation launch then reads a second parameter list (behind the first, in the same buffers).
    bool own_octave = false;
    if (compute_orientation)
        for (uint64_t i = 0; i < n_kp && !own_octave; ++i)
            own_octave = kps[i].class_id < L && kps[i].octave != r->plan[(size_t)kps[i].class_id].octave;
    const uint64_t n_par = own_octave ? 2 * n_kp : n_kp;
    AKZ_TRY(ensure_pinned(c, c->pin[PIN_PARAMS], n_par * sizeof(KpParam)));
    KpParam* params = (KpParam*)c->pin[PIN_PARAMS].p;
    for (uint64_t i = 0; i < n_kp; ++i) {
        const akz_keypoint& k = kps[i];
        if (k.class_id >= L || k.octave > 30) {  // the reference indexes evolutions[class_id] and would panic
            set_error("akz_result_describe_keypoints: keypoint class_id / octave out of range");
            return AKZ_ERR_INVALID_ARG;
        }
        params[i] = kp_param(k.x, k.y, k.size, k.octave, (uint32_t)k.class_id, (uint32_t)img);
        if (own_octave) params[n_kp + i] = kp_param(k.x, k.y, k.size, r->plan[(size_t)k.class_id].octave, (uint32_t)k.class_id, (uint32_t)img);
    }
    AKZ_TRY(ensure(c, c->kp_in, n_par * sizeof(KpParam)));
    AKZ_TRY(ensure(c, c->kp_out, n_kp * sizeof(OrientOut)));
    AKZ_TRY(ensure(c, c->cosi, n_kp * 2 * sizeof(float)));
    AKZ_TRY(ensure_pinned(c, c->pin[PIN_COUNT_SUMS], n_kp * std::max(sizeof(OrientOut), 2 * sizeof(float))));
    KpParam* d_kp = (KpParam*)c->kp_in.p;
    AKZ_HIP_TRY(hipMemcpyAsync(d_kp, params, n_par * sizeof(KpParam), hipMemcpyHostToDevice, s));
    if (compute_orientation) {
        unsigned long long wmask = 0;
        uint32_t nwin = 0;
        orientation_windows(&wmask, &nwin);
        OrientOut* d_oo = (OrientOut*)c->kp_out.p;
        launch::orientation(s, tab, own_octave ? d_kp + n_kp : d_kp, (uint32_t)n_kp, wmask, nwin, d_oo);
        AKZ_HIP_TRY(hipGetLastError());
        OrientOut* oo = (OrientOut*)c->pin[PIN_COUNT_SUMS].p;
        AKZ_HIP_TRY(hipMemcpyAsync(oo, d_oo, n_kp * sizeof(OrientOut), hipMemcpyDeviceToHost, s));
        AKZ_HIP_TRY(hipStreamSynchronize(s));
        for (uint64_t i = 0; i < n_kp; ++i)  // no window sum above zero: the angle keeps its value (scale_space_extrema.rs:322-327)
            if (oo[i].found) kps[i].angle = atan2f(oo[i].sum_y, oo[i].sum_x);
    }
    AKZ_TRY(ensure_pinned(c, c->pin[PIN_COSI], n_kp * 2 * sizeof(float)));
    float* cosi = (float*)c->pin[PIN_COSI].p;
    for (uint64_t i = 0; i < n_kp; ++i) {
        cosi[2 * i] = cosf(kps[i].angle);  // descriptors.rs:55-56
        cosi[2 * i + 1] = sinf(kps[i].angle);
    }
    AKZ_HIP_TRY(hipMemcpyAsync(c->cosi.p, cosi, n_kp * 2 * sizeof(float), hipMemcpyHostToDevice, s));
    AKZ_TRY(ensure(c, c->match_a, n_kp * 64));
    uint8_t* d_rows = (uint8_t*)c->match_a.p;
    launch::mldb(s, tab, d_kp, (const float*)c->cosi.p, (uint32_t)n_kp, (uint32_t)r->cfg.descriptor_channels, d_rows);
    AKZ_HIP_TRY(hipGetLastError());
    AKZ_TRY(ensure_pinned(c, c->pin[PIN_ROWS], n_kp * 64));
    uint8_t* rows = (uint8_t*)c->pin[PIN_ROWS].p;
    AKZ_HIP_TRY(hipMemcpyAsync(rows, d_rows, n_kp * 64, hipMemcpyDeviceToHost, s));
    AKZ_HIP_TRY(hipStreamSynchronize(s));
    const size_t nb = ((6 + 36 + 120) * r->cfg.descriptor_channels + 7) / 8;
    for (uint64_t i = 0; i < n_kp; ++i) std::memcpy(descriptors + i * nb, rows + i * 64, nb);
    return AKZ_OK;
}
int akz_result_device_descriptors(const akz_result* r, uint64_t img, const uint8_t** d_desc, uint64_t* n_keypoints) {
    AKZ_TRY(check_img(r, img));
    if (d_desc) *d_desc = r->d_desc64 ? r->d_desc64 + r->desc_off[(size_t)img] * 64 : nullptr;
    if (n_keypoints) *n_keypoints = r->kps[(size_t)img].size();
    return AKZ_OK;
}
int akz_result_copy_device_descriptors(const akz_result* r, uint8_t* d_dst, uint64_t capacity_rows, uint64_t* rows) {
    if (!r) return AKZ_ERR_INVALID_ARG;
    const uint64_t total = r->desc_off.empty() ? 0 : r->desc_off.back();
    if (rows) *rows = total;
    if (total == 0) return AKZ_OK;
    if (!d_dst || capacity_rows < total) {
        set_error("copy_device_descriptors: destination too small");
        return AKZ_ERR_BUFFER;
    }
    AKZ_TRY(bind(r->ctx, true, false));
    // on the auxiliary stream and complete on return: the context's main stream may already be busy
    // with the next batch, and the caller typically hands d_dst to a collective on yet another stream
    akz_ctx* c = r->ctx;
    AKZ_TRY(ensure_aux(c));
    AKZ_HIP_TRY(hipMemcpyAsync(d_dst, r->d_desc64, total * 64, hipMemcpyDeviceToDevice, c->aux));
    AKZ_HIP_TRY(hipStreamSynchronize(c->aux));
    return AKZ_OK;
}
int akz_result_contrast(const akz_result* r, uint64_t img, double* k) {
    AKZ_TRY(check_img(r, img));
    if (!k) return AKZ_ERR_INVALID_ARG;
    *k = r->k_host[(size_t)img];
    return AKZ_OK;
}
int akz_result_level_info(const akz_result* r, uint64_t level, double* etime, double* esigma, uint32_t* octave,
                          uint32_t* sublevel, uint32_t* sigma_size, uint32_t* w, uint32_t* h, uint64_t* n_tau,
                          double* tau, uint64_t tau_cap) {
    if (!r) return AKZ_ERR_INVALID_ARG;
    return level_info_out(r->plan, level, etime, esigma, octave, sublevel, sigma_size, w, h, nullptr, n_tau, tau,
                          tau_cap);
}
int akz_result_device_plane(const akz_result* r, uint64_t img, uint64_t level, akz_plane plane,
                            const float** d_plane) {
    AKZ_TRY(check_img(r, img));
    if (level >= r->plan.size() || (int)plane < 0 || (int)plane > 9 || !d_plane) {
        set_error("level/plane out of range");
        return AKZ_ERR_INVALID_ARG;
    }
    const float* base = r->planes[(size_t)level][(int)plane];
    const LevelPlan& lv = r->plan[(size_t)level];
    *d_plane = base ? base + (size_t)img * lv.w * lv.h : nullptr;
    return AKZ_OK;
}
// A plane that the extraction did not keep (Lxx, Lyy, Lxy, Lstep without AKZ_KEEP_ALL_PLANES) is recomputed for one
// image from planes that are always kept, with the kernels and in the order of the extraction: second derivatives
// from the level's Lsmooth (detector_response.rs:9-13), Lstep by repeating the level's diffusion from the previous
// level's Lt (lib.rs:80-92, :109-118).  Bit-identical to the kept planes; *d_out points into context scratch memory
// that the next call overwrites.
static int recompute_plane(const akz_result* r, uint64_t img, uint64_t level, akz_plane plane, const float** d_out) {
    akz_ctx* c = r->ctx;
    AKZ_TRY(bind(c));
    const JobForm f = no_job_form(c);
    const LevelPlan& lv = r->plan[(size_t)level];
    const size_t px = (size_t)lv.w * lv.h, pb = px * sizeof(float);
    auto img_plane = [&](uint64_t l, int p) { return r->planes[(size_t)l][p] + (size_t)img * r->plan[(size_t)l].w * r->plan[(size_t)l].h; };
    *d_out = nullptr;
    if (plane == AKZ_LXX || plane == AKZ_LYY || plane == AKZ_LXY) {
        for (int k = 0; k < 6; ++k) AKZ_TRY(ensure(c, c->lazy[k], pb));
        float* b[6];
        for (int k = 0; k < 6; ++k) b[k] = (float*)c->lazy[k].p;
        AKZ_TRY(detector_impl(c, f, img_plane(level, AKZ_LSMOOTH), lv.det_sigma, b[0], b[1], b[2], b[3], b[4], b[5], lv.w, lv.h, 1));
        *d_out = plane == AKZ_LXX ? b[2] : plane == AKZ_LYY ? b[3] : b[4];
        return AKZ_OK;
    }
    if (plane == AKZ_LSTEP && level > 0) {
        const LevelPlan& pv = r->plan[(size_t)level - 1];
        for (int k = 0; k < 4; ++k) AKZ_TRY(ensure(c, c->lazy[k], std::max(pb, (size_t)4)));
        float *A = (float*)c->lazy[0].p, *B = (float*)c->lazy[1].p, *step = (float*)c->lazy[2].p;
        const float* in = img_plane(level - 1, AKZ_LT);
        if (lv.octave > pv.octave) {  // first level of an octave: the 2x2 mean of the previous level's Lt
            launch::half_size(c->stream, in, (float*)c->lazy[3].p, pv.w, pv.h, 1);
            in = (const float*)c->lazy[3].p;
        }
        AKZ_HIP_TRY(hipMemsetAsync(step, 0, pb, c->stream));  // a level without diffusion steps keeps the zero plane (lib.rs:107)
        AKZ_TRY(fed_impl(c, f, in, A, B, img_plane(level, AKZ_LFLOW), step, lv.w, lv.h, 1, lv.tau.data(), (uint32_t)lv.tau.size()));
        *d_out = step;
        return AKZ_OK;
    }
    return AKZ_OK;  // level 0 has no Lflow / Lstep (0 x 0 in the reference)
}

int akz_fetch_plane(const akz_result* r, uint64_t img, uint64_t level, akz_plane plane, float* out, uint64_t* n_px) {
    const float* d = nullptr;
    AKZ_TRY(akz_result_device_plane(r, img, level, plane, &d));
    const LevelPlan& lv = r->plan[(size_t)level];
    const bool lazy = !d && (plane == AKZ_LXX || plane == AKZ_LYY || plane == AKZ_LXY || (plane == AKZ_LSTEP && level > 0));
    if (lazy && !out) {  // size query
        if (n_px) *n_px = (uint64_t)lv.w * lv.h;
        return AKZ_OK;
    }
    if (lazy) AKZ_TRY(recompute_plane(r, img, level, plane, &d));
    const uint64_t npx = d ? (uint64_t)lv.w * lv.h : 0;
    if (n_px) *n_px = npx;
    if (out && npx) {
        AKZ_TRY(bind(r->ctx));
        AKZ_HIP_TRY(hipMemcpyAsync(out, d, npx * sizeof(float), hipMemcpyDeviceToHost, r->ctx->stream));
        AKZ_HIP_TRY(hipStreamSynchronize(r->ctx->stream));
    }
    return AKZ_OK;
}

// ---- akz_fetch_pyramid -------------------------------------------------------------------------------------------------
// Staging of pageable destinations: kFetchStageBufs pinned buffers of kFetchStageBytes.  The downloads of two buffers are
// queued while the host copies the third one out.  8 MiB: one pinned D2H copy of 1 / 2 / 4 / 8 / 16 / 32 MiB moves
// 36.1 / 43.6 / 49.2 / 52.9 / 55.2 / 56.1 GB/s on an MI355X (profiles/r07_pyramid_fetch.json), so 8 MiB is 0.94 of the
// largest copy's rate while the ring stays at 24 MiB of page-locked memory per context.
static constexpr int kFetchStageBufs = 3;
static constexpr size_t kFetchStageBytes = (size_t)8 << 20;
static_assert(kFetchStageBufs <= 4, "akz_ctx::fetch_chunk has 4 events");
// host copies out of staging are split into pieces of this size across the context's worker threads
static constexpr size_t kFetchHostPiece = (size_t)512 << 10;

// [p, p + bytes) lies inside one page-locked host allocation (hipHostMalloc / hipHostRegister): the DMA may write it
// directly.  Anything the runtime cannot vouch for -- pageable memory, a range that runs past the locked block -- is staged.
static bool pinned_range(const void* p, size_t bytes) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
    void* start = nullptr;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)p) != hipSuccess ||
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const uintptr_t b = (uintptr_t)start, q = (uintptr_t)p;
    return q >= b && q + bytes <= b + size;
}

static int fetch_events(akz_ctx* c) {
    for (Stream& s : c->fetch) AKZ_TRY(s.ensure());
    for (Event* e : {&c->fetch_chunk[0], &c->fetch_chunk[1], &c->fetch_chunk[2], &c->fetch_chunk[3], &c->fetch_start,
                     &c->fetch_join, &c->fetch_ready[0], &c->fetch_ready[1], &c->fetch_free[0], &c->fetch_free[1]})
        AKZ_TRY(e->ensure());
    return AKZ_OK;
}

namespace {
// Downloads on the context's two fetch streams, alternately, so that one copy's start-up hides under the other's transfer.
// A pinned destination is written by the DMA itself; a pageable one goes through the staging ring: a chunk fills one
// buffer (pieces of consecutive planes back to back, so the small coarse planes share one round trip), completes on its
// event, and is copied out on the worker pool while the chunks behind it are in flight.
struct FetchEngine {
    explicit FetchEngine(akz_ctx* ctx) : c(ctx) {}
    akz_ctx* c;
    struct Piece { size_t off; float* dst; size_t bytes; };
    std::vector<Piece> pieces[kFetchStageBufs];
    size_t used = 0;
    uint64_t filled = 0, drained = 0;  // chunks closed / copied out
    uint64_t direct = 0;               // pinned destinations written
    char* stage(uint64_t chunk) const { return (char*)c->fetch_stage.p + (chunk % kFetchStageBufs) * kFetchStageBytes; }

    int copy(const float* src, float* dst, size_t bytes) {
        if (pinned_range(dst, bytes)) {
            AKZ_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->fetch[direct++ % 2]));
            return AKZ_OK;
        }
        if (!c->fetch_stage.p) AKZ_TRY(ensure_pinned(c, c->fetch_stage, kFetchStageBufs * kFetchStageBytes));
        const char* s = (const char*)src;
        char* d = (char*)dst;
        while (bytes) {
            if (used == kFetchStageBytes) AKZ_TRY(close());
            const size_t n = std::min(bytes, kFetchStageBytes - used);
            AKZ_HIP_TRY(hipMemcpyAsync(stage(filled) + used, s, n, hipMemcpyDeviceToHost, c->fetch[filled % 2]));
            pieces[filled % kFetchStageBufs].push_back({used, (float*)d, n});
            used += n, s += n, d += n, bytes -= n;
        }
        return AKZ_OK;
    }
    // the current chunk is complete on the stream; its buffer's successor must be free before anything is staged into it
    int close() {
        if (!used) return AKZ_OK;
        AKZ_HIP_TRY(hipEventRecord(c->fetch_chunk[filled % kFetchStageBufs], c->fetch[filled % 2]));
        ++filled;
        used = 0;
        if (filled - drained == (uint64_t)kFetchStageBufs) AKZ_TRY(drain());
        return AKZ_OK;
    }
    int drain() {
        const int b = (int)(drained % kFetchStageBufs);
        AKZ_HIP_TRY(hipEventSynchronize(c->fetch_chunk[b]));
        const char* base = stage(drained);
        struct Part { const char* src; char* dst; size_t bytes; };
        std::vector<Part> parts;
        for (const Piece& p : pieces[b])
            for (size_t o = 0; o < p.bytes; o += kFetchHostPiece)
                parts.push_back({base + p.off + o, (char*)p.dst + o, std::min(kFetchHostPiece, p.bytes - o)});
        c->pool().run(parts.size(), [&](size_t i) { std::memcpy(parts[i].dst, parts[i].src, parts[i].bytes); });
        pieces[b].clear();
        ++drained;
        return AKZ_OK;
    }
    int finish() {
        AKZ_TRY(close());
        while (drained < filled) AKZ_TRY(drain());
        for (hipStream_t s : c->fetch) AKZ_HIP_TRY(hipStreamSynchronize(s));  // the direct (pinned) downloads
        return AKZ_OK;
    }
};
}  // namespace

static int fetch_pyramid(const akz_result* r, uint64_t img, float* const* dst, uint64_t* bytes_out) {
    akz_ctx* c = r->ctx;
    const size_t L = r->plan.size();
    auto px_of = [&](size_t l) { return (size_t)r->plan[l].w * r->plan[l].h; };
    auto img_plane = [&](size_t l, int p) -> const float* {
        return r->planes[l][p] ? r->planes[l][p] + (size_t)img * px_of(l) : nullptr;
    };
    // what each level needs recomputed (Lxx / Lyy / Lxy from Lsmooth, Lstep from the previous level's Lt): the planes
    // akz_fetch_plane recomputes, requested and not kept
    std::vector<uint8_t> need_deriv(L, 0), need_step(L, 0);
    std::vector<size_t> rc;  // the levels to recompute, in order; level rc[k] uses output set k % 2
    size_t rc_px = 0;
    for (size_t l = 0; l < L; ++l) {
        for (int p : {(int)AKZ_LXX, (int)AKZ_LYY, (int)AKZ_LXY})
            if (dst[l * 10 + p] && !r->planes[l][p] && r->planes[l][AKZ_LSMOOTH]) need_deriv[l] = 1;
        if (l > 0 && dst[l * 10 + AKZ_LSTEP] && !r->planes[l][AKZ_LSTEP] && r->planes[l - 1][AKZ_LT] && r->planes[l][AKZ_LFLOW])
            need_step[l] = 1;
        if (need_deriv[l] || need_step[l]) {
            rc.push_back(l);
            rc_px = std::max(rc_px, px_of(l));
        }
    }
    AKZ_TRY(fetch_events(c));
    if (!rc.empty()) {
        const size_t pb = std::max(rc_px * sizeof(float), (size_t)4);
        for (DevBuf& b : c->fetch_tmp) AKZ_TRY(ensure(c, b, pb));
        for (size_t s = 0; s < std::min<size_t>(rc.size(), 2); ++s)
            for (DevBuf& b : c->fetch_out[s]) AKZ_TRY(ensure(c, b, pb));
    }
    // everything queued on the context's stream so far (the result's own kernels included) comes before the downloads
    AKZ_HIP_TRY(hipEventRecord(c->fetch_start, c->stream));
    for (hipStream_t s : c->fetch) AKZ_HIP_TRY(hipStreamWaitEvent(s, c->fetch_start, 0));

    // recomputation k on the context's stream, with the kernels and the argument order of recompute_plane.  Its output
    // set was last read by the downloads of recomputation k - 2, which are queued by then (see the walk below).
    const JobForm form = no_job_form(c);
    auto recompute = [&](size_t k) -> int {
        const size_t l = rc[k], s = k % 2;
        const LevelPlan& lv = r->plan[l];
        float* t[3] = {(float*)c->fetch_tmp[0].p, (float*)c->fetch_tmp[1].p, (float*)c->fetch_tmp[2].p};
        float* o[4] = {(float*)c->fetch_out[s][0].p, (float*)c->fetch_out[s][1].p, (float*)c->fetch_out[s][2].p,
                       (float*)c->fetch_out[s][3].p};
        if (k >= 2) AKZ_HIP_TRY(hipStreamWaitEvent(c->stream, c->fetch_free[s], 0));
        if (need_deriv[l])
            AKZ_TRY(detector_impl(c, form, img_plane(l, AKZ_LSMOOTH), lv.det_sigma, t[0], t[1], o[0], o[1], o[2], t[2], lv.w, lv.h, 1));
        if (need_step[l]) {
            const LevelPlan& pv = r->plan[l - 1];
            const float* in = img_plane(l - 1, AKZ_LT);
            if (lv.octave > pv.octave) {  // first level of an octave: the 2x2 mean of the previous level's Lt
                launch::half_size(c->stream, in, t[2], pv.w, pv.h, 1);
                in = t[2];
            }
            if (lv.tau.empty())  // a level without diffusion steps keeps the zero plane (lib.rs:107)
                AKZ_HIP_TRY(hipMemsetAsync(o[3], 0, px_of(l) * sizeof(float), c->stream));
            AKZ_TRY(fed_impl(c, form, in, t[0], t[1], img_plane(l, AKZ_LFLOW), o[3], lv.w, lv.h, 1, lv.tau.data(), (uint32_t)lv.tau.size()));
        }
        AKZ_HIP_TRY(hipGetLastError());
        AKZ_HIP_TRY(hipEventRecord(c->fetch_ready[s], c->stream));
        return AKZ_OK;
    };

    FetchEngine eng(c);
    uint64_t bytes = 0;
    size_t next_rc = 0, k = 0;  // recomputations queued / the first one at or after the current level
    for (size_t l = 0; l < L; ++l) {
        while (k < rc.size() && rc[k] < l) ++k;
        // one recomputation ahead of the downloads: level l's next one runs while this level is being copied
        for (; next_rc < rc.size() && next_rc <= k + 1; ++next_rc) AKZ_TRY(recompute(next_rc));
        const bool mine = k < rc.size() && rc[k] == l;
        if (mine)
            for (hipStream_t s : c->fetch) AKZ_HIP_TRY(hipStreamWaitEvent(s, c->fetch_ready[k % 2], 0));
        for (int p = 0; p < 10; ++p) {
            float* d = dst[l * 10 + p];
            if (!d) continue;
            const float* src = img_plane(l, p);
            if (!src && mine && p >= AKZ_LXX && p <= AKZ_LXY && need_deriv[l]) src = (const float*)c->fetch_out[k % 2][p - AKZ_LXX].p;
            if (!src && mine && p == AKZ_LSTEP && need_step[l]) src = (const float*)c->fetch_out[k % 2][3].p;
            if (!src) continue;  // level 0's Lflow / Lstep
            const size_t nb = px_of(l) * sizeof(float);
            AKZ_TRY(eng.copy(src, d, nb));
            bytes += nb;
        }
        if (mine) {  // both streams' downloads of the set are queued: join them into the one event the next user waits for
            AKZ_HIP_TRY(hipEventRecord(c->fetch_join, c->fetch[1]));
            AKZ_HIP_TRY(hipStreamWaitEvent(c->fetch[0], c->fetch_join, 0));
            AKZ_HIP_TRY(hipEventRecord(c->fetch_free[k % 2], c->fetch[0]));
        }
    }
    AKZ_TRY(eng.finish());
    if (bytes_out) *bytes_out = bytes;
    return AKZ_OK;
}

int akz_fetch_pyramid(const akz_result* r, uint64_t img, float* const* dst, uint64_t n_dst, uint64_t* bytes_out) {
    AKZ_TRY(check_img(r, img));
    if (!dst || n_dst != (uint64_t)r->plan.size() * 10) {
        set_error("akz_fetch_pyramid: dst must hold n_levels * 10 entries");
        return AKZ_ERR_INVALID_ARG;
    }
    AKZ_TRY(bind(r->ctx));
    const int rc = fetch_pyramid(r, img, dst, bytes_out);
    if (rc != AKZ_OK) {  // nothing of this call may still be writing when it returns
        for (hipStream_t s : r->ctx->fetch)
            if (s) (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(r->ctx->stream);
    }
    return rc;
}


}  // extern "C"
