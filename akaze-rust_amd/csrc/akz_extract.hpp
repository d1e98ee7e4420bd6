// What the translation units of extract_features share (akz_extract.cpp, akz_extract_begin.cpp, akz_extract_finish.cpp,
// akz_result.cpp, akz_place.cpp): results and jobs, opening a job, the two halves.  Host only.
#pragma once
#include "akz_ctx.hpp"
#include "akz_frames.hpp"

struct akz_result {
    akz_ctx* ctx = nullptr;
    akz_config cfg;
    uint32_t w = 0, h = 0, n = 0, flags = 0;
    uint64_t big_px = 0;            // the job-size gate this job was begun under (gates::kBigPxSync / kBigPxAsync)
    std::vector<LevelPlan> plan;
    void* slab = nullptr;
    size_t slab_bytes = 0;
    float* planes[kMaxLevels][10];  // image 0 of the batch; stride = level w*h
    double* d_k = nullptr;          // inside the slab
    std::vector<double> k_host;
    std::vector<std::vector<akz_keypoint>> kps;
    std::vector<uint8_t> rows64;             // host copy of the 64-byte rows (all images)
    uint8_t* d_desc64 = nullptr;             // all images back to back, 64-byte rows
    size_t desc_block_bytes = 0;             // pooled device block behind d_desc64
    std::vector<uint64_t> desc_off;          // first row of each image in d_desc64
    std::vector<uint64_t> n_extrema;
};

// A job's detection mask on the device: height x width bytes per image, nonzero = detect here (akz_mask.hip); d == nullptr: none.
struct MaskSpec {
    const uint8_t* d = nullptr;
    uint64_t row_pitch = 0, frame_stride = 0;  // bytes; frame_stride 0: one mask for every image of the batch
};

// An extraction in flight: everything up to the NMS candidates is enqueued on the context's
// stream by extract_begin (no host synchronisation); extract_finish picks the candidates up on
// the auxiliary stream once `nms_done` fires and runs the host keypoint logic, orientation and
// descriptors.  With two jobs in flight the host phase of one batch runs under the kernels of the
// next while the scale-space kernels of both stay serialised on one stream.
struct ResultDeleter {
    void operator()(akz_result* r) const;
};
struct akz_job {
    std::unique_ptr<akz_result, ResultDeleter> r;
    int slot = -1;            // candidate / counter buffers used by this job
    uint32_t cap = 0;         // candidate capacity per image
    Event nms_done;
    uint64_t seq = 0;         // position in the context's order of begins (fed_ev ring)
    double t_begin_ms = 0.0;
    // eager finish: the lane's thread runs the finish half and leaves its outcome here (guarded by fin->m)
    std::shared_ptr<Finisher> fin;
    bool finished = false;
    int rc = 0;
    akz_result* out = nullptr;
    std::string err;
    // jobs of the context that the caller has begun and not collected yet (this one included), counted until the job object
    // goes: a job begun with none other in the caller's hand is being waited for, one begun with company is part of a stream
    std::shared_ptr<std::atomic<int>> in_hand;
    bool alone_at_begin = true;
    hipStream_t done_stream = nullptr;  // the stream the begin chain ended on (the main stream, or the forked coarse chain's)
    MaskSpec mask;            // the job's list is then c->cand_mask_slot[slot], what the mask keeps of c->cand_slot[slot]
    ~akz_job() {
        if (in_hand) --*in_hand;
    }
};

// the shape of a job as the context remembers it between jobs (last_cand_shape, sel_skip_shape)
inline uint64_t shape_key(uint32_t w, uint32_t h, uint32_t n) { return ((uint64_t)w << 40) | ((uint64_t)h << 16) | n; }
// a speculative size: as many as the last job had + 25 % + pad, capped
inline uint32_t like_last_job(uint32_t last, uint32_t pad, uint32_t cap) { return std::min<uint32_t>(cap, last + last / 4 + pad); }

// The header the device's selection leaves per image: kSelHdrWords 32-bit words (akz_sort.hip: SelOut::hdr, written by
// k_select and its sel_header_extras).  kSelHdrTotal is the whole job's, read from image 0's header.
constexpr uint32_t kSelHdrWords = 16;
enum SelHdr : uint32_t {
    kSelHdrKeypoints = 0,  // keypoints of the image
    kSelHdrExtrema = 1,    // extrema before the refinement
    kSelHdrFallback = 2,   // 0: selected on the device; else why the image goes to the host's selection
    kSelHdrRounds = 3,     // looks of the slowest thread
    kSelHdrTicks = 4,      // .. 7: 10 ns ticks of the four phases
    kSelHdrTotal = 8,      // the candidate list's length (all images)
    kSelHdrFlags = 9,      // the image's neighbour-list flags
    kSelHdrContrast = 10,  // .. 11: the image's contrast factor (a double)
};
inline const uint32_t* sel_hdr(const akz_ctx* c, uint32_t img) { return (const uint32_t*)c->pin[PIN_SEL_HDR].p + (size_t)img * kSelHdrWords; }

// the planes the keypoint kernels gather from
inline LevelTable level_table(const akz_result* r) {
    LevelTable tab;
    std::memset(&tab, 0, sizeof(tab));
    for (size_t l = 0; l < r->plan.size(); ++l)
        tab.lv[l] = {r->planes[l][AKZ_LT], r->planes[l][AKZ_LX], r->planes[l][AKZ_LY], r->plan[l].w, r->plan[l].h, (uint64_t)r->plan[l].w * r->plan[l].h};
    return tab;
}
// a keypoint as the orientation and M-LDB kernels take it: in the coordinates of its level, `octave` giving the ratio
inline KpParam kp_param(float x, float y, float size, uint32_t octave, uint32_t level, uint32_t img) {
    const float ratio = (float)(1u << octave);
    return KpParam{x / ratio, y / ratio, std::round(0.5f * size / ratio), level, img, {0, 0, 0}};
}

// ---- akz_result.cpp: slab pool, result / job lifetime ----
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
AKZ_LOCAL int slab_acquire(akz_ctx* c, size_t bytes, void** p, size_t* got);
AKZ_LOCAL void slab_release(akz_ctx* c, void* p, size_t bytes);
AKZ_LOCAL void result_delete(akz_result* r);
AKZ_LOCAL void job_release(akz_job* j);
AKZ_LOCAL void job_wait(akz_job* j);
AKZ_LOCAL void job_destroy(akz_job* j);
// Opening a job: job_open takes a free candidate slot (`want_slot`, or the first free one) and builds the job, its result and
// the plan; job_layout acquires the slab and places the wanted (level, plane) pairs and the contrast factors in it.  Until
// keep(), leaving the scope returns the device blocks to the pool.
struct JobOpening {
    std::unique_ptr<akz_job> job;
    int slot = -1;
    bool drain_side = false;  // the begin half: work already enqueued (possibly on the coarse stream, which nothing has joined yet) still writes the slab
    bool laid_out = false;
    ~JobOpening();
    akz_job* keep(uint32_t cap);  // the job holds its slot from here on
};
AKZ_LOCAL int free_slot(const akz_ctx* c, int want = -1);  // -1: none (or `want` is busy)
AKZ_LOCAL int job_open(akz_ctx* c, const char* who, int want_slot, uint32_t w, uint32_t h, uint32_t n, uint32_t flags, const akz_config& cfg,
                       JobOpening& o);
AKZ_LOCAL int job_layout(JobOpening& o, const std::vector<std::pair<uint32_t, int>>& wanted);
// ---- akz_place.cpp ----
AKZ_LOCAL int place_lanes(akz_ctx* c);
// ---- akz_extract_begin.cpp (instantiated for uint8_t and float) / akz_extract_finish.cpp ----
template <typename T>
AKZ_LOCAL int extract_begin(akz_ctx* c, const T* d_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfgp, uint32_t flags, akz_job** out,
                            int want_slot = -1, hipEvent_t input_ready = nullptr, bool sync_call = false, const MaskSpec* mask = nullptr);
// launch::mask_candidates of job r on stream s, with its kernel row (AKZ_KR_MASK_CANDIDATES under AKZ_ST_NMS): c->cand_slot[slot] ->
// c->cand_mask_slot[slot], which the caller has made `cap` records long
AKZ_LOCAL int mask_enqueue(akz_ctx* c, hipStream_t s, const akz_result* r, const MaskSpec& m, int slot, uint32_t cap, uint32_t* d_count);
// The finish half proper.  The job shell stays with the caller; on failure everything the job held is released.
AKZ_LOCAL int extract_finish_body(akz_job* jobp, akz_result** out);
// ---- akz_extract.cpp / akz_frames_api.cpp: device frames in a layout of the caller's (akz_frames.hpp) ----
AKZ_LOCAL int extract_begin_frames(akz_ctx* c, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, const akz_config* cfg, uint32_t flags, akz_job** out,
                                   const MaskSpec* mask = nullptr);
AKZ_LOCAL int extract_frames(akz_ctx* c, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, const akz_config* cfg, uint32_t flags, akz_result** out,
                             const MaskSpec* mask = nullptr);
// k_frame_luma on stream s of context c, with its profile row (stage 10)
AKZ_LOCAL int frames_enqueue(akz_ctx* c, hipStream_t s, const uint8_t* d_src, const FrameSpec& fs, uint32_t n, uint8_t* d_luma);
