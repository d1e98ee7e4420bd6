// The context of libakaze_hip.so and what every translation unit of the C ABI shares: akz_ctx (streams, scratch, pools, profile),
// the stage timer, buffer helpers and the entry-point prologue (bind).  The C ABI itself is split by boundary area:
//   akz_api.cpp      context lifecycle, host-side planning, profile, modes and measurement hooks
//   akz_ops.cpp      the per-op entry points (`pub mod ops` / `types::image`) and the launch helpers the pipeline shares with them
//   akz_extract.cpp  extract_features: the C entry points, lanes and the finisher thread, gate calibration, the graph probe
//     akz_extract_begin.cpp / akz_extract_finish.cpp  its two halves (private header: akz_extract.hpp)
//     akz_result.cpp   slab pool, result / job lifetime, the result accessors, plane and pyramid downloads
//     akz_place.cpp    stream placement
//   akz_match_api.cpp  descriptor_match in all its forms, match_features
//   akz_jpeg_api.cpp   file ingest with JPEG reconstruction on the device (akz_extract_features_file / _files)
// Every size / host-thread gate that picks between kernel families or paths is a named constant of akz_gates.hpp.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <sched.h>
#include <time.h>
#include <type_traits>

#include "akz_internal.hpp"
#include "akz_select.hpp"
#include "akz_pool.hpp"
#include "akz_gates.hpp"
#include "akz_pairs_layout.hpp"

// functions shared by the library's translation units, none of them exported
#define AKZ_LOCAL __attribute__((visibility("hidden")))

namespace akz {
const std::string& get_error();
}
using namespace akz;

namespace {
struct SelKpHost {  // a keypoint of the device's selection as the host fetches it (akz_sort.hip: SelKp)
    sel::KpRec rec;
    OrientOut sums;
};
static_assert(sizeof(SelKpHost) == 32, "the device writes 32-byte records");
}  // namespace

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// What the library holds of the runtime -- memory blocks, events, streams -- lives in three move-only owners: each frees its handle
// when it goes, so a context (CtxOwned below) or a function that declares one has said all there is to say about its lifetime.
// res::live counts what they hold, process-wide (akz_debug_resource_counts): up on acquire, down on release.
namespace res {
enum Kind { kDevBlocks = 0, kDevBytes, kPinBlocks, kPinBytes, kEvents, kStreams, kKinds_ };
AKZ_LOCAL inline std::atomic<uint64_t> live[kKinds_];
inline void up(Kind k, uint64_t n = 1) { live[k].fetch_add(n, std::memory_order_relaxed); }
inline void down(Kind k, uint64_t n = 1) { live[k].fetch_sub(n, std::memory_order_relaxed); }
}  // namespace res
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool pinned = false;  // page-locked host memory (ensure_pinned, the matcher's rings), else device memory
    size_t known = 0;     // a scratch claim on the first `known` bytes; 0: nothing known, as of every fresh block
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), pinned(o.pinned), known(o.known) { o.forget(); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            (void)release();
            p = o.p, bytes = o.bytes, pinned = o.pinned, known = o.known;
            o.forget();
        }
        return *this;
    }
    ~DevBuf() { (void)release(); }
    // an empty buffer gets exactly `want` bytes (the growth rules are the callers': ensure, ensure_pinned, the rings, the slabs)
    hipError_t acquire(size_t want, bool pin) {
        const hipError_t e = pin ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want);
        if (e != hipSuccess) return p = nullptr, e;
        bytes = want, pinned = pin;
        res::up(pin ? res::kPinBlocks : res::kDevBlocks);
        res::up(pin ? res::kPinBytes : res::kDevBytes, want);
        return hipSuccess;
    }
    hipError_t release() {
        if (!p) return hipSuccess;
        res::down(pinned ? res::kPinBlocks : res::kDevBlocks);
        res::down(pinned ? res::kPinBytes : res::kDevBytes, bytes);
        void* gone = p;
        forget();
        return pinned ? hipHostFree(gone) : hipFree(gone);
    }
    // a device block on its way through raw pointers (a result's slab: akz_result.cpp); it stays counted in between
    static DevBuf adopt(void* block, size_t block_bytes) {
        DevBuf b;
        b.p = block, b.bytes = block_bytes;
        return b;
    }
    void* detach() {
        void* block = p;
        forget();
        return block;
    }

private:
    void forget() { p = nullptr, bytes = 0, known = 0; }
};
// An event / a stream: converts to the raw handle, so record, wait and launch sites spell it as they would the handle; ensure()
// creates it on first use.  A Stream may also BORROW a handle (the caller's stream of akz_ctx_create), which it never destroys.
struct Event {
    hipEvent_t h = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : h(o.h) { o.h = nullptr; }
    Event& operator=(Event&& o) noexcept {
        if (this != &o) reset(), h = o.h, o.h = nullptr;
        return *this;
    }
    ~Event() { reset(); }
    operator hipEvent_t() const { return h; }
    int ensure(unsigned flags = hipEventDisableTiming) {
        if (h) return AKZ_OK;
        AKZ_HIP_TRY(hipEventCreateWithFlags(&h, flags));
        res::up(res::kEvents);
        return AKZ_OK;
    }
    void reset() {
        if (!h) return;
        (void)hipEventDestroy(h);
        res::down(res::kEvents);
        h = nullptr;
    }
};
struct Stream {
    hipStream_t h = nullptr;
    bool owned = false;
    Stream() = default;
    Stream(Stream&& o) noexcept : h(o.h), owned(o.owned) { o.h = nullptr, o.owned = false; }
    Stream& operator=(Stream&& o) noexcept {
        if (this != &o) reset(std::move(o));
        return *this;
    }
    ~Stream() { reset(); }
    operator hipStream_t() const { return h; }
    int ensure() {  // (non-blocking, like every stream of the library)
        if (h) return AKZ_OK;
        AKZ_HIP_TRY(hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
        res::up(res::kStreams);
        owned = true;
        return AKZ_OK;
    }
    static Stream borrow(hipStream_t theirs) {
        Stream s;
        s.h = theirs;
        return s;
    }
    // a stream of another component that hands it over for good / takes it back (akz::place_streams_beside)
    static Stream adopt(hipStream_t theirs) {
        Stream s;
        s.h = theirs, s.owned = theirs != nullptr;
        if (s.owned) res::up(res::kStreams);
        return s;
    }
    hipStream_t detach() {
        if (h && owned) res::down(res::kStreams);
        hipStream_t out = h;
        h = nullptr, owned = false;
        return out;
    }
    void reset() {
        if (h && owned) {
            (void)hipStreamDestroy(h);
            res::down(res::kStreams);
        }
        h = nullptr, owned = false;
    }
    void reset(Stream&& fresh) {  // destroys what it owns and holds `fresh` from here on
        reset();
        h = fresh.h, owned = fresh.owned;
        fresh.h = nullptr, fresh.owned = false;
    }
};


// Pixels per launch (w * h * batch) from which a launch fills the chip on its own: the column-march kernels, the fork of
// the coarse chain and the resident coarse octave engage from here on (swept again in round 3: 4 Mpx is -7 ... -9 % on
// 8-frame batches, 8 000 000 -- so that a lone 4K frame qualifies -- changes nothing for it: that frame is bound by the
// host's per-image selection and the finish round trips, not by its kernels).
// From which job size (w*h*n pixels) a job takes the BATCH path -- column-march kernels, the coarse chain forked onto its own
// stream, the resident tail -- instead of the chain of tiled launches (profiles/r05_lone_ab.txt, one MI355X):
//   job            latency of one call   per job in a stream of jobs
//   1 x 1080p      0.98 / 1.21 ms        0.60 / 0.62 ms      (tiled chain / batch path)
//   1 x 2016x1512  1.21 / 1.28           0.77 / 0.67
//   2 x 1080p      1.42 / 1.51           0.90 / 0.78
//   3 x 1080p      1.76 / 1.78           1.09 / 0.92
//   1 x 4K         2.65 / 2.40           1.50 / 1.37
// Which jobs take the batch path (column marches, forked coarse chain, resident tail) is decided by job size per entry point:
// (the two values: akz_gates.hpp, gates::kBigPxSync / kBigPxAsync)
// The finish half of a lane's jobs on a thread of the library (akz_ctx_set_eager_finish): started by begin, so that the
// candidate round trip, the host keypoint logic and the keypoint kernels of frame i run while the caller's thread
// enqueues frame i + 1 on another lane; akz_extract_finish then only collects the result.  One thread per lane, jobs
// in the order they were begun.  Every other use of the lane (bind) first waits until the thread is idle, so the lane's
// state is never touched from two threads at once.
struct akz_job;
struct Finisher {
    std::thread th;
    std::mutex m;
    std::condition_variable wake, done;
    std::vector<akz_job*> queue;
    unsigned in_flight = 0;  // queued + running
    bool quit = false;
};

// akz_ctx::pin, the pinned host staging.  Ten buffers, two of them with two users that never overlap within a job: which allocation grows
// when is part of the latency behaviour, so the sharing stays as it is
enum Pin {
    PIN_LIST = 0,       // the candidate list, or the device selection's SelKpHost records
    PIN_COUNT_SUMS,     // the list's length (first word), later the orientation sums of the host's path
    PIN_ROWS,           // 64-byte descriptor rows
    PIN_PARAMS,         // keypoint parameters (KpParam)
    PIN_COSI,           // (cos, sin) per keypoint
    PIN_CONTRAST,       // contrast factors, one double per image
    PIN_REL,            // neighbour lists of the candidates
    PIN_REL_FLAGS,      // ... and their per-image flags
    PIN_SEL_HDR,        // the device selection's headers (akz_extract.hpp: kSel*)
    PIN_SPARE,          // (no user: the device selection's records carry their orientation sums)
    PIN_COUNT_
};
// The keys of akz_debug_set_schedule (include/akaze_hip_debug.h carries the same list): measurement hooks, results are identical.
//  0 SCHED_EARLY_STREAM     where the early stages (level-0 blur, contrast factor) of a batch whose input is complete run:
//                           0 = the copy stream if the stream-placement probe found it a hardware queue and a pipe of its own,
//                           1 = the copy stream regardless, 2 = a stream of their own (a fifth busy stream), 3 = the context's
//                           stream (no running ahead).  Default 0.
//  1 SCHED_EARLY_HOLD       what the early stages wait for: 0 = nothing, 1 = the fine-level diffusion of the batch before,
//                           2 = the first octave's diffusion of the batch before.  Default 1.
//  2 SCHED_NO_PROBE         1 = no stream-placement probe: streams stay as the runtime placed them.  Default 0.
//  3 SCHED_FORK_OCTAVE      the octave at which the coarse chain of a batch forks onto its own stream; 0 = octave 2.  Default 0.
//  4 SCHED_JOB_KPX          the job size in thousands of pixels (w*h*n) from which a job takes the batch path (column-march
//                           kernels, forked coarse chain, resident tail); the same value replaces lane_px, the size below which a
//                           context with lanes deals its jobs to them; 0 = the gates of akz_debug_gates (big_px_sync,
//                           big_px_async, lane_px).  Default 0.
//  5 SCHED_DET_BEHIND_LEVEL 1 = the column-march detector of a fine level right behind its level kernel, 0 = behind the whole
//                           fine chain (profiles/r06_interleave.txt).  Default 0.
//  6 SCHED_PREP_OWN_LAUNCH  1 = every level's preparation as a launch of its own and no tiled preparation family chosen per job,
//                           0 = on the tiled path the last diffusion launch of a level also prepares the next level of the
//                           octave (k_fed_own's epilogue).  Default 0.
//  7 SCHED_DET_BAND_ROWS    process-wide: the least interior rows of a band of the detector march -- how finely a small job's
//                           column marches are cut into workgroups; 0 = the planner's rule (40).  Default 0.
//  8 SCHED_LEVEL_BAND_ROWS  process-wide: the same for the level march, plus 1000 x the same for the level-0 marches; 0 = the
//                           planners' rules (level march: 20 below 48 Mpx per launch).  Default 0.
//  9 SCHED_FINISH_FORM      bit 0 = the waited-for job's headers, keypoint records and descriptor rows come to the host as three
//                           copies behind the descriptor kernel, clear = that kernel stores them into the host's pinned buffers
//                           itself; bit 1 = the keypoint kernels of a job that is alone in the context's hands on the auxiliary
//                           stream, as every other job's, clear = on the main stream, in order behind its detectors, when its
//                           chain ended there.  Default 0.
// 10 SCHED_HEAD_SPLIT       1 = level 0 of a tiled-family job as separate launches (blur, clearing of the contrast scratch, blur,
//                           maximum, histogram, percentile, and level 1's preparation as a k_prep launch), 0 = k_head +
//                           k_contrast_hist_final, and level 1's Lflow from k_head's Scharr pair.  Default 0.
// 11 SCHED_DET_SETS         how the column-march detectors of a range of levels are launched: 1 = one launch per level, 2 = one
//                           launch per set of up to four levels that share sigma_size, the width's parity and the kept planes
//                           (largest first), 0 = whichever of the two DESIGN.md 4 names the default, 11 .. 14 = sets, cut into
//                           1 .. 4 x 3 x CUs cells instead of kDetSetWaves x (process-wide: the sweep behind that constant).
//                           Default 0.
enum Sched {
    SCHED_EARLY_STREAM = 0,
    SCHED_EARLY_HOLD,
    SCHED_NO_PROBE,
    SCHED_FORK_OCTAVE,
    SCHED_JOB_KPX,
    SCHED_DET_BEHIND_LEVEL,
    SCHED_PREP_OWN_LAUNCH,
    SCHED_DET_BAND_ROWS,
    SCHED_LEVEL_BAND_ROWS,
    SCHED_FINISH_FORM,
    SCHED_HEAD_SPLIT,
    SCHED_DET_SETS,
    SCHED_COUNT_
};
// What a user sets on a context: one value, written by the setters on the context they are called on and handed to its lanes whole
// (lane_settings, push_settings below).  State that moves at run time (cand_cap_hint, the claims, the last-job fields) is not here.
struct CtxSettings {
    int det_mode = 2;  // 0: tiled pair, 2: auto, 4: one tiled kernel, 5: column march (akz_ctx_set_detector_mode)
    int prep_mode = 2;  // level preparation: 0 LDS-tiled, 1 streaming, 2 auto (fused with the first diffusion steps for large launches), 3 fused wherever supported
    int match_mode = 2;  // 0: popcount kernel, 1: matrix cores on int8 operands, 2 (default) / 3: on FP4 operands (akz_ctx_set_match_mode)
    int fed_mode = 2;  // 0: k_fed_step (1 step/launch), 2: k_fed_own (<= 8 steps/launch; <= 16 for small launches)
    uint64_t stream_min_px = gates::kStreamPx;  // pixels per launch (w*h*n) from which the streaming kernels pay off
    uint64_t big_px_sync = gates::kBigPxSync, big_px_async = gates::kBigPxAsync;  // (sched[SCHED_JOB_KPX] sets both: measurement)
    uint64_t lane_px = gates::kLanePx;  // jobs below it go to the lanes, if the context has any (sched[SCHED_JOB_KPX] sets it too)
    int profiling = 0;  // 0 off, 1 FED spans + host-clock stages, 2 every stage
    unsigned host_threads = 0;  // akz_ctx_set_host_threads; 0 = sized by host_cpu_share()
    uint32_t dbg_pair_chunks = 0, dbg_set_chunks = 0;  // akz_debug_set_match_chunks (0: automatic)
    uint32_t dbg_knn_chunks = 0;  // akz_debug_set_knn_chunks (0: automatic)
    int dbg_host_sort = -1;  // akz_debug_set_host_sort: 1 / 0 force the host / the device sort, -1 automatic
    int dbg_select = -1;  // akz_debug_set_select: 2 / 1 / 0 force the device / the neighbour-list / the grid selection, -1 automatic
    bool dbg_alloc_fill = false;  // akz_debug_set_alloc_fill: fresh device memory is filled with kAllocFillByte
    int dbg_device_libm = -1;  // akz_debug_set_device_libm: 0 = the host's libm always, -1 = automatic (device_libm_mode)
    int sched[SCHED_COUNT_] = {0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // akz_debug_set_schedule, indexed by Sched
};
static_assert(std::is_trivially_copyable<CtxSettings>::value, "lanes get the block by plain assignment");
// Everything a context owns of the runtime, and nothing else: handles only (no mutex, no atomic), so that the whole set is released
// by assigning an empty one (akz_ctx_destroy) -- a buffer, event or stream added here needs its declaration and nothing more.
struct CtxOwned {
    Stream stream;                           // the caller's stream, borrowed (akz_ctx_create); a lane's is its own (akz_ctx_set_lanes, place_lanes); what other threads synchronise with
    DevBuf scratch[6];                       // f32 plane temporaries (largest level x batch)
    DevBuf scratch_coarse;                   // the coarse chain's own diffusion scratch: it outlives the batch's join (see extract_begin)
    DevBuf lazy[6];                          // one-image planes of akz_fetch_plane's recomputation (never shared with scratch users)
    // Scratch CLAIMS: three buffers are read by a job for what an earlier job left in them, so that no clearing
    // launch is needed.  What is known of each is its DevBuf::known and nothing else: every (re)allocation and release starts it at
    // zero, the launch code drops it before it enqueues anything that dirties the range and raises it once the memset / the launches
    // that restore the content are enqueued, and akz_debug_audit_scratch checks every raised claim on the device.
    DevBuf small;                            // hmax bits / histogram / counters; claim: its first `known` bytes are zero (head_impl: its histogram pass leaves them so)
    DevBuf cand;                             // NMS candidates
    DevBuf cand_sorted, sort_scratch;        // the list in scan order (device sort of extract_finish) and the sort's scratch
    DevBuf rel_scratch;                      // the selection's neighbour lists (launch::candidate_relations)
    DevBuf sel_scratch, sel_recs;            // the selection on the device (launch::select_device): its scratch, the selected keypoints
    DevBuf bucket_scratch;                   // launch::sort_candidates_buckets; claim: its first `known` bytes (its counters) are zero
    DevBuf kp_in, kp_out;                    // keypoint params / orientation sums
    DevBuf match_a, match_b, match_out;
    DevBuf match_state;                      // k_match_merge_compact's per-workgroup counts (zeroed when allocated, then told apart by epoch);
                                             // single-stream: only ever touched by launches on `stream` (see match_device_impl);
                                             // claim: no word of its first `known` bytes carries an epoch beyond match_epoch
    DevBuf ransac_dev, ransac_pin;           // match_features: the trials' inputs and outputs on the device / pinned staging of both
    // akz_match_features_pairs: the sets' rows and x / y; raw lists, their counts and points; pair table and two slots of
    // trial samples; models and inlier counts; kept lists with their counts -- and the pinned staging of each
    DevBuf mp_in, mp_raw, mp_tab, mp_trials, mp_keep;
    DevBuf mp_pin_in, mp_pin_tab, mp_pin_smp[2], mp_pin_out;
    // guided matching (akz_guided_api.cpp): pair table | models, chunk records, lists of a call; pinned: table | models, counts
    DevBuf gd_tab, gd_rec, gd_out;
    DevBuf gd_pin_tab, gd_pin_cnt, gd_pin_out;
    // the cross-check (akz_cross_api.cpp): reverse lists | their counts | cross records of a call; pinned: the records
    DevBuf cx_rev, cx_pin_tab;
    // k-nearest-neighbour matching (akz_knn_api.cpp): the partial lists of a scan; rows | records | counts of a host-array call
    DevBuf kn_part, kn_io;
    // the keypoint budget (akz_budget_api.cpp): x | y | response | set table | block table, then rank | kept indices | radius2 of a
    // call; pinned: the upload's image, then kept indices | radius2.  No claim: every call initialises what its kernels accumulate into
    DevBuf kb_dev, kb_pin;
    Event kb_split_ev[4];                    // akz_debug_keypoint_budget_split: stage boundaries of a timed call
    Event mp_smp_ev[2];
    Event mp_split_ev[7];                    // akz_debug_match_pairs_split: stage boundaries of a timed call; akz_debug_resection_split uses the
                                             // first five for the resection call's (one call at a time runs on a context's stream)
    // The matcher's scratch, twice.  Side 0 serves every call on the context's stream (descriptor_match, the pairs calls, kNN);
    // akz_match_all_pairs runs the launches of consecutive lead images alternately there and on the finish stream with side 1
    // (akz::match_sets_at), so that the small launches around one image's pass (unpack, seed, compactions: 130 us of 550) run
    // under the other's
    struct MatchSide {
        DevBuf q8, t8, pop, tab;             // MFMA matcher: unpacked int8 images of the two sets, bit counts, set tables
        DevBuf cols;                         // both-direction launches: the train rows' (best, second) state, seed records and bound
        DevBuf rec;                          // chunk records [chunk][query], then the merged ones
        static constexpr int kRing = 4;
        DevBuf ring;                         // pinned staging ring of the multi-set matcher's tables: kRing slots of ring.bytes / kRing
        uint64_t ring_next = 0;
        Event ring_ev[kRing];
    } ms[2];
    DevBuf cosi;                             // (cos, sin) per keypoint
    DevBuf pin[PIN_COUNT_];                  // pinned host staging (enum Pin)
    std::vector<DevBuf> slab_pool;           // freed device blocks (pyramid slabs, descriptor rows), guarded by akz_ctx::slab_m
    // extractions in flight (akz_extract_begin_* / akz_extract_finish)
    static constexpr int kSlots = 3;
    DevBuf cand_slot[kSlots], count_slot[kSlots];
    DevBuf cand_mask_slot[kSlots];      // a masked job's list: what launch::mask_candidates keeps of cand_slot (same capacity; allocated by the first masked job of the slot; no claim)
    DevBuf mask_up;                     // akz_extract_gray_u8_masked: the host mask on the device for the length of that (synchronous) call; no claim
    Stream aux;                         // finish-side copies and keypoint kernels (created under aux_m: the caller's thread and the finisher's may both be first)
    Stream coarse;                      // the coarse octaves' chain (diffusion + detectors), next to the fine detectors
    Stream pre;                         // level-0 blur + contrast factor of a batch whose input is known to be complete:
    Event pre_done;                     // they run ahead, under the kernels of the batch before (extract_begin)
    Stream copy;                        // uploads of host frames (akz_extract_begin_host_*), under the kernels of the batch before
    DevBuf stage[kSlots];               // staging buffers of those uploads, one per job slot
    Event staged[kSlots];
    Event lane_in;                      // inputs of the job are ready on the caller's stream
    Event probe_ev[2];                  // stream placement (place_streams)
    struct Span { int stage; Event a, b; int row; };
    std::vector<Span> spans;          // recorded, not yet resolved
    std::vector<Event> ev_pool;       // recycled events (both guarded by akz_ctx::ev_m)
    // Every extract_begin records, behind its last fine-level diffusion launch, the event fed_ev[seq % kFedRing] of its
    // sequence number: the keypoint kernels of job i are held back until job i + 1 has passed that point, and the early
    // stages of job i + 1 until job i has (see extract_begin).  Four slots: at most kSlots jobs are in flight.
    static constexpr int kFedRing = 4;
    Event fed_ev[kFedRing];
    // ... and pre_ev[seq % kFedRing] behind the last diffusion launch of its FIRST octave: from there to the detectors the
    // main stream carries the half-resolution octave's launches, which are bound by latency and leave most of the chip's
    // bandwidth unused -- that is where the next job's blur and contrast passes go (sched[SCHED_EARLY_HOLD] = 2)
    Event pre_ev[kFedRing];
    // akz_fetch_pyramid (akz_result.cpp), private to it like `lazy`: the streams its downloads run on, the pinned staging ring
    // pageable destinations are filled through, and the recomputation of lean results -- temporaries that only the
    // context's stream touches, and two sets of outputs (Lxx, Lyy, Lxy, Lstep) that the downloads read alternately
    Stream fetch[2];                         // downloads alternate between two streams (two copy engines)
    DevBuf fetch_stage;                      // pinned: kFetchStageBufs buffers of kFetchStageBytes
    Event fetch_chunk[4];                    // a staging buffer's download is complete
    DevBuf fetch_tmp[3], fetch_out[2][4];
    Event fetch_start, fetch_join, fetch_ready[2], fetch_free[2];
    // JPEG reconstruction (akz_jpeg_api.cpp): pinned staging the host decoder writes coefficients (or a host-decoded luma
    // frame) into, one slot per decoding thread, each with the event of the upload that last read it; the device's
    // coefficients and component planes of the frame being reconstructed, the luma frames of a file-based extraction;
    // akz_ctx::jpeg_m orders the uploads of a batch's decoding threads on the stream
    static constexpr int kJpegSlots = 16;
    DevBuf jpeg_pin[kJpegSlots];
    Event jpeg_up[kJpegSlots];
    DevBuf jpeg_coef, jpeg_plane, jpeg_frames;
    // the resection (akz_resection_api.cpp): problem table | done | need | five planes (the upload), the rounds' state, then
    // kept counts | fits | trials | poses | kept indices (the read-back); pinned: the upload's image, the running count, the
    // read-back.  No claim: every call writes or clears what its kernels read.  (Last, and 64 bytes together: every member that
    // the extraction's threads share keeps its place within its cache line.)
    DevBuf rs_dev, rs_pin;
};
static_assert(std::is_nothrow_move_assignable<CtxOwned>::value && !std::is_copy_constructible<CtxOwned>::value, "released by assigning an empty one; never copied");
struct akz_ctx : CtxOwned {
    CtxSettings settings;  // a lane's: lane_settings(its parent's), kept so by push_settings
    int device = 0;
    std::atomic<uint32_t> last_total_kp{0};  // keypoints of the previous finished job (speculative fetch size of the device selection)
    std::atomic<int> sel_last_mode{-1};      // akz_debug_select_info: how the last finished job was selected (0 grids, 1 lists, 2 device), the
    std::atomic<int> sel_skip{0};            // jobs of shape sel_skip_shape that leave the device's selection out (the last one fell back)
    std::atomic<uint64_t> sel_skip_shape{0};
    std::atomic<uint32_t> sel_last_ticks[4];
    std::atomic<uint32_t> sel_last_rounds{0}, sel_last_fallback{0};  // device's longest run of rounds, images that sent it back to the host
    uint32_t match_epoch = 0;
    bool kb_split_on = false;
    double kb_split_ms[3] = {};
    bool mp_split_on = false;
    double mp_split_ms[6] = {};
    int libm_last = 0;          // how the last finished job got its angles: 0 host libm, 1 / 2 the device's FMA / SSE2 forms
    std::mutex slab_m;                  // guards slab_pool: results are freed by the caller while a lane's finisher thread allocates
    std::atomic<bool> slot_busy[kSlots] = {{false}, {false}, {false}};  // (begin on the caller's thread, finish possibly on the finisher's)
    std::atomic<uint32_t> cand_cap_hint{1u << 15};  // grows to 1.25x the largest candidate count seen
    std::atomic<int> live_results{0};   // akz_result objects (also inside jobs) and akz_bank objects that still point at this context
    bool dead = false;                  // akz_ctx_destroy was called; the struct lives until the last result is freed
    std::atomic<uint32_t> last_total_cands{0};  // candidates of the previous finished job (speculative fetch size)
    std::atomic<uint64_t> last_cand_shape{0};   // ... and its shape (akz_extract.hpp: shape_key)
    // akz_debug_mask_counts: the last finished masked job -- candidates before the mask, kept, NMS passes redone -- and when it
    // finished (a process-wide count: a context with lanes reports the latest of its own and theirs)
    std::atomic<uint64_t> mask_last[3] = {{0}, {0}, {0}}, mask_stamp{0};
    std::mutex aux_m;                   // guards the creation of aux
    // Lanes: child contexts (own streams, scratch planes, candidate slots) that small jobs are dealt to in turn, so that
    // the launch chains of consecutive single frames -- 44 back-to-back launches of a few hundred workgroups each --
    // overlap on the chip instead of queueing on one stream (akz_ctx_set_lanes).
    std::vector<akz_ctx*> lanes;
    unsigned next_lane = 0;
    bool is_lane = false;               // this context is a lane of another one
    bool eager_finish = true;           // akz_ctx_set_eager_finish (default on): the finish half of every job begun through
                                        // akz_extract_begin_* runs on the context's own thread (a lane's on the lane's)
    std::shared_ptr<Finisher> fin;      // (a lane's) finisher thread (shared with its jobs: one may outlive the context), started with its first eager job
    // Stream placement (place_streams): the runtime multiplexes a process's streams onto a few in-order hardware queues
    // (GPU_MAX_HW_QUEUES, 4 by default); two busy streams of a context on one queue serialise the whole pipeline, so the
    // first large batch measures which of the context's streams actually run side by side and replaces those that do not
    bool placed = false;
    int pre_mode = 0;            // early stages: 0 on the context's stream, 2 on the copy stream
    int place_replaced = 0;      // streams that were re-created because they shared a queue with another one
    int place_collisions = 0;    // pairs that still share a queue (no free queue was found)
    int place_retries = 0;       // probe measurements that were repeated because the first answer was "shared" or ambiguous
    int lane_collisions = 0;     // lanes whose stream still shares a queue or a pipe with another lane's
    akz_profile prof{};
    // akz_debug_kernel_rows: the spans of the two dominant stages by kernel variant and launch shape (what bench.py lists
    // behind roofline.kernel); a span's `row` indexes this table (-1: not broken down)
    std::vector<akz_kernel_row> rows;
    std::mutex ev_m;                  // guards spans and ev_pool (begin records on the caller's thread while a finish resolves)
    std::atomic<uint64_t> begin_seq{0};  // sequence number of the job begun last
    std::shared_ptr<std::atomic<int>> in_hand = std::make_shared<std::atomic<int>>(0);  // akz_job::in_hand
    std::unique_ptr<WorkerPool> workers;  // host threads of the finish half (started on first use)
    WorkerPool& pool() {
        if (!workers) workers.reset(new WorkerPool(std::min(settings.host_threads ? settings.host_threads : host_cpu_share(), 16u) - 1));
        return *workers;
    }
    std::mutex jpeg_m;                  // orders the uploads of a batch's JPEG decoding threads on the stream
    bool rs_split_on = false;           // akz_debug_resection_split
    double rs_split_ms[4] = {};
};
// What a lane runs with: its parent's settings, with the job gates no lower than lane_px (a job that is dealt to a lane runs there
// as a one-stream chain)
AKZ_LOCAL inline CtxSettings lane_settings(const CtxSettings& parent) {
    CtxSettings s = parent;
    for (uint64_t* big_px : {&s.big_px_sync, &s.big_px_async}) *big_px = std::max(*big_px, s.lane_px);
    return s;
}
// the end of every setter: what was written to c->settings reaches the lanes
AKZ_LOCAL inline void push_settings(akz_ctx* c) {
    for (akz_ctx* l : c->lanes) l->settings = lane_settings(c->settings);
}
// What a job decides for the launch helpers (akz_ops.cpp) it shares with the per-op entry points and the lazy recomputations.
// Everything else they depend on (fed_mode, det_mode, stream_min_px, sched[], profiling) is a context setting no job overrides.
struct JobForm {
    hipStream_t stream;     // the stream to enqueue on
    int prep_mode;          // the preparation mode in force (CtxSettings::prep_mode; extract_begin: 0 for jobs below gates::kTiledPrepPx)
    // pixels per LAUNCH (level w*h*n) from which the blur, the contrast passes and the detectors take their column-march
    // form: 8 Mpx (a 32 x 480x270 level: 41 us tiled against 66 for the march, which would run one strip per image row);
    // inside a batch-path job smaller than that, the job's own size -- its full-resolution launches march, the rest is tiled
    uint64_t march_min_px;
};
// outside a job: the context's stream, the mode as the user set it, the 8 Mpx gate
AKZ_LOCAL inline JobForm no_job_form(const akz_ctx* c) { return JobForm{c->stream, c->settings.prep_mode, gates::kMarchPx}; }

// akz_debug_kernel_rows stage of the JPEG rows: the reconstruction has no akz_profile stage of its own
constexpr int kStageIngest = 10;

// akz_debug_kernel_rows stage of the candidate sort's rows (extract_finish): counted, never timed -- no events, no akz_profile stage
constexpr int kStageSort = 11;
// the row of kernel variant (kind, param) on launches of shape (w, h, n) in c->rows, created on first use (under c->ev_m)
AKZ_LOCAL inline int kernel_row_locked(akz_ctx* c, int stage, uint32_t kind, uint32_t param, uint32_t w, uint32_t h, uint32_t n) {
    for (size_t i = 0; i < c->rows.size(); ++i) {
        const akz_kernel_row& r = c->rows[i];
        if (r.stage == (uint32_t)stage && r.kind == kind && r.param == param && r.w == w && r.h == h && r.n == n) return (int)i;
    }
    akz_kernel_row r{};
    r.stage = (uint32_t)stage, r.kind = kind, r.param = param, r.w = w, r.h = h, r.n = n;
    c->rows.push_back(r);
    return (int)c->rows.size() - 1;
}
// launches that are counted without a span (profiling on): which sort a job's candidates took
AKZ_LOCAL inline void kernel_row_count(akz_ctx* c, int stage, uint32_t kind, uint32_t w, uint32_t h, uint32_t n, uint64_t launches, uint64_t px) {
    if (!c->settings.profiling) return;
    std::lock_guard<std::mutex> lk(c->ev_m);
    akz_kernel_row& r = c->rows[(size_t)kernel_row_locked(c, stage, kind, 0, w, h, n)];
    r.launches += launches;
    r.px += px;
}

// RAII stage timer: device stages bracket the enqueued work with two events on the stream; they
// are resolved (hipEventElapsedTime) at the end of the extract call, after the final sync.
struct StageTimer {
    akz_ctx* c;
    int stage;
    Event a, b;
    static Event get(akz_ctx* c) {  // a timing event from the context's pool (an empty one if the runtime has none to give)
        Event e;
        {
            std::lock_guard<std::mutex> lk(c->ev_m);
            if (!c->ev_pool.empty()) {
                e = std::move(c->ev_pool.back());
                c->ev_pool.pop_back();
                return e;
            }
        }
        (void)e.ensure(hipEventDefault);
        return e;
    }
    bool on;
    hipStream_t s;
    int row = -1;
    StageTimer(akz_ctx* ctx, int st, hipStream_t stream) : c(ctx), stage(st), s(stream) {
        on = c->settings.profiling >= 2 || (c->settings.profiling == 1 && (st == AKZ_ST_FED || st == AKZ_ST_DETECTOR));
        if (!on) return;
        a = get(c);
        b = get(c);
        (void)hipEventRecord(a, s);
    }
    // the span belongs to kernel variant (kind, param) on launches of shape (w, h, n): `launches` launches over `px` level
    // pixels (x batch) that advance `px_steps` pixel-steps (FED kinds)
    void kernel(uint32_t kind, uint32_t param, uint32_t w, uint32_t h, uint32_t n, uint64_t launches, uint64_t px, uint64_t px_steps = 0) {
        if (!on) return;
        std::lock_guard<std::mutex> lk(c->ev_m);
        if (row < 0) row = kernel_row_locked(c, stage, kind, param, w, h, n);
        c->rows[(size_t)row].launches += launches;
        c->rows[(size_t)row].px += px;
        c->rows[(size_t)row].px_steps += px_steps;
    }
    ~StageTimer() {
        if (!on) return;
        (void)hipEventRecord(b, s);
        std::lock_guard<std::mutex> lk(c->ev_m);
        c->spans.push_back({stage, std::move(a), std::move(b), row});
    }
};
AKZ_LOCAL inline void ev_put(akz_ctx* c, Event&& e) {
    if (!e) return;
    std::lock_guard<std::mutex> lk(c->ev_m);
    c->ev_pool.push_back(std::move(e));
}
AKZ_LOCAL inline void resolve_spans(akz_ctx* c) {
    std::lock_guard<std::mutex> lk(c->ev_m);
    std::vector<akz_ctx::Span> pending;
    for (auto& sp : c->spans) {
        if (hipEventQuery(sp.b) != hipSuccess) {  // still in flight (a later job): keep for the next call
            pending.push_back(std::move(sp));
            continue;
        }
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            if (sp.stage < kStageIngest) c->prof.ms[sp.stage] += (double)ms;
            if (sp.row >= 0 && (size_t)sp.row < c->rows.size()) c->rows[(size_t)sp.row].ms += (double)ms;
        }
        c->ev_pool.push_back(std::move(sp.a));
        c->ev_pool.push_back(std::move(sp.b));
    }
    c->spans.swap(pending);
}
AKZ_LOCAL inline double now_ms() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec * 1e3 + (double)ts.tv_nsec * 1e-6;
}

// Wait for the context's streams before memory they may still use is freed: the caller's stream, the finish half's, and the
// side streams of the begin half (coarse chain, early stages, uploads).  The first failure is returned; every stream is waited for.
enum : unsigned { kSyncMain = 1, kSyncAux = 2, kSyncSide = 4, kSyncAll = 7 };
AKZ_LOCAL inline hipError_t sync_all_streams(akz_ctx* c, unsigned which = kSyncAll) {
    hipError_t first = hipSuccess;
    auto wait = [&](hipStream_t s) {
        const hipError_t e = hipStreamSynchronize(s);
        if (first == hipSuccess) first = e;
    };
    if (which & kSyncMain) wait(c->stream);
    if ((which & kSyncAux) && c->aux) wait(c->aux);
    for (hipStream_t s : {c->coarse.h, c->pre.h, c->copy.h})
        if ((which & kSyncSide) && s) wait(s);
    return first;
}
// akz_debug_set_alloc_fill: what hipMalloc returned holds 0xA5 bytes before anybody sees it (a debug mode: a fill and a wait)
constexpr int kAllocFillByte = 0xA5;
AKZ_LOCAL inline hipError_t alloc_fill(const akz_ctx* c, void* p, size_t bytes) {
    if (!c->settings.dbg_alloc_fill) return hipSuccess;
    const hipError_t e = hipMemset(p, kAllocFillByte, bytes);
    return e != hipSuccess ? e : hipDeviceSynchronize();
}
AKZ_LOCAL inline int ensure(akz_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return AKZ_OK;
    if (b.p) {
        AKZ_HIP_TRY(sync_all_streams(c));
        AKZ_HIP_TRY(b.release());
    }
    const size_t want = bytes + bytes / 8 + 256;
    AKZ_HIP_TRY(b.acquire(want, false));  // (fresh memory holds nothing known: b.known is 0)
    AKZ_HIP_TRY(alloc_fill(c, b.p, want));
    return AKZ_OK;
}
AKZ_LOCAL inline int ensure_pinned(akz_ctx* c, DevBuf& b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return AKZ_OK;
    if (b.p) {  // (the caller's stream and the finish half's only, as ever: every user of pinned staging synchronises its stream before it returns)
        AKZ_HIP_TRY(sync_all_streams(c, kSyncMain | kSyncAux));
        AKZ_HIP_TRY(b.release());
    }
    AKZ_HIP_TRY(b.acquire(bytes + bytes / 4 + 4096, true));
    return AKZ_OK;
}
// The auxiliary stream carries the finish-side copies and the per-keypoint kernels.  (A lowest-priority
// stream was measured and made no difference to the main-stream kernels, so it is a plain stream.)
AKZ_LOCAL inline int ensure_aux(akz_ctx* c) {
    // (the matcher's entry points bind without draining the finisher thread, whose finish half creates the stream too)
    std::lock_guard<std::mutex> lk(c->aux_m);
    return c->aux.ensure();
}
// wait until the context's finisher thread (if any) has nothing queued or running; a no-op on that thread itself
AKZ_LOCAL inline void finisher_drain(akz_ctx* c) {
    Finisher* f = c->fin.get();
    if (!f || f->th.get_id() == std::this_thread::get_id()) return;
    std::unique_lock<std::mutex> lk(f->m);
    f->done.wait(lk, [&] { return f->in_flight == 0; });
}
AKZ_LOCAL inline void finisher_stop(akz_ctx* c) {
    Finisher* f = c->fin.get();
    if (!f) return;
    {
        std::unique_lock<std::mutex> lk(f->m);
        f->done.wait(lk, [&] { return f->in_flight == 0; });
        f->quit = true;
    }
    f->wake.notify_all();
    if (f->th.joinable()) f->th.join();
    c->fin.reset();
}
// drain_self = false: extract_begin on a context whose jobs are finished by its own thread -- the two halves touch disjoint
// state (see akz_ctx) and run side by side; every other entry point waits until that thread is idle
AKZ_LOCAL inline int bind(akz_ctx* c, bool lanes_too = true, bool drain_self = true) {
    if (!c) {
        set_error("null context");
        return AKZ_ERR_INVALID_ARG;
    }
    if (c->dead) {
        set_error("the context of this object was destroyed");
        return AKZ_ERR_INVALID_ARG;
    }
    if (drain_self) finisher_drain(c);
    if (lanes_too)  // (every call but the one that deals a job to a lane: setters forward to the lanes, queries read them)
        for (akz_ctx* l : c->lanes) finisher_drain(l);
    AKZ_HIP_TRY(hipSetDevice(c->device));
    // The HIP runtime keeps ONE last-error slot per thread, shared with every other user of the runtime in the
    // process (PyTorch probes that fail on purpose, ...): drop whatever is in it so that the hipGetLastError()
    // checks after this entry point's launches report this entry point's errors only.
    (void)hipGetLastError();
    return AKZ_OK;
}


// ---- shared between the translation units of the C ABI ----------------------------------------------------------------
AKZ_LOCAL inline size_t plane_bytes(uint32_t w, uint32_t h, uint32_t n) { return (size_t)w * h * n * sizeof(float); }
// akz_api.cpp
AKZ_LOCAL int level_info_out(const std::vector<LevelPlan>& plan, uint64_t level, double* etime, double* esigma, uint32_t* octave,
                   uint32_t* sublevel, uint32_t* sigma_size, uint32_t* lw, uint32_t* lh, uint32_t* det_sigma, uint64_t* n_tau,
                   double* tau, uint64_t tau_cap);
// akz_ops.cpp: the launch helpers behind the per-op entry points, which the extraction pipeline calls as well
template <typename T>
AKZ_LOCAL int gaussian_blur_impl(akz_ctx* c, const JobForm& f, const T* d_in, float* d_out, uint32_t w, uint32_t h, uint32_t n, float sigma);
// level 0 of a small job in two launches (k_head, k_contrast_hist_final); *fused = false: not this job (the separate stages follow)
template <typename T>
AKZ_LOCAL int head_impl(akz_ctx* c, const JobForm& f, const T* d_in, float* d_lt0, float* d_blurred, float* d_gx, float* d_gy, uint32_t w, uint32_t h, uint32_t n,
                        float sigma0, double percentile, double gscale, uint64_t nbins, double* d_k_out, bool* fused, uint32_t* d_zero_word = nullptr);
AKZ_LOCAL int contrast_impl(akz_ctx* c, const JobForm& f, const float* d_in, uint32_t w, uint32_t h, uint32_t n, double percentile, double gscale, uint64_t nbins,
                  double* d_k_out);
AKZ_LOCAL uint32_t fed_max_fuse(const akz_ctx* c, uint32_t w, uint32_t h, uint32_t n);
AKZ_LOCAL uint32_t fed_num_launches(const akz_ctx* c, uint32_t n_tau, uint32_t w, uint32_t h, uint32_t n);
AKZ_LOCAL float* fed_dst(uint32_t launches, uint32_t k /*1-based*/, float* A, float* B);
// next / next_done: the last launch may also prepare the NEXT level (launch::fed_fused's epilogue); *next_done says whether it did
AKZ_LOCAL int fed_impl(akz_ctx* c, const JobForm& f, const float* in, float* A, float* B, const float* lflow, float* lstep, uint32_t w, uint32_t h, uint32_t n,
             const double* taus, uint32_t n_tau, const launch::FedNextPrep* next = nullptr, bool* next_done = nullptr);
AKZ_LOCAL int detector_family(const akz_ctx* c, const JobForm& f, uint32_t sigma, uint32_t w, uint32_t h, uint32_t n, float border_m,
                    bool nms = true);
AKZ_LOCAL int detector_impl(akz_ctx* c, const JobForm& f, const float* lsmooth, uint32_t sigma, float* lx, float* ly, float* lxx, float* lyy, float* lxy,
                  float* ldet_out, uint32_t w, uint32_t h, uint32_t n);
// akz_place.cpp
AKZ_LOCAL int place_streams(akz_ctx* c);
// akz_match_api.cpp: the tail of every scan of one train set -- merge of the chunk records, ratio test, ordered compaction
AKZ_LOCAL int match_finish(akz_ctx* c, MatchRec* rec, uint32_t n0, uint32_t chunks, uint32_t thr, double lowes_ratio, akz_match* d_out,
                           uint64_t* d_n_out);
// ---- the pairs calls (akz_match_api.cpp, akz_match_seeded_api.cpp, akz_guided_api.cpp) -----------------------------------
struct GuidedPairSpec {
    uint64_t q_row0, n0, t_row0, n1, out_off;
};
struct GuidedStage {  // the second stage of akz_match_features_{homography,fundamental}_guided(_pairs)
    float radius;
    double ratio;
};
struct PoseStage {  // the pose stage of akz_match_features_seeded_pose_pairs: launch::pairs_pose after the refit (akz_pose.hip)
    const akz_camera* d_cameras;  // two per pair (image 0, image 1), on the device (the front's own bytes)
    akz_pose* poses;              // one per pair
    float* points;                // 3 floats per slot of out, may be null
};
struct RefineStage {  // the refit stage of akz_match_features_{homography,fundamental}_refined(_pairs): launch::model_refit after the pick
    uint32_t max_iterations;
    uint32_t* iterations;  // one per pair, may be null
};
// The inputs of a pairs call as its entry point got them.  bank: the sets lie in a feature bank; sets, n_sets and desc_bytes are then the
// bank's (counts alone, both pointers of a set null).  Null: the caller's sets.
struct PairsCall {
    const char* name;  // the prefix of the entry point's error texts
    akz_ctx* c;
    const akz_feature_set* sets;
    uint64_t n_sets;
    const uint64_t* pairs;
    uint64_t n_pairs, desc_bytes;
    akz_match* out;
    uint64_t* n_out;
    const akz_bank* bank;
};
// What the opening of a pairs call leaves to the rest of it.  pairs_open fills the first group, pairs_front the second.
struct AKZ_LOCAL PairsFront {
    SetsBlock block;             // the sets a pair names in c->mp_in, or the bank's block (akz_pairs_layout.hpp)
    std::vector<uint64_t> used;  // the sets to upload, in order of first use; none over a bank
    uint64_t cap1 = 0;           // the room of `out` (sum of the first sets' descriptors), at least 1
    size_t b_cnt = 0;

    bool timed = false;                    // akz_debug_match_pairs_split is on
    std::vector<launch::PairJobHost> tab;  // one record per pair; raw_off, kp0_off, kp1_off and cnt_idx filled in
    akz_match* d_raw = nullptr;            // c->mp_raw = raw lists | counts | points
    uint64_t* d_cnt = nullptr;
    float* d_pts = nullptr;
    launch::PairJobHost *d_tab = nullptr, *h_tab = nullptr;  // c->mp_tab = table | the caller's bytes; c->mp_pin_tab = table | counts | the caller's
    uint64_t* h_cnt = nullptr;                               // (read back; valid after the caller's synchronise)
    char *d_own = nullptr, *h_own = nullptr;
};
// (PairsKeep, the kept block of c->mp_keep and c->mp_pin_out: akz_pairs_layout.hpp)
// A feature bank (akz_bank_api.cpp; include/akaze_hip.h): feature sets resident on the device in the layout the pairs calls scan --
// `dev` is the SetsBlock `block`, every set placed in index order.  Immutable once created.  It owns `dev` and counts among its
// context's live objects (akz_ctx::live_results), as a result does.
struct akz_bank {
    akz_ctx* ctx = nullptr;
    uint64_t desc_bytes = 0;
    std::vector<akz_feature_set> sets;  // the counts of every set; both pointers null
    SetsBlock block;
    DevBuf dev;
    // a bank under a keypoint budget (akz_bank_create_from_*_budget): the block has its src part, block.d_src[r] = the index in its source
    // set of the keypoint row r came from, and `src` is its host copy (akz_bank_set_indices).  Both absent otherwise: the identity.
    bool budgeted = false;
    std::vector<uint32_t> src;
};
// akz_budget_api.cpp: the keypoint budget's refusals and its plan / enqueue half, shared with the budgeted bank (akz_bank_api.cpp).
// budget_options_ok: every refusal that does not depend on a set's keypoints; budget_set_ok: those of one set, which `what` names
// ("" or "set 3: "); `name` ends in ": ".  budget_enqueue: over checked sets of at most kBudgetMaxKeypoints keypoints together
// (only keypoints / n_keypoints are read) -- the set and block tables, the ONE upload of x | y | response and the tables, and
// launch::budget, on the context's stream; it neither copies back nor synchronises.  Afterwards set s has its x, y and response at
// [tab[s].base, + n) of d_x, d_y, d_r and its tab[s].keep kept indices, ascending, at d_idx + tab[s].out_off; h_down: b_idx +
// 4 * total bytes of pinned memory for the caller's read-back (kept indices | radius2).
constexpr uint64_t kBudgetMaxKeypoints = 0x7fffffffull;
AKZ_LOCAL bool budget_options_ok(const char* name, const akz_keypoint_budget* opt, const void* indices, const void* n_out, const void* radius2);
AKZ_LOCAL bool budget_set_ok(const char* name, const std::string& what, const akz_keypoint* k, uint64_t n);
struct BudgetPlan {
    std::vector<launch::BudgetSet> tab;
    uint32_t total = 0, kept = 0;
    const float *d_x = nullptr, *d_y = nullptr, *d_r = nullptr;
    uint32_t* d_idx = nullptr;  // `kept` indices, then (b_idx bytes on) the radius2 of all `total` keypoints
    size_t b_idx = 0;
    char* h_down = nullptr;
};
AKZ_LOCAL int budget_enqueue(akz_ctx* c, const akz_feature_set* sets, uint64_t n_sets, const akz_keypoint_budget& o, BudgetPlan& p);
// akz_match_api.cpp.  set_refusal: what every call refuses of one feature set, without the prefix that says where (null: nothing).
// table_upload: a host table to the device through pinned staging, on the context's stream.
// pairs_open: the refusals (guided: those of the guided scan too), bind, the placement of every distinct set in order of first use and
// the room for its rows.  pairs_front: the opening, the upload, the scans (cross: both directions and launch::pairs_cross_filter), the
// table, launch::pair_points and the enqueued read-back of the counts -- it does not synchronise.  b_dev_own / b_pin_own: the caller's
// bytes behind the table in c->mp_tab and behind the counts in c->mp_pin_tab.
// Over a bank (q.bank) the opening is pairs_open_bank -- the refusals a bank leaves to make, bind, and f.block is the bank's own;
// nothing is placed or uploaded and c->mp_in / c->mp_pin_in are not touched.  Without one the call enqueues what it always did.
AKZ_LOCAL const char* set_refusal(const akz_feature_set& s);
AKZ_LOCAL inline int table_upload(akz_ctx* c, void* d_dst, void* h_pin, const void* tab, size_t bytes) {
    std::memcpy(h_pin, tab, bytes);
    AKZ_HIP_TRY(hipMemcpyAsync(d_dst, h_pin, bytes, hipMemcpyHostToDevice, c->stream));
    return AKZ_OK;
}
AKZ_LOCAL int pairs_open(const PairsCall& q, bool guided, PairsFront& f);
AKZ_LOCAL int pairs_open_bank(const PairsCall& q, bool guided, PairsFront& f);
// the sets `order` names: rows (padded to 64 bytes) and the x / y of their first n_descriptors keypoints, through c->mp_pin_in
// (laid out as b) to where b is bound
AKZ_LOCAL int pairs_upload(akz_ctx* c, const akz_feature_set* sets, uint64_t desc_bytes, const SetsBlock& b, const std::vector<uint64_t>& order);
AKZ_LOCAL int pairs_front(const PairsCall& q, double lowes_ratio, bool guided, bool cross, size_t b_dev_own, size_t b_pin_own, PairsFront& f);
AKZ_LOCAL int pairs_table_upload(akz_ctx* c, PairsFront& f);  // f.tab -> f.d_tab through f.h_tab
AKZ_LOCAL int pairs_keep(akz_ctx* c, const PairsFront& f, uint64_t n_keep, PairsKeep& k);
// pairs_tail: launch::pairs_pick_filter over the trials' models and counts (d_mdl, d_inl), launch::model_refit given `refine`,
// launch::pairs_pose given `pose`, the ONE read-back of head and kept lists, the guided stage given `guided`, the synchronise, the copy-out and the intervals of a timed call
// (t_host: the caller's host time, interval 2).  model .. trials_run: one per pair, each may be null.
AKZ_LOCAL int pairs_tail(const PairsCall& q, const PairsFront& f, const PairsKeep& k, launch::RansacModel kind, const float* d_mdl,
                         const int32_t* d_inl, float epsilon_inliers, const RefineStage* refine, float refit_epsilon, const GuidedStage* guided,
                         int guided_kind, double t_host, float* model, int* found, uint32_t* fits, uint64_t* trials_run,
                         const PoseStage* pose = nullptr);
// the lists of a pairs call to out / n_out: pair p's guided list (h_gcnt[p] records at its fixed place in d_gout, fetched by ONE read-back
// of the span such lists occupy) where h_gcnt is given and h_found is null or h_found[p] set, else its kept list (h_kcnt, h_keep, tab)
AKZ_LOCAL int pairs_copy_out(const PairsCall& q, const uint64_t* h_gcnt, const int32_t* h_found, const akz_match* d_gout, const uint64_t* h_kcnt,
                             const akz_match* h_keep, const launch::PairJobHost* tab);
// akz_match_api.cpp: the descriptor scans of every pair over the sets placed in b; fills the pair records' raw_off, kp0_off, kp1_off, cnt_idx
// -- and, given `cross`, the opposite direction of every pair to d_rev / d_rcnt with the records of launch::pairs_cross_filter
AKZ_LOCAL int pairs_scans(const PairsCall& q, double lowes_ratio, const SetsBlock& b, akz_match* d_raw, uint64_t* d_cnt,
                          std::vector<launch::PairJobHost>& tab, akz_match* d_rev = nullptr, uint64_t* d_rcnt = nullptr,
                          std::vector<launch::CrossJobHost>* cross = nullptr, uint64_t distance_threshold = 10000);
// akz_guided_api.cpp: the guided scan of many pairs whose sets lie on the device in b, enqueued on the
// context's stream -- scan, merge, ratio test and ordered compaction; pair p's list goes to d_out + spec[p].out_off, its
// length to d_cnt[p].  d_models: 9 floats per pair ON THE DEVICE; d_found (optional): pairs whose flag is 0 give empty lists.
// guided_specs: every pair's rows as placed in b, its list at the fixed place out / d_out give it.
AKZ_LOCAL int guided_limits(const char* name, const akz_feature_set* sets, const uint64_t* pairs, uint64_t n_pairs,
                            const std::vector<uint8_t>& seen);
AKZ_LOCAL std::vector<GuidedPairSpec> guided_specs(const PairsCall& q, const SetsBlock& b);
AKZ_LOCAL int guided_enqueue(akz_ctx* c, const std::vector<GuidedPairSpec>& spec, const SetsBlock& b, int kind, const float* d_models,
                             const int32_t* d_found, float radius, uint64_t distance_threshold, double lowes_ratio, akz_match* d_out,
                             uint64_t* d_cnt);
// akz_match_seeded_api.cpp: the seeded pairs call; cross: with cross(A, B) as every pair's raw list (akz_cross_api.cpp); pose: with the
// pose stage behind it (akz_pose_api.cpp)
struct SeededPose {
    const akz_camera* cameras;  // one per set, the caller's
    akz_pose* poses;            // one per pair
    float* points;              // may be null
};
AKZ_LOCAL int match_seeded_pairs_impl(const PairsCall& q, bool cross, const akz_ransac_options* options, float* model, int* found,
                                      uint32_t* iterations, uint64_t* trials_run, const SeededPose* pose = nullptr);
// akz_match_seeded_api.cpp: the rounds of every seeded call (the pairs calls, akz_resection_seeded_problems) over n entries -- pairs or
// problems -- with models of model_floats floats.  SeededState is what the rounds keep: on the device every entry's best model and
// count, its ring of a round's models and counts and the running counts per round (bytes() at place()'s address; clear() enqueues the
// two memsets), and the caller's tables(): done | need (one window of rounds per entry; none without a stopping rule) on the device
// and pinned, and a pinned word for the count read back.  d_trials: the trials-run words on the device.
struct SeededState {
    static constexpr uint32_t kWindow = 8;  // rounds enqueued between two looks at the entries still running
    uint64_t n;
    uint32_t model_floats, max_trials, n_rounds;
    double confidence;
    size_t b_bm, b_bi, b_rm, b_ri, b_run, b_done, b_need;
    float *d_bm = nullptr, *d_rm = nullptr;
    int32_t *d_bi = nullptr, *d_ri = nullptr;
    uint32_t *d_run = nullptr, *d_done = nullptr, *d_need = nullptr /* stays null: no stopping rule */, *d_trials = nullptr;
    uint32_t *h_done = nullptr, *h_need = nullptr, *h_run = nullptr;
    SeededState(uint64_t n, uint32_t model_floats, const akz_ransac_options& opt);
    bool stopping() const { return confidence > 0.0; }
    size_t bytes() const { return b_bm + b_bi + b_rm + b_ri + b_run; }
    void place(void* d_state);
    void tables(void* d_done_need, void* h_done_need, void* h_word);
    int clear(hipStream_t st) const;
};
// seeded_rounds_device: need[entry][k] (seeded_need over n_of(entry) elements, samples of K) for the first window of the entries with
// h_done == 0; upload() -- the caller's: what it enqueues between the tables and the first round, done | need among it --; then while
// entries run the rounds: round(r) -- the caller's launch into the ring --, launch::seeded_update, and after every window the read of
// running[r] and the next table.  t_need (optional) grows by the time spent on the tables.
AKZ_LOCAL int seeded_rounds_device(hipStream_t st, SeededState& s, int K, uint64_t n_running, const std::function<uint64_t(uint64_t)>& n_of,
                            const std::function<int()>& upload, const std::function<void(uint32_t)>& round, double* t_need = nullptr);
// akz_pose_api.cpp: the refusals of akz_match_features_seeded_pose_pairs that are not the seeded call's
AKZ_LOCAL int pose_pairs_refusals(const char* name, const akz_ransac_options* options, const akz_camera* cameras, uint64_t n_sets,
                                  const akz_pose* poses);
// ... and the one camera rule of every call that takes an akz_camera (akz_recover_pose_host's): finite fields, fx and fy not zero
AKZ_LOCAL bool camera_ok(const akz_camera& k);
// akz_extract_finish.cpp
AKZ_LOCAL int device_libm_mode(akz_ctx* c);  // 0: host libm; 1 / 2: the device's FMA / SSE2 forms reproduce it (akz_libm.hpp)
