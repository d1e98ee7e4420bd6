/* Measurement and test hooks of libakaze_hip.so: NOT part of the drop-in boundary (include/akaze_hip.h).  A host that
   replaces the reference crate never needs these; the bench, the tools and the tests do.  Same conventions (status-code
   returns, no exceptions across the ABI). */
#ifndef AKAZE_HIP_DEBUG_H
#define AKAZE_HIP_DEBUG_H
#include "akaze_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Is the begin phase of an extraction (scale space + detector + extrema of a batch: ~45 dependent launches for a lone
   1080p frame) shorter as ONE hipGraph launch?  Captures it for (d_imgs, w, h, n, cfg) and times `reps` graph launches
   against `reps` plain enqueues, each from an idle stream (HIP events): *ms_graph, *ms_plain per launch, *graph_nodes
   (may be NULL) the node count.  Results of the probe's extractions are discarded. */
int akz_ctx_graph_probe(akz_ctx* ctx, const uint8_t* d_imgs, uint32_t w, uint32_t h, uint32_t n, const akz_config* cfg,
                        uint32_t flags, uint32_t reps, double* ms_graph, double* ms_plain, uint64_t* graph_nodes);
/* Diagnostics (host only, no GPU work): the row bands the column-march planners cut an n-image batch of w x h into.
   kind 0: detector / blur march with filter half width `half_width` (interior rows half_width .. h-1-half_width),
   kind 1: level march (interior rows 1 .. h-2; first and last band shorter).  Writes up to `cap` (first, end) row pairs
   to rows, the number of bands to *n_bands.  Used by the CPU tests to check that the bands tile the rows exactly. */
int akz_debug_march_bands(int kind, uint32_t w, uint32_t h, uint32_t n, int half_width, int32_t* rows, uint32_t cap,
                          uint32_t* n_bands);
/* Diagnostics (host only, no GPU work): one k_detector_march launch over a SET of n_entries <= 4 levels (w[e] x h[e], n
   images each, largest first) as the planner cuts it and as the kernel's prologue decodes it.  cells[4 i ..] = (entry, image,
   band, strip) of workgroup i, all -1 for a padding workgroup (every entry's cell count is rounded up to a multiple of 8;
   XCD i & 7 walks a contiguous eighth of every entry); up to `cap` workgroups are written.  grids[3 e ..] = (strips, bands,
   interior rows per band) of entry e; *n_workgroups = the grid size.  Used by the CPU tests. */
int akz_debug_detector_set_cells(int half_width, const uint32_t* w, const uint32_t* h, uint32_t n_entries, uint32_t n, int32_t* cells,
                                 uint32_t cap, int32_t* grids, uint32_t* n_workgroups);
/* names of the default FED kernel and of the detector kernel that large launches take (for bench / profiles) */
const char* akz_fed_kernel_name(void);
const char* akz_detector_kernel_name(void);
/* Test hook: force the chunk counts of the matrix-core matcher (train rows per workgroup column): `pair_chunks` for a
   pair call, `set_chunks` (1..16) per set of a multi-set call; 0 = automatic (the default).  Results are identical for
   every value -- which is what the tests that use this check. */
int akz_debug_set_match_chunks(akz_ctx* ctx, uint32_t pair_chunks, uint32_t set_chunks);
/* Test hook: the train rows per LDS tile of the matrix-core matcher (launch::match_mfma_tile_rows()), so that tests can place
   their set sizes one below, at and one above it.  No GPU call, no context. */
int akz_debug_match_tile_rows(uint32_t* rows);
/* Test hook: the query rows that seed the opposite direction of akz_descriptor_match_sets_mutual_device for a query set of n0
   rows (launch::match_cols_seed_rows(n0): min(n0, AKZ_MM_SEED_TILES tiles)); the rows from there on enter through the atomic
   candidate path, so tests can plant rows on both sides of that boundary.  No GPU call, no context. */
int akz_debug_match_seed_rows(uint32_t n0, uint32_t* rows);
/* Test hook: force the number of train chunks of the k-nearest-neighbour scan (akz_descriptor_match_knn*), so that tests reach
   the merge of the chunks' partial lists at a few hundred rows; 0 = automatic (the default).  The counterpart of pair_chunks
   above.  Results are identical for every value. */
int akz_debug_set_knn_chunks(akz_ctx* ctx, uint32_t chunks);
/* Measurement hook: schedule variants (results are identical).  A context with lanes (akz_ctx_set_lanes) hands every key to them,
   whichever of the two calls comes first.  Keys outside 0 .. 11 are refused.  The keys (csrc/akz_ctx.hpp carries the same list above its enum Sched):
    0 SCHED_EARLY_STREAM     where the early stages (level-0 blur, contrast factor) of a batch whose input is complete run:
                             0 = the copy stream if the stream-placement probe found it a hardware queue and a pipe of its own,
                             1 = the copy stream regardless, 2 = a stream of their own (a fifth busy stream), 3 = the context's
                             stream (no running ahead).  Default 0.
    1 SCHED_EARLY_HOLD       what the early stages wait for: 0 = nothing, 1 = the fine-level diffusion of the batch before,
                             2 = the first octave's diffusion of the batch before.  Default 1.
    2 SCHED_NO_PROBE         1 = no stream-placement probe: streams stay as the runtime placed them.  Default 0.
    3 SCHED_FORK_OCTAVE      the octave at which the coarse chain of a batch forks onto its own stream; 0 = octave 2.  Default 0.
    4 SCHED_JOB_KPX          the job size in thousands of pixels (w*h*n) from which a job takes the batch path (column-march
                             kernels, forked coarse chain, resident tail); the same value replaces lane_px, the size below which a
                             context with lanes deals its jobs to them; 0 = the gates of akz_debug_gates (big_px_sync,
                             big_px_async, lane_px).  Default 0.
    5 SCHED_DET_BEHIND_LEVEL 1 = the column-march detector of a fine level right behind its level kernel, 0 = behind the whole
                             fine chain (profiles/r06_interleave.txt).  Default 0.
    6 SCHED_PREP_OWN_LAUNCH  1 = every level's preparation as a launch of its own and no tiled preparation family chosen per job,
                             0 = on the tiled path the last diffusion launch of a level also prepares the next level of the
                             octave (k_fed_own's epilogue).  Default 0.
    7 SCHED_DET_BAND_ROWS    process-wide: the least interior rows of a band of the detector march -- how finely a small job's
                             column marches are cut into workgroups; 0 = the planner's rule (40).  Default 0.
    8 SCHED_LEVEL_BAND_ROWS  process-wide: the same for the level march, plus 1000 x the same for the level-0 marches; 0 = the
                             planners' rules (level march: 20 below 48 Mpx per launch).  Default 0.
    9 SCHED_FINISH_FORM      bit 0 = the waited-for job's headers, keypoint records and descriptor rows come to the host as three
                             copies behind the descriptor kernel, clear = that kernel stores them into the host's pinned buffers
                             itself; bit 1 = the keypoint kernels of a job that is alone in the context's hands on the auxiliary
                             stream, as every other job's, clear = on the main stream, in order behind its detectors, when its
                             chain ended there.  Default 0.
   10 SCHED_HEAD_SPLIT       1 = level 0 of a tiled-family job as separate launches (blur, clearing of the contrast scratch, blur,
                             maximum, histogram, percentile, and level 1's preparation as a k_prep launch), 0 = k_head +
                             k_contrast_hist_final, and level 1's Lflow from k_head's Scharr pair.  Default 0.
   11 SCHED_DET_SETS         how the column-march detectors of a range of levels are launched: 1 = one launch per level, 2 = one
                             launch per set of up to four levels that share sigma_size, the width's parity and the kept planes
                             (largest first), 0 = whichever of the two DESIGN.md 4 names the default, 11 .. 14 = sets, cut into
                             1 .. 4 x 3 x CUs cells instead of kDetSetWaves x (process-wide: the sweep behind that constant).
                             Default 0. */
int akz_debug_set_schedule(akz_ctx* ctx, int key, int value);
/* What the stream-placement probe of the context's first large batch found: info[0] = it has run, info[1] = early stages on
   the context's stream (0) or the copy stream (2), info[2] = streams it re-created because they shared a hardware queue
   or a command-processor pipe with another busy stream of the context, info[3] = streams that still share one. */
int akz_debug_stream_placement(akz_ctx* ctx, int* info);
/* The probe's decision as a pure function of its timings (host only, no GPU): bit 0 = the two streams share a hardware
   queue, bit 1 = a command-processor pipe, bit 2 = too close to a threshold to trust a single measurement (the probe then
   repeats it and lets the shortest decide).  spin_pair_ms: two spins of spin_ms each on two streams, first start to second
   end; tiny_pair_ms: 24 + 24 interleaved tiny kernels on the two streams (negative: not measured); tiny_alone_ms: 24 of
   them on one stream. */
int akz_debug_placement_verdict(float spin_pair_ms, float tiny_pair_ms, float tiny_alone_ms, float spin_ms);
/* The orientation's libm calls ON the device.  The reference's angle is atan2f of two sums, its descriptor pattern is rotated
   by cosf / sinf of that angle -- the platform's libm, i.e. glibc's float routines on the machine the reference runs on.
   csrc/akz_libm.hpp states those routines (glibc 2.35: fdlibm atan2f / atanf, sincosf.h in its FMA and SSE2 builds) as IEEE
   arithmetic; a job whose keypoint selection ran on the device then needs no host round trip between orientation and
   descriptors.  Used only where it is PROVEN equal: on x86-64, with the build glibc's own selector picks for this CPU, after
   a self-test of ~2 million arguments of each function against the process's libm (once per process).
   akz_debug_device_libm: *available = 0 (the host's libm is used), 1 (device, FMA build), 2 (device, SSE2 build); *last_job =
   the same for the last finished job (0 also when that job's selection ran on the host).  akz_debug_set_device_libm(ctx, 0)
   switches it off, (ctx, -1) back to automatic.  akz_debug_libm_eval: d_out3[3 i .. 3 i + 2] = atan2f(d_a[i], d_b[i]),
   cosf(d_a[i]), sinf(d_a[i]) as the device forms them (fma != 0: the FMA build) -- NaN for |d_a[i]| >= 120. */
int akz_debug_device_libm(akz_ctx* ctx, int* available, int* last_job);
int akz_debug_set_device_libm(akz_ctx* ctx, int mode);
int akz_debug_libm_eval(akz_ctx* ctx, const float* d_a, const float* d_b, float* d_out3, uint64_t n, int fma);
/* The gate table (csrc/akz_gates.hpp): every size / host-thread threshold that chooses between two equivalent kernel families
   or paths -- name, value, what it counts, what lies on either side.  Results never depend on a gate.  *rows points at a
   static table of *n entries.  (big_px_sync / big_px_async are the compiled-in values; akz_ctx_calibrate_gates and
   akz_debug_set_schedule(ctx, 4, ...) change a context's own copies.) */
typedef struct akz_gate {
    const char* name;
    double value;
    const char* unit;
    const char* meaning;
} akz_gate;
int akz_debug_gates(const akz_gate** rows, uint64_t* n);
/* Re-derives the two JOB gates of this context from timings on the machine at hand instead of the compiled-in values (which
   were tuned on a 16-core host of one pool): lone synthetic frames of 0.9 / 1.4 / 2.1 / 4.1 / 8.3 Mpx are extracted through
   the synchronous call and through the begin / finish interface (two jobs in flight), each with the batch path forced on
   and off; a gate becomes the smallest size from which the batch path is the faster one at that size and at every larger
   one (the largest size + 1 if it never is).  ~0.2 s, allocates what such jobs allocate; the caller's stream must be idle.
   *sync_px / *async_px (may be NULL): the gates chosen; ms (may be NULL): 5 sizes x {sync lone, sync batch, streamed lone,
   streamed batch} = 20 medians in milliseconds.  Results of extractions never depend on the outcome. */
int akz_ctx_calibrate_gates(akz_ctx* ctx, uint64_t* sync_px, uint64_t* async_px, double* ms);
/* Measurement hook: the HIP-event spans of the diffusion and detector stages (akz_ctx_set_profiling) broken down by kernel
   variant and launch shape -- the rows behind bench.py's roofline.kernel, which names a group of kernels.  kind: see below;
   param: fused FED steps of a k_level_march launch (+16: the octave's 2x2 mean folded in, +32: Lstep written), FED steps
   covered by a group of k_fed_own launches, levels inside a k_octave_resident launch, sigma_size of a detector launch;
   (w, h, n): the launch's level size and batch (the largest level of a k_detector_tiled launch over several levels);
   launches, px = level pixels x batch, px_steps = pixel-steps advanced, ms = sum of the spans.  Rows accumulate like
   akz_profile; reset != 0 zeroes the figures.  *n_rows = rows there are (may exceed cap).  The rows of a context with lanes
   (akz_ctx_set_lanes) include its lanes', summed per kernel variant and shape, as its profile does.
   JPEG reconstruction (akz_extract_features_file / _files, akz_image_load_luma_device) adds rows of stage 10, which no
   akz_profile stage counts: k_jpeg_idct (px = coefficients), k_jpeg_luma (px = output pixels) and the coefficient upload
   (px = bytes copied), each with param = components and (w, h, 1) = the frame.
   The device sort of a job's extrema candidates adds one row of stage 11 per job, counted and never timed (ms stays 0; any
   profiling level): k_sort_rows (one launch), the four k_bucket_* launches, or the key / radix sort / gather chain around
   rocPRIM -- param 0, (w, h, n) = the frame and the batch, px = the list's capacity.
   The conversion of caller-held frames (akz_luma_from_frames_device, akz_extract_*_device_frames) adds one row of stage 10 per
   launch: k_frame_luma, param = the akz_frame_format, (w, h, n) = the frames, px = output pixels.
   A masked extraction (akz_extract_*_masked) adds one row of stage AKZ_ST_NMS (5) per filter launch, timed with every stage
   (profiling level 2): k_mask_candidates, param = masks (1: shared, else n), (w, h, n) = the frames, px = the list's capacity.
   One launch per job, one more for every extrema pass the overflow path redid; unmasked jobs leave no such row.
   akz_bank_create_from_results adds one row of stage 10 per bank with at least one row: k_bank_gather, ONE launch, param =
   desc_bytes, w = 64, h = the bank's rows, n = its segments (images), px = rows copied.
   akz_bank_create_from_results_budget / _from_sets_budget add, instead, one row of stage 10 per bank with at least one row:
   k_bank_select, ONE launch, param = desc_bytes, w = 64, h = the bank's rows, n = its sets, px = rows kept. */
enum { AKZ_KR_LEVEL_MARCH = 1, AKZ_KR_FED_OWN = 2, AKZ_KR_OCTAVE_RESIDENT = 3, AKZ_KR_DETECTOR_TILED = 4, AKZ_KR_DETECTOR_MARCH = 5,
       AKZ_KR_JPEG_IDCT = 6, AKZ_KR_JPEG_LUMA = 7, AKZ_KR_JPEG_COPY = 8, AKZ_KR_SORT_ROWS = 9, AKZ_KR_SORT_BUCKETS = 10,
       AKZ_KR_SORT_RADIX = 11, AKZ_KR_FRAME_LUMA = 12, AKZ_KR_MASK_CANDIDATES = 13, AKZ_KR_BANK_GATHER = 14,
       AKZ_KR_BANK_SELECT = 15 };
typedef struct akz_kernel_row {
    uint32_t stage, kind, param, w, h, n;
    uint64_t launches, px, px_steps;
    double ms;
} akz_kernel_row;
int akz_debug_kernel_rows(akz_ctx* ctx, akz_kernel_row* out, uint32_t cap, uint32_t* n_rows, int reset);
/* Test hook: pm_g2's reciprocal on its own -- d_out[i] = (1.0 / d_x[i]) as f32 the way every level kernel forms it
   (csrc/akz_pm_g2.hpp: refined hardware reciprocal, the full f64 division only where the f32 rounding could depend on it). */
int akz_debug_rcp_f64_to_f32(akz_ctx* ctx, const double* d_x, float* d_out, uint64_t n);
/* Test hook: where the extrema candidates are put into scan order: 1 = bucketed and sorted on the HOST (also the fallback
   that a candidate-list overflow and over-wide sort keys take), 0 = device sort, -1 = automatic (the default: device
   sort for contexts with fewer than four host threads).  Results are identical. */
int akz_debug_set_host_sort(akz_ctx* ctx, int on);
/* Test hook: where and how the order-dependent keypoint selection runs: 2 = on the device (dependency rounds over the
   neighbour lists, k_select; a job with an image whose lists overflowed falls back to 1), 1 = on the host from the device's
   neighbour lists (k_relations; needs the device sort, which it switches on), 0 = on the host from its spatial grids,
   -1 = automatic (the default: on the device for contexts with fewer than four host threads, for jobs that do not take the
   batch path, for jobs of fewer than four images, for the job that is waited for and for images of 6 Mpx and more; the grids otherwise).  Results are identical. */
int akz_debug_set_select(akz_ctx* ctx, int mode);
/* The selection of the last finished job: info[0] = where it ran (0 / 1 / 2 as above), info[1] = the most dependency rounds
   an image took on the device, info[2] = images that sent the job back to the host's selection, info[3] = candidates,
   info[4 .. 7] = 10 ns ticks of k_select's phases on image 0 (first states, turns, second pass, output).  info: 8 ints. */
int akz_debug_select_info(akz_ctx* ctx, int* info);

/* Test hooks for the scratch that one job leaves in a known state for the next (the claimed buffers).
   akz_debug_set_alloc_fill(ctx, on != 0): every device allocation the context (and its lanes) makes from now on -- scratch, slabs
   of results -- is filled with bytes 0xA5 before the allocating call returns (a fill and a wait: a debug mode), so that "fresh
   memory is not zero" is a fact and not luck.  Results are identical.
   akz_debug_audit_scratch: waits for the context's streams, then copies the range of every claim that is raised to the host and
   checks it against what the claim says: `small` (contrast scratch: zero), `bucket_scratch` (the bucket sort's counters: zero),
   `match_state` (the look-back words of the merging compaction: none carries an epoch beyond the context's).  Three rows per
   context, the lanes' behind the context's own ("lane0.small", ...): the claimed bytes (0: nothing claimed, nothing checked) and
   the offset of the first offending byte / word, -1 for none.  Read-only: it launches nothing and changes no claim.  *n_rows = rows
   there are (may exceed cap). */
typedef struct akz_scratch_audit {
    char name[32];
    uint64_t claimed_bytes;
    int64_t first_bad;
} akz_scratch_audit;
int akz_debug_set_alloc_fill(akz_ctx* ctx, int on);
int akz_debug_audit_scratch(akz_ctx* ctx, akz_scratch_audit* out, uint32_t cap, uint32_t* n_rows);
/* Test hook: what the library holds of the runtime right now, process-wide, over all contexts, jobs and results: out[0] = device
   blocks, out[1] = their bytes, out[2] = pinned host blocks, out[3] = their bytes, out[4] = events, out[5] = streams (the caller's
   stream of akz_ctx_create is not the library's and not counted; nor are the objects of akz_comm_*, akz_device_malloc and
   akz_stream_create).  A context that is created, used and destroyed, its results freed, leaves all six where they were.  No GPU
   call, no context. */
int akz_debug_resource_counts(uint64_t out[6]);
/* Test hook: the detection mask's kernel alone (k_mask_candidates, csrc/akz_mask.hip), enqueued on the context's stream and not
   synchronised.  d_records: a device list of the 32-byte records akz_host_select_keypoints documents, {u32 level, u32 flat_idx,
   f32 v, xp, xm, yp, ym, u32 img}, in a buffer of `capacity` records; d_counts: four u32 on the device, 8-byte aligned, [0] = the
   list's length on entry.  (w, h, cfg, n) give the level table, (d_mask, mask_layout, n_masks) the mask as akz_extract_device_frames_masked takes
   it (same refusals; a null mask is refused).  On completion d_kept (capacity records, not d_records) holds the kept records
   in any order, d_counts[0] the kept count and d_counts[1] the length on entry.  A length above the capacity leaves
   d_counts[0] as it is, sets d_counts[1] to it and copies the first `capacity` records through unfiltered: the extraction's
   overflow path then redoes the list with room.  d_counts[2], [3] are the kernel's own and zero afterwards.  A record whose
   level, image or index lies outside the tables is dropped. */
int akz_debug_mask_candidates(akz_ctx* ctx, const void* d_records, uint32_t capacity, uint32_t* d_counts, const uint8_t* d_mask,
                              const akz_frame_layout* mask_layout, uint32_t n_masks, uint32_t w, uint32_t h, const akz_config* cfg,
                              uint32_t n, void* d_kept);
/* The last finished masked job of the context (or of its lanes, whichever finished last): out[0] = candidates before the mask,
   out[1] = candidates kept, out[2] = extrema passes the overflow path redid (each followed by a filter launch of its own).
   The capacity bookkeeping of the context (the next job's list size) is fed out[0], not out[1]. */
int akz_debug_mask_counts(akz_ctx* ctx, uint64_t out[3]);
/* Test hook: the feature bank's kernel alone (k_bank_gather, csrc/akz_bank.hip) over caller-held device rows: n_rows rows of 64
   bytes at d_src (16-byte aligned) to d_dst, as a table of three segments -- the first half, an empty segment, the rest -- through
   the code path akz_bank_create_from_results takes; complete on return.  Bytes of a row at or beyond desc_bytes (1..64) arrive as
   zero whatever d_src holds there. */
int akz_debug_bank_gather(akz_ctx* ctx, const uint8_t* d_src, uint64_t n_rows, uint64_t desc_bytes, uint8_t* d_dst);
/* Test hook: the budgeted bank's kernel alone (k_bank_select, csrc/akz_bank.hip) on caller-made inputs, through the code path
   the budgeted constructors take; complete on return.  On the device: the source rows of n_sets sets packed one behind the
   other (sum of n rows of 64 bytes at d_src, 16-byte aligned) and their x and y (sum of n floats each).  On the host: every
   set's n and keep, and the keep indices of every set one behind the other -- per set ascending and below n, which the hook
   checks, refusing otherwise before anything is uploaded or launched.  On the device afterwards, for the sum of keep rows:
   d_rows (64 bytes each, the bytes at or beyond desc_bytes zero), d_x, d_y and d_index (the u32 source index of every row).
   The hook's table holds an empty record of its own in front of and behind the caller's sets. */
int akz_debug_bank_select(akz_ctx* ctx, const uint8_t* d_src, const float* d_sx, const float* d_sy, uint64_t n_sets, const uint64_t* n,
                          const uint64_t* keep, const uint32_t* indices, uint64_t desc_bytes, uint8_t* d_rows, float* d_x, float* d_y,
                          uint32_t* d_index);

/* The samples akz_match_features / akz_match_features_pairs draw for `trials` RANSAC trials over n_matches matches, from a
   source of their own seeded [s0, s1] (the calling thread's source is untouched): 8 ascending indices per trial. */
int akz_debug_ransac_samples(uint64_t s0, uint64_t s1, uint64_t n_matches, uint64_t trials, uint64_t* out);
/* The same draw loop with k = 8 or 4 indices per trial (the homography RANSAC draws 4); n_matches < k is refused. */
int akz_debug_ransac_samples_k(uint64_t s0, uint64_t s1, uint64_t n_matches, uint64_t trials, int k, uint64_t* out);
/* Where akz_match_features_pairs (or a homography call on a context) spends its time: enable != 0 times the context's later
   calls (events on its stream); ms (optional, 6 doubles) receives the last timed call's uploads, scans, host draws, trials, pick + filter and read-back
   in ms (the trials: first trial launch to last trial's end, overlapping the draws). */
int akz_debug_match_pairs_split(akz_ctx* ctx, int enable, double* ms);
/* The same for akz_keypoint_budget_sets: ms (optional, 3 doubles) receives the last timed call's upload, kernels and download. */
int akz_debug_keypoint_budget_split(akz_ctx* ctx, int enable, double* ms);
/* The same for akz_resection_seeded_problems: ms (optional, 4 doubles) receives the last timed call's upload (with the clearing
   memsets), rounds (first round's launch to the last update's end, the window look-ups of a call with confidence > 0 included),
   filter + refit and read-back. */
int akz_debug_resection_split(akz_ctx* ctx, int enable, double* ms);
/* Test hook: the queries per workgroup and the keypoints per LDS stage of k_budget_walk, so that tests can place their set sizes
   one below, at and one above them.  No GPU call, no context. */
int akz_debug_keypoint_budget_tiles(uint32_t* query_tile, uint32_t* train_tile);

/* ---- kernel-family selectors and the synthetic frame generator (tests, bench, tools): every mode gives bit-identical
   results; a drop-in host never calls these ---------------------------------------------------------------------- */
/* Deterministic synthetic 8-bit luma frame (integer-only, SplitMix64-seeded):
   gradient background + w*h/2048 random rectangles/discs + +-8 noise.  (shift_x, shift_y)
   translates the shapes, giving a second view of the same frame for match tests.  Host code. */
int akz_synth_frame_u8(uint8_t* out, uint32_t w, uint32_t h, uint64_t frame_index, int32_t shift_x,
                       int32_t shift_y);
/* FED kernel variant: 2 (default) = k_fed_own, LDS tile + register ownership, up to 8 explicit steps per launch (16
   for launches of a few workgroups); 0 = k_fed_step, one launch per step.  Results are bit-identical. */
int akz_ctx_set_fed_mode(akz_ctx* ctx, int mode);
/* Matcher kernel: 2 (default) and 3 = matrix cores on FP4 operands (k_match_fp4: descriptor bits as +-1 in e2m1,
   v_mfma_scale_f32_32x32x64_f8f6f4 with unit block scales, hamming = (488 - dot) / 2, exact in f32), 1 = matrix cores
   on int8 operands (k_match_mfma), 0 = popcount kernel (k_match).  Results are identical. */
int akz_ctx_set_match_mode(akz_ctx* ctx, int mode);
/* Detector kernel variant: 2 (default) = automatic (the one-pass column march k_detector_march for launches of
   8 Mpx and more, the one-kernel LDS-tiled form k_detector_tiled below that); 5 = column march wherever it is
   supported (sigma_size <= 4); 4 = the LDS-tiled kernel; 0 = the LDS-tiled kernel pair (the fallback for other
   kernel sizes).  Results are bit-identical. */
int akz_ctx_set_detector_mode(akz_ctx* ctx, int mode);
/* Level preparation (Lsmooth, Lflow of a level): 2 (default) = automatic — for launches of 8 Mpx and more the
   preparation and the level's first (up to four) diffusion steps run in ONE kernel (k_level_march), smaller launches take
   the streaming or the LDS-tiled preparation kernel; 3 = the fused kernel wherever it is supported; 1 = streaming
   preparation, 0 = LDS-tiled preparation (both without fusion).  Results are bit-identical. */
int akz_ctx_set_prep_mode(akz_ctx* ctx, int mode);

#ifdef __cplusplus
}
#endif
#endif /* AKAZE_HIP_DEBUG_H */
