// C ABI of libakaze_hip.so, part 3d: stream placement -- which of a context's streams run side by side, measured.
#include "akz_extract.hpp"

// The HIP runtime multiplexes a process's streams onto GPU_MAX_HW_QUEUES in-order hardware queues (4 by default), and the
// command processor of the chip has FOUR pipes: hardware queues k and k + 4 share one, and a pipe switches between its
// queues at ~25 us a switch (tools/queues/queue_probe.hip: 40 tiny kernels on each of two streams drain in 0.23 ms on
// different pipes, in 1.0 ms on one; a dependency across two queues of one pipe costs +55 us).  A batch pipeline that
// keeps four streams busy -- the caller's, the coarse chain's, the finish half's, the uploads' / early stages' -- therefore
// wants exactly four queues on four pipes: two of its streams on one QUEUE serialise everything behind everything
// (13.4 -> 7.7 Gpix/s, round 3), two on one PIPE cost 15 % (11.7 against 13.8 Gpix/s, round 4).  Which queue a stream got
// cannot be asked, so it is measured.
// Do streams a and b get in each other's way?  (1) a 120 us single-wave spin on each, from idle: on one hardware queue the
// second starts when the first has finished; (2) 24 tiny kernels on each, interleaved: on one pipe they drain several
// times slower than `alone_ms`, what 24 of them take on one stream.
// The verdict is a pure function of the probe's timings (akz::placement_verdict, unit-tested on the recorded timings of
// profiles/r04_queue_probe.txt).  Everything that disturbs a measurement -- the host thread preempted between two launches,
// a profiler that serialises dispatches, a neighbour's kernels -- can only make it LONGER, so a measurement that says
// "shared" is repeated (up to three in all) and the shortest one decides: a stream is only given up on evidence that
// repeats.
int akz::placement_verdict(float spin_pair_ms, float tiny_pair_ms, float tiny_alone_ms, float spin_ms) {
    int v = 0;
    // one hardware queue: the second spin starts when the first has finished (2 x; side by side 1.0-1.3 x)
    if (spin_pair_ms > 1.6f * spin_ms) v |= kPlaceQueue;
    // one pipe of the command processor: 24 + 24 interleaved tiny kernels drain ~8 x slower than 24 on one stream (different
    // pipes: 1.6-2.5 x); between 3 x and 6 x a single measurement is not trusted either way
    if (tiny_pair_ms >= 0.0f) {
        if (tiny_pair_ms > 4.0f * tiny_alone_ms) v |= kPlacePipe;
        if (tiny_pair_ms > 3.0f * tiny_alone_ms && tiny_pair_ms < 6.0f * tiny_alone_ms) v |= kPlaceAmbiguous;
    }
    if (spin_pair_ms > 1.35f * spin_ms && spin_pair_ms < 1.9f * spin_ms) v |= kPlaceAmbiguous;
    return v;
}
static int streams_interfere(akz_ctx* c, hipStream_t a, hipStream_t b, float alone_ms, bool* bad) {
    constexpr uint32_t kDelayUs = 120;
    constexpr float kSpinMs = (float)kDelayUs * 1e-3f;
    *bad = false;
    float spin_best = 1e30f, tiny_best = 1e30f;
    for (int attempt = 0; attempt < 3; ++attempt) {
        float ms = 0.0f;
        AKZ_HIP_TRY(hipEventRecord(c->probe_ev[0], a));
        launch::delay(a, kDelayUs);
        launch::delay(b, kDelayUs);
        AKZ_HIP_TRY(hipEventRecord(c->probe_ev[1], b));
        AKZ_HIP_TRY(hipGetLastError());
        AKZ_HIP_TRY(hipEventSynchronize(c->probe_ev[1]));
        AKZ_HIP_TRY(hipStreamSynchronize(a));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms, c->probe_ev[0], c->probe_ev[1]));
        spin_best = std::min(spin_best, ms);
        if (!(akz::placement_verdict(spin_best, -1.0f, alone_ms, kSpinMs) & (akz::kPlaceQueue | akz::kPlaceAmbiguous))) break;
        if (attempt < 2) ++c->place_retries;
    }
    if (akz::placement_verdict(spin_best, -1.0f, alone_ms, kSpinMs) & akz::kPlaceQueue) {
        *bad = true;
        return AKZ_OK;
    }
    for (int attempt = 0; attempt < 3; ++attempt) {
        float ms = 0.0f;
        AKZ_HIP_TRY(hipEventRecord(c->probe_ev[0], a));
        for (int k = 0; k < 24; ++k) {
            launch::delay(a, 1);
            launch::delay(b, 1);
        }
        AKZ_HIP_TRY(hipEventRecord(c->probe_ev[1], b));
        AKZ_HIP_TRY(hipGetLastError());
        AKZ_HIP_TRY(hipEventSynchronize(c->probe_ev[1]));
        AKZ_HIP_TRY(hipStreamSynchronize(a));
        AKZ_HIP_TRY(hipEventElapsedTime(&ms, c->probe_ev[0], c->probe_ev[1]));
        tiny_best = std::min(tiny_best, ms);
        if (!(akz::placement_verdict(0.0f, tiny_best, alone_ms, kSpinMs) & (akz::kPlacePipe | akz::kPlaceAmbiguous))) break;
        if (attempt < 2) ++c->place_retries;
    }
    *bad = (akz::placement_verdict(0.0f, tiny_best, alone_ms, kSpinMs) & akz::kPlacePipe) != 0;  // (different pipes: 1.8 x, one pipe: 8 x)
    return AKZ_OK;
}
// The first large batch of a context checks that its busy streams do not share a hardware queue or a pipe.  A stream of the
// library that does is replaced by a fresh one (up to eight tries: the runtime hands a new stream the least-used queue,
// and the rejected ones stay alive until the end so that they keep theirs occupied).  The early stages of a batch run
// on the copy stream (idle for resident frames; for host frames the blur has to follow the upload anyway) -- a fifth busy
// stream would have to share a pipe with one of the four.  About 0.4 ms per pair, once per context.
// the probe's working set: streams already accepted, rejected ones (kept alive until the end so that they keep their queues
// occupied), the time 24 tiny kernels take on one stream
struct StreamPlacer {
    akz_ctx* c;
    float alone_ms = 0.0f;
    std::vector<hipStream_t> accepted;
    std::vector<Stream> rejected;
    explicit StreamPlacer(akz_ctx* ctx) : c(ctx) {}
    int calibrate(hipStream_t on) {
        for (Event& e : c->probe_ev) AKZ_TRY(e.ensure(hipEventDefault));
        launch::delay(on, 1);  // (the first launch of a kernel loads its code object: not part of a measurement)
        AKZ_HIP_TRY(hipStreamSynchronize(on));
        alone_ms = 1e30f;
        for (int attempt = 0; attempt < 3; ++attempt) {  // (the shortest of three: see placement_verdict)
            float ms = 0.0f;
            AKZ_HIP_TRY(hipEventRecord(c->probe_ev[0], on));
            for (int k = 0; k < 24; ++k) launch::delay(on, 1);
            AKZ_HIP_TRY(hipEventRecord(c->probe_ev[1], on));
            AKZ_HIP_TRY(hipEventSynchronize(c->probe_ev[1]));
            AKZ_HIP_TRY(hipEventElapsedTime(&ms, c->probe_ev[0], c->probe_ev[1]));
            alone_ms = std::min(alone_ms, ms);
        }
        return AKZ_OK;
    }
    int collides(hipStream_t x, bool* hit) {
        *hit = false;
        for (hipStream_t a : accepted) {
            AKZ_TRY(streams_interfere(c, a, x, alone_ms, hit));
            if (*hit) return AKZ_OK;
        }
        return AKZ_OK;
    }
    // slot ends up a stream that interferes with none of `accepted` (and joins them), or keeps its value (free = false)
    int settle(Stream& slot, bool* free) {
        bool hit = false;
        AKZ_TRY(collides(slot, &hit));
        for (int attempt = 0; hit && attempt < 8; ++attempt) {
            rejected.emplace_back();
            Stream& fresh = rejected.back();
            AKZ_TRY(fresh.ensure());
            bool fresh_hit = false;
            AKZ_TRY(collides(fresh, &fresh_hit));
            if (!fresh_hit) {  // (the one that goes takes fresh's place among the rejects)
                std::swap(slot, fresh);
                hit = false;
                ++c->place_replaced;
            }
        }
        *free = !hit;
        accepted.push_back(slot);
        return AKZ_OK;
    }
};
int place_streams(akz_ctx* c) {
    if (c->is_lane) {
        c->placed = true;
        return AKZ_OK;
    }
    // a stream that is being captured into a graph cannot be synchronised or timed: the probe waits for a call outside
    // the capture (akz_ctx_warmup is the place to run it once, up front)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (c->stream && hipStreamIsCapturing(c->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone) return AKZ_OK;
    (void)hipGetLastError();
    c->placed = true;
    finisher_drain(c);  // (the finish half uses c->aux)
    AKZ_TRY(ensure_aux(c));
    AKZ_TRY(c->coarse.ensure());
    AKZ_TRY(c->copy.ensure());
    if (c->settings.sched[SCHED_NO_PROBE]) {  // (measurement: no probe -- streams as the runtime placed them)
        c->pre_mode = 2;
        return AKZ_OK;
    }
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    AKZ_HIP_TRY(hipStreamSynchronize(c->aux));
    AKZ_HIP_TRY(hipStreamSynchronize(c->coarse));
    AKZ_HIP_TRY(hipStreamSynchronize(c->copy));
    StreamPlacer sp(c);
    AKZ_TRY(sp.calibrate(c->stream));
    sp.accepted.push_back(c->stream);
    bool free_coarse = false, free_aux = false, free_copy = false;
    AKZ_TRY(sp.settle(c->coarse, &free_coarse));
    AKZ_TRY(sp.settle(c->aux, &free_aux));
    AKZ_TRY(sp.settle(c->copy, &free_copy));
    c->place_collisions = (free_coarse ? 0 : 1) + (free_aux ? 0 : 1) + (free_copy ? 0 : 1);
    c->pre_mode = free_copy ? 2 : 0;
    return AKZ_OK;
}
// Lanes: a lane enqueues both halves of its jobs on its one stream, and the point of lanes is that their launch chains run
// side by side -- the same check for the lanes' streams (among themselves: the caller's stream carries only the events
// that order a lane behind the caller's work).  Up to four lanes can have a pipe each.
int place_lanes(akz_ctx* c) {
    if (c->settings.sched[SCHED_NO_PROBE] || c->lanes.empty()) return AKZ_OK;
    for (akz_ctx* l : c->lanes) AKZ_HIP_TRY(hipStreamSynchronize(l->stream));
    StreamPlacer sp(c);
    AKZ_TRY(sp.calibrate(c->lanes[0]->stream));
    c->lane_collisions = 0;
    for (akz_ctx* l : c->lanes) {
        bool free = false;
        AKZ_TRY(sp.settle(l->stream, &free));  // (a replaced stream goes with the placer's rejects; the lane owns the new one)
        if (!free) ++c->lane_collisions;
    }
    return AKZ_OK;
}

// Streams of another component of the process that are busy beside a context's (the exchange stream of akz_comm: one RCCL
// collective per step): they get queues and pipes that the caller's stream, the coarse chain's and the finish half's do not
// use -- with four pipes that leaves the copy stream's, which carries the least.
int akz::place_streams_beside(akz_ctx* c, hipStream_t* slots, int n_slots, int* still_shared) {
    AKZ_TRY(bind(c));
    if (still_shared) *still_shared = 0;
    if (c->is_lane || c->settings.sched[SCHED_NO_PROBE] || n_slots <= 0) return AKZ_OK;
    if (!c->placed) AKZ_TRY(place_streams(c));
    AKZ_HIP_TRY(hipStreamSynchronize(c->stream));
    AKZ_HIP_TRY(hipStreamSynchronize(c->coarse));
    AKZ_HIP_TRY(hipStreamSynchronize(c->aux));
    for (int i = 0; i < n_slots; ++i) AKZ_HIP_TRY(hipStreamSynchronize(slots[i]));
    StreamPlacer sp(c);
    AKZ_TRY(sp.calibrate(c->stream));
    sp.accepted = {c->stream, c->coarse, c->aux};
    for (int i = 0; i < n_slots; ++i) {
        bool free = false;
        Stream slot = Stream::adopt(slots[i]);  // (the component's stream for the length of the probe: settle may replace it)
        const int rc = sp.settle(slot, &free);
        slots[i] = slot.detach();
        AKZ_TRY(rc);
        sp.accepted.pop_back();  // (the component's own streams may share among themselves)
        if (!free && still_shared) ++*still_shared;
    }
    return AKZ_OK;
}
