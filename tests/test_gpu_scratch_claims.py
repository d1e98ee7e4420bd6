"""Scratch that one job leaves in a known state for the next (the claimed buffers), under akz_debug_set_alloc_fill --
every fresh device allocation holds 0xA5 bytes, so "fresh memory is not zero" is a fact and not luck -- and with
akz_debug_audit_scratch after every job: a claim that does not hold on the device fails the test THERE, before another job runs on
that context (no kernel ever runs on scratch known to be unclean).

  (a) the bucket sort's counters: a first device-sorted job with too many buckets allocates them and takes rocPRIM; the job that
      fits the bucket sort afterwards must not trust them;
  (b) the contrast scratch through jobs whose histogram grows and shrinks, per level-preparation mode and across modes;
  (c) the look-back state of the merging compaction through growing and shrinking query sets;
  (e) a mixed sequence on a filled context equals the same sequence on a plain one, and the oracle.
(d: DESIGN.md 3.1 finds no fourth claimed buffer.)  Expected values come from the oracle or from the float64 contrast restatement of
tests/test_config_space.py; every comparison is bit for bit."""
import numpy as np
import pytest

from test_gpu_extract import assert_same_result

pytestmark = pytest.mark.gpu

KIND_SORT_ROWS, KIND_SORT_BUCKETS, KIND_SORT_RADIX = 9, 10, 11  # AKZ_KR_SORT_* (include/akaze_hip_debug.h)


def filled_context(amd):
    """A context of its own whose every allocation is filled, switched on before its first job."""
    import torch
    c = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    c.debug_set_alloc_fill(True)
    return c


def audit(c, what):
    """Every raised claim holds on the device, or the test ends here: the caller starts no further job on `c`."""
    rows = c.debug_audit_scratch()
    assert [r["name"] for r in rows] == ["small", "bucket_scratch", "match_state"], rows
    bad = [r for r in rows if r["first_bad"] is not None]
    assert not bad, (what, bad)
    return {r["name"]: r["claimed_bytes"] for r in rows}


def gate(amd, name):
    (g,) = [g for g in amd.gates() if g["name"] == name]
    return int(g["value"])


# ---- (a) bucket counters ------------------------------------------------------------------------------------------------------
# Frames 2000 high and narrower than 160 have one octave: four levels of 2000 rows.  24 x 2000 is accepted by the plan, but frames
# of 24 .. 56 x 2000 give no keypoint at all (nothing survives the border exclusion) and equality would hold vacuously; 64 is the
# narrowest width whose frames have keypoints (about 230 each), with the same level heights and so the same bucket counts.
BUCKET_W, BUCKET_H = 64, 2000


def texture(w, h, seed, block=6):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((h + block - 1) // block, (w + block - 1) // block), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((block, block), np.uint8))[:h, :w])


@pytest.fixture(scope="module")
def bucket_jobs(amd, ref):
    """Job A: the smallest batch of BUCKET_W x BUCKET_H frames whose (image, level, row) buckets exceed the sort_buckets gate; job
    B: its first two frames.  The oracle's results of A's frames, computed once."""
    buckets_max = gate(amd, "sort_buckets")
    plan = amd.plan_levels(BUCKET_W, BUCKET_H)  # (the plan accepts the shape)
    heights = []
    while ref.plan_level_size(BUCKET_W, BUCKET_H, len(heights)) is not None:
        heights.append(ref.plan_level_size(BUCKET_W, BUCKET_H, len(heights))[1])
    assert heights == [lv["h"] for lv in plan] == [BUCKET_H] * 4
    n_a = buckets_max // sum(heights) + 1
    assert n_a * sum(heights) > buckets_max >= 2 * (sum(heights) + len(heights)) and n_a == 9
    frames = np.stack([texture(BUCKET_W, BUCKET_H, 900 + i) for i in range(n_a)])
    rfs = [ref.extract(f) for f in frames]
    assert all(rf.num_keypoints > 100 for rf in rfs)
    yield frames, rfs
    for rf in rfs:
        rf.close()


@pytest.mark.parametrize("select", [None, 2, 1], ids=["host_selection", "device_selection", "neighbour_lists"])
def test_bucket_counters_after_a_job_that_took_rocprim(amd, bucket_jobs, select):
    """A, B, A, B with a candidate hint that reallocates the bucket scratch, B -- on the device sort.  A takes rocPRIM and leaves the
    counters it allocated alone (no claim); every B takes the bucket sort and equals the oracle.  With the selection on the device or
    from the neighbour lists the bucket starts are candidate_relations' row table in rel_scratch."""
    import torch
    frames, rfs = bucket_jobs
    d = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    counters = (gate(amd, "sort_buckets") + 1) * 4
    counters = (counters + 255) // 256 * 256
    c = filled_context(amd)
    try:
        c.debug_set_host_sort(False)
        c.debug_set_select(select)
        c.set_profiling(1)
        claimed = []
        for step, (job, hint) in enumerate((("A", None), ("B", None), ("A", None), ("B", 32768 * len(frames)), ("B", None))):
            if hint:
                c.set_candidate_hint(hint)  # B's list capacity: twice A's, past the head-room of the scratch A allocated
            n = len(frames) if job == "A" else 2
            c.kernel_rows(reset=True)
            res = c.extract_features(d[:n], keep_all_planes=False)
            sorts = {r["kind"]: r["launches"] for r in c.kernel_rows(reset=True) if r["kind"] in (KIND_SORT_ROWS, KIND_SORT_BUCKETS, KIND_SORT_RADIX)}
            assert sorts == ({KIND_SORT_RADIX: 3} if job == "A" else {KIND_SORT_BUCKETS: 4}), (step, job, sorts)
            claimed.append(audit(c, (select, step, job))["bucket_scratch"])
            for i in range(n):
                assert_same_result(res, rfs[i], planes=False, img=i)
            res.close()
            if select is not None:
                assert c.debug_select_info()[0] == select, (step, c.debug_select_info())
        assert claimed == [0, counters, counters, counters, counters], claimed  # (A neither cleans them nor loses B's claim)
    finally:
        c.close()


# ---- (b) contrast scratch -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contrast_jobs(amd, ref):
    """The job sequence of tests/test_gpu_config.py::test_contrast_scratch_through_a_sequence_of_jobs -- (6 frames, few bins)
    alternating with (1 frame, 4096 bins) at 320 x 240 -- with every job's expected contrast factors, computed once."""
    from test_config_space import PERCENTILE_EXTRAS, contrast_from_histogram, gradient_histogram, percentile_for, u8_unit
    w, h = 320, 240
    frames = np.stack([amd.synth_frame(w, h, 500 + i) for i in range(6)])
    pairs = []
    for f in frames:
        b = ref.gaussian_blur(ref.gaussian_blur(u8_unit(f), 1.6), 1.0)
        pairs.append((ref.scharr(b, True, False, 1), ref.scharr(b, False, True, 1)))
    hists = {}

    def hist(i, nbins):
        if (i, nbins) not in hists:
            hists[(i, nbins)] = gradient_histogram(*pairs[i], nbins)
        return hists[(i, nbins)]

    rng = np.random.default_rng(0)
    jobs = []
    for step, pct in enumerate(PERCENTILE_EXTRAS + [None] * 6):
        for n, nbins in ((6, (1, 2, 3, 7, 300, 640)[step % 6]), (1, 4096)):
            i0 = step % 6 if n == 1 else 0
            if pct is None:  # a percentile exactly at the cumulative count of some bin of the first image
                hm, hs, npts = hist(i0, nbins)
                p = percentile_for(npts, int(np.cumsum(hs)[rng.integers(0, nbins)]) + int(rng.integers(0, 2)))
            else:
                p = pct
            jobs.append((i0, n, nbins, p, [contrast_from_histogram(*hist(i0 + i, nbins), p) for i in range(n)]))
    assert len(jobs) == 30
    return frames, jobs


def small_bytes(n, nbins, fused):
    """the cleared part of the contrast scratch: maxima | bins (| tickets of the fused head), in whole 256 bytes"""
    return (n * (8 + (4 if fused else 0) + nbins * 4) + 255) // 256 * 256


@pytest.mark.parametrize("modes", [(0,), (3,), (1,), (0, 3, 1)], ids=["fused_head", "march", "stream", "switching"])
def test_contrast_scratch_claims(amd, contrast_jobs, modes):
    """Under prep mode 0 k_head + k_contrast_hist_final leave what they used zero and the next job skips the clearing launch where
    the claim covers it; the march / stream passes (3 / 1) clear for themselves and leave the scratch dirty, so the claim must be
    gone when mode 0 comes back ("another family used it last").  The buffer is reallocated when the 4096-bin job first outgrows
    the 6-frame job's."""
    import torch
    frames, jobs = contrast_jobs
    d6 = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    c = filled_context(amd)
    try:
        known = 0
        for j, (i0, n, nbins, p, want) in enumerate(jobs):
            mode = modes[j % len(modes)]
            c.set_prep_mode(mode)
            cfg = amd.Config(contrast_factor_num_bins=nbins, contrast_percentile=p)
            res = c.extract_features(d6[i0:i0 + n], cfg, keep_all_planes=False)
            claimed = audit(c, (modes, j, mode, n, nbins))["small"]
            got = [res.contrast(i) for i in range(n)]
            res.close()
            assert got == want, (modes, j, mode, n, nbins, p, got, want)
            # what the claim may say: nothing after a pass that does not clean up; after the fused head at least its own range and
            # never more than the largest range cleaned since the claim was last dropped
            if mode != 0:
                assert claimed == 0, (modes, j, claimed)
                known = 0
            else:
                known = max(known, small_bytes(n, nbins, True))
                assert small_bytes(n, nbins, True) <= claimed <= known, (modes, j, claimed, known)
                known = claimed
    finally:
        c.close()


# ---- (c) matcher state --------------------------------------------------------------------------------------------------------
def match_sets(n0, n1, seed, every=4):
    """The sets of tests/test_gpu_ops.py::test_descriptor_match -- random rows with near-duplicates planted so that the ratio test
    passes -- every `every`-th query row, each at a train row of its own: the matches are spread over all workgroups of the
    compaction."""
    rng = np.random.default_rng(seed)
    d0 = rng.integers(0, 256, (n0, 61), dtype=np.uint8)
    d1 = rng.integers(0, 256, (n1, 61), dtype=np.uint8)
    rows = np.arange(0, n0, every)
    at = rng.permutation(n1)[:len(rows)]
    assert len(at) == len(rows)
    d1[at] = d0[rows]
    d1[at, rows % 61] ^= 0x11
    return d0, d1


def test_match_state_through_growing_and_shrinking_query_sets(amd, ref):
    """2048 query rows (the first size that takes k_match_merge_compact) three times, so that the epochs advance over the same words;
    300 rows in between (the single-workgroup compaction: no state); 5000 rows, which the first allocation still holds (twice the
    need plus the 256 bytes and the eighth every allocation adds: 418 bytes, 52 words); 14 000 rows, past it -- the state is
    reallocated and must be cleared again, 0xA5A5A5A5 reads as an epoch that no call has reached --; 2048 again."""
    lo, hi = gate(amd, "merge_compact_min_rows"), gate(amd, "merge_compact_max_rows")
    assert lo == 2048 and 300 < lo and 14000 <= hi
    cases = {}
    for key, n0, n1, every in (("a", 2048, 1300, 4), ("b", 2048, 1300, 4), ("tiny", 300, 1300, 4), ("more", 5000, 1300, 4),
                               ("grown", 14000, 450, 32)):
        d0, d1 = match_sets(n0, n1, 40 + n0 + len(cases), every)
        cases[key] = (d0, d1, ref.descriptor_match(d0, d1, 10000, 0.86))
        assert len(cases[key][2]) == len(range(0, n0, every))  # the planted rows, in every workgroup's 256
    words = lambda n: ((n + 255) // 256 + 1) * 8  # launch::match_merge_compact_state_bytes
    c = filled_context(amd)
    try:
        state = []
        for call, key in enumerate(("a", "b", "a", "tiny", "more", "b", "grown", "a")):
            d0, d1, exp = cases[key]
            got = c.descriptor_match(d0, d1, 10000, 0.86)
            state.append(audit(c, (call, key))["match_state"])
            assert np.array_equal(got, exp), (call, key, len(got), len(exp))
        assert state[0] >= 2 * words(2048) and state[:6] == [state[0]] * 6 and words(5000) <= state[0], state
        assert state[0] < words(14000) and 2 * words(14000) <= state[6] == state[7], state  # (grown once, by the 14 000-row call)
    finally:
        c.close()


# ---- (e) filled allocations change no result ----------------------------------------------------------------------------------
def mixed_sequence(c, amd, ref, check):
    """A short walk over the entry points on context `c` -> every result as bytes, in order.  check(what): called after every job
    (the filled context audits there)."""
    import torch
    from test_seeded_ransac_host import options, planted
    out = []
    feats = {}
    scene = texture(320, 240, 77, 9)
    for w, h in ((163, 81), (320, 240)):
        for n in (1, 3):
            if w == 320:  # views of one scene, each moved on by (5, 3) pixels
                frames = np.stack([np.roll(scene, (3 * i, 5 * i), (0, 1)) for i in range(n)])
            else:
                frames = np.stack([texture(w, h, 700 + i, 9) for i in range(n)])
            rfs = [ref.extract(f) for f in frames]
            assert all(rf.num_keypoints > 20 for rf in rfs)
            d = torch.from_numpy(frames).cuda()
            torch.cuda.synchronize()
            for keep in (True, False):
                res = c.extract_features(d, keep_all_planes=keep)
                check(("extract", w, h, n, keep))
                for i in range(n):
                    assert_same_result(res, rfs[i], planes=True, img=i)  # (every plane fetched; a lean result recomputes them)
                    pyr = res.pyramid(i)
                    out.append(b"".join(a.tobytes() for lv in pyr for a in lv.values()))
                    kp, desc = res.keypoints(i), res.descriptors(i)
                    out += [kp.tobytes(), desc.tobytes(), np.float64(res.contrast(i)).tobytes()]
                    if keep:
                        k2, d2 = res.describe_keypoints(kp.copy(), img=i)
                        assert np.array_equal(d2, desc) and np.array_equal(k2["angle"], kp["angle"]), (w, h, n, i)
                        out += [k2.tobytes(), d2.tobytes()]
                    if (w, n) == (320, 3):
                        feats[i] = (kp, desc)
                check(("planes", w, h, n, keep))
                res.close()
            for rf in rfs:
                rf.close()
    fa, fb = feats[0], feats[1]
    assert len(fa[0]) > 500 and len(fb[0]) > 500
    exp = ref.descriptor_match(fa[1], fb[1], 10000, 0.86)
    assert len(exp) > 500
    for mode in (0, 1, 2, 3):
        c.set_match_mode(mode)
        got = c.descriptor_match(fa[1], fb[1], 10000, 0.86)
        check(("descriptor_match", mode))
        assert np.array_equal(got, exp), mode
        out.append(got.tobytes())
    c.set_match_mode(2)
    for k in (1, 2, 5):
        recs, counts = c.descriptor_match_knn(fa[1], fb[1], k, 120)
        check(("knn", k))
        erecs, ecounts = amd.descriptor_match_knn_host(fa[1], fb[1], k, 120)
        assert np.array_equal(counts, ecounts) and recs.tobytes() == erecs.tobytes(), k
        out += [recs.tobytes(), counts.tobytes()]
    got = c.descriptor_match_cross(fa[1], fb[1], 10000, 0.86)
    check("cross")
    assert np.array_equal(got, amd.descriptor_match_cross_host(fa[1], fb[1], 10000, 0.86)) and len(got) > 500
    out.append(got.tobytes())
    shift = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, 3.0], [0.0, 0.0, 1.0]], np.float32)
    got = amd.descriptor_match_guided(fa[0], fa[1], fb[0], fb[1], shift, 0, 3.0, 10000, 0.86, ctx=c)
    check("guided")
    assert np.array_equal(got, amd.descriptor_match_guided_host(fa[0], fa[1], fb[0], fb[1], shift, 0, 3.0, 10000, 0.86)) and len(got) > 500
    out.append(got.tobytes())
    pa, pb, _ = planted(amd, "H", 257, 757)
    opt = options(amd, "H", max_trials=1000, confidence=0.99, refine_iterations=2, stream_base=3, lowes_ratio=0.86)
    m, model, fits, trials = c.match_features_seeded_pairs([pa, pb], [(0, 1)], opt)[0]
    check("seeded pairs")
    em, emodel, efits, etrials = amd.remove_outliers_seeded(pa[0], pb[0], c.descriptor_match(pa[1], pb[1], 10000, 0.86), opt, stream=3)
    assert model is not None and np.array_equal(m, em) and (fits, trials) == (efits, etrials)
    assert np.asarray(model, np.float32).tobytes() == np.asarray(emodel, np.float32).tobytes()
    out += [m.tobytes(), np.asarray(model, np.float32).tobytes(), np.int64([fits, trials]).tobytes()]
    return out


def test_filled_allocations_change_no_result(amd, ref):
    """Extraction of 1 and 3 frames at 163 x 81 and 320 x 240, all planes kept and lean, every plane fetched; describe_keypoints;
    descriptor_match in each matcher mode; knn, cross-checked and guided matching; one seeded-RANSAC pairs call: on a context whose
    allocations are filled with 0xA5 every result is the plain context's, and the oracle's / the host statement's where there is one.
    A difference means that some kernel reads memory the job did not write."""
    import torch
    plain = amd.Context(0, torch.cuda.current_stream().cuda_stream)
    try:
        want = mixed_sequence(plain, amd, ref, lambda what: None)
    finally:
        plain.close()
    c = filled_context(amd)
    try:
        got = mixed_sequence(c, amd, ref, lambda what: audit(c, what))
    finally:
        c.close()
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, len(g), len(w))
