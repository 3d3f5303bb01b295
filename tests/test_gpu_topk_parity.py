"""GPU side of the selection-kernel parity suite (tests/topk_parity_util.py; the CPU side, tests/test_topk_parity_host.py, shows that
the case table reaches every branch of topk_merge_kernel and topk_merge_fast_kernel in f32, bf16 and fp16).  Selection is exact:
every assertion here is bit for bit, values compared as int32 views so that -0.0 / +0.0 and the infinities count.

(a) ops.topk_merge / ops.topk_finish over the whole table against `select_ref`, on padded and guarded inputs.
(b) rpo_topk_merge_candidates on hand-built lists against `merge_ref`: every sort size, the counter / overflow protocol.
(c) rpo_sim_topk_filter (the EPI 2 / EPI 3 epilogues of sim_tile256_kernel) on an integer grid against the score matrix of the same
    frame and the `before` rule, as sets.
(d) every path of FlatIPIndex.search on an integer-grid corpus: one answer, `select_ref` of the float64 score matrix.

What these tests found.  Everything the suite was asked to cover held as it stood.  One defect came out of writing the fast
kernel's model (its capacity assertion) and the row kind built to reach it, `nan_flood`: a first group of mostly NaN leaves a list
that is still short of k winners AND carries candidates; the next group then starts with the quarter bootstrap, whose 256 V appends
(2048 in 16-bit storage, the whole list) ran over the list on top of the carried ones, and the excess was dropped without a trace.
On the kernel as it was, bf16-nan-flood-k1024 and f16-nan-flood-k1024 returned winners that differed between two launches on the
same input (which appends are lost depends on the order of the atomics); f32 (1024 appends) held.  topk.hip now settles such a
list before the bootstrap quarter, between two barriers that fence the counter; the model's `settle_carry` branch.
"""
import functools

import numpy as np
import pytest
import torch

import topk_parity_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [c["name"] for c in U.CASES]
BY_NAME = {c["name"]: c for c in U.CASES}
IDX_FILL = -1


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """A device error ends the session: nothing more is started on a GPU that has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                     # noqa: BLE001 -- whatever the runtime raises
        pytest.exit(f"device error, stopping: {e}", returncode=3)


def ops():
    from rankpo_amd import ops as o
    return o


def lib():
    from rankpo_amd import _lib
    return _lib.load()


def check(rc, what):
    from rankpo_amd import _lib
    _lib.check(rc, what)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    return ops()._dt(torch.empty(0, dtype=dtype))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(vals, idx, want):
    """(f32 values, int64 indices) on the device against a numpy reference pair, bit for bit."""
    return np.array_equal(U.bits32(vals), U.bits32(want[0])) and np.array_equal(idx.cpu().numpy(), want[1])


def _guarded_rows(rows, width, dtype, fill, guard):
    """[guard + rows + guard, width] filled with `fill` -> (buffer, the contiguous payload view)."""
    buf = torch.full((guard + rows + guard, width), fill, dtype=dtype, device=DEV)
    return buf, buf[guard:guard + rows]


def _holds_fill(part):
    return bool(torch.isnan(part).all()) if part.dtype.is_floating_point else bool((part == IDX_FILL).all())


# ------------------------------------------------------------------------------------------------
# (a) the two selection kernels over the table
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_data(name):
    case = BY_NAME[name]
    m, rows = U.build_case(case)
    return m, U.select_ref(rows, case["k"], case["col0"])


@pytest.mark.parametrize("name", IDS)
def test_topk_merge_table(name):
    """Every chunk of a case through ops.topk_merge in its delivery order, then ops.topk_finish, against select_ref.  The score
    matrix carries +inf in its padding columns and guard rows (a read past a row's end would win).  The winners live in the middle
    of a buffer prefilled with NaN / -1: the first call is repeated through the C entry into that prefill (`first` must ignore what
    the lists hold) and must equal what ops.topk_merge allocated; afterwards the rows that were not addressed still hold the
    prefill."""
    case = BY_NAME[name]
    m, want = _case_data(name)
    md = m.to(DEV)
    k, split, rows, col0 = case["k"], case["split"], case["rows"], case["col0"]
    G = 4
    bufv, bv = _guarded_rows(rows * split, k, torch.float32, float("nan"), G)
    bufi, bi = _guarded_rows(rows * split, k, torch.int64, IDX_FILL, G)
    for n, (c0, c1) in enumerate(case["chunks"]):
        view = U.chunk_view(md, case, c0, c1)
        kern = U.selection_kernel(U.chunk_view(m, case, c0, c1), split)
        assert U.selection_kernel(view, split) == kern                                                          # the host test's choice
        assert md.data_ptr() % 16 == 0                                                                           # ... and its premise
        if n == 0:
            fv, fi = ops().topk_merge(view, col0 + c0, None, None, k, split=split)
            check(lib().rpo_topk_merge_split(view.data_ptr(), view.stride(0), rows, c1 - c0, col0 + c0, k, _dt(case["dtype"]), split,
                                             bv.data_ptr(), bi.data_ptr(), 1, _stream()), "rpo_topk_merge_split")
            assert torch.equal(_bits(fv), _bits(bv)) and torch.equal(fi, bi), (name, "first call: allocated against prefilled lists")
        else:
            rv, ri = ops().topk_merge(view, col0 + c0, bv, bi, k, split=split)
            assert rv.data_ptr() == bv.data_ptr() and ri.data_ptr() == bi.data_ptr()
    ov, oi = ops().topk_finish(bv, bi, split)
    got_v, got_i = U.bits32(ov), oi.cpu().numpy()
    bad = np.nonzero((got_v != U.bits32(want[0])) | (got_i != want[1]))
    assert len(bad[0]) == 0, (name, "row %d (%s) place %d: got (%r, %d), want (%r, %d)" % (
        bad[0][0], case["kinds"][bad[0][0]], bad[1][0], float(ov[bad[0][0], bad[1][0]]), got_i[bad[0][0], bad[1][0]],
        float(want[0][bad[0][0], bad[1][0]]), want[1][bad[0][0], bad[1][0]]))
    for buf in (bufv, bufi):
        assert _holds_fill(buf[:G]) and _holds_fill(buf[G + rows * split:]), (name, "winner rows that were not addressed were written")
    assert torch.equal(md.cpu().view(torch.int16 if m.element_size() == 2 else torch.int32),
                       m.view(torch.int16 if m.element_size() == 2 else torch.int32)), (name, "the scores were written")


# ------------------------------------------------------------------------------------------------
# (b) rpo_topk_merge_candidates on hand-built lists
# ------------------------------------------------------------------------------------------------
def _winner_list(rs, k, real, lo, hi):
    """A valid winner list: `real` (value, index) pairs with integer values in [lo, hi) (many ties) and distinct EVEN indices,
    sorted, padded to k."""
    v = rs.randint(lo, hi, size=real).astype(np.float32)
    i = (rs.choice(1 << 20, size=real, replace=False).astype(np.int64) * 2) + (1 << 40)
    return U.merge_ref((v[None], i[None]), k=k)


def _run_candidates(k, cap, counts, seed, short=()):
    """One launch over len(counts) rows.  Row r holds counts[r] candidates (cap of them are stored when counts[r] > cap): integer
    values that tie the winners' values, ODD indices interleaved with the winners' even ones (smaller and larger than a tied
    winner's).  Rows in `short` start from a list with k / 2 real winners.  Rows with count 0 hold junk winners (NaN, -5): the kernel
    must leave them alone."""
    rs = np.random.RandomState(seed)
    rows = len(counts)
    G = 3
    bufv, bv = _guarded_rows(rows, k, torch.float32, float("nan"), G)
    bufi, bi = _guarded_rows(rows, k, torch.int64, IDX_FILL, G)
    cbufv, cv = _guarded_rows(rows, cap, torch.float32, float("nan"), G)
    cbufi, ci = _guarded_rows(rows, cap, torch.int64, IDX_FILL, G)
    cntbuf = torch.full((G + rows + G,), IDX_FILL, dtype=torch.int32, device=DEV)
    cnt = cntbuf[G:G + rows]
    flagbuf = torch.full((2 * G + 1,), IDX_FILL, dtype=torch.int32, device=DEV)
    flagbuf[G] = 0
    want_v = np.full((rows, k), np.nan, dtype=np.float32)
    want_i = np.full((rows, k), -5, dtype=np.int64)
    hv, hi_ = np.full((rows, k), np.nan, dtype=np.float32), np.full((rows, k), -5, dtype=np.int64)
    hcv, hci = np.full((rows, cap), np.nan, dtype=np.float32), np.full((rows, cap), IDX_FILL, dtype=np.int64)
    for r, count in enumerate(counts):
        if count == 0:
            continue
        wv, wi = _winner_list(rs, k, k // 2 if r in short else k, 0, 8)
        stored = min(count, cap)
        cvals = rs.randint(0, 10, size=stored).astype(np.float32)
        cidx = (rs.choice(1 << 20, size=stored, replace=False).astype(np.int64) * 2 + 1) + (1 << 40)
        if stored >= 3:                                         # the same value as the k-th winner, just below and just above its index
            cvals[0], cidx[0] = wv[0, k - 1], (wi[0, k - 1] - 1 if wi[0, k - 1] != U.INT64_MAX else cidx[0])
            cvals[1], cidx[1] = wv[0, k - 1], (wi[0, k - 1] + 1 if wi[0, k - 1] != U.INT64_MAX else cidx[1])
            cvals[2], cidx[2] = wv[0, 0], wi[0, 0] - 1          # and ahead of the best
        hv[r], hi_[r] = wv[0], wi[0]
        hcv[r, :stored], hci[r, :stored] = cvals, cidx
        want_v[r], want_i[r] = (a[0] for a in U.merge_ref((wv, wi), (cvals[None], cidx[None]), k=k))
    bv.copy_(torch.from_numpy(hv))
    bi.copy_(torch.from_numpy(hi_))
    cv.copy_(torch.from_numpy(hcv))
    ci.copy_(torch.from_numpy(hci))
    cnt.copy_(torch.tensor(counts, dtype=torch.int32))
    check(lib().rpo_topk_merge_candidates(cv.data_ptr(), ci.data_ptr(), cnt.data_ptr(), rows, cap, k, bv.data_ptr(), bi.data_ptr(),
                                          flagbuf[G:].data_ptr(), _stream()), "rpo_topk_merge_candidates")
    assert np.array_equal(U.bits32(bv), U.bits32(want_v)), ("values", k, cap, counts)
    assert np.array_equal(bi.cpu().numpy(), want_i), ("indices", k, cap, counts)
    assert int(cnt.abs().sum()) == 0, "every counter is reset"
    assert int(flagbuf[G]) == int(any(c > cap for c in counts)), "the overflow flag"
    for buf, n in ((bufv, rows), (bufi, rows), (cbufv, rows), (cbufi, rows)):
        assert _holds_fill(buf[:G]) and _holds_fill(buf[G + n:])
    assert _holds_fill(cntbuf[:G]) and _holds_fill(cntbuf[G + rows:]) and _holds_fill(flagbuf[:G]) and _holds_fill(flagbuf[G + 1:])
    assert np.array_equal(U.bits32(cv), U.bits32(hcv)) and np.array_equal(ci.cpu().numpy(), hci), "the lists are inputs"


def test_merge_candidates_every_sort_size():
    """k = 40, cap = 4056 = kTopkSlots - k: k + count = 64, 65, 128, 129, ..., 4096 in ONE launch, between rows of count 0 (the
    block-uniform early return: winners untouched, counter still 0) and 1; the last row's count equals cap.  No overflow: the flag
    stays 0."""
    k, cap = 40, U.TOPK_SLOTS - 40
    totals = [64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096]
    counts = [0, 1] + [t - k for t in totals[:7]] + [0] + [t - k for t in totals[7:]] + [0, 2]
    assert counts[-3] == cap
    _run_candidates(k, cap, counts, seed=1, short=(1, 4))


def test_merge_candidates_overflow_merges_the_first_cap_entries():
    """count > cap: the flag is raised, the result is the merge of the cap stored entries, the counter is reset; rows below cap in
    the same launch are merged in full."""
    _run_candidates(100, 1024, [0, 1024, 1025, 5000, 1, 300, 2 ** 30], seed=2, short=(4,))
    _run_candidates(1, 64, [63, 64, 65, 0, 1], seed=3)                       # k = 1: 64 and 65 slots; count > cap with a 128-slot sort


def test_merge_candidates_k1024_cap3072():
    """The search's own largest frame: k = 1024 with search_candidate_cap(1024) = 3072 slots."""
    assert ops().search_candidate_cap(1024) == 3072
    _run_candidates(1024, 3072, [0, 1, 1024, 1025, 3071, 3072, 0, 7], seed=4, short=(1, 3))
    _run_candidates(1024, 3072, [3073, 0, 3072, 1], seed=5)


# ------------------------------------------------------------------------------------------------
# (c) the filter epilogues of the 256 x 256 frame
# ------------------------------------------------------------------------------------------------
FILTER_SHAPES = [(256, 49_152), (257, 24_576 + 77)]
FILTER_MODES = [("bf16-rounded", torch.bfloat16, 1), ("bf16-f32", torch.bfloat16, 0), ("f16-f32", torch.float16, 0)]


def _grid(rows, d, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-1, 2, (rows, d), generator=g).to(dtype).to(DEV)


@pytest.mark.parametrize("mode", FILTER_MODES, ids=[m[0] for m in FILTER_MODES])
@pytest.mark.parametrize("Q,P", FILTER_SHAPES)
def test_filter_candidates_are_the_before_set(Q, P, mode):
    """rpo_sim_topk_filter alone, d = 64, operands in {-1, 0, 1}: the scores are exact integers with hundreds of ties per row.  Per
    row the (value, index) candidates must be, as a set, the elements of the frame's own score matrix (ops.similarity for rounded
    bf16 scores, ops.similarity_f32 otherwise) that come `before` the row's threshold (best_val[:, k - 1], best_idx[:, k - 1]):
      rows 0 mod 3: +inf -- nothing passes, the counter stays 0;
      rows 1 mod 3: the row's exact 99.9 % quantile, with an index bound beyond the chunk (all ties pass) or at its start (none);
      rows 2 mod 3: the row's top-1 % value, tied at an occurrence in the middle of the chunk: only smaller global indices pass;
    for col0 in {0, 12 345, 2^40}.  Then once more with cap below most rows' counts: the counter still reports the true count and
    exactly cap entries are written, all of them members of the set.  The workspace sits between guard rows (a 256-row tile past
    Q = 257 would land there).  Finite operands only: NaN scores are outside the fused step's contract (FlatIPIndex never feeds
    it a list without k real winners, and `before` admits no NaN)."""
    tag, dtype, rounded = mode
    d, k, G = 64, 5, 256
    q, p = _grid(Q, d, 11 + Q, dtype), _grid(P, d, 13 + P, dtype)
    assert ops().search_filter_takes(q, p)
    S = ops().similarity(q, p).float() if rounded else ops().similarity_f32(q, p)
    assert S.dtype == torch.float32 and S.shape == (Q, P)
    assert torch.equal(S.double(), q.double() @ p.double().T)                      # the grid keeps every frame exact
    r = torch.arange(Q, device=DEV)
    cols = torch.arange(P, device=DEV)
    srt = torch.sort(S, dim=1, descending=True).values
    q999, q99 = srt[:, max(1, P // 1000) - 1], srt[:, P // 100 - 1]
    tv = torch.where(r % 3 == 0, torch.full_like(q999, float("inf")), torch.where(r % 3 == 1, q999, q99))
    dist = torch.where(S == q99[:, None], (cols - P // 2).abs()[None, :], torch.full((1, 1), P, device=DEV))
    mid = dist.argmin(dim=1)                                                        # the tie nearest the middle of the chunk
    assert bool((S[r, mid] == q99).all()) and bool(((mid - P // 2).abs() < P // 4).all())
    for col0 in (0, 12_345, 2 ** 40):
        ti = torch.where(r % 3 == 2, col0 + mid, torch.where(r % 6 == 1, torch.full_like(mid, col0 + P), torch.full_like(mid, col0)))
        want = (S > tv[:, None]) | ((S == tv[:, None]) & ((col0 + cols)[None, :] < ti[:, None]))
        wcount = want.sum(1)
        assert int(wcount[0::3].sum()) == 0 and int(wcount[1::3].min()) > 0 and int(wcount[2::3].min()) > P // 200
        best_val = torch.full((Q, k), float("nan"), device=DEV)                     # only column k - 1 is the kernel's to read
        best_idx = torch.full((Q, k), IDX_FILL, dtype=torch.int64, device=DEV)
        best_val[:, k - 1], best_idx[:, k - 1] = tv, ti
        for cap in (int(wcount.max()) + 3, 16):
            cbufv, cv = _guarded_rows(Q, cap, torch.float32, float("nan"), G)
            cbufi, ci = _guarded_rows(Q, cap, torch.int64, IDX_FILL, G)
            cntbuf = torch.full((G + Q + G,), IDX_FILL, dtype=torch.int32, device=DEV)
            cnt = cntbuf[G:G + Q]
            cnt.zero_()
            check(lib().rpo_sim_topk_filter(q.data_ptr(), p.data_ptr(), Q, P, d, _dt(dtype), col0, k, rounded, best_val.data_ptr(),
                                            best_idx.data_ptr(), cv.data_ptr(), ci.data_ptr(), cnt.data_ptr(), cap, _stream()),
                  "rpo_sim_topk_filter")
            what = (tag, Q, P, col0, cap)
            assert torch.equal(cnt.long(), wcount), (what, "the counters are not the set sizes")
            stored = cnt.long().clamp(max=cap)
            valid = torch.arange(cap, device=DEV)[None, :] < stored[:, None]
            assert _holds_fill(cv[~valid]) and _holds_fill(ci[~valid]), (what, "written beyond a list's count")
            rr = r[:, None].expand(Q, cap)[valid]
            local = ci[valid] - col0
            assert bool(((local >= 0) & (local < P)).all()), (what, "an index outside the chunk")
            assert torch.equal(_bits(cv[valid]), _bits(S[rr, local])), (what, "a candidate's value is not its score")
            seen = torch.zeros((Q, P), dtype=torch.int32, device=DEV)
            seen.index_put_((rr, local), torch.ones_like(local, dtype=torch.int32), accumulate=True)
            assert int(seen.max()) <= 1, (what, "a candidate twice")
            assert not bool((seen.bool() & ~want).any()), (what, "a candidate outside the set")
            assert torch.equal(seen.sum(1), stored), what
            if cap > 16:
                assert torch.equal(seen.bool(), want), (what, "the lists are not the set")
            else:
                assert int((wcount > cap).sum()) > Q // 3
            for buf in (cbufv, cbufi):
                assert _holds_fill(buf[:G]) and _holds_fill(buf[G + Q:]), (what, "written outside [0, Q) x cap")
            assert _holds_fill(cntbuf[:G]) and _holds_fill(cntbuf[G + Q:]), (what, "a counter outside [0, Q)")
        assert bool(torch.isnan(best_val[:, :k - 1]).all()) and torch.equal(best_val[:, k - 1], tv) and torch.equal(best_idx[:, k - 1], ti)


# ------------------------------------------------------------------------------------------------
# (d) one answer from every search path
# ------------------------------------------------------------------------------------------------
NCORPUS, NQ, SEARCH_D = 60_011, 257, 64
INDEX_KINDS = ["f32", "f32+bf16", "f32+f16", "bf16"]


@functools.lru_cache(maxsize=None)
def _search_problem(grid):
    """(queries, corpus, select_ref of the float64 score matrix at k = 1024).  'bf16': entries in {-1, 0, 1}.  'f16': a fifth of
    the corpus' ones are 1 + 2^-9, exact in fp16 and not in bf16; the queries stay on the integer grid, so every score is a multiple
    of 2^-9 below 2^7: exact in f32 in any summation order."""
    g = torch.Generator().manual_seed(60_011)
    q = torch.randint(-1, 2, (NQ, SEARCH_D), generator=g).float()
    c = torch.randint(-1, 2, (NCORPUS, SEARCH_D), generator=g).float()
    if grid == "f16":
        c = torch.where((c == 1) & (torch.rand(c.shape, generator=g) < 0.2), torch.full_like(c, 1 + 2.0 ** -9), c)
        assert torch.equal(c.half().float(), c) and not torch.equal(c.bfloat16().float(), c)
    else:
        assert torch.equal(c.bfloat16().float(), c)
    S = q.double() @ c.double().T
    assert torch.equal(S.float().double(), S)
    return q, c, U.select_ref(S.numpy(), 1024)


@functools.lru_cache(maxsize=None)
def _index(kind):
    from rankpo_amd.retrieval import FlatIPIndex
    q, c, ref = _search_problem("f16" if kind == "f32+f16" else "bf16")
    if kind == "bf16":
        ix = FlatIPIndex(c, device=DEV, dtype=torch.bfloat16)
    else:
        ix = FlatIPIndex(c, device=DEV, dtype=torch.float32, exact16=kind != "f32")
    want16 = {"f32": None, "bf16": None, "f32+bf16": torch.bfloat16, "f32+f16": torch.float16}[kind]
    assert (ix.emb16 is None) == (want16 is None) and (want16 is None or ix.emb16.dtype == want16)
    return ix, q.to(DEV), ref


@pytest.mark.parametrize("k", [1, 100, 1024])
@pytest.mark.parametrize("kind", INDEX_KINDS)
def test_every_search_path_gives_the_one_answer(kind, k):
    """An integer-grid corpus of 60 011 x 64 and 257 queries: every score is exact in every kernel, so an f32 index on the f32
    kernel, on its bf16 copy, on its fp16 copy (a corpus exact in fp16 only) and a bf16 index, each with the fused step on and off,
    one and four winner lists per row, and chunks of 30 000 rows (three chunks, the last of 11 rows) or one chunk schedule for
    the whole corpus, must all return select_ref of the float64 score matrix, values and indices, with thousands of ties per row."""
    o = ops()
    ix, q, ref = _index(kind)
    want = (ref[0][:, :k], ref[1][:, :k])
    real, steps = o.search_step, []
    o.search_step = lambda *a, **kw: (steps.append(a[2]), real(*a, **kw))[1]
    try:
        for chunk_rows in (30_000, 262_144):
            for split in (1, 4):
                for fused in (True, False):
                    ix.chunk_rows, ix.split, ix.fused = chunk_rows, split, fused
                    del steps[:]
                    v, i = ix.search(q, k)
                    assert v.dtype == torch.float32 and _same(v, i, want), (kind, k, chunk_rows, split, fused)
                    assert bool(steps) == (fused and split == 1 and kind != "f32"), (kind, k, chunk_rows, split, fused, steps)
    finally:
        o.search_step = real
        ix.chunk_rows, ix.split, ix.fused = 262_144, None, True
    assert ix.fused_overflows == 0
