"""GPU tests of the exact f32 search on three bf16 planes (FlatIPIndex(f32_planes=True)): the split kernel against its torch oracle,
the plane-walking scoring frame (score matrix and fused filter step) on inputs whose scores are known exactly, on random normalised
embeddings against f64 with a derived bound, and the cases in which the index or a search declines the planes."""
import numpy as np
import pytest
import torch

from oracle.scoring_ref import topk_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _wrapped(names):
    """Context: ops.<name> wrapped so that every call appends (name, col0 or None) to the returned list."""
    import contextlib
    from rankpo_amd import ops

    @contextlib.contextmanager
    def cm():
        calls, real = [], {n: getattr(ops, n) for n in names}
        try:
            for n in names:
                setattr(ops, n, (lambda n_: lambda *a, **kw: (calls.append((n_, a[2] if len(a) > 2 and isinstance(a[2], int) else None)),
                                                              real[n_](*a, **kw))[1])(n))
            yield calls
        finally:
            for n in names:
                setattr(ops, n, real[n])
    return cm()


PLANE_OPS = ("split_bf16x3", "similarity_f32_planes", "search_step_planes")


# ------------------------------------------------------------------------------------------------------------------
# (a) the split kernel
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,d", [(1, 64), (1, 384), (257, 64), (257, 384)])
def test_split_kernel_equals_the_torch_oracle_bit_for_bit(rows, d):
    """rpo_split_bf16x3 == ops.split_bf16x3_ref on values of many magnitudes with +0 and -0 among them (flag clean), then with a
    2^-130 (h would be a bf16 subnormal) and with an inf (flag raised for each of the two, planes still as the oracle's).  Planes are
    compared as 16-bit patterns; a NaN plane (inf - inf) has no single pattern and is compared as `is NaN at the same place`."""
    from rankpo_amd import ops
    g = torch.Generator().manual_seed(rows * 1000 + d)
    x = torch.randn(rows, d, generator=g) * torch.pow(torch.tensor(2.0), torch.randint(-20, 21, (rows, d), generator=g).float())
    x[0, 3], x[rows - 1, d - 2] = 0.0, -0.0
    for bad, want in ((None, 0), (2.0 ** -130, 1), (float("inf"), 1)):
        xx = x.clone()
        if bad is not None:
            xx[rows // 2, d // 2 + 1] = bad
        ref, ref_flag = ops.split_bf16x3_ref(xx)
        planes, flag = ops.split_bf16x3(xx.to(DEV))
        assert planes.shape == (rows, 3 * d) and planes.dtype == torch.bfloat16
        assert int(flag.item()) == want == int(bool(ref_flag)), (bad, int(flag.item()), bool(ref_flag))
        got = planes.cpu()
        nan = torch.isnan(ref.float())
        assert torch.equal(torch.isnan(got.float()), nan)
        assert torch.equal(got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])
    with pytest.raises(ValueError):
        ops.split_bf16x3(torch.zeros(4, 96, device=DEV))


# ------------------------------------------------------------------------------------------------------------------
# (b) one-hot operands: every score is one exact product
# ------------------------------------------------------------------------------------------------------------------
def test_one_hot_operands_score_exactly_with_all_three_planes_live():
    """d = 128, 300 queries, random normal f32 corpus rows (h, m and l all non-zero).  The corpus has 100,000 rows, not 60,000: at 300
    queries (two tile rows) 60,000 rows hold only two chunks of the >= 192 tiles the frame takes, i.e. ONE fused step; 100,000 rows
    with chunk_rows = 49,152 give two.
    One-hot queries +-2^e e_j (m = l = 0 on the query side): every score is +-2^e corpus[c, j] bit for bit -- l + m + h of the corpus
    value summed in that order is exact -- and the winners are topk_ref's of the f64 matrix, k = 10 and 100.
    Symmetric: 50 one-hot rows 2^5 e_j planted in the corpus, full-precision queries: their scores are q[r, j] 2^5 bit for bit, in the
    frame's score matrix and where the fused step hands them to the winners.  (The other scores of that search are rounded sums; its
    winners as a whole are case (d)'s subject.)"""
    from rankpo_amd import ops
    from rankpo_amd.retrieval import FlatIPIndex
    d, nq, n = 128, 300, 100_000
    g = torch.Generator(device=DEV).manual_seed(5)
    corpus = torch.randn(n, d, generator=g, device=DEV)
    r = torch.arange(nq, device=DEV)
    j = (r * 7) % d
    val = torch.pow(torch.tensor(2.0, device=DEV), ((r % 17) - 8).float()) * (1 - 2 * (r % 2)).float()
    q = torch.zeros(nq, d, device=DEV)
    q[r, j] = val
    ix = FlatIPIndex(corpus, device=DEV, chunk_rows=49_152, f32_planes=True)
    assert ix.emb16 is None and ix.emb_planes is not None and ix.emb_planes.shape == (n, 3 * d)
    assert int((ix.emb_planes[:, d:2 * d] != 0).sum()) > 0.9 * n * d and int((ix.emb_planes[:, 2 * d:] != 0).sum()) > 0.9 * n * d
    f64 = (q.double() @ corpus.double().T).cpu().numpy()
    rv, ri = topk_ref(f64, 100)
    for k in (10, 100):
        with _wrapped(PLANE_OPS + ("search_step",)) as calls:
            fv, fi = ix.search(q, k)
        steps = [c for c in calls if c[0] == "search_step_planes"]
        assert len(steps) >= 2 and not [c for c in calls if c[0] == "search_step"] and ix.fused_overflows == 0, calls
        want = val[:, None] * corpus[:, j].T.gather(1, fi)                           # one f32 product each: exact
        assert torch.equal(fv, want)
        assert np.array_equal(fi.cpu().numpy(), ri[:, :k]) and np.array_equal(fv.cpu().numpy(), rv[:, :k])
    # symmetric
    rows = torch.linspace(100, n - 100, 50, device=DEV).long()                       # in every chunk
    cols = (torch.arange(50, device=DEV) * 5) % d
    c2 = corpus.clone()
    c2[rows] = 0
    c2[rows, cols] = 32.0
    q2 = torch.randn(nq, d, generator=g, device=DEV)
    ix2 = FlatIPIndex(c2, device=DEV, chunk_rows=49_152, f32_planes=True)
    assert ix2.emb_planes is not None
    qp, flag = ops.split_bf16x3(q2)
    assert int(flag.item()) == 0
    want = q2[:, cols] * 32.0                                                         # [nq, 50]
    for c0, c1 in ix2.chunk_schedule(nq, 100):
        s = ops.similarity_f32_planes(qp, ix2.emb_planes[c0:c1])
        m = (rows >= c0) & (rows < c1)
        assert bool(m.any()) and torch.equal(s[:, rows[m] - c0], want[:, m])
    fv, fi = ix2.search(q2, 100)
    hit = (fi[:, :, None] == rows[None, None, :])                                    # [nq, k, 50]
    later = hit & (rows >= ix2.chunk_schedule(nq, 100)[1][0])[None, None, :]
    assert int(later.sum()) > 100                                                    # the fused step delivered planted rows
    qi, ki, pi = hit.nonzero(as_tuple=True)
    assert torch.equal(fv[qi, ki], want[qi, pi])


# ------------------------------------------------------------------------------------------------------------------
# (c) an integer grid: every partial sum is exact in f32, whatever the order
# ------------------------------------------------------------------------------------------------------------------
def test_integer_grid_scores_are_exact_and_ties_take_the_smaller_index():
    """Corpus values n / 4096, |n| <= 4095 (odd |n| > 2048 among them: exact in neither bf16 nor fp16), queries j / 32, |j| <= 31,
    d = 128: every product and every partial sum is an integer below 2^24 over 2^17, exact in f32.  Duplicated corpus rows tie.
    Scores == the f64 dot, indices == topk_ref (ties to the smaller index), the result == the f32_planes=False search bit for bit,
    fused == unfused, and the fused step ran once per chunk after the first while `search_step` never ran."""
    from rankpo_amd.retrieval import FlatIPIndex, exact_in_16
    d, nq, n, k = 128, 300, 100_000, 100
    assert 31 * 4095 * d < 2 ** 24
    g = torch.Generator(device=DEV).manual_seed(11)
    ints = torch.randint(-4095, 4096, (n, d), generator=g, device=DEV)
    ints[50_000:50_100] = ints[100:200]
    ints[99_000:99_050] = ints[100:150]
    assert bool(((ints.abs() > 2048) & (ints % 2 != 0)).any())
    corpus = ints.float() / 4096
    q = torch.randint(-31, 32, (nq, d), generator=g, device=DEV).float() / 32
    assert exact_in_16(corpus, torch.bfloat16) is None and exact_in_16(corpus, torch.float16) is None
    ix = FlatIPIndex(corpus, device=DEV, chunk_rows=49_152, f32_planes=True)
    assert ix.emb16 is None and ix.emb_planes is not None
    with _wrapped(PLANE_OPS + ("search_step",)) as calls:
        fv, fi = ix.search(q, k)
    sched = ix.chunk_schedule(nq, k)
    assert len(sched) >= 3 and [c for c in calls if c[0] == "search_step_planes"] == [("search_step_planes", c0) for c0, _ in sched[1:]]
    assert not [c for c in calls if c[0] == "search_step"] and ix.fused_overflows == 0
    f64 = q.double() @ corpus.double().T
    assert torch.equal(fv.double(), f64.gather(1, fi))
    rv, ri = topk_ref(f64.cpu().numpy(), k)
    assert np.array_equal(fi.cpu().numpy(), ri) and np.array_equal(fv.cpu().numpy(), rv)
    assert bool((fv[:, :-1] == fv[:, 1:]).any())                                      # (ties among the winners)
    ix.fused = False
    with _wrapped(PLANE_OPS) as calls:
        pv, pi = ix.search(q, k)
    assert not [c for c in calls if c[0] == "search_step_planes"] and len([c for c in calls if c[0] == "similarity_f32_planes"]) == len(sched)
    assert torch.equal(pi, fi) and torch.equal(pv, fv)
    sv, si = FlatIPIndex(corpus, device=DEV, chunk_rows=49_152).search(q, k)
    assert torch.equal(si, fi) and torch.equal(sv, fv)


# ------------------------------------------------------------------------------------------------------------------
# (d) random normalised f32 embeddings against f64
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,ncorpus,d,k", [(300, 70_000, 64, 10), (1024, 40_000, 384, 100)])
def test_random_normalised_embeddings_against_f64(nq, ncorpus, d, k):
    """B = (6 d 2^-23 + 2^-22) |q| |c|: the worst case of an f32 sum of 6 d exact terms, sum_i |t_i| <= ~|q| |c| by Cauchy-Schwarz, at
    (n - 1) u with u = 2^-24, doubled for the matrix unit's unspecified internal rounding, plus the dropped pairs' 2 (2^-23 + 2^-32).
    Every winner's score is within B of its f64 score, every non-selected f64 score is <= the k-th winner + 2 B, and more than 99 % of
    the indices are those of the f32 kernel's search (the figure test_gpu_kernels.py uses between two summation orders)."""
    from rankpo_amd.retrieval import FlatIPIndex
    g = torch.Generator(device=DEV).manual_seed(nq + ncorpus)
    corpus = torch.nn.functional.normalize(torch.randn(ncorpus, d, generator=g, device=DEV), dim=-1)
    q = torch.nn.functional.normalize(torch.randn(nq, d, generator=g, device=DEV), dim=-1)
    ix = FlatIPIndex(corpus, device=DEV, chunk_rows=24_576 if nq > 512 else 49_152, f32_planes=True)
    assert ix.emb16 is None and ix.emb_planes is not None
    with _wrapped(PLANE_OPS) as calls:
        fv, fi = ix.search(q, k)
    assert [c for c in calls if c[0] == "search_step_planes"] and ix.fused_overflows == 0
    sv, si = FlatIPIndex(corpus, device=DEV, chunk_rows=ix.chunk_rows).search(q, k)
    f64 = q.double() @ corpus.double().T
    norms = q.double().norm(dim=1)[:, None] * corpus.double().norm(dim=1)[None, :]
    B = (6 * d * 2.0 ** -23 + 2.0 ** -22) * norms
    err_p = (fv.double() - f64.gather(1, fi)).abs()
    err_s = (sv.double() - f64.gather(1, si)).abs()
    print(f"\nmax |score - f64|: planes {float(err_p.max()):.3e}, f32 kernel {float(err_s.max()):.3e}, bound B {float(B.min()):.3e} "
          f"(nq {nq}, corpus {ncorpus}, d {d}, k {k})")
    assert bool((err_p <= B.gather(1, fi)).all())
    rest = f64.clone()
    rest.scatter_(1, fi, float("-inf"))
    assert bool((rest <= fv[:, -1:].double() + 2 * B).all())
    assert float((si == fi).float().mean()) > 0.99


# ------------------------------------------------------------------------------------------------------------------
# (e) declines
# ------------------------------------------------------------------------------------------------------------------
def test_the_planes_are_declined_where_they_do_not_apply():
    from rankpo_amd.retrieval import FlatIPIndex, create_faiss_index
    g = torch.Generator(device=DEV).manual_seed(23)
    corpus = torch.nn.functional.normalize(torch.randn(60_000, 64, generator=g, device=DEV), dim=-1)
    q = torch.nn.functional.normalize(torch.randn(300, 64, generator=g, device=DEV), dim=-1)
    with _wrapped(PLANE_OPS) as calls:                                               # the default index: no plane op at all
        a = FlatIPIndex(corpus, device=DEV, chunk_rows=30_000)
        assert a.emb_planes is None
        av, ai = a.search(q, 10)
        assert create_faiss_index(corpus, device=DEV).emb_planes is None
    assert calls == []
    assert create_faiss_index(corpus, device=DEV, f32_planes=True).emb_planes is not None
    c96 = torch.nn.functional.normalize(torch.randn(60_000, 96, generator=g, device=DEV), dim=-1)
    assert FlatIPIndex(c96, device=DEV, f32_planes=True).emb_planes is None          # d % 64
    tiny = corpus.clone()
    tiny[12_345, 6] = 2.0 ** -130
    assert FlatIPIndex(tiny, device=DEV, f32_planes=True).emb_planes is None         # a plane below the normal range
    b16 = FlatIPIndex(corpus.to(torch.bfloat16).float(), device=DEV, f32_planes=True)
    assert b16.emb16 is not None and b16.emb_planes is None                          # exact in bf16: the 16-bit copy wins
    # queries with an inf: that call goes to the f32 kernel, the same result as the default index
    p = FlatIPIndex(corpus, device=DEV, chunk_rows=30_000, f32_planes=True)
    qi = q.clone()
    qi[7, 3] = float("inf")
    with _wrapped(PLANE_OPS) as calls:
        pv, pi = p.search(qi, 10)
    assert [c[0] for c in calls] == ["split_bf16x3"]
    dv, di = a.search(qi, 10)
    assert torch.equal(pi, di) and torch.equal(torch.nan_to_num(pv, nan=-7.0), torch.nan_to_num(dv, nan=-7.0))
    with _wrapped(PLANE_OPS) as calls:                                               # and clean queries take the planes
        p.search(q, 10)
    assert "search_step_planes" in [c[0] for c in calls]


def test_candidate_overflow_redoes_the_search_through_the_plane_score_matrix():
    """The ascending corpus of test_fused_search_step_overflow_falls_back_to_the_score_matrix in f32 (every later chunk beats everything
    before it): the candidate lists run over, `fused_overflows` counts it, and the result is topk_ref's of the frame's score matrix and, independently of the
    frame, within the f64 bound of case (d)."""
    from rankpo_amd import ops
    from rankpo_amd.retrieval import FlatIPIndex
    g = torch.Generator(device=DEV).manual_seed(4)
    d, n, nq, k = 64, 75_000, 300, 50
    u = torch.nn.functional.normalize(torch.randn(d, generator=g, device=DEV), dim=0)
    scale = torch.linspace(0.1, 1.0, n, device=DEV)[:, None]
    corpus = scale * u[None, :] + 0.001 * torch.randn(n, d, generator=g, device=DEV)
    q = u[None, :] + 0.01 * torch.randn(nq, d, generator=g, device=DEV)
    ix = FlatIPIndex(corpus, device=DEV, chunk_rows=25_000, f32_planes=True)
    assert ix.emb_planes is not None
    sched = ix.chunk_schedule(nq, k)
    assert len(sched) == 3
    with _wrapped(PLANE_OPS) as calls:
        fv, fi = ix.search(q, k)
    assert ix.fused_overflows == 1 and len([c for c in calls if c[0] == "search_step_planes"]) == 2
    qp, _ = ops.split_bf16x3(q)
    full = torch.cat([ops.similarity_f32_planes(qp, ix.emb_planes[c0:c1]) for c0, c1 in sched], 1)
    rv, ri = topk_ref(full.cpu().numpy(), k)
    assert np.array_equal(fi.cpu().numpy(), ri) and np.array_equal(fv.cpu().numpy(), rv)
    # and on its own feet, against f64 (the bound of test_random_normalised_embeddings_against_f64)
    f64 = q.double() @ corpus.double().T
    B = (6 * d * 2.0 ** -23 + 2.0 ** -22) * q.double().norm(dim=1)[:, None] * corpus.double().norm(dim=1)[None, :]
    assert bool(((fv.double() - f64.gather(1, fi)).abs() <= B.gather(1, fi)).all())
    f64.scatter_(1, fi, float("-inf"))
    assert bool((f64 <= fv[:, -1:].double() + 2 * B).all())
