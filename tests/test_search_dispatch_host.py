"""Which ops `FlatIPIndex.search` calls, on which corpus chunks and in which order -- no GPU: the index is built on CPU tensors and
the search functions of `rankpo_amd.ops` are replaced ON THE MODULE by recording fakes that compute with torch (search() looks
them up by attribute at call time, which is also how tests/test_gpu_topk_parity.py and tests/test_gpu_search_planes.py count calls).

The constructor runs on the CPU, but its `exact_in_16` / `exact_in_planes` answer None for tensors that are not on a GPU, so the
tests set `emb16` / `emb_planes` on the built object themselves; `retrieval.exact_in_16`, which search() asks about the queries,
is replaced by its torch statement without the memory rule.

Every case asserts the exact sequence of (op name, first row, end row, round_scores) -- round_scores is None for the ops that do
not take it -- and that the winners are those of the full score matrix."""
import pytest
import torch

from rankpo_amd import ops, retrieval

NQ, NTOTAL, D, K = 1024, 70_000, 64, 10
CHUNK_ROWS = 24_576
# 1024 query rows: the first fused chunk is 48 x 256 rows (192 tiles), the later ones grow up to chunk_rows, the tail joins the last
FUSED = [(0, 12_288), (12_288, 36_864), (36_864, 70_000)]
PLAIN = [(0, 24_576), (24_576, 49_152), (49_152, 70_000)]


@pytest.fixture(scope="module")
def data():
    g = torch.Generator().manual_seed(20_261)
    emb = torch.randn(NTOTAL, D, generator=g)
    q = torch.randn(NQ, D, generator=g)
    out = {"f32": (emb, q)}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        out[name] = (emb.to(dt).float(), q.to(dt).float())                     # every value exact in dt
    return out


def _rows(p, width):
    assert p.stride(0) == width and p.storage_offset() % width == 0
    c0 = p.storage_offset() // width
    return c0, c0 + p.shape[0]


def _unplane(x):
    d = x.shape[1] // 3
    return x[:, :d].float() + x[:, d:2 * d].float() + x[:, 2 * d:].float()


class Fakes:
    """Recording stand-ins for the search functions of rankpo_amd.ops."""

    def __init__(self, monkeypatch, refuse=(), overflow_at=None):
        self.log, self.preds = [], []
        self.refuse, self.overflow_at, self.steps = set(refuse), overflow_at, 0
        for name in ("similarity", "similarity_f32", "similarity_f32_planes", "topk_merge", "search_step", "search_step_planes",
                     "split_bf16x3", "search_filter_takes", "search_planes_takes", "search_filter_ok"):
            monkeypatch.setattr(ops, name, getattr(self, name))
        monkeypatch.setattr(retrieval, "exact_in_16", self.exact_in_16)

    @staticmethod
    def exact_in_16(x, dtype=torch.bfloat16):
        if x.dtype != torch.float32 or x.numel() == 0:
            return None
        h = x.to(dtype)
        return h if bool((h.float() == x).all()) else None

    def search_filter_ok(self, nq, rows, d):
        return True

    def search_filter_takes(self, q, p):
        c0, c1 = _rows(p, p.shape[1])
        self.preds.append(("search_filter_takes", c0, c1))
        return q.dtype in (torch.bfloat16, torch.float16) and p.dtype == q.dtype and c0 not in self.refuse

    def search_planes_takes(self, qp, cp):
        c0, c1 = _rows(cp, cp.shape[1])
        self.preds.append(("search_planes_takes", c0, c1))
        return c0 not in self.refuse

    def split_bf16x3(self, x):
        self.log.append(("split_bf16x3", None, None, None))
        planes, inexact = ops.split_bf16x3_ref(x)
        return planes, inexact.to(torch.int32).view(1)

    def _scores(self, name, q, p, rnd=None):
        self.log.append((name,) + _rows(p, p.shape[1]) + (rnd,))
        if name.endswith("planes"):
            return _unplane(q) @ _unplane(p).T
        return q.float() @ p.float().T

    def similarity(self, q, p):
        assert q.dtype == p.dtype
        return self._scores("similarity", q, p).to(q.dtype)

    def similarity_f32(self, q, p):
        assert q.dtype == p.dtype and q.dtype in (torch.bfloat16, torch.float16)
        return self._scores("similarity_f32", q, p)

    def similarity_f32_planes(self, qp, cp):
        assert qp.dtype == cp.dtype == torch.bfloat16 and qp.shape[1] == cp.shape[1] == 3 * D
        return self._scores("similarity_f32_planes", qp, cp)

    @staticmethod
    def _merge(scores, col0, best_val, best_idx, k):
        idx = torch.arange(col0, col0 + scores.shape[1]).expand(scores.shape[0], -1)
        v, i = scores.float(), idx
        if best_val is not None:
            v, i = torch.cat([best_val, v], 1), torch.cat([best_idx, i], 1)
        top = torch.topk(v, k, dim=1)
        return top.values, i.gather(1, top.indices)

    def topk_merge(self, scores, col0, best_val=None, best_idx=None, k=100, split=1):
        assert split == 1
        self.log.append(("topk_merge", col0, col0 + scores.shape[1], None))
        return self._merge(scores, col0, best_val, best_idx, k)

    def _step(self, name, q, p, col0, best_val, best_idx, ws, rnd):
        scores = self._scores(name, q, p, rnd)
        assert col0 == self.log[-1][1] and (ws.rows, ws.k) == best_val.shape == best_idx.shape
        if rnd:
            scores = scores.to(q.dtype)
        v, i = self._merge(scores, col0, best_val, best_idx, best_val.shape[1])
        best_val.copy_(v)
        best_idx.copy_(i)
        if self.steps == self.overflow_at:
            ws.overflow.fill_(1)
        self.steps += 1
        return best_val, best_idx

    def search_step(self, q, p, col0, best_val, best_idx, ws, round_scores=True):
        return self._step("search_step", q, p, col0, best_val, best_idx, ws, bool(round_scores))

    def search_step_planes(self, qp, cp, col0, best_val, best_idx, ws):
        return self._step("search_step_planes", qp, cp, col0, best_val, best_idx, ws, None)


def make_index(data, kind, fused=True):
    """kind: f32 | f32+bf16 | f32+fp16 | bf16 | planes -> (index, queries f32, reference score matrix)."""
    emb, q = data[{"f32+bf16": "bf16", "f32+fp16": "fp16", "bf16": "bf16"}.get(kind, "f32")]
    ix = retrieval.FlatIPIndex(emb, device="cpu", dtype=torch.bfloat16 if kind == "bf16" else torch.float32, chunk_rows=CHUNK_ROWS,
                               exact16=False)
    assert ix.emb16 is None and ix.emb_planes is None               # nothing is "exact" without a GPU: set by hand
    if kind == "f32+bf16":
        ix.emb16 = emb.to(torch.bfloat16)
    elif kind == "f32+fp16":
        ix.emb16 = emb.to(torch.float16)
    elif kind == "planes":
        ix.emb_planes, inexact = ops.split_bf16x3_ref(emb)
        assert not bool(inexact)
    ix.fused = fused
    return ix, q, q @ emb.T


def walk(sched, scores, step=None, rnd=None, first_scores=None, fallback=()):
    """The expected calls of one walk: the score matrix + topk_merge on a chunk that starts below k, is refused, or when there is
    no step; the step otherwise."""
    out = []
    for c0, c1 in sched:
        if step is not None and c0 >= K and c0 not in fallback:
            out.append((step, c0, c1, rnd))
        else:
            out += [("similarity" if c0 in fallback else scores, c0, c1, None), ("topk_merge", c0, c1, None)]
    return out


def check_winners(out, ref, exact_scores=True):
    vals, idx = out
    assert vals.shape == idx.shape == (NQ, K) and vals.dtype == torch.float32 and idx.dtype == torch.int64
    want = torch.topk(ref, K, dim=1)
    if exact_scores:
        assert torch.allclose(vals, want.values, rtol=1e-4, atol=1e-4)
        assert (idx == want.indices).float().mean() > 0.999         # chunked and whole products differ in the last bit at most
    else:
        assert torch.allclose(vals, want.values, rtol=2 ** -7, atol=2 ** -7)       # bf16 scores


SPLIT = [("split_bf16x3", None, None, None)]
# kind -> (calls of a fused search, calls of a search with fused off)
EXPECTED = {
    "f32": (walk(PLAIN, "similarity"), walk(PLAIN, "similarity")),
    "f32+bf16": (walk(FUSED, "similarity_f32", "search_step", False), walk(PLAIN, "similarity_f32")),
    "f32+fp16": (walk(FUSED, "similarity_f32", "search_step", False), walk(PLAIN, "similarity_f32")),
    "bf16": (walk(FUSED, "similarity", "search_step", True), walk(PLAIN, "similarity")),
    "planes": (SPLIT + walk(FUSED, "similarity_f32_planes", "search_step_planes"), SPLIT + walk(FUSED, "similarity_f32_planes")),
}


def test_schedules_are_the_ones_the_cases_name(data, monkeypatch):
    Fakes(monkeypatch)
    for kind in EXPECTED:
        ix, q, _ = make_index(data, kind)
        assert ix.chunk_schedule(NQ, K, False) == PLAIN
        assert ix.chunk_schedule(NQ, K, True) == (PLAIN if kind == "f32" else FUSED)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kind", list(EXPECTED))
def test_search_calls_per_index_kind(data, monkeypatch, kind, fused):
    f = Fakes(monkeypatch)
    ix, q, ref = make_index(data, kind, fused)
    out = ix.search(q, K)
    assert f.log == EXPECTED[kind][0 if fused else 1]
    assert ix.fused is fused and ix.fused_overflows == 0
    check_winners(out, ref, exact_scores=kind != "bf16")
    if kind == "planes":                                            # decided for all chunks up front, not asked again
        assert f.preds == [("search_planes_takes", c0, c1) for c0, c1 in FUSED]
    elif kind == "f32":
        assert f.preds == []
    else:                                                           # asked per chunk
        assert f.preds == [("search_filter_takes", c0, c1) for c0, c1 in (FUSED if fused else PLAIN)]


def test_queries_not_exact_in_16_bits_take_the_plain_kernel(data, monkeypatch):
    f = Fakes(monkeypatch)
    ix, _, _ = make_index(data, "f32+bf16")
    emb, q = data["f32"]                                            # queries with full f32 mantissas
    out = ix.search(q, K)
    assert f.log == walk(PLAIN, "similarity") and f.preds == []
    check_winners(out, q @ ix.emb.T)


@pytest.mark.parametrize("kind", ["f32+bf16", "f32+fp16", "bf16"])
def test_overflow_on_the_16_bit_frames_redoes_the_plain_schedule(data, monkeypatch, kind):
    f = Fakes(monkeypatch, overflow_at=0)
    ix, q, ref = make_index(data, kind)
    out = ix.search(q, K)
    first, plain = EXPECTED[kind]
    assert f.log == first + plain
    assert ix.fused_overflows == 1 and ix.fused is True
    check_winners(out, ref, exact_scores=kind != "bf16")
    f.log.clear()
    f.overflow_at = None                                            # the next search is fused again
    ix.search(q, K)
    assert f.log == first and ix.fused_overflows == 1


def test_overflow_on_planes_redoes_the_same_schedule_without_steps(data, monkeypatch):
    f = Fakes(monkeypatch, overflow_at=1)                           # the second (last) step call raises the flag
    ix, q, ref = make_index(data, "planes")
    out = ix.search(q, K)
    first, matrix = EXPECTED["planes"]
    assert f.log == first + matrix[1:]                              # the queries are split once
    assert not any(c[0] == "search_step_planes" for c in f.log[len(first):])
    assert ix.fused_overflows == 1 and ix.fused is True
    check_winners(out, ref)


@pytest.mark.parametrize("kind", ["f32+bf16", "f32+fp16"])
def test_a_refused_chunk_alone_goes_to_similarity(data, monkeypatch, kind):
    c0 = FUSED[1][0]
    f = Fakes(monkeypatch, refuse=[c0])
    ix, q, ref = make_index(data, kind)
    out = ix.search(q, K)
    assert f.log == walk(FUSED, "similarity_f32", "search_step", False, fallback=(c0,))
    assert f.log[2:4] == [("similarity", FUSED[1][0], FUSED[1][1], None), ("topk_merge", FUSED[1][0], FUSED[1][1], None)]
    check_winners(out, ref)
    # the first chunk refused: its score matrix comes from `similarity` too
    f2 = Fakes(monkeypatch, refuse=[0])
    out = ix.search(q, K)
    assert f2.log == walk(FUSED, "similarity_f32", "search_step", False, fallback=(0,))
    check_winners(out, ref)


def test_a_refused_bf16_chunk_goes_through_its_score_matrix(data, monkeypatch):
    c0 = FUSED[2][0]
    f = Fakes(monkeypatch, refuse=[c0])
    ix, q, ref = make_index(data, "bf16")
    out = ix.search(q, K)
    assert f.log == walk(FUSED, "similarity", "search_step", True, fallback=(c0,))
    check_winners(out, ref, exact_scores=False)


def test_planes_with_a_refused_chunk_return_to_the_plain_kernel(data, monkeypatch):
    f = Fakes(monkeypatch, refuse=[FUSED[1][0]])
    ix, q, ref = make_index(data, "planes")
    out = ix.search(q, K)
    assert f.log == SPLIT + walk(PLAIN, "similarity")
    assert f.preds == [("search_planes_takes", c0, c1) for c0, c1 in FUSED[:2]]
    check_winners(out, ref)


def test_planes_with_an_inexact_query_only_split_it(data, monkeypatch):
    f = Fakes(monkeypatch)
    ix, q, _ = make_index(data, "planes")
    q = q.clone()
    q[3, 5] = float("inf")
    ix.search(q, K)
    assert f.log == SPLIT + walk(PLAIN, "similarity") and f.preds == []
