"""CPU side of the selection-kernel parity suite (tests/topk_parity_util.py; the GPU side is tests/test_gpu_topk_parity.py): the
reference is the documented order and agrees with two other statements of it, every row generator has the property it is in the
catalogue for, the control-flow models of the two kernels return the reference's winners on every table entry, and the table
reaches every branch of both kernels in every storage dtype -- which is what keeps the GPU tests from being vacuous."""
import functools

import numpy as np
import pytest
import torch

import topk_parity_util as U
from oracle.scoring_ref import topk_ref

IDS = [c["name"] for c in U.CASES]
BY_NAME = {c["name"]: c for c in U.CASES}


@functools.lru_cache(maxsize=None)
def _built(name):
    return U.build_case(BY_NAME[name])


@functools.lru_cache(maxsize=None)
def _modelled(name):
    m, rows = _built(name)
    return U.run_models(BY_NAME[name], m, rows)


def _same(got, want):
    return np.array_equal(U.bits32(got[0]), U.bits32(want[0])) and np.array_equal(got[1], want[1])


def _torch_lex(rows, k):
    """value descending, index ascending, by two stable torch sorts in float64."""
    v = rows.double()
    o = torch.sort(v, dim=1, descending=True, stable=True).indices[:, :k]          # columns are already index-ascending
    return rows.float().gather(1, o).numpy(), o.numpy()


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in IDS if BY_NAME[n]["cols"] >= BY_NAME[n]["k"]])
def test_select_ref_equals_topk_ref_and_a_torch_sort(name):
    """Every NaN-free row of the table with cols >= k (the others: test_select_ref_padding_rule)."""
    case = BY_NAME[name]
    _, rows = _built(name)
    keep = [r for r, kind in enumerate(case["kinds"]) if kind not in U.NAN_KINDS]
    assert keep
    rows = rows[keep]
    got = U.select_ref(rows, case["k"])
    assert _same(got, topk_ref(rows.float().numpy(), case["k"]))
    assert _same(got, _torch_lex(rows, case["k"]))
    shifted = U.select_ref(rows, case["k"], col0=case["col0"] + 12345)
    assert np.array_equal(shifted[1], got[1] + case["col0"] + 12345) and np.array_equal(U.bits32(shifted[0]), U.bits32(got[0]))


def test_select_ref_by_hand():
    nan, inf = float("nan"), float("inf")
    row = np.array([nan, 0.0, -0.0, 2.0, -inf, 2.0, inf, nan, -1.0], dtype=np.float32)
    v, i = U.select_ref(row, 9, col0=10)
    assert i[0].tolist() == [16, 13, 15, 11, 12, 18, 14, U.INT64_MAX, U.INT64_MAX]          # the real -inf column beats the padding
    want = np.array([inf, 2.0, 2.0, 0.0, -0.0, -1.0, -inf, -inf, -inf], dtype=np.float32)
    assert np.array_equal(U.bits32(v[0]), U.bits32(want))                                   # +0 before -0: by index, signs kept
    v, i = U.select_ref(row, 2)
    assert i[0].tolist() == [6, 3] and v[0].tolist() == [inf, 2.0]
    # merge_ref: the same order over lists; the padding of a short list does not displace a real -inf
    a = (np.array([[2.0, -inf]], dtype=np.float32), np.array([[7, U.INT64_MAX]]))
    b = (np.array([[2.0, -inf]], dtype=np.float32), np.array([[3, 5]]))
    v, i = U.merge_ref(a, b, k=4)
    assert i[0].tolist() == [3, 7, 5, U.INT64_MAX] and v[0].tolist() == [2.0, 2.0, -inf, -inf]
    v, i = U.merge_ref(a, b)
    assert i[0].tolist() == [3, 7]


@pytest.mark.parametrize("name", [n for n in IDS if BY_NAME[n]["cols"] < BY_NAME[n]["k"] or set(BY_NAME[n]["kinds"]) & set(U.NAN_KINDS)])
def test_select_ref_padding_rule(name):
    """NaN never wins; fewer than k non-NaN columns: the real ones, best first, then (-inf, INT64_MAX)."""
    case = BY_NAME[name]
    _, rows = _built(name)
    k, col0 = case["k"], case["col0"]
    v, i = U.select_ref(rows, k, col0)
    r32 = rows.float().numpy()
    assert not np.isnan(v).any()
    for r in range(case["rows"]):
        real = int((~np.isnan(r32[r])).sum())
        n = min(k, real)
        assert (i[r, :n] >= col0).all() and (i[r, :n] < col0 + case["cols"]).all() and len(set(i[r, :n].tolist())) == n
        assert not np.isnan(r32[r][i[r, :n] - col0]).any()
        assert np.array_equal(U.bits32(v[r, :n]), U.bits32(r32[r][i[r, :n] - col0]))
        assert (i[r, n:] == U.INT64_MAX).all() and np.isneginf(v[r, n:]).all()
        # sorted: value descending, index ascending among equals; nothing left out beats the last one kept
        a, b = v[r, :n - 1].astype(np.float64), v[r, 1:n].astype(np.float64)
        assert (a >= b).all() and (np.diff(i[r, :n])[a == b] > 0).all()
        if n == k:
            out = np.ones(case["cols"], dtype=bool)
            out[i[r] - col0] = False
            out &= ~np.isnan(r32[r])
            cols = np.arange(case["cols"]) + col0
            assert not U._before(r32[r][out], cols[out], v[r, k - 1], i[r, k - 1]).any()


def test_merge_ref_of_chunks_and_segments_is_select_ref():
    rows = torch.stack([U.make_row(kind, 5000, 100, 3, torch.float32) for kind in ("normal", "plateau", "nan_sprinkled", "mostly_neg_inf")])
    want = U.select_ref(rows, 100, col0=2 ** 40)
    cuts = [0, 37, 2000, 2001, 5000]
    parts = [U.select_ref(rows[:, a:b], 100, col0=2 ** 40 + a) for a, b in zip(cuts, cuts[1:])]
    assert _same(U.merge_ref(*parts), want) and _same(U.merge_ref(*parts[::-1]), want)


# ------------------------------------------------------------------------------------------------
# the catalogue
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", U.DTYPES, ids=[U.TAG[t] for t in U.DTYPES])
@pytest.mark.parametrize("k", [1, 100, 1024])
def test_generators_have_the_property_they_claim(dtype, k):
    V, S, G = U.VEC[dtype], U.fast_seg(dtype), U.fast_group(dtype)
    cols = G + (S * 7) // 8 + V - 1
    cap = min(U.TOPK_SLOTS - k, U.TOPK_CAP)
    row = {kind: U.make_row(kind, cols, k, 1, dtype) for kind in U.ROW_KINDS}
    f = {kind: x.float().numpy() for kind, x in row.items()}
    for kind, x in row.items():
        assert x.dtype == dtype and x.shape == (cols,)
        assert torch.equal(x, U.make_row(kind, cols, k, 1, dtype)) or kind in U.NAN_KINDS           # deterministic
        assert bool(torch.isnan(x).any()) == (kind in U.NAN_KINDS)
    assert (np.diff(f["ascending"].astype(np.float64)) > 0).all() and (np.diff(f["descending"].astype(np.float64)) < 0).all()
    assert len(np.unique(f["constant"])) == 1 and np.isfinite(f["constant"]).all()
    assert set(np.unique(f["quantised"]).tolist()) == set(range(12))
    if dtype != torch.float32:
        top = float(torch.finfo(dtype).max)
        assert f["ascending"][-1] == top and f["descending"][0] == top and f["constant"][0] == top
    # plateau: k / 2 distinct values above it, > 2048 ties straddling the k-th place, across the first segment boundary and spread
    p = f["plateau"]
    ties = np.nonzero(p == 1.0)[0]
    assert len(ties) > U.TOPK_CAP and int((p > 1.0).sum()) == k // 2 == len(np.unique(p[p > 1.0])) and k // 2 < k <= k // 2 + len(ties)
    assert p[S - 1] == 1.0 and p[S] == 1.0 and ties[0] < S and ties[-1] >= G
    assert U.select_ref(p, k)[0][0, k - 1] == 1.0
    # mostly_neg_inf: fewer than k finite columns, hence fewer than k finite thread maxima; the rest are real -inf columns
    n = f["mostly_neg_inf"]
    assert int(np.isfinite(n).sum()) == k // 2 < k and np.isneginf(n[~np.isfinite(n)]).all()
    assert int(np.isfinite(U.thread_maxima(n, V)).sum()) < k
    assert (U.select_ref(n, k)[1] < cols).all()                                                   # real columns, not the padding
    assert int(np.isposinf(f["pos_inf"]).sum()) == 7 and np.isposinf(f["pos_inf"][-1])
    # signed_zero: both zeros and subnormals of either sign, nothing else
    z = row["signed_zero"]
    zb = U.bits32(z.float())
    assert (zb == 0).any() and (zb == np.int32(-2 ** 31)).any()
    tiny = torch.finfo(dtype).tiny
    assert bool((z.float().abs() < tiny).all()) and bool((z.float() > 0).any()) and bool((z.float() < 0).any())
    # late_spike: the V - 1 last columns (the ragged tail of the last vector) beat everything else
    s = f["late_spike"]
    assert cols % V == V - 1 and s[cols - (V - 1):].min() > s[:cols - (V - 1)].max()
    assert set(U.select_ref(s, min(k, V - 1))[1][0].tolist()) <= set(range(cols - (V - 1), cols))
    # nan_sprinkled: at both ends and in between
    nn = np.isnan(f["nan_sprinkled"])
    assert nn[0] and nn[-1] and nn[1:-1].sum() > 10 and (~nn).sum() > k
    # nan_flood (k > 24): fewer than k non-NaN columns in the first group, none in its first quarter-segment; behind it no NaN
    if k > 24:
        x = f["nan_flood"]
        live = ~np.isnan(x[:G])
        assert 0 < int(live.sum()) == k - 24 <= cap // 2 and not live[:256 * V].any() and not np.isnan(x[G:]).any()
        assert x[G:].min() > x[:G][live].max() and int(live.sum()) + 256 * V > cap - (dtype == torch.float32) * 2048
    # quiet_then_flood (k <= 1000): the first group leaves 1 .. cap / 2 candidates behind, the second runs the list over
    if k + 10 <= cap // 2:
        q = f["quiet_then_flood"]
        t0 = np.sort(U.thread_maxima(q, V))[::-1][k - 1]
        left = int((q[:G] >= t0).sum())
        assert k <= left <= k + 10 <= cap // 2
        assert q[G:].min() > q[:G].max() and cols - G > cap


# ------------------------------------------------------------------------------------------------
# the models and the table
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IDS)
def test_models_return_the_reference_winners(name):
    case = BY_NAME[name]
    _, rows = _built(name)
    vals, idx, _ = _modelled(name)
    assert _same((vals, idx), U.select_ref(rows, case["k"], case["col0"]))


def test_models_take_winners_in_and_follow_the_kernel_choice():
    """The two models agree with each other on one list, first call and merge call, for a threshold handed in."""
    row = U.make_row("plateau", 9001, 100, 5, torch.float32).float().numpy()
    a = U.slow_kernel_model(row[:4500], 100, 4, True, None, col0=7)
    b = U.fast_kernel_model(row[:4500], 100, 4, True, None, col0=7)
    assert _same(a[:2], b[:2])
    a2 = U.slow_kernel_model(row[4500:], 100, 4, False, a[:2], col0=4507)
    b2 = U.fast_kernel_model(row[4500:], 100, 4, False, b[:2], col0=4507)
    want = U.select_ref(row, 100, col0=7)
    assert _same(a2[:2], b2[:2]) and _same((a2[0][None], a2[1][None]), want)
    assert a2[2] <= set(U.SLOW_BRANCHES) and b2[2] <= set(U.FAST_BRANCHES)


@pytest.mark.parametrize("dtype", U.DTYPES, ids=[U.TAG[t] for t in U.DTYPES])
def test_table_reaches_every_branch(dtype):
    reach = set()
    for c in U.CASES:
        if c["dtype"] == dtype:
            reach |= _modelled(c["name"])[2]
    fast = sorted({r.split("/")[2] for r in reach if r.startswith(("fast/first/", "fast/merge/"))}, key=U.FAST_BRANCHES.index)
    slow = sorted({r.split("/")[2] for r in reach if r.startswith(("slow/first/", "slow/merge/"))}, key=U.SLOW_BRANCHES.index)
    print("%s fast: %s" % (U.TAG[dtype], " ".join(fast)))
    print("%s slow: %s" % (U.TAG[dtype], " ".join(slow)))
    assert fast == U.FAST_BRANCHES and slow == U.SLOW_BRANCHES
    assert "fast/first/quarter_first" in reach and "fast/merge/quarter_merge" in reach
    # every row kind and every k through both kernels; the features the table is asked to hold
    for kern in ("fast", "slow"):
        assert {"%s/kind/%s" % (kern, kind) for kind in U.ROW_KINDS if kind not in ("quiet_then_flood", "nan_flood")} <= reach, kern
        assert {"%s/k%d" % (kern, k) for k in U.K_VALUES if k != 64} <= reach, kern
        assert {"%s/split%d" % (kern, s) for s in (1, 2, 4, 8)} <= reach and "%s/col0>=2^40" % kern in reach
        assert "%s/out_of_order" % kern in reach
    assert {"fast/kind/quiet_then_flood", "fast/kind/nan_flood", "fast/k64", "fast/completes_short_list", "slow/cols<k", "slow/cols==k", "slow/unaligned_stride",
            "slow/segment_shorter_than_k", "slow/zero_segment"} <= reach


def test_every_case_reaches_something_new():
    """A case that reaches nothing beyond the earlier cases of its dtype is dropped, not kept."""
    seen = {}
    for c in U.CASES:
        reach = _modelled(c["name"])[2]
        s = seen.setdefault(c["dtype"], set())
        assert reach - s, c["name"]
        s |= reach


def test_selection_kernel_covers_both_kernels_in_every_mode():
    reach = set().union(*[_modelled(c["name"])[2] for c in U.CASES])
    want = {"%s/%s/%s/%s" % (kern, U.TAG[t], fm, sp) for kern in ("fast", "slow") for t in U.DTYPES for fm in ("first", "merge")
            for sp in ("split1", "split>1")}
    assert want <= reach, sorted(want - reach)
    # the rule itself, on views of one allocation
    for t in U.DTYPES:
        V = U.VEC[t]
        m = torch.zeros(4, 4096 * 8 + 2 * V, dtype=t)
        assert U.selection_kernel(m[:, :4096]) == "fast" and U.selection_kernel(m[:, :4095]) == "slow"
        assert U.selection_kernel(m[:, V:V + 4096]) == "fast" and U.selection_kernel(m[:, 1:4097]) == "slow"        # base off by one element
        assert U.selection_kernel(m[:, :4 * 4096], 4) == "fast" and U.selection_kernel(m[:, :4 * 4096 - 4 * V], 4) == "slow"
        assert U.selection_kernel(m[:, :4 * 4096 - 4 * V + 1], 4) == "fast"                                             # seg rounds up to a vector
        odd = torch.zeros(4, 4096 * 2 + 1, dtype=t)
        assert U.selection_kernel(odd[:, :4096]) == "slow"                                                          # stride % V != 0
    c = BY_NAME["f32-slow-unaligned-k100"]
    assert c["ld"] % 4 == 1 and c["ld"] >= c["cols"] + 4
