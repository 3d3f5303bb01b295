"""Shared by tests/test_topk_parity_host.py (CPU) and tests/test_gpu_topk_parity.py (GPU): bit-exact parity of the selection kernels
behind FlatIPIndex.search -- topk_merge_kernel ("slow"), topk_merge_fast_kernel ("fast"), topk_merge_cand_kernel (rankpo_amd/csrc/
topk.hip) and the filter epilogues of sim_tile256_kernel (infonce.hip) -- on hard score rows.  Importing it needs no GPU.

Five parts.

(1) The reference: `select_ref` and `merge_ref`.  Independent of the kernels and of oracle.scoring_ref.topk_ref.
(2) The catalogue of score rows (`ROW_KINDS`, `make_row`): generators of (cols, k, seed) per storage dtype.  Beyond the kinds the
    suite was asked for it holds `nan_flood`, the row that showed the one defect these tests found (tests/test_gpu_topk_parity.py).
(3) Two CPU models of the kernels' CONTROL FLOW, `fast_kernel_model` and `slow_kernel_model`: which elements pass the block-uniform
    threshold of a step, how many (atomic order does not change a count), which branch follows.  A re-selection is a plain
    lexicographic sort, not the kernels' bitonic network; what they share with the kernels is the thread-to-column mapping, the list
    capacity and the branch conditions, restated from topk.hip.  Each returns the winners and the set of branches taken.
(4) `selection_kernel`: topk_launch's choice between the two kernels.
(5) The case table `CASES`, `build_case` (the padded and guarded score matrix of a case) and `run_models` (a case through the
    models, list by list as ops.topk_merge / ops.topk_finish run it).

Order (topk.hip `before`): value descending, ties by the smaller corpus index.  NaN never wins: `before` is false whenever one of
its values is a NaN, so a NaN score is never admitted to a list; a row with fewer than k non-NaN columns ends in the padding
(-inf, INT64_MAX).  A real -inf column beats the padding (equal value, smaller index).  +0.0 and -0.0 are equal in value (the tie
goes to the smaller index) and keep their sign bit in the output.
"""
import functools
import zlib

import numpy as np
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
TAG = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}             # Elem<T>::kVec: elements per 16 bytes
ESIZE = {torch.float32: 4, torch.bfloat16: 2, torch.float16: 2}
INT64_MAX = 2 ** 63 - 1
NEG_INF = float("-inf")

# topk.hip
TOPK_THREADS, TOPK_MAX_K, TOPK_CAP, TOPK_SEG, TOPK_SLOTS = 256, 1024, 2048, 1024, 4096
FAST_THREADS, FAST_DEPTH, FAST_MIN_SEG = 1024, 4, 4096
SORT_SIZES = [64, 128, 256, 512, 1024, 2048, 4096]
K_VALUES = [1, 63, 64, 65, 100, 1023, 1024]


def fast_seg(dtype):
    """Columns of one segment of the fast kernel: 1024 threads x one 16-byte vector."""
    return FAST_THREADS * VEC[dtype]


def fast_group(dtype):
    """Columns of one full group: 16 384 in f32, 32 768 in 16-bit storage."""
    return FAST_DEPTH * fast_seg(dtype)


# ------------------------------------------------------------------------------------------------
# (1) the reference
# ------------------------------------------------------------------------------------------------
def _f32(scores):
    if torch.is_tensor(scores):
        return scores.detach().float().cpu().numpy()
    return np.asarray(scores, dtype=np.float32)


def _order(v32, idx):
    """Positions of one list's non-NaN pairs, best first: value descending (compared as float64 of the stored values), then
    index ascending."""
    keep = np.nonzero(~np.isnan(v32))[0]
    o = np.lexsort((idx[keep], -v32[keep].astype(np.float64)))          # last key first: -value ascending, then index ascending
    return keep[o]


def _pad(v, i, k):
    n = len(v)
    if n >= k:
        return v[:k], i[:k]
    return (np.concatenate([v, np.full(k - n, -np.inf, dtype=np.float32)]),
            np.concatenate([i, np.full(k - n, INT64_MAX, dtype=np.int64)]))


def select_ref(scores, k, col0=0):
    """Top-k per row of `scores` [rows, cols] (numpy or torch, any storage dtype; a single row is taken as [1, cols]) ->
    (values f32 [rows, k] with the stored bit patterns, indices int64 [rows, k]).  Per row: the non-NaN (value, col0 + column)
    pairs sorted by value descending, then index ascending; the first k, padded with (-inf, INT64_MAX).  NaN never wins (module
    docstring)."""
    s = _f32(scores)
    s = s[None, :] if s.ndim == 1 else s
    cols = np.arange(s.shape[1], dtype=np.int64) + int(col0)
    vals = np.empty((s.shape[0], k), dtype=np.float32)
    idx = np.empty((s.shape[0], k), dtype=np.int64)
    for r in range(s.shape[0]):
        o = _order(s[r], cols)[:k]
        vals[r], idx[r] = _pad(s[r][o], cols[o], k)
    return vals, idx


def merge_ref(*lists, k=None):
    """The k best of the concatenation of `lists`, each a pair (values [rows, n_i], indices [rows, n_i]), in select_ref's order:
    the merge of chunk winners, of split lists, of winners and candidates.  The padding (-inf, INT64_MAX) sorts behind every real
    pair.  k defaults to the first list's width."""
    v = np.concatenate([_f32(a) for a, _ in lists], axis=1)
    i = np.concatenate([(b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)).astype(np.int64) for _, b in lists], axis=1)
    k = lists[0][0].shape[1] if k is None else k
    vals = np.empty((v.shape[0], k), dtype=np.float32)
    idx = np.empty((v.shape[0], k), dtype=np.int64)
    for r in range(v.shape[0]):
        o = _order(v[r], i[r])[:k]
        vals[r], idx[r] = _pad(v[r][o], i[r][o], k)
    return vals, idx


def bits32(x):
    """int32 view of f32 values (numpy or torch): -0.0 / +0.0 and the infinities compare by bit pattern."""
    if torch.is_tensor(x):
        return x.detach().contiguous().cpu().numpy().view(np.int32)
    return np.ascontiguousarray(x, dtype=np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------
# (2) the catalogue of score rows
# ------------------------------------------------------------------------------------------------
ROW_KINDS = ["normal", "ascending", "descending", "constant", "quantised", "plateau", "mostly_neg_inf", "pos_inf", "signed_zero",
             "late_spike", "quiet_then_flood", "nan_sprinkled", "nan_flood"]
NAN_KINDS = ("nan_sprinkled", "nan_flood")
PLATEAU_TIES = 2600                                    # > kTopkCap
_POS_BITS = {torch.bfloat16: 0x7f7f, torch.float16: 0x7bff}            # the largest finite value's bit pattern


def _seed(*parts):
    return zlib.crc32("/".join(str(p) for p in parts).encode()) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def ordered16(dtype):
    """Every finite value of a 16-bit dtype except -0, ascending (subnormals included), as a tensor of that dtype."""
    top = _POS_BITS[dtype]
    neg = np.arange(0x8000 + top, 0x8000, -1, dtype=np.int64)           # -max .. the smallest negative subnormal
    pos = np.arange(0, top + 1, dtype=np.int64)                         # +0 .. +max
    pat = np.concatenate([neg, pos]).astype(np.uint16).view(np.int16)
    return torch.from_numpy(pat.copy()).view(dtype)


def _ascending(cols, dtype):
    if dtype == torch.float32:
        return (torch.arange(cols, dtype=torch.float32) - cols // 2) * 0.5
    o = ordered16(dtype)
    assert cols <= len(o)
    return o[len(o) - cols:].clone()                                    # ends at the type's largest finite value


def _top_values(n, dtype):
    """n distinct large values, all above 4."""
    if dtype == torch.float32:
        return 8.0 + torch.arange(n, dtype=torch.float32)
    o = ordered16(dtype)
    return o[len(o) - n:].clone() if n else o[:0].clone()


def make_row(kind, cols, k, seed, dtype):
    """One score row [cols] of the catalogue in `dtype`; every value is exact in `dtype`.  `seed` tells the rows of a case apart."""
    g = torch.Generator().manual_seed(_seed(kind, cols, k, seed, TAG[dtype]))
    rs = np.random.RandomState(_seed("np", kind, cols, k, seed, TAG[dtype]))
    V = VEC[dtype]
    randn = lambda: torch.randn(cols, generator=g, dtype=torch.float32).to(dtype)      # noqa: E731
    if kind == "normal":
        x = randn()
    elif kind == "ascending":
        x = _ascending(cols, dtype)
    elif kind == "descending":
        x = _ascending(cols, dtype).flip(0).clone()
    elif kind == "constant":
        x = torch.full((cols,), 0.75 if dtype == torch.float32 else float(torch.finfo(dtype).max), dtype=dtype)
    elif kind == "quantised":
        x = torch.randint(0, 12, (cols,), generator=g).to(dtype)
    elif kind == "plateau":
        # k / 2 distinct large values; the plateau value 1 at > 2048 columns: a solid run across the first segment boundary of the
        # fast kernel (and across the chunk boundaries the table puts there), the rest spread evenly over the whole row; below: [-2, -1]
        x = (-1.0 - torch.rand(cols, generator=g)).to(dtype)
        ties = PLATEAU_TIES if cols >= 2 * PLATEAU_TIES else cols // 2
        run, S = ties // 2, fast_seg(dtype)
        lo = (S if cols > S + run else cols // 2) - run // 2
        at = np.zeros(cols, dtype=bool)
        at[lo:lo + run] = True
        rest = np.nonzero(~at)[0]
        at[rest[np.linspace(0, len(rest) - 1, ties - run).astype(np.int64)]] = True
        x[torch.from_numpy(at)] = 1.0
        free = np.nonzero(~at)[0]
        big = rs.choice(free, size=k // 2, replace=False)
        x[torch.from_numpy(big)] = _top_values(k // 2, dtype)
    elif kind == "mostly_neg_inf":
        x = torch.full((cols,), NEG_INF, dtype=dtype)
        n = min(k // 2, cols // 2)
        x[torch.from_numpy(rs.choice(cols, size=n, replace=False))] = randn()[:n]
    elif kind == "pos_inf":
        x = randn()
        at = rs.choice(cols, size=min(7, cols), replace=False)
        at[0] = cols - 1
        x[torch.from_numpy(at)] = float("inf")
    elif kind == "signed_zero":
        # +0, -0, and the smallest subnormals of either sign (f32 subnormals in f32 and bf16; fp16's own in fp16)
        sub = {torch.float32: 2.0 ** -149, torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}[dtype]
        pick = torch.randint(0, 8, (cols,), generator=g)
        table = torch.tensor([0.0, -0.0, 0.0, -0.0, sub, -sub, 3 * sub, -2 * sub], dtype=torch.float64)
        x = table[pick].to(dtype)
    elif kind == "late_spike":
        x = randn().clamp(-4.0, 4.0)
        x[cols - (V - 1):] = _top_values(V - 1, dtype)
    elif kind == "quiet_then_flood":
        # the first full group of the fast kernel: k + 10 values above the noise, each in another thread's columns, so that the
        # maxima bootstrap lets between k and k + 10 elements through: a short list is left behind.  Everything after that group is
        # above all of it: the next group's appends run over the list
        G, S = fast_group(dtype), fast_seg(dtype)
        x = torch.rand(cols, generator=g).to(dtype)
        n = min(k + 10, FAST_THREADS)
        tids = rs.choice(FAST_THREADS, size=n, replace=False)
        at = rs.randint(0, FAST_DEPTH, size=n) * S + tids * V + rs.randint(0, V, size=n)
        at = at[at < min(cols, G)]
        x[torch.from_numpy(at)] = (2.0 + torch.arange(len(at), dtype=torch.float32) / 16.0).to(dtype)
        if cols > G:
            x[G:] = (128.0 + torch.randint(0, 128, (cols - G,), generator=g).float()).to(dtype)
    elif kind == "nan_sprinkled":
        x = randn()
        at = rs.choice(cols, size=max(2, cols // 64), replace=False)
        at[0], at[1] = 0, cols - 1
        x[torch.from_numpy(at)] = float("nan")
    elif kind == "nan_flood":
        # the first full group: NaN but for k - 24 low values outside its first quarter-segment, so the list is still short of k
        # winners after it; behind it no NaN at all and everything higher: the next group's bootstrap quarter (256 V columns, all
        # of which pass an empty threshold) would come on top of those candidates if the kernel carried them
        G = fast_group(dtype)
        x = torch.full((cols,), float("nan"), dtype=dtype)
        n = max(0, min(k - 24, FAST_THREADS))
        at = 256 * V + rs.choice(min(cols, G) - 256 * V, size=n, replace=False)
        x[torch.from_numpy(at)] = (-1.0 - torch.rand(n, generator=g)).to(dtype)
        if cols > G:
            x[G:] = (1.0 + torch.rand(cols - G, generator=g)).to(dtype)
    else:
        raise ValueError(kind)
    assert x.dtype == dtype and x.shape == (cols,)
    return x


def thread_maxima(row32, V):
    """The 1024 thread maxima of the fast kernel's FIRST group over a row (f32 numpy): thread t owns columns
    [s SEG + t V, s SEG + (t + 1) V) of segments s = 0 .. 3.  NaN is skipped (fmaxf); a thread without a column holds -inf."""
    SEG = FAST_THREADS * V
    n = min(len(row32), FAST_DEPTH * SEG)
    full = np.full(FAST_DEPTH * SEG, -np.inf, dtype=np.float32)
    full[:n] = np.where(np.isnan(row32[:n]), -np.inf, row32[:n])
    return full.reshape(FAST_DEPTH, FAST_THREADS, V).max(axis=(0, 2))


# ------------------------------------------------------------------------------------------------
# (3) the control-flow models
# ------------------------------------------------------------------------------------------------
FAST_BRANCHES = ["maxima_taken", "maxima_declined", "quarter_first", "quarter_merge", "overflow_empty", "overflow_nonempty",
                 "reselect_half", "carry", "settle_carry", "ragged_tail", "short_group"] + ["sort%d" % n for n in SORT_SIZES]
SLOW_BRANCHES = ["reselect_count", "reselect_last", "no_reselect"]


def _before(v, ix, tv, ti):
    """topk.hip `before`, element-wise on numpy arrays (a NaN on either side: False)."""
    with np.errstate(invalid="ignore"):
        return (v > tv) | ((v == tv) & (ix < ti))


class _List:
    """The k winners of a list plus its pending candidates; `reselect` is the exact lexicographic selection."""

    def __init__(self, k, first, winners_in):
        self.k = k
        if first or winners_in is None:
            self.wv, self.wi = np.full(k, -np.inf, dtype=np.float32), np.full(k, INT64_MAX, dtype=np.int64)
        else:
            self.wv, self.wi = np.array(winners_in[0], dtype=np.float32), np.array(winners_in[1], dtype=np.int64)
            assert self.wv.shape == (k,) and self.wi.shape == (k,)
        self.cv, self.ci = np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.int64)

    @property
    def thr(self):
        return self.wv[self.k - 1], self.wi[self.k - 1]

    @property
    def count(self):
        return len(self.cv)

    def append(self, v, ix):
        self.cv, self.ci = np.concatenate([self.cv, v]), np.concatenate([self.ci, ix])

    def reselect(self):
        v, i = np.concatenate([self.wv, self.cv]), np.concatenate([self.wi, self.ci])
        o = np.lexsort((i, -v.astype(np.float64)))[:self.k]
        self.wv, self.wi = v[o], i[o]
        self.cv, self.ci = self.cv[:0], self.ci[:0]


def fast_kernel_model(row, k, V, first, winners_in=None, col0=0):
    """topk_merge_fast_kernel on ONE list: `row` the list's columns as f32 (numpy), `winners_in` = (values [k], indices [k]) of a
    merge call.  -> (values [k], indices [k], set of FAST_BRANCHES).  Groups of kFastDepth segments of 1024 V columns; thread t of
    segment s holds columns [s SEG + t V, + V).  Every step filters under ONE threshold (tv, ti) -- the kernel's registers, renewed
    by a re-selection or by the maxima bootstrap only -- so the number of appends is the number of elements that pass it, whatever
    the order of the atomics."""
    row = np.asarray(row, dtype=np.float32)
    cols, SEG = len(row), FAST_THREADS * V
    ix = np.arange(cols, dtype=np.int64) + int(col0)
    L = _List(k, first, winners_in)
    cap = min(TOPK_SLOTS - k, TOPK_CAP)
    br = set()
    thr = list(L.thr)                                    # tv, ti

    def reselect():
        assert L.count <= cap, "the model never lets a list run over"
        n = 64
        while n < k + L.count:
            n <<= 1
        br.add("sort%d" % n)
        L.reselect()
        thr[0], thr[1] = L.thr

    def passing(lo, hi):
        """The elements of columns [lo, hi), clipped to the row, that pass the current threshold."""
        lo, hi = min(lo, cols), min(hi, cols)
        m = _before(row[lo:hi], ix[lo:hi], thr[0], thr[1])
        return row[lo:hi][m], ix[lo:hi][m]

    nseg = -(-cols // SEG)
    for s0 in range(0, nseg, FAST_DEPTH):
        g_lo, g_hi = s0 * SEG, min(cols, (s0 + FAST_DEPTH) * SEG)
        if nseg - s0 < FAST_DEPTH:
            br.add("short_group")
        if g_hi == cols and cols % V:
            br.add("ragged_tail")                        # one thread's vector straddles the end: the element-wise fetch
        boot = thr[0] == -np.inf and thr[1] == INT64_MAX
        if boot and L.count:
            # a list still short of k winners that carries candidates (a group of mostly NaN) is settled before the bootstrap
            # quarter, whose 256 V appends would not fit the list on top of them in 16-bit storage
            br.add("settle_carry")
            reselect()
            boot = thr[0] == -np.inf and thr[1] == INT64_MAX
        if boot and first and s0 == 0:
            t0 = np.sort(thread_maxima(row, V))[::-1][k - 1]
            if t0 > -np.inf:
                br.add("maxima_taken")
                boot, thr[0] = False, t0                 # ties at t0 all pass: the index bound stays INT64_MAX
            else:
                br.add("maxima_declined")
        q_hi = g_lo
        if boot:
            br.add("quarter_first" if first else "quarter_merge")
            q_hi = g_lo + 256 * V
            v, i = passing(g_lo, q_hi)
            assert L.count == 0
            L.append(v, i)
            reselect()
        before_count = L.count
        v, i = passing(q_hi, g_hi)
        count = before_count + len(v)
        if count > cap:
            br.add("overflow_nonempty" if before_count else "overflow_empty")
            reselect()                                   # settles what was there; after the maxima bootstrap: an empty threshold again
            for u in range(min(FAST_DEPTH, nseg - s0)):
                for part in range(4):
                    lo = (s0 + u) * SEG + part * 256 * V
                    if boot and u == 0 and part == 0:
                        continue                         # the bootstrap quarter is in already
                    v, i = passing(lo, lo + 256 * V)
                    if len(v):
                        L.append(v, i)
                        reselect()
        elif count > cap // 2:
            br.add("reselect_half")
            L.append(v, i)
            reselect()
        else:
            if len(v):
                br.add("carry")
            L.append(v, i)
    if L.count:
        reselect()
    return L.wv, L.wi, br


def slow_kernel_model(row, k, V=None, first=True, winners_in=None, col0=0):
    """topk_merge_kernel on one list: segments of 1024 columns, a re-selection when the list could run over during the next segment
    (count > kTopkCap - kTopkSeg) or after the last segment with anything pending.  -> (values, indices, set of SLOW_BRANCHES)."""
    row = np.asarray(row, dtype=np.float32)
    cols = len(row)
    ix = np.arange(cols, dtype=np.int64) + int(col0)
    L = _List(k, first, winners_in)
    br = set()
    for c0 in range(0, cols, TOPK_SEG):
        cend = min(c0 + TOPK_SEG, cols)
        tv, ti = L.thr
        m = _before(row[c0:cend], ix[c0:cend], tv, ti)
        L.append(row[c0:cend][m], ix[c0:cend][m])
        assert L.count <= TOPK_CAP
        if L.count > TOPK_CAP - TOPK_SEG:
            br.add("reselect_count")
            L.reselect()
        elif cend == cols and L.count > 0:
            br.add("reselect_last")
            L.reselect()
        else:
            br.add("no_reselect")
    return L.wv, L.wi, br


# ------------------------------------------------------------------------------------------------
# (4) the launch's choice
# ------------------------------------------------------------------------------------------------
def split_seg(cols, split, dtype):
    """topk_launch: a list's columns, ceil(cols / split) rounded up to whole 16-byte vectors (split == 1: the chunk)."""
    V = VEC[dtype]
    return cols if split == 1 else -(-(-(-cols // split)) // V) * V


def selection_kernel(scores, split=1):
    """'fast' or 'slow' as topk_launch chooses for the chunk `scores` ([rows, cols] tensor or view): the streaming kernel needs a
    row stride that is a multiple of the vector length, a 16-byte aligned base and lists of >= 4096 columns.  The base's alignment
    is judged by the view's offset in its allocation (allocations are at least 16-byte aligned on either device)."""
    V = VEC[scores.dtype]
    seg = split_seg(scores.shape[1], split, scores.dtype)
    aligned = (scores.storage_offset() * ESIZE[scores.dtype]) % 16 == 0
    return "fast" if scores.stride(0) % V == 0 and aligned and seg >= FAST_MIN_SEG else "slow"


# ------------------------------------------------------------------------------------------------
# (5) the case table
# ------------------------------------------------------------------------------------------------
GUARD_ROWS = 2


def _case(name, dtype, kinds, cols, k, cuts=(), order=None, split=1, col0=0, ld=None):
    """cuts: the inner chunk boundaries; order: the chunks' delivery order (default: ascending); ld: the row stride (default: the
    columns rounded up to a vector, plus two vectors of padding)."""
    V = VEC[dtype]
    bounds = [0] + list(cuts) + [cols]
    chunks = [(a, b) for a, b in zip(bounds, bounds[1:])]
    assert all(a < b for a, b in chunks) and k in K_VALUES
    order = list(range(len(chunks))) if order is None else list(order)
    assert sorted(order) == list(range(len(chunks)))
    return {"name": "%s-%s" % (TAG[dtype], name), "dtype": dtype, "kinds": list(kinds), "rows": len(kinds), "cols": cols, "k": k,
            "chunks": [chunks[j] for j in order], "split": split, "col0": col0,
            "ld": (-(-cols // V) + 2) * V if ld is None else ld}


def _odd_ld(cols, V):
    """The smallest row stride >= cols + V with stride % V == 1."""
    return cols + (1 - cols) % V + V


def cases(dtype):
    """The table for one storage dtype.  S = one segment of the fast kernel, G = one full group; R = G + ~S ragged columns: a second,
    short group.  Every case is there for a branch or a feature no earlier case reaches (tests/test_topk_parity_host.py)."""
    V, S, G = VEC[dtype], fast_seg(dtype), fast_group(dtype)
    R = G + (S * 7) // 8 + V - 1                         # 19 971 f32 / 39 943 16-bit columns: R % V == V - 1
    c = []
    f = lambda *a, **kw: c.append(_case(*a, **kw))       # noqa: E731
    # -- the fast kernel, first call, one chunk: the whole catalogue over the k values
    f("cat-k100", dtype, ["normal", "ascending", "descending", "constant", "quantised", "plateau", "mostly_neg_inf", "pos_inf"], R, 100)
    f("cat2-k100", dtype, ["signed_zero", "late_spike", "quiet_then_flood", "nan_sprinkled"], R, 100)
    f("cat-k1", dtype, ["normal", "ascending", "constant", "mostly_neg_inf", "signed_zero", "late_spike", "nan_sprinkled"], R, 1)
    f("cat-k63", dtype, ["descending", "plateau", "quiet_then_flood", "pos_inf"], R, 63)
    f("cat-k64", dtype, ["descending", "plateau", "quiet_then_flood", "quantised"], R, 64)
    f("cat-k65", dtype, ["descending", "plateau", "quiet_then_flood", "mostly_neg_inf"], R, 65)
    f("cat-k1023", dtype, ["normal", "ascending", "descending", "constant", "plateau", "mostly_neg_inf", "nan_sprinkled"], R, 1023)
    f("cat-k1024", dtype, ["normal", "ascending", "descending", "quantised", "plateau", "mostly_neg_inf", "signed_zero", "late_spike"],
      R, 1024)
    # -- a list short of k winners that carries candidates into the next group's bootstrap quarter (a first group of mostly NaN)
    f("nan-flood-k1024", dtype, ["nan_flood", "normal", "nan_flood"], G + S + 3, 1024)
    if dtype != torch.float32:
        # 16-bit rows: the 512-slot sort and the `count > cap / 2` re-selection of a first call, which the catalogue leaves out:
        # quantised chunks whose count of 11s sets k + count (k = 1; ~340 of 4096 and ~1365 of 16 384 columns)
        f("quant-k1-half", dtype, ["quantised", "quantised"], 4096, 1)
        f("quant-k1-2seg", dtype, ["quantised", "quantised"], 16384, 1)
    if dtype == torch.float32:
        # f32 reaches the 4096-slot sort only with k + count > 2048 in ONE group (a replayed quarter offers 1024 elements): a merge
        # call on 8192 columns behind 6000, k = 1024: ~1400 of them beat the k-th winner
        f("merge-half-k1024", dtype, ["normal", "normal"], 6000 + 8192, 1024, cuts=[6000])
    # -- chunked: merge calls of the fast kernel (chunks cut on vector boundaries), in and out of order, a large col0
    f("chunks-k100", dtype, ["normal", "ascending", "descending", "plateau", "quantised", "nan_sprinkled"], R, 100, cuts=[S, 3 * S])
    f("chunks-rev-k64", dtype, ["normal", "ascending", "plateau", "pos_inf", "signed_zero"], R, 64, cuts=[S, 2 * S], order=[2, 0, 1])
    f("chunks-col0-k1024", dtype, ["normal", "descending", "plateau", "mostly_neg_inf"], R, 1024, cuts=[G], order=[1, 0], col0=2 ** 40)
    # -- a first chunk shorter than k (slow kernel), completed by a later chunk: the fast kernel's quarter bootstrap on a merge call
    f("short-then-fast-k100", dtype, ["normal", "ascending", "constant", "mostly_neg_inf", "nan_sprinkled"], 5 * V + R, 100, cuts=[5 * V])
    f("short-then-fast-k1024", dtype, ["normal", "descending", "quantised"], 64 * V + S + 3, 1024, cuts=[64 * V])
    # -- the slow kernel: short chunks, cols < k and cols == k, a list completed later, an unaligned row stride
    f("slow-cols-lt-k", dtype, ["normal", "constant", "mostly_neg_inf", "nan_sprinkled", "signed_zero"], 37, 100)
    f("slow-cols-eq-k", dtype, ["normal", "ascending", "constant", "pos_inf"], 100, 100)
    f("slow-chunks-k65", dtype, ["normal", "ascending", "descending", "plateau", "quantised", "late_spike"], 4001, 65,
      cuts=[40, 1064, 3000], order=[1, 0, 3, 2])
    f("slow-unaligned-k100", dtype, ["normal", "ascending", "descending", "constant", "plateau", "pos_inf", "nan_sprinkled", "late_spike"],
      R, 100, ld=_odd_ld(R, V))                        # stride % V == 1: the streaming kernel must be declined
    f("slow-unaligned-k1023", dtype, ["ascending", "quantised", "mostly_neg_inf"], S + 5, 1023, cuts=[S // 2 + 1], ld=_odd_ld(S + 5, V))
    f("slow-col0-k1", dtype, ["normal", "constant", "signed_zero"], 3000, 1, cuts=[1000], order=[1, 0], col0=2 ** 40)
    # -- split lists: segments of >= 4096 columns (fast) and below (slow), a segment shorter than k, a segment of zero columns
    #    (lists of the fast kernel are never short: a segment below 4096 columns sends the whole launch to the slow kernel)
    f("split2-fast-k100", dtype, ["normal", "ascending", "plateau", "mostly_neg_inf", "late_spike", "signed_zero"], 2 * S + 3 * V + 1, 100, split=2)
    f("split4-fast-k64", dtype, ["normal", "descending", "plateau", "nan_sprinkled"], 2 * 16384 + 10 * V - 1, 64, split=4,
      cuts=[16384 + 8 * V], col0=2 ** 40)
    f("split8-fast-k1024", dtype, ["normal", "ascending", "constant", "quantised"], 8 * 4096 + 5, 1024, split=8)
    f("split2-slow-k100", dtype, ["normal", "ascending", "plateau", "pos_inf", "signed_zero"], 3001, 100, split=2, cuts=[1500], order=[1, 0])
    f("split8-slow-short-seg", dtype, ["normal", "descending", "constant", "mostly_neg_inf"], 7 * 40 + 3, 63, split=8)
    f("split4-slow-zero-seg", dtype, ["normal", "ascending", "quantised"], 3 * 2 * V, 1, split=4)
    return c


CASES = [c for t in DTYPES for c in cases(t)]


def build_case(case):
    """-> (matrix [GUARD_ROWS + rows + GUARD_ROWS, ld] in the storage dtype: guard rows and the columns beyond `cols` hold +inf, so a
    read past a row's end or into a neighbour would win; rows [rows, cols]: the score rows themselves)."""
    dtype, cols, k = case["dtype"], case["cols"], case["k"]
    rows = torch.stack([make_row(kind, cols, k, r, dtype) for r, kind in enumerate(case["kinds"])])
    m = torch.full((case["rows"] + 2 * GUARD_ROWS, case["ld"]), float("inf"), dtype=dtype)
    m[GUARD_ROWS:GUARD_ROWS + case["rows"], :cols] = rows
    return m, rows


def chunk_view(m, case, c0, c1):
    return m[GUARD_ROWS:GUARD_ROWS + case["rows"], c0:c1]


def run_models(case, m=None, rows=None):
    """The case through the models, list by list as ops.topk_merge runs it, then `merge_ref` over a row's lists (ops.topk_finish).
    -> (values [rows, k], indices [rows, k], reach).  `reach` is what the case exercises, as strings: 'fast/first/<branch>' or
    'slow/merge/<branch>' for every branch a model took (FAST_BRANCHES, SLOW_BRANCHES), '<kernel>/<dtype>/<first|merge>/<split1|
    split>1>' for every launch, and per kernel the case's k, row kinds and features: '<kernel>/k100', '<kernel>/kind/plateau',
    '<kernel>/split4', '<kernel>/cols<k', '<kernel>/cols==k', '<kernel>/completes_short_list', '<kernel>/out_of_order',
    '<kernel>/segment_shorter_than_k', '<kernel>/zero_segment', '<kernel>/unaligned_stride', '<kernel>/col0>=2^40'."""
    if m is None:
        m, rows = build_case(case)
    dtype, k, split, V = case["dtype"], case["k"], case["split"], VEC[case["dtype"]]
    r32 = rows.float().numpy()
    lists = [[None] * split for _ in range(case["rows"])]
    reach, kernels = set(), set()
    for n, (c0, c1) in enumerate(case["chunks"]):
        view = chunk_view(m, case, c0, c1)
        kern = selection_kernel(view, split)
        kernels.add(kern)
        model = fast_kernel_model if kern == "fast" else slow_kernel_model
        first, fm = n == 0, "first" if n == 0 else "merge"
        cols = c1 - c0
        seg = split_seg(cols, split, dtype)
        reach.add("%s/%s/%s/%s" % (kern, TAG[dtype], fm, "split1" if split == 1 else "split>1"))
        for r in range(case["rows"]):
            for s in range(split):
                lo, hi = min(cols, s * seg), min(cols, (s + 1) * seg)
                if split > 1 and hi - lo == 0:
                    reach.add("%s/zero_segment" % kern)
                elif split > 1 and hi - lo < k:
                    reach.add("%s/segment_shorter_than_k" % kern)
                if not first and lists[r][s][1][k - 1] == INT64_MAX and hi > lo:
                    reach.add("%s/completes_short_list" % kern)
                wv, wi, br = model(r32[r, c0 + lo:c0 + hi], k, V, first, lists[r][s], col0=case["col0"] + c0 + lo)
                lists[r][s] = (wv, wi)
                reach.update("%s/%s/%s" % (kern, fm, b) for b in br)
    merged = [merge_ref(*[(a[None], b[None]) for a, b in lists[r]], k=k) for r in range(case["rows"])]
    vals, idx = np.stack([v[0] for v, _ in merged]), np.stack([i[0] for _, i in merged])
    feats = {"split%d" % split, "k%d" % k} | {"kind/" + kind for kind in case["kinds"]}
    if case["cols"] < k:
        feats.add("cols<k")
    if case["cols"] == k:
        feats.add("cols==k")
    if [a for a, _ in case["chunks"]] != sorted(a for a, _ in case["chunks"]):
        feats.add("out_of_order")
    if case["col0"] >= 2 ** 40:
        feats.add("col0>=2^40")
    if case["ld"] % V:
        feats.add("unaligned_stride")
    reach.update("%s/%s" % (kern, x) for kern in kernels for x in feats)
    return vals, idx, reach
