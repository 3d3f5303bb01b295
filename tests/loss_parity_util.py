"""Shared by tests/test_loss_parity_host.py (CPU) and tests/test_gpu_loss_parity.py (GPU): the case table, the hard-logit regimes
and the STATED tolerances of the loss-head parity tests (csrc/infonce.hip, csrc/rankpo.hip).

1. `infonce_path` is a pure-Python mirror of the host dispatch of csrc/infonce.hip: `make_plan` (lines 1456-1490) and the skinny
   sub-dispatch of `fwd_impl` (lines 1565-1609: the `sim_small_kernel` conditions 1569-1576, `ng` 1566, `one_block` 1591-1593,
   the ticket finalize 1597-1602).  `INFONCE_CASES` is checked against it, per dtype, by the host test.
   `skinny-multi+ce_finalize` is NOT reachable: a multi-block skinny launch hands lse / loss to `ce_finalize_kernel` only when
   statistics are requested without a score buffer (line 1597), and `rpo_infonce_fwd` refuses a null `scores_out` (line 1695).

2. Regimes: seeded builders of (q, p, T, marks) in float64; the tests round them to the storage dtype.

3. Tolerances introduced here (everything else is an existing test's number, named where it is used).

   Scores, float32: |s - s64| <= 3e-5 |s64| + 8 ulp32(max |s64|).  The existing shape tests allow 3e-5 absolute at T = 0.02, where
   the largest score of unit rows is 50 and ulp32(50) = 3.8e-6: 3e-5 is 8 ulps of the largest score, i.e. the float32 accumulation
   error of the dot product (bounded in units of |q| |p|, not of the dot itself) divided by T.  Kept in ulps it reads 2.4e-4 at
   |s| = 256 (T = 2^-8) and 1.5e-5 at |s| <= 16 (T = 1).

   lse, loss (float32 in the kernels, compared with the float64 max-subtracted logsumexp of the scores the kernel RETURNED):
     row i:   |lse_i  - lse64_i | <= N_LSE ulp32(A_i) + REL_LOG |lse64_i - m_i| + ABS_LOG,   A_i = max(|lse64_i|, |m_i|)
              |loss_i - loss64_i| <= N_ROW ulp32(max(A_i, |s_target,i|)) + the same two terms
     N_LSE = 2 roundings at the magnitude of the row maximum m: the product m * log2(e) inside exp_sub (it shifts every exponent of
     a block by the same amount, i.e. moves log l by at most half an ulp32(|m| log2 e) * ln 2 < half an ulp32(|m|)), and the sum
     m + logf(l).  N_ROW = 3 adds the difference lse - s_target.  REL_LOG = 2e-5 and ABS_LOG = 2e-6 are the project's existing
     rtol / atol of this check, applied to the log-sum part log l = lse - m alone (v_exp_f32 / v_log_f32 and the float32 sum of l).
     mean:    |loss - loss64| <= mean_i(row bound) + REDUCE_ROUNDINGS 2^-24 mean_i |loss64_i|
     REDUCE_ROUNDINGS = 24: block_sum is 6 shuffle levels + at most 7 serial adds over the waves, `ce_finalize_kernel` adds at most
     8 block sums (Q <= 2048 here), `first_finalize_kernel` 2 serial trips, and the division by Q: 24 >= 6 + 7 + 8 + 2 + 1.
   The host test evaluates the kernels' formulas in numpy float32 (block partials with the exp2 / fma form, merged in block order
   for every case's block width) and asserts that they stay inside these bounds; measured headroom is in its docstring.

   RankPO per-row loss against the float64 formulas on the RETURNED float32 scores:
     |l_b - l64_b| <= RANKPO_ROUNDINGS 2^-24 M_b + REL_LOG |log part| + ABS_LOG,
     M_b = (beta / T) (|c| + |r| + |ref_c| + |ref_r|) + beta |gamma| + (|c| + |r|) / T + 1
     RANKPO_ROUNDINGS = 10: c - r, ref_c - ref_r, their difference, / T, - gamma, * beta, log1pf's sum, the two label-smoothing
     products and their difference (sigmoid); c / T, r / T, m + logf, lse - t0 (SFT: 4 more, of the 10 only 2 are shared) -- each at
     most half an ulp of an intermediate that M_b bounds, so 10 units of 2^-24 M_b cover both chains.
"""
import numpy as np

import lowp_util as LU
from conftest import unit
from oracle import scoring_ref as R

DTYPES = ("f32", "bf16", "f16")
ELEM_SIZE = {"f32": 4, "bf16": 2, "f16": 2}
ULP_STORE = {"bf16": 2.0 ** -7, "f16": 2.0 ** -10}      # as tests/test_gpu_kernels.py and tests/test_gpu_f16.py (ULP16) use them
GL = 0.37                                               # grad_loss of the existing shape tests

N_LSE, N_ROW, REL_LOG, ABS_LOG, REDUCE_ROUNDINGS = 2, 3, 2e-5, 2e-6, 24
RANKPO_ROUNDINGS = 10
LOG2E32 = np.float32(1.4426950408889634)                # RPO_LOG2E


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------------ dispatch mirror
ALL_LABELS = ("small", "skinny4-1blk", "skinny1-1blk", "skinny-multi", "rowwise-chunk", "rowwise-k", "rowwise-unaligned",
              "tile64x64", "tile128x64", "tile128x128", "tile256")


def reachable_labels(tag):
    return set(ALL_LABELS) - (set() if tag == "bf16" else {"tile256"})


def infonce_path(Q, P, d, tag, aligned=True):
    """(label, columns per softmax partial) the forward takes; csrc/infonce.hip make_plan 1456-1490, fwd_impl 1565-1609."""
    es = ELEM_SIZE[tag]
    CE, KE = 16 // es, 128 // es                                       # 1459 (kTileRowBytes = 128)
    if not (aligned and d % CE == 0):                                  # 1460-1463
        return ("rowwise-chunk" if d % CE else "rowwise-unaligned"), 1
    if Q <= 64:                                                        # 1464-1467: PATH_SKINNY
        nPb = cdiv(P, 16)
        ng = 4 if Q <= 16 else 1                                       # 1566
        row_bytes = d * es                                             # 1569-1576: sim_small_kernel
        kcb = 1024
        while 2 * kcb < row_bytes:
            kcb *= 2
        lds = max((16 + 16 * nPb) * (kcb + 32), 8 * 8 * 64 * 16)       # kSmallMaxGroups = 8
        if (Q <= 16 and nPb <= 8 and kcb <= 8192 and Q * (kcb // 1024) <= 8 * 4 and P * (kcb // 1024) <= 8 * 14
                and lds <= 150 * 1024 and row_bytes % 16 == 0):        # kSmallQPieces = 4, kSmallPPieces = 14
            return "small", 16
        npass = cdiv(nPb, ng) * cdiv(Q, 16)                            # 1588
        one_block = nPb <= 16 and (Q + P) * d * es <= 384 * 1024       # 1591-1592 (kSkinnyMaxFusedGroups = 16)
        nblk = 1 if one_block else npass                               # 1593
        if nblk == 1:
            return f"skinny{ng}-1blk", 16
        return "skinny-multi", 16                                      # 1597-1602: scores_out is never null -> ticket finalize
    if d % KE != 0:                                                    # 1464, 1468-1470
        return "rowwise-k", 1
    big = (tag == "bf16" and cdiv(P, 256) * cdiv(Q, 256) >= 192 and P * d * 2 < 2 ** 32 and Q * d * 2 < 2 ** 32)   # 1474-1475
    if big:
        return "tile256", 256
    tp = tq = 128                                                      # 1477-1486
    if cdiv(P, 128) * cdiv(Q, 128) < 512:
        tq = 64
        if cdiv(P, 128) * cdiv(Q, 64) < 512:
            tp = 64
    return f"tile{tp}x{tq}", tp


# Q, P, d, dtypes, aligned.  Single-digit K-step counts (a K step is 128 bytes of a row) except the two d = 2048 skinny cases,
# whose paths are chosen by the BYTES of the problem (one_block: (Q + P) d es <= 384 KiB).
INFONCE_CASES = [
    (8, 48, 256, DTYPES, True),        # small
    (9, 27, 264, DTYPES, True),        # small, ragged second passage group, partial last 1 KiB piece
    (8, 64, 2048, DTYPES, True),       # skinny, 4 groups per pass, one block (f32: over 384 KiB but a single pass)
    (33, 99, 72, DTYPES, True),        # skinny, 1 group per pass, one block, ragged rows and columns
    (16, 270, 64, DTYPES, True),       # skinny, 17 groups > 16: 5 blocks, ticket finalize, ragged last group
    (40, 290, 72, DTYPES, True),       # skinny, 1 group per pass, 57 blocks
    (16, 96, 2048, DTYPES, True),      # skinny, 2 blocks because of its bytes
    (3, 9, 7, DTYPES, True),           # rowwise: d % CE != 0 for every dtype
    (100, 300, 72, DTYPES, True),      # rowwise: Q > 64, d % KE != 0 for every dtype (72 % 32, 72 % 64)
    (100, 300, 128, DTYPES, False),    # rowwise: q and p one element into a larger allocation
    (130, 390, 192, DTYPES, True),     # 64 x 64 tiles, ragged (3 / 6 K steps)
    (1000, 4000, 64, DTYPES, True),    # 128 x 64 tiles: 32 x 16 = 512 >= 512 > 32 x 8, ragged
    (2040, 4090, 64, DTYPES, True),    # 128 x 128 tiles: 32 x 16 = 512, ragged; bf16: 16 x 8 = 128 tiles of 256 < 192
    (2040, 6100, 64, ("bf16",), True),  # 256 x 256 tiles: 24 x 8 = 192, ragged (f32 / f16 would repeat 128 x 128)
]
INFONCE_REGIMES = ("hot", "cold", "flat", "split", "unscaled")
FIRST_CASES = [(300, 6, 64), (1, 1, 8), (8, 40, 2048), (5, 7, 36)]         # B, G, d (RPO_TARGET_FIRST)
FIRST_REGIMES = ("hot", "cold", "flat", "unscaled")
GEMM_CASE = (512, 1536, 128)                                                # ops._GEMM_BWD_MIN_PAIRS: 512 x 1536 >= 256 Ki
WINDOW_CASE = (40, 290, 72, (8, 16, 50, 100))                               # q_row0, q_rows, p_row0, p_rows
TWICE_CASE = (16, 270, 64)


def case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]}" + ("" if len(c) < 5 or c[4] else "-unaligned")


# ------------------------------------------------------------------------------------------------------------------ rounding
def round_store(x, tag):
    """float64 values of x after the cast to the storage dtype."""
    if tag == "f32":
        return np.asarray(x, dtype=np.float32).astype(np.float64)
    return LU.round_to(x, "bf16" if tag == "bf16" else "fp16")


def expected_scores(raw, T, tag):
    """The reference's rounding points on the float64 dots `raw`: round(round(dot) / T) in 16-bit storage, dot / T in float32."""
    if tag == "f32":
        return raw / T
    return round_store(round_store(raw, tag) / T, tag)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def score_errors(s, exp, tag):
    """(worst error in units of its tolerance, description).  f32: 3e-5 relative + 8 ulp32(max |exp|); 16-bit: 2 storage ulps,
    computed as test_infonce_forward_backward_shapes / test_infonce_f16_forward_backward_shapes do."""
    if tag == "f32":
        tol = 3e-5 * np.abs(exp) + 8 * ulp32(np.abs(exp).max())
        return float((np.abs(s - exp) / tol).max())
    ulps = (np.abs(s - exp) / (np.maximum(np.abs(exp), 1e-2) * ULP_STORE[tag])).max()
    return float(ulps / (2.0 + 1e-6))


# ------------------------------------------------------------------------------------------------------------------ InfoNCE regimes
def _rs(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 12345) % (2 ** 31)
    return np.random.RandomState(seed)


def _base(rs, Q, P, d, bump=True):
    q, p = unit(rs.randn(Q, d)), unit(rs.randn(P, d))
    G = P // Q
    if bump:
        tgt = np.arange(Q) * G
        p[tgt] = unit(p[tgt] + (2.0 / np.sqrt(d)) * q)
    return q, p


def infonce_regime(regime, Q, P, d, block_cols=16):
    """(q, p, T, marks) in float64.  target column of row i: i * (P // Q).  `block_cols`: columns per softmax partial of the path
    the case takes (for `split`)."""
    G = P // Q
    tgt = np.arange(Q) * G
    rs = _rs(INFONCE_REGIMES.index(regime), Q, P, d)
    marks = {"regime": regime, "target": tgt}
    if regime == "hot":
        T = 2.0 ** -8
        q, p = _base(rs, Q, P, d, bump=False)
        kind = np.arange(Q) % 3                       # 0: duplicate at the target; 1: at column 0; 2: at column P - 1
        assert Q == 1 or (P - 1) % G != 0 or (P - 1) // G >= Q, "column P - 1 must not be a target"
        q[kind == 1] = q[0]                           # column 0 is row 0's target (kind 0): the rows that peak there share q[0]
        if (kind == 2).any():
            q[kind == 2] = q[np.argmax(kind == 2)]
            p[P - 1] = q[np.argmax(kind == 2)]
        p[tgt[kind == 0]] = q[kind == 0]
        marks["kind"] = kind
        marks["planted"] = np.where(kind == 0, tgt, np.where(kind == 1, 0, P - 1))
    elif regime == "cold":
        T = 2.0 ** -8
        c = unit(rs.randn(d))
        q = unit(c + 0.3 * unit(rs.randn(Q, d)))
        p = -unit(c + 0.3 * unit(rs.randn(P, d)))
    elif regime == "flat":
        T = 2.0 ** -5
        u = unit(rs.randn(d))
        q, p = np.tile(u, (Q, 1)), np.tile(u, (P, 1))
    elif regime == "split":
        T = 2.0 ** -7
        q, p = _base(rs, Q, P, d, bump=False)
        taken = set(tgt.tolist())                     # a duplicate never overwrites a target row of p, nor another duplicate
        cols = np.zeros(Q, dtype=np.int64)
        for i in range(Q):                            # the first free column of another block, scanning from half a row away
            for c in ((tgt[i] + P // 2 + k) % P for k in range(P)):
                if c not in taken and c // block_cols != tgt[i] // block_cols:
                    break
            else:
                raise AssertionError("no column of another partial block left for row %d" % i)
            taken.add(int(c))
            cols[i] = c
        p[cols] = q
        marks["planted"] = cols
    elif regime == "unscaled":
        T = 1.0
        q, p = _base(rs, Q, P, d)
        q, p = 4.0 * q, 4.0 * p
    else:
        raise ValueError(regime)
    return q, p, T, marks


def first_regime(regime, B, G, d):
    """RPO_TARGET_FIRST inputs: q [B, d], p [B G, d], target g = 0."""
    rs = _rs(100 + FIRST_REGIMES.index(regime), B, G, d)
    marks = {"regime": regime}
    if regime == "hot":
        T = 2.0 ** -8
        q, p = unit(rs.randn(B, d)), unit(rs.randn(B * G, d))
        where = np.where(np.arange(B) < (B + 1) // 2, 0, G - 1)        # the planted maximum: g = 0, then g = G - 1
        p[np.arange(B) * G + where] = q
        marks["planted"] = where
    elif regime == "cold":
        T = 2.0 ** -8
        c = unit(rs.randn(d))
        q = unit(c + 0.3 * unit(rs.randn(B, d)))
        p = -unit(c + 0.3 * unit(rs.randn(B * G, d)))
    elif regime == "flat":
        T = 2.0 ** -5
        u = unit(rs.randn(d))
        q, p = np.tile(u, (B, 1)), np.tile(u, (B * G, 1))
    elif regime == "unscaled":
        T = 1.0
        q, p = 4.0 * unit(rs.randn(B, d)), 4.0 * unit(rs.randn(B * G, d))
    else:
        raise ValueError(regime)
    return q, p, T, marks


# ------------------------------------------------------------------------------------------------------------------ CE reference + bounds
def ce_from_scores(s, tgt):
    """float64 max-subtracted logsumexp / CE of the score matrix s [rows, cols]; target column tgt[i] of row i."""
    s = np.asarray(s, dtype=np.float64)
    rows = np.arange(s.shape[0])
    m = s.max(-1)
    logl = np.log(np.exp(s - m[:, None]).sum(-1))
    lse = m + logl
    st = s[rows, tgt]
    rowloss = lse - st
    return dict(m=m, logl=logl, lse=lse, s_target=st, rowloss=rowloss, loss=float(rowloss.mean()))


def lse_bound(ce):
    A = np.maximum(np.abs(ce["lse"]), np.abs(ce["m"]))
    return N_LSE * ulp32(A) + REL_LOG * np.abs(ce["logl"]) + ABS_LOG


def rowloss_bound(ce):
    A = np.maximum(np.maximum(np.abs(ce["lse"]), np.abs(ce["m"])), np.abs(ce["s_target"]))
    return N_ROW * ulp32(A) + REL_LOG * np.abs(ce["logl"]) + ABS_LOG


def loss_bound(ce):
    return float(rowloss_bound(ce).mean() + REDUCE_ROUNDINGS * 2.0 ** -24 * np.abs(ce["rowloss"]).mean())


def softmax_grads(s, ce, tgt, T, gl, qv, pv, first_G=None):
    """dq, dp in float64 from the returned scores: dS = gl (softmax - onehot) / (rows T).  Also sum_j |dS_ij| per row."""
    Q = s.shape[0]
    ds = np.exp(s - ce["lse"][:, None])
    ds[np.arange(Q), tgt] -= 1
    ds *= gl / Q / T
    if first_G is None:
        return ds, ds @ pv, ds.T @ qv
    pg = pv.reshape(Q, first_G, -1)
    return ds, np.einsum("bg,bgd->bd", ds, pg), np.einsum("bg,bd->bgd", ds, qv).reshape(pv.shape)


# ------------------------------------------------------------------------------------------------------------------ float32 emulation
def _fma32(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 values is exact, the sum is rounded once (then to float32;
    double rounding can differ from fmaf in the last bit only on exact ties)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _merge32(m, l, om, ol):
    """softmax_merge (csrc/infonce.hip 91-97) on float32 arrays."""
    with np.errstate(invalid="ignore", over="ignore"):
        M = np.maximum(m, om)
        a = np.where(np.isneginf(m), np.float32(0), l * np.exp((m - M).astype(np.float32)))
        b = np.where(np.isneginf(om), np.float32(0), ol * np.exp((om - M).astype(np.float32)))
    return M, (a + b).astype(np.float32)


def infonce_stats_f32(s, tgt, block_cols):
    """lse [rows], loss as the kernels compute them, in numpy float32: per block of `block_cols` columns the partial
    (max, sum exp2(fma(v, log2e, -max log2e))) -- columns past the end masked out --, partials merged in block order by
    softmax_merge, lse = m + logf(l), row loss = lse - s_target, float32 sum / rows.  block_cols = 1: the per-score merge of
    sim_rowwise_kernel and first_finalize_kernel."""
    s32 = np.asarray(s, dtype=np.float32)
    rows, cols = s32.shape
    if block_cols == 1:
        m = np.full(rows, -np.inf, np.float32)
        l = np.zeros(rows, np.float32)
        for j in range(cols):
            m, l = _merge32(m, l, s32[:, j], np.ones(rows, np.float32))
    else:
        nb = cdiv(cols, block_cols)
        pad = np.full((rows, nb * block_cols), -np.inf, np.float32)
        pad[:, :cols] = s32
        pad = pad.reshape(rows, nb, block_cols)
        bm = pad.max(-1)
        with np.errstate(invalid="ignore"):
            e = np.exp2(_fma32(pad, LOG2E32, -(bm * LOG2E32).astype(np.float32)[:, :, None]))
        e[np.isneginf(pad)] = 0
        bl = e.sum(-1, dtype=np.float32)
        m = np.full(rows, -np.inf, np.float32)
        l = np.zeros(rows, np.float32)
        for b in range(nb):
            m, l = _merge32(m, l, bm[:, b], bl[:, b])
    lse = (m + np.log(l)).astype(np.float32)
    rowloss = (lse - s32[np.arange(rows), tgt]).astype(np.float32)
    loss = np.float32(rowloss.sum(dtype=np.float32) / np.float32(rows))
    return lse.astype(np.float64), float(loss)


# ------------------------------------------------------------------------------------------------------------------ RankPO
RANKPO_SHAPES = [(1, 8, True), (3, 7, True), (5, 20, True), (300, 64, True), (4, 2056, True), (5, 64, False)]   # B, d, aligned
RANKPO_REGIMES = {
    # name: config, with_ref
    "sat": (dict(beta=10.0, temperature=2.0 ** -6, reference_free=True), False),
    "sat-smooth": (dict(beta=10.0, temperature=2.0 ** -6, label_smoothing=0.1, reference_free=True), False),
    "sat-ref": (dict(beta=10.0, temperature=2.0 ** -6, reference_free=False), True),
    "sat-ref-smooth": (dict(beta=10.0, temperature=2.0 ** -6, label_smoothing=0.1, reference_free=False), True),
    "sat-sft": (dict(beta=10.0, temperature=2.0 ** -6, sft_weight=0.5, reference_free=True), False),
    "hinge": (dict(beta=2.0, temperature=0.25, loss_type="hinge", reference_free=True), False),
    "sft-only": (dict(beta=2.0, temperature=0.25, rankpo_weight=0.0, sft_weight=1.0, reference_free=True), False),
    "gamma": (dict(beta=2.0, temperature=0.25, gamma_beta_ratio=0.5, reference_free=True), False),
}
RANKPO_DEFAULTS = dict(beta=0.1, temperature=1.0, gamma_beta_ratio=0.0, label_smoothing=0.0, rankpo_weight=1.0, sft_weight=0.0,
                       loss_type="sigmoid", reference_free=False)


def rankpo_config(name):
    return dict(RANKPO_DEFAULTS, **RANKPO_REGIMES[name][0])


def rankpo_regime(name, B, d, tag):
    """(q [B, d], p [2 B, d], ref_chosen, ref_rejected, marks): values already rounded to the storage dtype `tag` (ref scores are
    float32).  p rows are c_b q_b / r_b q_b plus noise of norm 0.01, so chosen / rejected scores are c_b, r_b to within 0.01."""
    cfg = rankpo_config(name)
    rs = _rs(200 + list(RANKPO_REGIMES).index(name), B, d)
    q = unit(rs.randn(B, d))
    marks = {"kink": np.zeros(B, bool)}
    if name.startswith("sat"):
        table = np.array([(0.95, 0.05), (0.05, 0.95), (0.9, -0.9), (-0.9, 0.9)])      # c - r = +-0.9, +-1.8
        cr = table[np.arange(B) % 4]
    else:
        cr = rs.uniform(-1, 1, size=(B, 2))
    noise = 0.01 * unit(rs.randn(2 * B, d))
    p = np.repeat(q, 2, 0) * cr.reshape(-1, 1) + noise
    if name == "hinge":
        kink = np.arange(B) % 3 == 0
        q[kink] = 0
        q[kink, 0] = 1                                                   # q = e0, c = 0.5, r = 0.375: beta (c - r) / T == 1 exactly
        p[np.repeat(kink, 2)] = 0
        p[np.flatnonzero(kink) * 2, 0] = 0.5
        p[np.flatnonzero(kink) * 2 + 1, 0] = 0.375
        marks["kink"] = kink
    q, p = round_store(q, tag), round_store(p, tag)
    rc = rr = None
    if RANKPO_REGIMES[name][1]:
        # comparable size, and on the side that keeps |beta z| saturated: (rc - rr) has the sign of -(c - r)
        gap = -np.sign(cr[:, 0] - cr[:, 1]) * rs.uniform(0.1, 0.9, size=B)
        mid = rs.uniform(-0.3, 0.3, size=B)
        rc, rr = round_store(mid + gap / 2, "f32"), round_store(mid - gap / 2, "f32")
    if name == "hinge":
        s = R.rankpo_scores(q, p)
        hz = 1 - cfg["beta"] * ((s[:, 0] - s[:, 1]) / cfg["temperature"] - cfg["gamma_beta_ratio"])
        assert (hz[marks["kink"]] == 0).all(), "kink rows must sit exactly on the kink"
        assert (np.abs(hz[~marks["kink"]]) > 1e-3).all(), "a random row lies within 1e-3 of the hinge kink: change the seed"
    return q, p, rc, rr, marks


def rankpo_rows_f64(scores, rc, rr, cfg):
    """Per-row rankpo loss, SFT loss and the bound's magnitude M_b in float64 on given [B, 2] scores."""
    s = np.asarray(scores, dtype=np.float64)
    c, r = s[:, 0], s[:, 1]
    B = len(c)
    rc = np.zeros(B) if rc is None else np.asarray(rc, dtype=np.float64)
    rr = np.zeros(B) if rr is None else np.asarray(rr, dtype=np.float64)
    beta, T, gamma = cfg["beta"], cfg["temperature"], cfg["gamma_beta_ratio"]
    losses = R.rankpo_loss(c, r, rc, rr, beta=beta, temperature=T, gamma_beta_ratio=gamma, label_smoothing=cfg["label_smoothing"],
                           loss_type=cfg["loss_type"], reference_free=cfg["reference_free"])
    if cfg["rankpo_weight"] <= 0:
        losses = np.zeros(B)
    ts = s / T
    sft = R._logsumexp(ts) - ts[:, 0]
    if cfg["reference_free"]:
        rc, rr = 0 * rc, 0 * rr
    M = (beta / T) * (np.abs(c) + np.abs(r) + np.abs(rc) + np.abs(rr)) + beta * abs(gamma) + (np.abs(c) + np.abs(r)) / T + 1
    z = beta * ((c - r - (rc - rr)) / T - gamma)
    logpart = np.log1p(np.exp(-np.abs(z))) + np.log1p(np.exp(-np.abs(ts[:, 0] - ts[:, 1])))
    bound = RANKPO_ROUNDINGS * 2.0 ** -24 * M + REL_LOG * logpart + ABS_LOG
    return losses, sft, bound


def rankpo_loss_bound(losses, sft, bound, cfg):
    """|loss - loss64| on the returned scores: weighted mean of the row bounds + the float32 reduction (block_sum: 6 + 3 levels,
    2 serial trips at B = 300, * 1 / B, the two weights and their sum: REDUCE_ROUNDINGS covers them)."""
    w, ws = max(cfg["rankpo_weight"], 0.0), max(cfg["sft_weight"], 0.0)
    mag = w * np.abs(losses).mean() + ws * np.abs(sft).mean()
    return float((w + ws) * bound.mean() + REDUCE_ROUNDINGS * 2.0 ** -24 * mag)


def rankpo_finalize_f32(scores, rc, rr, cfg):
    """rankpo_finalize_kernel's formulas (csrc/rankpo.hip 42-49, 61-117) in numpy float32: per-row losses, loss."""
    f = np.float32
    s = np.asarray(scores, dtype=f)
    c, r = s[:, 0], s[:, 1]
    B = len(c)
    rc = np.zeros(B, f) if rc is None else np.asarray(rc, dtype=f)
    rr = np.zeros(B, f) if rr is None else np.asarray(rr, dtype=f)
    beta, T, gamma, ls = f(cfg["beta"]), f(cfg["temperature"]), f(cfg["gamma_beta_ratio"]), f(cfg["label_smoothing"])

    def logsig(x):
        return (np.minimum(x, f(0)) - np.log1p(np.exp(-np.abs(x)))).astype(f)

    lb = np.zeros(B, f)
    loss = f(0)
    if cfg["rankpo_weight"] > 0:
        adv = (c - r).astype(f)
        if not cfg["reference_free"]:
            adv = (adv - (rc - rr)).astype(f)
        bz = (beta * ((adv / T).astype(f) - gamma)).astype(f)
        if cfg["loss_type"] == "sigmoid":
            lb = (-logsig(bz) * (f(1) - ls) - logsig(-bz) * ls).astype(f)
        else:
            lb = np.maximum(f(1) - bz, f(0)).astype(f)
        loss = f(loss + f(cfg["rankpo_weight"]) * f(lb.sum(dtype=f) * f(1.0 / B)))
    if cfg["sft_weight"] > 0:
        t0, t1 = (c / T).astype(f), (r / T).astype(f)
        m = np.maximum(t0, t1)
        lse = (m + np.log(np.exp(t0 - m) + np.exp(t1 - m))).astype(f)
        loss = f(loss + f(cfg["sft_weight"]) * f((lse - t0).astype(f).sum(dtype=f) * f(1.0 / B)))
    return lb.astype(np.float64), float(loss)
