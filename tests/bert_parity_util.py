"""Shared by tests/test_bert_parity_host.py (CPU) and tests/test_gpu_bert_parity.py (GPU): float64 parity of every kernel of
rankpo_amd/csrc/bert_ops.hip on 16-bit storage, at every row width and on hard inputs.  Importing it needs no GPU.

Four parts.

(1) Mirrors of the dispatch, restated from the C entries: `row_vectors`, `layernorm_bwd_blocks`, `gelu_grid`.
(2) Case tables: ROW_WIDTHS (every NV = 1, 2, 4, 8 vectors per lane with a full and a partially filled last vector, and the
    smallest row d = 8), LN_BWD_ROWS, ATTN_LENS, the cross case, GELU_SHAPES, DROP_WIDTHS.
(3) Deterministic input builders (CPU generator, values exact in the storage dtype, the same tensors on the CPU and the GPU side).
(4) float64 references, float32 restatements of the kernels' own formulas with their rounding points (host test only), and the
    error rules as functions.

LayerNorm row regimes (`ln_rows`):
  random    2 * randn.
  offset    a common per-row value of +-64 plus unit noise: mean >> std, where a one-pass variance E[x^2] - mean^2 loses its digits.
  outlier   randn with two columns per row at +-60 x the LARGEST of the row's other entries, at columns that differ from row to
            row (XLM-R hidden states look like this).  "60 x the rest" has to mean the largest of the rest: against the typical
            entry two columns of 60 sigma carry 7200 / (7200 + d) of the variance, which is 64 % at d = 4096; against the largest
            they carry >= 90 % at every width of ROW_WIDTHS (checked on the host).
  tiny_var  a constant c (1, -1, 0.5, 2, -0.25 by row) plus k ulps of the storage dtype: k = +1 in a quarter of the columns, -1 in
            another quarter, 0 in the rest, shuffled.  Every entry is a multiple of one ulp q with d |c| / q < 2^24 and k sums to
            zero, so the f32 row sum d c and the mean c are exact.  With a free k the mean would be fl(sum / d), off by up to
            2^-24 |c| wherever d is no power of two; std is ~ 0.7 ulp(c), so that is 7e-5 std in fp16, five times the one-ulp
            rule's spacing 2^-16 at its floor: no f32 LayerNorm, torch's included, meets that rule there (tried on the host).
  const     exactly constant rows, using only the values 0, 1, -2.  Their f32 row sum d * c is exact, the f32 mean is exactly c,
            x - mean is exactly 0 and the forward's y equals beta bit for bit (asserted as such).  Any other constant would make
            x - mean pure rounding noise of the mean, which eps = 1e-12 amplifies by 1e6, in torch's kernels as well.
In the `a + b` form the non-degenerate regimes add b = 0.25 * randn (the sum rounds), the degenerate ones (tiny_var, const) split the
row exactly, a = b = x / 2, so that the stored sum is the regime's row bit for bit.

Attention regimes (`attn_case`; scale = 1 / sqrt(hd) throughout):
  random          randn.
  saturated       q, k = sqrt(60) * randn: scaled scores ~ N(0, 60^2), as tests/test_gpu_bert_native.py builds them.  The winner's
                  lead over the runner-up is random (mean ~ 20 at 100 keys), so only a fraction of the rows reaches
                  max P >= 1 - 1e-6 (the host test asserts at least a quarter of each case's rows with >= 2 keys do).
  identical_keys  every key row equals the first one: P is uniform, as the forward test builds it.
  spike           one key per query wins by a fixed gap B^2 * scale ~ 32 over keys that differ by < 4: max P >= 1 - 1e-6 in EVERY
                  row.  The winner's position cycles over 0, 31, 32 and lk - 1 (clipped to the sequence) with the query index.
  offset          q and k share component 0: Cq in every query, Ck = 4 in every key, Cq Ck scale >= 100 (Cq = 144 at hd 32, 203 at
                  hd 64); the other components are 0.5 * randn (q) and randn (k): every scaled score of a row is >= 100 while the
                  row's spread stays < 10, so lse is large and the softmax ordinary.  The large factor sits in q because
                  dq[0] = scale Ck sum_k dS_k is Ck times a sum that cancels exactly (sum_k dS_k = 0): with Ck = Cq = 24 that one
                  component's rounding noise alone reaches the whole bound of a correct kernel (tried on the host).
GELU inputs (`gelu_case`): 3 * randn with both tails planted (-40 .. 40), +-0 and |u| = 200; in fp16 every fifth dh is scaled into
the subnormals.  No infinities or NaNs anywhere: out of scope.

Error rules.  U = the storage unit roundoff 2^-(explicit mantissa bits + 1).
  `one_ulp_ratio`  |got - ref| in ulps of the storage dtype at max(|ref|, floor): the forward rule of tests/test_gpu_bert_native.py
                   (`_within_one_ulp`) with its floors 2^-6 (LayerNorm) and 2^-10 (GELU).
  `rule_bound`     ||got - ref|| <= 1.5 ||control - ref|| + 2 U ||ref|| (+ extra), norms per row / block / tensor: the project's rule
                   (error <= 1.5 x the error of the stock PyTorch op in the same storage dtype + 2 U), multiplied through by the
                   unit's own reference norm so that an exactly zero reference needs no division.
  `lse_bound`      the f32 bound on the forward's lse against the float64 lse of the stored inputs, derived from the kernel's
                   arithmetic.  u32 = 2^-24, A_j = sum_i |q_i k_ij|, S_abs = |scale| max_j A_j, lk keys, hd head dims:
                     - products of two 16-bit values are exact in f32; the MFMA adds hd of them with at most hd roundings of
                       partial sums <= A_j; the constant scale * log2(e) carries two roundings and the multiply by it one:
                       |d s_j| <= (hd + 3) u32 S_abs in natural-log units.  lse is 1-Lipschitz in max_j |d s_j|.
                     - p_j = exp2(x_j - m): the subtraction's rounding moves p_j by ln 2 |x_j - m| u32 relatively, and the p-weighted
                       mean of ln 2 |x_j - m| is at most ln lk; v_exp_f32 is good to 1 ulp = 2 u32; the online sum of lk positive
                       terms with one fma per 32-key step adds (lk + 2 ceil(lk / 32)) u32: |d ln L| <= (2 lk + ln lk + 4) u32.
                     - log2f: 2 u32 |log2 L| <= 2 u32 ln lk / ln 2; the sum m + log2 L, the constant ln 2 and the multiply: 3 u32 |lse|.
                   Rounded up: |lse - lse64| <= u32 ((hd + 4) S_abs + 3 lk + 8 + 4 |lse64|).  The host test confirms that a float32
                   evaluation of the kernel's formula stays inside it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import hidden_dropout_util as HU

DTYPES = [torch.bfloat16, torch.float16]
TAG = {torch.bfloat16: "bf16", torch.float16: "f16"}
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
MANT = {torch.bfloat16: 7, torch.float16: 10}        # explicit mantissa bits
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
LN_FLOOR = 2.0 ** -6          # tests/test_gpu_bert_native.py: LayerNorm outputs are O(1)
GELU_FLOOR = 2.0 ** -10       # ... and its GELU floor
U32 = 2.0 ** -24
LOG2E = 1.4426950408889634

# ------------------------------------------------------------------------------------------------
# (1) mirrors of the dispatch
# ------------------------------------------------------------------------------------------------
ROW_LANES, ROW_VEC = 64, 8             # one wave per row, 8 elements per 16-byte vector
LN_BWD_WAVES, LN_BWD_MAX_BLOCKS = 4, 1024
GELU_THREADS, GELU_MAX_BLOCKS = 256, 8192


def row_vectors(d):
    """NV of the row kernels: ceil(d / 512) rounded up to 1, 2, 4 or 8; 0 = too wide (d > 4096)."""
    nv = -(-d // (ROW_LANES * ROW_VEC))
    return 1 if nv <= 1 else 2 if nv <= 2 else 4 if nv <= 4 else 8 if nv <= 8 else 0


def last_vector(d):
    """'full' when every lane of the wave holds NV vectors (d == 512 NV), else 'partial' (the `c0 < d` guard cuts lanes off)."""
    return "full" if d == ROW_LANES * ROW_VEC * row_vectors(d) else "partial"


def layernorm_bwd_blocks(rows):
    return min(-(-max(rows, 1) // LN_BWD_WAVES), LN_BWD_MAX_BLOCKS)


rpo_layernorm_bwd_blocks = layernorm_bwd_blocks       # the C entry's name


def layernorm_bwd_row_class(rows):
    """How the rows fall on the waves of the (capped) grid."""
    waves = layernorm_bwd_blocks(rows) * LN_BWD_WAVES
    if rows < LN_BWD_WAVES:
        return "fewer rows than waves"
    if rows == LN_BWD_WAVES * LN_BWD_MAX_BLOCKS:
        return "one row per wave at the cap"
    if rows == LN_BWD_WAVES * LN_BWD_MAX_BLOCKS + 1:
        return "two rows for one wave"
    return "one row per wave" if rows <= waves else "several rows per wave"


def attn_instance(hd, p):
    """(HD, DROP) of the attention kernel templates the C entries launch: DROP is `thr > 0`, thr = round(p * 65536); None where the
    entries answer UNSUPPORTED."""
    return (hd, HU.threshold(p) > 0) if hd in (32, 64) and 0.0 <= p < 1.0 else None


def gelu_grid(rows, cols):
    return min(-(-(rows * cols // ROW_VEC) // GELU_THREADS), GELU_MAX_BLOCKS)


def gelu_passes(rows, cols):
    """Trips of the longest thread through the grid-stride loop."""
    return -(-(rows * cols // ROW_VEC) // (gelu_grid(rows, cols) * GELU_THREADS))


# ------------------------------------------------------------------------------------------------
# (2) case tables
# ------------------------------------------------------------------------------------------------
ROW_WIDTHS = [8, 136, 512, 520, 1024, 1032, 2048, 2056, 4096]
LN_ROWS = 5
LN_BWD_ROWS = [1, 2, 3, 4, 5, 4096, 4097]
LN_BWD_SMALL_ROWS = [1, 2, 3, 4, 5]           # also run at d = 1032; the large counts at d = 128 only
LN_BWD_WIDTH, LN_BWD_WIDE = 128, 1032
DROP_WIDTHS = [2056, 4096, 1032, 2048, 136, 512, 520, 1024]     # NV 8, NV 4 (never run before), and NV 1 and 2, partial and full
DROP_PS = [0.1, 0.5]
ATTN_LENS = [1, 2, 31, 32, 33, 63, 64, 65, 100]
CROSS_LENS_Q, CROSS_LENS_K = [5, 33, 64, 1], [40, 7, 65, 100]
ATTN_HEADS = [(32, 4), (64, 3)]               # (head dim, heads)
ATTN_PS = [0.0, 0.1]
ATTN_SEED = 0x1234567887654321
GELU_SHAPES = [(1, 8), (37, 520), (5470, 3072)]
LN_REGIMES = ["random", "offset", "outlier", "tiny_var", "const"]
LN_DEGENERATE = ("tiny_var", "const")
ATTN_REGIMES = ["random", "saturated", "identical_keys", "spike", "offset"]
ATTN_CANCELLING = ("saturated", "spike")      # the regimes in which dq / dk get 2 U ||abs||
CONST_VALUES = (0.0, 1.0, -2.0)
TINY_CENTRES = (1.0, -1.0, 0.5, 2.0, -0.25)
OFFSET_CQ, OFFSET_CK = {32: 144.0, 64: 203.0}, 4.0
ROW_KERNEL_WIDTHS = {                         # the widths at which the GPU tests run each of the six row kernels
    "add_layernorm_kernel<DROP false>": ROW_WIDTHS, "bert_embed_ln_kernel<DROP false>": ROW_WIDTHS,
    "layernorm_bwd_kernel<DROP false>": ROW_WIDTHS,
    "add_layernorm_kernel<DROP true>": DROP_WIDTHS,
    "bert_embed_ln_kernel<DROP true>": DROP_WIDTHS,
    "layernorm_bwd_kernel<DROP true>": DROP_WIDTHS,
}


def attn_shapes():
    """(label, lens_q, lens_k): self-attention, the CLS shape (one query per sequence) and the cross case."""
    return [("self", ATTN_LENS, ATTN_LENS), ("cls", [1] * len(ATTN_LENS), ATTN_LENS), ("cross", CROSS_LENS_Q, CROSS_LENS_K)]


# ------------------------------------------------------------------------------------------------
# (3) input builders
# ------------------------------------------------------------------------------------------------
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def ulp_at(x, dtype):
    """Spacing of `dtype` at |x| (float64 tensor)."""
    a = x.abs().clamp_min(MIN_NORMAL[dtype])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


def ln_rows(regime, rows, d, dtype, seed=0):
    """[rows, d] in the storage dtype (module docstring)."""
    gen = _gen(LN_REGIMES.index(regime), rows, d, MANT[dtype], seed)
    r = torch.arange(rows)
    if regime == "random":
        x = 2 * _randn(gen, rows, d)
    elif regime == "offset":
        x = 64.0 * (1 - 2 * (r % 2)).float()[:, None] + _randn(gen, rows, d)
    elif regime == "outlier":
        x = _randn(gen, rows, d)
        c1 = (7 * r + 3) % d
        c2 = (c1 + 1 + (3 * r) % (d - 1)) % d
        x[r, c1] = x[r, c2] = 0.0
        m = x.abs().amax(-1)
        x[r, c1], x[r, c2] = 60 * m, -60 * m
    elif regime == "tiny_var":
        c = torch.tensor(TINY_CENTRES)[r % len(TINY_CENTRES)][:, None]
        k = torch.cat([torch.ones(d // 4), -torch.ones(d // 4), torch.zeros(d - 2 * (d // 4))])      # sums to zero
        k = torch.stack([k[torch.randperm(d, generator=gen)] for _ in range(rows)])
        x = c + k * ulp_at(c.double(), dtype).float()
    elif regime == "const":
        x = torch.tensor(CONST_VALUES)[r % len(CONST_VALUES)][:, None].expand(rows, d).contiguous()
    else:
        raise ValueError(regime)
    out = x.to(dtype)
    if regime in LN_DEGENERATE:
        assert torch.equal(out.float(), x)                   # built on the storage grid
    return out


def ln_case(regime, rows, d, dtype, seed=0):
    """x: the regime's rows (the input of the b = None form); a, b with round(a + b) = s for the `a + b` form; gamma, beta, dy."""
    gen = _gen(77, LN_REGIMES.index(regime), rows, d, MANT[dtype], seed)
    x = ln_rows(regime, rows, d, dtype, seed)
    if regime in LN_DEGENERATE:
        a = b = (x.float() * 0.5).to(dtype)
        assert torch.equal(a.float() * 2, x.float())
    else:
        a, b = x, (0.25 * _randn(gen, rows, d)).to(dtype)
    s = (a.float() + b.float()).to(dtype)                    # the kernel's (and torch's) rounded sum
    return {"x": x, "a": a, "b": b.clone(), "s": s, "gamma": (1 + 0.1 * _randn(gen, d)).to(dtype),
            "beta": (0.1 * _randn(gen, d)).to(dtype), "dy": _randn(gen, rows, d).to(dtype)}


EMBED_V, EMBED_P, EMBED_TT, EMBED_PAD = 7, 7, 2, 2
EMBED_IDS = [0, EMBED_V - 1, 3, 3, 3, 3, 3, 3, EMBED_PAD, EMBED_PAD, 1, 0]      # first and last row, heavy repeats, the padding row
EMBED_POS = [0, EMBED_P - 1, 1, 1, 1, 2, 2, 3, 4, 5, 0, EMBED_P - 1]
EMBED_TTS = [0, 1, 1, 1, 0, 0, 1, 1, 0, 1, 0, 1]


def embed_case(regime, d, dtype, seed=0):
    """Tables and indices whose token sums (word + type) + pos are rows of the regime: the word table holds the regime's rows; the
    other two add 0.25 * randn, or, for the degenerate regimes, word = pos table = x / 2 with pos = ids and a zero type table."""
    gen = _gen(99, LN_REGIMES.index(regime), d, MANT[dtype], seed)
    x = ln_rows(regime, EMBED_V, d, dtype, seed + 1)
    ids = torch.tensor(EMBED_IDS, dtype=torch.int32)
    if regime in LN_DEGENERATE:
        word = pos_t = (x.float() * 0.5).to(dtype)
        type_t = torch.zeros(EMBED_TT, d, dtype=dtype)
        pos = ids.clone()
    else:
        word, pos_t = x, (0.25 * _randn(gen, EMBED_P, d)).to(dtype)
        type_t = (0.25 * _randn(gen, EMBED_TT, d)).to(dtype)
        pos = torch.tensor(EMBED_POS, dtype=torch.int32)
    return {"word": word, "pos_t": pos_t.clone(), "type_t": type_t, "ids": ids, "pos": pos,
            "tts": torch.tensor(EMBED_TTS, dtype=torch.int32), "gamma": (1 + 0.1 * _randn(gen, d)).to(dtype),
            "beta": (0.1 * _randn(gen, d)).to(dtype), "dy": _randn(gen, len(EMBED_IDS), d).to(dtype)}


def embed_sum(c, with_types, dtype):
    """The stored sum (word + type) + pos of every token, rounded where the kernel rounds."""
    t_rows = c["type_t"][c["tts"].long()] if with_types else c["type_t"][0].expand(len(c["ids"]), -1)
    s = (c["word"][c["ids"].long()].float() + t_rows.float()).to(dtype)
    return (s.float() + c["pos_t"][c["pos"].long()].float()).to(dtype)


def spike_positions(lk):
    out = []
    for p in (0, 31, 32, lk - 1):
        p = min(p, lk - 1)
        if p not in out:
            out.append(p)
    return out


def spike_winner(n, i, lk):
    """The winning key of query i of sequence n."""
    w = spike_positions(lk)
    return w[(i + n) % len(w)]


def attn_case(regime, lens_q, lens_k, nh, hd, dtype, seed=0):
    """q [Tq, nh, hd], k / v [Tk, nh, hd], do [Tq, nh * hd] in the storage dtype (module docstring)."""
    gen = _gen(55, ATTN_REGIMES.index(regime), sum(lens_q), sum(lens_k), nh, hd, MANT[dtype], seed)
    Tq, Tk = sum(lens_q), sum(lens_k)
    q, k, v = _randn(gen, Tq, nh, hd), _randn(gen, Tk, nh, hd), _randn(gen, Tk, nh, hd)
    do = _randn(gen, Tq, nh * hd)
    cu_q, cu_k = np.concatenate([[0], np.cumsum(lens_q)]), np.concatenate([[0], np.cumsum(lens_k)])
    if regime == "saturated":
        q, k = q * math.sqrt(60.0), k * math.sqrt(60.0)
    elif regime == "identical_keys":
        k = k[:1].expand(Tk, nh, hd).contiguous()
    elif regime == "spike":
        B = float(torch.tensor(math.sqrt(32.0 * math.sqrt(hd))).to(dtype))
        q, k = 0.5 * q, 0.5 * k
        q[:, :, :4], k[:, :, :4] = 0.0, 0.0
        for n in range(len(lens_q)):
            w = spike_positions(lens_k[n])
            for t, pos in enumerate(w):
                k[cu_k[n] + pos, :, t] = B
            for i in range(lens_q[n]):
                q[cu_q[n] + i, :, (i + n) % len(w)] = B
    elif regime == "offset":
        q = 0.5 * q
        q[:, :, 0], k[:, :, 0] = OFFSET_CQ[hd], OFFSET_CK
    elif regime != "random":
        raise ValueError(regime)
    return q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype)


def attn_keep_host(seed, q_row0, k_row0, lq, lk, nh, p):
    """The attention dropout's keep mask uint8 [nh, lq, lk] on the host: the hidden dropout's function (hidden_dropout_util) with
    (head, packed query row, packed key row) in the places of (site, row, column), as bert_ops.hip states."""
    return torch.from_numpy(np.stack([HU.hidden_keep(seed, h, q_row0, lq, k_row0 + lk, p)[:, k_row0:] for h in range(nh)]))


def gelu_case(rows, cols, dtype, seed=0):
    """u, dh [rows, cols] in the storage dtype."""
    gen = _gen(33, rows, cols, MANT[dtype], seed)
    u, dh = 3 * _randn(gen, rows, cols), _randn(gen, rows, cols)
    flat = u.view(-1)
    if flat.numel() >= 64:
        plant = torch.cat([torch.linspace(-40, 40, 33), torch.tensor([0.0, -0.0, 200.0, -200.0, 9.0, -9.0])])
    else:
        plant = torch.tensor([-40.0, -9.0, -0.0, 0.0, 9.0, 40.0, 200.0, -200.0])
    flat[:plant.numel()] = plant
    if dtype == torch.float16:
        dh.view(-1)[1::5] *= 2.0 ** -17                      # fp16 subnormals (below 2^-14)
    return u.to(dtype), dh.to(dtype)


# ------------------------------------------------------------------------------------------------
# (4) float64 references, float32 restatements, error rules
# ------------------------------------------------------------------------------------------------
def ln_stats64(s, eps):
    s = s.double()
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    return mu, var, 1.0 / torch.sqrt(var + eps)


def ln_fwd64(s, gamma, beta, eps):
    """float64 LayerNorm of the stored rounded sum s."""
    mu, _, rstd = ln_stats64(s, eps)
    return (s.double() - mu) * rstd * gamma.double() + beta.double()


def ln_bwd64(s, gamma, dy, eps):
    """float64 (ds, dgamma, dbeta) from the stored rounded sum s."""
    mu, _, rstd = ln_stats64(s, eps)
    xh = (s.double() - mu) * rstd
    g = dy.double() * gamma.double()
    ds = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return ds, (dy.double() * xh).sum(0), dy.double().sum(0)


def gelu64(u):
    u = u.double()
    return 0.5 * u * (1 + torch.erf(u / math.sqrt(2)))


def gelu_bwd64(u, dh):
    """(du, the size of what cancels |dh| (Phi + |u| phi)) in float64."""
    u, dh = u.double(), dh.double()
    cdf = 0.5 * torch.erfc(-u / math.sqrt(2))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
    return dh * (cdf + u * pdf), dh.abs() * (cdf + u.abs() * pdf)


def attn64(q, k, v, do, scale, keep, p):
    """float64 forward + backward of one sequence: q/do [lq, nh, hd], k/v [lk, nh, hd], keep [nh, lq, lk] or None.
    Returns (out, dq, dk, dv) and the norm-with-absolute-values versions of dq, dk, dv."""
    q, k, v, do = (t.double().transpose(0, 1) for t in (q, k, v, do))          # [nh, l, hd]
    P = torch.softmax(q @ k.transpose(1, 2) * scale, -1)
    kp = torch.ones_like(P) if keep is None else keep.double() / (1 - p)
    Pd = P * kp
    out = Pd @ v
    dPd = do @ v.transpose(1, 2)
    dP = dPd * kp
    delta = (do * out).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dq, dk, dv = dS @ k * scale, dS.transpose(1, 2) @ q * scale, Pd.transpose(1, 2) @ do
    delta_abs = (do.abs() * out.abs()).sum(-1, keepdim=True)    # sum |dO| |O| with the reference's own O
    dSa = P * (dP.abs() + delta_abs)
    absn = (dSa @ k.abs() * scale, dSa.transpose(1, 2) @ q.abs() * scale, Pd.transpose(1, 2) @ do.abs())
    # the channel of delta alone: an error e_q of delta moves dq[q] by scale e_q (P K)[q] and dk[k] by scale sum_q P[q, k] e_q Q[q]
    absd = (delta_abs * (P @ k).abs() * scale, (P * delta_abs).transpose(1, 2) @ q.abs() * scale, None)
    return (out, dq, dk, dv), absn, absd


def attn_scores64(q, k, scale):
    """(scaled scores [nh, lq, lk], lse [nh, lq], S_abs [nh, lq]) of one sequence in float64."""
    q, k = (t.double().transpose(0, 1) for t in (q, k))
    s = q @ k.transpose(1, 2) * scale
    s_abs = (q.abs() @ k.abs().transpose(1, 2)).amax(-1) * abs(scale)
    return s, torch.logsumexp(s, -1), s_abs


def lse_bound(s_abs, lse64, lk, hd):
    """Module docstring: u32 ((hd + 4) S_abs + 3 lk + 8 + 4 |lse64|)."""
    return U32 * ((hd + 4) * s_abs + 3 * lk + 8 + 4 * lse64.abs())


def one_ulp_ratio(got, ref, dtype, floor):
    """max |got - ref| / ulp(max(|ref|, floor)): <= 1 is the forward rule."""
    return float(((got.double() - ref).abs() / ulp_at(ref.abs().clamp_min(floor), dtype)).max())


def rule_bound(ctrl_err, ref_norm, dtype, extra=0.0):
    """1.5 x the control's error + 2 U of the unit's own reference norm (+ a derived extra term): all norms of ONE unit."""
    return 1.5 * ctrl_err + 2 * U[dtype] * ref_norm + extra


def block_norm(t):
    """Frobenius norm per head of a [nh, l, hd] tensor: one (sequence, head) block each."""
    return t.flatten(-2).norm(dim=-1)


def attn_control(q, k, v, do, scale, keep, p):
    """The controls of one sequence.  Without dropout: torch's SDPA.  Under dropout SDPA's own mask cannot be replayed, so, as
    tests/test_gpu_bert_train.py does, SDPA's undropped error is carried over to the dropped reference at the ratio of the two
    reference norms (`ref0` is the undropped float64 reference).  That stands in for a control only while a block keeps
    probabilities the storage format can hold.  `lost` [nh] marks the (sequence, head) blocks in which EVERY kept probability of
    EVERY query row lies below the smallest normal number of the storage dtype (fp16: 2^-14; bf16: never): the mask has dropped
    each row's dominant keys, what is left is stored with an absolute error of 2^-25 instead of a relative one of U (P and dS
    alike, which the kernels round to the storage dtype), and an undropped control says nothing about that.  For those blocks
    alone the control is `eager_replay_control`, the stock 16-bit attention with the mask, which meets the same underflow."""
    ctrl = {"sdpa": sdpa_control(q, k, v, do, scale), "ref0": None, "replay": None, "lost": None}
    if keep is not None:
        ctrl["ref0"] = attn64(q, k, v, do, scale, None, 0.0)[0]
        s64, lse64, _ = attn_scores64(q, k, scale)
        P = torch.exp(s64 - lse64[..., None])
        ctrl["lost"] = (P * keep.double()).amax((-2, -1)) < MIN_NORMAL[q.dtype]
        if bool(ctrl["lost"].any()):
            ctrl["replay"] = eager_replay_control(q, k, v, do, scale, keep, p)
    return ctrl


def attn_bounds(dtype, regime, lk, p, ref, ctrl, absn, absd):
    """The per-block bounds of (out, dq, dk, dv) of one sequence; ref [nh, l, hd], ctrl from `attn_control`.
    Where the undropped reference of a block is exactly zero (one key: dq = dk = 0) SDPA's error is carried over as it is.
    Extra terms, and nothing else:
      dq, dk  + 2 U ||abs|| in the `saturated` and `spike` regimes and for one-key sequences: there P is (nearly) one-hot, dP of
              the winner equals delta and dS = P (dP - delta) cancels (exactly so with one key: dq = dk = 0), while the kernels
              subtract two f32 sums of the same products taken in different orders, from a rounded O; ||abs|| is the same
              expression with absolute values, the size of what cancels, and 2 U its two 16-bit roundings (O and dS).
      dq, dk  + U ||abs_delta|| under dropout elsewhere: delta is taken from the stored O, rounded AFTER the mask and 1 / (1 - p).
      out, dv never; dq, dk in `random`, `identical_keys` and `offset` without dropout never."""
    bounds = []
    for i, name in enumerate(("out", "dq", "dk", "dv")):
        n = block_norm(ref[i])
        extra = torch.zeros_like(n)
        if name in ("dq", "dk"):
            if regime in ATTN_CANCELLING or lk == 1:
                extra = extra + 2 * U[dtype] * block_norm(absn[i - 1])
            elif p > 0:
                extra = extra + U[dtype] * block_norm(absd[i - 1])
        if ctrl["ref0"] is None:
            c_err = block_norm(ctrl["sdpa"][i].double() - ref[i])
        else:
            n0 = block_norm(ctrl["ref0"][i])
            carry = torch.where(n0 > 0, n / n0.clamp_min(1e-300), torch.ones_like(n))
            c_err = block_norm(ctrl["sdpa"][i].double() - ctrl["ref0"][i]) * carry
            if ctrl["replay"] is not None:
                c_err = torch.where(ctrl["lost"], block_norm(ctrl["replay"][i].double() - ref[i]), c_err)
        bounds.append(rule_bound(c_err, n, dtype, extra))
    return bounds


# ---- float32 restatements of the kernels' own formulas (host test: the bounds are reachable by a correct kernel) ----------------
def _r(x, dtype):
    return x.to(dtype).float()


def ln_fwd_restate(s, gamma, beta, eps, dtype):
    """Two-pass statistics in f32, one rounding."""
    x = s.float()
    d = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / d
    c = x - mean
    rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) / d + torch.tensor(eps, dtype=torch.float32))
    return (c * rstd * gamma.float() + beta.float()).to(dtype)


def ln_bwd_restate(s, gamma, dy, eps, dtype):
    """ds = rstd (g - mean g - xhat mean(g xhat)) in f32 from the two-pass statistics; dgamma / dbeta as f32 sums."""
    x, dyf = s.float(), dy.float()
    d = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / d
    c = x - mean
    rstd = torch.rsqrt((c * c).sum(-1, keepdim=True) / d + torch.tensor(eps, dtype=torch.float32))
    xh, g = c * rstd, dyf * gamma.float()
    ds = rstd * (g - g.sum(-1, keepdim=True) / d - xh * ((g * xh).sum(-1, keepdim=True) / d))
    return ds.to(dtype), (dyf * xh).sum(0), dyf.sum(0)


def gelu_restate(u, dtype):
    x = u.float()
    return (0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))).to(dtype)


def gelu_bwd_restate(u, dh, dtype):
    """dh (Phi + u phi), Phi = erfc(-u / sqrt 2) / 2, in f32."""
    x = u.float()
    cdf = 0.5 * torch.erfc(-x * 0.70710678118654752)
    pdf = 0.3989422804014327 * torch.exp(-0.5 * x * x)
    return (dh.float() * (x * pdf + cdf)).to(dtype)


def attn_restate(q, k, v, do, scale, dtype, keep, p):
    """One sequence in f32 with the kernels' rounding points: P and dS rounded to the storage dtype before the products, delta from
    the rounded O, lse = (m + log2 L) ln 2, P recomputed from lse in the backward.  -> (out, dq, dk, dv) [nh, l, hd], lse [nh, lq]."""
    qf, kf, vf, dof = (t.float().transpose(0, 1) for t in (q, k, v, do))
    sl = torch.tensor(scale * LOG2E, dtype=torch.float32)
    x = (qf @ kf.transpose(1, 2)) * sl
    m = x.amax(-1, keepdim=True)
    pe = torch.exp2(x - m)
    L = pe.sum(-1, keepdim=True)
    lse = (m + torch.log2(L)) * torch.tensor(math.log(2.0), dtype=torch.float32)
    kp = torch.ones_like(pe) if keep is None else keep.float()
    inv_keep = torch.tensor(1.0 / (1.0 - p), dtype=torch.float32) if keep is not None else torch.tensor(1.0)
    out = _r((_r(pe * kp, dtype) @ vf) * (inv_keep / L), dtype)
    pr = torch.exp2(x - lse * torch.tensor(LOG2E, dtype=torch.float32))
    dP = (dof @ vf.transpose(1, 2)) * kp * inv_keep
    delta = (dof * out).sum(-1, keepdim=True)
    dS = _r(pr * (dP - delta), dtype)
    sc = torch.tensor(scale, dtype=torch.float32)
    dq, dk = _r((dS @ kf) * sc, dtype), _r((dS.transpose(1, 2) @ qf) * sc, dtype)
    dv = _r((_r(pr * kp, dtype).transpose(1, 2) @ dof) * inv_keep, dtype)
    return (out, dq, dk, dv), lse[..., 0]


def sdpa_control(q, k, v, do, scale):
    """torch's own SDPA forward + backward in the storage dtype on the tensors' device, one sequence, no dropout: the control.
    -> (out, dq, dk, dv) [nh, l, hd]."""
    qs, ks, vs = (t.transpose(0, 1)[None].detach().clone().requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qs, ks, vs, scale=scale)
    o.backward(do.transpose(0, 1)[None])
    return (o[0].detach(),) + tuple(t.grad[0] for t in (qs, ks, vs))


def eager_replay_control(q, k, v, do, scale, keep, p):
    """The stock 16-bit attention WITH the dropout mask, one sequence, as an eager BERT layer runs it in the storage dtype: scores
    from a 16-bit matmul, softmax, keep / (1 - p), times V, and autograd's backward of that (P and dS come out rounded to the
    storage dtype).  Its 16-bit scores make it 10-100 times less exact than SDPA in the `offset` and `saturated` regimes, so it is
    the control of the `lost` blocks of `attn_control` only.  -> (out, dq, dk, dv) [nh, l, hd]."""
    qs, ks, vs = (t.transpose(0, 1).detach().clone().requires_grad_(True) for t in (q, k, v))
    P = torch.softmax((qs @ ks.transpose(1, 2)) * scale, -1)
    P = P * keep.to(q.dtype) / (1 - p)
    o = P @ vs
    o.backward(do.transpose(0, 1))
    return (o.detach(),) + tuple(t.grad for t in (qs, ks, vs))


def layernorm_control(s, gamma, beta, dy, eps):
    """torch's own LayerNorm forward + backward in the storage dtype on the tensors' device -> (y, ds, dgamma, dbeta)."""
    sc, gc, bc = (t.detach().clone().requires_grad_(True) for t in (s, gamma, beta))
    y = F.layer_norm(sc, (s.shape[-1],), gc, bc, eps)
    y.backward(dy)
    return y.detach(), sc.grad, gc.grad, bc.grad


def gelu_control(u, dh):
    """torch's own exact GELU backward in the storage dtype."""
    uc = u.detach().clone().requires_grad_(True)
    F.gelu(uc).backward(dh)
    return uc.grad
