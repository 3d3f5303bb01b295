"""Shared by tests/test_pool_parity_host.py (CPU) and tests/test_gpu_pool_parity.py (GPU): float64 parity of every path of
rankpo_amd/csrc/pool_normalize.hip in bf16, fp16 and f32 storage, on hard inputs.  Importing it needs no GPU.

Four parts.

(1) Mirrors of the dispatch, restated from the C++ (line numbers of pool_normalize.hip in the functions' docstrings): `fwd_kernel`
    (launch_fwd), `block_row_path` (the block kernel's per-row choice), `argmin_path`, `bwd_fill` (launch_bwd).
(2) Case tables: FWD_CASES and BWD_CASES, built per storage dtype from V = elements per 16 bytes.
(3) Deterministic builders, seeded per case (CPU generator; the same tensors on the CPU and the GPU side).
(4) float64 references, float32 restatements with the kernels' rounding points (host test only), the error rules.

Forward layout.  A forward case is ONE flat buffer `h` and the strides (sn, sl) the C entry takes: row l of sample n starts at element
h_off + n sn + l sl.  With sn = sl = ld the samples are overlapping windows of a [N + L, ld] matrix (sample n's row l is matrix row
n + l), which is legal because h is only read, and keeps N >= 512, L = 1024, d = 4096 at a few MB.  Two samples whose pooled rows
fall on the same matrix row share that row.  Everything that is not a pooled row -- other rows, padding columns, the lead-in --
holds SENTINEL, a large finite value: a wrong index gives a gross error, and the GPU test asserts that the whole buffer is unchanged.

Pooled-row regimes (`pool_rows`; the regime of a row is decided by the rank of its offset, so every launch mixes them):
  random     randn.
  offset     +-64 per row plus unit noise: mean >> spread.
  outlier    randn with one element (an even column that moves with the row) at 2^12 x the largest of the others.
  large      fp16: +-65504 in every 8th column, 2^-6 randn elsewhere.  bf16 / f32: 2^55 randn in every other column, randn elsewhere;
             ss ~ 2^110 d / 2 < 2^123 stays finite in f32 (asserted on the host, for the sum of squares in f32).
  zero       all +0.
  below_eps  norm <= eps / 4: (2 rand - 1) 2^-42 / sqrt(d) per element, so norm <= 2^-42 = 2.3e-13 (eps = 1e-12).  bf16 and f32 only:
             fp16's smallest non-zero value is 6e-8, so the fp16 table holds `zero` in this slot (REGIMES[float16]).
  above_eps  norm >= 4 eps.  bf16 / f32: +-2^-38 (1 + |randn|) per element, norm >= 2^-38 sqrt(d) >= 2^-37 = 7.3e-12 for d >= 4.
             fp16: +-2^-14 (1 + j / 4), the smallest normal numbers (norm ~ 1e-4; subnormal rows would put dx = g / norm beyond
             fp16's range in the backward).
  The factor 4 on both sides of eps keeps the kernel's `nrm >= eps` switch away from rounding.
Gradients (`pool_grads`): `random` randn; `parallel` g = c x rounded to storage with c = 1 / rms(x); `orthogonal` randn on the odd
columns while x is zeroed there, so every product g_i x_i is exactly 0.  In fp16 `large` every g is scaled by 2^12 (G_SCALE): the
exact dx ~ g / (65504 sqrt(d / 8)) of a unit g is an fp16 subnormal, where storage rounding is absolute (2^-25) and no relative rule
can hold, for any kernel.

Mask rows (`mask_row`): ones, zeros, leftpad, last_zero, holes, fz<p> (ones, the first zero at p, then zeros or a 0/1 mix) for p in
FIRST_ZEROS where p < L, and three 64-bit kinds with the minimum planted at a seam position >= 1:
  wide_a  values in {2^40, 2^40 + 1}, element 0 = 2^40 + 1: a compare through f32 (or of the high halves alone) ties all of them and
          answers 0.  A truncation to the low 32 bits keeps the order of these two values, so this kind cannot tell it apart;
  wide_c  values in {2^40 + 1, 2^41}, element 0 = 2^41: the low half of 2^41 is 0, a truncating compare or shuffle answers 0;
  wide_b  values in {-2^40, 0, 1}, element 0 = 0: the low half of -2^40 is 0 (a truncating compare ties and answers 0), and an
          unsigned compare takes -2^40 for the largest.
No row is made of INT64_MAX (the kernels' own identity element).

Error rules.  U = unit roundoff of the storage dtype (2^-8 bf16, 2^-11 fp16, 2^-24 f32), u32 = 2^-24.
  index            exact (oracle.scoring_ref.last_token_index on the int64 rows; 0 in CLS mode).
  normalize = 0    out is the pooled row bit for bit, norm_out is 0, the backward's dx is g bit for bit.
  norm_out         `norm_rel_bound(d)` = (ceil(d / 64) / 2 + 12) u32 relative to the float64 norm.  Derivation: ss is a sum of d
                   non-negative terms; every kernel path adds a term through a chain of at most ceil(d / 64) + 8 serial adds per
                   thread (the wave kernel: V NV <= d / 64 + V real terms per lane, zero padding adds exactly; the block kernel:
                   fewer), 6 shuffle adds and 4 adds over the waves' partials: <= ceil(d / 64) + 18 roundings of partial sums <= ss,
                   plus one for the product (f32 storage; products of 16-bit values are exact).  sqrt halves the relative error and
                   adds its own <= 1 ulp = 2 u32: (ceil(d / 64) + 19) / 2 + 2 <= ceil(d / 64) / 2 + 12.  A zero row gives exactly 0.
                   (f32 storage sums in f64 since these tests were written -- see tests/test_gpu_pool_parity.py -- and stays far
                   inside the same bound.)
  forward, 16-bit  `one_ulp_ratio`(got, ref, dtype, floor = MIN_NORMAL) <= 1 (bert_parity_util's rule).
  forward, f32     per row: max|got - ref| <= 1.5 max|control - ref| + 2 ulp(f32) at max|ref| (tests/test_gpu_bert_f32.py); the
                   control is the stock F.normalize in f32 on the gathered rows.
  backward         per row: ||got - ref|| <= `rule_bound`(||control - ref||, ||ref||, dtype, extra) = 1.5 ctrl + 2 U ||ref|| + extra;
                   the control is autograd through the stock F.normalize in the storage dtype on the gathered rows.  Where the
                   control itself is not finite (fp16: eps = 1e-12 rounds to 0 and 0 / 0 = NaN on a zero row), or the row's
                   norm lies beyond the storage dtype's range (fp16 `large`: the stock op's norm is inf and its dx is 0, a
                   100 % error), its term is dropped, which only tightens the bound.
                   extra = 0 for `random` and `orthogonal` g.  `parallel`: the exact dx = (g - y (y.g)) / n nearly cancels, while
                   the kernel uses the stored y^ = y + e, |e_i| <= U |y_i| so ||e|| <= U, its f32 norm n^ = n (1 + eta),
                   |eta| <= norm_rel_bound(d), and an f32 dot product p^ of g and y^ (chain: ceil(d / 256) serial adds + 6 + 4,
                   so |p^ - g.y^| <= (ceil(d / 256) + 11) u32 ||g||).  y^ (y^.g) - y (y.g) = e (y.g) + y (e.g) + O(U^2): norm
                   <= U |y.g| + U ||g||; the common factor (1 + eta) of y^ enters twice: 2 |eta| |y.g|.  With |y.g| <= ||g||:
                     extra = ||g|| / max(n, eps) x (2 U + 2 norm_rel_bound(d) + (ceil(d / 256) + 11) u32)
                   (`parallel_extra`); the issue's "about 2 U |y.g| / max(||x||, eps)" is its first term.
  clamped rows     (`zero`, `below_eps`; the kernel takes the `nrm < eps` branch): dx = g / eps, where eps is the f32 value the C
                   entry receives (EPS).  16-bit: within one ulp of the float64 quotient elementwise (two f32 roundings of 2^-24
                   and one to storage); where the quotient rounds to +-inf in fp16 the kernel must return that inf; a zero g
                   gives 0.  f32: the backward rule above.
  off-row          every element of dh outside the pooled rows is +0 by bit pattern; every guard keeps its fill.
"""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import scoring_ref as R

DTYPES = [torch.bfloat16, torch.float16, torch.float32]
TAG = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}
VEC = {torch.bfloat16: 8, torch.float16: 8, torch.float32: 4}            # Elem<T>::kVec: elements per 16 bytes
ESIZE = {torch.bfloat16: 2, torch.float16: 2, torch.float32: 4}
MANT = {torch.bfloat16: 7, torch.float16: 10, torch.float32: 23}
U = {t: 2.0 ** -(m + 1) for t, m in MANT.items()}
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14, torch.float32: 2.0 ** -126}
INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
U32 = 2.0 ** -24
EPS = float(np.float32(1e-12))          # ops.F_NORMALIZE_EPS as the C entry receives it (a float argument)
SENTINEL = -24576.0                     # exact in all three dtypes
POOL_LAST, POOL_CLS = 0, 1
RPO_ERR_INVALID_ARG, RPO_ERR_UNSUPPORTED = -1, -2                       # include/rankpo_hip.h

# ------------------------------------------------------------------------------------------------
# (1) mirrors of the dispatch
# ------------------------------------------------------------------------------------------------
POOL_THREADS, WAVE, FILL_PER_THREAD = 256, 64, 4                        # kPoolThreads, RPO_WAVE, kFillPerThread
BWD_MAX_N = 65535


def _cdiv(a, b):
    return -(-a // b)


def fwd_kernel(dtype, N, L, d, sn, sl, mode, h_off=0, out_off=0):
    """launch_fwd (pool_normalize.hip:299-323): 'wave/NV1' .. 'wave/NV8' or 'block'.  `h_off` / `out_off` are the element offsets
    of the two base pointers from a 16-byte aligned allocation."""
    V = VEC[dtype]
    vecs = _cdiv(d, V * WAVE)
    wave_ok = (d % V == 0 and vecs <= 8 and h_off % V == 0 and out_off % V == 0 and sn % V == 0 and sl % V == 0
               and mode == POOL_LAST and N >= 512 and L <= 1024)
    if not wave_ok:
        return "block"
    return "wave/NV%d" % (1 if vecs <= 1 else 2 if vecs <= 2 else 4 if vecs <= 4 else 8)


def block_row_path(dtype, d, row_off, out_row_off):
    """pool_normalize_fwd_kernel's choice for one sample (pool_normalize.hip:68-73, 101-133) from the element offsets of the
    pooled row (h_off + n sn + idx sl) and of the output row (out_off + n d)."""
    V = VEC[dtype]
    vec = d % V == 0 and row_off % V == 0 and out_row_off % V == 0
    return "block/scalar" if not vec else "block/onevec" if d <= POOL_THREADS * V else "block/vecloop"


def argmin_path(mode, L, mask_row_off):
    """block_argmin_first / wave_argmin_first (pool_normalize.hip:20, 160): 16-byte pieces when L is even and the row starts on
    16 bytes; `mask_row_off` = mask_off + n L in int64 elements."""
    if mode != POOL_LAST:
        return "none"
    return "vec16" if L % 2 == 0 and mask_row_off % 2 == 0 else "scalar"


def wave_scan_rounds(L):
    """Trips of wave_argmin_first's 16-byte scan (pool_normalize.hip:163): 4 x 64 pieces of two elements per trip."""
    return _cdiv(L // 2, 4 * WAVE)


def bwd_fill(dtype, L, d, has_dh, dh_off=0):
    """launch_bwd (pool_normalize.hip:329-336) -> ('vec' | 'scalar' | 'none', bx)."""
    V = VEC[dtype]
    if not has_dh:
        return "none", 1
    vec_ok = d % V == 0 and dh_off % V == 0 and L * (d // V) < 2 ** 31
    per_sample = L * (d // V) if vec_ok else L * d
    return ("vec" if vec_ok else "scalar"), max(1, _cdiv(per_sample, POOL_THREADS * (FILL_PER_THREAD if vec_ok else 8)))


# ------------------------------------------------------------------------------------------------
# (2) case tables
# ------------------------------------------------------------------------------------------------
L_TABLE = [1, 2, 7, 8, 255, 256, 257, 510, 512, 514, 1024, 1026]
FIRST_ZEROS = [0, 1, 63, 64, 255, 256, 257, 511, 512]
N_EDGE = [511, 512, 513, 514, 515]
REGIMES = {
    torch.bfloat16: ["random", "offset", "outlier", "large", "zero", "below_eps", "above_eps"],
    torch.float16: ["random", "offset", "outlier", "large", "zero", "zero", "above_eps"],      # fp16 holds no below_eps row
    torch.float32: ["random", "offset", "outlier", "large", "zero", "below_eps", "above_eps"],
}
CLAMPED = ("zero", "below_eps")
G_REGIMES = ["random", "parallel", "orthogonal"]
WIDE_A = (2 ** 40, 2 ** 40 + 1)
WIDE_B = (-2 ** 40, 0, 1)
WIDE_C = (2 ** 40 + 1, 2 ** 41)


def odd_width(dtype, big):
    """The d % V != 0 widths: 12 / 2050 in 16-bit storage (2050: nine trips of the scalar loop), 6 / 1026 in f32."""
    return {2: (12, 2050), 4: (6, 1026)}[ESIZE[dtype]][1 if big else 0]


def wave_widths(dtype):
    """V (one lane), then for NV = 1, 2, 4, 8 the partial width V 64 NV / 2 + V and the full width V 64 NV."""
    V = VEC[dtype]
    return [V, 33 * V, 64 * V, 65 * V, 128 * V, 129 * V, 256 * V, 257 * V, 512 * V]


def mask_kinds(L):
    if L < 2:
        return ["ones", "zeros"]
    return (["ones", "zeros", "leftpad", "last_zero", "holes"] + ["fz%d" % p for p in FIRST_ZEROS if p < L]
            + ["wide_a", "wide_b", "wide_c"])


def _fwd_case(name, dtype, N, L, d, ld=None, sn=None, sl=None, mode=POOL_LAST, normalize=1, mask_off=0, h_off=0, out_off=0,
              mask=True):
    ld = d + 2 * VEC[dtype] if ld is None else ld
    return {"name": "%s-%s" % (TAG[dtype], name), "dtype": dtype, "N": N, "L": L, "d": d, "sn": ld if sn is None else sn,
            "sl": ld if sl is None else sl, "mode": mode, "normalize": normalize, "mask_off": mask_off, "h_off": h_off,
            "out_off": out_off, "mask": mask}


def fwd_cases(dtype):
    V = VEC[dtype]
    c, W = [], wave_widths(dtype)
    f = lambda *a, **k: c.append(_fwd_case(*a, **k))       # noqa: E731
    # -- the wave kernel: every L <= 1024 of L_TABLE against the nine widths and N = 512 .. 515 (idle waves in the last block)
    for i, L in enumerate(L_TABLE[:-1]):
        d = W[i % len(W)]
        f("wave-L%d-d%d" % (L, d), dtype, N_EDGE[1 + i % 4], L, d, ld=d if i % 2 else None)
    for L, d in ((2, 64 * V), (512, 256 * V), (1024, 512 * V)):                # even L, mask base off by 8 bytes: the scalar scan
        f("wave-maskoff-L%d-d%d" % (L, d), dtype, 512, L, d, mask_off=1)
    for d in (33 * V, 128 * V, 129 * V, 512 * V):                              # NV 1, 2, 4, 8 without the normalisation
        f("wave-copy-d%d" % d, dtype, 513, 8, d, normalize=0)
    # -- the dispatch edges, each from the block kernel's side (the wave side: the cases above)
    f("edge-N511", dtype, 511, 8, 64 * V)
    f("edge-L1026", dtype, 512, 1026, 64 * V)
    f("edge-vecs9", dtype, 512, 8, 513 * V)
    f("edge-sn", dtype, 512, 8, 64 * V, ld=65 * V, sn=8 * 65 * V + V // 2)   # sn % V != 0: every other sample unaligned
    f("edge-sl", dtype, 512, 8, 64 * V, ld=64 * V + V // 2)                    # sl = d + V / 2: rows of odd n + idx unaligned
    f("edge-hbase", dtype, 512, 8, 64 * V, h_off=V // 2)
    f("edge-outbase", dtype, 512, 8, 64 * V, out_off=1)
    f("edge-oddd", dtype, 512, 8, odd_width(dtype, False))
    f("edge-cls", dtype, 512, 8, 64 * V, mode=POOL_CLS)
    # -- the block kernel at N = 1 .. 5: the smallest row, the one-vector / loop edge, vecs = 9, the widest wave width
    for N, L, d in ((1, 1, V), (2, 2, 256 * V), (3, 7, 257 * V), (4, 255, 513 * V), (5, 256, 512 * V)):
        f("block-N%d-L%d-d%d" % (N, L, d), dtype, N, L, d)
    # -- the block scan's seams with every mask kind in one launch, over the three row paths
    for L, d in ((257, 64 * V), (510, odd_width(dtype, False)), (512, 256 * V), (514, odd_width(dtype, True)), (1024, 33 * V),
                 (1026, 257 * V)):
        f("block-L%d-d%d" % (L, d), dtype, 40, L, d)
    for L, d in ((2, V), (256, 64 * V), (1026, 65 * V)):
        f("block-maskoff-L%d-d%d" % (L, d), dtype, 40, L, d, mask_off=1)
    f("block-mixed-align", dtype, 40, 8, 64 * V, ld=64 * V + V // 2)
    f("block-mixed-align-loop", dtype, 40, 8, 257 * V, ld=257 * V + V // 2)
    for d in (64 * V, 257 * V, odd_width(dtype, True)):
        f("block-copy-d%d" % d, dtype, 20, 8, d, normalize=0)
    # -- CLS: the production call [N, 1, d] with mask = NULL, a window with a mask the kernel must ignore, and the plain copy
    for d in (384, 768, 1024):
        f("cls-prod-d%d" % d, dtype, 700, 1, d, ld=d, mode=POOL_CLS, mask=False)
    f("cls-window", dtype, 40, 8, 33 * V, mode=POOL_CLS)
    f("cls-copy", dtype, 5, 3, 64 * V, mode=POOL_CLS, normalize=0, mask=False)
    f("cls-copy-odd", dtype, 5, 3, odd_width(dtype, False), mode=POOL_CLS, normalize=0, mask=False)
    return c


FWD_CASES = [c for t in DTYPES for c in fwd_cases(t)]


def _bwd_case(name, dtype, N, L, d, idx, g="random", rows="random", normalize=1, dh_off=0):
    assert len(idx) == N and all(0 <= i < L for i in idx)
    return {"name": "%s-%s" % (TAG[dtype], name), "dtype": dtype, "N": N, "L": L, "d": d, "idx": list(idx), "g": g, "rows": rows,
            "normalize": normalize, "dh_off": dh_off}


def bwd_cases(dtype):
    V = VEC[dtype]
    c = []
    f = lambda *a, **k: c.append(_bwd_case(*a, **k))       # noqa: E731
    # -- the vector fill at its block seams: 1023 / 1024 / 1025 chunks per sample (d = V: one chunk per row), pooled row first,
    #    last, and on either side of the seam
    for L in (1023, 1024, 1025):
        f("fill-chunks%d" % L, dtype, 4, L, V, [0, L - 1, 1022, min(1023, L - 1)])
    # 4 rows of 257 chunks: row 3 = chunks 771 .. 1027 straddles the seam at 1024; 241 rows of 17 chunks = 4097 chunks, five blocks
    f("fill-straddle", dtype, 4, 4, 257 * V, [0, 1, 2, 3])
    f("fill-chunks4097", dtype, 4, 241, 17 * V, [0, 240, 60, 120])          # row 60: chunks 1020 .. 1036; row 120: 2040 .. 2056
    # -- the scalar fill: d % V != 0 (small and wide), and an aligned width with dh off by one element
    f("sfill-odd", dtype, 3, 3, odd_width(dtype, False), [0, 2, 1])
    f("sfill-odd-wide", dtype, 3, 3, odd_width(dtype, True), [2, 0, 1])
    f("sfill-dhoff", dtype, 3, 5, 64 * V, [0, 4, 2], dh_off=1)
    # -- the largest grid the entry accepts.  Its rows are `axis` rows, +-2^k in one column: norm, y, the dot product and dx are
    #    exact in every dtype, so all 65535 results must equal the reference (among that many random rows of d = V some are
    #    nearly parallel to their g by chance, and the `random` rule, which has no cancellation term, is not owed to them)
    f("grid-N65535", dtype, BWD_MAX_N, 1, V, [0] * BWD_MAX_N, rows="axis")
    # -- every row regime against every gradient regime, one row each, at a narrow and a wide row (one and several trips of the
    #    dot-product loop) and at an odd width
    nreg = len(REGIMES[dtype])
    for g in G_REGIMES:
        for d in (33 * V, 513 * V, odd_width(dtype, True)):
            f("regimes-%s-d%d" % (g, d), dtype, nreg, 3, d, [i % 3 for i in range(nreg)], g=g, rows="all")
    # -- without the normalisation: dx = g bit for bit
    f("copy-vec", dtype, 3, 4, 33 * V, [0, 3, 1], rows="all3", normalize=0)
    f("copy-scalar", dtype, 3, 4, odd_width(dtype, False), [3, 0, 2], rows="all3", normalize=0)
    return c


BWD_CASES = [c for t in DTYPES for c in bwd_cases(t)]
G_SCALE = {(torch.float16, "large"): 2.0 ** 12}


# ------------------------------------------------------------------------------------------------
# (3) builders
# ------------------------------------------------------------------------------------------------
def _seed(name):
    return zlib.crc32(name.encode()) % (2 ** 31 - 1)


def _randn(gen, *shape):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def pool_rows(regime, rows, d, dtype, gen):
    """[rows, d] in the storage dtype (module docstring)."""
    r, col = torch.arange(rows)[:, None], torch.arange(d)[None, :]
    z = _randn(gen, rows, d)
    if regime == "random":
        x = z
    elif regime == "offset":
        x = 64.0 * (1 - 2 * (r % 2)).float() + z
    elif regime == "outlier":
        at = col == (6 * r + 2) % d
        m = z.masked_fill(at, 0.0).abs().amax(-1, keepdim=True).clamp_min(2.0 ** -4)
        x = torch.where(at, 4096.0 * m * torch.where(r % 2 == 0, 1.0, -1.0), z)
    elif regime == "large":
        if dtype == torch.float16:
            x = torch.where((col + r) % 8 == 0, 65504.0 * torch.where(z >= 0, 1.0, -1.0), z * 2.0 ** -6)
        else:
            x = torch.where((col + r) % 2 == 0, z * 2.0 ** 55, z)
    elif regime == "zero":
        x = torch.zeros(rows, d)
    elif regime == "below_eps":
        assert dtype != torch.float16
        u = 2 * torch.rand(rows, d, generator=gen, dtype=torch.float32) - 1
        x = u * (2.0 ** -42 / math.sqrt(d))
    elif regime == "above_eps":
        s = torch.where(z >= 0, 1.0, -1.0)
        x = s * 2.0 ** -14 * (1 + (col % 4) / 4.0) if dtype == torch.float16 else s * 2.0 ** -38 * (1 + z.abs())
    else:
        raise ValueError(regime)
    return x.to(dtype)


def mask_row(kind, L, n, rs):
    """One int64 mask row (module docstring); `n` picks the variant, `rs` a numpy RandomState."""
    m = np.ones(L, dtype=np.int64)
    seams = [p for p in FIRST_ZEROS if 1 <= p < L]
    plant = seams[n % len(seams)] if seams else 0
    if kind == "ones":
        pass
    elif kind == "zeros":
        m[:] = 0
    elif kind == "leftpad":
        m[:max(1, L // 2)] = 0
    elif kind == "last_zero":
        m[L - 1] = 0
    elif kind == "holes":
        m = rs.randint(0, 2, size=L).astype(np.int64)
    elif kind.startswith("fz"):
        p = int(kind[2:])
        m[p:] = rs.randint(0, 2, size=L - p) if n % 2 else 0
        m[p] = 0
    elif kind in ("wide_a", "wide_b", "wide_c"):
        lo, hi = {"wide_a": WIDE_A, "wide_c": WIDE_C, "wide_b": (WIDE_B[0], WIDE_B[1])}[kind]       # (minimum, decoy at element 0)
        others = {"wide_a": [hi], "wide_c": [hi], "wide_b": [0, 1]}[kind]
        m = np.array(others, dtype=np.int64)[rs.randint(0, len(others), size=L)]
        m[plant:] = np.where(rs.randint(0, 2, size=L - plant) == 1, lo, m[plant:])
        m[0], m[plant] = hi, lo
    else:
        raise ValueError(kind)
    return m


def build_masks(case):
    """-> (mask [N, L] int64 numpy or None, kinds per sample)."""
    N, L = case["N"], case["L"]
    if not case["mask"]:
        return None, ["none"] * N
    rs = np.random.RandomState(_seed(case["name"]) % (2 ** 31))
    kinds = mask_kinds(L)
    rot = _seed(case["name"]) % len(kinds)
    per = [kinds[(n + rot) % len(kinds)] for n in range(N)]
    return np.stack([mask_row(k, L, n, rs) for n, k in enumerate(per)]), per


def build_fwd(case):
    """The CPU tensors of a forward case: `h` flat (storage dtype, SENTINEL outside the pooled rows), `mask` flat int64 with
    `mask_off` leading elements (or None), `idx` [N] int64 (the reference index), `offs` [N] element offsets of the pooled rows,
    `x` [N, d] the pooled rows, `regime` / `kind` per sample."""
    dtype, N, L, d, sn, sl = (case[k] for k in ("dtype", "N", "L", "d", "sn", "sl"))
    gen = torch.Generator().manual_seed(_seed(case["name"]))
    mk, kinds = build_masks(case)
    idx = R.last_token_index(mk).astype(np.int64) if case["mode"] == POOL_LAST else np.zeros(N, dtype=np.int64)
    offs = case["h_off"] + np.arange(N, dtype=np.int64) * sn + idx * sl
    uniq, inv = np.unique(offs, return_inverse=True)
    assert len(uniq) == 1 or int(np.diff(uniq).min()) >= d, "pooled rows overlap"
    regs = REGIMES[dtype]
    rows = torch.empty(len(uniq), d, dtype=dtype)
    rot = _seed(case["name"]) % len(regs)
    slot = (np.arange(len(uniq)) + rot) % len(regs)
    for s, reg in enumerate(regs):
        sel = np.nonzero(slot == s)[0]
        if len(sel):
            rows[torch.from_numpy(sel)] = pool_rows(reg, len(sel), d, dtype, gen)
    size = case["h_off"] + (N - 1) * sn + (L - 1) * sl + d + 2 * VEC[dtype]
    h = torch.full((size,), SENTINEL, dtype=dtype)
    h[(torch.from_numpy(uniq)[:, None] + torch.arange(d)[None, :]).reshape(-1)] = rows.reshape(-1)
    mask = None
    if mk is not None:
        mask = torch.cat([torch.full((case["mask_off"],), 7, dtype=torch.int64), torch.from_numpy(mk).reshape(-1)])
    inv = torch.from_numpy(np.asarray(inv).reshape(-1))
    return {"h": h, "mask": mask, "mask2d": mk, "idx": torch.from_numpy(idx), "offs": torch.from_numpy(offs), "x": rows[inv],
            "regime": [regs[int(slot[j])] for j in inv.tolist()], "kind": kinds}


def fwd_paths(case, b):
    """What the launch runs: the kernel, and per sample the row path and the argmin path (through the mirrors)."""
    dtype, N, L, d = case["dtype"], case["N"], case["L"], case["d"]
    k = fwd_kernel(dtype, N, L, d, case["sn"], case["sl"], case["mode"], case["h_off"], case["out_off"])
    rows = [k if k != "block" else block_row_path(dtype, d, int(b["offs"][n]), case["out_off"] + n * d) for n in range(N)]
    arg = [argmin_path(case["mode"], L, case["mask_off"] + n * L) for n in range(N)]
    return k, rows, arg


def pool_grads(g_regime, x, regime, gen):
    """(x', g): g [N, d] in x's dtype and the rows x' the case runs on (`orthogonal` zeroes x on the odd columns)."""
    dtype = x.dtype
    N, d = x.shape
    scale = torch.tensor([G_SCALE.get((dtype, r), 1.0) for r in regime], dtype=torch.float64)[:, None]
    if g_regime == "random":
        g = _randn(gen, N, d).double()
    elif g_regime == "parallel":
        rms = x.double().pow(2).mean(-1, keepdim=True).sqrt()
        g = x.double() / torch.where(rms > 0, rms, torch.ones_like(rms))
    elif g_regime == "orthogonal":
        odd = (torch.arange(d) % 2 == 1)[None, :]
        x = torch.where(odd, torch.zeros_like(x), x)
        g = torch.where(odd, _randn(gen, N, d), torch.zeros(N, d)).double()
    else:
        raise ValueError(g_regime)
    return x, (g * scale).to(dtype)


def build_bwd(case):
    """The CPU tensors of a backward case: x [N, d] pooled rows, g [N, d], idx [N] int32, `regime` per row."""
    dtype, N, d = case["dtype"], case["N"], case["d"]
    gen = torch.Generator().manual_seed(_seed(case["name"]))
    regs = REGIMES[dtype]
    if case["rows"] == "random":
        regime = ["random"] * N
        x = pool_rows("random", N, d, dtype, gen)
    elif case["rows"] == "axis":
        regime = ["axis"] * N
        n = torch.arange(N)
        x = torch.zeros(N, d)
        x[n, n % d] = torch.exp2(((n % 7) - 3).float()) * (1 - 2 * (n % 2)).float()
        x = x.to(dtype)
    else:
        regime = regs[:N] if case["rows"] == "all" else ["offset", "large", "zero"]
        assert len(regime) == N
        x = torch.cat([pool_rows(r, 1, d, dtype, gen) for r in regime])
    x, g = pool_grads(case["g"], x, regime, gen)
    return {"x": x, "g": g, "idx": torch.tensor(case["idx"], dtype=torch.int32), "regime": regime}


# ------------------------------------------------------------------------------------------------
# (4) float64 references, float32 restatements, error rules
# ------------------------------------------------------------------------------------------------
def fwd64(x, normalize, eps=EPS):
    """(out, norm) in float64 from the stored rows; norm_out is 0 without the normalisation (the kernel never forms ss)."""
    x = x.double()
    n = x.pow(2).sum(-1).sqrt()
    if not normalize:
        return x, torch.zeros_like(n)
    return x / n.clamp_min(eps)[:, None], n


def bwd64(x, g, normalize, eps=EPS):
    """dx in float64: the derivative of x / max(||x||, eps) at the stored x, applied to g."""
    x, g = x.double(), g.double()
    if not normalize:
        return g
    n = x.pow(2).sum(-1, keepdim=True).sqrt()
    y = x / n.clamp_min(1e-300)
    through = (g - y * (y * g).sum(-1, keepdim=True)) / n.clamp_min(1e-300)
    return torch.where(n >= eps, through, g / eps)


def fwd_restate(x, normalize, dtype, eps=EPS):
    """The kernels' forward in f32 with their one rounding to storage -> (out in storage dtype, norm f32).  f32 storage sums the
    squares in f64, as the kernels do (pool_normalize.hip: SsAcc)."""
    xf = x.float()
    if not normalize:
        return xf.to(dtype), torch.zeros(x.shape[0])
    nrm = x.double().pow(2).sum(-1).sqrt().float() if dtype == torch.float32 else (xf * xf).sum(-1).sqrt()     # SsAcc<T>
    return (xf / torch.maximum(nrm, torch.tensor(eps, dtype=torch.float32))[:, None]).to(dtype), nrm


def bwd_restate(g, y, nrm, normalize, dtype, eps=EPS):
    """The kernel's backward in f32 from the STORED y and the f32 norm."""
    gf, yf = g.float(), y.float()
    if not normalize:
        return gf.to(dtype)
    e32 = torch.tensor(eps, dtype=torch.float32)
    through = (nrm >= e32)[:, None]
    proj = (gf * yf).sum(-1, keepdim=True)
    inv = (1.0 / torch.maximum(nrm, e32))[:, None]
    return torch.where(through, (gf - yf * proj) * inv, gf * inv).to(dtype)


def fwd_control_f32(x, normalize, eps=EPS):
    """The stock F.normalize in f32 on the gathered rows (on x's device)."""
    return F.normalize(x.float(), dim=-1, eps=eps) if normalize else x.float()


def bwd_control(x, g, normalize, eps=EPS):
    """Autograd through the stock F.normalize in the storage dtype on the gathered rows (on x's device)."""
    if not normalize:
        return g.clone()
    xs = x.detach().clone().requires_grad_(True)
    F.normalize(xs, dim=-1, eps=eps).backward(g)
    return xs.grad


def ulp_at(x, dtype):
    """Spacing of `dtype` at |x| (float64 tensor)."""
    a = x.abs().clamp_min(MIN_NORMAL[dtype])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


def one_ulp_ratio(got, ref, dtype, floor):
    """max |got - ref| / ulp(max(|ref|, floor)), as bert_parity_util.one_ulp_ratio; per row when `got` is 2-D."""
    r = (got.double() - ref).abs() / ulp_at(ref.abs().clamp_min(floor), dtype)
    return r.amax(-1)


def rule_bound(ctrl_err, ref_norm, dtype, extra=0.0):
    """bert_parity_util.rule_bound with f32 storage included; a non-finite control error is dropped (module docstring)."""
    ctrl_err = torch.where(torch.isfinite(ctrl_err), ctrl_err, torch.zeros_like(ctrl_err))
    return 1.5 * ctrl_err + 2 * U[dtype] * ref_norm + extra


def norm_rel_bound(d):
    return (_cdiv(d, 64) / 2 + 12) * U32


def parallel_extra(x, g, d, dtype, eps=EPS):
    """Module docstring: ||g|| / max(n, eps) x (2 U + 2 norm_rel_bound(d) + (ceil(d / 256) + 11) u32), per row."""
    n = x.double().pow(2).sum(-1).sqrt().clamp_min(eps)
    return g.double().norm(dim=-1) / n * (2 * U[dtype] + 2 * norm_rel_bound(d) + (_cdiv(d, 256) + 11) * U32)


def f32_floor(ref):
    """2 ulp of f32 at max|ref| of each row (tests/test_gpu_bert_f32.py `_floor`)."""
    a = ref.abs().amax(-1).clamp_min(2.0 ** -126)
    return 2 * torch.exp2(torch.floor(torch.log2(a)) - 23)


def bits(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def check_fwd(case, b, out, idx, norm, ctrl32=None):
    """All forward rules on CPU tensors: out [N, d] storage dtype, idx [N] int32, norm [N] f32; `ctrl32` the f32 control's output
    (f32 storage only).  Returns {regime: worst ratio}; raises AssertionError with the case's name."""
    dtype, d, name = case["dtype"], case["d"], case["name"]
    assert torch.equal(idx.long(), b["idx"]), (name, "index", idx.tolist()[:8], b["idx"].tolist()[:8])
    x = b["x"]
    ref, n64 = fwd64(x, case["normalize"])
    worst = {}
    if not case["normalize"]:
        assert torch.equal(bits(out), bits(x)), (name, "the copy is not bit-exact")
        assert bool((norm == 0).all()), (name, "norm_out without the normalisation")
        return {"copy": 0.0}
    assert torch.isfinite(out.float()).all() and torch.isfinite(norm).all(), name
    nerr = (norm.double() - n64).abs()
    nb = norm_rel_bound(d) * n64
    assert bool((nerr <= nb).all()) and bool((norm[n64 == 0] == 0).all()), (name, "norm_out", float((nerr / nb.clamp_min(1e-300)).max()))
    worst["norm"] = round(float((nerr / nb.clamp_min(1e-300)).max()), 3)
    if dtype == torch.float32:
        err = (out.double() - ref).abs().amax(-1)
        bound = 1.5 * (ctrl32.double() - ref).abs().amax(-1) + f32_floor(ref)
        ratio = err / bound
    else:
        ratio = one_ulp_ratio(out, ref, dtype, MIN_NORMAL[dtype])
    for reg in set(b["regime"]):
        sel = torch.tensor([r == reg for r in b["regime"]])
        worst[reg] = round(float(ratio[sel].max()), 3)
    assert bool((ratio <= 1.0).all()), (name, "forward", worst)
    return worst


def check_bwd(case, b, dx, ctrl):
    """All backward rules on one [N, d] CPU result `dx` (storage dtype); `ctrl` the control's dx.  -> {regime: worst ratio}."""
    dtype, d, name = case["dtype"], case["d"], case["name"]
    x, g = b["x"], b["g"]
    if not case["normalize"]:
        assert torch.equal(bits(dx), bits(g)), (name, "dx is not g bit for bit")
        return {"copy": 0.0}
    ref = bwd64(x, g, 1)
    n64 = x.double().pow(2).sum(-1).sqrt()
    clamped = n64 < EPS
    regs = sorted(set(b["regime"]))
    of = {reg: torch.tensor([r == reg for r in b["regime"]]) for reg in regs}
    for reg in regs:
        assert bool((clamped[of[reg]] == (reg in CLAMPED)).all()), (name, reg)
    err = (dx.double() - ref).norm(dim=-1)
    extra = parallel_extra(x, g, d, dtype) if case["g"] == "parallel" else torch.zeros_like(err)
    ctrl_err = (ctrl.double() - ref).norm(dim=-1)
    ctrl_err = torch.where(n64 <= torch.finfo(dtype).max, ctrl_err, torch.zeros_like(ctrl_err))     # fp16 `large`: no control
    bound = rule_bound(ctrl_err, ref.norm(dim=-1), dtype, extra)
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, float("inf")).double())
    by_ulp = clamped & (dtype != torch.float32)                      # 16-bit clamped rows: the elementwise rule instead
    for n in torch.nonzero(by_ulp).flatten().tolist():
        want = ref[n].to(dtype)                                      # +-inf where g / eps leaves fp16
        fin = torch.isfinite(want.float())
        assert torch.equal(dx[n][~fin], want[~fin]), (name, b["regime"][n], "overflowing elements")
        ratio[n] = float(one_ulp_ratio(dx[n][fin], ref[n][fin], dtype, MIN_NORMAL[dtype])) if bool(fin.any()) else 0.0
        assert bool((dx[n][g[n] == 0] == 0).all()), (name, b["regime"][n])
    assert torch.isfinite(dx[~by_ulp].float()).all(), name
    worst = {reg: round(float(ratio[of[reg]].max()), 3) for reg in regs}
    assert bool((ratio <= 1.0).all()), (name, case["g"], worst, err[ratio > 1].tolist()[:4], bound[ratio > 1].tolist()[:4])
    return worst
