"""Float64 parity of the hand-written kernels of the Llama training path outside attention: fused residual add + RMSNorm
(forward, backward), SwiGLU (forward, backward, transposed-product backward), RoPE (forward, backward) and the flat AdamW step
with the gradient sum of squares that feeds clipping (rankpo_amd/csrc/encoder_ops.hip, rankpo_amd/csrc/optim.hip).

References are float64 computations on the EXACT stored inputs (the bf16 / f32 tensors the kernel reads, upcast, never
re-rounded; the f32 cos / sin tables as given; the f32 scalars as the C ABI receives them), on the device.

Error model.  No bound scales with a tensor's global maximum.
  * Reductions (RMSNorm y / dx, the dw partials, the sum-of-squares partials): per row (per wave and column for dw, per block
    for sumsq), against the terms the row sums, so one wrong row among 10^5 shows.
  * Elementwise outputs (SwiGLU, RoPE, AdamW): |out - ref| <= c u sum|terms| + 1/2 ulp_T(max(|ref|, |out|)) with u = 2^-24, the
    f32 unit roundoff of the kernels' arithmetic; the half ulp is the final rounding to the stored type (taken at the larger of
    the two magnitudes, so that a result rounded across a binade boundary is covered).  Every c is derived beside its use.
  * Where PyTorch computes the same operation on the same inputs (F.rms_norm, F.silu(g) * u autograd) it runs as a CONTROL:
    per row, kernel error <= 1.5 x control error + FLOOR[T].  HF-style RoPE rounds cos / sin to the storage type, a weaker
    operation than the kernel's f32 tables: it is a sanity bound only.

Outputs the kernels are meant to write are NaN-prefilled, padding beyond a row / a buffer is checked untouched, and the cases
are chosen to reach every thread mapping and loop of the kernels (each regime asserts that its inputs reach it).  Calls go
through the C ABI (`_lib.load()`), except where the autograd wiring of `ops` is itself under test."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")

U = 2.0 ** -24                                   # f32 unit roundoff: every kernel computes in f32
U_STORE = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8}   # relative rounding of the final store (f32: counted in the c's)
P_BITS = {torch.float32: 24, torch.bfloat16: 8}  # significand bits of the storage type
VEC = {torch.float32: 4, torch.bfloat16: 8}      # elements per 16-byte vector (Elem<T>::kVec)
# additive floor of the control rule.  bf16: 2^-10 is ~ 1/2 of the per-row rounding error of one bf16 store (u_bf16 / sqrt(3) ~
# 2^-9.3), so two implementations that both round once stay inside 1.5 x + floor with many sigma to spare.  f32: 2^-18 = 64 u
# covers what the kernels' f32 approximations (rsqrtf, __expf) may lose against PyTorch's correctly rounded libm at the
# magnitudes that dominate a row's norm; the a-priori bounds below are the tight check there.
FLOOR = {torch.float32: 2.0 ** -18, torch.bfloat16: 2.0 ** -10}
RPO_ERR_UNSUPPORTED = -2                          # include/rankpo_hip.h


def _lib():
    from rankpo_amd import _lib as L
    return L.load()


def _abi():
    from rankpo_amd.ops import _dt, _stream
    return _dt, _stream


def _p(t):
    return None if t is None else t.data_ptr()


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _cdiv(a, b):
    return -(-a // b)


def half_ulp(a, dtype):
    """1/2 ulp of the storage type at float64 magnitudes a (subnormal spacing below the normal range, 2^-126)."""
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, -125), e.clamp(min=-125))
    return torch.ldexp(torch.ones_like(a), e - P_BITS[dtype] - 1)


def check_elem(name, out, ref, bound):
    """|out - ref| <= bound + 1/2 ulp_T per element; NaN / inf fail."""
    o = out.double()
    tol = bound + half_ulp(torch.maximum(ref.abs(), o.abs().nan_to_num(0.0, 0.0, 0.0)), out.dtype)
    err = (o - ref).abs()
    bad = ~(err <= tol)
    if bad.any():
        i = int(bad.flatten().nonzero()[0])
        ratio = float((err / tol).nan_to_num(float("inf")).max())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at flat index {i}: "
                             f"out {float(o.flatten()[i])!r} ref {float(ref.flatten()[i])!r} tol {float(tol.flatten()[i]):.3e}; "
                             f"worst err / tol {ratio:.3g}")


def check_rows(name, err, bound):
    """per-row errors against per-row bounds (NaN fails)."""
    bad = ~(err <= bound)
    if bad.any():
        i = int(bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} rows out of bound; first row {i}: err {float(err[i]):.3e} "
                             f"bound {float(bound[i]):.3e}")


def check_control(name, err, ctrl_err, dtype):
    check_rows(name + " (vs control)", err, 1.5 * ctrl_err + FLOOR[dtype])


def row_norm(x):
    return x.reshape(x.shape[0], -1).norm(dim=1)


# ============================================================================================================ RMSNorm
NORM_EPS = 1e-5
EPS32 = float(np.float32(NORM_EPS))               # what the kernel receives (c_float)


def norm_kmax(dtype, d):
    """the KMAX instantiation launch_norm_fwd / _bwd pick for width d."""
    kk = _cdiv(d // VEC[dtype], 64)
    return next(k for k in (1, 2, 4, 8, 16) if kk <= k)


def c_rstd(d):
    # rstd = rsqrtf(ss / d + eps): ss sums d squares as one chain of d / 64 fma per lane and a 6-step butterfly,
    # relative error <= (d / 64 + 6) u; * inv_d (inv_d rounded: u; product: u) and + eps (u): (d / 64 + 9) u on the mean;
    # the square root halves that, (d / 128 + 4.5) u; rsqrtf is a 1-ulp (<= 2 u) approximation: d / 128 + 6.5 -> d / 128 + 8
    return d / 128 + 8


def _norm_inputs(dtype, rows, d, with_delta, with_dres, seed):
    """rows of very different scale (10^-3 .. 10^3, independently for x and the incoming gradients)."""
    g = _gen(seed)
    sx = 10.0 ** (torch.rand(rows, 1, device=DEV, generator=g) * 6 - 3)
    x = (torch.randn(rows, d, device=DEV, generator=g) * sx).to(dtype)
    delta = (0.5 * torch.randn(rows, d, device=DEV, generator=g) * sx).to(dtype) if with_delta else None
    w = (1 + 0.25 * torch.randn(d, device=DEV, generator=g)).to(dtype)
    sy = 10.0 ** (torch.rand(rows, 1, device=DEV, generator=g) * 6 - 3)
    dy = (torch.randn(rows, d, device=DEV, generator=g) * sy).to(dtype)
    dres = (torch.randn(rows, d, device=DEV, generator=g) * sy).to(dtype) if with_dres else None
    return x, delta, w, dy, dres


def _norm_fwd(x, delta, w):
    _dt, _stream = _abi()
    rows, d = x.shape
    y = torch.full_like(x, NAN)
    rstd = torch.full((rows,), NAN, dtype=torch.float32, device=DEV)
    xn = torch.full_like(x, NAN) if delta is not None else None
    rc = _lib().rpo_add_rmsnorm_fwd(x.data_ptr(), _p(delta), w.data_ptr(), NORM_EPS, _p(xn), y.data_ptr(), rstd.data_ptr(),
                                    rows, d, _dt(x), _stream(x))
    return rc, (xn if delta is not None else x), y, rstd


def _norm_parity(dtype, rows, d, with_delta, with_dres, seed, backward=True, control=True):
    lib = _lib()
    _dt, _stream = _abi()
    x, delta, w, dy, dres = _norm_inputs(dtype, rows, d, with_delta, with_dres, seed)
    rc, xn, y, rstd = _norm_fwd(x, delta, w)
    assert rc == 0, rc
    if with_delta:   # x + delta in f32, rounded once to the storage type: exactly torch's f32 add + RNE cast
        assert torch.equal(xn, (x.float() + delta.float()).to(dtype)), "x_new"
    nw = lib.rpo_add_rmsnorm_waves(rows)
    rpw = _cdiv(rows, nw)
    used = _cdiv(rows, rpw)                               # waves that own at least one row
    assert nw % 4 == 0 and nw >= used
    if backward:
        dx = torch.full_like(x, NAN)
        dwp = torch.full((nw, d), NAN, dtype=torch.float32, device=DEV)
        rc = lib.rpo_add_rmsnorm_bwd(dy.data_ptr(), xn.data_ptr(), w.data_ptr(), rstd.data_ptr(), _p(dres), dx.data_ptr(),
                                     dwp.data_ptr(), rows, d, _dt(x), _stream(x))
        assert rc == 0, rc
    if control:
        xl, wl = xn.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
        yc = F.rms_norm(xl, (d,), wl, NORM_EPS)
        if backward:
            yc.backward(dy)
        yc = yc.detach()
    torch.cuda.synchronize()
    f = torch.float64
    wd = w.to(f)[None]
    e_y, e_yc = torch.empty(rows, dtype=f, device=DEV), torch.empty(rows, dtype=f, device=DEV)
    e_dx, e_dxc = torch.empty(rows, dtype=f, device=DEV), torch.empty(rows, dtype=f, device=DEV)
    dw_ref, dw_abs = torch.zeros(d, dtype=f, device=DEV), torch.zeros(d, dtype=f, device=DEV)
    y_tol = (c_rstd(d) + 3) * U + U_STORE[dtype]          # y = (x rstd) w: rstd's error + 2 products (+1 u: second order)
    cw = max(1, (1 << 23) // (d * rpw))                   # waves per reference chunk (~8 M float64 elements per temporary)
    for w0 in range(0, used, cw):
        w1 = min(used, w0 + cw)
        r0, r1 = w0 * rpw, min(rows, w1 * rpw)
        xs = xn[r0:r1].to(f)
        rstd_ref = (xs.square().mean(1) + EPS32).rsqrt()
        check_rows(f"rstd rows {r0}..", (rstd[r0:r1].to(f) - rstd_ref).abs() / rstd_ref,
                   torch.full_like(rstd_ref, c_rstd(d) * U))
        yref = xs * rstd_ref[:, None] * wd
        nref = row_norm(yref)
        e_y[r0:r1] = row_norm(y[r0:r1].to(f) - yref) / nref
        if control:
            e_yc[r0:r1] = row_norm(yc[r0:r1].to(f) - yref) / nref
        if not backward:
            continue
        # the backward reads the forward's f32 rstd: the reference uses the same value
        rs = rstd[r0:r1].to(f)[:, None]
        dys = dy[r0:r1].to(f)
        xh = xs * rs
        gg = dys * wd
        t = gg * xh
        c = t.mean(1, keepdim=True)
        cabs = t.abs().mean(1, keepdim=True)
        dxr = (gg - xh * c) * rs
        # dx = (g - xh c) rstd + dres: c sums d products as a d / 64 fma chain per lane + a 6-step butterfly, with xh and g
        # rounded (2 u) and * inv_d (2 u): |dc| <= (d / 64 + 10) u mean|g xh|; the second pass rounds xh, g, xh c, the
        # difference and the product by rstd (<= 4 u on |g| + |xh c|), the + dres 1 u
        bnd = ((d / 64 + 10) * xh.abs() * cabs + 4 * (gg.abs() + (xh * c).abs())) * rs * U
        if with_dres:
            dr = dres[r0:r1].to(f)
            dxr = dxr + dr
            bnd = bnd + dr.abs() * U
        nref = row_norm(dxr)
        e = row_norm(dx[r0:r1].to(f) - dxr)
        # + the final rounding to the storage type, relative to the f32 value (|ref| (1 + its f32 error < 2^-10))
        check_rows(f"dx rows {r0}..", e, row_norm(bnd) + U_STORE[dtype] * nref * (1 + 2.0 ** -10))
        e_dx[r0:r1] = e / nref
        if control and not with_dres:
            e_dxc[r0:r1] = row_norm(xl.grad[r0:r1].to(f) - dxr) / nref
        # dw partial of wave k = sum over ITS rows (k rpw .. (k + 1) rpw) of dy xh, one f32 fma chain of rpw terms per lane
        # with xh = x rstd rounded: <= (rpw + 1) u sum|dy xh| -> rpw + 2
        pt = dys * xh
        pad = (w1 - w0) * rpw - (r1 - r0)
        pt = torch.cat([pt, pt.new_zeros(pad, d)]) if pad else pt
        pref = pt.view(w1 - w0, rpw, d).sum(1)
        pabs = pt.abs().view(w1 - w0, rpw, d).sum(1)
        check_elem(f"dw_partial waves {w0}..{w1}", dwp[w0:w1], pref, (rpw + 2) * U * pabs)
        dw_ref += pref.sum(0)
        dw_abs += pabs.sum(0)
    check_rows("y", e_y, torch.full_like(e_y, y_tol))
    if control:
        check_control("y", e_y, e_yc, dtype)
    if not backward:
        return
    # every wave that owns no row still writes its dw_partial row: zeros (the caller sums all nw rows of a torch.empty buffer)
    assert (dwp[used:] == 0).all(), f"dw_partial rows {used}..{nw} (waves without a row) not all zero"
    if control:
        if not with_dres:
            check_control("dx", e_dx, e_dxc, dtype)
        den = dw_abs.clamp_min(1e-300)                    # (a column whose terms are all zero: both sides must be exactly 0)
        e_dw = (dwp.to(f).sum(0) - dw_ref).abs() / den
        e_dwc = (wl.grad.to(f) - dw_ref).abs() / den
        check_control("dw per column", e_dw, e_dwc, dtype)


NORM_ROWS = [1, 5, 8191, 8192, 8193, 3 * 8192 + 5]
# every KMAX that ops.fused_norm_ok admits, with widths that are no multiple of 64 V (a lane without a vector in the last k)
NORM_WIDTHS = [(torch.float32, d) for d in (200, 384, 520, 1032, 2048)] + \
              [(torch.bfloat16, d) for d in (200, 520, 1032, 2048, 3080, 4096)]


def test_norm_cases_cover_every_kmax():
    from rankpo_amd import ops
    for dtype in (torch.float32, torch.bfloat16):
        ds = [d for t, d in NORM_WIDTHS if t == dtype]
        assert all(ops.fused_norm_ok(torch.empty(1, d, device=DEV, dtype=dtype)) for d in ds)
        assert {norm_kmax(dtype, d) for d in ds} == {1, 2, 4, 8}, dtype
        assert any(d % (64 * VEC[dtype]) for d in ds if norm_kmax(dtype, d) == 8)
    rpw = {r: _cdiv(r, _lib().rpo_add_rmsnorm_waves(r)) for r in NORM_ROWS}
    assert rpw[1] == rpw[8192] == 1 and rpw[8193] == 2 and rpw[3 * 8192 + 5] == 4
    assert _lib().rpo_add_rmsnorm_waves(5) == 8             # 3 waves without a row


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", NORM_ROWS)
@pytest.mark.parametrize("delta_dres", [(True, True), (False, False)], ids=["delta+dres", "plain"])
def test_add_rmsnorm_rows(dtype, rows, delta_dres):
    """1 / 5 rows (waves without a row), 8191 / 8192 (one row per wave), 8193 (2 rows per wave, half the waves idle),
    3 x 8192 + 5 (4 rows per wave, ragged last wave): the multi-row loop r0 .. r1 of both kernels."""
    _norm_parity(dtype, rows, 520, *delta_dres, seed=rows)


@pytest.mark.parametrize("dtype,d", NORM_WIDTHS, ids=[f"{'f32' if t == torch.float32 else 'bf16'}-{d}" for t, d in NORM_WIDTHS])
@pytest.mark.parametrize("delta_dres", [(True, False), (False, True)], ids=["delta", "dres"])
def test_add_rmsnorm_widths(dtype, d, delta_dres):
    """every KMAX instantiation at 20000 rows (3 rows per wave, a last wave of 2)."""
    _norm_parity(dtype, 20000, d, *delta_dres, seed=d)


def test_add_rmsnorm_production_scale():
    """the cfg-2 batch shape: 151 552 x 2048 bf16, 19 rows per wave, a last wave of 8 rows, 215 waves without a row."""
    rows = 151552
    assert _cdiv(rows, _lib().rpo_add_rmsnorm_waves(rows)) >= 16
    _norm_parity(torch.bfloat16, rows, 2048, True, True, seed=7)


def test_add_rmsnorm_f32_4096_forward_only_abi():
    """f32 d = 4096 (KMAX = 16) exists in the forward only; ops never routes it (fused_norm_ok), the backward refuses it."""
    from rankpo_amd import ops
    assert not ops.fused_norm_ok(torch.empty(1, 4096, device=DEV))
    assert norm_kmax(torch.float32, 4096) == 16
    rows, d = 3 * 8192 + 5, 4096
    _norm_parity(torch.float32, rows, d, True, False, seed=11, backward=False)
    _dt, _stream = _abi()
    x = torch.randn(8, d, device=DEV)
    rstd = torch.ones(8, device=DEV)
    dx, dwp = torch.full_like(x, NAN), torch.full((8, d), NAN, device=DEV)
    rc = _lib().rpo_add_rmsnorm_bwd(x.data_ptr(), x.data_ptr(), x[0].data_ptr(), rstd.data_ptr(), None, dx.data_ptr(),
                                    dwp.data_ptr(), 8, d, _dt(x), _stream(x))
    assert rc == RPO_ERR_UNSUPPORTED, rc
    torch.cuda.synchronize()
    assert dx.isnan().all() and dwp.isnan().all()


def test_add_rmsnorm_ops_autograd_idle_waves():
    """through ops.add_rmsnorm (its torch.empty dw_partial buffer, the f32 sum, the dres fold): 3 x 8192 + 5 bf16 rows."""
    from rankpo_amd import ops
    dtype, rows, d = torch.bfloat16, 3 * 8192 + 5, 2048
    x0, dl0, w0, gy, gx = _norm_inputs(dtype, rows, d, True, True, seed=5)
    x, dl, w = (t.clone().requires_grad_(True) for t in (x0, dl0, w0))
    xn, y = ops.add_rmsnorm(x, dl, w, NORM_EPS)
    nw = _lib().rpo_add_rmsnorm_waves(rows)
    rpw = _cdiv(rows, nw)
    # a NaN block of exactly the dw_partial size, freed just before the backward: the caching allocator hands it back, so a
    # row the kernel leaves unwritten reads NaN instead of whatever the block held
    poison = torch.full((nw, d), NAN, dtype=torch.float32, device=DEV)
    del poison
    ((y * gy).float().sum() + (xn * gx).float().sum()).backward()
    f = torch.float64
    xs = xn.detach().to(f)
    assert torch.equal(xn, (x0.float() + dl0.float()).to(dtype))
    _, _, _, rstd = _norm_fwd(xn.detach(), None, w0)     # the rstd the forward saved (same kernel, same x_new)
    rs = rstd.to(f)[:, None]
    xh = xs * rs
    pt = gy.to(f) * xh
    ref = pt.sum(0)
    # dw = bf16(f32 sum over the nw partials): partials as above ((rpw + 2) u sum|terms|), torch's f32 sum of 8192 rows <= 64 u
    # of the same terms (any summation tree of depth <= 64), then one bf16 rounding
    check_elem("ops dw", w.grad, ref, (rpw + 2 + 64) * U * pt.abs().sum(0))
    gg = gy.to(f) * w0.to(f)[None]
    c = (gg * xh).mean(1, keepdim=True)
    dxr = (gg - xh * c) * rs + gx.to(f)
    e = row_norm(x.grad.to(f) - dxr) / row_norm(dxr)
    # the dx bound of _norm_parity, (d / 64 + 10) u on c and 4 u on the second pass + 1 u for dres, taken relative to the row
    # (no cancellation on these inputs: dres is as large as dy's share) with 1 u to spare; then one bf16 rounding (+ 2^-10 of
    # it for the f32 error it rounds)
    check_rows("ops dx", e, torch.full_like(e, (d / 64 + 16) * U + U_STORE[dtype] * (1 + 2.0 ** -10)))
    assert torch.equal(x.grad, dl.grad)


# ============================================================================================================ RoPE
ROPE_THETA = 500000.0                             # Llama 3
ROPE_MAX_POS = 131071


def rope_tables(pos, hd):
    """f32 [len(pos), hd / 2] tables, angles in float64, rounded once: the tables as the kernel is given them."""
    inv = 1.0 / ROPE_THETA ** (torch.arange(0, hd, 2, device=DEV, dtype=torch.float64) / hd)
    ang = pos.to(torch.float64)[:, None] * inv[None]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def rope_ref(x, cos, sin, heads, hd, sign):
    """float64 rotation of the first heads * hd columns of x [rows, row_len]; row r uses table row r % period.  Returns the
    reference [rows, heads, hd] and the magnitudes of the two terms each element sums."""
    rows, half = x.shape[0], hd // 2
    idx = torch.arange(rows, device=DEV) % cos.shape[0]
    c = cos.to(torch.float64)[idx][:, None, :]
    s = sign * sin.to(torch.float64)[idx][:, None, :]
    xr = x[:, :heads * hd].to(torch.float64).view(rows, heads, hd)
    x1, x2 = xr[..., :half], xr[..., half:]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)
    terms = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], -1)
    return ref, terms


def check_rope(name, out, ref, terms, heads, hd):
    # x1 cos - x2 sin: two products and a difference in f32 (an FMA contraction only drops a rounding): <= 2 u (|x1 c| + |x2 s|)
    check_elem(name, out[:, :heads * hd].reshape(ref.shape), ref, 2 * U * terms)


def rope_mapping(dtype, hd, heads):
    """the thread mapping rope_kernel takes for this shape."""
    total = heads * (hd // 2) // VEC[dtype]
    if total <= 128:
        return "rows-per-block" if 256 % total == 0 else "rows-per-block+idle"
    return "one-pass" if total <= 256 else "strided"


ROPE_CASES = [                                    # (dtype, head_dim, heads): (low, high) vector pairs per row
    (torch.bfloat16, 64, 6),                      # 24: rpb = 10 rows per block, 16 idle threads
    (torch.bfloat16, 128, 8),                     # 64: Llama-3-8B K heads (the rotary fold's call), rpb = 4
    (torch.bfloat16, 128, 16),                    # 128: the last shape with rpb > 1 (rpb = 2)
    (torch.bfloat16, 64, 40),                     # 160: one pass, 96 idle threads
    (torch.bfloat16, 128, 32),                    # 256: one pass, every thread
    (torch.bfloat16, 128, 40),                    # 320: the strided loop (Llama-3-8B q|k heads)
    (torch.float32, 64, 6),                       # 48: rpb = 5, 16 idle threads
    (torch.float32, 128, 8),                      # 128: pairs == 128 boundary
    (torch.float32, 64, 20),                      # 160: one pass
    (torch.float32, 128, 40),                     # 640: strided loop, three trips
]


def test_rope_cases_cover_every_mapping():
    for dtype in (torch.float32, torch.bfloat16):
        cases = [(hd, h) for t, hd, h in ROPE_CASES if t == dtype]
        maps = {rope_mapping(dtype, hd, h) for hd, h in cases}
        assert {"rows-per-block+idle", "one-pass", "strided"} <= maps, (dtype, maps)
        assert any(h * (hd // 2) // VEC[dtype] == 128 for hd, h in cases)
        assert {64, 128} <= {hd for hd, _ in cases}
    assert {(128, 40), (128, 8)} <= {(hd, h) for t, hd, h in ROPE_CASES if t == torch.bfloat16}


@pytest.mark.parametrize("dtype,hd,heads", ROPE_CASES,
                         ids=[f"{'f32' if t == torch.float32 else 'bf16'}-hd{hd}-h{h}" for t, hd, h in ROPE_CASES])
@pytest.mark.parametrize("tables", ["padded", "packed"])
def test_rope_parity(dtype, hd, heads, tables):
    """forward and backward, out of place (NaN-prefilled) and in place.  padded: period = L tables, rows = N L, a row stride of
    heads + 2 heads (fused q|k|v: the columns beyond stay bit-identical / unwritten); packed: one table row per token,
    positions up to 131 071."""
    lib = _lib()
    _dt, _stream = _abi()
    g = _gen(hd * 100 + heads)
    if tables == "padded":
        N, L = 5, 61
        rows, pos, extra = N * L, torch.arange(L, device=DEV), 2 * hd
    else:
        rows, extra = 307, 0
        pos = torch.randint(0, ROPE_MAX_POS + 1, (rows,), device=DEV, generator=g)
        pos[0], pos[1] = ROPE_MAX_POS, 0
    cos, sin = rope_tables(pos, hd)
    period = cos.shape[0]
    row_len = heads * hd + extra
    x = torch.randn(rows, row_len, device=DEV, generator=g).to(dtype)
    rpb = max(1, 256 // (heads * (hd // 2) // VEC[dtype])) if heads * (hd // 2) // VEC[dtype] <= 128 else 1
    assert _cdiv(rows, rpb) < rows or rpb == 1          # the in-place row loop would revisit rows if it stepped by gridDim.x
    for backward in (0, 1):
        ref, terms = rope_ref(x, cos, sin, heads, hd, -1.0 if backward else 1.0)
        out = torch.full_like(x, NAN)
        assert lib.rpo_rope(x.data_ptr(), out.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, period,
                            _dt(x), backward, _stream(x)) == 0
        xi = x.clone()
        assert lib.rpo_rope(xi.data_ptr(), xi.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, period,
                            _dt(x), backward, _stream(x)) == 0
        torch.cuda.synchronize()
        check_rope(f"rope bwd={backward} out of place", out, ref, terms, heads, hd)
        check_rope(f"rope bwd={backward} in place", xi, ref, terms, heads, hd)
        assert torch.equal(xi[:, :heads * hd], out[:, :heads * hd])        # same arithmetic either way
        if extra:
            assert out[:, heads * hd:].isnan().all(), "out-of-place rope wrote beyond the rotated heads"
            assert torch.equal(xi[:, heads * hd:], x[:, heads * hd:]), "in-place rope changed the columns beyond the rotated heads"
        if not backward:
            # sanity control: HF's formula with the tables rounded to the storage type, in the storage type
            c2 = torch.cat([cos, cos], -1).to(dtype)[torch.arange(rows, device=DEV) % period][:, None]
            s2 = torch.cat([sin, sin], -1).to(dtype)[torch.arange(rows, device=DEV) % period][:, None]
            xv = x[:, :heads * hd].view(rows, heads, hd)
            ctrl = xv * c2 + torch.cat([-xv[..., hd // 2:], xv[..., :hd // 2]], -1) * s2
            nref = row_norm(ref)
            check_control("rope fwd", row_norm(out[:, :heads * hd].to(torch.float64).view_as(ref) - ref) / nref,
                          row_norm(ctrl.to(torch.float64) - ref) / nref, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("grad_inplace", [True, False])
@pytest.mark.parametrize("extra_heads", [8, 0])
def test_rope_ops_autograd(dtype, grad_inplace, extra_heads):
    """ops.rope_ on a Llama-3-8B q|k|v row (40 rotated heads of 128 + 8 v heads, packed positions), and with no pass-through
    columns (grad_inplace=False then writes a fresh torch.empty gradient: every element must be written)."""
    from rankpo_amd import ops
    g = _gen(17 + extra_heads)
    heads, hd, rows = 40, 128, 2 * 97
    pos = torch.randint(0, ROPE_MAX_POS + 1, (rows,), device=DEV, generator=g)
    pos[-1] = ROPE_MAX_POS
    cos, sin = rope_tables(pos, hd)
    row_len = (heads + extra_heads) * hd
    x0 = torch.randn(rows, row_len, device=DEV, generator=g).to(dtype)
    gy = torch.randn(rows, row_len, device=DEV, generator=g).to(dtype)
    x = x0.clone().requires_grad_(True)
    y = ops.rope_(x * 1.0, cos, sin, heads, hd, grad_inplace=grad_inplace)
    y.backward(gy.clone())                      # grad_inplace rotates the incoming gradient buffer itself
    ref, terms = rope_ref(x0, cos, sin, heads, hd, 1.0)
    check_rope("ops.rope_ forward", y.detach(), ref, terms, heads, hd)
    ref, terms = rope_ref(gy, cos, sin, heads, hd, -1.0)
    check_rope("ops.rope_ backward", x.grad, ref, terms, heads, hd)
    assert torch.equal(y.detach()[:, heads * hd:], x0[:, heads * hd:])
    assert torch.equal(x.grad[:, heads * hd:], gy[:, heads * hd:])


# ============================================================================================================ SwiGLU
G0 = -1.2784645427610738                          # the zero of silu'(g) = s (1 + g (1 - s)), s = sigmoid(g)
EXP_OVERFLOW = 88.7228                            # ln(FLT_MAX): __expf(-g) = inf below g = -88.72
SW_SHAPES = [(203, 520, True), (37, 264, False), (1100, 1032, False)]   # (rows, cols, fused g|u layout)
SW_REGIMES = ["normal", "saturated", "cluster"]


def _gates(regime, rows, cols, dtype, g):
    if regime == "normal":
        return torch.randn(rows, cols, device=DEV, generator=g).to(dtype)
    if regime == "saturated":
        mag = 10 + 90 * torch.rand(rows, cols, device=DEV, generator=g)
        return torch.where(torch.rand(rows, cols, device=DEV, generator=g) < 0.5, -mag, mag).to(dtype)
    return (G0 + 0.02 * torch.randn(rows, cols, device=DEV, generator=g)).to(dtype)


def swiglu_ref(g, u, d=None):
    """float64 prod = silu(g) u, du = d silu(g), dg = d u silu'(g), with the per-element error bounds of the kernels' f32
    arithmetic (rounding to the storage type excluded: check_elem adds it)."""
    f = torch.float64
    g, u = g.to(f), u.to(f)
    s, oms = torch.sigmoid(g), torch.sigmoid(-g)          # 1 - s without cancellation
    silu = g * s
    # s = 1 / (1 + __expf(-g)).  __expf: 2 + 1.17 |g| ulp (the documented bound of the fast exp: the argument is scaled by
    # log2(e) and rounded before v_exp_f32), 1 ulp <= 2 u: relative error (3 |g| + 4) u in e = exp(-g), which moves s by
    # s (1 - s) times that; 1 + e and the reciprocal: 3 u of s.  Below g = -88.72, e = inf and s = 0 where s < 2^-127: the
    # absolute floor 2^-126 (the f32 normal range) covers that and any denormal flush.
    es = s * oms * (3 * g.abs() + 4) * U + 3 * U * s + 2.0 ** -126
    e_silu = g.abs() * es + U * silu.abs()                # silu = g s: s's error times |g|, one rounding
    out = {"prod": (silu * u, u.abs() * (e_silu + U * silu.abs())),   # * u: one more rounding
           "terms": {"prod": (silu * u).abs()}}
    if d is not None:
        d = d.to(f)
        out["du"] = (d * silu, d.abs() * (e_silu + U * silu.abs()))
        P = s + silu * oms
        TP = s + silu.abs() * oms                         # the terms of silu' = s + silu (1 - s), which cancel near G0
        # dg = (d u) (s + silu (1 - s)): s's error enters P through s, silu and 1 - s (<= (1 + |g| + |silu|) es); the
        # roundings of silu, 1 - s, silu (1 - s), the sum, d u and the final product: <= 6 u of the terms
        out["dg"] = (d * u * P, (d * u).abs() * ((1 + g.abs() + silu.abs()) * es + 6 * U * TP))
        out["_TP"], out["_P"] = TP, P
        out["terms"].update(du=(d * silu).abs(), dg=(d * u).abs() * TP)
    return out


def bits(t):
    """the raw bits of a tensor (NaN-safe equality)."""
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _sw_inputs(dtype, rows, cols, fused, regime, seed):
    """g, u views with a common row stride, dout: [rows, cols] views into (padded) buffers, as the C ABI takes them."""
    V = VEC[dtype]
    g = _gen(seed)
    gt = _gates(regime, rows, cols, dtype, g)
    ut = torch.randn(rows, cols, device=DEV, generator=g).to(dtype)
    dt = torch.randn(rows, cols, device=DEV, generator=g).to(dtype)
    if fused:                                             # ops' layout: one [rows, 2 cols] gate|up projection output
        gu = torch.cat([gt, ut], -1).contiguous()
        gv, uv, ld_gu = gu[:, :cols], gu[:, cols:], 2 * cols
        dbuf, ld_d = dt.contiguous(), cols
    else:                                                 # separate buffers, strides beyond the row
        ld_gu, ld_d = cols + 2 * V, cols + V
        gb = torch.full((rows, ld_gu), NAN, dtype=dtype, device=DEV)
        ub = torch.full((rows, ld_gu), NAN, dtype=dtype, device=DEV)
        dbuf = torch.full((rows, ld_d), NAN, dtype=dtype, device=DEV)
        gb[:, :cols], ub[:, :cols], dbuf[:, :cols] = gt, ut, dt
        gv, uv = gb[:, :cols], ub[:, :cols]
    if regime == "saturated":
        gf = gv.float()
        assert (gf.abs() >= 10).all() and (gf < -EXP_OVERFLOW).any() and (gf > 17).any()   # exp(-g) = inf; s rounds to 1
    elif regime == "cluster":
        r = swiglu_ref(gv, uv, dbuf[:, :cols])
        assert (r["_P"].abs() < 2.0 ** -5 * r["_TP"]).float().mean() >= 0.5               # silu' cancels to < 2^-5 of its terms
    else:
        assert gv.float().abs().max() < 8 and (gv.float().abs() > 2).any()
    return gv, uv, ld_gu, dbuf, ld_d


def _sw_out(rows, cols, ld, dtype):
    buf = torch.full((rows, ld), NAN, dtype=dtype, device=DEV)
    return buf, buf[:, :cols]


def _sw_dgu(rows, cols, fused, dtype):
    """dg, du views with one row stride (the ABI's ld_dgu) and the buffers whose columns beyond `cols` must stay unwritten."""
    if fused:                                             # ops' layout: [dg | du] of one [rows, 2 cols] buffer
        b = torch.full((rows, 2 * cols), NAN, dtype=dtype, device=DEV)
        return b[:, :cols], b[:, cols:], 2 * cols, []
    ld = cols + 3 * VEC[dtype]
    (gb, dg), (ub, du) = _sw_out(rows, cols, ld, dtype), _sw_out(rows, cols, ld, dtype)
    return dg, du, ld, [gb, ub]


def _sw_control(gv, uv, d):
    gl, ul = gv.detach().clone().requires_grad_(True), uv.detach().clone().requires_grad_(True)
    prod = F.silu(gl) * ul
    prod.backward(d)
    return {"prod": prod.detach(), "dg": gl.grad, "du": ul.grad}


def _sw_check(name, key, got, ref, ctrl, dtype):
    r, bound = ref[key]
    check_elem(name, got, r, bound)
    t = row_norm(ref["terms"][key])
    check_control(name, row_norm(got.double() - r) / t, row_norm(ctrl[key].double() - r) / t, dtype)


def _check_pads(name, bufs, cols):
    for b in bufs:
        assert b[:, cols:].isnan().all(), f"{name}: written beyond the {cols} columns of a row"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SW_SHAPES, ids=[f"{r}x{c}{'-fused' if f else ''}" for r, c, f in SW_SHAPES])
@pytest.mark.parametrize("regime", SW_REGIMES)
def test_swiglu_rowmajor_parity(dtype, shape, regime):
    """rpo_swiglu_fwd, then rpo_swiglu_bwd without a product, with a separate product, and with the product written over
    dout in place (as ops does)."""
    lib = _lib()
    _dt, _stream = _abi()
    rows, cols, fused = shape
    V = VEC[dtype]
    gv, uv, ld_gu, dbuf, ld_d = _sw_inputs(dtype, rows, cols, fused, regime, seed=rows + cols + len(regime))
    dv = dbuf[:, :cols]
    ref = swiglu_ref(gv, uv, dv)
    ctrl = _sw_control(gv, uv, dv)
    st, dt = _stream(gv), _dt(gv)
    ld_o = cols if fused else cols + V
    ob, o = _sw_out(rows, cols, ld_o, dtype)
    assert lib.rpo_swiglu_fwd(gv.data_ptr(), uv.data_ptr(), o.data_ptr(), rows, cols, ld_gu, ld_o, dt, st) == 0
    checks = [("fwd: prod", "prod", o)]
    pads = [ob] if not fused else []
    untouched = []
    for mode in ("none", "separate", "over-dout"):
        dg, du, ld_dgu, pb = _sw_dgu(rows, cols, fused, dtype)
        pads += pb
        dbuf2 = dbuf.clone()
        d2 = dbuf2[:, :cols]
        prod, ld_p = None, ld_o
        if mode == "separate":
            pbuf, prod = _sw_out(rows, cols, ld_o, dtype)
            pads += [pbuf] if not fused else []
        elif mode == "over-dout":
            prod, ld_p = d2, ld_d
            pads += [dbuf2] if not fused else []
        else:
            untouched.append(dbuf2)
        assert lib.rpo_swiglu_bwd(gv.data_ptr(), uv.data_ptr(), d2.data_ptr(), dg.data_ptr(), du.data_ptr(), _p(prod), rows,
                                  cols, ld_gu, ld_d, ld_dgu, ld_p, dt, st) == 0
        checks += [(f"{mode}: dg", "dg", dg), (f"{mode}: du", "du", du)]
        if prod is not None:
            checks.append((f"{mode}: prod", "prod", prod))
    torch.cuda.synchronize()
    for name, key, t in checks:
        _sw_check(name, key, t, ref, ctrl, dtype)
    _check_pads("swiglu row-major", pads, cols)
    for b in untouched:
        assert torch.equal(bits(b), bits(dbuf)), "dout changed without a product output"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SW_SHAPES, ids=[f"{r}x{c}{'-fused' if f else ''}" for r, c, f in SW_SHAPES])
@pytest.mark.parametrize("regime", SW_REGIMES)
@pytest.mark.parametrize("dgu_t", [False, True], ids=["prod_t", "prod_t+dgu_t"])
def test_swiglu_transposed_parity(dtype, shape, regime, dgu_t):
    """rpo_swiglu_bwd_t (64 x TC tiles, TC = 256 bf16 / 128 f32) on ragged rows and columns, against float64 on its own:
    row-major dg / du, the transposed product and (DGU_T) the transposed dg | du; the transposed buffers have a row stride
    beyond `rows` whose padding must stay NaN."""
    lib = _lib()
    _dt, _stream = _abi()
    rows, cols, fused = shape
    V = VEC[dtype]
    tc = 256 if dtype == torch.bfloat16 else 128
    assert rows % 64 and cols % tc                      # ragged in both directions
    gv, uv, ld_gu, dbuf, ld_d = _sw_inputs(dtype, rows, cols, fused, regime, seed=3 * rows + cols + len(regime))
    dv = dbuf[:, :cols]
    ref = swiglu_ref(gv, uv, dv)
    ctrl = _sw_control(gv, uv, dv)
    dg, du, ld_dgu, pads = _sw_dgu(rows, cols, fused, dtype)
    ld_t = _cdiv(rows, V) * V + V
    pt = torch.full((cols, ld_t), NAN, dtype=dtype, device=DEV)
    dgt = torch.full((2 * cols, ld_t), NAN, dtype=dtype, device=DEV) if dgu_t else None
    assert lib.rpo_swiglu_bwd_t(gv.data_ptr(), uv.data_ptr(), dv.data_ptr(), dg.data_ptr(), du.data_ptr(), pt.data_ptr(),
                                _p(dgt), rows, cols, ld_gu, ld_d, ld_dgu, ld_t, _dt(gv), _stream(gv)) == 0
    torch.cuda.synchronize()
    _sw_check("bwd_t dg", "dg", dg, ref, ctrl, dtype)
    _sw_check("bwd_t du", "du", du, ref, ctrl, dtype)
    r, b = ref["prod"]
    check_elem("bwd_t prod^T", pt[:, :rows], r.t(), b.t())
    _check_pads("bwd_t dg / du", pads, cols)
    _check_pads("bwd_t prod^T", [pt], rows)
    if dgu_t:
        for k, key in enumerate(("dg", "du")):
            r, b = ref[key]
            check_elem(f"bwd_t {key}^T", dgt[k * cols:(k + 1) * cols, :rows], r.t(), b.t())
        _check_pads("bwd_t dgu^T", [dgt], rows)


# ============================================================================================================ AdamW, sumsq
def f32(x):
    return float(np.float32(x))


ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.1)
ADAM_N = 4 * (256 * 37 + 101)                     # 38 292: n / 4 % 256 = 101 (a partial last block), n % 8 == 4
ADAM_BIG = 300_000_004                            # >= 3 x 10^8 parameters (n % 8 == 4)
ADAM_PAD = 64                                     # sentinel elements behind every buffer
ADAM_CASES = [                                    # (dtype, n, step t, device grad_scale or None)
    (torch.float32, ADAM_N, 1, 0.37),
    (torch.float32, ADAM_N, 5000, None),
    (torch.bfloat16, ADAM_N, 1, 0.37),
    (torch.bfloat16, ADAM_N, 5000, 2.5),
    (torch.bfloat16, ADAM_BIG, 5000, 0.37),
]


@pytest.mark.parametrize("dtype,n,t,gs", ADAM_CASES,
                         ids=[f"{'f32' if d == torch.float32 else 'bf16'}-n{n}-t{t}-gs{gs}" for d, n, t, gs in ADAM_CASES])
def test_adamw_step_parity(dtype, n, t, gs):
    """one rpo_adamw_step against float64 AdamW on the same f32 state, the f32 scalars the ABI receives and the device
    grad_scale; weight decay on; zero moments (with zero and with 1e-9 gradients: eps dominates the denominator); the bf16
    parameter bit-equal to round-to-nearest-even of the new f32 master; the elements behind n untouched."""
    lib = _lib()
    _dt, _stream = _abi()
    assert n % 4 == 0 and (n // 4) % 256 != 0
    if dtype == torch.bfloat16:
        assert n % 8 == 4
    gen = _gen(n % 1000 + t)
    N = n + ADAM_PAD
    sentinel = 7.0

    def buf(x, dt=torch.float32):
        b = torch.full((N,), sentinel, dtype=dt, device=DEV)
        b[:n] = x
        return b

    w0 = buf(0.05 * torch.randn(n, device=DEV, generator=gen))
    gval = torch.randn(n, device=DEV, generator=gen) * 10.0 ** (-4 * torch.rand(n, device=DEV, generator=gen))
    m0 = buf(1e-3 * torch.randn(n, device=DEV, generator=gen))
    v0 = buf((1e-3 * torch.randn(n, device=DEV, generator=gen)).square())
    i = torch.arange(n, device=DEV)
    zero = i % 8 == 3                                    # zero moments ...
    m0[:n][zero] = 0
    v0[:n][zero] = 0
    gval[i % 16 == 3] = 0                                # ... with a zero gradient (no update but the decay)
    gval[i % 16 == 11] *= 1e-9                           # ... with a gradient whose sqrt(v) is below eps
    grad = buf(gval.to(dtype), dtype)
    m, v = m0.clone(), v0.clone()
    if dtype == torch.bfloat16:
        master, param = w0.clone(), buf(w0[:n].to(dtype), dtype)
    else:
        master, param = None, w0.clone()
    p_before = param.clone()
    gs_t = torch.tensor([gs], dtype=torch.float32, device=DEV) if gs is not None else None
    a = ADAM
    bc1, bc2 = 1.0 - a["beta1"] ** t, 1.0 - a["beta2"] ** t
    rc = lib.rpo_adamw_step(param.data_ptr(), _p(master), grad.data_ptr(), m.data_ptr(), v.data_ptr(), n, _dt(grad), a["lr"],
                            a["beta1"], a["beta2"], a["eps"], a["wd"], bc1, bc2, _p(gs_t), _stream(grad))
    assert rc == 0, rc
    torch.cuda.synchronize()
    wk = master if master is not None else param
    for name, b, b0 in (("m", m, m0), ("v", v, v0), ("master", wk, w0)):
        assert (b[n:] == b0[n:]).all(), f"{name}: elements behind n written"
    assert torch.equal(param[n:], p_before[n:]) and (grad[n:] == sentinel).all()
    if dtype == torch.bfloat16:
        assert torch.equal(param[:n], master[:n].to(dtype)), "bf16 parameter != RNE(f32 master)"
    lr, b1, b2, eps, wd = (f32(a[k]) for k in ("lr", "beta1", "beta2", "eps", "wd"))
    bc1, bc2, gsv = f32(bc1), f32(bc2), (f32(gs) if gs is not None else 1.0)
    step, decay = lr / bc1, 1.0 - lr * wd
    eps_dom = 0
    ch = 1 << 24
    for c0 in range(0, n, ch):
        sl = slice(c0, min(n, c0 + ch))
        f = torch.float64
        gk = grad[sl].to(f) * gsv
        mo, vo, wo = m0[sl].to(f), v0[sl].to(f), w0[sl].to(f)
        m_ref = b1 * mo + (1 - b1) * gk                  # 1 - beta1 / 1 - beta2 are exact in f32 (Sterbenz)
        v_ref = b2 * vo + (1 - b2) * gk * gk
        sq = v_ref.sqrt() / math.sqrt(bc2)
        denom = sq + eps
        upd = step * m_ref / denom
        w_ref = wo * decay - upd
        eps_dom += int((sq < eps).sum())
        # m = b1 m + (1 - b1) gk: gk = g * grad_scale rounded, two products, one sum: <= 3 u of the terms
        b_m = 3 * U * (b1 * mo.abs() + (1 - b1) * gk.abs())
        # v = b2 v + (1 - b2) gk gk: gk's rounding twice, two products, b2 v, the sum: <= 5 u of v (all terms >= 0)
        b_v = 5 * U * v_ref
        # w = w decay - step m / denom: w decay (decay = 1 - lr wd rounded: 2 u); the update carries m's error through
        # step / denom and a relative 12 u: denom (v's 5 u halved, sqrtf, 1 / sqrtf(bc2): 2 u, the product, + eps: 7.5 u),
        # lr / bc1, the quotient and the product (3 u), rounded up; the final difference: u |w|
        b_w = 2 * U * (wo * decay).abs() + step * b_m / denom + 12 * U * upd.abs() + U * w_ref.abs()
        check_elem(f"m [{c0}..]", m[sl], m_ref, b_m)
        check_elem(f"v [{c0}..]", v[sl], v_ref, b_v)
        check_elem(f"w [{c0}..]", wk[sl], w_ref, b_w)
    assert eps_dom > 0, "no element where eps dominates the denominator"
    assert wd > 0 and (gs is None or gsv != 1.0)


SUMSQ_NBLK = 1024                                 # FlatAdamW._nblk (rankpo_amd/train_step.py)
SUMSQ_TAIL = 64.0                                 # the elements behind the last whole vector (block 0 sums them)
SUMSQ_CASES = [                                   # (dtype, n)
    (torch.float32, 4 * 9573 + 3),                # 38 active blocks, 3 tail elements
    (torch.bfloat16, 4 * 9573),                   # n % 8 == 4: a 4-element tail
    (torch.bfloat16, 4004),                       # 500 vectors: 2 active blocks, 1022 idle
    (torch.bfloat16, ADAM_BIG),                   # 3 x 10^8
    (torch.float32, 300_000_003),
]


@pytest.mark.parametrize("dtype,n", SUMSQ_CASES, ids=[f"{'f32' if d == torch.float32 else 'bf16'}-n{n}" for d, n in SUMSQ_CASES])
def test_sumsq_partial_parity(dtype, n):
    """rpo_sumsq_partial at FlatAdamW's 1024 blocks: every block's partial against float64 over the contiguous chunk it owns
    (block 0 also the tail behind the last whole vector), idle blocks exactly 0."""
    lib = _lib()
    _dt, _stream = _abi()
    V = VEC[dtype]
    nv = n // V
    assert n % V, "a tail for block 0"
    x = torch.randn(n, device=DEV, generator=_gen(n % 997)).to(dtype)
    x[nv * V:] = SUMSQ_TAIL
    part = torch.full((SUMSQ_NBLK,), NAN, dtype=torch.float32, device=DEV)
    assert lib.rpo_sumsq_partial(x.data_ptr(), n, _dt(x), part.data_ptr(), SUMSQ_NBLK, _stream(x)) == 0
    torch.cuda.synchronize()
    per = _cdiv(_cdiv(nv, SUMSQ_NBLK), 256) * 256       # vectors per block, in whole 256-vector rows (sumsq_kernel)
    active = _cdiv(nv, per)
    ref = torch.zeros(SUMSQ_NBLK, dtype=torch.float64, device=DEV)
    body = x[:nv * V]
    step = max(1, (1 << 25) // (per * V))
    for b0 in range(0, active, step):
        b1 = min(active, b0 + step)
        full = min(b1, nv // per)
        if full > b0:
            ref[b0:full] = body[b0 * per * V:full * per * V].to(torch.float64).square().view(full - b0, per * V).sum(1)
        if b1 > full:                                     # the last active block's partial chunk
            ref[full] = body[full * per * V:].to(torch.float64).square().sum()
    tail = x[nv * V:].to(torch.float64).square().sum()
    ref[0] += tail
    # one thread adds per V / 1024 elements per accumulator (4 accumulators, 4 vectors per trip) and up to 3 V more in the
    # remainder loop, then 2 adds to combine, 6 butterfly steps, 2 steps over the 4 waves, and the tail's fma: a sum of
    # non-negative terms, relative error <= (per V / 1024 + 3 V + 12) u
    c = per * V / 1024 + 3 * V + 12
    assert tail > 100 * c * U * ref[0], "the tail must be visible above block 0's bound"
    check_elem("sumsq partials", part, ref, c * U * ref)
    if active < SUMSQ_NBLK:
        assert (part[active:] == 0).all()
