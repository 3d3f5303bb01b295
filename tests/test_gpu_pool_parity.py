"""float64 parity of every path of rankpo_amd/csrc/pool_normalize.hip in bf16, fp16 and f32 storage: the wave kernel at NV = 1, 2,
4, 8 with full and partial last vectors, the block kernel's one-vector, vector-loop and scalar row paths (launches that mix aligned
and unaligned pooled rows included), both argmin scans of both kernels at their lane, wave and thread-stride seams and on 64-bit
mask values, every dispatch edge from both sides, both pooling modes with and without the normalisation, and the backward's two
fills at their block seams with all three output combinations (dh, drow, both) and the largest grid.  tests/pool_parity_util.py
holds the tables, the builders, the float64 references and the error rules with their derivations; tests/test_pool_parity_host.py
proves on the CPU that the tables reach every instance and edge, that the regimes are what they claim and that a correct kernel
can meet every rule.

The forward and backward cases go through the C ABI.  A forward case reads overlapping windows of one small buffer (sn = sl = ld),
so N >= 512, L = 1024, d = 4096 costs a few MB; everything outside the pooled rows holds a sentinel and the whole buffer must come
back unchanged.  Every output (out, idx_out, norm_out, dh, drow) is allocated with guards on both sides and pre-filled (NaN, or a
marker for the indices); the guards must keep their fill, and every element of dh off the pooled rows must be +0 by bit pattern.
Refused calls must return their code before any launch: their buffers are far smaller than the refused shape and must not change.

Out of scope: L (d / V) >= 2^31 in the backward (the scalar fill's other entry condition) needs a 32 GB gradient.

Measured on an MI355X, ratio to the bound (ulps for the 16-bit forward), range over the cases of each storage dtype (the tests print
them per case):
  index: exact in all 156 forward cases.  norm_out against its derived bound: bf16 <= 0.15, fp16 <= 0.17, f32 0.02-0.08.
  forward, 16-bit (ulps): 0.45-0.50 in every regime (bf16 `offset` 0.16-0.50, fp16 `above_eps` 0.17-0.50: short rows whose values fall
    on the grid), `zero` 0; the copies bit-exact.
  forward, f32 (err / (1.5 control + 2 ulp)): random 0.20-0.36, offset 0.21-0.34, outlier 0.09-0.46, large 0.16-0.37, below_eps
    0.17-0.18, above_eps 0.09-0.33.
  backward, err / bound, g random | parallel | orthogonal:
    bf16  random 0.13-0.20 | 0.11-0.14 | 0.16;  offset 0.14-0.16 | 0.19-0.38 | 0.08-0.16;  outlier 0.16-0.17 | <= 0.002 | 0.16;
          large 0.13-0.17 | 0.11-0.15 | 0.12-0.17;  above_eps 0.13-0.15 | 0.08-0.14 | 0.13-0.16;  zero / below_eps 0.48-0.49 ulp.
    fp16  random 0.14-0.22 | 0.08-0.09 | 0.16;  offset 0.13-0.14 | 0.10-0.21 | 0.08-0.16;  outlier 0.18-0.20 | <= 0.02 | 0.19-0.21;
          large 0.21-0.22 | 0.01-0.37 | 0.21-0.24;  above_eps 0.14-0.16 | 0.18-0.26 | 0.14-0.16;  zero: every element +-inf or 0, as
          the float64 quotient rounds.
    f32   random 0.21-0.57 | 0.01-0.02 | 0.14-0.33;  offset 0.24-0.43 | 0.01 | 0.12-0.36;  outlier 0.22-0.39 | 0.02-0.06 | 0.11-0.16;
          large 0.19-0.33 | 0.01 | 0.15-0.39;  above_eps 0.22-0.47 | 0.01 | 0.16-0.23;  zero / below_eps 0.16-0.18 | <= 0.01 | 0.16-0.18.
    The 65535-sample grid (exact `axis` rows) and every normalize = 0 case: bit-exact.  ops.pool_normalize: forward 0.50 ulp,
    backward 0.15-0.16.
  dh and drow agreed bit for bit in every output combination, every off-row element of dh was +0, no guard and no input changed.
Found by these tests and fixed in the same change: the f32-storage forward summed the squares in f32, and on `outlier` rows (one
element 2^12 x the rest, so y is just below 1 there, where an f32 ulp is finest) that element came out 3 ulps off while the stock
F.normalize stayed within one: err / bound 1.42 (wave kernel NV 8, d = 2048) and 1.37 (block kernel, CLS, d = 768).  The f32
instantiations now sum in f64 (pool_normalize.hip, SsAcc); the 16-bit instantiations and the backward compile to the same code as
before.  The two suspects the suite was written for -- the int64 lane shuffles and compares of the two argmin routines, and the
per-block alignment decision when sl makes alternate rows unaligned -- hold on every case.
"""
import pytest
import torch

import pool_parity_util as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64                   # elements on both sides of every output: a multiple of V, so the guarded view stays 16-byte aligned
IDX_FILL = -7777


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


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dt(dtype):
    return ops()._dt(torch.empty(0, dtype=dtype))


def _guarded(n, dtype, fill, off=0):
    """A device buffer of GUARD + off + n + GUARD elements filled with `fill`; -> (buffer, first element of the payload)."""
    buf = torch.full((GUARD + off + n + GUARD,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, GUARD + off


def _ptr(buf, first):
    return buf.data_ptr() + first * buf.element_size()


def _untouched(buf, first, n, name):
    """Both guards of a buffer still hold their fill (NaN for floating buffers, IDX_FILL for the indices)."""
    for part in (buf[:first], buf[first + n:]):
        ok = torch.isnan(part).all() if buf.dtype.is_floating_point else (part == IDX_FILL).all()
        assert bool(ok), f"{name}: written outside its extent"


def _fwd_call(dtype, h_ptr, sn, sl, mask_ptr, N, L, d, mode, normalize, out_off=0):
    """rpo_pool_normalize_fwd into guarded, pre-filled outputs -> (out [N, d], idx [N], norm [N]) on the device."""
    ob, o0 = _guarded(N * d, dtype, float("nan"), out_off)
    ib, i0 = _guarded(N, torch.int32, IDX_FILL)
    nb, n0 = _guarded(N, torch.float32, float("nan"))
    rc = lib().rpo_pool_normalize_fwd(h_ptr, sn, sl, mask_ptr, N, L, d, _dt(dtype), mode, normalize, P.EPS, _ptr(ob, o0),
                                      _ptr(ib, i0), _ptr(nb, n0), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _untouched(ob, o0, N * d, "out")
    _untouched(ib, i0, N, "idx_out")
    _untouched(nb, n0, N, "norm_out")
    return ob[o0:o0 + N * d].view(N, d), ib[i0:i0 + N], nb[n0:n0 + N]


# ------------------------------------------------------------------------------------------------
# forward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.FWD_CASES, ids=[c["name"] for c in P.FWD_CASES])
def test_forward_parity(case):
    dtype, N, L, d = case["dtype"], case["N"], case["L"], case["d"]
    b = P.build_fwd(case)
    kernel, rows, arg = P.fwd_paths(case, b)
    h = b["h"].to(DEV)
    mask = None if b["mask"] is None else b["mask"].to(DEV)
    assert h.data_ptr() % 16 == 0 and (mask is None or mask.data_ptr() % 16 == 0)
    # every row the kernel may form lies inside the buffer
    assert case["h_off"] + (N - 1) * case["sn"] + (L - 1) * case["sl"] + d <= h.numel()
    assert mask is None or case["mask_off"] + N * L == mask.numel()
    out, idx, norm = _fwd_call(dtype, _ptr(h, case["h_off"]), case["sn"], case["sl"], None if mask is None else _ptr(mask, case["mask_off"]),
                               N, L, d, case["mode"], case["normalize"], case["out_off"])
    assert torch.equal(P.bits(h.cpu()), P.bits(b["h"])), "h was written"
    assert mask is None or torch.equal(mask.cpu(), b["mask"]), "the mask was written"
    ctrl = P.fwd_control_f32(b["x"].to(DEV), case["normalize"]).cpu() if dtype == torch.float32 else None
    worst = P.check_fwd(case, b, out.cpu(), idx.cpu(), norm.cpu(), ctrl)
    print(f"\n{case['name']}: {kernel} rows {sorted(set(rows))} argmin {sorted(set(arg))}: worst ratio {worst}")


# ------------------------------------------------------------------------------------------------
# backward
# ------------------------------------------------------------------------------------------------
def _bwd_call(dtype, g, y, idx, norm, N, L, d, normalize, want_dh, want_drow, dh_off):
    """rpo_pool_normalize_bwd into guarded NaN-filled outputs -> (dh [N, L, d] or None, drow [N, d] or None) on the device."""
    hb, h0 = _guarded(N * L * d, dtype, float("nan"), dh_off) if want_dh else (None, 0)
    rb, r0 = _guarded(N * d, dtype, float("nan")) if want_drow else (None, 0)
    rc = lib().rpo_pool_normalize_bwd(g.data_ptr(), y.data_ptr(), idx.data_ptr(), norm.data_ptr(), N, L, d, _dt(dtype), normalize,
                                      P.EPS, _ptr(hb, h0) if want_dh else None, _ptr(rb, r0) if want_drow else None, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    dh = drow = None
    if want_dh:
        _untouched(hb, h0, N * L * d, "dh")
        dh = hb[h0:h0 + N * L * d].view(N, L, d)
    if want_drow:
        _untouched(rb, r0, N * d, "drow")
        drow = rb[r0:r0 + N * d].view(N, d)
    return dh, drow


def _split_dh(dh, idx):
    """(the pooled rows [N, d], whether every other element is +0 by bit pattern)."""
    N, L, d = dh.shape
    n = torch.arange(N, device=dh.device)
    rows = dh[n, idx.long()].clone()
    bits = P.bits(dh).clone()
    bits[n, idx.long()] = 0
    return rows, not bool(bits.any())


@pytest.mark.parametrize("case", P.BWD_CASES, ids=[c["name"] for c in P.BWD_CASES])
def test_backward_parity(case):
    dtype, N, L, d = case["dtype"], case["N"], case["L"], case["d"]
    b = P.build_bwd(case)
    x, g, idx = b["x"].to(DEV), b["g"].to(DEV), b["idx"].to(DEV)
    # out and norm from the forward kernel on the same rows (CLS mode on [N, 1, d]); idx is the case's own
    y, _, norm = _fwd_call(dtype, x.data_ptr(), d, d, None, N, 1, d, P.POOL_CLS, case["normalize"])
    y, norm = y.contiguous(), norm.contiguous()
    dh_a, _ = _bwd_call(dtype, g, y, idx, norm, N, L, d, case["normalize"], True, False, case["dh_off"])
    _, drow_b = _bwd_call(dtype, g, y, idx, norm, N, L, d, case["normalize"], False, True, case["dh_off"])
    dh_c, drow_c = _bwd_call(dtype, g, y, idx, norm, N, L, d, case["normalize"], True, True, case["dh_off"])
    for name, dh in (("dh only", dh_a), ("both", dh_c)):
        rows, clean = _split_dh(dh, idx)
        assert clean, f"{case['name']} ({name}): dh is not +0 off the pooled rows"
        assert torch.equal(P.bits(rows), P.bits(drow_c)), f"{case['name']} ({name}): dh and drow differ"
    assert torch.equal(P.bits(drow_b), P.bits(drow_c)), f"{case['name']}: drow alone differs"
    assert torch.equal(g.cpu(), b["g"]) and torch.equal(idx.cpu(), b["idx"])
    ctrl = P.bwd_control(x, g, case["normalize"]).cpu()
    worst = P.check_bwd(case, b, drow_c.cpu(), ctrl)
    print(f"\n{case['name']}: fill {P.bwd_fill(dtype, L, d, True, case['dh_off'])} g {case['g']}: worst err / bound {worst}")


# ------------------------------------------------------------------------------------------------
# the autograd wrapper
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_ops_pool_normalize_autograd(dtype):
    """ops.pool_normalize: h with a non-unit inner stride (the wrapper's .contiguous()), return_index, the gradient arriving
    non-contiguous, and CLS with mask = None."""
    N, L, d = 5, 7, 264
    gen = torch.Generator().manual_seed(11)
    case = {"name": f"{P.TAG[dtype]}-ops", "dtype": dtype, "N": N, "L": L, "d": d, "normalize": 1, "g": "random", "mask": True,
            "mode": P.POOL_LAST}
    mk, _ = P.build_masks(case)
    idx_ref = torch.from_numpy(P.R.last_token_index(mk).astype("int64"))
    wide = torch.randn(N, L, 2 * d, generator=gen).to(dtype).to(DEV).requires_grad_(True)
    h = wide[:, :, ::2]
    assert h.stride(2) == 2
    g = torch.randn(N, 2 * d, generator=gen).to(dtype).to(DEV)[:, 1::2]
    assert not g.is_contiguous()
    for mode, mask, idx_want in (("last", torch.from_numpy(mk).to(DEV), idx_ref), ("cls", None, torch.zeros(N, dtype=torch.int64))):
        wide.grad = None
        e, idx = ops().pool_normalize(h, mask, mode, True, return_index=True)
        x = h.detach()[torch.arange(N, device=DEV), idx_want.to(DEV)].cpu()
        b = {"idx": idx_want, "x": x, "regime": ["random"] * N, "g": g.cpu().contiguous()}
        out_ref, n64 = P.fwd64(x, 1)
        assert torch.equal(idx.cpu().long(), idx_want), (mode, idx.tolist())
        r = float(P.one_ulp_ratio(e.detach().cpu(), out_ref, dtype, P.MIN_NORMAL[dtype]).max())
        assert r <= 1.0, (mode, r)
        e.backward(g)
        dwide = wide.grad
        assert not bool(P.bits(dwide[:, :, 1::2]).any()), "the columns h does not view got a gradient"
        rows, clean = _split_dh(dwide[:, :, ::2].contiguous(), idx_want.to(DEV))
        assert clean, mode
        worst = P.check_bwd(case, b, rows.cpu(), P.bwd_control(x.to(DEV), g.contiguous(), 1).cpu())
        print(f"\nops.pool_normalize {mode} {P.TAG[dtype]}: forward {r:.3f} ulp, backward err / bound {worst}")
    # the production CLS call: [N, 1, d], mask = None
    h1 = torch.randn(N, 1, d, generator=gen).to(dtype).to(DEV)
    e1 = ops().pool_normalize(h1, None, "cls", True)
    assert float(P.one_ulp_ratio(e1.cpu(), P.fwd64(h1[:, 0].cpu(), 1)[0], dtype, P.MIN_NORMAL[dtype]).max()) <= 1.0


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_refused_calls_return_before_any_launch():
    """Every refusal returns its code with buffers of 256 bytes standing in for shapes of gigabytes: no byte may change."""
    L_ = lib()
    inv, uns = P.RPO_ERR_INVALID_ARG, P.RPO_ERR_UNSUPPORTED
    names = ("h", "mask", "out", "idx", "norm", "g", "dh", "drow")
    bufs = {n: torch.full((256,), 0x5A, dtype=torch.uint8, device=DEV) for n in names}
    p = {n: t.data_ptr() for n, t in bufs.items()}
    bf = _dt(torch.bfloat16)
    big = 1 << 20

    def fwd(h=p["h"], mask=p["mask"], N=big, L=big, d=big, dt=bf, mode=P.POOL_LAST, out=p["out"], idx=p["idx"], norm=p["norm"]):
        return L_.rpo_pool_normalize_fwd(h, big * big, big, mask, N, L, d, dt, mode, 1, P.EPS, out, idx, norm, _stream())

    def bwd(g=p["g"], y=p["out"], idx=p["idx"], norm=p["norm"], N=1000, L=big, d=big, dt=bf, dh=p["dh"], drow=p["drow"]):
        return L_.rpo_pool_normalize_bwd(g, y, idx, norm, N, L, d, dt, 1, P.EPS, dh, drow, _stream())

    got = {
        "bwd N = 65536": (bwd(N=65536), uns), "bwd N = 65536, drow only": (bwd(N=65536, dh=None), uns),
        "pool_mode = 2": (fwd(mode=2), inv), "pool_mode = -1": (fwd(mode=-1), inv),
        "last-token pooling without a mask": (fwd(mask=None), inv),
        "fwd h = NULL": (fwd(h=None), inv), "fwd out = NULL": (fwd(out=None), inv), "fwd idx_out = NULL": (fwd(idx=None), inv),
        "fwd norm_out = NULL": (fwd(norm=None), inv), "fwd dtype 7": (fwd(dt=7), inv),
        "bwd dh = drow = NULL": (bwd(dh=None, drow=None), inv), "bwd grad_out = NULL": (bwd(g=None), inv),
        "bwd out = NULL": (bwd(y=None), inv), "bwd idx = NULL": (bwd(idx=None), inv), "bwd norm = NULL": (bwd(norm=None), inv),
        "bwd dtype 7": (bwd(dt=7), inv),
        "fwd L > INT32_MAX": (fwd(L=1 << 31), uns), "fwd N > INT32_MAX": (fwd(N=1 << 31), uns), "bwd L > INT32_MAX": (bwd(L=1 << 31), uns),
    }
    for v in (0, -1):
        for k in ("N", "L", "d"):
            got[f"fwd {k} = {v}"] = (fwd(**{k: v}), inv)
            got[f"bwd {k} = {v}"] = (bwd(**{k: v}), inv)
    torch.cuda.synchronize()
    wrong = {k: v for k, v in got.items() if v[0] != v[1]}
    assert not wrong, wrong
    for n, t in bufs.items():
        assert bool((t == 0x5A).all()), f"a refused call wrote {n}"
