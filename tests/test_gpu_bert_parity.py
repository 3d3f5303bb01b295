"""float64 parity of every 16-bit kernel of rankpo_amd/csrc/bert_ops.hip at every row width and on hard inputs: the LayerNorm family
at every NV (vectors per lane) with a full and a partially filled last vector, the LayerNorm backward at the row counts where waves
own no row, one row or two, the dropout-fused row kernels at every NV (4 and 8 had never run), GELU beyond one grid pass, and
the attention forward and backward per (sequence, head) block on the second tile boundary, on cross shapes and in the
saturated, identical-key, spike and offset regimes.  tests/bert_parity_util.py holds the tables, the builders, the float64
references and the error rules with their derivations (every extra term and the lse bound); tests/test_bert_parity_host.py proves on the CPU that the tables reach every
template instance, that the regimes are what they claim and that a correct kernel can meet the bounds.

Error rule, the project's own: error <= 1.5 x the error of the stock PyTorch op in the same storage dtype + 2 U, per row, per
(sequence, head) block or per tensor against that unit's own reference norm; the one-ulp rule with its floors for the LayerNorm,
embedding and GELU forwards; the dropout-fused row kernels bit for bit against the unfused op through the dumped mask.  out and dv
never get an extra term; dq and dk get 2 U ||abs|| in the `saturated` and `spike` regimes and for one-key sequences, U ||abs_delta||
under dropout elsewhere, and nothing in `random`, `identical_keys` and `offset` without dropout.  Every output buffer is allocated
NaN-filled; every row-strided operand that goes through a C entry has padding columns whose canary must survive.

Measured on an MI355X, max err / bound (ulps for the one-ulp rule), range over the cases of each test (the tests print them).  A
ratio of 0.666 = 1 / 1.5 is an error EQUAL to the control's, on a block or element whose exact value lies below what the storage
format holds and which kernel and control both return as 0.
  add_layernorm forward (ulps): random 0.50, offset 0.48-0.70, outlier 0.48-0.50, tiny_var 0.46-0.50, const 0 (y = beta bit for
  bit); layernorm_bwd ds 0.16-0.24 in every regime, width and row count, dgamma / dbeta <= 0.001 (f32 partial sums against a
  control that rounds to 16 bits).  bert_embed_ln forward 0.45-0.67 ulp; word / pos / type gradients 0.20-0.28, gamma / beta
  0.16-0.23.  GELU forward 0.50-0.52 ulp; backward 0.09-0.67 (0.666 on fp16 elements below the subnormals).
  Attention training forward + backward, out / dq / dk / dv, p = 0 (control: SDPA) and p = 0.1 (control: SDPA's error carried over;
  the eager replay on the fp16 blocks whose kept probabilities are all subnormal) apart:
    random          p 0: 0.22-0.25 / 0.32-0.61 / 0.32-0.61 / 0.23-0.25     p 0.1: 0.25-0.28 / 0.20-0.24 / 0.20-0.24 / 0.26-0.28
    offset          p 0: 0.23-0.25 / 0.44-0.57 / 0.42-0.59 / 0.22-0.26     p 0.1: 0.24-0.27 / 0.17-0.29 / 0.20-0.38 / 0.24-0.28
    identical_keys  p 0: 0.19-0.20 / 0.67-0.69 / 0.32-0.58 / 0.23-0.26     p 0.1: 0.22-0.27 / 0.21-0.57 / 0.20-0.22 / 0.25-0.28
    saturated bf16  p 0: 0.18-0.19 / 0.06-0.08 / 0.07-0.08 / 0.22-0.26     p 0.1: 0.37-0.46 / 0.10-0.11 / 0.10-0.11 / 0.34-0.47
    saturated fp16  p 0: 0.18-0.19 / 0.06      / 0.06-0.08 / 0.24-0.25     p 0.1: 0.26-0.74 / 0.06-0.75 / 0.06-0.77 / 0.33-0.81
    spike bf16      p 0: 0    / 0    / 0    / 0.18-0.19                    p 0.1: 0.33-0.37 / 0.07-0.13 / 0.07-0.13 / 0.33-0.35
    spike fp16      p 0: 0    / 0    / 0    / 0.18                         p 0.1: 0.666 in all four
  One ratio exceeds 0.8: dv 0.805 (out 0.74, dq 0.75, dk 0.77) of fp16 `saturated` at p = 0.1, head dim 32, on the one-query block
  of the cross case (100 keys) whose winning key the mask drops: its largest kept probability is 1.4e-7, an fp16 subnormal of two
  significant bits, in the kernel and in the eager replay that is this block's control; no other block of the regime exceeds 0.67.  The spike fp16 p = 0.1 figures are the same kind of block with every kept probability below fp16's range.
  The non-training forward: out 0.18-0.25 (spike: 0, out = the winner's V row exactly).  lse against its derived f32 bound:
  0.015-0.095.
Found by these tests and fixed in the same change: gelu_bwd_kernel returned du = 0 where phi(u) is a subnormal f32 (|u| > 13.2; the
5470 x 3072 case holds several dozen such u), a 100 % error on values bf16 still holds (1e-38 .. 1e-40).
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bert_parity_util as B
import hidden_dropout_util as HU
from test_gpu_hidden_dropout import StandIn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [B.TAG[t] for t in B.DTYPES]
CANARY = -24576.0            # exact in bf16 and fp16


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


def _padded(x, pad):
    """x [rows, d] copied into the first d columns of a [rows, d + pad] device buffer whose other columns hold the canary."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), CANARY, dtype=x.dtype, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf, buf[:, :x.shape[1]]


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _nan_padded(rows, d, pad, dtype):
    buf = _nan((rows, d + pad), dtype)
    return buf, buf[:, :d]


def _intact(d, inputs=(), outputs=()):
    """The padding columns of input buffers still hold the canary, and only it; those of output buffers their NaN, and only it."""
    for buf in inputs:
        assert buf.shape[1] > d and bool((buf[:, d:] == CANARY).all()), "the padding of an input was written"
    for buf in outputs:
        assert buf.shape[1] > d and bool(torch.isnan(buf[:, d:]).all()), "the padding of an output was written"


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


# ------------------------------------------------------------------------------------------------
# LayerNorm family
# ------------------------------------------------------------------------------------------------
def _ln_bwd(s, gamma, dy, eps, extra_blocks=0):
    """rpo_layernorm_bwd through the C entry on row-strided s / dy into a NaN-filled row-strided ds and NaN-filled partials with
    `extra_blocks` rows more than the entry writes.  -> (ds buffer, ds view, partials [2, nb + extra, d], nb)."""
    o, L = ops(), lib()
    rows, d = s.shape
    nb = L.rpo_layernorm_bwd_blocks(rows)
    assert nb == B.rpo_layernorm_bwd_blocks(rows)
    ds_buf, ds = _nan_padded(rows, d, 24, s.dtype)
    part = _nan((2, nb + extra_blocks, d), torch.float32)
    assert L.rpo_layernorm_bwd(s.data_ptr(), s.stride(0), gamma.data_ptr(), dy.data_ptr(), dy.stride(0), eps, ds.data_ptr(),
                               ds.stride(0), part[0].data_ptr(), part[1].data_ptr(), rows, d, o._dt(s), _stream()) == 0
    return ds_buf, ds, part, nb


def _check_ln_bwd(s, gamma, beta, dy, eps, ds, dg, db, label, worst):
    """ds per row, dgamma / dbeta per tensor, against float64 from the stored s by the control rule."""
    dtype = s.dtype
    assert torch.isfinite(ds.float()).all() and torch.isfinite(dg).all() and torch.isfinite(db).all(), label
    ds64, dg64, db64 = B.ln_bwd64(s, gamma, dy, eps)
    _, cds, cdg, cdb = B.layernorm_control(s.contiguous(), gamma, beta, dy.contiguous(), eps)
    err = (ds.double() - ds64).norm(dim=-1)
    bound = B.rule_bound((cds.double() - ds64).norm(dim=-1), ds64.norm(dim=-1), dtype)
    worst["ds"] = max(worst.get("ds", 0.0), round(float((err / bound.clamp_min(1e-300)).max()), 3))
    assert (err <= bound).all(), (label, "ds", err.tolist(), bound.tolist())
    for name, got, ctrl, ref in (("dgamma", dg, cdg, dg64), ("dbeta", db, cdb, db64)):
        e, bnd = float((got.double() - ref).norm()), float(B.rule_bound((ctrl.double() - ref).norm(), ref.norm(), dtype))
        worst[name] = max(worst.get(name, 0.0), round(e / max(bnd, 1e-300), 3))
        assert e <= bnd, (label, name, e, bnd)


def _bwd_eps(regime):
    return 1e-5 if regime in B.LN_DEGENERATE else 1e-12       # at 1e-12 the exact ds of a constant row overflows fp16


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("d", B.ROW_WIDTHS)
def test_add_layernorm_forward_and_backward_every_width_and_regime(dtype, d):
    o, L = ops(), lib()
    rows, worst = B.LN_ROWS, {}
    for regime in B.LN_REGIMES:
        c = _dev(B.ln_case(regime, rows, d, dtype))
        label = (regime, d, B.TAG[dtype])
        g, be = c["gamma"], c["beta"]
        a_buf, a = _padded(c["a"], 8)
        b_buf, b = _padded(c["b"], 16)
        x_buf, x = _padded(c["x"], 40)
        dy_buf, dy = _padded(c["dy"], 48)
        y_buf, y = _nan_padded(rows, d, 24, dtype)
        # forward, a + b and b = None
        assert o.add_layernorm(a, b, g, be, 1e-12, out=y) is y
        r = B.one_ulp_ratio(y, B.ln_fwd64(c["s"], g, be, 1e-12), dtype, B.LN_FLOOR)
        y1_buf, y1 = _nan_padded(rows, d, 8, dtype)
        o.add_layernorm(x, None, g, be, 1e-12, out=y1)
        r1 = B.one_ulp_ratio(y1, B.ln_fwd64(c["x"], g, be, 1e-12), dtype, B.LN_FLOOR)
        worst[f"fwd {regime}"] = round(max(r, r1), 3)
        assert torch.isfinite(y.float()).all() and r <= 1.0 and r1 <= 1.0, (label, r, r1)
        if regime == "const":
            assert torch.equal(y, be.expand_as(y)) and torch.equal(y1, be.expand_as(y1)), label      # y = beta bit for bit
        # the training forward: y bit-equal to the forward, s the rounded sum
        y2_buf, y2 = _nan_padded(rows, d, 16, dtype)
        s_buf, s = _nan_padded(rows, d, 32, dtype)
        assert L.rpo_add_layernorm_train_fwd(a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), g.data_ptr(), be.data_ptr(), 1e-12,
                                             y2.data_ptr(), y2.stride(0), s.data_ptr(), s.stride(0), rows, d, o._dt(a), _stream()) == 0
        assert torch.equal(y2, y) and torch.equal(s, c["s"]), label
        # backward from the stored s
        eps = _bwd_eps(regime)
        ds_buf, ds, part, nb = _ln_bwd(s, g, dy, eps)
        sums = part.sum(1)
        w = {}
        _check_ln_bwd(c["s"], g, be, c["dy"], eps, ds, sums[0], sums[1], label, w)
        worst[f"bwd {regime}"] = w
        _intact(d, (a_buf, b_buf, x_buf, dy_buf), (y_buf, y1_buf, y2_buf, s_buf, ds_buf))
    print(f"\nadd_layernorm d{d} NV{B.row_vectors(d)} {B.last_vector(d)} {B.TAG[dtype]}: fwd in ulps, bwd err / bound {worst}")


def _embed64_grads(c, with_types, dtype, eps, pad):
    """float64 gradients of the embedding + LayerNorm with the forward's two roundings passed straight through."""
    w64, p64, t64, g64, b64 = (c[k].detach().double().requires_grad_(True) for k in ("word", "pos_t", "type_t", "gamma", "beta"))
    T, d = len(c["ids"]), c["word"].shape[1]
    w_rows = F.embedding(c["ids"].long(), w64, padding_idx=pad)
    t_rows = t64[c["tts"].long()] if with_types else t64[0].expand(T, d)
    s = w_rows + t_rows
    s = (s.to(dtype).double() - s).detach() + s
    s = s + p64[c["pos"].long()]
    s = (s.to(dtype).double() - s).detach() + s
    F.layer_norm(s, (d,), g64, b64, eps).backward(c["dy"].double())
    return [t.grad for t in (w64, p64, t64, g64, b64)]


def _embed_ctrl_grads(c, with_types, eps, pad):
    """The stock ops in the storage dtype under autograd: the control."""
    w, pt, tt, g, be = (c[k].detach().clone().requires_grad_(True) for k in ("word", "pos_t", "type_t", "gamma", "beta"))
    T, d = len(c["ids"]), c["word"].shape[1]
    t_rows = tt[c["tts"].long()] if with_types else tt[0].expand(T, d)
    s = (F.embedding(c["ids"].long(), w, padding_idx=pad) + t_rows) + pt[c["pos"].long()]
    F.layer_norm(s, (d,), g, be, eps).backward(c["dy"])
    return [t.grad for t in (w, pt, tt, g, be)]


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("d", B.ROW_WIDTHS)
def test_bert_embed_ln_every_width_and_regime(dtype, d):
    o, L = ops(), lib()
    worst = {}
    T, pad = len(B.EMBED_IDS), B.EMBED_PAD
    for regime in B.LN_REGIMES:
        c = _dev(B.embed_case(regime, d, dtype))
        g, be = c["gamma"], c["beta"]
        for with_types in (True, False):
            label = (regime, d, B.TAG[dtype], with_types)
            tts = c["tts"] if with_types else None
            s_ref = B.embed_sum(c, with_types, dtype)
            y = o.bert_embed_ln(c["ids"], c["pos"], tts, c["word"], c["type_t"], c["pos_t"], g, be, 1e-12)
            r = B.one_ulp_ratio(y, B.ln_fwd64(s_ref, g, be, 1e-12), dtype, B.LN_FLOOR)
            worst[f"fwd {regime}"] = max(worst.get(f"fwd {regime}", 0.0), round(r, 3))
            assert torch.isfinite(y.float()).all() and r <= 1.0, (label, r)
            # the training entry on row-strided NaN-filled outputs: y bit-equal, s the rounded sum
            y_buf, y2 = _nan_padded(T, d, 8, dtype)
            s_buf, s = _nan_padded(T, d, 16, dtype)
            assert L.rpo_bert_embed_ln_train_fwd(c["ids"].data_ptr(), tts.data_ptr() if with_types else None, c["pos"].data_ptr(), T,
                                                 c["word"].data_ptr(), B.EMBED_V, c["type_t"].data_ptr(), B.EMBED_TT,
                                                 c["pos_t"].data_ptr(), B.EMBED_P, g.data_ptr(), be.data_ptr(), 1e-12, y2.data_ptr(),
                                                 y2.stride(0), s.data_ptr(), s.stride(0), d, o._dt(y), _stream()) == 0
            assert torch.equal(y2, y) and torch.equal(s, s_ref), label
            _intact(d, (), (y_buf, s_buf))
            # under autograd with a padding_idx: every table and LayerNorm parameter per tensor by the control rule
            eps = 1e-5
            leaves = [c[k].detach().clone().requires_grad_(True) for k in ("word", "type_t", "pos_t", "gamma", "beta")]
            yt = o.bert_embed_ln_train(c["ids"], c["pos"], tts, *leaves, eps, pad)
            assert torch.equal(yt, o.bert_embed_ln(c["ids"], c["pos"], tts, c["word"], c["type_t"], c["pos_t"], g, be, eps)), label
            yt.backward(c["dy"])
            got = [leaves[i].grad for i in (0, 2, 1, 3, 4)]                      # word, pos, type, gamma, beta
            assert float(got[0][pad].abs().max()) == 0.0, label                  # padding_idx keeps its zero gradient
            ref, ctrl = _embed64_grads(c, with_types, dtype, eps, pad), _embed_ctrl_grads(c, with_types, eps, pad)
            for name, gg, rr, cc in zip(("word", "pos", "type", "gamma", "beta"), got, ref, ctrl):
                assert torch.isfinite(gg.float()).all(), (label, name)
                e, bnd = float((gg.double() - rr).norm()), float(B.rule_bound((cc.double() - rr).norm(), rr.norm(), dtype))
                worst[f"d{name}"] = max(worst.get(f"d{name}", 0.0), round(e / max(bnd, 1e-300), 3))
                assert e <= bnd, (label, name, e, bnd)
    print(f"\nbert_embed_ln d{d} NV{B.row_vectors(d)} {B.last_vector(d)} {B.TAG[dtype]}: fwd in ulps, grads err / bound {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("rows", B.LN_BWD_ROWS)
def test_layernorm_bwd_row_counts(dtype, rows):
    """Fewer rows than the block's 4 waves, one row per wave up to the capped grid, two rows for one wave: exactly
    rpo_layernorm_bwd_blocks(rows) partial rows are written, their sum meets the rule, and a second call gives the same bits."""
    worst = {}
    for d in [B.LN_BWD_WIDTH] + ([B.LN_BWD_WIDE] if rows in B.LN_BWD_SMALL_ROWS else []):
        c = _dev(B.ln_case("random", rows, d, dtype))
        s_buf, s = _padded(c["s"], 8)
        dy_buf, dy = _padded(c["dy"], 16)
        ds_buf, ds, part, nb = _ln_bwd(s, c["gamma"], dy, 1e-12, extra_blocks=3)
        assert nb == B.rpo_layernorm_bwd_blocks(rows) and torch.isfinite(part[:, :nb]).all() and torch.isnan(part[:, nb:]).all()
        sums = part[:, :nb].sum(1)
        _check_ln_bwd(c["s"], c["gamma"], c["beta"], c["dy"], 1e-12, ds, sums[0], sums[1], (rows, d, B.TAG[dtype]), worst)
        ds_buf2, ds2, part2, _ = _ln_bwd(s, c["gamma"], dy, 1e-12, extra_blocks=3)
        assert torch.equal(ds2, ds) and torch.equal(part2[:, :nb], part[:, :nb])
        _intact(d, (s_buf, dy_buf), (ds_buf, ds_buf2))
    print(f"\nlayernorm_bwd rows {rows} ({B.layernorm_bwd_row_class(rows)}) {B.TAG[dtype]}: err / bound {worst}")


# ------------------------------------------------------------------------------------------------
# dropout-fused row kernels at the widths that were never run
# ------------------------------------------------------------------------------------------------
def _grads(y, dy, *ts):
    for t in ts:
        t.grad = None
    y.backward(dy)
    return [t.grad.clone() for t in ts]


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("p", B.DROP_PS)
def test_dropout_fused_row_kernels_at_wide_rows(dtype, p):
    """rpo_add_layernorm_drop_fwd, rpo_bert_embed_ln_drop_fwd and rpo_layernorm_drop_bwd (site_in and site_out) bit for bit against
    the unfused op through the dumped mask and the stand-in of tests/test_gpu_hidden_dropout.py; the dump against the numpy
    restatement of the keep function: a wrong column group beyond column 1024 shows in either."""
    o = ops()
    eps, rows, pad = 1e-12, B.LN_ROWS, B.EMBED_PAD
    hs = o.bert_hidden_seed(HU.SEEDS[0])
    scale = o.hidden_dropout_scale(p)
    assert scale == HU.scale(p)
    for d in B.DROP_WIDTHS:
        for row0, site in ((0, 0), (1000003, 3)):
            got = o.hidden_dropout_mask(row0, rows, d, p, hs, site, DEV)
            assert np.array_equal(got.cpu().numpy(), HU.hidden_keep(hs, site, row0, rows, d, p)), (d, row0, site)
        label = (B.TAG[dtype], p, d)
        c = _dev(B.ln_case("random", rows, d, dtype))
        a, g, be = (c[k].clone().requires_grad_(True) for k in ("a", "gamma", "beta"))
        big = torch.cat([c["b"], c["b"].flip(1)], 1).contiguous().requires_grad_(True)        # b: a row-strided dense output
        b = big[:, :d]
        for site in (1, 4):
            mask = o.hidden_dropout_mask(0, rows, d, p, hs, site, DEV)
            y1 = o.add_layernorm_train(a, b, g, be, eps, p, hs, site)
            y0 = o.add_layernorm_train(a, StandIn.apply(b, mask, scale), g, be, eps)
            assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0), label
            s1, s0 = y1.grad_fn.saved_tensors[0], y0.grad_fn.saved_tensors[0]
            assert torch.equal(s1, s0) and torch.equal(s0, a.detach() + StandIn.apply(b.detach(), mask, scale)), label
            g1 = _grads(y1, c["dy"], a, big, g, be)
            g0 = _grads(y0, c["dy"], a, big, g, be)
            for name, x1, x0 in zip(("ds", "db", "dgamma", "dbeta"), g1, g0):
                assert torch.isfinite(x1.float()).all() and torch.equal(x1, x0), (name, site) + label
            assert not torch.equal(g1[0], g1[1][:, :d]) and float(g1[1][:, d:].abs().max()) == 0.0
            dropped = mask == 0
            assert torch.equal(s1[dropped], a.detach()[dropped]), label
        # the embedding site: dropout after the LayerNorm, the mask on dy in the backward
        e = _dev(B.embed_case("random", d, dtype))
        T = len(B.EMBED_IDS)
        mask = o.hidden_dropout_mask(0, T, d, p, hs, 0, DEV)
        for tts in (e["tts"], None):
            tabs = [e[k].clone().requires_grad_(True) for k in ("word", "type_t", "pos_t", "gamma", "beta")]
            y1 = o.bert_embed_ln_train(e["ids"], e["pos"], tts, *tabs, eps, pad, p, hs)
            plain = o.bert_embed_ln_train(e["ids"], e["pos"], tts, *tabs, eps, pad)
            y0 = StandIn.apply(plain, mask, scale)
            assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0), label
            s, w = plain.grad_fn.saved_tensors[0], e["gamma"]
            assert torch.equal(y1.grad_fn.saved_tensors[0], s), label
            ds1, none, dg1, db1 = o.layernorm_drop_bwd(s, w, e["dy"], eps, p, hs, site_in=0)
            ds0, dg0, db0 = o.layernorm_bwd(s, w, (e["dy"].float() * scale).to(dtype) * mask.to(dtype), eps)
            assert none is None and torch.equal(ds1, ds0) and torch.equal(dg1, dg0) and torch.equal(db1, db0), label
            assert torch.isfinite(ds1.float()).all() and torch.isfinite(dg1).all() and torch.isfinite(db1).all()
            g1 = _grads(y1, e["dy"], tabs[3], tabs[4])
            g0 = _grads(y0, e["dy"], tabs[3], tabs[4])
            assert torch.equal(g1[0], g0[0]) and torch.equal(g1[1], g0[1]), label


# ------------------------------------------------------------------------------------------------
# GELU
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("rows,cols", B.GELU_SHAPES)
def test_gelu_forward_and_backward_through_the_c_entries(dtype, rows, cols):
    o, L = ops(), lib()
    assert B.gelu_passes(rows, cols) == (2 if rows * cols > 8 * 256 * 8192 else 1)
    u_cpu, dh_cpu = B.gelu_case(rows, cols, dtype)
    u_buf, u = _padded(u_cpu, 8)
    dh_buf, dh = _padded(dh_cpu, 16)
    x_buf, x = _padded(u_cpu, 24)                                # gelu_ works in place on it
    h_buf, h = _nan_padded(rows, cols, 32, dtype)
    du_buf, du = _nan_padded(rows, cols, 40, dtype)
    dt, st = o._dt(u), _stream()
    assert L.rpo_gelu_fwd(x.data_ptr(), rows, cols, x.stride(0), dt, st) == 0
    assert L.rpo_gelu_out_fwd(u.data_ptr(), u.stride(0), h.data_ptr(), h.stride(0), rows, cols, dt, st) == 0
    assert L.rpo_gelu_bwd(u.data_ptr(), u.stride(0), dh.data_ptr(), dh.stride(0), du.data_ptr(), du.stride(0), rows, cols, dt, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(u, u_cpu.to(DEV)) and torch.equal(dh, dh_cpu.to(DEV))
    assert torch.equal(x.view(torch.int16), h.view(torch.int16))                 # gelu_ and gelu_out: the same bits, -0 included
    _intact(cols, (u_buf, dh_buf), (h_buf, du_buf))
    assert bool((x_buf[:, cols:] == CANARY).all())               # gelu_ in place: the padding of its buffer too
    assert torch.isfinite(h.float()).all() and torch.isfinite(du.float()).all()
    fwd = bwd = 0.0
    step = 512                                                   # slices: the float64 copies stay small
    for r0 in range(0, rows, step):
        us, dhs = u[r0:r0 + step].contiguous(), dh[r0:r0 + step].contiguous()
        fwd = max(fwd, B.one_ulp_ratio(h[r0:r0 + step], B.gelu64(us), dtype, B.GELU_FLOOR))
        ref, size = B.gelu_bwd64(us, dhs)
        err = (du[r0:r0 + step].double() - ref).abs()
        # per element; Phi + u phi cancels for u < 0: the floor is relative to |dh| (Phi + |u| phi), the size of what cancels
        bound = 1.5 * (B.gelu_control(us, dhs).double() - ref).abs() + 2 * B.U[dtype] * size
        bad = err > bound
        assert not bad.any(), ("gelu_bwd", rows, cols, r0, int(bad.sum()), float((err - bound).max()))
        pos = bound > 0
        if pos.any():
            bwd = max(bwd, float((err[pos] / bound[pos]).max()))
    print(f"\ngelu {rows}x{cols} {B.TAG[dtype]} ({B.gelu_passes(rows, cols)} grid pass(es)): fwd {fwd:.3f} ulp, bwd err / bound {bwd:.3f}")
    assert fwd <= 1.0, (rows, cols, fwd)


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _tables(lens_q, lens_k):
    o = ops()
    cu_q, cu_k = [0] + np.cumsum(lens_q).tolist(), [0] + np.cumsum(lens_k).tolist()
    return (cu_q, cu_k, torch.tensor(cu_q, dtype=torch.int32, device=DEV), torch.tensor(cu_k, dtype=torch.int32, device=DEV),
            o.bidir_attn_tile_table(lens_q, lens_k, DEV), torch.from_numpy(o.bidir_attn_key_tile_list(lens_q, lens_k)).to(DEV))


def _check_lse(lse, q, k, cu_q, cu_k, scale, hd, label, worst):
    """lse [nh, Tq] against the float64 lse of the stored inputs, inside the derived f32 bound (util docstring)."""
    for n in range(len(cu_q) - 1):
        a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
        _, lse64, s_abs = B.attn_scores64(q[a:b], k[c:e], scale)
        r = (lse[:, a:b].double() - lse64).abs() / B.lse_bound(s_abs, lse64, e - c, hd)
        worst["lse"] = max(worst.get("lse", 0.0), round(float(r.max()), 3))
        assert (r <= 1).all(), (label, "lse", "seq", n, float(r.max()))


def _run_attn(dtype, hd, nh, regime, shape, p, worst, names=("out", "dq", "dk", "dv")):
    """Training forward + backward of one (regime, shape, p): out, lse, dq, dk, dv per (sequence, head) block."""
    o = ops()
    label_s, lens_q, lens_k = shape
    label = f"{regime} {label_s} p{p} hd{hd} {B.TAG[dtype]}"
    scale, d, Tq, Tk = 1.0 / math.sqrt(hd), nh * hd, sum(lens_q), sum(lens_k)
    q, k, v, do = (t.to(DEV) for t in B.attn_case(regime, lens_q, lens_k, nh, hd, dtype))
    if label_s == "self":                                        # q|k|v as column blocks of ONE buffer, and their gradients
        qkv = torch.cat([t.reshape(Tk, d) for t in (q, k, v)], 1).contiguous()
        q, k, v = (qkv[:, j * d:(j + 1) * d].view(Tk, nh, hd) for j in range(3))
        dqkv = _nan((Tk, 3 * d), dtype)
        dq, dk, dv = (dqkv[:, j * d:(j + 1) * d].view(Tk, nh, hd) for j in range(3))
    else:
        dq, dk, dv = _nan((Tq, nh, hd), dtype), _nan((Tk, nh, hd), dtype), _nan((Tk, nh, hd), dtype)
    cu_q, cu_k, cq, ck, qt, kt = _tables(lens_q, lens_k)
    out, lse = o.bidir_attn_train_fwd(q, k, v, cq, ck, qt, scale, p, B.ATTN_SEED)
    if p == 0:
        out0, lse0 = o.bidir_attn_fwd(q, k, v, cq, ck, qt, scale, want_lse=True)
        assert torch.equal(out, out0) and torch.equal(lse, lse0), label         # the training entry without dropout = the forward
    o.bidir_attn_bwd(q, k, v, out, do, lse, cq, ck, qt, kt, scale, dq, dk, dv, p, B.ATTN_SEED)
    torch.cuda.synchronize()
    assert torch.isfinite(lse).all(), label
    _check_lse(lse, q, k, cu_q, cu_k, scale, hd, label, worst)
    for n in range(len(lens_q)):
        a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
        keep = None
        if p > 0:
            keep = o.bidir_attn_dropout_mask(a, c, b - a, e - c, nh, p, B.ATTN_SEED, DEV)
            assert torch.equal(keep.cpu(), B.attn_keep_host(B.ATTN_SEED, a, c, b - a, e - c, nh, p)), (label, n)
        don = do[a:b].view(-1, nh, hd)
        ref, absn, absd = B.attn64(q[a:b], k[c:e], v[c:e], don, scale, keep, p)
        ctrl = B.attn_control(q[a:b], k[c:e], v[c:e], don, scale, keep, p)
        bounds = B.attn_bounds(dtype, regime, e - c, p, ref, ctrl, absn, absd)
        got = (out[a:b].view(-1, nh, hd), dq[a:b], dk[c:e], dv[c:e])
        for name, g, r, bnd in zip(("out", "dq", "dk", "dv"), got, ref, bounds):
            g = g.transpose(0, 1)
            assert torch.isfinite(g.float()).all(), (label, n, name)
            if name not in names:
                continue
            err = B.block_norm(g.double() - r)
            key = f"{name} p{p:g}"        # the two use different controls: reported apart
            worst[key] = max(worst.get(key, 0.0), round(float((err / bnd.clamp_min(1e-300)).max()), 3))
            assert (err <= bnd).all(), (label, "seq", n, "lens", b - a, e - c, name, err.tolist(), bnd.tolist())


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
@pytest.mark.parametrize("regime", B.ATTN_REGIMES)
def test_bidir_attn_train_fwd_and_bwd_per_block(dtype, hd, nh, regime):
    """Self, CLS and cross shapes, with and without dropout.  dq of `identical_keys` without dropout is asserted by the same rule
    in test_identical_keys_dq_without_an_extra_term, where what that comparison rests on is written down."""
    worst = {}
    for shape in B.attn_shapes():
        for p in B.ATTN_PS:
            names = ("out", "dk", "dv") if regime == "identical_keys" and p == 0 else ("out", "dq", "dk", "dv")
            _run_attn(dtype, hd, nh, regime, shape, p, worst, names)
    print(f"\nattention {regime} hd{hd} {B.TAG[dtype]}: max err / bound {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
def test_identical_keys_dq_without_an_extra_term(dtype, hd, nh):
    """dq = scale dS K with every key row equal to k0 is k0 * scale * sum_k dS_k, and sum_k dS_k = 0 exactly: the float64 reference
    is its own rounding noise (~ 1e-16), the kernel's dq is U-sized rounding noise of the 16-bit dS times k0, and so is the
    control's.  The rule gives dq no extra term in this regime, so this compares one noise with 1.5 x another, per block.  It
    holds because the control, a fused SDPA that rounds dS to 16 bits as the kernel does, makes nearly the same errors: measured
    max err / bound 0.667 (hd 32, both dtypes; hd 64 bf16) and 0.689 (hd 64 fp16), the same in two runs.  A control that keeps dS
    in f32 (the CPU's) does not bound it: tests/test_bert_parity_host.py shows the exact cancellation and prints those factors.
    So this test depends on which backend torch's SDPA picks: if it fails after a torch or ROCm upgrade while every other
    attention test here passes, a changed SDPA backward is the first suspect, not the kernel."""
    worst = {}
    for shape in B.attn_shapes():
        _run_attn(dtype, hd, nh, "identical_keys", shape, 0.0, worst, ("dq",))
    print(f"\nattention identical_keys dq hd{hd} {B.TAG[dtype]}: max err / bound {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
def test_bidir_attn_fwd_per_block(dtype, hd, nh):
    """The non-training entry: out per (sequence, head) block by the control rule, no extra term in any regime; lse against the
    float64 lse of the stored inputs inside the derived f32 bound."""
    o = ops()
    scale = 1.0 / math.sqrt(hd)
    for regime in B.ATTN_REGIMES:
        worst = {}
        for label_s, lens_q, lens_k in B.attn_shapes():
            label = f"fwd {regime} {label_s} hd{hd} {B.TAG[dtype]}"
            q, k, v, _ = (t.to(DEV) for t in B.attn_case(regime, lens_q, lens_k, nh, hd, dtype))
            cu_q, cu_k, cq, ck, qt, _ = _tables(lens_q, lens_k)
            out, lse = o.bidir_attn_fwd(q, k, v, cq, ck, qt, scale, want_lse=True)
            out_only, none = o.bidir_attn_fwd(q, k, v, cq, ck, qt, scale)
            assert none is None and torch.equal(out, out_only), label
            torch.cuda.synchronize()
            assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all(), label
            _check_lse(lse, q, k, cu_q, cu_k, scale, hd, label, worst)
            for n in range(len(lens_q)):
                a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
                qs, ks, vs = (t.double().transpose(0, 1) for t in (q[a:b], k[c:e], v[c:e]))
                ref = torch.softmax(qs @ ks.transpose(1, 2) * scale, -1) @ vs
                ctrl = F.scaled_dot_product_attention(*(t.transpose(0, 1)[None] for t in (q[a:b], k[c:e], v[c:e])), scale=scale)[0]
                err = B.block_norm(out[a:b].view(-1, nh, hd).transpose(0, 1).double() - ref)
                bnd = B.rule_bound(B.block_norm(ctrl.double() - ref), B.block_norm(ref), dtype)
                worst["out"] = max(worst.get("out", 0.0), round(float((err / bnd.clamp_min(1e-300)).max()), 3))
                assert (err <= bnd).all(), (label, "seq", n, "lens", b - a, e - c, err.tolist(), bnd.tolist())
        print(f"\nattention forward {regime} hd{hd} {B.TAG[dtype]}: max err / bound {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
def test_bidir_attn_eight_distinct_row_strides(dtype, hd, nh):
    """q, k, v, out, dout, dq, dk, dv in separate allocations of eight different row strides, through the C entries: the same bits as
    the packed layout (which the tests above hold against float64), and every padding column untouched."""
    o, L = ops(), lib()
    scale, d, p = 1.0 / math.sqrt(hd), nh * hd, 0.1
    for label_s, lens_q, lens_k in (B.attn_shapes()[0], B.attn_shapes()[2]):
        Tq, Tk = sum(lens_q), sum(lens_k)
        q, k, v, do = (t.to(DEV) for t in B.attn_case("random", lens_q, lens_k, nh, hd, dtype))
        cu_q, cu_k, cq, ck, qt, kt = _tables(lens_q, lens_k)
        out0, lse0 = o.bidir_attn_train_fwd(q, k, v, cq, ck, qt, scale, p, B.ATTN_SEED)
        dq0, dk0, dv0 = _nan((Tq, nh, hd), dtype), _nan((Tk, nh, hd), dtype), _nan((Tk, nh, hd), dtype)
        o.bidir_attn_bwd(q, k, v, out0, do, lse0, cq, ck, qt, kt, scale, dq0, dk0, dv0, p, B.ATTN_SEED)
        (qb, qv), (kb, kv), (vb, vv), (dob, dov) = (_padded(t.reshape(t.shape[0], d), 8 * (i + 1)) for i, t in enumerate((q, k, v, do)))
        (ob, ov), (dqb, dqv) = _nan_padded(Tq, d, 40, dtype), _nan_padded(Tq, d, 48, dtype)
        (dkb, dkv), (dvb, dvv) = _nan_padded(Tk, d, 56, dtype), _nan_padded(Tk, d, 64, dtype)
        views = (qv, kv, vv, ov, dov, dqv, dkv, dvv)
        assert len({t.stride(0) for t in views}) == 8 and all(t.data_ptr() % 16 == 0 for t in views)
        lse = _nan((nh, Tq), torch.float32)
        dt, st = o._dt(q), _stream()
        assert L.rpo_bidir_attn_train_fwd(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), qv.stride(0), kv.stride(0), vv.stride(0),
                                          cq.data_ptr(), ck.data_ptr(), qt.data_ptr(), qt.shape[0], 2, 32, Tq, nh, nh, hd, dt, scale, p,
                                          B.ATTN_SEED, ov.data_ptr(), ov.stride(0), lse.data_ptr(), st) == 0
        assert L.rpo_bidir_attn_bwd(qv.data_ptr(), kv.data_ptr(), vv.data_ptr(), qv.stride(0), kv.stride(0), vv.stride(0), ov.data_ptr(),
                                    ov.stride(0), dov.data_ptr(), dov.stride(0), lse.data_ptr(), cq.data_ptr(), ck.data_ptr(),
                                    qt.data_ptr(), qt.shape[0], kt.data_ptr(), kt.shape[0], 2, 32, Tq, nh, nh, hd, dt, scale, p,
                                    B.ATTN_SEED, dqv.data_ptr(), dqv.stride(0), dkv.data_ptr(), dkv.stride(0), dvv.data_ptr(),
                                    dvv.stride(0), st) == 0
        torch.cuda.synchronize()
        label = (label_s, hd, B.TAG[dtype])
        assert torch.equal(ov, out0) and torch.equal(lse, lse0), label
        for name, got, want in (("dq", dqv, dq0), ("dk", dkv, dk0), ("dv", dvv, dv0)):
            assert torch.isfinite(got.float()).all() and torch.equal(got, want.reshape(-1, d)), (name,) + label
        _intact(d, (qb, kb, vb, dob), (ob, dqb, dkb, dvb))
