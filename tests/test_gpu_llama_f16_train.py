"""The fp16 attention of the packed Llama TRAINING pass (header section 9f: rpo_causal_attn_bwd_f16; `ops.causal_attn_f16_bwd`,
`ops.causal_attn_f16_train`, `encoder.LLAMA_FP16_NATIVE_TRAIN` / `LlamaEncoder.native_fp16_train` /
`ModelForTraining(native_fp16=True)`).

Rule for the kernels (the one of tests/test_gpu_attention_parity.py with fp16's unit roundoff: every constant of that file times
2^-3, as tests/test_gpu_llama_f16.py does for the forward: FLOOR 2^-13, ATOL 2^-15, RESOLUTION 2^-13, CEIL_GRAD_BLOCK 2^-8, ROUNDOFF
2^-10).  The reference is float64 on EXACTLY what the backward reads: the fp16 q / k / v / dout, the forward kernel's own fp16 out
and f32 lse (P = exp(scale q k^T - lse), delta = rowsum(dO o out), dS = P (dP - delta)).  Errors are relative Frobenius errors per
(sequence, head) block, the denominator at least ATOL per element and RESOLUTION x the norm of the magnitudes of the summed terms
(that file's `mag`: a gradient block that cancels far below its terms is judged against what fp16 operands can resolve).  The
control is `aten._flash_attention_backward` on the same tensors (lse re-laid to its padded [N, nh, max_q] layout) wherever it
accepts the form: self-attention (causal) and the one-query form (non-causal).  Rule: kernel <= 1.5 x control + FLOOR; the fixed
ceiling applies only where no control accepts the form (bottom-right aligned lq < lk) or the control returns non-finite values.
Kernel and control errors are printed for every case.

End to end: `ModelForTraining(native_fp16=True)` on fp16 weights against `oracle.encoder_ref.contrastive_step` in float64 on the
fp16-held weights, the switch-off step of the same process as the control: max-abs err_on <= 1.5 x err_off + 2 ulp(fp16 at
max|ref|) for the loss, the scores and every gradient, with the loss multiplied by a power of two chosen on the reference."""
import functools
import math

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from oracle import encoder_ref as E
from test_gpu_llama_f16 import (DEV, F16, HARD_LENS, LENS, SHAPES, _assert_regime, _cu, _fused, _ref_attn, _regime_inputs,
                                _ulp2_f16, _views, _visible, ops)

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -13
ATOL = 2.0 ** -15
RESOLUTION = 2.0 ** -13
CEIL_GRAD_BLOCK = 2.0 ** -8
ROUNDOFF = 2.0 ** -10
STEP = 32                      # keys per step of the dQ kernel = queries per step of the dK/dV kernel


# ------------------------------------------------------------------------------------------------
# reference, control, the metric
# ------------------------------------------------------------------------------------------------
def _bwd_ref(q, k, v, go, out, lse, lens_q, lens_k, scale):
    """float64 backward on exactly what the kernels read -> (dq, dk, dv), (mq, mk, mv): the gradients and the magnitudes of the
    terms each element sums (|dS| taken before the cancellation of dP - delta).  `scale` is taken as the entry reads it: the C
    argument is a float, so 1 / sqrt(128) arrives rounded to f32, and the forward kernel formed the lse given here with that very
    value.  A reference that multiplied the scores by the float64 1 / sqrt(128) instead would pair an lse of one scale with scores
    of another: at raw scores of 3e5 the two differ by 8e-4 in the exponent of p (3e-8 relative x 2.6e4), its p would not sum to
    one, and the distance from it would measure that mismatch, not a kernel (1 / sqrt(64) is exact either way)."""
    scale = float(np.float32(scale))
    nh, nkv, hd = q.shape[1], k.shape[1], q.shape[2]
    G, f = nh // nkv, torch.float64
    go, out = go.reshape(-1, nh, hd), out.reshape(-1, nh, hd)
    dq, mq = torch.zeros(q.shape, dtype=f, device=DEV), torch.zeros(q.shape, dtype=f, device=DEV)
    dk, dv, mk, mv = (torch.zeros(k.shape, dtype=f, device=DEV) for _ in range(4))
    oq = ok = 0
    for lq, lk in zip(lens_q, lens_k):
        rq, rk = slice(oq, oq + lq), slice(ok, ok + lk)
        oq, ok = oq + lq, ok + lk
        if lq == 0:
            continue
        vis = _visible(lq, lk)
        for hk in range(nkv):
            hs = slice(hk * G, (hk + 1) * G)
            qq, kk, vv = q[rq, hs].to(f).transpose(0, 1), k[rk, hk].to(f), v[rk, hk].to(f)
            gg, oo = go[rq, hs].to(f).transpose(0, 1), out[rq, hs].to(f).transpose(0, 1)
            sc = ((qq @ kk.T) * scale).masked_fill(~vis, -math.inf)
            p = torch.exp(sc - lse[hs, rq].to(f)[..., None]).masked_fill(~vis, 0.0)
            dp, delta = gg @ vv.T, (gg * oo).sum(-1, keepdim=True)
            ds, dsm = p * (dp - delta), p * (dp.abs() + delta.abs())
            dq[rq, hs] = (ds @ kk).transpose(0, 1) * scale
            dk[rk, hk] = (ds.transpose(1, 2) @ qq).sum(0) * scale
            dv[rk, hk] = (p.transpose(1, 2) @ gg).sum(0)
            mq[rq, hs] = (dsm @ kk.abs()).transpose(0, 1) * abs(scale)
            mk[rk, hk] = (dsm.transpose(1, 2) @ qq.abs()).sum(0) * abs(scale)
            mv[rk, hk] = (p.transpose(1, 2) @ gg.abs()).sum(0)
    return (dq, dk, dv), (mq, mk, mv)


def _pad_lse(lse, lens_q):
    """[nh, Tq] -> the flash op's [N, nh, max_q]."""
    out = torch.zeros(len(lens_q), lse.shape[0], max(lens_q), dtype=torch.float32, device=DEV)
    o0 = 0
    for n, lq in enumerate(lens_q):
        out[n, :, :lq] = lse[:, o0:o0 + lq]
        o0 += lq
    return out


def _bwd_control(q, k, v, go, out, lse, lens_q, lens_k, scale):
    """PyTorch's flash-attention backward on the same tensors, where it accepts the form; else None."""
    nh, hd = q.shape[1], q.shape[2]
    cu_k = _cu(lens_k)
    if list(lens_q) == list(lens_k):
        cu_q, mq, causal = cu_k, max(lens_k), True
    elif all(n == 1 for n in lens_q):
        cu_q, mq, causal = torch.arange(len(lens_q) + 1, dtype=torch.int32, device=DEV), 1, False
    else:
        return None
    z = torch.zeros((), dtype=torch.int64, device=DEV)
    try:
        d = torch.ops.aten._flash_attention_backward(go.reshape(-1, nh, hd).contiguous(), q.contiguous(), k.contiguous(),
                                                     v.contiguous(), out.reshape(-1, nh, hd).contiguous(), _pad_lse(lse, lens_q),
                                                     cu_q, cu_k, mq, max(lens_k), 0.0, causal, z, z, scale=scale)
    except RuntimeError:
        return None
    return d[0].double(), d[1].double(), d[2].double()


def _seg(x2, cu):
    cs = torch.cat([torch.zeros_like(x2[:1]), x2.cumsum(0)], 0)
    return cs[cu[1:].long()] - cs[cu[:-1].long()]


def _block_err(a, r, cu, mag):
    """Relative Frobenius error per (sequence, head) block [N, H]; an empty block (a sequence without queries) has error 0."""
    d2 = (a.double() - r).pow(2).sum(-1)
    r2 = r.pow(2).sum(-1)
    m2 = mag.pow(2).sum(-1) * RESOLUTION ** 2
    cnt = _seg(torch.ones_like(r2), cu)
    den = torch.maximum(_seg(r2, cu), _seg(m2, cu)).sqrt().clamp_min(ATOL * (cnt * r.shape[-1]).sqrt())
    return _seg(d2, cu).sqrt() / den.clamp_min(1e-300)


def _check(label, got, ref, ctrl, cu, mag, need_ctrl=False):
    assert torch.isfinite(got).all(), label
    e = _block_err(got, ref, cu, mag)
    if ctrl is not None and not torch.isfinite(ctrl).all():
        print(f"\n{label}: the control op returned non-finite values on these inputs: no control, the ceiling applies")
        ctrl = None
    assert ctrl is not None or not need_ctrl, (label, "no finite control on a case that requires one")
    if ctrl is not None:
        ec = _block_err(ctrl, ref, cu, mag)
        bound = 1.5 * ec + FLOOR
        print(f"\n{label}: worst block: kernel {float(e.max()):.3e}, control {float(ec.max()):.3e}; "
              f"worst kernel / bound {float((e / bound).max()):.3f}")
    else:
        bound = torch.full_like(e, CEIL_GRAD_BLOCK)
        print(f"\n{label}: worst block: kernel {float(e.max()):.3e}, no control, ceiling {CEIL_GRAD_BLOCK:.3e}")
    assert bool((e <= bound).all()), (label, float((e / bound).max()))


def _fwd(q, k, v, lens_q, lens_k, scale):
    o = ops()
    tiles = o.causal_attn_f16_tile_table(lens_q, lens_k, DEV)
    return o.causal_attn_f16(q, k, v, _cu(lens_q), _cu(lens_k), tiles, scale, want_lse=True)


def _raw(q, k, v, out, lse, dout, lens_q, lens_k, scale):
    o = ops()
    tiles = o.causal_attn_f16_tile_table(lens_q, lens_k, DEV)
    k_tiles = o.causal_attn_f16_key_tile_table(lens_q, lens_k, DEV)
    dq, dk, dv = o.causal_attn_f16_bwd(q, k, v, out, lse, dout, _cu(lens_q), _cu(lens_k), tiles, k_tiles, scale)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape and dq.dtype == dk.dtype == dv.dtype == F16
    nh, nkv, hd = q.shape[1], k.shape[1], q.shape[2]
    # dk | dv (and dq in front of them in self-attention) are column blocks of ONE buffer, as the fused projection's gradient lies
    assert dv.data_ptr() == dk.data_ptr() + 2 * nkv * hd and dk.stride(0) == dv.stride(0)
    if q.shape[0] == k.shape[0]:
        assert dk.data_ptr() == dq.data_ptr() + 2 * nh * hd and dq.stride(0) == dk.stride(0) == (nh + 2 * nkv) * hd
    return dq, dk, dv


def _bwd(q, k, v, dout, lens_q, lens_k, scale):
    """Forward, then the raw backward op: (dq, dk, dv)."""
    out, lse = _fwd(q, k, v, lens_q, lens_k, scale)
    return _raw(q, k, v, out, lse, dout, lens_q, lens_k, scale)


def _check_bwd(q, k, v, dout, lens_q, lens_k, scale, label, need_ctrl=False):
    out, lse = _fwd(q, k, v, lens_q, lens_k, scale)
    got = _raw(q, k, v, out, lse, dout, lens_q, lens_k, scale)
    ref, mag = _bwd_ref(q, k, v, dout, out, lse, lens_q, lens_k, scale)
    ctrl = _bwd_control(q, k, v, dout, out, lse, lens_q, lens_k, scale)
    for name, g, r, c, m, cu in zip(("dq", "dk", "dv"), got, ref, ctrl if ctrl is not None else (None,) * 3, mag,
                                    (_cu(lens_q), _cu(lens_k), _cu(lens_k))):
        _check(f"{label} {name}", g, r, c, cu, m, need_ctrl)
    return got


@functools.lru_cache(maxsize=None)
def _inputs(hd, nh, nkv):
    """One packed batch per shape, q / k / v column blocks of ONE buffer, and a random fp16 dout: made once, never modified."""
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh * 10 + nkv + 1)
    qkv, (q, k, v) = _fused(sum(LENS), nh, nkv, hd, gen)
    assert q.stride(0) == (nh + 2 * nkv) * hd and k.data_ptr() == qkv.data_ptr() + 2 * nh * hd and not q.is_contiguous()
    dout = torch.randn(sum(LENS), nh * hd, generator=gen, device=DEV).to(F16)
    return q, k, v, dout, 1.0 / math.sqrt(hd)


# ------------------------------------------------------------------------------------------------
# the kernels against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_self_attention(hd, nh, nkv):
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    _check_bwd(q, k, v, dout, LENS, LENS, scale, f"self hd{hd} nh{nh} nkv{nkv}", need_ctrl=True)


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_last_query_form(hd, nh, nkv):
    """One query per sequence (its last token) over the same K / V: it sees every key."""
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    last = torch.tensor(np.cumsum(LENS) - 1, device=DEV)
    ql = q.reshape(q.shape[0], -1).index_select(0, last).view(-1, nh, hd)
    _check_bwd(ql, k, v, dout.index_select(0, last), [1] * len(LENS), LENS, scale, f"last query hd{hd} nh{nh} nkv{nkv}",
               need_ctrl=True)


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_bottom_right_alignment(hd, nh, nkv):
    """lens_q[n] = ceil(lens_k[n] / 3): query i sees keys j <= i + (lk - lq).  No control takes the form: the ceiling."""
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    lens_q = [-(-n // 3) for n in LENS]
    assert max(lens_q) > 256 and any(n % 32 for n in lens_q)
    T = sum(lens_q)
    assert _bwd_control(q[:T], k, v, dout[:T], dout[:T], torch.zeros(nh, T, device=DEV), lens_q, LENS, scale) is None
    _check_bwd(q[:T], k, v, dout[:T], lens_q, LENS, scale, f"bottom-right hd{hd} nh{nh} nkv{nkv}")


def test_backward_long_sequence():
    """More than 128 key steps and more than 128 query steps."""
    gen = torch.Generator(device=DEV).manual_seed(4100)
    lens = [4100, 3]
    assert lens[0] > 128 * STEP
    _, (q, k, v) = _fused(sum(lens), 4, 1, 64, gen)
    dout = torch.randn(sum(lens), 4 * 64, generator=gen, device=DEV).to(F16)
    _check_bwd(q, k, v, dout, lens, lens, 0.125, "4100 keys", need_ctrl=True)


# ------------------------------------------------------------------------------------------------
# hard inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["flat", "spike", "sink", "growing", "negative"])
@pytest.mark.parametrize("hd", [64, 128])
def test_backward_regimes(hd, regime):
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = hd ** -0.5
    hit = set()
    for steps in ([(0, 1), (5, "last")] if regime == "spike" else [None]):
        qkv, spikes = _regime_inputs(hd, nh, nkv, lens, regime, 300 + hd + len(regime), steps)
        q, k, v = _views(qkv, nh, nkv, hd)
        gen = torch.Generator(device=DEV).manual_seed(hd + len(regime))
        dout = torch.randn(sum(lens), nh * hd, generator=gen, device=DEV).to(F16)
        if regime == "flat":        # randn q / k: logits ~ N(0, 1)
            s = torch.einsum("qhd,khd->hqk", q[18:218].double(), k[18:218].double().repeat_interleave(2, 1)) * scale
            assert 0.9 < float(s.std()) < 1.1 and float(s.abs().max()) < 8.0
        else:
            _assert_regime(regime, q, k, nh, nkv, lens, spikes, _ref_attn(q, k, v, lens, lens, scale)[1], scale)
        hit |= {(sp[7], sp[4]) for sp in spikes}
        _check_bwd(q, k, v, dout, lens, lens, scale, f"{regime} {steps} hd{hd}", need_ctrl=regime == "flat")
    if regime == "spike":
        assert {(0, 0), (1, 32), (5, 160), ("last", 192)} <= hit, hit


@pytest.mark.parametrize("case", ["saturated", "raw", "identical", "negative-scale"])
@pytest.mark.parametrize("hd", [64, 128])
def test_backward_hard_inputs(hd, case):
    """saturated: scores ~ +-60 after scaling (one key per query dominates).  raw: raw q . k beyond the fp16 range (a kernel that
    rounds S to fp16 sees inf).  identical: identical keys, uniform weights over the visible keys.  negative-scale: |scale| and a
    sign on q, as in the forward.

    The raw scores of [raw] reach 3e5, where one f32 rounding of a score (ulp 2^-5) times the scale is ~1e-3 in the exponent of
    p and the softmax is one-hot but for a handful of (query, key) pairs that carry a block's whole gradient: the kernels sum
    each 32-wide chunk of the head dim from zero and add the chunks without a rounding (`chunk_add`), and the reference takes
    the scale as the entry reads it (`_bwd_ref`)."""
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    # every case's inputs are drawn from ONE generator in a fixed order, whichever case runs: a case's inputs do not depend on
    # how the cases are split over tests
    dout = torch.randn(T, nh * hd, generator=gen, device=DEV).to(F16)
    sat = torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV)
    big = torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV)
    _, same = _fused(T, nh, nkv, hd, gen)
    if case == "saturated":
        mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
        sat[:, :(nh + nkv) * hd] *= mult
        q, k, v = _views(sat.to(F16), nh, nkv, hd)
        s = torch.einsum("qhd,khd->hqk", q[-65:].double(), k[-65:].double().repeat_interleave(2, 1)) * scale
        assert float(s.abs().max()) > 60.0 and float(s.std()) > 30.0
        _check_bwd(q, k, v, dout, lens, lens, scale, f"saturated hd{hd}")
    elif case == "raw":
        big[:, :(nh + nkv) * hd] *= 100.0
        q, k, v = _views(big.to(F16), nh, nkv, hd)
        raw = torch.einsum("qhd,khd->hqk", q[18:218].double(), k[18:218].double().repeat_interleave(2, 1))
        raw = raw.masked_fill(~_visible(200, 200), 0.0)
        assert float(raw.abs().max()) > 65504.0 and float(q.float().abs().max()) < 65504.0       # among the VISIBLE pairs
        _check_bwd(q, k, v, dout, lens, lens, scale, f"raw scores beyond fp16 hd{hd}")
    elif case == "identical":
        q, k, v = same
        _check_bwd(q, k[:1].expand(T, nkv, hd).contiguous(), v, dout, lens, lens, scale, f"identical keys hd{hd}")
    else:
        # against float64 under the ceiling (the flash op is no control at a negative scale unless it returns finite values), and
        # against the call on -q with |scale|: dq is its negation and dv its copy, bit for bit (the same products in the same
        # order); dk sums the NEGATED products q dS, and the rounding inside the MFMA's accumulation need not be symmetric in
        # the sign, so dk is held to the float64 reference only
        q, k, v = same
        neg = _check_bwd(q, k, v, dout, lens, lens, -scale, f"negative scale hd{hd}")
        pos = _bwd(-q, k, v, dout, lens, lens, scale)
        assert torch.equal(neg[0], -pos[0]) and torch.equal(neg[2], pos[2])
        assert _block_err(neg[1], pos[1].double(), _cu(lens), torch.zeros_like(pos[1], dtype=torch.float64)).max() <= ROUNDOFF


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("exp", [10, -10])
def test_scaled_dout_as_a_loss_scaler_makes_it(hd, exp):
    """dout x 2^10 and x 2^-10 (exact in fp16: no element of the base is subnormal after scaling down, none overflows after
    scaling up), held to the same rule against the equally scaled control."""
    gen = torch.Generator(device=DEV).manual_seed(17 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    base = torch.randn(sum(lens), nh * hd, generator=gen, device=DEV).clamp(-8, 8)
    base = torch.where(base.abs() < 2.0 ** -4, torch.full_like(base, 2.0 ** -4), base).to(F16)     # >= 2^-14 after x 2^-10
    dout = (base.float() * 2.0 ** exp).to(F16)
    assert torch.equal(dout.float() * 2.0 ** -exp, base.float()) and torch.isfinite(dout).all()
    _check_bwd(q, k, v, dout, lens, lens, 1.0 / math.sqrt(hd), f"dout x 2^{exp} hd{hd}", need_ctrl=True)


def test_an_infinite_dout_element_reaches_its_dq_row():
    gen = torch.Generator(device=DEV).manual_seed(23)
    hd, nh, nkv, lens = 64, 8, 2, [40, 70, 33]
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    dout = torch.randn(sum(lens), nh * hd, generator=gen, device=DEV).to(F16)
    base = _bwd(q, k, v, dout, lens, lens, 0.125)
    t, h = 40 + 50, 5                                            # query 50 of the middle sequence, head 5
    bad = dout.clone()
    bad[t, h * hd + 7] = math.inf
    got = _bwd(q, k, v, bad, lens, lens, 0.125)
    assert not torch.isfinite(got[0][t, h]).all()
    mid = slice(40, 110)
    for a, b in zip(got, base):
        assert torch.equal(a[:40], b[:40]) and torch.equal(a[110:], b[110:])
        assert torch.isfinite(a[:40]).all() and torch.isfinite(a[110:]).all()
    # inside the sequence: the other query heads' dq rows and the other kv heads' dk / dv rows are untouched as well
    keep = [x for x in range(nh) if x != h]
    assert torch.equal(got[0][mid][:, keep], base[0][mid][:, keep])
    other_kv = [x for x in range(nkv) if x != h // (nh // nkv)]
    assert torch.equal(got[1][mid][:, other_kv], base[1][mid][:, other_kv])
    assert torch.equal(got[2][mid][:, other_kv], base[2][mid][:, other_kv])
    assert not torch.isfinite(got[1][mid][:, h // (nh // nkv)]).all()


@pytest.mark.parametrize("hd", [64, 128])
def test_no_gradient_leaks_across_the_mask(hd):
    """dout = 0 for every query behind the middle position P of its sequence.  The keys behind P are seen by those queries only:
    their dk / dv rows are exact zeros, and so is dq of the queries behind P.  The rows up to P are BIT-equal to a call on the
    sequences truncated at P (both kernels start their steps at row 0 of the sequence resp. at the key entry's first row, so the
    steps are the same and what lies behind P enters every sum as an exact zero), and BIT-equal when the keys and values behind
    P change (x 1001): the queries up to P do not see them, and those behind contribute exact zeros."""
    gen = torch.Generator(device=DEV).manual_seed(70 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = 1.0 / math.sqrt(hd)
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    pos = torch.cat([torch.arange(n, device=DEV) for n in lens])
    P = torch.cat([torch.full((n,), n // 2, device=DEV) for n in lens])           # 0, 8, 100, 32
    behind = pos > P
    dout = (torch.randn(sum(lens), nh * hd, generator=gen, device=DEV) * (~behind)[:, None]).to(F16)
    dq, dk, dv = _bwd(q, k, v, dout, lens, lens, scale)
    for t in (dq, dk, dv):
        assert torch.isfinite(t).all() and (t[behind] == 0).all()
        assert (t[~behind] != 0).any()
    cut = [n // 2 + 1 for n in lens]
    tq, tk, tv = _bwd(q[~behind].contiguous(), k[~behind].contiguous(), v[~behind].contiguous(), dout[~behind].contiguous(),
                      cut, cut, scale)
    assert torch.equal(dq[~behind], tq) and torch.equal(dk[~behind], tk) and torch.equal(dv[~behind], tv)
    f = (1 + 1000 * behind[:, None, None].float())
    k2, v2 = (k.float() * f).to(F16).contiguous(), (v.float() * f).to(F16).contiguous()
    assert torch.isfinite(k2).all() and float(k2.float().abs().max()) > 1000.0
    fq, fk, fv = _bwd(q, k2, v2, dout, lens, lens, scale)
    assert torch.equal(fq[~behind], dq[~behind]) and torch.equal(fk[~behind], dk[~behind]) and torch.equal(fv[~behind], dv[~behind])
    # the dout of later queries: the dq rows of the earlier ones do not move (a lane owns one query)
    dout2 = dout.clone()
    dout2[behind] = torch.randn(int(behind.sum()), nh * hd, generator=gen, device=DEV).to(F16)
    gq, gk, gv = _bwd(q, k, v, dout2, lens, lens, scale)
    assert torch.equal(gq[~behind], dq[~behind]) and not torch.equal(gq[behind], dq[behind])
    assert not torch.equal(gk, dk) and not torch.equal(gv, dv)


def test_deterministic_and_independent_of_packing():
    gen = torch.Generator(device=DEV).manual_seed(5)
    hd, nh, nkv = 64, 8, 2
    la, lx, lb = 33, 70, 17
    _, (q, k, v) = _fused(la + lx + lb, nh, nkv, hd, gen)
    dout = torch.randn(la + lx + lb, nh * hd, generator=gen, device=DEV).to(F16)
    scale = 0.125
    one = _bwd(q, k, v, dout, [la, lx, lb], [la, lx, lb], scale)
    two = _bwd(q, k, v, dout, [la, lx, lb], [la, lx, lb], scale)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    mid = slice(la, la + lx)
    alone = _bwd(q[mid], k[mid], v[mid], dout[mid], [lx], [lx], scale)
    assert all(torch.equal(a[mid], b) for a, b in zip(one, alone))
    first = _bwd(q[la:], k[la:], v[la:], dout[la:], [lx, lb], [lx, lb], scale)
    assert all(torch.equal(a[:lx], b) for a, b in zip(first, alone))
    # the other order: b | a | x, the sequence last
    perm = torch.cat([torch.arange(la + lx, la + lx + lb), torch.arange(la), torch.arange(la, la + lx)]).to(DEV)
    swapped = _bwd(q[perm].contiguous(), k[perm].contiguous(), v[perm].contiguous(), dout[perm].contiguous(), [lb, la, lx],
                   [lb, la, lx], scale)
    assert all(torch.equal(a[lb + la:], b) for a, b in zip(swapped, alone))


def test_keys_without_queries_get_zeros():
    gen = torch.Generator(device=DEV).manual_seed(6)
    lens_q, lens_k = [0, 3], [4, 3]
    _, (_, k, v) = _fused(7, 4, 2, 64, gen)
    q = torch.randn(3, 4, 64, generator=gen, device=DEV).to(F16)
    dout = torch.randn(3, 4 * 64, generator=gen, device=DEV).to(F16)
    dq, dk, dv = _check_bwd(q, k, v, dout, lens_q, lens_k, 0.125, "lq == 0")
    assert (dk[:4] == 0).all() and (dv[:4] == 0).all() and (dk[4:] != 0).any()


def test_a_row_without_a_finite_lse_contributes_zeros():
    gen = torch.Generator(device=DEV).manual_seed(8)
    hd, nh, nkv, lens = 64, 4, 2, [40, 37]
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    dout = torch.randn(sum(lens), nh * hd, generator=gen, device=DEV).to(F16)
    out, lse = _fwd(q, k, v, lens, lens, 0.125)
    base = _raw(q, k, v, out, lse, dout, lens, lens, 0.125)
    t, h = 20, 3
    lse2 = lse.clone()
    lse2[h, t] = -math.inf
    got = _raw(q, k, v, out, lse2, dout, lens, lens, 0.125)
    assert all(torch.isfinite(g).all() for g in got)
    assert (got[0][t, h] == 0).all() and (base[0][t, h] != 0).any()
    rest = torch.ones(sum(lens), nh, dtype=torch.bool, device=DEV)
    rest[t, h] = False
    assert torch.equal(got[0][rest], base[0][rest])
    # the row's terms are gone from dk / dv of its kv head and sequence: what is left is the backward with that row's dout zeroed
    dz = dout.clone()
    dz[t, h * hd:(h + 1) * hd] = 0
    zero = _raw(q, k, v, out, lse, dz, lens, lens, 0.125)
    assert torch.equal(got[1], zero[1]) and torch.equal(got[2], zero[2])


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refuses_what_it_cannot_run():
    """RPO_ERR_UNSUPPORTED before any launch: the buffers here are far smaller than what the refused shapes would touch."""
    from rankpo_amd import _lib
    lib = _lib.load()
    OK, UNS = 0, -2
    st = torch.cuda.current_stream().cuda_stream
    xf = torch.zeros(4096 * 16, dtype=F16, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    p = xf.data_ptr()
    o1, o2, o3, o4 = (p + 4096 * 2 * i for i in (4, 6, 8, 10))

    def bwd(ptr=p, stride=256, tl=tiles, cols=2, qb=32, nh=2, nkv=1, hd=64, dq=o1, dkv=o2, ws=o3, dstride=128, n=1, nk=1):
        return lib.rpo_causal_attn_bwd_f16(ptr, ptr, ptr, ptr, ptr, stride, stride, stride, stride, stride, o4, cu.data_ptr(),
                                           cu.data_ptr(), tl.data_ptr(), n, tl.data_ptr(), nk, cols, qb, 1, nh, nkv, hd, 0.1, dq,
                                           dstride, dkv, dstride, dkv, dstride, ws, st)
    assert bwd() == OK                                         # the checks below do not refuse everything
    assert bwd(n=0, nk=0) == OK                                # empty work lists: nothing to launch
    assert bwd(n=0) == OK and bwd(nk=0) == OK                  # one empty list alone skips its kernel
    assert bwd(hd=32) == UNS
    assert bwd(hd=96, stride=768) == UNS
    assert bwd(nh=3, nkv=2) == UNS                             # nh % nkv
    assert bwd(nh=3, nkv=1) == UNS                             # 3 query heads per kv head
    assert bwd(nh=16, nkv=1, stride=4096) == UNS               # 16
    assert bwd(tl=tiles3, cols=3) == UNS                       # another table format
    assert bwd(qb=64) == UNS and bwd(qb=128) == UNS
    assert bwd(ptr=p + 8) == UNS and bwd(ptr=p + 2) == UNS     # misaligned q / k / v / out / dout
    assert bwd(dq=o1 + 8) == UNS and bwd(dkv=o2 + 4) == UNS and bwd(ws=o3 + 2) == UNS
    assert bwd(stride=260) == UNS and bwd(dstride=132) == UNS  # token strides that are no multiple of 8 elements
    torch.cuda.synchronize()


def test_wrapper_refuses_what_the_entry_refuses():
    o = ops()
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    q = torch.zeros(4, 2, 64, device=DEV, dtype=F16)
    lse = torch.zeros(2, 4, device=DEV)
    dq, dk, dv = o.causal_attn_f16_bwd(q, q, q, q.view(4, -1), lse, q.view(4, -1), cu, cu, tiles, tiles, 0.1)     # accepted
    assert (dq == 0).all() and (dk == 0).all() and (dv == 0).all()
    for bad in (q.float(), q.bfloat16(), q.cpu()):
        with pytest.raises(ValueError):
            o.causal_attn_f16_bwd(bad, bad, bad, bad.view(4, -1), lse, bad.view(4, -1), cu, cu, tiles, tiles, 0.1)
    q32 = torch.zeros(4, 3, 32, device=DEV, dtype=F16)
    with pytest.raises(ValueError):
        o.causal_attn_f16_bwd(q32, q32, q32, q32.view(4, -1), torch.zeros(3, 4, device=DEV), q32.view(4, -1), cu, cu, tiles, tiles, 0.1)
    q3 = torch.zeros(4, 3, 64, device=DEV, dtype=F16)
    with pytest.raises(ValueError):                            # 3 query heads per kv head
        o.causal_attn_f16_bwd(q3, q3[:, :1], q3[:, :1], q3.view(4, -1), torch.zeros(3, 4, device=DEV), q3.view(4, -1), cu, cu, tiles,
                              tiles, 0.1)
    odd = torch.zeros(4, 2 * 64 + 4, device=DEV, dtype=F16)[:, :128].view(4, 2, 64)         # token stride 132
    with pytest.raises(ValueError):
        o.causal_attn_f16_bwd(odd, odd, odd, q.view(4, -1), lse, q.view(4, -1), cu, cu, tiles, tiles, 0.1)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):                            # malformed lists
        o.causal_attn_f16_bwd(q, q, q, q.view(4, -1), lse, q.view(4, -1), cu, cu, tiles3, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16_bwd(q, q, q, q.view(4, -1), lse, q.view(4, -1), cu, cu, tiles, tiles.long(), 0.1)
    with pytest.raises(ValueError):                            # out of another dtype, lse of another shape
        o.causal_attn_f16_bwd(q, q, q, q.view(4, -1).float(), lse, q.view(4, -1), cu, cu, tiles, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16_bwd(q, q, q, q.view(4, -1), lse.T.contiguous(), q.view(4, -1), cu, cu, tiles, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16_key_tile_table([5], [4], DEV)


# ------------------------------------------------------------------------------------------------
# the autograd Function
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", [(64, 8, 2), (128, 4, 1)])
def test_autograd_function_is_the_raw_op(hd, nh, nkv):
    o = ops()
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    raw = _bwd(q, k, v, dout, LENS, LENS, scale)
    qkv = torch.cat([t.reshape(t.shape[0], -1) for t in (q, k, v)], 1).requires_grad_()
    qg, kg, vg = (t.view(-1, n, hd) for t, n in zip(qkv.split([nh * hd, nkv * hd, nkv * hd], 1), (nh, nkv, nkv)))
    cu = _cu(LENS)
    tiles, k_tiles = o.causal_attn_f16_tile_table(LENS, LENS, DEV), o.causal_attn_f16_key_tile_table(LENS, LENS, DEV)
    out = o.causal_attn_f16_train(qg, kg, vg, cu, cu, tiles, k_tiles, scale)
    assert out.requires_grad and out.dtype == F16 and torch.equal(out, o.causal_attn_f16(q, k, v, cu, cu, tiles, scale)[0])
    got = torch.autograd.grad(out, (qg, kg, vg), dout)
    assert all(torch.equal(a, b) for a, b in zip(got, raw))
    # through the fused buffer: its gradient is the three blocks side by side
    out = o.causal_attn_f16_train(qg, kg, vg, cu, cu, tiles, k_tiles, scale)
    (gqkv,) = torch.autograd.grad(out, (qkv,), dout)
    assert torch.equal(gqkv, torch.cat([t.reshape(t.shape[0], -1) for t in raw], 1))
    # dout of another stride: made contiguous, the same bits
    wide = torch.zeros(dout.shape[0], dout.shape[1] + 2, device=DEV, dtype=F16)
    wide[:, 1:-1] = dout
    out = o.causal_attn_f16_train(qg, kg, vg, cu, cu, tiles, k_tiles, scale)
    got = torch.autograd.grad(out, (qg, kg, vg), wide[:, 1:-1])
    assert all(torch.equal(a, b) for a, b in zip(got, raw))
    # the forward-only op keeps its contract: no autograd node
    assert o.causal_attn_f16(qg, kg, vg, cu, cu, tiles, scale)[0].grad_fn is None


# ------------------------------------------------------------------------------------------------
# end to end: ModelForTraining on an fp16 Llama encoder
# ------------------------------------------------------------------------------------------------
TEMP = 0.02


class Spy(TorchDispatchMode):
    """Counts the new ops and the stock flash ops (as the dispatcher sees them on the calling thread; the backward op runs on the
    autograd thread, where it can only follow a flash forward, which is counted)."""

    def __init__(self, poison=False):
        super().__init__()
        self.poison = poison
        self.n = {"train": 0, "full": 0, "last": 0, "bwd": 0, "flash_fwd": 0, "flash_bwd": 0}

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten._flash_attention_forward.default:
            self.n["flash_fwd"] += 1
        if func is torch.ops.aten._flash_attention_backward.default:
            self.n["flash_bwd"] += 1
        return func(*args, **(kwargs or {}))

    def __enter__(self):
        o = ops()
        self._train, self._bwd = o.causal_attn_f16_train, o.causal_attn_f16_bwd

        def train(q, k, *a, **kw):
            self.n["train"] += 1
            self.n["full" if q.shape[0] == k.shape[0] else "last"] += 1
            return self._train(q, k, *a, **kw)

        def bwd(q, k, v, out, lse, dout, *a, **kw):
            self.n["bwd"] += 1
            if self.poison:                                     # an overflow somewhere upstream: one dout element is inf
                dout = dout.contiguous().clone()
                dout.view(-1)[3] = math.inf
            return self._bwd(q, k, v, out, lse, dout, *a, **kw)
        o.causal_attn_f16_train, o.causal_attn_f16_bwd = train, bwd
        super().__enter__()
        return self

    def __exit__(self, *exc):
        super().__exit__(*exc)
        o = ops()
        o.causal_attn_f16_train, o.causal_attn_f16_bwd = self._train, self._bwd
        return False


def _build(hd, seed, dtype=F16, **kw):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import _cfg
    torch.manual_seed(seed)
    cfg = _cfg(PE, hd)
    enc = PE.LlamaEncoder(cfg).to(DEV, dtype)
    held = {k: v.detach().double().cpu() for k, v in enc.state_dict().items()}       # the weights as the model holds them
    model = rankpo_amd.ModelForTraining(encoder=enc, temperature=TEMP, **kw).train()
    return PE, cfg, held, model


def _batch(tok, rs, dev):
    """2 queries + 4 passages: 6 sequences of 1 .. 400 tokens."""
    from test_gpu_inference import _texts
    qt = _texts(rs, 1, 1, 60) + ["q"]                           # one 1-token row
    pt = _texts(rs, 3, 40, 400) + _texts(rs, 1, 380, 400)
    b = {"query": tok(qt, max_length=400), "passage": tok(pt, max_length=400)}
    return {s: {k: v.to(dev) for k, v in d.items()} for s, d in b.items()}


def _step(model, batch, mult=1.0):
    """(loss, scores, {name: grad}, spy counts) of one forward + backward of loss x mult."""
    model.zero_grad(set_to_none=True)
    with Spy() as spy:
        out = model(**batch)
        (out.loss.float() * mult).backward()
    grads = {k: p.grad.detach().clone() for k, p in model.model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return out.loss.detach().clone(), out.scores.detach().clone(), grads, spy.n


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def _loss_multiplier(ref_grads):
    """The power of two the loss is multiplied by, chosen on the float64 reference gradients: the largest that leaves one binade
    of headroom under 2^15 for the largest gradient element of any weight.  Then, for every weight gradient, at most 1 %
    of its non-zero elements lie below fp16's smallest normal 2^-14 (an exact zero -- an embedding row no token uses -- has nothing
    to lose) and none exceeds 2^15: asserted."""
    top = max(float(g.abs().max()) for g in ref_grads.values())
    mult = 2.0 ** (14 - math.ceil(math.log2(top)))
    for k, g in ref_grads.items():
        a = g.abs() * mult
        nz = a > 0
        assert float(a.max()) <= 2.0 ** 15, k
        assert int(nz.sum()) > 0 and float(((a < 2.0 ** -14) & nz).sum()) <= 0.01 * float(nz.sum()), k
    return mult


@pytest.fixture(scope="module", params=[64, 128])
def train_case(request):
    """One fp16 model per config with every switch off and its step BEFORE any switch is touched (the control), the same weights
    with native_fp16=True, the batch, and the float64 oracle step on the fp16-held weights: computed once, shared, never
    modified."""
    from test_gpu_inference import CharTok
    hd = request.param
    PE, cfg, held, off = _build(hd, 30 + hd)
    _, _, held_on, on = _build(hd, 30 + hd, native_fp16=True)
    assert all(torch.equal(held[k], held_on[k]) for k in held) and cfg.num_hidden_layers == 3
    assert not PE.LLAMA_FP16_NATIVE_TRAIN and not PE.LLAMA_FP16_NATIVE
    assert not off.model.native_fp16_train and not off.model.native_fp16
    assert on.model.native_fp16_train and on.model.native_fp16 and on.model.embed_tokens.weight.dtype == F16
    batch = _batch(CharTok(), np.random.RandomState(hd), DEV)
    lens = torch.cat([batch["query"]["attention_mask"].sum(1), batch["passage"]["attention_mask"].sum(1)]).tolist()
    assert len(lens) == 6 and min(lens) == 1 and 380 <= max(lens) <= 400
    w64 = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in held.items()}
    cpu = {s: {k: v.cpu() for k, v in d.items()} for s, d in batch.items()}
    loss, scores, _, _ = E.contrastive_step(w64, cfg.to_dict(), cpu, TEMP, dtype=torch.float64)
    loss.backward()
    names = [k for k, _ in off.model.named_parameters()]
    ref_g = {k: w64[k].grad for k in names}
    assert all(g is not None for g in ref_g.values())
    mult = _loss_multiplier(ref_g)
    base = _step(off, batch, mult)
    return dict(hd=hd, PE=PE, cfg=cfg, off=off, on=on, batch=batch, base=base, mult=mult,
                ref=(loss.detach(), scores.detach(), {k: g * mult for k, g in ref_g.items()}))


def test_switch_off_runs_what_it_ran(train_case, monkeypatch):
    c = train_case
    nl = c["cfg"].num_hidden_layers
    n = c["base"][3]
    assert n["train"] == 0 and n["bwd"] == 0 and n["flash_fwd"] == nl, n              # queries and passages: ONE packed pass
    again = _step(c["off"], c["batch"], c["mult"])
    _same_bits(again, c["base"])
    # the no-grad switch on: grad mode is not its business
    monkeypatch.setattr(c["PE"], "LLAMA_FP16_NATIVE", True)
    monkeypatch.setattr(c["off"].model, "native_fp16", True)
    res = _step(c["off"], c["batch"], c["mult"])
    assert res[3]["train"] == 0 and res[3]["bwd"] == 0 and res[3]["flash_fwd"] == nl, res[3]
    _same_bits(res, c["base"])


def _against_oracle(c, res, label):
    ref_loss, ref_scores, ref_g = c["ref"]
    base = c["base"]
    worst = (0.0, None, 0.0, 0.0)
    items = [("loss", res[0].view(1), base[0].view(1), ref_loss.view(1)), ("scores", res[1], base[1], ref_scores)]
    items += [(k, res[2][k], base[2][k], r) for k, r in ref_g.items()]
    for k, got, ctl, r in items:
        assert torch.isfinite(got).all(), k
        e = float((got.double().cpu() - r).abs().max())
        ce = float((ctl.double().cpu() - r).abs().max())
        bound = 1.5 * ce + _ulp2_f16(r)
        worst = max(worst, (e / bound, k, e, ce))
        assert e <= bound, (label, k, e, ce, bound)
    print(f"\n{label} hd{c['hd']} (loss x 2^{int(math.log2(c['mult']))}): worst err / bound {worst[0]:.3f} at {worst[1]} "
          f"(max-abs {worst[2]:.3e}, switch-off control {worst[3]:.3e})")


def test_training_step_vs_oracle(train_case, monkeypatch):
    c = train_case
    nl = c["cfg"].num_hidden_layers
    res = _step(c["on"], c["batch"], c["mult"])
    n = res[3]
    assert n["flash_fwd"] == 0 and n["flash_bwd"] == 0, n
    # queries and passages are ONE packed pass: one forward and one backward call per block, the last block's in the one-query form
    assert n["train"] == nl and n["full"] == nl - 1 and n["last"] == 1 and n["bwd"] == nl, n
    _against_oracle(c, res, "switch on")
    _same_bits(_step(c["on"], c["batch"], c["mult"]), res)                      # deterministic
    # the module switch on the switch-off model: the same path, the same bits
    monkeypatch.setattr(c["PE"], "LLAMA_FP16_NATIVE_TRAIN", True)
    mod = _step(c["off"], c["batch"], c["mult"])
    assert mod[3]["train"] == nl and mod[3]["flash_fwd"] == 0, mod[3]
    _same_bits(mod, res)


def test_training_step_with_checkpointing_vs_oracle(train_case):
    """gradient_checkpointing_enable(layers="all"): every block's forward runs twice (the recomputation runs the same deterministic
    kernel), its backward once; held to the same rule."""
    c = train_case
    nl = c["cfg"].num_hidden_layers
    c["on"].gradient_checkpointing_enable(layers="all")
    try:
        ck = _step(c["on"], c["batch"], c["mult"])
    finally:
        c["on"].model.gradient_checkpointing_disable()
    n = ck[3]
    assert n["flash_fwd"] == 0 and n["flash_bwd"] == 0 and n["train"] == 2 * nl and n["bwd"] == nl, n
    _against_oracle(c, ck, "switch on, checkpointed")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_other_dtypes_ignore_the_switch_and_the_keyword(dtype, monkeypatch):
    from test_gpu_inference import CharTok
    PE, cfg, _, off = _build(64, 9, dtype=dtype)
    batch = _batch(CharTok(), np.random.RandomState(3), DEV)
    a = _step(off, batch)
    _, _, _, on = _build(64, 9, dtype=dtype, native_fp16=True)
    monkeypatch.setattr(PE, "LLAMA_FP16_NATIVE_TRAIN", True)
    assert on.model.native_fp16_train and on.model.embed_tokens.weight.dtype == dtype
    b = _step(on, batch)
    assert b[3]["train"] == 0 and b[3]["bwd"] == 0, b[3]
    _same_bits(a, b)


def test_left_padded_batches_give_the_switch_off_bits(train_case):
    from test_gpu_bert_native import LeftTok
    c = train_case
    batch = _batch(LeftTok(), np.random.RandomState(8), DEV)
    a, b = _step(c["on"], batch), _step(c["off"], batch)
    assert a[3]["train"] == 0 and a[3]["bwd"] == 0, a[3]
    _same_bits(a, b)


def test_train_step_with_the_dynamic_loss_scaler():
    """TrainStep(loss_scale="dynamic") on the switch-on model: a finite step updates the parameters; a step in which one dout
    element of an attention backward is inf (the kernel carries it into dq, from where it reaches the weight gradients) is skipped
    and, with the hysteresis spent, halves the scale."""
    from rankpo_amd import TrainStep
    from test_gpu_inference import CharTok
    PE, cfg, _, model = _build(64, 41, native_fp16=True)
    batch = _batch(CharTok(), np.random.RandomState(5), DEV)
    ts = TrainStep(model.parameters(), lambda b: model(**b)["loss"], lr=1e-3, total_steps=100, warmup_ratio=0.0,
                   loss_scale="dynamic")
    ts.opt.load_loss_scale_state({"scale": 2.0 ** 8, "cur_hysteresis": 1})
    w0 = ts.opt.flat_param.clone()
    with Spy() as spy:
        loss = ts.step([batch])
    st = ts.loss_scale_state()
    assert spy.n["bwd"] == cfg.num_hidden_layers and spy.n["flash_fwd"] == 0, spy.n
    assert math.isfinite(float(loss)) and st["applied_steps"] == 1 and st["skipped_steps"] == 0 and st["scale"] == 2.0 ** 8, st
    assert not torch.equal(ts.opt.flat_param, w0) and bool(torch.isfinite(ts.opt.flat_param).all())
    w1 = ts.opt.flat_param.clone()
    with Spy(poison=True) as spy:
        ts.step([batch])
    st = ts.loss_scale_state()
    assert spy.n["bwd"] == cfg.num_hidden_layers, spy.n
    assert st["applied_steps"] == 1 and st["skipped_steps"] == 1 and st["scale"] == 2.0 ** 7, st
    assert torch.equal(ts.opt.flat_param, w1)
