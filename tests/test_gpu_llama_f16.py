"""The native fp16 pass of a Llama encoder (header section 9e: rpo_causal_attn_fwd_f16, `ops.causal_attn_f16`; the fp16 forward
instantiations of rpo_add_rmsnorm_fwd / rpo_rope / rpo_swiglu_fwd; `encoder.LLAMA_FP16_NATIVE` / `LlamaEncoder.native_fp16` /
`ModelForInference(native_fp16=True)`).

Rule for the attention kernel (the one of tests/test_gpu_attention_parity.py).  Errors are taken against a float64 reference on the
EXACT fp16 inputs (upcast, never re-rounded), per (sequence, head) block as relative Frobenius errors, and per row for the output.
Each block needs  kernel <= 1.5 x control + FLOOR, the control being what the switch-off path runs:
`torch.ops.aten._flash_attention_forward` on the same fp16 tensors, wherever it accepts the form (self-attention with causal=True;
the one-query form with cu_q = arange(N + 1), non-causal).  The constants are that file's with the bf16 unit roundoff 2^-8 replaced
by fp16's 2^-11, i.e. each times 2^-3: FLOOR 2^-13, CEIL_OUT_BLOCK 2^-10, CEIL_OUT_ROW 2^-9, LSE_TOL 2^-11 + 2^-16 |ref|, ROUNDOFF
2^-10 (and the per-element denominator floor ATOL 2^-15).  The fixed ceilings apply only where no control accepts the form
(bottom-right aligned lq < lk) and to single rows.  Kernel and control errors are printed for every case.

Where two calls run the same keys in the same key steps for a query (the kernel's key steps start at key 0 of the sequence in
every form, a lane owns one query, and a step in which a query sees no key leaves its state unchanged bit for bit), their rows
are asserted BIT-equal: the last-query form and the bottom-right form against the self-attention call, a sequence packed alone /
first / last, and the rows in front of modified future keys.

Row kernels: the references and bounds of tests/test_gpu_encoder_ops_parity.py with fp16 entries (U_STORE 2^-11, P_BITS 11, VEC 8,
FLOOR 2^-13) held in this file; the half-ulp term of its element check is taken with fp16's subnormal spacing (2^-24 below 2^-14),
which that file's f32 / bf16 form (2^-126) does not have to know about.

End to end: `ModelForInference.encode(use_fp16=True)` against `oracle.encoder_ref.embed` in float64 on the fp16-held weights, the
switch-off rows as the control: abs err <= 1.5 x control + 2 ulp(fp16 at max|ref|), and 1 - cos <= 1.5 x control + (2^-9)^2."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import test_gpu_encoder_ops_parity as P
from oracle import encoder_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16 = torch.float16
NAN = float("nan")

FLOOR = 2.0 ** -13
ATOL = 2.0 ** -15
CEIL_OUT_BLOCK = 2.0 ** -10
CEIL_OUT_ROW = 2.0 ** -9
LSE_TOL = 2.0 ** -11
ROUNDOFF = 2.0 ** -10

LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 512, 1000]
SHAPES = [(64, 8, 2), (128, 4, 1), (64, 4, 4), (64, 4, 2), (128, 8, 1)]     # (head_dim, query heads, kv heads): groups 4, 4, 1, 2, 8
HARD_LENS = [1, 17, 200, 65]
STEP = 32                                                                   # keys per step of causal_attn_fwd_f16_kernel


def ops():
    from rankpo_amd import ops as o
    return o


# ------------------------------------------------------------------------------------------------
# references, controls, the metric
# ------------------------------------------------------------------------------------------------
def _cu(lens):
    return torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32, device=DEV)


def _visible(lq, lk):
    i = torch.arange(lq, device=DEV)[:, None]
    j = torch.arange(lk, device=DEV)[None, :]
    return j <= i + (lk - lq)


def _ref_attn(q, k, v, lens_q, lens_k, scale):
    """float64 per sequence on the device, explicit bottom-right aligned mask: (out [Tq, nh, hd], lse [nh, Tq])."""
    G = q.shape[1] // k.shape[1]
    outs, lses, oq, ok = [], [], 0, 0
    for lq, lk in zip(lens_q, lens_k):
        qs = q[oq:oq + lq].double()
        kd, vd = k[ok:ok + lk].double().repeat_interleave(G, 1), v[ok:ok + lk].double().repeat_interleave(G, 1)
        s = torch.einsum("qhd,khd->hqk", qs, kd) * scale
        s = s.masked_fill(~_visible(lq, lk), -math.inf)
        lse = torch.logsumexp(s, -1)
        outs.append(torch.einsum("hqk,khd->qhd", torch.exp(s - lse[..., None]), vd))
        lses.append(lse)
        oq, ok = oq + lq, ok + lk
    return torch.cat(outs), torch.cat(lses, 1)


def _control(q, k, v, lens_q, lens_k, scale):
    """What the switch-off path runs on the same fp16 tensors, where it accepts the form; else None."""
    flash = torch.ops.aten._flash_attention_forward
    cu_k = _cu(lens_k)
    if list(lens_q) == list(lens_k):
        return flash(q.contiguous(), k.contiguous(), v.contiguous(), cu_k, cu_k, max(lens_k), max(lens_k), 0.0, True, False,
                     scale=scale)[0].double()
    if all(n == 1 for n in lens_q):
        cu_q = torch.arange(len(lens_q) + 1, dtype=torch.int32, device=DEV)
        return flash(q.contiguous(), k.contiguous(), v.contiguous(), cu_q, cu_k, 1, max(lens_k), 0.0, False, False,
                     scale=scale)[0].double()
    return None


def _seg(x2, cu):
    cs = torch.cat([torch.zeros_like(x2[:1]), x2.cumsum(0)], 0)
    return cs[cu[1:].long()] - cs[cu[:-1].long()]


def _block_err(a, r, cu, rows=False):
    """Relative Frobenius error per (sequence, head) block [N, H] or per (token, head) row [T, H]; the denominator is at least ATOL
    per element."""
    d2 = (a.double() - r).pow(2).sum(-1)
    r2 = r.pow(2).sum(-1)
    hd = r.shape[-1]
    if rows:
        return d2.sqrt() / r2.sqrt().clamp_min(ATOL * math.sqrt(hd))
    cnt = _seg(torch.ones_like(r2), cu)
    return _seg(d2, cu).sqrt() / _seg(r2, cu).sqrt().clamp_min(ATOL * (cnt * hd).sqrt())


def _check_out(label, out, ref, ctrl, cu):
    assert torch.isfinite(out).all(), label
    e = _block_err(out, ref, cu)
    if ctrl is not None and not torch.isfinite(ctrl).all():
        print(f"\n{label}: the control op returned non-finite values on these inputs: no control, the ceiling applies")
        ctrl = None
    if ctrl is not None:
        ec = _block_err(ctrl, ref, cu)
        bound = 1.5 * ec + FLOOR
        print(f"\n{label}: worst block: kernel {float(e.max()):.3e}, control {float(ec.max()):.3e}; "
              f"worst kernel / bound {float((e / bound).max()):.3f}")
    else:
        bound = torch.full_like(e, CEIL_OUT_BLOCK)
        print(f"\n{label}: worst block: kernel {float(e.max()):.3e}, no control, ceiling {CEIL_OUT_BLOCK:.3e}")
    assert bool((e <= bound).all()), (label, "blocks", float((e / bound).max()))
    er = _block_err(out, ref, cu, rows=True)
    print(f"{label}: worst row: kernel {float(er.max()):.3e}, ceiling {CEIL_OUT_ROW:.3e}")
    assert bool((er <= CEIL_OUT_ROW).all()), (label, "rows", float(er.max()))


def _check_lse(label, lse, ref):
    assert lse.dtype == torch.float32
    tol = LSE_TOL + 2.0 ** -16 * ref.abs()
    err = (lse.double() - ref).abs()
    print(f"{label} lse: worst |err| {float(err.max()):.3e}")
    assert bool((err <= tol).all()), (label, float((err - tol).max()))


def _run(q, k, v, lens_q, lens_k, scale, want_lse=True):
    o = ops()
    tiles = o.causal_attn_f16_tile_table(lens_q, lens_k, DEV)
    out, lse = o.causal_attn_f16(q, k, v, _cu(lens_q), _cu(lens_k), tiles, scale, want_lse=want_lse)
    assert out.dtype == F16 and out.shape == (q.shape[0], q.shape[1] * q.shape[2])
    return out.view(q.shape), lse


def _check_attn(q, k, v, lens_q, lens_k, scale, label):
    out, lse = _run(q, k, v, lens_q, lens_k, scale)
    assert lse.shape == (q.shape[1], q.shape[0])
    out2, none = _run(q, k, v, lens_q, lens_k, scale, want_lse=False)          # lse NULL: the same rows, bit for bit
    assert none is None and torch.equal(out, out2), label
    ref, ref_lse = _ref_attn(q, k, v, lens_q, lens_k, scale)
    _check_out(label, out, ref, _control(q, k, v, lens_q, lens_k, scale), _cu(lens_q))
    _check_lse(label, lse, ref_lse)
    return out, lse, ref


def _views(qkv, nh, nkv, hd):
    T, nq, nk = qkv.shape[0], nh * hd, nkv * hd
    return qkv[:, :nq].view(T, nh, hd), qkv[:, nq:nq + nk].view(T, nkv, hd), qkv[:, nq + nk:].view(T, nkv, hd)


def _fused(T, nh, nkv, hd, gen, mult=1.0):
    """q / k / v as column blocks of ONE [T, (nh + 2 nkv) hd] fp16 buffer (the fused projection output)."""
    qkv = (torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV) * mult).to(F16)
    return qkv, _views(qkv, nh, nkv, hd)


@functools.lru_cache(maxsize=None)
def _self_case(hd, nh, nkv):
    """One packed batch per shape and its self-attention result: computed once, shared by the tests below, never modified."""
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh * 10 + nkv)
    qkv, (q, k, v) = _fused(sum(LENS), nh, nkv, hd, gen)
    stride = (nh + 2 * nkv) * hd
    assert q.stride(0) == k.stride(0) == v.stride(0) == stride and q.dtype == F16 and not q.is_contiguous()
    assert q.data_ptr() == qkv.data_ptr() and k.data_ptr() == qkv.data_ptr() + 2 * nh * hd
    assert v.data_ptr() == k.data_ptr() + 2 * nkv * hd
    scale = 1.0 / math.sqrt(hd)
    out, lse, ref = _check_attn(q, k, v, LENS, LENS, scale, f"self hd{hd} nh{nh} nkv{nkv}")
    return q, k, v, scale, out, lse, ref


# ------------------------------------------------------------------------------------------------
# the kernel against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_causal_attention_f16_matches_f64(hd, nh, nkv):
    _self_case(hd, nh, nkv)


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_last_query_form(hd, nh, nkv):
    """One query per sequence (its last token) over the same K / V, against the non-causal control; the rows are those of the
    self-attention call: within ROUNDOFF, and bit for bit (both forms walk the key steps from key 0)."""
    q, k, v, scale, out, lse, ref = _self_case(hd, nh, nkv)
    last = torch.tensor(np.cumsum(LENS) - 1, device=DEV)
    ql = q.reshape(q.shape[0], -1).index_select(0, last).view(-1, nh, hd)
    ones = [1] * len(LENS)
    o1, l1, _ = _check_attn(ql, k, v, ones, LENS, scale, f"last query hd{hd} nh{nh} nkv{nkv}")
    want = out.index_select(0, last)
    e = _block_err(o1, want.double(), _cu(ones))
    assert bool((e <= ROUNDOFF).all()), float(e.max())
    assert torch.equal(o1, want) and torch.equal(l1, lse.index_select(1, last))


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_bottom_right_alignment(hd, nh, nkv):
    """lens_q[n] = ceil(lens_k[n] / 3), the queries being the last lq rows' q of each sequence: against float64 with the explicit
    mask under the block ceiling (no control takes the form), and against the same rows of the self-attention call."""
    q, k, v, scale, out, lse, _ = _self_case(hd, nh, nkv)
    lens_q = [-(-n // 3) for n in LENS]
    assert max(lens_q) > 256 and any(n % 32 for n in lens_q)
    ends = np.cumsum(LENS)
    idx = torch.cat([torch.arange(e - lq, e) for e, lq in zip(ends, lens_q)]).to(DEV)
    qs = q.reshape(q.shape[0], -1).index_select(0, idx).view(-1, nh, hd)
    assert _control(qs, k, v, lens_q, LENS, scale) is None
    o1, l1, _ = _check_attn(qs, k, v, lens_q, LENS, scale, f"bottom-right hd{hd} nh{nh} nkv{nkv}")
    want = out.index_select(0, idx)
    e = _block_err(o1, want.double(), _cu(lens_q))
    assert bool((e <= ROUNDOFF).all()), float(e.max())
    assert torch.equal(o1, want) and torch.equal(l1, lse.index_select(1, idx))


def test_long_sequence():
    """More than 128 key steps."""
    gen = torch.Generator(device=DEV).manual_seed(4100)
    lens = [4100, 3]
    assert lens[0] > 128 * STEP
    _, (q, k, v) = _fused(sum(lens), 4, 1, 64, gen)
    _check_attn(q, k, v, lens, lens, 0.125, "4100 keys")


# ------------------------------------------------------------------------------------------------
# hard inputs
# ------------------------------------------------------------------------------------------------
def _logits(q, k, scale, tq, h, hk, keys):
    return (k[keys, hk].double() @ q[tq, h].double()) * scale


def _regime_inputs(hd, nh, nkv, lens, regime, seed, spike_steps=None):
    """The regimes of tests/test_gpu_attention_parity.py (`make_inputs`) on fp16 storage, as column blocks of one fused buffer.
    spike: per (sequence, kv head hk) the key at the FIRST key of key step spike_steps[hk] (32-key steps, "last": the sequence's
    last step) carries a logit ~28 above the rest for two rows in three of the group's even q heads; growing: the keys grow by
    1 + pos / 12 (that file's 1 + pos / 60 over its 700 tokens, brought to the 200 of this file's longest row)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    T, G = sum(lens), nh // nkv
    scale = hd ** -0.5
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    pos = torch.cat([torch.arange(n, dtype=torch.float32) for n in lens]).to(DEV)
    q, k, v = rn(T, nh, hd), rn(T, nkv, hd), rn(T, nkv, hd)
    spikes, c = [], hd // 2 - 1
    if regime in ("spike", "sink"):
        for t in (q, k):
            t[..., c] = 0.0
            t[..., c + hd // 2] = 0.0
    if regime == "spike":
        a = float(torch.tensor(math.sqrt(28.0 / scale)).half())
        o0 = 0
        for si, n in enumerate(lens):
            for hk in range(nkv):
                sel = spike_steps[hk]
                j = ((n - 1) // STEP) * STEP if sel == "last" else sel * STEP
                if j < n:
                    k[o0 + j, hk, c] = a
                    rows = torch.arange(j, n, device=DEV)
                    rows = rows[(rows - j) % 3 != 1]
                    heads = [hk * G + x for x in range(G) if x % 2 == 0]
                    for h in heads:
                        q[o0 + rows, h, c] = a
                    spikes.append((si, o0, n, hk, j, rows, heads, sel))
            o0 += n
    elif regime == "sink":
        a = float(torch.tensor(math.sqrt(22.0 / scale)).half())
        first = torch.tensor([0] + list(np.cumsum(lens))[:-1], device=DEV)
        k[first, :, c] = a
        q[..., c] = a
    elif regime == "growing":
        q = q * 2.0 + 1.5
        k = (k * 0.3 + 0.4) * (1.0 + pos / 12.0)[:, None, None]
    elif regime == "negative":
        q = q * 0.5 + 1.5
        k = k * 0.2 - 8.0
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).to(F16).contiguous()
    return qkv, spikes


def _assert_regime(regime, q, k, nh, nkv, lens, spikes, ref_lse, scale):
    if regime == "spike":
        for si, o0, n, hk, j, rows, heads, sel in spikes:
            for i in rows[:: max(1, len(rows) // 4)].tolist()[:5]:
                s = _logits(q, k, scale, o0 + i, heads[-1], hk, torch.arange(o0, o0 + i + 1, device=DEV))
                others = torch.cat([s[:j], s[j + 1:]])
                if others.numel():
                    assert float(s[j] - others.max()) > 20.0, (si, hk, j, i)      # the spike dominates the row ...
                if j > 0:
                    assert float(s[j] - s[:j].max()) > 20.0                       # ... and the running maximum jumps at step j / 32
    elif regime == "sink":
        o0 = 0
        for si, n in enumerate(lens):
            if n > 1:
                for i in (1, n // 2, n - 1):
                    for h in (0, nh - 1):
                        s = _logits(q, k, scale, o0 + i, h, h // (nh // nkv), torch.arange(o0, o0 + i + 1, device=DEV))
                        assert float(s[0] - s[1:].max()) > 10.0, (si, i, h)
            o0 += n
    elif regime == "growing":
        assert float(ref_lse.max() - ref_lse.min()) > 50.0
    else:
        assert regime == "negative" and float(ref_lse.max()) < -50.0


@pytest.mark.parametrize("hd", [64, 128])
def test_hard_inputs(hd):
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    # saturated softmax: scores ~ +-60 after scaling (one key per query dominates)
    mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
    qkv = torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV)
    qkv[:, :(nh + nkv) * hd] *= mult
    q, k, v = _views(qkv.to(F16), nh, nkv, hd)
    _, _, ref = _check_attn(q, k, v, lens, lens, scale, f"saturated hd{hd}")
    s = torch.einsum("qhd,khd->hqk", q[-65:].double(), k[-65:].double().repeat_interleave(2, 1)) * scale
    assert float(s.abs().max()) > 60.0 and float(s.std()) > 30.0
    # raw q . k beyond the fp16 range: a kernel that rounds S to fp16 sees inf
    qkv = torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV)
    qkv[:, :(nh + nkv) * hd] *= 100.0
    q, k, v = _views(qkv.to(F16), nh, nkv, hd)
    raw = torch.einsum("qhd,khd->hqk", q[18:218].double(), k[18:218].double().repeat_interleave(2, 1))
    raw = raw.masked_fill(~_visible(200, 200), 0.0)
    assert float(raw.abs().max()) > 65504.0 and float(q.float().abs().max()) < 65504.0       # among the VISIBLE pairs
    _check_attn(q, k, v, lens, lens, scale, f"raw scores beyond fp16 hd{hd}")
    # identical keys: uniform weights over the visible keys, the output is the running mean of V
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen)
    k = k[:1].expand(T, nkv, hd).contiguous()
    _, _, ref = _check_attn(q, k, v, lens, lens, scale, f"identical keys hd{hd}")
    mean, o0 = [], 0
    for n in lens:
        mean.append(v[o0:o0 + n].double().cumsum(0) / torch.arange(1, n + 1, device=DEV)[:, None, None])
        o0 += n
    assert (ref - torch.cat(mean).repeat_interleave(nh // nkv, 1)).abs().max().item() < 1e-12
    # V at 0.9 x 65504 in one column: a mean of such values is finite, and so must the kernel's row be
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen)
    v = v.contiguous()
    v[:, :, 3] = 0.9 * 65504.0
    out, _, ref = _check_attn(q, k, v, lens, lens, scale, f"large V hd{hd}")
    assert float(ref.abs().max()) < 65504.0 and float(ref[..., 3].min()) > 0.89 * 65504.0 and torch.isfinite(out).all()


@pytest.mark.parametrize("regime", ["spike", "sink", "growing", "negative"])
@pytest.mark.parametrize("hd", [64, 128])
def test_regimes(hd, regime):
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = hd ** -0.5
    hit = set()
    for steps in ([(0, 1), (5, "last")] if regime == "spike" else [None]):
        qkv, spikes = _regime_inputs(hd, nh, nkv, lens, regime, 100 + hd + len(regime), steps)
        q, k, v = _views(qkv, nh, nkv, hd)
        ref_lse = _ref_attn(q, k, v, lens, lens, scale)[1]
        _assert_regime(regime, q, k, nh, nkv, lens, spikes, ref_lse, scale)
        hit |= {(sp[7], sp[4]) for sp in spikes}
        _check_attn(q, k, v, lens, lens, scale, f"{regime} {steps} hd{hd}")
    if regime == "spike":                       # the first key of key step 0, 1, 5 and the last (the 200-token row: key 192)
        assert {(0, 0), (1, 32), (5, 160), ("last", 192)} <= hit, hit


@pytest.mark.parametrize("hd", [64, 128])
def test_future_keys_do_not_leak(hd):
    """Every key behind position P = n // 2 of its sequence is multiplied by 1001.  A query at a position <= P sees none of them:
    its row and its lse are BIT-equal to those of the unmodified call.  The rows behind P differ."""
    gen = torch.Generator(device=DEV).manual_seed(70 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = 1.0 / math.sqrt(hd)
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    out, lse, _ = _check_attn(q, k, v, lens, lens, scale, f"leak base hd{hd}")
    pos = torch.cat([torch.arange(n, device=DEV) for n in lens])
    Pm = torch.cat([torch.full((n,), n // 2, device=DEV) for n in lens])           # 0, 8, 100, 32
    behind = pos > Pm
    assert behind.sum() > 100
    k2 = (k.float() * (1 + 1000 * behind[:, None, None].float())).to(F16).contiguous()
    assert torch.isfinite(k2).all() and float(k2.float().abs().max()) > 1000.0
    out2, lse2 = _run(q, k2, v, lens, lens, scale)
    assert torch.isfinite(out2).all() and torch.isfinite(lse2).all()
    assert torch.equal(out2[~behind], out[~behind]) and torch.equal(lse2[:, ~behind], lse[:, ~behind])
    assert not torch.equal(out2[behind], out[behind])


@pytest.mark.parametrize("hd,nh,nkv", [(64, 8, 2), (128, 4, 1)])
def test_packing_independence(hd, nh, nkv):
    """A sequence's rows are bit-equal whether it is packed alone, first or last among others."""
    gen = torch.Generator(device=DEV).manual_seed(5 + hd)
    scale = 1.0 / math.sqrt(hd)
    n, others = 77, [33, 200, 1]
    _, (q, k, v) = _fused(n + sum(others), nh, nkv, hd, gen)
    first, lse_f = _run(q, k, v, [n] + others, [n] + others, scale)
    alone, lse_a = _run(q[:n], k[:n], v[:n], [n], [n], scale)
    order = torch.cat([torch.arange(n, n + sum(others)), torch.arange(n)]).to(DEV)
    ql, kl, vl = (t.index_select(0, order) for t in (q, k, v))
    last, lse_l = _run(ql, kl, vl, others + [n], others + [n], scale)
    assert torch.equal(first[:n], alone) and torch.equal(last[-n:], alone)
    assert torch.equal(lse_f[:, :n], lse_a) and torch.equal(lse_l[:, -n:], lse_a)
    assert torch.equal(last[:-n], first[n:])


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refuses_what_it_cannot_run():
    """RPO_ERR_UNSUPPORTED before any launch: the buffers here are far smaller than what the refused shapes would read."""
    from rankpo_amd import _lib
    lib = _lib.load()
    OK, UNS = 0, -2
    st = torch.cuda.current_stream().cuda_stream
    xf = torch.zeros(4096 * 8, dtype=F16, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    p = xf.data_ptr()

    def attn(q=p, k=p, v=p, stride=256, tl=tiles, cols=2, qb=32, nh=2, nkv=1, hd=64, out=p + 4096 * 2, n=1):
        return lib.rpo_causal_attn_fwd_f16(q, k, v, stride, stride, stride, cu.data_ptr(), cu.data_ptr(), tl.data_ptr(), n,
                                           cols, qb, 1, nh, nkv, hd, 0.1, out, 128, None, st)
    assert attn() == OK                                        # the checks below do not refuse everything
    assert attn(n=0) == OK                                     # an empty work list: nothing to launch
    assert attn(hd=32) == UNS
    assert attn(hd=96, stride=768) == UNS
    assert attn(nh=3, nkv=2) == UNS                            # nh % nkv
    assert attn(nh=3, nkv=1) == UNS                            # 3 query heads per kv head
    assert attn(nh=16, nkv=1, stride=4096) == UNS              # 16
    assert attn(tl=tiles3, cols=3) == UNS                      # another table format
    assert attn(qb=64) == UNS and attn(qb=128) == UNS
    assert attn(q=p + 8) == UNS and attn(k=p + 8) == UNS and attn(v=p + 2) == UNS      # misaligned q / k / v
    assert attn(out=p + 4096 * 2 + 8) == UNS                   # misaligned out
    assert attn(stride=260) == UNS                             # a token stride that is no multiple of 8 elements
    torch.cuda.synchronize()


def test_wrapper_refuses_what_the_entry_refuses():
    o = ops()
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    q = torch.zeros(4, 2, 64, device=DEV, dtype=F16)
    assert o.causal_attn_f16_ok(q, q[:, :1], q[:, :1]) and o.causal_attn_f16_ok(q, q, q)
    for bad in (q.float(), q.bfloat16(), q.cpu()):
        assert not o.causal_attn_f16_ok(bad, bad, bad)
        with pytest.raises(ValueError):
            o.causal_attn_f16(bad, bad, bad, cu, cu, tiles, 0.1)
    q32 = torch.zeros(4, 3, 32, device=DEV, dtype=F16)
    assert not o.causal_attn_f16_ok(q32, q32, q32)
    q3 = torch.zeros(4, 3, 64, device=DEV, dtype=F16)
    assert not o.causal_attn_f16_ok(q3, q3[:, :1], q3[:, :1]) and not o.causal_attn_f16_ok(q3, q3[:, :2], q3[:, :2])
    odd = torch.zeros(4, 2 * 64 + 4, device=DEV, dtype=F16)[:, :128].view(4, 2, 64)         # token stride 132
    assert odd.stride(0) == 132 and not o.causal_attn_f16_ok(odd, odd, odd)
    with pytest.raises(ValueError):
        o.causal_attn_f16(odd, odd, odd, cu, cu, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16(q32, q32, q32, cu, cu, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16(q, q, q, cu, cu, torch.zeros(1, 3, dtype=torch.int32, device=DEV), 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f16_tile_table([5], [4], DEV)
    # the row-kernel gates: closed for fp16 outside the pass, open inside it under no-grad only
    x = torch.zeros(3, 128, device=DEV, dtype=F16)
    assert not o.fused_encoder_ops_ok(x) and not o.fused_norm_ok(x)
    with o.fp16_native():
        assert not o.fused_encoder_ops_ok(x) and not o.fused_norm_ok(x)            # grad mode is on
        with torch.no_grad():
            assert o.fused_encoder_ops_ok(x) and o.fused_encoder_ops_ok(x, 64) and o.fused_norm_ok(x)
            assert not o.fused_encoder_ops_ok(x, 24) and not o.fused_norm_ok(x[:, :100])
            assert not o.fused_norm_ok(torch.zeros(1, 8192, device=DEV, dtype=F16))
    with torch.no_grad():
        assert not o.fused_encoder_ops_ok(x) and not o.fused_norm_ok(x)


# ------------------------------------------------------------------------------------------------
# the row kernels in fp16
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def fp16_entries(monkeypatch):
    """The fp16 entries of the shared error model, for the duration of one test."""
    for table, val in ((P.U_STORE, 2.0 ** -11), (P.P_BITS, 11), (P.VEC, 8), (P.FLOOR, 2.0 ** -13)):
        monkeypatch.setitem(table, F16, val)


def _half_ulp16(a):
    """1/2 ulp of fp16 at float64 magnitudes a: 2^-25 below the normal range (2^-14)."""
    _, e = torch.frexp(a)
    e = torch.where(a == 0, torch.full_like(e, -13), e.clamp(min=-13))
    return torch.ldexp(torch.ones_like(a), e - 12)


def _check_elem16(name, out, ref, bound):
    """P.check_elem with fp16's subnormal spacing: |out - ref| <= bound + 1/2 ulp per element; NaN / inf fail."""
    o = out.double()
    tol = bound + _half_ulp16(torch.maximum(ref.abs(), o.abs().nan_to_num(0.0, 0.0, 0.0)))
    err = (o - ref).abs()
    bad = ~(err <= tol)
    assert not bad.any(), (name, int(bad.sum()), float((err / tol).nan_to_num(float("inf")).max()))


@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "plain"])
@pytest.mark.parametrize("rows", [1, 5, 8193])
@pytest.mark.parametrize("d", [200, 520, 2048, 4096])
def test_add_rmsnorm_fwd_f16(fp16_entries, rows, d, with_delta):
    """rstd, y per row against float64 and the f32-arithmetic bound, y against F.rms_norm as the control, x + delta rounded once."""
    assert {P.norm_kmax(F16, x) for x in (200, 520, 2048, 4096)} == {1, 2, 4, 8}
    P._norm_parity(F16, rows, d, with_delta, False, seed=rows + d, backward=False)


ROPE_F16 = [(64, 6), (128, 8), (128, 40)]


@pytest.mark.parametrize("hd,heads", ROPE_F16)
def test_rope_fwd_f16(fp16_entries, hd, heads):
    """The forward rotation with packed tables (one row per token, positions up to 131 071), out of place (NaN-prefilled) and in
    place; the backward rotation has no fp16 entry and is refused."""
    assert {P.rope_mapping(F16, h, n) for h, n in ROPE_F16} >= {"rows-per-block+idle", "rows-per-block", "strided"}
    lib = P._lib()
    _dt, _stream = P._abi()
    g = P._gen(hd * 100 + heads)
    rows = 307
    pos = torch.randint(0, P.ROPE_MAX_POS + 1, (rows,), device=DEV, generator=g)
    pos[0], pos[1] = P.ROPE_MAX_POS, 0
    cos, sin = P.rope_tables(pos, hd)
    extra = 2 * hd
    row_len = heads * hd + extra
    x = torch.randn(rows, row_len, device=DEV, generator=g).to(F16)
    ref, terms = P.rope_ref(x, cos, sin, heads, hd, 1.0)
    out = torch.full_like(x, NAN)
    assert lib.rpo_rope(x.data_ptr(), out.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, rows, _dt(x), 0,
                        _stream(x)) == 0
    xi = x.clone()
    assert lib.rpo_rope(xi.data_ptr(), xi.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, rows, _dt(x), 0,
                        _stream(x)) == 0
    nope = torch.full_like(x, NAN)
    assert lib.rpo_rope(x.data_ptr(), nope.data_ptr(), row_len, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, rows, _dt(x), 1,
                        _stream(x)) != 0
    torch.cuda.synchronize()
    assert nope.isnan().all()
    for name, t in (("out of place", out), ("in place", xi)):
        _check_elem16(f"rope fp16 {name}", t[:, :heads * hd].reshape(ref.shape), ref, 2 * P.U * terms)
    assert torch.equal(xi[:, :heads * hd], out[:, :heads * hd])
    assert out[:, heads * hd:].isnan().all() and torch.equal(xi[:, heads * hd:], x[:, heads * hd:])
    # sanity control: HF's formula with the tables rounded to the storage type, in the storage type
    c2 = torch.cat([cos, cos], -1).to(F16)[:, None]
    s2 = torch.cat([sin, sin], -1).to(F16)[:, None]
    xv = x[:, :heads * hd].view(rows, heads, hd)
    ctrl = xv * c2 + torch.cat([-xv[..., hd // 2:], xv[..., :hd // 2]], -1) * s2
    nref = P.row_norm(ref)
    P.check_control("rope fp16 fwd", P.row_norm(out[:, :heads * hd].double().view_as(ref) - ref) / nref,
                    P.row_norm(ctrl.double() - ref) / nref, F16)


@pytest.mark.parametrize("shape", P.SW_SHAPES, ids=[f"{r}x{c}{'-fused' if f else ''}" for r, c, f in P.SW_SHAPES])
@pytest.mark.parametrize("regime", P.SW_REGIMES)
def test_swiglu_fwd_f16(fp16_entries, shape, regime):
    lib = P._lib()
    _dt, _stream = P._abi()
    rows, cols, fused = shape
    gv, uv, ld_gu, _, _ = P._sw_inputs(F16, rows, cols, fused, regime, seed=rows + cols + len(regime))
    ref = P.swiglu_ref(gv, uv)
    ld_o = cols if fused else cols + 8
    ob, o = P._sw_out(rows, cols, ld_o, F16)
    assert lib.rpo_swiglu_fwd(gv.data_ptr(), uv.data_ptr(), o.data_ptr(), rows, cols, ld_gu, ld_o, _dt(gv), _stream(gv)) == 0
    torch.cuda.synchronize()
    r, bound = ref["prod"]
    _check_elem16(f"swiglu fp16 {regime}", o, r, bound)
    t = P.row_norm(ref["terms"]["prod"])
    ctrl = F.silu(gv) * uv
    P.check_control(f"swiglu fp16 {regime}", P.row_norm(o.double() - r) / t, P.row_norm(ctrl.double() - r) / t, F16)
    if not fused:
        assert ob[:, cols:].isnan().all(), "written beyond the columns of a row"


def test_row_kernels_inf_nan_reach_their_element_and_no_other(fp16_entries):
    lib = P._lib()
    _dt, _stream = P._abi()
    g = P._gen(3)
    rows, d = 6, 520
    # SwiGLU: elementwise
    gt = torch.randn(rows, d, device=DEV, generator=g).to(F16)
    ut = torch.randn(rows, d, device=DEV, generator=g).to(F16)
    gt[1, 7], ut[2, 9], gt[3, 500], ut[3, 500] = NAN, float("inf"), float("inf"), 1.0
    o = torch.full_like(gt, 0.0)
    assert lib.rpo_swiglu_fwd(gt.data_ptr(), ut.data_ptr(), o.data_ptr(), rows, d, d, d, _dt(gt), _stream(gt)) == 0
    bad = ~torch.isfinite(o)
    want = torch.zeros_like(bad)
    want[1, 7] = want[2, 9] = want[3, 500] = True
    assert torch.equal(bad, want) and o[1, 7].isnan() and o[3, 500] == float("inf")
    # RoPE: the pair (j, j + hd / 2) of one head of one row
    hd, heads = 64, 6
    x = torch.randn(rows, heads * hd, device=DEV, generator=g).to(F16)
    x[2, 3 * hd + 5] = float("inf")
    x[4, 1 * hd + 40] = NAN
    cos, sin = P.rope_tables(torch.arange(rows, device=DEV) + 1, hd)
    out = torch.empty_like(x)
    assert lib.rpo_rope(x.data_ptr(), out.data_ptr(), heads * hd, cos.data_ptr(), sin.data_ptr(), rows, heads, hd, rows, _dt(x), 0,
                        _stream(x)) == 0
    bad = ~torch.isfinite(out)
    want = torch.zeros_like(bad)
    want[2, 3 * hd + 5] = want[2, 3 * hd + 37] = want[4, 1 * hd + 40] = want[4, 1 * hd + 8] = True
    assert torch.equal(bad, want)
    # RMSNorm: the row (a reduction), and no other row
    x = torch.randn(rows, d, device=DEV, generator=g).to(F16)
    x[1, 3], x[4, 519] = float("inf"), NAN
    w = torch.ones(d, device=DEV, dtype=F16)
    rc, _, y, rstd = P._norm_fwd(x, None, w)
    torch.cuda.synchronize()
    assert rc == 0
    clean = [0, 2, 3, 5]
    assert torch.isfinite(y[clean]).all() and torch.isfinite(rstd[clean]).all()
    assert y[4].isnan().all() and rstd[4].isnan() and not torch.isfinite(y[1, 3]) and rstd[1] == 0


# ------------------------------------------------------------------------------------------------
# end to end: ModelForInference.encode on an fp16 Llama encoder
# ------------------------------------------------------------------------------------------------
def _errors(got, ref):
    got, ref = got.double(), ref.double()
    cos = (got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))
    return float((1 - cos).abs().max()), float((got - ref).abs().max())


def _ulp2_f16(ref):
    """2 ulp of fp16 at max|ref|."""
    return 2 * 2.0 ** (math.floor(math.log2(float(ref.abs().max()))) - 10)


def _build(hd, seed, **kw):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import CharTok, _cfg
    torch.manual_seed(seed)
    cfg = _cfg(PE, hd)
    enc = PE.LlamaEncoder(cfg)
    return PE, cfg, rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), device=0, **kw)


class Spy(TorchDispatchMode):
    """Counts the new op (full blocks / last-query form), the stock flash op (as the dispatcher sees it: the encoder calls it on
    torch.ops directly), F.rms_norm, the row-kernel wrappers, and host reads of device tensors."""

    def __init__(self):
        super().__init__()
        self.n = {"causal_attn_f16": 0, "full": 0, "last": 0, "flash": 0, "rms_norm": 0, "add_rmsnorm": 0, "rope_": 0, "swiglu": 0,
                  "syncs": 0}

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func is torch.ops.aten._flash_attention_forward.default:
            self.n["flash"] += 1
        return func(*args, **(kwargs or {}))

    def __enter__(self):
        o = ops()
        self._saved = (o.causal_attn_f16, o.add_rmsnorm, o.rope_, o.swiglu_down, F.rms_norm, torch.Tensor.tolist, torch.Tensor.item)

        def op(q, k, *a, **kw):
            self.n["causal_attn_f16"] += 1
            self.n["full" if q.shape[0] == k.shape[0] else "last"] += 1
            return self._saved[0](q, k, *a, **kw)

        def counted(key, fn):
            def f(*a, **kw):
                self.n[key] += 1
                return fn(*a, **kw)
            return f

        def host_read(fn):
            def f(t):
                self.n["syncs"] += int(t.is_cuda)
                return fn(t)
            return f
        o.causal_attn_f16 = op
        o.add_rmsnorm, o.rope_, o.swiglu_down = (counted("add_rmsnorm", self._saved[1]), counted("rope_", self._saved[2]),
                                                 counted("swiglu", self._saved[3]))
        F.rms_norm = counted("rms_norm", self._saved[4])
        torch.Tensor.tolist, torch.Tensor.item = host_read(self._saved[5]), host_read(self._saved[6])
        super().__enter__()
        return self

    def __exit__(self, *exc):
        super().__exit__(*exc)
        o = ops()
        (o.causal_attn_f16, o.add_rmsnorm, o.rope_, o.swiglu_down, F.rms_norm, torch.Tensor.tolist, torch.Tensor.item) = self._saved
        return False


KW = dict(batch_size=12, max_length=384)


@pytest.fixture(scope="module", params=[64, 128])
def f16_case(request):
    """One fp16 model per config (switch off), the same weights with native_fp16=True, the texts, the float64 oracle rows on the
    fp16-held weights and the switch-off rows (the control): computed once, shared by the tests below, never modified."""
    from test_gpu_inference import CharTok, _texts
    hd = request.param
    PE, cfg, inf = _build(hd, 20 + hd, use_fp16=True)
    _, _, inf_on = _build(hd, 20 + hd, use_fp16=True, native_fp16=True)
    sd, sd_on = inf.model.state_dict(), inf_on.model.state_dict()
    assert all(v.dtype == F16 and torch.equal(v, sd_on[k]) for k, v in sd.items())
    assert not inf.model.native_fp16 and inf_on.model.native_fp16 and not PE.LLAMA_FP16_NATIVE
    rs = np.random.RandomState(hd)
    texts = _texts(rs, 23, 40, 400) + ["q"] + _texts(rs, 8, 380, 400)        # 3 batches of 12 / 12 / 8; one 1-token row
    tok = CharTok()(texts, max_length=384)
    w64 = {k: v.detach().double().cpu() for k, v in sd.items()}
    with torch.no_grad():
        ref = E.embed(w64, cfg.to_dict(), tok, dtype=torch.float64).detach()
    assert ref.dtype == torch.float64
    off = inf.encode(texts, **KW)
    return dict(hd=hd, PE=PE, cfg=cfg, inf=inf, inf_on=inf_on, texts=texts, ref=ref, off=off)


def test_encode_switch_off_runs_what_it_ran(f16_case):
    c = f16_case
    with Spy() as spy:
        a = c["inf"].encode(c["texts"], **KW)
    n = spy.n
    assert n["causal_attn_f16"] == 0 and n["add_rmsnorm"] == 0 and n["rope_"] == 0 and n["swiglu"] == 0, n
    assert n["flash"] == 3 * c["cfg"].num_hidden_layers and n["rms_norm"] > 0 and n["syncs"] == 0, n
    np.testing.assert_array_equal(a, c["off"])
    with Spy():
        b = c["inf"].encode(c["texts"], **KW)
    np.testing.assert_array_equal(a, b)


def test_encode_native_fp16_vs_oracle(f16_case, monkeypatch):
    c = f16_case
    cfg, ref = c["cfg"], c["ref"]
    with Spy() as spy:
        out = c["inf_on"].encode(c["texts"], **KW)
    nb, nl = 3, cfg.num_hidden_layers
    n = spy.n
    assert n["causal_attn_f16"] == nb * nl and n["full"] == nb * (nl - 1) and n["last"] == nb, n
    assert n["flash"] == 0 and n["rms_norm"] == 0, n
    # per batch: 2 norms per block + the final norm; q|k|v rope per full block, q and k|v in the last; one SwiGLU per block
    assert n["add_rmsnorm"] == nb * (2 * nl + 1) and n["rope_"] == nb * (nl + 1) and n["swiglu"] == nb * nl, n
    assert n["syncs"] == 0, "encode() synchronised on a device tensor's contents"
    assert out.shape == (32, cfg.hidden_size) and np.isfinite(out).all()
    f_cos, f_abs = _errors(torch.tensor(out), ref)
    c_cos, c_abs = _errors(torch.tensor(c["off"]), ref)
    floor = _ulp2_f16(ref)
    print(f"\nencode fp16 llama hd{c['hd']}: native cos err {f_cos:.2e} abs {f_abs:.2e}; switch-off control {c_cos:.2e} / "
          f"{c_abs:.2e}; floor {floor:.2e}")
    assert f_abs <= 1.5 * c_abs + floor and f_cos <= 1.5 * c_cos + (2.0 ** -9) ** 2, (f_cos, c_cos, f_abs, c_abs)
    # the module switch on the switch-off model: the same path, the same rows
    monkeypatch.setattr(c["PE"], "LLAMA_FP16_NATIVE", True)
    with Spy() as spy:
        out_m = c["inf"].encode(c["texts"], **KW)
    assert spy.n["causal_attn_f16"] == nb * nl and spy.n["flash"] == 0 and spy.n["rms_norm"] == 0, spy.n
    np.testing.assert_array_equal(out_m, out)


def test_left_padded_batches_give_the_switch_off_rows(f16_case):
    from test_gpu_bert_native import LeftTok
    from test_gpu_inference import _texts
    c = f16_case
    texts = _texts(np.random.RandomState(8), 7, 5, 60)
    rows = []
    for inf in (c["inf_on"], c["inf"]):
        right = inf.tokenizer
        try:
            inf.tokenizer = LeftTok()
            with Spy() as spy:
                rows.append(inf.encode(texts, batch_size=4, max_length=64))
        finally:
            inf.tokenizer = right
        n = spy.n
        assert n["causal_attn_f16"] == 0 and n["add_rmsnorm"] == 0 and n["rope_"] == 0 and n["swiglu"] == 0, n    # the padded path
    np.testing.assert_array_equal(rows[0], rows[1])


def test_grad_mode_runs_what_it_ran(f16_case, monkeypatch):
    """Both switches on, grad mode: the new ops are not called; gradients finite and non-zero; bit-equal to the switch-off step if
    two switch-off steps are bit-equal to each other, else within 4 x the largest difference those two show (the switch-on step
    runs the same code as they do, so its distance from one of them is drawn from the distribution of their distance from each
    other: a bound AT one sample of that distance would fail every second run)."""
    from test_gpu_inference import CharTok, _texts
    c = f16_case
    tok = CharTok()(_texts(np.random.RandomState(9), 5, 3, 70) + ["q"], max_length=64)

    def step(inf):
        inf.model.zero_grad(set_to_none=True)
        with Spy() as spy:
            pooled = inf.model.pooled_last_token(tok["input_ids"], tok["attention_mask"])
            pooled.float().sum().backward()
        n = spy.n
        assert n["causal_attn_f16"] == 0 and n["add_rmsnorm"] == 0 and n["rope_"] == 0 and n["swiglu"] == 0 and n["flash"] > 0, n
        g = {k: p.grad.clone() for k, p in inf.model.named_parameters()}
        inf.model.zero_grad(set_to_none=True)
        return g
    off1, off2 = step(c["inf"]), step(c["inf"])
    monkeypatch.setattr(c["PE"], "LLAMA_FP16_NATIVE", True)
    on = step(c["inf_on"])
    assert on.keys() == off1.keys() and len(on) > 10
    assert all(torch.isfinite(g).all() for g in on.values()) and sum(float(g.float().abs().sum()) for g in on.values()) > 0
    if all(torch.equal(off1[k], off2[k]) for k in off1):
        for k in on:
            assert torch.equal(on[k], off1[k]), k
    else:
        for k in on:
            spread = float((off1[k].float() - off2[k].float()).abs().max())
            assert torch.allclose(on[k].float(), off1[k].float(), rtol=0.0, atol=4 * spread), k


@pytest.mark.parametrize("kw", [dict(use_bf16=True), dict()], ids=["bf16", "f32"])
def test_other_dtypes_ignore_the_switch(kw, monkeypatch):
    from test_gpu_inference import _texts
    texts = _texts(np.random.RandomState(8), 9, 5, 200)
    PE, cfg, inf = _build(64, 9, **kw)
    a = inf.encode(texts, batch_size=4, max_length=256)
    _, _, inf_on = _build(64, 9, native_fp16=True, **kw)
    monkeypatch.setattr(PE, "LLAMA_FP16_NATIVE", True)
    assert inf_on.model.native_fp16 and inf_on.model.embed_tokens.weight.dtype != F16
    with Spy() as spy:
        b = inf_on.encode(texts, batch_size=4, max_length=256)
    assert spy.n["causal_attn_f16"] == 0, spy.n
    np.testing.assert_array_equal(a, b)


def test_bert_model_accepts_and_ignores_the_keyword():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import CharTok, _texts
    texts = _texts(np.random.RandomState(8), 9, 5, 60)
    rows = []
    for kw in (dict(), dict(native_fp16=True)):
        torch.manual_seed(4)
        enc = PE.build_encoder(PE.bge_small_config(vocab_size=1024, hidden_size=128, intermediate_size=512, num_hidden_layers=2,
                                                   num_attention_heads=4))
        inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), device=0, use_fp16=True, **kw)
        assert not hasattr(inf.model, "native_fp16")
        with Spy() as spy:
            rows.append(inf.encode(texts, batch_size=4, max_length=64))
        assert spy.n["causal_attn_f16"] == 0
    np.testing.assert_array_equal(rows[0], rows[1])
