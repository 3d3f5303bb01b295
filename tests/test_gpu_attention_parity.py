"""Float64 parity of every shipped attention kernel variant, on the inputs where online-softmax kernels go wrong.

The hand-written causal varlen attention (forward, dQ, dK/dV, rotary fold) and the last-query attention are compared with a
float64 reference of the same operation on the EXACT bf16 inputs (upcast, never re-rounded), computed on the GPU one
(sequence, kv head) at a time.  Errors are measured per (sequence, head) block -- and per row for the forward output -- as a
relative Frobenius error, never against a bound scaled by a tensor's global maximum: a bug confined to one block or one row
shows however large the rest of the tensor is.

References.  The forward output is compared with float64 attention on the un-rotated input (rotary applied in float64).  The
forward kernel's lse and every backward are compared with float64 on exactly what the backward kernels read: the attention's own
bf16 q / k / v and that forward kernel's bf16 output and f32 lse (delta = rowsum(dO o out) is part of the operation; taken from
an exact output instead, the bf16 rounding of out turns into random 1-3 % errors on short rows, where dS cancels).

Bounds.  Where PyTorch's flash-attention ops accept the shape, they run on the same inputs as a CONTROL and every block must
satisfy  kernel error <= 1.5 x control error + FLOOR.  Where no control accepts the shape, and for single output rows, fixed
ceilings from the bf16 rounding budget apply (P is rounded to bf16 before P.V, l sums the rounded P, the result is rounded to bf16
once).  A gradient block that cancels far below the terms it sums (exactly zero for a one-token sequence) is judged against
RESOLUTION x the norm of those terms instead of its own norm.

Regimes (each asserts that its inputs reach it):
  flat      randn q / k / v: logits ~ N(0, 1);
  spike     per (sequence, kv head) one key at the FIRST key of key tile t in {0, 1, 5, last} carries a logit ~28 above the rest
            for chosen query rows of chosen q heads, so the running maximum jumps at a known tile (the forward's rescale branch);
  sink      key 0 of every sequence dominates every query by a logit gap >= 10 (P ~ 1 there and dS = P (dP - delta) cancels);
  growing   logits that keep growing along the sequence (lse spread > 50);
  negative  every logit far below zero (lse < -50): the running maximum must start at the data, not at 0.

Kernel variants are selected through `ops`' own A/B knobs with `monkeypatch` (ATTN_SWEEP_DOWN, ATTN_SWEEP_DOWN_HD128,
ATTN_GROUP_TAIL), never by a global left changed."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FLOOR = 2.0 ** -10          # additive floor of the control rule (a block where the control happens to be exact)
ATOL = 2.0 ** -12           # elements below this magnitude carry no relative meaning: the denominator's floor per element
RESOLUTION = 2.0 ** -10     # ... and a gradient block below 2^-10 x the norm of the terms it sums (bf16 dS resolves ~2^-9) neither
# fixed ceilings where no control accepts the shape, from the bf16 budget (unit roundoff u = 2^-8): the forward rounds P before
# P.V and the output once (2u per block, 4u for a single row); the backward rounds P before dP^T.dO and dS before dS.K / dS^T.Q
# (sums that cancel: dS sums to zero along a row) and each gradient once (8u)
CEIL_OUT_BLOCK = 2.0 ** -7
CEIL_OUT_ROW = 2.0 ** -6
CEIL_GRAD_BLOCK = 2.0 ** -5
LSE_TOL = 2.0 ** -8         # |lse - ref| <= LSE_TOL + 2^-16 |ref| (l sums bf16-rounded P: u relative at most)
ROUNDOFF = 2.0 ** -7        # two kernels that differ only in f32 summation order: bf16 round-off apart (per-block relative)

LENS_ALL = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 4095, 4096, 4097]
LENS_REGIME = [700, 333, 257, 129, 64, 17, 1]
GQA = [(8, 8), (6, 2), (10, 2), (12, 2), (28, 4), (16, 2)]
GAP = 28.0                  # spike logit above the rest
SINK_GAP = 16.0


def key_tile(hd):
    return 64 if hd == 64 else 32        # keys per tile of fa_fwd_kernel / of fa_fwd128_kernel and fa_fwd128w_kernel


# ---------------------------------------------------------------------------------------------------------------- reference
def _rot(x, c, s):
    """HF rotate_half layout: x * [c, c] + [-x2, x1] * [s, s]."""
    h = x.shape[-1] // 2
    return x * torch.cat([c, c], -1) + torch.cat([-x[..., h:], x[..., :h]], -1) * torch.cat([s, s], -1)


def _rot_t(g, c, s):
    """Transpose of `_rot` (the gradient w.r.t. the un-rotated input)."""
    h = g.shape[-1] // 2
    y = g * torch.cat([s, s], -1)
    return g * torch.cat([c, c], -1) + torch.cat([y[..., h:], -y[..., :h]], -1)


def fwd_ref(q, k, v, lens, scale, rope=None, last_query=False):
    """float64 attention on the exact bf16 inputs, one (sequence, kv head) at a time.  Causal: q [T, nh, hd]; last_query: q
    [N, nh, hd], one query per sequence that sees every key of it.  rope = (cos, sin) [T, hd / 2]: q and k are rotated here, in
    float64.  Returns out [Tq, nh, hd] and lse [nh, Tq]."""
    nh, nkv = q.shape[1], k.shape[1]
    G, f = nh // nkv, torch.float64
    out = torch.empty(q.shape, dtype=f, device=q.device)
    lse = torch.empty((nh, q.shape[0]), dtype=f, device=q.device)
    o0 = 0
    for si, n in enumerate(lens):
        rows = slice(si, si + 1) if last_query else slice(o0, o0 + n)
        for hk in range(nkv):
            hs = slice(hk * G, (hk + 1) * G)
            qq, kk, vv = q[rows, hs].to(f).transpose(0, 1), k[o0:o0 + n, hk].to(f), v[o0:o0 + n, hk].to(f)
            if rope is not None:
                c, sn = rope[0][o0:o0 + n].to(f), rope[1][o0:o0 + n].to(f)
                qq, kk = _rot(qq, c, sn), _rot(kk, c, sn)
            sc = (qq @ kk.T) * scale
            if not last_query:
                sc = sc.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=q.device).tril(), float("-inf"))
            ls = torch.logsumexp(sc, -1)
            out[rows, hs] = (torch.exp(sc - ls[..., None]) @ vv).transpose(0, 1)
            lse[hs, rows] = ls
        o0 += n
    return out, lse


def bwd_ref(q, k, v, go, out, lse, lens, scale, rope=None, last_query=False):
    """float64 attention BACKWARD on exactly what the backward kernels read: the attention's own bf16 q / k / v (rotated already
    when rope is given), dO, and the forward kernel's bf16 output and f32 lse [nh, Tq] (P = exp(scale q k^T - lse),
    delta = rowsum(dO o out), dS = P (dP - delta)).  rope = (cos, sin): dq / dk are rotated back (gradients w.r.t. the
    un-rotated q / k).  Returns the exact lse of these inputs [nh, Tq] (what the forward kernel's lse is checked against), dq, dk,
    dv, and the magnitudes of the terms each gradient element sums (|dS| taken before the cancellation of dP - delta), which
    set the resolution floor of `block_err`."""
    nh, nkv = q.shape[1], k.shape[1]
    G, f = nh // nkv, torch.float64
    dq = torch.empty(q.shape, dtype=f, device=q.device)
    dk, dv = torch.empty(k.shape, dtype=f, device=q.device), torch.empty(k.shape, dtype=f, device=q.device)
    lse_x = torch.empty((nh, q.shape[0]), dtype=f, device=q.device)
    mq, mk, mv = torch.empty_like(dq), torch.empty_like(dk), torch.empty_like(dv)
    o0 = 0
    for si, n in enumerate(lens):
        rows = slice(si, si + 1) if last_query else slice(o0, o0 + n)
        for hk in range(nkv):
            hs = slice(hk * G, (hk + 1) * G)
            qq, kk, vv = q[rows, hs].to(f).transpose(0, 1), k[o0:o0 + n, hk].to(f), v[o0:o0 + n, hk].to(f)
            gg, oo = go[rows, hs].to(f).transpose(0, 1), out[rows, hs].to(f).transpose(0, 1)
            sc = (qq @ kk.T) * scale
            if not last_query:
                sc = sc.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=q.device).tril(), float("-inf"))
            lse_x[hs, rows] = torch.logsumexp(sc, -1)
            p = torch.exp(sc - lse[hs, rows].to(f)[..., None])
            dp, delta = gg @ vv.T, (gg * oo).sum(-1, keepdim=True)
            ds, dsm = p * (dp - delta), p * (dp.abs() + delta.abs())
            dq[rows, hs] = (ds @ kk).transpose(0, 1) * scale
            dk[o0:o0 + n, hk] = (ds.transpose(1, 2) @ qq).sum(0) * scale
            dv[o0:o0 + n, hk] = (p.transpose(1, 2) @ gg).sum(0)
            mq[rows, hs] = (dsm @ kk.abs()).transpose(0, 1) * scale
            mk[o0:o0 + n, hk] = (dsm.transpose(1, 2) @ qq.abs()).sum(0) * scale
            mv[o0:o0 + n, hk] = (p.transpose(1, 2) @ gg.abs()).sum(0)
        o0 += n
    if rope is not None:
        c, sn = rope[0].to(f)[:, None], rope[1].to(f)[:, None]
        if not last_query:
            dq = _rot_t(dq, c, sn)
        dk = _rot_t(dk, c, sn)
    return lse_x, dq, dk, dv, (mq, mk, mv)


def _flash_args(lens, last_query, device):
    cu = torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=device)
    cu_q = torch.arange(len(lens) + 1, dtype=torch.int32, device=device) if last_query else cu
    return cu, cu_q, (1 if last_query else max(lens)), max(lens)


def fwd_control(q, k, v, lens, scale, rope=None, last_query=False):
    """PyTorch's flash-attention forward on the same bf16 inputs (rotary applied in float64 and rounded to bf16 once); None where
    the op refuses the shape."""
    cu, cu_q, mq, mk = _flash_args(lens, last_query, q.device)
    qc, kc = q.contiguous(), k.contiguous()
    if rope is not None:
        c, sn = rope[0].double()[:, None], rope[1].double()[:, None]
        qc, kc = _rot(q.double(), c, sn).to(torch.bfloat16), _rot(k.double(), c, sn).to(torch.bfloat16)
    try:
        return torch.ops.aten._flash_attention_forward(qc, kc, v.contiguous(), cu_q, cu, mq, mk, 0.0, not last_query, False,
                                                       scale=scale)[0].double()
    except RuntimeError:
        return None


def bwd_control(q, k, v, go, out, lse_padded, lens, scale, rope=None, last_query=False):
    """PyTorch's flash-attention backward on the same inputs as `bwd_ref` (lse in its [N, nh, max_q] layout), gradients rotated back
    in float64; None where the op refuses the shape."""
    cu, cu_q, mq, mk = _flash_args(lens, last_query, q.device)
    z = torch.zeros((), dtype=torch.int64, device=q.device)
    try:
        d = torch.ops.aten._flash_attention_backward(go.contiguous(), q.contiguous(), k.contiguous(), v.contiguous(),
                                                     out.contiguous(), lse_padded, cu_q, cu, mq, mk, 0.0, not last_query, z, z,
                                                     scale=scale)
    except RuntimeError:
        return None
    dq, dk, dv = d[0].double(), d[1].double(), d[2].double()
    if rope is not None:
        c, sn = rope[0].double()[:, None], rope[1].double()[:, None]
        dq, dk = (dq if last_query else _rot_t(dq, c, sn)), _rot_t(dk, c, sn)
    return dq, dk, dv


# ---------------------------------------------------------------------------------------------------------------- metric
def _seg(x2, cu):
    """x2 [T, H] -> per-segment sums [N, H]."""
    cs = torch.cat([torch.zeros_like(x2[:1]), x2.cumsum(0)], 0)
    return cs[cu[1:].long()] - cs[cu[:-1].long()]


def block_err(a, r, cu, rows=False, mag=None):
    """Relative Frobenius error per (sequence, head) block ([N, H]) or per (token, head) row ([T, H]).  The denominator is at
    least ATOL per element and, given the magnitudes `mag` of the terms the elements sum, RESOLUTION x their norm: a gradient
    that cancels far below its terms (a one-token sequence: exactly zero; a sink row) is judged against what a kernel that rounds
    dS to bf16 before the products can resolve."""
    d2 = (a.double() - r).pow(2).sum(-1)
    r2 = r.pow(2).sum(-1)
    m2 = mag.pow(2).sum(-1) * RESOLUTION ** 2 if mag is not None else torch.zeros_like(r2)
    hd = r.shape[-1]
    if rows:
        return d2.sqrt() / torch.maximum(r2, m2).sqrt().clamp_min(ATOL * math.sqrt(hd))
    cnt = _seg(torch.ones_like(r2), cu)
    return _seg(d2, cu).sqrt() / torch.maximum(_seg(r2, cu), _seg(m2, cu)).sqrt().clamp_min(ATOL * (cnt * hd).sqrt())


def check(name, got, ref, ctrl, cu, ceiling, rows=False, mag=None):
    """kernel <= 1.5 x control + FLOOR per block where a control exists, <= the fixed ceiling where none does."""
    e = block_err(got, ref, cu, rows, mag)
    bound = 1.5 * block_err(ctrl, ref, cu, rows, mag) + FLOOR if ctrl is not None else torch.full_like(e, ceiling)
    bad = e > bound
    if bad.any():
        i = int((e / bound).argmax())
        idx = np.unravel_index(i, tuple(e.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} {'rows' if rows else 'blocks'} over the bound; worst (seq/row, head) "
                             f"{tuple(int(x) for x in idx)}: error {e.flatten()[i]:.3e} > bound {bound.flatten()[i]:.3e}")
    return float((e / bound).max())


def check_lse(name, lse, ref, cols=None):
    ref = ref if cols is None else ref[:, cols]
    tol = LSE_TOL + 2.0 ** -16 * ref.abs()
    ok = (lse.double() - ref).abs() <= tol
    assert bool(ok.all()), (name, float(((lse.double() - ref).abs() - tol).max()))


def check_grads(tag, grads, B, BC, cu):
    """(dq, dk, dv) of one kernel variant against `bwd_ref` B and the control BC (or the fixed ceiling)."""
    return max(check(f"{tag} {name}", g, r, c, cu, CEIL_GRAD_BLOCK, mag=m)
               for name, g, r, c, m in zip(("dq", "dk", "dv"), grads, B[1:4], BC if BC is not None else (None,) * 3, B[4]))


def check_out(tag, out, ref, ctrl, cu, ref_rows=None):
    """Blocks by the control rule; single rows (64 / 128 elements: too few for a ratio of two implementations' rounding errors to
    be stable) against the fixed row ceiling, on `ref_rows`: the reference of the attention on the bf16 q / k it read (with the
    rotary fold, the rotated q / k are rounded to bf16 by design -- at logits of |s| ~ 100 that alone moves a softmax row by more
    than any bf16 attention budget; the block rule covers that rounding through the control, which rounds the same way)."""
    return max(check(f"{tag} out", out, ref, ctrl, cu, CEIL_OUT_BLOCK),
               check(f"{tag} out rows", out, ref if ref_rows is None else ref_rows, None, cu, CEIL_OUT_ROW, rows=True))


def roundoff_apart(name, a, b, cu):
    e = block_err(a, b.double(), cu)
    assert bool((e <= ROUNDOFF).all()), (name, float(e.max()))


# ---------------------------------------------------------------------------------------------------------------- inputs
def rope_tables(lens, hd, device):
    """Llama rotary tables for packed positions (theta 10000), f32 [T, hd / 2] (row t = token t, as the encoder passes them)."""
    pos = torch.cat([torch.arange(n, dtype=torch.float64) for n in lens]).to(device)
    inv = 10000.0 ** (-torch.arange(0, hd, 2, dtype=torch.float64, device=device) / hd)
    ang = pos[:, None] * inv[None]
    return ang.cos().float().contiguous(), ang.sin().float().contiguous()


def _logits(q, k, rope, scale, t_q, h, hk, keys):
    """float64 scaled logits of query token t_q (head h) against key tokens `keys` (kv head hk), rotary applied if given."""
    qq, kk = q[t_q, h].double(), k[keys, hk].double()
    if rope is not None:
        qq = _rot(qq, rope[0][t_q].double(), rope[1][t_q].double())
        kk = _rot(kk, rope[0][keys].double(), rope[1][keys].double())
    return (kk @ qq) * scale


def make_inputs(hd, nh, nkv, lens, regime, seed):
    """q [T, nh, hd], k / v [T, nkv, hd] as column views of ONE fused bf16 q|k|v buffer, dO, and the regime's record."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    T, G = sum(lens), nh // nkv
    scale = hd ** -0.5
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    pos = torch.cat([torch.arange(n, dtype=torch.float32) for n in lens]).to(DEV)
    q, k, v = rn(T, nh, hd), rn(T, nkv, hd), rn(T, nkv, hd)
    spikes = []
    c = hd // 2 - 1                     # the pair (c, c + hd / 2) turns slowest under the rotary: a spike survives the rotation
    if regime in ("spike", "sink"):
        for t in (q, k):
            t[..., c] = 0.0
            t[..., c + hd // 2] = 0.0
    if regime == "spike":
        a = float(torch.tensor(math.sqrt(GAP / scale)).bfloat16())
        BN = key_tile(hd)
        o0, case = 0, 0
        for si, n in enumerate(lens):
            for hk in range(nkv):
                t_sel = (0, 1, 5, "last")[case % 4]
                case += 1
                j = ((n - 1) // BN) * BN if t_sel == "last" else t_sel * BN
                if j >= n:
                    continue
                k[o0 + j, hk, c] = a
                rows = torch.arange(j, n, device=DEV)
                rows = rows[(rows - j) % 3 != 1]                      # two rows in three of those that see the spike
                heads = [hk * G + x for x in range(G) if x % 2 == 0]    # the group's even q heads (its first always)
                for h in heads:
                    q[o0 + rows, h, c] = a
                spikes.append((si, o0, n, hk, j, rows, heads, t_sel))
            o0 += n
    elif regime == "sink":
        a = float(torch.tensor(math.sqrt((SINK_GAP + 6.0) / scale)).bfloat16())
        first = torch.tensor([0] + list(np.cumsum(lens))[:-1], device=DEV)
        k[first, :, c] = a
        q[..., c] = a
    elif regime == "growing":
        q = q * 2.0 + 1.5
        k = (k * 0.3 + 0.4) * (1.0 + pos / 60.0)[:, None, None]
    elif regime == "negative":
        q = q * 0.5 + 1.5
        k = k * 0.2 - 8.0
    else:
        assert regime == "flat"
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], 1).to(torch.bfloat16).contiguous()
    go = rn(T, nh, hd).to(torch.bfloat16)
    return qkv, go, spikes


def views(x, nh, nkv, hd):
    nq, nk = nh * hd, nkv * hd
    return x[:, :nq].unflatten(1, (nh, hd)), x[:, nq:nq + nk].unflatten(1, (nkv, hd)), x[:, nq + nk:].unflatten(1, (nkv, hd))


def unrotate(qkv, nh, nkv, hd, rope):
    """The buffer whose rotation (by `rope`) is `qkv`: the rotary variants then see the regime's logits, not a rotated mix of them."""
    q, k, v = views(qkv, nh, nkv, hd)
    c, s = rope[0].double()[:, None], rope[1].double()[:, None]
    T = qkv.shape[0]
    return torch.cat([_rot_t(q.double(), c, s).reshape(T, -1), _rot_t(k.double(), c, s).reshape(T, -1), v.reshape(T, -1).double()],
                     1).to(torch.bfloat16).contiguous()


def assert_regime(regime, qkv, nh, nkv, hd, lens, spikes, R, rope=None):
    """The inputs reach the regime they are named after (on the reference's own logits)."""
    q, k, _ = views(qkv, nh, nkv, hd)
    scale = hd ** -0.5
    lse = R[1]
    if regime == "spike":
        BN = key_tile(hd)
        tiles_hit = set()
        for si, o0, n, hk, j, rows, heads, t_sel in spikes:
            for i in rows[:: max(1, len(rows) // 4)].tolist()[:5]:
                h = heads[-1]
                s = _logits(q, k, rope, scale, o0 + i, h, hk, torch.arange(o0, o0 + i + 1, device=DEV))
                others = torch.cat([s[:j], s[j + 1:]])
                if others.numel() == 0:
                    continue
                assert float(s[j] - others.max()) > 20.0, (si, hk, j, i)        # the spike dominates the row ...
                if j > 0:
                    assert float(s[j] - s[:j].max()) > 20.0                      # ... and the running max jumps at tile j / BN
            tiles_hit.add(t_sel)
        assert {0, 1, 5, "last"} <= tiles_hit, tiles_hit
    elif regime == "sink":
        o0 = 0
        for si, n in enumerate(lens):
            if n > 1:
                for i in (1, n // 2, n - 1):
                    for h in (0, nh - 1):
                        s = _logits(q, k, rope, scale, o0 + i, h, h // (nh // nkv), torch.arange(o0, o0 + i + 1, device=DEV))
                        assert float(s[0] - s[1:].max()) > 10.0, (si, i, h)
            o0 += n
    elif regime == "growing":
        assert float(lse.max() - lse.min()) > 50.0
    elif regime == "negative":
        assert float(lse.max()) < -50.0
    else:
        assert float(lse.abs().max()) < 15.0


# ---------------------------------------------------------------------------------------------------------------- runners
def grad_run(qkv, go, nh, nkv, hd, cu, tiles, k_tiles, key_block, rope=None, fwd_tiles=None):
    """The encoder's entry: ONE fused q|k|v buffer through flash_attn_varlen_qkv (rope None) or rope_flash_attn_varlen_qkv.
    Returns the output, (dq, dk, dv) as views of the one d(q|k|v) buffer, and the buffer the attention read (rotated in place by
    the rotary entry)."""
    from rankpo_amd import ops
    leaf = qkv.detach().clone().requires_grad_(True)
    x = leaf * 1.0
    scale = hd ** -0.5
    if rope is None:
        out = ops.flash_attn_varlen_qkv(x, nh, nkv, cu, tiles, k_tiles, scale, key_block=key_block, head_dim=hd, fwd_tiles=fwd_tiles)
    else:
        out = ops.rope_flash_attn_varlen_qkv(x, rope[0], rope[1], nh, nkv, cu, tiles, k_tiles, scale, key_block=key_block,
                                             head_dim=hd, fwd_tiles=fwd_tiles)
    out.backward(go)
    return out.detach(), views(leaf.grad, nh, nkv, hd), x.detach()


def _cu(lens):
    return torch.tensor([0] + list(np.cumsum(lens)), dtype=torch.int32, device=DEV)


class Verifier:
    """Checks the runs of one input set.  The forward output against `fwd_ref` (exact rotation of the un-rotated input) with
    PyTorch's forward as the control; the forward kernel's lse and every backward against `bwd_ref` on what the backward kernels
    read (the attention's own input buffer, that forward kernel's output and lse) with PyTorch's backward on the same as the
    control.  Backward references are shared by the variants that share a forward kernel."""

    def __init__(self, qkv, go, nh, nkv, hd, lens, rope=None):
        self.go, self.nh, self.nkv, self.hd, self.lens, self.rope = go, nh, nkv, hd, lens, rope
        self.cu, self.scale = _cu(lens), hd ** -0.5
        q, k, v = views(qkv, nh, nkv, hd)
        self.F = fwd_ref(q, k, v, lens, self.scale, rope)
        self.FC = fwd_control(q, k, v, lens, self.scale, rope)
        self.bwd = {}

    def __call__(self, tag, out, grads, x_act, tiles, q_block=128, fwd_name="fwd"):
        from rankpo_amd import ops
        q, k, v = views(x_act, self.nh, self.nkv, self.hd)
        out_k, lse_k = ops.flash_attn_varlen_fwd(q, k, v, self.cu, tiles, self.scale, q_block=q_block)
        assert torch.equal(out_k, out), tag                           # the split views of what the entry read: the same output
        if fwd_name not in self.bwd:
            _, lse_p = ops.flash_attn_varlen_fwd(q, k, v, self.cu, tiles, self.scale, padded_lse_len=max(self.lens),
                                                 num_seqs=len(self.lens), q_block=q_block)
            self.bwd[fwd_name] = (bwd_ref(q, k, v, self.go, out_k, lse_k, self.lens, self.scale, self.rope),
                                  bwd_control(q, k, v, self.go, out_k, lse_p, self.lens, self.scale, self.rope),
                                  fwd_ref(q, k, v, self.lens, self.scale)[0] if self.rope is not None else None)
        B, BC, F_act = self.bwd[fwd_name]
        worst = check_out(tag, out, self.F[0], self.FC, self.cu, F_act)
        check_lse(f"{tag} lse", lse_k, B[0])
        if grads is not None:
            worst = max(worst, check_grads(tag, grads, B, BC, self.cu))
        return worst


# ---------------------------------------------------------------------------------------------------------------- tests
REGIMES = ["flat", "spike", "sink", "growing", "negative"]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hd", [64, 128])
def test_every_variant_every_regime(hd, regime, monkeypatch):
    """Every shipped kernel instantiation of one head dim on one input set per regime (16 q / 2 kv heads: a group of 8, which every
    variant accepts): forward fa_fwd_kernel (hd 64) / fa_fwd128_kernel and fa_fwd128w_kernel (hd 128) on both query-list
    formats; backward fa_bwd_dq_kernel with fa_bwd_dkdv4_kernel<false>, <true> (key tables in group order False / True / 0.35)
    and fa_bwd_dkdv_kernel (hd 64), fa_bwd_dq128_kernel with fa_bwd_dkdv128_kernel<true> and <false> (hd 128); the rotary fold on
    every variant that takes it.  Cross-variant identities: dQ bit-identical across the dK/dV kernels, dK/dV of the different
    kernels bf16 round-off apart, the two list formats bit-identical."""
    from rankpo_amd import ops
    from rankpo_amd._lib import RankPOHipError
    nh, nkv, lens = 16, 2, LENS_REGIME
    qkv, go, spikes = make_inputs(hd, nh, nkv, lens, regime, seed=100 + hd + REGIMES.index(regime))
    cu, scale = _cu(lens), hd ** -0.5
    rope = rope_tables(lens, hd, DEV)
    qkv_r = unrotate(qkv, nh, nkv, hd, rope)                               # input of the rotary variants
    V = {False: Verifier(qkv, go, nh, nkv, hd, lens), True: Verifier(qkv_r, go, nh, nkv, hd, lens, rope)}
    assert_regime(regime, qkv, nh, nkv, hd, lens, spikes, V[False].F)
    assert_regime(regime, qkv_r, nh, nkv, hd, lens, spikes, V[True].F, rope)
    t3, t2 = ops.attn_tile_table(lens, DEV, nh, nkv), ops.attn_tile_table(lens, DEV)
    q, k, v = views(qkv, nh, nkv, hd)
    o3, l3 = ops.flash_attn_varlen_fwd(q, k, v, cu, t3, scale)
    o2, l2 = ops.flash_attn_varlen_fwd(q, k, v, cu, t2, scale)
    assert torch.equal(o2, o3) and torch.equal(l2, l3)                    # the list format is only a schedule
    ft = ops.attn_fwd_tile_table(lens, DEV, nh, nkv, hd)

    runs = {}
    for rope_on in (False, True):
        x = qkv_r if rope_on else qkv
        rp = rope if rope_on else None
        if hd == 64:
            kb = ops.ATTN_KEY_BLOCK
            with monkeypatch.context() as m:
                m.setattr(ops, "ATTN_SWEEP_DOWN", False)
                runs["up", rope_on] = grad_run(x, go, nh, nkv, hd, cu, t3, ops.attn_key_tile_table(lens, DEV, nkv), kb, rp)
            for name, tail in (("down", None), ("down_tail", 0.35), ("down_heaviest", False)):
                with monkeypatch.context() as m:
                    m.setattr(ops, "ATTN_SWEEP_DOWN", True)
                    if tail:
                        m.setattr(ops, "ATTN_GROUP_TAIL", tail)
                    kt = (ops.attn_key_tile_table(lens, DEV, nkv) if tail is not False
                          else ops.attn_key_tile_table(lens, DEV, nkv, group_order=False))
                    runs[name, rope_on] = grad_run(x, go, nh, nkv, hd, cu, t3, kt, kb, rp)
            if not rope_on:
                runs["kb64", rope_on] = grad_run(x, go, nh, nkv, hd, cu, t3, ops.attn_key_tile_table(lens, DEV, nkv, block_n=64), 64)
        else:
            kb = ops.ATTN_KEY_BLOCK_HD128
            assert ft is not None                                          # group 8: the one-wave forward takes it
            for name, down, fwd in (("down", True, None), ("up", False, None), ("up_w", False, ft)):
                with monkeypatch.context() as m:
                    m.setattr(ops, "ATTN_SWEEP_DOWN_HD128", down)
                    runs[name, rope_on] = grad_run(x, go, nh, nkv, hd, cu, t3, ops.attn_key_tile_table(lens, DEV, nkv, block_n=kb),
                                                   kb, rp, fwd_tiles=fwd)
        names = [key[0] for key in runs if key[1] == rope_on]
        for name in names:
            out, grads, x_act = runs[name, rope_on]
            w = name.endswith("_w")
            V[rope_on](f"hd{hd} {regime} {name} rope={rope_on}", out, grads, x_act, ft if w else t3, 64 if w else 128,
                       "fwd128w" if w else "fwd")
        ref = runs[names[0], rope_on][1]
        for name in names[1:]:
            g = runs[name, rope_on][1]
            if not name.endswith("_w"):                                  # (another forward: another output, another delta)
                assert torch.equal(g[0], ref[0]), ("dQ differs between dK/dV variants", name)
            for i in (1, 2):
                roundoff_apart(f"{name} d{'kv'[i - 1]}", g[i], ref[i], cu)
    assert ops.ATTN_SWEEP_DOWN is False and ops.ATTN_SWEEP_DOWN_HD128 is True and ops.ATTN_GROUP_TAIL == 0.0
    assert torch.equal(runs[("up" if hd == 64 else "down"), False][0], o3)
    if hd == 64:
        # the 64-key dK/dV kernel has no rotary epilogue: refused by the C call, and routed away by ops
        with pytest.raises(RankPOHipError, match="status -2"):
            ops.flash_attn_varlen_bwd(q, k, v, o3, go, l3, cu, t3, ops.attn_key_tile_table(lens, DEV, nkv, block_n=64), scale,
                                      key_block=64, rope=rope)
        with pytest.raises(ValueError):
            ops.rope_flash_attn_varlen_qkv(qkv.clone(), rope[0], rope[1], nh, nkv, cu, t3, None, scale, key_block=64)


@pytest.mark.parametrize("heads", GQA, ids=[f"{a}q{b}kv" for a, b in GQA])
@pytest.mark.parametrize("hd", [64, 128])
def test_every_group_every_length(hd, heads, monkeypatch):
    """Every GQA group (1, 3, 5, 6, 7, 8) at every edge length (1 .. 4097, one varlen batch) through the encoder's entry (rotary fold,
    XCD-dealt list) with both sweep settings (a non-power-of-two group falls to the ascending kernel when the descending one is
    asked for), the forward-only entry, the split-view forward on the [n, 2] list, and the one-wave forward where the group allows."""
    from rankpo_amd import ops
    nh, nkv = heads
    lens = LENS_ALL
    qkv, go, _ = make_inputs(hd, nh, nkv, lens, "flat", seed=7 * nh + nkv + hd)
    cu, scale = _cu(lens), hd ** -0.5
    rope = rope_tables(lens, hd, DEV)
    V = Verifier(qkv, go, nh, nkv, hd, lens, rope)
    t3, t2 = ops.attn_tile_table(lens, DEV, nh, nkv), ops.attn_tile_table(lens, DEV)
    kb = ops.ATTN_KEY_BLOCK if hd == 64 else ops.ATTN_KEY_BLOCK_HD128
    knob = "ATTN_SWEEP_DOWN" if hd == 64 else "ATTN_SWEEP_DOWN_HD128"
    res = {}
    for down in (False, True):
        with monkeypatch.context() as m:
            m.setattr(ops, knob, down)
            res[down] = grad_run(qkv, go, nh, nkv, hd, cu, t3, ops.attn_key_tile_table(lens, DEV, nkv, block_n=kb), kb, rope)
        V(f"hd{hd} {nh}/{nkv} sweep_down={down}", res[down][0], res[down][1], res[down][2], t3)
    assert torch.equal(res[False][0], res[True][0]) and torch.equal(res[False][1][0], res[True][1][0])
    for i in (1, 2):
        roundoff_apart(f"hd{hd} {nh}/{nkv} sweeps d{'kv'[i - 1]}", res[True][1][i], res[False][1][i], cu)
    x = qkv.clone()
    o_fold = ops.rope_flash_attn_varlen_qkv_fwd(x, rope[0], rope[1], nh, nkv, cu, t3, scale, head_dim=hd)
    assert torch.equal(o_fold, res[False][0]) and torch.equal(x, res[False][2])
    V(f"hd{hd} {nh}/{nkv} [n, 2] list", o_fold, None, x, t2)
    ft = ops.attn_fwd_tile_table(lens, DEV, nh, nkv, hd)
    if ft is not None:                                                     # fa_fwd128w_kernel where the group allows it
        q, k, v = views(x, nh, nkv, hd)
        o_w, _ = ops.flash_attn_varlen_fwd(q, k, v, cu, ft, scale, q_block=64)
        V(f"hd{hd} {nh}/{nkv} one-wave fwd", o_w, None, x, ft, 64, "fwd128w")


# ---------------------------------------------------------------------------------------------------------------- last query
LENS_LASTQ = [4097, 1, 2, 15, 16, 17, 33, 64, 65, 300, 1000]


def _lastq_inputs(hd, nh, nkv, lens, regime, seed):
    """q [N, nh, hd] (one query per sequence), kv [T, 2 nkv hd] fused k|v, dO [N, nh, hd]; spike: the row maximum sits in ONE lane
    group of the kernel (key j is read by group j % (number of groups))."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    T, N = sum(lens), len(lens)
    scale = hd ** -0.5
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    q, k, v = rn(N, nh, hd), rn(T, nkv, hd), rn(T, nkv, hd)
    pos = torch.cat([torch.arange(n, dtype=torch.float32) for n in lens]).to(DEV)
    first = [0] + list(np.cumsum(lens))[:-1]
    groups = (64 // (hd // 8)) * 4                     # lastq_attention.hip: G = (64 / (HD / 8)) x 4 waves
    marks = []
    if regime in ("spike", "sink"):
        k[..., 0] = 0.0
        a = float(torch.tensor(math.sqrt((GAP if regime == "spike" else SINK_GAP + 6.0) / scale)).bfloat16())
        q[..., 0] = a
        for si, n in enumerate(lens):
            j = 0 if regime == "sink" else (5 + 7 * si) % n
            k[first[si] + j, :, 0] = a
            marks.append((si, j, j % groups))
    elif regime == "growing":
        q = q * 2.0 + 1.5
        k = (k * 0.3 + 0.4) * (1.0 + pos / 60.0)[:, None, None]
    elif regime == "negative":
        q = q * 0.5 + 1.5
        k = k * 0.2 - 8.0
    kv = torch.cat([k.reshape(T, -1), v.reshape(T, -1)], 1).to(torch.bfloat16).contiguous()
    return q.to(torch.bfloat16), kv, rn(N, nh, hd).to(torch.bfloat16), marks


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("hd", [64, 128])
def test_last_query_every_group_every_regime(hd, regime):
    """lastq_fwd_kernel / lastq_bwd_kernel at groups 1, 2, 4 on every regime (spike: the row maximum in one lane group of the
    partial-(m, l, acc) merge), against float64 with PyTorch's flash op as the control; groups 3, 6, 8 refused."""
    from rankpo_amd import ops, _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    lens = LENS_LASTQ
    T, N = sum(lens), len(lens)
    cu, scale = _cu(lens), hd ** -0.5
    ones = torch.arange(N + 1, dtype=torch.int32, device=DEV)
    for G in (1, 2, 4):
        nkv = 2
        nh = G * nkv
        q, kv, go, marks = _lastq_inputs(hd, nh, nkv, lens, regime, seed=31 * G + hd + REGIMES.index(regime))
        k, v = kv[:, :nkv * hd].unflatten(1, (nkv, hd)), kv[:, nkv * hd:].unflatten(1, (nkv, hd))
        F = fwd_ref(q, k, v, lens, scale, last_query=True)
        if regime in ("spike", "sink"):
            o0 = 0
            for (si, j, grp), n in zip(marks, lens):
                if n > 1:
                    for h in (0, nh - 1):
                        s = _logits(q, k, None, scale, si, h, h // G, torch.arange(o0, o0 + n, device=DEV))
                        assert float(s[j] - torch.cat([s[:j], s[j + 1:]]).max()) > (20.0 if regime == "spike" else 10.0)
                o0 += n
            if regime == "spike":
                assert len({grp for _, _, grp in marks}) > 1         # different sequences put the maximum in different groups
        elif regime == "growing":
            assert float(F[1].max() - F[1].min()) > 50.0
        elif regime == "negative":
            assert float(F[1].max()) < -50.0
        assert ops.last_query_attn_ok(q, kv, nh, nkv, hd)
        qg, kvg = q.clone().requires_grad_(True), kv.clone().requires_grad_(True)
        out = ops.last_query_attn(qg, kvg, cu, nkv, hd, scale)
        out.backward(go)
        dk, dv = kvg.grad[:, :nkv * hd].unflatten(1, (nkv, hd)), kvg.grad[:, nkv * hd:].unflatten(1, (nkv, hd))
        lse = torch.empty(N, nh, device=DEV)                             # the lse the backward read (same kernel, same inputs)
        o_c = torch.empty_like(out)
        assert lib.rpo_lastq_attn_fwd(q.data_ptr(), nh * hd, kv.data_ptr(), kv.data_ptr() + nkv * hd * 2, 2 * nkv * hd, 2 * nkv * hd,
                                      cu.data_ptr(), N, nh, nkv, hd, scale, o_c.data_ptr(), nh * hd, lse.data_ptr(), st) == 0
        assert torch.equal(o_c, out.detach())
        tag = f"lastq hd{hd} G{G} {regime}"
        # out / dq: one row per (sequence, q head); dk / dv: blocks of (sequence, kv head)
        check(f"{tag} out", out.detach(), F[0], fwd_control(q, k, v, lens, scale, last_query=True), ones, CEIL_OUT_ROW, rows=True)
        check(f"{tag} out rows", out.detach(), F[0], None, ones, CEIL_OUT_ROW, rows=True)
        B = bwd_ref(q, k, v, go, out.detach(), lse.T, lens, scale, last_query=True)
        BC = bwd_control(q, k, v, go, out.detach(), lse[..., None].contiguous(), lens, scale, last_query=True)
        check_lse(f"{tag} lse", lse.T, B[0])
        cq, ck, cv = BC if BC is not None else (None,) * 3
        check(f"{tag} dq", qg.grad, B[1], cq, ones, CEIL_GRAD_BLOCK, rows=True, mag=B[4][0])
        check(f"{tag} dk", dk, B[2], ck, cu, CEIL_GRAD_BLOCK, mag=B[4][1])
        check(f"{tag} dv", dv, B[3], cv, cu, CEIL_GRAD_BLOCK, mag=B[4][2])
    # groups the kernel does not take: refused by ops' predicate and by the C calls (forward and backward)
    for nh, nkv in ((6, 2), (12, 2), (8, 1)):
        q = torch.randn(N, nh, hd, device=DEV).to(torch.bfloat16)
        kv = torch.randn(T, 2 * nkv * hd, device=DEV).to(torch.bfloat16)
        assert not ops.last_query_attn_ok(q, kv, nh, nkv, hd)
        o = torch.empty(N, nh, hd, device=DEV, dtype=torch.bfloat16)
        lse = torch.empty(N, nh, device=DEV)
        kp, vp, ks = kv.data_ptr(), kv.data_ptr() + nkv * hd * 2, 2 * nkv * hd
        assert lib.rpo_lastq_attn_fwd(q.data_ptr(), nh * hd, kp, vp, ks, ks, cu.data_ptr(), N, nh, nkv, hd, scale, o.data_ptr(),
                                      nh * hd, lse.data_ptr(), st) == -2
        dq, dkv = torch.empty_like(q), torch.empty_like(kv)
        assert lib.rpo_lastq_attn_bwd(q.data_ptr(), nh * hd, kp, vp, ks, ks, cu.data_ptr(), N, nh, nkv, hd, scale, o.data_ptr(),
                                      nh * hd, o.data_ptr(), nh * hd, lse.data_ptr(), dq.data_ptr(), nh * hd, dkv.data_ptr(),
                                      dkv.data_ptr() + nkv * hd * 2, ks, ks, st) == -2


# ---------------------------------------------------------------------------------------------------------------- end to end
class _Tok:
    pad_token = "<pad>"
    padding_side = "right"

    def __call__(self, texts, padding=True, truncation=True, max_length=512, return_tensors="pt"):
        ids = [[1 + (ord(c) * 7 + i) % 500 for i, c in enumerate(t)][:max_length] for t in texts]
        L = max(len(x) for x in ids)
        m = [[1] * len(x) + [0] * (L - len(x)) for x in ids]
        return {"input_ids": torch.tensor([x + [0] * (L - len(x)) for x in ids]), "attention_mask": torch.tensor(m)}


def _batch(rs, N, L, vocab):
    lens = rs.randint(1, L + 1, size=N)
    lens[0] = L
    m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
    return torch.tensor(rs.randint(1, vocab, size=(N, L)) * m), torch.tensor(m)


@pytest.mark.parametrize("hd", [64, 128])
def test_group_of_three_training_step_and_encode_vs_oracle(hd):
    """6 q / 2 kv heads (a group of 3, which the last-query kernel refuses: the last block falls back to PyTorch's op) through the
    packed encoder: a training step by bench.step_parity's control rule against the float32 oracle, with spies that the hand-written
    forward and backward ran (and with which key block), then ModelForInference.encode under no-grad against the oracle."""
    import importlib
    import rankpo_amd
    from oracle import encoder_ref as E
    from rankpo_amd import encoder as PE, ops
    bench = importlib.import_module("bench")
    torch.manual_seed(41 + hd)
    cfg = PE.llama_config(vocab_size=512, hidden_size=384, intermediate_size=768, num_hidden_layers=3,
                          num_attention_heads=6, num_key_value_heads=2, head_dim=hd, pad_token_id=0)
    enc = PE.LlamaEncoder(cfg)
    w32 = E.state_dict_to_f32(enc)
    w = {k: v.detach().clone().requires_grad_(True) for k, v in w32.items()}
    rs = np.random.RandomState(42 + hd)
    qi, qm = _batch(rs, 4, 70, 512)
    pi, pm = _batch(rs, 12, 150, 512)
    cb = {"query": {"input_ids": qi, "attention_mask": qm}, "passage": {"input_ids": pi, "attention_mask": pm}}
    ref = bench.oracle_step(w, cfg.to_dict(), cb, 0.02)
    calls, bcalls, lastq, fallback = [], [], [], []
    real = (ops.flash_attn_varlen_fwd, ops.flash_attn_varlen_bwd, ops.last_query_attn, PE._varlen_last_query_attention)
    ops.flash_attn_varlen_fwd = lambda q, *a, **kw: (calls.append((q.shape[-1], q.shape[1])), real[0](q, *a, **kw))[1]
    ops.flash_attn_varlen_bwd = lambda q, *a, **kw: (bcalls.append((q.shape[-1], kw.get("key_block"))), real[1](q, *a, **kw))[1]
    ops.last_query_attn = lambda *a, **kw: (lastq.append(1), real[2](*a, **kw))[1]
    PE._varlen_last_query_attention = lambda *a, **kw: (fallback.append(1), real[3](*a, **kw))[1]
    try:
        model = rankpo_amd.ModelForTraining(encoder=enc.to(DEV).to(torch.bfloat16), temperature=0.02).train()
        rep = bench.step_parity(model, cfg, 0.02, cb, ref, DEV, torch.bfloat16)
        n_train_fwd, n_train_bwd, n_fallback = len(calls), len(bcalls), len(fallback)
        assert all(c == (hd, 6) for c in calls), calls                 # every hand-written forward at this head layout
        calls.clear()
        inf = rankpo_amd.ModelForInference(encoder=model.model, tokenizer=_Tok(), use_bf16=True, device=0)
        texts = ["".join(chr(97 + int(c)) for c in rs.randint(0, 26, size=int(rs.randint(20, 300)))) for _ in range(10)]
        emb = inf.encode(texts, batch_size=10, max_length=320)
    finally:
        ops.flash_attn_varlen_fwd, ops.flash_attn_varlen_bwd, ops.last_query_attn, PE._varlen_last_query_attention = real
    print(f"\nhead_dim {hd}, 6 q / 2 kv heads, packed step:", rep)
    assert rep["pass"], rep
    assert n_train_fwd and n_train_bwd
    assert all(c == (hd, ops.ATTN_KEY_BLOCK if hd == 64 else ops.ATTN_KEY_BLOCK_HD128) for c in bcalls)
    assert not lastq and n_fallback                                      # group 3: the last block took PyTorch's op
    assert calls and all(c == (hd, 6) for c in calls) and len(fallback) > n_fallback
    # encode: the float32 oracle on the same (bf16-held) weights, and the oracle's eager arithmetic in bf16 as the control
    tok = _Tok()(texts, max_length=320)
    wd = {k: v.detach() for k, v in inf.model.state_dict().items()}
    with torch.no_grad():
        refe = E.embed({k: v.float().cpu() for k, v in wd.items()}, cfg.to_dict(), tok).detach().double()
        ctrl = E.embed(wd, cfg.to_dict(), {k: v.to(DEV) for k, v in tok.items()}, dtype=torch.bfloat16).double().cpu()
    got = torch.as_tensor(emb).double()
    cos = lambda a: float((1 - (a * refe).sum(-1) / (a.norm(dim=-1) * refe.norm(dim=-1))).abs().max())
    print(f"encode: cos err {cos(got):.2e}, eager-bf16 control {cos(ctrl):.2e}")
    assert cos(got) <= 1.5 * cos(ctrl) + 5e-6, (cos(got), cos(ctrl))


# ---------------------------------------------------------------------------------------------------------------- one-wave 64
def _need_onewave64():
    from rankpo_amd import _lib
    if not (_lib.load().rpo_build_flags() & _lib.RPO_BUILD_ONEWAVE64):
        pytest.skip("librankpo_hip.so was built without ONEWAVE64=1")


@pytest.mark.parametrize("regime", REGIMES)
def test_one_wave_64_every_regime(regime):
    """The optional head_dim-64 one-wave kernels (fa_fwd64w_kernel, fa_bwd_dq64w_kernel; `make ONEWAVE64=1`) on the same regimes."""
    _need_onewave64()
    from rankpo_amd import ops
    hd, nh, nkv, lens = 64, 16, 2, LENS_REGIME
    qkv, go, spikes = make_inputs(hd, nh, nkv, lens, regime, seed=300 + REGIMES.index(regime))
    cu, scale = _cu(lens), hd ** -0.5
    V = Verifier(qkv, go, nh, nkv, hd, lens)
    assert_regime(regime, qkv, nh, nkv, hd, lens, spikes, V.F)
    q, k, v = views(qkv, nh, nkv, hd)
    ft = ops.attn_fwd_tile_table(lens, DEV, nh, nkv, hd, force=True)
    out, _ = ops.flash_attn_varlen_fwd(q, k, v, cu, ft, scale, q_block=64)
    V(f"one-wave 64 {regime} fwd", out, None, qkv, ft, 64, "fwd64w")
    t128 = ops.attn_tile_table(lens, DEV, nh, nkv)
    o128, l128 = ops.flash_attn_varlen_fwd(q, k, v, cu, t128, scale)
    tl = ops.attn_tile_table(lens, DEV, nh, nkv, block_m=64, heads_per_block=4)
    grads = ops.flash_attn_varlen_bwd(q, k, v, o128, go, l128, cu, tl, ops.attn_key_tile_table(lens, DEV, nkv), scale, q_block=64)
    V(f"one-wave 64 {regime} bwd", o128, grads, qkv, t128)
