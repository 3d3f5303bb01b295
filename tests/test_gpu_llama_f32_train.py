"""The f32 attention of the packed Llama TRAINING pass (header section 9d: rpo_causal_attn_bwd_f32; `ops.causal_attn_f32_bwd`,
`ops.causal_attn_f32_train`, `encoder.LLAMA_F32_ATTENTION_TRAIN` / `LlamaEncoder.f32_attention_train` /
`ModelForTraining(f32_attention=True)`).

Error rule (tests/test_gpu_llama_f32.py): err <= 1.5 * control_err + floor per tensor (dq, dk, dv), both errors max-abs against a
float64 reference computed here, the control stock torch in f32 on the same inputs (SDPA with the explicit bottom-right boolean mask
per sequence, differentiated by autograd), floor = 2 ulp of f32 at max|ref| of the tensor compared."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_ref as E
from test_gpu_llama_f32 import DEV, F32, _cu, _floor, _fused, _rule, _seqs, _visible, ops

pytestmark = pytest.mark.gpu
LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 300]
SHAPES = [(64, 8, 2), (128, 4, 1), (64, 4, 4), (64, 4, 2), (128, 8, 1)]     # (head_dim, query heads, kv heads): groups 4, 4, 1, 2, 8
HARD_LENS = [1, 17, 200, 65]


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def _grads(q, k, v, dout, lens_q, lens_k, scale, dtype):
    """(dq, dk, dv) by autograd per sequence.  float64: the plain formula with the explicit mask; float32: stock SDPA with it."""
    G = q.shape[1] // k.shape[1]
    q, k, v = (t.detach().to(dtype).clone().requires_grad_() for t in (q, k, v))
    outs = []
    for qs, ks, vs in _seqs(q, k, v, lens_q, lens_k):
        if qs.shape[0] == 0:
            continue
        kr, vr = ks.repeat_interleave(G, 1), vs.repeat_interleave(G, 1)
        vis = _visible(qs.shape[0], ks.shape[0])
        if dtype == torch.float64:
            s = (torch.einsum("qhd,khd->hqk", qs, kr) * scale).masked_fill(~vis, -math.inf)
            outs.append(torch.einsum("hqk,khd->qhd", torch.softmax(s, -1), vr))
        else:
            qt, kt, vt = (t.transpose(0, 1)[None] for t in (qs, kr, vr))
            outs.append(F.scaled_dot_product_attention(qt, kt, vt, attn_mask=vis, scale=scale)[0].transpose(0, 1))
    return torch.autograd.grad(torch.cat(outs), (q, k, v), dout.to(dtype).view(q.shape))


def _bwd(q, k, v, dout, lens_q, lens_k, scale):
    """Forward, then the raw backward op: (dq, dk, dv)."""
    o = ops()
    cu_q, cu_k = _cu(lens_q), _cu(lens_k)
    tiles = o.causal_attn_f32_tile_table(lens_q, lens_k, DEV)
    k_tiles = o.causal_attn_f32_key_tile_table(lens_q, lens_k, DEV)
    out, lse = o.causal_attn_f32(q, k, v, cu_q, cu_k, tiles, scale, want_lse=True)
    dq, dk, dv = o.causal_attn_f32_bwd(q, k, v, out, lse, dout, cu_q, cu_k, tiles, k_tiles, scale)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape and dq.dtype == dk.dtype == dv.dtype == F32
    return dq, dk, dv


def _check_bwd(q, k, v, dout, lens_q, lens_k, scale, label):
    got = _bwd(q, k, v, dout, lens_q, lens_k, scale)
    ref = _grads(q, k, v, dout, lens_q, lens_k, scale, torch.float64)
    ctrl = _grads(q, k, v, dout, lens_q, lens_k, scale, F32)
    for name, g, c, r in zip(("dq", "dk", "dv"), got, ctrl, ref):
        _rule(g, c, r, f"{label} {name}")
    return got


@functools.lru_cache(maxsize=None)
def _inputs(hd, nh, nkv):
    """One packed batch per shape, q / k / v column blocks of ONE buffer, and a random dout: made once, never modified."""
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh * 10 + nkv + 1)
    qkv, (q, k, v) = _fused(sum(LENS), nh, nkv, hd, gen)
    assert q.stride(0) == (nh + 2 * nkv) * hd and k.data_ptr() == qkv.data_ptr() + 4 * nh * hd
    dout = torch.randn(sum(LENS), nh * hd, generator=gen, device=DEV)
    return q, k, v, dout, 1.0 / math.sqrt(hd)


# ------------------------------------------------------------------------------------------------
# the kernels against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_self_attention(hd, nh, nkv):
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    _check_bwd(q, k, v, dout, LENS, LENS, scale, f"self hd{hd} nh{nh} nkv{nkv}")


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_last_query_form(hd, nh, nkv):
    """One query per sequence (its last token) over the same K / V: it sees every key."""
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    last = torch.tensor(np.cumsum(LENS) - 1, device=DEV)
    ql = q.reshape(q.shape[0], -1).index_select(0, last).view(-1, nh, hd)
    _check_bwd(ql, k, v, dout.index_select(0, last), [1] * len(LENS), LENS, scale, f"last query hd{hd} nh{nh} nkv{nkv}")


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_backward_bottom_right_alignment(hd, nh, nkv):
    """lens_q[n] = ceil(lens_k[n] / 3): query i sees keys j <= i + (lk - lq)."""
    q, k, v, dout, scale = _inputs(hd, nh, nkv)
    lens_q = [-(-n // 3) for n in LENS]
    T = sum(lens_q)
    _check_bwd(q[:T], k, v, dout[:T], lens_q, LENS, scale, f"bottom-right hd{hd} nh{nh} nkv{nkv}")


def test_backward_long_sequence():
    """More than 32 key blocks and more than 32 query steps."""
    gen = torch.Generator(device=DEV).manual_seed(1100)
    lens = [1100, 3]
    _, (q, k, v) = _fused(sum(lens), 4, 1, 64, gen)
    dout = torch.randn(sum(lens), 4 * 64, generator=gen, device=DEV)
    _check_bwd(q, k, v, dout, lens, lens, 0.125, "1100 keys")


@pytest.mark.parametrize("hd", [64, 128])
def test_backward_hard_inputs(hd):
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    dout = torch.randn(T, nh * hd, generator=gen, device=DEV)
    # saturated softmax: scores ~ +-60 after scaling (one key per query dominates), as the forward's test builds them
    mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen, mult)
    _check_bwd(q, k, v / mult, dout, lens, lens, scale, f"saturated hd{hd}")
    # identical keys: uniform weights over the visible keys
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen)
    _check_bwd(q, k[:1].expand(T, nkv, hd).contiguous(), v, dout, lens, lens, scale, f"identical keys hd{hd}")
    # a large upstream gradient
    _check_bwd(q, k, v, dout * 1e4, lens, lens, scale, f"dout x 1e4 hd{hd}")
    # a negative scale is |scale| and a sign on q, as in the forward: the bits of the call on -q with |scale| (stock SDPA gives
    # NaN at a negative scale, so there is no control to hold it against)
    neg, pos = _bwd(q, k, v, dout, lens, lens, -scale), _bwd(-q, k, v, dout, lens, lens, scale)
    assert torch.equal(neg[0], -pos[0]) and torch.equal(neg[1], pos[1]) and torch.equal(neg[2], pos[2])


@pytest.mark.parametrize("hd", [64, 128])
def test_no_gradient_leaks_across_the_mask(hd):
    """dout = 0 for every query behind the middle position P of its sequence.  The keys behind P are seen by those queries only:
    their dk / dv rows are exact zeros, and so is dq of the queries behind P.  The rows up to P are BIT-equal to a call on the
    sequences truncated at P: what lies behind P enters every sum as an exact zero."""
    gen = torch.Generator(device=DEV).manual_seed(70 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = 1.0 / math.sqrt(hd)
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    pos = torch.cat([torch.arange(n, device=DEV) for n in lens])
    P = torch.cat([torch.full((n,), n // 2, device=DEV) for n in lens])           # 0, 8, 100, 32
    behind = pos > P
    dout = torch.randn(sum(lens), nh * hd, generator=gen, device=DEV) * (~behind)[:, None]
    dq, dk, dv = _bwd(q, k, v, dout, lens, lens, scale)
    for t in (dq, dk, dv):
        assert torch.isfinite(t).all() and (t[behind] == 0).all()
        assert (t[~behind] != 0).any()
    cut = [n // 2 + 1 for n in lens]
    tq, tk, tv = _bwd(q[~behind].contiguous(), k[~behind].contiguous(), v[~behind].contiguous(), dout[~behind].contiguous(),
                      cut, cut, scale)
    assert torch.equal(dq[~behind], tq) and torch.equal(dk[~behind], tk) and torch.equal(dv[~behind], tv)


def test_deterministic_and_independent_of_packing():
    gen = torch.Generator(device=DEV).manual_seed(5)
    hd, nh, nkv = 64, 8, 2
    la, lx, lb = 33, 70, 17
    _, (q, k, v) = _fused(la + lx + lb, nh, nkv, hd, gen)
    dout = torch.randn(la + lx + lb, nh * hd, generator=gen, device=DEV)
    scale = 0.125
    one = _bwd(q, k, v, dout, [la, lx, lb], [la, lx, lb], scale)
    two = _bwd(q, k, v, dout, [la, lx, lb], [la, lx, lb], scale)
    assert all(torch.equal(a, b) for a, b in zip(one, two))
    mid = slice(la, la + lx)
    alone = _bwd(q[mid], k[mid], v[mid], dout[mid], [lx], [lx], scale)
    assert all(torch.equal(a[mid], b) for a, b in zip(one, alone))
    # the other order: b | x | a
    perm = torch.cat([torch.arange(la + lx, la + lx + lb), torch.arange(la, la + lx), torch.arange(la)]).to(DEV)
    swapped = _bwd(q[perm].contiguous(), k[perm].contiguous(), v[perm].contiguous(), dout[perm].contiguous(), [lb, lx, la],
                   [lb, lx, la], scale)
    assert all(torch.equal(a[lb:lb + lx], b) for a, b in zip(swapped, alone))


def test_keys_without_queries_get_zeros():
    gen = torch.Generator(device=DEV).manual_seed(6)
    lens_q, lens_k = [0, 3], [4, 3]
    _, (_, k, v) = _fused(7, 4, 2, 64, gen)
    q = torch.randn(3, 4, 64, generator=gen, device=DEV)
    dout = torch.randn(3, 4 * 64, generator=gen, device=DEV)
    dq, dk, dv = _check_bwd(q, k, v, dout, lens_q, lens_k, 0.125, "lq == 0")
    assert (dk[:4] == 0).all() and (dv[:4] == 0).all() and (dk[4:] != 0).any()


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refuses_what_it_cannot_run():
    """RPO_ERR_UNSUPPORTED before any launch: the buffers here are far smaller than what the refused shapes would touch."""
    from rankpo_amd import _lib
    lib = _lib.load()
    OK, UNS = 0, -2
    st = torch.cuda.current_stream().cuda_stream
    xf = torch.zeros(4096 * 16, dtype=F32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    p = xf.data_ptr()
    o1, o2, o3, o4 = (p + 4096 * 4 * i for i in (4, 6, 8, 10))

    def bwd(ptr=p, stride=256, tl=tiles, cols=2, qb=32, nh=2, nkv=1, hd=64, dq=o1, dkv=o2, ws=o3, dstride=128, n=1, nk=1):
        return lib.rpo_causal_attn_bwd_f32(ptr, ptr, ptr, ptr, ptr, stride, stride, stride, stride, stride, o4, cu.data_ptr(),
                                           cu.data_ptr(), tl.data_ptr(), n, tl.data_ptr(), nk, cols, qb, 1, nh, nkv, hd, 0.1, dq,
                                           dstride, dkv, dstride, dkv, dstride, ws, st)
    assert bwd() == OK                                         # the checks below do not refuse everything
    assert bwd(n=0, nk=0) == OK                                # empty work lists: nothing to launch
    assert bwd(hd=32) == UNS
    assert bwd(hd=96, stride=768) == UNS
    assert bwd(nh=3, nkv=2) == UNS                             # nh % nkv
    assert bwd(nh=3, nkv=1) == UNS                             # 3 query heads per kv head
    assert bwd(nh=16, nkv=1, stride=4096) == UNS               # 16
    assert bwd(tl=tiles3, cols=3) == UNS                       # another table format
    assert bwd(qb=64) == UNS
    assert bwd(ptr=p + 4) == UNS                               # misaligned q / k / v / out / dout
    assert bwd(dq=o1 + 8) == UNS and bwd(dkv=o2 + 4) == UNS and bwd(ws=o3 + 8) == UNS
    assert bwd(stride=194) == UNS and bwd(dstride=130) == UNS  # rows not 16-byte aligned
    torch.cuda.synchronize()
    o = ops()
    q32 = torch.zeros(4, 3, 32, device=DEV)
    with pytest.raises(ValueError):
        o.causal_attn_f32_bwd(q32, q32, q32, q32.view(4, -1), torch.zeros(3, 4, device=DEV), q32.view(4, -1), cu, cu, tiles, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f32_key_tile_table([5], [4], DEV)


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
    tiles, k_tiles = o.causal_attn_f32_tile_table(LENS, LENS, DEV), o.causal_attn_f32_key_tile_table(LENS, LENS, DEV)
    out = o.causal_attn_f32_train(qg, kg, vg, cu, cu, tiles, k_tiles, scale)
    assert out.requires_grad and torch.equal(out, o.causal_attn_f32(q, k, v, cu, cu, tiles, scale)[0])
    got = torch.autograd.grad(out, (qg, kg, vg), dout)
    assert all(torch.equal(a, b) for a, b in zip(got, raw))
    # dout of another stride: made contiguous, the same bits
    wide = torch.zeros(dout.shape[0], dout.shape[1] + 2, device=DEV)
    wide[:, 1:-1] = dout
    out = o.causal_attn_f32_train(qg, kg, vg, cu, cu, tiles, k_tiles, scale)
    got = torch.autograd.grad(out, (qg, kg, vg), wide[:, 1:-1])
    assert all(torch.equal(a, b) for a, b in zip(got, raw))
    # the forward-only op keeps its contract: no autograd node
    assert o.causal_attn_f32(qg, kg, vg, cu, cu, tiles, scale)[0].grad_fn is None


# ------------------------------------------------------------------------------------------------
# end to end: ModelForTraining on an f32 Llama encoder
# ------------------------------------------------------------------------------------------------
TEMP = 0.02


class Spy:
    """Counts the new ops, stock SDPA, and host reads of device tensors."""

    def __init__(self):
        self.n = {"train": 0, "full": 0, "last": 0, "bwd": 0, "sdpa": 0, "syncs": 0}

    def __enter__(self):
        o = ops()
        self._train, self._bwd, self._sdpa = o.causal_attn_f32_train, o.causal_attn_f32_bwd, F.scaled_dot_product_attention
        self._tolist, self._item = torch.Tensor.tolist, torch.Tensor.item

        def train(q, k, *a, **kw):
            self.n["train"] += 1
            self.n["full" if q.shape[0] == k.shape[0] else "last"] += 1
            return self._train(q, k, *a, **kw)

        def bwd(*a, **kw):
            self.n["bwd"] += 1
            return self._bwd(*a, **kw)

        def sdpa(*a, **kw):
            self.n["sdpa"] += 1
            return self._sdpa(*a, **kw)

        def tolist(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._tolist(t)

        def item(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._item(t)
        o.causal_attn_f32_train, o.causal_attn_f32_bwd, F.scaled_dot_product_attention = train, bwd, sdpa
        torch.Tensor.tolist, torch.Tensor.item = tolist, item
        return self

    def __exit__(self, *exc):
        o = ops()
        o.causal_attn_f32_train, o.causal_attn_f32_bwd, F.scaled_dot_product_attention = self._train, self._bwd, self._sdpa
        torch.Tensor.tolist, torch.Tensor.item = self._tolist, self._item
        return False


def _build(hd, seed, dtype=F32, **kw):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import _cfg
    torch.manual_seed(seed)
    cfg = _cfg(PE, hd)
    enc = PE.LlamaEncoder(cfg)
    w32 = E.state_dict_to_f32(enc)
    model = rankpo_amd.ModelForTraining(encoder=enc.to(DEV, dtype), temperature=TEMP, **kw).train()
    return PE, cfg, w32, model


def _batch(tok, rs, dev):
    from test_gpu_inference import _texts
    qt = _texts(rs, 1, 1, 60) + ["q"]                           # one 1-token row
    pt = _texts(rs, 3, 40, 400) + _texts(rs, 1, 380, 400)
    b = {"query": tok(qt, max_length=400), "passage": tok(pt, max_length=400)}
    return {s: {k: v.to(dev) for k, v in d.items()} for s, d in b.items()}


def _step(model, batch):
    """(loss, scores, {name: grad}, spy counts) of one forward + backward."""
    model.zero_grad(set_to_none=True)
    with Spy() as spy:
        out = model(**batch)
        out.loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.model.named_parameters()}
    model.zero_grad(set_to_none=True)
    return out.loss.detach().clone(), out.scores.detach().clone(), grads, spy.n


def _same_bits(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.fixture(scope="module", params=[64, 128])
def train_case(request):
    """One f32 model per config with every switch off and its step BEFORE any switch is touched (the control), the same weights
    with f32_attention=True, the batch, and the float64 oracle step on the CPU: computed once, shared, never modified."""
    from test_gpu_inference import CharTok
    hd = request.param
    PE, cfg, w32, off = _build(hd, 30 + hd)
    _, _, w32_on, on = _build(hd, 30 + hd, f32_attention=True)
    assert all(torch.equal(w32[k], w32_on[k]) for k in w32)
    assert not PE.LLAMA_F32_ATTENTION_TRAIN and not PE.LLAMA_F32_ATTENTION
    assert not off.model.f32_attention_train and not off.model.f32_attention
    assert on.model.f32_attention_train and on.model.f32_attention and on.model.embed_tokens.weight.dtype == F32
    rs = np.random.RandomState(hd)
    batch = _batch(CharTok(), rs, DEV)
    base = _step(off, batch)
    w64 = {k: v.double().requires_grad_(v.is_floating_point()) for k, v in w32.items()}
    cpu = {s: {k: v.cpu() for k, v in d.items()} for s, d in batch.items()}
    loss, scores, _, _ = E.contrastive_step(w64, cfg.to_dict(), cpu, TEMP, dtype=torch.float64)
    loss.backward()
    ref = (loss.detach(), scores.detach(), {k: w64[k].grad for k in base[2]})
    assert all(g is not None for g in ref[2].values())
    return dict(hd=hd, PE=PE, cfg=cfg, off=off, on=on, batch=batch, base=base, ref=ref)


def test_switch_off_runs_what_it_ran(train_case, monkeypatch):
    c = train_case
    assert c["base"][3]["train"] == 0 and c["base"][3]["bwd"] == 0 and c["base"][3]["sdpa"] > 0
    again = _step(c["off"], c["batch"])
    _same_bits(again, c["base"])
    # the two no-grad switches on: grad mode is not theirs
    monkeypatch.setattr(c["PE"], "LLAMA_F32_ATTENTION", True)
    monkeypatch.setattr(c["off"].model, "f32_attention", True)
    res = _step(c["off"], c["batch"])
    assert res[3]["train"] == 0 and res[3]["bwd"] == 0 and res[3]["sdpa"] > 0, res[3]
    _same_bits(res, c["base"])


def test_training_step_vs_oracle(train_case, monkeypatch):
    c = train_case
    nl = c["cfg"].num_hidden_layers
    res = _step(c["on"], c["batch"])
    n = res[3]
    assert n["sdpa"] == 0, n
    assert n["train"] == nl and n["full"] == nl - 1 and n["last"] == 1 and n["bwd"] == nl, n
    assert n["syncs"] == c["base"][3]["syncs"], "the switch added a host read of a device tensor"
    ref_loss, ref_scores, ref_g = c["ref"]
    _rule(res[0].cpu().view(1), c["base"][0].cpu().view(1), ref_loss.view(1), f"loss hd{c['hd']}")
    _rule(res[1].cpu(), c["base"][1].cpu(), ref_scores, f"scores hd{c['hd']}")
    worst = (0.0, None)
    for k, r in ref_g.items():
        rn = r.norm().item()
        assert rn > 0, k
        e = (res[2][k].cpu().double() - r).norm().item() / rn
        ce = (c["base"][2][k].cpu().double() - r).norm().item() / rn
        worst = max(worst, (e / (1.5 * ce + 2.0 ** -22), k, e, ce))
        assert torch.isfinite(res[2][k]).all() and e <= 1.5 * ce + 2.0 ** -22, (k, e, ce)
    print(f"\ngradients hd{c['hd']}: worst err / bound {worst[0]:.3f} at {worst[1]} (rel. Frobenius {worst[2]:.3e}, control {worst[3]:.3e})")
    # the module switch on the switch-off model: the same path, the same bits
    monkeypatch.setattr(c["PE"], "LLAMA_F32_ATTENTION_TRAIN", True)
    mod = _step(c["off"], c["batch"])
    assert mod[3]["train"] == nl and mod[3]["sdpa"] == 0, mod[3]
    _same_bits(mod, res)


def _plain_and_checkpointed(c):
    nl = c["cfg"].num_hidden_layers
    plain = _step(c["on"], c["batch"])
    c["on"].gradient_checkpointing_enable(layers="all")
    try:
        ck = _step(c["on"], c["batch"])
    finally:
        c["on"].model.gradient_checkpointing_disable()
    assert ck[3]["sdpa"] == 0 and ck[3]["train"] == 2 * nl and ck[3]["bwd"] == nl, ck[3]      # every block's forward runs twice
    return plain, ck


def test_checkpointing_gives_the_same_bits(train_case):
    """gradient_checkpointing_enable(layers="all"), switch on, default configuration: loss and EVERY gradient are bit-equal to the
    plain switch-on step.  The recomputation runs the same deterministic forward kernel, the backward sees the same q, k, v, out
    and lse, and on this path a checkpointed block receives the (x, delta) pair an un-checkpointed one receives
    (`encoder._ckpt_single_input`): with x + delta formed by a torch add in front of the boundary (encoder.CKPT_SINGLE_INPUT, what
    the switch-off step keeps doing) 19 of the 29 gradients differed by a few ulp, worst 1.0e-5 at max|g| 24.5, because the sum
    of the residual and the norm gradient is then rounded outside the fused add + RMSNorm backward."""
    c = train_case
    assert c["PE"].CKPT_SINGLE_INPUT is True
    plain, ck = _plain_and_checkpointed(c)
    _same_bits(ck, plain)


def test_checkpointed_switch_off_step_keeps_its_single_input(train_case, monkeypatch):
    """With the switch off a checkpointed block still receives x + delta as one tensor: `checkpoint` is handed delta = None for
    every block; with the switch on, the pair (delta is a tensor for every block but the first)."""
    import rankpo_amd.encoder as PE
    c = train_case
    seen = []
    real = PE.checkpoint

    def spy(fn, x, delta, *a, **kw):
        seen.append(delta is None)
        return real(fn, x, delta, *a, **kw)
    monkeypatch.setattr(PE, "checkpoint", spy)
    nl = c["cfg"].num_hidden_layers
    for model, want in ((c["off"], [True] * nl), (c["on"], [True] + [False] * (nl - 1))):
        seen.clear()
        model.gradient_checkpointing_enable(layers="all")
        try:
            _step(model, c["batch"])
        finally:
            model.model.gradient_checkpointing_disable()
        assert seen == want, seen


@pytest.mark.parametrize("hd", [64, 128])
def test_bf16_model_ignores_every_switch(hd, monkeypatch):
    from test_gpu_inference import CharTok
    PE, cfg, _, off = _build(hd, 9, dtype=torch.bfloat16)
    batch = _batch(CharTok(), np.random.RandomState(3), DEV)
    a = _step(off, batch)
    _, _, _, on = _build(hd, 9, dtype=torch.bfloat16, f32_attention=True)
    monkeypatch.setattr(PE, "LLAMA_F32_ATTENTION_TRAIN", True)
    monkeypatch.setattr(PE, "LLAMA_F32_ATTENTION", True)
    assert on.model.f32_attention_train and on.model.embed_tokens.weight.dtype == torch.bfloat16
    b = _step(on, batch)
    assert b[3]["train"] == 0 and b[3]["bwd"] == 0, b[3]
    _same_bits(a, b)


def test_left_padded_batches_give_the_switch_off_bits(train_case):
    from test_gpu_bert_native import LeftTok
    c = train_case
    batch = _batch(LeftTok(), np.random.RandomState(8), DEV)
    a, b = _step(c["on"], batch), _step(c["off"], batch)
    assert a[3]["train"] == 0 and a[3]["bwd"] == 0 and a[3]["sdpa"] > 0, a[3]
    _same_bits(a, b)
