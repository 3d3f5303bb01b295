"""The f32 attention of the packed Llama pass (header section 9c: rpo_causal_attn_fwd_f32; `ops.causal_attn_f32`,
`encoder.LLAMA_F32_ATTENTION` / `LlamaEncoder.f32_attention` / `ModelForInference(f32_attention=True)`).

Error rule (the project's own, tests/test_gpu_bert_f32.py): err <= 1.5 * control_err + floor, both errors max-abs against a float64
reference computed here, the control stock torch in f32 on the same inputs (SDPA with an EXPLICIT boolean mask: its `is_causal` is
top-left aligned, the kernel's rule is bottom-right aligned), floor = 2 ulp of f32 (23 explicit mantissa bits) at max|ref|.  With
an f32 control (about 1e-7) the rule fails any kernel that rounds P or an intermediate to 16 bits."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
ULP2 = 2 * 2.0 ** -23
LENS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 512, 1000]
SHAPES = [(64, 8, 2), (128, 4, 1), (64, 4, 4), (64, 4, 2), (128, 8, 1)]     # (head_dim, query heads, kv heads): groups 4, 4, 1, 2, 8


def ops():
    from rankpo_amd import ops as o
    return o


def _floor(ref):
    """2 ulp of f32 at max|ref|."""
    a = max(float(ref.abs().max()), 2.0 ** -126)
    return 2 * 2.0 ** (math.floor(math.log2(a)) - 23)


def _rule(got, ctrl, ref, label):
    assert torch.isfinite(got).all(), label
    err = (got.double() - ref).abs().max().item()
    c_err = (ctrl.double() - ref).abs().max().item()
    floor = _floor(ref)
    print(f"\n{label}: kernel {err:.3e}, f32 torch control {c_err:.3e}, floor {floor:.3e}")
    assert err <= 1.5 * c_err + floor, (label, err, c_err, floor)


# ------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------
def _visible(lq, lk):
    """bool [lq, lk]: query i sees key j iff j <= i + (lk - lq)."""
    i = torch.arange(lq, device=DEV)[:, None]
    j = torch.arange(lk, device=DEV)[None, :]
    return j <= i + (lk - lq)


def _seqs(q, k, v, lens_q, lens_k):
    oq = ok = 0
    for lq, lk in zip(lens_q, lens_k):
        yield q[oq:oq + lq], k[ok:ok + lk], v[ok:ok + lk]
        oq, ok = oq + lq, ok + lk


def _ref_attn(q, k, v, lens_q, lens_k, scale):
    """float64 per sequence on the device: (out [Tq, nh, hd], lse [nh, Tq])."""
    G = q.shape[1] // k.shape[1]
    outs, lses = [], []
    for qs, ks, vs in _seqs(q, k, v, lens_q, lens_k):
        kd, vd = ks.double().repeat_interleave(G, 1), vs.double().repeat_interleave(G, 1)
        s = torch.einsum("qhd,khd->hqk", qs.double(), kd) * scale
        s = s.masked_fill(~_visible(qs.shape[0], ks.shape[0]), -math.inf)
        lse = torch.logsumexp(s, -1)
        outs.append(torch.einsum("hqk,khd->qhd", torch.exp(s - lse[..., None]), vd))
        lses.append(lse)
    return torch.cat(outs), torch.cat(lses, 1)


def _ctrl_attn(q, k, v, lens_q, lens_k, scale):
    """Stock torch in f32 per sequence: SDPA with the explicit mask for the output, logsumexp of the masked f32 scores for lse."""
    G = q.shape[1] // k.shape[1]
    outs, lses = [], []
    for qs, ks, vs in _seqs(q, k, v, lens_q, lens_k):
        ks, vs = ks.repeat_interleave(G, 1), vs.repeat_interleave(G, 1)
        vis = _visible(qs.shape[0], ks.shape[0])
        qt, kt, vt = (t.transpose(0, 1)[None] for t in (qs, ks, vs))
        outs.append(F.scaled_dot_product_attention(qt, kt, vt, attn_mask=vis, scale=scale)[0].transpose(0, 1))
        s = (torch.einsum("qhd,khd->hqk", qs, ks) * scale).masked_fill(~vis, -math.inf)
        lses.append(torch.logsumexp(s, -1))
    return torch.cat(outs), torch.cat(lses, 1)


def _cu(lens):
    return torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32, device=DEV)


def _run(q, k, v, lens_q, lens_k, scale, want_lse=True):
    o = ops()
    tiles = o.causal_attn_f32_tile_table(lens_q, lens_k, DEV)
    out, lse = o.causal_attn_f32(q, k, v, _cu(lens_q), _cu(lens_k), tiles, scale, want_lse=want_lse)
    assert out.dtype == F32 and out.shape == (q.shape[0], q.shape[1] * q.shape[2])
    return out.view(q.shape), lse


def _check_attn(q, k, v, lens_q, lens_k, scale, label):
    out, lse = _run(q, k, v, lens_q, lens_k, scale)
    assert lse.dtype == F32 and lse.shape == (q.shape[1], q.shape[0])
    out2, none = _run(q, k, v, lens_q, lens_k, scale, want_lse=False)          # lse NULL: the same rows
    assert none is None and torch.equal(out, out2), label
    ref, ref_lse = _ref_attn(q, k, v, lens_q, lens_k, scale)
    ctrl, ctrl_lse = _ctrl_attn(q, k, v, lens_q, lens_k, scale)
    _rule(out, ctrl, ref, label)
    _rule(lse, ctrl_lse, ref_lse, label + " lse")
    return out, lse, ref


def _fused(T, nh, nkv, hd, gen, mult=1.0):
    """q / k / v as column blocks of ONE [T, (nh + 2 nkv) hd] f32 buffer (the fused projection output)."""
    qkv = torch.randn(T, (nh + 2 * nkv) * hd, generator=gen, device=DEV) * mult
    nq, nk = nh * hd, nkv * hd
    return qkv, (qkv[:, :nq].view(T, nh, hd), qkv[:, nq:nq + nk].view(T, nkv, hd), qkv[:, nq + nk:].view(T, nkv, hd))


@functools.lru_cache(maxsize=None)
def _self_case(hd, nh, nkv):
    """One packed batch per shape and its self-attention result: computed once, shared by the tests below, never modified."""
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh * 10 + nkv)
    qkv, (q, k, v) = _fused(sum(LENS), nh, nkv, hd, gen)
    stride = (nh + 2 * nkv) * hd
    assert q.stride(0) == k.stride(0) == v.stride(0) == stride and q.dtype == F32
    assert k.data_ptr() == qkv.data_ptr() + 4 * nh * hd and v.data_ptr() == k.data_ptr() + 4 * nkv * hd
    assert not torch.equal(q, q.bfloat16().float())            # randn: not exact in bf16
    scale = 1.0 / math.sqrt(hd)
    out, lse, ref = _check_attn(q, k, v, LENS, LENS, scale, f"self hd{hd} nh{nh} nkv{nkv}")
    return q, k, v, scale, out, lse, ref


# ------------------------------------------------------------------------------------------------
# the kernel against float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_causal_attention_f32_matches_f64(hd, nh, nkv):
    _self_case(hd, nh, nkv)


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_last_query_form(hd, nh, nkv):
    """One query per sequence (its last token) over the same K / V: bottom-right aligned, so it sees every key."""
    q, k, v, scale, out, lse, ref = _self_case(hd, nh, nkv)
    last = torch.tensor(np.cumsum(LENS) - 1, device=DEV)
    ql = q.reshape(q.shape[0], -1).index_select(0, last).view(-1, nh, hd)
    ones = [1] * len(LENS)
    o1, l1, r1 = _check_attn(ql, k, v, ones, LENS, scale, f"last query hd{hd} nh{nh} nkv{nkv}")
    # the last row of each sequence from the self-attention call: the same keys in the same steps, the masked tail of the step aside
    want = out.index_select(0, last)
    assert (o1.double() - want.double()).abs().max().item() <= _floor(r1)
    assert (l1.double() - lse.index_select(1, last).double()).abs().max().item() <= _floor(lse.index_select(1, last).double())


@pytest.mark.parametrize("hd,nh,nkv", SHAPES)
def test_bottom_right_alignment(hd, nh, nkv):
    """lens_q[n] = ceil(lens_k[n] / 3): query i sees keys j <= i + (lk - lq), against float64 with the explicit mask."""
    q, k, v, scale, *_ = _self_case(hd, nh, nkv)
    lens_q = [-(-n // 3) for n in LENS]
    assert max(lens_q) > 256 and any(n % 32 for n in lens_q)
    qs = q[:sum(lens_q)]                                        # any rows of the buffer serve as queries: same stride
    assert qs.stride(0) == q.stride(0)
    _check_attn(qs, k, v, lens_q, LENS, scale, f"bottom-right hd{hd} nh{nh} nkv{nkv}")


def test_long_sequence():
    """More than 128 key steps, across the workload's 4 096 tokens."""
    gen = torch.Generator(device=DEV).manual_seed(4100)
    lens = [4100, 3]
    _, (q, k, v) = _fused(sum(lens), 4, 1, 64, gen)
    _check_attn(q, k, v, lens, lens, 0.125, "4100 keys")


# ------------------------------------------------------------------------------------------------
# hard inputs
# ------------------------------------------------------------------------------------------------
HARD_LENS = [1, 17, 200, 65]


@pytest.mark.parametrize("hd", [64, 128])
def test_hard_inputs(hd):
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    # saturated softmax: scores ~ +-60 after scaling (one key per query dominates)
    mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen, mult)
    v = v / mult
    _check_attn(q, k, v, lens, lens, scale, f"saturated hd{hd}")
    # identical keys: uniform weights over the visible keys, the output is the running mean of V
    _, (q, k, v) = _fused(T, nh, nkv, hd, gen)
    k = k[:1].expand(T, nkv, hd).contiguous()
    out, _, ref = _check_attn(q, k, v, lens, lens, scale, f"identical keys hd{hd}")
    mean = torch.cat([vs.double().cumsum(0) / torch.arange(1, n + 1, device=DEV)[:, None, None]
                      for n, (_, _, vs) in zip(lens, _seqs(q, k, v, lens, lens))]).repeat_interleave(nh // nkv, 1)
    assert (ref - mean).abs().max().item() < 1e-12              # what the rule above compared the kernel with


@pytest.mark.parametrize("hd", [64, 128])
def test_future_keys_do_not_leak(hd):
    """Every key behind position P of its sequence is multiplied by 1001.  A query at a position <= P sees none of them: its row
    depends on its visible keys only (the masked scores of its step are computed, then neither enter its running maximum nor its
    sum, and enter PV as exact zeros), so it is BIT-equal to the row of the unmodified call.  A leaked key would move the
    running maximum by three orders of magnitude and the row with it."""
    gen = torch.Generator(device=DEV).manual_seed(70 + hd)
    nh, nkv, lens = 4, 2, HARD_LENS
    scale = 1.0 / math.sqrt(hd)
    _, (q, k, v) = _fused(sum(lens), nh, nkv, hd, gen)
    out, lse, _ = _check_attn(q, k, v, lens, lens, scale, f"leak base hd{hd}")
    pos = torch.cat([torch.arange(n, device=DEV) for n in lens])
    P = torch.cat([torch.full((n,), n // 2, device=DEV) for n in lens])           # 0, 8, 100, 32: inside a step, not on its edge
    behind = pos > P
    assert behind.sum() > 100
    k2 = (k * (1 + 1000 * behind[:, None, None].float())).contiguous()
    out2, lse2 = _run(q, k2, v, lens, lens, scale)
    assert torch.isfinite(out2).all() and torch.isfinite(lse2).all()
    assert torch.equal(out2[~behind], out[~behind]) and torch.equal(lse2[:, ~behind], lse[:, ~behind])
    assert not torch.equal(out2[behind], out[behind])                              # the queries behind P do see them


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def test_entry_refuses_what_it_cannot_run():
    """RPO_ERR_UNSUPPORTED before any launch: the buffers here are far smaller than what the refused shapes would read."""
    from rankpo_amd import _lib
    lib = _lib.load()
    OK, UNS = 0, -2
    st = torch.cuda.current_stream().cuda_stream
    xf = torch.zeros(4096 * 8, dtype=F32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    p = xf.data_ptr()

    def attn(ptr=p, stride=256, tl=tiles, cols=2, qb=32, nh=2, nkv=1, hd=64, out=p + 4096 * 4, n=1):
        return lib.rpo_causal_attn_fwd_f32(ptr, ptr, ptr, stride, stride, stride, cu.data_ptr(), cu.data_ptr(), tl.data_ptr(), n,
                                           cols, qb, 1, nh, nkv, hd, 0.1, out, 128, None, st)
    assert attn() == OK                                        # the checks below do not refuse everything
    assert attn(n=0) == OK                                     # an empty work list: nothing to launch
    assert attn(hd=32) == UNS
    assert attn(hd=96, stride=768) == UNS
    assert attn(nh=3, nkv=2) == UNS                            # nh % nkv
    assert attn(nh=3, nkv=1) == UNS                            # 3 query heads per kv head
    assert attn(nh=16, nkv=1, stride=4096) == UNS              # 16
    assert attn(tl=tiles3, cols=3) == UNS                      # another table format
    assert attn(qb=64) == UNS
    assert attn(ptr=p + 4) == UNS                              # misaligned q / k / v
    assert attn(out=p + 4096 * 4 + 8) == UNS                   # misaligned out
    assert attn(stride=194) == UNS                             # rows not 16-byte aligned
    torch.cuda.synchronize()
    # the Python wrapper restates the rule
    o = ops()
    q = torch.zeros(4, 2, 64, device=DEV)
    assert o.causal_attn_f32_ok(q, q[:, :1], q[:, :1]) and o.causal_attn_f32_ok(q, q, q)
    assert not o.causal_attn_f32_ok(q.bfloat16(), q.bfloat16(), q.bfloat16()) and not o.causal_attn_f32_ok(q.cpu(), q.cpu(), q.cpu())
    q32 = torch.zeros(4, 3, 32, device=DEV)
    assert not o.causal_attn_f32_ok(q32, q32, q32)
    q3 = torch.zeros(4, 3, 64, device=DEV)
    assert not o.causal_attn_f32_ok(q3, q3[:, :1], q3[:, :1]) and not o.causal_attn_f32_ok(q3, q3[:, :2], q3[:, :2])
    odd = torch.zeros(4, 2 * 64 + 2, device=DEV)[:, :128].view(4, 2, 64)         # token stride 130
    assert not o.causal_attn_f32_ok(odd, odd, odd)
    with pytest.raises(ValueError):
        o.causal_attn_f32(q32, q32, q32, cu, cu, tiles, 0.1)
    with pytest.raises(ValueError):
        o.causal_attn_f32_tile_table([5], [4], DEV)


# ------------------------------------------------------------------------------------------------
# end to end: ModelForInference.encode on an f32 Llama encoder
# ------------------------------------------------------------------------------------------------
def _errors(got, ref):
    got, ref = got.double(), ref.double()
    cos = (got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))
    return float((1 - cos).abs().max()), float((got - ref).abs().max())


def _build(hd, seed, **kw):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import CharTok, _cfg
    torch.manual_seed(seed)
    cfg = _cfg(PE, hd)
    enc = PE.LlamaEncoder(cfg)
    w32 = E.state_dict_to_f32(enc)
    return PE, cfg, w32, rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), device=0, **kw)


class Spy:
    """Counts the new op, stock SDPA, and host reads of device tensors."""

    def __init__(self):
        self.n = {"causal_attn_f32": 0, "full": 0, "last": 0, "sdpa": 0, "syncs": 0}

    def __enter__(self):
        o = ops()
        self._op, self._sdpa = o.causal_attn_f32, F.scaled_dot_product_attention
        self._tolist, self._item = torch.Tensor.tolist, torch.Tensor.item

        def op(q, k, *a, **kw):
            self.n["causal_attn_f32"] += 1
            self.n["full" if q.shape[0] == k.shape[0] else "last"] += 1
            return self._op(q, k, *a, **kw)

        def sdpa(*a, **kw):
            self.n["sdpa"] += 1
            return self._sdpa(*a, **kw)

        def tolist(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._tolist(t)

        def item(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._item(t)
        o.causal_attn_f32, F.scaled_dot_product_attention = op, sdpa
        torch.Tensor.tolist, torch.Tensor.item = tolist, item
        return self

    def __exit__(self, *exc):
        ops().causal_attn_f32, F.scaled_dot_product_attention = self._op, self._sdpa
        torch.Tensor.tolist, torch.Tensor.item = self._tolist, self._item
        return False


KW = dict(batch_size=12, max_length=384)


@pytest.fixture(scope="module", params=[64, 128])
def f32_case(request):
    """One f32 model per config (switch off), the same weights with f32_attention=True, the texts, the float64 oracle rows (CPU)
    and the switch-off rows (the control): computed once, shared by the tests below, never modified."""
    from test_gpu_inference import CharTok, _texts
    hd = request.param
    PE, cfg, w32, inf = _build(hd, 20 + hd)
    _, _, w32_on, inf_on = _build(hd, 20 + hd, f32_attention=True)
    assert all(torch.equal(w32[k], w32_on[k]) for k in w32)
    assert inf.model.embed_tokens.weight.dtype == F32 and not inf.model.f32_attention and inf_on.model.f32_attention
    assert not PE.LLAMA_F32_ATTENTION
    rs = np.random.RandomState(hd)
    texts = _texts(rs, 23, 40, 400) + ["q"] + _texts(rs, 8, 380, 400)        # 3 batches of 12 / 12 / 8; one 1-token row
    tok = CharTok()(texts, max_length=384)
    w64 = {k: v.double() for k, v in w32.items()}
    with torch.no_grad():
        ref = E.embed(w64, cfg.to_dict(), tok, dtype=torch.float64).detach()
    assert ref.dtype == torch.float64
    off = inf.encode(texts, **KW)
    return dict(hd=hd, PE=PE, cfg=cfg, inf=inf, inf_on=inf_on, texts=texts, ref=ref, off=off)


def test_encode_switch_off_runs_what_it_ran(f32_case):
    c = f32_case
    with Spy() as spy:
        a = c["inf"].encode(c["texts"], **KW)
    assert spy.n["causal_attn_f32"] == 0 and spy.n["sdpa"] > 0 and spy.n["syncs"] == 0, spy.n
    np.testing.assert_array_equal(a, c["off"])


def test_encode_f32_attention_vs_oracle(f32_case, monkeypatch):
    c = f32_case
    cfg, ref = c["cfg"], c["ref"]
    with Spy() as spy:
        out = c["inf_on"].encode(c["texts"], **KW)
    nb, nl = 3, cfg.num_hidden_layers
    n = spy.n
    assert n["causal_attn_f32"] == nb * nl and n["full"] == nb * (nl - 1) and n["last"] == nb, n
    assert n["sdpa"] == 0, n
    assert n["syncs"] == 0, "encode() synchronised on a device tensor's contents"
    assert out.dtype == np.float32 and out.shape == (32, cfg.hidden_size) and np.isfinite(out).all()
    f_cos, f_abs = _errors(torch.tensor(out), ref)
    c_cos, c_abs = _errors(torch.tensor(c["off"]), ref)
    print(f"\nencode f32 llama hd{c['hd']}: f32 attention cos err {f_cos:.2e} abs {f_abs:.2e}; "
          f"per-sequence SDPA control {c_cos:.2e} / {c_abs:.2e}")
    assert f_abs <= 1.5 * c_abs + ULP2 and f_cos <= 1.5 * c_cos + ULP2 ** 2, (f_cos, c_cos, f_abs, c_abs)
    # the module switch on the switch-off model: the same path, the same rows
    monkeypatch.setattr(c["PE"], "LLAMA_F32_ATTENTION", True)
    with Spy() as spy:
        out_m = c["inf"].encode(c["texts"], **KW)
    assert spy.n["causal_attn_f32"] == nb * nl and spy.n["sdpa"] == 0, spy.n
    np.testing.assert_array_equal(out_m, out)


def test_left_padded_batches_give_the_switch_off_rows(f32_case):
    from test_gpu_bert_native import LeftTok
    from test_gpu_inference import _texts
    c = f32_case
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
        assert spy.n["causal_attn_f32"] == 0 and spy.n["sdpa"] > 0, spy.n
    np.testing.assert_array_equal(rows[0], rows[1])


def test_grad_mode_runs_what_it_ran(f32_case, monkeypatch):
    from test_gpu_inference import CharTok, _texts
    c = f32_case
    monkeypatch.setattr(c["PE"], "LLAMA_F32_ATTENTION", True)               # both switches on for inf_on
    tok = CharTok()(_texts(np.random.RandomState(9), 5, 3, 70) + ["q"], max_length=64)
    grads = []
    for inf, on in ((c["inf_on"], True), (c["inf"], False)):
        if not on:
            monkeypatch.setattr(c["PE"], "LLAMA_F32_ATTENTION", False)
        inf.model.zero_grad(set_to_none=True)
        with Spy() as spy:
            pooled = inf.model.pooled_last_token(tok["input_ids"], tok["attention_mask"])
            pooled.sum().backward()
        assert spy.n["causal_attn_f32"] == 0 and spy.n["sdpa"] > 0, spy.n
        grads.append({k: p.grad.clone() for k, p in inf.model.named_parameters()})
        inf.model.zero_grad(set_to_none=True)
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 10
    for k in grads[0]:
        assert torch.isfinite(grads[0][k]).all() and torch.equal(grads[0][k], grads[1][k]), k
    assert sum(float(g.abs().sum()) for g in grads[0].values()) > 0


@pytest.mark.parametrize("hd", [64, 128])
def test_bf16_model_ignores_both_switches(hd, monkeypatch):
    from test_gpu_inference import _texts
    texts = _texts(np.random.RandomState(8), 9, 5, 200)
    PE, cfg, _, inf = _build(hd, 9, use_bf16=True)
    a = inf.encode(texts, batch_size=4, max_length=256)
    _, _, _, inf_on = _build(hd, 9, use_bf16=True, f32_attention=True)
    monkeypatch.setattr(PE, "LLAMA_F32_ATTENTION", True)
    assert inf_on.model.f32_attention and inf_on.model.embed_tokens.weight.dtype == torch.bfloat16
    with Spy() as spy:
        b = inf_on.encode(texts, batch_size=4, max_length=256)
    assert spy.n["causal_attn_f32"] == 0, spy.n
    np.testing.assert_array_equal(a, b)
