"""The packed BERT / XLM-R forward (bert_ops.hip, `BertEncoder.pooled_cls`, `ModelForInference.encode` for CLS-pooled models):
each kernel against float64, and the encode path end to end against the float32 oracle by the repo's control rule."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
MANT = {torch.bfloat16: 7, torch.float16: 10}        # explicit mantissa bits
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}
LN_FLOOR = 2.0 ** -6       # LayerNorm outputs are O(1): 1 ulp at 1/64 of that scale below it
LENS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 1000]


def ops():
    from rankpo_amd import ops as o
    return o


def _ulp(ref, dtype):
    """Spacing of `dtype` at |ref| (float64 tensor)."""
    a = ref.abs().clamp_min(MIN_NORMAL[dtype])
    return torch.exp2(torch.floor(torch.log2(a)) - MANT[dtype])


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
def _ref_attn(q, k, v, cu_q, cu_k, scale):
    """float64 per sequence on the device: (out [Tq, nh, hd], lse [nh, Tq])."""
    outs, lses = [], []
    for n in range(len(cu_q) - 1):
        qs, ks, vs = (t.double() for t in (q[cu_q[n]:cu_q[n + 1]], k[cu_k[n]:cu_k[n + 1]], v[cu_k[n]:cu_k[n + 1]]))
        s = torch.einsum("qhd,khd->hqk", qs, ks) * scale
        lse = torch.logsumexp(s, -1)
        outs.append(torch.einsum("hqk,khd->qhd", torch.exp(s - lse[..., None]), vs))
        lses.append(lse)
    return torch.cat(outs), torch.cat(lses, 1)


def _ctrl_attn(q, k, v, cu_q, cu_k, scale):
    """torch SDPA in the storage dtype, per sequence: the control of the error rule."""
    outs = []
    for n in range(len(cu_q) - 1):
        qs, ks, vs = (t.transpose(0, 1)[None] for t in (q[cu_q[n]:cu_q[n + 1]], k[cu_k[n]:cu_k[n + 1]], v[cu_k[n]:cu_k[n + 1]]))
        outs.append(F.scaled_dot_product_attention(qs, ks, vs, scale=scale)[0].transpose(0, 1))
    return torch.cat(outs)


def _check_attn(q, k, v, lens_q, lens_k, dtype, scale, label):
    o = ops()
    cu_q = [0] + np.cumsum(lens_q).tolist()
    cu_k = [0] + np.cumsum(lens_k).tolist()
    cq = torch.tensor(cu_q, dtype=torch.int32, device=DEV)
    ck = torch.tensor(cu_k, dtype=torch.int32, device=DEV)
    tiles = o.bidir_attn_tile_table(lens_q, lens_k, DEV)
    out, lse = o.bidir_attn_fwd(q, k, v, cq, ck, tiles, scale, want_lse=True)
    ref, ref_lse = _ref_attn(q, k, v, cu_q, cu_k, scale)
    ctrl = _ctrl_attn(q, k, v, cu_q, cu_k, scale)
    nh, hd = q.shape[1], q.shape[2]
    got = out.view(-1, nh, hd).double()
    assert torch.isfinite(got).all() and torch.isfinite(lse).all(), label
    err = (got - ref).abs().max().item()
    c_err = (ctrl.double() - ref).abs().max().item()
    floor = 2 * _ulp(ref.abs().max(), dtype).item()
    print(f"\n{label}: kernel {err:.3e}, sdpa control {c_err:.3e}, floor {floor:.3e}")
    assert err <= 1.5 * c_err + floor, (label, err, c_err, floor)
    assert (lse.double() - ref_lse).abs().max().item() < 1e-3 * max(1.0, ref_lse.abs().max().item()), label


def _fused(T, nh, hd, dtype, gen, mult=1.0):
    """q / k / v as column blocks of ONE [T, 3 nh hd] buffer (the fused projection output): token stride 3 nh hd."""
    qkv = (torch.randn(T, 3 * nh * hd, generator=gen, device=DEV) * mult).to(dtype)
    d = nh * hd
    return qkv, (qkv[:, j * d:(j + 1) * d].view(T, nh, hd) for j in range(3))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,nh", [(32, 4), (32, 12), (64, 12), (64, 16)])
def test_bidir_attention_matches_f64(dtype, hd, nh):
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh)
    T = sum(LENS)
    qkv, (q, k, v) = _fused(T, nh, hd, dtype, gen)
    assert q.stride(0) == 3 * nh * hd
    scale = 1.0 / math.sqrt(hd)
    _check_attn(q, k, v, LENS, LENS, dtype, scale, f"self hd{hd} nh{nh} {dtype}")
    # the CLS-only mode: one query per sequence (its first token), every key of the sequence
    cls = torch.tensor([0] + np.cumsum(LENS)[:-1].tolist(), device=DEV)
    qc = q.reshape(T, -1).index_select(0, cls).view(-1, nh, hd)
    _check_attn(qc, k, v, [1] * len(LENS), LENS, dtype, scale, f"cls hd{hd} nh{nh} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_bidir_attention_8192_keys(dtype):
    gen = torch.Generator(device=DEV).manual_seed(8192)
    lens = [8192, 3]
    _, (q, k, v) = _fused(sum(lens), 4, 64, dtype, gen)
    _check_attn(q, k, v, lens, lens, dtype, 0.125, f"8192 keys {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd", [32, 64])
def test_bidir_attention_hard_inputs(dtype, hd):
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, lens = 4, [1, 17, 200, 65]
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    # saturated softmax: scores ~ +-60 after scaling (one key per query dominates)
    mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
    _, (q, k, v) = _fused(T, nh, hd, dtype, gen, mult)
    v = v / mult
    _check_attn(q, k, v, lens, lens, dtype, scale, f"saturated hd{hd} {dtype}")
    # identical keys: uniform weights, the output is the mean of V
    _, (q, k, v) = _fused(T, nh, hd, dtype, gen)
    k = k[:1].expand(T, nh, hd).contiguous()
    _check_attn(q, k, v, lens, lens, dtype, scale, f"identical keys hd{hd} {dtype}")


# ------------------------------------------------------------------------------------------------
# LayerNorm / GELU / embedding + LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln64(s, g, b, eps):
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    return (s - mu) / torch.sqrt(var + eps) * g.double() + b.double()


def _within_one_ulp(got, ref, dtype, label, floor):
    """|got - ref| <= 1 ulp of `dtype` at max(|ref|, floor): below `floor` the f32 arithmetic's own absolute error (the same in
    torch's kernels: cancellation in 1 + erf(x / sqrt 2), the f32 statistics of LayerNorm) is larger than the spacing there."""
    bad = (got.double() - ref).abs() > _ulp(ref.abs().clamp_min(floor), dtype)
    assert not bad.any(), (label, int(bad.sum()), (got.double() - ref).abs().max().item())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [384, 768, 1024, 136])
def test_add_layernorm_one_ulp(dtype, d):
    gen = torch.Generator(device=DEV).manual_seed(d)
    rows = 37
    a = (torch.randn(rows, d, generator=gen, device=DEV) * 2).to(dtype)
    big = (torch.randn(rows, 2 * d, generator=gen, device=DEV)).to(dtype)
    b = big[:, :d]                                             # row-strided dense output
    g = (1 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
    be = (0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
    out = torch.full((rows, d + 8), float("nan"), dtype=dtype, device=DEV)
    y = ops().add_layernorm(a, b, g, be, 1e-12, out=out[:, :d])
    s = (a.double() + b.double()).to(dtype).double()           # the reference's rounded sum
    _within_one_ulp(y, _ln64(s, g, be, 1e-12), dtype, f"add_ln d{d}", LN_FLOOR)
    assert torch.isnan(out[:, d:].float()).all()               # nothing beyond the row
    y2 = ops().add_layernorm(a, None, g, be, 1e-5)
    _within_one_ulp(y2, _ln64(a.double(), g, be, 1e-5), dtype, f"ln d{d}", LN_FLOOR)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_one_ulp(dtype):
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.randn(33, 1536, generator=gen, device=DEV) * 3).to(dtype)
    x64 = x.double()
    ref = 0.5 * x64 * (1 + torch.erf(x64 / math.sqrt(2)))
    y = ops().gelu_(x.clone())
    _within_one_ulp(y, ref, dtype, "gelu", 2.0 ** -10)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("with_types", [True, False])
def test_embed_layernorm_one_ulp(dtype, with_types):
    gen = torch.Generator(device=DEV).manual_seed(11)
    d, V, P, TT, T = 768, 300, 514, 2, 97
    word, pe = (torch.randn(n, d, generator=gen, device=DEV).to(dtype) for n in (V, P))
    te = torch.randn(TT, d, generator=gen, device=DEV).to(dtype)
    g = (1 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
    be = (0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
    ids = torch.randint(0, V, (T,), generator=gen, device=DEV, dtype=torch.int32)
    pos = torch.randint(0, P, (T,), generator=gen, device=DEV, dtype=torch.int32)
    tts = torch.randint(0, TT, (T,), generator=gen, device=DEV, dtype=torch.int32) if with_types else None
    y = ops().bert_embed_ln(ids, pos, tts, word, te, pe, g, be, 1e-12)
    t_rows = te[tts.long()] if with_types else te[0].expand(T, d)
    s = (word[ids.long()].double() + t_rows.double()).to(dtype).double()
    s = (s + pe[pos.long()].double()).to(dtype).double()
    _within_one_ulp(y, _ln64(s, g, be, 1e-12), dtype, "embed_ln", LN_FLOOR)


def test_unsupported_shapes_and_dtypes():
    from rankpo_amd import _lib
    lib = _lib.load()
    UNS = -2
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(4096 * 8, dtype=torch.float16, device=DEV)
    xf = torch.zeros(4096 * 8, dtype=torch.float32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    p, pf = x.data_ptr(), xf.data_ptr()

    def attn(ptr=p, stride=192, tl=tiles, cols=2, qb=32, nh=2, nkv=2, hd=32, dt=2):
        return lib.rpo_bidir_attn_fwd(ptr, ptr, ptr, stride, stride, stride, cu.data_ptr(), cu.data_ptr(), tl.data_ptr(), 1, cols,
                                      qb, 4, nh, nkv, hd, dt, 0.1, ptr, 64, None, st)
    assert attn(hd=128, stride=768) == UNS
    assert attn(hd=16) == UNS
    assert attn(ptr=pf, dt=0) == UNS                           # f32 storage
    assert attn(nkv=1) == UNS                                  # grouped heads
    assert attn(tl=tiles3, cols=3) == UNS                      # another table format
    assert attn(qb=64) == UNS
    assert lib.rpo_add_layernorm_fwd(p, 12, p, 12, p, p, 1e-5, p, 12, 2, 12, 2, st) == UNS        # d % 8
    assert lib.rpo_add_layernorm_fwd(p, 4104, p, 4104, p, p, 1e-5, p, 4104, 2, 4104, 2, st) == UNS  # d > 4096
    assert lib.rpo_add_layernorm_fwd(pf, 64, pf, 64, pf, pf, 1e-5, pf, 64, 2, 64, 0, st) == UNS
    assert lib.rpo_gelu_fwd(p, 2, 12, 12, 2, st) == UNS
    assert lib.rpo_gelu_fwd(pf, 2, 64, 64, 0, st) == UNS
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib.rpo_bert_embed_ln_fwd(ids.data_ptr(), None, ids.data_ptr(), 2, p, 4, p, 1, p, 4, p, p, 1e-5, p, 12, 12, 2,
                                     st) == UNS
    assert lib.rpo_bert_embed_ln_fwd(ids.data_ptr(), None, ids.data_ptr(), 2, pf, 4, pf, 1, pf, 4, pf, pf, 1e-5, pf, 64, 64, 0,
                                     st) == UNS
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# end to end: ModelForInference.encode
# ------------------------------------------------------------------------------------------------
def _cfg(PE, kind):
    if kind == "bge-small":          # head_dim 32, BERT positions
        return PE.bge_small_config(vocab_size=1024, hidden_size=128, intermediate_size=512, num_hidden_layers=3,
                                   num_attention_heads=4, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    return PE.xlm_roberta_config(vocab_size=1024, hidden_size=256, intermediate_size=1024, num_hidden_layers=2,   # head_dim 64
                                 num_attention_heads=4, max_position_embeddings=514, hidden_dropout_prob=0.1,
                                 attention_probs_dropout_prob=0.1)


class Spy:
    """Counts the new entry points and the stock ops the native path replaces."""
    NAMES = ("bidir_attn_fwd", "add_layernorm", "gelu_", "bert_embed_ln")

    def __init__(self):
        self.n = {k: 0 for k in self.NAMES + ("sdpa", "layernorm", "syncs")}

    def __enter__(self):
        o = ops()
        self._real = {k: getattr(o, k) for k in self.NAMES}
        for k in self.NAMES:
            def wrap(*a, _k=k, **kw):
                self.n[_k] += 1
                return self._real[_k](*a, **kw)
            setattr(o, k, wrap)
        self._sdpa, self._ln = F.scaled_dot_product_attention, torch.nn.LayerNorm.forward
        self._tolist, self._item = torch.Tensor.tolist, torch.Tensor.item

        def sdpa(*a, **kw):
            self.n["sdpa"] += 1
            return self._sdpa(*a, **kw)

        def ln(mod, *a, **kw):
            self.n["layernorm"] += 1
            return self._ln(mod, *a, **kw)

        def tolist(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._tolist(t)

        def item(t):
            self.n["syncs"] += int(t.is_cuda)
            return self._item(t)
        F.scaled_dot_product_attention, torch.nn.LayerNorm.forward = sdpa, ln
        torch.Tensor.tolist, torch.Tensor.item = tolist, item
        return self

    def __exit__(self, *exc):
        o = ops()
        for k in self.NAMES:
            setattr(o, k, self._real[k])
        F.scaled_dot_product_attention, torch.nn.LayerNorm.forward = self._sdpa, self._ln
        torch.Tensor.tolist, torch.Tensor.item = self._tolist, self._item
        return False


def _errors(got, ref):
    got, ref = got.double(), ref.double()
    cos = (got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))
    return float((1 - cos).abs().max()), float((got - ref).abs().max())


def _model(kind, dtype, seed):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_inference import CharTok
    torch.manual_seed(seed)
    cfg = _cfg(PE, kind)
    enc = PE.build_encoder(cfg)
    w32 = E.state_dict_to_f32(enc)
    flags = {"use_fp16": True} if dtype == torch.float16 else ({"use_bf16": True} if dtype == torch.bfloat16 else {})
    inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), device=0, **flags)
    return PE, cfg, w32, inf


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_encode_native_path_vs_oracle(kind, dtype):
    from test_gpu_inference import CharTok, _texts
    PE, cfg, w32, inf = _model(kind, dtype, 31)
    rs = np.random.RandomState(4)
    texts = _texts(rs, 21, 20, 300) + ["q"] + _texts(rs, 6, 280, 300)          # 3 batches of 10 / 10 / 8, one 1-token row
    tok = CharTok()(texts, max_length=320)
    ref = E.embed(w32, cfg.to_dict(), tok).detach()
    wd = {k: v.detach() for k, v in inf.model.state_dict().items()}
    with torch.no_grad():
        ctrl = E.embed(wd, cfg.to_dict(), {k: v.to(DEV) for k, v in tok.items()}, dtype=dtype).float().cpu()
    c_cos, c_abs = _errors(ctrl, ref)
    with Spy() as spy:
        out = inf.encode(texts, batch_size=10, max_length=320)
    nb, nl = 3, cfg.num_hidden_layers
    n = spy.n
    assert n["bidir_attn_fwd"] == nb * nl and n["add_layernorm"] == 2 * nb * nl and n["gelu_"] == nb * nl, n
    assert n["bert_embed_ln"] == nb and n["sdpa"] == 0 and n["layernorm"] == 0, n
    assert n["syncs"] == 0, "encode() synchronised on a device tensor's contents"
    assert out.shape == (28, cfg.hidden_size) and np.isfinite(out.astype(np.float64)).all()
    f_cos, f_abs = _errors(torch.tensor(out.astype(np.float32)), ref)
    print(f"\nencode {kind} {dtype}: native cos err {f_cos:.2e} abs {f_abs:.2e}; eager control {c_cos:.2e} / {c_abs:.2e}")
    floor = 2 * 2.0 ** -MANT[dtype]
    assert f_cos <= 1.5 * c_cos + floor ** 2 and f_abs <= 1.5 * c_abs + floor, (f_cos, c_cos, f_abs, c_abs)
    # bucket_by_length: other batches, rows back in input order
    out_b = inf.encode(texts, batch_size=10, max_length=320, bucket_by_length=True)
    assert np.abs(out_b.astype(np.float64) - out.astype(np.float64)).max() < 4 * 2.0 ** -MANT[dtype]


class LeftTok:
    """CharTok with LEFT padding: column 0 is a pad token for every row but the longest."""
    pad_token = "<pad>"
    padding_side = "left"

    def __call__(self, texts, **kw):
        from test_gpu_inference import CharTok
        o = CharTok()(texts, **kw)
        return {k: torch.flip(v, [1]) for k, v in o.items()}


@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_declined_batches_and_models_give_the_old_rows(kind, monkeypatch):
    from test_gpu_inference import _texts
    PE, cfg, w32, inf = _model(kind, torch.float16, 9)
    texts = _texts(np.random.RandomState(8), 7, 5, 60)

    def both(model_inf, **kw):
        with Spy() as spy:
            a = model_inf.encode(texts, batch_size=4, max_length=64, **kw)
        monkeypatch.setattr(PE, "BERT_NATIVE", False)
        b = model_inf.encode(texts, batch_size=4, max_length=64, **kw)
        monkeypatch.setattr(PE, "BERT_NATIVE", True)
        return a, b, spy.n
    # left padding: the CLS column holds pad tokens -> declined, the padded path's rows bit for bit
    inf.tokenizer = LeftTok()
    a, b, n = both(inf)
    assert n["bidir_attn_fwd"] == 0 and n["sdpa"] > 0, n
    np.testing.assert_array_equal(a, b)
    # an f32 model: declined
    _, _, _, inf32 = _model(kind, None, 9)
    a, b, n = both(inf32)
    assert n["bidir_attn_fwd"] == 0 and n["sdpa"] > 0, n
    np.testing.assert_array_equal(a, b)
    # train mode with dropout: pooled_cls declines (encode itself always runs eval mode)
    from test_gpu_inference import CharTok
    tok = CharTok()(texts, max_length=64)
    inf.model.train()
    with torch.no_grad():
        assert inf.model.pooled_cls(tok["input_ids"], tok["attention_mask"]) is None
        inf.model.eval()
        got = inf.model.pooled_cls(tok["input_ids"], tok["attention_mask"])
        pad = inf.model(input_ids=tok["input_ids"].to(DEV), attention_mask=tok["attention_mask"].to(DEV)).last_hidden_state[:, 0]
    assert got is not None and got.shape == pad.shape
    assert (got.double() - pad.double()).abs().max().item() < 0.05
    # a holed mask: the native CLS rows equal the padded path's (positions from the padded layout)
    m = tok["attention_mask"].clone()
    m[:, 2] = 0
    m[:, 0] = 1
    with torch.no_grad():
        got = inf.model.pooled_cls(tok["input_ids"], m)
        pad = inf.model(input_ids=tok["input_ids"].to(DEV), attention_mask=m.to(DEV)).last_hidden_state[:, 0]
    assert got is not None
    assert (got.double() - pad.double()).abs().max().item() < 0.05
