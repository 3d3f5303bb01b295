"""The packed f32 forward of the BERT / XLM-R encoder (header section 9b: rpo_bidir_attn_fwd_f32 and the row kernels on float;
`BertEncoder.native_f32` / `encoder.BERT_NATIVE_F32` / `ModelForInference(packed_f32=True)`).

Error rule (the project's own, test_gpu_bert_native.py `_check_attn`): err <= 1.5 * control_err + floor, both errors max-abs
against a float64 reference computed here, the control stock torch in f32 on the same inputs, floor = 2 ulp of f32 (23 explicit
mantissa bits) at max|ref|.  With an f32 control (about 1e-7) the rule fails any kernel that rounds P or an intermediate to 16 bits."""
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
# attention
# ------------------------------------------------------------------------------------------------
def _seqs(q, k, v, cu_q, cu_k):
    for n in range(len(cu_q) - 1):
        yield q[cu_q[n]:cu_q[n + 1]], k[cu_k[n]:cu_k[n + 1]], v[cu_k[n]:cu_k[n + 1]]


def _ref_attn(q, k, v, cu_q, cu_k, scale):
    """float64 per sequence on the device: (out [Tq, nh, hd], lse [nh, Tq])."""
    outs, lses = [], []
    for qs, ks, vs in _seqs(q, k, v, cu_q, cu_k):
        s = torch.einsum("qhd,khd->hqk", qs.double(), ks.double()) * scale
        lse = torch.logsumexp(s, -1)
        outs.append(torch.einsum("hqk,khd->qhd", torch.exp(s - lse[..., None]), vs.double()))
        lses.append(lse)
    return torch.cat(outs), torch.cat(lses, 1)


def _ctrl_attn(q, k, v, cu_q, cu_k, scale):
    """Stock torch in f32 per sequence: SDPA for the output, logsumexp of the f32 scores for lse."""
    outs, lses = [], []
    for qs, ks, vs in _seqs(q, k, v, cu_q, cu_k):
        qt, kt, vt = (t.transpose(0, 1)[None] for t in (qs, ks, vs))
        outs.append(F.scaled_dot_product_attention(qt, kt, vt, scale=scale)[0].transpose(0, 1))
        lses.append(torch.logsumexp(torch.einsum("qhd,khd->hqk", qs, ks) * scale, -1))
    return torch.cat(outs), torch.cat(lses, 1)


def _check_attn(q, k, v, lens_q, lens_k, scale, label):
    o = ops()
    cu_q = [0] + np.cumsum(lens_q).tolist()
    cu_k = [0] + np.cumsum(lens_k).tolist()
    cq = torch.tensor(cu_q, dtype=torch.int32, device=DEV)
    ck = torch.tensor(cu_k, dtype=torch.int32, device=DEV)
    tiles = o.bidir_attn_tile_table(lens_q, lens_k, DEV)
    out, lse = o.bidir_attn_fwd(q, k, v, cq, ck, tiles, scale, want_lse=True)
    assert out.dtype == F32 and lse.dtype == F32
    out2, none = o.bidir_attn_fwd(q, k, v, cq, ck, tiles, scale)               # lse NULL: the same rows
    assert none is None and torch.equal(out, out2), label
    ref, ref_lse = _ref_attn(q, k, v, cu_q, cu_k, scale)
    ctrl, ctrl_lse = _ctrl_attn(q, k, v, cu_q, cu_k, scale)
    nh, hd = q.shape[1], q.shape[2]
    _rule(out.view(-1, nh, hd), ctrl, ref, label)
    _rule(lse, ctrl_lse, ref_lse, label + " lse")


def _fused(T, nh, hd, gen, mult=1.0):
    """q / k / v as column blocks of ONE [T, 3 nh hd] f32 buffer (the fused projection output): token stride 3 nh hd."""
    qkv = torch.randn(T, 3 * nh * hd, generator=gen, device=DEV) * mult
    d = nh * hd
    return qkv, (qkv[:, j * d:(j + 1) * d].view(T, nh, hd) for j in range(3))


@pytest.mark.parametrize("hd,nh", [(32, 4), (64, 12)])
def test_attention_f32_matches_f64(hd, nh):
    gen = torch.Generator(device=DEV).manual_seed(hd * 100 + nh)
    T = sum(LENS)
    qkv, (q, k, v) = _fused(T, nh, hd, gen)
    assert q.stride(0) == 3 * nh * hd and q.dtype == F32
    assert not torch.equal(q, q.bfloat16().float())            # randn: not exact in bf16
    scale = 1.0 / math.sqrt(hd)
    _check_attn(q, k, v, LENS, LENS, scale, f"self hd{hd} nh{nh}")
    # the CLS-only mode: one query per sequence (its first token), every key of the sequence
    cls = torch.tensor([0] + np.cumsum(LENS)[:-1].tolist(), device=DEV)
    qc = q.reshape(T, -1).index_select(0, cls).view(-1, nh, hd)
    _check_attn(qc, k, v, [1] * len(LENS), LENS, scale, f"cls hd{hd} nh{nh}")


def test_attention_f32_8192_keys():
    gen = torch.Generator(device=DEV).manual_seed(8192)
    lens = [8192, 3]
    _, (q, k, v) = _fused(sum(lens), 4, 64, gen)
    _check_attn(q, k, v, lens, lens, 0.125, "8192 keys")


@pytest.mark.parametrize("hd", [32, 64])
def test_attention_f32_hard_inputs(hd):
    gen = torch.Generator(device=DEV).manual_seed(7 + hd)
    nh, lens = 4, [1, 17, 200, 65]
    T = sum(lens)
    scale = 1.0 / math.sqrt(hd)
    # saturated softmax: scores ~ +-60 after scaling (one key per query dominates)
    mult = math.sqrt(60.0 / (scale * math.sqrt(hd)))
    _, (q, k, v) = _fused(T, nh, hd, gen, mult)
    v = v / mult
    _check_attn(q, k, v, lens, lens, scale, f"saturated hd{hd}")
    # identical keys: uniform weights, the output is the mean of V
    _, (q, k, v) = _fused(T, nh, hd, gen)
    k = k[:1].expand(T, nh, hd).contiguous()
    _check_attn(q, k, v, lens, lens, scale, f"identical keys hd{hd}")


# ------------------------------------------------------------------------------------------------
# LayerNorm / GELU / embedding + LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln64(s, g, b, eps):
    mu = s.mean(-1, keepdim=True)
    var = ((s - mu) ** 2).mean(-1, keepdim=True)
    return (s - mu) / torch.sqrt(var + eps) * g.double() + b.double()


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("d", [8, 384, 768, 1024, 4096])
def test_add_layernorm_f32(d, rows):
    gen = torch.Generator(device=DEV).manual_seed(d + rows)
    a = torch.randn(rows, d, generator=gen, device=DEV) * 2
    b = torch.randn(rows, 2 * d, generator=gen, device=DEV)[:, :d]              # row-strided dense output
    g = 1 + 0.1 * torch.randn(d, generator=gen, device=DEV)
    be = 0.1 * torch.randn(d, generator=gen, device=DEV)
    out = torch.full((rows, d + 8), float("nan"), device=DEV)                   # an output row stride larger than d
    y = ops().add_layernorm(a, b, g, be, 1e-12, out=out[:, :d])
    assert y.data_ptr() == out.data_ptr() and torch.isnan(out[:, d:]).all()     # nothing beyond the row
    _rule(y, F.layer_norm(a + b, (d,), g, be, 1e-12), _ln64(a.double() + b.double(), g, be, 1e-12), f"add_ln d{d} rows{rows}")
    y2 = ops().add_layernorm(a, None, g, be, 1e-5)                               # b NULL
    assert y2.is_contiguous() and y2.dtype == F32
    _rule(y2, F.layer_norm(a, (d,), g, be, 1e-5), _ln64(a.double(), g, be, 1e-5), f"ln d{d} rows{rows}")


def test_gelu_f32():
    gen = torch.Generator(device=DEV).manual_seed(5)
    cols = 4096
    big = torch.full((4, cols + 8), float("nan"), device=DEV)
    x = big[:, :cols]                                                           # row stride cols + 8
    x[0] = torch.linspace(-10, 10, cols, device=DEV)                            # |x| up to 10: both tails
    x[1] = torch.linspace(-2.0 ** -10, 2.0 ** -10, cols, device=DEV)            # a grid around 0
    x[2] = torch.randn(cols, generator=gen, device=DEV) * 3
    x[3] = torch.cat([torch.zeros(8, device=DEV), torch.randn(cols - 8, generator=gen, device=DEV) * 1e-4])
    x64 = x.double()
    ref = 0.5 * x64 * (1 + torch.erf(x64 / math.sqrt(2)))
    ctrl = F.gelu(x.contiguous())
    y = ops().gelu_(x)
    assert y.data_ptr() == big.data_ptr() and torch.isnan(big[:, cols:]).all()
    _rule(y, ctrl, ref, "gelu")


@pytest.mark.parametrize("case", ["types", "no_types", "roberta_positions"])
def test_embed_layernorm_f32(case):
    from rankpo_amd import encoder as PE
    gen = torch.Generator(device=DEV).manual_seed(11)
    d, V, P, TT = 768, 300, 514, 2
    word, pe = (torch.randn(n, d, generator=gen, device=DEV) for n in (V, P))
    te = torch.randn(TT, d, generator=gen, device=DEV)
    g = 1 + 0.1 * torch.randn(d, generator=gen, device=DEV)
    be = 0.1 * torch.randn(d, generator=gen, device=DEV)
    if case == "roberta_positions":      # positions of a padded [3, 40] batch by the RoBERTa rule (pad id 1: they start at 2)
        cpu = torch.Generator().manual_seed(3)
        lens = [40, 1, 17]
        mask = torch.tensor([[1] * n + [0] * (40 - n) for n in lens])
        ids2 = torch.randint(2, V, (3, 40), generator=cpu) * mask + (1 - mask)
        ids, pos, tts, got_lens = PE.bert_pack(ids2, mask, None, roberta=True, pad_id=1)
        assert got_lens == lens and int(pos.min()) == 2 and int(pos.max()) == 41
        ids, pos = ids.to(DEV, torch.int32), pos.to(DEV, torch.int32)
    else:
        T = 97
        ids = torch.randint(0, V, (T,), generator=gen, device=DEV, dtype=torch.int32)
        pos = torch.randint(0, P, (T,), generator=gen, device=DEV, dtype=torch.int32)
        tts = torch.randint(0, TT, (T,), generator=gen, device=DEV, dtype=torch.int32) if case == "types" else None
    T = ids.shape[0]
    y = ops().bert_embed_ln(ids, pos, tts, word, te, pe, g, be, 1e-12)
    assert y.shape == (T, d) and y.dtype == F32
    t_rows = te[tts.long()] if tts is not None else te[0].expand(T, d)
    ctrl = F.layer_norm((word[ids.long()] + t_rows) + pe[pos.long()], (d,), g, be, 1e-12)
    s64 = word[ids.long()].double() + t_rows.double() + pe[pos.long()].double()
    _rule(y, ctrl, _ln64(s64, g, be, 1e-12), f"embed_ln {case}")


def test_f32_entries_refuse_what_they_cannot_run():
    """RPO_ERR_UNSUPPORTED before any launch: the buffers here are far smaller than what the refused shapes would read."""
    from rankpo_amd import _lib
    lib = _lib.load()
    OK, UNS = 0, -2
    st = torch.cuda.current_stream().cuda_stream
    xf = torch.zeros(4096 * 8, dtype=F32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    tiles3 = torch.zeros(1, 3, dtype=torch.int32, device=DEV)
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = xf.data_ptr()

    def attn(ptr=p, stride=192, tl=tiles, cols=2, qb=32, nh=2, nkv=2, hd=32, out=p + 4096 * 4):
        return lib.rpo_bidir_attn_fwd_f32(ptr, ptr, ptr, stride, stride, stride, cu.data_ptr(), cu.data_ptr(), tl.data_ptr(), 1,
                                          cols, qb, 4, nh, nkv, hd, 0.1, out, 64, None, st)
    assert attn() == OK                                        # the checks below do not refuse everything
    assert attn(hd=128, stride=768) == UNS
    assert attn(hd=16) == UNS
    assert attn(nkv=1) == UNS                                  # grouped heads
    assert attn(tl=tiles3, cols=3) == UNS                      # another table format
    assert attn(qb=64) == UNS
    assert attn(ptr=p + 4) == UNS                              # misaligned q / k / v
    assert attn(out=p + 4096 * 4 + 8) == UNS                   # misaligned out
    assert attn(stride=194) == UNS                             # rows not 16-byte aligned
    ln = lib.rpo_add_layernorm_fwd_f32
    assert ln(p, 64, p, 64, p, p, 1e-5, p + 4096 * 4, 64, 2, 64, st) == OK
    assert ln(p, 12, p, 12, p, p, 1e-5, p, 12, 2, 12, st) == UNS               # d % 8
    assert ln(p, 4104, p, 4104, p, p, 1e-5, p, 4104, 2, 4104, st) == UNS       # d > 4096
    assert ln(p + 4, 64, p, 64, p, p, 1e-5, p, 64, 2, 64, st) == UNS           # misaligned
    assert ln(p, 66, p, 64, p, p, 1e-5, p, 64, 2, 64, st) == UNS               # row stride not 16 bytes
    assert lib.rpo_gelu_fwd_f32(p, 2, 64, 64, st) == OK
    assert lib.rpo_gelu_fwd_f32(p, 2, 12, 12, st) == UNS
    assert lib.rpo_gelu_fwd_f32(p + 4, 2, 64, 64, st) == UNS

    def emb(d=64, y=p + 4096 * 4, ldy=64, word=p):
        return lib.rpo_bert_embed_ln_fwd_f32(ids.data_ptr(), None, ids.data_ptr(), 2, word, 4, p, 1, p, 4, p, p, 1e-5, y, ldy, d, st)
    assert emb() == OK
    assert emb(d=12, ldy=12) == UNS
    assert emb(d=4104, ldy=4104) == UNS
    assert emb(y=p + 4096 * 4 + 4) == UNS
    assert emb(word=p + 8) == UNS
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# end to end: ModelForInference.encode on an f32 encoder
# ------------------------------------------------------------------------------------------------
def _errors(got, ref):
    got, ref = got.double(), ref.double()
    cos = (got * ref).sum(-1) / (got.norm(dim=-1) * ref.norm(dim=-1))
    return float((1 - cos).abs().max()), float((got - ref).abs().max())


def _build(kind, seed, **kw):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from test_gpu_bert_native import _cfg
    from test_gpu_inference import CharTok
    torch.manual_seed(seed)
    cfg = _cfg(PE, kind)
    enc = PE.build_encoder(cfg)
    w32 = E.state_dict_to_f32(enc)
    return PE, cfg, w32, rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), device=0, **kw)


@pytest.fixture(scope="module", params=["bge-small", "xlm-r"])
def f32_case(request):
    """One f32 model per config (switch off), the same weights with packed_f32=True, the texts, the float64 oracle rows (CPU)
    and the padded f32 rows (the control): computed once, shared by the tests below, never modified."""
    from test_gpu_inference import CharTok, _texts
    kind = request.param
    PE, cfg, w32, inf = _build(kind, 31)
    _, _, w32_on, inf_on = _build(kind, 31, packed_f32=True)
    assert all(torch.equal(w32[k], w32_on[k]) for k in w32)
    assert inf.model.embeddings.word_embeddings.weight.dtype == F32 and not inf.model.native_f32 and inf_on.model.native_f32
    rs = np.random.RandomState(4)
    texts = _texts(rs, 21, 20, 300) + ["q"] + _texts(rs, 6, 280, 300)          # 3 batches of 10 / 10 / 8, one 1-token row
    tok = CharTok()(texts, max_length=320)
    w64 = {k: v.double() for k, v in w32.items()}
    with torch.no_grad():
        ref = E.embed(w64, cfg.to_dict(), tok, dtype=torch.float64).detach()
    assert ref.dtype == torch.float64
    padded = inf.encode(texts, batch_size=10, max_length=320)
    return dict(kind=kind, PE=PE, cfg=cfg, inf=inf, inf_on=inf_on, texts=texts, ref=ref, padded=padded)


def _spy():
    from test_gpu_bert_native import Spy
    return Spy()


def test_encode_f32_switch_off_is_the_padded_path(f32_case, monkeypatch):
    c = f32_case
    assert c["PE"].BERT_NATIVE and not c["PE"].BERT_NATIVE_F32 and not c["inf"].model.native_f32
    with _spy() as spy:
        a = c["inf"].encode(c["texts"], batch_size=10, max_length=320)
    n = spy.n
    assert n["bidir_attn_fwd"] == n["add_layernorm"] == n["gelu_"] == n["bert_embed_ln"] == 0 and n["sdpa"] > 0, n
    monkeypatch.setattr(c["PE"], "BERT_NATIVE", False)
    b = c["inf"].encode(c["texts"], batch_size=10, max_length=320)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, c["padded"])
    with torch.no_grad():
        c["inf"].model.eval()
        assert c["inf"].model.native_decline_reason() == "BERT_NATIVE is off"
        monkeypatch.setattr(c["PE"], "BERT_NATIVE", True)
        assert c["inf"].model.native_decline_reason() == "storage dtype"


@pytest.mark.parametrize("switch", ["packed_f32", "BERT_NATIVE_F32"])
def test_encode_f32_packed_path_vs_oracle(f32_case, switch, monkeypatch):
    c = f32_case
    cfg, ref = c["cfg"], c["ref"]
    if switch == "packed_f32":
        inf = c["inf_on"]
    else:
        inf = c["inf"]
        monkeypatch.setattr(c["PE"], "BERT_NATIVE_F32", True)
    with _spy() as spy:
        out = inf.encode(c["texts"], batch_size=10, max_length=320)
    nb, nl = 3, cfg.num_hidden_layers
    n = spy.n
    assert n["bidir_attn_fwd"] == nb * nl and n["add_layernorm"] == 2 * nb * nl and n["gelu_"] == nb * nl, n
    assert n["bert_embed_ln"] == nb and n["sdpa"] == 0 and n["layernorm"] == 0, n
    assert n["syncs"] == 0, "encode() synchronised on a device tensor's contents"
    assert out.dtype == np.float32 and out.shape == (28, cfg.hidden_size) and np.isfinite(out).all()
    f_cos, f_abs = _errors(torch.tensor(out), ref)
    c_cos, c_abs = _errors(torch.tensor(c["padded"]), ref)
    print(f"\nencode f32 {c['kind']} ({switch}): packed cos err {f_cos:.2e} abs {f_abs:.2e}; padded f32 control {c_cos:.2e} / {c_abs:.2e}")
    assert f_abs <= 1.5 * c_abs + ULP2 and f_cos <= 1.5 * c_cos + ULP2 ** 2, (f_cos, c_cos, f_abs, c_abs)


def test_encode_f32_bucket_by_length(f32_case):
    c = f32_case
    kw = dict(batch_size=10, max_length=320)
    out = c["inf_on"].encode(c["texts"], **kw)
    out_b = c["inf_on"].encode(c["texts"], bucket_by_length=True, **kw)
    pad_b = c["inf"].encode(c["texts"], bucket_by_length=True, **kw)
    moved = np.abs(out_b.astype(np.float64) - out.astype(np.float64)).max()
    moved_padded = np.abs(pad_b.astype(np.float64) - c["padded"].astype(np.float64)).max()
    print(f"\nbucket_by_length {c['kind']}: packed rows move {moved:.3e}, padded f32 rows move {moved_padded:.3e}")
    # other batches, so other GEMM shapes: within 4 ulp, or 1.5 x what the same regrouping does to the padded f32 path
    assert moved <= max(2 * ULP2, 1.5 * moved_padded), (moved, moved_padded)


@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_16_bit_model_ignores_the_f32_switch(kind, monkeypatch):
    from test_gpu_inference import _texts
    texts = _texts(np.random.RandomState(8), 7, 5, 60)
    PE, cfg, _, inf = _build(kind, 9, use_fp16=True)
    a = inf.encode(texts, batch_size=4, max_length=64)
    _, _, _, inf_on = _build(kind, 9, use_fp16=True, packed_f32=True)
    monkeypatch.setattr(PE, "BERT_NATIVE_F32", True)
    assert inf_on.model.native_f32 and inf_on.model.embeddings.word_embeddings.weight.dtype == torch.float16
    with _spy() as spy:
        b = inf_on.encode(texts, batch_size=4, max_length=64)
    assert spy.n["bidir_attn_fwd"] == 2 * cfg.num_hidden_layers and spy.n["sdpa"] == 0, spy.n
    assert a.dtype == b.dtype == np.float16
    np.testing.assert_array_equal(a, b)


def test_declined_f32_batches_give_the_padded_rows(f32_case, monkeypatch):
    from test_gpu_bert_native import LeftTok
    from test_gpu_inference import CharTok, _texts
    c = f32_case
    inf, inf_on = c["inf"], c["inf_on"]
    texts = _texts(np.random.RandomState(8), 7, 5, 60)
    # left padding: the CLS column holds pad tokens -> declined with the switch on, the padded path's rows bit for bit
    right = inf_on.tokenizer
    try:
        inf_on.tokenizer = LeftTok()
        with _spy() as spy:
            a = inf_on.encode(texts, batch_size=4, max_length=64)
    finally:
        inf_on.tokenizer = right
    assert spy.n["bidir_attn_fwd"] == 0 and spy.n["sdpa"] > 0, spy.n
    try:
        inf.tokenizer = LeftTok()
        b = inf.encode(texts, batch_size=4, max_length=64)
    finally:
        inf.tokenizer = right
    np.testing.assert_array_equal(a, b)
    # train mode with dropout: pooled_cls declines (encode itself always runs eval mode); the caller's padded forward draws the
    # same masks from the same seed whether the switch is on or off
    tok = CharTok()(texts, max_length=64)

    def rows(m):
        torch.manual_seed(77)
        with torch.no_grad():
            pooled = m.model.pooled_cls(tok["input_ids"], tok["attention_mask"])
            if pooled is not None:
                return pooled, True
            return m.model(input_ids=tok["input_ids"].to(DEV), attention_mask=tok["attention_mask"].to(DEV)).last_hidden_state[:, 0], False
    try:
        inf.model.train()
        inf_on.model.train()
        with torch.no_grad():
            assert inf_on.model.native_decline_reason() == "training with dropout"
        (ra, native_a), (rb, native_b) = rows(inf_on), rows(inf)
        assert not native_a and not native_b and torch.equal(ra, rb)
    finally:
        inf.model.eval()
        inf_on.model.eval()
    got, native = rows(inf_on)
    assert native and got.shape == ra.shape and torch.isfinite(got).all()
