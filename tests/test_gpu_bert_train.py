"""The packed BERT / XLM-R training step (bert_ops.hip backward kernels and dropout, `BertEncoder.pooled_cls_train`,
`ModelForTraining.embed` for CLS-pooled models): every kernel against float64 computed from the exact stored inputs, and the
training step end to end against the float32 oracle, by the repo's control rule (error <= 1.5 x the error of the stock PyTorch
op / path in the same storage dtype + a floor from the storage format).

Errors are Frobenius norms per (sequence, head) block, per row or per tensor, relative to that block's / row's / tensor's own
reference (never to a global maximum).  U = the storage unit roundoff 2^-(mantissa bits + 1).

Attention: ||got - ref|| <= (1.5 c + 2 U) ||ref|| per (sequence, head) block, c = the relative error of torch's SDPA forward +
backward on the same sequence in the same dtype (without dropout: SDPA's own mask cannot be replayed).  The floor 2 U: one
rounding of the stored result plus one of an MFMA operand, as in the attention and encoder-op parity tests.  A sequence with ONE
key is the exception: there dS = P (dP - delta) = 0 exactly, so dq = dk = 0 and ||ref|| = 0, while the kernels subtract two f32 sums
of the same products taken in different orders (and, under dropout, delta is taken from the ROUNDED stored O); for those blocks
only, 2 U ||abs|| is added, ||abs|| being the same expression evaluated with absolute values (the size of what cancels).
Under dropout the control cannot share one effect with the kernels: delta = rowsum(dO o O) is taken from the stored O, which is
rounded AFTER the 1 / (1 - p) scaling and the mask, so delta is off by up to U sum |dO| |O| from the sum P o dP it stands for, and
on short sequences with a peaked softmax dP - delta is much smaller than delta.  For p > 0, dq and dk therefore add U ||abs_delta||:
with e_q = sum |dO| |O| over the head dim of query q (the reference's own O), dq[q] moves by at most scale e_q |(P K)[q]| and dk[k]
by at most scale sum_q P[q, k] e_q |Q[q]|; one rounding, constant 1, of that one channel.
Measured on an MI355X, max err / bound over the blocks, range over the cases of each test, sequences of >= 512 keys ("long") and
shorter ones apart (the tests print them).  Without dropout: out 0.20-0.25 long, 0.19-0.22 short; dq 0.21-0.27 long, 0.35-0.58
short; dk 0.21-0.23 long, 0.35-0.58 short; dv 0.20-0.23 long, 0.22-0.24 short.  With dropout 0.1 / 0.5: out 0.20-0.34 long,
0.20-0.27 short; dq 0.17-0.27 long, 0.15-0.25 short; dk 0.09-0.24 long, 0.09-0.26 short; dv 0.20-0.23 long, 0.22-0.39 short.
LayerNorm / GELU / end to end: relative error <= 1.5 x the control's + 2 U, the denominator of a cancelling quantity extended by
the size of what cancels (stated at each place): one rounding of the stored result plus one of a stored input the backward re-reads
(O, s, u) to the same precision.  Every output buffer is allocated NaN-filled."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bert_parity_util import attn64 as _attn64     # float64 forward + backward of one sequence, with its absn / absd terms
from oracle import encoder_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
TEMP = 0.02
LENS = [1, 2, 31, 32, 33, 100, 512, 777]


def ops():
    from rankpo_amd import ops as o
    return o


def _nan(shape, dtype):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------
# attention backward, with and without dropout
# ------------------------------------------------------------------------------------------------
def _sdpa_ctrl(q, k, v, do, scale):
    """torch's own SDPA forward + backward in the storage dtype, one sequence, no dropout: the control."""
    qs, ks, vs = (t.transpose(0, 1)[None].detach().clone().requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qs, ks, vs, scale=scale)
    o.backward(do.transpose(0, 1)[None])
    return (o[0],) + tuple(t.grad[0] for t in (qs, ks, vs))                      # [nh, l, hd]


def _run_attn_case(dtype, hd, nh, lens_q, lens_k, cls, p, seed, label):
    o = ops()
    gen = torch.Generator(device=DEV).manual_seed(hd * 1000 + nh + len(lens_q) + int(cls))
    d, Tk, Tq = nh * hd, sum(lens_k), sum(lens_q)
    scale = 1.0 / math.sqrt(hd)
    qkv = torch.randn(Tk, 3 * d, generator=gen, device=DEV).to(dtype)           # q|k|v as column blocks of ONE buffer
    dqkv = _nan((Tk, 3 * d), dtype)
    q, k, v = (qkv[:, j * d:(j + 1) * d].view(Tk, nh, hd) for j in range(3))
    dq, dk, dv = (dqkv[:, j * d:(j + 1) * d].view(Tk, nh, hd) for j in range(3))
    cu_k = [0] + np.cumsum(lens_k).tolist()
    cu_q = [0] + np.cumsum(lens_q).tolist()
    if cls:                                                                      # one query per sequence: its first token
        q = q.reshape(Tk, d).index_select(0, torch.tensor(cu_k[:-1], device=DEV)).view(Tq, nh, hd).contiguous()
        dq = _nan((Tq, nh, hd), dtype)
    assert cls or q.stride(0) == 3 * d
    cq = torch.tensor(cu_q, dtype=torch.int32, device=DEV)
    ck = torch.tensor(cu_k, dtype=torch.int32, device=DEV)
    qt = o.bidir_attn_tile_table(lens_q, lens_k, DEV)
    kt = torch.from_numpy(o.bidir_attn_key_tile_list(lens_q, lens_k)).to(DEV)
    out, lse = o.bidir_attn_train_fwd(q, k, v, cq, ck, qt, scale, p, seed)
    if p == 0:
        out0, lse0 = o.bidir_attn_fwd(q, k, v, cq, ck, qt, scale, want_lse=True)
        assert torch.equal(out, out0) and torch.equal(lse, lse0), label         # the training entry without dropout = the forward
    do = torch.randn(Tq, d, generator=gen, device=DEV).to(dtype)
    o.bidir_attn_bwd(q, k, v, out, do, lse, cq, ck, qt, kt, scale, dq, dk, dv, p, seed)
    torch.cuda.synchronize()
    worst = {}                                                # max err / bound, sequences of >= 512 keys and shorter ones apart
    for n in range(len(lens_q)):
        a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
        keep = o.bidir_attn_dropout_mask(a, c, b - a, e - c, nh, p, seed, DEV) if p > 0 else None
        don = do[a:b].view(-1, nh, hd)
        ref, absn, absd = _attn64(q[a:b], k[c:e], v[c:e], don, scale, keep, p)
        ctrl = _sdpa_ctrl(q[a:b], k[c:e], v[c:e], don, scale)
        ref0 = ref if p == 0 else _attn64(q[a:b], k[c:e], v[c:e], don, scale, None, 0.0)[0]
        got = (out[a:b].view(-1, nh, hd), dq[a:b], dk[c:e], dv[c:e])
        for name, g, r, r0, cc, an, ad in zip(("out", "dq", "dk", "dv"), got, ref, ref0, ctrl, (None,) + absn, (None,) + absd):
            g = g.transpose(0, 1)
            assert torch.isfinite(g.float()).all(), (label, n, name)
            fro = lambda t: t.flatten(-2).norm(dim=-1)
            # ||got - ref|| <= (1.5 x the control's relative error + 2 U) ||ref||; a one-key sequence (exact dq = dk = 0: nothing
            # to be relative to) adds 2 U ||abs||; under dropout dq / dk add U ||abs_delta|| (delta from the rounded stored O)
            c_rel = fro(cc.double() - r0) / fro(r0).clamp_min(1e-300)
            err = fro(g.double() - r)
            bound = (1.5 * c_rel + 2 * U[dtype]) * fro(r)
            if e - c == 1 and an is not None:
                bound = bound + 2 * U[dtype] * fro(an)
            elif p > 0 and ad is not None:
                bound = bound + U[dtype] * fro(ad)
            wk = name + (" long" if e - c >= 512 else " short")
            worst[wk] = max(worst.get(wk, 0.0), round(float((err / bound.clamp_min(1e-300)).max().detach()), 3))
            assert (err <= bound).all(), (label, "seq", n, "lens", b - a, e - c, name, err.tolist(), bound.tolist())
    print(f"\n{label}: max err / bound {worst}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,nh", [(32, 4), (64, 3)])
def test_bidir_attn_bwd_matches_f64(dtype, hd, nh):
    _run_attn_case(dtype, hd, nh, LENS, LENS, False, 0.0, 0, f"self hd{hd} {dtype}")
    _run_attn_case(dtype, hd, nh, [1] * len(LENS), LENS, True, 0.0, 0, f"cls hd{hd} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("hd,nh", [(32, 4), (64, 3)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_bidir_attn_dropout_fwd_bwd_match_f64_with_dumped_mask(dtype, hd, nh, p):
    """Forward, dQ kernel, dK/dV kernel and the dump agree on the mask: a disagreement is an O(1) error."""
    seed = 0x1234567887654321 + int(p * 10)
    _run_attn_case(dtype, hd, nh, LENS, LENS, False, p, seed, f"self p{p} hd{hd} {dtype}")
    _run_attn_case(dtype, hd, nh, [1] * len(LENS), LENS, True, p, seed, f"cls p{p} hd{hd} {dtype}")


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_properties(p):
    o = ops()
    nh, lq, lk = 2, 64, 16384                                  # 2.1e6 elements; rows of 16384
    seed = 987654321987
    m = o.bidir_attn_dropout_mask(1000, 3, lq, lk, nh, p, seed, DEV)
    assert m.dtype == torch.uint8 and m.shape == (nh, lq, lk) and int(m.max()) == 1 and int(m.min()) == 0
    mf = m.double()
    sig = lambda n: math.sqrt(p * (1 - p) / n)
    assert ((mf.mean((1, 2)) - (1 - p)).abs() <= 4 * sig(lq * lk)).all(), mf.mean((1, 2))
    assert ((mf.mean(2) - (1 - p)).abs() <= 4 * sig(lk)).all()                 # per row
    assert torch.equal(m, o.bidir_attn_dropout_mask(1000, 3, lq, lk, nh, p, seed, DEV))   # same seed, same mask
    f = 2 * p * (1 - p)
    tol = 4 * math.sqrt(f * (1 - f) / (lq * lk))
    other_layer = o.bidir_attn_dropout_mask(1000, 3, lq, lk, nh, p, o.bert_layer_seed(seed, 1), DEV)
    other_seed = o.bidir_attn_dropout_mask(1000, 3, lq, lk, nh, p, seed + 1, DEV)
    for name, a, b in (("heads", m[0], m[1]), ("layers", m[0], other_layer[0]), ("seeds", m[0], other_seed[0])):
        diff = (a != b).double().mean().item()
        assert abs(diff - f) <= tol, (name, diff, f, tol)
    # one head / one row of a dump = the same entries of the whole dump
    assert torch.equal(o.bidir_attn_dropout_mask(1000 + 5, 3, 1, lk, 1, p, seed, DEV, head0=1)[0, 0], m[1, 5])


# ------------------------------------------------------------------------------------------------
# LayerNorm / GELU backward
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [128, 384, 768, 1024, 4096])
def test_layernorm_train_fwd_and_bwd_match_f64(dtype, d):
    o = ops()
    from rankpo_amd import _lib
    lib = _lib.load()
    eps = 1e-12
    floor = 2 * U[dtype]
    for rows in (1, 63, 64, 65, 8192):
        gen = torch.Generator(device=DEV).manual_seed(d + rows)
        a = (torch.randn(rows, d, generator=gen, device=DEV) * 2).to(dtype)
        b = torch.randn(rows, 2 * d, generator=gen, device=DEV).to(dtype)[:, :d]          # row-strided dense output
        g = (1 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
        be = (0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype)
        dy = torch.randn(rows, d, generator=gen, device=DEV).to(dtype)
        # the training forward: y bit for bit the forward's, s = the rounded sum
        y, s = _nan((rows, d), dtype), _nan((rows, d), dtype)
        st = torch.cuda.current_stream().cuda_stream
        assert lib.rpo_add_layernorm_train_fwd(a.data_ptr(), d, b.data_ptr(), 2 * d, g.data_ptr(), be.data_ptr(), eps, y.data_ptr(),
                                               d, s.data_ptr(), d, rows, d, o._dt(a), st) == 0
        assert torch.equal(y, o.add_layernorm(a, b, g, be, eps)) and torch.equal(s, a + b)
        ds, dg, db = o.layernorm_bwd(s, g, dy, eps)
        assert torch.isfinite(ds.float()).all() and torch.isfinite(dg).all() and torch.isfinite(db).all()
        s64 = s.double().requires_grad_(True)
        g64, b64 = g.double().requires_grad_(True), be.double().requires_grad_(True)
        F.layer_norm(s64, (d,), g64, b64, eps).backward(dy.double())
        sc = s.clone().requires_grad_(True)
        gc, bc = g.clone().requires_grad_(True), be.clone().requires_grad_(True)
        F.layer_norm(sc, (d,), gc, bc, eps).backward(dy)
        err = (ds.double() - s64.grad).norm(dim=-1) / s64.grad.norm(dim=-1)
        c_err = (sc.grad.double() - s64.grad).norm(dim=-1) / s64.grad.norm(dim=-1)
        assert (err <= 1.5 * c_err + floor).all(), ("ds", rows, d, float((err - 1.5 * c_err).max()), floor)
        for name, got, ctrl, ref in (("dgamma", dg, gc.grad, g64.grad), ("dbeta", db, bc.grad, b64.grad)):
            e1 = float((got.double() - ref).norm() / ref.norm())
            e2 = float((ctrl.double() - ref).norm() / ref.norm())
            assert e1 <= 1.5 * e2 + floor, (name, rows, d, e1, e2, floor)


def test_layernorm_autograd_function_and_embedding_scatter():
    """`add_layernorm_train` (b None and not None) and `bert_embed_ln_train` under torch.autograd against float64."""
    o = ops()
    dtype, d, rows = torch.float16, 256, 50
    gen = torch.Generator(device=DEV).manual_seed(3)
    mk = lambda *sh, m=1.0: (torch.randn(*sh, generator=gen, device=DEV) * m).to(dtype).requires_grad_(True)
    a, b, g, be = mk(rows, d), mk(rows, d), mk(d), mk(d, m=0.1)
    dy = torch.randn(rows, d, generator=gen, device=DEV).to(dtype)
    o.add_layernorm_train(a, b, g, be, 1e-5).backward(dy)
    s64 = (a + b).detach().double().requires_grad_(True)
    g64, b64 = g.detach().double().requires_grad_(True), be.detach().double().requires_grad_(True)
    F.layer_norm(s64, (d,), g64, b64, 1e-5).backward(dy.double())
    tol = 4 * U[dtype]
    assert torch.equal(a.grad, b.grad)
    for got, ref in ((a.grad, s64.grad), (g.grad, g64.grad), (be.grad, b64.grad)):
        assert float((got.double() - ref).norm() / ref.norm()) < tol
    V, P, TT, T = 40, 30, 2, 200                                # few rows: many tokens add into each table row
    word, pe, te, g, be = mk(V, d), mk(P, d), mk(TT, d), mk(d), mk(d, m=0.1)
    ids = torch.randint(0, V, (T,), generator=gen, device=DEV, dtype=torch.int32)
    pos = torch.randint(0, P, (T,), generator=gen, device=DEV, dtype=torch.int32)
    for tts in (torch.randint(0, TT, (T,), generator=gen, device=DEV, dtype=torch.int32), None):
        for t in (word, pe, te, g, be):
            t.grad = None
        dy = torch.randn(T, d, generator=gen, device=DEV).to(dtype)
        y = o.bert_embed_ln_train(ids, pos, tts, word, te, pe, g, be, 1e-5, 7)
        assert torch.equal(y, o.bert_embed_ln(ids, pos, tts, word, te, pe, g, be, 1e-5))
        y.backward(dy)
        w64, p64, t64, g64, b64 = (t.detach().double().requires_grad_(True) for t in (word, pe, te, g, be))
        w_pad = torch.nn.functional.embedding(ids.long(), w64, padding_idx=7)
        t_rows = t64[tts.long()] if tts is not None else t64[0].expand(T, d)
        s = ((w_pad + t_rows).to(dtype).double() - (w_pad + t_rows)).detach() + (w_pad + t_rows)      # the forward's roundings
        s = ((s + p64[pos.long()]).to(dtype).double() - (s + p64[pos.long()])).detach() + (s + p64[pos.long()])
        F.layer_norm(s, (d,), g64, b64, 1e-5).backward(dy.double())
        assert float(word.grad[7].abs().max()) == 0.0           # padding_idx keeps its zero gradient
        for name, got, ref in (("word", word.grad, w64.grad), ("pos", pe.grad, p64.grad), ("type", te.grad, t64.grad),
                               ("gamma", g.grad, g64.grad), ("beta", be.grad, b64.grad)):
            assert float((got.double() - ref).norm() / ref.norm()) < tol, (name, tts is None)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gelu_out_and_bwd_match_f64(dtype):
    o = ops()
    gen = torch.Generator(device=DEV).manual_seed(5)
    rows, cols = 65, 1536
    big = (torch.randn(rows, 2 * cols, generator=gen, device=DEV) * 3).to(dtype)
    u = big[:, :cols]                                          # row-strided
    u[0, :64] = torch.linspace(-9, 9, 64, device=DEV).to(dtype)   # both tails
    dh = torch.randn(rows, cols, generator=gen, device=DEV).to(dtype)
    keep = u.clone()
    h = o.gelu_out(u)
    assert torch.equal(u, keep) and torch.equal(h, o.gelu_(u.clone().contiguous()))
    du = o.gelu_bwd(u, dh)
    assert torch.isfinite(du.float()).all()
    u64, dh64 = u.double(), dh.double()
    cdf = 0.5 * torch.erfc(-u64 / math.sqrt(2))
    pdf = torch.exp(-0.5 * u64 * u64) / math.sqrt(2 * math.pi)
    ref = dh64 * (cdf + u64 * pdf)
    uc = u.clone().requires_grad_(True)
    F.gelu(uc).backward(dh)
    # per element; Phi + u phi cancels for u < 0: the floor is relative to |dh| (Phi + |u| phi), the size of what cancels
    floor = 2 * U[dtype] * dh64.abs() * (cdf + u64.abs() * pdf)
    err, c_err = (du.double() - ref).abs(), (uc.grad.double() - ref).abs()
    bad = err > 1.5 * c_err + floor
    assert not bad.any(), (int(bad.sum()), float((err - 1.5 * c_err - floor).max()))
    # the autograd function
    ua = u.clone().requires_grad_(True)
    o.gelu(ua).backward(dh)
    assert torch.equal(ua.grad, du)


def test_training_entries_reject_f32_and_bad_shapes():
    from rankpo_amd import _lib
    lib = _lib.load()
    UNS, INV = -2, -1
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(4096 * 8, dtype=torch.float16, device=DEV)
    xf = torch.zeros(4096 * 8, dtype=torch.float32, device=DEV)
    cu = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    tiles = torch.zeros(1, 2, dtype=torch.int32, device=DEV)
    p, pf, c, t = x.data_ptr(), xf.data_ptr(), cu.data_ptr(), tiles.data_ptr()

    def fwd(ptr=p, hd=32, dt=2, pd=0.1, stride=192):
        return lib.rpo_bidir_attn_train_fwd(ptr, ptr, ptr, stride, stride, stride, c, c, t, 1, 2, 32, 4, 2, 2, hd, dt, 0.1, pd, 5, ptr,
                                            64, pf, st)

    def bwd(ptr=p, hd=32, dt=2, pd=0.1, stride=192, nkv=2):
        return lib.rpo_bidir_attn_bwd(ptr, ptr, ptr, stride, stride, stride, ptr, 64, ptr, 64, pf, c, c, t, 1, t, 1, 2, 32, 4, 2, nkv,
                                      hd, dt, 0.1, pd, 5, ptr, stride, ptr, stride, ptr, stride, st)
    assert fwd(ptr=pf, dt=0) == UNS and bwd(ptr=pf, dt=0) == UNS
    assert fwd(hd=128, stride=768) == UNS and bwd(hd=16) == UNS and bwd(nkv=1) == UNS
    assert fwd(pd=1.0) == INV and bwd(pd=-0.1) == INV
    assert lib.rpo_layernorm_bwd(pf, 64, pf, pf, 64, 1e-5, pf, 64, pf, pf, 2, 64, 0, st) == UNS
    assert lib.rpo_layernorm_bwd(p, 12, p, p, 12, 1e-5, p, 12, pf, pf, 2, 12, 2, st) == UNS
    assert lib.rpo_add_layernorm_train_fwd(pf, 64, pf, 64, pf, pf, 1e-5, pf, 64, pf, 64, 2, 64, 0, st) == UNS
    assert lib.rpo_gelu_out_fwd(pf, 64, pf, 64, 2, 64, 0, st) == UNS and lib.rpo_gelu_bwd(pf, 64, pf, 64, pf, 64, 2, 64, 0, st) == UNS
    assert lib.rpo_gelu_bwd(p, 12, p, 12, p, 12, 2, 12, 2, st) == UNS
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib.rpo_bert_embed_ln_train_fwd(ids.data_ptr(), None, ids.data_ptr(), 2, pf, 4, pf, 1, pf, 4, pf, pf, 1e-5, pf, 64, pf, 64,
                                           64, 0, st) == UNS
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# end to end: ModelForTraining
# ------------------------------------------------------------------------------------------------
def _cfg(PE, kind, p_drop):
    if kind == "bge-small":          # head_dim 32, BERT positions
        return PE.bge_small_config(vocab_size=1024, hidden_size=128, intermediate_size=512, num_hidden_layers=3,
                                   num_attention_heads=4, hidden_dropout_prob=p_drop, attention_probs_dropout_prob=p_drop)
    return PE.xlm_roberta_config(vocab_size=1024, hidden_size=256, intermediate_size=1024, num_hidden_layers=2,   # head_dim 64
                                 num_attention_heads=4, max_position_embeddings=514, hidden_dropout_prob=p_drop,
                                 attention_probs_dropout_prob=p_drop)


def _batch(rs, cfg, B=4, G=3, Lq=40, Lp=96):
    """Ragged right-padded towers, each with a length-1 row and a full-length row."""
    pad = cfg.pad_token_id

    def side(N, L):
        lens = rs.randint(2, L, size=N)
        lens[0], lens[1] = L, 1
        m = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        ids = rs.randint(pad + 1, cfg.vocab_size, size=(N, L)) * m + pad * (1 - m)
        return {"input_ids": torch.tensor(ids), "attention_mask": torch.tensor(m)}
    return {"query": side(B, Lq), "passage": side(B * G, Lp)}


class TrainSpy:
    def __init__(self):
        self.n = {"bidir_attn_bwd": 0, "sdpa": 0}

    def __enter__(self):
        o = ops()
        self._bwd, self._sdpa = o.bidir_attn_bwd, F.scaled_dot_product_attention

        def bwd(*a, **kw):
            self.n["bidir_attn_bwd"] += 1
            return self._bwd(*a, **kw)

        def sdpa(*a, **kw):
            self.n["sdpa"] += 1
            return self._sdpa(*a, **kw)
        o.bidir_attn_bwd, F.scaled_dot_product_attention = bwd, sdpa
        return self

    def __exit__(self, *exc):
        ops().bidir_attn_bwd, F.scaled_dot_product_attention = self._bwd, self._sdpa
        return False


LOSS_SCALE = 256.0      # fp16 needs it (the reference's fp16 BGE run scales its loss); the same factor for every arm and dtype


def _step(model, gb):
    """One forward + backward -> (loss, scores, {name: unscaled float64 gradient})."""
    model.zero_grad(set_to_none=True)
    out = model(**gb)
    (out.loss * LOSS_SCALE).backward()
    grads = {k: v.grad.double().cpu() / LOSS_SCALE for k, v in model.model.named_parameters()}
    return out.loss.detach().double().cpu(), out.scores.detach().double().cpu(), grads


def _tensor_errors(grads, ref, dtype):
    """Relative Frobenius error per parameter.  The key bias has no gradient (softmax is invariant to it): its exact gradient is a
    sum that cancels to zero, of the magnitude of the query bias gradient of the same block, which stands in the denominator."""
    errs = {}
    for k, r in ref.items():
        den = r.norm()
        if k.endswith("attention.self.key.bias"):
            den = den + ref[k.replace(".key.", ".query.")].norm()
        errs[k] = float((grads[k] - r).norm() / den)
    return errs


def _make(kind, dtype, p_drop, seed):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    torch.manual_seed(seed)
    cfg = _cfg(PE, kind, p_drop)
    enc = PE.build_encoder(cfg)
    # LayerNorm parameters and biases off their initial 1 / 0, so that every parameter's gradient is exercised
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias") or "LayerNorm" in n:
                p.add_(0.05 * torch.randn_like(p))
    w32 = E.state_dict_to_f32(enc)
    model = rankpo_amd.ModelForTraining(encoder=enc.to(DEV).to(dtype), temperature=TEMP).train()
    return PE, cfg, w32, model


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_training_step_vs_oracle_and_padded_path(kind, dtype, monkeypatch):
    PE, cfg, w32, model = _make(kind, dtype, 0.0, 17)
    batch = _batch(np.random.RandomState(3), cfg)
    gb = {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in batch.items()}
    for v in w32.values():
        v.requires_grad_(True)
    ref_loss, ref_s, _, _ = E.contrastive_step(w32, cfg.to_dict(), batch, TEMP)
    ref_loss.backward()
    names = [k for k, _ in model.model.named_parameters()]
    ref_g = {k: w32[k].grad.double() for k in names}
    with TrainSpy() as spy:
        loss, s, g = _step(model, gb)
    assert spy.n["bidir_attn_bwd"] == 2 * cfg.num_hidden_layers and spy.n["sdpa"] == 0, spy.n     # once per block and tower
    monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", False)
    with TrainSpy() as spy0:
        loss0, s0, g0 = _step(model, gb)
    monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", True)
    assert spy0.n["bidir_attn_bwd"] == 0 and spy0.n["sdpa"] > 0, spy0.n
    floor = 2 * U[dtype]
    ref_s64 = ref_s.detach().double()
    e_s, e_s0 = float((s - ref_s64).norm() / ref_s64.norm()), float((s0 - ref_s64).norm() / ref_s64.norm())
    e_l, e_l0 = abs(float(loss - ref_loss.detach())), abs(float(loss0 - ref_loss.detach()))
    print(f"\n{kind} {dtype}: scores native {e_s:.2e} padded {e_s0:.2e}; loss native {e_l:.2e} padded {e_l0:.2e}")
    assert e_s <= 1.5 * e_s0 + floor, (e_s, e_s0)
    # the loss (f32, from the stored unit rows) to the same relative floor
    assert e_l <= 1.5 * e_l0 + floor * abs(float(ref_loss)), (e_l, e_l0)
    en, ep = _tensor_errors(g, ref_g, dtype), _tensor_errors(g0, ref_g, dtype)
    worst = max(names, key=lambda k: en[k] - 1.5 * ep[k])
    print(f"worst parameter {worst}: native {en[worst]:.2e} padded {ep[worst]:.2e}; floor {floor:.2e}")
    bad = {k: (en[k], ep[k]) for k in names if not en[k] <= 1.5 * ep[k] + floor}
    assert not bad, bad


@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_training_declines_fall_back_to_the_padded_path_bit_for_bit(kind, monkeypatch):
    PE, cfg, w32, model = _make(kind, torch.float16, 0.0, 19)
    batch = _batch(np.random.RandomState(5), cfg)

    def both(gb):
        with TrainSpy() as spy:
            la, sa, ga = _step(model, gb)
        monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", False)
        lb, sb, gb_ = _step(model, gb)
        lb2, sb2, gb2 = _step(model, gb)
        monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", True)
        assert spy.n["sdpa"] > 0 and spy.n["bidir_attn_bwd"] == 0, spy.n
        assert torch.equal(la, lb) and torch.equal(sa, sb)
        # gradients: bit for bit wherever the padded path reproduces itself bit for bit (its embedding and attention backward
        # may add in an order that is not fixed); elsewhere as close as two runs of the padded path are to each other
        for k in ga:
            if torch.equal(gb_[k], gb2[k]):
                assert torch.equal(ga[k], gb_[k]), k
            else:
                assert float((ga[k] - gb_[k]).norm()) <= 2 * float((gb2[k] - gb_[k]).norm()), k

    def dev(bt):
        return {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in bt.items()}
    holed = {k: {kk: vv.clone() for kk, vv in v.items()} for k, v in batch.items()}
    holed["query"]["attention_mask"][0, 2] = 0                # a hole in the full-length row of each tower
    holed["passage"]["attention_mask"][0, 2] = 0
    both(dev(holed))
    nocls = {k: {kk: vv.clone() for kk, vv in v.items()} for k, v in batch.items()}
    nocls["query"]["attention_mask"][0, 0] = 0                # a masked CLS column
    nocls["passage"]["attention_mask"][0, 0] = 0
    both(dev(nocls))
    model.gradient_checkpointing_enable()
    both(dev(batch))


def _replay_tower(w, cfg, pk, hmasks, amasks, p_h, p_a, dtype):
    """The packed training forward of one tower in plain torch (autograd through `w`), with the recorded dropout masks."""
    W = lambda k: w[k].to(dtype)
    d, nh, eps = cfg.hidden_size, cfg.num_attention_heads, cfg.layer_norm_eps
    hd, L = d // nh, cfg.num_hidden_layers
    cu = [0] + np.cumsum(pk["lens"]).tolist()
    hm = iter(hmasks)
    drop = lambda t: t * next(hm).to(t.dtype) / (1 - p_h)
    x = (W("embeddings.word_embeddings.weight")[pk["ids"]] + W("embeddings.token_type_embeddings.weight")[0]) \
        + W("embeddings.position_embeddings.weight")[pk["pos"]]
    x = drop(F.layer_norm(x, (d,), W("embeddings.LayerNorm.weight"), W("embeddings.LayerNorm.bias"), eps))
    cls = torch.tensor(cu[:-1], device=x.device)
    for i in range(L):
        p = f"encoder.layer.{i}."
        lin = lambda name, t: F.linear(t, W(p + name + ".weight"), W(p + name + ".bias"))
        last = i == L - 1
        res = x.index_select(0, cls) if last else x
        q, k, v = lin("attention.self.query", res), lin("attention.self.key", x), lin("attention.self.value", x)
        outs = []
        for n in range(len(pk["lens"])):
            ks, vs = (t[cu[n]:cu[n + 1]].view(-1, nh, hd).transpose(0, 1) for t in (k, v))
            qs = (q[n:n + 1] if last else q[cu[n]:cu[n + 1]]).view(-1, nh, hd).transpose(0, 1)
            P = torch.softmax((qs @ ks.transpose(1, 2)).float() / math.sqrt(hd), -1).to(dtype)
            P = P * amasks[i][n].to(dtype) / (1 - p_a)
            outs.append((P @ vs).transpose(0, 1).reshape(-1, d))
        o = torch.cat(outs)
        x = F.layer_norm(drop(lin("attention.output.dense", o)) + res, (d,), W(p + "attention.output.LayerNorm.weight"),
                         W(p + "attention.output.LayerNorm.bias"), eps)
        h = F.gelu(lin("intermediate.dense", x))
        x = F.layer_norm(drop(lin("output.dense", h)) + x, (d,), W(p + "output.LayerNorm.weight"),
                         W(p + "output.LayerNorm.bias"), eps)
    return x


def _replay_step(w, cfg, towers, p_h, p_a, dtype):
    """-> (loss, scores).  float32: plain torch.  Storage dtype (the control): the pooled rows of the torch encoder through the
    product's own scoring tail (HIP normalise + InfoNCE), so that the two arms differ in the encoder alone."""
    q, p = (_replay_tower(w, cfg, t["pk"], t["hmasks"], t["amasks"], p_h, p_a, dtype) for t in towers)
    if dtype != torch.float32:
        o = ops()
        q, p = (o.pool_normalize(t[:, None, :], None, "cls", True) for t in (q, p))
        return o.infonce_loss(q, p, TEMP)
    q, p = F.normalize(q, dim=-1), F.normalize(p, dim=-1)
    G = p.shape[0] // q.shape[0]
    s = q @ p.T / TEMP
    t = torch.arange(q.shape[0], device=s.device) * G
    return F.cross_entropy(s, t), s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_training_step_with_dropout_vs_replay(kind, dtype, monkeypatch):
    p_drop = 0.1
    PE, cfg, w32, model = _make(kind, dtype, p_drop, 23)
    enc = model.model
    batch = _batch(np.random.RandomState(7), cfg)
    gb = {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in batch.items()}
    o = ops()
    towers = []
    real_drop, real_train = PE._hidden_dropout, enc.pooled_cls_train

    def rec_drop(x, p):
        y = real_drop(x, p)
        towers[-1]["hmasks"].append((y != 0).detach())
        return y

    def rec_train(ids, mask, tts=None):
        towers.append({"hmasks": []})
        out = real_train(ids, mask, tts)
        towers[-1]["seed"] = enc.last_dropout_seed
        ids_p, pos_p, _, lens = PE.bert_pack(ids.cpu(), mask.cpu(), None, roberta=enc.embeddings.roberta_positions,
                                             pad_id=enc.embeddings.pad_id)
        towers[-1]["pk"] = {"ids": ids_p.to(DEV), "pos": pos_p.to(DEV), "lens": lens}
        return out
    monkeypatch.setattr(PE, "_hidden_dropout", rec_drop)
    monkeypatch.setattr(enc, "pooled_cls_train", rec_train)

    def run(seed):
        del towers[:]
        torch.manual_seed(seed)
        with TrainSpy() as spy:
            res = _step(model, gb)
        assert spy.n["bidir_attn_bwd"] == 2 * cfg.num_hidden_layers and spy.n["sdpa"] == 0, spy.n
        return res
    loss, s, g = run(101)
    assert len(towers) == 2 and all(len(t["hmasks"]) == 1 + 2 * cfg.num_hidden_layers for t in towers)
    nh, L = cfg.num_attention_heads, cfg.num_hidden_layers
    for t in towers:                                          # the attention masks of every block, from the dump
        cu = [0] + np.cumsum(t["pk"]["lens"]).tolist()
        t["amasks"] = [[o.bidir_attn_dropout_mask(n if i == L - 1 else cu[n], cu[n], 1 if i == L - 1 else cu[n + 1] - cu[n],
                                                  cu[n + 1] - cu[n], nh, p_drop, o.bert_layer_seed(t["seed"], i), DEV)
                        for n in range(len(t["pk"]["lens"]))] for i in range(L)]
    names = [k for k, _ in enc.named_parameters()]

    def replay(dtype_r):
        w = {k: (w32[k].to(DEV) if dtype_r == torch.float32 else w32[k].to(DEV).to(dtype_r)).requires_grad_(True) for k in names}
        l, sc = _replay_step(w, cfg, towers, p_drop, p_drop, dtype_r)
        (l * LOSS_SCALE).backward()
        return l.detach().double().cpu(), sc.detach().double().cpu(), {k: w[k].grad.double().cpu() / LOSS_SCALE for k in names}
    # the float32 replay runs on the storage dtype's weights (what the model holds), upcast
    w32 = {k: v.detach().float().cpu() for k, v in enc.state_dict().items()}
    r_loss, r_s, r_g = replay(torch.float32)
    c_loss, c_s, c_g = replay(dtype)
    floor = 2 * U[dtype]
    e_l, e_l0 = abs(float(loss - r_loss)), abs(float(c_loss - r_loss))
    e_s, e_s0 = float((s - r_s).norm() / r_s.norm()), float((c_s - r_s).norm() / r_s.norm())
    en, ep = _tensor_errors(g, r_g, dtype), _tensor_errors(c_g, r_g, dtype)
    worst = max(names, key=lambda k: en[k] - 1.5 * ep[k])
    print(f"\n{kind} {dtype} dropout: loss native {e_l:.2e} replay-in-dtype {e_l0:.2e}; scores {e_s:.2e} vs {e_s0:.2e}; "
          f"worst parameter {worst}: {en[worst]:.2e} vs {ep[worst]:.2e}; floor {floor:.2e}")
    assert e_s <= 1.5 * e_s0 + floor, (e_s, e_s0)
    assert e_l <= 1.5 * e_l0 + floor * abs(float(r_loss)), (e_l, e_l0)
    bad = {k: (en[k], ep[k]) for k in names if not en[k] <= 1.5 * ep[k] + floor}
    assert not bad, bad
    # the same torch seed: the same step, bit for bit, except the embedding tables (index_add_ is atomic-based)
    loss2, s2, g2 = run(101)
    assert torch.equal(loss, loss2) and torch.equal(s, s2)
    for k in names:
        if "embeddings" in k and "LayerNorm" not in k:
            assert float((g[k] - g2[k]).norm()) <= 1e-3 * float(g[k].norm()), k
        else:
            assert torch.equal(g[k], g2[k]), k
    loss3, _, _ = run(202)
    assert not torch.equal(loss, loss3)
