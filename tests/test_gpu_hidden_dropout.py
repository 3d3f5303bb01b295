"""The hidden dropout fused into the row kernels of the packed BERT / XLM-R training step (bert_ops.hip: rpo_add_layernorm_drop_fwd,
rpo_bert_embed_ln_drop_fwd, rpo_layernorm_drop_bwd, rpo_hidden_dropout_mask).

Everything here is bit for bit.  The dump is compared with the numpy restatement of the keep function
(tests/hidden_dropout_util.py).  The fused kernels are compared with the UNFUSED ops fed through a test-side stand-in for the
dropout pass, `(x.float() * scale).to(dtype) * mask` forward and the same on the gradient backward, with the dumped mask and
`ops.hidden_dropout_scale`: the fused kernels round where a separate pass rounds, so nothing but equality is expected.
Shapes: d = 64 (one vector per lane, lanes 8.. masked off), 384 (BGE-small), 1024 (two vectors per lane); rows 1, 5, 37 (not
multiples of the 4 waves of a block, more than one block); dense outputs row-strided."""
import numpy as np
import pytest
import torch

import hidden_dropout_util as HU

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16]
DIMS = [64, 384, 1024]
ROWS = [1, 5, 37]
EPS = 1e-12


def ops():
    from rankpo_amd import ops as o
    return o


class StandIn(torch.autograd.Function):
    """A separate dropout pass with a given mask: one rounding after the scaling, forward and backward."""

    @staticmethod
    def forward(ctx, x, mask, scale):
        ctx.save_for_backward(mask)
        ctx.scale = scale
        return (x.float() * scale).to(x.dtype) * mask.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return (g.float() * ctx.scale).to(g.dtype) * mask.to(g.dtype), None, None


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_mask_dump_equals_the_numpy_restatement(p):
    o = ops()
    for seed in HU.SEEDS[:2]:
        hs = o.bert_hidden_seed(seed)
        for d in DIMS:
            for rows in ROWS:
                for row0, site in ((0, 0), (1000003, 1), (77, 6)):
                    got = o.hidden_dropout_mask(row0, rows, d, p, hs, site, DEV)
                    assert got.dtype == torch.uint8 and got.shape == (rows, d)
                    ref = HU.hidden_keep(hs, site, row0, rows, d, p)
                    assert np.array_equal(got.cpu().numpy(), ref), (seed, d, rows, row0, site)
    # p below 2^-17 quantises to no dropout; the last representable row
    assert int(o.hidden_dropout_mask(0, 5, 64, 1e-6, 3, 0, DEV).min()) == 1
    top = 2 ** 31 - 1 - 3
    assert np.array_equal(o.hidden_dropout_mask(top, 3, 64, p, 3, 2, DEV).cpu().numpy(), HU.hidden_keep(3, 2, top, 3, 64, p))


def _ln_case(dtype, d, rows, seed=0):
    gen = torch.Generator(device=DEV).manual_seed(1000 * d + rows + seed)
    a = (torch.randn(rows, d, generator=gen, device=DEV) * 2).to(dtype).requires_grad_(True)
    big = torch.randn(rows, 2 * d, generator=gen, device=DEV).to(dtype).requires_grad_(True)     # b: a row-strided dense output
    g = (1 + 0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype).requires_grad_(True)
    be = (0.1 * torch.randn(d, generator=gen, device=DEV)).to(dtype).requires_grad_(True)
    dy = torch.randn(rows, d, generator=gen, device=DEV).to(dtype)
    return a, big, g, be, dy


def _grads(y, dy, *ts):
    for t in ts:
        t.grad = None
    y.backward(dy)
    return [t.grad.clone() for t in ts]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_fused_add_layernorm_equals_the_unfused_op_through_the_stand_in(dtype, p):
    o = ops()
    hs = o.bert_hidden_seed(HU.SEEDS[0])
    scale = o.hidden_dropout_scale(p)
    assert scale == HU.scale(p)
    for d in DIMS:
        for rows in ROWS:
            for site in (1, 4):
                a, big, g, be, dy = _ln_case(dtype, d, rows)
                d_ = d
                b = big[:, :d_]
                mask = o.hidden_dropout_mask(0, rows, d, p, hs, site, DEV)
                y1 = o.add_layernorm_train(a, b, g, be, EPS, p, hs, site)
                y0 = o.add_layernorm_train(a, StandIn.apply(b, mask, scale), g, be, EPS)
                label = (dtype, p, d, rows, site)
                assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0), label
                # the stored sum s of both forwards (saved for the backward)
                s1, s0 = y1.grad_fn.saved_tensors[0], y0.grad_fn.saved_tensors[0]
                assert torch.equal(s1, s0) and torch.equal(s0, a.detach() + StandIn.apply(b.detach(), mask, scale)), label
                g1 = _grads(y1, dy, a, big, g, be)
                g0 = _grads(y0, dy, a, big, g, be)
                for name, x1, x0 in zip(("ds", "db", "dgamma", "dbeta"), g1, g0):
                    assert torch.isfinite(x1.float()).all() and torch.equal(x1, x0), (name,) + label
                assert not torch.equal(g1[0], g1[1][:, :d])                  # db is the dropped ds, not ds
                assert float(g1[1][:, d:].abs().max()) == 0.0               # the columns beside b receive nothing
                # a dropped element of b contributes nothing: s = a there
                dropped = mask == 0
                assert torch.equal(s1[dropped], a.detach()[dropped]), label


@pytest.mark.parametrize("dtype", DTYPES)
def test_fused_embedding_site_equals_the_unfused_op_through_the_stand_in(dtype):
    o = ops()
    p, pad = 0.1, 7
    hs = o.bert_hidden_seed(HU.SEEDS[1])
    scale = o.hidden_dropout_scale(p)
    for d in DIMS:
        for T in (1, 37):
            gen = torch.Generator(device=DEV).manual_seed(d + T)
            mk = lambda *sh, m=1.0: (torch.randn(*sh, generator=gen, device=DEV) * m).to(dtype).requires_grad_(True)
            V, P, TT = 40, 30, 2
            word, pe, te, g, be = mk(V, d), mk(P, d), mk(TT, d), mk(d), mk(d, m=0.1)
            with torch.no_grad():
                word[pad].zero_()
            ids = torch.randint(0, V, (T,), generator=gen, device=DEV, dtype=torch.int32)
            ids[::3] = pad                                                  # ids that hit the padding row
            pos = torch.randint(0, P, (T,), generator=gen, device=DEV, dtype=torch.int32)
            dy = torch.randn(T, d, generator=gen, device=DEV).to(dtype)
            mask = o.hidden_dropout_mask(0, T, d, p, hs, 0, DEV)
            for tts in (torch.randint(0, TT, (T,), generator=gen, device=DEV, dtype=torch.int32), None):
                label = (dtype, d, T, tts is None)
                y1 = o.bert_embed_ln_train(ids, pos, tts, word, te, pe, g, be, EPS, pad, p, hs)
                plain = o.bert_embed_ln_train(ids, pos, tts, word, te, pe, g, be, EPS, pad)
                y0 = StandIn.apply(plain, mask, scale)
                assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0), label
                assert torch.equal(y1.grad_fn.saved_tensors[0], plain.grad_fn.saved_tensors[0]), label      # the stored sum s
                # the backward kernel itself: the input-side mask on dy, everything after it as the unfused kernel
                s, w = plain.grad_fn.saved_tensors[0], g.detach()
                ds1, none, dg1, db1 = o.layernorm_drop_bwd(s, w, dy, EPS, p, hs, site_in=0)
                ds0, dg0, db0 = o.layernorm_bwd(s, w, (dy.float() * scale).to(dtype) * mask.to(dtype), EPS)
                assert none is None and torch.equal(ds1, ds0) and torch.equal(dg1, dg0) and torch.equal(db1, db0), label
                # under autograd: the LayerNorm parameters bit for bit; the tables go through an atomic index_add_ of the same
                # ds: bit for bit where the unfused op reproduces itself, else within twice its own run-to-run distance
                ts = (word, pe, te, g, be)
                g1, g0, g0b = _grads(y1, dy, *ts), _grads(y0, dy, *ts), None
                y0b = StandIn.apply(o.bert_embed_ln_train(ids, pos, tts, word, te, pe, g, be, EPS, pad), mask, scale)
                g0b = _grads(y0b, dy, *ts)
                assert float(g1[0][pad].abs().max()) == 0.0                 # padding_idx keeps its zero gradient
                for name, x1, x0, x0b in zip(("word", "pos", "type", "gamma", "beta"), g1, g0, g0b):
                    if torch.equal(x0, x0b):
                        assert torch.equal(x1, x0), (name,) + label
                    else:
                        assert name in ("word", "pos", "type"), name
                        assert float((x1.double() - x0.double()).norm()) <= 2 * float((x0b.double() - x0.double()).norm()), (name,) + label


@pytest.mark.parametrize("dtype", DTYPES)
def test_p_zero_reproduces_the_ops_as_they_were(dtype):
    o = ops()
    from rankpo_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for d in DIMS:
        rows = 37
        a, big, g, be, dy = _ln_case(dtype, d, rows, seed=5)
        b = big[:, :d]
        y1 = o.add_layernorm_train(a, b, g, be, EPS, 0.0, 12345, 3)
        assert torch.equal(y1, o.add_layernorm(a.detach(), b.detach(), g.detach(), be.detach(), EPS))
        g1 = _grads(y1, dy, a, big, g, be)
        g0 = _grads(o.add_layernorm_train(a, b, g, be, EPS), dy, a, big, g, be)
        assert all(torch.equal(x1, x0) for x1, x0 in zip(g1, g0))
        assert torch.equal(g1[0], g1[1][:, :d])                              # without dropout ds is the gradient of both addends
        # the drop entries themselves with p = 0: keep everything, scale nothing
        y, s = (torch.full((rows, d), float("nan"), dtype=dtype, device=DEV) for _ in range(2))
        assert lib.rpo_add_layernorm_drop_fwd(a.data_ptr(), d, b.data_ptr(), 2 * d, g.data_ptr(), be.data_ptr(), EPS, y.data_ptr(), d,
                                              s.data_ptr(), d, rows, d, o._dt(a), 0.0, 12345, 3, st) == 0
        assert torch.equal(y, y1) and torch.equal(s, a.detach() + b.detach())
        ds1, db1, dg1, dbe1 = o.layernorm_drop_bwd(s, g.detach(), dy, EPS, 0.0, 12345, site_out=3)
        ds0, dg0, dbe0 = o.layernorm_bwd(s, g.detach(), dy, EPS)
        assert torch.equal(ds1, ds0) and torch.equal(db1, ds0) and torch.equal(dg1, dg0) and torch.equal(dbe1, dbe0)
    # and b = None keeps working without dropout, and is refused with it
    a, big, g, be, dy = _ln_case(dtype, 64, 5)
    assert torch.equal(o.add_layernorm_train(a, None, g, be, EPS, 0.0), o.add_layernorm(a.detach(), None, g.detach(), be.detach(), EPS))
    with pytest.raises(ValueError):
        o.add_layernorm_train(a, None, g, be, EPS, 0.1, 1, 1)
    torch.cuda.synchronize()
