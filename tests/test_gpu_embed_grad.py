"""The sorted embedding-table gradient on the GPU (`ops.embed_grad_sorted`, rankpo_amd/csrc/embed_grad.hip) and the packed BERT /
XLM-R step with `encoder.BERT_DETERMINISTIC_EMBED_GRAD` on.

The order of the sum is part of the kernel's contract, so its result must equal the float32 CPU restatement of that order
(tests/embed_grad_util.py) BIT FOR BIT; the float64 bounds are derived there, not measured.  With the switch on, two same-seed steps
must agree in every gradient, the three embedding tables included."""
import functools

import numpy as np
import pytest
import torch

import embed_grad_util as EG
from test_gpu_bert_train import DEV, DTYPES, _step, ops

pytestmark = pytest.mark.gpu
WIDTHS = [8, 64, 384, 520, 1024]        # 520 and 1024: more than one 512-column slice, 520 with a ragged one
ROWS, PAD = 14, 4


@functools.lru_cache(maxsize=None)
def _case(dtype, d):
    """One run per (dtype, d), shared by the tests below: (x, ids, got on the CPU, plan on the device)."""
    o = ops()
    ids = EG.segment_ids(o.EMBED_GRAD_CHUNK, ROWS, PAD, seed=d)
    x = EG.normal_values(len(ids), d, dtype, seed=d + 1)
    plan = o.embed_grad_plan_to(o.embed_grad_plan(ids), DEV)
    got = o.embed_grad_sorted(x.to(DEV), plan, ROWS, PAD)
    assert got.dtype == dtype and got.shape == (ROWS, d) and got.is_contiguous()
    return x, ids, got.cpu(), plan


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_equals_the_documented_order_bit_for_bit(dtype, d):
    x, ids, got, _ = _case(dtype, d)
    emu = EG.emulate(x, ids, ROWS, ops().EMBED_GRAD_CHUNK, dtype, PAD)
    assert torch.isfinite(got.float()).all()
    assert float(got[PAD].abs().max()) == 0.0 and (ids == PAD).sum() == 5          # contributions arrive, the row stays zero
    untouched = [r for r in range(ROWS) if r not in set(ids.tolist())]
    assert untouched and float(got[untouched].abs().max()) == 0.0
    assert torch.equal(got, emu), (float((got.double() - emu.double()).abs().max()),
                                   (got != emu).any(1).nonzero().flatten().tolist())


@pytest.mark.parametrize("ids", [[3], [2] * 70, list(range(9, -1, -1))], ids=["single-token", "all-equal", "all-distinct"])
def test_edge_id_lists_bit_for_bit(ids):
    o, dtype, d, rows = ops(), torch.float16, 72, 10
    ids = np.asarray(ids, dtype=np.int64)
    x = EG.normal_values(len(ids), d, dtype, seed=len(ids))
    got = o.embed_grad_sorted(x.to(DEV), o.embed_grad_plan_to(o.embed_grad_plan(ids), DEV), rows).cpu()
    assert torch.equal(got, EG.emulate(x, ids, rows, o.EMBED_GRAD_CHUNK, dtype))
    assert int((got != 0).any(1).sum()) == len(set(ids.tolist()))


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_f64_parity(dtype, d):
    x, ids, got, _ = _case(dtype, d)
    ref, mag, n = EG.reference64(x, ids, ROWS, PAD)
    err, bound = (got.double() - ref).abs(), EG.parity_bound(ref, mag, n, dtype)
    print(f"embed_grad f64 parity {dtype} d={d}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_two_calls_return_equal_bits(dtype):
    x, _, got, plan = _case(dtype, 520)
    xd = x.to(DEV)
    for _ in range(2):
        assert torch.equal(ops().embed_grad_sorted(xd, plan, ROWS, PAD).cpu(), got)
    # a strided ds (row stride 528) is taken as it is
    wide = torch.zeros(x.shape[0], 528, dtype=dtype, device=DEV)
    wide[:, :520] = xd
    assert torch.equal(ops().embed_grad_sorted(wide[:, :520], plan, ROWS, PAD).cpu(), got)


@pytest.mark.parametrize("d", [64, 520])
@pytest.mark.parametrize("dtype", DTYPES)
def test_agrees_with_the_index_add_path(dtype, d):
    x, ids, got, _ = _case(dtype, d)
    stock = torch.zeros(ROWS, d, dtype=torch.float32, device=DEV).index_add_(0, torch.tensor(ids, device=DEV), x.to(DEV).float())
    stock[PAD].zero_()
    stock = stock.to(dtype).cpu()
    ref, mag, n = EG.reference64(x, ids, ROWS, PAD)
    err, bound = (got.double() - stock.double()).abs(), EG.agreement_bound(ref, mag, n, dtype)
    print(f"embed_grad vs index_add_ {dtype} d={d}: max diff / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", DTYPES)
def test_inf_and_nan_reach_their_row_and_column_only(dtype):
    o = ops()
    x, ids, _, plan = _case(dtype, 520)
    x = x.clone()
    long_row = int(np.bincount(ids).argmax())                                # the segment of 3 chunk + 1 rows: through the partials
    short_row = int(ids[np.flatnonzero(np.bincount(ids)[ids] == o.EMBED_GRAD_CHUNK - 1)[0]])
    t_inf, t_nan = int(np.flatnonzero(ids == long_row)[40]), int(np.flatnonzero(ids == short_row)[3])
    x[t_inf, 515], x[t_nan, 7] = float("inf"), float("nan")
    x[int(np.flatnonzero(ids == PAD)[0]), 100] = float("nan")                # into the padding row: goes nowhere
    got = o.embed_grad_sorted(x.to(DEV), plan, ROWS, PAD).cpu().float()
    bad = (~torch.isfinite(got)).nonzero().tolist()
    assert sorted(bad) == sorted([[long_row, 515], [short_row, 7]]), bad
    assert got[long_row, 515] == float("inf") and torch.isnan(got[short_row, 7])


def test_rejects_what_the_kernel_does_not_take():
    o = ops()
    from rankpo_amd._lib import RankPOHipError
    _, ids, _, plan = _case(torch.float16, 64)
    with pytest.raises(RankPOHipError, match="status -2"):
        o.embed_grad_sorted(torch.zeros(len(ids), 64, device=DEV), plan, ROWS)                     # f32 storage
    with pytest.raises(RankPOHipError, match="status -2"):
        o.embed_grad_sorted(torch.zeros(len(ids), 60, dtype=torch.float16, device=DEV), plan, ROWS)   # d % 8
    with pytest.raises(ValueError):
        o.embed_grad_sorted(torch.zeros(3, 64, dtype=torch.float16, device=DEV), plan, ROWS)      # another T


def _embed_backward_peak(o, plans_on):
    """Peak allocation across the backward of `bert_embed_ln_train` over what was allocated before it, and the gradients' bytes."""
    dtype, V, P, TT, d, T = torch.float16, 65536, 64, 2, 128, 256
    gen = torch.Generator(device=DEV).manual_seed(9)
    mk = lambda *sh: (torch.randn(*sh, generator=gen, device=DEV) * 0.1).to(dtype).requires_grad_(True)
    word, pe, te, g, be = mk(V, d), mk(P, d), mk(TT, d), mk(d), mk(d)
    ids = torch.randint(0, V, (T,), generator=gen, device=DEV, dtype=torch.int32)
    pos = torch.randint(0, P, (T,), generator=gen, device=DEV, dtype=torch.int32)
    tts = torch.randint(0, TT, (T,), generator=gen, device=DEV, dtype=torch.int32)
    plans = tuple(o.embed_grad_plan_to(o.embed_grad_plan(t.cpu()), DEV) for t in (ids, pos, tts)) if plans_on else None
    dy = torch.randn(T, d, generator=gen, device=DEV).to(dtype)
    y = o.bert_embed_ln_train(ids, pos, tts, word, te, pe, g, be, 1e-12, 0, plans=plans)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y.backward(dy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    grads = sum(t.grad.numel() * t.grad.element_size() for t in (word, pe, te))
    return peak, grads, (word.grad, pe.grad, te.grad)


def test_backward_builds_no_f32_table():
    """Fails on the stock scatter, which holds the f32 table and its 16-bit copy together: three times the gradient's bytes."""
    peak, grads, (gw, gp, gt) = _embed_backward_peak(ops(), True)
    print(f"embedding backward with plans: peak {peak} bytes over the start, table gradients {grads} bytes")
    assert peak < 2 * grads, (peak, grads)
    stock_peak, _, (sw, sp, st) = _embed_backward_peak(ops(), False)        # same seeded inputs through the stock path
    print(f"embedding backward, stock scatter: peak {stock_peak} bytes over the start")
    for a, b in ((gw, sw), (gp, sp), (gt, st)):
        assert float((a.double() - b.double()).norm()) <= 2.0 ** -9 * float(b.double().norm())
    assert float(gw[0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------
# the whole step
# ------------------------------------------------------------------------------------------------
P_DROP = 0.1
TABLES = ("embeddings.word_embeddings.weight", "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight")


def _tiny(dtype, seed):
    import rankpo_amd
    from rankpo_amd import encoder as PE
    torch.manual_seed(seed)
    cfg = PE.bge_small_config(vocab_size=50, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2,
                              hidden_dropout_prob=P_DROP, attention_probs_dropout_prob=P_DROP)
    enc = PE.build_encoder(cfg)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("bias") or "LayerNorm" in n:
                p.add_(0.05 * torch.randn_like(p))
    model = rankpo_amd.ModelForTraining(encoder=enc.to(DEV).to(dtype), temperature=0.02).train()
    rs = np.random.RandomState(seed)

    def side(lens):                       # right-padded to 40, both token types, few distinct ids: every table row is hit often
        lens = np.asarray(lens)
        m = (np.arange(40)[None, :] < lens[:, None]).astype(np.int64)
        ids = rs.randint(1, cfg.vocab_size, size=m.shape) * m
        tts = (np.arange(40)[None, :] >= (lens[:, None] + 1) // 2).astype(np.int64) * m
        return {"input_ids": torch.tensor(ids).to(DEV), "attention_mask": torch.tensor(m).to(DEV),
                "token_type_ids": torch.tensor(tts).to(DEV)}
    batch = {"query": side([40, 1]), "passage": side([33, 1, 40, 17])}      # 6 sequences of 1 .. 40 tokens
    return PE, cfg, model, batch


def _seeded(model, batch, seed):
    torch.manual_seed(seed)
    return _step(model, batch)


def _all_equal(a, b, label):
    (la, sa, ga), (lb, sb, gb) = a, b
    assert torch.isfinite(la) and torch.equal(la, lb) and torch.equal(sa, sb), label
    assert set(ga) == set(gb) and all(t in ga for t in TABLES)
    for k in ga:
        assert torch.isfinite(ga[k]).all() and (k not in TABLES or float(ga[k].abs().max()) > 0), (label, k)
        assert torch.equal(ga[k], gb[k]), (label, k, float((ga[k] - gb[k]).abs().max()))


@pytest.mark.parametrize("dtype", DTYPES)
def test_whole_step_is_bit_reproducible_with_the_switch_on(dtype, monkeypatch):
    PE, cfg, model, batch = _tiny(dtype, 5)
    calls = []
    real = ops().embed_grad_sorted
    monkeypatch.setattr(ops(), "embed_grad_sorted", lambda *a, **kw: calls.append(a[2]) or real(*a, **kw))
    monkeypatch.setattr(PE, "BERT_DETERMINISTIC_EMBED_GRAD", True)
    a = _seeded(model, batch, 77)
    assert sorted(calls) == sorted(2 * [cfg.vocab_size, cfg.max_position_embeddings, cfg.type_vocab_size]), calls   # two towers
    b = _seeded(model, batch, 77)
    _all_equal(a, b, "same seed")
    assert not torch.equal(_seeded(model, batch, 78)[0], a[0])               # dropout is on: another seed, another step
    # checkpointing the packed blocks changes nothing, the tables included (the embedding is outside the checkpointed blocks)
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", True)
    plain = _seeded(model, batch, 77)
    model.gradient_checkpointing_enable(packed=True)
    assert model.model.checkpoint_packed
    _all_equal(_seeded(model, batch, 77), plain, "checkpointed")


@pytest.mark.parametrize("dtype", DTYPES)
def test_switch_on_agrees_with_switch_off(dtype, monkeypatch):
    """Bit for bit everywhere but the three tables; there within the agreement bound, from the float64 sums of the very ds rows."""
    from test_gpu_bert_train import LOSS_SCALE
    PE, cfg, model, batch = _tiny(dtype, 6)
    o, enc = ops(), model.model
    seen = []
    real = o.embed_grad_sorted

    def spy(ds, plan, rows, padding_idx=None):
        seen.append((ds.detach().cpu(), np.asarray(plan.seg_ids), np.asarray(plan.seg_start), plan.order.cpu().numpy(), rows,
                     padding_idx))
        return real(ds, plan, rows, padding_idx)
    calls = []
    monkeypatch.setattr(o, "embed_grad_sorted", lambda *a, **kw: calls.append(1) or real(*a, **kw))
    off = _seeded(model, batch, 91)
    assert not calls                                                         # switch off: the stock scatter, as ever
    monkeypatch.setattr(o, "embed_grad_sorted", spy)
    monkeypatch.setattr(PE, "BERT_DETERMINISTIC_EMBED_GRAD", True)
    on = _seeded(model, batch, 91)
    assert len(seen) == 6
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1])
    for k in off[2]:
        if k not in TABLES:
            assert torch.equal(on[2][k], off[2][k]), k
    # a parameter's gradient = the sum over the two towers of their table gradients, each rounded to storage, added in storage
    by_rows = {cfg.vocab_size: TABLES[0], cfg.max_position_embeddings: TABLES[1], cfg.type_vocab_size: TABLES[2]}
    bound = {k: 0.0 for k in TABLES}
    total = {k: 0.0 for k in TABLES}
    for ds, seg_ids, seg_start, order, rows, pad in seen:
        ids = np.empty(len(order), np.int64)
        ids[order] = np.repeat(seg_ids, np.diff(seg_start))
        ref, mag, n = EG.reference64(ds, ids, rows, pad)
        k = by_rows[rows]
        bound[k] = bound[k] + EG.agreement_bound(ref, mag, n, dtype)
        total[k] = total[k] + ref
    for k in TABLES:
        b = (bound[k] + 2 * EG.ulp(total[k], dtype)) / LOSS_SCALE            # + the tower add's rounding on either side
        err = (on[2][k] - off[2][k]).abs()
        print(f"switch on vs off {dtype} {k}: max diff / bound = {float((err / b.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= b).all()), k


def test_api_presence():
    """The entries, the op and the switch this file tests: missing from the library and the package before them."""
    from rankpo_amd import _lib, encoder
    lib = _lib.load()
    assert hasattr(lib, "rpo_embed_grad_sorted") and hasattr(lib, "rpo_embed_grad_workspace_elems")
    assert callable(ops().embed_grad_sorted) and callable(ops().embed_grad_plan) and ops().EMBED_GRAD_CHUNK >= 1
    assert encoder.BERT_DETERMINISTIC_EMBED_GRAD is False
