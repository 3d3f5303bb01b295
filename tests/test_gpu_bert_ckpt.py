"""Gradient checkpointing on the packed BERT / XLM-R training step (`BertEncoder.gradient_checkpointing_enable(packed=True)`) and
the fused hidden dropout it rests on (`encoder.BERT_FUSED_HIDDEN_DROPOUT`), end to end on the small configs of
tests/test_gpu_bert_train.py.

Nothing here is approximate: the fused dropout rounds where the separate pass rounds, and a recomputed block repeats the same
deterministic kernels with the same stateless masks.  So loss and scores must pass `torch.equal`, and so must every gradient that
the baseline reproduces over two runs of its own; the embedding tables go through an atomic `index_add_`, and where the baseline
differs from itself the candidate may differ from it by at most twice that distance (the rule of
`test_training_declines_fall_back_to_the_padded_path_bit_for_bit`)."""
import numpy as np
import pytest
import torch

from test_gpu_bert_train import DEV, DTYPES, TrainSpy, _batch, _make, _step, ops

pytestmark = pytest.mark.gpu
P_DROP = 0.1


def _dev(batch):
    return {k: {kk: vv.to(DEV) for kk, vv in v.items()} for k, v in batch.items()}


def _same_step(cand, base, base2, label):
    (l1, s1, g1), (l0, s0, g0), (_, _, g0b) = cand, base, base2
    assert torch.isfinite(l1) and torch.equal(l1, l0) and torch.equal(s1, s0), (label, float(l1), float(l0))
    for k in g0:
        assert torch.isfinite(g1[k]).all(), (label, k)
        if torch.equal(g0[k], g0b[k]):
            assert torch.equal(g1[k], g0[k]), (label, k, float((g1[k] - g0[k]).norm()), float(g0[k].norm()))
        else:
            assert float((g1[k] - g0[k]).norm()) <= 2 * float((g0b[k] - g0[k]).norm()), (label, k)


def _seeded_step(model, gb, seed):
    torch.manual_seed(seed)
    return _step(model, gb)


class AttnFwdSpy:
    """Counts the entries into the attention forward (the first pass and a checkpoint's recomputation alike)."""

    def __enter__(self):
        o = ops()
        self.n, self._fwd = 0, o.bidir_attn_train_fwd

        def fwd(*a, **kw):
            self.n += 1
            return self._fwd(*a, **kw)
        o.bidir_attn_train_fwd = fwd
        return self

    def __exit__(self, *exc):
        ops().bidir_attn_train_fwd = self._fwd
        return False


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_fused_hidden_dropout_equals_the_unfused_step_with_the_dumped_masks(kind, dtype, monkeypatch):
    PE, cfg, _, model = _make(kind, dtype, P_DROP, 29)
    enc, o = model.model, ops()
    gb = _dev(_batch(np.random.RandomState(11), cfg))
    from test_gpu_hidden_dropout import StandIn
    scale = o.hidden_dropout_scale(P_DROP)
    real_train = enc.pooled_cls_train
    state = {"site": 0, "calls": 0}

    def stand_in(x, p):
        """`_hidden_dropout` of the unfused step with the fused step's masks: site by call order, rows from 0."""
        assert p == P_DROP
        mask = o.hidden_dropout_mask(0, x.shape[0], x.shape[1], p, o.bert_hidden_seed(enc.last_dropout_seed), state["site"], DEV)
        state["site"] += 1
        state["calls"] += 1
        return StandIn.apply(x, mask, scale)

    def train(ids, mask, tts=None):
        state["site"] = 0                                                    # a tower = a call = its own seed and sites 0 ..
        return real_train(ids, mask, tts)
    monkeypatch.setattr(enc, "pooled_cls_train", train)
    monkeypatch.setattr(PE, "_hidden_dropout", stand_in)
    with TrainSpy() as spy:
        base = _seeded_step(model, gb, 301)
    assert spy.n["sdpa"] == 0 and state["calls"] == 2 * (1 + 2 * cfg.num_hidden_layers), (spy.n, state)
    base2 = _seeded_step(model, gb, 301)
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", True)
    state["calls"] = 0
    with TrainSpy() as spy:
        cand = _seeded_step(model, gb, 301)
    assert spy.n["sdpa"] == 0 and spy.n["bidir_attn_bwd"] == 2 * cfg.num_hidden_layers, spy.n
    assert state["calls"] == 0                                               # the fused step never calls `_hidden_dropout`
    _same_step(cand, base, base2, (kind, dtype))
    other = _seeded_step(model, gb, 302)
    assert not torch.equal(other[0], cand[0])                                # another seed, other masks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["bge-small", "xlm-r"])
def test_packed_checkpointing_equals_the_step_without_it(kind, dtype, monkeypatch):
    PE, cfg, _, model = _make(kind, dtype, P_DROP, 31)
    gb = _dev(_batch(np.random.RandomState(13), cfg))
    L = cfg.num_hidden_layers
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", True)
    with TrainSpy() as spy, AttnFwdSpy() as fwd:
        base = _seeded_step(model, gb, 401)
    assert spy.n["sdpa"] == 0 and spy.n["bidir_attn_bwd"] == 2 * L and fwd.n == 2 * L, (spy.n, fwd.n)
    base2 = _seeded_step(model, gb, 401)
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", False)             # packed=True forces it on by itself
    model.gradient_checkpointing_enable(packed=True)
    assert model.model.checkpoint_packed
    calls = []
    real_drop = PE._hidden_dropout
    monkeypatch.setattr(PE, "_hidden_dropout", lambda x, p: calls.append(p) or real_drop(x, p))
    with TrainSpy() as spy, AttnFwdSpy() as fwd:
        cand = _seeded_step(model, gb, 401)
    assert spy.n["sdpa"] == 0 and spy.n["bidir_attn_bwd"] == 2 * L, spy.n    # the packed path, one backward per block and tower
    assert fwd.n == 2 * 2 * L, fwd.n                                         # the attention forward twice per block and tower
    assert not calls
    _same_step(cand, base, base2, (kind, dtype))


def test_checkpointed_forward_keeps_no_block_activation(monkeypatch):
    PE, cfg, _, model = _make("bge-small", torch.float16, P_DROP, 37)
    gb = _dev(_batch(np.random.RandomState(17), cfg))
    d, inter = cfg.hidden_size, cfg.intermediate_size

    def saved_widths():
        widths = []
        pack = lambda t: (widths.append(t.shape[-1]) if t.is_floating_point() and t.dim() == 2 else None, t)[1]
        with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
            out = model(**gb)
        out.loss.backward()
        return widths
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", True)
    plain = saved_widths()
    assert inter in plain and 3 * d in plain, sorted(set(plain))
    model.gradient_checkpointing_enable(packed=True)
    kept = saved_widths()
    assert inter not in kept and 3 * d not in kept, sorted(set(kept))


def test_bare_flag_still_takes_the_padded_path():
    _, cfg, _, model = _make("bge-small", torch.float16, P_DROP, 41)
    gb = _dev(_batch(np.random.RandomState(19), cfg))
    model.gradient_checkpointing_enable()
    assert not model.model.checkpoint_packed
    with TrainSpy() as spy:
        _step(model, gb)
    assert spy.n["sdpa"] > 0 and spy.n["bidir_attn_bwd"] == 0, spy.n


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("lens", [[7, 1, 33], [40], [1]], ids=["with-length-1", "single-sequence", "single-token"])
def test_ragged_packs_checkpointed_equals_not(lens, dtype, monkeypatch):
    """The CLS-only last block with N = 1 and the sites' row 0, on the encoder alone (a one-row InfoNCE has no gradient)."""
    PE, cfg, _, model = _make("xlm-r", dtype, P_DROP, 43)
    enc = model.model
    rs = np.random.RandomState(len(lens))
    L, pad = max(lens), cfg.pad_token_id
    m = (np.arange(L)[None, :] < np.asarray(lens)[:, None]).astype(np.int64)
    ids = torch.tensor(rs.randint(pad + 1, cfg.vocab_size, size=m.shape) * m + pad * (1 - m)).to(DEV)
    mask = torch.tensor(m).to(DEV)
    dy = torch.randn(len(lens), cfg.hidden_size, generator=torch.Generator().manual_seed(3)).to(DEV).to(dtype)

    def step():
        enc.zero_grad(set_to_none=True)
        torch.manual_seed(501)
        out = enc.pooled_cls_train(ids, mask)
        assert out is not None and out.shape == (len(lens), cfg.hidden_size)
        out.backward(dy)
        return out.detach().clone(), {k: v.grad.double().cpu() for k, v in enc.named_parameters()}
    monkeypatch.setattr(PE, "BERT_FUSED_HIDDEN_DROPOUT", True)
    (y0, g0), (_, g0b) = step(), step()
    enc.gradient_checkpointing_enable(packed=True)
    with AttnFwdSpy() as fwd:
        y1, g1 = step()
    assert fwd.n == 2 * cfg.num_hidden_layers, fwd.n
    assert torch.isfinite(y1.float()).all() and torch.equal(y1, y0)
    for k in g0:
        if torch.equal(g0[k], g0b[k]):
            assert torch.equal(g1[k], g0[k]), k
        else:
            assert float((g1[k] - g0[k]).norm()) <= 2 * float((g0b[k] - g0[k]).norm()), k
