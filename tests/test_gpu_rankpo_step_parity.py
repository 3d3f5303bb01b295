"""A RankPO training step (`RankPOTrainer.get_batch_loss_metrics` on a packed bf16 Llama policy, with and without a ref model),
EVERY weight gradient against float64, per head arm: what joins the encoder's step (tests/test_gpu_llama_step_parity.py) and the
scoring kernels (tests/test_gpu_loss_parity.py) -- `_embed_pair`'s packed pass, cat and split, the ref-model leg under
`inference_mode`, the head's cotangent (paired dots only, rows from saturated to steep, whole rows zeroed by the hinge) through the
last block on the pooled rows, the left-padded decline to the padded path, `compute_loss`'s deferred metrics, and the f32 Llama
switches with policy and ref model in one step.

Rule, float64 reference, controls, head arms and the conditions C1-C3 on their inputs are tests/rankpo_step_parity_util.py's; the
float64 graph and the eager control graph are built once per (layout, batch) and shared by the arms.  Every arm installs spies for
the duration of its product step alone and compares what ran with what the arm is named after.  Two injected defects (the ref
columns exchanged, `_embed_pair`'s split moved by one row) show that the harness can fail, and where.  Every arm prints its worst
tensor as a table row (profiles/rankpo_step_grad_parity.md holds a copy)."""
import collections

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import llama_step_parity_util as U
import rankpo_step_parity_util as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Spy:
    """Records what one product step ran, per encoder.  Installed through a `monkeypatch` context of its own."""

    def __init__(self, m, pol, ref=None):
        from rankpo_amd import _lib, encoder as PE, ops
        self.n, self.multi, self.pool, self.head_refs, self.last_rows, self.ckpt = collections.Counter(), [], [], [], [], 0
        lib = _lib.load()
        who = {id(pol): "pol"}
        layer_of = {id(layer): "pol" for layer in pol.layers}
        if ref is not None:
            who[id(ref)] = "ref"
            layer_of.update({id(layer): "ref" for layer in ref.layers})

        def count(obj, name, key, record=None):
            real = getattr(obj, name)

            def spy(*a, **kw):
                self.n[key] += 1
                out = real(*a, **kw)
                if record is not None:
                    record(out, *a, **kw)
                return out
            m.setattr(obj, name, spy)
        for k in ("rpo_rankpo_fwd", "rpo_rankpo_bwd"):
            count(lib, k, k)
        count(ops, "flash_attn_varlen_bwd", "bwd")
        count(ops, "rope_flash_attn_varlen_qkv", "fused_grad")
        count(ops, "rope_flash_attn_varlen_qkv_fwd", "fused_nograd")
        count(ops, "last_query_attn", "lastq")
        count(PE, "checkpoint", "ckpt")
        count(PE.LlamaEncoder, "pooled_last_token_multi", "multi",
              lambda out, enc, batches: self.multi.append((who[id(enc)], out is not None, torch.is_grad_enabled(), len(batches))))
        count(PE.LlamaLayer, "forward_last_rows", "last_rows",
              lambda out, layer, *a, **kw: self.last_rows.append((layer_of[id(layer)], torch.is_grad_enabled())))
        count(ops, "pool_normalize", "pool",
              lambda out, h, mask, mode="last", *a, **kw: self.pool.append((mode, mask is not None, torch.is_grad_enabled(), tuple(h.shape))))
        count(ops, "rankpo_loss_metrics", "head",
              lambda out, q, p, cfg, rc=None, rr=None: self.head_refs.append(None if rc is None else (rc.requires_grad or rr.requires_grad)))


def _check_packed_step(spy, c, with_ref, ckpt=0):
    """What a packed step of case `c` must have run: the policy, the ref model (arms with one), the head."""
    nb = c.cfg.num_hidden_layers
    full = nb - 1
    n = spy.n
    # the policy: one packed pass for query ‖ passage that returned rows, under grad; the last block on the pooled rows
    pol_multi = [x for x in spy.multi if x[0] == "pol"]
    assert pol_multi == [("pol", True, True, 2)], spy.multi
    assert n["bwd"] == full, n                                     # the policy's full blocks, and nobody else's
    assert n["fused_grad"] == full + min(ckpt, full), n
    # (a recomputation that torch.utils.checkpoint stops early is counted when it starts and never returns to be recorded)
    assert [x for x in spy.last_rows if x[0] == "pol"] == [("pol", True)], spy.last_rows
    assert n["last_rows"] == 1 + int(ckpt == nb) + int(with_ref), n
    assert n["ckpt"] == ckpt, n
    # the ref model: its packed pass ran, under no-grad, on the forward-only kernels; no backward kernel beyond the policy's
    if with_ref:
        assert [x for x in spy.multi if x[0] == "ref"] == [("ref", True, False, 2)], spy.multi
        assert [x for x in spy.last_rows if x[0] == "ref"] == [("ref", False)], spy.last_rows
        assert n["fused_nograd"] == full, n
        assert spy.head_refs == [None, False], spy.head_refs       # the ref leg's own head call, then the policy's with ref scores
    else:
        assert len(spy.multi) == 1 and n["fused_nograd"] == 0 and spy.head_refs == [None], (spy.multi, n, spy.head_refs)
    assert n["lastq"] == (2 if with_ref else 1) + int(ckpt == nb), n
    # the rows go through pool_normalize as ONE [nq + np, 1, d] tensor per encoder
    rows = c.batch["query"]["input_ids"].shape[0] + c.batch["passage"]["input_ids"].shape[0]
    want = ([("cls", False, False, (rows, 1, c.cfg.hidden_size))] if with_ref else []) + [("cls", False, True, (rows, 1, c.cfg.hidden_size))]
    assert sorted(spy.pool) == sorted(want), spy.pool
    # the head
    assert n["rpo_rankpo_fwd"] == (2 if with_ref else 1) and n["rpo_rankpo_bwd"] == 1, n


def _run_arm(monkeypatch, c, arm, ckpt=0, name=None):
    with_ref = R.ARMS[arm][1]
    with monkeypatch.context() as m:
        if ckpt:
            m.setattr(c.pol, "gradient_checkpointing", True)
            m.setattr(c.pol, "checkpoint_layers", None if ckpt == c.cfg.num_hidden_layers else ckpt)
            m.setattr(c.pol, "memory_plan", None)
        spy = Spy(m, c.pol, c.ref if with_ref else None)
        fast = R.fast_step(c, arm)
        torch.cuda.synchronize()
    print()
    fails, rec = R.judge(c, arm, fast, name=name)
    return fails, spy, fast


@pytest.mark.parametrize("arm", list(R.ARMS))
def test_every_head_arm_every_gradient(monkeypatch, arm):
    """Config S hd64 (8 / 2 heads) on 8 queries + 16 passages, >= 4096 packed tokens: the filler fires in both encoders."""
    c = R.case_r("hd64")
    fails, spy, _ = _run_arm(monkeypatch, c, arm)
    _check_packed_step(spy, c, R.ARMS[arm][1])
    assert not fails, fails


@pytest.mark.parametrize("arm", ["H2", "H4"])
def test_head_dim_128(monkeypatch, arm):
    c = R.case_r("hd128_g2")
    fails, spy, _ = _run_arm(monkeypatch, c, arm)
    _check_packed_step(spy, c, True)
    assert not fails, fails


def test_every_block_checkpointed(monkeypatch):
    """`gradient_checkpointing` on all 4 blocks of the policy (the last one on the pooled rows included): same reference, same
    controls, same rule."""
    c = R.case_r("hd64")
    assert c.pol.training
    nb = c.cfg.num_hidden_layers
    fails, spy, _ = _run_arm(monkeypatch, c, "H2", ckpt=nb, name="H2 every block checkpointed hd64")
    _check_packed_step(spy, c, True, ckpt=nb)
    assert not fails, fails


def test_left_padded_batch_takes_the_padded_path(monkeypatch):
    """The same rows left-padded: `pooled_last_token_multi` declines for the policy and for the ref model, both run the padded
    `model(**inputs)` pass with `pool_normalize(..., "last")` and its dense [N, L, d] backward.  The rule runs against this batch's
    own float64 reference and eager control; the padded path never consults `hand_attention`, so there is no control (ii)."""
    c = R.case_left("hd64")
    fails, spy, _ = _run_arm(monkeypatch, c, "H2", name="H2 left-padded hd64")
    assert spy.multi and all(not returned for _, returned, _, _ in spy.multi), spy.multi
    assert {(w, g) for w, _, g, _ in spy.multi} == {("pol", True), ("ref", False)}, spy.multi
    d = c.cfg.hidden_size
    want = [("last", True, grad, (n, L, d)) for grad in (True, False) for n, L in ((R.NQ, 128), (R.NP, 320))]
    assert sorted(spy.pool) == sorted(want), spy.pool
    assert spy.n["bwd"] == 0 and spy.n["last_rows"] == 0 and spy.n["rpo_rankpo_fwd"] == 2 and spy.n["rpo_rankpo_bwd"] == 1, spy.n
    assert not fails, fails


def test_compute_loss_is_the_same_step():
    """`compute_loss(model, batch)` on the deferred-metrics path: the loss bits and the gradient bits of `get_batch_loss_metrics`,
    and after two calls `log` returns each metric as the mean of the two resolved vectors."""
    import rankpo_amd
    c = R.case_r("hd64")
    knobs = R.ARMS["H2"][0]
    params = [dict(c.pol.named_parameters())[n] for n in c.names]
    second = U.to_device(R.batch_r(R.BATCH_SEEDS["hd64"] + 1)[0], DEV)
    tr = rankpo_amd.RankPOTrainer(c.pol, c.ref, **knobs)
    want, resolved = [], []
    for b in (c.dev_batch, second):
        loss, metrics = tr.get_batch_loss_metrics(c.pol, b)
        want.append((loss.detach().clone(), torch.autograd.grad(loss, params)))
        resolved.append(metrics)
    assert tr._pending_metrics is None and not tr._stored_metrics["train"]
    for b, (loss0, g0) in zip((c.dev_batch, second), want):
        loss = tr.compute_loss(c.pol, b)
        assert torch.is_tensor(loss) and loss.requires_grad and torch.equal(loss.detach(), loss0)
        for n, a, g in zip(c.names, torch.autograd.grad(loss, params), g0):
            assert torch.equal(a, g), n
    assert tr._pending_metrics[2] == 2
    logs = tr.log({"loss": 0.0})
    assert set(logs) == {"loss"} | set(resolved[0]) and len(resolved[0]) == 9
    for k in resolved[0]:
        mean = float((torch.tensor(resolved[0][k], dtype=torch.float32) + torch.tensor(resolved[1][k], dtype=torch.float32)) / 2)
        assert logs[k] == pytest.approx(mean, rel=1e-6, abs=1e-7), k
    assert any(abs(resolved[0][k] - resolved[1][k]) > 1e-3 for k in resolved[0])     # the two batches do differ
    assert tr._pending_metrics is None


# ------------------------------------------------------------------------------------------------------------------------------
# f32 policy and f32 ref model on the f32 kernels, in one step
# ------------------------------------------------------------------------------------------------------------------------------
def test_f32_policy_and_ref_on_the_f32_kernels(monkeypatch):
    """Policy under grad mode on `causal_attn_f32_train` / `_bwd`, the ref model in the same step on the no-grad f32 op.  Reference:
    float64 on the host.  Control: the same two encoders with every f32 switch off.  Rule (tests/test_gpu_llama_f32_train.py):
    err <= 1.5 x control + 2^-22 per parameter in the relative Frobenius norm; loss and scores by that file's `_rule`."""
    import rankpo_amd
    import test_gpu_llama_f32_train as FT
    from rankpo_amd import ops
    from test_gpu_inference import CharTok, _texts
    from test_gpu_llama_f32 import _rule
    PE, cfg, w_pol, pol = FT._build(64, 94, f32_attention=True)
    _, _, w_ref, ref = FT._build(64, 95, f32_attention=True)
    pol, ref = pol.model, ref.model
    assert pol.f32_attention_train and ref.f32_attention and pol.embed_tokens.weight.dtype == torch.float32
    rs = np.random.RandomState(64)
    tok = CharTok()
    host = {"query": tok(_texts(rs, 3, 1, 60) + ["q"], max_length=400),
            "passage": tok(_texts(rs, 7, 40, 400) + _texts(rs, 1, 380, 400), max_length=400)}
    batch = U.to_device(host, DEV)
    names = U.param_names(pol)
    knobs = R.ARMS["H2"][0]
    nl = cfg.num_hidden_layers
    seen = collections.Counter()

    def count(obj, name, key):
        real = getattr(obj, name)

        def spy(*a, **kw):
            seen[key, torch.is_inference_mode_enabled()] += 1
            return real(*a, **kw)
        return obj, name, spy

    def step():
        seen.clear()
        with monkeypatch.context() as m:
            for obj, name, key in ((ops, "causal_attn_f32_train", "train"), (ops, "causal_attn_f32_bwd", "bwd"),
                                   (ops, "causal_attn_f32", "fwd"), (F, "scaled_dot_product_attention", "sdpa")):
                m.setattr(*count(obj, name, key))
            out = R.trainer_step(pol, ref, knobs, batch, names)
            torch.cuda.synchronize()
        return out, dict(seen)
    fast, n = step()
    # the policy: one training node per block (the last one the one-query form) and its backward; the ref: the no-grad op per block
    assert n.get(("train", False)) == nl and n.get(("bwd", False)) == nl and n.get(("fwd", True)) == nl, n
    assert not any(k[0] == "sdpa" for k in n) and not any(k[0] in ("train", "bwd") and k[1] for k in n), n
    for e in (pol, ref):
        monkeypatch.setattr(e, "f32_attention", False)
        monkeypatch.setattr(e, "f32_attention_train", False)
    assert not PE.LLAMA_F32_ATTENTION and not PE.LLAMA_F32_ATTENTION_TRAIN
    ctrl, n = step()
    assert {k[0] for k in n} == {"sdpa"}, n
    o = R.Oracle64(w_pol, w_ref, cfg.to_dict(), host, names, arms={"H2": R.ARMS["H2"]})
    loss, scores, grads, _ = o.step("H2")
    _rule(fast[0].cpu().view(1), ctrl[0].cpu().view(1), torch.tensor([loss], dtype=torch.float64), "loss f32 policy + ref")
    _rule(fast[1].cpu(), ctrl[1].cpu(), scores, "scores f32 policy ‖ ref")
    worst = (0.0, None)
    for k in names:
        e, ce = U.rel_err(fast[2][k], grads[k]), U.rel_err(ctrl[2][k], grads[k])
        assert e is not None and ce is not None, k
        worst = max(worst, (e / (1.5 * ce + 2.0 ** -22), k, e, ce))
        assert e <= 1.5 * ce + 2.0 ** -22, (k, e, ce)
    print(f"\nf32 policy + ref, H2: worst err / bound {worst[0]:.3f} at {worst[1]} (rel. Frobenius {worst[2]:.3e}, control {worst[3]:.3e})")


# ------------------------------------------------------------------------------------------------------------------------------
# the harness must be able to fail: two defects injected at the Python level
# ------------------------------------------------------------------------------------------------------------------------------
def test_injected_exchanged_ref_columns(monkeypatch):
    """`ops.rankpo_loss_metrics` receives `ref_chosen` / `ref_rejected` exchanged: H2 fails on the loss statistic and on
    gradients; H1 (reference-free, no ref model) passes under the same patch."""
    from rankpo_amd import ops
    c = R.case_r("hd64")
    real = ops.rankpo_loss_metrics
    for arm in ("H1", "H2"):
        R.flash_step(c, arm)                                       # control (ii) is the healthy product: made before the patch
    monkeypatch.setattr(ops, "rankpo_loss_metrics", lambda q, p, cfg, rc=None, rr=None: real(q, p, cfg, rr, rc))
    print()
    fails, _ = R.judge(c, "H2", R.fast_step(c, "H2"), name="defect (a) exchanged ref columns, H2")
    assert "loss_abs_err" in U.failed_names(fails, "stat"), fails
    assert U.failed_names(fails, "grad"), fails
    print(f"defect (a): {len(U.failed_names(fails, 'grad'))} of {len(c.names)} gradients over their bound; metrics: {U.failed_names(fails, 'metric')}")
    fails, _ = R.judge(c, "H1", R.fast_step(c, "H1"), name="defect (a) exchanged ref columns, H1")
    assert not fails, fails


def test_injected_split_moved_by_one_row(monkeypatch):
    """`_embed_pair`'s split one row early: the last query row becomes the first passage row.  Either the head refuses the shapes
    (7 queries, 17 passages) or the rule fails; the test accepts either and says which happened."""
    import rankpo_amd
    c = R.case_r("hd64")
    real = rankpo_amd.RankPOTrainer._embed_pair
    R.flash_step(c, "H1")                                          # control (ii) is the healthy product: made before the patch

    def bad(self, model, batch):
        q, p = real(self, model, batch)
        both, nq = torch.cat([q, p], 0), q.shape[0] - 1
        return both[:nq].contiguous(), both[nq:].contiguous()
    monkeypatch.setattr(rankpo_amd.RankPOTrainer, "_embed_pair", bad)
    try:
        fast = R.fast_step(c, "H1")
    except ValueError as e:
        assert "2 passages" in str(e), e
        print(f"\ndefect (b): the head refused the shapes: {e}")
        return
    print()
    fails, _ = R.judge(c, "H1", fast, name="defect (b) split moved by one row, H1")
    print(f"defect (b): the rule failed: {U.failed_names(fails)}")
    assert fails
