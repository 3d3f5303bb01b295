"""Host side of the RankPO step gradient parity (tests/rankpo_step_parity_util.py): the plain-torch head is the numpy oracle's
`rankpo_batch_loss_metrics` for every arm's knobs, the committed batch seed meets C1 and C2 on both layouts and on the left-padded
batch, and the keyword arguments `U.rule` gained for this head report a tensor over its bound, a missing tensor, a guard failure, a
loss over the L-scaled tolerance, a metric over its bound and a flipped `rewards/accuracies`, each under its own name."""
import numpy as np
import pytest
import torch

import llama_step_parity_util as U
import rankpo_step_parity_util as R
from oracle import scoring_ref as S

NAMES = ["a.weight", "b.weight", "c.weight"]


def _unit(gen, n, d=24):
    x = torch.randn(n, d, generator=gen, dtype=torch.float64)
    return x / x.norm(dim=-1, keepdim=True)


@pytest.mark.parametrize("arm", list(R.ARMS))
def test_head_is_the_numpy_oracle(arm):
    """Loss, scores, all metrics and autograd's (dq, dp) against scoring_ref's, 1e-12 relative: both are float64 restatements of
    the same few operations."""
    knobs, with_ref = R.ARMS[arm]
    gen = torch.Generator().manual_seed(11 + len(arm) + int(arm[1:]))
    B = 7
    q, p = _unit(gen, B).requires_grad_(True), _unit(gen, 2 * B).requires_grad_(True)
    rc, rr = ((torch.rand(B, generator=gen, dtype=torch.float64) - 0.5), (torch.rand(B, generator=gen, dtype=torch.float64) - 0.5)) \
        if with_ref else (None, None)
    loss, scores, metrics = R.rankpo_head(q, p, rc, rr, knobs)
    dq, dp = torch.autograd.grad(loss, (q, p))
    o = S.rankpo_batch_loss_metrics(q.detach().numpy(), p.detach().numpy(), None if rc is None else rc.numpy(),
                                    None if rr is None else rr.numpy(), **R.knobs_of(arm))
    close = lambda a, b: np.testing.assert_allclose(np.asarray(a), np.asarray(b), rtol=1e-12, atol=1e-15)
    close(float(loss.detach()), o["loss"])
    close(scores.detach().numpy(), o["scores"])
    assert set(metrics) == set(o["metrics"]) and set(metrics) <= set(R.METRIC_KEYS)
    assert set(R.lipschitz(knobs)[1]) | set(R.EXACT_METRICS) == set(metrics)           # every metric has its comparison
    for k, v in o["metrics"].items():
        close(float(metrics[k]), v)
    close(dq.numpy(), o["dq"])
    close(dp.numpy(), o["dp"])
    # dtype-generic: the float32 head of the controls
    l32 = R.rankpo_head(q.detach().float(), p.detach().float(), None if rc is None else rc.float(), None if rr is None else rr.float(), knobs)
    assert l32[0].dtype == torch.float32 and l32[1].dtype == torch.float32
    assert abs(float(l32[0]) - o["loss"]) <= 1e-4 * max(1.0, abs(o["loss"]))


def test_lipschitz_constants():
    L, lk = R.lipschitz(R.ARMS["H2"][0])
    assert L == pytest.approx(2 * (1.0 * 2.0 + 0.5) / 0.1) and lk["rankpo_loss"] == pytest.approx(40.0) and lk["sft_loss"] == pytest.approx(20.0)
    assert lk["rewards/margins"] == 4.0 and lk["rewards/chosen"] == 2.0 and lk["scores/margins"] == 2.0 and lk["scores/rejected"] == 1.0
    L, lk = R.lipschitz(R.ARMS["H5"][0])
    assert L == pytest.approx(20.0) and "rankpo_loss" not in lk and lk["rewards/chosen"] == pytest.approx(0.1)
    assert all(R.knobs_of(a)["beta"] / R.knobs_of(a)["temperature"] <= 20 for a in R.ARMS)


def test_conditions_on_hand_made_scores():
    s = torch.tensor([[0.5, 0.1], [0.2, 0.3], [0.3, 0.0], [0.0, 0.25]], dtype=torch.float64)     # adv 0.4, -0.1, 0.3, -0.25
    rs = torch.tensor([[0.1, 0.0], [0.0, 0.0], [0.0, 0.1], [0.0, 0.0]], dtype=torch.float64)     # ref adv 0.1, 0, -0.1, 0
    c = R.conditions(s, rs, "H3")                                                                # 1 - 10 adv = -3, 2, -2, 3.5
    assert c["c2"] == pytest.approx(0.1) and c["c1"] == pytest.approx(2.0) and (c["active"], c["inactive"]) == (2, 2)
    c = R.conditions(s, rs, "H4")                                                                # adv - ref adv 0.3, -0.1, 0.4, -0.25
    assert c["c2"] == pytest.approx(0.1) and c["c1"] == pytest.approx(2.0) and R.conditions_hold(c)
    assert "c1" not in R.conditions(s, rs, "H2")
    near = s.clone()
    near[1] = torch.tensor([0.2, 0.19])                                                          # adv 0.01: C2; 1 - 0.1 = 0.9 is fine
    assert not R.conditions_hold(R.conditions(near, rs, "H1")) and R.conditions(near, rs, "H3")["c1"] == pytest.approx(0.9)
    near[1] = torch.tensor([0.3, 0.19])                                                          # adv 0.11: |1 - 1.1| = 0.1 < 0.25
    assert not R.conditions_hold(R.conditions(near, rs, "H3")) and R.conditions_hold(R.conditions(near, rs, "H1"))
    amp, bad = R.c3(dict(c2=0.03), 2e-3, "H1")                                                   # 40 x 2e-3 = 0.08 <= 0.1; 0.03 >= 8e-3
    assert amp == pytest.approx(0.08) and bad == []
    assert len(R.c3(dict(c2=0.03), 3e-3, "H1")[1]) == 1 and len(R.c3(dict(c2=0.02, c1=0.25, active=2, inactive=2), 6e-3, "H3")[1]) == 3


def test_committed_seed_meets_c1_and_c2_on_both_layouts_and_left_padded():
    """Forwards only.  Each layout's seed is the first one >= 0 that holds (`R.search_seed`); `R.MARGINS` is what it achieved."""
    assert set(R.BATCH_SEEDS) == set(R.LAYOUTS)
    batch, tot = R.batch_r(R.BATCH_SEEDS["hd64"])
    assert tot >= 4096 and tot % 256 != 0
    assert batch["query"]["input_ids"].shape == (R.NQ, 128) and batch["passage"]["input_ids"].shape == (R.NP, 320)
    left = R.left_padded(batch)
    for side in ("query", "passage"):
        m, lm = batch[side]["attention_mask"], left[side]["attention_mask"]
        assert torch.equal(m.sum(-1), lm.sum(-1)) and bool((lm[:, -1] == 1).all()) and int(lm[:, 0].sum()) < lm.shape[0]
        for i, n in enumerate(m.sum(-1).tolist()):
            assert torch.equal(batch[side]["input_ids"][i, :n], left[side]["input_ids"][i, m.shape[1] - n:])
    conds = {(lay,) + key: c for lay in R.LAYOUTS for key, c in R.seed_conditions(R.BATCH_SEEDS[lay], lay).items()}
    assert set(conds) == {(lay, side, arm) for lay, side in (("hd64", "right"), ("hd64", "left"), ("hd128_g2", "right")) for arm in R.ARMS}
    for key, c in conds.items():
        assert R.conditions_hold(c), (key, c)
        want = R.MARGINS["/".join(key)]
        assert {k: (round(v, 4) if isinstance(v, float) else v) for k, v in c.items()} == want, (key, c, want)
    # the same rows to the left: relative positions only, so the same cosines up to the oracle's float32 rotary angles (HF's:
    # an angle of up to 320 rad carries 320 x 2^-24 = 2e-5 rad of rounding, another one at the shifted position)
    diff = max(abs(conds["hd64", "left", a]["c2"] - conds["hd64", "right", a]["c2"]) for a in R.ARMS)
    print(f"\nC2 margins, left-padded against right-padded: they differ by at most {diff:.2e}")
    assert diff < 1e-4


def test_float64_reference_reaches_every_parameter_on_every_arm():
    """`Oracle64` on a tiny batch: one graph, one backward per arm, every gradient norm > 0 (asserted inside); policy ‖ ref scores
    for the arms with a ref model."""
    from rankpo_amd import encoder as PE
    cfg = U.cfg_s(PE, "hd64")
    pol, ref = U.build_encoder(PE, cfg, seed=0), U.build_encoder(PE, cfg, seed=1)
    rs = np.random.RandomState(3)
    batch = {"query": U.FP._side(rs, 3, 6, 3), "passage": U.FP._side(rs, 6, 9, 4)}
    names = U.param_names(pol)
    o = R.Oracle64(R.bf16_state(pol), R.bf16_state(ref), cfg.to_dict(), batch, names)
    for arm, (knobs, with_ref) in R.ARMS.items():
        loss, scores, grads, metrics = o.step(arm)
        assert scores.shape == (3, 4 if with_ref else 2) and scores.dtype == torch.float64 and sorted(grads) == sorted(names)
        assert o.step(arm) is o.step(arm)
    assert not torch.equal(o.step("H1")[2]["norm.weight"], o.step("H7")[2]["norm.weight"])
    assert torch.equal(o.step("H2")[1][:, 2:], o.ref_scores) and not o.ref_scores.requires_grad


# ------------------------------------------------------------------------------------------------------------------------------
# the keyword arguments of U.rule
# ------------------------------------------------------------------------------------------------------------------------------
KNOBS = R.ARMS["H2"][0]
L, LK = R.lipschitz(KNOBS)


def _ref():
    g = torch.Generator().manual_seed(0)
    scores = (torch.rand(4, 4, generator=g, dtype=torch.float64) - 0.5)
    metrics = {"rankpo_loss": 0.7, "sft_loss": 0.9, "rewards/chosen": 0.3, "rewards/rejected": -0.2, "rewards/accuracies": 0.75,
               "rewards/margins": 0.5, "scores/chosen": 0.15, "scores/rejected": -0.1, "scores/margins": 0.25}
    return (1.25, scores, {n: torch.randn(4, 8, generator=g, dtype=torch.float64) for n in NAMES}), metrics


def _off(ref, rel, seed, cos=0.0, d_loss=0.0):
    """Gradients moved by a relative error `rel`, scores by `cos` in RMS, the loss by `d_loss`."""
    g = torch.Generator().manual_seed(seed)
    grads = {}
    for n, t in ref[2].items():
        e = torch.randn(t.shape, generator=g, dtype=torch.float64)
        grads[n] = (t + rel * t.norm() * e / e.norm())
    e = torch.randn(ref[1].shape, generator=g, dtype=torch.float64)
    return torch.tensor(ref[0] + d_loss, dtype=torch.float64), ref[1] + cos * e / e.pow(2).mean().sqrt(), grads


def _rule(ref, fast, eager, flash, metrics=None, **kw):
    lines = []
    kw = dict(dict(score_scale=1.0, loss_lipschitz=L), **kw)
    if metrics is not None:
        kw.update(metrics=metrics, metric_lipschitz=LK, exact_metrics=R.EXACT_METRICS)
    return U.rule(ref, fast, eager, flash, NAMES, arm="host", out=lines.append, **kw), lines


def test_extended_rule_reports_each_failure_under_its_name():
    ref, mref = _ref()
    eager, flash = _off(ref, 1e-2, 1, cos=1e-3), _off(ref, 1.2e-2, 2, cos=1e-3)
    m = lambda d=0.0, **over: dict({k: v + d for k, v in mref.items()}, **over)
    ms = lambda fast: (mref, fast, m(1e-4, **{"rewards/accuracies": 0.75}), m(-1e-4, **{"rewards/accuracies": 0.75}))
    ok = _off(ref, 1e-2, 3, cos=1e-3)
    fails, lines = _rule(ref, ok, eager, flash, ms(m()))
    assert fails == [] and len(lines) == 1 and lines[0].startswith("| host | ")
    # a tensor over its bound; a missing tensor
    bad = _off(ref, 1e-2, 3, cos=1e-3)
    bad[2]["b.weight"] = _off(ref, 2e-2, 4)[2]["b.weight"]
    fails, lines = _rule(ref, bad, eager, flash, ms(m()))
    assert [(r["kind"], r["name"]) for r in fails] == [("grad", "b.weight")] and any("FAIL" in x and "b.weight" in x for x in lines)
    del bad[2]["b.weight"]
    assert [(r["kind"], r["name"]) for r in _rule(ref, bad, eager, flash, ms(m()))[0]] == [("missing", "b.weight")]
    # the guard: only the stock-flash control is off
    fl = _off(ref, 1.2e-2, 2, cos=1e-3)
    fl[2]["c.weight"] = _off(ref, 8e-2, 5)[2]["c.weight"]
    assert [(r["kind"], r["name"]) for r in _rule(ref, ok, eager, fl, ms(m()))[0]] == [("guard", "c.weight")]
    # the loss: 1.5 x max(control loss error, L x control cosine RMS error) + 5e-6 L, with L = 50 here, not 1 / T
    assert L == pytest.approx(50.0)
    for d_loss, want in ((1.4 * L * 1e-3, []), (1.6 * L * 1e-3 + 5e-6 * L, ["loss_abs_err"])):
        fails, _ = _rule(ref, _off(ref, 1e-2, 3, cos=1e-3, d_loss=d_loss), eager, flash, ms(m()))
        assert U.failed_names(fails) == want and all(r["kind"] == "stat" for r in fails), fails
    # ... and the controls' own loss error widens it
    e2 = _off(ref, 1e-2, 1, cos=1e-3, d_loss=0.2)
    assert _rule(ref, _off(ref, 1e-2, 3, cos=1e-3, d_loss=0.29), e2, flash, ms(m()))[0] == []
    # scores are cosines: no x T
    fails, _ = _rule(ref, _off(ref, 1e-2, 3, cos=2e-3), eager, flash, ms(m()))
    assert U.failed_names(fails, "stat") == ["cos_max_err", "cos_rms_err"]
    assert U.errors(ok, ref, NAMES, score_scale=1.0)["cos_rms_err"] == pytest.approx(1e-3)
    assert U.errors(ok, ref, NAMES)["cos_rms_err"] == pytest.approx(1e-3 * U.T_CONTRASTIVE)
    # a metric over its bound (rewards/margins: 1.5 x max(1e-4, 4 x 1e-3) + 2e-5 = 6.02e-3), one inside it
    assert _rule(ref, ok, eager, flash, ms(m(**{"rewards/margins": mref["rewards/margins"] + 5.9e-3})))[0] == []
    fails, lines = _rule(ref, ok, eager, flash, ms(m(**{"rewards/margins": mref["rewards/margins"] + 6.1e-3})))
    assert [(r["kind"], r["name"]) for r in fails] == [("metric", "rewards/margins")] and any("rewards/margins" in x for x in lines)
    # a flipped accuracy: exact, whatever the controls say
    fails, _ = _rule(ref, ok, eager, flash, ms(m(**{"rewards/accuracies": 0.5})))
    assert [(r["kind"], r["name"]) for r in fails] == [("metric", "rewards/accuracies")]
    # a metric the fast path lacks, or has beyond the reference's
    lacking = m()
    del lacking["sft_loss"]
    assert [(r["kind"], r["name"]) for r in _rule(ref, ok, eager, flash, ms(lacking))[0]] == [("metric", "sft_loss")]
    assert [(r["kind"], r["name"]) for r in _rule(ref, ok, eager, flash, ms(m(extra=1.0)))[0]] == [("metric", "extra")]
    # without a stock-flash control the eager one alone sets every bound
    assert _rule(ref, ok, eager, None, (mref, m(), m(1e-4, **{"rewards/accuracies": 0.75}), None))[0] == []


def test_old_signature_returns_what_it_returned():
    """The keyword arguments left at their defaults: the InfoNCE statistics (scores x T, loss against cosine RMS / T)."""
    ref, _ = _ref()
    T = U.T_CONTRASTIVE
    eager, flash = _off(ref, 1e-2, 1, cos=1e-3 / T), _off(ref, 1.2e-2, 2, cos=1e-3 / T)
    lines = []
    fast = _off(ref, 1e-2, 3, cos=1e-3 / T, d_loss=1.4 * 1e-3 / T)
    assert U.rule(ref, fast, eager, flash, NAMES, arm="old", out=lines.append) == []
    fast = _off(ref, 1e-2, 3, cos=1e-3 / T, d_loss=1.6 * 1e-3 / T + 5e-6 / T)
    fails = U.rule(ref, fast, eager, flash, NAMES, arm="old", out=lines.append)
    assert [(r["kind"], r["name"], r["bound"]) for r in fails] == [("stat", "loss_abs_err", fails[0]["bound"])]
    e = max(U.errors(c, ref, NAMES)["cos_rms_err"] for c in (eager, flash))
    assert fails[0]["bound"] == 1.5 * max(0.0, e / T) + 5e-6 / T                       # the expression as it was, to the bit
