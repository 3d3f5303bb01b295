"""Every weight gradient of a RankPO training step (`RankPOTrainer.get_batch_loss_metrics` on a packed bf16 Llama policy, with and
without a ref model) against float64, per head arm: the head in plain torch, the case, its float64 reference, its two controls and
the conditions that make the comparison a measurement and not a coin toss.

The rule is tests/llama_step_parity_util.py's (`U.rule`: per tensor 1.5 x the larger control + 1e-4, guard 2.5 x + 1e-5, over all
of `named_parameters()`), with the two statistics that need the head's scale handed over as keyword arguments:

  scores   RankPO scores are unscaled cosines: `score_scale=1.0`.  With a ref model the step's "scores" are policy ‖ ref, [B, 4]:
           the ref leg's rows are judged like the policy's, and the controls' cosine error is the RMS over both.
  loss     |d loss| <= L * cosine RMS error, L = 2 (rankpo_weight * beta + sft_weight) / T (`lipschitz`): |d l / d adv| <= beta / T
           for the sigmoid (label smoothing included) and the hinge loss, the cross entropy over two scores / T has a gradient
           <= 1 / T per score, and the mean over B rows of |dc| + |dr| is <= 2 x the RMS over the 2B scores.
  metrics  the same form per metric with its own constant (beta for rewards/*, 2 beta for rewards/margins, 1 for scores/*, 2 for
           scores/margins, 2 beta / T for rankpo_loss, 2 / T for sft_loss); rewards/accuracies is compared exactly.

reference  float64 on the host: the policy's `E.embed(..., force_last=True)` graph is built once per (layout, batch) and kept, the
           ref encoder's scores come from a no-grad float64 forward, and every head arm is `rankpo_head` in float64 on that
           graph followed by `torch.autograd.grad(..., retain_graph=True)`; every gradient norm is asserted > 0.
controls   both in bf16 on the device, `step_parity`'s two: (i) the oracle's eager `E.embed` on the policy's and on the ref's
           weights, unit rows taken `.float()` into `rankpo_head` in float32; (ii) the same `RankPOTrainer` call as the fast path
           with `hand_attention = False` on both encoders.  The product head keeps f32 dots and has f64 parity tests of its own, so
           the controls differ from the fast path in the encoder arithmetic and every head or glue error counts against the fast
           path.

Head arms (`ARMS`): beta / T <= 20 everywhere -- a sharper head turns the bf16 score noise into O(1) changes of single rows'
weights, in all three paths alike --; saturation is reached through gamma and the ref scores.  Conditions, on the float64
reference alone (`conditions`; asserted on the host by tests/test_rankpo_step_parity_host.py and again on the device):

  C1  hinge arms: min over rows of |1 - beta z| >= 0.25, at least 2 rows active and 2 inactive;
  C2  every arm: min over rows of |chosen reward - rejected reward| / beta >= 0.02 (cosine units);
  C3  (needs the device, `c3`): (2 beta / T) * the cosine max error of control (i), policy and ref together, <= 0.1; the C1
      margin >= 4 x that, the C2 margin >= 4 x that cosine max error.

`BATCH_SEEDS[layout]` is the first seed >= 0 at which C1 and C2 hold for every arm on that layout (on hd64: and on the
left-padded batch; `search_seed`, float64 forwards on the host); `MARGINS` records what each achieved.  One seed per layout, not
one for both: the advantages of these random models cluster around 0 (standard deviation about 0.15), so a row misses C2 with
probability about 0.1 and a hinge row its kink band about as often.  Every seed of 0-1005 was looked at: 21 meet every
condition on hd64 (the first is 65), none of the 21 meets them on hd128_g2 as well (whose first is 7).  Every arm of every layout
meets every condition on the batch it runs on.

Importable without a GPU."""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import torch

import llama_step_parity_util as U
from oracle import encoder_ref as E

FP = U.FP
LAYOUTS = ("hd64", "hd128_g2")
NQ, NP = 8, 16                                       # 8 queries, chosen ‖ rejected per query
C1_MIN, C2_MIN, C3_CAP, C3_SAFETY = 0.25, 0.02, 0.1, 4.0
HEAD_DEFAULTS = dict(beta=0.1, temperature=1.0, gamma_beta_ratio=0.0, sft_weight=0.0, rankpo_weight=1.0, loss_type="sigmoid",
                     label_smoothing=0.0, reference_free=False)          # RankPOTrainer's own defaults
METRIC_KEYS = ("rankpo_loss", "sft_loss", "rewards/chosen", "rewards/rejected", "rewards/accuracies", "rewards/margins",
               "scores/chosen", "scores/rejected", "scores/margins")
EXACT_METRICS = ("rewards/accuracies",)

# name -> (knobs, with a ref model)
ARMS = {
    "H1": (dict(reference_free=True, beta=2.0, temperature=0.1), False),                       # the bench's and smoke()'s head
    "H2": (dict(beta=2.0, temperature=0.1, sft_weight=0.5, label_smoothing=0.1, gamma_beta_ratio=0.25, reference_free=False), True),
    "H3": (dict(loss_type="hinge", reference_free=True, beta=1.0, temperature=0.1), False),
    "H4": (dict(loss_type="hinge", reference_free=False, beta=1.0, temperature=0.1), True),
    "H5": (dict(rankpo_weight=0.0, sft_weight=1.0, temperature=0.1), False),
    "H6": (dict(reference_free=True, beta=2.0, temperature=0.1, gamma_beta_ratio=-3.0), False),  # every row in the flat tail
    "H7": (dict(reference_free=True, beta=2.0, temperature=0.1, gamma_beta_ratio=3.0), False),   # every row on the linear side
    "H8": (dict(reference_free=True, beta=2.0, temperature=0.1), True),                          # ref given, used by rewards/* only
}
ARM_TITLES = {"H1": "free-sigmoid", "H2": "ref-sigmoid-sft", "H3": "free-hinge", "H4": "ref-hinge", "H5": "sft-only",
              "H6": "saturated", "H7": "steep", "H8": "ref given, reference_free"}

BATCH_SEEDS = {"hd64": 65, "hd128_g2": 7}           # see `search_seed`; MARGINS: what the float64 reference gives at these seeds
MARGINS = {                                          # "layout/right | left/arm": conditions(...) rounded to 4 places
    "hd64/right/H1": {"c2": 0.0357},
    "hd64/right/H2": {"c2": 0.0542},
    "hd64/right/H3": {"c2": 0.0357, "c1": 0.6414, "active": 6, "inactive": 2},
    "hd64/right/H4": {"c2": 0.0542, "c1": 0.3243, "active": 5, "inactive": 3},
    "hd64/right/H5": {"c2": 0.0357},
    "hd64/right/H6": {"c2": 0.0357},
    "hd64/right/H7": {"c2": 0.0357},
    "hd64/right/H8": {"c2": 0.0542},
    "hd64/left/H1": {"c2": 0.0357},
    "hd64/left/H2": {"c2": 0.0542},
    "hd64/left/H3": {"c2": 0.0357, "c1": 0.6414, "active": 6, "inactive": 2},
    "hd64/left/H4": {"c2": 0.0542, "c1": 0.3243, "active": 5, "inactive": 3},
    "hd64/left/H5": {"c2": 0.0357},
    "hd64/left/H6": {"c2": 0.0357},
    "hd64/left/H7": {"c2": 0.0357},
    "hd64/left/H8": {"c2": 0.0542},
    "hd128_g2/right/H1": {"c2": 0.0282},
    "hd128_g2/right/H2": {"c2": 0.1289},
    "hd128_g2/right/H3": {"c2": 0.0282, "c1": 0.3178, "active": 6, "inactive": 2},
    "hd128_g2/right/H4": {"c2": 0.1289, "c1": 0.3335, "active": 4, "inactive": 4},
    "hd128_g2/right/H5": {"c2": 0.0282},
    "hd128_g2/right/H6": {"c2": 0.0282},
    "hd128_g2/right/H7": {"c2": 0.0282},
    "hd128_g2/right/H8": {"c2": 0.1289},
}


def knobs_of(arm):
    return dict(HEAD_DEFAULTS, **ARMS[arm][0])


# ------------------------------------------------------------------------------------------------------------------------------
# the head in plain torch
# ------------------------------------------------------------------------------------------------------------------------------
def rankpo_head(q, p, ref_c, ref_r, knobs):
    """`get_batch_loss_metrics` of the reference on given unit rows (rankpo_trainer.py:458-520), differentiable, in the dtype of
    `q`: q [B, d], p [2B, d] (chosen, rejected per query), ref_c / ref_r [B] or None (no ref model: 0, :467).  Returns (loss,
    scores [B, 2], {metric: 0-dim tensor}); the metrics dict has the keys the reference builds (:496-520)."""
    k = dict(HEAD_DEFAULTS, **knobs)
    beta, T = k["beta"], k["temperature"]
    B = q.shape[0]
    assert p.shape[0] == 2 * B, (q.shape, p.shape)
    scores = torch.einsum("bd,bgd->bg", q, p.view(B, 2, -1))                                # :436-443, unscaled
    c, r = scores[:, 0], scores[:, 1]
    rc = torch.zeros_like(c) if ref_c is None else ref_c.to(c.dtype)
    rr = torch.zeros_like(r) if ref_r is None else ref_r.to(r.dtype)
    loss, metrics = 0.0, {}
    if k["rankpo_weight"] > 0.0:                                                            # :485-496
        adv = c - r                                                                         # :545
        if not k["reference_free"]:
            adv = adv - (rc - rr)                                                           # :546-548
        z = adv / T - k["gamma_beta_ratio"]                                                 # :550-554
        if k["loss_type"] == "sigmoid":
            ls = k["label_smoothing"]
            losses = -torch.nn.functional.logsigmoid(beta * z) * (1 - ls) - torch.nn.functional.logsigmoid(-beta * z) * ls
        elif k["loss_type"] == "hinge":
            losses = torch.relu(1 - beta * z)
        else:
            raise ValueError(f"Unknown loss type: {k['loss_type']}. Should be one of ['sigmoid', 'hinge']")
        metrics["rankpo_loss"] = losses.mean()
        loss = loss + k["rankpo_weight"] * metrics["rankpo_loss"]
    if k["sft_weight"] > 0.0:                                                               # :499-505
        ts = scores / T
        metrics["sft_loss"] = (torch.logsumexp(ts, -1) - ts[:, 0]).mean()
        loss = loss + k["sft_weight"] * metrics["sft_loss"]
    cr, rw = beta * (c - rc), beta * (r - rr)                                               # :509-510
    metrics["rewards/chosen"], metrics["rewards/rejected"] = cr.mean(), rw.mean()
    metrics["rewards/accuracies"] = (cr > rw).to(c.dtype).mean()
    metrics["rewards/margins"] = (cr - rw).mean()
    metrics["scores/chosen"], metrics["scores/rejected"], metrics["scores/margins"] = c.mean(), r.mean(), (c - r).mean()
    return loss, scores, {key: v.detach() for key, v in metrics.items()}


def lipschitz(knobs):
    """(L of the loss, {metric: L_k}) in the cosines; see the module docstring."""
    k = dict(HEAD_DEFAULTS, **knobs)
    beta, T = k["beta"], k["temperature"]
    lk = {"rewards/chosen": beta, "rewards/rejected": beta, "rewards/margins": 2 * beta, "scores/chosen": 1.0,
          "scores/rejected": 1.0, "scores/margins": 2.0}
    if k["rankpo_weight"] > 0.0:
        lk["rankpo_loss"] = 2 * beta / T
    if k["sft_weight"] > 0.0:
        lk["sft_loss"] = 2 / T
    return 2 * (max(k["rankpo_weight"], 0.0) * beta + max(k["sft_weight"], 0.0)) / T, lk


# ------------------------------------------------------------------------------------------------------------------------------
# the conditions, from float64 scores alone
# ------------------------------------------------------------------------------------------------------------------------------
def conditions(scores, ref_scores, arm):
    """C1 / C2 margins of one arm from the float64 policy scores [B, 2] and ref scores [B, 2] (ignored by an arm without a ref
    model): dict(c2=..., c1=... / active / inactive for a hinge arm)."""
    k, with_ref = knobs_of(arm), ARMS[arm][1]
    adv = (scores[:, 0] - scores[:, 1]).double()
    radv = (ref_scores[:, 0] - ref_scores[:, 1]).double() if with_ref else torch.zeros_like(adv)
    out = {"c2": float((adv - radv).abs().min())}               # (beta (c - rc) - beta (r - rr)) / beta
    if k["loss_type"] == "hinge":
        z = (adv - (0 if k["reference_free"] else radv)) / k["temperature"] - k["gamma_beta_ratio"]
        h = 1 - k["beta"] * z
        out.update(c1=float(h.abs().min()), active=int((h > 0).sum()), inactive=int((h <= 0).sum()))
    return out


def conditions_hold(cond):
    return cond["c2"] >= C2_MIN and ("c1" not in cond or (cond["c1"] >= C1_MIN and cond["active"] >= 2 and cond["inactive"] >= 2))


def c3(cond, cos_max_err, arm):
    """C3 for one arm from the measured cosine max error of control (i): (amplification, [what does not hold])."""
    k = knobs_of(arm)
    amp = 2 * k["beta"] / k["temperature"] * cos_max_err
    bad = []
    if not amp <= C3_CAP:
        bad.append(f"(2 beta / T) cos_max_err = {amp:.3e} > {C3_CAP}")
    if "c1" in cond and not cond["c1"] >= C3_SAFETY * amp:
        bad.append(f"C1 margin {cond['c1']:.3e} < 4 x {amp:.3e}")
    if not cond["c2"] >= C3_SAFETY * cos_max_err:
        bad.append(f"C2 margin {cond['c2']:.3e} < 4 x {cos_max_err:.3e}")
    return amp, bad


# ------------------------------------------------------------------------------------------------------------------------------
# the batch
# ------------------------------------------------------------------------------------------------------------------------------
def batch_r(seed):
    """8 queries of 64-128 tokens + 16 passages of 160-320 tokens (chosen ‖ rejected per query): >= 4096 packed tokens, not a
    multiple of 256."""
    rs = np.random.RandomState(seed)
    b = {"query": FP._side(rs, NQ, 128, 64), "passage": FP._side(rs, NP, 320, 160)}
    return U._off_256(b)


def left_padded(batch):
    """The same rows, every one moved to the right end of its width: column 0 is a pad token for every row but the longest."""
    out = {}
    for side, d in batch.items():
        ids, m = d["input_ids"], d["attention_mask"]
        L = m.shape[1]
        nid, nm = torch.zeros_like(ids), torch.zeros_like(m)
        for i, n in enumerate(m.sum(-1).tolist()):
            nid[i, L - n:], nm[i, L - n:] = ids[i, :n], 1
        out[side] = {"input_ids": nid, "attention_mask": nm}
    return out


def bf16_state(enc):
    """The values a bf16 copy of `enc` holds, on the host."""
    return {k: v.detach().to("cpu", torch.bfloat16) for k, v in enc.state_dict().items()}


def embed_pair(w, cd, batch, dtype):
    return (E.embed(w, cd, batch["query"], dtype=dtype, force_last=True), E.embed(w, cd, batch["passage"], dtype=dtype, force_last=True))


def scores_of(q, p):
    return torch.einsum("bd,bgd->bg", q, p.view(q.shape[0], 2, -1))


@functools.lru_cache(maxsize=None)
def host_encoders(layout):
    """(cfg, the policy's bf16-held weights, the ref model's) on the host: seeds 0 and 1 of `U.build_encoder`."""
    from rankpo_amd import encoder as PE
    cfg = U.cfg_s(PE, layout)
    return cfg, bf16_state(U.build_encoder(PE, cfg, seed=0)), bf16_state(U.build_encoder(PE, cfg, seed=1))


def scores64(layout, batch):
    """Float64 policy and ref scores of `batch`, forwards only."""
    cfg, pol, ref = host_encoders(layout)
    with torch.no_grad():
        return tuple(scores_of(*embed_pair({k: v.double() for k, v in sd.items()}, cfg.to_dict(), batch, torch.float64))
                     for sd in (pol, ref))


def seed_conditions(seed, layout, left=None):
    """{("right" | "left", arm): conditions} of one batch seed on one layout, from float64 forwards of both encoders; `left`:
    the left-padded batch too (default: where a test runs it, on hd64)."""
    out = {}
    batch, tot = batch_r(seed)
    assert tot >= 4096 and tot % 256 != 0, tot
    for side, b in (("right", batch),) + ((("left", left_padded(batch)),) if (layout == "hd64" if left is None else left) else ()):
        s, rs = scores64(layout, b)
        for arm in ARMS:
            out[side, arm] = conditions(s, rs, arm)
    return out


def search_seed(layout, start=0, stop=100000, out=print):
    """The first seed >= `start` at which C1 and C2 hold for every arm on `layout` (and on its left-padded batch)."""
    for seed in range(start, stop):
        conds = seed_conditions(seed, layout)
        bad = [key for key, c in conds.items() if not conditions_hold(c)]
        out(f"{layout} seed {seed}: {'holds' if not bad else 'misses ' + str(bad[:3])}")
        if not bad:
            return seed, conds
    raise RuntimeError("no seed found")


# ------------------------------------------------------------------------------------------------------------------------------
# float64 reference: one graph per (weights, batch), one backward per head arm
# ------------------------------------------------------------------------------------------------------------------------------
class Oracle64:
    def __init__(self, pol_sd, ref_sd, cd, batch, names, arms=ARMS, dtype=torch.float64):
        self.names, self.arms, self.steps = names, arms, {}
        self.w = {k: v.detach().to("cpu", dtype).requires_grad_(True) for k, v in pol_sd.items()}
        self.q, self.p = embed_pair(self.w, cd, batch, dtype)
        self.scores = scores_of(self.q, self.p).detach()
        with torch.no_grad():
            self.ref_scores = scores_of(*embed_pair({k: v.detach().to("cpu", dtype) for k, v in ref_sd.items()}, cd, batch, dtype))

    def step(self, arm):
        """(loss, scores [B, 2] or policy ‖ ref [B, 4], {name: grad}, {metric: float}) of one head arm."""
        if arm not in self.steps:
            knobs, with_ref = self.arms[arm]
            rc, rr = (self.ref_scores[:, 0], self.ref_scores[:, 1]) if with_ref else (None, None)
            loss, scores, metrics = rankpo_head(self.q, self.p, rc, rr, knobs)
            got = torch.autograd.grad(loss, [self.w[n] for n in self.names], retain_graph=True, allow_unused=True)
            for n, g in zip(self.names, got):
                assert g is not None and float(g.norm()) > 0, f"float64 reference, arm {arm}: no gradient reaches {n}"
            self.steps[arm] = (float(loss.detach()), _cat(scores.detach(), self.ref_scores if with_ref else None),
                               {n: g.detach() for n, g in zip(self.names, got)}, {k: float(v) for k, v in metrics.items()})
        return self.steps[arm]

    def conditions(self, arm):
        return conditions(self.scores, self.ref_scores, arm)


def _cat(scores, ref_scores):
    return scores if ref_scores is None else torch.cat([scores, ref_scores.to(scores.dtype)], 1)


# ------------------------------------------------------------------------------------------------------------------------------
# the device side: fast path and the two controls
# ------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def head_calls():
    """Records every `ops.rankpo_loss_metrics` call while it is open: (ref_chosen, ref_rejected, scores returned)."""
    from rankpo_amd import ops
    real, calls = ops.rankpo_loss_metrics, []

    def spy(q, p, cfg, ref_chosen=None, ref_rejected=None):
        out = real(q, p, cfg, ref_chosen, ref_rejected)
        calls.append((ref_chosen, ref_rejected, out[1]))
        return out
    ops.rankpo_loss_metrics = spy
    try:
        yield calls
    finally:
        ops.rankpo_loss_metrics = real


def trainer_step(pol, ref, knobs, dev_batch, names, call="get_batch_loss_metrics"):
    """One RankPO step of the product: (loss, scores [B, 2] or policy ‖ ref [B, 4], {name: grad}, {metric: float}).  The scores
    are what the head returned inside the step; the .grad buffers stay untouched."""
    import rankpo_amd
    tr = rankpo_amd.RankPOTrainer(pol, ref, **knobs)
    params = dict(pol.named_parameters())
    with head_calls() as calls:
        loss, handle = tr.get_batch_loss_metrics(pol, dev_batch, sync_metrics=False)
        got = torch.autograd.grad(loss, [params[n] for n in names], allow_unused=True)
    assert len(calls) == (2 if ref is not None else 1), len(calls)
    ref_scores = calls[0][2].detach() if ref is not None else None
    return loss.detach(), _cat(calls[-1][2].detach().float(), ref_scores), dict(zip(names, got)), tr.resolve_metrics(handle)


@contextlib.contextmanager
def stock_flash(*encoders):
    for e in encoders:
        assert e.hand_attention
        e.hand_attention = False
    try:
        yield
    finally:
        for e in encoders:
            e.hand_attention = True


class Eager:
    """Control (i): the oracle's eager code in bf16 on the device; one graph, one backward per head arm."""

    def __init__(self, pol, ref, cd, dev_batch, names, arms=ARMS, dtype=torch.bfloat16):
        self.names, self.arms, self.steps = names, arms, {}
        dev = next(pol.parameters()).device
        self.w = {k: v.detach().to(dev, dtype).requires_grad_(True) for k, v in pol.state_dict().items()}
        q, p = embed_pair(self.w, cd, dev_batch, dtype)
        self.q, self.p = q.float(), p.float()
        with torch.no_grad():
            rq, rp = embed_pair({k: v.detach().to(dev, dtype) for k, v in ref.state_dict().items()}, cd, dev_batch, dtype)
            self.ref_scores = scores_of(rq.float(), rp.float())

    def step(self, arm):
        if arm not in self.steps:
            knobs, with_ref = self.arms[arm]
            rc, rr = (self.ref_scores[:, 0], self.ref_scores[:, 1]) if with_ref else (None, None)
            loss, scores, metrics = rankpo_head(self.q, self.p, rc, rr, knobs)
            got = torch.autograd.grad(loss, [self.w[n] for n in self.names], retain_graph=True, allow_unused=True)
            self.steps[arm] = (loss.detach(), _cat(scores.detach(), self.ref_scores if with_ref else None),
                               dict(zip(self.names, got)), {k: float(v) for k, v in metrics.items()})
        return self.steps[arm]


def make_case(layout, batch, tot, device="cuda:0", flash_control=True):
    from rankpo_amd import encoder as PE
    cfg = U.cfg_s(PE, layout)
    pol = U.build_encoder(PE, cfg, seed=0).to(device).to(torch.bfloat16)
    ref = U.build_encoder(PE, cfg, seed=1).to(device).to(torch.bfloat16)       # this case's own instance: the trainer freezes it
    names = U.param_names(pol)
    assert set(names) == set(pol.state_dict())
    dev_batch = U.to_device(batch, device)
    c = SimpleNamespace(layout=layout, cfg=cfg, pol=pol, ref=ref, names=names, batch=batch, dev_batch=dev_batch, tot=tot,
                        padded=(tot + 255) // 256 * 256, flash_control=flash_control, flash_steps={},
                        oracle=Oracle64(pol.state_dict(), ref.state_dict(), cfg.to_dict(), batch, names),
                        eager=Eager(pol, ref, cfg.to_dict(), dev_batch, names))
    return c


def flash_step(c, arm):
    """Control (ii): the same trainer call with PyTorch's flash-attention ops in both encoders; None where the path under test
    never consults `hand_attention` (the padded path)."""
    if not c.flash_control:
        return None
    if arm not in c.flash_steps:
        knobs, with_ref = ARMS[arm]
        with stock_flash(c.pol, c.ref):
            c.flash_steps[arm] = trainer_step(c.pol, c.ref if with_ref else None, knobs, c.dev_batch, c.names)
    return c.flash_steps[arm]


def fast_step(c, arm):
    knobs, with_ref = ARMS[arm]
    return trainer_step(c.pol, c.ref if with_ref else None, knobs, c.dev_batch, c.names)


def judge(c, arm, fast, name=None, out=print):
    """C3, then `U.rule` with the head's scales over every parameter, the loss, the scores and the metrics: (fails, C3 record)."""
    ref, eager, flash = c.oracle.step(arm), c.eager.step(arm), flash_step(c, arm)
    cond = c.oracle.conditions(arm)
    assert conditions_hold(cond), (arm, cond)
    cm = U.errors(eager[:3], ref[:3], c.names, score_scale=1.0)["cos_max_err"]
    amp, bad = c3(cond, cm, arm)
    out(f"C3 [{arm} {c.layout}]: control (i) cos_max_err {cm:.3e}, (2 beta / T) x that {amp:.3e}, C1 {cond.get('c1')}, C2 {cond['c2']:.4f}")
    assert not bad, f"arm {arm}: C3 does not hold on this device: {bad}"
    L, lk = lipschitz(ARMS[arm][0])
    fails = U.rule(ref[:3], fast[:3], eager[:3], None if flash is None else flash[:3], c.names, arm=name or f"{arm} {ARM_TITLES[arm]} {c.layout}",
                   score_scale=1.0, loss_lipschitz=L, metrics=(ref[3], fast[3], eager[3], None if flash is None else flash[3]),
                   metric_lipschitz=lk, exact_metrics=EXACT_METRICS, out=out)
    return fails, dict(cos_max_err=cm, amp=amp, **cond)


@functools.lru_cache(maxsize=None)
def case_r(layout="hd64"):
    batch, tot = batch_r(BATCH_SEEDS[layout])
    assert tot >= 4096 and tot % 256 != 0, tot
    return make_case(layout, batch, tot)


@functools.lru_cache(maxsize=None)
def case_left(layout="hd64"):
    """The left-padded variant of the same rows: a reference and a control (i) of its own; the padded path never consults
    `hand_attention`, so there is no control (ii)."""
    batch, tot = batch_r(BATCH_SEEDS[layout])
    return make_case(layout, left_padded(batch), tot, flash_control=False)
