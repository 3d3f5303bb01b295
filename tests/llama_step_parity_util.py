"""Every weight gradient of the bf16 packed Llama training step against a float64 oracle: the rule, its reference and controls.

`bench_parity.step_parity` judges a step by its loss, its scores and THREE weight gradients (`PARITY_GRADS`).  A weight gradient
feeds nothing downstream, so a wrong dW of a down, gate|up, o or v projection, a wrong RMSNorm weight gradient or a wrong gradient
of anything the last block computes on the pooled rows is invisible to it.  This module applies the same rule to EVERY entry of
`model.model.named_parameters()`:

  reference  oracle/encoder_ref.py's `contrastive_step` in float64 on the bf16-held weights, with its backward (`oracle64`);
  controls   the same step in bf16 on the device through (i) the oracle's eager code and (ii) the product's encoder with PyTorch's
             flash-attention ops (`hand_attention = False`): exactly the two controls of `step_parity`;
  statistic  per tensor, the relative Frobenius error against float64; for loss and scores what `step_parity` computes;
  bound      err_fast <= 1.5 * max(err_eager, err_flash) + 1e-4 per tensor (cosines: + 5e-6; loss: 1.5 * max(control loss error,
             control cosine RMS error / T) + 5e-6 / T);
  guard      err_flash <= 2.5 * err_eager + 1e-5 per tensor and cosine statistic: the stock-flash control runs the product's own
             glue, a glue defect inflates it together with the fast path, and only this comparison with the oracle's own code
             sees that.

1.5, 2.5, 1e-4 and 1e-5 are `step_parity`'s numbers.  `rule` returns the list of failures (tensor name and all three errors) and
prints the worst tensor of the arm as a table row.  The RMSNorm weights are moved off 1.0 before the bf16 cast, so that their
gradients (and the gradients through them) are not the special case of a unit weight; `oracle64` asserts that every parameter has a
non-zero float64 gradient.

Importable without a GPU (tests/test_llama_step_parity_host.py runs the rule on hand-made dicts)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import test_gpu_fastpath as FP                      # _cfg, _side, _batch: the batch and config of the bench-path gate
from oracle import encoder_ref as E

T_CONTRASTIVE = FP.T_CONTRASTIVE
FACTOR, GRAD_FLOOR, COS_FLOOR = 1.5, 1e-4, 5e-6     # bench_parity.step_parity's bound
GUARD, GUARD_FLOOR = 2.5, 1e-5                      # ... and its guard
NORM_JITTER = 0.05

# head layouts of config S (d 512 -- 384 for the group of three --, ff 1024, 4 blocks, llama3 rope): hd, q heads, kv heads, d
LAYOUTS_S = {"hd64": (64, 8, 2, 512), "hd128_g4": (128, 4, 1, 512), "hd128_g2": (128, 4, 2, 512),
             "g1": (128, 4, 4, 512), "g8": (64, 8, 1, 512), "g3": (64, 6, 2, 384)}


def cfg_s(PE, layout="hd64"):
    """Config S.  "hd64" and "hd128_g2" are `test_gpu_fastpath._cfg(PE, 64 / 128)` field for field."""
    hd, nh, nkv, d = LAYOUTS_S[layout]
    if (nkv, d) == (2, 512):
        return FP._cfg(PE, hd)
    return PE.llama_config(vocab_size=2048, hidden_size=d, intermediate_size=1024, num_hidden_layers=4, num_attention_heads=nh,
                           num_key_value_heads=nkv, head_dim=hd, pad_token_id=0,
                           rope_scaling=dict(PE.LLAMA3_ROPE, original_max_position_embeddings=128))


def cfg_l(PE):
    """Config L: the smallest model whose q|k|v (384 x 256) and o (256 x 256) weight gradients take `ops.wgrad`'s split-T branch
    (neither operand twice the other) once the packed batch has >= 32768 tokens."""
    return PE.llama_config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4,
                           num_key_value_heads=1, head_dim=64, pad_token_id=0,
                           rope_scaling=dict(PE.LLAMA3_ROPE, original_max_position_embeddings=128))


def batch_s(seed=2026):
    """`test_gpu_fastpath._batch()` (seed 2026: that very batch): 6 + 18 rows, >= 4096 packed tokens, not a multiple of 256."""
    if seed == 2026:
        return FP._batch()
    rs = np.random.RandomState(seed)
    b = {"query": FP._side(rs, 6, 128, 64), "passage": FP._side(rs, 18, 320, 160)}
    return _off_256(b)


def batch_l(seed=31):
    """4 queries of <= 512 tokens + 12 passages of 2816-3072 tokens, vocab 512: >= 32768 packed tokens."""
    rs = np.random.RandomState(seed)
    b = {"query": FP._side(rs, 4, 512, 256, 512), "passage": FP._side(rs, 12, 3072, 2816, 512)}
    return _off_256(b)


def batch_tiny(seed=5, vocab=512):
    """2 queries + 4 passages of a few tokens (the host test)."""
    rs = np.random.RandomState(seed)
    return {"query": FP._side(rs, 2, 6, 3, vocab), "passage": FP._side(rs, 4, 9, 4, vocab)}


def _off_256(b):
    tot = int(b["query"]["attention_mask"].sum() + b["passage"]["attention_mask"].sum())
    if tot % 256 == 0:                               # the filler must have something to do: drop row 1's last token
        m = b["query"]["attention_mask"]
        last = int(m[1].sum()) - 1
        m[1, last] = 0
        b["query"]["input_ids"][1, last] = 0
        tot -= 1
    return b, tot


def build_encoder(PE, cfg, seed=0):
    """A float32 LlamaEncoder on the host with every RMSNorm weight moved off 1.0 by 0.05 * randn (BEFORE any cast to bf16)."""
    torch.manual_seed(seed)
    enc = PE.LlamaEncoder(cfg)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for n, p in enc.named_parameters():
            if n.endswith("norm.weight") or n.endswith("layernorm.weight"):
                p.add_(NORM_JITTER * torch.randn(p.shape, generator=g))
    return enc


def build_model(PE, rankpo_amd, cfg, seed=0, device="cuda:0"):
    enc = build_encoder(PE, cfg, seed).to(device).to(torch.bfloat16)
    return enc, rankpo_amd.ModelForTraining(encoder=enc, temperature=T_CONTRASTIVE).train()


def param_names(enc):
    """The names every check iterates: exactly `named_parameters()` of the encoder, in its order."""
    return [n for n, _ in enc.named_parameters()]


def to_device(batch, device):
    return {k: {kk: vv.to(device) for kk, vv in v.items()} for k, v in batch.items()}


def oracle64(sd, cd, batch, temperature=T_CONTRASTIVE, device="cpu", block_checkpoint=False):
    """The float64 step of the oracle on the weights `sd` holds (their values as they are, e.g. bf16-rounded): (loss, scores,
    {name: grad}) on the host in float64, for EVERY key of `sd`; every gradient norm is asserted > 0."""
    w = {k: v.detach().to(device, torch.float64).requires_grad_(True) for k, v in sd.items()}
    loss, scores = E.contrastive_step(w, cd, to_device(batch, device), temperature, dtype=torch.float64,
                                      block_checkpoint=block_checkpoint)[:2]
    loss.backward()
    grads = {}
    for k, t in w.items():
        assert t.grad is not None and float(t.grad.norm()) > 0, f"float64 oracle: no gradient reaches {k}"
        grads[k] = t.grad.detach().cpu()
    return float(loss.detach()), scores.detach().cpu(), grads


def product_step(model, dev_batch, names):
    """One forward and backward of ModelForTraining: (loss, scores, {name: grad}); the .grad buffers stay untouched, a parameter
    no gradient reaches comes back as None."""
    params = dict(model.model.named_parameters())
    out = model(**dev_batch)
    got = torch.autograd.grad(out["loss"], [params[n] for n in names], allow_unused=True)
    return out["loss"].detach(), out["scores"].detach(), dict(zip(names, got))


def flash_control_step(model, dev_batch, names):
    """Control (ii): the same model with PyTorch's flash-attention ops both ways."""
    assert model.model.hand_attention
    model.model.hand_attention = False
    try:
        return product_step(model, dev_batch, names)
    finally:
        model.model.hand_attention = True


def eager_control_step(model, cfg, dev_batch, names, temperature=T_CONTRASTIVE, block_checkpoint=False):
    """Control (i): the oracle's eager code in bf16 on the device, on the model's weights."""
    dev = next(model.parameters()).device
    wd = {k: v.detach().to(dev, torch.bfloat16).requires_grad_(True) for k, v in model.model.state_dict().items()}
    loss, s = E.contrastive_step(wd, cfg.to_dict(), dev_batch, temperature, dtype=torch.bfloat16, block_checkpoint=block_checkpoint)[:2]
    got = torch.autograd.grad(loss, [wd[n] for n in names], allow_unused=True)
    return loss.detach(), s.detach(), dict(zip(names, got))


def accumulate_bf16(steps):
    """Two (or more) steps' gradients summed the way a bf16 gradient buffer accumulates them: rounded to bf16 after every add."""
    out = {}
    for n in steps[0][2]:
        gs = [s[2].get(n) for s in steps]
        if any(g is None for g in gs):
            out[n] = None
            continue
        buf = torch.zeros_like(gs[0], dtype=torch.bfloat16)
        for g in gs:
            buf += g.to(torch.bfloat16)
        out[n] = buf
    return out


def rel_err(got, ref):
    """Relative Frobenius error against the float64 reference; None where `got` is missing, of another shape or not finite."""
    if got is None or tuple(got.shape) != tuple(ref.shape):
        return None
    g = got.detach().to("cpu", torch.float64)
    if not bool(torch.isfinite(g).all()):
        return None
    return float((g - ref).norm() / ref.norm().clamp_min(1e-300))


def errors(step, ref, names, temperature=T_CONTRASTIVE, score_scale=None):
    """A step (loss, scores, grads) against the reference (loss, scores, grads): `step_parity`'s loss and cosine statistics and
    the per-tensor gradient errors.  loss / scores None: gradients only (an accumulated step has no single loss).  `score_scale`:
    what turns a score difference into a cosine difference; None = `temperature` (InfoNCE's scores are cosines / T), 1.0 for a
    head whose scores are the cosines themselves."""
    loss, scores, grads = step
    out = {"grad": {n: rel_err(grads.get(n), ref[2][n]) for n in names}}
    if loss is not None:
        dc = (scores.detach().to("cpu", torch.float64) - ref[1]) * (temperature if score_scale is None else score_scale)
        out.update(loss_abs_err=abs(float(loss) - ref[0]), cos_rms_err=float(dc.pow(2).mean().sqrt()),
                   cos_max_err=float(dc.abs().max()))
    return out


TABLE_HEAD = "| arm | worst tensor | err fast | err eager | err flash | bound | fast / larger control |"


def rule(ref, fast, eager, flash, names, arm="", temperature=T_CONTRASTIVE, factors=None, out=print, score_scale=None,
         loss_lipschitz=None, metrics=None, metric_lipschitz=None, exact_metrics=()):
    """The rule of the module docstring.  ref / fast / eager / flash: (loss, scores, {name: grad}); `flash` may be None (an encoder
    without hand-written attention has no such control).  `factors`: {tensor name: factor} replacing 1.5 for that tensor on this
    arm -- a documented rounding point, see the caller's comment; nothing else is widened.  Returns the failures as dicts
    (kind: "grad" over its bound, "missing" = absent / None / wrong shape / non-finite, "control" = a control lacks the tensor,
    "guard" = the two controls disagree, "stat" = loss / cosine statistic; name; fast, eager, flash, bound) and prints one table
    row: the tensor that uses most of its bound.

    For a head other than InfoNCE (tests/rankpo_step_parity_util.py): `score_scale` as in `errors`; `loss_lipschitz` = L, the
    loss's Lipschitz constant in the cosines, which stands where InfoNCE has 1 / T (|d loss| <= L * cosine RMS error, floor
    5e-6 * L).  `metrics` = (ref, fast, eager, flash-or-None) dicts of floats with `metric_lipschitz` = {key: L_k}: the fast
    path's keys must be the reference's, every key of `metric_lipschitz` is held to 1.5 * max(control error, L_k * control cosine
    RMS error) + 5e-6 * L_k, every key of `exact_metrics` must equal the reference's value (kind "metric")."""
    factors = factors or {}
    ef, ee = errors(fast, ref, names, temperature, score_scale), errors(eager, ref, names, temperature, score_scale)
    el = errors(flash, ref, names, temperature, score_scale) if flash is not None else None
    fails, worst = [], None
    for n in names:
        f, e, l = ef["grad"][n], ee["grad"][n], (el["grad"][n] if el is not None else None)
        rec = dict(name=n, fast=f, eager=e, flash=l, bound=None)
        if e is None or (el is not None and l is None):
            fails.append(dict(rec, kind="control"))
            continue
        ctrl = max(e, l) if l is not None else e
        rec["bound"] = factors.get(n, FACTOR) * ctrl + GRAD_FLOOR
        if f is None:
            fails.append(dict(rec, kind="missing"))
        else:
            if not f <= rec["bound"]:
                fails.append(dict(rec, kind="grad"))
            if worst is None or f / rec["bound"] > worst["fast"] / worst["bound"]:
                worst = dict(rec, ratio=f / max(ctrl, 1e-300))
        if l is not None and not l <= GUARD * e + GUARD_FLOOR:
            fails.append(dict(rec, kind="guard", bound=GUARD * e + GUARD_FLOOR))
    if "loss_abs_err" in ef:
        both = [ee] + ([el] if el is not None else [])
        ctrl = {k: max(c[k] for c in both) for k in ("loss_abs_err", "cos_rms_err", "cos_max_err")}
        tol = {"cos_rms_err": FACTOR * ctrl["cos_rms_err"] + COS_FLOOR, "cos_max_err": FACTOR * ctrl["cos_max_err"] + COS_FLOOR,
               "loss_abs_err": FACTOR * max(ctrl["loss_abs_err"], ctrl["cos_rms_err"] / temperature) + COS_FLOOR / temperature}
        if loss_lipschitz is not None:
            tol["loss_abs_err"] = FACTOR * max(ctrl["loss_abs_err"], loss_lipschitz * ctrl["cos_rms_err"]) + COS_FLOOR * loss_lipschitz
        for k, t in tol.items():
            rec = dict(name=k, fast=ef[k], eager=ee[k], flash=el[k] if el is not None else None, bound=t)
            if not ef[k] <= t:
                fails.append(dict(rec, kind="stat"))
            if el is not None and k != "loss_abs_err" and not el[k] <= GUARD * ee[k] + GUARD_FLOOR:
                fails.append(dict(rec, kind="guard", bound=GUARD * ee[k] + GUARD_FLOOR))
    if metrics is not None:
        assert "loss_abs_err" in ef, "metrics are judged against the controls' cosine error: the steps need their scores"
        mr, mf, me, ml = metrics
        assert (ml is None) == (flash is None)
        ctrls = [me] + ([ml] if ml is not None else [])
        for k in sorted(set(mr) | set(mf)):
            if k not in mr or k not in mf or any(k not in c for c in ctrls):
                fails.append(dict(name=k, kind="metric", fast=None, eager=None, flash=None, bound=None))
                continue
            err = lambda m: abs(float(m[k]) - float(mr[k]))
            rec = dict(name=k, fast=err(mf), eager=err(me), flash=err(ml) if ml is not None else None, bound=None)
            if k in exact_metrics:
                rec["bound"] = 0.0
            elif k in (metric_lipschitz or {}):
                lk = metric_lipschitz[k]
                rec["bound"] = FACTOR * max(max(err(c) for c in ctrls), lk * ctrl["cos_rms_err"]) + COS_FLOOR * lk
            else:
                raise KeyError(f"metric {k} has neither a Lipschitz constant nor an exact comparison")
            if not rec["fast"] <= rec["bound"]:
                fails.append(dict(rec, kind="metric"))
    fmt = lambda x: "-" if x is None else f"{x:.3e}"
    if worst is not None:
        out(f"| {arm} | {worst['name']} | {fmt(worst['fast'])} | {fmt(worst['eager'])} | {fmt(worst['flash'])} | "
            f"{fmt(worst['bound'])} | {worst['ratio']:.2f} |")
    for r in fails:
        out(f"  FAIL [{arm}] {r['kind']} {r['name']}: fast {fmt(r['fast'])} eager {fmt(r['eager'])} flash {fmt(r['flash'])} "
            f"bound {fmt(r['bound'])}")
    return fails


def failed_names(fails, kind=None):
    return sorted({r["name"] for r in fails if kind is None or r["kind"] == kind})


# ------------------------------------------------------------------------------------------------------------------------------
# one (config, batch) case on the device: model, float64 reference and the two controls, computed once and shared by every arm
# ------------------------------------------------------------------------------------------------------------------------------
def make_case(PE, rankpo_amd, cfg, batch, tot, device="cuda:0", seed=0, ref_device="cpu", block_checkpoint=False):
    enc, model = build_model(PE, rankpo_amd, cfg, seed, device)
    names = param_names(enc)
    assert set(names) == set(enc.state_dict()), "a parameter of the encoder is missing from its state dict (or the reverse)"
    dev_batch = to_device(batch, device)
    ref = oracle64(enc.state_dict(), cfg.to_dict(), batch, T_CONTRASTIVE, device=ref_device, block_checkpoint=block_checkpoint)
    if ref_device != "cpu":
        torch.cuda.empty_cache()
    eager = eager_control_step(model, cfg, dev_batch, names, block_checkpoint=block_checkpoint)
    flash = flash_control_step(model, dev_batch, names)
    return SimpleNamespace(cfg=cfg, enc=enc, model=model, names=names, batch=batch, tot=tot, padded=(tot + 255) // 256 * 256,
                           dev_batch=dev_batch, ref=ref, eager=eager, flash=flash,
                           rows=sum(v["input_ids"].shape[0] for v in batch.values()))


@functools.lru_cache(maxsize=None)
def case_s(layout="hd64", batch_seed=2026, seed=0):
    """Config S in `layout` on `batch_s(batch_seed)`; the float64 oracle runs on the host."""
    import rankpo_amd
    from rankpo_amd import encoder as PE
    batch, tot = batch_s(batch_seed)
    assert tot >= 4096 and tot % 256 != 0, tot
    return make_case(PE, rankpo_amd, cfg_s(PE, layout), batch, tot, seed=seed)


@functools.lru_cache(maxsize=None)
def case_l(batch_seed=31, seed=0):
    """Config L: the float64 oracle runs on the device with every block checkpointed (a [12, 4, 3072, 3072] float64 score tensor
    per block), and so does the eager bf16 control."""
    import rankpo_amd
    from rankpo_amd import encoder as PE
    batch, tot = batch_l(batch_seed)
    assert (tot + 255) // 256 * 256 >= 32768, tot
    return make_case(PE, rankpo_amd, cfg_l(PE), batch, tot, seed=seed, ref_device="cuda:0", block_checkpoint=True)
