"""Host side of the Llama step gradient parity (tests/llama_step_parity_util.py): the rule on hand-made dicts -- it passes equal
gradients and fails a missing, None, NaN or over-bound tensor under that tensor's name, and its guard fires when only the
stock-flash control is off --, the float64 oracle reaches every parameter of the S and L configs, and the names the GPU test
iterates are exactly `named_parameters()`."""
import pytest
import torch

import llama_step_parity_util as U

NAMES = ["a.weight", "b.weight", "c.weight"]


def _ref():
    g = torch.Generator().manual_seed(0)
    return 1.25, torch.randn(2, 6, generator=g, dtype=torch.float64) / U.T_CONTRASTIVE, \
        {n: torch.randn(4, 8, generator=g, dtype=torch.float64) for n in NAMES}


def _off(ref, rel, seed, scores_rel=None):
    """The reference moved by a relative error of `rel` on every gradient (and `scores_rel` on loss and scores)."""
    g = torch.Generator().manual_seed(seed)
    sr = rel if scores_rel is None else scores_rel
    grads = {}
    for n, t in ref[2].items():
        e = torch.randn(t.shape, generator=g, dtype=torch.float64)
        grads[n] = (t + rel * t.norm() * e / e.norm()).float()
    return torch.tensor(ref[0] * (1 + sr)), (ref[1] * (1 + sr)).float(), grads


def _rule(ref, fast, eager, flash, **kw):
    lines = []
    return U.rule(ref, fast, eager, flash, NAMES, arm="host", out=lines.append, **kw), lines


def test_rule_passes_equal_and_within_bound_gradients():
    ref = _ref()
    eager, flash = _off(ref, 1e-2, 1), _off(ref, 1.2e-2, 2)
    for fast in (_off(ref, 0.0, 3), _off(ref, 1e-2, 3), _off(ref, 1.7e-2, 3)):      # bound: 1.5 x 1.2e-2 + 1e-4
        fails, lines = _rule(ref, fast, eager, flash)
        assert fails == [], fails
        assert len(lines) == 1 and lines[0].startswith("| host | ")                 # the worst tensor, as a table row
    # without a stock-flash control the eager one alone sets the bound
    assert _rule(ref, _off(ref, 1.4e-2, 3), eager, None)[0] == []
    assert U.failed_names(_rule(ref, _off(ref, 1.7e-2, 3, scores_rel=1e-2), eager, None)[0]) == NAMES


@pytest.mark.parametrize("how", ["missing", "none", "nan", "inf", "shape", "over"])
def test_rule_fails_one_bad_tensor_under_its_own_name(how):
    ref = _ref()
    eager, flash = _off(ref, 1e-2, 1), _off(ref, 1.2e-2, 2)
    fast = _off(ref, 1e-2, 3)
    g = fast[2]
    if how == "missing":
        del g["b.weight"]
    elif how == "none":
        g["b.weight"] = None
    elif how == "nan":
        g["b.weight"][1, 2] = float("nan")
    elif how == "inf":
        g["b.weight"][0, 0] = float("inf")
    elif how == "shape":
        g["b.weight"] = g["b.weight"][:, :4]
    else:
        g["b.weight"] = _off(ref, 2e-2, 4)[2]["b.weight"]                            # over 1.5 x 1.2e-2 + 1e-4 = 1.81e-2
    fails, lines = _rule(ref, fast, eager, flash)
    assert U.failed_names(fails) == ["b.weight"], fails
    assert {r["kind"] for r in fails} == ({"grad"} if how == "over" else {"missing"})
    assert all(r["eager"] is not None and r["flash"] is not None for r in fails)     # both control errors are reported
    assert any("b.weight" in ln and "FAIL" in ln for ln in lines)


def test_a_per_tensor_factor_widens_that_tensor_only():
    ref = _ref()
    eager, flash = _off(ref, 1e-2, 1), _off(ref, 1.2e-2, 2)
    fast = _off(ref, 2e-2, 3, scores_rel=1e-2)
    assert U.failed_names(_rule(ref, fast, eager, flash)[0]) == NAMES
    assert U.failed_names(_rule(ref, fast, eager, flash, factors={"b.weight": 2.0})[0]) == ["a.weight", "c.weight"]


def test_guard_fires_when_only_the_stock_flash_control_is_off():
    """A glue defect shared by the fast path and the stock-flash control: the bound follows the inflated control and says
    nothing, the comparison of the two controls names the tensor."""
    ref = _ref()
    eager = _off(ref, 1e-2, 1)
    flash, fast = _off(ref, 1.2e-2, 2), _off(ref, 1.2e-2, 3)
    flash[2]["c.weight"] = _off(ref, 8e-2, 5)[2]["c.weight"]
    fast[2]["c.weight"] = _off(ref, 8e-2, 6)[2]["c.weight"]
    fails, _ = _rule(ref, fast, eager, flash)
    assert [(r["kind"], r["name"]) for r in fails] == [("guard", "c.weight")], fails
    # at 2.5 x the eager control the guard still holds
    flash[2]["c.weight"] = _off(ref, 2.4e-2, 5)[2]["c.weight"]
    fast[2]["c.weight"] = _off(ref, 2.4e-2, 6)[2]["c.weight"]
    assert _rule(ref, fast, eager, flash)[0] == []
    # a control that lacks a tensor is a failure of its own, never a free pass
    del flash[2]["a.weight"]
    assert [(r["kind"], r["name"]) for r in _rule(ref, fast, eager, flash)[0]] == [("control", "a.weight")]


def test_loss_and_cosine_statistics_follow_step_parity():
    ref = _ref()
    eager, flash = _off(ref, 1e-2, 1, scores_rel=1e-3), _off(ref, 1e-2, 2, scores_rel=1e-3)
    assert _rule(ref, _off(ref, 1e-2, 3, scores_rel=1.4e-3), eager, flash)[0] == []
    fails, _ = _rule(ref, _off(ref, 1e-2, 3, scores_rel=4e-3), eager, flash)
    assert U.failed_names(fails, "stat") == ["cos_max_err", "cos_rms_err"] and U.failed_names(fails, "grad") == []
    # the loss: 1.5 x max(control loss error, control cosine RMS error / T) + 5e-6 / T
    ok = _off(ref, 1e-2, 3, scores_rel=1e-3)
    rms_over_t = max(U.errors(c, ref, NAMES)["cos_rms_err"] for c in (eager, flash)) / U.T_CONTRASTIVE
    for d_loss, bad in ((1.4 * rms_over_t, []), (1.6 * rms_over_t + 5e-6 / U.T_CONTRASTIVE, ["loss_abs_err"])):
        fails, _ = _rule(ref, (torch.tensor(ref[0] + d_loss, dtype=torch.float64), ok[1], ok[2]), eager, flash)
        assert U.failed_names(fails) == bad, fails
    # gradients only (an accumulated step has no single loss): no statistic is judged
    acc = (None, None, _off(ref, 1e-2, 3)[2])
    assert _rule(ref, acc, eager, flash)[0] == []


def test_accumulate_bf16_rounds_after_every_add():
    a = {"w": torch.tensor([1.0, 256.0]).bfloat16()}
    b = {"w": torch.tensor([2.0 ** -8, 1.0]).bfloat16()}
    got = U.accumulate_bf16([(None, None, a), (None, None, b)])["w"]
    assert got.dtype == torch.bfloat16 and got.tolist() == [1.0, 256.0]             # both adds are ties that round to even
    assert U.accumulate_bf16([(None, None, a), (None, None, {"w": None})])["w"] is None


@pytest.mark.parametrize("which", ["hd64", "hd128_g4", "g3", "L"])
def test_float64_oracle_reaches_every_parameter(which):
    """Every parameter of the S and L configs gets a non-zero float64 gradient (norm weights off 1.0), on a 2-query batch; the names
    iterated are exactly `named_parameters()`: 9 per block, the embedding table and the final norm."""
    from rankpo_amd import encoder as PE
    cfg = U.cfg_l(PE) if which == "L" else U.cfg_s(PE, which)
    enc = U.build_encoder(PE, cfg, seed=0)
    names = U.param_names(enc)
    assert names == [n for n, _ in enc.named_parameters()] and set(names) == set(enc.state_dict())
    assert len(names) == 9 * cfg.num_hidden_layers + 2 and len(set(names)) == len(names)
    norms = [p for n, p in enc.named_parameters() if n.endswith("norm.weight")]
    assert len(norms) == 2 * cfg.num_hidden_layers + 1 and all(float((p.detach() - 1).abs().max()) > 1e-3 for p in norms)
    sd = {k: v.to(torch.bfloat16) for k, v in enc.state_dict().items()}              # the values a bf16 model holds
    loss, scores, grads = U.oracle64(sd, cfg.to_dict(), U.batch_tiny())
    assert sorted(grads) == sorted(names) and scores.shape == (2, 4) and scores.dtype == torch.float64
    assert all(g.dtype == torch.float64 and g.shape == sd[n].shape and float(g.norm()) > 0 for n, g in grads.items())


def test_configs_and_batches_are_the_ones_the_arms_need():
    from rankpo_amd import encoder as PE
    for layout, (hd, nh, nkv, d) in U.LAYOUTS_S.items():
        c = U.cfg_s(PE, layout)
        assert (c.head_dim, c.num_attention_heads, c.num_key_value_heads, c.hidden_size) == (hd, nh, nkv, d)
        assert (c.intermediate_size, c.num_hidden_layers, c.rope_scaling["rope_type"]) == (1024, 4, "llama3")
        assert c.intermediate_size >= 2 * c.hidden_size                              # the transposed SwiGLU product's gate
    for hd in (64, 128):                                                             # the bench-path gate's own configs
        assert U.cfg_s(PE, "hd64" if hd == 64 else "hd128_g2").to_dict() == U.FP._cfg(PE, hd).to_dict()
    c = U.cfg_l(PE)
    nq, nk = c.num_attention_heads * c.head_dim, c.num_key_value_heads * c.head_dim
    assert (nq + 2 * nk, c.hidden_size) == (384, 256)                                # q|k|v 384 x 256, o 256 x 256:
    assert not nq + 2 * nk >= 2 * c.hidden_size and not c.hidden_size >= 2 * nq       # neither operand twice the other
    for seed in (2026, 1, 2):
        _, tot = U.batch_s(seed)
        assert tot >= 4096 and tot % 256 != 0
    b, tot = U.batch_l()
    assert (tot + 255) // 256 * 256 >= 32768 and tot % 256 != 0
    assert int(b["query"]["attention_mask"].sum(-1).max()) <= 512
    lens = b["passage"]["attention_mask"].sum(-1)
    assert b["passage"]["input_ids"].shape == (12, 3072) and int(lens.min()) >= 2816 and int(lens.max()) == 3072
