"""The bf16 packed Llama training step, EVERY weight gradient against float64, on every arm of the Python glue between the kernels
(rankpo_amd/ops.py, rankpo_amd/encoder.py): `ops.wgrad`'s five branches, `_SwiGLUDown.backward`'s transposed-product and `dgu_t`
paths, `_LinearTN`, `_FusedWeight` as a view of the flat buffer, `FOLD_ROPE` 0 / 1 / 2, checkpointing (partial, pair input,
recomputed output), the 256-token filler, head groups 1 / 2 / 3 / 4 / 8 at head_dim 64 and 128, the last block on the pooled rows.

The rule, the float64 reference and the two bf16 controls are tests/llama_step_parity_util.py's (`bench_parity.step_parity`'s bound and
guard, applied per tensor to all of `named_parameters()`).  Reference and controls are computed once per (config, batch) and shared
by the arms, which differ in product switches only; every switch is set through `monkeypatch`.  Every arm installs spies for the
duration of its product step alone (the controls are not counted) and compares what ran -- kernels, branches of `wgrad`, transposes,
checkpoint calls -- with what the arm is named after (`_expected`).  Two injected defects (a lost tail tile in one weight gradient, a
lost dK in the last block) show that the harness can fail, and where.  Every arm prints its worst tensor as a table row
(profiles/llama_step_grad_parity.md holds a copy)."""
import collections
import re

import pytest
import torch

import llama_step_parity_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Spy:
    """Records what one product step ran.  Installed through a `monkeypatch` context of its own, so it is gone before anything
    else (a control, the next arm) runs."""

    def __init__(self, m):
        from rankpo_amd import _lib, encoder as PE, ops
        self.ops, self.n = ops, collections.Counter()
        self.wgrad, self.transposed, self.bmm_f32, self.fwd, self.bwd, self.fused, self.ckpt, self.views = [], [], [], [], [], [], [], []
        self.hits0 = ops.WGRAD_DY_T_HITS
        lib = _lib.load()

        def count(obj, name, key, record=None):
            real = getattr(obj, name)

            def spy(*a, **kw):
                self.n[key] += 1
                if record is not None:
                    record(*a, **kw)
                return real(*a, **kw)
            m.setattr(obj, name, spy)
        for k in ("rpo_swiglu_fwd", "rpo_swiglu_bwd", "rpo_swiglu_bwd_t"):
            count(lib, k, k)
        count(ops, "_wt", "wt")
        count(ops, "rope_", "rope_")
        count(ops, "last_query_attn", "lastq")
        count(PE, "_varlen_last_query_attention", "lastq_fallback")
        count(ops, "transpose2d", "transpose2d", lambda x: self.transposed.append(tuple(x.shape)))
        count(ops, "wgrad", "wgrad", lambda dy2, x2, dy_t=None: self.wgrad.append((dy2.shape[0], dy2.shape[1], x2.shape[1], dy_t is not None)))
        count(ops, "flash_attn_varlen_fwd", "fwd",
              lambda q, *a, **kw: self.fwd.append((q.shape[0], kw.get("q_block", 128), kw.get("rope") is not None)))
        count(ops, "flash_attn_varlen_bwd", "bwd", lambda q, *a, **kw: self.bwd.append((q.shape[0], kw.get("rope") is not None)))
        count(ops, "rope_flash_attn_varlen_qkv", "fused",
              lambda qkv, *a, **kw: self.fused.append((qkv.shape[-2], bool(kw.get("fold_forward", True)))))
        count(PE, "checkpoint", "ckpt", lambda fn, x, delta, *a, **kw: self.ckpt.append(delta is None))
        count(PE.LlamaLayer, "forward_last_rows", "last_rows")
        real_bmm, real_fw = torch.bmm, PE.fused_weight

        def bmm(a, b, **kw):
            if kw.get("out_dtype") == torch.float32:
                self.bmm_f32.append((tuple(a.shape), tuple(b.shape)))
            return real_bmm(a, b, **kw)

        def fused_weight(ws):
            out = real_fw(ws)
            self.views.append(out.data_ptr() == ws[0].data_ptr())
            return out
        m.setattr(torch, "bmm", bmm)
        m.setattr(PE, "fused_weight", fused_weight)

    def summary(self, act_rows):
        n = self.n
        return dict(fused=self.fused, fwd=self.fwd, bwd=self.bwd, rope_=n["rope_"], lastq=n["lastq"], lastq_fallback=n["lastq_fallback"],
                    last_rows=n["last_rows"], ckpt=self.ckpt, swiglu_fwd=n["rpo_swiglu_fwd"], swiglu_bwd=n["rpo_swiglu_bwd"],
                    swiglu_bwd_t=n["rpo_swiglu_bwd_t"], dy_t_hits=self.ops.WGRAD_DY_T_HITS - self.hits0, wt=n["wt"],
                    wgrad=collections.Counter(self.wgrad), bmm_f32=sorted(self.bmm_f32),
                    act_transposes=sum(s[0] in act_rows for s in self.transposed),
                    weight_transposes=sum(s[0] not in act_rows for s in self.transposed))


SW = dict(fold=2, linear_tn=True, mixed=True, prod_t=True, dgu_t=True, dgu_limit=None, ckpt=0, single=True, skip=True, fill=True, split=4)


def _apply(monkeypatch, c, sw):
    from rankpo_amd import encoder as PE, ops
    for mod, name, key in ((PE, "FOLD_ROPE", "fold"), (ops, "LINEAR_TN", "linear_tn"), (ops, "WGRAD_MIXED", "mixed"),
                           (ops, "SWIGLU_PROD_T", "prod_t"), (ops, "SWIGLU_DGU_T", "dgu_t"), (PE, "CKPT_SINGLE_INPUT", "single"),
                           (ops, "SKIP_RECOMPUTED_OUTPUT", "skip"), (ops, "WGRAD_SPLIT_T", "split")):
        monkeypatch.setattr(mod, name, sw[key])
    if sw["dgu_limit"] is not None:
        monkeypatch.setattr(ops, "SWIGLU_DGU_T_MAX_BYTES", sw["dgu_limit"])
    monkeypatch.setattr(c.enc, "pack_fill", sw["fill"])
    monkeypatch.setattr(c.enc, "gradient_checkpointing", sw["ckpt"] > 0)
    monkeypatch.setattr(c.enc, "checkpoint_layers", None if sw["ckpt"] == c.cfg.num_hidden_layers else sw["ckpt"])
    monkeypatch.setattr(c.enc, "memory_plan", None)


def _expected(c, sw):
    """What a step of case `c` under the switches `sw` must run, from the gates of ops.py / encoder.py restated on the shapes."""
    from rankpo_amd import ops
    cfg = c.cfg
    nb, d, ff, hd, nh, nkv = cfg.num_hidden_layers, cfg.hidden_size, cfg.intermediate_size, cfg.head_dim, cfg.num_attention_heads, cfg.num_key_value_heads
    full, nq, nk2 = nb - 1, nh * hd, 2 * nkv * hd
    W = nq + nk2
    T = c.padded if sw["fill"] else c.tot
    R = c.rows + (1 if sw["fill"] else 0)                                  # rows of the last block: one per sequence, the filler's too
    ck_full, ck_last = min(sw["ckpt"], full), int(sw["ckpt"] == nb)
    fwds, lasts = full + ck_full, 1 + ck_last                             # forwards of the full blocks / of the last one, recomputations included
    q_block = 64 if (hd in ops.FWD_ONE_WAVE_HEAD_DIMS and (nh // nkv) % 4 == 0) else 128
    lastq_ok = nh // nkv in (1, 2, 4)
    tn, mixed = sw["linear_tn"], sw["mixed"]
    prod_t = mixed and sw["prod_t"] and ff >= 2 * d and T >= 4096 and T % 8 == 0
    hit = prod_t and sw["dgu_t"] and tn and (sw["dgu_limit"] is None or 2 * ff * T * 2 <= sw["dgu_limit"])
    wg = collections.Counter()
    if tn:                                                                # (tokens, n, k, dy_t handed over) of every `wgrad` call
        for key, times in (((T, W, d, False), full), ((T, d, nq, False), full), ((T, 2 * ff, d, hit), full), ((T, nk2, d, False), 1),
                           ((R, 2 * ff, d, False), 1)):
            wg[key] += times
    if not prod_t:
        wg[(T, d, ff, False)] += full
    wg[(R, d, ff, False)] += 1
    two = lambda n, k: int(mixed and (n >= 2 * k or k >= 2 * n))          # wgrad transposes the smaller operand
    act = full * (int(prod_t) + (two(d, ff) if not prod_t else 0) + (1 if hit else two(2 * ff, d) if tn else 0)
                  + (two(W, d) + two(d, nq) if tn else 0))
    act += (two(nk2, d) + two(2 * ff, d) if tn else 0) + two(d, ff)
    split = sw["split"] > 1 and mixed and tn and T >= 32768 and T % sw["split"] == 0 and not two(W, d)
    S = sw["split"]
    return dict(
        fused=[(T, sw["fold"] >= 2)] * (fwds if sw["fold"] else 0),
        fwd=[(T, q_block, sw["fold"] >= 2)] * fwds, bwd=[(T, sw["fold"] >= 1)] * full,
        rope_=2 * lasts + (0 if sw["fold"] else fwds),
        lastq=lasts if lastq_ok else 0, lastq_fallback=0 if lastq_ok else lasts, last_rows=lasts,
        ckpt=[i == 0 or sw["single"] for i in range(sw["ckpt"])],
        swiglu_fwd=nb + (0 if sw["skip"] else sw["ckpt"]), swiglu_bwd=nb - (full if prod_t else 0), swiglu_bwd_t=full if prod_t else 0,
        dy_t_hits=full if hit else 0, wt=(4 * full + 3) if tn else 0, wgrad=wg,
        bmm_f32=sorted([((S, W, T // S), (S, T // S, d)), ((S, d, T // S), (S, T // S, nq))] * full) if split else [],
        act_transposes=act, weight_transposes=(4 * full + 3) if tn else 0)


def _run_arm(monkeypatch, name, c, over, factors=None):
    sw = dict(SW, **over)
    _apply(monkeypatch, c, sw)
    with monkeypatch.context() as m:
        spy = Spy(m)
        fast = U.product_step(c.model, c.dev_batch, c.names)
        torch.cuda.synchronize()
    print()
    fails = U.rule(c.ref, fast, c.eager, c.flash, c.names, arm=name, factors=factors)
    T = c.padded if sw["fill"] else c.tot
    got, want = spy.summary({T, c.rows + (1 if sw["fill"] else 0)}), _expected(c, sw)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"arm {name}: the branches it is named after did not run as stated (got, expected): {wrong}"
    return fails, spy, sw


ARMS_S = [
    # 1. default switches, head_dim 64, 8 / 2 heads
    ("default hd64 8/2", "hd64", {}),
    # 2. head_dim 128: 4 / 1 heads (the one-wave forward list) with every block checkpointed; 4 / 2 heads (the 128-query forward)
    ("hd128 4/1 ckpt all", "hd128_g4", dict(ckpt=4)),
    ("hd128 4/2", "hd128_g2", {}),
    # 3. FOLD_ROPE 1 and 0 at both head dims (128: both forward kernels)
    ("FOLD_ROPE=1 hd64", "hd64", dict(fold=1)), ("FOLD_ROPE=0 hd64", "hd64", dict(fold=0)),
    ("FOLD_ROPE=1 hd128 4/1", "hd128_g4", dict(fold=1)), ("FOLD_ROPE=0 hd128 4/1", "hd128_g4", dict(fold=0)),
    ("FOLD_ROPE=1 hd128 4/2", "hd128_g2", dict(fold=1)), ("FOLD_ROPE=0 hd128 4/2", "hd128_g2", dict(fold=0)),
    # 4. the four GEMM-layout switches, each alone and all together
    ("LINEAR_TN off", "hd64", dict(linear_tn=False)), ("WGRAD_MIXED off", "hd64", dict(mixed=False)),
    ("SWIGLU_PROD_T off", "hd64", dict(prod_t=False)), ("SWIGLU_DGU_T off", "hd64", dict(dgu_t=False)),
    ("all four off", "hd64", dict(linear_tn=False, mixed=False, prod_t=False, dgu_t=False)),
    ("dgu_t over its size limit", "hd64", dict(dgu_limit=1 << 20)),
    # 5. checkpointing: 2 of 4 (a checkpointed block hands (x, delta) to an un-checkpointed one), all, the pair input, the recomputed output
    ("ckpt 2 of 4", "hd64", dict(ckpt=2)), ("ckpt all", "hd64", dict(ckpt=4)),
    ("ckpt all, CKPT_SINGLE_INPUT off", "hd64", dict(ckpt=4, single=False)),
    ("ckpt all, SKIP_RECOMPUTED_OUTPUT off", "hd64", dict(ckpt=4, skip=False)),
    # 6. head groups 1, 8 and 3 (8 and 3: `last_query_attn_ok` declines, the last block takes PyTorch's op)
    ("group 1 (4/4 hd128)", "g1", {}), ("group 8 (8/1 hd64)", "g8", {}), ("group 3 (6/2 hd64 d384)", "g3", {}),
    # 7. no filler: the packed token count is no multiple of 256
    ("pack_fill off", "hd64", dict(fill=False)),
]


@pytest.mark.parametrize("name,layout,over", ARMS_S, ids=[re.sub(r"[^A-Za-z0-9]+", "_", a[0]).strip("_") for a in ARMS_S])
def test_config_s_every_gradient(monkeypatch, name, layout, over):
    """Config S (d 512, ff 1024, 4 blocks, llama3 rope) on `test_gpu_fastpath._batch()`: >= 4096 packed tokens, so the filler fires,
    the full blocks take the transposed SwiGLU product and `dgu_t`, and the last block's MLP on N rows takes `rpo_swiglu_bwd` and the
    `k >= 2n` branch of `wgrad`."""
    c = U.case_s(layout)
    fails, spy, sw = _run_arm(monkeypatch, name, c, over)
    assert not fails, fails


def test_flat_buffers_fused_weights_are_views_and_gradients_accumulate(monkeypatch):
    """`TrainStep` moves the parameters into FlatAdamW's flat buffer: q|k|v and gate|up are then zero-copy views (`_FusedWeight`), and
    `micro_step` on two different micro-batches accumulates into the bf16 flat gradient buffer.  Reference: the sum of the two float64
    gradients; each control accumulates its two bf16 gradients in a bf16 buffer the same way."""
    import rankpo_amd
    from rankpo_amd import encoder as PE
    from rankpo_amd.train_step import TrainStep
    a, b = U.case_s("hd64"), U.case_s("hd64", 2)
    enc, model = U.build_model(PE, rankpo_amd, a.cfg, seed=0, device=DEV)
    for n, p in enc.named_parameters():                       # the weights the two references and their controls were computed on
        assert torch.equal(p, dict(a.enc.named_parameters())[n]) and torch.equal(p, dict(b.enc.named_parameters())[n])
    ts = TrainStep(list(enc.parameters()), lambda batch: model(**batch)["loss"])
    for layer in enc.layers:
        at, mlp = layer.self_attn, layer.mlp
        w = PE.fused_weight([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight])
        assert w.data_ptr() == at.q_proj.weight.data_ptr() and w.shape[0] == sum(x.weight.shape[0] for x in (at.q_proj, at.k_proj, at.v_proj))
        assert torch.equal(w, torch.cat([at.q_proj.weight, at.k_proj.weight, at.v_proj.weight], 0))
        assert PE.fused_weight([at.k_proj.weight, at.v_proj.weight]).data_ptr() == at.k_proj.weight.data_ptr()
        assert PE.fused_weight([mlp.gate_proj.weight, mlp.up_proj.weight]).data_ptr() == mlp.gate_proj.weight.data_ptr()
    with monkeypatch.context() as m:
        spy = Spy(m)
        ts.micro_step(a.dev_batch, last=False)
        ts.micro_step(b.dev_batch, last=True)
        torch.cuda.synchronize()
    assert spy.views and all(spy.views), spy.views            # the steps themselves ran on the views
    flat = ts.opt.reducer.flat
    grads = {}
    for n, p in enc.named_parameters():
        assert p.grad is not None and flat.data_ptr() <= p.grad.data_ptr() < flat.data_ptr() + flat.numel() * 2, n
        grads[n] = p.grad
    ref = (None, None, {n: a.ref[2][n] + b.ref[2][n] for n in a.names})
    print()
    fails = U.rule(ref, (None, None, grads), (None, None, U.accumulate_bf16([a.eager, b.eager])),
                   (None, None, U.accumulate_bf16([a.flash, b.flash])), a.names, arm="flat buffers, 2 micro-batches")
    assert not fails, fails


@pytest.mark.parametrize("name,over", [("L split-T wgrad", {}), ("L WGRAD_SPLIT_T=0", dict(split=0))], ids=["split_t", "one_gemm"])
def test_config_l_split_t_weight_gradient(monkeypatch, name, over):
    """Config L (d 256, 4 / 1 heads of 64, ff 512, 2 blocks) on 4 queries + 12 passages of 2816-3072 tokens: >= 32768 packed tokens,
    where the q|k|v (384 x 256) and o (256 x 256) weight gradients of the full block take the split-T `bmm` with float32 partials
    (`_expected` asserts both ran: `bmm_f32`), and the same step with WGRAD_SPLIT_T = 0 (one GEMM each)."""
    from rankpo_amd import ops
    if not over and not ops._bmm_f32_out_ok(torch.device(DEV)):
        pytest.skip("this torch / backend does not run bmm(bf16, bf16, out_dtype=float32): ops.wgrad never takes the split-T branch")
    c = U.case_l()
    assert c.padded >= 32768
    fails, spy, sw = _run_arm(monkeypatch, name, c, over)
    assert len(spy.bmm_f32) == (2 * (c.cfg.num_hidden_layers - 1) if not over else 0)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------------------
# the harness must be able to fail: two defects injected at the Python level
# ------------------------------------------------------------------------------------------------------------------------------
def _lost_tail_tile(m, c, T):
    """`ops.wgrad` loses the last 32 token rows of both operands in the call that produces block 1's down_proj gradient (the
    second [T, d] x [T, ff] call of a backward pass: blocks 2, 1, 0)."""
    from rankpo_amd import ops
    real, seen = ops.wgrad, {"n": 0}
    d, ff = c.cfg.hidden_size, c.cfg.intermediate_size

    def bad(dy2, x2, dy_t=None):
        if tuple(dy2.shape) == (T, d) and tuple(x2.shape) == (T, ff):
            seen["n"] += 1
            if seen["n"] == 2:
                return real(dy2[:-32], x2[:-32], dy_t)
        return real(dy2, x2, dy_t)
    m.setattr(ops, "wgrad", bad)
    return seen


def test_injected_lost_tail_tile_is_reported_at_its_tensor(monkeypatch):
    """Without the filler (its rows carry zero gradients: losing them changes nothing) and with SWIGLU_PROD_T off (so that the down
    projection's gradient goes through `ops.wgrad`).  Fast path alone: the bound reports exactly that tensor.  Fast path and
    stock-flash control alike (a glue defect): the bound follows the inflated control, the per-tensor guard reports the tensor.

    The batch is `batch_s(2)`, not the arms': with last-token pooling nearly all of a block's output gradient sits on the pooled
    rows, and a passage that is an easy negative carries almost none -- on the arms' batch the last 32 rows hold 0.7 % of the
    gradient norm at block 1's MLP output (measured on the float32 host path), a loss below the bf16 error of the controls that no
    control-relative bound can see.  On `batch_s(2)` the last passage is a hard negative and its tail holds 27 %.  That the
    defect is material is asserted here on the fast path's own two results, apart from the rule."""
    c = U.case_s("hd64", 2)
    bad_name = "layers.1.mlp.down_proj.weight"
    sw = dict(SW, prod_t=False, fill=False)
    _apply(monkeypatch, c, sw)
    healthy = U.product_step(c.model, c.dev_batch, c.names)
    with monkeypatch.context() as m:
        seen = _lost_tail_tile(m, c, c.tot)
        fast = U.product_step(c.model, c.dev_batch, c.names)
        assert seen["n"] == c.cfg.num_hidden_layers - 1
        seen["n"] = 0
        flash = U.flash_control_step(c.model, c.dev_batch, c.names)
        assert seen["n"] == c.cfg.num_hidden_layers - 1
    moved = {n: float((fast[2][n].double() - healthy[2][n].double()).norm() / healthy[2][n].double().norm()) for n in c.names}
    print(f"\ndefect A moves {bad_name} by {moved[bad_name]:.3f} (relative), every other tensor by <= "
          f"{max(v for n, v in moved.items() if n != bad_name):.1e}")
    assert moved[bad_name] >= 0.1 and all(v <= 1e-2 for n, v in moved.items() if n != bad_name), moved
    assert not U.rule(c.ref, healthy, c.eager, c.flash, c.names, arm="SWIGLU_PROD_T off, pack_fill off (batch 2)")
    fails = U.rule(c.ref, fast, c.eager, c.flash, c.names, arm="defect A, fast path only")
    assert [(r["kind"], r["name"]) for r in fails] == [("grad", bad_name)], fails
    fails = U.rule(c.ref, fast, c.eager, flash, c.names, arm="defect A, fast path and stock-flash control")
    assert ("guard", bad_name) in [(r["kind"], r["name"]) for r in fails] and U.failed_names(fails) == [bad_name], fails


def test_injected_lost_dk_of_the_last_block_is_reported_there(monkeypatch):
    """`ops.last_query_attn` returns a zero gradient for the k half of `kv`: the last block's k_proj.weight is reported, and no tensor
    of another block's MLP."""
    from rankpo_amd import ops
    c = U.case_s("hd64")
    _apply(monkeypatch, c, SW)
    real = ops.last_query_attn

    def bad(q, kv, cu, nkv, hd, scale):
        nk = nkv * hd
        kv.register_hook(lambda g: torch.cat([torch.zeros_like(g[..., :nk]), g[..., nk:]], -1))
        return real(q, kv, cu, nkv, hd, scale)
    with monkeypatch.context() as m:
        m.setattr(ops, "last_query_attn", bad)
        fast = U.product_step(c.model, c.dev_batch, c.names)
    print()
    fails = U.rule(c.ref, fast, c.eager, c.flash, c.names, arm="defect B, lost dK in the last block")
    last = c.cfg.num_hidden_layers - 1
    names = U.failed_names(fails)
    assert f"layers.{last}.self_attn.k_proj.weight" in names, fails
    assert not [n for n in names if ".mlp." in n and not n.startswith(f"layers.{last}.")], fails
