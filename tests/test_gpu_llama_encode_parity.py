"""The forward-only (no-grad) bf16 packed Llama path, EVERY pooled row against float64, on every arm of the glue it takes
(rankpo_amd/encoder.py, ops.py, modeling.py): the four entry points (`ModelForInference.encode()`, `pooled_last_token` on a device
batch, eval-mode `ModelForTraining`, the RankPO ref_model under `inference_mode`), sequence lengths on every 64- and 128-token tile
edge, the 256-token filler fired / not reached / met exactly / switched off, head groups 1 / 2 / 3 / 4 / 8 at head_dim 64 and 128
(3 and 8: the last block's PyTorch fallback), `FOLD_ROPE` 0 / 1 / 2, `FWD128_ONE_WAVE` off, `encode()`'s batching and
`bucket_by_length`, fp16 storage.

The rule, the float64 reference (one sequence at a time, unpadded) and the two controls are tests/llama_encode_parity_util.py's.
Reference and controls are computed once per (layout, lengths) and shared by the arms, which differ in switches only; every switch
is set through `monkeypatch`.  Every arm installs spies for the duration of its product call alone and compares what ran -- the
forward-only entry, the forward kernel's token count, query block, rotary fold and lse, the rotary passes, the last block's
attention, autograd nodes, device syncs -- with what the arm is named after (`_expected`: the gates of encoder.py / ops.py restated
on the arm's shapes).  Two injected defects (one row pooled a token early, two rows swapped) show that the harness fails, and at
which rows.  Every arm prints its worst row as a table row (profiles/llama_encode_parity.md holds a copy)."""
import collections
import re

import pytest
import torch

import llama_encode_parity_util as U

pytestmark = pytest.mark.gpu
DEV = U.DEV


class Spy:
    """Records what one product call ran.  Installed through a `monkeypatch` context of its own, so it is gone before anything else
    (a control, the next arm) runs."""

    def __init__(self, m):
        from rankpo_amd import encoder as PE, ops
        self.n, self.fwd, self.syncs = collections.Counter(), [], []

        def count(obj, name, key, record=None):
            real = getattr(obj, name)

            def spy(*a, **kw):
                self.n[key] += 1
                if record is not None:
                    record(*a, **kw)
                return real(*a, **kw)
            m.setattr(obj, name, spy)
        count(ops, "rope_flash_attn_varlen_qkv_fwd", "fused")
        count(ops, "flash_attn_varlen_fwd", "fwd", lambda q, *a, **kw: self.fwd.append(
            (q.shape[0], kw.get("q_block", 128), kw.get("rope") is not None, bool(kw.get("want_lse", True)))))
        count(ops, "rope_", "rope_")
        count(ops, "last_query_attn", "lastq")
        count(PE, "_varlen_last_query_attention", "lastq_fallback")
        count(ops, "rope_flash_attn_varlen_qkv", "node")             # the autograd nodes of the training path (FOLD_ROPE >= 1, 0)
        count(ops, "flash_attn_varlen_qkv", "node")
        count(PE.LlamaLayer, "forward_last_rows", "last_rows")
        for name in ("tolist", "item", "cpu"):                       # what reads a device tensor's contents on the host

            def sync(t, *a, _real=getattr(torch.Tensor, name), _name=name, **kw):
                if t.is_cuda:
                    self.syncs.append(_name)
                return _real(t, *a, **kw)
            m.setattr(torch.Tensor, name, sync)

    def summary(self):
        n = self.n
        return dict(fused=n["fused"], fwd=self.fwd, rope_=n["rope_"], lastq=n["lastq"], lastq_fallback=n["lastq_fallback"],
                    last_rows=n["last_rows"], node=n["node"], syncs=self.syncs)


SW = dict(fold=2, one_wave=True, fill=True)


def _apply(monkeypatch, c, sw):
    from rankpo_amd import encoder as PE
    monkeypatch.setattr(PE, "FOLD_ROPE", sw["fold"])
    monkeypatch.setattr(PE, "FWD128_ONE_WAVE", sw["one_wave"])
    monkeypatch.setattr(c.enc, "pack_fill", sw["fill"])


def _expected(c, sw, packs=None, host=True):
    """What the product must run on case `c` under the switches `sw`, from the gates of encoder.py / ops.py restated on the shapes.
    packs: the real token count of every packed pass, in order (None: one pass over all rows); host: host batches (no sync)."""
    from rankpo_amd import ops
    cfg = c.cfg
    full, hd, rep = cfg.num_hidden_layers - 1, cfg.head_dim, cfg.num_attention_heads // cfg.num_key_value_heads
    packs = [c.tot] if packs is None else packs
    if c.storage != "bf16":          # no hand-written encoder kernel takes fp16: PyTorch's rotary, flash-attention ops and no filler
        return dict(fused=0, fwd=[], rope_=0, lastq=0, lastq_fallback=len(packs), last_rows=len(packs), node=0,
                    syncs=[] if host else ["tolist"] * len(packs))
    Ts = [t + U.n_fill(t, sw["fill"]) for t in packs]
    q_block = 64 if (sw["one_wave"] and hd in ops.FWD_ONE_WAVE_HEAD_DIMS and rep % 4 == 0) else 128
    lastq_ok = rep in (1, 2, 4)
    fold = bool(sw["fold"])
    return dict(fused=len(Ts) * full if fold else 0,
                fwd=[(T, q_block, fold, False) for T in Ts for _ in range(full)],
                rope_=len(Ts) * (2 + (0 if fold else full)),
                lastq=len(Ts) if lastq_ok else 0, lastq_fallback=0 if lastq_ok else len(Ts), last_rows=len(Ts), node=0,
                syncs=[] if host else ["tolist"] * len(Ts))


# ------------------------------------------------------------------------------------------------------------------------------
# the entry points: each returns the unit rows [N, d] of case `c` in input order, on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _encode(c, texts=None, **kw):
    return c.inf.encode(c.texts if texts is None else texts, max_length=U.MAX_LENGTH, convert_to_numpy=False,
                        **dict(dict(batch_size=64), **kw))


def _pooled_device(c):
    with torch.no_grad():
        return U.pooled_rows(c.enc, c.dev_tok["input_ids"], c.dev_tok["attention_mask"])


def _split(c, nq=8):
    """Rows 0 .. nq - 1 as the query batch at ITS padded width, the rest as the passage batch: two widths in one pack."""
    ids, m = c.dev_tok["input_ids"], c.dev_tok["attention_mask"]
    wq = max(c.lens[:nq])
    assert wq < ids.shape[1]
    return {"query": {"input_ids": ids[:nq, :wq].contiguous(), "attention_mask": m[:nq, :wq].contiguous()},
            "passage": {"input_ids": ids[nq:].contiguous(), "attention_mask": m[nq:].contiguous()}}


def _eval_training(c):
    import rankpo_amd
    model = rankpo_amd.ModelForTraining(encoder=c.enc, temperature=0.02).eval()
    with torch.no_grad():
        out = model(**_split(c))
    assert out.loss is None and out.scores.shape == (8, c.rows - 8)
    return torch.cat([out.q_reps, out.p_reps], 0)


def _ref_model(c):
    import rankpo_amd
    grad = [p.requires_grad for p in c.enc.parameters()]
    try:
        tr = rankpo_amd.RankPOTrainer(None, c.enc)                  # freezes its ref_model: undone below, the case is shared
        with torch.inference_mode():
            q, p = tr._embed_pair(tr.ref_model, _split(c))
    finally:
        for p_, g in zip(c.enc.parameters(), grad):
            p_.requires_grad_(g)
    return torch.cat([q, p], 0)


ENTRY = {"encode": (_encode, True), "pooled_last_token": (_pooled_device, False), "eval ModelForTraining": (_eval_training, False),
         "ref_model": (_ref_model, False)}


def _run_arm(monkeypatch, name, c, over=None, run=_encode, packs=None, host=True, rows=None):
    """One product call under the switches `over` with the spies on; the rule on its rows (`rows`: the case's rows it returns)."""
    sw = dict(SW, **(over or {}))
    _apply(monkeypatch, c, sw)
    with monkeypatch.context() as m:
        spy = Spy(m)
        fast = run(c)
        got = spy.summary()
    torch.cuda.synchronize()
    want = _expected(c, sw, packs, host)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"arm {name}: the branches it is named after did not run as stated (got, expected): {wrong}"
    sel = list(range(c.rows)) if rows is None else rows
    print()
    fails = U.rule(c.ref[sel], fast.float().cpu(), c.eager[sel], c.flash[sel] if c.flash is not None else None,
                   [c.lens[i] for i in sel], arm=name)
    return fails, fast


_ids = lambda arms: [re.sub(r"[^A-Za-z0-9]+", "_", a[0]).strip("_") for a in arms]


def test_entry_points_meet_the_rule_and_give_bit_equal_rows(monkeypatch):
    """FILL at hd64 through the four no-grad entry points: same kernels on the same shapes -- only the index upload (one pinned
    int32 upload of a host batch, int64 indices of a device batch) and the grad-mode flavour (`no_grad`, `inference_mode`) differ."""
    c = U.case_s("hd64", "FILL")
    rows = {}
    for name, (run, host) in ENTRY.items():
        fails, rows[name] = _run_arm(monkeypatch, f"{name}, FILL hd64", c, run=run, host=host)
        assert not fails, fails
        assert rows[name].dtype == torch.bfloat16 and rows[name].is_cuda and rows[name].shape == c.ref.shape
    for name in ENTRY:
        assert torch.equal(rows[name], rows["encode"]), \
            (name, (rows[name].float() - rows["encode"].float()).abs().amax(-1).nonzero().flatten().tolist())


ARMS = [
    # 1. lengths at head_dim 64 (128-query forward) and 128 4/1 (the forward's own 64-query list): no filler, a filler of 128, the
    #    threshold met exactly, the filler switched off
    ("EDGES hd64", "hd64", "EDGES", {}), ("FILL hd64", "hd64", "FILL", {}), ("EXACT hd64", "hd64", "EXACT", {}),
    ("EDGES hd128 4/1", "hd128_g4", "EDGES", {}), ("FILL hd128 4/1", "hd128_g4", "FILL", {}), ("EXACT hd128 4/1", "hd128_g4", "EXACT", {}),
    ("pack_fill off, FILL hd64", "hd64", "FILL", dict(fill=False)),
    ("pack_fill off, FILL hd128 4/1", "hd128_g4", "FILL", dict(fill=False)),
    # 2. head layouts on FILL: 128 4/2 (the 128-query forward at head_dim 128), groups 1, 8 and 3 (8 and 3: `last_query_attn_ok`
    #    declines, the last block takes PyTorch's op)
    ("FILL hd128 4/2", "hd128_g2", "FILL", {}), ("FILL group 1 (4/4 hd128)", "g1", "FILL", {}),
    ("FILL group 8 (8/1 hd64)", "g8", "FILL", {}), ("FILL group 3 (6/2 hd64 d384)", "g3", "FILL", {}),
    # 3. FOLD_ROPE 0: a rotary pass of its own over q and k, then the forward kernel without the fold
    ("FOLD_ROPE=0 hd64", "hd64", "FILL", dict(fold=0)), ("FOLD_ROPE=0 hd128 4/1", "hd128_g4", "FILL", dict(fold=0)),
    ("FOLD_ROPE=0 hd128 4/2", "hd128_g2", "FILL", dict(fold=0)),
    # 4. FWD128_ONE_WAVE off: head_dim 128 4/1 on the 128-query list
    ("FWD128_ONE_WAVE off hd128 4/1", "hd128_g4", "FILL", dict(one_wave=False)),
]


@pytest.mark.parametrize("name,layout,which,over", ARMS, ids=_ids(ARMS))
def test_encode_every_row(monkeypatch, name, layout, which, over):
    """Config S (d 512, ff 1024, 4 blocks, llama3 rope) through `encode()` in one batch (host packing: no device sync)."""
    c = U.case_s(layout, which)
    if over.get("one_wave") is False:
        assert _expected(c, SW)["fwd"][0][1] == 64 and _expected(c, dict(SW, **over))["fwd"][0][1] == 128
    fails, _ = _run_arm(monkeypatch, name, c, over)
    assert not fails, fails


@pytest.mark.parametrize("layout", ["hd64", "hd128_g4"])
def test_fold_rope_1_is_the_default_arm_bit_for_bit(monkeypatch, layout):
    """Under no-grad FOLD_ROPE 1 takes the branch FOLD_ROPE 2 takes (the forward-only entry always folds the q rotation)."""
    c = U.case_s(layout, "FILL")
    fails, default = _run_arm(monkeypatch, f"FOLD_ROPE=2 {layout}", c, dict(fold=2))
    assert not fails, fails
    fails, one = _run_arm(monkeypatch, f"FOLD_ROPE=1 {layout}", c, dict(fold=1))
    assert not fails, fails
    assert torch.equal(one, default)


def test_encode_batches_and_buckets_return_rows_in_input_order(monkeypatch):
    """`encode(batch_size=6)` on FILL: three packs of 322 / 1088 / 2814 tokens, none at the filler's threshold; with
    `bucket_by_length` the packs are formed over the rows sorted by length (3068 / 960 / 196 tokens) and the rows come back in
    input order; a single string comes back as one row."""
    c = U.case_s("hd64", "FILL")
    fails, _ = _run_arm(monkeypatch, "encode(batch_size=6), FILL hd64", c, run=lambda c: _encode(c, batch_size=6),
                        packs=[322, 1088, 2814])
    assert not fails, fails
    fails, _ = _run_arm(monkeypatch, "encode(batch_size=6, bucket_by_length), FILL hd64", c,
                        run=lambda c: _encode(c, batch_size=6, bucket_by_length=True), packs=[3068, 960, 196])
    assert not fails, fails
    for r in (9, 0):
        one = {}
        fails, _ = _run_arm(monkeypatch, f"encode(str), row {r} of FILL hd64", c, packs=[c.lens[r]], rows=[r],
                            run=lambda c: one.setdefault("x", _encode(c, c.texts[r]))[None])
        assert not fails, fails
        assert one["x"].shape == (c.cfg.hidden_size,)


def test_fp16_storage_runs_no_hand_written_encoder_kernel(monkeypatch):
    """`use_fp16`: PyTorch's rotary and flash-attention ops, no filler (`_expected`: every hand-written count is zero).  The rule
    against the eager fp16 control alone."""
    c = U.case_s("hd64", "FILL", "fp16")
    assert c.flash is None and next(c.enc.parameters()).dtype == torch.float16
    fails, fast = _run_arm(monkeypatch, "fp16 storage, FILL hd64", c)
    assert fast.dtype == torch.float16
    assert not fails, fails


def test_spies_notice_an_arm_that_ran_another_branch(monkeypatch):
    """The spies are not vacuous: the same call with the hand-written attention switched off (the stock-flash control's branch) is
    refused as not being the arm it is named after."""
    c = U.case_s("hd64", "EDGES")
    monkeypatch.setattr(c.enc, "hand_attention", False)
    with pytest.raises(AssertionError, match="did not run as stated") as e:
        _run_arm(monkeypatch, "EDGES hd64, hand_attention off", c)
    assert all(k in str(e.value) for k in ("fused", "fwd", "rope_", "lastq")), str(e.value)


CASES = sorted({(a[1], a[2]) for a in ARMS})


def test_control_spread_is_inside_the_per_row_factor():
    """The two controls alone, over every (layout, lengths) case of this file: the largest per-row ratio of their errors either way.
    A per-row factor below it would fail a correct fast path that merely rounds like the other control; the factor in force is
    U.ROW_FACTOR (1.25 x the spread measured on one MI355X where that exceeds 1.2, never above 2.0)."""
    print()
    worst = 0.0
    for layout, which in CASES:
        c = U.case_s(layout, which)
        s, row = U.control_spread(c.ref, c.eager, c.flash)
        ee, el = U.row_errors(c.eager, c.ref), U.row_errors(c.flash, c.ref)
        print(f"| {which} {layout} | spread {s:.3f} at row {row} ({c.lens[row]}) | eager rms {U.rms(ee):.3e} min {min(ee):.3e} max "
              f"{max(ee):.3e} | flash rms {U.rms(el):.3e} min {min(el):.3e} max {max(el):.3e} |")
        worst = max(worst, s)
    print(f"largest control-against-control spread {worst:.3f}; per-row factor in force {U.ROW_FACTOR:.4f}")
    assert worst <= U.ROW_FACTOR <= U.ROW_FACTOR_CAP


# ------------------------------------------------------------------------------------------------------------------------------
# the harness must be able to fail: two defects injected at the Python level, with valid indices, on top of the real kernels
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,row", [("hd64", 7), ("hd128_g4", 3), ("g8", 17)], ids=["hd64_row7", "hd128_row3", "g8_row17"])
def test_injected_early_pooled_token_is_reported_at_its_row(monkeypatch, layout, row):
    """`forward_last_rows` receives a `last_idx` whose entry for one row of length >= 2 is the token BEFORE its last."""
    from rankpo_amd import encoder as PE
    c = U.case_s(layout, "FILL")
    assert c.lens[row] >= 2
    real = PE.LlamaLayer.forward_last_rows

    def bad(layer, x, delta, rope, ctx, last_idx):
        li = last_idx.clone()
        li[row] -= 1
        return real(layer, x, delta, rope, ctx, li)
    monkeypatch.setattr(PE.LlamaLayer, "forward_last_rows", bad)
    fast = _encode(c)
    print()
    fails = U.rule(c.ref, fast.float().cpu(), c.eager, c.flash, c.lens, arm=f"defect A: row {row} pooled one token early, {layout}")
    assert [(r["kind"], r["row"], r["len"]) for r in fails if r["kind"] != "rms"] == [("row", row, c.lens[row])], fails


def test_injected_swapped_rows_are_reported_at_those_two_rows(monkeypatch):
    """The pooled rows of two sequences come back swapped."""
    from rankpo_amd import encoder as PE
    c = U.case_s("hd64", "FILL")
    a, b = 4, 12
    real = PE.LlamaEncoder.pooled_last_token_multi

    def bad(enc, batches):
        out = real(enc, batches)
        perm = list(range(out[0].shape[0]))
        perm[a], perm[b] = b, a
        return [out[0][perm]] + out[1:]
    monkeypatch.setattr(PE.LlamaEncoder, "pooled_last_token_multi", bad)
    fast = _encode(c)
    print()
    fails = U.rule(c.ref, fast.float().cpu(), c.eager, c.flash, c.lens, arm=f"defect B: rows {a} and {b} swapped, hd64")
    assert [(r["kind"], r["row"]) for r in fails if r["kind"] != "rms"] == [("row", a), ("row", b)], fails
