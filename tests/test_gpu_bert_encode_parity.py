"""The forward-only packed BERT / XLM-R path (`BertEncoder.pooled_cls`, `ModelForInference.encode()`), EVERY CLS row against
float64, on every arm of the glue around the kernels (rankpo_amd/encoder.py): the three entry points (`encode()`, `pooled_cls` on
host and on device tensors), bf16 / fp16 / f32 storage (f32 through `packed_f32` and through BERT_NATIVE_F32), 4 and 12 heads of
32 and 64, `encode()`'s batching and `bucket_by_length`, token types, holed masks (XLM-R: with a real token that carries the pad
id), a model without blocks.  Lengths sit on every 32-token tile edge and on the last row of the position table.

The models (every bias, LayerNorm parameter and the token-type table off its initial value), the float64 reference (one sequence
at a time), the two controls and the rule are tests/bert_encode_parity_util.py's.  Reference and controls are computed once per
(layout, storage, mask kind) and shared by the arms.  Every arm runs under a spy and compares what ran -- the four hand-written
entry points, the token and row counts of every pack and attention call, stock SDPA and nn.LayerNorm, device syncs -- with what
the arm is named after (`_expected`: the gates of encoder.py restated on the arm's shapes).  Injected defects (a CLS index one
token late, two CLS queries exchanged, the value half of the fused k|v bias dropped) show that the harness fails, and at which
rows.  Every arm prints its worst row as a table row (profiles/bert_encode_parity.md holds a copy)."""
import re

import pytest
import torch
import torch.nn.functional as F

import bert_encode_parity_util as U
from test_gpu_bert_native import Spy as NativeSpy

pytestmark = pytest.mark.gpu
DEV = U.DEV


@pytest.fixture(autouse=True)
def _stop_on_device_error():
    """A device error ends the session: nothing more is started on a GPU that has just faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                     # noqa: BLE001 -- whatever the runtime raises
        pytest.exit(f"device error, stopping: {e}", returncode=3)


class Spy(NativeSpy):
    """test_gpu_bert_native.Spy, which counts the four hand-written entry points, stock SDPA and nn.LayerNorm and the `tolist` /
    `item` of device tensors, plus: `cpu` of a device tensor as a sync, the packed token count of every `bert_embed_ln` call
    (`packs`) and the (query rows, key rows) of every `bidir_attn_fwd` call (`attn`)."""

    def __enter__(self):
        super().__enter__()
        from rankpo_amd import ops
        self.packs, self.attn = [], []
        embed, attn, self._cpu = ops.bert_embed_ln, ops.bidir_attn_fwd, torch.Tensor.cpu

        def embed_spy(ids, *a, **kw):
            self.packs.append(int(ids.shape[0]))
            return embed(ids, *a, **kw)

        def attn_spy(q, k, *a, **kw):
            self.attn.append((int(q.shape[0]), int(k.shape[0])))
            return attn(q, k, *a, **kw)

        def cpu(t, *a, **kw):
            self.n["syncs"] += int(t.is_cuda)
            return self._cpu(t, *a, **kw)
        ops.bert_embed_ln, ops.bidir_attn_fwd, torch.Tensor.cpu = embed_spy, attn_spy, cpu
        return self

    def __exit__(self, *exc):
        torch.Tensor.cpu = self._cpu
        return super().__exit__(*exc)                           # puts the real ops back

    def summary(self):
        return dict(self.n, packs=self.packs, attn=self.attn)


def _expected(c, packs, syncs=0):
    """What the product must run on case `c`, from the gates of encoder.py restated on the shapes.  packs: (rows, tokens) of every
    packed pass, in order.  `native_decline_reason` takes the model (16-bit storage, or f32 with a switch on; head_dim 32 or 64;
    d a multiple of 8); `pooled_cls` then runs one `bert_embed_ln` per pack, per block one attention call (all but the last block
    T queries on T keys, the last block the N CLS queries on T keys), two add + LayerNorm and one GELU; no stock SDPA or
    nn.LayerNorm; host tensors are packed on the host (no sync), device tensors cost one `cpu` each."""
    cfg = c.cfg
    nl, P = cfg.num_hidden_layers, len(packs)
    assert cfg.hidden_size // cfg.num_attention_heads in (32, 64) and cfg.hidden_size % 8 == 0
    return dict(bidir_attn_fwd=P * nl, add_layernorm=2 * P * nl, gelu_=P * nl, bert_embed_ln=P, sdpa=0, layernorm=0, syncs=syncs,
                packs=[T for _, T in packs], attn=[qk for N, T in packs for qk in [(T, T)] * (nl - 1) + [(N, T)] * min(nl, 1)])


# ------------------------------------------------------------------------------------------------------------------------------
# the entry points: each returns the unit rows [N, d] of case `c` in input order, on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _encode(c, inf=None, texts=None, **kw):
    return (inf or c.inf).encode(c.texts if texts is None else texts, max_length=U.MAX_LENGTH, convert_to_numpy=False,
                                 **dict(dict(batch_size=64), **kw))


def _pooled(c, tok=None, inf=None):
    """`pooled_cls` on `tok` (None: the case's host tensors, token types included if it has any), then `ops.pool_normalize`."""
    from rankpo_amd import ops
    tok = c.tok if tok is None else tok
    with torch.no_grad():
        pooled = (inf or c.inf).model.pooled_cls(tok["input_ids"], tok["attention_mask"], tok.get("token_type_ids"))
    assert pooled is not None
    return ops.pool_normalize(pooled[:, None, :], None, "cls", True)


def _run_arm(name, c, run=_encode, packs=None, syncs=0, rows=None):
    """One product call with the spy on; the rule on its rows (`rows`: the case's rows it returns)."""
    with Spy() as spy:
        fast = run(c)
    torch.cuda.synchronize()
    got = spy.summary()
    want = _expected(c, [(c.rows, c.tot)] if packs is None else packs, syncs)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"arm {name}: the branches it is named after did not run as stated (got, expected): {wrong}"
    sel = list(range(c.rows)) if rows is None else rows
    print()
    fails = U.rule(c.ref[sel], fast.float().cpu(), c.eager[sel], c.padded[sel], [c.lens[i] for i in sel], c.storage, arm=name)
    return fails, fast


def _same(a, b):
    assert torch.equal(a, b), (a.float() - b.float()).abs().amax(-1).nonzero().flatten().tolist()


_ids = lambda arms: [re.sub(r"[^A-Za-z0-9]+", "_", " ".join(map(str, a))).strip("_") for a in arms]
FAST_INF = lambda c: c.inf_on if c.storage == "f32" else c.inf            # the model whose `encode()` takes the packed path


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64"])
def test_entry_points_meet_the_rule_and_give_bit_equal_rows(layout):
    """`encode()` (host tensors: no sync), `pooled_cls` on host tensors followed by `ops.pool_normalize`, `pooled_cls` on device
    tensors (one `cpu` per tensor: packing is host work): the same kernels on the same shapes."""
    c = U.case_s(layout, "bf16")
    dev = {k: c.dev_tok[k] for k in ("input_ids", "attention_mask")}
    arms = {"encode()": (_encode, 0), "pooled_cls, host tensors": (_pooled, 0),
            "pooled_cls, device tensors": (lambda c: _pooled(c, dev), 2)}
    rows = {}
    for name, (run, syncs) in arms.items():
        fails, rows[name] = _run_arm(f"{name}, {layout} bf16", c, run=run, syncs=syncs)
        assert not fails, fails
        assert rows[name].dtype == torch.bfloat16 and rows[name].is_cuda and rows[name].shape == c.ref.shape
    for name in arms:
        _same(rows[name], rows["encode()"])


STORAGE_ARMS = [(layout, storage) for layout in ("bge_hd32", "xlmr_hd64", "bge_12x32", "xlmr_12x64") for storage in ("bf16", "fp16")]


@pytest.mark.parametrize("layout,storage", STORAGE_ARMS, ids=_ids(STORAGE_ARMS))
def test_encode_every_row_16_bit(layout, storage):
    c = U.case_s(layout, storage)
    fails, fast = _run_arm(f"encode(), {layout} {storage}", c)
    assert fast.dtype == U.STORAGE[storage]
    assert not fails, fails


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64", "xlmr_12x64"])
def test_encode_every_row_f32_by_either_switch(layout, monkeypatch):
    """`ModelForInference(packed_f32=True)` and BERT_NATIVE_F32 on a model without it: the same branch, bit-equal rows."""
    from rankpo_amd import encoder as PE
    c = U.case_s(layout, "f32")
    assert not PE.BERT_NATIVE_F32 and c.inf_on.model.native_f32 and not c.inf.model.native_f32
    fails, by_model = _run_arm(f"encode(), packed_f32, {layout} f32", c, run=lambda c: _encode(c, c.inf_on))
    assert by_model.dtype == torch.float32
    assert not fails, fails
    monkeypatch.setattr(PE, "BERT_NATIVE_F32", True)
    fails, by_switch = _run_arm(f"encode(), BERT_NATIVE_F32, {layout} f32", c)
    assert not fails, fails
    _same(by_switch, by_model)


def _packs(lens, order, batch_size):
    return [(len(order[i:i + batch_size]), sum(lens[r] for r in order[i:i + batch_size])) for i in range(0, len(order), batch_size)]


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64"])
def test_encode_batches_and_buckets_return_rows_in_input_order(layout):
    """`encode(batch_size=6)` on EDGES: four packs in input order; with `bucket_by_length` the packs are formed over the rows
    sorted by length, longest first, and the rows come back in input order; a single string comes back as one row of shape [d]."""
    c = U.case_s(layout, "bf16")
    N = c.rows
    packs = _packs(c.lens, list(range(N)), 6)
    assert packs == [(6, 162), (6, 544), (6, 1536), (2, 513)]
    fails, _ = _run_arm(f"encode(batch_size=6), {layout}", c, run=lambda c: _encode(c, batch_size=6), packs=packs)
    assert not fails, fails
    by_len = sorted(range(N), key=lambda i: -c.lens[i])
    packs = _packs(c.lens, by_len, 6)
    assert packs == [(6, 1920), (6, 608), (6, 225), (2, 2)] and by_len != list(range(N))
    fails, _ = _run_arm(f"encode(batch_size=6, bucket_by_length), {layout}", c,
                        run=lambda c: _encode(c, batch_size=6, bucket_by_length=True), packs=packs)
    assert not fails, fails
    for r in (9, 19):
        one = {}
        fails, _ = _run_arm(f"encode(str), row {r} of {layout}", c, packs=[(1, c.lens[r])], rows=[r],
                            run=lambda c: one.setdefault("x", _encode(c, texts=c.texts[r]))[None])
        assert not fails, fails
        assert one["x"].shape == (c.cfg.hidden_size,)


@pytest.mark.parametrize("storage", ["bf16", "f32"])
def test_token_types_reach_every_row(storage):
    """`pooled_cls(ids, mask, token_type_ids)` with a 0/1 pattern that differs per row, against the oracle given the same types;
    all types 0 is bit-equal to passing none."""
    c = U.case_s("bge_hd32", storage, "types")
    inf = FAST_INF(c)
    tts = c.tok["token_type_ids"]
    assert tts.shape == c.tok["input_ids"].shape and int(tts.max()) == 1 and bool((tts[:, 0] == torch.arange(c.rows) % 2).all())
    fails, _ = _run_arm(f"pooled_cls, token types, bge_hd32 {storage}", c, run=lambda c: _pooled(c, inf=inf))
    assert not fails, fails
    plain = U.case_s("bge_hd32", storage)
    none = {k: c.tok[k] for k in ("input_ids", "attention_mask")}
    fails, no_types = _run_arm(f"pooled_cls, no token types, bge_hd32 {storage}", plain, run=lambda c: _pooled(c, none, inf))
    assert not fails, fails
    fails, zeros = _run_arm(f"pooled_cls, token types all 0, bge_hd32 {storage}", plain,
                            run=lambda c: _pooled(c, dict(none, token_type_ids=torch.zeros_like(tts)), inf))
    assert not fails, fails
    _same(zeros, no_types)
    # the types matter: the rows of the pattern are not the rows without it
    typed = [r for r in range(c.rows) if bool(tts[r].any())]
    errs = U.row_errors(no_types.float().cpu(), c.ref)
    assert len(typed) >= c.rows - 2 and min(errs[r] for r in typed) > 0.05, errs


HOLED_ARMS = [(layout, storage) for layout in ("bge_hd32", "xlmr_hd64") for storage in ("bf16", "f32")]


@pytest.mark.parametrize("layout,storage", HOLED_ARMS, ids=_ids(HOLED_ARMS))
def test_holed_masks_take_their_positions_from_the_padded_layout(layout, storage):
    """One hole per row of length >= 3, at a different column per row: `bert_pack` drops the token and keeps the positions of the
    padded layout (BERT: the column; XLM-R: the running count of non-pad IDS, holes included).  XLM-R: row 9 also has a real token
    with the pad id, which takes position pad_id and is skipped by the count.  Reference: the oracle one sequence at a time at the
    padded width with the row's mask."""
    c = U.case_s(layout, storage, "holed")
    assert c.lens == [n - (n >= 3) for n in U.EDGES] and (c.pad_tok is not None) == layout.startswith("xlmr")
    if c.pad_tok is not None:
        r, col, v = c.pad_tok
        assert int(c.tok["input_ids"][r, col]) == v == c.cfg.pad_token_id and int(c.tok["attention_mask"][r, col]) == 1
    fails, _ = _run_arm(f"pooled_cls, holed mask, {layout} {storage}", c, run=lambda c: _pooled(c, inf=FAST_INF(c)))
    assert not fails, fails


def test_a_model_without_blocks_returns_the_embedding_rows():
    """`num_hidden_layers=0`: the rows are the normalised embedding-LayerNorm CLS rows; no attention, LayerNorm or GELU call."""
    c = U.case_s("bge_hd32_L0", "bf16")
    assert len(c.enc.encoder.layer) == 0
    want = _expected(c, [(c.rows, c.tot)])
    assert want["attn"] == [] and want["bidir_attn_fwd"] == want["add_layernorm"] == want["gelu_"] == 0 and want["bert_embed_ln"] == 1
    fails, _ = _run_arm("encode(), no blocks, bge_hd32 bf16", c)
    assert not fails, fails


def test_spies_notice_an_arm_that_ran_another_branch(monkeypatch):
    """The spies are not vacuous: the same call with BERT_NATIVE off (the padded control's branch) is refused as not being the arm
    it is named after."""
    from rankpo_amd import encoder as PE
    c = U.case_s("bge_hd32", "bf16")
    monkeypatch.setattr(PE, "BERT_NATIVE", False)
    with pytest.raises(AssertionError, match="did not run as stated") as e:
        _run_arm("encode(), BERT_NATIVE off", c)
    assert all(k in str(e.value) for k in ("bidir_attn_fwd", "add_layernorm", "gelu_", "bert_embed_ln", "sdpa", "layernorm")), str(e.value)


CASES = ([(l, s, "plain") for l, s in STORAGE_ARMS] + [(l, "f32", "plain") for l in ("bge_hd32", "xlmr_hd64", "xlmr_12x64")]
         + [(l, s, "holed") for l, s in HOLED_ARMS] + [("bge_hd32", "bf16", "types"), ("bge_hd32", "f32", "types"),
                                                      ("bge_hd32_L0", "bf16", "plain")])


@pytest.mark.parametrize("storage", ["bf16", "fp16", "f32"])
def test_control_spread_is_inside_the_per_row_factor(storage):
    """The two controls alone, over every case of this file in `storage`: the largest per-row ratio of their errors either way.  A
    per-row factor below it would fail a correct fast path that merely rounds like the other control; the factor in force is
    U.ROW_FACTOR[storage] (1.25 x the spread measured on one MI355X where that exceeds 1.2, never above 2.0).

    Per storage type because the rule is: the float32 controls differ by 1.08 to 1.30 per case, the 16-bit ones by 1.20 to 1.47.
    tests/bert_encode_parity_util.py and profiles/bert_encode_parity.md hold the figures."""
    print()
    worst = 0.0
    for layout, st, kind in CASES:
        if st != storage:
            continue
        c = U.case_s(layout, st, kind)
        s, row = U.control_spread(c.ref, c.eager, c.padded)
        ee, ep = U.row_errors(c.eager, c.ref), U.row_errors(c.padded, c.ref)
        print(f"| {layout} {st} {kind} | spread {s:.3f} at row {row} ({c.lens[row]}) | eager rms {U.rms(ee):.3e} min {min(ee):.3e} "
              f"max {max(ee):.3e} | padded rms {U.rms(ep):.3e} min {min(ep):.3e} max {max(ep):.3e} |")
        worst = max(worst, s)
    print(f"largest control-against-control spread in {storage} {worst:.3f}; per-row factor in force {U.ROW_FACTOR[storage]:.4f}")
    assert worst <= 1.02 * U.MEASURED_CONTROL_SPREAD[storage], "the recorded spread, which the factor is derived from, is out of date"
    assert worst <= U.ROW_FACTOR[storage] <= U.ROW_FACTOR_CAP


# ------------------------------------------------------------------------------------------------------------------------------
# the harness must be able to fail: defects injected at the Python level, with valid indices, on top of the real kernels
# ------------------------------------------------------------------------------------------------------------------------------
def _judge(c, fast, arm):
    print()
    return U.rule(c.ref, fast.float().cpu(), c.eager, c.padded, c.lens, c.storage, arm=arm)


@pytest.mark.parametrize("layout,row", [("bge_hd32", 7), ("xlmr_hd64", 1), ("xlmr_12x64", 18)],
                         ids=["bge_row7", "xlmr_row1", "12x64_row18"])
def test_injected_late_cls_index_is_reported_at_its_row(monkeypatch, layout, row):
    """(a) `_pack_upload`'s result with `cls_idx[row] += 1` for one row of length >= 2: the last block gathers that sequence's
    SECOND token as its CLS row.  The index stays inside the sequence."""
    from rankpo_amd import encoder as PE
    c = U.case_s(layout, "bf16")
    assert c.lens[row] >= 2
    real = PE.BertEncoder._pack_upload

    def bad(enc, *a, **kw):
        pk = real(enc, *a, **kw)
        idx = pk.cls_idx.clone()
        idx[row] += 1
        pk.cls_idx = idx
        return pk
    monkeypatch.setattr(PE.BertEncoder, "_pack_upload", bad)
    fails = _judge(c, _encode(c), f"defect (a): row {row} gathers its second token, {layout}")
    assert [(r["kind"], r["row"], r["len"]) for r in fails if r["kind"] != "rms"] == [("row", row, c.lens[row])], fails


def test_the_order_of_the_cls_work_list_is_free_but_exchanged_queries_are_reported_at_those_two_rows(monkeypatch):
    """(b) An entry of `tiles_cls` is (sequence, first query row); the kernel takes queries AND keys from the sequence's `cu`
    entries, so two entries with their sequence ids exchanged are the same two work items in another order: bit-equal rows (first
    half).  The defect such an exchange stands for -- sequence a's work item computing with sequence b's query and the reverse -- is
    injected where it can exist, in the CLS query rows handed to the last block's attention: exactly rows a and b are reported."""
    from rankpo_amd import encoder as PE, ops
    c = U.case_s("bge_hd32", "bf16")
    a, b = 4, 12
    assert c.lens[a] != c.lens[b]
    good = _encode(c)
    real = PE.BertEncoder._pack_upload
    order = ops.bidir_attn_tile_list([1] * c.rows, c.lens)[:, 0].tolist()
    ia, ib = order.index(a), order.index(b)

    def exchanged(enc, *args, **kw):
        pk = real(enc, *args, **kw)
        t = pk.tiles_cls.clone()
        t[ia, 0], t[ib, 0] = b, a
        pk.tiles_cls = t
        return pk
    with monkeypatch.context() as m:
        m.setattr(PE.BertEncoder, "_pack_upload", exchanged)
        _same(_encode(c), good)
    real_attn = ops.bidir_attn_fwd

    def bad(q, k, *args, **kw):
        if q.shape[0] == c.rows and k.shape[0] == c.tot:              # the last block: N CLS queries on all keys
            perm = list(range(c.rows))
            perm[a], perm[b] = b, a
            q = q[perm]
        return real_attn(q, k, *args, **kw)
    monkeypatch.setattr(ops, "bidir_attn_fwd", bad)
    fails = _judge(c, _encode(c), f"defect (b): the CLS queries of rows {a} and {b} exchanged, bge_hd32")
    assert [(r["kind"], r["row"]) for r in fails if r["kind"] != "rms"] == [("row", a), ("row", b)], fails


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64"])
def test_injected_dropped_value_bias_of_the_fused_kv_projection_is_reported(monkeypatch, layout):
    """(c) The value half of the last block's concatenated k|v bias zeroed through a wrapped `F.linear`: every row moves.  (The
    KEY half is dead by construction: a key bias adds q . b_k to every score of a query, and the softmax does not see it.)"""
    c = U.case_s(layout, "bf16")
    d = c.cfg.hidden_size
    real, hit = F.linear, []

    def bad(x, w, bias=None):
        if bias is not None and w.shape[0] == 2 * d and w.shape[1] == d:
            hit.append(x.shape[0])
            bias = torch.cat([bias[:d], torch.zeros_like(bias[d:])])
        return real(x, w, bias)
    monkeypatch.setattr(F, "linear", bad)
    fast = _encode(c)
    monkeypatch.setattr(F, "linear", real)
    assert hit == [c.tot]
    fails = _judge(c, fast, f"defect (c): the value bias of the fused k|v projection dropped, {layout}")
    assert "rms" in {r["kind"] for r in fails} or len(U.failed_rows(fails, "row")) >= 2, fails
