"""Host side of the BERT / XLM-R encode parity (tests/bert_encode_parity_util.py): the rule on hand-made arrays -- it passes a
correct perturbation, reports exactly the moved row and exactly the two swapped rows, gives a missing, a non-finite and an extra
row their kinds, its guard fires when the controls disagree, it refuses a per-row factor above the cap, and its floors follow
the storage type --, the float64 oracle run one sequence at a time equals the padded one, every jittered bias and LayerNorm tensor
moves the float64 rows (key biases: provably not, see there), EDGES covers the tile edges, the last position row and a
non-identity work-list order, `bert_pack` hands the token types of the packed tokens to the kernels as the oracle reads them, and
the oracle's LayerNorm on 16-bit storage rounds once, as nn.LayerNorm does."""
import pytest
import torch

import bert_encode_parity_util as U

LENS = [1, 2, 31, 32, 33, 512]
D = 32


def _ref():
    g = torch.Generator().manual_seed(0)
    r = torch.randn(len(LENS), D, generator=g, dtype=torch.float64)
    return r / r.norm(dim=-1, keepdim=True)


def _off(ref, err, seed, rows=None):
    """The reference with every row (or the rows of `rows`: {row: err}) moved by an L2 distance of `err`."""
    g = torch.Generator().manual_seed(seed)
    e = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    e = e / e.norm(dim=-1, keepdim=True)
    scale = torch.full((ref.shape[0], 1), float(err), dtype=torch.float64)
    for r, v in (rows or {}).items():
        scale[r] = v
    return ref + scale * e


def _rule(ref, fast, eager, padded, storage="bf16", **kw):
    """The rule at the per-row factor 1.5 the hand-made figures below are laid out for (None: the factor in force)."""
    lines = []
    kw.setdefault("row_factor", 1.5)
    return U.rule(ref, fast, eager, padded, LENS, storage, arm="host", out=lines.append, **kw), lines


def test_rule_passes_a_correct_perturbation():
    ref = _ref()
    eager, padded = _off(ref, 8e-3, 1), _off(ref, 6e-3, 2)
    for fast in (_off(ref, 0.0, 3), _off(ref, 6e-3, 3), _off(ref, 1.2e-2, 3)):       # bound: 1.5 x 8e-3 + 1e-4 = 1.21e-2
        fails, lines = _rule(ref, fast, eager, padded)
        assert fails == [], fails
        assert len(lines) == 1 and lines[0].startswith("| host | ")                  # the worst row, as a table row
    assert _rule(ref, _off(ref, 6e-3, 3).float().bfloat16().float().numpy(), eager, padded)[0] == []


def test_rule_reports_exactly_the_moved_row_and_exactly_the_two_swapped_rows():
    ref = _ref()
    eager, padded = _off(ref, 8e-3, 1), _off(ref, 6e-3, 2)
    fails, lines = _rule(ref, _off(ref, 6e-3, 3, rows={4: 1.3e-2}), eager, padded)   # over 1.21e-2; the RMS stays inside 1.5 x
    assert [(r["kind"], r["row"], r["len"]) for r in fails] == [("row", 4, 33)], fails
    assert any("FAIL" in ln and "row 4 (length 33)" in ln for ln in lines) and lines[0].startswith("| host | 4 (33) |")
    fast = _off(ref, 6e-3, 3)
    fast[[1, 5]] = fast[[5, 1]]
    fails, _ = _rule(ref, fast, eager, padded)
    assert [(r["kind"], r["row"]) for r in fails if r["kind"] != "rms"] == [("row", 1), ("row", 5)], fails


@pytest.mark.parametrize("how", ["fewer", "nan", "extra", "width", "none"])
def test_rule_gives_a_missing_a_non_finite_and_an_extra_row_their_kind(how):
    ref = _ref()
    eager, padded = _off(ref, 8e-3, 1), _off(ref, 6e-3, 2)
    fast = _off(ref, 6e-3, 3)
    N = len(LENS)
    if how == "fewer":
        fails, want = _rule(ref, fast[:-1], eager, padded)[0], [("missing", N - 1)]
    elif how == "nan":
        fast[3, 5] = float("nan")
        fails, want = _rule(ref, fast, eager, padded)[0], [("nonfinite", 3)]
    elif how == "extra":
        fails, want = _rule(ref, torch.cat([fast, fast[:1]]), eager, padded)[0], [("extra", N)]
    elif how == "width":
        fails, want = _rule(ref, fast[:, :-1], eager, padded)[0], [("shape", i) for i in range(N)]
    else:
        fails, want = _rule(ref, None, eager, padded)[0], [("missing", i) for i in range(N)]
    assert [(r["kind"], r["row"]) for r in fails] == want, fails


def test_guard_fires_when_the_controls_disagree():
    """A glue defect shared by the fast path and the padded control (both run the product's embeddings and weights): the bound
    follows the inflated control and says nothing, the comparison with the oracle's own eager code names the row."""
    ref = _ref()
    eager = _off(ref, 8e-3, 1)
    padded, fast = _off(ref, 6e-3, 2, rows={5: 8e-2}), _off(ref, 6e-3, 3, rows={5: 8e-2})
    fails, _ = _rule(ref, fast, eager, padded)
    assert [(r["kind"], r["row"], r["len"]) for r in fails if r["kind"] != "rms"] == [("guard", 5, 512)], fails
    padded, fast = _off(ref, 6e-3, 2, rows={5: 1.9e-2}), _off(ref, 6e-3, 3, rows={5: 1.9e-2})        # 2.5 x 8e-3 = 2e-2
    assert _rule(ref, fast, eager, padded)[0] == []
    assert [(r["kind"], r["row"]) for r in _rule(ref, fast, eager, padded[:-1])[0]] == [("control", 5)]


def test_per_row_factor_is_capped_and_the_floors_follow_the_storage_type():
    ref = _ref()
    eager, padded = _off(ref, 8e-3, 1), _off(ref, 6e-3, 2)
    fast = _off(ref, 6e-3, 3, rows={1: 1.5e-2})
    assert U.failed_rows(_rule(ref, fast, eager, padded)[0]) == [1]
    assert _rule(ref, fast, eager, padded, row_factor=2.0)[0] == []                  # 2 x 8e-3 + 1e-4
    with pytest.raises(ValueError, match="per-row factor"):
        _rule(ref, fast, eager, padded, row_factor=2.01)
    # the factor in force, per storage type: 1.5 up to a measured control spread of 1.2, else 1.25 x the spread, never above 2.0
    assert U.FACTOR == 1.5 and U.ROW_FACTOR_CAP == 2.0 and set(U.ROW_FACTOR) == set(U.MEASURED_CONTROL_SPREAD) == set(U.STORAGE)
    for storage, spread in U.MEASURED_CONTROL_SPREAD.items():
        assert U.ROW_FACTOR[storage] == min(1.5 if spread <= 1.2 else 1.25 * spread, 2.0) and U.ROW_FACTOR[storage] >= U.FACTOR
    edge = U.ROW_FACTOR["bf16"] * 8e-3 + 1e-4                                        # ... and it is the rule's default
    assert _rule(ref, _off(ref, 6e-3, 3, rows={1: 0.99 * edge}), eager, padded, row_factor=None)[0] == []
    assert U.failed_rows(_rule(ref, _off(ref, 6e-3, 3, rows={1: 1.01 * edge}), eager, padded, row_factor=None)[0]) == [1]
    # floors: bench_parity.step_parity's bf16 numbers times u / u_bf16
    assert U.floors("bf16") == (1e-4, 1e-5) and U.floors("fp16") == (1e-4 / 8, 1e-5 / 8)
    assert U.floors("f32") == (1e-4 * 2.0 ** -16, 1e-5 * 2.0 ** -16)
    # an f32 arm is not made vacuous by a bf16 floor: controls at 1e-6, a row at 2e-6 fails in f32 (and would pass under 1e-4)
    e6, p6 = _off(ref, 1e-6, 1), _off(ref, 8e-7, 2)
    fast = _off(ref, 1e-6, 3, rows={2: 2e-6})
    assert [(r["kind"], r["row"]) for r in _rule(ref, fast, e6, p6, "f32")[0]] == [("row", 2)]
    assert _rule(ref, fast, e6, p6, "bf16")[0] == []
    # ... and the f32 guard floor does not excuse a padded control 3 x the eager one
    assert [(r["kind"], r["row"]) for r in _rule(ref, _off(ref, 1e-6, 3), e6, _off(ref, 8e-7, 2, rows={0: 3e-6}), "f32")[0]] \
        == [("guard", 0)]


def test_edges_cover_the_tile_edges_the_last_position_row_and_a_non_identity_sort():
    order = U.check_edges()                     # asserts the three properties (and the positions through `bert_pack`)
    assert order[:3] == [18, 17, 16] and order != sorted(order)
    assert sum(U.EDGES) == 2755 and len(U.EDGES) == 20
    texts = U.make_texts(U.EDGES)
    assert texts[0] != texts[19] and U.tokenise(texts)["input_ids"].shape == (20, 512)
    ids, m, holes = U.holed(U.tokenise(texts), (9, 40, 1))
    assert sorted(holes) == list(range(2, 19)) and m.sum(-1).tolist() == [n - (n >= 3) for n in U.EDGES]
    assert int(ids[9, 40]) == 1 and int(m[9, 40]) == 1 and all(0 < c < U.EDGES[r] - 1 for r, c in holes.items())


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64"])
def test_per_sequence_float64_oracle_equals_the_padded_one(layout):
    cfg, sd = U.host_weights(layout, "bf16")
    tok = dict(U.tokenise(U.make_texts(U.EDGES)))
    one = U.reference_rows(sd, cfg.to_dict(), tok)
    assert one.dtype == torch.float64 and one.shape == (20, cfg.hidden_size)
    assert float((one.norm(dim=-1) - 1).abs().max()) < 1e-12
    pad = U.padded_reference_rows(sd, cfg.to_dict(), tok)
    worst = float((one - pad).norm(dim=-1).max())
    print(f"\nper-sequence against padded float64 oracle, {layout}: max row distance {worst:.2e}")
    assert worst <= 1e-12
    # holed masks (XLM-R: with the pad id on a real token): one row at a time at the padded width equals the one padded call
    tok["input_ids"], tok["attention_mask"], _ = U.holed(tok, (9, 40, cfg.pad_token_id) if layout.startswith("xlmr") else None)
    one_h = U.reference_rows(sd, cfg.to_dict(), tok, padded=True)
    assert float((one_h - U.padded_reference_rows(sd, cfg.to_dict(), tok)).norm(dim=-1).max()) <= 1e-12
    moved = (one_h - one).norm(dim=-1)
    assert bool((moved[2:19] > 1e-3).all()) and float(moved[[0, 1, 19]].max()) < 1e-12         # a hole changes its row, and only it


@pytest.mark.parametrize("layout", ["bge_hd32", "xlmr_hd64"])
def test_every_jittered_bias_and_layernorm_tensor_moves_the_float64_rows(layout):
    """Each `*.bias`, LayerNorm weight / bias and the token-type table put back to its initial value (bias 0, LayerNorm weight 1,
    the table 0) on its own: every float64 row moves by more than the bf16 floor, so a glue defect that drops, swaps or
    mis-concatenates one is visible.  The two exceptions are exact: a KEY bias adds q . b_k to all scores of a query, which the
    softmax does not see -- asserted dead, so the k half of the fused q|k|v and k|v biases is known to be out of reach of any
    forward test (the value half and the weights of both are not); and a QUERY bias cannot move a one-token row."""
    cfg, sd = U.host_weights(layout, "f32")
    tok = dict(U.tokenise([t for t, n in zip(U.make_texts(U.EDGES), U.EDGES) if n <= 129]))
    if cfg.type_vocab_size == 2:
        tok["token_type_ids"] = U.token_types(tok)
    base = U.padded_reference_rows(sd, cfg.to_dict(), tok)
    names = [k for k in sd if U.JITTERED(k)]
    assert len(names) == 3 + 2 * 10 and all(k in names for k in ("embeddings.token_type_embeddings.weight",
                                                                 "encoder.layer.1.attention.self.value.bias"))
    floor = U.floors("bf16")[0]
    one_token = tok["attention_mask"].sum(-1) == 1
    assert int(one_token.sum()) == 2
    for k in names:
        reset = torch.ones_like(sd[k]) if k.endswith("LayerNorm.weight") else torch.zeros_like(sd[k])
        moved = (U.padded_reference_rows(dict(sd, **{k: reset}), cfg.to_dict(), tok) - base).norm(dim=-1)
        if k.endswith("attention.self.key.bias"):
            assert float(moved.max()) < 1e-12, (k, moved)
        elif k.endswith("attention.self.query.bias"):          # a one-token row has one key: its softmax is 1 whatever the score
            assert float(moved[~one_token].min()) > floor and float(moved[one_token].max()) < 1e-12, (k, moved)
        else:
            assert float(moved.min()) > floor, (k, moved)


def test_bert_pack_hands_over_the_token_types_the_oracle_reads():
    """With token types given, `bert_pack`'s `tts` are the types of the mask == 1 tokens row by row -- what the oracle's new
    `token_type_ids` argument selects for the same tokens -- and the oracle's default is type 0 for every token."""
    from rankpo_amd import encoder as PE
    from oracle import encoder_ref as E
    cfg, sd = U.host_weights("bge_hd32", "f32")
    tok = dict(U.tokenise(U.make_texts(U.EDGES[:8])))
    tok["input_ids"], tok["attention_mask"], _ = U.holed(tok)
    tts = U.token_types(tok)
    ids, pos, got, lens = PE.bert_pack(tok["input_ids"], tok["attention_mask"], tts)
    m = tok["attention_mask"].bool()
    assert got.dtype == torch.int64 and torch.equal(got, tts[m]) and torch.equal(ids, tok["input_ids"][m])
    assert lens == m.sum(-1).tolist() and set(got.tolist()) == {0, 1}
    assert PE.bert_pack(tok["input_ids"], tok["attention_mask"])[2] is None
    w = {k: v.double() for k, v in sd.items()}
    cd = cfg.to_dict()
    with torch.no_grad():
        none = E.embed(w, cd, tok, dtype=torch.float64)
        zeros = E.embed(w, cd, dict(tok, token_type_ids=torch.zeros_like(tts)), dtype=torch.float64)
        typed = E.embed(w, cd, dict(tok, token_type_ids=tts), dtype=torch.float64)
        # the oracle's embedding sum, restated on the packed tokens from `bert_pack`'s three outputs
        table = lambda n: w[f"embeddings.{n}.weight"]
        x = table("word_embeddings")[ids] + table("token_type_embeddings")[got] + table("position_embeddings")[pos]
        h = E.bert_forward(w, dict(cd, num_hidden_layers=0), tok["input_ids"], tok["attention_mask"], torch.float64, token_type_ids=tts)
    assert torch.equal(none, zeros) and float((typed - none).norm(dim=-1)[1:].min()) > 1e-3       # row 0: one token of type 0
    ln = E._ln(x, w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], cd["layer_norm_eps"])
    assert float((h[m] - ln).abs().max()) < 1e-12


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_oracle_layernorm_on_16_bit_storage_rounds_once(dtype):
    """`oracle.encoder_ref._ln` in 16-bit storage is nn.LayerNorm's arithmetic (float32 statistics and affine map, one rounding):
    within one unit in the last place of torch's own kernel on every element and equal on nearly all, and as close to float64 as
    that kernel is.  Rounding every elementwise step to the storage type gave 1.5 x the error, which no LayerNorm kernel has, and
    made the eager control of the encode parity a looser yardstick than the padded path it is paired with."""
    from oracle import encoder_ref as E
    g = torch.Generator().manual_seed(3)
    x = (2 * torch.randn(64, 384, generator=g)).to(dtype)
    w, b = (1 + 0.05 * torch.randn(384, generator=g)).to(dtype), (0.05 * torch.randn(384, generator=g)).to(dtype)
    got = E._ln(x, w, b, 1e-12)
    stock = torch.nn.functional.layer_norm(x.float(), (384,), w.float(), b.float(), 1e-12).to(dtype)
    ref = E._ln(x.double(), w.double(), b.double(), 1e-12)
    assert got.dtype == dtype
    ulp = torch.finfo(dtype).eps * ref.abs().clamp_min(2.0 ** -6)
    assert bool(((got.double() - stock.double()).abs() <= ulp).all()) and float((got == stock).float().mean()) > 0.99
    err, stock_err = (float((t.double() - ref).norm()) for t in (got, stock))
    assert err <= 1.01 * stock_err, (err, stock_err)
    # float32 and float64 inputs are untouched: the same expression as ever, in the input's type
    x32 = x.float()
    mu, var = x32.mean(-1, keepdim=True), ((x32 - x32.mean(-1, keepdim=True)) ** 2).mean(-1, keepdim=True)
    assert torch.equal(E._ln(x32, w.float(), b.float(), 1e-5), (x32 - mu) / torch.sqrt(var + 1e-5) * w.float() + b.float())
