"""Host side of the Llama encode parity (tests/llama_encode_parity_util.py): the rule on hand-made arrays -- it passes rows within
their bound and fails a row over its bound, a missing, non-finite or mis-shaped row under that row's index and length, its guard
fires when only the stock-flash control is off, and it refuses a per-row factor above the cap --, the float64 oracle run one
sequence at a time equals the padded one, the three length sets have the totals and filler sizes the GPU arms are named after, and
the product's float32 packed path on the host meets the float64 rows to float32 round-off."""
import pytest
import torch

import llama_encode_parity_util as U

LENS = [1, 2, 63, 64, 65, 300]
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
    return (ref + scale * e).float()


def _rule(ref, fast, eager, flash, **kw):
    """The rule at the per-row factor 1.5 the hand-made figures below are laid out for (None: the factor in force)."""
    lines = []
    kw.setdefault("row_factor", 1.5)
    return U.rule(ref, fast, eager, flash, LENS, arm="host", out=lines.append, **kw), lines


def test_rule_passes_rows_within_their_bound():
    ref = _ref()
    eager, flash = _off(ref, 7e-3, 1), _off(ref, 8e-3, 2)
    for fast in (_off(ref, 0.0, 3), _off(ref, 8e-3, 3), _off(ref, 1.2e-2, 3)):       # bound: 1.5 x 8e-3 + 1e-4 = 1.21e-2
        fails, lines = _rule(ref, fast, eager, flash)
        assert fails == [], fails
        assert len(lines) == 1 and lines[0].startswith("| host | ")                  # the worst row, as a table row
    # any float type, numpy included
    assert _rule(ref, _off(ref, 8e-3, 3).bfloat16().float().numpy(), eager, flash)[0] == []
    # without a stock-flash control the eager one alone sets the bound: 1.5 x 7e-3 + 1e-4
    assert _rule(ref, _off(ref, 1.05e-2, 3), eager, None)[0] == []
    assert U.failed_rows(_rule(ref, _off(ref, 1.1e-2, 3), eager, None)[0], "row") == list(range(len(LENS)))


def test_rule_reports_one_row_over_its_bound_by_index_and_length():
    ref = _ref()
    eager, flash = _off(ref, 7e-3, 1), _off(ref, 8e-3, 2)
    fast = _off(ref, 7e-3, 3, rows={4: 1.3e-2})                                      # over 1.21e-2; the RMS stays inside 1.5 x
    fails, lines = _rule(ref, fast, eager, flash)
    assert [(r["kind"], r["row"], r["len"]) for r in fails] == [("row", 4, 65)], fails
    assert abs(fails[0]["fast"] - 1.3e-2) < 1e-6 and abs(fails[0]["bound"] - 1.21e-2) < 1e-6
    assert any("FAIL" in ln and "row 4 (length 65)" in ln for ln in lines)
    assert lines[0].startswith("| host | 4 (65) |")
    # a row far off also moves the RMS over its bound: both are reported, the row by its index
    fails, _ = _rule(ref, _off(ref, 7e-3, 3, rows={2: 0.5}), eager, flash)
    assert [(r["kind"], r["row"]) for r in fails] == [("row", 2), ("rms", None)], fails
    # the RMS bound alone: every row inside 1.5 x its larger control but the case as a whole over 1.5 x the larger control RMS
    eager2 = _off(ref, 8e-3, 1, rows={0: 2e-3, 1: 2e-3, 2: 2e-3})
    flash2 = _off(ref, 2e-3, 2, rows={0: 8e-3, 1: 8e-3, 2: 8e-3})
    fails, _ = _rule(ref, _off(ref, 1.2e-2, 3), eager2, flash2)
    assert [(r["kind"], r["row"]) for r in fails if r["kind"] != "guard"] == [("rms", None)], fails


@pytest.mark.parametrize("how", ["none", "fewer", "nan", "inf", "width", "extra"])
def test_rule_reports_a_missing_non_finite_or_mis_shaped_row(how):
    ref = _ref()
    eager, flash = _off(ref, 7e-3, 1), _off(ref, 8e-3, 2)
    fast = _off(ref, 7e-3, 3)
    N = len(LENS)
    if how == "none":
        fails, _ = _rule(ref, None, eager, flash)
        want = [("missing", i) for i in range(N)]
    elif how == "fewer":
        fails, _ = _rule(ref, fast[:-1], eager, flash)
        want = [("missing", N - 1)]
    elif how in ("nan", "inf"):
        fast[3, 5] = float(how)
        fails, lines = _rule(ref, fast, eager, flash)
        want = [("nonfinite", 3)]
        assert any("row 3 (length 64)" in ln for ln in lines)
    elif how == "width":
        fails, _ = _rule(ref, fast[:, :-1], eager, flash)
        want = [("shape", i) for i in range(N)]
    else:                                                                            # e.g. a filler's row that was not dropped
        fails, _ = _rule(ref, torch.cat([fast, fast[:1]]), eager, flash)
        want = [("extra", N)]
    assert [(r["kind"], r["row"]) for r in fails] == want, fails
    assert all(r["eager"] is not None and r["flash"] is not None for r in fails if r["kind"] != "extra")


def test_guard_fires_when_only_the_stock_flash_control_is_off():
    """A glue defect shared by the fast path and the stock-flash control: the bound follows the inflated control and says nothing,
    the comparison of the two controls names the row."""
    ref = _ref()
    eager = _off(ref, 7e-3, 1)
    flash, fast = _off(ref, 8e-3, 2, rows={5: 8e-2}), _off(ref, 8e-3, 3, rows={5: 8e-2})
    fails, _ = _rule(ref, fast, eager, flash)
    assert [(r["kind"], r["row"], r["len"]) for r in fails if r["kind"] != "rms"] == [("guard", 5, 300)], fails
    # at 2.5 x the eager control the guard still holds
    flash, fast = _off(ref, 8e-3, 2, rows={5: 1.7e-2}), _off(ref, 8e-3, 3, rows={5: 1.7e-2})
    assert _rule(ref, fast, eager, flash)[0] == []
    # a control that lacks a row is a failure of its own, never a free pass
    assert [(r["kind"], r["row"]) for r in _rule(ref, fast, eager, flash[:-1])[0]] == [("control", 5)]
    bad = eager.clone()
    bad[0, 0] = float("nan")
    assert [(r["kind"], r["row"]) for r in _rule(ref, fast, bad, flash)[0]] == [("control", 0)]


def test_per_row_factor_is_capped():
    ref = _ref()
    eager, flash = _off(ref, 7e-3, 1), _off(ref, 8e-3, 2)
    fast = _off(ref, 7e-3, 3, rows={1: 1.5e-2})
    assert U.failed_rows(_rule(ref, fast, eager, flash)[0]) == [1]
    assert _rule(ref, fast, eager, flash, row_factor=2.0)[0] == []                   # 2 x 8e-3 + 1e-4
    with pytest.raises(ValueError, match="per-row factor"):
        _rule(ref, fast, eager, flash, row_factor=2.01)
    assert U.FACTOR == 1.5 and U.FACTOR <= U.ROW_FACTOR <= U.ROW_FACTOR_CAP == 2.0
    # the factor in force is the default
    edge = U.ROW_FACTOR * 8e-3 + 1e-4
    assert _rule(ref, _off(ref, 7e-3, 3, rows={1: 0.99 * edge}), eager, flash, row_factor=None)[0] == []
    assert U.failed_rows(_rule(ref, _off(ref, 7e-3, 3, rows={1: 1.01 * edge}), eager, flash, row_factor=None)[0]) == [1]
    assert (U.FLOOR, U.GUARD, U.GUARD_FLOOR) == (1e-4, 2.5, 1e-5)
    # the widest per-row factor leaves the RMS factor at 1.5
    fails, _ = _rule(ref, _off(ref, 1.5e-2, 3), eager, flash, row_factor=2.0)
    assert [(r["kind"], r["row"]) for r in fails] == [("rms", None)], fails


def test_control_spread_is_the_largest_per_row_ratio_either_way():
    ref = _ref()
    eager, flash = _off(ref, 7e-3, 1, rows={2: 3.5e-3}), _off(ref, 7e-3, 2, rows={4: 5e-3})
    s, row = U.control_spread(ref, eager, flash)
    assert row == 2 and abs(s - 2.0) < 1e-3                                          # rows 2: 7 / 3.5, 4: 7 / 5


def test_totals_filler_sizes_and_texts():
    assert (sum(U.EDGES), sum(U.FILL), sum(U.EXACT)) == (2224, 4224, 4096)
    assert (U.n_fill(2224), U.n_fill(4224), U.n_fill(4096), U.n_fill(4224, pack_fill=False)) == (0, 128, 0, 0)
    assert U.n_fill(4095) == 0 and U.n_fill(4097) == 255
    assert U.EDGES[0] == U.EDGES[-1] == 1 and U.FILL[:16] == U.EDGES and U.EXACT[:17] == U.FILL[:17]
    for b in (64, 128):                                                              # every tile edge up to 256, one below, one above
        assert all({k - 1, k, k + 1} <= set(U.EDGES) for k in range(b, 257, b))
    # encode(batch_size=6) on FILL: three packs, none at the filler's threshold, in input order and sorted by length
    packs = [sum(U.FILL[i:i + 6]) for i in range(0, 18, 6)]
    assert packs == [322, 1088, 2814] and max(packs) < U.FILL_FROM
    by_len = sorted(U.FILL, reverse=True)
    assert [sum(by_len[i:i + 6]) for i in range(0, 18, 6)] == [3068, 960, 196]
    for lens in U.LENGTHS.values():
        texts = U.make_texts(lens)
        tok = U.tokenise(texts)
        assert tok["attention_mask"].sum(-1).tolist() == lens and tok["input_ids"].shape == (len(lens), max(lens))
        assert int(tok["input_ids"].max()) < 2048 and texts[0] != texts[15]
    assert U.make_texts(U.FILL)[:17] == U.make_texts(U.EXACT)[:17] and U.make_texts(U.EDGES) == U.make_texts(U.FILL)[:16]


@pytest.mark.parametrize("layout", ["hd64", "g3"])
def test_per_sequence_float64_oracle_equals_the_padded_one(layout):
    cfg, sd = U.host_weights(layout, "bf16")
    texts = U.make_texts(U.EDGES)
    tok = U.tokenise(texts)
    one = U.cached_reference_rows(layout, "bf16", 0, tuple(texts))
    assert one.dtype == torch.float64 and one.shape == (16, cfg.hidden_size)
    assert float((one.norm(dim=-1) - 1).abs().max()) < 1e-12
    pad = U.padded_reference_rows(sd, cfg.to_dict(), tok)
    worst = float((one - pad).norm(dim=-1).max())
    print(f"\nper-sequence against padded float64 oracle, {layout}: max row distance {worst:.2e}")
    assert worst <= 1e-12
    assert torch.equal(one, U.reference_rows(sd, cfg.to_dict(), tok))                 # the per-text cache changes nothing


def test_product_f32_packed_path_on_the_host_meets_the_float64_rows():
    """The product's packed path (`pooled_last_token`: host packing, per-sequence attention, the last block on the pooled rows) in
    float32 on the host, on the bf16-held weights, against the float64 rows.  Bound: a correct bf16 row sits 6.3e-3 to 8.9e-3 from
    float64, i.e. 1.6 to 2.3 units of bf16 round-off (2^-8); float32 GEMMs also accumulate in float32, which for the longest
    reduction here (1024 terms) adds up to sqrt(1024) = 32 round-offs where bf16 GEMMs with float32 accumulators add none of their
    own: (2.3 + 32) x 2^-24 = 2.0e-6 per row."""
    from rankpo_amd import encoder as PE
    cfg, sd = U.host_weights("hd64", "bf16")
    enc = PE.LlamaEncoder(cfg)
    enc.load_state_dict({k: v.float() for k, v in sd.items()})
    enc.eval()
    texts = U.make_texts(U.EDGES)
    tok = U.tokenise(texts)
    ref = U.cached_reference_rows("hd64", "bf16", 0, tuple(texts))
    with torch.no_grad():
        pooled = enc.pooled_last_token(tok["input_ids"], tok["attention_mask"])
    assert pooled.dtype == torch.float32 and pooled.shape == ref.shape
    got = pooled.double() / pooled.double().norm(dim=-1, keepdim=True)                # the scoring ops run on a HIP device only
    errs = U.row_errors(got, ref)
    print("\nf32 packed host path against float64, per row: " + " ".join(f"{e:.1e}" for e in errs))
    assert all(isinstance(e, float) for e in errs) and max(errs) <= (2.3 + 32) * 2.0 ** -24, errs
