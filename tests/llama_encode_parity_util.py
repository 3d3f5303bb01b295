"""Every pooled row of the forward-only (no-grad) bf16 packed Llama path against a float64 oracle: the rule, its reference and controls.

The no-grad twin of tests/llama_step_parity_util.py.  `ModelForInference.encode()`, the RankPO ref_model under `inference_mode`
and eval-mode `ModelForTraining` take branches of the glue (rankpo_amd/encoder.py, ops.py) that a training step never takes: the
forward-only rotary + attention entry, the last block on the pooled rows, the host-side packing, the 256-token filler, `encode()`'s
batching.  A defect there moves ONE row (a wrong work list for one sequence, a `last_idx` off by one, rows in the wrong order), which
a maximum over all rows does not localise and an average over them dilutes.  This module judges every row on its own:

  reference  oracle/encoder_ref.py's `embed` in float64 on the model's 16-bit-held weights, ONE SEQUENCE AT A TIME, UNPADDED: it
             owes nothing to pad handling.  Unit rows in float64 (`reference_rows`).
  controls   on the same weights, on the device: (i) the oracle's eager code in the storage type, (ii) the product under no_grad
             with PyTorch's flash-attention ops (`hand_attention = False`).
  statistic  per row ||got - ref||_2 (ref is a unit row); over a case the RMS of these.
  bound      RMS: fast <= 1.5 * max(controls) + 1e-4.  Per row: fast <= ROW_FACTOR * max(controls) + 1e-4.
  guard      per row flash <= 2.5 * eager + 1e-5: control (ii) runs the product's own glue, a glue defect inflates it together with
             the fast path, and only this comparison with the oracle's own code sees that.

1.5, 2.5, 1e-4 and 1e-5 are `bench_parity.step_parity`'s numbers.  ROW_FACTOR: two correct bf16 implementations differ per row by
more than their RMS does.  On the host (bf16, config S, 34 rows, layouts hd64 and hd128 4/1) the oracle's eager code and the
product's packed path differ per row by a factor of at most 1.29 (median 1.10), hence 1.5.  On the device the spread is measured
from the two controls alone, `control_spread` (profiles/llama_encode_parity.md records it): above 1.2 the factor is 1.25 x the
measured spread, and never more than ROW_FACTOR_CAP = 2.0 -- if the controls alone need more, the case is ill-chosen.

Lengths: `test_gpu_inference.CharTok` gives one token per character, so texts of exact lengths give exact token counts.  EDGES puts
a row at every 64- and 128-token tile edge (and one below, one above), starts and ends with a one-token row, and the last row's
pooled token is the pack's final token; FILL crosses the filler's threshold off a multiple of 256 (a filler of 128 fires); EXACT
meets the threshold on a multiple of 256 (no filler).

Importable without a GPU (tests/test_llama_encode_parity_host.py runs the rule on hand-made arrays)."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from llama_step_parity_util import build_encoder, cfg_s
from oracle import encoder_ref as E
from test_gpu_inference import CharTok

FACTOR, FLOOR = 1.5, 1e-4                           # bench_parity.step_parity's bound (the RMS factor stays 1.5)
GUARD, GUARD_FLOOR = 2.5, 1e-5                      # ... and its guard
ROW_FACTOR_CAP = 2.0
# The per-row factor in force: 1.5 (the host spread of 1.29) unless the largest per-row spread of the two controls measured on
# the device over all cases exceeds 1.2; then 1.25 x that spread.  Measured on one MI355X over the ten (layout, lengths) cases of
# tests/test_gpu_llama_encode_parity.py: 1.354 (layout g3 on FILL, row 8 of 191 tokens; 1.270 to 1.354 per case), from the two
# controls alone -- profiles/llama_encode_parity.md holds the run.
MEASURED_CONTROL_SPREAD = 1.354
ROW_FACTOR = 1.25 * MEASURED_CONTROL_SPREAD if MEASURED_CONTROL_SPREAD > 1.2 else 1.5        # 1.6925
assert FACTOR <= ROW_FACTOR <= ROW_FACTOR_CAP

EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 1]
FILL = EDGES + [700, 1300]
EXACT = EDGES + [700, 1172]
LENGTHS = {"EDGES": EDGES, "FILL": FILL, "EXACT": EXACT}
FILL_FROM, FILL_TO = 4096, 256                      # `pooled_last_token_multi`: from 4096 packed tokens on, up to a multiple of 256
MAX_LENGTH = 2048                                   # the tokenizer's truncation, above every row
STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def n_fill(total, pack_fill=True):
    """The filler `LlamaEncoder.pooled_last_token_multi` appends to a bf16 pack of `total` tokens on the device."""
    return (-total) % FILL_TO if pack_fill and total >= FILL_FROM else 0


assert (sum(EDGES), sum(FILL), sum(EXACT)) == (2224, 4224, 4096)
assert (n_fill(sum(EDGES)), n_fill(sum(FILL)), n_fill(sum(EXACT))) == (0, 128, 0)
assert EDGES[0] == EDGES[-1] == 1


def make_texts(lens):
    """Row i: the first lens[i] characters of row i's own stream of letters, so the rows EDGES, FILL and EXACT share are the same
    texts (and the two one-token rows are different tokens)."""
    out = ["".join(chr(97 + int(c)) for c in np.random.RandomState(7000 + i).randint(0, 26, size=MAX_LENGTH)[:n])
           for i, n in enumerate(lens)]
    assert [len(t) for t in out] == list(lens) and len(set(out)) == len(out)
    return out


def tokenise(texts):
    tok = CharTok()(texts, max_length=MAX_LENGTH)
    assert tok["attention_mask"].sum(-1).tolist() == [len(t) for t in texts]
    return tok


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 reference: one sequence at a time, unpadded
# ------------------------------------------------------------------------------------------------------------------------------
def reference_rows(sd, cd, tok):
    """Float64 unit rows [N, d] of `oracle.encoder_ref.embed` on the weights `sd` holds (their values as they are), every sequence
    on its own at its own length."""
    w = {k: v.detach().to("cpu", torch.float64) for k, v in sd.items()}
    lens = tok["attention_mask"].sum(-1).tolist()
    rows = []
    with torch.no_grad():
        for i, n in enumerate(lens):
            one = {"input_ids": tok["input_ids"][i:i + 1, :n].cpu(), "attention_mask": tok["attention_mask"][i:i + 1, :n].cpu()}
            rows.append(E.embed(w, cd, one, dtype=torch.float64))
    return torch.cat(rows, 0)


def padded_reference_rows(sd, cd, tok):
    """The same rows from ONE padded call (the host test compares the two)."""
    w = {k: v.detach().to("cpu", torch.float64) for k, v in sd.items()}
    with torch.no_grad():
        return E.embed(w, cd, {k: v.cpu() for k, v in tok.items()}, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def host_weights(layout="hd64", storage="bf16", seed=0):
    """(config, the encoder's state dict in `storage` on the host): what a model built from `build_encoder(seed)` and cast holds."""
    from rankpo_amd import encoder as PE
    cfg = cfg_s(PE, layout)
    enc = build_encoder(PE, cfg, seed)
    return cfg, {k: v.detach().to(STORAGE[storage]) for k, v in enc.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _reference_row(layout, storage, seed, text):
    cfg, sd = host_weights(layout, storage, seed)
    return reference_rows(sd, cfg.to_dict(), tokenise([text]))[0]


def cached_reference_rows(layout, storage, seed, texts):
    """`reference_rows` with one cache entry per (weights, text): EDGES, FILL and EXACT share 16 or 17 of their rows."""
    return torch.stack([_reference_row(layout, storage, seed, t) for t in texts])


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
def row_errors(got, ref):
    """Per row of `ref` [N, d]: ||got_i - ref_i||_2 as a float, or why there is none: "missing" (no tensor, or fewer rows),
    "shape" (not [*, d]), "nonfinite"."""
    N, d = ref.shape
    if got is None:
        return ["missing"] * N
    g = torch.as_tensor(got).detach().to("cpu", torch.float64)
    if g.dim() != 2 or g.shape[1] != d:
        return ["shape"] * N
    out = []
    for i in range(N):
        if i >= g.shape[0]:
            out.append("missing")
        elif not bool(torch.isfinite(g[i]).all()):
            out.append("nonfinite")
        else:
            out.append(float((g[i] - ref[i]).norm()))
    return out


def rms(errs):
    """RMS of the per-row errors; None unless every row has one."""
    if not errs or any(not isinstance(e, float) for e in errs):
        return None
    return math.sqrt(sum(e * e for e in errs) / len(errs))


def control_spread(ref, eager, flash):
    """The largest per-row max(e_flash / e_eager, e_eager / e_flash) of the two controls, and its row."""
    ee, el = row_errors(eager, ref), row_errors(flash, ref)
    assert all(isinstance(e, float) and e > 0 for e in ee + el), (ee, el)
    s = [max(l / e, e / l) for e, l in zip(ee, el)]
    return max(s), s.index(max(s))


TABLE_HEAD = ("| arm | worst row (length) | err fast | err eager | err flash | bound | fast / larger control | rms fast | rms eager | "
              "rms flash |")


def rule(ref, fast, eager, flash, lens, arm="", row_factor=None, out=print, floor=FLOOR, guard_floor=GUARD_FLOOR):
    """The rule of the module docstring.  ref: float64 unit rows [N, d]; fast / eager / flash: [N, d] tensors (or arrays) of any
    float type; `flash` may be None (storage without hand-written attention has no such control); lens: the N token counts.
    `row_factor`: the per-row factor (None: ROW_FACTOR); above ROW_FACTOR_CAP it is refused.  `floor` / `guard_floor`: the additive
    terms of the bounds and of the guard (tests/bert_encode_parity_util.py scales them by the storage type's round-off).
    Returns the failures as dicts (kind: "row" over its bound, "missing" / "shape" / "nonfinite" = the fast path has no such row,
    "control" = a control has none, "guard" = the two controls disagree, "rms" = the case's RMS (row None), "extra" = more rows
    than sequences (row N); row, len; fast, eager, flash, bound) and prints one table row: the row that uses most of its bound."""
    row_factor = ROW_FACTOR if row_factor is None else row_factor
    if not row_factor <= ROW_FACTOR_CAP:
        raise ValueError(f"per-row factor {row_factor} > {ROW_FACTOR_CAP}: if the controls alone need more, change the case")
    N = ref.shape[0]
    assert len(lens) == N, (len(lens), N)
    ef, ee = row_errors(fast, ref), row_errors(eager, ref)
    el = row_errors(flash, ref) if flash is not None else None
    fails, worst = [], None
    for i in range(N):
        f, e, l = ef[i], ee[i], (el[i] if el is not None else None)
        rec = dict(row=i, len=lens[i], fast=f, eager=e, flash=l, bound=None)
        if not isinstance(e, float) or (el is not None and not isinstance(l, float)):
            fails.append(dict(rec, kind="control"))
            continue
        ctrl = max(e, l) if l is not None else e
        rec["bound"] = row_factor * ctrl + floor
        if not isinstance(f, float):
            fails.append(dict(rec, kind=f))
        else:
            if not f <= rec["bound"]:
                fails.append(dict(rec, kind="row"))
            if worst is None or f / rec["bound"] > worst["fast"] / worst["bound"]:
                worst = dict(rec, ratio=f / max(ctrl, 1e-300))
        if l is not None and not l <= GUARD * e + guard_floor:
            fails.append(dict(rec, kind="guard", bound=GUARD * e + guard_floor))
    got_rows = None if fast is None or torch.as_tensor(fast).dim() != 2 else int(torch.as_tensor(fast).shape[0])
    if got_rows is not None and got_rows > N:
        fails.append(dict(kind="extra", row=N, len=None, fast=float(got_rows), eager=None, flash=None, bound=float(N)))
    rf, re_, rl = rms(ef), rms(ee), (rms(el) if el is not None else None)
    if rf is not None and re_ is not None and (el is None or rl is not None):
        bound = FACTOR * max(re_, rl if rl is not None else 0.0) + floor
        if not rf <= bound:
            fails.append(dict(kind="rms", row=None, len=None, fast=rf, eager=re_, flash=rl, bound=bound))
    fmt = lambda x: "-" if x is None else (x if isinstance(x, str) else f"{x:.3e}")
    if worst is not None:
        out(f"| {arm} | {worst['row']} ({worst['len']}) | {fmt(worst['fast'])} | {fmt(worst['eager'])} | {fmt(worst['flash'])} | "
            f"{fmt(worst['bound'])} | {worst['ratio']:.2f} | {fmt(rf)} | {fmt(re_)} | {fmt(rl)} |")
    for r in fails:
        out(f"  FAIL [{arm}] {r['kind']} row {r['row']} (length {r['len']}): fast {fmt(r['fast'])} eager {fmt(r['eager'])} "
            f"flash {fmt(r['flash'])} bound {fmt(r['bound'])}")
    return fails


def failed_rows(fails, kind=None):
    return sorted({r["row"] for r in fails if kind is None or r["kind"] == kind}, key=lambda r: (r is None, r))


# ------------------------------------------------------------------------------------------------------------------------------
# one (layout, lengths, storage) case on the device: model, float64 reference and the controls, computed once, shared by every arm
# ------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def model_s(layout="hd64", storage="bf16", seed=0):
    """`ModelForInference` on config S in `layout`, its weights the ones `host_weights` holds (asserted)."""
    import rankpo_amd
    from rankpo_amd import encoder as PE
    cfg, sd = host_weights(layout, storage, seed)
    inf = rankpo_amd.ModelForInference(encoder=build_encoder(PE, cfg, seed), tokenizer=CharTok(), use_bf16=storage == "bf16",
                                       use_fp16=storage == "fp16", device=0)
    held = inf.model.state_dict()
    assert set(held) == set(sd) and all(held[k].dtype == STORAGE[storage] and torch.equal(held[k].cpu(), sd[k]) for k in sd)
    return inf


def pooled_rows(enc, ids, mask):
    """The product's unit rows through `pooled_last_token` (what every entry point does with the pooled rows)."""
    from rankpo_amd import ops
    pooled = enc.pooled_last_token(ids, mask)
    assert pooled is not None
    return ops.pool_normalize(pooled[:, None, :], None, "cls", True)


def eager_control(enc, cd, dev_tok):
    """Control (i): the oracle's eager code in the model's storage type on the device, on the model's weights."""
    wd = {k: v.detach() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        return E.embed(wd, cd, dev_tok, dtype=next(iter(wd.values())).dtype).float().cpu()


def flash_control(enc, dev_tok):
    """Control (ii): the product under no_grad with PyTorch's flash-attention ops."""
    assert enc.hand_attention
    enc.hand_attention = False
    try:
        with torch.no_grad():
            return pooled_rows(enc, dev_tok["input_ids"], dev_tok["attention_mask"]).float().cpu()
    finally:
        enc.hand_attention = True


@functools.lru_cache(maxsize=None)
def case_s(layout="hd64", which="FILL", storage="bf16", seed=0):
    lens = LENGTHS[which]
    inf = model_s(layout, storage, seed)
    enc, cfg = inf.model, inf.model.config
    texts = make_texts(lens)
    tok = tokenise(texts)
    dev_tok = {k: v.to(DEV) for k, v in tok.items()}
    ref = cached_reference_rows(layout, storage, seed, tuple(texts))
    assert ref.shape == (len(lens), cfg.hidden_size) and float((ref.norm(dim=-1) - 1).abs().max()) < 1e-12
    eager = eager_control(enc, cfg.to_dict(), dev_tok)
    flash = flash_control(enc, dev_tok) if storage == "bf16" else None
    tot = sum(lens)
    return SimpleNamespace(layout=layout, which=which, storage=storage, inf=inf, enc=enc, cfg=cfg, lens=list(lens), texts=texts,
                           tok=tok, dev_tok=dev_tok, ref=ref, eager=eager, flash=flash, tot=tot, rows=len(lens))
