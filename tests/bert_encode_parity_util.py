"""Every CLS row of the forward-only packed BERT / XLM-R path (`BertEncoder.pooled_cls`, reached from `ModelForInference.encode()`)
against a float64 oracle: the models, the lengths, the reference, the controls and the rule.

The BERT twin of tests/llama_encode_parity_util.py, whose per-row rule it imports.  The kernels have tests of their own
(test_gpu_bert_parity.py, test_gpu_bert_native.py, test_gpu_bert_f32.py); this module is about the glue around them in
rankpo_amd/encoder.py: `bert_pack`, the one int32 upload, `cu` / `cu_cls`, the two work lists sorted by key length, the `cls_idx`
gather, the last block (K / V for every token, the rest for the N CLS rows), the per-call `torch.cat` of the q|k|v and k|v weights
and biases, RoBERTa position ids, token types, `encode()`'s batching.  A defect there moves ONE row, or only shows with a bias or a
LayerNorm parameter off its initial value, so

  models     `build_encoder` on small configs (LAYOUTS), two blocks, intermediate = 4 d, vocab 1024; before any cast every `*.bias`,
             every LayerNorm weight / bias and the token-type table get += 0.05 randn from a seeded generator (`build_model`).
  lengths    `CharTok` gives one token per character.  EDGES puts a row at, below and above every multiple of 32 up to 128 (the
             attention's 32-query / 32-key tiles), at 256 and at the end of the position table (512 tokens: BERT position 511,
             XLM-R position 513), and starts and ends with a one-token row, so the longest-keys-first sort of the work lists is
             no identity (`check_edges`).
  reference  oracle/encoder_ref.py's `embed` in float64 on the weights as the model holds them, ONE SEQUENCE AT A TIME at its own
             length: unit rows that owe nothing to pad handling (`reference_rows`).  A holed mask takes its positions from the
             padded layout, so there it is one sequence at a time at the padded width with that row's mask (`padded=True`).
  controls   on the device on the same weights: (i) the oracle's eager code in the storage type, (ii) the product's padded
             PyTorch path (`encode()` with BERT_NATIVE off; float32: the model without `packed_f32`), its attention on SDPA's
             reproducible MATH backend (`padded_control` says why).
  rule       llama_encode_parity_util.rule: per row ||got - ref||_2 <= ROW_FACTOR[storage] max(controls) + floor, over a case RMS <= 1.5
             max(controls) + floor, guard per row padded <= 2.5 eager + guard_floor.  floor = 1e-4 u / u_bf16 and guard_floor =
             1e-5 u / u_bf16 with u = 2^-8 / 2^-11 / 2^-24 for bf16 / fp16 / f32: `bench_parity.step_parity`'s bf16 numbers scaled
             by the unit round-off, so that a bf16 floor does not make the f32 arms vacuous.

Importable without a GPU (tests/test_bert_encode_parity_host.py)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import llama_encode_parity_util as L
from llama_encode_parity_util import (FACTOR, GUARD, ROW_FACTOR_CAP, control_spread, failed_rows, rms,  # noqa: F401 -- re-exported
                                      row_errors)
from oracle import encoder_ref as E
from test_gpu_inference import CharTok

STORAGE = {"bf16": torch.bfloat16, "fp16": torch.float16, "f32": torch.float32}
UNIT = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11, "f32": 2.0 ** -24}            # unit round-off


def floors(storage):
    """(floor, guard_floor) of the rule for `storage`: the Llama util's bf16 numbers scaled by the unit round-off."""
    s = UNIT[storage] / UNIT["bf16"]
    return L.FLOOR * s, L.GUARD_FLOOR * s


# The per-row factor in force: 1.5 unless the largest per-row spread of the two controls alone, measured on the device over all the
# cases of tests/test_gpu_bert_encode_parity.py (`control_spread`), exceeds 1.2; then 1.25 x that spread, and never more than
# ROW_FACTOR_CAP = 2.0 -- if the controls alone need more, the case is ill-chosen.  profiles/bert_encode_parity.md holds the run.
#
# Measured on one MI355X over the 18 cases of that file, per storage type (the rule is per storage type), from the controls alone:
#   bf16  1.470 (bge_hd32, row 8 of 95 tokens; 1.201 to 1.470 per case)                                         -> factor 1.8375
#   fp16  1.446 (bge_12x32, row 17 of 511 tokens; 1.268 to 1.446 per case)                                      -> factor 1.8075
#   f32   1.304 (xlmr_hd64, row 1 of 2 tokens; 1.079 to 1.304 per case)                                         -> factor 1.63
# These are the figures with oracle.encoder_ref._ln keeping its 16-bit LayerNorm statistics in float32, as nn.LayerNorm does.  When
# it rounded every elementwise step to the storage type, the eager control's error was 1.5 x the padded control's on EVERY 16-bit
# case (bf16 RMS 9.1e-3 to 1.02e-2 against 6.2e-3 to 6.8e-3; the embedding LayerNorm alone 4.6e-3 against 3.4e-3) and the spread
# 1.61 to 2.05 per case, above the cap whatever the case: the first run of these tests found that, and `_ln` was mended.
MEASURED_CONTROL_SPREAD = {"bf16": 1.470, "fp16": 1.446, "f32": 1.304}
ROW_FACTOR = {s: min(1.25 * v if v > 1.2 else 1.5, ROW_FACTOR_CAP) for s, v in MEASURED_CONTROL_SPREAD.items()}
assert all(FACTOR <= f <= ROW_FACTOR_CAP for f in ROW_FACTOR.values())

EDGES = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 1]
MAX_LENGTH = 512
TILE = 32                                             # kAttnQBlock = kAttnKeys of rpo_bidir_attn_fwd
VOCAB = 1024

# name -> (config function of rankpo_amd.encoder, its keywords); intermediate = 4 d
LAYOUTS = {
    "bge_hd32": ("bge_small_config", dict(hidden_size=128, num_attention_heads=4, max_position_embeddings=512)),
    "xlmr_hd64": ("xlm_roberta_config", dict(hidden_size=256, num_attention_heads=4, max_position_embeddings=514)),
    "bge_12x32": ("bge_small_config", dict(hidden_size=384, num_attention_heads=12, max_position_embeddings=512)),
    "xlmr_12x64": ("xlm_roberta_config", dict(hidden_size=768, num_attention_heads=12, max_position_embeddings=514)),
    "bge_hd32_L0": ("bge_small_config", dict(hidden_size=128, num_attention_heads=4, max_position_embeddings=512,
                                             num_hidden_layers=0)),
}


def config(layout):
    from rankpo_amd import encoder as PE
    fn, kw = LAYOUTS[layout]
    d = kw["hidden_size"]
    # initializer_range d^-1/2 instead of BERT's 0.02: projections then keep the scale of the LayerNorm output and the attention
    # scores have about unit variance, so the softmax is neither uniform nor saturated and attention carries a share of the CLS row
    # that a defect in it moves.  At 0.02 the attention branch of these small models is a few 1e-3 of a 512-token row, below a bf16
    # bound, and the query biases move no row by the bf16 floor (tests/test_bert_encode_parity_host.py asserts that they do here).
    kw = dict(dict(vocab_size=VOCAB, num_hidden_layers=2, intermediate_size=4 * d, initializer_range=d ** -0.5), **kw)
    return getattr(PE, fn)(**kw)


JITTERED = lambda name: name.endswith(".bias") or "LayerNorm" in name or name == "embeddings.token_type_embeddings.weight"


def build_model(layout, seed=0):
    """The float32 encoder of `layout` as initialised from `seed`, then every parameter `JITTERED` names moved off its initial
    0 / 1 / N(0, 1 / d) by 0.05 randn: a bias dropped or concatenated in the wrong order, a LayerNorm weight taken for its bias, a
    token-type row taken for another then change the rows."""
    from rankpo_amd import encoder as PE
    cfg = config(layout)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        enc = PE.build_encoder(cfg)
    g = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for name, p in enc.named_parameters():
            if JITTERED(name):
                p.add_(0.05 * torch.randn(p.shape, generator=g))
    return cfg, enc.eval()


@functools.lru_cache(maxsize=None)
def host_weights(layout="bge_hd32", storage="bf16", seed=0):
    """(config, the encoder's state dict in `storage` on the host): what a model built by `build_model(seed)` and cast holds."""
    cfg, enc = build_model(layout, seed)
    return cfg, {k: v.detach().to(STORAGE[storage]) for k, v in enc.state_dict().items()}


# ------------------------------------------------------------------------------------------------------------------------------
# texts, masks, token types
# ------------------------------------------------------------------------------------------------------------------------------
def make_texts(lens):
    """Row i: the first lens[i] characters of row i's own stream of letters (so the two one-token rows are different tokens).  No
    character becomes token id 1, XLM-R's pad id, which takes no position of its own: `CharTok` maps character c in column j to
    1 + (7 ord(c) + j) % 1000, and a letter that would give 1 is replaced by its successor."""
    out = []
    for i, n in enumerate(lens):
        s = [97 + int(c) for c in np.random.RandomState(9000 + i).randint(0, 26, size=MAX_LENGTH)[:n]]
        s = [97 + (c - 97 + 1) % 26 if (7 * c + j) % 1000 == 0 else c for j, c in enumerate(s)]
        out.append("".join(map(chr, s)))
    assert [len(t) for t in out] == list(lens) and len(set(out)) == len(out)
    return out


def tokenise(texts):
    tok = CharTok()(texts, max_length=MAX_LENGTH)
    assert tok["attention_mask"].sum(-1).tolist() == [len(t) for t in texts]
    real = tok["input_ids"][tok["attention_mask"].bool()]
    assert int(real.min()) >= 2 and int(real.max()) < VOCAB          # neither pad id (BERT 0, XLM-R 1) among the real tokens
    return tok


def holed(tok, pad_id_token=None):
    """(input_ids, attention_mask) with one hole per row of length >= 3, at a different column per row, the CLS column set.
    pad_id_token = (row, column, id): that REAL token (mask 1, not the row's hole) gets `id` -- XLM-R's pad id in mid-row, a token
    that takes position pad_id and is not counted by the tokens after it."""
    ids, m = tok["input_ids"].clone(), tok["attention_mask"].clone()
    lens = m.sum(-1).tolist()
    cols = {}
    for r, n in enumerate(lens):
        if n >= 3:
            cols[r] = 1 + (37 * r) % (n - 2)                          # 1 .. n - 2: neither the CLS column nor the last token
            m[r, cols[r]] = 0
    assert len(set(cols.values())) == len(cols) >= 2 and bool((m[:, 0] == 1).all())
    if pad_id_token is not None:
        r, c, v = pad_id_token
        assert 0 < c < lens[r] - 1 and cols.get(r) != c and int(m[r, c]) == 1
        ids[r, c] = v
    return ids, m, cols


def token_types(tok):
    """A 0/1 pattern [N, L] that differs per row (row r: runs of r + 1 tokens, starting on 0 or 1 by the parity of r); 0 on pads."""
    m = tok["attention_mask"]
    N, Lw = m.shape
    c, r = torch.arange(Lw)[None, :], torch.arange(N)[:, None]
    tts = ((c // (r + 1) + r) % 2) * m
    assert len({tuple(t[:n].tolist()) for t, n in zip(tts, m.sum(-1).tolist()) if n >= 8}) == sum(n >= 8 for n in m.sum(-1).tolist())
    return tts.to(torch.int64)


def check_edges(lens=EDGES):
    """What the arms rely on: a row at, below and above every multiple of 32 up to 128 and at 256, the longest row on the last
    row of either position table, a work-list order that is not the input order."""
    from rankpo_amd import encoder as PE, ops
    assert lens[0] == lens[-1] == 1
    assert all({k - 1, k, k + 1} <= set(lens) for k in list(range(TILE, 129, TILE)) + [256])
    assert max(lens) == MAX_LENGTH and {MAX_LENGTH - 1, MAX_LENGTH} <= set(lens)
    tok = tokenise(make_texts(lens))
    for layout in ("bge_hd32", "xlmr_hd64"):
        cfg = config(layout)
        roberta = "Roberta" in cfg.architectures[0]
        _, pos, _, got = PE.bert_pack(tok["input_ids"], tok["attention_mask"], roberta=roberta, pad_id=cfg.pad_token_id)
        assert got == list(lens)
        assert int(pos.max()) == cfg.max_position_embeddings - 1 == (513 if roberta else 511)      # the table's last row
        assert int(pos.min()) == (cfg.pad_token_id + 1 if roberta else 0)
    order = ops.bidir_attn_tile_list([1] * len(lens), lens)[:, 0].tolist()
    assert sorted(order) == list(range(len(lens))) and order != list(range(len(lens)))
    assert order[0] == lens.index(max(lens)) and set(order[-2:]) == {0, len(lens) - 1}
    return order


# ------------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ------------------------------------------------------------------------------------------------------------------------------
def _w64(sd, device="cpu"):
    return {k: v.detach().to(device, torch.float64) for k, v in sd.items()}


def reference_rows(sd, cd, tok, padded=False, device="cpu"):
    """Float64 unit rows [N, d] of `oracle.encoder_ref.embed` on the weights `sd` holds (their values as they are), one sequence
    at a time.  padded=False: at its own length (a right-padded 0/1 mask); True: at the padded width with the row's own mask.
    tok: input_ids, attention_mask and optionally token_type_ids.  device: where the float64 arithmetic runs."""
    w = _w64(sd, device)
    m = tok["attention_mask"]
    rows = []
    with torch.no_grad():
        for i, n in enumerate(m.sum(-1).tolist()):
            if not padded:
                assert bool(m[i, :n].all())
            one = {k: v[i:i + 1, :(m.shape[1] if padded else n)].to(device) for k, v in tok.items()}
            rows.append(E.embed(w, cd, one, dtype=torch.float64).cpu())
    return torch.cat(rows, 0)


def padded_reference_rows(sd, cd, tok, device="cpu"):
    """The same rows from ONE padded call (the host test compares the two)."""
    with torch.no_grad():
        return E.embed(_w64(sd, device), cd, {k: v.to(device) for k, v in tok.items()}, dtype=torch.float64).cpu()


# ------------------------------------------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------------------------------------------
TABLE_HEAD = ("| arm | worst row (length) | err fast | err eager | err padded | bound | fast / larger control | rms fast | rms eager | "
              "rms padded |")


def rule(ref, fast, eager, padded, lens, storage, arm="", row_factor=None, out=print):
    """llama_encode_parity_util.rule with the padded path as the second control, the per-row factor and the floors of `storage`.
    Failure kinds: "row", "rms", "guard", "control", "missing", "shape", "nonfinite", "extra"."""
    floor, guard_floor = floors(storage)
    return L.rule(ref, fast, eager, padded, lens, arm=arm, row_factor=ROW_FACTOR[storage] if row_factor is None else row_factor,
                  out=out, floor=floor, guard_floor=guard_floor)


# ------------------------------------------------------------------------------------------------------------------------------
# one (layout, storage, mask kind) case on the device: model, float64 reference and the controls, computed once, shared by the arms
# ------------------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
REF_DEVICE = "cpu"                    # where the float64 reference runs: 2755 tokens through two blocks at d 768 take the host under 1 s


@functools.lru_cache(maxsize=None)
def model_s(layout="bge_hd32", storage="bf16", packed_f32=False, seed=0):
    """`ModelForInference` on `layout`, its weights the ones `host_weights` holds (asserted), in eval mode."""
    import rankpo_amd
    cfg, sd = host_weights(layout, storage, seed)
    _, enc = build_model(layout, seed)
    inf = rankpo_amd.ModelForInference(encoder=enc, tokenizer=CharTok(), use_bf16=storage == "bf16", use_fp16=storage == "fp16",
                                       device=0, packed_f32=packed_f32)
    inf.model.eval()
    held = inf.model.state_dict()
    assert set(held) == set(sd) and all(held[k].dtype == STORAGE[storage] and torch.equal(held[k].cpu(), sd[k]) for k in sd)
    assert inf.model.native_f32 == bool(packed_f32)
    return inf


def eager_control(enc, cd, dev_tok):
    """Control (i): the oracle's eager code in the model's storage type on the device, on the model's weights."""
    wd = {k: v.detach() for k, v in enc.state_dict().items()}
    with torch.no_grad():
        return E.embed(wd, cd, dev_tok, dtype=next(iter(wd.values())).dtype).float().cpu()


def padded_control(inf, texts=None, dev_tok=None):
    """Control (ii): the product's padded PyTorch path on a model that does not opt into the packed f32 forward.  texts: through
    `encode()` with BERT_NATIVE off; dev_tok (a mask or token types `encode()` cannot be given): the padded forward itself.

    Under SDPA's MATH backend, because a yardstick has to be reproducible and PyTorch's fused attention kernels are not on the
    MI355X: the padded fp16 forward of xlmr_12x64 on EDGES, repeated 80 times in one process, gave 9 to 12 distinct results with
    single rows (63 to 65, 255 to 257 and 511 tokens) up to 15 x their median error, under hipBLASLt and hipBLAS alike; with the
    MATH backend 80 repeats are bit-equal and no row is off (and the RMS is the same: 7.72e-4 against 7.80e-4).  The packed path
    gave one result in 60 repeats.  profiles/bert_encode_parity.md has the figures."""
    from torch.nn.attention import SDPBackend, sdpa_kernel
    from rankpo_amd import encoder as PE, ops
    assert not inf.model.native_f32
    with sdpa_kernel([SDPBackend.MATH]):
        if texts is not None:
            on = PE.BERT_NATIVE
            PE.BERT_NATIVE = False
            try:
                return inf.encode(texts, batch_size=64, max_length=MAX_LENGTH, convert_to_numpy=False).float().cpu()
            finally:
                PE.BERT_NATIVE = on
        with torch.no_grad():
            h = inf.model(**dev_tok).last_hidden_state
            return ops.pool_normalize(h, dev_tok["attention_mask"], "cls", True).float().cpu()


KINDS = ("plain", "holed", "types")


@functools.lru_cache(maxsize=None)
def case_s(layout="bge_hd32", storage="bf16", kind="plain", seed=0):
    """kind: "plain" = EDGES as the tokenizer gives them; "holed" = one hole per row of length >= 3 (XLM-R: also one real token
    with the pad id in mid-row); "types" = a 0/1 token-type pattern that differs per row."""
    check_edges()
    inf = model_s(layout, storage, False, seed)
    enc, cfg = inf.model, inf.model.config
    texts = make_texts(EDGES)
    tok = dict(tokenise(texts))
    pad_tok = None
    if kind == "holed":
        roberta = "Roberta" in cfg.architectures[0]
        pad_tok = (9, 40, cfg.pad_token_id) if roberta else None          # row 9: 96 tokens
        tok["input_ids"], tok["attention_mask"], holes = holed(tok, pad_tok)
    elif kind == "types":
        assert cfg.type_vocab_size == 2
        tok["token_type_ids"] = token_types(tok)
    lens = tok["attention_mask"].sum(-1).tolist()
    dev_tok = {k: v.to(DEV) for k, v in tok.items()}
    ref = reference_rows(host_weights(layout, storage, seed)[1], cfg.to_dict(), tok, padded=kind == "holed",
                         device=REF_DEVICE)
    assert ref.shape == (len(EDGES), cfg.hidden_size) and float((ref.norm(dim=-1) - 1).abs().max()) < 1e-12
    eager = eager_control(enc, cfg.to_dict(), dev_tok)
    padded = padded_control(inf, texts) if kind == "plain" else padded_control(inf, dev_tok=dev_tok)
    return SimpleNamespace(layout=layout, storage=storage, kind=kind, inf=inf, enc=enc, cfg=cfg, lens=lens, texts=texts, tok=tok,
                           dev_tok=dev_tok, ref=ref, eager=eager, padded=padded, tot=sum(lens), rows=len(lens), pad_tok=pad_tok,
                           inf_on=model_s(layout, storage, True, seed) if storage == "f32" else None)
