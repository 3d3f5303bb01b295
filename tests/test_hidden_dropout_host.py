"""CPU side of the fused hidden dropout and of gradient checkpointing on the packed BERT / XLM-R step: the statistics of the keep
function's numpy restatement (tests/hidden_dropout_util.py; tests/test_gpu_hidden_dropout.py compares the kernels' dump with it bit
for bit), the seed that keeps hidden and attention dropout apart, and the opt-in's decline logic."""
import math

import numpy as np
import torch

import hidden_dropout_util as HU
from rankpo_amd import encoder as PE
from rankpo_amd import ops

ROWS, D, P = 512, 1024, 0.1
N = ROWS * D


def _share():
    return 1.0 - HU.threshold(P) / 65536.0


def test_threshold_and_scale():
    assert HU.threshold(0.1) == 6554 and HU.threshold(0.5) == 32768 and HU.threshold(0.0) == 0
    for p in (0.1, 0.5, 0.25, 0.0, 1e-7):
        assert ops.hidden_dropout_scale(p) == HU.scale(p), p        # the library's f32 factor
    assert ops.hidden_dropout_scale(0.5) == 2.0 and ops.hidden_dropout_scale(0.0) == 1.0


def test_kept_share_within_5_sigma():
    q = _share()
    tol = 5 * math.sqrt(q * (1 - q) / N)                             # 5 sqrt(0.09 / 524288) = 2.1e-3
    assert abs(tol - 2.1e-3) < 1e-4
    for seed in HU.SEEDS:
        for site in (0, 1, 2, 47):
            m = HU.hidden_keep(ops.bert_hidden_seed(seed), site, 0, ROWS, D, P)
            assert m.shape == (ROWS, D) and m.dtype == np.uint8
            assert abs(m.mean() - q) <= tol, (seed, site, m.mean(), q, tol)
            # per row and per column (1024 resp. 512 draws each): no row or column is off by 6 sigma
            assert np.abs(m.mean(1) - q).max() <= 6 * math.sqrt(q * (1 - q) / D)
            assert np.abs(m.mean(0) - q).max() <= 6 * math.sqrt(q * (1 - q) / ROWS)


def test_sites_and_seeds_are_independent():
    """Two sites, two seeds, and two row windows agree on the product of the shares: P(both kept) = q^2, not more."""
    q = _share()
    tol = 5 * math.sqrt(q * q * (1 - q * q) / N)
    s0, s1 = (ops.bert_hidden_seed(s) for s in HU.SEEDS[:2])
    base = HU.hidden_keep(s0, 1, 0, ROWS, D, P)
    for name, other in (("site", HU.hidden_keep(s0, 2, 0, ROWS, D, P)), ("seed", HU.hidden_keep(s1, 1, 0, ROWS, D, P)),
                        ("seed + 1", HU.hidden_keep(s0 + 1, 1, 0, ROWS, D, P)),
                        ("rows", HU.hidden_keep(s0, 1, ROWS, ROWS, D, P))):
        both = (base & other).mean()
        assert abs(both - q * q) <= tol, (name, both, q * q, tol)
    # a window of a mask = the same entries of the whole mask
    assert np.array_equal(HU.hidden_keep(s0, 1, 5, 3, D, P), base[5:8])


def test_hidden_seed_never_equals_a_layer_seed():
    for seed in (0, 1, 12345, 2 ** 31, 2 ** 63 - 2, 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 2 ** 64 - 1) + HU.SEEDS:
        h = ops.bert_hidden_seed(seed)
        assert 0 <= h < 2 ** 64
        assert h not in {ops.bert_layer_seed(seed, i) for i in range(4096)}
    assert [ops.bert_hidden_site(), ops.bert_hidden_site(0), ops.bert_hidden_site(0, True), ops.bert_hidden_site(3),
            ops.bert_hidden_site(3, True)] == [0, 1, 2, 7, 8]


def _bert():
    return PE.BertEncoder(PE.bert_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                         num_attention_heads=2, max_position_embeddings=32, hidden_dropout_prob=0.1,
                                         attention_probs_dropout_prob=0.1))


def test_packed_checkpointing_opt_in_does_not_decline(monkeypatch):
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)
    assert PE.BERT_FUSED_HIDDEN_DROPOUT is False
    enc = _bert().half().train()
    assert enc.gradient_checkpointing is False and enc.checkpoint_packed is False
    enc.gradient_checkpointing_enable()
    assert enc.gradient_checkpointing and not enc.checkpoint_packed
    assert enc.native_train_decline_reason() == "gradient checkpointing"       # the bare call: as ever
    enc.gradient_checkpointing_enable(packed=True)
    assert enc.gradient_checkpointing and enc.checkpoint_packed
    assert enc.native_train_decline_reason() is None
    enc.gradient_checkpointing_enable(use_reentrant=False)                      # HF-style keywords: still the bare call
    assert enc.native_train_decline_reason() == "gradient checkpointing"
    enc.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"use_reentrant": False})
    assert enc.native_train_decline_reason() == "gradient checkpointing"
    enc.gradient_checkpointing_enable(gradient_checkpointing_kwargs={"packed": True})     # how the HF Trainer passes its kwargs
    assert enc.checkpoint_packed and enc.native_train_decline_reason() is None
    # the other conditions still decline under the opt-in
    enc.gradient_checkpointing_enable(packed=True)
    with torch.no_grad():
        assert enc.native_train_decline_reason() == "grad disabled"
    assert _bert().train().native_train_decline_reason() == "storage dtype"


def test_model_for_training_forwards_the_keyword(monkeypatch):
    import rankpo_amd
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)
    model = rankpo_amd.ModelForTraining(encoder=_bert().half(), temperature=0.02).train()
    model.gradient_checkpointing_enable()
    assert model.model.native_train_decline_reason() == "gradient checkpointing"
    model.gradient_checkpointing_enable(packed=True)
    assert model.model.checkpoint_packed and model.model.native_train_decline_reason() is None


def test_new_entry_points_are_bound():
    from rankpo_amd import _lib
    for name in ("rpo_add_layernorm_drop_fwd", "rpo_bert_embed_ln_drop_fwd", "rpo_layernorm_drop_bwd", "rpo_hidden_dropout_mask",
                 "rpo_hidden_dropout_scale"):
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.rpo_hidden_dropout_scale(1.0) == 0.0 and lib.rpo_hidden_dropout_scale(-0.5) == 0.0   # outside [0, 1)
    # rows == 0 is a no-op success and bad arguments are status codes: every call below returns before a launch, so the
    # non-null, 16-byte aligned dummy pointer is never dereferenced
    p = 16
    assert lib.rpo_add_layernorm_drop_fwd(p, 64, p, 64, p, p, 1e-5, p, 64, p, 64, 0, 64, 2, 0.1, 5, 1, None) == 0
    assert lib.rpo_layernorm_drop_bwd(p, 64, p, p, 64, 1e-5, p, 64, p, 64, p, p, 0, 64, 2, 0.1, 5, -1, 1, None) == 0
    assert lib.rpo_hidden_dropout_mask(0, 0, 64, 0.1, 5, 0, p, None) == 0
    assert lib.rpo_add_layernorm_drop_fwd(p, 64, p, 64, p, p, 1e-5, p, 64, p, 64, 0, 64, 2, 1.0, 5, 1, None) == -1    # p_drop
    assert lib.rpo_add_layernorm_drop_fwd(p, 64, p, 64, p, p, 1e-5, p, 64, p, 64, 0, 64, 0, 0.1, 5, 1, None) == -2    # f32
    assert lib.rpo_add_layernorm_drop_fwd(p, 12, p, 12, p, p, 1e-5, p, 12, p, 12, 0, 12, 2, 0.1, 5, 1, None) == -2    # d % 8
    assert lib.rpo_add_layernorm_drop_fwd(p, 64, p, 64, p, p, 1e-5, p, 64, p, 64, 0, 64, 2, 0.1, 5, -1, None) == -1   # site
    assert lib.rpo_layernorm_drop_bwd(p, 8192, p, p, 8192, 1e-5, p, 8192, p, 8192, p, p, 0, 8192, 2, 0.1, 5, -1, 1, None) == -2   # d > 4096


# ------------------------------------------------------------------------------------------------
# status codes of the row entries and of the two attention forwards: (entry, arguments, status), recorded from the library as it
# was before the row kernels' dropout twins were folded into templates.  0 = OK, -1 = INVALID_ARG, -2 = UNSUPPORTED.  Every call
# returns before a launch (rows / ntiles == 0, or an argument that is refused), so the dummy pointer PTR is never dereferenced.
# ------------------------------------------------------------------------------------------------
PTR = 16
ENTRY_STATUS = [
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_add_layernorm_fwd", (0, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 1, None), -1),  # null a
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, 0, 64, 0, 64, 1, None), -1),  # null y
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, 0, PTR, 1e-05, PTR, 64, 0, 64, 1, None), -1),  # null gamma
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, 8, PTR, 1e-05, PTR, 64, 0, 64, 1, None), -2),  # misaligned gamma
    ("rpo_add_layernorm_fwd", (PTR, 12, PTR, 12, PTR, PTR, 1e-05, PTR, 12, 0, 12, 1, None), -2),  # d % 8
    ("rpo_add_layernorm_fwd", (PTR, 4104, PTR, 4104, PTR, PTR, 1e-05, PTR, 4104, 0, 4104, 1, None), -2),  # d too wide
    ("rpo_add_layernorm_fwd", (PTR, 4096, PTR, 4096, PTR, PTR, 1e-05, PTR, 4096, 0, 4096, 1, None), 0),  # d 4096
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 56, 0, 64, 1, None), -1),  # stride < d
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 68, 0, 64, 1, None), -2),  # misaligned stride
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 68, PTR, PTR, 1e-05, PTR, 64, 0, 64, 1, None), -2),  # misaligned stride of b
    ("rpo_add_layernorm_fwd", (PTR, 64, 0, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 1, None), 0),  # null b
    ("rpo_add_layernorm_fwd", (PTR, 64, 0, 3, PTR, PTR, 1e-05, PTR, 64, 0, 64, 1, None), 0),  # null b, its stride unchecked
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 0, None), -2),  # dtype f32
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 2, None), 0),  # dtype f16
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 7, None), -1),  # bad dtype
    ("rpo_add_layernorm_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, -1, 64, 1, None), -1),  # rows < 0
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_add_layernorm_train_fwd", (0, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), -1),  # null a
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, 0, 64, PTR, 64, 0, 64, 1, None), -1),  # null y
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, 0, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), -1),  # null gamma
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, 8, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), -2),  # misaligned gamma
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 0, 64, 1, None), -1),  # null s
    ("rpo_add_layernorm_train_fwd", (PTR, 12, PTR, 12, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 0, 12, 1, None), -2),  # d % 8
    ("rpo_add_layernorm_train_fwd", (PTR, 4104, PTR, 4104, PTR, PTR, 1e-05, PTR, 4104, PTR, 4104, 0, 4104, 1, None), -2),  # d too wide
    ("rpo_add_layernorm_train_fwd", (PTR, 4096, PTR, 4096, PTR, PTR, 1e-05, PTR, 4096, PTR, 4096, 0, 4096, 1, None), 0),  # d 4096
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 56, PTR, 64, 0, 64, 1, None), -1),  # stride < d
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 68, PTR, 64, 0, 64, 1, None), -2),  # misaligned stride
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 68, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), -2),  # misaligned stride of b
    ("rpo_add_layernorm_train_fwd", (PTR, 64, 0, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), 0),  # null b
    ("rpo_add_layernorm_train_fwd", (PTR, 64, 0, 3, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, None), 0),  # null b, its stride unchecked
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 0, None), -2),  # dtype f32
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 2, None), 0),  # dtype f16
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 7, None), -1),  # bad dtype
    ("rpo_add_layernorm_train_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, -1, 64, 1, None), -1),  # rows < 0
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), 0),  # ok, nothing to do
    ("rpo_add_layernorm_drop_fwd", (0, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null a
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, 0, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null y
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, 0, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null gamma
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, 8, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -2),  # misaligned gamma
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null s
    ("rpo_add_layernorm_drop_fwd", (PTR, 12, PTR, 12, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 0, 12, 1, 0.1, 5, 1, None), -2),  # d % 8
    ("rpo_add_layernorm_drop_fwd", (PTR, 4104, PTR, 4104, PTR, PTR, 1e-05, PTR, 4104, PTR, 4104, 0, 4104, 1, 0.1, 5, 1, None), -2),  # d too wide
    ("rpo_add_layernorm_drop_fwd", (PTR, 4096, PTR, 4096, PTR, PTR, 1e-05, PTR, 4096, PTR, 4096, 0, 4096, 1, 0.1, 5, 1, None), 0),  # d 4096
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 56, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # stride < d
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 68, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -2),  # misaligned stride
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 68, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -2),  # misaligned stride of b
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, 0, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null b
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, 0, 3, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1, None), -1),  # null b, its stride unchecked
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 0, 0.1, 5, 1, None), -2),  # dtype f32
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 2, 0.1, 5, 1, None), 0),  # dtype f16
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 7, 0.1, 5, 1, None), -1),  # bad dtype
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, -1, 64, 1, 0.1, 5, 1, None), -1),  # rows < 0
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 1.0, 5, 1, None), -1),  # p_drop 1
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.0, 5, 1, None), 0),  # p_drop 0
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, -1, None), -1),  # site -1
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1048577, None), -1),  # site too large
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 0, 64, 1, 0.1, 5, 1048576, None), 0),  # site at the bound
    ("rpo_add_layernorm_drop_fwd", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 2147483648, 64, 1, 0.1, 5, 1, None), -1),  # rows 2^31
    ("rpo_add_layernorm_drop_fwd", (PTR, 12, PTR, 12, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 2147483648, 12, 1, 0.1, 5, 1, None), -1),  # rows 2^31, d % 8
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, None), 0),  # ok, nothing to do
    ("rpo_add_layernorm_fwd_f32", (0, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, None), -1),  # null a
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, 0, 64, 0, 64, None), -1),  # null y
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, 0, PTR, 1e-05, PTR, 64, 0, 64, None), -1),  # null gamma
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, 8, PTR, 1e-05, PTR, 64, 0, 64, None), -2),  # misaligned gamma
    ("rpo_add_layernorm_fwd_f32", (PTR, 12, PTR, 12, PTR, PTR, 1e-05, PTR, 12, 0, 12, None), -2),  # d % 8
    ("rpo_add_layernorm_fwd_f32", (PTR, 4104, PTR, 4104, PTR, PTR, 1e-05, PTR, 4104, 0, 4104, None), -2),  # d too wide
    ("rpo_add_layernorm_fwd_f32", (PTR, 4096, PTR, 4096, PTR, PTR, 1e-05, PTR, 4096, 0, 4096, None), 0),  # d 4096
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 56, 0, 64, None), -1),  # stride < d
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 66, 0, 64, None), -2),  # misaligned stride
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 68, 0, 64, None), 0),  # stride % 4 only
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 66, PTR, PTR, 1e-05, PTR, 64, 0, 64, None), -2),  # misaligned stride of b
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, 0, 64, PTR, PTR, 1e-05, PTR, 64, 0, 64, None), 0),  # null b
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, 0, 3, PTR, PTR, 1e-05, PTR, 64, 0, 64, None), 0),  # null b, its stride unchecked
    ("rpo_add_layernorm_fwd_f32", (PTR, 64, PTR, 64, PTR, PTR, 1e-05, PTR, 64, -1, 64, None), -1),  # rows < 0
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_bert_embed_ln_fwd", (0, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), -1),  # null ids
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, 0, 64, 64, 1, None), -1),  # null y
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 0, PTR, 1e-05, PTR, 64, 64, 1, None), -1),  # null gamma
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 8, PTR, 1e-05, PTR, 64, 64, 1, None), -2),  # misaligned gamma
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 12, 12, 1, None), -2),  # d % 8
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4104, 4104, 1, None), -2),  # d too wide
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4096, 4096, 1, None), 0),  # d 4096
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 56, 64, 1, None), -1),  # stride < d
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 68, 64, 1, None), -2),  # misaligned stride
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 0, None), -2),  # dtype f32
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 2, None), 0),  # dtype f16
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 7, None), -1),  # bad dtype
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, -1, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), -1),  # rows < 0
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 0, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), -1),  # vocab 0
    ("rpo_bert_embed_ln_fwd", (PTR, 0, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), 0),  # null token types
    ("rpo_bert_embed_ln_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, 24, 8, PTR, PTR, 1e-05, PTR, 64, 64, 1, None), -2),  # misaligned table
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_bert_embed_ln_train_fwd", (0, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -1),  # null ids
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, 0, 64, PTR, 64, 64, 1, None), -1),  # null y
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 0, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -1),  # null gamma
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 8, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -2),  # misaligned gamma
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 0, 64, 64, 1, None), -1),  # null s
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 12, 1, None), -2),  # d % 8
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4104, PTR, 4104, 4104, 1, None), -2),  # d too wide
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4096, PTR, 4096, 4096, 1, None), 0),  # d 4096
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 56, PTR, 64, 64, 1, None), -1),  # stride < d
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 68, PTR, 64, 64, 1, None), -2),  # misaligned stride
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 0, None), -2),  # dtype f32
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 2, None), 0),  # dtype f16
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 7, None), -1),  # bad dtype
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, -1, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -1),  # rows < 0
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 0, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -1),  # vocab 0
    ("rpo_bert_embed_ln_train_fwd", (PTR, 0, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), 0),  # null token types
    ("rpo_bert_embed_ln_train_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, 24, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, None), -2),  # misaligned table
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), 0),  # ok, nothing to do
    ("rpo_bert_embed_ln_drop_fwd", (0, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # null ids
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, 0, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # null y
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 0, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # null gamma
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 8, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -2),  # misaligned gamma
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 0, 64, 64, 1, 0.1, 5, 1, None), -1),  # null s
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 12, 1, 0.1, 5, 1, None), -2),  # d % 8
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4104, PTR, 4104, 4104, 1, 0.1, 5, 1, None), -2),  # d too wide
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4096, PTR, 4096, 4096, 1, 0.1, 5, 1, None), 0),  # d 4096
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 56, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # stride < d
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 68, PTR, 64, 64, 1, 0.1, 5, 1, None), -2),  # misaligned stride
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 0, 0.1, 5, 1, None), -2),  # dtype f32
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 2, 0.1, 5, 1, None), 0),  # dtype f16
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 7, 0.1, 5, 1, None), -1),  # bad dtype
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, -1, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # rows < 0
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 0, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # vocab 0
    ("rpo_bert_embed_ln_drop_fwd", (PTR, 0, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), 0),  # null token types
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, 24, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -2),  # misaligned table
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 1.0, 5, 1, None), -1),  # p_drop 1
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.0, 5, 1, None), 0),  # p_drop 0
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, -1, None), -1),  # site -1
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1048577, None), -1),  # site too large
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1048576, None), 0),  # site at the bound
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 2147483648, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, PTR, 64, 64, 1, 0.1, 5, 1, None), -1),  # rows 2^31
    ("rpo_bert_embed_ln_drop_fwd", (PTR, PTR, PTR, 2147483648, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 12, PTR, 12, 12, 1, 0.1, 5, 1, None), -1),  # rows 2^31, d % 8
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), 0),  # ok, nothing to do
    ("rpo_bert_embed_ln_fwd_f32", (0, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), -1),  # null ids
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, 0, 64, 64, None), -1),  # null y
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 0, PTR, 1e-05, PTR, 64, 64, None), -1),  # null gamma
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, 8, PTR, 1e-05, PTR, 64, 64, None), -2),  # misaligned gamma
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 12, 12, None), -2),  # d % 8
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4104, 4104, None), -2),  # d too wide
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 4096, 4096, None), 0),  # d 4096
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 56, 64, None), -1),  # stride < d
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 66, 64, None), -2),  # misaligned stride
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 68, 64, None), 0),  # stride % 4 only
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, -1, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), -1),  # rows < 0
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 0, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), -1),  # vocab 0
    ("rpo_bert_embed_ln_fwd_f32", (PTR, 0, PTR, 0, PTR, 10, PTR, 2, PTR, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), 0),  # null token types
    ("rpo_bert_embed_ln_fwd_f32", (PTR, PTR, PTR, 0, PTR, 10, PTR, 2, 24, 8, PTR, PTR, 1e-05, PTR, 64, 64, None), -2),  # misaligned table
    ("rpo_layernorm_bwd", (0, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 4, 64, 1, None), -1),  # null s
    ("rpo_layernorm_bwd", (PTR, 64, 0, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 4, 64, 1, None), -1),  # null gamma
    ("rpo_layernorm_bwd", (PTR, 64, 8, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 4, 64, 1, None), -2),  # misaligned gamma
    ("rpo_layernorm_bwd", (PTR, 12, PTR, PTR, 12, 1e-05, PTR, 12, PTR, PTR, 4, 12, 1, None), -2),  # d % 8
    ("rpo_layernorm_bwd", (PTR, 4104, PTR, PTR, 4104, 1e-05, PTR, 4104, PTR, PTR, 4, 4104, 1, None), -2),  # d too wide
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 56, PTR, PTR, 4, 64, 1, None), -1),  # stride < d
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 68, PTR, PTR, 4, 64, 1, None), -2),  # misaligned stride
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 4, 64, 0, None), -2),  # dtype f32
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 4, 64, 7, None), -1),  # bad dtype
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, PTR, -1, 64, 1, None), -1),  # rows < 0
    ("rpo_layernorm_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, PTR, 0, 64, 1, None), -1),  # rows == 0
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), 0),  # ok, nothing to do
    ("rpo_layernorm_drop_bwd", (0, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), -1),  # null s
    ("rpo_layernorm_drop_bwd", (PTR, 64, 0, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), -1),  # null gamma
    ("rpo_layernorm_drop_bwd", (PTR, 64, 8, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), -2),  # misaligned gamma
    ("rpo_layernorm_drop_bwd", (PTR, 12, PTR, PTR, 12, 1e-05, PTR, 12, PTR, 12, PTR, PTR, 0, 12, 1, 0.1, 5, -1, 1, None), -2),  # d % 8
    ("rpo_layernorm_drop_bwd", (PTR, 4104, PTR, PTR, 4104, 1e-05, PTR, 4104, PTR, 4104, PTR, PTR, 0, 4104, 1, 0.1, 5, -1, 1, None), -2),  # d too wide
    ("rpo_layernorm_drop_bwd", (PTR, 4096, PTR, PTR, 4096, 1e-05, PTR, 4096, PTR, 4096, PTR, PTR, 0, 4096, 1, 0.1, 5, -1, 1, None), 0),  # d 4096
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 56, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), -1),  # stride < d
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 68, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), -2),  # misaligned stride
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, 0, 3, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1, None), 0),  # null db
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, 0, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, -1, None), 0),  # null db, no site_out
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, -1, None), -1),  # db without site_out
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, 1048577, 1, None), -1),  # site_in too large
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, 0, 1, None), 0),  # site_in set
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 0, 0.1, 5, -1, 1, None), -2),  # dtype f32
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 2, 0.1, 5, -1, 1, None), 0),  # dtype f16
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 7, 0.1, 5, -1, 1, None), -1),  # bad dtype
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, -1, 64, 1, 0.1, 5, -1, 1, None), -1),  # rows < 0
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 1.0, 5, -1, 1, None), -1),  # p_drop 1
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.0, 5, -1, 1, None), 0),  # p_drop 0
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, -1, None), -1),  # site -1
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1048577, None), -1),  # site too large
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 0, 64, 1, 0.1, 5, -1, 1048576, None), 0),  # site at the bound
    ("rpo_layernorm_drop_bwd", (PTR, 64, PTR, PTR, 64, 1e-05, PTR, 64, PTR, 64, PTR, PTR, 2147483648, 64, 1, 0.1, 5, -1, 1, None), -1),  # rows 2^31
    ("rpo_layernorm_drop_bwd", (PTR, 12, PTR, PTR, 12, 1e-05, PTR, 12, PTR, 12, PTR, PTR, 2147483648, 12, 1, 0.1, 5, -1, 1, None), -1),  # rows 2^31, d % 8
    ("rpo_gelu_fwd", (PTR, 0, 64, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_gelu_fwd", (0, 0, 64, 64, 1, None), -1),  # null a
    ("rpo_gelu_fwd", (PTR, 0, 12, 12, 1, None), -2),  # d % 8
    ("rpo_gelu_fwd", (PTR, 0, 4104, 4104, 1, None), 0),  # d too wide
    ("rpo_gelu_fwd", (PTR, 0, 4096, 4096, 1, None), 0),  # d 4096
    ("rpo_gelu_fwd", (PTR, 0, 64, 56, 1, None), -1),  # stride < d
    ("rpo_gelu_fwd", (PTR, 0, 64, 68, 1, None), -2),  # misaligned stride
    ("rpo_gelu_fwd", (PTR, 0, 64, 64, 0, None), -2),  # dtype f32
    ("rpo_gelu_fwd", (PTR, 0, 64, 64, 2, None), 0),  # dtype f16
    ("rpo_gelu_fwd", (PTR, 0, 64, 64, 7, None), -1),  # bad dtype
    ("rpo_gelu_fwd", (PTR, -1, 64, 64, 1, None), -1),  # rows < 0
    ("rpo_gelu_fwd_f32", (PTR, 0, 64, 64, None), 0),  # ok, nothing to do
    ("rpo_gelu_fwd_f32", (0, 0, 64, 64, None), -1),  # null a
    ("rpo_gelu_fwd_f32", (PTR, 0, 12, 12, None), -2),  # d % 8
    ("rpo_gelu_fwd_f32", (PTR, 0, 4104, 4104, None), 0),  # d too wide
    ("rpo_gelu_fwd_f32", (PTR, 0, 4096, 4096, None), 0),  # d 4096
    ("rpo_gelu_fwd_f32", (PTR, 0, 64, 56, None), -1),  # stride < d
    ("rpo_gelu_fwd_f32", (PTR, 0, 64, 66, None), -2),  # misaligned stride
    ("rpo_gelu_fwd_f32", (PTR, 0, 64, 68, None), 0),  # stride % 4 only
    ("rpo_gelu_fwd_f32", (PTR, -1, 64, 64, None), -1),  # rows < 0
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 64, 0, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_gelu_out_fwd", (0, 64, PTR, 64, 0, 64, 1, None), -1),  # null a
    ("rpo_gelu_out_fwd", (PTR, 64, 0, 64, 0, 64, 1, None), -1),  # null y
    ("rpo_gelu_out_fwd", (PTR, 12, PTR, 12, 0, 12, 1, None), -2),  # d % 8
    ("rpo_gelu_out_fwd", (PTR, 4104, PTR, 4104, 0, 4104, 1, None), 0),  # d too wide
    ("rpo_gelu_out_fwd", (PTR, 4096, PTR, 4096, 0, 4096, 1, None), 0),  # d 4096
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 56, 0, 64, 1, None), -1),  # stride < d
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 68, 0, 64, 1, None), -2),  # misaligned stride
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 64, 0, 64, 0, None), -2),  # dtype f32
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 64, 0, 64, 2, None), 0),  # dtype f16
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 64, 0, 64, 7, None), -1),  # bad dtype
    ("rpo_gelu_out_fwd", (PTR, 64, PTR, 64, -1, 64, 1, None), -1),  # rows < 0
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 64, 0, 64, 1, None), 0),  # ok, nothing to do
    ("rpo_gelu_bwd", (0, 64, PTR, 64, PTR, 64, 0, 64, 1, None), -1),  # null a
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, 0, 64, 0, 64, 1, None), -1),  # null y
    ("rpo_gelu_bwd", (PTR, 12, PTR, 12, PTR, 12, 0, 12, 1, None), -2),  # d % 8
    ("rpo_gelu_bwd", (PTR, 4104, PTR, 4104, PTR, 4104, 0, 4104, 1, None), 0),  # d too wide
    ("rpo_gelu_bwd", (PTR, 4096, PTR, 4096, PTR, 4096, 0, 4096, 1, None), 0),  # d 4096
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 56, 0, 64, 1, None), -1),  # stride < d
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 68, 0, 64, 1, None), -2),  # misaligned stride
    ("rpo_gelu_bwd", (PTR, 64, PTR, 68, PTR, 64, 0, 64, 1, None), -2),  # misaligned stride of b
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 64, 0, 64, 0, None), -2),  # dtype f32
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 64, 0, 64, 2, None), 0),  # dtype f16
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 64, 0, 64, 7, None), -1),  # bad dtype
    ("rpo_gelu_bwd", (PTR, 64, PTR, 64, PTR, 64, -1, 64, 1, None), -1),  # rows < 0
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 64, PTR, None), 0),  # ok, nothing to do
    ("rpo_bidir_attn_fwd", (0, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 64, PTR, None), -1),  # null q
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0, 64, PTR, None), -1),  # null y
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 48, 1, 0.125, PTR, 64, PTR, None), -2),  # head_dim 48
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 12, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 64, PTR, None), -2),  # misaligned stride
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 6, PTR, None), -2),  # misaligned out stride
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 0, 0.125, PTR, 64, PTR, None), -2),  # dtype f32
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 7, 0.125, PTR, 64, PTR, None), -1),  # bad dtype
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 64, 0, None), 0),  # null lse
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 1, 32, 1, 0.125, PTR, 64, PTR, None), -2),  # kv heads
    ("rpo_bidir_attn_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, -1, 2, 32, 8, 2, 2, 32, 1, 0.125, PTR, 64, PTR, None), -1),  # negative ntiles
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), 0),  # ok, nothing to do
    ("rpo_bidir_attn_train_fwd", (0, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), -1),  # null q
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, 0, 64, PTR, None), -1),  # null y
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 48, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), -2),  # head_dim 48
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 12, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), -2),  # misaligned stride
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 6, PTR, None), -2),  # misaligned out stride
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 0, 0.125, 0.1, 5, PTR, 64, PTR, None), -2),  # dtype f32
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 7, 0.125, 0.1, 5, PTR, 64, PTR, None), -1),  # bad dtype
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 64, 0, None), -1),  # null lse
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 1, 32, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), -2),  # kv heads
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, -1, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.1, 5, PTR, 64, PTR, None), -1),  # negative ntiles
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 1.0, 5, PTR, 64, PTR, None), -1),  # p_drop 1
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, -0.5, 5, PTR, 64, PTR, None), -1),  # p_drop < 0
    ("rpo_bidir_attn_train_fwd", (PTR, PTR, PTR, 64, 64, 64, PTR, PTR, PTR, 0, 2, 32, 8, 2, 2, 32, 1, 0.125, 0.0, 5, PTR, 64, PTR, None), 0),  # p_drop 0
]


def test_row_and_attention_entries_keep_their_status_codes():
    from rankpo_amd import _lib
    lib = _lib.load()
    assert len({entry for entry, _, _ in ENTRY_STATUS}) == 16           # the 14 row entries and the two attention forwards
    for entry, args, want in ENTRY_STATUS:
        assert want in (0, -1, -2)
        assert getattr(lib, entry)(*args) == want, (entry, args, want)
