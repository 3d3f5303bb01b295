"""Host logic of the packed BERT / XLM-R training step (`BertEncoder.pooled_cls_train`): every condition under which it
declines, the unchanged verdicts of the forward-only path, the key-side work list of the attention backward and the per-layer
attention-dropout seed."""
import numpy as np
import pytest
import torch

from rankpo_amd import encoder as PE
from rankpo_amd import ops


def _bert(**kw):
    cfg = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
               max_position_embeddings=32, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg.update(kw)
    return PE.BertEncoder(PE.bert_config(**cfg))


def test_every_train_decline_condition(monkeypatch):
    ids = torch.randint(5, 50, (2, 7))
    m = torch.ones(2, 7, dtype=torch.int64)
    enc = _bert().train()
    assert enc.native_train_decline_reason() == "not on a HIP device"          # a CPU model
    assert enc.pooled_cls_train(ids, m) is None
    # with the device test passed, each remaining condition declines on its own
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)
    assert enc.native_train_decline_reason() == "storage dtype"                # f32
    for dt in (torch.float16, torch.bfloat16):
        assert _bert().to(dt).train().native_train_decline_reason() is None
    h = enc.to(torch.float16)
    with torch.no_grad():
        assert h.native_train_decline_reason() == "grad disabled"
    monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", False)
    assert h.native_train_decline_reason() == "BERT_NATIVE_TRAIN is off"
    assert h.pooled_cls_train(ids, m) is None
    monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", True)
    assert _bert(hidden_size=96, num_attention_heads=1).half().native_train_decline_reason() == "shape"    # head_dim 96
    assert _bert(hidden_size=128, num_attention_heads=1).half().native_train_decline_reason() == "shape"   # head_dim 128
    assert _bert(intermediate_size=132).half().native_train_decline_reason() == "shape"
    assert _bert(hidden_act="gelu_new").half().native_train_decline_reason() == "activation"
    ck = _bert().half().train()
    ck.gradient_checkpointing_enable()
    assert ck.native_train_decline_reason() == "gradient checkpointing"
    # dropout does NOT decline, in train or eval mode
    assert _bert(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1).half().train().native_train_decline_reason() is None
    assert _bert(hidden_dropout_prob=0.1).half().eval().native_train_decline_reason() is None
    # mask / id declines return None before anything touches a device
    assert h.pooled_cls_train(ids, None) is None
    bad = m.clone()
    bad[0, 0] = 0                                                               # CLS column masked
    assert h.pooled_cls_train(ids, bad) is None
    bad = m.clone()
    bad[1, 2] = 3                                                               # not 0/1
    assert h.pooled_cls_train(ids, bad) is None
    bad = m.clone()
    bad[1, 2] = 0                                                               # a hole: not right-padded
    assert h.pooled_cls_train(ids, bad) is None
    big = ids.clone()
    big[0, 1] = 64                                                              # outside the vocabulary
    assert h.pooled_cls_train(big, m) is None
    far = torch.randint(5, 50, (1, 40))                                         # position 32+ outside the table
    assert h.pooled_cls_train(far, torch.ones_like(far)) is None
    tt = torch.full_like(ids, 2)                                                # token type outside its table
    assert h.pooled_cls_train(ids, m, tt) is None


def test_forward_only_path_keeps_its_verdicts(monkeypatch):
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)
    enc = _bert().half().eval()
    assert enc.native_decline_reason() == "grad enabled"
    for flag in (True, False):                       # the training flag does not reach the forward-only path
        monkeypatch.setattr(PE, "BERT_NATIVE_TRAIN", flag)
        assert enc.native_decline_reason() == "grad enabled"
        with torch.inference_mode():
            assert enc.native_decline_reason() is None
            assert _bert(hidden_dropout_prob=0.1).half().train().native_decline_reason() == "training with dropout"
            assert _bert(attention_probs_dropout_prob=0.1).half().train().native_decline_reason() == "training with dropout"
            assert _bert().half().train().native_decline_reason() is None


@pytest.mark.parametrize("lens_q,lens_k", [([1, 31, 32, 33, 512],) * 2, ([512, 33, 32, 31, 1, 1],) * 2,
                                           ([1] * 5, [1, 31, 32, 33, 512])])
def test_key_work_list_covers_every_key_once(lens_q, lens_k):
    kb = ops.BIDIR_ATTN_Q_BLOCK
    t = ops.bidir_attn_key_tile_list(lens_q, lens_k)
    assert t.dtype == np.int32 and t.shape[1] == 2
    covered = {s: np.zeros(n, dtype=np.int64) for s, n in enumerate(lens_k)}
    for s, k0 in t.tolist():
        assert 0 <= k0 < lens_k[s] and k0 % kb == 0
        covered[s][k0:k0 + kb] += 1
    for s, c in covered.items():
        assert (c == 1).all(), (s, c)
    queries = [lens_q[s] for s in t[:, 0]]
    assert queries == sorted(queries, reverse=True)          # the longest-running entries first


def test_layer_seed_is_injective_over_layers():
    for seed in (0, 1, 12345, 2 ** 31, 2 ** 63 - 2, 0x9E3779B97F4A7C15, 2 ** 64 - 1):
        seeds = [ops.bert_layer_seed(seed, i) for i in range(48)]
        assert len(set(seeds)) == 48
        assert all(0 <= s < 2 ** 64 for s in seeds)
        assert seeds[0] == seed
