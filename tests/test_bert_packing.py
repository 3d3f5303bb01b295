"""Host logic of the packed BERT / XLM-R forward (`BertEncoder.pooled_cls`): packing and position ids against the padded
`BertEmbeddings` rules, the attention work list, and every condition under which the native path declines."""
import numpy as np
import pytest
import torch

from rankpo_amd import encoder as PE
from rankpo_amd import ops


def _padded_positions(ids, roberta, pad_id):
    """What the padded path feeds its position table (BertEmbeddings.forward / HF create_position_ids_from_input_ids)."""
    N, L = ids.shape
    if not roberta:
        return np.tile(np.arange(L), (N, 1))
    keep = (ids != pad_id).astype(np.int64)
    return np.cumsum(keep, 1) * keep + pad_id


def _batch(rs, pad_id):
    ids = rs.randint(5, 100, size=(4, 9))
    m = np.zeros((4, 9), dtype=np.int64)
    m[0, :9] = 1                                   # full row
    m[1, :3] = 1                                   # right-padded
    m[2, [0, 1, 4, 5, 8]] = 1                      # holes
    m[3, :6] = 1
    ids[3, 2] = pad_id                             # a pad id inside the mask
    ids[m == 0] = pad_id
    return ids, m


@pytest.mark.parametrize("roberta,pad_id", [(False, 0), (True, 1)])
def test_pack_matches_padded_embedding_rules(roberta, pad_id):
    rs = np.random.RandomState(3)
    ids, m = _batch(rs, pad_id)
    tt = rs.randint(0, 2, size=ids.shape)
    out = PE.bert_pack(torch.tensor(ids), torch.tensor(m), torch.tensor(tt), roberta=roberta, pad_id=pad_id)
    assert out is not None
    p_ids, p_pos, p_tt, lens = out
    keep = m.reshape(-1) == 1
    assert lens == m.sum(1).tolist()
    np.testing.assert_array_equal(p_ids.numpy(), ids.reshape(-1)[keep])
    np.testing.assert_array_equal(p_pos.numpy(), _padded_positions(ids, roberta, pad_id).reshape(-1)[keep])
    np.testing.assert_array_equal(p_tt.numpy(), tt.reshape(-1)[keep])
    # the first packed token of each row is its column-0 (CLS) token
    cu = np.concatenate([[0], np.cumsum(lens)])
    np.testing.assert_array_equal(p_ids.numpy()[cu[:-1]], ids[:, 0])
    assert PE.bert_pack(torch.tensor(ids), torch.tensor(m), None, roberta=roberta, pad_id=pad_id)[2] is None


def test_pack_declines_bad_masks():
    ids = torch.randint(5, 50, (3, 6))
    m = torch.ones(3, 6, dtype=torch.int64)
    assert PE.bert_pack(ids, m) is not None
    m2 = m.clone()
    m2[1, 3] = 2                                   # not 0/1
    assert PE.bert_pack(ids, m2) is None
    m3 = m.clone()
    m3[2, 0] = 0                                   # CLS column masked (left padding): HF reads a pad token's row
    assert PE.bert_pack(ids, m3) is None
    m4 = m.clone()
    m4[0] = 0                                      # a row with no token
    assert PE.bert_pack(ids, m4) is None


@pytest.mark.parametrize("lens_q,lens_k", [([1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 1000, 8192],) * 2,
                                           ([1] * 5, [3, 700, 1, 64, 65])])
def test_work_list_covers_every_query_tile_once_longest_first(lens_q, lens_k):
    qb = ops.BIDIR_ATTN_Q_BLOCK
    t = ops.bidir_attn_tile_list(lens_q, lens_k)
    assert t.dtype == np.int32 and t.shape[1] == 2
    want = sorted((s, q0) for s, n in enumerate(lens_q) for q0 in range(0, n, qb))
    assert sorted(map(tuple, t.tolist())) == want
    keys = [lens_k[s] for s in t[:, 0]]
    assert keys == sorted(keys, reverse=True)


def _bert(**kw):
    cfg = dict(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
               max_position_embeddings=32, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    cfg.update(kw)
    return PE.BertEncoder(PE.bert_config(**cfg))


def test_every_decline_condition(monkeypatch):
    ids = torch.randint(5, 50, (2, 7))
    m = torch.ones(2, 7, dtype=torch.int64)
    enc = _bert().eval()
    assert enc.native_decline_reason() is not None            # grad mode on, and a CPU model
    with torch.no_grad():
        assert enc.native_decline_reason() == "not on a HIP device"
        assert enc.pooled_cls(ids, m) is None
    # with the device test passed, each remaining condition declines on its own
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)
    assert enc.native_decline_reason() == "grad enabled"
    with torch.inference_mode():
        assert enc.native_decline_reason() == "storage dtype"               # f32
        h = enc.to(torch.float16)
        assert h.native_decline_reason() is None
        monkeypatch.setattr(PE, "BERT_NATIVE", False)
        assert h.native_decline_reason() == "BERT_NATIVE is off"
        monkeypatch.setattr(PE, "BERT_NATIVE", True)
        assert _bert(hidden_size=96, num_attention_heads=1).half().eval().native_decline_reason() == "shape"   # head_dim 96
        assert _bert(hidden_size=128, num_attention_heads=1).half().eval().native_decline_reason() == "shape"  # head_dim 128
        assert _bert(hidden_act="gelu_new").half().eval().native_decline_reason() == "activation"
        tr = _bert(hidden_dropout_prob=0.1).half().train()
        assert tr.native_decline_reason() == "training with dropout"
        assert _bert().half().train().native_decline_reason() is None      # train mode, every p == 0
        # mask / id declines return None before anything touches a device
        assert h.pooled_cls(ids, None) is None
        bad = m.clone()
        bad[0, 0] = 0
        assert h.pooled_cls(ids, bad) is None
        bad = m.clone()
        bad[1, 2] = 3
        assert h.pooled_cls(ids, bad) is None
        big = ids.clone()
        big[0, 1] = 64                                                      # outside the vocabulary
        assert h.pooled_cls(big, m) is None
        far = torch.randint(5, 50, (1, 40))                                 # position 32+ outside the table
        assert h.pooled_cls(far, torch.ones_like(far)) is None


def test_bert_kernels_have_no_transcendental_hazard(tmp_path):
    """The ISA scan tests/test_host_logic.py runs over the library's other sources, for bert_ops.hip (`make isa-bert`)."""
    import os
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    root = os.path.join(os.path.dirname(__file__), "..")
    subprocess.run(["make", "-s", "-C", os.path.join(root, "rankpo_amd", "csrc"), "isa-bert", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["bert_ops.s"]
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
