"""Host side of the packed f32 forward: the opt-in switches, the decline rule for float32 storage, and the ctypes table against
the header's section (9b).  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Tok:
    pad_token = "<pad>"
    padding_side = "right"


def _bert(PE, **kw):
    return PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                num_attention_heads=2, **kw))


def test_switches_default_off_and_packed_f32_sets_the_model_attribute():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    assert PE.BERT_NATIVE_F32 is False
    enc = _bert(PE)
    assert enc.native_f32 is False
    assert rankpo_amd.ModelForInference(encoder=enc, tokenizer=Tok()).model.native_f32 is False
    assert rankpo_amd.ModelForInference(encoder=_bert(PE), tokenizer=Tok(), packed_f32=True).model.native_f32 is True
    with pytest.raises(TypeError):                              # keyword-only
        rankpo_amd.ModelForInference(None, None, True, False, False, 0, True)
    llama = PE.build_encoder(PE.llama_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                             num_attention_heads=2, num_key_value_heads=1, head_dim=32, pad_token_id=0))
    inf = rankpo_amd.ModelForInference(encoder=llama, tokenizer=Tok(), packed_f32=True)       # ignored for Llama
    assert not hasattr(inf.model, "native_f32")


def test_decline_rule_for_f32_storage(monkeypatch):
    from rankpo_amd import encoder as PE
    monkeypatch.setattr(PE, "_on_hip_device", lambda t: True)   # the rule itself is host logic
    enc = _bert(PE).eval()
    with torch.no_grad():
        assert enc.native_decline_reason() == "storage dtype"  # f32, both switches off: as ever
        enc.native_f32 = True
        assert enc.native_decline_reason() is None
        enc.native_f32 = False
        monkeypatch.setattr(PE, "BERT_NATIVE_F32", True)
        assert enc.native_decline_reason() is None
        assert enc.double().native_decline_reason() == "storage dtype"         # only float32 is opted in
        enc.float()
        monkeypatch.setattr(PE, "BERT_NATIVE", False)
        assert enc.native_decline_reason() == "BERT_NATIVE is off"
        monkeypatch.setattr(PE, "BERT_NATIVE", True)
        enc.train()
        assert enc.native_decline_reason() == "training with dropout"
        enc.eval()
        assert enc.half().native_decline_reason() is None      # 16-bit storage never asked for the switch
    enc.float()
    assert enc.native_decline_reason() == "grad enabled"
    # the training step has no f32 form, whatever the switches say
    enc.native_f32 = True
    enc.train()
    assert enc.native_train_decline_reason() == "storage dtype"


def test_f32_entries_in_the_ctypes_table_match_the_header():
    from rankpo_amd import _lib
    header = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    assert "(9b) f32 storage" in header
    for base in ("rpo_bidir_attn_fwd", "rpo_add_layernorm_fwd", "rpo_gelu_fwd", "rpo_bert_embed_ln_fwd"):
        res, args = _lib.SIGNATURES[base + "_f32"]
        sres, sargs = _lib.SIGNATURES[base]
        drop = [i for i, a in enumerate(sargs) if a is _lib._i32]
        assert res is sres and len(drop) == 1                   # the sibling's list without its one `int dtype`
        assert args == sargs[:drop[0]] + sargs[drop[0] + 1:]
        decl = re.search(r"\bint " + base + r"_f32\(([^;]*)\);", header)
        assert decl and len(decl.group(1).split(",")) == len(args) and "dtype" not in decl.group(1)
