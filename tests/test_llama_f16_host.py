"""Host side of the native fp16 pass of a Llama encoder: the opt-in switches, the work list of `ops.causal_attn_f16`, the ctypes
table against the header's section (9e), the source rules and the ISA scan of causal_attn_f16.hip, and the gates of the fp16 row
kernels.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Tok:
    pad_token = "<pad>"
    padding_side = "right"

    def __call__(self, texts, padding=True, truncation=True, max_length=512, return_tensors="pt"):
        ids = [[1 + (ord(c) * 7 + i) % 60 for i, c in enumerate(t)][:max_length] for t in texts]
        L = max(len(x) for x in ids)
        return {"input_ids": torch.tensor([x + [0] * (L - len(x)) for x in ids]),
                "attention_mask": torch.tensor([[1] * len(x) + [0] * (L - len(x)) for x in ids])}


def _llama(PE):
    torch.manual_seed(3)
    return PE.build_encoder(PE.llama_config(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=2,
                                            num_attention_heads=2, num_key_value_heads=1, head_dim=64, pad_token_id=0))


def test_switches_default_off_and_the_keyword_sets_the_model_attribute():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    assert PE.LLAMA_FP16_NATIVE is False
    enc = _llama(PE)
    assert enc.native_fp16 is False
    assert rankpo_amd.ModelForInference(encoder=enc, tokenizer=Tok()).model.native_fp16 is False
    assert rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), native_fp16=True).model.native_fp16 is True
    # the other keywords leave the attribute alone
    inf = rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), packed_f32=True, f32_attention=True)
    assert inf.model.native_fp16 is False and inf.model.f32_attention is True
    # a BERT encoder takes the keyword and is left untouched
    bert = PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                num_attention_heads=2))
    inf = rankpo_amd.ModelForInference(encoder=bert, tokenizer=Tok(), native_fp16=True)
    assert not hasattr(inf.model, "native_fp16") and inf.model.native_f32 is False


def test_the_keyword_is_keyword_only():
    import rankpo_amd
    p = inspect.signature(rankpo_amd.ModelForInference.__init__).parameters["native_fp16"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    names = list(inspect.signature(rankpo_amd.ModelForInference.__init__).parameters)
    assert names.index("native_fp16") > names.index("f32_attention") > names.index("packed_f32")
    with pytest.raises(TypeError):
        rankpo_amd.ModelForInference(None, None, True, False, False, 0, None, None, Tok(), False, False, True)


def test_cpu_model_and_bert_are_unaffected(monkeypatch):
    """On the CPU the keyword and the module switch are inert: the rows are the switch-off rows, bit for bit."""
    import rankpo_amd
    from rankpo_amd import encoder as PE, ops
    tok = Tok()(["abc", "a", "hello world, hello", "xyzzy" * 5], max_length=32)
    ids, mask = tok["input_ids"], tok["attention_mask"]
    called = []
    monkeypatch.setattr(ops, "causal_attn_f16", lambda *a, **k: called.append(1))
    bert = lambda: PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                        num_attention_heads=2)).eval()
    rows = {"llama": lambda m: m.pooled_last_token(ids, mask), "bert": lambda m: m(ids, mask).last_hidden_state[:, 0]}
    for name, make in (("llama", lambda: _llama(PE)), ("bert", bert)):
        torch.manual_seed(5)
        a = rankpo_amd.ModelForInference(encoder=make(), tokenizer=Tok(), device="cpu").model
        torch.manual_seed(5)
        b = rankpo_amd.ModelForInference(encoder=make(), tokenizer=Tok(), device="cpu", native_fp16=True).model
        assert a.embed_tokens.weight.device.type == "cpu" if name == "llama" else True
        with torch.no_grad():
            ra = rows[name](a)
            with monkeypatch.context() as m:
                m.setattr(PE, "LLAMA_FP16_NATIVE", True)
                rb = rows[name](b)
        assert ra.dtype == torch.float32 and torch.isfinite(ra).all() and torch.equal(ra, rb), name
    assert not called


def test_varlen_ctx_keeps_its_constructor():
    """The old positional call and the pinned parameter list stand (tests/test_llama_f32_train_host.py compares the whole list, so
    the fp16 work lists are attributes with default None that the encoder sets, not constructor arguments)."""
    from rankpo_amd import encoder as PE
    ctx = PE.VarlenCtx("cu", [3], 3, "t", "k", "f", "a", "b", "c", "d")
    assert (ctx.tiles, ctx.k_tiles, ctx.fwd_tiles, ctx.f32_tiles, ctx.f32_last_tiles, ctx.f32_k_tiles, ctx.f32_last_k_tiles) == \
        ("t", "k", "f", "a", "b", "c", "d")
    assert ctx.f16_tiles is None and ctx.f16_last_tiles is None
    names = list(inspect.signature(PE.VarlenCtx.__init__).parameters)
    assert names == ["self", "cu", "lens", "max_len", "tiles", "k_tiles", "fwd_tiles", "f32_tiles", "f32_last_tiles", "f32_k_tiles",
                     "f32_last_k_tiles"]
    ctx.f16_tiles, ctx.f16_last_tiles = "x", "y"
    assert PE.VarlenCtx("cu", [3], 3).f16_tiles is None                                     # per object, not shared


LENS = [1, 32, 33, 1000, 31, 64, 7, 1000, 65]


@pytest.mark.parametrize("form", ["self", "last", "thirds"])
def test_tile_list(form):
    from rankpo_amd import ops
    lens_k = LENS
    lens_q = {"self": LENS, "last": [1] * len(LENS), "thirds": [-(-n // 3) for n in LENS]}[form]
    tl = ops.causal_attn_f16_tile_list(lens_q, lens_k)
    assert ops.CAUSAL_ATTN_F16_Q_BLOCK == 32
    assert tl.dtype == np.int32 and tl.ndim == 2 and tl.shape[1] == 2
    # brute force: every (sequence, 32-query block) exactly once, and the last key that each entry's last query sees
    want = {}
    for n, (lq, lk) in enumerate(zip(lens_q, lens_k)):
        for q0 in range(0, lq, 32):
            want[(n, q0)] = max(j for i in range(q0, min(q0 + 32, lq)) for j in range(lk) if j <= i + (lk - lq))
    assert sorted(map(tuple, tl.tolist())) == sorted(want)
    last = np.array([want[tuple(e)] for e in tl.tolist()])
    assert (np.diff(last) <= 0).all()                              # the longest-running entries first
    assert last[0] == max(lens_k) - 1
    if form == "last":
        assert len(tl) == len(LENS) and (tl[:, 1] == 0).all()      # one entry per sequence
    # one list format for the f32 and the fp16 kernel
    np.testing.assert_array_equal(tl, ops.causal_attn_f32_tile_list(lens_q, lens_k))


def test_tile_list_refuses_queries_in_front_of_every_key():
    from rankpo_amd import ops
    with pytest.raises(ValueError):
        ops.causal_attn_f16_tile_list([5, 9], [5, 8])
    with pytest.raises(ValueError):
        ops.causal_attn_f16_tile_list([2], [1, 1])
    assert ops.causal_attn_f16_tile_list([], []).shape == (0, 2)
    assert ops.causal_attn_f16_tile_list([0, 3], [4, 3]).tolist() == [[1, 0]]


def test_entry_in_the_ctypes_table_matches_the_header():
    from rankpo_amd import _lib
    header = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    assert "(9e) causal fp16 attention" in header
    sec = header[header.index("(9e) causal fp16 attention"):header.index("(10) packed TRAINING step")]
    for word in ("deterministic", "j <= i + (lk - lq)", "v_mfma_f32_16x16x32_f16", "modeling.py:453-454", "RPO_ERR_UNSUPPORTED",
                 "% 8 == 0", "rounded to fp16 exactly once"):
        assert word in sec, word
    assert "f32, bf16 or fp16" in header[:header.index("#ifndef RANKPO_HIP_H")]
    res, args = _lib.SIGNATURES["rpo_causal_attn_fwd_f16"]
    decl = re.search(r"\bint rpo_causal_attn_fwd_f16\(([^;]*)\);", header)
    decl32 = re.search(r"\bint rpo_causal_attn_fwd_f32\(([^;]*)\);", header)
    assert decl and decl32 and res is _lib.SIGNATURES["rpo_causal_attn_fwd_f32"][0]
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 21 and "dtype" not in decl.group(1)
    for p, a in zip(params, args):
        want = _lib._vp if ("*" in p or "rpo_stream_t" in p) else _lib._f32 if p.startswith("float") else _lib._i64
        assert a is want, (p, a)
    # the argument order of rpo_causal_attn_fwd_f32: the same ctypes row and the same declaration, names included
    assert args == _lib.SIGNATURES["rpo_causal_attn_fwd_f32"][1]
    assert params == [p.strip() for p in decl32.group(1).split(",")]


def test_kernel_source_is_plain_hip():
    src = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_f16.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", code)
    # what the four units share: held to the same rule
    common = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_common.hpp")).read()
    common = "\n".join(line.split("//")[0] for line in common.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", common)
    assert '#include "causal_attn_common.hpp"' in src
    assert "__builtin_amdgcn_mfma_f32_16x16x32_f16" in code
    mk = open(os.path.join(ROOT, "rankpo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^LLAMA_F16_SRCS := causal_attn_f16\.hip$", mk, re.M) and "$(LLAMA_F16_SRCS:.hip=.o)" in mk
    # the pinned lines: as before
    for line in (r"SRCS := pool_normalize\.hip infonce\.hip rankpo\.hip optim\.hip encoder_ops\.hip attention\.hip lastq_attention\.hip "
                 r"topk\.hip", r"BERT_SRCS := bert_ops\.hip", r"EMBED_SRCS := embed_grad\.hip", r"LLAMA_F32_SRCS := causal_attn_f32\.hip",
                 r"LLAMA_F32_BWD_SRCS := causal_attn_f32_bwd\.hip"):
        assert re.search("^" + line + "$", mk, re.M), line
    assert re.search(r"^\.isa_checked: attention\.hip infonce\.hip \$\(INCS\)", mk, re.M)


def test_causal_f16_kernel_has_no_transcendental_hazard_and_no_scratch(tmp_path):
    """`make isa-llama-f16` writes the new file's ISA only, with the flags of the build; tools/check_trans_hazard.py passes on it;
    none of the 8 instantiations (head_dim 64 / 128 x groups 1 / 2 / 4 / 8: what rpo_causal_attn_fwd_f16 dispatches) uses scratch."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rankpo_amd", "csrc"), "isa-llama-f16", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["causal_attn_f16.s"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    isa = open(files[0]).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len(sizes) == 8 and set(sizes) == {"0"}, sizes
    assert len(set(re.findall(r"\.name:\s*(\S*causal_attn_fwd_f16_kernel\S*)", isa))) == 8
    assert "v_mfma_f32_16x16x32_f16" in isa


def test_gates_refuse_cpu_and_fp16_outside_the_pass():
    from rankpo_amd import ops
    q = torch.zeros(4, 2, 64, dtype=torch.float16)
    assert not ops.causal_attn_f16_ok(q, q[:, :1], q[:, :1])                    # CPU tensors
    with pytest.raises(ValueError):
        ops.causal_attn_f16(q, q, q, None, None, None, 0.125)
    assert ops.causal_attn_f16_shape_ok(32, 8, 64) and ops.causal_attn_f16_shape_ok(8, 8, 128)
    assert not ops.causal_attn_f16_shape_ok(6, 2, 64) and not ops.causal_attn_f16_shape_ok(16, 1, 64)
    assert not ops.causal_attn_f16_shape_ok(4, 2, 96) and not ops.causal_attn_f16_shape_ok(3, 2, 64)
    x = torch.zeros(3, 128, dtype=torch.float16)
    assert not ops.fused_encoder_ops_ok(x) and not ops.fused_encoder_ops_ok(x, 64) and not ops.fused_norm_ok(x)
    with torch.no_grad(), ops.fp16_native():                                     # the context alone does not open them on the CPU
        assert ops.fp16_native.active()
        assert not ops.fused_encoder_ops_ok(x) and not ops.fused_norm_ok(x)
    assert not ops.fp16_native.active()
