"""Host side of the fp16 attention of the packed Llama TRAINING pass: the opt-in switches, the key work list of
`ops.causal_attn_f16_bwd`, the ctypes table against the header's section (9f), the source rules and the ISA scan of
causal_attn_f16_bwd.hip.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_llama_f16_host import ROOT, Tok, _llama

LENS = [1, 32, 33, 1000, 31, 64, 7, 1000, 65]


def test_switches_default_off_and_the_keyword_sets_both_model_attributes():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    assert PE.LLAMA_FP16_NATIVE_TRAIN is False and PE.LLAMA_FP16_NATIVE is False
    enc = _llama(PE)
    assert enc.native_fp16_train is False and enc.native_fp16 is False
    m = rankpo_amd.ModelForTraining(encoder=enc, temperature=0.02)
    assert m.model.native_fp16_train is False and m.model.native_fp16 is False
    m = rankpo_amd.ModelForTraining(encoder=_llama(PE), temperature=0.02, native_fp16=True)
    assert m.model.native_fp16_train is True and m.model.native_fp16 is True
    assert m.model.f32_attention_train is False and m.model.f32_attention is False
    # the other keyword leaves the attributes alone
    m = rankpo_amd.ModelForTraining(encoder=_llama(PE), temperature=0.02, f32_attention=True)
    assert m.model.native_fp16_train is False and m.model.native_fp16 is False and m.model.f32_attention_train is True
    # a BERT encoder takes the keyword and is left untouched
    bert = PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                num_attention_heads=2))
    m = rankpo_amd.ModelForTraining(encoder=bert, temperature=0.02, native_fp16=True)
    assert not hasattr(m.model, "native_fp16_train") and not hasattr(m.model, "native_fp16")
    # ModelForInference keeps its meaning: the no-grad switch only
    inf = rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), native_fp16=True)
    assert inf.model.native_fp16 is True and inf.model.native_fp16_train is False


def test_the_keyword_is_keyword_only():
    import rankpo_amd
    p = inspect.signature(rankpo_amd.ModelForTraining.__init__).parameters["native_fp16"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    names = list(inspect.signature(rankpo_amd.ModelForTraining.__init__).parameters)
    assert names.index("native_fp16") > names.index("f32_attention")
    # ModelForInference's parameter list is as it was
    names = list(inspect.signature(rankpo_amd.ModelForInference.__init__).parameters)
    assert names[-1] == "native_fp16" and "native_fp16_train" not in names


def test_varlen_ctx_keeps_its_constructor_and_the_lists_are_attributes():
    from rankpo_amd import encoder as PE
    names = list(inspect.signature(PE.VarlenCtx.__init__).parameters)
    assert names == ["self", "cu", "lens", "max_len", "tiles", "k_tiles", "fwd_tiles", "f32_tiles", "f32_last_tiles", "f32_k_tiles",
                     "f32_last_k_tiles"]
    a, b = PE.VarlenCtx("cu", [3], 3), PE.VarlenCtx("cu", [3], 3)
    assert a.f16_k_tiles is None and a.f16_last_k_tiles is None and a.f16_tiles is None and a.f16_last_tiles is None
    a.f16_k_tiles, a.f16_last_k_tiles = "k", "l"                  # set per object: the class and other objects keep None
    assert b.f16_k_tiles is None and b.f16_last_k_tiles is None
    assert PE.VarlenCtx.f16_k_tiles is None and PE.VarlenCtx.f16_last_k_tiles is None


def test_cpu_model_runs_what_it_ran(monkeypatch):
    """Switch and keyword on a CPU fp16-less model: no list is built, the step is the switch-off step bit for bit."""
    import rankpo_amd
    from rankpo_amd import encoder as PE
    tok = Tok()(["ab", "cdefg", "abc", "d", "efghij", "kl"])

    def step(**kw):
        m = rankpo_amd.ModelForTraining(encoder=_llama(PE), temperature=0.02, **kw).train()
        pooled = m.model.pooled_last_token(tok["input_ids"], tok["attention_mask"])
        pooled.sum().backward()
        return pooled.detach(), {k: p.grad.clone() for k, p in m.model.named_parameters()}
    a = step()
    monkeypatch.setattr(PE, "LLAMA_FP16_NATIVE_TRAIN", True)
    b = step(native_fp16=True)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("form", ["self", "last", "thirds"])
def test_key_tile_list_is_the_f32_list(form):
    from rankpo_amd import ops
    assert ops.causal_attn_f16_key_tile_list is ops.causal_attn_f32_key_tile_list
    assert ops.causal_attn_f16_key_tile_table is ops.causal_attn_f32_key_tile_table
    lens_q = {"self": LENS, "last": [1] * len(LENS), "thirds": [-(-n // 3) for n in LENS]}[form]
    tl = ops.causal_attn_f16_key_tile_list(lens_q, LENS)
    assert tl.dtype == np.int32 and tl.ndim == 2 and tl.shape[1] == 2
    np.testing.assert_array_equal(tl, ops.causal_attn_f32_key_tile_list(lens_q, LENS))
    want = sorted((n, k0) for n, lk in enumerate(LENS) for k0 in range(0, lk, 32))
    assert sorted(map(tuple, tl.tolist())) == want                 # every (sequence, 32-key block) exactly once
    with pytest.raises(ValueError):
        ops.causal_attn_f16_key_tile_list([5, 9], [5, 8])


def test_raw_op_refuses_cpu_tensors():
    from rankpo_amd import ops
    q = torch.zeros(4, 2, 64, dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.causal_attn_f16_bwd(q, q, q, q.view(4, -1), torch.zeros(2, 4), q.view(4, -1), None, None, None, None, 0.125)


def test_entry_in_the_ctypes_table_matches_the_header():
    from rankpo_amd import _lib
    header = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    assert "(9f) backward of the causal fp16 attention" in header
    sec = header[header.index("(9f) backward of the causal fp16 attention"):header.index("(10) packed TRAINING step")]
    for word in ("exactly once", "v_mfma_f32_16x16x32_f16", "deterministic", "RPO_ERR_UNSUPPORTED", "% 8 == 0", "j <= i + (lk - lq)",
                 "Summation order", "Zero fill", "exact zeros", "num_heads * total_q", "hi + lo"):
        assert word in sec, word
    # the very row of the f32 backward
    assert _lib.SIGNATURES["rpo_causal_attn_bwd_f16"] is _lib.SIGNATURES["rpo_causal_attn_bwd_f32"]
    res, args = _lib.SIGNATURES["rpo_causal_attn_bwd_f16"]
    decl = re.search(r"\bint rpo_causal_attn_bwd_f16\(([^;]*)\);", header)
    decl32 = re.search(r"\bint rpo_causal_attn_bwd_f32\(([^;]*)\);", header)
    assert decl and decl32 and res is _lib.SIGNATURES["rpo_causal_attn_fwd_f16"][0]
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 32 and "dtype" not in decl.group(1)
    for p, a in zip(params, args):
        want = _lib._vp if ("*" in p or "rpo_stream_t" in p) else _lib._f32 if p.startswith("float") else _lib._i64
        assert a is want, (p, a)
    # the same declaration as the f32 backward, names included
    assert params == [p.strip() for p in decl32.group(1).split(",")]
    # the forward entries are as they were
    assert len(_lib.SIGNATURES["rpo_causal_attn_fwd_f16"][1]) == 21 and len(_lib.SIGNATURES["rpo_causal_attn_fwd_f32"][1]) == 21


def test_kernel_source_is_plain_hip():
    src = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_f16_bwd.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", code)
    # what the four units share: held to the same rule
    common = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_common.hpp")).read()
    common = "\n".join(line.split("//")[0] for line in common.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", common)
    assert '#include "causal_attn_common.hpp"' in src
    assert "__builtin_amdgcn_mfma_f32_16x16x32_f16" in code
    mk = open(os.path.join(ROOT, "rankpo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^LLAMA_F16_BWD_SRCS := causal_attn_f16_bwd\.hip$", mk, re.M) and "$(LLAMA_F16_BWD_SRCS:.hip=.o)" in mk
    assert re.search(r"^OBJS \+= \$\(LLAMA_F16_BWD_SRCS:\.hip=\.o\)$", mk, re.M)
    assert re.search(r"^FLAGS_causal_attn_f16_bwd :=", mk, re.M)
    # the pinned lines: as before
    for line in (r"LLAMA_F16_SRCS := causal_attn_f16\.hip", r"LLAMA_F32_BWD_SRCS := causal_attn_f32_bwd\.hip",
                 r"LLAMA_F32_SRCS := causal_attn_f32\.hip"):
        assert re.search("^" + line + "$", mk, re.M), line


def test_backward_kernels_have_no_transcendental_hazard_and_no_scratch(tmp_path):
    """`make isa-llama-f16-bwd` writes the new file's ISA only, with the flags of the build; tools/check_trans_hazard.py passes on
    it; none of the 16 instantiations (2 kernels x head_dim 64 / 128 x groups 1 / 2 / 4 / 8: what rpo_causal_attn_bwd_f16
    dispatches) uses scratch."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rankpo_amd", "csrc"), "isa-llama-f16-bwd", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["causal_attn_f16_bwd.s"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    isa = open(files[0]).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len(sizes) == 16 and set(sizes) == {"0"}, sizes
    names = set(re.findall(r"\.name:\s*(\S*causal_attn_bwd_\w+_f16_kernel\S*)", isa))
    assert len(names) == 16, names
    assert len({n for n in names if "causal_attn_bwd_dq_f16_kernel" in n}) == 8
    assert len({n for n in names if "causal_attn_bwd_dkdv_f16_kernel" in n}) == 8
    assert "v_mfma_f32_16x16x32_f16" in isa
