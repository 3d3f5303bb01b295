"""Host side of the f32 attention of the packed Llama TRAINING pass: the opt-in switches, the key work list of
`ops.causal_attn_f32_bwd`, the ctypes table against the header's section (9d), and the ISA scan of causal_attn_f32_bwd.hip.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

from test_llama_f32_host import LENS, ROOT, Tok, _llama


def test_switches_default_off_and_the_keyword_sets_both_model_attributes():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    assert PE.LLAMA_F32_ATTENTION_TRAIN is False and PE.LLAMA_F32_ATTENTION is False
    enc = _llama(PE)
    assert enc.f32_attention_train is False and enc.f32_attention is False
    m = rankpo_amd.ModelForTraining(encoder=enc, temperature=0.02)
    assert m.model.f32_attention_train is False and m.model.f32_attention is False
    m = rankpo_amd.ModelForTraining(encoder=_llama(PE), temperature=0.02, f32_attention=True)
    assert m.model.f32_attention_train is True and m.model.f32_attention is True
    # a BERT encoder is left untouched
    bert = PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                num_attention_heads=2))
    m = rankpo_amd.ModelForTraining(encoder=bert, temperature=0.02, f32_attention=True)
    assert not hasattr(m.model, "f32_attention_train") and not hasattr(m.model, "f32_attention")
    # ModelForInference keeps its meaning: the no-grad switch only
    inf = rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), f32_attention=True)
    assert inf.model.f32_attention is True and inf.model.f32_attention_train is False


def test_the_keyword_is_keyword_only():
    import rankpo_amd
    p = inspect.signature(rankpo_amd.ModelForTraining.__init__).parameters["f32_attention"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False


def test_varlen_ctx_keeps_its_constructor():
    from rankpo_amd import encoder as PE
    ctx = PE.VarlenCtx("cu", [3], 3, "t", "k", "f", "a", "b")
    assert (ctx.tiles, ctx.k_tiles, ctx.fwd_tiles, ctx.f32_tiles, ctx.f32_last_tiles) == ("t", "k", "f", "a", "b")
    assert ctx.f32_k_tiles is None and ctx.f32_last_k_tiles is None
    ctx = PE.VarlenCtx("cu", [3], 3, f32_k_tiles="c", f32_last_k_tiles="d")
    assert (ctx.tiles, ctx.f32_tiles, ctx.f32_k_tiles, ctx.f32_last_k_tiles) == (None, None, "c", "d")
    names = list(inspect.signature(PE.VarlenCtx.__init__).parameters)
    assert names == ["self", "cu", "lens", "max_len", "tiles", "k_tiles", "fwd_tiles", "f32_tiles", "f32_last_tiles", "f32_k_tiles",
                     "f32_last_k_tiles"]


@pytest.mark.parametrize("form", ["self", "last", "thirds", "none"])
def test_key_tile_list(form):
    from rankpo_amd import ops
    lens_k = LENS
    lens_q = {"self": LENS, "last": [1] * len(LENS), "thirds": [-(-n // 3) for n in LENS],
              "none": [0 if n % 2 else n for n in LENS]}[form]
    tl = ops.causal_attn_f32_key_tile_list(lens_q, lens_k)
    assert tl.dtype == np.int32 and tl.ndim == 2 and tl.shape[1] == 2
    want = sorted((n, k0) for n, lk in enumerate(lens_k) for k0 in range(0, lk, 32))
    assert sorted(map(tuple, tl.tolist())) == want                 # every (sequence, 32-key block) exactly once, lq == 0 included
    lq, lk = np.asarray(lens_q)[tl[:, 0]], np.asarray(lens_k)[tl[:, 0]]
    visible = lq - np.maximum(0, tl[:, 1] - (lk - lq))             # the queries that see the entry's first key
    assert (visible >= 0).all() and (np.diff(visible) <= 0).all()  # the entries with the most visible queries first
    assert visible[0] == max(lens_q)


def test_key_tile_list_refuses_what_the_query_list_refuses():
    from rankpo_amd import ops
    with pytest.raises(ValueError):
        ops.causal_attn_f32_key_tile_list([5, 9], [5, 8])
    with pytest.raises(ValueError):
        ops.causal_attn_f32_key_tile_list([2], [1, 1])
    assert ops.causal_attn_f32_key_tile_list([], []).shape == (0, 2)
    assert sorted(map(tuple, ops.causal_attn_f32_key_tile_list([0, 3], [4, 3]).tolist())) == [(0, 0), (1, 0)]
    assert ops.causal_attn_f32_key_tile_list([0, 0], [0, 0]).shape == (0, 2)


def test_entry_in_the_ctypes_table_matches_the_header():
    from rankpo_amd import _lib
    header = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    assert "(9d) backward of the causal f32 attention" in header
    sec = header[header.index("(9d) backward of the causal f32 attention"):header.index("(10) packed TRAINING step")]
    for word in ("deterministic", "Summation order", "Zero fill", "exact zeros"):
        assert word in sec, word
    res, args = _lib.SIGNATURES["rpo_causal_attn_bwd_f32"]
    decl = re.search(r"\bint rpo_causal_attn_bwd_f32\(([^;]*)\);", header)
    assert decl and res is _lib.SIGNATURES["rpo_causal_attn_fwd_f32"][0]
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 32 and "dtype" not in decl.group(1)
    for p, a in zip(params, args):
        want = _lib._vp if ("*" in p or "rpo_stream_t" in p) else _lib._f32 if p.startswith("float") else _lib._i64
        assert a is want, (p, a)
    # the forward entry is as it was
    assert len(_lib.SIGNATURES["rpo_causal_attn_fwd_f32"][1]) == 21


def test_kernel_source_is_plain_hip():
    src = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_f32_bwd.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", code)
    # what the four units share: held to the same rule
    common = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_common.hpp")).read()
    common = "\n".join(line.split("//")[0] for line in common.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt|atomic", common)
    assert '#include "causal_attn_common.hpp"' in src
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code
    mk = open(os.path.join(ROOT, "rankpo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^LLAMA_F32_BWD_SRCS := causal_attn_f32_bwd\.hip$", mk, re.M) and "$(LLAMA_F32_BWD_SRCS:.hip=.o)" in mk
    assert re.search(r"^LLAMA_F32_SRCS := causal_attn_f32\.hip$", mk, re.M)                     # the forward's list: as before


def test_backward_kernels_have_no_transcendental_hazard_and_no_scratch(tmp_path):
    """`make isa-llama-f32-bwd` writes the new file's ISA only; tools/check_trans_hazard.py passes on it; none of the 16
    instantiations (2 kernels x head_dim 64 / 128 x groups 1 / 2 / 4 / 8: what rpo_causal_attn_bwd_f32 dispatches) uses scratch."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rankpo_amd", "csrc"), "isa-llama-f32-bwd", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["causal_attn_f32_bwd.s"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    isa = open(files[0]).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len(sizes) == 16 and set(sizes) == {"0"}, sizes
    assert len(set(re.findall(r"\.name:\s*(\S*causal_attn_bwd_dq_f32_kernel\S*)", isa))) == 8
    assert len(set(re.findall(r"\.name:\s*(\S*causal_attn_bwd_dkdv_f32_kernel\S*)", isa))) == 8
