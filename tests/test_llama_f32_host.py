"""Host side of the f32 attention of the packed Llama pass: the opt-in switches, the work list of `ops.causal_attn_f32`, the ctypes
table against the header's section (9c), and the ISA scan of causal_attn_f32.hip.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Tok:
    pad_token = "<pad>"
    padding_side = "right"


def _llama(PE):
    return PE.build_encoder(PE.llama_config(vocab_size=64, hidden_size=128, intermediate_size=128, num_hidden_layers=1,
                                            num_attention_heads=2, num_key_value_heads=1, head_dim=64, pad_token_id=0))


def test_switches_default_off_and_the_keyword_sets_the_model_attribute():
    import rankpo_amd
    from rankpo_amd import encoder as PE
    assert PE.LLAMA_F32_ATTENTION is False
    enc = _llama(PE)
    assert enc.f32_attention is False
    assert rankpo_amd.ModelForInference(encoder=enc, tokenizer=Tok()).model.f32_attention is False
    assert rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), f32_attention=True).model.f32_attention is True
    # packed_f32 stays "BERT family only": a Llama encoder is left untouched
    inf = rankpo_amd.ModelForInference(encoder=_llama(PE), tokenizer=Tok(), packed_f32=True)
    assert inf.model.f32_attention is False and not hasattr(inf.model, "native_f32")
    # and f32_attention leaves a BERT encoder untouched
    bert = PE.build_encoder(PE.bge_small_config(vocab_size=64, hidden_size=64, intermediate_size=128, num_hidden_layers=1,
                                                num_attention_heads=2))
    inf = rankpo_amd.ModelForInference(encoder=bert, tokenizer=Tok(), f32_attention=True)
    assert inf.model.native_f32 is False and not hasattr(inf.model, "f32_attention")


def test_the_keyword_is_keyword_only():
    import rankpo_amd
    p = inspect.signature(rankpo_amd.ModelForInference.__init__).parameters["f32_attention"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    with pytest.raises(TypeError):
        rankpo_amd.ModelForInference(None, None, True, False, False, 0, None, None, Tok(), False, True)


def test_varlen_ctx_keeps_its_constructor():
    from rankpo_amd import encoder as PE
    ctx = PE.VarlenCtx("cu", [3], 3, "t", "k", "f")
    assert (ctx.tiles, ctx.k_tiles, ctx.fwd_tiles, ctx.f32_tiles, ctx.f32_last_tiles) == ("t", "k", "f", None, None)
    ctx = PE.VarlenCtx("cu", [3], 3, f32_tiles="a", f32_last_tiles="b")
    assert (ctx.tiles, ctx.f32_tiles, ctx.f32_last_tiles) == (None, "a", "b")


LENS = [1, 32, 33, 1000, 31, 64, 7, 1000, 65]


def _last_key(tl, lens_q, lens_k):
    lq, lk = np.asarray(lens_q)[tl[:, 0]], np.asarray(lens_k)[tl[:, 0]]
    return np.minimum(tl[:, 1] + 32, lq) - 1 + (lk - lq)


@pytest.mark.parametrize("form", ["self", "last", "thirds"])
def test_tile_list(form):
    from rankpo_amd import ops
    lens_k = LENS
    lens_q = {"self": LENS, "last": [1] * len(LENS), "thirds": [-(-n // 3) for n in LENS]}[form]
    tl = ops.causal_attn_f32_tile_list(lens_q, lens_k)
    assert tl.dtype == np.int32 and tl.ndim == 2 and tl.shape[1] == 2
    want = sorted((n, q0) for n, lq in enumerate(lens_q) for q0 in range(0, lq, 32))
    assert sorted(map(tuple, tl.tolist())) == want                 # every (sequence, 32-query block) exactly once
    last = _last_key(tl, lens_q, lens_k)
    assert (np.diff(last) <= 0).all()                              # the longest-running entries first
    assert last[0] == max(lens_k) - 1
    if form == "last":
        assert len(tl) == len(LENS) and (tl[:, 1] == 0).all()      # one entry per sequence


def test_tile_list_refuses_queries_in_front_of_every_key():
    from rankpo_amd import ops
    with pytest.raises(ValueError):
        ops.causal_attn_f32_tile_list([5, 9], [5, 8])
    with pytest.raises(ValueError):
        ops.causal_attn_f32_tile_list([2], [1, 1])
    assert ops.causal_attn_f32_tile_list([], []).shape == (0, 2)
    assert ops.causal_attn_f32_tile_list([0, 3], [4, 3]).tolist() == [[1, 0]]


def test_entry_in_the_ctypes_table_matches_the_header():
    from rankpo_amd import _lib
    header = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    assert "(9c) causal f32 attention" in header
    res, args = _lib.SIGNATURES["rpo_causal_attn_fwd_f32"]
    decl = re.search(r"\bint rpo_causal_attn_fwd_f32\(([^;]*)\);", header)
    assert decl and res is _lib.SIGNATURES["rpo_bidir_attn_fwd_f32"][0]
    params = [p.strip() for p in decl.group(1).split(",")]
    assert len(params) == len(args) == 21 and "dtype" not in decl.group(1)
    # pointers, 64-bit integers and the one float, position by position
    for p, a in zip(params, args):
        want = _lib._vp if ("*" in p or "rpo_stream_t" in p) else _lib._f32 if p.startswith("float") else _lib._i64
        assert a is want, (p, a)
    # the argument order of rpo_bidir_attn_fwd_f32
    assert args == _lib.SIGNATURES["rpo_bidir_attn_fwd_f32"][1]


def test_kernel_source_is_plain_hip():
    """What the issue asks of the translation unit: no asm statements and no counted waits, so none of the build's ISA signature
    checks has to know about it; and the Makefile links it from a list of its own."""
    src = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_f32.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt", code)
    # what the four units share: held to the same rule
    common = open(os.path.join(ROOT, "rankpo_amd", "csrc", "causal_attn_common.hpp")).read()
    common = "\n".join(line.split("//")[0] for line in common.splitlines())
    assert not re.search(r"\basm\b|__asm__|s_waitcnt|__builtin_amdgcn_s_waitcnt", common)
    assert '#include "causal_attn_common.hpp"' in src
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in code
    mk = open(os.path.join(ROOT, "rankpo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^LLAMA_F32_SRCS := causal_attn_f32\.hip$", mk, re.M) and "$(LLAMA_F32_SRCS:.hip=.o)" in mk
    assert re.search(r"^\.isa_checked: attention\.hip infonce\.hip \$\(INCS\)", mk, re.M)       # the checked files: as before


def test_causal_f32_kernel_has_no_transcendental_hazard(tmp_path):
    """The ISA scan tests/test_host_logic.py runs over the library's other sources, for causal_attn_f32.hip
    (`make isa-llama-f32`)."""
    import shutil
    import subprocess
    import sys
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rankpo_amd", "csrc"), "isa-llama-f32", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["causal_attn_f32.s"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    # the kernel must not spill: no scratch in any of its instantiations
    isa = open(files[0]).read()
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", isa)
    assert len(sizes) == 8 and set(sizes) == {"0"}, sizes
