"""Host side of how a packed Llama pass picks its attention: which op `_varlen_causal_attention` / `_varlen_last_query_attention`
call for every storage dtype, grad mode and set of work lists, and which lists `_native_attention_lists` builds for each of the
four opt-in switches.  The ops are stubs that record their names.  No GPU."""
import pytest
import torch

from test_llama_f16_host import _llama

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
QUERY_LISTS = {"f32": ("f32_tiles", "f32_last_tiles"), "f16": ("f16_tiles", "f16_last_tiles")}
KEY_LISTS = {"f32": ("f32_k_tiles", "f32_last_k_tiles"), "f16": ("f16_k_tiles", "f16_last_k_tiles")}
# which attributes of the VarlenCtx are set (each to its own name, so that a stub can tell which list it was handed)
LISTS = {"none": (), "hand": ("tiles", "k_tiles"), "f16": QUERY_LISTS["f16"], "f16_train": QUERY_LISTS["f16"] + KEY_LISTS["f16"],
         "f32": QUERY_LISTS["f32"], "f32_train": QUERY_LISTS["f32"] + KEY_LISTS["f32"],
         "all": ("tiles", "k_tiles") + QUERY_LISTS["f16"] + KEY_LISTS["f16"] + QUERY_LISTS["f32"] + KEY_LISTS["f32"]}

HAND, FLASH, SDPA = "flash_attn_varlen", "aten._flash_attention_forward", "scaled_dot_product_attention"
A16, T16, A32, T32 = "causal_attn_f16", "causal_attn_f16_train", "causal_attn_f32", "causal_attn_f32_train"
# (dtype, lists) -> what is called on (a HIP tensor under no-grad, a HIP tensor under grad mode, a CPU tensor under no-grad, a CPU
# tensor under grad mode); written out from the branches of the two functions as they stood before they shared one native branch
FULL = {
    (BF16, "none"): (FLASH, FLASH, SDPA, SDPA), (BF16, "hand"): (HAND, HAND, SDPA, SDPA),
    (BF16, "f16"): (FLASH, FLASH, SDPA, SDPA), (BF16, "f16_train"): (FLASH, FLASH, SDPA, SDPA),
    (BF16, "f32"): (FLASH, FLASH, SDPA, SDPA), (BF16, "f32_train"): (FLASH, FLASH, SDPA, SDPA),
    (BF16, "all"): (HAND, HAND, SDPA, SDPA),
    (F16, "none"): (FLASH, FLASH, SDPA, SDPA), (F16, "hand"): (FLASH, FLASH, SDPA, SDPA),
    (F16, "f16"): (A16, FLASH, A16, SDPA), (F16, "f16_train"): (A16, T16, A16, T16),
    (F16, "f32"): (FLASH, FLASH, SDPA, SDPA), (F16, "f32_train"): (FLASH, FLASH, SDPA, SDPA),
    (F16, "all"): (A16, T16, A16, T16),
    (F32, "none"): (SDPA, SDPA, SDPA, SDPA), (F32, "hand"): (SDPA, SDPA, SDPA, SDPA),
    (F32, "f16"): (SDPA, SDPA, SDPA, SDPA), (F32, "f16_train"): (SDPA, SDPA, SDPA, SDPA),
    (F32, "f32"): (A32, SDPA, A32, SDPA), (F32, "f32_train"): (A32, T32, A32, T32),
    (F32, "all"): (A32, T32, A32, T32),
}
# the one-query form has no hand-written bf16 branch
LAST = {**FULL, (BF16, "hand"): (FLASH, FLASH, SDPA, SDPA), (BF16, "all"): (FLASH, FLASH, SDPA, SDPA)}


class HipLike(torch.Tensor):
    """A CPU tensor that says it is on a HIP device: the branches read `is_cuda`, the stubs never touch the data."""
    is_cuda = property(lambda self: True)


@pytest.fixture
def calls(monkeypatch):
    from rankpo_amd import encoder as PE, ops
    log = []

    def rows(q):
        return q.reshape(q.shape[0], -1)

    def fwd(name):
        def f(q, k, v, cu_q, cu_k, tiles, scale, want_lse=False):
            log.append((name, tiles, None))
            return rows(q), None
        return f

    def train(name):
        def f(q, k, v, cu_q, cu_k, tiles, k_tiles, scale):
            log.append((name, tiles, k_tiles))
            return rows(q)
        return f

    def hand(q, *a, **kw):
        log.append((HAND, None, None))
        return q

    def flash(q, *a, **kw):
        log.append((FLASH, None, None))
        return (q,)

    def sdpa(q, *a, **kw):
        if not log or log[-1][0] != SDPA:                     # one call per sequence: counted once
            log.append((SDPA, None, None))
        return q
    monkeypatch.setattr(ops, A16, fwd(A16))
    monkeypatch.setattr(ops, A32, fwd(A32))
    monkeypatch.setattr(ops, T16, train(T16))
    monkeypatch.setattr(ops, T32, train(T32))
    monkeypatch.setattr(ops, "flash_attn_varlen", hand)
    # the layout rule of the real predicates holds for the tensors of this test; their dtype rule stays
    monkeypatch.setattr(ops, "causal_attn_f16_ok", lambda q, k, v: q.dtype == F16)
    monkeypatch.setattr(ops, "causal_attn_f32_ok", lambda q, k, v: q.dtype == F32)
    monkeypatch.setattr(torch.ops.aten, "_flash_attention_forward", flash)
    monkeypatch.setattr(PE.F, "scaled_dot_product_attention", sdpa)
    return log


@pytest.mark.parametrize("form", ["full", "last"])
def test_every_dtype_grad_mode_and_list_set_calls_what_it_called(calls, form):
    from rankpo_amd import encoder as PE
    lens = [3, 5]
    for (dtype, lists), want in (FULL if form == "full" else LAST).items():
        for col, (hip, grad) in enumerate(((True, False), (True, True), (False, False), (False, True))):
            ctx = PE.VarlenCtx(torch.tensor([0, 3, 8], dtype=torch.int32), lens, 5)
            for name in LISTS[lists]:
                setattr(ctx, name, name)
            kv = torch.zeros(sum(lens), 1, 64, dtype=dtype)
            q = torch.zeros(sum(lens) if form == "full" else len(lens), 2, 64, dtype=dtype)
            if hip:
                q, kv = q.as_subclass(HipLike), kv.as_subclass(HipLike)
            del calls[:]
            with torch.set_grad_enabled(grad):
                out = (PE._varlen_causal_attention if form == "full" else PE._varlen_last_query_attention)(q, kv, kv, ctx)
            case = (form, dtype, lists, "hip" if hip else "cpu", "grad" if grad else "no-grad")
            assert out.shape == q.shape, case
            assert [c[0] for c in calls] == [want[col]], (case, calls)
            if want[col] in (A16, T16, A32, T32):             # the lists of its own dtype and form, the key list under grad only
                tag, mid = want[col][12:15], "_last" if form == "last" else ""
                assert calls[0][1:] == (f"{tag}{mid}_tiles", f"{tag}{mid}_k_tiles" if want[col] in (T16, T32) else None), case


LENS = [1, 32, 33, 65]


@pytest.mark.parametrize("how", ["module switch", "model attribute"])
def test_each_switch_builds_exactly_its_lists(monkeypatch, how):
    """No-grad kinds: the two query lists; training kinds: all four; off, another dtype or another grad mode: none."""
    from rankpo_amd import encoder as PE, ops
    one = [1] * len(LENS)
    switches = {("LLAMA_F32_ATTENTION", "f32_attention"): (F32, False, "f32"),
                ("LLAMA_F32_ATTENTION_TRAIN", "f32_attention_train"): (F32, True, "f32"),
                ("LLAMA_FP16_NATIVE", "native_fp16"): (F16, False, "f16"),
                ("LLAMA_FP16_NATIVE_TRAIN", "native_fp16_train"): (F16, True, "f16")}
    enc = _llama(PE)
    for dtype in (BF16, F16, F32):                            # everything off
        for grad in (False, True):
            with torch.set_grad_enabled(grad):
                assert PE._native_attention_lists(enc, dtype, LENS, "cpu") == {}
    for (switch, attr), (on_dtype, on_grad, tag) in switches.items():
        enc = _llama(PE)
        with monkeypatch.context() as m:
            if how == "module switch":
                m.setattr(PE, switch, True)
            else:
                setattr(enc, attr, True)
            for dtype in (BF16, F16, F32):
                for grad in (False, True):
                    with torch.set_grad_enabled(grad):
                        got = PE._native_attention_lists(enc, dtype, LENS, "cpu")
                    if (dtype, grad) != (on_dtype, on_grad):
                        assert got == {}, (switch, dtype, grad)
                        continue
                    want = {f"{tag}_tiles": ops.causal_attn_f32_tile_table(LENS, LENS, "cpu"),
                            f"{tag}_last_tiles": ops.causal_attn_f32_tile_table(one, LENS, "cpu")}
                    if grad:
                        want[f"{tag}_k_tiles"] = ops.causal_attn_f32_key_tile_table(LENS, LENS, "cpu")
                        want[f"{tag}_last_k_tiles"] = ops.causal_attn_f32_key_tile_table(one, LENS, "cpu")
                    assert sorted(got) == sorted(want), (switch, sorted(got))
                    for name in want:
                        assert got[name].dtype == torch.int32 and torch.equal(got[name], want[name]), (switch, name)
                    assert len(got[f"{tag}_tiles"]) == 7 and len(got[f"{tag}_last_tiles"]) == 4      # 1 + 1 + 2 + 3 blocks
    # a head shape the kernels refuse: nothing, whatever the switch says
    enc = _llama(PE)
    enc.f32_attention = enc.native_fp16 = True
    enc.config.head_dim = 96
    with torch.no_grad():
        assert PE._native_attention_lists(enc, F32, LENS, "cpu") == {} and PE._native_attention_lists(enc, F16, LENS, "cpu") == {}
