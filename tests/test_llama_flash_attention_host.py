"""Host side of how a packed Llama block reaches the hand-written bf16 flash attention: which op `LlamaAttention.forward` calls, and
with which lists and switches, for every storage dtype, head_dim, grad mode, `FOLD_ROPE` arm and set of work lists; and which
one-query attention `LlamaLayer.forward_last_rows` calls.  The ops are stubs with the real signatures that record their names and
arguments.  No GPU."""
import math

import pytest
import torch

from test_llama_native_attention_host import HipLike

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
ROPE_QKV, ROPE_QKV_FWD, QKV, CAUSAL = ("rope_flash_attn_varlen_qkv", "rope_flash_attn_varlen_qkv_fwd", "flash_attn_varlen_qkv",
                                       "_varlen_causal_attention")
LASTQ, VARLEN_LASTQ = "last_query_attn", "_varlen_last_query_attention"
# which lists the VarlenCtx holds (each its own name, so that a stub can tell which one it was handed)
LISTS = {"none": (), "tiles": ("tiles",), "tiles+k": ("tiles", "k_tiles"), "tiles+k+fwd": ("tiles", "k_tiles", "fwd_tiles")}
# bf16 at head_dim 64 / 128: (lists, grad mode, FOLD_ROPE) -> the attention op; written out from the branches of
# `LlamaAttention.forward` as they stood with the predicate spelled three times.  The key list alone selects the autograd node,
# whatever the grad mode; the forward-only entry needs no-grad and a folded rotary.
HAND = {
    ("none", False, 0): CAUSAL, ("none", False, 1): CAUSAL, ("none", False, 2): CAUSAL,
    ("none", True, 0): CAUSAL, ("none", True, 1): CAUSAL, ("none", True, 2): CAUSAL,
    ("tiles", False, 0): CAUSAL, ("tiles", False, 1): ROPE_QKV_FWD, ("tiles", False, 2): ROPE_QKV_FWD,
    ("tiles", True, 0): CAUSAL, ("tiles", True, 1): CAUSAL, ("tiles", True, 2): CAUSAL,
    ("tiles+k", False, 0): QKV, ("tiles+k", False, 1): ROPE_QKV, ("tiles+k", False, 2): ROPE_QKV,
    ("tiles+k", True, 0): QKV, ("tiles+k", True, 1): ROPE_QKV, ("tiles+k", True, 2): ROPE_QKV,
    ("tiles+k+fwd", False, 0): QKV, ("tiles+k+fwd", False, 1): ROPE_QKV, ("tiles+k+fwd", False, 2): ROPE_QKV,
    ("tiles+k+fwd", True, 0): QKV, ("tiles+k+fwd", True, 1): ROPE_QKV, ("tiles+k+fwd", True, 2): ROPE_QKV,
}
NH, NKV, LENS = 4, 1, [3, 5]
L = sum(LENS)


def _cfg(PE, hd, nh=NH):
    return PE.llama_config(vocab_size=64, hidden_size=64, intermediate_size=64, num_hidden_layers=1, num_attention_heads=nh,
                           num_key_value_heads=NKV, head_dim=hd, pad_token_id=0)


def _ctx(PE, lists):
    ctx = PE.VarlenCtx(torch.tensor([0, 3, 8], dtype=torch.int32), LENS, max(LENS))
    for name in LISTS[lists]:
        setattr(ctx, name, name)
    return ctx


@pytest.fixture
def calls(monkeypatch):
    from rankpo_amd import encoder as PE, ops
    log = []

    def heads(qkv, nh, hd):
        return torch.zeros(qkv.numel() // qkv.shape[-1], nh, hd, dtype=qkv.dtype)

    def rope_qkv(qkv, cos, sin, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block=None, head_dim=64, fold_forward=True,
                 fwd_tiles=None):
        log.append((ROPE_QKV, dict(shape=tuple(qkv.shape), nh=num_heads, nkv=num_kv_heads, cu=cu, tiles=tiles, k_tiles=k_tiles,
                                   scale=scale, key_block=key_block, head_dim=head_dim, fold_forward=fold_forward,
                                   fwd_tiles=fwd_tiles)))
        return heads(qkv, num_heads, head_dim)

    def rope_qkv_fwd(qkv, cos, sin, num_heads, num_kv_heads, cu, tiles, scale, head_dim=64, fwd_tiles=None):
        log.append((ROPE_QKV_FWD, dict(shape=tuple(qkv.shape), nh=num_heads, nkv=num_kv_heads, cu=cu, tiles=tiles, scale=scale,
                                       head_dim=head_dim, fwd_tiles=fwd_tiles)))
        return heads(qkv, num_heads, head_dim)

    def qkv_node(qkv, num_heads, num_kv_heads, cu, tiles, k_tiles, scale, key_block=None, head_dim=64, fwd_tiles=None):
        log.append((QKV, dict(shape=tuple(qkv.shape), nh=num_heads, nkv=num_kv_heads, cu=cu, tiles=tiles, k_tiles=k_tiles, scale=scale,
                              key_block=key_block, head_dim=head_dim, fwd_tiles=fwd_tiles)))
        return heads(qkv, num_heads, head_dim)

    def rope_(x, cos, sin, heads, head_dim, grad_inplace=False):
        log.append(("rope_", dict(shape=tuple(x.shape), heads=heads, head_dim=head_dim, grad_inplace=grad_inplace)))
        return x

    def causal(q, k, v, ctx):
        log.append((CAUSAL, dict(q=tuple(q.shape), k=tuple(k.shape), v=tuple(v.shape), ctx=ctx)))
        return torch.zeros(q.shape, dtype=q.dtype)

    def lastq(q, kv, cu, num_kv_heads, head_dim, scale):
        log.append((LASTQ, dict(q=tuple(q.shape), kv=tuple(kv.shape), cu=cu, nkv=num_kv_heads, head_dim=head_dim, scale=scale)))
        return torch.zeros(q.shape, dtype=q.dtype)

    def varlen_lastq(q, k, v, ctx):
        log.append((VARLEN_LASTQ, dict(q=tuple(q.shape), k=tuple(k.shape), v=tuple(v.shape), ctx=ctx)))
        return torch.zeros(q.shape, dtype=q.dtype)

    monkeypatch.setattr(ops, ROPE_QKV, rope_qkv)
    monkeypatch.setattr(ops, ROPE_QKV_FWD, rope_qkv_fwd)
    monkeypatch.setattr(ops, QKV, qkv_node)
    monkeypatch.setattr(ops, "rope_", rope_)
    monkeypatch.setattr(ops, LASTQ, lastq)
    monkeypatch.setattr(ops, "fused_norm_ok", lambda x: False)
    monkeypatch.setattr(PE, CAUSAL, causal)
    monkeypatch.setattr(PE, VARLEN_LASTQ, varlen_lastq)
    monkeypatch.setattr(PE.LlamaMLP, "forward", lambda self, x, last_in_block=False: torch.zeros(x.shape, dtype=x.dtype))
    return log


@pytest.mark.parametrize("hd", [64, 128, 96])
@pytest.mark.parametrize("dtype", [BF16, F16, F32])
def test_attention_forward_calls_what_it_called(calls, monkeypatch, dtype, hd):
    from rankpo_amd import encoder as PE
    torch.manual_seed(0)
    att = PE.LlamaAttention(_cfg(PE, hd)).to(dtype)
    rope = PE.RopeTables(torch.zeros(L, hd // 2))
    W, scale = (NH + 2 * NKV) * hd, 1.0 / math.sqrt(hd)
    fused = dtype in (BF16, F32)               # ops.fused_encoder_ops_ok: an fp16 tensor only inside the native fp16 pass
    rope_call = ("rope_", dict(shape=(1, L, W), heads=NH + NKV, head_dim=hd, grad_inplace=True))
    for (lists, grad, fold), hand in HAND.items():
        monkeypatch.setattr(PE, "FOLD_ROPE", fold)
        ctx = _ctx(PE, lists)
        fwd_tiles = "fwd_tiles" if lists == "tiles+k+fwd" else None
        x = torch.zeros(1, L, 64, dtype=dtype).as_subclass(HipLike)
        del calls[:]
        with torch.set_grad_enabled(grad):
            out = att(x, rope, ctx)
        case = (dtype, hd, lists, "grad" if grad else "no-grad", fold)
        assert out.shape == (1, L, 64) and out.dtype == dtype, case
        op = hand if dtype == BF16 and hd in (64, 128) else CAUSAL
        if op == ROPE_QKV:
            want = [(ROPE_QKV, dict(shape=(1, L, W), nh=NH, nkv=NKV, cu=ctx.cu, tiles="tiles", k_tiles="k_tiles", scale=scale,
                                    key_block=None, head_dim=hd, fold_forward=fold >= 2, fwd_tiles=fwd_tiles))]
        elif op == ROPE_QKV_FWD:
            want = [(ROPE_QKV_FWD, dict(shape=(1, L, W), nh=NH, nkv=NKV, cu=ctx.cu, tiles="tiles", scale=scale, head_dim=hd,
                                        fwd_tiles=fwd_tiles))]
        elif op == QKV:
            want = [rope_call, (QKV, dict(shape=(L, W), nh=NH, nkv=NKV, cu=ctx.cu, tiles="tiles", k_tiles="k_tiles", scale=scale,
                                          key_block=None, head_dim=hd, fwd_tiles=fwd_tiles))]
        else:
            want = [rope_call] * fused + [(CAUSAL, dict(q=(L, NH, hd), k=(L, NKV, hd), v=(L, NKV, hd), ctx=ctx))]
        assert [c[0] for c in calls] == [w[0] for w in want], (case, [c[0] for c in calls])
        for (name, got), (_, exp) in zip(calls, want):
            assert sorted(got) == sorted(exp), (case, name)
            for key in exp:
                assert got[key] is exp[key] or got[key] == exp[key], (case, name, key, got[key])


def test_attention_forward_on_padded_batches_calls_no_packed_op(calls):
    """Not a VarlenCtx (a mask, or None): the SDPA branch, whatever the lists would have said."""
    from rankpo_amd import encoder as PE
    att = PE.LlamaAttention(_cfg(PE, 64)).to(BF16)
    rope = PE.RopeTables(torch.zeros(L, 32))
    x = torch.zeros(2, L, 64, dtype=BF16).as_subclass(HipLike)
    with torch.no_grad():
        out = att(x, rope, None)
    assert out.shape == (2, L, 64) and [c[0] for c in calls] == ["rope_"]


# (dtype, head_dim, q heads, ctx.tiles set) -> the one-query attention of the last block: the hand-written one needs ctx.tiles
# (hand_attention is on) and `ops.last_query_attn_ok` (HIP bf16, head_dim 64 / 128, 1 / 2 / 4 q heads per kv head)
LAST_ROWS = {
    (BF16, 64, 4, True): LASTQ, (BF16, 128, 4, True): LASTQ, (BF16, 64, 2, True): LASTQ,
    (BF16, 64, 4, False): VARLEN_LASTQ, (BF16, 128, 4, False): VARLEN_LASTQ,
    (BF16, 96, 4, True): VARLEN_LASTQ, (BF16, 64, 8, True): VARLEN_LASTQ,
    (F32, 64, 4, True): VARLEN_LASTQ, (F32, 64, 4, False): VARLEN_LASTQ,
    (F16, 64, 4, True): VARLEN_LASTQ, (F16, 64, 4, False): VARLEN_LASTQ,
}


@pytest.mark.parametrize("grad", [False, True])
def test_forward_last_rows_calls_what_it_called(calls, grad):
    from rankpo_amd import encoder as PE
    torch.manual_seed(0)
    N = len(LENS)
    last_idx = torch.tensor([2, 7])
    for (dtype, hd, nh, tiles), op in LAST_ROWS.items():
        layer = PE.LlamaLayer(_cfg(PE, hd, nh)).to(dtype)
        rope = PE.RopeTables(torch.zeros(L, hd // 2))
        ctx = _ctx(PE, "tiles" if tiles else "none")
        x = torch.zeros(1, L, 64, dtype=dtype).as_subclass(HipLike)
        del calls[:]
        with torch.set_grad_enabled(grad):
            out = layer.forward_last_rows(x, None, rope, ctx, last_idx)
        case = (dtype, hd, nh, tiles, grad)
        assert out.shape == (N, 64) and out.dtype == dtype, case
        ropes = [("rope_", dict(shape=(N, nh * hd), heads=nh, head_dim=hd, grad_inplace=False)),
                 ("rope_", dict(shape=(1, L, 2 * NKV * hd), heads=NKV, head_dim=hd, grad_inplace=True))] * (dtype != F16)
        if op == LASTQ:
            want = ropes + [(LASTQ, dict(q=(N, nh, hd), kv=(1, L, 2 * NKV * hd), cu=ctx.cu, nkv=NKV, head_dim=hd,
                                         scale=1.0 / math.sqrt(hd)))]
        else:
            want = ropes + [(VARLEN_LASTQ, dict(q=(N, nh, hd), k=(L, NKV, hd), v=(L, NKV, hd), ctx=ctx))]
        assert [c[0] for c in calls] == [w[0] for w in want], (case, [c[0] for c in calls])
        for (name, got), (_, exp) in zip(calls, want):
            assert sorted(got) == sorted(exp), (case, name)
            for key in exp:
                assert got[key] is exp[key] or got[key] == exp[key], (case, name, key, got[key])
