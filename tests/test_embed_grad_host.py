"""Host side of the sorted embedding-table gradient (`ops.embed_grad_plan`, rankpo_amd/csrc/embed_grad.hip): the plan of hand-made
id lists, the documented order of the sum against float64, and the new source's place in the library.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import embed_grad_util as EG

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CHUNK = 4       # small, so that hand-made lists reach every segment length


def ops():
    from rankpo_amd import ops as o
    return o


def _seg_list(lens, seed):
    ids = np.concatenate([np.full(n, 3 * i + 2) for i, n in enumerate(lens)])
    np.random.RandomState(seed).shuffle(ids)
    return ids


CASES = {
    "all-distinct": np.array([9, 4, 7, 0, 5, 2]),
    "all-equal": np.full(11, 6),
    "single-token": np.array([3]),
    "lengths": _seg_list([1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1], 1),
    # ids beyond 16 bits (XLM-R's vocabulary: the two-pass sort), some agreeing in their low halves, up to the largest table row
    "wide-ids": np.array([70000, 4464, 3, 65539, 3, 250001, 70000, 4464, 131075, 3, (1 << 31) - 1, 65539, 70000, 70000, 70000, 4464]),
    "default-chunk": None,        # the lengths case at ops.EMBED_GRAD_CHUNK, filled in below
}


def _case(name):
    if name == "default-chunk":
        c = ops().EMBED_GRAD_CHUNK
        return _seg_list([1, c - 1, c, c + 1, 3 * c + 1], 2), c
    return CASES[name], CHUNK


def _check_plan(ids, chunk, p):
    T = len(ids)
    for a in (p.order, p.seg_ids, p.seg_start, p.chunks, p.multi):
        assert isinstance(a, np.ndarray) and a.dtype == np.int32
    # the order is THE stable ascending sort
    assert p.order.tolist() == sorted(range(T), key=lambda t: (ids[t], t))
    # the segments partition it, one per distinct id
    assert p.seg_ids.tolist() == sorted(set(ids.tolist()))
    assert p.seg_start[0] == 0 and p.seg_start[-1] == T and (np.diff(p.seg_start) >= 1).all()
    for s, r in enumerate(p.seg_ids):
        toks = p.order[p.seg_start[s]:p.seg_start[s + 1]]
        assert (ids[toks] == r).all() and (np.diff(toks) > 0).all()
    # the chunks partition every segment into consecutive pieces from its first row, none longer than `chunk`, all but the last full
    pos, slots, multi = 0, 0, []
    by_seg = {int(r): [] for r in p.seg_ids}
    for r, start, n, slot in p.chunks.tolist():
        assert start == pos and 1 <= n <= chunk
        pos += n
        by_seg[r].append((start, n, slot))
    assert pos == T
    for s, r in enumerate(p.seg_ids.tolist()):
        ch = by_seg[r]
        assert ch[0][0] == p.seg_start[s] and sum(n for _, n, _ in ch) == p.seg_start[s + 1] - p.seg_start[s]
        assert all(n == chunk for _, n, _ in ch[:-1]) and len(ch) == -(-(p.seg_start[s + 1] - p.seg_start[s]) // chunk)
        if len(ch) == 1:
            assert ch[0][2] == -1
        else:
            assert [slot for _, _, slot in ch] == list(range(slots, slots + len(ch)))
            multi.append([r, slots, len(ch)])
            slots += len(ch)
    assert p.multi.tolist() == multi and p.n_partials == slots


@pytest.mark.parametrize("name", list(CASES))
def test_plan_of_hand_made_ids(name):
    ids, chunk = _case(name)
    _check_plan(ids, chunk, ops().embed_grad_plan(ids, chunk))
    _check_plan(ids, chunk, ops().embed_grad_plan(torch.tensor(ids), chunk))          # what `bert_pack` hands over


def test_plan_literal():
    p = ops().embed_grad_plan([5, 2, 5, 5, 2, 9, 5, 5], chunk=2)
    assert p.order.tolist() == [1, 4, 0, 2, 3, 6, 7, 5]
    assert p.seg_ids.tolist() == [2, 5, 9] and p.seg_start.tolist() == [0, 2, 7, 8]
    assert p.chunks.tolist() == [[2, 0, 2, -1], [5, 2, 2, 0], [5, 4, 2, 1], [5, 6, 1, 2], [9, 7, 1, -1]]
    assert p.multi.tolist() == [[5, 0, 3]] and p.n_partials == 3
    empty = ops().embed_grad_plan(np.zeros(0, np.int64))
    assert empty.order.shape == (0,) and empty.chunks.shape == (0, 4) and empty.multi.shape == (0, 3) and empty.n_partials == 0
    assert empty.seg_start.tolist() == [0]
    for bad in (dict(ids=[1, 2], chunk=0), dict(ids=[1, -1]), dict(ids=[1, 1 << 31])):
        with pytest.raises(ValueError):
            ops().embed_grad_plan(**bad)


def _walk_plan(x, p, table_rows, dtype, padding_idx):
    """What the two kernels do with a plan, in float32 on the CPU."""
    x32 = x.float()
    out = torch.zeros(table_rows, x32.shape[1], dtype=dtype)
    ws = torch.zeros(p.n_partials, x32.shape[1], dtype=torch.float32)
    for r, start, n, slot in p.chunks.tolist():
        if r == padding_idx:
            continue
        acc = torch.zeros(x32.shape[1])
        for t in p.order[start:start + n]:
            acc = acc + x32[int(t)]
        if slot < 0:
            out[r] = acc.to(dtype)
        else:
            ws[slot] = acc
    for r, slot0, k in p.multi.tolist():
        if r == padding_idx:
            continue
        acc = torch.zeros(x32.shape[1])
        for i in range(k):
            acc = acc + ws[slot0 + i]
        out[r] = acc.to(dtype)
    return out


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_documented_order_follows_from_the_plan_and_agrees_with_f64(dtype):
    o = ops()
    chunk, rows, pad, d = o.EMBED_GRAD_CHUNK, 14, 4, 24
    ids = EG.segment_ids(chunk, rows, pad)
    x = EG.normal_values(len(ids), d, dtype, seed=5)
    emu = EG.emulate(x, ids, rows, chunk, dtype, pad)
    assert torch.equal(emu, _walk_plan(x, o.embed_grad_plan(ids), rows, dtype, pad))
    ref, mag, n = EG.reference64(x, ids, rows, pad)
    assert sorted(n[n > 0].tolist()) == [1, chunk - 1, chunk, chunk + 1, 3 * chunk + 1]
    assert float(emu[pad].abs().max()) == 0.0 and float(emu[n == 0].abs().max()) == 0.0
    err = (emu.double() - ref).abs()
    bound = EG.parity_bound(ref, mag, n, dtype)
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert float(err.max()) > 0.0                                            # the rounding is there: the bound is not vacuous


def test_ulp_of_the_storage_types():
    r = torch.tensor([0.0, 1.0, 1.5, 2.0, -3.0, 2.0 ** -14, 2.0 ** -20, 1000.0], dtype=torch.float64)
    assert EG.ulp(r, torch.float16).tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -9, 2.0 ** -24, 2.0 ** -24, 0.5]
    assert EG.ulp(r, torch.bfloat16)[1:5].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6]


def test_new_entries_are_declared_and_bound():
    from rankpo_amd import _lib, encoder
    hdr = open(os.path.join(ROOT, "include", "rankpo_hip.h")).read()
    for name in ("rpo_embed_grad_sorted", "rpo_embed_grad_workspace_elems"):
        assert name in _lib.SIGNATURES and name + "(" in hdr
    lib = _lib.load()
    assert lib.rpo_embed_grad_workspace_elems(7, 1024) == 7 * 1024 and lib.rpo_embed_grad_workspace_elems(0, 1024) == 0
    assert encoder.BERT_DETERMINISTIC_EMBED_GRAD is False                     # opt-in
    # argument checks need no device: they come before any launch
    c = lambda **kw: lib.rpo_embed_grad_sorted(*[kw.get(k, v) for k, v in (
        ("ds", 4096), ("ldds", 64), ("T", 4), ("d", 64), ("dtype", _lib.RPO_DT_F16), ("order", 4096), ("chunks", 4096), ("nc", 1),
        ("multi", None), ("nm", 0), ("np", 0), ("out", 8192), ("ldout", 64), ("rows", 10), ("pad", -1), ("ws", None), ("wse", 0),
        ("stream", None))])
    assert c(dtype=_lib.RPO_DT_F32) == -2 and c(d=60, ldds=64) == -2 and c(ds=4098) == -2 and c(ldout=68) == -2
    assert c(ds=None) == -1 and c(pad=10) == -1 and c(nm=1, multi=4096) == -1
    assert c(nm=1, multi=4096, np=2, ws=4096, wse=127) == -3


def test_embed_grad_kernels_have_no_transcendental_hazard(tmp_path):
    """The ISA scan of tests/test_bert_packing.py, for embed_grad.hip (`make isa-embed`)."""
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "rankpo_amd", "csrc"), "isa-embed", f"ISA_DIR={tmp_path}"],
                   check=True, capture_output=True, text=True)
    files = sorted(str(p) for p in tmp_path.glob("*.s"))
    assert [os.path.basename(f) for f in files] == ["embed_grad.s"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_trans_hazard.py")] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
