"""CPU side of the tests of the sorted embedding-table gradient (`ops.embed_grad_sorted`, rankpo_amd/csrc/embed_grad.hip): the
documented order of the sum restated in float32 from the ids alone (not from the plan the kernel walks), the float64 reference, the
error bounds and the id lists.  Importing it needs no GPU."""
import numpy as np
import torch

U32 = 2.0 ** -24                     # unit roundoff of float32
MANT = {torch.float16: 10, torch.bfloat16: 7}
EMIN = {torch.float16: -14, torch.bfloat16: -126}


def emulate(x, ids, table_rows, chunk, dtype, padding_idx=None):
    """x [T, d] (CPU, any float dtype) -> [table_rows, d] of `dtype`, in the documented order: per distinct id its rows in ascending
    token order, cut into chunks of `chunk` from the first; a chunk is summed one row after the other in float32 onto 0; one chunk:
    rounded once; several: the chunk sums added one after the other in chunk order onto 0, rounded once."""
    x32 = x.detach().cpu().float()
    ids = np.asarray(ids).reshape(-1)
    out = torch.zeros(table_rows, x32.shape[1], dtype=dtype)
    for r in np.unique(ids):
        if padding_idx is not None and r == padding_idx:
            continue
        toks = np.flatnonzero(ids == r)
        parts = []
        for c0 in range(0, len(toks), chunk):
            acc = torch.zeros(x32.shape[1], dtype=torch.float32)
            for t in toks[c0:c0 + chunk]:
                acc = acc + x32[int(t)]
            parts.append(acc)
        total = parts[0]
        if len(parts) > 1:
            total = torch.zeros(x32.shape[1], dtype=torch.float32)
            for p in parts:
                total = total + p
        out[int(r)] = total.to(dtype)
    return out


def reference64(x, ids, table_rows, padding_idx=None):
    """(float64 segment sums [table_rows, d], sum of |x_i| per element, segment length per row)."""
    x64 = x.detach().cpu().double()
    idx = torch.as_tensor(np.asarray(ids).reshape(-1), dtype=torch.int64)
    ref = torch.zeros(table_rows, x64.shape[1], dtype=torch.float64).index_add_(0, idx, x64)
    mag = torch.zeros_like(ref).index_add_(0, idx, x64.abs())
    n = torch.zeros(table_rows, dtype=torch.float64).index_add_(0, idx, torch.ones(idx.shape[0], dtype=torch.float64))
    if padding_idx is not None:
        ref[padding_idx], mag[padding_idx], n[padding_idx] = 0.0, 0.0, 0.0
    return ref, mag, n


def ulp(ref, dtype):
    """Spacing of `dtype` at |ref| (float64 tensor): 2^(max(floor(log2 |ref|), emin) - mantissa bits)."""
    _, e = np.frexp(ref.abs().numpy())                        # |ref| = m 2^e, 0.5 <= m < 1; frexp(0) = (0, 0)
    e = np.where(ref.numpy() == 0, EMIN[dtype], e - 1)
    return torch.from_numpy(np.ldexp(1.0, np.maximum(e, EMIN[dtype]) - MANT[dtype]))


def parity_bound(ref, mag, n, dtype):
    """|got - ref| <= 0.5 ulp(ref) + n 2^-24 sum |x_i|: n - 1 float32 adds in any order (each at most 2^-24 of a partial sum that
    sum |x_i| bounds), then one rounding to storage."""
    return 0.5 * ulp(ref, dtype) + n[:, None] * U32 * mag


def agreement_bound(ref, mag, n, dtype):
    """Two float32 sums of the same terms in different orders, each rounded once to storage."""
    return ulp(ref, dtype) + 2 * n[:, None] * U32 * mag


def segment_ids(chunk, table_rows, padding_idx, seed=0):
    """Ids whose segment lengths are 1, chunk - 1, chunk, chunk + 1 and 3 chunk + 1, plus 5 hits of `padding_idx`, shuffled;
    the table rows in between stay untouched."""
    lens = [1, max(chunk - 1, 1), chunk, chunk + 1, 3 * chunk + 1]
    rows = [r for r in range(table_rows) if r != padding_idx][1::2][:len(lens)]
    assert len(rows) == len(lens)
    ids = np.concatenate([np.full(n, r) for r, n in zip(rows, lens)] + [np.full(5, padding_idx)])
    np.random.RandomState(seed).shuffle(ids)
    return ids.astype(np.int64)


def normal_values(T, d, dtype, seed=0):
    """Storage-dtype values of both signs with magnitudes in [0.25, 4): no tiny numbers, nothing near a denormal."""
    g = torch.Generator().manual_seed(seed)
    mag = 0.25 + 3.75 * torch.rand(T, d, generator=g)
    sign = torch.where(torch.rand(T, d, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign).to(dtype)
