"""CPU side of the BERT kernel parity tests (tests/bert_parity_util.py, tests/test_gpu_bert_parity.py):
  - the case tables reach every template instance of rankpo_amd/csrc/bert_ops.hip's row and attention kernels, a GELU shape beyond
    one grid pass and the three LayerNorm-backward row classes (printed);
  - every input regime is what it claims, in float64;
  - every bound the GPU tests use is reachable by a correct kernel: a plain torch float32 restatement of the kernels' own formulas
    with their rounding points, evaluated on the very inputs of the GPU tests (all but the 5470 x 3072 GELU case), stays inside it.
    The control is the CPU torch op in the storage dtype.  This is a plausibility check of the rule, not of the kernels."""
import math

import pytest
import torch

import bert_parity_util as B

IDS = [B.TAG[t] for t in B.DTYPES]


# ------------------------------------------------------------------------------------------------
# the tables reach every instance
# ------------------------------------------------------------------------------------------------
def test_mirrors_of_the_dispatch():
    assert [B.row_vectors(d) for d in (8, 512, 513, 1024, 1025, 2048, 2049, 4096, 4104)] == [1, 1, 2, 2, 4, 4, 8, 8, 0]
    assert [B.rpo_layernorm_bwd_blocks(r) for r in (0, 1, 4, 5, 4096, 4097, 10 ** 6)] == [1, 1, 1, 2, 1024, 1024, 1024]
    assert [B.gelu_grid(*s) for s in B.GELU_SHAPES] == [1, 10, 8192]
    assert B.gelu_grid(8192 * 256 // 384, 3072) == 8192 and B.gelu_passes(8192 * 256 // 384, 3072) == 1     # 5461 rows: exactly one pass


def test_row_widths_reach_every_instance_of_the_six_row_kernels():
    want = {(t, nv, lv) for t in IDS for nv in (1, 2, 4, 8) for lv in ("full", "partial")}
    print()
    for kernel, widths in B.ROW_KERNEL_WIDTHS.items():
        got = {}
        for d in widths:
            assert d % 8 == 0 and B.row_vectors(d) > 0
            for t in IDS:
                got.setdefault((t, B.row_vectors(d), B.last_vector(d)), []).append(d)
        print(f"{kernel}: " + "; ".join(f"{t} NV{nv} {lv}: d = {sorted(set(ds))}" for (t, nv, lv), ds in sorted(got.items())))
        assert set(got) == want, (kernel, sorted(want - set(got)))
    assert 8 in B.ROW_WIDTHS                                                      # the smallest row
    assert {B.row_vectors(d) for d in B.DROP_WIDTHS} == {1, 2, 4, 8}


def test_attention_tables_reach_every_instance_and_lens_class():
    inst = {(k,) + B.attn_instance(hd, p) for k in ("fwd", "bwd_dq", "bwd_dkv") for hd, _ in B.ATTN_HEADS for p in B.ATTN_PS}
    assert B.attn_instance(32, 2.0 ** -18) == (32, False) and B.attn_instance(64, 2.0 ** -16) == (64, True)      # thr = round(p 65536)
    assert inst == {(k, hd, dr) for k in ("fwd", "bwd_dq", "bwd_dkv") for hd in (32, 64) for dr in (False, True)}
    print("\n" + "; ".join(f"bidir_attn_{k}_kernel<HD {hd}, DROP {dr}>" for k, hd, dr in sorted(inst)) + " x {bf16, f16}")

    def cls(lk):
        return {1: "1", 32: "32", 33: "33", 63: "63", 64: "64", 65: "65"}.get(lk, "<32" if lk < 32 else ">65" if lk > 65 else None)
    for label, lq, lk in B.attn_shapes():
        assert len(lq) == len(lk) and min(lq) >= 1 and min(lk) >= 1
    got = {cls(lk) for lk in B.ATTN_LENS}
    print("key-length classes of ATTN_LENS:", sorted(got))
    assert got == {"1", "<32", "32", "33", "63", "64", "65", ">65"}
    # the cross case: more keys than queries, fewer, one apart across a tile boundary, one query
    assert all(a != b for a, b in zip(B.CROSS_LENS_Q, B.CROSS_LENS_K))
    assert [lq for _, lq, _ in B.attn_shapes()][1] == [1] * len(B.ATTN_LENS)


def test_layernorm_bwd_rows_and_gelu_shapes_reach_their_paths():
    classes = {r: B.layernorm_bwd_row_class(r) for r in B.LN_BWD_ROWS}
    print("\nlayernorm_bwd rows:", classes)
    assert {"fewer rows than waves", "one row per wave at the cap", "two rows for one wave"} <= set(classes.values())
    assert [classes[r] for r in (1, 2, 3)] == ["fewer rows than waves"] * 3
    assert B.layernorm_bwd_blocks(4096) == B.layernorm_bwd_blocks(4097) == B.LN_BWD_MAX_BLOCKS
    passes = {s: B.gelu_passes(*s) for s in B.GELU_SHAPES}
    print("gelu grid-stride passes:", passes)
    assert passes[B.GELU_SHAPES[-1]] == 2 and passes[B.GELU_SHAPES[0]] == 1
    rows, cols = B.GELU_SHAPES[-1]
    assert B.gelu_passes(rows - 10, cols) == 1                 # the smallest workload-shaped row count beyond one pass, nearly


# ------------------------------------------------------------------------------------------------
# every regime is what it claims
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_layernorm_regimes_are_what_they_claim(dtype):
    for d in B.ROW_WIDTHS:
        for regime in B.LN_REGIMES:
            c = B.ln_case(regime, B.LN_ROWS, d, dtype)
            assert torch.equal(c["s"], (c["a"].double() + c["b"].double()).to(dtype))
            for x in (c["x"].double(), c["s"].double()):       # the b = None form and the a + b form
                assert torch.isfinite(x).all()
                mu, var = x.mean(-1), x.var(-1, unbiased=False)
                if regime == "offset":
                    assert (mu.abs() / var.sqrt() >= 32).all(), (d, mu.abs() / var.sqrt())
                    assert (mu > 0).any() and (mu < 0).any()
                elif regime == "outlier":
                    top2 = ((x - mu[:, None]) ** 2).topk(2, dim=-1)
                    assert (top2.values.sum(-1) / (var * d) >= 0.9).all(), (d, top2.values.sum(-1) / (var * d))
                    assert len({tuple(r) for r in top2.indices.sort(-1).values.tolist()}) == B.LN_ROWS       # other columns per row
                elif regime == "tiny_var":
                    q = B.ulp_at(torch.tensor(B.TINY_CENTRES, dtype=torch.float64)[torch.arange(B.LN_ROWS) % 5], dtype)
                    assert ((x - x.median(-1, keepdim=True).values).abs().amax(-1) <= 2 * q).all() and (var > 0).all()
                elif regime == "const":
                    assert (x == x[:, :1]).all() and set(x[:, 0].tolist()) <= set(B.CONST_VALUES)
                    s32 = x.float().sum(-1)                       # the f32 row sum is exact, in any order: so is the mean
                    assert torch.equal(s32.double(), x[:, 0] * d) and torch.equal((s32 / d).double(), x[:, 0])
            if regime in B.LN_DEGENERATE:
                assert torch.equal(c["s"], c["x"])
            e = B.embed_case(regime, d, dtype)
            for wt in (True, False):
                s = B.embed_sum(e, wt, dtype)
                if regime in B.LN_DEGENERATE:
                    assert torch.equal(s, B.ln_rows(regime, B.EMBED_V, d, dtype, 1)[e["ids"].long()])
            assert {0, B.EMBED_V - 1, B.EMBED_PAD} <= set(e["ids"].tolist()) and {0, B.EMBED_P - 1} <= set(e["pos"].tolist())
            assert set(e["tts"].tolist()) == {0, B.EMBED_TT - 1} and e["ids"].tolist().count(3) >= 6


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
def test_attention_regimes_are_what_they_claim(dtype, hd, nh):
    scale = 1.0 / math.sqrt(hd)
    for label, lens_q, lens_k in B.attn_shapes():
        cu_q, cu_k = [0] + torch.tensor(lens_q).cumsum(0).tolist(), [0] + torch.tensor(lens_k).cumsum(0).tolist()
        for regime in B.ATTN_REGIMES:
            q, k, v, do = B.attn_case(regime, lens_q, lens_k, nh, hd, dtype)
            assert all(torch.isfinite(t.float()).all() for t in (q, k, v, do))
            sat_rows = sat_hit = 0
            for n in range(len(lens_q)):
                a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
                s, lse, _ = B.attn_scores64(q[a:b], k[c:e], scale)
                P = torch.exp(s - lse[..., None])
                if regime == "spike":
                    assert (P.amax(-1) >= 1 - 1e-6).all(), (label, n)
                    win = torch.tensor([B.spike_winner(n, i, e - c) for i in range(b - a)])
                    assert (P.argmax(-1) == win[None]).all()
                    if e - c > 1:
                        rest = s.clone()
                        rest.scatter_(-1, win[None, :, None].expand(nh, -1, 1), float("-inf"))
                        gap = s.amax(-1) - rest.amax(-1)
                        assert (gap >= 24).all() and (gap <= 40).all(), (label, n, gap.min(), gap.max())
                elif regime == "saturated":
                    if e - c > 1:
                        sat_rows += P[..., 0].numel()
                        sat_hit += int((P.amax(-1) >= 1 - 1e-6).sum())
                elif regime == "identical_keys":
                    assert (P.amax(-1) - P.amin(-1)).max() <= 1e-12 and torch.allclose(P, torch.full_like(P, 1.0 / (e - c)), rtol=1e-12)
                elif regime == "offset":
                    common = float(q[a, 0, 0]) * float(k[c, 0, 0]) * scale
                    assert float(k[c, 0, 0]) == B.OFFSET_CK and common >= 100 and (q[a:b, :, 0] == q[a, 0, 0]).all() and (k[c:e, :, 0] == k[c, 0, 0]).all()
                    assert (s.amin(-1) >= 100 - 10).all() and (s.amax(-1) - s.amin(-1) < 10).all(), (label, n)
                    assert (lse >= 100 - 10).all()
            if regime == "saturated":
                assert sat_hit >= sat_rows / 4, (label, sat_hit, sat_rows)
            if regime == "spike" and label == "self":
                wins = {B.spike_winner(n, i, lk) for n, lk in enumerate(lens_k) for i in range(lk)}
                assert {0, 31, 32} <= wins and all(lk - 1 in {B.spike_winner(n, i, lk) for i in range(lk)} for n, lk in enumerate(lens_k))


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_gelu_inputs_are_what_they_claim(dtype):
    for rows, cols in B.GELU_SHAPES[:2]:
        u, dh = B.gelu_case(rows, cols, dtype)
        uf = u.double().view(-1)
        assert torch.isfinite(uf).all() and torch.isfinite(dh.float()).all()
        assert uf.min() == -200 and uf.max() == 200 and (uf == 40).any() and (uf == -40).any()
        zeros = u.view(-1)[uf == 0]
        assert torch.signbit(zeros).any() and (~torch.signbit(zeros)).any()                         # +0 and -0
        if dtype == torch.float16:
            sub = (dh.double().abs() > 0) & (dh.double().abs() < 2.0 ** -14)
            assert sub.any()


# ------------------------------------------------------------------------------------------------
# the bounds are reachable by a correct kernel
# ------------------------------------------------------------------------------------------------
def _bwd_eps(regime):
    return 1e-5 if regime in B.LN_DEGENERATE else 1e-12       # at 1e-12 the exact ds of a constant row overflows fp16


def _check_ln_bwd(s, gamma, beta, dy, eps, dtype, label):
    """The restated backward against the rule: ds per row, dgamma / dbeta per tensor.  -> the three err / bound ratios."""
    ds64, dg64, db64 = B.ln_bwd64(s, gamma, dy, eps)
    _, cds, cdg, cdb = B.layernorm_control(s, gamma, beta, dy, eps)
    ds, dg, db = B.ln_bwd_restate(s, gamma, dy, eps, dtype)
    err = (ds.double() - ds64).norm(dim=-1)
    bound = B.rule_bound((cds.double() - ds64).norm(dim=-1), ds64.norm(dim=-1), dtype)
    assert (err <= bound).all(), (label, "ds", err.tolist(), bound.tolist())
    ratios = [float((err / bound.clamp_min(1e-300)).max())]
    for name, got, ctrl, ref in (("dgamma", dg, cdg, dg64), ("dbeta", db, cdb, db64)):
        e, bnd = float((got.double() - ref).norm()), float(B.rule_bound((ctrl.double() - ref).norm(), ref.norm(), dtype))
        assert e <= bnd, (label, name, e, bnd)
        ratios.append(e / max(bnd, 1e-300))
    return ratios


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_layernorm_bounds_are_reachable(dtype):
    worst = {}
    for d in B.ROW_WIDTHS:
        for regime in B.LN_REGIMES:
            c = B.ln_case(regime, B.LN_ROWS, d, dtype)
            for form, s in (("x", c["x"]), ("a+b", c["s"])):
                y = B.ln_fwd_restate(s, c["gamma"], c["beta"], 1e-12, dtype)
                r = B.one_ulp_ratio(y, B.ln_fwd64(s, c["gamma"], c["beta"], 1e-12), dtype, B.LN_FLOOR)
                assert r <= 1.0, (regime, d, form, r)
                worst[f"fwd {regime}"] = max(worst.get(f"fwd {regime}", 0), round(r, 3))
                if regime == "const":
                    assert torch.equal(y, c["beta"].expand_as(y))
            rs = _check_ln_bwd(c["s"], c["gamma"], c["beta"], c["dy"], _bwd_eps(regime), dtype, (regime, d))
            worst[f"bwd {regime}"] = [max(a, round(b, 3)) for a, b in zip(worst.get(f"bwd {regime}", [0, 0, 0]), rs)]
            e = B.embed_case(regime, d, dtype)
            for wt in (True, False):
                s = B.embed_sum(e, wt, dtype)
                r = B.one_ulp_ratio(B.ln_fwd_restate(s, e["gamma"], e["beta"], 1e-12, dtype),
                                    B.ln_fwd64(s, e["gamma"], e["beta"], 1e-12), dtype, B.LN_FLOOR)
                assert r <= 1.0, ("embed", regime, d, wt, r)
    for rows in B.LN_BWD_ROWS:
        for d in [B.LN_BWD_WIDTH] + ([B.LN_BWD_WIDE] if rows in B.LN_BWD_SMALL_ROWS else []):
            c = B.ln_case("random", rows, d, dtype)
            _check_ln_bwd(c["s"], c["gamma"], c["beta"], c["dy"], 1e-12, dtype, ("rows", rows, d))
    print(f"\n{B.TAG[dtype]} restatement, max err / bound (fwd in ulps; bwd ds, dgamma, dbeta): {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
def test_gelu_bounds_are_reachable(dtype):
    for rows, cols in B.GELU_SHAPES[:2]:
        u, dh = B.gelu_case(rows, cols, dtype)
        r = B.one_ulp_ratio(B.gelu_restate(u, dtype), B.gelu64(u), dtype, B.GELU_FLOOR)
        assert r <= 1.0, (rows, cols, r)
        ref, size = B.gelu_bwd64(u, dh)
        err = (B.gelu_bwd_restate(u, dh, dtype).double() - ref).abs()
        bound = 1.5 * (B.gelu_control(u, dh).double() - ref).abs() + 2 * B.U[dtype] * size
        assert (err <= bound).all(), (rows, cols, int((err > bound).sum()), float((err - bound).max()))


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
@pytest.mark.parametrize("regime", B.ATTN_REGIMES)
def test_attention_bounds_are_reachable(dtype, hd, nh, regime):
    scale = 1.0 / math.sqrt(hd)
    worst = {}
    for label, lens_q, lens_k in B.attn_shapes():
        cu_q, cu_k = [0] + torch.tensor(lens_q).cumsum(0).tolist(), [0] + torch.tensor(lens_k).cumsum(0).tolist()
        q, k, v, do = B.attn_case(regime, lens_q, lens_k, nh, hd, dtype)
        for p in B.ATTN_PS:
            for n in range(len(lens_q)):
                a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
                keep = B.attn_keep_host(B.ATTN_SEED, a, c, b - a, e - c, nh, p) if p > 0 else None
                don = do[a:b].view(-1, nh, hd)
                ref, absn, absd = B.attn64(q[a:b], k[c:e], v[c:e], don, scale, keep, p)
                ctrl = B.attn_control(q[a:b], k[c:e], v[c:e], don, scale, keep, p)
                got, lse = B.attn_restate(q[a:b], k[c:e], v[c:e], don, scale, dtype, keep, p)
                bounds = B.attn_bounds(dtype, regime, e - c, p, ref, ctrl, absn, absd)
                for name, g, r, bnd in zip(("out", "dq", "dk", "dv"), got, ref, bounds):
                    if regime == "identical_keys" and p == 0 and name == "dq":
                        continue                                 # test_identical_keys_dq_reference_cancels_exactly
                    err = B.block_norm(g.double() - r)
                    key = f"{name} p{p:g}"        # the two use different controls: reported apart
                    worst[key] = max(worst.get(key, 0.0), round(float((err / bnd.clamp_min(1e-300)).max()), 3))
                    assert (err <= bnd).all(), (label, regime, "p", p, "seq", n, "lens", b - a, e - c, name, err.tolist(), bnd.tolist())
                _, lse64, s_abs = B.attn_scores64(q[a:b], k[c:e], scale)
                r = (lse.double() - lse64).abs() / B.lse_bound(s_abs, lse64, e - c, hd)
                worst["lse"] = max(worst.get("lse", 0.0), round(float(r.max()), 3))
                assert (r <= 1).all(), (label, regime, n, float(r.max()))
    print(f"\n{regime} hd{hd} {B.TAG[dtype]} restatement: max err / bound {worst}")


@pytest.mark.parametrize("dtype", B.DTYPES, ids=IDS)
@pytest.mark.parametrize("hd,nh", B.ATTN_HEADS)
def test_identical_keys_dq_reference_cancels_exactly(dtype, hd, nh):
    """The one bound of the GPU tests that this file cannot show to be reachable with the CPU control.  With every key row equal to
    k0, dq = scale k0 sum_k dS_k and sum_k dS_k = 0 exactly: the float64 reference is its own rounding noise (asserted: below
    1e-12 of ||abs||), a correct kernel returns the rounding noise of its 16-bit dS times k0 (asserted: within 2 U ||abs||, what a
    one-key sequence is allowed), and the rule gives dq no extra term in this regime, so err <= 1.5 x the control's error compares
    one noise with another.  The GPU control (a fused SDPA that rounds dS to 16 bits as the kernel does) makes nearly the same
    errors as the kernel, and the GPU test asserts the rule as it stands; the CPU SDPA keeps dS in f32 and is no stand-in for it:
    the restatement misses its bound by the factors printed here (up to ~ 20 on the one-query blocks)."""
    scale = 1.0 / math.sqrt(hd)
    worst = 0.0
    for label, lens_q, lens_k in B.attn_shapes():
        cu_q, cu_k = [0] + torch.tensor(lens_q).cumsum(0).tolist(), [0] + torch.tensor(lens_k).cumsum(0).tolist()
        q, k, v, do = B.attn_case("identical_keys", lens_q, lens_k, nh, hd, dtype)
        for n in range(len(lens_q)):
            a, b, c, e = cu_q[n], cu_q[n + 1], cu_k[n], cu_k[n + 1]
            don = do[a:b].view(-1, nh, hd)
            ref, absn, absd = B.attn64(q[a:b], k[c:e], v[c:e], don, scale, None, 0.0)
            ctrl = B.attn_control(q[a:b], k[c:e], v[c:e], don, scale, None, 0.0)
            got, _ = B.attn_restate(q[a:b], k[c:e], v[c:e], don, scale, dtype, None, 0.0)
            size = B.block_norm(absn[0])
            assert (B.block_norm(ref[1]) <= 1e-12 * size).all(), (label, n)
            err = B.block_norm(got[1].double() - ref[1])
            assert (err <= 2 * B.U[dtype] * size).all(), (label, n, err.tolist(), size.tolist())
            bnd = B.attn_bounds(dtype, "identical_keys", e - c, 0.0, ref, ctrl, absn, absd)[1]
            worst = max(worst, float((err / bnd.clamp_min(1e-300)).max()))
    print(f"\nidentical_keys dq hd{hd} {B.TAG[dtype]} restatement: max err / (bound with the CPU control) {worst:.2f}")
