"""CPU side of the pooling parity tests (tests/pool_parity_util.py, tests/test_gpu_pool_parity.py):
  - the case tables reach every template instance and path of rankpo_amd/csrc/pool_normalize.hip (12 wave instances, 9 block
    (dtype x row path) instances, both argmin paths in both forward kernels, both fills of the backward) and every dispatch edge
    from both sides, shown through the mirrors of the dispatch (printed);
  - the tables hold the widths, lengths, mask rows, sample counts, strides and modes the suite promises;
  - every regime is what it claims, in float64; the 64-bit mask rows are decided where a narrower compare goes wrong;
  - every rule the GPU tests use is reachable by a correct kernel: a plain torch float32 restatement of the kernels' formulas with
    their rounding points, on the very inputs of every GPU case, passes `check_fwd` / `check_bwd` with the CPU torch op as the
    control.  This keeps the rules honest; it says nothing about the kernels.
  - no dtype skips a regime: fp16 has its own table entry where it cannot express one."""
import numpy as np
import pytest
import torch

import pool_parity_util as P

IDS = [P.TAG[t] for t in P.DTYPES]


def _cases(table, dtype):
    return [c for c in table if c["dtype"] == dtype]


# ------------------------------------------------------------------------------------------------
# the mirrors and what the tables reach
# ------------------------------------------------------------------------------------------------
def test_mirrors_of_the_dispatch():
    bf, f32 = torch.bfloat16, torch.float32

    def k(d, N=512, L=8, sn=None, sl=None, mode=P.POOL_LAST, **offs):
        return P.fwd_kernel(bf, N, L, d, d if sn is None else sn, d if sl is None else sl, mode, **offs)

    assert [k(d) for d in (8, 512, 520, 1024, 1032, 2048, 2056, 4096, 4104)] == \
        ["wave/NV1", "wave/NV1", "wave/NV2", "wave/NV2", "wave/NV4", "wave/NV4", "wave/NV8", "wave/NV8", "block"]
    assert P.fwd_kernel(f32, 512, 8, 2048, 2048, 2048, 0) == "wave/NV8" and P.fwd_kernel(f32, 512, 8, 2052, 2052, 2052, 0) == "block"
    assert k(512, N=511) == "block" and k(512, L=1024) == "wave/NV1" and k(512, L=1025) == "block"
    assert k(512, sn=516) == "block" and k(512, sl=516) == "block" and k(512, mode=1) == "block" and k(12) == "block"
    assert k(512, h_off=4) == "block" and k(512, out_off=1) == "block"
    assert [P.block_row_path(bf, d, 0, 0) for d in (8, 2048, 2056, 12)] == ["block/onevec", "block/onevec", "block/vecloop", "block/scalar"]
    assert P.block_row_path(bf, 512, 4, 0) == "block/scalar" and P.block_row_path(f32, 1024, 0, 0) == "block/onevec"
    assert P.block_row_path(f32, 1028, 0, 0) == "block/vecloop"
    assert [P.argmin_path(0, L, o) for L, o in ((8, 0), (8, 1), (7, 0), (7, 7))] == ["vec16", "scalar", "scalar", "scalar"]
    assert P.argmin_path(1, 8, 0) == "none"
    assert [P.wave_scan_rounds(L) for L in (2, 510, 512, 514, 1024)] == [1, 1, 1, 2, 2]
    assert P.bwd_fill(bf, 1024, 8, True) == ("vec", 1) and P.bwd_fill(bf, 1025, 8, True) == ("vec", 2)
    assert P.bwd_fill(bf, 241, 136, True) == ("vec", 5) and P.bwd_fill(bf, 3, 12, True) == ("scalar", 1)
    assert P.bwd_fill(bf, 5, 512, True, dh_off=1) == ("scalar", 2) and P.bwd_fill(bf, 5, 512, False) == ("none", 1)
    assert P.bwd_fill(bf, 2 ** 31, 8, True)[0] == "scalar"            # L (d / V) >= 2^31: out of scope for a test (32 GB)


@pytest.fixture(scope="module")
def survey():
    """One pass over FWD_CASES: per case the kernel, the sets of row paths, argmin paths, mask kinds and regimes."""
    out = {}
    for c in P.FWD_CASES:
        b = P.build_fwd(c)
        k, rows, arg = P.fwd_paths(c, b)
        out[c["name"]] = {"case": c, "kernel": k, "rows": set(rows), "argmin": set(arg), "kinds": set(b["kind"]),
                          "regimes": set(b["regime"]), "idx_parity": {int(i) % 2 for i in b["idx"]},
                          "fz_by_argmin": {(a, kd) for a, kd in zip(arg, b["kind"])}}
    return out


def test_forward_tables_reach_every_instance_and_path(survey):
    waves, blocks, argmins, per = set(), set(), set(), {}
    for name, s in survey.items():
        t = P.TAG[s["case"]["dtype"]]
        for r in s["rows"]:
            (waves if r.startswith("wave") else blocks).add((t, r))
            per.setdefault((t, r), []).append(name.split("-", 1)[1])
        argmins |= {(s["kernel"].split("/")[0], a) for a in s["argmin"]}
    print()
    for key in sorted(per):
        print("%s %s: %s" % (key[0], key[1], ", ".join(per[key])))
    assert waves == {(t, "wave/NV%d" % nv) for t in IDS for nv in (1, 2, 4, 8)}                       # 12 wave instances
    assert blocks == {(t, "block/" + p) for t in IDS for p in ("onevec", "vecloop", "scalar")}        # 9 block instances
    assert argmins == {(k, a) for k in ("wave", "block") for a in ("vec16", "scalar")} | {("block", "none")}
    for t in P.DTYPES:
        tag = P.TAG[t]
        # the block kernel's vector loop and fp16 at all in the block kernel; 16-bit widths above 2048 that it serves
        assert survey[tag + "-block-N5-L256-d%d" % (512 * P.VEC[t])]["rows"] == {"block/vecloop"}
        assert survey[tag + "-block-N4-L255-d%d" % (513 * P.VEC[t])]["rows"] == {"block/vecloop"}
        # one launch that mixes aligned and unaligned pooled rows, with both parities of idx
        for name in ("-block-mixed-align", "-edge-sl"):
            assert survey[tag + name]["rows"] == {"block/onevec", "block/scalar"} and survey[tag + name]["idx_parity"] == {0, 1}
        assert survey[tag + "-block-mixed-align-loop"]["rows"] == {"block/vecloop", "block/scalar"}
        assert survey[tag + "-edge-sn"]["rows"] == {"block/onevec", "block/scalar"}
        # an even L with the mask base off by 8 bytes: the scalar scan in both kernels
        for name, s in survey.items():
            if name.startswith(tag) and "maskoff" in name:
                assert s["case"]["L"] % 2 == 0 and s["argmin"] == {"scalar"}, name
        # odd L: every row scalar; even L on an aligned base: every row in 16-byte pieces
        assert survey[tag + "-wave-L255-d%d" % (128 * P.VEC[t])]["argmin"] == {"scalar"}
        assert survey[tag + "-wave-L256-d%d" % (129 * P.VEC[t])]["argmin"] == {"vec16"}


def test_every_dispatch_edge_from_both_sides(survey):
    for t in P.DTYPES:
        tag, V = P.TAG[t], P.VEC[t]
        k = lambda name: survey[tag + "-" + name]["kernel"]      # noqa: E731
        c = lambda name: survey[tag + "-" + name]["case"]        # noqa: E731
        wave_twin = P.fwd_kernel(t, 512, 8, 64 * V, 66 * V, 66 * V, P.POOL_LAST)
        assert wave_twin == "wave/NV1"                           # the shape every `edge-*` case departs from in ONE respect
        assert k("edge-N511") == "block" and c("edge-N511")["N"] == 511 and k("wave-L1-d%d" % V).startswith("wave")     # N = 512
        assert {survey[n]["case"]["N"] for n in survey if n.startswith(tag + "-wave-L")} == {512, 513, 514, 515}
        assert k("edge-L1026") == "block" and k("wave-L1024-d%d" % (33 * V)) == "wave/NV1"
        assert k("edge-vecs9") == "block" and c("edge-vecs9")["d"] == 513 * V and k("wave-L512-d%d" % (512 * V)) == "wave/NV8"
        assert k("edge-sn") == "block" and c("edge-sn")["sn"] % V != 0 and c("edge-sn")["sl"] % V == 0
        assert k("edge-sl") == "block" and c("edge-sl")["sl"] == 64 * V + V // 2
        assert k("edge-hbase") == "block" and k("edge-outbase") == "block" and k("edge-oddd") == "block" and k("edge-cls") == "block"
        for name in ("edge-sn", "edge-sl", "edge-hbase", "edge-outbase", "edge-cls"):
            assert (c(name)["N"], c(name)["L"], c(name)["d"]) == (512, 8, 64 * V)
        # the block kernel's one-vector / loop edge, from both sides
        assert survey[tag + "-block-N2-L2-d%d" % (256 * V)]["rows"] == {"block/onevec"}
        assert survey[tag + "-block-N3-L7-d%d" % (257 * V)]["rows"] == {"block/vecloop"}


def test_forward_tables_hold_what_they_promise(survey):
    for t in P.DTYPES:
        tag, V = P.TAG[t], P.VEC[t]
        mine = {n: s for n, s in survey.items() if n.startswith(tag + "-")}
        widths = {s["case"]["d"] for s in mine.values()}
        want = {V, 257 * V, 256 * V, 513 * V, P.odd_width(t, False), P.odd_width(t, True), 384, 768, 1024}
        want |= {V * 64 * nv for nv in (1, 2, 4, 8)} | {V * 32 * nv + V for nv in (1, 2, 4, 8)}
        assert want <= widths, sorted(want - widths)
        assert P.odd_width(t, True) > 256 and P.odd_width(t, True) % V and P.odd_width(t, False) % V
        for kern in ("wave", "block"):
            Ls = {s["case"]["L"] for s in mine.values() if s["kernel"].startswith(kern) and s["case"]["mode"] == P.POOL_LAST}
            assert {L for L in P.L_TABLE if kern == "block" or L <= 1024} <= Ls | ({1, 2, 7, 8, 255, 256} if kern == "block" else set()), (kern, sorted(Ls))
            kinds = set().union(*(s["kinds"] for s in mine.values() if s["kernel"].startswith(kern)))
            assert set(P.mask_kinds(1026 if kern == "block" else 1024)) <= kinds, (kern, sorted(kinds))
            # the first zero at every seam position under BOTH scans of the kernel
            seen = set().union(*(s["fz_by_argmin"] for s in mine.values() if s["kernel"].startswith(kern)))
            for p in P.FIRST_ZEROS:
                for a in ("vec16", "scalar"):
                    assert (a, "fz%d" % p) in seen, (tag, kern, a, p)
            for wide in ("wide_a", "wide_b", "wide_c"):
                for a in ("vec16", "scalar"):
                    assert (a, wide) in seen, (tag, kern, a, wide)
        assert {1, 2, 7, 8, 255, 256} <= {s["case"]["L"] for s in mine.values() if s["kernel"] == "block"}
        Ns = {s["case"]["N"] for s in mine.values()}
        assert set(P.N_EDGE) | {1, 2, 3, 4, 5, 700} <= Ns
        modes = {(s["case"]["mode"], s["case"]["normalize"]) for s in mine.values()}
        assert modes == {(0, 0), (0, 1), (1, 0), (1, 1)}
        for d in (384, 768, 1024):
            c = mine[tag + "-cls-prod-d%d" % d]["case"]
            assert (c["N"], c["L"], c["mask"], c["mode"], c["sn"], c["sl"]) == (700, 1, False, P.POOL_CLS, d, d)
        assert any(s["case"]["sn"] > s["case"]["d"] for s in mine.values()) and any(s["case"]["sn"] == s["case"]["d"] for s in mine.values())
        # every regime of the dtype in every launch of eight or more distinct rows
        for n, s in mine.items():
            if s["case"]["N"] >= 40:
                assert s["regimes"] == set(P.REGIMES[t]), n
    assert "below_eps" not in P.REGIMES[torch.float16] and len(P.REGIMES[torch.float16]) == len(P.REGIMES[torch.bfloat16])


def test_backward_tables_reach_both_fills_and_every_seam():
    print()
    for t in P.DTYPES:
        tag, V = P.TAG[t], P.VEC[t]
        cs = {c["name"].split("-", 1)[1]: c for c in _cases(P.BWD_CASES, t)}
        fill = {n: P.bwd_fill(t, c["L"], c["d"], True, c["dh_off"]) for n, c in cs.items()}
        print(tag, {n: f for n, f in fill.items() if not n.startswith("regimes")})
        chunks = {n: c["L"] * (c["d"] // V) for n, c in cs.items() if fill[n][0] == "vec"}
        assert {1023, 1024, 1025, 1028, 4097} <= set(chunks.values())
        assert fill["fill-chunks1023"] == ("vec", 1) and fill["fill-chunks1024"] == ("vec", 1) and fill["fill-chunks1025"] == ("vec", 2)
        assert fill["fill-chunks4097"] == ("vec", 5) and fill["fill-straddle"] == ("vec", 2)
        # pooled row first, last, on both sides of the 1024-chunk seam, and straddling it
        assert cs["fill-chunks1025"]["idx"] == [0, 1024, 1022, 1023]
        cpr = cs["fill-straddle"]["d"] // V
        assert 3 * cpr < 1024 < 4 * cpr and 3 in cs["fill-straddle"]["idx"]
        c = cs["fill-chunks4097"]
        assert any(i * 17 < 1024 < (i + 1) * 17 for i in c["idx"]) and any(i * 17 < 2048 < (i + 1) * 17 for i in c["idx"])
        assert [fill[n][0] for n in ("sfill-odd", "sfill-odd-wide", "sfill-dhoff")] == ["scalar"] * 3
        assert cs["sfill-odd-wide"]["d"] % V and cs["sfill-odd-wide"]["d"] > 256 and cs["sfill-dhoff"]["d"] % V == 0
        assert fill["sfill-odd-wide"][1] > 1                                   # the scalar fill over several blocks
        c = cs["grid-N65535"]
        assert (c["N"], c["L"], c["d"]) == (P.BWD_MAX_N, 1, V) and c["N"] * c["d"] * P.ESIZE[t] <= 2 ** 21
        for g in P.G_REGIMES:
            names = [n for n in cs if n.startswith("regimes-" + g)]
            assert len(names) == 3 and all(cs[n]["rows"] == "all" and cs[n]["N"] == len(P.REGIMES[t]) for n in names)
        assert {cs[n]["normalize"] for n in cs} == {0, 1}


# ------------------------------------------------------------------------------------------------
# every regime is what it claims
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_row_regimes_are_what_they_claim(dtype):
    V = P.VEC[dtype]
    for d in (V, 33 * V, P.odd_width(dtype, True), 513 * V):
        gen = torch.Generator().manual_seed(d)
        for reg in sorted(set(P.REGIMES[dtype])):
            x = P.pool_rows(reg, 6, d, dtype, gen)
            assert torch.isfinite(x.float()).all(), (reg, d)
            x64 = x.double()
            n = x64.norm(dim=-1)
            ss32 = (x.float() * x.float()).sum(-1)
            assert torch.isfinite(ss32).all(), (reg, d)
            if reg == "offset":
                assert bool((x64.mean(-1).abs() >= 16 * x64.std(-1, unbiased=False)).all()) or d == V
                assert bool((x64.mean(-1).abs() >= 60).all())
            elif reg == "outlier":
                top2 = x64.abs().topk(2, dim=-1).values
                assert bool((top2[:, 0] >= 4000 * top2[:, 1]).all()), (d, top2)
            elif reg == "large":
                if dtype == torch.float16:
                    assert bool((x64.abs().amax(-1) == 65504).all()) and bool((x64.abs().amin(-1) < 1).all())
                else:
                    assert bool((x64.abs().amax(-1) >= 2.0 ** 53).all()) and float(ss32.max()) < 2.0 ** 124
                    assert float((x.float() * x.float()).max()) * d < 3.0e38            # finite in ANY order of summation
            elif reg == "zero":
                assert bool((P.bits(x) == 0).all())
            elif reg == "below_eps":
                assert bool((n > 0).all()) and bool((n <= P.EPS / 4).all()), (d, n)
                assert bool((ss32 > 0).all())                                            # the squares do not flush to zero
            elif reg == "above_eps":
                assert bool((n >= 4 * P.EPS).all()) and bool((n < 1e-2).all()), (d, n)
    assert ("below_eps" in P.REGIMES[dtype]) == (dtype != torch.float16)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_gradient_regimes_are_what_they_claim(dtype):
    for c in _cases(P.BWD_CASES, dtype):
        b = P.build_bwd(c)
        x, g = b["x"].double(), b["g"].double()
        assert torch.isfinite(b["g"].float()).all() and torch.isfinite(b["x"].float()).all(), c["name"]
        if c["g"] == "orthogonal":
            assert bool(((x * g) == 0).all()) and float((x * g).sum()) == 0.0
            assert bool((g.abs().sum(-1) > 0).all())
        elif c["g"] == "parallel":
            for n, reg in enumerate(b["regime"]):
                if reg == "zero":
                    assert bool((g[n] == 0).all())
                    continue
                cos = float((x[n] * g[n]).sum() / (x[n].norm() * g[n].norm()))
                assert cos >= 1 - 4 * P.U[dtype], (c["name"], reg, cos)
                if reg not in P.CLAMPED:                # the exact dx nearly cancels: far below g / n
                    dx = P.bwd64(b["x"][n:n + 1], b["g"][n:n + 1], 1)
                    assert float(dx.norm()) <= 4 * P.U[dtype] * float(g[n].norm() / x[n].norm()), (c["name"], reg)
        if c["rows"] == "all":
            n64 = x.norm(dim=-1)
            for n, reg in enumerate(b["regime"]):
                assert (float(n64[n]) <= P.EPS / 4) if reg in P.CLAMPED else (float(n64[n]) >= 4 * P.EPS), (c["name"], reg)


def _argmin_first(vals):
    return int(np.argmin(vals))


def test_mask_rows_are_what_they_claim():
    rs = np.random.RandomState(5)
    for L in P.L_TABLE:
        for n in range(12):
            for kind in P.mask_kinds(L):
                m = P.mask_row(kind, L, n, rs)
                assert m.dtype == np.int64 and m.shape == (L,) and int(m.max()) < 2 ** 62, (kind, L)
                am = _argmin_first(m)
                if kind.startswith("fz"):
                    assert am == int(kind[2:]) and bool((m[:am] == 1).all())
                elif kind == "ones":
                    assert am == 0 and int(P.R.last_token_index(m[None])[0]) == L - 1
                elif kind == "last_zero":
                    assert am == L - 1
                elif kind.startswith("wide"):
                    assert am >= 1
                    low = (m & 0xFFFFFFFF).astype(np.int64)                     # a compare or shuffle that keeps the low half only
                    high = m >> 32                                                # ... the high half only
                    via_f32 = m.astype(np.float32)                                # ... or goes through f32
                    unsigned = m.astype(np.uint64)
                    if kind == "wide_a":
                        assert set(m.tolist()) <= set(P.WIDE_A)
                        assert _argmin_first(high) != am and _argmin_first(via_f32) != am
                    elif kind == "wide_c":
                        assert set(m.tolist()) <= set(P.WIDE_C) and _argmin_first(low) != am
                    else:
                        assert set(m.tolist()) <= set(P.WIDE_B) and int(m.min()) < 0
                        assert _argmin_first(low) != am and _argmin_first(unsigned) != am
    # the planted minimum of the wide rows visits every seam position that fits
    seen = {(k, _argmin_first(P.mask_row(k, 1024, n, rs))) for k in ("wide_a", "wide_b", "wide_c") for n in range(16)}
    assert {p for _, p in seen} == {p for p in P.FIRST_ZEROS if p >= 1}


# ------------------------------------------------------------------------------------------------
# a correct kernel can meet every rule: the float32 restatements on every case
# ------------------------------------------------------------------------------------------------
def _merge(dst, src):
    for k, v in src.items():
        dst[k] = max(dst.get(k, 0.0), v)


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_restated_forward_meets_every_rule_on_every_case(dtype):
    worst = {}
    for c in _cases(P.FWD_CASES, dtype):
        b = P.build_fwd(c)
        out, nrm = P.fwd_restate(b["x"], c["normalize"], dtype)
        ctrl = P.fwd_control_f32(b["x"], c["normalize"]) if dtype == torch.float32 else None
        _merge(worst, P.check_fwd(c, b, out, b["idx"].int(), nrm, ctrl))
    print("\nrestated forward %s, worst ratio per regime over %d cases: %s" % (P.TAG[dtype], len(_cases(P.FWD_CASES, dtype)), worst))


@pytest.mark.parametrize("dtype", P.DTYPES, ids=IDS)
def test_restated_backward_meets_every_rule_on_every_case(dtype):
    worst = {}
    for c in _cases(P.BWD_CASES, dtype):
        b = P.build_bwd(c)
        y, nrm = P.fwd_restate(b["x"], c["normalize"], dtype)
        dx = P.bwd_restate(b["g"], y, nrm, c["normalize"], dtype)
        w = P.check_bwd(c, b, dx, P.bwd_control(b["x"], b["g"], c["normalize"]))
        _merge(worst.setdefault(c["g"], {}), w)
    print("\nrestated backward %s, worst err / bound per gradient and row regime: %s" % (P.TAG[dtype], worst))


def test_a_wrong_kernel_misses_the_rules():
    """The rules bite: an index off by one row, a norm off by 1e-5, y taken before its rounding, a non-zero off-row pattern."""
    c = next(c for c in P.FWD_CASES if c["name"] == "bf16-block-L257-d512")
    b = P.build_fwd(c)
    out, nrm = P.fwd_restate(b["x"], 1, c["dtype"])
    with pytest.raises(AssertionError):
        P.check_fwd(c, b, out, (b["idx"] + 1).int() % c["L"], nrm)
    with pytest.raises(AssertionError):
        P.check_fwd(c, b, out, b["idx"].int(), nrm * (1 + 1e-5))
    with pytest.raises(AssertionError):
        P.check_fwd(c, b, (out.float() * (1 + 2.0 ** -6)).to(c["dtype"]), b["idx"].int(), nrm)
    c = next(c for c in P.BWD_CASES if c["name"] == "bf16-regimes-random-d264")
    b = P.build_bwd(c)
    y, nrm = P.fwd_restate(b["x"], 1, c["dtype"])
    dx = P.bwd_restate(b["g"], y, nrm, 1, c["dtype"])
    ctrl = P.bwd_control(b["x"], b["g"], 1)
    P.check_bwd(c, b, dx, ctrl)
    with pytest.raises(AssertionError):
        P.check_bwd(c, b, (dx.float() * 1.05).to(c["dtype"]), ctrl)
    with pytest.raises(AssertionError):                         # the projection dropped: dx = g / n
        P.check_bwd(c, b, P.bwd_restate(b["g"], torch.zeros_like(y), nrm, 1, c["dtype"]), ctrl)
