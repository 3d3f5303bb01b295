"""CPU side of the loss-head parity tests (tests/loss_parity_util.py): the case table reaches every forward path of
csrc/infonce.hip for every dtype that can reach it, and every tolerance the GPU tests introduce holds for a plain numpy float32
evaluation of the kernels' own formulas against float64, on the very inputs the GPU tests use."""
import numpy as np
import pytest

import loss_parity_util as U
from oracle import scoring_ref as R


def _stored_scores(case, regime, tag, every=1):
    """The scores a correct kernel stores for (case, regime, tag), rows [::every] (score rows are independent of each other)."""
    Q, P, d = case[:3]
    label, bc = U.infonce_path(Q, P, d, tag, case[4])
    q, p, T, marks = U.infonce_regime(regime, Q, P, d, bc)
    qv, pv = U.round_store(q[::every], tag), U.round_store(p, tag)
    s = U.round_store(U.expected_scores(R.similarity(qv, pv), T, tag), tag)
    return s, marks["target"][::every], label, bc


@pytest.mark.parametrize("tag", U.DTYPES)
def test_infonce_cases_cover_every_forward_path(tag):
    """Every label of the dispatch mirror that `tag` can reach is reached by a case of the table (`tile256` is bf16 only;
    `skinny-multi+ce_finalize` is unreachable through the C ABI, see the util's docstring), the paths named in the table's comments
    are the ones the mirror gives, and the extra cases (GEMM-form backward, own-row window, run-twice) take the paths they name."""
    got = {}
    for c in U.INFONCE_CASES:
        if tag in c[3]:
            got.setdefault(U.infonce_path(c[0], c[1], c[2], tag, c[4])[0], []).append(U.case_id(c))
    print(f"\n{tag}: " + "; ".join(f"{k}: {', '.join(v)}" for k, v in sorted(got.items())))
    assert set(got) == U.reachable_labels(tag), (sorted(set(got) ^ U.reachable_labels(tag)))
    want = ["small", "small", "skinny4-1blk", "skinny1-1blk", "skinny-multi", "skinny-multi", "skinny-multi", "rowwise-chunk",
            "rowwise-k", "rowwise-unaligned", "tile64x64", "tile128x64", "tile128x128", "tile256"]
    for c, w in zip(U.INFONCE_CASES, want):
        if tag in c[3]:
            assert U.infonce_path(c[0], c[1], c[2], tag, c[4])[0] == w, (c, w)
    assert U.infonce_path(*U.TWICE_CASE, tag)[0] == "skinny-multi"
    assert U.infonce_path(*U.WINDOW_CASE[:3], tag)[0] == "skinny-multi"
    assert U.infonce_path(*U.GEMM_CASE, tag)[0].startswith("tile")
    # the alignment flag alone moves (100, 300, 128) to the rowwise kernel
    assert U.infonce_path(100, 300, 128, tag, True)[0].startswith("tile")


def test_regimes_are_what_they_claim():
    """float64 scores of the builders: `hot` peaks at 256 on the planted column (not the target for two thirds of the rows), `cold`
    keeps every score below -200, `flat` is constant, `split` puts the row maximum (128) in another partial block than the target
    and every other score more than 100 below it at d = 2048, where exp(m - M) is zero in float32; random unit rows of d = 64 .. 264
    reach cosines of 0.6, so there the gap is 40 .. 100 and exp(m - M) is 1e-18 .. 1e-43: below an ulp of l, not zero),
    `unscaled` has T == 1 and |s| < 16."""
    for case in U.INFONCE_CASES[:-3]:
        Q, P, d = case[:3]
        bc = U.infonce_path(Q, P, d, "bf16", case[4])[1]
        for regime in U.INFONCE_REGIMES:
            q, p, T, mk = U.infonce_regime(regime, Q, P, d, bc)
            s = R.similarity(q, p) / T
            rows = np.arange(Q)
            if regime == "hot":
                assert T == 2.0 ** -8 and np.allclose(s[rows, mk["planted"]], 256.0, atol=1e-9)
                assert (s[rows, mk["planted"]] >= s.max(-1) - 1e-9).all()
                if Q >= 3:
                    assert (mk["planted"] != mk["target"]).sum() >= Q // 2
                    assert (s.max(-1) - s[rows, mk["target"]])[mk["kind"] != 0].min() > 100
            elif regime == "cold":
                assert s.max() < -200 or d < 16, s.max()
                assert s.max() < -100
            elif regime == "flat":
                assert np.ptp(s) < 1e-9
            elif regime == "split":
                assert (mk["planted"] // bc != mk["target"] // bc).all()
                assert np.allclose(s[rows, mk["planted"]], 128.0, atol=1e-9)
                other = s.copy()
                other[rows, mk["planted"]] = -np.inf
                # every column but the planted one (hence every other block's maximum) is far below it
                assert (128.0 - other.max(-1)).min() > (100 if d >= 2048 else 40 if d >= 64 else 0), (case, (128.0 - other.max(-1)).min())
            else:
                assert T == 1.0 and np.abs(s).max() < 16.0 + 1e-9


def test_infonce_float32_formula_stays_inside_the_stated_bounds():
    """The kernels' max-subtracted formula in numpy float32 -- block partials (max, sum exp2(fma(v, log2 e, -max log2 e))) over the
    block width of each case's path, merged in block order by softmax_merge, lse = m + logf(l), row loss = lse - s_target, float32
    mean -- against the float64 logsumexp / CE of the same stored scores, for every case, regime and dtype of the table (problems
    over a million scores: every 8th row, rows being independent) and for the RPO_TARGET_FIRST cases.  It must stay inside `lse_bound` /
    `loss_bound`; this is what justifies N_LSE = 2, N_ROW = 3, REL_LOG, ABS_LOG and REDUCE_ROUNDINGS.

    Measured (numpy 2, x86-64): worst |lse32 - lse64| / bound = 0.41 (33 x 99 x 72 f32 `cold`) and worst |loss32 - loss64| / bound
    = 0.06 over the in-batch cases; 0.23 and 0.06 over the first-target cases: a factor of two on a row and of sixteen on the mean
    left for the kernels' different summation orders and for v_exp_f32 / v_log_f32 (1 ulp each) in place of libm."""
    worst = {"lse": (0.0, None), "loss": (0.0, None)}

    def check(s, tgt, bc, name):
        ce = U.ce_from_scores(s, tgt)
        lse32, loss32 = U.infonce_stats_f32(s, tgt, bc)
        assert np.isfinite(lse32).all() and np.isfinite(loss32), name
        r_lse = float((np.abs(lse32 - ce["lse"]) / U.lse_bound(ce)).max())
        r_loss = abs(loss32 - ce["loss"]) / U.loss_bound(ce)
        assert r_lse <= 1.0 and r_loss <= 1.0, (name, r_lse, r_loss)
        for k, r in (("lse", r_lse), ("loss", r_loss)):
            if r > worst[k][0]:
                worst[k] = (r, name)
        return r_lse, r_loss

    for case in U.INFONCE_CASES:
        every = 1 if case[0] * case[1] <= 2 ** 20 else 8
        for tag in case[3]:
            for regime in U.INFONCE_REGIMES:
                s, tgt, label, bc = _stored_scores(case, regime, tag, every)
                r = check(s, tgt, bc, (U.case_id(case), tag, regime, label))
                print(f"{U.case_id(case):>22} {tag:>4} {regime:>8} {label:>17}: lse {r[0]:.3f}  loss {r[1]:.3f}  of the bound")
    print("in-batch worst:", worst)
    worst = {"lse": (0.0, None), "loss": (0.0, None)}
    for B, G, d in U.FIRST_CASES:
        for tag in U.DTYPES:
            for regime in U.FIRST_REGIMES:
                q, p, T, _ = U.first_regime(regime, B, G, d)
                qv, pv = U.round_store(q, tag), U.round_store(p, tag)
                raw = np.einsum("bd,bgd->bg", qv, pv.reshape(B, G, d))
                s = U.round_store(U.expected_scores(raw, T, tag), tag)
                r = check(s, np.zeros(B, int), 1, (B, G, d, tag, regime))
                print(f"first {B}x{G}x{d} {tag:>4} {regime:>8}: lse {r[0]:.3f}  loss {r[1]:.3f}  of the bound")
    print("first-target worst:", worst)


def test_rankpo_float32_formula_stays_inside_the_stated_bounds():
    """rankpo_finalize_kernel's formulas in numpy float32 (log_sigmoid = min(x, 0) - log1p(exp(-|x|)), the SFT term's two-way
    logsumexp, float32 means and weights) on the float32-rounded float64 scores of every RankPO shape, regime and dtype, against the
    float64 oracle formulas on the same scores: per-row losses inside `rankpo_rows_f64`'s bound (RANKPO_ROUNDINGS = 10 units of
    2^-24 M_b), the loss inside `rankpo_loss_bound`.

    Measured: worst per-row error / bound = 0.22, worst loss error / bound = 0.05 (row losses up to 1721 in the `sat` regimes)."""
    worst_row = worst_loss = 0.0
    big = 0.0
    for B, d, _ in U.RANKPO_SHAPES:
        for name in U.RANKPO_REGIMES:
            cfg = U.rankpo_config(name)
            for tag in U.DTYPES:
                q, p, rc, rr, _ = U.rankpo_regime(name, B, d, tag)
                s = R.rankpo_scores(q, p).astype(np.float32).astype(np.float64)
                losses, sft, bound = U.rankpo_rows_f64(s, rc, rr, cfg)
                lb32, loss32 = U.rankpo_finalize_f32(s, rc, rr, cfg)
                loss64 = cfg["rankpo_weight"] * losses.mean() + (cfg["sft_weight"] * sft.mean() if cfg["sft_weight"] > 0 else 0.0)
                assert np.isfinite(lb32).all() and np.isfinite(loss32)
                r_row = float((np.abs(lb32 - losses) / bound).max())
                r_loss = abs(loss32 - loss64) / U.rankpo_loss_bound(losses, sft, bound, cfg)
                assert r_row <= 1.0 and r_loss <= 1.0, (B, d, name, tag, r_row, r_loss)
                worst_row, worst_loss, big = max(worst_row, r_row), max(worst_loss, r_loss), max(big, np.abs(losses).max())
                print(f"rankpo {B}x{d} {name:>15} {tag:>4}: rows {r_row:.3f}  loss {r_loss:.3f}  of the bound (max row loss {np.abs(losses).max():.1f})")
    print(f"rankpo worst: rows {worst_row:.3f}, loss {worst_loss:.3f}; largest row loss {big:.1f}")
    assert big > 500          # the regimes do reach losses in the hundreds


def test_rankpo_regimes_are_what_they_claim():
    for B, d, _ in U.RANKPO_SHAPES:
        for name in U.RANKPO_REGIMES:
            cfg = U.rankpo_config(name)
            q, p, rc, rr, mk = U.rankpo_regime(name, B, d, "bf16")
            s = R.rankpo_scores(q, p)
            r0 = 0 if rc is None else rc - rr
            bz = cfg["beta"] * ((s[:, 0] - s[:, 1] - r0) / cfg["temperature"] - cfg["gamma_beta_ratio"])
            if name.startswith("sat"):
                assert np.abs(bz).min() > 400, (name, np.abs(bz).min())            # both sigmoids saturate ...
                assert B < 2 or ((bz > 0).any() and (bz < 0).any())                 # ... both ways
                assert np.abs((s[:, 0] - s[:, 1]) / cfg["temperature"]).min() > 50  # SFT: |t0 - t1| = 58 .. 115
            if name == "hinge":
                assert mk["kink"].any() and (bz[mk["kink"]] == 1.0).all()
