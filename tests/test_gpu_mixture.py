"""The mixture profile on the GPU (csrc/edmix.inc: k_mix_profile) against the long-double checker (tests/mixture_checker.py), against
the tree's own route (a strict run at each mixture and the posterior's log-evidence), bit for bit against itself, and fit_prop_tumor on
the device against the checker-driven search.

The bar is the posterior's (tests/posterior_checker.py): 8 (m + 1) 2^-52 max(1, max |finite alpha|), absolute, per chain.  The emissions
are the checker's bit for bit (the oracle's PORTABLE flavour is the strict mode's arithmetic), so the bar is the whole budget against
the checker; against the tree's route -- a backward recurrence where this kernel runs a forward one -- it is twice the bar.

Shapes: chromosomes of 0, 1, 2, 3, T - 1, T, T + 1, 2 T, 2 T + 1 and 3 T + 5 exons, T the kernel's tile (mixture_geometry).  One reference
is computed for 17 pairs x 16 mixtures and shared: a value depends on its pair and its mixture alone, so every narrower case is a slice.

Measured on an MI355X when this file was written (test_report prints the figures with -s): see DESIGN.md 4.21.
"""
import ctypes as C

import numpy as np
import pytest

import mixture_checker as mc
import posterior_checker as pc
from test_mixture_host import FRACTIONS, SEED, recovery_case

pytestmark = pytest.mark.gpu

S_MAX, G_MAX = 17, 16
FIT_SIZES = (1, 2, 130, 0, 200)      # the host test's seeded case at the smallest sizes that keep its three fractions informative
REPORT = {"values": 0, "frac": 0.0, "frac_route": 0.0, "nan": 0, "fit_margin": np.inf}
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _case(edlib, oracle):
    """layout, counts (E, 17) with obs = 0 and tot = 0 cells, phi, expected, the grid (16, 17) and the checker's (logZ, bar) for it"""
    if "case" not in _CACHE:
        T = edlib.mixture_geometry()["tile"]
        sizes = (0, 1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T + 5)
        rng = np.random.default_rng(17)
        chrom_off, start, end, test, ref, _, _ = mc.draw(sizes, [(None, 1.0, 0.5, 0.2)[s % 4] for s in range(S_MAX)], 23, depth=300.0)
        E = test.shape[0]
        for s in range(S_MAX):                                  # cells without tumour reads, and cells without reads at all
            rows = rng.choice(E, 12, replace=False)
            test[rows[:6], s] = 0
            test[rows[6:], s], ref[rows[6:], s] = 0, 0
        test[0, :], ref[0, :] = 0, 0                            # the chain of one exon: no reads for anybody
        phi = rng.uniform(5e-4, 3e-3, S_MAX)
        expected = rng.uniform(0.30, 0.55, S_MAX)
        grid = rng.uniform(0.0, 1.0, (G_MAX, S_MAX))
        grid[0, 0::2] = 0.0
        grid[3, :] = 1.0
        grid[4, :] = grid[2, :]                                 # a repeated value
        grid[9, 1::3] = 0.0
        grid[15, 1::2] = 1.0
        grid[15, 0] = grid[0, 0]
        trs = pc.transitions(chrom_off, start, end, 1e-4, 50000.0)
        ll = mc.emissions(oracle, test, ref, phi, expected, grid)
        z, bar = mc.logz(ll, chrom_off, trs, G_MAX, S_MAX)
        _CACHE["case"] = dict(T=T, sizes=sizes, chrom_off=chrom_off, start=start, end=end, test=test, ref=ref, phi=phi, expected=expected,
                              grid=grid, z=z, bar=bar)
    return _CACHE["case"]


def _profile(plan, k, S, G, layout, grid=None):
    test, ref = k["test"][:, :S], k["ref"][:, :S]
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    grid = k["grid"][:G, :S] if grid is None else grid
    return plan.mixture_profile(np.ascontiguousarray(test), np.ascontiguousarray(ref), k["phi"][:S], k["expected"][:S], grid, layout=layout)


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("G", [1, 5, 16])
@pytest.mark.parametrize("S", [1, 3, 17])
def test_edges_against_the_checker(edlib, oracle, S, G, layout):
    k = _case(edlib, oracle)
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    got = _profile(plan, k, S, G, layout)
    plan.close()
    assert got.shape == (G, len(k["sizes"]), S)
    want, bar = k["z"][:G, :, :S], k["bar"][:G, :, :S]
    empty = np.array(k["sizes"]) == 0
    assert np.all(got[:, empty, :] == 0.0)
    assert np.all(np.isfinite(want.astype(np.float64)[:, ~empty, :])) and np.all(np.isfinite(got))
    frac = (np.abs(got.astype(np.longdouble) - want).astype(np.float64)[:, ~empty, :] / bar[:, ~empty, :])
    print("S = %d, G = %d, layout %d: largest share of the bar %.4f" % (S, G, layout, frac.max()))
    REPORT["values"] += frac.size
    REPORT["frac"] = max(REPORT["frac"], float(frac.max()))
    assert np.all(frac <= 1.0), float(frac.max())
    # the repeated mixtures (rows 2 and 4; 1.0 in rows 3 and 15 of the odd pairs) have the same bits
    if G >= 5:
        assert np.array_equal(bits(got[2]), bits(got[4]))
    if G == 16 and S >= 2:
        assert np.array_equal(bits(got[3, :, 1]), bits(got[15, :, 1]))


def test_against_the_strict_run_and_the_posterior(edlib, oracle):
    """per mixture: Batch.set_mixture, a strict run, Batch.log_evidence -- within twice the bar; pairs outside the model's domain
    (phi >= 1, expected 0 and 1) are NaN for NaN, and change nothing for their neighbours"""
    k = _case(edlib, oracle)
    S, G = 7, 4
    phi, expected = k["phi"][:S].copy(), k["expected"][:S].copy()
    phi[1], expected[3], expected[5] = 1.5, 0.0, 1.0
    test, ref = np.ascontiguousarray(k["test"][:, :S]), np.ascontiguousarray(k["ref"][:, :S])
    grid = np.ascontiguousarray(k["grid"][[0, 1, 3, 7], :S])
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    got = plan.mixture_profile(test, ref, phi, expected, grid)
    good = plan.mixture_profile(test, ref, k["phi"][:S], k["expected"][:S], grid)
    nonempty = np.array(k["sizes"]) > 0
    for g in range(G):
        b = edlib.Batch(plan, S)
        b.set_mixture(grid[g])
        b.run(test, ref, phi, expected)
        route, ll = b.log_evidence(), b.loglik()
        b.close()
        assert np.array_equal(np.isnan(route), np.isnan(got[g])), g
        res = pc.run(ll, k["chrom_off"], pc.transitions(k["chrom_off"], k["start"], k["end"], 1e-4, 50000.0), np.float64)
        for c, r in enumerate(res):
            if r is None:
                assert np.all(got[g, c] == 0.0) and np.all(route[c] == 0.0)
                continue
            fin = np.isfinite(route[c])
            bar = pc.bar(k["sizes"][c], r["alpha"])
            frac = np.abs(got[g, c, fin] - route[c, fin]) / (2 * bar[fin])
            REPORT["frac_route"] = max(REPORT["frac_route"], float(frac.max()) if frac.size else 0.0)
            assert np.all(frac <= 1.0), (g, c, float(frac.max()))
            assert np.array_equal(np.isinf(route[c]), np.isinf(got[g, c]))
    plan.close()
    # (which values of such a pair are NaN is the strict arithmetic's business -- the pattern was compared with the route's above)
    bad = np.isnan(got[:, nonempty, :]).any(axis=(0, 1))
    print("pairs with NaN values:", np.flatnonzero(bad).tolist(), "fully NaN:", np.flatnonzero(np.isnan(got[:, nonempty, :]).all(axis=(0, 1))).tolist())
    REPORT["nan"] += int(np.isnan(got).sum())
    assert bad[[1, 3, 5]].any() and not bad[[0, 2, 4, 6]].any()
    assert np.array_equal(bits(got[:, :, [0, 2, 4, 6]]), bits(good[:, :, [0, 2, 4, 6]]))


def test_a_value_has_the_same_bits_wherever_it_is_computed(edlib, oracle):
    """the same (pair, mixture) in a batch of 1 and of 17, at g = 0 and g = 15, with G from 1 to 16, in both layouts and next to other
    grid values: identical bytes"""
    k = _case(edlib, oracle)
    p0, m0 = 5, 0.37
    one = {key: np.ascontiguousarray(k[key][:, p0:p0 + 1]) for key in ("test", "ref")}
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    base = plan.mixture_profile(one["test"], one["ref"], k["phi"][p0:p0 + 1], k["expected"][p0:p0 + 1], np.array([m0]))
    assert base.shape == (1, len(k["sizes"]), 1) and np.all(np.isfinite(base))
    rng = np.random.default_rng(5)
    n = 0
    for layout in (0, 1):
        alone = plan.mixture_profile(one["test"].T.copy() if layout else one["test"], one["ref"].T.copy() if layout else one["ref"],
                                     k["phi"][p0:p0 + 1], k["expected"][p0:p0 + 1], np.array([[m0]]), layout=layout)
        assert np.array_equal(bits(alone), bits(base))
        for G in (1, 2, 7, 16):
            for others in range(2):
                grid = rng.uniform(0.0, 1.0, (G, S_MAX))
                grid[G - 1, p0] = m0
                grid[0, p0] = m0 if others else grid[0, p0]
                got = _profile(plan, k, S_MAX, G, layout, grid=grid)
                assert np.array_equal(bits(got[G - 1, :, p0]), bits(base[0, :, 0])), (layout, G, others)
                if others:
                    assert np.array_equal(bits(got[0, :, p0]), bits(base[0, :, 0])), (layout, G)
                n += 1
    assert n == 16
    plan.close()


def _tolerances(fit, keep):
    """allowed differences of estimate, se and gain per pair: +- the sum of the chains' bars on every ordinate of the checker's last
    grid, propagated to first order through the vertex and curvature formulas, times 2"""
    grid, l, bar = keep[-1]
    S = l.shape[1]
    cols = np.arange(S)
    k = fit["trace"][-1]["k"]
    km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, 15)
    h = grid[1] - grid[0]
    lm, lk, lp = l[km, cols], l[k, cols], l[kp, cols]
    dm, dk, dp = bar[km, cols], bar[k, cols], bar[kp, cols]
    d2, a = (lm - 2 * lk) + lp, lm - lp
    vertex = (k >= 1) & (k <= 14) & (d2 < 0)
    with np.errstate(all="ignore"):
        t_m = 2 * 0.5 * h * (np.abs(1 / d2 - a / d2 ** 2) * dm + np.abs(-1 / d2 - a / d2 ** 2) * dp + np.abs(2 * a / d2 ** 2) * dk)
        t_se = 2 * 0.5 * h * (-d2) ** -1.5 * (dm + 2 * dk + dp)
    null_bar = keep[0][2][0]                                    # l(0) is the first ordinate of round 0
    return np.where(vertex, t_m, 0.0), np.where(vertex, t_se, 0.0), 2 * (dk + null_bar)


def test_fit_on_the_device_follows_the_checker(edlib, oracle):
    """the device-driven and the checker-driven (long double) search choose the same k* in every round for every pair -- the checker's
    two largest ordinates are more than twice the summed bars apart in every round, asserted here -- and end within the propagated bars"""
    from exomedepth_amd import fit_prop_tumor
    key = ("ld", FIT_SIZES, SEED)
    if key not in _CACHE:
        data = mc.draw(FIT_SIZES, FRACTIONS, SEED)
        chrom_off, start, end, test, ref, phi, expected = data
        keep = []
        ev = mc.evaluator(oracle, chrom_off, start, end, test, ref, phi, expected, fast=False, keep=keep)
        _CACHE[key] = (data, fit_prop_tumor(chrom_off, start, end, phi=phi, expected=expected, evaluate=ev), keep)
    (chrom_off, start, end, test, ref, phi, expected), cpu, keep = _CACHE[key]
    S = len(FRACTIONS)
    cols = np.arange(S)
    for r, (grid, l, bar) in enumerate(keep):
        srt = np.sort(l, axis=0)
        margin = (srt[-1] - srt[-2]) / (2 * bar[np.argmax(l, axis=0), cols])
        REPORT["fit_margin"] = min(REPORT["fit_margin"], float(margin.min()))
        assert np.all(margin > 1.0), (r, margin)                # 0 pairs excused
    assert np.array_equal(cpu["informative"], [True, True, True, False])
    dev = edlib.fit_prop_tumor(chrom_off, start, end, test, ref, phi=phi, expected=expected)
    print({k: v for k, v in dev.items() if k not in ("trace", "profile")})
    assert dev["evaluations"] == cpu["evaluations"] == 3
    for r in range(3):
        assert np.array_equal(dev["trace"][r]["k"], cpu["trace"][r]["k"]), r
        assert np.array_equal(dev["trace"][r]["grid"], cpu["trace"][r]["grid"]), r
        assert np.all(np.abs(dev["trace"][r]["values"] - keep[r][1]) <= keep[r][2]), r
    t_m, t_se, t_gain = _tolerances(cpu, keep)
    assert np.all(np.abs(dev["estimate"] - cpu["estimate"]) <= t_m), (dev["estimate"], cpu["estimate"], t_m)
    both = ~np.isnan(cpu["se"])
    assert np.array_equal(np.isnan(dev["se"]), np.isnan(cpu["se"])) and np.all(np.abs(dev["se"] - cpu["se"])[both] <= t_se[both])
    assert np.all(np.abs(dev["gain"] - cpu["gain"]) <= t_gain)
    assert np.array_equal(dev["informative"], cpu["informative"]) and np.array_equal(dev["at_bound"], cpu["at_bound"])
    assert np.array_equal(np.isnan(dev["prop_tumor"]), np.isnan(cpu["prop_tumor"]))
    inf = cpu["informative"]
    assert np.all(np.abs(dev["prop_tumor"] - cpu["prop_tumor"])[inf] <= t_m[inf])
    # the one-pair convenience is the same fit
    x = edlib.ExomeDepth(test[:, 1].astype(float), ref[:, 1].astype(float), phi=float(phi[1]), expected=float(expected[1]))
    chrom = np.repeat([str(c + 1) for c in range(len(FIT_SIZES))], FIT_SIZES)
    alone = x.fit_prop_tumor(chrom, start, end)
    assert bits(alone["estimate"])[0] == bits(dev["estimate"])[1] and bits(alone["gain"])[0] == bits(dev["gain"])[1]


def test_somatic_call_with_a_fitted_fraction(edlib, capsys):
    """somatic_CNV_call(prop_tumor="fit"): the estimate is used and recorded for an informative pair; a CNV-free pair is called at 1.0
    with a line on stderr; the result equals the numeric call at the value used"""
    chrom_off, start, end, test, ref, phi, expected = mc.draw(FIT_SIZES, FRACTIONS, SEED)
    chrom = np.repeat([str(c + 1) for c in range(len(FIT_SIZES))], FIT_SIZES)
    names = np.array(["e%d" % i for i in range(start.size)], dtype=object)
    for s, informative in ((1, True), (3, False)):
        capsys.readouterr()
        x = edlib.somatic_CNV_call(ref[:, s].astype(float), test[:, s].astype(float), prop_tumor="fit", chromosome=chrom, start=start,
                                   end=end, names=names)
        err = capsys.readouterr().err
        fit = x.prop_tumor_fit
        assert bool(fit["informative"][0]) == informative
        if informative:
            assert x.prop_tumor == fit["prop_tumor"][0] and abs(x.prop_tumor - FRACTIONS[s]) <= 1.0 / 15 and "Fitted prop_tumor" in err
        else:
            assert x.prop_tumor == 1.0 and np.isnan(fit["prop_tumor"][0]) and "not identifiable" in err
        y = edlib.somatic_CNV_call(ref[:, s].astype(float), test[:, s].astype(float), prop_tumor=x.prop_tumor, chromosome=chrom,
                                   start=start, end=end, names=names)
        assert y.CNV_calls == x.CNV_calls and np.array_equal(bits(y.likelihood), bits(x.likelihood))
        assert bool(x.CNV_calls) == informative
    with pytest.raises(ValueError):
        edlib.somatic_CNV_call(ref[:, 0], test[:, 0], prop_tumor="guess", chromosome=chrom, start=start, end=end, names=names)


def test_refusals(edlib, oracle):
    """n_grid of 0 and 17, a layout that does not exist and a NULL pointer: ED_ERR_INVALID with a message, and nothing is launched (the
    output keeps what it held)"""
    k = _case(edlib, oracle)
    S = 3
    lib = edlib._lib.lib()
    plan = edlib.Plan(k["chrom_off"], k["start"], k["end"])
    Cn = len(k["sizes"])
    d = {key: edlib.DeviceArray(np.ascontiguousarray(k[key][:, :S])) for key in ("test", "ref")}
    d.update({key: edlib.DeviceArray(np.ascontiguousarray(k[key][:S])) for key in ("phi", "expected")})
    d["grid"] = edlib.DeviceArray(np.ascontiguousarray(np.repeat(k["grid"][:, :S], 2, axis=0)[:17]))
    mark = np.full((17, Cn, S), -7.5)
    out = edlib.DeviceArray(mark)

    def call(n_grid=16, layout=0, null=None):
        p = {key: (None if key == null else v.ptr) for key, v in d.items()}
        o = None if null == "out" else out.ptr
        return lib.ed_plan_mixture_profile(plan.handle if null != "plan" else None, p["test"], p["ref"], layout, S, p["phi"], p["expected"],
                                           p["grid"], n_grid, o, None)
    cases = [dict(n_grid=0), dict(n_grid=17), dict(n_grid=-1), dict(layout=2), dict(layout=-1)] + \
            [dict(null=key) for key in ("test", "ref", "phi", "expected", "grid", "out", "plan")]
    for kw in cases:
        assert call(**kw) == -1, kw                             # ED_ERR_INVALID
        msg = lib.ed_last_error().decode()
        assert "ed_plan_mixture_profile" in msg, (kw, msg)
    edlib.api.check(lib.ed_synchronize(None))
    assert np.array_equal(bits(out.to_host()), bits(mark))
    assert call() == 0
    edlib.api.check(lib.ed_synchronize(None))
    assert not np.any(out.to_host()[:16] == -7.5)
    with pytest.raises(edlib.EdError, match="n_grid = 17"):
        plan.mixture_profile(k["test"][:, :S], k["ref"][:, :S], k["phi"][:S], k["expected"][:S], np.linspace(0, 1, 17))
    with pytest.raises(edlib.EdError, match="layout"):
        plan.mixture_profile(k["test"][:, :S].T, k["ref"][:, :S].T, k["phi"][:S], k["expected"][:S], np.linspace(0, 1, 4), layout=2)
    assert edlib.mixture_geometry() == {"tile": k["T"], "max_grid": 16, "pairs_per_workgroup": 1, "lds_bytes": edlib.mixture_geometry()["lds_bytes"]}
    assert 2 * k["T"] * 33 * 8 <= edlib.mixture_geometry()["lds_bytes"] <= 160 * 1024
    for v in d.values():
        v.free()
    out.free()
    plan.close()


def test_report():
    """the figures quoted in DESIGN.md 4.21 (printed with -s)"""
    print("\nmixture profile: %(values)d values against the long-double checker, largest share of the bar %(frac).4f; against the strict "
          "run and the posterior's log-evidence the largest share of twice the bar %(frac_route).4f (%(nan)d NaN values of pairs outside "
          "the domain); fit: the checker's two largest ordinates are at least %(fit_margin).2f x twice the summed bars apart" % REPORT)
    assert REPORT["values"] > 0 and REPORT["nan"] > 0
