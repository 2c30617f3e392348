"""The quantile map without a GPU: the checker's two forms against each other and against a plain scipy form, the edges of the
definition, the cut and bin rules, the planted cases the GPU test uses, the interface's declarations and the stand-alone check of
csrc/ed_quant_plan.hpp."""
import math
import os
import re
import subprocess
import sys

import mpmath as mp
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_checker as qc  # noqa: E402

TOTALS = (0, 1, 2, 3, 5, 17, 63, 64, 255, 256, 257, 511, 512, 513, 600, 1025, 4099)
PHIS = (1e-5, 0.003, 0.05, 0.2)
EXPECTED = (0.05, 0.11, 0.4)
PROBS = (1e-9, 0.025, 0.3, 0.5, 0.975, 1.0 - 1e-4)


def test_walked_checker_is_the_definition():
    """the checker's walk from x = 0 and its term-by-term form from loggamma are the same numbers: masses, C, quantile, below and G"""
    for n, phi, e in ((0, 0.05, 0.1), (1, 0.2, 0.4), (37, 0.003, 0.11), (300, 1e-5, 0.05), (257, 0.2, 0.4)):
        a, b = qc.shapes(phi, e)
        (pw, cw), (pd, cd) = qc.dist(n, a, b), qc.dist(n, a, b, direct=True)
        assert len(pw) == len(pd) == n + 1
        for x in range(n + 1):
            assert abs(pw[x] - pd[x]) <= 1e-30 * pd[x] and abs(cw[x] - cd[x]) <= 1e-30
        assert abs(cw[-1] - 1) <= 1e-30
        for p in PROBS:
            (qw, bw, xw), (qd, bd, xd) = qc.quantile(n, a, b, p), qc.quantile(n, a, b, p, direct=True)
            assert xw == xd and abs(qw - qd) * pd[xd] <= 1e-28 and abs(bw - bd) <= 1e-30
            assert abs(qc.G(float(qw), n, a, b) - qc.G(float(qw), n, a, b, direct=True)) <= 1e-28
            assert abs(qc.G(float(qw), n, a, b) - mp.mpf(p)) <= 4 * qc.U * max(float(qw), 1.0) * float(pd[xd])     # (q rounded to a double)


@pytest.mark.parametrize("phi", PHIS)
def test_checker_agrees_with_the_scipy_form(phi):
    """qbetabinom.ab restated with betaln / gammaln in binary64 against the checker, in probability space: |q_scipy - q| pm[cut] where the
    two name the same value, |G(q_scipy) - p| always.  The bar, 2e-9, is scipy's: log-gamma terms of magnitude up to a + b + n = 1e5 at
    phi = 1e-5, a few ulp each, put 1e-10 into a mass (the largest seen when this was written: 2.4e-10) -- an observation about this
    restatement, not the kernel's bar (quantile_checker.bar).  No case returns NaN."""
    worst = 0.0
    for e in EXPECTED:
        a, b = qc.shapes(phi, e)
        for n in TOTALS:
            pm, _ = qc.dist(n, a, b)
            for p in PROBS:
                q, _, x = qc.quantile(n, a, b, p)
                got = qc.scipy_qbetabinom_ab(p, n, a, b)
                assert got == got, (phi, e, n, p)
                err = float(abs(qc.G(got, n, a, b) - mp.mpf(p)))
                if qc.cut_of(got) == x:
                    err = max(err, float(abs(mp.mpf(got) - q) * pm[x]))
                worst = max(worst, err)
                assert err <= 2e-9, (phi, e, n, p, got, float(q), err)
    print("phi = %g: largest error in probability %.3g" % (phi, worst))


def test_edges_of_the_definition():
    a, b = qc.shapes(0.05, 0.11)
    for p in (1e-9, 0.5, 1.0 - 1e-4):
        q, bl, x = qc.quantile(0, a, b, p)                      # n = 0: pm = [1], q = p
        assert x == 0 and bl == 0 and float(q) == p
        assert qc.scipy_qbetabinom_ab(p, 0, a, b) == p
    for n in (0, 5, 300):
        for p in (1.0, 1.5, float("inf")):                      # p >= 1: nothing crosses
            assert qc.quantile(n, a, b, p) == (None, None, None)
            assert math.isnan(qc.scipy_qbetabinom_ab(p, n, a, b))
    # cut = 0: q = p / pm[0] in (0, 1); cut = n: the last cell
    pm, C = qc.dist(5, a, b)
    q, bl, x = qc.quantile(5, a, b, float(pm[0]) / 3)
    assert x == 0 and bl == 0 and 0 < q < 1 and abs(q - mp.mpf(1) / 3) < 1e-15
    q, bl, x = qc.quantile(5, a, b, float(C[4] + pm[5] / 2))
    assert x == 5 and bl == C[4] and 5 < q < 6
    # G is continuous across a cell's end and q inverts it
    for xx in (1, 2, 5):
        assert abs(qc.G(float(xx), 5, a, b) - C[xx - 1]) <= 1e-30 and abs(qc.G(xx + 1e-9, 5, a, b) - C[xx - 1]) <= 1e-8
    assert abs(qc.G(-1.0, 5, a, b) + pm[0]) <= 1e-30 and abs(qc.G(6.0, 5, a, b) - 1) <= 1e-30


def test_cut_of_inverts_every_quantile_of_the_grid():
    """cut_of(q) = ceil(q) - 1 is the cut of every q of the grid rounded to a double -- cut = 0 included, where q = p / pm[0] lies in (0, 1)
    -- unless q rounds to a whole number, the tie C(q - 1) = p, where it names the value below (csrc/ed_quant_plan.hpp)"""
    n_whole = n_zero = 0
    for phi in PHIS:
        for e in EXPECTED:
            a, b = qc.shapes(phi, e)
            for n in TOTALS:
                cuts = []
                for p in PROBS:
                    q, _, x = qc.quantile(n, a, b, p)
                    qf = float(q)
                    n_zero += x == 0
                    if qf == math.floor(qf) and qf > 0:
                        n_whole += 1
                        assert qc.cut_of(qf) in (x - 1, x)
                    else:
                        assert qc.cut_of(qf) == x, (phi, e, n, p, qf, x)
                    cuts.append(x)
                assert cuts == sorted(cuts)
                for obs in {0, n, *cuts, *[c - 1 for c in cuts if c > 0]}:
                    assert qc.bin_of(obs, cuts) == sum(1 for c in cuts if c <= obs)
    assert n_zero > 50
    print("%d quantiles at cut 0, %d rounded to a whole number" % (n_zero, n_whole))
    assert qc.cut_of(float("nan")) == qc.NO_CUT and qc.cut_of(0.0) == 0 and qc.cut_of(1.0) == 0 and qc.cut_of(1.5) == 1
    assert qc.bin_of(3, [3, 7]) == 1 and qc.bin_of(2, [3, 7]) == 0 and qc.bin_of(7, [3, 7]) == 2 and qc.bin_of(10 ** 9, [3, qc.NO_CUT]) == 1


def test_planted_cases_cross_where_they_say():
    """every case the GPU test plants: the checker puts each probability into the named value's cell, at least a quarter of its mass (a
    thousandth for the one far below pm[0]) and a hundred bars of the device's walk from either end -- but for the probability within
    rounding of 1, which is there for that"""
    W = 256
    names = []
    for name, n, phi, e, probs, cuts in qc.planted_cases():
        a, b = qc.shapes(phi, e)
        pm, _ = qc.dist(n, a, b)
        assert list(probs) == sorted(probs) and all(0 < p < 1 for p in probs)
        for p, x in zip(probs, cuts):
            assert qc.cut(n, a, b, p) == x, (name, p, x)
            if p < 1.0 - 1e-15:
                share = 9e-4 if "far below" in name else 0.24
                assert qc.margin(n, a, b, p, x) >= share * float(pm[x]), name
                assert qc.margin(n, a, b, p, x) > 100 * qc.bar(n, x, qc.log_mass_span(n, a, b, x + 4)), name
        names.append(name)
    by = {c[0]: c for c in qc.planted_cases()}
    assert by["last value of the first tile"][5] == [W - 1] and by["first value of the second tile"][5] == [W]
    assert by["crossing at n"][5] == [by["crossing at n"][1]] and by["crossing at 0: p / pm[0]"][5] == [0]
    x1, x2 = by["two in adjacent values of one lane"][5]
    assert x2 == x1 + 1 and x1 // 4 == x2 // 4
    x1, x2 = by["adjacent values of two lanes"][5]
    assert x2 == x1 + 1 and x1 // 4 + 1 == x2 // 4
    x1, x2 = by["two in one cell"][5]
    assert x1 == x2 and by["two in one cell"][4][0] < by["two in one cell"][4][1]
    n, phi, e = by["a probability far below a small pm[0]"][1:4]
    assert by["a probability far below a small pm[0]"][4][0] < 1e-3 * float(qc.dist(n, *qc.shapes(phi, e))[0][0]) * 1.001
    assert len(names) == len(set(names)) == 10


def test_the_bar_grows_with_the_walk_and_stays_small():
    assert qc.bar(1, 0, 1.0) < 1e-13 and qc.bar(4099, 4099, 50.0) < 1e-10 and qc.bar(32769, 32769, 2e4) < 1e-7
    assert qc.bar(600, 10, 5.0) < qc.bar(600, 500, 5.0) < qc.bar(4099, 500, 5.0) < qc.bar(4099, 500, 500.0)


def test_documented_examples_of_the_reference():
    """The three examples of the reference's manual pages (R/tools.R:17-18, :40).  No R is available to produce golden values, so they are
    checked as the definition: the scipy restatement of qbetabinom.ab's own lines against the 40-digit checker, which the GPU test
    (tests/test_gpu_quantile.py) holds the device to for the same three calls."""
    cases = [(0.2, 50, qc.shapes(0.4, 0.3)), (0.2, 50, qc.shapes(0.1, 0.8)), (0.5, 50, (0.2, 0.25))]
    for p, n, (a, b) in cases:
        q, bl, x = qc.quantile(n, a, b, p)
        got = qc.scipy_qbetabinom_ab(p, n, a, b)
        pm, _ = qc.dist(n, a, b)
        assert qc.cut_of(got) == x and abs(mp.mpf(got) - q) * pm[x] <= 1e-13, (p, n, a, b, got, float(q))
        assert 0 <= x <= n and x < float(q) + 1e-12 <= x + 1 + 1e-12
    # qbetabinom(0.2, 50, 0.4, 0.3): a = 0.45, b = 1.05 -- the median-ish of a U-shaped law lies low; with (0.1, 0.8) high
    assert qc.quantile(50, *cases[0][2], 0.2)[2] < 10 < 30 < qc.quantile(50, *cases[1][2], 0.2)[2]


def test_interface_declares_the_quantile_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edquant.inc")).read()
    for sym in ("ed_plan_quantile_map", "ed_quant_regions", "ed_quant_copy_exons", "ed_quant_copy_table", "ed_quant_stats", "ed_quant_geometry",
                "ed_qbetabinom_ab"):
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT int %s\(" % sym, source), sym
    assert "ed_quant_free" in names and re.search(r"\bvoid ed_quant_free\(", header) and "ED_EXPORT void ed_quant_free(" in source
    core = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    assert '#include "edquant.inc"' in core and '#include "ed_quant_plan.hpp"' in core
    for k in ("k_bq_walk", "k_bq_points", "k_bq_regions"):
        assert k in source, k
    csrc = os.path.join(ROOT, "exomedepth_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".inc", ".hpp", ".h"))}
    totals = texts["edtotals.inc"]
    assert core.index('#include "edtotals.inc"') < core.index('#include "edpower.inc"') < core.index('#include "edquant.inc"')
    # the occupancy passes, the exon kernel and the CDF walk are the shared core's (edtotals.inc): defined there once, used here, not copied
    for k in ("k_pw_scan", "k_pw_mark", "k_pw_rank", "k_pw_jobs", "k_pw_slots", "k_tm_exons", "bb_open", "bb_step"):
        assert len(re.findall(r"^(?:__device__ __forceinline__ \w+ )?%s\(" % k, totals, flags=re.M)) == 1, k
        assert not re.search(r"^(?:__device__ __forceinline__ \w+ )?%s\(" % k, source, flags=re.M), k
    assert "pw_occupy(" in source and "tm_copy_exons(" in source and "bb_open(" in source and "bb_step(" in source
    assert "k_bq_exons" not in "".join(texts.values()) and "k_pw_exons" not in "".join(texts.values())
    # one step ratio under csrc/: the quantile map and the draws form C from the same source
    ratio = "frcp((xd + 1.0) * (b + rest))"
    assert {f: t.count(ratio) for f, t in texts.items() if ratio in t} == {"edtotals.inc": 1}
    plan = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "ed_quant_plan.hpp")).read()
    assert "hip" not in plan.lower().replace("no hip", "") and "kMaxProbs = 16" in plan
    import exomedepth_amd
    from exomedepth_amd import api
    for name in ("QuantileMap", "normal_range", "qbetabinom", "qbetabinom_ab", "quantile_geometry"):
        assert getattr(exomedepth_amd, name) is getattr(api, name) and name in exomedepth_amd.__all__
    assert callable(api.Plan.quantile_map) and callable(api.ExomeDepth.normal_range)
    for k in ("regions", "exons", "table", "stats", "free"):
        assert callable(getattr(api.QuantileMap, k))
    assert api.quantile_geometry()["max_probs"] == 16


def test_quant_plan_checker(tmp_path):
    """tools/quant_plan_check.cpp compiles (without the sanitizer flags its header comment gives for a run by hand) and exits with 0"""
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "quant_plan_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "quant_plan_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout
