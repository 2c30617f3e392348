"""The detection-power map without a GPU: the checker against a plain numpy / scipy form, its elementary properties, the interface's
declarations, the coordinate mapping of regions and the stand-alone check of the geometry."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import power_checker as pc  # noqa: E402

TOTALS = (1, 2, 3, 5, 17, 64, 255, 256, 257, 600, 1025)


@pytest.mark.parametrize("phi", [0.003, 0.05, 0.2])
def test_checker_agrees_with_the_scipy_form(phi):
    """mean and variance of the mpmath checker and of betaln / gammaln in binary64 agree within the walk's bar, 2e-10 of E|D| and of E[D^2]"""
    worst = 0.0
    for mixture in (1.0, 0.3):
        for n in TOTALS:
            want = pc.moments(n, phi, 0.1, mixture)
            got = pc.scipy_moments(n, phi, 0.1, mixture)
            for T in pc.STATES:
                bm, bv = pc.RTOL * want["abs_" + T], pc.RTOL * want["sq_" + T]
                em, ev = abs(got["mean_" + T] - want["mean_" + T]), abs(got["var_" + T] - want["var_" + T])
                worst = max(worst, em / bm, ev / bv)
                assert em <= bm and ev <= bv, (phi, mixture, n, T, em / bm, ev / bv)
    print("largest fraction of the bar at phi = %g: %.3g" % (phi, worst))


def test_walked_checker_is_the_definition():
    """the checker's walk from x = 0 and its term-by-term form from loggamma are the same numbers"""
    for n, phi, e, m in ((0, 0.05, 0.1, 1.0), (1, 0.2, 0.4, 0.3), (37, 0.003, 0.11, 1.0), (300, 1e-5, 0.05, 0.3)):
        a, b = pc.moments(n, phi, e, m), pc.moments(n, phi, e, m, direct=True)
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-25 + 1e-20 * abs(b[k]), (n, phi, e, m, k, a[k], b[k])


def test_mean_is_a_divergence_and_an_empty_exon_says_nothing():
    for phi in (1e-5, 0.003, 0.2):
        for e in (0.05, 0.4):
            for m in (1.0, 0.3):
                z = pc.moments(0, phi, e, m)
                assert all(z[k] == 0.0 for k in z), z
                for n in (1, 4, 257):
                    r = pc.moments(n, phi, e, m)
                    for T in pc.STATES:
                        assert r["mean_" + T] >= 0.0 and r["var_" + T] >= 0.0 and r["abs_" + T] >= r["mean_" + T]
    assert pc.in_model(*pc.shape_params(0.2, 0.1)) and not pc.in_model(*pc.shape_params(0.9, 0.1))
    # mixture 0 and a dyadic expected: the three states are the same distribution
    r = pc.moments(100, 0.01, 0.125, 0.0)
    assert all(r[k] == 0.0 for k in r)


def test_region_sum_order():
    assert pc.region_sum([]) == 0.0 and pc.region_sum([3.0]) == 3.0
    v = np.zeros(65)
    v[0], v[1], v[32] = 1e16, 1.0, -1e16
    assert pc.region_sum(v) == 1.0                 # lanes 0 and 32 meet first
    v[1], v[64] = 0.0, 1.0
    assert pc.region_sum(v) == 0.0                 # value 64 is lane 0's second: lost in 1e16 before lane 32 comes in
    rng = np.random.default_rng(5)
    x = rng.random(513)
    assert abs(pc.region_sum(x) - np.sum(x)) <= 513 * 2.0 ** -52 * np.sum(x)


def test_interface_declares_the_power_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edpower.inc")).read()
    for sym in ("ed_plan_power_map", "ed_power_regions", "ed_power_copy_exons", "ed_power_copy_table", "ed_power_stats", "ed_power_geometry"):
        assert sym in names, sym
        assert re.search(r"\b%s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT int %s\(" % sym, source), sym
    assert "ed_power_free" in names and re.search(r"\bvoid ed_power_free\(", header) and "ED_EXPORT void ed_power_free(" in source
    core = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    assert "k_pw_walk" in source and '#include "edpower.inc"' in core and '#include "ed_power_plan.hpp"' in core
    import exomedepth_amd
    from exomedepth_amd import api
    for name in ("PowerMap", "detection_power", "region_runs", "power_geometry", "power_from_moments", "POWER_DTYPE"):
        assert getattr(exomedepth_amd, name) is getattr(api, name) and name in exomedepth_amd.__all__
    assert callable(api.Plan.power_map) and callable(api.ExomeDepth.detection_power)
    for k in ("regions", "exons", "table", "stats", "free"):
        assert callable(getattr(api.PowerMap, k))


def test_region_runs():
    from exomedepth_amd import region_runs
    chrom = ["1"] * 5 + ["2"] + ["X"] * 4
    start = np.array([10, 100, 200, 300, 400, 50, 10, 20, 25, 40])
    end = start + 50
    end[8] = 200                                   # an exon of X that reaches far beyond its neighbours
    regions = [("1", 0, 1000),                     # the whole chromosome
               ("1", 100, 260), ("1", 101, 260),   # nested: the second starts inside exon 1 and loses it
               ("1", 120, 330),                    # overlapping the two before: cuts exons 1 and 3, holds exon 2
               ("1", 151, 199),                    # between two exons: nothing inside
               ("1", 460, 9000),                   # behind the last exon
               ("2", 0, 100), ("2", 60, 100),      # a one-exon chromosome: held, cut
               ("7", 0, 1),                        # a chromosome without exons
               ("X", 10, 95), ("X", 0, 70)]        # exon 8 lies between the first and the last exon inside and is not inside itself
    r = region_runs(chrom, start, end, regions)
    got = [(int(x["chrom"]), int(x["start_exon"]), int(x["end_exon"]), int(x["nexons"])) for x in r]
    assert got == [(0, 0, 4, 5), (0, 1, 2, 2), (0, 2, 2, 1), (0, 2, 2, 1), (0, -1, -1, 0), (0, -1, -1, 0), (1, 5, 5, 1), (1, -1, -1, 0),
                   (-1, -1, -1, 0), (2, 6, 9, 4), (2, 6, 7, 2)]
    # the rule itself, region by region: first and last exon wholly inside
    for (c, s, e), x in zip(regions, r):
        inside = [i for i in range(len(chrom)) if chrom[i] == c and start[i] >= s and end[i] <= e]
        assert (int(x["start_exon"]), int(x["end_exon"])) == ((inside[0], inside[-1]) if inside else (-1, -1))
    with pytest.raises(ValueError, match="contiguous"):
        region_runs(["1", "2", "1"], [1, 2, 3], [2, 3, 4], [])
    assert region_runs([], [], [], [("1", 0, 10)])["nexons"][0] == 0


def test_power_from_moments():
    from exomedepth_amd import power_from_moments
    from scipy.special import ndtr
    p = power_from_moments([1.0, 1.0, 1.0, 3.0, np.nan, 1.0], [0.0, 0.0, 0.0, 4.0, 1.0, np.nan], [0.0, 2.0, 1.0, 1.0, 0.0, 0.0])
    assert p[0] == 1.0 and p[1] == 0.0 and p[2] == 0.0 and p[3] == ndtr(1.0) and np.isnan(p[4]) and np.isnan(p[5])


def test_power_plan_checker(tmp_path):
    """tools/power_plan_check.cpp compiles (without the sanitizer flags its header comment gives for a run by hand) and exits with 0"""
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "power_plan_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "power_plan_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout
