"""The copy-ratio profile and call_copy_number without a device: copy_number_from_profile and the search's interval / parabola logic on
hand-made profiles, what the C entries refuse before they need a device, the stand-alone check of the item builder
(tools/ratio_plan_check.cpp, under the host sanitizers), and the recovery of planted copy ratios with the search driven by the checker
(tests/ratio_checker.py).  (A plan cannot be made without a device, so what ed_plan_ratio_profile says about ROWS is asserted on the
host-only row_fault by the stand-alone program here and through the entry itself in tests/test_gpu_ratio.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ratio_checker as rc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
Q95 = 3.841458820694124          # chi^2_1 quantiles
Q999 = 10.827566170662733
PLANTED = (0.05, 0.5, 0.75, 1.5, 2.0)
SEED = 11
_CACHE = {}


def closed_form(fn):
    """an objective in the copy ratio as call_copy_number's `evaluate` takes it (doses in, values out)"""
    return lambda doses: fn(1.0 + np.asarray(doses) / 2.0)


def rows_of(n):
    from exomedepth_amd import CALL_DTYPE
    return np.zeros(n, dtype=CALL_DTYPE)


def test_copy_number_from_profile():
    from exomedepth_amd import COPY_RATIO_GRID, copy_number_from_profile
    r = np.array(COPY_RATIO_GRID)
    assert r.size == 16 and all(x in r for x in (0.5, 1.0, 1.5, 2.0)) and abs(r[0] - 0.05) < 1e-15 and np.all(np.diff(r) > 0)
    L = np.stack([-300.0 * (r - 0.5) ** 2,            # a heterozygous deletion
                  -300.0 * (r - 2.2) ** 2,            # beyond four copies: CN 4
                  np.zeros(16),                       # a tie of all five: the first
                  -300.0 * (r - 0.1) ** 2,            # nearly nothing left: CN 0
                  np.where(r == 1.5, np.nan, -r)])    # a hole at CN 3
    out = copy_number_from_profile(r, L)
    assert out["cn"].tolist() == [1, 4, 0, 0, 0] and out["log10_bf_cn"].shape == (5, 5)
    assert np.all(out["log10_bf_cn"][:, 2] == 0.0)
    want = np.log10(np.e) * (L[0][[0, 3, 7, 11, 15]] - L[0][7])
    assert np.array_equal(out["log10_bf_cn"][0], want)
    assert np.isnan(out["log10_bf_cn"][4, 3]) and not np.isnan(out["log10_bf_cn"][4, [0, 1, 2, 4]]).any()
    # per-row ratios, the copy numbers at other columns, one of them missing; a profile without the normal ratio says nothing
    rr = np.array([[2.0, 1.0, 0.5, 0.05], [1.0, 1.5, 0.7, 0.3]])
    out = copy_number_from_profile(rr, np.array([[5.0, 1.0, 2.0, 3.0], [0.0, -1.0, 9.0, 9.0]]))
    assert out["cn"].tolist() == [4, 2] and np.isnan(out["log10_bf_cn"][0, 3]) and np.isnan(out["log10_bf_cn"][1, [0, 1, 4]]).all()
    out = copy_number_from_profile([0.5, 1.5], [[1.0, 2.0]])
    assert out["cn"].tolist() == [-1] and np.isnan(out["log10_bf_cn"]).all()
    with pytest.raises(ValueError):
        copy_number_from_profile(r[:5], L)


def test_search_peak_on_a_grid_point_and_between_two():
    from exomedepth_amd import call_copy_number
    # 0.75 is a point of the first grid; 0.8 lies between two; the curvature 2 * 800 gives se = 1 / 40 and an interval of 1.96 se
    fit = call_copy_number([0, 1], [1], [2], rows_of(2), evaluate=closed_form(lambda r: 7.0 - 800.0 * (r - np.array([0.75, 0.8])[None, :]) ** 2))
    assert fit["trace"][0]["k"].tolist() == [5, 5] and fit["evaluations"] == 3
    half = np.sqrt(Q95) / 40.0
    for j, r0 in enumerate((0.75, 0.8)):
        assert abs(fit["ratio"][j] - r0) <= 1e-9 and abs(fit["ratio_se"][j] - 0.025) <= 1e-9
        assert abs(fit["ratio_lo"][j] - (r0 - half)) <= 2e-4 and abs(fit["ratio_hi"][j] - (r0 + half)) <= 2e-4
        assert fit["ratio_lo"][j] < fit["ratio"][j] < fit["ratio_hi"][j] and fit["informative"][j]
        # Lmax is the largest value evaluated: within the last grid's spacing (1 / 8 * (2 / 15)^2) of the vertex
        assert 0.0 <= 7.0 - fit["log_likelihood"][j] <= 800.0 * (0.125 * (2.0 / 15) ** 2) ** 2
    assert fit["cn"].tolist() == [1, 2]                      # 0.75 is as far from 0.5 as from 1: the first of the tie
    assert abs(fit["mosaic_gain"][0] - 2 * 800.0 * 0.25 ** 2) <= 1e-2 and abs(fit["mosaic_gain"][1] - 2 * 800.0 * 0.2 ** 2) <= 1e-2


def test_search_flat_monotone_and_nan():
    from exomedepth_amd import call_copy_number
    flat = call_copy_number([0, 1], [1], [2], rows_of(1), evaluate=closed_form(lambda r: np.zeros_like(r)))
    assert all(t["k"][0] == 0 for t in flat["trace"]) and not flat["informative"][0]
    assert flat["cn"][0] == 0 and flat["mosaic_gain"][0] == 0.0 and np.isnan(flat["ratio_se"][0])
    assert abs(flat["ratio_lo"][0] - 0.05) < 1e-15 and flat["ratio_hi"][0] == 2.0        # never crossed: the grid's range
    up = call_copy_number([0, 1], [1], [2], rows_of(1), evaluate=closed_form(lambda r: 30.0 * r))
    assert all(t["k"][0] == 15 for t in up["trace"]) and up["ratio"][0] == 2.0 and np.isnan(up["ratio_se"][0]) and up["ratio_hi"][0] == 2.0
    assert abs(up["ratio_lo"][0] - (2.0 - Q95 / 60.0)) <= 2e-3 and up["cn"][0] == 4 and up["mosaic_gain"][0] == 0.0 and up["informative"][0]
    down = call_copy_number([0, 1], [1], [2], rows_of(1), evaluate=closed_form(lambda r: -30.0 * r))
    assert abs(down["ratio"][0] - 0.05) < 1e-15 and abs(down["ratio_lo"][0] - 0.05) < 1e-15 and down["cn"][0] == 0

    def objective(poison):
        def f(doses):
            r = 1.0 + np.asarray(doses) / 2.0
            l = 5.0 - 400.0 * (r - np.array([0.5, 1.2, 1.5])[None, :]) ** 2
            if poison:
                l[:, 1] = np.nan
            return l
        return f
    clean = call_copy_number([0, 1], [1], [2], rows_of(3), evaluate=objective(False))
    dirty = call_copy_number([0, 1], [1], [2], rows_of(3), evaluate=objective(True))
    for k in ("ratio", "ratio_se", "ratio_lo", "ratio_hi", "mosaic_gain", "log_likelihood"):
        assert np.isnan(dirty[k][1]), k
        assert np.array_equal(dirty[k][[0, 2]], clean[k][[0, 2]]), k
    assert dirty["cn"].tolist() == [1, -1, 3] and np.isnan(dirty["log10_bf_cn"][1]).all() and dirty["informative"].tolist() == [True, False, True]
    late = call_copy_number([0, 1], [1], [2], rows_of(1), evaluate=lambda d: np.where(np.asarray(d) == -1.0, np.nan, -np.asarray(d) ** 2))
    assert np.isnan(late["ratio"][0]) and late["cn"][0] == -1 and not late["informative"][0]      # a NaN at any ratio evaluated
    with pytest.raises(ValueError):
        call_copy_number([0, 1], [1], [2], rows_of(1), rounds=0, evaluate=closed_form(lambda r: r))
    with pytest.raises(ValueError):
        call_copy_number([0, 1], [1], [2], rows_of(1), ratio_floor=0.5, evaluate=closed_form(lambda r: r))
    none = call_copy_number([0, 1], [1], [2], rows_of(0), evaluate=closed_form(lambda r: r))
    assert none["ratio"].shape == (0,) and none["log10_bf_cn"].shape == (0, 5)


def test_entries_refuse_before_they_need_a_device():
    from exomedepth_amd import _lib
    L = _lib.lib()
    one = np.zeros(1)
    for G in (0, 17, -1):
        assert L.ed_plan_ratio_profile(None, None, 0, None, None, 0, 1, None, None, None, G, None, None) == -1          # ED_ERR_INVALID
        assert ("G = %d is outside 1 .. 16" % G) in L.ed_last_error().decode()
        assert L.ed_batch_copy_call_ratio_profile(None, one.ctypes.data, G, one.ctypes.data, 1) == -1
        assert ("G = %d is outside 1 .. 16" % G) in L.ed_last_error().decode()
        assert L.ed_plan_ratio_profile_dd(None, None, 0, None, None, 0, 1, None, None, None, G, None, None, None) == -1   # ... with the tails
        assert ("G = %d is outside 1 .. 16" % G) in L.ed_last_error().decode()
        assert L.ed_batch_copy_call_ratio_profile_dd(None, one.ctypes.data, G, one.ctypes.data, one.ctypes.data, 1) == -1
        assert ("G = %d is outside 1 .. 16" % G) in L.ed_last_error().decode()
    assert L.ed_plan_ratio_profile_dd(None, None, 0, None, None, 0, 1, None, None, None, 16, None, None, None) == -1
    assert "NULL plan" in L.ed_last_error().decode()
    assert L.ed_plan_ratio_profile(None, None, 0, None, None, 0, 1, None, None, None, 16, None, None) == -1
    assert "NULL plan" in L.ed_last_error().decode()
    assert L.ed_batch_copy_call_ratio_profile(None, one.ctypes.data, 1, one.ctypes.data, 1) == -1
    assert L.ed_batch_call_ratio_ms(None, None) == -1 and L.ed_ratio_geometry(None) == -1
    geo = (C.c_int32 * 4)()
    assert L.ed_ratio_geometry(geo) == 0
    assert geo[0] >= 1 and 0 <= geo[1] <= 4 and geo[2] == 16 and geo[3] >= 1
    from exomedepth_amd import ratio_geometry
    assert ratio_geometry() == dict(zip(("seg_tiles", "narrow", "max_grid", "items_per_workgroup"), (int(v) for v in geo)))


def test_ratio_plan_checker(tmp_path):
    """tools/ratio_plan_check.cpp compiles with the host sanitizers and exits with 0: every exon of every row in exactly one item, segments
    in order, limits and bad rows refused"""
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "ratio_plan_check")
    # (the sanitizers' runtimes are linked statically: the stand-alone program carries them, nothing has to be first among the loaded libraries)
    subprocess.run([cc, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tools", "ratio_plan_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout


def recovery_case(oracle):
    """(planted ratios, rows, the checker-driven fit) -- computed once, shared, left unchanged"""
    if "fit" not in _CACHE:
        from exomedepth_amd import call_copy_number
        rng = np.random.default_rng(SEED)
        planted = np.repeat(PLANTED, 8)
        lengths = rng.integers(20, 41, planted.size)
        chrom_off, rows, test, ref, phi, expected = rc.draw_rows(planted, lengths, SEED + 1)
        keep = []
        fit = call_copy_number(chrom_off, None, None, rows, evaluate=rc.evaluator(oracle, rows, test, ref, phi, expected, keep=keep))
        _CACHE["fit"] = (planted, rows, fit, keep)
    return _CACHE["fit"]


def test_planted_ratios_are_recovered_with_the_checker(oracle):
    """40 rows of 20 - 40 exons drawn from the model at mixture_checker.draw's defaults (totals around 2 000, phi = 5e-4, expected 0.5),
    eight each at the copy ratios 0.05, 0.5, 0.75, 1.5 and 2: the planted ratio lies in the 95 % interval of at least 34 rows, cn is the
    planted copy number of every integer row, mosaic_gain is beyond the 0.999 quantile of chi^2_1 for the 0.75 rows and below it for at
    least 30 of the 32 others.  (The defaults' depth carries the conditions: the exon count was not raised.)"""
    planted, rows, fit, keep = recovery_case(oracle)
    assert fit["evaluations"] == 3 == len(keep) and fit["profile"].shape == (16, 40)
    inside = (fit["ratio_lo"] <= planted) & (planted <= fit["ratio_hi"])
    beyond = fit["mosaic_gain"] > Q999
    for j in range(40):
        print("row %2d planted %.2f  ratio %.4f [%.4f, %.4f] se %.4f  cn %d  mosaic_gain %8.2f%s" % (
            j, planted[j], fit["ratio"][j], fit["ratio_lo"][j], fit["ratio_hi"][j], fit["ratio_se"][j], fit["cn"][j], fit["mosaic_gain"][j],
            "" if inside[j] else "  <- outside"))
    assert np.all(fit["informative"]) and np.all(fit["ratio_lo"] <= fit["ratio"]) and np.all(fit["ratio"] <= fit["ratio_hi"])
    assert inside.sum() >= 34, inside.sum()
    whole = planted != 0.75
    want_cn = {0.05: 0, 0.5: 1, 1.5: 3, 2.0: 4}
    assert fit["cn"][whole].tolist() == [want_cn[r] for r in planted[whole]]
    assert np.all(beyond[~whole]) and (~beyond[whole]).sum() >= 30, (beyond[~whole], (~beyond[whole]).sum())
    assert np.all(fit["mosaic_gain"] >= 0.0)


def test_interface_declares_the_ratio_entries():
    from exomedepth_amd import _lib
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edratio.inc")).read()
    for sym in ("ed_plan_ratio_profile", "ed_batch_copy_call_ratio_profile", "ed_plan_ratio_profile_dd", "ed_batch_copy_call_ratio_profile_dd",
                "ed_batch_call_ratio_ms", "ed_ratio_geometry"):
        assert sym in names, sym
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT int %s\(" % sym, source), sym
    core = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    assert "k_ratio_profile" in source and '#include "edratio.inc"' in core and '#include "ed_ratio_plan.hpp"' in core
    import exomedepth_amd
    from exomedepth_amd import api
    for name in ("call_copy_number", "copy_number_from_profile", "ratio_geometry", "COPY_RATIO_GRID"):
        assert getattr(exomedepth_amd, name) is getattr(api, name) and name in exomedepth_amd.__all__
    assert callable(api.Plan.ratio_profile) and callable(api.Batch.call_ratio_profile) and callable(api.Batch.call_ratio_ms)
    import inspect
    assert inspect.signature(api.ExomeDepth.CallCNVs).parameters["copy_number"].default is False
