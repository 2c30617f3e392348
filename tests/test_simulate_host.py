"""Draws from the fitted model without a GPU: the checker's Philox against the published vectors and against csrc/ed_philox.hpp compiled
as it is, the checker's draw against the 40-digit quantile and a scipy inversion, false_calls_per_sample against a double loop, the
interface's declarations, tools/philox_check.cpp under the host sanitizers, and the planted case the GPU pipeline test calls."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quantile_checker as qc  # noqa: E402
import simulate_checker as sc  # noqa: E402

TOTALS = (0, 1, 2, 3, 5, 63, 64, 255, 256, 257, 511, 512, 513, 1025, 4099)
PHIS = (1e-5, 0.003, 0.05, 0.2)
EXPECTED = (0.05, 0.11, 0.4)
CC = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
TOOL = os.path.join(ROOT, "tools", "philox_check.cpp")


def test_checker_philox_reproduces_the_known_answers():
    for counter, key, want in sc.KNOWN:
        assert sc.philox4x32_10(counter, key) == want
    assert sc.u53_of(0) == 2.0 ** -53 and sc.u53_of(2 ** 52 - 1) == 1.0 - 2.0 ** -53
    # key = (seed & 0xffffffff, seed >> 32), counter = (exon, sample, replicate, stream)
    w = sc.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert sc.u53(0x299f31d0a4093822, 0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344) == sc.u53_of(((w[0] >> 12) << 32) | w[1])


def test_header_philox_equals_the_checker(tmp_path):
    """csrc/ed_philox.hpp compiled plainly (tools/philox_check.cpp --emit) against the checker on 10 000 counters: exons at and above 2^31
    given as unsigned, seeds above 2^32, every word and the uniform's bits"""
    exe = str(tmp_path / "philox_emit")
    subprocess.run([CC, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", TOOL, "-o", exe, "-lstdc++", "-lm"], check=True)
    rng = np.random.default_rng(11)
    n = 10000
    seed = rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)
    seed[::7] = rng.integers(0, 2 ** 32, size=len(seed[::7]), dtype=np.uint64)
    seed[1::7] |= np.uint64(1) << np.uint64(63)
    exon = rng.integers(0, 2 ** 32, size=n, dtype=np.uint64)
    exon[::3] |= np.uint64(1) << np.uint64(31)
    exon[:4] = (0, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1)
    sample = rng.integers(0, 2 ** 20, size=n, dtype=np.uint64)
    rep = rng.integers(0, 1000, size=n, dtype=np.uint64)
    stream = rng.integers(0, 2, size=n, dtype=np.uint64)
    assert int(seed.max()) > 2 ** 32 and int(exon.max()) >= 2 ** 31
    text = "".join("%d %d %d %d %d\n" % t for t in zip(seed.tolist(), exon.tolist(), sample.tolist(), rep.tolist(), stream.tolist()))
    r = subprocess.run([exe, "--emit"], input=text, capture_output=True, text=True, check=True)
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == n
    for i, line in enumerate(lines):
        got = [int(t, 16) for t in line.split()]
        sd = int(seed[i])
        want = sc.philox4x32_10((int(exon[i]), int(sample[i]), int(rep[i]), int(stream[i])), (sd & sc.MASK, sd >> 32))
        assert tuple(got[:4]) == want, i
        u = sc.u53(sd, int(exon[i]), int(sample[i]), int(rep[i]), int(stream[i]))
        assert got[4] == int(np.float64(u).view(np.uint64)), i
        assert 2.0 ** -53 <= u <= 1.0 - 2.0 ** -53


def test_philox_check_under_the_host_sanitizers(tmp_path):
    """tools/philox_check.cpp, a stand-alone host program, built with -fsanitize=address,undefined and run: the three vectors, the edges of
    the uniform, the loop against straight-line rounds.  (The runtimes are linked into the program where the compiler has them as
    archives, so that the program does not depend on the order in which shared libraries are loaded.)"""
    exe = str(tmp_path / "philox_check")
    base = [CC, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", TOOL, "-o", exe, "-lstdc++", "-lm"]
    if subprocess.run(base + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "checks passed" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


@pytest.mark.parametrize("phi", PHIS)
def test_checker_draw_is_the_quantile_cut_and_agrees_with_scipy(phi):
    """The checker's draw is quantile_checker.quantile(...)'s cut at 40 digits (n where nothing crosses); it agrees with the inversion of
    scipy.stats.betabinom.cdf wherever u is further than 2e-9 -- the bar tests/test_quantile_host.py holds scipy to -- from a step."""
    rng = np.random.default_rng(3)
    n_cmp = n_near = 0
    for e in EXPECTED:
        a, b = sc.shapes(phi, e)
        for n in TOTALS:
            us = [sc.u53(77, k, n, 0) for k in range(6)] + [2.0 ** -53, 1.0 - 2.0 ** -53, float(rng.uniform())]
            for u in us:
                x = sc.draw(n, a, b, u)
                _, _, cut = qc.quantile(n, a, b, u)
                assert x == (cut if cut is not None else n) and 0 <= x <= n
                if n == 0:
                    assert x == 0
                    continue
                with qc.mp.workdps(qc.DPS):                     # the definition itself: C(x - 1) <= u < C(x), or nothing crosses
                    assert sc.C_at(n, a, b, x - 1) <= u and (sc.C_at(n, a, b, x) > u or x == n)
                d, _ = sc.step_distance(n, a, b, u)
                if d > 2e-9:
                    assert sc.scipy_draw(n, a, b, u) == x, (phi, e, n, u)
                    n_cmp += 1
                else:
                    n_near += 1
    print("phi = %g: %d draws compared with scipy, %d within 2e-9 of a step" % (phi, n_cmp, n_near))
    assert n_cmp > 300


def test_judge_takes_the_draw_and_refuses_its_neighbours():
    a, b = sc.shapes(0.05, 0.11)
    n = 257
    pm, C = qc.dist(n, a, b)
    u = float(C[29] + pm[30] / 2)
    assert sc.draw(n, a, b, u) == 30
    assert sc.judge(30, n, a, b, u)[0] == 0.0
    assert sc.judge(29, n, a, b, u)[0] > 1e6 and sc.judge(31, n, a, b, u)[0] > 1e6
    # on a step either neighbour is within the bar
    us = float(C[30])
    assert sc.judge(30, n, a, b, us)[0] <= 1.0 and sc.judge(31, n, a, b, us)[0] <= 1.0
    assert sc.judge(n, n, a, b, 1.0 - 2.0 ** -53)[0] <= 1.0
    # (a uniform has to lie inside [0, 1): C(0) - 4 bar does at n = 257, C(255) + 4 bar at n = 600)
    names = [t[0] for t in sc.planted_uniforms(n, a, b)] + [t[0] for t in sc.planted_uniforms(600, *sc.shapes(0.003, 0.4))]
    for want in ("smallest", "largest", "C(0) -4 bar", "C(255) +4 bar", "C(256) -4 bar", "two in one value", "adjacent values of one lane",
                 "adjacent values of two lanes"):
        assert want in names, want


def test_false_calls_per_sample_against_the_double_loop():
    import exomedepth_amd as ed
    rng = np.random.default_rng(9)
    null_bf = np.round(rng.gamma(2.0, 4.0, 500), 1)             # rounded: ties within the null and with the real calls
    null_kind = rng.integers(1, 3, 500)
    bf = np.concatenate([null_bf[:40], np.round(rng.gamma(2.0, 6.0, 60), 1), [0.0, 1e9, -5.0]])
    kind = rng.integers(1, 3, bf.size)
    got = ed.false_calls_per_sample(bf, null_bf, 120)
    assert np.array_equal(got, sc.false_calls_loop(bf, null_bf, 120))
    got = ed.false_calls_per_sample(bf, null_bf, 120, kind, null_kind)
    assert np.array_equal(got, sc.false_calls_loop(bf, null_bf, 120, kind, null_kind))
    assert got.max() > 0 and got[-2] == 0.0
    assert np.sum(np.isin(bf, null_bf)) >= 40                   # ties are there
    # a type the null table does not hold; an empty null table; NaN
    only_del = null_kind == 1
    got = ed.false_calls_per_sample(bf, null_bf[only_del], 120, kind, null_kind[only_del])
    assert np.array_equal(got, sc.false_calls_loop(bf, null_bf[only_del], 120, kind, null_kind[only_del])) and np.all(got[kind == 2] == 0)
    assert np.array_equal(ed.false_calls_per_sample(bf, [], 7), np.zeros(bf.size))
    assert np.array_equal(ed.false_calls_per_sample(bf, [], 7, kind, []), np.zeros(bf.size))
    assert ed.false_calls_per_sample([], null_bf, 7).size == 0
    got = ed.false_calls_per_sample([np.nan, 3.0], [np.nan, 3.0, 4.0], 2)
    assert np.isnan(got[0]) and got[1] == 1.0
    with pytest.raises(ValueError):
        ed.false_calls_per_sample(bf, null_bf, 0)
    with pytest.raises(ValueError):
        ed.false_calls_per_sample(bf, null_bf, 5, kind, None)


def test_interface_declares_the_simulate_entries():
    from exomedepth_amd import _lib
    import ctypes as C
    names = {n for n, _, _ in _lib.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    source = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edsim.inc")).read()
    L = C.CDLL(_lib.LIB_PATH)
    for sym in ("ed_runif53", "ed_rbetabinom_ab_u", "ed_plan_simulate", "ed_plan_simulate_cells", "ed_sim_stats", "ed_sim_geometry"):
        assert sym in names, sym
        assert re.search(r"\bint %s\(" % sym, header), sym
        assert re.search(r"ED_EXPORT int %s\(" % sym, source), sym
        assert hasattr(L, sym), sym
    core = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edcore.hip")).read()
    assert '#include "edsim.inc"' in core and '#include "ed_philox.hpp"' in core
    for k in ("k_sim_walk", "k_sim_points", "k_sim_count", "k_sim_fill"):
        assert re.search(r"^%s\(" % k, source, flags=re.M), k
    for k in ("k_pw_scan", "k_pw_mark", "k_pw_rank", "k_pw_jobs", "k_pw_slots", "k_annot_scan_block"):      # used, not copied
        assert not re.search(r"^%s\(" % k, source, flags=re.M), k
    assert "pw_occupy(" in source and "k_annot_scan_block" in source
    # the CDF walk and the samples' shapes are the shared core's (edtotals.inc, in front of the three maps): used here, not restated
    totals = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "edtotals.inc")).read()
    assert core.index('#include "edtotals.inc"') < core.index('#include "edsim.inc"')
    for k, ret in (("bb_open", "BbWalk"), ("bb_step", "BbTile"), ("sim_shapes", "int64_t")):
        assert len(re.findall(r"^(?:__device__ __forceinline__ )?%s %s\(" % (ret, k), totals, flags=re.M)) == 1, k
        assert not re.search(r"^(?:__device__ __forceinline__ )?%s %s\(" % (ret, k), source, flags=re.M) and k + "(" in source, k
    assert "frcp((xd + 1.0) * (b + rest))" not in source and totals.count("frcp((xd + 1.0) * (b + rest))") == 1
    hdr = open(os.path.join(ROOT, "exomedepth_amd", "csrc", "ed_philox.hpp")).read()
    assert "#include <hip" not in hdr and "0xD2511F53" in hdr and "0xCD9E8D57" in hdr and "0x9E3779B9" in hdr and "0xBB67AE85" in hdr
    import exomedepth_amd
    from exomedepth_amd import api
    for name in ("runif53", "rbetabinom", "rbetabinom_ab", "rbetabinom_ab_u", "sim_geometry", "null_call_table", "false_calls_per_sample"):
        assert getattr(exomedepth_amd, name) is getattr(api, name) and name in exomedepth_amd.__all__
    assert callable(api.Plan.simulate) and callable(api.ExomeDepth.null_calls)
    g = api.sim_geometry()
    assert g["chunk"] == 64 and g["walk_tile"] == 256 and g["max_total"] == api.quantile_geometry()["max_total"]


def test_planted_case_is_called_by_the_cpu_restatement(oracle):
    """The case tests/test_gpu_simulate.py plants -- a 12-exon row at totals near 900, ratio 0.5, in four samples -- on the CPU: the
    checker's draws and the oracle's CallCNVs call a deletion over the row in every one of the replicates, and no uniform of the input
    lies within the bar of a step (so the device has one right draw per cell).  Seed: simulate_checker.PLANT_SEED, the first one tried."""
    case = sc.planted_case()
    rows = case[7]
    assert sc.PLANT_LAST - sc.PLANT_FIRST + 1 == 12 and len(rows) == 4
    tot = case[3] + case[4]
    assert tot.min() >= 880 and tot.max() <= 920
    for r in range(sc.PLANT_REPLICATES):
        calls, nearest = sc.cpu_calls(case, oracle, sc.PLANT_SEED, r, sc.PLANT_SAMPLES)
        assert nearest > 1.0, nearest
        for s in sc.PLANT_SAMPLES:
            hit = [c for c in calls[s] if c[2] == 1 and c[0] <= sc.PLANT_FIRST and c[1] >= sc.PLANT_LAST]
            assert len(hit) == 1, (r, s, calls[s])
            assert hit[0][0] >= sc.PLANT_FIRST - 1 and hit[0][1] <= sc.PLANT_LAST + 1, (r, s, hit)
