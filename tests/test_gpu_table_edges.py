"""The table-driven emission modes (csrc/edtab.inc: k_tab_stats / k_tab_stats_sm, tab_dims_of, k_tab_build<256> / <64>, k_emit_tab,
k_emit_tab_sm with emit_tail_share, k_tab_cold) swept over the edges of their tables, LDS windows, strict lists and work distribution.

The expectation is never a device result.  tests/table_edge_cases.py restates the table geometry on the host -- the shape parameters,
the subsampled statistics, tab_dims_of with its tail branch, tab_windows, the block map / SmGrid / chunk / wave / strict list of mode 2
-- and plants counts on every edge those give, per sample (tests/test_table_edges_host.py asserts the plants and their places on the
CPU).  Per case and per run (mode 1; mode 2 with layout 0, layout 1, layout 1 at 16 bits; overlap groups off, so that the one
emission launch is the restated one):
  1  table_dims and table_windows of every sample equal the restatement exactly;
  2  the not-served mask comes from the restated dims: n_cold_cells, n_samples_without_tables, n_cells_without_tables are exact, and in
     mode 2 cold_list_overflow > 0 exactly when the restated largest list load exceeds the list's slots;
  3  every not-served cell and every cell of a sample without tables carries the checker's PORTABLE bits (NaN for NaN); n_gsl_errors is
     the checker's count;
  4  every served cell is within spacing(D1) + spacing(D2) + spacing(D3) + spacing(want) of the host definition (oracle.dtab inside the
     tables or windows, oracle.dtab_tail beyond a tail sample's windows, oracle.dtab_combine of the three: the combination is the shared
     ed_dtab_combine, each input may sit one ulp off the sequential definition by the parallel scan's association), and >= 99.5 % of
     the served cells of a case are bit-equal;
  5  every served cell is within 1e-10 relative of the checker's LIBM flavour (no absolute floor); cells without reads are +0;
  6  pinned table lengths 1 024 ... 12 288 (on and just past the sweeps of both forms of k_tab_build): every entry within one ulp of
     oracle.dtab, at most 0.1 % differ at all;
  7  a 16-bit run equals its 32-bit run bit for bit wherever the counts are the same; layout 1 equals layout 0 bit for bit.
Further: the capacity of one strict list (a whole block, one more, one less, two workgroups on one list), a reused batch against a
fresh one, and case A through the cohort pipeline at 32 and 16 bits with its default overlap groups.

Measured on one MI355X (test_report, -s; also DESIGN.md 4.11).  Cases A - D together, per run: 35 697 planted cells; mode 1: 1 481 037
served, 124 963 not served, 261 000 cells of samples without tables; mode 2 (either layout): 1 463 370 / 142 630 / 261 000; at 16 bits
1 466 113 / 139 887 / 261 000.  Every served value was bit-equal to the host definition (largest deviation 0.000 of the bar of
assertion 4, share of bit-equal values 1.00000), in the small shapes, the capacity designs and the reused batch too; the largest relative
deviation from the LIBM flavour was 1.75e-11 (cases A, B, C1), 4.1e-13 in C0, 3.2e-13 in D.  The 405 792 table entries compared at the
pinned lengths, per S, were all bit-equal (0 differ, 0 ulp).  Restated dims and windows matched the device in every sample of every run.
Both outcomes of the strict lists occur among A - D (restated largest load / slots: C0 3 / 64, D 4 / 64; A 296 / 64, B 323 / 67,
C1 205 / 64: the flag and the full re-scan); the batch's default overlap groups made two emission launches in every case, the cohort ran
case A as one.  Wall time of the file 8.4 s, of which the checker 6.4 s; the slowest test (case B: 4 300 x 257 in five runs) 3.6 s.

Value-only mutants of csrc/edtab.inc (in-bounds reads, no store address changed), built aside and each run ONCE against this file:
  k_emit_tab_sm `idx[1] < nres[1]` -> `<=` (the ref look-up at n2 reads the first entry of the tot window): failed
      test_planted_edges[A], [B], [C0], [D] (the samples with n2 < Lr; C1 has none) and test_a_reused_batch_is_a_fresh_one;
  tab_cell_served `nref < Lr` -> `<=`: failed test_planted_edges (all five), 14 of the 15 small shapes (not 1 x 1, whose only cell is
      (63, 63)), test_a_reused_batch_is_a_fresh_one, test_case_A_through_the_cohort (both);
  tab_cell_served `obs >= N0` -> `>`: failed test_planted_edges[A], [B], [C1] (the cases with a finite N0),
      test_a_reused_batch_is_a_fresh_one, test_case_A_through_the_cohort (both);
  k_tab_build drops the running total after its first sweep: failed test_pinned_table_lengths[130] and [257], test_planted_edges
      (all five), test_a_reused_batch_is_a_fresh_one;
  the list test `at < per` -> `at < per - 1`: failed test_capacity_of_a_strict_list and nothing else.
"""
import time

import numpy as np
import pytest

import table_edge_cases as tc
from test_gpu_tables import bits, close_rel

pytestmark = pytest.mark.gpu

RUNS = (("mode 1", 1, 0, 32), ("mode 2, layout 0", 2, 0, 32), ("mode 2, layout 1", 2, 1, 32), ("mode 2, layout 1, 16 bits", 2, 1, 16))
_CACHE, _PLANS = {}, {}
T0 = [None]
CHECKER_SECONDS = [0.0]
REPORT = {}


def cached(key, make):
    if T0[0] is None:
        T0[0] = time.time()
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def get_case(oracle, name):
    make = {"A": tc.case_A, "A2": tc.case_A2, "B": tc.case_B, "C0": lambda o: tc.case_C(o, 0), "C1": lambda o: tc.case_C(o, 1), "D": tc.case_D}
    return cached(("case", name), lambda: make[name](oracle))


def plan_of(ed, case):
    key = (tuple(case["chrom_off"].tolist()), int(case["start"][0]) if case["E"] else 0)
    if key not in _PLANS:
        _PLANS[key] = ed.Plan(case["chrom_off"], case["start"], case["end"])
    return _PLANS[key]


def checker(oracle, case, bits_):
    """per sample the checker's PORTABLE matrix, its error count and the LIBM matrix, for the 32-bit or the 16-bit counts (computed once)"""
    def make():
        t0 = time.time()
        test, ref = (case["test"], case["ref"]) if bits_ == 32 else (case["test16"], case["ref16"])
        base = _CACHE.get(("checker", case["name"], 32)) if bits_ == 16 else None
        E, S = case["E"], case["S"]
        port = np.empty((E, 3, S)); libm = np.empty((E, 3, S)); nerr = np.zeros(S, dtype=np.int64)
        for s in range(S):
            if base is not None and np.array_equal(test[:, s], case["test"][:, s]) and np.array_equal(ref[:, s], case["ref"][:, s]):
                port[:, :, s], libm[:, :, s], nerr[s] = base[0][:, :, s], base[1][:, :, s], base[2][s]
                continue
            port[:, :, s], nerr[s] = oracle.get_loglike_matrix(case["phi"][s], case["p"][s], test[:, s] + ref[:, s], test[:, s], 1.0, oracle.PORTABLE)
            libm[:, :, s], _ = oracle.get_loglike_matrix(case["phi"][s], case["p"][s], test[:, s] + ref[:, s], test[:, s], 1.0, oracle.LIBM)
        CHECKER_SECONDS[0] += time.time() - t0
        return port, libm, nerr
    return cached(("checker", case["name"], bits_), make)


def definition(oracle, case, tails, caps=None):
    """[E][3][S] host definition of the served cells and its bar (NaN where a cell is not served), for the 32-bit counts"""
    def make():
        t0 = time.time()
        dims, wins, shapes = case["pre"][tails]
        other = _CACHE.get(("definition", case["name"], 1 - tails))
        E, S = case["E"], case["S"]
        want = np.full((E, 3, S), np.nan); bar = np.full((E, 3, S), np.nan)
        for s in range(S):
            if other is not None and dims[s] == case["pre"][1 - tails][0][s] and wins[s] == case["pre"][1 - tails][1][s]:
                want[:, :, s], bar[:, :, s] = other[0][:, :, s], other[1][:, :, s]      # (only a tail sample differs between the modes)
                continue
            ok = tc.served_mask(case["test"][:, s], case["ref"][:, s], dims[s])
            want[ok, :, s], bar[ok, :, s] = tc.host_definition(oracle, shapes[s], case["test"][ok, s], case["ref"][ok, s], wins[s])
        CHECKER_SECONDS[0] += time.time() - t0
        return want, bar
    return cached(("definition", case["name"], tails), make)


def same_or_both_nan(got, want):
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def run_batch(ed, case, mode, layout, bits_, caps=None, tails=None, overlap=0, batch=None):
    plan = plan_of(ed, case)
    b = batch if batch is not None else ed.Batch(plan, case["S"])
    if batch is None:
        b.set_viterbi_overlap(overlap)
        if caps is not None:
            b.set_emit_mode(mode, cap_obs=caps[0], cap_ref=caps[1], reach=caps[2], tails=tails)
        else:
            b.set_emit_mode(mode, tails=tails)
        b.set_counts_layout(layout)
        if bits_ == 16:
            b.set_counts_bits(16)
    test, ref = (case["test"], case["ref"]) if bits_ == 32 else (case["test16"], case["ref16"])
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    if bits_ == 16:
        test, ref = test.astype(np.uint16), ref.astype(np.uint16)
    b.run(test, ref, case["phi"], case["p"])
    return b


def check_run(oracle, case, b, mode, bits_, full=True, single_launch=True, caps=None, tails=None):
    """assertions 1 - 5 of one run; returns its likelihood matrix and the figures of the report"""
    S, E = case["S"], case["E"]
    t = (1 if mode == 2 else 0) if tails is None else tails
    dims, wins, _ = case["pre"][t]
    test, ref = (case["test"], case["ref"]) if bits_ == 32 else (case["test16"], case["ref16"])
    # 1
    got_d = [b.table_dims(s) for s in range(S)]
    got_w = [b.table_windows(s) for s in range(S)]
    bad = [(s, case["kinds"][s], got_d[s], dims[s], got_w[s], wins[s]) for s in range(S) if got_d[s] != dims[s] or got_w[s] != wins[s]]
    assert not bad, "dims / windows (sample, kind, device, restated): %s" % bad[:4]
    # 2
    notab = np.array([d[0] == 0 for d in dims])
    served = np.stack([tc.served_mask(test[:, s], ref[:, s], dims[s]) for s in range(S)], axis=1)
    cold = ~served & ~notab[None, :]
    st = b.table_stats()
    assert st["n_cold_cells"] == int(cold.sum()) == b.n_cold_cells(), (st, int(cold.sum()))
    assert st["n_samples_without_tables"] == int(notab.sum()) and st["n_cells_without_tables"] == int(notab.sum()) * E, st
    if mode == 2 and single_launch:
        assert b.n_emit_launches == 1
        loads = case["geo"].list_loads(cold)
        per = tc.cold_cap_per(E, S)
        assert (st["cold_list_overflow"] > 0) == bool(loads.max() > per), (st, int(loads.max()), per)
        max_load = "%d of %d" % (loads.max(), per)
    else:
        max_load = None
    # 3
    port, libm, nerr = checker(oracle, case, bits_)
    ll = b.loglik()
    sel = np.broadcast_to(~served[:, None, :], ll.shape)
    ok = same_or_both_nan(ll[sel], port[sel])
    assert ok.all(), "not served: %d values differ from the checker's bits, first (exon, state, sample) %s" % ((~ok).sum(), np.argwhere(sel & ~same_or_both_nan(ll, port))[:4].tolist())
    assert b.n_gsl_errors() == int(nerr.sum()), (b.n_gsl_errors(), int(nerr.sum()))
    # 5
    sv = ~sel
    ok = close_rel(ll, libm) | sel
    assert ok.all(), "served: beyond 1e-10 of the LIBM flavour at (exon, state, sample) %s" % [(e, q, s, int(test[e, s]), int(ref[e, s]), case["kinds"][s]) for e, q, s in np.argwhere(~ok)[:4].tolist()]
    empty = np.broadcast_to(((test + ref) == 0)[:, None, :], ll.shape) & sv
    assert (ll[empty] == 0).all() and not np.signbit(ll[empty]).any()
    nz = sv & (libm != 0) & np.isfinite(libm)
    fig = dict(served=int(served.sum()), cold=int(cold.sum()), notab=int(notab.sum()) * E, planted=int(case["planted"].sum()) if "planted" in case else 0,
               rel=float(np.max(np.abs(ll[nz] - libm[nz]) / np.abs(libm[nz]))) if nz.any() else 0.0, frac=0.0, equal=1.0, max_load=max_load)
    # 4
    if full and bits_ == 32:
        want, bar = definition(oracle, case, t)
        assert np.array_equal(np.isnan(want), sel)
        dev = np.abs(ll[sv] - want[sv])
        over = dev > bar[sv]
        assert not over.any(), "served: beyond the bar of the host definition at (exon, state, sample) %s" % np.argwhere(sv & (np.abs(ll - want) > bar))[:4].tolist()
        fig["frac"] = float(np.max(dev / bar[sv]))
        fig["equal"] = float(np.mean(bits(ll[sv]) == bits(want[sv])))
        assert fig["equal"] >= 0.995, fig
    return ll, fig


def note(case, run, fig):
    REPORT[(case, run)] = fig


@pytest.mark.parametrize("name", ["A", "B", "C0", "C1", "D"])
def test_planted_edges(edlib, oracle, name):
    """cases A - D in every run; assertion 7 between the runs"""
    case = get_case(oracle, name)
    lls = {}
    for run, mode, layout, bits_ in RUNS:
        b = run_batch(edlib, case, mode, layout, bits_)
        lls[run], fig = check_run(oracle, case, b, mode, bits_)
        note(name, run, fig)
        b.close()
    assert np.array_equal(bits(lls["mode 2, layout 1"]), bits(lls["mode 2, layout 0"]))
    # the batch's default overlap groups (one emission launch and one strict pass per group, the lists zeroed in between): the same bits, the
    # not-served cells summed over the groups
    b = run_batch(edlib, case, 2, 1, 32, overlap=1)
    ll_g, fig = check_run(oracle, case, b, 2, 32, full=False, single_launch=False)
    note(name, "mode 2, layout 1, overlap groups (%d launches)" % b.n_emit_launches, fig)
    b.close()
    assert np.array_equal(bits(ll_g), bits(lls["mode 2, layout 1"]))
    common = np.broadcast_to(((case["test"] == case["test16"]) & (case["ref"] == case["ref16"]))[:, None, :], lls["mode 1"].shape)
    assert common.sum() < common.size and common.mean() > 0.99              # the 16-bit run holds a subset of the plants
    assert np.array_equal(bits(lls["mode 2, layout 1, 16 bits"][common]), bits(lls["mode 2, layout 1"][common]))
    if name == "A":
        _CACHE[("ll", "A", 32)], _CACHE[("ll", "A", 16)] = lls["mode 2, layout 1"], lls["mode 2, layout 1, 16 bits"]


@pytest.mark.parametrize("E,S", tc.SMALL_SHAPES)
def test_small_shapes_with_pinned_lengths(edlib, oracle, E, S):
    """E around one block, S around the tile widths; Ly = Lr = 64 by the caps whatever is planted, plants at 63 / 64 / 65"""
    case = cached(("case", "small", E, S), lambda: tc.case_small(oracle, E, S))
    lls = {}
    for run, mode, layout, bits_ in RUNS:
        b = run_batch(edlib, case, mode, layout, bits_, caps=tc.SMALL_CAPS, tails=0)
        lls[run], fig = check_run(oracle, case, b, mode, bits_, tails=0)
        note("small", (run, E, S), fig)
        b.close()
    assert np.array_equal(bits(lls["mode 2, layout 1"]), bits(lls["mode 2, layout 0"]))
    assert np.array_equal(bits(lls["mode 2, layout 1, 16 bits"]), bits(lls["mode 2, layout 1"]))      # (nothing here exceeds 16 bits)
    assert np.array_equal(case["test"], case["test16"]) and np.array_equal(case["ref"], case["ref16"])


@pytest.mark.parametrize("S", [130, 257])
def test_pinned_table_lengths(edlib, oracle, S):
    """k_tab_build<256> (S = 130) and <64> (S = 257) at table lengths on and just past their sweeps of 4 096 and 1 024 entries: every entry of
    samples 0, S / 2 and S - 1 within one ulp of the sequential definition, at most 0.1 % of them different at all"""
    n_diff = n_all = 0
    worst = 0.0
    for caps in tc.PINNED_CAPS:
        case = cached(("case", "pinned", S, caps), lambda: tc.case_pinned(oracle, S, caps))
        b = run_batch(edlib, case, 1, 0, 32, caps=case["caps"], tails=0)
        dims, wins, shapes = case["pre"][0]
        for s in (0, S // 2, S - 1):
            assert b.table_dims(s) == dims[s] and dims[s][:2] == caps, (s, b.table_dims(s), dims[s])
            ly, lr, t1, t2, t3 = b.emit_tables(s)
            assert (ly, lr) == caps and t1.shape[0] == ly and t2.shape[0] == lr and t3.shape[0] == ly + lr
            a1, a2 = shapes[s]
            for st in range(3):
                for tab, x0 in ((t1, a1[st]), (t2, a2[st]), (t3, a1[st] + a2[st])):
                    t0 = time.time()
                    want = oracle.dtab(x0, tab.shape[0])
                    CHECKER_SECONDS[0] += time.time() - t0
                    d = bits(tab[:, st]) != bits(want)
                    n_diff += int(d.sum()); n_all += d.size
                    ulp = np.abs(tab[:, st] - want) / np.spacing(np.abs(want))
                    assert np.all(ulp <= 1.0), (caps, s, st, tab.shape[0], int(np.argmax(ulp)), float(ulp.max()))
                    worst = max(worst, float(ulp.max()))
        b.close()
    assert n_diff <= n_all // 1000, (n_diff, n_all)
    REPORT[("pinned", S)] = dict(entries=n_all, differ=n_diff, worst_ulp=worst)


def test_capacity_of_a_strict_list(edlib, oracle):
    """mode 2, one sample, one launch, 64 slots per list: a whole block of not-served cells fills its list exactly and does not raise the flag,
    one more cell in the next block the same wave takes does; 63 cells do not; two waves of different workgroups that share a list, together at
    64 and at 65.  Every assertion of a run holds in all of them (a raised flag means the full re-scan, which must give the same bits)."""
    base, designs = cached("capacity", lambda: tc.capacity_designs(oracle))
    for layout in (1, 0):
        for name, (t, r, load, over) in designs.items():
            case = dict(base, name="capacity_" + name, test=t, ref=r, test16=t, ref16=r, kinds=[("table",)], planted=~tc.served_mask(t, r, base["dims"]),
                        pre={1: ([base["dims"]], [base["win"]], [tc.shape_params(base["phi"][0], base["p"][0])])})
            b = run_batch(edlib, case, 2, layout, 32)
            assert b.n_emit_launches == 1
            ll, fig = check_run(oracle, case, b, 2, 32, full=(layout == 1))
            st = b.table_stats()
            assert fig["cold"] == load and (st["cold_list_overflow"] > 0) == over, (name, st, load)
            if name == "whole_block_plus_one":
                assert st["cold_list_overflow"] >= 1
            note("capacity", (name, layout), fig)
            b.close()
            for k in [k for k in _CACHE if isinstance(k, tuple) and len(k) > 1 and k[1] == case["name"]]:
                del _CACHE[k]


def test_a_reused_batch_is_a_fresh_one(edlib, oracle):
    """one batch run with case A's plants, then with case A2's (other positions, the sample kinds moved on: other samples are tail samples or
    have no tables): what a fresh batch gives, bit for bit, statistics included"""
    a, a2 = get_case(oracle, "A"), get_case(oracle, "A2")
    b = run_batch(edlib, a, 2, 1, 32)
    check_run(oracle, a, b, 2, 32, full=False)
    run_batch(edlib, a2, 2, 1, 32, batch=b)
    ll, fig = check_run(oracle, a2, b, 2, 32)
    note("A2", "mode 2, layout 1 (reused batch)", fig)
    f = run_batch(edlib, a2, 2, 1, 32)
    assert np.array_equal(bits(ll), bits(f.loglik()))
    assert b.table_stats() == f.table_stats() and b.n_gsl_errors() == f.n_gsl_errors()
    assert [b.table_dims(s) for s in range(a["S"])] == [f.table_dims(s) for s in range(a["S"])]
    assert [b.table_windows(s) for s in range(a["S"])] == [f.table_windows(s) for s in range(a["S"])]
    assert np.array_equal(b.path(), f.path()) and np.array_equal(b.calls(), f.calls())
    b.close(); f.close()


@pytest.mark.parametrize("bits_", [32, 16])
def test_case_A_through_the_cohort(edlib, oracle, bits_):
    """case A's slab through the cohort pipeline (emit mode 2, sample-major counts, its default overlap groups): the batch's likelihood bits;
    n_cold_cells is summed over the groups' launches"""
    ed = edlib
    case = get_case(oracle, "A")
    S = case["S"]
    want = _CACHE.get(("ll", "A", bits_))
    if want is None:
        b = run_batch(ed, case, 2, 1, bits_)
        want = b.loglik(); b.close()
    test, ref = (case["test"], case["ref"]) if bits_ == 32 else (case["test16"], case["ref16"])
    dt = np.uint16 if bits_ == 16 else np.int32
    tt, rt = np.ascontiguousarray(test.T.astype(dt)), np.ascontiguousarray(ref.T.astype(dt))
    co = ed.Cohort(plan_of(ed, case), S, 2, emit_mode=2, counts_layout=1, counts_bits=bits_)
    hold = [ed.DeviceArray(tt), ed.DeviceArray(rt), ed.DeviceArray(case["phi"]), ed.DeviceArray(case["p"])]
    tk = co.submit(hold[0], hold[1], phi=hold[2], expected=hold[3], n_samples=S)
    got = co.results(tk, S, loglik=True)
    assert np.array_equal(bits(got["loglik"]), bits(want))
    b, _, _ = co.batch(tk)
    dims = case["pre"][1][0]
    cold = sum(int((~tc.served_mask(test[:, s], ref[:, s], dims[s])).sum()) for s in range(S) if dims[s][0] > 0)
    st = b.table_stats()
    assert st["n_cold_cells"] == cold and st["n_samples_without_tables"] == sum(d[0] == 0 for d in dims), (st, cold, co.n_emit_launches)
    assert [b.table_dims(s) for s in range(S)] == dims
    REPORT[("cohort", bits_)] = dict(launches=co.n_emit_launches, cold=cold)
    co.close()


def test_report():
    """the figures quoted in DESIGN.md 4.11 (printed with -s)"""
    print()
    for run, _, _, _ in RUNS:
        figs = [f for (c, r), f in REPORT.items() if c in ("A", "B", "C0", "C1", "D") and r == run]
        if figs:
            print("%-26s cases A - D: planted %d, served %d, not served %d (+ %d of samples without tables); largest deviation %.3f of the bar of "
                  "assertion 4, %.2e relative of LIBM; bit-equal %.5f" % (run, sum(f["planted"] for f in figs), sum(f["served"] for f in figs), sum(f["cold"] for f in figs),
                                                                         sum(f["notab"] for f in figs), max(f["frac"] for f in figs), max(f["rel"] for f in figs),
                                                                         min(f["equal"] for f in figs)))
    for key, f in sorted(REPORT.items(), key=str):
        print(key, f)
    wall = time.time() - T0[0]
    print("wall time of the file %.1f s, of which the checker %.1f s (%.0f %%)" % (wall, CHECKER_SECONDS[0], 100.0 * CHECKER_SECONDS[0] / wall))
    assert any(k[0] == "A" for k in REPORT)
    for p in _PLANS.values():
        p.close()
    _PLANS.clear(); _CACHE.clear()
