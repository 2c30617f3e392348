"""The histogram form of the dispersion fit (csrc/edfit_hist.inc: k_fit_hist, k_fit_hist_sm, k_fit_hnewton, k_fit_hnm; geometries 8, 4, 2)
with counts placed ON its edges: the last bin of each level and the first value beyond it, lists at and one past their capacity, rows on
both sides of every chunk, half, span and block boundary, bins at 16 383 / 16 384 / 64 511 and 128 / 129 early movers, batch widths around
the 4-sample Newton workgroup and the 8 / 4 / 2-sample histogram workgroup, batch depths on both sides of the automatic geometry's thresholds,
and columns with nothing to fit.  The catalogue is tests/fit_hist_cases.py; tests/test_fit_hist_cases_host.py shows on the CPU that every
column is well conditioned and that the checker's MLE of it moves by more than 1000 bars under an off-by-one bin, a lost cell or a run of
rows counted twice.

Every held column is compared with the checker's maximum-likelihood fit on sufficient statistics (oracle.fit_mle_hist) at FIT_REL_TOL, scaled
by _check_mle of tests/test_gpu_fit_invariance.py; group D (columns on a few values) at the bar of
tests/test_gpu_fit.py::test_sample_major_histograms_with_bins_that_leave_the_lds_early; fit mode 1 with oracle.fit_nm at the bars of
tests/test_gpu_fit_concordance.py.  No bar is new."""
import numpy as np
import pytest

import fit_hist_cases as fc
from test_gpu_fit_invariance import FIT_REL_TOL, _check_mle, _plan, _same_bits

pytestmark = pytest.mark.gpu

HOT_BARS = (1e-6, 1e-8)      # test_sample_major_histograms_with_bins_that_leave_the_lds_early: phi, expected
NM_BARS = (2e-3, 2e-4)       # test_gpu_fit_concordance.py: phi, p
REPORT = {}                  # group -> [columns held, largest deviation in bars]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------

class _HistChecker:
    """oracle.fit_mle_hist under the name _check_mle calls (the same estimator on sufficient statistics), one call per distinct column"""

    def __init__(self, oracle):
        self.oracle, self.seen = oracle, {}

    def fit_mle(self, y, r):
        y, r = np.ascontiguousarray(y, dtype=np.int32), np.ascontiguousarray(r, dtype=np.int32)
        key = (y.size, hash(y.tobytes()), hash(r.tobytes()))
        if key not in self.seen:
            self.seen[key] = self.oracle.fit_mle_hist(y, r)
        return self.seen[key]


_CHECKER = {}


def _checker(oracle):
    return _CHECKER.setdefault("c", _HistChecker(oracle))


def _batch(edlib, case, mode=0):
    plan = _plan(edlib, case.E)
    b = edlib.Batch(plan, case.S)
    if case.layout:
        b.set_emit_mode(2); b.set_counts_layout(1)
        if case.bits == 16:
            b.set_counts_bits(16)
    b.set_fit_histograms(case.g)
    if mode:
        from exomedepth_amd._lib import check, lib
        check(lib().ed_batch_set_fit_mode(b.handle, mode))
    return plan, b


def _fit_on(edlib, b, case):
    t, r = case.matrices()
    dphi, dexp = edlib.DeviceArray(np.zeros(case.S)), edlib.DeviceArray(np.zeros(case.S))
    b.fit(edlib.DeviceArray(t), edlib.DeviceArray(r), dphi, dexp, by=case.by)
    nu = b.fit_unconverged()[0]
    return dphi.to_host(), dexp.to_host(), nu


def _fit(edlib, case, mode=0, repeats=1):
    """(phi, expected, unconverged) of the case on a fresh batch; repeats > 1: a list, the same batch fitting again"""
    plan, b = _batch(edlib, case, mode)
    out = [_fit_on(edlib, b, case) for _ in range(repeats)]
    b.close(); plan.close()
    return out[0] if repeats == 1 else out


def _as(case, name=None, g=None, layout=None, bits=None, cols=None):
    """the case in another form or with other columns"""
    layout = case.layout if layout is None else layout
    return fc.Case(name or case.name, case.group, case.g if g is None else g, layout, cols or case.cols,
                   bits=(case.bits if bits is None else bits) if layout else 32, by=case.by, E=case.E, slot=case.slot, runs=case.runs)


def _in_bars(oracle, col, phi, exp):
    """deviation of (phi, expected) from the checker's MLE of the column, in units of the column's bar"""
    ophi, op = _checker(oracle).fit_mle(col.y, col.r)[:2]
    if col.bar == "hot":
        return max(abs(phi - ophi) / ophi / HOT_BARS[0], abs(exp - op) / op / HOT_BARS[1])
    return max(abs(phi - ophi) / ophi, abs(exp - op) / op) / max(1.0, 2e-6 / (ophi * ophi)) / FIT_REL_TOL


def _hold(oracle, case, phi, exp, nu, what=None):
    """every column of the case: held ones against the checker (the figures first, then the assertions), the others finite and in range"""
    what = what or case.name
    assert nu == 0, (what, "fit_unconverged", nu)
    assert np.all(np.isfinite(phi)) and np.all(np.isfinite(exp)) and np.all((phi > 0) & (phi < 1)) and np.all((exp > 0) & (exp < 1)), (what, phi, exp)
    rep = REPORT.setdefault(case.group, [0, 0.0])
    fracs = {}
    for s, col in enumerate(case.cols):
        if col.held:
            fracs[s] = _in_bars(oracle, col, phi[s], exp[s])
            rep[0] += 1
            rep[1] = max(rep[1], fracs[s])
    print("%-52s largest deviation %.3g bars" % (what, max(fracs.values(), default=0.0)))
    tol = [s for s, col in enumerate(case.cols) if col.held and col.bar == "tol"]
    if tol:
        _check_mle(_checker(oracle), np.stack([case.cols[s].y for s in tol], 1), np.stack([case.cols[s].r for s in tol], 1), phi[tol], exp[tol], 0, what)
    for s, col in enumerate(case.cols):
        if col.held and col.bar == "hot":
            assert fracs[s] < 1.0, (what, col.name, fracs[s], phi[s], exp[s])


# ---- every case against the checker ------------------------------------------------------------------------------------------------------

PARTS = {
    "A g8": lambda: [c for c in fc.group_A() if c.g == 8], "A g4": lambda: [c for c in fc.group_A() if c.g == 4],
    "A g2": lambda: [c for c in fc.group_A() if c.g == 2],
    "B g8": lambda: [c for c in fc.group_B() if c.g == 8], "B g4": lambda: [c for c in fc.group_B() if c.g == 4],
    "B g2": lambda: [c for c in fc.group_B() if c.g == 2],
    "C rows, layout 0": lambda: [c for c in fc.group_C() if c.layout == 0 and c.E < 65536],
    "C chunks, layout 0": lambda: [c for c in fc.group_C() if c.layout == 0 and c.E >= 65536],
    "C layout 1, 32-bit": lambda: [c for c in fc.group_C() if c.layout == 1 and c.bits == 32],
    "C layout 1, 16-bit": lambda: [c for c in fc.group_C() if c.layout == 1 and c.bits == 16],
    "D two chunks": lambda: list(fc.group_D()[:2]), "D 128 early movers": lambda: [fc.group_D()[2]], "D 129 early movers": lambda: [fc.group_D()[3]],
    "E g8": lambda: [c for c in fc.group_E() if c.g == 8], "E g2": lambda: [c for c in fc.group_E() if c.g == 2],
    "F": lambda: list(fc.group_F()), "G": lambda: list(fc.group_G()),
}


def test_the_parts_are_the_catalogue():
    assert sorted(c.name for p in PARTS.values() for c in p()) == sorted(c.name for c in fc.catalogue())


@pytest.mark.parametrize("part", list(PARTS))
def test_edge_cases_against_the_checker(edlib, oracle, part):
    for case in PARTS[part]():
        phi, exp, nu = _fit(edlib, case)
        _hold(oracle, case, phi, exp, nu)


# ---- the same column in every form --------------------------------------------------------------------------------------------------------

FORMS = [(g, layout, 32) for layout in (0, 1) for g in fc.GEOMETRIES] + [(g, 1, 16) for g in fc.GEOMETRIES] + [(0, 0, 32)]   # (0: per cell)


@pytest.mark.parametrize("g", fc.GEOMETRIES)
def test_edge_columns_agree_across_forms(edlib, oracle, g):
    """the edge columns made for geometry g (group A, and group B's of the [E][S] layout), each alone: the three forced geometries, both layouts,
    int32 and uint16, and the per-cell form agree pairwise within 2 bars"""
    cols = [(fc.E_A, fc.edge_column(g, e[0])) for e in fc.edge_values(g)] + [(fc.E_B(g, 0), fc.list_column(g, 0, k)) for k in fc.B_KINDS]
    worst = 0.0
    for E, col in cols:
        ophi, op = _checker(oracle).fit_mle(col.y, col.r)[:2]
        bar = FIT_REL_TOL * max(1.0, 2e-6 / (ophi * ophi))
        got = {}
        for hg, layout, bits in FORMS:
            case = fc.Case("%s as (%d, %d, %d)" % (col.name, hg, layout, bits), "A", hg, layout, [col], bits=bits, E=E)
            phi, exp, nu = _fit(edlib, case)
            assert nu == 0, case.name
            got[(hg, layout, bits)] = (phi[0], exp[0])
        v = np.array(list(got.values()))
        spread = max((v[:, 0].max() - v[:, 0].min()) / v[:, 0].min(), (v[:, 1].max() - v[:, 1].min()) / v[:, 1].min()) / bar
        worst = max(worst, spread)
        assert spread < 2.0, (g, col.name, spread, got)
    print("geometry %d's %d edge columns in %d forms: largest pairwise distance %.3g bars" % (g, len(cols), len(FORMS), worst))
    REPORT["forms g%d" % g] = [len(cols), worst / 2.0]


# ---- bit for bit ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group,g", [(grp, g) for grp in "AB" for g in fc.GEOMETRIES])
def test_edge_columns_repeat_and_ignore_their_neighbours(edlib, group, g):
    """a fit repeated on the same batch, a fit on a fresh batch, and the edge column alone against the edge column among its neighbours: the
    same bits -- in particular the sample whose list ran out beside the one whose list is exactly full, in one Newton workgroup"""
    for case in (fc.group_A() if group == "A" else fc.group_B()):
        if case.g != g:
            continue
        (phi, exp, nu), (phi2, exp2, nu2) = _fit(edlib, case, repeats=2)
        phi3, exp3, nu3 = _fit(edlib, case)
        assert nu == nu2 == nu3 == 0, case.name
        for what, a, b in (("repeated on the batch", phi2, exp2), ("on a fresh batch", phi3, exp3)):
            _same_bits(a, phi, "%s %s: phi" % (case.name, what))
            _same_bits(b, exp, "%s %s: expected" % (case.name, what))
        for s in ((0, 1) if case.name.endswith("pair") else (case.slot,)):
            p1, e1, _ = _fit(edlib, _as(case, name=case.name + " alone", cols=[case.cols[s]]))
            _same_bits(p1[0], phi[s], "%s: phi of column %d alone against among its neighbours" % (case.name, s))
            _same_bits(e1[0], exp[s], "%s: expected of column %d alone against among its neighbours" % (case.name, s))


# ---- what the workspace held before ---------------------------------------------------------------------------------------------------------

def _poisons(monkeypatch):
    for poison in (None, "165", "255"):
        if poison is None:
            monkeypatch.delenv("ED_FIT_POISON", raising=False)
        else:
            monkeypatch.setenv("ED_FIT_POISON", poison)
        yield poison
    monkeypatch.delenv("ED_FIT_POISON", raising=False)


@pytest.mark.parametrize("part", ["B g8", "B g4", "B g2", "C up to 3 rows", "G"])
def test_results_do_not_depend_on_what_the_workspace_held(edlib, monkeypatch, part):
    """ED_FIT_POISON unset, 165 and 255 (the histograms, lists and list counts start every fit from that byte): the same bits"""
    cases = [c for c in fc.group_C() if c.E <= 3] if part.startswith("C") else PARTS[part]()
    assert cases
    want = {}
    for poison in _poisons(monkeypatch):
        for case in cases:
            phi, exp, nu = _fit(edlib, case)
            assert nu == 0, (case.name, poison)
            if poison is None:
                want[case.name] = (phi, exp)
            _same_bits(phi, want[case.name][0], "%s, poison %s: phi" % (case.name, poison))
            _same_bits(exp, want[case.name][1], "%s, poison %s: expected" % (case.name, poison))


@pytest.mark.parametrize("layout", [0, 1])
def test_one_batch_fitted_shallow_deep_shallow(edlib, oracle, monkeypatch, layout):
    """automatic geometry, one batch object: the first fit launches all three geometries, each later one the geometry the fit before points to,
    and the device picks among the launched ones from the data (fit_hist_runs) -- so the deep batch is served by geometry 8's kernels and the
    shallow one after it by geometry 2's.  Every result to the checker's MLE at the bar, and the same bits whatever the workspace held."""
    seq = fc.F_sequence(layout)
    want = None
    for poison in _poisons(monkeypatch):
        plan, b = _batch(edlib, seq[0])
        got = [_fit_on(edlib, b, case) for case in seq]
        b.close(); plan.close()
        if want is None:
            want = got
            for case, (phi, exp, nu) in zip(seq, got):
                _hold(oracle, case, phi, exp, nu, "%s (layout %d, reused batch)" % (case.name, layout))
        for case, (phi, exp, nu), (wphi, wexp, _) in zip(seq, got, want):
            _same_bits(phi, wphi, "%s, poison %s: phi" % (case.name, poison))
            _same_bits(exp, wexp, "%s, poison %s: expected" % (case.name, poison))


# ---- nothing to fit ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("g", fc.GEOMETRIES)
def test_columns_with_nothing_to_fit(edlib, g):
    """an all-zero column and a column with one informative cell between live columns of their workgroup: finite values in (0, 1), the same
    bits whatever the neighbours; the neighbours' bits are those of a batch without them"""
    for case in fc.group_G():
        if case.g != g:
            continue
        phi, exp, nu = _fit(edlib, case)
        assert nu == 0 and np.all(np.isfinite(phi)) and np.all((phi > 0) & (phi < 1)) and np.all((exp > 0) & (exp < 1)), (case.name, phi, exp)
        others = [fc.ordinary(g, fc.E_A, 5 + k) for k in range(3)]
        phi2, exp2, _ = _fit(edlib, _as(case, cols=[others[0], case.cols[1], others[1], case.cols[3], others[2]]))
        alone = [_fit(edlib, _as(case, cols=[case.cols[s]])) for s in (1, 3)]
        for k, s in enumerate((1, 3)):
            for what, a, b in (("other neighbours", phi2[s], exp2[s]), ("alone", alone[k][0][0], alone[k][1][0])):
                _same_bits(a, phi[s], "%s: phi of the %s column, %s" % (case.name, case.cols[s].name, what))
                _same_bits(b, exp[s], "%s: expected of the %s column, %s" % (case.name, case.cols[s].name, what))
        live = [0, 2, 4]
        phi3, exp3, _ = _fit(edlib, _as(case, cols=[case.cols[s] for s in live]))
        _same_bits(phi3, phi[live], "%s: phi of the live columns without the empty ones" % case.name)
        _same_bits(exp3, exp[live], "%s: expected of the live columns without the empty ones" % case.name)


# ---- fit mode 1 reads the same bins and lists -------------------------------------------------------------------------------------------

_NM = {}


def _nm(oracle, col):
    if col.key not in _NM:
        _NM[col.key] = oracle.fit_nm(col.y, col.r, with_status=True)
    return _NM[col.key]


@pytest.mark.parametrize("group,g", [(grp, g) for grp in "AB" for g in fc.GEOMETRIES])
def test_nelder_mead_fit_on_the_edges(edlib, oracle, group, g):
    """k_fit_hnm on groups A and B with one half of the rows planted: every column against the checker's Nelder-Mead (oracle.fit_nm) at the
    bars of tests/test_gpu_fit_concordance.py.  It cannot see an off-by-one bin; it sees a lost class
    (tests/test_fit_hist_cases_host.py::test_fit_mode_1_columns_show_a_lost_class)."""
    rep = REPORT.setdefault("mode 1", [0, 0.0])
    for case in (fc.group_A(0.5) if group == "A" else fc.group_B(0.5)):
        if case.g != g:
            continue
        phi, p, nu = _fit(edlib, case, mode=1)
        assert nu == 0, case.name
        for s, col in enumerate(case.cols):
            ophi, op, ne, fail = _nm(oracle, col)
            frac = max(abs(phi[s] - ophi) / ophi / NM_BARS[0], abs(p[s] - op) / op / NM_BARS[1])
            rep[0] += 1
            rep[1] = max(rep[1], frac)
            assert fail == 0 and frac < 1.0, (case.name, s, col.name, phi[s], ophi, p[s], op, frac)


def test_report():
    """per group: columns held to the checker and the largest deviation as a fraction of its bar (DESIGN.md 4.5 quotes these)"""
    for group in sorted(REPORT):
        n, frac = REPORT[group]
        print("fit edges, %-10s %5d columns, largest deviation %.3g of the bar" % (group + ":", n, frac))
    assert REPORT and all(frac < 1.0 for _, frac in REPORT.values())
