"""A column's fit depends on that column alone.

The contract tested here: the fitted (phi, expected) of a column is a function of that column's counts and of the batch's
declared options (fit form, histogram geometry, count layout and width, fit mode) -- and of nothing else.  Not of the other
columns of the batch, not of the slot or wave the column takes, not of the order in which waves reach an atomic (k_fit_compact
packs the columns still iterating in that order), not of what the workspace held before, not of the run.  The same holds for
what the emissions, the Viterbi pass and the call table make of a sample with given (phi, p).  Every comparison below is bit for
bit; every probe is also held to the checker's long-double maximum-likelihood fit (oracle.fit_mle) at FIT_REL_TOL, since a
uniformly wrong answer would be invariant too.

The one dependence on the batch by design: with the automatic histogram geometry the batch's deepest sample picks the geometry
(fit_hist_geometry), and the geometries group their sums differently; those results agree to FIT_REL_TOL, not to the bit.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIT_REL_TOL = 1e-8


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------

def _as_bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(got, want, what):
    """bitwise equality of float64 arrays; on failure the message carries the largest distance in ulps (from the log alone)"""
    g, w = _as_bits(got), _as_bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        d = np.abs(g.astype(object) - w.astype(object)) if g.size < 64 else np.abs(g - w)
        bad = np.flatnonzero(g.ravel() != w.ravel())
        pytest.fail("%s: not bit-identical -- %d of %d values differ, max %d ulp apart (first at flat index %d: %r vs %r)"
                    % (what, bad.size, g.size, int(np.max(d)), bad[0], np.asarray(got).ravel()[bad[0]], np.asarray(want).ravel()[bad[0]]))


def _plan(edlib, E):
    return edlib.Plan(np.array([0, E], dtype=np.int32), np.arange(E, dtype=np.int32) * 100, np.arange(E, dtype=np.int32) * 100 + 50)


def _betabin(rng, E, depth, phi, p, sd=0.3):
    """one column: totals log-normal around `depth`, a beta-binomial split with dispersion phi (0: binomial) and proportion p"""
    t, r = _betabin_cols(rng, E, [depth], [phi], [p], sd)
    return t[:, 0], r[:, 0]


def _betabin_cols(rng, E, depth, phi, p, sd=0.3):
    """[E][S] columns as _betabin, one (depth, phi, p) per column"""
    depth, phi, p = (np.asarray(v, dtype=np.float64)[None, :] for v in (depth, phi, p))
    S = depth.shape[1]
    n = rng.poisson(depth * rng.lognormal(0.0, sd, (E, S))).astype(np.int64)
    ph = np.where(phi > 0, phi, 0.5)
    q = np.where(phi > 0, rng.beta(np.broadcast_to(p * (1 - ph) / ph, (E, S)), np.broadcast_to((1 - p) * (1 - ph) / ph, (E, S))), p)
    y = rng.binomial(n, q)
    return y.astype(np.int32), (n - y).astype(np.int32)


def _fit(edlib, plan, test, ref, hist=0, layout=0, bits=32, mode=0, batch=None):
    """(phi, expected, n_unconverged) of the [E][S] counts under the given options; `batch`: fit with that one (reused)"""
    E, S = test.shape
    b = batch or edlib.Batch(plan, S)
    if batch is None:
        if layout:
            b.set_emit_mode(2); b.set_counts_layout(1)
            if bits == 16:
                b.set_counts_bits(16)
        b.set_fit_histograms(hist)
        if mode:
            from exomedepth_amd._lib import check, lib
            check(lib().ed_batch_set_fit_mode(b.handle, mode))
    if layout:
        t, r = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
        if bits == 16:
            assert test.max() <= 65535 and ref.max() <= 65535
            t, r = t.astype(np.uint16), r.astype(np.uint16)
    else:
        t, r = test, ref
    dphi, dexp = edlib.DeviceArray(np.zeros(S)), edlib.DeviceArray(np.zeros(S))
    b.fit(edlib.DeviceArray(t), edlib.DeviceArray(r), dphi, dexp)
    nu = b.fit_unconverged()[0]
    out = dphi.to_host(), dexp.to_host(), nu
    if batch is None:
        b.close()
    return out


def _check_mle(oracle, test, ref, phi, exp, n_unconverged=0, what=""):
    """each column against the checker's long-double MLE at FIT_REL_TOL; below phi ~ 1.5e-3 the binary64 gradient sums locate the dispersion to
    ~2e-14 / phi^2 only, so the bar is scaled there as in test_gpu_fit.py::test_per_cell_fit_on_ill_conditioned_columns.  Columns
    the fit reports as not converged (at most n_unconverged of them) may lie beyond."""
    beyond = []
    for s in range(test.shape[1]):
        ophi, op, _, _ = oracle.fit_mle(test[:, s], ref[:, s])
        err = max(abs(phi[s] - ophi) / ophi, abs(exp[s] - op) / op) / max(1.0, 2e-6 / (ophi * ophi))
        if not err < FIT_REL_TOL:
            beyond.append((s, phi[s], ophi, exp[s], op, err))
    assert len(beyond) <= n_unconverged, (what, beyond)


# ---- A1 / A2: the per-cell fit (k_fit_accum) ------------------------------------------------------------------------------------------

def _probe_columns(rng, E):
    """16 probes: deep (every argument >= 32: the short digamma series), shallow-tailed (a few cells just below 32), ill-conditioned (tiny phi or a
    proportion near 0: more than three full passes, so that a large batch packs them)"""
    cols = []
    for k in range(5):
        cols.append(_betabin(rng, E, 600.0 * (k + 1), 1e-3 * (1 + k % 3), 0.2 + 0.06 * k))
    for k in range(5):
        cols.append(_betabin(rng, E, 5000.0 + 600 * k, 3e-3, 0.01 + 0.001 * k))
    for k in range(6):
        phi, p = ((2e-5, 5e-3), (5e-5, 0.02), (1e-4, 3e-3), (3e-5, 0.4), (2e-4, 2e-3), (1e-3, 3e-3))[k]
        cols.append(_betabin(rng, E, 1500.0 + 300 * k, phi, p))
    return np.stack([c[0] for c in cols], 1), np.stack([c[1] for c in cols], 1)


def _mates(rng, E, S, kind):
    """shallow (~5 reads, phi 0.05: shape arguments below 32, the long series), deep (shape arguments in the hundreds: the short one) or mixed"""
    k = np.full(S, ("shallow", "deep").index(kind)) if kind != "mixed" else np.arange(S) % 3
    depth = np.choose(k, [np.full(S, 5.0), np.full(S, 300.0), rng.uniform(10, 2000, S)])
    phi = np.choose(k, [np.full(S, 0.05), np.full(S, 1e-3), np.exp(rng.uniform(np.log(2e-4), np.log(0.02), S))])
    p = np.choose(k, [np.full(S, 0.3), np.full(S, 0.4), rng.uniform(0.01, 0.5, S)])
    return _betabin_cols(rng, E, depth, phi, p)


def _place(probe_t, probe_r, mate_t, mate_r, slots):
    t, r = mate_t.copy(), mate_r.copy()
    t[:, slots], r[:, slots] = probe_t, probe_r
    return t, r


def _compositions(rng, pt, pr, sizes):
    """name -> (test, ref, probe slots) of the probes in batches of different make-up"""
    E, P = pt.shape
    out = {"alone": (pt, pr, np.arange(P))}
    perm = rng.permutation(P)
    inv = np.argsort(perm)
    out["permuted"] = (pt[:, perm], pr[:, perm], inv)              # probe k sits at slot inv[k]
    slots = np.array([64 * k + (5 * k + 3) % 64 for k in range(P)])   # one probe per wave, each at another lane
    for kind in ("shallow", "deep"):
        mt, mr = _mates(rng, E, 64 * P, kind)
        out["waves of %s mates" % kind] = _place(pt, pr, mt, mr, slots) + (slots,)
    for S in sizes:                                                 # S >= 4096: the columns still iterating are packed (k_fit_compact)
        mt, mr = _mates(rng, E, S, "mixed")
        sl = np.sort(rng.choice(S, P, replace=False))
        out["S = %d" % S] = _place(pt, pr, mt, mr, sl) + (sl,)
    return out


def _assert_invariant(edlib, oracle, E, seed, sizes):
    rng = np.random.default_rng(seed)
    pt, pr = _probe_columns(rng, E)
    plan = _plan(edlib, E)
    comps = _compositions(rng, pt, pr, sizes)
    res = {}
    for name, (t, r, sl) in comps.items():
        phi, exp, nu = _fit(edlib, plan, t, r)
        res[name] = (phi[sl], exp[sl], nu)
    plan.close()
    phi0, exp0, nu0 = res["alone"]
    _check_mle(oracle, pt, pr, phi0, exp0, nu0, "probes alone, E %d" % E)
    assert res["permuted"][2] == nu0                                # the same columns: the same number left unconverged
    for name, (phi, exp, _) in res.items():
        _same_bits(phi, phi0, "E %d, phi of the probes: %s against alone" % (E, name))
        _same_bits(exp, exp0, "E %d, expected of the probes: %s against alone" % (E, name))


def test_per_cell_fit_ignores_batch_mates_and_slots(edlib, oracle):
    """set_fit_histograms(0): the probes alone, permuted, one per 64-column wave among shallow mates (the old wave vote: the long series for all)
    and among deep mates (the short series for all), and scattered through batches of 4 096 and 8 192 columns that pack their slow columns --
    the same bits each time."""
    _assert_invariant(edlib, oracle, 2000, 31, (4096, 8192))


def test_per_cell_fit_with_coarse_passes_ignores_batch_mates(edlib, oracle):
    """the same with E >= 8192, where coarse passes on every 16th exon precede the full ones"""
    _assert_invariant(edlib, oracle, 8200, 32, (4096,))


def test_per_cell_fit_repeats_bit_for_bit(edlib):
    """the mixed 8 192-column batch (slow columns packed in atomic order) fitted three times on fresh batches and three times through one
    reused batch: every output identical"""
    rng = np.random.default_rng(33)
    E, S = 2000, 8192
    pt, pr = _probe_columns(rng, E)
    mt, mr = _mates(rng, E, S, "mixed")
    t, r = _place(pt, pr, mt, mr, np.arange(0, S, S // pt.shape[1]))
    plan = _plan(edlib, E)
    runs = [_fit(edlib, plan, t, r) for _ in range(3)]
    b = edlib.Batch(plan, S)
    b.set_fit_histograms(0)
    runs += [_fit(edlib, plan, t, r, batch=b) for _ in range(3)]
    b.close(); plan.close()
    for k, (phi, exp, nu) in enumerate(runs[1:], 1):
        _same_bits(phi, runs[0][0], "phi, run %d against run 0" % k)
        _same_bits(exp, runs[0][1], "expected, run %d against run 0" % k)
        assert nu == runs[0][2], (k, nu, runs[0][2])


# ---- A3: the reference-set searches ---------------------------------------------------------------------------------------------------

def _spread_cohort(S=256, E=3000, seed=34):
    """samples whose depths span two decades: the K x S cumulative references of a wave mix deep and shallow tests"""
    rng = np.random.default_rng(seed)
    lam = rng.lognormal(np.log(40.0), 0.7, E)
    sf = np.exp(rng.uniform(np.log(0.1), np.log(10.0), S))
    grp = rng.integers(0, 6, S)
    gnoise = rng.normal(0, 0.12, (E, 6))
    mu = lam[:, None] * sf[None, :] * np.exp(gnoise[:, grp] + rng.normal(0, 0.05, (E, S)))
    return rng.poisson(mu).astype(np.int32), rng.integers(80, 600, E).astype(float)


def _same_selection_bits(a, b, what):
    assert np.array_equal(a["n_chosen"], b["n_chosen"]) and np.array_equal(a["choice"], b["choice"]), what
    ra, rb = a["summary.stats"], b["summary.stats"]
    for f in ra.dtype.names:
        if ra.dtype[f].kind == "f":
            _same_bits(ra[f], rb[f], "%s: summary.stats %s" % (what, f))
        else:
            assert np.array_equal(ra[f], rb[f]), (what, f)


@pytest.mark.parametrize("form", ["row-major", "column-major"])
def test_cohort_reference_sets_repeat_bit_for_bit(edlib, monkeypatch, form):
    """cohort_select_reference_sets three times on 256 samples of widely spread depth (8 192 cumulative references: packed when they are fitted
    column by column): choices and every statistic identical"""
    if form == "row-major":
        monkeypatch.setenv("ED_REFCOHORT_ROWMAJOR", "1")
    counts, bl = _spread_cohort()
    runs = [edlib.cohort_select_reference_sets(counts, bl, 0, max_refs=32, want_reference=False) for _ in range(3)]
    path = edlib.refcohort_last_path()
    assert (path["chunks_row_major"] > 0) == (form == "row-major"), path
    assert np.all(runs[0]["n_chosen"] >= 1)
    for k in (1, 2):
        _same_selection_bits(runs[k], runs[0], "%s run %d against run 0" % (form, k))


def test_single_test_reference_set_repeats_bit_for_bit(edlib):
    """select_reference_set (one test, the row-major per-cell fit of its cumulative references) three times on tests of low, medium and high depth"""
    counts, bl = _spread_cohort(S=200)
    order = np.argsort(counts.sum(axis=0))
    for t in (order[0], order[100], order[-1]):
        others = np.ascontiguousarray(np.delete(counts, t, axis=1))
        runs = [edlib.select_reference_set(counts[:, t], others, bl, 0) for _ in range(3)]
        for k in (1, 2):
            assert runs[k]["reference.choice"] == runs[0]["reference.choice"] and runs[k]["n.bins"] == runs[0]["n.bins"]
            ra, rb = runs[k]["summary.stats"], runs[0]["summary.stats"]
            for f in ra.dtype.names:
                if ra.dtype[f].kind == "f":
                    _same_bits(ra[f], rb[f], "test %d run %d: summary.stats %s" % (t, k, f))
                else:
                    assert np.array_equal(ra[f], rb[f]), (t, k, f)


# ---- A4: the histogram fit (k_fit_hist / k_fit_hist_sm / k_fit_hnewton / k_fit_hnm) --------------------------------------------------------

E4 = 3000


def _hist_mates(rng, kind, S):
    t, r = np.zeros((E4, S), np.int32), np.zeros((E4, S), np.int32)
    for s in range(S):
        if kind == "shallow":
            t[:, s], r[:, s] = _betabin(rng, E4, 5.0, 0.02, 0.3)
        elif kind == "deep":                    # beyond every bin of geometry 8: k_fit_hnewton sums that sample cell by cell (!fits)
            t[:, s], r[:, s] = _betabin(rng, E4, 3000.0, 2e-3, 0.3)
        elif kind == "binomial":                # pinned at the phi floor
            t[:, s], r[:, s] = _betabin(rng, E4, 300.0, 0.0, 0.15)
    return t, r                                 # "zero": all-zero columns


HIST_MATES = ("shallow", "deep", "zero", "binomial")
HIST_SLOTS = (0, 1, 2, 3, 6, 9)                 # the four positions of k_fit_hnewton's 4-sample workgroup; several k_fit_hist sample groups
HIST_LAYOUTS = ((0, 32), (1, 32), (1, 16))      # [E][S] int32, sample-major int32, sample-major uint16


def _hist_placements(probe_t, probe_r, seed, slots=HIST_SLOTS, S=16):
    rng = np.random.default_rng(seed)
    for kind in HIST_MATES:
        mt, mr = _hist_mates(rng, kind, S)
        for sl in slots:
            t, r = _place(probe_t[:, None], probe_r[:, None], mt, mr, [sl])
            yield kind, sl, t, r


@pytest.mark.parametrize("geometry", [8, 4, 2])
def test_histogram_fit_ignores_batch_mates_slots_and_workspace(edlib, oracle, monkeypatch, geometry):
    """a probe sample at each slot of the Newton kernel's 4-sample workgroup and in other k_fit_hist sample groups, beside shallow, deep (per-cell
    inside k_fit_hnewton), all-zero and binomial mates, in both count layouts and with 16-bit counts, with the workspace poisoned by three byte
    patterns (ED_FIT_POISON) or not: the same bits wherever it sits, and the checker's MLE to FIT_REL_TOL"""
    rng = np.random.default_rng(40 + geometry)
    pt, pr = _betabin(rng, E4, 150.0, 4e-3, 0.3)
    ophi, op, _, _ = oracle.fit_mle(pt, pr)
    plan = _plan(edlib, E4)
    for layout, bits in HIST_LAYOUTS:
        want = None
        for poison in (None, "0", "165", "255"):
            if poison is None:
                monkeypatch.delenv("ED_FIT_POISON", raising=False)
            else:
                monkeypatch.setenv("ED_FIT_POISON", poison)
            for kind, sl, t, r in _hist_placements(pt, pr, 50 + geometry):
                phi, exp, _ = _fit(edlib, plan, t, r, hist=geometry, layout=layout, bits=bits)
                got = (phi[sl], exp[sl])
                what = "geometry %d layout %d %d-bit, poison %s, %s mates, slot %d" % (geometry, layout, bits, poison, kind, sl)
                if want is None:
                    want = got
                    assert abs(got[0] - ophi) / ophi < FIT_REL_TOL and abs(got[1] - op) / op < FIT_REL_TOL, (what, got, ophi, op)
                _same_bits(got[0], want[0], what + ": phi")
                _same_bits(got[1], want[1], what + ": expected")
    monkeypatch.delenv("ED_FIT_POISON", raising=False)
    plan.close()


def test_histogram_fit_of_a_sample_beyond_the_bins_repeats(edlib, oracle, monkeypatch):
    """a probe beyond every bin of geometry 8 (k_fit_hnewton's per-cell path, !fits) fitted five times from different slots, beside different
    mates, with and without a poisoned workspace -- in both layouts: the same bits"""
    rng = np.random.default_rng(47)
    pt, pr = _betabin(rng, E4, 3000.0, 3e-3, 0.35)
    ophi, op, _, _ = oracle.fit_mle(pt, pr)
    plan = _plan(edlib, E4)
    mt, mr = _hist_mates(rng, "shallow", 16)
    mt[:, 8:], mr[:, 8:] = _hist_mates(rng, "deep", 8)
    for layout, bits in HIST_LAYOUTS:
        want = None
        for k, (sl, poison) in enumerate(((0, None), (3, "165"), (9, None), (1, "0"), (14, "255"))):
            if poison is None:
                monkeypatch.delenv("ED_FIT_POISON", raising=False)
            else:
                monkeypatch.setenv("ED_FIT_POISON", poison)
            t, r = _place(pt[:, None], pr[:, None], mt, mr, [sl])
            phi, exp, _ = _fit(edlib, plan, t, r, hist=8, layout=layout, bits=bits)
            got = (phi[sl], exp[sl])
            if want is None:
                want = got
                assert abs(got[0] - ophi) / ophi < FIT_REL_TOL and abs(got[1] - op) / op < FIT_REL_TOL, (layout, bits, got, ophi, op)
            _same_bits(got[0], want[0], "layout %d %d-bit, repeat %d: phi" % (layout, bits, k))
            _same_bits(got[1], want[1], "layout %d %d-bit, repeat %d: expected" % (layout, bits, k))
    monkeypatch.delenv("ED_FIT_POISON", raising=False)
    plan.close()


def test_nelder_mead_fit_ignores_batch_mates_and_slots(edlib, oracle, monkeypatch):
    """fit mode 1 (k_fit_hnm: aod's Nelder-Mead on the histograms) -- the same placements, both layouts, plain and poisoned workspace: the same bits.
    Its stopping rule is optim()'s reltol on the objective, so it is held to the MLE at 2e-2 in phi and 2e-3 in the proportion (test_gpu_fit.py's
    bar for the Nelder-Mead stand-in), not at FIT_REL_TOL."""
    rng = np.random.default_rng(48)
    pt, pr = _betabin(rng, E4, 150.0, 4e-3, 0.3)
    ophi, op, _, _ = oracle.fit_mle(pt, pr)
    plan = _plan(edlib, E4)
    for layout, bits in HIST_LAYOUTS[:2]:
        want = None
        for poison in (None, "165"):
            if poison is None:
                monkeypatch.delenv("ED_FIT_POISON", raising=False)
            else:
                monkeypatch.setenv("ED_FIT_POISON", poison)
            for kind, sl, t, r in _hist_placements(pt, pr, 49, slots=(0, 3, 9)):
                phi, exp, _ = _fit(edlib, plan, t, r, hist=8, layout=layout, bits=bits, mode=1)
                got = (phi[sl], exp[sl])
                what = "fit mode 1 layout %d, poison %s, %s mates, slot %d" % (layout, poison, kind, sl)
                if want is None:
                    want = got
                    assert abs(got[0] - ophi) / ophi < 2e-2 and abs(got[1] - op) / op < 2e-3, (what, got, ophi, op)
                _same_bits(got[0], want[0], what + ": phi")
                _same_bits(got[1], want[1], what + ": expected")
    monkeypatch.delenv("ED_FIT_POISON", raising=False)
    plan.close()


def test_automatic_geometry_is_the_one_batch_dependence(edlib, oracle):
    """With the automatic geometry the batch's deepest sample picks the histogram geometry (fit_hist_geometry): the one dependence on the batch
    by design.  The same probe beside mates that select geometry 8, 4 and 2: each result to the MLE at FIT_REL_TOL, and the three to each other."""
    rng = np.random.default_rng(51)
    pt, pr = _betabin(rng, E4, 150.0, 4e-3, 0.3)
    ophi, op, _, _ = oracle.fit_mle(pt, pr)
    plan = _plan(edlib, E4)
    got = []
    for depth in (100.0, 2200.0, 3000.0):
        mt, mr = np.zeros((E4, 8), np.int32), np.zeros((E4, 8), np.int32)
        for s in range(8):
            mt[:, s], mr[:, s] = _betabin(rng, E4, depth, 3e-3, 0.3)
        t, r = _place(pt[:, None], pr[:, None], mt, mr, [2])
        phi, exp, _ = _fit(edlib, plan, t, r, hist=1)
        got.append((phi[2], exp[2]))
        assert abs(phi[2] - ophi) / ophi < FIT_REL_TOL and abs(exp[2] - op) / op < FIT_REL_TOL, (depth, phi[2], ophi, exp[2], op)
    plan.close()
    for phi, exp in got[1:]:
        assert abs(phi - got[0][0]) / got[0][0] < FIT_REL_TOL and abs(exp - got[0][1]) / got[0][1] < FIT_REL_TOL


# ---- A5: emissions -> Viterbi -> calls with given (phi, p) ----------------------------------------------------------------------------

EMIT_FORMS = ((0, 0, 32), (1, 0, 32), (2, 0, 32), (2, 1, 32), (2, 1, 16))   # (emit mode, counts layout, count width) the library accepts


def _run_one(edlib, plan, test, ref, phi, p, form, s):
    """(log-likelihood column, path column, call rows with sample = 0) of sample s"""
    mode, layout, bits = form
    S = test.shape[1]
    b = edlib.Batch(plan, S)
    if mode:
        b.set_emit_mode(mode)
    if layout:
        b.set_counts_layout(1)
        t, r = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
        if bits == 16:
            b.set_counts_bits(16)
            t, r = t.astype(np.uint16), r.astype(np.uint16)
    else:
        t, r = test, ref
    b.run(t, r, phi, p)
    ll, path, calls = b.loglik(), b.path(), b.calls()
    b.close()
    mine = calls[calls["sample"] == s].copy()
    mine["sample"] = 0
    return ll[:, :, s].copy(), path[:, s].copy(), mine


def test_emissions_path_and_calls_ignore_batch_mates(edlib):
    """one sample with given (phi, p) alone, at several slots of 130- and 1 024-sample batches, and beside a deep tail sample (1 600 reads per
    exon), a sample the tables do not serve (phi = 1e-9) and an all-zero sample -- in every accepted combination of emission mode, count layout
    and width: its log-likelihoods, path and calls are the same bits everywhere (the tables' dimensions are the sample's own: tab_dims_of)"""
    from exomedepth_amd import synth
    E = 2000
    chrom_off, start, end = synth.exon_design(E, 3, 61)
    pt, pr, pp, pphi, _ = synth.counts_numpy(chrom_off, 1, 61, n_segments=8, mean_depth=12.0)
    rng = np.random.default_rng(62)
    settings = {"alone": (pt, pr, pphi, pp, 0)}
    for S, slots in ((130, (0, 63, 64, 129)), (1024, (5, 511, 1023))):
        mt, mr, mp, mphi, _ = synth.counts_numpy(chrom_off, S, 63 + S, n_segments=8, mean_depth=12.0)
        for sl in slots:
            t, r = _place(pt, pr, mt, mr, [sl])
            phi, p = mphi.copy(), mp.copy()
            phi[sl], p[sl] = pphi[0], pp[0]
            settings["S = %d, slot %d" % (S, sl)] = (t, r, phi, p, sl)
    tt, tr = _betabin(rng, E, 1600.0, 4e-3, 0.4)
    ut, ur, _, _, _ = synth.counts_numpy(chrom_off, 1, 64, n_segments=4, mean_depth=12.0)
    t = np.stack([tt, pt[:, 0], ut[:, 0], np.zeros(E, np.int32)], 1)
    r = np.stack([tr, pr[:, 0], ur[:, 0], np.zeros(E, np.int32)], 1)
    settings["beside tail, unserved and zero samples"] = (t, r, np.array([4e-3, pphi[0], 1e-9, 5e-3]), np.array([0.4, pp[0], 0.45, 0.4]), 1)
    plan = edlib.Plan(chrom_off, start, end)
    for form in EMIT_FORMS:
        want = None
        for name, (t, r, phi, p, sl) in settings.items():
            got = _run_one(edlib, plan, t, r, phi, p, form, sl)
            what = "emit mode %d layout %d %d-bit, %s" % (form + (name,))
            if want is None:
                want = got
                assert len(got[2]) > 0, what
            _same_bits(got[0], want[0], what + ": log-likelihoods")
            assert np.array_equal(got[1], want[1]), what + ": path"
            assert np.array_equal(got[2], want[2]), what + ": calls"
    plan.close()
