"""Forward-backward on the GPU (csrc/edpost.inc: k_fb_backward, k_fb_forward, k_call_post) against the long-double checker
(tests/posterior_checker.py) evaluated on the device's own likelihood matrix, so that the emission modes' tolerances do not enter.

The bar, for logZ and every finite log gamma of a chain of m exons: 8 (m + 1) 2^-52 max(1, max |finite alpha|), absolute -- a
log-sum-exp step adds a few ulp of its result to the error it inherits, ed_pexp / ed_plog are 1-ulp functions.  log_p_all gets twice the
bar (two beta, one log gamma, a short sum); post_mean / post_min the bar applied to the exponent plus 4 ulp.  A wrong row, gap or state
shows as an error of order 1.

One layout puts a chromosome length on each side of the 16-exon word, of the 8-step register ring and of two and three rings, with an
empty chromosome inside; every exon has its own gap.  Counts carry planted deletions and duplications; that every sample has an exon with
gamma(del) > 1/2 and one with gamma(dup) > 1/2 at the loud setting is a condition, computed on the CPU from the CPU checker's
likelihoods and asserted before any device value is read.

Measured on an MI355X when this file was written (test_report prints the figures with -s): see DESIGN.md 4.18.
"""
import numpy as np
import pytest

import posterior_checker as pc
from test_gpu_chain_geometry import LOUD, SETTINGS

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 0, 47, 48, 49, 255, 256, 257, 513)
WIDTHS = (1, 3, 16, 17, 64, 65, 130)
S_MAX = 130
STRONG = 8000
REPORT = {"chains": 0, "values": 0, "rows": 0, "frac_gamma": 0.0, "frac_logz": 0.0, "frac_all": 0.0, "frac_post": 0.0}
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Layout:
    def __init__(self, sizes, seed, special_gaps=False):
        self.sizes = [int(n) for n in sizes]
        self.chrom_off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self.E, self.C = int(self.chrom_off[-1]), len(self.sizes)
        rng = np.random.default_rng(seed)
        gaps = rng.integers(100, 9000, self.E).astype(np.int64)          # uneven: every exon has its own row of log-transitions
        if special_gaps:
            for c in range(self.C):
                lo, m = int(self.chrom_off[c]), self.sizes[c]
                if m >= 8:
                    gaps[lo + 3] = 0                                     # C = -inf
                    gaps[lo + m // 2] = 100_000_000                      # the rows equal the from-normal row
        start = np.empty(self.E, dtype=np.int64)
        for c in range(self.C):
            lo, hi = self.chrom_off[c], self.chrom_off[c + 1]
            start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
        assert self.E == 0 or start.max() < 2_000_000_000
        self.start = start.astype(np.int32)
        self.end = (start + rng.integers(50, 400, self.E)).astype(np.int32)


def _layout():
    if "layout" not in _CACHE:
        _CACHE["layout"] = Layout(SIZES, 41)
    return _CACHE["layout"]


def _counts(seed=7):
    """(test, ref int32 [E][S_MAX], phi, p): states in geometric blocks (mean 5 exons, half of the exons in a CNV state) at depth 40, and
    deep planted blocks -- a deletion and a duplication per sample in each of the two longest chains, whole short chains in one state"""
    key = ("counts", seed)
    if key not in _CACHE:
        L = _layout()
        rng = np.random.default_rng(seed)
        E, S = L.E, S_MAX
        p = rng.uniform(0.30, 0.50, S)
        phi = rng.uniform(5e-4, 3e-3, S)
        ratio = np.array([1.0, 0.5, 1.5])
        pp = p[None, :] * ratio[:, None] / (p[None, :] * ratio[:, None] + 1 - p[None, :])
        state = np.empty((E, S), dtype=np.int64)
        for s in range(S):
            nb = E // 3 + 64
            state[:, s] = np.repeat(rng.choice(np.array([0, 0, 1, 2]), nb), rng.geometric(0.2, nb))[:E]
        sv = np.arange(S)
        tot = rng.poisson(40.0, (E, S))
        test = rng.binomial(tot, pp[state, sv[None, :]]).astype(np.int32)
        ref = (tot - test).astype(np.int32)
        t_strong = np.rint(STRONG * pp).astype(np.int32)

        def plant(rows, s, st):
            test[rows, s] = t_strong[st, s]
            ref[rows, s] = STRONG - t_strong[st, s]
        for c in (L.sizes.index(513), L.sizes.index(257)):
            lo = int(L.chrom_off[c])
            for s in range(S):
                a = lo + 20 + s % 7
                plant(np.arange(a, a + 6), s, 1 + (c + s) % 2)
                plant(np.arange(a + 40, a + 45), s, 2 - (c + s) % 2)
                plant(np.arange(a + 60, a + 63), s, 1)                 # a direct deletion -> duplication switch
                plant(np.arange(a + 63, a + 66), s, 2)
        for c in (0, 1, 2):                                            # chains of 1, 2, 3 exons in one CNV state for a third of the samples
            lo, m = int(L.chrom_off[c]), L.sizes[c]
            for s in range(c, S, 3):
                plant(np.arange(lo, lo + m), s, 1 + (c + s) % 2)
        _CACHE[key] = (test, ref, phi, p)
    return _CACHE[key]


def _cpu_condition(oracle):
    """every sample has an exon with gamma(del) > 1/2 and one with gamma(dup) > 1/2 at the loud setting: from the CPU checker's own
    likelihoods, without the device"""
    if "rich" not in _CACHE:
        L = _layout()
        test, ref, phi, p = _counts()
        cols = []
        for s in range(S_MAX):
            ll, nerr = oracle.get_loglike_matrix(phi[s], p[s], test[:, s] + ref[:, s], test[:, s], 1.0, oracle.PORTABLE)
            assert nerr == 0
            cols.append(np.asarray(ll))
        ll = np.ascontiguousarray(np.stack(cols, axis=2))
        tp, ln = SETTINGS[LOUD]
        res = pc.run(ll, L.chrom_off, pc.transitions(L.chrom_off, L.start, L.end, tp, ln), np.float64)
        g = np.concatenate([r["log_gamma"] for r in res if r is not None], axis=0)          # (E, 3, S)
        _CACHE["rich"] = (bool(np.all(np.exp(g[:, 1, :]).max(axis=0) > 0.5)), bool(np.all(np.exp(g[:, 2, :]).max(axis=0) > 0.5)))
    assert _CACHE["rich"] == (True, True)


def _compare(L, trs, ll, got_lp, got_ev, calls=None, got_cp=None, skip=()):
    """device log posterior (E, 2, S), log-evidence (C, S) and call rows against the long-double checker on ll (E, 3, S); chains in
    `skip` (c, s) are left alone.  Updates REPORT."""
    S = ll.shape[2]
    want = pc.run(ll, L.chrom_off, trs, np.longdouble)
    bars = {}
    for c, res in enumerate(want):
        lo, m = int(L.chrom_off[c]), L.sizes[c]
        if res is None:
            assert np.all(got_ev[c] == 0.0), c
            continue
        bar = pc.bar(m, res["alpha"])
        bars[c] = bar
        keep = np.array([(c, s) not in skip for s in range(S)])
        z = res["logZ"].astype(np.float64)
        fin_z = np.isfinite(z) & keep
        assert np.array_equal(np.isneginf(z) & keep, np.isneginf(got_ev[c]) & keep), c
        with np.errstate(invalid="ignore"):
            dz = np.abs((got_ev[c].astype(np.longdouble) - res["logZ"])[fin_z]).astype(np.float64)
        assert np.all(dz <= bar[fin_z]), (c, dz.max(), bar.min())
        if dz.size:
            REPORT["frac_logz"] = max(REPORT["frac_logz"], float((dz / bar[fin_z]).max()))
        w = res["log_gamma"][:, 1:, :]                                                       # (m, 2, S)
        g = got_lp[lo:lo + m]
        fin = np.isfinite(w.astype(np.float64)) & fin_z[None, None, :]
        ninf = np.isneginf(w.astype(np.float64)) & fin_z[None, None, :]
        assert np.array_equal(np.isneginf(g) & fin_z[None, None, :], ninf), c
        d = np.where(fin, np.abs(np.where(fin, g, 0).astype(np.longdouble) - np.where(fin, w, 0)), 0).astype(np.float64)
        frac = d / bar[None, None, :]
        assert np.all(frac <= 1.0), (c, float(frac.max()), np.argwhere(frac > 1.0)[:4])
        REPORT["frac_gamma"] = max(REPORT["frac_gamma"], float(frac.max()))
        REPORT["chains"] += int(fin_z.sum())
        REPORT["values"] += int(fin.sum())
    if calls is None:
        return want
    assert len(calls) == len(got_cp)
    for r, q in zip(calls, got_cp):
        c, s, t = int(r["chrom"]), int(r["sample"]), int(r["type"])
        if (c, s) in skip:
            continue
        lo = int(L.chrom_off[c])
        a, b = int(r["start_exon"]) - lo, int(r["end_exon"]) - lo
        mean, mn, all_, z = pc.call_post(want[c], ll[lo:lo + L.sizes[c]], trs[c], a, b, t, s)
        bar = bars[c][s]
        assert bits(q["log_evidence"]) == bits(got_ev[c, s])
        d_all = abs(float(np.longdouble(q["log_p_all"]) - all_))
        assert d_all <= 2 * bar, (c, s, a, b, t, d_all, bar)
        REPORT["frac_all"] = max(REPORT["frac_all"], d_all / (2 * bar))
        for gotv, wantv in ((q["post_mean"], mean), (q["post_min"], mn)):
            tol = float(wantv) * np.expm1(bar) + 4 * np.spacing(float(wantv))
            dv = abs(float(np.longdouble(gotv) - wantv))
            assert dv <= tol, (c, s, a, b, t, dv, tol)
            REPORT["frac_post"] = max(REPORT["frac_post"], dv / tol)
        REPORT["rows"] += 1
    return want


def _plan(edlib, L, setting):
    tp, ln = SETTINGS[setting]
    return edlib.Plan(L.chrom_off, L.start, L.end, tp, ln), pc.transitions(L.chrom_off, L.start, L.end, tp, ln)


def _run(b, data, S):
    test, ref, phi, p = data
    b.run(np.ascontiguousarray(test[:, :S]), np.ascontiguousarray(ref[:, :S]), phi[:S], p[:S])


def test_layout_covers_the_geometry():
    """a property of this file, checked without the device: both sides of the 16-exon word and of one, two, three and more rings of 8
    steps; an empty chromosome between non-empty ones; the widths on both sides of 16 chains per wave"""
    assert {1, 2, 3, 15, 16, 17, 31, 32, 33, 47, 48, 49, 255, 256, 257, 513} <= set(SIZES) and 0 in SIZES[1:-1]
    assert {1, 16, 17, 64, 65} <= set(WIDTHS) and max(WIDTHS) > 128


@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("setting", range(3))
@pytest.mark.parametrize("mode", [0, 2])
def test_every_chain_against_the_checker(edlib, oracle, mode, setting, S):
    _cpu_condition(oracle)
    L = _layout()
    plan, trs = _plan(edlib, L, setting)
    b = edlib.Batch(plan, S)
    if mode:
        b.set_emit_mode(mode)
    _run(b, _counts(), S)
    ll = b.loglik()
    got = b.posterior(log=True)
    ev = b.log_evidence()
    calls, cp = b.calls(), b.call_posterior()
    assert len(calls) > 0 and b.n_posterior_passes() == 1
    p = b.posterior()
    assert np.array_equal(bits(p), bits(np.exp(got)))
    want = _compare(L, trs, ll, got, ev, calls, cp)
    if setting == LOUD:                       # the condition holds for the device's own matrix too
        g = np.concatenate([r["log_gamma"] for r in want if r is not None], axis=0).astype(np.float64)
        assert np.all(np.exp(g[:, 1, :]).max(axis=0) > 0.5) and np.all(np.exp(g[:, 2, :]).max(axis=0) > 0.5)
    b.close()
    plan.close()


def _supplied(L, S, seed):
    rng = np.random.default_rng(seed)
    return -rng.gamma(2.0, 3.0, (L.E, 3, S))


@pytest.mark.parametrize("setting", range(3))
def test_supplied_matrices(edlib, setting):
    """ed_plan_posterior on the caller's own emissions: -inf in one and in all three states of an exon, a NaN in one chain, a gap of 0 and
    one of 10^8 in every chain of 8 exons or more"""
    L = Layout((5, 40, 64, 0, 33, 130), 9, special_gaps=True)
    S = 6
    plan, trs = _plan(edlib, L, setting)
    assert any(np.isneginf(tr["C"][1:-1]).any() for tr in trs if tr)
    big = [tr for tr in trs if tr and len(tr["A"]) > 9]
    assert all(np.any((tr["A"] == tr["c0"]) & (tr["B"] == tr["c1"]) & (tr["C"] == tr["c1"])) for tr in big)
    clean = _supplied(L, S, 21 + setting)
    lo1, lo2, lo4 = (int(L.chrom_off[c]) for c in (1, 2, 4))
    clean[lo1 + 7, 0, 1] = -np.inf                      # sample 1, chain 1: deletion impossible at one exon
    clean[lo4 + 32, 2, 1] = -np.inf                     # ... and duplication at the last exon of chain 4
    clean[lo1, 1, 4] = -np.inf                          # sample 4, chain 1: normal impossible at the first exon
    clean[lo2 + 9, :, 2] = -np.inf                      # sample 2, chain 2: no state can emit exon 9
    dirty = clean.copy()
    dirty[lo2 + 30, 1, 3] = np.nan                      # sample 3, chain 2: a NaN emission
    res = {}
    for name, ll in (("clean", clean), ("dirty", dirty)):
        post = plan.posterior(edlib.DeviceArray(ll), S)
        res[name] = (post.log_posterior(), post.log_evidence(), post.beta())
        post.free()
    got_lp, got_ev, got_beta = res["clean"]
    want = _compare(L, trs, clean, got_lp, got_ev)
    assert np.isneginf(got_ev[2, 2]) and np.isneginf(want[2]["logZ"][2])
    assert np.isneginf(got_lp[lo1 + 7, 0, 1]) and np.isneginf(got_lp[lo4 + 32, 1, 1])
    # beta against the checker, where finite (the same bar)
    for c, r in enumerate(want):
        if r is None:
            continue
        lo, m = int(L.chrom_off[c]), L.sizes[c]
        w = r["beta"].astype(np.float64)
        fin = np.isfinite(w) & np.isfinite(r["logZ"].astype(np.float64))[None, None, :]
        d = np.where(fin, np.abs(np.where(fin, got_beta[lo:lo + m], 0).astype(np.longdouble) - np.where(fin, r["beta"], 0)), 0).astype(np.float64)
        assert np.all(d <= pc.bar(m, r["alpha"])[None, None, :]), c
    # the NaN chain: NaN evidence; every other chain of the matrix bit for bit what it is without the NaN
    d_lp, d_ev, _ = res["dirty"]
    assert np.isnan(d_ev[2, 3])
    mask = np.ones((L.C, S), bool)
    mask[2, 3] = False
    assert np.array_equal(bits(d_ev)[mask], bits(got_ev)[mask])
    same = np.ones((L.E, 2, S), bool)
    same[lo2:lo2 + 64, :, 3] = False
    assert np.array_equal(bits(d_lp)[same], bits(got_lp)[same])
    plan.close()


def test_width_independence_and_repeated_requests(edlib):
    """sample s alone equals sample s inside 65 and 130 samples, bit for bit (the passes on one matrix, cut three ways); two requests on a
    batch return the same bits and the second launches nothing"""
    L = _layout()
    plan, _ = _plan(edlib, L, 1)
    b = edlib.Batch(plan, S_MAX)
    _run(b, _counts(), S_MAX)
    ll = b.loglik()
    first, ev1 = b.posterior(log=True), b.log_evidence()
    cp1 = b.call_posterior()
    assert b.n_posterior_passes() == 1
    second, ev2 = b.posterior(log=True), b.log_evidence()
    assert b.n_posterior_passes() == 1
    assert np.array_equal(bits(first), bits(second)) and np.array_equal(bits(ev1), bits(ev2)) and b.call_posterior().tobytes() == cp1.tobytes()
    full = plan.posterior(ll, S_MAX)
    lp130, ev130 = full.log_posterior(), full.log_evidence()
    full.free()
    assert np.array_equal(bits(lp130), bits(first)) and np.array_equal(bits(ev130), bits(ev1))
    half = plan.posterior(np.ascontiguousarray(ll[:, :, :65]), 65)
    lp65, ev65 = half.log_posterior(), half.log_evidence()
    half.free()
    assert np.array_equal(bits(lp65), bits(lp130[:, :, :65])) and np.array_equal(bits(ev65), bits(ev130[:, :65]))
    for s in (0, 15, 16, 64, 129):
        one = plan.posterior(np.ascontiguousarray(ll[:, :, s:s + 1]), 1)
        lp1, e1 = one.log_posterior(), one.log_evidence()
        one.free()
        assert np.array_equal(bits(lp1[:, :, 0]), bits(lp130[:, :, s])) and np.array_equal(bits(e1[:, 0]), bits(ev130[:, s])), s
    b.close()
    plan.close()


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("async_tail", [False, True])
def test_a_batch_is_reusable(edlib, mode, async_tail):
    """run, request, run with other counts, request: every request gives the result of the run before it (under an asynchronous tail
    too); paths, call tables and their decoration are byte-identical with and without posterior requests"""
    L = _layout()
    S = 65
    plan, _ = _plan(edlib, L, 2)
    dA, dB = _counts(7), _counts(8)

    def batch():
        b = edlib.Batch(plan, S)
        if mode:
            b.set_emit_mode(mode)
        if async_tail:
            b.set_async_tail(True)
        return b
    fresh = {}
    for name, d in (("A", dA), ("B", dB)):
        b = batch()
        _run(b, d, S)
        fresh[name] = (b.posterior(log=True), b.log_evidence(), b.call_posterior())
        b.close()
    assert not np.array_equal(bits(fresh["A"][0]), bits(fresh["B"][0]))
    quiet, loud = batch(), batch()
    for name, d in (("A", dA), ("B", dB)):
        _run(quiet, d, S)
        _run(loud, d, S)
        lp, ev, cp = loud.posterior(log=True), loud.log_evidence(), loud.call_posterior()        # between two runs
        assert np.array_equal(bits(lp), bits(fresh[name][0])) and np.array_equal(bits(ev), bits(fresh[name][1])), name
        assert cp.tobytes() == fresh[name][2].tobytes(), name
        assert loud.calls().tobytes() == quiet.calls().tobytes() and loud.call_info().tobytes() == quiet.call_info().tobytes(), name
        assert loud.path().tobytes() == quiet.path().tobytes(), name
    assert loud.n_posterior_passes() == 2 and quiet.n_posterior_passes() == 0
    for b in (quiet, loud):
        b.close()
    plan.close()


def test_cohort_and_callcnvs_equal_the_batch(edlib):
    from exomedepth_amd.api import CALL_DTYPE
    L = _layout()
    S = 17
    test, ref, phi, p = (np.ascontiguousarray(x[..., :S]) for x in _counts())
    plan, _ = _plan(edlib, L, 1)
    b = edlib.Batch(plan, S)
    b.run(test, ref, phi, p)
    want_cp, want_ev, want_p = b.call_posterior(), b.log_evidence(), b.posterior()
    co = edlib.Cohort(plan, S, 2)
    dev = [edlib.DeviceArray(x) for x in (test, ref, phi, p)]
    t = co.submit(dev[0], dev[1], dev[2], dev[3], n_samples=S)
    plain = co.results(t, S)
    assert "call_posterior" not in plain and "posterior" not in plain
    out = co.results(t, S, posterior="matrix")
    assert out["calls"].tobytes() == b.calls().tobytes() and out["call_posterior"].tobytes() == want_cp.tobytes()
    assert np.array_equal(bits(out["log_evidence"]), bits(want_ev)) and np.array_equal(bits(out["posterior"]), bits(want_p))
    assert "posterior" not in co.results(t, S, posterior=True)
    co.close()
    # fused mode without the matrix: an error, not a guess
    f = edlib.Batch(plan, S)
    f.set_fused(True)
    f.keep_loglik(False)
    f.run(test, ref, phi, p)
    with pytest.raises(edlib.EdError, match="likelihood matrix"):
        f.posterior()
    f.close()
    b.close()
    plan.close()
    # CallCNVs on the two longest chromosomes of sample 0, constant and per-exon parameters
    tp, ln = SETTINGS[1]
    rows = np.concatenate([np.arange(L.chrom_off[c], L.chrom_off[c + 1]) for c in (L.sizes.index(257), L.sizes.index(513))])
    chrom = np.repeat(["1", "2"], [257, 513])
    names = np.array(["e%d" % i for i in range(rows.size)], dtype=object)
    ct, cr = test[rows, 0].astype(float), ref[rows, 0].astype(float)
    st_, en_ = L.start[rows], (L.start[rows] + 60).astype(np.int32)       # (CallCNVs orders exons by their mid-points: keep that the order of the starts)
    base = ("start.p", "end.p", "type", "nexons", "start", "end", "chromosome", "id", "BF", "reads.expected", "reads.observed", "reads.ratio")
    for phi_x in (float(phi[0]), np.where(np.arange(rows.size) % 2 == 0, phi[0], 1.5 * phi[0])):
        x = edlib.ExomeDepth(ct, cr, phi=phi_x, expected=float(p[0]))
        x.CallCNVs(chrom, st_, en_, names, tp, ln)
        quiet = [dict(r) for r in x.CNV_calls]
        assert quiet and all(tuple(r.keys()) == base for r in quiet)
        x.CallCNVs(chrom, st_, en_, names, tp, ln, posterior=True)
        assert all(tuple(r.keys()) == base + ("post.mean", "post.min", "post.all", "log.evidence") for r in x.CNV_calls)
        assert [{k: r[k] for k in base} for r in x.CNV_calls] == quiet
        pl = edlib.Plan(np.array([0, 257, 770], np.int32), st_, en_, tp, ln)
        post = pl.posterior(np.ascontiguousarray(x.likelihood).reshape(-1, 3, 1), 1)
        tab = np.zeros(len(quiet), dtype=CALL_DTYPE)
        tab["chrom"] = [int(r["chromosome"]) - 1 for r in quiet]
        tab["start_exon"] = [r["start.p"] - 1 for r in quiet]
        tab["end_exon"] = [r["end.p"] - 1 for r in quiet]
        tab["type"] = [1 if r["type"] == "deletion" else 2 for r in quiet]
        cp = post.call_posterior(tab)
        for r, q in zip(x.CNV_calls, cp):
            assert (r["post.mean"], r["post.min"], r["post.all"], r["log.evidence"]) == tuple(float(q[k]) for k in cp.dtype.names)
            assert 0.0 <= r["post.min"] <= r["post.mean"] <= 1.0 + 1e-12 and r["post.all"] <= 1e-12
        post.free()
        pl.close()


def test_report():
    """the figures quoted in DESIGN.md 4.18 (printed with -s); the fractions are of the bars of this file's docstring"""
    print("\nposterior: %(chains)d chains, %(values)d finite log gamma, %(rows)d call rows; largest deviation as a fraction of its bar: "
          "log gamma %(frac_gamma).4f, logZ %(frac_logz).4f, log_p_all %(frac_all).4f, post_mean / post_min %(frac_post).4f" % REPORT)
    assert REPORT["chains"] > 0 and REPORT["rows"] > 0
