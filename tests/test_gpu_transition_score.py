"""The transition score on the GPU (csrc/edscore.inc: k_fb_score) against the long-double checker (tests/score_checker.py) evaluated on
the device's own likelihood matrix, and fit_transitions on the device.

The bar, per chain and parameter q in {t, L}, absolute: (2 bar_post + 2^-50) D_q, with bar_post = 8 (m + 1) 2^-52 max(1, max |alpha|) the
posterior's bar (tests/posterior_checker.py) and D_q = sum over the chain's gaps of max_{k->j} |d_q lt_g[k->j]|: log xi is a sum of two
quantities under the posterior's bar, the table entries agree to 4 ulp, and sum_{k,j} xi = 1 per step.  Where D_q = 0 (a chain of one
exon: both gaps padded) the device value is exactly 0.

Shapes are the posterior tests': a chromosome length on each side of the 16-exon word, of the 8-step register ring and of two and three
rings, an empty chromosome inside; widths on both sides of 16 chains per wave.

Measured on an MI355X when this file was written (test_report prints the figures with -s): see DESIGN.md 4.19.
"""
import numpy as np
import pytest

import posterior_checker as pc
import score_checker as sc
from test_gpu_posterior import SIZES, S_MAX, WIDTHS, Layout, _counts, _layout, _run, _supplied, bits

pytestmark = pytest.mark.gpu

SETTINGS = ((1e-4, 50000.0), (0.04, 6000.0), (0.3, 300.0))
GEN = (0.04, 6000.0)
FIT_SIZES = (1, 2, 3, 17, 0, 33, 257, 513, 700)
REPORT = {"chains": 0, "frac_t": 0.0, "frac_L": 0.0, "exact_zero": 0, "nan": 0}


def _plan(edlib, L, setting):
    tp, ln = SETTINGS[setting]
    return (edlib.Plan(L.chrom_off, L.start, L.end, tp, ln), pc.transitions(L.chrom_off, L.start, L.end, tp, ln),
            sc.derivatives(L.chrom_off, L.start, L.end, tp, ln))


def _compare(L, trs, dvs, ll, got_ev, got_sc, skip=()):
    """device log-evidence (C, S) and score (C, 2, S) against the long-double checker on ll (E, 3, S); chains in `skip` (c, s) are left
    alone.  Updates REPORT."""
    S = ll.shape[2]
    assert got_ev.shape == (L.C, S) and got_sc.shape == (L.C, 2, S)
    want = sc.run(ll, L.chrom_off, trs, dvs, np.longdouble)
    for c, r in enumerate(want):
        m = L.sizes[c]
        if r is None:
            assert np.all(got_ev[c] == 0.0) and np.all(got_sc[c] == 0.0), c
            continue
        res, w = r
        keep = np.array([(c, s) not in skip for s in range(S)])
        fin = np.isfinite(res["logZ"].astype(np.float64)) & keep
        bad = ~np.isfinite(res["logZ"].astype(np.float64)) & keep
        assert np.all(np.isnan(got_sc[c][:, bad])), c                     # a chain without a finite log-evidence has no score
        REPORT["nan"] += int(bad.sum())
        bar = pc.bar(m, res["alpha"])
        for q, D in enumerate(sc.weight(dvs[c], m)):
            g = got_sc[c, q]
            assert np.all(np.isfinite(g[fin])), (c, q)
            if D == 0.0:
                assert np.all(g[fin] == 0.0), (c, q)
                REPORT["exact_zero"] += int(fin.sum())
                continue
            d = np.abs(g[fin].astype(np.longdouble) - w[q][fin]).astype(np.float64)
            lim = (2 * bar[fin] + 2.0 ** -50) * D
            frac = d / lim
            if frac.size:
                key = "frac_t" if q == 0 else "frac_L"
                REPORT[key] = max(REPORT[key], float(frac.max()))
            assert np.all(frac <= 1.0), (c, q, float(frac.max()))
        REPORT["chains"] += int(fin.sum())
    return want


@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("setting", range(3))
@pytest.mark.parametrize("mode", [0, 2])
def test_every_chain_against_the_checker(edlib, mode, setting, S):
    L = _layout()
    plan, trs, dvs = _plan(edlib, L, setting)
    b = edlib.Batch(plan, S)
    if mode:
        b.set_emit_mode(mode)
    _run(b, _counts(), S)
    ll = b.loglik()
    ev, score = b.transition_score()
    assert b.n_score_passes() == 1 and b.n_posterior_passes() == 1 and plan.n_score_tables() == 1
    assert np.array_equal(bits(ev), bits(b.log_evidence()))               # logZ returned with the score is the posterior's
    _compare(L, trs, dvs, ll, ev, score)
    b.close()
    plan.close()


@pytest.mark.parametrize("setting", range(3))
def test_supplied_matrices(edlib, setting):
    """Plan.transition_score on the caller's own emissions: -inf in one and in all three states of an exon, a gap of 0 and one of 10^8 in
    every chain of 8 exons or more; a NaN in one chain leaves every other chain's bits alone and reads NaN itself"""
    L = Layout((5, 40, 64, 0, 33, 130, 1), 9, special_gaps=True)
    S = 6
    plan, trs, dvs = _plan(edlib, L, setting)
    assert any(np.isneginf(tr["C"][1:-1]).any() for tr in trs if tr)
    assert all(np.all(dv["Ct"][np.isneginf(tr["C"])] == 0) and np.all(dv["CL"][np.isneginf(tr["C"])] == 0) for tr, dv in zip(trs, dvs) if tr)
    clean = _supplied(L, S, 21 + setting)
    lo1, lo2, lo4 = (int(L.chrom_off[c]) for c in (1, 2, 4))
    clean[lo1 + 7, 0, 1] = -np.inf                      # sample 1, chain 1: deletion impossible at one exon
    clean[lo4 + 32, 2, 1] = -np.inf                     # ... and duplication at the last exon of chain 4
    clean[lo1, 1, 4] = -np.inf                          # sample 4, chain 1: normal impossible at the first exon
    clean[lo2 + 9, :, 2] = -np.inf                      # sample 2, chain 2: no state can emit exon 9
    dirty = clean.copy()
    dirty[lo2 + 30, 1, 3] = np.nan                      # sample 3, chain 2: a NaN emission
    ev, score = plan.transition_score(edlib.DeviceArray(clean), S)
    post = plan.posterior(clean, S)
    assert np.array_equal(bits(ev), bits(post.log_evidence()))            # the same backward pass, the same bits
    post.free()
    _compare(L, trs, dvs, clean, ev, score)
    assert np.isneginf(ev[2, 2]) and np.all(np.isnan(score[2, :, 2]))
    d_ev, d_score = plan.transition_score(dirty, S)
    assert np.isnan(d_ev[2, 3]) and np.all(np.isnan(d_score[2, :, 3]))
    mask = np.ones((L.C, 2, S), bool)
    mask[2, :, 3] = False
    assert np.array_equal(bits(d_score)[mask], bits(score)[mask])
    assert np.array_equal(bits(d_ev)[mask[:, 0, :]], bits(ev)[mask[:, 0, :]])
    assert plan.n_score_tables() == 1
    plan.close()


def test_width_independence(edlib):
    """a sample's scores have the same bits alone, in 65 samples and in 130 samples"""
    L = _layout()
    plan, _, _ = _plan(edlib, L, 1)
    b = edlib.Batch(plan, S_MAX)
    _run(b, _counts(), S_MAX)
    ll = b.loglik()
    ev_b, sc_b = b.transition_score()
    ev130, sc130 = plan.transition_score(ll, S_MAX)
    assert np.array_equal(bits(sc130), bits(sc_b)) and np.array_equal(bits(ev130), bits(ev_b))
    ev65, sc65 = plan.transition_score(np.ascontiguousarray(ll[:, :, :65]), 65)
    assert np.array_equal(bits(sc65), bits(sc130[:, :, :65])) and np.array_equal(bits(ev65), bits(ev130[:, :65]))
    for s in (0, 15, 16, 64, 129):
        ev1, sc1 = plan.transition_score(np.ascontiguousarray(ll[:, :, s:s + 1]), 1)
        assert np.array_equal(bits(sc1[:, :, 0]), bits(sc130[:, :, s])) and np.array_equal(bits(ev1[:, 0]), bits(ev130[:, s])), s
    b.close()
    plan.close()


@pytest.mark.parametrize("async_tail", [False, True])
def test_requests(edlib, async_tail):
    """a second request launches nothing; a new run invalidates the scores; a batch reused (under an asynchronous tail too) gives the
    bits of a fresh batch; posterior requests before or after do not change them"""
    L = _layout()
    S = 65
    plan, _, _ = _plan(edlib, L, 2)
    dA, dB = _counts(7), _counts(8)

    def batch():
        b = edlib.Batch(plan, S)
        if async_tail:
            b.set_async_tail(True)
        return b
    fresh = {}
    for name, d in (("A", dA), ("B", dB)):
        b = batch()
        _run(b, d, S)
        fresh[name] = b.transition_score()
        b.close()
    assert not np.array_equal(bits(fresh["A"][1]), bits(fresh["B"][1]))
    b = batch()
    for k, (name, d) in enumerate((("A", dA), ("B", dB), ("A", dA))):
        _run(b, d, S)
        if k == 1:
            b.posterior()                                                 # the posterior first: the score pass follows it
        ev, score = b.transition_score()
        assert b.n_score_passes() == k + 1 and b.n_posterior_passes() == k + 1
        ev2, score2 = b.transition_score()
        assert b.n_score_passes() == k + 1 and b.n_posterior_passes() == k + 1
        assert np.array_equal(bits(score), bits(score2)) and np.array_equal(bits(ev), bits(ev2))
        assert np.array_equal(bits(score), bits(fresh[name][1])) and np.array_equal(bits(ev), bits(fresh[name][0])), name
    assert plan.n_score_tables() == 1
    b.close()
    plan.close()


def test_a_fused_batch_without_the_matrix_is_refused(edlib):
    L = _layout()
    S = 17
    test, ref, phi, p = (np.ascontiguousarray(x[..., :S]) for x in _counts())
    plan, _, _ = _plan(edlib, L, 1)
    f = edlib.Batch(plan, S)
    f.set_fused(True)
    f.keep_loglik(False)
    f.run(test, ref, phi, p)
    with pytest.raises(edlib.EdError, match="likelihood matrix"):
        f.transition_score()
    assert f.n_score_passes() == 0
    with pytest.raises(edlib.EdError):
        edlib.fit_transitions(L.chrom_off, L.start, L.end, f)
    f.close()
    plan.close()


def test_fit_transitions_on_the_device(edlib):
    """data drawn from the model (48 samples): from the defaults the device fit converges to a log-evidence no smaller than that of the
    generating parameters, and no smaller than the checker-driven fit's less 2 reltol |l|; a batch, a device array and a list of slabs
    are the same cohort"""
    chrom_off, start, end, ll = sc.draw(FIT_SIZES, 48, GEN[0], GEN[1], 11)
    reltol = float(np.sqrt(2.0 ** -52))
    fit = edlib.fit_transitions(chrom_off, start, end, ll, 48)
    print({k: v for k, v in fit.items() if k != "trace"})
    assert fit["converged"] and fit["iterations"] <= 100
    gen = edlib.Plan(chrom_off, start, end, GEN[0], GEN[1])
    l_gen = float(gen.transition_score(ll, 48)[0].sum())
    gen.close()
    assert fit["log_evidence"] >= l_gen and fit["log_evidence"] >= fit["log_evidence_start"]
    cpu = edlib.fit_transitions(chrom_off, start, end, evaluate=sc.fast_evaluator(chrom_off, start, end, ll))
    print({k: v for k, v in cpu.items() if k != "trace"})
    assert cpu["converged"]
    assert fit["log_evidence"] >= cpu["log_evidence"] - 2 * reltol * abs(cpu["log_evidence"])
    # the same cohort as two slabs (one of them a device array): the same evaluations up to the order of the sum
    dev = edlib.DeviceArray(np.ascontiguousarray(ll[:, :, :20]))
    two = edlib.fit_transitions(chrom_off, start, end, [dev, np.ascontiguousarray(ll[:, :, 20:])], [20, 28], max_iter=2)
    one = edlib.fit_transitions(chrom_off, start, end, ll, 48, max_iter=2)
    assert abs(two["log_evidence_start"] - one["log_evidence_start"]) <= 1e-12 * abs(one["log_evidence_start"])
    assert abs(two["log_evidence"] - one["log_evidence"]) <= 1e-9 * abs(one["log_evidence"])
    dev.free()
    # a chain without a finite log-evidence is named
    bad = ll.copy()
    bad[int(chrom_off[3]) + 4, :, 7] = -np.inf
    with pytest.raises(ValueError, match="chromosome 3, sample 7"):
        edlib.fit_transitions(chrom_off, start, end, bad, 48)


def test_fit_transitions_of_one_sample(edlib):
    """ExomeDepth.fit_transitions: the one-sample convenience runs the same fit on the object's likelihood slot"""
    L = _layout()
    test, ref, phi, p = _counts()
    rows = np.concatenate([np.arange(L.chrom_off[c], L.chrom_off[c + 1]) for c in (L.sizes.index(257), L.sizes.index(513))])
    chrom = np.repeat(["1", "2"], [257, 513])
    x = edlib.ExomeDepth(test[rows, 0].astype(float), ref[rows, 0].astype(float), phi=float(phi[0]), expected=float(p[0]))
    st_, en_ = L.start[rows], (L.start[rows] + 60).astype(np.int32)
    fit = x.fit_transitions(chrom, st_, en_, transition_probability=0.05, expected_CNV_length=3000.0)
    same = edlib.fit_transitions(np.array([0, 257, 770], np.int32), st_, en_, np.ascontiguousarray(x.likelihood).reshape(-1, 3, 1), 1, 0.05, 3000.0)
    assert fit["converged"] and fit["log_evidence"] >= fit["log_evidence_start"]
    assert fit["log_evidence"] == same["log_evidence"] and fit["transition_probability"] == same["transition_probability"]


def test_report():
    """the figures quoted in DESIGN.md 4.19 (printed with -s); the fractions are of the bar of this file's docstring"""
    print("\ntransition score: %(chains)d chains with a finite log-evidence (%(nan)d without: NaN scores, %(exact_zero)d values exactly 0); "
          "largest deviation as a fraction of its bar: d/dt %(frac_t).4f, d/dL %(frac_L).4f" % REPORT)
    assert REPORT["chains"] > 0 and REPORT["exact_zero"] > 0 and REPORT["nan"] > 0
