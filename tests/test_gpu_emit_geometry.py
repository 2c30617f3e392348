"""The depth-binned (`phi.bins > 1`) and covariate models swept over the geometry of their kernels: k_bins_ctab, k_emit_bins_tab and
k_emit_bins (csrc/edbins.inc) with the emission launch block of batch_run_impl, cov_expected, the fits k_fitb_* / k_fitc_* with
k_bins_colmax and the order-statistic bisection, the histogram form k_lh_* (csrc/edbins_hist.inc), and the piece arithmetic of the
cohort's cut launch.

The expectation is always the CPU checker (oracle/), never a device result.  The emission tests write phi_bins, edges, expected (or
beta, phi) into device arrays by hand, so no fit tolerance stands between the inputs and the bits that are compared, and the reference
counts are planted (tests/emit_geometry_cases.py): 0, every mid-point of the levels that is an integer and its two neighbours, floor and
ceiling of the others, every edge, counts outside the mid-points, 8191 / 8192 / 8193 / ~200 000 around the end of the table of constants
(kBinsRtab = 8192), cells with test = 0 and with test = ref = 0.  Where a sample has fewer exons than plants (E <= 5) the plants are
dealt round the samples.  At E = 130 and 258 the counts beyond the table sit in chosen tiles: two tiles of workgroup 0 filled by every
sample, tiles with exactly one such cell (first lane, last lane, last exon row), tile 31 (the last of a workgroup's walk of 32), the
partial last workgroup, and all other tiles with none.  tests/test_emit_geometry_host.py asserts all of that from the arrays, and the
preconditions of the fit cases (every level populated, the checker's dispersions inside [1e-3, 0.1]), on the CPU.

NOT RUN ON A DEVICE.  When this file was written no MI355X could be reached: the host half (tests/test_emit_geometry_host.py: the
generators, every planted count, the tile placement, the checker's side of every comparison, the preconditions of the fit cases)
passes on the CPU; no test below has executed, no wall time is measured, and no tolerance below is known to be met or missed.

Value-only mutants of the kernels (each changes values, no address).  The seven libraries were built aside; none has been run, so
the table names the tests whose planted inputs reach the mutated value, not tests seen to fail:
  emit_bins_tile with ctab, `mine = r >= rtab` -> `r > rtab`: every sample of the (130, 130), (258, 2), (1027, 65) and fold cases
      holds a reference count of exactly 8192 (test_bins_emissions_match_the_checker, test_bins_grid_fold, the mixture and reuse tests);
  k_bins_ctab evaluates phi at r + 1: every cell of every bins emission test whose phi.linear is not constant around its count;
  k_bins_ctab ignores mix_s: test_bins_per_sample_mixture (distinct mixtures in (0.2, 1]);
  k_bins_edges without fmin(., q): test_fit_bins_over_block_and_chunk_edges compares the edges of every column bit for bit, and
      test_emit_geometry_host.py::test_some_column_needs_the_clamp_of_the_last_edge asserts that (B - 1) * by > q occurs among them;
  bins_phi_linear returns y[B-2] as yright: the "above" plants, 8191 .. 200 000, and the phi_linear comparison itself;
  cov_expected reads beta[k] for beta[k + 1]: test_cov_emissions_match_the_checker at K >= 1 (expected_cov bit for bit);
  k_emit_bins stops its 32-tile walk one tile early: the count of ~200 000 that lane 0 of every sample block puts into tile 31 at
      E = 130 and 258 (asserted by test_tile_placement_of_the_counts_beyond_the_table).
"""
import math

import numpy as np
import pytest

import emit_geometry_cases as gc
from test_gpu_parity import bits

pytestmark = pytest.mark.gpu

FIT_REL_TOL = 1e-7       # tests/test_gpu_bins.py
_CACHE = {}


# ---------------------------------------------------------------------------------------------------------------------------
# expectations (checker only; shared between the tests and with tests/test_emit_geometry_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def bins_case(idx, ood_sample=None, seed=None):
    E, S, B, sizes = gc.BINS_SHAPES[idx]
    seed = 100 + idx if seed is None else seed
    return cached(("bins", idx, ood_sample, seed), lambda: gc.bins_emit_case(E, S, B, sizes, seed, ood_sample=ood_sample))


def phi_linear_expect(case):
    """bins_oracle.approx_linear on the mid-points, per sample (evaluated once per distinct reference count)"""
    from oracle import bins_oracle as bo
    out = np.empty((case["E"], case["S"]))
    for s in range(case["S"]):
        u, inv = np.unique(case["ref"][:, s], return_inverse=True)
        out[:, s] = bo.approx_linear(u.astype(np.float64), gc.midpoints(case["edges"][:, s]), case["phi_bins"][:, s])[inv.ravel()]
    return out


def emit_expect(oracle, case, phi_es, exp_es, mix=None, calls=True):
    """the checker's likelihoods (E, 3, S), GSL error counts (S), paths (E, S) and call tables for per-cell phi and expected"""
    E, S = case["E"], case["S"]
    ll = np.empty((E, 3, S)); nerr = np.zeros(S, dtype=np.int64); path = np.zeros((E, S), dtype=np.int8); tabs = []
    for s in range(S):
        m = 1.0 if mix is None else float(mix[s])
        l, nerr[s] = oracle.get_loglike_matrix(phi_es[:, s], exp_es[:, s], case["test"][:, s] + case["ref"][:, s], case["test"][:, s], m,
                                               oracle.PORTABLE)
        ll[:, :, s] = l
        if calls:
            path[:, s], c = oracle.callcnvs(l, case["chrom_off"], case["start"], case["end"])
            tabs.append(c)
    return {"ll": ll, "nerr": nerr, "path": path, "calls": tabs}


def bins_expect(oracle, case, key, mix=None, calls=True):
    def make():
        philin = phi_linear_expect(case)
        out = emit_expect(oracle, case, philin, np.repeat(case["expected"][None, :], case["E"], axis=0), mix, calls)
        out["philin"] = philin
        return out
    return cached(("bins_expect", key, None if mix is None else tuple(mix)), make)


def same_or_both_nan(got, want):
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def check_emissions(got, want, S, nan_ok=False, table=True):
    ll, path, calls, info = got
    if nan_ok:
        ok = same_or_both_nan(ll, want["ll"])
    else:
        ok = bits(ll) == bits(want["ll"])
    assert np.all(ok), "likelihood: %d cells differ, first (exon, state, sample) %s" % ((~ok).sum(), np.argwhere(~ok)[:4].tolist())
    if not table:
        return 0
    bad = np.argwhere(path.astype(np.int8) != want["path"])
    assert bad.size == 0, "path: first (exon, sample) %s" % bad[:4].tolist()
    assert len(info) == len(calls)
    k = 0
    for s in range(S):
        m, w = calls[calls["sample"] == s], want["calls"][s]
        assert len(m) == len(w), "sample %d" % s
        assert np.array_equal(m["start_exon"] + 1, w[:, 0].astype(np.int64))
        assert np.array_equal(m["end_exon"] + 1, w[:, 1].astype(np.int64))
        assert np.array_equal(m["type"], w[:, 2].astype(np.int64))
        k += len(m)
    assert k == len(calls)
    return k


class BinsRun:
    """a plan and a batch of one shape; run(case) -> (loglik, path, calls, info)"""

    def __init__(self, edlib, case):
        self.ed = edlib
        self.plan = edlib.Plan(case["chrom_off"], case["start"], case["end"])
        self.batch = edlib.Batch(self.plan, case["S"])

    def run(self, case, mix="keep"):
        ed, b = self.ed, self.batch
        if mix is None or isinstance(mix, np.ndarray):
            b.set_mixture(mix)
        self.d = [ed.DeviceArray(case["phi_bins"]), ed.DeviceArray(case["edges"]), ed.DeviceArray(case["expected"])]
        b.run_bins(case["test"], case["ref"], case["B"], *self.d)
        return b.loglik(), b.path(), b.calls(), b.call_info()

    def phi_linear(self, case):
        return self.batch.phi_linear(case["ref"], case["B"], self.d[0], self.d[1])

    def close(self):
        self.batch.close(); self.plan.close()


# ---------------------------------------------------------------------------------------------------------------------------
# 1. emissions of the depth-binned model, hand-set parameters
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(len(gc.BINS_SHAPES)), ids=["%dx%d" % s[:2] for s in gc.BINS_SHAPES])
def test_bins_emissions_match_the_checker(edlib, oracle, idx):
    case = bins_case(idx)
    want = bins_expect(oracle, case, ("shape", idx))
    r = BinsRun(edlib, case)
    got = r.run(case)
    philin = r.phi_linear(case)
    nerr = r.batch.n_gsl_errors()
    r.close()
    assert np.array_equal(bits(philin), bits(want["philin"]))
    n = check_emissions(got, want, case["S"])
    assert nerr == int(want["nerr"].sum()) == 0
    if case["E"] >= 130:
        assert n > 0


def test_bins_out_of_domain_sample_goes_through_the_cold_path(edlib, oracle):
    """sample 70 (second sample block) has a level dispersion of 1.5: over a range of reference counts its table entries are not
    finite, those cells are left to k_emit_bins and evaluated by lnbeta_cold -- NaN where the checker has NaN, the checker's bits
    elsewhere, the checker's number of GSL errors"""
    case = bins_case(4, ood_sample=70)
    want = bins_expect(oracle, case, ("ood", 4), calls=False)
    r = BinsRun(edlib, case)
    got = r.run(case)
    nerr = r.batch.n_gsl_errors()
    r.close()
    check_emissions(got, want, case["S"], nan_ok=True, table=False)
    print("GSL errors: device %d, checker %d" % (nerr, int(want["nerr"].sum())))
    assert int(want["nerr"].sum()) > 0
    assert nerr == int(want["nerr"].sum())


@pytest.mark.parametrize("idx", [3, 4], ids=["5x63", "130x130"])
def test_bins_per_sample_mixture(edlib, oracle, idx):
    case = bins_case(idx)
    mix = gc.mixtures(case["S"])
    r = BinsRun(edlib, case)
    got = r.run(case, mix=mix)
    check_emissions(got, bins_expect(oracle, case, ("shape", idx), mix=mix), case["S"])
    got = r.run(case, mix=None)                       # set_mixture(None): the scalar argument counts again
    check_emissions(got, bins_expect(oracle, case, ("shape", idx)), case["S"])
    r.close()


def test_bins_batch_carries_nothing_over(edlib, oracle):
    """A, then B (other levels, other parameters, an out-of-domain sample: another table, other left_out bytes), then A on one batch"""
    a = bins_case(4)
    E, S, _, sizes = gc.BINS_SHAPES[4]
    b = cached(("bins", "reuse"), lambda: dict(gc.bins_emit_case(E, S, 3, sizes, 177, ood_sample=3, placed=False),
                                               chrom_off=a["chrom_off"], start=a["start"], end=a["end"]))
    r = BinsRun(edlib, a)
    first = r.run(a)
    second = r.run(b)
    third = r.run(a)
    r.close()
    check_emissions(first, bins_expect(oracle, a, ("shape", 4)), S)
    check_emissions(second, bins_expect(oracle, b, ("reuse",), calls=False), S, nan_ok=True, table=False)
    for x, y in zip(first, third):
        assert x.tobytes() == y.tobytes()


def test_bins_grid_fold(edlib, oracle):
    """E = 262 145: 65 537 exon blocks, gridDim.z = 2 in k_emit_bins_tab (blockIdx.y + blockIdx.z * 65535) and, with the cells beyond the
    table in the first and the last block, workgroups 0 and 2048 of k_emit_bins' walk.  Likelihoods and paths of both samples."""
    case = cached(("fold",), gc.bins_fold_case)
    want = bins_expect(oracle, case, ("fold",))
    r = BinsRun(edlib, case)
    got = r.run(case)
    r.close()
    check_emissions(got, want, case["S"])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. emissions of the covariate model, hand-set parameters
# ---------------------------------------------------------------------------------------------------------------------------
def cov_case(idx):
    E, S, K, sizes = gc.COV_SHAPES[idx]
    return cached(("cov", idx), lambda: gc.cov_emit_case(E, S, K, sizes, 200 + idx))


def cov_expect(oracle, case, key, mix=None):
    def make():
        expd, _ = gc.cov_restate_expected(case["X"], case["beta"], oracle.pexp)
        out = emit_expect(oracle, case, np.repeat(case["phi"][None, :], case["E"], axis=0), expd, mix)
        out["expected"] = expd
        return out
    return cached(("cov_expect", key, None if mix is None else tuple(mix)), make)


def _run_cov(edlib, case, mix=None):
    plan = edlib.Plan(case["chrom_off"], case["start"], case["end"])
    b = edlib.Batch(plan, case["S"])
    if mix is not None:
        b.set_mixture(mix)
    dbeta, dphi = edlib.DeviceArray(case["beta"]), edlib.DeviceArray(case["phi"])
    b.run_cov(case["test"], case["ref"], case["X"], dbeta, dphi)
    got = b.loglik(), b.path(), b.calls(), b.call_info()
    expd = b.expected_cov(case["X"], dbeta)
    b.close(); plan.close()
    return got, expd


def _check_cov(case, got, expd, want):
    assert np.array_equal(bits(expd), bits(want["expected"]))        # -ffp-contract=off: the restated order of operations, bit for bit
    n = check_emissions(got, want, case["S"])
    tot = (case["test"].astype(np.int64) + case["ref"]).astype(np.float64)
    for c, f in zip(got[2], got[3]):                                  # reads.expected of EVERY call (R/class_definition.R:398)
        s, a, b = int(c["sample"]), int(c["start_exon"]), int(c["end_exon"])
        assert f["reads_expected"] == int(math.fsum(tot[a:b + 1, s] * want["expected"][a:b + 1, s])), (s, a, b)
    return n


@pytest.mark.parametrize("idx", range(len(gc.COV_SHAPES)), ids=["%dx%d-K%d" % s[:3] for s in gc.COV_SHAPES])
def test_cov_emissions_match_the_checker(edlib, oracle, idx):
    case = cov_case(idx)
    got, expd = _run_cov(edlib, case)
    n = _check_cov(case, got, expd, cov_expect(oracle, case, idx))
    if case["E"] >= 130:
        assert n > 0


def test_cov_per_sample_mixture(edlib, oracle):
    case = cov_case(2)
    mix = gc.mixtures(case["S"])
    got, expd = _run_cov(edlib, case, mix)
    assert _check_cov(case, got, expd, cov_expect(oracle, case, 2, mix=mix)) > 0


# ---------------------------------------------------------------------------------------------------------------------------
# 3. fits over sample-block and chunk edges
# ---------------------------------------------------------------------------------------------------------------------------
def one_chromosome(E):
    st = (np.arange(E, dtype=np.int64) * 1000).astype(np.int32)
    return np.array([0, E], dtype=np.int32), st, st + 100


def _fit_bins(edlib, test, ref, B, form):
    E, S = test.shape
    plan = edlib.Plan(*one_chromosome(E))
    batch = edlib.Batch(plan, S)
    batch.set_fit_histograms(form)
    d = [edlib.DeviceArray(np.zeros((B, S))), edlib.DeviceArray(np.zeros((B + 1, S))), edlib.DeviceArray(np.zeros(S))]
    batch.fit_bins(test, ref, B, *d)
    took = batch.fit_bins_form
    out = [x.to_host() for x in d]
    batch.close(); plan.close()
    return took, out


def _check_fit_bins(test, ref, B, out, cols, label):
    from oracle import bins_oracle as bo
    phib, edges, exp = out
    for s in range(test.shape[1]):                    # complete.bins of EVERY column, bit for bit
        complete, _ = bo.depth_bins(ref[:, s], B)
        assert np.array_equal(bits(edges[:, s]), bits(complete)), (label, s, edges[:, s], complete)
    worst = [0.0, 0.0]
    res = []
    for s in cols:
        ophi, op, _, _ = bo.fit_bins(test[:, s], ref[:, s], B)
        res.append((s, np.max(np.abs(phib[:, s] - ophi) / ophi), abs(exp[s] - op) / op))
        worst = [max(worst[0], res[-1][1]), max(worst[1], res[-1][2])]
    print("%s: worst relative error phi_bins %.3g, expected %.3g" % (label, worst[0], worst[1]))
    for s, ephi, eexp in res:
        assert ephi < FIT_REL_TOL and eexp < FIT_REL_TOL, (label, s, ephi, eexp)


@pytest.mark.parametrize("i", range(len(gc.FIT_BINS)), ids=["E%d-S%d-B%d-form%d" % c for c in gc.FIT_BINS])
def test_fit_bins_over_block_and_chunk_edges(edlib, oracle, i):
    E, S, B, form = gc.FIT_BINS[i]
    test, ref = gc.fit_bins_case(**gc.fit_bins_args(i))
    took, out = _fit_bins(edlib, test, ref, B, form)
    assert took == form
    _check_fit_bins(test, ref, B, out, gc.check_cols(S), "E%d S%d B%d form %d" % (E, S, B, form))


@pytest.mark.parametrize("i", range(len(gc.FIT_COV)), ids=["E%d-S%d-K%d" % c for c in gc.FIT_COV])
def test_fit_cov_over_block_and_chunk_edges(edlib, oracle, i):
    E, S, K = gc.FIT_COV[i]
    X, test, ref = gc.fit_cov_case(E, S, K, 950 + i)
    plan = edlib.Plan(*one_chromosome(E))
    batch = edlib.Batch(plan, S)
    dbeta = edlib.DeviceArray(np.zeros((K + 1, S))); dphi = edlib.DeviceArray(np.zeros(S))
    batch.fit_cov(test, ref, X, dbeta, dphi)
    beta, phi = dbeta.to_host(), dphi.to_host()
    batch.close(); plan.close()
    res = []
    for s in gc.check_cols(S):
        obeta, ophi, _, _ = oracle.fit_mle_cov(test[:, s], ref[:, s], X)
        res.append((s, np.max(np.abs(beta[:, s] - obeta) / np.maximum(1.0, np.abs(obeta))), abs(phi[s] - ophi) / ophi))
    print("E%d S%d K%d: worst error beta %.3g (scaled), phi %.3g (relative)" % (E, S, K, max(r[1] for r in res), max(r[2] for r in res)))
    for s, eb, ep in res:
        assert eb < 1e-7 and ep < 1e-6, (s, eb, ep)


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
def test_histogram_form_at_the_end_of_its_reference_bins(edlib, oracle, outside):
    """csrc/edbins_hist.inc, k_lh_select:
        if (y == kLhY - 1 && k1 >= (int64_t)pre[kLhY][lane]) { atomicOr(flags, (int)LH_FLAG_QUANTILE); ...
    pre[kLhY] is the number of reference counts below 8192 (k_lh_rhist: `if ((unsigned)r < (unsigned)kLhKq) atomicAdd(...) else ++bey`)
    and k1 the 0-based rank of the upper order statistic: with exactly k1 + 1 counts below 8192 (the statistic is 8191) the form holds,
    with exactly k1 in one column it declines for the call."""
    test, ref = gc.quantile_edge_case(outside)
    took, out = _fit_bins(edlib, test, ref, 3, 1)
    assert took == (0 if outside else 1)
    _check_fit_bins(test, ref, 3, out, range(test.shape[1]), "quantile %s the bins" % ("outside" if outside else "inside"))


def test_histogram_form_declines_when_the_list_runs_out(edlib, oracle):
    """more than kLhListTotal = 32 768 cells of one sample with a test count outside the 1024 y bins"""
    test, ref = cached(("list",), gc.list_overflow_case)
    took, out = _fit_bins(edlib, test, ref, 3, 1)
    assert took == 0
    _check_fit_bins(test, ref, 3, out, [0], "list overflow")


def test_histogram_form_declines_for_a_count_of_two_to_the_28(edlib, oracle):
    """one test count of 2^28 in column 1: the form declines for the call and every column is still the checker's"""
    test, ref = gc.range_case()
    took, out = _fit_bins(edlib, test, ref, 3, 1)
    assert took == 0
    _check_fit_bins(test, ref, 3, out, range(test.shape[1]), "count of 2^28")


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the cohort's cut launch
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,pieces", [(6, None), (130, 1), (130, 3), (130, 256)], ids=["E6-default", "E130-1", "E130-3", "E130-256"])
def test_cohort_piece_arithmetic(edlib, oracle, E, pieces):
    """Cohort(phi_bins = 3), two slabs in flight, slabs of 65 samples.  E = 6: 2 exon blocks under the default 10 pieces (the launch is
    cut into min(pieces, blocks)); E = 130: 33 blocks in 1, 3 and (clamped) 33 pieces.  Each slab against the checker fed the slab's own
    fitted parameters."""
    B, n = 3, gc.COHORT_SLAB
    chrom_off, start, end, slabs = cached(("cohort", E), lambda: gc.cohort_case(E))
    plan = edlib.Plan(chrom_off, start, end)
    co = edlib.Cohort(plan, n, 2, phi_bins=B)
    if pieces is not None:
        co.set_option("bins_pieces", pieces)
    dev = [(edlib.DeviceArray(t), edlib.DeviceArray(r)) for t, r in slabs]
    tickets, got = [], []
    for i, (dt, dr) in enumerate(dev):
        if len(tickets) >= 2:
            got.append(co.results(tickets[len(got)], n, path=True, loglik=True))
        tickets.append(co.submit(dt, dr, n_samples=n))
    while len(got) < len(tickets):
        got.append(co.results(tickets[len(got)], n, path=True, loglik=True))
    co.close(); plan.close()
    total = 0
    for i, g in enumerate(got):
        case = {"E": E, "S": n, "B": B, "chrom_off": chrom_off, "start": start, "end": end, "test": slabs[i][0], "ref": slabs[i][1],
                "phi_bins": g["phi_bins"], "edges": g["edges"], "expected": g["expected"]}
        assert np.all(np.isfinite(g["phi_bins"])) and np.all(np.isfinite(g["edges"])) and np.all(np.isfinite(g["expected"]))
        want = emit_expect(oracle, case, phi_linear_expect(case), np.repeat(g["expected"][None, :], E, axis=0))
        total += check_emissions((g["loglik"], g["path"], g["calls"], g["info"]), want, n)
    if E >= 130:
        assert total > 0
