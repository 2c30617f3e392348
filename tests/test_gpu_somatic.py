"""Somatic CNV calls for cohorts of matched tumour / normal pairs, each pair at its own tumour fraction (reference
R/class_definition.R:442-461, somatic.CNV.call: new('ExomeDepth', test = tumor, reference = normal, prop.tumor) + CallCNVs(1e-4)).

The per-sample mixture (ed_batch_set_mixture, ed_cohort_submit_mix, ed_cohort_run_host_mix, ed_multi_run_host_mix, the length-S
prop.tumor of .Call("ed_call_cnvs_batch")) must give every sample exactly what the scalar path gives it with that sample's value:
likelihood bits, Viterbi path, call table and decoration -- in every emit mode, layout, wire format, slab width and lane count,
whatever the other samples' values.
"""
import os

import numpy as np
import pytest

from test_shim import MIXTURE_FMT, shim  # noqa: F401  (the module's fixture: shim/edcore_shim.c driven through SEXPs)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
LEVELS = (1.0, 0.8, 0.5, 0.3, 0.1, 0.05)


def _mixtures(S, seed):
    rng = np.random.default_rng(seed)
    m = np.array([LEVELS[i % len(LEVELS)] for i in range(S)])
    rng.shuffle(m)
    return m


def _somatic_case(E, S, seed, C_=4, K=1.0):
    """normal depth ~ tumour depth (K = 1), not the germline case's 8x aggregate reference"""
    from exomedepth_amd import synth
    chrom_off, start, end = synth.exon_design(E, C_, seed=seed)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, seed=seed, K=K, n_segments=6, mean_depth=100.0)
    return chrom_off, start, end, test, ref, p, phi


def _batch_results(edlib, plan, test, ref, phi, p, mode, mixture=1.0, per_sample=None):
    S = test.shape[1]
    b = edlib.Batch(plan, S)
    if mode:
        b.set_emit_mode(mode)
    if per_sample is not None:
        b.set_mixture(per_sample)
    b.run(test, ref, phi, p, mixture=mixture)
    out = {"loglik": b.loglik().copy(), "path": b.path().copy(), "calls": b.calls().copy(), "info": b.call_info().copy()}
    b.close()
    return out


def _rows(calls, cols):
    return np.isin(calls["sample"], np.asarray(cols))


def _assert_columns_equal(got, want, cols):
    """columns `cols` of two batch results: likelihood bits, path, call rows and their decoration"""
    cols = np.asarray(cols)
    assert got["loglik"][:, :, cols].tobytes() == want["loglik"][:, :, cols].tobytes()
    assert np.array_equal(got["path"][:, cols], want["path"][:, cols])
    rg, rw = _rows(got["calls"], cols), _rows(want["calls"], cols)
    assert got["calls"][rg].tobytes() == want["calls"][rw].tobytes()
    assert got["info"][rg].tobytes() == want["info"][rw].tobytes()


@pytest.fixture(scope="module")
def batch_case(edlib):
    chrom_off, start, end, test, ref, p, phi = _somatic_case(20000, 64, seed=41)
    m = _mixtures(64, 5)
    plan = edlib.Plan(chrom_off, start, end)
    yield edlib, plan, test, ref, p, phi, m
    plan.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_per_sample_mixture_equals_the_scalar_path_bit_for_bit(batch_case, mode):
    edlib, plan, test, ref, p, phi, m = batch_case
    got = _batch_results(edlib, plan, test, ref, phi, p, mode, mixture=0.77, per_sample=m)   # (the scalar is ignored while it is set)
    assert len(got["calls"]) > 50
    for v in np.unique(m):
        want = _batch_results(edlib, plan, test, ref, phi, p, mode, mixture=v)
        _assert_columns_equal(got, want, np.nonzero(m == v)[0])
    # the mixture does change the results on this data: the comparison can tell the values apart
    one = _batch_results(edlib, plan, test, ref, phi, p, mode, mixture=1.0)
    low = np.nonzero(m == 0.3)[0]
    assert got["loglik"][:, :, low].tobytes() != one["loglik"][:, :, low].tobytes()


def test_set_mixture_none_restores_the_scalar_and_the_self_checks_see_it(batch_case):
    edlib, plan, test, ref, p, phi, m = batch_case
    b = edlib.Batch(plan, test.shape[1])
    b.set_mixture(m)
    b.run(test, ref, phi, p)
    assert b.verify_emissions(test, ref, phi, p)[1] == 0            # (n_compared, n_mismatch, first): the per-cell check reads m too
    b.set_mixture(None)
    b.run(test, ref, phi, p, mixture=0.5)
    ll = b.loglik().copy()
    assert b.verify_emissions(test, ref, phi, p, mixture=0.5)[1] == 0
    b.close()
    want = _batch_results(edlib, plan, test, ref, phi, p, 0, mixture=0.5)
    assert ll.tobytes() == want["loglik"].tobytes()


@pytest.mark.parametrize("mode", [0, 2])
def test_batch_mates_and_order_do_not_matter(batch_case, mode):
    edlib, plan, test, ref, p, phi, m = batch_case
    S = test.shape[1]
    base = _batch_results(edlib, plan, test, ref, phi, p, mode, per_sample=m)
    perm = np.random.default_rng(9).permutation(S)
    got = _batch_results(edlib, plan, np.ascontiguousarray(test[:, perm]), np.ascontiguousarray(ref[:, perm]), phi[perm], p[perm], mode,
                         per_sample=m[perm])
    assert got["loglik"].tobytes() == base["loglik"][:, :, perm].tobytes()
    assert np.array_equal(got["path"], base["path"][:, perm])
    for k in (0, 17, S - 1):                                          # column k of the permuted run is column perm[k] of the first
        rg, rb = got["calls"]["sample"] == k, base["calls"]["sample"] == perm[k]
        a, b = got["calls"][rg].copy(), base["calls"][rb].copy()
        a["sample"] = 0; b["sample"] = 0
        assert a.tobytes() == b.tobytes() and got["info"][rg].tobytes() == base["info"][rb].tobytes()
    assert np.array_equal(np.sort(perm[got["calls"]["sample"]]), np.sort(base["calls"]["sample"]))
    # one sample's result does not move when every other sample's mixture changes
    k = 23
    m2 = np.random.default_rng(10).uniform(0.02, 1.0, S)
    m2[k] = m[k]
    other = _batch_results(edlib, plan, test, ref, phi, p, mode, per_sample=m2)
    _assert_columns_equal(other, base, [k])


def test_against_the_cpu_checker(edlib, oracle):
    """mode 0: the checker's portable arithmetic bit for bit; modes 1 / 2: within 1e-10 relative of its libm flavour; identical calls"""
    chrom_off, start, end, test, ref, p, phi = _somatic_case(6000, 24, seed=43, C_=3)
    m = _mixtures(24, 6)
    plan = edlib.Plan(chrom_off, start, end)
    for mode in (0, 1, 2):
        got = _batch_results(edlib, plan, test, ref, phi, p, mode, per_sample=m)
        for s in range(test.shape[1]):
            flav = oracle.PORTABLE if mode == 0 else oracle.LIBM
            ell, _ = oracle.get_loglike_matrix(phi[s], p[s], test[:, s] + ref[:, s], test[:, s], mixture=m[s], flavour=flav)
            if mode == 0:
                assert np.array_equal(got["loglik"][:, :, s].view(np.int64), ell.view(np.int64)), (mode, s)
            else:
                assert np.all(np.abs(got["loglik"][:, :, s] - ell) <= 1e-10 * np.abs(ell)), (mode, s)
            epath, ecalls = oracle.callcnvs(ell, chrom_off, start, end)
            assert np.array_equal(got["path"][:, s].astype(np.int8), epath), (mode, s)
            mine = got["calls"][got["calls"]["sample"] == s]
            assert (mine["start_exon"] + 1).tolist() == ecalls[:, 0].astype(int).tolist(), (mode, s)
    plan.close()


def _golden_pair():
    g = np.load(os.path.join(GOLD, "exomecount_chr1.npz"))
    counts, start, end = g["counts"], g["start"], g["end"]
    order = np.lexsort((0.5 * (start.astype(float) + end.astype(float)),))
    return counts[order], start[order].astype(np.int32), end[order].astype(np.int32)


def test_reference_counts_against_the_cpu_checker(edlib, oracle):
    """the reference's own counts (data/ExomeCount.RData, chromosome 1): Exome1 as the tumour against Exome2 as its normal, at 0.5 and 0.2"""
    counts, start, end = _golden_pair()
    E = counts.shape[0]
    tumor, normal = counts[:, 0].astype(np.int32), counts[:, 1].astype(np.int32)
    phi, pe, _, _ = oracle.fit_mle(tumor, normal)
    m = np.array([0.5, 0.2, 1.0])
    test = np.ascontiguousarray(np.repeat(tumor[:, None], 3, axis=1)); ref = np.ascontiguousarray(np.repeat(normal[:, None], 3, axis=1))
    chrom_off = np.array([0, E], np.int32)
    plan = edlib.Plan(chrom_off, start, end)
    got = _batch_results(edlib, plan, test, ref, np.full(3, phi), np.full(3, pe), 0, per_sample=m)
    paths = []
    for s in range(3):
        ell, _ = oracle.get_loglike_matrix(phi, pe, tumor + normal, tumor, mixture=m[s], flavour=oracle.PORTABLE)
        assert np.array_equal(got["loglik"][:, :, s].view(np.int64), ell.view(np.int64))
        epath, ecalls = oracle.callcnvs(ell, chrom_off, start, end)
        assert np.array_equal(got["path"][:, s].astype(np.int8), epath)
        mine = got["calls"][got["calls"]["sample"] == s]
        assert (mine["start_exon"] + 1).tolist() == ecalls[:, 0].astype(int).tolist()
        paths.append(epath)
    assert not np.array_equal(paths[0], paths[2])                    # the tumour fraction changes the calls on these counts
    plan.close()


@pytest.fixture(scope="module")
def cohort_case(edlib):
    chrom_off, start, end, test, ref, p, phi = _somatic_case(8000, 150, seed=47)
    m = _mixtures(150, 7)
    yield edlib, chrom_off, start, end, test, ref, p, phi, m


def _host(a, layout, wire):
    dt = np.int32 if wire == 4 else np.uint16
    return a.astype(dt) if layout == 0 else np.ascontiguousarray(a.T.astype(dt))


def _per_column_equal(got, want, cols, layout):
    rg, rw = _rows(got["calls"], cols), _rows(want["calls"], cols)
    assert got["calls"][rg].tobytes() == want["calls"][rw].tobytes()
    assert got["info"][rg].tobytes() == want["info"][rw].tobytes()
    pg = got["path"] if layout == 0 else got["path"].T
    pw = want["path"] if layout == 0 else want["path"].T
    assert np.array_equal(pg[:, cols], pw[:, cols])
    for k in ("phi", "expected"):
        if k in got:
            assert got[k][cols].tobytes() == want[k][cols].tobytes()


@pytest.mark.parametrize("layout,wire,emit,bins,slab,in_flight,lanes,given", [
    (0, 4, 0, 1, 64, 2, 1, True), (0, 2, 0, 1, 64, 2, 1, False), (1, 4, 2, 1, 64, 2, 1, False), (1, 2, 2, 1, 48, 6, 3, True),
    (0, 4, 0, 3, 64, 2, 1, False), (1, 4, 2, 1, 150, 2, 1, True)])
def test_cohort_host_fed_per_pair_mixtures(cohort_case, layout, wire, emit, bins, slab, in_flight, lanes, given):
    edlib, chrom_off, start, end, test, ref, p, phi, m = cohort_case
    opts = {}
    if emit:
        opts["emit_mode"] = emit
    if emit == 2 and layout == 1:
        opts["counts_layout"] = 1
    if bins > 1:
        opts["phi_bins"] = bins
    if lanes > 1:
        opts["lanes"] = lanes
    plan = edlib.Plan(chrom_off, start, end)
    co = edlib.Cohort(plan, slab, in_flight, **opts)
    th, rh = _host(test, layout, wire), _host(ref, layout, wire)
    kw = {"phi": phi, "expected": p} if given else {}
    got = co.run_host(th, rh, layout, mixture=m, want_path=True, **kw)
    assert len(got["calls"]) > 100
    for v in np.unique(m):
        want = co.run_host(th, rh, layout, mixture=float(v), want_path=True, **kw)
        _per_column_equal(got, want, np.nonzero(m == v)[0], layout)
    co.close(); plan.close()


def test_cohort_device_slabs_take_a_device_mixture_array(cohort_case):
    edlib, chrom_off, start, end, test, ref, p, phi, m = cohort_case
    plan = edlib.Plan(chrom_off, start, end)
    co = edlib.Cohort(plan, 150, 2)
    t0 = co.submit(edlib.DeviceArray(test), edlib.DeviceArray(ref), mixture=edlib.DeviceArray(m))
    t1 = co.submit(edlib.DeviceArray(test), edlib.DeviceArray(ref), mixture=0.3)     # the slot's next scalar submission is scalar again
    g0, g1 = co.results(t0, 150, path=True), co.results(t1, 150, path=True)
    co.close()
    co2 = edlib.Cohort(plan, 150, 1)
    for v in np.unique(m):
        tw = co2.submit(edlib.DeviceArray(test), edlib.DeviceArray(ref), mixture=float(v))
        want = co2.results(tw, 150, path=True)
        cols = np.nonzero(m == v)[0]
        rg, rw = _rows(g0["calls"], cols), _rows(want["calls"], cols)
        assert g0["calls"][rg].tobytes() == want["calls"][rw].tobytes() and g0["info"][rg].tobytes() == want["info"][rw].tobytes()
        assert np.array_equal(g0["path"][:, cols], want["path"][:, cols])
        if v == 0.3:
            assert g1["calls"].tobytes() == want["calls"].tobytes() and np.array_equal(g1["path"], want["path"])
    co2.close(); plan.close()


@pytest.mark.parametrize("emit", [0, 2])
def test_multi_device_per_pair_mixtures(cohort_case, emit):
    edlib, chrom_off, start, end, test, ref, p, phi, m = cohort_case
    opts = {"emit_mode": 2, "counts_layout": 1} if emit == 2 else {}
    th, rh = _host(test, 1, 4), _host(ref, 1, 4)
    outs = []
    for devices in ([0], [0, 0], [0, 0, 0]):
        md = edlib.MultiDevice(chrom_off, start, end, 48, devices=devices, **opts)
        outs.append(md.run_host(th, rh, 1, mixture=m, want_path=True))
        md.close()
    for o in outs[1:]:
        for k in ("calls", "info", "phi", "expected", "path"):
            assert o[k].tobytes() == outs[0][k].tobytes(), k
    co = edlib.Cohort(edlib.Plan(chrom_off, start, end), 48, 2, **opts)
    single = co.run_host(th, rh, 1, mixture=m, want_path=True)
    co.close()
    for k in ("calls", "info", "phi", "expected", "path"):
        assert outs[0][k].tobytes() == single[k].tobytes(), k


def test_host_entries_reject_non_finite_mixtures(cohort_case):
    edlib, chrom_off, start, end, test, ref, p, phi, m = cohort_case
    from exomedepth_amd._lib import ED_OK, lib
    import ctypes as C
    plan = edlib.Plan(chrom_off, start, end)
    co = edlib.Cohort(plan, 64, 2)
    bad = m.copy(); bad[70] = np.nan
    th, rh = _host(test, 0, 4), _host(ref, 0, 4)
    n = C.c_int64(-1)
    rc = lib().ed_cohort_run_host_mix(co.handle, C.c_void_p(th.ctypes.data), C.c_void_p(rh.ctypes.data), th.shape[1], 0, 4, None, None,
                                      bad.ctypes.data_as(C.c_void_p), None, None, None, C.byref(n))
    assert rc != ED_OK and b"not a finite number" in lib().ed_last_error() and n.value == -1
    co.close(); plan.close()


def _shim_args(sh, chrom_off, start, end, test, ref, prop, devices):
    return (sh.int_matrix(test), sh.int_matrix(ref), sh.integer(chrom_off), sh.integer(start), sh.integer(end), sh.real([1e-4]),
            sh.real([50000.0]), sh.nil, sh.nil, sh.real(prop), sh.integer([64]), sh.integer([1]), sh.integer([0]), sh.integer([1]),
            sh.integer([2]), sh.integer(devices))


def test_shim_per_pair_prop_tumor_equals_the_ctypes_path(shim, cohort_case):  # noqa: F811
    edlib, chrom_off, start, end, test, ref, p, phi, m = cohort_case
    S = test.shape[1]
    res, out, err = shim.dot_call("ed_call_cnvs_batch", *_shim_args(shim, chrom_off, start, end, test, ref, m, [0]))
    assert res is not None and err == ""
    assert out == "".join(MIXTURE_FMT % v for v in m if v != 1)     # the reference's loop of somatic.CNV.call prints one per pair
    got = shim.as_list(res)
    md = edlib.MultiDevice(chrom_off, start, end, 64, devices=[0], emit_mode=2, counts_layout=1)
    want = md.run_host(_host(test, 1, 4), _host(ref, 1, 4), 1, mixture=m, want_path=True)
    md.close()
    c, info = want["calls"], want["info"]
    assert np.array_equal(got["sample"], c["sample"] + 1) and np.array_equal(got["start.p"], c["start_exon"] + 1)
    assert np.array_equal(got["end.p"], c["end_exon"] + 1) and np.array_equal(got["type"], c["type"]) and len(c) > 100
    assert got["BF"].tobytes() == info["BF"].tobytes() and got["reads.ratio"].tobytes() == info["reads_ratio"].tobytes()
    assert np.array_equal(got["path"], want["path"].T)
    assert got["phi"].tobytes() == want["phi"].tobytes()
    assert shim.R.minir_protect_balance() == 0
    # length 1: today's path, unchanged
    res1, out1, err1 = shim.dot_call("ed_call_cnvs_batch", *_shim_args(shim, chrom_off, start, end, test, ref, [0.5], [0]))
    assert res1 is not None and err1 == "" and out1 == MIXTURE_FMT % 0.5
    md = edlib.MultiDevice(chrom_off, start, end, 64, devices=[0], emit_mode=2, counts_layout=1)
    w1 = md.run_host(_host(test, 1, 4), _host(ref, 1, 4), 1, mixture=0.5, want_path=True)
    md.close()
    g1 = shim.as_list(res1)
    assert np.array_equal(g1["start.p"], w1["calls"]["start_exon"] + 1) and np.array_equal(g1["path"], w1["path"].T)
    cols = np.nonzero(m == 0.5)[0]
    assert np.array_equal(got["path"][:, cols], g1["path"][:, cols])
    assert S == 150


def test_somatic_cnv_call_mirror(edlib, oracle):
    import contextlib
    import io
    counts, start, end = _golden_pair()
    n = 6000
    tumor, normal = counts[:n, 0].astype(float), counts[:n, 1].astype(float)
    start, end = start[:n], end[:n]
    chrom = ["1"] * n
    names = ["e%d" % i for i in range(n)]
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()) as msg:
        x = edlib.somatic_CNV_call(normal, tumor, 0.4, chrom, start, end, names)
        y = edlib.ExomeDepth(tumor, normal, prop_tumor=0.4).CallCNVs(chrom, start, end, names, transition_probability=1e-4)
    assert msg.getvalue().splitlines() == ["Warning: this function is largely untested and experimental", "Initializing the exomeDepth object",
                                           "Now calling the CNVs"]
    assert isinstance(x, edlib.ExomeDepth) and x.prop_tumor == 0.4
    assert x.likelihood.tobytes() == y.likelihood.tobytes() and x.CNV_calls == y.CNV_calls and len(x.CNV_calls) > 0
    L, _ = oracle.get_loglike_matrix(x.phi[0], x.expected[0], (tumor + normal).astype(np.int32), tumor.astype(np.int32), 0.4, oracle.PORTABLE)
    assert np.array_equal(x.likelihood.view(np.int64), np.ascontiguousarray(L).view(np.int64))
    epath, ecalls = oracle.callcnvs(L, np.array([0, n], np.int32), start, end)
    assert np.array_equal(x.Viterbi_path, epath)
    assert [c["start.p"] for c in x.CNV_calls] == ecalls[:, 0].astype(int).tolist()
