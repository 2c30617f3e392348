"""Every device buffer, pinned block, event and stream of the library has one owner (csrc/ed_own.hpp).

The owners count what they hold (ed_live_allocations: allocations alive, their bytes; memory handed to the caller by ed_malloc /
ed_host_alloc is not counted), which makes three claims exact, unlike the device's free memory, which belongs to everybody on it:
  (a) after every object has been destroyed and the two scratches released, both figures are back where they started -- whatever lazily
      made set, workspace or grow-only buffer the objects made on the way;
  (b) in steady state nothing is allocated: the figures do not move over ten further runs of the same shapes;
  (c) a rebuilt object does not depend on what the one before it left behind: the same create -> run -> destroy cycle gives the same
      call table every time.
Small shapes only: 600 exons in 3 chromosomes, the middle one empty, 70 samples (more than one 64-sample workgroup width) and 1.
"""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, S = 600, 70
SIZES = (350, 0, 250)
B = 3                      # depth levels of the depth-binned model

_CACHE = {}


def _settle():
    """the figures are the process's: objects that earlier tests dropped without closing go now, not in the middle of a test, and the two
    process-wide scratches, which earlier tests may have left filled, start empty"""
    from exomedepth_amd import _lib
    gc.collect()
    assert _lib.lib().ed_release_scratch() == 0
    _lib.lib().ed_dropin_release()


def _live(edlib):
    from exomedepth_amd import _lib
    n, by = C.c_int64(-1), C.c_int64(-1)
    _lib.lib().ed_live_allocations(C.byref(n), C.byref(by))
    return n.value, by.value


def _design():
    if "design" not in _CACHE:
        from exomedepth_amd import synth
        chrom_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        _, start, end = synth.exon_design(E, 1, seed=7)          # positions increase along the whole design, so within every chromosome
        _CACHE["design"] = (chrom_off, start, end)
    return _CACHE["design"]


def _data(n, seed=11):
    """(test, ref int32 [E][n], phi[n], p[n]) -- deterministic, made once per width"""
    key = ("data", n, seed)
    if key not in _CACHE:
        from exomedepth_amd import synth
        test, ref, p, phi, _ = synth.counts_numpy(_design()[0], n, seed=seed, n_segments=3, mean_depth=80.0)
        _CACHE[key] = (test, ref, phi, p)
    return _CACHE[key]


def _sm(a):
    return np.ascontiguousarray(a.T)


def _drive_batches(ed, plan, n):
    """every lazily made set, workspace and grow-only buffer of a batch of n samples, once"""
    test, ref, phi, p = _data(n)
    out = []
    b = ed.Batch(plan, n)                                        # strict run; call info; the byte path on request; the [E][3][S] matrix
    b.run(test, ref, phi, p)
    out.append(b.calls()); b.call_info(); b.path(); b.loglik()
    b.close()
    b = ed.Batch(plan, n)                                        # emit mode 1: the tile tables
    b.set_emit_mode(1)
    b.run(test, ref, phi, p)
    out.append(b.calls())
    b.close()
    for layout in (0, 1):                                        # emit mode 2: the tables + the sample-major set; its row form on request
        b = ed.Batch(plan, n)
        b.set_emit_mode(2); b.set_counts_layout(layout)
        b.run(_sm(test) if layout else test, _sm(ref) if layout else ref, phi, p)
        out.append(b.calls()); b.call_info(); b.loglik(); b.path()
        if layout:                                               # the histogram fit from sample-major counts
            dphi, dexp = ed.DeviceArray(np.zeros(n)), ed.DeviceArray(np.zeros(n))
            b.fit(_sm(test), _sm(ref), dphi, dexp)
            b.fit_unconverged()
        b.close()
    for keep in (True, False):                                   # fused, with and without the likelihood matrix
        b = ed.Batch(plan, n)
        b.set_fused(True); b.keep_loglik(keep)
        b.run(test, ref, phi, p)
        out.append(b.calls())
        if keep:
            b.keep_loglik(False)                                 # the one deliberate free of the matrix
        b.close()
    for hist in (True, False):                                   # the fit: histogram form (the four histogram buffers) and per cell
        b = ed.Batch(plan, n)
        b.set_fit_histograms(hist)
        dphi, dexp = ed.DeviceArray(np.zeros(n)), ed.DeviceArray(np.zeros(n))
        b.fit(test, ref, dphi, dexp)
        b.fit_unconverged()
        b.run(test, ref, dphi, dexp)
        out.append(b.calls())
        b.close()
    b = ed.Batch(plan, n)                                        # depth-binned model: both workspaces, the table of constants
    d = [ed.DeviceArray(np.zeros((B, n))), ed.DeviceArray(np.zeros((B + 1, n))), ed.DeviceArray(np.zeros(n))]
    b.fit_bins(test, ref, B, *d)
    b.run_bins(test, ref, B, *d)
    out.append(b.calls())
    b.close()
    b = ed.Batch(plan, n)                                        # covariate model
    X = np.linspace(-0.5, 0.5, E).reshape(E, 1)
    dbeta, dphi = ed.DeviceArray(np.zeros((2, n))), ed.DeviceArray(np.zeros(n))
    b.fit_cov(test, ref, X, dbeta, dphi)
    b.run_cov(test, ref, X, dbeta, dphi)
    out.append(b.calls()); b.call_info()
    b.close()
    b = ed.Batch(plan, n)                                        # asynchronous tail: its stream and events
    b.set_async_tail(True)
    b.run(test, ref, phi, p)
    b.run(test, ref, phi, p)
    out.append(b.calls()); b.path()
    b.close()
    return out


def _cohort_host(ed, plan, n_total, **options):
    """a two-slot cohort of 70-sample slabs fed from host memory; n_total = 170 ends on a ragged slab of 30 (the slot's `odd` batch)"""
    parts = [_data(S, 11), _data(S, 12), _data(S, 13)]
    test = np.ascontiguousarray(np.concatenate([q[0] for q in parts], axis=1)[:, :n_total])
    ref = np.ascontiguousarray(np.concatenate([q[1] for q in parts], axis=1)[:, :n_total])
    phi = np.concatenate([q[2] for q in parts])[:n_total]
    p = np.concatenate([q[3] for q in parts])[:n_total]
    co = ed.Cohort(plan, S, 2, **options)
    return co, test, ref, phi, p


def test_everything_made_is_released(edlib):
    """(a) object lifetimes: count and bytes return to their starting values exactly"""
    ed = edlib
    from exomedepth_amd import _lib
    _settle()
    start = _live(ed)
    assert start[0] >= 0 and start[1] >= 0
    chrom_off, es, ee = _design()
    plan = ed.Plan(chrom_off, es, ee)
    with_plan = _live(ed)
    assert with_plan[0] == start[0] + 3 and with_plan[1] > start[1]      # the plan's three tables
    _drive_batches(ed, plan, S)
    _drive_batches(ed, plan, 1)
    assert _live(ed) == with_plan                                # every batch took what it made with it
    # cohorts fed from host memory: given parameters; fitted with three depth levels; 170 columns = two whole slabs and a ragged one
    co, test, ref, phi, p = _cohort_host(ed, plan, 170)
    got = co.run_host(test, ref, 0, phi=phi, expected=p, want_path=True)
    assert got["path"].shape == (E, 170)
    co.run_host(_sm(test[:, :140]), _sm(ref[:, :140]), 1, phi=phi[:140], expected=p[:140], want_path=True)     # the column-major path copy
    co.close()
    co, test, ref, phi, p = _cohort_host(ed, plan, 170, phi_bins=B)
    co.run_host(test, ref, 0)
    co.close()
    co, test, ref, phi, p = _cohort_host(ed, plan, 170, emit_mode=2, counts_layout=1)
    co.run_host(_sm(test), _sm(ref), 1)                          # fitted on the device, sample-major tables, 16-bit host slabs
    co.close()
    # the annotation object: its track, the grow-only work and hit blocks
    names = np.array(["1", "2", "3"])[np.repeat(np.arange(3), SIZES)]
    track = ed.Annotation(names, es, ee)
    track.overlaps(names[::3], es[::3], ee[::3] + 500, min_overlap=0.1)
    track.close()
    # the two scratches: reference sets for every sample; the two reference-shaped entries
    counts = np.ascontiguousarray(_data(S)[0] + _data(S)[1])
    ed.cohort_select_reference_sets(counts, None, 0, max_refs=8, want_reference=True)
    ll = ed.get_loglike_matrix(0.01, 0.2, np.arange(50, 150, dtype=np.int32), np.arange(10, 110, dtype=np.int32) // 5)
    T = np.array([[0.9998, 0.0001, 0.0001], [0.5, 0.5, 0.0], [0.5, 0.0, 0.5]])
    ed.viterbi_hmm(T, ll[:, [1, 0, 2]], np.arange(100, dtype=np.int32) * 1000, 50000.0)
    assert _live(ed)[0] > with_plan[0]                           # the scratches are kept between calls ...
    plan.close()
    assert _lib.lib().ed_release_scratch() == 0                  # ... until they are given back
    _lib.lib().ed_dropin_release()
    assert _live(ed) == start


def test_steady_state_allocates_nothing(edlib):
    """(b) after two warm-up runs the figures stay where they are over ten further runs of the same shapes (this cannot show a free
    followed by an equal allocation: the rule that steady-state paths never free is held by review)"""
    ed = edlib
    _settle()
    chrom_off, es, ee = _design()
    plan = ed.Plan(chrom_off, es, ee)
    test, ref, phi, p = _data(S)
    b = ed.Batch(plan, S)
    b.set_emit_mode(2)
    co, ctest, cref, cphi, cp = _cohort_host(ed, plan, 170)

    def step():
        b.run(test, ref, phi, p)
        b.calls(); b.call_info(); b.path()
        co.run_host(ctest, cref, 0, phi=cphi, expected=cp)

    step(); step()
    warm = _live(ed)
    for _ in range(10):
        step()
        assert _live(ed) == warm
    b.close(); co.close(); plan.close()


def test_rebuilt_objects_give_the_same_calls(edlib):
    """(c) five create -> run -> destroy cycles: identical call tables"""
    ed = edlib
    chrom_off, es, ee = _design()
    test, ref, phi, p = _data(S)
    first = None
    for cycle in range(5):
        plan = ed.Plan(chrom_off, es, ee)
        b = ed.Batch(plan, S)
        b.set_emit_mode(2)
        dphi, dexp = ed.DeviceArray(np.zeros(S)), ed.DeviceArray(np.zeros(S))
        b.fit(test, ref, dphi, dexp)
        b.run(test, ref, dphi, dexp)
        got = [b.calls().tobytes(), b.call_info().tobytes(), b.path().tobytes()]
        b.close()
        co, ctest, cref, _, _ = _cohort_host(ed, plan, 170)
        out = co.run_host(ctest, cref, 0)                        # fitted on the device
        got += [out["calls"].tobytes(), out["phi"].tobytes(), out["expected"].tobytes()]
        co.close(); plan.close()
        assert len(got[0]) > 0 and len(got[3]) > 0
        if first is None:
            first = got
        assert got == first, cycle
