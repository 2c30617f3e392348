"""The byte-per-exon Viterbi path [n_exons][n_samples] is made on request (csrc/edcore.hip: ensure_path, ed_batch::path_valid).

A run leaves the states packed 16 exons per word (ppath); k_path_expand turns them into the interface's `path` when somebody asks:
the device pointer (ed_batch_path), the host getter (ed_batch_copy_path), a cohort's results / batch views and its host-side
collector.  What can go wrong is the bookkeeping -- a request that does not expand, an expand of a stale ppath, an expand that is not
ordered behind the run it belongs to -- and the word edges of the expansion, so the design puts a chromosome length on every edge of
a 16-exon word and of a 4-word workgroup row (1, 15, 16, 17, 33, 255, 257, and an empty chromosome), at sample counts on both sides of
the 64-sample workgroup width (1, 63, 65).

The expected path of every column is the CPU checker's Viterbi on the checker's own likelihood matrix (portable flavour for the strict
mode, whose bits it shares; LIBM flavour, the reference's arithmetic, for the table mode), computed once per data set and shared.
Inputs are exomedepth_amd.synth's at seeds 100 / 101 (the seeds of the chain-geometry sweep's two data sets) and 102 .. 104.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 15, 16, 17, 0, 33, 255, 257)          # exons per chromosome; 0: an empty chromosome between non-empty ones
WIDTHS = (1, 63, 65)
MODES = ((0, 0), (2, 0), (2, 1))                  # (emit mode, counts layout); layout 1 ([S][E]) is served by emit mode 2 only
POISON = 0xEE                                     # not a state: a path that was not expanded after the poisoning cannot pass

_CACHE = {}


def _design():
    if "design" not in _CACHE:
        from exomedepth_amd import synth
        chrom_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
        E = int(chrom_off[-1])
        _, start, end = synth.exon_design(E, 1, seed=100)       # positions increase along the whole design, so within every chromosome
        _CACHE["design"] = (chrom_off, start, end, E)
    return _CACHE["design"]


def _data(seed, S):
    """(test, ref int32 [E][S], phi[S], p[S]) -- deterministic, made once"""
    key = ("data", seed, S)
    if key not in _CACHE:
        from exomedepth_amd import synth
        chrom_off = _design()[0]
        test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, seed=seed, n_segments=6, mean_depth=80.0)
        _CACHE[key] = (test, ref, phi, p)
    return _CACHE[key]


def _want(oracle, seed, S, mode):
    """(path uint8 [E][S], call rows per sample as sets) of the checker on its own matrix; read-only, shared by the tests"""
    key = ("want", seed, S, mode)
    if key not in _CACHE:
        chrom_off, start, end, E = _design()
        test, ref, phi, p = _data(seed, S)
        flavour = oracle.PORTABLE if mode == 0 else oracle.LIBM
        path = np.empty((E, S), dtype=np.uint8)
        calls = []
        for s in range(S):
            ell, _ = oracle.get_loglike_matrix(phi[s], p[s], test[:, s] + ref[:, s], test[:, s], 1.0, flavour)
            epath, ecalls = oracle.callcnvs(ell, chrom_off, start, end)
            path[:, s] = epath.astype(np.uint8)
            calls.append({(int(r[0]) - 1, int(r[1]) - 1, int(r[2]), int(r[3])) for r in ecalls})
        path.setflags(write=False)
        _CACHE[key] = (path, calls)
    return _CACHE[key]


def _call_sets(calls, S):
    return [{(int(r["start_exon"]), int(r["end_exon"]), int(r["type"]), int(r["nexons"])) for r in calls[calls["sample"] == s]} for s in range(S)]


def _batch(edlib, plan, S, mode, layout):
    b = edlib.Batch(plan, S)
    if mode:
        b.set_emit_mode(mode)
    if layout:
        b.set_counts_layout(layout)
    return b


def _run(b, data, layout):
    test, ref, phi, p = data
    if layout:
        test, ref = np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)
    b.run(test, ref, phi, p)


def _view(ptr, E, S):
    """torch uint8 [E][S] tensor on the library's own buffer (no copy)"""
    import torch
    from exomedepth_amd import dist as eddist
    return torch.as_tensor(eddist._DevicePointer(ptr, (E, S), "|u1"), device=torch.device("cuda", torch.cuda.current_device()))


def _poison(ptr, E, S):
    import torch
    _view(ptr, E, S).fill_(POISON)
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def plan(edlib):
    chrom_off, start, end, _ = _design()
    pl = edlib.Plan(chrom_off, start, end)
    yield pl
    pl.close()


def test_design_covers_the_edges():
    """a property of this file, checked without the device: word edges, a workgroup row's edge (4 words), an empty chromosome inside"""
    chrom_off, _, _, E = _design()
    assert {1, 15, 16, 17, 33, 255, 257} <= set(SIZES) and 0 in SIZES[1:-1]
    assert E % 16 != 0 and any(int(o) % 16 for o in chrom_off[1:-1])          # chromosomes start inside a row of the byte path
    assert max(SIZES) > 4 * 16 * 4                                            # more than one workgroup row of words


@pytest.mark.parametrize("S", WIDTHS)
@pytest.mark.parametrize("mode,layout", MODES)
def test_path_by_every_batch_route(edlib, oracle, plan, S, mode, layout):
    """host getter and device pointer against the checker; the call table does not depend on the path having been asked for; a second
    request gives the same bytes; after another run on other counts (the buffer poisoned in between) a request gives that run's path"""
    E = _design()[3]
    dA, dB = _data(100, S), _data(101, S)
    wantA, callsA = _want(oracle, 100, S, mode)
    wantB, callsB = _want(oracle, 101, S, mode)
    assert not np.array_equal(wantA, wantB)
    # a batch whose path is never asked for: calls, call counts
    quiet = _batch(edlib, plan, S, mode, layout)
    _run(quiet, dA, layout)
    n_quiet, calls_quiet = quiet.n_calls(), quiet.calls()
    assert n_quiet == sum(len(c) for c in callsA) and _call_sets(calls_quiet, S) == callsA
    # route 1: the host getter, before anything else is read
    b = _batch(edlib, plan, S, mode, layout)
    _run(b, dA, layout)
    got = b.path()
    assert np.array_equal(got, wantA), np.argwhere(got != wantA)[:8]
    assert b.n_calls() == n_quiet and b.calls().tobytes() == calls_quiet.tobytes()
    assert b.path().tobytes() == got.tobytes()                                # a second request: the same bytes
    # route 2: the device pointer, on a batch of its own
    d = _batch(edlib, plan, S, mode, layout)
    _run(d, dA, layout)
    ptr = d.device_pointers()["path"]
    assert ptr
    got_d = _view(ptr, E, S).cpu().numpy()
    assert np.array_equal(got_d, wantA), np.argwhere(got_d != wantA)[:8]
    assert d.device_pointers()["path"] == ptr and _view(ptr, E, S).cpu().numpy().tobytes() == got_d.tobytes()
    assert d.calls().tobytes() == calls_quiet.tobytes()
    # another run, other counts: the path asked for afterwards is that run's
    ptr_b = b.device_pointers()["path"]                                       # (already made: launches nothing)
    for bb, pp in ((b, ptr_b), (d, ptr)):
        _poison(pp, E, S)
        _run(bb, dB, layout)
    got = b.path()                                                            # host getter first on b ...
    assert np.array_equal(got, wantB), np.argwhere(got != wantB)[:8]
    assert d.device_pointers()["path"] == ptr                                 # ... the pointer (unchanged) first on d
    got_d = _view(ptr, E, S).cpu().numpy()
    assert np.array_equal(got_d, wantB), np.argwhere(got_d != wantB)[:8]
    assert np.array_equal(_view(ptr_b, E, S).cpu().numpy(), wantB)
    # the quiet batch runs again too and still has never been asked: the same call table as the batches that were
    _run(quiet, dB, layout)
    calls_quiet = quiet.calls()
    assert _call_sets(calls_quiet, S) == callsB
    assert b.calls().tobytes() == calls_quiet.tobytes() and d.calls().tobytes() == calls_quiet.tobytes()
    assert quiet.path().tobytes() == got.tobytes()                            # ... and a path when it finally is
    for x in (quiet, b, d):
        x.close()


def test_fused_mode_follows_the_same_rule(edlib, oracle, plan):
    """the one-kernel mode leaves the states packed as well; its path is made on request like every other mode's"""
    S, E = 65, _design()[3]
    b = edlib.Batch(plan, S)
    b.set_fused(True)
    for seed in (100, 101):
        want, calls = _want(oracle, seed, S, 0)
        if seed == 101:
            _poison(b.device_pointers()["path"], E, S)
        _run(b, _data(seed, S), 0)
        assert _call_sets(b.calls(), S) == calls
        assert np.array_equal(b.path(), want)
    b.close()


@pytest.mark.parametrize("opts", [dict(), dict(emit_mode=2, lanes=3), dict(emit_mode=2)], ids=["strict", "tables-3-lanes", "tables"])
def test_path_of_an_earlier_ticket_while_later_slabs_are_in_flight(edlib, oracle, plan, opts):
    """a cohort of three slots, five submissions: every ticket's path is asked for while the slabs submitted after it are in flight (its
    expansion has to be ordered behind ITS run, and the slot's next run behind the expansion), through results() and through the
    batch view's device pointer in turn"""
    S, E = 65, _design()[3]
    mode = opts.get("emit_mode", 0)
    seeds = (100, 101, 102, 103, 104)
    co = edlib.Cohort(plan, S, 3, **opts)
    keep, tickets = [], []

    def check(j):
        want, calls = _want(oracle, seeds[j], S, mode)
        if j % 2 == 0:
            got = co.results(tickets[j], S, path=True, info=False)
            assert _call_sets(got["calls"], S) == calls, j
            path = got["path"]
        else:
            b, _, _ = co.batch(tickets[j])
            ptr = b.device_pointers()["path"]
            assert ptr
            path = _view(ptr, E, S).cpu().numpy()
            assert np.array_equal(b.path(), path), j
        assert np.array_equal(path, want), (j, np.argwhere(path != want)[:8])

    for j, seed in enumerate(seeds):
        test, ref, phi, p = _data(seed, S)
        dev = [edlib.DeviceArray(x) for x in (test, ref, phi, p)]
        keep.append(dev)
        tickets.append(co.submit(dev[0], dev[1], dev[2], dev[3], n_samples=S))
        if j >= 2:
            check(j - 2)                       # the oldest ticket still held: two later slabs are in flight
    check(3)
    check(4)
    co.close()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("emit_mode", [0, 2])
def test_path_through_the_host_side_collector(edlib, oracle, plan, layout, emit_mode):
    """ed_cohort_run_host with the path wanted: slabs of 65 samples and a ragged last one, two slots"""
    E = _design()[3]
    S = 65
    parts = [_data(seed, S) for seed in (100, 101)] + [tuple(x[..., :30] for x in _data(102, S))]
    test, ref = (np.ascontiguousarray(np.concatenate([q[i] for q in parts], axis=1)) for i in (0, 1))
    phi, p = (np.concatenate([q[i] for q in parts]) for i in (2, 3))
    want = np.concatenate([_want(oracle, 100, S, emit_mode)[0], _want(oracle, 101, S, emit_mode)[0], _want(oracle, 102, S, emit_mode)[0][:, :30]], axis=1)
    co = edlib.Cohort(plan, S, 2, emit_mode=emit_mode)
    if layout:
        out = co.run_host(np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T), 1, phi=phi, expected=p, want_path=True)
        got = out["path"].T
    else:
        out = co.run_host(test, ref, 0, phi=phi, expected=p, want_path=True)
        got = out["path"]
    assert got.shape == (E, want.shape[1]) and np.array_equal(got, want), np.argwhere(got != want)[:8]
    co.close()
