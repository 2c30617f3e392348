"""The batched Viterbi, trace-back and call kernels (k_viterbi, k_viterbi_sm, k_emit_viterbi, k_tb_maps / k_tb_chain / k_tb_paths,
k_scan_counts, k_calls_fill, k_call_info) swept over chain geometry.

Everything that is hard about these kernels is data movement keyed to a chain's length and position: 16-step words, a 32-step
register ring, tiles issued in pairs with a partial tail, cooperative loads past a chromosome's end, rows that start at an odd
exon, groups of 16 words in the trace-back, chains cut into 8 runs by the call table, a persistent grid whose waves take several
items in turn.  The layouts here put a chromosome length on every one of those boundaries, at every alignment, and the counts make
every exon matter: about half of the exons are in a CNV state, in blocks of a few exons, and every exon has its own gap to the
next, so that an emission, a row of log-transitions, a back-pointer or a packed state that is moved, dropped or read from a
neighbouring row changes the answer.

What is compared, for EVERY (sample, chromosome) chain of every configuration: the path against the checker's Viterbi on that
batch's own likelihood matrix, the call table field by field against the checker's and against a run-length encoding of the path
done here in numpy, the decoration of every call, and the likelihoods (strict mode: the checker's bits; table modes: 1e-10).

The richness of the inputs is a condition (`_assert_rich`), computed on the CPU from the checker's output and asserted before any
device result is looked at.  A state change "inside" a word is a position x of that word whose state differs from exon x - 1
(for the one-exon last word of a chain of 16 k + 1 exons that is the change at the word boundary itself).

Layouts (chromosome sizes in order, 0 = an empty chromosome) are built by `_layouts`.  The overlap groups of a batch come from
fixed cut sets (at most 5 groups), so more than 8 groups in flight -- the queue-counter pairs are shared modulo 8 -- cannot be
produced through the interface and are not covered here.

Measured on an MI355X when this file was written (test_report prints the figures of a run with -s): 127 configurations of
test_every_chain_against_the_checker compare 504 444 (sample, chromosome) chains; state changes at (0.3, 2000): at least one per 4.1
exons in every sample; over the samples of a layout at (0.05, 3000) one per 11.2 or denser, at (1e-4, 5e4) one per 23.8 or denser
(worst single sample there: one per 30.7); the file takes 38 s of the suite's 283 s, 4 s of it in the checker (8 threads).
The S x mode grid is thinned, the chromosome sizes are not: every mode runs the edges layout at S = 1, 17, 65, 130 (the strict
modes at all eight widths), the strict two-kernel path and the timed mode at all three settings and the others in rotation; the long
and the many-chromosome layouts run fewer widths per mode (`_cases`).

Value-only mutants of the kernels (built aside, each run once) and the tests of this file that failed on them:
  k_viterbi_sm, the ring's refill takes the neighbouring step for a tile's last slot: all 55 mode-2 configurations of
      test_every_chain_against_the_checker, test_grid_smaller_than_the_work (6 of 6), the mode-2 cases of test_a_batch_is_reusable (6)
      and of test_device_slabs_through_the_cohort;
  k_viterbi and k_viterbi_sm, the tail tile does one step too few: the 112 configurations that are not fused, the grid test (6),
      test_a_batch_is_reusable (12 of 16: not the fused ones), the cohort test;
  k_tb_chain, the state carried across a group of 16 words taken one word late: test_every_chain_against_the_checker in every
      configuration that ran (paths differ from exon 255 of the chains of more than 256 exons on); this mutant leaves the call counts
      and the packed path inconsistent, the decoration then reads records that were never written, and the run lost its device in
      the 33rd configuration -- it is not one to run again;
  k_calls_fill, a run that starts inside a CNV takes `start` from its own first exon: all 127 configurations, the grid test, all 16
      cases of test_a_batch_is_reusable, the cohort test;
  k_viterbi_sm, `v` not restarted for a wave's second item: test_grid_smaller_than_the_work (6 of 6), the 130-sample mode-2 cases
      of the many-chromosome layout (test_every_chain_against_the_checker[many-sm-l1-130-1], test_a_batch_is_reusable[many-sm*]) and
      one cohort case (six slabs in flight: waves that finish early take a second item there too)."""
import concurrent.futures
import ctypes
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REL_TOL = 1e-10   # north_star tolerance on log-likelihoods (tests/test_gpu_tables.py)
ABS_TOL = 0.0

SETTINGS = ((1e-4, 5e4), (0.05, 3000.0), (0.3, 2000.0))   # (transition probability, expected CNV length)
LOUD = 2                                                    # the setting whose conditions hold for every sample
S_MAX = 130
S_ALL = (1, 15, 16, 17, 63, 64, 65, 130)
S_THIN = (1, 17, 65, 130)
STRONG = 8000                                               # depth of a planted cell
# in-chain exon offsets a call must span: words and the ring (16 .. 96), the 8 runs of a 128-exon chain (16 .. 112), the trace-back
# groups (256 = 16 words, 272, 512, 4096 = 256 words) and, in the long chain, 32768
BOUNDS = (16, 32, 48, 64, 80, 96, 112, 128, 256, 272, 512, 4096, 32768)
CHECKER_SECONDS = [0.0]                                     # wall time spent in the checker (reported by the last test)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def close(got, want):
    both_nan = np.isnan(got) & np.isnan(want)
    return both_nan | (got == want) | (np.abs(got - want) <= np.maximum(ABS_TOL, REL_TOL * np.abs(want)))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. layouts
# ---------------------------------------------------------------------------------------------------------------------------
class Layout:
    def __init__(self, name, sizes, seed):
        self.name = name
        self.sizes = [int(n) for n in sizes]
        self.chrom_off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int32)
        self.E = int(self.chrom_off[-1])
        self.C = len(self.sizes)
        rng = np.random.default_rng(seed)
        # uneven gaps: every exon has its own row of log-transitions, so a row taken from a neighbouring step shows
        gaps = rng.integers(100, 9000, self.E).astype(np.int64)
        start = np.empty(self.E, dtype=np.int64)
        for c in range(self.C):
            lo, hi = self.chrom_off[c], self.chrom_off[c + 1]
            start[lo:hi] = 1000 + np.cumsum(gaps[lo:hi])
        assert start.max() < 2_000_000_000
        self.start = start.astype(np.int32)
        self.end = (start + rng.integers(50, 400, self.E)).astype(np.int32)
        self.chrom_of = np.repeat(np.arange(self.C), self.sizes).astype(np.int32)
        self.nonempty = [c for c in range(self.C) if self.sizes[c] > 0]


def _edge_sizes():
    s = [1, 2, 3]
    s += [n + d for n in (16, 32, 48, 64, 80, 96) for d in (-1, 0, 1)]        # words, the ring, the prologue (tiles 0-4 in flight)
    s += [127, 128, 129]                                                        # 8 words: one per run of k_calls_fill
    s += [255, 256, 257, 271, 272, 273, 511, 512, 513, 4095, 4096, 4097]       # groups of 16 words in k_tb_chain; 256 words exactly
    return s


def _layouts():
    out = {}
    # "edges": every boundary length, equal lengths (the job sort breaks ties by index), a seeded shuffle so that chromosomes start at
    # odd exons and at every residue mod 16; empty chromosomes first, last and in between; the last non-empty chromosome is the
    # shortest (1 exon) and E is not a multiple of 16
    rng = np.random.default_rng(20261016)
    sizes = _edge_sizes() + [33, 33, 16, 1, 97, 129]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    sizes.remove(1)
    for at in (29, 17, 17, 6):
        sizes.insert(at, 0)
    out["edges"] = Layout("edges", [0] + sizes + [1, 0], 1)
    # "long": one chain of more than 32 769 exons, the last and the longest; E a multiple of 16
    out["long"] = Layout("long", [7, 0, 38, 2, 135, 0, 32778], 2)
    # "many": more than 64 non-empty chromosomes (the segment ballot), more than 10 (every cut set of the overlap groups is a real
    # cut), and enough of them that k_viterbi_sm's persistent grid has more items than waves (test_grid_smaller_than_the_work)
    rng = np.random.default_rng(77)
    sizes = [int(n) for n in rng.integers(1, 72, 400)] + [130, 131, 160, 200, 255, 257, 300, 300, 129, 144]
    sizes = [sizes[i] for i in rng.permutation(len(sizes))]
    for at in (300, 120, 120, 5):
        sizes.insert(at, 0)
    out["many"] = Layout("many", [0] + sizes, 3)
    return out


LAYOUTS = _layouts()


def test_layouts_cover_the_geometry():
    """the lists hold what they are meant to hold (a property of this file, checked without the device)"""
    ed, lg, mn = LAYOUTS["edges"], LAYOUTS["long"], LAYOUTS["many"]
    assert set(_edge_sizes()) <= set(ed.sizes)
    starts = np.array([ed.chrom_off[c] for c in ed.nonempty])
    assert int(np.sum(starts % 2 == 1)) >= 8 and len(set(int(x) % 16 for x in starts)) >= 8
    for L in (ed, mn):                                                  # empty chromosomes first / between non-empty ones
        assert L.sizes[0] == 0 and any(L.sizes[c] == 0 for c in range(L.nonempty[0], L.nonempty[-1]))
    assert ed.sizes[-1] == 0 and lg.sizes[1] == 0                       # ... and last
    assert ed.sizes[ed.nonempty[-1]] == 1 == min(n for n in ed.sizes if n) and ed.E % 16 != 0      # the last is the shortest
    assert lg.sizes[lg.nonempty[-1]] == max(lg.sizes) >= 32769 and lg.E % 16 == 0                 # the last is the longest
    assert len([n for n in ed.sizes if n == 33]) >= 3 and len(set(mn.sizes)) < len(mn.nonempty)   # equal lengths
    assert len(mn.nonempty) > 64 and len(ed.nonempty) > 10
    for b in BOUNDS:                                                    # every boundary class lies inside some chain, with room
        assert any(n >= b + 8 for L in (ed, lg) for n in L.sizes), b


# ---------------------------------------------------------------------------------------------------------------------------
# 2. counts that make every exon matter
# ---------------------------------------------------------------------------------------------------------------------------
def _run_boundaries(m):
    """in-chain exons at which k_calls_fill's runs 1..7 begin (chains of at least 8 words)"""
    nw = (m + 15) // 16
    return [16 * (nw * sg // 8) for sg in range(1, 8)]


def make_counts(L, seed, S=S_MAX, depth=40.0):
    """(test, ref int32 [E][S], phi[S], p[S]).  States in geometric blocks (mean 5 exons), half of the exons in a CNV state, depth
    about 40 (64 in the long chain's layout, whose quietest setting would otherwise change state less than once per 32 exons),
    test counts binomial around the state's proportion; runs of cells without reads at chromosome starts, ends and
    across word boundaries; and, planted with deep cells as tests/test_gpu_parity.py::test_calls_across_segment_boundaries does,
    what `_assert_rich` demands of every sample at every setting."""
    rng = np.random.default_rng(seed)
    E = L.E
    p = rng.uniform(0.30, 0.50, S)
    phi = rng.uniform(5e-4, 3e-3, S)
    ratio = np.array([1.0, 0.5, 1.5])
    pp = p[None, :] * ratio[:, None] / (p[None, :] * ratio[:, None] + 1 - p[None, :])      # [state][sample]
    state = np.empty((E, S), dtype=np.int64)
    nb = E // 3 + 64
    for s in range(S):
        lens = rng.geometric(1.0 / 5.0, nb)
        st = rng.choice(np.array([0, 0, 1, 2]), nb)
        state[:, s] = np.repeat(st, lens)[:E]
    sv = np.arange(S)
    tot = rng.poisson(depth, (E, S))
    test = rng.binomial(tot, pp[state, sv[None, :]]).astype(np.int32)
    ref = (tot - test).astype(np.int32)
    t_strong = np.rint(STRONG * pp).astype(np.int32)                                        # [state][sample]

    def strong(rows, cols, st):
        """deep cells of state st (a scalar or one per column) at exons `rows` (global) of the samples `cols`"""
        rows, cols = np.atleast_1d(rows), np.atleast_1d(cols)
        if rows.size == 0 or cols.size == 0:
            return
        t = t_strong[np.broadcast_to(st, cols.shape), cols]
        test[np.ix_(rows, cols)] = t[None, :]
        ref[np.ix_(rows, cols)] = STRONG - t[None, :]

    def zero(rows, cols):
        if len(rows) and len(cols):
            test[np.ix_(rows, cols)] = 0
            ref[np.ix_(rows, cols)] = 0

    rank8 = 0       # rank among the chains of at least 8 words
    first48 = True
    first_short = True
    for c in L.nonempty:
        lo, m = int(L.chrom_off[c]), L.sizes[c]
        nw = (m + 15) // 16
        # -- cells without reads across word boundaries (emissions exactly [0, 0, 0])
        if m >= 48:
            for s in range(S):
                words = [1 + (7 * c + s) % (nw - 1)] if nw <= 64 else [w for w in range(1, nw) if (w + s) % 11 == 0]
                for w in words:
                    test[lo + 16 * w - 2:lo + 16 * w + 2, s] = 0
                    ref[lo + 16 * w - 2:lo + 16 * w + 2, s] = 0
        # -- a call across every boundary class (in shorter chains for half of the samples: the other half keep the drawn counts)
        for b in BOUNDS:
            if m >= b + 8:
                cols = sv if (b >= 4096 or nw >= 64) else sv[(c + sv) % 2 == 0]
                strong(lo + np.arange(b - 2, b + 2), cols, 1 + (c + cols + b // 16) % 2)
        # -- ... and across the place where each of k_calls_fill's runs begins
        if nw >= 8:
            rb = _run_boundaries(m)
            for s in range(S):
                for x in (rb if nw >= 64 else [rb[(rank8 + s) % 7]]):
                    if x + 2 <= m - 6:
                        strong(lo + np.arange(x - 2, x + 2), s, 1 + (s + x // 16) % 2)
            rank8 += 1
        # -- the direct deletion -> duplication switch (the second call inherits the first one's start)
        if m >= 48:
            cols = sv if first48 else sv[(c + sv) % 4 == 0]
            first48 = False
            for s in cols:
                a = lo + 19 + s % 4
                strong(a - 1, s, 0)
                strong(np.arange(a, a + 4), s, 1)
                strong(np.arange(a + 4, a + 7), s, 2)
                strong(a + 7, s, 0)
        if m >= 32:
            # -- a state change inside the first word, three ways (one with cells without reads at the chromosome's start)
            u = (c + 2 * sv) % 3
            k1 = 1 + (c + sv) % 2
            z = 1 + c % 3
            strong(lo, sv[u == 0], 0); strong(lo + np.array([1, 2]), sv[u == 0], k1[u == 0])
            strong(lo + np.array([0, 1, 2]), sv[u == 1], k1[u == 1]); strong(lo + 3, sv[u == 1], 0)
            zero(lo + np.arange(z), sv[u == 2]); strong(lo + z, sv[u == 2], 0)
            strong(lo + np.array([z + 1, z + 2]), sv[u == 2], k1[u == 2])
            # -- ... and inside the last word: a call that reaches the last exon, one that ends before it, cells without reads
            lastw = m - 16 * ((m - 1) // 16)
            v = (c + sv) % 3
            if lastw < z + 2:
                v = np.where(v == 2, 0, v)
            k2 = 1 + (c // 2 + sv) % 2
            e = lo + m
            strong(e - 2, sv[v == 0], 0); strong(e - 1, sv[v == 0], k2[v == 0])
            strong(e - 2, sv[v == 1], k2[v == 1]); strong(e - 1, sv[v == 1], 0)
            zero(np.arange(e - z, e), sv[v == 2]); strong(e - z - 1, sv[v == 2], 0)
            strong(e - z - 2, sv[v == 2], k2[v == 2])
        else:
            # -- a chain that is one CNV state from end to end
            cols = sv if first_short else sv[(c + sv) % 5 == 0]
            first_short = False
            strong(lo + np.arange(m), cols, 1 + (c + cols) % 2)
    assert test.min() >= 0 and ref.min() >= 0 and max(test.max(), ref.max()) < 65536       # (the 16-bit format holds them)
    return test, ref, phi, p


def _pool():
    return concurrent.futures.ThreadPoolExecutor(max_workers=8)      # (the checker is C behind ctypes: the threads run side by side)


def checker_loglik(oracle, test, ref, phi, p):
    """the checker's portable likelihoods [E][3][S]"""
    t0 = time.perf_counter()
    S = test.shape[1]

    def one(s):
        ll, nerr = oracle.get_loglike_matrix(phi[s], p[s], test[:, s] + ref[:, s], test[:, s], 1.0, oracle.PORTABLE)
        assert nerr == 0
        return ll
    with _pool() as ex:
        cols = list(ex.map(one, range(S)))
    CHECKER_SECONDS[0] += time.perf_counter() - t0
    return np.ascontiguousarray(np.stack(cols, axis=2))


def checker_calls(oracle, L, ll, setting):
    """the checker's Viterbi and summary on ll [E][3][S]: (path int8 [E][S], call table in the library's record format, 0-based)"""
    from exomedepth_amd.api import CALL_DTYPE
    t0 = time.perf_counter()
    S = ll.shape[2]
    tp, ln = SETTINGS[setting]
    with _pool() as ex:
        res = list(ex.map(lambda s: oracle.callcnvs(ll[:, :, s], L.chrom_off, L.start, L.end, tp, ln), range(S)))
    CHECKER_SECONDS[0] += time.perf_counter() - t0
    path = np.stack([r[0] for r in res], axis=1)
    n = [len(r[1]) for r in res]
    calls = np.zeros(sum(n), dtype=CALL_DTYPE)
    allc = np.concatenate([r[1] for r in res], axis=0)
    calls["sample"] = np.repeat(np.arange(S), n)
    calls["start_exon"] = allc[:, 0].astype(np.int64) - 1
    calls["end_exon"] = allc[:, 1].astype(np.int64) - 1
    calls["type"] = allc[:, 2].astype(np.int64)
    calls["nexons"] = allc[:, 3].astype(np.int64)
    calls["chrom"] = L.chrom_of[calls["end_exon"]]
    return path, calls


def rle_calls(L, path):
    """The call table as a run-length encoding of path [E][S], independent of the checker: a dummy normal exon closes every
    chain; a call is pushed wherever the state changes after a CNV state, covering the run of equal states that ends there; its
    start is where the path last left state 0 (a direct switch between the CNV states keeps the first call's start)."""
    from exomedepth_amd.api import CALL_DTYPE
    E, S = path.shape
    ext = np.insert(path.T.astype(np.int8), L.chrom_off[1:], 0, axis=1)          # [S][E + C]: a 0 after every chromosome
    ext = np.concatenate([np.zeros((S, 1), np.int8), ext], axis=1)               # ... and one in front
    exon = np.insert(np.arange(E), L.chrom_off[1:], -1)                          # ext column k + 1 -> exon (or -1)
    s_idx, k = np.nonzero(ext[:, 1:] != ext[:, :-1])                             # changes, ordered by (sample, position)
    before = ext[s_idx, k]
    idx = np.arange(len(k))
    left0 = np.maximum.accumulate(np.where(before == 0, idx, 0))                 # the last change that left state 0
    push = before != 0
    out = np.zeros(int(push.sum()), dtype=CALL_DTYPE)
    out["sample"] = s_idx[push]
    out["end_exon"] = exon[k[push] - 1]
    out["type"] = before[push]
    out["nexons"] = k[push] - k[idx[push] - 1]
    out["start_exon"] = exon[k[left0[push]]]
    out["chrom"] = L.chrom_of[out["end_exon"]]
    return out


def _assert_rich(L, path, calls, setting):
    """The conditions on the inputs, from the checker's path and calls.  Returns the measured figures."""
    E, S = path.shape
    sizes = np.array(L.sizes)
    change = np.zeros((E, S), dtype=bool)
    change[1:] = path[1:] != path[:-1]
    change[L.chrom_off[:-1][sizes > 0]] = False                                   # a chromosome's first exon has no exon before it
    per_sample = change.sum(axis=0)
    fig = {"E": E, "changes_min": int(per_sample.min()), "changes_max": int(per_sample.max()),
           "exons_per_change_worst_sample": round(E / max(int(per_sample.min()), 1), 2),
           "exons_per_change_all": round(E * S / max(int(per_sample.sum()), 1), 2), "calls": len(calls)}
    # -- at least one change per 32 exons; a change inside the first and inside the last word of every chain of 32 exons or more
    first = np.ones(S, dtype=bool); last = np.ones(S, dtype=bool)
    first_any = True; last_any = True
    for c in L.nonempty:
        lo, m = int(L.chrom_off[c]), L.sizes[c]
        if m < 32:
            continue
        f = change[lo:lo + 16].any(axis=0)
        l = change[lo + 16 * ((m - 1) // 16):lo + m].any(axis=0)
        first &= f; last &= l
        first_any &= bool(f.any()); last_any &= bool(l.any())
    if setting == LOUD:
        assert np.all(per_sample * 32 >= E), ("density per sample", fig)
        assert first.all() and last.all(), "a chain without a change in its first / last word"
    else:
        assert per_sample.sum() * 32 >= E * S, ("density", fig)
        assert first_any and last_any
    # -- per sample, at every setting: calls across every boundary class and every run boundary, the quirk, a call that reaches
    # -- its chain's last exon, a chain that is one CNV state from end to end
    lo_c = L.chrom_off[calls["chrom"]].astype(np.int64)
    m_c = sizes[calls["chrom"]]
    e_in = calls["end_exon"] - lo_c
    a_in = e_in - calls["nexons"] + 1                                             # the run of equal states the call closes
    for b in BOUNDS:
        if not any(n >= b + 8 for n in L.sizes):
            continue
        hit = (a_in < b) & (b <= e_in)
        assert np.all(np.bincount(calls["sample"][hit], minlength=S) > 0), ("no call across in-chain exon", b)
    nw_c = (m_c + 15) // 16
    for sg in range(1, 8):
        bx = 16 * (nw_c * sg // 8)
        hit = (nw_c >= 8) & (a_in < bx) & (bx <= e_in)
        assert np.all(np.bincount(calls["sample"][hit], minlength=S) > 0), ("no call across the beginning of run", sg)
    quirk = (calls["sample"][1:] == calls["sample"][:-1]) & (calls["start_exon"][1:] == calls["start_exon"][:-1]) & \
            (calls["type"][:-1] == 1) & (calls["type"][1:] == 2)
    assert np.all(np.bincount(calls["sample"][1:][quirk], minlength=S) > 0), "no direct deletion -> duplication switch"
    assert np.all(np.bincount(calls["sample"][e_in == m_c - 1], minlength=S) > 0), "no call reaches its chain's last exon"
    whole = (a_in == 0) & (e_in == m_c - 1)
    assert np.all(np.bincount(calls["sample"][whole], minlength=S) > 0), "no chain that is one CNV state from end to end"
    return fig


_REF = {}


def reference(oracle, lname, dset, setting):
    """checker results of data set `dset` ('A' / 'B') of a layout: dict(test, ref, phi, p, ll) and, per setting, (path, calls, fig);
    the richness conditions are asserted here, before anything from the device is compared"""
    L = LAYOUTS[lname]
    key = (lname, dset)
    if key not in _REF:
        seed = {"edges": 100, "long": 200, "many": 300}[lname] + (0 if dset == "A" else 1)
        test, ref, phi, p = make_counts(L, seed, depth=64.0 if lname == "long" else 40.0)
        _REF[key] = dict(test=test, ref=ref, phi=phi, p=p, ll=checker_loglik(oracle, test, ref, phi, p), by_setting={})
    d = _REF[key]
    if setting not in d["by_setting"]:
        path, calls = checker_calls(oracle, L, d["ll"], setting)
        fig = _assert_rich(L, path, calls, setting)
        d["by_setting"][setting] = (path, calls, fig)
    return d


@pytest.mark.parametrize("setting", range(3))
@pytest.mark.parametrize("lname", ["edges", "long", "many"])
def test_inputs_are_rich(oracle, lname, setting):
    """the conditions of `_assert_rich` hold for the committed seeds; cells without reads (emissions exactly [0, 0, 0]) sit at
    chromosome starts, at chromosome ends and across word boundaries in every sample"""
    L = LAYOUTS[lname]
    sizes = np.array(L.sizes)
    for dset in ("A", "B") if lname != "long" else ("A",):
        d = reference(oracle, lname, dset, setting)
        path, calls, fig = d["by_setting"][setting]
        print("%s/%s setting %s: %s" % (lname, dset, SETTINGS[setting], fig))
        dead = (d["test"] == 0) & (d["ref"] == 0)
        assert np.all(d["ll"].transpose(0, 2, 1)[dead] == 0.0)
        first = L.chrom_off[:-1][sizes >= 32]; last = L.chrom_off[1:][sizes >= 32] - 1
        assert dead[first].any(axis=0).all() and dead[last].any(axis=0).all()
        across = np.zeros(S_MAX, dtype=bool)
        for c in L.nonempty:
            lo = int(L.chrom_off[c])
            for w in range(1, (L.sizes[c] + 15) // 16):
                across |= dead[lo + 16 * w - 1] & dead[lo + 16 * w]
        assert across.all()


# ---------------------------------------------------------------------------------------------------------------------------
# 3. one batch against the checker
# ---------------------------------------------------------------------------------------------------------------------------
MODES = {
    "strict":        dict(),
    "strict-serial": dict(overlap=False),
    "fused":         dict(fused=True),
    "fused-noll":    dict(fused=True, keep=False),
    "tables":        dict(emit=1),
    "sm":            dict(emit=2),
    "sm-serial":     dict(emit=2, overlap=False),
    "sm-l1":         dict(emit=2, layout=1),
    "sm-l1-serial":  dict(emit=2, layout=1, overlap=False),
    "sm-u16":        dict(emit=2, layout=1, bits=16),
    "sm-u16-serial": dict(emit=2, layout=1, bits=16, overlap=False),
}


def new_batch(edlib, plan, S, mode):
    o = MODES[mode]
    b = edlib.Batch(plan, S)
    if o.get("fused"):
        b.set_fused(True)
        b.keep_loglik(o.get("keep", True))
    if o.get("emit"):
        b.set_emit_mode(o["emit"])
    if o.get("layout"):
        b.set_counts_layout(1)
    if o.get("bits"):
        b.set_counts_bits(16)
    if "overlap" in o:
        b.set_viterbi_overlap(o["overlap"])
    return b


def counts_for(mode, d, S):
    """the first S samples of a data set in the form the mode's batch takes"""
    o = MODES[mode]
    t, r = d["test"][:, :S], d["ref"][:, :S]
    if o.get("layout"):
        dt = np.uint16 if o.get("bits") else np.int32
        return np.ascontiguousarray(t.T).astype(dt), np.ascontiguousarray(r.T).astype(dt)
    return np.ascontiguousarray(t), np.ascontiguousarray(r)


def run_batch(batch, mode, d, S):
    t, r = counts_for(mode, d, S)
    batch.run(t, r, d["phi"][:S].copy(), d["p"][:S].copy())
    out = dict(path=batch.path(), calls=batch.calls(), info=batch.call_info(), n_calls=batch.n_calls())
    out["ll"] = batch.loglik() if MODES[mode].get("keep", True) else None
    return out


def check_against_checker(oracle, L, d, setting, S, mode, got):
    """every chain, every call; returns the likelihood matrix the results were checked on"""
    o = MODES[mode]
    want_path, want_calls, _ = d["by_setting"][setting]
    ll_ref = d["ll"][:, :, :S]
    test, ref, p = d["test"][:, :S], d["ref"][:, :S], d["p"][:S]
    # -- likelihoods
    if got["ll"] is None:
        ll = ll_ref                                               # (matrix not kept: path, calls and decoration against the checker's)
        same = True
    else:
        ll = got["ll"]
        same = np.array_equal(bits(ll), bits(ll_ref))
        if not o.get("emit"):
            assert same, "strict likelihoods are not the checker's bits"
        else:
            ok = close(ll, ll_ref)
            assert ok.all(), ("likelihoods beyond 1e-10", int((~ok).sum()), np.argwhere(~ok)[:3])
    # -- the path: the checker's Viterbi on this batch's own likelihoods
    if same:
        epath, ecalls = want_path[:, :S], want_calls[want_calls["sample"] < S]
    else:
        epath, ecalls = checker_calls(oracle, L, ll, setting)
    bad = np.argwhere(got["path"].astype(np.int8) != epath)
    assert len(bad) == 0, ("path differs; (chromosome, exon in it, its size, sample):", len(bad),
                           [(int(L.chrom_of[e]), int(e - L.chrom_off[L.chrom_of[e]]), L.sizes[L.chrom_of[e]], int(s)) for e, s in bad[:6]])
    # -- the call table: the checker's, field by field and in its order; its size; the run-length encoding of the path
    calls = got["calls"]
    assert len(calls) == got["n_calls"] == len(ecalls)
    for f in ("sample", "chrom", "start_exon", "end_exon", "type", "nexons"):
        assert np.array_equal(calls[f], ecalls[f]), (f, np.flatnonzero(calls[f] != ecalls[f])[:5])
    key = (calls["sample"].astype(np.int64) * (L.C + 1) + calls["chrom"]) * (L.E + 1) + calls["end_exon"]
    assert np.all(np.diff(key) > 0)                               # ordered by (sample, chromosome, position)
    assert np.array_equal(calls, rle_calls(L, got["path"]))
    # -- the decoration of EVERY call (the formulas of tests/test_gpu_parity.py::_batch_vs_oracle)
    info = got["info"]
    assert len(info) == len(calls) > 0
    s0, a, b1 = calls["sample"].astype(np.int64), calls["start_exon"].astype(np.int64), calls["end_exon"].astype(np.int64) + 1
    seg = (np.stack([a, b1], axis=1) + (s0 * (L.E + 1))[:, None]).ravel()

    def sums(cols, dtype):                                        # the sum over [a, b1) of each call's own sample column
        flat = np.zeros((cols.shape[1], L.E + 1), dtype=dtype)    # [S][E + 1]
        flat[:, :L.E] = cols.T
        return np.add.reduceat(flat.ravel(), seg)[::2]
    assert np.array_equal(info["reads_observed"], sums(test, np.int64))
    tot_p = (test + ref) * p[None, :]
    assert np.array_equal(info["reads_expected"], np.floor(sums(tot_p, np.longdouble)).astype(np.int64))
    d_del = sums(ll[:, 0, :] - ll[:, 1, :], np.longdouble)
    d_dup = sums(ll[:, 2, :] - ll[:, 1, :], np.longdouble)
    bf = (np.log10(np.e) * np.where(calls["type"] == 1, d_del, d_dup)).astype(np.float64)
    assert np.all(np.abs(info["BF_raw"] - bf) <= 1e-12 * np.maximum(1.0, np.abs(bf))), "BF_raw"
    return ll


def _cases():
    """(layout, mode, S, setting).  The strict two-kernel path and the timed mode run the edges layout at every setting; the other
    modes, and the other layouts, take the settings in rotation; the long and the many-chromosome layouts run a thinner S x mode grid."""
    out = []
    for mode in MODES:
        o = MODES[mode]
        strict = not o.get("emit") and not o.get("fused")
        k = list(MODES).index(mode)
        for i, S in enumerate(S_ALL if strict else S_THIN):
            for setting in (range(3) if mode in ("strict", "sm") else [(i + k) % 3]):
                out.append(("edges", mode, S, setting))
        if mode == "strict":
            long_s = S_ALL
        elif mode in ("strict-serial", "sm", "sm-u16-serial"):
            long_s = S_THIN
        else:
            long_s = (17, 65)
        out += [("long", mode, S, (i + k + 1) % 3) for i, S in enumerate(long_s)]
        if mode == "strict":
            many_s = (1, 16, 64, 130)
        elif mode in ("fused", "tables", "sm-l1"):
            many_s = (17, 130)
        else:
            many_s = (17,) if mode != "strict-serial" else (65,)   # (mode 2 at 130: test_grid_smaller_than_the_work)
        out += [("many", mode, S, (i + k + 2) % 3) for i, S in enumerate(many_s)]
    return out


_PLANS = {}


def plan_for(edlib, lname, setting):
    if (lname, setting) not in _PLANS:
        L = LAYOUTS[lname]
        _PLANS[(lname, setting)] = edlib.Plan(L.chrom_off, L.start, L.end, *SETTINGS[setting])
    return _PLANS[(lname, setting)]


_STRICT_LL = {}     # (layout, S) -> the strict mode's own likelihood matrix, for the comparison with mode 2's


@pytest.mark.parametrize("lname,mode,S,setting", _cases())
def test_every_chain_against_the_checker(edlib, oracle, lname, mode, S, setting):
    """One configuration: the path of every (sample, chromosome) chain, every call and its decoration, the likelihoods."""
    L = LAYOUTS[lname]
    d = reference(oracle, lname, "A", setting)                    # (asserts the richness of the inputs first)
    b = new_batch(edlib, plan_for(edlib, lname, setting), S, mode)
    try:
        got = run_batch(b, mode, d, S)
        if MODES[mode].get("keep", True) is False:
            with pytest.raises(edlib.EdError):
                b.loglik()
        assert b.n_gsl_errors() == 0
    finally:
        b.close()
    ll = check_against_checker(oracle, L, d, setting, S, mode, got)
    if mode == "strict":
        _STRICT_LL[(lname, S)] = ll
    if MODES[mode].get("emit") == 2 and (lname, S) in _STRICT_LL:       # the on-request transposition of the sample-major matrix
        assert close(ll, _STRICT_LL[(lname, S)]).all() and close(_STRICT_LL[(lname, S)], ll).all()


def test_strict_and_sample_major_likelihoods_agree(edlib, oracle):
    """the strict matrix and mode 2's (transposed on request from [S][3][Epad]) of the same data, directly"""
    for lname, S in (("edges", 65), ("long", 17), ("many", 130)):
        d = reference(oracle, lname, "A", 0)
        out = {}
        for mode in ("strict", "sm", "sm-l1"):
            b = new_batch(edlib, plan_for(edlib, lname, 0), S, mode)
            out[mode] = run_batch(b, mode, d, S)["ll"]
            b.close()
        assert np.array_equal(bits(out["strict"]), bits(d["ll"][:, :, :S]))
        for mode in ("sm", "sm-l1"):
            assert close(out[mode], out["strict"]).all() and close(out["strict"], out[mode]).all(), mode
        assert np.array_equal(bits(out["sm"]), bits(out["sm-l1"]))


# ---------------------------------------------------------------------------------------------------------------------------
# 4. the persistent grid with more items than waves; reuse of a batch; the cohort pipeline
# ---------------------------------------------------------------------------------------------------------------------------
def compute_units():
    from exomedepth_amd._lib import check, lib
    name = ctypes.create_string_buffer(256)
    cu, mem = ctypes.c_int(0), ctypes.c_size_t(0)
    check(lib().ed_device_info(0, name, 256, ctypes.byref(cu), ctypes.byref(mem)))
    return cu.value


@pytest.mark.parametrize("mode", ["sm-serial", "sm", "sm-u16-serial"])
@pytest.mark.parametrize("setting", [0, 2])
def test_grid_smaller_than_the_work(edlib, oracle, mode, setting):
    """k_viterbi_sm's persistent grid has one wave per SIMD (4 per compute unit); with more (chromosome, sample group) items than
    that, a wave takes several in turn: the restart of the recurrence, the barrier, both LDS buffers and the counters that the last
    wave resets are exercised more than once per wave.  Twice on one batch: the second launch starts from the counters the first
    left."""
    L = LAYOUTS["many"]
    S = S_MAX
    items = ((S + 15) // 16) * len(L.nonempty)
    assert items > 4 * compute_units(), (items, compute_units())
    d = reference(oracle, "many", "A", setting)
    b = new_batch(edlib, plan_for(edlib, "many", setting), S, mode)
    try:
        for _ in range(2):
            got = run_batch(b, mode, d, S)
            check_against_checker(oracle, L, d, setting, S, mode, got)
    finally:
        b.close()


def _same_results(got, want, what):
    for k in ("path", "calls", "info"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["n_calls"] == want["n_calls"]
    if want["ll"] is not None:
        assert got["ll"].tobytes() == want["ll"].tobytes(), (what, "ll")


@pytest.mark.parametrize("mode", ["strict", "strict-serial", "fused", "fused-noll", "tables", "sm", "sm-serial", "sm-u16"])
@pytest.mark.parametrize("lname", ["edges", "many"])
def test_a_batch_is_reusable(edlib, oracle, lname, mode):
    """data set A, then B (other counts, the same plan), then A again on ONE batch object: every run equals a fresh batch's.  Stale
    high bits of the packed paths, maps, group states and last states, and the queue counters of the launch before, would show.
    Then two batches of different widths on one plan, one after the other."""
    setting = LOUD
    S = 130 if lname == "many" else 65
    L = LAYOUTS[lname]
    dA, dB = reference(oracle, lname, "A", setting), reference(oracle, lname, "B", setting)
    plan = plan_for(edlib, lname, setting)
    fresh = {}
    for name, d in (("A", dA), ("B", dB)):
        b = new_batch(edlib, plan, S, mode)
        fresh[name] = run_batch(b, mode, d, S)
        b.close()
        check_against_checker(oracle, L, d, setting, S, mode, fresh[name])
    assert fresh["A"]["path"].tobytes() != fresh["B"]["path"].tobytes()
    b = new_batch(edlib, plan, S, mode)
    for name, d in (("A", dA), ("B", dB), ("A", dA), ("A", dA), ("B", dB)):
        _same_results(run_batch(b, mode, d, S), fresh[name], (name, "reused"))
    # two widths on one plan (the second is created while the first is alive), one after the other
    S2 = 17
    b2 = new_batch(edlib, plan, S2, mode)
    got2 = run_batch(b2, mode, dB, S2)
    check_against_checker(oracle, L, dB, setting, S2, mode, got2)
    _same_results(run_batch(b, mode, dA, S), fresh["A"], "wide after narrow")
    _same_results(run_batch(b2, mode, dB, S2), got2, "narrow after wide")
    b.close(); b2.close()


_SINGLE = {}


@pytest.mark.parametrize("slab", [17, 64])
@pytest.mark.parametrize("in_flight,lanes", [(1, 1), (6, 1), (6, 3)])
@pytest.mark.parametrize("emit_mode", [0, 2])
def test_device_slabs_through_the_cohort(edlib, oracle, emit_mode, in_flight, lanes, slab):
    """the edges layout as device slabs of 17 or 64 samples through the cohort pipeline, 130 samples with a ragged last slab,
    parameters given: every slab's likelihoods, paths, calls and decoration are the columns of the single 130-sample batch"""
    lname, S = "edges", S_MAX
    setting = (emit_mode // 2 + in_flight + slab) % 3
    L = LAYOUTS[lname]
    d = reference(oracle, lname, "A", setting)
    plan = plan_for(edlib, lname, setting)
    mode = "sm" if emit_mode else "strict"
    if (mode, setting) not in _SINGLE:
        b = new_batch(edlib, plan, S, mode)
        _SINGLE[(mode, setting)] = run_batch(b, mode, d, S)
        b.close()
        check_against_checker(oracle, L, d, setting, S, mode, _SINGLE[(mode, setting)])
    want = _SINGLE[(mode, setting)]
    opts = dict(emit_mode=emit_mode) if emit_mode else dict()
    if lanes != 1:
        opts["lanes"] = lanes
    co = edlib.Cohort(plan, slab, in_flight, **opts)
    slabs = [(lo, min(lo + slab, S)) for lo in range(0, S, slab)]
    assert slabs[-1][1] - slabs[-1][0] < slab

    def collect(j, ticket):
        lo, hi = slabs[j]
        got = co.results(ticket, hi - lo, path=True, loglik=True)
        assert np.array_equal(got["path"], want["path"][:, lo:hi]), ("path of slab", j)
        assert got["loglik"].tobytes() == np.ascontiguousarray(want["ll"][:, :, lo:hi]).tobytes(), ("likelihoods of slab", j)
        sel = (want["calls"]["sample"] >= lo) & (want["calls"]["sample"] < hi)
        wc = want["calls"][sel].copy(); wc["sample"] -= lo
        assert np.array_equal(got["calls"], wc), ("calls of slab", j)
        assert got["info"].tobytes() == want["info"][sel].tobytes(), ("decoration of slab", j)
    try:
        dev, tickets = [], []
        for j, (lo, hi) in enumerate(slabs):
            if len(tickets) >= in_flight:
                k = len(tickets) - in_flight
                collect(k, tickets[k])
            arrs = [edlib.DeviceArray(np.ascontiguousarray(d["test"][:, lo:hi])), edlib.DeviceArray(np.ascontiguousarray(d["ref"][:, lo:hi])),
                    edlib.DeviceArray(d["phi"][lo:hi].copy()), edlib.DeviceArray(d["p"][lo:hi].copy())]
            dev.append(arrs)
            tickets.append(co.submit(arrs[0], arrs[1], phi=arrs[2], expected=arrs[3], n_samples=hi - lo))
        for k in range(max(0, len(tickets) - in_flight), len(tickets)):
            collect(k, tickets[k])
    finally:
        co.close()


def test_report(oracle):
    """what the sweep covered (printed with -s): sizes, chains compared, the measured densities, the checker's time"""
    cases = _cases()
    chains = sum(S * len(LAYOUTS[lname].nonempty) for lname, _, S, _ in cases)
    print("configurations %d, (sample, chromosome) chains compared in them %d" % (len(cases), chains))
    for lname in ("edges", "long", "many"):
        L = LAYOUTS[lname]
        print("layout %s: E = %d, %d chromosomes (%d non-empty), sizes %s" % (lname, L.E, L.C, len(L.nonempty), L.sizes))
    for (lname, dset), d in sorted(_REF.items()):
        for setting, (_, _, fig) in sorted(d["by_setting"].items()):
            print("inputs %s/%s %s: %s" % (lname, dset, SETTINGS[setting], fig))
    print("checker wall time %.1f s (8 threads)" % CHECKER_SECONDS[0])
    for p in _PLANS.values():
        p.close()
    _PLANS.clear(); _REF.clear(); _SINGLE.clear(); _STRICT_LL.clear()
