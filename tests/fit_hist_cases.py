"""Inputs of tests/test_gpu_fit_edges.py: the histogram form of the single-dispersion fit (csrc/edfit_hist.inc: k_fit_hist, k_fit_hist_sm,
k_fit_hnewton, k_fit_hnm, three geometries each) with counts placed ON the edges of its bins, lists, chunks and walks.  numpy only: the
constants of the source restated (tests/test_fit_hist_cases_host.py checks them against the source text), a host restatement of where a cell
goes (route), on which overflow list (region), whether a sample's lists run out (ran_out) and how many bins leave the LDS early (carries),
a column builder, and the catalogue.  Every case is a function of its name; tests/test_fit_hist_cases_host.py verifies on the CPU, with the
checker alone, that each case is what the GPU test takes it for and that the checker's MLE of each column moves by far more than the GPU
test's bar when a planted cell moves by one count, a cell is lost or a run of rows is counted twice."""
import zlib
from functools import lru_cache

import numpy as np

# ---- constants (csrc/edfit_hist.inc unless said otherwise; the line each comes from is quoted in test_fit_hist_cases_host.py) --------------
GEOMETRIES = (8, 4, 2)      # ED_HG_KS: samples per workgroup of k_fit_hist (hg8::, hg4::, hg2::)
HIST_BLOCK = 1024           # kHistBlock
HIST_HALVES = 2             # kHistHalves
HIST_CHUNK = 65535          # kHistChunk: rows between two flushes of k_fit_hist's 16-bit bins
SM_CHUNK = 49152 - 1024     # kSmChunk = 48 128: rows between two looks at k_fit_hist_sm's bins
SM_HOT = 0x4000             # kSmHot = 16 384: a bin at or beyond it at the end of a chunk leaves the LDS
SM_CARRY = 128              # kSmCarry: bins that can leave; one more and the sample is summed cell by cell
HS_BLOCK = 256              # kHsBlock: threads (= list regions in use) of k_fit_hist_sm
HN_S = 4                    # kHnS: samples per workgroup of k_fit_hnewton / k_fit_hnm
SPAN32 = HS_BLOCK * 4       # exons per vector span, int32 counts (four per lane and load)
SPAN16 = HS_BLOCK * 8       # ... uint16 counts (eight per lane and load)
DEPTH_8 = 1843              # fit_hist_geometry (csrc/ed_fit_job.hpp): depth <= 1843 -> 8, <= 2662 -> 4, else 2
DEPTH_4 = 2662


class Geo:
    """the constants of geometry g"""

    def __init__(self, g):
        self.g = g
        self.Ky = 1024 * 8 // g                 # kHistKy
        self.Kr = 4096 * 8 // g                 # kHistKr
        self.Kn = 4096 * 8 // g                 # kHistKn
        self.K2 = 3072 if g == 2 else 5120      # kOv2
        self.R0 = self.Kr - self.Ky             # kOv2R0: second-level r range [R0, R0 + K2); n range [Kn, Kn + K2)
        self.rows = HIST_BLOCK // g             # kHistRows
        self.G = HIST_HALVES * self.rows        # kHistGroups: lists per sample
        self.sm2 = g != 2                       # kSm2: k_fit_hist_sm fills the second level itself
        self.K = self.Ky + self.Kr + self.Kn    # kHistK
        self.sm_bins = self.K + (2 * self.K2 if self.sm2 else 0)   # kSmBins


GEO = {g: Geo(g) for g in GEOMETRIES}


def cap(E_max, g):
    """Launch::cap_of: cells per list of a workspace made for E_max rows (the plan's exon count)"""
    G = GEO[g].G
    return min(65535 // G, max(8, (E_max // G) // 3 + 1))


def geometry_of(depth):
    return 8 if depth <= DEPTH_8 else (4 if depth <= DEPTH_4 else 2)


def per_xcd(S, g):
    """`per` of k_fit_hist: (half, sample group) pairs each of the 8 XCDs owns"""
    return (HIST_HALVES * ((S + g - 1) // g) + 7) // 8


# ---- where a cell goes ------------------------------------------------------------------------------------------------------------------
SKIP, FIRST, MIXED, SECOND, LIST = range(5)
ROUTES = ("skip", "first", "mixed", "second", "list")


def route(y, r, g, layout):
    """route code of each cell (arrays): layout 0 -- k_fit_hist then k_fit_hnewton's re-binning of the lists; layout 1 -- k_fit_hist_sm (which
    for g = 8, 4 places each of r and n on the first level that holds it) then the same re-binning"""
    G = GEO[g]
    y = np.asarray(y, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    n = y + r
    yin = (y >= 0) & (y < G.Ky)
    r1, n1 = (r >= 0) & (r < G.Kr), (n >= 0) & (n < G.Kn)
    r2, n2 = (r >= G.R0) & (r < G.R0 + G.K2), (n >= G.Kn) & (n < G.Kn + G.K2)
    out = np.full(y.shape, LIST, dtype=np.int8)
    if layout == 1 and G.sm2:
        placed = yin & (r1 | r2) & (n1 | n2)
        out[placed] = MIXED
        out[placed & ~r1 & ~n1] = SECOND
        out[placed & r1 & n1] = FIRST
    else:
        out[yin & r2 & n2] = SECOND
        out[yin & r1 & n1] = FIRST
    out[n <= 0] = SKIP
    return out


def on_list(y, r, g, layout):
    """the cells the HISTOGRAM kernel puts on a list (what its per-list count `nov` counts and the capacity is compared with): in layout 0, and
    in layout 1 at g = 2, those include the cells k_fit_hnewton then moves to the second level"""
    c = route(y, r, g, layout)
    return (c == LIST) if (layout == 1 and GEO[g].sm2) else ((c == LIST) | (c == SECOND))


def vec_of(bits, by, pitch):
    """lanes' vector width in k_fit_hist_sm: 4 (int32), 8 (uint16) or 0 = the scalar walk serves the whole row (device pointers are 16-byte aligned)"""
    if by != 1:
        return 0
    if bits == 32:
        return 4 if pitch % 4 == 0 else 0
    return 8 if pitch % 8 == 0 else 0


def in_vector_walk(rows, E, vec):
    """layout 1: is the row met by the vector spans of its chunk (else by the scalar tail)?"""
    rows = np.asarray(rows, dtype=np.int64)
    if not vec:
        return np.zeros(rows.shape, dtype=bool)
    c0 = rows // SM_CHUNK * SM_CHUNK
    c1 = np.minimum(c0 + SM_CHUNK, E)
    span = HS_BLOCK * vec
    return (rows - c0) < (c1 - c0) // span * span


def region(rows, E, g, layout, vec=0):
    """the overflow list of the cell of each row (E: rows of the fit)"""
    rows = np.asarray(rows, dtype=np.int64)
    G = GEO[g]
    if layout == 0:
        half = (rows >= (E * 1) // HIST_HALVES).astype(np.int64)     # r0 of half 1 = E * 1 / 2
        r0 = half * ((E * 1) // HIST_HALVES)
        return half * G.rows + ((rows - r0) % HIST_CHUNK) % G.rows   # e = c0 + tid / kHistSamples + k * kHistRows, c0 = r0 + 65535 * chunk
    c0 = rows // SM_CHUNK * SM_CHUNK
    c1 = np.minimum(c0 + SM_CHUNK, E)
    o = rows - c0
    if vec:
        span = HS_BLOCK * vec
        nfull = (c1 - c0) // span
        return np.where(o < nfull * span, (o % span) // vec, (o - nfull * span) % HS_BLOCK)
    return o % HS_BLOCK


def list_counts(y, r, g, layout, vec=0):
    """cells per list after the histogram kernel, [kHistGroups]"""
    sel = np.flatnonzero(on_list(y, r, g, layout))
    return np.bincount(region(sel, len(y), g, layout, vec), minlength=GEO[g].G)


def carries(y, r, g):
    """layout 1: (bins that leave the LDS early, the largest value a 16-bit bin reaches) -- k_fit_hist_sm looks at the bins at the end of every
    chunk that another chunk follows"""
    G = GEO[g]
    y = np.asarray(y, dtype=np.int64)
    r = np.asarray(r, dtype=np.int64)
    n = y + r
    c = route(y, r, g, 1)
    placed = (c != SKIP) & ~on_list(y, r, g, 1)
    br = np.where(r < G.Kr, G.Ky + r, G.K + (r - G.R0))
    bn = np.where(n < G.Kn, G.Ky + G.Kr + n, G.K + G.K2 + (n - G.Kn))
    h = np.zeros(G.sm_bins + 2 * G.K2, dtype=np.int64)
    moved, top = 0, 0
    E = len(y)
    for c0 in range(0, max(E, 1), SM_CHUNK):
        c1 = min(c0 + SM_CHUNK, E)
        p = placed[c0:c1]
        for b in (y[c0:c1][p], br[c0:c1][p], bn[c0:c1][p]):
            h += np.bincount(b, minlength=h.size)
        top = max(top, int(h.max()))
        if c1 < E:
            hot = h >= SM_HOT
            moved += int(hot.sum())
            h[hot] = 0
    return moved, top


def ran_out(y, r, E_max, g, layout, vec=0):
    """is the sample summed cell by cell in k_fit_hnewton / k_fit_hnm: a list beyond its capacity, or (layout 1) more early movers than kSmCarry"""
    if layout == 1 and carries(y, r, g)[0] > SM_CARRY:
        return True
    return bool(np.any(list_counts(y, r, g, layout, vec) > cap(E_max, g)))


def depth_of(y, r, layout):
    """int(sum n / #{n > 0}) over the rows the starting moments read (k_fit_moments / k_fit_moments_sm with stride 4 below 65 536 rows, 16 from
    there on; fit mode 0): what k_fit_start's atomicMax takes of this sample"""
    E = len(y)
    stride = 16 if E >= 65536 else 4
    e = np.arange(E)
    seen = ((e % 256) % stride == 0) if layout == 0 else ((e // 64) % stride == 0)
    n = (np.asarray(y, dtype=np.int64) + np.asarray(r, dtype=np.int64))[seen]
    cnt = int((n > 0).sum())
    return int(float(n[n > 0].sum()) / cnt) if cnt else 0


def moment_rows(E, layout):
    stride = 16 if E >= 65536 else 4
    e = np.arange(E)
    return np.flatnonzero(((e % 256) % stride == 0) if layout == 0 else ((e // 64) % stride == 0))


# ---- the column builder -----------------------------------------------------------------------------------------------------------------
P_LOW, P_HIGH = 0.06, 0.3          # proportions: the low one keeps y inside its bins up to the far edge of the second level


def _rng(*key):
    return np.random.default_rng([zlib.crc32(repr(key).encode()), 20250])


def seg_params(k, p0=P_LOW):
    """(phi, p) of row segment k: different for every half, chunk and list region that a case tells apart, phi in [3e-3, 2e-2]"""
    return (4e-3, 8e-3, 1.2e-2, 5e-3, 1e-2, 6.5e-3)[k % 6], p0 * (1.0 + 0.07 * ((3 * k) % 5 - 2))


def bb(rng, n, phi, p):
    """beta-binomial draws y of totals n (arrays)"""
    n = np.asarray(n, dtype=np.int64)
    phi = np.broadcast_to(np.asarray(phi, dtype=np.float64), n.shape)
    p = np.broadcast_to(np.asarray(p, dtype=np.float64), n.shape)
    q = rng.beta(p * (1 - phi) / phi, (1 - p) * (1 - phi) / phi)
    return rng.binomial(n, q).astype(np.int64)


def segments(E, layout):
    """segment of each row: layout 0 -- (half, chunk of the half); layout 1 -- chunk, and inside a single chunk the two halves too (so that every
    column has two runs of rows drawn from different parameters); None (a column used in both layouts) -- the halves"""
    e = np.arange(E)
    half = (e >= E // 2).astype(np.int64)
    if layout == 1 and E > SM_CHUNK:
        return e // SM_CHUNK
    if layout == 0 and E > 2 * HIST_CHUNK:
        return half * 3 + 1 + ((e - half * (E // 2)) // HIST_CHUNK)
    return half


class Column:
    """one column of a fit: y, r (the rows fitted), the rows planted on an edge and which coordinate a one-count move shifts, the run of rows
    condition (ii) counts twice, the row it removes, and how the GPU test holds the column"""

    def __init__(self, name, y, r, planted, move="r", held=True, bar="tol", drop=None):
        self.name = name
        self.y = np.ascontiguousarray(y, dtype=np.int32)
        self.r = np.ascontiguousarray(r, dtype=np.int32)
        assert self.y.min(initial=0) >= 0 and self.r.min(initial=0) >= 0
        self.planted = np.asarray(planted, dtype=np.int64)
        self.move = move
        self.held = held                  # compared with the checker's MLE (else: finite, in range and the same bits everywhere)
        self.bar = bar                    # "tol": FIT_REL_TOL as _check_mle scales it; "hot": 1e-6 / 1e-8 (columns on few values, group D)
        self.drop = int(self.planted[len(self.planted) // 2]) if drop is None and len(self.planted) else drop    # (group D: the rows of one plateau)
        self.key = zlib.crc32(self.y.tobytes()) ^ (zlib.crc32(self.r.tobytes()) << 1) ^ len(self.y)

    # the three altered data sets of condition (ii): handed to the checker only
    def moved(self):
        y, r = self.y.copy(), self.r.copy()
        (y if self.move == "y" else r)[self.planted] += 1
        return y, r

    def dropped(self):
        return np.delete(self.y, self.drop), np.delete(self.r, self.drop)

    def twice(self, layout):
        E = len(self.y)
        run = min(max(E // 2, 1), HIST_CHUNK if layout == 0 else SM_CHUNK)
        return np.concatenate([self.y, self.y[:run]]), np.concatenate([self.r, self.r[:run]])


def body(rng, E, g, layout=None, p0=P_LOW, depth=None, sd=0.25, phi_scale=1.0):
    """E beta-binomial cells inside the first level of geometry g, each segment of rows with its own (phi, p)"""
    G = GEO[g]
    seg = segments(E, layout)
    phi = np.array([seg_params(k, p0)[0] for k in range(int(seg.max(initial=0)) + 1)])[seg] * phi_scale
    p = np.array([seg_params(k, p0)[1] for k in range(int(seg.max(initial=0)) + 1)])[seg]
    n = np.clip(rng.poisson((depth or 0.3 * G.Kn) * rng.lognormal(0.0, sd, E)), 2, G.Kn - 2).astype(np.int64)
    y = np.minimum(bb(rng, n, phi, p), G.Ky - 2)
    return y, n - y, phi, p


def quarter(rng, E, share=0.25):
    k = max(1, int(round(E * share))) if E > 1 else 0
    return np.sort(rng.choice(E, k, replace=False))


def ordinary(g, E, k, layout=None, share=0.25, p0=P_LOW):
    """a neighbour: a body of which a share of the rows has the total fixed at one first-level value (a heavy n bin), y drawn"""
    rng = _rng("ordinary", g, E, k, layout, share, p0)
    y, r, phi, p = body(rng, E, g, layout, p0=p0, depth=(0.3 - 0.02 * (k % 4)) * GEO[g].Kn)
    pl = quarter(rng, E, share)
    n0 = int(0.33 * GEO[g].Kn) + 7 * k
    y[pl] = np.minimum(bb(rng, np.full(len(pl), n0), phi[pl], p[pl]), GEO[g].Ky - 2)
    r[pl] = n0 - y[pl]
    return Column("ordinary%d" % k, y, r, pl, "r")


# ---- the catalogue ----------------------------------------------------------------------------------------------------------------------
class Case:
    """name, group, geometry asked for (8 / 4 / 2, or 1 = automatic), counts layout, count width, row step `by`, the plan's exon count E (which
    is also the row pitch of sample-major counts), columns (fitted rows: (E - 1) // by + 1 of them), the edge column's slot"""

    def __init__(self, name, group, g, layout, cols, bits=32, by=1, E=None, slot=None, runs=None):
        self.name, self.group, self.g, self.layout, self.bits, self.by, self.slot = name, group, g, layout, bits, by, slot
        self.cols = cols
        rows = len(cols[0].y)
        assert all(len(c.y) == rows for c in cols)
        self.E = E if E is not None else rows
        assert (self.E - 1) // by + 1 == rows, (name, self.E, by, rows)
        self.S = len(cols)
        self.rows = rows
        self.runs = runs                   # the geometry that runs (automatic cases); the forced one otherwise
        self.vec = vec_of(bits, by, self.E) if layout == 1 else 0

    @property
    def geometry(self):
        return self.runs if self.g == 1 else self.g

    def matrices(self):
        """(test, ref) as the library takes them: [E][S] int32, or [S][E] int32 / uint16; rows that `by` skips hold other counts"""
        t = np.zeros((self.E, self.S), dtype=np.int64)
        r = np.zeros((self.E, self.S), dtype=np.int64)
        if self.by > 1:
            rng = _rng("skipped rows", self.name)
            t[:] = rng.integers(0, 900, t.shape)
            r[:] = rng.integers(0, 3000, r.shape)
        for s, c in enumerate(self.cols):
            t[::self.by, s], r[::self.by, s] = c.y, c.r
        dt = np.int32 if self.bits == 32 else np.uint16
        assert t.max(initial=0) <= np.iinfo(dt).max and r.max(initial=0) <= np.iinfo(dt).max
        if self.layout:
            return np.ascontiguousarray(t.T.astype(dt)), np.ascontiguousarray(r.T.astype(dt))
        return t.astype(np.int32), r.astype(np.int32)

    def ran_out(self, s):
        return ran_out(self.cols[s].y, self.cols[s].r, self.E, self.geometry, self.layout, self.vec)


E_A = 2048


def edge_values(g):
    """group A: (name, coordinate, value, proportion of the planted draws, share of the rows)"""
    G = GEO[g]
    return (("n=Kn-1", "n", G.Kn - 1, P_LOW, 0.25), ("n=Kn", "n", G.Kn, P_LOW, 0.25),
            ("n=Kn+K2-1", "n", G.Kn + G.K2 - 1, P_LOW, 0.25), ("n=Kn+K2", "n", G.Kn + G.K2, P_LOW, 0.25),
            ("r=Kr-1", "r", G.Kr - 1, P_LOW, 0.25), ("r=Kr", "r", G.Kr, P_LOW, 0.25),
            ("r=R0+K2-1", "r", G.R0 + G.K2 - 1, P_LOW, 0.25), ("r=R0+K2", "r", G.R0 + G.K2, P_LOW, 0.25),
            ("y=0", "y", 0, P_HIGH, 0.25), ("y=Ky-1", "y", G.Ky - 1, P_HIGH, 0.25), ("y=Ky,small n", "y", G.Ky, P_HIGH, 0.25),
            ("y=Ky,large n", "y", G.Ky, 0.15, 0.25), ("r=0", "r", 0, P_HIGH, 0.25), ("n=0", "zero", 0, P_LOW, 0.1))


@lru_cache(maxsize=None)
def edge_column(g, edge, share=None, E=E_A):
    """the body of geometry g with a share of the rows planted on the named edge value (the other coordinate a beta-binomial draw)"""
    name, coord, v, pp, sh = [e for e in edge_values(g) if e[0] == edge][0]
    share = share or sh
    G = GEO[g]
    rng = _rng("edge", g, edge, share, E)
    high = coord == "y" or edge == "r=0"
    y, r, phi, p = body(rng, E, g, None, p0=(P_HIGH if high else P_LOW), depth=(0.15 if high else 0.3) * G.Kn)
    pl = quarter(rng, E, share)
    k = len(pl)
    pr = p[pl] * (pp / (P_HIGH if high else P_LOW))
    move = "r"
    if coord == "n":
        y[pl] = bb(rng, np.full(k, v), phi[pl], pr)
        r[pl] = v - y[pl]                                   # r := edge_n - y
    elif edge == "r=0":
        r[pl] = 0                                           # n = y
        y[pl] = np.maximum(y[pl], 1)
    elif coord == "r":
        y[pl] = bb(rng, np.full(k, int(round(v / (1 - pp)))), phi[pl], pr)
        r[pl] = v                                           # r := edge
    elif edge == "y=0":
        y[pl] = 0
        move = "y"
    elif coord == "y":
        n0 = int(round(v / pp))
        r[pl] = n0 - bb(rng, np.full(k, n0), phi[pl], pr)   # r drawn
        y[pl] = v                                           # y := edge
        move = "y"
    else:
        y[pl] = 0
        r[pl] = 0
    drop = None
    if coord == "zero":                                     # (a cell with n = 0 carries nothing: the cell condition (ii) removes is one of the body's)
        drop = int(np.setdiff1d(np.arange(E), pl)[E // 3])
    return Column(edge, y, r, pl, move, drop=drop)


@lru_cache(maxsize=None)
def group_A(share=None):
    out = []
    for g in GEOMETRIES:
        mates = [ordinary(g, E_A, k) for k in range(4)]
        for layout in (0, 1):
            for e in edge_values(g):
                col = edge_column(g, e[0], share)
                out.append(Case("A g%d layout %d %s" % (g, layout, e[0]), "A", g, layout, mates[:2] + [col] + mates[2:], slot=2))
    return tuple(out)


def E_B(g, layout):
    """ten rows per list and a ragged end (k_fit_hist: 2 * kHistRows lists; k_fit_hist_sm: its 256 threads'); cap = 8 in every geometry"""
    return 2 * 10 * (GEO[g].rows if layout == 0 else GEO[8].rows) + 37


def _far(rng, g, k, phi, p):
    """k cells beyond both levels: r >= max(R0 + K2, Kr) on a thousand values, y a draw inside its bins"""
    G = GEO[g]
    r = max(G.R0 + G.K2, G.Kr) + 11 + (rng.permutation(4 * k)[:k] % 997) * 3     # (geometry 2: R0 + K2 < Kr)
    y = np.minimum(bb(rng, np.round(r / (1 - p)).astype(np.int64), phi, p), G.Ky - 2)
    return y, r


def _second(rng, g, k, phi, p):
    """k cells of the second level: n in [Kn, Kn + K2) and r = n - y in [R0, R0 + K2)"""
    G = GEO[g]
    n = G.Kn + (G.K2 // 8 + rng.integers(0, 3 * G.K2 // 8, k) if g != 2 else rng.integers(0, 512, k))
    # (geometry 2: K2 < Ky, so r = n - y < R0 + K2 needs y > n - Kn + Ky - K2 -- a larger proportion than the body's)
    y = np.clip(bb(rng, n, phi, p if g != 2 else p * (0.16 / P_LOW)), np.maximum(1, n - (G.R0 + G.K2) + 1), G.Ky - 2)
    r = n - y
    assert np.all((r >= G.R0) & (r < G.R0 + G.K2))
    return y, r


def _rows_of_region(E, g, layout, vec, reg):
    return np.flatnonzero(region(np.arange(E), E, g, layout, vec) == reg)


def _spread(rng, E, g, layout, vec, k, per_list, avoid):
    """k rows with at most per_list of them on one list, none on list `avoid`"""
    reg = region(np.arange(E), E, g, layout, vec)
    cnt = np.zeros(GEO[g].G, dtype=np.int64)
    out = []
    for e in rng.permutation(E):
        if reg[e] != avoid and cnt[reg[e]] < per_list:
            cnt[reg[e]] += 1
            out.append(e)
            if len(out) == k:
                break
    return np.sort(np.array(out, dtype=np.int64))


@lru_cache(maxsize=None)
def list_column(g, layout, kind, share=0.25):
    """group B columns at E_B(g) rows.  kind: "cap" / "cap+1" -- one list (the last of half 0, or of thread 77) holds exactly that many cells beyond
    both levels, the others fewer than the capacity; "all" -- every cell beyond both levels; "second" -- the list cells all fall in the second level;
    "interleaved" -- one list holds second-level and residual cells in turn"""
    G = GEO[g]
    E = E_B(g, layout)
    vec = vec_of(32, 1, E) if layout else 0
    c = cap(E, g)
    rng = _rng("list", g, layout, kind, share)
    y, r, phi, p = body(rng, E, g, layout)
    target = G.rows - 1 if layout == 0 else 77
    rows_t = _rows_of_region(E, g, layout, vec, target)
    if kind in ("cap", "cap+1"):
        k = c + (kind == "cap+1")
        assert len(rows_t) >= k
        pl = np.sort(np.concatenate([rows_t[:k], _spread(rng, E, g, layout, vec, int(E * share) - k, c - 1, target)]))
        y[pl], r[pl] = _far(rng, g, len(pl), phi[pl], p[pl])
    elif kind == "all":
        y, r = _far(rng, g, E, phi, p)
        pl = quarter(rng, E, share)                         # (the planted class: another proportion, so that it is a class)
        y[pl], r[pl] = _far(rng, g, len(pl), phi[pl], 1.5 * p[pl])
    elif kind == "second":
        pl = _spread(rng, E, g, layout, vec, int(E * share), c - 1, -1)
        y[pl], r[pl] = _second(rng, g, len(pl), phi[pl], p[pl])
    else:
        assert kind == "interleaved" and len(rows_t) >= c
        rest = _spread(rng, E, g, layout, vec, int(E * share) - c, c - 1, target)
        y[rest], r[rest] = _second(rng, g, len(rest), phi[rest], p[rest])
        a, b = rows_t[0:c:2], rows_t[1:c:2]
        y[a], r[a] = _second(rng, g, len(a), phi[a], p[a])
        y[b], r[b] = _far(rng, g, len(b), phi[b], p[b])
        pl = np.sort(np.concatenate([rest, rows_t[:c]]))
    return Column("list:" + kind, y, r, pl, "r")


B_KINDS = ("cap", "cap+1", "all", "second", "interleaved")


@lru_cache(maxsize=None)
def group_B(share=0.25):
    out = []
    for g in GEOMETRIES:
        for layout in (0, 1):
            E = E_B(g, layout)
            m = [ordinary(g, E, k, layout) for k in range(2)]
            for kind in B_KINDS:
                out.append(Case("B g%d layout %d %s" % (g, layout, kind), "B", g, layout, [m[0], list_column(g, layout, kind, share), m[1]], slot=1))
            out.append(Case("B g%d layout %d pair" % (g, layout), "B", g, layout,
                            [list_column(g, layout, "cap", share), list_column(g, layout, "cap+1", share), m[0], m[1]], slot=1))
    return tuple(out)


def _sentinels(E, layout):
    """the rows next to every boundary of the walk: first and last row, both sides of the half and of each chunk boundary"""
    edges = {0, E - 1}
    if layout == 0:
        h = E // 2
        edges |= {h - 1, h}
        for base, end in ((0, h), (h, E)):
            for c in range(base + HIST_CHUNK, end, HIST_CHUNK):
                edges |= {c - 1, c}
    else:
        for c in range(SM_CHUNK, E, SM_CHUNK):
            edges |= {c - 1, c}
    return np.array(sorted(e for e in edges if 0 <= e < E), dtype=np.int64)


@lru_cache(maxsize=None)
def row_column(g, E, layout, k, top16=False, r_const=False):
    """groups C and E: a body whose boundary rows (_sentinels) are outliers -- y about twice its expectation, each on its own value -- so that a
    boundary row lost or met twice moves the MLE however long the column is; a quarter of the rows has the total fixed (a heavy bin).
    top16: one cell with r = 65 535 - y (the largest uint16 total).  r_const: r is one value in EVERY row (an r bin reaches exactly 65 535 at
    each flush of a full chunk of k_fit_hist) while y is drawn."""
    G = GEO[g]
    rng = _rng("rows", g, E, layout, k, top16, r_const)
    y, r, phi, p = body(rng, E, g, layout, depth=(0.3 - 0.02 * (k % 4)) * G.Kn)
    pl = quarter(rng, E) if E > 1 else np.array([0])
    if r_const:
        r[:] = int(0.28 * G.Kn)
        y = np.clip(bb(rng, np.round(r / (1 - p)).astype(np.int64), phi, p), 0, G.Ky - 2)
        pl = np.arange(E)
    elif E > 3:
        n0 = int(0.33 * G.Kn) + 5 * k
        y[pl] = np.minimum(bb(rng, np.full(len(pl), n0), phi[pl], p[pl]), G.Ky - 2)
        r[pl] = n0 - y[pl]
    drop = None
    if E > 4096:
        sn = _sentinels(E, layout)
        y[sn] = np.minimum(2 * y[sn] + 40 + 3 * np.arange(len(sn)), G.Ky - 2)
        drop = int(sn[len(sn) // 2 - 1])       # the last row of a chunk or half
    if top16:
        e = E // 3
        r[e] = 65535 - y[e]
    return Column("rows%d" % k, y, r, pl, "r", held=E >= 127, drop=drop)


C_ROWS_0 = ((8, (1, 2, 3, 127, 128, 129, 4 * 128 - 1, 4 * 128, 4 * 128 + 1, 2 * 4 * 128 + 1)),
            (2, (1, 2, 3, 511, 512, 513, 4 * 512 - 1, 4 * 512, 4 * 512 + 1, 2 * 4 * 512 + 1)))
C_CHUNK_0 = (2 * 65535 - 1, 2 * 65535, 2 * 65535 + 1, 2 * 65535 + 2, 4 * 65535 + 3)
C_ROWS_1 = (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3 * 1024 + 5)
C_ROWS_1V = (1028, 2056, 3080, 48128 + 1032)         # pitch = E a multiple of 4 (1028) or of 8: the vector walk serves the row, and E is no whole number of spans -- spans, then a tail
C_CHUNK_1 = (48127, 48128, 48129, 2 * 48128 + 1)
C_PITCH = ((32, 2 * 1024 + 2), (32, 48128 + 1026), (16, 2 * 2048 + 4), (16, 48128 + 2052))   # pitch = E: no multiple of 4 / of 8
C_BY = ((2, 2 * 1500 + 1), (7, 7 * 700 + 3))


@lru_cache(maxsize=None)
def group_C():
    out = []
    for g, Es in C_ROWS_0:
        for E in Es:
            out.append(Case("C g%d layout 0 E %d" % (g, E), "C", g, 0, [row_column(g, E, 0, k) for k in range(3)]))
    for E in C_CHUNK_0:
        cols = [row_column(8, E, 0, 0), row_column(8, E, 0, 1, r_const=True), row_column(8, E, 0, 2)]
        out.append(Case("C g8 layout 0 E %d (chunks)" % E, "C", 8, 0, cols))
    for bits in (32, 16):
        for E in C_ROWS_1 + C_ROWS_1V + C_CHUNK_1:
            cols = [row_column(8, E, 1, k, top16=(bits == 16 and k == 1 and E > 8)) for k in range(3)]
            out.append(Case("C g8 layout 1 %d-bit E %d" % (bits, E), "C", 8, 1, cols, bits=bits))
    for bits, E in C_PITCH:
        out.append(Case("C g8 layout 1 %d-bit pitch %d (scalar walk)" % (bits, E), "C", 8, 1, [row_column(8, E, 1, k) for k in range(3)], bits=bits))
    for by, E in C_BY:
        rows = (E - 1) // by + 1
        for layout in (0, 1):
            out.append(Case("C g8 layout %d by %d E %d" % (layout, by, E), "C", 8, layout, [row_column(8, rows, layout, 4 + k) for k in range(3)], by=by, E=E))
    return tuple(out)


def _plateau(rng, g, k, taken):
    """a count pair inside the first level for k identical rows, on bins no earlier plateau used"""
    G = GEO[g]
    while True:
        n = int(rng.integers(G.Kn // 8, G.Kn // 2))
        y = int(np.clip(bb(rng, np.array([n]), 8e-3, 0.25)[0], 1, G.Ky - 2))
        if ("y", y) not in taken and ("r", n - y) not in taken and ("n", n) not in taken:
            taken |= {("y", y), ("r", n - y), ("n", n)}
            return y, n - y


@lru_cache(maxsize=None)
def hot_column(kind):
    """group D (layout 1, geometry 8): runs of identical rows that fill a bin to a chosen count inside a chunk; the rest of each chunk is a thin
    body.  Every plateau has its own values, so the MLE is determined.  kinds: "16383|16384" -- two bins at those counts at the end of the
    first of two chunks; "64511" -- a bin left at 16 383 and then hit by every row of the next chunk; ("carries", k) -- exactly k early movers"""
    g = 8
    rng = _rng("hot", kind)
    taken = set()
    plan = []                     # per chunk: list of (rows, y, r)
    if kind == "16383|16384":
        a, b = _plateau(rng, g, 0, taken), _plateau(rng, g, 0, taken)
        plan = [[(SM_HOT - 1,) + a, (SM_HOT,) + b], []]
        tail = 3000
    elif kind == "64511":
        a = _plateau(rng, g, 0, taken)
        plan = [[(SM_HOT - 1,) + a], [(SM_CHUNK,) + a], []]
        tail = 2049
    else:
        k = kind[1]
        left = k
        while left > 0:
            a = _plateau(rng, g, 0, taken)
            if left >= 9 or left == 6:                      # two plateaus on six bins
                plan.append([(SM_HOT,) + a, (SM_HOT,) + _plateau(rng, g, 0, taken)])
                left -= 6
            elif left == 5 or left == 8:                    # two plateaus sharing their y bin: five
                r2 = a[1] + 37
                taken |= {("r", r2), ("n", a[0] + r2)}
                plan.append([(SM_HOT,) + a, (SM_HOT, a[0], r2)])
                left -= 5
            else:
                assert left in (3, 7) or left % 3 == 0, left
                plan.append([(SM_HOT,) + a])
                left -= 3
        plan.append([])
        tail = 2049
    ys, rs, pls = [], [], []
    at = 0
    for ci, runs in enumerate(plan):
        last = ci == len(plan) - 1
        rows = tail if last else SM_CHUNK
        y, r, _, _ = body(rng, rows, g, None, p0=0.25, depth=0.2 * GEO[g].Kn, sd=0.35, phi_scale=2.5)   # (spread: no bin of the body nears kSmHot over all the chunks)
        o = sum(k for k, _, _ in runs)
        assert o <= rows
        for _ in range(64):                                  # no body cell on a bin of any plateau: the plateaus' bins hold exactly what the case says
            hit_y, hit = np.zeros(rows, dtype=bool), np.zeros(rows, dtype=bool)
            for kind_, v in taken:
                if kind_ == "y":
                    hit_y |= y == v
                else:
                    hit |= {"r": r, "n": y + r}[kind_] == v
            hit_y[:o] = False
            hit[:o] = False
            if not hit.any() and not hit_y.any():
                break
            y[hit_y] += 1
            r[hit & ~hit_y] += 1
        assert not hit.any() and not hit_y.any()
        o = 0
        for k, yy, rr in runs:
            y[o:o + k], r[o:o + k] = yy, rr
            pls.append(at + np.arange(o, o + k))
            o += k
        perm = rng.permutation(rows) if o < rows else np.arange(rows)     # plateau rows scattered over the chunk's threads
        inv = np.argsort(perm)
        ys.append(y[perm]); rs.append(r[perm])
        for j in range(len(runs)):
            i = len(pls) - len(runs) + j
            pls[i] = at + inv[pls[i] - at]
        at += rows
    y, r = np.concatenate(ys), np.concatenate(rs)
    return Column("hot:%s" % (kind,), y, r, np.sort(np.concatenate(pls)), "r", bar="hot", drop=pls[-1])


D_KINDS = ("16383|16384", "64511", ("carries", SM_CARRY), ("carries", SM_CARRY + 1))


@lru_cache(maxsize=None)
def group_D():
    out = []
    for kind in D_KINDS:
        col = hot_column(kind)
        mate = row_column(8, len(col.y), 1, 9)
        out.append(Case("D %s" % (kind,), "D", 8, 1, [col, mate], slot=0))
    return tuple(out)


E_WIDTHS = ((8, (1, 3, 4, 5, 7, 8, 9, 13, 17, 33, 65)), (2, (1, 2, 3, 9)))
E_E = 1024


@lru_cache(maxsize=None)
def group_E():
    out = []
    for g, widths in E_WIDTHS:
        for S in widths:
            out.append(Case("E g%d S %d" % (g, S), "E", g, 0, [row_column(g, E_E, 0, 100 + k) for k in range(S)]))
    return tuple(out)


F_DEPTHS = (DEPTH_8, DEPTH_8 + 1, DEPTH_4, DEPTH_4 + 1)


@lru_cache(maxsize=None)
def depth_column(depth, layout, E=E_A):
    """a column whose k_fit_start depth -- int(sum n / #cells) over the rows the moments read -- is exactly `depth`: the sum is made
    depth * cells + cells // 2 by moving reference counts of rows the moments read"""
    g = geometry_of(depth)
    rng = _rng("depth", depth, layout, E)
    y, r, phi, p = body(rng, E, g, None, depth=float(depth), sd=0.05)
    rows = moment_rows(E, layout)
    want = depth * len(rows) + len(rows) // 2
    diff = want - int((y + r)[rows].sum())
    step = np.full(len(rows), diff // len(rows), dtype=np.int64)
    step[:diff - int(step.sum())] += 1
    r[rows] += step
    assert r.min() >= 0 and int((y + r)[rows].sum()) == want and depth_of(y, r, layout) == depth
    return Column("depth %d" % depth, y, r, quarter(rng, E), "r")


@lru_cache(maxsize=None)
def group_F():
    out = []
    for layout in (0, 1):
        for d in F_DEPTHS:
            shallow = [ordinary(8, E_A, 20 + k, None, p0=0.2) for k in range(4)]    # first level of every geometry
            cols = shallow[:3] + [depth_column(d, layout)] + shallow[3:]
            out.append(Case("F layout %d depth %d" % (layout, d), "F", 1, layout, cols, slot=3, runs=geometry_of(d)))
    return tuple(out)


def F_sequence(layout):
    """the batches one batch object fits in turn: shallow, deep, shallow (the hint of each fit is the depth of the one before)"""
    shallow = [ordinary(8, E_A, 20 + k, None, p0=0.2) for k in range(4)]
    deep = [depth_column(DEPTH_4 + 1, layout)] + [ordinary(2, E_A, 30 + k) for k in range(3)]
    return (Case("F seq shallow", "F", 1, layout, shallow, runs=8), Case("F seq deep", "F", 1, layout, deep, runs=2),
            Case("F seq shallow again", "F", 1, layout, shallow[::-1], runs=8))


def nothing_column(kind, E=E_A):
    y, r = np.zeros(E, dtype=np.int64), np.zeros(E, dtype=np.int64)
    if kind == "one cell":
        y[8], r[8] = 31, 402         # a row the starting moments read in both layouts
    return Column(kind, y, r, np.array([8]), "r", held=False)


@lru_cache(maxsize=None)
def group_G():
    out = []
    for g in GEOMETRIES:
        for layout in (0, 1):
            m = [ordinary(g, E_A, k) for k in range(3)]
            cols = [m[0], nothing_column("zeros"), m[1], nothing_column("one cell"), m[2]]
            out.append(Case("G g%d layout %d" % (g, layout), "G", g, layout, cols))
    return tuple(out)


def catalogue():
    return group_A() + group_B() + group_C() + group_D() + group_E() + group_F() + group_G()
