"""Inputs and host restatements for the sweep of the table-driven emission modes (csrc/edtab.inc) over their table, window and list
edges.  No device: tests/test_table_edges_host.py checks everything here on the CPU, tests/test_gpu_table_edges.py runs it.

Restated from the device code, in numpy / Python floats (the library is built without fma contraction, so the same operations in the
same order give the same doubles; every logarithm the device takes with ed_plog is taken with the checker's plog):
  shape_params     k_sample_consts: sd = sqrt((phi e)(1 - e)), then a1, a2 per state
  tab_stats        k_tab_stats / k_tab_stats_sm: integer sums over every `step`-th 64-exon piece
  tab_dims_of      (Ly, Lr, Tm1, N0 | reason) and the windows, tail samples included
  tab_windows      (n1, n2, n3)
  SmGeometry       the block map of mode 2 (64-exon blocks per chromosome, in job order), edplan::sm_grid, the chunk of a block, the
                   wave that takes it and the strict list (blockIdx.x * 16 + wave) % 1024 its cold cells land in
  served_mask      tab_cell_served

Planted counts (plant_values) sit on every one of those edges, per sample, from the sample's own restated dims and windows; with
E >= 4096 they go into exons the statistics do not read, so they cannot move the dims they were derived from.
"""
import numpy as np

SM_ENTRIES = 6144            # kSmEntries
SM_T1_MAX = 1024             # kSmT1Max
TAIL_MEAN_OVER_WINDOW = 1.25
TAIL_MAX_COUNT = 1 << 24
TAIL_FROM = 64               # ED_DTAB_TAIL_FROM
COND_BAR = 3e-11             # kTabCondBar
FEW_READS = 15200.0          # kTabFewReads
COLD_LISTS = 1024            # kColdLists
SM_WAVES = 16                # kSmBlock / 64
NO_N0 = 0x7FFFFFFF
DEFAULT_CAPS = (4096, 32768, 8.0)      # cap_obs, cap_ref, reach of ed_batch


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------
def shape_params(phi, e, mixture=1.0):
    """(a1[3], a2[3]) as k_sample_consts forms them (state_props, shape_params of edcore.hip)"""
    with np.errstate(all="ignore"):
        phi, e, one = np.float64(phi), np.float64(e), np.float64(1.0)
        sd = np.sqrt((phi * e) * (one - e))
        a1, a2 = [], []
        for odds in (1 - 0.5 * mixture, None, 1 + 0.5 * mixture):
            ep = e if odds is None else (e * np.float64(odds)) / ((e * np.float64(odds) + one) - e)
            x = ((ep * ep) * (one - ep)) / (sd * sd) - ep
            a1.append(float(x)); a2.append(float(((one - ep) / ep) * x))
    return a1, a2


def stat_exons(E):
    """the exons k_tab_stats / k_tab_stats_sm read: every step-th piece of 64, step = 16 from 4096 exons on"""
    step = 16 if E >= 4096 else 1
    e = np.arange(E)
    return e[(e // 64) % step == 0]


def tab_stats(test, ref):
    """(sum of test counts, sum of reference counts, exons seen) per sample, from [E][S] counts; negative counts add nothing"""
    idx = stat_exons(test.shape[0])
    sy = np.maximum(test[idx].astype(np.int64), 0).sum(axis=0)
    sr = np.maximum(ref[idx].astype(np.int64), 0).sum(axis=0)
    return sy, sr, idx.size


def tab_windows(Ly, Lr):
    n1 = min(Ly, SM_T1_MAX)
    n2 = min((SM_ENTRIES - n1) // 2, Lr)
    n3 = min(SM_ENTRIES - n1 - n2, Ly + Lr)
    return n1, n2, n3


class _Bounds:
    def __init__(self, oracle):
        self.oracle = oracle

    def plog(self, x):
        return np.float64(self.oracle.plog(np.array([x], dtype=np.float64))[0])

    def cond(self, a12, amin, n):          # tab_cond_bound
        n = np.float64(n)
        x = n / (2.0 * a12)
        lg = self.plog(1.0 + x) if x > 1e-6 else x
        return 2.0 ** -51 * n * self.plog(a12 + n) / (amin * lg)

    def cond_tail(self, a12, amin, n):     # tab_cond_bound_tail
        n = np.float64(n)
        x = n / (2.0 * a12)
        lg = self.plog(1.0 + x) if x > 1e-6 else x
        return 2.0 ** -50 * (a12 + n) * self.plog(a12 + n) / (amin * lg)

    def ref0(self, a12, a2, n):            # tab_ref0_bound
        n = np.float64(n)
        x = n / a12
        lg = self.plog(1.0 + x) if x > 1e-6 else x
        return 2.0 ** -53 * (a2 + n) * (1.0 / a2 + self.plog(a12 + n) + 1.0) / (a2 * lg)


def _shape_ok(x):
    return x >= 2.0 ** -1000 and x <= 2.0 ** 1000      # (NaN: False)


def tab_dims_of(oracle, a1, a2, cflags, sy, sr, n, reach=8.0, cap_y=4096, cap_r=32768, tails=0):
    """tab_dims_of of csrc/edtab.inc: ((Ly, Lr, Tm1, N0 or reason), (n1, n2, n3, tail))"""
    B = _Bounds(oracle)
    with np.errstate(all="ignore"):
        nn = np.float64(n)
        my = np.float64(sy) / nn if n > 0 else np.float64(0.0)
        mr = np.float64(sr) / nn if n > 0 else np.float64(0.0)
        Ly = int(min(reach * my + 64.0, float(cap_y))); Lr = int(min(reach * mr + 64.0, float(cap_r)))
        Ly = (Ly + 7) & ~7; Lr = (Lr + 7) & ~7
        Ly = min(Ly, cap_y); Lr = min(Lr, cap_r)
        reason = 0
        a12s, amins, a2s = [], [], []
        for st in range(3):
            x, y = np.float64(a1[st]), np.float64(a2[st])
            xy = x + y
            if reason == 0 and cflags[st] != 0:
                reason = 1
            if reason == 0 and not (_shape_ok(x) and _shape_ok(y) and _shape_ok(xy)):
                reason = 2
            a12s.append(xy); amins.append(min(x, y) if not (np.isnan(x) or np.isnan(y)) else x); a2s.append(y)
        if reason:
            return (0, 0, 0, reason), (0, 0, 0, 0)
        win = (0, 0, 0, 0)
        tail = False
        if tails:
            w0 = tab_windows(Ly, Lr)
            ok = (my + mr) >= TAIL_MEAN_OVER_WINDOW * float(w0[2]) and min(w0) >= TAIL_FROM
            for st in range(3):
                ok = ok and B.cond(a12s[st], amins[st], w0[0] + w0[1]) <= COND_BAR and B.cond_tail(a12s[st], amins[st], w0[1]) <= COND_BAR
            if ok:
                lo, hi = w0[0] + w0[1], TAIL_MAX_COUNT
                top = all(B.cond_tail(a12s[st], amins[st], hi) <= COND_BAR for st in range(3))
                if not top:
                    while hi - lo > 8:
                        mid = lo + ((hi - lo) >> 1)
                        if all(B.cond_tail(a12s[st], amins[st], mid) <= COND_BAR for st in range(3)):
                            lo = mid
                        else:
                            hi = mid
                else:
                    lo = hi
                share = mr / max(my + mr, np.float64(1.0))
                nLr = int(min(max(np.float64(lo) * share, float(w0[1])), float(lo - w0[0]))) & ~7
                nLy = (lo - nLr) & ~7
                if nLy >= w0[0] and nLr >= w0[1]:
                    Ly, Lr, tail, win = nLy, nLr, True, w0 + (1,)
        if not tail:
            for _ in range(64):
                if all(B.cond(a12s[st], amins[st], Ly + Lr) <= COND_BAR for st in range(3)):
                    break
                if Ly <= 64 and Lr <= 64:
                    return (0, 0, 0, 3), (0, 0, 0, 0)
                if Lr >= Ly:
                    Lr = max((Lr - (Lr >> 3)) & ~7, 64)
                else:
                    Ly = max((Ly - (Ly >> 3)) & ~7, 64)
            if not all(B.cond(a12s[st], amins[st], Ly + Lr) <= COND_BAR for st in range(3)):
                return (0, 0, 0, 3), (0, 0, 0, 0)
            win = tab_windows(Ly, Lr) + (0,)
        tmin = 0.0
        for st in range(3):
            if a12s[st] > 2e3:
                tmin = max(tmin, float(np.ceil(a12s[st] * B.plog(a12s[st]) / FEW_READS)))
        if tmin > 1.0 and 4.0 * tmin > my + mr:
            return (0, 0, 0, 4), (0, 0, 0, 0)
        Tm1 = int(min(tmin - 1.0, 2147483000.0)) if tmin > 1.0 else 0
        N0 = NO_N0
        for st in range(3):
            if B.ref0(a12s[st], a2s[st], Ly - 1) <= COND_BAR:
                continue
            lo, hi = 0, Ly - 1
            while hi - lo > 1:
                mid = (lo + hi) >> 1
                if B.ref0(a12s[st], a2s[st], mid) <= COND_BAR:
                    lo = mid
                else:
                    hi = mid
            N0 = min(N0, hi)
        return (Ly, Lr, Tm1, N0), win


def restate(oracle, test, ref, phi, expected, tails, caps=DEFAULT_CAPS):
    """per sample: dims, windows, shape parameters -- without the device"""
    S = test.shape[1]
    sy, sr, n = tab_stats(test, ref)
    dims, wins, shapes = [], [], []
    for s in range(S):
        a1, a2 = shape_params(phi[s], expected[s])
        _, sites = oracle.lnbeta_sites(np.array(a1), np.array(a2), oracle.PORTABLE)
        d, w = tab_dims_of(oracle, a1, a2, [int(c != 0) for c in sites], int(sy[s]), int(sr[s]), n, caps[2], caps[0], caps[1], tails)
        dims.append(d); wins.append(w); shapes.append((a1, a2))
    return dims, wins, shapes


def served_mask(obs, ref, dims):
    """tab_cell_served for one sample's counts (a sample without tables serves nothing)"""
    Ly, Lr, Tm1, N0 = dims
    if Ly == 0:
        return np.zeros(np.shape(obs), dtype=bool)
    o, r = np.asarray(obs, dtype=np.int64), np.asarray(ref, dtype=np.int64)
    tot = o + r
    return (o >= 0) & (o < Ly) & (r >= 0) & (r < Lr) & ~((tot >= 1) & (tot <= Tm1)) & ~((r == 0) & (o >= N0))


def cold_cap_per(E, S):
    """slots of one strict list: cold_cap / 1024 of tab_setup"""
    cap = min(max(E * S // 16, 1 << 16), 1 << 28) // COLD_LISTS * COLD_LISTS
    return cap // COLD_LISTS


class SmGeometry:
    """mode 2 with ONE emission launch over all blocks (overlap groups off): which workgroup, wave and strict list take a block"""

    def __init__(self, chrom_off, S):
        chrom_off = [int(v) for v in chrom_off]
        C = len(chrom_off) - 1
        self.order = sorted((c for c in range(C) if chrom_off[c + 1] > chrom_off[c]), key=lambda c: (-(chrom_off[c + 1] - chrom_off[c]), c))
        blocks = []
        for c in self.order:
            eb, ee = chrom_off[c], chrom_off[c + 1]
            for q in range((eb // 64) * 64, ee, 64):
                blocks.append((max(q, eb), min(q + 64, ee), c))
        self.blocks = blocks
        self.S, self.E, self.nblk = S, chrom_off[-1], len(blocks)
        nsplit = max(1, min(16, (512 + S - 1) // S))
        self.nsplit = max(1, min(nsplit, self.nblk // 32))
        self.per = (self.nblk + self.nsplit - 1) // self.nsplit if self.nblk else 0
        b = np.arange(self.nblk)
        self.chunk = b // max(self.per, 1)
        self.wave = (b - self.chunk * self.per) % SM_WAVES
        self.exon_block = np.full(self.E, -1, dtype=np.int64)
        for i, (lo, hi, _) in enumerate(blocks):
            self.exon_block[lo:hi] = i
        assert (self.exon_block >= 0).all()

    def chunk_range(self, c):
        return c * self.per, min((c + 1) * self.per, self.nblk)

    def workgroup(self, s, chunk):
        return ((s // 8) * self.nsplit + chunk) * 8 + (s & 7)

    def list_of(self, s, b):
        return (self.workgroup(s, int(self.chunk[b])) * SM_WAVES + int(self.wave[b])) % COLD_LISTS

    def list_loads(self, cold):
        """cold: [E][S] mask of not-served cells of samples WITH tables -> the 1024 list loads"""
        load = np.zeros(COLD_LISTS, dtype=np.int64)
        for s in range(self.S):
            e = np.flatnonzero(cold[:, s])
            if e.size:
                b = self.exon_block[e]
                np.add.at(load, (self.workgroup(s, self.chunk[b]) * SM_WAVES + self.wave[b]) % COLD_LISTS, 1)
        return load


# ---------------------------------------------------------------------------------------------------------------------------
# planted counts
# ---------------------------------------------------------------------------------------------------------------------------
def plant_values(dims, win):
    """every (obs, ref) on an edge of one sample's tables, windows and rules (what does not exist for the sample is dropped)"""
    Ly, Lr, Tm1, N0 = dims
    if Ly == 0:
        return [(0, 0), (0, 1), (1, 0), (63, 64), (64, 63), (65, 65), (1, 1), (2, 0), (0, 70000), (4096, 3)]
    n1, n2, n3, tail = win
    obs = {0, 1, n1 - 1, n1, n1 + 1, Ly - 2, Ly - 1, Ly, Ly + 1}
    ref = {0, 1, n2 - 1, n2, n2 + 1, Lr - 2, Lr - 1, Lr, Lr + 1}
    if tail:
        obs |= {63, 64, 65}; ref |= {63, 64, 65}
    out = [(o, r) for o in sorted(obs) for r in sorted(ref)]
    tots = [n3 - 1, n3, n3 + 1]
    if tail:
        tots += [Ly + Lr - 2, Ly + Lr - 1, Ly + Lr, Ly + Lr + 1]        # either side of the served limit (2^24 where the search reached its end)
    for t in tots:
        out += [(0, t), (1, t - 1), (t // 2, t - t // 2), (min(t, Ly - 1), t - min(t, Ly - 1))]
    for t in (Tm1, Tm1 + 1, Tm1 + 2):
        out += [(o, t - o) for o in range(0, 4) if 0 <= t - o <= 3]
        if Tm1 > 0:
            out += [(0, t), (t, 0), (1, t - 1), (t // 2, t - t // 2)]
    out.append((0, 0))
    if N0 != NO_N0:
        out += [(N0 - 1, 0), (N0, 0), (N0 + 1, 0)]
    seen, uniq = set(), []
    for o, r in out:
        if o >= 0 and r >= 0 and o + r < 2 ** 31 - 1 and (o, r) not in seen:
            seen.add((o, r)); uniq.append((int(o), int(r)))
    return uniq


# the sample kinds of a multi-sample case: (kind, phi, expected, mean test depth)
N0_PAIRS = [(0.05, 0.998), (0.3, 0.9995), (0.01, 0.99), (0.1, 0.97), (0.02, 0.998), (0.15, 0.9995), (0.2, 0.99), (0.005, 0.97)]
KINDS = [("table", 0.010, 0.03, 30.0), ("table", 0.020, 0.10, 150.0), ("tail", 0.010, 0.11, 900.0), ("few", 1e-4, 0.30, 100.0),
         ("n0", N0_PAIRS[0][0], N0_PAIRS[0][1], 300.0), ("table", 0.015, 0.30, 30.0), ("notab", 1.5, 0.10, 100.0),
         ("table", 0.010, 0.50, 150.0), ("tail", 0.012, 0.30, 1600.0), ("few", 3e-4, 0.10, 100.0),
         ("n0", N0_PAIRS[1][0], N0_PAIRS[1][1], 300.0), ("table", 0.005, 0.80, 30.0), ("table", 0.030, 0.80, 150.0),
         ("tail", 0.008, 0.50, 1700.0), ("tail", 0.020, 0.05, 950.0), ("tail", 2e-4, 0.50, 1700.0)] + [("n0", f, p, 300.0) for f, p in N0_PAIRS[2:]]

SIZES_4300 = [1500, 129, 1, 0, 63, 64, 65, 127, 1300, 1051]
SIZES_33K = [11300, 129, 1, 0, 63, 64, 65, 127, 11000, 10351]


def design(sizes, seed):
    """(chrom_off, start, end) for chromosomes of these sizes"""
    rng = np.random.default_rng(seed)
    chrom_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    E = int(chrom_off[-1])
    start = np.empty(E, dtype=np.int64)
    for c in range(len(sizes)):
        lo, hi = chrom_off[c], chrom_off[c + 1]
        start[lo:hi] = np.cumsum(rng.integers(600, 6000, hi - lo))
    return chrom_off, start.astype(np.int32), (start + rng.integers(50, 400, E)).astype(np.int32)


def background(rng, E, kinds):
    """counts of the sample kinds: totals log-normal around depth / expected, split binomially"""
    S = len(kinds)
    test = np.empty((E, S), dtype=np.int32); ref = np.empty((E, S), dtype=np.int32)
    for s, (_, _, p, depth) in enumerate(kinds):
        tot = rng.poisson(depth / p * np.exp(rng.normal(-0.08, 0.4, E)))
        test[:, s] = rng.binomial(tot, p)
        ref[:, s] = tot - test[:, s]
    return test, ref


def special_exons(geo, free):
    """exons at the places the mode-2 walk can go wrong, by name, among the exons the statistics do not read (`free`: [E] mask)"""
    out = {}
    full = [i for i, (lo, hi, _) in enumerate(geo.blocks) if hi - lo == 64 and free[lo] and free[hi - 1]]
    mid = full[len(full) // 3]
    out["lane0"] = geo.blocks[mid][0]
    out["lane63"] = geo.blocks[full[len(full) // 2]][1] - 1
    last_of = {}
    for i, (lo, hi, c) in enumerate(geo.blocks):
        last_of[c] = i
    partial = [i for i in last_of.values() if 1 < geo.blocks[i][1] - geo.blocks[i][0] < 64 and free[geo.blocks[i][1] - 1]]
    out["partial_last_block"] = geo.blocks[partial[0]][1] - 1
    one = [i for i, (lo, hi, c) in enumerate(geo.blocks) if hi - lo == 1 and last_of[c] == i and (i == 0 or geo.blocks[i - 1][2] != c)]
    out["one_exon_chromosome"] = geo.blocks[one[0]][0]
    if geo.nsplit > 1:
        c0 = [c for c in range(geo.nsplit - 1) if free[geo.blocks[geo.chunk_range(c)[1] - 1][0]] and free[geo.blocks[geo.chunk_range(c)[1]][0]]][0]
        end = geo.chunk_range(c0)[1]
        out["chunk_last_block"] = geo.blocks[end - 1][0]
        out["next_chunk_first_block"] = geo.blocks[end][0]
        out["flush_block"] = [geo.blocks[i][0] for i in range(end - SM_WAVES, end - 1) if free[geo.blocks[i][0]]][-1]
    return out


def make_case(oracle, name, sizes, kinds, seed, caps=DEFAULT_CAPS, tails_modes=(0, 1), negative=True):
    """one case: design, background, the restated dims of both table modes (mode 1 has no tail samples), the plants of both put into exons
    the statistics do not read, the 16-bit variant (plants that fit)"""
    rng = np.random.default_rng(seed)
    chrom_off, start, end = design(sizes, 5)         # (one design per size list: cases of one shape share a plan)
    E, S = int(chrom_off[-1]), len(kinds)
    phi = np.array([k[1] for k in kinds]); p = np.array([k[2] for k in kinds])
    test, ref = background(rng, E, kinds)
    geo = SmGeometry(chrom_off, S)
    free = np.ones(E, dtype=bool)
    pinned = E < 4096                   # the statistics read every exon: only cases whose lengths the caps pin may plant
    if not pinned:
        free[stat_exons(E)] = False
    pre = {t: restate(oracle, test, ref, phi, p, t, caps) for t in tails_modes}
    planted = np.zeros((E, S), dtype=bool)
    spec = special_exons(geo, free) if not pinned else {}
    spec_list = list(spec.values())
    others = np.setdiff1d(np.flatnonzero(free), np.array(spec_list, dtype=np.int64))
    plants = []
    for s in range(S):
        vals, seen = [], set()
        for t in tails_modes:
            for v in plant_values(pre[t][0][s], pre[t][1][s]):
                if v not in seen:
                    seen.add(v); vals.append(v)
        if pinned:
            vals = [(o, r) for o in (63, 64, 65) for r in (63, 64, 65)] + [(0, 0), (0, 63), (64, 0)]
            pos = np.arange(min(E, len(vals)))
            vals = [vals[(int(e) + s * E) % len(vals)] for e in pos]
        else:
            k = s % max(len(vals), 1)
            vals = vals[k:] + vals[:k]                   # another value at each special place from sample to sample
            pos = np.concatenate([np.array(spec_list, dtype=np.int64), rng.permutation(others)])[:len(vals)]
            assert len(pos) == len(vals)
        for e, (o, r) in zip(pos, vals):
            test[e, s], ref[e, s] = o, r
        planted[pos, s] = True
        plants.append(vals)
    neg = None
    if negative and not pinned:
        s_neg = next(s for s in range(S) if kinds[s][0] != "notab")
        e_neg = int(np.flatnonzero(free & ~planted[:, s_neg])[7])
        test[e_neg, s_neg] = -3
        planted[e_neg, s_neg] = True
        neg = (e_neg, s_neg)
    # 16 bits: plants that do not fit go back to a background value (the negative count too); 65 535 itself is planted
    t16, r16 = test.copy(), ref.copy()
    big = (test > 65535) | (ref > 65535) | (test < 0)
    t16[big] = 7; r16[big] = 11
    if not pinned:
        s_top = next(s for s in range(S) if kinds[s][0] != "notab")
        e_top = np.flatnonzero(free & ~planted[:, s_top])[11:13]
        t16[e_top[0], s_top] = 65535; r16[e_top[1], s_top] = 65535
        test[e_top[0], s_top] = 65535; ref[e_top[1], s_top] = 65535
        planted[e_top, s_top] = True
    return dict(name=name, chrom_off=chrom_off, start=start, end=end, E=E, S=S, kinds=kinds, phi=phi, p=p, test=test, ref=ref, test16=t16, ref16=r16,
                geo=geo, free=free, planted=planted, plants=plants, special=spec, pre=pre, caps=caps, negative=neg, pinned=pinned)


def kinds_for(S, first=0):
    """S sample kinds, cycling through KINDS; later cycles move phi a little so that no two samples share their tables"""
    out = []
    for s in range(S):
        kind, phi, p, depth = KINDS[(first + s) % len(KINDS)]
        cyc = (first + s) // len(KINDS)
        if kind in ("table", "tail"):
            phi = phi * (1.0 + 0.11 * cyc)
        out.append((kind, phi, p, depth))
    return out


def case_A(oracle):
    return make_case(oracle, "A", SIZES_4300, kinds_for(130), 11)


def case_A2(oracle):
    """case A's shape with other plants at other places and the sample kinds moved on by three: another sample's tail status"""
    return make_case(oracle, "A2", SIZES_4300, kinds_for(130, first=3), 19)


def case_B(oracle):
    return make_case(oracle, "B", SIZES_4300, kinds_for(257), 12)


def case_C(oracle, variant):
    """S = 3 cannot hold every sample kind at once: two triples, which together hold them all"""
    kinds = [[KINDS[0], KINDS[6], KINDS[7]], [KINDS[2], KINDS[3], KINDS[4]]][variant]
    return make_case(oracle, "C%d" % variant, SIZES_33K, kinds, 13 + variant)


def case_D(oracle):
    return make_case(oracle, "D", SIZES_4300, [KINDS[1]], 15)


SMALL_SHAPES = [(E, S) for E in (1, 63, 64, 65, 130) for S in (1, 9, 17)]
SMALL_CAPS = (64, 64, 8.0)


def case_small(oracle, E, S):
    sizes = [65, 0, 1, 64] if E == 130 else [E]
    kinds = [("table", 0.01 + 0.002 * (s % 5), 0.1 + 0.05 * (s % 7), 100.0) for s in range(S)]
    return make_case(oracle, "small_%d_%d" % (E, S), sizes, kinds, 1000 + 31 * E + S, caps=SMALL_CAPS, tails_modes=(0,), negative=False)


# pinned table lengths for k_tab_build: tails off, counts deep enough that the restated lengths ARE the caps
PINNED_CAPS = [(1024, 4096), (1032, 4104), (4096, 8192)]
PINNED_LENGTHS = sorted({v for cy, cr in PINNED_CAPS for v in (cy, cr, cy + cr)})     # 1024 1032 4096 4104 5120 5136 8192 12288


def case_pinned(oracle, S, caps):
    kinds = [("table", 0.01 + 0.001 * (s % 9), 0.3 + 0.02 * (s % 5), 1100.0) for s in range(S)]
    rng = np.random.default_rng(2000 + S + caps[0])
    chrom_off, start, end = design([150, 50], 77)
    E = 200
    test, ref = background(rng, E, kinds)
    phi = np.array([k[1] for k in kinds]); p = np.array([k[2] for k in kinds])
    c = (caps[0], caps[1], 8.0)
    return dict(name="pinned_%d_%d" % (S, caps[0]), chrom_off=chrom_off, start=start, end=end, E=E, S=S, kinds=kinds, phi=phi, p=p, test=test, ref=ref,
                caps=c, pre={0: restate(oracle, test, ref, phi, p, 0, c)})


# ---------------------------------------------------------------------------------------------------------------------------
# the capacity of one strict list (mode 2, one sample, one launch, per = 64)
# ---------------------------------------------------------------------------------------------------------------------------
def capacity_designs(oracle):
    """One table sample whose background counts are all served; not-served cells (obs = Ly) are put where the restated list assignment
    says: returns the shared design and, per design name, (test, ref, largest list load expected, overflow expected)"""
    kinds = [("table", 0.01, 0.3, 30.0)]
    chrom_off, start, end = design(SIZES_33K, 21)
    E = int(chrom_off[-1])
    rng = np.random.default_rng(21)
    test, ref = background(rng, E, kinds)
    phi = np.array([kinds[0][1]]); p = np.array([kinds[0][2]])
    geo = SmGeometry(chrom_off, 1)
    dims, wins, _ = restate(oracle, test, ref, phi, p, 1)
    Ly, Lr, Tm1, N0 = dims[0]
    assert Ly > 0 and Tm1 == 0 and N0 == NO_N0 and wins[0][3] == 0
    free = np.ones(E, dtype=bool); free[stat_exons(E)] = False
    # every background cell served (the statistics' exons already are, or the design is rejected by the host test)
    test[free[:, None] & (test >= Ly)] = Ly - 1
    ref[free[:, None] & (ref >= Lr)] = Lr - 1
    per = cold_cap_per(E, 1)

    def full_free_block(chunk, wave, skip=0):
        lo, hi = geo.chunk_range(chunk)
        hits = [b for b in range(lo, hi) if geo.wave[b] == wave and geo.blocks[b][1] - geo.blocks[b][0] == 64 and free[geo.blocks[b][0]]
                and b + SM_WAVES < hi and free[geo.blocks[b + SM_WAVES][0]]]
        return hits[skip]

    def with_cold(cells):
        t, r = test.copy(), ref.copy()
        t[cells, 0] = Ly
        return t, r

    out = {}
    b0 = full_free_block(1, 5)
    blk = np.arange(geo.blocks[b0][0], geo.blocks[b0][1])
    nxt = geo.blocks[b0 + SM_WAVES][0] + 9                     # the next block the same wave takes
    out["whole_block"] = with_cold(blk) + (per, False)
    out["whole_block_plus_one"] = with_cold(np.append(blk, nxt)) + (per + 1, True)
    out["one_short"] = with_cold(blk[:per - 1]) + (per - 1, False)
    # two waves of different workgroups on one list: chunks 0 and 8 (workgroups 0 and 64: 64 * 16 = 1024 lists apart), the same wave
    ba, bb = full_free_block(0, 3), full_free_block(8, 3)
    assert geo.list_of(0, ba) == geo.list_of(0, bb) and geo.workgroup(0, 0) != geo.workgroup(0, 8)
    ea = np.arange(geo.blocks[ba][0], geo.blocks[ba][0] + per // 2)
    eb = np.arange(geo.blocks[bb][0] + 64 - (per - per // 2), geo.blocks[bb][0] + 64)
    out["two_workgroups_at_capacity"] = with_cold(np.concatenate([ea, eb])) + (per, False)
    out["two_workgroups_one_over"] = with_cold(np.concatenate([ea, eb, [geo.blocks[bb][0]]])) + (per + 1, True)
    base = dict(chrom_off=chrom_off, start=start, end=end, E=E, S=1, phi=phi, p=p, geo=geo, dims=dims[0], win=wins[0], per=per, free=free)
    return base, out


# ---------------------------------------------------------------------------------------------------------------------------
# the host definition of a served cell (assertion 4) and its bar
# ---------------------------------------------------------------------------------------------------------------------------
def host_definition(oracle, shapes, obs, ref, win):
    """served cells of one sample: (want [n][3], bar [n][3]).  Entries from oracle.dtab inside the tables (a tail sample: inside its
    windows), oracle.dtab_tail beyond a tail sample's windows, oracle.dtab_combine of the three.  bar = spacing(D1) + spacing(D2) +
    spacing(D3) + spacing(want)"""
    a1, a2 = shapes
    obs = np.asarray(obs, dtype=np.int64); ref = np.asarray(ref, dtype=np.int64)
    n1, n2, n3, tail = win
    want = np.empty((obs.size, 3)); bar = np.empty((obs.size, 3))
    if obs.size == 0:
        return want, bar
    for st in range(3):
        parts = []
        for x0, idx, nwin in ((a1[st], obs, n1), (a2[st], ref, n2), (a1[st] + a2[st], obs + ref, n3)):
            if tail:
                inside = idx < nwin
                d = np.empty(idx.size)
                d[inside] = oracle.dtab(x0, nwin)[idx[inside]]
                if (~inside).any():
                    d[~inside] = oracle.dtab_tail(x0, idx[~inside].astype(np.float64))
            else:
                d = oracle.dtab(x0, int(idx.max()) + 1)[idx]
            parts.append(d)
        want[:, st] = oracle.dtab_combine(*parts)
        bar[:, st] = sum(np.spacing(np.abs(d)) for d in parts) + np.spacing(np.abs(want[:, st]))
    return want, bar
