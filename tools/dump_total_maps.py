#!/usr/bin/env python3
"""Every output of the maps indexed by a cell's total (csrc/edtotals.inc: the detection-power map, the quantile map, the draws from the
fitted model) for one fixed, small input, into one .npz: for a change that must not move a bit of them.  Run it on a build of the commit
before the change and on a build after it, then compare the two files:

    python tools/dump_total_maps.py before.npz            (ED_LIB_VARIANT=<name> loads exomedepth_amd/libedcore_<name>.so instead)
    python tools/dump_total_maps.py after.npz
    python tools/dump_total_maps.py --compare before.npz after.npz       exit status 1 unless every array is equal byte for byte

The input holds the smallest shapes at which the family's kernels change path: 131 exons (two region tiles of 64 and 3) on two chromosomes,
5 samples (one more than the waves of a region or walk workgroup), one of them with shapes outside the model, in both layouts; totals 0,
1, 255, 256, 257 (the walk tile's edge), occupancy_cap - 1 (the narrow map) and, in a second map, occupancy_cap and max_total (the wide
map); one cell above max_total (skipped); 1, 2 and 16 probabilities; region rows of 1, 64 and 65 exons and one without an exon.
A few seconds on one device.  The times in stats() are left out: they are not results.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (66, 65)                                   # exons of the two chromosomes
PHI = (0.003, 0.05, 0.2, 1.5, 1e-5)                # sample 3: no positive shapes
EXPECTED = (0.05, 0.11, 0.4, 0.1, 0.11)
PROB_LISTS = ((0.5,), (0.025, 0.975),
              (1e-4, 0.001, 0.01, 0.025, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.975, 0.99, 1.0 - 1e-4))
ROWS = ((0, 5, 5), (0, 1, 64), (1, 66, 130), (1, -1, -1))
POINTS = (2.0 ** -53, 0.025, 0.5, 0.975, 1.0 - 2.0 ** -53)
SEED = 20261021


def design():
    chrom_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    start = np.concatenate([np.arange(m, dtype=np.int64) * 1000 + 1 for m in SIZES]).astype(np.int32)
    return chrom_off, start, (start + 120).astype(np.int32)


def edge_totals(geometry, wide):
    cap, top = geometry["occupancy_cap"], geometry["max_total"]
    return [0, 1, 255, 256, 257, cap - 1] + ([cap, top] if wide else [])


def counts(geometry, wide):
    """(test, ref) int32 (E, S): every sample sees every edge total, at another exon each; exon 130 of sample 2 is above max_total"""
    E, S = sum(SIZES), len(PHI)
    rng = np.random.default_rng(131 + int(wide))
    edges = edge_totals(geometry, wide)
    base = np.concatenate([edges, rng.integers(0, 600, E - len(edges))]).astype(np.int64)
    tot = np.stack([np.roll(base, 7 * s) for s in range(S)], axis=1)
    test = np.minimum(tot, (tot * rng.random((E, S)) * 0.3).astype(np.int64))
    ref = tot - test
    test[E - 1, 2], ref[E - 1, 2] = 1, geometry["max_total"]
    return test.astype(np.int32), ref.astype(np.int32)


def dump():
    import exomedepth_amd as ed
    out = {}
    g = ed.power_geometry()
    chrom_off, start, end = design()
    plan = ed.Plan(chrom_off, start, end)
    S = len(PHI)
    for wide in (False, True):
        test, ref = counts(g, wide)
        for layout in (0, 1):
            tag = "%s.l%d" % ("wide" if wide else "narrow", layout)
            t, r = (np.ascontiguousarray(test.T), np.ascontiguousarray(ref.T)) if layout else (test, ref)
            pm = plan.power_map(t, r, PHI, EXPECTED, layout=layout)
            out[tag + ".power.exons"] = pm.exons()
            for s in range(S):
                for k, v in pm.table(s).items():
                    out["%s.power.table%d.%s" % (tag, s, k)] = v
            reg = pm.regions(ROWS)
            for k in reg.dtype.names:
                out["%s.power.regions.%s" % (tag, k)] = np.ascontiguousarray(reg[k])
            out[tag + ".power.counters"] = np.array([v for k, v in pm.stats().items() if not k.endswith("_ms")], dtype=np.int64)
            pm.free()
            for probs in PROB_LISTS:
                q = "%s.quant%d" % (tag, len(probs))
                qm = plan.quantile_map(t, r, PHI, EXPECTED, probs, layout=layout)
                out[q + ".exons"] = qm.exons()
                for s in range(S):
                    for k, v in qm.table(s).items():
                        out["%s.table%d.%s" % (q, s, k)] = v
                for k, v in qm.regions(ROWS).items():
                    out["%s.regions.%s" % (q, k)] = v
                out[q + ".counters"] = np.array([v for k, v in qm.stats().items() if not k.endswith("_ms")], dtype=np.int64)
                qm.free()
            plant = np.zeros(3, dtype=ed.CALL_DTYPE)
            plant["sample"], plant["start_exon"], plant["end_exon"] = (0, 2, 4), (0, 64, 130), (0, 64, 130)
            for rep in (0, 1):
                sim = plan.simulate(t, r, PHI, EXPECTED, SEED, replicate=rep, layout=layout, plant=(plant, (0.5, 1.5, 0.5)))
                out["%s.sim%d.test" % (tag, rep)], out["%s.sim%d.ref" % (tag, rep)] = sim[0].to_host(), sim[1].to_host()
                out["%s.sim%d.counters" % (tag, rep)] = np.array([v for k, v in sim.stats().items() if not k.endswith("_ms")], dtype=np.int64)
                sim.free()
    plan.close()
    # the element-wise entries over the grid of totals (one above max_total: NaN / -1), the samples' shapes and the points
    totals = edge_totals(g, True) + [g["max_total"] + 1]
    phi, e = np.array(PHI), np.array(EXPECTED)
    with np.errstate(all="ignore"):
        a, b = e * (1. - phi) / phi, (1. - e) * (1. - phi) / phi
    n, s, p = [x.ravel() for x in np.meshgrid(np.array(totals, dtype=np.float64), np.arange(S), np.array(POINTS), indexing="ij")]
    s = s.astype(np.int64)
    out["points.qbetabinom_ab"] = ed.qbetabinom_ab(p, n, a[s], b[s])
    out["points.rbetabinom_ab_u"] = ed.rbetabinom_ab_u(p, n, a[s], b[s])
    return out


def as_words(a):
    """floats as their bit patterns, so that NaNs compare"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def compare(path_a, path_b):
    A, B = np.load(path_a), np.load(path_b)
    names = sorted(set(A.files) | set(B.files))
    elements = differing = 0
    for k in names:
        if k not in A.files or k not in B.files or A[k].shape != B[k].shape or A[k].dtype != B[k].dtype:
            print("%s: on one side only, or another shape or type" % k)
            differing += 1
            continue
        d = int(np.count_nonzero(as_words(A[k]) != as_words(B[k])))
        elements += int(A[k].size)
        differing += d
        if d:
            print("%s: %d of %d elements differ" % (k, d, A[k].size))
    print("%d arrays, %d elements, %d differing" % (len(names), elements, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    arrays = dump()
    np.savez(sys.argv[1], **arrays)
    print("%d arrays, %d elements -> %s" % (len(arrays), sum(int(np.size(v)) for v in arrays.values()), sys.argv[1]))
