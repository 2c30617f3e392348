"""Time of the detection-power map (csrc/edpower.inc) on bench.py's flagship workload (exomedepth_amd.synth: 200 000 exons, 24 chromosomes,
depth 100, 1 024 samples) with 20 000 regions of 10 exons, next to a plain numpy / scipy form of the same table.

  map            ed_plan_power_map on device-resident counts: wall seconds of the call (it returns complete), and the library's own split into
                 occupancy (k_pw_scan, k_pw_mark, k_pw_rank, k_pw_jobs, k_pw_slots and the two read-backs between them) and walk (k_pw_walk),
                 host-timed between waits; the first call, which pays first-use work, is dropped
  regions        ed_power_regions to host arrays: wall seconds of the call (the copies of 4 R S doubles to pageable memory included) and the
                 kernels alone (k_pw_regions + k_pw_price)
  jobs           occupied totals per sample -- one walk each -- and cells per job: what walking per total instead of per cell saves
  scipy          one sample's table by betaln / gammaln in binary64 on this machine's CPU, one total after the other, and that time times the
                 number of samples: an extrapolation, not a measurement of 1 024 samples
    python tools/bench_power_map.py [--exons 200000] [--samples 1024] [--regions 20000] [--reps 3] [--out profiles/power_map.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def scipy_table(np, totals, a1, a2):
    from scipy.special import betaln, gammaln
    out = np.zeros((4, totals.size))
    for i, n in enumerate(totals):
        n = float(n)
        x = np.arange(n + 1.0)
        e = [betaln(a1[j] + x, a2[j] + n - x) - betaln(a1[j], a2[j]) for j in range(3)]
        lch = gammaln(n + 1.0) - gammaln(x + 1.0) - gammaln(n - x + 1.0)
        for k, T in ((0, 0), (2, 2)):
            P = np.exp(lch + e[T])
            D = math.log10(math.e) * (e[T] - e[1])
            m = np.sum(P * D)
            out[k, i], out[k + 1, i] = m, np.sum(P * (D - m) ** 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--regions", type=int, default=20_000)
    ap.add_argument("--region-exons", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_map.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    E, S, Cn = args.exons, args.samples, args.chroms
    dev = torch.device("cuda", 0)
    chrom_off, start, end = synth.exon_design(E, Cn, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    phi_h, p_h = phi.cpu().numpy(), p.cpu().numpy()
    plan = ed.Plan(chrom_off, start, end)
    walls, stats = [], []
    pm = None
    for _ in range(args.reps + 1):
        if pm is not None:
            pm.free()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pm = plan.power_map(test, ref, phi_h, p_h)
        walls.append(time.perf_counter() - t0)
        stats.append(pm.stats())
    walls, stats = walls[1:], stats[1:]
    st = stats[-1]
    # regions of region_exons exons, spread over the chromosomes
    rng = np.random.default_rng(5)
    rows = np.zeros(args.regions, dtype=ed.api.CALL_DTYPE)
    sizes = np.diff(chrom_off)
    c = rng.choice(Cn, args.regions, p=sizes / sizes.sum())
    first = chrom_off[c] + (rng.random(args.regions) * np.maximum(sizes[c] - args.region_exons, 1)).astype(np.int64)
    rows["chrom"], rows["start_exon"], rows["end_exon"] = c, first, np.minimum(first + args.region_exons - 1, chrom_off[c + 1] - 1)
    R = rows.size
    sums, empty = np.zeros((4, R, S)), np.zeros((R, S), dtype=np.int32)
    price, nex = np.zeros(R), np.zeros(R, dtype=np.int32)
    lib = ed._lib.lib()
    reg_wall, reg_kernel = [], []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        ed.api.check(lib.ed_power_regions(pm.handle, rows.ctypes.data, R, sums.ctypes.data, empty.ctypes.data, price.ctypes.data, nex.ctypes.data, None))
        reg_wall.append(time.perf_counter() - t0)
        reg_kernel.append(pm.stats()["regions_ms"])
    reg_wall, reg_kernel = reg_wall[1:], reg_kernel[1:]
    assert np.all(np.isfinite(sums)) and np.all(nex >= 1)
    # one sample's table by scipy
    tab = pm.table(0)
    sd = math.sqrt(phi_h[0] * p_h[0] * (1 - p_h[0]))
    a1, a2 = [], []
    for odds in (0.5, 1.0, 1.5):
        ep = p_h[0] * odds / (p_h[0] * odds + 1 - p_h[0]) if odds != 1.0 else p_h[0]
        a1.append(ep * ep * (1 - ep) / (sd * sd) - ep)
        a2.append((1 - ep) / ep * a1[-1])
    t0 = time.perf_counter()
    want = scipy_table(np, tab["totals"], a1, a2)
    scipy_s = time.perf_counter() - t0
    got = np.stack([tab[k] for k in ("mean_del", "var_del", "mean_dup", "var_dup")])
    rel = float(np.max(np.abs(got - want)[:, tab["totals"] > 0] / np.abs(want)[:, tab["totals"] > 0]))
    pm.free()
    plan.close()
    med = lambda v: float(np.median(v))
    out = {"exons": E, "samples": S, "chromosomes": Cn, "depth": args.depth, "geometry": ed.power_geometry(), "device": torch.cuda.get_device_name(0),
           "map": {"wall_seconds": walls, "wall_seconds_median": med(walls), "occupancy_ms": [s["occupancy_ms"] for s in stats],
                   "occupancy_ms_median": med([s["occupancy_ms"] for s in stats]), "walk_ms": [s["walk_ms"] for s in stats],
                   "walk_ms_median": med([s["walk_ms"] for s in stats])},
           "jobs": {"n_jobs": st["n_jobs"], "per_sample": st["n_jobs"] / S, "most_of_one_sample": st["max_jobs"], "cells_per_job": E * S / max(st["n_jobs"], 1),
                    "largest_total": st["largest_total"], "n_skipped": st["n_skipped"], "n_bad_samples": st["n_bad_samples"]},
           "regions": {"rows": R, "exons_per_row": args.region_exons, "wall_seconds": reg_wall, "wall_seconds_median": med(reg_wall),
                       "kernels_ms": reg_kernel, "kernels_ms_median": med(reg_kernel), "bytes_to_host": int(sums.nbytes + empty.nbytes)},
           "whole_call_seconds_median": med(walls) + med(reg_wall),
           "scipy": {"one_sample_seconds": scipy_s, "totals_of_that_sample": int(tab["totals"].size), "all_samples_seconds_extrapolated": scipy_s * S,
                     "note": "one sample timed once and multiplied by the number of samples", "largest_relative_difference": rel}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("map", "jobs", "regions", "whole_call_seconds_median", "scipy")}))


if __name__ == "__main__":
    main()
