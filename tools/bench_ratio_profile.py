"""Time of the copy-ratio profile (csrc/edratio.inc: k_ratio_profile, k_ratio_sum) on bench.py's flagship workload (exomedepth_amd.synth:
200 000 exons, 24 chromosomes, depth 100, 1 024 samples), next to the route the tree offers without it.

  calls     the call table of a strict run x the 16 ratios of COPY_RATIO_GRID: Batch.call_ratio_profile -- wall milliseconds of the
            request (call table to the host, item list, uploads, kernels, values back) and the kernels alone (Batch.call_ratio_ms)
  regions   20 000 regions of 10 exons x every sample x 16 ratios: Plan.ratio_profile's entry on device-resident counts, in slices of
            samples -- wall seconds, copies of the doses and the values included
  route     what both cost at the parent commit, timed ONCE for one ratio: a strict Batch.run at mixture |dose| with the likelihood matrix
            kept, the matrix copied to the host, and its column summed per row there; times 16 is an extrapolation, not a measurement
    python tools/bench_ratio_profile.py [--exons 200000] [--samples 1024] [--regions 20000] [--reps 3] [--out profiles/ratio_profile.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--regions", type=int, default=20_000)
    ap.add_argument("--region-exons", type=int, default=10)
    ap.add_argument("--slices", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ratio_profile.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    E, S, Cn, G = args.exons, args.samples, args.chroms, 16
    dev = torch.device("cuda", 0)
    chrom_off, start, end = synth.exon_design(E, Cn, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    plan = ed.Plan(chrom_off, start, end)
    ratios = np.array(ed.COPY_RATIO_GRID)

    # ---- the run's own call table
    bt = ed.Batch(plan, S)
    bt.enable_timing(True)
    bt.run(test, ref, phi, p)
    calls = bt.calls()
    wall, kern = [], []
    for _ in range(args.reps + 1):
        t0 = time.perf_counter()
        L, _ = bt.call_ratio_profile(ratios)
        wall.append(1e3 * (time.perf_counter() - t0))
        kern.append(bt.call_ratio_ms())
    wall, kern = wall[1:], kern[1:]
    n_ex = calls["end_exon"].astype(np.int64) - calls["start_exon"] + 1
    cn = ed.copy_number_from_profile(ratios, L)["cn"]
    out_calls = {"calls": int(calls.size), "exons_in_calls": int(n_ex.sum()), "median_exons_per_call": float(np.median(n_ex)) if calls.size else 0.0,
                 "rows_of_up_to_4_exons": int((n_ex <= 4).sum()), "request_wall_ms": wall, "request_wall_ms_median": float(np.median(wall)),
                 "kernel_ms": kern, "kernel_ms_median": float(np.median(kern)), "nan_values": int(np.isnan(L).sum()),
                 "copy_numbers_0_to_4": [int((cn == k).sum()) for k in range(5)]}

    # ---- the old route for one ratio (dose -1: the deletion column at mixture 1): run, matrix to the host, per-row sums there
    t0 = time.perf_counter()
    bt.run(test, ref, phi, p, mixture=1.0)
    bt.n_calls()
    run_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    ll = bt.loglik()
    copy_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    col = np.ascontiguousarray(ll[:, 0, :])
    old = np.array([col[a:b + 1, s].sum() for s, a, b in zip(calls["sample"], calls["start_exon"], calls["end_exon"])])
    sum_calls_ms = 1e3 * (time.perf_counter() - t0)
    k = int(np.flatnonzero(ratios == 0.5)[0])
    same = float(np.nanmax(np.abs(old - L[:, k]) / np.abs(L[:, k]))) if calls.size else 0.0
    # regions: runs of region_exons exons inside one chromosome, spread over the design
    first = []
    per = args.regions // Cn + 1
    for c in range(Cn):
        lo, hi = int(chrom_off[c]), int(chrom_off[c + 1]) - args.region_exons
        if hi > lo:
            first.append(np.linspace(lo, hi, per).astype(np.int64))
    first = np.sort(np.concatenate(first))[:args.regions]
    chrom = (np.searchsorted(chrom_off, first, side="right") - 1).astype(np.int32)
    t0 = time.perf_counter()
    cs = np.concatenate([np.zeros((1, S)), np.cumsum(col, axis=0)])
    old_regions = cs[first + args.region_exons] - cs[first]
    sum_regions_ms = 1e3 * (time.perf_counter() - t0)
    del ll, col, cs
    bt.close()

    # ---- regions x samples, in slices of samples
    R = int(first.size)
    wall_regions, worst = 0.0, 0.0
    for part in np.array_split(np.arange(S), args.slices):
        rows = np.zeros(R * part.size, dtype=ed.CALL_DTYPE)
        rows["sample"] = np.tile(part, R)
        rows["chrom"] = np.repeat(chrom, part.size)
        rows["start_exon"] = np.repeat(first, part.size)
        rows["end_exon"] = rows["start_exon"] + args.region_exons - 1
        doses = np.repeat((2.0 * (ratios - 1.0))[:, None], rows.size, axis=1)
        t0 = time.perf_counter()
        Lr = plan._ratio_doses(rows, test.data_ptr(), ref.data_ptr(), phi.data_ptr(), p.data_ptr(), S, doses)
        wall_regions += time.perf_counter() - t0
        got = Lr[k].reshape(R, part.size)
        worst = max(worst, float(np.nanmax(np.abs(got - old_regions[:, part]) / np.abs(got))))
        del rows, doses, Lr
    plan.close()
    one_calls, one_regions = run_ms + copy_ms + sum_calls_ms, run_ms + copy_ms + sum_regions_ms
    out = {"exons": E, "samples": S, "chromosomes": Cn, "depth": args.depth, "grid": G, "geometry": ed.ratio_geometry(),
           "device": torch.cuda.get_device_name(0), "call_table": out_calls,
           "regions": {"regions": R, "exons_per_region": args.region_exons, "rows": R * S, "values": R * S * G, "slices": args.slices,
                       "wall_seconds": wall_regions, "lnbeta_per_second": R * S * G * args.region_exons / wall_regions},
           "narrow_mapping": {"built": False, "note": "a lane per (exon, column) for rows of up to 4 exons was not built: only the single "
                                                      "mapping was measured, see call_table.kernel_ms and rows_of_up_to_4_exons"},
           "route": {"strict_run_ms": run_ms, "matrix_to_host_ms": copy_ms, "host_sums_calls_ms": sum_calls_ms, "host_sums_regions_ms": sum_regions_ms,
                     "one_ratio_calls_ms": one_calls, "one_ratio_regions_ms": one_regions, "sixteen_ratios_calls_ms_extrapolated": 16 * one_calls,
                     "sixteen_ratios_regions_ms_extrapolated": 16 * one_regions, "note": "timed once for one ratio and multiplied by 16",
                     "largest_relative_difference_calls": same, "largest_relative_difference_regions": worst}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
