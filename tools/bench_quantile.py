"""Time of the quantile map (csrc/edquant.inc) on bench.py's flagship workload (exomedepth_amd.synth: 200 000 exons, 24 chromosomes, depth
100, 1 024 samples) with 20 000 regions of 10 exons, at the plot's two probabilities and at a list of 16, next to a plain scipy form of
one sample's table.

  map            ed_plan_quantile_map on device-resident counts: wall seconds of the call (it returns complete), and the library's own split
                 into occupancy (the power map's five passes, the two read-backs between them and k_bq_obs) and walk (k_bq_walk), host-timed
                 between waits; the first call, which pays first-use work, is dropped
  tiles          256-value tiles the walks took, against what walks to the end of every total would take: the early exit
  regions        ed_quant_regions to host arrays: wall seconds of the call (the copies of R S (K + 1) records to pageable memory included) and
                 the kernel alone (k_bq_regions)
  exons          ed_quant_copy_exons: wall seconds (2 K S E doubles to pageable memory) and k_bq_exons alone; at the two probabilities only --
                 at 16 the host array is 52 GB
  scipy          one sample's table by betaln / gammaln in binary64 on this machine's CPU, one total after the other (qbetabinom.ab line by
                 line), and that time times the number of samples: an extrapolation, not a measurement of 1 024 samples
    python tools/bench_quantile.py [--exons 200000] [--samples 1024] [--regions 20000] [--reps 3] [--out profiles/quantile_map.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIST16 = (1e-4, 0.001, 0.01, 0.025, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.975, 0.99, 1.0 - 1e-4)


def scipy_table(np, totals, a, b, probs):
    from scipy.special import betaln, gammaln
    out = np.zeros((len(probs), totals.size))
    for i, n in enumerate(totals):
        n = float(n)
        x = np.arange(n + 1.0)
        pm = np.exp(gammaln(n + 1.0) - gammaln(x + 1.0) - gammaln(n - x + 1.0) + betaln(a + x, b + n - x) - betaln(a, b))
        cs = np.cumsum(pm)
        for k, p in enumerate(probs):
            above = int(np.argmax(cs > p))
            out[k, i] = above + (p - cs[above - 1]) / pm[above] if above > 0 else p / pm[0]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quantile_map.json"))
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
    rng = np.random.default_rng(5)
    rows = np.zeros(args.regions, dtype=ed.api.CALL_DTYPE)
    sizes = np.diff(chrom_off)
    c = rng.choice(Cn, args.regions, p=sizes / sizes.sum())
    first = chrom_off[c] + (rng.random(args.regions) * np.maximum(sizes[c] - args.region_exons, 1)).astype(np.int64)
    rows["chrom"], rows["start_exon"], rows["end_exon"] = c, first, np.minimum(first + args.region_exons - 1, chrom_off[c + 1] - 1)
    R = rows.size
    lib = ed._lib.lib()
    med = lambda v: float(np.median(v))
    out = {"exons": E, "samples": S, "chromosomes": Cn, "depth": args.depth, "geometry": ed.quantile_geometry(), "device": torch.cuda.get_device_name(0),
           "requests": {}}
    for name, probs in (("band", (0.025, 0.975)), ("list16", LIST16)):
        K = len(probs)
        walls, stats = [], []
        qm = None
        for _ in range(args.reps + 1):
            if qm is not None:
                qm.free()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qm = plan.quantile_map(test, ref, phi_h, p_h, probs)
            walls.append(time.perf_counter() - t0)
            stats.append(qm.stats())
        walls, stats = walls[1:], stats[1:]
        st = stats[-1]
        obs, exp, empty = np.zeros((R, S, K + 1), dtype=np.int32), np.zeros((R, S, K + 1)), np.zeros((R, S), dtype=np.int32)
        reg_wall, reg_kernel = [], []
        for _ in range(args.reps + 1):
            t0 = time.perf_counter()
            ed.api.check(lib.ed_quant_regions(qm.handle, rows.ctypes.data, R, obs.ctypes.data, exp.ctypes.data, empty.ctypes.data, None))
            reg_wall.append(time.perf_counter() - t0)
            reg_kernel.append(qm.stats()["regions_ms"])
        reg_wall, reg_kernel = reg_wall[1:], reg_kernel[1:]
        assert np.all(np.isfinite(exp)) and np.all(obs.sum(axis=2) + empty == (rows["end_exon"] - rows["start_exon"] + 1)[:, None])
        rec = {"probs": list(probs),
               "map": {"wall_seconds": walls, "wall_seconds_median": med(walls), "occupancy_ms": [s["occupancy_ms"] for s in stats],
                       "occupancy_ms_median": med([s["occupancy_ms"] for s in stats]), "walk_ms": [s["walk_ms"] for s in stats],
                       "walk_ms_median": med([s["walk_ms"] for s in stats])},
               "tiles": {"walked": st["tiles_walked"], "full_walk": st["tiles_full"], "share": st["tiles_walked"] / max(st["tiles_full"], 1)},
               "jobs": {"n_jobs": st["n_jobs"], "per_sample": st["n_jobs"] / S, "most_of_one_sample": st["max_jobs"], "largest_total": st["largest_total"],
                        "n_skipped": st["n_skipped"], "n_bad_samples": st["n_bad_samples"]},
               "regions": {"rows": R, "exons_per_row": args.region_exons, "wall_seconds": reg_wall, "wall_seconds_median": med(reg_wall),
                           "kernel_ms": reg_kernel, "kernel_ms_median": med(reg_kernel), "bytes_to_host": int(obs.nbytes + exp.nbytes + empty.nbytes)}}
        del obs, exp, empty
        if name == "band":
            ex = np.zeros((2, K, S, E))
            ex_wall, ex_kernel = [], []
            for _ in range(2):
                t0 = time.perf_counter()
                ed.api.check(lib.ed_quant_copy_exons(qm.handle, ex.ctypes.data, None))
                ex_wall.append(time.perf_counter() - t0)
                ex_kernel.append(qm.stats()["exons_ms"])
            rec["exons"] = {"wall_seconds": ex_wall[1:], "kernel_ms": ex_kernel[1:], "bytes_to_host": int(ex.nbytes),
                            "share_outside_band": float(np.mean((test[:, 0].cpu().numpy() < np.ceil(ex[0, 0, 0]) - 1) |
                                                                (test[:, 0].cpu().numpy() >= np.ceil(ex[0, 1, 0]) - 1)))}
            del ex
            # one sample's table by scipy
            tab = qm.table(0)
            a, b = p_h[0] * (1 - phi_h[0]) / phi_h[0], (1 - p_h[0]) * (1 - phi_h[0]) / phi_h[0]
            t0 = time.perf_counter()
            want = scipy_table(np, tab["totals"], a, b, probs)
            scipy_s = time.perf_counter() - t0
            out["scipy"] = {"one_sample_seconds": scipy_s, "totals_of_that_sample": int(tab["totals"].size), "all_samples_seconds_extrapolated": scipy_s * S,
                            "note": "one sample timed once and multiplied by the number of samples",
                            "largest_difference_of_q": float(np.max(np.abs(tab["q"] - want)))}
        else:
            rec["exons"] = "not measured: the host array of 2 x 16 x samples x exons doubles is 52 GB"
        rec["whole_request_seconds_median"] = med(walls) + med(reg_wall)
        out["requests"][name] = rec
        print("%s: map %.3f s (walk %.1f ms), regions %.3f s" % (name, med(walls), rec["map"]["walk_ms_median"], med(reg_wall)), file=sys.stderr, flush=True)
        qm.free()
    plan.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"requests": out["requests"], "scipy": out["scipy"]}))


if __name__ == "__main__":
    main()
