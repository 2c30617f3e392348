"""Measure the draws from the fitted model (csrc/edsim.inc) on one device and write profiles/null_draw.json.

    python tools/bench_simulate.py [--out profiles/null_draw.json] [--bench-ab this.jsonl parent.jsonl]

At 200 000 exons x 1 024 samples, depth 100 (bench.py's synthetic cohort and its fitted phi / expected), medians of three after a dropped
first run:
  one replicate's draw (Plan.simulate): wall time and the library's split into occupancy, grouping and walk; tiles walked as a share of one
  full walk per 64 cells; cells per job;
  the same cells drawn by synth.counts_torch's gamma / binomial lines in the same process -- ANOTHER distribution of bits: float32 shapes,
  torch's generators, not reproducible across versions; a time to stand beside, not a rival implementation of the same function;
  the element-wise entry (rbetabinom_ab_u, host arrays in and out) on 10^6 of the cells, scaled to all of them: an EXTRAPOLATION;
  the fit + run step the draw feeds (Batch.fit + Batch.run).
Then, on a cohort of 20 000 exons x 64 samples without a CNV in it, deletions (ratio 0.5) and duplications (ratio 1.5) of 1, 3 and 10 exons
planted at eight places in every sample: the share of (replicate, sample, place) in which the unchanged pipeline calls a CNV of that type
over the planted exons, beside detection_power's normal approximation `power` for the same rows.
--bench-ab: two files of bench.py default lines (this tree's and the parent commit's, alternated on one machine) are folded into the result:
this tree's median must lie inside the parent's own spread widened by that spread once more.  No pass mark on anything else."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med3(fn, sync):
    """median of three after a dropped first: (median seconds, the three, whatever the last call returned)"""
    ts, last = [], None
    for k in range(4):
        sync()
        t0 = time.perf_counter()
        last = fn(k)
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts[1:])), [float(t) for t in ts[1:]], last


def big(args, ed, synth, torch):
    dev = torch.device("cuda", 0)
    sync = torch.cuda.synchronize
    E, S, C = args.exons, args.samples, 24
    chrom_off, start, end = synth.exon_design(E, C, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    plan = ed.Plan(chrom_off, start, end)
    batch = ed.Batch(plan, S)
    ph, pe = torch.empty(S, dtype=torch.float64, device=dev), torch.empty(S, dtype=torch.float64, device=dev)

    def step(_):
        batch.fit(test, ref, ph, pe)
        batch.run(test, ref, ph, pe)
        return batch.n_calls()

    t_step, steps, n_calls = med3(step, sync)
    phi_h, exp_h = ph.cpu().numpy(), pe.cpu().numpy()
    out = {"exons": E, "samples": S, "depth": args.depth, "cells": E * S,
           "fit_plus_run": {"ms": t_step * 1e3, "each_ms": [t * 1e3 for t in steps], "n_calls": int(n_calls)}}

    def draw(k):
        sim = plan.simulate(test, ref, phi_h, exp_h, seed=2024, replicate=k)
        st = sim.stats()
        sim.free()
        return st

    t_draw, draws, st = med3(draw, sync)
    stats = []
    for k in range(3):
        stats.append(draw(10 + k))
    out["draw"] = {"ms": t_draw * 1e3, "each_ms": [t * 1e3 for t in draws],
                   "occupancy_ms": float(np.median([s["occupancy_ms"] for s in stats])), "grouping_ms": float(np.median([s["grouping_ms"] for s in stats])),
                   "walk_ms": float(np.median([s["walk_ms"] for s in stats])), "n_jobs": st["n_jobs"], "cells_drawn": st["cells_drawn"],
                   "cells_skipped": st["cells_skipped"], "cells_per_job": st["cells_drawn"] / max(st["n_jobs"], 1),
                   "tiles_walked": st["tiles_walked"], "tiles_full": st["tiles_full"], "tiles_share": st["tiles_walked"] / max(st["tiles_full"], 1),
                   "note": "ms = wall time of Plan.simulate (allocation of the two outputs, the copy of the inputs into them and the tally included); "
                           "the three parts are the library's own, host-timed between waits"}
    out["draw"]["ratio_to_fit_plus_run"] = out["draw"]["ms"] / out["fit_plus_run"]["ms"]

    # synth.counts_torch's gamma / binomial lines on the same cells (float32 shapes, torch's generators: another distribution of bits)
    pt, pht = torch.tensor(exp_h, device=dev), torch.tensor(phi_h, device=dev)
    theta = (1 - pht) / pht
    a32, b32 = (pt * theta).float()[None, :], ((1 - pt) * theta).float()[None, :]
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sink = torch.empty((args.chunk, S), dtype=torch.int32, device=dev)

    def torch_draw(_):
        for lo in range(0, E, args.chunk):
            hi = min(lo + args.chunk, E)
            tot = (test[lo:hi] + ref[lo:hi]).double()
            ga = torch._standard_gamma(a32.expand(hi - lo, S).contiguous())
            gb = torch._standard_gamma(b32.expand(hi - lo, S).contiguous())
            lamb = (ga / (ga + gb)).double().clamp_(0.0, 1.0)
            sink[:hi - lo] = torch.binomial(tot, lamb, generator=g).to(torch.int32)
        return None

    t_torch, each, _ = med3(torch_draw, sync)
    out["torch_gamma_binomial"] = {"ms": t_torch * 1e3, "each_ms": [t * 1e3 for t in each],
                                   "note": "synth.counts_torch's lines: float32 gamma shapes, torch's generators; a different distribution of bits, "
                                           "not reproducible across torch versions and not tied to qbetabinom"}

    # the element-wise entry on 10^6 cells, scaled
    rng = np.random.default_rng(3)
    n_el = min(10 ** 6, E * S)
    ei, si = rng.integers(0, E, n_el), rng.integers(0, S, n_el)
    tot_h = (test + ref)[torch.as_tensor(ei, device=dev), torch.as_tensor(si, device=dev)].cpu().numpy().astype(np.float64)
    a_h, b_h = (exp_h * (1. - phi_h) / phi_h)[si], ((1. - exp_h) * (1. - phi_h) / phi_h)[si]
    u_h = ed.runif53(2024, ei, si, 0)
    t_el, each, x = med3(lambda _: ed.rbetabinom_ab_u(u_h, tot_h, a_h, b_h), sync)
    out["element_wise"] = {"cells": n_el, "ms": t_el * 1e3, "each_ms": [t * 1e3 for t in each], "scaled_to_all_cells_ms": t_el * 1e3 * (E * S / n_el),
                           "note": "EXTRAPOLATION: 10^6 cells through rbetabinom_ab_u (host arrays in and out, one wavefront and one walk per cell), "
                                   "multiplied by cells / 10^6"}
    batch.close(); plan.close()
    return out


def planted(args, ed, synth):
    E, S, C = 20000, 64, 24
    chrom_off, start, end = synth.exon_design(E, C, seed=7)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, 7, n_segments=0, mean_depth=args.depth)
    plan = ed.Plan(chrom_off, start, end)
    batch = ed.Batch(plan, S)
    dp, de = ed.DeviceArray(np.zeros(S)), ed.DeviceArray(np.zeros(S))
    batch.fit(test, ref, dp, de)
    phi_h, exp_h = dp.to_host(np.float64, (S,)), de.to_host(np.float64, (S,))
    batch.close(); plan.close()
    sizes = np.diff(chrom_off)
    table = []
    for kind, ratio, typ in (("deletion", 0.5, 1), ("duplication", 1.5, 2)):
        for L in (1, 3, 10):
            rows = []
            for c in range(8):
                first = int(chrom_off[c]) + int(sizes[c]) // 2
                rows.append((c, first, first + L - 1))
            rows = np.array(rows)
            t0 = time.perf_counter()
            out = ed.null_call_table(chrom_off, start, end, test, ref, phi_h, exp_h, args.replicates, seed=31 + L, plant=(rows, ratio))
            wall = time.perf_counter() - t0
            calls = out["calls"]
            hit = 0
            for c, first, last in rows:
                m = calls[(calls["type"] == typ) & (calls["start_exon"] <= last) & (calls["end_exon"] >= first)]
                hit += len(set(zip(m["replicate"].tolist(), m["sample"].tolist())))
            pw = ed.detection_power(chrom_off, start, end, test, ref, phi_h, exp_h, rows)
            power = pw["power_del" if typ == 1 else "power_dup"]
            table.append({"type": kind, "ratio": ratio, "n_exons": L, "places": len(rows), "samples": S, "replicates": args.replicates,
                          "called_share": hit / float(len(rows) * S * args.replicates), "detection_power_mean": float(np.mean(power)),
                          "detection_power_min": float(np.min(power)), "detection_power_max": float(np.max(power)),
                          "other_calls_per_sample": float((len(calls) - hit) / float(S * args.replicates)), "wall_s": wall})
    return {"exons": E, "samples": S, "depth": args.depth, "rows": table,
            "note": "called_share: of (replicate, sample, place), those with a call of the planted type over the planted exons, each replicate refitted "
                    "as a real run would be; detection_power_*: power_del / power_dup of the same rows over the samples (normal approximation)"}


def bench_ab(this_path, parent_path):
    def values(path):
        return [json.loads(l)["ms_per_step"] for l in open(path) if l.startswith("{")]
    mine, parent = values(this_path), values(parent_path)
    spread = max(parent) - min(parent)
    lo, hi = min(parent) - spread, max(parent) + spread
    med = float(np.median(mine))
    return {"this_tree_ms_per_step": mine, "parent_ms_per_step": parent, "this_tree_median": med, "parent_median": float(np.median(parent)),
            "parent_spread": spread, "allowed": [lo, hi], "inside": bool(lo <= med <= hi),
            "note": "bench.py's default line, the two trees alternated on one machine, three runs each"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "null_draw.json"))
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--replicates", type=int, default=10)
    ap.add_argument("--bench-ab", nargs=2, default=None)
    args = ap.parse_args()
    import torch                      # first: the library then binds to the same HIP runtime (as bench.py does)
    torch.cuda.init()
    import exomedepth_amd as ed
    from exomedepth_amd import _build, synth
    res = {"tool": "tools/bench_simulate.py", "csrc_sha16": _build.csrc_sha16(), "device": torch.cuda.get_device_name(0),
           "method": "medians of three after a dropped first run, wall time between device synchronisations"}
    res["cohort"] = big(args, ed, synth, torch)
    res["planted"] = planted(args, ed, synth)
    if args.bench_ab:
        res["bench_ab"] = bench_ab(*args.bench_ab)
    text = json.dumps(res, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
