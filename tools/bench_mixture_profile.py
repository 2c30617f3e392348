"""Time of the mixture-profile kernel (csrc/edmix.inc: k_mix_profile) and of a whole fit_prop_tumor, next to what the tree offers
without it for ONE mixture value: a strict run with a per-pair mixture (Batch.set_mixture) and the posterior's backward pass.

The data is bench.py's flagship workload (exomedepth_amd.synth: 200 000 exons, 24 chromosomes, depth 100) read as tumour / normal pairs,
at 1024 pairs and at 64.  Per width:
  profile_ms     one launch at 16 mixtures per pair (events on the stream; the first launch, which uploads the plan's launch rows, is dropped)
  fit            wall seconds of fit_prop_tumor (three rounds: three such launches, their copies to the host and the search in numpy)
  route          the strict run (wall, synchronised) + k_fb_backward (events) for one mixture, timed ONCE, and that sum times 16: what
                 a 16-point profile would cost by the old route -- an extrapolation, not a measurement of sixteen runs
    python tools/bench_mixture_profile.py [--exons 200000] [--samples 1024,64] [--reps 3] [--out profiles/mixture_profile.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_width(args, S, np, torch, ed, synth):
    E, Cn = args.exons, args.chroms
    dev = torch.device("cuda", 0)
    chrom_off, start, end = synth.exon_design(E, Cn, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    plan = ed.Plan(chrom_off, start, end)
    lib = ed._lib.lib()
    stream = torch.cuda.current_stream().cuda_stream
    G = 16
    grid = torch.linspace(0.0, 1.0, G, dtype=torch.float64, device=dev)[:, None].repeat(1, S).contiguous()
    logev = torch.empty((G, Cn, S), dtype=torch.float64, device=dev)
    times = []
    for _ in range(args.reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ed.api.check(lib.ed_plan_mixture_profile(plan.handle, C.c_void_p(test.data_ptr()), C.c_void_p(ref.data_ptr()), 0, S,
                                                 C.c_void_p(phi.data_ptr()), C.c_void_p(p.data_ptr()), C.c_void_p(grid.data_ptr()), G,
                                                 C.c_void_p(logev.data_ptr()), C.c_void_p(stream)))
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times = times[1:]
    l = logev.sum(dim=1).cpu().numpy()
    assert np.all(np.isfinite(l))
    t0 = time.perf_counter()
    fit = ed.fit_prop_tumor(chrom_off, start, end, test, ref, phi=phi.cpu().numpy(), expected=p.cpu().numpy())
    fit_wall = time.perf_counter() - t0
    # the old route, one mixture per pair: strict emissions + Viterbi + call table, then the posterior's passes
    bt = ed.Batch(plan, S)
    bt.enable_timing(True)
    bt.set_mixture(grid[G // 2].contiguous())
    bt.run(test, ref, phi, p, stream=stream)
    bt.n_calls()                      # (allocations and first-use work: dropped)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bt.run(test, ref, phi, p, stream=stream)
    bt.n_calls()
    torch.cuda.synchronize()
    run_ms = 1e3 * (time.perf_counter() - t0)
    ev = bt.log_evidence()
    back_ms = bt.posterior_ms()["backward"]
    same = float(np.max(np.abs(ev.sum(axis=0) - l[G // 2]) / np.abs(l[G // 2])))
    bt.close()
    plan.close()
    med = float(np.median(times))
    return {"pairs": S, "profile_ms": times, "profile_ms_median": med, "lnbeta_pairs_per_second": E * S * (1 + 2 * G) / (med * 1e-3),
            "chain_steps_per_second": E * S * G / (med * 1e-3),
            "fit": {"wall_seconds": fit_wall, "evaluations": int(fit["evaluations"]), "informative_pairs": int(fit["informative"].sum()),
                    "at_bound_pairs": int(fit["at_bound"].sum())},
            "route": {"strict_run_ms": run_ms, "backward_ms": back_ms, "one_mixture_ms": run_ms + back_ms,
                      "sixteen_mixtures_ms_extrapolated": 16 * (run_ms + back_ms),
                      "note": "timed once for one mixture and multiplied by 16", "largest_relative_difference_of_l": same},
            "speedup_over_route_extrapolated": 16 * (run_ms + back_ms) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", default="1024,64")
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mixture_profile.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    out = {"exons": args.exons, "chromosomes": args.chroms, "depth": args.depth, "grid": 16, "geometry": ed.mixture_geometry(),
           "device": torch.cuda.get_device_name(0), "widths": [one_width(args, int(s), np, torch, ed, synth) for s in args.samples.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["widths"]))


if __name__ == "__main__":
    main()
