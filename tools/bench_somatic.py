"""Cost of the per-pair tumour fraction: a host-fed cohort of matched tumour / normal pairs (normal depth ~ tumour depth, ~100 reads
per exon) through ed_cohort_run_host_mix (one mixture per pair) and through ed_cohort_run_host (one scalar), alternated in one process.
Also records the table mode's eligibility (table_stats, cold cells) of that somatic cohort next to a germline-like cohort whose
references are 8x aggregates.  Prints one JSON line.
    python tools/bench_somatic.py [--exons 200000] [--pairs 1024] [--reps 3] [--slab 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200000)
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slab", type=int, default=256)
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    import exomedepth_amd as ed
    from exomedepth_amd import synth
    E, S = a.exons, a.pairs
    chrom_off, start, end = synth.exon_design(E, 24, seed=3)
    rng = np.random.default_rng(17)

    def cohort(K):
        """beta-binomial counts with planted CNVs (synth.counts_numpy, ~100 test reads per exon), laid out sample-major (layout 1: R's
        column-major exons x pairs); K = reference depth / test depth.  256 distinct pairs (the generator takes ~10 s per 128 at 200 000
        exons), repeated to the cohort's width"""
        n = min(S, 256)
        test, ref = np.empty((n, E), np.int32), np.empty((n, E), np.int32)
        for s0 in range(0, n, 128):
            k = min(128, n - s0)
            t_, r_, _, _, _ = synth.counts_numpy(chrom_off, k, seed=1000 + s0, K=K, n_segments=20, mean_depth=100.0)
            test[s0:s0 + k], ref[s0:s0 + k] = t_.T, r_.T
        reps = (S + n - 1) // n
        return np.ascontiguousarray(np.tile(test, (reps, 1))[:S]), np.ascontiguousarray(np.tile(ref, (reps, 1))[:S])
    tumor, normal = cohort(1.0)                                                   # normal depth ~ tumour depth, ~100 reads per exon
    mix = rng.choice([1.0, 0.8, 0.5, 0.3, 0.1, 0.05], S)
    plan = ed.Plan(chrom_off, start, end)
    co = ed.Cohort(plan, a.slab, 2, emit_mode=2, counts_layout=1)
    co.run_host(tumor, normal, 1, mixture=mix)                                    # warm-up: buffers, tables, code objects
    co.run_host(tumor, normal, 1, mixture=0.5)
    t = {"mix": [], "scalar": []}
    for _ in range(a.reps):
        for kind in ("mix", "scalar"):
            t0 = time.perf_counter()
            out = co.run_host(tumor, normal, 1, mixture=mix if kind == "mix" else 0.5)
            t[kind].append(time.perf_counter() - t0)
    somatic_stats = out["table_stats"]
    del tumor, normal
    test8, ref8 = cohort(8.0)                                                     # germline-like: 8x aggregate references
    germ = co.run_host(test8, ref8, 1, mixture=1.0)
    co.close(); plan.close()
    res = {"exons": E, "pairs": S, "slab": a.slab, "emit_mode": 2, "reps": a.reps,
           "mix_s": t["mix"], "scalar_s": t["scalar"],
           "mix_min_s": min(t["mix"]), "scalar_min_s": min(t["scalar"]),
           "mix_over_scalar": min(t["mix"]) / min(t["scalar"]),
           "table_stats_somatic_1x": somatic_stats, "table_stats_germline_8x": germ["table_stats"]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
