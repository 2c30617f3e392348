"""Time of the transition-score kernel (csrc/edscore.inc: k_fb_score) on the benchmark's batch, next to the forward-backward kernels of
the same process, and the wall time of one whole fit_transitions on that batch.

The batch is bench.py's flagship workload (exomedepth_amd.synth: 200 000 exons x 1024 samples, 24 chromosomes, depth 100) in the
table-driven sample-major emission mode; the posterior and the score are requested after every run and the kernels are timed by events
on the run's stream (ed_batch_posterior_ms, ed_batch_transition_score_ms).  Bytes are what the score kernel reads and writes once.
fit_transitions then runs on the batch itself (its [E][3][S] matrix stays on the device), from the defaults.
    python tools/bench_transition_score.py [--exons 200000] [--samples 1024] [--reps 3] [--out profiles/transition_score.json]
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transition_score.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    E, S, C = args.exons, args.samples, args.chroms
    dev = torch.device("cuda", 0)
    chrom_off, start, end = synth.exon_design(E, C, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    plan = ed.Plan(chrom_off, start, end)
    b = ed.Batch(plan, S)
    b.enable_timing(True)
    b.set_emit_mode(2)
    stream = torch.cuda.current_stream().cuda_stream
    reps = []
    for _ in range(args.reps + 1):    # the first repetition allocates the buffers and builds the plan's table of derivatives: dropped
        b.run(test, ref, phi, p, stream=stream)
        b.posterior(log=True)
        ev, score = b.transition_score()
        ms = b.posterior_ms()
        ms.pop("call_post", None)
        ms["score"] = b.transition_score_ms()
        reps.append(ms)
        assert b.n_score_passes() == len(reps) and b.n_posterior_passes() == len(reps) and plan.n_score_tables() == 1
    assert np.all(np.isfinite(ev)) and np.all(np.isfinite(score))
    reps = reps[1:]
    cells = E * S
    bytes_ = {"score": cells * (24 + 24) + (C + E) * (64 + 128) + C * S * (8 + 16)}
    med = {k: float(np.median([r[k] for r in reps])) for k in reps[0]}
    out = {"exons": E, "samples": S, "chromosomes": C, "depth": args.depth, "emit_mode": 2, "reps": reps, "median_ms": med,
           "bytes": bytes_, "GBps": {"score": bytes_["score"] / (med["score"] * 1e6)} if med["score"] > 0 else {},
           "score_over_forward": med["score"] / med["forward"] if med["forward"] > 0 else None,
           "device_us_per_chain": {k: 1e3 * med[k] / (C * S) for k in med},
           "score_at_defaults": {"log_evidence": float(ev.sum()), "d_dt": float(score[:, 0, :].sum()), "d_dL": float(score[:, 1, :].sum())},
           "device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    fit = ed.fit_transitions(chrom_off, start, end, b, max_iter=args.max_iter)
    wall = time.perf_counter() - t0
    out["fit"] = {k: v for k, v in fit.items() if k != "trace"}
    out["fit"]["wall_seconds"] = wall
    out["fit"]["seconds_per_evaluation"] = wall / max(fit["evaluations"], 1)
    b.close()
    plan.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median_ms"]), json.dumps(out["fit"]))


if __name__ == "__main__":
    main()
