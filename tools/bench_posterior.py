"""Times of the forward-backward kernels (csrc/edpost.inc) on the benchmark's batch, next to the same run's Viterbi stage.

The batch is bench.py's flagship workload (exomedepth_amd.synth: 200 000 exons x 1024 samples, 24 chromosomes, depth 100) in the
table-driven sample-major emission mode; the posterior is requested after every run and the three kernels are timed by events on the
run's stream (ed_batch_posterior_ms).  Bytes are what the kernels read and write once (the register rings re-read nothing).  The
numpy checker (tests/posterior_checker.py) is timed on one chain of the longest chromosome's length.
    python tools/bench_posterior.py [--exons 200000] [--samples 1024] [--reps 3] [--out profiles/posterior.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth
    import posterior_checker as pc

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
    n_calls = span = 0
    for _ in range(args.reps + 1):    # the first repetition allocates the posterior's buffers and is dropped
        b.run(test, ref, phi, p, stream=stream)
        calls = b.calls()
        cp = b.call_posterior()
        ms = b.posterior_ms()
        ms["viterbi_stage"] = b.stage_ms()["viterbi"]
        reps.append(ms)
        n_calls = int(len(calls))
        span = int(np.sum(calls["end_exon"].astype(np.int64) - calls["start_exon"] + 1))
        assert len(cp) == n_calls and b.n_posterior_passes() == len(reps)
    ev = b.log_evidence()
    assert np.all(np.isfinite(ev))
    reps = reps[1:]
    cells = E * S
    bytes_ = {"backward": cells * (24 + 24) + (C + E) * 64, "forward": cells * (24 + 24 + 16) + (C + E) * 64 + C * S * 8,
              "call_post": n_calls * (24 + 32 + 8 + 8 + 24) + span * (8 + 8 + 8)}
    med = {k: float(np.median([r[k] for r in reps])) for k in reps[0]}
    out = {"exons": E, "samples": S, "chromosomes": C, "depth": args.depth, "emit_mode": 2, "reps": reps, "median_ms": med,
           "bytes": bytes_, "GBps": {k: bytes_[k] / (med[k] * 1e6) for k in bytes_ if med[k] > 0},
           "n_calls": n_calls, "call_exons": span,
           "device": torch.cuda.get_device_name(0)}
    b.close()
    plan.close()
    # the checker, one chain as long as the longest chromosome
    m = int(np.max(np.diff(chrom_off)))
    c = int(np.argmax(np.diff(chrom_off)))
    one = np.array([0, m], np.int32)
    lo = int(chrom_off[c])
    trs = pc.transitions(one, start[lo:lo + m], end[lo:lo + m], plan.transition_probability, plan.expected_CNV_length)
    ll = -np.random.default_rng(1).gamma(2.0, 3.0, (m, 3, 1))
    chk = {}
    for name, dt in (("float64", np.float64), ("longdouble", np.longdouble)):
        t0 = time.perf_counter()
        pc.chain(ll, trs[0], dt)
        chk[name] = time.perf_counter() - t0
    out["checker_seconds_per_chain"] = dict(chk, exons=m)
    out["device_us_per_chain"] = {k: 1e3 * med[k] / (C * S) for k in ("backward", "forward")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out["median_ms"]), json.dumps(out["checker_seconds_per_chain"]))


if __name__ == "__main__":
    main()
