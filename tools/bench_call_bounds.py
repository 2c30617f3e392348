"""Times of k_call_bounds (csrc/edbounds.inc) next to k_call_post and the two forward-backward passes of the same run.

Two tables on the posterior bench's batch (exomedepth_amd.synth: 200 000 exons x 1024 samples, 24 chromosomes, depth 100, table-driven
sample-major emission mode):
  cohort     the run's own call table (about 1.5 x 10^4 short rows)
  long_rows  the same counts with the longest chromosome of EVERY sample far outside the normal state (500 reads at every exon, the
             test count at the expectation of a ratio of 8: every exon favours a CNV state -- whichever has the heavier tail under the
             sample's parameters -- by more than the two log(t / 2) it costs to stay in it across two long gaps), so that the call table
             also holds one row per sample that spans the whole chain (19 352 exons at the default design): what a thread per row pays a
             dependent round trip per exon for, and a wave per row a tile of 64 exons per step
Each repetition runs the batch, requests the posterior, the per-call summary and the bounds, and reads the events on the run's stream
(ed_batch_posterior_ms, ed_batch_call_bounds_ms).  The first repetition of a table allocates and is dropped.
    python tools/bench_call_bounds.py [--exons 200000] [--samples 1024] [--reps 7] [--out profiles/call_bounds.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--level", type=float, default=0.95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "call_bounds.json"))
    args = ap.parse_args()
    import numpy as np
    import torch                      # first: libedcore binds to the HIP runtime torch brought up
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    E, S, C = args.exons, args.samples, args.chroms
    dev = torch.device("cuda", 0)
    chrom_off, start, end = synth.exon_design(E, C, seed=20250620)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    c_long = int(np.argmax(np.diff(chrom_off)))
    lo, hi = int(chrom_off[c_long]), int(chrom_off[c_long + 1])
    # the long-row table: on the longest chromosome every exon is deep and every sample's test count the expectation of a ratio of 8
    pp = 8.0 * p / (8.0 * p + 1.0 - p)
    tot = torch.full((hi - lo, S), 500.0, device=dev, dtype=torch.float64)
    test_l, ref_l = test.clone(), ref.clone()
    test_l[lo:hi] = torch.round(tot * pp[None, :]).to(torch.int32)
    ref_l[lo:hi] = (tot.to(torch.int32) - test_l[lo:hi])
    plan = ed.Plan(chrom_off, start, end)
    b = ed.Batch(plan, S)
    b.enable_timing(True)
    b.set_emit_mode(2)
    stream = torch.cuda.current_stream().cuda_stream
    out = {"exons": E, "samples": S, "chromosomes": C, "depth": args.depth, "emit_mode": 2, "level": args.level,
           "longest_chain": hi - lo, "device": torch.cuda.get_device_name(0), "tables": {}}
    for name, (t_, r_) in (("cohort", (test, ref)), ("long_rows", (test_l, ref_l))):
        reps = []
        for _ in range(args.reps + 1):
            b.run(t_, r_, phi, p, stream=stream)
            calls = b.calls()
            cp = b.call_posterior()
            cb = b.call_bounds(args.level)
            ms = b.posterior_ms()
            ms["call_bounds"] = b.call_bounds_ms()
            reps.append(ms)
            assert len(cp) == len(cb) == len(calls)
        reps = reps[1:]
        span = calls["end_exon"].astype(np.int64) - calls["start_exon"] + 1
        whole = int(np.sum((calls["chrom"] == c_long) & (calls["start_exon"] == lo) & (calls["end_exon"] == hi - 1)))
        walked = (cb["end_hi"].astype(np.int64) - cb["start_lo"] + 1) + span            # exons a row's walks and its anchor pass touch, at least
        stat = {k: {"median": float(np.median([r[k] for r in reps])), "min": float(min(r[k] for r in reps)), "max": float(max(r[k] for r in reps))}
                for k in reps[0]}
        out["tables"][name] = {"reps": reps, "ms": stat, "n_calls": int(len(calls)), "call_exons": int(span.sum()), "longest_row": int(span.max()),
                               "rows_spanning_the_longest_chain": whole, "rows_flagged": int(np.sum(cb["flags"] != 0)), "exons_walked_at_least": int(walked.sum()),
                               "call_post_over_call_bounds": stat["call_post"]["median"] / stat["call_bounds"]["median"]}
        print(name, json.dumps({k: v["median"] for k, v in stat.items()}), "rows", len(calls), "whole-chain rows", whole)
    b.close()
    plan.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    assert out["tables"]["long_rows"]["rows_spanning_the_longest_chain"] == S, "the long-row table does not hold one whole-chain row per sample"


if __name__ == "__main__":
    main()
