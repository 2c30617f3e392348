#!/usr/bin/env python
"""Times the annotation join (csrc/edannot.inc, api.Annotation.overlaps) on two synthetic tables drawn with a seed and prints one JSON line:

  exons   --calls calls (runs of 1-12 consecutive exons of a --exons-exon design, as CallCNVs makes them) against the design's own exon track
  self    the self-join of a call table of --calls calls over --samples samples in which --regions regions are each called in --carriers
          samples with jittered ends (group = sample, kind = type): what cohort_call_recurrence runs

Beside each time stands the time of tests/annot_checker.py's sort-and-window host form on the same input, and whether the two results are equal.
The device times are wall times of the whole call -- argument checks, uploads, both passes, the scan, the copy of the hits back -- medians over
--steps calls after --warmup; `create_ms` is the one-off sort and upload of the track.  No torch; builds the library if it is not there.

    python tools/bench_annot.py [--exons 200000] [--calls 100000] [--samples 8192] [--regions 5] [--carriers 3000] [--steps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _exon_case(rng, n_exons, n_calls, seed):
    from exomedepth_amd import synth
    chrom_off, start, end = synth.exon_design(n_exons, 24, seed)
    ecode = np.repeat(np.arange(24), np.diff(chrom_off))
    s = rng.integers(0, n_exons, n_calls)
    e = np.minimum(s + rng.integers(0, 12, n_calls), chrom_off[ecode[s] + 1] - 1)
    subj = {"chrom": ecode, "start": start.astype(np.int64), "end": end.astype(np.int64)}
    qry = {"chrom": ecode[s], "start": start[s].astype(np.int64), "end": end[e].astype(np.int64)}
    return subj, qry


def _self_case(rng, n_calls, n_samples, n_regions, n_carriers):
    n_rec = n_regions * n_carriers
    chrom = rng.integers(0, 24, n_calls)
    start = rng.integers(0, 150_000_000, n_calls)
    length = rng.integers(500, 60_000, n_calls)
    sample = rng.integers(0, n_samples, n_calls)
    kind = rng.integers(1, 3, n_calls)
    for r in range(n_regions):
        sl = slice(r * n_carriers, (r + 1) * n_carriers)
        c, s0, ln = rng.integers(0, 24), rng.integers(0, 150_000_000), rng.integers(20_000, 200_000)
        chrom[sl] = c
        start[sl] = s0 + rng.integers(-2000, 2001, n_carriers)
        length[sl] = ln + rng.integers(-2000, 2001, n_carriers)
        sample[sl] = rng.permutation(n_samples)[:n_carriers] if n_carriers <= n_samples else rng.integers(0, n_samples, n_carriers)
        kind[sl] = 1 + (r & 1)
    p = rng.permutation(n_calls)
    t = {"chrom": chrom[p], "start": np.maximum(start[p], 0), "group": sample[p], "kind": kind[p]}
    t["end"] = t["start"] + length[p]
    return t, n_rec


def _time(f, steps, warmup):
    ts, out = [], None
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out = f()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200000)
    ap.add_argument("--calls", type=int, default=100000)
    ap.add_argument("--samples", type=int, default=8192)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--carriers", type=int, default=3000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from exomedepth_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build()
    import exomedepth_amd as ed
    import annot_checker as ac
    if ed.device_count() <= 0:
        raise SystemExit("bench_annot: no GPU (a measurement path does not fall back)")
    rng = np.random.default_rng(a.seed)
    rec = {"tool": "bench_annot", "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "geometry": ed.annot_geometry(),
           "kernel_sources": _build.csrc_sha16()}
    names = lambda ids: np.char.add("c", np.asarray(ids).astype(str))

    def run(tag, S, Q, filt):
        g = dict(group=S["group"], kind=S["kind"]) if filt else {}
        t0 = time.perf_counter()
        track = ed.Annotation(names(S["chrom"]), S["start"], S["end"], **g)
        create_ms = (time.perf_counter() - t0) * 1e3
        qn = names(Q["chrom"])
        qg = dict(group=Q["group"], kind=Q["kind"]) if filt else {}
        try:
            ms, got = _time(lambda: track.overlaps(qn, Q["start"], Q["end"], min_overlap=0.5, **qg), a.steps, a.warmup)
            ms_count, _ = _time(lambda: track.overlaps(qn, Q["start"], Q["end"], min_overlap=0.5, want_hits=False, **qg), a.steps, a.warmup)
        finally:
            track.close()
        cg = dict(s_group=S["group"], q_group=Q["group"], s_kind=S["kind"], q_kind=Q["kind"]) if filt else {}
        t0 = time.perf_counter()
        want = ac.windowed(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"], 0.5, **cg)
        host_ms = (time.perf_counter() - t0) * 1e3
        widths = ac.window_widths(S["chrom"], S["start"], S["end"], Q["chrom"], Q["start"], Q["end"])
        rec[tag] = {"subjects": int(len(S["start"])), "queries": int(len(Q["start"])), "hits": int(got[1][-1]),
                    "candidates": int(widths.sum()), "widest_window": int(widths.max()),
                    "wide_queries": int(np.sum(widths > rec["geometry"]["wide_threshold"])),
                    "create_ms": create_ms, "join_ms": ms, "count_only_ms": ms_count, "host_windowed_ms": host_ms,
                    "equal_to_host": bool(all(np.array_equal(x, y) for x, y in zip(got, want)))}

    S, Q = _exon_case(rng, a.exons, a.calls, a.seed)
    run("exons", S, Q, False)
    T, n_rec = _self_case(rng, a.calls, a.samples, a.regions, a.carriers)
    run("self", T, T, True)
    rec["self"]["recurrent_calls"] = n_rec
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
