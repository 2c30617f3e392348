#!/usr/bin/env python
"""Times the GC column (csrc/edgc.inc, api.gc_content, fasta.FastaIndex) on one synthetic sequence and writes one JSON record.

The file: one sequence of --bases bases (A, C, G, T, with runs of N and some lower case), 60 bases a line, written to a temporary directory and
read back through the page cache (it has just been written: the figures hold no disk time).  Two target sets on it:

  exome   --exome-targets targets of about 150 bases (log-normal), spread over the whole sequence, in order, no overlaps
  genes   --gene-targets targets of gene size (log-normal around 25 kb, 1 kb .. 500 kb), uniform starts, overlapping freely

and per set

  wall_ms         gc_content(index, ...) from the file to the column: the reads of the file's pieces, their staging, upload and counting,
                  the copy back and the division
  kernel_ms       k_gc_count alone, from the events the library brackets it with (ed_gc_kernel_ms)
  read_ms         the same pieces read from the file and nothing else
  upload_ms       the bytes of those pieces from pinned host memory to the device and nothing else (64 MiB a copy)
  host_numpy_ms   the same column in numpy on the host: the file into memory, a 256-entry class table, two running sums, two differences
  equal           the device column and the host's are the same bits (asserted)

index_scan_ms is FastaIndex on the file without a .fai (the numpy scan for line ends).  Medians over --steps repetitions after --warmup, with the
spread (min, max).

    python tools/bench_gc.py [--bases 250000000] [--exome-targets 200000] [--gene-targets 20000] [--steps 3] [--warmup 1] [--out profiles/gc_content.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH = 60
PIECE = 64 << 20


def write_sequence(rng, n_bases, path):
    letters = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n_bases, dtype=np.uint8)]
    for s in rng.integers(0, n_bases - 200000, 40):                   # runs of N: the gaps of an assembly
        letters[s:s + int(rng.integers(1000, 200000))] = 78
    for s in rng.integers(0, n_bases - 5000, n_bases // 100000):      # soft-masked repeats
        letters[s:s + int(rng.integers(100, 5000))] |= 0x20
    full = n_bases // WIDTH
    with open(path, "wb") as f:
        f.write(b">bench synthetic sequence\n")
        body = np.empty((full, WIDTH + 1), np.uint8)
        body[:, :WIDTH] = letters[:full * WIDTH].reshape(full, WIDTH)
        body[:, WIDTH] = 10
        f.write(body.tobytes())
        if n_bases > full * WIDTH:
            f.write(letters[full * WIDTH:].tobytes() + b"\n")


def exome_targets(rng, n_bases, n):
    width = np.clip(np.exp(rng.normal(np.log(150.0), 0.6, n)), 20, 8000).astype(np.int64)
    room = n_bases - int(width.sum()) - n
    gap = rng.exponential(1.0, n)
    gap = 1 + (gap / gap.sum() * room * 0.98).astype(np.int64)
    start = np.cumsum(gap + width) - width + 1
    return start, start + width - 1


def gene_targets(rng, n_bases, n):
    width = np.clip(np.exp(rng.normal(np.log(25000.0), 1.0, n)), 1000, 500000).astype(np.int64)
    start = 1 + (rng.random(n) * (n_bases - width)).astype(np.int64)
    return start, start + width - 1


def host_numpy(idx, start, end):
    """the column on the host: what a numpy user would write"""
    data = np.fromfile(idx.path, dtype=np.uint8)
    table = np.zeros(256, np.int8)
    table[list(b"GCgc")] = 1
    gc = np.zeros(data.size + 1, np.int32)
    np.cumsum(table[data], dtype=np.int32, out=gc[1:])
    table[list(b"ATat")] = 1
    atgc = np.zeros(data.size + 1, np.int32)
    np.cumsum(table[data], dtype=np.int32, out=atgc[1:])
    first, last = idx.byte_range("bench", start, end)
    g, a = gc[last] - gc[first], atgc[last] - atgc[first]
    out = np.full(g.size, np.nan)
    np.divide(g, a, out=out, where=a > 0)
    return out


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def _same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64), b[~np.isnan(b)].view(np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=250_000_000)
    ap.add_argument("--exome-targets", type=int, default=200_000)
    ap.add_argument("--gene-targets", type=int, default=20_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from exomedepth_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build()
    import exomedepth_amd as ed
    from exomedepth_amd import _lib
    from exomedepth_amd.fasta import FastaIndex
    if ed.device_count() <= 0:
        raise SystemExit("bench_gc: no GPU (a measurement path does not fall back)")
    rng = np.random.default_rng(a.seed)
    out = {"tool": "bench_gc", "seed": a.seed, "bases": a.bases, "line_bases": WIDTH, "geometry": ed.gc_geometry(), "kernel_sources": _build.csrc_sha16(),
           "file": "a temporary file just written: read through the page cache"}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.fa")
        write_sequence(rng, a.bases, path)
        out["file_bytes"] = os.path.getsize(path)
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            idx = FastaIndex(path)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["index_scan_ms"] = _stats(ts)
        assert idx.records == [("bench", a.bases, 26, WIDTH, WIDTH + 1)]
        pinned = ed.PinnedArray((PIECE,), np.uint8)
        dev = ed.DeviceArray(nbytes=PIECE)
        for case, (start, end) in (("exome", exome_targets(rng, a.bases, a.exome_targets)), ("genes", gene_targets(rng, a.bases, a.gene_targets))):
            chrom = ["bench"] * start.size
            wall, kern, got, st = [], [], None, {}
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                got = ed.gc_content(idx, chrom, start, end, stats=st)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    wall.append((t1 - t0) * 1e3); kern.append(st["kernel_ms"])
            first, last = idx.byte_range("bench", start, end)
            lo, hi = int(first.min()), int(last.max())
            read, up = [], []
            for i in range(a.steps):
                t0 = time.perf_counter()
                with open(path, "rb") as f:
                    f.seek(lo)
                    for p in range(lo, hi, PIECE):
                        f.read(min(PIECE, hi - p))
                read.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                for p in range(lo, hi, PIECE):
                    _lib.check(_lib.lib().ed_memcpy_h2d(dev.ptr, pinned.ptr, min(PIECE, hi - p)))
                up.append((time.perf_counter() - t0) * 1e3)
            host, want = [], None
            for i in range(2):
                t0 = time.perf_counter()
                want = host_numpy(idx, start, end)
                host.append((time.perf_counter() - t0) * 1e3)
            assert _same(got, want), "the device column differs from the host's"
            width = end - start + 1
            out[case] = {"targets": int(start.size), "median_target_bases": int(np.median(width)), "target_bytes": int((last - first).sum()),
                         "pieces": st["pieces"], "bytes_read": st["bytes_read"], "equal": True, "nan_targets": int(np.isnan(got).sum()),
                         "wall_ms": _stats(wall), "kernel_ms": _stats(kern), "read_ms": _stats(read), "upload_ms": _stats(up), "host_numpy_ms": _stats(host)}
            k = out[case]["kernel_ms"]["median_ms"]
            out[case]["kernel_GBps_of_target_bytes"] = out[case]["target_bytes"] / (k * 1e-3) / 1e9 if k > 0 else None
            out[case]["upload_GBps"] = (hi - lo) / (out[case]["upload_ms"]["median_ms"] * 1e-3) / 1e9
        pinned.free(); dev.free()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
