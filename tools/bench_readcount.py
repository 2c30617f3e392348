#!/usr/bin/env python
"""Times the read counter (csrc/edreadcount.inc, api.ReadCounter) on one synthetic coordinate-sorted sample and writes one JSON record:

  device_ms       ReadCounter.add + finish + the copy of the column back: the upload of the four record arrays (staged, under the kernels) plus
                  the counting -- wall time of the whole call sequence
  kernel_ms       k_rcnt_bin + k_rcnt_finish alone, from the events the library brackets them with
  host_rank_ms    the same rank method on the host: the filter, np.searchsorted twice per chromosome, np.bincount, cumsum -- on this machine
  equal           the device counts and the host form's are the same array (asserted)
  inflate_scan    reading a BAM file made by the tests' writer (tests/readcount_checker.py): BGZF blocks inflated on the thread pool, records
                  scanned by ed_bam_scan_records -- no device in it; records/s and what that makes for --records records

The sample: --records records against --exons exons on 24 chromosomes, exon widths log-normal around 130 bp, gaps exponential (mean 14 kb), about
40 % of the fragments drawn off target (uniform over the chromosome), the rest on a random exon; mostly proper pairs, some duplicates, unpaired
reads, low mapq.  Sorted by (chromosome, position) as a BAM is.  Medians over --steps repetitions after --warmup, with the spread (min, max).

    python tools/bench_readcount.py [--records 50000000] [--exons 200000] [--steps 5] [--warmup 2] [--bam-records 400000] [--out profiles/readcount.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CHROM = 24


def design(rng, n_exons):
    """exons of 24 chromosomes, in genomic order: (chrom id, start, end) 1-based closed, and the span of every chromosome"""
    per = np.full(N_CHROM, n_exons // N_CHROM)
    per[:n_exons - per.sum()] += 1
    chrom = np.repeat(np.arange(N_CHROM), per)
    width = np.clip(np.exp(rng.normal(np.log(130.0), 0.7, n_exons)), 20, 8000).astype(np.int64)
    gap = 50 + rng.exponential(14000.0, n_exons).astype(np.int64)
    start = np.empty(n_exons, np.int64)
    span = np.zeros(N_CHROM, np.int64)
    off = np.concatenate([[0], np.cumsum(per)])
    for c in range(N_CHROM):
        s = slice(off[c], off[c + 1])
        start[s] = 10000 + np.cumsum(gap[s] + width[s]) - width[s]
        span[c] = start[s][-1] + width[s][-1] + 10000
    return chrom, start, start + width - 1, span


def sample(rng, n, chrom, start, end, span):
    """(refid, pos, tlen, flag_mapq) of n records, coordinate-sorted"""
    on = rng.random(n) >= 0.4
    e = rng.integers(0, start.size, n)
    tlen = np.clip(rng.normal(300.0, 60.0, n), 60, 900).astype(np.int64)
    refid = np.where(on, chrom[e], rng.integers(0, N_CHROM, n))
    pos = np.where(on, start[e] - tlen + 1 + (rng.random(n) * (end[e] - start[e] + tlen)).astype(np.int64), (rng.random(n) * span[refid]).astype(np.int64))
    pos = np.maximum(pos, 0)
    flag = np.full(n, 0x1 | 0x2 | 0x40, np.int64)
    u = rng.random(n)
    flag = np.where(u < 0.06, flag | 0x400, flag)                  # duplicates
    flag = np.where((u >= 0.06) & (u < 0.08), 0, flag)             # unpaired
    flag = np.where((u >= 0.08) & (u < 0.10), 0x1 | 0x10, flag)    # not proper pairs
    flag = np.where(rng.random(n) < 0.5, flag | 0x10, flag)
    tlen = np.where(rng.random(n) < 0.5, tlen, -tlen)              # the mate to the right / to the left
    mapq = np.where(rng.random(n) < 0.07, rng.integers(0, 21, n), 60)
    order = np.lexsort((pos, refid))
    return (refid[order].astype(np.int32), pos[order].astype(np.int32), tlen[order].astype(np.int32),
            (flag | (mapq << 16))[order].astype(np.uint32))


def host_rank_form(rec, chrom, start, end, min_mapq=20, read_width=300):
    """getBamCounts' rule by the kernel's method, in numpy: filter, two searches, two histograms, two scans"""
    refid, pos, tlen, fm = rec
    flag, mapq = fm & 0xFFFF, (fm >> 16) & 0xFF
    paired = (flag & 0x1) != 0
    keep = (mapq != 255) & (mapq > min_mapq) & np.where(paired, ((flag & 0x2) != 0) & ((flag & (0x4 | 0x8 | 0x100 | 0x400)) == 0) & (tlen > 0),
                                                        (flag & (0x4 | 0x100 | 0x400)) == 0)
    fs = pos.astype(np.int64) + 1
    fe = fs + np.where(paired, tlen, read_width)
    out = np.zeros(start.size, np.int64)
    lo = np.searchsorted(refid, np.arange(N_CHROM), "left")       # the records are sorted by chromosome
    hi = np.searchsorted(refid, np.arange(N_CHROM), "right")
    for c in range(N_CHROM):
        ex = np.flatnonzero(chrom == c)
        k = keep[lo[c]:hi[c]]
        a, b = fs[lo[c]:hi[c]][k], fe[lo[c]:hi[c]][k]
        by_end, by_start = np.argsort(end[ex], kind="stable"), np.argsort(start[ex], kind="stable")
        rA = np.searchsorted(end[ex][by_end], a, "left")
        rB = np.searchsorted(start[ex][by_start], b, "right")
        cumA = np.cumsum(np.bincount(rA, minlength=ex.size + 1)[:ex.size])
        cumB = np.cumsum(np.bincount(rB, minlength=ex.size + 1)[:ex.size])
        rank_end, rank_start = np.empty(ex.size, np.int64), np.empty(ex.size, np.int64)
        rank_end[by_end] = np.arange(ex.size)
        rank_start[by_start] = np.arange(ex.size)
        out[ex] = cumA[rank_end] - cumB[rank_start]
    return out


def _stats(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "n": len(ts)}


def _bam_case(rng, n_records, path):
    """a BAM of n_records records of 150 bases (a 30-byte name, one CIGAR operation, qualities from a narrow alphabet), BGZF blocks by the tests' writer"""
    import readcount_checker as rck
    head, _ = rck.bam_stream("@HD\tVN:1.0\tSO:coordinate\n", [("c%d" % c, 250000000) for c in range(N_CHROM)], [])
    l_name, l_seq = 30, 150
    size = 32 + l_name + 4 + (l_seq + 1) // 2 + l_seq
    body = np.zeros((n_records, 4 + size), np.uint8)
    fixed = np.zeros(n_records, dtype=[("bs", "<i4"), ("refid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cigar", "<u2"),
                                       ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")])
    fixed["bs"], fixed["l_name"], fixed["n_cigar"], fixed["l_seq"], fixed["mapq"], fixed["flag"] = size, l_name, 1, l_seq, 60, 0x63
    fixed["refid"] = np.sort(rng.integers(0, N_CHROM, n_records))
    fixed["pos"] = rng.integers(0, 200000000, n_records)
    fixed["tlen"] = rng.integers(100, 500, n_records)
    body[:, :36] = fixed.view(np.uint8).reshape(n_records, 36)
    body[:, 36:36 + l_name - 1] = rng.integers(48, 58, (n_records, l_name - 1))
    body[:, 36 + l_name:36 + l_name + 4] = np.frombuffer(np.uint32((l_seq << 4) | 0).tobytes(), np.uint8)
    body[:, 40 + l_name:40 + l_name + 75] = rng.integers(0, 256, (n_records, 75)) & 0x77 | 0x11
    body[:, 40 + l_name + 75:] = rng.choice(np.array([11, 25, 37, 37, 37, 40], np.uint8), (n_records, l_seq))
    stream = head + body.tobytes()
    rck.write_bgzf(path, stream, 65280)
    return fixed, len(stream)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=50_000_000)
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=3)
    ap.add_argument("--bam-records", type=int, default=400_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from exomedepth_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build()
    import exomedepth_amd as ed
    from exomedepth_amd import bam
    if ed.device_count() <= 0:
        raise SystemExit("bench_readcount: no GPU (a measurement path does not fall back)")
    rng = np.random.default_rng(a.seed)
    chrom, start, end, span = design(rng, a.exons)
    rec = sample(rng, a.records, chrom, start, end, span)
    names = ["c%d" % c for c in range(N_CHROM)]
    out = {"tool": "bench_readcount", "seed": a.seed, "records": a.records, "exons": a.exons, "geometry": ed.readcount_geometry(),
           "kernel_sources": _build.csrc_sha16(), "threads": bam.n_threads(), "record_bytes_uploaded": 16 * a.records}

    rc = ed.ReadCounter([names[c] for c in chrom], start, end, 1)
    wall, kern_bin, kern_fin, got, prev = [], [], [], None, 0
    try:
        for i in range(a.warmup + a.steps):
            k0 = rc.kernel_ms()
            t0 = time.perf_counter()
            rc.add(0, rec, names)
            rc.finish(0)
            col = rc.counts()[:, 0]
            t1 = time.perf_counter()
            k1 = rc.kernel_ms()
            got = col.astype(np.int64) - prev                                # the column accumulates over the repetitions
            prev = col.astype(np.int64)
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e3); kern_bin.append(k1[0] - k0[0]); kern_fin.append(k1[1] - k0[1])
    finally:
        rc.close()
    host, want = [], None
    for i in range(a.host_steps):
        t0 = time.perf_counter()
        want = host_rank_form(rec, chrom, start, end)
        host.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(got, want), "device counts differ from the host form"
    out["equal"] = True
    out["counted_fragments"] = int(want.sum())
    out["exons_hit"] = int(np.count_nonzero(want))
    out["device_ms"], out["kernel_bin_ms"], out["kernel_finish_ms"], out["host_rank_ms"] = _stats(wall), _stats(kern_bin), _stats(kern_fin), _stats(host)
    out["records_per_s_device"] = a.records / (out["device_ms"]["median_ms"] / 1e3)
    out["records_per_s_kernel"] = a.records / ((out["kernel_bin_ms"]["median_ms"] + out["kernel_finish_ms"]["median_ms"]) / 1e3)

    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.bam")
        fixed, n_inflated = _bam_case(rng, a.bam_records, path)
        ts = []
        for i in range(1 + 3):
            t0 = time.perf_counter()
            with bam.BamFile(path) as b:
                r = b.records()
            if i:
                ts.append((time.perf_counter() - t0) * 1e3)
        assert np.array_equal(r[1], fixed["pos"]) and np.array_equal(r[2], fixed["tlen"]) and np.array_equal(r[0], fixed["refid"])
        out["inflate_scan"] = dict(_stats(ts), records=a.bam_records, inflated_bytes=n_inflated, compressed_bytes=os.path.getsize(path))
        out["inflate_scan"]["records_per_s"] = a.bam_records / (statistics.median(ts) / 1e3)
        out["inflate_scan"]["ms_for_the_sample"] = a.records / out["inflate_scan"]["records_per_s"] * 1e3
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
