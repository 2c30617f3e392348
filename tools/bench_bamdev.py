#!/usr/bin/env python
"""Times reading a BAM file by both routes -- the host's (exomedepth_amd.bam.BamFile: thread pool + ed_bam_scan_records) and the device's
(csrc/edinflate.inc through bam.DeviceInflater / bam.DeviceBamFile) -- on written samples and writes one JSON record:

    python tools/bench_bamdev.py [--records 400000] [--reps 5] [--warmup 2] [--out profiles/bam_device.json]

The sample comes from the tests' writer (tests/readcount_checker.write_bam): coordinate-sorted records of 150 bases, in two files -- one whose
blocks start on record boundaries and one cut at a fixed payload size (which changes nothing for the inflating; it is the case a device record scan
would have to fix up).  Per file and route: median wall milliseconds of the whole inflated() generator (file read, staging, upload, kernel and the
copy back included), inflated bytes per second; the records leg (host: BamFile.chunks() = inflate + scan; device: DeviceBamFile.batches() =
upload, inflate, scan, gather, the fields staying on the device) with the three kernel figures of ed_bamdev_kernel_ms; and the whole getBamCounts by
both routes.  The writer's records carry made-up constant bases and qualities, which compress about 39-fold; a third file ("random_bases") has
random bases and qualities drawn from a skewed distribution, which compress about as a real BAM does.  The device stream and records are compared
with the host's."""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                           # noqa: E402

import exomedepth_amd as ed                                  # noqa: E402
from exomedepth_amd import bam                               # noqa: E402
import readcount_checker as rck                              # noqa: E402


def write_sample(path, n, aligned):
    r = np.random.default_rng(1)
    pos = np.sort(r.integers(0, 2 * 10 ** 8, n))
    recs = [(0, int(p), 60, 0x1 | 0x2 | (0x10 if k & 1 else 0), 300, 12, 1, 150) for k, p in enumerate(pos)]
    stream, first = rck.bam_stream("@HD\tVN:1.0\tSO:coordinate\n", [("1", 249250621)], recs)
    if not aligned:
        rck.write_bgzf(path, stream, 65280)
        return
    sizes, p, start = [first], first, first                  # the header a block of its own, then whole records up to 65 280 bytes a block
    while p < len(stream):
        bs = 4 + struct.unpack_from("<i", stream, p)[0]
        if p + bs - start > 65280:
            sizes.append(p - start)
            start = p
        p += bs
    sizes.append(p - start)
    rck.write_bgzf(path, stream, sizes)


def write_random_sample(path, n):
    """records of 150 random bases with skewed random qualities, blocks on record boundaries"""
    r = np.random.default_rng(2)
    name, rec_len = 13, 32 + 13 + 4 + 75 + 150
    a = np.zeros((n, 4 + rec_len), np.uint8)
    fixed = np.zeros(n, dtype=[("bs", "<i4"), ("refid", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("ncig", "<u2"),
                               ("flag", "<u2"), ("lseq", "<u4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")])
    fixed["bs"], fixed["pos"], fixed["lname"], fixed["mapq"], fixed["bin"] = rec_len, np.sort(r.integers(0, 2 * 10 ** 8, n)), name, 60, 4680
    fixed["ncig"], fixed["flag"], fixed["lseq"], fixed["nref"], fixed["npos"], fixed["tlen"] = 1, 0x3, 150, -1, -1, 300
    a[:, :36] = fixed.view(np.uint8).reshape(n, 36)
    a[:, 36:36 + name - 1] = r.integers(48, 58, (n, name - 1))
    a[:, 36 + name:36 + name + 4] = np.frombuffer(struct.pack("<I", 150 << 4), np.uint8)
    nib = np.array([1, 2, 4, 8], np.uint8)
    a[:, 53:128] = (nib[r.integers(0, 4, (n, 75))] << 4) | nib[r.integers(0, 4, (n, 75))]
    a[:, 128:] = np.minimum(40, r.geometric(0.12, (n, 150)) + 2).astype(np.uint8)
    head, first = rck.bam_stream("@HD\tVN:1.0\tSO:coordinate\n", [("1", 249250621)], [])
    per = 65280 // (4 + rec_len)
    body = a.tobytes()
    sizes = [first] + [per * (4 + rec_len)] * (n // per) + ([(n % per) * (4 + rec_len)] if n % per else [])
    rck.write_bgzf(path, head + body, sizes)


def timed(fn, reps, warmup):
    out = []
    for k in range(reps + warmup):
        t = time.perf_counter()
        r = fn()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=400000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_device.json"))
    a = ap.parse_args()
    rec = {"records": a.records, "threads": bam.n_threads(), "geometry": bam.bamdev_geometry(), "files": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for name, aligned in (("blocks_on_record_boundaries", True), ("fixed_payload_65280", False), ("random_bases", None)):
            path = os.path.join(tmp, name + ".bam")
            if aligned is None:
                write_random_sample(path, a.records)
            else:
                write_sample(path, a.records, aligned)
            host_ms, host = timed(lambda: b"".join(bam.inflated(path)), a.reps, a.warmup)
            kms = []

            def device():
                with bam.DeviceInflater(0, 32 << 20) as d, open(path, "rb") as f:
                    d.begin()
                    data = f.read()
                    off = 0
                    while off < len(data):
                        off += d.push(memoryview(data)[off:])
                    d.end()
                    kms.append(d.kernel_ms()[0])
                return None
            timed(device, a.reps, a.warmup)
            dev_ms, dev = timed(lambda: b"".join(bam.inflated(path, device=0)), a.reps, a.warmup)
            assert dev == host
            rec["files"][name] = {"compressed_bytes": os.path.getsize(path), "inflated_bytes": len(host),
                                  "host_inflate_ms": round(host_ms, 3), "device_inflate_ms": round(dev_ms, 3),
                                  "k_bgzf_inflate_ms": round(statistics.median(kms[a.warmup:]), 4),
                                  "host_inflated_GBps": round(len(host) / host_ms / 1e6, 3), "device_inflated_GBps": round(len(host) / dev_ms / 1e6, 3),
                                  "kernel_inflated_GBps": round(len(host) / statistics.median(kms[a.warmup:]) / 1e6, 3),
                                  "device_over_host": round(host_ms / dev_ms, 3)}
            def host_records():
                with bam.BamFile(path) as b:
                    return [c for c in b.chunks()]

            def device_records():
                f = bam.DeviceBamFile(path)
                n = sum(r.n for r in f.batches())
                return n, f.kernel_ms
            hr_ms, hr = timed(host_records, a.reps, a.warmup)
            dr_ms, (n_dev, k3) = timed(device_records, a.reps, a.warmup)
            assert n_dev == sum(c[0].size for c in hr) == a.records
            want = tuple(np.concatenate([c[k] for c in hr]) for k in range(4))
            assert all(np.array_equal(x, y) for x, y in zip(bam.DeviceBamFile(path).records(), want))
            rec["files"][name].update({"host_records_ms": round(hr_ms, 3), "device_records_ms": round(dr_ms, 3),
                                       "device_records_over_host": round(hr_ms / dr_ms, 3),
                                       "kernel_ms_inflate_scan_gather": [round(v, 4) for v in k3]})
            if aligned is not False:
                s = np.arange(0, 2 * 10 ** 8, 10 ** 4)
                frame = {"chromosome": ["1"] * s.size, "start": s, "end": s + 10 ** 4}
                h_ms, h = timed(lambda: ed.getBamCounts(bed_frame=frame, bam_files=[path]), a.reps, a.warmup)
                d_ms, d = timed(lambda: ed.getBamCounts(bed_frame=frame, bam_files=[path], inflate="device"), a.reps, a.warmup)
                assert all(np.array_equal(np.asarray(h[k]), np.asarray(d[k])) for k in h)
                rec["files"][name]["getBamCounts_ms"] = {"inflate_host": round(h_ms, 3), "inflate_device": round(d_ms, 3)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
