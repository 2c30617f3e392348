"""The BGZF block decoder's rules (exomedepth_amd/csrc/ed_inflate.hpp -- the header the device kernel k_bgzf_inflate is built from) are host code as
well: tools/inflate_check.cpp runs its serial inflate_block, without zlib, over the cases of tests/inflate_cases.py, which Python's zlib labels.
A block is accepted if and only if exomedepth_amd.bam._inflate returns, and then the bytes are equal.  CPU test: the checker compiles (without the
sanitizer flags its header comment gives for a run by hand) and exits with status 0."""
import os
import re
import struct
import subprocess

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(tmp_path, rows, n_print):
    """rows [(block, accept code, expected bytes)] through the checker: {case: (status name, longest code, DEFLATE blocks)}"""
    path = tmp_path / "cases.bin"
    with open(path, "wb") as f:
        f.write(b"EDINFCS1" + struct.pack("<I", len(rows)))
        for b, accept, p in rows:
            f.write(struct.pack("<III", len(b), accept, len(p)) + b + p)
    cc = os.environ.get("ED_SHIM_CC", "gcc")          # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "inflate_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "inflate_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe, str(path), "--sample"], capture_output=True, text=True)     # (the hand run under the sanitizers takes every truncation)
    lines = r.stdout.splitlines()
    print("\n".join(lines[:n_print] + [l for l in lines[n_print:] if not l.startswith("case ")]), r.stderr)
    assert r.returncode == 0
    assert lines[-1].startswith("ok")
    got = {}
    for line in lines:
        m = re.match(r"case (\d+) status (\w+) max_code_len (\d+) deflate_blocks (\d+)", line)
        if m:
            got[int(m.group(1))] = (m.group(2), int(m.group(3)), int(m.group(4)))
    assert len(got) == len(rows)
    return got


def test_inflate_checker(tmp_path):
    good = ic.cases()
    bad = ic.bad_blocks()
    rows = [(b, 2, p) for _, b, p in good] + [(b, 0, b"") for _, b, _ in bad]
    n_fixed = len(rows)
    n_corrupt_accepted = 0
    for _, b, _ in ic.small_blocks():
        for c, p in ic.corruptions(b):
            rows.append((c, 0 if p is None else 1, p or b""))
            n_corrupt_accepted += p is not None
    assert n_corrupt_accepted > 0                     # the header bytes _inflate does not read: corrupting them changes nothing
    got = _check(tmp_path, rows, n_fixed)
    names = [n for n, _, _ in good]
    assert got[names.index("fibonacci huffman-only")][1] == 15          # the walk past the primary table was really taken
    assert got[names.index("full flush")][2] >= 3                       # two coded blocks and the empty stored one between them
    for k, (name, _, status) in enumerate(bad):
        assert got[len(good) + k][0] != "OK", name
        if status is not None:
            assert got[len(good) + k][0] == status, (name, got[len(good) + k][0])


def test_inflate_checker_lane_cases(tmp_path):
    """the hand-made blocks at the lane executor's edges and the refusals zlib's output never reaches, through the serial executor (accept code 1:
    --sample adds no truncation runs).  The same lists run on emulated lanes in tests/test_inflate_lanes_host.py and on the device."""
    good = list(ic.lane_cases()) + ic.oversize_cases()
    bad = ic.lane_bad_blocks()
    assert len(ic.triples()) >= 1500 and all(len(p) <= ic.MAX_LANE_PAYLOAD or "isize" in n or "stored 65" in n for n, _, p in good)
    got = _check(tmp_path, [(b, 1, p) for _, b, p in good] + [(b, 0, b"") for _, b, _ in bad], len(good) + len(bad))
    names = [n for n, _, _ in good]
    for k, name in enumerate(names):
        assert got[k][0] == "OK", name
    assert got[names.index("all fifteen code lengths in both codes")][1] == 15
    assert got[names.index("stored fixed dynamic stored fixed, 64 pending")][2] == 5
    for k, (name, _, status) in enumerate(bad):
        assert got[len(good) + k][0] == status, (name, got[len(good) + k][0])
