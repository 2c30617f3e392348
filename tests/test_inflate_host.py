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
    print("\n".join(lines[:n_fixed] + [l for l in lines[n_fixed:] if not l.startswith("case ")]), r.stderr)
    assert r.returncode == 0
    assert lines[-1].startswith("ok")
    got = {}
    for line in lines:
        m = re.match(r"case (\d+) status (\w+) max_code_len (\d+) deflate_blocks (\d+)", line)
        if m:
            got[int(m.group(1))] = (m.group(2), int(m.group(3)), int(m.group(4)))
    assert len(got) == len(rows)
    names = [n for n, _, _ in good]
    assert got[names.index("fibonacci huffman-only")][1] == 15          # the walk past the primary table was really taken
    assert got[names.index("full flush")][2] >= 3                       # two coded blocks and the empty stored one between them
    for k, (name, _, status) in enumerate(bad):
        assert got[len(good) + k][0] != "OK", name
        if status is not None:
            assert got[len(good) + k][0] == status, (name, got[len(good) + k][0])
