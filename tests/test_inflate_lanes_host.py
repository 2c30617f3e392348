"""The decoder's lane executor (edinf::Lanes in exomedepth_amd/csrc/ed_inflate.hpp -- what k_bgzf_inflate runs on the 64 lanes of a wavefront) on
the CPU: tools/inflate_lanes_check.cpp runs inflate_stream on 64 and on 3 emulated lanes, one lane at a time between two barriers, in forward,
reverse and seeded random order, over the hand-made blocks of tests/inflate_cases.py (lane_cases, lane_bad_blocks, oversize_cases) and the cases()
blocks under 4 KiB.  Python's zlib labels the blocks; the refusals must get the Serial executor's status.

Then the header's claim "a w.sync() stands wherever a lane reads what another lane wrote" is turned round: for every `w.sync();` in the header a
copy without that one statement is built and run, and must FAIL under some schedule -- or the site is listed in REDUNDANT with its argument.
CPU test; the processes run side by side."""
import os
import re
import struct
import subprocess

import inflate_cases as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "exomedepth_amd", "csrc", "ed_inflate.hpp")
SOURCE = os.path.join(ROOT, "tools", "inflate_lanes_check.cpp")
# a process each: (part of the cases, schedules)
SCHEDULES = [(part, [s]) for s in ("64:forward", "64:reverse", "64:random:1") for part in ("0/2", "1/2")] + [("0/1", ["3:forward", "3:reverse", "3:random:1", "3:random:2"])]
MUTANT_SCHEDULES = ["64:forward", "64:reverse", "64:random:1", "3:reverse"]

# Sites (function # ordinal within it) whose removal no schedule can show, each with the reason.  DESIGN 4.25 has the same list.
REDUNDANT = {
    "fixed_tables#1": "what follows it only WRITES t.lens, a lane its own entries; the last readers of t.lens (the third phase of the previous "
                      "block's huff_build) lie before that huff_build's closing barrier, and the next reader lies behind the opening barrier of "
                      "the huff_build that follows",
    "read_dynamic_tables#1": "t.cl_lens and t.cl are touched only between this point and the opening barrier of huff_build(t.lit); every lane "
                             "writes all of cl_lens itself, with the same values, and a lane that is ahead stops at huff_build(t.cl)'s opening barrier",
}
# the issue's three: if the emulator misses one of these, the cases or the schedules are too weak
MUST_DETECT = ("copy_match#1", "inflate_stream#1", "huff_build#2")
SYNC = "w.sync();"


def sync_sites(text):
    """[(label, offset)] of every `w.sync();` statement of the header, labelled by the function it stands in"""
    funcs = [(m.start(), m.group(1)) for m in re.finditer(r"^ED_INF_HD \w[\w ]*?\b(\w+)\(", text, re.M)]
    out, seen = [], {}
    for m in re.finditer(re.escape(SYNC), text):
        line = text[text.rfind("\n", 0, m.start()) + 1:m.start()]
        if "//" in line:                                     # (the header's comment speaks of w.sync() too)
            continue
        name = [n for at, n in funcs if at < m.start()][-1]
        seen[name] = seen.get(name, 0) + 1
        out.append(("%s#%d" % (name, seen[name]), m.start()))
    return out


def _compile(cc, exe, opt, defines=()):
    return subprocess.Popen([cc, "-std=c++17", opt, "-Wall", "-Wextra", "-Werror", *defines, SOURCE, "-o", exe, "-lstdc++", "-lm"],
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_lane_executor_under_schedules_and_sync_mutation(tmp_path):
    cc = os.environ.get("ED_SHIM_CC", "gcc")                  # the compiler tests/test_shim.py builds with
    text = open(HEADER).read()
    sites = sync_sites(text)
    labels = [l for l, _ in sites]
    assert len(labels) >= 7 and set(MUST_DETECT) <= set(labels) and set(REDUNDANT) <= set(labels), labels
    assert not set(MUST_DETECT) & set(REDUNDANT)
    # the compilers first: they run while the cases are made
    exe = str(tmp_path / "inflate_lanes_check")
    builds = [("shipped", exe, _compile(cc, exe, "-O1"))]
    for label, at in sites:
        d = tmp_path / re.sub(r"\W", "_", label)
        d.mkdir()
        (d / "ed_inflate.hpp").write_text(text[:at] + text[at + len(SYNC):])
        m_exe = str(d / "inflate_lanes_check")
        # a decoder that lost a barrier may walk tables another lane is still writing: room behind them (15 lengths x 288 symbols x 2 bytes at most)
        defines = ['-DED_INFLATE_HEADER="%s"' % (d / "ed_inflate.hpp"), "-DED_LANES_TABLE_SLACK=16384"]
        builds.append((label, m_exe, _compile(cc, m_exe, "-O0", defines)))

    lane, over, bad = list(ic.lane_cases()), ic.oversize_cases(), ic.lane_bad_blocks()
    small = [c for c in ic.cases() if len(c[1]) < 4096]
    assert len(ic.triples()) >= 1500 and len(small) >= 20
    rows = [(n, b, 1, p) for n, b, p in lane + over + small] + [(n, b, 0, b"") for n, b, _ in bad]
    rows.sort(key=lambda r: len(r[1]))                       # the short ones first: a copy that lost a barrier it needs fails at once
    path, tables_path = str(tmp_path / "cases.bin"), str(tmp_path / "tables.bin")
    # (the two listed sites stand in the table building, once a DEFLATE block, whatever its length: their copies run on the blocks under 4 KiB,
    # which build every table the longer ones build -- the fixed code, DENSE_LIT / DENSE_DIST, zlib's)
    for name, sel in ((path, rows), (tables_path, [r for r in rows if len(r[1]) < 4096])):
        with open(name, "wb") as f:
            f.write(b"EDINFCS1" + struct.pack("<I", len(sel)))
            for _, b, accept, p in sel:
                f.write(struct.pack("<III", len(b), accept, len(p)) + b + p)

    for label, _, proc in builds:
        out, _ = proc.communicate(timeout=300)
        assert proc.returncode == 0, (label, out)
    runs = [("shipped", s, subprocess.Popen([exe, path, "--part", part] + s, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
            for part, s in SCHEDULES]
    for label, m_exe, _ in builds[1:]:
        if label in REDUNDANT:                               # must pass
            runs.append((label, MUTANT_SCHEDULES, subprocess.Popen([m_exe, tables_path] + MUTANT_SCHEDULES, stdout=subprocess.PIPE,
                                                                   stderr=subprocess.STDOUT, text=True)))
        else:
            runs.append((label, MUTANT_SCHEDULES, subprocess.Popen([m_exe, path, "--first"] + MUTANT_SCHEDULES, stdout=subprocess.PIPE,
                                                                   stderr=subprocess.STDOUT, text=True)))
    detected, missed, n_ok, n_runs = [], [], 0, 0
    for label, sched, proc in runs:
        out, _ = proc.communicate(timeout=300)
        tail = "\n".join(out.splitlines()[-6:])
        if label == "shipped":
            print(" ".join(sched), "->", tail)
            if proc.returncode != 0:
                print("\n".join("case %d = %s" % (k, r[0]) for k, r in enumerate(rows)))
            m = re.match(r"ok: (\d+) cases \(part \d+ of (\d+)\) under (\d+) schedules, (\d+) runs", out.splitlines()[-1])
            assert proc.returncode == 0 and m and (int(m.group(1)), int(m.group(3))) == (len(rows), len(sched)), out[-3000:]
            n_ok += 1
            n_runs += int(m.group(4))
        elif label in REDUNDANT:
            assert proc.returncode == 0, "%s is listed as redundant, yet the emulator fails without it: take it off the list\n%s" % (label, tail)
        else:
            # any other end than a clean pass is a detection: a failed check (exit status 1) or a fault of the decoder that walked half-written tables
            (missed if proc.returncode == 0 else detected).append(label)
            print("without %s:" % label, out.splitlines()[0] if out else "(exit status %d)" % proc.returncode)
    assert n_ok == len(SCHEDULES) and n_runs == 7 * len(rows)      # every case under the three orders on 64 lanes and the four on 3
    print("detected:", detected, "redundant:", sorted(REDUNDANT))
    assert not missed, "no schedule shows the loss of %s: strengthen the cases or the schedules, or argue the site redundant" % missed
    assert set(MUST_DETECT) <= set(detected)
