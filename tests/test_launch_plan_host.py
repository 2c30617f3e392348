"""The launch plan of ed_batch_run (exomedepth_amd/csrc/ed_launch_plan.hpp: job order, overlap groups, segment tables, the head / cut / rest
pieces of a group's emissions, grids) is host arithmetic: tools/launch_plan_check.cpp checks it against hand-derived cases and, over a seeded
sweep of designs, against its own restatement of the kernels' index decode.  CPU test: the checker compiles (without the sanitizer flags its
header comment gives for a run by hand) and exits with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_plan_checker(tmp_path):
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "launch_plan_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "launch_plan_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout
