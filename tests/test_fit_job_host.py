"""The request of the dispersion fit (exomedepth_amd/csrc/ed_fit_job.hpp: the four named constructors of a FitJob, the refusals fit_columns
applies before it enqueues anything, the choice of histogram geometries to launch) is host code: tools/fit_job_check.cpp checks it against the
strides and messages the callers used before there was a FitJob.  CPU test: the checker compiles (without the sanitizer flags its header
comment gives for a run by hand) and exits with status 0."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fit_job_checker(tmp_path):
    cc = os.environ.get("ED_SHIM_CC", "gcc")       # the compiler tests/test_shim.py builds with
    exe = str(tmp_path / "fit_job_check")
    subprocess.run([cc, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tools", "fit_job_check.cpp"), "-o", exe, "-lstdc++", "-lm"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0
    assert "ok" in r.stdout
