"""Build libedcore.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libedcore.so")
SOURCES = ["edcore.hip"]
def _deps():
    """every file the library is built from: all of csrc/ (sources, .inc, headers -- generated tables included) + the C-ABI header"""
    names = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".inc", ".hpp", ".h")))
    return names + ["../../include/exomedepth_amd.h"]


DEPS = _deps()
# -ffp-contract=off is part of the numerical contract (see csrc/ed_pmath.h): no implicit fma.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
         "-fvisibility=hidden"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, /opt/rocm/bin/hipcc, PATH)")


def csrc_sha16():
    """Fingerprint of the kernel sources (the files libedcore.so is built from).  rocprofv3 summaries under profiles/ are
    stamped with it (tools/profile_round.sh); bench.py only quotes counter-derived figures from a profile whose stamp
    equals the tree's, so a changed kernel can never be described by a stale profile."""
    import hashlib
    h = hashlib.sha256()
    for d in sorted(DEPS):
        p = os.path.join(CSRC, d)
        if os.path.exists(p):
            h.update(d.encode()); h.update(open(p, "rb").read())
    return h.hexdigest()[:16]


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    for d in DEPS:
        p = os.path.join(CSRC, d)
        if os.path.exists(p) and os.path.getmtime(p) > t:
            return True
    return False


def build(force=False, verbose=False):
    if not force and not stale():
        return LIB
    cmd = [hipcc()] + FLAGS + ["-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(" ".join(cmd))
        print(r.stdout)
        print(r.stderr)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed building libedcore.so")
    return LIB


# Diagnostic variants of the library (same sources, different code generation); never loaded by the package itself.
VARIANTS = {# every automatic variable starts from a bit pattern (0xAA...) instead of whatever the register or stack slot held: a read of an uninitialised
            # variable shows up as a wrong (and reproducible) result instead of a run-to-run difference -- host and device code
            "autoinit": ["-ftrivial-auto-var-init=pattern"],
            # k_fit_hnewton's per-cell path with the short digamma series (irreproducible fits), alone and with pattern-initialised variables
            "hnshort": ["-DED_HN_SHORT_SERIES"], "hnshortinit": ["-DED_HN_SHORT_SERIES", "-ftrivial-auto-var-init=pattern"],
            "hnshortplain": ["-DED_HN_SHORT_SERIES", "-DED_FIT_PLAIN_FMA"], "fitplain": ["-DED_FIT_PLAIN_FMA"],
            # k_tb_paths also writes the byte-per-exon path in every run, as it did before the path was made on request (edcore.hip, trace-back
            # block): the other side of tools/ab.sh eagerpath
            "eagerpath": ["-DED_EAGER_BYTE_PATH"],
            # host code under the sanitizers (device code is left alone: -fno-gpu-sanitize); tools/sanitize.sh
            # (no -shared-libsan: the runtime is whatever tools/sanitize.sh preloads -- gcc's stock libasan / libtsan; ROCm's own
            # ASan runtime intercepts hsa_amd_memory_pool_allocate for DEVICE instrumentation and fails on a plain process)
            "asan": ["-fsanitize=address,undefined", "-fno-sanitize=vptr,function", "-fno-gpu-sanitize", "-g", "-fno-omit-frame-pointer", "-Wl,--unresolved-symbols=ignore-all"],
            "tsan": ["-fsanitize=thread", "-fno-gpu-sanitize", "-g", "-fno-omit-frame-pointer", "-Wl,--unresolved-symbols=ignore-all"]}


def variant_path(name):
    return os.path.join(HERE, "libedcore_%s.so" % name)


def build_variant(name, force=False, verbose=False):
    out = variant_path(name)
    if not force and os.path.exists(out) and not stale() and os.path.getmtime(out) >= os.path.getmtime(LIB):
        return out
    cmd = [hipcc()] + FLAGS + VARIANTS[name] + ["-o", out] + [os.path.join(CSRC, s) for s in SOURCES]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(" ".join(cmd)); print(r.stdout); print(r.stderr)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed building %s" % out)
    return out


if __name__ == "__main__":
    print(build(force=True, verbose=True))
