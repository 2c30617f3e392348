#!/usr/bin/env python
"""Times correct_counts_using_PCA on the synthetic cohort (synth.counts_torch, 200 000 exons x 1 024 samples, nPCs = 3) and prints one JSON line:
per-stage milliseconds from ed_pca_last_info (medians over the timed calls, after warm-up), the iteration count, the Gram kernel's achieved FP64
TFLOP/s (2 n S^2 flop of the algorithm over the Gram stage's time), and the yardstick: torch's FP64 Z.T @ Z (rocBLAS) on a materialised double Z of
the same selected rows in the same process -- bare, and with the time to build Z in torch added.

    python tools/bench_pca.py [--exons 200000] [--samples 1024] [--npcs 3] [--steps 5] [--warmup 2] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_MATRIX_PEAK_TFLOPS = 78.6      # MI355X, v_mfma_f64: the floor of the Gram stage is its flop over this


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exons", type=int, default=200000)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--npcs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch          # first: libedcore.so must bind to the HIP runtime torch brought up
    if not torch.cuda.is_available():
        raise SystemExit("bench_pca: no GPU (a measurement path does not fall back)")
    import exomedepth_amd as ed
    from exomedepth_amd import synth

    dev = torch.device("cuda:0")
    chrom_off, _, _ = synth.exon_design(a.exons, 24, a.seed)
    counts = synth.counts_torch(chrom_off, a.samples, dev, seed=a.seed)[0].contiguous()
    E, S = int(counts.shape[0]), int(counts.shape[1])
    out = torch.empty_like(counts)
    torch.cuda.synchronize()
    rec = {"tool": "bench_pca", "exons": E, "samples": S, "nPCs": a.npcs, "steps": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    infos, error = [], None
    for i in range(a.warmup + a.steps):
        try:
            ed.correct_counts_using_PCA(counts, a.npcs, out=out)
        except ed.EdError as e:          # e.g. no gap in the spectrum of a cohort without batch structure: reported, with the stages that ran
            error = str(e)
        if i >= a.warmup:
            infos.append(ed.pca_last_info())
    med = lambda f: statistics.median(f(x) for x in infos)
    n = infos[0]["n_selected"]
    rec.update({"converged": error is None, "error": error, "n_selected": n, "iterations": infos[0]["iterations"], "block": infos[0]["block"],
                "residual_over_theta1": infos[0]["residual"], "theta_k_over_theta_k1": infos[0]["gap"],
                "ms": {k: med(lambda x, k=k: x["ms"][k]) for k in ("rowstats", "gram", "eigen", "residual", "total")}})
    flop = 2.0 * n * S * S
    rec["gram_flop"] = flop
    rec["gram_tflops"] = flop / (rec["ms"]["gram"] * 1e-3) / 1e12
    rec["gram_floor_ms_at_fp64_matrix_peak"] = flop / (FP64_MATRIX_PEAK_TFLOPS * 1e12) * 1e3
    rec["eigen_ms_per_iteration"] = rec["ms"]["eigen"] / max(1, rec["iterations"])
    # the yardstick: Z materialised by torch from the same rows, then rocBLAS dgemm
    g = ed.pca_gram(counts)
    sel = torch.from_numpy(g["selected"]).to(dev)
    div = torch.from_numpy(g["div"]).to(dev)
    centre = torch.from_numpy(g["centre"]).to(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_build, t_mm = [], []
    G = None
    for i in range(a.warmup + a.steps):
        ev[0].record()
        Z = counts[sel].double() / div[None, :] - centre[sel][:, None]
        ev[1].record()
        G = Z.T @ Z
        ev[2].record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            t_build.append(ev[0].elapsed_time(ev[1])); t_mm.append(ev[1].elapsed_time(ev[2]))
        del Z
    rec["yardstick_ms"] = {"torch_build_Z": statistics.median(t_build), "rocblas_dgemm": statistics.median(t_mm),
                           "build_plus_dgemm": statistics.median(t_build) + statistics.median(t_mm)}
    rec["yardstick_dgemm_tflops"] = flop / (rec["yardstick_ms"]["rocblas_dgemm"] * 1e-3) / 1e12
    Gd = torch.from_numpy(g["G"]).to(dev)
    rec["max_rel_diff_G_vs_torch"] = float(((Gd - G).abs().max() / G.abs().max()).item())
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
