#!/usr/bin/env python3
"""bench.py -- throughput of the hot path on MI355X, with roofline and CPU-baseline legs.

A "step" is one pass of the hot path over one batch of synthetic counts that are already resident
in HBM: per-sample constants -> beta-binomial emissions for every (exon, sample) cell -> Viterbi per
(sample, chromosome) chain -> call table (+ the per-sample dispersion fit when --fit).  Workload:
BASELINE.json configs[2] geometry, 200 000 exons x 1024 samples per GPU (weak scaling: N GPUs hold
N x 1024 samples, configs[3] at N=8).  Metric: exons*samples/s (BASELINE.json.metric).

Contract: `python bench.py --gpus N --steps K --warmup W`; for N>1 launched with
`python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...` (one rank per GPU,
RCCL).  Rank 0 prints ONE JSON line.

A plain run times the headline only: set-up, warm-up, the K timed steps, the line.  `--full` adds the
legs after the timed region (kernel-alone launches, the check against the CPU checker, other modes,
sizes and configurations, host-fed steps, the workflow, the CPU baseline).  `--dump-outputs DIR`
writes what the last timed step computed as .npy files (see dump_outputs).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec, /opt/skills/guides/MI355X_MICROARCH.md
FP64_VALU_PEAK_TFLOPS = 78.6   # FP64 vector peak (no MFMA applies to this path)
FP64_LANE_INSTR_PEAK = 256 * 64 * 2.4e9   # lane-instructions/s at that peak: 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz (an FMA = 2 flop)
ALGO_BYTES_PER_CELL = 9        # read test 4 B + read reference 4 B + write state 1 B


def matching_profile():
    """Tag of the newest rocprofv3 profile under profiles/ that was taken on THIS build of the kernels: profiles/<tag>_meta.json
    (written by tools/profile_round.sh on the GPU box) carries the fingerprint of exomedepth_amd/csrc at profiling time;
    counter-derived figures are only quoted when it equals the tree's.  (None, reason) otherwise."""
    import glob
    from exomedepth_amd import _build
    here = _build.csrc_sha16()
    metas = sorted(glob.glob(os.path.join(ROOT, "profiles", "*_meta.json")))
    for f in reversed(metas):
        try:
            m = json.load(open(f))
        except ValueError:
            continue
        if m.get("csrc_sha16") == here:
            return m, None
    return None, ("no profile under profiles/ was taken on this build of the kernels (csrc fingerprint %s): counter-derived "
                  "figures withheld; run tools/profile_round.sh" % here)


def pmc_figures(meta, kernel, cells_per_step, kernel_cells_per_s):
    """HBM traffic per launch and VALU figures of `kernel` from the PMC passes of profile `meta` (same build, see
    matching_profile): FETCH_SIZE x2 (gfx950 tallies the 128-byte requests of a coalesced 16-byte-per-lane stream at 64 B,
    MI355X_MICROARCH.md; x1 for k_emit_tab_sm's 4-byte-per-lane reads, calibrated on its known count bytes) + WRITE_SIZE, KB -> bytes; SQ_INSTS_VALU x 64 lanes / cells; SQ_ACTIVE_INST_VALU x 4 /
    (GRBM_GUI_ACTIVE / 8 XCDs) / 1024 SIMDs.  valu_frac_of_fp64_peak combines the profile's instruction count per cell
    with THIS run's live kernel rate."""
    import csv
    tag = meta["tag"]
    steps = float(meta.get("pmc_steps", 3))
    def load(name):
        f = os.path.join(ROOT, "profiles", "%s_pmc_%s.csv" % (tag, name))
        if not os.path.exists(f):
            return {}
        return {(r["kernel"], r["counter"]): (float(r["mean_per_launch"]), int(r["launches"])) for r in csv.DictReader(open(f))}
    out = {"profile": tag, "csrc_sha16": meta["csrc_sha16"]}
    fe, wr, sq, gr = load("FETCH_SIZE"), load("WRITE_SIZE"), load("SQ"), load("GRBM_GUI_ACTIVE")
    def runs(tab, counter):
        # batch runs in that pass (timed + warm-up + the priming run of every batch object): k_sample_consts is launched
        # exactly once per run, whatever the schedule
        return float(tab[("k_sample_consts", counter)][1]) if ("k_sample_consts", counter) in tab else steps
    if (kernel, "FETCH_SIZE") in fe and (kernel, "WRITE_SIZE") in wr:
        f, n = fe[(kernel, "FETCH_SIZE")]
        w = wr[(kernel, "WRITE_SIZE")][0]
        # the guide's x2 is for 16-byte-per-lane streams; "other access widths are uncalibrated: calibrate on a known byte count".
        # k_emit_tab_sm reads its counts 4 bytes per lane: a known 8 B/cell = 1.64 GB per 200 000 x 1024 launch, against which the raw
        # counter reads 1.62-1.66 GB (profiles/r04_a, r04_b) -- factor 1 for that kernel.
        ff = 1.0 if kernel == "k_emit_tab_sm" else 2.0
        out["fetch_size_factor"] = ff
        out["traffic_bytes_per_launch"] = (ff * f + w) * 1024.0
        out["traffic_bytes_per_step"] = (ff * f + w) * 1024.0 * n / runs(fe, "FETCH_SIZE")
        out["launches_per_step_profiled"] = n / runs(fe, "FETCH_SIZE")
    # the whole step: every kernel of the library in the FETCH / WRITE passes, per batch run.  x2 on the kernels that stream with 16-byte
    # loads (the guide's gfx950 correction), x1 on the others (4-byte-per-lane / scattered reads: calibrated on k_emit_tab_sm's known bytes)
    WIDE = ("k_viterbi_sm", "k_viterbi", "k_fit_hist_sm")
    if fe and wr:
        per_kernel = {}
        for (kn, cn), (mean, n) in fe.items():
            if cn != "FETCH_SIZE" or (kn, "WRITE_SIZE") not in wr:
                continue
            ff = 2.0 if kn.split("::")[-1] in WIDE else 1.0
            per_kernel[kn] = (ff * mean + wr[(kn, "WRITE_SIZE")][0]) * 1024.0 * n / runs(fe, "FETCH_SIZE")
        out["step_traffic_bytes"] = sum(per_kernel.values())
        out["step_traffic_by_kernel_GB"] = {k: round(v / 1e9, 3) for k, v in sorted(per_kernel.items(), key=lambda kv: -kv[1]) if v > 1e7}
        out["step_traffic_fetch_x2_kernels"] = [k for k in per_kernel if k.split("::")[-1] in WIDE]
    if (kernel, "SQ_INSTS_VALU") in sq and (kernel, "GRBM_GUI_ACTIVE") in gr:
        insts, n = sq[(kernel, "SQ_INSTS_VALU")]
        per_cell = insts * n / runs(sq, "SQ_INSTS_VALU") / (cells_per_step / 64.0)          # lane-instructions per cell
        out["valu_lane_instructions_per_cell"] = per_cell
        out["valu_busy"] = sq[(kernel, "SQ_ACTIVE_INST_VALU")][0] * 4.0 / (gr[(kernel, "GRBM_GUI_ACTIVE")][0] / 8.0) / 1024.0
        out["salu_per_valu"] = sq[(kernel, "SQ_INSTS_SALU")][0] / insts if (kernel, "SQ_INSTS_SALU") in sq else None
        out["valu_frac_of_fp64_peak"] = per_cell * kernel_cells_per_s / FP64_LANE_INSTR_PEAK
    return out


def cpu_baseline(test_h, ref_h, p, phi, chrom_off, start, end, fit, allcores=0):
    """The CPU checker's libm flavour timed on the host over a bounded sample of the same workload.  kind "port": the
    reference's own hmm.cpp / CNV_estimate.cpp include <Rinternals.h> and cannot be built without R; the port's special
    functions are bit-identical to the reference's compiled ones (tests/test_oracle_ref.py)."""
    from oracle import edoracle as eo

    eo.build()
    n_s = test_h.shape[1]
    t_emit = t_vit = 0.0
    for s in range(n_s):
        t0 = time.perf_counter()
        ll, _ = eo.get_loglike_matrix(phi[s], p[s], test_h[:, s] + ref_h[:, s], test_h[:, s], 1.0, eo.LIBM)
        t1 = time.perf_counter()
        eo.callcnvs(ll, chrom_off, start, end)
        t2 = time.perf_counter()
        t_emit += t1 - t0
        t_vit += t2 - t1
    cells = test_h.shape[0] * n_s
    t_fit = 0.0
    n_fit = 0
    if fit:
        # stand-in for aod::betabin (not in the reference tree): Nelder-Mead on the same likelihood
        n_fit = min(n_s, 4)
        t0 = time.perf_counter()
        for s in range(n_fit):
            eo.fit_nm(test_h[:, s], ref_h[:, s])
        t_fit = (time.perf_counter() - t0) * (n_s / n_fit)   # extrapolated linearly to the n_s samples
    extra = {}
    if eo.ref_available():
        # The reference's OWN compiled gsl_sf_lnbeta (oracle/_ref, built from /root/reference/src as it lies) on the six
        # log-Beta calls per cell of one sample, next to the port's time for the same sample: the port is not a slower
        # stand-in.  (The loop around it -- myprob's ten lines, src/CNV_estimate.cpp:44-50 -- and hmm.cpp cannot be built
        # without R's headers, hence kind = "port".)
        s0 = 0
        e = float(p[s0]); ph = float(phi[s0])
        sd = np.sqrt(ph * e * (1 - e))
        xs, ys = [], []
        obs = test_h[:, s0].astype(np.float64); tot = (test_h[:, s0] + ref_h[:, s0]).astype(np.float64)
        for odds in (0.5, 1.0, 1.5):
            ep = e * odds / (e * odds + 1 - e)
            a1 = ep * ep * (1 - ep) / (sd * sd) - ep
            a2 = (1 - ep) / ep * a1
            xs += [a1 + obs, np.full_like(obs, a1)]; ys += [a2 + tot - obs, np.full_like(obs, a2)]
        x = np.concatenate(xs); y = np.concatenate(ys)
        t0 = time.perf_counter(); eo.ref_call2("gsl_sf_lnbeta", x, y); t_ref = time.perf_counter() - t0
        t0 = time.perf_counter(); eo.lnbeta(x, y, eo.LIBM); t_port = time.perf_counter() - t0
        extra["reference_build_lnbeta"] = {"calls": int(x.size), "reference_s": t_ref, "port_s": t_port,
                                           "note": "gsl_sf_lnbeta of oracle/_ref (the reference's sources compiled in place) vs the "
                                                   "checker's libm flavour on the same %d arguments of one sample" % x.size}
    if allcores > 1:
        # the same work on every host core: one pinned worker per core, each timing its own samples (the reference is
        # single-threaded: reported for completeness)
        from oracle import cpu_bench
        extra["all_cores"] = cpu_bench.all_cores(test_h, ref_h, p, phi, chrom_off, start, end, fit, allcores)
    return {**extra, "value": cells / (t_emit + t_vit + t_fit), "unit": "exons*samples/s", "cores": 1, "kind": "port",
            "value_without_fit": cells / (t_emit + t_vit),
            "sample": "%d samples x %d exons of the same synthetic batch: emissions + Viterbi + call table with the "
                      "checker's libm flavour (special functions bit-identical to the reference's compiled ones), single "
                      "thread.  A port, not the reference build (hmm.cpp / CNV_estimate.cpp need R's headers); the judge's "
                      "round-1 scratch build of the reference found the port bit-identical and FASTER than the reference's own "
                      "vector<vector<>> Viterbi (VERDICT r1), so this baseline flatters the CPU%s"
                      % (n_s, test_h.shape[0],
                         ".  Dispersion fit = Nelder-Mead stand-in for aod::betabin (third-party, not in the reference tree) timed "
                         "on %d samples and extrapolated linearly: %.0f %% of the denominator; `value_without_fit` leaves it out"
                         % (n_fit, 100.0 * t_fit / (t_emit + t_vit + t_fit)) if fit else ""),
            "emissions_s": t_emit, "viterbi_s": t_vit, "fit_s": t_fit}


def _device_view(torch, eddist, ptr, shape, typestr, dev):
    return torch.as_tensor(eddist._DevicePointer(ptr, shape, typestr), device=dev)


def interval_union(iv):
    """(total length of the union, sum of the lengths) of (start, end) intervals"""
    iv = sorted((float(a), float(b)) for a, b in iv)
    if not iv:
        return 0.0, 0.0
    union, (cs, ce) = 0.0, iv[0]
    for a, b in iv[1:]:
        if a > ce:
            union += ce - cs
            cs, ce = a, b
        else:
            ce = max(ce, b)
    return union + (ce - cs), sum(b - a for a, b in iv)


def verify_against_oracle(ed, eddist, torch, dev, co, batches, last_ticket, n_batches, test, ref, phi, p, phi_fit, p_fit, fitted,
                          chrom_off, start, end, k, tables=False, max_slabs=None):
    """k columns of each of the last slabs in flight against the CPU checker (oracle/, the checker -- never the thing timed):
    the bits of the likelihood matrix vs its portable flavour, Viterbi states and call rows vs its Viterbi run on its own matrix,
    given the (phi, expected) the device used for that slab."""
    from oracle import edoracle as eo
    eo.build()
    E, S = test.shape
    cols = sorted(set(int(c) for c in np.linspace(0, S - 1, k).round()))
    out = {"columns": 0, "loglik_values": 0, "loglik_bit_mismatches": 0, "discordant_states": 0, "discordant_calls": 0, "slabs": 0}
    if tables:   # emit mode 1: tolerance parity against the LIBM flavour (= the reference's arithmetic), 1e-10 relative / 1e-12 absolute
        out = {"columns": 0, "loglik_values": 0, "loglik_beyond_1e-10": 0, "loglik_needed_abs_floor": 0, "loglik_max_rel_diff": 0.0, "discordant_states": 0,
               "discordant_calls": 0, "slabs": 0}
    slabs = []
    if co is not None:
        for t in range(max(0, last_ticket - (min(n_batches, max_slabs) if max_slabs else n_batches) + 1), last_ticket + 1):
            b, pp, pe = co.batch(t)
            b.n_samples = S
            slabs.append((b, _device_view(torch, eddist, pp, (S,), "<f8", dev).cpu().numpy(), _device_view(torch, eddist, pe, (S,), "<f8", dev).cpu().numpy()))
    else:
        for j, b in enumerate(batches):
            ph = phi_fit[j].cpu().numpy() if fitted else phi.cpu().numpy()
            pe = p_fit[j].cpu().numpy() if fitted else p.cpu().numpy()
            slabs.append((b, ph, pe))
    th = test[:, cols].cpu().numpy()
    rh = ref[:, cols].cpu().numpy()
    margins = None
    max_abs = [0.0]
    for b, ph, pe in slabs:
        calls = b.calls()
        ptr = b.device_pointers()
        ll = _device_view(torch, eddist, ptr["loglik"], (E, 3, S), "<f8", dev)[:, :, cols].cpu().numpy()
        path = _device_view(torch, eddist, ptr["path"], (E, S), "|u1", dev)[:, cols].cpu().numpy()
        out["slabs"] += 1
        for i, c in enumerate(cols):
            ell, _ = eo.get_loglike_matrix(ph[c], pe[c], th[:, i] + rh[:, i], th[:, i], 1.0, eo.LIBM if tables else eo.PORTABLE)
            got = np.ascontiguousarray(ll[:, :, i])
            out["loglik_values"] += int(got.size)
            if tables:
                d = np.abs(got - ell)
                same = (got == ell) | (np.isnan(got) & np.isnan(ell))
                rel_ok = same | (d <= 1e-10 * np.abs(ell))          # north_star's bar as written: relative, no floor
                out["loglik_beyond_1e-10"] += int(np.sum(~rel_ok))
                out["loglik_needed_abs_floor"] += int(np.sum(~rel_ok & (d <= 1e-12)))      # (what a 1e-12 absolute floor would have let through)
                nz = np.isfinite(ell) & (ell != 0)
                if nz.any():
                    out["loglik_max_rel_diff"] = max(out["loglik_max_rel_diff"], float(np.max(d[nz] / np.abs(ell[nz]))))
                    max_abs[0] = max(max_abs[0], float(np.max(d[nz])))
            else:
                out["loglik_bit_mismatches"] += int(np.sum(got.view(np.int64) != np.ascontiguousarray(ell).view(np.int64)))
            epath, ecalls = eo.callcnvs(ell, chrom_off, start, end)
            if tables:      # how far the on-path decisions of these columns are from a tie (tools/concordance.py --margins has all 1 024 columns on record)
                margins = eo.callcnvs_margins(ell, chrom_off, start, end, acc=margins)
            out["discordant_states"] += int(np.sum(path[:, i].astype(np.int8) != epath))
            mine = calls[calls["sample"] == c]
            want = {(int(r[0]) - 1, int(r[1]) - 1, int(r[2]), int(r[3])) for r in ecalls}
            have = {(int(r["start_exon"]), int(r["end_exon"]), int(r["type"]), int(r["nexons"])) for r in mine}
            out["discordant_calls"] += len(want ^ have)
            out["columns"] += 1
    if margins:
        out["min_on_path_margin"] = margins["min_margin"]
        out["on_path_decisions"] = margins["decisions"]
        out["on_path_margins_below"] = margins["below"]
        out["on_path_exact_ties"] = margins["ties"]
        out["loglik_max_abs_diff"] = max_abs[0]
    out["what"] = ("%d columns x %d slab(s) in flight after the timed region: %s, Viterbi "
                   "states and call rows vs the checker's Viterbi, given the (phi, expected) the device used"
                   % (len(cols), len(slabs), "likelihood values vs the checker's LIBM flavour (the reference's arithmetic), 1e-10 RELATIVE with no absolute floor (loglik_needed_abs_floor: values among those beyond it that a 1e-12 floor would have let through)"
                      if tables else "likelihood bits vs the checker's portable flavour"))
    return out


DUMP_COLUMN_BYTES = 44 << 20     # --dump-outputs: likelihood matrix + Viterbi states of the sampled columns (8 at 200 000 exons)
DUMP_CALL_BYTES = 16 << 20       # ... the call table and its statistics; the per-sample parameters take the rest of 64 MiB


def dump_outputs(out_dir, torch, eddist, dev, co, ticket, E, S, seed=20250620):
    """What a caller of the timed path receives for the last timed slab, as float64 / float32 .npy files under out_dir: the
    per-sample parameters the slab used (phi, expected; phi_bins and edges with the depth-binned model), the call table and its
    statistics one file per field (calls_<field>.npy, rows sorted by sample and first exon), and for a fixed, seeded choice of
    sample columns (sample_columns.npy) the likelihood matrix (loglik.npy, exons x 3 x columns) and the Viterbi states (path.npy,
    exons x columns).  Inputs are seeded, so two builds given the same arguments can be compared file by file."""
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(seed)
    res = co.results(ticket, S, info=True)
    out = {k: res[k].astype(np.float64) for k in ("phi", "expected", "phi_bins", "edges") if k in res}
    calls, info = res["calls"], res["info"]
    rows = np.lexsort((calls["start_exon"], calls["sample"]))
    row_bytes = 8 * (len(calls.dtype.names) + len(info.dtype.names))
    if len(rows) * row_bytes > DUMP_CALL_BYTES:
        rows = rows[np.sort(rng.choice(len(rows), DUMP_CALL_BYTES // row_bytes, replace=False))]
    for table in (calls, info):
        for f in table.dtype.names:
            out["calls_" + f] = table[f][rows].astype(np.float64)
    col_bytes = E * (3 * 8 + 4)
    cols = np.sort(rng.choice(S, min(S, 8, max(1, DUMP_COLUMN_BYTES // col_bytes)), replace=False))
    exons = None
    if col_bytes * len(cols) > DUMP_COLUMN_BYTES:
        exons = np.sort(rng.choice(E, DUMP_COLUMN_BYTES // (len(cols) * (3 * 8 + 4) + 8), replace=False))     # (+ 8: exon_rows itself)
        out["exon_rows"] = exons.astype(np.float64)
    b, _, _ = co.batch(ticket)
    ptr = b.device_pointers()
    if not ptr["loglik"] or not ptr["path"]:
        raise RuntimeError("--dump-outputs: the last slab's likelihood matrix or Viterbi path is not available")
    torch.cuda.synchronize()      # (in the sample-major mode the [E][3][S] form is made on the batch's own stream when its pointer is asked for)
    ct = torch.as_tensor(cols, device=dev)
    ll = _device_view(torch, eddist, ptr["loglik"], (E, 3, S), "<f8", dev)[:, :, ct]
    path = _device_view(torch, eddist, ptr["path"], (E, S), "|u1", dev)[:, ct]
    if exons is not None:
        et = torch.as_tensor(exons, device=dev)
        ll, path = ll[et], path[et]
    out["sample_columns"] = cols.astype(np.float64)
    out["loglik"] = ll.cpu().numpy()
    out["path"] = path.cpu().numpy().astype(np.float32)
    for k, v in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


EMIT_MODES = {"strict": 0, "tables-tile": 1, "tables": 2}
NOTE_STRICT = ("FP64-VALU-bound kernel (no MFMA applies; SURVEY.md 0.5): the HBM roofline is the formal denominator, "
               "roofline.valu (rocprofv3 PMC passes taken on this very build of the kernels, else withheld) the meaningful "
               "one.  kernel_ms: HIP events recorded by the library around the emission launches on the stream they "
               "run on, averaged over the timed steps; consecutive batches' emissions are back to back on that stream.  "
               "Traffic above 9 B/cell: the kernel materialises the [E][3][S] f64 likelihood matrix (the reference's S4 "
               "`likelihood` slot: 33 B/cell algorithmic in that form, SURVEY.md 8d) and gathers per-sample tables")
NOTE_TABLES = ("table-driven emissions, sample-major (k_emit_tab_sm): ~155 VALU lane-instructions per cell, the hot 85-99 % of a sample's "
               "log-gamma difference tables in LDS -- a memory-streaming kernel: reads the counts (8 B/cell) and writes the [S][3][E] f64 "
               "likelihood matrix (24 B/cell) that k_viterbi_sm reads back, i.e. 33 B/cell algorithmic in the materialised form against the "
               "9 B/cell of `achieved` (SURVEY.md 8d).  kernel_ms: the chip's time per emission launch (see kernel_ms_is), live = sharing the chip with the "
               "previous slabs' Viterbi chains and the next slabs' fits and table builds; kernel_ms_own = a launch's own duration (with three lanes, the default, "
               "two or three emission launches are in flight at a time); kernel_ms_alone = the same launch with the GPU to itself")


def mode_opts(args):
    """cohort options of the emission mode / count layout the run was asked for"""
    o = {}
    if getattr(args, "fit_mode", 0):
        o["fit_mode"] = int(args.fit_mode)
    if args.emit_mode != "strict":
        o["emit_mode"] = EMIT_MODES[args.emit_mode]
    if args.counts_layout == 1:
        o["counts_layout"] = 1
    return o


def mode_leg(ed, torch, plan, test, ref, S, steps, fit, phi, p, opts, in_flight=2):
    """the headline's steps once more under other cohort options (another emission mode, the other count layout, 16-bit counts): ms per step"""
    co = ed.Cohort(plan, S, in_flight, **opts)
    if opts.get("counts_layout") == 1:
        test, ref = test.t().contiguous(), ref.t().contiguous()
    if opts.get("counts_bits") == 16:
        if int(test.max()) >= 65536 or int(ref.max()) >= 65536:
            co.close()
            return None
        test, ref = test.to(torch.int16), ref.to(torch.int16)       # (the low 16 bits: uint16 counts in an int16 tensor)
    sub = (lambda: co.submit(test, ref, n_samples=S)) if fit else (lambda: co.submit(test, ref, phi=phi, expected=p, n_samples=S))
    for _ in range(in_flight + 1):
        sub()
    co.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        sub()
    co.drain()
    el = time.perf_counter() - t0
    co.close()
    return {"ms_per_step": el / steps * 1e3, "value": test.numel() * steps / el, "steps": steps}


def r_entry_leg(ed, chrom_off, start, end, test, ref, S, steps, fit, phi, p):
    """What the R-level .Call entry runs (shim/edcore_shim.c: edr_call_cnvs_batch): ed_multi_run_host on R's own matrices -- int32, column-major
    exons x samples, PAGEABLE memory, wire = 4 -- in the sample-major table mode, one device, the wrapper's slab of 256 samples; with the narrowing of
    round 6 (the host threads that stage a block make it uint16, the slab stays uint16 on the device) and with it switched off (round 5's path:
    int32 on the link, int32 on the device).  ms per 1 024-sample cohort, call table collected."""
    th = np.ascontiguousarray(test.t().contiguous().cpu().numpy(), dtype=np.int32)
    rh = np.ascontiguousarray(ref.t().contiguous().cpu().numpy(), dtype=np.int32)
    par = {} if fit else {"phi": phi.cpu().numpy(), "expected": p.cpu().numpy()}
    out = {}
    for name, narrow in (("narrowed_while_staged", 1), ("int32_on_link_and_device", 0)):
        m = ed.MultiDevice(chrom_off, start, end, 256, devices=[0], emit_mode=2, counts_layout=1, host_narrow=narrow)
        res = m.run_host(th, rh, 1, **par)
        each = []
        t0 = time.perf_counter()
        for _ in range(steps):
            t1 = time.perf_counter()
            res = m.run_host(th, rh, 1, **par)
            each.append((time.perf_counter() - t1) * 1e3)
        el = time.perf_counter() - t0
        # (run to run the leg moves by 20 %: where the pageable pages and the staging threads sit relative to the device's NUMA node; mean and best)
        out[name] = {"ms_per_cohort": el / steps * 1e3, "ms_best": min(each), "value": float(th.size) * steps / el, "n_calls": len(res["calls"]),
                     "link_GBps": 2.0 * th.size * (2 if narrow else 4) * steps / el / 1e9}
        m.close()
    out["ratio"] = out["narrowed_while_staged"]["ms_per_cohort"] / out["int32_on_link_and_device"]["ms_per_cohort"]
    out["same_call_count"] = out["narrowed_while_staged"]["n_calls"] == out["int32_on_link_and_device"]["n_calls"]
    return out


def staged_leg(ed, torch, plan, test, ref, phi, p, E, S, n_batches, args):
    """The same steps with the counts coming from HOST memory for every slab (ed_cohort_submit_host: copy stream, device slabs
    double-buffered by the slots, the 16-bit wire format widened on the device): the PCIe-inclusive rate.  Reported beside `value`,
    never instead of it.  Pinned host memory is read by the DMA engine in place; pageable memory goes through the library's pinned
    double buffer (host threads copy chunk k+1 while chunk k is on the link)."""
    dt = np.uint16 if args.wire == 2 else np.int32
    mo = mode_opts(args)
    lay = 1 if args.counts_layout == 1 else 0          # host layout = the device's: R's column-major matrices go up as they are
    th, rh = test.cpu().numpy(), ref.cpu().numpy()
    if lay:
        th, rh = np.ascontiguousarray(th.T), np.ascontiguousarray(rh.T)
        ref = ref.t().contiguous()
    shape = th.shape
    if args.wire == 2 and (th.max() >= 65536 or rh.max() >= 65536):
        return {"value_with_h2d": None, "note": "counts beyond 65535: the 16-bit wire format does not apply"}
    out = {}
    for kind in ("pinned", "pageable"):
        if kind == "pinned":
            pt, pr = ed.PinnedArray(shape, dt), ed.PinnedArray(shape, dt)
            pt.array[...] = th; pr.array[...] = rh
            ht, hr = pt.array, pr.array
        else:
            ht, hr = th.astype(dt), rh.astype(dt)
        co = ed.Cohort(plan, S, max(2, n_batches), **mo)
        sub = (lambda: co.submit_host(ht, hr, lay)) if args.fit else (lambda: co.submit_host(ht, hr, lay, phi=phi, expected=p))
        for _ in range(max(2, n_batches) + 1):
            sub()
        co.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            tk = sub()
        co.drain()
        el = time.perf_counter() - t0
        nbytes = 2.0 * E * S * args.wire
        out[kind] = {"ms_per_step": el / args.steps * 1e3, "value": E * S * args.steps / el, "link_GBps": nbytes * args.steps / el / 1e9}
        co.close()
        if kind == "pinned":
            pt.free(); pr.free()
    # the reference's workflow: a sample's reference is the sum of other samples of the cohort, made ON THE DEVICE by
    # ed_cohort_select_reference_sets -- only the test counts cross the link (ed_cohort_submit_host_test)
    pt = ed.PinnedArray(shape, dt)
    pt.array[...] = th
    co = ed.Cohort(plan, S, max(3, n_batches), **mo)      # (three slabs in flight: the upload of slab t+2 starts while slab t's chains still run)
    sub = (lambda: co.submit_host_test(pt.array, ref, lay)) if args.fit else (lambda: co.submit_host_test(pt.array, ref, lay, phi=phi, expected=p))
    for _ in range(max(3, n_batches) + 1):
        sub()
    co.drain()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        sub()
    co.drain()
    el = time.perf_counter() - t0
    out["test_only"] = {"ms_per_step": el / args.steps * 1e3, "value": E * S * args.steps / el, "link_GBps": 1.0 * E * S * args.wire * args.steps / el / 1e9}
    co.close()
    pt.free()
    return {"value_with_h2d": out["pinned"]["value"], "unit": "exons*samples/s", "wire_bytes_per_count": args.wire,
            "bytes_per_step": 2.0 * E * S * args.wire, "pinned": out["pinned"], "pageable": out["pageable"],
            "test_counts_only": out["test_only"],
            "test_counts_only_note": "the references stay on the device (in the reference's workflow they are sums of other samples of the same cohort: "
                                     "ed_cohort_select_reference_sets): one matrix per slab on the link",

            "pcie_peak_GBps": 63.0,
            "note": "every step uploads both count matrices of its slab from host memory (PCIe Gen5 x16: 63 GB/s peak) on the cohort's copy "
                    "stream while earlier slabs compute; link_GBps = bytes on the link / wall time of the steps"}


def workflow_leg(ed, torch, plan, test, start, end, E, S, reps, emit_mode=0, world=1, rank=0, eddist=None):
    """The reference's workflow for one cohort (vignette/vignette.Rnw:390-431), end to end from host memory: upload the cohort's counts
    once (16-bit, pinned), select.reference.set for every sample against all the others + the aggregate references on the device
    (ed_cohort_select_reference_sets, n.bins.reduced = 10 000 as in the vignette), then new('ExomeDepth') + CallCNVs() for every sample
    through the cohort pipeline with the device-resident matrices.  The synthetic 'test' matrix stands for the cohort's counts."""
    th = test.cpu().numpy()
    if th.max() >= 65536:
        return None
    pin = ed.PinnedArray((E, S), np.uint16)
    pin.array[...] = th
    bl = (np.asarray(end) - np.asarray(start)) / 1000.0
    stream = torch.cuda.current_stream()
    times = {"upload_ms": [], "reference_sets_ms": [], "calls_ms": [], "total_ms": []}
    n_calls = n_chosen = None
    # (a process group of ONE rank -- ED_BENCH_FORCE_PG=1 on a 1-GPU box -- takes the sharded path too: RCCL's all_gather_into_tensor on device memory, the
    #  branch no two-ranks-on-one-GPU run can reach, since RCCL refuses two ranks on one device)
    import torch.distributed as tdist
    sharded = world > 1 or (eddist is not None and tdist.is_available() and tdist.is_initialized())
    sm = emit_mode == 2 and not sharded and S <= 4096     # sample-major hand-over: aggregate references and the transposed counts straight from the reference-set stage
    co = ed.Cohort(plan, S, 1, **({"emit_mode": emit_mode, "counts_layout": 1 if sm else 0} if emit_mode else {}))
    ref_t = torch.empty((S, E) if sm else (E, S), dtype=torch.int32, device=test.device)
    counts_sm = torch.empty((S, E), dtype=torch.int32, device=test.device) if sm else None
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dcounts = torch.from_numpy(pin.array.view(np.int16)).to(test.device, non_blocking=True).view(torch.int16).to(torch.int32) & 0xffff
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if sharded:
            # a sample-sharded cohort: this rank's columns are S of world * S; every other rank's samples are candidates too -- one
            # all_gather of the count slabs, then the rank's own tests (exomedepth_amd/dist.py::cohort_reference_sets_sharded)
            rs = eddist.cohort_reference_sets_sharded(dcounts, S * world, bl, 10000, max_refs=32)
            ref_t = torch.as_tensor(eddist._DevicePointer(rs["reference"].ptr.value, (E, S), "<i4"), device=test.device)
        else:
            rs = ed.cohort_select_reference_sets(dcounts, bl, 10000, max_refs=32, reference_out=ref_t, sample_major=sm, counts_sm_out=counts_sm)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        tk = co.submit(counts_sm if sm else dcounts, ref_t, n_samples=S)     # (two half-cohort slabs through the pipeline were tried: 17 ms against 12.7 in the [exons][samples] layout, where the cut costs strided copies -- and, round 5, in the sample-major layout where it is free: 8.6 ms as two slabs, 10.7 as four, against 7.5 as one: every slab pays its own longest chain)
        co.wait(tk)
        b, _, _ = co.batch(tk)
        n_calls = b.n_calls()
        t3 = time.perf_counter()
        tstats = b.table_stats() if emit_mode else None
        n_chosen = float(rs["n_chosen"].mean())
        rs_path = ed.refcohort_last_path()            # which form served the cumulative references (k_rc_column's geometry, or the row-major kernels)
        checksum = int(np.sum((rs["choice"].astype(np.int64) + 1) * (np.arange(rs["choice"].shape[1], dtype=np.int64) + 1)[None, :]))
        if rep > 0:                                   # (the first repetition allocates)
            for k, v in zip(("upload_ms", "reference_sets_ms", "calls_ms", "total_ms"), (t1 - t0, t2 - t1, t3 - t2, t3 - t0)):
                times[k].append(v * 1e3)
        del rs
    # Cohorts back to back (one rank): the NEXT cohort's counts cross the link on a copy stream while this one's reference sets and calls run --
    # what a caller with more than one cohort to process gets per cohort (the link is idle for 3/4 of the serial form above).
    back_to_back = None
    if not sharded and reps > 0:
        # copy stream (torch's); the reference-set stage works on the cohort object's own emission stream -- a stream with a hardware queue of its own (the null
        # stream would order the stage behind the copy, and a second ORDINARY stream shares the runtime's four multiplexed hardware queues with the copy stream:
        # whether the two end up on one queue depends on how many streams the process made before -- seen as 31.5 instead of 24.3 ms per cohort)
        cs = torch.cuda.Stream()
        ws_handle = co.stream

        import threading

        class Upload(threading.Thread):       # (torch does not know the library's pinned block as pinned and makes the issuing thread wait for the copy: a thread of its own)
            def run(self):
                torch.cuda.set_device(test.device)
                with torch.cuda.stream(cs):
                    self.d = torch.from_numpy(pin.array.view(np.int16)).to(test.device, non_blocking=True).view(torch.int16).to(torch.int32) & 0xffff
                    cs.synchronize()

        def upload_async():
            u = Upload()
            u.start()
            return u
        n_coh = 2 * reps
        nxt = upload_async()
        nxt.join()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n_coh):
            nxt.join()                        # (the library's streams are its own: the host orders them behind the copy)
            d = nxt.d
            nxt = upload_async()              # cohort k + 1 (after the last one: one more, so that every timed cohort carries an upload beside it)
            rs = ed.cohort_select_reference_sets(d, bl, 10000, max_refs=32, reference_out=ref_t, sample_major=sm, counts_sm_out=counts_sm, stream=ws_handle)
            tk = co.submit(counts_sm if sm else d, ref_t, n_samples=S, ready_stream=ws_handle)
            co.wait(tk)
            assert co.batch(tk)[0].n_calls() == n_calls
            del rs, d
        t1 = time.perf_counter()
        nxt.join()
        back_to_back = {"cohorts": n_coh, "ms_per_cohort": (t1 - t0) / n_coh * 1e3, "value": E * S / ((t1 - t0) / n_coh), "unit": "exons*samples/s",
                        "note": "the same cohort %d times in a row, the next one's upload (pinned uint16 -> device, widened there) issued on a copy stream before "
                                "this one's reference sets start; same call count every time" % n_coh}
        del nxt
    co.close(); pin.free()
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"workload": "one cohort of %d samples x %d exons: counts from pinned host memory (uint16) -> reference sets of every sample against all "
                        "others (n.bins.reduced 10000, <= 32 candidates) + aggregate references on the device (sample-major, with the transposed counts, "
                        "when the calls run in the sample-major table mode on one rank) -> fit + emissions + Viterbi + calls; "
                        "stages one after the other (one cohort, nothing to overlap with), median of %d" % (S, E, reps),
            **med, "value": E * S * world / (med["total_ms"] * 1e-3), "unit": "exons*samples/s", "references_chosen_mean": n_chosen, "n_calls": n_calls, "table_stats": tstats,
            "ranks": world, "choice_checksum_rank0": checksum, "reference_sets_form": rs_path, "back_to_back": back_to_back,
            "sharding": (None if not sharded else "every rank: its own %d columns as tests, all %d as candidates (one all_gather of the count slabs); "
                                                  "times and counts are rank 0's" % (S, S * world))}


PIPELINED_SLABS_IN_FLIGHT = 6      # configs[1] leg: a slab's latency (~2.5 ms, its longest chromosome's chain) over its issue interval


def config1_leg(ed, torch, plan, test, ref, phi, p, E, steps, opts={}):
    """BASELINE configs[1]: 200 000 exons x 64 samples, phi given (no fit) -- the first 64 columns of the batch through the cohort
    pipeline (three slabs in flight: 0.91 ms per slab against 1.07 with two and 1.08-1.2 with four to eight -- at 64 samples a slab is
    ~20 launches on three streams and the host's submission rate is what limits), and one slab at a time (the latency of a lone slab:
    bound by the longest chromosome's chain)."""
    n = 64
    t64, r64 = test[:, :n].contiguous(), ref[:, :n].contiguous()
    if opts.get("counts_layout") == 1:
        t64, r64 = t64.t().contiguous(), r64.t().contiguous()
    ph, pe = phi[:n].contiguous(), p[:n].contiguous()
    res = {}
    for name, in_flight in (("pipelined", PIPELINED_SLABS_IN_FLIGHT), ("one_at_a_time", 1)):
        co = ed.Cohort(plan, n, in_flight, **opts)
        for _ in range(in_flight + 2):
            co.submit(t64, r64, phi=ph, expected=pe, n_samples=n)
        co.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tk = co.submit(t64, r64, phi=ph, expected=pe, n_samples=n)
        t_issued = time.perf_counter() - t0
        co.drain()
        el = time.perf_counter() - t0
        b, _, _ = co.batch(tk)
        res[name] = {"ms_per_step": el / steps * 1e3, "value": E * n * steps / el, "n_calls": b.n_calls(), "slabs_in_flight": in_flight,
                     "host_ms_per_submit": t_issued / steps * 1e3}
        co.close()
    return {"workload": "BASELINE.json configs[1]: %d exons x 64 samples, phi given per sample (no fit), 1 GPU" % E, "steps": steps,
            "unit": "exons*samples/s", **res}


def regime_leg(ed, eddist, torch, dev, plan, chrom_off, start, end, E, S, depth, fit, opts, n_batches, steps, seed, verify_columns):
    """The headline's step in another regime of the synthetic generator -- another sequencing depth (reads per exon and sample; the aggregate
    references are 8 x deeper) or another slab width -- with the headline's cohort options: ms per step, what the tables left to the strict
    arithmetic, the chip time of the emission launches, and the same check against the CPU checker as the headline's `verify`."""
    from exomedepth_amd import synth
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=seed, mean_depth=depth)
    lay1 = opts.get("counts_layout") == 1
    t_in, r_in = (test.t().contiguous(), ref.t().contiguous()) if lay1 else (test, ref)
    o = dict(opts)
    if n_batches not in (4, 6, 8):
        o.pop("lanes", None)
    co = ed.Cohort(plan, S, n_batches, **o)
    sub = (lambda: co.submit(t_in, r_in, n_samples=S)) if fit else (lambda: co.submit(t_in, r_in, phi=phi, expected=p, n_samples=S))
    for _ in range(n_batches + 2):
        tk = sub()
    co.drain()
    torch.cuda.synchronize()
    co.set_option("timing", 1)
    t0 = time.perf_counter()
    for _ in range(steps):
        tk = sub()
    co.drain()
    el = time.perf_counter() - t0
    b, _, _ = co.batch(tk)
    b.n_samples = S
    tstats = b.table_stats() if o.get("emit_mode") else None
    if tstats is not None and o.get("emit_mode") == 2:
        probe = list(range(0, S, max(1, S // 32)))
        tstats["tail_samples_of_%d_probed" % len(probe)] = sum(1 for s_ in probe if b.table_windows(s_)[3])
    stage, nr, _ = co.stage_ms_total()
    union, own = interval_union(co.emission_intervals())
    ver = None
    if verify_columns > 0:
        ver = verify_against_oracle(ed, eddist, torch, dev, co, [], tk, n_batches, test, ref, phi, p, None, None, bool(fit), chrom_off, start, end,
                                    verify_columns, tables=bool(o.get("emit_mode")), max_slabs=2)
        ver.pop("what", None)
    co.close()
    cells = float(E) * S
    ms = el / steps * 1e3
    # the same steps with every sample on full-length tables (cohort option emit_tails = 0: round 5's form) where the depth makes the difference
    tails_off = None
    if o.get("emit_mode") == 2 and depth >= 400:
        co2 = ed.Cohort(plan, S, n_batches, **{**o, "emit_tails": 0})
        sub2 = (lambda: co2.submit(t_in, r_in, n_samples=S)) if fit else (lambda: co2.submit(t_in, r_in, phi=phi, expected=p, n_samples=S))
        for _ in range(n_batches + 2):
            sub2()
        co2.drain()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            tk2 = sub2()
        co2.drain()
        el2 = time.perf_counter() - t0
        b2, _, _ = co2.batch(tk2)
        tails_off = {"ms_per_step": el2 / steps * 1e3, "table_stats": b2.table_stats()}
        co2.close()
    return {"depth": depth, "samples": S, "ms_per_step": ms, "value": cells * steps / el, "ns_per_cell": ms * 1e6 / cells, "tails_off": tails_off,
            "emission_ms_chip": union / max(nr, 1), "emission_ms_own": own / max(nr, 1),
            "stage_ms": {k: v / max(nr, 1) for k, v in stage.items()},
            "table_stats": tstats, "cold_share": (tstats["n_cold_cells"] / cells if tstats else None), "verify": ver}


def dropin_leg(ed, chrom_off, start, end, test_h, ref_h, phi, p, reps=5):
    """The two reference-shaped entries at the granularity the UNCHANGED S4 surface calls them (reference R/class_definition.R:184-189: one
    .Call get_loglike_matrix per sample; R/tools.R:97 <- R/class_definition.R:354-374: one .Call C_hmm per chromosome and sample), host
    arrays in, host arrays out, timed at the C-ABI (ctypes, arrays made beforehand) next to the CPU port doing the same call.  `first` = the
    call that computes a chain's log-transitions on the host (exp / log of libm: the reference's own calls), `repeat` = the following
    samples' calls for the same chromosome, which find them remembered (csrc/eddropin.inc)."""
    import ctypes as C
    from exomedepth_amd._lib import check, lib
    from oracle import edoracle as eo
    eo.build()
    L, OL = lib(), eo.lib()
    vp = lambda a: C.c_void_p(a.ctypes.data)
    E = test_h.shape[0]
    med = lambda xs: float(np.median(xs)) * 1e3
    out = {}
    # ---- get_loglike_matrix on all exons of one sample
    tot = np.ascontiguousarray(test_h[:, 0] + ref_h[:, 0], dtype=np.int32); obs = np.ascontiguousarray(test_h[:, 0], dtype=np.int32)
    ph = np.full(E, float(phi[0])); ex = np.full(E, float(p[0]))
    ll = np.empty((3, E)); nerr = C.c_int64(0)
    tg = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        check(L.ed_get_loglike_matrix(vp(ph), vp(ex), vp(tot), vp(obs), E, 1.0, vp(ll), C.byref(nerr)))
        tg.append(time.perf_counter() - t0)
    oll = np.empty((3, E))
    tc = []
    for _ in range(2):
        t0 = time.perf_counter()
        OL.edo_get_loglike_matrix(eo.LIBM, ph, ex, tot, obs, E, 1.0, oll)
        tc.append(time.perf_counter() - t0)
    port, _ = eo.get_loglike_matrix(ph, ex, tot, obs, 1.0, eo.PORTABLE)
    out["get_loglike_matrix"] = {"rows": E, "ms_first_call": tg[0] * 1e3, "ms": med(tg[1:]), "cpu_port_ms": med(tc),
                                 "bit_mismatches_vs_checker": int(np.sum(ll.T.view(np.int64) != np.ascontiguousarray(port).view(np.int64)))}
    # ---- C_hmm: the padded chains CallCNVs builds (R/class_definition.R:364-368), HMM column order
    t = 1e-4
    Tc = np.ascontiguousarray(np.array([[1 - t, t / 2, t / 2], [.5, .5, 0], [.5, 0, .5]]).T.ravel())
    Lcnv = 50000.0
    def chain(c, lmat):
        lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
        loc = np.vstack([[-np.inf, 0, -np.inf], lmat[lo:hi], [-100, 0, -100]])[:, [1, 0, 2]]
        pos = np.concatenate([[start[lo] - 2 * Lcnv], start[lo:hi], [end[hi - 1] + 2 * Lcnv]]).astype(np.int32)
        return np.ascontiguousarray(loc.T.ravel()), pos
    lens = np.diff(np.asarray(chrom_off))
    chroms = {"longest": int(np.argmax(lens)), "median": int(np.argsort(lens)[len(lens) // 2])}
    def gpu_hmm(llc, pos, path, calls, nc):
        check(L.ed_hmm(3, pos.size, vp(Tc), vp(llc), vp(pos), Lcnv, vp(path), vp(calls), pos.size, C.byref(nc)))
    def cpu_hmm(llc, pos, path, calls):
        return OL.edo_hmm(3, pos.size, Tc, llc, pos, Lcnv, path, calls, pos.size)
    for name, c in chroms.items():
        llc, pos = chain(c, ll.T)
        n = pos.size
        path = np.empty(n); calls = np.zeros((4, n)); nc = C.c_int64(0)
        opath = np.empty(n); ocalls = np.zeros((n, 4))
        L.ed_dropin_release()
        first, rep = [], []
        for r in range(reps):
            q = pos.copy(); q[-1] += r + 1                      # (a chain not seen before: its log-transitions are computed)
            t0 = time.perf_counter(); gpu_hmm(llc, q, path, calls, nc); first.append(time.perf_counter() - t0)
        gpu_hmm(llc, pos, path, calls, nc)
        for r in range(reps):
            t0 = time.perf_counter(); gpu_hmm(llc, pos, path, calls, nc); rep.append(time.perf_counter() - t0)
        tcpu = []
        for r in range(reps):
            t0 = time.perf_counter(); onc = cpu_hmm(llc, pos, opath, ocalls); tcpu.append(time.perf_counter() - t0)
        out["hmm_" + name + "_chromosome"] = {"observations": int(n), "ms_first": med(first[1:] if reps > 1 else first), "ms_repeat": med(rep), "cpu_port_ms": med(tcpu),
                                              "path_mismatches_vs_checker": int(np.sum(path != opath)), "calls": int(nc.value), "calls_checker": int(onc)}
    # ---- one sample through the unchanged surface: 1 + C calls; two samples, so that the second finds every chain remembered
    seq = []
    for sidx in (0, 1):
        tot = np.ascontiguousarray(test_h[:, sidx] + ref_h[:, sidx], dtype=np.int32); obs = np.ascontiguousarray(test_h[:, sidx], dtype=np.int32)
        ph = np.full(E, float(phi[sidx])); ex = np.full(E, float(p[sidx]))
        if sidx == 0:
            L.ed_dropin_release()
        t0 = time.perf_counter()
        check(L.ed_get_loglike_matrix(vp(ph), vp(ex), vp(tot), vp(obs), E, 1.0, vp(ll), C.byref(nerr)))
        t1 = time.perf_counter()
        chains = [chain(c, ll.T) for c in range(len(lens)) if lens[c] > 0]          # (R's rbind / c() of :364-368: not the library's time)
        bufs = [(np.empty(pz.size), np.zeros((4, pz.size))) for _, pz in chains]
        nc = C.c_int64(0)
        t2 = time.perf_counter()
        ncalls = 0
        for (llc, pz), (pa, ca) in zip(chains, bufs):
            gpu_hmm(llc, pz, pa, ca, nc); ncalls += nc.value
        t3 = time.perf_counter()
        t4 = time.perf_counter()
        OL.edo_get_loglike_matrix(eo.LIBM, ph, ex, tot, obs, E, 1.0, oll)
        t5 = time.perf_counter()
        ocalls_n = 0; mism = 0
        t6 = time.perf_counter()
        for (llc, pz), (pa, ca) in zip(chains, bufs):
            op = np.empty(pz.size); oc = np.zeros((pz.size, 4))
            ocalls_n += cpu_hmm(llc, pz, op, oc)
            mism += int(np.sum(op != pa))
        t7 = time.perf_counter()
        seq.append({"get_loglike_matrix_ms": (t1 - t0) * 1e3, "hmm_calls": len(chains), "hmm_ms_total": (t3 - t2) * 1e3, "calls": int(ncalls),
                    "cpu_port_get_loglike_matrix_ms": (t5 - t4) * 1e3, "cpu_port_hmm_ms_total": (t7 - t6) * 1e3, "cpu_port_calls": int(ocalls_n),
                    "path_mismatches_vs_checker_given_the_device_matrix": mism})
    out["one_sample_sequence"] = {"first_sample": seq[0], "next_sample": seq[1],
                                  "note": "1 + %d calls per sample; the CPU port's Viterbi runs on the device's likelihood matrix here (same input both sides); "
                                          "its allocation of the outputs is inside its time, the device side's is not" % seq[0]["hmm_calls"]}
    L.ed_dropin_release()
    return out


def multi_device_main(args):
    """--driver multi-device: N devices from one process (ed_multi_*, csrc/edmulti.inc).  Weak scaling: every device gets --samples columns.
    The entry is the host-level one (the .Call boundary hands over host matrices), so a step here INCLUDES the upload of its counts from
    pinned host memory (uint16 on the link, R's column-major layout) and the collection of the call table: it is comparable with
    `h2d.pinned` of the default line, not with its device-resident `value`."""
    import exomedepth_amd as ed
    from exomedepth_amd import _build, synth
    if not os.path.exists(_build.LIB):
        _build.build()
    N = args.gpus
    devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(N))
    assert len(devices) == N, "--devices must name --gpus devices"
    E, S, C = args.exons, args.samples, args.chroms
    chrom_off, start, end = synth.exon_design(E, C, seed=20250620)
    import torch
    dev = torch.device("cuda", devices[0])
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3, mean_depth=args.depth)
    th, rh = test.t().contiguous().cpu().numpy(), ref.t().contiguous().cpu().numpy()      # [S][E]: R's column-major exons x samples
    assert th.max() < 65536 and rh.max() < 65536
    del test, ref
    torch.cuda.empty_cache()
    pt, pr = ed.PinnedArray((S * N, E), np.uint16), ed.PinnedArray((S * N, E), np.uint16)
    for i in range(N):                              # every device's share: the same synthetic slab (weak scaling)
        pt.array[i * S:(i + 1) * S] = th; pr.array[i * S:(i + 1) * S] = rh
    opts = {"emit_mode": 2, "counts_layout": 1} if args.emit_mode == "tables" else {}
    slab = min(S, 256)                              # four slabs per device and step from the shared queue: upload of the next under the compute of the last
    m = ed.MultiDevice(chrom_off, start, end, slab, devices=devices, **opts)
    par = {} if args.fit else {"phi": np.tile(phi.cpu().numpy(), N), "expected": np.tile(p.cpu().numpy(), N)}
    for _ in range(max(1, args.warmup)):
        res = m.run_host(pt.array, pr.array, 1, **par)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = m.run_host(pt.array, pr.array, 1, **par)
    el = time.perf_counter() - t0
    n_calls = len(res["calls"])

    out = {"metric": "exons*samples/s through betabinom emissions + Viterbi" + (" + dispersion fit" if args.fit else ""),
           "value": float(E) * S * N * args.steps / el, "unit": "exons*samples/s", "n_gpus": N, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": el / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
           "config": {"workload": "BASELINE.json configs[2] geometry per device: %d exons x %d samples, %d chromosomes, phi %s; ONE process, %d device(s) %s, "
                                  "host-resident counts (pinned, uint16 on the link, [samples][exons]) -> ed_multi_run_host -> merged call table"
                                  % (E, S, C, "fitted on device" if args.fit else "given", N, devices),
                      "exons": E, "samples_per_gpu": S, "samples_total": S * N, "fit": bool(args.fit), "emit_mode": args.emit_mode, "driver": "multi-device (ed_multi_run_host: one host thread per device, slabs from one queue, no collective)",
                      "slab_samples": slab, "devices": devices},
           "includes_h2d": True, "bytes_on_the_link_per_step": 2.0 * 2 * E * S * N,
           "devices": res["devices"],
           "devices_note": "last step: slabs / columns every device took from the shared queue, wall seconds of its host thread, the NUMA node the thread was kept on "
                           "(-1 unknown): an uneven split on an otherwise idle node points at a slow device or link",
           "n_calls": n_calls, "table_stats": res["table_stats"], "n_unconverged": res["n_unconverged"],
           "note": "host-fed: comparable with h2d.pinned of the default line (N = 1), not with its device-resident value; no roofline / cpu_baseline "
                   "on this line (see the default line)"}
    print(json.dumps(out))
    m.close(); pt.free(); pr.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--exons", type=int, default=200_000)
    ap.add_argument("--samples", type=int, default=1024, help="samples per GPU")
    ap.add_argument("--chroms", type=int, default=24)
    ap.add_argument("--depth", type=float, default=100.0, help="median reads per exon and sample of the synthetic counts (SURVEY.md 8d: 100)")
    ap.add_argument("--fit", type=int, default=1, help="1 (default): the step includes the per-sample dispersion fit (configs[2]); 0: phi given (configs[1] style)")
    ap.add_argument("--emit-mode", default="tables", choices=["strict", "tables", "tables-tile"], help="tables (default): per-(sample, state) "
                    "log-gamma difference tables, three lookups and a sum per cell, sample-major with the tables in LDS (csrc/edtab.inc; "
                    "within 1e-10 of the reference's arithmetic and the same Viterbi paths: verified after the timed region); strict: "
                    "every log-Beta through GSL's routes operation for operation (bit-identical to the checker); tables-tile: the tables "
                    "through L1/L2 on [exons][samples] tiles (diagnostic)")
    ap.add_argument("--fit-mode", type=int, default=0, choices=[0, 1], help="0 (default): maximum-likelihood (phi, expected) by Newton's method on the "
                    "count histograms; 1: aod::betabin's procedure (Nelder-Mead from the glm start, optim()'s tolerances) on the same histograms -- "
                    "a point inside optim()'s tolerance region, not pinned against aod itself.  The default line carries mode 1's rate "
                    "under extra.other_modes.fit_mode_1")
    ap.add_argument("--counts-layout", type=int, default=-1, help="1: the device count matrices are handed over sample-major, [samples][exons] -- "
                    "the memory image of R's column-major exons x samples matrix (emit mode tables only: no transposition inside the step); "
                    "0: [exons][samples]; -1 (default): 1 with --emit-mode tables, else 0")
    ap.add_argument("--strict-steps", type=int, default=6, help="--full with --emit-mode tables: timed steps of the same workload in strict mode and in "
                    "tables mode with [exons][samples] inputs, run after the timed region and reported under extra (0 = skip)")
    ap.add_argument("--fused", type=int, default=0, help="1: emissions + Viterbi as one kernel (csrc/edfused.inc)")
    ap.add_argument("--keep-loglik", type=int, default=1, help="fused mode: 0 = do not materialise the likelihood matrix")
    ap.add_argument("--phi-bins", type=int, default=1, help="> 1: the depth-binned dispersion model (phi.bins, csrc/edbins.inc); "
                    "an optional mode, not the headline configuration")
    ap.add_argument("--cov", type=int, default=0, help="> 0: the mean model with that many per-exon covariates (csrc/edcov.inc); "
                    "an optional mode, not the headline configuration")
    ap.add_argument("--counts-bits", type=int, default=32, help="16: the headline's device-resident counts are uint16 [samples][exons] (cohort option counts_bits; needs "
                    "--counts-layout 1): half the bytes of every pass over the counts.  The other legs keep int32")
    ap.add_argument("--lanes", type=int, default=0, help="cohort option `lanes`: 0 (default) = --batches-in-flight / 2 when that is 4, 6 or 8; 1 = one pipeline (round 4's form)")
    ap.add_argument("--pipeline", type=int, default=1, help="1 (default): --batches-in-flight slabs in flight (fit of the next batch and the Viterbi tail "
                    "of the previous one run underneath the emissions); 0: steps strictly one after the other")
    ap.add_argument("--viterbi-overlap", type=int, default=0, help="pipelined mode only: 0 (default) = all emissions of a batch as one "
                    "launch, its chains afterwards, next to the next batch's fit; 1 = chains of a chromosome group underneath "
                    "the emissions of the following groups (the lone-batch schedule); -1 = the library's default")
    ap.add_argument("--fit-priority", type=int, default=0, help="priority of the stream the fit runs on in pipelined mode (0 = normal; -1 = high: "
                    "the fit then pushes into the running emission launch and costs it more than it saves, 12.2 against 11.5 ms)")
    ap.add_argument("--kernel-alone", type=int, default=1, help="1 (default): with --full, after the timed region, time three emission launches with the GPU to "
                    "themselves (roofline.kernel_ms_alone); 0: skip (profiling passes, so that per-kernel averages contain the live launches only)")
    ap.add_argument("--pretouch-streams", type=int, default=0, help="(diagnostic) use that many unrelated streams before the pipeline's streams are first used")
    ap.add_argument("--hw-queues", type=int, default=0, help="(diagnostic) GPU_MAX_HW_QUEUES for this process unless the environment already sets it "
                    "(0, default = leave the runtime alone: the cohort pipeline gives its streams hardware queues of their own)")
    ap.add_argument("--driver", default="cohort", choices=["cohort", "python", "multi-device"], help="cohort (default): the steps are submitted to the "
                    "library's cohort pipeline (ed_cohort_*: its own streams, batch rotation, event-ordered stages); python: round 2's "
                    "orchestration of two batch objects with torch streams (kept for comparison); multi-device: ONE process drives --gpus N devices "
                    "through ed_multi_run_host (one host thread per device, no process group) -- the second N > 1 path, what the R-level "
                    ".Call entry runs on; launched as a plain `python bench.py --gpus N --driver multi-device`, NOT under torch.distributed.run")
    ap.add_argument("--devices", default="", help="--driver multi-device: comma-separated device ordinals (default 0..N-1; '0,0' = two pipelines on one GPU)")
    ap.add_argument("--split", type=float, default=-1.0, help="cohort driver: fraction of a slab's emission launch after which the next slab's fit "
                    "is issued (-1 = the library's default)")
    ap.add_argument("--own-queues", type=int, default=-1, help="cohort driver: 1 = every stream of the pipeline gets a hardware queue of its own, "
                    "0 = ordinary streams (-1 = the library's default, 1)")
    ap.add_argument("--tables-early", type=int, default=-1, help="cohort driver: 1 = a slab's per-sample constants and tables are made right behind its "
                    "fit on the fit stream, 0 = at the boundary between two emission launches (-1 = the library's default, 0)")
    ap.add_argument("--stage-inputs", type=int, default=1, help="1 (default, N = 1 only): with --full, additionally time the same steps with the counts uploaded from "
                    "host memory for every slab (copy stream, double-buffered device slabs): reported as value_with_h2d, never as value; 0: skip")
    ap.add_argument("--wire", type=int, default=2, help="--stage-inputs: bytes per count on the link (2 = uint16 widened on the device, 4 = int32)")
    ap.add_argument("--fit-concordance", type=int, default=64, help="--full: columns of the batch on which the whole path is run twice after the timed "
                    "region -- maximum-likelihood fit vs aod::betabin's Nelder-Mead procedure -- and the differences counted (0 = skip)")
    ap.add_argument("--config1-steps", type=int, default=20, help="--full: timed steps of the BASELINE configs[1] leg (200 000 x 64, phi given) run after "
                    "the headline and reported under extra.config1 (0 = skip)")
    ap.add_argument("--verify-columns", type=int, default=4, help="--full: columns of the last slabs checked against the CPU oracle after the timed region (0 = skip)")
    ap.add_argument("--batches-in-flight", type=int, default=6, help="slabs in flight in the library's cohort pipeline = batch objects used in rotation (>= 2).  "
                    "6 (default): three LANES of two slots -- independent pipelines inside the cohort object, one lane's emission launch fills the CUs that "
                    "another's table build and chains leave idle (profiles/r05_ab_lanes.txt, one box: 3.72-3.81 ms per step; 4 = two lanes: 3.79-3.90; "
                    "2 = one lane, round 4's form: 4.17-4.20; 8: 4.2)")
    ap.add_argument("--workflow-reps", type=int, default=3, help="--full, after the timed region: the reference's workflow for one cohort end to end -- "
                    "upload, reference sets, calls -- reported under extra.workflow; 0: skip")
    ap.add_argument("--regimes", type=int, default=1, help="1 (default, --full, N = 1, the default workload only): the headline's step at depths 25 / 400 / 1600 and at 64 / 256 samples "
                    "per slab, each with table statistics and the check against the CPU checker: extra.regimes")
    ap.add_argument("--dropin", type=int, default=1, help="1 (default, --full, N = 1): time the two reference-shaped entries (ed_get_loglike_matrix on all exons of a sample, ed_hmm on the "
                    "longest / a median chromosome, the 1 + 24-call sequence of one sample) next to the CPU port: extra.dropin")
    ap.add_argument("--lib-variant", default="", help="load exomedepth_amd/libedcore_<name>.so instead of libedcore.so (experiments only)")
    ap.add_argument("--cpu-all-cores", type=int, default=1, help="1: also time the CPU baseline with one sample per host core "
                    "(process-level parallelism; reported inside cpu_baseline.all_cores)")
    ap.add_argument("--cpu-samples", type=int, default=12, help="--full: columns timed on the host for cpu_baseline (0 = skip)")
    ap.add_argument("--full", action="store_true", help="after the timed region, also run the legs that check and extend the headline (each "
                    "under its own option above): kernel alone, verify, fit concordance, configs[1], host-fed steps, workflow, drop-in entries, regimes, "
                    "other modes, CPU baseline.  Without it a run times the headline only")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps, write what the last one computed as .npy files "
                    "under DIR (cohort driver; rank 0's slab): per-sample parameters, call table, likelihoods and Viterbi states of sampled columns")
    args = ap.parse_args()
    if args.cov > 0 or args.phi_bins > 1 or args.fused:      # the table-driven mode serves the default model (per-sample phi and expected)
        args.emit_mode = "strict"
    if args.counts_layout < 0:
        args.counts_layout = 1 if args.emit_mode == "tables" else 0
    assert args.counts_layout == 0 or args.emit_mode == "tables", "--counts-layout 1 goes with --emit-mode tables"

    # HIP multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) in creation order, and which streams share
    # a queue decides how the pipelined schedule unfolds.  With 6, the fit of the next batch is served in
    # the middle of this batch's emission launch and the chains ride under the start of the next one: 0.6 ms between
    # emission launches instead of 2.3, 5-6 % more exons*samples/s (measured on three boxes; 4, 5, 7, 8, 16: slower).
    # Must be in the environment before the HIP runtime starts, i.e. before torch is imported.
    if args.hw_queues > 0:
        os.environ.setdefault("GPU_MAX_HW_QUEUES", str(args.hw_queues))

    if args.driver == "multi-device":
        if args.dump_outputs:
            ap.error("--dump-outputs needs the cohort driver")
        return multi_device_main(args)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # ED_BENCH_BACKEND=gloo + ED_BENCH_SHARE_GPU=1 let the N>1 code path be exercised on a 1-GPU box (functional
    # check only: every rank then uses GPU 0 and the call-table gather goes through host memory)
    backend = os.environ.get("ED_BENCH_BACKEND", "nccl")
    if os.environ.get("ED_BENCH_SHARE_GPU") == "1":
        local_rank = 0
    # ED_BENCH_FORCE_PG=1: a process group of ONE rank on a 1-GPU box -- RCCL's streams and queue usage without a second GPU
    use_pg = world > 1 or os.environ.get("ED_BENCH_FORCE_PG") == "1"

    def init_pg():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        # stdout carries ONE line, the JSON record.  With NCCL_DEBUG=VERSION (the GPU boxes export it) RCCL printf()s a five-line banner to stdout when its
        # communicator is made; NCCL_DEBUG_FILE does not move it.  So file descriptor 1 points at stderr while the group and its communicator come up
        # (the first collective), the C library's buffers are flushed there, and stdout is put back: the banner lands next to the other diagnostics.
        import ctypes
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            if backend == "nccl":
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
            else:
                dist.init_process_group(backend)
            dist.barrier()
            torch.cuda.synchronize()
            ctypes.CDLL(None).fflush(None)
        finally:
            os.dup2(saved, 1)
            os.close(saved)

    # The process group is initialised AFTER the pipeline's streams have been used once (below): hardware queues are handed to
    # streams in order of first use, and RCCL takes one when it starts -- which would shift the stream-to-queue mapping of
    # DESIGN.md 4.10 (vi) by one and cost its 5-6 %.  Only a never-built tree needs the group first (ranks wait for rank 0's build).
    from exomedepth_amd import _build as _build0
    pg_early = use_pg and (not os.path.exists(_build0.LIB) or os.environ.get("ED_BENCH_PG_FIRST") == "1")
    if pg_early:
        init_pg()
    cdev = torch.device("cuda", local_rank) if backend == "nccl" else torch.device("cpu")   # device of the collectives
    if args.gpus != world:
        if rank == 0:
            print("bench.py: --gpus %d but WORLD_SIZE=%d (launch with torch.distributed.run for N>1)"
                  % (args.gpus, world), file=sys.stderr)
        if args.gpus > 1 and world == 1:
            sys.exit(2)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    if args.lib_variant:      # a diagnostic build of the library (exomedepth_amd/_build.py::VARIANTS), never the default
        from exomedepth_amd import _build as _b, _lib as _l
        _l.LIB_PATH = _b.variant_path(args.lib_variant)
    import exomedepth_amd as ed
    from exomedepth_amd import _build, dist as eddist
    if not os.path.exists(_build.LIB) and rank == 0:   # never-built tree: compile the HIP library (there is no other path)
        _build.build()
    if pg_early:
        dist.barrier()
    from exomedepth_amd import synth

    E, S, C = args.exons, args.samples, args.chroms
    chrom_off, start, end = synth.exon_design(E, C, seed=20250620)
    torch.manual_seed(20250620 + 3 + rank)
    test, ref, p, phi = synth.counts_torch(chrom_off, S, dev, seed=20250620 + 3 + 1000 * rank, mean_depth=args.depth)
    torch.cuda.synchronize()

    # (diagnostic) other streams used before the pipeline's: shifts the stream-to-hardware-queue mapping by that many
    _pre_streams = [torch.cuda.Stream(device=dev) for _ in range(max(0, args.pretouch_streams))]
    for _s in _pre_streams:
        with torch.cuda.stream(_s):
            torch.zeros(8, device=dev).add_(1)
    torch.cuda.synchronize()
    plan = ed.Plan(chrom_off, start, end, 1e-4, 50000.0, device=local_rank)
    plain = args.cov == 0 and args.phi_bins == 1
    bins_cohort = args.driver == "cohort" and args.cov == 0 and args.phi_bins > 1 and args.fit and not args.fused
    use_cohort = args.driver == "cohort" and (plain or bins_cohort) and not args.fused
    if args.dump_outputs and not use_cohort:
        ap.error("--dump-outputs needs the cohort driver")
    step_no = [0]
    if use_cohort:
        # The library's cohort pipeline: every step is ONE submission (ed_cohort_submit); the library owns the streams, rotates
        # its batch objects and orders the stages of consecutive slabs with events (csrc/edcohort.inc).
        # --pipeline 0: one slab in flight, i.e. the steps strictly one after the other.
        n_batches = max(2, args.batches_in_flight) if args.pipeline else 1
        opts = {"timing": 0 if os.environ.get("ED_BENCH_NO_STAGE_TIMING") == "1" else 1}   # (diagnostic: what do the library's stage events cost?)
        if args.viterbi_overlap >= 0:
            opts["viterbi_overlap"] = args.viterbi_overlap
        if args.split >= 0:
            opts["split"] = args.split
        if args.own_queues >= 0:
            opts["own_queues"] = args.own_queues
        if args.tables_early >= 0:
            opts["tables_early"] = args.tables_early
        if bins_cohort:
            args.emit_mode, args.counts_layout = "strict", 0
        opts.update(mode_opts(args))
        if args.counts_bits == 16:
            opts["counts_bits"] = 16
        if n_batches in (4, 6, 8) and args.lanes != 1:
            opts["lanes"] = args.lanes if args.lanes > 1 else n_batches // 2      # independent pipelines inside the cohort object (csrc/edcohort.inc)
        if bins_cohort:
            opts["phi_bins"] = args.phi_bins          # the depth-binned model through the same pipeline (option phi_bins)
            if os.environ.get("ED_BENCH_BINS_PIECES"):
                opts["bins_pieces"] = int(os.environ["ED_BENCH_BINS_PIECES"])
        co = ed.Cohort(plan, S, n_batches, **opts)
        opts_headline = dict(opts)
        batches = []
        last_ticket = [-1]

        # what the steps are handed: the [E][S] matrices, or (--counts-layout 1) their sample-major images, made once, outside the timed region
        test_in, ref_in = (test.t().contiguous(), ref.t().contiguous()) if args.counts_layout == 1 else (test, ref)
        if args.counts_bits == 16:
            assert args.counts_layout == 1 and int(test.max()) < 65536 and int(ref.max()) < 65536 and int(test.min()) >= 0 and int(ref.min()) >= 0
            test_in, ref_in = test_in.to(torch.int16), ref_in.to(torch.int16)     # (the low 16 bits: uint16 counts in an int16 tensor)

        def step():
            step_no[0] += 1
            if args.fit:
                last_ticket[0] = co.submit(test_in, ref_in, n_samples=S)
            else:
                last_ticket[0] = co.submit(test_in, ref_in, phi=phi, expected=p, n_samples=S)

        def last_batch():
            b, _, _ = co.batch(last_ticket[0])
            b.n_samples = S
            return b

        def drain():
            co.drain()

        def stage_totals():
            return [co.stage_ms_total()]

        def reset_timing():
            co.set_option("timing", 1)

        n_launch_of = lambda: co.n_emit_launches
    else:
        # round 2's driver: two batch objects used alternately, orchestrated here with torch streams
        n_batches = max(2, args.batches_in_flight) if (args.pipeline and plain and not args.fused) else 1
        batches = [ed.Batch(plan, S) for _ in range(n_batches)]
        for b in batches:
            b.enable_timing(True)
            b.set_fused(bool(args.fused))
            b.keep_loglik(bool(args.keep_loglik))
            b.set_async_tail(n_batches >= 2)
            if args.emit_mode != "strict" and plain and not args.fused:
                b.set_emit_mode(EMIT_MODES[args.emit_mode])
                b.set_counts_layout(args.counts_layout)
            if n_batches >= 2 and args.viterbi_overlap >= 0:
                b.set_viterbi_overlap(bool(args.viterbi_overlap))
        main_stream = torch.cuda.current_stream()
        fit_stream = torch.cuda.Stream(device=dev, priority=args.fit_priority) if n_batches >= 2 else main_stream
        stream = main_stream.cuda_stream
        phi_fit = [torch.empty(S, dtype=torch.float64, device=dev) for _ in batches]
        p_fit = [torch.empty(S, dtype=torch.float64, device=dev) for _ in batches]
        phib_fit = torch.empty((max(args.phi_bins, 1), S), dtype=torch.float64, device=dev)
        Xcov = (torch.rand((E, max(args.cov, 1)), dtype=torch.float64, device=dev) - 0.5) * 0.4 if args.cov > 0 else None
        beta_fit = torch.empty((max(args.cov, 0) + 1, S), dtype=torch.float64, device=dev)
        edges_fit = torch.empty((max(args.phi_bins, 1) + 1, S), dtype=torch.float64, device=dev)
        emitted = [None] * n_batches     # per batch object: event on the main stream after its last run's emission launches

        def step():
            k = step_no[0] % n_batches
            step_no[0] += 1
            b = batches[k]
            if args.cov > 0:
                b.fit_cov(test, ref, Xcov, beta_fit, phi_fit[0], stream=stream)
                b.run_cov(test, ref, Xcov, beta_fit, phi_fit[0], 1.0, stream=stream)
            elif args.phi_bins > 1:
                b.fit_bins(test, ref, args.phi_bins, phib_fit, edges_fit, p_fit[0], stream=stream)
                b.run_bins(test, ref, args.phi_bins, phib_fit, edges_fit, p_fit[0], 1.0, stream=stream)
            elif args.fit:
                if fit_stream is not main_stream and emitted[k] is not None:
                    fit_stream.wait_event(emitted[k])   # (phi, expected) of this batch object's previous run are still being read
                b.fit(test, ref, phi_fit[k], p_fit[k], stream=fit_stream.cuda_stream)
                if fit_stream is not main_stream:
                    main_stream.wait_stream(fit_stream)      # the emissions of this batch need its (phi, expected)
                b.run(test, ref, phi_fit[k], p_fit[k], 1.0, stream=stream)
                if fit_stream is not main_stream:
                    emitted[k] = torch.cuda.Event()
                    emitted[k].record(main_stream)
            else:
                b.run(test, ref, phi, p, 1.0, stream=stream)

        def last_batch():
            return batches[(step_no[0] - 1) % n_batches]

        def drain():
            for j, b in enumerate(batches):
                if j < step_no[0]:
                    b.n_calls()                               # (a batch object that has run: wait for its tail)

        def stage_totals():
            return [b.stage_ms_total() for b in batches]

        def reset_timing():
            for b in batches:
                b.enable_timing(True)

        n_launch_of = lambda: batches[0].n_emit_launches

    def finish(collect=True):
        """final gather of the compact call tables (the path's only collective); every slab in flight is drained"""
        drain()
        last = last_batch()
        if world > 1 and collect:
            # rows straight from the device table when the collectives run on the GPU (RCCL); through the host for gloo
            t = eddist.device_call_table(last) if cdev.type == "cuda" else eddist.calls_to_tensor(last.calls(), cdev)
            g = eddist.gather_call_tables(t, rank * S)
            return int(g.shape[0]) if g is not None else 0
        return last.n_calls()

    for _ in range(n_batches):        # setup: every batch object allocates its working set (likelihood matrix, fit workspace) once
        step()                        # ... and every stream of the pipeline is used for the first time
    finish(collect=pg_early)
    torch.cuda.synchronize()
    if use_pg and not pg_early:
        init_pg()
    if use_pg:
        dist.barrier()
    step_no[0] = 0
    for _ in range(args.warmup):
        step()
    finish()
    torch.cuda.synchronize()
    reset_timing()                    # (resets the stage-time sums: the warm-up is not part of them)
    if use_pg:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    n_calls = finish()
    torch.cuda.synchronize()
    if use_pg:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    table_stats = last_batch().table_stats() if (plain and not args.fused and args.emit_mode != "strict") else None    # (after the clock: the last timed step's)
    if use_pg:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
    if args.dump_outputs and rank == 0:       # before anything else is submitted: the last timed slab's results are still in its batch object
        dump_outputs(args.dump_outputs, torch, eddist, dev, co, last_ticket[0], E, S)

    cells_per_step = E * S * world
    value = cells_per_step * args.steps / elapsed
    # per-stage device times: HIP events recorded by the library on the streams the kernels run on, summed over the timed steps
    stage_ms = {k: 0.0 for k in ed.Batch.STAGES}
    n_timed = 0
    for tot, nr, nf in stage_totals():
        n_timed += nr
        for k, v in tot.items():
            stage_ms[k] += v
    assert n_timed == args.steps or os.environ.get("ED_BENCH_NO_STAGE_TIMING") == "1", (n_timed, args.steps)
    stage_ms = {k: v / args.steps for k, v in stage_ms.items()}
    n_launch = max(1, n_launch_of())   # emission launches per step
    # chip time of the emission launches: with several lanes they run side by side, so the union of their intervals (HIP events of the library on
    # the streams the launches run on, relative to one reference event) is what the chip spends on them, their mean length a launch's own duration
    emit_union_ms = emit_own_ms = None
    if use_cohort and os.environ.get("ED_BENCH_NO_STAGE_TIMING") != "1":
        iv = co.emission_intervals()
        if len(iv) == args.steps:
            u, o_ = interval_union(iv)
            emit_union_ms, emit_own_ms = u / args.steps, o_ / args.steps
    # (outside the timed region) the emission launches with the GPU to themselves: one slab, given phi, nothing queued on
    # other streams -- what the kernel takes when it does not host the next slab's fit and the previous slab's chains
    alone_ms = None
    if args.full and plain and not args.fused and args.pipeline and rank == 0 and args.kernel_alone:
        if use_cohort:
            b_last, pp, pe = co.batch(last_ticket[0])
            par = (ed.api._RawDevice(pp), ed.api._RawDevice(pe)) if args.fit else (phi, p)
            reset_timing()
            for _ in range(3):
                last_ticket[0] = co.submit(test_in, ref_in, phi=par[0], expected=par[1], n_samples=S)
                co.drain()
            alone_ms = co.stage_ms_total()[0]["emissions"] / 3.0
        else:
            bb = batches[0]
            bb.enable_timing(True)
            for _ in range(3):
                bb.run(test, ref, phi_fit[0] if args.fit else phi, p_fit[0] if args.fit else p, 1.0, stream=stream)
                torch.cuda.synchronize()
                bb.wait()
            alone_ms = bb.stage_ms()["emissions"]

    # ---- after the timed region (--full): the bench checks what it timed, and carries the legs the headline does not --------
    # A leg that fails on ONE rank must not cost the line its headline (measured above): it reports {"error": ...} instead.  (With several
    # ranks a leg holds collectives -- a rank that skipped the rest of it would leave the others waiting -- so there a failure stays fatal.)
    def leg(fn, *a, **k):
        if world > 1:
            return fn(*a, **k)
        try:
            return fn(*a, **k)
        except Exception as e:          # noqa: BLE001
            import traceback
            return {"error": "%s: %s" % (type(e).__name__, e), "where": traceback.format_exc().strip().splitlines()[-3:]}
    verify = None
    if args.full and world == 1 and args.verify_columns > 0 and plain and not args.fused:      # (N = 1 only, like cpu_baseline: the other ranks would wait)
        verify = leg(verify_against_oracle, ed, eddist, torch, dev, co if use_cohort else None, batches, last_ticket[0] if use_cohort else None,
                                       n_batches, test, ref, phi, p, phi_fit if not use_cohort else None, p_fit if not use_cohort else None,
                                       bool(args.fit), chrom_off, start, end, args.verify_columns, tables=args.emit_mode != "strict")
    # The headline's cohort object is done: its streams (a hardware queue each) go back before the other legs make theirs -- with the four slabs / two lanes
    # of the default line, the 200 000 x 64 leg's six-slot pipeline otherwise finds the device's hardware queues oversubscribed now and then and runs
    # its slabs one after the other (1.6 ms per slab instead of 0.66, bimodal from run to run).
    if use_cohort:
        co.close()
        co = None
    fit_conc = None
    if args.full and world == 1 and args.fit and plain and not args.fused and args.fit_concordance > 0:
        from exomedepth_amd import concordance
        k = min(args.fit_concordance, S)
        fit_conc = leg(concordance.fit_mode_concordance, plan, test[:, :k].contiguous(), ref[:, :k].contiguous())
    config1 = None
    if args.full and world == 1 and args.config1_steps > 0 and plain and not args.fused and S >= 64:
        config1 = leg(config1_leg, ed, torch, plan, test, ref, phi, p, E, args.config1_steps, mode_opts(args))
    staged = None
    if args.full and world == 1 and args.stage_inputs and use_cohort:
        staged = leg(staged_leg, ed, torch, plan, test, ref, phi, p, E, S, min(n_batches, 2), args)     # (host-fed slabs: two / three slabs in flight, one lane -- the link is the bound)
    if staged is not None and "error" not in staged and args.emit_mode == "tables" and args.counts_layout == 1:
        staged["r_entry"] = leg(r_entry_leg, ed, chrom_off, start, end, test, ref, S, max(2, args.steps // 3), args.fit, phi, p)
    workflow = None
    if args.full and args.workflow_reps > 0 and plain and args.fit and not args.fused and S >= 64 and (world == 1 or use_pg):
        workflow = leg(workflow_leg, ed, torch, plan, test, start, end, E, S, args.workflow_reps, EMIT_MODES[args.emit_mode], world, rank, eddist)
    dropin = None
    if args.full and world == 1 and args.dropin and plain and not args.fused:
        dropin = leg(dropin_leg, ed, chrom_off, start, end, test[:, :2].cpu().numpy(), ref[:, :2].cpu().numpy(), phi.cpu().numpy(), p.cpu().numpy())
    regimes = None
    if args.full and world == 1 and args.regimes and use_cohort and plain and not args.fused and args.emit_mode == "tables" and (E, S, int(args.depth)) == (200_000, 1024, 100):
        regimes = []
        for (dpt, ss) in ((25.0, 1024), (400.0, 1024), (1600.0, 1024), (100.0, 256), (100.0, 64)):
            regimes.append(leg(regime_leg, ed, eddist, torch, dev, plan, chrom_off, start, end, E, ss, dpt, args.fit, {k: v for k, v in opts_headline.items() if k != "timing"},
                               n_batches, 8, 20250620 + 3 + int(dpt) + ss, 2))
    other_modes = None
    if args.full and world == 1 and args.strict_steps > 0 and plain and not args.fused and use_cohort and args.emit_mode == "tables":
        other_modes = {"strict": leg(mode_leg, ed, torch, plan, test, ref, S, args.strict_steps, args.fit, phi, p, {}),
                       "fit_mode_1": (leg(mode_leg, ed, torch, plan, test, ref, S, args.strict_steps, True, phi, p, {**mode_opts(args), "fit_mode": 1})
                                      if args.fit and args.fit_mode == 0 else None),
                       "tables_counts_exons_x_samples": leg(mode_leg, ed, torch, plan, test, ref, S, args.strict_steps, args.fit, phi, p, {"emit_mode": 2}),
                       "tables_counts_16_bit": (leg(mode_leg, ed, torch, plan, test, ref, S, 2 * args.strict_steps, args.fit, phi, p,
                                                    {**opts_headline, "counts_bits": 16, "timing": 0}, n_batches) if args.counts_layout == 1 and args.counts_bits == 32 else None),
                       "tables_counts_32_bit_same_leg": (leg(mode_leg, ed, torch, plan, test, ref, S, 2 * args.strict_steps, args.fit, phi, p,
                                                             {**opts_headline, "timing": 0}, n_batches) if args.counts_layout == 1 and args.counts_bits == 32 else None),
                       "note": "the same workload and pipeline, after the timed region: strict = emit mode 0 (GSL's arithmetic operation for operation, "
                               "bit-identical to the checker: rounds 1-3's headline); fit_mode_1 = the headline's mode with the dispersion fit by "
                               "aod::betabin's Nelder-Mead procedure (--fit-mode 1) instead of Newton's method; tables_counts_exons_x_samples = the headline's mode handed "
                               "[exons][samples] count matrices (it then transposes them inside every step); tables_counts_16_bit = the headline's mode, slabs in flight and lanes with the "
                               "device-resident counts as uint16 (cohort option counts_bits = 16: half the bytes of every pass over the counts; same likelihood bits, paths, calls), and "
                               "tables_counts_32_bit_same_leg = the headline's own configuration run the same way right after it, for comparison"}

    if rank == 0:
        kernel = "k_emit_viterbi" if args.fused else ({"strict": "k_emit_batch", "tables-tile": "k_emit_tab", "tables": "k_emit_tab_sm"}[args.emit_mode] if plain else "k_emit_bins")
        # kernel_ms: the CHIP's time per emission launch over the timed steps = union of the launches' intervals / launches.  One pipeline: that is the
        # launch's own duration.  Several lanes (the default): the emission launches of consecutive slabs run side by side, a launch's own duration
        # (kernel_ms_own, what a kernel trace's average shows) is longer than the chip spends on it, and dividing bytes by it would measure the overlap.
        own_ms_step = stage_ms["emissions"]
        chip_ms_step = emit_union_ms if emit_union_ms else own_ms_step
        t_emit = chip_ms_step * 1e-3
        achieved = ALGO_BYTES_PER_CELL * E * S / t_emit / 1e9 if t_emit > 0 else 0.0
        kernel_cells_per_s = (E * S / t_emit) if t_emit else 0.0
        meta, why_not = matching_profile()
        if meta:
            # the counters describe the workload they were collected on: same exons x samples, same kernel, same number of
            # emission launches per run (profiles/<tag>_meta.json "workload"); anything else gets no counter figures
            w = meta.get("workload", {"exons": 200_000, "samples_per_gpu": 1024, "kernel": "k_emit_batch", "emission_launches_per_run": 1})
            if (w.get("exons"), w.get("samples_per_gpu"), w.get("kernel"), w.get("emission_launches_per_run")) != (E, S, kernel, n_launch):
                meta, why_not = None, ("profile %s was collected on %s: its counters are not quoted for this workload / schedule"
                                       % (meta["tag"], json.dumps(w)))
        pmc = pmc_figures(meta, kernel, float(E) * S, kernel_cells_per_s) if meta else None
        traffic = pmc.get("traffic_bytes_per_step") / n_launch if pmc and "traffic_bytes_per_step" in pmc else None
        step_ms = elapsed / args.steps * 1e3
        gbs = lambda ms: (ALGO_BYTES_PER_CELL * E * S / (ms * 1e-3) / 1e9) if ms else None
        frac_of = lambda ms: (gbs(ms) / HBM_PEAK_GBS) if ms else None
        out = {
            "metric": "exons*samples/s through betabinom emissions + Viterbi" + (" + dispersion fit" if args.fit else ""),
            "value": value, "unit": "exons*samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": step_ms, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[2] geometry: %d exons x %d samples per GPU, %d chromosomes, "
                                   "phi %s, transition.probability 1e-4, expected.CNV.length 5e4"
                                   % (E, S, C, "fitted on device" if args.fit else "given per sample (fixed)"),
                       "exons": E, "samples_per_gpu": S, "samples_total": S * world, "fit": bool(args.fit), "fit_mode": args.fit_mode, "emit_mode": args.emit_mode, "counts_layout": ("[samples][exons]" if args.counts_layout == 1 else "[exons][samples]"), "counts_bits": args.counts_bits, "fused": bool(args.fused), "phi_bins": args.phi_bins, "covariates": args.cov,
                       "depth": args.depth, "batches_in_flight": n_batches, "driver": ("cohort (ed_cohort_submit: the library's own streams and batch rotation)" if use_cohort else "python (torch streams)"),
                       "parallelism": "samples sharded, %d rank(s); call tables gathered to rank 0 over RCCL" % world},
            "roofline": {"bound": "hbm", "kernel": kernel, "achieved": achieved, "peak": HBM_PEAK_GBS,
                         "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                         "traffic_source": (pmc["profile"] + "_pmc_FETCH_SIZE/WRITE_SIZE.csv") if traffic is not None else why_not,
                         "algorithmic_bytes_per_cell": ALGO_BYTES_PER_CELL, "launches_per_step": n_launch,
                         "algorithmic_bytes_per_launch": ALGO_BYTES_PER_CELL * E * S / n_launch,
                         "kernel_ms": chip_ms_step / n_launch, "kernel_ms_per_step": chip_ms_step,
                         "kernel_ms_is": ("union of the emission launches' intervals over the timed steps / launches (HIP events of the library on the streams the launches "
                                          "run on: ed_cohort_emission_intervals) = the chip's time per launch; <= ms_per_step by construction" if emit_union_ms
                                          else "mean duration of the emission launches (HIP events of the library on the stream they run on)"),
                         "kernel_ms_own": own_ms_step / n_launch,
                         "launches_in_flight": (own_ms_step / chip_ms_step if chip_ms_step else None),
                         "lanes": (opts.get("lanes", 1) if use_cohort else 1),
                         "kernel_ms_alone": alone_ms,
                         "frac_own": frac_of(own_ms_step), "frac_alone": frac_of(alone_ms), "frac_step": frac_of(step_ms),
                         "kernel_cells_per_s": kernel_cells_per_s,
                         "step_traffic_bytes": (pmc.get("step_traffic_bytes") if pmc else None),
                         "step_traffic_over_algorithmic": (pmc["step_traffic_bytes"] / (ALGO_BYTES_PER_CELL * float(E) * S) if pmc and pmc.get("step_traffic_bytes") else None),
                         "step_traffic_GBps": (pmc["step_traffic_bytes"] / (elapsed / args.steps) / 1e9 if pmc and pmc.get("step_traffic_bytes") else None),
                         "algorithmic_bytes_per_cell_with_likelihood_matrix": 33,
                         "frac_with_likelihood_matrix": (33 * E * S / t_emit / 1e9 / HBM_PEAK_GBS) if t_emit > 0 else None,
                         "frac_alone_with_likelihood_matrix": (33 * E * S / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if alone_ms else None,
                         "profile": ({"tag": meta["tag"], "timed_launches": meta.get("emission_overlap"),
                                      "reproduce": "profiles/%s_kernel_stats_timed.csv: bytes per launch / union_ms_per_launch of %s / 8 TB/s = frac; its mean_ms = kernel_ms_own"
                                                   % (meta["tag"], kernel)} if meta else None),
                         "frac_note": "frac: a launch's algorithmic bytes over the chip's time for it (kernel_ms).  frac_own: over the launch's own duration -- with several "
                                      "lanes in flight that measures how many launches share the chip (launches_in_flight), not the kernel.  frac_alone: the same "
                                      "launch with the GPU to itself.  frac_step: the whole step (ms_per_step) against the same bytes",
                         "valu": pmc if pmc else why_not,
                         "note": (NOTE_TABLES if args.emit_mode == "tables" and plain else NOTE_STRICT)},
            "stage_ms": stage_ms,
            "stage_ms_note": "device time between the library's stage events, mean per step.  With 2 batches in flight `viterbi` and "
                             "`call_table` are latencies of the batch's tail on its own streams and `fit` runs on a second stream: "
                             "they overlap the emissions of the neighbouring batch and do not add up to ms_per_step",
            "n_calls": n_calls,
            "table_stats": table_stats,
            "table_stats_note": "table-driven emission modes, last timed step: cells on the strict lists (outside their sample's tables or under its "
                                "few-reads rule), samples without tables (evaluated whole by the strict arithmetic) and their cells, launches whose "
                                "lists ran out (every cell looked at again)",
            "verify": verify,
            "fit_concordance": fit_conc,
            "extra": {"config1": config1, "workflow": workflow, "other_modes": other_modes, "dropin": dropin,
                      "regimes": ({"rows": regimes, "headline_row": {"depth": args.depth, "samples": S, "ms_per_step": step_ms, "ns_per_cell": step_ms * 1e6 / (float(E) * S),
                                                                        "emission_ms_chip": chip_ms_step, "emission_ms_own": own_ms_step, "table_stats": table_stats},
                                   "note": "the default line's step in other regimes of the synthetic generator (depth = median reads per exon and test sample; the aggregate "
                                           "references are 8 x deeper), same cohort options, 8 timed steps each, 2 columns of the last 2 slabs checked against the CPU checker"}
                                  if regimes else None)},
        }
        if staged:
            if "value_with_h2d" in staged:
                out["value_with_h2d"] = staged.pop("value_with_h2d")
            out["h2d"] = staged
        if args.full and world == 1 and args.cpu_samples > 0:
            k = min(args.cpu_samples, S)
            ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
            out["cpu_baseline"] = leg(cpu_baseline, test[:, :k].cpu().numpy(), ref[:, :k].cpu().numpy(),
                                      p[:k].cpu().numpy(), phi[:k].cpu().numpy(), chrom_off, start, end, bool(args.fit),
                                      allcores=ncores if args.cpu_all_cores else 0)
            if "error" not in out["cpu_baseline"]:
                out["speedup_vs_cpu_1core"] = value / out["cpu_baseline"]["value"]
                out["speedup_vs_cpu_1core_without_fit_standin"] = value / out["cpu_baseline"]["value_without_fit"]
        print(json.dumps(out))
    for b in batches:
        b.close()
    if use_cohort and co is not None:
        co.close()
    plan.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
