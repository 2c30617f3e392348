"""Host-side mirror of the reference's interface for the hot path, on top of the C-ABI (libedcore.so).

Names, argument meaning and error behaviour follow the reference's R layer so that the parity tests
read like the reference's own examples:

    get_loglike_matrix(...)   <- .Call("get_loglike_matrix", ...)      reference R/class_definition.R:184-189
    viterbi_hmm(...)          <- viterbi.hmm()                         reference R/tools.R:88-103
    ExomeDepth(...)           <- new('ExomeDepth', test=, reference=)  reference R/class_definition.R:82-191
    ExomeDepth.CallCNVs(...)  <- CallCNVs()                            reference R/class_definition.R:311-419
    ExomeDepth.TestCNV(...)   <- TestCNV()                             reference R/class_definition.R:243-256
    Plan / Batch              the batched, device-resident interface (no counterpart in the reference,
                              whose granularity is one sample and one chromosome per call)

All arithmetic of the path runs on the GPU; this module only marshals buffers (numpy on the host,
optionally torch CUDA tensors for device-resident inputs).
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from . import _lib
from ._lib import EdCall, EdCallInfo, EdError, EdRefsetRow, check, lib

CALL_DTYPE = np.dtype([("sample", "<i4"), ("chrom", "<i4"), ("start_exon", "<i4"), ("end_exon", "<i4"),
                       ("type", "<i4"), ("nexons", "<i4")])
assert CALL_DTYPE.itemsize == C.sizeof(EdCall)
CALL_INFO_DTYPE = np.dtype([("BF_raw", "<f8"), ("BF", "<f8"), ("reads_expected", "<i8"), ("reads_observed", "<i8"),
                            ("reads_ratio", "<f8")])
assert CALL_INFO_DTYPE.itemsize == C.sizeof(EdCallInfo)
CALL_POST_DTYPE = np.dtype([("post_mean", "<f8"), ("post_min", "<f8"), ("log_p_all", "<f8"), ("log_evidence", "<f8")])
CALL_BOUNDS_DTYPE = np.dtype([("anchor_exon", "<i4"), ("start_lo", "<i4"), ("start_hi", "<i4"), ("end_lo", "<i4"), ("end_hi", "<i4"),
                              ("flags", "<i4"), ("log_anchor", "<f8"), ("log_keep_start", "<f8"), ("log_keep_end", "<f8")])
assert CALL_BOUNDS_DTYPE.itemsize == 48


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _as_r_integer(x):
    """R's as.integer() on a numeric vector: truncation toward zero (R/class_definition.R:187-188)."""
    a = np.asarray(x)
    if a.dtype.kind in "iu":
        return a.astype(np.int32)
    return np.trunc(a).astype(np.int32)


# ---------------------------------------------------------------------------------------------
# the two .Call drop-ins
# ---------------------------------------------------------------------------------------------
def get_loglike_matrix(phi, expected, total, observed, mixture=1.0, return_errors=False):
    """Per-exon log-likelihoods of the three copy-number states; (n,3) array with columns
    (deletion, normal, duplication) -- reference src/CNV_estimate.cpp:52-85."""
    total = _i32(total)
    n = total.size
    phi = _f64(np.broadcast_to(np.asarray(phi, dtype=np.float64), (n,)))
    expected = _f64(np.broadcast_to(np.asarray(expected, dtype=np.float64), (n,)))
    observed = _i32(observed)
    if observed.size != n:
        raise ValueError("total and observed must have the same length")
    if mixture != 1:
        # reference src/CNV_estimate.cpp:61
        sys.stdout.write("As a warning (this could be normal), the mixture coefficient is %f\n" % mixture)
    out = np.empty((3, n), dtype=np.float64)  # column-major n x 3
    nerr = C.c_int64(0)
    check(lib().ed_get_loglike_matrix(_ptr(phi), _ptr(expected), _ptr(total), _ptr(observed), n, float(mixture),
                                      _ptr(out), C.byref(nerr)))
    return (out.T, nerr.value) if return_errors else out.T


def device_count():
    """HIP devices visible to the process (ed_device_count)"""
    return int(lib().ed_device_count())


def viterbi_hmm(transitions, loglikelihood, positions, expected_CNV_length):
    """reference R/tools.R:88-103.  loglikelihood: (nobs, nstates) in HMM order (normal, deletion,
    duplication).  Returns {'Viterbi.path': int array, 'calls': structured array with fields
    start.p, end.p, type, nexons} (1-based positions like the reference)."""
    T = np.asarray(transitions, dtype=np.float64)
    ll = np.asarray(loglikelihood, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1]:
        raise ValueError("Transition matrix is not square")
    positions = _i32(positions)
    if positions.size != ll.shape[0]:
        raise ValueError("The number of positions are not matching the number of rows of the likelihood matrix "
                         "%d and %d" % (positions.size, ll.shape[0]))
    nstates, nobs = T.shape[0], ll.shape[0]
    Tc = _f64(T.T.ravel())
    llc = _f64(ll.T.ravel())
    path = np.empty(nobs, dtype=np.float64)
    cap = max(nobs, 1)
    calls = np.zeros((4, cap), dtype=np.float64)  # column-major cap x 4
    nc = C.c_int64(0)
    check(lib().ed_hmm(nstates, nobs, _ptr(Tc), _ptr(llc), _ptr(positions), float(expected_CNV_length), _ptr(path),
                       _ptr(calls), cap, C.byref(nc)))
    k = nc.value
    rec = np.zeros(k, dtype=[("start.p", "f8"), ("end.p", "f8"), ("type", "f8"), ("nexons", "f8")])
    for j, name in enumerate(rec.dtype.names):
        rec[name] = calls[j, :k]
    return {"Viterbi.path": path.astype(np.int64), "calls": rec}


# ---------------------------------------------------------------------------------------------
# device buffers
# ---------------------------------------------------------------------------------------------
class DeviceArray:
    """A device allocation made through the library (for callers without torch)."""

    def __init__(self, host=None, nbytes=None):
        self.ptr = C.c_void_p()
        self.host_dtype = None
        self.shape = None
        if host is not None:
            host = np.ascontiguousarray(host)
            nbytes = host.nbytes
            self.host_dtype, self.shape = host.dtype, host.shape
        self.nbytes = int(nbytes)
        check(lib().ed_malloc(C.byref(self.ptr), self.nbytes))
        if host is not None and self.nbytes:
            check(lib().ed_memcpy_h2d(self.ptr, _ptr(host), self.nbytes))

    def to_host(self, dtype=None, shape=None):
        out = np.empty(shape if shape is not None else self.shape, dtype=dtype if dtype is not None else self.host_dtype)
        if out.nbytes:
            check(lib().ed_memcpy_d2h(_ptr(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            lib().ed_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _RawDevice:
    """a bare device pointer owned by somebody else (e.g. a cohort slot's fitted parameters)"""

    def __init__(self, ptr):
        self.ptr = C.c_void_p(ptr)


def _device_pointer(x, dtype, keep):
    """Return a c_void_p for x: a torch CUDA tensor (used in place), a DeviceArray, or host data
    (uploaded; the temporary is appended to `keep`)."""
    if isinstance(x, (DeviceArray, _RawDevice)):
        return x.ptr
    if hasattr(x, "data_ptr") and hasattr(x, "is_cuda"):
        if not x.is_cuda:
            x = x.cuda()
            keep.append(x)
        if not x.is_contiguous():
            raise ValueError("device tensors must be contiguous")
        want = {np.dtype(np.int32): ("torch.int32",), np.dtype(np.float64): ("torch.float64",),
                np.dtype(np.uint16): ("torch.uint16", "torch.int16")}[np.dtype(dtype)]     # (16-bit counts: the bit pattern is what counts)
        if str(x.dtype) not in want:
            raise ValueError("expected a %s tensor, got %s" % (want[0], x.dtype))
        return C.c_void_p(x.data_ptr())
    if np.dtype(dtype) == np.dtype(np.uint16):
        xa = np.asarray(x)
        if xa.dtype != np.uint16 and xa.size and (xa.min() < 0 or xa.max() > 65535):
            raise ValueError("16-bit counts (set_counts_bits(16) / counts_bits = 16) hold 0 .. 65535")
    d = DeviceArray(np.ascontiguousarray(x, dtype=dtype))
    keep.append(d)
    return d.ptr


def _is_device(x):
    return isinstance(x, (DeviceArray, _RawDevice)) or (hasattr(x, "data_ptr") and getattr(x, "is_cuda", False))


@contextlib.contextmanager
def _staged():
    """the `keep` list of one call: what _device_pointer uploads for it, and any DeviceArray the call appends itself, is freed on the way out"""
    keep = []
    try:
        yield keep
    finally:
        for d in keep:
            if isinstance(d, DeviceArray):
                d.free()


def _n_samples_of(phi):
    """the number of samples, from the per-sample dispersions: host data, a DeviceArray or a torch device tensor"""
    if isinstance(phi, DeviceArray) and phi.shape is None:
        return phi.nbytes // 8
    return int(np.size(phi)) if not _is_device(phi) else int(phi.shape[0])


def _check_counts_shape(x, n_exons, S, layout):
    """a host count matrix is (n_exons, S) with layout 0, (S, n_exons) with layout 1; a device array is taken as it is"""
    want = (n_exons, S) if not layout else (S, n_exons)
    if not _is_device(x) and np.shape(x) != want:
        raise ValueError("counts must have shape %s with layout %r, got %s" % (want, layout, np.shape(x)))


def _per_sample_mixture(mixture, n, device_ok=False):
    """None for a scalar mixture (today's path); otherwise the per-sample form: a float64[n] host array, checked here (one finite value
    per sample) before any device work -- or, with device_ok, a device array passed through as it is"""
    if device_ok and _is_device(mixture):
        return mixture
    if np.ndim(mixture) == 0:
        return None
    m = np.ascontiguousarray(mixture, dtype=np.float64)
    if m.ndim != 1 or m.size != n:
        raise ValueError("mixture / prop_tumor must be a scalar or one value per sample (%d), got shape %s" % (n, m.shape))
    if not np.all(np.isfinite(m)):
        raise ValueError("mixture / prop_tumor must be finite")
    return m


class Plan:
    """Exon design + HMM parameters (CallCNVs arguments, reference R/class_definition.R:261, :311).
    Exons must be ordered by (chromosome, position); chrom_off delimits the chromosomes."""

    def __init__(self, chrom_off, start, end, transition_probability=1e-4, expected_CNV_length=50000.0, device=0):
        self.chrom_off = _i32(chrom_off)
        self.start = _i32(start)
        self.end = _i32(end)
        self.n_exons = int(self.start.size)
        self.n_chrom = int(self.chrom_off.size - 1)
        self.transition_probability = float(transition_probability)
        self.expected_CNV_length = float(expected_CNV_length)
        self.handle = C.c_void_p()
        check(lib().ed_plan_create(C.byref(self.handle), int(device), self.n_exons, self.n_chrom, _ptr(self.chrom_off),
                                   _ptr(self.start), _ptr(self.end), self.transition_probability,
                                   self.expected_CNV_length))

    def posterior(self, loglik, n_samples, stream=None):
        """Forward-backward on a likelihood matrix (n_exons, 3, n_samples) -- columns deletion, normal, duplication; host data, a
        DeviceArray or a torch device tensor: the caller's own emissions are as good as a batch's.  Returns a Posterior."""
        return Posterior(self, loglik, int(n_samples), stream)

    def transition_score(self, loglik, n_samples, stream=None):
        """(log_evidence (n_chrom, n_samples), score (n_chrom, 2, n_samples)) of a likelihood matrix as Plan.posterior takes it:
        score[:, 0, :] is d log_evidence / d transition_probability, score[:, 1, :] d log_evidence / d expected_CNV_length of every
        (chromosome, sample) chain at this plan's values (include/exomedepth_amd.h: ed_plan_transition_score)."""
        S, E = int(n_samples), self.n_exons
        if not _is_device(loglik) and np.shape(loglik) != (E, 3, S):
            raise ValueError("loglik must have shape (%d, 3, %d), got %s" % (E, S, np.shape(loglik)))
        with _staged() as keep:
            ll = _device_pointer(loglik, np.float64, keep)
            work = DeviceArray(nbytes=E * 3 * S * 8)
            keep.append(work)
            return self._transition_score(ll, S, work, stream)

    def _transition_score(self, ll, S, work, stream=None):
        """... on a device pointer, with the caller's work array (n_exons * 3 * S doubles)"""
        Cn = self.n_chrom
        logev, score = DeviceArray(nbytes=Cn * S * 8), DeviceArray(nbytes=Cn * 2 * S * 8)
        try:
            check(lib().ed_plan_transition_score(self.handle, ll, S, work.ptr, logev.ptr, score.ptr, stream))
            check(lib().ed_synchronize(stream))
            return logev.to_host(np.float64, (Cn, S)), score.to_host(np.float64, (Cn, 2, S))
        finally:
            logev.free()
            score.free()

    def n_score_tables(self):
        """times this plan has built and uploaded its table of derivatives (0 before the first score request, 1 ever after)"""
        return int(lib().ed_plan_n_score_tables(self.handle))

    def mixture_profile(self, test, ref, phi, expected, grid, layout=0, stream=None):
        """The log-evidence of every (pair, chromosome) chain at every mixture of `grid`, from the counts (include/exomedepth_amd.h:
        ed_plan_mixture_profile): (G, n_chrom, S) float64.  test / ref: int32 counts of the tumours and their normals, (n_exons, S) with
        layout 0 or (S, n_exons) with layout 1; phi, expected: float64 (S,); host arrays, DeviceArrays or torch device tensors.  grid:
        (G, S), every pair its own mixtures, or (G,), the same for every pair; 1 <= G <= 16."""
        S = _n_samples_of(phi)
        if _is_device(grid):
            G = int(grid.shape[0])
            if tuple(grid.shape) != (G, S):
                raise ValueError("a device grid must have shape (G, %d), got %s" % (S, tuple(grid.shape)))
        else:
            grid = np.asarray(grid, dtype=np.float64)
            if grid.ndim == 1:
                grid = np.repeat(grid[:, None], S, axis=1)
            if grid.ndim != 2 or grid.shape[1] != S:
                raise ValueError("grid must have shape (G, %d) or (G,), got %s" % (S, grid.shape))
            G = int(grid.shape[0])
        for x in (test, ref):
            _check_counts_shape(x, self.n_exons, S, layout)
        with _staged() as keep:
            out = DeviceArray(nbytes=max(G, 1) * self.n_chrom * S * 8)
            keep.append(out)
            pt, pr = _device_pointer(test, np.int32, keep), _device_pointer(ref, np.int32, keep)
            pp, pe = _device_pointer(phi, np.float64, keep), _device_pointer(expected, np.float64, keep)
            pg = _device_pointer(grid, np.float64, keep)
            check(lib().ed_plan_mixture_profile(self.handle, pt, pr, int(layout), S, pp, pe, pg, G, out.ptr, C.c_void_p(stream or 0)))
            check(lib().ed_synchronize(C.c_void_p(stream or 0)))
            return out.to_host(np.float64, (G, self.n_chrom, S))

    def ratio_profile(self, rows, test, ref, phi, expected, ratios, layout=0, stream=None, tail=False):
        """The summed log-likelihood of every row's exons at every copy ratio of `ratios`, from the counts (include/exomedepth_amd.h:
        ed_plan_ratio_profile): (L (n_rows, G), ratios_used (n_rows, G)).  rows: records with sample, chrom, start_exon, end_exon (global
        0-based exon indices; Batch.calls(), or region_runs' rows with a `sample` field added).  test / ref: int32 counts, (n_exons, S)
        with layout 0 or (S, n_exons) with layout 1; phi, expected: float64 (S,); host arrays, DeviceArrays or torch device tensors.
        ratios: (G,), the same for every row, or (n_rows, G); 1 <= G <= 16.  A ratio r is evaluated at the dose mu = 2 (r - 1), and
        ratios_used = 1 + mu / 2 is the ratio that dose stands for; a ratio outside (0, 2] (or NaN) reads NaN.
        tail=True: (L, ratios_used, L_tail) -- L + L_tail is the double-double sum the kernel holds (ed_plan_ratio_profile_dd).  |L| is
        hundreds of times the difference of two of a row's values, so take a difference as (L_a - L_b) + (tail_a - tail_b).

        Genotyping known regions across a cohort needs nothing else:

            runs = region_runs(chromosome, start, end, regions)                  # one exon run per region
            runs = runs[runs["nexons"] > 0]
            rows = np.zeros(len(runs) * S, dtype=CALL_DTYPE)                     # regions x samples
            for k in ("chrom", "start_exon", "end_exon", "nexons"):
                rows[k] = np.repeat(runs[k], S)
            rows["sample"] = np.tile(np.arange(S), len(runs))
            L, r = plan.ratio_profile(rows, test, ref, phi, expected, COPY_RATIO_GRID)
            cn = copy_number_from_profile(r, L)["cn"].reshape(len(runs), S)"""
        rows = _ratio_rows(rows)
        n = int(rows.size)
        S = _n_samples_of(phi)
        ratios = np.asarray(ratios, dtype=np.float64)
        if ratios.ndim == 1:
            ratios = np.repeat(ratios[None, :], n, axis=0)
        if ratios.ndim != 2 or ratios.shape[0] != n:
            raise ValueError("ratios must have shape (G,) or (%d, G), got %s" % (n, ratios.shape))
        doses = np.ascontiguousarray((2.0 * (ratios - 1.0)).T)
        for x in (test, ref):
            _check_counts_shape(x, self.n_exons, S, layout)
        with _staged() as keep:
            pt, pr = _device_pointer(test, np.int32, keep), _device_pointer(ref, np.int32, keep)
            pp, pe = _device_pointer(phi, np.float64, keep), _device_pointer(expected, np.float64, keep)
            if tail:
                L, T = self._ratio_doses(rows, pt, pr, pp, pe, S, doses, layout, stream, tail=True)
                return np.ascontiguousarray(L.T), np.ascontiguousarray((1.0 + doses / 2.0).T), np.ascontiguousarray(T.T)
            L = self._ratio_doses(rows, pt, pr, pp, pe, S, doses, layout, stream)
            return np.ascontiguousarray(L.T), np.ascontiguousarray((1.0 + doses / 2.0).T)

    def _ratio_doses(self, rows, pt, pr, pp, pe, S, doses, layout=0, stream=None, tail=False):
        """... on device pointers and doses (G, n_rows): L (G, n_rows); tail=True: (L, L_tail)"""
        doses = np.ascontiguousarray(doses, dtype=np.float64)
        G, n = doses.shape
        out = np.empty((G, n), dtype=np.float64)
        if tail:
            rest = np.empty((G, n), dtype=np.float64)
            check(lib().ed_plan_ratio_profile_dd(self.handle, _ptr(rows) if n else None, n, pt, pr, int(layout), int(S), pp, pe,
                                                 _ptr(doses) if n else None, int(G), _ptr(out) if n else None, _ptr(rest) if n else None,
                                                 C.c_void_p(stream or 0)))
            return out, rest
        check(lib().ed_plan_ratio_profile(self.handle, _ptr(rows) if n else None, n, pt, pr, int(layout), int(S), pp, pe,
                                          _ptr(doses) if n else None, int(G), _ptr(out) if n else None, C.c_void_p(stream or 0)))
        return out

    def power_map(self, test, ref, phi, expected, mixture=1.0, layout=0, stream=None):
        """The detection-power map of the samples (include/exomedepth_amd.h: ed_plan_power_map): a PowerMap.  test / ref: int32 counts,
        (n_exons, S) with layout 0 or (S, n_exons) with layout 1 -- host arrays, or both DeviceArrays / torch device tensors; phi, expected:
        one value per sample (host); mixture: a scalar or one value per sample."""
        return PowerMap(self, test, ref, phi, expected, mixture, layout, stream)

    def quantile_map(self, test, ref, phi, expected, probs=(0.025, 0.975), layout=0, stream=None):
        """The quantile map of the samples (include/exomedepth_amd.h: ed_plan_quantile_map): a QuantileMap.  Counts, phi and expected as
        power_map takes them; probs: 1 .. 16 probabilities inside (0, 1), strictly ascending."""
        return QuantileMap(self, test, ref, phi, expected, probs, layout, stream)

    def simulate(self, test, ref, phi, expected, seed, replicate=0, sample0=0, layout=0, stream=None, plant=None):
        """A cohort's counts redrawn under its own fitted normal state (include/exomedepth_amd.h: ed_plan_simulate): every cell keeps its
        total n = test + ref, test* is the draw from BetaBinomial(n; phi_s, expected_s) at the uniform of the counter (exon, sample0 + s,
        replicate, 0) under `seed`, ref* = n - test*.  test / ref: int32 counts, (n_exons, S) with layout 0 or (S, n_exons) with layout 1,
        host arrays, DeviceArrays or torch device tensors; phi, expected: one value per sample (host).  Returns SimulatedCounts: the pair
        (test*, ref*) of DeviceArrays in the input's layout -- they go straight into Batch.fit / Batch.run / Cohort.submit -- with .stats().
        A seed reproduces a sample's draws alone or in any slab (pass the slab's first global sample index as sample0), in either layout.
        plant = (rows, ratio): the cells of those rows are then redrawn at the proportion e c / (e c + 1 - e) of copy ratio c, on stream 1
        (rows: records with sample, start_exon, end_exon, or (chrom, first, last) triples for every sample)."""
        return _simulate(self, test, ref, phi, expected, seed, replicate, sample0, layout, stream, plant)

    def close(self):
        if self.handle:
            lib().ed_plan_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Posterior:
    """Device-resident result of Plan.posterior: the backward messages, the log posterior of deletion / duplication per exon and the
    log-evidence of every (sample, chromosome) chain (include/exomedepth_amd.h: ed_plan_posterior)."""

    def __init__(self, plan, loglik, n_samples, stream=None):
        self.plan, self.n_samples, self.stream = plan, n_samples, stream
        E, Cn, S = plan.n_exons, plan.n_chrom, n_samples
        if not _is_device(loglik) and np.shape(loglik) != (E, 3, S):
            raise ValueError("loglik must have shape (%d, 3, %d), got %s" % (E, S, np.shape(loglik)))
        self._keep = []
        self._ll = _device_pointer(loglik, np.float64, self._keep)
        if _is_device(loglik):
            self._keep.append(loglik)
        self._work = DeviceArray(nbytes=E * 3 * S * 8)
        self._logpost = DeviceArray(nbytes=E * 2 * S * 8)
        self._logev = DeviceArray(nbytes=Cn * S * 8)
        check(lib().ed_plan_posterior(plan.handle, self._ll, S, self._work.ptr, self._logpost.ptr, self._logev.ptr, stream))
        check(lib().ed_synchronize(stream))

    def log_posterior(self):
        """(n_exons, 2, n_samples): [:,0,:] deletion, [:,1,:] duplication"""
        return self._logpost.to_host(np.float64, (self.plan.n_exons, 2, self.n_samples))

    def posterior(self):
        return np.exp(self.log_posterior())

    def log_evidence(self):
        """(n_chrom, n_samples)"""
        return self._logev.to_host(np.float64, (self.plan.n_chrom, self.n_samples))

    def beta(self):
        """(n_exons, 3, n_samples) backward log-messages, rows in HMM state order: normal, deletion, duplication"""
        return self._work.to_host(np.float64, (self.plan.n_exons, 3, self.n_samples))

    def device_pointers(self):
        return {"work": self._work.ptr.value, "logpost": self._logpost.ptr.value, "log_evidence": self._logev.ptr.value}

    def call_posterior(self, calls):
        """post_mean, post_min, log_p_all, log_evidence of call rows (a CALL_DTYPE array)"""
        calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
        out = np.zeros(calls.size, dtype=CALL_POST_DTYPE)
        check(lib().ed_plan_call_posterior(self.plan.handle, _ptr(calls), calls.size, self._ll, self.n_samples, self._work.ptr,
                                           self._logpost.ptr, self._logev.ptr, _ptr(out), self.stream))
        return out

    def call_bounds(self, calls, level=0.95):
        """breakpoint credible intervals of call rows (a CALL_DTYPE array) at `level`: a CALL_BOUNDS_DTYPE array
        (include/exomedepth_amd.h: ed_plan_call_bounds)"""
        calls = np.ascontiguousarray(calls, dtype=CALL_DTYPE)
        out = np.zeros(calls.size, dtype=CALL_BOUNDS_DTYPE)
        check(lib().ed_plan_call_bounds(self.plan.handle, _ptr(calls), calls.size, self._ll, self.n_samples, self._work.ptr,
                                        self._logpost.ptr, float(level), _ptr(out), self.stream))
        return out

    def free(self):
        for d in (self._work, self._logpost, self._logev):
            d.free()
        self._keep = []


class Batch:
    """Device working set for n_samples samples of a plan.  Count matrices are int32
    [n_exons][n_samples] (sample-minor)."""

    STAGES = ("sample_consts", "emissions", "viterbi", "call_table", "fit")

    def __init__(self, plan, n_samples):
        self.plan = plan
        self.n_samples = int(n_samples)
        self.handle = C.c_void_p()
        self._keep_run = []   # device temporaries uploaded for the last run*(): call_info() / verify read the run's inputs
        self._keep_fit = []   # ... for the last fit*() (outputs may be read by the caller after the call)
        check(lib().ed_batch_create(C.byref(self.handle), plan.handle, self.n_samples))

    _owned = True

    @classmethod
    def _view(cls, plan, n_samples, handle):
        """a Batch interface on a batch object owned by somebody else (a Cohort's slot): close() leaves it alone"""
        b = cls.__new__(cls)
        b.plan, b.n_samples, b.handle = plan, int(n_samples), C.c_void_p(handle)
        b._keep_run, b._keep_fit, b._owned = [], [], False
        return b

    def close(self):
        if self.handle and self._owned:
            lib().ed_batch_destroy(self.handle)
        self.handle = C.c_void_p()
        self._keep_run = []
        self._keep_fit = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def enable_timing(self, on=True):
        check(lib().ed_batch_enable_timing(self.handle, 1 if on else 0))

    def set_fused(self, fused=True):
        """fused=True: emissions + Viterbi as one kernel (minimal HBM traffic); default is the two-kernel path."""
        check(lib().ed_batch_set_fused(self.handle, 1 if fused else 0))

    def keep_loglik(self, keep=True):
        """Keep (default) or drop the (n_exons, 3, n_samples) likelihood matrix -- 24 bytes per cell of HBM."""
        check(lib().ed_batch_keep_loglik(self.handle, 1 if keep else 0))

    def set_async_tail(self, on=True):
        """on: run() leaves the Viterbi tail and the call table on streams of the batch instead of joining them into the
        caller's stream (two batches used alternately then overlap; see ed_batch_set_async_tail)."""
        check(lib().ed_batch_set_async_tail(self.handle, 1 if on else 0))

    def set_viterbi_overlap(self, on=True):
        """on (default): chains of a chromosome group run underneath the emissions of the next groups; off: all emissions,
        then all chains (what a pipeline of batches wants, see ed_batch_set_viterbi_overlap)"""
        check(lib().ed_batch_set_viterbi_overlap(self.handle, 1 if on else 0))

    def wait(self, stream=None):
        """make `stream` wait (on the device) for the last run() of this batch, asynchronous tail included"""
        check(lib().ed_batch_wait(self.handle, C.c_void_p(stream or 0)))

    def set_fit_histograms(self, on=True):
        """fit(): iterate on per-sample count histograms (default; True / 1: geometry picked from the data's depth,
        8 / 4 / 2: that geometry) or per cell on every pass (False / 0)."""
        check(lib().ed_batch_set_fit_histograms(self.handle, int(on)))

    @property
    def n_emit_launches(self):
        """emission-kernel launches per run (overlap groups; 1 in fused mode)"""
        return int(lib().ed_batch_n_emit_launches(self.handle))

    def fit(self, test, ref, phi_out, expected_out, stream=None, by=1):
        """Per-sample beta-binomial fit (phi, expected) -- counterpart of aod::betabin at reference
        R/class_definition.R:118.  phi_out/expected_out: device float64[n_samples].
        by > 1: fit on exons 0, by, 2*by, ... only (scalar subset.for.speed = n  <=>  by = n_exons // n, :107-113)."""
        keep = []
        cdt = getattr(self, "_cdt", np.int32)
        pt = _device_pointer(test, cdt, keep)
        pr = _device_pointer(ref, cdt, keep)
        pp = _device_pointer(phi_out, np.float64, keep)
        pe = _device_pointer(expected_out, np.float64, keep)
        self._keep_fit = keep
        check(lib().ed_batch_fit_subset(self.handle, pt, pr, int(by), pp, pe, C.c_void_p(stream or 0)))

    def fit_unconverged(self):
        """(number of samples whose last fit() did not converge, first such sample or -1); synchronises the fit"""
        n, first = C.c_int64(0), C.c_int32(-1)
        check(lib().ed_batch_fit_n_unconverged(self.handle, C.byref(n), C.byref(first)))
        return n.value, first.value

    def run(self, test, ref, phi, expected, mixture=1.0, stream=None):
        """Emissions + Viterbi + call table.  Arguments may be torch CUDA tensors (used in place),
        DeviceArrays, or host arrays (uploaded).  Asynchronous on `stream`."""
        keep = []
        cdt = getattr(self, "_cdt", np.int32)
        pt = _device_pointer(test, cdt, keep)
        pr = _device_pointer(ref, cdt, keep)
        pp = _device_pointer(phi, np.float64, keep)
        pe = _device_pointer(expected, np.float64, keep)
        self._keep_run = keep  # keep temporaries alive until the next run
        check(lib().ed_batch_run(self.handle, pt, pr, pp, pe, float(mixture), C.c_void_p(stream or 0)))

    def set_mixture(self, mixture):
        """One mixture per sample (ed_batch_set_mixture): matched tumour / normal pairs, each at its own tumour fraction.  A host
        float64[n_samples] (uploaded) or a device array (used in place); the batch keeps it alive.  None turns it off.  While it is set,
        the `mixture` argument of run*() and verify_emissions*() is ignored."""
        if mixture is None:
            check(lib().ed_batch_set_mixture(self.handle, None))
            self._mix = None
            return
        m = _per_sample_mixture(mixture, self.n_samples, device_ok=True)
        if m is None:
            raise ValueError("set_mixture takes one value per sample (use the `mixture` argument of run() for one value)")
        keep = []
        p = _device_pointer(m, np.float64, keep)
        check(lib().ed_batch_set_mixture(self.handle, p))
        self._mix = keep + [mixture]

    @property
    def fit_bins_form(self):
        """form the last fit_bins took: 1 = count histograms, 0 = per cell (set_fit_histograms(0), or data beyond the bins)"""
        return int(lib().ed_batch_fit_bins_form(self.handle))

    def fit_bins_unconverged(self):
        """samples the last depth-binned fit left short of its tolerance (the binned Newton's own flags)"""
        n = C.c_int64(0)
        check(lib().ed_batch_fit_bins_n_unconverged(self.handle, C.byref(n)))
        return n.value

    def fit_bins(self, test, ref, phi_bins, phi_bins_out, edges_out, expected_out, stream=None):
        """phi.bins > 1 (reference R/class_definition.R:120-147): per sample the depth levels of the reference
        counts (edges_out: (phi_bins + 1, n_samples) complete.bins), one dispersion per level (phi_bins_out:
        (phi_bins, n_samples)) and the common expected proportion.  Raises EdError("Binning did not happen
        properly ...") like the reference's stop() when a level is empty.  Synchronous."""
        keep = []
        pt = _device_pointer(test, np.int32, keep)
        pr = _device_pointer(ref, np.int32, keep)
        pp = _device_pointer(phi_bins_out, np.float64, keep)
        pg = _device_pointer(edges_out, np.float64, keep)
        pe = _device_pointer(expected_out, np.float64, keep)
        self._keep_fit = keep
        check(lib().ed_batch_fit_bins(self.handle, pt, pr, int(phi_bins), pp, pg, pe, C.c_void_p(stream or 0)))

    def run_bins(self, test, ref, phi_bins, phi_bins_dev, edges_dev, expected, mixture=1.0, stream=None):
        """run() with the per-exon dispersion phi.linear of the phi.bins > 1 model (interpolated on the fly)."""
        keep = []
        pt = _device_pointer(test, np.int32, keep)
        pr = _device_pointer(ref, np.int32, keep)
        pp = _device_pointer(phi_bins_dev, np.float64, keep)
        pg = _device_pointer(edges_dev, np.float64, keep)
        pe = _device_pointer(expected, np.float64, keep)
        self._keep_run = keep
        check(lib().ed_batch_run_bins(self.handle, pt, pr, int(phi_bins), pp, pg, pe, float(mixture), C.c_void_p(stream or 0)))

    def phi_linear(self, ref, phi_bins, phi_bins_dev, edges_dev):
        """(n_exons, n_samples) host array: the S4 `phi` slot of the phi.bins > 1 model."""
        keep = []
        pr = _device_pointer(ref, np.int32, keep)
        pp = _device_pointer(phi_bins_dev, np.float64, keep)
        pg = _device_pointer(edges_dev, np.float64, keep)
        out = DeviceArray(np.zeros((self.plan.n_exons, self.n_samples)))
        check(lib().ed_batch_phi_linear(self.handle, pr, int(phi_bins), pp, pg, out.ptr, None))
        check(lib().ed_synchronize(None))
        return out.to_host().reshape(self.plan.n_exons, self.n_samples)

    def _cov_matrix(self, X):
        """(matrix, K) of the covariates: a host array (n_exons, K), a DeviceArray made from one, or a torch CUDA tensor."""
        if hasattr(X, "data_ptr") or hasattr(X, "ptr"):
            return X, int(X.shape[1])
        X = np.ascontiguousarray(X, dtype=np.float64).reshape(self.plan.n_exons, -1)
        return X, int(X.shape[1])

    def fit_cov(self, test, ref, X, beta_out, phi_out, stream=None):
        """Mean model with covariates (`data` + `formula ~ x1 + ...`, reference R/class_definition.R:86-118): X is the
        (n_exons, K) covariate matrix shared by the samples; beta_out (K + 1, n_samples), phi_out (n_samples).  Synchronous."""
        keep = []
        pt = _device_pointer(test, np.int32, keep)
        pr = _device_pointer(ref, np.int32, keep)
        X, K = self._cov_matrix(X)
        px = _device_pointer(X, np.float64, keep) if K > 0 else None
        pb = _device_pointer(beta_out, np.float64, keep)
        pp = _device_pointer(phi_out, np.float64, keep)
        self._keep_fit = keep
        check(lib().ed_batch_fit_cov(self.handle, pt, pr, px, K, pb, pp, C.c_void_p(stream or 0)))

    def run_cov(self, test, ref, X, beta, phi, mixture=1.0, stream=None):
        """run() with expected = plogis(X beta) per exon."""
        keep = []
        pt = _device_pointer(test, np.int32, keep)
        pr = _device_pointer(ref, np.int32, keep)
        X, K = self._cov_matrix(X)
        px = _device_pointer(X, np.float64, keep) if K > 0 else None
        pb = _device_pointer(beta, np.float64, keep)
        pp = _device_pointer(phi, np.float64, keep)
        self._keep_run = keep
        check(lib().ed_batch_run_cov(self.handle, pt, pr, px, K, pb, pp, float(mixture), C.c_void_p(stream or 0)))

    def expected_cov(self, X, beta):
        """(n_exons, n_samples) host array: the S4 `expected` slot, fitted(mod) = plogis(X beta)."""
        keep = []
        X, K = self._cov_matrix(X)
        px = _device_pointer(X, np.float64, keep) if K > 0 else None
        pb = _device_pointer(beta, np.float64, keep)
        out = DeviceArray(np.zeros((self.plan.n_exons, self.n_samples)))
        check(lib().ed_batch_expected_cov(self.handle, px, K, pb, out.ptr, None))
        check(lib().ed_synchronize(None))
        return out.to_host().reshape(self.plan.n_exons, self.n_samples)

    # ---- results ----
    def n_calls(self):
        n = C.c_int64(0)
        check(lib().ed_batch_n_calls(self.handle, C.byref(n)))
        return n.value

    def n_gsl_errors(self):
        n = C.c_int64(0)
        check(lib().ed_batch_n_gsl_errors(self.handle, C.byref(n)))
        return n.value

    def calls(self):
        n = self.n_calls()
        out = np.zeros(n, dtype=CALL_DTYPE)
        check(lib().ed_batch_copy_calls(self.handle, _ptr(out), n))
        return out

    def call_info(self):
        """BF, reads.expected, reads.observed, reads.ratio of every call (R/class_definition.R:379-405)."""
        n = self.n_calls()
        out = np.zeros(n, dtype=CALL_INFO_DTYPE)
        check(lib().ed_batch_copy_call_info(self.handle, _ptr(out), n))
        return out

    def path(self):
        out = np.empty((self.plan.n_exons, self.n_samples), dtype=np.uint8)
        check(lib().ed_batch_copy_path(self.handle, _ptr(out)))
        return out

    def posterior(self, log=False):
        """(n_exons, 2, n_samples): posterior probability of [:,0,:] deletion and [:,1,:] duplication at every exon of the last run
        (log=True: its logarithm, as the device holds it).  Forward-backward on the run's likelihood matrix, made on the first request."""
        out = np.empty((self.plan.n_exons, 2, self.n_samples), dtype=np.float64)
        check(lib().ed_batch_copy_posterior(self.handle, _ptr(out)))
        return out if log else np.exp(out)

    def log_evidence(self):
        """(n_chrom, n_samples): log-probability of every chain's observations under the HMM (0 for an empty chromosome)"""
        out = np.empty((self.plan.n_chrom, self.n_samples), dtype=np.float64)
        check(lib().ed_batch_copy_log_evidence(self.handle, _ptr(out)))
        return out

    def call_posterior(self):
        """post_mean, post_min, log_p_all, log_evidence of every call (row i belongs to row i of calls())"""
        n = self.n_calls()
        out = np.zeros(n, dtype=CALL_POST_DTYPE)
        check(lib().ed_batch_copy_call_posterior(self.handle, _ptr(out), n))
        return out

    def posterior_ms(self):
        """with enable_timing(): dict(backward, forward, call_post) in ms of the last run's posterior request (0: not timed)"""
        ms = (C.c_float * 3)()
        check(lib().ed_batch_posterior_ms(self.handle, ms))
        return dict(zip(("backward", "forward", "call_post"), (float(x) for x in ms)))

    def call_bounds(self, level=0.95):
        """breakpoint credible intervals of every call at `level` (row i belongs to row i of calls()): anchor_exon, start_lo <= start_hi
        <= anchor_exon <= end_lo <= end_hi (global 0-based exon indices), flags, log_anchor, log_keep_start, log_keep_end.  One kernel
        behind the posterior's passes, which are made on the first request after a run."""
        n = self.n_calls()
        out = np.zeros(n, dtype=CALL_BOUNDS_DTYPE)
        check(lib().ed_batch_copy_call_bounds(self.handle, float(level), _ptr(out), n))
        return out

    def call_bounds_ms(self):
        """with enable_timing(): milliseconds of k_call_bounds in the last call_bounds() of this run (0: not timed)"""
        ms = C.c_float(0)
        check(lib().ed_batch_call_bounds_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def call_ratio_profile(self, ratios, tail=False):
        """(L (n_calls, G), ratios_used (n_calls, G)): the copy-ratio profile of every call of the last run() (row i belongs to row i of
        calls()), as Plan.ratio_profile on the run's own counts, phi and expected.  ratios: (G,) or (n_calls, G), 1 <= G <= 16.  Not
        available after run_bins() / run_cov().  tail=True: (L, ratios_used, L_tail), L + L_tail the double-double sums: with ratios
        (0.5, 1, 1.5), log10(e) ((L[:, k] - L[:, 1]) + (L_tail[:, k] - L_tail[:, 1])) at the call's type is call_info()'s BF_raw to a
        few units in the last place, which the rounded values' difference alone is not (|L| is hundreds of times the difference)."""
        n = self.n_calls()
        ratios = np.asarray(ratios, dtype=np.float64)
        if ratios.ndim == 1:
            ratios = np.repeat(ratios[None, :], n, axis=0)
        if ratios.ndim != 2 or ratios.shape[0] != n:
            raise ValueError("ratios must have shape (G,) or (%d, G), got %s" % (n, ratios.shape))
        doses = np.ascontiguousarray((2.0 * (ratios - 1.0)).T)
        if tail:
            L, T = self._call_ratio_doses(doses, tail=True)
            return np.ascontiguousarray(L.T), np.ascontiguousarray((1.0 + doses / 2.0).T), np.ascontiguousarray(T.T)
        L = self._call_ratio_doses(doses)
        return np.ascontiguousarray(L.T), np.ascontiguousarray((1.0 + doses / 2.0).T)

    def _call_ratio_doses(self, doses, tail=False):
        """... on doses (G, n_calls): L (G, n_calls); tail=True: (L, L_tail)"""
        doses = np.ascontiguousarray(doses, dtype=np.float64)
        G, n = doses.shape
        out = np.empty((G, n), dtype=np.float64)
        if tail:
            rest = np.empty((G, n), dtype=np.float64)
            check(lib().ed_batch_copy_call_ratio_profile_dd(self.handle, _ptr(doses) if n else None, int(G), _ptr(out) if n else None,
                                                            _ptr(rest) if n else None, n))
            return out, rest
        check(lib().ed_batch_copy_call_ratio_profile(self.handle, _ptr(doses) if n else None, int(G), _ptr(out) if n else None, n))
        return out

    def call_ratio_ms(self):
        """with enable_timing(): milliseconds of the profile's kernels in the last call_ratio_profile() of this run (0: not timed)"""
        ms = C.c_float(0)
        check(lib().ed_batch_call_ratio_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def n_posterior_passes(self):
        """times the forward-backward passes have been enqueued on this batch (a second request after a run launches nothing)"""
        return int(lib().ed_batch_n_posterior_passes(self.handle))

    def transition_score(self):
        """(log_evidence (n_chrom, n_samples), score (n_chrom, 2, n_samples)) of the last run: score[:, 0, :] is
        d log_evidence / d transition_probability, score[:, 1, :] d log_evidence / d expected_CNV_length of every chain at the plan's
        values.  One more pass behind the posterior's, made on the first request."""
        out = np.empty((self.plan.n_chrom, 2, self.n_samples), dtype=np.float64)
        check(lib().ed_batch_copy_transition_score(self.handle, _ptr(out)))
        return self.log_evidence(), out

    def n_score_passes(self):
        """times the score pass has been enqueued on this batch (a second request after a run launches nothing)"""
        return int(lib().ed_batch_n_score_passes(self.handle))

    def transition_score_ms(self):
        """with enable_timing(): milliseconds of the last run's score pass (0: not timed)"""
        ms = C.c_float(0)
        check(lib().ed_batch_transition_score_ms(self.handle, C.byref(ms)))
        return float(ms.value)

    def loglik(self):
        """(n_exons, 3, n_samples): [:,0,:] deletion, [:,1,:] normal, [:,2,:] duplication."""
        out = np.empty((self.plan.n_exons, 3, self.n_samples), dtype=np.float64)
        check(lib().ed_batch_copy_loglik(self.handle, _ptr(out)))
        return out

    def verify_emissions(self, test, ref, phi, expected, mixture=1.0, cap=16):
        """Device-side self-check of the last run()'s likelihood matrix: every cell re-evaluated with the reference's own
        per-cell loop (no hoisting, tables or binning) and compared bit for bit.  Arguments: what run() was given.
        Returns (values compared, values that differ, first mismatches as a list of dicts)."""
        keep = []
        pt = _device_pointer(test, np.int32, keep)
        pr = _device_pointer(ref, np.int32, keep)
        pp = _device_pointer(phi, np.float64, keep)
        pe = _device_pointer(expected, np.float64, keep)
        first = (_lib.EdEmitMismatch * max(int(cap), 1))()
        ncmp, nbad = C.c_int64(0), C.c_int64(0)
        check(lib().ed_batch_verify_emissions(self.handle, pt, pr, pp, pe, float(mixture), C.byref(ncmp), C.byref(nbad),
                                              C.cast(first, C.c_void_p), int(cap)))
        rec = [{f: getattr(first[i], f) for f in ("exon", "sample", "state", "observed", "total", "got", "want")}
               for i in range(min(int(cap), nbad.value))]
        return ncmp.value, nbad.value, rec

    def set_emit_mode(self, mode, cap_obs=None, cap_ref=None, reach=None, tails=None):
        """mode 0 / "strict": GSL's arithmetic operation for operation (default); 1 / "tables": log-gamma difference tables per
        (sample, state) -- three gathers and a sum per cell, ~1e-14 relative (see ed_batch_set_emit_mode)."""
        m = {"strict": 0, "tables": 1, "tables-sm": 2}.get(mode, mode)
        if cap_obs is not None or cap_ref is not None or reach is not None:
            check(lib().ed_batch_set_emit_tables(self.handle, int(cap_obs or 4096), int(cap_ref or 32768), float(reach or 8.0)))
        if tails is not None:
            self.set_emit_tails(tails)
        check(lib().ed_batch_set_emit_mode(self.handle, int(m)))

    def set_counts_layout(self, layout):
        """0: device count matrices are [n_exons][n_samples]; 1: [n_samples][n_exons] (R's column-major matrix; fit + emit mode 2)"""
        check(lib().ed_batch_set_counts_layout(self.handle, int(layout)))

    def set_counts_bits(self, bits):
        """32 (default): int32 device counts; 16: uint16, (n_samples, n_exons) -- counts_layout 1 + emit mode 2 only (ed_batch_set_counts_bits)"""
        check(lib().ed_batch_set_counts_bits(self.handle, int(bits)))
        self._cdt = np.uint16 if int(bits) == 16 else np.int32

    def verify_emissions_tol(self, test, ref, phi, expected, mixture=1.0, rel_tol=1e-10, abs_tol=1e-12, cap=16):
        """verify_emissions with a tolerance: returns a dict(compared, beyond, max_rel, max_abs, first)."""
        keep = []
        cdt = getattr(self, "_cdt", np.int32)
        pt = _device_pointer(test, cdt, keep)
        pr = _device_pointer(ref, cdt, keep)
        pp = _device_pointer(phi, np.float64, keep)
        pe = _device_pointer(expected, np.float64, keep)
        first = (_lib.EdEmitMismatch * max(int(cap), 1))()
        ncmp, nbad, mr, ma = C.c_int64(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        check(lib().ed_batch_verify_emissions_tol(self.handle, pt, pr, pp, pe, float(mixture), float(rel_tol), float(abs_tol), C.byref(ncmp),
                                                  C.byref(nbad), C.byref(mr), C.byref(ma), C.cast(first, C.c_void_p), int(cap)))
        rec = [{f: getattr(first[i], f) for f in ("exon", "sample", "state", "observed", "total", "got", "want")}
               for i in range(min(int(cap), nbad.value))]
        return {"compared": ncmp.value, "beyond": nbad.value, "max_rel": mr.value, "max_abs": ma.value, "first": rec}

    def emit_tables(self, sample):
        """emit mode 1: (Ly, Lr, obs table [Ly][3], ref table [Lr][3], tot table [Ly + Lr][3]) of one sample, as the last run built them"""
        dims = (C.c_int32 * 2)()
        check(lib().ed_batch_copy_emit_tables(self.handle, int(sample), dims, None, 0))
        ly, lr = int(dims[0]), int(dims[1])
        ent = np.empty((2 * (ly + lr), 3))
        if ent.size:
            check(lib().ed_batch_copy_emit_tables(self.handle, int(sample), dims, _ptr(ent), ent.shape[0]))
        return ly, lr, ent[:ly], ent[ly:ly + lr], ent[ly + lr:]

    def n_cold_cells(self):
        n = C.c_int64(0)
        check(lib().ed_batch_n_cold_cells(self.handle, C.byref(n)))
        return n.value

    TABLE_STATS = ("n_cold_cells", "n_samples_without_tables", "cold_list_overflow", "n_cells_without_tables")

    def table_stats(self):
        """table-driven modes: what the last run left to the strict arithmetic (ed_batch_table_stats)"""
        v = (C.c_int64 * 4)()
        check(lib().ed_batch_table_stats(self.handle, v))
        return dict(zip(self.TABLE_STATS, (int(x) for x in v)))

    def table_dims(self, sample):
        """(Ly, Lr, Tm1, w) of one sample in the last run (ed_batch_copy_table_dims): w = N0 of the ref = 0 rule, or the reason when Ly = 0"""
        d = (C.c_int32 * 4)()
        check(lib().ed_batch_copy_table_dims(self.handle, int(sample), d))
        return tuple(int(x) for x in d)

    def table_windows(self, sample):
        """(n1, n2, n3, tail) of one sample in the last run (ed_batch_copy_table_windows): the LDS windows of the sample-major table mode and whether
        the sample is a tail sample (Stirling's series beyond the windows)"""
        d = (C.c_int32 * 4)()
        check(lib().ed_batch_copy_table_windows(self.handle, int(sample), d))
        return tuple(int(x) for x in d)

    def set_emit_tails(self, on=True):
        check(lib().ed_batch_set_emit_tails(self.handle, int(bool(on))))

    def device_pointers(self):
        L = lib()
        return {"loglik": L.ed_batch_loglik(self.handle), "path": L.ed_batch_path(self.handle),
                "calls": L.ed_batch_calls(self.handle)}

    def stage_ms_total(self):
        """(dict of stage -> summed milliseconds, timed runs, timed fits) since enable_timing()"""
        ms = (C.c_double * 5)()
        nr, nf = C.c_int64(0), C.c_int64(0)
        check(lib().ed_batch_stage_ms_total(self.handle, ms, C.byref(nr), C.byref(nf)))
        return dict(zip(self.STAGES, [float(v) for v in ms])), nr.value, nf.value

    def stage_ms(self):
        ms = (C.c_float * 5)()
        check(lib().ed_batch_stage_ms(self.handle, ms))
        return dict(zip(self.STAGES, [float(v) for v in ms]))


class PinnedArray:
    """A numpy array in pinned host memory (ed_host_alloc): the DMA engine reads it in place, no staging copy."""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        self.ptr = C.c_void_p()
        check(lib().ed_host_alloc(C.byref(self.ptr), self.nbytes))
        buf = (C.c_char * max(self.nbytes, 1)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=self.dtype, count=int(np.prod(self.shape))).reshape(self.shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().ed_host_free(self.ptr)
            self.ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _host_slab(a, layout):
    """a host count slab in the memory layout the C entry reads: layout 0 -- rows of consecutive samples, any row pitch (a window of
    the first columns of a wider matrix stays in place); layout 1 -- dense (n, n_exons).  Anything else (Fortran order, strided
    columns, negative strides) is copied into that form rather than uploaded as it lies."""
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("a count slab is a 2-d array")
    if layout == 0:
        ok = (a.shape[1] <= 1 or a.strides[1] == a.itemsize) and a.strides[0] % a.itemsize == 0 and (a.shape[0] <= 1 or a.strides[0] >= a.shape[1] * a.itemsize)
        return a if ok or a.size == 0 else np.ascontiguousarray(a)
    if layout == 1:
        return a if a.flags.c_contiguous else np.ascontiguousarray(a)
    raise ValueError("layout is 0 ((n_exons, n) arrays) or 1 ((n, n_exons) arrays = R's column-major matrix)")


class Cohort:
    """Slabs of a cohort through the library's pipeline (ed_cohort_*): the loop of reference vignette/vignette.Rnw:390-431
    -- new('ExomeDepth') + CallCNVs() per sample -- for slabs of samples, on streams the library owns.

    submit() / submit_host() return a ticket; batch(ticket) gives a Batch view holding that slab's results (valid until
    `slabs_in_flight` further slabs have been submitted).  run_host() does a whole host-resident cohort."""

    STAGES = Batch.STAGES

    def __init__(self, plan, slab_samples, slabs_in_flight=2, **options):
        self.plan = plan
        self.slab_samples = int(slab_samples)
        self.slabs_in_flight = int(slabs_in_flight)
        self.handle = C.c_void_p()
        self._keep = {}
        check(lib().ed_cohort_create(C.byref(self.handle), plan.handle, self.slab_samples, self.slabs_in_flight))
        self.phi_bins = 1
        for k, v in options.items():
            self.set_option(k, v)

    def set_option(self, name, value):
        check(lib().ed_cohort_set_option(self.handle, name.encode(), float(value)))
        if name == "counts_bits":
            self._counts_bits = int(value)
        if name == "phi_bins":
            self.phi_bins = int(value)

    def close(self):
        if self.handle:
            lib().ed_cohort_destroy(self.handle)
            self.handle = C.c_void_p()
        self._keep = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return lib().ed_cohort_stream(self.handle)

    @property
    def n_emit_launches(self):
        return int(lib().ed_cohort_n_emit_launches(self.handle))

    def submit(self, test, ref, phi=None, expected=None, mixture=1.0, ready_stream=None, n_samples=None):
        """one slab, counts on the device: (n_exons, n) int32 torch CUDA tensors / DeviceArrays (host arrays are uploaded
        synchronously first -- use submit_host for the staged path).  phi / expected: device float64[n] or None (fit).
        mixture: a scalar, or one value per sample of the slab (host float64[n], uploaded; or a device array: ed_cohort_submit_mix)."""
        keep = []
        if n_samples is None:
            n_samples = int(test.shape[1])
        mix = _per_sample_mixture(mixture, int(n_samples), device_ok=True)
        cdt = np.uint16 if getattr(self, "_counts_bits", 32) == 16 else np.int32
        pt = _device_pointer(test, cdt, keep)
        pr = _device_pointer(ref, cdt, keep)
        pp = _device_pointer(phi, np.float64, keep) if phi is not None else None
        pe = _device_pointer(expected, np.float64, keep) if expected is not None else None
        t = C.c_int64(-1)
        if mix is None:
            check(lib().ed_cohort_submit(self.handle, pt, pr, int(n_samples), pp, pe, float(mixture), C.c_void_p(ready_stream or 0), C.byref(t)))
        else:
            pm = _device_pointer(mix, np.float64, keep)
            check(lib().ed_cohort_submit_mix(self.handle, pt, pr, int(n_samples), pp, pe, pm, C.c_void_p(ready_stream or 0), C.byref(t)))
        # the slab's counts are read until its results have been collected (the call decoration): keep them alive that long
        self._keep[t.value % self.slabs_in_flight] = keep + [test, ref, phi, expected, mixture]
        return t.value

    def submit_host(self, test, ref, layout, phi=None, expected=None, mixture=1.0, n_samples=None, row_stride=None):
        """one slab from host memory.  layout 0: (n_exons, n) sample-minor arrays (or a window of the first n columns of a wider
        matrix: pass n_samples and row_stride); layout 1: R's column-major n_exons x n matrix, i.e. a C-contiguous (n, n_exons)
        array.  dtype int32 or uint16 (the 16-bit wire format).  numpy arrays or PinnedArray.array views."""
        test, ref = _host_slab(test, layout), _host_slab(ref, layout)
        if test.dtype != ref.dtype or test.dtype not in (np.dtype(np.int32), np.dtype(np.uint16)):
            raise ValueError("test and ref must both be int32 or both uint16")
        wire = test.dtype.itemsize
        if n_samples is None:
            n_samples = int(test.shape[1] if layout == 0 else test.shape[0])
        if row_stride is None:
            if layout == 0 and test.strides[0] != ref.strides[0]:
                raise ValueError("test and ref windows must share their row stride")
            row_stride = int(test.strides[0] // wire) if layout == 0 else 0
        keep = []
        pp = _device_pointer(phi, np.float64, keep) if phi is not None else None
        pe = _device_pointer(expected, np.float64, keep) if expected is not None else None
        t = C.c_int64(-1)
        check(lib().ed_cohort_submit_host(self.handle, C.c_void_p(test.ctypes.data), C.c_void_p(ref.ctypes.data), int(n_samples),
                                          int(layout), int(wire), int(row_stride), pp, pe, float(mixture), C.byref(t)))
        self._keep[t.value % self.slabs_in_flight] = keep + [test, ref]
        return t.value

    def submit_host_test(self, test, ref, layout, phi=None, expected=None, mixture=1.0, n_samples=None, row_stride=None):
        """one slab whose TEST counts come from host memory (as submit_host) and whose references are on the device already
        (ref: int32 CUDA tensor / DeviceArray in the cohort's DEVICE layout -- (n_exons, n) with counts_layout 0, e.g. a window of
        cohort_select_reference_sets' aggregate references; (n, n_exons) with counts_layout 1)"""
        test = _host_slab(test, layout)
        if test.dtype not in (np.dtype(np.int32), np.dtype(np.uint16)):
            raise ValueError("test must be int32 or uint16")
        wire = test.dtype.itemsize
        if n_samples is None:
            n_samples = int(test.shape[1] if layout == 0 else test.shape[0])
        if row_stride is None:
            row_stride = int(test.strides[0] // wire) if layout == 0 else 0
        keep = []
        pr = _device_pointer(ref, np.int32, keep)
        pp = _device_pointer(phi, np.float64, keep) if phi is not None else None
        pe = _device_pointer(expected, np.float64, keep) if expected is not None else None
        t = C.c_int64(-1)
        check(lib().ed_cohort_submit_host_test(self.handle, C.c_void_p(test.ctypes.data), pr, int(n_samples), int(layout), int(wire),
                                               int(row_stride), pp, pe, float(mixture), C.byref(t)))
        self._keep[t.value % self.slabs_in_flight] = keep + [test, ref]
        return t.value

    def batch(self, ticket):
        """(Batch view, device pointer of phi, device pointer of expected) of a ticket"""
        h, pp, pe = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().ed_cohort_batch(self.handle, int(ticket), C.byref(h), C.byref(pp), C.byref(pe)))
        b = Batch._view(self.plan, int(lib().ed_batch_n_samples(h)), h.value)   # the ticket's own width (a short last slab has its own batch)
        return b, pp.value, pe.value

    def results(self, ticket, n_samples, path=False, loglik=False, info=True, posterior=False, breakpoints=None):
        """host copies of a ticket's results: dict(calls, info, phi, expected[, path][, loglik]); with the option phi_bins = B > 1
        phi_bins (B, n) and edges (B + 1, n) stand where phi is.  posterior=True adds call_posterior (Batch.call_posterior) and
        log_evidence; posterior="matrix" also the exon posteriors (Batch.posterior) as `posterior`; breakpoints=level adds call_bounds
        (Batch.call_bounds at that level)"""
        b, pp, pe = self.batch(ticket)
        b.n_samples = int(n_samples)
        out = {"calls": b.calls()}
        if info:
            out["info"] = b.call_info()
        exp = np.empty(n_samples)
        if self.phi_bins > 1:
            phib, edges = np.empty((self.phi_bins, n_samples)), np.empty((self.phi_bins + 1, n_samples))
            check(lib().ed_cohort_copy_bins_params(self.handle, int(ticket), _ptr(phib), _ptr(edges), _ptr(exp)))
            out["phi_bins"], out["edges"] = phib, edges
        else:
            phi = np.empty(n_samples)
            check(lib().ed_cohort_copy_params(self.handle, int(ticket), _ptr(phi), _ptr(exp)))
            out["phi"] = phi
        out["expected"] = exp
        if path:
            out["path"] = b.path()
        if loglik:
            out["loglik"] = b.loglik()
        if posterior:
            out["call_posterior"] = b.call_posterior()
            out["log_evidence"] = b.log_evidence()
            if posterior == "matrix":
                out["posterior"] = b.posterior()
        if breakpoints is not None:
            out["call_bounds"] = b.call_bounds(breakpoints)
        return out

    def wait(self, ticket):
        check(lib().ed_cohort_wait(self.handle, int(ticket)))

    def drain(self):
        check(lib().ed_cohort_drain(self.handle))

    def stage_ms_total(self):
        ms = (C.c_double * 5)()
        nr, nf = C.c_int64(0), C.c_int64(0)
        check(lib().ed_cohort_stage_ms_total(self.handle, ms, C.byref(nr), C.byref(nf)))
        return dict(zip(self.STAGES, [float(v) for v in ms])), nr.value, nf.value

    def n_wide_slabs(self):
        """host-fed int32 slabs that held a count outside 0 .. 65 535 and went up 32 bits wide (ed_cohort_n_wide_slabs)"""
        n = C.c_int64(0)
        check(lib().ed_cohort_n_wide_slabs(self.handle, C.byref(n)))
        return n.value

    def emission_intervals(self):
        """option timing: (n, 2) array of (start_ms, end_ms) of the emission stage of every timed run, relative to one reference event
        (ed_cohort_emission_intervals) -- with several lanes the launches overlap; their union is the chip time they take"""
        n = C.c_int64(0)
        check(lib().ed_cohort_emission_intervals(self.handle, None, 0, C.byref(n)))
        out = np.empty((max(n.value, 0), 2), dtype=np.float32)
        if n.value > 0:
            check(lib().ed_cohort_emission_intervals(self.handle, _ptr(out), n.value, C.byref(n)))
        return out

    def ingest_stats(self):
        b, s = C.c_double(0), C.c_double(0)
        check(lib().ed_cohort_ingest_stats(self.handle, C.byref(b), C.byref(s)))
        return b.value, s.value

    def run_host(self, test, ref, layout, phi=None, expected=None, mixture=1.0, want_path=False):
        """CallCNVs for a whole host-resident cohort (ed_cohort_run_host).  layout 0: (n_exons, S) arrays; layout 1: (S, n_exons)
        arrays (R's column-major n_exons x S matrix).  mixture: a scalar, or one value per column (matched tumour / normal pairs:
        test = tumours, ref = normals; ed_cohort_run_host_mix).  Returns dict(calls, info, phi, expected, n_unconverged,
        n_gsl_errors[, path])."""
        test, ref = np.ascontiguousarray(test), np.ascontiguousarray(ref)
        if test.dtype != ref.dtype or test.dtype not in (np.dtype(np.int32), np.dtype(np.uint16)):
            raise ValueError("test and ref must both be int32 or both uint16")
        S = int(test.shape[1] if layout == 0 else test.shape[0])
        mix = _per_sample_mixture(mixture, S)
        E = self.plan.n_exons
        ph = _f64(phi) if phi is not None else None
        ex = _f64(expected) if expected is not None else None
        phi_out, exp_out = np.empty(S), np.empty(S)
        path = np.empty((E, S) if layout == 0 else (S, E), dtype=np.uint8) if want_path else None
        n = C.c_int64(0)
        args = (self.handle, C.c_void_p(test.ctypes.data), C.c_void_p(ref.ctypes.data), S, int(layout), int(test.dtype.itemsize),
                _ptr(ph) if ph is not None else None, _ptr(ex) if ex is not None else None)
        outs = (_ptr(phi_out), _ptr(exp_out), _ptr(path) if path is not None else None, C.byref(n))
        if mix is None:
            check(lib().ed_cohort_run_host(*args, float(mixture), *outs))
        else:
            check(lib().ed_cohort_run_host_mix(*args, _ptr(mix), *outs))
        calls = np.zeros(n.value, dtype=CALL_DTYPE)
        info = np.zeros(n.value, dtype=CALL_INFO_DTYPE)
        check(lib().ed_cohort_copy_calls(self.handle, _ptr(calls), _ptr(info), n.value))
        nu, ne = C.c_int64(0), C.c_int64(0)
        check(lib().ed_cohort_run_status(self.handle, C.byref(nu), C.byref(ne)))
        out = {"calls": calls, "info": info, "phi": phi_out, "expected": exp_out, "n_unconverged": nu.value, "n_gsl_errors": ne.value}
        ts = (C.c_int64 * 4)()
        check(lib().ed_cohort_table_status(self.handle, ts))
        out["table_stats"] = dict(zip(Batch.TABLE_STATS, (int(x) for x in ts)))
        if self.phi_bins > 1:
            del out["phi"]
            out["phi_bins"], out["edges"] = np.empty((self.phi_bins, S)), np.empty((self.phi_bins + 1, S))
            check(lib().ed_cohort_copy_bins(self.handle, _ptr(out["phi_bins"]), _ptr(out["edges"])))
        if want_path:
            out["path"] = path
        return out


class MultiDevice:
    """ed_cohort_run_host over several devices from ONE process (ed_multi_*; csrc/edmulti.inc): the exon design replicated per
    device, the slabs dealt from one queue, one host thread per device, call tables put together in column order.
    devices=None: every visible device once; a device may be listed more than once."""

    def __init__(self, chrom_off, start, end, slab_samples, devices=None, slabs_in_flight=2, transition_probability=1e-4,
                 expected_cnv_length=50000.0, **options):
        chrom_off = np.ascontiguousarray(chrom_off, dtype=np.int32)
        start = np.ascontiguousarray(start, dtype=np.int32)
        end = np.ascontiguousarray(end, dtype=np.int32)
        self.n_exons = int(start.size)
        self.handle = C.c_void_p()
        dv = np.ascontiguousarray(devices, dtype=np.int32) if devices is not None else None
        check(lib().ed_multi_create(C.byref(self.handle), _ptr(dv) if dv is not None else None, int(dv.size) if dv is not None else 0,
                                    self.n_exons, int(chrom_off.size - 1), _ptr(chrom_off), _ptr(start), _ptr(end),
                                    float(transition_probability), float(expected_cnv_length), int(slab_samples), int(slabs_in_flight)))
        self.phi_bins = 1
        for k, v in options.items():
            self.set_option(k, v)

    @property
    def n_devices(self):
        return int(lib().ed_multi_n_devices(self.handle))

    def set_option(self, name, value):
        check(lib().ed_multi_set_option(self.handle, name.encode(), float(value)))
        if name == "phi_bins":
            self.phi_bins = int(value)

    def close(self):
        if self.handle:
            lib().ed_multi_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run_host(self, test, ref, layout, phi=None, expected=None, mixture=1.0, want_path=False):
        """as Cohort.run_host (mixture: a scalar or one value per column); the result also carries `devices`: per device the slabs /
        columns it took from the queue, its thread's seconds, its NUMA node"""
        test, ref = np.ascontiguousarray(test), np.ascontiguousarray(ref)
        if test.dtype != ref.dtype or test.dtype not in (np.dtype(np.int32), np.dtype(np.uint16)):
            raise ValueError("test and ref must both be int32 or both uint16")
        S = int(test.shape[1] if layout == 0 else test.shape[0])
        mix = _per_sample_mixture(mixture, S)
        E = self.n_exons
        ph = _f64(phi) if phi is not None else None
        ex = _f64(expected) if expected is not None else None
        phi_out, exp_out = np.empty(S), np.empty(S)
        path = np.empty((E, S) if layout == 0 else (S, E), dtype=np.uint8) if want_path else None
        n = C.c_int64(0)
        args = (self.handle, C.c_void_p(test.ctypes.data), C.c_void_p(ref.ctypes.data), S, int(layout), int(test.dtype.itemsize),
                _ptr(ph) if ph is not None else None, _ptr(ex) if ex is not None else None)
        outs = (_ptr(phi_out), _ptr(exp_out), _ptr(path) if path is not None else None, C.byref(n))
        if mix is None:
            check(lib().ed_multi_run_host(*args, float(mixture), *outs))
        else:
            check(lib().ed_multi_run_host_mix(*args, _ptr(mix), *outs))
        calls = np.zeros(n.value, dtype=CALL_DTYPE)
        info = np.zeros(n.value, dtype=CALL_INFO_DTYPE)
        check(lib().ed_multi_copy_calls(self.handle, _ptr(calls), _ptr(info), n.value))
        nu, ne = C.c_int64(0), C.c_int64(0)
        check(lib().ed_multi_run_status(self.handle, C.byref(nu), C.byref(ne)))
        out = {"calls": calls, "info": info, "phi": phi_out, "expected": exp_out, "n_unconverged": nu.value, "n_gsl_errors": ne.value}
        ts = (C.c_int64 * 4)()
        check(lib().ed_multi_table_status(self.handle, ts))
        out["table_stats"] = dict(zip(Batch.TABLE_STATS, (int(x) for x in ts)))
        if self.phi_bins > 1:
            del out["phi"]
            out["phi_bins"], out["edges"] = np.empty((self.phi_bins, S)), np.empty((self.phi_bins + 1, S))
            check(lib().ed_multi_copy_bins(self.handle, _ptr(out["phi_bins"]), _ptr(out["edges"])))
        if want_path:
            out["path"] = path
        D = self.n_devices
        dv, ns, nc, sec, nn = (C.c_int * D)(), (C.c_int64 * D)(), (C.c_int64 * D)(), (C.c_double * D)(), (C.c_int * D)()
        check(lib().ed_multi_device_stats(self.handle, dv, ns, nc, sec, nn))
        out["devices"] = [{"device": int(dv[i]), "slabs": int(ns[i]), "columns": int(nc[i]), "seconds": float(sec[i]), "numa_node": int(nn[i])} for i in range(D)]
        return out


# ---------------------------------------------------------------------------------------------
# exon ordering of CallCNVs (reference R/class_definition.R:323-336)
# ---------------------------------------------------------------------------------------------
# ---------------------------------------------------------------------------------------------
# maximum-likelihood fit of the HMM's two transition parameters (no counterpart in the reference)
# ---------------------------------------------------------------------------------------------
def _vmmin(fn, x0, reltol, max_iter, trace):
    """R optim's BFGS (src/appl/optim.c: vmmin) for a function that returns its value and gradient together: inverse-Hessian update,
    backtracking line search (step 1, x 0.2, sufficient decrease 1e-4), restart from the identity when the update is refused, stop
    when an accepted step changes f by no more than reltol (|f| + reltol).  A trial whose value is not finite is a failed step.
    Returns (x, f, iterations, evaluations, converged)."""
    n = len(x0)
    b = np.array(x0, dtype=np.float64)
    f, g = fn(b)
    if not np.isfinite(f):
        raise ValueError("the objective is not finite at the starting values")
    evals, iters, gradcount = 1, 0, 1
    ilast = gradcount
    B = np.eye(n)
    converged = False
    while True:
        if ilast == gradcount:
            B = np.eye(n)
        t = -B.dot(g)
        gradproj = float(t.dot(g))
        count = 0
        if gradproj < 0.0:
            step, accepted, f_new, g_new, b_new = 1.0, False, f, g, b
            while True:
                b_new = b + step * t
                count = int(np.sum(10.0 + b == 10.0 + b_new))
                if count == n:
                    break
                f_new, g_new = fn(b_new)
                evals += 1
                accepted = bool(np.isfinite(f_new)) and f_new <= f + gradproj * step * 1e-4
                trace.append({"x": b_new.copy(), "value": float(f_new), "accepted": accepted})
                if accepted:
                    break
                step *= 0.2
            if accepted:
                enough = abs(f_new - f) > reltol * (abs(f) + reltol)
                c = g_new - g
                tt = step * t
                b, f, g = b_new, f_new, g_new
                gradcount += 1
                iters += 1
                if not enough:
                    converged = True
                    break
                D1 = float(tt.dot(c))
                if D1 > 0.0:
                    X = B.dot(c)
                    D2 = 1.0 + float(c.dot(X)) / D1
                    B = B + (D2 * np.outer(tt, tt) - np.outer(tt, X) - np.outer(X, tt)) / D1
                else:
                    ilast = gradcount
            elif ilast < gradcount:      # no step along this direction: once more from the identity
                ilast = gradcount
                continue
            else:                        # ... and none along the gradient either
                converged = True
                break
        elif ilast == gradcount:         # uphill along the gradient itself: it is zero
            converged = True
            break
        else:
            ilast = gradcount
            continue
        if iters >= max_iter:
            break
        if gradcount - ilast > 2 * n:
            ilast = gradcount            # periodic restart
    return b, f, iters, evals, converged


def _score_sources(plan_args, loglik, n_samples):
    """the cohort's slabs as (device pointer, n_samples, what keeps it alive); host data is uploaded once"""
    n_exons = int(np.size(plan_args[1]))
    items = list(loglik) if isinstance(loglik, (list, tuple)) else [loglik]
    widths = list(n_samples) if isinstance(n_samples, (list, tuple, np.ndarray)) else [n_samples] * len(items)
    if len(widths) != len(items):
        raise ValueError("n_samples: one value, or one per slab")
    out = []
    for x, S in zip(items, widths):
        if isinstance(x, Batch):
            ptr = lib().ed_batch_loglik(x.handle)
            if not ptr:
                raise EdError("libedcore: %s" % lib().ed_last_error().decode(errors="replace"))
            x.n_calls()                                  # (waits for the run and for the matrix's [E][3][S] form)
            out.append((C.c_void_p(ptr), x.n_samples, x))
            continue
        if S is None:
            S = int(x.shape[-1])
        S = int(S)
        if not _is_device(x) and np.shape(x) != (n_exons, 3, S):
            raise ValueError("loglik must have shape (%d, 3, %d), got %s" % (n_exons, S, np.shape(x)))
        keep = [x]
        out.append((_device_pointer(x, np.float64, keep), S, keep))
    return out


def fit_transitions(chrom_off, start, end, loglik=None, n_samples=None, transition_probability=1e-4, expected_CNV_length=50000.0,
                    reltol=None, max_iter=100, evaluate=None, device=0):
    """Maximum-likelihood fit of the HMM's transition probability t and expected CNV length L on a cohort: maximises
    l(t, L) = the sum of the log-evidence of every (sample, chromosome) chain, from the given starting values.

    loglik: a likelihood matrix (n_exons, 3, n_samples) as Plan.posterior takes it (host data, a DeviceArray, a torch device tensor),
    a Batch that has run, or a list of these for a cohort of several slabs (n_samples then one value or one per slab; a Batch and
    anything with a shape know theirs).  Each evaluation is a fresh Plan at the trial values and one Plan.transition_score per slab;
    a plan the library refuses (a padded position beyond 32 bits) is a failed trial step.  The search is R optim's BFGS with its
    backtracking line search on x = (logit t, log L), in numpy; reltol defaults to sqrt(2^-52) with optim's stopping rule.
    evaluate: a callable (t, L) -> (l, dl/dt, dl/dL) that stands for the device evaluation.

    Returns a dict: transition_probability, expected_CNV_length, log_evidence (at the end), log_evidence_start, iterations,
    evaluations, converged, trace (every evaluation: t, L, log_evidence, accepted)."""
    if reltol is None:
        reltol = float(np.sqrt(2.0 ** -52))
    plan_args = (_i32(chrom_off), _i32(start), _i32(end))
    sources, works = None, {}
    if evaluate is None:
        if loglik is None:
            raise ValueError("fit_transitions: a likelihood matrix (or `evaluate`) is needed")
        sources = _score_sources(plan_args, loglik, n_samples)

        def evaluate(t, L):
            try:
                plan = Plan(plan_args[0], plan_args[1], plan_args[2], t, L, device)
            except EdError:
                return np.inf, 0.0, 0.0               # refused: a failed trial step
            try:
                tot = np.zeros(3)
                for k, (ptr, S, _) in enumerate(sources):
                    if S not in works:
                        works[S] = DeviceArray(nbytes=plan.n_exons * 3 * S * 8)
                    ev, sc = plan._transition_score(ptr, S, works[S])
                    if not np.all(np.isfinite(ev)):
                        c, s = (int(v) for v in np.argwhere(~np.isfinite(ev))[0])
                        raise ValueError("fit_transitions: the log-evidence of the chain of chromosome %d, sample %d%s is %r at "
                                         "transition_probability = %r, expected_CNV_length = %r"
                                         % (c, s, " of slab %d" % k if len(sources) > 1 else "", float(ev[c, s]), t, L))
                    tot += (ev.sum(), sc[:, 0, :].sum(), sc[:, 1, :].sum())
                return float(tot[0]), float(tot[1]), float(tot[2])
            finally:
                plan.close()

    calls = []

    def fn(x):
        with np.errstate(over="ignore", under="ignore"):
            t, L = float(1.0 / (1.0 + np.exp(-x[0]))), float(np.exp(x[1]))
        if not (0.0 < t < 1.0 and 0.0 < L < np.inf):
            calls.append((t, L, -np.inf))
            return np.inf, np.zeros(2)
        l, dt, dL = evaluate(t, L)
        calls.append((t, L, float(l)))
        if not (np.isfinite(l) and np.isfinite(dt) and np.isfinite(dL)):
            return np.inf, np.zeros(2)
        return -float(l), -np.array([dt * t * (1.0 - t), dL * L])

    t0, L0 = float(transition_probability), float(expected_CNV_length)
    if not (0.0 < t0 < 1.0 and 0.0 < L0 < np.inf):
        raise ValueError("fit_transitions: starting values must satisfy 0 < transition_probability < 1, 0 < expected_CNV_length")
    steps = []
    try:
        x, f, iters, evals, converged = _vmmin(fn, (np.log(t0 / (1.0 - t0)), np.log(L0)), float(reltol), int(max_iter), steps)
    finally:
        for w in works.values():
            w.free()
        for _, _, keep in (sources or ()):
            if isinstance(keep, list):
                for d in keep[1:]:
                    if isinstance(d, DeviceArray):
                        d.free()
    trace = [{"transition_probability": calls[0][0], "expected_CNV_length": calls[0][1], "log_evidence": calls[0][2], "accepted": True}]
    for (t, L, l), s in zip(calls[1:], steps):
        trace.append({"transition_probability": t, "expected_CNV_length": L, "log_evidence": l, "accepted": s["accepted"]})
    return {"transition_probability": float(1.0 / (1.0 + np.exp(-x[0]))), "expected_CNV_length": float(np.exp(x[1])),
            "log_evidence": -float(f), "log_evidence_start": float(calls[0][2]), "iterations": int(iters), "evaluations": int(evals),
            "converged": bool(converged), "trace": trace}


def mixture_geometry():
    """{tile, max_grid, pairs_per_workgroup, lds_bytes} of the mixture-profile kernel (ed_mix_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_mix_geometry(out))
    return dict(zip(("tile", "max_grid", "pairs_per_workgroup", "lds_bytes"), (int(v) for v in out)))


MIX_GRID = 16      # grid points of a round of fit_prop_tumor's search: one launch of the profile kernel


def _refine_grid(lo, hi):
    """16 equally spaced values from lo to hi, both ends exactly; lo, hi (S,) -> (16, S)"""
    k = np.arange(MIX_GRID, dtype=np.float64)[:, None] / (MIX_GRID - 1)
    g = lo[None, :] + (hi - lo)[None, :] * k
    g[0], g[-1] = lo, hi
    return g


def _first_argmax(l):
    """first index of the largest value per column, NaN ranked below everything"""
    return np.argmax(np.where(np.isnan(l), -np.inf, l), axis=0)


def _prop_tumor_search(evaluate, n_pairs, lower, upper, rounds, min_gain):
    """fit_prop_tumor's search on `evaluate`: grid (G, S) -> l (G, S).  Pure numpy, vectorised over the pairs."""
    S = int(n_pairs)
    lower = np.array(np.broadcast_to(np.asarray(lower, dtype=np.float64), (S,)))
    upper = np.array(np.broadcast_to(np.asarray(upper, dtype=np.float64), (S,)))
    if rounds < 1 or not np.all(np.isfinite(lower) & np.isfinite(upper) & (lower < upper)):
        raise ValueError("fit_prop_tumor: rounds >= 1 and finite lower < upper are needed")
    cols = np.arange(S)
    grid = _refine_grid(lower, upper)
    l = np.array(evaluate(grid), dtype=np.float64).reshape(MIX_GRID, S)
    profile, n_eval = l.copy(), 1
    bad = np.isnan(l).any(axis=0)
    trace = [{"grid": grid.copy(), "values": l.copy(), "k": _first_argmax(l)}]
    for _ in range(1, int(rounds)):
        k = trace[-1]["k"]
        grid = _refine_grid(grid[np.maximum(k - 1, 0), cols], grid[np.minimum(k + 1, MIX_GRID - 1), cols])
        l = np.array(evaluate(grid), dtype=np.float64).reshape(MIX_GRID, S)
        n_eval += 1
        bad |= np.isnan(l).any(axis=0)
        trace.append({"grid": grid.copy(), "values": l.copy(), "k": _first_argmax(l)})
    if np.all(lower == 0.0):
        null = profile[0].copy()
    else:
        null = np.array(evaluate(np.zeros((1, S))), dtype=np.float64).reshape(S)
        n_eval += 1
        bad |= np.isnan(null)
    k = trace[-1]["k"]
    h = grid[1] - grid[0]
    mk, lk = grid[k, cols], l[k, cols]
    km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, MIX_GRID - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        d2 = (l[km, cols] - 2.0 * lk) + l[kp, cols]
        vertex = (k >= 1) & (k <= MIX_GRID - 2) & (d2 < 0.0)
        off = h * (0.5 * (l[km, cols] - l[kp, cols]) / d2)
        m = np.where(vertex, np.clip(mk + off, grid[km, cols], grid[kp, cols]), mk)
        se = np.where(vertex, h / np.sqrt(-d2), np.nan)
    at_bound = ~vertex & ((mk == lower) | (mk == upper))
    gain = lk - null
    informative = ~bad & (gain >= min_gain)
    nan = np.full(S, np.nan)
    return {"prop_tumor": np.where(informative, m, nan), "estimate": np.where(bad, nan, m), "log_evidence": np.where(bad, nan, lk),
            "log_evidence_null": np.where(bad, nan, null), "gain": np.where(bad, nan, gain), "se": np.where(bad, nan, se),
            "informative": informative, "at_bound": at_bound & ~bad, "profile": profile, "evaluations": n_eval, "trace": trace}


def fit_prop_tumor(chrom_off, start, end, tumor=None, normal=None, phi=None, expected=None, lower=0.0, upper=1.0, rounds=3, min_gain=5.41,
                   transition_probability=1e-4, expected_CNV_length=50000.0, evaluate=None, device=0):
    """Maximum-likelihood tumour fraction (prop.tumor, the mixture of the somatic model) of every tumour / normal pair: per pair s the
    maximiser over [lower, upper] of l_s(m) = the sum over the chromosomes of the log-evidence of the pair's chains at mixture m, with the
    transition parameters given (not in the reference, whose somatic.CNV.call takes prop.tumor on faith).

    tumor, normal: counts (n_exons, n_pairs), or (n_exons,) for one pair.  phi, expected: one value per pair; when None both are fitted
    by Batch.fit, which -- as the reference's fit -- ignores the mixture.  Every evaluation is one launch of Plan.mixture_profile at 16
    mixtures per pair.  evaluate: a callable grid (G, n_pairs) -> l (G, n_pairs) that stands for the device (the number of pairs is
    then taken from phi, expected, lower or upper, else 1).

    The search is deterministic and runs in numpy: round 0 evaluates m_k = lower + (upper - lower) k / 15, k = 0 .. 15; every later
    round takes k* = the first index of the largest value, brackets [m_max(k* - 1, 0), m_min(k* + 1, 15)] and evaluates 16 equally spaced
    values with both ends; the spacing shrinks by 2 / 15 a round (three rounds: 1.2e-3 of the interval).  At the end, where k* of the
    last grid is interior and the second difference there is negative, the estimate is the vertex of the parabola through k* - 1, k*,
    k* + 1, clamped to the bracket, with se = spacing / sqrt(-second difference); elsewhere it is m_k*, se is NaN and at_bound says
    whether m_k* is `lower` or `upper`.

    Returns a dict of per-pair arrays: prop_tumor (NaN where the pair is not informative), estimate (the same without that mask),
    log_evidence (the largest value of the last grid), log_evidence_null (l_s(0): from the profile when lower == 0, else one extra
    evaluation), gain = log_evidence - log_evidence_null, se, informative (gain >= min_gain; 5.41 is half the 0.999 quantile of chi^2_1),
    at_bound; and profile (round 0, (16, n_pairs)), evaluations, trace (per round grid, values, k).  A pair whose evidence is NaN at
    any value evaluated (phi >= 1, expected 0 or 1) is reported NaN and not informative; the other pairs are not affected.

    What the profile can identify (checked on data drawn from the model: chromosomes of up to 1 300 exons with three planted segments of
    8 - 40 exons, two seeds): at totals around 2 000 reads and phi = 5e-4 the fractions 1.0 / 0.6 / 0.3 are recovered to the first
    grid's spacing with gains of thousands / a thousand / hundreds of log units.  A pair without a somatic CNV, and one at a fraction of
    0.1, gain at most 1.3: m = 0 makes the three states' emissions equal, so "no CNV" and "no tumour" are the same statement and the
    pair is reported not informative.  At totals around 200 and phi = 2e-3 a fraction of 0.3 is not identifiable either (gain 0.07)."""
    if evaluate is not None:
        S = max(int(np.size(x)) for x in (phi, expected, lower, upper) if x is not None)
        return _prop_tumor_search(evaluate, S, lower, upper, rounds, min_gain)
    if tumor is None or normal is None:
        raise ValueError("fit_prop_tumor: tumour and normal counts (or `evaluate`) are needed")
    chrom_off, start, end = _i32(chrom_off), _i32(start), _i32(end)
    E = int(start.size)
    on_dev = _is_device(tumor) and _is_device(normal)           # int32 (n_exons, n_pairs) device arrays are used in place
    if not on_dev:
        tumor, normal = _i32(tumor), _i32(normal)
        if tumor.ndim == 1:
            tumor, normal = tumor.reshape(E, 1), normal.reshape(-1, 1)
    if len(tumor.shape) != 2 or tumor.shape[0] != E or tuple(normal.shape) != tuple(tumor.shape):
        raise ValueError("fit_prop_tumor: tumor and normal must both have shape (%d, n_pairs)" % E)
    S = int(tumor.shape[1])
    plan = Plan(chrom_off, start, end, transition_probability, expected_CNV_length, device)
    dev = []
    try:
        dt, dn = (tumor, normal) if on_dev else (DeviceArray(tumor), DeviceArray(normal))
        if not on_dev:
            dev += [dt, dn]
        if phi is None or expected is None:
            dp, de = DeviceArray(np.zeros(S)), DeviceArray(np.zeros(S))
            dev += [dp, de]
            batch = Batch(plan, S)
            try:
                batch.fit(dt, dn, dp, de)
                check(lib().ed_synchronize(None))
                if batch.fit_unconverged()[0]:
                    import warnings
                    warnings.warn("beta-binomial fit: the Newton iteration did not converge (phi, expected are its last iterate)")
            finally:
                batch.close()
            phi, expected = dp.to_host(), de.to_host()
        else:
            phi = _f64(np.broadcast_to(np.asarray(phi, dtype=np.float64), (S,)))
            expected = _f64(np.broadcast_to(np.asarray(expected, dtype=np.float64), (S,)))
            dp, de = DeviceArray(phi), DeviceArray(expected)
            dev += [dp, de]

        def on_device(grid):
            return plan.mixture_profile(dt, dn, dp, de, np.ascontiguousarray(grid, dtype=np.float64)).sum(axis=1)
        fit = _prop_tumor_search(on_device, S, lower, upper, rounds, min_gain)
        fit["phi"], fit["expected"] = np.array(phi), np.array(expected)
        return fit
    finally:
        for d in dev:
            d.free()
        plan.close()


# ---------------------------------------------------------------------------------------------
# the copy number of a call: the likelihood profile over the copy ratio
# ---------------------------------------------------------------------------------------------
COPY_RATIOS = (0.5, 1.0, 1.5, 2.0)       # the copy ratios of CN 1 .. 4; CN 0 is evaluated at `ratio_floor`


def ratio_geometry():
    """{seg_tiles, narrow, max_grid, items_per_workgroup} of the copy-ratio profile's kernel (ed_ratio_geometry): a wavefront takes up to
    seg_tiles tiles of 64 exons of a row; narrow = 0: there is no second mapping for short rows.  For tests placing rows on the edges."""
    out = (C.c_int32 * 4)()
    check(lib().ed_ratio_geometry(out))
    return dict(zip(("seg_tiles", "narrow", "max_grid", "items_per_workgroup"), (int(v) for v in out)))


def _ratio_rows(rows):
    """rows as ed_call records: a CALL_DTYPE array as it is, else the fields sample, chrom, start_exon, end_exon of a structured array"""
    rows = np.asarray(rows)
    if rows.dtype == CALL_DTYPE:
        return np.ascontiguousarray(rows).reshape(-1)
    out = np.zeros(rows.size, dtype=CALL_DTYPE)
    for k in ("sample", "chrom", "start_exon", "end_exon"):
        out[k] = rows[k].reshape(-1)
    out["nexons"] = out["end_exon"] - out["start_exon"] + 1
    return out


def _dose_grid(ratio_floor):
    """the 16 doses of the first round: four from the floor to CN 1, then steps of 1/8 of a ratio up to CN 4; CN 0 .. 4 are the
    indices 0, 3, 7, 11, 15"""
    lo = 2.0 * (float(ratio_floor) - 1.0)
    g = np.concatenate([lo + (-1.0 - lo) * np.arange(4) / 3.0, -1.0 + np.arange(1, 13) / 4.0])
    g[0], g[3] = lo, -1.0
    return g


_CN_INDEX = (0, 3, 7, 11, 15)
COPY_RATIO_GRID = tuple(float(1.0 + d / 2.0) for d in _dose_grid(0.05))     # that grid as ratios, at the default floor


def _chi2_1(level):
    """the `level` quantile of chi^2 with one degree of freedom"""
    from statistics import NormalDist
    if not 0.0 < level < 1.0:
        raise ValueError("level must lie in (0, 1), got %r" % (level,))
    return NormalDist().inv_cdf(0.5 + 0.5 * level) ** 2


def copy_number_from_profile(ratios, L, ratio_floor=0.05):
    """The evidence for the copy numbers 0 .. 4 of every row from its profile (pure numpy).  ratios (G,) or (n_rows, G), L (n_rows, G):
    what Plan.ratio_profile / Batch.call_ratio_profile return.  Per row
        log10_bf_cn[k] = log10(e) (L(r_k) - L(1)),  r = ratio_floor, 0.5, 1, 1.5, 2  for CN k = 0 .. 4
    read at the columns whose ratio equals r_k (the first such column; NaN where the row was not evaluated there), and cn = the copy
    number with the largest value, the first on ties, -1 where none is a number.  The model degenerates at ratio 0 (the expected
    proportion goes to 0), so CN 0 is evaluated at `ratio_floor`: a modelling parameter that stands for the residual reads a homozygous
    deletion still collects (mis-mapped reads, contamination), not a measured number.
    Returns {"log10_bf_cn": (n_rows, 5), "cn": (n_rows,) int64, "ratios": the five ratios}."""
    L = np.asarray(L, dtype=np.float64)
    if L.ndim == 1:
        L = L[None, :]
    n, G = L.shape
    ratios = np.asarray(ratios, dtype=np.float64)
    if ratios.ndim == 1:
        ratios = np.broadcast_to(ratios[None, :], (n, ratios.size))
    if ratios.shape != (n, G):
        raise ValueError("ratios must have shape (G,) or (n_rows, G) matching L %s, got %s" % (L.shape, ratios.shape))
    want = np.array((float(ratio_floor),) + COPY_RATIOS)
    at = np.full((n, 5), np.nan)
    rows = np.arange(n)
    used = 1.0 + (2.0 * (want - 1.0)) / 2.0                           # what ratio_profile reports for these ratios (the floor's last bit may differ)
    for k in range(5):
        hit = (ratios == want[k]) | (ratios == used[k])
        col = np.argmax(hit, axis=1)                                  # the first column at that ratio
        at[:, k] = np.where(hit.any(axis=1), L[rows, col] if G else np.nan, np.nan)
    bf = np.log10(np.e) * (at - at[:, 2:3])
    ranked = np.where(np.isnan(bf), -np.inf, bf)
    cn = np.where(np.isnan(bf).all(axis=1), -1, np.argmax(ranked, axis=1)).astype(np.int64)
    return {"log10_bf_cn": bf, "cn": cn, "ratios": want}


def _ratio_search(evaluate, n_rows, rounds, level, ratio_floor):
    """call_copy_number's search on `evaluate`: doses (G, n_rows) -> L (G, n_rows).  Pure numpy, vectorised over the rows."""
    n = int(n_rows)
    if rounds < 1 or not 0.0 < ratio_floor < 0.5:
        raise ValueError("call_copy_number: rounds >= 1 and 0 < ratio_floor < 0.5 are needed")
    q = _chi2_1(level)
    cols = np.arange(n)
    grid = np.repeat(_dose_grid(ratio_floor)[:, None], n, axis=1)
    l = np.array(evaluate(grid), dtype=np.float64).reshape(MIX_GRID, n)
    profile = l.copy()
    trace = [{"grid": grid.copy(), "values": l.copy(), "k": _first_argmax(l)}]
    for _ in range(1, int(rounds)):
        k = trace[-1]["k"]
        grid = _refine_grid(grid[np.maximum(k - 1, 0), cols], grid[np.minimum(k + 1, MIX_GRID - 1), cols])
        l = np.array(evaluate(grid), dtype=np.float64).reshape(MIX_GRID, n)
        trace.append({"grid": grid.copy(), "values": l.copy(), "k": _first_argmax(l)})
    bad = np.zeros(n, dtype=bool)
    for r in trace:
        bad |= np.isnan(r["values"]).any(axis=0)
    # the estimate: the vertex of the parabola through the last grid's largest value and its neighbours (the spacing of the first
    # grid is not even, so the step is written for three abscissae)
    k = trace[-1]["k"]
    km, kp = np.maximum(k - 1, 0), np.minimum(k + 1, MIX_GRID - 1)
    xk, lk = grid[k, cols], l[k, cols]
    with np.errstate(invalid="ignore", divide="ignore"):
        h1, h2 = xk - grid[km, cols], grid[kp, cols] - xk
        s1, s2 = (lk - l[km, cols]) / h1, (l[kp, cols] - lk) / h2
        d2 = 2.0 * (s2 - s1) / (h1 + h2)
        d1 = (s2 * h1 + s1 * h2) / (h1 + h2)
        vertex = (k >= 1) & (k <= MIX_GRID - 2) & (d2 < 0.0)
        m = np.where(vertex, np.clip(xk - d1 / d2, grid[km, cols], grid[kp, cols]), xk)
        se = np.where(vertex, 1.0 / np.sqrt(-d2), np.nan)
    # the profile-likelihood interval on every point evaluated: z = sqrt(2 (Lmax - L)) is linear where L is a parabola, so its crossing of
    # sqrt(q) is interpolated linearly between the last point inside and the first outside, walking out from the largest value
    x = np.concatenate([r["grid"] for r in trace], axis=0)
    y = np.concatenate([r["values"] for r in trace], axis=0)
    order = np.argsort(x, axis=0, kind="stable")
    x, y = np.take_along_axis(x, order, axis=0), np.take_along_axis(y, order, axis=0)
    top = _first_argmax(y)
    lmax = y[top, cols] if n else np.zeros(0)
    with np.errstate(invalid="ignore"):
        z = np.sqrt(np.maximum(2.0 * (lmax[None, :] - y), 0.0))
    zq = np.sqrt(q)
    P = x.shape[0]
    lo, hi = np.empty(n), np.empty(n)
    for j in range(n):
        t = int(top[j])
        a = t
        while a > 0 and z[a - 1, j] <= zq:
            a -= 1
        lo[j] = x[0, j] if a == 0 else x[a, j] - (x[a, j] - x[a - 1, j]) * (zq - z[a, j]) / (z[a - 1, j] - z[a, j])
        b = t
        while b < P - 1 and z[b + 1, j] <= zq:
            b += 1
        hi[j] = x[P - 1, j] if b == P - 1 else x[b, j] + (x[b + 1, j] - x[b, j]) * (zq - z[b, j]) / (z[b + 1, j] - z[b, j])
    ratios0 = 1.0 + trace[0]["grid"].T / 2.0
    cnp = copy_number_from_profile(ratios0, profile.T, ratios0[0, 0] if n else ratio_floor)
    cn_l = profile[list(_CN_INDEX), :]
    with np.errstate(invalid="ignore"):
        gain = 2.0 * (lmax - np.max(cn_l, axis=0)) if n else np.zeros(0)
        informative = ~bad & (2.0 * (np.max(profile, axis=0) - np.min(profile, axis=0)) >= q) if n else np.zeros(0, dtype=bool)
    nan = np.full(n, np.nan)
    floor_dose = _dose_grid(ratio_floor)[0]

    def as_ratio(d):                       # the floor's dose stands for ratio_floor itself (1 + dose / 2 may differ from it in the last bit)
        return np.where(bad, nan, np.where(d == floor_dose, float(ratio_floor), 1.0 + d / 2.0))
    return {"ratio": as_ratio(m), "ratio_se": np.where(bad, nan, se / 2.0), "ratio_lo": as_ratio(lo), "ratio_hi": as_ratio(hi),
            "cn": np.where(bad, -1, cnp["cn"]), "log10_bf_cn": np.where(bad[:, None], np.nan, cnp["log10_bf_cn"]),
            "mosaic_gain": np.where(bad, nan, gain), "informative": informative, "log_likelihood": np.where(bad, nan, lmax),
            "profile": profile, "evaluations": len(trace), "trace": trace}


def call_copy_number(chrom_off, start, end, rows, test=None, ref=None, phi=None, expected=None, rounds=3, level=0.95, ratio_floor=0.05,
                     evaluate=None, layout=0, device=0):
    """How many copies is a call?  Per row (sample, first exon .. last exon) the maximum-likelihood copy ratio of its exons with a
    profile-likelihood interval, the evidence for the copy numbers 0 .. 4 and a test of whether any of them fits (not in the reference,
    whose advice is to look at reads.ratio).  The objective is Plan.ratio_profile's L(row, ratio): the beta-binomial emission of the HMM
    at any copy ratio instead of the three the states stand for.

    rows: records with sample, chrom, start_exon, end_exon -- a call table (Batch.calls()) or regions crossed with samples.  test,
    ref: counts (n_exons, S), or (S, n_exons) with layout=1; phi, expected: one value per sample.  evaluate: a callable doses
    (G, n_rows) -> L (G, n_rows) that stands for the device (dose = 2 (ratio - 1)).

    The search is deterministic and runs in numpy.  Round 1 evaluates a fixed grid of 16 ratios from ratio_floor to 2 that holds the
    ratios of CN 0 .. 4 (ratio_floor, 0.5, 1, 1.5, 2); every later round takes the first index k* of the row's largest value, brackets
    the two neighbours and evaluates 16 equally spaced ratios with both ends.  Per row:
      ratio        the vertex of the parabola through k* - 1, k*, k* + 1 of the last grid, clamped to the bracket (the grid point itself
                   where k* is the grid's end or the points are not concave)
      ratio_se     from the parabola's curvature, 1 / sqrt(-L''); NaN without a vertex
      ratio_lo, ratio_hi   where 2 (Lmax - L) crosses the chi^2_1 quantile of `level`, Lmax the largest value evaluated; interpolated
                   (linearly in the square root of that deviance) on all points evaluated, the grid's end where it is never crossed
      cn, log10_bf_cn      copy_number_from_profile on round 1
      mosaic_gain  2 (Lmax - the largest L at the five copy numbers): chi^2_1 under "the copy ratio is one of them"; large for a mosaic
                   or subclonal event
      informative  False where the profile's range over round 1, 2 (max - min), stays below the quantile: the row says nothing
    and log_likelihood (Lmax), profile (round 1, (16, n_rows)), evaluations, trace.  A row with a NaN at any ratio evaluated reads NaN,
    cn -1, and is not informative; the other rows are not affected."""
    rows = _ratio_rows(rows)
    n = int(rows.size)
    if evaluate is not None:
        return _ratio_search(evaluate, n, rounds, level, ratio_floor)
    if test is None or ref is None or phi is None or expected is None:
        raise ValueError("call_copy_number: counts, phi and expected (or `evaluate`) are needed")
    plan = Plan(chrom_off, start, end, device=device)
    try:
        with _staged() as keep:
            S = _n_samples_of(phi)
            pt, pr = _device_pointer(test, np.int32, keep), _device_pointer(ref, np.int32, keep)
            pp, pe = _device_pointer(phi, np.float64, keep), _device_pointer(expected, np.float64, keep)
            return _ratio_search(lambda doses: plan._ratio_doses(rows, pt, pr, pp, pe, S, doses, layout), n, rounds, level, ratio_floor)
    finally:
        plan.close()


# ---------------------------------------------------------------------------------------------
# detection power: the expected Bayes factor of a CNV per exon and per region
# ---------------------------------------------------------------------------------------------
POWER_DTYPE = np.dtype([("chrom", "<i4"), ("first_exon", "<i4"), ("last_exon", "<i4"), ("n_exons", "<i4"), ("n_empty", "<i4"),
                        ("mean_del", "<f8"), ("var_del", "<f8"), ("mean_dup", "<f8"), ("var_dup", "<f8"), ("price", "<f8"),
                        ("threshold", "<f8"), ("power_del", "<f8"), ("power_dup", "<f8")])


def power_geometry():
    """{walk_tile, occupancy_cap, max_total, region_tile} of the detection-power kernels (ed_power_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_power_geometry(out))
    return dict(zip(("walk_tile", "occupancy_cap", "max_total", "region_tile"), (int(v) for v in out)))


def _normal_cdf(z):
    try:
        from scipy.special import ndtr
        return ndtr(z)
    except ImportError:
        import math
        return np.frompyfunc(lambda v: 0.5 * math.erfc(-v / math.sqrt(2.0)) if v == v else v, 1, 1)(z).astype(np.float64)


def power_from_moments(mean, var, threshold):
    """P(sum of the exons' Bayes-factor terms > threshold) when the region truly carries the CNV, by the NORMAL APPROXIMATION of a sum
    of independent exon terms: Phi((mean - threshold) / sqrt(var)).  Where var is 0 the result is 1 or 0 by the sign of mean - threshold
    (0 where they are equal); NaN stays NaN.  A few exons at low depth are far from normal: read the figure as a guide there."""
    mean, var, threshold = np.broadcast_arrays(np.asarray(mean, np.float64), np.asarray(var, np.float64), np.asarray(threshold, np.float64))
    d = mean - threshold
    out = np.full(d.shape, np.nan)
    ok = ~(np.isnan(d) | np.isnan(var))
    pos = ok & (var > 0)
    out[pos] = _normal_cdf(d[pos] / np.sqrt(var[pos]))
    flat = ok & ~(var > 0)
    out[flat] = (d[flat] > 0).astype(np.float64)
    return out


def _region_rows(rows):
    """call-shaped rows from a CALL_DTYPE array (or any structured array with chrom, start_exon, end_exon) or from (chrom, first, last) triples"""
    a = np.asarray(rows)
    if a.dtype.names:
        out = np.zeros(a.size, dtype=CALL_DTYPE)
        for k in ("chrom", "start_exon", "end_exon"):
            out[k] = a[k].ravel()
        return out
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError("region rows must fit 32-bit integers")
    out = np.zeros(a.shape[0], dtype=CALL_DTYPE)
    out["chrom"], out["start_exon"], out["end_exon"] = a[:, 0], a[:, 1], a[:, 2]
    return out


_MAP_COUNTERS = ("n_samples", "n_exons", "n_jobs", "max_jobs", "n_skipped", "n_bad_samples", "largest_total", "map_words")


class _TotalsMap:
    """What the device-resident maps indexed by a cell's total share (csrc/edtotals.inc): a handle of the entries ed_<_ENTRY>_*, the
    samples' parameters, the staging of the counts, a sample's table, the common counters."""
    _ENTRY = None       # "power", "quant"

    def __init__(self, plan, phi, expected, stream):
        self.plan, self.stream = plan, stream
        self._phi, self._expected = _f64(np.atleast_1d(phi)), _f64(np.atleast_1d(expected))
        self.n_samples = _n_samples_of(self._phi)
        if self._expected.size != self.n_samples:
            raise ValueError("phi and expected must have one value per sample")
        self.handle = C.c_void_p()

    def _counts(self, test, ref, layout, keep):
        """(test pointer, ref pointer, on the device?) inside `with _staged() as keep`"""
        on_dev = _is_device(test) and _is_device(ref)
        if not on_dev and (_is_device(test) or _is_device(ref)):
            raise ValueError("test and ref must both be device arrays or both be host arrays")
        if on_dev:
            return _device_pointer(test, np.int32, keep), _device_pointer(ref, np.int32, keep), 1
        test, ref = _i32(test), _i32(ref)
        for x in (test, ref):
            _check_counts_shape(x, self.plan.n_exons, self.n_samples, layout)
        keep.extend((test, ref))       # (the converted copies live as long as the call)
        return _ptr(test), _ptr(ref), 0

    @staticmethod
    def _live_rows(rows):
        """(rows as call-shaped records, the mask of the (chrom, -1, -1) rows, the others contiguous)"""
        rows = _region_rows(rows)
        none = (rows["start_exon"] == -1) & (rows["end_exon"] == -1)
        return rows, none, np.ascontiguousarray(rows[~none])

    def _entry(self, what):
        return getattr(lib(), "ed_%s_%s" % (self._ENTRY, what))

    def _table(self, sample, *channels):
        """(totals [k], values [*channels][max(k, 1)], k) of the sample: one call for k, one for the arrays"""
        n = C.c_int64(0)
        check(self._entry("copy_table")(self.handle, int(sample), None, None, 0, C.byref(n)))
        k = int(n.value)
        totals, values = np.zeros(k, dtype=np.int32), np.zeros(channels + (max(k, 1),))
        if k:
            check(self._entry("copy_table")(self.handle, int(sample), _ptr(totals), _ptr(values), k, C.byref(n)))
        return totals, values, k

    def _stats(self, *more):
        cnt, ms = (C.c_int64 * (8 + len(more)))(), (C.c_double * 4)()
        check(self._entry("stats")(self.handle, cnt, ms))
        out = dict(zip(_MAP_COUNTERS + more, (int(v) for v in cnt)))
        out.update(zip(("occupancy_ms", "walk_ms", "regions_ms", "exons_ms"), (float(v) for v in ms)))
        return out

    def free(self):
        if self.handle:
            self._entry("free")(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class PowerMap(_TotalsMap):
    """Device-resident detection-power map of Plan.power_map: per sample the table of (total, mean_del, var_del, mean_dup, var_dup) of
    its occupied totals, and per (sample, exon) the table slot of the exon's total.  mean_T is the expected contribution of an exon to a
    call's BF column when the exon truly is in state T, var_T its variance (include/exomedepth_amd.h)."""
    _ENTRY = "power"

    def __init__(self, plan, test, ref, phi, expected, mixture=1.0, layout=0, stream=None):
        super().__init__(plan, phi, expected, stream)
        S = self.n_samples
        mix = _per_sample_mixture(mixture, S)
        with _staged() as keep:
            pt, pr, on_dev = self._counts(test, ref, layout, keep)
            check(lib().ed_plan_power_map(C.byref(self.handle), plan.handle, pt, pr, on_dev, int(layout), S, _ptr(self._phi), _ptr(self._expected),
                                          _ptr(mix) if mix is not None else None, 1.0 if mix is not None else float(mixture),
                                          C.c_void_p(stream or 0)))

    def regions(self, rows, threshold=None):
        """Per (region, sample): a POWER_DTYPE array of shape (n_regions, n_samples).  rows: a call table (CALL_DTYPE; chrom, start_exon
        and end_exon are read) or (chrom, first_exon, last_exon) triples -- a contiguous run of exons inside one chromosome of the plan;
        a row of (chrom, -1, -1) stands for a region with no exon inside (region_runs makes such rows): n_exons 0, sums 0, price NaN.
        mean_T / var_T are the sums over the run's exons, n_empty counts its exons without reads, price is the evidence at which
        Viterbi prefers exactly this segment to all normal; power_T = power_from_moments(mean_T, var_T, threshold) with threshold =
        price unless given (a scalar or one value per region)."""
        rows, none, live = self._live_rows(rows)
        R, S, n = rows.size, self.n_samples, int(live.size)
        sums, empty = np.zeros((4, n, S)), np.zeros((n, S), dtype=np.int32)
        price, nex = np.zeros(n), np.zeros(n, dtype=np.int32)
        check(lib().ed_power_regions(self.handle, _ptr(live), n, _ptr(sums), _ptr(empty), _ptr(price), _ptr(nex), C.c_void_p(self.stream or 0)))
        out = np.zeros((R, S), dtype=POWER_DTYPE)
        out["chrom"], out["first_exon"], out["last_exon"] = rows["chrom"][:, None], rows["start_exon"][:, None], rows["end_exon"][:, None]
        out["price"][none] = np.nan
        at = np.flatnonzero(~none)
        out["n_exons"][at], out["n_empty"][at], out["price"][at] = nex[:, None], empty, price[:, None]
        for c, k in enumerate(("mean_del", "var_del", "mean_dup", "var_dup")):
            out[k][at] = sums[c]
        thr = out["price"] if threshold is None else np.broadcast_to(np.asarray(threshold, dtype=np.float64).reshape(-1, 1), (R, 1))
        out["threshold"] = thr
        out["power_del"] = power_from_moments(out["mean_del"], out["var_del"], out["threshold"])
        out["power_dup"] = power_from_moments(out["mean_dup"], out["var_dup"], out["threshold"])
        return out

    def exons(self):
        """(4, n_samples, n_exons): mean_del, var_del, mean_dup, var_dup of every exon; NaN where the total was skipped or the sample is
        outside the model"""
        out = np.zeros((4, self.n_samples, self.plan.n_exons))
        check(lib().ed_power_copy_exons(self.handle, _ptr(out), C.c_void_p(self.stream or 0)))
        return out

    def table(self, sample):
        """the sample's table: dict of totals (ascending, int32) and mean_del, var_del, mean_dup, var_dup"""
        totals, values, k = self._table(sample, 4)
        return {"totals": totals, "mean_del": values[0, :k].copy(), "var_del": values[1, :k].copy(), "mean_dup": values[2, :k].copy(),
                "var_dup": values[3, :k].copy()}

    def stats(self):
        """n_samples, n_exons, n_jobs (occupied totals over all samples), max_jobs (of one sample), n_skipped (cells whose total is above
        the largest one walked), n_bad_samples (parameters outside the model), largest_total, map_words; occupancy_ms, walk_ms,
        regions_ms, exons_ms (the last call of each), host-timed between waits"""
        return self._stats()


def region_runs(chromosome, start, end, regions):
    """Coordinate regions to runs of exons.  chromosome, start, end: the exons in the plan's order (each chromosome one contiguous block;
    the block's index is the plan's chromosome index); regions: (chromosome, start, end) triples.  A region's run goes from the first to
    the last exon lying wholly inside it (start_i >= start and end_i <= end: TestCNV's rule); an exon between those two that is not
    wholly inside belongs to the run as well -- a call cannot skip it.  Returns a CALL_DTYPE array (chrom, start_exon, end_exon, nexons =
    the run's length); a region with no exon inside has start_exon = end_exon = -1 and nexons = 0 (chrom -1 when its chromosome has no
    exon at all)."""
    chromosome = np.asarray([str(c) for c in chromosome], dtype=object)
    start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    if not (chromosome.size == start.size == end.size):
        raise ValueError("chromosome, start and end must have one entry per exon")
    blocks = {}
    i, n = 0, int(chromosome.size)
    while i < n:
        j = i
        while j < n and chromosome[j] == chromosome[i]:
            j += 1
        if chromosome[i] in blocks:
            raise ValueError("the exons of chromosome %s are not one contiguous block" % chromosome[i])
        blocks[chromosome[i]] = (len(blocks), i, j)
        i = j
    mono = {c: bool(np.all(np.diff(start[lo:hi]) >= 0) and np.all(np.diff(end[lo:hi]) >= 0)) for c, (_, lo, hi) in blocks.items()}
    regions = list(regions)
    out = np.zeros(len(regions), dtype=CALL_DTYPE)
    out["chrom"], out["start_exon"], out["end_exon"] = -1, -1, -1
    for r, (c, s, e) in enumerate(regions):
        c = str(c)
        if c not in blocks:
            continue
        k, lo, hi = blocks[c]
        out["chrom"][r] = k
        if mono[c]:
            first = lo + int(np.searchsorted(start[lo:hi], s, "left"))
            last = lo + int(np.searchsorted(end[lo:hi], e, "right")) - 1
        else:
            inside = np.flatnonzero((start[lo:hi] >= s) & (end[lo:hi] <= e))
            first, last = (lo + int(inside[0]), lo + int(inside[-1])) if inside.size else (0, -1)
        if first <= last:
            out["start_exon"][r], out["end_exon"][r], out["nexons"][r] = first, last, last - first + 1
    return out


def detection_power(chrom_off, start, end, test, ref, phi, expected, rows, mixture=1.0, threshold=None, layout=0,
                    transition_probability=1e-4, expected_CNV_length=50000.0, exons=False, device=0):
    """Detection power of a cohort: PowerMap.regions(rows, threshold) of the samples' map on a plan of (chrom_off, start, end) with the
    given transition parameters; with exons=True a pair (regions, PowerMap.exons()).  Arguments as Plan and Plan.power_map take them.
    Answers, of a negative result: could a heterozygous deletion / duplication of this region have been seen in this sample at this depth?"""
    plan = Plan(chrom_off, start, end, transition_probability, expected_CNV_length, device)
    pm = None
    try:
        pm = plan.power_map(test, ref, phi, expected, mixture, layout)
        reg = pm.regions(rows, threshold)
        return (reg, pm.exons()) if exons else reg
    finally:
        if pm is not None:
            pm.free()
        plan.close()


# ---------------------------------------------------------------------------------------------
# beta-binomial quantiles: qbetabinom, the normal range of every exon and how a region's counts fall into it
# ---------------------------------------------------------------------------------------------
def quantile_geometry():
    """{walk_tile, occupancy_cap, max_total, region_tile, max_probs} of the quantile kernels (ed_quant_geometry)"""
    out = (C.c_int32 * 5)()
    check(lib().ed_quant_geometry(out))
    return dict(zip(("walk_tile", "occupancy_cap", "max_total", "region_tile", "max_probs"), (int(v) for v in out)))


def qbetabinom_ab(p, size, shape1, shape2):
    """reference R/tools.R:42-53 qbetabinom.ab, element by element: with pm the beta-binomial masses of 0 .. size and cs their running
    sum, above = the first value with cs > p, the result is (above - 1) + (p - cs[above - 1]) / pm[above] (p / pm[0] for the first value).
    The arguments are recycled to the longest, as R recycles them (on the host); a float64 array of that length (0-d arguments: length
    1).  NaN (R's NA) where p >= 1, where a shape is not positive and finite, and where size is not a whole number in 0 .. max_total
    (quantile_geometry)."""
    args = [_f64(np.atleast_1d(x)).ravel() for x in (p, size, shape1, shape2)]
    n = 0 if any(a.size == 0 for a in args) else max(a.size for a in args)
    args = [np.ascontiguousarray(np.resize(a, n)) for a in args]
    out = np.zeros(n)
    check(lib().ed_qbetabinom_ab(*[_ptr(a) if n else None for a in args], n, _ptr(out) if n else None))
    return out


def qbetabinom(p, size, phi, prob):
    """reference R/tools.R:21-25: qbetabinom_ab at shape1 = prob (1 - phi) / phi, shape2 = (1 - prob)(1 - phi) / phi"""
    phi, prob = _f64(np.atleast_1d(phi)).ravel(), _f64(np.atleast_1d(prob)).ravel()
    n = 0 if not (phi.size and prob.size) else max(phi.size, prob.size)
    phi, prob = np.resize(phi, n), np.resize(prob, n)
    with np.errstate(all="ignore"):
        a, b = prob * (1. - phi) / phi, (1. - prob) * (1. - phi) / phi
    return qbetabinom_ab(p, size, a, b)


class QuantileMap(_TotalsMap):
    """Device-resident quantile map of Plan.quantile_map: per sample the table of (total, q_k, below_k) of its occupied totals at the K
    requested probabilities, per (sample, exon) the table slot of the exon's total, and the test counts.  q_k = qbetabinom(p_k, total,
    phi, expected) under the sample's fitted normal state, below_k = the mass strictly below its cut (include/exomedepth_amd.h)."""
    _ENTRY = "quant"

    def __init__(self, plan, test, ref, phi, expected, probs=(0.025, 0.975), layout=0, stream=None):
        super().__init__(plan, phi, expected, stream)
        self.probs = _f64(np.atleast_1d(probs)).ravel()
        with _staged() as keep:
            pt, pr, on_dev = self._counts(test, ref, layout, keep)
            check(lib().ed_plan_quantile_map(C.byref(self.handle), plan.handle, pt, pr, on_dev, int(layout), _ptr(self._phi), _ptr(self._expected),
                                             _ptr(self.probs) if self.probs.size else None, int(self.probs.size), self.n_samples,
                                             C.c_void_p(stream or 0)))

    def regions(self, rows):
        """Per (region, sample), a dict of observed (n_regions, n_samples, K + 1) int32: the run's exons per bin, the bin of an exon being
        the number of k with test count >= ceil(q_k) - 1 (closed below: a count on a cut is in the upper bin); expected (same shape): the
        sum over the run's exons of the mass the fitted model puts into each bin; n_empty (n_regions, n_samples): the run's exons that
        read NaN and are in no bin; chi2 (n_regions, n_samples): sum over the bins with expected > 0 of (observed - expected)^2 /
        expected, on the host -- with a chromosome or the whole exome as the region, the sample's calibration statistic.  rows as
        PowerMap.regions takes them; a row of (chrom, -1, -1) is a region with no exon inside: zeros."""
        rows, none, live = self._live_rows(rows)
        R, S, KB, n = rows.size, self.n_samples, self.probs.size + 1, int(live.size)
        obs, exp, empty = np.zeros((n, S, KB), dtype=np.int32), np.zeros((n, S, KB)), np.zeros((n, S), dtype=np.int32)
        check(lib().ed_quant_regions(self.handle, _ptr(live), n, _ptr(obs), _ptr(exp), _ptr(empty), C.c_void_p(self.stream or 0)))
        out = {"observed": np.zeros((R, S, KB), dtype=np.int32), "expected": np.zeros((R, S, KB)), "n_empty": np.zeros((R, S), dtype=np.int32)}
        at = np.flatnonzero(~none)
        out["observed"][at], out["expected"][at], out["n_empty"][at] = obs, exp, empty
        e = out["expected"]
        with np.errstate(all="ignore"):
            out["chi2"] = np.sum(np.where(e > 0, (out["observed"] - e) ** 2 / np.where(e > 0, e, 1.0), np.where(np.isnan(e), np.nan, 0.0)), axis=2)
        return out

    def exons(self):
        """(2, K, n_samples, n_exons): q, then below, of every exon; NaN where the total was skipped, the sample is outside the model or
        nothing was crossed"""
        out = np.zeros((2, self.probs.size, self.n_samples, self.plan.n_exons))
        check(lib().ed_quant_copy_exons(self.handle, _ptr(out), C.c_void_p(self.stream or 0)))
        return out

    def table(self, sample):
        """the sample's table: dict of totals (ascending, int32), q (K, n_totals) and below (K, n_totals)"""
        totals, values, k = self._table(sample, 2, self.probs.size)
        return {"totals": totals, "q": values[0, :, :k].copy(), "below": values[1, :, :k].copy()}

    def stats(self):
        """PowerMap.stats' counters (n_samples .. map_words), n_probs, tiles_walked, tiles_full (what full walks of the same jobs take), and its
        four times"""
        return self._stats("n_probs", "tiles_walked", "tiles_full")


def normal_range(chrom_off, start, end, test, ref, phi, expected, rows=None, probs=(0.025, 0.975), layout=0, device=0):
    """The normal range of a cohort: QuantileMap.exons() of the samples' map on a plan of (chrom_off, start, end) -- (2, K, n_samples,
    n_exons): the quantiles of every exon's test count under its sample's fitted model, then the mass below each -- and, with rows,
    a pair of that and QuantileMap.regions(rows).  Arguments as Plan and Plan.quantile_map take them."""
    plan = Plan(chrom_off, start, end, device=device)
    qm = None
    try:
        qm = plan.quantile_map(test, ref, phi, expected, probs, layout)
        ex = qm.exons()
        return ex if rows is None else (ex, qm.regions(rows))
    finally:
        if qm is not None:
            qm.free()
        plan.close()


# ---------------------------------------------------------------------------------------------
# draws from the fitted model: rbetabinom, null cohorts, and what a Bayes factor means on data without a CNV
# ---------------------------------------------------------------------------------------------
STREAM_NULL, STREAM_PLANTED = 0, 1
NULL_CALL_DTYPE = np.dtype([("replicate", "<i4")] + CALL_DTYPE.descr + CALL_INFO_DTYPE.descr)


def sim_geometry():
    """{walk_tile, occupancy_cap, max_total, region_tile, chunk} of the draw kernels (ed_sim_geometry); chunk: the cells one walk serves"""
    out = (C.c_int32 * 5)()
    check(lib().ed_sim_geometry(out))
    return dict(zip(("walk_tile", "occupancy_cap", "max_total", "region_tile", "chunk"), (int(v) for v in out)))


def _u32(x, what):
    a = np.atleast_1d(np.asarray(x))
    if a.dtype.kind not in "iu":
        raise ValueError("%s must be whole numbers" % what)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xffffffff):
        raise ValueError("%s must lie in 0 .. 2^32 - 1" % what)
    return a.astype(np.uint32).ravel()


def _seed64(seed):
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must lie in 0 .. 2^64 - 1")
    return seed


def runif53(seed, exon, sample, replicate, stream=0):
    """The uniforms behind the draws (include/exomedepth_amd.h: ed_runif53): Philox4x32-10 under the key of the 64-bit `seed` at the
    counters (exon, sample, replicate, stream), recycled to the longest; u = (2 k + 1) 2^-53 of 52 output bits: never 0, never 1.
    A float64 array."""
    args = [_u32(exon, "exon"), _u32(sample, "sample"), _u32(replicate, "replicate")]
    n = 0 if any(a.size == 0 for a in args) else max(a.size for a in args)
    args = [np.ascontiguousarray(np.resize(a, n)) for a in args]
    out = np.zeros(n)
    check(lib().ed_runif53(_seed64(seed), *[_ptr(a) if n else None for a in args], int(_u32(stream, "stream")[0]), n, _ptr(out) if n else None))
    return out


def rbetabinom_ab_u(u, size, shape1, shape2):
    """The draw from BetaBinomial(size, shape1, shape2) at a given uniform, element by element (ed_rbetabinom_ab_u): the smallest x in
    0 .. size whose distribution function exceeds u -- qbetabinom_ab's cut --, size where nothing crosses.  Recycled to the longest as
    qbetabinom_ab recycles; an int32 array.  -1 where u is outside [0, 1), a shape is not positive and finite or size is not a whole
    number in 0 .. max_total (sim_geometry)."""
    args = [_f64(np.atleast_1d(x)).ravel() for x in (u, size, shape1, shape2)]
    n = 0 if any(a.size == 0 for a in args) else max(a.size for a in args)
    args = [np.ascontiguousarray(np.resize(a, n)) for a in args]
    out = np.zeros(n, dtype=np.int32)
    check(lib().ed_rbetabinom_ab_u(*[_ptr(a) if n else None for a in args], n, _ptr(out) if n else None))
    return out


def rbetabinom_ab(size, shape1, shape2, seed, index=None, replicate=0):
    """Draws from BetaBinomial(size, shape1, shape2), recycled to the longest: element i is rbetabinom_ab_u at the uniform of the counter
    (index[i] -- i when index is None --, 0, replicate, 0) under `seed`.  The same (seed, index, replicate) gives the same draw in any
    call, whatever else the call holds."""
    args = [_f64(np.atleast_1d(x)).ravel() for x in (size, shape1, shape2)]
    idx = None if index is None else _u32(index, "index")
    sizes = [a.size for a in args] + ([idx.size] if idx is not None else [])
    n = 0 if any(k == 0 for k in sizes) else max(sizes)
    idx = np.arange(n, dtype=np.uint32) if idx is None else np.resize(idx, n)
    u = runif53(seed, idx, 0, replicate, STREAM_NULL) if n else np.zeros(0)
    return rbetabinom_ab_u(u, *[np.resize(a, n) for a in args])


def rbetabinom(size, phi, prob, seed, index=None, replicate=0):
    """rbetabinom_ab at shape1 = prob (1 - phi) / phi, shape2 = (1 - prob)(1 - phi) / phi, formed as qbetabinom forms them"""
    phi, prob = _f64(np.atleast_1d(phi)).ravel(), _f64(np.atleast_1d(prob)).ravel()
    n = 0 if not (phi.size and prob.size) else max(phi.size, prob.size)
    phi, prob = np.resize(phi, n), np.resize(prob, n)
    with np.errstate(all="ignore"):
        a, b = prob * (1. - phi) / phi, (1. - prob) * (1. - phi) / phi
    return rbetabinom_ab(size, a, b, seed, index, replicate)


def planted_prob(expected, ratio):
    """the proportion of test reads of a cell at copy ratio `ratio`: e c / (e c + 1 - e), the caller's own odds rule"""
    e, c = np.asarray(expected, dtype=np.float64), np.asarray(ratio, dtype=np.float64)
    return e * c / (e * c + 1 - e)


def _plant_cells(plant, n_exons, S, layout, phi, expected):
    """plant = (rows, ratio) -> (exon, sample, a, b) of every planted cell, a cell named twice taken once (its last row counts).  rows:
    records with sample, start_exon, end_exon (a call table), or (chrom, first, last) triples standing for every sample; ratio: a
    scalar or one per row, > 0 and finite."""
    rows, ratio = plant
    a = np.asarray(rows)
    per_sample = bool(a.dtype.names and "sample" in a.dtype.names)
    rows = _ratio_rows(rows) if per_sample else _region_rows(rows)
    ratio = np.asarray(ratio, dtype=np.float64)
    if ratio.ndim == 0:
        ratio = np.full(rows.size, float(ratio))
    if ratio.shape != (rows.size,):
        raise ValueError("plant: ratio must be a scalar or one value per row")
    if not np.all(np.isfinite(ratio) & (ratio > 0)):
        raise ValueError("plant: every ratio must be finite and > 0")
    first, last = rows["start_exon"].astype(np.int64), rows["end_exon"].astype(np.int64)
    if rows.size and (first.min() < 0 or last.max() >= n_exons or np.any(first > last)):
        raise ValueError("plant: a row does not lie inside the plan's exons")
    if per_sample and rows.size and (rows["sample"].min() < 0 or rows["sample"].max() >= S):
        raise ValueError("plant: a row names a sample outside the counts")
    cells = {}
    for r in range(rows.size):
        for s in ([int(rows["sample"][r])] if per_sample else range(S)):
            for e in range(int(first[r]), int(last[r]) + 1):
                cells[(e, s)] = ratio[r]
    keys = sorted(cells)
    ce = np.array([k[0] for k in keys], dtype=np.int32)
    cs = np.array([k[1] for k in keys], dtype=np.int32)
    c = np.array([cells[k] for k in keys], dtype=np.float64)
    ph, pr = phi[cs], planted_prob(expected[cs], c)
    with np.errstate(all="ignore"):
        return ce, cs, pr * (1. - ph) / ph, (1. - pr) * (1. - ph) / ph


class SimulatedCounts(tuple):
    """(test*, ref*) of Plan.simulate: two DeviceArrays of int32 counts in the input's layout, and .stats() of the draw"""

    def __new__(cls, test, ref, stats):
        self = super().__new__(cls, (test, ref))
        self._stats = stats
        return self

    def stats(self):
        """n_jobs (occupied (sample, total) pairs), tiles_walked, tiles_full (one full walk per 64 cells of the same jobs), cells_drawn,
        cells_skipped (kept as they were: a total outside 0 .. max_total, or a sample whose shapes are outside the model),
        n_bad_samples, n_planted; occupancy_ms, grouping_ms, walk_ms, host-timed between waits"""
        return dict(self._stats)

    def free(self):
        for d in self:
            d.free()


def _simulate(plan, test, ref, phi, expected, seed, replicate=0, sample0=0, layout=0, stream=None, plant=None):
    phi, expected = _f64(np.atleast_1d(phi)).ravel(), _f64(np.atleast_1d(expected)).ravel()
    S = int(phi.size)
    if expected.size != S:
        raise ValueError("phi and expected must have one value per sample")
    E = plan.n_exons
    for x in (test, ref):
        _check_counts_shape(x, E, S, layout)
    cells = _plant_cells(plant, E, S, layout, phi, expected) if plant is not None else None
    shape = (S, E) if layout else (E, S)
    out = [DeviceArray(nbytes=max(E * S, 1) * 4) for _ in range(2)]
    try:
        for d in out:
            d.host_dtype, d.shape = np.dtype(np.int32), shape
        with _staged() as keep:
            pt, pr = _device_pointer(test, np.int32, keep), _device_pointer(ref, np.int32, keep)
            st = C.c_void_p(stream or 0)
            check(lib().ed_plan_simulate(plan.handle, pt, pr, _ptr(phi), _ptr(expected), S, int(sample0), int(layout), _seed64(seed),
                                         int(replicate), out[0].ptr, out[1].ptr, st))
            cnt, ms = (C.c_int64 * 6)(), (C.c_double * 3)()
            check(lib().ed_sim_stats(cnt, ms))
            stats = dict(zip(("n_jobs", "tiles_walked", "tiles_full", "cells_drawn", "cells_skipped", "n_bad_samples"), (int(v) for v in cnt)))
            stats.update(zip(("occupancy_ms", "grouping_ms", "walk_ms"), (float(v) for v in ms)))
            stats["n_planted"] = 0
            if cells is not None and cells[0].size:
                ce, cs, a, b = cells
                check(lib().ed_plan_simulate_cells(plan.handle, pt, pr, _ptr(ce), _ptr(cs), _ptr(a), _ptr(b), int(ce.size), S, int(sample0),
                                                   int(layout), _seed64(seed), int(replicate), STREAM_PLANTED, out[0].ptr, out[1].ptr, st))
                stats["n_planted"] = int(ce.size)
    except Exception:
        for d in out:
            d.free()
        raise
    return SimulatedCounts(out[0], out[1], stats)


def null_call_table(chrom_off, start, end, test, ref, phi, expected, replicates, seed, refit=True, transition_probability=1e-4,
                    expected_CNV_length=50000, plant=None, device=0):
    """What the unchanged pipeline calls on data drawn from the fitted model itself.  Per replicate (replicates: a count, or the
    replicate numbers): draw the cohort (Plan.simulate; with plant = (rows, ratio) the planted cells on top), then -- refit=True -- fit
    phi and expected on the draw as a real run would (Batch.fit) and run (Batch.run), or run at the given parameters.  test / ref:
    (n_exons, S) int32 counts.  Returns a dict: calls, a NULL_CALL_DTYPE array -- every replicate's call table with call_info's columns
    (BF among them) under a `replicate` column --; replicates (R,); phi, expected (R, S), the parameters each replicate ran at;
    n_samples; n_null_samples = R x S, what false_calls_per_sample divides by; stats, each draw's SimulatedCounts.stats()."""
    reps = list(range(int(replicates))) if np.ndim(replicates) == 0 else [int(r) for r in replicates]
    phi, expected = _f64(np.atleast_1d(phi)).ravel(), _f64(np.atleast_1d(expected)).ravel()
    S = int(phi.size)
    plan = Plan(chrom_off, start, end, transition_probability, expected_CNV_length, device)
    batch = None
    tables, phis, exps, stats = [], [], [], []
    try:
        batch = Batch(plan, S)
        with _staged() as keep:
            for x in (test, ref):
                _check_counts_shape(x, plan.n_exons, S, 0)
            pt, pr = _RawDevice(_device_pointer(test, np.int32, keep).value), _RawDevice(_device_pointer(ref, np.int32, keep).value)
            for r in reps:
                sim = plan.simulate(pt, pr, phi, expected, seed, replicate=r, plant=plant)
                try:
                    if refit:
                        dp, de = DeviceArray(nbytes=S * 8), DeviceArray(nbytes=S * 8)
                        keep.extend([dp, de])
                        batch.fit(sim[0], sim[1], dp, de)
                        batch.run(sim[0], sim[1], dp, de)
                        calls, info = batch.calls(), batch.call_info()
                        phis.append(dp.to_host(np.float64, (S,)))
                        exps.append(de.to_host(np.float64, (S,)))
                    else:
                        batch.run(sim[0], sim[1], phi, expected)
                        calls, info = batch.calls(), batch.call_info()
                        phis.append(phi.copy())
                        exps.append(expected.copy())
                finally:
                    sim.free()
                stats.append(sim.stats())
                t = np.zeros(calls.size, dtype=NULL_CALL_DTYPE)
                t["replicate"] = r
                for k in CALL_DTYPE.names:
                    t[k] = calls[k]
                for k in CALL_INFO_DTYPE.names:
                    t[k] = info[k]
                tables.append(t)
    finally:
        if batch is not None:
            batch.close()
        plan.close()
    R = len(reps)
    return {"calls": np.concatenate(tables) if tables else np.zeros(0, dtype=NULL_CALL_DTYPE), "replicates": np.array(reps, dtype=np.int64),
            "phi": np.array(phis).reshape(R, S), "expected": np.array(exps).reshape(R, S), "n_samples": S, "n_null_samples": R * S,
            "stats": stats}


def false_calls_per_sample(bf, null_bf, n_null_samples, kind=None, null_kind=None):
    """For every real call: #{null calls of its type with BF >= its BF} / n_null_samples -- the number of calls at least this strong
    that the pipeline is expected to make in one exome with no CNV in it.  bf: the real calls' Bayes factors; null_bf: those of a null
    table (null_call_table's calls["BF"]); n_null_samples: the samples the null table was drawn for (replicates x samples).  kind /
    null_kind: the calls' types (1 deletion, 2 duplication, or any labels); both or neither; without them every null call counts.  On the
    host: a sort and a binary search per type.  NaN where a real BF is NaN; a null BF that is NaN counts nowhere."""
    bf, null_bf = np.asarray(bf, dtype=np.float64).ravel(), np.asarray(null_bf, dtype=np.float64).ravel()
    if not n_null_samples > 0:
        raise ValueError("n_null_samples must be positive")
    if (kind is None) != (null_kind is None):
        raise ValueError("kind and null_kind go together")
    if kind is None:
        kind, null_kind = np.zeros(bf.size, dtype=np.int64), np.zeros(null_bf.size, dtype=np.int64)
    kind, null_kind = np.asarray(kind).ravel(), np.asarray(null_kind).ravel()
    if kind.size != bf.size or null_kind.size != null_bf.size:
        raise ValueError("one type per call")
    out = np.zeros(bf.size)
    for t in np.unique(kind):
        mine = kind == t
        pool = np.sort(null_bf[(null_kind == t) & ~np.isnan(null_bf)])
        out[mine] = (pool.size - np.searchsorted(pool, bf[mine], "left")) / float(n_null_samples)
    out[np.isnan(bf)] = np.nan
    return out


def chromosome_order(chromosome, start, end):
    """Return (order, chrom_levels, chrom_codes_sorted, chrom_off).  Levels are '1'..'22' first (those
    present), then the other names in first-seen order; exons are ordered by (level, midpoint) with
    ties kept in input order, as R's order() does."""
    chromosome = np.asarray([str(c) for c in chromosome], dtype=object)
    used = []
    seen = set()
    for c in chromosome:
        if c not in seen:
            seen.add(c)
            used.append(c)
    autos = [str(i) for i in range(1, 23)]
    levels = [c for c in autos if c in seen] + [c for c in used if c not in autos]
    code_of = {c: i for i, c in enumerate(levels)}
    codes = np.fromiter((code_of[c] for c in chromosome), dtype=np.int64, count=chromosome.size)
    mid = 0.5 * (np.asarray(start, dtype=np.float64) + np.asarray(end, dtype=np.float64))
    order = np.lexsort((mid, codes))  # stable: last key is primary
    sc = codes[order]
    chrom_off = np.zeros(len(levels) + 1, dtype=np.int32)
    for i in range(len(levels)):
        chrom_off[i + 1] = chrom_off[i] + int(np.sum(sc == i))
    return order, levels, sc, chrom_off


class ExomeDepth:
    """Mirror of the reference's S4 class (R/class_definition.R:36-46) for one test sample.

    phi / expected: if given, the fixed dispersion and expected proportion (the reference gets them
    from aod::betabin, :118, :168); if omitted they are fitted on the GPU (ed_batch_fit)."""

    def __init__(self, test, reference, phi=None, expected=None, prop_tumor=1.0, subset_for_speed=None, phi_bins=1,
                 data=None, formula="cbind(test, reference) ~ 1", verbose=False):
        test = np.asarray(test, dtype=np.float64)
        reference = np.asarray(reference, dtype=np.float64)
        if test.size != reference.size:
            raise ValueError("Length of test and numeric must match")   # R/class_definition.R:92
        self.test, self.reference = test, reference
        self.prop_tumor = float(prop_tumor)
        self.phi = np.zeros(0)
        self.expected = np.zeros(0)
        self.likelihood = np.zeros((0, 3))
        self.annotations = None
        self.CNV_calls = None
        self.cor_test_reference = None
        if np.sum(test > 5) < 5:                                       # R/class_definition.R:94-97
            if verbose:
                print("It looks like the test samples has only %d bins with more than 5 reads." % np.sum(test > 5))
            return
        n = test.size
        self.formula = formula
        terms = _formula_terms(formula)
        if (phi is None or expected is None) and terms:                 # covariates: `data` columns named in the formula
            if phi_bins != 1 or subset_for_speed is not None:
                raise NotImplementedError("covariates together with phi.bins > 1 or subset.for.speed are not implemented")
            if data is None:
                raise ValueError("the formula refers to covariates but no `data` was given")
            X = np.stack([np.asarray(data[t], dtype=np.float64) for t in terms], axis=1)
            if X.shape[0] != n:
                raise ValueError("`data` must have one row per exon")
            phi, expected = fit_betabin_cov(_as_r_integer(test), _as_r_integer(reference), X)
        if (phi is None or expected is None) and phi_bins != 1:        # R/class_definition.R:120-147
            if subset_for_speed is not None:
                raise ValueError("Subset for speed option is not compatible with variable phi. This will be fixed later on "
                                 "but for now please adapt your code.")
            phi, expected = fit_betabin_bins(_as_r_integer(test), _as_r_integer(reference), int(phi_bins))
        if phi is None or expected is None:
            rows = np.arange(n)
            if subset_for_speed is not None:                           # R/class_definition.R:107-113
                sub = np.atleast_1d(np.asarray(subset_for_speed))
                if sub.size == 1 and np.issubdtype(sub.dtype, np.number):
                    by = int(np.floor(n / float(sub[0])))
                    if by < 1:
                        raise ValueError("wrong sign in 'by' argument")   # R's seq() error for by = 0
                    rows = np.arange(0, n, by)                         # seq(from = 1, to = nrow, by = floor(nrow / n))
                else:
                    sub = sub.astype(np.int64)
                    rows = sub[(sub >= 1) & (sub <= n)] - 1            # keep existing (1-based) rows only
            phi, expected = fit_betabin(_as_r_integer(test[rows]), _as_r_integer(reference[rows]))
        self.phi = np.full(n, float(phi)) if np.ndim(phi) == 0 else _f64(phi)
        self.expected = np.full(n, float(expected)) if np.ndim(expected) == 0 else _f64(expected)
        self.likelihood = np.array(get_loglike_matrix(self.phi, self.expected, _as_r_integer(reference + test),
                                                      _as_r_integer(test), mixture=prop_tumor))

    def TestCNV(self, chromosome, start, end, type):
        """reference R/class_definition.R:243-256 (needs CallCNVs annotations for the positions)."""
        if type not in ("deletion", "duplication"):
            raise ValueError("type must be either duplication or deletion\n")
        if self.annotations is None:
            raise ValueError("This function cannot be used if the position of the exons/DNA segments was not included")
        a = self.annotations
        which = (a["chromosome"] == str(chromosome)) & (a["start"] >= start) & (a["end"] <= end)
        col = 0 if type == "deletion" else 2
        return float(np.sum(self.likelihood[which, col] - self.likelihood[which, 1]))

    def CallCNVs(self, chromosome, start, end, name, transition_probability=1e-4, expected_CNV_length=50000, posterior=False, breakpoints=False,
                 copy_number=False):
        """reference R/class_definition.R:311-419: order exons, one Viterbi chain per chromosome,
        call table with start.p/end.p (1-based, global), type, nexons, start, end, chromosome, id.

        One intentional difference on UNSORTED input: the reference reorders x@test, x@reference, x@annotations and
        x@likelihood (:327-336) but not x@expected / x@phi, and then indexes x@expected with the reordered positions
        (:396) -- with a per-exon `expected` (covariates in the formula) its reads.expected is then summed over the wrong
        exons.  Here phi and expected are reordered with everything else, so reads.expected belongs to the call's exons.
        With the default formula (expected constant) the two agree.

        posterior=True adds four columns from the HMM's forward-backward pass (not in the reference): post.mean / post.min, the mean
        and the smallest posterior probability of the call's type over its exons; post.all, the log-probability that every exon of
        the call is in that state; log.evidence, the log-evidence of the call's chromosome.

        breakpoints=True (level 0.95) or a level in (0, 1) appends ten columns, after whatever else the call has: the credible intervals
        of the call's two breakpoints from the same posterior (Batch.call_bounds).  start.p.lo <= start.p.hi <= end.p.lo <= end.p.hi are
        exon positions, 1-based like start.p; start.lo / start.hi are those exons' start coordinates, end.lo / end.hi their end
        coordinates; start.keep / end.keep the probability that the run of the call's state through its best-supported exon reaches at
        least the call's own first / last exon.  A call that cannot be walked keeps its own positions and NaN.

        copy_number=True appends six columns from the call's likelihood profile over the copy ratio (call_copy_number with its defaults,
        on the run's own counts): copy.ratio, the maximum-likelihood copy ratio, with its 95 % profile-likelihood interval copy.ratio.lo /
        copy.ratio.hi; copy.number, the best of CN 0 .. 4; BF.copy.number, the log10 Bayes factor of that copy number against the
        runner-up; mosaic.gain, twice the log-likelihood the free ratio gains over the best copy number (chi^2_1 when the call has an
        integer copy number).  Needs one (phi, expected) for the sample: not available with phi.bins > 1 or covariates."""
        if breakpoints is None or isinstance(breakpoints, (bool, np.bool_)):
            level = 0.95 if breakpoints else None
        else:
            level = float(breakpoints)
        if self.phi.size == 0:
            self.CNV_calls = []
            return self
        n = self.likelihood.shape[0]
        if not (len(start) == len(chromosome) == len(end) == len(name)):
            raise ValueError("Chromosome, name, start and end vector must have the same lengths.\n")
        if n != len(chromosome):
            raise ValueError("The annotation vectors must have the same length as the data in the ExomeDepth x")
        order, levels, codes, chrom_off = chromosome_order(chromosome, start, end)
        start = np.asarray(start)[order]
        end = np.asarray(end)[order]
        name = np.asarray(name, dtype=object)[order]
        chrom_sorted = np.asarray([str(c) for c in chromosome], dtype=object)[order]
        if np.any(order != np.arange(n)):
            self.test = self.test[order]
            self.reference = self.reference[order]
            self.likelihood = self.likelihood[order]
            self.phi = self.phi[order]
            self.expected = self.expected[order]
        self.annotations = {"name": name, "chromosome": chrom_sorted, "start": start, "end": end}
        self.cor_test_reference = float(np.corrcoef(self.test, self.reference)[0, 1])
        constant = bool(np.all(self.phi == self.phi[0]) and np.all(self.expected == self.expected[0]))
        if copy_number and not constant:
            raise NotImplementedError("copy_number=True needs one (phi, expected) for the sample: phi.bins > 1 and covariates are not served")
        ccn = None
        if constant:
            plan = Plan(chrom_off, start, end, transition_probability, expected_CNV_length)
            batch = Batch(plan, 1)
            try:
                # the likelihood is recomputed on the device from the same inputs -- prop.tumor included -- hence
                # bit-identical to the slot the reference runs its Viterbi on (R/class_definition.R:364)
                batch.run(_as_r_integer(self.test).reshape(n, 1), _as_r_integer(self.reference).reshape(n, 1),
                          self.phi[:1], self.expected[:1], mixture=self.prop_tumor)
                raw = batch.calls()
                self.Viterbi_path = batch.path()[:, 0].astype(np.int64)
                cpost = batch.call_posterior() if posterior else None
                cbnd = batch.call_bounds(level) if level is not None else None
                if copy_number and len(raw):
                    ccn = _ratio_search(batch._call_ratio_doses, len(raw), 3, 0.95, 0.05)
            finally:
                batch.close()
                plan.close()
        else:
            # per-exon phi (phi.bins > 1) or expected: the likelihood slot itself goes through the .Call-shaped
            # entry, chromosome by chromosome, exactly as R/class_definition.R:343-374 does
            tp = transition_probability
            T = np.array([[1. - tp, tp / 2., tp / 2.], [0.5, 0.5, 0.], [0.5, 0., 0.5]])
            raw = []
            self.Viterbi_path = np.zeros(n, dtype=np.int64)
            for c in range(len(chrom_off) - 1):
                lo, hi = int(chrom_off[c]), int(chrom_off[c + 1])
                if hi <= lo:
                    continue
                ll = np.vstack([[-np.inf, 0., -np.inf], self.likelihood[lo:hi][:, [1, 0, 2]], [-100., 0., -100.]])
                pos = np.concatenate([[start[lo] - 2 * expected_CNV_length], start[lo:hi],
                                      [end[hi - 1] + 2 * expected_CNV_length]])
                res = viterbi_hmm(T, ll, _as_r_integer(pos.astype(np.float64)), expected_CNV_length)
                self.Viterbi_path[lo:hi] = res["Viterbi.path"][1:-1]
                for r in res["calls"]:
                    raw.append({"start_exon": int(r["start.p"]) - 2 + lo, "end_exon": int(r["end.p"]) - 2 + lo,
                                "type": int(r["type"]), "nexons": int(r["nexons"]), "chrom": c})
            cpost = cbnd = None
            if posterior or level is not None:
                rows = np.zeros(len(raw), dtype=CALL_DTYPE)
                for k in ("chrom", "start_exon", "end_exon", "type", "nexons"):
                    rows[k] = [r[k] for r in raw]
                plan = Plan(chrom_off, start, end, transition_probability, expected_CNV_length)
                try:
                    post = plan.posterior(np.ascontiguousarray(self.likelihood).reshape(n, 3, 1), 1)
                    cpost = post.call_posterior(rows) if posterior else None
                    cbnd = post.call_bounds(rows, level) if level is not None else None
                    post.free()
                finally:
                    plan.close()
        calls = []
        total = self.test + self.reference
        for r in raw:
            s, e = int(r["start_exon"]), int(r["end_exon"])
            typ = ["deletion", "duplication"][int(r["type"]) - 1]
            col = 0 if typ == "deletion" else 2
            bf = float(np.sum(self.likelihood[s:e + 1, col] - self.likelihood[s:e + 1, 1]))
            reads_expected = int(np.sum(total[s:e + 1] * self.expected[s:e + 1]))
            reads_observed = float(np.sum(self.test[s:e + 1]))
            with np.errstate(divide="ignore", invalid="ignore"):   # obs / 0 is Inf in R (and in k_call_info), 0 / 0 NaN
                ratio = float(np.float64(reads_observed) / np.float64(reads_expected))
            cid = ("chr%s:%d-%d" % (chrom_sorted[s], start[s], end[e])).replace("chrchr", "chr")
            calls.append({"start.p": s + 1, "end.p": e + 1, "type": typ, "nexons": int(r["nexons"]),
                          "start": int(start[s]), "end": int(end[e]), "chromosome": chrom_sorted[s], "id": cid,
                          "BF": _signif(np.log10(np.e) * bf, 3), "reads.expected": reads_expected,
                          "reads.observed": reads_observed,
                          "reads.ratio": _signif(ratio, 3)})
            if cpost is not None:
                q = cpost[len(calls) - 1]
                calls[-1].update({"post.mean": float(q["post_mean"]), "post.min": float(q["post_min"]),
                                  "post.all": float(q["log_p_all"]), "log.evidence": float(q["log_evidence"])})
            if cbnd is not None:
                q = cbnd[len(calls) - 1]
                slo, shi, elo, ehi = (int(q[k]) for k in ("start_lo", "start_hi", "end_lo", "end_hi"))
                calls[-1].update({"start.p.lo": slo + 1, "start.p.hi": shi + 1, "end.p.lo": elo + 1, "end.p.hi": ehi + 1,
                                  "start.lo": int(start[slo]), "start.hi": int(start[shi]), "end.lo": int(end[elo]), "end.hi": int(end[ehi]),
                                  "start.keep": float(np.exp(q["log_keep_start"])), "end.keep": float(np.exp(q["log_keep_end"]))})
            if ccn is not None:
                i = len(calls) - 1
                bf = np.sort(ccn["log10_bf_cn"][i])          # (a NaN row stays NaN throughout)
                calls[-1].update({"copy.ratio": float(ccn["ratio"][i]), "copy.ratio.lo": float(ccn["ratio_lo"][i]),
                                  "copy.ratio.hi": float(ccn["ratio_hi"][i]), "copy.number": int(ccn["cn"][i]),
                                  "BF.copy.number": float(bf[-1] - bf[-2]), "mosaic.gain": float(ccn["mosaic_gain"][i])})
        self.CNV_calls = calls
        return self

    def fit_transitions(self, chromosome, start, end, transition_probability=1e-4, expected_CNV_length=50000.0, **options):
        """Maximum-likelihood transition_probability and expected_CNV_length of this sample's likelihood slot (fit_transitions on one
        sample; not in the reference).  Exons are ordered as CallCNVs orders them; nothing of the object is changed.  Returns
        fit_transitions' dict."""
        n = self.likelihood.shape[0]
        if not (len(start) == len(chromosome) == len(end) == n):
            raise ValueError("The annotation vectors must have the same length as the data in the ExomeDepth x")
        order, _, _, chrom_off = chromosome_order(chromosome, start, end)
        ll = np.ascontiguousarray(np.asarray(self.likelihood, dtype=np.float64)[order]).reshape(n, 3, 1)
        return fit_transitions(chrom_off, np.asarray(start)[order], np.asarray(end)[order], ll, 1, transition_probability,
                               expected_CNV_length, **options)

    def fit_prop_tumor(self, chromosome, start, end, **options):
        """Maximum-likelihood tumour fraction of this pair (test = tumour, reference = normal) at the object's phi and expected:
        fit_prop_tumor on one pair (not in the reference).  Exons are ordered as CallCNVs orders them; nothing of the object is changed.
        Returns fit_prop_tumor's dict (arrays of length 1)."""
        n = self.test.size
        if not (len(start) == len(chromosome) == len(end) == n):
            raise ValueError("The annotation vectors must have the same length as the data in the ExomeDepth x")
        if self.phi.size == 0:
            raise ValueError("the object has no fitted phi / expected (too few bins with reads)")
        if not (np.all(self.phi == self.phi[0]) and np.all(self.expected == self.expected[0])):
            raise NotImplementedError("fit_prop_tumor with a per-exon phi or expected (phi.bins > 1, covariates) is not implemented")
        order, _, _, chrom_off = chromosome_order(chromosome, start, end)
        return fit_prop_tumor(chrom_off, np.asarray(start)[order], np.asarray(end)[order], _as_r_integer(self.test[order]),
                              _as_r_integer(self.reference[order]), phi=self.phi[:1], expected=self.expected[:1], **options)

    def detection_power(self, chromosome, start, end, regions=None, threshold=None, transition_probability=1e-4, expected_CNV_length=50000.0):
        """Detection power of this sample at the object's phi, expected and prop_tumor (detection_power on one sample; not in the
        reference): a POWER_DTYPE array, one row per region.  regions: (chromosome, start, end) coordinate triples, mapped to exon runs
        by region_runs; None: the object's own CNV_calls (after CallCNVs, whose exon order the object then has), one row per call.
        Exons are ordered as CallCNVs orders them; nothing of the object is changed."""
        n = self.test.size
        if not (len(start) == len(chromosome) == len(end) == n):
            raise ValueError("The annotation vectors must have the same length as the data in the ExomeDepth x")
        if self.phi.size == 0:
            raise ValueError("the object has no fitted phi / expected (too few bins with reads)")
        if not (np.all(self.phi == self.phi[0]) and np.all(self.expected == self.expected[0])):
            raise NotImplementedError("detection_power with a per-exon phi or expected (phi.bins > 1, covariates) is not implemented: "
                                      "there the value is no longer a function of the exon's total")
        order, _, _, chrom_off = chromosome_order(chromosome, start, end)
        s_start, s_end = np.asarray(start)[order], np.asarray(end)[order]
        if regions is None:
            if self.CNV_calls is None:
                raise ValueError("regions=None needs the object's CNV_calls: run CallCNVs first")
            rows = np.zeros(len(self.CNV_calls), dtype=CALL_DTYPE)
            first = np.array([c["start.p"] - 1 for c in self.CNV_calls], dtype=np.int64)
            rows["start_exon"], rows["end_exon"] = first, [c["end.p"] - 1 for c in self.CNV_calls]
            rows["chrom"] = np.searchsorted(chrom_off, first, "right") - 1
        else:
            rows = region_runs(np.asarray([str(c) for c in chromosome], dtype=object)[order], s_start, s_end, regions)
        out = detection_power(chrom_off, s_start, s_end, _as_r_integer(self.test[order]).reshape(n, 1),
                              _as_r_integer(self.reference[order]).reshape(n, 1), self.phi[:1], self.expected[:1], rows, mixture=self.prop_tumor,
                              threshold=threshold, transition_probability=transition_probability, expected_CNV_length=expected_CNV_length)
        return out[:, 0]

    def normal_range(self, sequence, xlim, count_threshold=10, probs=(0.025, 0.975)):
        """The data frame the reference's plot method draws (R/plot_CNVs_method.R:33-63), without the drawing: for the exons of
        chromosome `sequence` wholly inside xlim whose expected test count (test + reference) * expected exceeds count_threshold, a dict
        of columns middle, ratio (observed / expected proportion of test reads), test, reference, total_counts, phi, my_min_norm /
        my_max_norm = qbetabinom(probs[0] / probs[1], total_counts, phi, expected) exon by exon -- a per-exon phi (phi.bins > 1) as the
        reference takes it (:51) --, my_min_norm_prop / my_max_norm_prop = those over total_counts, and outside (not in the reference):
        -1 / 0 / +1 where the ratio lies below / inside / above the two proportions over expected, the band the plot draws.  None where
        no exon is selected (the reference warns and returns NULL).  Needs the annotations CallCNVs stores."""
        if self.annotations is None:
            raise ValueError("This function cannot be used if the position of the exons/DNA segments was not included")
        if len(probs) != 2 or not probs[0] < probs[1]:
            raise ValueError("probs must be the lower and the upper probability of the band")
        a = self.annotations
        total = self.test + self.reference
        sel = np.flatnonzero((np.asarray(a["chromosome"], dtype=object) == str(sequence)) & (np.asarray(a["start"]) >= xlim[0]) &
                             (np.asarray(a["end"]) <= xlim[1]) & (total * self.expected > count_threshold))
        if sel.size == 0:
            return None
        test, reference, expected, phi = self.test[sel], self.reference[sel], self.expected[sel], self.phi[sel]
        out = {"middle": 0.5 * (np.asarray(a["start"], dtype=np.float64)[sel] + np.asarray(a["end"], dtype=np.float64)[sel])}
        with np.errstate(divide="ignore", invalid="ignore"):
            out["ratio"] = (test / (reference + test)) / expected
            out.update({"test": test, "reference": reference, "total_counts": test + reference, "phi": phi})
            out["my_min_norm"] = qbetabinom(probs[0], out["total_counts"], phi, expected)
            out["my_max_norm"] = qbetabinom(probs[1], out["total_counts"], phi, expected)
            out["my_min_norm_prop"] = out["my_min_norm"] / out["total_counts"]
            out["my_max_norm_prop"] = out["my_max_norm"] / out["total_counts"]
            out["outside"] = (out["ratio"] > out["my_max_norm_prop"] / expected).astype(np.int8) - (out["ratio"] < out["my_min_norm_prop"] / expected).astype(np.int8)
        return out

    def null_calls(self, chromosome, start, end, replicates=100, seed=0, refit=True, transition_probability=1e-4, expected_CNV_length=50000.0,
                   plant=None):
        """What CallCNVs calls on draws from this sample's own fitted model (null_call_table on one sample; not in the reference): the
        dict null_call_table returns, its calls' exon indices in CallCNVs' order.  With the object's own calls,
        false_calls_per_sample([c["BF"] ...], out["calls"]["BF"], out["n_null_samples"], kinds, out["calls"]["type"]) says how many calls
        that strong an exome without a CNV is expected to give.  Nothing of the object is changed."""
        n = self.test.size
        if not (len(start) == len(chromosome) == len(end) == n):
            raise ValueError("The annotation vectors must have the same length as the data in the ExomeDepth x")
        if self.phi.size == 0:
            raise ValueError("the object has no fitted phi / expected (too few bins with reads)")
        if not (np.all(self.phi == self.phi[0]) and np.all(self.expected == self.expected[0])):
            raise NotImplementedError("null_calls with a per-exon phi or expected (phi.bins > 1, covariates) is not implemented")
        order, _, _, chrom_off = chromosome_order(chromosome, start, end)
        return null_call_table(chrom_off, np.asarray(start)[order], np.asarray(end)[order], _as_r_integer(self.test[order]).reshape(n, 1),
                               _as_r_integer(self.reference[order]).reshape(n, 1), self.phi[:1], self.expected[:1], replicates, seed, refit=refit,
                               transition_probability=transition_probability, expected_CNV_length=expected_CNV_length, plant=plant)

    def AnnotateExtra(self, reference_annotation, min_overlap=0.5, column_name=None):
        """reference R/annotate_extra.R:41-73: adds `column_name` to every row of CNV_calls -- the `names` of the annotation's intervals the
        call overlaps by more than min_overlap x (end - start), joined with ",", or None where R leaves NA (no such interval).
        reference_annotation: an Annotation built with names (what stands for the GRanges and its `names` metadata column).  The names
        of one call come in genomic order of the annotation's intervals (Annotation.overlaps)."""
        if column_name is None:
            raise TypeError('argument "column_name" is missing, with no default')     # as the R generic: no default
        if not isinstance(reference_annotation, Annotation) or reference_annotation.names is None:
            raise ValueError("reference_annotation must be an Annotation with names")
        calls = self.CNV_calls or []
        if calls:
            _, offsets, hits = reference_annotation.overlaps([c["chromosome"] for c in calls], [c["start"] for c in calls],
                                                             [c["end"] for c in calls], min_overlap=min_overlap)
            for c, v in zip(calls, _join_hit_names(reference_annotation.names, offsets, hits)):
                c[column_name] = v
        return self


def somatic_CNV_call(normal, tumor, prop_tumor=1.0, chromosome=None, start=None, end=None, names=None):
    """reference R/class_definition.R:442-461: one matched tumour / normal pair -- new('ExomeDepth', test = tumor, reference = normal,
    prop.tumor = prop_tumor) (the fit ignores prop_tumor; the likelihood sees it) followed by CallCNVs(transition.probability = 1e-4)
    with the default expected.CNV.length.  Returns the ExomeDepth object.  A cohort of pairs, each at its own tumour fraction:
    Cohort.run_host / MultiDevice.run_host with test = tumours, ref = normals and one mixture per column.

    prop_tumor = "fit" (not in the reference): the fraction is first estimated by maximum likelihood (ExomeDepth.fit_prop_tumor, at the
    transition parameters of the call).  The estimate is used where the pair is informative; where it is not -- no somatic CNV, too low
    a fraction, too shallow data: see fit_prop_tumor -- 1.0 is used and a line on stderr says why.  The fit is recorded on the returned
    object as prop_tumor_fit.  A numeric prop_tumor behaves as it always has."""
    if chromosome is None or start is None or end is None or names is None:
        raise ValueError("chromosome, start, end and names are required (R/class_definition.R:442)")
    fit_it = isinstance(prop_tumor, str)
    if fit_it and prop_tumor != "fit":
        raise ValueError('prop_tumor is a number or "fit"')
    if not fit_it and np.ndim(prop_tumor) != 0:
        raise ValueError("prop_tumor is one value for the pair")
    sys.stderr.write("Warning: this function is largely untested and experimental\n")     # message() lines of :444-451
    sys.stderr.write("Initializing the exomeDepth object\n")
    if not fit_it:
        x = ExomeDepth(test=tumor, reference=normal, prop_tumor=prop_tumor, formula="cbind(test, reference) ~ 1")
        sys.stderr.write("Now calling the CNVs\n")
        return x.CallCNVs(chromosome, start, end, names, transition_probability=1e-4)
    x = ExomeDepth(test=tumor, reference=normal, prop_tumor=1.0, formula="cbind(test, reference) ~ 1")   # (the fit ignores prop_tumor)
    fit = None
    if x.phi.size:
        sys.stderr.write("Fitting the tumour fraction\n")
        fit = x.fit_prop_tumor(chromosome, start, end, transition_probability=1e-4)
        if fit["informative"][0]:
            m = float(fit["prop_tumor"][0])
            sys.stderr.write("Fitted prop_tumor = %.4f (se %.2g, gain %.1f log units over prop_tumor = 0)\n" % (m, fit["se"][0], fit["gain"][0]))
            x = ExomeDepth(test=tumor, reference=normal, phi=float(x.phi[0]), expected=float(x.expected[0]), prop_tumor=m,
                           formula="cbind(test, reference) ~ 1")
        else:
            sys.stderr.write("The tumour fraction is not identifiable for this pair (gain %.2f log units over prop_tumor = 0: no somatic CNV, "
                             "a low fraction or shallow data); using prop_tumor = 1\n" % fit["gain"][0])
    x.prop_tumor_fit = fit
    sys.stderr.write("Now calling the CNVs\n")
    return x.CallCNVs(chromosome, start, end, names, transition_probability=1e-4)


# ---------------------------------------------------------------------------------------------
# annotation overlap (reference R/annotate_extra.R:41-73) and the cohort's self-join
# ---------------------------------------------------------------------------------------------
def _join_hit_names(names, offsets, hits):
    """paste(names[hits of call q], collapse = ",") per call, None where the call has no hit (R/annotate_extra.R:67-71)"""
    return [",".join(str(names[int(h)]) for h in hits[int(offsets[q]):int(offsets[q + 1])]) if offsets[q + 1] > offsets[q] else None
            for q in range(len(offsets) - 1)]


def annot_geometry():
    """{wide_threshold, queries_per_workgroup, wave_pass, scan_block} of the join kernels (ed_annot_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_annot_geometry(out))
    return dict(zip(("wide_threshold", "queries_per_workgroup", "wave_pass", "scan_block"), (int(v) for v in out)))


def _coords(start, end):
    """int32 coordinates; a value that int32 cannot hold is refused here instead of wrapping silently"""
    out = []
    for a in (np.asarray(start), np.asarray(end)):
        if a.size:
            if a.dtype.kind not in "iu" and not (a.dtype.kind == "f" and np.all(a == np.trunc(a))):
                raise ValueError("interval coordinates must be integers")
            if a.min() < -2**31 or a.max() > 2**31 - 1:
                raise ValueError("interval coordinates must fit int32")
        out.append(_i32(a).ravel())
    return out


class Annotation:
    """An annotation track on the device (ed_annot): intervals `chromosome`, `start`, `end` (closed, 0 <= start <= end), optionally with
    `names` (what AnnotateExtra pastes), a `group` and a `kind` per interval (int32; the two optional filters of overlaps()).
    Chromosome names are mapped to ids here; "chr1" and "1" are DIFFERENT names, as in GenomicRanges.
    Every interval must have 0 <= start <= end: a zero-width row (end == start - 1, which IRanges accepts as an empty range and some exon
    designs carry) is refused with the rest -- it can overlap nothing, so the caller leaves such rows out (and keeps its own indices as names)."""

    def __init__(self, chromosome, start, end, names=None, group=None, kind=None, device=0):
        chrom = np.asarray([str(c) for c in chromosome], dtype=object)
        self.start, self.end = _coords(start, end)
        if not (chrom.size == self.start.size == self.end.size):
            raise ValueError("chromosome, start and end must have the same length")
        self.n = int(self.start.size)
        levels, codes = np.unique(chrom.astype(str), return_inverse=True) if self.n else (np.zeros(0, dtype=str), np.zeros(0, np.int64))
        self.levels = [str(x) for x in levels]
        self._code_of = {c: i for i, c in enumerate(self.levels)}
        self.chrom = _i32(codes)
        self.names = None if names is None else np.asarray(names, dtype=object)
        if self.names is not None and self.names.size != self.n:
            raise ValueError("names must have one entry per interval")
        self.group = None if group is None else _i32(group).ravel()
        self.kind = None if kind is None else _i32(kind).ravel()
        for a in (self.group, self.kind):
            if a is not None and a.size != self.n:
                raise ValueError("group / kind must have one entry per interval")
        self.handle = C.c_void_p()
        check(lib().ed_annot_create(C.byref(self.handle), int(device), self.n, len(self.levels), _ptr(self.chrom), _ptr(self.start),
                                    _ptr(self.end), None if self.group is None else _ptr(self.group),
                                    None if self.kind is None else _ptr(self.kind)))

    def close(self):
        if self.handle:
            lib().ed_annot_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def chromosome_ids(self, chromosome):
        """ids of query chromosome names; a name the track does not have is -1 (no hits)"""
        chrom = np.asarray([str(c) for c in chromosome], dtype=str)
        if chrom.size == 0:
            return np.zeros(0, np.int32)
        u, inv = np.unique(chrom, return_inverse=True)
        return _i32(np.asarray([self._code_of.get(str(x), -1) for x in u], dtype=np.int32)[inv])

    def overlaps(self, chromosome, start, end, min_overlap=0.5, group=None, kind=None, want_hits=True):
        """The intervals of the track every query interval hits (include/exomedepth_amd.h, "Annotation overlap": the overlap of
        R/annotate_extra.R:63-65, `ov > min_overlap * (end - start)` with ov = min(ends) - max(starts), no + 1).
        group / kind (int32 per query): drop pairs of equal group / keep only pairs of equal kind; the track must have been given the array.
        Returns (counts int64 [n_q], offsets int64 [n_q + 1], hits int32 [offsets[-1]]): query q hits the track's intervals
        hits[offsets[q]:offsets[q + 1]] (indices into the arrays the track was made from), ascending by (start, index).  want_hits=False:
        hits is None (count only).  A chromosome name the track does not have gives no hits."""
        if not self.handle:
            raise EdError("Annotation is closed")
        qs, qe = _coords(start, end)
        qc = self.chromosome_ids(chromosome)
        n_q = int(qs.size)
        if not (qc.size == n_q == qe.size):
            raise ValueError("chromosome, start and end must have the same length")
        qg = None if group is None else _i32(group).ravel()
        qk = None if kind is None else _i32(kind).ravel()
        for a in (qg, qk):
            if a is not None and a.size != n_q:
                raise ValueError("group / kind must have one entry per query")
        counts = np.zeros(n_q, np.int64)
        offsets = np.zeros(n_q + 1, np.int64)
        total = C.c_int64(0)
        args = (self.handle, n_q, _ptr(qc), _ptr(qs), _ptr(qe), None if qg is None else _ptr(qg), None if qk is None else _ptr(qk),
                float(min_overlap), _ptr(counts), _ptr(offsets))
        if not want_hits:
            check(lib().ed_annot_overlaps(*args, None, 0, C.byref(total)))
            return counts, offsets, None
        # one call when the guess holds the hits; the library reports the total either way and writes nothing when they do not fit
        hits = np.empty(max(1024, 4 * n_q), np.int32)
        rc = lib().ed_annot_overlaps(*args, _ptr(hits), hits.size, C.byref(total))
        if rc != _lib.ED_OK and total.value > hits.size:
            hits = np.empty(total.value, np.int32)
            rc = lib().ed_annot_overlaps(*args, _ptr(hits), hits.size, C.byref(total))
        check(rc)
        return counts, offsets, hits if hits.size == total.value else hits[:total.value].copy()


def _call_intervals(calls, chromosome_names, exon_start, exon_end):
    """a structured ed_call array as genomic intervals, as CallCNVs makes them: start[start_exon], end[end_exon], the plan's chromosome level"""
    calls = np.asarray(calls)
    names = np.asarray([str(c) for c in chromosome_names], dtype=object)
    es, ee = np.asarray(exon_start), np.asarray(exon_end)
    return names[calls["chrom"]], es[calls["start_exon"]], ee[calls["end_exon"]]


def annotate_calls(calls, chromosome_names, exon_start, exon_end, annotation, min_overlap=0.5):
    """AnnotateExtra for a cohort's call table: `calls` is the structured ed_call array of Batch.calls(), Cohort.results(...) or
    MultiDevice.run_host(...), chromosome_names the plan's chromosome levels (calls["chrom"] indexes them), exon_start / exon_end the
    plan's exon coordinates.  Returns (counts, offsets, hits) of Annotation.overlaps for the calls in table order."""
    chrom, start, end = _call_intervals(calls, chromosome_names, exon_start, exon_end)
    return annotation.overlaps(chrom, start, end, min_overlap=min_overlap)


def cohort_call_recurrence(calls, chromosome_names, exon_start, exon_end, min_overlap=0.5, same_type=True, carriers=False, device=0):
    """The call table joined against itself under AnnotateExtra's rule: per call, the number of calls of OTHER samples that overlap it by more
    than min_overlap x its own length (the rule is asymmetric: a short call inside a long one counts the long one, not the reverse, for
    min_overlap near 1) -- of the same type only when same_type is set.  The group is the sample, so a call never counts itself or its
    sample-mates.  carriers=True returns (n_calls, n_carriers) with n_carriers the number of DISTINCT other samples among those calls; the join
    (windows, tests, filters, compaction) runs on the device, the distinct count is made on the host from the CSR result."""
    calls = np.asarray(calls)
    chrom, start, end = _call_intervals(calls, chromosome_names, exon_start, exon_end)
    sample = _i32(calls["sample"])
    kind = _i32(calls["type"]) if same_type else None
    track = Annotation(chrom, start, end, group=sample, kind=kind, device=device)
    try:
        counts, offsets, hits = track.overlaps(chrom, start, end, min_overlap=min_overlap, group=sample, kind=kind, want_hits=bool(carriers))
    finally:
        track.close()
    if not carriers:
        return counts
    n = calls.size
    if n == 0 or hits.size == 0:
        return counts, np.zeros(n, np.int64)
    K = int(sample.max()) + 1
    pairs = np.unique(np.repeat(np.arange(n, dtype=np.int64), counts) * K + sample[hits])     # distinct (call, other sample)
    n_carriers = np.bincount(pairs // K, minlength=n).astype(np.int64)
    return counts, n_carriers


REFSET_DTYPE = np.dtype([("ref_index", "<i4"), ("selected", "<i4"), ("correlation", "<f8"), ("expected_BF", "<f8"),
                         ("phi", "<f8"), ("ratio_sd", "<f8"), ("mean_p", "<f8"), ("median_depth", "<f8")])
assert REFSET_DTYPE.itemsize == C.sizeof(EdRefsetRow)


def select_reference_set(test_counts, reference_counts, bin_length=None, n_bins_reduced=0, names=None, prefix_window=None):
    """reference R/optimize_reference_set.R:53-148 (formula ~ 1, phi.bins = 1).

    test_counts: (E,) ; reference_counts: (E, R) matrix, one column per candidate reference sample (host array,
    or a torch CUDA int32 tensor of shape (E, R)).  Returns {'reference.choice': [...], 'summary.stats':
    structured array (REFSET_DTYPE, sorted by decreasing correlation), 'n.bins': int}.
    prefix_window=(begin, end): raw statistics of those cumulative references only (a rank's share, see
    dist.select_reference_set_sharded); 'reference.choice' is then None until refset_finalize()."""
    keep = []
    if hasattr(reference_counts, "shape") and len(reference_counts.shape) != 2:
        raise ValueError("The reference sequence count data must be provided as a matrix")
    E, R = int(reference_counts.shape[0]), int(reference_counts.shape[1])
    if int(np.prod(np.shape(test_counts))) != E and not hasattr(test_counts, "data_ptr"):
        raise ValueError("The number of rows of the reference matrix must match the length of the test count data\n")
    if not hasattr(test_counts, "data_ptr"):
        test_counts = _as_r_integer(np.asarray(test_counts))
    if not hasattr(reference_counts, "data_ptr"):
        reference_counts = _as_r_integer(np.asarray(reference_counts))
    pt = _device_pointer(test_counts, np.int32, keep)
    pr = _device_pointer(reference_counts, np.int32, keep)
    bl = None
    if bin_length is not None:
        bl = _f64(bin_length)
        if np.any(bl == 0):
            z = int(np.sum(bl == 0))
            raise ValueError("bin.length contains %d zero%s. This causes NAs in correlation computing. All bin lengths "
                             "must be positive" % (z, "s" if z > 1 else ""))
    rows = np.zeros(R, dtype=REFSET_DTYPE)
    n_chosen = C.c_int32(0)
    n_sel = C.c_int64(0)
    if prefix_window is not None:
        check(lib().ed_select_reference_set_part(pt, pr, E, R, _ptr(bl) if bl is not None else None, int(n_bins_reduced),
                                                 int(prefix_window[0]), int(prefix_window[1]), _ptr(rows),
                                                 C.byref(n_chosen), C.byref(n_sel), None))
        return {"reference.choice": None, "summary.stats": rows, "n.bins": int(n_sel.value),
                "low.coverage": n_chosen.value == 1}
    check(lib().ed_select_reference_set(pt, pr, E, R, _ptr(bl) if bl is not None else None, int(n_bins_reduced),
                                        _ptr(rows), C.byref(n_chosen), C.byref(n_sel), None))
    if names is None:
        names = ["X%d" % (i + 1) for i in range(R)]       # R/optimize_reference_set.R:76
    choice = [names[int(i)] for i in rows["ref_index"][: n_chosen.value]]
    return {"reference.choice": choice, "summary.stats": rows, "n.bins": int(n_sel.value)}


def refcohort_last_path():
    """ed_refcohort_last_path: how the last cohort_select_reference_sets call formed the statistics of its cumulative references --
    dict(chunks_by_columns, chunks_row_major, columns_beyond_bins, max_newton_iterations, columns_large_geometry)."""
    out = (C.c_int64 * 5)()
    check(lib().ed_refcohort_last_path(out))
    return dict(zip(("chunks_by_columns", "chunks_row_major", "columns_beyond_bins", "max_newton_iterations", "columns_large_geometry"), (int(v) for v in out)))


def cohort_select_reference_sets(counts, bin_length=None, n_bins_reduced=0, max_refs=32, want_reference=True, want_correlations=False,
                                 reference_out=None, test_range=None, sample_major=False, counts_sm_out=None, stream=None, grow_max_refs=True):
    """select.reference.set for every sample of a cohort against all the others (reference vignette/vignette.Rnw:390-402 loop;
    R/optimize_reference_set.R:53-148 per sample), in one call.

    counts: (E, S) int32 host array or torch CUDA tensor.  Returns dict(n_chosen (S,), choice (S, K) -1 padded,
    summary.stats (S, K) REFSET_DTYPE, n.bins[, reference: DeviceArray (E, S) aggregate reference][, correlations (S, S)]).
    test_range = (t0, t1): only the samples t0 <= t < t1 as tests (all S still candidates) -- one rank's share of a sample-sharded
    cohort; the per-test outputs then have t1 - t0 rows / columns (ed_cohort_select_reference_sets_range).
    sample_major=True: the aggregate references come back sample-major, (n_tests, E) -- R's column-major matrix, what Cohort(emit_mode=2,
    counts_layout=1) takes -- and counts_sm_out (an (S, E) int32 device array), when given, receives the count matrix transposed alongside
    (ed_cohort_select_reference_sets_sm).
    stream: the HIP stream (its handle as an integer, e.g. torch.cuda.Stream().cuda_stream) the entry's kernels and copies are issued on; None =
    the null stream, which is ordered against every blocking stream of the process -- a caller that wants a copy on another stream to run
    beside this call names a stream of its own here.  The entry returns when its work is complete either way.
    grow_max_refs: a test whose choice is LONGER than max_refs is an error of the C entry ("call again with a larger max_refs": its outputs
    have max_refs columns); True = this wrapper does that, doubling max_refs until every choice fits (the result never depends on
    max_refs otherwise).  With thousands of candidates (a rank of a sample-sharded cohort: 8 191 of them) choices of 33 - 35 do occur."""
    if grow_max_refs:
        k = int(max_refs if max_refs > 0 else 32)
        while True:
            try:
                return cohort_select_reference_sets(counts, bin_length, n_bins_reduced, k, want_reference, want_correlations, reference_out, test_range,
                                                    sample_major, counts_sm_out, stream, grow_max_refs=False)
            except EdError as e:
                if "larger max_refs" not in str(e) or k >= int(counts.shape[1]) - 1:
                    raise
                k = min(2 * k, int(counts.shape[1]) - 1)
    keep = []
    E, S = int(counts.shape[0]), int(counts.shape[1])
    t0, t1 = (0, S) if test_range is None else (int(test_range[0]), int(test_range[1]))
    Sr = t1 - t0
    if not _is_device(counts):             # (a DeviceArray -- correct_counts_using_PCA's result, say -- is used in place, like a torch CUDA tensor)
        counts = _as_r_integer(np.asarray(counts))
    pc = _device_pointer(counts, np.int32, keep)
    K = int(min(max_refs if max_refs > 0 else 32, S - 1))
    bl = _f64(bin_length) if bin_length is not None else None
    n_chosen = np.zeros(Sr, dtype=np.int32)
    choice = np.full((Sr, K), -1, dtype=np.int32)
    rows = np.zeros((Sr, K), dtype=REFSET_DTYPE)
    corr = np.zeros((Sr, S)) if want_correlations else None
    ref = DeviceArray(nbytes=E * Sr * 4) if (want_reference and reference_out is None) else None
    if ref is not None:
        ref.host_dtype, ref.shape = np.dtype(np.int32), ((Sr, E) if sample_major else (E, Sr))
    ref_ptr = ref.ptr if ref is not None else None
    if reference_out is not None:          # the caller's own (E, S) int32 device array (a torch CUDA tensor, say) receives the aggregate references
        ref_ptr = _device_pointer(reference_out, np.int32, keep)
    nsel = C.c_int64(0)
    if sample_major:
        if ref_ptr is None:
            raise ValueError("sample_major=True returns the aggregate references: want_reference or reference_out")
        cs_ptr = _device_pointer(counts_sm_out, np.int32, keep) if counts_sm_out is not None else None
        check(lib().ed_cohort_select_reference_sets_sm(pc, E, S, _ptr(bl) if bl is not None else None, int(n_bins_reduced), K, t0, t1,
                                                       _ptr(n_chosen), _ptr(choice), _ptr(rows), _ptr(corr) if corr is not None else None,
                                                       ref_ptr, cs_ptr, C.byref(nsel), C.c_void_p(stream or 0)))
    else:
        check(lib().ed_cohort_select_reference_sets_range(pc, E, S, _ptr(bl) if bl is not None else None, int(n_bins_reduced), K, t0, t1,
                                                          _ptr(n_chosen), _ptr(choice), _ptr(rows), _ptr(corr) if corr is not None else None,
                                                          ref_ptr, C.byref(nsel), C.c_void_p(stream or 0)))
    out = {"n_chosen": n_chosen, "choice": choice, "summary.stats": rows, "n.bins": int(nsel.value)}
    if ref is not None:
        out["reference"] = ref
    elif reference_out is not None:
        out["reference"] = reference_out
    if corr is not None:
        out["correlations"] = corr
    return out


def _pca_inputs(count_data, mask_exons, sample_div):
    """the input checks of R/PCA_for_read_count.R:43, :60-61 (their messages) shared by the two PCA entries; nothing touches the device yet"""
    shape = getattr(count_data, "shape", None)
    if shape is None or len(shape) != 2:
        raise ValueError("The input to the PCA correction must be a matrix")
    E, S = int(shape[0]), int(shape[1])
    if not _is_device(count_data):
        count_data = _as_r_integer(np.asarray(count_data))
    mask = None
    if mask_exons is not None:
        m = np.asarray(mask_exons)
        if m.dtype != np.bool_:
            raise ValueError("The mask exons argument must be a logical vector")
        if m.ndim != 1 or m.size != E:
            raise ValueError("The length of the mask exons argument does not match the number of exons")
        mask = np.ascontiguousarray(m, dtype=np.uint8)
    div = None
    if sample_div is not None:
        div = _f64(sample_div)
        if div.shape != (S,):
            raise ValueError("sample_div must hold one value per sample (%d), got shape %s" % (S, div.shape))
    return E, S, count_data, mask, div


def correct_counts_using_PCA(count_data, nPCs=3, mask_exons=None, *, sample_div=None, exon_mul=None, sample_mul=None, sd_min=2.0,
                             tol=1e-12, max_iter=500, out=None, stream=None):
    """reference R/PCA_for_read_count.R:41-78: the count matrix with its first nPCs principal components removed, for the whole cohort, on the device.

    count_data: (E, S) host array or torch CUDA int32 tensor, exons by samples.  mask_exons: boolean (E,), exons kept out of the PCA (they are
    still corrected).  Returns a DeviceArray (E, S) int32 -- or `out`, the caller's own (E, S) int32 device array -- that
    cohort_select_reference_sets and Cohort.submit take as it is.

    As the reference computes it: the depth normalisation divides sample (column) i by max(1, rowSums(count_data)[i] / 1000) -- the per-EXON
    vector indexed by the SAMPLE number (:50-51), so it needs S <= E -- and the result is scaled back by rowSums[e] / 1000 per exon (:75).
    That is what the reference's users get, and the default here.  sample_div (S,), exon_mul (E,), sample_mul (S,) replace those vectors:
    out = rint(max(0, exon_mul[e] * sample_mul[s] * (residual + centre[e]))); e.g. sample_div = sample_mul = max(1, colSums / 1000),
    exon_mul = 1 is a per-sample depth normalisation.  Saturation: with v the product before rounding, out = rint(min(2147483647, max(0, v))),
    rint half-even; a negative v and a NaN v (an infinite multiplier times a zero one) give 0 -- R's pmax(0, .) keeps the NaN, an int32 cannot --
    and a v above the int32 range, +inf included, gives exactly 2147483647.  The multipliers are not checked: zero, negative and infinite values
    follow this rule.  sd_min: the reference's 2 (:56).
    tol, max_iter: the eigenvectors come from a subspace iteration stopped at |G u - theta u| <= tol * theta_1; a call that does not get
    there raises EdError (never an answer from an unconverged subspace).  pca_last_info() describes the last call.
    stream: as cohort_select_reference_sets."""
    keep = []
    E, S, count_data, mask, div = _pca_inputs(count_data, mask_exons, sample_div)
    nPCs = int(nPCs)
    em = sm = None
    if exon_mul is not None:
        em = _f64(exon_mul)
        if em.shape != (E,):
            raise ValueError("exon_mul must hold one value per exon (%d), got shape %s" % (E, em.shape))
    if sample_mul is not None:
        sm = _f64(sample_mul)
        if sm.shape != (S,):
            raise ValueError("sample_mul must hold one value per sample (%d), got shape %s" % (S, sm.shape))
    if out is not None:
        if tuple(out.shape) != (E, S):
            raise ValueError("out must have the shape of count_data %s, got %s" % ((E, S), tuple(out.shape)))
        if not _is_device(out):
            raise ValueError("out must be a device array (a torch CUDA int32 tensor or a DeviceArray)")
    pc = _device_pointer(count_data, np.int32, keep)
    if out is not None:
        res, po = out, _device_pointer(out, np.int32, keep)
    else:
        res = DeviceArray(nbytes=E * S * 4)
        res.host_dtype, res.shape = np.dtype(np.int32), (E, S)
        po = res.ptr
    check(lib().ed_correct_counts_pca(pc, E, S, nPCs, _ptr(mask) if mask is not None else None, _ptr(div) if div is not None else None,
                                      _ptr(em) if em is not None else None, _ptr(sm) if sm is not None else None, float(sd_min), float(tol),
                                      int(max_iter), po, C.c_void_p(stream or 0)))
    return res


def pca_gram(count_data, mask_exons=None, *, sample_div=None, sd_min=2.0, stream=None):
    """The first two stages of correct_counts_using_PCA alone (ed_pca_gram): dict(G (S, S) -- the Gram matrix of the centred, normalised
    counts over the selected exons, whose eigenvalues are the spectrum to look at before choosing nPCs --, centre (E,), div (S,),
    selected (E,) bool, n_selected)."""
    keep = []
    E, S, count_data, mask, div = _pca_inputs(count_data, mask_exons, sample_div)
    pc = _device_pointer(count_data, np.int32, keep)
    G = np.zeros((S, S))
    centre = np.zeros(E)
    dv = np.zeros(S)
    sel = np.zeros(E, dtype=np.uint8)
    n = C.c_int64(0)
    check(lib().ed_pca_gram(pc, E, S, _ptr(mask) if mask is not None else None, _ptr(div) if div is not None else None, float(sd_min),
                            _ptr(G), _ptr(centre), _ptr(dv), _ptr(sel), C.byref(n), C.c_void_p(stream or 0)))
    return {"G": G, "centre": centre, "div": dv, "selected": sel.astype(bool), "n_selected": int(n.value)}


PCA_INFO_N, PCA_INFO_THETA = 96, 16


def pca_last_info():
    """ed_pca_last_info: the last correct_counts_using_PCA of the process that reached its iteration -- dict(converged, iterations, residual (over theta_1), n_selected,
    block, nPCs, ms (dict: rowstats, gram, eigen, residual, total; device events), gram_slices, rows_per_slice, gap (theta_k / theta_k+1),
    theta (theta_1 .. theta_{k+1}), U (S, nPCs) the eigenvectors)."""
    out = (C.c_double * PCA_INFO_N)()
    check(lib().ed_pca_last_info(out))
    k = int(out[4])
    S, kk = C.c_int64(0), C.c_int32(0)
    check(lib().ed_pca_last_basis(None, 0, C.byref(S), C.byref(kk)))
    U = np.zeros((int(S.value), int(kk.value)))
    if U.size:
        check(lib().ed_pca_last_basis(_ptr(U), U.size, None, None))
    return {"converged": bool(out[13]), "iterations": int(out[0]), "residual": float(out[1]), "n_selected": int(out[2]), "block": int(out[3]), "nPCs": k,
            "ms": {"rowstats": float(out[5]), "gram": float(out[6]), "eigen": float(out[7]), "residual": float(out[8]), "total": float(out[9])},
            "gram_slices": int(out[10]), "rows_per_slice": int(out[11]), "gap": float(out[12]),
            "theta": np.array([out[PCA_INFO_THETA + i] for i in range(k + 1)]), "U": U}


def get_power_betabinom(size, my_phi, my_p, my_alt_p, theory=False, frequentist=False, limit=False):
    """reference R/tools.R:128-166 (vectorised over its arguments): the expected log10 Bayes factor.  theory=True is the
    reference's binomial case (:137-142).  `frequentist` is accepted and ignored, as in the reference (it is never read).
    limit=True (:145-153) is, in the reference, a Monte-Carlo average over 2000 draws of R's generator; here its expectation
    (sum over 0 < x < size of dbetabinom.ab(x; alt) times the log10 ratio of the beta densities at x / size): the same quantity
    without the sampling noise."""
    mode = 1 if theory else (2 if limit else 0)     # (theory wins, as the reference's two `if` blocks have it)
    size, my_phi, my_p, my_alt_p = np.broadcast_arrays(_f64(np.atleast_1d(size)), _f64(np.atleast_1d(my_phi)),
                                                       _f64(np.atleast_1d(my_p)), _f64(np.atleast_1d(my_alt_p)))
    size, my_phi, my_p, my_alt_p = (_f64(a) for a in (size, my_phi, my_p, my_alt_p))
    out = np.empty(size.size, dtype=np.float64)
    check(lib().ed_get_power_betabinom_mode(size.size, _ptr(size), _ptr(my_phi), _ptr(my_p), _ptr(my_alt_p), mode, _ptr(out)))
    return out if out.size > 1 else float(out[0])


def refset_finalize(rows, names=None):
    """Early exit + reference.choice (R/optimize_reference_set.R:130, :143-145) on a complete table of raw rows."""
    rows = np.ascontiguousarray(rows, dtype=REFSET_DTYPE).copy()
    n_chosen = C.c_int32(0)
    check(lib().ed_refset_finalize(_ptr(rows), rows.size, C.byref(n_chosen)))
    if names is None:
        names = ["X%d" % (i + 1) for i in range(rows.size)]
    return {"reference.choice": [names[int(i)] for i in rows["ref_index"][: n_chosen.value]], "summary.stats": rows}


def _signif(x, digits):
    """R's signif() for the call table's BF and reads.ratio (R/class_definition.R:403-404)."""
    if x == 0 or not np.isfinite(x):
        return x
    from math import floor, log10
    e = digits - 1 - int(floor(log10(abs(x))))
    return round(x * 10 ** e) / 10 ** e if e >= 0 else round(x / 10 ** (-e)) * 10 ** (-e)


def fit_betabin_bins(test, reference, phi_bins):
    """phi.bins > 1 for one sample on the GPU: returns (phi.linear per exon, expected)."""
    test = _i32(test)
    reference = _i32(reference)
    n = test.size
    plan = Plan(np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) + 1)
    batch = Batch(plan, 1)
    try:
        phib = DeviceArray(np.zeros(phi_bins))
        edges = DeviceArray(np.zeros(phi_bins + 1))
        exp = DeviceArray(np.zeros(1))
        t = DeviceArray(test.reshape(n, 1))
        r = DeviceArray(reference.reshape(n, 1))
        batch.fit_bins(t, r, phi_bins, phib, edges, exp)
        phi_lin = batch.phi_linear(r, phi_bins, phib, edges)[:, 0]
        return phi_lin, float(exp.to_host()[0])
    finally:
        batch.close()
        plan.close()


def _formula_terms(formula):
    """Right-hand-side terms of 'cbind(test, reference) ~ x1 + x2' ('1' = intercept only -> [])."""
    if "~" not in formula:
        raise ValueError("formula must look like 'cbind(test, reference) ~ ...'")
    rhs = formula.split("~", 1)[1]
    terms = [t.strip() for t in rhs.split("+")]
    terms = [t for t in terms if t not in ("", "1")]
    for t in terms:
        if not t.replace("_", "").replace(".", "").isalnum():
            raise NotImplementedError("only main effects of numeric covariates are implemented (term %r)" % t)
    return terms


def fit_betabin_cov(test, reference, X):
    """Covariate model for one sample on the GPU: returns (phi, expected per exon)."""
    test = _i32(test)
    reference = _i32(reference)
    n = test.size
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(n, -1)
    plan = Plan(np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) + 1)
    batch = Batch(plan, 1)
    try:
        beta = DeviceArray(np.zeros((X.shape[1] + 1, 1)))
        phi = DeviceArray(np.zeros(1))
        t = DeviceArray(test.reshape(n, 1))
        r = DeviceArray(reference.reshape(n, 1))
        batch.fit_cov(t, r, X, beta, phi)
        expected = batch.expected_cov(X, beta)[:, 0]
        return float(phi.to_host()[0]), expected
    finally:
        batch.close()
        plan.close()


def fit_betabin(test, reference):
    """Fit (phi, expected) of  cbind(test, reference) ~ 1  for one sample on the GPU."""
    test = _i32(test)
    reference = _i32(reference)
    n = test.size
    plan = Plan(np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32) + 1)
    batch = Batch(plan, 1)
    try:
        phi = DeviceArray(np.zeros(1))
        exp = DeviceArray(np.zeros(1))
        batch.fit(test.reshape(n, 1), reference.reshape(n, 1), phi, exp)
        check(lib().ed_synchronize(None))
        if batch.fit_unconverged()[0]:
            import warnings
            warnings.warn("beta-binomial fit: the Newton iteration did not converge (phi, expected are its last iterate)")
        return float(phi.to_host()[0]), float(exp.to_host()[0])
    finally:
        batch.close()
        plan.close()


# ---------------------------------------------------------------------------------------------
# reads per exon: getBamCounts and count.everted.reads (reference R/countBamInGranges.R)
# ---------------------------------------------------------------------------------------------
def readcount_geometry():
    """{block, records_per_workgroup, lds_window, finish_block} of the counting kernels (ed_readcount_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_readcount_geometry(out))
    return dict(zip(("block", "records_per_workgroup", "lds_window", "finish_block"), (int(v) for v in out)))


class _ReadCountMatrix(_RawDevice):
    """the device count matrix of a ReadCounter, int32 (n_columns, n_exons): one row a sample -- R's column-major exon x sample matrix as it
    lies in memory, what Cohort(emit_mode=2, counts_layout=1).submit takes as it is.  It lives as long as its counter (kept alive here)."""

    def __init__(self, counter, ptr):
        _RawDevice.__init__(self, ptr)
        self.counter = counter
        self.shape = (counter.n_columns, counter.n)
        self.host_dtype = np.dtype(np.int32)
        self.nbytes = 4 * counter.n_columns * counter.n

    def to_host(self):
        out = np.empty(self.shape, np.int32)
        if out.nbytes:
            check(lib().ed_memcpy_d2h(_ptr(out), self.ptr, out.nbytes))
        return out


class ReadCounter:
    """Exon x sample read counts on the device (ed_readcount): exons `chromosome`, `start`, `end` as closed 1-based ranges (a BED row is
    [start + 1, end]), 1 <= start <= end, `n_columns` samples.  add() takes a chunk of BAM record fields for one column, finish() turns the
    chunks added into that column's counts; a column is added to and finished before the next one is begun."""

    def __init__(self, chromosome, start, end, n_columns, device=0):
        chrom = [str(c) for c in chromosome]
        self.start, self.end = _coords(start, end)
        if not (len(chrom) == self.start.size == self.end.size):
            raise ValueError("chromosome, start and end must have the same length")
        self.n = int(self.start.size)
        self.n_columns = int(n_columns)
        self.levels = list(dict.fromkeys(chrom))                       # first-seen order
        self._code_of = {c: i for i, c in enumerate(self.levels)}
        self.chrom = _i32(np.fromiter((self._code_of[c] for c in chrom), dtype=np.int32, count=self.n))
        self._maps = {}
        self.handle = C.c_void_p()
        check(lib().ed_readcount_create(C.byref(self.handle), int(device), self.n, len(self.levels), _ptr(self.chrom), _ptr(self.start),
                                        _ptr(self.end), self.n_columns))

    def close(self):
        if self.handle:
            lib().ed_readcount_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if not self.handle:
            raise EdError("ReadCounter is closed")

    def ref_to_chrom(self, ref_names):
        """int32 per reference sequence of a BAM header: the id of the target chromosome of that name, -1 where the exons have none"""
        key = tuple(ref_names)
        if key not in self._maps:
            self._maps = {key: _i32(np.asarray([self._code_of.get(str(r), -1) for r in key], dtype=np.int32))}
        return self._maps[key]

    def add(self, column, records, ref_names, mode=0, min_mapq=20, read_width=300):
        """one chunk of records -- (refid, pos, tlen, flag_mapq) arrays as bam.BamFile.chunks() yields them -- into `column`.
        ref_names: the BAM header's sequence names (refid indexes them).  mode 0: getBamCounts' rule, 1: everted reads."""
        self._open()
        refid, pos, tlen = (_i32(records[k]).ravel() for k in range(3))
        fm = np.ascontiguousarray(records[3], dtype=np.uint32).ravel()
        if not (refid.size == pos.size == tlen.size == fm.size):
            raise ValueError("the four record arrays must have the same length")
        r2c = self.ref_to_chrom(ref_names)
        check(lib().ed_readcount_add(self.handle, int(column), int(mode), int(refid.size), _ptr(refid), _ptr(pos), _ptr(tlen), _ptr(fm),
                                     int(r2c.size), _ptr(r2c) if r2c.size else None, int(min_mapq), int(read_width)))

    def add_device(self, column, device_records, ref_names, mode=0, min_mapq=20, read_width=300):
        """add() for records that are on the device already (bam.DeviceRecords, from DeviceBamFile.batches()): ed_readcount_add_device"""
        self._open()
        r2c = self.ref_to_chrom(ref_names)
        p = [C.c_void_p(x) for x in device_records.ptrs]
        check(lib().ed_readcount_add_device(self.handle, int(column), int(mode), int(device_records.n), p[0], p[1], p[2], p[3], int(r2c.size),
                                            _ptr(r2c) if r2c.size else None, int(min_mapq), int(read_width), None))

    def finish(self, column):
        self._open()
        check(lib().ed_readcount_finish(self.handle, int(column)))

    def counts(self, column0=0, n_columns=None):
        """host int32 (n_exons, n_columns): the whole matrix, or the columns column0 .. column0 + n_columns - 1"""
        self._open()
        k = self.n_columns - int(column0) if n_columns is None else int(n_columns)
        out = np.empty((max(k, 0), self.n), np.int32)
        check(lib().ed_readcount_copy(self.handle, int(column0), k, _ptr(out)))
        return out.T

    def device_counts(self, exon_major=False):
        """the matrix on the device, everything added and finished so far in it.  Default: the matrix where it was made, int32
        (n_columns, n_exons), sample-major (see _ReadCountMatrix) -- what Cohort(emit_mode=2, counts_layout=1).submit takes.
        exon_major=True: a DeviceArray int32 (n_exons, n_columns), transposed on the device (ed_readcount_copy_exon_major) -- what
        correct_counts_using_PCA, cohort_select_reference_sets and Cohort.submit in the default layout take.  Neither touches the host."""
        self._open()
        if exon_major:
            out = DeviceArray(nbytes=max(4, 4 * self.n * self.n_columns))
            out.host_dtype, out.shape = np.dtype(np.int32), (self.n, self.n_columns)
            check(lib().ed_readcount_copy_exon_major(self.handle, out.ptr))
            return out
        p = lib().ed_readcount_device_counts(self.handle)
        if not p:
            raise EdError("libedcore: %s" % lib().ed_last_error().decode(errors="replace"))
        return _ReadCountMatrix(self, p)

    def kernel_ms(self):
        """(k_rcnt_bin, k_rcnt_finish) device milliseconds of this counter so far"""
        self._open()
        a, b = C.c_double(0), C.c_double(0)
        check(lib().ed_readcount_kernel_ms(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value


def _bed_columns(bed_frame, bed_file):
    """the columns of a BED frame: a mapping of column name -> values (a dict, a pandas DataFrame), or a sequence of columns; else the
    tab-separated file, no header (read.delim(header = FALSE))"""
    if bed_frame is None:
        if bed_file is None:
            raise ValueError("If no bed data frame is provided there must be a link to a bed file")
        rows = []
        with open(bed_file) as f:
            for line in f:
                line = line.rstrip("\r\n")
                if line:
                    rows.append(line.split("\t"))
        if rows and min(len(r) for r in rows) < 3:
            raise ValueError("bed_file: every line needs chromosome, start and end, tab-separated")
        cols = [[r[k] for r in rows] for k in range(min(len(r) for r in rows))] if rows else [[], [], []]
        cols[1] = np.asarray([int(x) for x in cols[1]], dtype=np.int64)
        cols[2] = np.asarray([int(x) for x in cols[2]], dtype=np.int64)
        return cols
    if hasattr(bed_frame, "keys"):
        return [np.asarray(bed_frame[k]) for k in list(bed_frame.keys())]
    return [np.asarray(c) for c in bed_frame]


def bed_targets(bed_frame=None, bed_file=None, include_chr=False, reorder=True):
    """The target frame of getBamCounts (reorder=True, R/countBamInGranges.R:308-331) or count.everted.reads (reorder=False, :438-450), on the
    host: dict(chromosome, start, end[, exon]).  start is the BED start + 1 (targets are closed 1-based ranges); exon is there when the frame has a
    fourth column of text.  reorder: chromosome levels '1'..'22' first, then the other names in first-seen order, rows by start + end within a
    chromosome, ties in input order (chromosome_order); otherwise the caller's row order stands.  include_chr prefixes 'chr' to the names."""
    cols = _bed_columns(bed_frame, bed_file)
    if len(cols) < 3:
        raise ValueError("the first three columns of the bed frame must be chromosome, start, end")
    chrom = [("chr" + str(c)) if include_chr else str(c) for c in cols[0]]
    bstart, bend = _coords(cols[1], cols[2])
    if not (len(chrom) == bstart.size == bend.size):
        raise ValueError("chromosome, start and end must have the same length")
    names = None
    if len(cols) >= 4:
        c4 = np.asarray(cols[3])
        if c4.dtype.kind in "US" or (c4.dtype.kind == "O" and all(isinstance(x, str) for x in c4)):
            names = np.asarray([str(x) for x in c4], dtype=object)
    order = chromosome_order(chrom, bstart, bend)[0] if (reorder and len(chrom)) else np.arange(len(chrom))
    start = bstart.astype(np.int64)[order] + 1
    if start.size and start.max() > 2**31 - 1:
        raise ValueError("interval coordinates must fit int32")
    out = {"chromosome": np.asarray(chrom, dtype=object)[order], "start": start.astype(np.int32), "end": bend[order]}
    if names is not None:
        out["exon"] = names[order]
    return out


def gc_geometry():
    """{block, segment_bytes, step_bytes, lane_bytes} of the letter counter (ed_gc_geometry): for tests placing shapes on the edges"""
    out = (C.c_int32 * 4)()
    check(lib().ed_gc_geometry(out))
    return dict(zip(("block", "segment_bytes", "step_bytes", "lane_bytes"), (int(v) for v in out)))


class GcCounter:
    """Letters of byte ranges of a file, summed per target on the device (ed_gc): add() takes one piece of the file and the ranges that touch
    it, counts() gives int32 (gc, atgc) per target -- #{C, G} and #{A, C, G, T}, either case; every other byte counts in neither."""

    def __init__(self, n_targets, device=0):
        self.n = int(n_targets)
        self.handle = C.c_void_p()
        check(lib().ed_gc_create(C.byref(self.handle), int(device), self.n))

    def close(self):
        if self.handle:
            lib().ed_gc_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _open(self):
        if not self.handle:
            raise EdError("GcCounter is closed")

    def add(self, data, file_offset, first, last_excl, target):
        """data: the file's bytes [file_offset, file_offset + len(data)) (bytes, or a uint8 array); first, last_excl: file byte addresses of the
        ranges, which may reach beyond the piece on either side (they are clipped to it); target: the index each range adds to"""
        self._open()
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8)
        first, last_excl, target = (np.ascontiguousarray(a, dtype=np.int64).ravel() for a in (first, last_excl, target))
        if not (first.size == last_excl.size == target.size):
            raise ValueError("first, last_excl and target must have the same length")
        check(lib().ed_gc_add(self.handle, _ptr(buf) if buf.size else None, int(buf.size), int(file_offset), int(first.size),
                              _ptr(first) if first.size else None, _ptr(last_excl) if first.size else None, _ptr(target) if first.size else None))

    def counts(self):
        self._open()
        gc, atgc = np.empty(self.n, np.int32), np.empty(self.n, np.int32)
        check(lib().ed_gc_copy(self.handle, _ptr(gc) if self.n else None, _ptr(atgc) if self.n else None))
        return gc, atgc

    def kernel_ms(self):
        """k_gc_count device milliseconds of this counter so far"""
        self._open()
        ms = C.c_double(0)
        check(lib().ed_gc_kernel_ms(self.handle, C.byref(ms)))
        return ms.value


def gc_content(fasta, chromosome, start, end, *, flank=0, counts=False, batch_bytes=64 << 20, device=0, stats=None):
    """GC content of every target [start, end] (1-based, both included: the count frame's own columns) of the uncompressed FASTA file `fasta` (a
    path or a fasta.FastaIndex), counted on the device: float64 gc / atgc, where gc counts the letters G and C and atgc the letters A, T, G and C,
    in either case -- letterFrequency(x, "GC") / letterFrequency(x, "ATGC") of the reference's referenceFasta block (R/countBamInGranges.R:333-344).
    N, the IUPAC codes and everything else count in neither; a target without any of the four letters gives NaN (NA in R), which the caller drops
    or imputes before using the column as a covariate.  counts=True: the int32 arrays (gc, atgc) instead.
    flank widens every target by that many bases on both sides, clipped to its sequence.  The file is read in pieces of batch_bytes, two in flight
    (the next is read while the one before is uploaded and counted); a piece goes to the device with the ranges that touch it, and a target cut by
    a piece's border is the sum of its parts, so no result depends on batch_bytes.  Sequences without a target are not read.
    stats: a dict that receives pieces, bytes_read and kernel_ms (k_gc_count's device time), for tools/bench_gc.py.
    ValueError: a sequence the file does not have, a target beyond its sequence's end, start < 1, end < start."""
    from . import fasta as _fasta
    idx = fasta if isinstance(fasta, _fasta.FastaIndex) else _fasta.FastaIndex(fasta)
    flank, batch_bytes = int(flank), int(batch_bytes)
    if flank < 0 or batch_bytes < 1:
        raise ValueError("flank >= 0 and batch_bytes >= 1 wanted")
    chrom = [str(c) for c in chromosome]
    start = np.asarray(start).astype(np.int64).ravel()
    end = np.asarray(end).astype(np.int64).ravel()
    if not (len(chrom) == start.size == end.size):
        raise ValueError("chromosome, start and end must have the same length")
    n = start.size
    if n:
        first, last = idx.byte_range(chrom, start, end)                # the targets as given: refusals name the caller's rows
        if flank:
            length = idx.length[idx.rows(chrom)]
            first, last = idx.byte_range(chrom, np.maximum(start - flank, 1), np.minimum(end + flank, length))
    else:
        first = last = np.zeros(0, np.int64)
    counter = GcCounter(n, device=device)
    pieces = bytes_read = 0
    try:
        if n:
            order = np.argsort(first, kind="stable")
            sf, sl = first[order], last[order]
            reach = np.maximum.accumulate(sl)                          # ascending, like sf: what searchsorted needs
            # a sequence's bytes lie together in the file, so the sorted ranges are grouped by sequence: one stretch of the file -- from its
            # first target's first byte to its targets' last -- per sequence that holds a target
            seq = idx.rows(chrom)[order]
            cut = np.flatnonzero(seq[1:] != seq[:-1]) + 1
            lo_of, hi_of = sf[np.r_[0, cut]], reach[np.r_[cut - 1, n - 1]]
            with open(idx.path, "rb") as f:
                for a, b in zip(lo_of.tolist(), hi_of.tolist()):
                    for p in range(a, b, batch_bytes):
                        q = min(p + batch_bytes, b)
                        i0 = int(np.searchsorted(reach, p, side="right"))      # the ranges before end at or before p
                        i1 = int(np.searchsorted(sf, q, side="left"))          # the ranges from here on begin at or after q
                        if i0 >= i1:
                            continue                                           # a piece between targets
                        f.seek(p)
                        data = f.read(q - p)
                        if len(data) != q - p:
                            raise ValueError("%s ends before byte %d: the file does not fit its index" % (idx.path, q))
                        counter.add(data, p, sf[i0:i1], sl[i0:i1], order[i0:i1])
                        pieces, bytes_read = pieces + 1, bytes_read + len(data)
        gc, atgc = counter.counts()
        if stats is not None:
            stats.update(pieces=pieces, bytes_read=bytes_read, kernel_ms=counter.kernel_ms())
    finally:
        counter.close()
    if counts:
        return gc, atgc
    out = np.full(n, np.nan)
    np.divide(gc, atgc, out=out, where=atgc > 0)
    return out


def _count_bams(frame, bam_files, mode, min_mapq, read_width, device, inflate="host"):
    from . import bam as _bam
    if inflate not in ("host", "device"):
        raise ValueError("inflate must be 'host' or 'device', not %r" % (inflate,))
    bam_files = [bam_files] if isinstance(bam_files, (str, bytes)) or hasattr(bam_files, "__fspath__") else list(bam_files)
    if not bam_files:
        raise ValueError("bam_files is empty")
    bad = np.flatnonzero((frame["start"] < 1) | (frame["end"] < frame["start"]))
    if bad.size:
        raise ValueError("target %d is [%d, %d] after the BED start's + 1: 1 <= start <= end wanted (a BED row needs 0 <= start < end)"
                         % (bad[0], frame["start"][bad[0]], frame["end"][bad[0]]))
    targets = list(dict.fromkeys(frame["chromosome"]))
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(_bam.n_threads()) as pool:
        headers = []
        for path in bam_files:                       # every header is checked before any device work
            with _bam.BamFile(path, pool, batch_bytes=1 << 20) as b:
                headers.append(b.ref_names)
            missing = [c for c in targets if c not in set(headers[-1])]
            if missing:
                raise ValueError("Some sequences in the target data frame cannot be found in the header of the BAM file %s: %s"
                                 % (path, ", ".join(missing)))
        rc = ReadCounter(frame["chromosome"], frame["start"], frame["end"], len(bam_files), device=device)
        try:
            for col, path in enumerate(bam_files):
                if inflate == "device":              # the file crosses the link compressed; its record fields never visit the host
                    b = _bam.DeviceBamFile(path, device=device)
                    for rec in b.batches():
                        rc.add_device(col, rec, b.ref_names, mode=mode, min_mapq=min_mapq, read_width=read_width)
                    rc.finish(col)
                    continue
                with _bam.BamFile(path, pool) as b:
                    for rec in b.chunks():           # the kernels of one chunk run while the next is inflated and scanned
                        rc.add(col, rec, b.ref_names, mode=mode, min_mapq=min_mapq, read_width=read_width)
                rc.finish(col)
            counts = rc.counts()
        finally:
            rc.close()
    out = dict(frame)
    for col, path in enumerate(bam_files):
        out[os.path.basename(os.fspath(path))] = np.ascontiguousarray(counts[:, col])
    return out


def getBamCounts(bed_frame=None, bed_file=None, bam_files=(), index_files=None, min_mapq=20, read_width=300, include_chr=False, device=0,
                 inflate="host", reference_fasta=None):
    """reference R/countBamInGranges.R:298-370: the exon x sample count frame from BAM files and a BED frame, counted on the device.
    Returns a dict of columns in the reference's order -- chromosome, start (BED start + 1), end, exon when the frame has a fourth text column,
    GC when reference_fasta is given, then one int32 array per basename(bam) -- with rows in the reference's order (bed_targets).  A fragment per
    record as include/exomedepth_amd.h states it ("Reads per exon", mode 0); every target chromosome must be named in each BAM header
    (ValueError).  index_files is accepted and ignored: the whole file is scanned, which gives the same counts.
    reference_fasta (the reference's referenceFasta): an uncompressed FASTA file, or a fasta.FastaIndex; the frame gains the float64 column GC,
    the fraction of G and C among the A, T, G and C of every re-ordered target, counted on the device (gc_content) before any BAM file is opened.
    A target without any of the four letters has NaN (NA in R): drop or impute it before the column serves as a covariate
    (ExomeDepth(..., data={"GC": ...}, formula="cbind(test, reference) ~ GC")).  Without the argument the frame has no such column.
    inflate: "host" (the default) inflates the files' BGZF blocks on the host's thread pool; "device" sends them to the device compressed and
    inflates, scans and gathers them there (bam.DeviceBamFile, ReadCounter.add_device) -- the same frame and the same errors for the same files; the headers are checked on the host first."""
    frame = bed_targets(bed_frame, bed_file, include_chr=include_chr, reorder=True)
    if reference_fasta is not None:
        frame["GC"] = gc_content(reference_fasta, frame["chromosome"], frame["start"], frame["end"], device=device)
    return _count_bams(frame, bam_files, 0, min_mapq, read_width, device, inflate)


def count_everted_reads(bed_frame=None, bed_file=None, bam_files=(), index_files=None, min_mapq=20, include_chr=False, device=0, inflate="host"):
    """reference R/countBamInGranges.R:424-468: everted read pairs (duplication evidence) per region; as getBamCounts, but the rows keep
    the caller's order and the rule is the everted one (mode 1: mapq >= min_mapq); inflate as there."""
    frame = bed_targets(bed_frame, bed_file, include_chr=include_chr, reorder=False)
    return _count_bams(frame, bam_files, 1, min_mapq, 0, device, inflate)
