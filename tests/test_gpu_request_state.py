"""What a batch makes from a finished run on request -- the posterior, the per-call posterior, the breakpoint intervals, the transition
score and the copy-ratio profile of the calls -- and the timers of those requests, across several runs of ONE batch (a
run invalidates; the first request makes; a second launches nothing).

tests/test_gpu_bounds.py covers the staleness of the bounds timer after a second run; this file pins all four timers and both pass
counters through the same sequence, and that timing changes no result.

The shape is the smallest that exercises everything: chromosomes of 70, 1 and 130 exons (one chain longer than a 64-exon tile, one of a
single exon) and 5 samples (no multiple of 4); the generator's counts without random segments, with one deletion and one duplication
planted, so that the call kernels have rows to work on.
"""
import numpy as np
import pytest

from exomedepth_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (70, 1, 130)
S = 5
GRID = (0.5, 0.75, 1.0, 1.25, 1.5)


def case():
    """(chrom_off, start, end, (test, ref, phi, expected)): sample 1 carries a deletion of exons 20 .. 31 (the 70-exon chain), sample 3
    a duplication of exons 120 .. 135 (the 130-exon chain, across its first tile edge)"""
    chrom_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    E = int(chrom_off[-1])
    start = np.concatenate([10000 + 3000 * np.arange(m) for m in SIZES]).astype(np.int32)
    end = (start + 150).astype(np.int32)
    test, ref, p, phi, _ = synth.counts_numpy(chrom_off, S, seed=41, n_segments=0, mean_depth=100.0)
    assert test.shape == (E, S)
    test[20:32, 1] = np.rint(0.5 * test[20:32, 1]).astype(np.int32)
    test[120:136, 3] = np.rint(1.5 * test[120:136, 3]).astype(np.int32)
    return chrom_off, start, end, (test, ref, phi, p)


def requests(b):
    """every on-request result of the batch's last run, by name"""
    out = {"log_posterior": b.posterior(log=True), "call_posterior": b.call_posterior(), "call_bounds": b.call_bounds()}
    out["log_evidence"], out["score"] = b.transition_score()
    out["ratio_L"], out["ratio_used"] = b.call_ratio_profile(GRID)
    return out


def _timers(b):
    return tuple(b.posterior_ms().values()) + (b.transition_score_ms(), b.call_bounds_ms(), b.call_ratio_ms())


def test_timers_and_pass_counters_across_runs(edlib):
    chrom_off, start, end, data = case()
    plan = edlib.Plan(chrom_off, start, end)
    b = edlib.Batch(plan, S)
    b.enable_timing()
    b.run(*data)
    n = b.n_calls()
    assert n >= 1
    # 1. after a run, before any request
    assert tuple(b.posterior_ms().values()) == (0.0, 0.0, 0.0)
    assert b.transition_score_ms() == 0.0 and b.call_bounds_ms() == 0.0 and b.call_ratio_ms() == 0.0
    assert b.n_posterior_passes() == 0 and b.n_score_passes() == 0
    # 2. the passes
    got = {"log_posterior": b.posterior(log=True)}
    ms = tuple(b.posterior_ms().values())
    assert ms[0] > 0.0 and ms[1] > 0.0 and ms[2] == 0.0
    # 3. the per-call summary
    got["call_posterior"] = b.call_posterior()
    assert tuple(b.posterior_ms().values())[2] > 0.0
    # 4. a second request launches nothing
    assert b.posterior(log=True).tobytes() == got["log_posterior"].tobytes()
    assert b.n_posterior_passes() == 1
    # 5. the other three requests
    got["call_bounds"] = b.call_bounds()
    assert b.call_bounds_ms() > 0.0
    got["log_evidence"], got["score"] = b.transition_score()
    assert b.transition_score_ms() > 0.0 and b.n_score_passes() == 1 and b.n_posterior_passes() == 1
    got["ratio_L"], got["ratio_used"] = b.call_ratio_profile(GRID)
    assert b.call_ratio_ms() > 0.0
    assert len(got["call_posterior"]) == len(got["call_bounds"]) == len(got["ratio_L"]) == n
    # 6. a second run with the same inputs, no request
    b.run(*data)
    assert b.n_calls() == n
    assert _timers(b) == (0.0,) * 6
    assert b.n_posterior_passes() == 1 and b.n_score_passes() == 1
    # 7. the bounds bring the passes with them; nothing else has been timed in this run
    assert b.call_bounds().tobytes() == got["call_bounds"].tobytes()
    assert b.n_posterior_passes() == 2 and b.call_bounds_ms() > 0.0
    assert tuple(b.posterior_ms().values())[2] == 0.0 and b.transition_score_ms() == 0.0
    # 8. the score
    assert b.transition_score()[1].tobytes() == got["score"].tobytes()
    assert b.n_score_passes() == 2 and b.n_posterior_passes() == 2 and b.transition_score_ms() > 0.0
    # without timing: every timer reads 0 and every array is bit for bit what the timed pass returned
    b.enable_timing(False)
    b.run(*data)
    quiet = requests(b)
    assert _timers(b) == (0.0,) * 6
    assert b.n_posterior_passes() == 3 and b.n_score_passes() == 3
    assert sorted(quiet) == sorted(got)
    for name, a in got.items():
        assert quiet[name].dtype == a.dtype and quiet[name].tobytes() == a.tobytes(), name
    b.close()
    plan.close()
