"""Per-pair tumour fractions (somatic.CNV.call for cohorts), the parts that need no GPU: argument checks that fail before any device
work -- in the Python wrappers and in the R entry ed_call_cnvs_batch -- the notice lines the R entry prints, and the new C entries
being declared, bound and exported (tests/test_abi.py checks every declared entry is a function-try-block)."""
import inspect
import os
import re

import numpy as np
import pytest

from test_shim import MIXTURE_FMT, shim  # noqa: F401  (the module's fixture: shim/edcore_shim.c driven through SEXPs)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ed_batch_set_mixture", "ed_cohort_submit_mix", "ed_cohort_run_host_mix", "ed_multi_run_host_mix")
LEN_MSG = "prop.tumor must have length 1 or one value per sample"


def test_new_entries_are_declared_bound_and_exported():
    from exomedepth_amd import _lib
    header = open(os.path.join(ROOT, "include", "exomedepth_amd.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in bound, name
    src = "".join(open(os.path.join(ROOT, "exomedepth_amd", "csrc", f)).read() for f in ("edcore.hip", "edcohort.inc", "edmulti.inc"))
    for name in NEW:
        assert re.search(r"ED_EXPORT int %s\(" % name, src) and 'ED_CATCH("%s")' % name in src, name


def _fake(cls, **fields):
    """an API object that never reached the library: any call into it would fail on its NULL handle"""
    import ctypes as C
    o = cls.__new__(cls)
    o.handle = C.c_void_p()
    for k, v in fields.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("bad", [np.ones(5), np.ones((2, 6)), np.array([0.5, np.nan, 1, 1, 1, 1]), np.array([np.inf] * 6)])
def test_python_wrappers_check_the_mixture_before_any_device_work(bad):
    import exomedepth_amd as ed
    from exomedepth_amd import api

    class P:
        n_exons = 4
    E, S = 4, 6
    test = np.ones((E, S), np.int32)
    co = _fake(ed.Cohort, plan=P(), slabs_in_flight=2, _keep={}, phi_bins=1)
    with pytest.raises(ValueError, match="mixture"):
        co.run_host(test, test, 0, mixture=bad)
    with pytest.raises(ValueError, match="mixture"):
        co.submit(test, test, mixture=bad)
    md = _fake(ed.MultiDevice, n_exons=E, phi_bins=1)
    with pytest.raises(ValueError, match="mixture"):
        md.run_host(test, test, 0, mixture=bad)
    b = _fake(ed.Batch, plan=P(), n_samples=S, _keep_run=[], _keep_fit=[], _owned=False)
    with pytest.raises(ValueError, match="mixture"):
        b.set_mixture(bad)
    assert api._per_sample_mixture(0.3, S) is None and api._per_sample_mixture(np.float64(1.0), S) is None
    assert api._per_sample_mixture([0.5] * S, S).tobytes() == np.full(S, 0.5).tobytes()


def test_somatic_cnv_call_follows_the_reference_signature():
    import exomedepth_amd as ed
    params = list(inspect.signature(ed.somatic_CNV_call).parameters.items())
    assert [k for k, _ in params] == ["normal", "tumor", "prop_tumor", "chromosome", "start", "end", "names"]   # R/class_definition.R:442
    assert params[2][1].default == 1.0
    with pytest.raises(ValueError):
        ed.somatic_CNV_call(np.ones(10), np.ones(10), [0.5, 0.5], ["1"] * 10, np.arange(10), np.arange(10) + 1, ["e"] * 10)


def test_r_wrapper_somatic_cnv_call_cohort():
    text = open(os.path.join(ROOT, "shim", "R", "exomedepth_amd.R")).read()
    m = re.search(r"somatic\.CNV\.call\.cohort <- function\(([^{]*)\) \{", text, re.S)
    assert m, "somatic.CNV.call.cohort is not defined"
    formals = [a.strip() for a in " ".join(m.group(1).split()).split(",")]
    assert formals == ["normal", "tumor", "prop.tumor = 1", "chromosome", "start", "end", "names", "emit.mode = 2L", "devices = NULL",
                       "slab = 256L"]
    body = text[m.end():]
    body = body[:body.index("\n}\n")]
    assert '.Call("ed_call_cnvs_batch", tumor, normal,' in body and "as.double(1e-4)" in body and "as.double(50000)" in body
    assert [ln for ln in re.findall(r"message\('([^']*)'\)", body)] == ["Warning: this function is largely untested and experimental",
                                                                       "Initializing the exomeDepth object", "Now calling the CNVs"]


def _args(sh, E, S, prop):
    t = sh.int_matrix(np.full((E, S), 30)); r = sh.int_matrix(np.full((E, S), 90))
    return (t, r, sh.integer([0, E]), sh.integer(np.arange(E) * 100), sh.integer(np.arange(E) * 100 + 50), sh.real([1e-4]), sh.real([50000.0]),
            sh.nil, sh.nil, sh.real(prop), sh.integer([64]), sh.integer([0]), sh.integer([0]), sh.integer([1]), sh.integer([2]), sh.nil)


@pytest.mark.parametrize("prop", [[0.5, 0.5], [0.5] * 4, [0.5, np.nan, 1.0], [1.0, 1.0, np.inf]])
def test_shim_rejects_a_wrong_prop_tumor_before_any_device_work(shim, prop):  # noqa: F811
    res, out, err = shim.dot_call("ed_call_cnvs_batch", *_args(shim, 20, 3, prop))
    assert res is None and err == LEN_MSG and out == ""               # (no notice either: nothing was done)
    assert shim.R.minir_protect_balance() == 0


def test_shim_prints_the_mixture_notice_once_per_pair_not_at_one(shim):  # noqa: F811
    """the reference's loop of somatic.CNV.call prints src/CNV_estimate.cpp:61 once per pair whose value is not 1, in column order"""
    m = [0.5, 1.0, 0.25, 0.8]
    res, out, err = shim.dot_call("ed_call_cnvs_batch", *_args(shim, 20, 4, m))
    assert out == MIXTURE_FMT % 0.5 + MIXTURE_FMT % 0.25 + MIXTURE_FMT % 0.8
    from exomedepth_amd import _lib
    if _lib.lib().ed_device_count() == 0:
        assert res is None and "HIP device" in err          # then the device work fails loudly: no CPU fallback
    assert res is None or shim.R.minir_protect_balance() == 0
    res, out, err = shim.dot_call("ed_call_cnvs_batch", *_args(shim, 20, 4, [0.5]))   # length 1: one notice, as today
    assert out == MIXTURE_FMT % 0.5
