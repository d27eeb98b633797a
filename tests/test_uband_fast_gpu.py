"""The upper-band sweep's fast walk (hh_tune "ub_fast"): counts
enter the FMAs as exponent-zero doubles, the biases staged times 2^512.  The
conversion walk (ub_fast 0) is the reference: every partial, marginal and
weight is the same bit for bit, for ordinary biases and, through the range
guard (a workgroup whose staged biases are not all 0 or of magnitude in
[2^-400, 2^400] takes the conversion walk), for every other input."""
import contextlib

import numpy as np
import pytest

from hichap_master_amd import synth
from tests.knobs import tuned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ice():
    from hichap_master_amd import _lib, ice as ice_mod
    _lib.require_gpu()
    return ice_mod


_knobs = None  # the running test's knob settings, undone in reverse order when it ends


def _fast(on):
    _knobs.enter_context(tuned(ub_fast=1 if on else 0))


@pytest.fixture(autouse=True)
def _force_uband(ice):
    """the upper-band sweep whatever the size (these matrices are below the
    automatic threshold)"""
    global _knobs
    with contextlib.ExitStack() as _knobs, tuned(uband=2):
        yield


_CHROM = [14637]  # the C4 model on a chr8-size chromosome (tests/test_uband_gpu.py): several chunks per segment


def _chrom(ice):
    A, td = synth.calibrate(synth.genome_bins(10000, diploid=True), 5e9, 0.2)
    return ice.ContactMatrix.synthetic(list(_CHROM), A=A, trans_density=td, comp_block=200, seed=20201015)


def _pixels(ice):
    """the pixel genome of test_uband_matches_oracle: both bands hold counts
    at and beyond their ranges (300 > 255, 16 > 15)"""
    rng = np.random.default_rng(31)
    b1, b2, c, off = synth.coo_genome([1400, 900], rng, A=60.0, trans_density=0.02)
    c = c.copy()
    c[::97] = 300
    c[5::89] = 16
    return ice.ContactMatrix.from_pixels(b1, b2, c, int(off[-1]), off)


@pytest.fixture(scope="module", params=["chrom", "pixels"])
def matrix(request, ice):
    with tuned(uband=2):
        m = (_chrom if request.param == "chrom" else _pixels)(ice)
    inf = m.info()
    if request.param == "chrom":
        assert inf["band_w"] > 2 * 1008 and inf["band_w4"] - inf["band_w"] > 2 * 1008, inf
    else:
        assert inf["band_w4"] > inf["band_w"] > 0, inf
    assert not inf["upper"]
    yield m
    m.close()


def _sweep(ice, st, n, fast):
    """one sweep's marginals (count * b_i * b_j) of the state's biases"""
    import torch
    _fast(fast)
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    st.marg_local(2, out, None)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _one_sweep_opts(ice):
    return ice.IceOptions(tol=0.0, max_iters=10, mad_max=0, min_nnz=0)


def test_balance_bitwise(ice, matrix):
    opts = ice.IceOptions(max_iters=500)
    _fast(False)
    w0, s0 = ice.balance_matrix(matrix, opts)
    _fast(True)
    w1, s1 = ice.balance_matrix(matrix, opts)
    assert s1["iters"] == s0["iters"]
    np.testing.assert_array_equal(w1, w0)


def test_one_sweep_bitwise_and_no_fallback(ice, matrix):
    n = int(matrix.info()["n_bins"])
    b = np.random.default_rng(5).lognormal(0.0, 1.0, n)
    st = ice.IceState(matrix, _one_sweep_opts(ice))
    try:
        st.set_bias(b)
        np.testing.assert_array_equal(st.bias(), b)
        want = _sweep(ice, st, n, False)
        assert st.uband_fallbacks() == 0  # the forced conversion walk is no fallback
        got = _sweep(ice, st, n, True)
        assert st.uband_fallbacks() == 0
    finally:
        st.close()
    assert np.isfinite(want).all() and want.max() > 0
    np.testing.assert_array_equal(got, want)


def _guard_biases(case, n):
    b = np.random.default_rng(11).lognormal(0.0, 1.0, n)
    if case == "up":
        return b * np.ldexp(1.0, 450)
    if case == "down":
        return b * np.ldexp(1.0, -450)
    if case == "single":
        b[n // 3] = np.ldexp(1.0, 450)
    b[[5, n // 2, n - 7]] = 0.0  # "single" and "masked": bins without a bias
    b[[17, n // 2 + 1]] = np.nan
    return b


@pytest.mark.parametrize("case", ["up", "down", "single", "masked"])
def test_guard_bitwise(ice, matrix, case):
    """biases outside the range (all of them, or a single bin among zeros and
    NaNs) send their workgroups to the conversion walk: the same bits, and the
    counter shows it; zeros and NaNs alone are in range"""
    n = int(matrix.info()["n_bins"])
    b = _guard_biases(case, n)
    st = ice.IceState(matrix, _one_sweep_opts(ice))
    try:
        st.set_bias(b)
        want = _sweep(ice, st, n, False)
        assert st.uband_fallbacks() == 0
        got = _sweep(ice, st, n, True)
        fell = st.uband_fallbacks()
    finally:
        st.close()
    np.testing.assert_array_equal(got, want)
    if case == "masked":
        assert fell == 0
    else:
        assert fell > 0


def test_one_sweep_row_sums_equal_export(ice, matrix):
    """b = 1: the fast walk's marginals are the row sums of the exported
    table, exactly (integer counts).  The table is exported from the pixel
    genome (both bands, counts beyond their ranges; milliseconds); exporting
    the C4-model chromosome takes ~10 s, and the conversion walk's row sums on
    it are pinned to its export by tests/test_uband_gpu.py, so there the fast
    walk's b = 1 sweep is compared bit for bit with the conversion walk's."""
    n = int(matrix.info()["n_bins"])
    st = ice.IceState(matrix, _one_sweep_opts(ice))
    try:
        if n == sum(_CHROM):
            want = _sweep(ice, st, n, False)
        else:
            b1, b2, c = matrix.export_upper()
            want = np.bincount(b1, weights=c, minlength=n) + np.bincount(b2, weights=c, minlength=n)
        got = _sweep(ice, st, n, True)
        assert st.uband_fallbacks() == 0
    finally:
        st.close()
    assert want.max() > 0 and np.array_equal(want, np.round(want))
    np.testing.assert_array_equal(got, want)
