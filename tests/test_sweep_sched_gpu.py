"""The sweep's schedules (hh_tune "sweep_sched": 0 one stream, 1 all concurrent,
2 phased -- the flat kernel alone, then the tiled kernel beside the band
sweep).  Each sweep kernel writes its own partials, so the schedule cannot
change a bit: every test balances one matrix under the three schedules and
asks for equal weights and iteration counts, and reads the schedule that ran
from hh_ice_sweep_sched instead of assuming it.  A missing dependency between
the streams is a race; some hundred iterations of fork and join give it as
many chances on matrices that balance in well under a second."""
import numpy as np
import pytest

from hichap_master_amd import synth
from oracle import ice_ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

SCHEDS = (0, 1, 2)


@pytest.fixture(scope="module")
def ice():
    from hichap_master_amd import _lib, ice as ice_mod
    _lib.require_gpu()
    return ice_mod


def _case(seed, sizes, A):
    rng = np.random.default_rng(seed)
    return synth.coo_genome(list(sizes), rng, A=A, trans_density=0.01)


@pytest.fixture(scope="module")
def small():
    """The two-chromosome matrix of test_ice_gpu.py::test_band_concurrent_bitwise."""
    return _case(17, (1500, 900), 60.0)


def _sched(ice, m, opts):
    """The schedule a sweep of m takes under the knobs set now."""
    st = ice.IceState(m, opts)
    try:
        return st.sweep_sched()
    finally:
        st.close()


def _balance(ice, m, opts, sched, want=None):
    """Balance m under sweep_sched = sched; the getter must name `want`
    (default: the schedule asked for)."""
    with tuned(sweep_sched=sched):
        assert _sched(ice, m, opts) == (sched if want is None else want)
        return ice.balance_matrix(m, opts)


@pytest.mark.parametrize("fcols", [-1, 1])
@pytest.mark.parametrize("uband", [0, 2])
def test_bitwise_across_schedules(ice, small, fcols, uband):
    """Plain and column-grouped flat tiles (flat_cols), the symmetric band
    kernels and k_sweep_ubands (uband): one stream, all concurrent and phased
    give the same bits and the same iteration count."""
    b1, b2, c, off = small
    n = int(off[-1])
    opts = ice.IceOptions(max_iters=300)
    with tuned(sweep_single=0, conc_min_bytes=0, flat_cols=fcols, uband=uband):
        m = ice.ContactMatrix.from_pixels(b1, b2, c, n, off)
        inf = m.info()
        assert inf["n_units_flat"] > 0 and inf["n_units"] > inf["n_units_flat"] and inf["band_w"] > 0
        res = [_balance(ice, m, opts, k) for k in SCHEDS]
        m.close()
    for w, s in res[1:]:
        np.testing.assert_array_equal(w, res[0][0])
        assert s["iters"] == res[0][1]["iters"]


def test_converged_groups(ice):
    """--cis-only with three chromosomes of unequal size: the groups converge
    at different iterations, so the active flags change under the schedule
    and a kernel's whole launch can become a no-op.  Bitwise across the
    schedules, and the oracle's weights and iteration counts."""
    b1, b2, c, off = _case(19, (1500, 900, 300), 60.0)
    n = int(off[-1])
    opts = ice.IceOptions(max_iters=400, cis_only=True)
    with tuned(sweep_single=0, conc_min_bytes=0):
        m = ice.ContactMatrix.from_pixels(b1, b2, c, n, off, cis_only=True)
        res = [_balance(ice, m, opts, k) for k in SCHEDS]
        m.close()
    wr, sr = ice_ref.balance(b1, b2, c, n, off, cis_only=True, max_iters=400)
    assert len(set(np.atleast_1d(sr["iters"]).tolist())) > 1  # the case is what it claims
    for w, s in res:
        np.testing.assert_array_equal(w, res[0][0])
        np.testing.assert_array_equal(s["iters"], sr["iters"])
        np.testing.assert_allclose(w, wr, rtol=1e-9, equal_nan=True)


@pytest.mark.parametrize("empty", ["flat", "band"])
def test_empty_phases(ice, small, empty):
    """A plan without flat units (flat_max 0: the phased sweep's first phase
    is empty and its event is the fork itself) and a matrix without bands
    (band_w 0, band4 0: nothing for the side stream, which is then not used):
    the phased schedule equals one stream bitwise."""
    b1, b2, c, off = small
    n = int(off[-1])
    opts = ice.IceOptions(max_iters=300)
    layout = dict(flat_max=0) if empty == "flat" else dict(band_w=0, band4=0)
    with tuned(sweep_single=0, conc_min_bytes=0, **layout):
        m = ice.ContactMatrix.from_pixels(b1, b2, c, n, off)
        inf = m.info()
        assert inf["n_units"] > 0
        if empty == "flat":
            assert inf["n_units_flat"] == 0 and inf["band_w"] > 0
        else:
            assert inf["band_w"] == 0 and inf["band_w4"] <= 0 and inf["n_band"] == 0
        w0, s0 = _balance(ice, m, opts, 0)
        w2, s2 = _balance(ice, m, opts, 2)
        m.close()
    np.testing.assert_array_equal(w2, w0)
    assert s2["iters"] == s0["iters"]


def test_auto_rule(ice, small):
    """Auto takes the phased schedule only where the flat launch has a block
    for every CU: this matrix of 2 400 bins, with at most a handful of column
    groups, stays all concurrent once it forks (conc_min_bytes 0); with
    nothing forced its whole sweep is one launch, and without that one
    stream."""
    b1, b2, c, off = small
    n = int(off[-1])
    opts = ice.IceOptions(max_iters=300)
    m = ice.ContactMatrix.from_pixels(b1, b2, c, n, off)
    with tuned(sweep_sched=-1):
        assert _sched(ice, m, opts) == 3
        with tuned(sweep_single=0):
            assert _sched(ice, m, opts) == 0
            with tuned(conc_min_bytes=0):
                assert _sched(ice, m, opts) == 1
                with tuned(band_concurrent=0):
                    assert _sched(ice, m, opts) == 0
        with tuned(sweep_sched=2, conc_min_bytes=0):  # the single launch comes first
            assert _sched(ice, m, opts) == 3
    with tuned(sweep_sched=2, sweep_single=0, conc_min_bytes=0, band_concurrent=0):
        assert _sched(ice, m, opts) == 0  # band_concurrent 0 still forces one stream
    m.close()
