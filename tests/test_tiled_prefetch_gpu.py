"""The tiled sweep's pipelined loop (hh_tune "tiled_pf", ice.hip RowsPf): the
payload loads of a wave's next step are issued before the current step's data
are used.  Today's loop (tiled_pf 0: tile_rows / band_rows) is the reference:
every partial, marginal and weight is the same bit for bit, and with b = 1 a
sweep gives the exported table's row sums exactly.

Two matrices, both swept by k_sweep_tiled alone (no flat tiles, no
single-launch sweep):
  "lengths"     whole row-block units (band_rows' path): row lengths around
                every lane-group width, in both the narrow and the wide segment
  "row ranges"  one large tile cut into row-range units (tile_rows' path)"""
import numpy as np
import pytest

from tests.knobs import tuned

pytestmark = pytest.mark.gpu

KW = 8192  # tile width (columns), kR = 512 rows per row-block
# uint4 per row segment: every lane-group width G = 4..64, q + G == qe and one off
LENS = [0, 1, 5, 6, 7, 11, 12, 13, 23, 24, 25, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193]


@pytest.fixture(scope="module")
def ice():
    from hichap_master_amd import _lib, ice as ice_mod
    _lib.require_gpu()
    return ice_mod


@pytest.fixture(scope="module", autouse=True)
def _tiled_kernel_only(ice):
    """no flat tiles (build time), no single-launch sweep: k_sweep_tiled runs"""
    with tuned(flat_max=0, sweep_single=0):
        yield


def _entries(length, variant, epv):
    """entry count of a row segment: `length` uint4, or one entry below / above that boundary"""
    return max(0, epv * length + (variant - 1))


def _lengths_pixels():
    """rows 0..511 x columns [8192, 16384): row i holds a narrow segment
    (counts 1..7) and a wide one (counts 8..60000) whose lengths run through
    LENS x {one entry below, exact, one above a uint4 boundary}; a few entries
    per row in the short last column block (its mirror: a 300-row last block)"""
    n = 2 * KW + 300
    b1, b2, c = [], [], []
    for i in range(512):
        nn = _entries(LENS[i % 23], (i // 23) % 3, 8)
        nw = _entries(LENS[(i * 7 + 3) % 23], (i // 5) % 3, 4)
        k = np.arange(nn + nw)
        cols = KW + (i * 131 + k * 3) % KW  # distinct: 3 is coprime to 8192
        cnt = np.where(k < nn, 1 + (k + i) % 7, 8 + (k * 7919 + i * 31) % 59993)
        t = np.arange(i % 9)
        cols = np.concatenate([cols, 2 * KW + (i * 5 + t) % 300])
        cnt = np.concatenate([cnt, np.where(t % 4 == 3, 900 + i, 1 + t % 7)])
        b1.append(np.full(cols.size, i))
        b2.append(cols)
        c.append(cnt)
    return np.concatenate(b1), np.concatenate(b2), np.concatenate(c).astype(np.float64), n


def _ranges_pixels():
    """one tile of 512 rows x about 600 entries (narrow and wide mixed)"""
    n = 2 * KW
    rng = np.random.default_rng(77)
    b1, b2, c = [], [], []
    for i in range(512):
        m = 560 + int(rng.integers(0, 81))
        cols = KW + np.sort(rng.choice(KW, m, replace=False))
        cnt = np.where(rng.random(m) < 0.7, rng.integers(1, 8, m), rng.integers(8, 60001, m))
        b1.append(np.full(m, i))
        b2.append(cols)
        c.append(cnt)
    return np.concatenate(b1), np.concatenate(b2), np.concatenate(c).astype(np.float64), n


@pytest.fixture(scope="module", params=["lengths", "row ranges"])
def case(request, ice):
    """(matrix, n, row sums of its exported table)"""
    if request.param == "lengths":
        b1, b2, c, n = _lengths_pixels()
    else:
        b1, b2, c, n = _ranges_pixels()
    order = np.lexsort((b2, b1))
    off = np.array([0, n], np.int64)
    with tuned(unit_entries=4096 if request.param == "row ranges" else 0):
        m = ice.ContactMatrix.from_pixels(b1[order], b2[order], c[order], n, off)
    inf = m.info()
    assert inf["n_units_flat"] == 0 and inf["n_tiles"] >= 2, inf
    if request.param == "row ranges":
        assert inf["n_units"] > 40, inf  # the large tile is cut into row-range units
    e1, e2, ec = m.export_upper()
    assert ec.sum() == c.sum()
    sums = np.bincount(e1, weights=ec, minlength=n) + np.bincount(e2, weights=ec, minlength=n)
    yield m, n, sums
    m.close()


def _sweep(st, n, pf):
    """one sweep's marginals (count * b_i * b_j) of the state's biases"""
    import torch
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    with tuned(tiled_pf=pf):
        st.marg_local(2, out, None)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def _opts(ice):
    return ice.IceOptions(tol=0.0, max_iters=10, mad_max=0, min_nnz=0)


def test_row_sums_exact(ice, case):
    m, n, sums = case
    st = ice.IceState(m, _opts(ice))
    try:
        st.set_bias(np.ones(n))
        got = _sweep(st, n, 1)
    finally:
        st.close()
    assert sums.max() > 60000 and np.array_equal(sums, np.round(sums))
    np.testing.assert_array_equal(got, sums)


def test_one_sweep_bitwise(ice, case):
    m, n, _ = case
    b = np.random.default_rng(5).lognormal(0.0, 1.0, n)
    st = ice.IceState(m, _opts(ice))
    try:
        st.set_bias(b)
        want = _sweep(st, n, 0)
        got = _sweep(st, n, 1)
    finally:
        st.close()
    assert np.isfinite(want).all() and want.max() > 0
    np.testing.assert_array_equal(got, want)


def test_balance_bitwise(ice, case):
    m = case[0]
    opts = ice.IceOptions(max_iters=200)
    with tuned(tiled_pf=0):
        w0, s0 = ice.balance_matrix(m, opts)
    with tuned(tiled_pf=1):
        w1, s1 = ice.balance_matrix(m, opts)
    assert s1["iters"] == s0["iters"] and s0["iters"] > 1
    np.testing.assert_array_equal(w1, w0)
