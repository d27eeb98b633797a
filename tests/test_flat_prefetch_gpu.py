"""The column-grouped flat sweep with its runs carried raw (hh_tune
"flatw_pipe" 3, ice.hip flat_seg_c_raw / flat_seg_raw): the next run's loads
are issued before the current step's walk and masked only after it, and the
next tile's first runs are in flight while the row sums go out.  flatw_pipe 2
is the reference: every marginal, weight and iteration count is the same bit
for bit, for 8, 10 and 11 waves per block, and with b = 1 a sweep gives the
exported table's row sums exactly.

One matrix of short rows only (every tile flat), two chromosomes; cis-only
drops the contacts between them and balances them as separate groups, which
converge at different iterations.  The designed tiles (512-row blocks x
8192-column tiles, all cis) have narrow segments (counts 1..7, 8 per uint4)
and wide segments (counts >= 8, 4 per uint4) of the sizes in SHAPES; their
mirror images and the background contacts (_pixels) are further flat tiles of
other shapes, among them the short last row block's.
"""
import numpy as np
import pytest

from tests.knobs import tuned

pytestmark = pytest.mark.gpu

KW, KR = 8192, 512
N = 4 * KW + 300
SPLIT = 20000  # chromosomes [0, SPLIT) and [SPLIT, N)
# (first row, first column, columns available, narrow uint4, wide uint4, every row nonempty)
# narrow: 1, 7, 8, 9 (a last chunk shorter than 8 / one full element / one more), 511, 512, 513, 519, 520
# (one step of 64 * 8, one below / above, a second chunk of 1, 7, 8), 1500 and 1027 (several steps), 0;
# wide: 1, 127, 128, 129 (one step of 64 * 2 and one off), 300 and 515 (several steps), 0
SHAPES = [
    (0 * KR, 1 * KW, KW, 1, 127, False),
    (1 * KR, 1 * KW, KW, 7, 128, False),
    (2 * KR, 1 * KW, KW, 8, 129, False),
    (3 * KR, 1 * KW, KW, 9, 1, False),
    (4 * KR, 1 * KW, KW, 511, 300, False),
    (0 * KR, 2 * KW, SPLIT - 2 * KW, 512, 0, True),   # no wide entries, every row one uint4
    (1 * KR, 2 * KW, SPLIT - 2 * KW, 513, 5, True),
    (2 * KR, 2 * KW, SPLIT - 2 * KW, 519, 130, False),
    (3 * KR, 2 * KW, SPLIT - 2 * KW, 520, 64, False),
    (4 * KR, 2 * KW, SPLIT - 2 * KW, 1500, 515, True),
    (40 * KR, 3 * KW, KW, 0, 257, False),             # no narrow entries
    (41 * KR, 3 * KW, KW, 1027, 3, False),
]


def _row_lengths(total, full, seed):
    """uint4 per row of a 512-row block summing to `total`, each <= 40; `full`:
    no empty row (total >= 512), else rows with gaps between them"""
    rng = np.random.default_rng(seed)
    ln = np.zeros(KR, np.int64)
    if full:
        ln[:] = 1
    rows = np.arange(KR) if full else np.sort(rng.choice(KR, min(KR // 2, max(1, total)), replace=False))
    left = total - int(ln.sum())
    assert left >= 0
    while left > 0:
        r = int(rows[rng.integers(0, rows.size)])
        add = min(left, int(rng.integers(1, 9)), 40 - int(ln[r]))
        ln[r] += add
        left -= add
    assert ln.sum() == total and ln.max() <= 40
    return ln


def _pixels():
    b1, b2, c = [], [], []
    for t, (r0, c0, width, qn, qw, full) in enumerate(SHAPES):
        ln = _row_lengths(qn, full, 100 + t)
        lw = _row_lengths(qw, False, 200 + t)
        for i in range(KR):
            # a uint4 boundary, or up to 7 (3) entries below it: the padding of a row's last uint4
            nn = max(0, 8 * ln[i] - (i % 8 if ln[i] else 0))
            nw = max(0, 4 * lw[i] - (i % 4 if lw[i] else 0))
            if nn + nw == 0:
                continue
            k = np.arange(nn + nw)
            assert width % 3 and k.size < width
            cols = c0 + (i * 131 + k * 3) % width  # distinct: 3 is coprime to the width
            b1.append(np.full(k.size, r0 + i))
            b2.append(cols)
            # wide counts 8..100, and 600 times that (up to 60000) in every 64th row: a row scaled as a
            # whole keeps the matrix well conditioned for ICE, single huge counts would not
            big = 600 if i % 64 == 5 else 1
            c.append(np.where(k < nn, 1 + (k + i) % 7, big * (8 + (k * 7919 + i * 31) % 93)))
    # the short last column tile: five columns of eight narrow entries (its mirror: the 300-row last
    # row block, five rows of one uint4: a narrow segment shorter than a run)
    for j in range(5):
        b1.append(40 * KR + 17 * j + 64 * np.arange(8))
        b2.append(np.full(8, 4 * KW + 3 + 50 * j))
        c.append(1 + (j + np.arange(8)) % 7)
    # Background contacts so that ICE converges: the designed tiles alone are a bipartite graph (row
    # bins x column bins), on which the simultaneous update oscillates.  Random partners among the row
    # bins and among the column bins of each chromosome (other tiles than the designed ones; more flat
    # tiles of arbitrary shapes), and between the chromosomes (dropped in cis-only mode; without them
    # the genome-wide matrix has two components whose scales never agree).
    rng = np.random.default_rng(9)

    def background(lo, hi, lo2, hi2, k, cmax):
        r = np.repeat(np.arange(lo, hi), k)
        q = rng.integers(lo2, hi2, r.size)
        lo_, hi_ = np.minimum(r, q), np.maximum(r, q)
        keep = np.unique(lo_ * N + hi_, return_index=True)[1]
        keep = keep[hi_[keep] > lo_[keep]]
        b1.append(lo_[keep])
        b2.append(hi_[keep])
        c.append(rng.integers(1, cmax, keep.size))

    background(0, 5 * KR, 0, 5 * KR, 8, 30)
    background(KW, SPLIT, KW, SPLIT, 8, 30)
    background(40 * KR, 42 * KR, 40 * KR, 42 * KR, 8, 30)
    background(3 * KW, 4 * KW, 3 * KW, 4 * KW, 8, 30)
    background(0, 5 * KR, 3 * KW, 4 * KW, 4, 30)   # trans: row bins of chromosome 0 x column bins of 1
    background(KW, SPLIT, 3 * KW, 4 * KW, 2, 30)   # trans: column bins of 0 x column bins of 1
    b1, b2, c = np.concatenate(b1), np.concatenate(b2), np.concatenate(c).astype(np.float64)
    order = np.lexsort((b2, b1))
    return b1[order], b2[order], c[order]


@pytest.fixture(scope="module")
def ice():
    from hichap_master_amd import _lib, ice as ice_mod
    _lib.require_gpu()
    return ice_mod


@pytest.fixture(scope="module", autouse=True)
def _column_groups(ice):
    """column groups on this small matrix (build time): k_sweep_flatw runs"""
    with tuned(flat_cols=1):
        yield


@pytest.fixture(scope="module")
def pixels():
    return _pixels()


@pytest.fixture(scope="module", params=[0, 1], ids=["genome-wide", "cis-only"])
def case(request, ice, pixels):
    """(matrix, row sums of its exported table)"""
    b1, b2, c = pixels
    # distinct columns per row, nothing lost to a duplicate
    assert np.unique(b1 * N + b2).size == b1.size
    off = np.array([0, SPLIT, N], np.int64)
    m = ice.ContactMatrix.from_pixels(b1, b2, c, N, off, cis_only=request.param)
    inf = m.info()
    assert inf["n_units_flat"] > 0 and inf["n_units_flat"] == inf["n_units"], inf  # every tile flat
    e1, e2, ec = m.export_upper()
    kept = ((b1 < SPLIT) == (b2 < SPLIT)) if request.param else np.ones(b1.size, bool)
    assert not kept.all() or not request.param
    assert ec.sum() == c[kept].sum() and e1.size == kept.sum()
    sums = np.bincount(e1, weights=ec, minlength=N) + np.bincount(e2, weights=ec, minlength=N)
    yield m, sums
    m.close()


def _sweep(st, pipe, waves):
    """one sweep's marginals (count * b_i * b_j) of the state's biases"""
    import torch
    out = torch.zeros(N, dtype=torch.float64, device="cuda")
    with tuned(flatw_pipe=pipe, flatw_waves=waves):
        st.marg_local(2, out, None)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def _opts(ice):
    return ice.IceOptions(tol=0.0, max_iters=10, mad_max=0, min_nnz=0)


def test_shapes(pixels):
    """the designed tiles have the segment sizes of SHAPES"""
    b1, b2, c = pixels
    for r0, c0, width, qn, qw, full in SHAPES:
        t = (b1 >= r0) & (b1 < r0 + KR) & (b2 >= c0) & (b2 < c0 + width)
        nn = np.bincount(b1[t & (c < 8)] - r0, minlength=KR)
        nw = np.bincount(b1[t & (c >= 8)] - r0, minlength=KR)
        assert ((nn + 7) // 8).sum() == qn and ((nw + 3) // 4).sum() == qw
        assert ((nn > 0).all()) == full
        assert ((nn + 7) // 8).max() <= 64 and ((nw + 3) // 4).max() <= 64


@pytest.mark.parametrize("waves", [8, 10, 11])
def test_row_sums_exact(ice, case, waves):
    m, sums = case
    st = ice.IceState(m, _opts(ice))
    try:
        st.set_bias(np.ones(N))
        got = _sweep(st, 3, waves)
    finally:
        st.close()
    assert sums.max() > 60000 and np.array_equal(sums, np.round(sums))
    np.testing.assert_array_equal(got, sums)


@pytest.mark.parametrize("waves", [8, 10, 11])
def test_one_sweep_bitwise(ice, case, waves):
    m, _ = case
    b = np.random.default_rng(5).lognormal(0.0, 1.0, N)
    st = ice.IceState(m, _opts(ice))
    try:
        st.set_bias(b)
        want = _sweep(st, 2, waves)
        got = _sweep(st, 3, waves)
    finally:
        st.close()
    assert np.isfinite(want).all() and want.max() > 0
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("waves", [8, 10, 11])
def test_balance_bitwise(ice, case, request, waves):
    m = case[0]
    # (no bin filters: the sparse bins stay in; the CPU oracle takes 227 iterations genome-wide and
    # 92 / 148 for the two chromosomes)
    opts = ice.IceOptions(max_iters=400, mad_max=0, min_nnz=0)
    with tuned(flatw_waves=waves, flatw_pipe=2):
        w0, s0 = ice.balance_matrix(m, opts)
    with tuned(flatw_waves=waves, flatw_pipe=3):
        w1, s1 = ice.balance_matrix(m, opts)
    it0, it1 = np.atleast_1d(s0["iters"]), np.atleast_1d(s1["iters"])
    print("iterations:", it0)
    np.testing.assert_array_equal(it1, it0)
    assert it0.min() > 1 and it0.max() < 400
    if "cis-only" in request.node.name:
        # the chromosomes converge at different iterations: the earlier one's tiles are then skipped
        assert it0.size == 2 and it0[0] != it0[1], it0
    np.testing.assert_array_equal(w1, w0)
