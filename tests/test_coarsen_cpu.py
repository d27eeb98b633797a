"""The host side of coarsen / zoomify (hichap_master_amd/coarsen.py) and the
NumPy restatement the GPU tests compare with (tests/coarsen_ref.py): the bin
map on ragged chromosomes, the restatement against a dense block sum, the
zoom plan, the composition identity and the float-count rule.  No GPU."""
import numpy as np
import pytest

from tests.coarsen_ref import coarsen_ref, dense_block_sum, ref_bin_map, ref_offsets, table_to_dense

RAGGED = (37, 5, 1, 64)
OFF = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
FACTORS = (1, 2, 4, 5, 50, 64, 100)


def _table(rng, off=OFF, density=0.2, hi=40):
    n = int(off[-1])
    i, j = np.triu_indices(n)
    keep = rng.random(i.size) < density
    return i[keep].astype(np.int64), j[keep].astype(np.int64), rng.integers(1, hi, int(keep.sum())).astype(np.int32)


@pytest.mark.parametrize("k", FACTORS)
def test_coarse_offsets_and_map(k):
    from hichap_master_amd.coarsen import coarse_bin_map, coarse_offsets
    coff = coarse_offsets(OFF, k)
    assert coff.dtype == np.int64
    assert coff.tolist() == np.concatenate([[0], np.cumsum([-(-n // k) for n in RAGGED])]).tolist()
    m = coarse_bin_map(OFF, k)
    assert m.shape == (int(OFF[-1]),) and m.dtype == np.int64
    # from the definition, bin by bin; a coarse bin never spans two chromosomes
    want = []
    for c, n in enumerate(RAGGED):
        want += [int(coff[c]) + i // k for i in range(n)]
    assert m.tolist() == want
    for c in range(len(RAGGED)):
        seg = m[OFF[c]:OFF[c + 1]]
        assert seg.min() == coff[c] and seg.max() == coff[c + 1] - 1
    np.testing.assert_array_equal(m, ref_bin_map(OFF, k))
    np.testing.assert_array_equal(coff, ref_offsets(OFF, k))
    if k == 1:
        assert m.tolist() == list(range(int(OFF[-1])))


def test_map_argument_errors():
    from hichap_master_amd.coarsen import coarse_bin_map, coarse_offsets
    with pytest.raises(ValueError):
        coarse_offsets(OFF, 0)
    with pytest.raises(ValueError):
        coarse_bin_map(OFF, 2.5)
    with pytest.raises(ValueError):
        coarse_offsets([0, 5, 3], 2)


@pytest.mark.parametrize("k", FACTORS)
def test_restatement_against_dense_block_sum(k):
    rng = np.random.default_rng(100 + k)
    b1, b2, c = _table(rng)
    o1, o2, oc, coff = coarsen_ref(b1, b2, c, OFF, k)
    nbc = int(coff[-1])
    assert oc.dtype == np.int64 and int(oc.sum()) == int(c.astype(np.int64).sum())
    assert np.all(o1 <= o2) and np.all(np.diff(o1 * nbc + o2) > 0)
    D = table_to_dense(b1, b2, c, int(OFF[-1]))
    want = dense_block_sum(D, OFF, k)
    np.testing.assert_array_equal(table_to_dense(o1, o2, oc, nbc), want)
    # every nonzero cell of the block sum is a stored pixel (counts here are >= 1)
    assert o1.size == np.count_nonzero(np.triu(want))


def test_restatement_keeps_stored_zeros_and_is_exact_past_2_53():
    b1 = np.array([0, 0, 2], dtype=np.int64)
    b2 = np.array([0, 1, 3], dtype=np.int64)
    o1, o2, oc, _ = coarsen_ref(b1, b2, np.array([2 ** 62, 2 ** 62 - 1, 0]), [0, 4], 2)
    assert (o1.tolist(), o2.tolist(), oc.tolist()) == ([0, 1], [0, 1], [2 ** 63 - 1, 0])


def test_composition_on_the_restatement():
    """k = 2 twice equals k = 4, the coarse offsets included: what zoomify relies on."""
    rng = np.random.default_rng(9)
    b1, b2, c = _table(rng)
    a1, a2, ac, aoff = coarsen_ref(b1, b2, c, OFF, 2)
    t1, t2, tc, toff = coarsen_ref(a1, a2, ac, aoff, 2)
    w1, w2, wc, woff = coarsen_ref(b1, b2, c, OFF, 4)
    for got, want in ((t1, w1), (t2, w2), (tc, wc), (toff, woff)):
        np.testing.assert_array_equal(got, want)


def test_zoom_plan():
    from hichap_master_amd.coarsen import zoom_plan
    assert zoom_plan(10000, [40000, 200000, 500000, 1000000]) == [
        (40000, 10000, 4), (200000, 40000, 5), (500000, 10000, 50), (1000000, 500000, 2)]
    # any order, repeats once
    assert zoom_plan(10000, [1000000, 40000, 40000]) == [(40000, 10000, 4), (1000000, 40000, 25)]
    assert zoom_plan(40000, []) == []
    for bad in ([15000], [10000], [5000], [40000, 25000]):
        with pytest.raises(ValueError):
            zoom_plan(10000, bad)


def test_non_integer_float_counts_raise():
    from hichap_master_amd.coarsen import coarsen_pixels, integer_counts
    b1 = np.array([0, 1], dtype=np.int64)
    with pytest.raises(ValueError, match="GPU coarsening takes integer counts"):
        coarsen_pixels(b1, b1 + 1, np.array([1.0, 2.5]), [0, 3], 2)
    with pytest.raises(ValueError, match="GPU coarsening takes integer counts"):
        coarsen_pixels(b1, b1 + 1, np.array([1.0, np.nan]), [0, 3], 2)
    # integer-valued floats are cast, as balance_cooler does
    c = integer_counts(np.array([3.0, 0.0, 7.0]))
    assert c.dtype == np.int64 and c.tolist() == [3, 0, 7]
