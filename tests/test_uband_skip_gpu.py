"""Cis-only dense bands and the upper-band sweep without its dead rectangles
(hh_tune "band_cis" and "ub_skip").  A trans pixel inside
the band widths goes to the tiles, so every band slot past a row's chromosome
end is 0; a wave task (128 rows x one 1008-slot chunk) made of such slots only
is not walked, and a workgroup of four such tasks is not launched.  The
marginals are the exported table's, ub_skip 0 and 1 agree bit for bit, and so
do row shards with the whole matrix (the dead test depends on global rows and
chromosome offsets only)."""
import numpy as np
import pytest

from hichap_master_amd import synth
from oracle import ice_ref
from tests import uband_dead_ref as ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ice():
    from hichap_master_amd import _lib, ice as ice_mod
    _lib.require_gpu()
    return ice_mod


@pytest.fixture(autouse=True)
def _force_uband(ice):
    """the upper-band sweep whatever the size (these matrices are below the
    automatic threshold)"""
    with tuned(uband=2):
        yield


# ------------------------------------------------------------ synthetic case
# the C4 model (its A and trans density) on a small genome whose chromosome
# sizes are multiples of the 512-row workgroup: W8 2 400 (three uint8 chunks),
# W4 3 712 (two nibble chunks); the 640-row chromosome's nibble rectangles
# are all dead, the other two have dead tails
_SIZES = [5120, 3072, 640]
_MODEL = {}


def _model():
    if not _MODEL:
        A, td = synth.calibrate(synth.genome_bins(10000, diploid=True), 5e9, 0.2)
        _MODEL.update(A=A, trans_density=td, comp_block=200, seed=20201015)
    return dict(_MODEL)


@pytest.fixture(scope="module")
def genome(ice):
    """the matrix, its exported table (once) and the NumPy dead table"""
    with tuned(uband=2):
        m = ice.ContactMatrix.synthetic(list(_SIZES), **_model())
    inf = m.info()
    b1, b2, c = m.export_upper()
    off = np.concatenate([[0], np.cumsum(_SIZES)]).astype(np.int64)
    g = dict(m=m, inf=inf, b1=b1, b2=b2, c=c, off=off, n=int(off[-1]),
             dead=ref.dead(off, int(inf["band_w"]), int(inf["band_w4"])))
    yield g
    m.close()


def _one_sweep_opts(ice):
    return ice.IceOptions(tol=0.0, max_iters=10, mad_max=0, min_nnz=0)


def _sweep(st, n, skip):
    """one sweep's marginals (count * b_i * b_j) of the state's biases"""
    import torch
    out = torch.zeros(n, dtype=torch.float64, device="cuda")
    with tuned(ub_skip=1 if skip else 0):
        st.marg_local(2, out, None)
        torch.cuda.synchronize()
    return out.cpu().numpy()


def test_not_vacuous(ice, genome):
    inf, dead, off = genome["inf"], genome["dead"], genome["off"]
    w8, w4 = int(inf["band_w"]), int(inf["band_w4"])
    assert w8 > 1008 and w4 > w8 and not inf["upper"], inf
    ch = ref.chunks(w8, w4)
    bits = np.array([b for b, _, _ in ch])
    assert (bits == 8).sum() >= 2 and (bits == 4).sum() >= 2, inf  # several chunks per segment
    st = ice.IceState(genome["m"], _one_sweep_opts(ice))
    try:
        skipped, tasks = st.uband_skipped()
        swept = {}
        for skip in (0, 1):
            with tuned(ub_skip=skip):
                swept[skip] = st.swept_bytes()
    finally:
        st.close()
    assert tasks == dead.size and skipped == int(dead.sum()) > 0
    assert dead[64:69, bits == 4].all()  # the 640-row chromosome's nibble rectangles
    # the band bytes of the dead rectangles leave the byte count: a row's
    # W8 + 16 uint8 and (W4 - W8) / 2 + 16 nibble bytes, 1008 slots per chunk
    n8, n4 = int((bits == 8).sum()), int((bits == 4).sum())
    cb = [1008] * (n8 - 1) + [w8 + 16 - 1008 * (n8 - 1)] + [504] * (n4 - 1) + [(w4 - w8) // 2 + 16 - 504 * (n4 - 1)]
    assert swept[0] - swept[1] == 128 * int((dead * np.array(cb)).sum())
    # a trans pixel that the band could have held, inside a dead rectangle
    b1, b2, c = genome["b1"], genome["b2"], genome["c"]
    chrom = np.searchsorted(off, np.arange(genome["n"]), side="right") - 1
    d = b2 - b1
    trans = chrom[b1] != chrom[b2]
    fits = trans & (((d <= w8) & (c <= 255)) | ((d > w8) & (d <= w4) & (c <= 15)))
    assert fits.sum() > 1000
    hit = 0
    for k, (cbits, kc, base) in enumerate(ch):
        in_chunk = fits & (d >= base) & (d < base + 1008 - 15) & ((d <= w8) == (cbits == 8))
        hit += int(dead[b1[in_chunk] // 128, k].sum())
    assert hit > 0


def test_row_sums_equal_export(ice, genome):
    """b = 1: the marginals are the row sums of the exported table, exactly"""
    n = genome["n"]
    want = (np.bincount(genome["b1"], weights=genome["c"], minlength=n) +
            np.bincount(genome["b2"], weights=genome["c"], minlength=n))
    st = ice.IceState(genome["m"], _one_sweep_opts(ice))
    try:
        got = _sweep(st, n, True)
        assert st.uband_fallbacks() == 0
    finally:
        st.close()
    assert want.max() > 0 and np.array_equal(want, np.round(want))
    np.testing.assert_array_equal(got, want)


def test_lognormal_biases(ice, genome):
    """log-normal biases: the table's marginals at the full-size window
    tolerance; ub_skip 0 and 1 bit for bit; no workgroup leaves the fast walk"""
    n, b1, b2, c = genome["n"], genome["b1"], genome["b2"], genome["c"]
    b = np.random.default_rng(5).lognormal(0.0, 1.0, n)
    v = c * b[b1] * b[b2]
    want = np.bincount(b1, weights=v, minlength=n) + np.bincount(b2, weights=v, minlength=n)
    st = ice.IceState(genome["m"], _one_sweep_opts(ice))
    try:
        st.set_bias(b)
        walked = _sweep(st, n, False)
        got = _sweep(st, n, True)
        again = _sweep(st, n, False)  # (the partials a skipped task leaves untouched were zeros)
        assert st.uband_fallbacks() == 0
    finally:
        st.close()
    np.testing.assert_array_equal(got, walked)
    np.testing.assert_array_equal(again, walked)
    np.testing.assert_allclose(got, want, rtol=1e-12)


def _balance(ice, opts, row_ranges=None):
    """balance the genome whole, or as row shards on one GPU with a manual
    marginal gather (the sharded driver's exchange)"""
    sizes, kw = list(_SIZES), _model()
    if row_ranges is None:
        m = ice.ContactMatrix.synthetic(sizes, **kw)
        try:
            return ice.balance_matrix(m, opts)
        finally:
            m.close()
    from tests.shard_exchange import balance_states
    rr = np.asarray(row_ranges, dtype=np.int64)
    shards = [ice.ContactMatrix.synthetic(sizes, row_range=(int(rr[k]), int(rr[k + 1])), **kw)
              for k in range(len(rr) - 1)]
    states = [ice.IceState(m, opts) for m in shards]
    try:
        dead = [st.uband_skipped()[0] for st in states]
        res = balance_states(states, rr, opts.max_iters)
    finally:
        for st in states:
            st.close()
        for m in shards:
            m.close()
    assert dead[-1] > 0  # (the last shard holds chromosome ends)
    for w, _ in res[1:]:
        np.testing.assert_array_equal(w, res[0][0])
    return res[0]


@pytest.fixture(scope="module")
def whole(ice):
    with tuned(uband=2):
        return _balance(ice, ice.IceOptions(max_iters=60))


def test_balance_skip_bitwise(ice, whole):
    with tuned(ub_skip=0):
        w, s = _balance(ice, ice.IceOptions(max_iters=60))
    np.testing.assert_array_equal(w, whole[0])
    assert s["iters"] == whole[1]["iters"]


# 512-row cuts inside the first and the second chromosome
@pytest.mark.parametrize("cuts", [[0, 2560, 8832], [0, 1024, 6656, 8832]])
def test_shards_bitwise(ice, whole, cuts):
    w, s = _balance(ice, ice.IceOptions(max_iters=60), row_ranges=cuts)
    np.testing.assert_array_equal(w, whole[0])
    assert s["iters"] == whole[1]["iters"]


# ---------------------------------------------------------- pixel-table case
_PX_SIZES = [1024, 512, 384]
_PX_W = 1024  # forced uint8 band: chunk 1 (from diagonal 1008) is dead for the two short chromosomes


@pytest.fixture(scope="module")
def table():
    """counts at and beyond both band ranges (300 > 255, 16 > 15), as the
    pixel genome of tests/test_uband_fast_gpu.py"""
    rng = np.random.default_rng(31)
    b1, b2, c, off = synth.coo_genome(list(_PX_SIZES), rng, A=60.0, trans_density=0.02)
    c = c.copy()
    c[::97] = 300
    c[5::89] = 16
    return b1, b2, c, off, int(off[-1])


def _build(ice, table, how, cis_only=False):
    import torch
    b1, b2, c, off, n = table
    with tuned(band_w=_PX_W, host_build=1 if how == "host" else 0):
        if how == "device":
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()  # noqa: E731
            return ice.ContactMatrix.from_device_pixels(t(b1), t(b2), t(c), n, off, cis_only=cis_only)
        return ice.ContactMatrix.from_pixels(b1, b2, c, n, off, cis_only=cis_only)


def _balance_px(ice, m, cis_only=False):
    opts = ice.IceOptions(cis_only=cis_only)
    st = ice.IceState(m, opts)
    skipped, tasks = st.uband_skipped()
    st.close()
    return ice.balance_matrix(m, opts), skipped, tasks


def test_pixel_table_builders_and_oracle(ice, table):
    b1, b2, c, off, n = table
    dead = ref.dead(off, _PX_W, _PX_W)
    assert dead.shape == (15, 2) and dead[8:, 1].all() and not dead[0, 1] and not dead[:, 0].any()
    res = {}
    for how in ("host", "device"):
        m = _build(ice, table, how)
        try:
            inf = m.info()
            assert inf["band_w"] == inf["band_w4"] == _PX_W, inf
            res[how] = (_balance_px(ice, m), inf["n_band"], m.export_upper())
        finally:
            m.close()
    (wh, sh), skipped, tasks = res["host"][0]
    (wd, sd), skipped_d, _ = res["device"][0]
    assert skipped == skipped_d == int(dead.sum()) and tasks == dead.size
    assert res["host"][1] == res["device"][1]
    for x, y in zip(res["host"][2], res["device"][2]):
        np.testing.assert_array_equal(x, y)
    # the table comes back whole: trans pixels inside the band width included
    e1, e2, ec = res["host"][2]
    keep = b1 != b2  # (ignore_diags 1)
    o = np.lexsort((e2, e1))
    np.testing.assert_array_equal(e1[o], b1[keep])
    np.testing.assert_array_equal(e2[o], b2[keep])
    np.testing.assert_array_equal(ec[o], c[keep])
    chrom = np.searchsorted(off, np.arange(n), side="right") - 1
    cis_fits = (chrom[b1] == chrom[b2]) & keep & (b2 - b1 <= _PX_W) & (c <= 255)
    assert res["host"][1] == 2 * int(cis_fits.sum())  # both triangles; no trans pixel in the band
    np.testing.assert_array_equal(wd, wh)
    assert sd["iters"] == sh["iters"]
    w_ref, st_ref = ice_ref.balance(b1, b2, c, n, off)
    assert sh["iters"] == st_ref["iters"]
    np.testing.assert_allclose(wh, w_ref, rtol=1e-9, equal_nan=True)


def test_pixel_table_cis_only_layout_unchanged(ice, table):
    """--cis-only never stored a trans pixel: the layout, and so every bit of
    the weights, is that of band_cis 0"""
    out = {}
    for cis in (1, 0):
        with tuned(band_cis=cis):
            m = _build(ice, table, "auto", cis_only=True)
        try:
            (w, s), skipped, _ = _balance_px(ice, m, cis_only=True)
            out[cis] = (w, s, skipped, m.info()["n_band"])
        finally:
            m.close()
    assert out[1][2] > 0 and out[0][2] == 0  # (without the rule no rectangle is known to be empty)
    assert out[1][3] == out[0][3]
    np.testing.assert_array_equal(out[1][0], out[0][0])
    np.testing.assert_array_equal(np.atleast_1d(out[1][1]["iters"]), np.atleast_1d(out[0][1]["iters"]))
