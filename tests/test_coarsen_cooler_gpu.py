"""``coolio.coarsen_cooler`` / ``coolio.zoomify`` on a small synthetic
multi-chromosome cooler (100 kb bins; chromosome lengths that are no multiple
of any coarse bin size): every level against the block sum of the fine dense
matrix, its indexes and bin table, the source group kept byte for byte, the
balanced levels against ``ice.balance`` on their tables, and the readers that
consume the new groups."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from hichap_master_amd import coolio, h5, ice, synth
from tests.coarsen_ref import coarsen_ref, dense_block_sum, table_to_dense

pytestmark = pytest.mark.gpu

RES = 100000
CHROMS = [("1", 61_300_000), ("2", 43_500_000), ("X", 25_700_000)]
LEVELS = (200000, 500000, 1000000)        # 1 Mb is taken from 500 kb (x 2), the others from the base


@functools.lru_cache(maxsize=None)
def _genome():
    nb = [-(-L // RES) for _, L in CHROMS]
    b1, b2, c, off = synth.coo_genome(nb, np.random.default_rng(11), A=30.0, trans_density=0.05)
    c = c.astype(np.int32)
    for a in (b1, b2, c, off):
        a.setflags(write=False)
    return b1, b2, c, off


@pytest.fixture
def cool(tmp_path):
    b1, b2, c, off = _genome()
    path = str(tmp_path / "sample.cool")
    coolio.create_cooler(path, {RES: (CHROMS, b1, b2, c)}, metadata={"onlyIntra": "False"}, assembly="hg19")
    return path


def _group_bytes(path, grp):
    out = {}
    with h5.File(path) as f:
        for sub in ("pixels", "bins", "indexes", "chroms"):
            g = f[f"{grp}/{sub}"]
            for k in g.keys():
                out[f"{sub}/{k}"] = (g[k].read().tobytes(), repr(sorted(dict(g[k].attrs).items(), key=str)))
    return out


def _check_level(path, res):
    b1, b2, c, off = _genome()
    k = res // RES
    w1, w2, wc, woff = coarsen_ref(b1, b2, c, off, k)
    D = table_to_dense(b1, b2, c, int(off[-1]))
    with coolio.Cooler(f"{path}::{res}") as co:
        assert co.chromnames == [n for n, _ in CHROMS] and co.chromsizes == dict(CHROMS)
        assert co.binsize == res == co.info["bin-size"]
        assert co.info["nnz"] == w1.size and co.info["nbins"] == int(woff[-1]) == co.n_bins
        assert co.info["storage-mode"] == "symmetric-upper" and co.info["assembly"] == "hg19"
        np.testing.assert_array_equal(co.chrom_offsets(), woff)
        assert woff.tolist() == np.concatenate([[0], np.cumsum([-(-L // res) for _, L in CHROMS])]).tolist()
        t1, t2, tc = co.pixels_table()
        np.testing.assert_array_equal(t1, w1)
        np.testing.assert_array_equal(t2, w2)
        np.testing.assert_array_equal(tc, wc)
        assert tc.dtype == np.int32 and t1.dtype == np.int64
        np.testing.assert_array_equal(co._g("indexes")["bin1_offset"].read(),
                                      np.searchsorted(w1, np.arange(int(woff[-1]) + 1)))
        start, end = co._g("bins")["start"].read(), co._g("bins")["end"].read()
        for q, (name, L) in enumerate(CHROMS):
            lo, hi = int(woff[q]), int(woff[q + 1])
            s = np.arange(0, L, res)
            np.testing.assert_array_equal(start[lo:hi], s)
            np.testing.assert_array_equal(end[lo:hi], np.minimum(s + res, L))
            flo, fhi = int(off[q]), int(off[q + 1])
            want = dense_block_sum(D[flo:fhi, flo:fhi], [0, fhi - flo], k)
            np.testing.assert_array_equal(co.matrix(balance=False).fetch(name), want)
    return w1, w2, wc, woff


def test_zoomify_levels_new_file(cool, tmp_path):
    dst = str(tmp_path / "zoom.mcool")
    nnz = coolio.zoomify(f"{cool}::{RES}", LEVELS, dst_path=dst)
    assert sorted(coolio.cooler_groups(dst), key=int) == [str(r) for r in LEVELS]
    for res in LEVELS:
        w = _check_level(dst, res)
        assert nnz[res] == w[0].size
    assert sorted(coolio.cooler_groups(cool)) == [str(RES)]        # the source file is untouched


def test_zoomify_into_source_keeps_source_group(cool):
    w = np.linspace(0.5, 2.0, int(_genome()[3][-1]))
    w[::9] = np.nan
    h5.append_dataset(cool, f"{RES}/bins", "weight", w, {"cis_only": False, "ignore_diags": 1, "scale": 12.5})
    before = _group_bytes(cool, str(RES))
    assert "bins/weight" in before
    coolio.zoomify(f"{cool}::{RES}", LEVELS)
    assert sorted(coolio.cooler_groups(cool), key=int) == [str(RES)] + [str(r) for r in LEVELS]
    assert _group_bytes(cool, str(RES)) == before
    for res in LEVELS:
        _check_level(cool, res)
    # again, one level: the other levels and the source stay as they are
    lv = _group_bytes(cool, "500000")
    coolio.zoomify(f"{cool}::{RES}", [200000])
    assert _group_bytes(cool, str(RES)) == before and _group_bytes(cool, "500000") == lv


def test_coarsen_cooler(cool, tmp_path):
    dst = str(tmp_path / "c5.cool")
    o1, o2, oc = coolio.coarsen_cooler(f"{cool}::{RES}", f"{dst}::500000", 5)
    w1, w2, wc, _ = _check_level(dst, 500000)
    np.testing.assert_array_equal(o1, w1)
    np.testing.assert_array_equal(oc, wc)
    assert coolio.cooler_groups(dst) == ["500000"]
    with pytest.raises(ValueError):
        coolio.coarsen_cooler(f"{cool}::{RES}", f"{dst}::400000", 5)
    # into the source's file: its group survives byte for byte
    before = _group_bytes(cool, str(RES))
    coolio.coarsen_cooler(f"{cool}::{RES}", f"{cool}::200000", 2, balance=True, cis_only=True)
    assert _group_bytes(cool, str(RES)) == before
    t = _check_level(cool, 200000)
    wt, st = ice.balance(t[0], t[1], t[2], int(t[3][-1]), t[3], cis_only=True)
    with coolio.Cooler(f"{cool}::200000") as co:
        np.testing.assert_array_equal(co.weights(), wt)
    # a level of a level: 100 kb -> 200 kb -> 1 Mb equals 100 kb -> 1 Mb
    coolio.coarsen_cooler(f"{cool}::200000", f"{cool}::1000000", 5)
    _check_level(cool, 1000000)


def test_zoomify_balanced_levels(cool):
    coolio.zoomify(f"{cool}::{RES}", LEVELS, balance=True)
    for res in LEVELS:
        t = _check_level(cool, res)
        wt, st = ice.balance(t[0], t[1], t[2], int(t[3][-1]), t[3])
        with coolio.Cooler(f"{cool}::{res}") as co:
            np.testing.assert_array_equal(co.weights(), wt)         # NaNs in the same places
        a = h5.File(cool)[f"{res}/bins/weight"].attrs
        for key in ("tol", "min_nnz", "min_count", "mad_max", "cis_only", "ignore_diags", "converged", "var",
                    "scale", "divisive_weights"):
            assert key in a, key
        assert a["cis_only"] is False and a["ignore_diags"] == 1 and a["mad_max"] == 5
        assert a["converged"] == st["converged"] and a["scale"] == st["scale"] and a["var"] == st["var"]


def test_structurefind_reads_the_new_groups(cool, tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    coolio.zoomify(f"{cool}::{RES}", [200000, 500000], balance=True)
    b1, b2, c, off = _genome()
    D = table_to_dense(b1, b2, c, int(off[-1]))
    sf = StructureFind(cooler_fil=cool, Res=200000)
    comp = sf.Compartment()
    for q, (name, L) in enumerate(CHROMS):
        flo, fhi = int(off[q]), int(off[q + 1])
        M = dense_block_sum(D[flo:fhi, flo:fhi], [0, fhi - flo], 2)
        np.testing.assert_array_equal(comp[name], StructureFind(Res=200000).compartment(M))
    out = str(tmp_path / "ins")
    r = StructureFind(cooler_fil=cool, Res=500000).run_Insulation(out, windows=(2000000,))
    assert sorted(r) == sorted(n for n, _ in CHROMS)
    assert r["1"]["L"].shape == (1, -(-CHROMS[0][1] // 500000)) and np.isfinite(r["1"]["L"]).any()
    assert len(os.listdir(out)) == 2


H5 = os.environ.get("HDF5_PREFIX", "/opt/conda")
HAVE_H5 = all(os.path.exists(os.path.join(H5, p)) for p in ("include/hdf5.h", "lib/libhdf5.so", "bin/h5dump"))


@pytest.mark.skipif(not HAVE_H5 or shutil.which("gcc") is None, reason="libhdf5 tools absent")
def test_libhdf5_header_dump(cool):
    """The header dump tests/test_h5_libhdf5.py applies to written coolers."""
    coolio.zoomify(f"{cool}::{RES}", LEVELS, balance=True)
    r = subprocess.run([os.path.join(H5, "bin", "h5dump"), "-H", cool], capture_output=True, text=True)
    assert r.returncode == 0 and "error" not in (r.stdout + r.stderr).lower(), r.stderr[-2000:]
