"""``coolio.merge_coolers`` / ``coolio.downsample_cooler`` on small synthetic
two-chromosome coolers (100 kb bins): the written groups read back against
tests/merge_ref.py and tests/sample_ref.py, their indexes and metadata, the
other groups of a destination file kept, and the readers that consume them."""
import functools
import json

import numpy as np
import pytest

from hichap_master_amd import coolio, h5, ice, synth
from hichap_master_amd.sample import sample_threshold
from tests.merge_ref import merge_ref
from tests.sample_ref import sample_ref

pytestmark = pytest.mark.gpu

RES = 100000
CHROMS = [("1", 21_300_000), ("X", 12_750_000)]


@functools.lru_cache(maxsize=None)
def _genome(seed):
    nb = [-(-L // RES) for _, L in CHROMS]
    b1, b2, c, off = synth.coo_genome(nb, np.random.default_rng(seed), A=30.0, trans_density=0.05)
    c = c.astype(np.int32)
    for a in (b1, b2, c, off):
        a.setflags(write=False)
    return b1, b2, c, off


@pytest.fixture
def cools(tmp_path):
    paths = []
    for k, seed in enumerate((11, 12)):
        b1, b2, c, _ = _genome(seed)
        p = str(tmp_path / f"rep{k}.cool")
        coolio.create_cooler(p, {RES: (CHROMS, b1, b2, c)}, metadata={"rep": k}, assembly="hg19")
        paths.append(p)
    return paths


def _group_bytes(path, grp):
    out = {}
    with h5.File(path) as f:
        for sub in ("pixels", "bins", "indexes", "chroms"):
            g = f[f"{grp}/{sub}"]
            for k in g.keys():
                out[f"{sub}/{k}"] = (g[k].read().tobytes(), repr(sorted(dict(g[k].attrs).items(), key=str)))
    return out


def _check_group(uri, want):
    w1, w2, wc = want
    n = int(_genome(11)[3][-1])
    with coolio.Cooler(uri) as co:
        assert co.chromnames == [c for c, _ in CHROMS] and co.chromsizes == dict(CHROMS)
        assert co.binsize == RES and co.n_bins == n == co.info["nbins"]
        assert co.info["nnz"] == w1.size and co.info["assembly"] == "hg19"
        t1, t2, tc = co.pixels_table()
        np.testing.assert_array_equal(t1, w1)
        np.testing.assert_array_equal(t2, w2)
        np.testing.assert_array_equal(tc, wc)
        assert tc.dtype == np.int32 and t1.dtype == np.int64
        np.testing.assert_array_equal(co._g("indexes")["bin1_offset"].read(), np.searchsorted(w1, np.arange(n + 1)))
        np.testing.assert_array_equal(co.chrom_offsets(), _genome(11)[3])
        return json.loads(co.info["metadata"]), "weight" in co._g("bins")


def test_merge_coolers_new_file(cools, tmp_path):
    a, b = _genome(11), _genome(12)
    want = merge_ref([a[:3], b[:3]], int(a[3][-1]))
    assert want[0].size > max(a[0].size, b[0].size)              # the tables differ
    dst = str(tmp_path / "merged.cool")
    uris = [f"{p}::{RES}" for p in cools]
    out = coolio.merge_coolers(uris, f"{dst}::{RES}")
    for g, w in zip(out, want):
        np.testing.assert_array_equal(g, w)
    meta, has_weight = _check_group(f"{dst}::{RES}", want)
    assert meta == {"rep": 0, "merged-from": uris} and not has_weight
    assert coolio.cooler_groups(dst) == [str(RES)]
    # one source: the identity
    coolio.merge_coolers(uris[:1], dst)
    _check_group(f"{dst}::{RES}", a[:3])


def test_merge_into_a_source_file_keeps_its_other_groups(cools):
    a, b = _genome(11), _genome(12)
    coolio.zoomify(f"{cools[0]}::{RES}", [200000], balance=True)
    before = _group_bytes(cools[0], "200000")
    assert "bins/weight" in before
    uris = [f"{p}::{RES}" for p in cools]
    coolio.merge_coolers(uris, f"{cools[0]}::{RES}", balance=True, cis_only=True)
    assert sorted(coolio.cooler_groups(cools[0]), key=int) == [str(RES), "200000"]
    assert _group_bytes(cools[0], "200000") == before
    want = merge_ref([a[:3], b[:3]], int(a[3][-1]))
    meta, has_weight = _check_group(f"{cools[0]}::{RES}", want)
    assert has_weight and meta["merged-from"] == uris
    wt, st = ice.balance(*want, int(a[3][-1]), a[3], cis_only=True)
    with coolio.Cooler(f"{cools[0]}::{RES}") as co:
        np.testing.assert_array_equal(co.weights(), wt)          # NaNs in the same places


def test_downsample_cooler(cools, tmp_path):
    b1, b2, c, off = _genome(11)
    dst = str(tmp_path / "half.cool")
    out = coolio.downsample_cooler(f"{cools[0]}::{RES}", f"{dst}::{RES}", frac=1 / 2, seed=3)
    want = sample_ref(b1, b2, c, 2 ** 63, 3)
    for g, w in zip(out, want):
        np.testing.assert_array_equal(g, w)
    meta, has_weight = _check_group(f"{dst}::{RES}", want)
    assert meta == {"rep": 0, "sample": {"frac": 0.5, "threshold": str(2 ** 63), "seed": 3}} and not has_weight
    total = int(c.sum())
    assert abs(int(want[2].sum()) - total / 2) <= 5 * np.sqrt(total / 4)
    # a target total: the shallower replicate's depth
    target = total // 3
    coolio.downsample_cooler(f"{cools[0]}::{RES}", dst, count=target, seed=3, balance=True)
    want = sample_ref(b1, b2, c, sample_threshold(count=target, total=total), 3)
    meta, has_weight = _check_group(f"{dst}::{RES}", want)
    assert has_weight and meta["sample"]["threshold"] == str((target << 64) // total)


def test_structurefind_opens_a_merged_group(cools, tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    dst = str(tmp_path / "merged.cool")
    coolio.merge_coolers([f"{p}::{RES}" for p in cools], dst, balance=True)
    out = str(tmp_path / "ins")
    r = StructureFind(cooler_fil=dst, Res=RES).run_Insulation(out, windows=(1000000,))
    assert sorted(r) == sorted(n for n, _ in CHROMS)
    assert r["1"]["L"].shape == (1, -(-CHROMS[0][1] // RES)) and np.isfinite(r["1"]["L"]).any()
