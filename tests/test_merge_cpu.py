"""``merge.merge_pixels`` / ``coolio.merge_coolers`` without a GPU: every
argument error is raised before the library is called, and the restatement
(tests/merge_ref.py) sums what it should."""
import numpy as np
import pytest

from hichap_master_amd import coolio
from hichap_master_amd.merge import MAX_TABLES, merge_pixels
from tests.merge_ref import merge_ref

T = (np.array([0, 0, 2]), np.array([0, 3, 2]), np.array([1, 2, 3]))


def test_merge_ref_by_hand():
    a = ([0, 0, 2], [0, 3, 2], [1, 2, 3])
    b = ([0, 1, 2], [3, 1, 2], [2 ** 40, 0, 5])
    o1, o2, oc = merge_ref([a, b], 4)
    assert o1.tolist() == [0, 0, 1, 2] and o2.tolist() == [0, 3, 1, 2]
    assert oc.tolist() == [1, 2 ** 40 + 2, 0, 8] and oc.dtype == np.int64
    e = merge_ref([([], [], []), ([], [], [])], 4)
    assert all(x.size == 0 for x in e)


def test_merge_pixels_argument_errors():
    import torch
    assert MAX_TABLES == 64
    with pytest.raises(ValueError):
        merge_pixels([], 4)                                     # K = 0
    with pytest.raises(ValueError):
        merge_pixels([T] * 65, 4)                               # K > 64
    with pytest.raises(ValueError):
        merge_pixels([T, tuple(torch.from_numpy(x) for x in T)], 4)      # host and device tables mixed
    with pytest.raises(ValueError):
        merge_pixels([T, (T[0], torch.from_numpy(T[1]), T[2])], 4)
    with pytest.raises(ValueError):
        merge_pixels([T, T[:2]], 4)
    with pytest.raises(ValueError):
        merge_pixels([T], 0)
    with pytest.raises(ValueError, match="GPU merging takes integer counts"):
        merge_pixels([T, (T[0], T[1], T[2] + 0.5)], 4)          # float counts that are no integers
    with pytest.raises(ValueError):
        merge_pixels([T, (T[0], T[1][:2], T[2])], 4)


def _cool(path, chroms, res=1000):
    nb = sum(-(-L // res) for _, L in chroms)
    b1 = np.arange(nb, dtype=np.int64)
    coolio.create_cooler(path, {res: (chroms, b1, b1, np.ones(nb, np.int32))})
    return f"{path}::{res}"


def test_merge_coolers_argument_errors(tmp_path):
    chroms = [("1", 9500), ("2", 4000)]
    a = _cool(str(tmp_path / "a.cool"), chroms)
    dst = str(tmp_path / "m.cool")
    with pytest.raises(ValueError, match="bp"):                  # another chromosome length
        coolio.merge_coolers([a, _cool(str(tmp_path / "b.cool"), [("1", 9500), ("2", 4100)])], dst)
    with pytest.raises(ValueError, match="chromosome 1 is 2"):   # another name
        coolio.merge_coolers([a, _cool(str(tmp_path / "c.cool"), [("1", 9500), ("X", 4000)])], dst)
    with pytest.raises(ValueError, match="bin sizes"):
        coolio.merge_coolers([a, _cool(str(tmp_path / "d.cool"), chroms, res=500)], dst)
    with pytest.raises(ValueError, match="chromosomes in one cooler"):
        coolio.merge_coolers([a, a, _cool(str(tmp_path / "e.cool"), chroms[:1])], dst)
    with pytest.raises(ValueError):
        coolio.merge_coolers([], dst)
    with pytest.raises(ValueError):
        coolio.merge_coolers([a] * 65, dst)
    with pytest.raises(ValueError, match="resolution"):
        coolio.merge_coolers([a, a], dst + "::2000")
