"""The shared stage of one chromosome's pixel table (csrc/pixel_table.hpp):
the band build reads the chromosome's slice of the weights by local index,
device tables are used in place, and an empty table still gets its ``valid``
from the weights and ``bad``.  The table is test_insulation_gpu's (11 / 200 / 9
bins, the middle chromosome queried, trans pixels on both sides); the weights
are genome-wide with a NaN in the first chromosome and at the last bin of the
last, which a read outside the slice would pick up."""
import functools

import numpy as np
import pytest

from hichap_master_amd import insulation as ins
from hichap_master_amd._lib import call, ptr
from hichap_master_amd.StructureFind import column_band
from tests import insulation_ref as ref
from tests.test_insulation_gpu import LO, N, NB, _table

pytestmark = pytest.mark.gpu

BANDS = (0, 30, N + 5)
WINDOWS = (1, 5, 17)
BAD = (0, 57, N - 1)


@functools.lru_cache(maxsize=None)
def _weights():
    w = np.random.default_rng(11).uniform(0.05, 3.0, NB)
    w[[3, LO + 90, NB - 1]] = np.nan          # in 'a', in 'b' (its cells are 0), the last bin of 'c'
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _dense():
    """The dense matrix of 'b' as cooler balances it (NaN -> 0)."""
    b1, b2, cnt = _table()
    w = _weights()
    keep = (b1 >= LO) & (b2 < LO + N)
    val = np.nan_to_num(cnt[keep] * w[b1[keep]] * w[b2[keep]])
    M = np.zeros((N, N))
    M[b1[keep] - LO, b2[keep] - LO] = val
    M[b2[keep] - LO, b1[keep] - LO] = val
    M.setflags(write=False)
    return M


def _band(b1, b2, cnt, w, B, device):
    """hh_band_from_pixels of chromosome 'b', host arrays or device tensors."""
    if not device:
        band = np.full((2 * B + 1, N), -1.0)
        call("hh_band_from_pixels", ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), NB, LO, N, B, ptr(band), 0, None)
        return band
    import torch
    b1, b2, cnt, w = (torch.from_numpy(np.array(a)).cuda() for a in (b1, b2, cnt, w))
    band = torch.full((2 * B + 1, N), -1.0, dtype=torch.float64, device="cuda")
    call("hh_band_from_pixels", ptr(b1), ptr(b2), ptr(cnt), b1.numel(), ptr(w), NB, LO, N, B, ptr(band), 1, None)
    return band.cpu().numpy()


@pytest.mark.parametrize("B", BANDS)
def test_band_host_and_device(B):
    b1, b2, cnt = _table()
    host, dev = (_band(b1, b2, cnt, _weights(), B, device) for device in (False, True))
    assert host.tobytes() == dev.tobytes()
    np.testing.assert_array_equal(host, column_band(_dense(), B))


@pytest.mark.parametrize("device", (False, True))
def test_empty_table(device):
    b1, b2, cnt = (a[:0] for a in _table())
    w = _weights()
    for B in BANDS:
        band = _band(b1, b2, cnt, w, B, device)
        assert band.shape == (2 * B + 1, N) and not band.any()
    bad = np.zeros(N, np.uint8)
    bad[list(BAD)] = 1
    valid = np.isfinite(w[LO:LO + N]).astype(np.uint8) & (1 - bad)
    _, n_want = ref.diamond_sums(np.zeros((N, N)), valid, WINDOWS, 1)
    if device:
        import torch
        b1, b2, cnt = (torch.from_numpy(np.array(a)).cuda() for a in (b1, b2, cnt))
    S, n = ins.diamond_sums_pixels(b1, b2, cnt, w, LO, N, WINDOWS, 1, bad)
    if device:
        assert S.is_cuda and n.is_cuda
        S, n = S.cpu().numpy(), n.cpu().numpy()
    assert not S.any()
    np.testing.assert_array_equal(n, n_want)
