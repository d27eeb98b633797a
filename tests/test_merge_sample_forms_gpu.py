"""The corners of hh_merge_* / hh_sample_* that ``merge_pixels`` and
``downsample_pixels`` do not reach from their usual inputs: the ``on_device =
0`` form of the device entry points (int32 host arrays, uploaded by the
library; results in device arrays), and tables of no pixels through the sample
passes.  Every comparison is exact, against tests/merge_ref.py and
tests/sample_ref.py."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from hichap_master_amd._lib import call, ptr
from hichap_master_amd.merge import merge_pixels
from hichap_master_amd.sample import downsample_pixels, sample_threshold
from tests.merge_ref import merge_ref
from tests.sample_ref import sample_ref, table107

pytestmark = pytest.mark.gpu


def _pointers(arrays):
    return (C.c_void_p * len(arrays))(*[ptr(a).value if a.size else None for a in arrays])


def _outputs(n, wide):
    import torch
    return (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"),
            torch.empty(n, dtype=torch.int64 if wide else torch.int32, device="cuda"))


def test_merge_count_takes_int32_host_arrays():
    b1, b2, c, off = table107()
    n_bins = int(off[-1])
    halves = [(b1[::2], b2[::2], c[::2]), (b1[1::3], b2[1::3], c[1::3]), (b1[:0], b2[:0], c[:0])]
    want = merge_ref(halves, n_bins)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    t1, t2 = [i32(t[0]) for t in halves], [i32(t[1]) for t in halves]
    tc = [i32(halves[0][2]), np.ascontiguousarray(halves[1][2], dtype=np.int64), i32(halves[2][2])]
    c64 = np.array([0, 1, 0], np.int32)
    nnz = np.array([a.size for a in t1], np.int64)
    h, n, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0)
    call("hh_merge_count", _pointers(t1), _pointers(t2), _pointers(tc), ptr(c64), ptr(nnz), 3, n_bins, 0, None,
         C.byref(h), C.byref(n), C.byref(mx))
    try:
        assert n.value == want[0].size and mx.value == int(want[2].max())
        o1, o2, oc = _outputs(n.value, False)
        call("hh_merge_write", h, ptr(o1), ptr(o2), ptr(oc), 0, None)
    finally:
        call("hh_merge_free", h)
    for g, w in zip((o1, o2, oc), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)
    for g, w in zip(merge_pixels(halves, n_bins), want):            # the host form agrees
        np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("wide", (False, True))
def test_sample_count_takes_int32_host_arrays(wide):
    b1, b2, c, _ = table107()
    thr = sample_threshold(frac=Fraction(37, 100))
    want = sample_ref(b1, b2, c, thr, 1)
    a1, a2 = (np.ascontiguousarray(a, dtype=np.int32) for a in (b1, b2))
    ac = np.ascontiguousarray(c, dtype=np.int64 if wide else np.int32)
    h, n, tot, mx = C.c_void_p(), C.c_int64(0), C.c_int64(0), C.c_int64(0)
    call("hh_sample_count", ptr(a1), ptr(a2), ptr(ac), int(wide), a1.size, thr, 1, 0, None, C.byref(h), C.byref(n),
         C.byref(tot), C.byref(mx))
    try:
        assert n.value == want[0].size and tot.value == int(want[2].sum()) and mx.value == int(want[2].max())
        o1, o2, oc = _outputs(n.value, False)
        call("hh_sample_write", h, ptr(o1), ptr(o2), ptr(oc), 0, None)
    finally:
        call("hh_sample_free", h)
    for g, w in zip((o1, o2, oc), want):
        np.testing.assert_array_equal(g.cpu().numpy(), w)


def test_sample_of_no_pixels():
    import torch
    e = np.zeros(0, np.int64)
    for out in (downsample_pixels(e, e, e, frac=0.5, seed=2), downsample_pixels(e, e, e, count_target=0)):
        assert [x.size for x in out] == [0, 0, 0]
        assert out[0].dtype == np.int64 and out[2].dtype == np.int32
    z = torch.zeros(0, dtype=torch.int32, device="cuda")
    for cnt in (z, z.to(torch.int64)):
        d = downsample_pixels(z, z, cnt, frac=0.5)
        assert [x.numel() for x in d] == [0, 0, 0] and all(x.is_cuda and x.dtype == torch.int32 for x in d)
    # the entry point itself: NULL arrays with nnz = 0, both forms
    h, n, tot, mx = C.c_void_p(), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)
    call("hh_sample_count", None, None, None, 0, 0, 1 << 63, 0, 1, None, C.byref(h), C.byref(n), C.byref(tot),
         C.byref(mx))
    try:
        assert (n.value, tot.value, mx.value) == (0, 0, 0)
        call("hh_sample_write", h, None, None, None, 0, None)
    finally:
        call("hh_sample_free", h)
    h = C.c_void_p()
    call("hh_sample_count_host", None, None, None, 0, 1 << 63, 0, None, C.byref(h), C.byref(n), C.byref(tot),
         C.byref(mx))
    try:
        assert (n.value, tot.value, mx.value) == (0, 0, 0)
        call("hh_sample_write_host", h, None, None, None, 0, None)
    finally:
        call("hh_sample_free", h)
