"""hh_tune "sweep_sched" (hichap_master_amd/csrc/tune.hip) without a device:
the schedule knob's default, a set / get round trip of the phased schedule and
the rejection of the values on either side of its range with the key named in
the error.  (tests/test_tune_cpu.py pins the older keys in the same way.)"""
import os

import pytest

from hichap_master_amd import _lib
from tests import knobs

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libhichap_hip.so is not built")

KEY = "sweep_sched"
SESSION = {kv.split("=")[0].strip() for kv in filter(None, os.environ.get("HH_TUNE", "").split(","))}
HH_ERR_ARG = -1  # include/hichap_hip.h


def _rejected(value):
    with pytest.raises(_lib.HipLibraryError) as e:
        _lib.call("hh_tune", KEY.encode(), value)
    assert e.value.code == HH_ERR_ARG and KEY in str(e.value), e.value


def test_default_is_auto():
    if KEY not in SESSION:
        assert knobs.get(KEY) == -1


@pytest.mark.parametrize("legal", [0, 1, 2, -1])
def test_roundtrip_and_rejection(legal):
    before = knobs.get(KEY)
    with knobs.tuned(**{KEY: legal}):
        assert knobs.get(KEY) == legal
        for illegal in (3, -2):
            _rejected(illegal)
            assert knobs.get(KEY) == legal  # a rejected value changes nothing
    assert knobs.get(KEY) == before
