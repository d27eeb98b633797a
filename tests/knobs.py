"""Tuning knobs for tests: the one place under tests/ that calls hh_tune.

``tuned(key=value, ...)`` sets the knobs for the length of a ``with`` block
and puts back the values it read on entry -- not the table defaults: a knob
set for the whole session (HH_PCA_P / HH_PCA_METHOD, HH_TUNE) survives.
"""
import contextlib
import ctypes


def get(key):
    from hichap_master_amd._lib import call
    v = ctypes.c_int64()
    call("hh_tune_get", key.encode(), ctypes.byref(v))
    return v.value


@contextlib.contextmanager
def tuned(**kv):
    from hichap_master_amd._lib import call
    old = [(k, get(k)) for k in kv]  # every key read before the first is set: an unknown key changes nothing
    try:
        for k, v in kv.items():
            call("hh_tune", k.encode(), int(v))
        yield
    finally:
        for k, v in reversed(old):
            call("hh_tune", k.encode(), v)
