"""hh_tune / hh_tune_get (hichap_master_amd/csrc/tune.hip) without a device:
every key's documented default, a set / get round trip of a legal value, the
rejection of an illegal one and of every retired key with the key named in the
error, and tests.knobs.tuned() putting back what it read when its block is
left through an exception.  "sweep_trace" allocates device memory and is left
alone; nothing else here touches a device."""
import os

import pytest

from hichap_master_amd import _lib
from tests import knobs

pytestmark = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason="libhichap_hip.so is not built")

# key: (default, a legal value that is not the default, an illegal value)
KEYS = {
    "band_w": (-1, 48, 40),
    "band4": (1, 0, 2),
    "band_cis": (1, 0, -1),
    "flat_max": (64, 255, 256),
    "flat_cols": (-1, 1, 2),
    "flat_group": (0, 33, 257),
    "unit_entries": (0, 4096, 4095),
    "upper_tiles": (-1, 0, 2),
    "host_build": (0, 1, 2),
    "build_debug": (0, 1, -1),
    "flatw_pipe": (3, 2, 1),
    "flatw_waves": (11, 10, 9),
    "flatw_waves_up": (8, 11, 10),
    "flat_defer": (1, 0, 2),
    "tiled_pf": (1, 2, 3),
    "band_rows": (0, 128, 32),
    "band_fused": (1, 0, 2),
    "band_concurrent": (1, 0, 2),
    "split_tiles": (1, 0, 2),
    "conc_order": (1, 2, 3),
    "conc_min_bytes": (8 << 30, 0, -1),
    "uband": (1, 2, 3),
    "ub_skip": (1, 0, 2),
    "ub_xcd": (1, 0, 2),
    "ub_fast": (1, 0, 2),
    "sweep_single": (-1, 1, 2),
    "iter_events": (1, 0, 2),
    "fuse_stats": (-1, 2, 3),
    "pca_method": (1, 0, 2),
    "pca_p": (8, 2, 9),
    "pca_coop": (1, 0, 2),
    "pca_debug": (0, 2, -1),
    "syrk_split": (-1, 64, 65),
    "cor_sym": (3, 0, 4),
    "ortho_tpb": (0, 8, 3),
    "ortho_min_tpb": (2, 1, 3),
    "ortho_lowsync": (1, 0, 2),
    "ortho_grid_cap": (0, 64, 65),
    "ortho_abort_test": (0, 2, 3),
    "symvc_rows": (32, 1024, 40),
    "symvc_out": (1, 0, 2),
    "symvc_stream": (1, 0, 2),
    "twostep_devglue": (1, 0, 2),
    "twostep_budget_mb": (0, 40, -1),
    "parse_ablate": (0, 3, 4),
    "rank_lds_buckets": (8192, 0, 8193),
    "coarsen_tile": (8192, 64, 63),
    "saddle_diag_tile": (256, 64, 257),
    "pileup_chunk": (64, 1, 0),
}
# keys a whole test session may have set from the environment (tests/conftest.py, HH_TUNE)
SESSION = {k for k in ("pca_p", "pca_method") if os.environ.get("HH_" + k.upper())} | {
    kv.split("=")[0].strip() for kv in filter(None, os.environ.get("HH_TUNE", "").split(","))}
HH_ERR_ARG = -1  # include/hichap_hip.h
RETIRED = ["sweep_ablate", "sweep_nb", "band_dpp", "flatw_u", "band4_density_pct", "band8_big_pct", "unit_lpt",
           "unit_lpt_lists", "tile_cost", "band_lpt", "uband_min_bytes", "conc_ub_min_bytes", "single_max_bytes"]


def _rejected(key, value):
    with pytest.raises(_lib.HipLibraryError) as e:
        _lib.call("hh_tune", key.encode(), value)
    assert e.value.code == HH_ERR_ARG and key in str(e.value), e.value


@pytest.mark.parametrize("key", sorted(KEYS))
def test_default_roundtrip_and_rejection(key):
    default, legal, illegal = KEYS[key]
    if key not in SESSION:
        assert knobs.get(key) == default
    before = knobs.get(key)
    with knobs.tuned(**{key: legal}):
        assert knobs.get(key) == legal
        _rejected(key, illegal)
        assert knobs.get(key) == legal  # a rejected value changes nothing
    assert knobs.get(key) == before


@pytest.mark.parametrize("key", RETIRED)
def test_retired_keys_are_unknown(key):
    _rejected(key, 1)
    with pytest.raises(_lib.HipLibraryError, match=key):
        knobs.get(key)


@pytest.mark.skipif(os.path.basename(_lib.LIB_PATH) != "libhichap_hip.so", reason="about the default build")
def test_upper_tiles_needs_its_build():
    """(the default library has 8192-column tiles: no upper-triangle tiles to switch on)"""
    _rejected("upper_tiles", 1)
    assert knobs.get("upper_tiles") == -1


def test_tuned_restores_after_an_exception():
    before = (knobs.get("flatw_pipe"), knobs.get("band_w"))
    with knobs.tuned(flatw_pipe=2, band_w=64):  # the state a block inherits is not the default
        with pytest.raises(ZeroDivisionError):
            with knobs.tuned(flatw_pipe=0, band_w=-1, uband=2):
                assert (knobs.get("flatw_pipe"), knobs.get("band_w"), knobs.get("uband")) == (0, -1, 2)
                1 / 0
        assert (knobs.get("flatw_pipe"), knobs.get("band_w"), knobs.get("uband")) == (2, 64, 1)
        # an illegal value among the settings: the ones already made are undone as well
        with pytest.raises(_lib.HipLibraryError, match="flatw_pipe"):
            with knobs.tuned(band_w=0, flatw_pipe=1):
                pass
        assert (knobs.get("flatw_pipe"), knobs.get("band_w")) == (2, 64)
    assert (knobs.get("flatw_pipe"), knobs.get("band_w")) == before
