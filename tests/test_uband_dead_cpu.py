"""The dead-rectangle test of the upper-band sweep, on the CPU:
the predicate the solver evaluates at create (tests/uband_dead_ref.py restates
it; tests/test_uband_skip_gpu.py compares the library's count with it) against
the positions themselves, and the share of the C4 geometry it removes."""
import numpy as np
import pytest

from hichap_master_amd import synth
from tests import uband_dead_ref as ref

# two uint8 chunks and three nibble chunks (the widths of the GPU test's genome)
W8, W4 = 1504, 3712


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _layouts():
    rng = np.random.default_rng(20)
    out = {
        "multiples_of_512": [5120, 3072, 640],
        # chromosomes shorter than 128 rows and than a chunk; blocks that straddle one and two boundaries
        "short": [50, 100, 700, 30, 1000, 90, 300, 20, 40, 2000],
        "two_boundaries_in_a_block": [1000, 30, 40, 1490],
        "last_partial_block": [1024, 512, 384 + 77],
        "single": [3000],
        "single_short": [100],
    }
    for k in range(4):  # random: lengths from below a 16-row group to several chunks
        out[f"random{k}"] = rng.choice([7, 15, 16, 17, 100, 127, 129, 600, 1009, 2500], rng.integers(2, 9)).tolist()
    return out


_LAYOUTS = _layouts()


def test_chunk_geometry():
    ch = ref.chunks(W8, W4)
    assert [b for b, _, _ in ch] == [8, 8, 4, 4, 4]
    assert [base for _, _, base in ch] == [0, 1008, W8 + 1, W8 + 1 + 1008, W8 + 1 + 2016]
    assert len(ref.chunks(2768, 9584)) == 3 + 7  # C4
    assert ref.chunks(992, 992) == [(8, 0, 0)] and len(ref.chunks(1008, 1008)) == 2  # W8 + 1 slots + 15 back


@pytest.mark.parametrize("name", list(_LAYOUTS))
def test_predicate_is_exact(name):
    """dead if and only if no position (r, r + d) the walk addresses is cis"""
    off = _offsets(_LAYOUTS[name])
    got, want = ref.dead(off, W8, W4), ref.dead_brute(off, W8, W4)
    assert got.shape == ((off[-1] + 127) // 128, 5)
    np.testing.assert_array_equal(got, want)
    assert not got[:, 0].any()  # diagonal 1 is cis for every row but a chromosome's last: chunk 0 lives
    if name == "multiples_of_512":
        assert got[64:69, 2:].all()  # the 640-row chromosome: every nibble rectangle (W8 + 1 > 640)
        assert got[:, 2:].sum() > got[:, :2].sum() > 0


@pytest.mark.parametrize("name", ["single", "single_short"])
def test_single_chromosome(name):
    """one chromosome: its end is the matrix's, so the only dead rectangles are
    those whose every addressed column lies past the last bin (no slot there
    can hold a pixel under any layout rule); everything else is walked"""
    off = _offsets(_LAYOUTS[name])
    n = int(off[-1])
    got = ref.dead(off, W8, W4)
    for b in range(got.shape[0]):
        rows = np.arange(b * 128, min(b * 128 + 128, n))
        for k, (_, kc, base) in enumerate(ref.chunks(W8, W4)):
            first = rows + base - ((rows & 15) if kc > 0 else 0)  # first column each row addresses
            assert got[b, k] == bool((first >= n).all())
    assert not got[:, 0].any()


def test_room_table():
    """room(r) = bins from r to the end of its chromosome (a function of the
    global row and the offsets only, so every shard marks the same tasks)"""
    off = _offsets(_LAYOUTS["short"])
    rm = ref.room(off)
    assert rm[0] == 50 and rm[49] == 1 and rm[50] == 100 and rm[-1] == 1
    whole = ref.dead(off, W8, W4)
    assert whole.any() and not whole.all()


def test_c4_dead_share():
    """the flagship geometry (hg19 10 kb diploid, W8 2 768, W4 9 584): the
    uint8 / nibble rectangles without a cis position, and the share of the
    slot work (VALU instructions: 4.5 / 4.1 per slot) they are.  The estimate
    this work started from was 6.2 % / 40.8 % / 30.2 %; the exact coverage of
    the chunks (a chunk's rows reach 15 slots back, the last chunk of a
    segment is walked in full) gives 6.9 % / 41.5 % / 30.4 %."""
    off = _offsets(synth.genome_bins(10000, diploid=True))
    assert off[-1] == 607282
    d8, d4, work = ref.dead_share(off, 2768, 9584)
    assert abs(d8 - 0.062) < 0.01 and abs(d4 - 0.408) < 0.01 and abs(work - 0.302) < 0.01, (d8, d4, work)
    assert abs(d8 - 0.0690) < 5e-4 and abs(d4 - 0.4150) < 5e-4 and abs(work - 0.3043) < 5e-4, (d8, d4, work)
