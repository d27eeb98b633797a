"""The flat sweep's run schedule (ice.hip k_sweep_flatw, hh_tune "flatw_pipe"),
restated in NumPy.

A wave walks a segment of qb uint4 in steps of 64 * U uint4; in step q0 lane l
holds the run [q0 + U l, q0 + U l + U), zeros past qb.  flatw_pipe 2 loads a
run masked (flat_load / flat_load_ilv: the select sits at the load);
flatw_pipe 3 issues the same loads raw (flat_issue / flat_issue_ilv) and
applies the mask where the run is first walked (flat_apply / flat_apply_ilv),
from the consuming step's (q0, qb).  Here, for every (qb, q0) of a range that
covers the shapes of tests/test_flat_prefetch_gpu.py:

  * the mask applied at the consuming step is the mask applied at the load;
  * every address issued lies in [0, qb), and both schedules issue the same
    multiset of addresses, in the same order;
  * flat_ilv_pos maps a chunk's logical uint4 one to one onto its stored
    positions, and the interleaved loads read exactly the registers the
    lane-major loads read.
"""
import numpy as np
import pytest

U = 8    # kFlatU = kFlatIlvU: uint4 per lane and step, narrow segments (interleaved)
UW = 2   # wide segments (lane-major)
LANES = np.arange(64)


def ilv_cnt(m, k):
    """flat_ilv_cnt: lanes that hold element k of their run in a chunk of m uint4"""
    return (m - k + U - 1) // U if m > k else 0


def ilv_pos(m, i):
    """flat_ilv_pos: chunk-relative stored position of chunk-relative logical uint4 i"""
    k = i % U
    return sum(ilv_cnt(m, j) for j in range(k)) + i // U


def issue_ilv(q0, qb):
    """flat_issue_ilv / flat_load_ilv: addresses (U, 64) of the chunk at q0, in instruction order"""
    m = min(qb - q0, 64 * U)
    addr = np.empty((U, 64), np.int64)
    base = q0
    for k in range(U):
        cnt = ilv_cnt(m, k)
        addr[k] = np.where(LANES < cnt, base + LANES, q0)
        base += cnt
    return addr


def mask_ilv(q0, qb):
    m = min(qb - q0, 64 * U)
    return np.array([LANES < ilv_cnt(m, k) for k in range(U)])


def issue_plain(q0, qb, u, qa=0):
    """flat_issue / flat_load: lane-major addresses (u, 64) of the step at q0"""
    s = q0 + LANES * u
    return np.array([np.where(s + k < qb, s + k, qa) for k in range(u)])


def mask_plain(q0, qb, u):
    s = q0 + LANES * u
    return np.array([s + k < qb for k in range(u)])


def schedule(qb, u, ilv, raw):
    """Program order of one segment as (event, q0) pairs.  Both forms issue the
    first run before the segment (the tile's prologue, or the previous tile's
    end) and the next run before the current step's walk; the masked form
    ("load") masks at the issue, the raw form at "apply", after the walk."""
    ev = [("issue", 0)]
    if raw:
        ev.append(("apply", 0))
    q0 = 0
    while True:
        qn = q0 + 64 * u
        if qn < qb:
            ev.append(("issue", qn))
        ev.append(("walk", q0))
        if qn >= qb:
            break
        if raw:
            ev.append(("apply", qn))
        q0 = qn
    return ev


def run_schedule(qb, u, ilv, raw, mem):
    """Executes a schedule on a payload `mem` (stored order); returns the runs
    the walks saw, (steps, u, 64), and the addresses issued in order."""
    issue = (lambda q0: issue_ilv(q0, qb)) if ilv else (lambda q0: issue_plain(q0, qb, u))
    mask = (lambda q0: mask_ilv(q0, qb)) if ilv else (lambda q0: mask_plain(q0, qb, u))
    r = v = None
    seen, addrs = [], []
    for what, q0 in schedule(qb, u, ilv, raw):
        if what == "issue":
            a = issue(q0)
            assert a.min() >= 0 and a.max() < qb, (qb, q0)
            addrs.append(a)
            r = mem[a]
            if not raw:
                pending = np.where(mask(q0), r, 0)
                if v is None:
                    v = pending
        elif what == "apply":
            v = np.where(mask(q0), r, 0)  # the first use of r: after the previous walk
        else:
            seen.append(v.copy())
            if not raw and q0 + 64 * u < qb:
                v = pending  # v = vn
    return np.array(seen), np.concatenate([a.ravel() for a in addrs])


NARROW = sorted(set(list(range(1, 40)) + [63, 64, 65, 127, 128, 129]
                    + list(range(505, 530)) + [1023, 1024, 1025, 1031, 1032, 1033, 1535, 1536, 1537, 2049, 2600]))
WIDE = sorted(set(list(range(1, 12)) + [63, 64, 65] + list(range(125, 132)) + list(range(253, 260)) + [383, 384, 385, 700]))


@pytest.mark.parametrize("qb", NARROW)
def test_interleaved_segment(qb):
    # the stored (interleaved) payload of a segment whose logical uint4 i holds i + 1
    mem = np.zeros(qb, np.int64)
    for c0 in range(0, qb, 64 * U):
        m = min(qb - c0, 64 * U)
        pos = np.array([ilv_pos(m, i) for i in range(m)])
        assert sorted(pos) == list(range(m))  # one to one onto the chunk
        mem[c0 + pos] = c0 + np.arange(m) + 1
    old, a_old = run_schedule(qb, U, True, False, mem)
    new, a_new = run_schedule(qb, U, True, True, mem)
    np.testing.assert_array_equal(a_new, a_old)  # the same addresses in the same order
    np.testing.assert_array_equal(new, old)
    # and they are the lane-major runs: lane l, element k of step q0 = logical q0 + U l + k
    for st, q0 in enumerate(range(0, qb, 64 * U)):
        s = q0 + LANES[None, :] * U + np.arange(U)[:, None]
        np.testing.assert_array_equal(new[st], np.where(s < qb, s + 1, 0))
        # the mask of the consuming step is the mask of the load
        np.testing.assert_array_equal(mask_ilv(q0, qb), s < qb)
    # every stored uint4 is read exactly once by an unmasked lane
    on = np.concatenate([mask_ilv(q0, qb).ravel() for q0 in range(0, qb, 64 * U)])
    assert sorted(a_new[on]) == list(range(qb))


@pytest.mark.parametrize("qb", WIDE)
def test_plain_segment(qb):
    mem = np.arange(qb, dtype=np.int64) + 1
    old, a_old = run_schedule(qb, UW, False, False, mem)
    new, a_new = run_schedule(qb, UW, False, True, mem)
    np.testing.assert_array_equal(a_new, a_old)
    np.testing.assert_array_equal(new, old)
    for st, q0 in enumerate(range(0, qb, 64 * UW)):
        s = q0 + LANES[None, :] * UW + np.arange(UW)[:, None]
        np.testing.assert_array_equal(new[st], np.where(s < qb, s + 1, 0))
    on = np.concatenate([mask_plain(q0, qb, UW).ravel() for q0 in range(0, qb, 64 * UW)])
    assert sorted(a_new[on]) == list(range(qb))


def test_schedule_order():
    """raw form: issue(next) -> walk(current) -> apply(next); no walk between
    an apply and the issue it masks other than the current step's"""
    ev = schedule(3 * 64 * U + 5, U, True, True)
    assert ev == [("issue", 0), ("apply", 0),
                  ("issue", 512), ("walk", 0), ("apply", 512),
                  ("issue", 1024), ("walk", 512), ("apply", 1024),
                  ("issue", 1536), ("walk", 1024), ("apply", 1536),
                  ("walk", 1536)]
    assert schedule(64 * U, U, True, True) == [("issue", 0), ("apply", 0), ("walk", 0)]
