"""CPU restatement of the tiled sweep's pipelined step sequence
(hichap_master_amd/csrc/ice.hip: RowsPf, hh_tune "tiled_pf"): which uint4 of
which row a wave requests at each step -- the loads of the wave's next step
issued before the current step's data are used, across batch boundaries too
-- and which it uses, with the clamp of finished lanes to slot 0.  Checked
against the plain loops it replaces (tile_rows / band_rows: per batch of NB
rows per lane group, step by step) on random ragged segments (empty rows,
one-row bands, lengths around every lane-group width), so the schedule is
pinned independently of the GPU."""
import numpy as np
import pytest

NW = 8    # waves per block (kSweepWaves)
NB = 2    # rows per lane group at a time
OFF = -1  # a lane past its row's end: reads slot 0, uses zeros

# uint4 per row: around every lane-group width G = 4..64 and its multiples
LENS = [0, 1, 5, 6, 7, 11, 12, 13, 23, 24, 25, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193]


class Guarded:
    """an LDS array of which only [0, n) may be read"""

    def __init__(self, a, n):
        self.a, self.n = np.asarray(a), n

    def __getitem__(self, i):
        assert 0 <= i < self.n, f"read at {i}, valid [0, {self.n})"
        return int(self.a[i])


def row_of(perm, v):
    return v if perm is None else perm[v]


def bounds(rp4, perm, w, hi, G, S, gi, li):
    """q / qe of the batch at slot w for one lane (zeros for slots at or past hi)"""
    q, qe = [0] * NB, [0] * NB
    for k in range(NB):
        v = w + k * S + gi
        if v < hi:
            r = row_of(perm, v)
            q[k] = rp4[r] + li
            qe[k] = rp4[r + 1]
    return q, qe


def today(rp4, perm, lo, hi, G, wave):
    """tile_rows / band_rows: the (row slot, uint4) pairs one wave uses, step
    by step; a step = a list over k of 64 lane entries (slot v, q) or OFF"""
    RP = 64 // G
    S = NW * RP
    steps = []
    for v0 in range(lo + wave * RP, hi, NB * S):
        lanes = [bounds(rp4, perm, v0, hi, G, S, lane // G, lane % G) for lane in range(64)]
        while any(q[k] < qe[k] for q, qe in lanes for k in range(NB)):
            step = []
            for k in range(NB):
                row = []
                for lane, (q, qe) in enumerate(lanes):
                    row.append((v0 + k * S + lane // G, q[k]) if q[k] < qe[k] else OFF)
                    q[k] += G
                step.append(row)
            steps.append(step)
    return steps


def pipelined(rp4, perm, lo, hi, G, wave):
    """RowsPf::run / step for one wave.  Returns (requests, uses): requests[i]
    = per k the 64 slots asked for by the i-th issue (index into the segment,
    0 for a clamped lane) with the (row slot, q) it stands for or OFF; uses[i]
    = what step i consumes, in the form of today()."""
    RP = 64 // G
    S = NW * RP
    v0 = lo + wave * RP
    if v0 >= hi:
        return [], []
    gl = [(lane // G, lane % G) for lane in range(64)]
    cur = [bounds(rp4, perm, v0, hi, G, S, gi, li) for gi, li in gl]
    nxt = [bounds(rp4, perm, v0 + NB * S, hi, G, S, gi, li) for gi, li in gl]
    slot0 = v0  # the batch the lanes' q / qe belong to

    def issue():
        req = []
        for k in range(NB):
            row = []
            for lane, (q, qe) in enumerate(cur):
                on = q[k] < qe[k]
                row.append((q[k] if on else 0, (slot0 + k * S + lane // G, q[k]) if on else OFF))
            req.append(row)
        return req

    requests, uses = [issue()], []
    while True:
        use = []
        for k in range(NB):
            use.append([(v0 + k * S + lane // G, q[k]) if q[k] < qe[k] else OFF for lane, (q, qe) in enumerate(cur)])
        more = False
        for q, qe in cur:
            for k in range(NB):
                q[k] += G
                more |= q[k] < qe[k]
        nxt_batch = v0 + NB * S < hi
        if not more:
            cur = nxt
            slot0 = v0 + NB * S
        requests.append(issue())  # 1. the next step's loads ...
        uses.append(use)          # 2. ... before this step's data are used
        if not more:              # 3. the batch ends
            nxt = [bounds(rp4, perm, v0 + 2 * NB * S, hi, G, S, gi, li) if nxt_batch else ([0] * NB, [0] * NB)
                   for gi, li in gl]
            v0 += NB * S
        if not (more or nxt_batch):
            return requests, uses


def make_segment(rng, nrows, lens):
    """row pointers in uint4 for `nrows` rows with the given lengths"""
    rp4 = np.zeros(nrows + 1, np.int64)
    rp4[1:] = np.cumsum(lens)
    return rp4


def check(rp4, perm, lo, hi, G):
    nrows = len(rp4) - 1
    seen = np.zeros(int(rp4[-1]), np.int64)
    g_rp = Guarded(rp4, nrows + 1)
    g_perm = None if perm is None else Guarded(perm, hi)  # nothing at or past hi
    for wave in range(NW):
        want = today(rp4, perm, lo, hi, G, wave)
        requests, uses = pipelined(g_rp, g_perm, lo, hi, G, wave)
        # empty batches take one step of finished lanes in the pipelined loop, none today
        got = [u for u in uses if any(e != OFF for row in u for e in row)]
        assert got == want, (G, wave)
        # each step uses exactly what was requested one issue earlier; the last issue is all clamped
        assert len(requests) == len(uses) + (1 if uses else 0)
        for req, use in zip(requests, uses):
            assert [[e for _, e in row] for row in req] == use
        if requests:
            assert all(idx == 0 and e == OFF for row in requests[-1] for idx, e in row)
        for req in requests:
            for row in req:
                for idx, e in row:
                    if e == OFF:
                        assert idx == 0
                        continue
                    v, q = e
                    assert lo <= v < hi and idx == q
                    r = row_of(perm, v)
                    assert rp4[r] <= q < rp4[r + 1], "request outside its row's segment"
        for use in uses:
            for row in use:
                for e in row:
                    if e != OFF:
                        seen[e[1]] += 1
    rows = [row_of(perm, v) for v in range(lo, hi)]
    expect = np.zeros_like(seen)
    for r in rows:
        expect[rp4[r]:rp4[r + 1]] += 1
    np.testing.assert_array_equal(seen, expect)  # every uint4 of every row of [lo, hi) exactly once


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_row_ranges(G):
    """tile_rows: rows [ra, rb) of the tile in index order, units starting and
    ending mid-block"""
    rng = np.random.default_rng(100 + G)
    lens = rng.choice(LENS, 512)
    lens[rng.random(512) < 0.1] = 0
    rp4 = make_segment(rng, 512, lens)
    RPB = (64 // G) * NB * NW  # rows per block step
    for lo, hi in [(0, 512), (0, 1), (7, 8), (3, 3 + RPB), (5, 5 + RPB + 1), (100, 100 + 2 * RPB - 1), (37, 300),
                   (511, 512), (512 - RPB // 2, 512)]:
        check(rp4, None, lo, min(hi, 512), G)


@pytest.mark.parametrize("G", [4, 8, 16, 32, 64])
def test_bands(G):
    """band_rows: rows perm[lo..hi) of the tile's length order"""
    rng = np.random.default_rng(200 + G)
    lens = rng.choice(LENS, 512)
    lens[:40] = 0
    rp4 = make_segment(rng, 512, lens)
    perm = np.argsort(-lens, kind="stable").astype(np.uint16)
    RPB = (64 // G) * NB * NW
    cuts = sorted(c for c in {0, 1, 2, RPB - 1, RPB, RPB + 1, 3 * RPB + 5, 300, 470, 511, 512} if c <= 512)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        check(rp4, perm, lo, hi, G)
    check(rp4, perm, 0, 512, G)
    check(rp4, perm, 480, 512, G)  # empty rows only


def test_all_empty_and_single():
    rp4 = make_segment(None, 512, np.zeros(512, np.int64))
    check(rp4, None, 0, 512, 16)
    one = np.zeros(512, np.int64)
    one[200] = 193
    rp4 = make_segment(None, 512, one)
    for G in (4, 64):
        check(rp4, None, 0, 512, G)
        check(rp4, None, 200, 201, G)
