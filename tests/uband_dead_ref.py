"""The upper-band sweep's dead rectangles restated in NumPy
(test infrastructure).

A wave task is 128 globally aligned rows x one chunk of 1008 band slots.  The
uint8 segment holds diagonals 0..W8 (chunk kc starts at diagonal 1008 kc), the
nibble segment diagonals W8+1..W4 (chunk kc starts at W8 + 1 + 1008 kc); a
segment of S slots has ceil((S + 15) / 1008) chunks.  Row r of the task is
read shifted back by m = r mod 16 slots: in a chunk kc > 0 the walk addresses
its diagonals [base - m, base + 1008 - m), in chunk 0 (where the slots in
front lie outside the segment and read as 0) [base, base + 1008 - m).  With
cis-only bands a slot (r, r + d) can hold a count only if r + d is below the
end of r's chromosome, d < room(r), so the task is dead when

    kc > 0:  max over its rows r < n of room(r) + (r mod 16)  <=  base
    kc = 0:  max over its rows r < n of room(r)               <=  base
"""
import numpy as np

ROWS, CHUNK = 128, 1008
VALU8, VALU4 = 4.5, 4.1  # VALU instructions per slot of the two walks


def chunks(w8, w4):
    """[(bits, kc, base)] in chunk-index order: the uint8 segment's, then the
    nibble segment's"""
    out = []
    if w8 > 0:
        out += [(8, kc, CHUNK * kc) for kc in range((w8 + 1 + 15 + CHUNK - 1) // CHUNK)]
    if w4 > w8:
        out += [(4, kc, w8 + 1 + CHUNK * kc) for kc in range((w4 - w8 + 15 + CHUNK - 1) // CHUNK)]
    return out


def room(offsets):
    """room(r) = end of r's chromosome - r, for every bin"""
    off = np.asarray(offsets, dtype=np.int64)
    r = np.arange(off[-1], dtype=np.int64)
    return off[np.searchsorted(off, r, side="right")] - r


def dead(offsets, w8, w4):
    """bool [128-row blocks with a row below n, chunks]: the predicate"""
    rm = room(offsets)
    n = rm.size
    nblk = (n + ROWS - 1) // ROWS
    pad = np.full(nblk * ROWS, np.iinfo(np.int64).min // 2)
    pad[:n] = rm
    pad15 = pad.copy()
    pad15[:n] += np.arange(n) & 15
    top, top15 = pad.reshape(nblk, ROWS).max(1), pad15.reshape(nblk, ROWS).max(1)
    ch = chunks(w8, w4)
    out = np.zeros((nblk, len(ch)), dtype=bool)
    for k, (_, kc, base) in enumerate(ch):
        out[:, k] = (top15 if kc > 0 else top) <= base
    return out


def dead_brute(offsets, w8, w4):
    """the same table from the positions themselves: a task is dead if and
    only if no (r, r + d), d >= 1, that its walk addresses is cis"""
    off = np.asarray(offsets, dtype=np.int64)
    n = int(off[-1])
    chrom = np.searchsorted(off, np.arange(n), side="right") - 1
    nblk = (n + ROWS - 1) // ROWS
    ch = chunks(w8, w4)
    out = np.ones((nblk, len(ch)), dtype=bool)
    j = np.arange(-15, CHUNK)[None, :]
    for b in range(nblk):
        r = np.arange(b * ROWS, min((b + 1) * ROWS, n))[:, None]
        m = r & 15
        for k, (_, kc, base) in enumerate(ch):
            touched = (j >= (-m if kc > 0 else 0)) & (j < CHUNK - m)
            d = base + j
            c = r + d
            ok = touched & (d >= 1) & (c < n)
            cis = ok & (chrom[np.minimum(c, n - 1)] == chrom[r])
            out[b, k] = not cis.any()
    return out


def dead_share(offsets, w8, w4):
    """(share of the uint8 tasks, of the nibble tasks, of the slot work
    weighted by the walks' VALU instructions per slot) that is dead"""
    t = dead(offsets, w8, w4)
    bits = np.array([b for b, _, _ in chunks(w8, w4)])
    wt = np.where(bits == 8, VALU8, VALU4)
    return (float(t[:, bits == 8].mean()), float(t[:, bits == 4].mean()),
            float((t * wt).sum() / (wt.sum() * t.shape[0])))
