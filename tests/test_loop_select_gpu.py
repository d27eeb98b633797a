"""Loop selection on the GPU: ``hh_diag_rank_pixels`` (csrc/select.hip) against
``bisect_left`` on the dense matrix with exact equality, its LDS / global
bucket paths, error returns and device-pointer form; ``run_Loops`` end to end
on a cooler; the reference's golden fixture through ``StructureFind``."""
import bisect
import functools

import numpy as np
import pytest

from hichap_master_amd import coolio, loops
from hichap_master_amd._lib import HipLibraryError, call
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

LO = 11  # the chromosome starts at global bin 11: bins before it belong to another one



@functools.lru_cache(maxsize=None)
def _case(N):
    """(pixel table, queries, dense value, dense less) of one chromosome."""
    rng = np.random.default_rng(100 + N)
    dens = 0.5 if N <= 130 else 0.03
    H = np.triu(rng.integers(1, 60, (N, N)) * (rng.random((N, N)) < dens))
    if N > 8:
        H[np.arange(N - 5), np.arange(5, N)] = 7          # diagonal 5: every entry ties
        H[np.arange(N - 3), np.arange(3, N)] = 1 + np.arange(N - 3) % 50   # diagonal 3: many thresholds
        H[2, 6] = 0                                      # an absent pixel
    H = H + np.triu(H, 1).T
    r, c = np.nonzero(np.triu(H))
    b1, b2, cnt = r + LO, c + LO, H[r, c].astype(np.int64)
    # pixels of the chromosome before, of the one after, and trans pixels on both sides
    f1 = np.array([0, 3, LO + N, 2, LO, LO + N - 1])
    f2 = np.array([5, 3, LO + N + 4, LO, LO + N, LO + N + 2])
    b1, b2, cnt = np.concatenate([b1, f1]), np.concatenate([b2, f2]), np.concatenate([cnt, np.full(6, 40)])
    p = rng.permutation(b1.size)
    b1, b2, cnt = b1[p], b2[p], cnt[p]
    if N <= 130:
        rows, cols = np.triu_indices(N)                  # every pixel: all diagonals, stored or not
    else:
        rows = rng.integers(0, N, 3000)
        cols = rng.integers(0, N, 3000)
        rows, cols = np.minimum(rows, cols), np.maximum(rows, cols)
        d3 = np.arange(N - 3)
        rows = np.concatenate([rows, [0, 0, N - 1, 2], d3, np.arange(N - 5)])
        cols = np.concatenate([cols, [0, N - 1, N - 1, 6], d3 + 3, np.arange(N - 5) + 5])
    rows, cols = np.concatenate([rows, rows[:7]]), np.concatenate([cols, cols[:7]])   # repeats
    p = rng.permutation(rows.size)                       # unsorted
    rows, cols = rows[p], cols[p]
    diags = {}
    value = H[rows, cols].astype(np.int64)
    less = np.empty(rows.size, np.int64)
    for k, (a, b) in enumerate(zip(rows, cols)):
        if b - a not in diags:
            diags[b - a] = sorted(H.diagonal(b - a))
        less[k] = bisect.bisect_left(diags[b - a], H[a, b])
    for a in (b1, b2, cnt, rows, cols, value, less):
        a.setflags(write=False)
    return (b1, b2, cnt), (rows, cols), value, less, H


@pytest.mark.parametrize("N", [1, 2, 37, 130, 1000])
def test_diag_rank_equals_dense_bisect(N):
    (b1, b2, cnt), (rows, cols), value, less, H = _case(N)
    v, l = loops.diag_rank(b1, b2, cnt, LO, N, rows, cols)
    assert v.dtype == np.int64 and l.dtype == np.int64
    np.testing.assert_array_equal(v, value)
    np.testing.assert_array_equal(l, less)
    assert np.all(l[v == 0] == 0)
    if N > 8:
        absent = (rows == 2) & (cols == 6)
        assert absent.any() and np.all(v[absent] == 0) and np.all(l[absent] == 0)
        tie = (cols - rows == 5)
        assert np.all(v[tie] == 7) and np.all(l[tie] == 0)     # nothing on the diagonal is smaller
        assert ((rows == 0) & (cols == N - 1)).any() and (rows == cols).any()
    # two runs: bitwise equal
    v2, l2 = loops.diag_rank(b1, b2, cnt, LO, N, rows, cols)
    assert v.tobytes() == v2.tobytes() and l.tobytes() == l2.tobytes()


def test_diag_rank_empty_inputs():
    e = np.empty(0, np.int64)
    v, l = loops.diag_rank(e, e, e, 0, 12, [0, 3, 11], [0, 7, 11])
    assert v.tolist() == [0, 0, 0] and l.tolist() == [0, 0, 0]
    (b1, b2, cnt), _, _, _, _ = _case(37)
    v, l = loops.diag_rank(b1, b2, cnt, LO, 37, [], [])
    assert v.size == 0 and l.size == 0
    v, l = loops.diag_rank(e, e, e, 0, 1, [], [])
    assert v.size == 0 and l.size == 0


def test_diag_rank_bucket_switch():
    """Diagonal 3 of the N = 130 case carries 50 thresholds: with 16 LDS
    buckets it counts in global memory while the short diagonals stay in
    LDS; with 0 every diagonal does.  Same input, identical output."""
    N = 130
    (b1, b2, cnt), (rows, cols), value, less, H = _case(N)
    assert np.unique(H.diagonal(3)).size + 1 > 16            # diagonal 3 cannot fit
    assert any(np.unique(H.diagonal(d)[H.diagonal(d) > 0]).size + 1 <= 16 for d in range(100, N))  # some do
    out = {}
    for knob in (8192, 16, 0):
        with tuned(rank_lds_buckets=knob):
            out[knob] = loops.diag_rank(b1, b2, cnt, LO, N, rows, cols)
    for knob in (8192, 16, 0):
        np.testing.assert_array_equal(out[knob][0], value)
        np.testing.assert_array_equal(out[knob][1], less)
    # one diagonal only, more thresholds than the lowered budget
    on3 = cols - rows == 3
    with tuned(rank_lds_buckets=16):
        v, l = loops.diag_rank(b1, b2, cnt, LO, N, rows[on3], cols[on3])
    np.testing.assert_array_equal(v, value[on3])
    np.testing.assert_array_equal(l, less[on3])


def test_diag_rank_errors():
    (b1, b2, cnt), (rows, cols), _, _, _ = _case(37)
    bad = cnt.copy()
    inside = np.nonzero((b1 >= LO) & (b2 < LO + 37))[0][0]
    bad[inside] = -1
    with pytest.raises(HipLibraryError, match="negative count"):
        loops.diag_rank(b1, b2, bad, LO, 37, rows, cols)
    with pytest.raises(HipLibraryError, match="query"):
        loops.diag_rank(b1, b2, cnt, LO, 37, [0, 1], [5, 37])        # qcol >= N
    with pytest.raises(HipLibraryError, match="query"):
        loops.diag_rank(b1, b2, cnt, LO, 37, [0, 6], [5, 5])         # qrow > qcol
    with pytest.raises(HipLibraryError, match="query"):
        loops.diag_rank(b1, b2, cnt, LO, 37, [-1], [5])
    with pytest.raises(HipLibraryError, match="bin1 > bin2"):
        loops.diag_rank(b2, b1, cnt, LO, 37, rows, cols)
    # the library is still usable
    v, _ = loops.diag_rank(b1, b2, cnt, LO, 37, rows, cols)
    np.testing.assert_array_equal(v, _case(37)[2])


def test_diag_rank_device_pointers():
    import torch
    (b1, b2, cnt), (rows, cols), value, less, _ = _case(130)
    d1, d2, dc = (torch.from_numpy(np.array(a)).cuda() for a in (b1, b2, cnt))
    v, l = loops.diag_rank(d1, d2, dc, LO, 130, rows, cols)
    hv, hl = loops.diag_rank(b1, b2, cnt, LO, 130, rows, cols)
    assert v.tobytes() == hv.tobytes() and l.tobytes() == hl.tobytes()
    np.testing.assert_array_equal(l, less)


# ------------------------------------------------------------ end to end
def _chrom_pixels(rng, N, depth):
    i = np.arange(N)
    d = np.abs(i[:, None] - i[None, :])
    lam = depth * (d + 1.0) ** -1.05 * rng.lognormal(0, 0.2, N)[:, None]
    lam = np.triu(lam) + np.triu(lam, 1).T
    for _ in range(N // 25):
        a = int(rng.integers(5, N - 80))
        b = a + int(rng.integers(6, 60))
        lam[a - 1:a + 2, b - 1:b + 2] *= 4.0
    H = np.triu(rng.poisson(np.triu(lam)))
    gaps = rng.choice(N, size=max(N // 80, 1), replace=False)
    H[gaps, :] = 0
    H[:, gaps] = 0
    r, c = np.nonzero(H)
    return r, c, H[r, c].astype(np.int32), np.sort(gaps)


def _cooler(tmp_path, res, names, sizes, seed, depth):
    rng = np.random.default_rng(seed)
    chromsizes = [(nm, N * res - res // 2) for nm, N in zip(names, sizes)]
    b1, b2, cnt, gaps, off = [], [], [], {}, 0
    for nm, N in zip(names, sizes):
        r, c, v, g = _chrom_pixels(rng, N, depth)
        b1.append(r + off)
        b2.append(c + off)
        cnt.append(v)
        gaps[nm] = g
        off += N
    path = str(tmp_path / "sample.cool")
    coolio.create_cooler(path, {res: (chromsizes, np.concatenate(b1), np.concatenate(b2), np.concatenate(cnt))})
    coolio.balance_cooler(f"{path}::{res}", ignore_diags=1, cis_only=True)
    return path, f"{path}::{res}", gaps


def _numpy_rank(uri):
    def fn(chro, rows, cols):
        with coolio.Cooler(uri) as c:
            lo, hi = c.extent(chro)
            b1, b2, v = c.pixel_rows(lo, hi)
        val, less = loops.diag_rank_reference(b1, b2, v, lo, hi - lo, rows, cols)
        return val, less, hi - lo
    return fn


@pytest.mark.parametrize("allelic", [False, "Maternal"])
def test_run_loops_end_to_end(tmp_path, allelic):
    from hichap_master_amd.StructureFind import StructureFind
    res = 20000
    names = ["chr1", "chr2"] if allelic is False else ["M1", "P1", "M2"]
    sizes = [700, 500] if allelic is False else [600, 600, 400]
    path, uri, gaps = _cooler(tmp_path, res, names, sizes, seed=9, depth=60.0)
    sf = StructureFind(path, res, Allelic=allelic, GapFile={str(res): gaps} if allelic else None,
                       Loop_ratio=0.6, Loop_strength=8)
    out = tmp_path / "Sample"
    sf.run_Loops(str(out))
    raw = out / "Sample_Loops_20K.txt"
    sel = out / "Selected_Sample_Loops_20K.txt"
    clu = out / ("Cluster_Selected_Sample_Loops_20K.txt" if allelic is False else "Cluster_Sample_Loops_20K.txt")
    want_files = {raw.name, clu.name} | ({sel.name} if allelic is False else set())
    assert {p.name for p in out.iterdir()} == want_files
    assert sf.out_fil == str(clu)
    rank = _numpy_rank(uri)
    check = tmp_path / "check"
    check.mkdir()
    src = raw
    if allelic is False:
        raw_lines = raw.read_text().splitlines(keepends=True)
        want = loops.loop_select(raw_lines, rank, res, 0.6, 8)
        assert sel.read_text() == "".join(want)
        assert 1 < len(want) < len(raw_lines)              # some lines pass, some are rejected
        src = sel
    copy = check / src.name
    copy.write_text(src.read_text())
    want_clu = loops.loop_cluster(str(copy), res, allelic, lambda ch, r, c: rank(ch, r, c)[0])
    assert clu.read_text() == open(want_clu).read()
    lines = clu.read_text().splitlines()[1:]
    assert len(lines) >= 1
    got = sf.Loading_Loops()
    assert got is sf.loops and got["chr"].tolist() == [ln.split("\t")[0] for ln in lines]
    assert got["start"].tolist() == [int(ln.split("\t")[1]) for ln in lines]
    assert got["end"].tolist() == [int(ln.split("\t")[2]) for ln in lines]


@pytest.mark.parametrize("case,allelic", [("trad", False), ("maternal", "Maternal")])
def test_golden_fixture_from_cooler(tmp_path, golden, case, allelic):
    """The reference's Loop_Selecting / LoopCluster outputs at 40 kb
    (tests/golden/make_golden_loopselect.py) from a cooler built from the
    fixture's matrices."""
    from hichap_master_amd.StructureFind import StructureFind
    g = golden("loopselect_40k")
    res = int(g["res"])
    mats = {k.split("/")[-1]: g[k].astype(np.int64) for k in g if k.startswith(case + "/M/")}
    names = sorted(mats)
    b1, b2, cnt, off = [], [], [], 0
    for nm in names:
        r, c = np.nonzero(np.triu(mats[nm]))
        b1.append(r + off)
        b2.append(c + off)
        cnt.append(mats[nm][r, c].astype(np.int32))
        off += mats[nm].shape[0]
    path = str(tmp_path / "golden.cool")
    coolio.create_cooler(path, {res: ([(nm, mats[nm].shape[0] * res) for nm in names], np.concatenate(b1),
                                      np.concatenate(b2), np.concatenate(cnt))})
    sf = StructureFind(path, res, Allelic=allelic, Loop_ratio=float(g["ratio"]), Loop_strength=int(g["strength"]))
    rawfil = tmp_path / "g_Loops_40K.txt"
    rawfil.write_text(bytes(g[f"{case}/raw"]).decode())
    if allelic is False:
        sel = tmp_path / "Selected_g_Loops_40K.txt"
        sf.Loop_Selecting(str(rawfil), str(sel))
        assert sel.read_text() == bytes(g["trad/selected"]).decode()
        rawfil = sel
    sf.LoopCluster(str(rawfil))

    def by_chrom(text):
        per = {}
        for ln in text.splitlines()[1:]:
            per.setdefault(ln.split("\t")[0], []).append(ln)
        return per
    got, want = open(sf.out_fil).read(), bytes(g[f"{case}/cluster"]).decode()
    assert got.splitlines()[0] == want.splitlines()[0]
    assert by_chrom(got) == by_chrom(want)
