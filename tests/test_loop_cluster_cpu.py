"""Loop selection and loop clustering on the host (no GPU):

* ``loops.loop_select`` / ``loops.loop_cluster`` against the reference's own
  ``Loop_Selecting`` / ``LoopCluster`` outputs (tests/golden/loopselect_40k.npz,
  made by tests/golden/make_golden_loopselect.py), compared per chromosome:
  the cross-chromosome order is a stated deviation;
* the iterator-skip quirk of ``peakcluster`` on its own;
* Python-2 number formatting of the Cluster_ file;
* ``run_Loops(plot=True)`` raises before any work;
* the rank identity ``bisect_left = zeros + smaller stored pixels`` of
  ``loops.diag_rank_reference`` against ``bisect_left`` on dense matrices."""
import bisect
import math

import numpy as np
import pytest

from hichap_master_amd import loops


def _text(g, key):
    return bytes(g[key]).decode()


def _pixels(H):
    r, c = np.nonzero(np.triu(H))
    return r, c, H[r, c].astype(np.int64)


def _dense_rank(H, rows, cols):
    value = np.array([H[r][c] for r, c in zip(rows, cols)], dtype=np.int64)
    less = np.array([bisect.bisect_left(sorted(H.diagonal(c - r)), H[r][c]) for r, c in zip(rows, cols)],
                    dtype=np.int64)
    return value, less


def _by_chrom(text):
    lines = text.splitlines()
    per = {}
    for ln in lines[1:]:
        per.setdefault(ln.split("\t")[0], []).append(ln)
    return lines[0], per


@pytest.fixture(scope="module")
def fx(golden):
    g = golden("loopselect_40k")
    mats = {case: {k.split("/")[-1]: g[k].astype(np.int64) for k in g if k.startswith(case + "/M/")}
            for case in ("trad", "maternal")}
    return g, mats


def _rank_fn(mats):
    def fn(chro, rows, cols):
        H = mats[chro]
        b1, b2, c = _pixels(H)
        v, less = loops.diag_rank_reference(b1, b2, c, 0, H.shape[0], rows, cols)
        return v, less, H.shape[0]
    return fn


def test_loop_select_golden(fx):
    g, mats = fx
    raw = _text(g, "trad/raw").splitlines(keepends=True)
    out = loops.loop_select(raw, _rank_fn(mats["trad"]), int(g["res"]), float(g["ratio"]), int(g["strength"]))
    want = _text(g, "trad/selected")
    assert "".join(out) == want          # line order is the input's: the whole file is identical
    assert out[0].count("\t") == 8 and out[1].count("\t") == 9   # nine-name header, ten-column lines
    assert 1 < len(out) < len(raw)


@pytest.mark.parametrize("case,allelic", [("trad", False), ("maternal", "Maternal")])
def test_loop_cluster_golden(fx, tmp_path, case, allelic):
    g, mats = fx
    src = "selected" if case == "trad" else "raw"
    rawfil = tmp_path / ("Selected_g_Loops_40K.txt" if case == "trad" else "g_Loops_40K.txt")
    rawfil.write_text(_text(g, f"{case}/{src}"))
    seen = []

    def value_fn(chro, rows, cols):
        seen.append(chro)
        return _dense_rank(mats[case][chro], rows, cols)[0]

    out = loops.loop_cluster(str(rawfil), int(g["res"]), allelic, value_fn, float(g["weight_q"]))
    assert out == str(tmp_path / ("Cluster_" + rawfil.name))
    head, got = _by_chrom(open(out).read())
    whead, want = _by_chrom(_text(g, f"{case}/cluster"))
    assert head == whead
    assert set(got) == set(want) and got == {k: want[k] for k in got}
    assert sorted(seen) == (["1", "2"] if allelic is False else ["M1", "M2"])
    if allelic:
        assert any("\t1e-20\t" in ln for v in got.values() for ln in v)     # the w_q == 0 loop


def test_peak_cluster_iterator_skip():
    res = 40000
    dis = res * math.sqrt(2) + 1000
    A, B, Cc, D = [("1", a * res, b * res, q) for a, b, q in ((10, 50, .01), (11, 50, .02), (11, 51, .03),
                                                               (12, 51, .04))]
    cls = loops.peak_cluster([D, B, Cc, A], dis, ["1"])
    # B joins A and is removed; C slides into its place and is never examined
    # (a loop over a snapshot would give [A, B, C], [D])
    assert cls == [[A, B], [Cc, D]]
    assert loops.filter_initial(cls) == [("1", 10 * res, 50 * res, .01, 2.0), ("1", 11 * res, 51 * res, .03, 2.0)]
    final, rounds = loops.cluster_rounds([D, B, Cc, A], res)
    assert final == [("1", 10 * res, 50 * res, .01, 4.0)] and rounds == 2


def test_cluster_number_formatting(tmp_path):
    head = "h\n"
    line = "%s\t%d\t%d\t17\t2\t0.1\t0.1\t2\t0.1\t%s\n"
    raw = tmp_path / "x_Loops_40K.txt"
    raw.write_text(head + line % ("chr10_random", 400000, 2000000, "2.5e-07") + line % ("2", 80000, 800000, "0")
                   + line % ("2", 4000000, 8000000, "0.04"))

    def value_fn(chro, rows, cols):
        return [17 + int(r) for r in rows]

    out = loops.loop_cluster(str(raw), 40000, False, value_fn)
    assert open(out).read().splitlines() == [
        "chr\tstart\tend\tIF\tweight_Q-value\taggregateNum",
        "chr10_random\t400000\t2000000\t27\t2.5e-08\t1.0",
        "2\t80000\t800000\t19\t0.0\t1.0"]
    got = []

    def value_fn_m(chro, rows, cols):
        got.append(chro)
        return [17 + int(r) for r in rows]

    out = loops.loop_cluster(str(raw), 40000, "Paternal", value_fn_m)
    assert got == ["Pchr10_random", "P2"]
    assert open(out).read().splitlines()[1:] == ["chr10_random\t400000\t2000000\t27.0\t2.5e-08\t1",
                                                 "2\t80000\t800000\t19.0\t1e-20\t1"]
    empty = tmp_path / "e_Loops_40K.txt"
    empty.write_text(head)
    assert open(loops.loop_cluster(str(empty), 40000, False, value_fn)).read() == loops.CLUSTER_HEAD


def test_run_loops_plot_raises(tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    sf = StructureFind(None, 40000)
    target = tmp_path / "out"
    with pytest.raises(NotImplementedError):
        sf.run_Loops(str(target), plot=True)
    assert not target.exists()


@pytest.mark.parametrize("N,seed", [(1, 0), (2, 1), (9, 2), (40, 3)])
def test_rank_identity_against_bisect(N, seed):
    rng = np.random.default_rng(seed)
    H = np.triu(rng.integers(0, 4, (N, N)) * rng.integers(0, 2, (N, N)))    # many zeros and ties
    if N >= 9:
        H[np.arange(N - 3), np.arange(3, N)] = 2       # a diagonal where every entry ties
    H = H + np.triu(H, 1).T
    rows, cols = np.triu_indices(N)                    # every pixel, stored or not
    lo = 5
    b1, b2, c = _pixels(H)
    b1, b2 = b1 + lo, b2 + lo
    # foreign pixels: before, after and across the chromosome's end
    b1 = np.concatenate([b1, [0, lo + N, lo]])
    b2 = np.concatenate([b2, [2, lo + N + 1, lo + N]])
    c = np.concatenate([c, [9, 9, 9]])
    v, less = loops.diag_rank_reference(b1, b2, c, lo, N, rows, cols)
    wv, wl = _dense_rank(H, rows, cols)
    np.testing.assert_array_equal(v, wv)
    np.testing.assert_array_equal(less, wl)
    assert np.all(less[v == 0] == 0)
