"""Host logic of hichap_master_amd.AllelicSpecificity against the reference's
own tables (tests/golden/make_golden_allelic.py), with the two GPU calls
replaced by NumPy stand-ins defined here: a dense slice for
``pixel_windows`` and the sorted outer difference + ``searchsorted`` for
``pairdiff_rank``.  The stand-ins and helpers are shared with
tests/test_allelic_gpu.py, which runs the same comparisons on the kernels."""
import numpy as np
import pytest

from hichap_master_amd import AllelicSpecificity as AS
from hichap_master_amd import coolio

# text and integer columns must be identical; float columns agree at this
# rtol: the arithmetic is the reference's own NumPy / SciPy calls on equal
# inputs, so the margin covers library-version differences between machines
RTOL = 1e-9


# ------------------------------------------------------------- stand-ins
def dense_from_pixels(bin1, bin2, count, lo, N):
    b1 = np.asarray(bin1, dtype=np.int64) - lo
    b2 = np.asarray(bin2, dtype=np.int64) - lo
    c = np.asarray(count, dtype=np.float64)
    k = (b1 >= 0) & (b1 < N) & (b2 >= 0) & (b2 < N)
    H = np.zeros((N, N))
    H[b1[k], b2[k]] = c[k]
    H[b2[k], b1[k]] = c[k]
    return H


def dense_windows(bin1, bin2, count, lo, N, wrow, wcol, h, w, stream=None):
    H = dense_from_pixels(bin1, bin2, count, lo, N)
    out = np.zeros((len(wrow), h, w))
    for k, (r, c) in enumerate(zip(wrow, wcol)):
        if r < 0 or c < 0 or r + h > N or c + w > N:
            raise ValueError(f"window {k} leaves [0, {N})")
        out[k] = H[r:r + h, c:c + w]
    return out


def outer_rank(a, b, q, stream=None):
    return np.searchsorted(np.sort(np.subtract.outer(np.asarray(a), np.asarray(b)).ravel()), q, "left")


@pytest.fixture
def numpy_standins(monkeypatch):
    monkeypatch.setattr(AS, "pixel_windows", dense_windows)
    monkeypatch.setattr(AS, "pairdiff_rank", outer_rank)


# --------------------------------------------------------------- helpers
def fixture_matrices(g):
    """{'M1': numerators of the upper triangle as a dense int64 matrix, ...}"""
    out = {}
    for chro, N in zip(g["chroms"].tolist(), g["sizes"].tolist()):
        for hap in "MP":
            num = np.zeros((N, N), dtype=np.int64)
            num[np.triu_indices(N)] = g[f"numer/{hap}{chro}"]
            out[hap + chro] = num
    return out


def write_cooler(path, res, numer, rename=None):
    """The haplotype cooler of the fixture: float counts numerator / 64,
    chromosomes M1, P1, M2, P2 in file order."""
    names = list(numer)
    b1, b2, cnt, off = [], [], [], 0
    for nm in names:
        r, c = np.nonzero(numer[nm])
        b1.append(r + off)
        b2.append(c + off)
        cnt.append(numer[nm][r, c] / 64.0)
        off += numer[nm].shape[0]
    sizes = [((rename or {}).get(nm, nm), numer[nm].shape[0] * res) for nm in names]
    coolio.create_cooler(path, {res: (sizes, np.concatenate(b1), np.concatenate(b2), np.concatenate(cnt))})
    return path


def text_of(g, key):
    return bytes(g[key]).decode()


def assert_table(got, want, float_cols, skip=()):
    """``skip``: {(line, column)} not compared (the golden's STALE fields)."""
    got, want = got.splitlines(), want.splitlines()
    assert got[0] == want[0]
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got[1:], want[1:])):
        fa, fb = a.split("\t"), b.split("\t")
        assert len(fa) == len(fb)
        for col, (x, y) in enumerate(zip(fa, fb)):
            if (k, col) in skip:
                continue
            if col in float_cols and "NA" not in (x, y):
                assert np.isclose(float(x), float(y), rtol=RTOL, atol=0.0), (k, col, x, y)
            else:
                assert x == y, (k, col, x, y)


def sample_restated(H, b, o):
    """SampleGenerate restated on the dense matrix."""
    Z = H - np.diag(H.diagonal())
    up, down, mid = Z[b - o:b, b - o:b], Z[b:b + o, b:b + o], np.tril(Z[b - o:b, b:b + o])
    nz = [x[x != 0] for x in (up, down, mid)]
    BG = (nz[0].sum() + nz[1].sum() + nz[2].sum()) / (len(nz[0]) + len(nz[1]) + len(nz[2]))
    return (mid / BG).reshape(-1)


def check_boundary_table(g, got):
    """The boundary table against the golden; the STALE fields of the
    one-valid-position lines (deviation 1) against a NumPy restatement."""
    from scipy.stats import ttest_rel
    res, o = int(g["res"]), int(g["offset"])
    want = text_of(g, "boundary_table")
    stale = {(k, col) for k, ln in enumerate(want.splitlines()[1:]) for col, x in enumerate(ln.split("\t"))
             if x == "STALE"}
    assert_table(got, want, {3, 4, 5, 6, 7}, skip=stale)
    kinds = g["boundary_kinds"].tolist()
    bounds = [ln.split() for ln in text_of(g, "boundary_file").splitlines()]
    written = [(b, k) for b, k in zip(bounds, kinds) if k not in ("equal_skipped", "neither")]
    lines = [ln.split("\t") for ln in got.splitlines()[1:]]
    assert len(written) == len(lines)
    assert {k for k, _ in stale} == {k for k, (_, kind) in enumerate(written) if kind.endswith("_only")}
    assert len(stale) == 3 * 4
    H = {nm: (lambda n: (np.triu(n) + np.triu(n, 1).T) / 64.0)(num) for nm, num in fixture_matrices(g).items()}
    for k, ((chro, p1, p2), kind) in enumerate(written):
        assert lines[k][:3] == [chro, p1, p2]
        if not kind.endswith("_only"):
            continue
        b = (int(p1) if kind == "first_only" else int(p2)) // res
        M_S, P_S = sample_restated(H["M" + chro], b, o), sample_restated(H["P" + chro], b, o)
        keep = (M_S != 0) & (P_S != 0)
        stat, p = ttest_rel(M_S[keep], P_S[keep])
        np.testing.assert_allclose([float(x) for x in lines[k][3:7]], [M_S[keep].mean(), P_S[keep].mean(), stat, p],
                                   rtol=RTOL, atol=0)


def run_loops(g, tmp_path, cool, name=lambda c: c):
    fil = tmp_path / "g_Loops_40K.txt"
    fil.write_text("".join("\t".join([name(ln.split("\t")[0])] + ln.split("\t")[1:]) + "\n"
                           for ln in text_of(g, "loop_file").splitlines()))
    L = AS.LoopAllelicSpecificity(cool, str(fil), int(g["res"]))
    L.Running()
    assert L.outfile == str(tmp_path / "Allelic_Specificity_g_Loops_40K.txt")
    return L, open(L.outfile).read()


def run_boundaries(g, tmp_path, cool, key="boundary_file"):
    fil = tmp_path / (key + ".txt")
    fil.write_text(text_of(g, key))
    B = AS.BoundaryAllelicSpecificity(cool, str(fil), int(g["res"]))
    out = tmp_path / (key + "_AS.txt")
    B.Running(str(out))
    return B, out.read_text()


def run_compartments(g, tmp_path, fm=None, fp=None):
    if fm is None:
        fm, fp = tmp_path / "M_PC.txt", tmp_path / "P_PC.txt"
        fm.write_text(text_of(g, "pc_m"))
        fp.write_text(text_of(g, "pc_p"))
    Cm = AS.CompartmentAllelicSpecificity(str(fm), str(fp), int(g["res"]))
    out = tmp_path / "compartment_AS.txt"
    Cm.Running(str(out))
    return Cm, out.read_text()


@pytest.fixture
def fixture_cooler(golden, tmp_path):
    g = golden("allelic_40k")
    return g, write_cooler(str(tmp_path / "hap.cool"), int(g["res"]), fixture_matrices(g))


# ----------------------------------------------------------------- tests
def test_loop_table_equals_reference(fixture_cooler, tmp_path, numpy_standins):
    g, cool = fixture_cooler
    L, got = run_loops(g, tmp_path, cool)
    assert_table(got, text_of(g, "loop_table"), {5, 6, 7, 8, 9, 10})
    n = len(got.splitlines()) - 1
    assert L.Data.size == n and L.Mean.size > n and np.all(np.diff(L.Mean) >= 0) and np.all(L.Mean != 0)
    assert 0 < L.p < 1 and L.p == L.sum_M / L.sum_T


def test_single_stat_branches(golden):
    g = golden("allelic_40k")
    L = AS.LoopAllelicSpecificity("none.cool", "none.txt", 40000)
    want = g["stat_out"]
    assert np.isnan(want).sum() == 4 and np.isfinite(want).sum() == 4
    for (p, count, nobs), w in zip(g["stat_in"].tolist(), want.tolist()):
        got = L.calculate_single_stat(p, count, nobs)
        if np.isnan(w):
            assert got == "NA" and L.calculate_Pvalue(got) == "NA"
        else:
            assert np.isclose(got, w, rtol=RTOL, atol=0)
            assert 0 <= L.calculate_Pvalue(got) <= 1


def test_loop_names_are_kept_whole(golden, tmp_path, numpy_standins):
    """Deviation 4: 'S8' would cut 'chr1_random' to 'chr1_ran'."""
    g = golden("allelic_40k")
    ren = {h + c: h + "chr" + c + "_random" for h in "MP" for c in "12"}
    cool = write_cooler(str(tmp_path / "named.cool"), int(g["res"]), fixture_matrices(g), rename=ren)
    _, got = run_loops(g, tmp_path, cool, name=lambda c: "chr" + c + "_random")
    assert {ln.split("\t")[0] for ln in got.splitlines()[1:]} == {"chr1_random", "chr2_random"}
    short = got.replace("chr1_random\t", "1\t").replace("chr2_random\t", "2\t")
    assert_table(short, text_of(g, "loop_table"), {5, 6, 7, 8, 9, 10})


def test_boundary_table_equals_reference(fixture_cooler, tmp_path, numpy_standins):
    g, cool = fixture_cooler
    B, got = run_boundaries(g, tmp_path, cool)
    check_boundary_table(g, got)
    assert B.results.size == len(got.splitlines()) - 1
    assert np.all(np.isfinite(B.results["q_value"]))


def test_boundaries_near_chromosome_ends_are_skipped(fixture_cooler, tmp_path, numpy_standins, capsys):
    """Deviation 2: windows leaving [0, N) are skipped; windows touching bin
    0 and bin N are not; the q-values stay finite."""
    g, cool = fixture_cooler
    res, o = int(g["res"]), int(g["offset"])
    N = dict(zip(g["chroms"].tolist(), g["sizes"].tolist()))
    B, got = run_boundaries(g, tmp_path, cool, key="boundary_edge_file")
    out = capsys.readouterr().out
    bounds = [ln.split() for ln in text_of(g, "boundary_edge_file").splitlines()]
    fits = [all(int(p) // res - o >= 0 and int(p) // res + o <= N[c] for p in (p1, p2)) for c, p1, p2 in bounds]
    assert fits.count(False) == 4 and out.count("too close to the chromosome end") == 4
    assert any(int(p1) // res == o for (c, p1, p2), f in zip(bounds, fits) if f)
    assert any(int(p1) // res + o == N[c] for (c, p1, p2), f in zip(bounds, fits) if f)
    rows = [ln.split("\t")[:3] for ln in got.splitlines()[1:]]
    assert rows == [b for b, f in zip(bounds, fits) if f]
    assert np.all(np.isfinite(B.results["p_value"])) and np.all(np.isfinite(B.results["q_value"]))


def test_boundaries_without_pairs_or_cells_are_skipped(golden, tmp_path, numpy_standins, capsys):
    """Deviation 3: a window without a nonzero cell, and samples that pass
    the zero test but share fewer than 2 nonzero positions."""
    g = golden("allelic_40k")
    res, o = int(g["res"]), int(g["offset"])
    numer = fixture_matrices(g)
    numer["M1"][50:76, :] = 0
    numer["M1"][:, 50:76] = 0                        # the window of bin 62 is empty in M
    r, c = np.tril_indices(o)
    even = (r + c) % 2 == 0
    numer["M2"][40 + r[even], 50 + c[even]] = 0      # bin 50 of '2': M and P nonzero on
    numer["P2"][40 + r[~even], 50 + c[~even]] = 0    # complementary cells of the block
    cool = write_cooler(str(tmp_path / "holes.cool"), res, numer)
    fil = tmp_path / "b.txt"
    fil.write_text("".join("%s\t%d\t%d\n" % (ch, a * res, b * res) for ch, a, b in
                           [("1", 20, 20), ("1", 62, 62), ("2", 50, 50), ("2", 15, 15), ("1", 62, 20)]))
    B = AS.BoundaryAllelicSpecificity(cool, str(fil), res)
    B.Running(str(tmp_path / "b_AS.txt"))
    out = capsys.readouterr().out
    assert out.count("without a nonzero cell") == 2 and out.count("fewer than 2 nonzero pairs") == 1
    assert B.results["chr"].tolist() == ["1", "2"] and B.results["boundary1"].tolist() == [20 * res, 15 * res]
    assert np.all(np.isfinite(B.results["q_value"]))


def test_compartment_table_equals_reference(golden, tmp_path, numpy_standins):
    g = golden("allelic_40k")
    Cm, got = run_compartments(g, tmp_path)
    assert_table(got, text_of(g, "compartment_table"), {2, 3, 4, 5, 6})
    assert Cm.n_BG == Cm.M_candidate.size * Cm.P_candidate.size == Cm.results.size ** 2
    assert list(Cm.M_PC) == g["chroms"].tolist()
    assert not hasattr(Cm, "BG")


def test_run_compartment_plot_raises_before_any_work(tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    out = tmp_path / "Sample"
    with pytest.raises(NotImplementedError, match="Plot_Compartment"):
        StructureFind(str(tmp_path / "absent.cool"), 40000).run_Compartment(str(out))
    assert not out.exists()
