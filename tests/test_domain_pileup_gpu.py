"""Domain pileups on the GPU (csrc/pileup.hip):
``hh_domain_pileup_pixels`` against the dense restatement
(tests/domain_pileup_ref.py) -- bit for bit where every product, quotient and
sum is exact in fp64 (which the test establishes with exact rationals), within
a bound derived from the number of terms otherwise -- against
``pileup_pixels`` where the two definitions meet, then ``run_DomainPileup`` on
a chromosome with planted domains, through the traditional (balanced) path,
the haplotype (raw) path and a domain file."""
import fractions
import os

import numpy as np
import pytest

from hichap_master_amd import _lib, coolio, h5
from hichap_master_amd import domain_pileup as dp
from hichap_master_amd import pileup as pu
from hichap_master_amd._lib import HipLibraryError, ptr
from hichap_master_amd.StructureFind import StructureFind, py2_float_str
from tests import domain_pileup_data as data
from tests import domain_pileup_ref as ref
from tests.knobs import tuned

pytestmark = pytest.mark.gpu

RES, N, LO, NB, N_EXP = data.RES, data.N, data.LO, data.NB, data.N_EXP
HH_ERR_ARG = -1
U53 = 2.0 ** -53


@pytest.fixture(autouse=True)
def small_chunk():
    """16 features per chunk: ten chunks, the last one partial, lie inside the
    lists of 150 features."""
    with tuned(pileup_chunk=data.CHUNK):
        yield


def _dev(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.array(a)).cuda() for a in arrays]


def _call(kind, which, R, P, use_e, min_dist, device=False):
    b1, b2, cnt = data.table()
    w, bad = data.weights(kind)
    start, end = data.features(which)
    e = data.expected_vector(kind, use_e)
    if device:
        b1, b2, cnt, w, bad, start, end, e = _dev(b1, b2, cnt, w, bad, start, end, e)
    S, Wn = dp.domain_pileup_pixels(b1, b2, cnt, w, LO, N, start, end, R, P, e, min_dist, bad)
    if device:
        assert S.is_cuda and Wn.is_cuda
        S, Wn = S.cpu().numpy(), Wn.cpu().numpy()
    G = R + 2 * P
    assert S.dtype == Wn.dtype == np.float64 and S.shape == Wn.shape == (G, G)
    return S, Wn


def test_reference_is_not_vacuous():
    """What the shared input exercises: stored terms in every cell of the
    upper triangle, several terms per feature and cell at L > R, cells that
    lose weight to invalid bins, to min_dist, to the expected and to the ends
    of the chromosome."""
    M = 150
    for R, P in data.GRIDS:
        S, Wn, m = data.want("general_nan", "general", R, P, False, 0)
        assert (m > 0).all() and (S > 0).all() and (Wn > 0).all() and (Wn < M).all()
        S, Wn, m = data.want("general_nan", "general", R, P, True, 3)
        assert m.sum() > 0 and (R + 2 * P == 127 or ((m > 0).all() and (Wn > 0).all()))
    S, Wn, m = data.want("general_nan", "general", 8, 4, False, 0)
    assert m.max() > 40 * M and Wn[0, 0] < Wn[6, 6] < M                 # many terms per feature; flanks off the ends
    Wn3 = data.want("general_nan", "general", 8, 4, False, 3)[1]
    assert (Wn3[np.arange(16), np.arange(16)] < Wn[np.arange(16), np.arange(16)]).all()   # min_dist bites the diagonal
    We = data.want("general_nan", "general", 8, 4, True, 0)[1]
    assert (We <= Wn).all() and (We < Wn).sum() > 100                   # the expected's NaN, zero and cut-off
    L = np.diff(np.array(data.features("general")), axis=0)[0]
    for R, _ in data.GRIDS:
        assert (L == R).any() and ((L % R == 0) & (L > R)).any()
        assert R == 1 or ((L < R).any() and ((L % R != 0) & (L > R)).any())


# ------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("R,P", data.GRIDS)
def test_exact_regime_is_exact(R, P):
    """Counts in 1/64, weights and expected powers of two, every L a power of
    two: no sum, product or quotient of this regime rounds, so any order of
    the additions gives the restatement's bits.  Two ways: the bits are
    counted on the input, and the float restatement equals the restatement in
    exact rationals (at G = 127, where a pixel feeds up to 63 x 63 cells, on
    the first 24 features: a chunk and a partial one)."""
    b1, b2, cnt = data.table()
    start, end = data.features("pow2")
    L = (end - start).astype(np.int64)
    k = cnt * 64
    assert np.array_equal(k, np.rint(k)) and 0 < k.min() and k.max() < 2 ** 12          # counts: 12 bits above 2^-6
    assert (L & (L - 1) == 0).all() and L.max() == 64                                   # phi = c / 2^(<= 12)
    for kind in ("exact_nan", "raw_bad"):
        w = data.weights(kind)[0]
        e = data.expected_vector(kind, True)
        ok = np.isfinite(e) & (e > 0)
        for x in ([] if w is None else [w[np.isfinite(w)]]) + [e[ok]]:
            assert np.array_equal(np.frexp(x)[0], np.full(x.size, 0.5))                 # powers of two
        assert (w is None or w[np.isfinite(w)].min() >= 2.0 ** -3) and e[ok].max() <= 4.0
        # a term is k 2^-6 w w / e * c / L^2 with c an integer < 2^13 (o <= min(L, R) <= 63, doubled): k c has at most
        # 25 bits, and every term is a multiple of 2^-(6 + 3 + 3 + 2 + 12) = 2^-26; the terms are non-negative, so
        # every partial sum is a multiple of 2^-26 below the final sum: exact while that stays below 2^27
        for use_e in (False, True):
            S, Wn, m = data.want(kind, "pow2", R, P, use_e, 0)
            assert S.max() < 2.0 ** 27 and np.array_equal(S * 2.0 ** 26, np.rint(S * 2.0 ** 26))
            assert Wn.max() <= 150 and np.array_equal(Wn * 2.0 ** 12, np.rint(Wn * 2.0 ** 12))
    G = R + 2 * P
    n = 150 if G < 127 else data.CHUNK + 8
    for kind in ("exact_nan", "raw_bad") if G < 127 else ("exact_nan",):
        args = (*data.dense(kind), start[:n], end[:n], R, P, data.expected_vector(kind, True), 0, data.CHUNK)
        S, Wn, m = data.want(kind, "pow2", R, P, True, 0) if n == 150 else ref.domain_pileup_sums(*args)
        Sq, Wq, mq = ref.domain_pileup_sums(*args, number=fractions.Fraction)
        assert np.array_equal(m, mq) and m.sum() > 0
        assert all(fractions.Fraction(float(S[u, v])) == Sq[u][v] for u in range(G) for v in range(G))
        assert all(fractions.Fraction(float(Wn[u, v])) == Wq[u][v] for u in range(G) for v in range(G))


@pytest.mark.parametrize("kind", ["exact_nan", "raw_bad"])
@pytest.mark.parametrize("min_dist", [0, 3])
@pytest.mark.parametrize("use_e", [False, True])
@pytest.mark.parametrize("R,P", data.GRIDS)
def test_exact(R, P, use_e, min_dist, kind):
    S, Wn, m = data.want(kind, "pow2", R, P, use_e, min_dist)
    assert Wn.sum() > 0 and S.sum() > 0
    got_S, got_Wn = _call(kind, "pow2", R, P, use_e, min_dist)
    assert np.array_equal(got_Wn, Wn)
    assert np.array_equal(got_S, S)


# -------------------------------------------------- 2. random positive weights
def _rtol(m):
    """At most 5 roundings per term (two products, the division by the
    expected, phi, t * phi) and at most 3 m additions of non-negative values
    on the way of m terms into a cell (inside the features, into the chunks,
    across the chunks): a relative (3 m + 6) 2^-53 to first order on either
    side, and the restatement's own float sums double it.  Derived from the
    input, not measured."""
    return 2.0 * (3.0 * m + 6.0) * U53


@pytest.mark.parametrize("kind,R,P,use_e,min_dist", [
    ("general_nan", 8, 4, True, 3), ("general_bad", 8, 4, False, 0), ("general_bad", 7, 3, True, 0),
    ("general_nan", 5, 0, False, 3), ("general_nan", 1, 0, True, 0), ("general_bad", 63, 32, True, 3)])
def test_general(kind, R, P, use_e, min_dist):
    S, Wn, m = data.want(kind, "general", R, P, use_e, min_dist)
    S1, Wn1, m1 = data.want(kind, "general", R, P, use_e, min_dist, chunk=1 << 20)      # one chunk: plain ascending k
    assert np.array_equal(m1, m) and m.sum() > 0
    for device in (False, True):
        got_S, got_Wn = _call(kind, "general", R, P, use_e, min_dist, device)
        assert np.array_equal(got_Wn, Wn)                                               # determined by the definition
        for want_S in (S, S1):
            err = np.abs(got_S - want_S)
            bound = _rtol(m) * np.abs(want_S)
            print(f"{kind} R={R} P={P} expected={use_e} min_dist={min_dist} device={device}: max error / bound "
                  f"{(err / np.where(bound > 0, bound, 1.0)).max():.3g}, cells differing {int((got_S != want_S).sum())} "
                  f"of {got_S.size}, max terms per cell {int(m.max())}")
            assert (err <= bound).all()


# --------------------------------------------------------------- 3. reduction
@pytest.mark.parametrize("kind,use_e,min_dist", [("general_nan", True, 2), ("general_bad", True, 0),
                                                 ("general_bad", False, 3)])
def test_reduces_to_the_pileup(kind, use_e, min_dist):
    """(R, P) = (7, 3) and every L = 7: each output cell is one bin, so S and
    Wn are ``pileup_pixels``' S and Cn for the on-diagonal features start + 3,
    flank 6, bit for bit."""
    b1, b2, cnt = data.table()
    w, bad = data.weights(kind)
    start, end = data.features("seven")
    assert ((end - start) == 7).all()
    e = data.expected_vector(kind, use_e)
    S, Wn = dp.domain_pileup_pixels(b1, b2, cnt, w, LO, N, start, end, 7, 3, e, min_dist, bad)
    S0, Cn0 = pu.pileup_pixels(b1, b2, cnt, w, LO, N, start + 3, start + 3, 6, e, min_dist, bad)
    assert S0.sum() > 0 and Cn0.max() > 50
    assert S.tobytes() == S0.tobytes()
    assert np.array_equal(Wn, Cn0.astype(np.float64))
    want = data.want(kind, "seven", 7, 3, use_e, min_dist)
    assert np.array_equal(S, want[0]) and np.array_equal(Wn, want[1])


# ------------------------------------------------- 4. symmetry and agreement
def test_bitwise():
    kind, (R, P) = "general_nan", (8, 4)
    S1, W1 = _call(kind, "general", R, P, True, 3)
    S2, W2 = _call(kind, "general", R, P, True, 3)
    S3, W3 = _call(kind, "general", R, P, True, 3, device=True)
    assert S1.tobytes() == S2.tobytes() == S3.tobytes()                 # two calls; host form = device form
    assert W1.tobytes() == W2.tobytes() == W3.tobytes()
    assert S1.tobytes() == S1.T.copy().tobytes() and W1.tobytes() == W1.T.copy().tobytes()
    assert (S1 > 0).all()
    for R, P in ((63, 32), (7, 3)):
        S, W = _call("general_bad", "general", R, P, False, 0, device=True)
        assert S.tobytes() == S.T.copy().tobytes() and W.tobytes() == W.T.copy().tobytes() and (S > 0).all()
    # the in-feature order is the restatement's (ascending a, then b): the same bits, at both chunk sizes
    want = data.want(kind, "general", R, P, True, 3) if (R, P) == (8, 4) else data.want(kind, "general", 8, 4, True, 3)
    assert np.array_equal(S1, want[0]) and np.array_equal(W1, want[1])
    with tuned(pileup_chunk=data.DEFAULT_CHUNK):
        S5, W5 = _call("general_bad", "general", 8, 4, True, 0)
    want = data.want("general_bad", "general", 8, 4, True, 0, chunk=data.DEFAULT_CHUNK)
    assert np.array_equal(S5, want[0]) and np.array_equal(W5, want[1])
    assert not np.array_equal(S5, data.want("general_bad", "general", 8, 4, True, 0)[0])   # (the chunk size matters)


# ------------------------------------------------------------------ 5. errors
def test_no_features_and_no_pixels():
    b1, b2, cnt = data.table()
    w, bad = data.weights("exact_nan")
    none = (np.empty(0, np.int64), np.empty(0, np.int64), np.empty(0))
    start, end = data.features("pow2")
    e = data.expected_vector("exact_nan", True)
    for device in (False, True):
        t = _dev(b1, b2, cnt, w, e, start, end, *none) if device else (b1, b2, cnt, w, e, start, end, *none)
        tb1, tb2, tc, tw, te, ts, tend, n1, n2, nc = t
        S, Wn = dp.domain_pileup_pixels(tb1, tb2, tc, tw, LO, N, ts[:0], tend[:0], 8, 4, te, 3)       # M = 0
        S0, Wn0 = dp.domain_pileup_pixels(n1, n2, nc, tw, LO, N, ts, tend, 8, 4, te, 3)               # nnz = 0
        if device:
            S, Wn, S0, Wn0 = (x.cpu().numpy() for x in (S, Wn, S0, Wn0))
        assert S.shape == (16, 16) and not S.any() and not Wn.any()
        assert not S0.any() and np.array_equal(Wn0, data.want("exact_nan", "pow2", 8, 4, True, 3)[1])


def test_argument_errors_leave_outputs_untouched():
    b1, b2, cnt = data.table()
    w = data.weights("exact_nan")[0]
    start, end = data.features("pow2")
    e = data.expected_vector("exact_nan", True)
    lib = _lib.load()
    S, Wn = np.full((127, 127), -7.5), np.full((127, 127), -3.25)

    def run(N_=N, R=8, P=4, min_dist=0, n_weight=NB, n_exp=N_EXP, start_=start, end_=end, ex=e):
        return lib.hh_domain_pileup_pixels(ptr(b1), ptr(b2), ptr(cnt), b1.size, ptr(w), n_weight, LO, N_, None,
                                           ptr(start_), ptr(end_), start_.size, R, P, ptr(ex), n_exp, min_dist,
                                           ptr(S), ptr(Wn), 0, None)

    assert run(N_=0) == HH_ERR_ARG                                                           # N < 1
    assert run(R=0) == HH_ERR_ARG and run(P=-1) == HH_ERR_ARG and run(R=64, P=32) == HH_ERR_ARG   # R, P, G = 128
    assert b"body" in lib.hh_last_error()
    assert run(R=128, P=0) == HH_ERR_ARG
    assert run(min_dist=-1) == HH_ERR_ARG                                                    # min_dist
    assert b"min_dist" in lib.hh_last_error()
    assert run(n_exp=0) == HH_ERR_ARG and run(n_exp=N + 1) == HH_ERR_ARG                     # n_expected
    assert b"n_expected" in lib.hh_last_error()
    for k, (s, t) in ((0, (-1, 3)), (149, (10, N + 1)), (70, (5, 5)), (33, (9, 4)), (100, (N, N))):   # a bad feature
        s2, e2 = start.copy(), end.copy()
        s2[k], e2[k] = s, t
        assert run(start_=s2, end_=e2) == HH_ERR_ARG, (s, t)
        assert b"feature" in lib.hh_last_error()
    assert run(n_weight=LO + N - 1) == HH_ERR_ARG                                            # weights
    assert b"weights do not cover" in lib.hh_last_error()
    assert np.all(S == -7.5) and np.all(Wn == -3.25)
    import torch                                                                             # the device form too
    tb1, tb2, tc, tw, te = _dev(b1, b2, cnt, w, e)
    tS = torch.full((16, 16), -7.5, dtype=torch.float64).cuda()
    tW = torch.full((16, 16), -3.25, dtype=torch.float64).cuda()
    for s, t in ((-1, 3), (10, N + 1), (5, 5), (9, 4)):
        s2, e2 = start.copy(), end.copy()
        s2[100], e2[100] = s, t
        ts, tend = _dev(s2, e2)
        assert lib.hh_domain_pileup_pixels(ptr(tb1), ptr(tb2), ptr(tc), b1.size, ptr(tw), NB, LO, N, None, ptr(ts),
                                           ptr(tend), 150, 8, 4, ptr(te), N_EXP, 0, ptr(tS), ptr(tW), 1,
                                           None) == HH_ERR_ARG
        assert b"feature" in lib.hh_last_error()
    assert bool((tS == -7.5).all()) and bool((tW == -3.25).all())
    with pytest.raises(HipLibraryError, match="body"):
        dp.domain_pileup_pixels(b1, b2, cnt, w, LO, N, start, end, 64, 32)
    # the library is still usable, and only the G x G head of the outputs is written
    assert run(n_exp=0, ex=None) == 0                                                        # (ignored without one)
    S[:], Wn[:] = -7.5, -3.25
    assert run(min_dist=3) == 0
    want = data.want("exact_nan", "pow2", 8, 4, True, 3)
    assert np.array_equal(S.ravel()[:256].reshape(16, 16), want[0])
    assert np.array_equal(Wn.ravel()[:256].reshape(16, 16), want[1])
    assert np.all(S.ravel()[256:] == -7.5) and np.all(Wn.ravel()[256:] == -3.25)


# ------------------------------------------------------- 6. run_DomainPileup
BODY, PAD = 8, 4
BP = [(s * RES + 123, e * RES - 4567) for s, e in data.PLANTED]        # inside the first and the last bin


def _read(out):
    prefix = os.path.basename(out)
    res = StructureFind.properU(RES)
    return [[ln.rstrip("\n").split("\t") for ln in open(os.path.join(out, f"{prefix}_{what}_{res}.txt"))]
            for what in ("DomainPileup", "DomainPileupWeight", "DomainScore")]


def _check_files(r, out):
    pil, wgt, score = _read(out)
    assert pil == [[py2_float_str(x) for x in row] for row in r["pileup"]]
    assert wgt == [[py2_float_str(x) for x in row] for row in r["Wn"]]
    want = [[k, py2_float_str(r["scores"][k])] for k in dp.SCORE_NAMES]
    want += [["n_features", str(r["n_features"])], ["n_dropped", str(r["n_dropped"])]]
    if "scores_ratio" in r:
        want += [[k + "_over_controls", py2_float_str(r["scores_ratio"][k])] for k in dp.SCORE_NAMES]
    assert score == want
    got = np.array([[float(x) for x in row] for row in pil])            # '%.12g' rounds to 5e-12 (relative)
    np.testing.assert_allclose(got, r["pileup"], rtol=5e-12, atol=0, equal_nan=True)


def _check_sums(r, chrom, M, valid, dmin, starts, ends):
    """The call's sums against the restatement fed with the call's own
    expected: the same association, so the same bits."""
    rc = r["chroms"][chrom]
    assert rc["start"].tolist() == list(starts) and rc["end"].tolist() == list(ends)
    S, Wn, _ = ref.domain_pileup_sums(M, valid, rc["start"], rc["end"], BODY, PAD, rc["expected"], dmin, data.CHUNK)
    assert np.array_equal(rc["Wn"], Wn) and np.array_equal(rc["S"], S)
    assert np.array_equal(r["Wn"], Wn) and np.array_equal(r["S"], S)
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(r["pileup"], np.where(Wn > 0, S / Wn, np.nan))


def _cooler(tmp_path, name, domains=True):
    b1, b2, count, weight = data.planted(domains)
    path = str(tmp_path / name)
    coolio.create_cooler(path, {RES: ([("chr1", weight.size * RES)], b1, b2, count)})
    h5.append_dataset(path, f"{RES}/bins", "weight", weight)
    return path, ref.dense(b1, b2, count, weight, 0, weight.size), ref.validity(weight, 0, weight.size, None)


def test_run_domain_pileup_traditional(tmp_path):
    path, M, valid = _cooler(tmp_path, "trad.cool")
    sf = StructureFind(path, Res=RES)
    out = str(tmp_path / "planted")
    feats = {"chr1": (np.array([a for a, _ in BP]), np.array([b for _, b in BP]))}
    r = sf.run_DomainPileup(out, features=feats, body=BODY, pad=PAD, n_shifts=2, seed=4)
    assert r is sf.DomainPileup_dict and (r["body"], r["pad"]) == (BODY, PAD)
    assert r["n_features"] == len(BP) and r["n_dropped"] == 0
    starts, ends = [s for s, _ in data.PLANTED], [e for _, e in data.PLANTED]
    _check_sums(r, "chr1", M, valid, 2, starts, ends)                    # floor(start), ceil(end)
    _check_files(r, out)
    print("traditional: scores", r["scores"], "over controls", r["scores_ratio"], "controls", r["n_controls"])
    assert r["scores"]["strength"] > 1 and r["scores_ratio"]["strength"] > 1
    rc = r["chroms"]["chr1"]
    assert r["n_controls"] == rc["start_c"].size > 10
    lengths = set((np.array(ends) - np.array(starts)).tolist())
    assert set((rc["end_c"] - rc["start_c"]).tolist()) <= lengths and rc["start_c"].min() >= 0   # moved, not resized
    assert rc["end_c"].max() <= M.shape[0] and not set(zip(rc["start_c"].tolist(), rc["end_c"].tolist())) & set(data.PLANTED)
    Sc, Wc, _ = ref.domain_pileup_sums(M, valid, rc["start_c"], rc["end_c"], BODY, PAD, rc["expected"], 2, data.CHUNK)
    assert np.array_equal(r["S_c"], Sc) and np.array_equal(r["Wn_c"], Wc)
    # a _Domain_ file, the size filters and a distance in bp; observed only
    df = str(tmp_path / "x_Domain_10K.txt")
    with open(df, "w") as f:
        for a, b in BP:
            f.write(f"chr1\t{a}\t{b}\n")
    out2 = str(tmp_path / "observed")
    r2 = sf.run_DomainPileup(out2, domain_file=df, body=BODY, pad=PAD, expected=False, min_dist=4 * RES,
                             min_size=10 * RES, max_size=50 * RES)
    keep = [(s, e) for (s, e), (a, b) in zip(data.PLANTED, BP) if 10 * RES <= b - a <= 50 * RES]
    assert 0 < len(keep) < len(BP) and r2["n_features"] == len(keep) and r2["n_dropped"] == len(BP) - len(keep)
    assert "pileup_c" not in r2 and r2["chroms"]["chr1"]["expected"] is None
    _check_sums(r2, "chr1", M, valid, 4, [s for s, _ in keep], [e for _, e in keep])
    _check_files(r2, out2)


def test_run_domain_pileup_without_domains(tmp_path):
    """No domains planted: the pileup over expected is flat, and so is the
    pileup over the shifted controls."""
    path, M, valid = _cooler(tmp_path, "flat.cool", domains=False)
    feats = {"chr1": (np.array([a for a, _ in BP]), np.array([b for _, b in BP]))}
    r = StructureFind(path, Res=RES).run_DomainPileup(str(tmp_path / "flat"), features=feats, body=BODY, pad=PAD,
                                                      n_shifts=2, seed=4)
    print("no domains: scores", r["scores"], "over controls", r["scores_ratio"])
    assert 0.8 <= r["scores_ratio"]["strength"] <= 1.25
    assert 0.8 <= r["scores"]["strength"] <= 1.25


def test_run_domain_pileup_haplotype(tmp_path):
    """The planted chromosome as the maternal haplotype 'Mb' (raw counts, no
    weights), the NaN-weight bins as its gap list, next to a paternal 'Pb'
    that must not be read; the features are named 'b'."""
    b1, b2, count, weight = data.planted()
    Nc = weight.size
    gap = np.nonzero(~np.isfinite(weight))[0]
    pb = Nc + np.arange(30)
    path = str(tmp_path / "hap.cool")
    coolio.create_cooler(path, {RES: ([("Mb", Nc * RES), ("Pb", 30 * RES)], np.concatenate([b1, pb]),
                                      np.concatenate([b2, pb]), np.concatenate([count, np.full(30, 9)]))})
    out = str(tmp_path / "hap")
    sf = StructureFind(path, Res=RES, Allelic="Maternal", GapFile={str(RES): {"Mb": gap, "Pb": np.array([0])}})
    feats = (np.array([a for a, _ in BP]), np.array([b for _, b in BP]))
    with pytest.raises(ValueError, match="Mb"):
        sf.run_DomainPileup(out, features={"Mb": feats}, body=BODY, pad=PAD)              # names carry no prefix
    r = sf.run_DomainPileup(out, features={"b": feats}, body=BODY, pad=PAD)
    bad = np.zeros(Nc, np.uint8)
    bad[gap] = 1
    M = ref.dense(b1, b2, count, None, 0, Nc)
    assert list(r["chroms"]) == ["Mb"]
    _check_sums(r, "Mb", M, ref.validity(None, 0, Nc, bad), 2, [s for s, _ in data.PLANTED],
                [e for _, e in data.PLANTED])
    _check_files(r, out)
    assert r["scores"]["strength"] > 1 and "scores_ratio" not in r
