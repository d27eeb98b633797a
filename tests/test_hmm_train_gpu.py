"""Baum-Welch training of the TAD HMM on the GPU (hh_hmm_bw_*,
hichap_master_amd/csrc/hmm_train.hip) against exhaustive enumeration, the
closed form and the NumPy restatement (tests/hmm_train_ref.py; ghmm itself is
absent: parity with ghmm unpinned), and the Python layers above it
(GaussianMixtureHMM.baumWelch, updateParameter, modelTrain, tad_domains
without a model, run_TADs).

Tolerances are the project's: rtol 1e-9 for HIP against NumPy with another
summation order, rtol 1e-12 for log P (test_tads.py); means, which
may sit near zero, get atol = 1e-9 max|x| beside the rtol."""
import os
import random

import numpy as np
import pytest

from tests import hmm_train_ref as ref
from tests.test_hmm_train_ref import enumeration_case, mstep_from_posteriors
from tests.test_tads import _sf

pytestmark = pytest.mark.gpu

NAMES = ("A", "pi", "mean", "var", "weight")


def _hmm(model):
    from hichap_master_amd.tads import GaussianMixtureHMM
    A, pi, mean, var, weight = ref.copy_model(model)
    return GaussianMixtureHMM(A, [[mean[i], var[i], weight[i]] for i in range(mean.shape[0])], pi)


def _params(m):
    return m.A, m.pi, m.mean, m.var, m.weight


def _prior(k):
    A, B, pi = getattr(_sf(), f"init_parameter_state{k}")()
    B = np.array(B, float)
    return np.array(A, float), np.array(pi, float), B[:, 0].copy(), B[:, 1].copy(), B[:, 2].copy()


def _gpu_step(seqs, model):
    from hichap_master_amd.tads import BaumWelchTrainer
    m = _hmm(model)
    with BaumWelchTrainer(seqs, *m.mean.shape) as tr:
        logp = tr.step(m)
    return _params(m), logp


def _assert_model_close(got, want, xmax, rtol=1e-9):
    for g, w, name in zip(got, want, NAMES):
        np.testing.assert_allclose(g, w, rtol=rtol, atol=1e-9 * xmax if name == "mean" else 0, err_msg=name)


def _xmax(seqs):
    return max(float(np.max(np.abs(s))) for s in seqs)


# ------------------------------------------------ 3. enumeration, closed form
@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("seed", range(3))
def test_step_equals_enumeration(S, seed):
    model, seqs = enumeration_case(S, seed)
    post = [ref.enumerate_posteriors(x, model) for x in seqs]
    want = mstep_from_posteriors(seqs, post, model)
    got, logp = _gpu_step(seqs, model)
    np.testing.assert_allclose(logp, sum(p[3] for p in post), rtol=1e-12)
    _assert_model_close(got, want, _xmax(seqs))
    assert np.array_equal(got[0] == 0.0, model[0] == 0.0)


def test_single_gaussian_closed_form():
    rng = np.random.default_rng(11)
    seqs = [rng.normal(2.0, 3.0, n) for n in (1, 2, 70)]
    model = (np.array([[1.0]]), np.array([1.0]), np.array([[0.5]]), np.array([[4.0]]), np.array([[1.0]]))
    (A, pi, mean, var, weight), logp = _gpu_step(seqs, model)
    allx = np.concatenate(seqs)
    np.testing.assert_array_equal(A, [[1.0]])
    np.testing.assert_array_equal(pi, [1.0])
    np.testing.assert_allclose(weight, [[1.0]], rtol=1e-12)
    np.testing.assert_allclose(mean, [[allx.mean()]], rtol=1e-9)
    np.testing.assert_allclose(var, [[allx.var()]], rtol=1e-9)
    np.testing.assert_allclose(logp, np.sum(-0.5 * np.log(2 * np.pi * 4.0) - 0.5 * (allx - 0.5) ** 2 / 4.0), rtol=1e-12)


# ------------------------------------------------------------ 4. launch edges
def _di_like(rng, n):
    x = np.cumsum(rng.normal(0, 1.5, n)) % 25 - 12
    x[rng.random(n) < 0.06] = 0.0
    return x


def _edge_seqs(case):
    rng = np.random.default_rng(40 + case)
    if case == 0:
        return [_di_like(rng, n) for n in (1, 2, 7, 8, 63, 64, 65, 129, 1000)]
    if case == 1:
        return [_di_like(rng, 333)]
    return [_di_like(rng, int(n)) for n in rng.integers(8, 41, 300)]


@pytest.mark.parametrize("k", [3, 5, 6])
@pytest.mark.parametrize("case", [0, 1, 2])
def test_launch_edges_one_step(case, k):
    seqs = _edge_seqs(case)
    model = _prior(k)
    want, want_logp, _ = ref.step(seqs, model)
    got, logp = _gpu_step(seqs, model)
    np.testing.assert_allclose(logp, want_logp, rtol=1e-12)
    _assert_model_close(got, want, _xmax(seqs))
    again, logp2 = _gpu_step(seqs, model)
    assert logp2 == logp
    for g, a, name in zip(got, again, NAMES):
        assert np.array_equal(g, a), name


# ------------------------------------------------------------- 6. the tails
def test_tail_observations():
    rng = np.random.default_rng(6)
    x = _di_like(rng, 50)
    x[7], x[31] = 400.0, -400.0
    model = _prior(3)
    want, want_logp, _ = ref.step([x], model)
    got, logp = _gpu_step([x], model)
    assert np.isfinite(logp)
    np.testing.assert_allclose(logp, want_logp, rtol=1e-12)
    _assert_model_close(got, want, 400.0)


# ------------------------------------------------- 5, 7. full training runs
def three_state_sequences(seed=2024, n_seq=40):
    """~4 000 observations from a 3-state chain with means (6, 0, -6)."""
    rng = np.random.default_rng(seed)
    P = np.array([[0.90, 0.10, 0.00], [0.04, 0.88, 0.08], [0.12, 0.00, 0.88]])
    means = np.array([6.0, 0.0, -6.0])
    seqs = []
    for n in rng.integers(40, 161, n_seq):
        s, x = int(rng.integers(0, 3)), np.empty(n)
        for t in range(n):
            x[t] = rng.normal(means[s], 1.6)
            s = int(rng.choice(3, p=P[s]))
        seqs.append(x)
    return seqs


@pytest.fixture(scope="module")
def trained3():
    """The NumPy reference's run from the 3-state prior, computed once."""
    seqs = three_state_sequences()
    model, iters, trace, status = ref.train(seqs, _prior(3))
    return seqs, model, iters, trace, status


def test_full_training_matches_reference(trained3):
    from hichap_master_amd.tads import BW_LOGP_DROPPED, BW_MAX_ITER, BaumWelchTrainer
    seqs, _, ref_iters, ref_trace, ref_status = trained3
    # conditions on the fixture (checked on the CPU): the stopping ratios stay
    # 1 % away from eps, the reference floors no variance
    ratios = np.diff(ref_trace) / np.abs(ref_trace[1:])
    assert np.all(np.abs(ratios / 1e-4 - 1.0) > 0.01) and ref_status == 0
    xmax = _xmax(seqs)
    with BaumWelchTrainer(seqs, 3, 3) as tr:
        m = _hmm(_prior(3))
        iters, trace, status = tr.train(m)
        assert iters == ref_iters and status == 0
        np.testing.assert_allclose(trace, ref_trace, rtol=1e-9)
        assert np.all(np.diff(trace) >= -1e-9 * np.abs(trace[1:]))
        assert status & (BW_LOGP_DROPPED | BW_MAX_ITER) == 0
        # one reference step from the GPU's own parameters after k iterations
        for k in (0, 3, iters - 1):
            before, after = _hmm(_prior(3)), _hmm(_prior(3))
            assert tr.train(before, max_iter=k)[0] == k
            assert tr.train(after, max_iter=k + 1)[0] == k + 1
            want, _, _ = ref.step(seqs, _params(before))
            _assert_model_close(_params(after), want, xmax)
    # the public method: same run, in place
    m2 = _hmm(_prior(3))
    it2, tr2 = m2.baumWelch(seqs)
    assert it2 == iters and np.array_equal(tr2, trace)
    for a, b in zip(_params(m), _params(m2)):
        assert np.array_equal(a, b)


def test_structure_is_preserved():
    seqs = three_state_sequences(seed=77, n_seq=12)
    A0 = _prior(5)[0]
    m = _hmm(_prior(5))
    iters, trace = m.baumWelch(seqs)
    assert iters >= 2 and np.all(np.isfinite(trace))
    assert np.all(m.A[A0 == 0.0] == 0.0)
    np.testing.assert_allclose(m.A.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.weight.sum(axis=1), 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.pi.sum(), 1.0, rtol=0, atol=1e-12)


# ----------------------------------------------------------------- 8. errors
def test_errors():
    from hichap_master_amd._lib import HipLibraryError
    from hichap_master_amd.tads import BaumWelchTrainer
    x = np.linspace(-3, 3, 9)
    with pytest.raises(HipLibraryError, match="not finite"):
        BaumWelchTrainer([x, np.array([1.0, np.nan])], 3, 3)
    with pytest.raises(HipLibraryError, match="empty"):
        BaumWelchTrainer([x, np.empty(0), x], 3, 3)
    with pytest.raises(HipLibraryError):
        BaumWelchTrainer([x], 9, 3)
    with pytest.raises(HipLibraryError):
        BaumWelchTrainer([x], 3, 9)
    # state 1 is entered with certainty and has no way out
    A = np.array([[0.0, 1.0], [0.0, 0.0]])
    dead = (A, np.array([1.0, 0.0]), np.zeros((2, 1)), np.ones((2, 1)), np.ones((2, 1)))
    m = _hmm(dead)
    with BaumWelchTrainer([x[:2], x], 2, 1) as tr:
        with pytest.raises(HipLibraryError, match="zero likelihood"):
            tr.step(m)
        for got, want in zip(_params(m), dead):  # a failed step leaves the parameters alone
            assert np.array_equal(got, want)
        assert np.isfinite(tr.step(_hmm((np.array([[0.0, 1.0], [0.5, 0.5]]),) + dead[1:])))


# ------------------------------------------------------------------- 9. API
def _tad_matrices():
    """The matrices of test_tads.test_tad_chain_on_gpu_matches_oracle_scans."""
    from hichap_master_amd import synth
    rng = np.random.default_rng(5)
    mats = {}
    for c, n in (("1", 420), ("2", 300)):
        M = synth.dense_chrom(n, rng, A=30.0, gap_frac=0.04).astype(np.float64)
        tad = np.repeat(np.arange(n), rng.integers(6, 20, n))[:n]
        M = M * np.where(tad[:, None] == tad[None, :], 4.0, 1.0)
        w = 1.0 / np.sqrt(np.maximum(M.sum(axis=1), 1.0))
        mats[c] = M * w[:, None] * w[None, :]
    return mats


def test_tad_domains_trains_its_own_model():
    mats = _tad_matrices()
    sf = _sf()
    assert sf.model is None
    dom = sf.tad_domains(mats)  # NotImplementedError before training was built
    assert all(len(dom[c]) > 0 for c in mats)
    # the NumPy reference under the same three-pass rule on the same segments
    seqs = [sf.DI_all_train[c][k] for c in sorted(sf.DI_all_train) for k in sorted(sf.DI_all_train[c])]
    raw = []
    m_ref, _, _ = ref.train_three_pass(seqs, _prior(3), raw=raw)
    # Condition on the fixture.  These matrices have exact-zero DI values, on
    # which one mixture component collapses, so the reference DOES floor
    # variances here (estimates <= 0.34 x the floor; the smallest one kept is
    # 1.69 x the floor).  What the comparison needs is that no flooring
    # decision is marginal: every estimate is a factor 1.5 away from the floor.
    raw = np.array(raw)
    assert not np.any((raw > 1e-4 / 1.5) & (raw < 1e-4 * 1.5))
    other = _sf()
    dom_ref = other.tad_domains(mats, model=_hmm(m_ref))
    for c in mats:
        np.testing.assert_array_equal(dom[c]["start"], dom_ref[c]["start"])
        np.testing.assert_array_equal(dom[c]["end"], dom_ref[c]["end"])
    # the insertion order of DI_all_train does not matter
    shuffled = {}
    for c in ["2", "1"]:
        keys = list(sf.DI_all_train[c])
        random.Random(3).shuffle(keys)
        shuffled[c] = {k: sf.DI_all_train[c][k] for k in keys}
    again = _sf()
    again.DI_all_train = shuffled
    again.modelTrain()
    for a, b in zip(_params(again.model), _params(sf.model)):
        assert np.array_equal(a, b)
    # updateParameter hands back its input pi, the model keeps the trained one
    A, B, pi = sf.init_parameter_state3()
    AA, BB, pi_out, model = sf.updateParameter(sf.DI_all_train, A, B, pi)
    assert pi_out is pi and BB.shape == (3, 3, 3) and AA.shape == (3, 3)
    assert not np.array_equal(model.pi, np.array(pi))
    np.testing.assert_array_equal(BB[:, 0], model.mean)
    np.testing.assert_array_equal(AA, model.A)
    bad = _sf(state_num=4)
    bad.DI_all_train = shuffled
    with pytest.raises(Exception, match="Only 3, 5, 6"):
        bad.modelTrain()


# -------------------------------------------------------------- 10. run_TADs
def test_run_tads_writes_the_four_files(tmp_path):
    from hichap_master_amd.StructureFind import StructureFind
    from tests.test_file_drivers_gpu import _cooler
    res = 40000
    path, _, _ = _cooler(tmp_path, res, ["chr1", "chr2"], [500, 320], seed=21)
    sf = StructureFind(path, res)
    with pytest.raises(NotImplementedError):
        sf.run_TADs(str(tmp_path / "never"))  # plot defaults to True, as in the reference
    assert not os.path.exists(tmp_path / "never")
    out = tmp_path / "TADs"
    sf.run_TADs(str(out) + "/", plot=False)

    def rows(kind):
        with open(out / f"TADs_{kind}_40K.txt") as f:
            return [ln.rstrip("\n").split("\t") for ln in f]

    def per_chrom(rws, conv):
        d = {}
        for r in rws:
            d.setdefault(r[0], []).append(conv(r[1]) if len(r) == 2 else tuple(conv(v) for v in r[1:]))
        return d

    di = per_chrom(rows("DI"), float)
    for c in ("chr1", "chr2"):
        np.testing.assert_allclose(di[c], sf.DI_dict[c], rtol=1e-11)
        assert per_chrom(rows("All_Boundary"), int).get(c, []) == list(sf.boundary_index[c]["boundary"])
        assert per_chrom(rows("Filtered_Boundary"), int).get(c, []) == list(sf.boundary_filtered[c])
        assert per_chrom(rows("Domain"), int).get(c, []) == list(zip(sf.Domain_dict[c]["start"],
                                                                     sf.Domain_dict[c]["end"]))
    assert sum(len(sf.Domain_dict[c]) for c in sf.Domain_dict) > 0
    assert sf.properU(1500000) == "1M500K" and sf.properU(2000000) == "2M" and sf.properU(5000) == "5K"
