"""The NumPy reference of the Baum-Welch training (tests/hmm_train_ref.py)
pinned without a GPU: one EM step against the M-step built from exact
posteriors (all S^n state paths enumerated), and the single-Gaussian closed
form."""
import numpy as np
import pytest

from tests import hmm_train_ref as ref
from tests.test_tads import _random_model


def mstep_from_posteriors(seqs, post, model, var_floor=1e-4):
    """The M-step written from its definition on exact gamma / xi / gamma_im
    (two-pass variance around the NEW mean)."""
    A, pi, mean, var, weight = ref.copy_model(model)
    S, M = mean.shape
    g1 = sum(p[0][0] for p in post)
    xi = sum(p[1].sum(axis=0) for p in post)
    gex = sum(p[0][:-1].sum(axis=0) for p in post)
    gall = sum(p[0].sum(axis=0) for p in post)
    s0 = sum(p[2].sum(axis=0) for p in post)
    sx = sum((p[2] * np.asarray(x)[:, None, None]).sum(axis=0) for x, p in zip(seqs, post))
    pi = g1 / len(seqs)
    for i in range(S):
        if gex[i] > 0:
            A[i] = xi[i] / gex[i]
        for m in range(M):
            if gall[i] > 0:
                weight[i, m] = s0[i, m] / gall[i]
            if s0[i, m] > 0:
                mean[i, m] = sx[i, m] / s0[i, m]
                v = sum((p[2][:, i, m] * (np.asarray(x) - mean[i, m]) ** 2).sum() for x, p in zip(seqs, post))
                var[i, m] = max(v / s0[i, m], var_floor)
    return A, pi, mean, var, weight


def enumeration_case(S, seed):
    """Random model with zero transitions and sequences of n = 1, 2, 5, 6."""
    rng = np.random.default_rng(700 + 10 * S + seed)
    model = _random_model(rng, S, 2, zero_frac=0.4)
    while not np.any(model[0] == 0.0):
        model = _random_model(rng, S, 2, zero_frac=0.4)
    seqs = [rng.normal(0, 6, n) for n in (1, 2, 5, 6)]
    return model, seqs


@pytest.mark.parametrize("S", [2, 3])
@pytest.mark.parametrize("seed", range(3))
def test_step_equals_enumeration(S, seed):
    model, seqs = enumeration_case(S, seed)
    assert np.any(model[0] == 0.0)
    post = [ref.enumerate_posteriors(x, model) for x in seqs]
    want = mstep_from_posteriors(seqs, post, model)
    got, logp, floored = ref.step(seqs, model)
    assert floored == 0
    np.testing.assert_allclose(logp, sum(p[3] for p in post), rtol=1e-12)
    xmax = max(np.max(np.abs(x)) for x in seqs)  # a mean may sit near zero: atol beside the rtol
    for g, w, name in zip(got, want, ("A", "pi", "mean", "var", "weight")):
        np.testing.assert_allclose(g, w, rtol=1e-12, atol=1e-12 * xmax if name == "mean" else 0, err_msg=name)
    assert np.array_equal(got[0] == 0.0, model[0] == 0.0)


def test_single_gaussian_closed_form():
    rng = np.random.default_rng(11)
    seqs = [rng.normal(2.0, 3.0, n) for n in (1, 2, 70)]
    model = (np.array([[1.0]]), np.array([1.0]), np.array([[0.5]]), np.array([[4.0]]), np.array([[1.0]]))
    (A, pi, mean, var, weight), logp, _ = ref.step(seqs, model)
    allx = np.concatenate(seqs)
    np.testing.assert_array_equal(A, [[1.0]])
    np.testing.assert_array_equal(pi, [1.0])
    np.testing.assert_allclose(weight, [[1.0]], rtol=1e-12)
    np.testing.assert_allclose(mean, [[allx.mean()]], rtol=1e-12)
    np.testing.assert_allclose(var, [[allx.var()]], rtol=1e-12)
    np.testing.assert_allclose(logp, np.sum(-0.5 * np.log(2 * np.pi * 4.0) - 0.5 * (allx - 0.5) ** 2 / 4.0), rtol=1e-12)


def test_training_raises_the_likelihood_and_stops():
    rng = np.random.default_rng(3)
    seqs = [np.concatenate([rng.normal(m, 1.5, 12) for m in (5, 0, -5)]) for _ in range(6)]
    model = (np.array([[0.85, 0.15, 0.0], [0.05, 0.8, 0.15], [0.19, 0.01, 0.8]]), np.array([0.4, 0.3, 0.3]),
             np.array([[3.0, 6, 9], [-3, 0, 3], [-6, -3, 0]]), np.full((3, 3), 3.0), np.full((3, 3), 1 / 3))
    trained, iters, trace, status = ref.train(seqs, model)
    assert 2 <= iters < 500 and status & ref.MAX_ITER == 0 and status & ref.LOGP_DROPPED == 0
    assert np.all(np.diff(trace) >= -1e-9 * np.abs(trace[1:]))
    assert trained[0][0, 2] == 0.0
    _, _, _, st1 = ref.train(seqs, model, max_iter=1)
    assert st1 & ref.MAX_ITER
