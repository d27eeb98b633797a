"""NumPy restatement of the Baum-Welch training of the Gaussian-mixture TAD
HMM (the HIP path is hichap_master_amd/csrc/hmm_train.hip),
and exact posteriors by enumeration of every state path for tiny sequences.

A model is the tuple ``(A, pi, mean, var, weight)``: A (S, S), pi (S,),
mean / var / weight (S, M), as ``GaussianMixtureHMM`` holds them.  Nothing
here is tuned to the HIP code: ``estep`` follows the scaled recursions as
written in the definition, ``enumerate_posteriors`` sums the joint
probability of all S^n paths directly.
"""
import itertools

import numpy as np

MAX_ITER, LOGP_DROPPED, VAR_FLOORED = 1, 2, 4


def copy_model(model):
    return tuple(np.array(p, dtype=np.float64, copy=True) for p in model)


def emissions(x, mean, var, weight):
    """(e, shift): e[t, i, m] = w_im N(x_t; mu_im, v_im) / exp(shift_t), shift_t
    the largest log term of observation t."""
    x = np.asarray(x, np.float64)
    with np.errstate(divide="ignore"):
        lw = np.where(weight > 0, np.log(np.where(weight > 0, weight, 1.0)), -np.inf)
    lt = lw - 0.5 * np.log(2.0 * np.pi * var) - 0.5 * (x[:, None, None] - mean) ** 2 / var
    shift = lt.max(axis=(1, 2))
    return np.exp(lt - shift[:, None, None]), shift


def estep(seqs, model):
    """Sufficient statistics of all sequences and their log likelihood."""
    A, pi, mean, var, weight = model
    S, M = mean.shape
    st = {"xi": np.zeros((S, S)), "gex": np.zeros(S), "gall": np.zeros(S), "g1": np.zeros(S),
          "s0": np.zeros((S, M)), "s1": np.zeros((S, M)), "s2": np.zeros((S, M)), "K": len(seqs)}
    logp = 0.0
    for x in seqs:
        x = np.asarray(x, np.float64)
        n = x.size
        if n < 1:
            raise ValueError("empty sequence")
        e, shift = emissions(x, mean, var, weight)
        b = e.sum(axis=2)
        alpha = np.empty((n, S))
        c = np.empty(n)
        u = pi * b[0]
        for t in range(n):
            if t:
                u = (alpha[t - 1] @ A) * b[t]
            c[t] = u.sum()
            if not c[t] > 0.0:
                raise ValueError("sequence has zero likelihood under the model")
            alpha[t] = u / c[t]
        beta = np.ones((n, S))
        for t in range(n - 2, -1, -1):
            v = b[t + 1] * beta[t + 1] / c[t + 1]
            beta[t] = A @ v
            st["xi"] += alpha[t][:, None] * A * v[None, :]
        gamma = alpha * beta
        logp += float(np.sum(np.log(c) + shift))
        st["g1"] += gamma[0]
        st["gex"] += gamma[:-1].sum(axis=0)
        st["gall"] += gamma.sum(axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            gim = np.where(b[:, :, None] > 0, gamma[:, :, None] * e / b[:, :, None], 0.0)
        d = x[:, None, None] - mean
        st["s0"] += gim.sum(axis=0)
        st["s1"] += (gim * d).sum(axis=0)
        st["s2"] += (gim * d * d).sum(axis=0)
    return st, logp


def mstep(st, model, var_floor=1e-4, raw=None):
    """New model from the statistics; a re-estimate whose denominator is 0
    keeps its old value.  Returns (model, number of floored variances); a list
    passed as ``raw`` collects every variance estimate before the floor."""
    A, pi, mean, var, weight = copy_model(model)
    S, M = mean.shape
    floored = 0
    pi = st["g1"] / st["K"]
    for i in range(S):
        if st["gex"][i] > 0:
            A[i] = st["xi"][i] / st["gex"][i]
        for m in range(M):
            if st["gall"][i] > 0:
                weight[i, m] = st["s0"][i, m] / st["gall"][i]
            s0 = st["s0"][i, m]
            if s0 > 0:
                dm = st["s1"][i, m] / s0
                mean[i, m] += dm
                v = st["s2"][i, m] / s0 - dm * dm
                if raw is not None:
                    raw.append(v)
                if not v >= var_floor:
                    v, floored = var_floor, floored + 1
                var[i, m] = v
    return (A, pi, mean, var, weight), floored


def step(seqs, model, var_floor=1e-4, raw=None):
    """One EM iteration: (new model, log P under the input model, floored)."""
    st, logp = estep(seqs, copy_model(model))
    new, floored = mstep(st, model, var_floor, raw)
    return new, logp, floored


def train(seqs, model, max_iter=500, eps=1e-4, var_floor=1e-4, raw=None):
    """The training loop: iteration k records L_k (under the parameters
    entering it), applies its M-step, and stops the run when k >= 1 and
    0 <= L_k - L_{k-1} < eps |L_k|.  Returns (model, iters, trace, status)."""
    model = copy_model(model)
    trace, status = [], MAX_ITER
    for k in range(max_iter):
        model, logp, floored = step(seqs, model, var_floor, raw)
        trace.append(logp)
        if floored:
            status |= VAR_FLOORED
        if k >= 1:
            d = logp - trace[k - 1]
            if d < -1e-9 * abs(logp):
                status |= LOGP_DROPPED
            if 0.0 <= d < eps * abs(logp):
                status &= ~MAX_ITER
                break
    return model, len(trace), np.array(trace), status


def train_three_pass(seqs, model, **kw):
    """modelTrain's rule (StructureFind.py:1106-1108): three training runs,
    each restarting from the FIRST model's pi (updateParameter returns its
    input pi).  Returns (model of the third run, [iters], status bits)."""
    pi0 = np.array(model[1], dtype=np.float64)
    cur, iters, status = copy_model(model), [], 0
    for _ in range(3):
        start = (cur[0], pi0.copy(), cur[2], cur[3], cur[4])
        cur, it, _, st = train(seqs, start, **kw)
        iters.append(it)
        status |= st
    return cur, iters, status


def enumerate_posteriors(x, model):
    """Exact gamma (n, S), xi (n - 1, S, S), gamma_im (n, S, M) and log P of
    one short sequence, by summing the joint density over all S^n paths."""
    A, pi, mean, var, weight = (np.asarray(p, np.float64) for p in model)
    x = np.asarray(x, np.float64)
    n, (S, M) = x.size, mean.shape
    dens = weight * np.exp(-0.5 * (x[:, None, None] - mean) ** 2 / var) / np.sqrt(2.0 * np.pi * var)  # (n, S, M)
    b = dens.sum(axis=2)
    gamma = np.zeros((n, S))
    xi = np.zeros((max(n - 1, 0), S, S))
    total = 0.0
    for path in itertools.product(range(S), repeat=n):
        p = pi[path[0]] * b[0, path[0]]
        for t in range(1, n):
            p *= A[path[t - 1], path[t]] * b[t, path[t]]
        total += p
        for t in range(n):
            gamma[t, path[t]] += p
        for t in range(n - 1):
            xi[t, path[t], path[t + 1]] += p
    gamma /= total
    xi /= total
    with np.errstate(invalid="ignore", divide="ignore"):
        gim = np.where(b[:, :, None] > 0, gamma[:, :, None] * dens / b[:, :, None], 0.0)
    return gamma, xi, gim, float(np.log(total))
