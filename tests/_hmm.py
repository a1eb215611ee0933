"""Shared cases for the Baum-Welch tests: seeded models, ragged observation matrices and an
independent fp64 log-space forward-backward."""
from __future__ import annotations

import numpy as np

from avenir_amd.models import hmm_em as H


def model(S: int, O: int, seed: int, zero_symbol: bool = False):
    """Seeded fp32 (A, B, pi); with ``zero_symbol`` no state emits the last symbol, so a row that
    holds it is impossible under the model."""
    A, B, pi = H.random_start(S, O, seed)
    if zero_symbol and O > 1:
        B[:, -1] = 0.0
        B /= B.sum(1, keepdims=True)
    return A.astype(np.float32), B.astype(np.float32), pi.astype(np.float32)


def ragged_obs(N: int, T: int, O: int, seed: int, special: bool = True, symbols: int | None = None):
    """[N, T] int16 rows of random length (0..T) over the first ``symbols`` symbols; with
    ``special`` every eighth row is cut by an out-of-range token instead of -1 and every fifth
    row holds symbol O - 1 (impossible under a ``zero_symbol`` model)."""
    rng = np.random.default_rng(seed)
    hi = symbols or (O - 1 if special and O > 1 else O)
    obs = rng.integers(0, hi, (N, T)).astype(np.int16)
    lens = rng.integers(0, T + 1, N)
    if N > 2:
        lens[0], lens[-1] = T, T      # full rows at both ends of the batch
    for r in range(N):
        if lens[r] < T:
            obs[r, lens[r]:] = -1
            if special and r % 8 == 3:
                obs[r, lens[r]] = min(O + 3, 32767)
        if special and r % 5 == 2 and lens[r] > 0 and O > 1:
            obs[r, rng.integers(0, lens[r])] = O - 1
    return obs


def sample(A, B, pi, N: int, T: int, seed: int):
    """N sequences of length T drawn from the model."""
    rng = np.random.default_rng(seed)
    S, O = B.shape
    cA, cB = np.cumsum(A.astype(np.float64), 1), np.cumsum(B.astype(np.float64), 1)
    obs = np.zeros((N, T), np.int16)
    s = np.minimum(np.searchsorted(np.cumsum(pi.astype(np.float64)), rng.random(N)), S - 1)
    for t in range(T):
        u = rng.random(N)
        obs[:, t] = np.minimum((u[:, None] > cB[s]).sum(1), O - 1)
        u = rng.random(N)
        s = np.minimum((u[:, None] > cA[s]).sum(1), S - 1)
    return obs


def oracle(obs, A, B, pi):
    """fp64 log-space forward-backward, independent of the twin: (trans, emit, init expected
    counts, total log-likelihood, steps, sequences, empty, impossible)."""
    from scipy.special import logsumexp
    A, B, pi = (np.asarray(x, np.float64) for x in (A, B, pi))
    with np.errstate(divide="ignore"):
        lA, lB, lp = np.log(A), np.log(B), np.log(pi)
    S, O = B.shape
    trans, emit, init = np.zeros((S, S)), np.zeros((S, O)), np.zeros(S)
    ll = 0.0
    steps = seqs = empty = imp = 0
    for row in np.asarray(obs):
        L = 0
        while L < len(row) and 0 <= row[L] < O:
            L += 1
        if L == 0:
            empty += 1
            continue
        o = row[:L]
        la = np.zeros((L, S))
        la[0] = lp + lB[:, o[0]]
        for t in range(1, L):
            la[t] = logsumexp(la[t - 1][:, None] + lA, axis=0) + lB[:, o[t]]
        z = logsumexp(la[L - 1])
        if not np.isfinite(z):
            imp += 1
            continue
        lb = np.zeros((L, S))
        for t in range(L - 2, -1, -1):
            lb[t] = logsumexp(lA + (lB[:, o[t + 1]] + lb[t + 1])[None, :], axis=1)
        g = np.exp(la + lb - z)
        for t in range(L):
            emit[:, o[t]] += g[t]
        init += g[0]
        for t in range(1, L):
            trans += np.exp(la[t - 1][:, None] + lA + (lB[:, o[t]] + lb[t])[None, :] - z)
        ll += z
        steps += L
        seqs += 1
    return trans, emit, init, ll, steps, seqs, empty, imp


def count_bound(ref, T: int, S: int, n_steps: int):
    """Per-cell bound of the fixed-point tables against the fp64 counts: all-positive fp32 sums of
    S + 1 terms over T steps, plus the quantisation of n_steps contributions."""
    return 2 * T * (S + 4) * 2.0 ** -24 * np.maximum(ref, 1e-3) + n_steps * 2.0 ** -33


def ll_bound(n_steps: int, S: int) -> float:
    return 2 * n_steps * (S + 4) * 2.0 ** -24


def to_float(q):
    return np.asarray(q, np.int64).astype(np.float64) * 2.0 ** -H.COUNT_FRAC_BITS
