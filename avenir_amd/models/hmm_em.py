"""Baum-Welch (EM) training of discrete hidden Markov models: unsupervised from observation
sequences alone, or semi-supervised by refining a tagged / partially tagged estimate.

The E-step arithmetic is defined once, by :func:`hmm_estep_reference` (plain loops), and the HIP
kernel ``hmm_estep_kernel`` (csrc/kernels/hmm.hip) follows it operation for operation, so the two
agree bit for bit and no kernel-against-twin tolerance exists:

* probability space, fp32, every multiply and add rounded on its own (no fused multiply-add), no
  ``exp`` / ``log``;
* forward ``alpha_t(j) = (sum_i alpha_{t-1}(i) A[i][j]) B[j][o_t]``, the sum over i ascending from
  0; backward ``w(j) = B[j][o_{t+1}] beta_{t+1}(j)``, ``beta_t(i) = sum_j A[i][j] w(j)``, j ascending;
* after every step the vector is multiplied by ``2^-e``, e the binary exponent (``frexp``) of its
  largest element; the exponents are carried as integers, so scaling is exact and no sequence
  length underflows;
* ``Z = sum_i alpha_{L-1}(i)`` (i ascending), one IEEE division ``r = 1 / Z`` per sequence;
  posteriors are products with ``r`` shifted by the integer exponent difference (``ldexp``);
* every posterior is converted on its own to ``2^-COUNT_FRAC_BITS`` fixed point (round to nearest
  even) and added as a 64-bit integer: the three tables are exact, order-free sums, equal for every
  grid, chunking, order of atomics and number of ranks;
* a negative or out-of-range observation ends a sequence (an invalid first one makes it empty); a
  sequence whose vector maximum becomes 0 is impossible under the model and contributes nothing;
* per sequence the scaled normaliser ``Z`` (float32) and the summed exponent ``E`` (int32) are
  kept; its log-likelihood ``log(Z) + E ln 2`` is evaluated by :func:`loglik_fixed` in numpy fp64
  and rounded to ``2^-LL_FRAC_BITS`` fixed point, so the total, and with it the stopping decision,
  is an integer sum as well.

Subnormals: the gfx950 build runs the kernel in the compiler's default float mode
(``float_denorm_mode_32 = 3`` in the code object: fp32 subnormals are kept, inputs and results), and
numpy on the host keeps them too, so the twin needs no flush and follows the kernel as it is.

The M-step (:func:`hmm_mstep`) is one numpy fp64 function on the host for both devices; its result
is stored as the fp32 values the next E-step reads, so a device fit and a host fit walk the same
models bit for bit.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

COUNT_FRAC_BITS = 32            # expected counts: units of 2^-32
LL_FRAC_BITS = 24               # log-likelihoods: units of 2^-24 (|ll| per step < 2^7, steps < 2^31)
MAX_DEVICE_STATES = 64          # larger models take the twin
MAX_SYMBOLS = 32767             # int16 observations
MAX_STEPS = 1 << 31             # observation steps per call: no table cell can overflow int64
# Kept forward vectors of one launch, T * (S + 1) * 4 bytes per row.  Measured
# (profiles/hmm_em_bench.jsonl, "caps"): fewer, larger launches win as long as each one fills the
# chip, and nothing is gained by keeping a chunk inside the Infinity Cache; 1 GiB runs 2^14 rows of
# 256 steps x 32 states in one launch and 2^20 rows of 64 x 8 in three.  Chunking cannot change a
# result.
DEFAULT_WORKSPACE_BYTES = 1 << 30
STAT_NAMES = ("sequences", "steps", "empty", "impossible")

_F32 = np.float32


def _tables(A, B, pi):
    f = lambda x: np.ascontiguousarray((x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)),
                                       dtype=_F32)
    A, B, pi = f(A), f(B), f(pi).reshape(-1)
    S = A.shape[0]
    if A.shape != (S, S) or B.ndim != 2 or B.shape[0] != S or pi.shape != (S,) or S < 1 or B.shape[1] < 1:
        raise ValueError("hmm_estep: A must be [S, S], B [S, O] and pi [S]")
    return A, B, pi


def _obs_array(obs) -> np.ndarray:
    o = obs.detach().cpu().numpy() if isinstance(obs, torch.Tensor) else np.asarray(obs)
    if o.ndim != 2:
        raise ValueError("hmm_estep: obs must be [N, T]")
    return o


def _quant(x: np.ndarray, d) -> np.ndarray:
    """x * 2^d rounded to the nearest even integer (x >= 0 fp32; exact: an fp32 value times a power
    of two is an integer or rounds once)."""
    return np.rint(np.ldexp(x, np.clip(d, -400, 400).astype(np.int32))).astype(np.int64)


def _bin_exp(m) -> int:
    return int(np.frexp(m)[1]) if m > 0 else 0


def loglik_fixed(Z, E) -> int:
    """Sum over sequences of ``log(Z) + E ln 2`` (numpy fp64), each rounded to 2^-LL_FRAC_BITS
    fixed point; rows with Z = 0 (empty or impossible) add nothing.  The one evaluation shared by
    twin and kernel, every chunking and every world size."""
    z = (Z.detach().cpu().numpy() if isinstance(Z, torch.Tensor) else np.asarray(Z)).astype(np.float64)
    e = (E.detach().cpu().numpy() if isinstance(E, torch.Tensor) else np.asarray(E)).astype(np.float64)
    ok = z > 0
    ll = np.log(z[ok]) + e[ok] * np.log(2.0)
    return int(np.rint(ll * float(1 << LL_FRAC_BITS)).astype(np.int64).sum())


# ================================================================================================
# the definition
# ================================================================================================
def hmm_estep_reference(obs, A, B, pi):
    """The E-step, written as its definition: ``(trans_q [S, S], emit_q [S, O], init_q [S]`` int64
    fixed point, ``Z [N]`` float32, ``E [N]`` int32, ``stats [4]`` int64 (STAT_NAMES)``)``."""
    obs = _obs_array(obs)
    A, B, pi = _tables(A, B, pi)
    N, T = obs.shape
    S, O = B.shape
    trans_q = np.zeros((S, S), np.int64)
    emit_q = np.zeros((S, O), np.int64)
    init_q = np.zeros(S, np.int64)
    Z = np.zeros(N, _F32)
    E = np.zeros(N, np.int32)
    stats = np.zeros(4, np.int64)
    for r in range(N):
        o = obs[r]
        L = 0
        while L < T and 0 <= o[L] < O:
            L += 1
        if L == 0:
            stats[2] += 1
            continue
        # forward
        alpha = np.zeros((L, S), _F32)
        cexp = np.zeros(L, np.int64)
        possible = True
        for t in range(L):
            if t == 0:
                acc = pi
            else:
                acc = np.zeros(S, _F32)
                for i in range(S):
                    acc = acc + alpha[t - 1, i] * A[i, :]
            a = acc * B[:, o[t]]
            m = a.max()
            if not m > 0:
                possible = False
                break
            e = _bin_exp(m)
            alpha[t] = np.ldexp(a, -e)
            cexp[t] = (cexp[t - 1] if t else 0) + e
        if not possible:
            stats[3] += 1
            continue
        z = _F32(0)
        for i in range(S):
            z = z + alpha[L - 1, i]
        rinv = _F32(1) / z
        Etot = int(cexp[L - 1])
        Z[r], E[r] = z, Etot
        stats[0] += 1
        stats[1] += L
        # backward, with the posteriors of every step
        beta = np.ones(S, _F32)
        bexp = 0
        for t in range(L - 1, -1, -1):
            if t < L - 1:
                w = B[:, o[t + 1]] * beta
                d = int(cexp[t]) + bexp - Etot + COUNT_FRAC_BITS
                for i in range(S):
                    xi = ((alpha[t, i] * A[i, :]) * w) * rinv
                    trans_q[i] += _quant(xi, np.int64(d))
                nb = np.zeros(S, _F32)
                for j in range(S):
                    nb = nb + A[:, j] * w[j]
                e = _bin_exp(nb.max())
                beta = np.ldexp(nb, -e)
                bexp += e
            g = _quant((alpha[t] * beta) * rinv, np.int64(int(cexp[t]) + bexp - Etot + COUNT_FRAC_BITS))
            emit_q[:, o[t]] += g
            if t == 0:
                init_q += g
    return trans_q, emit_q, init_q, Z, E, stats


# ================================================================================================
# the same arithmetic, vectorised over the rows (the CPU path)
# ================================================================================================
def hmm_estep_numpy(obs, A, B, pi):
    """:func:`hmm_estep_reference` with the row loop vectorised; every element goes through the
    same operations in the same order, so the outputs are identical bit for bit."""
    obs = _obs_array(obs)
    A, B, pi = _tables(A, B, pi)
    N, T = obs.shape
    S, O = B.shape
    valid = (obs >= 0) & (obs < O)
    L = np.cumprod(valid, axis=1).sum(1).astype(np.int64) if T else np.zeros(N, np.int64)
    trans_q = np.zeros((S, S), np.int64)
    emit_qT = np.zeros((O, S), np.int64)
    init_q = np.zeros(S, np.int64)
    Z = np.zeros(N, _F32)
    E = np.zeros(N, np.int32)
    alive = L > 0
    Tm = int(L.max()) if N else 0
    alpha = np.zeros((Tm, N, S), _F32)
    cexp = np.zeros((Tm, N), np.int64)
    BT = np.ascontiguousarray(B.T)
    for t in range(Tm):
        idx = np.nonzero(alive & (L > t))[0]
        if idx.size == 0:
            break
        if t == 0:
            acc = np.broadcast_to(pi, (idx.size, S))
        else:
            prev = alpha[t - 1, idx]
            acc = np.zeros((idx.size, S), _F32)
            for i in range(S):
                acc = acc + prev[:, i:i + 1] * A[i][None, :]
        a = acc * BT[obs[idx, t]]
        m = a.max(1)
        bad = ~(m > 0)
        alive[idx[bad]] = False
        e = np.where(bad, 0, np.frexp(m)[1]).astype(np.int64)
        alpha[t, idx] = np.ldexp(a, (-e)[:, None].astype(np.int32))
        cexp[t, idx] = (cexp[t - 1, idx] if t else 0) + e
    good = np.nonzero(alive)[0]
    stats = np.array([good.size, int(L[good].sum()), int((L == 0).sum()), int(((L > 0) & ~alive).sum())], np.int64)
    if good.size:
        last = alpha[L[good] - 1, good]
        z = np.zeros(good.size, _F32)
        for i in range(S):
            z = z + last[:, i]
        Z[good] = z
        E[good] = cexp[L[good] - 1, good]
    rinv_all = np.zeros(N, _F32)
    rinv_all[good] = _F32(1) / Z[good]
    Eall = E.astype(np.int64)
    beta = np.zeros((N, S), _F32)
    bexp = np.zeros(N, np.int64)
    for t in range(Tm - 1, -1, -1):
        endi = np.nonzero(alive & (L - 1 == t))[0]
        stepi = np.nonzero(alive & (L - 1 > t))[0]
        if stepi.size:
            w = BT[obs[stepi, t + 1]] * beta[stepi]
            rinv = rinv_all[stepi][:, None]
            d = (cexp[t, stepi] + bexp[stepi] - Eall[stepi] + COUNT_FRAC_BITS)[:, None]
            at = alpha[t, stepi]
            for i in range(S):
                xi = ((at[:, i:i + 1] * A[i][None, :]) * w) * rinv
                trans_q[i] += _quant(xi, d).sum(0)
            nb = np.zeros((stepi.size, S), _F32)
            for j in range(S):
                nb = nb + A[:, j][None, :] * w[:, j:j + 1]
            e = np.frexp(nb.max(1))[1].astype(np.int64)     # frexp(0) has exponent 0
            beta[stepi] = np.ldexp(nb, (-e)[:, None].astype(np.int32))
            bexp[stepi] += e
        if endi.size:
            beta[endi] = 1
            bexp[endi] = 0
        idx = np.concatenate([stepi, endi])
        if idx.size:
            g = _quant((alpha[t, idx] * beta[idx]) * rinv_all[idx][:, None],
                       (cexp[t, idx] + bexp[idx] - Eall[idx] + COUNT_FRAC_BITS)[:, None])
            np.add.at(emit_qT, obs[idx, t], g)
            if t == 0:
                init_q += g.sum(0)
    return trans_q, np.ascontiguousarray(emit_qT.T), init_q, Z, E, stats


# ================================================================================================
# launcher
# ================================================================================================
def hmm_estep(obs: torch.Tensor, A, B, pi, workspace_bytes: int | None = None):
    """One E-step over ``obs`` [N, T] int16: ``(trans_q, emit_q, init_q`` int64, ``Z`` float32 [N],
    ``E`` int32 [N], ``stats`` int64 [4]) as tensors on the device of ``obs``.  Device tensors go
    to ``hmm_estep_kernel`` in chunks of rows whose kept forward vectors stay under
    ``workspace_bytes`` (default DEFAULT_WORKSPACE_BYTES); CPU tensors, more than
    MAX_DEVICE_STATES states and more than MAX_SYMBOLS symbols take the numpy twin."""
    if obs.dim() != 2:
        raise ValueError("hmm_estep: obs must be [N, T]")
    N, T = obs.shape
    if N * T >= MAX_STEPS:
        raise ValueError("hmm_estep: N * T must stay below 2^31 observation steps per call")
    dev = obs.device
    t32 = lambda x: torch.as_tensor(x).to(dtype=torch.float32).contiguous()
    A, B, pi = t32(A), t32(B), t32(pi).reshape(-1)
    S, O = A.shape[0], (B.shape[1] if B.dim() == 2 else 0)
    if A.shape != (S, S) or B.dim() != 2 or B.shape[0] != S or pi.numel() != S or S < 1 or O < 1:
        raise ValueError("hmm_estep: A must be [S, S], B [S, O] and pi [S]")
    if dev.type != "cuda" or S > MAX_DEVICE_STATES or O > MAX_SYMBOLS:
        out = hmm_estep_numpy(obs, A, B, pi)
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in out)
    from .. import _native
    C = _native.C()
    obs = obs.to(torch.int16).contiguous()
    A, B, pi = A.to(dev), B.to(dev), pi.to(dev)
    trans = torch.zeros((S, S), dtype=torch.int64, device=dev)
    emit = torch.zeros((S, O), dtype=torch.int64, device=dev)
    init = torch.zeros(S, dtype=torch.int64, device=dev)
    stats = torch.zeros(4, dtype=torch.int64, device=dev)
    Z = torch.zeros(N, dtype=torch.float32, device=dev)
    E = torch.zeros(N, dtype=torch.int32, device=dev)
    if N == 0 or T == 0:
        stats[2] = N
        return trans, emit, init, Z, E, stats
    per_row = T * (S + 1)
    cap = DEFAULT_WORKSPACE_BYTES if workspace_bytes is None else int(workspace_bytes)
    rows = int(min(N, max(1, cap // (4 * per_row))))
    ws = torch.empty(rows * per_row, dtype=torch.float32, device=dev)
    for lo in range(0, N, rows):
        hi = min(N, lo + rows)
        C.hmm_estep(obs[lo:hi], A, B, pi, trans, emit, init, Z[lo:hi], E[lo:hi], stats, ws)
    return trans, emit, init, Z, E, stats


# ================================================================================================
# M-step and the fit
# ================================================================================================
def normalised_rows(q, prev, prior: float = 0.0) -> np.ndarray:
    """fp64 rows ``(count + prior) / sum``; a row whose counts total 0 (a state never visited)
    keeps ``prev``."""
    q = np.asarray(q, np.int64)
    prev = np.asarray(prev, np.float64).reshape(q.shape)
    c = q.astype(np.float64) * 2.0 ** -COUNT_FRAC_BITS + float(prior)
    tot = c.sum(-1, keepdims=True)
    seen = q.sum(-1, keepdims=True) > 0
    return np.where(seen, c / np.where(seen, tot, 1.0), prev)


def hmm_mstep(trans_q, emit_q, init_q, prev, prior: float = 0.0):
    """New ``(A, B, pi)`` from the fixed-point tables, in numpy fp64 on the host, stored as the
    float32 values the next E-step reads.  ``prev`` is the ``(A, B, pi)`` that produced the tables."""
    n = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    A0, B0, p0 = (n(x) for x in prev)
    A = normalised_rows(n(trans_q), A0, prior).astype(_F32)
    B = normalised_rows(n(emit_q), B0, prior).astype(_F32)
    pi = normalised_rows(n(init_q).reshape(1, -1), p0.reshape(1, -1), prior)[0].astype(_F32)
    return A, B, pi


@dataclass(frozen=True)
class HmmFit:
    model: object                 # HiddenMarkovModel (A, B, pi float64 copies of the fp32 tables)
    log_likelihood: tuple         # one float per tested iteration: the corpus total under the
    #                               model that ENTERED that iteration
    iterations: int
    converged: bool
    stats: dict                   # STAT_NAMES of the last E-step, summed over ranks


def random_start(S: int, O: int, seed: int):
    """Rows of normalised ``1 + U(0, 1)`` in fp64 from ``seed`` alone (host generator)."""
    rng = np.random.default_rng(int(seed))
    row = lambda *shape: (lambda x: x / x.sum(-1, keepdims=True))(1.0 + rng.random(shape))
    return row(S, S), row(S, O), row(S)


def fit_unsupervised(obs: torch.Tensor, states: list[str], observations: list[str], init=None, iters: int = 50,
                     tol: float | None = 1e-4, check_every: int = 1, prior: float = 0.0, seed: int = 0,
                     comm=None, workspace_bytes: int | None = None) -> HmmFit:
    """Baum-Welch over this rank's rows of ``obs``; see HiddenMarkovModelBuilder.fit_unsupervised."""
    from ..parallel.comm import get_comm
    from .markov import HiddenMarkovModel
    S, O = len(states), len(observations)
    if init is not None:
        if len(init.states) != S or len(init.observations) != O:
            raise ValueError("fit_unsupervised: init has other states / observations than the builder")
        start = tuple(x.detach().cpu().numpy().astype(np.float64) for x in (init.A, init.B, init.pi))
    else:
        start = random_start(S, O, seed)
    for x in start:
        if not np.all(np.isfinite(x)) or (x < 0).any():
            raise ValueError("fit_unsupervised: the start model must be finite and non-negative")
    A, B, pi = (np.ascontiguousarray(x, dtype=_F32) for x in start)
    comm = comm or get_comm()
    hist: list[float] = []
    prev_total = None
    converged = False
    stats = dict.fromkeys(STAT_NAMES, 0)
    done = 0
    nt, ne = S * S, S * O
    for it in range(1, int(iters) + 1):
        trans, emit, ini, Z, E, st = hmm_estep(obs, A, B, pi, workspace_bytes=workspace_bytes)
        test = tol is not None and (it % max(1, int(check_every)) == 0 or it == iters)
        ll = torch.tensor([loglik_fixed(Z, E) if test else 0], dtype=torch.int64, device=trans.device)
        pack = torch.cat([trans.reshape(-1), emit.reshape(-1), ini.reshape(-1), st.reshape(-1), ll])
        if comm.is_distributed:
            comm.all_reduce(pack)
        pack = pack.cpu().numpy()       # the one device-to-host copy of the iteration
        A, B, pi = hmm_mstep(pack[:nt].reshape(S, S), pack[nt:nt + ne].reshape(S, O), pack[nt + ne:nt + ne + S],
                             (A, B, pi), prior)
        stats = {k: int(v) for k, v in zip(STAT_NAMES, pack[nt + ne + S:nt + ne + S + 4])}
        done = it
        if test:
            total = int(pack[-1])
            hist.append(total * 2.0 ** -LL_FRAC_BITS)
            if prev_total is not None and total - prev_total < tol * abs(total):
                converged = True
                break
            prev_total = total
    t64 = lambda x: torch.from_numpy(np.asarray(x, np.float64).copy())
    model = HiddenMarkovModel(list(states), list(observations), t64(A), t64(B), t64(pi))
    return HmmFit(model, tuple(hist), done, converged, stats)


def posterior_counts(model, obs: torch.Tensor):
    """Expected ``(transition [S, S], emission [S, O], initial [S])`` counts of ``obs`` under
    ``model`` as float64 tensors on the device of ``obs``."""
    tq, eq, iq, _, _, _ = hmm_estep(obs, model.A, model.B, model.pi)
    return tuple(x.double() * 2.0 ** -COUNT_FRAC_BITS for x in (tq, eq, iq))
