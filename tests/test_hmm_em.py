"""Baum-Welch training (models/hmm_em.py): the twin against an independent fp64 forward-backward,
its exact invariants, the M-step rules, EM monotonicity, world sizes, the job and a golden replay."""
from pathlib import Path

import numpy as np
import pytest
import torch

from avenir_amd.models import hmm_em as H
from avenir_amd.models.markov import HiddenMarkovModel, HiddenMarkovModelBuilder

import _hmm
from _dist import run_world

NAMES = ("trans_q", "emit_q", "init_q", "Z", "E", "stats")
SHAPES = [(3, 5, 12, 40), (8, 16, 64, 64), (32, 20, 200, 8), (64, 7, 40, 6)]      # S, O, T, N
GOLDEN = Path(__file__).parent / "golden" / "hmm_em" / "hmm_em.npz"


def _same(a, b):
    for n, x, y in zip(NAMES, a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), n


def _total_ll(out) -> float:
    return H.loglik_fixed(out[3], out[4]) * 2.0 ** -H.LL_FRAC_BITS


@pytest.fixture(scope="module")
def cases():
    """(obs, model, twin outputs, oracle) per shape: computed once, read by several tests."""
    out = {}
    for S, O, T, N in SHAPES:
        A, B, pi = _hmm.model(S, O, seed=S)
        obs = _hmm.ragged_obs(N, T, O, seed=T, special=False)
        obs.setflags(write=False)
        out[S] = (obs, (A, B, pi), H.hmm_estep_numpy(obs, A, B, pi), _hmm.oracle(obs, A, B, pi))
    return out


@pytest.mark.parametrize("S,O,T,N", SHAPES)
def test_twin_against_fp64_log_space(cases, S, O, T, N):
    obs, _, got, ref = cases[S]
    n_steps = int(got[5][1])
    assert (n_steps, int(got[5][0]), int(got[5][2]), int(got[5][3])) == ref[4:]
    for name, q, r in zip(NAMES, got[:3], ref[:3]):
        err = np.abs(_hmm.to_float(q) - r)
        bound = _hmm.count_bound(r, T, S, n_steps)
        print(f"{name} S={S}: worst error / bound {float((err / bound).max()):.3g}")
        assert (err <= bound).all(), name
    print(f"log-likelihood S={S}: error {abs(_total_ll(got) - ref[3]):.3g}, bound {_hmm.ll_bound(n_steps, S):.3g}")
    assert abs(_total_ll(got) - ref[3]) <= _hmm.ll_bound(n_steps, S)


@pytest.mark.parametrize("S,O,T,N", SHAPES[:2] + [(33, 4, 9, 5)])
def test_fast_twin_is_the_plain_twin(S, O, T, N):
    A, B, pi = _hmm.model(S, O, seed=S + 1, zero_symbol=True)
    obs = _hmm.ragged_obs(N, T, O, seed=S)
    ref = H.hmm_estep_reference(obs, A, B, pi)
    _same(H.hmm_estep_numpy(obs, A, B, pi), ref)
    assert ref[5][3] > 0 or N < 5           # impossible rows were among them
    out = H.hmm_estep(torch.from_numpy(obs), A, B, pi)     # the launcher's CPU path: same names, dtypes
    assert [x.dtype for x in out] == [torch.int64] * 3 + [torch.float32, torch.int32, torch.int64]
    _same([x.numpy() for x in out], ref)


def test_exact_invariants(cases):
    obs, (A, B, pi), got, _ = cases[8]
    perm = np.random.default_rng(0).permutation(len(obs))
    shuffled = H.hmm_estep_numpy(obs[perm], A, B, pi)
    for n, x, y in zip(NAMES, got, shuffled):
        assert np.array_equal(x[perm] if n in ("Z", "E") else x, y), n
    # a row ended by -1 or by an out-of-range token equals the explicitly shorter row
    row = np.arange(20, dtype=np.int16).reshape(1, 20) % 16
    short = H.hmm_estep_numpy(row[:, :11], A, B, pi)
    for stop in (-1, 16, 32767, -32768):
        cut = row.copy()
        cut[0, 11] = stop
        _same(H.hmm_estep_numpy(cut, A, B, pi), short)
    empty = row.copy()
    empty[0, 0] = -1
    st = H.hmm_estep_numpy(empty, A, B, pi)[5]
    assert st.tolist() == [0, 0, 1, 0]
    # every sequence starts once, and a state's occupancy splits into its outgoing pairs and its
    # last-step posteriors (which sum to 1 per sequence): within the rounding of the posteriors
    # and the quantisation of the terms involved, not exactly
    n_seq, n_steps = int(got[5][0]), int(got[5][1])
    S, T = A.shape[0], obs.shape[1]
    fp = 2 * T * (S + 4) * 2.0 ** -24
    assert abs(_hmm.to_float(got[2]).sum() - n_seq) <= fp * n_seq + n_seq * S * 2.0 ** -33
    last = _hmm.to_float(got[1]).sum(1) - _hmm.to_float(got[0]).sum(1)
    assert abs(last.sum() - n_seq) <= fp * n_steps + n_steps * (S * S + S) * 2.0 ** -33
    assert (last >= -(fp * n_steps + n_steps * (S + 1) * 2.0 ** -33)).all()
    assert got[5][0] == len(obs) - got[5][2] - got[5][3]


def test_rescaling_keeps_long_products_finite():
    A = np.array([[0.7, 0.3], [0.4, 0.6]], np.float32)
    B = np.array([[0.2, 0.1], [0.15, 0.2]], np.float32)      # <= 0.2: the product of 400 underflows fp32
    pi = np.array([0.5, 0.5], np.float32)
    T = 400
    obs = _hmm.ragged_obs(6, T, 2, seed=5, special=False)
    obs[0] = np.resize(np.array([0, 1, 1], np.int16), T)
    got = H.hmm_estep_numpy(obs, A, B, pi)
    ref = _hmm.oracle(obs, A, B, pi)
    assert np.float32(0.2) ** 150 == 0 and got[4].min() < -700 and np.isfinite(got[3]).all()
    n_steps = int(got[5][1])
    for q, r in zip(got[:3], ref[:3]):
        assert (np.abs(_hmm.to_float(q) - r) <= _hmm.count_bound(r, T, 2, n_steps)).all()
    assert abs(_total_ll(got) - ref[3]) <= _hmm.ll_bound(n_steps, 2)
    # a zero emission: rows holding symbol 1 after state 0 is forced are impossible
    B0 = np.array([[1.0, 0.0], [1.0, 0.0]], np.float32)
    rows = np.array([[0, 0, 0], [0, 1, 0], [1, -1, -1], [-1, 0, 0], [0, 0, 1]], np.int16)
    st = H.hmm_estep_numpy(rows, A, B0, pi)[5]
    assert dict(zip(H.STAT_NAMES, st.tolist())) == {"sequences": 1, "steps": 3, "empty": 1, "impossible": 3}
    _same(H.hmm_estep_numpy(rows, A, B0, pi), H.hmm_estep_reference(rows, A, B0, pi))


def test_mstep_rules():
    q = lambda x: (np.asarray(x, np.float64) * 2.0 ** 32).astype(np.int64)
    prevA = np.array([[0.25, 0.75], [0.6, 0.4]], np.float32)
    prevB = np.array([[0.5, 0.25, 0.25], [0.1, 0.2, 0.7]], np.float32)
    prevpi = np.array([0.3, 0.7], np.float32)
    trans, emit, init = q([[1.0, 3.0], [0.0, 0.0]]), q([[2.0, 1.0, 1.0], [0.0, 0.0, 0.0]]), q([0.0, 0.0])
    A, B, pi = H.hmm_mstep(trans, emit, init, (prevA, prevB, prevpi))
    assert A.dtype == B.dtype == pi.dtype == np.float32
    assert A[0].tolist() == [0.25, 0.75] and B[0].tolist() == [0.5, 0.25, 0.25]
    assert np.array_equal(A[1], prevA[1]) and np.array_equal(B[1], prevB[1])       # never visited: kept
    assert np.array_equal(pi, prevpi)
    A2, _, _ = H.hmm_mstep(trans, emit, init, (prevA, prevB, prevpi), prior=1.0)
    assert A2[0].tolist() == [np.float32(2 / 6), np.float32(4 / 6)] and np.array_equal(A2[1], prevA[1])
    rows = H.normalised_rows(np.random.default_rng(1).integers(1, 2 ** 40, (50, 17)), np.zeros((50, 17)), 0.5)
    assert rows.dtype == np.float64 and np.abs(rows.sum(1) - 1).max() <= 4 * np.finfo(np.float64).eps
    # torch tensors are taken as well (the device fit hands the copied buffer over)
    A3, _, _ = H.hmm_mstep(torch.from_numpy(trans), torch.from_numpy(emit), torch.from_numpy(init),
                           tuple(torch.from_numpy(x) for x in (prevA, prevB, prevpi)))
    assert np.array_equal(A3, A)


def _em_totals(obs, A, B, pi, iters):
    """Log-likelihood of every model on the way, the last M-step's result included."""
    totals, steps = [], 0
    for _ in range(iters + 1):
        out = H.hmm_estep_numpy(obs, A, B, pi)
        totals.append(_total_ll(out))
        steps = int(out[5][1])
        A, B, pi = H.hmm_mstep(*out[:3], (A, B, pi))
    return totals, steps


def test_em_from_the_generating_model():
    S, O = 3, 6
    A, B, pi = _hmm.model(S, O, seed=40)
    obs = _hmm.sample(A, B, pi, 150, 25, seed=41)
    totals, steps = _em_totals(obs, A, B, pi, 5)
    bound = _hmm.ll_bound(steps, S)
    assert all(b >= a - bound for a, b in zip(totals, totals[1:]))
    assert totals[-1] >= totals[0] - bound


def test_em_from_a_random_start_on_separated_data():
    S, O = 3, 6
    A = np.array([[0.9, 0.05, 0.05], [0.05, 0.9, 0.05], [0.05, 0.05, 0.9]], np.float32)
    B = np.zeros((S, O), np.float32)
    for s in range(S):
        B[s, 2 * s:2 * s + 2] = 0.48
        B[s] += 0.01
    pi = np.full(S, 1 / 3, np.float32)
    obs = torch.from_numpy(_hmm.sample(A, B, pi, 200, 30, seed=43))
    b = HiddenMarkovModelBuilder(None, [f"o{i}" for i in range(O)])
    fit = b.fit_unsupervised(obs, n_states=S, iters=12, tol=0.0, seed=7)
    hist = fit.log_likelihood
    bound = _hmm.ll_bound(fit.stats["steps"], S)
    assert len(hist) >= 3 and all(y >= x - bound for x, y in zip(hist, hist[1:]))
    assert hist[-1] > hist[0] + 100 * bound             # it learned something
    assert fit.model.states == ["s0", "s1", "s2"] and fit.iterations == len(hist)
    assert fit.stats["sequences"] == 200 and fit.stats["steps"] == 6000
    # the stopping rule: a loose tolerance stops early and says so; tol=None keeps no history
    loose = b.fit_unsupervised(obs, n_states=S, iters=12, tol=0.05, seed=7)
    assert loose.converged and loose.iterations < fit.iterations
    assert loose.log_likelihood == hist[:loose.iterations]
    blind = b.fit_unsupervised(obs, n_states=S, iters=3, tol=None, seed=7)
    assert blind.log_likelihood == () and blind.iterations == 3 and not blind.converged
    every2 = b.fit_unsupervised(obs, n_states=S, iters=5, tol=0.0, check_every=2, seed=7)
    assert every2.log_likelihood == (hist[1], hist[3], hist[4])
    with pytest.raises(Exception):       # frozen
        fit.iterations = 0


def _rank_fit(rank, world, obs, S, O):
    from avenir_amd.models.markov import HiddenMarkovModelBuilder
    b = HiddenMarkovModelBuilder([f"s{i}" for i in range(S)], [f"o{i}" for i in range(O)])
    f = b.fit_unsupervised(obs[rank::world], iters=4, tol=0.0, seed=3)
    m = f.model
    return [x.numpy().tobytes() for x in (m.A, m.B, m.pi)], f.log_likelihood, f.iterations, f.converged, f.stats


def test_world_sizes_give_identical_fits():
    S, O = 3, 5
    A, B, pi = _hmm.model(S, O, seed=50)
    obs = torch.from_numpy(_hmm.sample(A, B, pi, 90, 10, seed=51))
    obs[4, 3:] = -1
    one = _rank_fit(0, 1, obs, S, O)
    assert one[2] >= 2
    for world in (2, 4):
        for res in run_world(_rank_fit, world, obs, S, O):
            assert res == one, world


def _write_obs(path, obs, names, delim=","):
    path.write_text("".join(f"u{r}{delim}" + delim.join(names[o] for o in row if o >= 0) + "\n"
                            for r, row in enumerate(obs)))


def test_trainer_job(tmp_path):
    from avenir_amd.cli import main
    A, B, pi = _hmm.model(3, 4, seed=31)
    obs = _hmm.sample(A, B, pi, 120, 12, seed=32)
    obs[7, 5:] = -1
    names = ["a", "b", "c", "d"]
    common = ["--device", "cpu", "-D", "hmmt.model.observations=a,b,c,d", "-D", "hmmt.model.states=X,Y,Z",
              "-D", "hmmt.max.iterations=4", "-D", "hmmt.seed=5"]
    native, split = tmp_path / "native.txt", tmp_path / "split.txt"
    _write_obs(tmp_path / "obs.csv", obs, names)
    _write_obs(tmp_path / "obs.txt", obs, names, "  ")
    assert main(["hiddenMarkovModelTrainer", "-i", str(tmp_path / "obs.csv"), "-o", str(native)] + common) == 0
    assert main(["hiddenMarkovModelTrainer", "-i", str(tmp_path / "obs.txt"), "-o", str(split),
                 "-D", "hmmt.field.delim.regex=\\s+"] + common) == 0
    lines = native.read_text().splitlines()
    assert lines == split.read_text().splitlines()
    assert lines[:2] == ["X,Y,Z", "a,b,c,d"] and len(lines) == 2 + 3 + 3 + 1
    assert all(abs(sum(int(x) for x in ln.split(",")) - 1000) <= 4 for ln in lines[2:])
    # the model equals the library fit on the same rows
    fit = HiddenMarkovModelBuilder(["X", "Y", "Z"], names).fit_unsupervised(torch.from_numpy(obs), iters=4, seed=5)
    assert lines == fit.model.to_lines(",", 1000)
    # viterbiStatePredictor reads it unchanged
    states = tmp_path / "states.txt"
    assert main(["viterbiStatePredictor", "-i", str(tmp_path / "obs.csv"), "-o", str(states), "--model", str(native),
                 "--device", "cpu"]) == 0
    dec = states.read_text().splitlines()
    assert len(dec) == 120 and dec[7].split(",")[0] == "u7" and len(dec[7].split(",")) == 6
    assert set(",".join(d.split(",", 1)[1] for d in dec).split(",")) <= {"X", "Y", "Z"}
    # an initial model is honoured: 0 iterations give its lines back
    start = HiddenMarkovModel(["H", "L"], ["a", "b", "c", "d"],
                              torch.tensor([[0.9, 0.1], [0.2, 0.8]], dtype=torch.float64),
                              torch.tensor([[0.7, 0.1, 0.1, 0.1], [0.1, 0.2, 0.3, 0.4]], dtype=torch.float64),
                              torch.tensor([0.5, 0.5], dtype=torch.float64))
    ip = tmp_path / "start.txt"
    ip.write_text("\n".join(start.to_lines(",", 1000)) + "\n")
    back, refined = tmp_path / "back.txt", tmp_path / "refined.txt"
    base = ["hiddenMarkovModelTrainer", "-i", str(tmp_path / "obs.csv"), "--device", "cpu",
            "-D", f"hmmt.initial.model.path={ip}"]
    assert main(base + ["-o", str(back), "-D", "hmmt.max.iterations=0"]) == 0
    assert back.read_text() == ip.read_text()
    assert main(base + ["-o", str(refined), "-D", "hmmt.max.iterations=3"]) == 0
    out = refined.read_text().splitlines()
    assert out[:2] == ["H,L", "a,b,c,d"] and out != back.read_text().splitlines()


def test_golden_replay():
    g = np.load(GOLDEN)
    obs, A, B, pi = g["obs"], g["A"], g["B"], g["pi"]
    got = H.hmm_estep_numpy(obs, A, B, pi)
    for n, x in zip(NAMES, got):
        assert x.dtype == g[n].dtype and np.array_equal(x, g[n]), n
    b = HiddenMarkovModelBuilder([f"s{i}" for i in range(A.shape[0])], [f"o{i}" for i in range(B.shape[1])])
    fit = b.fit_unsupervised(torch.from_numpy(obs), iters=5, tol=0.0, seed=int(g["fit_seed"]))
    assert np.array_equal(fit.model.A.numpy(), g["fit_A"]) and np.array_equal(fit.model.B.numpy(), g["fit_B"])
    assert np.array_equal(fit.model.pi.numpy(), g["fit_pi"])
    assert np.array_equal(np.asarray(fit.log_likelihood), g["fit_log_likelihood"])
    assert fit.iterations == int(g["fit_iterations"])
