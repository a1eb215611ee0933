"""hmm_estep_kernel (csrc/kernels/hmm.hip) against its numpy twin: every output bit-equal."""
import numpy as np
import pytest
import torch

from avenir_amd.models import hmm_em as H
from avenir_amd.models.markov import HiddenMarkovModel, HiddenMarkovModelBuilder

import _hmm

pytestmark = pytest.mark.gpu

NAMES = ("trans_q", "emit_q", "init_q", "Z", "E", "stats")
O_BIG = 6000      # 12 * S * O bytes of B and emission sums no longer fit in LDS at any S


def _device(obs, A, B, pi, **kw):
    out = H.hmm_estep(torch.from_numpy(obs).cuda(), A, B, pi, **kw)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in out]


def _assert_equal(got, want, what=""):
    for n, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, n, g.dtype, w.dtype)
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g,
                              w.view(np.int32) if w.dtype == np.float32 else w), (what, n)


@pytest.mark.parametrize("O", [5, O_BIG])
@pytest.mark.parametrize("S", [1, 3, 8, 32, 33, 64])
def test_kernel_equals_twin(S, O):
    A, B, pi = _hmm.model(S, O, seed=S + O, zero_symbol=True)
    kinds = set()
    for T in (1, 2, 65):
        for N in (1, 7, 8, 9, 257):
            # at O_BIG the rows draw from 7 symbols so that emission cells collide
            obs = _hmm.ragged_obs(N, T, O, seed=1000 * T + N, symbols=None if O == 5 else 7)
            want = H.hmm_estep_numpy(obs, A, B, pi)
            _assert_equal(_device(obs, A, B, pi), want, f"S={S} O={O} T={T} N={N}")
            st = want[5]
            assert st[0] + st[2] + st[3] == N
            kinds |= {k for k, v in zip(H.STAT_NAMES, st) if v}
    assert kinds == set(H.STAT_NAMES)       # the cases held good, empty and impossible rows


def test_rescale_case():
    A = np.array([[0.7, 0.3], [0.4, 0.6]], np.float32)
    B = np.array([[0.2, 0.1], [0.15, 0.2]], np.float32)     # 0.2^400 underflows fp32 unscaled
    pi = np.array([0.5, 0.5], np.float32)
    obs = _hmm.ragged_obs(9, 400, 2, seed=5, special=False)
    obs[0] = np.resize(np.array([0, 1, 1], np.int16), 400)
    want = H.hmm_estep_numpy(obs, A, B, pi)
    assert want[4].min() < -700 and np.isfinite(want[3]).all()
    _assert_equal(_device(obs, A, B, pi), want)


@pytest.mark.parametrize("case", ["mixed", "all_tiny"])
def test_subnormal_model(case):
    """Entries of 1e-30: products reach fp32 subnormals, which kernel and twin both keep."""
    S, O, T, N = 3, 4, 12, 33
    A, B, pi = _hmm.model(S, O, seed=9)
    if case == "mixed":       # a subnormal beside normal values: it survives the rescale as one
        pi = np.array([1e-9, 0.5, 0.5], np.float32)
        B[0, :] = 1e-30
        A[1, 0] = A[2, 0] = 1e-30
    else:                     # every first-step value is subnormal: frexp / ldexp scale them up
        pi = np.full(S, 1e-9, np.float32)
        B[:, :] = np.float32(1e-30) * (1 + np.arange(S * O, dtype=np.float32).reshape(S, O))
    obs = _hmm.ragged_obs(N, T, O, seed=11, special=False)
    first = pi[:, None] * B
    assert ((first > 0) & (first < np.finfo(np.float32).tiny)).any()
    want = H.hmm_estep_numpy(obs, A, B, pi)
    assert want[5][0] > 0
    _assert_equal(_device(obs, A, B, pi), want, case)


def test_chunking_cannot_change_a_result():
    S, O, T, N = 8, 5, 33, 100
    A, B, pi = _hmm.model(S, O, seed=2, zero_symbol=True)
    obs = _hmm.ragged_obs(N, T, O, seed=3)
    one = _device(obs, A, B, pi)
    per_row = T * (S + 1) * 4
    many = _device(obs, A, B, pi, workspace_bytes=per_row * 30)       # 4 chunks of <= 30 rows
    _assert_equal(many, one)
    _assert_equal(_device(obs, A, B, pi, workspace_bytes=1), one)     # one row per launch
    _assert_equal(one, H.hmm_estep_numpy(obs, A, B, pi))


def test_binding_validation():
    from avenir_amd import _native
    C = _native.C()
    dev = torch.device("cuda")

    def args(S=3, O=5, N=4, T=6):
        f = lambda *s: torch.full(s, 0.5, dtype=torch.float32, device=dev)
        z = lambda *s: torch.zeros(s, dtype=torch.int64, device=dev)
        return dict(obs=torch.zeros((N, T), dtype=torch.int16, device=dev), A=f(S, S), B=f(S, O), pi=f(S),
                    trans=z(S, S), emit=z(S, O), init=z(S), Z=f(N), E=torch.zeros(N, dtype=torch.int32, device=dev),
                    stats=z(4), workspace=f(N * T * (S + 1)))

    def call(a):
        C.hmm_estep(*[a[k] for k in ("obs", "A", "B", "pi", "trans", "emit", "init", "Z", "E", "stats", "workspace")])

    call(args())                                       # the well-formed call passes
    torch.cuda.synchronize()
    bad = []
    a = args(); a["obs"] = a["obs"].cpu(); bad.append(a)
    a = args(); a["A"] = a["A"].cpu(); bad.append(a)
    a = args(); a["obs"] = a["obs"].int(); bad.append(a)
    a = args(); a["B"] = a["B"].double(); bad.append(a)
    a = args(); a["trans"] = a["trans"].int(); bad.append(a)
    a = args(); a["E"] = a["E"].long(); bad.append(a)
    bad.append(args(S=65))
    a = args(); a["B"] = a["B"][:2].contiguous(); bad.append(a)
    a = args(); a["emit"] = a["emit"][:, :4].contiguous(); bad.append(a)
    a = args(); a["workspace"] = a["workspace"][:-1]; bad.append(a)
    a = args(); a["Z"] = a["Z"][:-1]; bad.append(a)
    for a in bad:
        with pytest.raises(RuntimeError):
            call(a)


def _fit_bits(fit):
    m = fit.model
    return ([x.numpy().tobytes() for x in (m.A, m.B, m.pi)], fit.log_likelihood, fit.iterations, fit.converged,
            fit.stats)


def test_fit_unsupervised_cuda_equals_cpu():
    S, O = 4, 6
    A, B, pi = _hmm.model(S, O, seed=21)
    obs = torch.from_numpy(_hmm.sample(A, B, pi, 300, 20, seed=22))
    obs[5, 7:] = -1
    b = HiddenMarkovModelBuilder([f"s{i}" for i in range(S)], [f"o{i}" for i in range(O)])
    kw = dict(iters=5, tol=0.0, seed=4, workspace_bytes=20 * (S + 1) * 4 * 64)
    cpu = b.fit_unsupervised(obs, **kw)
    gpu = b.fit_unsupervised(obs.cuda(), **kw)
    assert _fit_bits(cpu) == _fit_bits(gpu)
    assert len(cpu.log_likelihood) >= 2
    # semi-supervised: refining a given model, and the public posterior counts
    init = HiddenMarkovModel(b.states, b.observations, *(torch.from_numpy(x).double() for x in (A, B, pi)))
    assert _fit_bits(b.fit_unsupervised(obs, init=init, iters=2, tol=None)) == \
        _fit_bits(b.fit_unsupervised(obs.cuda(), init=init, iters=2, tol=None))
    for c, g in zip(init.posterior_counts(obs), init.posterior_counts(obs.cuda())):
        assert g.is_cuda and torch.equal(c, g.cpu())


def test_trainer_job_cuda_equals_cpu(tmp_path):
    from avenir_amd.cli import main
    A, B, pi = _hmm.model(3, 4, seed=31)
    obs = _hmm.sample(A, B, pi, 200, 12, seed=32)
    names = ["a", "b", "c", "d"]
    inp = tmp_path / "obs.txt"
    inp.write_text("".join(f"u{r}," + ",".join(names[o] for o in row) + "\n" for r, row in enumerate(obs)))
    outs = []
    for dev in ("cpu", "cuda"):
        out = tmp_path / f"model_{dev}.txt"
        assert main(["hiddenMarkovModelTrainer", "-i", str(inp), "-o", str(out), "--device", dev,
                     "-D", "hmmt.model.observations=a,b,c,d", "-D", "hmmt.model.state.count=3",
                     "-D", "hmmt.max.iterations=4", "-D", "hmmt.trans.prob.scale=1000000"]) == 0
        outs.append(out.read_text())
    assert outs[0] == outs[1] and len(outs[0].splitlines()) == 2 + 3 + 3 + 1
