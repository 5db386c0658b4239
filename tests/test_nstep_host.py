"""n-step returns without a GPU: the numpy restatement of include/fbdqn.h's n-step semantics that the GPU tests
(tests/test_gpu_nstep.py) compose one-step gathers with, checked on hand-worked tapes; and the CLI refusals that are decided before
anything touches the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def nstep_return(rews, terms, gamma):
    """rews f32[n, B], terms u8[n, B]: the one-step rows of transitions t, t+1, .., t+n-1 (of one env).  -> (R f32[B], done u8[B],
    Gamma): m = n, or k + 1 for the first k < n with term[k]; R = float32(sum_{k<m} g_k * float64(rew[k])) in ascending k with
    g_0 = 1, g_{k+1} = g_k * gamma (float64); done = any term[k]; Gamma = g_n."""
    rews, terms = np.asarray(rews, np.float32), np.asarray(terms, np.uint8)
    n, B = rews.shape
    R, done = np.empty(B, np.float32), np.zeros(B, np.uint8)
    for b in range(B):
        acc, g = 0.0, 1.0
        for k in range(n):
            acc += g * float(rews[k, b])
            g *= float(gamma)
            if terms[k, b]:
                done[b] = 1
                break
        R[b] = np.float32(acc)
    G = 1.0
    for _ in range(n):
        G *= float(gamma)
    return R, done, (float(gamma) if n == 1 else G)


def test_nstep_return_hand_worked_tapes():
    g = 0.9
    # columns: no terminal, terminal at k = 0, at k = 1, at k = n - 1 = 2
    rews = np.array([[0.1, -3.0, 0.1, 0.1],
                     [0.1, 0.1, -3.0, 3.0],
                     [3.0, 0.1, 0.1, -3.0]], np.float32)
    terms = np.array([[0, 1, 0, 0],
                      [0, 0, 1, 0],
                      [0, 0, 0, 1]], np.uint8)
    R, done, G = nstep_return(rews, terms, g)
    r01, r3, rm3 = float(np.float32(0.1)), 3.0, -3.0
    assert R[0] == np.float32(r01 + 0.9 * r01 + (0.9 * 0.9) * r3)
    assert R[1] == np.float32(rm3)                       # the crash ends the sum at once
    assert R[2] == np.float32(r01 + 0.9 * rm3)
    assert R[3] == np.float32(r01 + 0.9 * r3 + (0.9 * 0.9) * rm3)
    assert done.tolist() == [0, 1, 1, 1]
    assert G == 0.9 * 0.9 * 0.9 and G == (1.0 * 0.9) * 0.9 * 0.9


def test_nstep_return_at_n1_is_the_one_step_transition():
    rng = np.random.default_rng(0)
    rews = rng.choice(np.array([0.1, 3.0, -3.0], np.float32), (1, 50))
    terms = (rng.random((1, 50)) < 0.3).astype(np.uint8)
    R, done, G = nstep_return(rews, terms, 0.99)
    assert np.array_equal(R, rews[0]) and np.array_equal(done, terms[0]) and G == 0.99


def test_nstep_return_ignores_what_follows_the_first_terminal():
    rews = np.array([[0.1], [-3.0], [3.0], [3.0]], np.float32)
    terms = np.array([[0], [1], [1], [0]], np.uint8)
    R, done, _ = nstep_return(rews, terms, 0.99)
    R2, done2, _ = nstep_return(rews[:2], terms[:2], 0.99)
    assert R[0] == R2[0] and done[0] == done2[0] == 1


def test_bootstrap_gamma_matches_the_restatement():
    from dqnflappybird_amd.vec import bootstrap_gamma
    for n in (1, 2, 3, 5, 16):
        assert bootstrap_gamma(0.99, n) == nstep_return(np.zeros((n, 1)), np.zeros((n, 1)), 0.99)[2]


@pytest.mark.parametrize("args,msg", [(["--vec", "16", "--n-step", "0"], "--n-step must be in"),
                                      (["--vec", "16", "--n-step", "17"], "--n-step must be in"),
                                      (["--vec", "16", "--model", "prioritydqn", "--n-step", "3"], "uniform replay"),
                                      (["--model", "dqn", "--n-step", "3"], "needs --vec")])
def test_cli_refuses_bad_n_step(args, msg):
    p = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and msg in p.stderr, (p.returncode, p.stderr)


def test_vecbrain_refuses_n_step_it_cannot_honour():
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    with pytest.raises(ValueError, match="uniform"):
        VecBrain(4, algo="per", n_step=3, backend=CpuVecBackend())
    with pytest.raises(ValueError, match="1..16"):
        VecBrain(4, algo="dqn", n_step=0, backend=CpuVecBackend())
    with pytest.raises(ValueError, match="n-step"):                 # a backend without the setter cannot give n > 1 ...
        VecBrain(4, algo="dqn", n_step=3, capacity=64, observe=2, backend=CpuVecBackend())
    vb = VecBrain(4, algo="dqn", capacity=64, observe=2, backend=CpuVecBackend())       # ... and keeps working at n = 1
    assert vb.n_step == 1 and vb.boot_gamma == vb.gamma
