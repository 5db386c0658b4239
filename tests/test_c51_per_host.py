"""C51 with prioritized replay, host side: the KL priority and the memory's clipped priority restated in numpy (hand-worked cases), the
ABI constants and names, and the refusals of VecBrain and the command line that come before anything reaches the GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_kl_priority(m, p):
    """max(0, KL(m || p)) per row: sum over the atoms with m_i > 0 of m_i (log m_i - log p_i) (include/fbdqn.h FB_ALGO_C51_PER)"""
    m, p = np.atleast_2d(np.asarray(m, np.float64)), np.atleast_2d(np.asarray(p, np.float64))
    pos = m > 0
    terms = np.where(pos, m * (np.log(np.where(pos, m, 1.0)) - np.log(p)), 0.0)
    return np.maximum(terms.sum(-1), 0.0)


def np_priority(err):
    """Memory.batch_update's leaf for one |error| as the memory forms it: min(err + 0.01, 1)^0.6, fp32 (the reference's numpy arrays)"""
    e = np.float32(err) + np.float32(0.01)
    c = min(e, np.float32(1.0))
    return float(np.float32(np.float64(c) ** np.float64(np.float32(0.6))))


# ---------------------------------------------------------------------------------------------------------------- KL priorities
def test_kl_is_zero_when_the_prediction_is_the_target():
    m = np.array([[0.1, 0.2, 0.3, 0.4], [0.0, 0.5, 0.5, 0.0], [1.0, 0.0, 0.0, 0.0]])
    p = np.where(m > 0, m, 1e-9)
    p /= p.sum(1, keepdims=True)
    np.testing.assert_allclose(np_kl_priority(m[:1], m[:1]), [0.0], atol=1e-15)
    np.testing.assert_allclose(np_kl_priority(m, p), 0.0, atol=1e-8)


def test_kl_drops_the_empty_atoms():
    # m on two atoms, p spread over three: KL = 0.5 log(0.5 / 0.25) * 2 = log 2; the m = 0 atom adds nothing (0 log 0 = 0)
    np.testing.assert_allclose(np_kl_priority([0.5, 0.5, 0.0], [0.25, 0.25, 0.5]), [np.log(2.0)], rtol=1e-15)
    # all the target's mass on one atom: KL = -log p there
    np.testing.assert_allclose(np_kl_priority([0.0, 1.0, 0.0], [0.2, 0.3, 0.5]), [-np.log(0.3)], rtol=1e-15)
    # the uniform prediction: KL = log N - H(m), the figure early training sits at (~3 for 51 atoms and a two-atom target)
    N = 51
    m = np.zeros(N); m[20], m[21] = 0.3, 0.7
    h = -(0.3 * np.log(0.3) + 0.7 * np.log(0.7))
    np.testing.assert_allclose(np_kl_priority(m, np.full(N, 1.0 / N)), [np.log(N) - h], rtol=1e-13)
    assert np_kl_priority(m, np.full(N, 1.0 / N))[0] > 3.0


def test_kl_is_never_negative():
    rng = np.random.default_rng(0)
    for N in (2, 11, 51):
        p = rng.random((200, N)) + 1e-6; p /= p.sum(1, keepdims=True)
        m = rng.random((200, N)) * (rng.random((200, N)) < 0.3); m[:, 0] += 1e-3; m /= m.sum(1, keepdims=True)
        assert (np_kl_priority(m, p) >= 0).all()
        near = p * (1 + 1e-12 * rng.standard_normal((200, N)))      # rounding may push the exact KL below 0: clamped
        assert (np_kl_priority(p, near) >= 0).all()


def test_priorities_saturate_at_the_clip():
    assert np_priority(3.0) == 1.0 and np_priority(0.99) == 1.0
    assert np_priority(0.0) == pytest.approx(0.01 ** 0.6, rel=1e-6)
    assert np_priority(0.5) == pytest.approx(0.51 ** 0.6, rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------- names
def test_constants_and_names():
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd import vec, vecbrain
    assert (L.ALGO_C51_PER, L.ALGO_C51_DOUBLE_PER) == (7, 8)
    assert (L.ALGO_C51, L.ALGO_C51_DOUBLE, L.ALGO_PER) == (5, 6, 3)
    assert vec.ALGOS["c51per"] == 7 and vec.ALGOS["c51doubleper"] == 8
    assert set(vec.PER_ALGOS) == {"per", "c51per", "c51doubleper"}
    assert vec.C51_ALGOS == ("c51", "c51double")                 # (the uniform-memory C51 algos are unchanged)
    assert vecbrain.MEAN_LOSS["c51per"] and vecbrain.MEAN_LOSS["c51doubleper"]
    assert "c51per" in vecbrain.TARGET_SYNC and "c51doubleper" in vecbrain.TARGET_SYNC and "per" not in vecbrain.TARGET_SYNC
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "#define FB_ALGO_C51_PER 7" in hdr and "#define FB_ALGO_C51_DOUBLE_PER 8" in hdr


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_vecbrain_refusals_need_no_gpu():
    from dqnflappybird_amd.vecbrain import VecBrain
    for algo in ("c51per", "c51doubleper"):
        with pytest.raises(ValueError, match="dueling C51"):
            VecBrain(16, algo=algo, arch="dueling")
        with pytest.raises(ValueError, match="data-parallel C51"):
            VecBrain(16, algo=algo, world=2)
        with pytest.raises(ValueError, match="n_atoms"):
            VecBrain(16, algo=algo, n_atoms=80)

        class NoC51:                                  # a backend without C51 nets
            name = "stand-in"
            per_one_step = True
        with pytest.raises(ValueError, match="no C51 nets"):
            VecBrain(16, algo=algo, backend=NoC51())

        class NoOneStep:                              # C51 nets, but no one-call prioritized step
            name = "stand-in"
            c51 = True
        with pytest.raises(ValueError, match="per_one_step"):
            VecBrain(16, algo=algo, backend=NoOneStep())

        class NoPerNStep:                             # C51 nets and the prioritized step, n-step returns on uniform replay only
            name = "stand-in"
            c51 = True
            per_one_step = True
        with pytest.raises(ValueError, match="uniform replay only"):
            VecBrain(16, algo=algo, n_step=3, backend=NoPerNStep())


@pytest.mark.parametrize("model", ["c51per", "c51doubleper"])
def test_cli_needs_vec(model):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN", "--model", model, "--n-step", "3"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2
    assert f"--model {model} needs --vec" in out.stderr


def test_cli_keeps_refusing_n_step_with_prioritydqn():
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN", "--model", "prioritydqn", "--vec", "16", "--n-step", "3"],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "prioritydqn takes --n-step 1" in out.stderr
