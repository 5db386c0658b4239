"""Distributional (C51) Q-learning, host side: the categorical projection restated in numpy (the literal loop of include/fbdqn.h,
written independently of the torch restatement in tests/test_gpu_c51.py) against hand-worked cases, and the argument and checkpoint
checks that run before anything reaches the GPU."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_ERR_INVALID = -1                                   # include/fbdqn.h


def np_project(p_next, r, done, gamma, n_atoms, v_min, v_max):
    """m[B, N]: the projection of Tz_j = clamp(r + gamma (1 - done) z_j) onto the support, one atom at a time (float64).
    l == u keeps the whole mass on the atom."""
    p_next = np.asarray(p_next, np.float64)
    B = p_next.shape[0]
    dz = (v_max - v_min) / (n_atoms - 1)
    z = v_min + dz * np.arange(n_atoms)
    m = np.zeros((B, n_atoms))
    for b in range(B):
        for j in range(n_atoms):
            tz = min(max(float(r[b]) + gamma * (1.0 - float(done[b])) * z[j], v_min), v_max)
            bj = min(max((tz - v_min) / dz, 0.0), n_atoms - 1.0)
            l, u = int(np.floor(bj)), int(np.ceil(bj))
            if l == u:
                m[b, l] += p_next[b, j]
            else:
                m[b, l] += p_next[b, j] * (u - bj)
                m[b, u] += p_next[b, j] * (bj - l)
    return m


def test_projection_hand_worked_between_atoms():
    # support -1, 0, 1; r = 0.5, gamma = 1: Tz = -0.5, 0.5, 1.5 -> clamp 1; b = 0.5, 1.5, 2
    m = np_project([[0.2, 0.3, 0.5]], [0.5], [0], 1.0, 3, -1.0, 1.0)
    np.testing.assert_allclose(m, [[0.1, 0.1 + 0.15, 0.15 + 0.5]])
    assert abs(m.sum() - 1.0) < 1e-12


def test_projection_on_atoms_keeps_the_mass():
    # integer rewards on a unit grid with gamma = 1: every b_j lands on an atom (l == u), nothing is dropped
    p = np.full((1, 21), 1 / 21)
    m = np_project(p, [3.0], [0], 1.0, 21, -10.0, 10.0)
    want = np.zeros(21)
    for j in range(21):
        want[min(j + 3, 20)] += 1 / 21            # shift by three atoms, the top four pile up at v_max
    np.testing.assert_allclose(m[0], want)
    assert abs(m.sum() - 1.0) < 1e-12


def test_projection_terminal_and_clamps():
    p = np.array([[0.25, 0.25, 0.25, 0.25]])
    # done: all mass at r, between atoms -2/3 .. 2/3 grid of [-2, 2] with 4 atoms (dz = 4/3): r = 1 -> b = 2.25
    m = np_project(p, [1.0], [1], 0.99, 4, -2.0, 2.0)
    np.testing.assert_allclose(m, [[0, 0, 0.75, 0.25]])
    # beyond the support on either side: clamped to the end atoms
    np.testing.assert_allclose(np_project(p, [-30.0], [1], 0.99, 4, -2.0, 2.0), [[1, 0, 0, 0]])
    np.testing.assert_allclose(np_project(p, [30.0], [0], 0.5, 4, -2.0, 2.0), [[0, 0, 0, 1]])


def test_projection_preserves_mass_randomly():
    rng = np.random.default_rng(0)
    p = rng.random((64, 51)); p /= p.sum(1, keepdims=True)
    r = rng.choice([0.1, 3.0, -3.0], 64)
    m = np_project(p, r, (r == -3.0).astype(np.uint8), 0.99 ** 3, 51, -10.0, 10.0)
    np.testing.assert_allclose(m.sum(1), 1.0, atol=1e-12)
    assert (m >= 0).all()


def test_binding_declares_the_c51_abi():
    from dqnflappybird_amd import _lib as L
    assert L.ARCH_C51 == 2 and L.ALGO_C51 == 5 and L.ALGO_C51_DOUBLE == 6 and L.C51_MAX_ATOMS == 64
    for name in ("fb_qnet_create_c51", "fb_qnet_get_support", "fb_qnet_forward_dist"):
        assert name in L.SIGNATURES


def test_library_refuses_bad_supports_before_allocating():
    """fb_qnet_create_c51's checks need no GPU: they come before any allocation"""
    from dqnflappybird_amd import _lib as L
    lib = L.lib()
    h = ctypes.c_void_p()
    bad = [(512, 2, 1, -10.0, 10.0), (512, 2, 65, -10.0, 10.0), (512, 3, 51, -10.0, 10.0), (512, 2, 51, 10.0, -10.0),
           (512, 2, 51, 1.0, 1.0), (512, 2, 51, float("nan"), 10.0), (512, 2, 51, -10.0, float("inf")), (500, 2, 51, -10.0, 10.0),
           (512, 0, 51, -10.0, 10.0)]
    for fc, A, n, lo, hi in bad:
        assert lib.fb_qnet_create_c51(fc, A, n, lo, hi, 32, ctypes.byref(h)) == FB_ERR_INVALID, (fc, A, n, lo, hi)
        assert h.value is None
    msg = L.lib().fb_last_error().decode()
    assert "n_actions" in msg
    # the scalar-head creation call does not make C51 nets
    assert lib.fb_qnet_create(L.ARCH_C51, 512, 2, 32, ctypes.byref(h)) == FB_ERR_INVALID
    assert "fb_qnet_create_c51" in L.lib().fb_last_error().decode()


def test_check_support_mirrors_the_library():
    from dqnflappybird_amd.vec import check_support
    assert check_support(51, -10, 10) == (51, -10.0, 10.0)
    for args in [(1, -10, 10), (65, -10, 10), (51, 10, -10), (51, float("nan"), 1)]:
        with pytest.raises(ValueError):
            check_support(*args)
    with pytest.raises(ValueError, match="128"):
        check_support(51, -1, 1, actions=3)


def test_vecbrain_refusals_need_no_gpu():
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(ValueError, match="dueling C51"):
        VecBrain(16, algo="c51", arch="dueling")
    with pytest.raises(ValueError, match="data-parallel C51"):
        VecBrain(16, algo="c51double", world=2)
    with pytest.raises(ValueError, match="n_atoms"):
        VecBrain(16, algo="c51", n_atoms=80)

    class NoC51:                                      # a backend without C51 nets (e.g. tests/cpu_backend.py)
        name = "stand-in"
    with pytest.raises(ValueError, match="no C51 nets"):
        VecBrain(16, algo="c51", backend=NoC51())


def test_checkpoint_support_checks(tmp_path):
    from dqnflappybird_amd.vecbrain import check_checkpoint_support
    p = tmp_path / "c.npz"
    np.savez(p, support=np.array([51, -10.0, 10.0]))
    z = np.load(p)
    check_checkpoint_support(z, (51, -10.0, 10.0), p)
    with pytest.raises(ValueError, match="support"):
        check_checkpoint_support(z, (51, -10.0, 20.0), p)
    with pytest.raises(ValueError, match="scalar head"):
        check_checkpoint_support(z, None, p)
    q = tmp_path / "plain.npz"
    np.savez(q, online=np.zeros(3))
    with pytest.raises(ValueError, match="scalar-head"):
        check_checkpoint_support(np.load(q), (51, -10.0, 10.0), q)
    check_checkpoint_support(np.load(q), None, q)


def test_tf_bundle_refuses_a_c51_net(tmp_path):
    """the reference checkpoint format has a scalar 2-output head: a C51 parameter vector does not fit it"""
    from dqnflappybird_amd import tf_bundle
    n = 77984 + 1600 * 512 + 512 + 512 * 102 + 102
    with pytest.raises(ValueError, match="plain head"):
        tf_bundle.save_flat(str(tmp_path / "x"), np.zeros(n, np.float32))
