"""The dueling C51 head, host side: the ABI constant and creation call (its support checks come before any allocation, so they need no
GPU), the head's parameter layout, and the refusals of QNet, VecBrain, checkpoints, the TF bundle and the command line that come before
anything reaches the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_ERR_INVALID = -1
HEAD0 = 77984 + 1600 * 512 + 512


def test_header_and_binding_declare_the_dueling_c51_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "#define FB_ARCH_C51_DUELING 3" in hdr and L.ARCH_C51_DUELING == 3
    assert "int fb_qnet_create_c51_dueling(int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, " \
           "fb_qnet_t *out);" in hdr
    assert L.SIGNATURES["fb_qnet_create_c51_dueling"] == L.SIGNATURES["fb_qnet_create_c51"]


def test_library_refuses_bad_supports_before_allocating():
    from dqnflappybird_amd import _lib as L
    lib = L.lib()
    h = ctypes.c_void_p()
    bad = [(512, 2, 1, -10.0, 10.0), (512, 2, 65, -10.0, 10.0), (512, 3, 51, -10.0, 10.0), (512, 2, 51, 10.0, -10.0),
           (512, 2, 51, 1.0, 1.0), (512, 2, 51, float("nan"), 10.0), (512, 2, 51, -10.0, float("inf")), (500, 2, 51, -10.0, 10.0),
           (512, 0, 51, -10.0, 10.0), (512, 2, 51, -10.0, 10.0, 0)]
    for args in bad:
        fc, A, n, lo, hi = args[:5]
        mb = args[5] if len(args) > 5 else 32
        assert lib.fb_qnet_create_c51_dueling(fc, A, n, lo, hi, mb, ctypes.byref(h)) == FB_ERR_INVALID, args
        assert h.value is None
        assert "fb_qnet_create_c51_dueling" in lib.fb_last_error().decode()
    assert lib.fb_qnet_create_c51_dueling(512, 3, 51, -10.0, 10.0, 32, ctypes.byref(h)) == FB_ERR_INVALID
    assert "exceeds 128" in lib.fb_last_error().decode()
    # the scalar-head creation call makes neither distributional net
    assert lib.fb_qnet_create(L.ARCH_C51_DUELING, 512, 2, 32, ctypes.byref(h)) == FB_ERR_INVALID
    assert "fb_qnet_create_c51_dueling" in lib.fb_last_error().decode() and h.value is None


def test_head_layout_sizes():
    """W_v[FC, N] b_v[N] W_a[FC, A N] b_a[A N]: 78 489 head parameters at the default size, against C51's 52 326"""
    FC, N, A = 512, 51, 2
    assert FC * N + N + FC * A * N + A * N == 78489
    assert FC * A * N + A * N == 52326


def test_qnet_arch_checks_need_no_gpu():
    from dqnflappybird_amd.vec import QNet
    assert "c51dueling" in QNet.ARCHS
    with pytest.raises(ValueError, match="arch must be one of"):
        QNet(2, 512, "c51duel")
    with pytest.raises(ValueError, match="n_atoms"):
        QNet(2, 512, "c51dueling", n_atoms=80)
    with pytest.raises(ValueError, match="128"):
        QNet(3, 512, "c51dueling", n_atoms=51)


def test_vecbrain_refusals_need_no_gpu():
    from dqnflappybird_amd.vecbrain import VecBrain
    for algo in ("c51", "c51double", "c51per", "c51doubleper"):
        with pytest.raises(ValueError, match="dueling C51.*c51dueling"):
            VecBrain(16, algo=algo, arch="dueling")
        with pytest.raises(ValueError, match="data-parallel C51"):
            VecBrain(16, algo=algo, arch="c51dueling", world=2)

        class NoDuelingC51:                           # a backend with C51 nets but not the dueling head
            name = "stand-in"
            c51 = True
            per_one_step = True
        with pytest.raises(ValueError, match="no dueling C51 nets"):
            VecBrain(16, algo=algo, arch="c51dueling", backend=NoDuelingC51())
    for algo in ("dqn", "nature", "double", "per"):
        with pytest.raises(ValueError, match="C51 algo"):
            VecBrain(16, algo=algo, arch="c51dueling")


def test_checkpoint_head_checks(tmp_path):
    from dqnflappybird_amd.vecbrain import check_checkpoint_head
    old = tmp_path / "old.npz"                        # a C51 checkpoint from before the head was recorded
    np.savez(old, support=np.array([51, -10.0, 10.0]))
    check_checkpoint_head(np.load(old), "c51", old)
    with pytest.raises(ValueError, match="holds a c51 head, this VecBrain has a c51dueling head"):
        check_checkpoint_head(np.load(old), "c51dueling", old)
    new = tmp_path / "new.npz"
    np.savez(new, support=np.array([51, -10.0, 10.0]), head=np.array(["c51dueling"]))
    check_checkpoint_head(np.load(new), "c51dueling", new)
    with pytest.raises(ValueError, match="holds a c51dueling head, this VecBrain has a c51 head"):
        check_checkpoint_head(np.load(new), "c51", new)


def test_tf_bundle_refuses_a_dueling_c51_net(tmp_path):
    from dqnflappybird_amd import tf_bundle
    n = HEAD0 + 512 * 51 + 51 + 512 * 102 + 102
    with pytest.raises(ValueError, match="plain head"):
        tf_bundle.save_flat(str(tmp_path / "x"), np.zeros(n, np.float32))


def test_cli_rainbow_needs_vec():
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN", "--model", "rainbow", "--n-step", "3"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 2
    assert "--model rainbow needs --vec" in out.stderr
