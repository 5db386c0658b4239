"""Noisy C51 nets, host side: the ABI (header, binding, the noise stream), the creation call's refusals (made before any allocation, so
they need no GPU), the [mu | sigma] layout and the noise vector's size, and the refusals of QNet, VecBrain, checkpoints, the TF bundle
and the command line that come before anything reaches the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_ERR_INVALID = -1
TRUNK = 77984                                         # W_fc1 starts here: sigma covers the flat vector from this entry on
HEAD0 = TRUNK + 1600 * 512 + 512


def test_header_and_binding_declare_the_noisy_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "int fb_qnet_create_c51_noisy(int arch, int fc_width, int n_actions, int n_atoms, float v_min, float v_max, float sigma0, " \
           "int max_batch,\n                             fb_qnet_t *out);" in hdr
    for decl in ("int fb_qnet_is_noisy(fb_qnet_t h);", "int fb_qnet_reset_noise(fb_qnet_t h, int which, uint64_t seed, uint64_t step, int mode, "
                 "void *stream);", "int fb_qnet_get_noise(fb_qnet_t h, int which, float *out);", "#define FB_NOISE_SAMPLE 0",
                 "#define FB_NOISE_MEAN 1", "FB_STREAM_NOISE = 6"):
        assert decl in hdr, decl
    assert (L.NOISE_SAMPLE, L.NOISE_MEAN) == (0, 1)
    i, f, vp, u64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint64
    assert L.SIGNATURES["fb_qnet_create_c51_noisy"] == [i, i, i, i, f, f, f, i, vp]
    assert L.SIGNATURES["fb_qnet_is_noisy"] == [vp]
    assert L.SIGNATURES["fb_qnet_reset_noise"] == [vp, i, u64, u64, i, vp]
    assert L.SIGNATURES["fb_qnet_get_noise"] == [vp, i, vp]
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "#define FB_STREAM_NOISE 6u" in common


def test_library_refuses_bad_arguments_before_allocating():
    from dqnflappybird_amd import _lib as L
    lib = L.lib()
    h = ctypes.c_void_p()
    ok = (512, 2, 51, -10.0, 10.0, 0.5, 32)

    def create(arch, *args):
        fc, A, n, lo, hi, s0, mb = args
        return lib.fb_qnet_create_c51_noisy(arch, fc, A, n, lo, hi, s0, mb, ctypes.byref(h))

    for arch in (L.ARCH_PLAIN, L.ARCH_DUELING, 4, -1):            # noisy layers: the C51 heads only
        assert create(arch, *ok) == FB_ERR_INVALID and h.value is None
        assert "arch must be FB_ARCH_C51 (2) or FB_ARCH_C51_DUELING (3)" in lib.fb_last_error().decode()
    for arch in (L.ARCH_C51, L.ARCH_C51_DUELING):
        for s0 in (-0.5, -1e-30, float("nan"), float("inf"), float("-inf")):
            assert create(arch, *ok[:5], s0, 32) == FB_ERR_INVALID and h.value is None, s0
            assert "sigma0 must be finite and >= 0" in lib.fb_last_error().decode()
        bad = [(512, 2, 1, -10.0, 10.0), (512, 2, 65, -10.0, 10.0), (512, 3, 51, -10.0, 10.0), (512, 2, 51, 10.0, -10.0),
               (512, 2, 51, float("nan"), 10.0), (500, 2, 51, -10.0, 10.0), (512, 0, 51, -10.0, 10.0)]
        for args in bad:
            assert create(arch, *args, 0.5, 32) == FB_ERR_INVALID and h.value is None, args
            assert "fb_qnet_create_c51_noisy" in lib.fb_last_error().decode()
        assert create(arch, *ok[:6], 0) == FB_ERR_INVALID and h.value is None
    assert lib.fb_qnet_create_c51_noisy(L.ARCH_C51, *ok, None) == FB_ERR_INVALID
    # the calls on a handle refuse NULL / non-noisy handles without touching a device
    assert lib.fb_qnet_is_noisy(None) == 0
    assert lib.fb_qnet_reset_noise(None, 0, 1, 2, 0, None) == FB_ERR_INVALID
    assert lib.fb_qnet_get_noise(None, 0, None) == FB_ERR_INVALID


def n_mu(head, FC=512, A=2, N=51):
    head_n = FC * A * N + A * N if head == "c51" else FC * N + N + FC * A * N + A * N
    return TRUNK + 1600 * FC + FC + head_n


@pytest.mark.parametrize("head,mu,total,nz", [("c51", 950022, 1822060, 2726), ("c51dueling", 976185, 1874386, 3289)])
def test_sigma_block_layout_and_noise_size(head, mu, total, nz):
    """[mu | sigma]: sigma of W_fc1 b_fc1 and of every head tensor, in mu's order -- the flat vector from W_fc1 on, once more"""
    from dqnflappybird_amd.vec import noise_size
    assert n_mu(head) == mu
    assert mu + (mu - TRUNK) == total
    sig = 1600 * 512 + 512 + (mu - HEAD0)                  # fc1's sigma, then the head's
    assert total - mu == sig
    assert noise_size(512, 2, 51, head) == nz
    # per layer fan_in + fan_out: fc1 1600 + 512, then 512 + 102 (C51) or 512 + 51 and 512 + 102 (dueling C51)
    assert nz == 1600 + 512 + (512 + 51 if head == "c51dueling" else 0) + 512 + 102
    for N in (2, 64):
        assert noise_size(512, 2, N, head) == 1600 + 512 + (512 + N if head == "c51dueling" else 0) + 512 + 2 * N


def test_qnet_noisy_checks_need_no_gpu():
    from dqnflappybird_amd.vec import QNet, check_sigma0
    for arch in ("plain", "dueling"):
        with pytest.raises(ValueError, match="noisy layers are offered on the C51 heads only"):
            QNet(2, 512, arch, noisy=True)
    for s0 in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma0 must be finite and >= 0"):
            QNet(2, 512, "c51", noisy=True, sigma0=s0)
    assert check_sigma0(0.5) == 0.5 and check_sigma0(0) == 0.0


def test_vecbrain_noisy_refusals_need_no_gpu():
    from dqnflappybird_amd.vecbrain import VecBrain
    for algo in ("dqn", "nature", "double", "per"):
        with pytest.raises(ValueError, match="noisy layers are offered on the C51 heads only"):
            VecBrain(16, algo=algo, noisy=True)
    for algo in ("c51", "c51double", "c51per", "c51doubleper"):
        with pytest.raises(ValueError, match="data-parallel C51"):
            VecBrain(16, algo=algo, arch="c51dueling", noisy=True, world=2)

        class NoNoisy:                                    # a backend with (dueling) C51 nets but no noisy ones
            name = "stand-in"
            c51 = True
            c51_dueling = True
            per_one_step = True
        with pytest.raises(ValueError, match="no noisy C51 nets"):
            VecBrain(16, algo=algo, arch="c51dueling", noisy=True, backend=NoNoisy())


def test_checkpoint_noisy_checks(tmp_path):
    from dqnflappybird_amd.vecbrain import check_checkpoint_noisy
    old = tmp_path / "old.npz"                            # a checkpoint from before noisy nets: not noisy
    np.savez(old, support=np.array([51, -10.0, 10.0]), head=np.array(["c51dueling"]))
    check_checkpoint_noisy(np.load(old), False, None, old)
    with pytest.raises(ValueError, match="holds a non-noisy net, this VecBrain has a noisy net"):
        check_checkpoint_noisy(np.load(old), True, 0.5, old)
    new = tmp_path / "new.npz"
    np.savez(new, support=np.array([51, -10.0, 10.0]), head=np.array(["c51dueling"]), noisy=np.array([1]), sigma0=np.array([0.5]))
    check_checkpoint_noisy(np.load(new), True, 0.5, new)
    with pytest.raises(ValueError, match="holds a noisy net, this VecBrain has a non-noisy net"):
        check_checkpoint_noisy(np.load(new), False, None, new)


def test_tf_bundle_refuses_a_noisy_net(tmp_path):
    from dqnflappybird_amd import tf_bundle
    for head in ("c51", "c51dueling"):
        with pytest.raises(ValueError, match="plain head"):
            tf_bundle.save_flat(str(tmp_path / "x"), np.zeros(2 * n_mu(head) - TRUNK, np.float32))


@pytest.mark.parametrize("argv,msg", [
    (["--model", "nature", "--vec", "16", "--noisy"], "--noisy needs a C51 model"),
    (["--model", "duelingdqn", "--vec", "16", "--noisy"], "--noisy needs a C51 model"),
    (["--model", "rainbow", "--noisy"], "--noisy needs --vec"),
    (["--model", "c51", "--noisy"], "--noisy needs --vec"),
])
def test_cli_noisy_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr


def test_evaluate_noise_modes_need_no_gpu():
    from dqnflappybird_amd.evaluate import NOISE_MODES, evaluate

    class Plain:                                          # a non-noisy net: only the mean weights exist
        noisy = False
    assert NOISE_MODES == ("mean", "sample")
    with pytest.raises(ValueError, match="noise must be one of"):
        evaluate(Plain(), 16, noise="avg")
    with pytest.raises(ValueError, match="noise='sample' needs a noisy net"):
        evaluate(Plain(), 16, noise="sample")
