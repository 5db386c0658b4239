"""Per-env acting noise of noisy C51 nets, host side: the ABI (header, binding, the noise stream), the calls' refusals of a NULL handle
(no device touched), and the refusals of QNet, VecBrain and the command line that come before anything reaches the GPU."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_ERR_INVALID = -1


def test_header_and_binding_declare_the_acting_noise_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ACT_NOISE_SHARED 0", "#define FB_ACT_NOISE_PER_ENV 1", "int fb_qnet_set_acting_noise(fb_qnet_t h, int mode);",
                 "int fb_qnet_act_nib_env_noise(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,\n"
                 "                              uint8_t *actions, float *q, void *stream);", "FB_STREAM_ENV_NOISE = 7"):
        assert decl in hdr, decl
    assert (L.ACT_NOISE_SHARED, L.ACT_NOISE_PER_ENV) == (0, 1)
    i, f, vp, u64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_uint64
    assert L.SIGNATURES["fb_qnet_set_acting_noise"] == [vp, i]
    assert L.SIGNATURES["fb_qnet_act_nib_env_noise"] == [vp, vp, i, f, u64, u64, vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_act_nib_env_noise"] == L.SIGNATURES["fb_qnet_act_nib"]
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "#define FB_STREAM_ENV_NOISE 7u" in common


def test_library_refuses_a_null_handle():
    from dqnflappybird_amd import _lib as L
    lib = L.lib()
    for mode in (L.ACT_NOISE_SHARED, L.ACT_NOISE_PER_ENV, 2, -1):
        assert lib.fb_qnet_set_acting_noise(None, mode) == FB_ERR_INVALID
    assert "fb_qnet_set_acting_noise" in lib.fb_last_error().decode()
    buf = ctypes.create_string_buffer(16)
    assert lib.fb_qnet_act_nib_env_noise(None, buf, 1, 0.0, 1, 2, buf, None, None) == FB_ERR_INVALID
    assert "fb_qnet_act_nib_env_noise" in lib.fb_last_error().decode()


def test_qnet_acting_noise_needs_a_noisy_net():
    from dqnflappybird_amd.vec import ACTING_NOISE_MODES, QNet
    assert ACTING_NOISE_MODES == ("shared", "env")
    net = QNet.__new__(QNet)                              # (the host checks in front of any library call)
    net.noisy = False
    with pytest.raises(ValueError, match="set_acting_noise needs a noisy net"):
        net.set_acting_noise("env")
    with pytest.raises(ValueError, match="act_nib_env_noise needs a noisy net"):
        net.act_nib_env_noise(None, 0.0)


def test_vecbrain_acting_noise_refusals_need_no_gpu():
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    for algo in ("c51", "c51doubleper"):
        with pytest.raises(ValueError, match="acting_noise='env' needs a noisy net"):
            VecBrain(16, algo=algo, arch="c51dueling", acting_noise="env")
        for bad in ("per_env", "Env", None, 1):
            with pytest.raises(ValueError, match="acting_noise must be 'shared' or 'env'"):
                VecBrain(16, algo=algo, arch="c51dueling", noisy=True, acting_noise=bad)

        class NoEnvNoise:                                 # a backend with noisy C51 nets but no per-env acting noise
            name = "stand-in"
            c51 = True
            c51_dueling = True
            c51_noisy = True
            per_one_step = True
        with pytest.raises(ValueError, match="stand-in backend has no per-env acting noise"):
            VecBrain(16, algo=algo, arch="c51dueling", noisy=True, acting_noise="env", backend=NoEnvNoise())
    with pytest.raises(ValueError, match="backend has no per-env acting noise"):
        VecBrain(16, algo="c51", noisy=True, acting_noise="env", backend=CpuVecBackend())
    with pytest.raises(ValueError, match="acting_noise='env' needs a noisy net"):
        VecBrain(16, algo="dqn", acting_noise="env", backend=CpuVecBackend())


@pytest.mark.parametrize("argv,msg", [
    (["--model", "rainbow", "--vec", "16", "--acting-noise", "env"], "--acting-noise env needs --noisy"),
    (["--model", "c51", "--vec", "16", "--acting-noise", "env"], "--acting-noise env needs --noisy"),
    (["--model", "rainbow", "--vec", "16", "--noisy", "--acting-noise", "per-env"], "invalid choice"),
])
def test_cli_acting_noise_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
