"""Gradient clipping by global norm and soft target updates (include/fbdqn.h) without a GPU: the float64 restatement of the clip and the
header's hand-worked case, the ABI declarations, the value checks, every refusal the Python layers make before anything touches the GPU,
the command line's two flags, and the checkpoint keys."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_clip(g, G):
    """tf.clip_by_global_norm on one flat vector as include/fbdqn.h states it: float64 squares and sums, the norm rounded to fp32 once,
    c = G / max(norm, G) in fp32 (1 for G = 0 and for a norm that is not finite), g * c in fp32 -> (clipped fp32 vector, norm, c)"""
    g = np.asarray(g, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.float32(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    G = np.float32(G)
    c = np.float32(G / max(norm, G)) if G > 0 and np.isfinite(norm) else np.float32(1.0)
    return (g if c == 1.0 else g * c), float(norm), float(c)


def test_the_headers_hand_case_and_the_edge_cases():
    out, norm, c = np_clip([3.0, 4.0], 2.5)
    assert (norm, c) == (5.0, 0.5) and out.tolist() == [1.5, 2.0]
    g = np.array([3.0, 4.0], np.float32)
    for G in (5.0, 10.0, 0.0):                                   # norm <= G and G = 0: the same bits, c exactly 1
        out, norm, c = np_clip(g, G)
        assert out is g and (norm, c) == (5.0, 1.0)
    for bad in (np.inf, np.nan):
        out, norm, c = np_clip([1.0, bad], 2.5)
        assert not np.isfinite(norm) and c == 1.0
    rng = np.random.default_rng(0)
    tiny = (np.exp(rng.uniform(np.log(1e-9), np.log(1e-6), 100_003)) * rng.choice([-1.0, 1.0], 100_003)).astype(np.float32)
    out, norm, c = np_clip(tiny, 1e-6)                           # the reference's regime: no underflow, the clipped norm is G
    assert norm > 1e-6 and 0 < c < 1
    assert abs(np.linalg.norm(out.astype(np.float64)) - 1e-6) <= 1e-6 * 1e-6


def test_header_and_binding_declare_the_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("int fb_qnet_set_max_grad_norm(fb_qnet_t h, float g);", "int fb_qnet_get_max_grad_norm(fb_qnet_t h, float *g_host);",
                 "int fb_qnet_clip_grad(fb_qnet_t h, float *flat_grad, void *stream);",
                 "int fb_qnet_grad_norm(fb_qnet_t h, float *norm_host, float *scale_host);",
                 "int fb_qnet_soft_sync_target(fb_qnet_t h, float rho, void *stream);", "g = (3, 4), G = 2.5: norm 5, c 0.5, g <- (1.5, 2)"):
        assert decl in hdr, decl
    f, vp = ctypes.c_float, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_set_max_grad_norm"] == [vp, f] and L.SIGNATURES["fb_qnet_get_max_grad_norm"] == [vp, vp]
    assert L.SIGNATURES["fb_qnet_clip_grad"] == [vp, vp, vp] and L.SIGNATURES["fb_qnet_grad_norm"] == [vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_soft_sync_target"] == [vp, f, vp]
    lib = L.lib()                                                # (binds the symbols: a stale library raises here)
    for call in (lambda: lib.fb_qnet_set_max_grad_norm(None, 1.0), lambda: lib.fb_qnet_get_max_grad_norm(None, None),
                 lambda: lib.fb_qnet_clip_grad(None, None, None), lambda: lib.fb_qnet_grad_norm(None, None, None),
                 lambda: lib.fb_qnet_soft_sync_target(None, 0.5, None)):
        assert call() == -1 and "NULL" in lib.fb_last_error().decode()


def test_value_checks():
    from dqnflappybird_amd import vec, vecbrain
    assert vec.check_max_grad_norm(0) == 0.0 and vec.check_max_grad_norm(10) == 10.0
    assert vec.check_max_grad_norm(0.1) == float(np.float32(0.1))
    for bad in (float("nan"), float("inf"), -1.0, -1e-9, 1e39):  # (1e39 is infinite as the float the library takes)
        with pytest.raises(ValueError, match="max_grad_norm must be finite and >= 0"):
            vec.check_max_grad_norm(bad)
    assert vec.check_polyak(1) == 1.0 and vec.check_polyak(0.005) == float(np.float32(0.005))
    assert vec.check_polyak(0, allow_off=True) == 0.0 and vec.check_polyak(0.25, allow_off=True) == 0.25
    for bad in (0.0, -0.5, 1.0000001, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="polyak \\(rho\\) must be in \\(0, 1\\]"):
            vec.check_polyak(bad)
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="polyak \\(rho\\) must be in \\(0, 1\\] or 0 = off"):
            vec.check_polyak(bad, allow_off=True)
    assert vecbrain.HipVecBackend.grad_clip is True and vecbrain.HipVecBackend.polyak is True
    for name in ("set_max_grad_norm", "max_grad_norm", "clip_grad", "grad_norm", "soft_sync_target"):
        assert hasattr(vec.QNet, name), name


class _Capable:
    """a stub backend that claims every capability and fails if anything is built: the refusals come before"""
    name = "stub"
    per_one_step = per_n_step = c51 = c51_dueling = c51_noisy = qr = mdqn = huber = double_per = grad_clip = polyak = True

    def env(self, *a, **k):
        raise AssertionError("a refused VecBrain must not build anything")


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="doubleper", arch="dueling", max_grad_norm=-1.0), "max_grad_norm must be finite and >= 0"),
    (dict(algo="nature", max_grad_norm=float("nan")), "max_grad_norm must be finite and >= 0"),
    (dict(algo="c51", max_grad_norm=float("inf")), "max_grad_norm must be finite and >= 0"),
    (dict(algo="qr", polyak=-0.1), "polyak \\(rho\\) must be in \\(0, 1\\] or 0 = off"),
    (dict(algo="per", polyak=1.5), "polyak \\(rho\\) must be in \\(0, 1\\] or 0 = off"),
    (dict(algo="double", polyak=float("nan")), "polyak \\(rho\\) must be in \\(0, 1\\] or 0 = off"),
])
def test_vecbrain_refusals_before_anything_is_built(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, backend=_Capable(), **kw)


def test_accepted_values_reach_the_build():
    """good values pass every check: the stub's env() is the first thing built"""
    from dqnflappybird_amd.vecbrain import VecBrain
    for kw in (dict(algo="doubleper", arch="dueling", n_step=3, max_grad_norm=10.0, polyak=0.005), dict(algo="c51", max_grad_norm=10),
               dict(algo="qrdoubleper", arch="qrdueling", polyak=1.0), dict(algo="per", polyak=0.01)):
        with pytest.raises(AssertionError, match="must not build anything"):
            VecBrain(16, backend=_Capable(), **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="nature", max_grad_norm=10.0), "cpu-oracle \\(tests only\\) backend has no gradient clipping \\(grad_clip\\): max_grad_norm = 10.0 needs it"),
    (dict(algo="dqn", arch="dueling", polyak=0.005), "backend has no soft target updates \\(polyak\\): polyak = 0.005 needs it"),
    (dict(algo="double", world=2, max_grad_norm=1.0, polyak=0.5), "backend has no gradient clipping \\(grad_clip\\)"),
])
def test_vecbrain_refusals_on_a_backend_without_the_capability(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    assert not hasattr(CpuVecBackend, "grad_clip") and not hasattr(CpuVecBackend, "polyak")
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, backend=CpuVecBackend(), **kw)


def test_a_backend_without_the_capabilities_still_runs_with_both_off():
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    vb = VecBrain(4, algo="nature", backend=CpuVecBackend(), capacity=200, observe=2, batch=8, max_grad_norm=0.0, polyak=0.0)
    assert vb.max_grad_norm == 0.0 and vb.polyak == 0.0
    vb.run(5, log_every=0)                                       # (the hard sync's schedule, the unclipped step: as before)
    assert vb.timeStep == 5 and vb.last_loss is not None


class _Recorder:
    """the host logic of a polyak / clipping brain on stand-ins that record what VecBrain calls"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        return lambda *a, **k: self.calls.append((name, a))


def test_polyak_replaces_the_hard_sync_and_dp_clips_behind_the_reduction():
    from dqnflappybird_amd.vecbrain import VecBrain
    vb = VecBrain.__new__(VecBrain)
    net = _Recorder()
    vb.net, vb.algo, vb.replace_target_iter, vb.timeStep = net, "double", 500, 0
    vb.polyak = 0.0
    assert vb._hard_sync_due()
    vb.timeStep = 1
    assert not vb._hard_sync_due()
    vb.polyak, vb.timeStep = 0.005, 0
    assert not vb._hard_sync_due()                               # soft updates: no periodic copy, for any algo
    vb.grad, vb.max_grad_norm, order = "G", 10.0, []
    vb.reduce = lambda: order.append("reduce")
    vb._apply_reduced()
    assert order == ["reduce"] and [c[0] for c in net.calls] == ["clip_grad", "apply_adam"] and net.calls[0][1] == ("G",)
    net.calls.clear()
    vb.max_grad_norm = 0.0
    vb._apply_reduced()
    assert [c[0] for c in net.calls] == ["apply_adam"]


def test_cli_parses_both_flags():
    from dqnflappybird_amd.FlappyBirdDQN import build_parser, optimiser_kwargs
    p = build_parser()
    a = p.parse_args(["--model", "doubleper", "--vec", "1024", "--n-step", "3", "--max-grad-norm", "10", "--polyak", "0.005"])
    assert (a.max_grad_norm, a.polyak) == (10.0, 0.005)
    assert optimiser_kwargs(a, p) == dict(max_grad_norm=10.0, polyak=float(np.float32(0.005)))
    a = p.parse_args(["--model", "dqn", "--vec", "16"])
    assert (a.max_grad_norm, a.polyak) == (None, None) and optimiser_kwargs(a, p) == {}
    a = p.parse_args(["--model", "rainbow", "--vec", "16", "--polyak", "0"])
    assert optimiser_kwargs(a, p) == dict(polyak=0.0)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "ddqn", "--max-grad-norm", "10"], "--max-grad-norm / --polyak need --vec"),
    (["--model", "ddqn", "--polyak", "0.005"], "--max-grad-norm / --polyak need --vec"),
    (["--model", "ddqn", "--vec", "16", "--max-grad-norm", "-1"], "max_grad_norm must be finite and >= 0"),
    (["--model", "rainbow", "--vec", "16", "--max-grad-norm", "nan"], "max_grad_norm must be finite and >= 0"),
    (["--model", "qrdqn", "--vec", "16", "--polyak", "1.5"], "polyak (rho) must be in (0, 1] or 0 = off"),
    (["--model", "doubleper", "--vec", "16", "--polyak", "nan"], "polyak (rho) must be in (0, 1] or 0 = off"),
])
def test_cli_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr


def test_learn_curve_takes_both_flags():
    src = open(os.path.join(ROOT, "tools", "learn_curve.py")).read()
    assert '"--max-grad-norm"' in src and '"--polyak"' in src and "max_grad_norm=max_grad_norm, polyak=polyak" in src


def test_checkpoint_keys_round_trip_and_refuse_nothing(tmp_path):
    """both keys through np.savez as save() writes them (float64[1], only when on), read back by checkpoint_optimiser; a file without
    them reads as (0, 0); no value is a refusal -- they are optimiser settings, like the learning rate"""
    from dqnflappybird_amd.vec import check_max_grad_norm, check_polyak
    from dqnflappybird_amd.vecbrain import checkpoint_optimiser
    g, rho = check_max_grad_norm(10.0), check_polyak(0.005)
    both, none, one = (str(tmp_path / f"{n}.npz") for n in ("both", "none", "one"))
    np.savez(both, online=np.zeros(3, np.float32), max_grad_norm=np.array([g], np.float64), polyak=np.array([rho], np.float64))
    np.savez(none, online=np.zeros(3, np.float32))
    np.savez(one, online=np.zeros(3, np.float32), polyak=np.array([rho], np.float64))
    assert checkpoint_optimiser(np.load(both)) == (10.0, rho) and rho == float(np.float32(0.005))      # float32-rounded values survive exactly
    assert checkpoint_optimiser(np.load(none)) == (0.0, 0.0)
    assert checkpoint_optimiser(np.load(one)) == (0.0, rho)


def test_save_and_load_carry_the_keys(tmp_path):
    """VecBrain.save / load on the CPU stand-ins: a brain with both settings on writes both keys; a brain with other values loads the
    file without a refusal, keeps its own values and reports the file's"""
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend

    class Clipping(CpuVecBackend):                              # (claims the capabilities; the stand-in net records the calls)
        grad_clip = polyak = True

        def net(self, *a, **k):
            n = super().net(*a, **k)
            n.set_max_grad_norm = lambda g: setattr(n, "G", g)
            n.soft_sync_target = lambda rho: setattr(n, "soft", getattr(n, "soft", 0) + 1)
            return n

    kw = dict(algo="nature", capacity=200, observe=2, batch=8, seed=4)
    vb = VecBrain(4, backend=Clipping(), max_grad_norm=10.0, polyak=0.005, **kw)
    assert vb.net.G == 10.0
    vb.run(6, log_every=0)
    assert vb.net.soft == 3                                      # one soft update per train step (onlineTimeStep > observe), no hard sync needed
    path = str(tmp_path / "ck.npz")
    vb.save(path)
    z = np.load(path)
    assert z["max_grad_norm"].tolist() == [10.0] and z["polyak"].tolist() == [float(np.float32(0.005))]
    other = VecBrain(4, backend=Clipping(), max_grad_norm=0.0, polyak=0.5, **kw)
    other.load(path)
    assert (other.max_grad_norm, other.polyak) == (0.0, 0.5) and other.checkpoint_optimiser == (10.0, float(np.float32(0.005)))
    off = VecBrain(4, backend=CpuVecBackend(), **kw)
    p2 = str(tmp_path / "off.npz")
    off.save(p2)
    assert "max_grad_norm" not in np.load(p2).files and "polyak" not in np.load(p2).files
    off.load(path)                                               # a brain without either setting takes the file as well
    assert off.checkpoint_optimiser == (10.0, float(np.float32(0.005)))
