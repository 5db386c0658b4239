"""The Huber (clipped-error) loss and FB_ALGO_DOUBLE_PER of the scalar heads (include/fbdqn.h) without a GPU: the float64 restatements
the GPU tests compare the kernels with (np_huber, np_huber_clamp, np_double_per_target), the header's hand-worked case, continuity of value
and slope at |d| = delta, the clamp against the finite difference of the loss; the ABI declarations; and every refusal the Python layers
make before anything touches the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_huber(d, delta):
    """l(d) of include/fbdqn.h in float64: d^2 for |d| <= delta, delta (2 |d| - delta) beyond (twice the textbook Huber loss);
    delta = 0 means off: d^2 everywhere"""
    d = np.asarray(d, np.float64)
    if delta == 0:
        return d * d
    ad = np.abs(d)
    return np.where(ad <= delta, d * d, delta * (2.0 * ad - delta))


def np_huber_clamp(d, delta):
    """what the gradient takes where the squared loss takes d: clamp(d, -delta, delta) (d itself with delta = 0); dl/dd = 2 x this"""
    d = np.asarray(d, np.float64)
    return d if delta == 0 else np.clip(d, -delta, delta)


def np_double_per_target(q_on_s2, q_tg_s2, R, done, Gamma):
    """FB_ALGO_DOUBLE_PER's (and FB_ALGO_DOUBLE's) target in float64: a* = the FIRST maximum of the online net's q(s', .), the value
    from the target net.  -> (y [B], a* [B])"""
    q_on_s2, q_tg_s2 = np.asarray(q_on_s2, np.float64), np.asarray(q_tg_s2, np.float64)
    astar = np.argmax(q_on_s2, 1)                                # (np.argmax: the first maximum)
    v = q_tg_s2[np.arange(len(astar)), astar]
    y = np.asarray(R, np.float64) + np.where(np.asarray(done).astype(bool), 0.0, Gamma * v)
    return y, astar


# ---------------------------------------------------------------------------------------------------------------- the references
def test_the_headers_hand_case():
    d = np.array([0.5, -3.0])
    terms = np_huber(d, 1.0)
    assert terms.tolist() == [0.25, 5.0] and terms.mean() == 2.625
    scale = 2.0 / 2                                              # a mean over B = 2
    assert (-scale * np_huber_clamp(d, 1.0)).tolist() == [-0.5, 1.0]


@pytest.mark.parametrize("delta", [0.25, 1.0, 3.5])
def test_value_and_slope_are_continuous_and_the_zone_is_the_squared_loss(delta):
    grid = np.linspace(-4 * delta, 4 * delta, 1601)
    inside = np.abs(grid) <= delta
    assert inside.sum() > 300 and (~inside).sum() > 300
    assert np.array_equal(np_huber(grid, delta)[inside], (grid * grid)[inside])
    assert np.array_equal(np_huber_clamp(grid, delta)[inside], grid[inside])
    for sgn in (1.0, -1.0):
        e = np.array([np.nextafter(delta, 0.0), delta, np.nextafter(delta, np.inf)]) * sgn
        l = np_huber(e, delta)
        assert l[1] == delta * delta                             # |d| = delta: the quadratic branch, and the linear one gives the same value
        assert delta * (2 * abs(e[1]) - delta) == delta * delta
        assert np.all(np.abs(l - delta * delta) <= 4 * delta * np.spacing(delta) * 2)
        c = np_huber_clamp(e, delta)
        assert c[1] == sgn * delta and c[2] == sgn * delta and abs(c[0]) < delta          # the slope 2 clamp(d) meets 2 delta from both sides
    assert np.all(np_huber(grid, delta) <= grid * grid) and np.all(np.diff(np_huber(grid[grid >= 0], delta)) > 0)


@pytest.mark.parametrize("delta", [0.25, 1.0, 3.5])
def test_clamp_is_the_finite_difference_of_the_loss(delta):
    rng = np.random.default_rng(int(delta * 100))
    d = rng.uniform(-4 * delta, 4 * delta, 4000)
    h = 1e-6 * delta
    d = d[np.abs(np.abs(d) - delta) > 2 * h]                     # (the central difference straddles the junction there; the slope is continuous)
    fd = (np_huber(d + h, delta) - np_huber(d - h, delta)) / (2 * h)
    np.testing.assert_allclose(fd, 2.0 * np_huber_clamp(d, delta), rtol=0, atol=1e-8 * delta + 1e-9)
    at = np.array([delta, -delta])                               # at the junction itself: one-sided differences from both sides
    for s in (h, -h):
        np.testing.assert_allclose((np_huber(at + s, delta) - np_huber(at, delta)) / s, 2.0 * np_huber_clamp(at, delta), rtol=0, atol=4 * h)


def test_off_is_the_squared_loss():
    d = np.random.default_rng(0).normal(size=100) * 5
    assert np.array_equal(np_huber(d, 0.0), d * d) and np.array_equal(np_huber_clamp(d, 0.0), d)
    assert np.array_equal(np_huber(d, 1e30), d * d) and np.array_equal(np_huber_clamp(d, 1e30), d)


def test_double_per_target_first_maximum_and_one_action():
    q_on = np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 1.0, 3.0], [0.0, 0.0, 0.0]])
    q_tg = np.array([[10.0, 20.0, 30.0]] * 4)
    y, astar = np_double_per_target(q_on, q_tg, [0.1, 3.0, -3.0, 0.5], [0, 0, 1, 0], 0.5)
    assert astar.tolist() == [0, 1, 0, 0] and y.tolist() == [0.1 + 5.0, 3.0 + 10.0, -3.0, 0.5 + 5.0]
    rng = np.random.default_rng(1)
    q1, t1 = rng.normal(size=(64, 1)), rng.normal(size=(64, 1))
    R, done = rng.choice([0.1, 3.0, -3.0], 64), rng.integers(0, 2, 64)
    y, astar = np_double_per_target(q1, t1, R, done, 0.99)      # one action: FB_ALGO_PER's target (max over the target net's one Q)
    assert not astar.any() and np.array_equal(y, np.where(done == 1, R, R + 0.99 * t1.max(1)))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ALGO_DOUBLE_PER 16", "int fb_qnet_set_huber(fb_qnet_t h, float delta);",
                 "int fb_qnet_get_huber(fb_qnet_t h, float *delta_host);", "terms (0.25, 5), loss 2.625, dLoss/dq = (-0.5, +1.0)"):
        assert decl in hdr, decl
    assert "#define FB_ALGO_MDQN 14" in hdr and not any(line.split()[2:3] == ["13"] for line in hdr.splitlines() if line.startswith("#define FB_ALGO_"))
    assert L.ALGO_DOUBLE_PER == 16 and 13 not in [v for k, v in vars(L).items() if k.startswith("ALGO_")]
    f, vp = ctypes.c_float, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_set_huber"] == [vp, f]
    assert L.SIGNATURES["fb_qnet_get_huber"] == [vp, vp]
    lib = L.lib()                                                # (binds both symbols: a stale library raises here)
    assert lib.fb_qnet_set_huber(None, 1.0) == -1 and "NULL" in lib.fb_last_error().decode()
    assert lib.fb_qnet_get_huber(None, None) == -1 and "NULL" in lib.fb_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_algo_tables_and_value_checks():
    from dqnflappybird_amd import vec, vecbrain
    assert vec.ALGOS["doubleper"] == 16 and 13 not in vec.ALGOS.values()
    assert "doubleper" in vec.WEIGHTED_ALGOS and "double" not in vec.WEIGHTED_ALGOS
    assert set(vec.PER_ALGOS) == {"per", "c51per", "c51doubleper"}                               # (pinned by earlier tests: unchanged)
    assert set(vec.PRIORITIZED_ALGOS) == {"per", "c51per", "c51doubleper", "qrper", "qrdoubleper"}
    assert "doubleper" in vecbrain.PER_ALGOS and "doubleper" in vecbrain.TARGET_SYNC and vecbrain.MEAN_LOSS["doubleper"]
    assert vecbrain.HipVecBackend.huber is True and vecbrain.HipVecBackend.double_per is True
    assert vec.check_huber(0) == 0.0 and vec.check_huber(1) == 1.0 and vec.check_huber(0.1) == float(np.float32(0.1))
    for bad in (float("nan"), float("inf"), -1.0, -1e-9, 1e39):  # (1e39 is infinite as the float the library takes)
        with pytest.raises(ValueError, match="huber \\(delta\\) must be finite and >= 0"):
            vec.check_huber(bad)


class _Capable:
    """a stub backend that claims the capabilities and fails if anything is built: the refusals come before"""
    name = "stub"
    per_one_step = per_n_step = c51 = c51_dueling = c51_noisy = qr = mdqn = huber = double_per = True

    def env(self, *a, **k):
        raise AssertionError("a refused VecBrain must not build anything")


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="c51", huber=1.0), "Huber loss is offered on the scalar heads only"),
    (dict(algo="c51doubleper", arch="c51dueling", huber=0.5), "Huber loss is offered on the scalar heads only"),
    (dict(algo="qr", huber=1.0), "not with algo 'qr' \\(QR has its own kappa\\)"),
    (dict(algo="qrdoubleper", arch="qrdueling", huber=2.0), "Huber loss is offered on the scalar heads only"),
    (dict(algo="nature", huber=-1.0), "huber \\(delta\\) must be finite and >= 0"),
    (dict(algo="doubleper", huber=float("nan")), "huber \\(delta\\) must be finite and >= 0"),
    (dict(algo="c51", huber=float("inf")), "huber \\(delta\\) must be finite and >= 0"),
    (dict(algo="doubleper", arch="c51"), "scalar heads: arch must be 'plain' or 'dueling'"),
    (dict(algo="doubleper", arch="qrdueling"), "scalar heads: arch must be 'plain' or 'dueling'"),
    (dict(algo="doubleper", noisy=True), "not with algo 'doubleper'"),
    (dict(algo="doubleper", n_step=17), "n_step must be in 1..16"),
])
def test_vecbrain_refusals_before_anything_is_built(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, backend=_Capable(), **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="nature", huber=1.0), "cpu-oracle \\(tests only\\) backend has no Huber loss \\(huber\\): huber = 1.0 needs it"),
    (dict(algo="dqn", arch="dueling", huber=0.5), "backend has no Huber loss \\(huber\\)"),
    (dict(algo="doubleper"), "backend has no Double-DQN with prioritized replay \\(double_per\\): algo 'doubleper' needs it"),
    (dict(algo="doubleper", arch="dueling", world=2, n_step=3), "backend has no Double-DQN with prioritized replay"),
])
def test_vecbrain_refusals_on_a_backend_without_the_capability(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    assert not hasattr(CpuVecBackend, "huber") and not hasattr(CpuVecBackend, "double_per")
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, backend=CpuVecBackend(), **kw)


def test_a_backend_without_the_capability_still_runs_with_huber_off():
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    vb = VecBrain(4, algo="nature", backend=CpuVecBackend(), capacity=200, observe=2, huber=0.0)
    assert vb.huber == 0.0


def test_checkpoint_key_round_trip_and_named_refusals(tmp_path):
    from dqnflappybird_amd.vecbrain import check_checkpoint_huber
    from dqnflappybird_amd.vec import check_huber
    paths = {}
    for name, kw in (("one", dict(huber=np.array([check_huber(1.0)], np.float64))), ("tenth", dict(huber=np.array([check_huber(0.1)], np.float64))),
                     ("none", dict())):
        paths[name] = str(tmp_path / f"{name}.npz")
        np.savez(paths[name], online=np.zeros(3, np.float32), **kw)
    z = {k: np.load(p) for k, p in paths.items()}
    check_checkpoint_huber(z["one"], 1.0, "x")
    check_checkpoint_huber(z["tenth"], check_huber(0.1), "x")               # float32-rounded values survive the float64 array exactly
    check_checkpoint_huber(z["none"], 0.0, "x")                             # an absent key means 0
    check_checkpoint_huber(z["one"], None, "x")                             # a distributional brain does not read the key
    with pytest.raises(ValueError, match="checkpoint x was trained with huber \\(delta\\) = 1.0, this VecBrain has huber = 0.5"):
        check_checkpoint_huber(z["one"], 0.5, "x")
    with pytest.raises(ValueError, match="trained with huber \\(delta\\) = 1.0, this VecBrain has huber = 0.0"):
        check_checkpoint_huber(z["one"], 0.0, "x")
    with pytest.raises(ValueError, match="trained with huber \\(delta\\) = 0.0, this VecBrain has huber = 1.0"):
        check_checkpoint_huber(z["none"], 1.0, "x")


@pytest.mark.parametrize("argv,msg", [
    (["--model", "doubleper"], "--model doubleper needs --vec"),
    (["--model", "doubleper", "--vec", "16", "--noisy"], "--noisy needs a C51 model"),
    (["--model", "ddqn", "--huber", "1"], "--huber needs --vec"),
    (["--model", "ddqn", "--vec", "16", "--huber", "-1"], "huber (delta) must be finite and >= 0"),
    (["--model", "doubleper", "--vec", "16", "--huber", "nan"], "huber (delta) must be finite and >= 0"),
    (["--model", "c51", "--vec", "16", "--huber", "1"], "--huber needs a scalar-head model"),
    (["--model", "qrrainbow", "--vec", "16", "--huber", "1"], "--huber needs a scalar-head model"),
])
def test_cli_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
