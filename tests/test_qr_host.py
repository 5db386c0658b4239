"""QR-DQN, host side (include/fbdqn.h): a numpy restatement of the quantile Huber loss and its gradient written
as the literal double loop (checked against the header's worked case, the kinks at u = 0 and |u| = kappa, kappa != 1 and terminal
samples), the creation call's refusals (made before any allocation, so they need no GPU), and the refusals of QNet, VecBrain,
checkpoints and the command line that come before anything reaches the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FB_ERR_INVALID = -1


def np_qr_loss(theta, T, kappa):
    """l = (1/N) sum_i sum_j |tau_i - 1{u_ij < 0}| L_k(u_ij) / k and dl/dtheta_i, u_ij = T_j - theta_i, in float64, the double loop"""
    theta, T = np.asarray(theta, np.float64), np.asarray(T, np.float64)
    N = len(theta)
    loss, grad = 0.0, np.zeros(N)
    for i in range(N):
        tau = (2 * i + 1) / (2 * N)
        for j in range(N):
            u = T[j] - theta[i]
            w = abs(tau - (1.0 if u < 0 else 0.0))
            hub = 0.5 * u * u if abs(u) <= kappa else kappa * (abs(u) - 0.5 * kappa)
            loss += w * hub / kappa
            grad[i] -= w * min(max(u, -kappa), kappa) / kappa
    return loss / N, grad / N


def np_targets(r, done, G, theta_next):
    """T_j = R + Gamma (1 - done) theta'_j"""
    return r + G * (1.0 - done) * np.asarray(theta_next, np.float64)


def test_the_worked_case_of_the_header():
    loss, grad = np_qr_loss([0.0, 1.0], [0.5, 3.0], 1.0)
    assert loss == pytest.approx(0.90625, abs=1e-15)
    np.testing.assert_allclose(grad, [-0.1875, -0.3125], rtol=0, atol=1e-15)
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "l = 0.90625, dl/dtheta = [-0.1875, -0.3125]" in hdr


def test_u_exactly_zero_and_at_kappa():
    # u = 0: the weight is tau (1{0 < 0} = 0), the Huber term and the gradient both 0
    loss, grad = np_qr_loss([1.0, 1.0], [1.0, 1.0], 1.0)
    assert loss == 0.0 and (grad == 0.0).all()
    # |u| = kappa: both branches of L_k agree (k^2 / 2) and the clamp reaches +-1
    for k in (0.5, 1.0, 2.0):
        loss, grad = np_qr_loss([0.0, 0.0], [k, k], k)         # u_ij = k for all: weights tau_i, L = k^2 / 2
        assert loss == pytest.approx((0.25 + 0.75) * 2 * (0.5 * k * k / k) / 2)
        np.testing.assert_allclose(grad, [-(0.25 * 2) / 2, -(0.75 * 2) / 2])
        loss_m, grad_m = np_qr_loss([0.0, 0.0], [-k, -k], k)   # u_ij = -k: weights 1 - tau_i
        assert loss_m == pytest.approx(loss)
        np.testing.assert_allclose(grad_m, [(0.75 * 2) / 2, (0.25 * 2) / 2])
    # continuity across the kink |u| = kappa
    e = 1e-9
    lo, _ = np_qr_loss([0.0, 0.0], [1.0 - e, 1.0 - e], 1.0)
    hi, _ = np_qr_loss([0.0, 0.0], [1.0 + e, 1.0 + e], 1.0)
    assert abs(hi - lo) < 1e-8


@pytest.mark.parametrize("kappa", [0.25, 1.0, 3.0])
def test_loss_and_gradient_match_autograd(kappa):
    import torch
    rng = np.random.default_rng(int(kappa * 100))
    for N in (2, 5, 51):
        theta = rng.normal(0, 2, N)
        T = rng.normal(0, 2, N)
        loss, grad = np_qr_loss(theta, T, kappa)
        th = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
        u = torch.tensor(T, dtype=torch.float64)[None, :] - th[:, None]
        tau = (2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)
        w = (tau[:, None] - (u < 0).double()).abs()
        hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa))
        lt = (w * hub / kappa).sum() / N
        lt.backward()
        assert loss == pytest.approx(lt.item(), rel=1e-12)
        np.testing.assert_allclose(grad, th.grad.numpy(), rtol=1e-12, atol=1e-14)


def test_kappa_scales_the_loss_as_the_definition_says():
    """|u| >> kappa: L_k(u) / k = |u| - k / 2, the plain quantile (pinball) loss less a constant; the gradient saturates at +-tau"""
    theta, T = [0.0, 0.0, 0.0], [100.0, 100.0, 100.0]
    for k in (0.1, 1.0):
        loss, grad = np_qr_loss(theta, T, k)
        taus = np.array([1, 3, 5]) / 6
        assert loss == pytest.approx((taus * 3 * (100.0 - k / 2)).sum() / 3)
        np.testing.assert_allclose(grad, -taus * 3 / 3)


def test_terminal_samples_take_the_reward_for_every_target():
    rng = np.random.default_rng(3)
    theta_next = rng.normal(0, 5, 11)
    T = np_targets(-3.0, 1.0, 0.99 ** 3, theta_next)
    assert (T == -3.0).all()
    theta = rng.normal(0, 1, 11)
    loss, grad = np_qr_loss(theta, T, 1.0)
    loss_c, grad_c = np_qr_loss(theta, np.full(11, -3.0), 1.0)
    assert loss == loss_c and np.array_equal(grad, grad_c)
    T2 = np_targets(0.1, 0.0, 0.99, theta_next)
    np.testing.assert_allclose(T2, 0.1 + 0.99 * theta_next)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_qr_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ARCH_QR 4", "#define FB_ARCH_QR_DUELING 5", "#define FB_ALGO_QR 9", "#define FB_ALGO_QR_DOUBLE 10",
                 "#define FB_ALGO_QR_PER 11", "#define FB_ALGO_QR_DOUBLE_PER 12",
                 "int fb_qnet_create_qr(int arch, int fc_width, int n_actions, int n_quantiles, float kappa, int max_batch, fb_qnet_t *out);",
                 "int fb_qnet_get_quantiles(fb_qnet_t h, int *n_quantiles_host, float *kappa_host);",
                 "int fb_qnet_forward_quantiles(fb_qnet_t h, int which, const uint8_t *states, int batch, float *theta, void *stream);"):
        assert decl in hdr, decl
    assert (L.ARCH_QR, L.ARCH_QR_DUELING) == (4, 5)
    assert (L.ALGO_QR, L.ALGO_QR_DOUBLE, L.ALGO_QR_PER, L.ALGO_QR_DOUBLE_PER) == (9, 10, 11, 12)
    i, f, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_create_qr"] == [i, i, i, i, f, i, vp]
    assert L.SIGNATURES["fb_qnet_get_quantiles"] == [vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_forward_quantiles"] == L.SIGNATURES["fb_qnet_forward_dist"]


def test_library_refuses_bad_quantile_nets_before_allocating():
    from dqnflappybird_amd import _lib as L
    lib = L.lib()
    h = ctypes.c_void_p()
    bad = [(L.ARCH_QR, 512, 2, 1, 1.0), (L.ARCH_QR, 512, 2, 65, 1.0), (L.ARCH_QR, 512, 3, 51, 1.0), (L.ARCH_QR_DUELING, 512, 3, 43, 1.0),
           (L.ARCH_QR, 512, 2, 51, 0.0), (L.ARCH_QR, 512, 2, 51, -1.0), (L.ARCH_QR, 512, 2, 51, float("nan")),
           (L.ARCH_QR, 512, 2, 51, float("inf")), (L.ARCH_C51, 512, 2, 51, 1.0), (L.ARCH_PLAIN, 512, 2, 51, 1.0),
           (L.ARCH_QR, 500, 2, 51, 1.0), (L.ARCH_QR, 512, 0, 51, 1.0)]
    for arch, fc, A, n, k in bad:
        assert lib.fb_qnet_create_qr(arch, fc, A, n, k, 32, ctypes.byref(h)) == FB_ERR_INVALID, (arch, fc, A, n, k)
        assert h.value is None
        assert "fb_qnet_create_qr" in lib.fb_last_error().decode()
    assert lib.fb_qnet_create_qr(L.ARCH_QR, 512, 3, 51, 1.0, 32, ctypes.byref(h)) == FB_ERR_INVALID
    assert "exceeds 128" in lib.fb_last_error().decode()
    assert lib.fb_qnet_create_qr(L.ARCH_QR, 512, 2, 51, 0.0, 32, ctypes.byref(h)) == FB_ERR_INVALID
    assert "kappa" in lib.fb_last_error().decode()
    # the scalar-head creation call makes neither QR net
    for arch in (L.ARCH_QR, L.ARCH_QR_DUELING):
        assert lib.fb_qnet_create(arch, 512, 2, 32, ctypes.byref(h)) == FB_ERR_INVALID
        assert "fb_qnet_create_qr" in lib.fb_last_error().decode() and h.value is None


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_qnet_checks_need_no_gpu():
    from dqnflappybird_amd import vec
    from dqnflappybird_amd.vec import QNet, check_quantiles
    assert "qr" in QNet.ARCHS and "qrdueling" in QNet.ARCHS
    assert check_quantiles(51, 1.0) == (51, 1.0)
    assert vec.ALGOS["qr"] == 9 and vec.ALGOS["qrdouble"] == 10 and vec.ALGOS["qrper"] == 11 and vec.ALGOS["qrdoubleper"] == 12
    assert vec.QR_ALGOS == ("qr", "qrdouble") and vec.QR_PER_ALGOS == ("qrper", "qrdoubleper")
    assert set(vec.PRIORITIZED_ALGOS) == {"per", "c51per", "c51doubleper", "qrper", "qrdoubleper"}
    for kw, msg in ((dict(n_quantiles=1), "n_quantiles"), (dict(n_quantiles=65), "n_quantiles"), (dict(kappa=0.0), "kappa"),
                    (dict(kappa=float("nan")), "kappa"), (dict(kappa=-2.0), "kappa")):
        with pytest.raises(ValueError, match=msg):
            QNet(2, 512, "qr", **kw)
    with pytest.raises(ValueError, match="<= 128"):
        QNet(3, 512, "qrdueling", n_quantiles=51)
    with pytest.raises(ValueError, match="C51 heads only"):
        QNet(2, 512, "qr", noisy=True)


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="qr", arch="c51"), "QR head on the plain trunk"),
    (dict(algo="qrper", arch="dueling"), "QR head on the plain trunk"),
    (dict(algo="qr", world=2), "data-parallel QR"),
    (dict(algo="qrdoubleper", noisy=True), "noisy"),
    (dict(algo="qr", n_quantiles=1), "n_quantiles"),
    (dict(algo="qrdouble", kappa=0.0), "kappa"),
    (dict(algo="nature", arch="qr"), "QR head: it trains with a QR algo"),
    (dict(algo="c51", arch="qrdueling"), "QR head: it trains with a QR algo"),
])
def test_vecbrain_refusals_need_no_gpu(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, **kw)


def test_vecbrain_tables():
    from dqnflappybird_amd import vecbrain
    for algo in ("qr", "qrdouble", "qrper", "qrdoubleper"):
        assert vecbrain.MEAN_LOSS[algo] and algo in vecbrain.TARGET_SYNC
    assert set(vecbrain.PER_ALGOS) >= {"qrper", "qrdoubleper"} and "qr" not in vecbrain.PER_ALGOS


def test_checkpoint_head_checks(tmp_path):
    """a QR checkpoint goes into a QR brain of the same head, N and kappa only; C51 (recorded or not) and scalar checkpoints do not"""
    from dqnflappybird_amd.vecbrain import check_checkpoint_quantiles
    paths = {}
    for name, kw in (("qr", dict(head=np.array(["qr"]), quantiles=np.array([51, 1.0]))),
                     ("qrdueling", dict(head=np.array(["qrdueling"]), quantiles=np.array([51, 1.0]))),
                     ("c51", dict(head=np.array(["c51"]), support=np.array([51, -10.0, 10.0]))),
                     ("c51old", dict(support=np.array([51, -10.0, 10.0]))),
                     ("plain", dict())):
        paths[name] = str(tmp_path / f"{name}.npz")
        np.savez(paths[name], online=np.zeros(3, np.float32), **kw)
    z = {k: np.load(p) for k, p in paths.items()}
    check_checkpoint_quantiles(z["qr"], (51, 1.0), "qr", "x")
    check_checkpoint_quantiles(z["c51"], None, "c51", "x")
    check_checkpoint_quantiles(z["plain"], None, "plain", "x")
    with pytest.raises(ValueError, match="holds a qr \\(QR\\) head, this VecBrain has a c51 head"):
        check_checkpoint_quantiles(z["qr"], None, "c51", "x")
    with pytest.raises(ValueError, match="holds a c51 head, this VecBrain has a qr \\(QR\\) head"):
        check_checkpoint_quantiles(z["c51"], (51, 1.0), "qr", "x")
    with pytest.raises(ValueError, match="holds a c51 head"):
        check_checkpoint_quantiles(z["c51old"], (51, 1.0), "qr", "x")
    with pytest.raises(ValueError, match="holds a scalar head"):
        check_checkpoint_quantiles(z["plain"], (51, 1.0), "qr", "x")
    with pytest.raises(ValueError, match="qrdueling head, this VecBrain has a qr head"):
        check_checkpoint_quantiles(z["qrdueling"], (51, 1.0), "qr", "x")
    with pytest.raises(ValueError, match="n_quantiles, kappa"):
        check_checkpoint_quantiles(z["qr"], (41, 1.0), "qr", "x")
    with pytest.raises(ValueError, match="n_quantiles, kappa"):
        check_checkpoint_quantiles(z["qr"], (51, 0.5), "qr", "x")


@pytest.mark.parametrize("argv,msg", [
    (["--model", "qrdqn"], "--model qrdqn needs --vec"),
    (["--model", "qrrainbow"], "--model qrrainbow needs --vec"),
    (["--model", "qrdqnper", "--vec", "16", "--noisy"], "--noisy needs a C51 model"),
    (["--model", "qrdqn", "--vec", "16", "--n-quantiles", "65"], "n_quantiles must be in 2..64"),
    (["--model", "qrdqn", "--vec", "16", "--kappa", "0"], "kappa must be finite and > 0"),
    (["--model", "c51", "--vec", "16", "--kappa", "2"], "--n-quantiles / --kappa need a QR model"),
])
def test_cli_qr_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
