"""Implicit quantile networks, the host side: the ABI's declarations, the float64 restatements of the quantile function, the folded
greedy head and the pairwise quantile Huber loss (torch for autograd, numpy written independently; they must agree), the issue's two
worked cases, the fold identity, and every refusal that needs no GPU (check_iqn, VecIQN, the command line, the checkpoints of the four
loops).  tests/test_gpu_iqn.py imports the helpers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_oracle_qnet import split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
E = 64


def iqn_bounds(fc, A):
    """[(name, lo, hi)] of every parameter tensor of an IQN net's flat vector (include/fbdqn.h), in order"""
    sizes = [("W_conv1", 8192), ("b_conv1", 32), ("W_conv2", 32768), ("b_conv2", 64), ("W_conv3", 36864), ("b_conv3", 64),
             ("W_fc1", 1600 * fc), ("b_fc1", fc), ("W_q", fc * A), ("b_q", A), ("W_e", E * fc), ("b_e", fc)]
    out, o = [], 0
    for name, k in sizes:
        out.append((name, o, o + k))
        o += k
    return out


def n_plain(fc, A):
    return 77984 + 1600 * fc + fc + fc * A + A


def trunk64(p, states, fc, A):
    """relu(h_fc1) [B, fc] in float64 torch: tests/test_oracle_qnet.py::torch_forward's layers up to fc1"""
    w = split(p[:n_plain(fc, A)], fc, A, False)
    x = torch.as_tensor(np.array(states), dtype=torch.float64).permute(0, 3, 1, 2)
    h = F.relu(F.conv2d(x, w["w1"].permute(3, 2, 0, 1), w["b1"], stride=4, padding=2))
    h = F.max_pool2d(h, 2, 2)
    h = F.relu(F.conv2d(h, w["w2"].permute(3, 2, 0, 1), w["b2"], stride=2, padding=1))
    h = F.relu(F.conv2d(h, w["w3"].permute(3, 2, 0, 1), w["b3"], stride=1, padding=1))
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], 1600)
    return F.relu(h @ w["wf1"] + w["bf1"])


def head_parts(p, fc, A):
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    assert b["b_e"][1] == p.numel()
    cut = lambda n: p[b[n][0]:b[n][1]]
    return cut("W_q").view(fc, A), cut("b_q"), cut("W_e").view(E, fc), cut("b_e")


def pre64(p, tau, fc, A):
    """pre_k(tau) [..., fc] in float64 torch; tau: any shape, float32 values"""
    _, _, We, be = head_parts(p, fc, A)
    t = torch.as_tensor(np.asarray(tau, np.float64))
    c = torch.cos(np.pi * torch.arange(E, dtype=torch.float64) * t[..., None])
    return c @ We + be


def theta_from_h(p, h, tau, fc, A):
    """theta [B, M, A] from h [B, fc] and tau [B, M]"""
    Wq, bq, _, _ = head_parts(p, fc, A)
    phi = F.relu(pre64(p, tau, fc, A))                               # [B, M, fc]
    return (h[:, None, :] * phi) @ Wq + bq


def iqn_forward64(p, states, tau, fc, A):
    """the IQN net in float64 torch -> theta [B, M, A] at tau f32[B, M].  p: a float64 tensor (requires_grad for gradients)"""
    return theta_from_h(p, trunk64(p, states, fc, A), tau, fc, A)


def tau_grid(K, eta=1.0):
    """the acting grid, as include/fbdqn.h forms it: float32 of eta (2 i + 1) / (2 K) in double"""
    return (np.float64(F32(eta)) * (2 * np.arange(K) + 1) / (2 * K)).astype(F32)


def qbar_from_h(p, h, K, eta, fc, A):
    """Qbar [B, A]: the mean of float64 theta over the acting grid"""
    tau = np.broadcast_to(tau_grid(K, eta), (h.shape[0], K))
    return theta_from_h(p, h, tau, fc, A).mean(1)


def iqn_qbar64(p, states, K, eta, fc, A):
    return qbar_from_h(p, trunk64(p, states, fc, A), K, eta, fc, A)


def torch_iqn_loss(theta, T, tau, kappa):
    """the quantile Huber loss of the paper in float64 torch: theta [B, N] (requires grad), T [B, N'] (a constant), tau [B, N]
    -> (loss, l_b [B]); mean over j, sum over i, mean over b"""
    T = T.detach()
    u = T[:, None, :] - theta[:, :, None]                            # [B, N, N']
    au = u.abs()
    hub = torch.where(au <= kappa, 0.5 * u * u, kappa * (au - 0.5 * kappa))
    w = (torch.as_tensor(np.asarray(tau, np.float64))[:, :, None] - (u.detach() < 0).double()).abs()
    lb = (w * hub / kappa).sum(2).sum(1) / T.shape[1]
    return lb.mean(), lb


def np_iqn_loss(theta, T, tau, kappa, B=None):
    """the same in float64 numpy with explicit loops, and the gradient of include/fbdqn.h's formula -> (l_b [B], dl_b/dtheta [B, N] / B)"""
    theta, T, tau = (np.asarray(x, np.float64) for x in (theta, T, tau))
    nb, N = theta.shape
    Np = T.shape[1]
    B = nb if B is None else B
    lb, g = np.zeros(nb), np.zeros((nb, N))
    for b in range(nb):
        for i in range(N):
            for j in range(Np):
                u = T[b, j] - theta[b, i]
                w = abs(tau[b, i] - (1.0 if u < 0 else 0.0))
                L = 0.5 * u * u if abs(u) <= kappa else kappa * (abs(u) - 0.5 * kappa)
                lb[b] += w * L / kappa
                g[b, i] += w * min(max(u, -kappa), kappa) / kappa
        lb[b] /= Np
    return lb, -g / Np / B


WORKED = [  # (kappa, tau, theta, T, l, dl/dtheta): the issue's two cases
    (1.0, [0.25, 0.75], [0.0, 1.0], [0.5, 3.0], 0.90625, [-0.1875, -0.3125]),
    (0.5, [0.125, 0.6875], [0.2, -0.4], [0.1, 1.0, -2.0], 1.0560416666666667, [0.30833333333333335, -0.35416666666666669]),
]


def philox(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 as csrc/fb_common.h writes it -> (x, y, z, w)"""
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def np_draw_taus(batch, n, seed, step, which):
    """fb_iqn_draw_taus restated: counter (b * 64 + i, step_lo, 10, step_hi) under the seed; .x online, .y target"""
    out = np.empty((batch, n), F32)
    for b in range(batch):
        for i in range(n):
            o = philox(seed & 0xFFFFFFFF, seed >> 32, b * 64 + i, step & 0xFFFFFFFF, 10, step >> 32)
            out[b, i] = F32(2 * (o[which] >> 9) + 1) * F32(2.0 ** -24)
    return out


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_iqn_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ARCH_IQN 8", "#define FB_IQN_COS 64",
                 "int fb_qnet_create_iqn(int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch, fb_qnet_t *out);",
                 "int fb_qnet_set_iqn_risk(fb_qnet_t h, float eta);", "int fb_qnet_get_iqn(", "int fb_qnet_forward_iqn(", "int fb_iqn_draw_taus(",
                 "int fb_qnet_iqn_train_step(", "int fb_iqn_train_from_replay(", "int fb_iqn_step("):
        assert decl in hdr, decl
    assert L.ARCH_IQN == 8 and L.IQN_DEFAULTS == (8, 8, 32, 1.0) and L.IQN_COS == 64
    want = {"fb_qnet_create_iqn": 8, "fb_qnet_set_iqn_risk": 2, "fb_qnet_get_iqn": 6, "fb_qnet_forward_iqn": 8, "fb_iqn_draw_taus": 7,
            "fb_qnet_iqn_train_step": 17, "fb_iqn_train_from_replay": 17, "fb_iqn_step": 13}
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n, name
    for word in ("b_e is filled with 1.0, NOT 0.01", "(float)cos(M_PI * (double)j * (double)tau)", "FB_STREAM_TAU = 10",
                 "tauhat_i = (float)((double)eta * (2 i + 1) / (2 K))", "not offered prioritized replay, dueling or noisy IQN"):
        assert word in hdr, word
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "#define FB_STREAM_TAU 10u" in common


# ---------------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("kappa,tau,theta,T,l,g", WORKED)
def test_worked_cases(kappa, tau, theta, T, l, g):
    lb, dg = np_iqn_loss([theta], [T], [tau], kappa)
    assert abs(lb[0] - l) < 1e-14
    np.testing.assert_allclose(dg[0], g, rtol=0, atol=1e-14)
    th = torch.tensor([theta], dtype=torch.float64, requires_grad=True)
    loss, tl = torch_iqn_loss(th, torch.tensor([T], dtype=torch.float64), [tau], kappa)
    loss.backward()
    assert abs(loss.item() - l) < 1e-14 and abs(tl[0].item() - l) < 1e-14
    np.testing.assert_allclose(th.grad.numpy()[0], g, rtol=0, atol=1e-14)


@pytest.mark.parametrize("N,Np,kappa", [(8, 8, 1.0), (5, 7, 0.5), (64, 64, 2.0), (1, 1, 1.0)])
def test_torch_and_numpy_restatements_agree(N, Np, kappa):
    B = 9
    rng = np.random.default_rng(N * 100 + Np)
    theta, T = rng.normal(size=(B, N)) * 2, rng.normal(size=(B, Np)) * 2
    tau = rng.random((B, N)).astype(F32)
    u = T[:, None, :] - theta[:, :, None]
    if N > 1:
        assert (u < 0).any() and (u > 0).any() and (np.abs(u) < kappa).any() and (np.abs(u) > kappa).any()
    lb, g = np_iqn_loss(theta, T, tau, kappa)
    th = torch.tensor(theta, requires_grad=True)
    loss, tl = torch_iqn_loss(th, torch.tensor(T), tau, kappa)
    loss.backward()
    np.testing.assert_allclose(tl.detach().numpy(), lb, rtol=1e-13)
    np.testing.assert_allclose(th.grad.numpy(), g, rtol=1e-12, atol=1e-15)
    assert abs(loss.item() - lb.mean()) < 1e-13


def test_the_fold_identity():
    """theta is linear in phi: the mean of theta over any fixed set of tau is the plain head over phibar * W_q, exactly"""
    fc, A, K = 128, 3, 32
    rng = np.random.default_rng(3)
    p = torch.tensor(rng.normal(size=iqn_bounds(fc, A)[-1][2]) * 0.05)
    h = torch.tensor(np.abs(rng.normal(size=(6, fc))))
    for eta in (1.0, 0.25):
        qbar = qbar_from_h(p, h, K, eta, fc, A)
        Wq, bq, _, _ = head_parts(p, fc, A)
        phibar = F.relu(pre64(p, tau_grid(K, eta), fc, A)).mean(0)
        assert (F.relu(pre64(p, tau_grid(K, eta), fc, A)) == 0).any()              # both sides of phi's ReLU occur
        folded = h @ (phibar[:, None] * Wq) + bq
        assert (qbar - folded).abs().max().item() < 1e-14
    g1, g4 = tau_grid(K, 1.0), tau_grid(K, 0.25)
    assert g1[0] == F32(1 / 64) and g1[-1] == F32(63 / 64) and g4[-1] == F32(0.25 * 63 / 64) and (np.diff(g1) > 0).all()


def test_iqn_forward64_reads_the_layout_and_starts_as_the_plain_net():
    fc, A = 128, 2
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    n = b["b_e"][1]
    assert n == n_plain(fc, A) + E * fc + fc
    rng = np.random.default_rng(0)
    p = torch.tensor(rng.normal(size=n) * 0.05)
    s = (rng.random((4, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    tau = rng.random((4, 5)).astype(F32)
    from tests.test_oracle_qnet import torch_forward
    plain = torch_forward(p[:n_plain(fc, A)], torch.as_tensor(s, dtype=torch.float64), fc, A, False)
    p1 = p.clone()
    p1[b["W_e"][0]:b["W_e"][1]] = 0
    p1[b["b_e"][0]:b["b_e"][1]] = 1
    th = iqn_forward64(p1, s, tau, fc, A)
    assert th.shape == (4, 5, A) and (th - plain[:, None, :]).abs().max().item() < 1e-12      # W_e = 0, b_e = 1: phi = 1
    j0 = 3                                                       # W_e one-hot in row j0, b_e = 0: phi = relu(cos(pi j0 tau))
    p2 = p1.clone()
    p2[b["b_e"][0]:b["b_e"][1]] = 0
    p2[b["W_e"][0] + j0 * fc:b["W_e"][0] + (j0 + 1) * fc] = 1
    th2 = iqn_forward64(p2, s, tau, fc, A)
    bq = p[b["b_q"][0]:b["b_q"][1]]
    want = torch.relu(torch.cos(torch.as_tensor(np.pi * j0 * tau.astype(np.float64))))[:, :, None] * (plain - bq)[:, None, :] + bq
    assert (th2 - want).abs().max().item() < 1e-12


def test_np_draw_taus_is_exact_and_inside_the_unit_interval():
    t0, t1 = np_draw_taus(3, 8, 5, (1 << 32) + 7, 0), np_draw_taus(3, 8, 5, (1 << 32) + 7, 1)
    assert ((t0 > 0) & (t0 < 1)).all() and not np.array_equal(t0, t1)
    assert np.array_equal((t0.astype(np.float64) * 2 ** 24) % 2, np.ones_like(t0, np.float64))      # odd multiples of 2^-24: exact
    assert philox(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)            # Random123's known answer


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_check_iqn():
    from dqnflappybird_amd import vec
    assert vec.check_iqn(8, 8, 32, 1.0) == (8, 8, 32, 1.0, 1.0)
    assert vec.check_iqn(1, 64, 1, 0.5, 0.25, 8) == (1, 64, 1, 0.5, 0.25)
    for args, msg in (((0, 8, 32, 1.0), "n_tau must be an integer in 1..64"), ((65, 8, 32, 1.0), "n_tau must be"),
                      ((8, 0, 32, 1.0), "n_tau_next must be an integer in 1..64"), ((8, 8, 65, 1.0), "n_tau_act must be an integer in 1..64"),
                      ((8, 8.5, 32, 1.0), "n_tau_next must be an integer"), ((8, 8, 32, 0.0), "kappa must be finite and > 0"),
                      ((8, 8, 32, float("nan")), "kappa must be"), ((8, 8, 32, 1e39), "kappa must be"),
                      ((8, 8, 32, 1.0, 0.0), "eta \\(CVaR level\\) must be in \\(0, 1\\]"), ((8, 8, 32, 1.0, 1.5), "eta"),
                      ((8, 8, 32, 1.0, float("nan")), "eta")):
        with pytest.raises(ValueError, match=msg):
            vec.check_iqn(*args)
    for A in (1, 9):
        with pytest.raises(ValueError, match="actions must be in 2..8"):
            vec.check_iqn(8, 8, 32, 1.0, 1.0, A)
    assert "iqn" in vec.QNet.ARCHS and vec.IQN_DEFAULTS == (8, 8, 32, 1.0)
    assert "iqn" not in vec.ALGOS                                    # the IQN loop is a module of its own, not a VecBrain algo


@pytest.mark.parametrize("kw,msg", [
    (dict(batch=0), "batch must be in 1..256"),
    (dict(batch=257), "batch must be in 1..256"),
    (dict(batch=64), "batch 64 > n_envs 32"),
    (dict(n_tau=0), "n_tau must be an integer in 1..64"),
    (dict(n_tau_next=65), "n_tau_next must be an integer in 1..64"),
    (dict(n_tau_act=0), "n_tau_act must be an integer in 1..64"),
    (dict(kappa=0), "kappa must be finite and > 0"),
    (dict(cvar=0), "eta \\(CVaR level\\) must be in"),
    (dict(n_step=0), "n_step must be in 1..16"),
    (dict(n_step=17), "n_step must be in 1..16"),
    (dict(polyak=1.5), "polyak \\(rho\\) must be in"),
    (dict(replace_target_iter=0), "replace_target_iter must be >= 1"),
    (dict(observe=-1), "observe must be >= 0"),
    (dict(observe=1, n_step=3), "observe must be >= n_step - 1 = 2"),
    (dict(explore=0), "explore must be >= 1"),
    (dict(initial_epsilon=0.1, final_epsilon=0.2), "the epsilon schedule needs"),
    (dict(gamma=1.5), "gamma must be in \\[0, 1\\]"),
    (dict(lr=0.0), "lr must be finite and > 0"),
    (dict(max_grad_norm=-1), "max_grad_norm must be finite and >= 0"),
    (dict(capacity=40), "capacity 40 < max\\(2, n_step\\) x n_envs = 64"),
])
def test_vec_iqn_refusals_before_the_gpu(kw, msg):
    from dqnflappybird_amd.veciqn import VecIQN
    with pytest.raises(ValueError, match=msg):
        VecIQN(32, **kw)
    with pytest.raises(ValueError, match="n_envs must be >= 1"):
        VecIQN(0)


def test_checkpoints_of_the_four_loops_refuse_each_other(tmp_path):
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain, checkpoint_head
    from dqnflappybird_amd.veciqn import VecIQN
    from dqnflappybird_amd.vecsac import VecSAC
    files = {}
    for head in ("iqn", "sac", "ac", None):
        files[head] = str(tmp_path / f"{head}.npz")
        kw = {} if head is None else dict(head=np.array([head]))
        np.savez(files[head], online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 0], np.int64), **kw)
    assert checkpoint_head(np.load(files["iqn"])) == "iqn"
    vb = VecBrain.__new__(VecBrain)                              # (load refuses before it touches anything of the object but world)
    vb.world = 1
    with pytest.raises(ValueError, match="holds an iqn head \\(a VecIQN's\\), this is a VecBrain"):
        vb.load(files["iqn"])
    with pytest.raises(ValueError, match="holds a iqn head .*this is a VecActorCritic"):
        VecActorCritic.__new__(VecActorCritic).load(files["iqn"])
    with pytest.raises(ValueError, match="holds a iqn head \\(another loop's\\), this is a VecSAC"):
        VecSAC.__new__(VecSAC).load(files["iqn"])
    vi = VecIQN.__new__(VecIQN)
    for head, name in (("sac", "sac"), ("ac", "ac"), (None, "scalar")):
        with pytest.raises(ValueError, match=f"holds a {name} head \\(another loop's\\), this is a VecIQN"):
            vi.load(files[head])


@pytest.mark.parametrize("argv,msg", [
    (["--model", "iqn"], "--model iqn needs --vec"),
    (["--model", "iqn", "--vec", "32", "--n-tau", "0"], "n_tau must be an integer in 1..64"),
    (["--model", "iqn", "--vec", "32", "--n-tau-target", "65"], "n_tau_next must be an integer in 1..64"),
    (["--model", "iqn", "--vec", "32", "--n-tau-act", "100"], "n_tau_act must be an integer in 1..64"),
    (["--model", "iqn", "--vec", "32", "--kappa", "0"], "kappa must be finite and > 0"),
    (["--model", "iqn", "--vec", "32", "--cvar", "1.5"], "eta (CVaR level) must be in (0, 1]"),
    (["--model", "iqn", "--vec", "32", "--n-step", "17"], "n_step must be in 1..16"),
    (["--model", "iqn", "--vec", "32", "--polyak", "2"], "polyak (rho) must be in"),
    (["--model", "iqn", "--vec", "32", "--max-grad-norm", "-2"], "max_grad_norm must be finite and >= 0"),
    (["--model", "iqn", "--vec", "32", "--noisy"], "--noisy is not an option of --model iqn"),
    (["--model", "iqn", "--vec", "32", "--huber", "1"], "--huber is not an option of --model iqn"),
    (["--model", "iqn", "--vec", "32", "--n-quantiles", "8"], "--n-quantiles is not an option of --model iqn"),
    (["--model", "iqn", "--vec", "32", "--tau", "0.1"], "--tau / --alpha / --clip is not an option of --model iqn"),
    (["--model", "iqn", "--vec", "32", "--alpha-lr", "0.1"], "--alpha-lr need --model sac"),
    (["--model", "iqn", "--vec", "32", "--rollout", "5"], "--rollout need --model a2c"),
    (["--model", "qrdqn", "--vec", "32", "--n-tau", "4"], "--n-tau need --model iqn"),
    (["--model", "sac", "--vec", "32", "--cvar", "0.5"], "--cvar need --model iqn"),
    (["--model", "ddqn", "--vec", "32", "--double"], "--double need --model iqn"),
])
def test_cli_iqn_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
