"""Discrete soft actor-critic, the host side: the ABI's declarations, a float32 numpy restatement of the pinned train step against
float64 torch autograd, the float64 forward that reads the three-head layout, and every refusal that needs no GPU (check_sac, VecSAC,
the command line, the checkpoints of the three loops).  tests/test_gpu_sac.py imports the helpers."""
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


def sac_bounds(fc, A):
    """[(name, lo, hi)] of every parameter tensor of a SAC net's flat vector (include/fbdqn.h), in order"""
    sizes = [("W_conv1", 8192), ("b_conv1", 32), ("W_conv2", 32768), ("b_conv2", 64), ("W_conv3", 36864), ("b_conv3", 64),
             ("W_fc1", 1600 * fc), ("b_fc1", fc), ("W_pi", fc * A), ("b_pi", A), ("W_q1", fc * A), ("b_q1", A), ("W_q2", fc * A), ("b_q2", A)]
    out, o = [], 0
    for name, k in sizes:
        out.append((name, o, o + k))
        o += k
    return out


def sac_forward64(p, states, fc, A):
    """the SAC net in float64 torch: tests/test_oracle_qnet.py::torch_forward's layers, then the three RAW heads.  p: a float64 tensor
    (requires_grad for gradients), states u8 [B, 80, 80, 4] -> (logits, Q1, Q2), each [B, A]"""
    n_plain = 77984 + 1600 * fc + fc + fc * A + A
    w = split(p[:n_plain], fc, A, False)
    x = torch.as_tensor(np.array(states), dtype=torch.float64).permute(0, 3, 1, 2)
    h = F.relu(F.conv2d(x, w["w1"].permute(3, 2, 0, 1), w["b1"], stride=4, padding=2))
    h = F.max_pool2d(h, 2, 2)
    h = F.relu(F.conv2d(h, w["w2"].permute(3, 2, 0, 1), w["b2"], stride=2, padding=1))
    h = F.relu(F.conv2d(h, w["w3"].permute(3, 2, 0, 1), w["b3"], stride=1, padding=1))
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], 1600)
    h = F.relu(h @ w["wf1"] + w["bf1"])
    b = {n: (lo, hi) for n, lo, hi in sac_bounds(fc, A)}
    head = lambda wn, bn: h @ p[b[wn][0]:b[wn][1]].view(fc, A) + p[b[bn][0]:b[bn][1]]
    assert b["b_q2"][1] == p.numel()
    return h @ w["wq"] + w["bq"], head("W_q1", "b_q1"), head("W_q2", "b_q2")


def np_softmax32(z):
    """the pinned float32 softmax, ascending c -> (p, log p)"""
    z = np.asarray(z, F32)
    m = z.max(1)
    e = np.exp((z - m[:, None]).astype(F32)).astype(F32)
    s = np.zeros(len(z), F32)
    for c in range(z.shape[1]):
        s = (s + e[:, c]).astype(F32)
    lse = (m + np.log(s).astype(F32)).astype(F32)
    return (e / s[:, None]).astype(F32), (z - lse[:, None]).astype(F32)


def np_soft_value(p, lp, q1, q2, alpha):
    """V = sum_c p_c (min(Q1_c, Q2_c) - alpha log p_c), float32, ascending c from 0"""
    V = np.zeros(len(p), F32)
    for c in range(p.shape[1]):
        V = (V + p[:, c] * (np.minimum(q1[:, c], q2[:, c]) - F32(alpha) * lp[:, c]).astype(F32)).astype(F32)
    return V


def np_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha):
    """the SAC train step of include/fbdqn.h from the head outputs, in float32 and the pinned order: z / q1 / q2 of s (online), zn of s'
    (online), q1n / q2n of s' (target), each [B, A] -> (loss[6], dLoss/dz, dLoss/dQ1, dLoss/dQ2 (each [B, A]), y [B])"""
    z, q1, q2, zn, q1n, q2n = (np.asarray(x, F32) for x in (z, q1, q2, zn, q1n, q2n))
    B, A = z.shape
    a = np.minimum(np.asarray(a, np.int64), A - 1)
    al, Bf = F32(alpha), F32(B)
    pn, lpn = np_softmax32(zn)
    Vn = np_soft_value(pn, lpn, q1n, q2n, al)
    rd = np.where(np.asarray(r, F32) == F32(0.1), 0.1, np.asarray(r, F32).astype(np.float64))
    y = np.where(np.asarray(t) != 0, rd, rd + float(gamma) * Vn.astype(np.float64)).astype(F32)
    ar = np.arange(B)
    d1, d2 = (q1[ar, a] - y).astype(F32), (q2[ar, a] - y).astype(F32)
    dq1, dq2 = np.zeros_like(z), np.zeros_like(z)
    dq1[ar, a] = ((F32(2) * d1).astype(F32) / Bf).astype(F32)
    dq2[ar, a] = ((F32(2) * d2).astype(F32) / Bf).astype(F32)
    p, lp = np_softmax32(z)
    f = ((al * lp).astype(F32) - np.minimum(q1, q2)).astype(F32)
    Lpi, H = np.zeros(B, F32), np.zeros(B, F32)
    for c in range(A):
        Lpi = (Lpi + (p[:, c] * f[:, c]).astype(F32)).astype(F32)
        H = (H - (p[:, c] * lp[:, c]).astype(F32)).astype(F32)
    dz = ((p * (f - Lpi[:, None]).astype(F32)).astype(F32) / Bf).astype(F32)

    def mean(x):
        s = F32(0)
        for v in x:
            s = F32(s + v)
        return F32(s / Bf)
    m1, m2, mp, mh = mean((d1 * d1).astype(F32)), mean((d2 * d2).astype(F32)), mean(Lpi), mean(H)
    return np.array([F32(F32(m1 + m2) + mp), m1, m2, mp, mh, al], F32), dz, dq1, dq2, y


def torch_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha):
    """the same step in float64 torch, written from the paper's formulas: -> (total, mean d1^2, mean d2^2, mean L_pi, mean H, y);
    the total's autograd gradient is the step's (y and min Q are constants)"""
    B, A = z.shape
    a = torch.as_tensor(np.minimum(np.asarray(a, np.int64), A - 1))
    lpn = torch.log_softmax(zn, 1)
    Vn = (lpn.exp() * (torch.minimum(q1n, q2n) - alpha * lpn)).sum(1)
    rd = torch.as_tensor(np.where(np.asarray(r, F32) == F32(0.1), 0.1, np.asarray(r, np.float64)))
    nd = torch.as_tensor((np.asarray(t) == 0).astype(np.float64))
    y = (rd + nd * gamma * Vn).detach()
    ar = torch.arange(B)
    l1, l2 = ((q1[ar, a] - y) ** 2).mean(), ((q2[ar, a] - y) ** 2).mean()
    lp = torch.log_softmax(z, 1)
    lpi = (lp.exp() * (alpha * lp - torch.minimum(q1, q2).detach())).sum(1).mean()
    H = -(lp.exp() * lp).sum(1).mean()
    return l1 + l2 + lpi, l1, l2, lpi, H, y


def np_alpha_adam(state, mh, target_entropy, alpha_lr, b1=0.9, b2=0.999, eps=1e-8):
    """one temperature step of include/fbdqn.h on (log alpha, m, v, pow1, pow2), float32 in the pinned order"""
    la, m, v, p1, p2 = (F32(x) for x in state)
    b1, b2, eps, one = F32(b1), F32(b2), F32(eps), F32(1)
    g = F32(F32(mh) - F32(target_entropy))
    at = F32(F32(F32(alpha_lr) * np.sqrt(F32(one - p2))) / F32(one - p1))
    p1, p2 = F32(p1 * b1), F32(p2 * b2)
    m = F32(m + F32(F32(g - m) * F32(one - b1)))
    v = F32(v + F32(F32(F32(g * g) - v) * F32(one - b2)))
    la = F32(la - F32(F32(m * at) / F32(np.sqrt(v) + eps)))
    return np.array([la, m, v, p1, p2], F32)


def sac_heads(rng, B, A, scale=2.0):
    """six random head outputs [B, A] (float32) with both orders of Q1 / Q2 at s and at s', actions, rewards of both kinds, terminals"""
    z, q1, q2, zn, q1n, q2n = ((rng.normal(size=(B, A)) * scale).astype(F32) for _ in range(6))
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], F32), B, p=[0.6, 0.2, 0.2])
    t = (rng.random(B) < 0.3).astype(np.uint8)
    if B > 1:
        t[0], t[1] = 1, 0
    return z, q1, q2, zn, q1n, q2n, a, r, t


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_sac_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ARCH_SAC 7", "int fb_qnet_create_sac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out);",
                 "int fb_qnet_set_sac(fb_qnet_t h, float alpha, float target_entropy, float alpha_lr);",
                 "int fb_qnet_get_sac(fb_qnet_t h, float *alpha_host, float *target_entropy_host, float *alpha_lr_host);",
                 "int fb_qnet_get_sac_state(", "int fb_qnet_set_sac_state(", "int fb_qnet_forward_sac(", "int fb_qnet_sac_train_step(",
                 "int fb_sac_train_from_replay(", "int fb_sac_step("):
        assert decl in hdr, decl
    assert L.ARCH_SAC == 7 and L.SAC_DEFAULTS == (0.2, 0.98, 0.0)
    want = {"fb_qnet_create_sac": 4, "fb_qnet_set_sac": 4, "fb_qnet_get_sac": 4, "fb_qnet_get_sac_state": 2, "fb_qnet_set_sac_state": 2,
            "fb_qnet_forward_sac": 8, "fb_qnet_sac_train_step": 12, "fb_sac_train_from_replay": 12, "fb_sac_step": 12}
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n, name
    for word in ("not offered data-parallel SAC", "log alpha -= (m * at) / (sqrtf(v) + eps)", "fminf(Q1_c, Q2_c) - alpha * log p_c"):
        assert word in hdr, word


# ---------------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("alpha", [0.2, 1e-3, 5.0])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_np_sac_loss_gradients_equal_autograd(A, alpha):
    """float32 in the pinned order against float64 autograd: the bound is float32's -- the losses to 1e-5 relative, a gradient element
    to 2e-6 of its tensor's largest (sums of at most 8 float32 products, eps 6e-8 each, with head outputs of magnitude <= ~8)"""
    B = 37
    rng = np.random.default_rng(100 * A + int(alpha * 1000))
    z, q1, q2, zn, q1n, q2n, a, r, t = sac_heads(rng, B, A)
    a[3] = A + 1                                                     # an action past the head reads A - 1
    assert (q1 < q2).any() and (q1 > q2).any() and (q1n < q2n).any() and (q1n > q2n).any() and t.any() and not t.all()
    loss, dz, dq1, dq2, y = np_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, alpha)
    tz, tq1, tq2 = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (z, q1, q2))
    tn = [torch.tensor(x.astype(np.float64), requires_grad=True) for x in (zn, q1n, q2n)]
    out = torch_sac_loss(tz, tq1, tq2, *tn, a, r, t, 0.99, float(F32(alpha)))
    out[0].backward()
    assert all(x.grad is None for x in tn)                           # no gradient through the target
    np.testing.assert_allclose(loss[:5], [o.item() for o in out[:5]], rtol=1e-5, atol=1e-6)
    assert loss[5] == F32(alpha)
    np.testing.assert_allclose(y, out[5].numpy(), rtol=1e-6, atol=1e-6)
    for got, ref in ((dz, tz.grad), (dq1, tq1.grad), (dq2, tq2.grad)):
        ref = ref.numpy()
        assert np.abs(ref).max() > 0
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * np.abs(ref).max())
    assert (dq1 != 0).sum() <= B and (d := dq1[np.arange(B), np.minimum(a, A - 1)]).all() and (d > 0).any() and (d < 0).any()
    assert np.array_equal(y[t != 0], np.where(r == F32(0.1), 0.1, r.astype(np.float64))[t != 0].astype(F32))


def test_np_alpha_adam_is_adam_on_log_alpha():
    """five steps of the pinned expression against float64 Adam (TF form) with the same gradients"""
    st = np.array([np.log(F32(0.2)), 0, 0, 0.9, 0.999], F32)
    la, m, v, p1, p2 = float(st[0]), 0.0, 0.0, 0.9, 0.999
    for mh in (0.69, 0.6, 0.71, 0.3, 0.68):
        st = np_alpha_adam(st, mh, 0.5, 1e-3)
        g = float(F32(mh)) - 0.5
        at = 1e-3 * np.sqrt(1 - p2) / (1 - p1)
        p1, p2 = p1 * 0.9, p2 * 0.999
        m, v = m + (g - m) * 0.1, v + (g * g - v) * 0.001
        la -= m * at / (np.sqrt(v) + 1e-8)
        np.testing.assert_allclose(st, [la, m, v, p1, p2], rtol=2e-5)
    assert st[0] < np.log(0.2)                                       # the entropy sat above its target: alpha fell


def test_sac_forward64_reads_the_three_head_layout():
    fc, A = 128, 3
    b = sac_bounds(fc, A)
    n = b[-1][2]
    assert n == 77984 + 1600 * fc + fc + 3 * (fc * A + A)
    rng = np.random.default_rng(0)
    p = torch.tensor(rng.normal(size=n) * 0.05)
    s = (rng.random((4, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    z, q1, q2 = sac_forward64(p, s, fc, A)
    from tests.test_oracle_qnet import torch_forward
    x = torch.as_tensor(s, dtype=torch.float64)
    tb = {name: (lo, hi) for name, lo, hi in b}
    plain = lambda wn, bn: torch.cat([p[:tb["W_pi"][0]], p[tb[wn][0]:tb[wn][1]], p[tb[bn][0]:tb[bn][1]]])
    for got, (wn, bn) in ((z, ("W_pi", "b_pi")), (q1, ("W_q1", "b_q1")), (q2, ("W_q2", "b_q2"))):
        assert torch.allclose(got, torch_forward(plain(wn, bn), x, fc, A, False), rtol=0, atol=1e-12), wn
    assert not torch.equal(q1, q2)


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_check_sac():
    from dqnflappybird_amd import vec
    a, h, lr = vec.check_sac(0.2, None, 0)
    assert (a, lr) == (float(F32(0.2)), 0.0) and h == float(F32(0.98) * np.log(F32(2)))
    assert vec.check_sac(1, -0.5, 1e-3, 8) == (1.0, -0.5, float(F32(1e-3)))
    for args, msg in (((0.0, None, 0), "alpha must be finite and > 0"), ((-1, None, 0), "alpha must be"), ((float("nan"), None, 0), "alpha must be"),
                      ((1e39, None, 0), "alpha must be"), ((0.2, float("inf"), 0), "target_entropy must be finite"),
                      ((0.2, float("nan"), 0), "target_entropy"), ((0.2, None, -1e-3), "alpha_lr must be finite and >= 0"),
                      ((0.2, None, float("nan")), "alpha_lr")):
        with pytest.raises(ValueError, match=msg):
            vec.check_sac(*args)
    for A in (1, 9):
        with pytest.raises(ValueError, match="actions must be in 2..8"):
            vec.check_sac(0.2, None, 0, A)
    assert "sac" in vec.QNet.ARCHS and vec.SAC_DEFAULTS == (0.2, 0.98, 0.0)


@pytest.mark.parametrize("kw,msg", [
    (dict(batch=0), "batch must be in 1..256"),
    (dict(batch=257), "batch must be in 1..256"),
    (dict(batch=64), "batch 64 > n_envs 32"),
    (dict(alpha=0), "alpha must be finite and > 0"),
    (dict(target_entropy=float("nan")), "target_entropy must be finite"),
    (dict(alpha_lr=-1), "alpha_lr must be finite and >= 0"),
    (dict(polyak=1.5), "polyak \\(rho\\) must be in"),
    (dict(observe=-1), "observe must be >= 0"),
    (dict(gamma=1.5), "gamma must be in \\[0, 1\\]"),
    (dict(lr=0.0), "lr must be finite and > 0"),
    (dict(max_grad_norm=-1), "max_grad_norm must be finite and >= 0"),
    (dict(capacity=40), "capacity 40 < 2 x n_envs = 64"),
])
def test_vec_sac_refusals_before_the_gpu(kw, msg):
    from dqnflappybird_amd.vecsac import VecSAC
    with pytest.raises(ValueError, match=msg):
        VecSAC(32, **kw)
    with pytest.raises(ValueError, match="n_envs must be >= 1"):
        VecSAC(0)


def test_checkpoints_of_the_three_loops_refuse_each_other(tmp_path):
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain, checkpoint_head
    from dqnflappybird_amd.vecsac import VecSAC
    files = {}
    for head in ("sac", "ac", None):
        files[head] = str(tmp_path / f"{head}.npz")
        kw = {} if head is None else dict(head=np.array([head]))
        np.savez(files[head], online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 0], np.int64), **kw)
    assert checkpoint_head(np.load(files["sac"])) == "sac"
    vb = VecBrain.__new__(VecBrain)                              # (load refuses before it touches anything of the object but world)
    vb.world = 1
    with pytest.raises(ValueError, match="holds a sac head \\(a VecSAC's\\), this is a VecBrain"):
        vb.load(files["sac"])
    with pytest.raises(ValueError, match="holds a sac head .*this is a VecActorCritic"):
        VecActorCritic.__new__(VecActorCritic).load(files["sac"])
    vs = VecSAC.__new__(VecSAC)
    with pytest.raises(ValueError, match="holds a ac head \\(another loop's\\), this is a VecSAC"):
        vs.load(files["ac"])
    with pytest.raises(ValueError, match="holds a scalar head \\(another loop's\\), this is a VecSAC"):
        vs.load(files[None])


@pytest.mark.parametrize("argv,msg", [
    (["--model", "sac"], "--model sac needs --vec"),
    (["--model", "sac", "--vec", "32", "--alpha", "0"], "alpha must be finite and > 0"),
    (["--model", "sac", "--vec", "32", "--alpha", "nan"], "alpha must be finite and > 0"),
    (["--model", "sac", "--vec", "32", "--target-entropy", "inf"], "target_entropy must be finite"),
    (["--model", "sac", "--vec", "32", "--alpha-lr", "-1"], "alpha_lr must be finite and >= 0"),
    (["--model", "sac", "--vec", "32", "--polyak", "2"], "polyak (rho) must be in"),
    (["--model", "sac", "--vec", "32", "--max-grad-norm", "-2"], "max_grad_norm must be finite and >= 0"),
    (["--model", "sac", "--vec", "32", "--noisy"], "--noisy is not an option of --model sac"),
    (["--model", "sac", "--vec", "32", "--n-step", "3"], "--n-step is not an option of --model sac"),
    (["--model", "sac", "--vec", "32", "--huber", "1"], "--huber"),
    (["--model", "sac", "--vec", "32", "--tau", "0.1"], "--tau / --clip is not an option of --model sac"),
    (["--model", "ddqn", "--vec", "32", "--alpha-lr", "0.001"], "--alpha-lr need --model sac"),
    (["--model", "a2c", "--vec", "32", "--target-entropy", "0.5"], "--target-entropy need --model sac"),
])
def test_cli_sac_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
