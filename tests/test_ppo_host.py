"""PPO on the actor-critic rollout (include/fbdqn.h: fb_qnet_ppo_train_step and its block) without a GPU: the ABI declarations; the
float64 / numpy restatements the GPU tests compare the kernels with -- np_ppo_loss's analytic gradients against torch autograd,
np_permute (the keyed Feistel permutation, on the oracle's Philox), np_normalize (the pinned summation order of fb_ac_normalize_adv)
-- and every refusal the Python layers make before anything touches the GPU."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_ac_host import ROOT

M32 = 0xFFFFFFFF
STREAM_PERM = 9
RSTAR = (0.5, 0.85, 1.0, 1.15, 2.0)          # the ratios the gradient tests place their samples at: each >= 0.05 from 1 +- 0.2
DSTAR = (0.05, -0.05, 0.5, -0.5)             # ... and V - value_old: each >= 0.15 from +- 0.2


# ---------------------------------------------------------------------------------------------------------------- restatements
def np_ppo_loss(z, V, a, adv, ret, logp_old, value_old, n_total, cv, ce, eps, vclip):
    """the PPO loss of include/fbdqn.h in float64 from logits z [B, A] and values V [B] -> (loss[6], dLoss/dz [B, A], dLoss/dV [B])"""
    z, V, adv, ret, lpo, vo = (np.asarray(x, np.float64) for x in (z, V, adv, ret, logp_old, value_old))
    a = np.asarray(a, np.int64)
    B = len(a)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    p, lp = e / s, z - (m + np.log(s))
    H = -(p * lp).sum(1)
    lr = lp[np.arange(B), a] - lpo
    r, lo, hi = np.exp(lr), 1.0 - eps, 1.0 + eps
    s1, s2 = r * adv, np.minimum(np.maximum(r, lo), hi) * adv
    lpi, w = -np.minimum(s1, s2), np.where(s1 <= s2, s1, 0.0)
    onehot = np.zeros_like(z)
    onehot[np.arange(B), a] = 1.0
    dz = (w[:, None] * (p - onehot) + ce * p * (lp + H[:, None])) / n_total
    e1, d = V - ret, V - vo
    plain = (abs(d) <= vclip) if vclip else np.ones(B, bool)
    e2 = (vo + np.copysign(vclip, d)) - ret
    lv = np.where(plain, e1 ** 2, np.maximum(e1 ** 2, e2 ** 2))
    dV = np.where(plain | (e1 ** 2 >= e2 ** 2), 2.0 * cv * e1 / n_total, 0.0)
    parts = np.array([lpi.sum(), lv.sum(), H.sum(), ((r < lo) | (r > hi)).sum(), ((r - 1.0) - lr).sum()]) / n_total
    return np.array([parts[0] + cv * parts[1] - ce * parts[2], *parts]), dz, dV


def torch_ppo_terms(z, V, a, adv, ret, logp_old, value_old, eps, vclip):
    """(sum L_pi, sum L_v, sum H) as float64 torch scalars, written the way PPO implementations write them (min of the two surrogates,
    max of the two squared errors) and differentiated by autograd; then sum 1{clipped} and sum ((r - 1) - log r) as floats"""
    t = lambda x: torch.as_tensor(np.asarray(x, np.float64))
    lp = torch.log_softmax(z, 1)
    H = -(lp.exp() * lp).sum(1)
    a = torch.as_tensor(np.asarray(a, np.int64))
    lr = lp[torch.arange(len(a)), a] - t(logp_old)
    r = lr.exp()
    lpi = -torch.minimum(r * t(adv), r.clamp(1.0 - eps, 1.0 + eps) * t(adv))
    lv = (V - t(ret)) ** 2
    if vclip:
        vc = t(value_old) + (V - t(value_old)).clamp(-vclip, vclip)
        lv = torch.maximum(lv, (vc - t(ret)) ** 2)
    clipped = ((r < 1.0 - eps) | (r > 1.0 + eps)).sum().item()
    return lpi.sum(), lv.sum(), H.sum(), float(clipped), ((r - 1.0) - lr).sum().item()


def ppo_targets(z64, V64, rng, eps=0.2, vclip=0.2):
    """a batch's (a, adv, ret, logp_old, value_old) placed clear of the loss's kinks ON THE FLOAT64 FORWARD (z64 [B, A], V64 [B]):
    sample b sits at the ratio RSTAR[b % 5] and at V - value_old = DSTAR[b % 4]; the advantages' sign alternates from one pass over the
    five ratios to the next, so both signs meet every ratio from B = 10 on; ret is redrawn until the two squared errors of the clipped
    value term differ by >= 0.05 in their roots (for value_clip = vclip; a sample inside the clip has no such kink).  Every sample is kept"""
    z64, V64 = np.asarray(z64, np.float64), np.asarray(V64, np.float64)
    B, A = z64.shape
    a = rng.integers(0, A, B).astype(np.uint8)
    lp = z64 - (z64.max(1, keepdims=True) + np.log(np.exp(z64 - z64.max(1, keepdims=True)).sum(1, keepdims=True)))
    rs = np.array([RSTAR[b % 5] for b in range(B)])
    ds = np.array([DSTAR[b % 4] for b in range(B)])
    adv = ((0.25 + np.abs(rng.normal(size=B)) * 2) * np.where((np.arange(B) // 5) % 2 == 0, 1.0, -1.0)).astype(np.float32)
    logp_old = (lp[np.arange(B), a] - np.log(rs)).astype(np.float32)
    value_old = (V64 - ds).astype(np.float32)
    ret = np.empty(B, np.float32)
    for b in range(B):
        while True:
            ret[b] = np.float32(V64[b] + rng.normal())
            e1 = V64[b] - float(ret[b])
            e2 = (float(value_old[b]) + np.copysign(vclip, ds[b])) - float(ret[b])
            if abs(ds[b]) <= vclip or abs(abs(e1) - abs(e2)) >= 0.05:
                break
    r = np.exp(lp[np.arange(B), a] - logp_old.astype(np.float64))
    assert (np.abs(r - (1 - eps)) >= 0.049).all() and (np.abs(r - (1 + eps)) >= 0.049).all()
    assert (np.abs(np.abs(V64 - value_old.astype(np.float64)) - vclip) >= 0.149).all()
    return a, adv, ret, logp_old, value_old


def np_permute(oracle, n, seed, draw):
    """fb_ac_permute in numpy (include/fbdqn.h): the 4-round Feistel network on k = 2 half bits over the oracle's Philox, cycle-walked"""
    k = 2
    while (1 << k) < n:
        k += 2
    half = k // 2
    mask = (1 << half) - 1
    F = np.array([oracle.philox(seed & M32, seed >> 32, R, draw & M32, STREAM_PERM, draw >> 32) for R in range(1 << half)], np.int64) & mask

    def encrypt(x):
        L, R = x >> half, x & mask
        for rnd in range(4):
            L, R = R, L ^ F[R, rnd]
        return (L << half) | R

    y = encrypt(np.arange(n, dtype=np.int64))
    while (y >= n).any():
        bad = y >= n
        y[bad] = encrypt(y[bad])
    return y


def _two_level_sum(v):
    """thread t of 256 sums the elements i = t (mod 256) in ascending i, then the 256 partial sums are added in ascending t (float64)"""
    rows = -(-len(v) // 256)
    pad = np.zeros(rows * 256, np.float64)
    pad[:len(v)] = v                                             # (x + 0.0 = x: the padding changes no bit)
    part = np.zeros(256, np.float64)
    for row in pad.reshape(rows, 256):
        part = part + row
    S = np.float64(0.0)
    for t in range(256):
        S = S + part[t]
    return S


def np_normalize(adv):
    """fb_ac_normalize_adv in numpy, operation for operation (float64, the header's order) -> f32 of adv's shape"""
    adv = np.asarray(adv, np.float32)
    x = adv.astype(np.float64).ravel()
    n = np.float64(len(x))
    mean = _two_level_sum(x) / n
    d = x - mean
    sd = np.sqrt(_two_level_sum(d * d) / n)
    return ((x - mean) / (sd + np.float64(1e-8))).astype(np.float32).reshape(adv.shape)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_ppo_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("int fb_qnet_set_ppo(fb_qnet_t h, float clip_eps, float value_clip);",
                 "int fb_qnet_get_ppo(fb_qnet_t h, float *clip_eps_host, float *value_clip_host);",
                 "int fb_qnet_ppo_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret,",
                 "int fb_ppo_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const int64_t *sel, const float *adv,",
                 "int fb_ac_normalize_adv(const float *adv, int64_t n, float *out, void *stream);",
                 "int fb_ac_permute(int64_t n, uint64_t seed, uint64_t draw, int64_t *out, void *stream);",
                 "FB_STREAM_PERM = 9", "s2 = fminf(fmaxf(r, lo), hi) adv", "w = (s1 <= s2) ? s1 : 0", "copysignf(value_clip, d)",
                 "(sd + 1e-8)", "(L, R) <- (R, L ^ (F_r(R) & mask))"):
        assert decl in hdr, decl
    assert "not offered PPO" not in hdr
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "#define FB_STREAM_PERM 9u" in common
    assert L.PPO_DEFAULTS == (0.2, 0.0)
    i, i64, u64, f, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_set_ppo"] == [vp, f, f] and L.SIGNATURES["fb_qnet_get_ppo"] == [vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_ppo_train_step"] == [vp, i, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]
    assert L.SIGNATURES["fb_ppo_train_from_replay"] == [vp, vp, i, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    assert L.SIGNATURES["fb_ac_normalize_adv"] == [vp, i64, vp, vp]
    assert L.SIGNATURES["fb_ac_permute"] == [i64, u64, u64, vp, vp]
    lib = L.lib()                                                # (binds every symbol: a stale library raises here)
    assert lib.fb_qnet_set_ppo(None, 0.2, 0.0) == -1 and "fb_qnet_set_ppo: NULL" in lib.fb_last_error().decode()
    assert lib.fb_ac_permute(0, 1, 2, None, None) == -1 and "fb_ac_permute" in lib.fb_last_error().decode()
    assert lib.fb_ac_normalize_adv(None, 4, None, None) == -1 and "fb_ac_normalize_adv" in lib.fb_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("cv,ce", [(0.5, 0.01), (1.0, 0.5)])
@pytest.mark.parametrize("vclip", [0.0, 0.2])
def test_np_ppo_loss_gradients_equal_autograd(A, cv, ce, vclip):
    rng = np.random.default_rng(10 * A + int(10 * vclip))
    B, nt, eps = 40, 160, 0.2
    z = torch.tensor(rng.normal(size=(B, A)) * 2, dtype=torch.float64, requires_grad=True)
    V = torch.tensor(rng.normal(size=B), dtype=torch.float64, requires_grad=True)
    a, adv, ret, lpo, vo = ppo_targets(z.detach().numpy(), V.detach().numpy(), rng)
    for k in range(5):                                           # both advantage signs meet every ratio
        assert {np.sign(x) for x in adv[k::5]} == {1.0, -1.0}
    lpi, lv, H, nclip, kl = torch_ppo_terms(z, V, a, adv, ret, lpo, vo, eps, vclip)
    loss = (lpi + cv * lv - ce * H) / nt
    loss.backward()
    got, dz, dV = np_ppo_loss(z.detach().numpy(), V.detach().numpy(), a, adv, ret, lpo, vo, nt, cv, ce, eps, vclip)
    np.testing.assert_allclose(got, [loss.item(), lpi.item() / nt, lv.item() / nt, H.item() / nt, nclip / nt, kl / nt], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dz, z.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dV, V.grad.numpy(), rtol=1e-12, atol=1e-14)
    assert got[4] == 16 / nt                                     # the ratios 0.5 and 2 are outside [0.8, 1.2]: two samples in five
    if A > 1:                                                    # clipped AND flat: r = 2 with adv > 0, r = 0.5 with adv < 0: no policy gradient
        flat = np.array([(b % 5 == 4 and adv[b] > 0) or (b % 5 == 0 and adv[b] < 0) for b in range(B)])
        _, dz_pi, _ = np_ppo_loss(z.detach().numpy(), V.detach().numpy(), a, adv, ret, lpo, vo, nt, cv, 0.0, eps, vclip)
        assert flat.any() and not dz_pi[flat].any() and (np.abs(dz_pi[~flat]).max(1) > 0).all()
    if vclip:                                                    # both branches of the clipped value term occur, and some dV are exactly 0
        assert (dV == 0).any() and (dV[np.abs(np.array([DSTAR[b % 4] for b in range(B)])) > vclip] != 0).any()
    else:
        assert (dV != 0).all()


def test_np_ppo_loss_at_ratio_one_is_a2c_with_no_log():
    """logp_old = log p_a (the rollout's own weights): r = 1, nothing clipped, KL 0, and dLoss/dz is A2C's"""
    from tests.test_ac_host import np_ac_loss
    rng = np.random.default_rng(3)
    B, A = 12, 3
    z, V = rng.normal(size=(B, A)), rng.normal(size=B)
    a, adv, ret = rng.integers(0, A, B), rng.normal(size=B), rng.normal(size=B)
    lp = z - (z.max(1, keepdims=True) + np.log(np.exp(z - z.max(1, keepdims=True)).sum(1, keepdims=True)))
    got, dz, dV = np_ppo_loss(z, V, a, adv, ret, lp[np.arange(B), a], V.copy(), B, 0.5, 0.01, 0.2, 0.2)
    want, dz0, dV0 = np_ac_loss(z, V, a, adv, ret, B, 0.5, 0.01)
    np.testing.assert_allclose(dz, dz0, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(dV, dV0, rtol=1e-12, atol=1e-15)
    assert got[4] == 0.0 and got[5] == 0.0 and np.isclose(got[2], want[2]) and np.isclose(got[1], -adv.sum() / B)


# ---------------------------------------------------------------------------------------------------------------- the permutation
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 4097, 5120])
def test_np_permute_is_a_keyed_permutation(oracle, n):
    seed, draw = (7 << 32) | 12345, (1 << 32) + 3
    x = np_permute(oracle, n, seed, draw)
    assert x.dtype == np.int64 and sorted(x.tolist()) == list(range(n))
    assert np.array_equal(np_permute(oracle, n, seed, draw), x)                  # fixed for a fixed key
    if n >= 255:
        others = [np_permute(oracle, n, seed, draw + 1), np_permute(oracle, n, seed + 1, draw), np_permute(oracle, n, seed, draw ^ (1 << 32))]
        assert all(not np.array_equal(o, x) for o in others)                     # each key word matters
        assert (x != np.arange(n)).mean() > 0.9 and (others[0] != x).mean() > 0.9


def test_np_permute_hand_case(oracle):
    """n = 5: k = 4 bits, half = 2; element 0 spelled out round by round"""
    seed, draw = 9, 4
    F = [oracle.philox(seed, 0, R, draw, STREAM_PERM, 0) & 3 for R in range(4)]
    x = 0
    while True:
        L, R = x >> 2, x & 3
        for rnd in range(4):
            L, R = R, L ^ int(F[R][rnd])
        x = (L << 2) | R
        if x < 5:
            break
    assert np_permute(oracle, 5, seed, draw)[0] == x


# ---------------------------------------------------------------------------------------------------------------- the normaliser
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1300])
def test_np_normalize_is_the_pinned_order(n):
    rng = np.random.default_rng(n)
    x = (rng.normal(size=n) * 3 + 1.5).astype(np.float32)
    part = [0.0] * 256
    for i in range(n):                                           # thread i % 256, ascending i
        part[i % 256] += float(x[i])
    S = 0.0
    for t in range(256):
        S += part[t]
    mean = S / n
    part = [0.0] * 256
    for i in range(n):
        d = float(x[i]) - mean
        part[i % 256] += d * d
    Q = 0.0
    for t in range(256):
        Q += part[t]
    sd = float(np.sqrt(np.float64(Q / n)))
    want = np.array([np.float32((float(v) - mean) / (sd + 1e-8)) for v in x], np.float32)
    got = np_normalize(x)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    if n == 1:
        assert got[0] == 0.0
    if n >= 255:
        g = got.astype(np.float64)
        assert abs(g.mean()) < 1e-6 and abs(g.std() - 1.0) < 1e-6


def test_np_normalize_of_a_constant_is_zero():
    for c in (0.0, 3.5, -0.1):
        assert not np_normalize(np.full(700, c, np.float32)).any()
    assert np_normalize(np.ones((5, 7), np.float32)).shape == (5, 7)


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_value_checks():
    from dqnflappybird_amd import vec
    from dqnflappybird_amd.vecac import check_ppo_args
    assert vec.check_ppo(0.2, 0) == (float(np.float32(0.2)), 0.0) and vec.check_ppo(1e-3, 10.0) == (float(np.float32(1e-3)), 10.0)
    for args, msg in (((0.0, 0.0), "clip_eps"), ((-0.2, 0.0), "clip_eps"), ((float("nan"), 0.0), "clip_eps"), ((float("inf"), 0.0), "clip_eps"),
                      ((1e39, 0.0), "clip_eps"), ((0.2, -1e-3), "value_clip"), ((0.2, float("nan")), "value_clip"), ((0.2, float("inf")), "value_clip")):
        with pytest.raises(ValueError, match=msg + " must be finite"):
            vec.check_ppo(*args)
    assert vec.PPO_DEFAULTS == (0.2, 0.0)
    assert check_ppo_args(16, 4, 2, 2, 0.2, 0.0) == (2, 2, float(np.float32(0.2)), 0.0)
    for args, msg in (((16, 4, 0, 2, 0.2, 0.0), "epochs must be >= 1"), ((16, 4, 2, 0, 0.2, 0.0), "minibatches must be >= 1 and divide"),
                      ((16, 4, 2, 3, 0.2, 0.0), "divide rollout x n_envs = 64"), ((16, 4, 2, 2, 0.0, 0.0), "clip_eps")):
        with pytest.raises(ValueError, match=msg):
            check_ppo_args(*args)
    with pytest.raises(ValueError, match="n must be in 1"):
        vec.ac_permute(0)
    with pytest.raises(ValueError, match="n must be in 1"):
        vec.ac_permute(2 ** 31)


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="trpo"), "algo must be one of"),
    (dict(algo="ppo", epochs=0), "epochs must be >= 1"),
    (dict(algo="ppo", minibatches=3), "minibatches must be >= 1 and divide rollout x n_envs = 80"),
    (dict(algo="ppo", clip_eps=0.0), "clip_eps must be finite and > 0"),
    (dict(algo="ppo", value_clip=-1.0), "value_clip must be finite and >= 0"),
    (dict(algo="ppo", rollout=0), "rollout must be in 1..128"),
])
def test_vec_actor_critic_ppo_refusals_before_the_gpu(kw, msg):
    from dqnflappybird_amd.vecac import VecActorCritic
    with pytest.raises(ValueError, match=msg):
        VecActorCritic(16, **kw)


def test_a2c_and_ppo_checkpoints_refuse_each_other(tmp_path):
    from dqnflappybird_amd.vecac import VecActorCritic
    a2c, ppo = str(tmp_path / "a2c.npz"), str(tmp_path / "ppo.npz")
    base = dict(head=np.array(["ac"]), online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 0, 16, 4, 512], np.int64))
    np.savez(a2c, **base)
    np.savez(ppo, ppo=np.array([4, 4, 0.2, 0.0, 1.0]), **base)
    va = VecActorCritic.__new__(VecActorCritic)                  # (load refuses before it touches anything of the object but algo)
    va.algo = "a2c"
    with pytest.raises(ValueError, match="holds a PPO run, this VecActorCritic runs algo='a2c'"):
        va.load(ppo)
    vp = VecActorCritic.__new__(VecActorCritic)
    vp.algo = "ppo"
    with pytest.raises(ValueError, match="holds an A2C run, this VecActorCritic runs algo='ppo'"):
        vp.load(a2c)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "ppo"], "--model ppo needs --vec"),
    (["--model", "ppo", "--vec", "16", "--rollout", "0"], "rollout must be in 1..128"),
    (["--model", "ppo", "--vec", "16", "--epochs", "0"], "epochs must be >= 1"),
    (["--model", "ppo", "--vec", "16", "--minibatches", "3"], "minibatches must be >= 1 and divide rollout x n_envs = 80"),
    (["--model", "ppo", "--vec", "16", "--clip-eps", "0"], "clip_eps must be finite and > 0"),
    (["--model", "ppo", "--vec", "16", "--value-clip", "-1"], "value_clip must be finite and >= 0"),
    (["--model", "ppo", "--vec", "16", "--entropy-coef", "nan"], "entropy_coef must be finite and >= 0"),
    (["--model", "ppo", "--vec", "16", "--noisy"], "--noisy is not an option of --model ppo"),
    (["--model", "ppo", "--vec", "16", "--n-step", "3"], "--n-step is not an option of --model ppo"),
    (["--model", "a2c", "--vec", "16", "--epochs", "2"], "--epochs need --model ppo, not --model a2c"),
    (["--model", "ddqn", "--vec", "16", "--clip-eps", "0.1", "--no-adv-norm"], "--clip-eps / --no-adv-norm need --model ppo"),
])
def test_cli_ppo_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
