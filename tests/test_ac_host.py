"""Advantage actor-critic (include/fbdqn.h: FB_ARCH_AC) without a GPU: the ABI declarations; the float64 / numpy restatements the
GPU tests compare the kernels with -- np_gae (the pinned order of fb_ac_gae) against hand cases, np_ac_loss's analytic gradients against
torch autograd, the rollout's index formula against a small deque model, the sampling rule -- and every refusal the Python layers make
before anything touches the GPU."""
import collections
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_oracle_qnet import split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 0xFFFFFFFF
STREAM_POLICY = 8
SAMPLE_SEED, SAMPLE_STEP = (11 << 32) | 20261, (1 << 32) + 7     # tests/test_gpu_ac.py's draw: see test_the_committed_sampling_seed


# ---------------------------------------------------------------------------------------------------------------- restatements
def np_gae(reward, terminal, value, gamma, lam):
    """fb_ac_gae in numpy, operation for operation (float64, the header's order) -> (adv f32[T, N], ret f32[T, N])"""
    reward, terminal, value = np.asarray(reward, np.float32), np.asarray(terminal), np.asarray(value, np.float32)
    T, N = reward.shape
    assert value.shape == (T + 1, N) and terminal.shape == (T, N)
    gl = np.float64(gamma) * np.float64(lam)
    adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    A = np.zeros(N, np.float64)
    for t in range(T - 1, -1, -1):
        r = np.where(reward[t] == np.float32(0.1), np.float64(0.1), reward[t].astype(np.float64))
        nd = terminal[t] == 0
        v = value[t].astype(np.float64)
        x = np.where(nd, np.float64(gamma) * value[t + 1].astype(np.float64), 0.0)
        delta = (r + x) - v
        A = delta + np.where(nd, gl * A, 0.0)
        adv[t] = A.astype(np.float32)
        ret[t] = (A + v).astype(np.float32)
    return adv, ret


def np_ac_loss(z, V, a, adv, ret, n_total, cv, ce):
    """the A2C loss of include/fbdqn.h in float64 from logits z [B, A] and values V [B] -> (loss[4], dLoss/dz [B, A], dLoss/dV [B])"""
    z, V, adv, ret = (np.asarray(x, np.float64) for x in (z, V, adv, ret))
    a = np.asarray(a, np.int64)
    B = len(a)
    m = z.max(1, keepdims=True)
    e = np.exp(z - m)
    s = e.sum(1, keepdims=True)
    p, lp = e / s, z - (m + np.log(s))
    H = -(p * lp).sum(1)
    lpi, lv = -adv * lp[np.arange(B), a], (V - ret) ** 2
    onehot = np.zeros_like(z)
    onehot[np.arange(B), a] = 1.0
    dz = (adv[:, None] * (p - onehot) + ce * p * (lp + H[:, None])) / n_total
    dV = 2.0 * cv * (V - ret) / n_total
    parts = np.array([lpi.sum(), lv.sum(), H.sum()]) / n_total
    return np.array([parts[0] + cv * parts[1] - ce * parts[2], *parts]), dz, dV


def ac_forward64(p, states, fc, A):
    """the actor-critic net in float64 torch: tests/test_oracle_qnet.py::torch_forward's layers, then the RAW heads of the dueling
    layout.  p: a float64 tensor (requires_grad for gradients), states u8 [B, 80, 80, 4] -> (logits [B, A], V [B])"""
    w = split(p, fc, A, True)
    x = torch.as_tensor(np.array(states), dtype=torch.float64).permute(0, 3, 1, 2)
    h = F.relu(F.conv2d(x, w["w1"].permute(3, 2, 0, 1), w["b1"], stride=4, padding=2))
    h = F.max_pool2d(h, 2, 2)
    h = F.relu(F.conv2d(h, w["w2"].permute(3, 2, 0, 1), w["b2"], stride=2, padding=1))
    h = F.relu(F.conv2d(h, w["w3"].permute(3, 2, 0, 1), w["b3"], stride=1, padding=1))
    h = h.permute(0, 2, 3, 1).reshape(h.shape[0], 1600)
    h = F.relu(h @ w["wf1"] + w["bf1"])
    return h @ w["wq"] + w["bq"], (h @ w["wv"] + w["bv"])[:, 0]


def torch_ac_terms(z, V, a, adv, ret):
    """(sum L_pi, sum L_v, sum H) as float64 torch scalars: the loss is (L_pi + c_v L_v - c_e H) / n_total, linear in the three"""
    lp = torch.log_softmax(z, 1)
    H = -(lp.exp() * lp).sum(1)
    a = torch.as_tensor(np.asarray(a, np.int64))
    lpi = -(torch.as_tensor(np.asarray(adv, np.float64)) * lp[torch.arange(len(a)), a])
    lv = (V - torch.as_tensor(np.asarray(ret, np.float64))) ** 2
    return lpi.sum(), lv.sum(), H.sum()


def nib_pack(states):
    """u8 states [n, 80, 80, 4] ({0, 255}) -> the env kernel's nibble states u8[n, FB_NIB_STRIDE] (include/fbdqn.h, fb_env_set_nib_buffer:
    byte (r + 2) * 44 + 4 + q holds pixels (r, 2q) in its low and (r, 2q + 1) in its high nibble, bit f = frame f)"""
    from dqnflappybird_amd import _lib as L
    s = (np.asarray(states) != 0).astype(np.uint8)
    n = s.shape[0]
    nibble = (s << np.arange(4, dtype=np.uint8)).sum(-1).astype(np.uint8)          # [n, 80, 80]
    b = nibble[:, :, 0::2] | (nibble[:, :, 1::2] << 4)                            # [n, 80, 40]
    full = np.zeros((n, L.NIB_ROWS, L.NIB_PITCH), np.uint8)
    full[:, 2:82, 4:] = b
    out = np.zeros((n, L.NIB_STRIDE), np.uint8)
    out[:, :L.NIB_ROWS * L.NIB_PITCH] = full.reshape(n, -1)
    return out


def nib_unpack(nib):
    """the inverse (tests/test_gpu_shims.py's unpack)"""
    from dqnflappybird_amd import _lib as L
    n = nib.shape[0]
    b = np.ascontiguousarray(nib[:, :L.NIB_ROWS * L.NIB_PITCH].reshape(n, L.NIB_ROWS, L.NIB_PITCH)[:, 2:82, 4:])
    px = np.stack([b & 0x0F, b >> 4], axis=-1).reshape(n, 6400)
    return (((px[..., None] >> np.arange(4)) & 1) * 255).astype(np.uint8).reshape(n, 80, 80, 4)


def policy_uniforms(oracle, n, seed, step):
    """u of rows 0 .. n-1 at (seed, step): (o.x >> 8) * 2^-24 as float32, o = philox(key = seed, counter = (row, step_lo, 8, step_hi))"""
    return np.array([np.float32(int(oracle.philox(seed & M32, seed >> 32, r, step & M32, STREAM_POLICY, step >> 32)[0]) >> 8) * np.float32(2.0 ** -24)
                     for r in range(n)], np.float32)


def np_sample(z, u, dtype=np.float32):
    """the sampling rule of include/fbdqn.h from logits z [n, A] and uniforms u [n], in `dtype` arithmetic (float32: the device's)
    -> (actions, logp of them, distance of u to the nearest inner cdf boundary)"""
    z = np.asarray(z, dtype)
    n, A = z.shape
    m = z.max(1)
    e = np.exp((z - m[:, None]).astype(dtype)).astype(dtype)
    s = np.zeros(n, dtype)
    for c in range(A):
        s = (s + e[:, c]).astype(dtype)
    p = (e / s[:, None]).astype(dtype)
    cum = np.zeros(n, dtype)
    act = np.full(n, A - 1, np.int64)
    found = np.zeros(n, bool)
    dist = np.full(n, np.inf)
    for c in range(A):
        cum = (cum + p[:, c]).astype(dtype)
        hit = ~found & (u.astype(dtype) < cum)
        act[hit] = c
        found |= hit
        if c < A - 1:
            dist = np.minimum(dist, np.abs(u.astype(np.float64) - cum.astype(np.float64)))
    lse = (m + np.log(s).astype(dtype)).astype(dtype)
    logp = (z[np.arange(n), act] - lse).astype(dtype)
    return act, logp, dist


def deque_rollout_model(cap, N, T, pushes):
    """a deque(maxlen = cap) that receives N transitions (t, e) per push: the positions of the newest T pushes' transitions"""
    d = collections.deque(maxlen=cap)
    for t in range(pushes):
        for e in range(N):
            d.append((t, e))
    want = [(t, e) for t in range(pushes - T, pushes) for e in range(N)]
    return [list(d).index(x) for x in want], len(d)


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_ac_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ARCH_AC 6",
                 "int fb_qnet_create_ac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out);",
                 "int fb_qnet_set_ac(fb_qnet_t h, float value_coef, float entropy_coef);",
                 "int fb_qnet_get_ac(fb_qnet_t h, float *value_coef_host, float *entropy_coef_host);",
                 "int fb_qnet_forward_ac(fb_qnet_t h, const uint8_t *states, int batch, float *logits, float *value, void *stream);",
                 "int fb_qnet_act_policy_nib(fb_qnet_t h, const uint8_t *nib_states, int n, uint64_t seed, uint64_t step, int greedy, uint8_t *actions,",
                 "int fb_ac_gae(const float *reward, const uint8_t *terminal, const float *value, int T, int N, double gamma, double lambda, float *adv,",
                 "int fb_qnet_ac_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret, int64_t n_total,",
                 "int fb_ac_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *adv, const float *ret,",
                 "int fb_ac_rollout_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_ac_rollout_buffers *b, int n_envs, uint64_t seed,",
                 "FB_STREAM_POLICY = 8", "r = (rew == 0.1f) ? 0.1 : (double)rew", "the smallest c with u < sum_{c' <= c} p_c'"):
        assert decl in hdr, decl
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "#define FB_STREAM_POLICY 8u" in common
    assert L.ARCH_AC == 6 and L.AC_DEFAULTS == (0.5, 0.01)
    i, i64, u64, f, d, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_create_ac"] == [i, i, i, vp]
    assert L.SIGNATURES["fb_qnet_set_ac"] == [vp, f, f] and L.SIGNATURES["fb_qnet_get_ac"] == [vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_forward_ac"] == [vp, vp, i, vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_act_policy_nib"] == [vp, vp, i, u64, u64, i, vp, vp, vp, vp, vp]
    assert L.SIGNATURES["fb_ac_gae"] == [vp, vp, vp, i, i, d, d, vp, vp, vp]
    assert L.SIGNATURES["fb_qnet_ac_train_step"] == [vp, i, vp, vp, vp, vp, i64, vp, vp, vp]
    assert L.SIGNATURES["fb_ac_train_from_replay"] == [vp, vp, i, vp, vp, vp, i64, vp, vp, vp, vp]
    assert L.SIGNATURES["fb_ac_rollout_step"] == [vp, vp, vp, vp, i, u64, u64, i, vp]
    assert [n for n, _ in L.AcRolloutBuffers._fields_] == ["nib", "actions", "frame_bits", "reward", "terminal", "score", "value", "logp", "slots"]
    lib = L.lib()                                                # (binds every symbol: a stale library raises here)
    assert lib.fb_qnet_set_ac(None, 0.5, 0.01) == -1 and "NULL" in lib.fb_last_error().decode()
    assert lib.fb_ac_gae(None, None, None, 1, 1, 0.99, 0.95, None, None, None) == -1 and "fb_ac_gae" in lib.fb_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- GAE
def test_gae_lambda_one_is_the_discounted_return():
    rng = np.random.default_rng(0)
    T, N, g = 6, 3, 0.9
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    adv, ret = np_gae(r, np.zeros((T, N), np.uint8), v, g, 1.0)
    for t in range(T):
        want = sum(g ** k * r[t + k].astype(np.float64) for k in range(T - t)) + g ** (T - t) * v[T].astype(np.float64)
        np.testing.assert_allclose(ret[t], want, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(adv[t], want - v[t], rtol=1e-6, atol=1e-6)


def test_gae_lambda_zero_is_one_step_td():
    rng = np.random.default_rng(1)
    T, N, g = 5, 4, 0.99
    r = rng.choice(np.array([0.1, 3, -3], np.float32), (T, N))
    term = (r == -3).astype(np.uint8)
    v = rng.normal(size=(T + 1, N)).astype(np.float32)
    adv, ret = np_gae(r, term, v, g, 0.0)
    r64 = np.where(r == np.float32(0.1), 0.1, r.astype(np.float64))              # 0.1f reads as 0.1
    want = r64 + np.where(term == 0, g * v[1:].astype(np.float64), 0.0) - v[:-1]
    assert np.array_equal(adv, want.astype(np.float32))
    assert np.array_equal(ret, (want + v[:-1]).astype(np.float32))
    assert term.any() and (r == np.float32(0.1)).any()


def test_gae_a_terminal_cuts_both_recursions():
    T, g, lam = 4, 0.5, 0.5
    r = np.array([[1.0], [2.0], [4.0], [8.0]], np.float32)
    v = np.array([[10.0], [20.0], [30.0], [40.0], [50.0]], np.float32)
    term = np.array([[0], [1], [0], [0]], np.uint8)
    adv, _ = np_gae(r, term, v, g, lam)
    d3 = 8 + g * 50 - 40
    d2 = 4 + g * 40 - 30
    d1 = 2 - 20                                                   # terminal: no bootstrap ...
    d0 = 1 + g * 20 - 10
    A3 = d3; A2 = d2 + g * lam * A3; A1 = d1; A0 = d0 + g * lam * A1      # ... and no advantage carried across it
    assert adv[:, 0].tolist() == [A0, A1, A2, A3]
    free, _ = np_gae(r, np.zeros_like(term), v, g, lam)
    assert free[1, 0] != adv[1, 0] and free[0, 0] != adv[0, 0] and free[2, 0] == adv[2, 0]


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("A", [1, 2, 3, 8])
@pytest.mark.parametrize("cv,ce", [(0.5, 0.01), (0.0, 0.0), (1.0, 0.5)])
def test_np_ac_loss_gradients_equal_autograd(A, cv, ce):
    rng = np.random.default_rng(A)
    B, nt = 9, 36
    z = torch.tensor(rng.normal(size=(B, A)) * 2, dtype=torch.float64, requires_grad=True)
    V = torch.tensor(rng.normal(size=B), dtype=torch.float64, requires_grad=True)
    a, adv, ret = rng.integers(0, A, B), rng.normal(size=B), rng.normal(size=B)
    lpi, lv, H = torch_ac_terms(z, V, a, adv, ret)
    loss = (lpi + cv * lv - ce * H) / nt
    loss.backward()
    got, dz, dV = np_ac_loss(z.detach().numpy(), V.detach().numpy(), a, adv, ret, nt, cv, ce)
    np.testing.assert_allclose(got, [loss.item(), lpi.item() / nt, lv.item() / nt, H.item() / nt], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dz, z.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dV, V.grad.numpy(), rtol=1e-12, atol=1e-14)
    if A == 1:
        assert not dz.any() and got[3] == 0.0                    # one action: p = 1, H = 0, no policy gradient


def test_ac_forward64_reads_the_dueling_layout_raw():
    """the raw heads against torch_forward's dueling combine: Q = V + (z - mean z) from the same parameters"""
    from tests.test_oracle_qnet import torch_forward
    rng = np.random.default_rng(5)
    fc, A = 128, 3
    n = 77984 + 1600 * fc + fc + fc + 1 + fc * A + A
    p = torch.tensor(rng.normal(size=n) * 0.03, dtype=torch.float64)
    s = (rng.random((4, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    z, V = ac_forward64(p, s, fc, A)
    q = torch_forward(p, torch.tensor(s, dtype=torch.float64), fc, A, True)
    np.testing.assert_allclose((V[:, None] + (z - z.mean(1, keepdim=True))).numpy(), q.numpy(), rtol=1e-12, atol=1e-12)
    assert z.abs().max() > 0


# ---------------------------------------------------------------------------------------------------------------- rollout indices
@pytest.mark.parametrize("cap,N,T,pushes", [(40, 4, 3, 3), (40, 4, 3, 7), (40, 4, 3, 10), (40, 4, 3, 23), (35, 5, 5, 7), (37, 5, 5, 9), (7, 1, 5, 30)])
def test_rollout_indices_against_a_deque(cap, N, T, pushes):
    """not yet full, just full, wrapped, and a capacity that is no multiple of the env count"""
    from dqnflappybird_amd.vecac import rollout_indices
    want, size = deque_rollout_model(cap, N, T, pushes)
    assert size == min(pushes * N, cap)
    idx = rollout_indices(size, T, N)
    assert idx.dtype == np.int64 and idx.tolist() == want
    total = pushes * N                                           # csrc/fb_gather.h: position j -> g = total - size + j, (t, e) = divmod(g, N)
    assert [divmod(total - size + int(j), N) for j in idx] == [(t, e) for t in range(pushes - T, pushes) for e in range(N)]
    with pytest.raises(ValueError, match="fewer than the rollout"):
        rollout_indices(T * N - 1, T, N)


# ---------------------------------------------------------------------------------------------------------------- sampling, nibble states
def test_nib_pack_is_the_documented_layout():
    from dqnflappybird_amd import _lib as L
    rng = np.random.default_rng(2)
    s = (rng.random((3, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    nib = nib_pack(s)
    assert nib.shape == (3, L.NIB_STRIDE) and np.array_equal(nib_unpack(nib), s)
    one = np.zeros((1, 80, 80, 4), np.uint8)
    one[0, 7, 11, 2] = 255                                        # pixel (7, 11): odd column -> high nibble of byte (7 + 2) * 44 + 4 + 5, frame 2
    assert np.flatnonzero(nib_pack(one)[0]).tolist() == [9 * 44 + 4 + 5] and nib_pack(one)[0, 9 * 44 + 9] == 1 << (4 + 2)


def test_np_sample_rule():
    z = np.log(np.array([[0.25, 0.25, 0.5]] * 5, np.float32))
    u = np.array([0.0, 0.2499, 0.25, 0.7, 0.99999994], np.float32)
    act, logp, dist = np_sample(z, u)
    assert act.tolist() == [0, 0, 1, 2, 2]                        # u < cum, strictly: u = 0.25 goes to the second action
    np.testing.assert_allclose(logp, np.log([0.25, 0.25, 0.25, 0.5, 0.5]), atol=1e-6)
    assert dist[2] == 0.0 and abs(dist[1] - 1e-4) < 1e-6
    a1, l1, d1 = np_sample(np.array([[3.5]], np.float32), np.array([0.9], np.float32))
    assert a1.tolist() == [0] and l1.tolist() == [0.0] and np.isinf(d1[0])


def sampling_case(oracle, fc, A, n=2048):
    """tests/test_gpu_ac.py's sampling case: the net's parameters, n random states, their float64 logits"""
    from tests.test_gpu_qnet import rand_states, trained_like_params
    cfg = oracle.qcfg(fc, A, True)
    p = trained_like_params(oracle, cfg, 1)
    p[77984 + 1600 * fc + fc:] *= np.float32(np.sqrt(512 / fc))
    s = rand_states(np.random.default_rng(1000 + fc + A), n)
    with torch.no_grad():
        z = torch.cat([ac_forward64(torch.from_numpy(p.astype(np.float64)), s[k:k + 256], fc, A)[0] for k in range(0, n, 256)]).numpy()
    return p, s, z


@pytest.mark.parametrize("fc,A", [(512, 2), (384, 3), (128, 8)])
def test_the_committed_sampling_seed(oracle, fc, A):
    """the GPU sampling test may skip rows whose u lies within 1e-5 of a cdf boundary; its seed is chosen so that the float64 reference
    has none; the draw is no greedy play in disguise: several actions occur, and some rows take another action than the argmax"""
    _, _, z = sampling_case(oracle, fc, A)
    u = policy_uniforms(oracle, len(z), SAMPLE_SEED, SAMPLE_STEP)
    act, _, dist = np_sample(z, u, np.float64)
    assert dist.min() >= 1e-5, (dist.min(), int(dist.argmin()))
    assert len(set(act.tolist())) >= min(A, 3) and (act != z.argmax(1)).mean() > 0.05


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_value_checks():
    from dqnflappybird_amd import vec
    assert vec.check_ac(0.5, 0.01) == (0.5, float(np.float32(0.01))) and vec.check_ac(0, 0) == (0.0, 0.0)
    for args, msg in (((-0.1, 0.01), "value_coef"), ((float("nan"), 0.01), "value_coef"), ((float("inf"), 0.0), "value_coef"),
                      ((0.5, -1e-3), "entropy_coef"), ((0.5, float("nan")), "entropy_coef"), ((0.5, 1e39), "entropy_coef")):
        with pytest.raises(ValueError, match=msg):
            vec.check_ac(*args)
    assert vec.check_gae(0.99, 0.95) == (0.99, 0.95) and vec.check_gae(1, 0) == (1.0, 0.0)
    for args, msg in (((1.5, 0.9), "gamma"), ((-0.1, 0.9), "gamma"), ((float("nan"), 0.9), "gamma"), ((0.99, 1.01), "gae_lambda"),
                      ((0.99, -1), "gae_lambda"), ((0.99, float("nan")), "gae_lambda")):
        with pytest.raises(ValueError, match=msg):
            vec.check_gae(*args)
    assert vec.check_rollout(1) == 1 and vec.check_rollout(128) == 128
    for t in (0, 129, -3):
        with pytest.raises(ValueError, match="rollout must be in 1..128"):
            vec.check_rollout(t)
    assert "ac" in vec.QNet.ARCHS and vec.AC_DEFAULTS == (0.5, 0.01)


@pytest.mark.parametrize("kw,msg", [
    (dict(rollout=0), "rollout must be in 1..128"),
    (dict(rollout=129), "rollout must be in 1..128"),
    (dict(gamma=1.5), "gamma must be in \\[0, 1\\]"),
    (dict(gae_lambda=-0.5), "gae_lambda must be in \\[0, 1\\]"),
    (dict(value_coef=-1), "value_coef must be finite and >= 0"),
    (dict(entropy_coef=float("nan")), "entropy_coef must be finite and >= 0"),
    (dict(max_grad_norm=-1), "max_grad_norm must be finite and >= 0"),
    (dict(capacity=16 * 6), "capacity 96 < \\(rollout \\+ 2\\) x n_envs = 112"),
    (dict(lr=0.0), "lr must be finite and > 0"),
])
def test_vec_actor_critic_refusals_before_the_gpu(kw, msg):
    from dqnflappybird_amd.vecac import VecActorCritic
    with pytest.raises(ValueError, match=msg):
        VecActorCritic(16, **kw)
    with pytest.raises(ValueError, match="n_envs must be >= 1"):
        VecActorCritic(0)


def test_checkpoints_of_the_two_loops_refuse_each_other(tmp_path):
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain, checkpoint_head
    ac, dqn = str(tmp_path / "ac.npz"), str(tmp_path / "dqn.npz")
    np.savez(ac, head=np.array(["ac"]), online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 0], np.int64))
    np.savez(dqn, online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 0], np.int64))
    assert checkpoint_head(np.load(ac)) == "ac" and checkpoint_head(np.load(dqn)) == "scalar"
    vb = VecBrain.__new__(VecBrain)                              # (load refuses before it touches anything of the object but world)
    vb.world = 1
    with pytest.raises(ValueError, match="holds an ac head \\(a VecActorCritic's\\), this is a VecBrain"):
        vb.load(ac)
    va = VecActorCritic.__new__(VecActorCritic)
    with pytest.raises(ValueError, match="holds a scalar head \\(a VecBrain's\\), this is a VecActorCritic"):
        va.load(dqn)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "a2c"], "--model a2c needs --vec"),
    (["--model", "a2c", "--vec", "16", "--rollout", "0"], "rollout must be in 1..128"),
    (["--model", "a2c", "--vec", "16", "--gae-lambda", "2"], "gae_lambda must be in [0, 1]"),
    (["--model", "a2c", "--vec", "16", "--value-coef", "-1"], "value_coef must be finite and >= 0"),
    (["--model", "a2c", "--vec", "16", "--entropy-coef", "nan"], "entropy_coef must be finite and >= 0"),
    (["--model", "a2c", "--vec", "16", "--max-grad-norm", "-2"], "max_grad_norm must be finite and >= 0"),
    (["--model", "a2c", "--vec", "16", "--noisy"], "--noisy is not an option of --model a2c"),
    (["--model", "a2c", "--vec", "16", "--n-step", "3"], "--n-step is not an option of --model a2c"),
    (["--model", "a2c", "--vec", "16", "--huber", "1"], "--huber"),
    (["--model", "ddqn", "--vec", "16", "--rollout", "5"], "--rollout need --model a2c"),
])
def test_cli_a2c_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
