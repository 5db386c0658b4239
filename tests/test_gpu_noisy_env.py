"""Per-env acting noise of noisy C51 nets on the MI355X (include/fbdqn.h): fb_qnet_act_nib_env_noise against a
float64 restatement built from the documented per-env draws (Philox stream 7, counter (e nz + k, step_lo, 7, step_hi)) with the
effective weights mu + sigma (.) (f(eps_out_e) x f(eps_in_e)) of each env; its reduction to mean-mode acting at sigma = 0, bit for bit;
its keying by env; the call's lack of side effects; fb_vec_step in per-env mode against the composed calls, bit for bit; the shared mode
untouched; the refusals; and a short VecBrain run."""
import ctypes

import numpy as np
import pytest

from tests.test_gpu_c51 import FC, GAMMA, _batch
from tests.test_gpu_c51_noisy import PER, _pipeline, effective, frozen, make_noisy, ref_q, same
from tests.test_gpu_nstep_per import per_memory  # noqa: F401  (the pipeline's prioritized memory)

pytestmark = pytest.mark.gpu
HEADS = ("c51", "c51dueling")
STREAM_ENV_NOISE = 7
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def philox_np(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 over an array of first counter words (numpy uint64 arithmetic)"""
    c0 = np.asarray(c0, np.uint64) & M32
    c1, c2, c3 = (np.full(c0.shape, v & M32, np.uint64) for v in (c1, c2, c3))
    k0, k1 = np.uint64(k0 & M32), np.uint64(k1 & M32)
    m0, m1, mask = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(M32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return c0, c1, c2, c3


def env_noise(seed, step, e, nz):
    """the documented draw of env e: f(z) (float64, z from the float32 uniforms) for k = 0 .. nz - 1"""
    r = philox_np(seed, seed >> 32, e * nz + np.arange(nz, dtype=np.uint64), step, STREAM_ENV_NOISE, step >> 32)
    u1 = ((r[0] >> np.uint64(8)) + np.uint64(1)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    u2 = (r[1] >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    z = np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))
    return np.copysign(np.sqrt(np.abs(z)), z)


def restate(net, head, N, s, seed, step, envs):
    """float64 Q of the given envs (rows of the u8 states s) through their own effective weights"""
    P = net.store_params(0).cpu().numpy()
    nz = net.noise_size
    return np.stack([ref_q(head, effective(P, env_noise(seed, step, e, nz), head, N, net.A, net.FC), s[e:e + 1], N, net.A, net.FC)[0]
                     for e in envs])


def chosen(n):
    return sorted({0, n - 1, n // 2, n // 3, (2 * n) // 3, n // 7, n - 2 if n > 1 else 0, min(n - 1, 129)})[:8]


_STATES = {}


def states(n, seed=5, steps=9):
    """n envs played a few random steps: (nibble states, u8 states of the same envs), cached per n"""
    import torch
    if n not in _STATES:
        from dqnflappybird_amd.vec import VecGameState, VecReplay
        env = VecGameState(n, seed=seed)
        rep = VecReplay(max(4000, 4 * n), n)
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        g = torch.Generator(device="cpu").manual_seed(n)
        for _ in range(steps):
            acts = torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8).cuda()
            env.frame_step(acts, want_u8=False)
            rep.push(env.frame_bits, acts, env.reward, env.terminal)
        _STATES[n] = (env, rep, nib, rep.current_state().cpu().numpy())
    return _STATES[n][2], _STATES[n][3]


def check_against_restatement(net, head, N, nib, s, seed, step, what):
    n = nib.shape[0]
    a, q = net.act_nib_env_noise(nib, 0.0, seed=seed, step=step, want_q=True)
    a, q = a.cpu().numpy(), q.cpu().numpy()
    envs = chosen(n)
    q0 = restate(net, head, N, s, seed, step, envs)
    np.testing.assert_allclose(q[envs], q0, rtol=0, atol=5e-4, err_msg=what)
    margin = np.abs(q0[:, 1] - q0[:, 0]) > 1e-3
    assert np.array_equal(a[envs][margin], q0.argmax(1)[margin]), what
    return q


# ---------------------------------------------------------------------------------------------------------------- the forward
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("N", [51, 2])
@pytest.mark.parametrize("n", [1, 37, 256, 300])
def test_acting_matches_the_restatement(torch_cuda, head, N, n):
    nib, s = states(n)
    for scale in (1.0, 1e-3):
        net, _, _ = make_noisy(head, N, max_batch=max(n, 32), sigma_scale=scale)
        net.reset_noise(0, 4, 4)                           # (never read by the call)
        q = check_against_restatement(net, head, N, nib, s, 2 ** 33 + 11, 2 ** 32 + 6, f"{head} N={N} n={n} sigma x {scale}")
        if scale == 1.0 and n > 1:
            assert np.abs(q[:, 1] - q[:, 0]).std() > 0


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n", [37, 1024])
def test_zero_sigma_is_mean_mode_acting_bit_for_bit(torch_cuda, head, n):
    nib, _ = states(n)
    net, _, _ = make_noisy(head, 51, max_batch=n, sigma0=0.0)
    for eps in (0.0, 0.3):
        a, q = (x.clone() for x in net.act_nib_env_noise(nib, eps, seed=3, step=8, want_q=True))
        net.mean_noise(0)
        a0, q0 = net.act_nib(nib, eps, seed=3, step=8, want_q=True)
        assert torch_cuda.equal(q, q0) and torch_cuda.equal(a, a0), eps
        net.reset_noise(0, 1, 1)


@pytest.mark.parametrize("head", HEADS)
def test_keyed_by_env(torch_cuda, head):
    """the first 300 rows of 1024 envs act as 300 envs do (the fused path at both counts)"""
    nib, _ = states(1024)
    net, _, _ = make_noisy(head, 51, max_batch=1024)
    a, q = (x.clone() for x in net.act_nib_env_noise(nib, 0.0, seed=9, step=5, want_q=True))
    a3, q3 = net.act_nib_env_noise(nib[:300], 0.0, seed=9, step=5, want_q=True)
    assert torch_cuda.equal(q[:300], q3) and torch_cuda.equal(a[:300], a3)


@pytest.mark.parametrize("head", HEADS)
def test_distinct_per_env_and_repeatable(torch_cuda, head):
    torch = torch_cuda
    nib, _ = states(300)
    same_nib = nib[7:8].repeat(300, 1).contiguous()      # one state in every row
    net, _, _ = make_noisy(head, 51, max_batch=300)
    q = net.act_nib_env_noise(same_nib, 0.0, seed=1, step=2, want_q=True)[1].clone()
    d = (q[:, 1] - q[:, 0]).cpu().numpy()
    assert len(np.unique(d)) == 300                        # pairwise distinct
    assert torch.equal(net.act_nib_env_noise(same_nib, 0.0, seed=1, step=2, want_q=True)[1], q)
    q2 = net.act_nib_env_noise(same_nib, 0.0, seed=1, step=3, want_q=True)[1]
    assert not torch.equal(q2, q) and (q2 != q).all()
    net.mean_noise(0)
    qm = net.act_nib(same_nib, 0.0, want_q=True)[1]
    assert (qm == qm[0]).all()                             # (the mean net alone gives every row the same Q)


@pytest.mark.parametrize("n", [37, 300])
def test_the_call_has_no_side_effects(torch_cuda, n):
    torch = torch_cuda
    from tests.test_gpu_c51 import _batch as batch
    nib, _ = states(n)
    for head in HEADS:
        net, _, _ = make_noisy(head, 51, max_batch=max(n, 32))
        net.set_hparams(lr=1e-3)
        s_, a_, r_, s2_, t_ = (torch.from_numpy(x).cuda() for x in batch(np.random.default_rng(1), 32))
        net.reset_noise(0, 5, 6); net.reset_noise(1, 5, 6)
        net.train_step("c51double", s_, a_, r_, s2_, t_, gamma=GAMMA)      # (Adam state and sigma planes in use)
        before, ovf = frozen(net), net.overflow_count()
        a0, q0 = (x.clone() for x in net.act_nib(nib, 0.0, seed=2, step=3, want_q=True))
        net.act_nib_env_noise(nib, 0.0, seed=2, step=3)
        torch.cuda.synchronize()
        assert same(frozen(net), before) and net.overflow_count() == ovf, head
        a1, q1 = net.act_nib(nib, 0.0, seed=2, step=3, want_q=True)
        assert torch.equal(q0, q1) and torch.equal(a0, a1), head


def test_sigma_planes_follow_every_change(torch_cuda):
    """after load_params, a fused train step, apply_adam and init_params the per-env forward reads sigma as it now is"""
    torch = torch_cuda
    head, N, n = "c51dueling", 51, 300
    nib, s = states(n)
    net, p_on, _ = make_noisy(head, N, max_batch=n)
    net.set_hparams(lr=3e-3)
    rng = np.random.default_rng(3)
    q_prev = check_against_restatement(net, head, N, nib, s, 1, 2, "make")
    p2 = p_on.copy()
    p2[p2.size // 2:] *= 3.0                               # (the second half of [mu | sigma] is all sigma)
    net.load_params(p2, 0)
    q = check_against_restatement(net, head, N, nib, s, 1, 2, "load_params")
    assert np.abs(q - q_prev).max() > 1e-2
    for k in range(2):
        s_, a_, r_, s2_, t_ = (torch.from_numpy(x).cuda() for x in _batch(rng, 32))
        net.reset_noise(0, 7, k); net.reset_noise(1, 7, k)
        if k == 0:
            net.train_step("c51", s_, a_, r_, s2_, t_, gamma=GAMMA)
        else:
            g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            net.train_step("c51double", s_, a_, r_, s2_, t_, gamma=GAMMA, flat_grad=g)
            net.apply_adam(g)
        check_against_restatement(net, head, N, nib, s, 1, 2, f"train {k}")
    net.init_params(11, 0)
    check_against_restatement(net, head, N, nib, s, 1, 2, "init_params")


# ---------------------------------------------------------------------------------------------------------------- fb_vec_step
VEC_CASES = [(algo, head, n) for algo in ("c51", "c51doubleper") for head in HEADS for n in (1, 3)]


@pytest.mark.parametrize("algo,head,n", VEC_CASES)
def test_vec_step_equals_composed_calls(torch_cuda, algo, head, n):
    """fb_vec_step in per-env mode == act_nib_env_noise -> frame_step -> push (-> sample) -> reset_noise(0) -> reset_noise(1) ->
    train_from_replay (-> batch_update): actions, indices, losses, parameters, both nets' noise and the memory's state"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps, seed, N = 32, 10, 1, 256
    per = algo in PER
    e1, r1, n1, nib1 = _pipeline(N, n, algo, head)
    e2, r2, n2, nib2 = _pipeline(N, n, algo, head)
    n1.set_acting_noise("env"); n2.set_acting_noise("env")
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 5 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib_env_noise(nib1, 0.0, seed=seed, step=step).clone()
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
        n1.reset_noise(0, seed, step)
        if train:
            n1.reset_noise(1, seed, step)
            if per:
                loss, _, r_, t_, ae = train_from_replay(r1, n1, algo, idx, gamma=GAMMA, isw=isw, want_abs_err=True)
                r1.update_priorities(idx, abs_err=ae)
            else:
                loss, _, r_, t_ = train_from_replay(r1, n1, algo, idx, gamma=GAMMA)
        a2 = one(0.0, seed=seed, step=step, train=train)
        assert torch.equal(a1, a2), step
        assert torch.equal(n1.noise(0), n2.noise(0)) and torch.equal(n1.noise(1), n2.noise(1)), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(r_, one.r) and torch.equal(t_, one.t), step
            if per:
                assert torch.equal(isw, one.isw) and torch.equal(ae, one.abs_err + 0.01), step
    assert torch.equal(n1.store_params(0), n2.store_params(0)) and torch.equal(n1.store_params(1), n2.store_params(1))
    assert (e1.get_state() == e2.get_state()).all()
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    # the step leaves the online sample of (seed, last step) in place
    noise = n2.noise(0).clone()
    n2.reset_noise(0, seed, steps - 1)
    assert torch.equal(n2.noise(0), noise)


@pytest.mark.parametrize("algo", ["c51", "c51doubleper"])
def test_shared_mode_is_unaffected(torch_cuda, algo):
    """a net switched to per-env and back (with a per-env call in between) steps exactly as a net never switched"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep
    e1, r1, n1, nib1 = _pipeline(256, 3, algo, "c51dueling")
    e2, r2, n2, nib2 = _pipeline(256, 3, algo, "c51dueling")
    n2.set_acting_noise("env")
    n2.act_nib_env_noise(nib2, 0.0, seed=4, step=4)
    n2.set_acting_noise("shared")
    s1, s2 = VecStep(e1, r1, n1, 32, algo, GAMMA), VecStep(e2, r2, n2, 32, algo, GAMMA)
    for step in range(9):
        a1, a2 = s1(0.0, seed=2, step=step, train=step >= 4), s2(0.0, seed=2, step=step, train=step >= 4)
        assert torch.equal(a1, a2) and torch.equal(s1.loss, s2.loss), step
    assert torch.equal(n1.store_params(0), n2.store_params(0)) and torch.equal(n1.noise(0), n2.noise(0))


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecStep
    N, B = 256, 32
    env, rep, net, nib = _pipeline(N, 1, "c51", "c51dueling")
    step = VecStep(env, rep, net, B, "c51", GAMMA)
    for k in range(3):
        step(0.0, seed=1, step=k, train=False)
    acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    blob, env_state, before = rep.state_blob().copy(), env.get_state().copy(), frozen(net)
    plain = QNet(2, FC, "c51", max_batch=N)
    assert L.lib().fb_qnet_set_acting_noise(plain.h, L.ACT_NOISE_PER_ENV) == -1
    assert "not a noisy net" in L.lib().fb_last_error().decode()
    assert L.lib().fb_qnet_act_nib_env_noise(plain.h, L.ptr(nib), N, 0.0, 1, 1, L.ptr(acts), None, L.current_stream()) == -1
    assert "needs a noisy net" in L.lib().fb_last_error().decode()
    for mode in (2, -1):
        assert L.lib().fb_qnet_set_acting_noise(net.h, mode) == -1
        assert "mode must be" in L.lib().fb_last_error().decode()
    for n in (0, 3 * N + 1):
        assert L.lib().fb_qnet_act_nib_env_noise(net.h, L.ptr(nib), n, 0.0, 1, 1, L.ptr(acts), None, L.current_stream()) == -1
    net.set_inference_dtype("bf16")
    net.set_acting_noise("env")
    with pytest.raises(ValueError, match="FB_DTYPE_F32 inference only"):
        net.act_nib_env_noise(nib, 0.0, seed=1, step=1)
    with pytest.raises(ValueError, match="FB_DTYPE_F32 inference only"):
        step(0.0, seed=1, step=3, train=True)
    torch.cuda.synchronize()
    assert np.array_equal(rep.state_blob(), blob) and np.array_equal(env.get_state(), env_state)
    assert same(frozen(net), before)
    net.set_inference_dtype("f32")                         # (and the mode stays per-env: the step runs)
    step(0.0, seed=1, step=3, train=False)
    assert not np.array_equal(env.get_state(), env_state)


# ---------------------------------------------------------------------------------------------------------------- VecBrain
def test_vecbrain_rainbow_with_per_env_noise(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="c51doubleper", arch="c51dueling", batch=32, capacity=20000, observe=50, seed=3, replace_target_iter=40, n_step=3,
              noisy=True, acting_noise="env")
    a = VecBrain(256, **kw)
    assert a.acting_noise == "env" and a.net.acting_noise == "env" and a.epsilon == 0.0
    a.run(300, log_every=0)
    assert a.last_loss is not None and torch.isfinite(a.last_loss).all()
    nz = a.net.noise(0).clone()
    a.net.reset_noise(0, a.seed, a.timeStep - 1)
    assert torch.equal(a.net.noise(0), nz)                 # the step left the (seed + rank, timeStep - 1) sample
    res = a.evaluate(512, max_steps=2000)
    assert (res.length > 0).all() and torch.equal(a.net.noise(0), nz)
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(6):
        a.step()
        ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.loss.clone(), a.net.noise(0).clone()))
    b = VecBrain(256, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(6):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.loss, b.net.noise(0))
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0))
