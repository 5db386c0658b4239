"""Noisy IQN on the GPU (include/fbdqn.h: fb_qnet_create_iqn_noisy; kernels: csrc/fb_iqn.hip) against the float64 restatements of
tests/test_iqn_noisy_host.py on effective weights: the layout and the draws; mean mode == the non-noisy net, bit for bit; the shared
sample through every forward-only path, never stale; every gradient of [mu | sigma] on kink-free minibatches; per-env acting against the
documented per-env draws; the fused steps == the composed calls, bit for bit; the refusals; the loop and its checkpoint.
Shapes: FC 128 (FC 384 once), A in {2, 3} (8 once), both heads, (N, N', K) in {(4, 5, 6), (1, 1, 1)}."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import nib_pack
from tests.test_gpu_ac import net_state, same_state
from tests.test_gpu_c51_noisy import np_noise
from tests.test_gpu_iqn import GAMMA, TAU_MARGIN, check_iqn_grads, eval_q, iqn_params, loop_state, same_loop, t64
from tests.test_gpu_iqn_dueling import check_grads as check_grads_dueling
from tests.test_gpu_iqn_dueling import iqnd_params
from tests.test_gpu_iqn_per import tree_state
from tests.test_gpu_noisy_env import chosen, env_noise, states
from tests.test_gpu_qnet import Q_ATOL, rand_states
from tests.test_iqn_host import F32, pre64, qbar_from_h, theta_from_h, torch_iqn_loss, trunk64
from tests.test_iqn_noisy_host import TRUNK, as_plain, effective, factors, layers, mu_bounds, n_mu, n_total, noisy_end
from tests.test_miqn_host import miqn_target64, miqn_tol

pytestmark = pytest.mark.gpu
HEADS = (False, True)                        # dueling
ARCH = {False: "iqnnoisy", True: "iqnduelingnoisy"}
PLAIN = {False: "iqn", True: "iqndueling"}
TAUS = (4, 5, 6)
ENV_ATOL = Q_ATOL                            # the per-env Q (profiles/iqn_noisy_time.txt holds the measured maxima)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def mu_params(oracle, fc, A, du, seed):
    return (iqnd_params if du else iqn_params)(oracle, fc, A, seed)


def make_noisy(oracle, fc=128, A=2, du=False, taus=TAUS, max_batch=32, sigma0=0.5, sigma_scale=1.0, lr=1e-4):
    """a noisy net holding the trained-like mu of the IQN tests (online: seed 1, target: seed 2) and sigma as initialised (x sigma_scale)
    -> (net, master online, master target)"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, ARCH[du], max_batch=max_batch, n_tau=taus[0], n_tau_next=taus[1], n_tau_act=taus[2], sigma0=sigma0)
    n = n_mu(fc, A, du)
    assert net.noisy and net.n_params == n_total(fc, A, du)
    ps = []
    for which in (0, 1):
        net.init_params(3 + which, which)
        p = net.store_params(which).cpu().numpy()
        p[:n] = mu_params(oracle, fc, A, du, 1 + which)
        p[n:] *= F32(sigma_scale)
        net.load_params(p, which)
        ps.append(p)
    net.set_hparams(lr=lr)
    return net, ps[0], ps[1]


def plain_twin(oracle, net, fc, A, du, taus=TAUS, max_batch=32, lr=1e-4):
    """the non-noisy net of the same head holding the noisy net's mu"""
    from dqnflappybird_amd.vec import QNet
    tw = QNet(A, fc, PLAIN[du], max_batch=max_batch, n_tau=taus[0], n_tau_next=taus[1], n_tau_act=taus[2])
    n = n_mu(fc, A, du)
    for which in (0, 1):
        tw.load_params(net.store_params(which)[:n].clone(), which)
    tw.set_hparams(lr=lr)
    return tw


def eff64(P, nz, fc, A, du):
    """the float64 IQN-layout view of the effective parameters of the master vector P under the noise vector nz"""
    return as_plain(effective(P, nz, fc, A, du), fc, A, du)


def qbar64(P, nz, s, K, eta, fc, A, du):
    import torch
    with torch.no_grad():
        q = eff64(P, nz, fc, A, du)
        return qbar_from_h(q, trunk64(q, s, fc, A), K, eta, fc, A).numpy()


def frozen(net):
    return net_state(net) + (net.noise(0).clone(), net.noise(1).clone())


def same_frozen(torch, x, y):
    return same_state(torch, x[:5], y[:5]) and torch.equal(x[5], y[5]) and torch.equal(x[6], y[6])


def a_batch(torch, rng, B, A):
    d = lambda x: torch.from_numpy(x).cuda()
    return (d(rand_states(rng, B)), d(rng.integers(0, A, B).astype(np.uint8)), d(rng.choice(np.array([0.1, 3, -3], F32), B)), d(rand_states(rng, B)),
            d((rng.random(B) < 0.3).astype(np.uint8)))


# ================================================================================================================ 1: layout / init
@pytest.mark.parametrize("fc,A,du", [(128, 2, False), (128, 3, True), (384, 3, False), (128, 8, True)])
def test_layout_init_and_the_draws(torch_cuda, fc, A, du):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet
    plain = QNet(A, fc, PLAIN[du], max_batch=8)
    ls, nz = layers(fc, A, du)
    n = n_mu(fc, A, du)
    for s0 in (0.5, 0.0, 1.7):
        net = QNet(A, fc, ARCH[du], max_batch=8, sigma0=s0)
        assert net.noisy and net.arch == ARCH[du] and L.lib().fb_qnet_is_noisy(net.h) == 1 and net.sigma0 == float(F32(s0))
        assert net.n_params == n_total(fc, A, du) == plain.n_params + noisy_end(fc, A, du) - TRUNK and plain.n_params == n
        net.init_params(21, 0); plain.init_params(21, 0)
        p = net.store_params(0).cpu().numpy()
        assert np.array_equal(p[:n], plain.store_params(0).cpu().numpy())           # mu: the non-noisy net's bits (b_e = 1 included)
        b = mu_bounds(fc, A, du)
        assert (p[b["b_e"][0]:b["b_e"][1]] == 1).all()
        want = np.concatenate([np.full((fi + 1) * fo, F32(np.float64(F32(s0)) / np.sqrt(fi)), F32) for _, fi, fo, _, _ in ls])
        assert np.array_equal(p[n:], want), s0
    assert net.noise_size == nz
    same = QNet(A, fc, ARCH[du], max_batch=8, noisy=True, sigma0=1.7)          # (the arch says it: the keyword is redundant, not refused)
    assert same.noisy and same.n_params == net.n_params and same.sigma0 == net.sigma0
    for which in (0, 1):                                             # a new net is in mean mode
        assert torch.equal(net.noise(which), torch.zeros(nz, device="cuda"))
    seed, step = (7 << 32) + 123, (3 << 32) + 77
    for which in (0, 1):
        net.reset_noise(which, seed, step)
        f = net.noise(which).cpu().numpy()
        z64, f32 = np_noise(seed, step, which, nz)
        zd = np.sign(f).astype(np.float64) * np.square(f.astype(np.float64))
        np.testing.assert_allclose(zd, z64, rtol=1e-5, atol=1e-5, err_msg=f"which={which}")
        np.testing.assert_allclose(f, f32, rtol=1e-5, atol=2e-3)
        assert np.abs(f - f32).mean() < 5e-6
    assert (net.noise(0) != net.noise(1)).float().mean().item() > 0.99
    net.mean_noise(0)
    assert torch.equal(net.noise(0), torch.zeros(nz, device="cuda")) and bool((net.noise(1) != 0).any())


# ================================================================================================================ 2: mean mode
def q_paths(torch, net, sd, nib, n, which=0):
    out = {"forward": net.forward(sd[:n].contiguous(), which).clone()}
    if which == 0:
        out["act"] = net.act(sd[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)[1].clone()
        out["act_nib"] = net.act_nib(nib[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)[1].clone()
        out["eval_q"] = eval_q(torch, net, nib[:n].contiguous()).clone()
    return out


@pytest.mark.parametrize("du", HEADS)
def test_mean_mode_is_the_non_noisy_net_bit_for_bit(torch_cuda, oracle, du):
    torch = torch_cuda
    fc, A = 128, 3
    net, p_on, _ = make_noisy(oracle, fc, A, du, max_batch=128)
    twin = plain_twin(oracle, net, fc, A, du, max_batch=128)
    n = n_mu(fc, A, du)
    s = rand_states(np.random.default_rng(2), 300)
    sd, nib = torch.from_numpy(s).cuda(), torch.from_numpy(nib_pack(s)).cuda()
    for which in (0, 1):
        for cnt in (5, 300):                                         # the small-batch and the large-batch forward
            x, y = q_paths(torch, net, sd, nib, cnt, which), q_paths(torch, twin, sd, nib, cnt, which)
            assert all(torch.equal(x[k], y[k]) for k in x), (which, cnt)
    tau = torch.from_numpy(np.maximum(np.random.default_rng(3).random((300, 4)).astype(F32), F32(1e-6))).cuda()
    assert torch.equal(net.forward_iqn(sd, tau), twin.forward_iqn(sd, tau))
    # a gradient-exporting step: mu's part equal bits, sigma's part all zeros
    rng = np.random.default_rng(5)
    for B, dq in ((32, False), (128, True)):
        batch = a_batch(torch, rng, B, A)
        g, g0 = torch.full((net.n_params,), 7.0, device="cuda"), torch.zeros(twin.n_params, device="cuda")
        l, y = net.iqn_train_step(*batch, gamma=GAMMA, double_q=dq, seed=3, step=B, flat_grad=g)
        l0, y0 = twin.iqn_train_step(*batch, gamma=GAMMA, double_q=dq, seed=3, step=B, flat_grad=g0)
        assert torch.equal(l, l0) and torch.equal(y, y0) and torch.equal(g[:n], g0) and g0.abs().max() > 0 and not g[n:].any(), B
    assert np.array_equal(net.store_params(0).cpu().numpy(), p_on)


@pytest.mark.parametrize("du", HEADS)
def test_twenty_steps_in_mean_mode_train_mu_as_the_non_noisy_net(torch_cuda, oracle, du):
    """20 steps with Adam in mean mode: mu equal bits, sigma unchanged.  fb_iqn_step itself draws a sample on a noisy net and so leaves mean
    mode: the steps are composed of the calls it makes -- act_nib, the env step, push + sample, fb_iqn_train_from_replay -- none of which
    draws (test_iqn_step_equals_the_composed_calls holds the fused step to that composition, with the draws, bit for bit)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecGameState, VecReplay, iqn_train_from_replay
    fc, A, N, B = 128, 2, 16, 8
    net, p_on, _ = make_noisy(oracle, fc, A, du, lr=1e-3)
    twin = plain_twin(oracle, net, fc, A, du, lr=1e-3)
    n = n_mu(fc, A, du)
    env, rep = VecGameState(N, seed=5), VecReplay(2000, N)
    rep.seed(7, "cpython")
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    for k in range(20):
        a1, q1 = net.act_nib(nib, 0.3, seed=9, step=k, want_q=True)
        a2, q2 = twin.act_nib(nib, 0.3, seed=9, step=k, want_q=True)
        assert torch.equal(a1, a2) and torch.equal(q1, q2), k
        _, rew, term, _ = env.frame_step(a1, want_u8=False)
        idx = rep.push_sample(env.frame_bits, a1, rew, term, B)
        l1 = iqn_train_from_replay(rep, net, idx, gamma=GAMMA, double_q=bool(k & 1), seed=9, step=k)[0].clone()
        l2 = iqn_train_from_replay(rep, twin, idx, gamma=GAMMA, double_q=bool(k & 1), seed=9, step=k)[0]
        assert torch.equal(l1, l2), k
        if k % 7 == 6:
            net.sync_target(); twin.sync_target()
    m, v, pw = net.adam_state()
    m0, v0, pw0 = twin.adam_state()
    got = net.store_params(0)
    assert torch.equal(got[:n], twin.store_params(0)) and not torch.equal(got[:n], torch.from_numpy(p_on[:n]).cuda())
    assert torch.equal(got[n:], torch.from_numpy(p_on[n:]).cuda())                  # sigma's gradient is 0: Adam leaves it alone
    assert torch.equal(m[:n], m0) and torch.equal(v[:n], v0) and not m[n:].any() and not v[n:].any() and np.array_equal(pw, pw0)
    assert torch.equal(net.store_params(1)[:n], twin.store_params(1))


# ================================================================================================================ 3: the shared sample
@pytest.mark.parametrize("fc,A,du,taus", [(128, 3, False, TAUS), (128, 2, True, TAUS), (128, 2, False, (1, 1, 1)), (128, 8, True, (4, 5, 32)),
                                            (384, 3, True, TAUS)])
def test_the_shared_sample_through_every_forward_only_path_and_never_stale(torch_cuda, oracle, fc, A, du, taus):
    torch = torch_cuda
    K = taus[2]
    net, p_on, p_tg = make_noisy(oracle, fc, A, du, taus=taus, max_batch=128, lr=1e-3)
    s = rand_states(np.random.default_rng(K + A), 300)
    sd, nib = torch.from_numpy(s).cuda(), torch.from_numpy(nib_pack(s)).cuda()
    tau = np.maximum(np.random.default_rng(A).random((40, 5)).astype(F32), F32(1e-6))
    eta = [1.0]

    def check(what, moved=True):
        worst = 0.0
        for which in (0, 1):
            P, e = net.store_params(which).cpu().numpy(), net.noise(which).cpu().numpy()
            want = qbar64(P, e, s, K, eta[0], fc, A, du)
            mean = qbar64(P, np.zeros_like(e), s[:40], K, eta[0], fc, A, du)
            if moved:
                assert np.abs(want[:40] - mean).max() > 30 * Q_ATOL, (what, which)      # the sample moves Qbar far past the bound
            for cnt in (5, 300):
                for q in q_paths(torch, net, sd, nib, cnt, which).values():
                    worst = max(worst, np.abs(q.cpu().numpy() - want[:cnt]).max())
            with torch.no_grad():
                q = eff64(P, e, fc, A, du)
                th0 = theta_from_h(q, trunk64(q, s[:40], fc, A), tau, fc, A).numpy()
            th = net.forward_iqn(sd[:40].contiguous(), torch.from_numpy(tau).cuda(), which).cpu().numpy()
            worst = max(worst, np.abs(th - th0).max())
        print(f"noisy iqn fc={fc} A={A} dueling={du} K={K} eta={eta[0]} after {what}: max |dQ|, |dtheta| {worst:.3e}")
        assert worst <= Q_ATOL, what

    check("load_params (mean mode)", moved=False)
    net.reset_noise(0, 11, 4); net.reset_noise(1, 11, 4)
    check("reset_noise")
    rng = np.random.default_rng(5)
    before = net.store_params(0).clone()
    net.iqn_train_step(*a_batch(torch, rng, 16, A), gamma=GAMMA, seed=3, step=0)
    n = n_mu(fc, A, du)
    after = net.store_params(0)
    assert not torch.equal(after[:n], before[:n]) and not torch.equal(after[n:], before[n:])          # mu and sigma both trained
    check("a fused train step")
    g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    net.iqn_train_step(*a_batch(torch, rng, 16, A), gamma=GAMMA, seed=3, step=1, flat_grad=g)
    net.apply_adam(g)
    check("export + apply_adam")
    net.set_iqn_risk(0.25)
    eta[0] = 0.25
    check("set_iqn_risk")
    net.soft_sync_target(0.3)
    check("soft_sync_target")
    net.sync_target()
    assert torch.equal(net.store_params(0), net.store_params(1))
    check("sync_target")
    net.init_params(seed=9, which=0)                                 # (the online net keeps its live sample: mu + sigma0 / sqrt(fan_in) (.) e)
    check("init_params")
    net.load_params(p_tg, 0)
    check("load_params")
    assert net.overflow_count() == 0


# ================================================================================================================ 4: gradients
_grads = {}


def ref_step(oracle, net, P_on, P_tg, fc, A, du, taus, B):
    """kink-free inputs under the EFFECTIVE online weights (the net's current sample), and the float64 loss, targets and gradient of
    [mu | sigma] for double_q = 0 and 1: tests/test_gpu_iqn.py::ref_step with the effective weights composed in torch"""
    import torch
    N, Np, K = taus
    e_on, e_tg = net.noise(0).cpu().numpy(), net.noise(1).cpu().numpy()
    n, ne = n_mu(fc, A, du), noisy_end(fc, A, du)
    eff32 = P_on[:n].copy()
    eff32[TRUNK:ne] += P_on[n:] * factors(e_on, fc, A, du, F32)
    pool, _ = kinkfree.pool(oracle, eff32, fc, seed=fc + int(du))
    s = np.array(pool[:B])
    rng = np.random.default_rng(1000 * fc + 10 * A + B + N)
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.6, 0.2, 0.2])
    t = (rng.random(B) < 0.25).astype(np.uint8)
    if B > 1:
        t[0], t[1] = 1, 0
    with torch.no_grad():
        Q, QT = eff64(P_on, e_on, fc, A, du), eff64(P_tg, e_tg, fc, A, du)
    s2 = rand_states(rng, B)
    for _ in range(20):
        with torch.no_grad():
            h2o, h2t = trunk64(Q, s2, fc, A), trunk64(QT, s2, fc, A)
            qo, qt = qbar_from_h(Q, h2o, K, 1.0, fc, A), qbar_from_h(QT, h2t, K, 1.0, fc, A)
        top = lambda q: (lambda v: (v[:, 0] - v[:, 1]).numpy())(q.topk(2, 1).values)
        bad = (top(qo) < 10 * Q_ATOL) | (top(qt) < 10 * Q_ATOL)
        if not bad.any():
            break
        s2[bad] = rand_states(rng, int(bad.sum()))
    assert not bad.any()
    tau, drawn = np.empty((B, N), F32), 0
    with torch.no_grad():
        for bi in range(B):
            for i in range(N):
                while True:
                    x = max(F32(rng.random()), F32(2.0 ** -24))
                    drawn += 1
                    if pre64(Q, np.array([x]), fc, A).abs().min().item() >= TAU_MARGIN:
                        break
                tau[bi, i] = x
    assert B * N >= 0.8 * drawn
    taup = np.maximum(rng.random((B, Np)).astype(F32), F32(2.0 ** -24))
    rd = torch.as_tensor(np.where(r == F32(0.1), 0.1, r.astype(np.float64)))
    nd = torch.as_tensor((t == 0).astype(np.float64))
    ar = torch.arange(B)
    pg = t64(P_on).requires_grad_(True)
    q = eff64(pg, e_on, fc, A, du)
    th = theta_from_h(q, trunk64(q, s, fc, A), tau, fc, A)[ar, :, torch.as_tensor(a.astype(np.int64))]
    out = {}
    for dq, qsel in ((0, qt), (1, qo)):
        astar = qsel.argmax(1)
        with torch.no_grad():
            T = rd[:, None] + nd[:, None] * GAMMA * theta_from_h(QT, h2t, taup, fc, A)[ar, :, astar]
        loss, lb = torch_iqn_loss(th, T, tau, 1.0)
        grad, = torch.autograd.grad(loss, pg, retain_graph=True)
        out[dq] = (loss.item(), T.numpy(), grad.numpy(), lb.detach().numpy())
    with torch.no_grad():                                            # Munchausen's inputs: Qbar-(s', .), Qbar-(s, .), theta-(s', c; tau'_j) of the target net
        hs = trunk64(QT, s, fc, A)
        mq = (qt.numpy(), qbar_from_h(QT, hs, K, 1.0, fc, A).numpy(), theta_from_h(QT, h2t, taup, fc, A).numpy())
    return dict(s=s, a=a, r=r, s2=s2, t=t, tau=tau, taup=taup, out=out, th=th, pg=pg, mq=mq)


def check_noisy_grads(g, g0, e32, fc, A, du):
    """check_grads' bounds (rtol 2e-3, atol 2e-5 x the tensor's largest reference element) for every mu tensor and every sigma tensor; then
    the sigma part == float32(g[q] e(q)) bit for bit, from the exported mu part"""
    n, ne = n_mu(fc, A, du), noisy_end(fc, A, du)
    if du:
        check_grads_dueling(g[:n], g0[:n], fc, A)
    else:
        check_iqn_grads(g[:n], g0[:n], fc, A)
    for k, (w, fi, fo, _, _) in enumerate(layers(fc, A, du)[0]):
        for name, lo, hi in ((f"sigma_W of layer {k}", w, w + fi * fo), (f"sigma_b of layer {k}", w + fi * fo, w + (fi + 1) * fo)):
            lo, hi = n + lo - TRUNK, n + hi - TRUNK
            scale = np.abs(g0[lo:hi]).max()
            assert scale > 0, name
            np.testing.assert_allclose(g[lo:hi], g0[lo:hi], rtol=2e-3, atol=2e-5 * scale, err_msg=name)
    assert np.array_equal(g[n:], (g[TRUNK:ne] * e32).astype(F32))


GRAD_CASES = [(128, 2, False, TAUS, 1), (128, 2, False, TAUS, 32), (128, 2, False, TAUS, 256), (128, 3, True, TAUS, 32), (128, 3, True, TAUS, 256),
              (128, 2, True, (1, 1, 1), 1), (128, 8, False, TAUS, 32), (384, 3, True, TAUS, 32)]


def grad_case(torch, oracle, fc, A, du, taus, B):
    key = (fc, A, du, taus, B)
    if key not in _grads:
        net, p_on, p_tg = make_noisy(oracle, fc, A, du, taus=taus, max_batch=max(B, 32))
        net.reset_noise(0, 5, 6); net.reset_noise(1, 5, 6)
        _grads[key] = (net, p_on, p_tg, ref_step(oracle, net, p_on, p_tg, fc, A, du, taus, B))
    return _grads[key]


@pytest.mark.parametrize("fc,A,du,taus,B", GRAD_CASES)
def test_train_step_against_autograd(torch_cuda, oracle, fc, A, du, taus, B):
    """gathered, gradient-exporting, double_q 0 and 1: the loss, the targets, every mu tensor and every sigma tensor; nothing is masked"""
    torch = torch_cuda
    net, p_on, p_tg, ref = grad_case(torch, oracle, fc, A, du, taus, B)
    e32 = factors(net.noise(0).cpu().numpy(), fc, A, du, F32)
    d = lambda x: torch.from_numpy(x).cuda()
    for dq in (0, 1):
        want, T0, g0, _ = ref["out"][dq]
        grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        loss, T = net.iqn_train_step(d(ref["s"]), d(ref["a"]), d(ref["r"]), d(ref["s2"]), d(ref["t"]), gamma=GAMMA, double_q=bool(dq), tau=d(ref["tau"]),
                                     tau_next=d(ref["taup"]), flat_grad=grad)
        print(f"noisy iqn fc={fc} A={A} dueling={du} B={B} double_q={dq}: loss {loss.item()!r} / {want!r}; max |dT| {np.abs(T.cpu().numpy() - T0).max():.3e}")
        np.testing.assert_allclose(T.cpu().numpy(), T0, rtol=0, atol=Q_ATOL)
        np.testing.assert_allclose(loss.item(), want, rtol=1e-4, atol=1e-6)
        check_noisy_grads(grad.cpu().numpy(), g0, e32, fc, A, du)
    assert np.array_equal(net.store_params(0).cpu().numpy(), p_on) and net.overflow_count() == 0          # gradient-only mode


def test_weighted_train_step_against_autograd(torch_cuda, oracle):
    """the prioritized form: w in (0, 1], abs_err = l_b without the weight"""
    torch = torch_cuda
    import torch as th_
    fc, A, du, taus, B = 128, 3, True, TAUS, 32
    net, p_on, _, ref = grad_case(torch, oracle, fc, A, du, taus, B)
    _, T0, _, lb0 = ref["out"][1]
    w = (1.0 - np.random.default_rng(B).random(B)).astype(F32)
    w[0], w[1] = 1.0, F32(2.0 ** -10)
    _, lb = torch_iqn_loss(ref["th"], th_.as_tensor(T0), ref["tau"], 1.0)
    lossw = (th_.as_tensor(w.astype(np.float64)) * lb).mean()
    g0, = th_.autograd.grad(lossw, ref["pg"], retain_graph=True)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, ae, T = net.iqn_per_train_step(d(ref["s"]), d(ref["a"]), d(ref["r"]), d(ref["s2"]), d(ref["t"]), d(w), gamma=GAMMA, double_q=True,
                                         tau=d(ref["tau"]), tau_next=d(ref["taup"]), flat_grad=grad)
    np.testing.assert_allclose(T.cpu().numpy(), T0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss.item(), lossw.item(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ae.cpu().numpy(), lb0, rtol=1e-4, atol=1e-6)
    check_noisy_grads(grad.cpu().numpy(), g0.numpy(), factors(net.noise(0).cpu().numpy(), fc, A, du, F32), fc, A, du)


def test_munchausen_train_step_against_autograd(torch_cuda, oracle):
    """the Munchausen target at (temp, alpha, l0) = (1, 0.9, -1) on the noisy net: T within tests/test_miqn_host.py::miqn_tol, every mu and
    sigma tensor within check_grads' own bounds -- what tests/test_gpu_miqn.py asks of the non-noisy net at temp = 1"""
    torch = torch_cuda
    import torch as th_
    fc, A, du, taus, B = 128, 2, False, TAUS, 32
    net, p_on, _, ref = grad_case(torch, oracle, fc, A, du, taus, B)
    temp, alpha, l0 = 1.0, 0.9, -1.0
    qn, qs, th_all = ref["mq"]
    m = miqn_target64(qn, qs, th_all, ref["a"], ref["r"], ref["t"], GAMMA, temp, alpha, l0)
    tol = miqn_tol(m["S"], temp)
    loss0, _ = torch_iqn_loss(ref["th"], th_.as_tensor(m["T"]), ref["tau"], 1.0)
    g0, = th_.autograd.grad(loss0, ref["pg"], retain_graph=True)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    net.set_iqn_munchausen(True, temp, alpha, l0)
    try:
        loss, T = net.iqn_train_step(d(ref["s"]), d(ref["a"]), d(ref["r"]), d(ref["s2"]), d(ref["t"]), gamma=GAMMA, tau=d(ref["tau"]), tau_next=d(ref["taup"]),
                                     flat_grad=grad)
    finally:
        net.set_iqn_munchausen(False)
    assert (np.abs(T.cpu().numpy() - m["T"]) <= tol).all()
    np.testing.assert_allclose(loss.item(), loss0.item(), rtol=1e-4, atol=tol.mean())
    check_noisy_grads(grad.cpu().numpy(), g0.numpy(), factors(net.noise(0).cpu().numpy(), fc, A, du, F32), fc, A, du)


# ================================================================================================================ 5: per-env acting
def restate_env(net, s, seed, step, envs, K, eta, fc, A, du):
    """float64 Qbar of the given envs (rows of the u8 states s), each through its own effective weights, from the documented draws"""
    P, nz = net.store_params(0).cpu().numpy(), net.noise_size
    return np.stack([qbar64(P, env_noise(seed, step, e, nz), s[e:e + 1], K, eta, fc, A, du)[0] for e in envs])


def check_env(net, nib, s, seed, step, K, eta, fc, A, du, what):
    n = nib.shape[0]
    a, q = net.act_nib_env_noise(nib, 0.0, seed=seed, step=step, want_q=True)
    a, q = a.cpu().numpy(), q.cpu().numpy()
    envs = chosen(n)
    q0 = restate_env(net, s, seed, step, envs, K, eta, fc, A, du)
    err = np.abs(q[envs] - q0).max()
    print(f"per-env {what}: max |dQ| {err:.3e}")
    assert err <= ENV_ATOL, what
    top = np.sort(q0, 1)
    margin = top[:, -1] - top[:, -2] > 1e-3
    assert np.array_equal(a[envs][margin], q0.argmax(1)[margin]), what
    return q


@pytest.mark.parametrize("du", HEADS)
@pytest.mark.parametrize("n", [1, 37, 256, 300])
def test_per_env_acting_matches_the_restatement(torch_cuda, oracle, du, n):
    fc, A = 128, 2
    nib, s = states(n)
    for scale in (1.0, 1e-3):
        for K, eta in ((32, 1.0), (32, 0.25), (1, 1.0), (1, 0.25)):
            net, _, _ = make_noisy(oracle, fc, A, du, taus=(4, 5, K), max_batch=max(n, 32), sigma_scale=scale)
            if eta != 1.0:
                net.set_iqn_risk(eta)
            net.reset_noise(0, 4, 4)                                 # (never read by the call)
            q = check_env(net, nib, s, 2 ** 33 + 11, 2 ** 32 + 6, K, eta, fc, A, du, f"dueling={du} n={n} sigma x {scale} K={K} eta={eta}")
            if scale == 1.0 and n > 1:
                assert np.abs(q[:, 1] - q[:, 0]).std() > 0
            assert net.overflow_count() == 0


@pytest.mark.parametrize("fc,A,du", [(128, 3, False), (128, 8, True), (384, 3, True)])
def test_per_env_acting_on_the_generic_head(torch_cuda, oracle, fc, A, du):
    """A != 2 (the generic action template), MAXA once, FC 384 (a stage of 256 units and one of 128) once; both sides of the fused-path switch"""
    for n in (37, 300):
        nib, s = states(n)
        net, _, _ = make_noisy(oracle, fc, A, du, max_batch=max(n, 32))
        check_env(net, nib, s, 3, 5, TAUS[2], 1.0, fc, A, du, f"fc={fc} A={A} dueling={du} n={n}")


@pytest.mark.parametrize("du", HEADS)
@pytest.mark.parametrize("n", [37, 1024])
def test_zero_sigma_is_mean_mode_acting_bit_for_bit(torch_cuda, oracle, du, n):
    nib, _ = states(n)
    net, _, _ = make_noisy(oracle, du=du, max_batch=n, sigma0=0.0)
    for eps in (0.0, 0.3):
        a, q = (x.clone() for x in net.act_nib_env_noise(nib, eps, seed=3, step=8, want_q=True))
        net.mean_noise(0)
        a0, q0 = net.act_nib(nib, eps, seed=3, step=8, want_q=True)
        assert torch_cuda.equal(q, q0) and torch_cuda.equal(a, a0), eps
        net.reset_noise(0, 1, 1)


@pytest.mark.parametrize("du", HEADS)
def test_keyed_by_env_distinct_and_repeatable(torch_cuda, oracle, du):
    torch = torch_cuda
    nib, _ = states(1024)
    net, _, _ = make_noisy(oracle, du=du, max_batch=1024)
    a, q = (x.clone() for x in net.act_nib_env_noise(nib, 0.0, seed=9, step=5, want_q=True))
    a3, q3 = net.act_nib_env_noise(nib[:300], 0.0, seed=9, step=5, want_q=True)
    assert torch.equal(q[:300], q3) and torch.equal(a[:300], a3)    # rows [0, 300) of 1024 envs == 300 envs
    same_nib = nib[7:8].repeat(300, 1).contiguous()                  # one state in every row
    q = net.act_nib_env_noise(same_nib, 0.0, seed=1, step=2, want_q=True)[1].clone()
    assert len(np.unique((q[:, 1] - q[:, 0]).cpu().numpy())) == 300
    assert torch.equal(net.act_nib_env_noise(same_nib, 0.0, seed=1, step=2, want_q=True)[1], q)
    q2 = net.act_nib_env_noise(same_nib, 0.0, seed=1, step=3, want_q=True)[1]
    assert not torch.equal(q2, q)
    net.mean_noise(0)
    qm = net.act_nib(same_nib, 0.0, want_q=True)[1]
    assert (qm == qm[0]).all()


@pytest.mark.parametrize("n", [37, 300])
def test_the_per_env_call_has_no_side_effects(torch_cuda, oracle, n):
    torch = torch_cuda
    nib, _ = states(n)
    for du in HEADS:
        net, _, _ = make_noisy(oracle, du=du, max_batch=max(n, 32), lr=1e-3)
        net.reset_noise(0, 5, 6); net.reset_noise(1, 5, 6)
        net.iqn_train_step(*a_batch(torch, np.random.default_rng(1), 32, 2), gamma=GAMMA, double_q=True, seed=1, step=1)      # (Adam state and sigma planes in use)
        before, ovf = frozen(net), net.overflow_count()
        a0, q0 = (x.clone() for x in net.act_nib(nib, 0.0, seed=2, step=3, want_q=True))
        s8 = torch.from_numpy(rand_states(np.random.default_rng(0), 8)).cuda()
        f0 = net.forward(s8).clone()
        net.act_nib_env_noise(nib, 0.0, seed=2, step=3)
        torch.cuda.synchronize()
        assert same_frozen(torch, frozen(net), before) and net.overflow_count() == ovf, du
        a1, q1 = net.act_nib(nib, 0.0, seed=2, step=3, want_q=True)
        assert torch.equal(q0, q1) and torch.equal(a0, a1) and torch.equal(net.forward(s8), f0), du      # the sample's fold is back


# ================================================================================================================ 6: the fused steps
PLAN = [(False, False, 0.5), (True, True, 0.0), (True, False, 0.5), (False, True, 0.0), (True, True, 0.1), (True, False, 1.0), (True, True, 0.3),
        (False, False, 0.0), (True, False, 0.0), (True, True, 0.5), (True, False, 0.2), (True, True, 0.0)]      # 12 steps: (train, double_q, epsilon)


def composed_act(net, nib, mode, eps, seed, k):
    """what the header says a step does up to the env step"""
    if mode == "shared":
        net.reset_noise(0, seed, k)
        return net.act_nib(nib, eps, seed=seed, step=k)
    return net.act_nib_env_noise(nib, eps, seed=seed, step=k)


def composed_noise(net, mode, seed, k, train):
    if mode == "env":
        net.reset_noise(0, seed, k)
    if train:
        net.reset_noise(1, seed, k)


@pytest.mark.parametrize("mode", ["shared", "env"])
@pytest.mark.parametrize("N", [37, 300])
def test_iqn_step_equals_the_composed_calls(torch_cuda, oracle, N, mode):
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnStep, VecGameState, VecReplay, iqn_train_from_replay
    seed, batch, du = (3 << 32) | 9, 32, N == 300

    def make():
        env, rep = VecGameState(N, seed=5), VecReplay(8000, N)
        net, _, _ = make_noisy(oracle, du=du, max_batch=max(N, batch))
        net.set_acting_noise(mode)
        rep.seed(7, "cpython")
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = make()
    e2, r2, n2, nib2 = make()
    steps = {dq: IqnStep(e1, r1, n1, batch, GAMMA, dq) for dq in (False, True)}
    for k, (train, dq, eps) in enumerate(PLAN):
        one = steps[dq]
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = composed_act(n2, nib2, mode, eps, seed, k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        idx = r2.push_sample(e2.frame_bits, a2, rew, term, batch)
        assert torch.equal(a1, a2) and torch.equal(one.idx, idx) and torch.equal(nib1, nib2), k
        composed_noise(n2, mode, seed, k, train)
        if train:
            loss, a_o, r_o, t_o = iqn_train_from_replay(r2, n2, idx, gamma=GAMMA, double_q=dq, seed=seed, step=k)
            assert torch.equal(one.loss, loss) and torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
        assert same_frozen(torch, frozen(n1), frozen(n2)), k
    x = torch.from_numpy(rand_states(np.random.default_rng(0), 8)).cuda()
    assert torch.equal(n1.forward(x), n2.forward(x)) and torch.equal(n1.forward(x, 1), n2.forward(x, 1))      # ... and the effective vectors and folds
    assert np.array_equal(e1.get_state(), e2.get_state()) and np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n1.overflow_count() == 0


@pytest.mark.parametrize("mode", ["shared", "env"])
@pytest.mark.parametrize("N,n_step", [(37, 1), (300, 3)])
def test_iqn_per_step_equals_the_composed_calls(torch_cuda, oracle, N, n_step, mode):
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep, VecGameState, VecReplay, iqn_per_train_from_replay
    seed, batch, du = (3 << 32) | 9, 32, N == 37

    def world():
        env = VecGameState(N, seed=5)
        rep = VecReplay(8192, N, prioritized=True, n_step=n_step, gamma=GAMMA)
        rep.seed(7)
        net, _, _ = make_noisy(oracle, du=du, max_batch=max(N, batch))
        net.set_acting_noise(mode)
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = world()
    e2, r2, n2, nib2 = world()
    steps = {dq: IqnPerStep(e1, r1, n1, batch, GAMMA, dq) for dq in (False, True)}
    for k, (train, dq, eps) in enumerate(PLAN):
        train = train and k >= n_step - 1
        one = steps[dq]
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = composed_act(n2, nib2, mode, eps, seed, k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        r2.push(e2.frame_bits, a2, rew, term)
        assert torch.equal(a1, a2) and torch.equal(nib1, nib2), k
        if train:
            idx, isw = r2.sample(batch)
            idx, isw = idx.clone(), isw.clone()
        composed_noise(n2, mode, seed, k, train)
        if train:
            loss, a_o, r_o, t_o, ae = iqn_per_train_from_replay(r2, n2, idx, isw.to(torch.float32), gamma=GAMMA, double_q=dq, seed=seed, step=k)
            assert torch.equal(one.idx, idx) and torch.equal(one.isw, isw), k
            assert torch.equal(one.loss, loss) and torch.equal(one.abs_err, ae) and torch.equal(one.a, a_o), k
            r2.update_priorities(idx, abs_err=ae.clone())
        assert same_frozen(torch, frozen(n1), frozen(n2)), k
        x, y = tree_state(r1), tree_state(r2)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], k
    assert np.array_equal(e1.get_state(), e2.get_state()) and np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


# ================================================================================================================ 7: refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import ALGOS, IqnStep, QNet, TrainSteps, VecGameState, VecReplay, VecStep, train_from_replay
    lib = L.lib()
    N, B = 16, 8
    net, _, _ = make_noisy(oracle, du=True)
    net.reset_noise(0, 1, 2); net.reset_noise(1, 1, 2)
    env, rep = VecGameState(N, seed=3), VecReplay(2000, N)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    for _ in range(6):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        rep.push(env.frame_bits, acts, env.reward, env.terminal)
    rep.seed(9, "cpython")
    blob, before, envs = np.asarray(rep.state_blob()).copy(), frozen(net), env.get_state().copy()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    s, a, r, s2, t = rep.gather(idx)

    def untouched():
        torch.cuda.synchronize()
        return np.array_equal(np.asarray(rep.state_blob()), blob) and same_frozen(torch, frozen(net), before) and np.array_equal(env.get_state(), envs)

    fails = lambda rc, word: rc == -1 and word in lib.fb_last_error().decode()
    h = C.c_void_p()
    ok = (0, 128, 2, 8, 8, 32, 1.0, 0.5)
    for bad, word in ((dict(sigma0=-0.5), "fb_qnet_create_iqn_noisy: sigma0 must be finite and >= 0"), (dict(sigma0=float("nan")), "sigma0 must be finite"),
                      (dict(sigma0=float("inf")), "sigma0 must be finite"), (dict(dueling=2), "dueling must be 0 or 1"),
                      (dict(fc=100), "fb_qnet_create_iqn_noisy: fc_width must be a multiple of 128"), (dict(A=1), "n_actions must be in 2..8"),
                      (dict(A=9), "n_actions must be in 2..8"), (dict(N=0), "n_tau=0"), (dict(Np=65), "n_tau_next=65"), (dict(K=0), "n_tau_act=0"),
                      (dict(kappa=0.0), "kappa must be finite and > 0")):
        v = dict(zip(("dueling", "fc", "A", "N", "Np", "K", "kappa", "sigma0"), ok))
        v.update(bad)
        rc = lib.fb_qnet_create_iqn_noisy(v["dueling"], v["fc"], v["A"], v["N"], v["Np"], v["K"], C.c_float(v["kappa"]), C.c_float(v["sigma0"]), 32, C.byref(h))
        assert fails(rc, word) and not h.value, bad
    assert fails(lib.fb_qnet_create_iqn_noisy(0, 128, 2, 8, 8, 32, C.c_float(1.0), C.c_float(0.5), 32, None), "out is NULL")
    # the older creators and the noise calls on a non-noisy net keep their words
    for arch in (L.ARCH_IQN, L.ARCH_IQN_DUELING):
        assert fails(lib.fb_qnet_create_c51_noisy(arch, 128, 2, 51, C.c_float(-10), C.c_float(10), C.c_float(0.5), 32, C.byref(h)),
                     f"arch must be FB_ARCH_C51 (2) or FB_ARCH_C51_DUELING (3), got {arch} (noisy layers are offered on the C51 heads only)")
    assert fails(lib.fb_qnet_create(L.ARCH_IQN, 128, 2, 32, C.byref(h)), "an IQN net is made by fb_qnet_create_iqn (it needs N, N', K and kappa)")
    assert fails(lib.fb_qnet_create(L.ARCH_IQN_DUELING, 128, 2, 32, C.byref(h)), "fb_qnet_create: arch must be 0 or 1")
    with pytest.raises(ValueError, match="noisy layers are offered on the C51 heads only \\(\\('c51', 'c51dueling'\\)\\), not arch 'iqn'"):
        QNet(2, 128, "iqn", noisy=True)
    iqn = QNet(2, 128, "iqn", max_batch=32)
    iqn.init_params(1)
    with pytest.raises(ValueError, match="reset_noise needs a noisy net"):
        iqn.reset_noise()
    out = torch.zeros(4096, device="cuda")
    a8 = torch.zeros(N, dtype=torch.uint8, device="cuda")
    assert fails(lib.fb_qnet_reset_noise(iqn.h, 0, 0, 0, 0, None), "fb_qnet_reset_noise: not a noisy net (fb_qnet_create_c51_noisy)")
    assert fails(lib.fb_qnet_get_noise(iqn.h, 0, L.ptr(out)), "fb_qnet_get_noise: not a noisy net (fb_qnet_create_c51_noisy)")
    assert fails(lib.fb_qnet_set_acting_noise(iqn.h, 1), "fb_qnet_set_acting_noise: not a noisy net (fb_qnet_create_c51_noisy)")
    assert fails(lib.fb_qnet_act_nib_env_noise(iqn.h, L.ptr(nib), N, C.c_float(0), 0, 0, L.ptr(a8), None, None),
                 "per-env acting noise needs a noisy net (fb_qnet_create_c51_noisy)")
    assert lib.fb_qnet_is_noisy(iqn.h) == 0
    # what a noisy IQN net is still refused, before any launch or counter change
    for algo in sorted(ALGOS):
        with pytest.raises(ValueError, match="fb_qnet_train_step: an IQN net trains through"):
            net.train_step(algo, s, a, r, s2, t, isw=r)
        with pytest.raises(ValueError, match="fb_train_from_replay: an IQN net"):
            train_from_replay(rep, net, algo, idx, isw=r)
    with pytest.raises(ValueError, match="fb_train_steps"):
        TrainSteps(rep, net, B, "dqn")(1)
    for mode in ("shared", "env"):
        net.set_acting_noise(mode)
        with pytest.raises(ValueError, match="fb_vec_step: an IQN net"):
            VecStep(env, rep, net, B, "dqn")(0.1, train=True)
    net.set_acting_noise("shared")
    buf = VecStep(env, rep, net, B, "dqn").buf
    assert lib.fb_vec_step_dp(None, env.h, rep.h, net.h, C.byref(buf), N, 0, B, 0.1, 0, 0, 1, 0.99, 0, None) == -1
    for call, msg in ((lambda: net.set_train_dtype("bf16"), "an IQN net trains in FB_DTYPE_F32 only"),
                      (lambda: net.set_inference_dtype("bf16"), "an IQN net computes in FB_DTYPE_F32 only"),
                      (lambda: net.set_acting_noise("per-env"), "acting noise must be one of"),
                      (lambda: net.act_nib_env_noise(torch.zeros((97, nib.shape[1]), dtype=torch.uint8, device="cuda"), 0.0), "exceeds 3\\*max_batch")):
        with pytest.raises(ValueError, match=msg):
            call()
    assert fails(lib.fb_qnet_reset_noise(net.h, 0, 0, 0, 7, None), "mode must be FB_NOISE_SAMPLE or FB_NOISE_MEAN")
    assert fails(lib.fb_qnet_set_acting_noise(net.h, 2), "mode must be FB_ACT_NOISE_SHARED or FB_ACT_NOISE_PER_ENV")
    sb = IqnStep(env, rep, net, B)
    assert fails(lib.fb_iqn_step(env.h, rep.h, net.h, C.byref(sb.buf), N, 0, 33, C.c_float(0.1), 0, 0, 1, 0.99, None), "exceeds min(max_batch, 256)")
    assert fails(lib.fb_iqn_step(env.h, rep.h, net.h, C.byref(sb.buf), N + 1, 0, B, C.c_float(0.1), 0, 0, 1, 0.99, None), "does not match")
    assert untouched()


# ================================================================================================================ 8: the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.veciqn import VecIQN
    v = VecIQN(16, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, lr=1e-4, explore=20, replace_target_iter=3, max_grad_norm=5.0,
               n_tau=4, n_tau_next=5, n_tau_act=6, noisy=True, **kw)
    losses = [v.step().clone() for _ in range(n)]
    return v, losses


LOOPS = [dict(acting_noise="shared"), dict(acting_noise="env"), dict(acting_noise="env", prioritized=True, dueling=True, n_step=3, double_q=True)]


@pytest.mark.parametrize("kw", LOOPS)
def test_vec_iqn_noisy_loop_and_checkpoint(torch_cuda, tmp_path, kw):
    torch = torch_cuda
    from dqnflappybird_amd.veciqn import VecIQN
    v, losses = run_steps(200, **kw)
    assert all(torch.isfinite(l).all() for l in losses) and losses[-1][0] > 0 and v.net.overflow_count() == 0
    assert v.noisy and v.net.noisy and v.initial_epsilon == 0.0 and v.epsilon == 0.0 and v.net.acting_noise == kw["acting_noise"]
    assert v.net.arch == ("iqnduelingnoisy" if kw.get("dueling") else "iqnnoisy") and v.timeStep == 200
    n = n_mu(128, 2, bool(kw.get("dueling")))
    p0 = v.net.store_params(0)
    fresh = VecIQN(16, batch=8, fc_width=128, seed=4, capacity=2000, noisy=True, **kw).net.store_params(0)
    assert not torch.equal(p0[:n], fresh[:n]) and not torch.equal(p0[n:], fresh[n:])                  # mu and sigma both trained
    v, losses = run_steps(7, **kw)
    st, nz = loop_state(v), (v.net.noise(0).clone(), v.net.noise(1).clone())
    assert bool(nz[0].any())                                         # the last step's online sample
    x = torch.from_numpy(rand_states(np.random.default_rng(0), 8)).cuda()
    q = v.net.forward(x).clone()
    for mode in ("mean", "sample"):                                  # evaluate() leaves the training state untouched: the sample is put back
        res = v.evaluate(n_envs=32, episodes=1, max_steps=200, noise=mode)
        assert res.score.shape == (32, 1) and same_loop(torch, loop_state(v), st), mode
        assert torch.equal(v.net.noise(0), nz[0]) and torch.equal(v.net.noise(1), nz[1]) and torch.equal(v.net.forward(x), q), mode
    path = str(tmp_path / "noisy.npz")
    v.save(path)
    z = np.load(path)
    assert str(z["head"][0]) == "iqn" and int(z["noisy"][0]) == 1 and float(z["sigma0"][0]) == 0.5 and str(z["acting_noise"][0]) == kw["acting_noise"]
    base = {k: w for k, w in kw.items() if k != "acting_noise"}
    mk = lambda **over: VecIQN(16, **{**dict(batch=8, fc_width=128, seed=4, capacity=2000, n_tau=4, n_tau_next=5, n_tau_act=6, noisy=True), **kw, **over})
    plain = VecIQN(16, batch=8, fc_width=128, seed=4, capacity=2000, n_tau=4, n_tau_next=5, n_tau_act=6, **base)
    with pytest.raises(ValueError, match="holds a noisy net, this VecIQN has a non-noisy net \\(noisy=False"):
        plain.load(path)
    other = str(tmp_path / "plain.npz")
    plain.save(other)
    assert "noisy" not in np.load(other).files
    resumed = mk(lr=3e-5)
    with pytest.raises(ValueError, match="holds a non-noisy net, this VecIQN has a noisy net \\(noisy=True"):
        resumed.load(other)
    with pytest.raises(ValueError, match="was written with sigma0 = 0.5, this VecIQN has sigma0 = 0.25"):
        mk(sigma0=0.25).load(path)
    with pytest.raises(ValueError, match="was written with acting_noise = "):
        mk(acting_noise="shared" if kw["acting_noise"] == "env" else "env").load(path)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and torch.equal(resumed.net.noise(0), nz[0]) and torch.equal(resumed.net.forward(x), q)
    more = [resumed.step().clone() for _ in range(4)]
    straight, l11 = run_steps(11, **kw)
    assert all(torch.equal(a, b) for a, b in zip(more, l11[7:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=128)
    assert net.arch == v.net.arch and net.noisy and torch.equal(net.store_params(), v.net.store_params()) and not net.noise(0).any()
    r2 = evaluate(net, 32, 1, 200)
    res = v.evaluate(n_envs=32, episodes=1, max_steps=200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    v.run(1, log_every=1)
