"""QR-DQN on the MI355X (include/fbdqn.h): the quantile head, Q = the mean of the quantiles, the target, the
quantile Huber loss and its gradients against a float64 torch-CPU restatement written here (the trunk of
tests/test_oracle_qnet.py::torch_forward, the head, the pairwise loss with autograd), and every path that trains or plays a QR net
against its composed calls, bit for bit."""
import ctypes
import zlib

import numpy as np
import pytest

from tests.test_gpu_c51 import _batch, greedy_next, head0
from tests.test_gpu_c51_dueling import ref_logits_d
from tests.test_gpu_eval import composed as composed_eval
from tests.test_gpu_nstep import played
from tests.test_gpu_nstep_per import per_memory
from tests.test_oracle_qnet import rand_states, tensor_bounds, torch_forward
from tests.test_qr_host import np_qr_loss

pytestmark = pytest.mark.gpu
GAMMA = 0.99
FC = 512
HEAD0 = head0()
DOUBLE = ("qrdouble", "qrdoubleper")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_qr(N=51, kappa=1.0, arch="qr", max_batch=256, seed=3, head_scale=1.0, A=2, fc=FC):
    """a QR net scaled as tests/test_gpu_c51.py::make_c51 scales a C51 net (weights x 3, the head x head_scale more)"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, arch, max_batch=max_batch, n_quantiles=N, kappa=kappa)
    ps = []
    for which in (0, 1):
        net.init_params(seed + which, which)
        p = net.store_params(which).cpu().numpy() * 3.0
        p[head0(fc):] *= head_scale
        net.load_params(p, which)
        ps.append(p)
    return net, ps[0], ps[1]


def ref_theta(p, s, N, arch="qr", A=2, fc=FC):
    """[B, A, N] float64 quantiles: the plain trunk with an A N-column head, or the dueling head's V + Adv - mean_a Adv"""
    import torch
    if arch == "qrdueling":
        return ref_logits_d(p, s, N, A, fc)
    return torch_forward(torch.as_tensor(p, dtype=torch.float64), torch.as_tensor(s, dtype=torch.float64), fc, A * N).view(len(s), A, N)


def ref_train(p_on, p_tg, s, a, r, s2, t, w, G, algo, N, kappa, dev_astar=None, arch="qr", A=2, fc=FC):
    """-> (loss, flat gradient, l_b per sample, max |u|) in float64 with autograd; w = None: the uniform algos' mean"""
    import torch
    P = torch.tensor(p_on, dtype=torch.float64, requires_grad=True)
    B = len(s)
    with torch.no_grad():
        tt = ref_theta(torch.tensor(p_tg, dtype=torch.float64), s2, N, arch, A, fc)
        sel = ref_theta(P.detach(), s2, N, arch, A, fc) if algo in DOUBLE else tt
        astar = greedy_next(sel.mean(-1), dev_astar)
        T = torch.as_tensor(r.astype(np.float64))[:, None] + G * (1.0 - torch.as_tensor(t.astype(np.float64)))[:, None] * tt[torch.arange(B), astar]
    th = ref_theta(P, s, N, arch, A, fc)[torch.arange(B), torch.as_tensor(a, dtype=torch.long)]
    u = T[:, None, :] - th[:, :, None]                       # [b, i, j]
    tau = (2 * torch.arange(N, dtype=torch.float64) + 1) / (2 * N)
    wt = (tau[None, :, None] - (u < 0).double()).abs()
    hub = torch.where(u.abs() <= kappa, 0.5 * u * u, kappa * (u.abs() - 0.5 * kappa))
    lb = (wt * hub / kappa).sum((1, 2)) / N
    loss = (torch.as_tensor(w, dtype=torch.float64) * lb).mean() if w is not None else lb.mean()
    loss.backward()
    # (one sample through the host test's literal double loop: the two restatements agree)
    l0, _ = np_qr_loss(th[0].detach().numpy(), T[0].numpy(), kappa)
    assert abs(l0 - lb[0].item()) < 1e-9 * max(1.0, l0)
    return loss.item(), P.grad.numpy(), lb.detach().numpy(), u.detach().abs().max().item()


def check_grads(g, g0, N, arch="qr", A=2, fc=FC):
    """tests/test_gpu_c51.py::_check_grads's tolerances, per tensor: the head tensors elementwise, the rest relative L2"""
    tensors = tensor_bounds(fc, A, "c51dueling" if arch == "qrdueling" else "c51", N)
    assert tensors[-1][2] == len(g0)
    for k, (_, lo, hi) in enumerate(tensors):
        ref, got = g0[lo:hi], g[lo:hi]
        scale = np.abs(ref).max()
        assert scale > 0, (lo, hi)
        if k >= 8:
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=f"params[{lo}:{hi}]")
        else:
            err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert err < 2e-3, (lo, hi, err)


def frozen(net):
    m, v, p = net.adam_state()
    return net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), p.copy()


def same(x, y):
    import torch
    return all(torch.equal(i, j) if torch.is_tensor(i) else np.array_equal(i, j) for i, j in zip(x, y))


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("N,A,arch", [(51, 2, "qr"), (11, 2, "qr"), (64, 2, "qr"), (42, 3, "qr"), (51, 2, "qrdueling")])
def test_forward_and_quantiles_match_the_restatement(torch_cuda, N, A, arch):
    torch = torch_cuda
    net, p_on, p_tg = make_qr(N, arch=arch, A=A, max_batch=700)
    assert net.quantiles() == (N, 1.0) and net.support is None
    rng = np.random.default_rng(N + A)
    s = rand_states(rng, 2048)
    with torch.no_grad():
        ref = {w: ref_theta(p, s, N, arch, A) for w, p in ((0, p_on), (1, p_tg))}
    sd = torch.from_numpy(s).cuda()
    for B in (1, 32, 255, 256, 2048):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            th = net.forward_quantiles(sd[:B].contiguous(), which).cpu().numpy()
            want = ref[which][:B].numpy()
            tol = 1e-4 * max(1.0, np.abs(want).max())
            np.testing.assert_allclose(th, want, rtol=0, atol=tol, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, want.mean(-1), rtol=0, atol=tol, err_msg=f"B={B} which={which}")
    # the quantiles of one action differ (the test would be weak otherwise)
    assert ref[0].std(-1).min().item() > 1e-3


@pytest.mark.parametrize("arch,c51arch", [("qr", "c51"), ("qrdueling", "c51dueling")])
def test_initial_parameters_equal_the_c51_nets(torch_cuda, arch, c51arch):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    for N, A in ((51, 2), (21, 3)):
        q = QNet(A, FC, arch, max_batch=8, n_quantiles=N)
        c = QNet(A, FC, c51arch, max_batch=8, n_atoms=N)
        assert q.n_params == c.n_params
        for which, seed in ((0, 5), (1, 6)):
            q.init_params(seed, which); c.init_params(seed, which)
            assert torch.equal(q.store_params(which), c.store_params(which))


# ---------------------------------------------------------------------------------------------------------------- training
def _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, G, N, kappa, arch="qr", w=None, A=2, fc=FC):
    d = lambda x: torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if algo in DOUBLE else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    isw = d(w.astype(np.float32)) if w is not None else None
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=isw, gamma=G, flat_grad=grad)
    loss0, g0, lb, umax = ref_train(p_on, p_tg, s, a, r, s2, t, w, G, algo, N, kappa, dev_astar, arch, A, fc)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_grads(grad.cpu().numpy(), g0, N, arch, A, fc)
    if w is not None:
        np.testing.assert_allclose(ae.cpu().numpy(), lb, rtol=1e-4, atol=1e-6)
    assert torch.equal(net.store_params(), before)              # gradient export leaves the parameters alone
    return umax


CASES = [(algo, B, G) for algo in ("qr", "qrdouble") for B in (1, 32, 255, 256) for G in (GAMMA, GAMMA ** 3)]


@pytest.mark.parametrize("algo,B,G", CASES)
def test_train_step_gradients_match_autograd(torch_cuda, algo, B, G):
    torch = torch_cuda
    net, p_on, p_tg = make_qr(max_batch=256)
    rng = np.random.default_rng(zlib.crc32(f"{algo}-{B}-{G}".encode()))
    s, a, r, s2, t = _batch(rng, B)
    if B >= 255:
        assert t.any() and not t.all()                       # terminal and bootstrapped samples both
    _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, G, 51, 1.0)


@pytest.mark.parametrize("algo", ["qr", "qrdouble"])
def test_gradients_far_past_kappa(torch_cuda, algo):
    """a small kappa and a sharpened head: nearly every |u| is many kappas wide (the linear branch and the clamp)"""
    torch = torch_cuda
    net, p_on, p_tg = make_qr(N=21, kappa=0.05, max_batch=64, head_scale=10.0)
    rng = np.random.default_rng(17)
    s, a, r, s2, t = _batch(rng, 64)
    umax = _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, GAMMA, 21, 0.05)
    assert umax > 100 * 0.05


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ["qr", "qrdouble"])
def test_dueling_gradients_match_autograd(torch_cuda, algo, B):
    torch = torch_cuda
    net, p_on, p_tg = make_qr(arch="qrdueling", max_batch=256)
    rng = np.random.default_rng(B + len(algo))
    s, a, r, s2, t = _batch(rng, B)
    _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, GAMMA ** 3, 51, 1.0, arch="qrdueling")


@pytest.mark.parametrize("arch", ["qr", "qrdueling"])
@pytest.mark.parametrize("algo,base", [("qrper", "qr"), ("qrdoubleper", "qrdouble")])
def test_per_weights(torch_cuda, algo, base, arch):
    """w = 1 gives the uniform algo's loss and gradient bit for bit; random weights match autograd; abs_err = l_b without w"""
    torch = torch_cuda
    net, p_on, p_tg = make_qr(arch=arch, max_batch=256)
    rng = np.random.default_rng(len(algo) + len(arch))
    for B in (32, 256):
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        g1 = torch.zeros(net.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        l1, _, _ = net.train_step(base, s, a, r, s2, t, gamma=GAMMA, flat_grad=g1)
        l1 = l1.clone()
        l2, ae, _ = net.train_step(algo, s, a, r, s2, t, isw=torch.ones(B, device="cuda"), gamma=GAMMA, flat_grad=g2)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)
        assert (ae >= 0).all()
        w = rng.uniform(0.2, 1.0, B)
        s, a, r, s2, t = _batch(rng, B)
        _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, GAMMA, 51, 1.0, arch=arch, w=w)


@pytest.mark.parametrize("arch", ["qr", "qrdueling"])
@pytest.mark.parametrize("B", [32, 256])
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, B, arch):
    torch = torch_cuda
    rng = np.random.default_rng(B)
    n1, _, _ = make_qr(arch=arch, max_batch=256)
    n2, _, _ = make_qr(arch=arch, max_batch=256)
    for n in (n1, n2):
        n.set_hparams(lr=1e-4)
    g = torch.zeros(n1.n_params, dtype=torch.float32, device="cuda")
    for k in range(3):
        algo = "qr" if k % 2 == 0 else "qrdouble"
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        l1, _, _ = n1.train_step(algo, s, a, r, s2, t, gamma=GAMMA)
        l1 = l1.clone()
        l2, _, _ = n2.train_step(algo, s, a, r, s2, t, gamma=GAMMA, flat_grad=g)
        n2.apply_adam(g)
        assert torch.equal(l1, l2)
        assert torch.equal(n1.store_params(), n2.store_params())
    m1, v1, p1 = n1.adam_state()
    m2, v2, p2 = n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)


def test_the_head_is_never_stale(torch_cuda):
    """a dueling QR net after load_params, init_params, a target sync, a fused train step and apply_adam: forward and acting give the
    restatement's Q of the parameters as they now are"""
    torch = torch_cuda
    N = 51
    net, p_on, _ = make_qr(N, arch="qrdueling", max_batch=256)
    net.set_hparams(lr=3e-3)
    rng = np.random.default_rng(7)
    s = rand_states(rng, 64)
    sd = torch.from_numpy(s).cuda()

    def check(which, what):
        with torch.no_grad():
            q0 = ref_theta(net.store_params(which).cpu().numpy(), s, N, "qrdueling").mean(-1).numpy()
        q = net.forward(sd, which).cpu().numpy()
        tol = 1e-4 * max(1.0, np.abs(q0).max())
        np.testing.assert_allclose(q, q0, rtol=0, atol=tol, err_msg=what)
        if which == 0:
            act, qa = net.act(sd, 0.0, want_q=True)
            np.testing.assert_allclose(qa.cpu().numpy(), q0, rtol=0, atol=tol, err_msg=what)
            sure = np.abs(q0[:, 0] - q0[:, 1]) > 10 * tol
            np.testing.assert_array_equal(act.cpu().numpy()[sure], q0.argmax(1)[sure], err_msg=what)
        return q

    q_prev = check(0, "make")
    p2 = p_on.copy()
    p2[HEAD0:] = rng.standard_normal(len(p2) - HEAD0).astype(np.float32) * 0.05
    net.load_params(p2, 0)
    q = check(0, "load_params")
    assert np.abs(q - q_prev).max() > 1e-2
    net.init_params(11, 0)
    check(0, "init_params")
    net.load_params(p2, 0)
    net.sync_target()
    check(1, "sync_target")
    for k in range(2):
        s_, a_, r_, s2_, t_ = (torch.from_numpy(x).cuda() for x in _batch(rng, 32))
        q_prev = net.forward(sd).cpu().numpy()
        if k == 0:
            net.train_step("qr", s_, a_, r_, s2_, t_, gamma=GAMMA)
            q = check(0, "fused train step")
        else:
            g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            net.train_step("qrdouble", s_, a_, r_, s2_, t_, gamma=GAMMA, flat_grad=g)
            net.apply_adam(g)
            q = check(0, "apply_adam")
        assert np.abs(q - q_prev).max() > 1e-4


# ---------------------------------------------------------------------------------------------------------------- ring-fed
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ["qr", "qrdouble"])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, algo, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(256, 20000, 30, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (1, 32, 255):
        n1, _, _ = make_qr(max_batch=256)
        n2, _, _ = make_qr(max_batch=256)
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        pop = rep.population
        for step in range(3):
            idx = torch.from_numpy(rng.integers(0, pop, B)).cuda()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, _, _ = n1.train_step(algo, s, a, r, s2, t, gamma=G, flat_grad=g1 if exp else None, want_aux=False)
            l2, a2, r2, t2 = train_from_replay(rep, n2, algo, idx, gamma=GAMMA, flat_grad=g2 if exp else None)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert torch.equal(l1, l2), (algo, n, B, step)
            if exp:
                assert torch.equal(g1, g2)
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params()), (algo, n, B, step)


@pytest.mark.parametrize("n", [1, 3])
def test_train_steps_equals_separate_calls(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import TrainSteps, train_from_replay
    B = 32

    def make():
        _, rep = played(256, 20000, 14, seed=5)
        rep.seed(9, "cpython"); rep.set_n_step(n, GAMMA)
        net, _, _ = make_qr(arch="qrdueling", max_batch=256)
        net.set_hparams(lr=1e-4)
        return rep, net, TrainSteps(rep, net, B, "qrdouble", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    for _ in range(6):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "qrdouble", idx, gamma=GAMMA)
    ts2(6)
    assert torch.equal(n1.store_params(), n2.store_params())


# ---------------------------------------------------------------------------------------------------------------- the full step
def _pipeline(N, B, n, arch="qr", prioritized=False, seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(N, seed=seed)
    if prioritized:
        rep = per_memory(6 * N + 13, N, n, "exact")
    else:
        rep = VecReplay(max(20000, 16 * N), N)
        rep.set_n_step(n, GAMMA)
        rep.seed(9, "cpython")
    net, _, _ = make_qr(arch=arch, max_batch=max(N, B))
    net.set_hparams(lr=1e-4)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("N", [256, 1024, 4096])
@pytest.mark.parametrize("n", [1, 3])
def test_vec_step_equals_separate_calls(torch_cuda, N, n):
    """fb_vec_step on a QR net == act_nib -> frame_step -> push -> sample -> train_from_replay: actions, indices, loss, parameters"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 24
    algo = "qrdouble" if n == 3 else "qr"
    e1, r1, n1, nib1 = _pipeline(N, B, n)
    e2, r2, n2, nib2 = _pipeline(N, B, n)
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 10 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, _ = r1.sample(B)
            loss, a, r, t = train_from_replay(r1, n1, algo, idx, gamma=GAMMA)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(a, one.a) and torch.equal(r, one.r) and torch.equal(t, one.t), step
    assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all()
    assert n2.split_stats() == (0, 0)                          # the one-stream schedule


@pytest.mark.parametrize("N", [256, 4096])
def test_prioritized_vec_step_equals_separate_calls(torch_cuda, N):
    """fb_vec_step(qrdoubleper on the dueling QR head, 3-step returns) == act -> frame_step -> push -> Memory.sample -> weighted
    train -> batch_update, with the memory's whole state blob at the end"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, n, algo = 32, 3, "qrdoubleper"
    steps = 16 if N == 4096 else 24
    e1, r1, n1, nib1 = _pipeline(N, B, n, "qrdueling", prioritized=True)
    e2, r2, n2, nib2 = _pipeline(N, B, n, "qrdueling", prioritized=True)
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(steps):
        train = step >= n - 1
        if train and step % 5 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
            loss, a_, r_, t_, ae = train_from_replay(r1, n1, algo, idx, gamma=GAMMA, isw=isw, want_abs_err=True)
            r1.update_priorities(idx, abs_err=ae)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(isw, one.isw), step
            assert torch.equal(loss, one.loss) and torch.equal(ae, one.abs_err + 0.01), step
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(n1.store_params(), n2.store_params())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


# ---------------------------------------------------------------------------------------------------------------- acting
def test_acting_is_the_argmax_of_the_mean_and_epsilon_follows_the_plain_rule(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    net, p_on, _ = make_qr(max_batch=400)
    rng = np.random.default_rng(4)
    s = rand_states(rng, 1100)
    with torch.no_grad():
        q = ref_theta(p_on, s, 51).mean(-1).numpy()
    sd = torch.from_numpy(s).cuda()
    plain = QNet(2, FC, "plain", max_batch=400)
    plain.init_params(1)
    tol = 1e-4 * max(1.0, np.abs(q).max())
    for B in (7, 200, 1100):
        act, qd = net.act(sd[:B].contiguous(), 0.0, seed=5, step=9, want_q=True)
        act = act.cpu().numpy()
        sure = np.abs(q[:B, 0] - q[:B, 1]) > 10 * tol
        assert sure.mean() > 0.9
        np.testing.assert_array_equal(act[sure], q[:B].argmax(1)[sure])
        np.testing.assert_array_equal(act, qd.cpu().numpy().argmax(1))
        for eps, seed, step in ((1.0, 5, 9), (1.0, 123, 4567), (0.3, 5, 9)):
            ac = net.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            ap = plain.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            if eps == 1.0:
                np.testing.assert_array_equal(ac, ap)
            else:
                greedy_q = net.act(sd[:B].contiguous(), 0.0).cpu().numpy()
                greedy_p = plain.act(sd[:B].contiguous(), 0.0).cpu().numpy()
                rand_p = plain.act(sd[:B].contiguous(), 1.0, seed=seed, step=step).cpu().numpy()
                took = ap != greedy_p
                np.testing.assert_array_equal(ac[took], rand_p[took])
                assert ((ac == greedy_q) | (ac == rand_p)).all()


# ---------------------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("arch", ["qr", "qrdueling"])
@pytest.mark.parametrize("n,M", [(1027, 1027), (200, 256)])
def test_eval_run_equals_composed_calls(torch_cuda, n, M, arch):
    from dqnflappybird_amd.evaluate import Evaluator
    net, _, _ = make_qr(arch=arch, max_batch=(M + 2) // 3, head_scale=3.0)
    s0, l0, t0, _ = composed_eval(net, M, n, 2, env_seed=11)
    res = Evaluator(n).run(net, n, 2, max_steps=100_000, env_seed=11)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all()


def test_eval_q_equals_act_nib(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecGameState
    net, _, _ = make_qr(max_batch=400)
    N = 1027
    env = VecGameState(N, seed=3)
    nib = env.track_state()
    env.observe()
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(30):
        env.frame_step((torch.rand(N, generator=g) < 0.15).to(torch.uint8).cuda(), want_u8=False)
    states = nib.clone()
    q = torch.empty((N, 2), dtype=torch.float32, device="cuda")
    L.check(L.lib().fb_eval_q(net.h, L.ptr(states), N, L.ptr(q), L.current_stream()), "fb_eval_q")
    _, qa = net.act_nib(states, 0.0, want_q=True)
    assert torch.equal(qa, q)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep, train_from_replay
    N, B = 256, 32
    qr, _, _ = make_qr(max_batch=N)
    c51 = QNet(2, FC, "c51", max_batch=N); c51.init_params(1); c51.init_params(2, which=1)
    plain = QNet(2, FC, "plain", max_batch=N); plain.init_params(1); plain.init_params(2, which=1)
    rng = np.random.default_rng(0)
    s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
    before = [frozen(x) for x in (qr, c51, plain)]
    ones = torch.ones(B, device="cuda")
    for net, algo, msg in ((plain, "qr", "needs a QR net"), (c51, "qrdouble", "C51 net trains with"), (plain, "qrper", "needs a QR net"),
                           (qr, "nature", "QR net trains with"), (qr, "dqn", "QR net trains with"), (qr, "per", "QR net trains with"),
                           (qr, "c51", "needs a C51 net"), (qr, "c51doubleper", "needs a C51 net")):
        with pytest.raises(ValueError, match=msg):
            net.train_step(algo, s, a, r, s2, t, isw=ones, gamma=GAMMA)
    torch.cuda.synchronize()
    assert all(same(frozen(x), b) for x, b in zip((qr, c51, plain), before))
    # memories of the wrong kind, through every training entry point
    env = VecGameState(N, seed=1); env.track_state(); env.observe()
    per = VecReplay(20000, N, prioritized=True); per.reset(env.frame_bits)
    uni = VecReplay(20000, N); uni.reset(env.frame_bits)
    for _ in range(4):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        per.push(env.frame_bits, acts, env.reward, env.terminal)
        uni.push(env.frame_bits, acts, env.reward, env.terminal)
    blob, uni_blob, env_state = per.state_blob().copy(), uni.state_blob().copy(), env.get_state().copy()
    idx0 = torch.zeros(B, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="uniform memory only"):
        train_from_replay(per, qr, "qr", idx0, gamma=GAMMA, isw=ones)
    with pytest.raises(ValueError, match="prioritized memory only"):
        train_from_replay(uni, qr, "qrper", idx0, gamma=GAMMA, isw=ones)
    with pytest.raises(ValueError, match="uniform memory only"):
        VecStep(env, per, qr, B, "qr", GAMMA)
    sb = VecStep(env, uni, qr, B, "qr", GAMMA).buf
    rc = L.lib().fb_vec_step(env.h, per.h, qr.h, ctypes.byref(sb), N, L.ALGO_QR, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "uniform memory only" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, plain.h, ctypes.byref(sb), N, L.ALGO_QR, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "QR" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, qr.h, ctypes.byref(sb), N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, qr.h, ctypes.byref(sb), N, 13, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "unknown algo" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, qr.h, ctypes.byref(sb), N, L.ALGO_QR_PER, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1                                          # (no isw buffers, then the memory's kind)
    rc = L.lib().fb_vec_step_dp(None, env.h, uni.h, qr.h, None, N, L.ALGO_QR, B, 0.0, 0, 0, 1, GAMMA, 1, L.current_stream())
    assert rc == -1 and "data-parallel QR" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_train_steps(uni.h, qr.h, L.ALGO_NATURE, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1 and "QR" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_train_steps(per.h, qr.h, L.ALGO_QR, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1 and "uniform memory only" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_train_steps(uni.h, qr.h, L.ALGO_QR_PER, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1
    # the noisy-net and C51-only calls
    assert L.lib().fb_qnet_set_acting_noise(qr.h, L.ACT_NOISE_PER_ENV) == -1
    nibs = torch.zeros((N, L.NIB_STRIDE), dtype=torch.uint8, device="cuda")
    acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
    assert L.lib().fb_qnet_act_nib_env_noise(qr.h, L.ptr(nibs), N, 0.0, 0, 0, L.ptr(acts), None, L.current_stream()) == -1
    assert L.lib().fb_qnet_reset_noise(qr.h, 0, 0, 0, L.NOISE_SAMPLE, L.current_stream()) == -1
    probs = torch.zeros((B, 2, 51), device="cuda")
    assert L.lib().fb_qnet_forward_dist(qr.h, 0, L.ptr(s), B, L.ptr(probs), L.current_stream()) == -1
    assert L.lib().fb_qnet_forward_quantiles(c51.h, 0, L.ptr(s), B, L.ptr(probs), L.current_stream()) == -1
    assert qr.support is None and c51.quantiles() is None and plain.quantiles() is None
    torch.cuda.synchronize()
    assert (probs == 0).all()
    assert np.array_equal(per.state_blob(), blob) and np.array_equal(uni.state_blob(), uni_blob)
    assert np.array_equal(env.get_state(), env_state)
    assert all(same(frozen(x), b) for x, b in zip((qr, c51, plain), before))


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_vecbrain_checkpoints_and_evaluate(torch_cuda, tmp_path):
    """VecBrain(algo='qrdoubleper', arch='qrdueling'): the target net is synced, save / load continues bit for bit; another N or kappa,
    a C51 brain and a QR brain of the other head refuse the checkpoint, a QR brain refuses a C51 one; evaluate() plays it"""
    torch = torch_cuda
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="qrdoubleper", arch="qrdueling", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4, n_step=3, kappa=2.0)
    a = VecBrain(256, **kw)
    assert a.net.quantiles() == (51, 2.0)
    a.run(20, log_every=0)
    assert not torch.equal(a.net.store_params(0), a.net.store_params(1))
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(10):
        a.step(); ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.loss.clone()))
    b = VecBrain(256, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(10):
        b.step()
        assert torch.equal(b.one_step.actions, ta[i][0]) and torch.equal(b.one_step.idx, ta[i][1]) and torch.equal(b.one_step.loss, ta[i][2]), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0)) and torch.equal(a.net.store_params(1), b.net.store_params(1))
    with pytest.raises(ValueError, match="n_quantiles, kappa"):
        VecBrain(256, **dict(kw, kappa=1.0)).load(ck)
    with pytest.raises(ValueError, match="qrdueling head, this VecBrain has a qr head"):
        VecBrain(256, **dict(kw, arch="qr")).load(ck)
    with pytest.raises(ValueError, match="QR"):
        VecBrain(256, **dict(kw, algo="c51doubleper", arch="c51dueling")).load(ck)
    c51 = VecBrain(256, **dict(kw, algo="c51", arch="plain"))
    c51.save(str(tmp_path / "c51"))
    with pytest.raises(ValueError, match="holds a c51 head"):
        VecBrain(256, **dict(kw, algo="qr", arch="qr")).load(str(tmp_path / "c51"))
    net = qnet_from_checkpoint(ck, max_batch=256)
    assert net.quantiles() == (51, 2.0)
    assert torch.equal(net.store_params(0).cpu(), torch.from_numpy(np.load(ck + ".npz")["online"]))
    res = evaluate(net, 512, episodes=1, env_seed=4)
    c = VecBrain(256, **kw)
    c.load(ck)
    res2 = c.evaluate(512, episodes=1, env_seed=4)
    assert (res.length > 0).all() and np.array_equal(res.score, res2.score) and np.array_equal(res.length, res2.length)
