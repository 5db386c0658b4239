"""Implicit quantile networks on the GPU (include/fbdqn.h: FB_ARCH_IQN; kernels: csrc/fb_iqn.hip) against the float64 restatements of
tests/test_iqn_host.py, under the project's bounds: Q_ATOL (tests/test_gpu_qnet.py) on theta, Qbar and T; rtol 1e-4 / atol 1e-6 on the
loss; per gradient tensor of the IQN layout (W_e and b_e included) elementwise rtol 2e-3 / atol 2e-5 x the tensor's largest reference
element (tests/test_gpu_sac.py::check_sac_grads' bounds) on kink-free inputs.  Then the exact cases and the compositions, bit for bit:
ring-fed == gathered, tau = NULL == iqn_draw_taus == numpy Philox, fused Adam == export + (clip) + apply_adam, fb_iqn_step == its
separate calls; the refusals; the loop and its checkpoint."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import nib_pack
from tests.test_gpu_ac import filled_replay, net_state, same_state
from tests.test_gpu_qnet import Q_ATOL, rand_states, trained_like_params
from tests.test_iqn_host import (E, F32, WORKED, head_parts, iqn_bounds, n_plain, np_draw_taus, pre64, qbar_from_h, tau_grid, theta_from_h,
                                 torch_iqn_loss, trunk64)

pytestmark = pytest.mark.gpu
SHAPES = [(512, 2, 8, 8, 32), (384, 3, 5, 7, 3), (128, 8, 64, 64, 64), (512, 2, 1, 1, 1)]      # (FC, A, N, N', K)
MAXB = 700                                   # rows: 3 x 700 >= 1027
GAMMA = 0.99
TAU_MARGIN = 1e-5                            # |pre_k(tau)| of an accepted tau (the fp32 error of pre is <= 5e-7)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def head0(fc):
    return 77984 + 1600 * fc + fc


_params = {}


def iqn_params(oracle, fc, A, seed=1):
    """trained-like parameters in the IQN layout: the trunk of tests/test_gpu_sac.py's net of that seed (its kink-free pool serves this net
    too), a plain net's head, W_e of scale 0.05 and b_e of scale 0.02 -- near 0, so that both sides of phi's ReLU occur"""
    if (fc, A, seed) not in _params:
        k = np.float32(np.sqrt(512 / fc))
        d = trained_like_params(oracle, oracle.qcfg(fc, A, True), seed)
        head = trained_like_params(oracle, oracle.qcfg(fc, A, False), seed + 10)[head0(fc):] * k
        rng = np.random.default_rng(1000 * fc + 10 * A + seed)
        p = np.concatenate([d[:head0(fc)], head, rng.normal(size=E * fc) * 0.05, rng.normal(size=fc) * 0.02]).astype(np.float32)
        assert len(p) == iqn_bounds(fc, A)[-1][2]
        p.setflags(write=False)
        _params[(fc, A, seed)] = p
    return _params[(fc, A, seed)]


_nets, _refs, _grads = {}, {}, {}


def case(oracle, shape):
    """one net per shape (gradient-exporting steps leave it as it was): online parameters of seed 1, target parameters of seed 2"""
    from dqnflappybird_amd.vec import QNet
    fc, A, N, Np, K = shape
    if shape not in _nets:
        net, p, pt = QNet(A, fc, "iqn", max_batch=MAXB, n_tau=N, n_tau_next=Np, n_tau_act=K), iqn_params(oracle, fc, A, 1), iqn_params(oracle, fc, A, 2)
        assert net.n_params == len(p) and net.iqn() == (N, Np, K, 1.0, 1.0)
        net.load_params(p, 0)
        net.load_params(pt, 1)
        _nets[shape] = (net, p, pt)
    return _nets[shape]


def t64(p):
    import torch
    return torch.from_numpy(np.asarray(p).astype(np.float64))


def h64(p, s, fc, A):
    import torch
    with torch.no_grad():
        return torch.cat([trunk64(t64(p), s[k:k + 256], fc, A) for k in range(0, len(s), 256)])


def forward_ref(oracle, fc, A, n=1027):
    """n random states and their float64 fc1 activations under the online and (the first 256) the target parameters, once per (fc, A)"""
    if (fc, A) not in _refs:
        s = rand_states(np.random.default_rng(7 * fc + A), n)
        _refs[(fc, A)] = (s, h64(iqn_params(oracle, fc, A, 1), s, fc, A), h64(iqn_params(oracle, fc, A, 2), s[:256], fc, A))
    return _refs[(fc, A)]


# ================================================================================================================ forward
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_iqn_against_float64(torch_cuda, oracle, shape):
    torch = torch_cuda
    fc, A, M, _, _ = shape
    net, p, pt = case(oracle, shape)
    s, h_on, h_tg = forward_ref(oracle, fc, A)
    rng = np.random.default_rng(fc + M)
    tau = np.maximum(rng.random((len(s), M)).astype(F32), F32(2.0 ** -24))
    with torch.no_grad():
        pre = pre64(t64(p), tau[:64], fc, A)
        assert (pre > 0).any() and (pre < 0).any()                   # both sides of phi's ReLU occur
        ref_on = torch.cat([theta_from_h(t64(p), h_on[k:k + 128], tau[k:k + 128], fc, A) for k in range(0, len(s), 128)]).numpy()
        ref_tg = theta_from_h(t64(pt), h_tg, tau[:256], fc, A).numpy()
    assert 0.05 < np.abs(ref_on).max() < 100 and (M == 1 or np.abs(ref_on[:, 0] - ref_on[:, -1]).max() > 1e-3)
    sd, td = torch.from_numpy(s).cuda(), torch.from_numpy(tau).cuda()
    for B in (1, 255, 1027):
        got = net.forward_iqn(sd[:B].contiguous(), td[:B].contiguous(), 0)
        assert got.shape == (B, M, A)
        err = np.abs(got.cpu().numpy() - ref_on[:B]).max()
        print(f"forward_iqn {shape} B={B}: max |d theta| {err:.3e}")
        assert err <= Q_ATOL
    got = net.forward_iqn(sd[:255].contiguous(), td[:255].contiguous(), 1)
    np.testing.assert_allclose(got.cpu().numpy(), ref_tg[:255], rtol=0, atol=Q_ATOL)
    assert net.overflow_count() == 0


def eval_q(torch, net, nib):
    from dqnflappybird_amd import _lib as L
    q = torch.empty((nib.shape[0], net.A), dtype=torch.float32, device="cuda")
    L.check(L.lib().fb_eval_q(net.h, L.ptr(nib), nib.shape[0], L.ptr(q), L.current_stream()), "fb_eval_q")
    return q


@pytest.mark.parametrize("K", [1, 32, 64])
def test_qbar_through_every_forward_only_path_and_never_stale(torch_cuda, oracle, K):
    """Qbar of forward / act / act_nib / fb_eval_q, both nets, == the mean of float64 theta over the acting grid, at eta = 1 and 0.25,
    and again after everything that changes the parameters or eta"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    net = QNet(A, fc, "iqn", max_batch=128, n_tau=4, n_tau_next=4, n_tau_act=K)
    net.set_hparams(lr=1e-3)
    net.load_params(iqn_params(oracle, fc, A, 1), 0)
    net.load_params(iqn_params(oracle, fc, A, 2), 1)
    s = rand_states(np.random.default_rng(K), 300)
    sd, nib = torch.from_numpy(s).cuda(), torch.from_numpy(nib_pack(s)).cuda()
    eta = [1.0]

    def check(what):
        worst = 0.0
        for which in (0, 1):
            p = net.store_params(which).cpu().numpy()
            with torch.no_grad():
                want = qbar_from_h(t64(p), h64(p, s, fc, A), K, eta[0], fc, A).numpy()
            assert np.abs(want).max() > 0.05
            for n in (5, 300):                                       # the small-batch and the large-batch forward
                q = net.forward(sd[:n].contiguous(), which)
                worst = max(worst, np.abs(q.cpu().numpy() - want[:n]).max())
                if which == 0:
                    a1, q1 = net.act(sd[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)
                    a2, q2 = net.act_nib(nib[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)
                    q3 = eval_q(torch, net, nib[:n].contiguous())
                    for qq in (q1, q2, q3):
                        worst = max(worst, np.abs(qq.cpu().numpy() - want[:n]).max())
                    assert torch.equal(q1, q) and np.array_equal(a1.cpu().numpy(), q1.cpu().numpy().argmax(1))      # the first maximum
                    assert np.array_equal(a2.cpu().numpy(), q2.cpu().numpy().argmax(1))
        print(f"Qbar K={K} eta={eta[0]} after {what}: max |dQ| {worst:.3e}")
        assert worst <= Q_ATOL, what

    check("load_params")
    rng = np.random.default_rng(5)
    B = 16
    st = lambda: torch.from_numpy(rand_states(rng, B)).cuda()
    a = torch.from_numpy(rng.integers(0, A, B).astype(np.uint8)).cuda()
    r = torch.from_numpy(rng.choice(np.array([0.1, 3, -3], F32), B)).cuda()
    t = torch.from_numpy((rng.random(B) < 0.3).astype(np.uint8)).cuda()
    before = net.store_params(0).clone()
    net.iqn_train_step(st(), a, r, st(), t, gamma=GAMMA, seed=3, step=0)
    assert not torch.equal(net.store_params(0), before)
    check("a fused train step")
    g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    net.iqn_train_step(st(), a, r, st(), t, gamma=GAMMA, seed=3, step=1, flat_grad=g)
    net.apply_adam(g)
    check("export + apply_adam")
    net.set_iqn_risk(0.25)
    eta[0] = 0.25
    assert net.iqn()[4] == 0.25
    check("set_iqn_risk")
    net.soft_sync_target(0.3)
    check("soft_sync_target")
    net.sync_target()
    assert torch.equal(net.store_params(0), net.store_params(1))
    check("sync_target")
    net.init_params(seed=9, which=0)
    pe = net.store_params(0).cpu().numpy()
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    assert (pe[b["b_e"][0]:b["b_e"][1]] == 1).all() and (pe[b["b_q"][0]:b["b_q"][1]] == F32(0.01)).all()
    net.load_params(iqn_params(oracle, fc, A, 2), 0)
    check("init_params + load_params")


def test_init_params_are_the_plain_nets_and_a_fresh_net_starts_as_it(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    iqn, plain = QNet(A, fc, "iqn", max_batch=8), QNet(A, fc, "plain", max_batch=8)
    iqn.init_params(seed=11); plain.init_params(seed=11)
    pi, pp = iqn.store_params().cpu().numpy(), plain.store_params().cpu().numpy()
    assert np.array_equal(pi[:len(pp)], pp) and len(pp) == n_plain(fc, A)          # trunk, fc1 and W_q b_q: the plain net's bits
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    we = pi[b["W_e"][0]:b["W_e"][1]]
    assert np.abs(we).max() <= 0.02 + 1e-9 and 0.005 < we.std() < 0.012 and (pi[b["b_e"][0]:b["b_e"][1]] == 1).all()
    assert iqn.iqn() == (8, 8, 32, 1.0, 1.0)
    s = torch.from_numpy(rand_states(np.random.default_rng(2), 6)).cuda()
    qi, qp = iqn.forward(s).cpu().numpy(), plain.forward(s).cpu().numpy()
    print(f"a fresh IQN net against the plain net of its seed: max |Qbar - Q| {np.abs(qi - qp).max():.3e} at max |Q - b_q| {np.abs(qp - 0.01).max():.3e}")


# ================================================================================================================ exact cases
def with_blocks(p, fc, A, **blocks):
    p = np.array(p)
    for n, lo, hi in iqn_bounds(fc, A):
        if n in blocks:
            p[lo:hi] = blocks[n]
    return p


@pytest.mark.parametrize("fc,A", [(512, 2), (384, 3), (128, 8)])
def test_exact_embeddings(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    p = iqn_params(oracle, fc, A)
    net, plain = QNet(A, fc, "iqn", max_batch=64, n_tau_act=7), QNet(A, fc, "plain", max_batch=64)
    plain.load_params(p[:n_plain(fc, A)])
    s = torch.from_numpy(rand_states(np.random.default_rng(fc), 40)).cuda()
    tau = torch.from_numpy(np.maximum(np.random.default_rng(A).random((40, 6)).astype(F32), F32(1e-6))).cuda()
    q = plain.forward(s)
    # W_e = 0, b_e = 1: phi = 1, theta(tau) and Qbar are the plain net's Q
    net.load_params(with_blocks(p, fc, A, W_e=0, b_e=1))
    th, qb = net.forward_iqn(s, tau), net.forward(s)
    print(f"W_e = 0, b_e = 1 ({fc}, {A}): Qbar bit-identical to the plain net's Q: {torch.equal(qb, q)}; theta: {torch.equal(th[:, 0], q)}; "
          f"max |dQbar| {(qb - q).abs().max().item():.3e}, max |dtheta| {(th - q[:, None, :]).abs().max().item():.3e}")
    assert (qb - q).abs().max().item() <= Q_ATOL and (th - q[:, None, :]).abs().max().item() <= Q_ATOL
    # W_e one-hot in row j0, b_e = 0: theta(tau) - b_q = relu(cos(pi j0 tau)) (plain Q - b_q): the cosine convention
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    bq = p[b["b_q"][0]:b["b_q"][1]].astype(np.float64)
    for j0 in (0, 1, 5, 63):
        we = np.zeros((E, fc), F32)
        we[j0] = 1
        net.load_params(with_blocks(p, fc, A, W_e=we.ravel(), b_e=0))
        th = net.forward_iqn(s, tau).cpu().numpy()
        c = np.maximum(np.cos(np.pi * j0 * tau.cpu().numpy().astype(np.float64)), 0)
        want = c[:, :, None] * (q.cpu().numpy().astype(np.float64) - bq)[:, None, :] + bq
        assert (c > 0.1).any() and (j0 == 0 or (c == 0).any())
        np.testing.assert_allclose(th, want, rtol=0, atol=2 * Q_ATOL, err_msg=f"j0={j0}")      # (the plain Q's own Q_ATOL, then theta's)


@pytest.mark.parametrize("kappa,tau,theta,T,l,g", WORKED)
def test_worked_cases_on_the_kernel(torch_cuda, oracle, kappa, tau, theta, T, l, g):
    """with a zero W_q and chosen biases: theta = b_q exactly, for every tau, so a sample holds ONE pair (theta_i, T_j) -- N = N' = 1, theta_i
    the online net's bias, T_j = r + 1.0 * the target net's bias -- and the pairs of a worked case are recombined on the host:
    l = (1 / N') sum_i sum_j l_ij, dl/dtheta_i = (1 / N') sum_j g_ij.  fp32 arithmetic on exact inputs: 1e-6"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 2
    N, Np = len(theta), len(T)
    p = iqn_params(oracle, fc, A)
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    s = torch.from_numpy(rand_states(np.random.default_rng(1), 1)).cuda()
    net = QNet(A, fc, "iqn", max_batch=4, n_tau=1, n_tau_next=1, n_tau_act=1, kappa=kappa)
    tot, grads = 0.0, []
    for i in range(N):
        lj = []
        for j in range(Np):
            net.load_params(with_blocks(p, fc, A, W_q=0, b_q=[theta[i], -50.0]), 0)
            net.load_params(with_blocks(p, fc, A, W_q=0, b_q=[T[j] - 0.5, -50.0]), 1)
            gr = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            loss, y = net.iqn_train_step(s, torch.zeros(1, dtype=torch.uint8, device="cuda"), torch.full((1,), 0.5, device="cuda"), s,
                                         torch.zeros(1, dtype=torch.uint8, device="cuda"), gamma=1.0,
                                         tau=torch.tensor([[tau[i]]], dtype=torch.float32, device="cuda"),
                                         tau_next=torch.tensor([[0.5]], dtype=torch.float32, device="cuda"), flat_grad=gr)
            assert abs(y.item() - T[j]) < 1e-6
            lj.append((loss.item(), gr[b["b_q"][0]].item(), gr[b["b_q"][0] + 1].item()))
        tot += sum(x[0] for x in lj) / Np
        grads.append(sum(x[1] for x in lj) / Np)
        assert all(x[2] == 0 for x in lj)                            # the other action's bias gets no gradient
    print(f"worked case kappa={kappa}: l {tot!r} (want {l}), dl/dtheta {grads} (want {g})")
    assert abs(tot - l) < 1e-6
    np.testing.assert_allclose(grads, g, rtol=0, atol=1e-6)


def test_worked_cases_whole_on_the_kernel(torch_cuda, oracle):
    """both worked cases as ONE sample each, through the kernel's own pairwise loop: one live fc1 unit k0, W_e one-hot at (1, k0) and
    b_e = 0, so theta(tau) = b_q + h_k0 W_q[k0, 0] relu(cos(pi tau)).  Online: the worked tau_i are given, and the two unknowns (b_q,
    W_q[k0, 0]) solve theta_1, theta_2.  Target: tau'_j = acos(x_j) / pi puts theta_tgt(tau'_j) on T_j - r (gamma = 1).  theta and T
    then hold to Q_ATOL, and the loss and b_q's gradient to what that leaves (below)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 2
    p = iqn_params(oracle, fc, A)
    b = {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    s_np = rand_states(np.random.default_rng(1), 1)
    s = torch.from_numpy(s_np).cuda()
    h = h64(p, s_np, fc, A)[0].numpy()
    k0 = int(np.argmax(h))                                           # one live fc1 unit carries everything
    assert h[k0] > 0.1
    for kappa, tau, theta, T, l, g in WORKED:
        N, Np = len(theta), len(T)
        # online: theta_i = b + S relu(cos(pi tau_i)) with S = h_k0 W_q[k0, 0]; the worked tau_i are given, so solve (b, S) for N = 2
        c = np.maximum(np.cos(np.pi * np.asarray(tau, np.float64)), 0)
        S = (theta[0] - theta[1]) / (c[0] - c[1])
        bb = theta[0] - S * c[0]
        we = np.zeros((E, fc), F32)
        we[1, k0] = 1
        wq = np.zeros((fc, A), F32)
        wq[k0, 0] = S / h[k0]
        net = QNet(A, fc, "iqn", max_batch=4, n_tau=N, n_tau_next=Np, n_tau_act=1, kappa=kappa)
        net.load_params(with_blocks(p, fc, A, W_q=wq.ravel(), b_q=[bb, -50.0], W_e=we.ravel(), b_e=0), 0)
        # target: theta_tgt(tau'_j) = lo + span relu(cos(pi tau'_j)) = T_j - r with r = 0.5, gamma = 1
        y = np.asarray(T, np.float64) - 0.5
        lo_, span = y.min() - 0.25, (y.max() - y.min()) + 0.5
        x = (y - lo_) / span
        taup = (np.arccos(x) / np.pi).astype(F32)
        wq2 = np.zeros((fc, A), F32)
        wq2[k0, 0] = span / h[k0]
        net.load_params(with_blocks(p, fc, A, W_q=wq2.ravel(), b_q=[lo_, -50.0], W_e=we.ravel(), b_e=0), 1)
        gr = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        z1 = torch.zeros(1, dtype=torch.uint8, device="cuda")
        loss, yT = net.iqn_train_step(s, z1, torch.full((1,), 0.5, device="cuda"), s, z1, gamma=1.0,
                                      tau=torch.tensor([tau], dtype=torch.float32, device="cuda"),
                                      tau_next=torch.from_numpy(taup[None]).cuda(), flat_grad=gr)
        th = net.forward_iqn(s, torch.tensor([tau], dtype=torch.float32, device="cuda"))[0, :, 0].cpu().numpy()
        print(f"worked case kappa={kappa}: theta {th.tolist()} T {yT[0].tolist()} loss {loss.item()!r} (want {l}) db_q {gr[b['b_q'][0]].item()!r} (want {sum(g)})")
        np.testing.assert_allclose(th, theta, rtol=0, atol=Q_ATOL)
        np.testing.assert_allclose(yT[0].cpu().numpy(), T, rtol=0, atol=Q_ATOL)
        # a pair's u moves by at most 2 Q_ATOL (theta_i and T_j); its loss term w L / kappa has slope <= 1 in u and its gradient term
        # w clamp(u) / kappa slope <= 1 / kappa (no worked u is 0, where w jumps); both are (1 / N') sums over N N' pairs
        assert abs(loss.item() - l) <= 2 * N * Q_ATOL
        assert abs(gr[b["b_q"][0]].item() - sum(g)) <= 2 * N * Q_ATOL / kappa


# ================================================================================================================ train step
def ref_step(oracle, shape, B):
    """kink-free inputs and the float64 loss, targets and gradient of the step, for double_q = 0 and 1"""
    import torch
    fc, A, N, Np, K = shape
    if (shape, B) not in _grads:
        p, ptg = iqn_params(oracle, fc, A, 1), iqn_params(oracle, fc, A, 2)
        pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
        s = np.array(pool[:B])
        rng = np.random.default_rng(1000 * fc + 10 * A + B + N)
        a = rng.integers(0, A, B).astype(np.uint8)
        r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.6, 0.2, 0.2])
        t = (rng.random(B) < 0.25).astype(np.uint8)
        if B > 1:
            t[0], t[1] = 1, 0
        P, PT = t64(p), t64(ptg)
        # s': replace a state whose float64 top-two Qbar gap (either net: both choose a* in one of the two modes) is below 10 Q_ATOL
        s2 = rand_states(rng, B)
        for _ in range(20):
            with torch.no_grad():
                h2o, h2t = trunk64(P, s2, fc, A), trunk64(PT, s2, fc, A)
                qo, qt = qbar_from_h(P, h2o, K, 1.0, fc, A), qbar_from_h(PT, h2t, K, 1.0, fc, A)
            top = lambda q: (lambda v: (v[:, 0] - v[:, 1]).numpy())(q.topk(2, 1).values)
            bad = (top(qo) < 10 * Q_ATOL) | (top(qt) < 10 * Q_ATOL)
            if not bad.any():
                break
            s2[bad] = rand_states(rng, int(bad.sum()))
        assert not bad.any()
        # tau: each redrawn alone while any |pre_k(tau)| < TAU_MARGIN under the online parameters; tau' needs no margin
        tau, drawn = np.empty((B, N), F32), 0
        with torch.no_grad():
            for bi in range(B):
                for i in range(N):
                    while True:
                        x = max(F32(rng.random()), F32(2.0 ** -24))
                        drawn += 1
                        if pre64(P, np.array([x]), fc, A).abs().min().item() >= TAU_MARGIN:
                            break
                    tau[bi, i] = x
        print(f"tau draws {shape} B={B}: accepted {B * N} of {drawn}")
        assert B * N >= 0.8 * drawn
        taup = np.maximum(rng.random((B, Np)).astype(F32), F32(2.0 ** -24))
        rd = torch.as_tensor(np.where(r == F32(0.1), 0.1, r.astype(np.float64)))
        nd = torch.as_tensor((t == 0).astype(np.float64))
        ar = torch.arange(B)
        out = {}
        pg = t64(p).requires_grad_(True)
        th = theta_from_h(pg, trunk64(pg, s, fc, A), tau, fc, A)[ar, :, torch.as_tensor(a.astype(np.int64))]
        for dq, qsel in ((0, qt), (1, qo)):
            astar = qsel.argmax(1)
            with torch.no_grad():
                T = rd[:, None] + nd[:, None] * GAMMA * theta_from_h(PT, h2t, taup, fc, A)[ar, :, astar]
            loss, _ = torch_iqn_loss(th, T, tau, 1.0)
            grad, = torch.autograd.grad(loss, pg, retain_graph=dq == 0)
            u = (T[:, None, :] - th.detach()[:, :, None]).numpy()
            if B >= 32:                                              # what the issue asks of the case
                assert (u > 0).any() and (u < 0).any() and (np.abs(u) < 1.0).any() and (np.abs(u) > 1.0).any() and t.any() and not t.all()
            out[dq] = (loss.item(), T.numpy(), grad.numpy())
        _grads[(shape, B)] = (s, a, r, s2, t, tau, taup, out)
    return _grads[(shape, B)]


def check_iqn_grads(g, g0, fc, A):
    """tests/test_gpu_sac.py::check_sac_grads' bounds over the IQN layout, every tensor elementwise (kink-free), W_e and b_e included"""
    for name, lo, hi in iqn_bounds(fc, A):
        ref, got = g0[lo:hi], g[lo:hi]
        scale = np.abs(ref).max()
        assert scale > 0, name
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=name)


@pytest.mark.parametrize("double_q", [0, 1])
@pytest.mark.parametrize("B", [1, 32, 255, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_train_step_against_autograd(torch_cuda, oracle, shape, B, double_q):
    """gathered, gradient-exporting: the loss, the targets and every gradient tensor; nothing is masked"""
    torch = torch_cuda
    fc, A, N, Np, K = shape
    net, p, ptg = case(oracle, shape)
    s, a, r, s2, t, tau, taup, out = ref_step(oracle, shape, B)
    want, T0, g0 = out[double_q]
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, T = net.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, double_q=bool(double_q), tau=d(tau), tau_next=d(taup), flat_grad=grad)
    loss, T = loss.item(), T.cpu().numpy()
    print(f"iqn {shape} B={B} double_q={double_q}: loss {loss!r} / {want!r}; max |dT| {np.abs(T - T0).max():.3e}")
    np.testing.assert_allclose(T, T0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
    check_iqn_grads(grad.cpu().numpy(), g0, fc, A)
    assert np.array_equal(net.store_params(0).cpu().numpy(), p) and np.array_equal(net.store_params(1).cpu().numpy(), ptg)      # gradient-only mode
    assert net.overflow_count() == 0


def test_an_action_past_the_head_reads_the_last_one(torch_cuda, oracle):
    torch = torch_cuda
    shape = SHAPES[1]
    net, p, ptg = case(oracle, shape)
    s, a, r, s2, t, tau, taup, _ = ref_step(oracle, shape, 32)
    d = lambda x: torch.from_numpy(x).cuda()
    g1, g2 = (torch.zeros(net.n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    a1, a2 = a.copy(), a.copy()
    a1[3], a2[3] = shape[1] - 1, 200
    l1, _ = net.iqn_train_step(d(s), d(a1), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g1)
    l2, _ = net.iqn_train_step(d(s), d(a2), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g2)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ================================================================================================================ compositions
def ring_pair(torch, oracle, B, n_nets, n_step=1, lr=1e-4):
    """B transitions of a played memory as ring positions and as gathered tensors, n_nets equal IQN nets (online / target differ)"""
    from dqnflappybird_amd.vec import QNet
    fc, A = 512, 2
    p, ptg = iqn_params(oracle, fc, A, 1), iqn_params(oracle, fc, A, 2)
    N, pushes = 64, 9
    env, rep, pushed = filled_replay(torch, N, pushes)
    if n_step > 1:
        rep.set_n_step(n_step, GAMMA)
    rng = np.random.default_rng(B)
    idx = torch.from_numpy(rng.permutation(N * (pushes - n_step))[:B].astype(np.int64)).cuda()
    s, a, r, s2, t = rep.gather(idx)
    nets = []
    for _ in range(n_nets):
        n = QNet(A, fc, "iqn", max_batch=256)
        n.load_params(p, 0); n.load_params(ptg, 1)
        n.set_hparams(lr=lr)
        nets.append(n)
    return rep, idx, (s, a, r, s2, t), nets, p


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B, n_step):
    """loss, targets, a / r / t and the exported gradient of fb_iqn_train_from_replay == those of fb_replay_gather +
    fb_qnet_iqn_train_step (given the bootstrap's discount, gamma^n), bit for bit"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2, n_step)
    g_gath, g_ring = (torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l_gath, y_gath = nets[0].iqn_train_step(s, a, r, s2, t, gamma=bootstrap_gamma(GAMMA, n_step), double_q=True, seed=5, step=6, flat_grad=g_gath)
    l_ring, a_o, r_o, t_o, y_ring = iqn_train_from_replay(rep, nets[1], idx, gamma=GAMMA, double_q=True, seed=5, step=6, flat_grad=g_ring,
                                                          want_target=True)
    assert torch.equal(a_o, a) and torch.equal(r_o, r) and torch.equal(t_o, t) and g_gath.abs().max() > 0
    print(f"ring-fed vs gathered B={B} n_step={n_step}: loss {l_gath.item()!r} / {l_ring.item()!r}, "
          f"{int((g_ring != g_gath).sum())} of {g_gath.numel()} gradient elements differ")
    assert torch.equal(l_ring, l_gath) and torch.equal(y_ring, y_gath) and torch.equal(g_ring, g_gath)
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p)    # the exporting ring-fed step left its net alone


def test_null_tau_is_the_documented_draw(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd.vec import iqn_draw_taus
    seed, step = (7 << 32) | 11, (1 << 32) | 5
    for which in (0, 1):
        for batch, n in ((1, 1), (33, 8), (256, 64)):
            got = iqn_draw_taus(batch, n, seed, step, which).cpu().numpy()
            want = np_draw_taus(min(batch, 40), n, seed, step, which)
            assert np.array_equal(got[:len(want)], want) and ((got > 0) & (got < 1)).all(), (which, batch, n)
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, 32, 1)
    net = nets[0]
    N, Np = net.iqn()[:2]
    g0, g1 = (torch.zeros(net.n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l0, y0 = net.iqn_train_step(s, a, r, s2, t, gamma=GAMMA, seed=seed, step=step, flat_grad=g0)
    l1, y1 = net.iqn_train_step(s, a, r, s2, t, gamma=GAMMA, tau=iqn_draw_taus(32, N, seed, step, 0), tau_next=iqn_draw_taus(32, Np, seed, step, 1),
                                seed=1, step=2, flat_grad=g1)
    assert torch.equal(l0, l1) and torch.equal(y0, y1) and torch.equal(g0, g1)
    l2, _ = net.iqn_train_step(s, a, r, s2, t, gamma=GAMMA, seed=seed, step=step + 1, flat_grad=g1)
    assert not torch.equal(l0, l2)                                   # another step: other tau


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("B,ring", [(32, False), (32, True), (256, True)])
def test_fused_adam_equals_export_plus_apply_adam(torch_cuda, oracle, B, ring, clip):
    """parameters, both Adam slots and the beta powers; clip > 0: the fused step of a net with a norm limit == export + clip_grad + apply_adam"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import iqn_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2)
    for n in nets:
        n.set_max_grad_norm(clip)
    g = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    kw = dict(gamma=GAMMA, seed=3, step=4)
    l0 = iqn_train_from_replay(rep, nets[0], idx, flat_grad=g, **kw)[0] if ring else nets[0].iqn_train_step(s, a, r, s2, t, flat_grad=g, **kw)[0]
    if clip:
        nets[0].clip_grad(g)
        assert nets[0].grad_norm()[1] < 1.0                          # the limit bites
    nets[0].apply_adam(g)
    l1 = iqn_train_from_replay(rep, nets[1], idx, **kw)[0] if ring else nets[1].iqn_train_step(s, a, r, s2, t, **kw)[0]
    st = [net_state(n) for n in nets]
    assert torch.equal(l0, l1) and same_state(torch, st[0], st[1])
    assert not torch.equal(st[0][0], torch.from_numpy(p).cuda())
    x = torch.from_numpy(rand_states(np.random.default_rng(0), 8)).cuda()
    assert torch.equal(nets[0].forward(x), nets[1].forward(x))        # ... and the folds behind both


@pytest.mark.parametrize("N,batch", [(8, 8), (300, 32)])
def test_iqn_step_equals_its_separate_calls(torch_cuda, oracle, N, batch):
    """8 mixed steps: actions, the loss, both nets, Adam, the envs, the memory"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnStep, QNet, VecGameState, VecReplay, iqn_train_from_replay
    seed = (3 << 32) | 9
    p = iqn_params(oracle, 512, 2)

    def make():
        env, rep, net = VecGameState(N, seed=5), VecReplay(4000, N), QNet(2, 512, "iqn", max_batch=max(N, batch))
        net.load_params(p, 0); net.load_params(iqn_params(oracle, 512, 2, 2), 1)
        net.set_hparams(lr=1e-4)
        rep.seed(7, "cpython")
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = make()
    e2, r2, n2, nib2 = make()
    steps = {dq: IqnStep(e1, r1, n1, batch, GAMMA, dq) for dq in (False, True)}
    drawn = set()
    for k, (train, dq, eps) in enumerate([(False, False, 0.5), (False, True, 0.0), (True, False, 0.5), (True, True, 0.1), (True, True, 0.0),
                                          (False, False, 1.0), (True, False, 0.3), (True, True, 0.5)]):
        one = steps[dq]
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = n2.act_nib(nib2, eps, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        idx = r2.push_sample(e2.frame_bits, a2, rew, term, batch)
        assert torch.equal(a1, a2) and torch.equal(one.idx, idx) and torch.equal(nib1, nib2), k
        if train:
            loss, a_o, r_o, t_o = iqn_train_from_replay(r2, n2, idx, gamma=GAMMA, double_q=dq, seed=seed, step=k)
            assert torch.equal(one.loss, loss) and torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
        assert same_state(torch, net_state(n1), net_state(n2)), k
        drawn |= set(a1.cpu().tolist())
    assert N < 300 or drawn == {0, 1}
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob())) and len(r1) == 8 * N
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), p)


# ================================================================================================================ refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import (ALGOS, AcRolloutStep, IqnStep, QNet, SacStep, TrainSteps, VecReplay, VecStep, ac_train_from_replay,
                                       iqn_train_from_replay, ppo_train_from_replay, sac_train_from_replay, train_from_replay)
    lib = L.lib()
    N, B = 16, 8
    iqn = QNet(2, 128, "iqn", max_batch=32)
    iqn.load_params(iqn_params(oracle, 128, 2), 0)
    env, rep, pushed = filled_replay(torch, N, 12, cap=2000)
    env.track_state()
    rep.seed(9, "cpython")
    blob, before, envs = np.asarray(rep.state_blob()).copy(), net_state(iqn), env.get_state().copy()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    s, a, r, s2, t = rep.gather(idx)
    untouched = lambda: (np.array_equal(np.asarray(rep.state_blob()), blob) and same_state(torch, net_state(iqn), before)
                         and np.array_equal(env.get_state(), envs))
    assert "iqn" not in ALGOS
    for algo in sorted(ALGOS):                                         # every FB_ALGO_* training entry point
        with pytest.raises(ValueError, match="fb_qnet_train_step: an IQN net trains through"):
            iqn.train_step(algo, s, a, r, s2, t, isw=r)
        with pytest.raises(ValueError, match="fb_train_from_replay: an IQN net"):
            train_from_replay(rep, iqn, algo, idx, isw=r)
    for algo in ("dqn", "double", "mdqn"):
        with pytest.raises(ValueError, match="fb_train_steps: an IQN net"):
            TrainSteps(rep, iqn, B, algo)(1)
        for train in (True, False):
            with pytest.raises(ValueError, match="fb_vec_step: an IQN net"):
                VecStep(env, rep, iqn, B, algo)(0.1, train=train)
    buf = VecStep(env, rep, iqn, B, "dqn").buf
    assert lib.fb_vec_step_dp(None, env.h, rep.h, iqn.h, C.byref(buf), N, 0, B, 0.1, 0, 0, 1, 0.99, 0, None) == -1
    assert "data-parallel IQN is not supported" in lib.fb_last_error().decode()
    adv = torch.zeros(B, dtype=torch.float32, device="cuda")
    for call, msg in ((lambda: iqn.set_huber(1.0), "fb_qnet_set_huber"), (lambda: iqn.huber(), "fb_qnet_get_huber"),
                      (lambda: iqn.set_munchausen(), "fb_qnet_set_munchausen"), (lambda: iqn.munchausen(), "fb_qnet_get_munchausen"),
                      (lambda: iqn.set_train_dtype("bf16"), "an IQN net trains in FB_DTYPE_F32 only"),
                      (lambda: iqn.set_inference_dtype("bf16"), "an IQN net computes in FB_DTYPE_F32 only"),
                      (lambda: iqn.set_ac(), "needs an actor-critic net"), (lambda: iqn.set_ppo(), "needs an actor-critic net"),
                      (lambda: iqn.forward_ac(s), "needs an actor-critic net"), (lambda: iqn.ac_train_step(s, a, adv, adv), "needs an actor-critic net"),
                      (lambda: ac_train_from_replay(rep, iqn, idx, adv, adv), "needs an actor-critic net"),
                      (lambda: ppo_train_from_replay(rep, iqn, idx, adv, adv, adv, adv), "needs an actor-critic net"),
                      (lambda: AcRolloutStep(env, rep, iqn, 5), "needs an actor-critic net"),
                      (lambda: iqn.set_sac(), "needs a SAC net"), (lambda: iqn.forward_sac(s), "needs a SAC net"),
                      (lambda: iqn.sac_train_step(s, a, r, s2, t), "needs a SAC net"), (lambda: sac_train_from_replay(rep, iqn, idx), "needs a SAC net"),
                      (lambda: SacStep(env, rep, iqn, B), "needs a SAC net"), (lambda: iqn.reset_noise(), "noisy"),
                      (lambda: QNet(2, 128, "iqn", noisy=True), "noisy layers are offered on the C51 heads only")):
        with pytest.raises(ValueError, match=msg):
            call()
    loss = torch.zeros(6, dtype=torch.float32, device="cuda")
    a_out = torch.zeros(B, dtype=torch.uint8, device="cuda")
    val = torch.zeros(max(N, 64) * 64, dtype=torch.float32, device="cuda")
    r32 = torch.zeros(B, dtype=torch.float32, device="cuda")
    fails = lambda rc, word: rc == -1 and word in lib.fb_last_error().decode()
    assert fails(lib.fb_qnet_forward_ac(iqn.h, L.ptr(s), B, L.ptr(loss), L.ptr(val), None), "not an actor-critic net")
    assert fails(lib.fb_qnet_act_policy_nib(iqn.h, L.ptr(env.nib), N, 0, 0, 0, L.ptr(a_out), L.ptr(val), None, None, None), "not an actor-critic or SAC net")
    assert fails(lib.fb_qnet_forward_sac(iqn.h, 0, L.ptr(s), B, L.ptr(val), L.ptr(val), L.ptr(val), None), "not a SAC net")
    assert fails(lib.fb_qnet_sac_train_step(iqn.h, B, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), 0.99, L.ptr(loss), None, None, None), "not a SAC net")
    assert fails(lib.fb_qnet_forward_dist(iqn.h, 0, L.ptr(s), B, L.ptr(val), None), "not a C51 net")
    assert fails(lib.fb_qnet_forward_quantiles(iqn.h, 0, L.ptr(s), B, L.ptr(val), None), "not a QR net")
    assert fails(lib.fb_qnet_reset_noise(iqn.h, 0, 0, 0, 0, None), "not a noisy net")
    h = C.c_void_p()
    assert fails(lib.fb_qnet_create(L.ARCH_IQN, 128, 2, 32, C.byref(h)), "fb_qnet_create_iqn")
    assert lib.fb_qnet_create_c51_noisy(L.ARCH_IQN, 128, 2, 51, C.c_float(-10), C.c_float(10), C.c_float(0.5), 32, C.byref(h)) == -1
    for bad, word in (((128, 1, 8, 8, 32, 1.0), "n_actions must be in 2..8"), ((128, 9, 8, 8, 32, 1.0), "n_actions must be in 2..8"),
                      ((128, 2, 0, 8, 32, 1.0), "n_tau=0"), ((128, 2, 65, 8, 32, 1.0), "n_tau=65"), ((128, 2, 8, 0, 32, 1.0), "n_tau_next=0"),
                      ((128, 2, 8, 65, 32, 1.0), "n_tau_next=65"), ((128, 2, 8, 8, 0, 1.0), "n_tau_act=0"), ((128, 2, 8, 8, 65, 1.0), "n_tau_act=65"),
                      ((128, 2, 8, 8, 32, 0.0), "kappa must be finite and > 0"), ((128, 2, 8, 8, 32, float("nan")), "kappa must be"),
                      ((100, 2, 8, 8, 32, 1.0), "fc_width must be a multiple of 128")):
        assert fails(lib.fb_qnet_create_iqn(*bad[:5], C.c_float(bad[5]), 32, C.byref(h)), word), bad
    for eta in (0.0, 1.5, float("nan")):
        assert fails(lib.fb_qnet_set_iqn_risk(iqn.h, C.c_float(eta)), "eta must be in (0, 1]")
        with pytest.raises(ValueError, match="eta"):
            iqn.set_iqn_risk(eta)
    # the training calls' own limits
    ts = lambda net, Bn, dq, g: lib.fb_qnet_iqn_train_step(net.h, dq, Bn, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), None, None, 0, 0, g,
                                                           L.ptr(loss), None, None, None)
    assert fails(ts(iqn, 33, 0, 0.99), "exceeds min(max_batch, 256)") and ts(iqn, 0, 0, 0.99) == -1
    assert fails(ts(iqn, B, 0, 1.5), "gamma must be in [0, 1]") and fails(ts(iqn, B, 2, 0.99), "double_q must be 0 or 1")
    assert fails(lib.fb_qnet_forward_iqn(iqn.h, 0, L.ptr(s), B, L.ptr(val), 65, L.ptr(val), None), "M 65 outside 1..64")
    assert lib.fb_qnet_forward_iqn(iqn.h, 0, L.ptr(s), B, L.ptr(val), 0, L.ptr(val), None) == -1
    assert fails(lib.fb_qnet_forward_iqn(iqn.h, 0, L.ptr(s), 97, L.ptr(val), 4, L.ptr(val), None), "exceeds 3*max_batch")
    assert lib.fb_iqn_draw_taus(0, 8, 0, 0, 0, L.ptr(val), None) == -1 and lib.fb_iqn_draw_taus(4, 65, 0, 0, 0, L.ptr(val), None) == -1
    assert lib.fb_iqn_draw_taus(4, 8, 0, 0, 2, L.ptr(val), None) == -1 and lib.fb_iqn_draw_taus(4, 8, 0, 0, 0, None, None) == -1
    rep.set_n_step(3, 0.99)
    with pytest.raises(ValueError, match="fb_iqn_train_from_replay: gamma 0.9.* differs from the gamma"):
        iqn_train_from_replay(rep, iqn, idx, gamma=0.9)
    sb = IqnStep(env, rep, iqn, B, gamma=0.9)
    with pytest.raises(ValueError, match="fb_iqn_step: gamma 0.9"):
        sb(train=True)
    rep.set_n_step(1, 0.99)
    per = VecReplay(2000, N, prioritized=True)
    with pytest.raises(ValueError, match="uniform memory only"):
        iqn_train_from_replay(per, iqn, idx)
    tr = lambda rp, net: lib.fb_iqn_train_from_replay(rp.h, net.h, 0, B, L.ptr(idx), L.ptr(a_out), L.ptr(r32), L.ptr(a_out), None, None, 0, 0, 0.99,
                                                      L.ptr(loss), None, None, None)
    assert fails(tr(per, iqn), "uniform memory only")
    with pytest.raises(ValueError, match="uniform memory only"):
        IqnStep(env, per, iqn, B)
    st = lambda rp, net, n, bt: lib.fb_iqn_step(env.h, rp.h, net.h, C.byref(sb.buf), n, 0, bt, C.c_float(0.1), 0, 0, 1, 0.99, None)
    assert fails(st(per, iqn, N, B), "uniform memory only") and fails(st(rep, iqn, N, 33), "exceeds min(max_batch, 256)")
    assert fails(st(rep, iqn, N + 1, B), "does not match")
    assert untouched()
    # ... and the IQN calls refuse every net that is not an IQN net
    for arch in ("plain", "dueling", "ac", "sac", "c51", "qr"):
        q = QNet(2, 128, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        for rc in (lib.fb_qnet_set_iqn_risk(q.h, C.c_float(0.5)), lib.fb_qnet_get_iqn(q.h, None, None, None, None, None),
                   lib.fb_qnet_forward_iqn(q.h, 0, L.ptr(s), B, L.ptr(val), 4, L.ptr(val), None), ts(q, B, 0, 0.99), tr(rep, q), st(rep, q, N, B)):
            assert rc == -1 and "not an IQN net (fb_qnet_create_iqn)" in lib.fb_last_error().decode(), arch
        tau = torch.full((B, 4), 0.5, device="cuda")
        for call in (lambda: q.set_iqn_risk(0.5), lambda: q.iqn(), lambda: q.forward_iqn(s, tau), lambda: q.iqn_train_step(s, a, r, s2, t),
                     lambda: iqn_train_from_replay(rep, q, idx), lambda: IqnStep(env, rep, q, B)):
            with pytest.raises(ValueError, match="needs an IQN net"):
                call()
        assert same_state(torch, net_state(q), qb) and untouched(), arch


# ================================================================================================================ the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.veciqn import VecIQN
    v = VecIQN(16, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, lr=1e-4, initial_epsilon=0.5, explore=20, n_step=2, double_q=True,
               replace_target_iter=3, max_grad_norm=5.0, cvar=0.5, n_tau=4, n_tau_next=5, n_tau_act=6, **kw)
    losses = [v.step().clone() for _ in range(n)]
    return v, losses


def loop_state(v):
    return (net_state(v.net), v.env.get_state(), v.nib.clone(), v.stats.clone(), np.asarray(v.replay.state_blob()).copy(), v.timeStep, v.epsilon)


def same_loop(torch, x, y):
    return (same_state(torch, x[0], y[0]) and np.array_equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
            and np.array_equal(x[4], y[4]) and x[5:] == y[5:])


def test_vec_iqn_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain
    from dqnflappybird_amd.veciqn import VecIQN
    from dqnflappybird_amd.vecsac import VecSAC
    v, losses = run_steps(7)
    assert not losses[2].any() and all(torch.isfinite(l).all() for l in losses) and losses[6][0] > 0       # steps 0 .. 2 observe, then training
    assert v.timeStep == 7 and len(v.replay) == 7 * 16 and v.epsilon < 0.5 and v.net.iqn() == (4, 5, 6, 1.0, 0.5)
    assert not torch.equal(v.net.store_params(0), v.net.store_params(1))
    st = loop_state(v)
    res = v.evaluate(n_envs=32, episodes=1, max_steps=200)            # evaluate() leaves the training state untouched
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(v), st)
    # save -> load -> four more steps == eleven steps straight
    path = str(tmp_path / "iqn.npz")
    v.save(path)
    assert str(np.load(path)["head"][0]) == "iqn"
    mk = lambda n=16, **kw: VecIQN(n, **{**dict(batch=8, fc_width=128, seed=4, capacity=2000, n_step=2, n_tau=4, n_tau_next=5, n_tau_act=6), **kw})
    with pytest.raises(ValueError, match="was written with seed 4"):
        mk(seed=123).load(path)
    with pytest.raises(ValueError, match="n_envs, batch, fc_width, n_step"):
        mk(32).load(path)
    with pytest.raises(ValueError, match="n_tau, n_tau_next, n_tau_act, kappa"):
        mk(n_tau=8).load(path)
    resumed = mk(lr=3e-5)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and resumed.double_q and resumed.net.iqn()[4] == 0.5
    more = [resumed.step().clone() for _ in range(4)]
    straight, l11 = run_steps(11)
    assert all(torch.equal(x, y) for x, y in zip(more, l11[7:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    # the four loops refuse each other's files; evaluate.py plays an iqn checkpoint
    with pytest.raises(ValueError, match="holds an iqn head"):
        VecBrain(16, observe=0, capacity=2000).load(path)
    with pytest.raises(ValueError, match="holds a iqn head"):
        VecActorCritic(16, rollout=2).load(path)
    with pytest.raises(ValueError, match="holds a iqn head"):
        VecSAC(16, batch=8, fc_width=128, capacity=2000).load(path)
    vb = str(tmp_path / "dqn.npz")
    VecBrain(16, observe=0, capacity=2000).save(vb)
    with pytest.raises(ValueError, match="this is a VecIQN"):
        resumed.load(vb)
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=128)
    assert net.arch == "iqn" and torch.equal(net.store_params(), v.net.store_params()) and net.iqn() == (4, 5, 6, 1.0, 0.5)
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    v.run(1, log_every=1)
