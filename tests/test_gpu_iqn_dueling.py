"""Dueling IQN on the GPU (include/fbdqn.h: FB_ARCH_IQN_DUELING; kernels: the DU instantiations of csrc/fb_iqn.hip) against the float64
restatements of tests/test_iqn_dueling_host.py under the bounds of tests/test_gpu_iqn.py: Q_ATOL on theta, Qbar and T; rtol 1e-4 / atol
1e-6 on the loss; per gradient tensor of the dueling layout (W_v, b_v, W_a, b_a, W_e, b_e included) elementwise rtol 2e-3 / atol 2e-5 x the
tensor's largest reference element, on kink-free inputs.  Then, bit for bit: the reduction to an IQN net (W_v = 0, b_v = 0, rows of W_a
that sum to 0), the shift of W_a's rows and of b_a at A = 2 and 8, ring-fed == gathered, fused Adam == export + (clip) + apply_adam,
fb_iqn_step / fb_iqn_per_step == their separate calls, unit weights == the uniform calls, w = 0.5; the refusals; the loops and their
checkpoints.  The parameters are tests/test_gpu_iqn.py::iqn_params' with the dueling net's own head, so the trunk, the embedding, the
kink-free pool and the tau acceptance are that test's."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import nib_pack
from tests.test_gpu_ac import filled_replay, net_state, same_state
from tests.test_gpu_iqn import GAMMA, MAXB, SHAPES, TAU_MARGIN, eval_q, forward_ref, h64, head0, iqn_params, loop_state, same_loop, t64
from tests.test_gpu_iqn_per import BATCH, CAP, NENV, f32_sum_in_order, grad_buf, leaves, tree_state, twin_memories
from tests.test_gpu_qnet import Q_ATOL, rand_states, trained_like_params
from tests.test_iqn_dueling_host import as_iqn, iqnd_bounds, n_dueling, np_eff
from tests.test_iqn_host import E, F32, iqn_bounds, pre64, qbar_from_h, theta_from_h, torch_iqn_loss, trunk64

pytestmark = pytest.mark.gpu
ARCH = "iqndueling"
EXACT_SHAPES = [(512, 2), (384, 3), (128, 8)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


_params = {}


def iqnd_params(oracle, fc, A, seed=1):
    """tests/test_gpu_iqn.py::iqn_params' recipe with the head of the dueling trained_like_params(oracle.qcfg(fc, A, True), seed) itself
    (scaled as that recipe scales its head) and the same W_e / b_e draws: the trunk and the embedding are iqn_params' bit for bit"""
    if (fc, A, seed) not in _params:
        k = np.float32(np.sqrt(512 / fc))
        d = trained_like_params(oracle, oracle.qcfg(fc, A, True), seed)
        rng = np.random.default_rng(1000 * fc + 10 * A + seed)
        p = np.concatenate([d[:head0(fc)], d[head0(fc):] * k, rng.normal(size=E * fc) * 0.05, rng.normal(size=fc) * 0.02]).astype(np.float32)
        assert len(p) == iqnd_bounds(fc, A)[-1][2]
        q = iqn_params(oracle, fc, A, seed)
        assert np.array_equal(p[:head0(fc)], q[:head0(fc)]) and np.array_equal(p[n_dueling(fc, A):], q[-(E + 1) * fc:])
        p.setflags(write=False)
        _params[(fc, A, seed)] = p
    return _params[(fc, A, seed)]


def bounds(fc, A):
    return {n: (lo, hi) for n, lo, hi in iqnd_bounds(fc, A)}


def with_blocks(p, fc, A, **blocks):
    p = np.array(p)
    for n, (lo, hi) in bounds(fc, A).items():
        if n in blocks:
            p[lo:hi] = np.asarray(blocks[n], F32).ravel() if np.ndim(blocks[n]) else blocks[n]
    return p


def eq64(p, fc, A):
    """the float64 IQN-layout view of the dueling vector p (effective columns): what test_iqn_host's restatements read"""
    return as_iqn(t64(p), fc, A)


_nets, _grads = {}, {}


def case(oracle, shape):
    """one net per shape (gradient-exporting steps leave it as it was): online parameters of seed 1, target parameters of seed 2"""
    from dqnflappybird_amd.vec import QNet
    fc, A, N, Np, K = shape
    if shape not in _nets:
        net, p, pt = QNet(A, fc, ARCH, max_batch=MAXB, n_tau=N, n_tau_next=Np, n_tau_act=K), iqnd_params(oracle, fc, A, 1), iqnd_params(oracle, fc, A, 2)
        assert net.n_params == len(p) and net.iqn() == (N, Np, K, 1.0, 1.0)
        net.load_params(p, 0)
        net.load_params(pt, 1)
        _nets[shape] = (net, p, pt)
    return _nets[shape]


def make_net(oracle, fc=128, A=2, max_batch=32, lr=1e-4, taus=(4, 5, 6), arch=ARCH):
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, arch, max_batch=max_batch, n_tau=taus[0], n_tau_next=taus[1], n_tau_act=taus[2])
    par = iqnd_params if arch == ARCH else iqn_params
    net.load_params(par(oracle, fc, A, 1), 0)
    net.load_params(par(oracle, fc, A, 2), 1)
    net.set_hparams(lr=lr)
    return net


# ================================================================================================================ forward
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_iqn_against_float64(torch_cuda, oracle, shape):
    torch = torch_cuda
    fc, A, M, _, _ = shape
    net, p, pt = case(oracle, shape)
    s, h_on, h_tg = forward_ref(oracle, fc, A)                       # (the trunk is iqn_params': its states and activations serve)
    rng = np.random.default_rng(fc + M)
    tau = np.maximum(rng.random((len(s), M)).astype(F32), F32(2.0 ** -24))
    with torch.no_grad():
        P, PT = eq64(p, fc, A), eq64(pt, fc, A)
        ref_on = torch.cat([theta_from_h(P, h_on[k:k + 128], tau[k:k + 128], fc, A) for k in range(0, len(s), 128)]).numpy()
        ref_tg = theta_from_h(PT, h_tg, tau[:256], fc, A).numpy()
    assert 0.05 < np.abs(ref_on).max() < 100 and (M == 1 or np.abs(ref_on[:, 0] - ref_on[:, -1]).max() > 1e-3)
    sd, td = torch.from_numpy(s).cuda(), torch.from_numpy(tau).cuda()
    for B in (1, 255, 1027):
        got = net.forward_iqn(sd[:B].contiguous(), td[:B].contiguous(), 0)
        assert got.shape == (B, M, A)
        err = np.abs(got.cpu().numpy() - ref_on[:B]).max()
        print(f"dueling forward_iqn {shape} B={B}: max |d theta| {err:.3e}")
        assert err <= Q_ATOL
    got = net.forward_iqn(sd[:255].contiguous(), td[:255].contiguous(), 1)
    np.testing.assert_allclose(got.cpu().numpy(), ref_tg[:255], rtol=0, atol=Q_ATOL)
    assert net.overflow_count() == 0


def q_paths(torch, net, sd, nib, n, which=0):
    """Qbar of the first n states through every forward-only path of net `which` (act / act_nib / fb_eval_q: the online net's)"""
    out = {"forward": net.forward(sd[:n].contiguous(), which)}
    if which == 0:
        a1, out["act"] = net.act(sd[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)
        a2, out["act_nib"] = net.act_nib(nib[:n].contiguous(), 0.0, seed=1, step=2, want_q=True)
        out["eval_q"] = eval_q(torch, net, nib[:n].contiguous())
        assert np.array_equal(a1.cpu().numpy(), out["act"].cpu().numpy().argmax(1))        # the first maximum
        assert np.array_equal(a2.cpu().numpy(), out["act_nib"].cpu().numpy().argmax(1))
    return out


@pytest.mark.parametrize("K", [1, 64])
def test_qbar_through_every_forward_only_path_and_never_stale(torch_cuda, oracle, K):
    """Qbar of forward / act / act_nib / fb_eval_q, both nets, small and large batches, == the mean of float64 theta over the acting grid at
    eta = 1 and 0.25, after every event that rebuilds the fold"""
    torch = torch_cuda
    fc, A = 128, 3
    net = make_net(oracle, fc, A, max_batch=128, lr=1e-3, taus=(4, 4, K))
    s = rand_states(np.random.default_rng(K), 300)
    sd, nib = torch.from_numpy(s).cuda(), torch.from_numpy(nib_pack(s)).cuda()
    eta = [1.0]

    def check(what, floor=0.05):
        worst = 0.0
        for which in (0, 1):
            p = net.store_params(which).cpu().numpy()
            with torch.no_grad():
                want = qbar_from_h(eq64(p, fc, A), h64(p, s, fc, A), K, eta[0], fc, A).numpy()
            assert np.abs(want).max() > floor
            for n in (5, 300):                                       # the small-batch and the large-batch forward
                for q in q_paths(torch, net, sd, nib, n, which).values():
                    worst = max(worst, np.abs(q.cpu().numpy() - want[:n]).max())
        print(f"dueling Qbar K={K} eta={eta[0]} after {what}: max |dQ| {worst:.3e}")
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
    net.iqn_per_train_step(st(), a, r, st(), t, torch.full((B,), 0.5, device="cuda"), gamma=GAMMA, seed=3, step=2)
    check("a fused prioritized train step")
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
    check("init_params", floor=0.01)                                # (a fresh net: Q ~ b_v = 0.01, still 100 Q_ATOL)
    net.load_params(iqnd_params(oracle, fc, A, 2), 0)
    check("load_params again")


def test_init_params_are_the_dueling_nets(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    iqnd, duel, iqn = QNet(A, fc, ARCH, max_batch=8), QNet(A, fc, "dueling", max_batch=8), QNet(A, fc, "iqn", max_batch=8)
    for n in (iqnd, duel, iqn):
        n.init_params(seed=11)
    pi, pd, pq = (n.store_params().cpu().numpy() for n in (iqnd, duel, iqn))
    assert len(pd) == n_dueling(fc, A) and np.array_equal(pi[:len(pd)], pd)        # up to b_a: the FB_ARCH_DUELING net of the seed, bit for bit
    b = bounds(fc, A)
    we = pi[b["W_e"][0]:b["W_e"][1]]
    assert np.abs(we).max() <= 0.02 + 1e-9 and 0.005 < we.std() < 0.012 and (pi[b["b_e"][0]:b["b_e"][1]] == 1).all()
    assert pi[b["b_v"][0]] == F32(0.01) and (pi[b["b_a"][0]:b["b_a"][1]] == F32(0.01)).all()
    assert len(pi) == len(pq) + fc + 1 and not np.array_equal(we, pq[-(E + 1) * fc:-fc])      # every weight by its own index
    assert iqnd.iqn() == (8, 8, 32, 1.0, 1.0) and iqnd.arch == ARCH
    s = torch.from_numpy(rand_states(np.random.default_rng(2), 6)).cuda()
    qi, qd = iqnd.forward(s).cpu().numpy(), duel.forward(s).cpu().numpy()
    print(f"a fresh dueling IQN net against the dueling net of its seed: max |Qbar - Q| {np.abs(qi - qd).max():.3e}")
    assert np.abs(qi - qd).max() < 0.05                              # (b_e = 1, W_e small: phi ~ 1, the net starts near the dueling net of its seed)


# ================================================================================================================ train step
def ref_step(oracle, shape, B):
    """tests/test_gpu_iqn.py::ref_step for the dueling net: kink-free s from the same pool, its rng, its tau acceptance; s' replaced while a
    float64 top-two Qbar gap of either net is below 10 Q_ATOL; the float64 loss, targets and gradient for double_q = 0 and 1"""
    import torch
    fc, A, N, Np, K = shape
    if (shape, B) not in _grads:
        p, ptg = iqnd_params(oracle, fc, A, 1), iqnd_params(oracle, fc, A, 2)
        pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
        s = np.array(pool[:B])
        rng = np.random.default_rng(1000 * fc + 10 * A + B + N)
        a = rng.integers(0, A, B).astype(np.uint8)
        r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.6, 0.2, 0.2])
        t = (rng.random(B) < 0.25).astype(np.uint8)
        if B > 1:
            t[0], t[1] = 1, 0
        with torch.no_grad():
            P, PT = eq64(p, fc, A), eq64(ptg, fc, A)
        s2 = rand_states(rng, B)
        rounds = 0
        for rounds in range(20):
            with torch.no_grad():
                h2o, h2t = trunk64(P, s2, fc, A), trunk64(PT, s2, fc, A)
                qo, qt = qbar_from_h(P, h2o, K, 1.0, fc, A), qbar_from_h(PT, h2t, K, 1.0, fc, A)
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
                        if pre64(P, np.array([x]), fc, A).abs().min().item() >= TAU_MARGIN:
                            break
                    tau[bi, i] = x
        print(f"dueling tau draws {shape} B={B}: accepted {B * N} of {drawn}; s' replacement rounds {rounds}")
        assert B * N >= 0.8 * drawn
        taup = np.maximum(rng.random((B, Np)).astype(F32), F32(2.0 ** -24))
        rd = torch.as_tensor(np.where(r == F32(0.1), 0.1, r.astype(np.float64)))
        nd = torch.as_tensor((t == 0).astype(np.float64))
        ar = torch.arange(B)
        out = {}
        pg = t64(p).requires_grad_(True)
        q = as_iqn(pg, fc, A)
        th = theta_from_h(q, trunk64(q, s, fc, A), tau, fc, A)[ar, :, torch.as_tensor(a.astype(np.int64))]
        for dq, qsel in ((0, qt), (1, qo)):
            astar = qsel.argmax(1)
            with torch.no_grad():
                T = rd[:, None] + nd[:, None] * GAMMA * theta_from_h(PT, h2t, taup, fc, A)[ar, :, astar]
            loss, lb = torch_iqn_loss(th, T, tau, 1.0)
            grad, = torch.autograd.grad(loss, pg, retain_graph=dq == 0)
            u = (T[:, None, :] - th.detach()[:, :, None]).numpy()
            if B >= 32:
                assert (u > 0).any() and (u < 0).any() and (np.abs(u) < 1.0).any() and (np.abs(u) > 1.0).any() and t.any() and not t.all()
            out[dq] = (loss.item(), T.numpy(), grad.numpy(), lb.detach().numpy())
        _grads[(shape, B)] = (s, a, r, s2, t, tau, taup, out)
    return _grads[(shape, B)]


def check_grads(g, g0, fc, A, only=None):
    """tests/test_gpu_sac.py::check_sac_grads' bounds over the dueling layout, every tensor elementwise (kink-free), W_v b_v W_a b_a W_e b_e
    included; then sum_c dW_a[k, c] = 0 and sum_c db_a[c] = 0 within W_a's / b_a's atol (the mean is subtracted on the device)"""
    b = bounds(fc, A)
    for name, (lo, hi) in b.items():
        if only and name not in only:
            continue
        ref, got = g0[lo:hi], g[lo:hi]
        scale = np.abs(ref).max()
        assert scale > 0, name
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=name)
    if not only:
        for name in ("W_a", "b_a"):
            lo, hi = b[name]
            rows = g[lo:hi].astype(np.float64).reshape(-1, A).sum(1)
            assert np.abs(rows).max() <= 2e-5 * np.abs(g0[lo:hi]).max(), name


TRAIN_CASES = [(SHAPES[0], B) for B in (1, 32, 255, 256)] + [(sh, 32) for sh in SHAPES[1:]]


@pytest.mark.parametrize("double_q", [0, 1])
@pytest.mark.parametrize("shape,B", TRAIN_CASES)
def test_train_step_against_autograd(torch_cuda, oracle, shape, B, double_q):
    """gathered, gradient-exporting: the loss, the targets and every gradient tensor; nothing is masked"""
    torch = torch_cuda
    fc, A, N, Np, K = shape
    net, p, ptg = case(oracle, shape)
    s, a, r, s2, t, tau, taup, out = ref_step(oracle, shape, B)
    want, T0, g0, _ = out[double_q]
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, T = net.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, double_q=bool(double_q), tau=d(tau), tau_next=d(taup), flat_grad=grad)
    loss, T = loss.item(), T.cpu().numpy()
    print(f"dueling iqn {shape} B={B} double_q={double_q}: loss {loss!r} / {want!r}; max |dT| {np.abs(T - T0).max():.3e}")
    np.testing.assert_allclose(T, T0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
    check_grads(grad.cpu().numpy(), g0, fc, A)
    assert np.array_equal(net.store_params(0).cpu().numpy(), p) and np.array_equal(net.store_params(1).cpu().numpy(), ptg)      # gradient-only mode
    assert net.overflow_count() == 0


@pytest.mark.parametrize("double_q", [0, 1])
def test_weighted_train_step_against_autograd(torch_cuda, oracle, double_q):
    """the prioritized form on the generic path (A = 3): w in (0, 1], abs_err = l_b without the weight"""
    torch = torch_cuda
    import torch as th_
    shape, B = SHAPES[1], 32
    fc, A, N, Np, K = shape
    net, p, ptg = case(oracle, shape)
    s, a, r, s2, t, tau, taup, out = ref_step(oracle, shape, B)
    _, T0, _, lb0 = out[double_q]
    rng = np.random.default_rng(B)
    w = (1.0 - rng.random(B)).astype(F32)
    w[0], w[1] = 1.0, F32(2.0 ** -10)
    pg = t64(p).requires_grad_(True)
    q = as_iqn(pg, fc, A)
    th = theta_from_h(q, trunk64(q, s, fc, A), tau, fc, A)[th_.arange(B), :, th_.as_tensor(a.astype(np.int64))]
    _, lb = torch_iqn_loss(th, th_.as_tensor(T0), tau, 1.0)
    lossw = (th_.as_tensor(w.astype(np.float64)) * lb).mean()
    g0, = th_.autograd.grad(lossw, pg)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = grad_buf(torch, net)
    loss, ae, T = net.iqn_per_train_step(d(s), d(a), d(r), d(s2), d(t), d(w), gamma=GAMMA, double_q=bool(double_q), tau=d(tau), tau_next=d(taup),
                                         flat_grad=grad)
    print(f"dueling iqn per double_q={double_q}: loss {loss.item()!r} / {lossw.item()!r}; max |d abs_err| {np.abs(ae.cpu().numpy() - lb0).max():.3e}")
    np.testing.assert_allclose(T.cpu().numpy(), T0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss.item(), lossw.item(), rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ae.cpu().numpy(), lb0, rtol=1e-4, atol=1e-6)
    check_grads(grad.cpu().numpy(), g0.numpy(), fc, A)


# ================================================================================================================ exact cases
def dyadic(x, bits=12):
    return (np.round(np.asarray(x, np.float64) * 2.0 ** bits) * 2.0 ** -bits).astype(F32)


def exact_inputs(torch, oracle, fc, A, B=32):
    rng = np.random.default_rng(fc + A)
    s, s2 = (torch.from_numpy(rand_states(rng, B)).cuda() for _ in range(2))
    a = torch.from_numpy(rng.integers(0, A, B).astype(np.uint8)).cuda()
    r = torch.from_numpy(rng.choice(np.array([0.1, 3, -3], F32), B)).cuda()
    t = torch.from_numpy((rng.random(B) < 0.3).astype(np.uint8)).cuda()
    tau = torch.from_numpy(np.maximum(rng.random((B, 8)).astype(F32), F32(2.0 ** -24))).cuda()
    taup = torch.from_numpy(np.maximum(rng.random((B, 8)).astype(F32), F32(2.0 ** -24))).cuda()
    w = torch.from_numpy((1.0 - rng.random(B)).astype(F32)).cuda()
    return s, a, r, s2, t, tau, taup, w


def all_outputs(torch, net, inp, double_q):
    """theta of both nets, Qbar on every path, then T / loss / abs_err / the gradient of the uniform and of the prioritized step"""
    s, a, r, s2, t, tau, taup, w = inp
    nib = torch.from_numpy(nib_pack(s.cpu().numpy())).cuda()
    out = {"theta0": net.forward_iqn(s, tau, 0), "theta1": net.forward_iqn(s2, taup, 1), "qbar1": net.forward(s2, 1)}
    out.update({f"q_{k}": v for k, v in q_paths(torch, net, s, nib, len(s)).items()})
    g, gw = grad_buf(torch, net), grad_buf(torch, net)
    out["loss"], out["T"] = net.iqn_train_step(s, a, r, s2, t, gamma=GAMMA, double_q=double_q, tau=tau, tau_next=taup, flat_grad=g)
    out["lossw"], out["abs_err"], out["Tw"] = net.iqn_per_train_step(s, a, r, s2, t, w, gamma=GAMMA, double_q=double_q, tau=tau, tau_next=taup, flat_grad=gw)
    return out, g.cpu().numpy(), gw.cpu().numpy()


@pytest.mark.parametrize("fc,A", EXACT_SHAPES)
def test_exact_reduction_to_iqn(torch_cuda, oracle, fc, A):
    """W_v = 0, b_v = 0 and W_a / b_a multiples of 2^-12 whose rows sum to exactly 0: We == W_a and be == b_a in fp32 (checked in numpy), so
    against the IQN net with W_q = W_a, b_q = b_a, the same trunk and embedding: theta, Qbar on every path, T, loss, abs_err and the gradients
    of the trunk, W_fc1, b_fc1, W_e, b_e bit for bit; dW_v == sum_c dW_q and dW_a == dW_q - dW_v / A within the gradient bound"""
    torch = torch_cuda
    bd, bi = bounds(fc, A), {n: (lo, hi) for n, lo, hi in iqn_bounds(fc, A)}
    nets = {}
    for which, seed in ((0, 1), (1, 2)):
        p = iqnd_params(oracle, fc, A, seed)
        wa = dyadic(p[bd["W_a"][0]:bd["W_a"][1]].reshape(fc, A))
        wa[:, -1] = -wa[:, :-1].sum(1, dtype=np.float64)
        ba = dyadic(p[bd["b_a"][0]:bd["b_a"][1]])
        ba[-1] = -ba[:-1].sum(dtype=np.float64)
        assert (wa.astype(np.float64).sum(1) == 0).all() and ba.astype(np.float64).sum() == 0 and np.abs(wa).max() > 0.01
        We, be = np_eff(np.zeros(fc, F32), np.zeros(1, F32), wa, ba)
        assert np.array_equal(We, wa) and np.array_equal(be, ba)      # the effective column IS W_a, in the pinned fp32 arithmetic
        pd = with_blocks(p, fc, A, W_v=0, b_v=0, W_a=wa, b_a=ba)
        pi = np.concatenate([pd[:head0(fc)], wa.ravel(), ba, pd[bd["W_e"][0]:]]).astype(F32)
        nets[which] = (pd, pi)
    from dqnflappybird_amd.vec import QNet
    nd, ni = QNet(A, fc, ARCH, max_batch=64), QNet(A, fc, "iqn", max_batch=64)
    for which in (0, 1):
        nd.load_params(nets[which][0], which)
        ni.load_params(nets[which][1], which)
    inp = exact_inputs(torch, oracle, fc, A)
    for dq in (False, True):
        od, gd, gwd = all_outputs(torch, nd, inp, dq)
        oi, gi, gwi = all_outputs(torch, ni, inp, dq)
        for k in od:
            assert torch.equal(od[k], oi[k]), (k, dq)
        assert od["loss"].item() > 0 and (od["abs_err"] > 0).all()
        for g_d, g_i in ((gd, gi), (gwd, gwi)):
            for name in ("W_conv1", "b_conv1", "W_conv2", "b_conv2", "W_conv3", "b_conv3", "W_fc1", "b_fc1", "W_e", "b_e"):
                x, y = g_d[bd[name][0]:bd[name][1]], g_i[bi[name][0]:bi[name][1]]
                assert np.abs(y).max() > 0 and np.array_equal(x, y), (name, dq)
            dwq, dbq = g_i[bi["W_q"][0]:bi["W_q"][1]].astype(np.float64).reshape(fc, A), g_i[bi["b_q"][0]:bi["b_q"][1]].astype(np.float64)
            want = np.zeros(len(g_d))
            want[bd["W_v"][0]:bd["W_v"][1]] = dwq.sum(1)
            want[bd["b_v"][0]] = dbq.sum()
            want[bd["W_a"][0]:bd["W_a"][1]] = (dwq - dwq.mean(1, keepdims=True)).ravel()
            want[bd["b_a"][0]:bd["b_a"][1]] = dbq - dbq.mean()
            check_grads(g_d, want, fc, A, only=("W_v", "b_v", "W_a", "b_a"))


@pytest.mark.parametrize("fc,A", EXACT_SHAPES)
def test_exact_shift_of_the_advantage_rows(torch_cuda, oracle, fc, A):
    """every head value a multiple of 2^-12; W_a[k, :] += c_k (dyadic) and b_a += a dyadic constant: at A = 2 and 8 the mean takes the shift
    exactly, so theta, Qbar, T, the loss, abs_err and the gradients of W_e / b_e keep their bits.  At A = 3 the division is inexact: numpy
    shows We moves, and the outputs are held to Q_ATOL"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    bd = bounds(fc, A)
    rng = np.random.default_rng(fc * A)
    ck = dyadic(rng.normal(size=fc) * 0.02)
    nets, moved = [QNet(A, fc, ARCH, max_batch=64) for _ in range(2)], False
    for which, seed in ((0, 1), (1, 2)):
        p = iqnd_params(oracle, fc, A, seed)
        cut = lambda n: p[bd[n][0]:bd[n][1]]
        wv, bv, wa, ba = dyadic(cut("W_v")), dyadic(cut("b_v")), dyadic(cut("W_a")).reshape(fc, A), dyadic(cut("b_a"))
        wa2, ba2 = (wa + ck[:, None]).astype(F32), (ba + F32(0.375)).astype(F32)
        assert np.array_equal(wa2.astype(np.float64), wa.astype(np.float64) + ck[:, None]) and np.abs(ck).max() > 0      # the shift itself is exact
        e1, e2 = np_eff(wv, bv, wa, ba), np_eff(wv, bv, wa2, ba2)
        moved |= not (np.array_equal(e1[0], e2[0]) and np.array_equal(e1[1], e2[1]))
        nets[0].load_params(with_blocks(p, fc, A, W_v=wv, b_v=bv, W_a=wa, b_a=ba), which)
        nets[1].load_params(with_blocks(p, fc, A, W_v=wv, b_v=bv, W_a=wa2, b_a=ba2), which)
    assert moved == (A == 3)
    inp = exact_inputs(torch, oracle, fc, A)
    o1, g1, gw1 = all_outputs(torch, nets[0], inp, True)
    o2, g2, gw2 = all_outputs(torch, nets[1], inp, True)
    lo, hi = bd["W_e"][0], bd["b_e"][1]
    if A != 3:
        for k in o1:
            assert torch.equal(o1[k], o2[k]), k
        assert np.abs(g1[lo:hi]).max() > 0 and np.array_equal(g1[lo:hi], g2[lo:hi]) and np.array_equal(gw1[lo:hi], gw2[lo:hi])
    else:
        for k in o1:
            if k not in ("loss", "lossw", "abs_err"):
                assert (o1[k] - o2[k]).abs().max().item() <= Q_ATOL, k
        print(f"shift at A = 3: max |d theta| {(o1['theta0'] - o2['theta0']).abs().max().item():.3e}, loss {o1['loss'].item()!r} / {o2['loss'].item()!r}")
        np.testing.assert_allclose(o2["loss"].item(), o1["loss"].item(), rtol=1e-4, atol=1e-6)


def test_an_action_past_the_head_reads_the_last_one(torch_cuda, oracle):
    torch = torch_cuda
    shape = SHAPES[1]
    net, p, ptg = case(oracle, shape)
    s, a, r, s2, t, tau, taup, _ = ref_step(oracle, shape, 32)
    d = lambda x: torch.from_numpy(x).cuda()
    g1, g2 = grad_buf(torch, net), grad_buf(torch, net)
    a1, a2 = a.copy(), a.copy()
    a1[3], a2[3] = shape[1] - 1, 200
    l1, _ = net.iqn_train_step(d(s), d(a1), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g1)
    l2, _ = net.iqn_train_step(d(s), d(a2), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g2)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


# ================================================================================================================ compositions
def ring_pair(torch, oracle, B, n_nets, n_step=1, lr=1e-4):
    """B transitions of a played memory as ring positions and as gathered tensors, n_nets equal dueling nets (online / target differ)"""
    fc, A = 512, 2
    N, pushes = 64, 9
    env, rep, pushed = filled_replay(torch, N, pushes)
    if n_step > 1:
        rep.set_n_step(n_step, GAMMA)
    rng = np.random.default_rng(B)
    idx = torch.from_numpy(rng.permutation(N * (pushes - n_step))[:B].astype(np.int64)).cuda()
    s, a, r, s2, t = rep.gather(idx)
    nets = [make_net(oracle, fc, A, max_batch=256, lr=lr, taus=(8, 8, 32)) for _ in range(n_nets)]
    return rep, idx, (s, a, r, s2, t), nets, iqnd_params(oracle, fc, A, 1)


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B, n_step):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2, n_step)
    g_gath, g_ring = grad_buf(torch, nets[0]), grad_buf(torch, nets[1])
    l_gath, y_gath = nets[0].iqn_train_step(s, a, r, s2, t, gamma=bootstrap_gamma(GAMMA, n_step), double_q=True, seed=5, step=6, flat_grad=g_gath)
    l_ring, a_o, r_o, t_o, y_ring = iqn_train_from_replay(rep, nets[1], idx, gamma=GAMMA, double_q=True, seed=5, step=6, flat_grad=g_ring,
                                                          want_target=True)
    assert torch.equal(a_o, a) and torch.equal(r_o, r) and torch.equal(t_o, t) and g_gath.abs().max() > 0
    print(f"dueling ring-fed vs gathered B={B} n_step={n_step}: loss {l_gath.item()!r} / {l_ring.item()!r}, "
          f"{int((g_ring != g_gath).sum())} of {g_gath.numel()} gradient elements differ")
    assert torch.equal(l_ring, l_gath) and torch.equal(y_ring, y_gath) and torch.equal(g_ring, g_gath)
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p)


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("B,ring", [(32, False), (32, True), (256, True)])
def test_fused_adam_equals_export_plus_apply_adam(torch_cuda, oracle, B, ring, clip):
    torch = torch_cuda
    from dqnflappybird_amd.vec import iqn_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2)
    for n in nets:
        n.set_max_grad_norm(clip)
    g = grad_buf(torch, nets[0])
    kw = dict(gamma=GAMMA, seed=3, step=4)
    l0 = iqn_train_from_replay(rep, nets[0], idx, flat_grad=g, **kw)[0] if ring else nets[0].iqn_train_step(s, a, r, s2, t, flat_grad=g, **kw)[0]
    if clip:
        nets[0].clip_grad(g)
        assert nets[0].grad_norm()[1] < 1.0
    nets[0].apply_adam(g)
    l1 = iqn_train_from_replay(rep, nets[1], idx, **kw)[0] if ring else nets[1].iqn_train_step(s, a, r, s2, t, **kw)[0]
    st = [net_state(n) for n in nets]
    assert torch.equal(l0, l1) and same_state(torch, st[0], st[1])
    b = bounds(512, 2)
    moved = (st[0][0].cpu().numpy() != p)
    assert all(moved[b[n][0]:b[n][1]].any() for n in ("W_v", "b_v", "W_a", "b_a", "W_e", "b_e", "W_fc1", "W_conv1"))      # Adam reached every part
    x = torch.from_numpy(rand_states(np.random.default_rng(0), 8)).cuda()
    assert torch.equal(nets[0].forward(x), nets[1].forward(x))        # ... and the folds behind both


@pytest.mark.parametrize("N,batch", [(8, 8), (300, 32)])
def test_iqn_step_equals_its_separate_calls(torch_cuda, oracle, N, batch):
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnStep, VecGameState, VecReplay, iqn_train_from_replay
    seed = (3 << 32) | 9
    p = iqnd_params(oracle, 512, 2)

    def make():
        env, rep, net = VecGameState(N, seed=5), VecReplay(4000, N), make_net(oracle, 512, 2, max_batch=max(N, batch), taus=(8, 8, 32))
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


# ---- the prioritized calls
@pytest.mark.parametrize("n_step", [1, 3])
def test_unit_weights_are_the_uniform_calls_and_half_weights_halve(torch_cuda, oracle, n_step):
    """gathered and ring-fed _per calls with w = 1 == the two uniform calls (loss, T, flat gradient), bit for bit; w = 0.5: the loss and the
    gradients of W_v, b_v, W_a, b_a, W_e, b_e exactly half, abs_err and T unchanged, the trunk within the gradient bound"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_per_train_from_replay, iqn_train_from_replay
    B, fc, A = BATCH, 128, 2
    env, per, uni = twin_memories(torch, 6, n_step)
    idx = leaves(np.random.default_rng(n_step), per, B)
    pos = idx - (per.capacity - 1)
    s, a, r, s2, t = (x.clone() for x in per.gather(idx))
    ones = torch.ones(B, dtype=torch.float32, device="cuda")
    net = make_net(oracle, fc, A)
    G = bootstrap_gamma(GAMMA, n_step)
    bd = bounds(fc, A)
    for dq in (False, True):
        g = [grad_buf(torch, net) for _ in range(5)]
        kw = dict(double_q=dq, seed=5, step=6)
        l0, y0 = net.iqn_train_step(s, a, r, s2, t, gamma=G, flat_grad=g[0], **kw)
        l1, _, _, _, y1 = iqn_train_from_replay(uni, net, pos, gamma=GAMMA, flat_grad=g[1], want_target=True, **kw)
        l2, ae2, y2 = net.iqn_per_train_step(s, a, r, s2, t, ones, gamma=G, flat_grad=g[2], **kw)
        l3, a3, r3, t3, y3, ae3 = iqn_per_train_from_replay(per, net, idx, ones, gamma=GAMMA, flat_grad=g[3], want_target=True, **kw)
        assert g[0].abs().max() > 0 and torch.equal(l0, l1) and torch.equal(g[0], g[1]) and torch.equal(y0, y1)
        for l, y, gg, ae in ((l2, y2, g[2], ae2), (l3, y3, g[3], ae3)):
            assert torch.equal(l, l0) and torch.equal(y, y0) and torch.equal(gg, g[0])
            assert (ae >= 0).all() and ae.max() > 0
            assert l.cpu().numpy()[0].view(np.uint32) == (f32_sum_in_order(ae.cpu().numpy()) / F32(B)).view(np.uint32)
        assert torch.equal(ae2, ae3) and torch.equal(a3, a) and torch.equal(r3, r) and torch.equal(t3, t)
        lh, aeh, yh = net.iqn_per_train_step(s, a, r, s2, t, 0.5 * ones, gamma=G, flat_grad=g[4], **kw)
        assert torch.equal(aeh, ae2) and torch.equal(yh, y0) and lh.item() == F32(0.5) * F32(l0.item())
        g1, gh = g[0].cpu().numpy(), g[4].cpu().numpy()
        for name in ("W_v", "b_v", "W_a", "b_a", "W_e", "b_e"):
            lo, hi = bd[name]
            assert np.abs(g1[lo:hi]).max() > 0 and np.array_equal(gh[lo:hi], F32(0.5) * g1[lo:hi]), name
        check_grads(gh, 0.5 * g1.astype(np.float64), fc, A, only=("W_conv1", "W_conv2", "W_conv3", "W_fc1", "b_fc1"))
    assert np.array_equal(net.store_params(0).cpu().numpy(), iqnd_params(oracle, fc, A, 1))      # gradient-only mode


@pytest.mark.parametrize("n_step", [1, 2])
def test_iqn_per_step_equals_its_separate_calls(torch_cuda, oracle, n_step):
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep, VecGameState, VecReplay, iqn_per_train_from_replay
    seed = (3 << 32) | 9

    def world():
        env = VecGameState(NENV, seed=5)
        rep = VecReplay(CAP, NENV, prioritized=True, n_step=n_step, gamma=GAMMA)
        rep.seed(7)
        net = make_net(oracle, max_batch=NENV)
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = world()
    e2, r2, n2, nib2 = world()
    steps = {dq: IqnPerStep(e1, r1, n1, BATCH, GAMMA, dq) for dq in (False, True)}
    trained = 0
    for k, (train, dq, eps) in enumerate([(False, False, 0.5), (True, True, 0.3), (True, False, 0.5), (False, True, 0.0), (True, True, 0.1),
                                          (True, False, 1.0)]):
        train = train and k >= n_step - 1
        one = steps[dq]
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = n2.act_nib(nib2, eps, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        r2.push(e2.frame_bits, a2, rew, term)
        assert torch.equal(a1, a2) and torch.equal(nib1, nib2), k
        if train:
            idx, isw = r2.sample(BATCH)
            idx, isw = idx.clone(), isw.clone()
            loss, a_o, r_o, t_o, ae = iqn_per_train_from_replay(r2, n2, idx, isw.to(torch.float32), gamma=GAMMA, double_q=dq, seed=seed, step=k)
            assert torch.equal(one.idx, idx) and torch.equal(one.isw, isw) and torch.equal(one.isw32, isw.to(torch.float32)), k
            assert torch.equal(one.loss, loss) and torch.equal(one.abs_err, ae) and (ae >= 0).all(), k
            assert torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
            r2.update_priorities(idx, abs_err=ae.clone())
            trained += 1
        assert same_state(torch, net_state(n1), net_state(n2)), k
        x, y = tree_state(r1), tree_state(r2)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], k
    assert trained == 4 and len(r1) == 6 * NENV
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), iqnd_params(oracle, 128, 2, 1))


# ================================================================================================================ refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    """a dueling IQN net is refused wherever an IQN net is, in the same words, and the IQN calls keep their own limits on it"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import (ALGOS, IqnPerStep, IqnStep, QNet, SacStep, TrainSteps, VecReplay, VecStep, iqn_per_train_from_replay,
                                       iqn_train_from_replay, sac_train_from_replay, train_from_replay)
    lib = L.lib()
    N, B = NENV, BATCH
    net = make_net(oracle)
    env, per, uni = twin_memories(torch, 6)
    env.track_state()
    blobs, before, envs = [np.asarray(m.state_blob()).copy() for m in (per, uni)], net_state(net), env.get_state().copy()

    def untouched():
        torch.cuda.synchronize()
        return (all(np.array_equal(np.asarray(m.state_blob()), b) for m, b in zip((per, uni), blobs)) and same_state(torch, net_state(net), before)
                and np.array_equal(env.get_state(), envs))

    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    lv = leaves(np.random.default_rng(0), per, B)
    s, a, r, s2, t = uni.gather(idx)
    for algo in sorted(ALGOS):
        with pytest.raises(ValueError, match="fb_qnet_train_step: an IQN net trains through"):
            net.train_step(algo, s, a, r, s2, t, isw=r)
        with pytest.raises(ValueError, match="fb_train_from_replay: an IQN net"):
            train_from_replay(uni, net, algo, idx, isw=r)
    with pytest.raises(ValueError, match="fb_train_steps: an IQN net"):
        TrainSteps(uni, net, B, "dqn")(1)
    with pytest.raises(ValueError, match="fb_vec_step: an IQN net"):
        VecStep(env, uni, net, B, "dqn")(0.1, train=True)
    buf = VecStep(env, uni, net, B, "dqn").buf
    assert lib.fb_vec_step_dp(None, env.h, uni.h, net.h, C.byref(buf), N, 0, B, 0.1, 0, 0, 1, 0.99, 0, None) == -1
    assert "data-parallel IQN is not supported" in lib.fb_last_error().decode()
    for call, msg in ((lambda: net.set_huber(1.0), "fb_qnet_set_huber"), (lambda: net.set_munchausen(), "fb_qnet_set_munchausen"),
                      (lambda: net.set_train_dtype("bf16"), "an IQN net trains in FB_DTYPE_F32 only"),
                      (lambda: net.set_inference_dtype("bf16"), "an IQN net computes in FB_DTYPE_F32 only"),
                      (lambda: net.set_ac(), "needs an actor-critic net"), (lambda: net.set_sac(), "needs a SAC net"),
                      (lambda: sac_train_from_replay(uni, net, idx), "needs a SAC net"), (lambda: SacStep(env, uni, net, B), "needs a SAC net"),
                      (lambda: net.reset_noise(), "noisy"), (lambda: QNet(2, 128, ARCH, noisy=True), "noisy layers are offered on the C51 heads only"),
                      (lambda: iqn_train_from_replay(per, net, lv), "uniform memory only"), (lambda: IqnStep(env, per, net, B), "uniform memory only"),
                      (lambda: iqn_per_train_from_replay(uni, net, idx, torch.ones(B, device="cuda")), "prioritized memory only"),
                      (lambda: IqnPerStep(env, uni, net, B), "prioritized memory only"),
                      (lambda: net.set_iqn_risk(0.0), "eta")):
        with pytest.raises(ValueError, match=msg):
            call()
    fails = lambda rc, word: rc == -1 and word in lib.fb_last_error().decode()
    val = torch.zeros(64 * 64, dtype=torch.float32, device="cuda")
    loss = torch.zeros(6, dtype=torch.float32, device="cuda")
    r32, a_out = torch.zeros(B, dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    h = C.c_void_p()
    assert fails(lib.fb_qnet_create(L.ARCH_IQN_DUELING, 128, 2, 32, C.byref(h)), "fb_qnet_create: arch must be 0 or 1") and not h.value
    assert fails(lib.fb_qnet_create(L.ARCH_IQN, 128, 2, 32, C.byref(h)), "fb_qnet_create_iqn")
    assert lib.fb_qnet_create_c51_noisy(L.ARCH_IQN_DUELING, 128, 2, 51, C.c_float(-10), C.c_float(10), C.c_float(0.5), 32, C.byref(h)) == -1
    for bad, word in (((128, 1, 8, 8, 32, 1.0), "fb_qnet_create_iqn_dueling: n_actions must be in 2..8"), ((128, 9, 8, 8, 32, 1.0), "n_actions must be in 2..8"),
                      ((128, 2, 0, 8, 32, 1.0), "n_tau=0"), ((128, 2, 65, 8, 32, 1.0), "n_tau=65"), ((128, 2, 8, 0, 32, 1.0), "n_tau_next=0"),
                      ((128, 2, 8, 8, 65, 1.0), "n_tau_act=65"), ((128, 2, 8, 8, 32, 0.0), "kappa must be finite and > 0"),
                      ((100, 2, 8, 8, 32, 1.0), "fb_qnet_create_iqn_dueling: fc_width must be a multiple of 128")):
        assert fails(lib.fb_qnet_create_iqn_dueling(*bad[:5], C.c_float(bad[5]), 32, C.byref(h)), word), bad
    assert fails(lib.fb_qnet_forward_dist(net.h, 0, L.ptr(s), B, L.ptr(val), None), "not a C51 net")
    assert fails(lib.fb_qnet_forward_quantiles(net.h, 0, L.ptr(s), B, L.ptr(val), None), "not a QR net")
    assert fails(lib.fb_qnet_forward_sac(net.h, 0, L.ptr(s), B, L.ptr(val), L.ptr(val), L.ptr(val), None), "not a SAC net")
    ts = lambda Bn, dq, g: lib.fb_qnet_iqn_train_step(net.h, dq, Bn, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), None, None, 0, 0, g,
                                                      L.ptr(loss), None, None, None)
    assert fails(ts(33, 0, 0.99), "exceeds min(max_batch, 256)") and fails(ts(B, 0, 1.5), "gamma must be in [0, 1]") and fails(ts(B, 2, 0.99), "double_q must be 0 or 1")
    assert fails(lib.fb_qnet_forward_iqn(net.h, 0, L.ptr(s), B, L.ptr(val), 65, L.ptr(val), None), "M 65 outside 1..64")
    assert fails(lib.fb_qnet_iqn_per_train_step(net.h, 0, B, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), None, None, None, 0, 0, 0.99, L.ptr(loss),
                                                None, None, None, None), "needs the importance weights (isw) and abs_err")
    sb = IqnStep(env, uni, net, B)
    st = lambda rp, n, bt: lib.fb_iqn_step(env.h, rp.h, net.h, C.byref(sb.buf), n, 0, bt, C.c_float(0.1), 0, 0, 1, 0.99, None)
    assert fails(st(per, N, B), "uniform memory only") and fails(st(uni, N, 33), "exceeds min(max_batch, 256)") and fails(st(uni, N + 1, B), "does not match")
    pb = IqnPerStep(env, per, net, B)
    assert fails(lib.fb_iqn_per_step(env.h, uni.h, net.h, C.byref(pb.buf), N, 0, B, C.c_float(0.1), 0, 0, 1, 0.99, None), "prioritized memory only")
    assert untouched()


# ================================================================================================================ the loops
def run_steps(n, **kw):
    from dqnflappybird_amd.veciqn import VecIQN
    v = VecIQN(16, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, lr=1e-4, initial_epsilon=0.5, explore=20, n_step=2, double_q=True,
               replace_target_iter=3, max_grad_norm=5.0, cvar=0.5, n_tau=4, n_tau_next=5, n_tau_act=6, dueling=True, **kw)
    losses = [v.step().clone() for _ in range(n)]
    return v, losses


@pytest.mark.parametrize("prioritized", [False, True])
def test_vec_iqn_dueling_loop_and_checkpoint(torch_cuda, tmp_path, prioritized):
    torch = torch_cuda
    from dqnflappybird_amd.veciqn import VecIQN
    v, losses = run_steps(7, prioritized=prioritized)
    assert not losses[2].any() and all(torch.isfinite(l).all() for l in losses) and losses[6][0] > 0
    assert v.timeStep == 7 and v.net.arch == ARCH and v.dueling and v.net.iqn() == (4, 5, 6, 1.0, 0.5)
    assert not torch.equal(v.net.store_params(0), v.net.store_params(1))
    st = loop_state(v)
    res = v.evaluate(n_envs=32, episodes=1, max_steps=200)
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(v), st)
    path = str(tmp_path / "iqnd.npz")
    v.save(path)
    z = np.load(path)
    assert str(z["head"][0]) == "iqn" and int(z["dueling"][0]) == 1 and int(z["prioritized"][0]) == int(prioritized)
    mk = lambda **kw: VecIQN(16, **{**dict(batch=8, fc_width=128, seed=4, capacity=2000, n_step=2, n_tau=4, n_tau_next=5, n_tau_act=6,
                                           prioritized=prioritized, dueling=True), **kw})
    plain = mk(dueling=False)
    with pytest.raises(ValueError, match="written by a VecIQN with a dueling IQN head, this VecIQN has a plain one"):
        plain.load(path)
    other = str(tmp_path / "iqn.npz")
    plain.save(other)
    resumed = mk(lr=3e-5)
    with pytest.raises(ValueError, match="written by a VecIQN with a plain IQN head, this VecIQN has a dueling one"):
        resumed.load(other)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and resumed.double_q and resumed.net.iqn()[4] == 0.5
    more = [resumed.step().clone() for _ in range(4)]
    straight, l11 = run_steps(11, prioritized=prioritized)
    assert all(torch.equal(x, y) for x, y in zip(more, l11[7:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=128)
    assert net.arch == ARCH and torch.equal(net.store_params(), v.net.store_params()) and net.iqn() == (4, 5, 6, 1.0, 0.5)
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    assert qnet_from_checkpoint(other, fc_width=128).arch == "iqn"
    v.run(1, log_every=1)
