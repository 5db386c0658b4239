"""Munchausen IQN on the GPU (include/fbdqn.h, the Munchausen IQN block; kernel: the MU instantiations of csrc/fb_iqn.hip's loss kernel)
against the float64 restatement of tests/test_miqn_host.py.  T is held elementwise to tol_bj = Q_ATOL (4 + S_bj / temp) (that file derives
it: only Q_ATOL, the project's bound on theta and Qbar, enters), the loss to rtol 1e-4 plus atol = mean tol_bj (the loss is 1 / kappa-
Lipschitz in T), the gradients to tests/test_gpu_iqn.py::check_iqn_grads' bounds -- unchanged at temp = 1, with max tol_bj / kappa added
to the atol factor at temp = 0.03.  Then, bit for bit: the hard limit (temp = 1e-6, alpha = 0 == IQN with double_q = 0), the clip at 0,
unit and half weights, ring-fed == gathered, the two loop steps == their separate calls, off == never touched; the refusals; the loop and
its checkpoint.  Every test calls the setter."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_iqn as gi
from tests import test_gpu_iqn_dueling as gd
from tests.test_gpu_ac import net_state, same_state
from tests.test_gpu_iqn import GAMMA, SHAPES, check_iqn_grads, iqn_params, t64
from tests.test_gpu_iqn_per import f32_sum_in_order, grad_buf, leaves, tree_state, twin_memories
from tests.test_gpu_qnet import Q_ATOL
from tests.test_iqn_dueling_host import as_iqn
from tests.test_iqn_host import F32, iqn_bounds, qbar_from_h, theta_from_h, torch_iqn_loss, trunk64
from tests.test_miqn_host import PARAMS, miqn_target64, miqn_tol

pytestmark = pytest.mark.gpu
KAPPA = 1.0
HARD = (1e-6, 0.0, -1.0)                     # (temp, alpha, l0) of the hard limit


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def params_of(oracle, fc, A, seed, dueling):
    return (gd.iqnd_params if dueling else iqn_params)(oracle, fc, A, seed)


_nets, _inputs, _refs = {}, {}, {}


def mcase(oracle, shape, dueling):
    """one net per (shape, kind) for the gradient-exporting tests (they leave the parameters as they were); every test sets the net's
    Munchausen setting itself"""
    from dqnflappybird_amd.vec import QNet
    fc, A, N, Np, K = shape
    if (shape, dueling) not in _nets:
        net = QNet(A, fc, "iqndueling" if dueling else "iqn", max_batch=256, n_tau=N, n_tau_next=Np, n_tau_act=K)
        assert net.iqn_munchausen() == (False, F32(0.03), F32(0.9), -1.0)          # a new net: off, the paper's values
        net.load_params(params_of(oracle, fc, A, 1, dueling), 0)
        net.load_params(params_of(oracle, fc, A, 2, dueling), 1)
        _nets[(shape, dueling)] = net
    return _nets[(shape, dueling)]


def ref_inputs(oracle, shape, B, dueling):
    """the kink-free minibatch of tests/test_gpu_iqn.py::ref_step (the dueling net: tests/test_gpu_iqn_dueling.py's), and in float64 under
    the TARGET parameters: Qbar(s', .) and Qbar(s, .) [B, A], theta(s', c; tau'_j) [B, N', A].  Needs no GPU"""
    import torch
    fc, A, N, Np, K = shape
    if (shape, B, dueling) not in _inputs:
        s, a, r, s2, t, tau, taup, _ = (gd.ref_step if dueling else gi.ref_step)(oracle, shape, B)
        with torch.no_grad():
            PT = t64(params_of(oracle, fc, A, 2, dueling))
            PT = as_iqn(PT, fc, A) if dueling else PT
            h2, hs = trunk64(PT, s2, fc, A), trunk64(PT, s, fc, A)
            qn, qs = qbar_from_h(PT, h2, K, 1.0, fc, A).numpy(), qbar_from_h(PT, hs, K, 1.0, fc, A).numpy()
            th = theta_from_h(PT, h2, taup, fc, A).numpy()
        _inputs[(shape, B, dueling)] = (s, a, r, s2, t, tau, taup, qn, qs, th)
    return _inputs[(shape, B, dueling)]


def ref_miqn(oracle, shape, B, dueling, par):
    """-> (alpha, l0) the case runs with, and the float64 target, tolerance, loss, per-sample loss and gradient of the step.  The issue's
    (alpha, l0) stay unless the stored actions leave every bonus on one side of the clip: then l0 is put half way between the smallest and
    the largest temp ln pi(a_b | s_b) of the batch, from the REFERENCE alone, and the case asserts again that both sides occur"""
    import torch
    fc, A, N, Np, K = shape
    temp, alpha, l0 = par
    key = (shape, B, dueling, par)
    if key not in _refs:
        s, a, r, s2, t, tau, taup, qn, qs, th_all = ref_inputs(oracle, shape, B, dueling)
        x = miqn_target64(qn, qs, th_all, a, r, t, GAMMA, temp, alpha, l0)["x"]
        if B >= 32 and not ((x < l0).any() and (x > l0).any()):
            assert x.min() < x.max() <= 0
            l0 = float(F32(0.5 * (x.min() + x.max())))
        ref = miqn_target64(qn, qs, th_all, a, r, t, GAMMA, temp, alpha, l0)
        if B >= 32:                                                      # what the issue asks of the case
            assert (ref["x"] < l0).any() and (ref["x"] > l0).any() and t.any() and not t.all()
        p = params_of(oracle, fc, A, 1, dueling)
        pg = t64(p).requires_grad_(True)
        q = as_iqn(pg, fc, A) if dueling else pg
        th = theta_from_h(q, trunk64(q, s, fc, A), tau, fc, A)[torch.arange(B), :, torch.as_tensor(a.astype(np.int64))]
        loss, lb = torch_iqn_loss(th, torch.as_tensor(ref["T"]), tau, KAPPA)
        grad, = torch.autograd.grad(loss, pg)
        _refs[key] = (alpha, l0, ref["T"], miqn_tol(ref["S"], temp), loss.item(), lb.detach().numpy(), grad.numpy(), ref)
    return _refs[key]


def check_grads_with(g, g0, bounds, extra):
    """check_iqn_grads' bounds (rtol 2e-3, atol 2e-5 x the tensor's largest reference element) with `extra` added to the atol factor"""
    for name, lo, hi in bounds:
        ref, got = g0[lo:hi], g[lo:hi]
        scale = np.abs(ref).max()
        assert scale > 0, name
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=(2e-5 + extra) * scale, err_msg=name)


def dev(torch):
    return lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ================================================================================================================ 1: float64 autograd
CASES = [(sh, B, False) for sh in SHAPES for B in (1, 32, 255, 256)] + [(sh, B, True) for sh in SHAPES[:2] for B in (1, 32, 255, 256)]


@pytest.mark.parametrize("par", PARAMS)
@pytest.mark.parametrize("shape,B,dueling", CASES)
def test_train_step_against_autograd(torch_cuda, oracle, shape, B, dueling, par):
    """gathered, gradient-exporting: T elementwise, the loss and every gradient tensor; nothing is masked"""
    torch = torch_cuda
    fc, A, N, Np, K = shape
    temp = par[0]
    net = mcase(oracle, shape, dueling)
    s, a, r, s2, t, tau, taup = ref_inputs(oracle, shape, B, dueling)[:7]
    alpha, l0, T0, tol, want, _, g0, ref = ref_miqn(oracle, shape, B, dueling, par)
    d = dev(torch)
    net.set_iqn_munchausen(True, temp, alpha, l0)
    assert net.iqn_munchausen() == (True, F32(temp), F32(alpha), F32(l0))
    grad = grad_buf(torch, net)
    loss, T = net.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=grad)
    loss, T = loss.item(), T.cpu().numpy()
    ratio = np.abs(T - T0) / tol
    print(f"miqn {shape} B={B} dueling={dueling} (temp, alpha, l0)=({temp}, {alpha}, {l0}): loss {loss!r} / {want!r}; max |dT| {np.abs(T - T0).max():.3e}, "
          f"largest |dT| / tol {ratio.max():.3e}, tol in [{tol.min():.3e}, {tol.max():.3e}]; bonus clipped on {int((ref['x'] < l0).sum())} of {B}")
    assert (ratio <= 1).all()
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=tol.mean())
    g = grad.cpu().numpy()
    if temp == 1.0:
        (gd.check_grads if dueling else check_iqn_grads)(g, g0, fc, A)
    elif dueling:
        check_grads_with(g, g0, [(n, lo, hi) for n, (lo, hi) in gd.bounds(fc, A).items()], tol.max() / KAPPA)
    else:
        check_grads_with(g, g0, iqn_bounds(fc, A), tol.max() / KAPPA)
    assert np.array_equal(net.store_params(0).cpu().numpy(), params_of(oracle, fc, A, 1, dueling))      # gradient-only mode
    assert net.overflow_count() == 0


# ================================================================================================================ 2: the hard limit
def all_outputs(torch, net, inp, w, **kw):
    d = dev(torch)
    s, a, r, s2, t, tau, taup = inp[:7]
    g = grad_buf(torch, net)
    loss, ae, T = net.iqn_per_train_step(d(s), d(a), d(r), d(s2), d(t), d(w), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g, **kw)
    return loss.clone(), ae.clone(), T.clone(), g


def same_outputs(torch, x, y):
    return all(torch.equal(p, q) for p, q in zip(x, y))


@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_hard_limit_is_iqn_bit_for_bit(torch_cuda, oracle, shape, B, dueling):
    """temp = 1e-6, alpha = 0: every target Qbar gap of ref_step's s' is >= 10 Q_ATOL = 1e-3 >= 104 temp, so pi is exactly one-hot and T,
    the loss, abs_err and the whole flat gradient are those of the IQN step with double_q = 0 (the weighted call, random weights)"""
    torch = torch_cuda
    net = mcase(oracle, shape, dueling)
    inp = ref_inputs(oracle, shape, B, dueling)
    qn = inp[7]
    top = np.sort(qn, 1)
    assert (top[:, -1] - top[:, -2]).min() >= 10 * Q_ATOL and 8 * Q_ATOL >= 104 * HARD[0]      # (the device's Qbar: within Q_ATOL of each entry)
    w = (1.0 - np.random.default_rng(B).random(B)).astype(F32)
    net.set_iqn_munchausen(False)
    hard = all_outputs(torch, net, inp, w, double_q=False)
    net.set_iqn_munchausen(True, *HARD)
    soft = all_outputs(torch, net, inp, w)
    print(f"hard limit {shape} B={B} dueling={dueling}: loss {soft[0].item()!r} / {hard[0].item()!r}, {int((soft[3] != hard[3]).sum())} gradient elements differ, "
          f"{int((soft[2] != hard[2]).sum())} targets differ")
    assert hard[3].abs().max() > 0 and same_outputs(torch, soft, hard)
    net.set_iqn_munchausen(True, 1.0, 0.0, -1.0)                        # ... and a soft policy is another target
    assert not torch.equal(all_outputs(torch, net, inp, w)[2], hard[2])


# ================================================================================================================ 3: the clip at 0
@pytest.mark.parametrize("dueling", [False, True])
def test_clip_at_zero_removes_the_bonus(torch_cuda, oracle, dueling):
    torch = torch_cuda
    shape, B = SHAPES[1], 32
    net = mcase(oracle, shape, dueling)
    inp = ref_inputs(oracle, shape, B, dueling)
    r, t = inp[2], inp[4]
    w = np.ones(B, F32)
    out = {}
    for alpha in (0.9, 0.0):
        net.set_iqn_munchausen(True, 0.03, alpha, 0.0)
        out[alpha] = all_outputs(torch, net, inp, w)
    assert same_outputs(torch, out[0.9], out[0.0]) and out[0.0][3].abs().max() > 0
    net.set_iqn_munchausen(True, 0.03, 0.9, -1.0)                       # with l0 = -1 the bonus is there ...
    T = all_outputs(torch, net, inp, w)[2].cpu().numpy()
    T0 = out[0.0][2].cpu().numpy()
    assert (T <= T0).all() and (T < T0).any()                            # (it is <= 0)
    # ... and on a terminal sample every T_j is the one value (float)(R + bonus)
    x = ref_miqn(oracle, shape, B, dueling, (0.03, 0.9, -1.0))[7]["x"]
    rd = np.where(r == F32(0.1), 0.1, r.astype(np.float64))
    term = np.flatnonzero(t)
    assert len(term) and len(term) < B
    for b in term:
        assert (T[b] == T[b, 0]).all() and (T0[b] == F32(rd[b])).all()
        assert abs(float(T[b, 0]) - (rd[b] + 0.9 * max(x[b], -1.0))) <= 2 * 0.9 * Q_ATOL + 1e-6      # the bonus moves by <= 2 alpha |dq|


# ================================================================================================================ 4: prioritized
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_unit_weights_are_the_uniform_bits_and_half_weights_halve(torch_cuda, oracle, shape):
    """tests/test_gpu_iqn_per.py::test_exact_weights' pattern with the setting on"""
    torch = torch_cuda
    fc, A = shape[:2]
    B = 32
    net = mcase(oracle, shape, False)
    inp = ref_inputs(oracle, shape, B, False)
    s, a, r, s2, t, tau, taup = inp[:7]
    d = dev(torch)
    net.set_iqn_munchausen(True, 0.03, 0.9, -1.0)
    g0 = grad_buf(torch, net)
    l0, T0 = net.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g0)
    l1, ae1, T1, g1 = all_outputs(torch, net, inp, np.ones(B, F32))
    assert torch.equal(l1, l0) and torch.equal(T1, T0) and torch.equal(g1, g0) and g0.abs().max() > 0 and (ae1 > 0).all()
    assert l1.cpu().numpy()[0].view(np.uint32) == (f32_sum_in_order(ae1.cpu().numpy()) / F32(B)).view(np.uint32)
    lh, aeh, Th, gh = all_outputs(torch, net, inp, np.full(B, 0.5, F32))
    assert torch.equal(aeh, ae1) and torch.equal(Th, T1)                # the priorities and T carry no weight
    assert lh.item() == F32(0.5) * F32(l1.item())
    g1, gh = g1.cpu().numpy(), gh.cpu().numpy()
    for name, lo, hi in iqn_bounds(fc, A):
        if name in ("W_q", "b_q", "W_e", "b_e"):
            assert np.abs(g1[lo:hi]).max() > 0 and np.array_equal(gh[lo:hi], F32(0.5) * g1[lo:hi]), name
    check_iqn_grads(gh, 0.5 * g1.astype(np.float64), fc, A)


# ================================================================================================================ 5: ring-fed == gathered
def set_on(nets, par=(0.03, 0.9, -1.0)):
    for n in nets:
        n.set_iqn_munchausen(True, *par)
        assert n.iqn_munchausen()[0] is True
    return nets


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B, n_step):
    """a uniform memory: the target-s slice reads the ring at fshift 0, the s' slice at fshift n"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = gi.ring_pair(torch, oracle, B, 2, n_step)
    set_on(nets)
    g_gath, g_ring = grad_buf(torch, nets[0]), grad_buf(torch, nets[1])
    l_gath, y_gath = nets[0].iqn_train_step(s, a, r, s2, t, gamma=bootstrap_gamma(GAMMA, n_step), seed=5, step=6, flat_grad=g_gath)
    l_ring, a_o, r_o, t_o, y_ring = iqn_train_from_replay(rep, nets[1], idx, gamma=GAMMA, seed=5, step=6, flat_grad=g_ring, want_target=True)
    print(f"miqn ring-fed vs gathered B={B} n_step={n_step}: loss {l_gath.item()!r} / {l_ring.item()!r}, "
          f"{int((g_ring != g_gath).sum())} of {g_gath.numel()} gradient elements differ")
    assert torch.equal(a_o, a) and torch.equal(r_o, r) and torch.equal(t_o, t) and g_gath.abs().max() > 0
    assert torch.equal(l_ring, l_gath) and torch.equal(y_ring, y_gath) and torch.equal(g_ring, g_gath)
    # a fused step of both forms: the parameters, Adam and the folds agree
    l1, _ = nets[0].iqn_train_step(s, a, r, s2, t, gamma=bootstrap_gamma(GAMMA, n_step), seed=5, step=6)
    l2 = iqn_train_from_replay(rep, nets[1], idx, gamma=GAMMA, seed=5, step=6)[0]
    assert torch.equal(l1, l2) and same_state(torch, net_state(nets[0]), net_state(nets[1]))
    assert not np.array_equal(nets[0].store_params(0).cpu().numpy(), p)


def per_net(oracle, max_batch=256):
    from tests.test_gpu_iqn_per import make_net
    return make_net(oracle, max_batch=max_batch)


@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_on_a_prioritized_memory_equals_gathered(torch_cuda, oracle, B, n_step):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_per_train_from_replay
    env, per, _ = twin_memories(torch, 22, n_step)
    assert per.population >= 256
    rng = np.random.default_rng(B + n_step)
    idx = leaves(rng, per, B)
    w = torch.from_numpy((1.0 - rng.random(B)).astype(F32)).cuda()
    s, a, r, s2, t = per.gather(idx)
    n1, n2 = set_on([per_net(oracle), per_net(oracle)])
    g1, g2 = grad_buf(torch, n1), grad_buf(torch, n2)
    G = bootstrap_gamma(GAMMA, n_step)
    kw = dict(seed=5, step=6)
    l1, ae1, y1 = n1.iqn_per_train_step(s, a, r, s2, t, w, gamma=G, flat_grad=g1, **kw)
    l2, a2, r2, t2, y2, ae2 = iqn_per_train_from_replay(per, n2, idx, w, gamma=GAMMA, flat_grad=g2, want_target=True, **kw)
    print(f"miqn per ring-fed vs gathered B={B} n_step={n_step}: loss {l1.item()!r} / {l2.item()!r}, {int((g1 != g2).sum())} gradient elements differ")
    assert torch.equal(a2, a) and torch.equal(r2, r) and torch.equal(t2, t) and g1.abs().max() > 0
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and torch.equal(y1, y2) and torch.equal(g1, g2)
    l1, ae1, _ = n1.iqn_per_train_step(s, a, r, s2, t, w, gamma=G, **kw)
    l2, _, _, _, ae2 = iqn_per_train_from_replay(per, n2, idx, w, gamma=GAMMA, **kw)
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and same_state(torch, net_state(n1), net_state(n2))


# ================================================================================================================ 6: the loop steps
NE, BT = 8, 8


def world(oracle, prioritized, n_step=1):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(NE, seed=5)
    if prioritized:
        rep = VecReplay(2000, NE, prioritized=True, n_step=n_step, gamma=GAMMA)
        rep.seed(7)
    else:
        rep = VecReplay(2000, NE)
        rep.seed(7, "cpython")
        if n_step > 1:
            rep.set_n_step(n_step, GAMMA)
    net = set_on([per_net(oracle, max_batch=NE)])[0]
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


PLAN = [(False, 0.5), (True, 0.3), (True, 0.5), (False, 0.0), (True, 0.1), (True, 1.0)]      # (train, epsilon)


def test_iqn_step_equals_its_separate_calls(torch_cuda, oracle):
    """two identically seeded worlds with the setting on: actions, idx, the loss, a / r / t, both nets and Adam, the envs, the memory"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnStep, iqn_train_from_replay
    seed = (3 << 32) | 9
    e1, r1, n1, nib1 = world(oracle, False)
    e2, r2, n2, nib2 = world(oracle, False)
    one = IqnStep(e1, r1, n1, BT, GAMMA, False)
    for k, (train, eps) in enumerate(PLAN):
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = n2.act_nib(nib2, eps, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        idx = r2.push_sample(e2.frame_bits, a2, rew, term, BT)
        assert torch.equal(a1, a2) and torch.equal(one.idx, idx) and torch.equal(nib1, nib2), k
        if train:
            loss, a_o, r_o, t_o, y = iqn_train_from_replay(r2, n2, idx, gamma=GAMMA, seed=seed, step=k, want_target=True)
            assert torch.equal(one.loss, loss) and torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
            assert torch.isfinite(y).all(), k                            # (the loop step hands out no T: it is held through the loss and the nets)
        assert same_state(torch, net_state(n1), net_state(n2)), k
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob())) and len(r1) == len(PLAN) * NE
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), iqn_params(oracle, 128, 2, 1))
    with pytest.raises(ValueError, match="fb_iqn_step: double_q = 1 on a net with Munchausen on"):
        IqnStep(e1, r1, n1, BT, GAMMA, True)(0.1, seed=seed, step=9, train=True)


@pytest.mark.parametrize("n_step", [1, 2])
def test_iqn_per_step_equals_its_separate_calls(torch_cuda, oracle, n_step):
    """... and on a prioritized memory: idx, isw, loss, abs_err (the priorities), a / r / t, T, both nets and Adam, the envs, the tree"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep, iqn_per_train_from_replay
    seed = (3 << 32) | 9
    e1, r1, n1, nib1 = world(oracle, True, n_step)
    e2, r2, n2, nib2 = world(oracle, True, n_step)
    one = IqnPerStep(e1, r1, n1, BT, GAMMA, False)
    trained = 0
    for k, (train, eps) in enumerate(PLAN):
        train = train and k >= n_step - 1
        a1 = one(eps, seed=seed, step=k, train=train)
        a2 = n2.act_nib(nib2, eps, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        r2.push(e2.frame_bits, a2, rew, term)
        assert torch.equal(a1, a2) and torch.equal(nib1, nib2), k
        if train:
            idx, isw = r2.sample(BT)
            idx, isw = idx.clone(), isw.clone()
            loss, a_o, r_o, t_o, y, ae = iqn_per_train_from_replay(r2, n2, idx, isw.to(torch.float32), gamma=GAMMA, seed=seed, step=k, want_target=True)
            assert torch.equal(one.idx, idx) and torch.equal(one.isw, isw) and torch.equal(one.isw32, isw.to(torch.float32)), k
            assert torch.equal(one.loss, loss) and torch.equal(one.abs_err, ae) and (ae >= 0).all() and torch.isfinite(y).all(), k
            assert torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
            r2.update_priorities(idx, abs_err=ae.clone())
            trained += 1
        assert same_state(torch, net_state(n1), net_state(n2)), k
        x, y = tree_state(r1), tree_state(r2)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], k
    assert trained == 4 and len(r1) == len(PLAN) * NE
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


# ================================================================================================================ 7: off is off
@pytest.mark.parametrize("dueling", [False, True])
def test_off_is_off(torch_cuda, oracle, dueling):
    """a net set on and then off again against a net never touched: T, loss, gradient, then the parameters after a fused step"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    shape, B = SHAPES[0], 32
    fc, A, N, Np, K = shape
    inp = ref_inputs(oracle, shape, B, dueling)
    s, a, r, s2, t, tau, taup = inp[:7]
    d = dev(torch)
    nets = []
    for _ in range(2):
        n = QNet(A, fc, "iqndueling" if dueling else "iqn", max_batch=B, n_tau=N, n_tau_next=Np, n_tau_act=K)
        n.load_params(params_of(oracle, fc, A, 1, dueling), 0); n.load_params(params_of(oracle, fc, A, 2, dueling), 1)
        n.set_hparams(lr=1e-4)
        nets.append(n)
    nets[0].set_iqn_munchausen(True, 0.5, 0.25, -2.0)
    g = grad_buf(torch, nets[0])
    _, T_on = nets[0].iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g)
    T_on = T_on.clone()
    nets[1].iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup), flat_grad=g)      # (as many exporting steps on both)
    nets[0].set_iqn_munchausen(False, 0.5, 0.25, -2.0)
    assert nets[0].iqn_munchausen() == (False, 0.5, 0.25, -2.0) and nets[1].iqn_munchausen()[0] is False
    for dq in (False, True):                                             # (off: double_q is taken again)
        out = []
        for n in nets:
            g = grad_buf(torch, n)
            loss, T = n.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, double_q=dq, tau=d(tau), tau_next=d(taup), flat_grad=g)
            out.append((loss.clone(), T.clone(), g))
        assert same_outputs(torch, out[0], out[1]) and out[0][2].abs().max() > 0
        assert not torch.equal(out[0][1], T_on)
    for n in nets:
        n.iqn_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, tau=d(tau), tau_next=d(taup))
    assert same_state(torch, net_state(nets[0]), net_state(nets[1]))
    assert not np.array_equal(nets[0].store_params(0).cpu().numpy(), params_of(oracle, fc, A, 1, dueling))


# ================================================================================================================ 8: refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import IqnPerStep, IqnStep, QNet, iqn_per_train_from_replay, iqn_train_from_replay
    from tests.test_gpu_iqn_per import BATCH as B, NENV
    lib = L.lib()
    env, per, uni = twin_memories(torch, 6)
    env.track_state()
    iqn = set_on([per_net(oracle, max_batch=32)], (0.5, 0.25, -2.0))[0]
    blobs = [np.asarray(m.state_blob()).copy() for m in (per, uni)]
    sizes = [len(m) for m in (per, uni)]
    before, envs = net_state(iqn), env.get_state().copy()

    def untouched():
        torch.cuda.synchronize()
        return (all(np.array_equal(np.asarray(m.state_blob()), b) for m, b in zip((per, uni), blobs)) and [len(m) for m in (per, uni)] == sizes
                and same_state(torch, net_state(iqn), before) and np.array_equal(env.get_state(), envs)
                and iqn.iqn_munchausen() == (True, 0.5, 0.25, -2.0))

    idx = leaves(np.random.default_rng(0), per, B)
    pos = idx - (per.capacity - 1)
    s, a, r, s2, t = per.gather(idx)
    w = torch.ones(B, dtype=torch.float32, device="cuda")
    ae = torch.zeros(B, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    a_o, t_o = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    r_o = torch.zeros(B, dtype=torch.float32, device="cuda")
    fails = lambda rc, *words: rc == -1 and all(x in lib.fb_last_error().decode() for x in words)
    su, sp = IqnStep(env, uni, iqn, B, GAMMA), IqnPerStep(env, per, iqn, B, GAMMA)
    six = {
        "fb_qnet_iqn_train_step": lambda dq: lib.fb_qnet_iqn_train_step(iqn.h, dq, B, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t), None, None, 0, 0, 0.99,
                                                                        L.ptr(loss), None, None, None),
        "fb_iqn_train_from_replay": lambda dq: lib.fb_iqn_train_from_replay(uni.h, iqn.h, dq, B, L.ptr(pos), L.ptr(a_o), L.ptr(r_o), L.ptr(t_o), None, None, 0, 0,
                                                                            GAMMA, L.ptr(loss), None, None, None),
        "fb_iqn_step": lambda dq: lib.fb_iqn_step(env.h, uni.h, iqn.h, C.byref(su.buf), NENV, dq, B, C.c_float(0.1), 0, 0, 1, GAMMA, None),
        "fb_qnet_iqn_per_train_step": lambda dq: lib.fb_qnet_iqn_per_train_step(iqn.h, dq, B, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t), L.ptr(w), None, None,
                                                                                0, 0, 0.99, L.ptr(loss), L.ptr(ae), None, None, None),
        "fb_iqn_per_train_from_replay": lambda dq: lib.fb_iqn_per_train_from_replay(per.h, iqn.h, dq, B, L.ptr(idx), L.ptr(w), L.ptr(a_o), L.ptr(r_o), L.ptr(t_o),
                                                                                    None, None, 0, 0, GAMMA, L.ptr(loss), L.ptr(ae), None, None, None),
        "fb_iqn_per_step": lambda dq: lib.fb_iqn_per_step(env.h, per.h, iqn.h, C.byref(sp.buf), NENV, dq, B, C.c_float(0.1), 0, 0, 1, GAMMA, None),
    }
    # on + double_q = 1 through all six training entry points: FB_ERR_INVALID, a message that names both
    for who, call in six.items():
        assert fails(call(1), who + ": double_q = 1", "Munchausen on (fb_qnet_set_iqn_munchausen)"), who
    assert untouched()
    for call in (lambda: iqn.iqn_train_step(s, a, r, s2, t, double_q=True), lambda: iqn_train_from_replay(uni, iqn, pos, gamma=GAMMA, double_q=True),
                 lambda: iqn.iqn_per_train_step(s, a, r, s2, t, w, double_q=True),
                 lambda: iqn_per_train_from_replay(per, iqn, idx, w, gamma=GAMMA, double_q=True),
                 lambda: IqnStep(env, uni, iqn, B, GAMMA, True)(0.1), lambda: IqnPerStep(env, per, iqn, B, GAMMA, True)(0.1)):
        with pytest.raises(ValueError, match="double_q = 1 on a net with Munchausen on"):
            call()
    assert untouched()
    # out-of-range temp / alpha / clip / on: nothing changes
    nan, inf = float("nan"), float("inf")
    for on, temp, alpha, clip, word in ((1, 0.0, 0.9, -1.0, "temp must be finite and > 0"), (1, -1.0, 0.9, -1.0, "temp must be"), (1, nan, 0.9, -1.0, "temp must be"),
                                        (0, inf, 0.9, -1.0, "temp must be"), (1, 0.03, 1.5, -1.0, "alpha must be in [0, 1]"), (1, 0.03, -0.1, -1.0, "alpha must be"),
                                        (1, 0.03, nan, -1.0, "alpha must be"), (1, 0.03, 0.9, 0.5, "the clip l0 must be finite and <= 0"),
                                        (0, 0.03, 0.9, -inf, "the clip l0 must be"), (1, 0.03, 0.9, nan, "the clip l0 must be"), (2, 0.03, 0.9, -1.0, "on must be 0 or 1"),
                                        (-1, 0.03, 0.9, -1.0, "on must be 0 or 1")):
        assert fails(lib.fb_qnet_set_iqn_munchausen(iqn.h, on, C.c_float(temp), C.c_float(alpha), C.c_float(clip)), "fb_qnet_set_iqn_munchausen: " + word)
    assert lib.fb_qnet_set_iqn_munchausen(None, 1, C.c_float(0.03), C.c_float(0.9), C.c_float(-1)) == -1
    assert lib.fb_qnet_get_iqn_munchausen(None, None, None, None, None) == -1
    for bad in (1, 0, None, "on"):
        with pytest.raises(ValueError, match="on must be True or False"):
            iqn.set_iqn_munchausen(bad)
    assert untouched()
    # fb_qnet_set_munchausen / _get_munchausen on an IQN net: still refused, word for word
    assert fails(lib.fb_qnet_set_munchausen(iqn.h, C.c_float(0.03), C.c_float(0.9), C.c_float(-1)),
                 "fb_qnet_set_munchausen: Munchausen-DQN trains the scalar Q heads only, not an IQN net (its loss has its own kappa)")
    assert fails(lib.fb_qnet_get_munchausen(iqn.h, None, None, None),
                 "fb_qnet_get_munchausen: Munchausen-DQN trains the scalar Q heads only, not an IQN net (its loss has its own kappa)")
    assert untouched()
    # the setter and the getter on every net that is not an IQN net
    for arch in ("plain", "dueling", "c51", "qr", "ac", "sac"):
        q = QNet(2, 128, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        md = q.munchausen() if arch in ("plain", "dueling") else None
        assert fails(lib.fb_qnet_set_iqn_munchausen(q.h, 1, C.c_float(0.03), C.c_float(0.9), C.c_float(-1)), "fb_qnet_set_iqn_munchausen: not an IQN net"), arch
        assert fails(lib.fb_qnet_get_iqn_munchausen(q.h, None, None, None, None), "fb_qnet_get_iqn_munchausen: not an IQN net"), arch
        for call in (lambda: q.set_iqn_munchausen(True), lambda: q.iqn_munchausen()):
            with pytest.raises(ValueError, match="needs an IQN net"):
                call()
        assert same_state(torch, net_state(q), qb) and (md is None or q.munchausen() == md), arch
    assert untouched()
    # the refusals were about the arguments: the same handles take the calls with double_q = 0
    for who, call in six.items():
        assert call(0) == 0, who
    torch.cuda.synchronize()
    assert not same_state(torch, net_state(iqn), before) and len(uni) == sizes[1] + NENV and len(per) == sizes[0] + NENV


# ================================================================================================================ 9: the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.veciqn import VecIQN
    kw = {**dict(munchausen=True, temp=0.05, alpha=0.8, clip=-0.5), **kw}
    v = VecIQN(8, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, lr=1e-4, initial_epsilon=0.5, explore=200, n_step=2, replace_target_iter=3,
               max_grad_norm=5.0, cvar=0.5, n_tau=4, n_tau_next=5, n_tau_act=6, **kw)
    return v, [v.step().clone() for _ in range(n)]


@pytest.mark.parametrize("prioritized,dueling", [(False, False), (True, True)])
def test_vec_iqn_munchausen_loop_and_checkpoint(torch_cuda, tmp_path, prioritized, dueling):
    torch = torch_cuda
    from dqnflappybird_amd.veciqn import VecIQN
    from tests.test_gpu_iqn_per import loop_state as per_state, same_loop as per_same
    state, same = (per_state, per_same) if prioritized else (gi.loop_state, gi.same_loop)
    kind = dict(prioritized=prioritized, dueling=dueling)
    v, losses = run_steps(200, **kind)
    assert not losses[2].any() and all(torch.isfinite(l).all() for l in losses) and losses[199][0] > 0
    assert v.timeStep == 200 and v.net.iqn_munchausen() == (True, F32(0.05), F32(0.8), -0.5) and v.munchausen and not v.double_q
    off, l_off = run_steps(8, munchausen=False, **kind)                  # the hard target trains something else
    assert off.net.iqn_munchausen()[0] is False and not all(torch.equal(x, y) for x, y in zip(losses[:8], l_off))
    st = state(v)
    res = v.evaluate(n_envs=32, episodes=1, max_steps=200)               # evaluate() leaves the training state untouched
    assert res.score.shape == (32, 1) and same(torch, state(v), st)
    path = str(tmp_path / "miqn.npz")
    v.save(path)
    assert np.load(path)["munchausen"].tolist() == [1.0, float(F32(0.05)), float(F32(0.8)), -0.5]
    mk = lambda **kw: VecIQN(8, **{**dict(batch=8, fc_width=128, seed=4, capacity=2000, n_step=2, n_tau=4, n_tau_next=5, n_tau_act=6, munchausen=True, temp=0.05,
                                          alpha=0.8, clip=-0.5), **kind, **kw})
    with pytest.raises(ValueError, match="with the Munchausen target, this VecIQN has the hard one \\(munchausen=False\\)"):
        mk(munchausen=False).load(path)
    with pytest.raises(ValueError, match="was trained with munchausen \\(temp, alpha, clip\\)"):
        mk(temp=0.03).load(path)
    resumed = mk(lr=3e-5)
    resumed.load(path)
    assert same(torch, state(resumed), st) and resumed.net.iqn_munchausen() == v.net.iqn_munchausen()
    more = [resumed.step().clone() for _ in range(4)]
    straight, l204 = run_steps(204, **kind)
    assert all(torch.equal(x, y) for x, y in zip(more, l204[200:])) and same(torch, state(resumed), state(straight))
    # a checkpoint without the key loads as off; one of the hard target is refused by a Munchausen loop, by name
    old = str(tmp_path / "old.npz")
    off.save(old)
    z = dict(np.load(old))
    assert z.pop("munchausen").tolist()[0] == 0.0
    np.savez(old, **z)
    plain = mk(munchausen=False)
    plain.load(old)
    assert plain.net.iqn_munchausen()[0] is False and same(torch, state(plain), state(off))
    with pytest.raises(ValueError, match="with the hard target, this VecIQN has the Munchausen one \\(munchausen=True\\)"):
        resumed.load(old)
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=128)                      # evaluate.py ignores the key: greedy play is unchanged
    assert torch.equal(net.store_params(), v.net.store_params()) and net.iqn_munchausen()[0] is False
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
