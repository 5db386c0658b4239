"""Prioritized IQN on the GPU (include/fbdqn.h, the prioritized IQN block; csrc/fb_iqn.hip: iqn_loss_kernel<.., true>) under the bounds of
tests/test_gpu_iqn.py -- Q_ATOL on T, rtol 1e-4 / atol 1e-6 on the loss and on abs_err, rtol 2e-3 / atol 2e-5 x the tensor's scale per
gradient tensor -- and, where the header promises bits, bit for bit: unit weights == the uniform calls, the exact weights 0 and 0.5,
ring-fed == gathered on a prioritized memory, fb_iqn_per_step == its separate calls, the leaves Memory.batch_update leaves, every
refusal, and the VecIQN(prioritized=True) loop with its checkpoint.  fc_width 128, 16 envs, capacity 2000, N = 4, N' = 5, batch 8
unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests.test_c51_per_host import np_priority
from tests.test_gpu_ac import net_state, same_state
from tests.test_gpu_iqn import GAMMA, check_iqn_grads, iqn_params, ref_step, t64
from tests.test_gpu_nstep_per import heaps
from tests.test_gpu_qnet import Q_ATOL
from tests.test_iqn_host import F32, iqn_bounds, theta_from_h, trunk64
from tests.test_iqn_per_host import torch_iqn_per_loss

pytestmark = pytest.mark.gpu
FC, NENV, CAP, NT, NTP, KACT, BATCH = 128, 16, 2000, 4, 5, 6, 8
FB_ERR_STATE = -4                            # include/fbdqn.h


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_net(oracle, A=2, max_batch=32, lr=1e-4):
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, FC, "iqn", max_batch=max_batch, n_tau=NT, n_tau_next=NTP, n_tau_act=KACT)
    net.load_params(iqn_params(oracle, FC, A, 1), 0)
    net.load_params(iqn_params(oracle, FC, A, 2), 1)
    net.set_hparams(lr=lr)
    return net


def twin_memories(torch, pushes, n_step=1, seed=3):
    """a prioritized and a uniform memory that received the same pushes of a played env (no wrap: leaf cap - 1 + d is deque position d)"""
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(NENV, seed=seed)
    per = VecReplay(CAP, NENV, prioritized=True, n_step=n_step, gamma=GAMMA)
    uni = VecReplay(CAP, NENV)
    per.seed(9, "numpy"); uni.seed(9, "cpython")
    env.observe(); per.reset(env.frame_bits); uni.reset(env.frame_bits)
    if n_step > 1:
        uni.set_n_step(n_step, GAMMA)
    g = torch.Generator(device="cpu").manual_seed(pushes + n_step)
    for _ in range(pushes):
        a = (torch.rand(NENV, generator=g) < 0.3).to(torch.uint8).cuda()
        env.frame_step(a, want_u8=False)
        per.push(env.frame_bits, a, env.reward, env.terminal)
        uni.push(env.frame_bits, a, env.reward, env.terminal)
    assert per.population == (pushes - n_step + 1) * NENV == uni.population < CAP
    return env, per, uni


def leaves(rng, per, B):
    import torch
    return torch.from_numpy((rng.permutation(per.population)[:B] + per.capacity - 1).astype(np.int64)).cuda()


def grad_buf(torch, net):
    return torch.zeros(net.n_params, dtype=torch.float32, device="cuda")


def f32_sum_in_order(x):
    t = F32(0)
    for v in np.asarray(x, F32):
        t = F32(t + v)
    return t


# ================================================================================================================ 1: w = 1
@pytest.mark.parametrize("n_step", [1, 3])
def test_unit_weights_are_the_uniform_calls_bit_for_bit(torch_cuda, oracle, n_step):
    """the gathered and the ring-fed _per call with w = 1 against the two uniform calls on the same transitions: loss, T, flat gradient"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_per_train_from_replay, iqn_train_from_replay
    B = BATCH
    env, per, uni = twin_memories(torch, 6, n_step)
    idx = leaves(np.random.default_rng(n_step), per, B)
    pos = idx - (per.capacity - 1)
    s, a, r, s2, t = (x.clone() for x in per.gather(idx))
    su = uni.gather(pos)
    assert all(torch.equal(x, y) for x, y in zip((s, a, r, s2, t), su))          # the same transitions
    ones = torch.ones(B, dtype=torch.float32, device="cuda")
    net = make_net(oracle)
    G = bootstrap_gamma(GAMMA, n_step)
    for dq in (False, True):
        g = [grad_buf(torch, net) for _ in range(4)]
        kw = dict(double_q=dq, seed=5, step=6)
        l0, y0 = net.iqn_train_step(s, a, r, s2, t, gamma=G, flat_grad=g[0], **kw)
        l1, _, _, _, y1 = iqn_train_from_replay(uni, net, pos, gamma=GAMMA, flat_grad=g[1], want_target=True, **kw)
        l2, ae2, y2 = net.iqn_per_train_step(s, a, r, s2, t, ones, gamma=G, flat_grad=g[2], **kw)
        l3, a3, r3, t3, y3, ae3 = iqn_per_train_from_replay(per, net, idx, ones, gamma=GAMMA, flat_grad=g[3], want_target=True, **kw)
        assert g[0].abs().max() > 0 and torch.equal(l0, l1) and torch.equal(g[0], g[1])
        for l, y, gg, ae in ((l2, y2, g[2], ae2), (l3, y3, g[3], ae3)):
            print(f"w = 1, n_step={n_step} double_q={dq}: loss {l.item()!r} / {l0.item()!r}, {int((gg != g[0]).sum())} gradient elements differ")
            assert torch.equal(l, l0) and torch.equal(y, y0) and torch.equal(gg, g[0])
            assert (ae >= 0).all() and ae.max() > 0
            assert l.cpu().numpy()[0].view(np.uint32) == (f32_sum_in_order(ae.cpu().numpy()) / F32(B)).view(np.uint32)
        assert torch.equal(ae2, ae3) and torch.equal(a3, a) and torch.equal(r3, r) and torch.equal(t3, t)
    assert np.array_equal(net.store_params(0).cpu().numpy(), iqn_params(oracle, FC, 2, 1))      # gradient-only mode


# ================================================================================================================ 2: autograd
_wref = {}


def ref_per_step(oracle, A, B):
    """tests/test_gpu_iqn.py::ref_step's kink-free inputs and float64 targets, weights in (0, 1] (both ends of the range among them), and
    the float64 weighted loss, l_b and gradient for double_q = 0 and 1; computed once per (A, B)"""
    import torch
    shape = (FC, A, NT, NTP, KACT)
    if (A, B) not in _wref:
        s, a, r, s2, t, tau, taup, out = ref_step(oracle, shape, B)
        rng = np.random.default_rng(100 * A + B)
        w = (1.0 - rng.random(B)).astype(F32)
        w[0], w[1] = 1.0, F32(2.0 ** -10)
        pg = t64(iqn_params(oracle, FC, A, 1)).requires_grad_(True)
        th = theta_from_h(pg, trunk64(pg, s, FC, A), tau, FC, A)[torch.arange(B), :, torch.as_tensor(a.astype(np.int64))]
        res = {}
        for dq in (0, 1):
            T0 = out[dq][1]
            loss, lb = torch_iqn_per_loss(th, torch.as_tensor(T0), tau, 1.0, w)
            grad, = torch.autograd.grad(loss, pg, retain_graph=dq == 0)
            res[dq] = (loss.item(), lb.detach().numpy(), T0, grad.numpy())
        _wref[(A, B)] = (s, a, r, s2, t, tau, taup, w, res)
    return _wref[(A, B)]


@pytest.mark.parametrize("double_q", [0, 1])
@pytest.mark.parametrize("B", [8, 32])
@pytest.mark.parametrize("A", [2, 5])
def test_weighted_step_against_autograd(torch_cuda, oracle, A, B, double_q):
    """random w in (0, 1]: the loss, abs_err (= l_b, unweighted), T and every gradient tensor; nothing is masked"""
    torch = torch_cuda
    s, a, r, s2, t, tau, taup, w, res = ref_per_step(oracle, A, B)
    want, lb0, T0, g0 = res[double_q]
    net = make_net(oracle, A)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = grad_buf(torch, net)
    loss, ae, T = net.iqn_per_train_step(d(s), d(a), d(r), d(s2), d(t), d(w), gamma=GAMMA, double_q=bool(double_q), tau=d(tau), tau_next=d(taup),
                                         flat_grad=grad)
    loss, ae, T = loss.item(), ae.cpu().numpy(), T.cpu().numpy()
    print(f"iqn per A={A} B={B} double_q={double_q}: loss {loss!r} / {want!r}; max |dT| {np.abs(T - T0).max():.3e}; "
          f"max |d abs_err| {np.abs(ae - lb0).max():.3e} at max l_b {lb0.max():.3e}")
    np.testing.assert_allclose(T, T0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ae, lb0, rtol=1e-4, atol=1e-6)
    assert (ae >= 0).all()
    check_iqn_grads(grad.cpu().numpy(), g0, FC, A)
    assert np.array_equal(net.store_params(0).cpu().numpy(), iqn_params(oracle, FC, A, 1))


# ================================================================================================================ 3: exact weights
@pytest.mark.parametrize("A", [2, 5])
def test_exact_weights(torch_cuda, oracle, A):
    """w = 0: loss 0 and an all-zero gradient, abs_err still the w = 1 values.  w = 0.5: the loss and the gradients of W_q, b_q, W_e, b_e
    are exactly half the w = 1 results (a power of two commutes with every fp32 operation of the two IQN kernels); the trunk and fc1
    tensors pass through the f16-plane backward and are held to the gradient tolerance"""
    torch = torch_cuda
    B = BATCH
    s, a, r, s2, t, tau, taup, _, _ = ref_per_step(oracle, A, B)
    net = make_net(oracle, A)
    d = lambda x: torch.from_numpy(x).cuda()
    out = {}
    for w in (1.0, 0.5, 0.0):
        g = grad_buf(torch, net)
        loss, ae, T = net.iqn_per_train_step(d(s), d(a), d(r), d(s2), d(t), torch.full((B,), w, dtype=torch.float32, device="cuda"), gamma=GAMMA,
                                             double_q=True, tau=d(tau), tau_next=d(taup), flat_grad=g)
        out[w] = (loss.cpu().numpy(), ae.cpu().numpy(), T.cpu().numpy(), g.cpu().numpy())
    l1, ae1, T1, g1 = out[1.0]
    assert l1[0] > 0 and np.abs(g1).max() > 0 and (ae1 > 0).all()
    for w in (0.5, 0.0):
        assert np.array_equal(out[w][1], ae1) and np.array_equal(out[w][2], T1), w        # the priorities and T carry no weight
    assert out[0.0][0][0] == 0 and not out[0.0][3].any()
    lh, _, _, gh = out[0.5]
    assert lh[0] == F32(0.5) * l1[0]
    for name, lo, hi in iqn_bounds(FC, A):
        if name in ("W_q", "b_q", "W_e", "b_e"):
            assert np.abs(g1[lo:hi]).max() > 0 and np.array_equal(gh[lo:hi], F32(0.5) * g1[lo:hi]), name
    check_iqn_grads(gh, 0.5 * g1.astype(np.float64), FC, A)


# ================================================================================================================ 4: ring-fed == gathered
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_on_a_prioritized_memory_equals_gathered(torch_cuda, oracle, B, n_step):
    """fb_iqn_per_train_from_replay at SumTree leaves == fb_replay_gather + fb_qnet_iqn_per_train_step (given Gamma = gamma^n): a / r / t,
    loss, abs_err, T, the exported gradient, then the parameters after a fused step, bit for bit"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, iqn_per_train_from_replay
    env, per, _ = twin_memories(torch, 22, n_step)
    assert per.population >= 256
    rng = np.random.default_rng(B + n_step)
    idx = leaves(rng, per, B)
    w = torch.from_numpy((1.0 - rng.random(B)).astype(F32)).cuda()
    s, a, r, s2, t = per.gather(idx)
    n1, n2 = make_net(oracle, max_batch=256), make_net(oracle, max_batch=256)
    g1, g2 = grad_buf(torch, n1), grad_buf(torch, n2)
    G = bootstrap_gamma(GAMMA, n_step)
    kw = dict(double_q=True, seed=5, step=6)
    l1, ae1, y1 = n1.iqn_per_train_step(s, a, r, s2, t, w, gamma=G, flat_grad=g1, **kw)
    l2, a2, r2, t2, y2, ae2 = iqn_per_train_from_replay(per, n2, idx, w, gamma=GAMMA, flat_grad=g2, want_target=True, **kw)
    print(f"per ring-fed vs gathered B={B} n_step={n_step}: loss {l1.item()!r} / {l2.item()!r}, {int((g1 != g2).sum())} gradient elements differ")
    assert torch.equal(a2, a) and torch.equal(r2, r) and torch.equal(t2, t) and g1.abs().max() > 0
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and torch.equal(y1, y2) and torch.equal(g1, g2)
    l1, ae1, _ = n1.iqn_per_train_step(s, a, r, s2, t, w, gamma=G, **kw)
    l2, _, _, _, ae2 = iqn_per_train_from_replay(per, n2, idx, w, gamma=GAMMA, **kw)
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and same_state(torch, net_state(n1), net_state(n2))
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), iqn_params(oracle, FC, 2, 1))


# ================================================================================================================ 5, 6: the loop step
def world(oracle, n_step, trained=True):
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay
    env = VecGameState(NENV, seed=5)
    rep = VecReplay(CAP, NENV, prioritized=True, n_step=n_step, gamma=GAMMA)
    rep.seed(7)
    if trained:
        net = make_net(oracle, max_batch=NENV)
    else:                                                            # the library's own initialisation: small losses, under the priority clip
        net = QNet(2, FC, "iqn", max_batch=NENV, n_tau=NT, n_tau_next=NTP, n_tau_act=KACT)
        net.init_params(3, which=0); net.init_params(4, which=1)
        net.set_hparams(lr=1e-4)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


def tree_state(rep):
    tree, ptr, size, beta = rep.per_state()
    return tree.view(np.uint64).copy(), ptr, size, beta


@pytest.mark.parametrize("n_step", [1, 2])
def test_iqn_per_step_equals_its_separate_calls(torch_cuda, oracle, n_step):
    """two identically seeded worlds, 6 steps: actions, idx, isw, loss, abs_err, a / r / t, both nets and Adam, the envs, per_state() (tree
    bytes, pointer, size, beta) and the memory's whole blob"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep, iqn_per_train_from_replay
    seed = (3 << 32) | 9
    e1, r1, n1, nib1 = world(oracle, n_step)
    e2, r2, n2, nib2 = world(oracle, n_step)
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
            assert torch.equal(one.loss, loss) and torch.equal(one.abs_err, ae) and (ae >= 0).all(), k      # l_b as the loss left it
            assert torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
            r2.update_priorities(idx, abs_err=ae.clone())
            trained += 1
        assert same_state(torch, net_state(n1), net_state(n2)), k
        x, y = tree_state(r1), tree_state(r2)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], k
    assert trained == 4 and len(r1) == 6 * NENV
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), iqn_params(oracle, FC, 2, 1))


def test_priorities_reach_the_tree(torch_cuda, oracle):
    """after a step the leaf of every sampled transition holds min(l_b + 0.01, 1)^0.6 of the abs_err the step left (the last write of a
    leaf drawn twice), as tests/test_gpu_c51_per.py checks its leaves"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep
    env, rep, net, _ = world(oracle, 1, trained=False)
    one = IqnPerStep(env, rep, net, BATCH, GAMMA, True)
    under = 0
    for step in range(4):
        one(0.05, seed=1, step=step, train=True)
        torch.cuda.synchronize()
        tree = heaps(rep)[0]
        want = {}
        for i, l in zip(one.idx.cpu().tolist(), one.abs_err.cpu().numpy()):
            want[i] = np_priority(l)
        np.testing.assert_allclose(tree[list(want)], np.array(list(want.values()), np.float64), rtol=1e-6, atol=0)
        under += int((np.array(list(want.values())) < 1.0).sum())
    assert under > 0


# ================================================================================================================ 7: refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import IqnPerStep, IqnStep, QNet, VecReplay, iqn_per_train_from_replay, iqn_train_from_replay
    lib = L.lib()
    B = BATCH
    env, per, uni = twin_memories(torch, 6)
    env.track_state()
    iqn = make_net(oracle)
    plain = QNet(2, FC, "plain", max_batch=32)
    plain.init_params(1); plain.init_params(2, which=1)
    per3 = VecReplay(CAP, NENV, prioritized=True, n_step=3, gamma=GAMMA)           # an n-step prioritized memory, its tree still empty
    per3.seed(9); per3.reset(env.frame_bits)
    blobs = [np.asarray(m.state_blob()).copy() for m in (per, uni, per3)]
    sizes = [len(m) for m in (per, uni, per3)]
    nets, envs = [net_state(iqn), net_state(plain)], env.get_state().copy()

    def untouched():
        torch.cuda.synchronize()
        return (all(np.array_equal(np.asarray(m.state_blob()), b) for m, b in zip((per, uni, per3), blobs)) and [len(m) for m in (per, uni, per3)] == sizes
                and same_state(torch, net_state(iqn), nets[0]) and same_state(torch, net_state(plain), nets[1]) and np.array_equal(env.get_state(), envs))

    idx = leaves(np.random.default_rng(0), per, B)
    s, a, r, s2, t = per.gather(idx)
    w = torch.ones(B, dtype=torch.float32, device="cuda")
    ae = torch.zeros(B, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    a_o, t_o = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    r_o = torch.zeros(B, dtype=torch.float32, device="cuda")
    fails = lambda rc, word, code=-1: rc == code and word in lib.fb_last_error().decode()
    ts = lambda net, Bn=B, dq=0, g=0.99, isw=w, err=ae: lib.fb_qnet_iqn_per_train_step(net.h, dq, Bn, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t), L.ptr(isw),
                                                                                      None, None, 0, 0, g, L.ptr(loss), L.ptr(err), None, None, None)
    tr = lambda rp, net, Bn=B, dq=0, g=0.99, isw=w, err=ae: lib.fb_iqn_per_train_from_replay(rp.h, net.h, dq, Bn, L.ptr(idx), L.ptr(isw), L.ptr(a_o), L.ptr(r_o),
                                                                                            L.ptr(t_o), None, None, 0, 0, g, L.ptr(loss), L.ptr(err), None, None, None)
    sb = IqnPerStep(env, per, iqn, B, GAMMA)
    st = lambda rp, net, n=NENV, Bn=B, dq=0, g=GAMMA, buf=sb.buf, train=1: lib.fb_iqn_per_step(env.h, rp.h, net.h, C.byref(buf), n, dq, Bn, C.c_float(0.1), 0, 0,
                                                                                              train, g, None)
    # a uniform memory
    assert fails(tr(uni, iqn), "fb_iqn_per_train_from_replay: trains from a prioritized memory only")
    for train in (0, 1):
        assert fails(st(uni, iqn, train=train), "fb_iqn_per_step: trains from a prioritized memory only")
    with pytest.raises(ValueError, match="iqn_per_train_from_replay trains from a prioritized memory only"):
        iqn_per_train_from_replay(uni, iqn, idx, w)
    with pytest.raises(ValueError, match="IqnPerStep trains from a prioritized memory only"):
        IqnPerStep(env, uni, iqn, B)
    # ... and the uniform calls keep refusing a prioritized one, with the words they had
    with pytest.raises(ValueError, match="uniform memory only"):
        iqn_train_from_replay(per, iqn, idx)
    with pytest.raises(ValueError, match="uniform memory only"):
        IqnStep(env, per, iqn, B)
    assert fails(lib.fb_iqn_train_from_replay(per.h, iqn.h, 0, B, L.ptr(idx), L.ptr(a_o), L.ptr(r_o), L.ptr(t_o), None, None, 0, 0, 0.99, L.ptr(loss), None,
                                              None, None), "IQN trains from a uniform memory only (prioritized replay is not offered)")
    assert fails(lib.fb_iqn_step(env.h, per.h, iqn.h, C.byref(sb.buf), NENV, 0, B, C.c_float(0.1), 0, 0, 1, 0.99, None), "uniform memory only")
    # a net that is not an IQN net
    for rc in (lambda: ts(plain), lambda: tr(per, plain), lambda: st(per, plain)):
        assert fails(rc(), "not an IQN net (fb_qnet_create_iqn)")
    for call in (lambda: plain.iqn_per_train_step(s, a, r, s2, t, w), lambda: iqn_per_train_from_replay(per, plain, idx, w),
                 lambda: IqnPerStep(env, per, plain, B)):
        with pytest.raises(ValueError, match="needs an IQN net"):
            call()
    # NULL isw / abs_err; a training step without one of the three buffers (a store-only step needs none of them: checked below)
    assert fails(ts(iqn, isw=None), "needs the importance weights") and fails(ts(iqn, err=None), "needs the importance weights")
    assert fails(tr(per, iqn, isw=None), "needs the importance weights") and fails(tr(per, iqn, err=None), "needs the importance weights")
    for field in ("isw", "isw32", "abs_err"):
        buf = L.StepBuffers()
        C.memmove(C.byref(buf), C.byref(sb.buf), C.sizeof(buf))
        setattr(buf, field, None)
        assert fails(st(per, iqn, buf=buf), "needs the isw / isw32 / abs_err buffers"), field
    for bad in (None, w[:4], w.double(), w.view(B, 1)):
        with pytest.raises(ValueError, match="isw must be a contiguous float32"):
            iqn.iqn_per_train_step(s, a, r, s2, t, bad)
        with pytest.raises(ValueError, match="isw must be a contiguous float32"):
            iqn_per_train_from_replay(per, iqn, idx, bad)
    # the batch, double_q and gamma rules of fb_qnet_iqn_check_train
    for call in (ts, lambda net, **kw: tr(per, net, **kw), lambda net, **kw: st(per, net, **kw)):
        assert fails(call(iqn, Bn=33), "exceeds min(max_batch, 256)") and call(iqn, Bn=0) == -1
        assert fails(call(iqn, g=1.5), "gamma must be in [0, 1]") and fails(call(iqn, dq=2), "double_q must be 0 or 1")
    # an n-step prioritized memory: the memory's gamma; FB_ERR_STATE while its tree is empty (a store-only step is no refusal)
    assert fails(tr(per3, iqn, g=0.9), "fb_iqn_per_train_from_replay: gamma 0.9") and fails(st(per3, iqn, g=0.9), "fb_iqn_per_step: gamma 0.9")
    assert fails(tr(per3, iqn, g=GAMMA), "holds no complete transition", FB_ERR_STATE)
    assert fails(st(per3, iqn, g=GAMMA), "holds no complete transition", FB_ERR_STATE)
    # an n_envs that is not the handles'
    assert fails(st(per, iqn, n=NENV + 1), "does not match")
    assert untouched()
    # the refusals were about the arguments: the same handles take the calls
    assert ts(iqn) == 0 and tr(per, iqn) == 0 and st(per, iqn, train=1) == 0 and st(per3, iqn, train=0) == 0
    torch.cuda.synchronize()
    assert len(per) == sizes[0] + NENV and len(per3) == NENV and not same_state(torch, net_state(iqn), nets[0])


# ================================================================================================================ 8: the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.veciqn import VecIQN
    v = VecIQN(NENV, batch=BATCH, fc_width=FC, observe=2, seed=4, capacity=CAP, lr=1e-4, initial_epsilon=0.5, explore=20, n_step=2, double_q=True,
               replace_target_iter=3, max_grad_norm=5.0, n_tau=NT, n_tau_next=NTP, n_tau_act=KACT, prioritized=True, **kw)
    return v, [v.step().clone() for _ in range(n)]


def loop_state(v):
    return (net_state(v.net), v.env.get_state(), v.nib.clone(), v.stats.clone(), np.asarray(v.replay.state_blob()).copy(), tree_state(v.replay),
            v.timeStep, v.epsilon)


def same_loop(torch, x, y):
    return (same_state(torch, x[0], y[0]) and np.array_equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
            and np.array_equal(x[4], y[4]) and np.array_equal(x[5][0], y[5][0]) and x[5][1:] == y[5][1:] and x[6:] == y[6:])


def test_vec_iqn_prioritized_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vec import IqnPerStep
    from dqnflappybird_amd.veciqn import VecIQN
    v, losses = run_steps(7)
    assert v.prioritized and v.replay.prioritized and isinstance(v.one_step, IqnPerStep) and v.replay.n_step == (2, GAMMA)
    assert not losses[2].any() and all(torch.isfinite(l).all() for l in losses) and losses[6][0] > 0       # steps 0 .. 2 observe, then training
    assert v.timeStep == 7 and len(v.replay) == 7 * NENV and v.replay.population == 6 * NENV and v.epsilon < 0.5
    leaf = heaps(v.replay)[0][CAP - 1:CAP - 1 + v.replay.population]
    print(f"leaves after 4 training steps: {int((leaf != 1.0).sum())} of {len(leaf)} moved off the initial priority 1.0, min {leaf.min():.4f}")
    assert (leaf > 0).all() and (leaf != 1.0).any()                   # the tree moved off its initial max priority
    st = loop_state(v)
    # save -> load -> four more steps == eleven steps straight
    path = str(tmp_path / "iqnper.npz")
    v.save(path)
    z = np.load(path)
    assert str(z["head"][0]) == "iqn" and int(z["prioritized"][0]) == 1
    mk = lambda **kw: VecIQN(NENV, **{**dict(batch=BATCH, fc_width=FC, seed=4, capacity=CAP, n_step=2, n_tau=NT, n_tau_next=NTP, n_tau_act=KACT,
                                             prioritized=True), **kw})
    resumed = mk(lr=3e-5)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and resumed.double_q and isinstance(resumed.one_step, IqnPerStep)
    more = [resumed.step().clone() for _ in range(4)]
    straight, l11 = run_steps(11)
    assert all(torch.equal(x, y) for x, y in zip(more, l11[7:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    # a uniform VecIQN refuses the file, and a prioritized one a uniform loop's
    uniform = mk(prioritized=False)
    with pytest.raises(ValueError, match="written by a VecIQN with a prioritized memory, this VecIQN has a uniform one"):
        uniform.load(path)
    upath = str(tmp_path / "iqn.npz")
    uniform.step()
    uniform.save(upath)
    assert int(np.load(upath)["prioritized"][0]) == 0
    with pytest.raises(ValueError, match="written by a VecIQN with a uniform memory, this VecIQN has a prioritized one"):
        resumed.load(upath)
    mk(prioritized=False).load(upath)
