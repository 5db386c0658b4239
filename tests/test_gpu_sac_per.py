"""Prioritized SAC and n-step returns on the GPU (include/fbdqn.h, the prioritized SAC block; csrc/fb_sac.hip: sac_loss_kernel<.., true>)
under the bounds of tests/test_gpu_sac.py -- Q_ATOL on the target, 2 Q_ATOL on abs_err (the mean of two differences of quantities each
held to Q_ATOL), rtol 1e-4 / atol 1e-6 on the loss numbers, rtol 2e-3 / atol 2e-5 x the tensor's scale per gradient tensor -- and, where
the header promises bits, bit for bit: unit weights == the uniform calls, the exact weights 0 and 0.5, ring-fed == gathered on a
prioritized memory at n = 1 and 3, fb_sac_per_step == its separate calls, the leaves Memory.batch_update leaves, the temperature under
weights, every refusal, and the VecSAC(prioritized=True, n_step=3) loop with its checkpoint.  fc_width 128, 16 envs, capacity 2000,
batch 8 unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

from tests.test_c51_per_host import np_priority
from tests.test_gpu_ac import net_state, same_state
from tests.test_gpu_nstep_per import Tape, heaps, per_memory, push
from tests.test_gpu_qnet import Q_ATOL
from tests.test_gpu_sac import GAMMA, SHAPES, check_sac_grads, ref_step, sac_params, sac_state_of, same_sac
from tests.test_sac_host import F32, np_alpha_adam, sac_bounds, sac_forward64
from tests.test_sac_per_host import torch_sac_per_loss

pytestmark = pytest.mark.gpu
FC, NENV, CAP, BATCH = 128, 16, 2000, 8
FB_ERR_STATE = -4                            # include/fbdqn.h
CRITIC_BLOCKS = ("W_q1", "b_q1", "W_q2", "b_q2")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_net(oracle, fc=FC, A=2, max_batch=32, lr=1e-4):
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, "sac", max_batch=max_batch)
    net.load_params(sac_params(oracle, fc, A, 1), 0)
    net.load_params(sac_params(oracle, fc, A, 2), 1)
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


def bits(x):
    return x.detach().cpu().numpy().view(np.uint32)


# ================================================================================================================ 1: w = 1
@pytest.mark.parametrize("n_step", [1, 3])
def test_unit_weights_are_the_uniform_calls_bit_for_bit(torch_cuda, oracle, n_step):
    """the gathered and the ring-fed _per call with w = 1 against the uniform calls on the same transitions: loss, y, the exported gradient,
    then parameters / Adam / the five temperature words after a fused step.  The uniform ring-fed call serves n = 1 only: at n = 3 the
    counterpart is fb_replay_gather on the uniform memory's n-step view, then fb_qnet_sac_train_step with Gamma"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, sac_per_train_from_replay, sac_train_from_replay
    B = BATCH
    env, per, uni = twin_memories(torch, 6, n_step)
    idx = leaves(np.random.default_rng(n_step), per, B)
    pos = idx - (per.capacity - 1)
    s, a, r, s2, t = (x.clone() for x in per.gather(idx))
    su = [x.clone() for x in uni.gather(pos)]
    assert all(torch.equal(x, y) for x, y in zip((s, a, r, s2, t), su))          # the same transitions
    ones = torch.ones(B, dtype=torch.float32, device="cuda")
    G = bootstrap_gamma(GAMMA, n_step)
    nets = [make_net(oracle) for _ in range(4)]
    for net in nets:
        net.set_sac(0.2, 0.4, 3e-3)                                  # the temperature learns: its words must agree as well
    g = [grad_buf(torch, nets[0]) for _ in range(4)]
    l0, y0 = nets[0].sac_train_step(*su, gamma=G, flat_grad=g[0])
    if n_step == 1:
        l1, _, _, _, y1 = sac_train_from_replay(uni, nets[1], pos, gamma=GAMMA, flat_grad=g[1], want_target=True)
    else:
        l1, y1 = nets[1].sac_train_step(*su, gamma=G, flat_grad=g[1])
    l2, y2, ae2 = nets[2].sac_per_train_step(s, a, r, s2, t, ones, gamma=G, flat_grad=g[2])
    l3, a3, r3, t3, y3, ae3 = sac_per_train_from_replay(per, nets[3], idx, ones, gamma=GAMMA, flat_grad=g[3], want_target=True)
    assert g[0].abs().max() > 0 and torch.equal(l0, l1) and torch.equal(g[0], g[1]) and torch.equal(y0, y1)
    for l, y, gg in ((l2, y2, g[2]), (l3, y3, g[3])):
        print(f"w = 1, n_step={n_step}: loss {l.tolist()} / {l0.tolist()}, {int((gg != g[0]).sum())} gradient elements differ")
        assert np.array_equal(bits(l), bits(l0)) and np.array_equal(bits(y), bits(y0)) and np.array_equal(bits(gg), bits(g[0]))
    assert torch.equal(ae2, ae3) and (ae2 >= 0).all() and ae2.max() > 0 and torch.equal(a3, a) and torch.equal(r3, r) and torch.equal(t3, t)
    assert all(np.array_equal(n.store_params(0).cpu().numpy(), sac_params(oracle, FC, 2, 1)) for n in nets)      # gradient-only mode
    # the fused steps
    f0 = nets[0].sac_train_step(*su, gamma=G)[0]
    f1 = sac_train_from_replay(uni, nets[1], pos, gamma=GAMMA)[0] if n_step == 1 else nets[1].sac_train_step(*su, gamma=G)[0]
    f2 = nets[2].sac_per_train_step(s, a, r, s2, t, ones, gamma=G)[0]
    f3 = sac_per_train_from_replay(per, nets[3], idx, ones, gamma=GAMMA)[0]
    st = [sac_state_of(n) for n in nets]
    for k in (1, 2, 3):
        assert torch.equal((f1, f2, f3)[k - 1], f0) and same_sac(torch, st[k], st[0]), k
    assert st[0][5][0] != np.log(F32(0.2)) and not np.array_equal(st[0][0].cpu().numpy(), sac_params(oracle, FC, 2, 1))


# ================================================================================================================ 2: autograd
_wref = {}


def ref_per_step(oracle, fc, A, B):
    """tests/test_gpu_sac.py::ref_step's kink-free inputs, weights in [0.2, 1] (and one exact 1), and the float64 weighted loss numbers,
    target, 0.5 (|d1| + |d2|) and gradient; computed once per (fc, A, B)"""
    import torch
    if (fc, A, B) not in _wref:
        s, a, r, s2, t, _, _, _ = ref_step(oracle, fc, A, B)
        rng = np.random.default_rng(10 * fc + A + B)
        w = (0.2 + 0.8 * rng.random(B)).astype(F32)
        w[0] = 1.0
        p, ptg = sac_params(oracle, fc, A, 1), sac_params(oracle, fc, A, 2)
        pt = torch.tensor(p.astype(np.float64), requires_grad=True)
        z, q1, q2 = sac_forward64(pt, s, fc, A)
        with torch.no_grad():
            zn = sac_forward64(pt.detach(), s2, fc, A)[0]
            _, q1n, q2n = sac_forward64(torch.from_numpy(ptg.astype(np.float64)), s2, fc, A)
        alpha = float(np.exp(np.log(F32(0.2))))
        out = torch_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, GAMMA, alpha, w)
        out[0].backward()
        d1 = (q1[torch.arange(B), torch.as_tensor(a.astype(np.int64))] - out[5]).detach().numpy()
        if B >= 32:                                                  # what tests/test_gpu_sac.py::ref_step asserts of its inputs
            assert (d1 > 0).any() and (d1 < 0).any() and t.any() and not t.all()
            for x, y in ((q1, q2), (q1n, q2n)):
                assert (x < y).any() and (x > y).any()
        _wref[(fc, A, B)] = (s, a, r, s2, t, w, [o.item() for o in out[:5]] + [alpha], out[5].numpy(), out[6].numpy(), pt.grad.numpy())
    return _wref[(fc, A, B)]


@pytest.mark.parametrize("B", [8, 32])
@pytest.mark.parametrize("fc,A", SHAPES)
def test_weighted_step_against_autograd(torch_cuda, oracle, fc, A, B):
    """random w in [0.2, 1]: the six loss numbers, abs_err (unweighted), the target and every gradient tensor; nothing is masked"""
    torch = torch_cuda
    s, a, r, s2, t, w, want, y0, ae0, g0 = ref_per_step(oracle, fc, A, B)
    net = make_net(oracle, fc, A)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = grad_buf(torch, net)
    loss, y, ae = net.sac_per_train_step(d(s), d(a), d(r), d(s2), d(t), d(w), gamma=GAMMA, flat_grad=grad)
    loss, y, ae = loss.cpu().numpy(), y.cpu().numpy(), ae.cpu().numpy()
    print(f"sac per ({fc}, {A}) B={B}: loss {loss.tolist()} / {want}; max |dy| {np.abs(y - y0).max():.3e}; "
          f"max |d abs_err| {np.abs(ae - ae0).max():.3e} at max abs_err {ae0.max():.3e}")
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(y, y0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(ae, ae0, rtol=0, atol=2 * Q_ATOL)
    assert (ae >= 0).all()
    check_sac_grads(grad.cpu().numpy(), g0, fc, A)
    assert np.array_equal(net.store_params(0).cpu().numpy(), sac_params(oracle, fc, A, 1))
    assert net.overflow_count() == 0


# ================================================================================================================ 3: exact weights
@pytest.mark.parametrize("fc,A", SHAPES)
def test_exact_weights(torch_cuda, oracle, fc, A):
    """w = 0: the gradients of both critics' weights and biases are exactly 0 and loss[1] = loss[2] = 0, the actor's numbers are the
    uniform step's bits and abs_err is still written.  w = 0.5: those four gradient blocks and m1 / m2 are bit for bit half the uniform
    step's -- a power-of-two scale passes through the fma chains exactly as long as nothing is subnormal, which the test checks"""
    torch = torch_cuda
    B = 32
    s, a, r, s2, t, _, _, _ = ref_step(oracle, fc, A, B)
    net = make_net(oracle, fc, A)
    d = lambda x: torch.from_numpy(x).cuda()
    gu = grad_buf(torch, net)
    lu, yu = net.sac_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=gu)
    lu, gu = lu.cpu().numpy(), gu.cpu().numpy()
    out = {}
    for w in (1.0, 0.5, 0.0):
        g = grad_buf(torch, net)
        loss, y, ae = net.sac_per_train_step(d(s), d(a), d(r), d(s2), d(t), torch.full((B,), w, dtype=torch.float32, device="cuda"), gamma=GAMMA,
                                             flat_grad=g)
        assert torch.equal(y, yu)
        out[w] = (loss.cpu().numpy(), ae.cpu().numpy(), g.cpu().numpy())
    l1, ae1, g1 = out[1.0]
    assert np.array_equal(l1.view(np.uint32), lu.view(np.uint32)) and np.array_equal(g1.view(np.uint32), gu.view(np.uint32))
    assert (ae1 > 0).all()
    tb = {n: (lo, hi) for n, lo, hi in sac_bounds(fc, A)}
    tiny = np.finfo(np.float32).tiny
    for w in (0.5, 0.0):
        lw, aew, gw = out[w]
        assert np.array_equal(aew, ae1), w                            # the priority carries no weight
        assert lw[3].view(np.uint32) == lu[3].view(np.uint32) and lw[4].view(np.uint32) == lu[4].view(np.uint32) and lw[5] == lu[5], w
    l0, _, g0 = out[0.0]
    assert l0[1] == 0 and l0[2] == 0 and l0[0].view(np.uint32) == F32(F32(F32(0) + F32(0)) + lu[3]).view(np.uint32)
    for name in CRITIC_BLOCKS:
        lo, hi = tb[name]
        assert not g0[lo:hi].any() and np.abs(gu[lo:hi]).max() > 0, name
    lo, hi = tb["W_pi"][0], tb["b_pi"][1]
    assert np.abs(g0[lo:hi]).max() > 0                                # the actor still learns
    lh, _, gh = out[0.5]
    for name in CRITIC_BLOCKS:
        lo, hi = tb[name]
        ref = gu[lo:hi]
        nz = ref != 0
        assert nz.any() and (np.abs(ref[nz]) >= 2 * tiny).all(), name    # normal numbers, and their halves too
        assert np.array_equal(gh[lo:hi].view(np.uint32), (F32(0.5) * ref).view(np.uint32)), name
    for k in (1, 2):
        assert lu[k] >= 2 * tiny and lh[k].view(np.uint32) == (F32(0.5) * lu[k]).view(np.uint32), k


# ================================================================================================================ 4: ring-fed == gathered
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_on_a_prioritized_memory_equals_gathered(torch_cuda, oracle, B, n_step):
    """fb_sac_per_train_from_replay at SumTree leaves == fb_replay_gather + fb_qnet_sac_per_train_step (given Gamma = gamma^n): a / R /
    done, the six loss numbers, abs_err, y, the exported gradient, then the nets after a fused step, bit for bit; at B = 256 the gathered
    form takes the per-state trunk.  The memory is tests/test_gpu_nstep_per.py's: a recorded tape of random pushes, no wrap, so leaf
    cap - 1 + d is transition (t, e) = divmod(d, N) and its window the tape's rows t .. t + n - 1 of env e"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, sac_per_train_from_replay
    N, cap, pushes = 64, 1500, 22
    rep = per_memory(cap, N, n_step)
    tape = Tape(N, seed=11 + n_step, p_term=0.15)
    rep.reset(tape.frames[0])
    for _ in range(pushes):
        push([rep], tape)
    pop = rep.population
    assert pop == (pushes - n_step + 1) * N and 256 <= pop < cap
    rng = np.random.default_rng(B + n_step)
    idx = torch.from_numpy((rng.permutation(pop)[:B] + cap - 1).astype(np.int64)).cuda()
    s, a, r, s2, t = rep.gather(idx)
    terms, t_h = np.stack(tape.terms), t.cpu().numpy()
    kinds = set()
    for b, j in enumerate(idx.cpu().numpy()):
        tt, e = divmod(int(j) - (cap - 1), N)
        win = terms[tt:tt + n_step, e]
        first = int(win.argmax()) if win.any() else -1
        assert bool(t_h[b]) == (first >= 0)
        kinds.add("none" if first < 0 else "last" if first == n_step - 1 else "early")
    assert kinds == ({"none", "last", "early"} if n_step == 3 else {"none", "last"})
    w = torch.from_numpy((0.2 + 0.8 * rng.random(B)).astype(F32)).cuda()
    n1, n2 = make_net(oracle, 512, 2, max_batch=256), make_net(oracle, 512, 2, max_batch=256)
    g1, g2 = grad_buf(torch, n1), grad_buf(torch, n2)
    G = bootstrap_gamma(GAMMA, n_step)
    l1, y1, ae1 = n1.sac_per_train_step(s, a, r, s2, t, w, gamma=G, flat_grad=g1)
    l2, a2, r2, t2, y2, ae2 = sac_per_train_from_replay(rep, n2, idx, w, gamma=GAMMA, flat_grad=g2, want_target=True)
    print(f"per ring-fed vs gathered B={B} n_step={n_step}: loss {l1.tolist()} / {l2.tolist()}, {int((g1 != g2).sum())} gradient elements differ")
    assert torch.equal(a2, a) and torch.equal(r2, r) and torch.equal(t2, t) and g1.abs().max() > 0
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and torch.equal(y1, y2) and torch.equal(g1, g2)
    # a finished window's target is its return, whatever s' holds
    done = t.cpu().numpy() != 0
    rr = r.cpu().numpy()
    assert np.array_equal(y1.cpu().numpy()[done], np.where(rr == F32(0.1), 0.1, rr.astype(np.float64)).astype(F32)[done])
    l1, _, ae1 = n1.sac_per_train_step(s, a, r, s2, t, w, gamma=G)
    l2, _, _, _, ae2 = sac_per_train_from_replay(rep, n2, idx, w, gamma=GAMMA)
    assert torch.equal(l1, l2) and torch.equal(ae1, ae2) and same_sac(torch, sac_state_of(n1), sac_state_of(n2))
    assert not np.array_equal(n1.store_params(0).cpu().numpy(), sac_params(oracle, 512, 2, 1))


# ================================================================================================================ 5, 6: the loop step
def world(oracle, N, batch, n_step, trained=True):
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay
    env = VecGameState(N, seed=5)
    rep = VecReplay(4000, N, prioritized=True, n_step=n_step, gamma=GAMMA)
    rep.seed(7)
    if trained:
        net = make_net(oracle, max_batch=max(N, batch))
    else:                                                            # the library's own initialisation: small errors, under the priority clip
        net = QNet(2, FC, "sac", max_batch=max(N, batch))
        net.init_params(3, which=0); net.init_params(4, which=1)
        net.set_hparams(lr=1e-4)
    net.set_sac(0.2, None, 1e-3)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


def tree_state(rep):
    tree, ptr, size, beta = rep.per_state()
    return tree.view(np.uint64).copy(), ptr, size, beta


@pytest.mark.parametrize("n_step", [1, 2])
@pytest.mark.parametrize("N,batch", [(8, 8), (300, 32)])
def test_sac_per_step_equals_its_separate_calls(torch_cuda, oracle, N, batch, n_step):
    """two identically seeded worlds, 8 steps with and without train and rho: actions, idx, isw, the six loss numbers, abs_err, a / r / t,
    both nets, Adam and the temperature words, the envs, per_state() (tree bytes, pointer, size, beta) and the memory's whole blob"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import SacPerStep, sac_per_train_from_replay
    seed = (3 << 32) | 9
    e1, r1, n1, nib1 = world(oracle, N, batch, n_step)
    e2, r2, n2, nib2 = world(oracle, N, batch, n_step)
    steps = {rho: SacPerStep(e1, r1, n1, batch, GAMMA, rho) for rho in (0.0, 0.01)}
    trained = 0
    for k, (train, rho) in enumerate([(False, 0.0), (True, 0.01), (True, 0.0), (False, 0.01), (True, 0.01), (True, 0.0), (False, 0.0), (True, 0.01)]):
        train = train and k >= n_step - 1
        one = steps[rho]
        a1 = one(seed=seed, step=k, train=train)
        a2, _, _ = n2.act_policy_nib(nib2, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        r2.push(e2.frame_bits, a2, rew, term)
        assert torch.equal(a1, a2) and torch.equal(nib1, nib2), k
        if train:
            idx, isw = r2.sample(batch)
            idx, isw = idx.clone(), isw.clone()
            loss, a_o, r_o, t_o, ae = sac_per_train_from_replay(r2, n2, idx, isw.to(torch.float32), gamma=GAMMA)
            assert torch.equal(one.idx, idx) and torch.equal(one.isw, isw) and torch.equal(one.isw32, isw.to(torch.float32)), k
            assert torch.equal(one.loss, loss) and torch.equal(one.abs_err, ae) and (ae >= 0).all(), k      # abs_err as the loss left it
            assert torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
            r2.update_priorities(idx, abs_err=ae.clone())
            trained += 1
        if rho:
            n2.soft_sync_target(rho)
        assert same_sac(torch, sac_state_of(n1), sac_state_of(n2)), k
        x, y = tree_state(r1), tree_state(r2)
        assert np.array_equal(x[0], y[0]) and x[1:] == y[1:], k
    assert trained == 5 and len(r1) == 8 * N and r1.population == (8 - n_step + 1) * N
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n1.sac_state()[0] != np.log(F32(0.2)) and not np.array_equal(n1.store_params(1).cpu().numpy(), sac_params(oracle, FC, 2, 2))


def test_priorities_reach_the_tree(torch_cuda, oracle):
    """after a step the leaf of every sampled transition holds min(abs_err + 0.01, 1)^0.6 of the abs_err the step left (the last write of
    a leaf drawn twice), as tests/test_gpu_iqn_per.py checks its leaves"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import SacPerStep
    env, rep, net, _ = world(oracle, NENV, BATCH, 1, trained=False)
    one = SacPerStep(env, rep, net, BATCH, GAMMA, 0.005)
    under = 0
    for step in range(4):
        one(seed=1, step=step, train=True)
        torch.cuda.synchronize()
        tree = heaps(rep)[0]
        want = {}
        for i, e in zip(one.idx.cpu().tolist(), one.abs_err.cpu().numpy()):
            want[i] = np_priority(e)
        np.testing.assert_allclose(tree[list(want)], np.array(list(want.values()), np.float64), rtol=1e-6, atol=0)
        under += int((np.array(list(want.values())) < 1.0).sum())
    assert under > 0


# ================================================================================================================ 7: temperature
def test_temperature_under_weights(torch_cuda, oracle):
    """five weighted fused steps with alpha_lr > 0 and weights != 1: the five words against the float32 restatement fed the device's own
    mh, rtol 1e-6 as tests/test_gpu_sac.py; mh is the UNWEIGHTED mean entropy -- the bits an exporting uniform step on the same net and
    minibatch reports just before"""
    torch = torch_cuda
    B = 32
    env, per, _ = twin_memories(torch, 6)
    rng = np.random.default_rng(4)
    idx = leaves(rng, per, B)
    s, a, r, s2, t = (x.clone() for x in per.gather(idx))
    w = torch.from_numpy((0.2 + 0.6 * rng.random(B)).astype(F32)).cuda()
    assert (w < 1).all()
    net = make_net(oracle)
    hbar, alr = 0.4, 3e-3
    net.set_sac(0.2, hbar, alr)
    st = net.sac_state()
    g = grad_buf(torch, net)
    for k in range(5):
        lu = net.sac_train_step(s, a, r, s2, t, gamma=GAMMA, flat_grad=g)[0].cpu().numpy()      # (exporting: leaves the net and the words alone)
        assert np.array_equal(net.sac_state(), st)
        loss = net.sac_per_train_step(s, a, r, s2, t, w, gamma=GAMMA)[0].cpu().numpy()
        assert loss[4].view(np.uint32) == lu[4].view(np.uint32) and loss[3].view(np.uint32) == lu[3].view(np.uint32), k
        assert 0 < loss[1] < lu[1] and 0 < loss[2] < lu[2], k          # ... while the critic terms carry the weights
        np.testing.assert_allclose(loss[5], np.exp(np.float64(st[0])), rtol=1e-6)                # the alpha the PREVIOUS step left
        st = np_alpha_adam(st, loss[4], hbar, alr)
        got = net.sac_state()
        print(f"temperature step {k}: device {got.tolist()} / numpy {st.tolist()} / max rel diff {(np.abs(got.astype(np.float64) - st) / np.abs(st)).max():.3e}")
        np.testing.assert_allclose(got, st, rtol=1e-6, atol=0)
        st = got
    assert net.sac()[0] != 0.2
    net.sac_per_train_step(s, a, r, s2, t, w, gamma=GAMMA, flat_grad=g)       # an exporting weighted step leaves the words alone
    assert np.array_equal(net.sac_state(), st)


# ================================================================================================================ 8: refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, SacPerStep, SacStep, VecReplay, sac_per_train_from_replay, sac_train_from_replay
    lib = L.lib()
    B = BATCH
    env, per, uni = twin_memories(torch, 6)
    env.track_state()
    sac = make_net(oracle)
    plain = QNet(2, FC, "plain", max_batch=32)
    plain.init_params(1); plain.init_params(2, which=1)
    per3 = VecReplay(CAP, NENV, prioritized=True, n_step=3, gamma=GAMMA)           # an n-step prioritized memory, its tree still empty
    per3.seed(9); per3.reset(env.frame_bits)
    blobs = [np.asarray(m.state_blob()).copy() for m in (per, uni, per3)]
    sizes = [len(m) for m in (per, uni, per3)]
    nets, envs = [sac_state_of(sac), net_state(plain)], env.get_state().copy()

    def untouched():
        torch.cuda.synchronize()
        return (all(np.array_equal(np.asarray(m.state_blob()), b) for m, b in zip((per, uni, per3), blobs)) and [len(m) for m in (per, uni, per3)] == sizes
                and same_sac(torch, sac_state_of(sac), nets[0]) and same_state(torch, net_state(plain), nets[1]) and np.array_equal(env.get_state(), envs))

    idx = leaves(np.random.default_rng(0), per, B)
    s, a, r, s2, t = per.gather(idx)
    w = torch.ones(B, dtype=torch.float32, device="cuda")
    ae = torch.zeros(B, dtype=torch.float32, device="cuda")
    loss = torch.zeros(6, dtype=torch.float32, device="cuda")
    a_o, t_o = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    r_o = torch.zeros(B, dtype=torch.float32, device="cuda")
    fails = lambda rc, word, code=-1: rc == code and word in lib.fb_last_error().decode()
    ts = lambda net, Bn=B, g=0.99, isw=w, err=ae: lib.fb_qnet_sac_per_train_step(net.h, Bn, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t), L.ptr(isw), g,
                                                                               L.ptr(loss), L.ptr(err), None, None, None)
    tr = lambda rp, net, Bn=B, g=0.99, isw=w, err=ae: lib.fb_sac_per_train_from_replay(rp.h, net.h, Bn, L.ptr(idx), L.ptr(isw), L.ptr(a_o), L.ptr(r_o), L.ptr(t_o),
                                                                                     g, L.ptr(loss), L.ptr(err), None, None, None)
    sb = SacPerStep(env, per, sac, B, GAMMA)
    st = lambda rp, net, n=NENV, Bn=B, g=GAMMA, buf=sb.buf, train=1, rho=0.0: lib.fb_sac_per_step(env.h, rp.h, net.h, C.byref(buf), n, Bn, 0, 0, train, g,
                                                                                                 C.c_float(rho), None)
    # a uniform memory
    assert fails(tr(uni, sac), "fb_sac_per_train_from_replay: trains from a prioritized memory only")
    for train in (0, 1):
        assert fails(st(uni, sac, train=train), "fb_sac_per_step: trains from a prioritized memory only")
    with pytest.raises(ValueError, match="sac_per_train_from_replay trains from a prioritized memory only"):
        sac_per_train_from_replay(uni, sac, idx, w)
    with pytest.raises(ValueError, match="SacPerStep trains from a prioritized memory only"):
        SacPerStep(env, uni, sac, B)
    # ... and the uniform calls keep refusing a prioritized one, with the words they had
    with pytest.raises(ValueError, match="uniform memory only"):
        sac_train_from_replay(per, sac, idx)
    with pytest.raises(ValueError, match="uniform memory only"):
        SacStep(env, per, sac, B)
    assert fails(lib.fb_sac_train_from_replay(per.h, sac.h, B, L.ptr(idx), L.ptr(a_o), L.ptr(r_o), L.ptr(t_o), 0.99, L.ptr(loss), None, None, None),
                 "SAC trains from a uniform memory only (prioritized replay is not offered)")
    assert fails(lib.fb_sac_step(env.h, per.h, sac.h, C.byref(sb.buf), NENV, B, 0, 0, 1, 0.99, C.c_float(0.0), None), "uniform memory only")
    # a net that is not a SAC net
    for rc in (lambda: ts(plain), lambda: tr(per, plain), lambda: st(per, plain)):
        assert fails(rc(), "not a SAC net (fb_qnet_create_sac)")
    for call in (lambda: plain.sac_per_train_step(s, a, r, s2, t, w), lambda: sac_per_train_from_replay(per, plain, idx, w),
                 lambda: SacPerStep(env, per, plain, B)):
        with pytest.raises(ValueError, match="needs a SAC net"):
            call()
    # NULL isw / abs_err; a training step without one of the three buffers (a store-only step needs none of them: checked below)
    assert fails(ts(sac, isw=None), "needs the importance weights") and fails(ts(sac, err=None), "needs the importance weights")
    assert fails(tr(per, sac, isw=None), "needs the importance weights") and fails(tr(per, sac, err=None), "needs the importance weights")
    for field in ("isw", "isw32", "abs_err"):
        buf = L.StepBuffers()
        C.memmove(C.byref(buf), C.byref(sb.buf), C.sizeof(buf))
        setattr(buf, field, None)
        assert fails(st(per, sac, buf=buf), "needs the isw / isw32 / abs_err buffers"), field
    for bad in (None, w[:4], w.double(), w.view(B, 1)):
        with pytest.raises(ValueError, match="isw must be a contiguous float32"):
            sac.sac_per_train_step(s, a, r, s2, t, bad)
        with pytest.raises(ValueError, match="isw must be a contiguous float32"):
            sac_per_train_from_replay(per, sac, idx, bad)
    # the batch, gamma and rho rules of the uniform calls
    for call in (ts, lambda net, **kw: tr(per, net, **kw), lambda net, **kw: st(per, net, **kw)):
        assert fails(call(sac, Bn=33), "exceeds min(max_batch, 256)") and call(sac, Bn=0) == -1
        assert fails(call(sac, g=1.5), "gamma must be in [0, 1]")
    for rho in (1.5, -0.1):
        assert fails(st(per, sac, rho=rho), "rho must be in [0, 1]")
    # an n-step prioritized memory: the memory's gamma; FB_ERR_STATE while its tree is empty (a store-only step is no refusal)
    assert fails(tr(per3, sac, g=0.9), "fb_sac_per_train_from_replay: gamma 0.9") and fails(st(per3, sac, g=0.9), "fb_sac_per_step: gamma 0.9")
    assert fails(tr(per3, sac, g=GAMMA), "holds no complete transition", FB_ERR_STATE)
    assert fails(st(per3, sac, g=GAMMA), "holds no complete transition", FB_ERR_STATE)
    # an n_envs that is not the handles'
    assert fails(st(per, sac, n=NENV + 1), "does not match")
    assert untouched()
    # the refusals were about the arguments: the same handles take the calls
    assert ts(sac) == 0 and tr(per, sac) == 0 and st(per, sac, train=1) == 0 and st(per3, sac, train=0) == 0
    torch.cuda.synchronize()
    assert len(per) == sizes[0] + NENV and len(per3) == NENV and not same_sac(torch, sac_state_of(sac), nets[0])


# ================================================================================================================ 9: the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.vecsac import VecSAC
    v = VecSAC(NENV, batch=BATCH, fc_width=FC, observe=2, seed=4, capacity=CAP, alpha_lr=1e-3, max_grad_norm=5.0, prioritized=True, n_step=3, **kw)
    return v, [v.step().clone() for _ in range(n)]


def loop_state(v):
    return (sac_state_of(v.net), v.env.get_state(), v.nib.clone(), v.stats.clone(), np.asarray(v.replay.state_blob()).copy(), tree_state(v.replay),
            v.timeStep)


def same_loop(torch, x, y):
    return (same_sac(torch, x[0], y[0]) and np.array_equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
            and np.array_equal(x[4], y[4]) and np.array_equal(x[5][0], y[5][0]) and x[5][1:] == y[5][1:] and x[6] == y[6])


def test_vec_sac_prioritized_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vec import SacPerStep
    from dqnflappybird_amd.vecsac import VecSAC
    v, losses = run_steps(6)
    assert v.prioritized and v.replay.prioritized and isinstance(v.one_step, SacPerStep) and v.replay.n_step == (3, GAMMA)
    assert not losses[1].any() and all(torch.isfinite(l).all() for l in losses) and losses[5][1] > 0       # two store-only steps, then training
    assert v.timeStep == 6 and len(v.replay) == 6 * NENV and v.replay.population == 4 * NENV and v.net.sac()[0] != 0.2
    leaf = heaps(v.replay)[0][CAP - 1:CAP - 1 + v.replay.population]
    print(f"leaves after 4 training steps: {int((leaf != 1.0).sum())} of {len(leaf)} moved off the initial priority 1.0, min {leaf.min():.4f}")
    assert (leaf > 0).all() and (leaf != 1.0).any()                   # the tree moved off its initial max priority
    st = loop_state(v)
    res = v.evaluate(n_envs=32, episodes=1, max_steps=200)            # evaluate() leaves the training state untouched
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(v), st)
    # save -> load -> four more steps == ten steps straight
    path = str(tmp_path / "sacper.npz")
    v.save(path)
    z = np.load(path)
    assert str(z["head"][0]) == "sac" and int(z["prioritized"][0]) == 1 and int(z["n_step"][0]) == 3
    mk = lambda **kw: VecSAC(NENV, **{**dict(batch=BATCH, fc_width=FC, observe=2, seed=4, capacity=CAP, prioritized=True, n_step=3), **kw})
    resumed = mk(lr=3e-5)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and isinstance(resumed.one_step, SacPerStep)
    more = [resumed.step().clone() for _ in range(4)]
    straight, l10 = run_steps(10)
    assert all(torch.equal(x, y) for x, y in zip(more, l10[6:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    # a uniform VecSAC refuses the file by name, a prioritized one of another n as well, and a prioritized one a uniform loop's
    uniform = mk(prioritized=False, n_step=1)
    with pytest.raises(ValueError, match="written by a VecSAC with a prioritized memory, this VecSAC has a uniform one"):
        uniform.load(path)
    with pytest.raises(ValueError, match="written with n_step = 3, this VecSAC has n_step = 2"):
        mk(n_step=2).load(path)
    upath = str(tmp_path / "sac.npz")
    uniform.step()
    uniform.save(upath)
    assert "prioritized" not in np.load(upath).files and "n_step" not in np.load(upath).files       # a uniform loop's file: the keys of before
    with pytest.raises(ValueError, match="written by a VecSAC with a uniform memory, this VecSAC has a prioritized one"):
        resumed.load(upath)
    mk(prioritized=False, n_step=1).load(upath)
    # evaluate.py plays the file as any head = 'sac' file
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=FC)
    assert net.arch == "sac" and torch.equal(net.store_params(), v.net.store_params())
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    v.run(1, log_every=1)
