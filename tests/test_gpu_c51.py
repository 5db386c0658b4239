"""Distributional (C51) Q-learning on the MI355X (include/fbdqn.h): the head, the projected target, the loss
and its gradients against a float64 torch-CPU restatement (the trunk of tests/test_oracle_qnet.py::torch_forward, the C51 head,
projection and loss with autograd; the projection cross-checked against tests/test_c51_host.py's numpy loop), and every path that
trains or plays a C51 net against its composed calls, bit for bit."""
import ctypes

import numpy as np
import pytest

from tests.test_c51_host import np_project
from tests.test_gpu_eval import composed as composed_eval
from tests.test_gpu_nstep import played
from tests.test_oracle_qnet import rand_states, tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
GAMMA = 0.99
FC = 512


def head0(fc=FC):
    """W_fc2's first entry (b_fc1 ends) in a net of fc1 width fc"""
    return 77984 + 1600 * fc + fc


HEAD0 = head0()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_c51(N=51, vmin=-10.0, vmax=10.0, max_batch=256, seed=3, head_scale=1.0, A=2, fc=FC):
    """a C51 net whose ReLUs switch and whose head gives distinctly non-uniform distributions (weights x 3, as the scalar tests do;
    head_scale multiplies the C51 head further -- x 10 makes the distributions nearly one-hot, with logit gaps of tens)"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, "c51", max_batch=max_batch, n_atoms=N, v_min=vmin, v_max=vmax)
    ps = []
    for which in (0, 1):
        net.init_params(seed + which, which)
        p = net.store_params(which).cpu().numpy() * 3.0
        p[head0(fc):] *= head_scale
        net.load_params(p, which)
        ps.append(p)
    return net, ps[0], ps[1]


def support(N, vmin, vmax):
    import torch
    return vmin + (vmax - vmin) / (N - 1) * torch.arange(N, dtype=torch.float64)


def ref_logits(p, s, N, A=2, fc=FC):
    """[B, A, N] float64: the plain trunk with an A N-column head is exactly the C51 logits"""
    import torch
    return torch_forward(p, torch.as_tensor(s, dtype=torch.float64), fc, A * N).view(len(s), A, N)


def greedy_next(q, dev_astar):
    """argmax_a q [B, A]; where the best two are within 1e-4 of each other (a tie at fp32 rounding) the device's choice dev_astar"""
    import torch
    astar = q.argmax(1)
    if dev_astar is None or q.shape[1] < 2:
        return astar
    top = q.topk(2, 1).values
    return torch.where((top[:, 0] - top[:, 1]).abs() < 1e-4, torch.as_tensor(dev_astar, dtype=torch.long), astar)


def torch_project(pn, r, done, G, N, vmin, vmax):
    import torch
    z = support(N, vmin, vmax)
    dz = (vmax - vmin) / (N - 1)
    tz = (r[:, None] + G * (1.0 - done[:, None]) * z[None]).clamp(vmin, vmax)
    b = ((tz - vmin) / dz).clamp(0, N - 1)
    lo, up = b.floor().long(), b.ceil().long()
    m = torch.zeros_like(pn)
    m.scatter_add_(1, lo, pn * (up.double() - b) + pn * (lo == up).double())
    m.scatter_add_(1, up, pn * (b - lo.double()))
    return m


def ref_train(p_on, p_tg, s, a, r, s2, t, G, algo, N, vmin, vmax, dev_astar=None, A=2, fc=FC):
    """-> (loss, flat gradient, m) in float64, with autograd; a* ties within 1e-4 take the device's choice"""
    import torch
    P = torch.tensor(p_on, dtype=torch.float64, requires_grad=True)
    z = support(N, vmin, vmax)
    B = len(s)
    with torch.no_grad():
        pt = torch.softmax(ref_logits(torch.tensor(p_tg, dtype=torch.float64), s2, N, A, fc), -1)
        sel = torch.softmax(ref_logits(P.detach(), s2, N, A, fc), -1) if algo == "c51double" else pt
        q = (sel * z).sum(-1)
        astar = greedy_next(q, dev_astar)
        pn = pt[torch.arange(B), astar]
        rr = torch.as_tensor(r.astype(np.float64))
        dd = torch.as_tensor(t.astype(np.float64))
        m = torch_project(pn, rr, dd, G, N, vmin, vmax)
        np.testing.assert_allclose(m.numpy(), np_project(pn.numpy(), r, t, G, N, vmin, vmax), rtol=0, atol=1e-12)
    lg = ref_logits(P, s, N, A, fc)[torch.arange(B), torch.as_tensor(a, dtype=torch.long)]
    loss = -(m * torch.log_softmax(lg, -1)).sum(-1).mean()
    loss.backward()
    return loss.item(), P.grad.numpy(), m.numpy()


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("N", [51, 11])
def test_forward_and_dist_match_the_restatement(torch_cuda, N):
    torch = torch_cuda
    net, p_on, p_tg = make_c51(N, max_batch=700)
    assert net.support == (N, -10.0, 10.0)
    assert net.n_params == HEAD0 + FC * 2 * N + 2 * N
    rng = np.random.default_rng(N)
    s = rand_states(rng, 2048)
    with torch.no_grad():
        pr = {w: torch.softmax(ref_logits(torch.tensor(p, dtype=torch.float64), s, N), -1) for w, p in ((0, p_on), (1, p_tg))}
    z = support(N, -10.0, 10.0)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 32, 255, 256, 2048):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            p = net.forward_dist(sd[:B].contiguous(), which).cpu().numpy()
            want_p = pr[which][:B].numpy()
            np.testing.assert_allclose(p, want_p, rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, (pr[which][:B] * z).sum(-1).numpy(), rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
            assert np.abs(p.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
    # the distributions are far from uniform (the test would be weak otherwise)
    assert pr[0].max().item() > 1.5 / N


# ---------------------------------------------------------------------------------------------------------------- training
def _batch(rng, B, ints=False):
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = rng.integers(0, 2, B).astype(np.uint8)
    if ints:
        r = rng.choice(np.array([1.0, 3.0, -3.0], np.float32), B)
    else:
        r = rng.choice(np.array([0.1, 3.0, -3.0], np.float32), B, p=[0.6, 0.2, 0.2])
    t = ((r == -3.0) & (rng.random(B) < 0.5)).astype(np.uint8)      # (non-terminal -3: Tz clamps at v_min; +3 at v_max)
    return s, a, r, s2, t


def _check_grads(g, g0, n_head_cols, fc=FC):
    """per tensor.  The head's gradients are continuous in the activations: elementwise, with the scalar tests' bounds.  The rest
    pass through ReLU / max-pool derivatives, which flip for the rare unit within rounding distance of its kink: relative L2 here,
    where the batches are taken as drawn.  On batches whose samples were each drawn clear of the kinks (tests/kinkfree.py) every
    tensor, the trunk and fc1 included, is compared elementwise: tests/test_gpu_kinkfree_grads.py::test_distributional."""
    tensors = tensor_bounds(fc, 1, "c51", n_head_cols)
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


CASES = [(algo, B, G) for algo in ("c51", "c51double") for B in (1, 32, 255, 256) for G in (GAMMA, GAMMA ** 3)]


@pytest.mark.parametrize("algo,B,G", CASES)
def test_train_step_gradients_match_autograd(torch_cuda, algo, B, G):
    torch = torch_cuda
    N = 51
    net, p_on, p_tg = make_c51(N, max_batch=256)
    import zlib
    rng = np.random.default_rng(zlib.crc32(f"{algo}-{B}-{G}".encode()))
    s, a, r, s2, t = _batch(rng, B)
    _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, G, N, -10.0, 10.0)


@pytest.mark.parametrize("algo", ["c51", "c51double"])
def test_gradients_when_every_target_lands_on_an_atom(torch_cuda, algo):
    """Gamma = 1, a unit grid (21 atoms on [-10, 10]) and integer rewards: every b_j is an integer (l == u), the whole mass stays"""
    torch = torch_cuda
    N = 21
    net, p_on, p_tg = make_c51(N, max_batch=64)
    rng = np.random.default_rng(21)
    s, a, r, s2, t = _batch(rng, 32, ints=True)
    m = _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, 1.0, N, -10.0, 10.0)
    np.testing.assert_allclose(m.sum(1), 1.0, atol=1e-12)


def _run_grad_case(torch, net, p_on, p_tg, algo, s, a, r, s2, t, G, N, vmin, vmax):
    d = lambda x: torch.from_numpy(x).cuda()
    which_next = 0 if algo == "c51double" else 1
    dev_astar = net.forward(d(s2), which_next).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, _, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=G, flat_grad=grad)
    loss0, g0, m = ref_train(p_on, p_tg, s, a, r, s2, t, G, algo, N, vmin, vmax, dev_astar)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    _check_grads(grad.cpu().numpy(), g0, 2 * N)
    assert torch.equal(net.store_params(), before)              # gradient export leaves the parameters alone
    # clamps on both sides happened in this batch (rewards +-3, non-terminal)
    return m


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ["c51", "c51double"])
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, algo, B):
    torch = torch_cuda
    rng = np.random.default_rng(B)
    n1, _, _ = make_c51(max_batch=256)
    n2, _, _ = make_c51(max_batch=256)
    for n in (n1, n2):
        n.set_hparams(lr=1e-4)
    g = torch.zeros(n1.n_params, dtype=torch.float32, device="cuda")
    for _ in range(3):
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        l1, _, _ = n1.train_step(algo, s, a, r, s2, t, gamma=GAMMA)
        l2, _, _ = n2.train_step(algo, s, a, r, s2, t, gamma=GAMMA, flat_grad=g)
        n2.apply_adam(g)
        assert torch.equal(l1, l2)
        assert torch.equal(n1.store_params(), n2.store_params())
    m1, v1, p1 = n1.adam_state()
    m2, v2, p2 = n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)


# ---------------------------------------------------------------------------------------------------------------- ring-fed
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ["c51", "c51double"])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, algo, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(256, 20000, 30, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (1, 32, 255):                                   # (the scalar heads' ring-fed tests' sizes: both shapes of the ring-fed trunk)
        n1, _, _ = make_c51(max_batch=256)
        n2, _, _ = make_c51(max_batch=256)
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
def test_train_steps_equals_separate_calls_and_replays_from_a_graph(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import TrainSteps, train_from_replay
    B = 32

    def make():
        _, rep = played(256, 20000, 14, seed=5)
        rep.seed(9, "cpython"); rep.set_n_step(n, GAMMA)
        net, _, _ = make_c51(max_batch=256)
        net.set_hparams(lr=1e-4)
        return rep, net, TrainSteps(rep, net, B, "c51", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    for _ in range(6):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "c51", idx, gamma=GAMMA)
    ts2(6)
    assert torch.equal(n1.store_params(), n2.store_params())
    (r3, n3, ts3), (r4, n4, ts4) = make(), make()
    ts3(1); ts4(1); torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ts3(2)
    graph.replay(); graph.replay()
    ts4(2); ts4(2)
    torch.cuda.synchronize()
    assert torch.equal(n3.store_params(), n4.store_params()) and torch.equal(ts3.loss, ts4.loss)
    assert not torch.equal(n3.store_params(), n1.store_params())


# ---------------------------------------------------------------------------------------------------------------- the full step
def _pipeline(N, B, n, seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env, rep = VecGameState(N, seed=seed), VecReplay(max(20000, 16 * N), N)
    net, _, _ = make_c51(max_batch=max(N, B))
    net.set_hparams(lr=1e-4)
    rep.seed(9, "cpython")
    rep.set_n_step(n, GAMMA)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("N", [256, 1024, 4096])
@pytest.mark.parametrize("n", [1, 3])
def test_vec_step_equals_separate_calls(torch_cuda, N, n):
    """fb_vec_step on a C51 net == act_nib -> frame_step -> push -> sample -> train_from_replay: actions, indices, loss, parameters"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 24
    e1, r1, n1, nib1 = _pipeline(N, B, n)
    e2, r2, n2, nib2 = _pipeline(N, B, n)
    one = VecStep(e2, r2, n2, B, "c51double", GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 10 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, _ = r1.sample(B)
            loss, a, r, t = train_from_replay(r1, n1, "c51double", idx, gamma=GAMMA)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(a, one.a) and torch.equal(r, one.r) and torch.equal(t, one.t), step
    assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all()
    assert n2.split_stats() == (0, 0)                          # the one-stream schedule


# ---------------------------------------------------------------------------------------------------------------- acting
def test_acting_is_the_argmax_and_epsilon_follows_the_plain_rule(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    net, p_on, _ = make_c51(max_batch=400)
    rng = np.random.default_rng(4)
    s = rand_states(rng, 1100)
    with torch.no_grad():
        q = (torch.softmax(ref_logits(torch.tensor(p_on, dtype=torch.float64), s, 51), -1) * support(51, -10.0, 10.0)).sum(-1).numpy()
    sd = torch.from_numpy(s).cuda()
    plain = QNet(2, FC, "plain", max_batch=400)
    plain.init_params(1)
    for B in (7, 200, 1100):
        act, qd = net.act(sd[:B].contiguous(), 0.0, seed=5, step=9, want_q=True)
        act = act.cpu().numpy()
        sure = np.abs(q[:B, 0] - q[:B, 1]) > 1e-4
        assert sure.mean() > 0.9
        np.testing.assert_array_equal(act[sure], q[:B].argmax(1)[sure])
        np.testing.assert_array_equal(act, qd.cpu().numpy().argmax(1))
        for eps, seed, step in ((1.0, 5, 9), (1.0, 123, 4567), (0.3, 5, 9)):
            ac = net.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            ap = plain.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            if eps == 1.0:
                np.testing.assert_array_equal(ac, ap)               # the same draws: randrange(2) of the same Philox counters
            else:                                                    # epsilon rows take the plain net's random action, the rest the argmax
                greedy_c = net.act(sd[:B].contiguous(), 0.0).cpu().numpy()
                greedy_p = plain.act(sd[:B].contiguous(), 0.0).cpu().numpy()
                rand_p = plain.act(sd[:B].contiguous(), 1.0, seed=seed, step=step).cpu().numpy()
                took = ap != greedy_p                                # (rows whose draw changed the plain net's action)
                np.testing.assert_array_equal(ac[took], rand_p[took])
                assert ((ac == greedy_c) | (ac == rand_p)).all()


# ---------------------------------------------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("n,M", [(1027, 1027), (200, 256)])
def test_eval_run_equals_composed_calls(torch_cuda, n, M):
    from dqnflappybird_amd.evaluate import Evaluator
    net, _, _ = make_c51(max_batch=(M + 2) // 3, head_scale=3.0)
    s0, l0, t0, _ = composed_eval(net, M, n, 2, env_seed=11)
    res = Evaluator(n).run(net, n, 2, max_steps=100_000, env_seed=11)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all()


def test_eval_q_is_row_independent(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecGameState
    net, _, _ = make_c51(max_batch=400)
    N = 1027
    env = VecGameState(N, seed=3)
    nib = env.track_state()
    env.observe()
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(30):
        env.frame_step((torch.rand(N, generator=g) < 0.15).to(torch.uint8).cuda(), want_u8=False)
    states = nib.clone()

    def q_of(x):
        q = torch.empty((x.shape[0], 2), dtype=torch.float32, device="cuda")
        L.check(L.lib().fb_eval_q(net.h, L.ptr(x), x.shape[0], L.ptr(q), L.current_stream()), "fb_eval_q")
        torch.cuda.synchronize()
        return q.cpu().numpy()

    q0 = q_of(states)
    _, qa = net.act_nib(states, 0.0, want_q=True)
    assert np.array_equal(qa.cpu().numpy(), q0)
    perm = torch.randperm(N, generator=g)
    assert np.array_equal(q_of(states[perm.cuda()].contiguous()), q0[perm.numpy()])
    for rows in (1, 7, 255):
        for r0 in range(0, min(N, 300), rows):
            r1 = min(N, r0 + rows)
            assert np.array_equal(q_of(states[r0:r1].contiguous()), q0[r0:r1]), (rows, r0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep, train_from_replay
    N, B = 256, 32
    c51, _, _ = make_c51(max_batch=N)
    plain = QNet(2, FC, "plain", max_batch=N); plain.init_params(1); plain.init_params(2, which=1)
    rng = np.random.default_rng(0)
    s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))

    def frozen(net):
        m, v, p = net.adam_state()
        return net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), p.copy()

    def same(x, y):
        return all(torch.equal(i, j) if torch.is_tensor(i) else np.array_equal(i, j) for i, j in zip(x, y))

    before_c, before_p = frozen(c51), frozen(plain)
    for net, algo, msg in ((plain, "c51", "C51 net"), (plain, "c51double", "C51 net"), (c51, "nature", "C51_DOUBLE only"),
                           (c51, "dqn", "C51"), (c51, "double", "C51"), (c51, "per", "C51")):
        with pytest.raises(ValueError, match=msg):
            net.train_step(algo, s, a, r, s2, t, isw=torch.ones(B, device="cuda"), gamma=GAMMA)
    torch.cuda.synchronize()
    assert same(frozen(c51), before_c) and same(frozen(plain), before_p)
    # a prioritized memory, through every training entry point
    env = VecGameState(N, seed=1); env.track_state(); env.observe()
    per = VecReplay(20000, N, prioritized=True); per.reset(env.frame_bits)
    uni = VecReplay(20000, N); uni.reset(env.frame_bits)
    for _ in range(4):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        per.push(env.frame_bits, acts, env.reward, env.terminal)
        uni.push(env.frame_bits, acts, env.reward, env.terminal)
    blob, env_state = per.state_blob().copy(), env.get_state().copy()
    with pytest.raises(ValueError, match="uniform memory only"):
        train_from_replay(per, c51, "c51", torch.zeros(B, dtype=torch.int64, device="cuda"), gamma=GAMMA, isw=torch.ones(B, device="cuda"))
    with pytest.raises(ValueError, match="uniform memory only"):
        VecStep(env, per, c51, B, "c51", GAMMA)
    # fb_vec_step itself (the Python class refuses first): the memory, the env and the net stay as they were
    sb = VecStep(env, uni, c51, B, "c51", GAMMA).buf
    rc = L.lib().fb_vec_step(env.h, per.h, c51.h, ctypes.byref(sb), N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "uniform memory only" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, plain.h, ctypes.byref(sb), N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    uni_blob = uni.state_blob().copy()
    rc = L.lib().fb_vec_step_dp(None, env.h, uni.h, c51.h, None, N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, 1, L.current_stream())
    assert rc == -1 and "data-parallel C51" in L.lib().fb_last_error().decode()
    # (non-NULL dummies: the checks come before any pointer is used)
    rc = L.lib().fb_train_steps(uni.h, c51.h, L.ALGO_NATURE, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_train_steps(per.h, c51.h, L.ALGO_C51, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1
    torch.cuda.synchronize()
    assert np.array_equal(per.state_blob(), blob) and np.array_equal(uni.state_blob(), uni_blob)
    assert np.array_equal(env.get_state(), env_state)
    assert same(frozen(c51), before_c)
    with pytest.raises(ValueError, match="C51"):
        plain.forward_dist(s)
    with pytest.raises(ValueError, match="C51"):
        L.check(L.lib().fb_qnet_create(L.ARCH_C51, FC, 2, 8, ctypes.byref(ctypes.c_void_p())), "fb_qnet_create")


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_vecbrain_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo='c51'): the target net is synced, save / load continues bit for bit; another support, or a scalar-head brain,
    refuses the checkpoint, and a C51 brain refuses a scalar one; evaluate.qnet_from_checkpoint loads it"""
    torch = torch_cuda
    from dqnflappybird_amd.evaluate import qnet_from_checkpoint
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="c51", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4, n_step=3, v_min=-5.0, v_max=15.0)
    a = VecBrain(256, **kw)
    assert a.net.support == (51, -5.0, 15.0)
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
    with pytest.raises(ValueError, match="support"):
        VecBrain(256, **dict(kw, v_max=10.0)).load(ck)
    with pytest.raises(ValueError, match="scalar head"):
        VecBrain(256, **dict(kw, algo="nature")).load(ck)
    plain = VecBrain(256, **dict(kw, algo="nature"))
    plain.save(str(tmp_path / "plain"))
    with pytest.raises(ValueError, match="scalar-head"):
        VecBrain(256, **kw).load(str(tmp_path / "plain"))
    net = qnet_from_checkpoint(ck, max_batch=256)
    assert net.support == (51, -5.0, 15.0)
    assert torch.equal(net.store_params(0).cpu(), torch.from_numpy(np.load(ck + ".npz")["online"]))
