"""The dueling C51 head on the MI355X (include/fbdqn.h): forward, distributions, the loss and every gradient
of the four C51 algos against a float64 torch-CPU restatement that writes the dueling head out directly (the trunk of
tests/test_oracle_qnet.py::torch_forward, then V + Adv - mean_a Adv per atom; nothing folded), the folded head's freshness after every
parameter change, and every path that trains or plays the net against its composed calls, bit for bit."""
import ctypes
import zlib

import numpy as np
import pytest

from tests.test_c51_per_host import np_kl_priority
from tests.test_gpu_c51 import FC, GAMMA, HEAD0, _batch, greedy_next, head0, support, torch_project
from tests.test_gpu_eval import composed as composed_eval
from tests.test_gpu_nstep import played
from tests.test_gpu_nstep_per import per_memory
from tests.test_oracle_qnet import rand_states, tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
ALGOS = ("c51", "c51double", "c51per", "c51doubleper")
PER = ("c51per", "c51doubleper")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def head_size(N, A=2, fc=FC):
    return fc * N + N + fc * A * N + A * N


def make_c51d(N=51, vmin=-10.0, vmax=10.0, max_batch=256, seed=3, head_scale=1.0, A=2, fc=FC):
    """a dueling C51 net scaled as tests/test_gpu_c51.py::make_c51 scales a C51 net (weights x 3, the head x head_scale more)"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, "c51dueling", max_batch=max_batch, n_atoms=N, v_min=vmin, v_max=vmax)
    ps = []
    for which in (0, 1):
        net.init_params(seed + which, which)
        p = net.store_params(which).cpu().numpy() * 3.0
        p[head0(fc):] *= head_scale
        net.load_params(p, which)
        ps.append(p)
    return net, ps[0], ps[1]


def ref_logits_d(P, s, N, A=2, fc=FC):
    """[B, A, N] float64: h = relu(fc1) through torch_forward's trunk (an identity head returns h itself), then the dueling head"""
    import torch
    P = torch.as_tensor(P, dtype=torch.float64)
    o = head0(fc)
    ident = torch.cat([P[:o], torch.eye(fc, dtype=torch.float64).flatten(), torch.zeros(fc, dtype=torch.float64)])
    h = torch_forward(ident, torch.as_tensor(s, dtype=torch.float64), fc, fc)
    wv = P[o:o + fc * N].view(fc, N); o += fc * N
    bv = P[o:o + N]; o += N
    wa = P[o:o + fc * A * N].view(fc, A * N); o += fc * A * N
    ba = P[o:o + A * N]
    v = h @ wv + bv
    adv = (h @ wa + ba).view(len(s), A, N)
    return v[:, None, :] + (adv - adv.mean(1, keepdim=True))


def ref_q(p, s, N, vmin=-10.0, vmax=10.0, A=2, fc=FC):
    import torch
    with torch.no_grad():
        return (torch.softmax(ref_logits_d(p, s, N, A, fc), -1) * support(N, vmin, vmax)).sum(-1).numpy()


def ref_train(p_on, p_tg, s, a, r, s2, t, w, G, algo, N, vmin, vmax, dev_astar, A=2, fc=FC):
    """-> (loss, flat gradient, KL per sample) in float64 with autograd; w = None: the uniform algos' mean"""
    import torch
    P = torch.tensor(p_on, dtype=torch.float64, requires_grad=True)
    z = support(N, vmin, vmax)
    B = len(s)
    with torch.no_grad():
        pt = torch.softmax(ref_logits_d(p_tg, s2, N, A, fc), -1)
        sel = torch.softmax(ref_logits_d(P.detach(), s2, N, A, fc), -1) if algo in ("c51double", "c51doubleper") else pt
        q = (sel * z).sum(-1)
        astar = greedy_next(q, dev_astar)
        m = torch_project(pt[torch.arange(B), astar], torch.as_tensor(r.astype(np.float64)), torch.as_tensor(t.astype(np.float64)),
                          G, N, vmin, vmax)
    logp = torch.log_softmax(ref_logits_d(P, s, N, A, fc)[torch.arange(B), torch.as_tensor(a, dtype=torch.long)], -1)
    ce = -(m * logp).sum(-1)
    loss = (torch.as_tensor(w, dtype=torch.float64) * ce).mean() if w is not None else ce.mean()
    loss.backward()
    return loss.item(), P.grad.numpy(), np_kl_priority(m.numpy(), logp.detach().exp().numpy())


def check_grads(g, g0, N, A=2, fc=FC):
    """tests/test_gpu_c51.py::_check_grads's tolerances, per tensor: the four head tensors elementwise, the rest relative L2"""
    tensors = tensor_bounds(fc, A, "c51dueling", N)
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
@pytest.mark.parametrize("N", [2, 51, 64])
def test_forward_dist_and_eval_q_match_the_restatement(torch_cuda, N):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    net, p_on, p_tg = make_c51d(N, max_batch=700)
    assert net.support == (N, -10.0, 10.0)
    assert net.n_params == HEAD0 + head_size(N)
    rng = np.random.default_rng(N)
    s = rand_states(rng, 2048)
    with torch.no_grad():
        pr = {w: torch.softmax(ref_logits_d(p, s, N), -1) for w, p in ((0, p_on), (1, p_tg))}
    z = support(N, -10.0, 10.0)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 32, 255, 256, 2048):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            p = net.forward_dist(sd[:B].contiguous(), which).cpu().numpy()
            np.testing.assert_allclose(p, pr[which][:B].numpy(), rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, (pr[which][:B] * z).sum(-1).numpy(), rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
    assert pr[0].max().item() > 1.5 / N
    # fb_eval_q on the env's nibble states: act_nib's Q, and the restatement's on the same states as frame stacks (the memory's)
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env, rep = VecGameState(300, seed=2), VecReplay(5000, 300)
    nib = env.track_state()
    env.observe()
    rep.reset(env.frame_bits)
    for k in range(12):
        acts = torch.full((300,), k % 3 == 0, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        rep.push(env.frame_bits, acts, env.reward, env.terminal)
    qe = torch.empty((300, 2), dtype=torch.float32, device="cuda")
    L.check(L.lib().fb_eval_q(net.h, L.ptr(nib), 300, L.ptr(qe), L.current_stream()), "fb_eval_q")
    _, qa = net.act_nib(nib, 0.0, want_q=True)
    assert torch.equal(qe, qa)
    np.testing.assert_allclose(qe.cpu().numpy(), ref_q(p_on, rep.current_state().cpu().numpy(), N), rtol=0, atol=1e-4)


# ---------------------------------------------------------------------------------------------------------------- training
CASES = [(algo, B) for algo in ALGOS for B in (1, 32, 255, 256)]


@pytest.mark.parametrize("algo,B", CASES)
def test_loss_and_every_gradient_match_autograd(torch_cuda, algo, B):
    torch = torch_cuda
    N = 51
    net, p_on, p_tg = make_c51d(N, max_batch=256)
    rng = np.random.default_rng(zlib.crc32(f"d-{algo}-{B}".encode()))
    s, a, r, s2, t = _batch(rng, B)
    d = lambda x: torch.from_numpy(x).cuda()
    w = (1.0 - rng.random(B)).astype(np.float32) if algo in PER else None       # (0, 1]: non-uniform weights
    dev_astar = net.forward(d(s2), 0 if "double" in algo else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w) if w is not None else None, gamma=GAMMA, flat_grad=grad,
                                 want_aux=algo in PER)
    loss0, g0, kl0 = ref_train(p_on, p_tg, s, a, r, s2, t, w.astype(np.float64) if w is not None else None, GAMMA, algo, N, -10.0, 10.0,
                               dev_astar)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_grads(grad.cpu().numpy(), g0, N)
    if algo in PER:
        np.testing.assert_allclose(ae.cpu().numpy(), kl0, rtol=1e-4, atol=5e-4)
    assert torch.equal(net.store_params(), before)


@pytest.mark.parametrize("N", [2, 64])
def test_gradients_at_the_support_limits(torch_cuda, N):
    """N = 64 with A = 2: the 192 output columns of the unfold (dW_v 64 + dW_a 128); N = 2: the smallest support"""
    torch = torch_cuda
    net, p_on, p_tg = make_c51d(N, max_batch=64)
    rng = np.random.default_rng(N + 100)
    s, a, r, s2, t = _batch(rng, 48)
    d = lambda x: torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, _, _ = net.train_step("c51", d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=grad)
    loss0, g0, _ = ref_train(p_on, p_tg, s, a, r, s2, t, None, GAMMA, "c51", N, -10.0, 10.0, dev_astar)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_grads(grad.cpu().numpy(), g0, N)


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ALGOS)
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, algo, B):
    torch = torch_cuda
    rng = np.random.default_rng(B + len(algo))
    n1, _, _ = make_c51d(max_batch=256)
    n2, _, _ = make_c51d(max_batch=256)
    for n in (n1, n2):
        n.set_hparams(lr=1e-4)
    g = torch.zeros(n1.n_params, dtype=torch.float32, device="cuda")
    for _ in range(3):
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        isw = torch.from_numpy((1.0 - rng.random(B)).astype(np.float32)).cuda() if algo in PER else None
        l1, _, _ = n1.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, want_aux=False)
        l2, _, _ = n2.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, flat_grad=g, want_aux=False)
        n2.apply_adam(g)
        assert torch.equal(l1, l2)
        assert torch.equal(n1.store_params(), n2.store_params())
    m1, v1, p1 = n1.adam_state()
    m2, v2, p2 = n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)


# ---------------------------------------------------------------------------------------------------------------- staleness
def test_the_head_is_never_stale(torch_cuda):
    """after load_params, init_params, a target sync, a fused train step and apply_adam, forward and acting give the restatement's Q
    of the parameters as they now are (a folded head left behind by any of them fails here)"""
    torch = torch_cuda
    N = 51
    net, p_on, _ = make_c51d(N, max_batch=256)
    net.set_hparams(lr=3e-3)                                 # (steps large enough to move Q well past the tolerance)
    rng = np.random.default_rng(7)
    s = rand_states(rng, 64)
    sd = torch.from_numpy(s).cuda()

    def check(which, what):
        p = net.store_params(which).cpu().numpy()
        q0 = ref_q(p, s, N)
        q = net.forward(sd, which).cpu().numpy()
        np.testing.assert_allclose(q, q0, rtol=0, atol=1e-4, err_msg=what)
        if which == 0:
            act, qa = net.act(sd, 0.0, want_q=True)
            np.testing.assert_allclose(qa.cpu().numpy(), q0, rtol=0, atol=1e-4, err_msg=what)
            sure = np.abs(q0[:, 0] - q0[:, 1]) > 1e-4
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
            net.train_step("c51", s_, a_, r_, s2_, t_, gamma=GAMMA)
            q = check(0, "fused train step")
        else:
            g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            net.train_step("c51double", s_, a_, r_, s2_, t_, gamma=GAMMA, flat_grad=g)
            net.apply_adam(g)
            q = check(0, "apply_adam")
        assert np.abs(q - q_prev).max() > 1e-4
    # b_v: all N entries start at 0.01
    net.init_params(5, 0)
    p = net.store_params(0).cpu().numpy()
    o = HEAD0 + FC * N
    assert (p[o:o + N] == np.float32(0.01)).all() and (p[o + N + FC * 2 * N:] == np.float32(0.01)).all()
    assert np.abs(p[HEAD0:o]).max() <= 0.02 and p[HEAD0:o].std() > 0.008        # W_v: truncated normal, stddev 0.01 (0.0088 after the cut)


# ---------------------------------------------------------------------------------------------------------------- composed calls
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ["c51", "c51double"])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, algo, n):
    """(the prioritized algos' ring-fed path: test_vec_step_equals_separate_calls, whose separate calls train from the ring)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(256, 20000, 30, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (1, 32, 255):
        n1, _, _ = make_c51d(max_batch=256)
        n2, _, _ = make_c51d(max_batch=256)
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(3):
            idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
            isw = torch.from_numpy((1.0 - rng.random(B)).astype(np.float32)).cuda() if algo in PER else None
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, ae1, _ = n1.train_step(algo, s, a, r, s2, t, isw=isw, gamma=G, flat_grad=g1 if exp else None, want_aux=algo in PER)
            out = train_from_replay(rep, n2, algo, idx, gamma=GAMMA, isw=isw, flat_grad=g2 if exp else None, want_abs_err=algo in PER)
            assert torch.equal(l1, out[0]), (algo, n, B, step)
            if algo in PER:
                assert torch.equal(ae1, out[4])
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
        net, _, _ = make_c51d(max_batch=256)
        net.set_hparams(lr=1e-4)
        return rep, net, TrainSteps(rep, net, B, "c51double", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    for _ in range(6):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "c51double", idx, gamma=GAMMA)
    ts2(6)
    assert torch.equal(n1.store_params(), n2.store_params())
    assert not torch.equal(n1.store_params(), make()[1].store_params())


def _pipeline(N, n, algo, seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(N, seed=seed)
    if algo in PER:
        rep = per_memory(6 * N + 13, N, n, "exact")
    else:
        rep = VecReplay(max(20000, 16 * N), N)
        rep.seed(9, "cpython")
        rep.set_n_step(n, GAMMA)
    net, _, _ = make_c51d(max_batch=N)
    net.set_hparams(lr=1e-4)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("N", [256, 1024])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ["c51double", "c51doubleper"])
def test_vec_step_equals_separate_calls(torch_cuda, algo, n, N):
    """fb_vec_step on a dueling C51 net == act_nib -> frame_step -> push -> sample -> train_from_replay (-> batch_update): actions,
    indices, weights, losses, priorities, parameters and the memory's state"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 16
    per = algo in PER
    e1, r1, n1, nib1 = _pipeline(N, n, algo)
    e2, r2, n2, nib2 = _pipeline(N, n, algo)
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 5 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            if per:
                idx, isw = r1.sample(B)
                loss, _, r_, t_, ae = train_from_replay(r1, n1, algo, idx, gamma=GAMMA, isw=isw, want_abs_err=True)
                r1.update_priorities(idx, abs_err=ae)
            else:
                idx, _ = r1.sample(B)
                loss, _, r_, t_ = train_from_replay(r1, n1, algo, idx, gamma=GAMMA)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(r_, one.r) and torch.equal(t_, one.t), step
            if per:
                assert torch.equal(isw, one.isw) and torch.equal(ae, one.abs_err + 0.01), step
    assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all()
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n2.split_stats() == (0, 0)                          # the one-stream schedule


# ---------------------------------------------------------------------------------------------------------------- acting, evaluation
def test_acting_is_the_argmax_and_epsilon_follows_the_plain_rule(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    net, p_on, _ = make_c51d(max_batch=400)
    rng = np.random.default_rng(4)
    s = rand_states(rng, 1100)
    q = ref_q(p_on, s, 51)
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
        for eps, seed, step in ((1.0, 5, 9), (1.0, 123, 4567)):
            ac = net.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            ap = plain.act(sd[:B].contiguous(), eps, seed=seed, step=step).cpu().numpy()
            np.testing.assert_array_equal(ac, ap)               # the same draws: randrange(2) of the same Philox counters


@pytest.mark.parametrize("n,M", [(1027, 1027), (200, 256)])
def test_eval_run_equals_composed_calls(torch_cuda, n, M):
    from dqnflappybird_amd.evaluate import Evaluator
    net, _, _ = make_c51d(max_batch=(M + 2) // 3, head_scale=3.0)
    s0, l0, t0, _ = composed_eval(net, M, n, 2, env_seed=11)
    res = Evaluator(n).run(net, n, 2, max_steps=100_000, env_seed=11)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all()


def test_eval_run_reads_the_current_head(torch_cuda):
    """fb_eval_run's head reads the copy the fused acting forward takes: after the parameters change it plays the new net"""
    from dqnflappybird_amd.evaluate import Evaluator
    net, p_on, _ = make_c51d(max_batch=343, head_scale=3.0)
    ev = Evaluator(1027)
    r0 = ev.run(net, 1027, 1, max_steps=100_000, env_seed=11)
    p2 = p_on.copy()
    p2[HEAD0:] = -p2[HEAD0:]
    net.load_params(p2, 0)
    s1, l1, t1, _ = composed_eval(net, 1027, 1027, 1, env_seed=11)
    r1 = ev.run(net, 1027, 1, max_steps=100_000, env_seed=11)
    assert np.array_equal(r1.length, l1) and np.array_equal(r1.score, s1)
    assert not np.array_equal(r1.length, r0.length)


def test_eval_q_is_row_independent(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecGameState
    net, _, _ = make_c51d(max_batch=400)
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
    perm = torch.randperm(N, generator=g)
    assert np.array_equal(q_of(states[perm.cuda()].contiguous()), q0[perm.numpy()])
    for rows in (1, 7, 255):
        for r0 in range(0, 300, rows):
            r1 = min(N, r0 + rows)
            assert np.array_equal(q_of(states[r0:r1].contiguous()), q0[r0:r1]), (rows, r0)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecGameState, VecReplay, VecStep
    N, B = 256, 32
    net, _, _ = make_c51d(max_batch=N)
    rng = np.random.default_rng(0)
    s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
    ones = torch.ones(B, device="cuda")
    before = frozen(net)
    for algo in ("dqn", "nature", "double", "per"):
        with pytest.raises(ValueError, match="C51"):
            net.train_step(algo, s, a, r, s2, t, isw=ones, gamma=GAMMA)
    env = VecGameState(N, seed=1); env.track_state(); env.observe()
    uni = VecReplay(20000, N); uni.reset(env.frame_bits)
    for _ in range(4):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        uni.push(env.frame_bits, acts, env.reward, env.terminal)
    blob, env_state = uni.state_blob().copy(), env.get_state().copy()
    sb = VecStep(env, uni, net, B, "c51", GAMMA).buf
    rc = L.lib().fb_vec_step(env.h, uni.h, net.h, ctypes.byref(sb), N, L.ALGO_NATURE, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step_dp(None, env.h, uni.h, net.h, None, N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, 1, L.current_stream())
    assert rc == -1 and "data-parallel C51" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_train_steps(uni.h, net.h, L.ALGO_NATURE, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(uni.state_blob(), blob) and np.array_equal(env.get_state(), env_state)
    assert same(frozen(net), before)
    for arch in (L.ARCH_C51, L.ARCH_C51_DUELING):
        with pytest.raises(ValueError, match="C51"):
            L.check(L.lib().fb_qnet_create(arch, FC, 2, 8, ctypes.byref(ctypes.c_void_p())), "fb_qnet_create")


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_vecbrain_rainbow_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo='c51doubleper', arch='c51dueling', n_step=3): save / load continues bit for bit; plain C51 and dueling C51
    refuse each other's checkpoints naming both heads; evaluate loads the checkpoint and plays it"""
    torch = torch_cuda
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="c51doubleper", arch="c51dueling", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4, n_step=3,
              v_min=-5.0, v_max=15.0)
    a = VecBrain(256, **kw)
    assert a.net.arch == "c51dueling" and a.net.support == (51, -5.0, 15.0) and a.net.n_params == HEAD0 + head_size(51)
    a.run(20, log_every=0)
    assert not torch.equal(a.net.store_params(0), a.net.store_params(1))
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(10):
        a.step()
        ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.loss.clone(), a.one_step.abs_err.clone()))
    b = VecBrain(256, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(10):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.loss, b.one_step.abs_err)
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0)) and torch.equal(a.net.store_params(1), b.net.store_params(1))
    with pytest.raises(ValueError, match="c51 head.*c51dueling head|c51dueling head.*c51 head"):
        VecBrain(256, **dict(kw, arch="plain")).load(ck)
    plain_c51 = VecBrain(256, **dict(kw, arch="c51"))
    plain_c51.save(str(tmp_path / "c51"))
    with pytest.raises(ValueError, match="c51 head.*c51dueling head"):
        VecBrain(256, **kw).load(str(tmp_path / "c51"))
    net = qnet_from_checkpoint(ck, max_batch=256)
    assert net.arch == "c51dueling" and net.support == (51, -5.0, 15.0)
    assert torch.equal(net.store_params(0).cpu(), torch.from_numpy(np.load(ck + ".npz")["online"]))
    res = evaluate(net, 512, max_steps=2000)
    assert (res.length > 0).all()
