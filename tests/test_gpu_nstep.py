"""n-step returns (include/fbdqn.h fb_replay_set_n_step) on the MI355X: the n-step view of the replay ring against its one-step
view composed in numpy (tests/test_nstep_host.py's restatement), every training path that reads it against the gathered form, the
sampler against CPython, the oracle's gradients, and the argument checks."""
import random

import numpy as np
import pytest

from tests.test_nstep_host import nstep_return

pytestmark = pytest.mark.gpu
GAMMA = 0.99


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def played(N, cap, steps, seed=3, p_flap=0.05):
    """a memory filled by N games with a crash-heavy policy (rarely flapping: the birds hit the ground every ~20 frames)"""
    import torch
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env, rep = VecGameState(N, seed=seed), VecReplay(cap, N)
    env.observe(); rep.reset(env.frame_bits)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        acts = torch.from_numpy((rng.random(N) < p_flap).astype(np.uint8)).cuda()
        env.frame_step(acts, want_u8=False)
        rep.push(env.frame_bits, acts, env.reward, env.terminal)
    return env, rep


def composed(rep, idx, n, gamma):
    """(s, a, R, s', done, Gamma, one-step terminals [n, B]) of deque positions idx at n steps, from the SAME memory's one-step
    gathers at j + k N (the memory is switched to n = 1 for them and back to (n, gamma) afterwards)"""
    rep.set_n_step(1, gamma)
    rows = [[x.cpu().numpy().copy() for x in rep.gather((idx + k * rep.n).contiguous())] for k in range(n)]
    rep.set_n_step(n, gamma)
    R, done, G = nstep_return(np.stack([r[2] for r in rows]), np.stack([r[4] for r in rows]), gamma)
    return rows[0][0], rows[0][1], R, rows[n - 1][3], done, G, np.stack([r[4] for r in rows])


def test_n1_view_is_the_one_step_memory(torch_cuda):
    """set_n_step(1, gamma) on one of two identical pipelines: 64 fb_vec_steps (split schedule on) give the same actions, rewards,
    indices, losses and parameters as the memory that was never given the setter."""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
    N, B = 256, 32
    L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")

    def make(n1):
        env, rep, net = VecGameState(N, seed=5), VecReplay(20000, N), QNet(max_batch=N)
        rep.seed(9, "cpython"); net.init_params(3, which=0); net.init_params(4, which=1)
        if n1:
            rep.set_n_step(3, GAMMA); rep.set_n_step(1, 0.5)
            assert rep.n_step == (1, 0.0)
        env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, net, VecStep(env, rep, net, B, "nature", GAMMA)

    e1, n1, one = make(False)
    e2, n2, two = make(True)
    for step in range(64):
        train = step >= 6
        a1 = one(0.05, seed=1, step=step, train=train).clone()
        r1 = e1.reward.clone()
        a2 = two(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2) and torch.equal(r1, e2.reward), step
        if train:
            assert torch.equal(one.idx, two.idx) and torch.equal(one.loss, two.loss), step
    assert torch.equal(n1.store_params(), n2.store_params())
    assert n2.split_stats()[0] == 58


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("N", [1, 7, 256])
def test_sampler_draws_from_the_n_step_population(torch_cuda, n, N):
    """random.sample(range(min(len, cap) - (n - 1) N), B) bit for bit, on a memory not yet full and on one that has wrapped; the
    Philox sampler stays inside the population too"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecReplay
    cap = 20 * N
    rep = VecReplay(cap, N)
    rep.set_n_step(n, GAMMA)
    g = torch.Generator(device="cuda").manual_seed(1)
    bits = torch.randint(0, 2 ** 62, (N, 100), device="cuda", generator=g)
    rep.reset(bits)
    acts, rews, terms = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda")
    seed = 100 * n + N
    for pushes in (12, 31):                                            # 12 N < cap: not full; 12 + 31 > 20: wrapped
        for _ in range(pushes):
            rep.push(torch.randint(0, 2 ** 62, (N, 100), device="cuda", generator=g), acts, rews, terms)
        pop = min(len(rep), cap) - (n - 1) * N
        assert rep.population == pop and pop > 0
        B = min(32, pop)
        rep.seed(seed, "cpython"); random.seed(seed)
        for _ in range(3):
            idx, _ = rep.sample(B)
            assert idx.cpu().tolist() == random.sample(range(pop), B), (pushes, pop)
        rep.seed(seed, "philox")
        idx, _ = rep.sample(B)
        h = idx.cpu().numpy()
        assert h.min() >= 0 and h.max() < pop
        assert len(rep) == min((12 + (pushes == 31) * 31) * N, cap)


def test_population_smaller_than_batch_fails_loudly(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd._lib import FbError
    from dqnflappybird_amd.vec import VecReplay
    N = 7
    rep = VecReplay(700, N)
    rep.set_n_step(3, GAMMA)
    rep.reset(torch.zeros((N, 100), dtype=torch.int64, device="cuda"))
    z8, zf = torch.zeros(N, dtype=torch.uint8, device="cuda"), torch.zeros(N, device="cuda")
    for _ in range(3):
        rep.push(torch.zeros((N, 100), dtype=torch.int64, device="cuda"), z8, zf, z8)
    assert len(rep) == 21 and rep.population == 7
    rep.sample(7)
    assert len(rep) == 21                                  # 7 of 7: fine
    rep.sample(8)
    with pytest.raises(FbError, match="Sample larger than population"):
        len(rep)


@pytest.mark.parametrize("n,capmult", [(2, 2), (3, 30), (5, 5), (5, 40)])
def test_gather_equals_composed_one_step_gathers(torch_cuda, n, capmult):
    """n-step fb_replay_gather of the whole population and of a drawn minibatch == the numpy composition of one-step gathers of the
    same memory at j + k N: s, a, s', R (float32 of the float64 sum) and done, bit for bit; capacities down to n N (the ring's last
    spare slots); a crash-heavy policy so that the set holds terminals at every offset k and transitions without one"""
    torch = torch_cuda
    N = 64
    _, rep = played(N, capmult * N, 60)
    rep.set_n_step(n, GAMMA)
    pop = rep.population
    assert pop == min(60 * N, capmult * N) - (n - 1) * N
    full = torch.arange(pop, device="cuda")
    rep.seed(2, "cpython")
    drawn, _ = rep.sample(min(64, pop))
    terms_full = None
    for idx in (full, drawn.clone()):
        s, a, r, s2, t = (x.cpu().numpy().copy() for x in rep.gather(idx))
        s0, a0, R0, s20, d0, _, terms = composed(rep, idx, n, GAMMA)
        terms_full = terms if terms_full is None else terms_full
        assert np.array_equal(s, s0) and np.array_equal(a, a0) and np.array_equal(s2, s20)
        assert np.array_equal(r.view(np.uint32), R0.view(np.uint32)) and np.array_equal(t, d0)
    # (the full population of the larger memories) terminals at every offset, and windows without any
    first = np.where(terms_full.any(0), terms_full.argmax(0), -1)
    if pop >= 1000:
        assert all((first == k).any() for k in range(n)) and (first < 0).any(), np.bincount(first + 1)


def _ring_vs_gathered(torch, rep, algo, arch, dtype, B, n, rng):
    from dqnflappybird_amd.vec import QNet, bootstrap_gamma, train_from_replay
    G = bootstrap_gamma(GAMMA, n)
    n1, n2 = QNet(max_batch=max(B, 2), arch=arch), QNet(max_batch=max(B, 2), arch=arch)
    for net in (n1, n2):
        net.init_params(7, which=0); net.init_params(8, which=1); net.set_hparams(lr=1e-4); net.set_train_dtype(dtype)
    pop = rep.population
    g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
    for step in range(3):
        idx = torch.from_numpy(rng.integers(0, pop, B)).cuda()
        idx[0] = pop - 1 if step else 0                                 # newest / oldest complete transition
        s, a, r, s2, t = rep.gather(idx)
        exp = step == 0                                                 # first step: the exported gradient, then Adam on it
        l1, _, _ = n1.train_step(algo, s, a, r, s2, t, gamma=G, flat_grad=g1 if exp else None, want_aux=False)
        l2, a2, r2, t2 = train_from_replay(rep, n2, algo, idx, gamma=GAMMA, flat_grad=g2 if exp else None)
        assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
        assert torch.equal(l1, l2), (algo, arch, dtype, B, step)
        if exp:
            assert torch.equal(g1, g2)
            n1.apply_adam(g1); n2.apply_adam(g2)
        assert torch.equal(n1.store_params(), n2.store_params())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["plain", "dueling"])
@pytest.mark.parametrize("algo", ["dqn", "nature", "double"])
def test_ring_fed_equals_gather_plus_train_step_with_Gamma(torch_cuda, algo, arch, dtype):
    """fb_train_from_replay at n = 3 == fb_replay_gather + fb_qnet_train_step(gamma = Gamma), bit for bit: a / R / done, loss, flat
    gradient and parameters after Adam, at B = 1, 32 and 255 (both conv trunk shapes of the ring-fed kernel)"""
    torch = torch_cuda
    _, rep = played(64, 1500, 40)                                         # the ring wraps
    rep.set_n_step(3, GAMMA)
    rng = np.random.default_rng(1)
    for B in (1, 32, 255):
        _ring_vs_gathered(torch, rep, algo, arch, dtype, B, 3, rng)


@pytest.mark.parametrize("algo,dueling", [("dqn", False), ("nature", False), ("double", True)])
def test_ring_fed_n_step_gradients_match_oracle(torch_cuda, oracle, algo, dueling):
    """the ring-fed n = 3 step's gradient against the oracle's train step fed the composed tuple (s, a, R, s', done) and Gamma, within
    the bounds of test_ring_fed_train_step_gradients_match_oracle"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, train_from_replay
    from tests.test_gpu_qnet import trained_like_params
    n, B = 3, 32
    _, rep = played(64, 4000, 50, p_flap=0.12)
    rep.set_n_step(n, GAMMA)
    cfg = oracle.qcfg(512, 2, dueling)
    p_on, p_tg = trained_like_params(oracle, cfg, 1), trained_like_params(oracle, cfg, 2)
    net = QNet(2, 512, "dueling" if dueling else "plain", max_batch=B)
    net.load_params(p_on, 0); net.load_params(p_tg, 1)
    rng = np.random.default_rng(5)
    for _ in range(60):                                                   # kink-free minibatch (see test_train_step_gradients_match_oracle)
        idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
        s, a, R, s2, done, G, _ = composed(rep, idx, n, GAMMA)
        oracle.forward(p_on, cfg, s)
        if oracle.last_margin(nonzero=True) > 2e-5:
            break
    else:
        pytest.fail("no kink-free batch found")
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, a2, r2, t2 = train_from_replay(rep, net, algo, idx, gamma=GAMMA, flat_grad=grad)
    assert np.array_equal(r2.cpu().numpy(), R) and np.array_equal(t2.cpu().numpy(), done) and np.array_equal(a2.cpu().numpy(), a)
    q, acts = oracle.forward(p_on, cfg, s, keep=True)
    if algo == "dqn":
        qn = oracle.forward(p_on, cfg, s2).max(1)
    elif algo == "double":
        am = oracle.forward(p_on, cfg, s2).argmax(1)
        qn = oracle.forward(p_tg, cfg, s2)[np.arange(B), am]
    else:
        qn = oracle.forward(p_tg, cfg, s2).max(1)
    _, loss0, _, dq = oracle.dqn_loss({"dqn": 0, "nature": 1, "double": 1}[algo], q, qn, a, R, done, gamma=G)
    g0 = oracle.backward(p_on, cfg, s, acts, dq)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    g = grad.cpu().numpy()
    bounds = [0, 8192, 8224, 40992, 41056, 77920, 77984, 77984 + 1600 * 512, 77984 + 1600 * 512 + 512, net.n_params]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        scale = np.abs(g0[lo:hi]).max()
        assert scale > 0
        np.testing.assert_allclose(g[lo:hi], g0[lo:hi], rtol=2e-3, atol=2e-5 * scale, err_msg=f"params[{lo}:{hi}]")


def _pipeline(N, cap, B, algo, n, seed=5, grad=False):
    import torch
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
    env, rep, net = VecGameState(N, seed=seed), VecReplay(cap, N), QNet(max_batch=max(N, B))
    rep.seed(9, "cpython"); net.init_params(3, which=0); net.init_params(4, which=1)
    rep.set_n_step(n, GAMMA)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    g = torch.zeros(net.n_params, device="cuda") if grad else None
    return env, rep, net, nib, g


def test_vec_step_n3_equals_separate_calls(torch_cuda):
    """fb_vec_step at n = 3 (split schedule, ring-fed train step) == act_nib -> frame_step -> push -> sample -> train_from_replay over
    100 steps: actions, indices, a / R / done, loss, parameters"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    N, B, steps = 256, 32, 100
    e1, r1, n1, nib1, _ = _pipeline(N, 20000, B, "nature", 3)
    e2, r2, n2, nib2, _ = _pipeline(N, 20000, B, "nature", 3)
    one = VecStep(e2, r2, n2, B, "nature", GAMMA)
    for step in range(steps):
        train = step >= 6
        if train and step % 20 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, _ = r1.sample(B)
            loss, a, r, t = train_from_replay(r1, n1, "nature", idx, gamma=GAMMA)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(a, one.a) and torch.equal(r, one.r) and torch.equal(t, one.t), step
    assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all()
    issued, clean = n2.split_stats()
    assert issued == steps - 6 and 0 < clean < issued, (issued, clean)


@pytest.mark.parametrize("N,capmult,steps", [(256, 64, 200), (1024, 48, 200), (4096, 40, 200)])
def test_split_schedule_equals_one_stream_at_n3(torch_cuda, N, capmult, steps):
    """the split schedule at n = 3 == the one-stream order, bit for bit, over 200 steps, in a memory small enough that dirty draws
    (a minibatch holding a transition whose row / frame the step's own push writes) are common; both kinds occur and no wait gives up"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecStep
    B = 32
    e1, r1, n1, nib1, _ = _pipeline(N, capmult * N, B, "nature", 3, seed=11)
    e2, r2, n2, nib2, _ = _pipeline(N, capmult * N, B, "nature", 3, seed=11)
    one, two = VecStep(e1, r1, n1, B, "nature", GAMMA), VecStep(e2, r2, n2, B, "nature", GAMMA)
    try:
        for step in range(steps):
            train = step >= 4
            if train and step % 25 == 0:
                n1.sync_target(); n2.sync_target()
            L.check(L.lib().fb_vec_step_set_schedule(0), "schedule")
            a1 = one(0.05, seed=2, step=step, train=train).clone()
            L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
            a2 = two(0.05, seed=2, step=step, train=train)
            assert torch.equal(a1, a2), step
            if train:
                assert torch.equal(one.idx, two.idx) and torch.equal(one.loss, two.loss) and torch.equal(one.r, two.r), step
    finally:
        L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
    assert torch.equal(n1.store_params(), n2.store_params()) and np.array_equal(r1.state_blob(), r2.state_blob())
    issued, clean = n2.split_stats()                      # (raises if a wait between the two streams gave up)
    assert issued == steps - 4 and 0 < clean < issued, (issued, clean)


def test_train_steps_n3_equals_separate_calls_and_replays_from_a_graph(torch_cuda):
    """fb_train_steps(8) at n = 3 == 8 x (sample + train_from_replay); and fb_train_steps captured into a hipGraph and replayed twice
    gives what the eager calls give"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, TrainSteps, train_from_replay
    N, B = 256, 32

    def make():
        _, rep = played(N, 20000, 14, seed=5)
        rep.seed(9, "cpython"); rep.set_n_step(3, GAMMA)
        net = QNet(max_batch=N); net.init_params(3); net.init_params(4, which=1)
        return rep, net, TrainSteps(rep, net, B, "nature", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    for _ in range(8):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "nature", idx, gamma=GAMMA)
    ts2(8)
    assert torch.equal(n1.store_params(), n2.store_params())
    nxt1, _ = r1.sample(B)
    assert torch.equal(nxt1, r2.sample(B)[0])                 # the generators are in the same place
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


def test_vec_step_dp_world1_n3_equals_fused(torch_cuda):
    """fb_vec_step_dp at world size 1 on an n = 3 memory == fb_vec_step with Adam fused, bit for bit"""
    torch = torch_cuda
    from dqnflappybird_amd.dist import NativeDP
    from dqnflappybird_amd.vec import VecStep
    N, B, steps = 256, 32, 30
    nd = NativeDP(rank=0, world=1, overlap=False)
    try:
        e1, r1, n1, _, _ = _pipeline(N, 20000, B, "dqn", 3)
        e2, r2, n2, _, g2 = _pipeline(N, 20000, B, "dqn", 3, grad=True)
        fused, dp = VecStep(e1, r1, n1, B, "dqn", GAMMA), VecStep(e2, r2, n2, B, "dqn", GAMMA, flat_grad=g2, dist=nd)
        for step in range(steps):
            train = step >= 6
            a1 = fused(0.05, seed=1, step=step, train=train).clone()
            a2 = dp(0.05, seed=1, step=step, train=train)
            assert torch.equal(a1, a2), step
            if train:
                assert torch.equal(fused.idx, dp.idx) and torch.equal(fused.loss, dp.loss), step
        assert torch.equal(n1.store_params(), n2.store_params())
    finally:
        torch.cuda.synchronize()
        nd.close()


def test_vecbrain_n_step_checkpoints(torch_cuda, tmp_path):
    """VecBrain(n_step=3): save / load continues bit for bit; a VecBrain of another n refuses the checkpoint; a checkpoint without
    n_step (written before n-step returns existed) loads as n = 1"""
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="nature", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4)
    a = VecBrain(256, n_step=3, **kw)
    assert a.replay.n_step == (3, 0.99)
    a.run(20, log_every=0)
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(10):
        a.step(); ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.loss.clone()))
    b = VecBrain(256, n_step=3, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(10):
        b.step()
        assert torch.equal(b.one_step.actions, ta[i][0]) and torch.equal(b.one_step.idx, ta[i][1]) and torch.equal(b.one_step.loss, ta[i][2]), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0))
    with pytest.raises(ValueError, match="n_step"):
        VecBrain(256, **kw).load(ck)
    z = dict(np.load(ck + ".npz"))
    assert int(z.pop("n_step")[0]) == 3
    np.savez(str(tmp_path / "old.npz"), **z)
    VecBrain(256, **kw).load(str(tmp_path / "old"))           # an n_step-less checkpoint is a one-step one
    with pytest.raises(ValueError, match="n_step"):
        VecBrain(256, n_step=3, **kw).load(str(tmp_path / "old"))


def test_rejected_arguments_leave_the_memory_alone(torch_cuda):
    """n outside 1..16, a prioritized memory, capacity < n N, and a training call whose gamma is not the memory's: FB_ERR_INVALID
    (ValueError), and the push counter, the view and the pipeline stay as they were"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, TrainSteps, VecGameState, VecReplay, VecStep, train_from_replay
    N, B = 64, 32
    env, rep, net = VecGameState(N, seed=5), VecReplay(5000, N), QNet(max_batch=N)
    rep.seed(9, "cpython"); net.init_params(3)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    rep.set_n_step(3, GAMMA)
    for bad in (0, 17):
        with pytest.raises(ValueError):
            rep.set_n_step(bad, GAMMA)
    assert rep.n_step == (3, GAMMA)
    with pytest.raises(ValueError):
        VecReplay(5000, N, prioritized=True).set_n_step(3, GAMMA)
    small = VecReplay(2 * N, N)
    with pytest.raises(ValueError):
        small.set_n_step(3, GAMMA)
    assert small.n_step == (1, 0.0)
    small.set_n_step(2, GAMMA)                            # cap = n N exactly is fine
    good, wrong = VecStep(env, rep, net, B, "dqn", GAMMA), VecStep(env, rep, net, B, "dqn", 0.98)
    for step in range(4):
        good(0.0, step=step, train=False)
    size, state, params = len(rep), env.get_state().copy(), net.store_params().clone()
    with pytest.raises(ValueError, match="gamma"):
        wrong(0.0, step=4, train=True)
    with pytest.raises(ValueError, match="gamma"):
        wrong(0.0, step=4, train=False)
    idx, _ = rep.sample(B)
    with pytest.raises(ValueError, match="gamma"):
        train_from_replay(rep, net, "dqn", idx, gamma=0.5)
    with pytest.raises(ValueError, match="gamma"):
        TrainSteps(rep, net, B, "dqn", 0.5)(2)
    assert len(rep) == size and (env.get_state() == state).all() and torch.equal(net.store_params(), params)
    good(0.0, step=4, train=True)                         # and the pipeline carries on
    assert len(rep) == size + N


def test_vec_step_n3_gather_and_own_draw_equal_separate_calls(torch_cuda):
    """the one-stream forms of fb_vec_step that its input selects at n = 3 == act_nib -> frame_step -> push -> sample ->
    train_from_replay over 40 steps: below 256 envs (64, CPython generator) the gather + train step with Gamma, with a generator that
    cannot ride in the env launch (256 envs, philox) the draw as a launch of its own; actions, indices, a / R / done, loss, parameters"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 40
    for N, rng in ((64, "cpython"), (256, "philox")):
        e1, r1, n1, nib1, _ = _pipeline(N, 20000, B, "nature", 3)
        e2, r2, n2, nib2, _ = _pipeline(N, 20000, B, "nature", 3)
        r1.seed(9, rng); r2.seed(9, rng)
        one = VecStep(e2, r2, n2, B, "nature", GAMMA)
        for step in range(steps):
            train = step >= 6
            a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
            e1.frame_step(a1, want_u8=False)
            r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
            if train:
                idx, _ = r1.sample(B)
                loss, a, r, t = train_from_replay(r1, n1, "nature", idx, gamma=GAMMA)
            a2 = one(0.05, seed=1, step=step, train=train)
            assert torch.equal(a1, a2), (N, step)
            if train:
                assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), (N, step)
                assert torch.equal(a, one.a) and torch.equal(r, one.r) and torch.equal(t, one.t), (N, step)
        assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all(), N
        assert n2.split_stats()[0] == 0, N                   # (neither input takes the split schedule)
