"""C51 with prioritized replay (include/fbdqn.h FB_ALGO_C51_PER / FB_ALGO_C51_DOUBLE_PER) on the MI355X: the
importance-weighted loss, its gradients and the KL priorities against a float64 autograd restatement; isw = 1 gives the uniform C51
algos' results bit for bit; the ring-fed step and fb_vec_step equal their composed calls (prioritized memories, n = 1 and 3, both tree
modes); the tree leaves hold min(KL + 0.01, 1)^0.6; every refusal leaves the handles as they were; VecBrain checkpoints continue."""
import ctypes

import numpy as np
import pytest

from tests.test_c51_per_host import np_kl_priority, np_priority
from tests.test_gpu_c51 import FC, GAMMA, _batch, _check_grads, greedy_next, make_c51, ref_logits, support, torch_project
from tests.test_gpu_nstep_per import Tape, heaps, per_memory, push

pytestmark = pytest.mark.gpu
ALGOS = ("c51per", "c51doubleper")
BASE = {"c51per": "c51", "c51doubleper": "c51double"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def ref_train_weighted(p_on, p_tg, s, a, r, s2, t, w, G, algo, N, vmin, vmax, dev_astar, A=2, fc=FC):
    """-> (loss, flat gradient, KL per sample) in float64 with autograd: loss = mean_b w_b CE_b, KL_b = sum_{m_i > 0} m_i log(m_i / p_i)"""
    import torch
    P = torch.tensor(p_on, dtype=torch.float64, requires_grad=True)
    z = support(N, vmin, vmax)
    B = len(s)
    with torch.no_grad():
        pt = torch.softmax(ref_logits(torch.tensor(p_tg, dtype=torch.float64), s2, N, A, fc), -1)
        sel = torch.softmax(ref_logits(P.detach(), s2, N, A, fc), -1) if algo == "c51doubleper" else pt
        q = (sel * z).sum(-1)
        astar = greedy_next(q, dev_astar)
        m = torch_project(pt[torch.arange(B), astar], torch.as_tensor(r.astype(np.float64)), torch.as_tensor(t.astype(np.float64)),
                          G, N, vmin, vmax)
    logp = torch.log_softmax(ref_logits(P, s, N, A, fc)[torch.arange(B), torch.as_tensor(a, dtype=torch.long)], -1)
    ce = -(m * logp).sum(-1)
    loss = (torch.as_tensor(w, dtype=torch.float64) * ce).mean()
    loss.backward()
    kl = np_kl_priority(m.numpy(), logp.detach().exp().numpy())
    return loss.item(), P.grad.numpy(), kl


# ---------------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("B", [1, 32, 255, 256])
@pytest.mark.parametrize("algo", ALGOS)
def test_weighted_loss_gradients_and_kl_match_autograd(torch_cuda, algo, B):
    torch = torch_cuda
    import zlib
    N = 51
    net, p_on, p_tg = make_c51(N, max_batch=256)
    rng = np.random.default_rng(zlib.crc32(f"{algo}-{B}".encode()))
    s, a, r, s2, t = _batch(rng, B)
    w = (1.0 - rng.random(B)).astype(np.float32)                 # (0, 1]
    d = lambda x: torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if algo == "c51doubleper" else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w), gamma=GAMMA, flat_grad=grad)
    loss0, g0, kl0 = ref_train_weighted(p_on, p_tg, s, a, r, s2, t, w.astype(np.float64), GAMMA, algo, N, -10.0, 10.0, dev_astar)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    _check_grads(grad.cpu().numpy(), g0, 2 * N)
    ae = ae.cpu().numpy()
    assert (ae >= 0).all()
    np.testing.assert_allclose(ae, kl0, rtol=1e-4, atol=5e-4)
    assert torch.equal(net.store_params(), before)


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ALGOS)
def test_unit_weights_are_the_uniform_algo_bit_for_bit(torch_cuda, algo, B):
    torch = torch_cuda
    rng = np.random.default_rng(B + 7)
    n1, _, _ = make_c51(max_batch=256)
    n2, _, _ = make_c51(max_batch=256)
    for n in (n1, n2):
        n.set_hparams(lr=1e-4)
    ones = torch.ones(B, dtype=torch.float32, device="cuda")
    for _ in range(4):
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        l1, _, _ = n1.train_step(BASE[algo], s, a, r, s2, t, gamma=GAMMA, want_aux=False)
        l2, ae, _ = n2.train_step(algo, s, a, r, s2, t, isw=ones, gamma=GAMMA)
        assert torch.equal(l1, l2)
        assert torch.equal(n1.store_params(0), n2.store_params(0))
        assert (ae >= 0).all()
    m1, v1, p1 = n1.adam_state()
    m2, v2, p2 = n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)


# ---------------------------------------------------------------------------------------------------------------- ring-fed
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ALGOS)
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, algo, n):
    """fb_train_from_replay(isw) on a prioritized memory == fb_replay_gather + fb_qnet_train_step(isw, Gamma): a / R / done, loss,
    KL priorities, the exported gradient and the parameters after Adam"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    N, cap = 64, 1500
    rep = per_memory(cap, N, n)
    tape = Tape(N, seed=11, p_term=0.15)
    rep.reset(tape.frames[0])
    for _ in range(40):                                     # the tree wraps
        push([rep], tape)
    G = bootstrap_gamma(GAMMA, n)
    for B in (1, 32, 255):
        n1, _, _ = make_c51(max_batch=256)
        n2, _, _ = make_c51(max_batch=256)
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(3):
            idx, isw = rep.sample(B)
            idx = idx.clone(); isw = isw.clone()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, ae1, _ = n1.train_step(algo, s, a, r, s2, t, isw=isw, gamma=G, flat_grad=g1 if exp else None)
            l2, a2, r2, t2, ae2 = train_from_replay(rep, n2, algo, idx, gamma=GAMMA, flat_grad=g2 if exp else None, isw=isw,
                                                    want_abs_err=True)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert torch.equal(l1, l2) and torch.equal(ae1, ae2), (algo, n, B, step)
            if exp:
                assert torch.equal(g1, g2)
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params()), (algo, n, B, step)
            rep.update_priorities(idx, abs_err=ae2.clone())


# ---------------------------------------------------------------------------------------------------------------- the full step
def _pipeline(N, cap, mode, n, scaled=True, seed=5):
    from dqnflappybird_amd.vec import QNet, VecGameState
    env, rep = VecGameState(N, seed=seed), per_memory(cap, N, n, mode)
    if scaled:
        net, _, _ = make_c51(max_batch=N)
    else:                                                   # the library's own initialisation: near-uniform distributions
        net = QNet(2, FC, "c51", max_batch=N)
        net.init_params(3, which=0); net.init_params(4, which=1)
    net.set_hparams(lr=1e-4)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_vec_step_equals_separate_calls(torch_cuda, N, n, mode):
    """fb_vec_step(C51 with PER) == act -> frame_step -> push -> Memory.sample -> weighted train -> batch_update: actions, leaf
    indices, importance weights, losses and priorities step by step, parameters and the memory's whole state blob (tree included) at
    the end.  4096 envs take the run-ahead store, sample and batch_update (exact mode)."""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    algo = "c51doubleper" if n == 3 else "c51per"
    B = 32
    cap = 6 * N + 13
    steps = 16 if N == 4096 else 24
    e1, r1, n1, nib1 = _pipeline(N, cap, mode, n)
    e2, r2, n2, nib2 = _pipeline(N, cap, mode, n)
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
            assert torch.equal(r_, one.r) and torch.equal(t_, one.t), step
    assert r2.population == cap                             # the tree has wrapped
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(n1.store_params(), n2.store_params())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n2.split_stats() == (0, 0)                          # the one-stream schedule


@pytest.mark.parametrize("N", [256, 4096])
def test_tree_leaves_are_the_clipped_kl_priorities(torch_cuda, N):
    """after a step, the leaf of every sampled transition holds min(KL + 0.01, 1)^0.6 of the priority the step returned (the last
    write of a leaf drawn twice); near-uniform distributions keep many KL values under the clip"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep
    B, cap = 64, 6 * N + 13
    env, rep, net, _ = _pipeline(N, cap, "exact", 1, scaled=False)
    one = VecStep(env, rep, net, B, "c51per", GAMMA)
    under = 0
    for step in range(6):
        one(0.05, seed=1, step=step, train=True)
        torch.cuda.synchronize()
        tree = heaps(rep)[0]
        kl = one.abs_err.cpu().numpy()
        want = {}
        for i, k in zip(one.idx.cpu().tolist(), kl):
            want[i] = np_priority(k)
        got = tree[list(want)]
        np.testing.assert_allclose(got, np.array(list(want.values()), np.float64), rtol=1e-6, atol=0)
        under += int((np.array(list(want.values())) < 1.0).sum())
    assert under > 0


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
    ones = torch.ones(B, device="cuda")

    def frozen(net):
        m, v, p = net.adam_state()
        return net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), p.copy()

    def same(x, y):
        return all(torch.equal(i, j) if torch.is_tensor(i) else np.array_equal(i, j) for i, j in zip(x, y))

    before_c, before_p = frozen(c51), frozen(plain)
    for algo in ALGOS:
        with pytest.raises(ValueError, match="C51 net"):
            plain.train_step(algo, s, a, r, s2, t, isw=ones, gamma=GAMMA)
        with pytest.raises(ValueError, match="isw"):
            c51.train_step(algo, s, a, r, s2, t, gamma=GAMMA)
    torch.cuda.synchronize()
    assert same(frozen(c51), before_c) and same(frozen(plain), before_p)
    env = VecGameState(N, seed=1); env.track_state(); env.observe()
    per = VecReplay(20000, N, prioritized=True); per.reset(env.frame_bits)
    uni = VecReplay(20000, N); uni.reset(env.frame_bits)
    for _ in range(4):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        per.push(env.frame_bits, acts, env.reward, env.terminal)
        uni.push(env.frame_bits, acts, env.reward, env.terminal)
    blob, uni_blob, env_state = per.state_blob().copy(), uni.state_blob().copy(), env.get_state().copy()
    idx = torch.zeros(B, dtype=torch.int64, device="cuda")
    sc = ctypes.c_void_p
    for algo, code in (("c51per", L.ALGO_C51_PER), ("c51doubleper", L.ALGO_C51_DOUBLE_PER)):
        # a uniform memory
        with pytest.raises(ValueError, match="prioritized memory only"):
            train_from_replay(uni, c51, algo, idx, gamma=GAMMA, isw=ones)
        with pytest.raises(ValueError, match="prioritized memory"):
            VecStep(env, uni, c51, B, algo, GAMMA)
        # missing importance weights (the library itself)
        rc = L.lib().fb_train_from_replay(per.h, c51.h, code, B, L.ptr(idx), None, sc(1), sc(1), sc(1), GAMMA, sc(1), None, None,
                                          L.current_stream())
        assert rc == -1 and "importance weights" in L.lib().fb_last_error().decode()
        # fb_vec_step: a uniform memory, a scalar net, no isw buffers
        sb_per = VecStep(env, per, c51, B, algo, GAMMA).buf
        sb_uni = VecStep(env, uni, c51, B, "c51", GAMMA).buf
        rc = L.lib().fb_vec_step(env.h, uni.h, c51.h, ctypes.byref(sb_per), N, code, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
        assert rc == -1 and "do not match" in L.lib().fb_last_error().decode()
        rc = L.lib().fb_vec_step(env.h, per.h, plain.h, ctypes.byref(sb_per), N, code, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
        assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
        rc = L.lib().fb_vec_step(env.h, per.h, c51.h, ctypes.byref(sb_uni), N, code, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
        assert rc == -1 and "isw" in L.lib().fb_last_error().decode()
        # fb_train_steps (no weights) and fb_vec_step_dp (non-NULL dummies: the checks come before any pointer is used)
        rc = L.lib().fb_train_steps(per.h, c51.h, code, B, 1, 1, 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
        assert rc == -1 and "importance weights" in L.lib().fb_last_error().decode()
        rc = L.lib().fb_vec_step_dp(None, env.h, per.h, c51.h, None, N, code, B, 0.0, 0, 0, 1, GAMMA, 1, L.current_stream())
        assert rc == -1 and "data-parallel C51" in L.lib().fb_last_error().decode()
    # the uniform algos keep refusing a prioritized memory, and plain PER a C51 net
    rc = L.lib().fb_vec_step(env.h, per.h, c51.h, ctypes.byref(sb_per), N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "uniform memory only" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, per.h, c51.h, ctypes.byref(sb_per), N, L.ALGO_PER, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    torch.cuda.synchronize()
    assert np.array_equal(per.state_blob(), blob) and np.array_equal(uni.state_blob(), uni_blob)
    assert np.array_equal(env.get_state(), env_state)
    assert same(frozen(c51), before_c) and same(frozen(plain), before_p)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def test_vecbrain_c51doubleper_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo='c51doubleper', n_step=3): a prioritized 3-step memory and a C51 net; the target net is synced every
    replace_target_iter steps; save / load continues bit for bit; evaluate.qnet_from_checkpoint loads the checkpoint"""
    torch = torch_cuda
    from dqnflappybird_amd.evaluate import qnet_from_checkpoint
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="c51doubleper", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4, n_step=3, v_min=-5.0, v_max=15.0)
    a = VecBrain(256, **kw)
    assert a.replay.prioritized and a.replay.n_step[0] == 3 and a.net.support == (51, -5.0, 15.0)
    tgt0 = a.net.store_params(1).clone()
    a.run(20, log_every=0)
    assert not torch.equal(a.net.store_params(1), tgt0)      # synced (the reference PER agent never syncs: 'per' alone keeps that)
    while a.timeStep % a.replace_target_iter:
        a.step()
    a.step()                                                 # the sync happens before this step's training
    synced = a.net.store_params(1).clone()
    a.step()
    assert torch.equal(a.net.store_params(1), synced) and not torch.equal(a.net.store_params(0), synced)
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(10):
        a.step()
        ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.isw.clone(), a.one_step.loss.clone(),
                   a.one_step.abs_err.clone()))
    b = VecBrain(256, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(10):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.isw, b.one_step.loss, b.one_step.abs_err)
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0)) and torch.equal(a.net.store_params(1), b.net.store_params(1))
    assert np.array_equal(np.asarray(a.replay.state_blob()), np.asarray(b.replay.state_blob()))
    net = qnet_from_checkpoint(ck, max_batch=256)
    assert net.support == (51, -5.0, 15.0)
    assert torch.equal(net.store_params(0).cpu(), torch.from_numpy(np.load(ck + ".npz")["online"]))
