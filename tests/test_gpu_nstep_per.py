"""Prioritized memories with n-step returns (include/fbdqn.h fb_replay_create_nstep) on the MI355X: the tree of an n = 3 memory is the
tree of an n = 1 memory two pushes behind (and the reference's SumTree driven with the lagged stores), every leaf reads the transition
the header names with its n-step return (a numpy restatement over the recorded pushes), the ring-fed train step and fb_vec_step equal
the separate calls, the state blob and VecBrain checkpoints continue bit for bit, and every refusal leaves the memory as it was."""

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


def per_memory(cap, N, n, mode="exact", seed=9):
    from dqnflappybird_amd.vec import VecReplay
    rep = VecReplay(cap, N, prioritized=True, n_step=n, gamma=GAMMA)
    rep.set_per_mode(mode)
    rep.seed(seed, "numpy")
    return rep


class Tape:
    """random pushes (frames, actions, rewards, terminals), kept on the host as well: frames[f] is frame f (0 = the reset frame), rows[t]
    the (a, r, term) row push t + 1 wrote"""

    def __init__(self, N, seed, p_term=0.25):
        import torch
        self.N, self.rng, self.p_term = N, np.random.default_rng(seed), p_term
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.frames, self.acts, self.rews, self.terms = [], [], [], []
        self.frames.append(self._bits())

    def _bits(self):
        import torch
        return torch.randint(-2 ** 62, 2 ** 62, (self.N, 100), device="cuda", generator=self.g, dtype=torch.int64)

    def next(self):
        import torch
        N = self.N
        bits = self._bits()
        a = self.rng.integers(0, 2, N).astype(np.uint8)
        r = self.rng.choice(np.array([0.1, 1.0, -1.0], np.float32), N)
        t = (self.rng.random(N) < self.p_term).astype(np.uint8)
        self.frames.append(bits); self.acts.append(a); self.rews.append(r); self.terms.append(t)
        return bits, torch.from_numpy(a).cuda(), torch.from_numpy(r).cuda(), torch.from_numpy(t).cuda()


def push(reps, tape):
    x = tape.next()
    for rp in reps:
        rp.push(*x)


def heaps(rep):
    """(tree, maxt, mint) f64[2 cap - 1] each: the last three parts of the state blob (fb_replay.hip blob_parts, 16-byte padded)"""
    blob = np.asarray(rep.state_blob())
    nb = 8 * (2 * rep.capacity - 1)
    pad = (nb + 15) & ~15
    end = blob.size
    out = []
    for k in (3, 2, 1):
        lo = end - k * pad
        out.append(blob[lo:lo + nb].view(np.float64).copy())
    return out


def assert_same_tree(a, b, what):
    ha, hb = heaps(a), heaps(b)
    for x, y, name in zip(ha, hb, ("tree", "maxt", "mint")):
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (what, name)
    assert a.per_state(want_tree=False)[1:] == b.per_state(want_tree=False)[1:], what      # data_pointer, size, beta


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("N", [1, 7, 64, 1024])
def test_lag_identity(torch_cuda, N, mode):
    """a prioritized n = 3 memory after S pushes == an n = 1 memory after S - 2 pushes of the same tape: tree, maxt, mint, pointer, size,
    beta byte for byte at every S, through several wraps of a small capacity (not a multiple of N), with Memory.sample (same uniforms)
    giving the same leaves and weights and Memory.batch_update applied to both"""
    torch = torch_cuda
    n = 3
    cap = 5 * N + 3 if N > 1 else 8
    a, b = per_memory(cap, N, n, mode), per_memory(cap, N, 1, mode)
    assert a.n_step == (3, GAMMA) and b.n_step == (1, 0.0)
    tape = Tape(N, seed=N)
    a.reset(tape.frames[0]); b.reset(tape.frames[0])
    rng = np.random.default_rng(100 + N)
    lagged = []
    S_total = 4 * ((cap + N - 1) // N) + n + 2
    for S in range(1, S_total + 1):
        x = tape.next()
        a.push(*x)
        lagged.append(x)
        if S >= n:
            b.push(*lagged[S - n])                         # (only the tree is compared: what b stores in its ring does not matter)
        else:
            assert a.population == 0
        assert_same_tree(a, b, S)
        assert a.population == min(max(0, S - n + 1) * N, cap) and len(a) == min(S * N, cap)
        if S >= n and S % 3 == 0:
            B = 32
            u = torch.from_numpy(rng.random(B)).cuda()
            (ia, wa), (ib, wb) = a.sample(B, uniforms=u), b.sample(B, uniforms=u)
            assert torch.equal(ia, ib) and torch.equal(wa, wb), S
            ps = torch.from_numpy((rng.random(B).astype(np.float32) * 1.2 + 0.01).clip(max=1.0) ** np.float32(0.6)).cuda()
            a.update_priorities(ia.clone(), priorities=ps); b.update_priorities(ib.clone(), priorities=ps)
            assert_same_tree(a, b, ("update", S))
    a.seed(4, "numpy"); b.seed(4, "numpy")                   # the memory's own generator (np.random.uniform's stream)
    (ia, wa), (ib, wb) = a.sample(16), b.sample(16)
    assert torch.equal(ia, ib) and torch.equal(wa, wb)


def test_lag_identity_against_the_reference_sumtree(torch_cuda, oracle):
    """N = 1, exact mode: the n = 3 memory's tree bytes, pointer and size are the reference SumTree's after one store per push from the
    third on; Memory.sample with the same uniforms picks the same leaves with the same weights"""
    torch = torch_cuda
    n, cap = 3, 8
    rep = per_memory(cap, 1, n)
    mem = oracle.Memory(cap)
    tape = Tape(1, seed=5)
    rep.reset(tape.frames[0])
    rng = np.random.default_rng(3)
    for S in range(1, 40):
        push([rep], tape)
        if S >= n:
            mem.store(1)
        tree, ptr, size, _ = rep.per_state()
        assert (ptr, size) == (mem.data_pointer, mem.size), S
        assert np.array_equal(tree.view(np.uint64), mem.tree.view(np.uint64)), S
        if S >= n and S % 4 == 0:
            u = rng.random(4)
            idx, isw = rep.sample(4, uniforms=torch.from_numpy(u).cuda())
            oi, ow = mem.sample(4, u=u)
            assert idx.cpu().tolist() == list(oi)
            np.testing.assert_allclose(isw.cpu().numpy(), ow, rtol=1e-13)
            ps = (rng.random(4).astype(np.float32) * 1.2 + 0.01).clip(max=1.0) ** np.float32(0.6)
            rep.update_priorities(idx, priorities=torch.from_numpy(ps).cuda())
            mem.batch_update_p(oi, ps)


def unpack(bits_row):
    """u8[80, 80] of a packed frame (bit p of the 6400-bit row-major image)"""
    return (np.unpackbits(np.ascontiguousarray(bits_row).view(np.uint8), bitorder="little").reshape(80, 80) * 255).astype(np.uint8)


def expected(tape, frames_h, cap, N, n, S, idx):
    """numpy restatement of the header: leaf -> transition (t, e) -> (s, a, R, s', done)"""
    C = max(0, S - n + 1) * N
    rews, terms, acts = np.stack(tape.rews), np.stack(tape.terms), np.stack(tape.acts)
    out = []
    for j in idx:
        d = int(j) - (cap - 1)
        assert 0 <= d < min(C, cap)
        g = d + cap * ((C - 1 - d) // cap)
        t, e = divmod(g, N)
        fr = lambda f: unpack(frames_h[max(f, 0)][e])
        s = np.stack([fr(f) for f in range(t - 3, t + 1)], axis=-1)
        s2 = np.stack([fr(f) for f in range(t + n - 3, t + n + 1)], axis=-1)
        R, done, _ = nstep_return(rews[t:t + n, e:e + 1], terms[t:t + n, e:e + 1], GAMMA)
        w = terms[t:t + n, e]
        out.append((s, acts[t, e], R[0], s2, done[0], int(w.argmax()) if w.any() else -1))
    return out


@pytest.mark.parametrize("N,cap", [(7, 96), (64, 613), (1, 10)])
def test_gathered_leaves_are_the_header_transitions(torch_cuda, N, cap):
    """fb_replay_gather of every filled leaf == the numpy restatement over the recorded pushes: (s, a, R, s', done) bit for bit, R the
    float32 of the float64 sum; before the tree fills, right after each wrap (the oldest leaves), at capacities not a multiple of N; a
    crash-heavy tape puts terminals at every offset of the 3-step window.  A leaf >= min(C, cap) raises the error flag."""
    torch = torch_cuda
    from dqnflappybird_amd._lib import FbError
    n = 3
    rep = per_memory(cap, N, n)
    tape = Tape(N, seed=cap)
    rep.reset(tape.frames[0])
    frames_h = [tape.frames[0].cpu().numpy().view(np.uint64)]
    T = (cap + N - 1) // N
    checks = {n, n + 1, n + T - 1, n + T, n + T + 1, n + 2 * T, n + 2 * T + 1, n + 3 * T + 2}
    firsts = set()                                          # offsets of the first terminal in the windows checked (-1: none)
    for S in range(1, max(checks) + 1):
        push([rep], tape)
        frames_h.append(tape.frames[-1].cpu().numpy().view(np.uint64))
        if S not in checks:
            continue
        pop = rep.population
        assert pop == min((S - n + 1) * N, cap)
        idx = torch.arange(cap - 1, cap - 1 + pop, device="cuda")
        s, a, r, s2, t = (x.cpu().numpy().copy() for x in rep.gather(idx))
        for b, (es, ea, eR, es2, ed, first) in enumerate(expected(tape, frames_h, cap, N, n, S, idx.cpu().numpy())):
            assert np.array_equal(s[b], es) and np.array_equal(s2[b], es2), (S, b)
            assert a[b] == ea and r[b].view(np.uint32) == np.float32(eR).view(np.uint32) and t[b] == ed, (S, b)
            firsts.add(first)
        assert len(rep) == min(S * N, cap)                  # (no error flag raised)
        if pop < cap:                                       # the first leaf past the filled ones
            rep.gather(torch.tensor([cap - 1 + pop], device="cuda"))
            with pytest.raises(ValueError, match="out of range"):
                len(rep)
    rep.gather(torch.tensor([2 * cap - 1], device="cuda"))      # past the last leaf
    with pytest.raises(ValueError, match="out of range"):
        len(rep)
    assert firsts == {-1, 0, 1, 2}


def test_index_past_an_empty_tree_raises_the_flag(torch_cuda):
    torch = torch_cuda
    rep = per_memory(30, 4, 3)
    tape = Tape(4, seed=1)
    rep.reset(tape.frames[0])
    push([rep], tape); push([rep], tape)                    # two pushes: C = 0
    assert rep.population == 0
    rep.gather(torch.tensor([29], device="cuda"))
    with pytest.raises(ValueError, match="out of range"):
        len(rep)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("arch", ["plain", "dueling"])
def test_ring_fed_per_step_equals_gather_plus_train_step(torch_cuda, arch, dtype):
    """fb_train_from_replay with importance weights at n = 3 == fb_replay_gather + fb_qnet_train_step(isw, gamma = Gamma), bit for bit:
    a / R / done, loss, |TD errors|, the exported gradient and the parameters after Adam, at B = 1, 32 and 255"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, bootstrap_gamma, train_from_replay
    N, cap, n = 64, 1500, 3
    rep = per_memory(cap, N, n)
    tape = Tape(N, seed=11, p_term=0.15)
    rep.reset(tape.frames[0])
    for _ in range(40):                                     # the tree wraps
        push([rep], tape)
    G = bootstrap_gamma(GAMMA, n)
    for B in (1, 32, 255):
        n1, n2 = QNet(max_batch=max(B, 2), arch=arch), QNet(max_batch=max(B, 2), arch=arch)
        for net in (n1, n2):
            net.init_params(7, which=0); net.init_params(8, which=1); net.set_hparams(lr=1e-4); net.set_train_dtype(dtype)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(3):
            idx, isw = rep.sample(B)
            idx = idx.clone(); isw = isw.clone()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, ae1, _ = n1.train_step("per", s, a, r, s2, t, isw=isw, gamma=G, flat_grad=g1 if exp else None, want_aux=True)
            l2, a2, r2, t2, ae2 = train_from_replay(rep, n2, "per", idx, gamma=GAMMA, flat_grad=g2 if exp else None, isw=isw,
                                                    want_abs_err=True)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert torch.equal(l1, l2) and torch.equal(ae1, ae2), (arch, dtype, B, step)
            if exp:
                assert torch.equal(g1, g2)
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params())
            rep.update_priorities(idx, abs_err=ae2.clone())


def _per_pipeline(N, cap, mode, n=3, seed=5):
    from dqnflappybird_amd.vec import QNet, VecGameState
    env, rep, net = VecGameState(N, seed=seed), per_memory(cap, N, n, mode), QNet(max_batch=N)
    net.init_params(3, which=0); net.init_params(4, which=1)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_vec_step_per_n3_equals_separate_calls(torch_cuda, N, mode):
    """fb_vec_step(algo = PER) at n = 3 == act -> frame_step -> push -> Memory.sample -> ring-fed weighted train -> batch_update, over
    enough steps to wrap the tree, training from the first step that can (the third push): actions, leaf indices, importance weights,
    losses, |TD errors| step by step, parameters and the whole state blob (ring, counters, generator, tree heaps) at the end.  4096 envs
    take the run-ahead store, sample and batch_update (exact mode)."""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, n = 32, 3
    cap = 6 * N + 13
    steps = 16 if N == 4096 else 24
    e1, r1, n1, nib1 = _per_pipeline(N, cap, mode)
    e2, r2, n2, nib2 = _per_pipeline(N, cap, mode)
    one = VecStep(e2, r2, n2, B, "per", GAMMA)
    for step in range(steps):
        train = step >= n - 1
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
            loss, a_, r_, t_, ae = train_from_replay(r1, n1, "per", idx, gamma=GAMMA, isw=isw, want_abs_err=True)
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


def test_state_blob_round_trip_and_refusals(torch_cuda):
    """the replay blob of an n = 3 prioritized memory continues bit for bit in a fresh n = 3 memory; an n = 1 memory refuses it and an
    n = 3 memory refuses an n = 1 blob, naming n, and both are left as they were"""
    torch = torch_cuda
    N, cap = 16, 200
    a = per_memory(cap, N, 3)
    tape = Tape(N, seed=21)
    a.reset(tape.frames[0])
    for _ in range(20):
        push([a], tape)
    blob = np.asarray(a.state_blob()).copy()
    b = per_memory(cap, N, 3, seed=77)
    b.load_state_blob(blob)
    assert np.array_equal(np.asarray(b.state_blob()), blob)
    for k in range(6):
        push([a, b], tape)
        (ia, wa), (ib, wb) = a.sample(8), b.sample(8)
        assert torch.equal(ia, ib) and torch.equal(wa, wb), k
        ae = torch.rand(8, device="cuda")
        a.update_priorities(ia.clone(), abs_err=ae.clone()); b.update_priorities(ib.clone(), abs_err=ae.clone())
    assert np.array_equal(np.asarray(a.state_blob()), np.asarray(b.state_blob()))
    one = per_memory(cap, N, 1)
    before = np.asarray(one.state_blob()).copy()
    with pytest.raises(ValueError, match="n = 3"):
        one.load_state_blob(blob)
    assert np.array_equal(np.asarray(one.state_blob()), before)
    three = per_memory(cap, N, 3)
    before = np.asarray(three.state_blob()).copy()
    with pytest.raises(ValueError, match="n = 1"):
        three.load_state_blob(np.asarray(one.state_blob()))
    assert np.array_equal(np.asarray(three.state_blob()), before)


def test_vecbrain_per_n_step_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo = 'per', n_step = 3) trains, saves, and a fresh VecBrain continues from the checkpoint bit for bit; a VecBrain of
    another n refuses it"""
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="per", batch=32, capacity=6000, observe=2, seed=3)
    a = VecBrain(256, n_step=3, **kw)
    assert a.replay.n_step == (3, 0.99) and a.replay.prioritized
    a.run(30, log_every=0)
    assert a.last_loss is not None and a.replay.population == 6000
    ck = str(tmp_path / "ck")
    a.save(ck)
    ta = []
    for _ in range(8):
        a.step(); ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.isw.clone(), a.one_step.loss.clone()))
    b = VecBrain(256, n_step=3, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(8):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.isw, b.one_step.loss)
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0))
    assert np.array_equal(np.asarray(a.replay.state_blob()), np.asarray(b.replay.state_blob()))
    with pytest.raises(ValueError, match="n_step"):
        VecBrain(256, **kw).load(ck)
    with pytest.raises(ValueError, match="n_step"):
        VecBrain(256, n_step=2, **kw).load(ck)


def test_refusals_leave_everything_as_it_was(torch_cuda):
    """fb_replay_create_nstep with n = 0 / 17, capacity < n N or a bad kind: FB_ERR_INVALID and no handle; set_n_step on a prioritized
    memory; Memory.sample, fb_train_from_replay and fb_vec_step(train = 1) before n pushes: FB_ERR_STATE; a training call whose gamma
    is not the memory's: FB_ERR_INVALID -- and the memory, the env and the net stay as they were"""
    import ctypes as C
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd._lib import FbError
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    for cap, N, kind, n in ((100, 4, 1, 0), (100, 4, 1, 17), (11, 4, 1, 3), (11, 4, 0, 3), (100, 4, 2, 3)):
        h = C.c_void_p()
        assert L.lib().fb_replay_create_nstep(cap, N, kind, n, GAMMA, C.byref(h)) == -1 and not h.value, (cap, N, kind, n)      # FB_ERR_INVALID
    h = C.c_void_p()
    assert L.lib().fb_replay_create_nstep(12, 4, 1, 3, GAMMA, C.byref(h)) == 0 and h.value      # cap = n N exactly is fine
    L.lib().fb_replay_destroy(h)
    N, B = 256, 32
    env, rep, net, nib = _per_pipeline(N, 6 * N, "exact")
    with pytest.raises(ValueError, match="fb_replay_create_nstep"):
        rep.set_n_step(3, GAMMA)
    with pytest.raises(ValueError, match="fb_replay_create_nstep"):
        rep.set_n_step(1, GAMMA)
    assert rep.n_step == (3, GAMMA)
    good, wrong = VecStep(env, rep, net, B, "per", GAMMA), VecStep(env, rep, net, B, "per", 0.98)
    idx = torch.full((B,), 6 * N - 1, dtype=torch.int64, device="cuda")
    isw = torch.ones(B, dtype=torch.float64, device="cuda")

    def snapshot():
        return len(rep), np.asarray(rep.state_blob()).copy(), env.get_state().copy(), net.store_params().clone()

    def same(a, b):
        return a[0] == b[0] and np.array_equal(a[1], b[1]) and (a[2] == b[2]).all() and torch.equal(a[3], b[3])

    for step in range(2):                                   # pushes 0 -> 1 -> 2: the tree is still empty, then it is not
        snap = snapshot()
        with pytest.raises(FbError, match="pushes"):
            rep.sample(B)
        with pytest.raises(FbError, match="pushes"):
            train_from_replay(rep, net, "per", idx, gamma=GAMMA, isw=isw)
        with pytest.raises(FbError, match="pushes"):
            good(0.0, step=step, train=True)                # (its push would be the first / second: still no complete transition)
        assert same(snap, snapshot()), step
        good(0.0, step=step, train=False)
    snap = snapshot()
    with pytest.raises(ValueError, match="gamma"):
        wrong(0.0, step=2, train=True)
    with pytest.raises(ValueError, match="gamma"):
        wrong(0.0, step=2, train=False)
    assert same(snap, snapshot())
    good(0.0, step=2, train=True)                           # the third push completes the first transitions: trains
    assert rep.population == N and len(rep) == 3 * N
    i2, w2 = rep.sample(B)
    snap = snapshot()
    with pytest.raises(ValueError, match="gamma"):
        train_from_replay(rep, net, "per", i2, gamma=0.5, isw=w2)
    assert same(snap, snapshot())
