"""Initial priorities from acting-time TD errors (include/fbdqn.h FB_PER_INIT_TD, fb_replay_prime_priorities) on the MI355X: after
every prime and every push the tree is the NumPy restatement's (tests/primecases.py) and a twin memory's whose leaves got the same
|TD errors| through fb_replay_update_priorities, bit for bit; the fallbacks leave the leaves at max_p; fb_vec_step equals the composed
calls; the setting switched off changes nothing; the record and VecBrain checkpoints resume bit for bit; every refusal leaves the
memory, the env and the net as they were."""
import ctypes as C

import numpy as np
import pytest

from tests.primecases import PrimedMemory, priority

pytestmark = pytest.mark.gpu
GAMMA = 0.99


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def per_memory(cap, N, n, init="td", seed=9, gamma=GAMMA):
    from dqnflappybird_amd.vec import VecReplay
    rep = VecReplay(cap, N, prioritized=True, n_step=n, gamma=gamma)
    rep.set_per_mode("fast")
    if init == "td":
        rep.set_priority_init("td", gamma)
    rep.seed(seed, "numpy")
    return rep


class Tape:
    """random steps: (q f32[N, A], actions) for the prime, (frame bits, actions, rewards, terminals) for the push"""

    def __init__(self, N, A, seed, p_term=0.25):
        import torch
        self.N, self.A, self.rng, self.p_term = N, A, np.random.default_rng(seed), p_term
        self.g = torch.Generator(device="cuda").manual_seed(seed)
        self.first = self._bits()

    def _bits(self):
        import torch
        return torch.randint(-2 ** 62, 2 ** 62, (self.N, 100), device="cuda", generator=self.g, dtype=torch.int64)

    def next(self):
        N = self.N
        q = (self.rng.normal(size=(N, self.A)) * 0.7).astype(np.float32)
        a = self.rng.integers(0, self.A, N).astype(np.uint8)
        r = self.rng.choice(np.array([0.1, 1.0, -1.0], np.float32), N)
        t = (self.rng.random(N) < self.p_term).astype(np.uint8)
        return q, a, r, t, self._bits()


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def heaps(rep):
    """(tree, maxt, mint) f64[2 cap - 1] each: the last three parts of the state blob (fb_replay.hip blob_parts, 16-byte padded)"""
    blob = np.asarray(rep.state_blob())
    nb = 8 * (2 * rep.capacity - 1)
    pad = (nb + 15) & ~15
    return [blob[blob.size - k * pad:blob.size - k * pad + nb].view(np.float64).copy() for k in (3, 2, 1)]


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def assert_tree_is(rep, t, what):
    """the device's three heaps, pointer and size against the restatement's FastTree"""
    for got, want, name in zip(heaps(rep), (t.tree, t.maxt, t.mint), ("tree", "maxt", "mint")):
        assert np.array_equal(bits(got), bits(want)), (what, name, np.flatnonzero(bits(got) != bits(want))[:8])
    assert rep.per_state(want_tree=False)[1:3] == (t.pointer, t.size), what


def assert_same_memory(a, b, what):
    for x, y, name in zip(heaps(a), heaps(b), ("tree", "maxt", "mint")):
        assert np.array_equal(bits(x), bits(y)), (what, name)
    assert a.per_state(want_tree=False)[1:] == b.per_state(want_tree=False)[1:], what


CASES = [(N, cap, n, A) for (N, cap) in ((5, 40), (8, 64), (64, 1000)) for n in (1, 3) for A in (2, 3)]


@pytest.mark.parametrize("N,cap,n,A", CASES)
def test_tree_against_the_restatement_and_the_twin_memory(torch_cuda, N, cap, n, A):
    """prime -> push -> (every third step) Memory.sample + batch_update, through two wraps of the ring: after every prime and every push
    the `td` memory's heaps are (1) the restatement's bit for bit -- delta and p with the header's float and double steps, every inner
    node left + right -- and (2) those of a twin memory at `max` whose newest leaves were given the restatement's delta through
    fb_replay_update_priorities in chunks of at most 32, which pins pow to the project's own batch_update.  (40 and 1000 are no powers
    of two: leaves at two depths; 5 does not divide 40's ring evenly past the wrap; 64 into 1000 wraps inside one range.)"""
    torch = torch_cuda
    rep, twin = per_memory(cap, N, n, "td"), per_memory(cap, N, n, "max")
    mem = PrimedMemory(cap, N, n, GAMMA)
    tape = Tape(N, A, seed=17 * N + n + A)
    rep.reset(tape.first); twin.reset(tape.first)
    rng = np.random.default_rng(N + n)
    steps = 2 * ((cap + N - 1) // N) + n + 3
    primed = 0
    for S in range(steps):
        q, a, r, t, fb = tape.next()
        rep.prime(dev(q), dev(a))
        mem.prime(q, a)
        assert (mem.last_p is not None) == (S >= n)
        if mem.last_p is not None:
            primed += 1
            leaves = np.array(mem.t.last_stored(N), np.int64)
            assert np.array_equal(priority(mem.last_delta), mem.last_p)
            for lo in range(0, N, 32):
                twin.update_priorities(dev(leaves[lo:lo + 32]), abs_err=dev(mem.last_delta[lo:lo + 32].copy()))
        assert_tree_is(rep, mem.t, ("prime", S))
        assert_same_memory(rep, twin, ("prime", S))
        for m in (rep, twin):
            m.push(fb, dev(a), dev(r), dev(t))
        mem.push(r, t)
        assert_tree_is(rep, mem.t, ("push", S))
        if S >= n and S % 3 == 0:                            # (some of the newest leaves get a batch_update: the next prime overwrites them)
            B = 16
            u = dev(rng.random(B))
            (i1, w1), (i2, w2) = rep.sample(B, uniforms=u), twin.sample(B, uniforms=u)
            assert torch.equal(i1, i2) and torch.equal(w1, w2), S
            ps = (rng.random(B).astype(np.float32) * 0.9 + 0.05)
            newest = np.array(mem.t.last_stored(N), np.int64)[:B // 2]
            idx = np.concatenate([i1.cpu().numpy()[:B - newest.size], newest])
            for m in (rep, twin):
                m.update_priorities(dev(idx), priorities=dev(ps))
            mem.t.set_leaves(idx, ps)
            assert_tree_is(rep, mem.t, ("update", S))
        assert_same_memory(rep, twin, ("step", S))
    assert primed == steps - n and mem.t.size == cap and steps * N > 2 * cap
    assert len(rep) == min(steps * N, cap)                  # (fb_replay_size: no index error was raised on the way)
    rows, first, last = rep.prime_state()
    assert (first, last) == (0, steps - 1) and rows.shape == (n + 1, N)
    assert np.array_equal(rows[(steps - 1) % (n + 1)], mem.rec[steps - 1])


def test_fallbacks_leave_the_leaves_at_max_p(torch_cuda):
    """the first n primes after a reset, the n primes after a switch of the setting, after a load without the record and after a step
    without the call change no byte of the tree (the leaves keep the max_p of their store); the prime behind them does"""
    N, cap, n, A = 8, 64, 3, 2
    rep = per_memory(cap, N, n, "td")
    tape = Tape(N, A, seed=3)
    rep.reset(tape.first)
    fell_back = []

    def step(prime=True):
        q, a, r, t, fb = tape.next()
        before = heaps(rep)
        if prime:
            rep.prime(dev(q), dev(a))
            fell_back.append(all(np.array_equal(bits(x), bits(y)) for x, y in zip(before, heaps(rep))))
        rep.push(fb, dev(a), dev(r), dev(t))

    for _ in range(5):
        step()
    assert fell_back == [True] * 3 + [False] * 2
    rep.set_priority_init("max"); rep.set_priority_init("td", GAMMA)      # the switch clears the record
    assert rep.prime_state()[1:] == (-1, -1)
    del fell_back[:]
    for _ in range(5):
        step()
    assert fell_back == [True] * 3 + [False] * 2
    rep.load_state_blob(np.asarray(rep.state_blob()).copy())               # a load without fb_replay_set_prime_state
    del fell_back[:]
    for _ in range(4):
        step()
    assert fell_back == [True] * 3 + [False]
    step(prime=False)                                                      # a step without the call: the rows before it are not consecutive
    del fell_back[:]
    for _ in range(4):
        step()
    assert fell_back == [True] * 3 + [False]
    rep.reset(tape.first)                                                  # ... and the reset
    assert rep.prime_state()[1:] == (-1, -1)
    del fell_back[:]
    for _ in range(4):
        step()
    assert fell_back == [True] * 3 + [False]


@pytest.mark.parametrize("n", [1, 3])
def test_an_unprimed_td_memory_is_a_max_memory(torch_cuda, n):
    """a `td` memory on which prime was never called stores, samples (its own generator) and updates like a `max` memory"""
    torch = torch_cuda
    N, cap = 8, 100
    a, b = per_memory(cap, N, n, "td"), per_memory(cap, N, n, "max")
    tape = Tape(N, 2, seed=11)
    a.reset(tape.first); b.reset(tape.first)
    for S in range(30):
        _, act, r, t, fb = tape.next()
        for m in (a, b):
            m.push(fb, dev(act), dev(r), dev(t))
        if S >= n:
            (ia, wa), (ib, wb) = a.sample(8), b.sample(8)
            assert torch.equal(ia, ib) and torch.equal(wa, wb), S
            ae = torch.rand(8, device="cuda")
            a.update_priorities(ia.clone(), abs_err=ae.clone()); b.update_priorities(ib.clone(), abs_err=ae.clone())
        assert_same_memory(a, b, S)
    assert np.array_equal(np.asarray(a.state_blob()), np.asarray(b.state_blob()))


def pipeline(N, cap, n, arch, init, seed=5):
    from dqnflappybird_amd.vec import QNet, VecGameState
    env, rep, net = VecGameState(N, seed=seed), per_memory(cap, N, n, init), QNet(2, 512, arch, max_batch=max(N, 32))
    net.init_params(3, which=0); net.init_params(4, which=1)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("arch", ["plain", "dueling"])
@pytest.mark.parametrize("algo", ["per", "doubleper"])
@pytest.mark.parametrize("N", [8, 256])
def test_vec_step_td_equals_the_composed_calls(torch_cuda, N, algo, arch, n):
    """fb_vec_step on a `td` memory == fb_qnet_act_nib (q out) -> prime -> fb_env_step -> fb_replay_push -> fb_replay_sample ->
    fb_train_from_replay -> fb_replay_update_priorities over 12 steps that wrap the tree (8 envs: the gathered route inside the call,
    256: the ring-fed one): actions, leaf indices, weights, losses, |TD errors| step by step; parameters, env state, the memory's blob
    (ring, counters, generator, heaps) and the record at the end"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B = 8 if N == 8 else 32
    cap = 5 * N + 3
    e1, r1, n1, nib1 = pipeline(N, cap, n, arch, "td")
    e2, r2, n2, nib2 = pipeline(N, cap, n, arch, "td")
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(12):
        train = step >= max(n - 1, 1)
        a1, q1 = n1.act_nib(nib1, 0.05, seed=1, step=step, want_q=True)
        r1.prime(q1, a1)
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
        assert_same_memory(r1, r2, step)
    assert r2.population == cap                             # the tree has wrapped
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(n1.store_params(), n2.store_params())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    (ra, fa, la), (rb, fb, lb) = r1.prime_state(), r2.prime_state()
    assert (fa, la) == (fb, lb) == (0, 11) and np.array_equal(ra.view(np.uint32), rb.view(np.uint32))
    tree = r2.per_state()[0]
    leaves = tree[cap - 1:]
    assert (leaves != leaves.max()).mean() > 0.5            # most leaves hold a TD-based priority, not the max_p of their store


@pytest.mark.parametrize("mode", ["exact", "fast"])
@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("algo", ["per", "doubleper"])
def test_the_setting_switched_off_changes_nothing(torch_cuda, algo, N, mode):
    """fb_vec_step over 12 steps on a memory that was set to `td` and back to `max` (and then, mode exact, to the exact tree, which `td`
    would refuse) == on a memory that never heard of the setting: outputs, parameters and the memory's blob byte for byte, at 8 envs
    (the gathered route) and 256 (the ring-fed one)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep
    B, n = (8 if N == 8 else 32), 3
    cap = 5 * N + 3
    e1, r1, n1, _ = pipeline(N, cap, n, "plain", "max")
    e2, r2, n2, _ = pipeline(N, cap, n, "plain", "td")
    r2.set_priority_init("max")
    assert r2.priority_init == "max" and r1.priority_init == "max"
    for r in (r1, r2):
        r.set_per_mode(mode)
    s1, s2 = VecStep(e1, r1, n1, B, algo, GAMMA), VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(12):
        train = step >= n - 1
        a1, a2 = s1(0.05, seed=1, step=step, train=train), s2(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            for x, y in ((s1.idx, s2.idx), (s1.isw, s2.isw), (s1.loss, s2.loss), (s1.abs_err, s2.abs_err)):
                assert torch.equal(x, y), step
    assert torch.equal(n1.store_params(), n2.store_params())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


def test_the_record_round_trips_with_the_blob(torch_cuda):
    """state_blob + prime_state in the middle of a run, loaded into a fresh memory: both continue bit for bit, the very next prime
    included; the blob alone (no record) falls back for n primes, and the blob has the size of a `max` memory's"""
    N, cap, n, A = 8, 64, 3, 3
    a = per_memory(cap, N, n, "td")
    tape = Tape(N, A, seed=23)
    a.reset(tape.first)

    def step(ms):
        q, act, r, t, fb = tape.next()
        for m in ms:
            m.prime(dev(q), dev(act)); m.push(fb, dev(act), dev(r), dev(t))

    for _ in range(11):
        step([a])
    blob, (rows, first, last) = np.asarray(a.state_blob()).copy(), a.prime_state()
    assert (first, last) == (0, 10)
    assert blob.size == np.asarray(per_memory(cap, N, n, "max").state_blob()).size
    b, c = per_memory(cap, N, n, "td", seed=77), per_memory(cap, N, n, "td", seed=78)
    b.load_state_blob(blob); b.load_prime_state(rows, first, last)
    c.load_state_blob(blob)
    assert c.prime_state()[1:] == (-1, -1)
    got = b.prime_state()
    assert got[1:] == (0, 10) and np.array_equal(got[0].view(np.uint32), rows.view(np.uint32))
    step([a, b, c])
    assert_same_memory(a, b, "first step after the load")
    assert not np.array_equal(bits(heaps(a)[0]), bits(heaps(c)[0]))        # (c's leaves kept their max_p)
    for k in range(6):
        step([a, b])
        assert_same_memory(a, b, k)
    assert np.array_equal(np.asarray(a.state_blob()), np.asarray(b.state_blob()))
    with pytest.raises(ValueError, match="floats"):
        b.load_prime_state(rows[:2], first, last)
    with pytest.raises(ValueError, match="push counts"):
        b.load_prime_state(rows, 5, 1000)
    assert_same_memory(a, b, "after the refused loads")


def test_vecbrain_td_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo = 'per', priority_init = 'td') trains, saves, and a fresh one continues from the checkpoint bit for bit; the file
    records the setting and the record; a `max` brain refuses it by name, and a `td` brain refuses a file without the key"""
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="per", batch=32, capacity=6000, observe=2, seed=3, n_step=3)
    a = VecBrain(256, priority_init="td", **kw)
    assert a.replay.priority_init == "td"
    a.run(30, log_every=0)
    assert a.last_loss is not None and a.replay.population == 6000
    ck = str(tmp_path / "ck")
    a.save(ck)
    z = np.load(ck + ".npz")
    assert str(z["priority_init"][0]) == "td" and z["prime_rows"].shape == (4, 256) and z["prime_span"].tolist() == [0, 29]
    ta = []
    for _ in range(8):
        a.step(); ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.isw.clone(), a.one_step.loss.clone()))
    b = VecBrain(256, priority_init="td", **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(8):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.isw, b.one_step.loss)
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0))
    assert np.array_equal(np.asarray(a.replay.state_blob()), np.asarray(b.replay.state_blob()))
    m = VecBrain(256, **kw)
    with pytest.raises(ValueError, match="priority_init = 'td', this VecBrain has priority_init = 'max'"):
        m.load(ck)
    m.run(4, log_every=0)
    ck2 = str(tmp_path / "ck_max")
    m.save(ck2)
    assert "priority_init" not in np.load(ck2 + ".npz").files      # a `max` brain writes the file it wrote before the setting
    with pytest.raises(ValueError, match="priority_init = 'max', this VecBrain has priority_init = 'td'"):
        b.load(ck2)


def test_refusals_leave_everything_as_it_was(torch_cuda):
    """every refusal of the header is FB_ERR_INVALID (ValueError) and changes neither the memory (blob, record, setting, tree mode),
    the envs nor the net"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import ALGOS, IqnPerStep, QNet, SacPerStep, VecReplay, VecStep
    # the setting itself: a uniform memory, an exact tree, capacity < n_envs, a bad mode -- nothing is allocated, nothing changes
    uni = VecReplay(100, 4)
    with pytest.raises(ValueError, match="not a prioritized memory"):
        uni.set_priority_init("td")
    exact = VecReplay(100, 4, prioritized=True)
    before = np.asarray(exact.state_blob()).copy()
    with pytest.raises(ValueError, match="FB_PER_FAST"):
        exact.set_priority_init("td")
    assert L.lib().fb_replay_set_priority_init(exact.h, L.PER_INIT_TD) == -1 and L.lib().fb_replay_set_priority_init(exact.h, 2) == -1
    assert exact.priority_init == "max" and np.array_equal(np.asarray(exact.state_blob()), before)
    with pytest.raises(ValueError, match="not FB_PER_INIT_TD"):
        exact.prime(torch.zeros(4, 2, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="not FB_PER_INIT_TD"):
        exact.prime_state()
    small, mode = C.c_void_p(), C.c_int(-1)                  # (capacity < n_envs: VecReplay itself refuses to build one)
    assert L.lib().fb_replay_create(3, 4, 1, C.byref(small)) == 0 and L.lib().fb_replay_set_per_mode(small, L.PER_FAST) == 0
    assert L.lib().fb_replay_set_priority_init(small, L.PER_INIT_TD) == -1
    assert "capacity 3 >= n_envs 4" in L.lib().fb_last_error().decode()
    assert L.lib().fb_replay_get_priority_init(small, C.byref(mode)) == 0 and mode.value == L.PER_INIT_MAX
    L.lib().fb_replay_destroy(small)
    # while it is on: the exact tree, an exact blob, a gamma that is not the n-step memory's
    N, B = 256, 32
    env, rep, net, nib = pipeline(N, 6 * N, 1, "plain", "td")
    with pytest.raises(ValueError, match="FB_PER_EXACT is refused"):
        rep.set_per_mode("exact")
    big_exact = VecReplay(6 * N, N, prioritized=True)
    with pytest.raises(ValueError, match="FB_PER_EXACT"):
        rep.load_state_blob(np.asarray(big_exact.state_blob()))
    rep3 = per_memory(6 * N, N, 3, "td")
    with pytest.raises(ValueError, match="gamma"):
        rep3.set_priority_init("td", 0.5)
    with pytest.raises(ValueError, match="n_actions"):
        L.check(L.lib().fb_replay_prime_priorities(rep.h, L.ptr(torch.zeros(N, 2, device="cuda")), L.ptr(torch.zeros(N, dtype=torch.uint8, device="cuda")),
                                                   0, None), "fb_replay_prime_priorities")
    good = VecStep(env, rep, net, B, "per", GAMMA)
    for step in range(3):
        good(0.05, seed=1, step=step, train=step >= 1)

    def snapshot():
        return (len(rep), np.asarray(rep.state_blob()).copy(), rep.prime_state(), rep.priority_init, env.get_state().copy(),
                net.store_params().clone())

    def same(a, b):
        return (a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2][0].view(np.uint32), b[2][0].view(np.uint32))
                and a[2][1:] == b[2][1:] and a[3] == b[3] and (a[4] == b[4]).all() and torch.equal(a[5], b[5]))

    snap = snapshot()
    # fb_vec_step on the `td` memory: FB_ALGO_MDQN_PER; a gamma that is not the memory's; C51 / QR / noisy / AC / SAC nets
    with pytest.raises(ValueError, match="FB_ALGO_MDQN_PER does not take a FB_PER_INIT_TD memory"):
        VecStep(env, rep, net, B, "mdqnper", GAMMA)(0.05, seed=1, step=3)
    for train in (True, False):
        with pytest.raises(ValueError, match="fb_replay_set_prime_gamma"):
            VecStep(env, rep, net, B, "per", 0.98)(0.05, seed=1, step=3, train=train)
    for kw, algo in ((dict(arch="c51"), "c51per"), (dict(arch="c51dueling"), "c51doubleper"), (dict(arch="c51", noisy=True), "c51per"),
                     (dict(arch="qr"), "qrper"), (dict(arch="qrdueling"), "qrdoubleper")):
        other = QNet(2, 512, max_batch=N, **kw)
        other.init_params(3, which=0); other.init_params(4, which=1)
        with pytest.raises(ValueError, match="FB_PER_INIT_TD memory takes FB_ALGO_PER / FB_ALGO_DOUBLE_PER on a scalar net only"):
            VecStep(env, rep, other, B, algo, GAMMA)(0.05, seed=1, step=3)
    for arch, word in (("ac", "actor-critic"), ("sac", "SAC")):
        other = QNet(2, 512, arch, max_batch=N)
        with pytest.raises(ValueError, match=word):
            VecStep(env, rep, other, B, "per", GAMMA)(0.05, seed=1, step=3)
    # fb_vec_step_dp (refused before it looks at its communicator)
    rc = L.lib().fb_vec_step_dp(None, env.h, rep.h, net.h, C.byref(good.buf), N, ALGOS["per"], B, 0.05, 1, 3, 1, GAMMA, 0, L.current_stream())
    assert rc == -1 and "fb_vec_step_dp: data parallel does not take a FB_PER_INIT_TD memory" in L.lib().fb_last_error().decode()
    # ... and the prioritized SAC and IQN steps, store-only or training
    sac, iqn = QNet(2, 512, "sac", max_batch=N), QNet(2, 512, "iqn", max_batch=N)
    for one in (SacPerStep(env, rep, sac, B, GAMMA), IqnPerStep(env, rep, iqn, B, GAMMA)):
        for train in (True, False):
            with pytest.raises(ValueError, match=f"{one.entry}: does not take a FB_PER_INIT_TD memory"):
                one(seed=1, step=3, train=train)
    assert same(snap, snapshot())
    good(0.05, seed=1, step=3)                               # ... and the step goes on
    assert len(rep) == 4 * N and rep.prime_state()[1:] == (0, 3)
