"""The replay samplers against CPython, Philox and the reference's Memory themselves, at every batch size where they branch.

(a) the stand-alone sampler over the whole case list of tests/samplecases.py: 150 (n, k) x 40 consecutive draws (6000) with seed 7,
    30 (n, k) x 40 (1200) with the two-word seed 2**40 + 7 -- tests/test_sampler_cases_host.py shows, from CPython alone, how often
    those draws sit on a block edge, in a block's last 63 words, on repeated candidates and on either side of setsize;
(b) push_sample while the population walks 64 .. 1100 through the pool path, over setsize and onto the capacity, B = 64, 65, 256;
(c) the env-launch rider, the gated draw of the split schedule and the conv3-backward rider (fb_train_steps) against
    random.sample itself, not against another launch of the same device code, also at B = 256 where pool and table sit in LDS
    the carrying kernel laid out;
(d) sample_philox_kernel element by element against the oracle's Philox4x32-10, with the call counter as the code keeps it;
(e) the Philox branch of Memory.sample (per_sample_kernel) against SumTree.get_leaf walked on the host;
(f) per_sample_kernel on NumPy's generator at n = 1, 33, 255, 256 against the reference's Memory, 512 words per round at n = 256.
Every comparison is exact, but for the importance weights (a pow: rtol 1e-13, as everywhere in the suite)."""
import random

import numpy as np
import pytest

from tests import samplecases as S

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
CAP = 1100                                # (b), (c): a capacity above setsize(256) = 1045, so that B = 256 ends on the set path
WIDE_KS = (64, 65, 256)                   # the k drawn with the two-word seed as well


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def zero_transition(torch, N):
    return (torch.zeros((N, 100), dtype=torch.int64, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"),
            torch.zeros(N, dtype=torch.float32, device="cuda"))


def filled_memory(torch, n, N, **kw):
    """a VecReplay of capacity n holding exactly n transitions (zero frames, N envs per push)"""
    from dqnflappybird_amd.vec import VecReplay
    rep = VecReplay(n, N, **kw)
    z8, za, zr = zero_transition(torch, N)
    rep.reset(z8)
    for _ in range(-(-n // N)):
        rep.push(z8, za, zr, za)
    assert len(rep) == n
    return rep


def assert_draws_equal(got, want, what):
    """got: [draws][k] from the device, want: the same from random.sample; the first draw that differs is reported"""
    for d, (g, w) in enumerate(zip(got, want)):
        if list(g) != list(w):
            at = next(i for i, (x, y) in enumerate(zip(g, w)) if x != y)
            pytest.fail(f"{what}: draw {d} differs from random.sample at element {at}: kernel {list(g)[at:at + 6]} ..., "
                        f"CPython {list(w)[at:at + 6]} ...")
    assert len(got) == len(want)


# ----------------------------------------------------------------------------- (a) the stand-alone sampler
@pytest.mark.parametrize("n", sorted(S.by_n()))
def test_sample_equals_cpython_over_the_case_list(torch_cuda, n):
    """every k of the list drawn from a memory of exactly n transitions: 40 consecutive sample(k) after seed() equal 40 consecutive
    random.sample(range(n), k) after random.seed(); k = 64, 65, 256 also with a seed of two key words"""
    torch = torch_cuda
    rep = filled_memory(torch, n, n if n <= 4099 else 4096)
    compared = 0
    for k in S.by_n()[n]:
        for seed in (S.SEED, S.SEED_WIDE) if k in WIDE_KS else (S.SEED,):
            out = torch.full((S.DRAWS, k), -7, dtype=torch.int64, device="cuda")
            rep.seed(seed, "cpython")
            for d in range(S.DRAWS):
                rep.sample(k, out=out[d])
            assert_draws_equal(out.cpu().tolist(), S.expected(seed, n, k), f"seed {seed}, n {n}, k {k}")
            compared += S.DRAWS
    assert len(rep) == n                           # (raises if the sticky error word is set)
    print(f"n = {n}: {compared} draws compared")


# ----------------------------------------------------------------------------- (b) push_sample
@pytest.mark.parametrize("B", [64, 65, 256])
def test_push_sample_equals_cpython_while_the_memory_fills(torch_cuda, B):
    """40 steps of 64 envs into 1100 slots: the population goes 64, 128, ... 1088, 1100, 1100 ...; B = 64 starts on n = k, B = 256
    on n = k = 256 (pool path), crosses setsize and stays at 1100, where every B = 256 draw meets repeated candidates"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecReplay
    N, steps = 64, 40
    rep = VecReplay(CAP, N)
    z8, za, zr = zero_transition(torch, N)
    rep.reset(z8)
    rep.seed(S.SEED, "cpython")
    r = random.Random(S.SEED)
    got, want, sizes = [], [], []
    for step in range(steps):
        pop = min((step + 1) * N, CAP)
        if pop < B:
            rep.push(z8, za, zr, za)
            continue
        got.append(rep.push_sample(z8, za, zr, za, B).clone())
        want.append(r.sample(range(pop), B))
        sizes.append(pop)
    assert sizes[0] == -(-B // N) * N and sizes[-1] == CAP and any(p <= S.setsize(B) for p in sizes) and any(p > S.setsize(B) for p in sizes)
    assert_draws_equal(torch.stack(got).cpu().tolist(), want, f"push_sample, B {B}")
    assert len(rep) == CAP
    print(f"B = {B}: {len(want)} draws compared")


# ----------------------------------------------------------------------------- (c) riders and the gated draw
@pytest.mark.parametrize("N,B,schedule", [(64, 32, 0), (64, 32, 1), (64, 256, 0), (64, 256, 1), (256, 32, 0), (256, 32, 1), (256, 255, 1)])
def test_vec_step_draws_equal_cpython(torch_cuda, N, B, schedule):
    """fb_vec_step's minibatch indices on every training step == random.sample(range(len(memory)), B).  64 envs: the draw rides in the
    env launch under either schedule setting; 256 envs (the fewest the split schedule takes, B < 256): schedule 1 draws in
    sample_gated_kernel, schedule 0 in the env launch"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
    steps = 40
    env, rep, net = VecGameState(N, seed=5), VecReplay(CAP, N), QNet(max_batch=max(N, B))
    rep.seed(S.SEED, "cpython"); net.init_params(3)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    one = VecStep(env, rep, net, B, "dqn")
    r = random.Random(S.SEED)
    got, want = [], []
    try:
        L.check(L.lib().fb_vec_step_set_schedule(schedule), "schedule")
        for step in range(steps):
            pop = min((step + 1) * N, CAP)
            one(0.05, seed=1, step=step, train=pop >= B)
            if pop >= B:
                got.append(one.idx.clone())
                want.append(r.sample(range(pop), B))
    finally:
        L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
    assert_draws_equal(torch.stack(got).cpu().tolist(), want, f"fb_vec_step, {N} envs, B {B}, schedule {schedule}")
    assert len(rep) == CAP
    issued, _ = net.split_stats()                  # (raises if a wait between the two streams gave up)
    assert issued == (len(want) if schedule == 1 and N >= 256 else 0)
    print(f"{N} envs, B = {B}, schedule {schedule}: {len(want)} draws compared, {issued} of them gated")


@pytest.mark.parametrize("B", [32, 256])
def test_train_steps_draws_equal_cpython(torch_cuda, B):
    """fb_train_steps on a full 1100-slot memory, a call of 2 steps and one of 3: step i's indices are in half i & 1 of the index
    buffer, the draws of steps 1 .. n - 1 rode in the step before's conv3 backward; then a stand-alone draw goes on in the stream"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, TrainSteps
    rep = filled_memory(torch, CAP, 100)
    net = QNet(max_batch=B)
    net.init_params(3)
    rep.seed(S.SEED, "cpython")
    want = S.expected(S.SEED, CAP, B, 6)
    ts = TrainSteps(rep, net, B, "dqn")
    ts(2)
    halves = ts.idx.view(2, B).cpu().tolist()
    assert_draws_equal([halves[1], halves[0]], [want[1], want[0]], f"fb_train_steps(2), B {B}")
    ts(3)
    halves = ts.idx.view(2, B).cpu().tolist()
    assert_draws_equal([halves[0], halves[1]], [want[4], want[3]], f"fb_train_steps(3), B {B}")
    assert_draws_equal([rep.sample(B)[0].cpu().tolist()], [want[5]], f"sample after fb_train_steps, B {B}")
    assert len(rep) == CAP
    print(f"B = {B}: 5 draws compared")


# ----------------------------------------------------------------------------- (d) Philox, uniform
def philox_indices(oracle, seed, n, k, call):
    return [(int(oracle.philox(seed & M32, seed >> 32, i, call, 2, 0)[0]) * n) >> 32 for i in range(k)]


@pytest.mark.parametrize("n", [300, 65537, 1_000_000])
def test_philox_sampler_equals_the_oracles_philox(torch_cuda, oracle, n):
    """element i of Philox sample call c on a handle == (philox(key = seed, counter = (i, c, FB_STREAM_SAMPLE = 2, 0)).x * n) >> 32,
    c counting that handle's Philox sample calls since its creation: neither seed() nor reset() rewinds it"""
    torch = torch_cuda
    N = 100 if n == 300 else 4096
    rep = filled_memory(torch, n, N)
    call = compared = 0
    for seed in (7, 2 ** 40 + 7):
        rep.seed(seed, "philox")                   # (the second seed: the counter goes on from 20)
        for k in (1, 32, 255, 256):
            for _ in range(5):
                got = rep.sample(k)[0].cpu().tolist()
                assert got == philox_indices(oracle, seed, n, k, call), (seed, n, k, call)
                call += 1
                compared += 1
    z8, za, zr = zero_transition(torch, N)
    rep.reset(z8)                                  # an emptied memory, one push: the population changes, the counter goes on
    rep.push(z8, za, zr, za)
    assert rep.sample(32)[0].cpu().tolist() == philox_indices(oracle, 2 ** 40 + 7, min(N, n), 32, call)
    assert call == 40 and len(rep) == min(N, n)
    print(f"n = {n}: {compared + 1} draws compared")


def test_philox_sampler_on_an_n_step_view(torch_cuda, oracle):
    """the same on set_n_step(3, 0.99): n is the view's population, len(memory) less the 2 N newest positions"""
    torch = torch_cuda
    N = 100
    rep = filled_memory(torch, 5000, N)
    rep.set_n_step(3, 0.99)
    n = rep.population
    assert n == 5000 - 2 * N
    call = 0
    for seed in (7, 2 ** 40 + 7):
        rep.seed(seed, "philox")
        for k in (1, 32, 255, 256):
            for _ in range(5):
                got = rep.sample(k)[0].cpu().tolist()
                assert got == philox_indices(oracle, seed, n, k, call), (seed, k, call)
                call += 1
    assert len(rep) == 5000
    print(f"{call} draws compared")


# ----------------------------------------------------------------------------- (e) Philox, prioritized
@pytest.mark.parametrize("cap,N,pushes", [(50, 5, 7), (5000, 100, 60)])
def test_per_philox_branch_equals_get_leaf_on_the_host(torch_cuda, oracle, cap, N, pushes):
    """Memory.sample with the segment uniforms from Philox: u_i from words x, y of philox(key = seed, counter = (i, call,
    FB_STREAM_PER = 3, 0)) the way NumPy forms a double, v_i = uniform(seg i, seg (i + 1)), the leaf by get_leaf on the device's own
    tree; weights (p / total / min_prob) ** -beta.  35 of 50 leaves filled, and 5000 leaves filled past the ring's wrap.  The call
    counter is the handle's: one per sample call (also one whose uniforms were injected), rewound by neither seed() nor reset()"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecReplay
    seed = 2 ** 40 + 7
    rep = VecReplay(cap, N, prioritized=True)
    z8, za, zr = zero_transition(torch, N)
    rng = np.random.default_rng(cap)

    def fill():
        rep.reset(z8)
        for _ in range(pushes):
            rep.push(z8, za, zr, za)
        size = min(pushes * N, cap)
        leaves = rng.choice(size, size=min(size, 200), replace=False).astype(np.int64) + cap - 1
        ps = (rng.random(len(leaves)).astype(np.float32) * 1.2 + 0.01).clip(max=1.0) ** np.float32(0.6)
        rep.update_priorities(torch.from_numpy(leaves).cuda(), priorities=torch.from_numpy(ps).cuda())
        return size

    def check(n, call):
        tree, _, filled, _ = rep.per_state()
        assert filled == size and len(np.unique(tree[cap - 1:cap - 1 + size])) > 10
        idx, isw = rep.sample(n)
        idx, isw = idx.cpu().numpy(), isw.cpu().numpy()
        beta = rep.per_state(want_tree=False)[3]
        total, seg = tree[0], tree[0] / n
        want = []
        for i in range(n):
            x, y = (int(w) for w in oracle.philox(seed & M32, seed >> 32, i, call, 3, 0)[:2])
            u = ((x >> 5) * 67108864.0 + (y >> 6)) / 9007199254740992.0
            want.append(S.get_leaf(tree, seg * i + (seg * (i + 1) - seg * i) * u))
        assert idx.tolist() == want, (n, call)
        min_prob = tree[cap - 1:cap - 1 + size].min() / total
        np.testing.assert_allclose(isw, (tree[idx] / total / min_prob) ** -beta, rtol=1e-13)
        return beta

    size = fill()
    rep.seed(seed, "philox")
    call, beta = 0, 0.4
    for n in (1, 32, 256):
        for _ in range(2):
            new = check(n, call)
            assert new == min(1.0, beta + 0.001)
            beta, call = new, call + 1
    rep.sample(32, uniforms=torch.from_numpy(rng.random(32)).cuda())      # injected uniforms: no Philox word is used, the counter advances
    call += 1
    rep.seed(seed, "philox")
    size = fill()                                  # reset(): beta is 0.4 again, the counter is not 0 again
    assert check(32, call) == 0.4 + 0.001
    assert call == 7
    print(f"cap = {cap}: 7 draws compared")


# ----------------------------------------------------------------------------- (f) NumPy generator, other batch sizes
@pytest.mark.parametrize("n", [1, 33, 255, 256])
def test_per_numpy_sampler_equals_the_reference_memory(torch_cuda, oracle, n):
    """Memory.sample(n) / batch_update rounds beside oracle.Memory on NumPy's own stream: 2 n words per round (n = 256: 512 of a
    624-word block, so the word fetch crosses the block edge in most rounds); indices equal, weights to 1e-13, tree bytes equal"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecReplay
    cap, N, seed, rounds = 5000, 50, 7, 10
    rep = VecReplay(cap, N, prioritized=True)
    z8, za, zr = zero_transition(torch, N)
    rep.reset(z8)
    rep.seed(seed, "numpy")
    mem, np_rng = oracle.Memory(cap), oracle.NpRandom(seed)
    rng = np.random.default_rng(n)
    for _ in range(97):                            # 4850 of 5000 leaves: the fourth round's store wraps the ring
        rep.push(z8, za, zr, za)
    mem.store(97 * N)
    crossed = 0
    for rnd in range(rounds):
        start = (2 * n * rnd) % S.BLOCK
        crossed += start + 2 * n > S.BLOCK
        idx, isw = rep.sample(n)
        oi, ow = mem.sample(n, np_rng=np_rng)
        assert idx.cpu().tolist() == list(oi), (n, rnd)
        np.testing.assert_allclose(isw.cpu().numpy(), ow, rtol=1e-13)
        ps = (rng.random(n).astype(np.float32) * 1.2 + 0.01).clip(max=1.0) ** np.float32(0.6)
        rep.update_priorities(idx, priorities=torch.from_numpy(ps).cuda())
        mem.batch_update_p(oi, ps)
        tree, ptr, size, beta = rep.per_state()
        assert (ptr, size, beta) == (mem.data_pointer, mem.size, mem.beta)
        assert np.array_equal(tree.view(np.uint64), mem.tree.view(np.uint64)), (n, rnd)
        rep.push(z8, za, zr, za)                   # the ring and the tree's pointer move on between the rounds
        mem.store(N)
    assert crossed >= (6 if n >= 255 else 0)
    print(f"n = {n}: {rounds} rounds compared, {crossed} of them fetch words on both sides of a block edge")
