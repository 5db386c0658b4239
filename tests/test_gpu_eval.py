"""On-device evaluation (fb_eval_run, dqnflappybird_amd/evaluate.py) against the composition of existing calls, the oracle, and the
training loop it must leave alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_net(oracle, arch, dtype, max_batch, scale, seed=5):
    from dqnflappybird_amd.vec import QNet
    cfg = oracle.qcfg(512, 2, arch == "dueling")
    p = oracle.init_params(cfg, seed=seed) * np.float32(scale)
    net = QNet(2, 512, arch, max_batch=max_batch)
    net.load_params(p)
    net.set_inference_dtype(dtype)
    return net, p, cfg


def composed(net, M, n, episodes, env_seed, max_steps=10 ** 9):
    """VecGameState(M) + act_nib(epsilon = 0) -> frame_step on all M rows; records of envs 0..n-1 kept on the host."""
    import torch
    from dqnflappybird_amd.vec import VecGameState
    env = VecGameState(M, seed=env_seed)
    nib = env.track_state()
    env.observe()
    score = np.zeros((n, episodes), np.int32)
    length = np.zeros((n, episodes), np.int32)
    trunc = np.zeros((n, episodes), np.uint8)
    k = np.zeros(n, np.int64)
    cur = np.zeros(n, np.int64)
    steps = 0
    while steps < max_steps and (k < episodes).any():
        act = net.act_nib(nib, 0.0)
        _, _, term, sc = env.frame_step(act, want_u8=False)
        steps += 1
        term = term.cpu().numpy()[:n].astype(bool)
        sc = sc.cpu().numpy()[:n]
        live = k < episodes
        cur[live] += 1
        end = live & term
        for e in np.nonzero(end)[0]:
            score[e, k[e]], length[e, k[e]] = sc[e], cur[e]
            k[e] += 1
            cur[e] = 0
    if steps == max_steps:
        st = env.get_state()[:n]
        for e in np.nonzero((k < episodes) & (cur > 0))[0]:
            score[e, k[e]], length[e, k[e]], trunc[e, k[e]] = st[e, 5], cur[e], 1
    torch.cuda.synchronize()
    return score, length, trunc, steps


# (n, M, arch, dtype, episodes, scale): M >= 256 keeps the composed path on the fused kernels; n < 256 shows that compaction below
# 256 live rows changes nothing.  The plain net at scale 3 plays episodes of different lengths (19 to 60-odd frames, three episodes
# per env: compactions at several chunk boundaries); the init scale, and the dueling nets of these seeds, mostly play one action
CASES = [
    (1027, 1027, "plain", "f32", 3, 3.0),
    (4096, 4096, "plain", "f32", 3, 3.0),
    (16, 256, "plain", "bf16", 3, 3.0),
    (200, 256, "dueling", "f32", 3, 3.0),
    (1027, 1027, "dueling", "f32", 1, 3.0),
    (256, 256, "plain", "f32", 1, 1.0),
    (300, 300, "plain", "bf16", 1, 3.0),
]


@pytest.mark.parametrize("n,M,arch,dtype,episodes,scale", CASES)
def test_equals_composed_calls(torch_cuda, oracle, n, M, arch, dtype, episodes, scale):
    from dqnflappybird_amd.evaluate import Evaluator
    net, p, _ = make_net(oracle, arch, dtype, max_batch=(M + 2) // 3, scale=scale)
    s0, l0, t0, _ = composed(net, M, n, episodes, env_seed=11)
    res = Evaluator(n).run(net, n, episodes, max_steps=100_000, env_seed=11)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all() and not res.truncated.any()
    assert res.steps == int(l0.sum(1).max())
    if arch == "plain" and scale > 1.0 and n >= 1000:
        assert len(np.unique(l0.sum(1))) >= 8            # envs die at different steps ...
        assert res.compactions >= 3                      # ... and the rows were compacted several times
    # the same records when the acting forward runs in passes of fewer rows than there are envs
    if n > 1000:
        small, _, _ = make_net(oracle, arch, dtype, max_batch=171, scale=scale)      # passes of 513 rows
        r2 = Evaluator(n).run(small, n, episodes, max_steps=100_000, env_seed=11)
        assert np.array_equal(r2.length, l0) and np.array_equal(r2.score, s0)


def test_acting_forward_is_row_independent(torch_cuda, oracle):
    """Q of a state through the evaluation's forward entry does not depend on its row, its slot in a five-state workgroup or the row
    count -- what compaction rests on -- and equals fb_qnet_act_nib's at >= 256 states."""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import VecGameState
    net, _, _ = make_net(oracle, "plain", "f32", max_batch=400, scale=3.0)
    N = 1027
    env = VecGameState(N, seed=3)
    nib = env.track_state()
    env.observe()
    g = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(40):                                  # varied stacks: random flaps, deaths and resets
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
    assert np.array_equal(q_of(states[:256].contiguous()), q0[:256])
    for rows in (1, 7, 255):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            assert np.array_equal(q_of(states[r0:r1].contiguous()), q0[r0:r1]), (rows, r0)
            if rows == 1 and r0 >= 64:
                break                                   # (one state per launch: the first 64 rows are enough)


def test_epsilon_draw_follows_the_env(torch_cuda, oracle):
    from dqnflappybird_amd.evaluate import evaluate
    net, _, _ = make_net(oracle, "plain", "f32", max_batch=64, scale=3.0)
    a = evaluate(net, 300, episodes=2, epsilon=0.05, env_seed=4, act_seed=9)
    b = evaluate(net, 4096, episodes=2, epsilon=0.05, env_seed=4, act_seed=9)
    c = evaluate(net, 300, episodes=2, epsilon=0.05, env_seed=4, act_seed=9)
    g = evaluate(net, 300, episodes=2, epsilon=0.0, env_seed=4, act_seed=9)
    for name in ("score", "length", "truncated"):
        assert np.array_equal(getattr(a, name), getattr(b, name)[:300]), name
        assert np.array_equal(getattr(a, name), getattr(c, name)), name
    assert not np.array_equal(a.length, g.length)            # the draw is live
    assert b.compactions >= 2 and a.compactions >= 2


def test_truncation(torch_cuda, oracle):
    from dqnflappybird_amd.evaluate import Evaluator
    net, _, _ = make_net(oracle, "plain", "f32", max_batch=86, scale=3.0)
    n, E, cap = 256, 3, 70
    s0, l0, t0, steps0 = composed(net, n, n, E, env_seed=2, max_steps=cap)
    res = Evaluator(n).run(net, n, E, max_steps=cap, env_seed=2)
    assert res.steps == cap == steps0
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    tr = res.truncated.astype(bool)
    assert tr.sum() > 0 and (res.length[tr] > 0).all() and (res.length[tr] <= cap).all()
    assert (res.length == 0).any()                            # absent entries are marked
    assert ((res.length == 0) <= (res.score == 0)).all()
    # every env has at most one truncated entry, after its completed ones
    for e in range(n):
        k = int((res.length[e] > 0).sum())
        assert not res.truncated[e, :max(k - 1, 0)].any()
    short = Evaluator(n).run(net, n, 2, max_steps=10, env_seed=2)      # nothing can end in 10 frames: every env truncated at 10
    assert short.steps == 10 and (short.length[:, 0] == 10).all() and short.truncated[:, 0].all() and (short.length[:, 1] == 0).all()


def _brain_state(b):
    m, v, pows = b.net.adam_state()
    return dict(online=b.net.store_params(0).cpu().numpy(), target=b.net.store_params(1).cpu().numpy(), m=m.cpu().numpy(),
                v=v.cpu().numpy(), pows=np.asarray(pows), env=b.env.get_state(), nib=b.nib.cpu().numpy(), stats=b.stats.cpu().numpy(),
                replay=np.frombuffer(bytes(b.replay.state_blob()), np.uint8), t=(b.timeStep, b.onlineTimeStep, b.epsilon))


@pytest.mark.parametrize("split", [1, 0])
def test_no_interference_with_training(torch_cuda, split):
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vecbrain import VecBrain
    L.lib().fb_vec_step_set_schedule(split)
    try:
        ref = VecBrain(1024, algo="nature", observe=100, capacity=50_000)
        ref.run(600, log_every=0)
        b = VecBrain(1024, algo="nature", observe=100, capacity=50_000)
        b.run(300, log_every=0)
        res = b.evaluate(n_envs=512, episodes=2, max_steps=5000)
        assert res.episodes > 0
        b.run(300, log_every=0)
        want, got = _brain_state(ref), _brain_state(b)
        for k in want:
            if k == "t":
                assert want[k] == got[k]
            else:
                assert np.array_equal(want[k], got[k]), k
        steps, _ = b.net.split_stats()                   # (raises if a wait between the two streams gave up)
        assert (steps > 0) == bool(split)
    finally:
        L.lib().fb_vec_step_set_schedule(1)


def test_validation(torch_cuda, oracle):
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.evaluate import Evaluator
    from dqnflappybird_amd.vec import QNet
    torch = torch_cuda
    lib = L.lib()
    net, _, _ = make_net(oracle, "plain", "f32", max_batch=16, scale=1.0)
    net3 = QNet(3, 512, "plain", max_batch=16)
    ev = Evaluator(64)
    out = [torch.full((64 * 64,), 7, dtype=torch.int32, device="cuda"), torch.full((64 * 64,), 7, dtype=torch.int32, device="cuda"),
           torch.full((64 * 64,), 7, dtype=torch.uint8, device="cuda")]
    steps = C.c_int64(-5)

    def run(h=None, n=8, e=1, ms=10, eps=0.0):
        return lib.fb_eval_run(ev.h, h if h is not None else net.h, n, e, ms, eps, 0, 0, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]),
                               C.byref(steps), L.current_stream())

    bad = [dict(h=net3.h), dict(e=0), dict(e=65), dict(n=0), dict(n=65537), dict(n=65), dict(ms=0), dict(eps=-0.1), dict(eps=1.5),
           dict(eps=float("nan"))]
    for kw in bad:
        assert run(**kw) == -1, kw
        assert lib.fb_last_error().decode().startswith("fb_eval_run"), kw
    assert lib.fb_eval_run(ev.h, None, 8, 1, 10, 0.0, 0, 0, L.ptr(out[0]), L.ptr(out[1]), L.ptr(out[2]), C.byref(steps),
                           L.current_stream()) == -1
    torch.cuda.synchronize()
    assert (out[0] == 7).all() and (out[1] == 7).all() and (out[2] == 7).all() and steps.value == -5      # nothing was launched
    h = C.c_void_p()
    assert lib.fb_eval_create(16, None, 0, C.byref(h)) == -1 and not h.value
    blob = L.sprite_blob()
    assert lib.fb_eval_create(0, blob, len(blob), C.byref(h)) == -1
    assert run() == 0 and steps.value == 10                  # a valid call still succeeds


def test_matches_the_oracle(torch_cuda, oracle):
    """16 envs, epsilon 0, two episodes: the oracle's Philox env and Q forward replay the same games on the CPU.  Records must agree in
    every env whose greedy decisions all had an oracle Q margin > 1e-3 (at least half of them)."""
    from dqnflappybird_amd.evaluate import evaluate
    n, E, seed = 16, 2, 21
    net, p, cfg = make_net(oracle, "plain", "f32", max_batch=16, scale=3.0, seed=13)
    res = evaluate(net, n, E, env_seed=seed)
    envs = [oracle.GameState(seed=seed, env_id=e) for e in range(n)]
    stack = np.stack([np.repeat(g.frame80()[:, :, None], 4, axis=2) for g in envs])
    score = np.zeros((n, E), np.int32)
    length = np.zeros((n, E), np.int32)
    k = np.zeros(n, int)
    cur = np.zeros(n, int)
    clean = np.ones(n, bool)
    while (k < E).any():
        live = np.nonzero(k < E)[0]
        q = oracle.forward(p, cfg, stack[live])
        for j, e in enumerate(live):
            clean[e] &= abs(float(q[j, 0]) - float(q[j, 1])) > 1e-3
            a = int(np.argmax(q[j]))
            _, term, sc = envs[e].step(a)
            cur[e] += 1
            stack[e] = np.concatenate([stack[e][:, :, 1:], envs[e].frame80()[:, :, None]], axis=2)
            if term:
                score[e, k[e]], length[e, k[e]] = sc, cur[e]
                k[e] += 1
                cur[e] = 0
    assert clean.sum() >= n // 2, clean
    assert np.array_equal(res.score[clean], score[clean]) and np.array_equal(res.length[clean], length[clean])
    assert not res.truncated.any()
