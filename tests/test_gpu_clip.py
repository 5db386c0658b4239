"""Global-norm gradient clipping on the device (include/fbdqn.h: fb_qnet_set_max_grad_norm, fb_qnet_clip_grad, fb_qnet_grad_norm).
References: numpy's float64 norm of the very gradient the kernels read; fp32 arithmetic on the device's own norm for the scale (exact);
the three public calls composed by hand for every train entry point (bit for bit).

Bounds.  The norm: squares and sums are float64 on the device, so what separates it from numpy's float64 norm is the summation order
(~1e-16 relative per add, far below) and ONE rounding to fp32, 2^-24 = 6e-8 relative: 1e-6 relative.  The clipped gradient's norm: every
element is g * c rounded to fp32 (<= 2^-24 relative each) and c itself is the rounded G / norm (2^-24) of a rounded norm (2^-24), so the new
norm is G to 3 * 2^-24 < 1e-6 relative.

Three nets: plain A = 2 FC = 512 (n % 4 == 2: the ragged tail), dueling A = 3 FC = 128 (n % 4 == 0), noisy dueling C51 at its defaults."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 0.99
NETS = ("plain", "dueling3", "noisy")
N_PARAMS = {"plain": 898_722, "dueling3": 283_428, "noisy": 976_185 + 898_201}
N_PARAMS_DUELING2 = 899_235                                  # dueling, A = 2, FC = 512 (the vector-step cases)
ALGO_OF = {"plain": "double", "dueling3": "double", "noisy": "c51doubleper", "qr": "qrdouble"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_net(kind, seed=3, max_batch=32):
    """the library's own initialisation x 3 (a trunk whose ReLUs switch, Q of O(1)); the noisy net with a drawn sample in both nets"""
    from dqnflappybird_amd.vec import QNet
    if kind == "plain":
        net = QNet(2, 512, "plain", max_batch=max_batch)
    elif kind == "dueling3":
        net = QNet(3, 128, "dueling", max_batch=max_batch)
    elif kind == "qr":
        net = QNet(2, 512, "qr", max_batch=max_batch)
    else:
        net = QNet(2, 512, "c51dueling", max_batch=max_batch, noisy=True)
    net.init_params(seed, which=0); net.init_params(seed + 1, which=1)
    for which in (0, 1):
        net.load_params(net.store_params(which) * 3.0, which)
    if kind == "noisy":
        net.reset_noise(0, 7, 1); net.reset_noise(1, 7, 1)
    net.set_hparams(lr=1e-4)
    return net


def batch(torch, rng, B, A):
    s = (rng.random((B, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    s2 = (rng.random((B, 80, 80, 4)) < 0.37).astype(np.uint8) * 255
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    t = (r == -3).astype(np.uint8)
    isw = rng.uniform(0.5, 1.0, B).astype(np.float32)
    return tuple(torch.from_numpy(x).cuda() for x in (s, a, r, s2, t, isw))


def step(net, algo, bt, flat_grad=None):
    s, a, r, s2, t, isw = bt
    weighted = algo.endswith("per")
    return net.train_step(algo, s, a, r, s2, t, isw=isw if weighted else None, gamma=GAMMA, flat_grad=flat_grad, want_aux=not algo.startswith(("c51", "qr")))


def f64_norm(g):
    return float(np.linalg.norm(g.cpu().numpy().astype(np.float64)))


def state(net):
    m, v, pows = net.adam_state()
    return net.store_params().clone(), m, v, np.array(pows)


def same_state(torch, x, y):
    return torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2]) and np.array_equal(x[3], y[3])


# ---------------------------------------------------------------------------------------------------------------- 1. the norm
@pytest.mark.parametrize("kind", NETS)
def test_norm_of_exported_and_synthetic_gradients(torch_cuda, kind):
    torch = torch_cuda
    net = make_net(kind)
    n = net.n_params
    assert n == N_PARAMS[kind] and n % 4 == {"plain": 2, "dueling3": 0, "noisy": 2}[kind]
    assert net.grad_norm() == (0.0, 1.0) and net.max_grad_norm == 0.0
    rng = np.random.default_rng(n)
    g = torch.zeros(n, dtype=torch.float32, device="cuda")
    for B in (4, 32):
        step(net, ALGO_OF[kind], batch(torch, rng, B, net.A), flat_grad=g)
        keep = g.clone()
        net.clip_grad(g)                                         # (G = 0: the diagnostic use)
        norm, scale = net.grad_norm()
        ref = f64_norm(keep)
        print(f"{kind} B={B}: device norm {norm!r}, float64 norm {ref!r}, rel {abs(norm - ref) / ref:.3g}")
        assert ref > 0 and abs(norm - ref) <= 1e-6 * ref and scale == 1.0
        assert torch.equal(g, keep)
        if kind == "noisy":                                      # sigma's part is in the norm (noisy_sgrad_kernel has written it by then)
            n_mu = 976_185
            assert f64_norm(keep[n_mu:]) > 0 and abs(norm - f64_norm(keep[:n_mu])) > 1e-6 * ref
    # the reference's regime (1e-9 .. 1e-6): nothing underflows to 0; and one large entry among them
    mag = np.exp(rng.uniform(np.log(1e-9), np.log(1e-6), n)) * rng.choice([-1.0, 1.0], n)
    for name, arr in (("tiny", mag), ("one 1e3", np.where(np.arange(n) == n - 1, 1e3, mag))):      # (the large one in the ragged tail where there is one)
        g.copy_(torch.from_numpy(arr.astype(np.float32)))
        ref = f64_norm(g)
        net.clip_grad(g)
        norm, scale = net.grad_norm()
        print(f"{kind} {name}: device norm {norm!r}, float64 norm {ref!r}")
        assert norm > 0 and abs(norm - ref) <= 1e-6 * ref and scale == 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. the scale
@pytest.mark.parametrize("kind", NETS)
def test_scale_is_exact_off_is_bit_identical_and_inf_passes(torch_cuda, kind):
    torch = torch_cuda
    net = make_net(kind)
    n = net.n_params
    rng = np.random.default_rng(n + 1)
    g0 = torch.zeros(n, dtype=torch.float32, device="cuda")
    step(net, ALGO_OF[kind], batch(torch, rng, 32, net.A), flat_grad=g0)
    net.clip_grad(g0)
    norm0 = net.grad_norm()[0]
    # G = 0.5 norm: every element is fp32(g) * fp32(c), c = G / norm in fp32 from the device's norm
    G = float(np.float32(0.5 * norm0))
    net.set_max_grad_norm(G)
    assert net.max_grad_norm == G
    g = g0.clone()
    net.clip_grad(g)
    norm, scale = net.grad_norm()
    c = np.float32(G) / max(np.float32(norm), np.float32(G))
    assert norm == norm0 and np.float32(scale) == c and scale < 1.0
    assert np.array_equal(g.cpu().numpy(), g0.cpu().numpy() * c)
    new = f64_norm(g)
    print(f"{kind}: G {G!r}, clipped float64 norm {new!r}, rel {abs(new - G) / G:.3g}")
    assert abs(new - G) <= 1e-6 * G
    g2 = g0.clone()
    net.clip_grad(g2)                                            # equal inputs, equal bits
    assert torch.equal(g, g2) and net.grad_norm() == (norm, scale)
    # G = 2 norm: untouched, c exactly 1; G = norm itself: c = G / max(norm, G) = 1
    for G2 in (float(np.float32(2.0 * norm0)), norm0):
        net.set_max_grad_norm(G2)
        g = g0.clone()
        net.clip_grad(g)
        assert torch.equal(g, g0) and net.grad_norm() == (norm0, 1.0)
    # G = 0: untouched, the norm recorded
    net.set_max_grad_norm(0.0)
    g = g0.clone(); g[5] = 2.0 * g0[5] + 1.0
    ref = f64_norm(g)
    keep = g.clone()
    net.clip_grad(g)
    norm, scale = net.grad_norm()
    assert torch.equal(g, keep) and abs(norm - ref) <= 1e-6 * ref and scale == 1.0
    # one inf: unchanged, a non-finite norm, scale 1; a NaN likewise
    net.set_max_grad_norm(G)
    for bad in (float("inf"), float("nan")):
        g = g0.clone(); g[n // 2] = bad
        keep = g.clone()
        net.clip_grad(g)
        norm, scale = net.grad_norm()
        assert not math.isfinite(norm) and scale == 1.0
        assert np.array_equal(g.cpu().numpy().view(np.uint32), keep.cpu().numpy().view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- 3. the step
STEP_CASES = [("plain", "double"), ("plain", "doubleper"), ("dueling3", "double"), ("dueling3", "doubleper"), ("noisy", "c51doubleper"),
              ("qr", "qrdouble")]


def composed_step(torch, net, algo, bt, g):
    out = step(net, algo, bt, flat_grad=g)
    net.clip_grad(g)
    net.apply_adam(g)
    return out


@pytest.mark.parametrize("kind,algo", STEP_CASES)
def test_clipped_step_equals_export_clip_apply(torch_cuda, kind, algo):
    """net A: G set, train_step(flat_grad = None); net B: export, clip_grad, apply_adam.  G from a dry run (half the smallest of its
    three norms), so that the clip acts in every step: asserted on both nets"""
    torch = torch_cuda
    rng = np.random.default_rng(len(kind) * 100 + len(algo))
    dry, A, B = make_net(kind), make_net(kind), make_net(kind)
    bts = [batch(torch, rng, 32, A.A) for _ in range(3)]
    g = torch.zeros(A.n_params, dtype=torch.float32, device="cuda")
    norms = []
    for bt in bts:
        composed_step(torch, dry, algo, bt, g)
        norms.append(dry.grad_norm()[0])
    assert all(math.isfinite(x) and x > 0 for x in norms)
    G = 0.5 * min(norms)
    A.set_max_grad_norm(G); B.set_max_grad_norm(G)
    start = state(A)
    for k, bt in enumerate(bts):
        la = [x.clone() if x is not None else None for x in step(A, algo, bt)]
        lb = composed_step(torch, B, algo, bt, g)
        (na, ca), (nb, cb) = A.grad_norm(), B.grad_norm()
        assert (na, ca) == (nb, cb) and ca < 1.0, (k, na, ca, nb, cb)
        assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(la, lb)), k      # loss, abs_err, q_target: the step's
        assert same_state(torch, state(A), state(B)), k
    assert not torch.equal(state(A)[0], start[0]) and not same_state(torch, state(A), state(dry))      # (it trained, and the clip changed where to)
    b1 = np.float32(0.9)
    for _ in range(3):                                           # three ticks of beta1's power, no more
        b1 = b1 * np.float32(0.9)
    assert state(A)[3][0] == b1


@pytest.mark.parametrize("kind,algo", [("plain", "double"), ("noisy", "c51doubleper")])
def test_off_is_off(torch_cuda, kind, algo):
    """G = 0 set explicitly (and set to a value, then back): the fused step of a net on which the setter was never called"""
    torch = torch_cuda
    rng = np.random.default_rng(12)
    A, B = make_net(kind), make_net(kind)
    A.set_max_grad_norm(3.0); A.set_max_grad_norm(0.0)
    for _ in range(3):
        bt = batch(torch, rng, 32, A.A)
        la, lb = step(A, algo, bt), step(B, algo, bt)
        assert torch.equal(la[0], lb[0])
    assert same_state(torch, state(A), state(B))
    assert A.grad_norm() == (0.0, 1.0)                           # (nothing clipped, nothing recorded)


# ---------------------------------------------------------------------------------------------------------------- 5. fb_vec_step
def vec_net(arch, max_batch):
    from dqnflappybird_amd.vec import QNet
    net = QNet(2, 512, arch, max_batch=max_batch)
    net.init_params(3, which=0); net.init_params(4, which=1)
    for which in (0, 1):
        net.load_params(net.store_params(which) * 3.0, which)
    net.set_hparams(lr=1e-4)
    return net


def pipeline(N, B, prioritized=False, arch="plain", seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(N, seed=seed)
    rep = VecReplay(6 * N + 13 if prioritized else 20000, N, prioritized=prioritized)
    rep.seed(9, "numpy" if prioritized else "cpython")
    net = vec_net(arch, max(N, B))
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


def composed_vec_steps(torch, pipe, algo, B, steps, first, g, clip, one=None, other=None):
    """`steps` steps of act_nib -> frame_step -> push -> sample -> train_from_replay(flat_grad) -> clip_grad -> apply_adam (-> batch_update)
    on `pipe`; with `one` (a VecStep on `other`'s twin pipeline) every step is compared with fb_vec_step.  clip_grad with the limit 0 only
    records the norm (the dry run).  -> the norms of the train steps"""
    from dqnflappybird_amd.vec import train_from_replay
    env, rep, net, nib = pipe
    per = algo == "doubleper"
    norms = []
    for k in range(steps):
        train = k >= first
        a1 = net.act_nib(nib, 0.05, seed=1, step=k)
        env.frame_step(a1, want_u8=False)
        rep.push(env.frame_bits, a1, env.reward, env.terminal)
        if train:
            idx, isw = rep.sample(B)
            out = train_from_replay(rep, net, algo, idx, gamma=GAMMA, flat_grad=g, isw=isw, want_abs_err=per)
            net.clip_grad(g)
            net.apply_adam(g)
            if per:
                rep.update_priorities(idx, abs_err=out[4])
            norms.append(net.grad_norm())
        if one is None:
            continue
        a2 = one(0.05, seed=1, step=k, train=train)
        assert torch.equal(a1, a2), k
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(out[0], one.loss), k
            assert norms[-1] == other.grad_norm() and (not clip or norms[-1][1] < 1.0), (k, norms[-1], other.grad_norm())
            if per:
                assert torch.equal(isw, one.isw) and torch.equal(out[4], one.abs_err + 0.01), k
    return [x[0] for x in norms]


@pytest.mark.parametrize("algo", ["double", "doubleper"])
def test_vec_step_equals_composed_one_stream_calls(torch_cuda, algo):
    """256 envs, B = 32, 4 train steps: fb_vec_step == act_nib -> frame_step -> push -> sample -> train_from_replay(flat_grad) ->
    clip_grad -> apply_adam (-> batch_update), and no step took the split schedule.  G: an eighth of the smallest norm of a dry run of the
    same pipeline without a limit (Adam's steps hardly depend on the gradient's scale, so the clipped run sees much the same norms; the
    norms of these minibatches differ by up to ~4x): the clip acts in every step, asserted"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep
    N, B, steps, first = 256, 32, 8, 4
    per = algo == "doubleper"
    g = torch.zeros(N_PARAMS_DUELING2, dtype=torch.float32, device="cuda")
    dry = composed_vec_steps(torch, pipeline(N, B, per, "dueling"), algo, B, steps, first, g, False)
    assert len(dry) == steps - first and all(math.isfinite(x) and x > 0 for x in dry)
    G = min(dry) / 8
    p1, p2 = pipeline(N, B, per, "dueling"), pipeline(N, B, per, "dueling")
    (e1, r1, n1, _), (e2, r2, n2, _) = p1, p2
    n1.set_max_grad_norm(G); n2.set_max_grad_norm(G)
    composed_vec_steps(torch, p1, algo, B, steps, first, g, True, VecStep(e2, r2, n2, B, algo, GAMMA), n2)
    assert same_state(torch, state(n1), state(n2)) and (e1.get_state() == e2.get_state()).all()
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n2.split_stats() == (0, 0)


def test_unclipped_vec_step_still_takes_the_split_schedule(torch_cuda):
    """the control of the case above: the same shape without a limit takes the split schedule where the machine offers it (a side stream
    that runs beside the caller's), and a limit set afterwards takes the net off it"""
    from dqnflappybird_amd.vec import VecStep
    e, r, n, _ = pipeline(256, 32)
    one = VecStep(e, r, n, 32, "double", GAMMA)
    for k in range(6):
        one(0.05, seed=1, step=k, train=k >= 3)
    issued = n.split_stats()[0]
    assert issued in (0, 3)
    n.set_max_grad_norm(1e-3)
    for k in range(6, 9):
        one(0.05, seed=1, step=k, train=True)
    assert n.split_stats()[0] == issued and n.grad_norm()[0] > 0


# ---------------------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_everything_as_it_was(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import TrainSteps, VecGameState, VecReplay
    net = make_net("plain")
    net.set_max_grad_norm(2.5)
    before = state(net)
    lib = L.lib()
    for bad in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert lib.fb_qnet_set_max_grad_norm(net.h, C.c_float(bad)) == -1, bad
        assert "finite and >= 0" in lib.fb_last_error().decode()
        with pytest.raises(ValueError, match="max_grad_norm must be finite and >= 0"):
            net.set_max_grad_norm(bad)
        assert net.max_grad_norm == 2.5
    for bad in (0.0, -0.25, 1.0000001, 2.0, float("nan"), float("inf")):
        assert lib.fb_qnet_soft_sync_target(net.h, C.c_float(bad), None) == -1, bad
        assert "rho must be in (0, 1]" in lib.fb_last_error().decode()
        with pytest.raises(ValueError, match="polyak \\(rho\\) must be in \\(0, 1\\]"):
            net.soft_sync_target(bad)
    target = net.store_params(1).clone()
    # fb_train_steps on a net that clips
    N = 16
    env, rep = VecGameState(N, seed=3), VecReplay(2000, N)
    env.observe(); rep.reset(env.frame_bits)
    acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
    for _ in range(12):
        env.frame_step(acts, want_u8=False)
        rep.push(env.frame_bits, acts, env.reward, env.terminal)
    rep.seed(9, "cpython")
    blob = np.asarray(rep.state_blob()).copy()
    ts = TrainSteps(rep, net, 8, "double", GAMMA)
    with pytest.raises(ValueError, match="fb_train_steps: the net clips its gradient"):
        ts(2)
    assert np.array_equal(np.asarray(rep.state_blob()), blob)    # (no draw: the generator has not moved)
    assert same_state(torch, state(net), before) and torch.equal(net.store_params(1), target)
    assert lib.fb_qnet_clip_grad(net.h, None, None) == -1 and lib.fb_qnet_grad_norm(None, None, None) == -1
    net.set_max_grad_norm(0.0)
    ts(2)                                                        # ... and with the limit off it runs
    assert not torch.equal(net.store_params(), before[0])


# ---------------------------------------------------------------------------------------------------------------- data parallel
def test_reduce_apply_at_world_size_1_clips_behind_the_reduction(torch_cuda):
    """fb_dist_reduce_apply on a net with G active == clip_grad + apply_adam (the all-reduce over one rank is the identity)"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.dist import NativeDP
    nd = NativeDP(rank=0, world=1, overlap=False)
    try:
        rng = np.random.default_rng(21)
        dry, A, B = make_net("plain"), make_net("plain"), make_net("plain")
        ga, gb = (torch.zeros(A.n_params, dtype=torch.float32, device="cuda") for _ in range(2))
        bts = [batch(torch, rng, 32, 2) for _ in range(3)]
        norms = []
        for bt in bts:                                           # the dry run: the norms without a limit
            composed_step(torch, dry, "double", bt, ga)
            norms.append(dry.grad_norm()[0])
        G = min(norms) / 4
        A.set_max_grad_norm(G); B.set_max_grad_norm(G)
        for k, bt in enumerate(bts):
            step(A, "double", bt, flat_grad=ga); step(B, "double", bt, flat_grad=gb)
            assert torch.equal(ga, gb)
            L.check(L.lib().fb_dist_reduce_apply(nd.handle, A.h, L.ptr(ga), 1, L.current_stream()), "fb_dist_reduce_apply")
            B.clip_grad(gb); B.apply_adam(gb)
            assert A.grad_norm() == B.grad_norm() and A.grad_norm()[1] < 1.0, (k, A.grad_norm())
            assert torch.equal(ga, gb) and same_state(torch, state(A), state(B)), k
    finally:
        torch.cuda.synchronize()
        nd.close()
