"""Munchausen-DQN on the device (include/fbdqn.h: FB_ALGO_MDQN / FB_ALGO_MDQN_PER), in both loss bodies: the fused small-batch one in
fc1_bwd2_md_kernel (B <= 255) and loss_head_md_kernel behind the LDS-staged pass (B = 256, where the plan's c.big begins: a slice of 256
states).  References: float64 autograd through tests/test_oracle_qnet.py::torch_forward with the target of
tests/test_mdqn_host.py::np_mdqn_target, under the bounds the scalar-algo tests use (tests/test_gpu_qnet.py Q_ATOL,
tests/test_gpu_shapes.py::check_scalar_grads, tests/test_gpu_kinkfree_grads.py for the ring-fed form) -- the target is 1-Lipschitz in
every q it reads and has no argmax, so nothing is masked and nothing widened; exact heads for the header's hand cases; FB_ALGO_NATURE bit
for bit at one action; the PER form; and every composition (fused Adam, ring-fed, fb_train_steps, fb_vec_step, fb_vec_step_dp) bit for bit."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests.test_exact_heads_host import with_head
from tests.test_gpu_configs import BF16_GRAD_REL, BF16_Q_REL
from tests.test_gpu_exact_heads import batch as exact_batch
from tests.test_gpu_exact_heads import make_net as exact_net
from tests.test_gpu_nstep import played
from tests.test_gpu_nstep_per import per_memory
from tests.test_gpu_qnet import Q_ATOL, rand_states
from tests.test_gpu_shapes import arch_of, check_scalar_grads, make_scalar, scalar_batch
from tests.test_mdqn_host import ALPHA, CLIP, TAU, np_mdqn_target
from tests.test_oracle_qnet import tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
GAMMA = 0.99
G3 = 0.99 * 0.99 * 0.99
SMALL_MAX = 255                       # the largest batch of the fused small-batch loss (run_plan: c.big = a slice of >= 256 states)
SHAPES = [(128, 1, False), (512, 2, False), (384, 3, True), (128, 8, False)]
BATCHES = [1, 32, SMALL_MAX, SMALL_MAX + 1, 256]
BATCHES = sorted(set(BATCHES))        # (SMALL_MAX + 1 is 256, the largest batch a train step takes)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


_nets = {}


def scalar_net(oracle, fc, A, dueling):
    """one net per shape for the gradient-exporting cases (they leave it as it was)"""
    key = (fc, A, dueling)
    if key not in _nets:
        _nets[key] = make_scalar(oracle, fc, A, dueling, 256)
    return _nets[key]


def autograd_ref(torch, p_on, p_tg, fc, A, dueling, s, a, r, s2, t, w, gammas, md=(TAU, ALPHA, CLIP)):
    """float64: one forward of the three slices, then per Gamma (y, loss, |err|, flat gradient)"""
    P = torch.from_numpy(p_on.astype(np.float64)).requires_grad_(True)
    T = torch.from_numpy(p_tg.astype(np.float64))
    S, S2 = torch.from_numpy(s).double(), torch.from_numpy(s2).double()
    q = torch_forward(P, S, fc, A, dueling)
    with torch.no_grad():
        q_s, q_s2 = torch_forward(T, S, fc, A, dueling).numpy(), torch_forward(T, S2, fc, A, dueling).numpy()
    R = np.where(r == np.float32(0.1), 0.1, r.astype(np.float64))           # (the kernels read the reward 0.1f as 0.1, as the other algos do)
    qa = q[torch.arange(len(a)), torch.from_numpy(a.astype(np.int64))]
    wt = torch.ones(len(a), dtype=torch.float64) if w is None else torch.from_numpy(w.astype(np.float64))
    out = []
    for G in gammas:
        y = np.float32(np_mdqn_target(q_s, q_s2, a, R, t, G, *md)[0]).astype(np.float64)      # (fed as float32, like every y here)
        d = torch.from_numpy(y) - qa
        loss = (wt * d * d).mean()
        g, = torch.autograd.grad(loss, P, retain_graph=True)
        out.append((y, loss.item(), d.detach().abs().numpy(), g.numpy()))
    return out, q_s, q_s2


def kink_free_batch(oracle, cfg, p_on, tag, B, A, algo):
    """tests/test_gpu_shapes.py::test_scalar_train_step's draw: at B <= 32 whole batches are rejected until the oracle's ReLU / pool margin
    clears 2e-5, so that every gradient element is comparable"""
    small = B <= 32
    for attempt in range(50 if small else 1):
        rng = np.random.default_rng(zlib.crc32(f"mdqn-{tag}-{B}-{attempt}".encode()))
        bt = scalar_batch(rng, B, A, "per" if algo == "mdqnper" else "nature")
        if not small:
            return bt, small
        oracle.forward(p_on, cfg, bt[0])
        if oracle.last_margin() > 2e-5:
            return bt, small
    pytest.fail("no kink-free batch found")


def run_and_check(torch, net, fc, A, dueling, algo, bt, refs, gammas, small):
    s, a, r, s2, t, isw = bt
    d = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    for G, (y0, loss0, ae0, g0) in zip(gammas, refs):
        loss, ae, y = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(isw), gamma=G, flat_grad=grad)
        y, ae, loss, g = y.cpu().numpy(), ae.cpu().numpy(), loss.item(), grad.cpu().numpy()
        print(f"mdqn ({fc}, {A}, {arch_of(dueling)}) {algo} B={len(a)} Gamma={G:.4f}: max|y - y0| {np.abs(y - y0).max():.2e}  "
              f"max|ae - ae0| {np.abs(ae - ae0).max():.2e}  loss {loss:.6g} / {loss0:.6g}")
        np.testing.assert_allclose(y, y0, rtol=0, atol=Q_ATOL)
        np.testing.assert_allclose(ae, ae0, rtol=0, atol=2 * Q_ATOL)
        np.testing.assert_allclose(loss, loss0, rtol=1e-4, atol=1e-6)
        check_scalar_grads(g, g0, fc, A, dueling, small)


# ================================================================================================================ against float64 autograd
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("fc,A,dueling", SHAPES)
def test_train_step_matches_autograd(torch_cuda, oracle, fc, A, dueling, B):
    """loss, y, |err| and every gradient tensor at n = 1 (gamma) and with Gamma = gamma^3; every minibatch holds terminals from B = 32 on"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, fc, A, dueling)
    assert net.munchausen() == tuple(np.float32(x) for x in (TAU, ALPHA, CLIP))
    bt, small = kink_free_batch(oracle, cfg, p_on, f"{fc}-{A}-{dueling}", B, A, "mdqn")
    if B >= 32:
        assert bt[4].any() and not bt[4].all()
    gammas = (GAMMA, G3)
    refs, _, _ = autograd_ref(torch, p_on, p_tg, fc, A, dueling, *bt[:5], None, gammas)
    run_and_check(torch, net, fc, A, dueling, "mdqn", bt, refs, gammas, small)
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)          # gradient-only mode


@pytest.mark.parametrize("B", [32, 256])
def test_other_parameters(torch_cuda, oracle, B):
    """(tau, alpha, l0) = (0.1, 0.5, -0.25) reach both kernels; the default values come back afterwards"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 512, 2, False)
    md = (0.1, 0.5, -0.25)
    bt, small = kink_free_batch(oracle, cfg, p_on, "other", B, 2, "mdqn")
    refs, q_s, _ = autograd_ref(torch, p_on, p_tg, 512, 2, False, *bt[:5], None, (GAMMA,), md)
    lp = np_mdqn_target(q_s, q_s, bt[1], np.zeros(B), np.ones(B), 0.0, md[0], 1.0, -1e9)[1]
    if B == 256:
        assert (lp < md[2]).any() and (lp > md[2]).any()                   # clipped and unclipped bonuses
    net.set_munchausen(*md)
    try:
        assert net.munchausen() == tuple(np.float32(x) for x in md)
        run_and_check(torch, net, 512, 2, False, "mdqn", bt, refs, (GAMMA,), small)
    finally:
        net.set_munchausen()
    assert net.munchausen() == tuple(np.float32(x) for x in (TAU, ALPHA, CLIP))


@pytest.mark.parametrize("B", [32, 256])
def test_q_gaps_beyond_2000_tau(torch_cuda, oracle, B):
    """the target net's head scaled so that a quarter of the samples' Q gaps exceed 2000 tau = 60 (exp(-2000) is 0 in every format):
    the log-sum-exp neither overflows nor loses the maximum"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 512, 2, False)
    bt, small = kink_free_batch(oracle, cfg, p_on, "gaps", B, 2, "mdqn")
    head = tensor_bounds(512, 2, "plain")[8][1]
    _, q_s, q_s2 = autograd_ref(torch, p_on, p_tg, 512, 2, False, *bt[:5], None, ())
    gaps = np.abs(np.concatenate([q_s[:, 0] - q_s[:, 1], q_s2[:, 0] - q_s2[:, 1]]))
    k = np.float32(2000 * TAU * 1.02 / np.quantile(gaps, 0.75))
    p_big = p_tg.copy()
    p_big[head:] *= k
    refs, q_s, q_s2 = autograd_ref(torch, p_on, p_big, 512, 2, False, *bt[:5], None, (GAMMA,))
    gaps = np.abs(np.concatenate([q_s[:, 0] - q_s[:, 1], q_s2[:, 0] - q_s2[:, 1]]))
    print(f"head x {k:.1f}: gaps / tau: median {np.median(gaps) / TAU:.0f} max {gaps.max() / TAU:.0f}; max|Q-| {max(np.abs(q_s).max(), np.abs(q_s2).max()):.1f}")
    assert (gaps > 2000 * TAU).mean() > 0.2
    net.load_params(p_big, 1)
    try:
        run_and_check(torch, net, 512, 2, False, "mdqn", bt, refs, (GAMMA,), small)
    finally:
        net.load_params(p_tg, 1)


# ================================================================================================================ exact heads
@pytest.mark.parametrize("B", [32, 256])
def test_hand_cases_on_the_kernel(torch_cuda, B):
    """zero head weights, chosen biases (tests/test_gpu_exact_heads.py): the header's worked cases on both loss bodies within 1e-6"""
    torch = torch_cuda
    net, ps = exact_net("plain", 2, 256)
    s, a, r, s2, t, _ = exact_batch(B, 2, 7)
    d = lambda x: torch.from_numpy(x).cuda()
    on = np.float32([0.5, -1.0])
    R = r.astype(np.float64)
    for c in (0.0, 1.5, -7.25):                                      # q-(s) = (c, c): the bonus is -alpha tau ln 2 for both actions
        net.load_params(with_head(ps[0], 512, 2, "plain", 0, on), 0)
        net.load_params(with_head(ps[1], 512, 2, "plain", 0, np.float32([c, c])), 1)
        _, _, y = net.train_step("mdqn", d(s), d(a), d(r), d(s2), d(t), gamma=0.5, flat_grad=torch.zeros(net.n_params, device="cuda"))
        assert np.abs(y.cpu().numpy() - (R - ALPHA * TAU * np.log(2.0) + np.where(t != 0, 0.0, 0.5 * (c + TAU * np.log(2.0))))).max() < 1e-6
    # q-(.) = (0, 2): -0.9 for a = 0 (clipped), -0 for a = 1; V = 2 + tau log1p(exp(-66.7)) = 2; done: y = R + bonus
    net.load_params(with_head(ps[1], 512, 2, "plain", 0, np.float32([0.0, 2.0])), 1)
    grad = torch.zeros(net.n_params, device="cuda")
    loss, ae, y = net.train_step("mdqn", d(s), d(a), d(r), d(s2), d(t), gamma=0.5, flat_grad=grad)
    bonus = np.where(a == 0, -0.9, -0.0)
    y0 = R + bonus + np.where(t != 0, 0.0, 0.5 * 2.0)
    assert t.any() and np.abs(y.cpu().numpy() - y0).max() < 1e-6
    assert np.abs(y.cpu().numpy()[t != 0] - (R + bonus)[t != 0]).max() < 1e-6
    d0 = y0 - on[a]
    assert np.abs(ae.cpu().numpy() - np.abs(d0)).max() < 1e-6 and abs(loss.item() - np.mean(d0 * d0)) < 1e-5
    gb = grad.cpu().numpy()[tensor_bounds(512, 2, "plain")[9][1]:]
    want = np.array([np.sum(-2.0 / B * d0[a == k]) for k in (0, 1)])
    np.testing.assert_allclose(gb, want, rtol=1e-5, atol=1e-6)


# ================================================================================================================ the A = 1 anchor
@pytest.mark.parametrize("B", [32, SMALL_MAX, 256])
@pytest.mark.parametrize("dueling", [False, True])
def test_one_action_is_nature_bit_for_bit(torch_cuda, oracle, B, dueling):
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 128, 1, dueling) if not dueling else make_scalar(oracle, 128, 1, True, 256)
    s, a, r, s2, t, _ = scalar_batch(np.random.default_rng(B), B, 1, "nature")
    d = lambda x: torch.from_numpy(x).cuda()
    out = {}
    for algo in ("nature", "mdqn"):
        grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        loss, ae, y = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=grad)
        out[algo] = (loss.clone(), ae.clone(), y.clone(), grad)
    for x, z in zip(out["nature"], out["mdqn"]):
        assert torch.equal(x, z)
    assert out["mdqn"][3].abs().max() > 0


# ================================================================================================================ the PER form
@pytest.mark.parametrize("B", [32, 256])
def test_per_form(torch_cuda, oracle, B):
    """mdqnper with w = 1 is mdqn bit for bit; a random w matches autograd (|err| without the weight)"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 384, 3, True)
    bt, small = kink_free_batch(oracle, cfg, p_on, "per", B, 3, "mdqnper")
    s, a, r, s2, t, isw = bt
    d = lambda x: torch.from_numpy(x).cuda()
    out = {}
    for algo, w in (("mdqn", None), ("mdqnper", np.ones(B, np.float32))):
        grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        loss, ae, y = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=None if w is None else d(w), gamma=GAMMA, flat_grad=grad)
        out[algo] = (loss.clone(), ae.clone(), y.clone(), grad)
    for x, z in zip(out["mdqn"], out["mdqnper"]):
        assert torch.equal(x, z)
    refs, _, _ = autograd_ref(torch, p_on, p_tg, 384, 3, True, s, a, r, s2, t, isw, (GAMMA,))
    run_and_check(torch, net, 384, 3, True, "mdqnper", bt, refs, (GAMMA,), small)


def test_batch_update_receives_abs_err(torch_cuda):
    """fb_vec_step(mdqnper): abs_err is |y - q(s, a)| of the step's own train call, and the tree holds min(|err| + 0.01, 1)^0.6 at idx"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    N, B = 32, 32
    (e1, r1, n1, nib1), (e2, r2, n2, _) = _pipeline(N, B, 1, True), _pipeline(N, B, 1, True)
    one = VecStep(e2, r2, n2, B, "mdqnper", GAMMA)
    for step in range(8):
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        one(0.05, seed=1, step=step, train=step >= 3)
        if step >= 3:
            idx, isw = r1.sample(B)
            s, a, r, s2, t = r1.gather(idx)
            _, ae, _ = n1.train_step("mdqnper", s, a, r, s2, t, isw=isw, gamma=GAMMA)
            assert torch.equal(idx, one.idx) and torch.equal(ae, one.abs_err), step
            r1.update_priorities(idx, abs_err=ae.clone())
            tree = r2.per_state()[0]
            want = np.minimum(ae.cpu().numpy().astype(np.float64) + 0.01, 1.0)
            il = idx.cpu().tolist()
            for i, w in zip(il, want):
                if il.count(i) == 1:                                   # (a leaf drawn twice keeps one of its two updates)
                    assert abs(tree[i] - w ** 0.6) < 1e-5, (step, i)
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


# ================================================================================================================ composition
def _net(arch="plain", max_batch=256):
    from dqnflappybird_amd.vec import QNet
    net = QNet(2, 512, arch, max_batch=max_batch)
    net.init_params(3, which=0); net.init_params(4, which=1)
    for which in (0, 1):                                              # (x 3: a trunk whose ReLUs switch, Q of O(1))
        net.load_params(net.store_params(which) * 3.0, which)
    net.set_hparams(lr=1e-4)
    return net


def _pipeline(N, B, n, prioritized=False, arch="plain", seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(N, seed=seed)
    if prioritized:
        rep = per_memory(6 * N + 13, N, n, "exact")
    else:
        rep = VecReplay(max(20000, 16 * N), N)
        rep.set_n_step(n, GAMMA)
        rep.seed(9, "cpython")
    net = _net(arch, max(N, B))
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


@pytest.mark.parametrize("B", [32, 256])
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, B):
    torch = torch_cuda
    nets = [_net("dueling"), _net("dueling")]
    s, a, r, s2, t, _ = scalar_batch(np.random.default_rng(B), B, 2, "nature")
    d = lambda x: torch.from_numpy(x).cuda()
    args = (d(s), d(a), d(r), d(s2), d(t))
    grad = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    before = nets[0].store_params().clone()
    for _ in range(2):
        l0 = nets[0].train_step("mdqn", *args, flat_grad=grad)[0].clone()
        nets[0].apply_adam(grad)
        l1 = nets[1].train_step("mdqn", *args)[0]
        assert torch.equal(l0, l1)
    assert torch.equal(nets[0].store_params(), nets[1].store_params()) and not torch.equal(nets[0].store_params(), before)
    (m0, v0, p0), (m1, v1, p1) = nets[0].adam_state(), nets[1].adam_state()
    assert torch.equal(m0, m1) and torch.equal(v0, v1) and np.array_equal(p0, p1)
    assert torch.equal(nets[0].store_params(1), nets[1].store_params(1))


@pytest.mark.parametrize("n", [1, 3])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(64, 4000, 40, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (32, SMALL_MAX, 256):
        # B = 256: the separate calls run the large-batch trunk (another summation order in conv2 / conv3), so equal to rounding only,
        # for every algo: the allowance of tests/test_gpu_shims.py::test_train_from_replay_equals_gather_plus_train_step
        same = torch.equal if B < 256 else (lambda x, y: torch.allclose(x, y, rtol=2e-4, atol=2e-6))
        n1, n2 = _net(), _net()
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(2):
            idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, _, _ = n1.train_step("mdqn", s, a, r, s2, t, gamma=G, flat_grad=g1 if exp else None, want_aux=False)
            l2, a2, r2, t2 = train_from_replay(rep, n2, "mdqn", idx, gamma=GAMMA, flat_grad=g2 if exp else None)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert same(l1, l2), (n, B, step)
            if exp:
                assert (torch.equal(g1, g2) if B < 256 else torch.allclose(g1, g2, rtol=2e-3, atol=2e-5 * g1.abs().max().item())) and g1.abs().max() > 0
                n1.apply_adam(g1); n2.apply_adam(g2)
            if B < 256:                                        # (at 256 Adam turns gradients that differ in rounding into steps of +-lr where they are ~0)
                assert torch.equal(n1.store_params(), n2.store_params()), (n, B, step)
            elif step == 0:
                break


def test_train_steps_equals_separate_calls(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import TrainSteps, train_from_replay
    B = 32

    def make():
        _, rep = played(256, 20000, 14, seed=5)
        rep.seed(9, "cpython")
        net = _net()
        return rep, net, TrainSteps(rep, net, B, "mdqn", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    before = n1.store_params().clone()
    for _ in range(5):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "mdqn", idx, gamma=GAMMA)
    ts2(5)
    assert torch.equal(n1.store_params(), n2.store_params()) and not torch.equal(n1.store_params(), before)


@pytest.mark.parametrize("N", [32, 256])
def test_vec_step_equals_composed_calls(torch_cuda, N):
    """uniform memory: 32 envs gather, 256 envs train from the ring beside the acting forward (the split schedule double takes)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 16
    (e1, r1, n1, nib1), (e2, r2, n2, _) = _pipeline(N, B, 1), _pipeline(N, B, 1)
    one = VecStep(e2, r2, n2, B, "mdqn", GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 6 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, _ = r1.sample(B)
            loss, a, r, t = train_from_replay(r1, n1, "mdqn", idx, gamma=GAMMA)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
    assert torch.equal(n1.store_params(), n2.store_params()) and (e1.get_state() == e2.get_state()).all()


@pytest.mark.parametrize("N", [32, 256])
def test_prioritized_vec_step_equals_composed_calls(torch_cuda, N):
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps = 32, 12
    (e1, r1, n1, nib1), (e2, r2, n2, _) = _pipeline(N, B, 1, True, "dueling"), _pipeline(N, B, 1, True, "dueling")
    one = VecStep(e2, r2, n2, B, "mdqnper", GAMMA)
    for step in range(steps):
        train = step >= 2
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
            loss, _, _, _, ae = train_from_replay(r1, n1, "mdqnper", idx, gamma=GAMMA, isw=isw, want_abs_err=True)
            r1.update_priorities(idx, abs_err=ae)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(isw, one.isw), step
            assert torch.equal(loss, one.loss) and torch.equal(ae, one.abs_err + 0.01), step
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(n1.store_params(), n2.store_params())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


def test_vec_step_dp_world1_equals_vec_step(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.dist import NativeDP
    from dqnflappybird_amd.vec import VecStep
    N, B, steps = 256, 32, 14
    nd = NativeDP(rank=0, world=1, overlap=False)
    try:
        (e1, r1, n1, _), (e2, r2, n2, _) = _pipeline(N, B, 1), _pipeline(N, B, 1)
        g2 = torch.zeros(n2.n_params, device="cuda")
        fused, dp = VecStep(e1, r1, n1, B, "mdqn", GAMMA), VecStep(e2, r2, n2, B, "mdqn", GAMMA, flat_grad=g2, dist=nd)
        for step in range(steps):
            train = step >= 4
            a1 = fused(0.05, seed=1, step=step, train=train).clone()
            a2 = dp(0.05, seed=1, step=step, train=train)
            assert torch.equal(a1, a2), step
            if train:
                assert torch.equal(fused.idx, dp.idx) and torch.equal(fused.loss, dp.loss), step
        assert torch.equal(n1.store_params(), n2.store_params())
    finally:
        torch.cuda.synchronize()
        nd.close()


# ================================================================================================================ setter and refusals
def snapshot(net, rep=None):
    m, v, pows = net.adam_state()
    out = [net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), pows.copy(), net.munchausen()]
    if rep is not None:
        out.append(np.asarray(rep.state_blob()).copy())
    return out


def same(x, y):
    import torch
    return all(torch.equal(p, q) if torch.is_tensor(p) else np.array_equal(p, q) for p, q in zip(x, y))


def test_setter_and_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, TrainSteps, VecStep, train_from_replay
    net = _net()
    lib = L.lib()
    assert net.munchausen() == tuple(np.float32(x) for x in L.MDQN_DEFAULTS)
    net.set_munchausen(0.1, 0.5, -0.25)
    before = snapshot(net)
    nan, inf = float("nan"), float("inf")
    for bad in ((0.0, 0.9, -1.0), (-1.0, 0.9, -1.0), (nan, 0.9, -1.0), (inf, 0.9, -1.0), (0.03, -0.1, -1.0), (0.03, 1.1, -1.0), (0.03, nan, -1.0),
                (0.03, 0.9, 0.1), (0.03, 0.9, -inf), (0.03, 0.9, nan)):
        assert lib.fb_qnet_set_munchausen(net.h, *bad) == -1, bad
        assert "fb_qnet_set_munchausen" in lib.fb_last_error().decode()
        assert same(before, snapshot(net)), bad
    net.set_munchausen(0.03, 0.0, 0.0)                                   # the closed ends are accepted
    net.set_munchausen(0.1, 0.5, -0.25)
    # the setter, the getter and the algos on C51 / QR / noisy nets; C51 / QR algos on the scalar net
    s, a, r, s2, t, _ = scalar_batch(np.random.default_rng(1), 32, 2, "nature")
    d = lambda x: torch.from_numpy(x).cuda()
    args = (d(s), d(a), d(r), d(s2), d(t))
    w = torch.ones(32, device="cuda")
    for kw in (dict(arch="c51"), dict(arch="qr"), dict(arch="c51dueling", noisy=True)):
        other = QNet(2, 512, max_batch=32, **kw)
        other.init_params(1, 0); other.init_params(2, 1)
        with pytest.raises(ValueError, match="scalar heads only"):
            other.set_munchausen()
        with pytest.raises(ValueError, match="scalar heads only"):
            other.munchausen()
        p0 = other.store_params().clone()
        for algo in ("mdqn", "mdqnper"):
            with pytest.raises(ValueError, match="net trains with"):
                other.train_step(algo, *args, isw=w)
        assert torch.equal(p0, other.store_params())
    for algo in ("c51", "qrper"):
        with pytest.raises(ValueError, match="needs a"):
            net.train_step(algo, *args, isw=w)
    with pytest.raises(ValueError, match="PER needs isw"):
        net.train_step("mdqnper", *args)
    assert same(before, snapshot(net))
    # memory kinds, in every ring-fed call
    _, uni = played(32, 4000, 6, seed=5)
    uni.seed(9, "cpython")
    env, per, _, _ = _pipeline(32, 32, 1, True)
    for step in range(4):
        acts = torch.zeros(32, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        per.push(env.frame_bits, acts, env.reward, env.terminal)
    idx = torch.arange(32, device="cuda")
    pidx, pw = per.sample(32)
    before_u, before_p = snapshot(net, uni), snapshot(net, per)
    with pytest.raises(ValueError, match="FB_ALGO_MDQN trains from a uniform memory only"):
        train_from_replay(per, net, "mdqn", pidx, gamma=GAMMA, isw=pw)
    with pytest.raises(ValueError, match="FB_ALGO_MDQN_PER trains from a prioritized memory only"):
        train_from_replay(uni, net, "mdqnper", idx, gamma=GAMMA, isw=w)
    with pytest.raises(ValueError, match="importance weights"):
        train_from_replay(per, net, "mdqnper", pidx, gamma=GAMMA)
    rc = lib.fb_train_from_replay(per.h, net.h, L.ALGO_MDQN_PER, 32, L.ptr(pidx), None, L.ptr(args[1]), L.ptr(args[2]), L.ptr(args[4]),
                                  C.c_double(GAMMA), L.ptr(w), None, None, L.current_stream())
    assert rc == -1 and "importance weights" in lib.fb_last_error().decode()
    with pytest.raises(ValueError, match="TrainSteps is for uniform replay"):
        TrainSteps(uni, net, 32, "mdqnper", GAMMA)
    ts = TrainSteps(uni, net, 32, "nature", GAMMA)
    ts.replay, ts.algo = per, L.ALGO_MDQN                             # (past the Python check: the library's own refusal)
    with pytest.raises(ValueError, match="uniform memory only"):
        ts(1)
    ts.replay, ts.algo = uni, L.ALGO_MDQN_PER
    with pytest.raises(ValueError, match="prioritized replay needs the importance weights"):
        ts(1)
    env_u = played(32, 4000, 1, seed=6)[0]
    env_u.track_state()
    with pytest.raises(ValueError, match="go with a prioritized memory"):
        VecStep(env_u, uni, net, 32, "mdqnper", GAMMA)
    with pytest.raises(ValueError, match="go with a prioritized memory"):
        VecStep(env_u, per, net, 32, "mdqn", GAMMA)
    one = VecStep(env_u, uni, net, 32, "nature", GAMMA)
    one.replay = per                                                   # (past the Python check again)
    one.algo = L.ALGO_MDQN
    with pytest.raises(ValueError, match="uniform memory only"):
        one(0.05, seed=1, step=0)
    one.replay, one.algo = uni, L.ALGO_MDQN_PER
    with pytest.raises(ValueError):
        one(0.05, seed=1, step=0)
    torch.cuda.synchronize()
    assert same(before_u, snapshot(net, uni)) and same(before_p, snapshot(net, per))
    assert net.munchausen() == tuple(np.float32(x) for x in (0.1, 0.5, -0.25))


# ================================================================================================================ bf16 training
@pytest.mark.parametrize("B", [32, 256])
def test_bf16_train_dtype(torch_cuda, oracle, B):
    """bf16 operands against the fp32 device result, within tests/test_gpu_configs.py's bounds; back in f32 the step is bit-identical"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 512, 2, False)
    # the net and the minibatch of tests/test_gpu_configs.py::test_bf16_training_gradients_within_relative_bound, on which the project's
    # bounds were set (make_scalar(512, 2) holds trained_like_params(1) / (2); the same generator, the same order of draws)
    rng = np.random.default_rng(B)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = rng.integers(0, 2, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    t = (r == -3).astype(np.uint8)
    d = lambda x: torch.from_numpy(x).cuda()
    args = (d(s), d(a), d(r), d(s2), d(t))

    def step(algo="mdqn"):
        grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        loss, ae, y = net.train_step(algo, *args, gamma=GAMMA, flat_grad=grad)
        return loss.clone(), ae.clone(), y.clone(), grad

    f32 = step()
    net.set_train_dtype("bf16")
    try:
        bf = step()
    finally:
        net.set_train_dtype("f32")
    again = step()
    assert all(torch.equal(x, z) for x, z in zip(f32, again))
    y32, ybf = f32[2].cpu().numpy(), bf[2].cpu().numpy()
    assert not np.array_equal(y32, ybf)
    assert np.abs(ybf - y32).max() < BF16_Q_REL * np.abs(y32).max()
    g32, gbf = f32[3].cpu().numpy(), bf[3].cpu().numpy()
    errs = {name: np.linalg.norm(gbf[lo:hi] - g32[lo:hi]) / np.linalg.norm(g32[lo:hi]) for name, lo, hi in tensor_bounds(512, 2, "plain")}
    print(f"bf16 B={B} mdqn: max|y_bf16 - y_f32| / max|y| {np.abs(ybf - y32).max() / np.abs(y32).max():.4f}  per-tensor gradient error "
          + "  ".join(f"{k} {v:.4f}" for k, v in errs.items()))
    for name, err in errs.items():
        assert 0 < err < BF16_GRAD_REL, (name, err)


# ================================================================================================================ end to end
def test_vecbrain_end_to_end(torch_cuda, tmp_path):
    """VecBrain(algo='mdqn') at 64 envs: a few hundred steps, save / load continues bit for bit and records (tau, alpha, l0), a brain
    with other values refuses the checkpoint by name, evaluate() plays"""
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="mdqn", arch="dueling", batch=32, capacity=20000, observe=20, seed=3, replace_target_iter=50, n_step=3)
    a = VecBrain(64, **kw)
    assert a.net.munchausen() == a.munchausen == tuple(np.float32(x) for x in (TAU, ALPHA, CLIP))
    a.net.set_hparams(lr=1e-4)
    p0 = a.net.store_params().clone()
    a.run(300, log_every=0)
    assert np.isfinite(a.last_loss.item()) and not torch.equal(p0, a.net.store_params())
    ck = str(tmp_path / "ck")
    a.save(ck)
    assert tuple(np.load(ck + ".npz")["munchausen"].tolist()) == a.munchausen
    b = VecBrain(64, **dict(kw, seed=77))
    b.net.set_hparams(lr=1e-4)
    b.load(ck)
    for _ in range(10):
        a.step(); b.step()
        assert torch.equal(a.one_step.actions, b.one_step.actions) and torch.equal(a.one_step.loss, b.one_step.loss)
    assert torch.equal(a.net.store_params(), b.net.store_params())
    with pytest.raises(ValueError, match="was trained with munchausen \\(tau, alpha, clip\\)"):
        VecBrain(64, **dict(kw, tau=0.1)).load(ck)
    VecBrain(64, **dict(kw, algo="nature")).load(ck)                   # the parameters are a scalar net's: another scalar algo takes them
    res = a.evaluate(n_envs=64, max_steps=500)
    assert res.mean_score >= 0 and torch.equal(a.net.store_params(), b.net.store_params())
