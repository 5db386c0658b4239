"""The Huber (clipped-error) loss and FB_ALGO_DOUBLE_PER on the device (include/fbdqn.h), in both scalar loss bodies: the fused
small-batch one (fc1_bwd2_x_kernel, B <= 255) and loss_head_x_kernel behind the LDS-staged pass (B = 256).  References: float64 autograd
through tests/test_oracle_qnet.py::torch_forward with the loss and targets of tests/test_huber_host.py, under the bounds the scalar-algo
tests use (tests/test_gpu_qnet.py Q_ATOL, tests/test_gpu_shapes.py::check_scalar_grads); exact heads for the header's hand-worked case,
|d| = delta and the first maximum on ties; the bit-for-bit statements of the header; every composition (fused Adam, ring-fed,
fb_train_steps, fb_vec_step on both schedules, fb_vec_step_dp); bf16 training; refusals that leave everything where it was; VecBrain.

The double target's a*: the scalar `double` cases of tests/test_gpu_shapes.py mask nothing, so nothing is masked here; the minibatches are
drawn (on the CPU reference) so that the online net's two best q(s', .) are more than Q_ATOL apart on every sample, and the case asserts it."""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests.test_exact_heads_host import tie_patterns, with_head
from tests.test_gpu_configs import BF16_GRAD_REL, BF16_Q_REL
from tests.test_gpu_exact_heads import batch as exact_batch
from tests.test_gpu_exact_heads import make_net as exact_net
from tests.test_gpu_mdqn import _net, _pipeline
from tests.test_gpu_nstep import played
from tests.test_gpu_qnet import Q_ATOL, rand_states
from tests.test_gpu_shapes import arch_of, check_scalar_grads, make_scalar, scalar_batch, top2_margin
from tests.test_huber_host import np_double_per_target, np_huber
from tests.test_mdqn_host import np_mdqn_target
from tests.test_oracle_qnet import tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
GAMMA = 0.99
G3 = 0.99 * 0.99 * 0.99
SMALL_MAX = 255                       # the largest batch of the fused small-batch loss (a slice of >= 256 states takes loss_head_*)
SHAPES = [(128, 1, False), (512, 2, False), (384, 3, True), (128, 8, False)]
BATCHES = [1, 32, SMALL_MAX, 256]
OLDER = ("dqn", "nature", "double", "per", "mdqn", "mdqnper")
WEIGHTED = ("per", "mdqnper", "doubleper")
# (algo, Huber on): Huber with every scalar algo; doubleper with the squared loss as well
CASES = [(algo, True) for algo in OLDER + ("doubleper",)] + [("doubleper", False)]
AUTOGRAD = [(fc, A, dueling, B, algo, hub) for fc, A, dueling in SHAPES for B in BATCHES for algo, hub in CASES]      # (the cases of one (shape, B) follow each other: one forward)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


_nets = {}
_fwd = {}


def scalar_net(oracle, fc, A, dueling):
    """one net per shape for the gradient-exporting cases (they leave it as it was, delta = 0 included)"""
    key = (fc, A, dueling)
    if key not in _nets:
        _nets[key] = make_scalar(oracle, fc, A, dueling, 256)
    return _nets[key]


def draw_batch(oracle, cfg, p_on, torch, fc, A, dueling, B):
    """tests/test_gpu_shapes.py::test_scalar_train_step's draw (at B <= 32 whole batches are rejected until the oracle's ReLU / pool margin
    clears 2e-5), with importance weights, terminals from B = 32 on, and the online net's two best q(s', .) more than Q_ATOL apart"""
    small = B <= 32
    P = torch.from_numpy(p_on.astype(np.float64))
    for attempt in range(60):
        rng = np.random.default_rng(zlib.crc32(f"huber-{fc}-{A}-{dueling}-{B}-{attempt}".encode()))
        bt = scalar_batch(rng, B, A, "per")
        if B >= 32 and not (bt[4].any() and not bt[4].all()):
            continue
        with torch.no_grad():
            q_on_s2 = torch_forward(P, torch.from_numpy(bt[3]).double(), fc, A, dueling).numpy()
        if not (top2_margin(q_on_s2) > Q_ATOL).all():
            continue
        if small:
            oracle.forward(p_on, cfg, bt[0])
            if not oracle.last_margin() > 2e-5:
                continue
        return bt, small, q_on_s2
    pytest.fail("no minibatch found")


def forward_once(torch, oracle, fc, A, dueling, B):
    """the float64 forward of the four slices, computed once per (shape, B) and shared by that shape's cases"""
    key = (fc, A, dueling, B)
    if key not in _fwd:
        _fwd.clear()                                             # (the cases of one key follow each other: keep one graph)
        net, cfg, p_on, p_tg = scalar_net(oracle, fc, A, dueling)
        bt, small, q_on_s2 = draw_batch(oracle, cfg, p_on, torch, fc, A, dueling, B)
        s, a, r, s2, t, isw = bt
        P = torch.from_numpy(p_on.astype(np.float64)).requires_grad_(True)
        T = torch.from_numpy(p_tg.astype(np.float64))
        S, S2 = torch.from_numpy(s).double(), torch.from_numpy(s2).double()
        q = torch_forward(P, S, fc, A, dueling)
        with torch.no_grad():
            q_tg_s, q_tg_s2 = torch_forward(T, S, fc, A, dueling).numpy(), torch_forward(T, S2, fc, A, dueling).numpy()
        qa = q[torch.arange(B), torch.from_numpy(a.astype(np.int64))]
        _fwd[key] = dict(bt=bt, small=small, P=P, qa=qa, q_on_s2=q_on_s2, q_tg_s=q_tg_s, q_tg_s2=q_tg_s2)
    return _fwd[key]


def np_target(algo, F, G):
    """y of every scalar algo in float64 (the reward 0.1f read as 0.1), rounded to float32 as the kernels hand it on"""
    s, a, r, s2, t, isw = F["bt"]
    R = np.where(r == np.float32(0.1), 0.1, r.astype(np.float64))
    if algo in ("mdqn", "mdqnper"):
        y = np_mdqn_target(F["q_tg_s"], F["q_tg_s2"], a, R, t, G)[0]
    elif algo in ("double", "doubleper"):
        y = np_double_per_target(F["q_on_s2"], F["q_tg_s2"], R, t, G)[0]
    else:
        boot = (F["q_on_s2"] if algo == "dqn" else F["q_tg_s2"]).max(1)
        y = R + np.where(t != 0, 0.0, G * boot)
    return np.float32(y).astype(np.float64)


def autograd_case(torch, F, algo, G, delta_of):
    """-> (delta, y, loss, |d|, flat gradient) in float64; delta_of(|d|) picks the threshold from the reference's own |d|"""
    isw = F["bt"][5]
    y = np_target(algo, F, G)
    d = torch.from_numpy(y) - F["qa"]
    absd = d.detach().abs().numpy()
    delta = float(np.float32(delta_of(absd)))
    w = torch.from_numpy(isw.astype(np.float64)) if algo in WEIGHTED else torch.ones(len(y), dtype=torch.float64)
    ad = d.abs()
    terms = d * d if delta == 0 else torch.where(ad <= delta, d * d, delta * (2.0 * ad - delta))
    assert np.allclose(terms.detach().numpy(), np_huber(d.detach().numpy(), delta), rtol=1e-15, atol=0)
    loss = (w * terms).sum() if algo == "dqn" else (w * terms).mean()
    g, = torch.autograd.grad(loss, F["P"], retain_graph=True)
    return delta, y, loss.item(), absd, g.numpy()


# ================================================================================================================ against float64 autograd
@pytest.mark.parametrize("fc,A,dueling,B,algo,hub", AUTOGRAD)
def test_train_step_matches_autograd(torch_cuda, oracle, fc, A, dueling, B, algo, hub):
    """loss, y, |err| (unclipped) and every gradient tensor, at n = 1 (gamma) and with Gamma = gamma^3.  delta is the median of the
    reference's own |d|, so at least a quarter of the samples lie on each side (asserted from B = 32 on); at B = 1 the one sample is put
    outside the zone (delta = |d| / 2) and inside it (2 |d|) in turn.  The Huber gradient is continuous in d: no sample is masked."""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, fc, A, dueling)
    F = forward_once(torch, oracle, fc, A, dueling, B)
    s, a, r, s2, t, isw = F["bt"]
    if B >= 32:
        assert t.any() and not t.all()
    if algo in ("double", "doubleper"):
        assert (top2_margin(F["q_on_s2"]) > Q_ATOL).all()
    d_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    args = (d_(s), d_(a), d_(r), d_(s2), d_(t))
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    picks = [lambda ad: 0.0] if not hub else ([np.median] if B > 1 else [lambda ad: 0.5 * ad[0], lambda ad: 2.0 * ad[0]])
    try:
        for G in (GAMMA, G3):
            for pick in picks:
                delta, y0, loss0, ae0, g0 = autograd_case(torch, F, algo, G, pick)
                if hub and B >= 32:
                    assert (ae0 <= delta).mean() >= 0.25 and (ae0 > delta).mean() >= 0.25, ((ae0 <= delta).mean(), delta)
                if hub and B == 1:
                    assert (ae0[0] > delta) == (pick is picks[0])
                net.set_huber(delta)
                assert net.huber() == np.float32(delta)
                loss, ae, y = net.train_step(algo, *args, isw=d_(isw) if algo in WEIGHTED else None, gamma=G, flat_grad=grad)
                y, ae, loss, g = y.cpu().numpy(), ae.cpu().numpy(), loss.item(), grad.cpu().numpy()
                print(f"huber ({fc}, {A}, {arch_of(dueling)}) {algo} B={B} Gamma={G:.4f} delta={delta:.4g}: inside {(ae0 <= delta).mean() if delta else 1:.2f}  "
                      f"max|y - y0| {np.abs(y - y0).max():.2e}  max|ae - ae0| {np.abs(ae - ae0).max():.2e}  loss {loss:.6g} / {loss0:.6g}")
                np.testing.assert_allclose(y, y0, rtol=0, atol=Q_ATOL)
                np.testing.assert_allclose(ae, ae0, rtol=0, atol=2 * Q_ATOL)
                np.testing.assert_allclose(loss, loss0, rtol=1e-4, atol=1e-6)
                check_scalar_grads(g, g0, fc, A, dueling, F["small"])
    finally:
        net.set_huber(0.0)
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)          # gradient-only mode


# ================================================================================================================ exact heads
def seq32(terms, B):
    """the loss as both bodies form it: the B terms added in float32 in sample order, then divided by B"""
    acc = np.float32(0)
    for x in np.asarray(terms, np.float32):
        acc = np.float32(acc + x)
    return np.float32(acc / np.float32(B))


@pytest.mark.parametrize("B", [4, 256])
def test_exact_hand_case_and_the_junction(torch_cuda, B):
    """zero head weights, chosen biases (tests/test_gpu_exact_heads.py): Q, y and d are exact floats, and so is every sum below (small
    multiples of 2^-6; 2 / B is a power of two), so everything is compared with equality -- the one loss whose partial sums round (terms
    1 + 2^-22) against the same float32 additions in sample order (seq32).  The target net's Q is (1, 1),
    Gamma = 0.5: y = r + 0.5 (r on a terminal sample)."""
    torch = torch_cuda
    net, ps = exact_net("plain", 2, 256)
    rng = np.random.default_rng(B)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = (np.arange(B) % 2).astype(np.uint8)
    t = (np.arange(B) % 4 == 3).astype(np.uint8)                 # (terminal samples among those of action 1)
    assert t.any() and not t.all()
    net.load_params(with_head(ps[1], 512, 2, "plain", 0, np.float32([1.0, 1.0])), 1)
    names = {name: (lo, hi) for name, lo, hi in tensor_bounds(512, 2, "plain")}

    def step(algo, on, r, delta, w=None):
        net.load_params(with_head(ps[0], 512, 2, "plain", 0, np.float32(on)), 0)
        net.set_huber(delta)
        d_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        grad = torch.zeros(net.n_params, device="cuda")
        loss, ae, y = net.train_step(algo, d_(s), d_(a), d_(r), d_(s2), d_(t), isw=None if w is None else d_(w), gamma=0.5, flat_grad=grad)
        lo, hi = names["b_q"]
        return np.float32(loss.item()), ae.cpu().numpy(), y.cpu().numpy(), grad.cpu().numpy()[lo:hi]

    try:
        # the header's worked case: delta 1, d = 0.5 on action 0's samples (y = 1, q = 0.5), d = -3 on action 1's (y = -4, q = -1)
        r = np.where(a == 0, 0.5, np.where(t != 0, -4.0, -4.5)).astype(np.float32)
        for algo in ("nature", "double", "per", "doubleper"):
            w = np.ones(B, np.float32) if algo in WEIGHTED else None
            loss, ae, y, gb = step(algo, [0.5, -1.0], r, 1.0, w)
            assert np.array_equal(y, np.where(a == 0, 1.0, -4.0).astype(np.float32)), algo
            assert np.array_equal(ae, np.where(a == 0, 0.5, 3.0).astype(np.float32)), algo        # |d|, not clipped
            assert loss == np.float32(2.625) and np.array_equal(gb, np.float32([-0.5, 1.0])), (algo, loss, gb)
        loss, ae, y, gb = step("dqn", [0.5, -1.0], r, 1.0)           # the sum: B x 2.625, scale 2 (FB_ALGO_DQN bootstraps from the ONLINE net)
        d0 = y.astype(np.float64) - np.where(a == 0, 0.5, -1.0)
        assert loss == np.float32(np_huber(d0, 1.0).sum()) and np.array_equal(ae, np.abs(d0).astype(np.float32))
        assert np.array_equal(gb, np.float32([(-2.0 * np.clip(d0, -1, 1))[a == k].sum() for k in (0, 1)]))
        # the squared loss on the same minibatch, for contrast: (0.25 + 9) / 2, gradient (-0.5, +3)
        loss, ae, y, gb = step("nature", [0.5, -1.0], r, 0.0)
        assert loss == np.float32(4.625) and np.array_equal(gb, np.float32([-0.5, 3.0]))
        # d = +-delta exactly (y = 0, q = -+1): the quadratic branch; terms 1, gradient -+1
        r0 = np.where(t != 0, 0.0, -0.5).astype(np.float32)
        loss, ae, y, gb = step("nature", [-1.0, 1.0], r0, 1.0)
        assert not y.any() and np.array_equal(ae, np.ones(B, np.float32)) and loss == np.float32(1.0) and np.array_equal(gb, np.float32([-1.0, 1.0]))
        # the next float above delta: the linear branch; delta (2 |d| - delta) = 1 + 2^-22, the gradient stays -+1 (unclipped: -+(1 + 2^-23))
        up = np.nextafter(np.float32(1.0), np.float32(2.0))
        loss, ae, y, gb = step("nature", [-up, up], r0, 1.0)
        assert np.array_equal(ae, np.full(B, up, np.float32)) and loss == seq32(np.full(B, 1.0 + 2.0 ** -22), B) and np.array_equal(gb, np.float32([-1.0, 1.0]))
        loss, ae, y, gb = step("nature", [-up, up], r0, 0.0)
        assert np.array_equal(gb, np.float32([-up, up]))                                              # (what the squared loss gives there)
        # delta = 3: d = -3 sits on the junction, the whole case is the squared loss's
        loss, ae, y, gb = step("per", [0.5, -1.0], r, 3.0, np.ones(B, np.float32))
        assert loss == np.float32(4.625) and np.array_equal(gb, np.float32([-0.5, 3.0]))
        # importance weights 1, 0.5, 0.25 (exact): w l(d) and w clamp(d)
        w = np.float32([1.0, 0.5, 0.25])[np.arange(B) % 3]
        loss, ae, y, gb = step("doubleper", [0.5, -1.0], r, 1.0, w)
        d0 = np.where(a == 0, 0.5, -3.0)
        assert loss == np.float32((w * np_huber(d0, 1.0)).sum() / B)
        assert np.array_equal(gb, np.float32([(-2.0 / B * w * np.clip(d0, -1, 1))[a == k].sum() for k in (0, 1)]))
    finally:
        net.set_huber(0.0)


@pytest.mark.parametrize("B", [4, 256])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_double_per_takes_the_first_maximum_on_exact_ties(torch_cuda, A, B):
    """a tied online net, a target net that differs per action: a* is np.argmax's, y = r + Gamma q-(s', a*) exactly; with w = 1 everything
    equals FB_ALGO_DOUBLE's bit for bit"""
    torch = torch_cuda
    net, ps = exact_net("plain", A, 256)
    s, a, r, s2, t, w = exact_batch(B, A, 3)
    tg = np.float32([2 * c + 1 for c in range(A)])
    net.load_params(with_head(ps[1], 512, A, "plain", 0, tg), 1)
    d_ = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    args = (d_(s), d_(a), d_(r), d_(s2), d_(t))
    for lv in tie_patterns(A):
        net.load_params(with_head(ps[0], 512, A, "plain", 0, np.float32(lv)), 0)
        want = r + np.where(t != 0, np.float32(0), np.float32(0.5) * tg[int(np.argmax(lv))])
        out = {}
        for algo, ww in (("double", None), ("doubleper", np.ones(B, np.float32)), ("doubleper", w)):
            grad = torch.zeros(net.n_params, device="cuda")
            loss, ae, y = net.train_step(algo, *args, isw=None if ww is None else d_(ww), gamma=0.5, flat_grad=grad)
            assert np.array_equal(y.cpu().numpy(), want.astype(np.float32)), (lv, algo)
            assert np.array_equal(ae.cpu().numpy(), np.abs(want - np.float32(lv)[a]).astype(np.float32)), (lv, algo)
            out[(algo, ww is w)] = (loss.clone(), ae.clone(), y.clone(), grad)
        for x, z in zip(out[("double", False)], out[("doubleper", False)]):
            assert torch.equal(x, z), lv


# ================================================================================================================ bit for bit
def _step(torch, net, algo, args, isw=None, gamma=GAMMA):
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, ae, y = net.train_step(algo, *args, isw=isw, gamma=gamma, flat_grad=grad)
    return loss.clone(), y.clone(), ae.clone(), grad


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", OLDER)
def test_a_huge_delta_is_the_squared_loss_bit_for_bit(torch_cuda, oracle, algo, B):
    """delta = 1e30 (the extended kernels) against delta = 0 (the kernels of before the setting): loss, y, |err|, flat gradient; and after
    set_huber(x), set_huber(0) the step is the untouched net's"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 384, 3, True)
    s, a, r, s2, t, isw = scalar_batch(np.random.default_rng(B), B, 3, "per")
    d_ = lambda x: torch.from_numpy(x).cuda()
    args, w = (d_(s), d_(a), d_(r), d_(s2), d_(t)), (d_(isw) if algo in WEIGHTED else None)
    off = _step(torch, net, algo, args, w)
    try:
        net.set_huber(1e30)
        huge = _step(torch, net, algo, args, w)
        net.set_huber(0.5)
        half = _step(torch, net, algo, args, w)
    finally:
        net.set_huber(0.0)
    again = _step(torch, net, algo, args, w)
    for x, z, v in zip(off, huge, again):
        assert torch.equal(x, z) and torch.equal(x, v)
    assert torch.equal(off[1], half[1]) and torch.equal(off[2], half[2])             # y and |err| do not depend on delta
    assert not torch.equal(off[3], half[3]) and half[0].item() < off[0].item() and off[3].abs().max() > 0


@pytest.mark.parametrize("B", [32, SMALL_MAX, 256])
@pytest.mark.parametrize("delta", [0.0, 0.75])
def test_double_per_anchors_bit_for_bit(torch_cuda, oracle, B, delta):
    """isw == 1: loss, y and gradient are FB_ALGO_DOUBLE's; one action: everything is FB_ALGO_PER's"""
    torch = torch_cuda
    d_ = lambda x: torch.from_numpy(x).cuda()
    net, cfg, p_on, p_tg = scalar_net(oracle, 384, 3, True)
    s, a, r, s2, t, isw = scalar_batch(np.random.default_rng(B), B, 3, "per")
    args = (d_(s), d_(a), d_(r), d_(s2), d_(t))
    one_net = scalar_net(oracle, 128, 1, False)[0]
    s1, a1, r1, s21, t1, isw1 = scalar_batch(np.random.default_rng(B + 1), B, 1, "per")
    args1 = (d_(s1), d_(a1), d_(r1), d_(s21), d_(t1))
    try:
        net.set_huber(delta); one_net.set_huber(delta)
        dbl = _step(torch, net, "double", args)
        dper = _step(torch, net, "doubleper", args, torch.ones(B, device="cuda"))
        wtd = _step(torch, net, "doubleper", args, d_(isw))
        per1 = _step(torch, one_net, "per", args1, d_(isw1))
        dper1 = _step(torch, one_net, "doubleper", args1, d_(isw1))
    finally:
        net.set_huber(0.0); one_net.set_huber(0.0)
    for x, z in zip(dbl, dper):
        assert torch.equal(x, z)
    assert torch.equal(dbl[1], wtd[1]) and torch.equal(dbl[2], wtd[2]) and not torch.equal(dbl[3], wtd[3])
    for x, z in zip(per1, dper1):
        assert torch.equal(x, z)
    assert dper1[3].abs().max() > 0


# ================================================================================================================ composition
@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ["double", "doubleper"])
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, algo, B):
    torch = torch_cuda
    nets = [_net("dueling"), _net("dueling")]
    s, a, r, s2, t, isw = scalar_batch(np.random.default_rng(B), B, 2, "per")
    d_ = lambda x: torch.from_numpy(x).cuda()
    args, w = (d_(s), d_(a), d_(r), d_(s2), d_(t)), (d_(isw) if algo in WEIGHTED else None)
    grad = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    ae = nets[0].train_step(algo, *args, isw=w, flat_grad=grad)[1].cpu().numpy()      # (gradient-only: the net stays as it was)
    delta = float(np.median(ae))                                 # the clip acts on half of this minibatch's first step
    assert (ae <= delta).mean() >= 0.25 and (ae > delta).mean() >= 0.25
    for n in nets:
        n.set_huber(delta)
    before = nets[0].store_params().clone()
    for _ in range(2):
        l0 = nets[0].train_step(algo, *args, isw=w, flat_grad=grad)[0].clone()
        nets[0].apply_adam(grad)
        l1 = nets[1].train_step(algo, *args, isw=w)[0]
        assert torch.equal(l0, l1)
    assert torch.equal(nets[0].store_params(), nets[1].store_params()) and not torch.equal(nets[0].store_params(), before)
    (m0, v0, p0), (m1, v1, p1) = nets[0].adam_state(), nets[1].adam_state()
    assert torch.equal(m0, m1) and torch.equal(v0, v1) and np.array_equal(p0, p1)
    assert torch.equal(nets[0].store_params(1), nets[1].store_params(1))


@pytest.mark.parametrize("n", [1, 3])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, n):
    """bit for bit below B = 256; at 256 the separate calls run the large-batch trunk (another summation order in conv2 / conv3): equal to
    rounding, for every algo -- the allowance of tests/test_gpu_shims.py::test_train_from_replay_equals_gather_plus_train_step"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(64, 4000, 40, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (32, SMALL_MAX, 256):
        same = torch.equal if B < 256 else (lambda x, y: torch.allclose(x, y, rtol=2e-4, atol=2e-6))
        n1, n2 = _net(), _net()
        n1.set_huber(0.5); n2.set_huber(0.5)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(2):
            idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, _, _ = n1.train_step("double", s, a, r, s2, t, gamma=G, flat_grad=g1 if exp else None, want_aux=False)
            l2, a2, r2, t2 = train_from_replay(rep, n2, "double", idx, gamma=GAMMA, flat_grad=g2 if exp else None)
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
        net.set_huber(0.5)
        return rep, net, TrainSteps(rep, net, B, "nature", GAMMA)

    (r1, n1, _), (r2, n2, ts2) = make(), make()
    plain = _net()
    before = n1.store_params().clone()
    for _ in range(5):
        idx, _ = r1.sample(B)
        train_from_replay(r1, n1, "nature", idx, gamma=GAMMA)
    ts2(5)
    assert torch.equal(n1.store_params(), n2.store_params()) and not torch.equal(n1.store_params(), before)
    r3 = make()[0]
    for _ in range(5):                                               # (and the clip acts: the squared loss ends elsewhere)
        idx, _ = r3.sample(B)
        train_from_replay(r3, plain, "nature", idx, gamma=GAMMA)
    assert not torch.equal(plain.store_params(), n1.store_params())


@pytest.mark.parametrize("delta", [0.0, 0.5])
def test_prioritized_n_step_vec_step_equals_composed_calls(torch_cuda, delta):
    """doubleper on a prioritized n = 3 memory, 256 envs (ring-fed, the tree work ahead on the memory's side stream), B = 32: actions,
    indices, weights, loss and |err| at every step, the nets, the envs and the memory's bytes at the end"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    N, B, steps = 256, 32, 30
    (e1, r1, n1, nib1), (e2, r2, n2, _) = _pipeline(N, B, 3, True, "dueling"), _pipeline(N, B, 3, True, "dueling")
    n1.set_huber(delta); n2.set_huber(delta)
    one = VecStep(e2, r2, n2, B, "doubleper", GAMMA)
    p0 = n1.store_params().clone()
    for step in range(steps):
        train = step >= 4
        if train and step % 8 == 0:
            n1.sync_target(); n2.sync_target()
        a1 = n1.act_nib(nib1, 0.05, seed=1, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
            loss, _, _, _, ae = train_from_replay(r1, n1, "doubleper", idx, gamma=GAMMA, isw=isw, want_abs_err=True)
            r1.update_priorities(idx, abs_err=ae)
        a2 = one(0.05, seed=1, step=step, train=train)
        assert torch.equal(a1, a2), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(isw, one.isw), step
            assert torch.equal(loss, one.loss) and torch.equal(ae, one.abs_err + 0.01), step
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(n1.store_params(), n2.store_params())
    assert not torch.equal(n1.store_params(), p0) and torch.equal(n1.store_params(1), n2.store_params(1))
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))


def test_split_schedule_equals_one_stream(torch_cuda):
    """dqn + Huber at 1024 envs, B = 32: the split schedule (fc1_bwd2_x_kernel carries the gate workgroup) against one stream, as
    tests/test_gpu_shims.py::test_split_schedule_equals_one_stream_over_many_steps; no wait between the streams gave up"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
    N, B, steps = 1024, 32, 60

    def make():
        env, rep, net = VecGameState(N, seed=11), VecReplay(60000, N), QNet(max_batch=max(N, B))
        rep.seed(4, "cpython"); net.init_params(5, which=0); net.init_params(6, which=1)
        net.set_huber(0.5)
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib, VecStep(env, rep, net, B, "dqn")

    e1, r1, n1, nib1, one = make()
    e2, r2, n2, nib2, two = make()
    try:
        for step in range(steps):
            train = step >= 4 and step % 9 != 5
            L.check(L.lib().fb_vec_step_set_schedule(0), "schedule")
            a1 = one(0.05, seed=2, step=step, train=train).clone()
            L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
            a2 = two(0.05, seed=2, step=step, train=train)
            assert torch.equal(a1, a2), step
            if train:
                assert torch.equal(one.idx, two.idx) and torch.equal(one.loss, two.loss), step
    finally:
        L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
    assert (e1.get_state() == e2.get_state()).all() and torch.equal(nib1, nib2)
    assert torch.equal(n1.store_params(), n2.store_params())
    (m1, v1, p1), (m2, v2, p2) = n1.adam_state(), n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)
    assert np.array_equal(r1.state_blob(), r2.state_blob())
    assert n1.split_stats() == (0, 0)
    issued, clean = n2.split_stats()                      # (raises if a wait between the two streams gave up)
    assert issued == sum(1 for k in range(steps) if k >= 4 and k % 9 != 5), (issued, clean)


def test_vec_step_dp_world1_equals_vec_step(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.dist import NativeDP
    from dqnflappybird_amd.vec import VecStep
    N, B, steps = 256, 32, 14
    nd = NativeDP(rank=0, world=1, overlap=False)
    try:
        (e1, r1, n1, _), (e2, r2, n2, _) = _pipeline(N, B, 1), _pipeline(N, B, 1)
        n1.set_huber(0.5); n2.set_huber(0.5)
        g2 = torch.zeros(n2.n_params, device="cuda")
        fused, dp = VecStep(e1, r1, n1, B, "nature", GAMMA), VecStep(e2, r2, n2, B, "nature", GAMMA, flat_grad=g2, dist=nd)
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


# ================================================================================================================ bf16 training
@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo,hub", [("double", True), ("doubleper", False), ("doubleper", True)])
def test_bf16_train_dtype(torch_cuda, oracle, algo, hub, B):
    """bf16 operands against the fp32 device result, within tests/test_gpu_configs.py's bounds, on the net and the minibatch those bounds
    were set on; back in f32 the step is bit-identical.  With Huber on, delta is the median of the minibatch's own fp32 |d| (which does
    not depend on delta), so that at least a quarter of the samples lie on each side of the clip: asserted"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = scalar_net(oracle, 512, 2, False)
    rng = np.random.default_rng(B)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = rng.integers(0, 2, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    t = (r == -3).astype(np.uint8)
    d_ = lambda x: torch.from_numpy(x).cuda()
    args = (d_(s), d_(a), d_(r), d_(s2), d_(t))
    w = torch.ones(B, device="cuda") if algo in WEIGHTED else None
    delta = 0.0
    if hub:
        ae = _step(torch, net, algo, args, w)[2].cpu().numpy()
        delta = float(np.median(ae))
        assert (ae <= delta).mean() >= 0.25 and (ae > delta).mean() >= 0.25
    try:
        net.set_huber(delta)
        f32 = _step(torch, net, algo, args, w)
        net.set_train_dtype("bf16")
        try:
            bf = _step(torch, net, algo, args, w)
        finally:
            net.set_train_dtype("f32")
        again = _step(torch, net, algo, args, w)
    finally:
        net.set_huber(0.0)
    assert all(torch.equal(x, z) for x, z in zip(f32, again))
    y32, ybf = f32[1].cpu().numpy(), bf[1].cpu().numpy()
    assert not np.array_equal(y32, ybf)
    assert np.abs(ybf - y32).max() < BF16_Q_REL * np.abs(y32).max()
    g32, gbf = f32[3].cpu().numpy(), bf[3].cpu().numpy()
    errs = {name: np.linalg.norm(gbf[lo:hi] - g32[lo:hi]) / np.linalg.norm(g32[lo:hi]) for name, lo, hi in tensor_bounds(512, 2, "plain")}
    print(f"bf16 B={B} {algo} delta={delta:.4g}: max|y_bf16 - y_f32| / max|y| {np.abs(ybf - y32).max() / np.abs(y32).max():.4f}  per-tensor gradient error "
          + "  ".join(f"{k} {v:.4f}" for k, v in errs.items()))
    for name, err in errs.items():
        assert 0 < err < BF16_GRAD_REL, (name, err)


# ================================================================================================================ setter and refusals
def snapshot(net, rep=None):
    m, v, pows = net.adam_state()
    out = [net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), pows.copy(), net.huber()]
    if rep is not None:
        out.append(np.asarray(rep.state_blob()).copy())
    return out


def same(x, y):
    import torch
    return all(torch.equal(p, q) if torch.is_tensor(p) else np.array_equal(p, q) for p, q in zip(x, y))


def test_setter_and_refusals_change_nothing(torch_cuda):
    """every FB_ERR_INVALID of the header's section; afterwards the parameters, the Adam slots and step counter (its beta powers), delta
    and the memories' bytes (push counter, tree, generator) are what they were"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, TrainSteps, VecStep, train_from_replay
    net = _net()
    lib = L.lib()
    assert net.huber() == 0.0                                          # a new scalar net: off
    net.set_huber(0.25)
    assert net.huber() == 0.25
    before = snapshot(net)
    for bad in (float("nan"), float("inf"), -float("inf"), -1.0, -1e-30):
        assert lib.fb_qnet_set_huber(net.h, bad) == -1, bad
        assert "fb_qnet_set_huber" in lib.fb_last_error().decode()
        with pytest.raises(ValueError, match="delta must be finite and >= 0"):
            net.set_huber(bad)
        assert same(before, snapshot(net)), bad
    s, a, r, s2, t, _ = scalar_batch(np.random.default_rng(1), 32, 2, "nature")
    d_ = lambda x: torch.from_numpy(x).cuda()
    args = (d_(s), d_(a), d_(r), d_(s2), d_(t))
    w = torch.ones(32, device="cuda")
    # the setter, the getter and the algo on C51 / QR / noisy nets
    for kw in (dict(arch="c51"), dict(arch="qr"), dict(arch="c51dueling", noisy=True)):
        other = QNet(2, 512, max_batch=32, **kw)
        other.init_params(1, 0); other.init_params(2, 1)
        with pytest.raises(ValueError, match="scalar heads only"):
            other.set_huber(1.0)
        with pytest.raises(ValueError, match="scalar heads only"):
            other.huber()
        p0 = other.store_params().clone()
        with pytest.raises(ValueError, match="net trains with"):
            other.train_step("doubleper", *args, isw=w)
        assert torch.equal(p0, other.store_params())
    # FB_ALGO_PG on a net whose delta is > 0 (accepted again at 0)
    with pytest.raises(ValueError, match="FB_ALGO_PG has no TD error to clip"):
        net.train_step("pg", *args, gamma=32.0, flat_grad=torch.zeros(net.n_params, device="cuda"))
    with pytest.raises(ValueError, match="PER needs isw"):
        net.train_step("doubleper", *args)
    assert lib.fb_qnet_train_step(net.h, 13, 32, *(L.ptr(x) for x in args[:2]), L.ptr(args[2]), L.ptr(args[3]), L.ptr(args[4]), None, C.c_double(GAMMA),
                                  L.ptr(w), None, None, None, L.current_stream()) == -1 and "unknown algo 13" in lib.fb_last_error().decode()
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
    with pytest.raises(ValueError, match="FB_ALGO_DOUBLE_PER trains from a prioritized memory only"):
        train_from_replay(uni, net, "doubleper", idx, gamma=GAMMA, isw=w)
    with pytest.raises(ValueError, match="importance weights"):
        train_from_replay(per, net, "doubleper", pidx, gamma=GAMMA)
    rc = lib.fb_train_from_replay(per.h, net.h, L.ALGO_DOUBLE_PER, 32, L.ptr(pidx), None, L.ptr(args[1]), L.ptr(args[2]), L.ptr(args[4]),
                                  C.c_double(GAMMA), L.ptr(w), None, None, L.current_stream())
    assert rc == -1 and "importance weights" in lib.fb_last_error().decode()
    rc = lib.fb_train_from_replay(per.h, net.h, 13, 32, L.ptr(pidx), L.ptr(w), L.ptr(args[1]), L.ptr(args[2]), L.ptr(args[4]),
                                  C.c_double(GAMMA), L.ptr(w), None, None, L.current_stream())
    assert rc == -1 and "unknown algo 13" in lib.fb_last_error().decode()
    with pytest.raises(ValueError, match="TrainSteps is for uniform replay"):
        TrainSteps(uni, net, 32, "doubleper", GAMMA)
    ts = TrainSteps(uni, net, 32, "nature", GAMMA)
    ts.algo = L.ALGO_DOUBLE_PER                                        # (past the Python check: the library's own refusal)
    with pytest.raises(ValueError, match="prioritized replay needs the importance weights"):
        ts(1)
    loss = torch.zeros(1, device="cuda")
    rc = lib.fb_profile_ring_kernel(per.h, net.h, 0, 1, L.ALGO_DOUBLE_PER, 32, L.ptr(pidx), L.ptr(args[1]), L.ptr(args[2]), L.ptr(args[4]), L.ptr(loss),
                                    L.current_stream())
    assert rc == -1 and "uniform memories only" in lib.fb_last_error().decode()
    env_u = played(32, 4000, 1, seed=6)[0]
    env_u.track_state()
    with pytest.raises(ValueError, match="go with a prioritized memory"):
        VecStep(env_u, uni, net, 32, "doubleper", GAMMA)
    with pytest.raises(ValueError, match="go with a prioritized memory"):
        VecStep(env_u, per, net, 32, "double", GAMMA)
    one = VecStep(env_u, uni, net, 32, "nature", GAMMA)
    one.algo = L.ALGO_DOUBLE_PER                                       # (past the Python check again: a step without isw buffers)
    with pytest.raises(ValueError, match="needs the isw / isw32 / abs_err buffers"):
        one(0.05, seed=1, step=0)
    two = VecStep(env_u, per, net, 32, "per", GAMMA)                   # (a step WITH the prioritized buffers, then a uniform memory under it)
    two.replay, two.algo = uni, L.ALGO_DOUBLE_PER
    with pytest.raises(ValueError, match="fb_vec_step: FB_ALGO_DOUBLE_PER trains from a prioritized memory only"):
        two(0.05, seed=1, step=0)
    torch.cuda.synchronize()
    assert same(before_u, snapshot(net, uni)) and same(before_p, snapshot(net, per))
    assert net.huber() == 0.25


# ================================================================================================================ end to end
def test_vecbrain_end_to_end(torch_cuda, tmp_path):
    """VecBrain(algo='doubleper', arch='dueling', n_step=3, huber=1.0) at 64 envs: a few hundred steps, save / load continues bit for bit
    and records delta, a brain with another delta refuses the checkpoint by name"""
    torch = torch_cuda
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="doubleper", arch="dueling", batch=32, capacity=20000, observe=20, seed=3, replace_target_iter=50, n_step=3, huber=1.0)
    a = VecBrain(64, **kw)
    assert a.net.huber() == a.huber == 1.0
    a.net.set_hparams(lr=1e-4)
    p0, t0 = a.net.store_params().clone(), a.net.store_params(1).clone()
    a.run(200, log_every=0)
    assert np.isfinite(a.last_loss.item()) and not torch.equal(p0, a.net.store_params())
    assert not torch.equal(t0, a.net.store_params(1))                  # the target net syncs, as for 'double'
    ck = str(tmp_path / "ck")
    a.save(ck)
    assert np.load(ck + ".npz")["huber"].tolist() == [1.0]
    b = VecBrain(64, **dict(kw, seed=77))
    b.net.set_hparams(lr=1e-4)
    b.load(ck)
    for _ in range(10):
        a.step(); b.step()
        assert torch.equal(a.one_step.actions, b.one_step.actions) and torch.equal(a.one_step.loss, b.one_step.loss)
    assert torch.equal(a.net.store_params(), b.net.store_params())
    with pytest.raises(ValueError, match="was trained with huber \\(delta\\) = 1.0, this VecBrain has huber = 0.5"):
        VecBrain(64, **dict(kw, huber=0.5)).load(ck)
    with pytest.raises(ValueError, match="was trained with huber \\(delta\\) = 1.0, this VecBrain has huber = 0.0"):
        VecBrain(64, **dict(kw, huber=0.0)).load(ck)
