"""Exact cases on the device.  A head whose weight matrix is all zero gives theta (or logits, or Q) that are its biases for every
state on every path (fmaf(x, 0, acc) leaves acc), and small integers and halves sum exactly in fp32 in any order, so these tests place
Q, theta and the targets T where they want them (tests/test_exact_heads_host.py builds the biases and checks their exactness on the
CPU) and assert what random data cannot reach:
  - np.argmax's FIRST maximum on bit-identical Q, in acting (act, act_nib small and fused trunk, fb_eval_q, fb_eval_run; the scalar
    plain and dueling heads, C51, dueling C51, noisy C51 with sigma = 0 under a shared sample and per-env noise, QR, dueling QR) and
    for a* in training (scalar double, c51double / c51doubleper, qrdouble / qrdoubleper with a tied online net and a target net that
    differs per action; qr / qrper with target rows of equal sums and different shapes), at A = 2 (the <2> instantiations) and A = 3,
    8 (<MAXA>), B < 256 and B = 256.  The reference is argmax, full stop: no device-chosen a*, no margin mask;
  - include/fbdqn.h's worked case of the quantile Huber loss, |u| = kappa on every pair with both signs, u = 0, terminal samples under
    a target net of huge biases, all on qr_loss_kernel itself;
  - integer ramps through forward_quantiles bit for bit, forward their exact mean, at N = 2 and N = 64."""
import numpy as np
import pytest

from tests.test_c51_host import np_project
from tests.test_exact_heads_host import (HEAD0, KINDS, N_DIST, arch_of, distinct_rows, expected_qr, fold32, layout, level_rows,
                                         shaped_rows, tie_patterns, with_head)
from tests.test_gpu_noisy_env import states
from tests.test_oracle_qnet import rand_states, tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
FC = 512
EPS32 = 2.0 ** -24


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def make_net(kind, A, max_batch, N=N_DIST, kappa=1.0):
    """-> (net, [online, target] flat vectors x 3, as the other tests scale a trunk so that its ReLUs switch)"""
    from dqnflappybird_amd.vec import QNet
    arch = arch_of(kind)
    kw = {}
    if "c51" in arch:
        kw = dict(n_atoms=N)
    elif arch.startswith("qr"):
        kw = dict(n_quantiles=N, kappa=kappa)
    if kind.startswith("noisy"):
        kw["noisy"] = True
    net = QNet(A, FC, arch, max_batch=max_batch, **kw)
    ps = []
    for which in (0, 1):
        net.init_params(3 + which, which)
        ps.append(net.store_params(which).cpu().numpy() * 3.0)
    return net, ps


def load(net, ps, kind, A, N, on, tg=None):
    """on / tg: (b, b_v) of the online / target net"""
    net.load_params(with_head(ps[0], FC, A, kind, N, *on), 0)
    if tg is not None:
        net.load_params(with_head(ps[1], FC, A, kind, N, *tg), 1)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def batch(B, A, seed):
    """states, every action in turn, rewards and a discount that are exact in fp32, terminal and bootstrapped samples"""
    rng = np.random.default_rng(seed)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = (np.arange(B) % A).astype(np.uint8)
    r = np.float32([0.5, 1.0, -1.0, 2.0, -0.5])[np.arange(B) % 5]
    t = (np.arange(B) % 7 == 3).astype(np.uint8)
    w = np.float32([1.0, 0.5, 0.25])[np.arange(B) % 3]
    if B >= 32:
        assert t.any() and not t.all() and len(set(a.tolist())) == A
    return s, a, r, s2, t, w


def head_grads(g, kind, A, N):
    """-> (the gradient of the head's [A, N] bias, of b_v or None, {name: slice} of every tensor)"""
    tb = {name: g[lo:hi] for name, lo, hi in tensor_bounds(FC, A, layout(kind), N)}
    gb = tb["b_adv"] if "b_adv" in tb else tb["b_head"]
    return gb.reshape(A, N), tb.get("b_v"), tb


def check_sum(got, want, absum, B, what, slack=0.0):
    """a sum of B fp32 terms, each exact or one rounding off (the division by B), formed in any order: within (B + 2) 2^-24 of the sum of
    the terms' magnitudes (slack: a relative allowance for terms that are not exact, said where it is used)"""
    bound = ((B + 2) * EPS32 + slack) * np.asarray(absum, np.float64)
    bad = np.abs(np.asarray(got, np.float64) - want) > bound
    assert not np.any(bad), (what, np.asarray(got)[bad][:4] if np.ndim(got) else got, np.asarray(want)[bad][:4] if np.ndim(want) else want)


# ================================================================================================================ acting
@pytest.mark.parametrize("A", [2, 3, 8])
@pytest.mark.parametrize("kind", KINDS)
def test_acting_takes_the_first_maximum(torch_cuda, kind, A):
    """bit-identical Q on two or on all actions: every acting path returns the lowest tied index on every row (a tie of 1 and 2 below
    action 0 leaves action 0; a tie of 1 and 2 above it gives 1), and the Q it returns is tied bit for bit, as constructed"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    net, ps = make_net(kind, A, 300)
    u8 = rand_states(np.random.default_rng(A), 300)
    xs = [torch.from_numpy(u8[:5]).cuda(), torch.from_numpy(u8).cuda()]
    nibs = [states(37)[0], states(300)[0]]
    for lv in tie_patterns(A):
        b, b_v = level_rows(kind, lv)
        load(net, ps, kind, A, N_DIST, (b, b_v))
        want = int(np.argmax(lv))
        first = [lv.index(x) for x in lv]                        # the first action of each action's level
        assert len(set(first)) < A and want == first[want]       # (a tie somewhere; at the top, or below action 0)

        def check(what, act, q):
            q = q.cpu().numpy()
            for a in range(A):
                assert np.array_equal(bits(q[:, a]), bits(q[:, first[a]])), (what, lv, a)
                assert lv[a] == lv[want] or (q[:, a] < q[:, want]).all(), (what, lv, a)
            if kind == "plain":
                assert np.array_equal(q, np.broadcast_to(np.float32(lv), q.shape)), (what, lv)
            if kind == "qr":
                assert np.array_equal(q, np.broadcast_to(np.float32(lv) - np.float32(0.5), q.shape)), (what, lv)
            if act is not None:
                assert np.array_equal(act.cpu().numpy(), np.full(len(q), want, np.uint8)), (what, lv)

        for x in xs:
            check(f"act B={len(x)}", *net.act(x, 0.0, seed=1, step=2, want_q=True))
        for nib in nibs:
            check(f"act_nib n={len(nib)}", *net.act_nib(nib, 0.0, seed=1, step=2, want_q=True))
        q = torch.empty((300, A), dtype=torch.float32, device="cuda")
        L.check(L.lib().fb_eval_q(net.h, L.ptr(nibs[1]), 300, L.ptr(q), L.current_stream()), "fb_eval_q")
        check("fb_eval_q", None, q)
        if kind.startswith("noisy"):                            # sigma = 0: a noise sample leaves mu's biases where they are
            net.reset_noise(0, seed=5, step=7)
            assert net.noise(0).abs().max().item() > 0
            for nib in nibs:
                check(f"shared sample n={len(nib)}", *net.act_nib(nib, 0.0, seed=1, step=2, want_q=True))
                check(f"per-env noise n={len(nib)}", *net.act_nib_env_noise(nib, 0.0, seed=9, step=4, want_q=True))
            net.mean_noise(0)


def const_play(n, action, env_seed, cap=3000):
    """(length, score) of the first episode of each of n fresh games under one constant action (0 where the cap came first)"""
    import torch
    from dqnflappybird_amd.vec import VecGameState
    env = VecGameState(n, seed=env_seed)
    env.track_state(); env.observe()
    acts = torch.full((n,), action, dtype=torch.uint8, device="cuda")
    length, score, cur, done = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, bool)
    for _ in range(cap):
        _, _, term, sc = env.frame_step(acts, want_u8=False)
        term, sc = term.cpu().numpy().astype(bool), sc.cpu().numpy()
        cur[~done] += 1
        end = ~done & term
        length[end], score[end] = cur[end], sc[end]
        done |= end
        if done.all():
            break
    return length, score


@pytest.mark.parametrize("kind", KINDS)
def test_eval_run_takes_the_first_maximum(torch_cuda, kind):
    """fb_eval_run with Q tied bit for bit on the game's two actions plays action 0 on every step of every game: its records are
    those of games played with the constant action 0 (and not those of the constant action 1)"""
    from dqnflappybird_amd.evaluate import Evaluator
    n = 64
    net, ps = make_net(kind, 2, 64)
    load(net, ps, kind, 2, N_DIST, level_rows(kind, [3, 3]))
    l0, s0 = const_play(n, 0, 11)
    l1, _ = const_play(n, 1, 11)
    assert (l0 > 0).all() and not np.array_equal(l0, l1)
    res = Evaluator(n).run(net, n, 1, max_steps=3000, env_seed=11)
    assert not res.truncated.any()
    assert np.array_equal(res.length[:, 0], l0) and np.array_equal(res.score[:, 0], s0)


# ================================================================================================================ a* in training
@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_scalar_double_takes_the_first_maximum(torch_cuda, oracle, A, B):
    """FB_ALGO_DOUBLE with an online net tied bit for bit on s' and a target net that differs per action by O(1): q_target, |err| and
    the loss are those of the first maximum.  r, gamma and the Q are halves and integers: y is exact, compared bit for bit"""
    torch = torch_cuda
    net, ps = make_net("plain", A, 256)
    s, a, r, s2, t, _ = batch(B, A, 100 + A)
    d = lambda x: torch.from_numpy(x).cuda()
    q_tg = np.float32([4, -2, 6, 0, -5, 3, 1, -7][:A])
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    for lv in tie_patterns(A):
        load(net, ps, "plain", A, 0, (np.float32(lv), None), (q_tg, None))
        astar = int(np.argmax(lv))
        last = max(x for x in range(A) if lv[x] == lv[astar])
        assert last == astar or q_tg[astar] != q_tg[last]
        loss, ae, y = net.train_step("double", d(s), d(a), d(r), d(s2), d(t), gamma=0.5, flat_grad=grad)
        q = np.broadcast_to(np.float32(lv), (B, A))
        y0, loss0, ae0, _ = oracle.dqn_loss(1, q, np.full(B, q_tg[astar], np.float32), a, r, t, gamma=0.5)      # (1: the mean)
        assert np.array_equal(y0, np.where(t != 0, r, r + np.float32(0.5) * q_tg[astar]).astype(np.float32))
        assert np.array_equal(y.cpu().numpy(), y0), lv
        assert np.array_equal(ae.cpu().numpy(), ae0), lv
        np.testing.assert_allclose(loss.item(), loss0, rtol=1e-6)


def expected_c51(lg_on, lg_sel, lg_tg, a, r, t, gamma, w, astar=None):
    """float64: -> (loss, dl/dlogits [A, N] summed over the batch / B, a*) of include/fbdqn.h's C51 loss with argmax's first maximum"""
    N = lg_on.shape[1]
    sm = lambda x: np.exp(x - x.max(-1, keepdims=True)) / np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)
    z = np.linspace(-10.0, 10.0, N)
    if astar is None:
        astar = int(np.argmax((sm(np.asarray(lg_sel, np.float64)) * z).sum(1)))
    B = len(a)
    pn = np.tile(sm(np.asarray(lg_tg, np.float64)[astar]), (B, 1))
    m = np_project(pn, r, t, gamma, N, -10.0, 10.0)
    p = sm(np.asarray(lg_on, np.float64))[a]
    lb = -(m * np.log(p)).sum(1)
    g = np.zeros((lg_on.shape[0], N))
    for b in range(B):
        g[a[b]] += w[b] * (p[b] - m[b]) / B
    return float((w * lb).mean()), g, astar


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ["c51double", "c51doubleper"])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_c51_double_takes_the_first_maximum(torch_cuda, A, algo, B):
    """the online net's distributions tie bit for bit on s', the target net's differ per action (peaked on atom (5 a + 2) mod N), so the
    projected m, and with it the loss and the logit gradient, show the choice: both follow the first maximum.  The softmax and the
    logarithms are fp32 (a few ulp each): loss within 1e-5 relative, the bias gradient within 1e-5 absolute on entries of O(0.1);
    the last tied action in a*'s place moves the loss by more than 1 % and a gradient entry by more than 1e-2 / A (asserted)"""
    torch = torch_cuda
    N = N_DIST
    net, ps = make_net("c51", A, 256)
    s, a, r, s2, t, w = batch(B, A, 200 + A)
    if algo == "c51double":
        w = np.ones(B, np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    lg_tg = np.float32([[-1.0 * abs(i - (5 * x + 2) % N) for i in range(N)] for x in range(A)])
    base = np.float32([0.5 * (i % 4) for i in range(N)])    # (uniform online logits would make the loss log N whatever m is)
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    for lv in tie_patterns(A):
        lg_on = level_rows("c51", lv)[0] + base[None, :]
        load(net, ps, "c51", A, N, (lg_on, None), (lg_tg, None))
        loss0, g0, astar = expected_c51(lg_on, lg_on, lg_tg, a, r, t, 0.5, w)
        assert astar == int(np.argmax(lv))
        last = max(x for x in range(A) if lv[x] == lv[astar])
        loss1, g1, _ = expected_c51(lg_on, lg_on, lg_tg, a, r, t, 0.5, w, astar=last)
        assert last == astar or abs(loss1 - loss0) > 1e-2 * loss0 and np.abs(g1 - g0).max() > 1e-2 / A
        loss, _, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w) if algo.endswith("per") else None, gamma=0.5,
                                    flat_grad=grad)
        gb, _, _ = head_grads(grad.cpu().numpy(), "c51", A, N)
        print(f"c51 tie A={A} {algo} B={B} {lv}: loss {loss.item():.7g} want {loss0:.7g} other {loss1:.7g} grad err {np.abs(gb - g0).max():.3g}")
        np.testing.assert_allclose(loss.item(), loss0, rtol=1e-5)
        np.testing.assert_allclose(gb, g0, rtol=0, atol=1e-5)


QR_TIES = [(arch, A, algo) for arch in ("qr", "qrdueling") for A in (2, 3, 8) for algo in ("qr", "qrper", "qrdouble", "qrdoubleper")
           if not (arch == "qrdueling" and A == 3 and algo in ("qr", "qrper"))]       # (equal sums need an exact fold: A a power of two)


@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("arch,A,algo", QR_TIES)
def test_qr_astar_takes_the_first_maximum(torch_cuda, arch, A, algo, B):
    """qrdouble / qrdoubleper: the online net's quantiles tie bit for bit on s' and the target net's rows differ per action.  qr / qrper
    (one net selects and is read): target rows of equal integer sums and different shapes, level + (a + 1) x [-3, -1, 1, 3].  Loss, l_b
    and the head-bias gradients are those of the first maximum.  Every term is exact in fp32 but the division by B and the order of
    the batch sums (check_sum); the dueling fold at A = 3 divides by 3, one more rounding per quantile: 1e-6 relative slack there"""
    torch = torch_cuda
    N = 4
    dueling = arch == "qrdueling"
    net, ps = make_net(arch, A, 256, N=N)
    s, a, r, s2, t, w = batch(B, A, 300 + A)
    per = algo.endswith("per")
    if not per:
        w = np.ones(B, np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    v = (np.arange(N) % 3).astype(np.float32) if dueling else None
    theta = lambda b: fold32(v, b) if dueling else np.asarray(b, np.float32)
    ramp = lambda lv: (np.float32(lv)[:, None] + (np.arange(N, dtype=np.float32) - N // 2)[None, :]).astype(np.float32)
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    slack = 1e-6 if dueling and A == 3 else 0.0
    for lv in tie_patterns(A):
        if "double" in algo:
            b_on, b_tg = ramp(lv), distinct_rows(A, N)
            th_on, th_tg = theta(b_on), theta(b_tg)
            th_sel = th_on
        else:
            b_on, b_tg = distinct_rows(A, N), shaped_rows(lv)
            th_on, th_tg = theta(b_on), theta(b_tg)
            th_sel = th_tg
        load(net, ps, arch, A, N, (b_on, v), (b_tg, v))
        loss0, lb0, g0, gabs, astar = expected_qr(th_on, th_sel, th_tg, a, r, t, 0.5, 1.0, w)
        assert astar == int(np.argmax(lv))
        last = max(x for x in range(A) if lv[x] == lv[astar])
        sel1 = np.array(th_sel, np.float64); sel1[last] += 1.0                       # what the last maximum would give
        loss1, _, g1, _, a1 = expected_qr(th_on, sel1, th_tg, a, r, t, 0.5, 1.0, w)
        assert a1 == last and (last == astar or abs(loss1 - loss0) > 1e-3 * loss0 and np.abs(g1 - g0).max() > 1e-3 / A)
        loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w) if per else None, gamma=0.5, flat_grad=grad)
        gb, gv, _ = head_grads(grad.cpu().numpy(), arch, A, N)
        what = (arch, A, algo, B, lv)
        check_sum(loss.item(), loss0, loss0, B, what, slack)
        if dueling:
            check_sum(gv, g0.sum(0), gabs.sum(0), B + A, what, slack)
            check_sum(gb, g0 - g0.mean(0, keepdims=True), gabs + gabs.mean(0, keepdims=True), B + A + 1, what, slack)
        else:
            check_sum(gb, g0, gabs, B, what, slack)
        if per:
            check_sum(ae.cpu().numpy(), lb0, lb0, 1, what, slack)


# ================================================================================================================ the quantile Huber loss
def ref_hidden(p, s):
    """float64 relu(fc1) [B, FC] of the trunk in p (an identity head on torch_forward, as tests/test_gpu_c51_dueling.py::ref_logits_d)"""
    import torch
    P = torch.as_tensor(p[:HEAD0(FC)], dtype=torch.float64)
    ident = torch.cat([P, torch.eye(FC, dtype=torch.float64).flatten(), torch.zeros(FC, dtype=torch.float64)])
    with torch.no_grad():
        return torch_forward(ident, torch.as_tensor(s, dtype=torch.float64), FC, FC).numpy()


@pytest.mark.parametrize("B", [1, 32, 256])
@pytest.mark.parametrize("A", [2, 3])
def test_the_headers_worked_case(torch_cuda, A, B):
    """include/fbdqn.h: N = 2, kappa = 1, theta = [0, 1] on the taken action, T = [0.5, 3] = 0.5 + 0.5 x [0, 5] (the target net's a*):
    l = 0.90625, dl/dtheta = [-0.1875, -0.3125] / B per sample.  tau = 1/4, 3/4, u in {0.5, 3, -0.5, 2}, the Huber terms 1/8, 5/2, 1/8,
    3/2 and their weighted sums are dyadic rationals of a few bits, and B is a power of two: every fp32 operation of the kernel is
    exact, in any order, so loss and bias gradient are compared at rtol 1e-6 (one rounding's worth, for the conversions on the way
    out).  The other actions' bias and weight gradients and, the head's weights being zero, the whole trunk's are exactly 0; W_fc2's
    gradient is the bias gradient times the batch mean of the activations (the float64 trunk, the head tensors' usual tolerance)"""
    torch = torch_cuda
    N = 2
    net, ps = make_net("qr", A, 256, N=N, kappa=1.0)
    rng = np.random.default_rng(B + A)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    d = lambda x: torch.from_numpy(x).cuda()
    h = ref_hidden(ps[0], s).mean(0)
    assert (h > 0).mean() > 0.1
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    for taken in range(A):
        astar = (taken + 1) % A
        th_on = np.float32([[10 + x, 20 + x] for x in range(A)]); th_on[taken] = [0, 1]
        th_tg = np.float32([[-4 - x, -2 - x] for x in range(A)]); th_tg[astar] = [0, 5]
        load(net, ps, "qr", A, N, (th_on, None), (th_tg, None))
        a, r, t = np.full(B, taken, np.uint8), np.full(B, 0.5, np.float32), np.zeros(B, np.uint8)
        loss0, _, g0, _, a0 = expected_qr(th_on, th_tg, th_tg, a, r, t, 0.5, 1.0)
        assert a0 == astar and loss0 == 0.90625 and np.array_equal(g0[taken], [-0.1875, -0.3125])
        for algo in ("qr", "qrper"):
            grad.fill_(7.0)
            loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=torch.ones(B, device="cuda") if algo == "qrper" else None,
                                         gamma=0.5, flat_grad=grad)
            g = grad.cpu().numpy()
            gb, _, tb = head_grads(g, "qr", A, N)
            np.testing.assert_allclose(loss.item(), 0.90625, rtol=1e-6)
            np.testing.assert_allclose(gb[taken], [-0.1875, -0.3125], rtol=1e-6)
            if algo == "qrper":
                np.testing.assert_allclose(ae.cpu().numpy(), np.full(B, 0.90625), rtol=1e-6)
            gw = tb["W_head"].reshape(FC, A, N)
            for x in range(A):
                if x != taken:
                    assert not gb[x].any() and not gw[:, x].any(), (taken, x)
            want = h[:, None] * g0[taken][None, :]
            np.testing.assert_allclose(gw[:, taken], want, rtol=2e-3, atol=2e-5 * np.abs(want).max())
            assert not g[:HEAD0(FC)].any()                       # dhf = sum_i g_i W[j, i] = 0: nothing reaches the trunk


KINK_A = [2, 3]


@pytest.mark.parametrize("B", [1, 255])
@pytest.mark.parametrize("kappa", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("A", KINK_A)
def test_kinks_terminals_and_zero_errors(torch_cuda, A, kappa, B):
    """theta = [a, a] on action a (N = 2) and targets placed so that |u| = kappa on every pair, with both signs in one batch: all
    terminal (T = r on every lane, under a target net whose biases are 1e30), none terminal (T = r + 0.5 x [4, 4]), and mixed; then
    u = 0 on every pair.  At |u| = kappa both branches of L_k give k^2 / 2 and the clamp gives +-k, at u = 0 loss and gradient are 0
    under either convention for the indicator, so this pins the values and the branches' agreement, not `<` against `<=`.  Expected
    values from np_qr_loss; each sample's are exact in fp32, the batch sums within check_sum's bound"""
    torch = torch_cuda
    N = 2
    net, ps = make_net("qr", A, 256, N=N, kappa=kappa)
    rng = np.random.default_rng(B)
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    d = lambda x: torch.from_numpy(x).cuda()
    k = np.float32(kappa)
    th_on = np.float32([[x, x] for x in range(A)])
    normal, huge = np.float32([[4, 4]] + [[-9, -9]] * (A - 1)), np.full((A, N), 1e30, np.float32)
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    for first in (0, 1) if B == 1 else (0,):
        i = np.arange(B) + first
        a = (i % A).astype(np.uint8)
        sign = np.where(i % 2 == 0, 1.0, -1.0).astype(np.float32)
        cases = [("all terminal", huge, np.ones(B, np.uint8), sign), ("none terminal", normal, np.zeros(B, np.uint8), sign),
                 ("zero", huge, np.ones(B, np.uint8), 0 * sign)]
        if B > 1:
            cases.append(("mixed", normal, (i % 3 == 0).astype(np.uint8), sign))
        for name, th_tg, t, sg in cases:
            r = (a + sg * k - np.where(t != 0, 0, 2)).astype(np.float32)
            load(net, ps, "qr", A, N, (th_on, None), (th_tg, None))
            loss0, lb0, g0, gabs, astar = expected_qr(th_on, th_tg, th_tg, a, r, t, 0.5, kappa)
            assert astar == 0
            if name != "zero":
                np.testing.assert_allclose(lb0, 0.5 * kappa, rtol=1e-15)       # |u| = kappa on every pair of every sample
                assert B == 1 or (g0 > 0).any() and (g0 < 0).any()
            for algo in ("qr", "qrper"):
                grad.fill_(7.0)
                loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=torch.ones(B, device="cuda") if algo == "qrper" else None,
                                             gamma=0.5, flat_grad=grad)
                g = grad.cpu().numpy()
                gb, _, tb = head_grads(g, "qr", A, N)
                what = (name, A, kappa, B, algo, first)
                if name == "zero":
                    assert loss.item() == 0.0 and not g.any(), what
                    continue
                check_sum(loss.item(), loss0, loss0, B, what)
                check_sum(gb, g0, gabs, B, what)
                if algo == "qrper":
                    assert np.array_equal(ae.cpu().numpy(), lb0.astype(np.float32)), what
                assert tb["W_head"].any() and not g[:HEAD0(FC)].any(), what


# ================================================================================================================ ramps
@pytest.mark.parametrize("arch", ["qr", "qrdueling"])
@pytest.mark.parametrize("N", [2, 64])
def test_integer_ramps_come_back_bit_for_bit(torch_cuda, arch, N):
    """integer ramps as biases at N = 64 (every lane on) and N = 2 (62 lanes masked): forward_quantiles returns them (through the
    fold, for the dueling head: integers and halves) bit for bit and forward their exact mean, both nets, both trunk paths"""
    torch = torch_cuda
    A = 2
    net, ps = make_net(arch, A, 700, N=N)
    i = np.arange(N, dtype=np.float32)
    bs = [np.float32([i - 20 + 100 * x for x in range(A)]), np.float32([3 * i - 7 * x for x in range(A)])]
    v = (i % 5).astype(np.float32) if arch == "qrdueling" else None
    load(net, ps, arch, A, N, (bs[0], v), (bs[1], v))
    sd = torch.from_numpy(rand_states(np.random.default_rng(N), 700)).cuda()
    for which in (0, 1):
        th0 = fold32(v, bs[which]) if v is not None else bs[which]
        exact = np.asarray(bs[which], np.float64) + (0 if v is None else v[None, :] - np.asarray(bs[which], np.float64).mean(0, keepdims=True))
        assert np.array_equal(th0.astype(np.float64), exact)
        q0 = (exact.sum(1) / N).astype(np.float32)
        assert np.array_equal(q0.astype(np.float64), exact.sum(1) / N)
        for B in (1, 255, 256, 700):
            th = net.forward_quantiles(sd[:B].contiguous(), which).cpu().numpy()
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            assert np.array_equal(bits(th), bits(np.broadcast_to(th0, th.shape))), (which, B)
            assert np.array_equal(bits(q), bits(np.broadcast_to(q0, q.shape))), (which, B)
