"""Noisy C51 nets on the MI355X (include/fbdqn.h): the noise against a numpy restatement of its Philox / Box-Muller
draw, forward, distributions, the loss and every gradient of [mu | sigma] against a float64 torch-CPU restatement that builds
mu + sigma (.) (f(eps_out) x f(eps_in)) directly (the trunk of tests/test_oracle_qnet.py::torch_forward, then the C51 or dueling C51
head), the reductions to the non-noisy net bit for bit (mean mode, sigma = 0), the effective weights' freshness after every change,
and every path that trains or plays the net against its composed calls, bit for bit."""
import ctypes
import zlib

import numpy as np
import pytest

from tests.test_c51_per_host import np_kl_priority
from tests.test_gpu_c51 import FC, GAMMA, _batch, _check_grads, greedy_next, head0, ref_logits, support, torch_project
from tests.test_gpu_c51_dueling import check_grads as check_grads_d
from tests.test_gpu_c51_dueling import head_size, ref_logits_d
from tests.test_gpu_eval import composed as composed_eval
from tests.test_gpu_nstep import played
from tests.test_gpu_nstep_per import per_memory
from tests.test_oracle_qnet import rand_states

pytestmark = pytest.mark.gpu
ALGOS = ("c51", "c51double", "c51per", "c51doubleper")
PER = ("c51per", "c51doubleper")
HEADS = ("c51", "c51dueling")
TRUNK = 77984                                              # W_fc1's first entry: sigma covers the vector from here on
STREAM_NOISE = 6


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def n_mu(head, N, A=2, fc=FC):
    return head0(fc) + (fc * A * N + A * N if head == "c51" else head_size(N, A, fc))


def layers(head, N, A=2, fc=FC):
    """(w, fan_in, fan_out) of the noisy layers in flat order, and their noise offsets (ein, eout)"""
    o, out, e = head0(fc), [(TRUNK, 1600, fc)], 0
    if head == "c51dueling":
        out.append((o, fc, N))
        o += fc * N + N
    out.append((o, fc, A * N))
    res = []
    for w, fi, fo in out:
        res.append((w, fi, fo, e, e + fi))
        e += fi + fo
    return res, e


def factors(head, N, nz, A=2, fc=FC):
    """e(q) for q in [TRUNK, n_mu): f(eps_out_j) f(eps_in_i) for a weight, f(eps_out_j) for a bias -- float64 [n_mu - TRUNK]"""
    nz = np.asarray(nz, np.float64)
    parts = []
    for w, fi, fo, ein, eout in layers(head, N, A, fc)[0]:
        parts += [np.outer(nz[ein:ein + fi], nz[eout:eout + fo]).ravel(), nz[eout:eout + fo]]
    e = np.concatenate(parts)
    assert e.size == n_mu(head, N, A, fc) - TRUNK
    return e


def factors32(head, N, nz, A=2, fc=FC):
    """the same products in float32, as the device forms them (f(eps_out) * f(eps_in))"""
    nz = np.asarray(nz, np.float32)
    parts = []
    for w, fi, fo, ein, eout in layers(head, N, A, fc)[0]:
        parts += [(nz[None, eout:eout + fo] * nz[ein:ein + fi, None]).ravel(), nz[eout:eout + fo]]
    return np.concatenate(parts)


def effective(P, nz, head, N, A=2, fc=FC):
    """float64 torch: the effective parameters mu + sigma (.) e of a master vector P = [mu | sigma] (differentiable in P)"""
    import torch
    n = n_mu(head, N, A, fc)
    E = torch.as_tensor(factors(head, N, nz, A, fc))
    P = torch.as_tensor(P, dtype=torch.float64)
    return torch.cat([P[:TRUNK], P[TRUNK:n] + P[n:] * E])


def logits(head, P_eff, s, N, A=2, fc=FC):
    import torch
    if head == "c51":
        return ref_logits(torch.as_tensor(P_eff, dtype=torch.float64), s, N, A, fc)
    return ref_logits_d(P_eff, s, N, A, fc)


def np_noise(seed, step, which, size):
    """the documented draw: element k of net `which` at (seed, step), via the oracle's Philox4x32-10 -> (z float64 of the float32
    uniforms, f(z) float32 with numpy's float32 log / cos)"""
    from oracle import oracle as orc
    z64, f32 = np.empty(size), np.empty(size, np.float32)
    for k in range(size):
        r = orc.philox(seed & 0xFFFFFFFF, seed >> 32, k, step & 0xFFFFFFFF, STREAM_NOISE, ((step >> 32) * 2 + which) & 0xFFFFFFFF)
        u1 = np.float32((int(r[0]) >> 8) + 1) * np.float32(1.0 / 16777216.0)
        u2 = np.float32(int(r[1]) >> 8) * np.float32(1.0 / 16777216.0)
        z64[k] = np.sqrt(-2.0 * np.log(np.float64(u1))) * np.cos(2.0 * np.pi * np.float64(u2))
        z = np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.28318530717958647692) * u2)
        f32[k] = np.copysign(np.sqrt(np.abs(z)), z)
    return z64, f32


def make_noisy(head="c51", N=51, max_batch=256, seed=3, sigma0=0.5, sigma_scale=1.0, A=2, fc=FC):
    """a noisy net with mu scaled as tests/test_gpu_c51.py::make_c51 scales a C51 net (x 3), sigma as initialised (x sigma_scale)"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(A, fc, head, max_batch=max_batch, n_atoms=N, noisy=True, sigma0=sigma0)
    n = n_mu(head, N, A, fc)
    ps = []
    for which in (0, 1):
        net.init_params(seed + which, which)
        p = net.store_params(which).cpu().numpy()
        p[:n] *= 3.0
        p[n:] *= sigma_scale
        net.load_params(p, which)
        ps.append(p)
    return net, ps[0], ps[1]


def plain_twin(head, N, mu_on, mu_tg, max_batch=256):
    """the non-noisy net of the same head holding the given mu"""
    from dqnflappybird_amd.vec import QNet
    net = QNet(2, FC, head, max_batch=max_batch, n_atoms=N)
    net.load_params(mu_on, 0)
    net.load_params(mu_tg, 1)
    return net


def ref_q(head, P_eff, s, N, A=2, fc=FC):
    import torch
    with torch.no_grad():
        return (torch.softmax(logits(head, P_eff, s, N, A, fc), -1) * support(N, -10.0, 10.0)).sum(-1).numpy()


def frozen(net):
    m, v, p = net.adam_state()
    return net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), p.copy(), net.noise(0).clone(), net.noise(1).clone()


def held(net):
    return net.store_params(0).clone(), net.store_params(1).clone(), net.noise(0).clone(), net.noise(1).clone()


def same(x, y):
    import torch
    return all(torch.equal(i, j) if torch.is_tensor(i) else np.array_equal(i, j) for i, j in zip(x, y))


# ---------------------------------------------------------------------------------------------------------------- the noise
@pytest.mark.parametrize("head", HEADS)
def test_noise_is_the_documented_draw(torch_cuda, head):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    net, _, _ = make_noisy(head, 51)
    size = net.noise_size
    assert size == layers(head, 51)[1]
    assert L.lib().fb_qnet_is_noisy(net.h) == 1
    for which in (0, 1):                                   # a new net is in mean mode
        assert torch.equal(net.noise(which), torch.zeros(size, device="cuda"))
    for seed, step in ((5, 9), ((7 << 32) + 123, (3 << 32) + 77)):
        for which in (0, 1):
            net.reset_noise(which, seed, step)
            f = net.noise(which).cpu().numpy()
            z64, f32 = np_noise(seed, step, which, size)
            zd = np.sign(f).astype(np.float64) * np.square(f.astype(np.float64))
            np.testing.assert_allclose(zd, z64, rtol=1e-5, atol=1e-5, err_msg=f"which={which}")
            np.testing.assert_allclose(f, f32, rtol=1e-5, atol=2e-3)
            assert np.abs(f - f32).mean() < 5e-6
            net.reset_noise(which, seed, step)                  # the same key: the same bits
            assert np.array_equal(net.noise(which).cpu().numpy(), f)
        a, b = net.noise(0).cpu().numpy(), net.noise(1).cpu().numpy()
        assert (a != b).mean() > 0.99                           # online and target: independent vectors for one key
        assert abs(np.corrcoef(a, b)[0, 1]) < 0.1
    # host memory works as well, and the statistics are those of f(N(0, 1))
    host = np.empty(size, np.float32)
    L.check(L.lib().fb_qnet_get_noise(net.h, 0, L.ptr(host)), "fb_qnet_get_noise")
    assert np.array_equal(host, net.noise(0).cpu().numpy())
    assert abs(np.mean(np.square(host) * np.sign(host))) < 0.1 and abs(np.mean(np.square(host) ** 2) - 1.0) < 0.15
    net.mean_noise(0)
    assert torch.equal(net.noise(0), torch.zeros(size, device="cuda")) and bool((net.noise(1) != 0).any())


def test_sigma_init(torch_cuda):
    """mu as the non-noisy net's (the same Philox draws), sigma = sigma0 / sqrt(fan_in) for weights and biases"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    for head in HEADS:
        N = 51
        plain = QNet(2, FC, head, n_atoms=N, max_batch=8)
        for s0 in (0.5, 0.0, 1.7):
            net = QNet(2, FC, head, n_atoms=N, max_batch=8, noisy=True, sigma0=s0)
            n = n_mu(head, N)
            assert net.n_params == 2 * n - TRUNK and net.noisy
            net.init_params(21, 0)
            plain.init_params(21, 0)
            p = net.store_params(0).cpu().numpy()
            assert np.array_equal(p[:n], plain.store_params(0).cpu().numpy())
            want = np.concatenate([np.full((fi + 1) * fo, np.float32(np.float64(np.float32(s0)) / np.sqrt(fi)), np.float32) for _, fi, fo, _, _ in layers(head, N)[0]])
            assert np.array_equal(p[n:], want), (head, s0)


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("N", [2, 51, 64])
@pytest.mark.parametrize("head", HEADS)
def test_forward_dist_and_eval_q_match_the_restatement(torch_cuda, head, N):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    net, p_on, p_tg = make_noisy(head, N, max_batch=700)
    net.reset_noise(0, 11, 4)
    net.reset_noise(1, 11, 4)
    eff = {w: effective(p, net.noise(w).cpu().numpy(), head, N) for w, p in ((0, p_on), (1, p_tg))}
    mu_only = effective(p_on, np.zeros(net.noise_size), head, N)
    rng = np.random.default_rng(N)
    s = rand_states(rng, 2048)
    with torch.no_grad():
        pr = {w: torch.softmax(logits(head, eff[w], s, N), -1) for w in (0, 1)}
        pm = torch.softmax(logits(head, mu_only, s[:256], N), -1)
    assert (pr[0][:256] - pm).abs().max().item() > 1e-2          # the noise moves the distributions well past the tolerance
    z = support(N, -10.0, 10.0)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 32, 255, 256, 2048):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            p = net.forward_dist(sd[:B].contiguous(), which).cpu().numpy()
            np.testing.assert_allclose(p, pr[which][:B].numpy(), rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, (pr[which][:B] * z).sum(-1).numpy(), rtol=0, atol=5e-4, err_msg=f"B={B} which={which}")
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env, rep = VecGameState(300, seed=2), VecReplay(5000, 300)
    nib = env.track_state()
    env.observe()
    rep.reset(env.frame_bits)
    for k in range(12):
        acts = torch.full((300,), k % 3 == 0, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        rep.push(env.frame_bits, acts, env.reward, env.terminal)
    qe = torch.empty((300, 2), dtype=torch.float32, device="cuda")
    L.check(L.lib().fb_eval_q(net.h, L.ptr(nib), 300, L.ptr(qe), L.current_stream()), "fb_eval_q")
    _, qa = net.act_nib(nib, 0.0, want_q=True)
    assert torch.equal(qe, qa)
    np.testing.assert_allclose(qe.cpu().numpy(), ref_q(head, eff[0], rep.current_state().cpu().numpy(), N), rtol=0, atol=5e-4)


# ---------------------------------------------------------------------------------------------------------------- training
def ref_train(head, m_on, nz_on, m_tg, nz_tg, s, a, r, s2, t, w, G, algo, N, dev_astar, A=2, fc=FC):
    """-> (loss, gradient of [mu | sigma], KL per sample) in float64 with autograd through mu + sigma (.) e"""
    import torch
    P = torch.tensor(m_on, dtype=torch.float64, requires_grad=True)
    z = support(N, -10.0, 10.0)
    B = len(s)
    eff = effective(P, nz_on, head, N, A, fc)
    with torch.no_grad():
        pt = torch.softmax(logits(head, effective(m_tg, nz_tg, head, N, A, fc), s2, N, A, fc), -1)
        sel = torch.softmax(logits(head, eff.detach(), s2, N, A, fc), -1) if algo in ("c51double", "c51doubleper") else pt
        q = (sel * z).sum(-1)
        astar = greedy_next(q, dev_astar)
        m = torch_project(pt[torch.arange(B), astar], torch.as_tensor(r.astype(np.float64)), torch.as_tensor(t.astype(np.float64)),
                          G, N, -10.0, 10.0)
    logp = torch.log_softmax(logits(head, eff, s, N, A, fc)[torch.arange(B), torch.as_tensor(a, dtype=torch.long)], -1)
    ce = -(m * logp).sum(-1)
    loss = (torch.as_tensor(w, dtype=torch.float64) * ce).mean() if w is not None else ce.mean()
    loss.backward()
    return loss.item(), P.grad.numpy(), np_kl_priority(m.numpy(), logp.detach().exp().numpy())


def check_noisy_grads(g, g0, head, N, nz_on, A=2, fc=FC):
    """mu: the non-noisy tests' per-tensor tolerances; sigma: exactly the device's mu gradient x e(q) in float32, and against
    autograd per layer (fc1 in relative L2 -- ReLU kinks -- the head elementwise)"""
    n = n_mu(head, N, A, fc)
    if head == "c51":
        _check_grads(g[:n], g0[:n], A * N, fc)
    else:
        check_grads_d(g[:n], g0[:n], N, A, fc)
    gs, gs0 = g[n:], g0[n:]
    assert np.array_equal(gs, g[TRUNK:n] * factors32(head, N, nz_on, A, fc))
    o = 0
    for k, (w, fi, fo, _, _) in enumerate(layers(head, N, A, fc)[0]):
        for lo, hi in ((o, o + fi * fo), (o + fi * fo, o + (fi + 1) * fo)):
            ref, got = gs0[lo:hi], gs[lo:hi]
            scale = np.abs(ref).max()
            assert scale > 0, (head, k, lo)
            if k == 0:
                assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 2e-3, (head, k, lo)
            else:
                np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=f"sigma[{lo}:{hi}]")
        o += (fi + 1) * fo


CASES = [(head, algo, B) for head in HEADS for algo in ALGOS for B in (1, 32, 255, 256)]


@pytest.mark.parametrize("head,algo,B", CASES)
def test_loss_and_every_gradient_match_autograd(torch_cuda, head, algo, B):
    torch = torch_cuda
    N = 51
    net, p_on, p_tg = make_noisy(head, N, max_batch=256)
    net.reset_noise(0, B, 1)
    net.reset_noise(1, B, 1)
    nz_on, nz_tg = net.noise(0).cpu().numpy(), net.noise(1).cpu().numpy()
    rng = np.random.default_rng(zlib.crc32(f"n-{head}-{algo}-{B}".encode()))
    s, a, r, s2, t = _batch(rng, B)
    d = lambda x: torch.from_numpy(x).cuda()
    w = (1.0 - rng.random(B)).astype(np.float32) if algo in PER else None
    dev_astar = net.forward(d(s2), 0 if "double" in algo else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = held(net)
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w) if w is not None else None, gamma=GAMMA, flat_grad=grad,
                                 want_aux=algo in PER)
    loss0, g0, kl0 = ref_train(head, p_on, nz_on, p_tg, nz_tg, s, a, r, s2, t, w.astype(np.float64) if w is not None else None, GAMMA,
                               algo, N, dev_astar)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_noisy_grads(grad.cpu().numpy(), g0, head, N, nz_on)
    if algo in PER:
        np.testing.assert_allclose(ae.cpu().numpy(), kl0, rtol=1e-4, atol=5e-4)
    assert same(held(net), before)                         # (an exported gradient changes no parameter, nor the noise)


# ---------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("algo", ["c51", "c51doubleper"])
@pytest.mark.parametrize("head", HEADS)
def test_mean_mode_trains_mu_as_the_plain_net(torch_cuda, head, algo):
    """in mean mode sigma's gradient is 0 and its Adam update a no-op: K fused steps leave mu (and its Adam state) bit for bit where the
    non-noisy net holding the same mu leaves its parameters, sigma where it was"""
    torch = torch_cuda
    N = 51
    n = n_mu(head, N)
    net, p_on, p_tg = make_noisy(head, N)
    twin = plain_twin(head, N, p_on[:n], p_tg[:n])
    for x in (net, twin):
        x.set_hparams(lr=1e-4)
    rng = np.random.default_rng(3)
    for step in range(4):
        B = 256 if step == 3 else 32
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        isw = torch.from_numpy((1.0 - rng.random(B)).astype(np.float32)).cuda() if algo in PER else None
        l1, e1, _ = net.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, want_aux=algo in PER)
        l2, e2, _ = twin.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, want_aux=algo in PER)
        assert torch.equal(l1, l2), step
        if algo in PER:
            assert torch.equal(e1, e2)
    p = net.store_params(0)
    assert torch.equal(p[:n], twin.store_params(0)) and not torch.equal(p[:n].cpu(), torch.from_numpy(p_on[:n]))
    assert torch.equal(p[n:].cpu(), torch.from_numpy(p_on[n:]))
    m1, v1, pw1 = net.adam_state()
    m2, v2, pw2 = twin.adam_state()
    assert torch.equal(m1[:n], m2) and torch.equal(v1[:n], v2) and np.array_equal(pw1, pw2)
    assert not bool(m1[n:].any()) and not bool(v1[n:].any())


@pytest.mark.parametrize("head", HEADS)
def test_zero_sigma_with_a_sample_is_the_plain_net(torch_cuda, head):
    torch = torch_cuda
    N = 51
    n = n_mu(head, N)
    net, p_on, p_tg = make_noisy(head, N, max_batch=400, sigma_scale=0.0)
    twin = plain_twin(head, N, p_on[:n], p_tg[:n], max_batch=400)
    net.reset_noise(0, 3, 3)
    net.reset_noise(1, 3, 3)
    assert bool((net.noise(0) != 0).any())
    s = torch.from_numpy(rand_states(np.random.default_rng(1), 1100)).cuda()
    for B in (7, 200, 256, 1100):
        x = s[:B].contiguous()
        for which in (0, 1):
            assert torch.equal(net.forward(x, which), twin.forward(x, which)), (B, which)
            assert torch.equal(net.forward_dist(x, which), twin.forward_dist(x, which)), (B, which)
        a1, q1 = net.act(x, 0.1, seed=4, step=B, want_q=True)
        a2, q2 = twin.act(x, 0.1, seed=4, step=B, want_q=True)
        assert torch.equal(a1, a2) and torch.equal(q1, q2)


# ---------------------------------------------------------------------------------------------------------------- composed calls
@pytest.mark.parametrize("B", [32, 256])
@pytest.mark.parametrize("algo", ALGOS)
def test_fused_adam_equals_exported_gradient_plus_apply(torch_cuda, algo, B):
    torch = torch_cuda
    rng = np.random.default_rng(B + len(algo))
    head = "c51dueling" if "double" in algo else "c51"
    n1, _, _ = make_noisy(head)
    n2, _, _ = make_noisy(head)
    for n in (n1, n2):
        n.set_hparams(lr=1e-4)
    g = torch.zeros(n1.n_params, dtype=torch.float32, device="cuda")
    for step in range(3):
        for n in (n1, n2):
            n.reset_noise(0, 1, step)
            n.reset_noise(1, 1, step)
        s, a, r, s2, t = (torch.from_numpy(x).cuda() for x in _batch(rng, B))
        isw = torch.from_numpy((1.0 - rng.random(B)).astype(np.float32)).cuda() if algo in PER else None
        l1, _, _ = n1.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, want_aux=False)
        l2, _, _ = n2.train_step(algo, s, a, r, s2, t, isw=isw, gamma=GAMMA, flat_grad=g, want_aux=False)
        n2.apply_adam(g)
        assert torch.equal(l1, l2)
        assert torch.equal(n1.store_params(), n2.store_params())
    m1, v1, p1 = n1.adam_state()
    m2, v2, p2 = n2.adam_state()
    assert torch.equal(m1, m2) and torch.equal(v1, v2) and np.array_equal(p1, p2)
    n = n_mu(head, 51)
    assert bool(m1[n:].any())                              # sigma did train


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("algo", ["c51", "c51double"])
def test_ring_fed_equals_gather_plus_train_step(torch_cuda, algo, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import bootstrap_gamma, train_from_replay
    _, rep = played(256, 20000, 30, seed=5)
    rep.set_n_step(n, GAMMA)
    G = bootstrap_gamma(GAMMA, n)
    rng = np.random.default_rng(n)
    for B in (1, 32, 255):
        n1, _, _ = make_noisy("c51dueling")
        n2, _, _ = make_noisy("c51dueling")
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(3):
            for net in (n1, n2):
                net.reset_noise(0, B, step)
                net.reset_noise(1, B, step)
            idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, _, _ = n1.train_step(algo, s, a, r, s2, t, gamma=G, flat_grad=g1 if exp else None, want_aux=False)
            out = train_from_replay(rep, n2, algo, idx, gamma=GAMMA, flat_grad=g2 if exp else None)
            assert torch.equal(l1, out[0]), (algo, n, B, step)
            if exp:
                assert torch.equal(g1, g2)
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params()), (algo, n, B, step)


def _pipeline(N, n, algo, head, seed=5):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env = VecGameState(N, seed=seed)
    if algo in PER:
        rep = per_memory(6 * N + 13, N, n, "exact")
    else:
        rep = VecReplay(max(20000, 16 * N), N)
        rep.seed(9, "cpython")
        rep.set_n_step(n, GAMMA)
    net, _, _ = make_noisy(head, max_batch=N)
    net.set_hparams(lr=1e-4)
    nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return env, rep, net, nib


VEC_CASES = [(algo, n, 256) for algo in ALGOS for n in (1, 3)] + [("c51double", 3, 64), ("c51doubleper", 3, 64)]


@pytest.mark.parametrize("algo,n,N", VEC_CASES)
def test_vec_step_equals_separate_calls(torch_cuda, algo, n, N):
    """fb_vec_step on a noisy net == reset_noise(0) -> act_nib -> frame_step -> push -> sample -> reset_noise(1) -> train_from_replay
    (-> batch_update): actions, indices, weights, losses, priorities, parameters, both nets' noise and the memory's state"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecStep, train_from_replay
    B, steps, seed = 32, 14, 1
    per = algo in PER
    head = "c51dueling" if "double" in algo else "c51"
    e1, r1, n1, nib1 = _pipeline(N, n, algo, head)
    e2, r2, n2, nib2 = _pipeline(N, n, algo, head)
    one = VecStep(e2, r2, n2, B, algo, GAMMA)
    for step in range(steps):
        train = step >= 4
        if train and step % 5 == 0:
            n1.sync_target(); n2.sync_target()
        n1.reset_noise(0, seed, step)
        a1 = n1.act_nib(nib1, 0.0, seed=seed, step=step)
        e1.frame_step(a1, want_u8=False)
        r1.push(e1.frame_bits, a1, e1.reward, e1.terminal)
        if train:
            idx, isw = r1.sample(B)
            n1.reset_noise(1, seed, step)
            if per:
                loss, _, r_, t_, ae = train_from_replay(r1, n1, algo, idx, gamma=GAMMA, isw=isw, want_abs_err=True)
                r1.update_priorities(idx, abs_err=ae)
            else:
                loss, _, r_, t_ = train_from_replay(r1, n1, algo, idx, gamma=GAMMA)
        a2 = one(0.0, seed=seed, step=step, train=train)
        assert torch.equal(a1, a2), step
        assert torch.equal(n1.noise(0), n2.noise(0)) and torch.equal(n1.noise(1), n2.noise(1)), step
        if train:
            assert torch.equal(idx, one.idx) and torch.equal(loss, one.loss), step
            assert torch.equal(r_, one.r) and torch.equal(t_, one.t), step
            if per:
                assert torch.equal(isw, one.isw) and torch.equal(ae, one.abs_err + 0.01), step
    assert torch.equal(n1.store_params(0), n2.store_params(0)) and torch.equal(n1.store_params(1), n2.store_params(1))
    assert (e1.get_state() == e2.get_state()).all()
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob()))
    assert n2.split_stats() == (0, 0)                      # the one-stream schedule
    assert bool(n2.noise(0).any()) and bool(n2.noise(1).any())


@pytest.mark.parametrize("noise", ["mean", "sample"])
def test_eval_run_equals_composed_calls(torch_cuda, noise):
    from dqnflappybird_amd.evaluate import evaluate
    net, _, _ = make_noisy("c51dueling", max_batch=343)
    act_seed = 17
    if noise == "mean":
        net.mean_noise(0)
    else:
        net.reset_noise(0, act_seed, 0)
    s0, l0, t0, _ = composed_eval(net, 1027, 1027, 1, env_seed=11)
    net.reset_noise(0, 99, 99)                             # evaluate() sets the online noise itself
    res = evaluate(net, 1027, 1, max_steps=100_000, env_seed=11, act_seed=act_seed, noise=noise)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all()
    assert bool(net.noise(0).any()) == (noise == "sample")


def test_the_effective_weights_are_never_stale(torch_cuda):
    """after init_params, load_params, a target sync, a fused train step, apply_adam and each reset, forward and acting give the
    restatement's Q of the master vector and noise as they now are (an effective vector left behind by any of them fails here)"""
    torch = torch_cuda
    N = 51
    for head in HEADS:
        net, p_on, _ = make_noisy(head, N)
        net.set_hparams(lr=3e-3)
        rng = np.random.default_rng(7)
        s = rand_states(rng, 64)
        sd = torch.from_numpy(s).cuda()

        def check(which, what):
            P = net.store_params(which).cpu().numpy()
            q0 = ref_q(head, effective(P, net.noise(which).cpu().numpy(), head, N), s, N)
            q = net.forward(sd, which).cpu().numpy()
            np.testing.assert_allclose(q, q0, rtol=0, atol=5e-4, err_msg=f"{head}: {what}")
            if which == 0:
                _, qa = net.act(sd, 0.0, want_q=True)
                np.testing.assert_allclose(qa.cpu().numpy(), q0, rtol=0, atol=5e-4, err_msg=f"{head}: {what}")
            return q

        q_prev = check(0, "make")
        net.reset_noise(0, 1, 2)
        q = check(0, "reset_noise")
        assert np.abs(q - q_prev).max() > 1e-2
        net.reset_noise(1, 1, 2)
        check(1, "reset_noise target")
        net.init_params(11, 0)
        check(0, "init_params")
        p2 = p_on.copy()
        p2[n_mu(head, N):] *= 2.0
        net.load_params(p2, 0)
        check(0, "load_params")
        net.sync_target()
        check(1, "sync_target")
        for k in range(2):
            s_, a_, r_, s2_, t_ = (torch.from_numpy(x).cuda() for x in _batch(rng, 32))
            q_prev = net.forward(sd).cpu().numpy()
            if k == 0:
                net.train_step("c51", s_, a_, r_, s2_, t_, gamma=GAMMA)
                q = check(0, "fused train step")
            else:
                g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
                net.train_step("c51double", s_, a_, r_, s2_, t_, gamma=GAMMA, flat_grad=g)
                net.apply_adam(g)
                q = check(0, "apply_adam")
            assert np.abs(q - q_prev).max() > 5e-3
        net.mean_noise(0)
        check(0, "mean")


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep
    N, B = 256, 32
    net, _, _ = make_noisy("c51dueling", max_batch=N)
    net.reset_noise(0, 1, 1)
    env = VecGameState(N, seed=1); env.track_state(); env.observe()
    uni = VecReplay(20000, N); uni.reset(env.frame_bits)
    for _ in range(4):
        acts = torch.zeros(N, dtype=torch.uint8, device="cuda")
        env.frame_step(acts, want_u8=False)
        uni.push(env.frame_bits, acts, env.reward, env.terminal)
    torch.cuda.synchronize()
    blob, env_state, before = uni.state_blob().copy(), env.get_state().copy(), frozen(net)
    sb = VecStep(env, uni, net, B, "c51", GAMMA).buf
    rc = L.lib().fb_vec_step_dp(None, env.h, uni.h, net.h, ctypes.byref(sb), N, L.ALGO_C51, B, 0.0, 0, 0, 1, GAMMA, 1, L.current_stream())
    assert rc == -1 and "noisy net" in L.lib().fb_last_error().decode()
    idx = torch.zeros(2 * B, dtype=torch.int64, device="cuda")
    rc = L.lib().fb_train_steps(uni.h, net.h, L.ALGO_C51, B, 1, L.ptr(idx), 1, 1, 1, 1, 1, 1, GAMMA, L.current_stream())
    assert rc == -1 and "noise key" in L.lib().fb_last_error().decode()
    rc = L.lib().fb_vec_step(env.h, uni.h, net.h, ctypes.byref(sb), N, L.ALGO_NATURE, B, 0.0, 0, 0, 1, GAMMA, L.current_stream())
    assert rc == -1 and "C51" in L.lib().fb_last_error().decode()
    for mode in (2, -1):
        assert L.lib().fb_qnet_reset_noise(net.h, 0, 1, 1, mode, L.current_stream()) == -1
    assert L.lib().fb_qnet_reset_noise(net.h, 2, 1, 1, 0, L.current_stream()) == -1
    torch.cuda.synchronize()
    assert np.array_equal(uni.state_blob(), blob) and np.array_equal(env.get_state(), env_state)
    assert same(frozen(net), before)
    plain = QNet(2, FC, "c51", max_batch=8)
    assert L.lib().fb_qnet_is_noisy(plain.h) == 0 and not plain.noisy
    with pytest.raises(ValueError, match="not a noisy net"):
        L.check(L.lib().fb_qnet_reset_noise(plain.h, 0, 1, 1, 0, L.current_stream()), "fb_qnet_reset_noise")
    with pytest.raises(ValueError, match="needs a noisy net"):
        plain.noise(0)


# ---------------------------------------------------------------------------------------------------------------- VecBrain
def test_vecbrain_noisy_rainbow_checkpoints(torch_cuda, tmp_path):
    """VecBrain(algo='c51doubleper', arch='c51dueling', n_step=3, noisy=True): epsilon 0 by default, save / load continues bit for
    bit, noisy and non-noisy checkpoints refuse each other by name; evaluate loads the checkpoint and plays it in mean mode"""
    torch = torch_cuda
    from dqnflappybird_amd.evaluate import qnet_from_checkpoint
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(algo="c51doubleper", arch="c51dueling", batch=32, capacity=20000, observe=6, seed=3, replace_target_iter=4, n_step=3,
              noisy=True, sigma0=0.4)
    a = VecBrain(256, **kw)
    assert a.epsilon == 0.0 and a.net.noisy and a.net.sigma0 == np.float32(0.4)
    assert VecBrain(256, **dict(kw, initial_epsilon=0.02)).epsilon == 0.02          # an explicit epsilon is honoured
    a.run(20, log_every=0)
    assert not torch.equal(a.net.store_params(0), a.net.store_params(1))
    ck = str(tmp_path / "ck")
    a.save(ck)
    z = np.load(ck + ".npz")
    assert int(z["noisy"][0]) == 1 and np.float32(z["sigma0"][0]) == np.float32(0.4) and z["online"].size == a.net.n_params
    ta = []
    for _ in range(10):
        a.step()
        ta.append((a.one_step.actions.clone(), a.one_step.idx.clone(), a.one_step.loss.clone(), a.one_step.abs_err.clone(), a.net.noise(0).clone()))
    b = VecBrain(256, **dict(kw, seed=77))
    b.load(ck)
    b.seed = a.seed
    for i in range(10):
        b.step()
        got = (b.one_step.actions, b.one_step.idx, b.one_step.loss, b.one_step.abs_err, b.net.noise(0))
        assert all(torch.equal(x, y) for x, y in zip(got, ta[i])), i
    assert torch.equal(a.net.store_params(0), b.net.store_params(0)) and torch.equal(a.net.store_params(1), b.net.store_params(1))
    with pytest.raises(ValueError, match="holds a noisy net, this VecBrain has a non-noisy net"):
        VecBrain(256, **dict(kw, noisy=False)).load(ck)
    plain = VecBrain(256, **dict(kw, noisy=False))
    plain.save(str(tmp_path / "plain"))
    with pytest.raises(ValueError, match="holds a non-noisy net, this VecBrain has a noisy net"):
        VecBrain(256, **kw).load(str(tmp_path / "plain"))
    # VecBrain.evaluate plays the mean weights and puts the online noise back
    nz = b.net.noise(0).clone()
    res = b.evaluate(512, max_steps=2000)
    assert (res.length > 0).all() and torch.equal(b.net.noise(0), nz)
    net = qnet_from_checkpoint(ck, max_batch=256)
    assert net.noisy and net.arch == "c51dueling" and net.sigma0 == np.float32(0.4)
    assert torch.equal(net.store_params(0).cpu(), torch.from_numpy(z["online"]))
    assert not bool(net.noise(0).any())
