"""Discrete soft actor-critic on the GPU (include/fbdqn.h: FB_ARCH_SAC; kernels: csrc/fb_sac.hip) against the float64 restatements of
tests/test_sac_host.py, under the bounds the other heads' tests use: Q_ATOL (tests/test_gpu_qnet.py) for logits, Q values and the target,
check_scalar_grads' rtol 2e-3 / atol 2e-5 x the tensor's largest reference element per gradient tensor of the SAC layout on kink-free
batches (tests/kinkfree.py), rtol 1e-4 / atol 1e-6 for the six loss numbers.  Then the exact cases and the compositions, bit for bit:
ring-fed == gathered, fused Adam == export + apply_adam, a clipped step == export + clip + apply, fb_sac_step == its separate calls;
the temperature's Adam step; the refusals; the loop and its checkpoint."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import SAMPLE_SEED, SAMPLE_STEP, nib_pack, np_sample, policy_uniforms, sampling_case
from tests.test_gpu_ac import filled_replay, net_state, same_state
from tests.test_gpu_qnet import Q_ATOL, rand_states, trained_like_params
from tests.test_sac_host import F32, np_alpha_adam, np_softmax32, sac_bounds, sac_forward64, torch_sac_loss

pytestmark = pytest.mark.gpu
SHAPES = [(512, 2), (384, 3), (128, 8)]
MAXB = 700                                   # rows: 3 x 700 >= the 2048 of the sampling case


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def head0(fc):
    return 77984 + 1600 * fc + fc


_params = {}


def sac_params(oracle, fc, A, seed=1):
    """trained-like parameters in the SAC layout: the trunk and W_pi b_pi of tests/test_gpu_ac.py's actor-critic net of that seed (so
    its kink-free pool and tests/test_ac_host.py::sampling_case serve this net too), the two Q heads from two other plain nets' heads.
    Two random heads on a non-negative h differ by a nearly constant offset per column; b_q2 is shifted by the median of Q1 - Q2 over 64
    random states, so that both orders of Q1 and Q2 occur among the samples of a batch (the min in the target and the actor term)"""
    import torch
    if (fc, A, seed) not in _params:
        k = np.float32(np.sqrt(512 / fc))
        d = trained_like_params(oracle, oracle.qcfg(fc, A, True), seed)
        heads = [trained_like_params(oracle, oracle.qcfg(fc, A, False), seed + 10 * i)[head0(fc):] for i in (1, 2)]
        p = np.concatenate([d[:head0(fc)], d[head0(fc) + fc + 1:] * k, heads[0] * k, heads[1] * k]).astype(np.float32)
        lo, hi = sac_bounds(fc, A)[-1][1:]
        assert len(p) == hi
        with torch.no_grad():
            _, q1, q2 = sac_forward64(torch.from_numpy(p.astype(np.float64)), rand_states(np.random.default_rng(fc + A + seed), 64), fc, A)
        p[lo:hi] += (q1 - q2).median(0).values.numpy().astype(np.float32)
        p.setflags(write=False)
        _params[(fc, A, seed)] = p
    return _params[(fc, A, seed)]


_nets, _refs, _grads = {}, {}, {}


def case(oracle, fc, A):
    """one net per shape (gradient-exporting steps leave it as it was): online parameters of seed 1, target parameters of seed 2"""
    from dqnflappybird_amd.vec import QNet
    if (fc, A) not in _nets:
        net, p, pt = QNet(A, fc, "sac", max_batch=MAXB), sac_params(oracle, fc, A, 1), sac_params(oracle, fc, A, 2)
        assert net.n_params == len(p)
        net.load_params(p, 0)
        net.load_params(pt, 1)
        _nets[(fc, A)] = (net, p, pt)
    return _nets[(fc, A)]


def heads64(p, s, fc, A):
    import torch
    with torch.no_grad():
        out = [sac_forward64(torch.from_numpy(p.astype(np.float64)), s[k:k + 256], fc, A) for k in range(0, len(s), 256)]
    return [torch.cat([o[i] for o in out]).numpy() for i in range(3)]


def forward_ref(oracle, fc, A, n=1027):
    """n random states and their float64 heads under the online and the target parameters, once per shape"""
    if (fc, A) not in _refs:
        s = rand_states(np.random.default_rng(7 * fc + A), n)
        _refs[(fc, A)] = (s, heads64(sac_params(oracle, fc, A, 1), s, fc, A), heads64(sac_params(oracle, fc, A, 2), s[:256], fc, A))
    return _refs[(fc, A)]


# ================================================================================================================ forward
@pytest.mark.parametrize("fc,A", SHAPES)
def test_forward_and_acting_forward(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    net, p, pt = case(oracle, fc, A)
    s, on, tg = forward_ref(oracle, fc, A)
    assert all(0.5 < np.abs(x).max() < 100 for x in on)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 5, 255, 256):
        x = sd[:B].contiguous()
        for which, ref in ((0, on), (1, tg)):
            out = net.forward_sac(x, which)
            for name, got, want in zip(("logits", "q1", "q2"), out, ref):
                assert got.shape == (B, A)
                np.testing.assert_allclose(got.cpu().numpy(), want[:B], rtol=0, atol=Q_ATOL, err_msg=f"{name} B={B} net {which}")
            assert torch.equal(net.forward(x, which), out[0]), (B, which)       # fb_qnet_forward: the logits as "Q", the same bits
        assert not torch.equal(out[1], out[2])
    nibd = torch.from_numpy(nib_pack(s)).cuda()
    alpha = net.sac()[0]
    for n in (1, 255, 256, 1027):                                   # both acting forms; 1027: a last trunk workgroup of two states
        nib = nibd[:n].contiguous()
        act, v, logp, z = net.act_policy_nib(nib, seed=3, step=4, want_logits=True)
        np.testing.assert_allclose(z.cpu().numpy(), on[0][:n], rtol=0, atol=Q_ATOL, err_msg=f"logits n={n}")
        # the soft state value from the RETURNED logits and the float64 Q heads: a convex combination of min Q (Q_ATOL) less alpha log p
        # (float32 rounding of a few terms of magnitude <= ~10: 2e-5)
        pz, lpz = np_softmax32(z.cpu().numpy())
        want = (pz.astype(np.float64) * (np.minimum(on[1][:n], on[2][:n]) - alpha * lpz.astype(np.float64))).sum(1)
        dv = np.abs(v.cpu().numpy() - want).max()
        print(f"soft value ({fc}, {A}) n={n}: max |dV| {dv:.3e}")
        assert dv <= Q_ATOL + 2e-5
        a2, _, l2 = net.act_policy_nib(nib, seed=3, step=4, value=None)
        assert torch.equal(a2, act) and torch.equal(l2, logp)
        ga, q = net.act_nib(nib, 0.0, seed=1, step=2, want_q=True)      # fb_qnet_act_nib: greedy play is the policy's argmax
        assert torch.equal(q, z) and np.array_equal(ga.cpu().numpy(), z.cpu().numpy().argmax(1)), n
    assert net.overflow_count() == 0


def test_init_params_are_the_plain_nets_then_distinct_heads(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    sac, plain = QNet(A, fc, "sac", max_batch=8), QNet(A, fc, "plain", max_batch=8)
    sac.init_params(seed=11); plain.init_params(seed=11)
    ps, pp = sac.store_params().cpu().numpy(), plain.store_params().cpu().numpy()
    assert np.array_equal(ps[:len(pp)], pp)                          # trunk, fc1 and W_pi b_pi: the plain net's bits
    b = {n: (lo, hi) for n, lo, hi in sac_bounds(fc, A)}
    w1, w2 = ps[b["W_q1"][0]:b["W_q1"][1]], ps[b["W_q2"][0]:b["W_q2"][1]]
    assert not np.array_equal(w1, w2) and np.abs(w1).max() <= 0.02 + 1e-9 and 0.005 < w1.std() < 0.012 and 0.005 < w2.std() < 0.012
    for n in ("b_q1", "b_q2", "b_pi"):
        assert (ps[b[n][0]:b[n][1]] == np.float32(0.01)).all(), n
    a, h, lr = sac.sac()
    assert abs(a - 0.2) < 1e-7 and abs(h - 0.98 * np.log(A)) < 1e-6 and lr == 0.0
    np.testing.assert_array_equal(sac.sac_state()[1:], np.array([0, 0, 0.9, 0.999], np.float32))


# ================================================================================================================ sampling
@pytest.mark.parametrize("fc,A", SHAPES)
def test_sampling_is_the_documented_draw(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    net, p, pt = case(oracle, fc, A)
    p2, s, z64 = sampling_case(oracle, fc, A)
    assert np.array_equal(p[:head0(fc)], p2[:head0(fc)])             # the actor-critic case's trunk and policy head: its logits
    n = len(s)
    nib = torch.from_numpy(nib_pack(s)).cuda()
    act, v, logp, z = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP, want_logits=True)
    act, logp, z = act.cpu().numpy(), logp.cpu().numpy(), z.cpu().numpy()
    np.testing.assert_allclose(z, z64, rtol=0, atol=Q_ATOL)
    u = policy_uniforms(oracle, n, SAMPLE_SEED, SAMPLE_STEP)
    want, _, dist = np_sample(z, u)                                  # float32 numpy from the RETURNED logits
    skip = dist < 1e-5
    print(f"sampling ({fc}, {A}): {int(skip.sum())} of {n} rows within 1e-5 of a cdf boundary; {int((act != want).sum())} rows differ")
    assert skip.sum() <= 2
    assert np.array_equal(act[~skip], want[~skip])
    z8 = z.astype(np.float64)
    lse = z8.max(1) + np.log(np.exp(z8 - z8.max(1, keepdims=True)).sum(1))
    np.testing.assert_allclose(logp, z8[np.arange(n), act] - lse, rtol=0, atol=1e-6)
    g, _, gl = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP, greedy=True)
    assert np.array_equal(g.cpu().numpy(), z.argmax(1))                # np.argmax: the first maximum
    np.testing.assert_allclose(gl.cpu().numpy(), z8.max(1) - lse, rtol=0, atol=1e-6)


def test_greedy_takes_the_first_of_equal_maxima(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    net, p = QNet(A, fc, "sac", max_batch=64), sac_params(oracle, fc, A).copy()
    b = {n: (lo, hi) for n, lo, hi in sac_bounds(fc, A)}
    w = p[b["W_pi"][0]:b["W_pi"][1]].reshape(fc, A)
    w[:, 1] = w[:, 2]
    w[:, 0] = w[:, 2] - np.float32(0.5)
    p[b["b_pi"][0]:b["b_pi"][1]] = 0.25
    net.load_params(p, 0)
    s = rand_states(np.random.default_rng(5), 40)
    act, _, _, z = net.act_policy_nib(torch.from_numpy(nib_pack(s)).cuda(), greedy=True, want_logits=True)
    z = z.cpu().numpy()
    assert np.array_equal(z[:, 1], z[:, 2]) and (z[:, 1] > z[:, 0]).all() and (act.cpu().numpy() == 1).all()


# ================================================================================================================ train step
GAMMA = 0.99


def ref_step(oracle, fc, A, B):
    """kink-free states s (a prefix of the shape's pool under the online trunk), random s', actions, rewards, terminals, and the float64
    loss numbers, target and gradient of the step at the net's default alpha"""
    import torch
    if (fc, A, B) not in _grads:
        p, ptg = sac_params(oracle, fc, A, 1), sac_params(oracle, fc, A, 2)
        pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
        s = np.array(pool[:B])
        rng = np.random.default_rng(1000 * fc + 10 * A + B)
        s2 = rand_states(rng, B)
        a = rng.integers(0, A, B).astype(np.uint8)
        r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.6, 0.2, 0.2])
        t = (rng.random(B) < 0.25).astype(np.uint8)
        if B > 1:
            t[0], t[1] = 1, 0
        pt = torch.tensor(p.astype(np.float64), requires_grad=True)
        z, q1, q2 = sac_forward64(pt, s, fc, A)
        with torch.no_grad():
            zn = sac_forward64(pt.detach(), s2, fc, A)[0]
            _, q1n, q2n = sac_forward64(torch.from_numpy(ptg.astype(np.float64)), s2, fc, A)
        alpha = float(np.exp(np.log(F32(0.2))))
        out = torch_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, GAMMA, alpha)
        out[0].backward()
        d1 = (q1[torch.arange(B), torch.as_tensor(a.astype(np.int64))] - out[5]).detach().numpy()
        if B >= 32:                                                  # what the issue asks of the case
            assert (d1 > 0).any() and (d1 < 0).any() and t.any() and not t.all()
            for x, y in ((q1, q2), (q1n, q2n)):
                assert (x < y).any() and (x > y).any()
        _grads[(fc, A, B)] = (s, a, r, s2, t, [o.item() for o in out[:5]] + [alpha], out[5].numpy(), pt.grad.numpy())
    return _grads[(fc, A, B)]


def check_sac_grads(g, g0, fc, A):
    """tests/test_gpu_shapes.py::check_scalar_grads' bounds over the SAC layout, every tensor elementwise (kink-free)"""
    for name, lo, hi in sac_bounds(fc, A):
        ref, got = g0[lo:hi], g[lo:hi]
        scale = np.abs(ref).max()
        assert scale > 0, name
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=name)


@pytest.mark.parametrize("B", [1, 32, 255, 256])
@pytest.mark.parametrize("fc,A", SHAPES)
def test_train_step_against_autograd(torch_cuda, oracle, fc, A, B):
    """gathered, gradient-exporting: the six loss numbers, the target and every gradient tensor"""
    torch = torch_cuda
    net, p, ptg = case(oracle, fc, A)
    s, a, r, s2, t, want, y0, g0 = ref_step(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, y = net.sac_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=grad)
    loss, y = loss.cpu().numpy(), y.cpu().numpy()
    print(f"sac ({fc}, {A}) B={B}: loss {loss.tolist()} / {want}; max |dy| {np.abs(y - y0).max():.3e}")
    np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(y, y0, rtol=0, atol=Q_ATOL)
    check_sac_grads(grad.cpu().numpy(), g0, fc, A)
    assert np.array_equal(net.store_params(0).cpu().numpy(), p) and np.array_equal(net.store_params(1).cpu().numpy(), ptg)      # gradient-only mode
    assert net.overflow_count() == 0


def zero_blocks(p, fc, A, names):
    p = p.copy()
    for n, lo, hi in sac_bounds(fc, A):
        if n in names:
            p[lo:hi] = 0
    return p


@pytest.mark.parametrize("fc,A", SHAPES)
def test_exact_cases(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    net, p, ptg = case(oracle, fc, A)
    B = 32
    s, a, r, s2, t, _, _, _ = ref_step(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    tb = {n: (lo, hi) for n, lo, hi in sac_bounds(fc, A)}
    ones = np.ones(B, np.uint8)
    r32 = np.where(r == F32(0.1), 0.1, r.astype(np.float64)).astype(np.float32)
    z = QNet(A, fc, "sac", max_batch=B)
    gz = torch.zeros(z.n_params, dtype=torch.float32, device="cuda")

    def mean32(x):
        acc = F32(0)
        for v in x:
            acc = F32(acc + v)
        return F32(acc / F32(B))

    # all terminal, both Q heads identically 0: y = the reward, d_i = -y, the two critic losses by hand in float32
    z.load_params(zero_blocks(p, fc, A, ("W_q1", "b_q1", "W_q2", "b_q2")), 0)
    z.load_params(ptg, 1)
    loss, y = z.sac_train_step(d(s), d(a), d(r), d(s2), d(ones), gamma=GAMMA, flat_grad=gz)
    loss, y = loss.cpu().numpy(), y.cpu().numpy()
    assert np.array_equal(y, r32)
    d1 = (F32(0) - y).astype(F32)
    assert loss[1] == loss[2] == mean32((d1 * d1).astype(F32))
    # zero policy weights, Q = the biases: a uniform policy, H = ln A, b_pi's gradient in float32 order, bit for bit.  log p and alpha
    # are taken as the device forms them (one logf, one expf): everything else is float32 arithmetic numpy repeats
    pz = zero_blocks(p, fc, A, ("W_pi", "b_pi", "W_q1", "W_q2"))
    rng = np.random.default_rng(A)
    bq1, bq2 = rng.normal(size=A).astype(F32), rng.normal(size=A).astype(F32)
    pz[tb["b_q1"][0]:tb["b_q1"][1]], pz[tb["b_q2"][0]:tb["b_q2"][1]] = bq1, bq2
    z.load_params(pz, 0)
    nib = torch.from_numpy(nib_pack(s[:4])).cuda()
    _, _, lp_dev, zz = z.act_policy_nib(nib, greedy=True, want_logits=True)
    assert not zz.any()
    lp = lp_dev.cpu().numpy()[0]
    np.testing.assert_allclose(lp, -np.log(A), rtol=1e-6)
    loss, _ = z.sac_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=gz)
    loss = loss.cpu().numpy()
    alpha = loss[5]
    np.testing.assert_allclose(loss[4], np.log(A), rtol=1e-6, atol=0)
    s_sum = F32(0)
    for c in range(A):
        s_sum = F32(s_sum + F32(1))
    pc = F32(F32(1) / s_sum)
    f = (F32(alpha * lp) - np.minimum(bq1, bq2)).astype(F32)
    Lpi = F32(0)
    for c in range(A):
        Lpi = F32(Lpi + F32(pc * f[c]))
    dz = (((pc * (f - Lpi).astype(F32)).astype(F32)) / F32(B)).astype(F32)
    want = np.zeros(A, F32)
    for b in range(B):
        want = (want + dz).astype(F32)
    lo, hi = tb["b_pi"]
    assert np.array_equal(gz[lo:hi].cpu().numpy(), want) and np.abs(want).max() > 0
    assert loss[3] == mean32(np.full(B, Lpi, F32))
    # two identical Q heads (both nets): identical gradients for both
    tw = p.copy()
    tw[tb["W_q2"][0]:tb["b_q2"][1]] = tw[tb["W_q1"][0]:tb["b_q1"][1]]
    ttw = ptg.copy()
    ttw[tb["W_q2"][0]:tb["b_q2"][1]] = ttw[tb["W_q1"][0]:tb["b_q1"][1]]
    z.load_params(tw, 0); z.load_params(ttw, 1)
    loss, _ = z.sac_train_step(d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=gz)
    g = gz.cpu().numpy()
    assert loss[1].item() == loss[2].item() > 0
    assert np.array_equal(g[tb["W_q1"][0]:tb["b_q1"][1]], g[tb["W_q2"][0]:tb["b_q2"][1]]) and np.abs(g[tb["W_q1"][0]:tb["W_q1"][1]]).max() > 0
    # doubling alpha on an all-terminal batch (y = the reward): only the actor's terms move
    z.load_params(p, 0); z.load_params(ptg, 1)
    l1, y1 = z.sac_train_step(d(s), d(a), d(r), d(s2), d(ones), gamma=GAMMA, flat_grad=gz)
    g1 = gz.cpu().numpy().copy()
    z.set_sac(alpha=0.4)
    l2, y2 = z.sac_train_step(d(s), d(a), d(r), d(s2), d(ones), gamma=GAMMA, flat_grad=gz)
    g2 = gz.cpu().numpy()
    l1, l2 = l1.cpu().numpy(), l2.cpu().numpy()
    assert torch.equal(y1, y2) and l1[1] == l2[1] and l1[2] == l2[2] and l1[4] == l2[4] and l1[3] != l2[3]
    np.testing.assert_allclose(l2[5], 2 * l1[5], rtol=1e-6)
    lo, hi = tb["W_q1"][0], tb["b_q2"][1]
    assert np.array_equal(g1[lo:hi], g2[lo:hi])
    lo, hi = tb["W_pi"][0], tb["b_pi"][1]
    assert not np.array_equal(g1[lo:hi], g2[lo:hi])


# ================================================================================================================ compositions
def ring_pair(torch, oracle, B, n_nets, lr=1e-4):
    """B transitions of a played memory as ring positions and as gathered tensors, n_nets equal SAC nets (online / target differ)"""
    from dqnflappybird_amd.vec import QNet
    fc, A = 512, 2
    p, ptg = sac_params(oracle, fc, A, 1), sac_params(oracle, fc, A, 2)
    N, pushes = 64, 9
    env, rep, pushed = filled_replay(torch, N, pushes)
    rng = np.random.default_rng(B)
    idx = torch.from_numpy(rng.permutation(N * (pushes - 1))[:B].astype(np.int64)).cuda()
    s, a, r, s2, t = rep.gather(idx)
    nets = []
    for _ in range(n_nets):
        n = QNet(A, fc, "sac", max_batch=256)
        n.load_params(p, 0); n.load_params(ptg, 1)
        n.set_hparams(lr=lr)
        nets.append(n)
    return rep, idx, (s, a, r, s2, t), nets, p


def sac_state_of(net):
    return net_state(net) + (net.sac_state(),)


def same_sac(torch, x, y):
    return same_state(torch, x[:5], y[:5]) and np.array_equal(x[5], y[5])


@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B):
    """loss, target, a / r / t and the exported gradient of fb_sac_train_from_replay == those of fb_replay_gather +
    fb_qnet_sac_train_step, bit for bit; at B = 256 the gathered form takes the per-state trunk (DESIGN.md sections 16 and 18)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import sac_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2)
    g_gath, g_ring = (torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l_gath, y_gath = nets[0].sac_train_step(s, a, r, s2, t, gamma=GAMMA, flat_grad=g_gath)
    l_ring, a_o, r_o, t_o, y_ring = sac_train_from_replay(rep, nets[1], idx, gamma=GAMMA, flat_grad=g_ring, want_target=True)
    assert torch.equal(a_o, a) and torch.equal(r_o, r) and torch.equal(t_o, t) and g_gath.abs().max() > 0
    dl, dg = (l_ring - l_gath).abs().max().item(), (g_ring - g_gath).abs().max().item()
    print(f"ring-fed vs gathered B={B}: max|dloss| {dl:.3e} (loss {l_gath.tolist()}), max|dgrad| {dg:.3e}, "
          f"{int((g_ring != g_gath).sum())} of {g_gath.numel()} gradient elements differ")
    assert torch.equal(l_ring, l_gath) and torch.equal(y_ring, y_gath) and torch.equal(g_ring, g_gath)
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p)    # the exporting ring-fed step left its net alone


@pytest.mark.parametrize("clip", [0.0, 0.05])
@pytest.mark.parametrize("B,ring", [(32, False), (32, True), (256, True)])
def test_fused_adam_equals_export_plus_apply_adam(torch_cuda, oracle, B, ring, clip):
    """parameters, both Adam slots, the beta powers and the temperature words; clip > 0: the fused step of a net with a norm limit ==
    export + clip_grad + apply_adam"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import sac_train_from_replay
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, B, 2)
    for n in nets:
        n.set_max_grad_norm(clip)
    g = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    if ring:
        l0 = sac_train_from_replay(rep, nets[0], idx, gamma=GAMMA, flat_grad=g)[0]
    else:
        l0 = nets[0].sac_train_step(s, a, r, s2, t, gamma=GAMMA, flat_grad=g)[0]
    if clip:
        nets[0].clip_grad(g)
        assert nets[0].grad_norm()[1] < 1.0                          # the limit bites
    nets[0].apply_adam(g)
    l1 = sac_train_from_replay(rep, nets[1], idx, gamma=GAMMA)[0] if ring else nets[1].sac_train_step(s, a, r, s2, t, gamma=GAMMA)[0]
    st = [sac_state_of(n) for n in nets]
    assert torch.equal(l0, l1) and same_sac(torch, st[0], st[1])
    assert not torch.equal(st[0][0], torch.from_numpy(p).cuda())


@pytest.mark.parametrize("N,batch", [(8, 8), (300, 32)])
def test_sac_step_equals_its_separate_calls(torch_cuda, oracle, N, batch):
    """8 steps, with and without train and rho: actions, the six loss numbers, both nets, Adam, the temperature, the envs, the memory"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet, SacStep, VecGameState, VecReplay, sac_train_from_replay
    seed = (3 << 32) | 9
    p = sac_params(oracle, 512, 2)

    def make():
        env, rep, net = VecGameState(N, seed=5), VecReplay(4000, N), QNet(2, 512, "sac", max_batch=max(N, batch))
        net.load_params(p, 0); net.load_params(sac_params(oracle, 512, 2, 2), 1)
        net.set_hparams(lr=1e-4)
        net.set_sac(0.2, None, 1e-3)
        rep.seed(7, "cpython")
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = make()
    e2, r2, n2, nib2 = make()
    steps = {rho: SacStep(e1, r1, n1, batch, GAMMA, rho) for rho in (0.0, 0.01)}
    drawn = set()
    for k, (train, rho) in enumerate([(False, 0.0), (False, 0.01), (True, 0.0), (True, 0.01), (True, 0.01), (False, 0.0), (True, 0.0), (True, 0.01)]):
        one = steps[rho]
        a1 = one(seed=seed, step=k, train=train)
        a2, _, _ = n2.act_policy_nib(nib2, seed=seed, step=k)
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        idx = r2.push_sample(e2.frame_bits, a2, rew, term, batch)
        assert torch.equal(a1, a2) and torch.equal(one.idx, idx) and torch.equal(nib1, nib2), k
        if train:
            loss, a_o, r_o, t_o = sac_train_from_replay(r2, n2, idx, gamma=GAMMA)
            assert torch.equal(one.loss, loss) and torch.equal(one.a, a_o) and torch.equal(one.r, r_o) and torch.equal(one.t, t_o), k
        if rho:
            n2.soft_sync_target(rho)
        assert same_sac(torch, sac_state_of(n1), sac_state_of(n2)), k
        drawn |= set(a1.cpu().tolist())
    assert N < 300 or drawn == {0, 1}
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob())) and len(r1) == 8 * N
    assert n1.sac_state()[0] != np.log(F32(0.2)) and not np.array_equal(n1.store_params(1).cpu().numpy(), sac_params(oracle, 512, 2, 2))


# ================================================================================================================ temperature
def test_temperature_update(torch_cuda, oracle):
    """alpha_lr > 0: five steps of (log alpha, m, v, pow1, pow2) against the float32 restatement of the pinned expression, fed the
    device's own mean H; rtol 1e-6 (ISSUE: printed).  alpha_lr = 0, an exporting step and apply_adam leave the words alone"""
    torch = torch_cuda
    rep, idx, (s, a, r, s2, t), nets, p = ring_pair(torch, oracle, 32, 1)
    net = nets[0]
    hbar, alr = 0.4, 3e-3
    net.set_sac(0.2, hbar, alr)
    st = net.sac_state()
    np.testing.assert_allclose(st[0], np.log(0.2), rtol=1e-6)
    np.testing.assert_array_equal(st[1:], np.array([0, 0, 0.9, 0.999], F32))
    worst = 0.0
    for k in range(5):
        loss, _ = net.sac_train_step(s, a, r, s2, t, gamma=GAMMA)
        loss = loss.cpu().numpy()
        np.testing.assert_allclose(loss[5], np.exp(np.float64(st[0])), rtol=1e-6)          # the alpha the PREVIOUS step left
        st = np_alpha_adam(st, loss[4], hbar, alr)
        got = net.sac_state()
        rel = np.abs(got.astype(np.float64) - st) / np.abs(st)
        worst = max(worst, rel.max())
        print(f"temperature step {k}: device {got.tolist()} / numpy {st.tolist()} / max rel diff {rel.max():.3e}")
        np.testing.assert_allclose(got, st, rtol=1e-6, atol=0)
        st = got
    print(f"temperature: worst relative difference over five steps {worst:.3e}")
    assert net.sac()[0] != 0.2
    g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    net.sac_train_step(s, a, r, s2, t, gamma=GAMMA, flat_grad=g)     # an exporting step ...
    net.apply_adam(g)                                                # ... and apply_adam
    assert np.array_equal(net.sac_state(), st)
    net.set_sac(0.3, hbar, 0.0)
    st0 = net.sac_state()
    net.sac_train_step(s, a, r, s2, t, gamma=GAMMA)
    assert np.array_equal(net.sac_state(), st0) and abs(st0[0] - np.log(0.3)) < 1e-6
    net.set_sac_state(st)
    assert np.array_equal(net.sac_state(), st)


# ================================================================================================================ refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import (ALGOS, AcRolloutStep, QNet, SacStep, TrainSteps, VecReplay, VecStep, ac_train_from_replay,
                                       ppo_train_from_replay, sac_train_from_replay, train_from_replay)
    lib = L.lib()
    N, B = 16, 8
    sac = QNet(2, 128, "sac", max_batch=32)
    sac.load_params(sac_params(oracle, 128, 2), 0)
    env, rep, pushed = filled_replay(torch, N, 12, cap=2000)
    env.track_state()
    rep.seed(9, "cpython")
    blob, before, envs = np.asarray(rep.state_blob()).copy(), sac_state_of(sac), env.get_state().copy()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    s, a, r, s2, t = rep.gather(idx)
    untouched = lambda: (np.array_equal(np.asarray(rep.state_blob()), blob) and same_sac(torch, sac_state_of(sac), before)
                         and np.array_equal(env.get_state(), envs))
    for algo in sorted(ALGOS):                                         # every FB_ALGO_* training entry point
        with pytest.raises(ValueError, match="fb_qnet_train_step: a SAC net trains through"):
            sac.train_step(algo, s, a, r, s2, t, isw=r)
        with pytest.raises(ValueError, match="fb_train_from_replay: a SAC net"):
            train_from_replay(rep, sac, algo, idx, isw=r)
    for algo in ("dqn", "double", "mdqn"):
        with pytest.raises(ValueError, match="fb_train_steps: a SAC net"):
            TrainSteps(rep, sac, B, algo)(1)
        for train in (True, False):
            with pytest.raises(ValueError, match="fb_vec_step: a SAC net"):
                VecStep(env, rep, sac, B, algo)(0.1, train=train)
    buf = VecStep(env, rep, sac, B, "dqn").buf
    assert lib.fb_vec_step_dp(None, env.h, rep.h, sac.h, C.byref(buf), N, 0, B, 0.1, 0, 0, 1, 0.99, 0, None) == -1
    assert "data-parallel SAC is not supported" in lib.fb_last_error().decode()
    adv = torch.zeros(B, dtype=torch.float32, device="cuda")
    for call, msg in ((lambda: sac.set_huber(1.0), "fb_qnet_set_huber"), (lambda: sac.huber(), "fb_qnet_get_huber"),
                      (lambda: sac.set_munchausen(), "fb_qnet_set_munchausen"), (lambda: sac.munchausen(), "fb_qnet_get_munchausen"),
                      (lambda: sac.set_train_dtype("bf16"), "a SAC net trains in FB_DTYPE_F32 only"),
                      (lambda: sac.set_inference_dtype("bf16"), "a SAC net computes in FB_DTYPE_F32 only"),
                      (lambda: sac.set_ac(), "needs an actor-critic net"), (lambda: sac.set_ppo(), "needs an actor-critic net"),
                      (lambda: sac.forward_ac(s), "needs an actor-critic net"), (lambda: sac.ac_train_step(s, a, adv, adv), "needs an actor-critic net"),
                      (lambda: ac_train_from_replay(rep, sac, idx, adv, adv), "needs an actor-critic net"),
                      (lambda: ppo_train_from_replay(rep, sac, idx, adv, adv, adv, adv), "needs an actor-critic net"),
                      (lambda: AcRolloutStep(env, rep, sac, 5), "needs an actor-critic net")):
        with pytest.raises(ValueError, match=msg):
            call()
    loss = torch.zeros(6, dtype=torch.float32, device="cuda")
    a_out = torch.zeros(B, dtype=torch.uint8, device="cuda")
    val = torch.zeros(N, dtype=torch.float32, device="cuda")
    for rc in (lib.fb_qnet_set_ac(sac.h, C.c_float(0.5), C.c_float(0.01)), lib.fb_qnet_set_ppo(sac.h, C.c_float(0.2), C.c_float(0)),
               lib.fb_qnet_forward_ac(sac.h, L.ptr(s), B, L.ptr(loss), L.ptr(val), None),
               lib.fb_qnet_ac_train_step(sac.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(adv), B, L.ptr(loss), None, None),
               lib.fb_qnet_ppo_train_step(sac.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(adv), L.ptr(adv), L.ptr(adv), B, L.ptr(loss), None, None),
               lib.fb_ac_train_from_replay(rep.h, sac.h, B, L.ptr(idx), L.ptr(adv), L.ptr(adv), B, L.ptr(a_out), L.ptr(loss), None, None)):
        assert rc == -1 and "not an actor-critic net" in lib.fb_last_error().decode()
    rb = L.AcRolloutBuffers(*(x.data_ptr() for x in (env.nib, a_out, env.frame_bits, env.reward, env.terminal, env.score, val, val)), 1)
    assert lib.fb_ac_rollout_step(env.h, rep.h, sac.h, C.byref(rb), N, 0, 0, 0, None) == -1
    h = C.c_void_p()
    assert lib.fb_qnet_create(L.ARCH_SAC, 128, 2, 32, C.byref(h)) == -1 and "fb_qnet_create_sac" in lib.fb_last_error().decode()
    assert lib.fb_qnet_create_c51_noisy(L.ARCH_SAC, 128, 2, 51, C.c_float(-10), C.c_float(10), C.c_float(0.5), 32, C.byref(h)) == -1
    for A in (1, 9):
        assert lib.fb_qnet_create_sac(128, A, 32, C.byref(h)) == -1 and "n_actions must be in 2..8" in lib.fb_last_error().decode()
    with pytest.raises(ValueError, match="noisy layers are offered on the C51 heads only"):
        QNet(2, 128, "sac", noisy=True)
    for bad, msg in (((0.0, 0.5, 0.0), "alpha must be finite and > 0"), ((float("nan"), 0.5, 0.0), "alpha must be"), ((0.2, float("inf"), 0.0), "target_entropy"),
                     ((0.2, 0.5, -1.0), "alpha_lr must be finite and >= 0"), ((0.2, 0.5, float("nan")), "alpha_lr")):
        assert lib.fb_qnet_set_sac(sac.h, *(C.c_float(x) for x in bad)) == -1 and msg in lib.fb_last_error().decode()
        with pytest.raises(ValueError, match=msg):
            sac.set_sac(*bad)
    # the training calls' own limits
    r32 = torch.zeros(B, dtype=torch.float32, device="cuda")
    assert lib.fb_qnet_sac_train_step(sac.h, 33, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), 0.99, L.ptr(loss), None, None, None) == -1
    assert "exceeds min(max_batch, 256)" in lib.fb_last_error().decode()
    assert lib.fb_qnet_sac_train_step(sac.h, 0, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), 0.99, L.ptr(loss), None, None, None) == -1
    assert lib.fb_qnet_sac_train_step(sac.h, B, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), 1.5, L.ptr(loss), None, None, None) == -1
    assert "gamma must be in [0, 1]" in lib.fb_last_error().decode()
    rep.set_n_step(3, 0.99)
    with pytest.raises(ValueError, match="3-step view"):
        sac_train_from_replay(rep, sac, idx)
    sb = SacStep(env, rep, sac, B)
    with pytest.raises(ValueError, match="fb_sac_step: the memory has a 3-step view"):
        sb(train=True)
    rep.set_n_step(1, 0.99)
    per = VecReplay(2000, N, prioritized=True)
    with pytest.raises(ValueError, match="uniform memory only"):
        sac_train_from_replay(per, sac, idx)
    assert lib.fb_sac_train_from_replay(per.h, sac.h, B, L.ptr(idx), L.ptr(a_out), L.ptr(r32), L.ptr(a_out), 0.99, L.ptr(loss), None, None, None) == -1
    assert "uniform memory only" in lib.fb_last_error().decode()
    with pytest.raises(ValueError, match="uniform memory only"):
        SacStep(env, per, sac, B)
    assert lib.fb_sac_step(env.h, per.h, sac.h, C.byref(sb.buf), N, B, 0, 0, 1, 0.99, C.c_float(0.0), None) == -1
    assert lib.fb_sac_step(env.h, rep.h, sac.h, C.byref(sb.buf), N, 33, 0, 0, 1, 0.99, C.c_float(0.0), None) == -1
    assert lib.fb_sac_step(env.h, rep.h, sac.h, C.byref(sb.buf), N, B, 0, 0, 1, 0.99, C.c_float(1.5), None) == -1 and "rho must be in [0, 1]" in lib.fb_last_error().decode()
    assert lib.fb_sac_step(env.h, rep.h, sac.h, C.byref(sb.buf), N + 1, B, 0, 0, 1, 0.99, C.c_float(0.0), None) == -1 and "does not match" in lib.fb_last_error().decode()
    assert untouched()
    # ... and the SAC calls refuse every net that is not a SAC net
    w5 = np.zeros(5, np.float32)
    for arch in ("plain", "dueling", "ac", "c51", "qr"):
        q = QNet(2, 128, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        for rc in (lib.fb_qnet_set_sac(q.h, C.c_float(0.2), C.c_float(0.5), C.c_float(0)), lib.fb_qnet_get_sac(q.h, None, None, None),
                   lib.fb_qnet_get_sac_state(q.h, L.ptr(w5)), lib.fb_qnet_set_sac_state(q.h, L.ptr(w5)),
                   lib.fb_qnet_forward_sac(q.h, 0, L.ptr(s), B, L.ptr(val), L.ptr(val), L.ptr(val), None),
                   lib.fb_qnet_sac_train_step(q.h, B, L.ptr(s), L.ptr(a), L.ptr(r32), L.ptr(s2), L.ptr(t), 0.99, L.ptr(loss), None, None, None),
                   lib.fb_sac_train_from_replay(rep.h, q.h, B, L.ptr(idx), L.ptr(a_out), L.ptr(r32), L.ptr(a_out), 0.99, L.ptr(loss), None, None, None),
                   lib.fb_sac_step(env.h, rep.h, q.h, C.byref(sb.buf), N, B, 0, 0, 1, 0.99, C.c_float(0.0), None)):
            assert rc == -1 and "not a SAC net (fb_qnet_create_sac)" in lib.fb_last_error().decode(), arch
        for call in (lambda: q.set_sac(), lambda: q.sac(), lambda: q.sac_state(), lambda: q.forward_sac(s), lambda: q.sac_train_step(s, a, r, s2, t),
                     lambda: sac_train_from_replay(rep, q, idx), lambda: SacStep(env, rep, q, B)):
            with pytest.raises(ValueError, match="needs a SAC net"):
                call()
        assert same_state(torch, net_state(q), qb) and untouched(), arch
    ac = QNet(2, 128, "ac", max_batch=32)                             # an actor-critic net still needs `value`
    assert lib.fb_qnet_act_policy_nib(ac.h, L.ptr(env.nib), N, 0, 0, 0, L.ptr(a_out), None, None, None, None) == -1


# ================================================================================================================ the loop
def run_steps(n, **kw):
    from dqnflappybird_amd.vecsac import VecSAC
    sac = VecSAC(16, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, alpha_lr=1e-3, max_grad_norm=5.0, **kw)
    losses = [sac.step().clone() for _ in range(n)]
    return sac, losses


def loop_state(sac):
    return (sac_state_of(sac.net), sac.env.get_state(), sac.nib.clone(), sac.stats.clone(), np.asarray(sac.replay.state_blob()).copy(), sac.timeStep)


def same_loop(torch, x, y):
    return (same_sac(torch, x[0], y[0]) and np.array_equal(x[1], y[1]) and torch.equal(x[2], y[2]) and torch.equal(x[3], y[3])
            and np.array_equal(x[4], y[4]) and x[5] == y[5])


def test_vec_sac_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain
    from dqnflappybird_amd.vecsac import VecSAC
    sac, losses = run_steps(6)
    assert not losses[1].any() and all(torch.isfinite(l).all() for l in losses) and losses[5][1] > 0       # two observing steps, then training
    assert abs(losses[2][4].item() - np.log(2)) < 1e-2                # a fresh policy is near uniform: H ~ ln 2
    assert sac.timeStep == 6 and len(sac.replay) == 6 * 16 and sac.net.sac()[0] != 0.2
    assert not torch.equal(sac.net.store_params(0), sac.net.store_params(1))
    st = loop_state(sac)
    res = sac.evaluate(n_envs=32, episodes=1, max_steps=200)          # evaluate() leaves the training state untouched
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(sac), st)
    # save -> load -> four more steps == ten steps straight
    path = str(tmp_path / "sac.npz")
    sac.save(path)
    assert str(np.load(path)["head"][0]) == "sac"
    with pytest.raises(ValueError, match="was written with seed 4"):
        VecSAC(16, batch=8, fc_width=128, seed=123, capacity=2000).load(path)
    with pytest.raises(ValueError, match="n_envs, batch, fc_width"):
        VecSAC(32, batch=8, fc_width=128, seed=4, capacity=2000).load(path)
    resumed = VecSAC(16, batch=8, fc_width=128, observe=2, seed=4, capacity=2000, lr=3e-5)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and resumed.net.sac()[2] == float(F32(1e-3))
    more = [resumed.step().clone() for _ in range(4)]
    straight, l10 = run_steps(10)
    assert all(torch.equal(x, y) for x, y in zip(more, l10[6:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    # the three loops refuse each other's files; evaluate.py plays a sac checkpoint
    with pytest.raises(ValueError, match="holds a sac head"):
        VecBrain(16, observe=0, capacity=2000).load(path)
    with pytest.raises(ValueError, match="holds a sac head"):
        VecActorCritic(16, rollout=2).load(path)
    vb = str(tmp_path / "dqn.npz")
    VecBrain(16, observe=0, capacity=2000).save(vb)
    with pytest.raises(ValueError, match="this is a VecSAC"):
        resumed.load(vb)
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path, fc_width=128)
    assert net.arch == "sac" and torch.equal(net.store_params(), sac.net.store_params())
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    sac.run(1, log_every=1)
