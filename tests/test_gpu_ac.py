"""Advantage actor-critic on the GPU (include/fbdqn.h: FB_ARCH_AC; kernels: csrc/fb_ac.hip) against the float64 restatements of
tests/test_ac_host.py, under the bounds the scalar heads' tests use: Q_ATOL (tests/test_gpu_qnet.py) for logits and V,
check_scalar_grads (tests/test_gpu_shapes.py) per gradient tensor on kink-free batches (tests/kinkfree.py), rtol 1e-4 / atol 1e-6 for
the four loss numbers.  The loss is smooth in every head output it reads: nothing is masked, nothing widened.  Then the compositions,
bit for bit: ring-fed == gathered, fused Adam == export + apply_adam, fb_ac_rollout_step == its three calls; the refusals; the loop."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import (SAMPLE_SEED, SAMPLE_STEP, ac_forward64, nib_pack, np_gae, np_sample, policy_uniforms, sampling_case,
                                torch_ac_terms)
from tests.test_gpu_qnet import Q_ATOL, rand_states, trained_like_params
from tests.test_gpu_shapes import check_scalar_grads
from tests.test_oracle_qnet import tensor_bounds

pytestmark = pytest.mark.gpu
SHAPES = [(128, 1), (512, 2), (384, 3), (128, 8)]
COEFS = [(0.5, 0.01), (0.0, 0.0), (1.0, 0.5)]
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


def ac_params(oracle, fc, A, seed=1):
    """trained-like parameters in the dueling layout (weights x 3, the head scaled by sqrt(512 / FC) more: tests/test_gpu_shapes.py)"""
    p = trained_like_params(oracle, oracle.qcfg(fc, A, True), seed)
    p[head0(fc):] *= np.float32(np.sqrt(512 / fc))
    return p


_nets, _refs = {}, {}


def case(oracle, fc, A):
    """one net per shape (gradient-exporting steps leave it as it was) and its parameters"""
    from dqnflappybird_amd.vec import QNet
    if (fc, A) not in _nets:
        net, p = QNet(A, fc, "ac", max_batch=MAXB), ac_params(oracle, fc, A)
        assert net.n_params == len(p) == tensor_bounds(fc, A, "dueling")[-1][2]
        net.load_params(p, 0)
        _nets[(fc, A)] = (net, p)
    return _nets[(fc, A)]


def forward_ref(oracle, fc, A, n=1027):
    """n random states and their float64 logits / values, once per shape"""
    import torch
    if (fc, A) not in _refs:
        p = ac_params(oracle, fc, A)
        s = rand_states(np.random.default_rng(7 * fc + A), n)
        with torch.no_grad():
            out = [ac_forward64(torch.from_numpy(p.astype(np.float64)), s[k:k + 256], fc, A) for k in range(0, n, 256)]
        _refs[(fc, A)] = (s, torch.cat([o[0] for o in out]).numpy(), torch.cat([o[1] for o in out]).numpy())
    return _refs[(fc, A)]


def net_state(net):
    m, v, pows = net.adam_state()
    return net.store_params(0).clone(), net.store_params(1).clone(), m.clone(), v.clone(), np.array(pows)


def same_state(torch, x, y):
    return all(torch.equal(a, b) for a, b in zip(x[:4], y[:4])) and np.array_equal(x[4], y[4])


# ================================================================================================================ forward
@pytest.mark.parametrize("fc,A", SHAPES)
def test_forward_and_acting_forward(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    net, p = case(oracle, fc, A)
    s, z0, v0 = forward_ref(oracle, fc, A)
    assert 0.5 < np.abs(z0).max() < 100 and 0.5 < np.abs(v0).max() < 100
    sd = torch.from_numpy(s).cuda()
    for B in (1, 5, 255, 256):
        x = sd[:B].contiguous()
        z, v = net.forward_ac(x)
        assert z.shape == (B, A) and v.shape == (B,)
        np.testing.assert_allclose(z.cpu().numpy(), z0[:B], rtol=0, atol=Q_ATOL, err_msg=f"logits B={B}")
        np.testing.assert_allclose(v.cpu().numpy(), v0[:B], rtol=0, atol=Q_ATOL, err_msg=f"V B={B}")
        assert torch.equal(net.forward(x), z), B                     # fb_qnet_forward: the logits as "Q", the same bits
    nibd = torch.from_numpy(nib_pack(s)).cuda()
    for n in (1, 255, 256, 1027):                                   # both acting forms; 1027: a last trunk workgroup of two states
        nib = nibd[:n].contiguous()
        act, v, logp, z = net.act_policy_nib(nib, seed=3, step=4, want_logits=True)
        np.testing.assert_allclose(z.cpu().numpy(), z0[:n], rtol=0, atol=Q_ATOL, err_msg=f"logits n={n}")
        np.testing.assert_allclose(v.cpu().numpy(), v0[:n], rtol=0, atol=Q_ATOL, err_msg=f"V n={n}")
        only_v = net.act_policy_nib(nib, value_only=True)
        assert torch.equal(only_v, v), n
        ga, q = net.act_nib(nib, 0.0, seed=1, step=2, want_q=True)      # fb_qnet_act_nib: greedy play is the policy's argmax
        assert torch.equal(q, z) and np.array_equal(ga.cpu().numpy(), z.cpu().numpy().argmax(1)), n
    assert net.overflow_count() == 0


# ================================================================================================================ sampling
@pytest.mark.parametrize("fc,A", [(512, 2), (384, 3), (128, 8)])
def test_sampling_is_the_documented_draw(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    net, p = case(oracle, fc, A)
    p2, s, z64 = sampling_case(oracle, fc, A)
    assert np.array_equal(p, p2)
    n = len(s)
    nib = torch.from_numpy(nib_pack(s)).cuda()
    act, v, logp, z = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP, want_logits=True)
    act, logp, z = act.cpu().numpy(), logp.cpu().numpy(), z.cpu().numpy()
    np.testing.assert_allclose(z, z64, rtol=0, atol=Q_ATOL)
    u = policy_uniforms(oracle, n, SAMPLE_SEED, SAMPLE_STEP)
    want, _, dist = np_sample(z, u)                                  # float32 numpy from the RETURNED logits
    skip = dist < 1e-5
    print(f"sampling ({fc}, {A}): {int(skip.sum())} of {n} rows within 1e-5 of a cdf boundary; "
          f"{int((act != want).sum())} rows differ; actions drawn {sorted(set(act.tolist()))}")
    assert skip.sum() <= 2
    assert np.array_equal(act[~skip], want[~skip])
    z8 = z.astype(np.float64)
    lse = z8.max(1) + np.log(np.exp(z8 - z8.max(1, keepdims=True)).sum(1))
    np.testing.assert_allclose(logp, z8[np.arange(n), act] - lse, rtol=0, atol=1e-6)
    again = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP)
    assert np.array_equal(again[0].cpu().numpy(), act) and np.array_equal(again[2].cpu().numpy(), logp)
    other = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP + 1)[0].cpu().numpy()
    u2 = policy_uniforms(oracle, n, SAMPLE_SEED, SAMPLE_STEP + 1)
    w2, _, d2 = np_sample(z, u2)
    assert not np.array_equal(other, act) and np.array_equal(other[d2 >= 1e-5], w2[d2 >= 1e-5])
    g, _, gl = net.act_policy_nib(nib, seed=SAMPLE_SEED, step=SAMPLE_STEP, greedy=True)
    assert np.array_equal(g.cpu().numpy(), z.argmax(1))                # np.argmax: the first maximum
    np.testing.assert_allclose(gl.cpu().numpy(), z8.max(1) - lse, rtol=0, atol=1e-6)


def test_one_action_always_draws_action_0(torch_cuda, oracle):
    torch = torch_cuda
    net, p = case(oracle, 128, 1)
    s, _, _ = forward_ref(oracle, 128, 1)
    for n in (37, 300):
        nib = torch.from_numpy(nib_pack(s[:n])).cuda()
        for greedy in (False, True):
            act, v, logp = net.act_policy_nib(nib, seed=5, step=6, greedy=greedy)
            assert not act.any() and not logp.any()


def test_greedy_takes_the_first_of_equal_maxima(torch_cuda, oracle):
    """equal columns of W_pi and equal biases: equal logits in columns 1 and 2 bit for bit, above column 0: the argmax is 1, the first of the two"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A = 128, 3
    net, p = QNet(A, fc, "ac", max_batch=64), ac_params(oracle, fc, A).copy()
    b = {n: (lo, hi) for n, lo, hi in tensor_bounds(fc, A, "dueling")}
    w = p[b["W_q"][0]:b["W_q"][1]].reshape(fc, A)
    w[:, 1] = w[:, 2]
    w[:, 0] = w[:, 2] - np.float32(0.5)
    p[b["b_q"][0]:b["b_q"][1]] = 0.25
    net.load_params(p, 0)
    s, _, _ = forward_ref(oracle, 128, 1)
    nib = torch.from_numpy(nib_pack(s[:40])).cuda()
    act, _, _, z = net.act_policy_nib(nib, greedy=True, want_logits=True)
    z = z.cpu().numpy()
    assert np.array_equal(z[:, 1], z[:, 2]) and (z[:, 1] > z[:, 0]).all() and (act.cpu().numpy() == 1).all()


# ================================================================================================================ GAE
@pytest.mark.parametrize("T,N", [(1, 1), (5, 7), (16, 1027), (128, 64)])
def test_gae_is_np_gae_bit_for_bit(torch_cuda, T, N):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_gae
    rng = np.random.default_rng(T * 10000 + N)
    r = rng.choice(np.array([0.1, 3, -3, 0.75, -1.3], np.float32), (T, N), p=[0.6, 0.1, 0.1, 0.1, 0.1])
    term = (rng.random((T, N)) < 0.15).astype(np.uint8)
    term[0, :] = rng.integers(0, 2, N)                              # terminals in the first ...
    term[T - 1, :] = rng.integers(0, 2, N)                          # ... and the last slot
    term[0, 0] = term[T - 1, 0] = 1
    r[0, 0] = np.float32(0.1)
    v = (rng.normal(size=(T + 1, N)) * 3).astype(np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    for lam in (0.0, 0.95, 1.0):
        for gamma in (0.99, 1.0):
            adv, ret = ac_gae(d(r), d(term), d(v), gamma, lam)
            a0, r0 = np_gae(r, term, v, gamma, lam)
            assert np.array_equal(adv.cpu().numpy(), a0), (lam, gamma)
            assert np.array_equal(ret.cpu().numpy(), r0), (lam, gamma)
    for bad in (dict(gamma=1.5), dict(gae_lambda=-0.1)):
        with pytest.raises(ValueError):
            ac_gae(d(r), d(term), d(v), **bad)
    with pytest.raises(ValueError, match="value must be float32"):
        ac_gae(d(r), d(term), d(v[:T]))


# ================================================================================================================ train step
_grads = {}


def ref_terms(oracle, fc, A, B):
    """kink-free states (a prefix of the shape's pool), the batch's targets, and the float64 gradients of sum L_pi, sum L_v, sum H:
    the loss is (L_pi + c_v L_v - c_e H) / n_total, LINEAR in the three, so every (c_v, c_e, n_total) of a batch shares them"""
    import torch
    if (fc, A, B) not in _grads:
        p = ac_params(oracle, fc, A)
        pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
        s = np.array(pool[:B])
        rng = np.random.default_rng(1000 * fc + 10 * A + B)
        a = rng.integers(0, A, B).astype(np.uint8)
        adv = (rng.normal(size=B) * 2).astype(np.float32)            # both signs
        if B > 1:
            adv[0], adv[1] = abs(adv[0]), -abs(adv[1])
        pt = torch.tensor(p.astype(np.float64), requires_grad=True)
        z, V = ac_forward64(pt, s, fc, A)
        ret = (V.detach().numpy() + rng.normal(size=B)).astype(np.float32)
        terms = torch_ac_terms(z, V, a, adv, ret)
        g = [torch.autograd.grad(t, pt, retain_graph=True, allow_unused=True)[0] for t in terms]
        g = [np.zeros(len(p)) if x is None else x.numpy() for x in g]
        _grads[(fc, A, B)] = (s, a, adv, ret, [t.item() for t in terms], g)
    return _grads[(fc, A, B)]


def check_ac_grads(g, g0, fc, A, cv):
    """tests/test_gpu_shapes.py::check_scalar_grads on the dueling layout, every tensor elementwise (kink-free).  c_v = 0: the value
    stream has no gradient at all, on both sides; with A = 1 as well (no policy gradient either) the whole gradient is exactly 0"""
    if cv == 0.0:
        for name, lo, hi in tensor_bounds(fc, A, "dueling"):
            if name in ("W_v", "b_v") or A == 1:
                assert not g0[lo:hi].any() and not g[lo:hi].any(), name
        if A == 1:
            return
    check_scalar_grads(g, g0, fc, A, True, True, value_free=cv == 0.0)


@pytest.mark.parametrize("B", [1, 32, 255, 256])
@pytest.mark.parametrize("fc,A", SHAPES)
def test_train_step_against_autograd(torch_cuda, oracle, fc, A, B):
    """gathered, gradient-exporting: the four loss numbers and every gradient tensor, n_total in {B, 4B}, the three (c_v, c_e)"""
    torch = torch_cuda
    net, p = case(oracle, fc, A)
    s, a, adv, ret, terms, g3 = ref_terms(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    sd, ad, advd, retd = d(s), d(a), d(adv), d(ret)
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    try:
        for cv, ce in COEFS:
            net.set_ac(cv, ce)
            assert net.ac() == (cv, float(np.float32(ce)))
            cv32, ce32 = float(np.float32(cv)), float(np.float32(ce))
            for nt in (B, 4 * B):
                loss = net.ac_train_step(sd, ad, advd, retd, n_total=nt, flat_grad=grad).cpu().numpy()
                parts = np.array(terms) / nt
                want = np.array([parts[0] + cv32 * parts[1] - ce32 * parts[2], *parts])
                g0 = (g3[0] + cv32 * g3[1] - ce32 * g3[2]) / nt
                print(f"a2c ({fc}, {A}) B={B} nt={nt} cv={cv} ce={ce}: loss {loss.tolist()} / {want.tolist()}")
                np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
                check_ac_grads(grad.cpu().numpy(), g0, fc, A, cv)
    finally:
        net.set_ac()
    assert np.array_equal(net.store_params().cpu().numpy(), p)        # gradient-only mode
    assert net.overflow_count() == 0


@pytest.mark.parametrize("fc,A", SHAPES)
def test_exact_cases(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    net, p = case(oracle, fc, A)
    B = 32
    s, a, adv, ret, _, _ = ref_terms(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    tb = {n: (lo, hi) for n, lo, hi in tensor_bounds(fc, A, "dueling")}
    # adv = 0, c_v = c_e = 0: nothing to learn from
    net.set_ac(0.0, 0.0)
    loss = net.ac_train_step(d(s), d(a), d(np.zeros(B, np.float32)), d(ret), n_total=B, flat_grad=grad)
    assert not grad.any() and loss[0].item() == 0.0 and loss[1].item() == 0.0
    # n_total x 2^k scales the loss and the gradient exactly
    net.set_ac(1.0, 0.5)
    l1 = net.ac_train_step(d(s), d(a), d(adv), d(ret), n_total=B, flat_grad=grad).clone()
    g1 = grad.clone()
    l8 = net.ac_train_step(d(s), d(a), d(adv), d(ret), n_total=8 * B, flat_grad=grad)
    assert torch.equal(l8 * 8, l1) and torch.equal(grad * 8, g1) and g1.abs().max() > 0
    net.set_ac()
    # zero head weights and biases: uniform policy, H = log A, b_pi's gradient = sum_b (1/A - onehot) adv_b / n_total in float32, in order
    z = QNet(A, fc, "ac", max_batch=B)
    pz = p.copy()
    pz[head0(fc):] = 0
    z.load_params(pz, 0)
    z.set_ac(0.5, 0.0)
    gz = torch.zeros(z.n_params, dtype=torch.float32, device="cuda")
    nt = 4 * B
    lz = z.ac_train_step(d(s), d(a), d(adv), d(ret), n_total=nt, flat_grad=gz).cpu().numpy()
    np.testing.assert_allclose(lz[3], B * np.log(A) / nt, rtol=1e-6, atol=0)
    np.testing.assert_allclose(lz[1], np.log(A) * adv.astype(np.float64).sum() / nt, rtol=1e-5, atol=1e-7)
    pc = np.float32(1) / np.float32(A) if A > 1 else np.float32(1)    # e_c / sum e = 1 / A in float32
    want = np.zeros(A, np.float32)
    for b in range(B):
        for c in range(A):
            want[c] += (adv[b] * (pc - np.float32(c == a[b]))) / np.float32(nt)
    lo, hi = tb["b_q"]
    assert np.array_equal(gz[lo:hi].cpu().numpy(), want)
    lo, hi = tb["W_q"]
    if A > 1:
        assert gz[lo:hi].abs().max() > 0


# ================================================================================================================ compositions
def filled_replay(torch, N, pushes, seed=3, cap=None):
    from dqnflappybird_amd.vec import VecGameState, VecReplay
    env, rep = VecGameState(N, seed=seed), VecReplay(cap or 4000, N)
    env.observe(); rep.reset(env.frame_bits)
    g = torch.Generator(device="cpu").manual_seed(N + pushes)
    acts = []
    for _ in range(pushes):
        a = (torch.rand(N, generator=g) < 0.3).to(torch.uint8).cuda()
        env.frame_step(a, want_u8=False)
        rep.push(env.frame_bits, a, env.reward, env.terminal)
        acts.append(a.cpu().numpy())
    return env, rep, np.concatenate(acts)


def ring_pair(torch, oracle, B, n_nets):
    """B transitions of a played memory as ring positions and as gathered tensors, advantages / returns for them, n_nets equal nets"""
    from dqnflappybird_amd.vec import QNet
    fc, A = 512, 2
    p = ac_params(oracle, fc, A)
    N, pushes = 64, 9
    env, rep, pushed = filled_replay(torch, N, pushes)
    assert len(rep) == N * pushes
    rng = np.random.default_rng(B)
    idx = torch.from_numpy(rng.permutation(N * pushes)[:B].astype(np.int64)).cuda()
    adv = torch.from_numpy((rng.normal(size=B) * 2).astype(np.float32)).cuda()
    ret = torch.from_numpy(rng.normal(size=B).astype(np.float32)).cuda()
    s, a, _, _, _ = rep.gather(idx)
    assert np.array_equal(a.cpu().numpy(), pushed[idx.cpu().numpy()])
    nets = []
    for _ in range(n_nets):
        n = QNet(A, fc, "ac", max_batch=256)
        n.load_params(p, 0)
        n.set_hparams(lr=1e-4)
        nets.append(n)
    return rep, idx, s, a, adv, ret, nets, p


def ring_and_gathered(torch, oracle, B):
    from dqnflappybird_amd.vec import ac_train_from_replay
    rep, idx, s, a, adv, ret, nets, p = ring_pair(torch, oracle, B, 2)
    g_gath, g_ring = (torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l_gath = nets[0].ac_train_step(s, a, adv, ret, n_total=2 * B, flat_grad=g_gath)
    l_ring, a_out = ac_train_from_replay(rep, nets[1], idx, adv, ret, n_total=2 * B, flat_grad=g_ring)
    assert torch.equal(a_out, a) and g_gath.abs().max() > 0          # a_out == the pushed actions (ring_pair: a is pushed[idx])
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p)    # the exporting ring-fed step left its net alone
    dl, dg = (l_ring - l_gath).abs().max().item(), (g_ring - g_gath).abs().max().item()
    print(f"ring-fed vs gathered B={B}: max|dloss| {dl:.3e} (loss {l_gath.tolist()}), max|dgrad| {dg:.3e} (max|grad| {g_gath.abs().max().item():.3e}), "
          f"{int((g_ring != g_gath).sum())} of {g_gath.numel()} gradient elements differ")
    return l_gath, l_ring, g_gath, g_ring


@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B):
    """the loss and the exported gradient of fb_ac_train_from_replay == those of fb_replay_gather + fb_qnet_ac_train_step, bit for bit.
    At B = 256 too: a gathered actor-critic batch of 256 takes the per-state conv trunk the ring-fed form computes, not the large-batch
    trunk of the other heads, which sums conv2 / conv3 in another order (measured before that routing: loss apart by 7.5e-8, the
    gradient by 2.0e-6 at a largest element of 2.1, in 476 083 of its 899 235 elements)"""
    torch = torch_cuda
    l_gath, l_ring, g_gath, g_ring = ring_and_gathered(torch, oracle, B)
    assert torch.equal(l_ring, l_gath) and torch.equal(g_ring, g_gath)


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("B", [32, 256])
def test_fused_adam_equals_export_plus_apply_adam(torch_cuda, oracle, B, ring):
    """parameters, both Adam slots and the beta powers, gathered and ring-fed"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_train_from_replay
    rep, idx, s, a, adv, ret, nets, p = ring_pair(torch, oracle, B, 2)
    g = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    if ring:
        l0, _ = ac_train_from_replay(rep, nets[0], idx, adv, ret, n_total=2 * B, flat_grad=g)
        nets[0].apply_adam(g)
        l1, _ = ac_train_from_replay(rep, nets[1], idx, adv, ret, n_total=2 * B)
    else:
        l0 = nets[0].ac_train_step(s, a, adv, ret, n_total=2 * B, flat_grad=g)
        nets[0].apply_adam(g)
        l1 = nets[1].ac_train_step(s, a, adv, ret, n_total=2 * B)
    st = [net_state(n) for n in nets]
    assert torch.equal(l0, l1) and same_state(torch, st[0], st[1])
    assert not torch.equal(st[0][0], torch.from_numpy(p).cuda())


def test_two_chunks_sum_to_the_gradient_of_the_whole(torch_cuda, oracle):
    """512 samples as two exported chunks of 256 with n_total = 512: their sum against the float64 gradient of the whole batch.  The
    second chunk is plain random states (not kink-free): check_scalar_grads' bounds for such a batch"""
    import torch as th
    torch = torch_cuda
    fc, A = 512, 2
    net, p = case(oracle, fc, A)
    s1, a1, adv1, ret1, _, _ = ref_terms(oracle, fc, A, 256)
    rng = np.random.default_rng(99)
    s2 = rand_states(rng, 256)
    a2 = rng.integers(0, A, 256).astype(np.uint8)
    adv2, ret2 = (rng.normal(size=256) * 2).astype(np.float32), rng.normal(size=256).astype(np.float32)
    s, a, adv, ret = np.concatenate([s1, s2]), np.concatenate([a1, a2]), np.concatenate([adv1, adv2]), np.concatenate([ret1, ret2])
    pt = th.tensor(p.astype(np.float64), requires_grad=True)
    cv, ce = net.ac()
    tot = 0.0
    for k in (0, 256):
        z, V = ac_forward64(pt, s[k:k + 256], fc, A)
        lpi, lv, H = torch_ac_terms(z, V, a[k:k + 256], adv[k:k + 256], ret[k:k + 256])
        part = (lpi + cv * lv - ce * H) / 512
        part.backward()
        tot += part.item()
    d = lambda x: torch.from_numpy(x).cuda()
    g, gsum, lsum = torch.zeros(net.n_params, dtype=torch.float32, device="cuda"), 0, 0
    for k in (0, 256):
        l = net.ac_train_step(d(s[k:k + 256]), d(a[k:k + 256]), d(adv[k:k + 256]), d(ret[k:k + 256]), n_total=512, flat_grad=g)
        gsum, lsum = gsum + g, lsum + l
    np.testing.assert_allclose(lsum[0].item(), tot, rtol=1e-4, atol=1e-6)
    check_scalar_grads(gsum.cpu().numpy(), pt.grad.numpy(), fc, A, True, False)


@pytest.mark.parametrize("N", [8, 300])
def test_rollout_step_equals_its_three_calls(torch_cuda, oracle, N):
    """12 steps (two rollouts of 6): actions, value, logp, reward, terminal per step, the env states and the replay blob at the end"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import AcRolloutStep, QNet, VecGameState, VecReplay
    T, seed = 6, (3 << 32) | 9
    p = ac_params(oracle, 512, 2)

    def make():
        env, rep, net = VecGameState(N, seed=5), VecReplay(N * (T + 2), N), QNet(2, 512, "ac", max_batch=N)
        net.load_params(p, 0)
        nib = env.track_state(); env.observe(); rep.reset(env.frame_bits)
        return env, rep, net, nib

    e1, r1, n1, nib1 = make()
    e2, r2, n2, nib2 = make()
    roll = AcRolloutStep(e1, r1, n1, T)
    val = torch.zeros((T, N), dtype=torch.float32, device="cuda")
    lgp = torch.zeros((T, N), dtype=torch.float32, device="cuda")
    drawn = set()
    for k in range(12):
        slot = k % T
        a1 = roll(slot, seed=seed, step=k)
        a2, _, _ = n2.act_policy_nib(nib2, seed=seed, step=k, value=val[slot], logp=lgp[slot])
        _, rew, term, _ = e2.frame_step(a2, want_u8=False)
        r2.push(e2.frame_bits, a2, rew, term)
        assert torch.equal(a1, a2) and torch.equal(roll.value[slot], val[slot]) and torch.equal(roll.logp[slot], lgp[slot]), k
        assert torch.equal(roll.reward[slot], rew) and torch.equal(roll.terminal[slot], term), k
        assert torch.equal(nib1, nib2), k
        drawn |= set(a1.cpu().tolist())
    assert N < 300 or drawn == {0, 1}
    assert np.array_equal(e1.get_state(), e2.get_state())
    assert np.array_equal(np.asarray(r1.state_blob()), np.asarray(r2.state_blob())) and len(r1) == min(12 * N, N * (T + 2))
    with pytest.raises(ValueError, match="slot 6 outside"):
        roll(T)


# ================================================================================================================ refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import (ALGOS, AcRolloutStep, QNet, TrainSteps, VecGameState, VecReplay, VecStep, ac_train_from_replay,
                                       train_from_replay)
    lib = L.lib()
    N, B = 16, 8
    ac = QNet(2, 128, "ac", max_batch=32)
    ac.load_params(ac_params(oracle, 128, 2), 0)
    env, rep, pushed = filled_replay(torch, N, 12, cap=2000)
    env.track_state()
    rep.seed(9, "cpython")
    blob, before, envs = np.asarray(rep.state_blob()).copy(), net_state(ac), env.get_state().copy()
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    s, a, r, s2, t = rep.gather(idx)
    untouched = lambda: (np.array_equal(np.asarray(rep.state_blob()), blob) and same_state(torch, net_state(ac), before)
                         and np.array_equal(env.get_state(), envs))
    for algo in sorted(ALGOS):                                         # every existing training algo, every training entry point
        with pytest.raises(ValueError, match="an actor-critic net trains through"):
            ac.train_step(algo, s, a, r, s2, t, isw=r)
        with pytest.raises(ValueError, match="fb_train_from_replay: an actor-critic net"):
            train_from_replay(rep, ac, algo, idx, isw=r)
    for algo in ("dqn", "double", "mdqn"):
        with pytest.raises(ValueError, match="fb_train_steps: an actor-critic net"):
            TrainSteps(rep, ac, B, algo)(1)
        with pytest.raises(ValueError, match="fb_vec_step: an actor-critic net"):
            VecStep(env, rep, ac, B, algo)(0.1, train=True)
        with pytest.raises(ValueError, match="fb_vec_step: an actor-critic net"):
            VecStep(env, rep, ac, B, algo)(0.1, train=False)
    buf = VecStep(env, rep, ac, B, "dqn").buf
    assert lib.fb_vec_step_dp(None, env.h, rep.h, ac.h, C.byref(buf), N, 0, B, 0.1, 0, 0, 1, 0.99, 0, None) == -1
    assert "data-parallel A2C is not supported" in lib.fb_last_error().decode()
    for call, msg in ((lambda: ac.set_huber(1.0), "fb_qnet_set_huber"), (lambda: ac.huber(), "fb_qnet_get_huber"),
                      (lambda: ac.set_munchausen(), "fb_qnet_set_munchausen"), (lambda: ac.munchausen(), "fb_qnet_get_munchausen"),
                      (lambda: ac.set_train_dtype("bf16"), "trains in FB_DTYPE_F32 only"),
                      (lambda: ac.set_inference_dtype("bf16"), "computes in FB_DTYPE_F32 only")):
        with pytest.raises(ValueError, match=msg):
            call()
    ac.set_train_dtype("f32"); ac.set_inference_dtype("f32")
    h = C.c_void_p()
    assert lib.fb_qnet_create(L.ARCH_AC, 128, 2, 32, C.byref(h)) == -1 and "fb_qnet_create_ac" in lib.fb_last_error().decode()
    assert lib.fb_qnet_create_c51_noisy(L.ARCH_AC, 128, 2, 51, C.c_float(-10), C.c_float(10), C.c_float(0.5), 32, C.byref(h)) == -1
    with pytest.raises(ValueError, match="noisy layers are offered on the C51 heads only"):
        QNet(2, 128, "ac", noisy=True)
    for bad in ((-1.0, 0.01), (float("nan"), 0.01), (0.5, float("inf")), (0.5, -0.0001)):
        assert lib.fb_qnet_set_ac(ac.h, C.c_float(bad[0]), C.c_float(bad[1])) == -1 and "finite and >= 0" in lib.fb_last_error().decode()
        with pytest.raises(ValueError):
            ac.set_ac(*bad)
    assert ac.ac() == (0.5, float(np.float32(0.01)))
    adv = torch.zeros(B, dtype=torch.float32, device="cuda")
    loss = torch.zeros(4, dtype=torch.float32, device="cuda")
    a_out = torch.zeros(B, dtype=torch.uint8, device="cuda")
    # the training calls' own limits
    assert lib.fb_qnet_ac_train_step(ac.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(adv), B - 1, L.ptr(loss), None, None) == -1
    assert "n_total" in lib.fb_last_error().decode()
    assert lib.fb_qnet_ac_train_step(ac.h, 33, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(adv), 64, L.ptr(loss), None, None) == -1
    assert "exceeds min(max_batch, 256)" in lib.fb_last_error().decode()
    assert lib.fb_ac_train_from_replay(rep.h, ac.h, B, L.ptr(idx), L.ptr(adv), L.ptr(adv), B - 1, L.ptr(a_out), L.ptr(loss), None, None) == -1
    rep.set_n_step(3, 0.99)
    with pytest.raises(ValueError, match="3-step view"):
        ac_train_from_replay(rep, ac, idx, adv, adv)
    rep.set_n_step(1, 0.99)
    per = VecReplay(2000, N, prioritized=True)
    with pytest.raises(ValueError, match="uniform memory only"):
        ac_train_from_replay(per, ac, idx, adv, adv)
    assert lib.fb_ac_train_from_replay(per.h, ac.h, B, L.ptr(idx), L.ptr(adv), L.ptr(adv), B, L.ptr(a_out), L.ptr(loss), None, None) == -1
    assert "uniform memory only" in lib.fb_last_error().decode()
    with pytest.raises(ValueError, match="uniform memory only"):
        AcRolloutStep(env, per, ac, 5)
    assert untouched()
    # ... and the new calls refuse every net that is not an actor-critic net
    for arch in ("plain", "dueling", "c51", "qr"):
        q = QNet(2, 128, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        nib = env.nib
        val = torch.zeros(N, dtype=torch.float32, device="cuda")
        for rc in (lib.fb_qnet_set_ac(q.h, C.c_float(0.5), C.c_float(0.01)), lib.fb_qnet_get_ac(q.h, None, None),
                   lib.fb_qnet_forward_ac(q.h, L.ptr(s), B, L.ptr(loss), L.ptr(val), None),
                   lib.fb_qnet_act_policy_nib(q.h, L.ptr(nib), N, 0, 0, 0, L.ptr(a_out), L.ptr(val), None, None, None),
                   lib.fb_qnet_ac_train_step(q.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(adv), B, L.ptr(loss), None, None),
                   lib.fb_ac_train_from_replay(rep.h, q.h, B, L.ptr(idx), L.ptr(adv), L.ptr(adv), B, L.ptr(a_out), L.ptr(loss), None, None)):
            assert rc == -1 and "not an actor-critic net (fb_qnet_create_ac)" in lib.fb_last_error().decode(), arch
        rb = L.AcRolloutBuffers(*(x.data_ptr() for x in (nib, a_out, env.frame_bits, env.reward, env.terminal, env.score, val, val)), 1)
        assert lib.fb_ac_rollout_step(env.h, rep.h, q.h, C.byref(rb), N, 0, 0, 0, None) == -1
        assert "not an actor-critic net" in lib.fb_last_error().decode()
        for call in (lambda: q.set_ac(), lambda: q.forward_ac(s), lambda: q.act_policy_nib(nib), lambda: q.ac_train_step(s, a, adv, adv),
                     lambda: ac_train_from_replay(rep, q, idx, adv, adv), lambda: AcRolloutStep(env, rep, q, 5)):
            with pytest.raises(ValueError, match="needs an actor-critic net"):
                call()
        assert same_state(torch, net_state(q), qb) and untouched(), arch
    with pytest.raises(ValueError, match="n_envs 16 does not match|does not match the env"):
        small = VecGameState(8, seed=1)
        small.track_state(); small.observe()
        AcRolloutStep(small, rep, ac, 5)(0)
    assert untouched()


# ================================================================================================================ the loop
def run_updates(torch, n, **kw):
    from dqnflappybird_amd.vecac import VecActorCritic
    ac = VecActorCritic(64, rollout=5, seed=4, **kw)
    losses = [ac.update().clone() for _ in range(n)]
    return ac, losses


def loop_state(ac):
    return (net_state(ac.net) + (ac.env.get_state(),), ac.nib.clone(), ac.stats.clone(), np.asarray(ac.replay.state_blob()).copy(),
            (ac.timeStep, ac.updates, ac.pushes))


def same_loop(torch, x, y):
    return (same_state(torch, x[0][:5], y[0][:5]) and np.array_equal(x[0][5], y[0][5]) and torch.equal(x[1], y[1]) and torch.equal(x[2], y[2])
            and np.array_equal(x[3], y[3]) and x[4] == y[4])


def test_vec_actor_critic_loop(torch_cuda, tmp_path):
    torch = torch_cuda
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain
    ac, losses = run_updates(torch, 3, max_grad_norm=5.0)
    p0 = VecActorCritic(64, rollout=5, seed=4).net.store_params()
    assert all(torch.isfinite(l).all() for l in losses) and not torch.equal(ac.net.store_params(), p0)
    assert ac.timeStep == 15 and ac.updates == 3 and len(ac.replay) == min(15 * 64, ac.capacity) == 7 * 64
    assert abs(losses[0][3].item() - np.log(2)) < 1e-2                # a fresh policy is near uniform: H ~ log 2
    norm, scale = ac.net.grad_norm()
    assert norm > 0 and 0 < scale <= 1
    again, l2 = run_updates(torch, 3, max_grad_norm=5.0)              # a rerun from the same seed is identical
    assert all(torch.equal(x, y) for x, y in zip(losses, l2)) and same_loop(torch, loop_state(ac), loop_state(again))
    # evaluate() leaves the training state untouched
    st = loop_state(ac)
    res = ac.evaluate(n_envs=32, episodes=1, max_steps=200)
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(ac), st)
    # save -> load -> two more updates == five updates straight
    path = str(tmp_path / "a2c.npz")
    ac.save(path)
    assert str(np.load(path)["head"][0]) == "ac"
    with pytest.raises(ValueError, match="was written with seed 4"):
        VecActorCritic(64, rollout=5, seed=123).load(path)
    resumed = VecActorCritic(64, rollout=5, seed=4, lr=3e-5)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), st) and resumed.max_grad_norm == 5.0 and resumed.net.max_grad_norm == 5.0
    more = [resumed.update().clone() for _ in range(2)]
    straight, l5 = run_updates(torch, 5, max_grad_norm=5.0)
    assert all(torch.equal(x, y) for x, y in zip(more, l5[3:])) and same_loop(torch, loop_state(resumed), loop_state(straight))
    # the two loops refuse each other's files; evaluate.py plays an ac checkpoint
    with pytest.raises(ValueError, match="holds an ac head"):
        VecBrain(16, observe=0, capacity=2000).load(path)
    vb = str(tmp_path / "dqn.npz")
    VecBrain(16, observe=0, capacity=2000).save(vb)
    with pytest.raises(ValueError, match="this is a VecActorCritic"):
        resumed.load(vb)
    with pytest.raises(ValueError, match="n_envs, rollout, fc_width"):
        VecActorCritic(32, rollout=5).load(path)
    from dqnflappybird_amd.evaluate import evaluate, qnet_from_checkpoint
    net = qnet_from_checkpoint(path)
    assert net.arch == "ac" and torch.equal(net.store_params(), ac.net.store_params())
    r2 = evaluate(net, 32, 1, 200)
    assert np.array_equal(r2.score, res.score) and np.array_equal(r2.length, res.length)
    ac.run(1, log_every=1)
