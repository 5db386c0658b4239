"""PPO on the GPU (include/fbdqn.h: fb_qnet_ppo_train_step and its block; kernels: csrc/fb_ac.hip) against the float64 restatements of
tests/test_ppo_host.py, under A2C's own bounds: rtol 1e-4 / atol 1e-6 for the six loss numbers, check_scalar_grads
(tests/test_gpu_shapes.py) per gradient tensor on kink-free states (tests/kinkfree.py).  The loss is smooth away from the clip edges,
and ppo_targets places every sample clear of them on the float64 forward alone: nothing is masked, nothing widened.  Then the exact
cases, the compositions bit for bit, the two small kernels against their numpy restatements bit for bit, A2C's bits beside a PPO step,
the refusals and the loop."""
import ctypes as C

import numpy as np
import pytest

from tests import kinkfree
from tests.test_ac_host import ac_forward64
from tests.test_gpu_ac import ac_params, case, filled_replay, loop_state, net_state, ref_terms, ring_pair, same_loop, same_state
from tests.test_gpu_qnet import rand_states
from tests.test_gpu_shapes import check_scalar_grads
from tests.test_ppo_host import np_normalize, np_permute, ppo_targets, torch_ppo_terms

pytestmark = pytest.mark.gpu
SHAPES = [(512, 2), (128, 8), (128, 1)]
COEFS = [(0.5, 0.01), (1.0, 0.5)]
EPS, VCLIPS = 0.2, (0.0, 0.2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


# ================================================================================================================ against float64 autograd
_refs = {}


def ppo_ref(oracle, fc, A, B):
    """kink-free states (a prefix of the shape's pool), targets clear of the clip edges, and per value_clip the five float64 sums with
    the gradients of sum L_pi, sum L_v, sum H: the loss is (L_pi + c_v L_v - c_e H) / n_total, LINEAR in the three"""
    import torch
    if (fc, A, B) not in _refs:
        p = ac_params(oracle, fc, A)
        pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
        s = np.array(pool[:B])
        pt = torch.tensor(p.astype(np.float64), requires_grad=True)
        z, V = ac_forward64(pt, s, fc, A)
        tg = ppo_targets(z.detach().numpy(), V.detach().numpy(), np.random.default_rng(2000 * fc + 10 * A + B), EPS, VCLIPS[1])
        grad = lambda t: torch.autograd.grad(t, pt, retain_graph=True, allow_unused=True)[0]
        host = lambda g: np.zeros(len(p)) if g is None else g.numpy()
        out, shared = {}, None
        for vclip in VCLIPS:
            lpi, lv, H, nclip, kl = torch_ppo_terms(z, V, *tg, EPS, vclip)
            shared = shared or (host(grad(lpi)), host(grad(H)))          # (neither depends on value_clip)
            out[vclip] = ([lpi.item(), lv.item(), H.item(), nclip, kl], [shared[0], host(grad(lv)), shared[1]])
        _refs[(fc, A, B)] = (s,) + tg + (out,)
    return _refs[(fc, A, B)]


def want_loss(sums, nt, cv32, ce32):
    parts = np.array(sums) / nt
    return np.array([parts[0] + cv32 * parts[1] - ce32 * parts[2], *parts])


@pytest.mark.parametrize("B", [1, 33, 256])
@pytest.mark.parametrize("fc,A", SHAPES)
def test_train_step_against_autograd(torch_cuda, oracle, fc, A, B):
    """gathered, gradient-exporting: the six loss numbers and every gradient tensor, value_clip off and on, the two (c_v, c_e)"""
    torch = torch_cuda
    net, p = case(oracle, fc, A)
    s, a, adv, ret, lpo, vo, refs = ppo_ref(oracle, fc, A, B)
    if B >= 10:
        assert all({np.sign(x) for x in adv[k::5]} == {1.0, -1.0} for k in range(5))      # both advantage signs at every ratio
    d = lambda x: torch.from_numpy(x).cuda()
    args = [d(x) for x in (s, a, adv, ret, lpo, vo)]
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    nt = 2 * B
    try:
        for vclip in VCLIPS:
            net.set_ppo(EPS, vclip)
            assert net.ppo() == (float(np.float32(EPS)), float(np.float32(vclip)))
            sums, g3 = refs[vclip]
            for cv, ce in COEFS:
                net.set_ac(cv, ce)
                cv32, ce32 = float(np.float32(cv)), float(np.float32(ce))
                loss = net.ppo_train_step(*args, n_total=nt, flat_grad=grad).cpu().numpy()
                want = want_loss(sums, nt, cv32, ce32)
                print(f"ppo ({fc}, {A}) B={B} value_clip={vclip} cv={cv} ce={ce}: loss {loss.tolist()} / {want.tolist()}")
                assert loss.shape == (6,)
                np.testing.assert_allclose(loss, want, rtol=1e-4, atol=1e-6)
                check_scalar_grads(grad.cpu().numpy(), (g3[0] + cv32 * g3[1] - ce32 * g3[2]) / nt, fc, A, True, True)
    finally:
        net.set_ac()
        net.set_ppo()
    assert np.array_equal(net.store_params().cpu().numpy(), p)        # gradient-only mode
    assert net.overflow_count() == 0


# ================================================================================================================ exact cases
@pytest.mark.parametrize("fc,A", [(512, 2), (128, 8)])
def test_exact_cases(torch_cuda, oracle, fc, A):
    torch = torch_cuda
    net, p = case(oracle, fc, A)
    B = 33
    s, a, adv, ret, lpo, vo, _ = ppo_ref(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    try:
        # every ratio at 2 (log p_a differs from the reference's by the forward's 1e-4 at most) with adv > 0: clipped and flat.  With
        # c_v = c_e = 0 nothing is left to learn from; the policy term is -(1 + eps) adv, summed in float32 in sample order
        lp2 = (lpo.astype(np.float64) + np.log(np.array([(0.5, 0.85, 1.0, 1.15, 2.0)[b % 5] for b in range(B)])) - np.log(2.0)).astype(np.float32)
        pos = np.abs(adv)
        net.set_ac(0.0, 0.0)
        net.set_ppo(EPS, 0.2)
        nt = 4 * B
        loss = net.ppo_train_step(d(s), d(a), d(pos), d(ret), d(lp2), d(vo), n_total=nt, flat_grad=grad).cpu().numpy()
        assert not grad.any()
        assert loss[4] == np.float32(B) / np.float32(nt)
        hi, t = np.float32(1.0) + np.float32(EPS), np.float32(0.0)
        for b in range(B):
            t = t + -(hi * pos[b])
        assert loss[1] == t / np.float32(nt) and loss[0] == loss[1]
        # n_total x 8 scales the loss and the gradient by exactly 1 / 8
        net.set_ac(1.0, 0.5)
        l1 = net.ppo_train_step(d(s), d(a), d(adv), d(ret), d(lpo), d(vo), n_total=B, flat_grad=grad).clone()
        g1 = grad.clone()
        l8 = net.ppo_train_step(d(s), d(a), d(adv), d(ret), d(lpo), d(vo), n_total=8 * B, flat_grad=grad)
        assert torch.equal(l8 * 8, l1) and torch.equal(grad * 8, g1) and g1.abs().max() > 0 and l1[4] > 0
        # an action past the head reads the last one
        far = a.copy()
        far[a == A - 1] = 200
        far[0] = 255
        last = a.copy()
        last[0] = A - 1
        lf = net.ppo_train_step(d(s), d(far), d(adv), d(ret), d(lpo), d(vo), n_total=B, flat_grad=grad).clone()
        gf = grad.clone()
        ll = net.ppo_train_step(d(s), d(last), d(adv), d(ret), d(lpo), d(vo), n_total=B, flat_grad=grad)
        assert (far >= A).sum() >= 2 and torch.equal(lf, ll) and torch.equal(gf, grad) and torch.isfinite(gf).all()
    finally:
        net.set_ac()
        net.set_ppo()
    assert np.array_equal(net.store_params().cpu().numpy(), p)


# ================================================================================================================ compositions
def ppo_pair(torch, oracle, B, n_nets):
    """tests/test_gpu_ac.py::ring_pair with the rollout's log-probabilities and values beside it, on nets that clip the value too"""
    rep, idx, s, a, adv, ret, nets, p = ring_pair(torch, oracle, B, n_nets)
    rng = np.random.default_rng(50 + B)
    lpo = torch.from_numpy((np.log(0.5) + 0.3 * rng.normal(size=B)).astype(np.float32)).cuda()
    vo = ret + torch.from_numpy((0.3 * rng.normal(size=B)).astype(np.float32)).cuda()
    for n in nets:
        n.set_ppo(EPS, 0.2)
    return rep, idx, s, a, adv, ret, lpo, vo, nets, p


@pytest.mark.parametrize("B", [32, 256])
def test_ring_fed_equals_gathered(torch_cuda, oracle, B):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ppo_train_from_replay
    rep, idx, s, a, adv, ret, lpo, vo, nets, p = ppo_pair(torch, oracle, B, 2)
    g_gath, g_ring = (torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l_gath = nets[0].ppo_train_step(s, a, adv, ret, lpo, vo, n_total=2 * B, flat_grad=g_gath)
    l_ring, a_out = ppo_train_from_replay(rep, nets[1], idx, adv, ret, lpo, vo, n_total=2 * B, flat_grad=g_ring)
    assert torch.equal(a_out, a) and g_gath.abs().max() > 0 and 0 < l_gath[4].item() < 0.5      # some ratios clipped, not all
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p)
    assert torch.equal(l_ring, l_gath) and torch.equal(g_ring, g_gath)


@pytest.mark.parametrize("B", [32, 256])
def test_sel_reads_the_rollout_buffers_in_place(torch_cuda, oracle, B):
    """sel = a slice of a permutation over buffers of 3 B + 7 == the pre-gathered buffers with sel NULL"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import ppo_train_from_replay
    rep, idx, s, a, adv, ret, lpo, vo, nets, p = ppo_pair(torch, oracle, B, 1)
    n = 3 * B + 7
    gen = torch.Generator(device="cpu").manual_seed(B)
    sel = torch.randperm(n, generator=gen)[:B].cuda()
    assert sel.max().item() >= B and sel.dtype == torch.int64
    long = []
    for x in (adv, ret, lpo, vo):
        buf = torch.randn(n, generator=gen).cuda() * 3                # (what no sample selects is never read into the result)
        buf[sel] = x
        long.append(buf)
    g0, g1 = (torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(2))
    l0, a0 = ppo_train_from_replay(rep, nets[0], idx, adv, ret, lpo, vo, n_total=B, flat_grad=g0)
    l1, a1 = ppo_train_from_replay(rep, nets[0], idx, *long, sel=sel, n_total=B, flat_grad=g1)
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(a0, a1) and g0.abs().max() > 0
    for bad in (n, -1):                                               # a position outside the buffers is refused on the host, before any launch
        wrong = sel.clone()
        wrong[B // 2] = bad
        with pytest.raises(ValueError, match=f"sel must lie in 0..{n - 1}"):
            ppo_train_from_replay(rep, nets[0], idx, *long, sel=wrong, n_total=B, flat_grad=g1)
    assert torch.equal(g0, g1) and np.array_equal(nets[0].store_params().cpu().numpy(), p)
    with pytest.raises(ValueError, match="sel must be int64"):
        ppo_train_from_replay(rep, nets[0], idx, *long, sel=sel[:B - 1], n_total=B, flat_grad=g1)
    with pytest.raises(ValueError, match="value_old must be a contiguous float32"):
        ppo_train_from_replay(rep, nets[0], idx, *long[:3], vo, sel=sel, n_total=B, flat_grad=g1)


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("B", [32, 256])
def test_fused_adam_equals_export_plus_apply_adam(torch_cuda, oracle, B, ring):
    """parameters, both Adam slots and the beta powers, gathered and ring-fed"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import ppo_train_from_replay
    rep, idx, s, a, adv, ret, lpo, vo, nets, p = ppo_pair(torch, oracle, B, 2)
    g = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    if ring:
        l0, _ = ppo_train_from_replay(rep, nets[0], idx, adv, ret, lpo, vo, n_total=2 * B, flat_grad=g)
        nets[0].apply_adam(g)
        l1, _ = ppo_train_from_replay(rep, nets[1], idx, adv, ret, lpo, vo, n_total=2 * B)
    else:
        l0 = nets[0].ppo_train_step(s, a, adv, ret, lpo, vo, n_total=2 * B, flat_grad=g)
        nets[0].apply_adam(g)
        l1 = nets[1].ppo_train_step(s, a, adv, ret, lpo, vo, n_total=2 * B)
    st = [net_state(n) for n in nets]
    assert torch.equal(l0, l1) and same_state(torch, st[0], st[1])
    assert not torch.equal(st[0][0], torch.from_numpy(p).cuda())


@pytest.mark.parametrize("B", [32, 256])
def test_two_chunks_sum_to_the_whole(torch_cuda, oracle, B):
    """2 B samples as two exported chunks of B with n_total = 2 B: the summed loss and gradient against float64 of the whole.  At B = 32
    all 64 states are kink-free; at B = 256 the second chunk is plain random states (the pool holds 256): check_scalar_grads' bounds
    for such a batch, as in A2C's test.  The targets are clear of the clip edges on the float64 forward in both"""
    import torch as th
    torch = torch_cuda
    fc, A = 512, 2
    net, p = case(oracle, fc, A)
    pool, _ = kinkfree.pool(oracle, p, fc, seed=fc)
    kink_free = 2 * B <= len(pool)
    s = np.array(pool[:2 * B]) if kink_free else np.concatenate([np.array(pool[:B]), rand_states(np.random.default_rng(98), B)])
    pt = th.tensor(p.astype(np.float64), requires_grad=True)
    with th.no_grad():
        fw = [ac_forward64(pt, s[k:k + B], fc, A) for k in (0, B)]
    z64, V64 = th.cat([f[0] for f in fw]).numpy(), th.cat([f[1] for f in fw]).numpy()
    tg = ppo_targets(z64, V64, np.random.default_rng(77 + B), EPS, 0.2)
    cv, ce = net.ac()
    sums = np.zeros(5)
    for k in (0, B):
        z, V = ac_forward64(pt, s[k:k + B], fc, A)
        lpi, lv, H, nclip, kl = torch_ppo_terms(z, V, *(x[k:k + B] for x in tg), EPS, 0.2)
        ((lpi + cv * lv - ce * H) / (2 * B)).backward()
        sums += [lpi.item(), lv.item(), H.item(), nclip, kl]
    d = lambda x: torch.from_numpy(x).cuda()
    g, gsum, lsum = torch.zeros(net.n_params, dtype=torch.float32, device="cuda"), 0, 0
    try:
        net.set_ppo(EPS, 0.2)
        for k in (0, B):
            l = net.ppo_train_step(d(s[k:k + B]), *(d(x[k:k + B]) for x in tg), n_total=2 * B, flat_grad=g)
            gsum, lsum = gsum + g, lsum + l
    finally:
        net.set_ppo()
    want = want_loss(sums, 2 * B, cv, ce)
    print(f"two chunks of {B}: loss {lsum.tolist()} / {want.tolist()}")
    np.testing.assert_allclose(lsum.cpu().numpy(), want, rtol=1e-4, atol=1e-6)
    check_scalar_grads(gsum.cpu().numpy(), pt.grad.numpy(), fc, A, True, kink_free)


# ================================================================================================================ the two small kernels
@pytest.mark.parametrize("n", [1, 2, 5, 256, 257, 5120])
def test_permute_is_np_permute_bit_for_bit(torch_cuda, oracle, n):
    from dqnflappybird_amd.vec import ac_permute
    for seed, draw in (((7 << 32) | 12345, (1 << 32) + 3), (0, 0), (4, 17)):
        got = ac_permute(n, seed, draw)
        assert got.dtype == torch_cuda.int64 and got.shape == (n,)
        assert np.array_equal(got.cpu().numpy(), np_permute(oracle, n, seed, draw)), (seed, draw)
    out = torch_cuda.full((n,), -1, dtype=torch_cuda.int64, device="cuda")
    assert ac_permute(n, 4, 17, out=out) is out and sorted(out.cpu().tolist()) == list(range(n))


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5120])
def test_normalize_adv_is_np_normalize_bit_for_bit(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_normalize_adv
    x = (np.random.default_rng(n).normal(size=n) * 3 + 1.5).astype(np.float32)
    want = np_normalize(x)
    xd = torch.from_numpy(x).cuda()
    got = ac_normalize_adv(xd)
    assert np.array_equal(xd.cpu().numpy(), x) and np.array_equal(got.cpu().numpy(), want)
    assert ac_normalize_adv(xd, out=xd) is xd and np.array_equal(xd.cpu().numpy(), want)           # in place
    two_d = torch.from_numpy(x[:n - n % 5].reshape(-1, 5) if n >= 5 else x.reshape(1, 1)).cuda()
    assert ac_normalize_adv(two_d).shape == two_d.shape
    const = torch.full((n,), 2.5, dtype=torch.float32, device="cuda")
    assert not ac_normalize_adv(const).any()


# ================================================================================================================ A2C untouched
def test_a2c_bits_do_not_change_beside_a_ppo_step(torch_cuda, oracle):
    """one A2C chunk (512, 2), B = 256 through ac_train_step before and after a PPO step on the same net: the same loss and gradient
    bits, and those of a net that never saw PPO.  Settings do not leak"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import QNet
    fc, A, B = 512, 2, 256
    p = ac_params(oracle, fc, A)
    s, a, adv, ret, _, _ = ref_terms(oracle, fc, A, B)
    d = lambda x: torch.from_numpy(x).cuda()
    nets = []
    for _ in range(2):
        n = QNet(A, fc, "ac", max_batch=B)
        n.load_params(p, 0)
        nets.append(n)
    g = [torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda") for _ in range(4)]
    before = nets[0].ac_train_step(d(s), d(a), d(adv), d(ret), n_total=2 * B, flat_grad=g[0]).clone()
    nets[0].set_ppo(0.1, 0.3)
    lp = nets[0].ppo_train_step(d(s), d(a), d(adv), d(ret), d(np.full(B, np.log(0.5), np.float32)), d(ret), n_total=2 * B, flat_grad=g[1])
    after = nets[0].ac_train_step(d(s), d(a), d(adv), d(ret), n_total=2 * B, flat_grad=g[2])
    other = nets[1].ac_train_step(d(s), d(a), d(adv), d(ret), n_total=2 * B, flat_grad=g[3])
    assert before.shape == (4,) and lp.shape == (6,) and not torch.equal(g[0], g[1])
    assert torch.equal(before, after) and torch.equal(g[0], g[2]) and torch.equal(before, other) and torch.equal(g[0], g[3])
    assert nets[0].ac() == nets[1].ac() and nets[1].ppo() == (float(np.float32(0.2)), 0.0)


# ================================================================================================================ refusals
def test_refusals_leave_everything_as_it_was(torch_cuda, oracle):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecReplay, ppo_train_from_replay
    lib = L.lib()
    N, B = 16, 8
    ac = QNet(2, 128, "ac", max_batch=32)
    ac.load_params(ac_params(oracle, 128, 2), 0)
    env, rep, _ = filled_replay(torch, N, 12, cap=2000)
    blob, before = np.asarray(rep.state_blob()).copy(), net_state(ac)
    untouched = lambda: np.array_equal(np.asarray(rep.state_blob()), blob) and same_state(torch, net_state(ac), before)
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    s, a, _, _, _ = rep.gather(idx)
    x = torch.zeros(B, dtype=torch.float32, device="cuda")
    loss = torch.zeros(6, dtype=torch.float32, device="cuda")
    a_out = torch.zeros(B, dtype=torch.uint8, device="cuda")
    err = lambda: lib.fb_last_error().decode()
    # bad settings
    for bad in ((0.0, 0.0), (-0.2, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.2, -0.5), (0.2, float("nan")), (0.2, float("inf"))):
        assert lib.fb_qnet_set_ppo(ac.h, C.c_float(bad[0]), C.c_float(bad[1])) == -1 and "must be finite" in err()
        with pytest.raises(ValueError, match="must be finite"):
            ac.set_ppo(*bad)
    assert ac.ppo() == (float(np.float32(0.2)), 0.0)
    # NULL arguments, the batch and n_total rules
    full = [L.ptr(t) for t in (s, a, x, x, x, x)]
    for k in range(6):
        args = list(full)
        args[k] = None
        assert lib.fb_qnet_ppo_train_step(ac.h, B, *args, B, L.ptr(loss), None, None) == -1 and "NULL argument" in err(), k
    assert lib.fb_qnet_ppo_train_step(ac.h, B, *full, B, None, None, None) == -1 and "NULL argument" in err()
    assert lib.fb_qnet_ppo_train_step(None, B, *full, B, L.ptr(loss), None, None) == -1
    assert lib.fb_qnet_ppo_train_step(ac.h, B, *full, B - 1, L.ptr(loss), None, None) == -1 and "n_total" in err()
    assert lib.fb_qnet_ppo_train_step(ac.h, 33, *full, 64, L.ptr(loss), None, None) == -1 and "exceeds min(max_batch, 256)" in err()
    assert lib.fb_qnet_ppo_train_step(ac.h, 0, *full, 64, L.ptr(loss), None, None) == -1
    ring = [L.ptr(t) for t in (idx, None, x, x, x, x)]
    for k in (0, 2, 3, 4, 5):
        args = list(ring)
        args[k] = None
        assert lib.fb_ppo_train_from_replay(rep.h, ac.h, B, *args, B, L.ptr(a_out), L.ptr(loss), None, None) == -1 and "NULL argument" in err(), k
    assert lib.fb_ppo_train_from_replay(rep.h, ac.h, B, *ring, B, None, L.ptr(loss), None, None) == -1 and "NULL argument" in err()
    assert lib.fb_ppo_train_from_replay(None, ac.h, B, *ring, B, L.ptr(a_out), L.ptr(loss), None, None) == -1
    assert lib.fb_ppo_train_from_replay(rep.h, ac.h, B, *ring, B - 1, L.ptr(a_out), L.ptr(loss), None, None) == -1 and "n_total" in err()
    assert lib.fb_ac_normalize_adv(L.ptr(x), 0, L.ptr(x), None) == -1 and lib.fb_ac_normalize_adv(None, B, L.ptr(x), None) == -1
    assert lib.fb_ac_permute(0, 0, 0, L.ptr(idx), None) == -1 and lib.fb_ac_permute(1 << 31, 0, 0, L.ptr(idx), None) == -1
    assert lib.fb_ac_permute(B, 0, 0, None, None) == -1
    # an n-step or a prioritized memory
    rep.set_n_step(3, 0.99)
    with pytest.raises(ValueError, match="3-step view"):
        ppo_train_from_replay(rep, ac, idx, x, x, x, x)
    rep.set_n_step(1, 0.99)
    per = VecReplay(2000, N, prioritized=True)
    with pytest.raises(ValueError, match="uniform memory only"):
        ppo_train_from_replay(per, ac, idx, x, x, x, x)
    assert lib.fb_ppo_train_from_replay(per.h, ac.h, B, *ring, B, L.ptr(a_out), L.ptr(loss), None, None) == -1 and "uniform memory only" in err()
    assert untouched() and not loss.any() and torch.equal(idx, torch.arange(B, device="cuda"))
    # every PPO entry point refuses a net that is not an actor-critic net
    for arch in ("plain", "dueling", "c51", "qr"):
        q = QNet(2, 128, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        for rc in (lib.fb_qnet_set_ppo(q.h, C.c_float(0.2), C.c_float(0.0)), lib.fb_qnet_get_ppo(q.h, None, None),
                   lib.fb_qnet_ppo_train_step(q.h, B, *full, B, L.ptr(loss), None, None),
                   lib.fb_ppo_train_from_replay(rep.h, q.h, B, *ring, B, L.ptr(a_out), L.ptr(loss), None, None)):
            assert rc == -1 and "not an actor-critic net (fb_qnet_create_ac)" in err(), arch
        for call in (lambda: q.set_ppo(), lambda: q.ppo(), lambda: q.ppo_train_step(s, a, x, x, x, x),
                     lambda: ppo_train_from_replay(rep, q, idx, x, x, x, x)):
            with pytest.raises(ValueError, match="needs an actor-critic net"):
                call()
        assert same_state(torch, net_state(q), qb) and untouched(), arch


# ================================================================================================================ the loop
def make_ppo(**kw):
    from dqnflappybird_amd.vecac import VecActorCritic
    return VecActorCritic(16, rollout=4, algo="ppo", epochs=2, minibatches=2, seed=4, **kw)


def test_vec_actor_critic_ppo_loop(torch_cuda, tmp_path, capsys):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ppo_train_from_replay
    from dqnflappybird_amd.vecac import VecActorCritic
    # a probe with the rollout's own weights, one minibatch, identity order: the ratio is 1 up to the difference of the acting and the
    # training trunk (both within Q_ATOL = 1e-4 of float64, far inside the clip range of 0.2): nothing is clipped, and the KL term
    # (r - 1) - lr is float32 rounding: r = expf(lr) carries half an ulp of 1 (6e-8), lr^2 / 2 <= 5e-9
    probe = make_ppo()
    adv, ret = probe.collect()
    g = torch.zeros(probe.net.n_params, dtype=torch.float32, device="cuda")
    tn = 64
    l, _ = ppo_train_from_replay(probe.replay, probe.net, probe._indices(), adv, ret, probe.roll.logp.view(-1), probe.roll.value[:4].view(-1),
                                 n_total=tn, flat_grad=g)
    print(f"probe: loss {l.tolist()}")
    assert l[4].item() == 0.0 and abs(l[5].item()) <= 1e-6 and g.abs().max() > 0 and torch.isfinite(l).all()
    # two runs of three updates agree bit for bit
    a, b = make_ppo(max_grad_norm=5.0), make_ppo(max_grad_norm=5.0)
    la, lb = [a.update().clone() for _ in range(3)], [b.update().clone() for _ in range(3)]
    assert all(x.shape == (6,) and torch.isfinite(x).all() for x in la)
    assert all(torch.equal(x, y) for x, y in zip(la, lb)) and same_loop(torch, loop_state(a), loop_state(b))
    assert a.timeStep == 12 and a.updates == 3 and not torch.equal(a.net.store_params(), make_ppo().net.store_params())
    assert abs(la[0][3].item() - np.log(2)) < 1e-2                    # a fresh policy is near uniform: H ~ log 2
    assert 0.0 <= la[2][4].item() <= 1.0
    # save after two updates + load + one update == three straight updates; the file's settings replace the object's
    c = make_ppo(max_grad_norm=5.0)
    for _ in range(2):
        c.update()
    path = str(tmp_path / "ppo.npz")
    c.save(path)
    z = np.load(path)
    assert str(z["head"][0]) == "ac" and z["ppo"].tolist() == [2.0, 2.0, float(np.float32(0.2)), 0.0, 1.0]
    resumed = VecActorCritic(16, rollout=4, algo="ppo", epochs=1, minibatches=4, clip_eps=0.3, value_clip=1.0, normalize_adv=False, seed=4)
    resumed.load(path)
    assert (resumed.epochs, resumed.minibatches, resumed.normalize_adv) == (2, 2, True) and resumed.net.ppo() == (float(np.float32(0.2)), 0.0)
    assert same_loop(torch, loop_state(resumed), loop_state(c))
    l3 = resumed.update()
    assert torch.equal(l3, la[2]) and same_loop(torch, loop_state(resumed), loop_state(a))
    # the two kinds of file refuse each other
    with pytest.raises(ValueError, match="holds a PPO run"):
        VecActorCritic(16, rollout=4, seed=4).load(path)
    a2c = str(tmp_path / "a2c.npz")
    VecActorCritic(16, rollout=4, seed=4).save(a2c)
    with pytest.raises(ValueError, match="holds an A2C run"):
        resumed.load(a2c)
    assert same_loop(torch, loop_state(resumed), loop_state(a))
    # evaluate() runs and leaves the training state alone; the log line names PPO's two numbers
    st = loop_state(a)
    res = a.evaluate(n_envs=32, episodes=1, max_steps=200)
    assert res.score.shape == (32, 1) and same_loop(torch, loop_state(a), st)
    capsys.readouterr()
    a.run(1, log_every=1)
    line = capsys.readouterr().out
    assert "CLIP_FRAC" in line and "APPROX_KL" in line and "GRAD_NORM" in line
