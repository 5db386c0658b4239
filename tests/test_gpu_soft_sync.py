"""Soft (Polyak) target updates on the device (include/fbdqn.h: fb_qnet_soft_sync_target).  References: the float64 lerp of the two stored
vectors; fb_qnet_sync_target for rho = 1; and, for everything the library derives from the target's parameters (W_conv1's fp16 planes,
the split planes and their version words, a noisy net's effective vector, a dueling distributional net's folded head), a fresh net whose
target was loaded with the stored lerped vector through fb_qnet_load_params: bit for bit.

Bound of the values: t' = t + rho * (o - t) in fp32 is three roundings -- (o - t) to 2^-24 |o - t| <= 2^-23 max(|t|, |o|), the product
rho * (.) the same again at most (rho <= 1), the sum 2^-24 |t'| <= 2^-24 max(|t|, |o|): 2^-22 max(|t|, |o|) per element covers them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GAMMA = 0.99
KINDS = ("plain", "dueling", "c51dueling", "qrdueling", "noisy")
RHO = 0.25


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def new_net(kind, max_batch=256):
    from dqnflappybird_amd.vec import QNet
    if kind in ("plain", "dueling"):
        return QNet(2, 512, kind, max_batch=max_batch)
    if kind == "noisy":
        return QNet(2, 512, "c51dueling", max_batch=max_batch, noisy=True)
    return QNet(2, 512, kind, max_batch=max_batch)


def make_net(kind, max_batch=256):
    """different seeds and scales for the two nets (x 3 and x 2: Q of O(1), and no entry -- bias or sigma -- equal in both); the noisy
    net's target with a drawn sample"""
    net = new_net(kind, max_batch)
    net.init_params(3, which=0); net.init_params(11, which=1)
    for which, k in ((0, 3.0), (1, 2.0)):
        net.load_params(net.store_params(which) * k, which)
    if kind == "noisy":
        net.reset_noise(0, 5, 2); net.reset_noise(1, 5, 2)
    return net


def twin_of(kind, online, target, max_batch=256):
    """a fresh net of the same shape: the given vectors loaded through fb_qnet_load_params, the same noise samples"""
    net = new_net(kind, max_batch)
    if kind == "noisy":
        net.reset_noise(0, 5, 2); net.reset_noise(1, 5, 2)
    net.load_params(online, 0); net.load_params(target, 1)
    return net


def states(torch, B, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.random((B, 80, 80, 4)) < 0.37).astype(np.uint8) * 255).cuda()


@pytest.mark.parametrize("kind", KINDS)
def test_values_and_rho_1(torch_cuda, kind):
    torch = torch_cuda
    net = make_net(kind, 32)
    assert net.n_params % 4 == {"plain": 2, "dueling": 3, "c51dueling": 1, "qrdueling": 1, "noisy": 2}[kind]      # (every one has a ragged tail)
    o, t = net.store_params(0).clone(), net.store_params(1).clone()
    assert not torch.equal(o, t)
    m, v, pows = net.adam_state()
    net.soft_sync_target(RHO)
    o2, t2 = net.store_params(0), net.store_params(1)
    assert torch.equal(o2, o)                                    # the online net: bit-unchanged
    o64, t64 = o.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
    want = t64 + float(np.float32(RHO)) * (o64 - t64)
    err = np.abs(t2.cpu().numpy().astype(np.float64) - want)
    bound = 2.0 ** -22 * np.maximum(np.abs(t64), np.abs(o64))
    print(f"{kind}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}, moved {int((t2 != t).sum())} of {t.numel()}")
    assert (err <= bound).all() and (t2 != t).float().mean() > 0.9
    m2, v2, pows2 = net.adam_state()
    assert torch.equal(m, m2) and torch.equal(v, v2) and np.array_equal(pows, pows2)
    if kind == "noisy":                                          # [mu | sigma]: sigma moves as well
        assert net.n_params == 976_185 + 898_201 and (t2 != t)[976_185:].float().mean() > 0.9
    # rho = 1 is fb_qnet_sync_target itself
    a, b = make_net(kind, 32), make_net(kind, 32)
    a.soft_sync_target(1.0); b.sync_target()
    assert torch.equal(a.store_params(1), b.store_params(1)) and torch.equal(a.store_params(1), a.store_params(0))
    s = states(torch, 8, 1)
    assert torch.equal(a.forward(s, 1), b.forward(s, 1)) and torch.equal(a.forward(s, 1), a.forward(s, 0))


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_derived_from_the_target_is_stale(torch_cuda, kind):
    """forward(which = 1) at B = 8 (the small-batch kernels) and B = 256 (the plane path) after a soft sync == a fresh net whose target was
    loaded with the stored lerped vector; twice in a row (the second sync starts from planes the first one built)"""
    torch = torch_cuda
    net = make_net(kind)
    before = {B: net.forward(states(torch, B, B), 1).clone() for B in (8, 256)}
    for rep in range(2):
        net.soft_sync_target(RHO)
        twin = twin_of(kind, net.store_params(0), net.store_params(1))
        for B in (8, 256):
            s = states(torch, B, B)
            q, q_twin = net.forward(s, 1).clone(), twin.forward(s, 1)
            assert torch.equal(q, q_twin), (kind, rep, B)
            assert not torch.equal(q, before[B]), (kind, rep, B)             # (and it moved)
            before[B] = q
        if kind in ("c51dueling", "noisy"):
            s = states(torch, 8, 3)
            assert torch.equal(net.forward_dist(s, 1), twin.forward_dist(s, 1))
        if kind == "qrdueling":
            s = states(torch, 8, 3)
            assert torch.equal(net.forward_quantiles(s, 1), twin.forward_quantiles(s, 1))
        if kind == "noisy":                                      # the target's own sample, not the online net's, and both samples kept
            assert torch.equal(net.noise(1), twin.noise(1)) and torch.equal(net.noise(0), twin.noise(0))
    assert torch.equal(net.forward(states(torch, 8, 8), 0), twin.forward(states(torch, 8, 8), 0))


@pytest.mark.parametrize("kind", ["plain", "dueling"])
@pytest.mark.parametrize("B", [32, 256])
def test_a_train_step_reads_the_new_target(torch_cuda, kind, B):
    """one FB_ALGO_DOUBLE step after a soft sync: the loss and q_target of the freshly loaded twin, bit for bit"""
    torch = torch_cuda
    net = make_net(kind)
    net.soft_sync_target(RHO)
    twin = twin_of(kind, net.store_params(0), net.store_params(1))
    rng = np.random.default_rng(B)
    s, s2 = states(torch, B, 1), states(torch, B, 2)
    a = torch.from_numpy(rng.integers(0, 2, B).astype(np.uint8)).cuda()
    r_ = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    r, t = torch.from_numpy(r_).cuda(), torch.from_numpy((r_ == -3).astype(np.uint8)).cuda()
    l1, e1, y1 = net.train_step("double", s, a, r, s2, t, gamma=GAMMA)
    l2, e2, y2 = twin.train_step("double", s, a, r, s2, t, gamma=GAMMA)
    assert torch.equal(l1, l2) and torch.equal(y1, y2) and torch.equal(e1, e2)
    assert torch.equal(net.store_params(0), twin.store_params(0))
    hard = make_net(kind)                                        # (... and not the old target's: y differs from an unsynced net's)
    _, _, y0 = hard.train_step("double", s, a, r, s2, t, gamma=GAMMA)
    assert not torch.equal(y0, y1)
