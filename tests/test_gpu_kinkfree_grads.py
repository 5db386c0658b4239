"""Every gradient tensor, ELEMENT BY ELEMENT, against the float64 references at batch sizes above 32 and for every distributional head:
the shapes at which the rest of the suite holds the convolution gradients (and, for the distributional heads, W_fc1 / b_fc1) only in
relative L2.  The minibatches come from tests/kinkfree.py: states rejected one by one until each clears a ReLU / max-pool margin of
1e-4 in the oracle, so that no unit's mask differs between the device and the reference and every element is comparable.  One
bound throughout, test_train_step_gradients_match_oracle's: assert_allclose(got, ref, rtol=2e-3, atol=2e-5 max|ref|) per tensor.

Which case reaches which launch (dqnflappybird_amd/csrc/fb_qnet.hip: conv_backward, fc1_backward, ring_trunk; zmax = 64 slabs):
  test_scalar_gathered, net (512, 2), B =
     33   fold1 begins (2 B > 64): conv_bw_kernel writes 66 sub-slabs, slab_fold_kernel fold 2 -> z1 = 33; fc1_bwd2_kernel's second
          32-row tile holds one row
     64   the last B of conv_bw_kernel: fold 2, z1 = zmax = 64, z3 = 64 per-sample slabs (four full chunks of slab_sum4)
     65   the first B of conv_bx_kernel + conv_dw21_kernel<2, false>: fold 3, z1 = 44 -> 132 slots for 130 sub-slabs (a partly empty
          last slab), zt3 = 7
     96   fold 3 exact (z1 = 64), three row tiles
    129   fold 5, z1 = 52 -> 260 slots for 258 sub-slabs, five row tiles with one row in the last
    200   fold 7, z1 = 58, zt3 = 20 (two chunks of slab_sum4, the second partly filled)
    255   fold 8, z1 = 64, zt3 = 25; the last B of fc1_bwd2_kernel and of the small forward
    256   the LDS-staged pass: conv1_sp / conv23_sp side outputs (p1, amax, h2, h3), loss_head_kernel, fc1_bwd_big_kernel<*, 4, 2>
          (its dh3 feeds conv_bx), conv_dwg_kernel (z3 = 16 group slabs), fold 8
     (384, 3, dueling) and (1024, 8) at 256: fc1_bwd_big_kernel<*, 0, 0>;  (128, 1, dueling) at 255: one short chunk of fc1_bwd2's DX role
  test_ring_fed (fb_train_from_replay: conv23_t_kernel<*, true, W16, NST> from the 1-bit ring, conv_dw21_kernel<2, true>)
    dqn 128 / 129             two slices of B: 256 states W16 on, 258 off
    double dueling 85 / 86    three slices: 255 on, 258 off
    per 200                   importance weights, two slices, W16 off
    double 256                c.big behind the ring trunk: the fc1 launch that takes both nets' rows, conv_dwg_kernel
    nature n = 3, 129         the NST instantiation
  test_distributional, fc 512, A = 2, at B = 1 / 32 (conv_bw), 65 (conv_bx + conv_dw21) and 256 (the large pass, c51_grad / qr loss at
    256 rows): C51, dueling C51, QR, dueling QR and noisy C51 with a noise sample, one uniform and one weighted algo each -- trunk,
    W_fc1 and b_fc1 included, which no test compared elementwise before; noisy: sigma's exact identity as in check_noisy_grads
  test_fused_equals_exported at 65 / 255 / 256: the fused step (adam_fused_kernel sums z1 / z3 slabs itself, two lanes per float4 for
    conv2 / conv3, four for the rest) leaves the parameters, m, v and beta powers that the exported gradient + apply_adam leaves, bit
    for bit -- which ties the elementwise result above to the path that exports no gradient

The references are computed once per net and shared (module-level caches): the oracle's forward of the pool and of the next states,
of which the cases take prefixes -- the oracle's passes are per sample, tests/test_kinkfree_host.py holds that."""
import os
import time
import zlib

import numpy as np
import pytest

from tests import kinkfree
from tests.test_gpu_c51 import GAMMA, _batch, make_c51
from tests.test_gpu_c51 import ref_train as ref_train_c51
from tests.test_gpu_c51_dueling import make_c51d
from tests.test_gpu_c51_dueling import ref_train as ref_train_c51d
from tests.test_gpu_c51_noisy import TRUNK, effective, factors32, layers, make_noisy, n_mu
from tests.test_gpu_c51_noisy import ref_train as ref_train_noisy
from tests.test_gpu_c51_per import ref_train_weighted
from tests.test_gpu_nstep import composed
from tests.test_gpu_qnet import Q_ATOL, oracle_train_grads, rand_states
from tests.test_gpu_qr import make_qr
from tests.test_gpu_qr import ref_train as ref_train_qr
from tests.test_gpu_shapes import arch_of, make_scalar
from tests.test_oracle_qnet import tensor_bounds

pytestmark = pytest.mark.gpu
RTOL, ATOL_REL = 2e-3, 2e-5          # test_train_step_gradients_match_oracle's bounds on kink-free data
MARGIN = kinkfree.MARGIN             # 1e-4; a case that fails in the pattern of a mask flip is re-run once at 5e-4 (see kinkfree.py)
KIND = {"dqn": 0, "nature": 1, "double": 1, "per": 2}
_T0 = time.time()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def report(line):
    """figures for whoever measures: appended to the file FB_GRAD_REPORT names, if it is set, before anything is asserted"""
    path = os.environ.get("FB_GRAD_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(f"[{time.time() - _T0:7.1f}s] {line}\n")


def check_elementwise(tag, g, g0, tensors, zero=()):
    """every tensor of the flat gradient elementwise; `zero`: tensors without any gradient (the advantage stream at A = 1)"""
    assert tensors[-1][2] == len(g0) == len(g), (tensors[-1][2], len(g0), len(g))
    fails = []
    for name, lo, hi in tensors:
        ref, got = g0[lo:hi], g[lo:hi]
        if name in zero:
            assert not ref.any() and not got.any(), name
            continue
        scale = np.abs(ref).max()
        assert scale > 0, name
        bad = np.abs(got - ref) > ATOL_REL * scale + RTOL * np.abs(ref)
        report(f"{tag} {name:8s} max|err|/max|ref| {np.abs(got - ref).max() / scale:.2e}  outside {int(bad.sum())} of {ref.size}")
        if bad.any():
            fails.append(name)
    for name, lo, hi in tensors:
        if name not in zero:
            np.testing.assert_allclose(g[lo:hi], g0[lo:hi], rtol=RTOL, atol=ATOL_REL * np.abs(g0[lo:hi]).max(),
                                       err_msg=f"{tag} {name} (tensors outside the bound: {fails})")


# ================================================================================================================ scalar heads
class Ref:
    """the oracle's passes over one net's fixed states s (kink-free) and next states s2, computed once and on demand; cases take
    prefixes.  grads() is tests/test_gpu_qnet.py::oracle_train_grads on those prefixes (test_scalar_gathered holds the two equal)"""

    def __init__(self, oracle, cfg, p_on, p_tg, s, s2):
        self.o, self.cfg, self.p_on, self.p_tg, self.s, self.s2 = oracle, cfg, p_on, p_tg, s, s2
        self._c = {}

    def _get(self, key, fn):
        if key not in self._c:
            self._c[key] = fn()
        return self._c[key]

    def grads(self, algo, B, a, r, t, isw, gamma=0.99):
        o, cfg = self.o, self.cfg
        q, acts = self._get("s", lambda: o.forward(self.p_on, cfg, self.s, keep=True))
        if algo == "dqn":
            qn = self._get("on2", lambda: o.forward(self.p_on, cfg, self.s2))[:B].max(1)
        elif algo == "double":
            am = self._get("on2", lambda: o.forward(self.p_on, cfg, self.s2))[:B].argmax(1)
            qn = self._get("tg2", lambda: o.forward(self.p_tg, cfg, self.s2))[np.arange(B), am]
        else:
            qn = self._get("tg2", lambda: o.forward(self.p_tg, cfg, self.s2))[:B].max(1)
        y, loss, ae, dq = o.dqn_loss(KIND[algo], q[:B], qn, a, r, t, isw=isw, gamma=gamma)
        return y, loss, ae, o.backward(self.p_on, cfg, self.s[:B], np.ascontiguousarray(acts[:B]), dq)


_scalar = {}


def scalar_case(oracle, fc, A, dueling):
    """one net per (fc, A, dueling), its kink-free pool and shared reference.  Gradient-exporting steps leave the net as it was."""
    key = (fc, A, dueling)
    if key not in _scalar:
        net, cfg, p_on, p_tg = make_scalar(oracle, fc, A, dueling, kinkfree.POOL)
        s, drawn = kinkfree.pool(oracle, p_on, fc, seed=fc, margin=MARGIN)
        report(f"pool ({fc}, {A}, {arch_of(dueling)}): accepted {len(s)} of {drawn} = {len(s) / drawn:.3f} at margin {MARGIN}")
        s2 = rand_states(np.random.default_rng(fc + 1), kinkfree.POOL)
        _scalar[key] = (net, cfg, p_on, p_tg, Ref(oracle, cfg, p_on, p_tg, s, s2))
    return _scalar[key]


def targets(rng, B, A, algo):
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    t = (r == -3).astype(np.uint8)
    isw = rng.random(B).astype(np.float32) if algo == "per" else None
    return a, r, t, isw


SCALAR = [(512, 2, False, "dqn", 33), (512, 2, True, "nature", 64), (512, 2, False, "double", 65), (512, 2, True, "per", 96),
          (512, 2, True, "dqn", 129), (512, 2, False, "nature", 200), (512, 2, True, "double", 255), (512, 2, False, "per", 256),
          (384, 3, True, "double", 256), (1024, 8, False, "nature", 256), (128, 1, True, "per", 255)]


@pytest.mark.parametrize("fc,A,dueling,algo,B", SCALAR)
def test_scalar_gathered(torch_cuda, oracle, fc, A, dueling, algo, B):
    """train_step(flat_grad) on gathered states: y, |err| and the loss with test_scalar_train_step's bounds, every gradient tensor
    elementwise against oracle_train_grads"""
    torch = torch_cuda
    net, cfg, p_on, p_tg, ref = scalar_case(oracle, fc, A, dueling)
    rng = np.random.default_rng(zlib.crc32(f"kf-{fc}-{A}-{dueling}-{algo}-{B}".encode()))
    a, r, t, isw = targets(rng, B, A, algo)
    s, s2 = ref.s[:B], ref.s2[:B]
    d = lambda x: None if x is None else torch.from_numpy(np.array(x)).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, ae, y = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(isw), flat_grad=grad)
    loss, ae, y, g = loss.item(), ae.cpu().numpy(), y.cpu().numpy(), grad.cpu().numpy()
    y0, loss0, ae0, g0 = ref.grads(algo, B, a, r, t, isw)
    if B == 33:                                                # the shared reference IS oracle_train_grads
        direct = oracle_train_grads(oracle, cfg, p_on, p_tg, algo, s, a, r, s2, t, isw)
        assert np.array_equal(direct[0], y0) and direct[1] == loss0 and np.array_equal(direct[2], ae0) and np.array_equal(direct[3], g0)
    tag = f"scalar ({fc}, {A}, {arch_of(dueling)}) {algo} B={B}"
    report(f"{tag} max|y - y0| {np.abs(y - y0).max():.2e}  loss {loss:.6g} / {loss0:.6g}")
    np.testing.assert_allclose(y, y0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(ae, ae0, rtol=0, atol=2 * Q_ATOL)
    np.testing.assert_allclose(loss, loss0, rtol=1e-4, atol=1e-6)
    check_elementwise(tag, g, g0, tensor_bounds(fc, A, arch_of(dueling)), zero=("W_q", "b_q") if dueling and A == 1 else ())
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)          # gradient-only mode


@pytest.mark.parametrize("B", [65, 255, 256])
def test_fused_equals_exported(torch_cuda, oracle, B):
    """(512, 2, plain, nature): train_step(flat_grad) + apply_adam on one net, the fused train_step on its twin: identical parameters,
    m, v and beta powers.  The exported gradient is the one test_scalar_gathered compares elementwise at these slab counts"""
    torch = torch_cuda
    _, _, _, _, ref = scalar_case(oracle, 512, 2, False)
    nets = [make_scalar(oracle, 512, 2, False, kinkfree.POOL)[0] for _ in range(2)]
    for n in nets:
        n.set_hparams(lr=1e-4)
    rng = np.random.default_rng(B)
    a, r, t, _ = targets(rng, B, 2, "nature")
    d = lambda x: torch.from_numpy(np.array(x)).cuda()
    args = (d(ref.s[:B]), d(a), d(r), d(ref.s2[:B]), d(t))
    grad = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    before = nets[0].store_params().clone()
    l0 = nets[0].train_step("nature", *args, flat_grad=grad)[0].clone()
    nets[0].apply_adam(grad)
    l1 = nets[1].train_step("nature", *args)[0]
    assert torch.equal(l0, l1)
    assert torch.equal(nets[0].store_params(), nets[1].store_params()) and not torch.equal(nets[0].store_params(), before)
    (m0, v0, p0), (m1, v1, p1) = nets[0].adam_state(), nets[1].adam_state()
    assert torch.equal(m0, m1) and torch.equal(v0, v1) and np.array_equal(p0, p1)
    assert torch.equal(nets[0].store_params(1), nets[1].store_params(1))


# ================================================================================================================ ring-fed
RING_ENVS, RING_CAP, RING_PUSHES = 64, 4000, 80        # 5120 pushes into 4000 slots: the ring has wrapped
_ring = {}


def ring_memory(torch):
    """the memory of test_ring_fed_train_step_gradients_match_oracle, pushed to until it has wrapped"""
    if "rep" not in _ring:
        from dqnflappybird_amd.vec import VecGameState, VecReplay
        env, rep = VecGameState(RING_ENVS, seed=11), VecReplay(RING_CAP, RING_ENVS)
        env.observe(); rep.reset(env.frame_bits)
        rng = np.random.default_rng(5)
        for _ in range(RING_PUSHES):
            acts = torch.from_numpy((rng.random(RING_ENVS) < 0.12).astype(np.uint8)).cuda()
            env.frame_step(acts, want_u8=False)
            rep.push(env.frame_bits, acts, env.reward, env.terminal)
        assert len(rep) == RING_CAP
        _ring["rep"] = rep
    return _ring["rep"]


def ring_case(torch, oracle, dueling):
    """(net, cfg, p_on, p_tg, 256 ring positions whose states are kink-free under the net's trunk, the one-step tuple gathered at
    them, the shared reference).  The positions leave room for the n = 3 view (population = len - 2 x envs)."""
    if dueling not in _ring:
        rep = ring_memory(torch)
        net, cfg, p_on, p_tg = make_scalar(oracle, 512, 2, dueling, kinkfree.POOL)
        rng = np.random.default_rng(7)
        drawn_idx = []

        def source():
            drawn_idx.append(int(rng.integers(0, len(rep) - 2 * RING_ENVS)))
            return rep.gather(torch.tensor(drawn_idx[-1:], dtype=torch.int64).cuda())[0].cpu().numpy()[0]

        picked = []
        s, drawn = kinkfree.kink_free_states(oracle, p_on, 512, kinkfree.POOL, None, MARGIN, source=source, nonzero=True, picked=picked)
        report(f"ring pool ({arch_of(dueling)}): accepted {len(s)} of {drawn} = {len(s) / drawn:.3f} at margin {MARGIN} (game frames)")
        idx = np.array(drawn_idx, np.int64)[picked]
        tup = [x.cpu().numpy().copy() for x in rep.gather(torch.from_numpy(idx).cuda())]
        assert np.array_equal(tup[0], s)
        assert len(set(idx.tolist())) > 200
        _ring[dueling] = (net, cfg, p_on, p_tg, idx, tup, Ref(oracle, cfg, p_on, p_tg, s, tup[3]))
    return _ring[dueling]


RING = [("dqn", False, 128, 1), ("dqn", False, 129, 1), ("double", True, 85, 1), ("double", True, 86, 1), ("per", False, 200, 1),
        ("double", False, 256, 1), ("nature", False, 129, 3)]


@pytest.mark.parametrize("algo,dueling,B,n", RING)
def test_ring_fed(torch_cuda, oracle, algo, dueling, B, n):
    """train_from_replay(flat_grad) against the oracle on the states the gather kernel expands from the same ring positions: the loss,
    |err| (per) and every gradient tensor elementwise; a, r, t as gathered (n = 3: the composed n-step tuple and Gamma)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import train_from_replay
    rep = ring_memory(torch)
    net, cfg, p_on, p_tg, idx, (s, a, r, s2, t), ref = ring_case(torch, oracle, dueling)
    idx, s, a, r, t = idx[:B], s[:B], a[:B], r[:B], t[:B]
    idxd = torch.from_numpy(idx).cuda()
    rng = np.random.default_rng(B)
    isw = rng.random(B).astype(np.float32) if algo == "per" else None
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    if n > 1:
        rep.set_n_step(n, GAMMA)
    try:
        if n > 1:
            assert idx.max() < rep.population
            s_n, a, r, s2, t, G, _ = composed(rep, idxd, n, GAMMA)
            assert np.array_equal(s_n, s)
        out = train_from_replay(rep, net, algo, idxd, gamma=GAMMA, flat_grad=grad, isw=None if isw is None else torch.from_numpy(isw).cuda(),
                                want_abs_err=True)
    finally:
        if n > 1:
            rep.set_n_step(1, GAMMA)
    loss, ae, g = out[0].item(), out[4].cpu().numpy(), grad.cpu().numpy()
    assert np.array_equal(out[1].cpu().numpy(), a) and np.array_equal(out[2].cpu().numpy(), r) and np.array_equal(out[3].cpu().numpy(), t)
    if n > 1:                                                  # (other next states than the shared reference's)
        q, acts = oracle.forward(p_on, cfg, s, keep=True)
        qn = oracle.forward(p_tg, cfg, s2).max(1)
        assert algo == "nature"
        _, loss0, ae0, dq = oracle.dqn_loss(KIND[algo], q, qn, a, r, t, gamma=G)
        g0 = oracle.backward(p_on, cfg, s, acts, dq)
    else:
        _, loss0, ae0, g0 = ref.grads(algo, B, a, r, t, isw, gamma=GAMMA)
    tag = f"ring {algo} {arch_of(dueling)} B={B} n={n}"
    report(f"{tag} loss {loss:.6g} / {loss0:.6g}  max|ae - ae0| {np.abs(ae - ae0).max():.2e}")
    np.testing.assert_allclose(loss, loss0, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(ae, ae0, rtol=0, atol=2 * Q_ATOL)
    check_elementwise(tag, g, g0, tensor_bounds(512, 2, arch_of(dueling)))
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)


# ================================================================================================================ distributional heads
N_DIST = 51
HEADS = {"c51": ("c51", "c51per"), "c51dueling": ("c51double", "c51doubleper"), "qr": ("qr", "qrdoubleper"),
         "qrdueling": ("qrdouble", "qrper"), "noisy": ("c51double", "c51per")}
_dist = {}


def dist_case(torch, oracle, head):
    """one net per head (fc 512, A = 2, N = 51), the kink-free pool under its online trunk (a noisy net: under mu + sigma (.) e) and
    one batch of 256 (a, r, s2, t) of which the cases take prefixes"""
    if head not in _dist:
        nz = None
        if head == "c51":
            net, p_on, p_tg = make_c51(N_DIST, max_batch=kinkfree.POOL)
        elif head == "c51dueling":
            net, p_on, p_tg = make_c51d(N_DIST, max_batch=kinkfree.POOL)
        elif head == "noisy":
            net, p_on, p_tg = make_noisy("c51", N_DIST, max_batch=kinkfree.POOL)
            net.reset_noise(0, 11, 4)
            net.reset_noise(1, 11, 4)
            nz = (net.noise(0).cpu().numpy(), net.noise(1).cpu().numpy())
        else:
            net, p_on, p_tg = make_qr(N_DIST, arch=head, max_batch=kinkfree.POOL)
        trunk = p_on if nz is None else effective(p_on, nz[0], "c51", N_DIST).numpy().astype(np.float32)
        s, drawn = kinkfree.pool(oracle, trunk, 512, seed=512, margin=MARGIN)
        report(f"pool {head}: accepted {len(s)} of {drawn} = {len(s) / drawn:.3f} at margin {MARGIN}")
        rng = np.random.default_rng(zlib.crc32(f"kf-dist-{head}".encode()))
        _, a, r, s2, t = _batch(rng, kinkfree.POOL)
        w = (1.0 - 0.8 * rng.random(kinkfree.POOL)).astype(np.float32)          # importance weights in [0.2, 1]
        _dist[head] = (net, p_on, p_tg, nz, s, a, r, s2, t, w)
    return _dist[head]


@pytest.mark.parametrize("B", [1, 32, 65, 256])
@pytest.mark.parametrize("weighted", [False, True], ids=["uniform", "weighted"])
@pytest.mark.parametrize("head", list(HEADS))
def test_distributional(torch_cuda, oracle, head, weighted, B):
    """the loss, the priorities (weighted algos) and every gradient tensor elementwise against the head's float64 restatement"""
    torch = torch_cuda
    net, p_on, p_tg, nz, s, a, r, s2, t, w = dist_case(torch, oracle, head)
    algo = HEADS[head][weighted]
    s, a, r, s2, t = np.array(s[:B]), a[:B], r[:B], s2[:B], t[:B]             # (a writable copy of the shared pool's prefix)
    w = w[:B] if weighted else None
    w64 = None if w is None else w.astype(np.float64)
    d = lambda x: None if x is None else torch.from_numpy(np.array(x)).cuda()
    dev_astar = net.forward(d(s2), 0 if "double" in algo else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w), gamma=GAMMA, flat_grad=grad)
    loss, g = loss.item(), grad.cpu().numpy()
    ae0 = None
    if head == "c51":
        if weighted:
            loss0, g0, ae0 = ref_train_weighted(p_on, p_tg, s, a, r, s2, t, w64, GAMMA, algo, N_DIST, -10.0, 10.0, dev_astar)
        else:
            loss0, g0, _ = ref_train_c51(p_on, p_tg, s, a, r, s2, t, GAMMA, algo, N_DIST, -10.0, 10.0, dev_astar)
    elif head == "c51dueling":
        loss0, g0, ae0 = ref_train_c51d(p_on, p_tg, s, a, r, s2, t, w64, GAMMA, algo, N_DIST, -10.0, 10.0, dev_astar)
    elif head == "noisy":
        loss0, g0, ae0 = ref_train_noisy("c51", p_on, nz[0], p_tg, nz[1], s, a, r, s2, t, w64, GAMMA, algo, N_DIST, dev_astar)
    else:
        loss0, g0, ae0, _ = ref_train_qr(p_on, p_tg, s, a, r, s2, t, w64, GAMMA, algo, N_DIST, 1.0, dev_astar, head)
    tag = f"dist {head} {algo} B={B}"
    report(f"{tag} loss {loss:.6g} / {loss0:.6g}")
    np.testing.assert_allclose(loss, loss0, rtol=1e-4, atol=1e-6)
    if weighted:                                               # the priorities, with the bounds of the heads' own tests
        if head.startswith("qr"):
            np.testing.assert_allclose(ae.cpu().numpy(), ae0, rtol=1e-4, atol=1e-6)
        else:
            np.testing.assert_allclose(ae.cpu().numpy(), ae0, rtol=1e-4, atol=5e-4)
    arch = "c51dueling" if head.endswith("dueling") else "c51"
    mu = tensor_bounds(512, 2, arch, N_DIST)
    if head != "noisy":
        check_elementwise(tag, g, g0, mu)
    else:
        # [mu | sigma]: mu as the plain net's tensors; sigma exactly the device's mu gradient x e(q) in float32 (check_noisy_grads's
        # identity), and every sigma tensor elementwise against autograd, fc1's included
        n = n_mu("c51", N_DIST)
        assert np.array_equal(g[n:], g[TRUNK:n] * factors32("c51", N_DIST, nz[0]))
        sig, o = [], n
        for k, (_, fi, fo, _, _) in enumerate(layers("c51", N_DIST)[0]):
            sig += [(f"sigma_W{k}", o, o + fi * fo), (f"sigma_b{k}", o + fi * fo, o + (fi + 1) * fo)]
            o += (fi + 1) * fo
        check_elementwise(tag, g, g0, mu + sig)
    assert torch.equal(net.store_params(), before)
