"""Q-network kernels at the fc1 widths and action counts the C ABI accepts besides the reference's 512 / 2 (fb_qnet_create*: fc_width
128 .. 4096 in steps of 128, n_actions 1 .. MAXA = 8, C51 with n_actions x n_atoms <= 128), against the suite's float64 references:
the oracle (oracle.forward / backward / dqn_loss / pg_loss, tests/test_gpu_qnet.py::oracle_train_grads) for the scalar heads, the
torch restatements of tests/test_gpu_c51*.py and tests/test_gpu_noisy_env.py for the C51 heads; and C51 in bf16-operand mode.

Which case reaches which instantiation (dqnflappybird_amd/csrc/):
  head_one_t<MAXA> (fb_head.h: head_kernel, acting, act)       test_scalar_forward_and_act / test_scalar_act_nib: every A != 2 case
  loss_head_kernel -> loss_head_body<MAXA> (B = 256)           test_scalar_train_step: (128, 1) per, (128, 1, dueling) dqn,
                                                               (384, 3, dueling) nature, (1024, 8) nature, (512, 5) per at B 256
  fc1_bwd2_kernel -> fc1_bwd2_body<MAXA, *> (B < 256)          test_scalar_train_step: A = 1, 3, 5, 8 at B 1 / 32 / 255;
                                                               test_pg_step_at_three_actions; test_actor_critic_critic_call
  fc1_bwd2_body DX role, ch = min(FC, 512)                     test_scalar_train_step: FC 128 / 384 (one short chunk), 1024 / 4096
                                                               (two / eight chunks of 512) at B < 256
  fc1_bwd_big_kernel<*, 0, 0> on the scalar heads              test_scalar_train_step: (128, 1), (384, 3), (1024, 8) at B 256 (FC != 512);
                                                               (512, 5) at B 256 keeps <*, 4, 2> with A != 2
  c51_head_kernel<MAXA>, c51_loss_kernel<MAXA, *>              test_c51_forward / test_c51_train_step: A = 1, 3, 8 (c51per: the
                                                               weighted instantiation)
  env_noise_head_kernel<MAXA, *>                               test_noisy_env_acting_at_three_actions (both heads)
  c51d_fold_kernel, c51_grad / c51d_grad grids (FC / 16)       test_c51_train_step (FC 128 / 384 / 1024 / 4096, A N = 64 / 126 / 128),
                                                               test_c51_dueling_forward / test_c51_dueling_train_step
  fc1_fk_kernel (FC / 16 grid), fc1_sp_kernel (FC / 64 tiles),  test_scalar_forward_and_act (B 1 / 33 / 255 and 256 / 700),
  wsplit / hf_act sizing                                       test_scalar_act_nib (the fused acting trunk), test_c51_forward
  adam_fused_kernel tail (n & 3)                               test_scalar_adam_bit_exact: parameter counts = 0, 1, 2, 3 (mod 4)
  C51 bf16 operands (fb_qnet_set_inference / train_dtype)      test_c51_bf16_inference, test_c51_bf16_training
  qr_head_kernel<2 | MAXA>, qr_loss_kernel<2 | MAXA, *>,        tests/test_gpu_qr_shapes.py (written after QR-DQN was added; its docstring
  QR bf16 operands                                             maps each instantiation to its cases): test_qr_forward, test_qr_acting,
                                                               test_qr_train_step, test_qr_dueling_train_step, test_qr_bf16_*
  first maximum on exact ties (every head kind), the QR        tests/test_gpu_exact_heads.py
  loss's worked case and kinks on the kernel
"""
import zlib

import numpy as np
import pytest

from tests.test_gpu_c51 import GAMMA, _check_grads, head0, make_c51, ref_logits, ref_train, support
from tests.test_gpu_c51_dueling import check_grads as check_grads_d
from tests.test_gpu_c51_dueling import make_c51d, ref_logits_d
from tests.test_gpu_c51_dueling import ref_train as ref_train_d
from tests.test_gpu_c51_noisy import check_noisy_grads, effective, held, logits, make_noisy, same
from tests.test_gpu_c51_noisy import ref_train as ref_train_noisy
from tests.test_gpu_c51_per import ref_train_weighted
from tests.test_gpu_configs import BF16_GRAD_REL, BF16_Q_REL
from tests.test_gpu_noisy_env import chosen, restate, states
from tests.test_gpu_qnet import Q_ATOL, oracle_train_grads, rand_states, trained_like_params
from tests.test_oracle_qnet import tensor_bounds, torch_forward

pytestmark = pytest.mark.gpu
M32 = 0xFFFFFFFF

# (FC, A, dueling) -> the parameter count mod 4: adam_fused_kernel's tail handles the last n & 3 elements
SCALAR = {(128, 1, False): 1, (128, 1, True): 2, (384, 3, True): 0, (1024, 8, False): 0, (4096, 2, True): 3, (512, 5, False): 1}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def arch_of(dueling):
    return "dueling" if dueling else "plain"


def make_scalar(oracle, fc, A, dueling, max_batch, seeds=(1, 2)):
    """a scalar-head net holding trained_like_params (weights x 3) with the head scaled by sqrt(512 / FC) more, so that Q stays
    O(1..10) at every width (the sum over FC units grows as sqrt(FC)) -> (net, cfg, online params, target params)"""
    from dqnflappybird_amd.vec import QNet
    cfg = oracle.qcfg(fc, A, dueling)
    net = QNet(A, fc, arch_of(dueling), max_batch=max_batch)
    ps = []
    for which, seed in enumerate(seeds):
        p = trained_like_params(oracle, cfg, seed)
        p[head0(fc):] *= np.float32(np.sqrt(512 / fc))
        net.load_params(p, which)
        ps.append(p)
    return net, cfg, ps[0], ps[1]


def ref_q(oracle, p, cfg, s):
    """float64-accumulated Q: the oracle, or above FC 512 tests/test_oracle_qnet.py::torch_forward in float64 (the oracle's fc1 loop
    costs ~70 ms per state at FC 4096; test_forward_backward_vs_torch_at_other_shapes holds the two together at these shapes)"""
    if cfg.fc <= 512:
        return oracle.forward(p, cfg, s)
    import torch
    with torch.no_grad():
        return torch_forward(torch.from_numpy(p.astype(np.float64)), torch.from_numpy(s).double(), cfg.fc, cfg.actions,
                             bool(cfg.dueling)).numpy()


def top2_margin(q):
    """per row, how far the greedy action is ahead of the runner-up (inf with one action)"""
    if q.shape[1] < 2:
        return np.full(len(q), np.inf)
    top = np.sort(q, 1)
    return top[:, -1] - top[:, -2]


def eps_draws(oracle, n, A, seed, step):
    """the random actions of epsilon = 1 for envs 0 .. n-1: randrange(A) = (Philox word 1 x A) >> 32 of the documented stream
    (key = seed, counter = (env, step lo, FB_STREAM_EPS = 1, step hi); tests/test_gpu_qnet.py::test_act_epsilon_stream_is_the_documented_philox)"""
    out = np.empty(n, np.uint8)
    for e in range(n):
        ph = oracle.philox(seed & M32, seed >> 32, e, step & M32, 1, step >> 32)
        out[e] = (int(ph[1]) * A) >> 32
    return out


# ================================================================================================================ scalar heads
@pytest.mark.parametrize("fc,A,dueling", list(SCALAR))
def test_scalar_forward_and_act(torch_cuda, oracle, fc, A, dueling):
    """Q within 1e-4 on both trunk paths (B 1 / 33 / 255: conv1_pool, conv23_t, fc1_fk; B 256 / 700: conv1_sp, conv23_sp, fc1_sp);
    greedy act = the reference's argmax above the margin and the argmax of its own Q; epsilon = 1 the documented draws"""
    torch = torch_cuda
    net, cfg, p, _ = make_scalar(oracle, fc, A, dueling, 700)
    assert net.n_params == oracle.nparams(cfg) == tensor_bounds(fc, A, arch_of(dueling))[-1][2]
    rng = np.random.default_rng(fc * 10 + A)
    s = rand_states(rng, 700)
    want = ref_q(oracle, p, cfg, s)
    assert 0.5 < np.abs(want).max() < 100                      # the regime of the 512 / 2 tests
    sd = torch.from_numpy(s).cuda()
    seed, step = (9 << 32) | 5, (1 << 32) + 17
    rand = eps_draws(oracle, 700, A, seed, step)
    if A > 1:
        assert len(set(rand.tolist())) == A                       # every action is drawn
    for B in (1, 33, 255, 256, 700):
        x = sd[:B].contiguous()
        q = net.forward(x).cpu().numpy()
        assert q.shape == (B, A)
        np.testing.assert_allclose(q, want[:B], rtol=0, atol=Q_ATOL, err_msg=f"forward B={B}")
        act, qa = net.act(x, 0.0, seed=3, step=5, want_q=True)
        act, qa = act.cpu().numpy(), qa.cpu().numpy()
        np.testing.assert_allclose(qa, want[:B], rtol=0, atol=Q_ATOL, err_msg=f"act B={B}")
        assert np.array_equal(act, qa.argmax(1)), B
        sure = top2_margin(want[:B]) > 1e-4
        assert sure.mean() > 0.9
        assert np.array_equal(act[sure], want[:B].argmax(1)[sure]), B
        assert np.array_equal(net.act(x, 1.0, seed=seed, step=step).cpu().numpy(), rand[:B]), B
    assert net.overflow_count() == 0


@pytest.mark.parametrize("fc,A,dueling", [c for c in SCALAR if c[1] != 2])
def test_scalar_act_nib(torch_cuda, oracle, fc, A, dueling):
    """the acting path VecBrain runs (nibble states; >= 256 envs: the fused trunk, fc1 on K slices, then the head) against the
    reference, Q within 1e-4 and the greedy action above the margin"""
    net, cfg, p, _ = make_scalar(oracle, fc, A, dueling, 300)
    for n in (37, 300):
        nib, s = states(n)
        act, q = net.act_nib(nib, 0.0, seed=1, step=2, want_q=True)
        act, q = act.cpu().numpy(), q.cpu().numpy()
        want = ref_q(oracle, p, cfg, s)
        np.testing.assert_allclose(q, want, rtol=0, atol=Q_ATOL, err_msg=f"n={n}")
        sure = top2_margin(want) > 1e-4
        assert np.array_equal(act[sure], want.argmax(1)[sure]) and np.array_equal(act, q.argmax(1)), n
    assert net.overflow_count() == 0


def scalar_batch(rng, B, A, algo):
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.8, 0.1, 0.1])
    t = (r == -3).astype(np.uint8)
    isw = rng.random(B).astype(np.float32) if algo == "per" else None
    return s, a, r, s2, t, isw


def check_scalar_grads(g, g0, fc, A, dueling, kink_free, value_free=False):
    """per tensor.  A kink-free batch (every ReLU input and pool margin above 2e-5): every tensor elementwise with
    test_train_step_gradients_match_oracle's bounds.  Otherwise (B >= 255 drawn as one batch: among its ~10^7 unit inputs some sit
    within rounding distance of a kink, and this test rejects whole batches only): fc1 and the head elementwise
    (test_config2_double_dqn_batch256_gradients), the convolutions in relative L2 (tests/test_gpu_c51.py::_check_grads).  The margin is
    a property of one sample, though: tests/kinkfree.py rejects samples one by one, and tests/test_gpu_kinkfree_grads.py compares every
    tensor elementwise at these batch sizes.  The dueling head's advantage stream at A = 1 has no gradient at all (Q = V); value_free:
    the loss's dQ sums to 0 over the actions (policy gradient), so the value stream's gradient is 0 up to rounding: on W_q's scale."""
    tensors = tensor_bounds(fc, A, arch_of(dueling))
    for k, (name, lo, hi) in enumerate(tensors):
        ref, got = g0[lo:hi], g[lo:hi]
        if dueling and A == 1 and name in ("W_q", "b_q"):
            assert not ref.any() and not got.any(), name
            continue
        if value_free and name in ("W_v", "b_v"):
            wq = [t for t in tensors if t[0] == "W_q"][0]
            np.testing.assert_allclose(got, ref, rtol=0, atol=2e-5 * np.abs(g0[wq[1]:wq[2]]).max(), err_msg=name)
            continue
        scale = np.abs(ref).max()
        assert scale > 0, name
        if kink_free or k >= 6:
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=2e-5 * scale, err_msg=name)
        else:
            err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
            assert err < 2e-3, (name, err)


TRAIN = [(128, 1, False, "dqn", 1), (128, 1, False, "nature", 32), (128, 1, False, "per", 256),
         (128, 1, True, "double", 32), (128, 1, True, "dqn", 256),
         (384, 3, True, "per", 32), (384, 3, True, "double", 255), (384, 3, True, "nature", 256),
         (1024, 8, False, "double", 32), (1024, 8, False, "per", 1), (1024, 8, False, "nature", 256),
         (4096, 2, True, "dqn", 1), (4096, 2, True, "double", 5),
         (512, 5, False, "double", 32), (512, 5, False, "dqn", 255), (512, 5, False, "per", 256)]


@pytest.mark.parametrize("fc,A,dueling,algo,B", TRAIN)
def test_scalar_train_step(torch_cuda, oracle, fc, A, dueling, algo, B):
    """y, |err|, loss and every gradient tensor of the gradient-exporting train step against oracle_train_grads"""
    torch = torch_cuda
    net, cfg, p_on, p_tg = make_scalar(oracle, fc, A, dueling, max(B, 32))
    small = B <= 32
    for attempt in range(50 if small else 1):
        rng = np.random.default_rng(zlib.crc32(f"shape-{fc}-{A}-{dueling}-{algo}-{B}-{attempt}".encode()))
        s, a, r, s2, t, isw = scalar_batch(rng, B, A, algo)
        if not small:
            break
        oracle.forward(p_on, cfg, s)
        if oracle.last_margin() > 2e-5:
            break
    else:
        pytest.fail("no kink-free batch found")
    d = lambda x: None if x is None else torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss, ae, y = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(isw), flat_grad=grad)
    y0, loss0, ae0, g0 = oracle_train_grads(oracle, cfg, p_on, p_tg, algo, s, a, r, s2, t, isw)
    np.testing.assert_allclose(y.cpu().numpy(), y0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(ae.cpu().numpy(), ae0, rtol=0, atol=2 * Q_ATOL)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_scalar_grads(grad.cpu().numpy(), g0, fc, A, dueling, small)
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)          # gradient-only mode


@pytest.mark.parametrize("fc,A,dueling", list(SCALAR))
def test_scalar_adam_bit_exact(torch_cuda, oracle, fc, A, dueling):
    """exported gradient + apply_adam == the oracle's TF Adam on that gradient, and the fused step == both, bit for bit: parameters,
    m, v and the beta powers, at parameter counts of every residue mod 4 (adam_fused_kernel's tail)"""
    torch = torch_cuda
    assert sorted(set(SCALAR.values())) == [0, 1, 2, 3]
    nets = [make_scalar(oracle, fc, A, dueling, 32, seeds=(6, 6)) for _ in range(2)]
    cfg, p0 = nets[0][1], nets[0][2]
    assert oracle.nparams(cfg) % 4 == SCALAR[(fc, A, dueling)]
    nets = [n[0] for n in nets]
    for n in nets:
        n.set_hparams(lr=1e-4)
    opt = oracle.Adam(p0.size, lr=1e-4)
    p_ref = p0.copy()
    grad = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    rng = np.random.default_rng(fc + A)
    d = lambda x: torch.from_numpy(x).cuda()
    for step in range(3):
        s, a, r, s2, t, _ = scalar_batch(rng, 32, A, "nature")
        nets[0].train_step("nature", d(s), d(a), d(r), d(s2), d(t), flat_grad=grad)
        nets[0].apply_adam(grad)
        nets[1].train_step("nature", d(s), d(a), d(r), d(s2), d(t))
        opt.step(p_ref, grad.cpu().numpy())
        for n in nets:
            m, v, pows = n.adam_state()
            assert np.array_equal(pows, np.array([opt.b1p.value, opt.b2p.value], np.float32)), step
            assert np.array_equal(m.cpu().numpy(), opt.m), step
            assert np.array_equal(v.cpu().numpy(), opt.v), step
            assert np.array_equal(n.store_params().cpu().numpy(), p_ref), step
    assert not np.array_equal(p_ref, p0)


@pytest.mark.parametrize("fc,A,dueling", [(1024, 8, False), (384, 3, True)])
def test_scalar_ring_fed_equals_gather_plus_train_step(torch_cuda, oracle, fc, A, dueling):
    """fb_train_from_replay == fb_replay_gather + fb_qnet_train_step, bit for bit (loss, gradient, parameters after Adam)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import train_from_replay
    from tests.test_gpu_nstep import played
    _, rep = played(256, 20000, 30, seed=5)
    rng = np.random.default_rng(fc)
    for B in (32, 255):                                      # (the ring-fed trunk's two shapes, as in tests/test_gpu_nstep.py)
        n1, _, _, _ = make_scalar(oracle, fc, A, dueling, 256)
        n2, _, _, _ = make_scalar(oracle, fc, A, dueling, 256)
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(2):
            idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
            s, a, r, s2, t = rep.gather(idx)
            exp = step == 0
            l1, _, _ = n1.train_step("double", s, a, r, s2, t, gamma=GAMMA, flat_grad=g1 if exp else None, want_aux=False)
            l2, a2, r2, t2 = train_from_replay(rep, n2, "double", idx, gamma=GAMMA, flat_grad=g2 if exp else None)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert torch.equal(l1, l2), (B, step)
            if exp:
                assert torch.equal(g1, g2)
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params()), (B, step)


@pytest.mark.parametrize("fc,dueling,B", [(384, False, 32), (384, True, 17)])
def test_pg_step_at_three_actions(torch_cuda, oracle, fc, dueling, B):
    """FB_ALGO_PG with three actions: loss and every gradient tensor against oracle.pg_loss + oracle.backward"""
    torch = torch_cuda
    A = 3
    net, cfg, p, _ = make_scalar(oracle, fc, A, dueling, 128)
    for attempt in range(60):
        rng = np.random.default_rng(zlib.crc32(f"pg3-{fc}-{dueling}-{B}-{attempt}".encode()))
        s = rand_states(rng, B)
        q, acts = oracle.forward(p, cfg, s, keep=True)
        if oracle.last_margin() > 2e-5:
            break
    else:
        pytest.fail("no kink-free batch found")
    a = rng.integers(0, A, B).astype(np.uint8)
    w = rng.choice(np.array([0.1, 3, -3], np.float32), B, p=[0.6, 0.2, 0.2])
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    loss = net.pg_step(d(s), d(a), d(w), flat_grad=grad)
    loss0, dq = oracle.pg_loss(q, a, w)
    g0 = oracle.backward(p, cfg, s, acts, dq)
    np.testing.assert_allclose(loss.item(), loss0, rtol=2e-5, atol=1e-6)
    check_scalar_grads(grad.cpu().numpy(), g0, fc, A, dueling, True, value_free=True)
    assert np.array_equal(net.store_params().cpu().numpy(), p)


def test_actor_critic_critic_call(torch_cuda, oracle):
    """BrainDQNActorCritic's critic step as it is made: a one-action plain net of batch 1, "dqn", action 0, not terminal; y, loss and
    every gradient against the oracle, then the fused Adam step against the oracle's on that gradient"""
    torch = torch_cuda
    from dqnflappybird_amd.BrainActorCritic import GAMMA as AC_GAMMA
    from dqnflappybird_amd.vec import QNet
    cfg = oracle.qcfg(512, 1, False)
    p = trained_like_params(oracle, cfg, 4)
    nets = [QNet(1, 512, "plain", max_batch=1) for _ in range(2)]
    for n in nets:
        n.load_params(p)
    for attempt in range(50):
        rng = np.random.default_rng(zlib.crc32(f"critic-{attempt}".encode()))
        s, s2 = rand_states(rng, 1), rand_states(rng, 1)
        oracle.forward(p, cfg, s)
        if oracle.last_margin() > 2e-5:
            break
    else:
        pytest.fail("no kink-free batch found")
    a0, t0, r = np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.array([0.1], np.float32)
    d = lambda x: torch.from_numpy(x).cuda()
    grad = torch.zeros(nets[0].n_params, dtype=torch.float32, device="cuda")
    loss, _, y = nets[0].train_step("dqn", d(s), d(a0), d(r), d(s2), d(t0), gamma=AC_GAMMA, flat_grad=grad)
    q, acts = oracle.forward(p, cfg, s, keep=True)
    qn = oracle.forward(p, cfg, s2).max(1)
    y0, loss0, _, dq = oracle.dqn_loss(0, q, qn, a0, r, t0, gamma=AC_GAMMA)
    g0 = oracle.backward(p, cfg, s, acts, dq)
    np.testing.assert_allclose(y.cpu().numpy(), y0, rtol=0, atol=Q_ATOL)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_scalar_grads(grad.cpu().numpy(), g0, 512, 1, False, True)
    nets[1].train_step("dqn", d(s), d(a0), d(r), d(s2), d(t0), gamma=AC_GAMMA)
    opt = oracle.Adam(p.size)
    p_ref = p.copy()
    opt.step(p_ref, grad.cpu().numpy())
    assert np.array_equal(nets[1].store_params().cpu().numpy(), p_ref)


# ================================================================================================================ C51 heads
# (A, N, FC, v_min, v_max): A N = 64, 126, 128 (the limit); [-1, 30] puts v_max's clamp at +3 + gamma z and v_min's at -3
C51 = [(1, 64, 128, -10.0, 10.0), (3, 42, 384, -1.0, 30.0), (8, 16, 1024, -10.0, 10.0), (2, 64, 4096, -10.0, 10.0)]
C51_IDS = [f"A{c[0]}-N{c[1]}-FC{c[2]}" for c in C51]


def c51_batch(rng, B, A):
    s, s2 = rand_states(rng, B), rand_states(rng, B)
    a = rng.integers(0, A, B).astype(np.uint8)
    r = rng.choice(np.array([0.1, 3.0, -3.0], np.float32), B, p=[0.6, 0.2, 0.2])
    t = ((r == -3.0) & (rng.random(B) < 0.5)).astype(np.uint8)
    return s, a, r, s2, t


def _c51_forward(torch, net, p_on, p_tg, A, N, fc, vmin, vmax, ref):
    """distributions within 1e-4; Q = sum_i p_i z_i weighs each p_i's error by |z_i| <= 10, and at FC 4096 (fp32 sums over 4096
    units) that reaches 1.4e-4: Q within 1e-4 up to FC 1024, 2e-4 at 4096"""
    q_atol = 1e-4 if fc <= 1024 else 2e-4
    rng = np.random.default_rng(A * N + fc)
    s = rand_states(rng, 700)
    with torch.no_grad():
        pr = {w: torch.softmax(ref(torch.tensor(p, dtype=torch.float64), s), -1) for w, p in ((0, p_on), (1, p_tg))}
    z = support(N, vmin, vmax)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 255, 256, 700):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            p = net.forward_dist(sd[:B].contiguous(), which).cpu().numpy()
            assert p.shape == (B, A, N) and q.shape == (B, A)
            np.testing.assert_allclose(p, pr[which][:B].numpy(), rtol=0, atol=1e-4, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, (pr[which][:B] * z).sum(-1).numpy(), rtol=0, atol=q_atol, err_msg=f"B={B} which={which}")
    assert pr[0].max().item() > 1.5 / N


@pytest.mark.parametrize("A,N,fc,vmin,vmax", C51, ids=C51_IDS)
def test_c51_forward(torch_cuda, A, N, fc, vmin, vmax):
    net, p_on, p_tg = make_c51(N, vmin, vmax, max_batch=700, head_scale=np.sqrt(512 / fc), A=A, fc=fc)
    assert net.n_params == tensor_bounds(fc, A, "c51", N)[-1][2]
    _c51_forward(torch_cuda, net, p_on, p_tg, A, N, fc, vmin, vmax, lambda P, s: ref_logits(P, s, N, A, fc))


@pytest.mark.parametrize("B", [1, 32, 256])
@pytest.mark.parametrize("algo", ["c51", "c51double", "c51per"])
@pytest.mark.parametrize("A,N,fc,vmin,vmax", C51, ids=C51_IDS)
def test_c51_train_step(torch_cuda, A, N, fc, vmin, vmax, algo, B):
    """loss and every gradient tensor against autograd; c51per: the importance-weighted loss and the KL priorities"""
    torch = torch_cuda
    net, p_on, p_tg = make_c51(N, vmin, vmax, max_batch=256, head_scale=np.sqrt(512 / fc), A=A, fc=fc)
    rng = np.random.default_rng(zlib.crc32(f"c51shape-{A}-{N}-{fc}-{algo}-{B}".encode()))
    s, a, r, s2, t = c51_batch(rng, B, A)
    w = (1.0 - rng.random(B)).astype(np.float32) if algo == "c51per" else None
    d = lambda x: None if x is None else torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if algo == "c51double" else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w), gamma=GAMMA, flat_grad=grad)
    if algo == "c51per":
        loss0, g0, kl0 = ref_train_weighted(p_on, p_tg, s, a, r, s2, t, w.astype(np.float64), GAMMA, algo, N, vmin, vmax, dev_astar, A, fc)
        np.testing.assert_allclose(ae.cpu().numpy(), kl0, rtol=1e-4, atol=5e-4)
    else:
        loss0, g0, _ = ref_train(p_on, p_tg, s, a, r, s2, t, GAMMA, algo, N, vmin, vmax, dev_astar, A, fc)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    _check_grads(grad.cpu().numpy(), g0, A * N, fc)
    assert torch.equal(net.store_params(), before)


@pytest.mark.parametrize("A,N,fc,vmin,vmax", C51, ids=C51_IDS)
def test_c51_dueling_forward(torch_cuda, A, N, fc, vmin, vmax):
    net, p_on, p_tg = make_c51d(N, vmin, vmax, max_batch=700, head_scale=np.sqrt(512 / fc), A=A, fc=fc)
    assert net.n_params == tensor_bounds(fc, A, "c51dueling", N)[-1][2]
    _c51_forward(torch_cuda, net, p_on, p_tg, A, N, fc, vmin, vmax, lambda P, s: ref_logits_d(P, s, N, A, fc))


# the dueling head's advantage stream has no gradient at A = 1: the cases with A >= 2, every algo once, every batch path
C51D_TRAIN = [(c, algo, B) for c in C51[1:] for algo, B in (("c51", 1), ("c51double", 256), ("c51per", 32), ("c51doubleper", 256))]


@pytest.mark.parametrize("case,algo,B", C51D_TRAIN, ids=[f"{C51_IDS[C51.index(c)]}-{a}-{b}" for c, a, b in C51D_TRAIN])
def test_c51_dueling_train_step(torch_cuda, case, algo, B):
    torch = torch_cuda
    A, N, fc, vmin, vmax = case
    net, p_on, p_tg = make_c51d(N, vmin, vmax, max_batch=256, head_scale=np.sqrt(512 / fc), A=A, fc=fc)
    rng = np.random.default_rng(zlib.crc32(f"c51dshape-{A}-{N}-{fc}-{algo}-{B}".encode()))
    s, a, r, s2, t = c51_batch(rng, B, A)
    per = algo.endswith("per")
    w = (1.0 - rng.random(B)).astype(np.float32) if per else None
    d = lambda x: None if x is None else torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if "double" in algo else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = net.store_params().clone()
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w), gamma=GAMMA, flat_grad=grad)
    loss0, g0, kl0 = ref_train_d(p_on, p_tg, s, a, r, s2, t, w.astype(np.float64) if per else None, GAMMA, algo, N, vmin, vmax,
                                 dev_astar, A, fc)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_grads_d(grad.cpu().numpy(), g0, N, A, fc)
    if per:
        np.testing.assert_allclose(ae.cpu().numpy(), kl0, rtol=1e-4, atol=5e-4)
    assert torch.equal(net.store_params(), before)


# ---------------------------------------------------------------------------------------------------------------- noisy nets
NOISY_A, NOISY_N, NOISY_FC = 3, 42, 384


@pytest.mark.parametrize("head,algo", [("c51", "c51doubleper"), ("c51dueling", "c51")])
def test_noisy_sample_mode_at_three_actions(torch_cuda, head, algo):
    """a noisy net with a noise sample: distributions and Q against mu + sigma (.) e, then the loss and every gradient of [mu | sigma]"""
    torch = torch_cuda
    A, N, fc = NOISY_A, NOISY_N, NOISY_FC
    net, p_on, p_tg = make_noisy(head, N, max_batch=256, A=A, fc=fc)
    net.reset_noise(0, 11, 4)
    net.reset_noise(1, 11, 4)
    nz_on, nz_tg = net.noise(0).cpu().numpy(), net.noise(1).cpu().numpy()
    rng = np.random.default_rng(zlib.crc32(f"noisy3-{head}-{algo}".encode()))
    s = rand_states(rng, 256)
    with torch.no_grad():
        pr = torch.softmax(logits(head, effective(p_on, nz_on, head, N, A, fc), s, N, A, fc), -1)
    sd = torch.from_numpy(s).cuda()
    for B in (1, 255, 256):
        p = net.forward_dist(sd[:B].contiguous()).cpu().numpy()
        q = net.forward(sd[:B].contiguous()).cpu().numpy()
        np.testing.assert_allclose(p, pr[:B].numpy(), rtol=0, atol=1e-4, err_msg=f"B={B}")
        np.testing.assert_allclose(q, (pr[:B] * support(N, -10.0, 10.0)).sum(-1).numpy(), rtol=0, atol=5e-4, err_msg=f"B={B}")
    B = 32
    s, a, r, s2, t = c51_batch(rng, B, A)
    per = algo.endswith("per")
    w = (1.0 - rng.random(B)).astype(np.float32) if per else None
    d = lambda x: None if x is None else torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if "double" in algo else 1).argmax(1).cpu().numpy()
    grad = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    before = held(net)
    loss, ae, _ = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), isw=d(w), gamma=GAMMA, flat_grad=grad, want_aux=per)
    loss0, g0, kl0 = ref_train_noisy(head, p_on, nz_on, p_tg, nz_tg, s, a, r, s2, t, w.astype(np.float64) if per else None, GAMMA,
                                     algo, N, dev_astar, A, fc)
    np.testing.assert_allclose(loss.item(), loss0, rtol=1e-4, atol=1e-6)
    check_noisy_grads(grad.cpu().numpy(), g0, head, N, nz_on, A, fc)
    if per:
        np.testing.assert_allclose(ae.cpu().numpy(), kl0, rtol=1e-4, atol=5e-4)
    assert same(held(net), before)


@pytest.mark.parametrize("head", ["c51", "c51dueling"])
@pytest.mark.parametrize("n", [37, 300])
def test_noisy_env_acting_at_three_actions(torch_cuda, head, n):
    """fb_qnet_act_nib_env_noise (env_noise_head_kernel<MAXA, *>) against the per-env restatement of tests/test_gpu_noisy_env.py"""
    A, N, fc = NOISY_A, NOISY_N, NOISY_FC
    nib, s = states(n)
    net, _, _ = make_noisy(head, N, max_batch=max(n, 32), A=A, fc=fc)
    seed, step = 2 ** 33 + 11, 2 ** 32 + 6
    a, q = net.act_nib_env_noise(nib, 0.0, seed=seed, step=step, want_q=True)
    a, q = a.cpu().numpy(), q.cpu().numpy()
    assert q.shape == (n, A)
    envs = chosen(n)
    q0 = restate(net, head, N, s, seed, step, envs)
    np.testing.assert_allclose(q[envs], q0, rtol=0, atol=5e-4)
    sure = top2_margin(q0) > 1e-3
    assert np.array_equal(a[envs][sure], q0.argmax(1)[sure])
    assert np.array_equal(a, q.argmax(1))


# ================================================================================================================ C51 in bf16
BF16_CASES = [("c51", 2, 51, 512), ("c51dueling", 2, 51, 512), ("c51", 3, 42, 384), ("c51dueling", 3, 42, 384)]


def _make(arch, A, N, fc, max_batch):
    maker = make_c51 if arch == "c51" else make_c51d
    return maker(N, max_batch=max_batch, A=A, fc=fc)


@pytest.mark.parametrize("arch,A,N,fc", BF16_CASES)
def test_c51_bf16_inference(torch_cuda, arch, A, N, fc):
    """bf16 operands on the >= 256-state forward: distributions and Q within test_gpu_configs' relative bound of fp32 (and not equal
    to them), the greedy actions agree above the margin, and f32 again gives the fp32 results bit for bit.  A C51 Q is an expectation
    over the support, so its scale is the support's width (v_max - v_min = 20), not max |Q|: the dueling head's two streams give
    logit errors whose Q error reaches 4.5 % of max |Q| = 10 (measured), 2.3 % of the width, and whose largest probability error is
    3.1 % of max p (measured at FC 512 / A 2): twice the relative bound for the dueling head's distributions"""
    torch = torch_cuda
    net, _, _ = _make(arch, A, N, fc, 512)
    sd = torch.from_numpy(rand_states(np.random.default_rng(A * N + fc), 512)).cuda()
    q32, p32 = net.forward(sd).cpu().numpy().copy(), net.forward_dist(sd).cpu().numpy()
    net.set_inference_dtype("bf16")
    q16, p16 = net.forward(sd).cpu().numpy().copy(), net.forward_dist(sd).cpu().numpy()
    net.set_inference_dtype("f32")
    assert np.array_equal(net.forward(sd).cpu().numpy(), q32) and np.array_equal(net.forward_dist(sd).cpu().numpy(), p32)
    qs = 20.0
    assert 0 < np.abs(q16 - q32).max() <= BF16_Q_REL * qs
    assert 0 < np.abs(p16 - p32).max() <= (2 if arch == "c51dueling" else 1) * BF16_Q_REL * p32.max()
    sure = top2_margin(q32) > 2 * BF16_Q_REL * qs
    assert sure.sum() >= 10
    assert np.array_equal(q16.argmax(1)[sure], q32.argmax(1)[sure])


@pytest.mark.parametrize("B,algo", [(256, "c51double"), (32, "c51")])
@pytest.mark.parametrize("arch,A,N,fc", BF16_CASES)
def test_c51_bf16_training(torch_cuda, arch, A, N, fc, B, algo):
    """bf16 training of a C51 net: loss and per-tensor gradients within test_gpu_configs' relative bounds of the fp32 device gradients
    (and not equal to them), the whole gradient within bound of the float64 reference, f32 again bit for bit, the master weights
    untouched in gradient-only mode"""
    torch = torch_cuda
    net, p_on, p_tg = _make(arch, A, N, fc, B)
    rng = np.random.default_rng(zlib.crc32(f"bf16-{arch}-{A}-{fc}-{B}".encode()))
    s, a, r, s2, t = c51_batch(rng, B, A)
    d = lambda x: torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if algo == "c51double" else 1).argmax(1).cpu().numpy()
    g32, g16, g_again = (torch.zeros(net.n_params, dtype=torch.float32, device="cuda") for _ in range(3))
    loss32 = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g32)[0].item()
    net.set_train_dtype("bf16")
    loss16 = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g16)[0].item()
    net.set_train_dtype("f32")
    loss_again = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g_again)[0].item()
    assert torch.equal(g_again, g32) and loss_again == loss32
    if arch == "c51":
        loss0, g0, _ = ref_train(p_on, p_tg, s, a, r, s2, t, GAMMA, algo, N, -10.0, 10.0, dev_astar, A, fc)
    else:
        loss0, g0, _ = ref_train_d(p_on, p_tg, s, a, r, s2, t, None, GAMMA, algo, N, -10.0, 10.0, dev_astar, A, fc)
    assert abs(loss32 - loss0) <= 1e-4 * abs(loss0) + 1e-6
    assert 0 < abs(loss16 - loss32) < 3 * BF16_Q_REL * abs(loss32)
    g16n, g32n = g16.cpu().numpy(), g32.cpu().numpy()
    for name, lo, hi in tensor_bounds(fc, A, arch, N):
        ref = g32n[lo:hi]
        rel = np.linalg.norm(g16n[lo:hi] - ref) / np.linalg.norm(ref)
        assert 0 < rel < BF16_GRAD_REL, (name, rel)
    assert np.linalg.norm(g16n - g0) / np.linalg.norm(g0) < BF16_GRAD_REL
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)
