"""QR-DQN kernels at the fc1 widths, action counts and quantile counts the C ABI accepts besides 512 / 2 / 51 (fb_qnet_create_qr: fc_width
128 .. 4096 in steps of 128, n_actions 1 .. MAXA = 8, 2 <= N <= 64, A N <= 128), against the float64 restatement of
tests/test_gpu_qr.py (ref_theta, ref_train: the trunk of tests/test_oracle_qnet.py::torch_forward, the quantile head, the pairwise
quantile Huber loss with autograd), and QR in bf16-operand mode.  The shapes are tests/test_gpu_shapes.py::C51's four, as (A, N, FC),
plus the smallest N the ABI accepts and a kappa below most |u|; the head is scaled by sqrt(512 / FC) as there.

Which case reaches which instantiation (dqnflappybird_amd/csrc/fb_qnet.hip):
  qr_head_kernel<2>                          test_qr_forward: A2-N64-FC4096, A2-N2-FC512 (every lane on / 62 lanes masked);
                                             test_qr_eval_run_at_fc128; test_qr_bf16_inference (2, 51, 512)
  qr_head_kernel<MAXA>                       test_qr_forward: A = 1, 3, 8; test_qr_acting (act, act_nib small and fused trunk,
                                             fb_eval_q) at A = 3 and 8, both heads; test_qr_bf16_inference (3, 42, 384)
  qr_loss_kernel<2>                          test_qr_train_step / test_qr_dueling_train_step: A2-N64-FC4096, A2-N2-FC512 with qr /
                                             qrdouble; test_qr_bf16_training (2, 51, 512)
  qr_loss_kernel<2, true>                    the same shapes with qrper / qrdoubleper
  qr_loss_kernel<MAXA>                       test_qr_train_step: A = 1, 3, 8 with qr / qrdouble at B 1 / 32 / 256;
                                             test_qr_dueling_train_step: A = 3, 8; test_qr_ring_fed_at_three_actions;
                                             test_qr_bf16_training (3, 42, 384)
  qr_loss_kernel<MAXA, true>                 test_qr_train_step: A = 1, 3, 8 with qrper; test_qr_dueling_train_step: A = 3, 8 with
                                             qrper / qrdoubleper
  c51d_fold_kernel, c51_grad / c51d_grad     test_qr_train_step / test_qr_dueling_train_step at FC 128 / 384 / 1024 / 4096 and
  grids (FC / 16), fc1_bwd2 / fc1_bwd_big    A N = 4, 63, 64, 126, 128, at B < 256 and B = 256
  QR bf16 operands (fb_qnet_set_inference /  test_qr_bf16_inference, test_qr_bf16_training
  train_dtype)
(The exact ties and the header's worked case on these instantiations: tests/test_gpu_exact_heads.py.)
"""
import zlib

import numpy as np
import pytest

from tests.test_gpu_configs import BF16_GRAD_REL, BF16_Q_REL
from tests.test_gpu_eval import composed as composed_eval
from tests.test_gpu_noisy_env import states
from tests.test_gpu_qr import DOUBLE, GAMMA, _run_grad_case, make_qr, ref_theta, ref_train
from tests.test_gpu_shapes import c51_batch, eps_draws, top2_margin
from tests.test_oracle_qnet import rand_states, tensor_bounds

pytestmark = pytest.mark.gpu

# (A, N, FC, kappa): A N = 64, 126, 128 (the limit), 128, 4, 63
QR = [(1, 64, 128, 1.0), (3, 42, 384, 1.0), (8, 16, 1024, 1.0), (2, 64, 4096, 1.0), (2, 2, 512, 1.0), (3, 21, 512, 0.25)]
QR_IDS = [f"A{c[0]}-N{c[1]}-FC{c[2]}" for c in QR]
ARCHS = ("qr", "qrdueling")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def bounds_arch(arch):
    return "c51dueling" if arch == "qrdueling" else "c51"


def make(case, arch, max_batch):
    A, N, fc, kappa = case
    net, p_on, p_tg = make_qr(N, kappa, arch, max_batch, head_scale=np.sqrt(512 / fc), A=A, fc=fc)
    assert net.quantiles() == (N, kappa) and net.n_params == tensor_bounds(fc, A, bounds_arch(arch), N)[-1][2]
    return net, p_on, p_tg


def qr_batch(tag, B, A):
    """tests/test_gpu_shapes.py::c51_batch from the first seed of a fixed sequence whose batch holds, at B >= 32, terminal and
    bootstrapped samples and every action (8 actions in 32 draws miss one about once in nine times)"""
    for attempt in range(100):
        rng = np.random.default_rng(zlib.crc32(f"{tag}-{B}-{A}-{attempt}".encode()))
        s, a, r, s2, t = c51_batch(rng, B, A)
        if B < 32 or (t.any() and not t.all() and len(set(a.tolist())) == A):
            break
    if B >= 32:
        assert t.any() and not t.all() and sorted(set(a.tolist())) == list(range(A))
    return rng, s, a, r, s2, t


# ---------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("case", QR, ids=QR_IDS)
def test_qr_forward(torch_cuda, case, arch):
    """theta and Q = its mean of both nets within tests/test_gpu_qr.py's 1e-4 x max(1, max |theta|) on both trunk paths (B 1 / 255:
    conv1_pool, conv23_t, fc1_fk; B 256 / 700: conv1_sp, conv23_sp, fc1_sp)"""
    torch = torch_cuda
    A, N, fc, _ = case
    net, p_on, p_tg = make(case, arch, 700)
    rng = np.random.default_rng(A * N + fc)
    s = rand_states(rng, 700)
    with torch.no_grad():
        ref = {w: ref_theta(p, s, N, arch, A, fc).numpy() for w, p in ((0, p_on), (1, p_tg))}
    assert 0.5 < np.abs(ref[0]).max() < 100                     # the regime of the 512 / 2 tests
    assert np.median(ref[0].std(-1)) > 0.1                      # the quantiles of one action differ
    sd = torch.from_numpy(s).cuda()
    for B in (1, 255, 256, 700):
        for which in (0, 1):
            q = net.forward(sd[:B].contiguous(), which).cpu().numpy()
            th = net.forward_quantiles(sd[:B].contiguous(), which).cpu().numpy()
            want = ref[which][:B]
            assert th.shape == (B, A, N) and q.shape == (B, A)
            tol = 1e-4 * max(1.0, np.abs(want).max())
            print(f"forward {arch} {case} B={B} which={which}: theta err {np.abs(th - want).max():.3g} q err "
                  f"{np.abs(q - want.mean(-1)).max():.3g} tol {tol:.3g}")
            np.testing.assert_allclose(th, want, rtol=0, atol=tol, err_msg=f"B={B} which={which}")
            np.testing.assert_allclose(q, want.mean(-1), rtol=0, atol=tol, err_msg=f"B={B} which={which}")
    assert net.overflow_count() == 0


# ---------------------------------------------------------------------------------------------------------------- acting
@pytest.mark.parametrize("arch", ARCHS)
@pytest.mark.parametrize("case", [c for c in QR if c[0] > 2], ids=[i for c, i in zip(QR, QR_IDS) if c[0] > 2])
def test_qr_acting(torch_cuda, oracle, case, arch):
    """qr_head_kernel<MAXA> with an action output: act on u8 states (7 and 300 rows), act_nib on nibble states (37 rows, and 300: the
    fused acting trunk) and fb_eval_q: Q within 1e-4 x max(1, max |theta|) of the restatement, the greedy action = the restatement's
    argmax where its top two are further apart than 10 x that (at least 90 % of the rows) and = the argmax of the Q returned with it
    on every row; epsilon = 1 gives the documented draws"""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    A, N, fc, _ = case
    net, p_on, _ = make(case, arch, 300)
    seed, step = (9 << 32) | 5, (1 << 32) + 17
    rand = eps_draws(oracle, 300, A, seed, step)
    assert len(set(rand.tolist())) == A                         # every action is drawn

    def check(what, act, q, s):
        act, q = act.cpu().numpy(), q.cpu().numpy()
        with torch.no_grad():
            th = ref_theta(p_on, s, N, arch, A, fc).numpy()
        want = th.mean(-1)
        tol = 1e-4 * max(1.0, np.abs(th).max())
        sure = top2_margin(want) > 10 * tol
        print(f"acting {arch} {case} {what}: q err {np.abs(q - want).max():.3g} tol {tol:.3g} sure {sure.mean():.3f}")
        assert q.shape == (len(s), A)
        np.testing.assert_allclose(q, want, rtol=0, atol=tol, err_msg=what)
        assert sure.mean() >= 0.9, what
        assert np.array_equal(act[sure], want.argmax(1)[sure]), what
        assert np.array_equal(act, q.argmax(1)), what

    s_all = rand_states(np.random.default_rng(A * N + fc + 1), 300)
    for B in (7, 300):
        x = torch.from_numpy(s_all[:B]).cuda()
        check(f"act B={B}", *net.act(x, 0.0, seed=3, step=5, want_q=True), s_all[:B])
        assert np.array_equal(net.act(x, 1.0, seed=seed, step=step).cpu().numpy(), rand[:B]), B
    for n in (37, 300):
        nib, s = states(n)
        check(f"act_nib n={n}", *net.act_nib(nib, 0.0, seed=1, step=2, want_q=True), s)
        assert np.array_equal(net.act_nib(nib, 1.0, seed=seed, step=step).cpu().numpy(), rand[:n]), n
    nib, s = states(300)
    act, _ = net.act_nib(nib, 0.0, want_q=True)
    q = torch.empty((300, A), dtype=torch.float32, device="cuda")
    L.check(L.lib().fb_eval_q(net.h, L.ptr(nib), 300, L.ptr(q), L.current_stream()), "fb_eval_q")
    check("fb_eval_q", act, q, s)
    assert net.overflow_count() == 0


# ---------------------------------------------------------------------------------------------------------------- training
@pytest.mark.parametrize("B", [1, 32, 256])
@pytest.mark.parametrize("algo", ["qr", "qrdouble", "qrper"])
@pytest.mark.parametrize("case", QR, ids=QR_IDS)
def test_qr_train_step(torch_cuda, case, algo, B):
    """loss and every gradient tensor of the plain QR head against autograd, with tests/test_gpu_qr.py's tolerances; qrper: random
    weights in (0, 1], the weighted loss, and abs_err = the unweighted l_b"""
    A, N, fc, kappa = case
    net, p_on, p_tg = make(case, "qr", 256)
    rng, s, a, r, s2, t = qr_batch(f"qrshape-{A}-{N}-{fc}-{algo}", B, A)
    w = 1.0 - rng.random(B) if algo == "qrper" else None
    _run_grad_case(torch_cuda, net, p_on, p_tg, algo, s, a, r, s2, t, GAMMA, N, kappa, w=w, A=A, fc=fc)
    assert net.overflow_count() == 0


# the dueling head's advantage stream has no gradient at A = 1: the shapes with A >= 2, every algo once, every batch path
QRD_TRAIN = [(c, algo, B) for c in QR[1:] for algo, B in (("qr", 1), ("qrdouble", 256), ("qrper", 32), ("qrdoubleper", 256))]


@pytest.mark.parametrize("case,algo,B", QRD_TRAIN, ids=[f"{QR_IDS[QR.index(c)]}-{a}-{b}" for c, a, b in QRD_TRAIN])
def test_qr_dueling_train_step(torch_cuda, case, algo, B):
    """the dueling QR head (c51d_fold_kernel, qr_loss_kernel on the folded head, c51d_grad_kernel's unfold) against autograd"""
    A, N, fc, kappa = case
    net, p_on, p_tg = make(case, "qrdueling", 256)
    rng, s, a, r, s2, t = qr_batch(f"qrdshape-{A}-{N}-{fc}-{algo}", B, A)
    w = 1.0 - rng.random(B) if algo.endswith("per") else None
    _run_grad_case(torch_cuda, net, p_on, p_tg, algo, s, a, r, s2, t, GAMMA, N, kappa, arch="qrdueling", w=w, A=A, fc=fc)
    assert net.overflow_count() == 0


def test_qr_ring_fed_at_three_actions(torch_cuda):
    """fb_train_from_replay == fb_replay_gather + fb_qnet_train_step bit for bit (loss, gradient, parameters after Adam) on a memory
    that holds all three actions (the memory keeps the action byte it is given; the games themselves are played with two)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import VecGameState, VecReplay, train_from_replay
    case = QR[1]
    A = case[0]
    env, rep = VecGameState(256, seed=5), VecReplay(20000, 256)
    env.observe(); rep.reset(env.frame_bits)
    rng = np.random.default_rng(5)
    for _ in range(30):
        env.frame_step(torch.from_numpy((rng.random(256) < 0.05).astype(np.uint8)).cuda(), want_u8=False)
        rep.push(env.frame_bits, torch.from_numpy(rng.integers(0, A, 256).astype(np.uint8)).cuda(), env.reward, env.terminal)
    for B in (32, 255):
        n1, _, _ = make(case, "qr", 256)
        n2, _, _ = make(case, "qr", 256)
        for net in (n1, n2):
            net.set_hparams(lr=1e-4)
        g1 = torch.zeros(n1.n_params, device="cuda"); g2 = torch.zeros_like(g1)
        for step in range(2):
            for _ in range(100):                                 # (crashes are rare in 30 frames: draw until the batch holds one)
                idx = torch.from_numpy(rng.integers(0, rep.population, B)).cuda()
                s, a, r, s2, t = rep.gather(idx)
                if t.any():
                    break
            assert sorted(set(a.cpu().tolist())) == list(range(A)) and t.any() and not t.all()
            exp = step == 0
            l1, _, _ = n1.train_step("qrdouble", s, a, r, s2, t, gamma=GAMMA, flat_grad=g1 if exp else None, want_aux=False)
            l2, a2, r2, t2 = train_from_replay(rep, n2, "qrdouble", idx, gamma=GAMMA, flat_grad=g2 if exp else None)
            assert torch.equal(a, a2) and torch.equal(r, r2) and torch.equal(t, t2)
            assert torch.equal(l1, l2), (B, step)
            if exp:
                assert torch.equal(g1, g2) and g1.abs().max().item() > 0
                n1.apply_adam(g1); n2.apply_adam(g2)
            assert torch.equal(n1.store_params(), n2.store_params()), (B, step)


def test_qr_eval_run_at_fc128(torch_cuda):
    """fb_eval_run on a QR net of fc1 width 128 (two actions: the game's; N = 64) == act_nib + frame_step composed"""
    from dqnflappybird_amd.evaluate import Evaluator
    n, M = 200, 256
    net, _, _ = make_qr(64, 1.0, "qr", (M + 2) // 3, head_scale=3.0 * np.sqrt(512 / 128), A=2, fc=128)
    s0, l0, t0, _ = composed_eval(net, M, n, 2, env_seed=11)
    res = Evaluator(n).run(net, n, 2, max_steps=100_000, env_seed=11)
    assert np.array_equal(res.length, l0) and np.array_equal(res.score, s0) and np.array_equal(res.truncated, t0)
    assert (res.length > 0).all()


# ================================================================================================================ QR in bf16
BF16_CASES = [(arch, A, N, fc) for arch in ARCHS for A, N, fc in ((2, 51, 512), (3, 42, 384))]


@pytest.mark.parametrize("arch,A,N,fc", BF16_CASES)
def test_qr_bf16_inference(torch_cuda, arch, A, N, fc):
    """bf16 operands on the >= 256-state forward: theta and Q within test_gpu_configs' relative bound of the fp32 results, on the scale
    max |theta| of the fp32 device result (a QR net has no support width), and not equal to them; the greedy actions agree above the
    margin (max |theta| is several times max |Q|, so that margin leaves few rows: 2048 states, and at least one row); f32 again gives
    the fp32 results bit for bit"""
    torch = torch_cuda
    net, _, _ = make_qr(N, 1.0, arch, 700, A=A, fc=fc)
    sd = torch.from_numpy(rand_states(np.random.default_rng(A * N + fc), 2048)).cuda()
    q32, th32 = net.forward(sd).cpu().numpy().copy(), net.forward_quantiles(sd).cpu().numpy()
    net.set_inference_dtype("bf16")
    q16, th16 = net.forward(sd).cpu().numpy().copy(), net.forward_quantiles(sd).cpu().numpy()
    net.set_inference_dtype("f32")
    assert np.array_equal(net.forward(sd).cpu().numpy(), q32) and np.array_equal(net.forward_quantiles(sd).cpu().numpy(), th32)
    scale = np.abs(th32).max()
    print(f"bf16 inference {arch} {A} {N} {fc}: scale {scale:.3g} q err {np.abs(q16 - q32).max() / scale:.3g} theta err "
          f"{np.abs(th16 - th32).max() / scale:.3g} of it")
    assert 0 < np.abs(q16 - q32).max() <= BF16_Q_REL * scale
    assert 0 < np.abs(th16 - th32).max() <= BF16_Q_REL * scale
    sure = top2_margin(q32) > 2 * BF16_Q_REL * scale
    print(f"rows above the margin: {sure.sum()}")
    assert sure.sum() >= 1
    assert np.array_equal(q16.argmax(1)[sure], q32.argmax(1)[sure])


@pytest.mark.parametrize("B,algo", [(256, "qrdouble"), (32, "qr")])
@pytest.mark.parametrize("arch,A,N,fc", BF16_CASES)
def test_qr_bf16_training(torch_cuda, arch, A, N, fc, B, algo):
    """bf16 training of a QR net: loss and per-tensor gradients within test_gpu_configs' relative bounds of the fp32 device gradients
    (and not equal to them), the whole gradient within bound of the float64 reference, f32 again bit for bit, the master weights
    untouched in gradient-only mode"""
    torch = torch_cuda
    net, p_on, p_tg = make_qr(N, 1.0, arch, B, A=A, fc=fc)
    _, s, a, r, s2, t = qr_batch(f"qrbf16-{arch}-{A}-{fc}", B, A)
    d = lambda x: torch.from_numpy(x).cuda()
    dev_astar = net.forward(d(s2), 0 if algo in DOUBLE else 1).argmax(1).cpu().numpy()
    g32, g16, g_again = (torch.zeros(net.n_params, dtype=torch.float32, device="cuda") for _ in range(3))
    loss32 = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g32)[0].item()
    net.set_train_dtype("bf16")
    loss16 = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g16)[0].item()
    net.set_train_dtype("f32")
    loss_again = net.train_step(algo, d(s), d(a), d(r), d(s2), d(t), gamma=GAMMA, flat_grad=g_again)[0].item()
    assert torch.equal(g_again, g32) and loss_again == loss32
    loss0, g0, _, _ = ref_train(p_on, p_tg, s, a, r, s2, t, None, GAMMA, algo, N, 1.0, dev_astar, arch, A, fc)
    assert abs(loss32 - loss0) <= 1e-4 * abs(loss0) + 1e-6
    g16n, g32n = g16.cpu().numpy(), g32.cpu().numpy()
    rels = {}
    for name, lo, hi in tensor_bounds(fc, A, bounds_arch(arch), N):
        ref = g32n[lo:hi]
        rels[name] = np.linalg.norm(g16n[lo:hi] - ref) / np.linalg.norm(ref)
    whole = np.linalg.norm(g16n - g0) / np.linalg.norm(g0)
    print(f"bf16 training {arch} {A} {N} {fc} {algo} B={B}: loss rel {abs(loss16 - loss32) / abs(loss32):.3g} whole {whole:.3g} "
          + " ".join(f"{k} {v:.3g}" for k, v in rels.items()))
    assert 0 < abs(loss16 - loss32) < 3 * BF16_Q_REL * abs(loss32)
    for name, rel in rels.items():
        assert 0 < rel < BF16_GRAD_REL, (name, rel)
    assert whole < BF16_GRAD_REL
    assert np.array_equal(net.store_params().cpu().numpy(), p_on)
