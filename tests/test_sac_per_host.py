"""Prioritized SAC and n-step returns, the host side: the ABI's declarations of the three calls, the float32 numpy restatement of the
importance-weighted train step (built on tests/test_sac_host.py's) against float64 torch autograd, a worked case under a weight of 0.5, the
n-step target on a hand-made row, VecSAC's and vec's new argument checks, the checkpoint refusals by name and the command line of
--model sacper.  tests/test_gpu_sac_per.py imports the helpers."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_sac_host import F32, np_sac_loss, sac_heads, torch_sac_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def np_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha, w):
    """the prioritized step of include/fbdqn.h from the head outputs, float32 in the pinned order: np_sac_loss's, then w_b multiplied LAST
    into dQ_i and into the terms of m1 / m2; dz, L_pi, H and y untouched -> (loss[6], dz, dQ1, dQ2, y, abs_err [B])"""
    loss, dz, dq1, dq2, y = np_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha)
    q1, q2, w = np.asarray(q1, F32), np.asarray(q2, F32), np.asarray(w, F32)
    B, A = q1.shape
    ar, ac = np.arange(B), np.minimum(np.asarray(a, np.int64), A - 1)
    d1, d2 = (q1[ar, ac] - y).astype(F32), (q2[ar, ac] - y).astype(F32)
    dq1, dq2 = (dq1 * w[:, None]).astype(F32), (dq2 * w[:, None]).astype(F32)

    def mean(x):
        s = F32(0)
        for v in x:
            s = F32(s + v)
        return F32(s / F32(B))
    m1, m2 = mean(((d1 * d1).astype(F32) * w).astype(F32)), mean(((d2 * d2).astype(F32) * w).astype(F32))
    loss = np.array([F32(F32(m1 + m2) + loss[3]), m1, m2, loss[3], loss[4], loss[5]], F32)
    abs_err = (F32(0.5) * (np.abs(d1) + np.abs(d2)).astype(F32)).astype(F32)
    return loss, dz, dq1, dq2, y, abs_err


def torch_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha, w):
    """the same in float64 torch: the critics' squared errors weighted by w_b, the actor term and the entropy as they were
    -> (total, mean w d1^2, mean w d2^2, mean L_pi, mean H, y, 0.5 (|d1| + |d2|) [B]); the total's autograd gradient is the step's"""
    _, _, _, lpi, H, y = torch_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, gamma, alpha)
    B, A = z.shape
    ar, ac = torch.arange(B), torch.as_tensor(np.minimum(np.asarray(a, np.int64), A - 1))
    wt = torch.as_tensor(np.asarray(w, np.float64))
    d1, d2 = q1[ar, ac] - y, q2[ar, ac] - y
    l1, l2 = (wt * d1 ** 2).mean(), (wt * d2 ** 2).mean()
    return l1 + l2 + lpi, l1, l2, lpi, H, y, (0.5 * (d1.abs() + d2.abs())).detach()


def nstep_target(R, done, Gamma, Vn):
    """y of the n-step form: done ? R : R + Gamma V'(s'), the double arithmetic of every target here"""
    rd = 0.1 if F32(R) == F32(0.1) else float(F32(R))
    return F32(rd if done else rd + float(Gamma) * float(F32(Vn)))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_prioritized_sac_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    decls = ("int fb_qnet_sac_per_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,\n"
             "                               const float *isw /*f32[B]*/, double gamma, float *loss /*f32[6]*/, float *abs_err /*f32[B]*/,\n"
             "                               float *q_target, float *flat_grad, void *stream);",
             "int fb_sac_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *isw, uint8_t *a_out,\n"
             "                                 float *r_out, uint8_t *t_out, double gamma, float *loss, float *abs_err, float *q_target,\n"
             "                                 float *flat_grad, void *stream);",
             "int fb_sac_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch, uint64_t seed, uint64_t step,\n"
             "                    int train, double gamma, float rho, void *stream);")
    for decl in decls:
        assert decl in hdr, decl
    # the argument lists of the header and of the binding, type by type
    ctype = {"fb_qnet_t": L._vp, "fb_replay_t": L._vp, "fb_env_t": L._vp, "int": L._i, "double": L._d, "float": L._f, "uint64_t": L._u64}
    for decl in decls:
        name = decl.split("(")[0].split()[-1]
        args = [x.strip() for x in decl.split("(", 1)[1].rsplit(")", 1)[0].replace("/*f32[B]*/", "").replace("/*f32[6]*/", "").split(",")]
        want = [L._vp if "*" in x else ctype[x.split()[0]] for x in args]
        assert L.SIGNATURES[name] == want, name
    want = {"fb_qnet_sac_per_train_step": 14, "fb_sac_per_train_from_replay": 14, "fb_sac_per_step": 12,
            "fb_qnet_sac_train_step": 12, "fb_sac_train_from_replay": 12, "fb_sac_step": 12}          # (the uniform calls keep theirs)
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n, name
    # the uniform block keeps its text; the prioritized calls have a block of their own BEHIND the uniform declarations
    assert "not offered data-parallel SAC, bf16, prioritized replay, n-step returns, noisy or distributional critics, riders or the split schedule." in hdr
    assert hdr.index("int fb_sac_train_from_replay(") < hdr.index("prioritized SAC and n-step returns") < hdr.index("int fb_qnet_sac_per_train_step(")
    assert hdr.index("int fb_sac_step(") < hdr.index("int fb_sac_per_step(")
    for word in ("w is multiplied LAST in both", "abs_err[b] = 0.5f * (fabsf(d_1) + fabsf(d_2)), written UNWEIGHTED", "NOT weighted: L_pi, H, dLoss/dz_c",
                 "the intermediate steps carry NO entropy bonus", "y = done ? R : R + Gamma * V'(s')", "returns FB_ERR_STATE before any launch",
                 "uniform n-step SAC through the ring"):
        assert word in hdr, word
    src = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_sac.hip")).read()
    assert "template <int AT, bool PW>" in src and "static int sac_per_check_memory(" in src and "static int sac_check_memory(" in src
    qnet = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_qnet.hip")).read()
    assert "sac_loss_kernel" not in qnet                              # host routing only: the kernels stay in fb_sac.hip's code object
    from dqnflappybird_amd import vec
    assert not any("sac" in a for a in vec.ALGOS)                     # the prioritized form takes no `algo` either


# ---------------------------------------------------------------------------------------------------------------- the loss
@pytest.mark.parametrize("A", [2, 3, 8])
def test_np_weighted_loss_gradients_equal_autograd(A):
    """float32 in the pinned order against float64 autograd under tests/test_sac_host.py's bounds (float32's: the losses to 1e-5
    relative, a gradient element to 2e-6 of its tensor's largest); weights in [0.2, 1] with one exact 0 and one exact 1"""
    B, alpha = 37, 0.2
    rng = np.random.default_rng(7 * A)
    z, q1, q2, zn, q1n, q2n, a, r, t = sac_heads(rng, B, A)
    a[3] = A + 1                                                     # an action past the head reads A - 1
    w = (0.2 + 0.8 * rng.random(B)).astype(F32)
    w[0], w[1] = 0.0, 1.0
    assert ((w[2:] >= 0.2) & (w[2:] <= 1)).all()
    loss, dz, dq1, dq2, y, ae = np_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, alpha, w)
    tz, tq1, tq2 = (torch.tensor(x.astype(np.float64), requires_grad=True) for x in (z, q1, q2))
    tn = [torch.tensor(x.astype(np.float64)) for x in (zn, q1n, q2n)]
    out = torch_sac_per_loss(tz, tq1, tq2, *tn, a, r, t, 0.99, float(F32(alpha)), w)
    out[0].backward()
    np.testing.assert_allclose(loss[:5], [o.item() for o in out[:5]], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(y, out[5].numpy(), rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(ae, out[6].numpy(), rtol=1e-5, atol=1e-6)
    for got, ref in ((dz, tz.grad), (dq1, tq1.grad), (dq2, tq2.grad)):
        ref = ref.numpy()
        assert np.abs(ref).max() > 0
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * np.abs(ref).max())
    assert not dq1[0].any() and not dq2[0].any() and ae[0] > 0 and dz[0].any()       # w = 0: no critic gradient; the priority and the actor stay
    # unit weights: the uniform restatement's bits in every output
    l0, dz0, dq10, dq20, y0 = np_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, alpha)
    l1, dz1, dq11, dq21, y1, _ = np_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, alpha, np.ones(B, F32))
    for x, x0 in ((l1, l0), (dz1, dz0), (dq11, dq10), (dq21, dq20), (y1, y0)):
        assert np.array_equal(x.view(np.uint32), x0.view(np.uint32))
    # the actor's outputs and the entropy carry no weight
    assert np.array_equal(dz, dz0) and loss[3] == l0[3] and loss[4] == l0[4] and np.array_equal(y, y0)


def test_worked_case_with_half_weights():
    """every w = 0.5: dQ and m1 / m2 exactly half, dz / L_pi / H unchanged, abs_err = 0.5 (|d1| + |d2|) without the weight"""
    B, A = 16, 3
    rng = np.random.default_rng(5)
    z, q1, q2, zn, q1n, q2n, a, r, t = sac_heads(rng, B, A)
    l0, dz0, dq10, dq20, y0 = np_sac_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, 0.2)
    lh, dzh, dq1h, dq2h, yh, ae = np_sac_per_loss(z, q1, q2, zn, q1n, q2n, a, r, t, 0.99, 0.2, np.full(B, 0.5, F32))
    assert np.array_equal(dq1h, F32(0.5) * dq10) and np.array_equal(dq2h, F32(0.5) * dq20) and np.abs(dq10).max() > 0
    assert lh[1] == F32(0.5) * l0[1] and lh[2] == F32(0.5) * l0[2] and l0[1] > 0 and l0[2] > 0
    assert np.array_equal(dzh, dz0) and lh[3] == l0[3] and lh[4] == l0[4] and lh[5] == l0[5] and np.array_equal(yh, y0)
    ar = np.arange(B)
    d1, d2 = (q1[ar, a] - y0).astype(F32), (q2[ar, a] - y0).astype(F32)
    assert np.array_equal(ae, (F32(0.5) * (np.abs(d1) + np.abs(d2)).astype(F32)).astype(F32)) and (ae > 0).all()
    # one sample by hand: Q1(s, a) = 1.5, Q2(s, a) = -0.5, a terminal reward of 1 -> d = (0.5, -1.5), priority 1, weighted terms 0.125 / 1.125
    one = lambda v: np.array([[v, 0.0]], F32)
    l, _, g1, g2, y, e = np_sac_per_loss(one(0), one(1.5), one(-0.5), one(0), one(0), one(0), [0], [1.0], [1], 0.99, 0.2, [0.5])
    assert y[0] == 1 and e[0] == 1 and l[1] == F32(0.125) and l[2] == F32(1.125) and g1[0, 0] == F32(0.5) and g2[0, 0] == F32(-1.5)


def test_n_step_target_on_a_hand_made_row():
    """(R, done, Gamma) as the ring delivers them: the bootstrap's soft value is discounted by Gamma = gamma^n, a finished window's is dropped,
    and the restatement takes them where the one-step form takes (r, t, gamma)"""
    gamma, n = 0.99, 3
    Gamma = gamma ** n
    zn, q1n, q2n = np.array([[0.0, 0.0]], F32), np.array([[2.0, 4.0]], F32), np.array([[3.0, 1.0]], F32)
    alpha = 0.5
    Vn = 0.5 * (2.0 + alpha * np.log(2.0)) + 0.5 * (1.0 + alpha * np.log(2.0))       # p = (1/2, 1/2), min Q = (2, 1), -alpha log p = alpha ln 2
    R = F32(0.1 + gamma * 0.1 + gamma * gamma * 1.0)                   # the plain 3-step return: no entropy bonus on the way
    z, q = np.zeros((1, 2), F32), np.array([[1.0, 0.0]], F32)
    for done in (0, 1):
        _, _, _, _, y, ae = np_sac_per_loss(z, q, q, zn, q1n, q2n, [0], [R], [done], Gamma, alpha, [1.0])
        want = float(R) if done else float(R) + Gamma * Vn
        assert abs(float(y[0]) - want) < 1e-6 and abs(float(y[0]) - float(nstep_target(R, done, Gamma, F32(Vn)))) < 1e-6
        assert abs(float(ae[0]) - abs(1.0 - want)) < 1e-6
    assert nstep_target(F32(0.1), 1, Gamma, 5.0) == F32(0.1) and nstep_target(F32(0.1), 0, Gamma, 0.0) == F32(0.1)
    from dqnflappybird_amd.vec import bootstrap_gamma
    assert abs(bootstrap_gamma(gamma, n) - Gamma) < 1e-15 and bootstrap_gamma(gamma, 1) == gamma


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_vec_sac_prioritized_argument_checks():
    from dqnflappybird_amd import vecsac
    from dqnflappybird_amd.vecsac import VecSAC
    assert len(inspect.signature(vecsac.check_args).parameters) == 11          # the CLI and the tests call it positionally
    sig = inspect.signature(VecSAC.__init__).parameters
    assert sig["prioritized"].default is False and sig["n_step"].default == 1
    assert vecsac.check_replay(False, 1, 32, 100, 65536) == (False, 1) and vecsac.check_replay(np.bool_(True), 3, 32, 2, 96) == (True, 3)
    for bad in (1, 0, "yes", None, 0.5):
        with pytest.raises(ValueError, match="prioritized must be True or False"):
            VecSAC(32, prioritized=bad)
    with pytest.raises(ValueError, match="n_step = 3 needs prioritized=True: n-step SAC runs on the prioritized memory only"):
        VecSAC(32, n_step=3)
    for n in (0, 17, -1):
        with pytest.raises(ValueError, match="n_step must be in 1..16"):
            VecSAC(32, prioritized=True, n_step=n)
    with pytest.raises(ValueError, match="observe must be >= n_step - 1 = 2"):
        VecSAC(32, prioritized=True, n_step=3, observe=1)
    with pytest.raises(ValueError, match="capacity 64 < max\\(2, n_step\\) x n_envs = 96"):
        VecSAC(32, prioritized=True, n_step=3, capacity=64)
    # the uniform loop's checks come first, with their words
    with pytest.raises(ValueError, match="capacity 40 < 2 x n_envs = 64"):
        VecSAC(32, prioritized=True, capacity=40)
    with pytest.raises(ValueError, match="batch 64 > n_envs 32"):
        VecSAC(32, prioritized=True, batch=64)


def test_vec_surface_checks_before_the_gpu():
    from dqnflappybird_amd import vec

    class Mem:
        def __init__(self, per):
            self.prioritized = per

    class Net:
        arch = "sac"

        def _need_sac(self, what):
            vec.QNet._need_sac(self, what)

    with pytest.raises(ValueError, match="sac_per_train_from_replay trains from a prioritized memory only"):
        vec.sac_per_train_from_replay(Mem(False), Net(), None, None)
    with pytest.raises(ValueError, match="sac_train_from_replay trains from a uniform memory only"):
        vec.sac_train_from_replay(Mem(True), Net(), None)
    with pytest.raises(ValueError, match="SacStep trains from a uniform memory only"):
        vec.SacStep(None, Mem(True), Net())
    with pytest.raises(ValueError, match="SacPerStep trains from a prioritized memory only"):
        vec.SacPerStep(None, Mem(False), Net())
    with pytest.raises(ValueError, match="call env.track_state\\(\\) first"):
        vec.SacPerStep(object(), Mem(True), Net())
    Net.arch = "plain"
    with pytest.raises(ValueError, match="SacPerStep needs a SAC net"):
        vec.SacPerStep(None, Mem(True), Net())
    with pytest.raises(ValueError, match="sac_per_train_from_replay needs a SAC net"):
        vec.sac_per_train_from_replay(Mem(True), Net(), None, None)
    with pytest.raises(ValueError, match="sac_per_train_step needs a SAC net"):
        vec.QNet.sac_per_train_step(Net(), *[None] * 6)
    assert issubclass(vec.SacPerStep, vec.SacStep) and vec.SacPerStep.entry == "fb_sac_per_step" and vec.SacStep.entry == "fb_sac_step"
    ok = torch.ones(8)
    for bad in (None, torch.ones(7), torch.ones(8, dtype=torch.float64), torch.ones(8, 1), torch.ones(16)[::2]):
        with pytest.raises(ValueError, match="isw must be a contiguous float32\\[8\\]"):
            vec.check_isw(8, bad)
    vec.check_isw(8, ok)


def test_checkpoint_of_the_other_memory_kind_or_n_is_refused_by_name(tmp_path):
    """load() refuses before it touches anything of the object but its settings; a file without the keys is a uniform loop's at n = 1"""
    from dqnflappybird_amd.vecsac import VecSAC
    files = {}
    for kind, kw in (("old", {}), ("per1", dict(prioritized=np.array([1], np.int64), n_step=np.array([1], np.int64))),
                     ("per3", dict(prioritized=np.array([1], np.int64), n_step=np.array([3], np.int64)))):
        files[kind] = str(tmp_path / f"{kind}.npz")
        np.savez(files[kind], head=np.array(["sac"]), online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 1, 128, 0], np.int64), **kw)

    def loop(per, n):
        v = VecSAC.__new__(VecSAC)
        v.prioritized, v.n_step, v.n, v.batch, v.fc_width = per, n, 2, 1, 128
        return v

    for kind in ("per1", "per3"):
        with pytest.raises(ValueError, match="written by a VecSAC with a prioritized memory, this VecSAC has a uniform one \\(prioritized=False\\)"):
            loop(False, 1).load(files[kind])
    with pytest.raises(ValueError, match="written by a VecSAC with a uniform memory, this VecSAC has a prioritized one \\(prioritized=True\\)"):
        loop(True, 3).load(files["old"])
    with pytest.raises(ValueError, match="written with n_step = 3, this VecSAC has n_step = 1"):
        loop(True, 1).load(files["per3"])
    with pytest.raises(ValueError, match="written with n_step = 1, this VecSAC has n_step = 3"):
        loop(True, 3).load(files["per1"])
    # ... and a file of the loop's own kind passes both: the next check speaks
    for v, kind in ((loop(False, 1), "old"), (loop(True, 1), "per1"), (loop(True, 3), "per3")):
        with pytest.raises(ValueError, match="n_envs, batch, fc_width"):
            v.load(files[kind])


# ---------------------------------------------------------------------------------------------------------------- the command line
def run_cli(argv):
    return subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "sacper"], "--model sacper needs --vec"),
    (["--model", "sacper", "--vec", "32", "--alpha", "0"], "alpha must be finite and > 0"),
    (["--model", "sacper", "--vec", "32", "--alpha-lr", "-1"], "alpha_lr must be finite and >= 0"),
    (["--model", "sacper", "--vec", "32", "--polyak", "2"], "polyak (rho) must be in"),
    (["--model", "sacper", "--vec", "32", "--n-step", "17"], "n_step must be in 1..16"),
    (["--model", "sacper", "--vec", "32", "--n-step", "0"], "n_step must be in 1..16"),
    (["--model", "sacper", "--vec", "32", "--noisy"], "--noisy is not an option of --model sacper"),
    (["--model", "sacper", "--vec", "32", "--huber", "1"], "--huber is not an option of --model sacper"),
    (["--model", "sacper", "--vec", "32", "--tau", "0.1"], "--tau / --clip is not an option of --model sacper"),
    (["--model", "sacper", "--vec", "32", "--n-tau", "4"], "--n-tau need --model iqn, not --model sacper"),
    (["--model", "sacper", "--vec", "32", "--rollout", "5"], "--rollout need --model a2c"),
    # ... and the messages of before stay as they are
    (["--model", "sac", "--vec", "32", "--n-step", "3"], "--n-step is not an option of --model sac (--alpha, --target-entropy, --alpha-lr, --polyak, --max-grad-norm are)"),
    (["--model", "sac"], "--model sac needs --vec: discrete soft actor-critic runs in the vectorised loop only"),
    (["--model", "sac", "--vec", "32", "--noisy"], "--noisy is not an option of --model sac (--alpha"),
    (["--model", "iqnper", "--vec", "32", "--alpha-lr", "0.1"], "--alpha-lr need --model sac, not --model iqnper"),
    (["--model", "ddqn", "--vec", "32", "--target-entropy", "0.5"], "--target-entropy need --model sac, not --model ddqn"),
])
def test_cli_sacper_refusals(argv, msg):
    out = run_cli(argv)
    assert out.returncode == 2
    assert msg in out.stderr


@pytest.mark.parametrize("argv,want,keys", [
    (["--model", "sac", "--vec", "32"], dict(alpha=0.2, alpha_lr=0.0, polyak=0.005, batch=32), set()),
    (["--model", "sacper", "--vec", "32"], dict(prioritized=True, n_step=1, alpha=0.2, batch=32), {"prioritized", "n_step"}),
    (["--model", "sacper", "--vec", "16", "--n-step", "3", "--alpha", "0.1", "--alpha-lr", "1e-4", "--target-entropy", "0.5", "--polyak", "0.01",
      "--max-grad-norm", "5"], dict(prioritized=True, n_step=3, alpha=0.1, alpha_lr=1e-4, target_entropy=0.5, polyak=0.01, max_grad_norm=5.0, batch=16),
     {"prioritized", "n_step"}),
])
def test_cli_sacper_accepted_argument_lists(argv, want, keys):
    """what the parser hands VecSAC, without a GPU; --model sac's keywords are the ones of before"""
    from dqnflappybird_amd import FlappyBirdDQN as cli
    parser = cli.build_parser()
    args = parser.parse_args(argv)
    kw = cli.sac_kwargs(args, parser)
    assert {k: kw[k] for k in want} == want
    assert set(kw) == {"alpha", "target_entropy", "alpha_lr", "polyak", "max_grad_norm", "batch"} | keys
    assert cli.iqn_kwargs(args, parser) is None and cli.a2c_kwargs(args, parser) is None
