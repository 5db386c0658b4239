"""Prioritized IQN, the host side: the ABI's declarations of the three calls, the float64 restatements of the importance-weighted
quantile Huber loss (numpy loops and torch autograd; they must agree), the header's N = 2 worked case under a weight of 0.5, the command
line of --model iqnper / rainbowiqn, and VecIQN's new argument checks.  tests/test_gpu_iqn_per.py imports the helpers."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_iqn_host import F32, WORKED, np_iqn_loss, torch_iqn_loss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_iqn_per_loss(theta, T, tau, kappa, w):
    """the weighted loss in float64 torch: mean_b w_b l_b -> (loss, l_b [B], unweighted: the priorities)"""
    _, lb = torch_iqn_loss(theta, T, tau, kappa)
    return (torch.as_tensor(np.asarray(w, np.float64)) * lb).mean(), lb


def np_iqn_per_loss(theta, T, tau, kappa, w):
    """the same in float64 numpy, with the gradient as include/fbdqn.h forms it: that of l_b / B, times w_b
    -> (loss, l_b [B], dloss/dtheta [B, N])"""
    lb, g = np_iqn_loss(theta, T, tau, kappa)
    w = np.asarray(w, np.float64)
    loss = 0.0
    for b in range(len(lb)):
        loss += w[b] * lb[b]
    return loss / len(lb), lb, g * w[:, None]


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_prioritized_iqn_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("int fb_qnet_iqn_per_train_step(fb_qnet_t h, int double_q, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,",
                 "int fb_iqn_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, const float *isw",
                 "int fb_iqn_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q, int batch, float epsilon,"):
        assert decl in hdr, decl
    want = {"fb_qnet_iqn_per_train_step": 19, "fb_iqn_per_train_from_replay": 19, "fb_iqn_per_step": 13,
            "fb_qnet_iqn_train_step": 17, "fb_iqn_train_from_replay": 17, "fb_iqn_step": 13}       # (the uniform calls keep theirs)
    for name, n in want.items():
        assert len(L.SIGNATURES[name]) == n, name
    # the uniform block keeps its "not offered" line; the prioritized calls have a block of their own BELOW the three uniform declarations
    assert "not offered prioritized replay, dueling or noisy IQN" in hdr
    assert hdr.index("int fb_iqn_train_from_replay(") < hdr.index("prioritized IQN: the three calls above") < hdr.index("int fb_qnet_iqn_per_train_step(")
    for word in ("the weight multiplied LAST", "abs_err[b] = l_b, WITHOUT the weight", "w = 1 gives the uniform call's loss, T and gradient bit for bit",
                 "IN LINE at every env count: no side stream, no sample-ahead, no riders"):
        assert word in hdr, word
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    src = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_iqn.hip")).read()
    assert "const float *isw; float *abs_err;" in common.split("struct IqnLossArgs {")[1].split("};")[0].splitlines()[-1]     # at the END of the struct
    assert "template <int AT, bool PW>" in src
    from dqnflappybird_amd import vec
    assert not any("iqn" in a for a in vec.ALGOS)                    # the prioritized form takes no `algo` either


# ---------------------------------------------------------------------------------------------------------------- the loss
def test_worked_case_with_half_weight():
    """the header's N = 2 QR case (kappa 1, theta [0, 1], T [0.5, 3]: l = 0.90625, dl/dtheta = [-0.1875, -0.3125]) with w = 0.5"""
    kappa, tau, theta, T, l, g = WORKED[0]
    assert (l, g) == (0.90625, [-0.1875, -0.3125])
    for B in (1, 4):                                                 # the sample alone, and as one of B (the others weigh nothing)
        th = np.array([theta] * B)
        w = np.array([0.5] + [0.0] * (B - 1))
        loss, lb, dg = np_iqn_per_loss(th, [T] * B, [tau] * B, kappa, w)
        assert lb[0] == 0.90625 and lb[0] * w[0] == 0.453125 and abs(loss - 0.453125 / B) < 1e-14
        np.testing.assert_allclose(dg[0], np.array([-0.09375, -0.15625]) / B, rtol=0, atol=1e-14)
        assert not dg[1:].any()
        tt = torch.tensor(th, dtype=torch.float64, requires_grad=True)
        tl, tlb = torch_iqn_per_loss(tt, torch.tensor([T] * B, dtype=torch.float64), [tau] * B, kappa, w)
        tl.backward()
        assert abs(tl.item() - 0.453125 / B) < 1e-14 and abs(tlb[0].item() - 0.90625) < 1e-14       # the priority carries no weight
        np.testing.assert_allclose(tt.grad.numpy()[0], np.array([-0.09375, -0.15625]) / B, rtol=0, atol=1e-14)


@pytest.mark.parametrize("N,Np,kappa", [(8, 8, 1.0), (5, 7, 0.5), (64, 64, 2.0), (1, 1, 1.0)])
def test_torch_and_numpy_weighted_restatements_agree(N, Np, kappa):
    B = 9
    rng = np.random.default_rng(N * 100 + Np + 1)
    theta, T = rng.normal(size=(B, N)) * 2, rng.normal(size=(B, Np)) * 2
    tau = rng.random((B, N)).astype(F32)
    w = 1.0 - rng.random(B)                                          # (0, 1]
    w[0], w[1] = 1.0, 0.0                                            # ... and the two ends
    loss, lb, g = np_iqn_per_loss(theta, T, tau, kappa, w)
    th = torch.tensor(theta, requires_grad=True)
    tl, tlb = torch_iqn_per_loss(th, torch.tensor(T), tau, kappa, w)
    tl.backward()
    assert abs(tl.item() - loss) < 1e-14 * max(1.0, abs(loss))
    np.testing.assert_allclose(tlb.detach().numpy(), lb, rtol=1e-14)
    np.testing.assert_allclose(th.grad.numpy(), g, rtol=1e-12, atol=1e-14)
    assert not th.grad.numpy()[1].any() and (lb >= 0).all() and lb[1] > 0        # w = 0: no gradient, the priority stays
    # w = 1 everywhere: the uniform loss and gradient
    l1, _, g1 = np_iqn_per_loss(theta, T, tau, kappa, np.ones(B))
    lb0, g0 = np_iqn_loss(theta, T, tau, kappa)
    assert abs(l1 - lb0.mean()) < 1e-14 * max(1.0, l1) and np.array_equal(g1, g0)


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_vec_iqn_prioritized_argument_checks():
    import inspect
    from dqnflappybird_amd import veciqn
    assert len(inspect.signature(veciqn.check_args).parameters) == 18          # the CLI and the tests call it positionally
    assert veciqn.check_prioritized(False) is False and veciqn.check_prioritized(True) is True and veciqn.check_prioritized(np.bool_(True)) is True
    for bad in (1, 0, "yes", None, 0.5):
        with pytest.raises(ValueError, match="prioritized must be True or False"):
            veciqn.check_prioritized(bad)
        with pytest.raises(ValueError, match="prioritized must be True or False"):
            veciqn.VecIQN(32, prioritized=bad)
    assert inspect.signature(veciqn.VecIQN.__init__).parameters["prioritized"].default is False
    # the other checks come first and are the uniform loop's
    with pytest.raises(ValueError, match="observe must be >= n_step - 1 = 2"):
        veciqn.VecIQN(32, prioritized=True, observe=1, n_step=3)
    with pytest.raises(ValueError, match="batch 64 > n_envs 32"):
        veciqn.VecIQN(32, prioritized=True, batch=64)


def test_checkpoint_of_the_other_memory_kind_is_refused_by_name(tmp_path):
    """load() refuses before it touches anything of the object but its settings; a file without the key is a uniform loop's"""
    from dqnflappybird_amd.veciqn import VecIQN
    files = {}
    for kind, kw in (("old", {}), ("uniform", dict(prioritized=np.array([0], np.int64))), ("per", dict(prioritized=np.array([1], np.int64)))):
        files[kind] = str(tmp_path / f"{kind}.npz")
        np.savez(files[kind], head=np.array(["iqn"]), online=np.zeros(3, np.float32), scalars=np.array([0, 0, 1, 1, 128, 0, 1, 1, 0, 1], np.int64), **kw)
    u, p = VecIQN.__new__(VecIQN), VecIQN.__new__(VecIQN)
    u.prioritized, p.prioritized = False, True
    with pytest.raises(ValueError, match="written by a VecIQN with a prioritized memory, this VecIQN has a uniform one"):
        u.load(files["per"])
    for kind in ("old", "uniform"):
        with pytest.raises(ValueError, match="written by a VecIQN with a uniform memory, this VecIQN has a prioritized one"):
            p.load(files[kind])
        u.n, u.batch, u.fc_width, u.n_step = 2, 1, 128, 1               # ... and passes that check in a uniform loop: the next one speaks
        with pytest.raises(ValueError, match="n_envs, batch, fc_width, n_step"):
            u.load(files[kind])


def test_vec_surface_checks_before_the_gpu():
    from dqnflappybird_amd import vec
    ok = torch.ones(8)
    vec.check_isw(8, ok)
    for bad in (None, torch.ones(7), torch.ones(8, dtype=torch.float64), torch.ones(8, 1), torch.ones(16)[::2]):
        with pytest.raises(ValueError, match="isw must be a contiguous float32\\[8\\]"):
            vec.check_isw(8, bad)

    class Mem:
        def __init__(self, per):
            self.prioritized = per

    class Net:
        arch = "iqn"

    for name in ("iqn_train_from_replay", "x"):
        with pytest.raises(ValueError, match="uniform memory only"):
            vec._ring_call(name, Mem(True), Net(), "iqn", "an IQN net", "trains from", None, 1)
    with pytest.raises(ValueError, match="iqn_per_train_from_replay trains from a prioritized memory only"):
        vec._ring_call("iqn_per_train_from_replay", Mem(False), Net(), "iqn", "an IQN net", "trains from", None, 1, prioritized=True)
    with pytest.raises(ValueError, match="IqnStep trains from a uniform memory only"):
        vec.IqnStep(None, Mem(True), Net())
    with pytest.raises(ValueError, match="IqnPerStep trains from a prioritized memory only"):
        vec.IqnPerStep(None, Mem(False), Net())
    Net.arch = "plain"
    with pytest.raises(ValueError, match="IqnPerStep needs an IQN net"):
        vec.IqnPerStep(None, Mem(True), Net())


# ---------------------------------------------------------------------------------------------------------------- the command line
def run_cli(argv):
    return subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "iqnper"], "--model iqnper needs --vec"),
    (["--model", "rainbowiqn"], "--model rainbowiqn needs --vec"),
    (["--model", "iqnper", "--vec", "32", "--n-tau", "0"], "n_tau must be an integer in 1..64"),
    (["--model", "iqnper", "--vec", "32", "--n-tau-target", "65"], "n_tau_next must be an integer in 1..64"),
    (["--model", "iqnper", "--vec", "32", "--kappa", "0"], "kappa must be finite and > 0"),
    (["--model", "rainbowiqn", "--vec", "32", "--cvar", "1.5"], "eta (CVaR level) must be in (0, 1]"),
    (["--model", "rainbowiqn", "--vec", "32", "--n-step", "17"], "n_step must be in 1..16"),
    (["--model", "iqnper", "--vec", "32", "--noisy"], "--noisy is not an option of --model iqnper"),
    (["--model", "rainbowiqn", "--vec", "32", "--noisy"], "--noisy is not an option of --model rainbowiqn"),
    (["--model", "iqnper", "--vec", "32", "--huber", "1"], "--huber is not an option of --model iqnper"),
    (["--model", "iqnper", "--vec", "32", "--n-quantiles", "8"], "--n-quantiles is not an option of --model iqnper"),
    (["--model", "iqnper", "--vec", "32", "--alpha-lr", "0.1"], "--alpha-lr need --model sac"),
    (["--model", "iqnper", "--vec", "32", "--rollout", "5"], "--rollout need --model a2c"),
    # ... and the messages of before stay as they are
    (["--model", "qrdqn", "--vec", "32", "--n-tau", "4"], "--n-tau need --model iqn, not --model qrdqn"),
    (["--model", "iqn", "--vec", "32", "--noisy"], "--noisy is not an option of --model iqn (--n-tau"),
    (["--model", "iqn"], "--model iqn needs --vec"),
])
def test_cli_iqnper_refusals(argv, msg):
    out = run_cli(argv)
    assert out.returncode == 2
    assert msg in out.stderr


@pytest.mark.parametrize("argv,want", [
    (["--model", "iqn", "--vec", "32"], dict(prioritized=False, double_q=False, n_step=1)),
    (["--model", "iqnper", "--vec", "32"], dict(prioritized=True, double_q=False, n_step=1)),
    (["--model", "iqnper", "--vec", "32", "--double", "--n-step", "3", "--n-tau", "4", "--cvar", "0.5"],
     dict(prioritized=True, double_q=True, n_step=3, n_tau=4, cvar=0.5)),
    (["--model", "rainbowiqn", "--vec", "16", "--n-step", "3", "--polyak", "0.01"], dict(prioritized=True, double_q=True, n_step=3, polyak=0.01, batch=16)),
])
def test_cli_iqnper_accepted_argument_lists(argv, want):
    """what the parser hands VecIQN, without a GPU"""
    from dqnflappybird_amd import FlappyBirdDQN as cli
    parser = cli.build_parser()
    kw = cli.iqn_kwargs(parser.parse_args(argv), parser)
    assert {k: kw[k] for k in want} == want
    assert set(kw) == {"batch", "double_q", "n_step", "n_tau", "n_tau_next", "n_tau_act", "kappa", "cvar", "polyak", "max_grad_norm", "prioritized"}
