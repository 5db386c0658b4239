"""Munchausen IQN, the host side (include/fbdqn.h, the Munchausen IQN block): the target in float64 numpy and, written apart from it, in
float32 numpy in the header's order; the decomposition of the soft value; the one-hot limit, bit for bit; the conditioning bound the GPU
tests take their tolerance of T from, tol_bj = Q_ATOL (4 + S_bj / temp); the refusals that need no GPU (check_munchausen, VecIQN, the
command line) and the checkpoint key.  tests/test_gpu_miqn.py imports the helpers."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_qnet import Q_ATOL
from tests.test_iqn_host import F32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = 0.99
PARAMS = [(1.0, 0.9, -1.0), (0.03, 0.9, -1.0)]               # (temp, alpha, l0): the issue's two settings


def lse(x, temp):
    """temp log sum_c exp(x_c / temp) over the last axis, float64"""
    x = np.asarray(x, np.float64)
    m = x.max(-1, keepdims=True)
    return (m + temp * np.log(np.exp((x - m) / temp).sum(-1, keepdims=True)))[..., 0]


def miqn_target64(qn, qs, th, a, r, t, gamma, temp, alpha, l0):
    """the Munchausen IQN target in float64: qn = Qbar-(s', .) [B, A], qs = Qbar-(s, .) [B, A], th = theta-(s', c; tau'_j) [B, N', A],
    stored actions a, rewards r (0.1f reads as 0.1), terminals t -> dict(T [B, N'], V, bonus [B], x = temp ln pi(a|s) [B], S [B, N'])"""
    qn, qs, th = (np.asarray(v, np.float64) for v in (qn, qs, th))
    temp, alpha, l0 = (float(F32(v)) for v in (temp, alpha, l0))
    A = qn.shape[1]
    ab = np.minimum(np.asarray(a, np.int64), A - 1)
    tl = qn - lse(qn, temp)[:, None]                                   # temp ln pi_c
    pi = np.exp(tl / temp)
    V = (pi[:, None, :] * (th - tl[:, None, :])).sum(2)
    x = qs[np.arange(len(qs)), ab] - lse(qs, temp)
    bonus = alpha * np.maximum(x, l0)
    rd = np.where(np.asarray(r, F32) == F32(0.1), 0.1, np.asarray(r, np.float64))
    T = (rd + bonus)[:, None] + np.where(np.asarray(t) != 0, 0.0, 1.0)[:, None] * gamma * V
    d = th - qn[:, None, :]
    return dict(T=T, V=V, bonus=bonus, x=x, S=d.max(2) - d.min(2))


def miqn_target32(qn, qs, th, a, r, t, gamma, temp, alpha, l0):
    """the same in float32 numpy, every operation and its order as include/fbdqn.h pins them (ascending c, a multiply then an add, the sums
    of T in float64 and one rounding) -> (T f32[B, N'], V f32[B, N'], pi f32[B, A], tl f32[B, A], bonus f32[B])"""
    qn, qs, th = (np.asarray(v, F32) for v in (qn, qs, th))
    temp, alpha, l0 = F32(temp), F32(alpha), F32(l0)
    B, A = qn.shape
    Np = th.shape[1]
    T, V = np.empty((B, Np), F32), np.empty((B, Np), F32)
    pi, tl, bonus = np.empty((B, A), F32), np.empty((B, A), F32), np.empty(B, F32)
    with np.errstate(under="ignore"):
        for b in range(B):
            m = qn[b, 0]
            for c in range(1, A):
                m = max(m, qn[b, c])
            e, s = np.empty(A, F32), F32(0)
            for c in range(A):
                e[c] = np.exp(F32(F32(qn[b, c] - m) / temp))
                s = F32(s + e[c])
            ln = F32(temp * np.log(s))
            for c in range(A):
                pi[b, c] = F32(e[c] / s)
                tl[b, c] = F32(F32(qn[b, c] - m) - ln)
            ms = qs[b, 0]
            for c in range(1, A):
                ms = max(ms, qs[b, c])
            ss = F32(0)
            for c in range(A):
                ss = F32(ss + np.exp(F32(F32(qs[b, c] - ms) / temp)))
            ab = min(int(a[b]), A - 1)
            bonus[b] = F32(alpha * max(F32(F32(qs[b, ab] - ms) - F32(temp * np.log(ss))), l0))
            rd = (0.1 if F32(r[b]) == F32(0.1) else float(r[b])) + float(bonus[b])
            for j in range(Np):
                v = F32(0)
                for c in range(A):
                    v = F32(v + F32(pi[b, c] * F32(th[b, j, c] - tl[b, c])))
                V[b, j] = v
                T[b, j] = F32(rd if t[b] else rd + gamma * float(v))
    return T, V, pi, tl, bonus


def miqn_tol(S, temp):
    """the tolerance of T at (b, j): Q_ATOL (4 + S_bj / temp).  To first order |dV_j| <= |dtheta| + |dq'| (1 + S_bj / (2 temp)) -- V_j =
    sum_c pi_c d_c + lse_temp(q') with d_c = theta_cj - q'_c: the weights pi move by at most |dq'| / temp in total variation against a
    spread S_bj of d, the lse by |dq'|, d by |dtheta| + |dq'| -- and the bonus by <= 2 alpha |dq|; with |dtheta|, |dq'|, |dq| <= Q_ATOL (the
    project's bound on theta and Qbar) that is Q_ATOL (4 + S_bj / (2 temp)); S / temp leaves the second order its half"""
    return Q_ATOL * (4.0 + np.asarray(S, np.float64) / float(F32(temp)))


# ================================================================================================================ the arithmetic
@pytest.mark.parametrize("temp", [1.0, 0.03, 1e-3])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_the_soft_value_decomposes(A, temp):
    """sum_c pi_c (theta_c - temp ln pi_c) = sum_c pi_c (theta_c - q'_c) + lse_temp(q')"""
    rng = np.random.default_rng(A)
    temp = float(F32(temp))                                              # (the net holds a float32)
    qn, th = rng.normal(size=(50, A)), rng.normal(size=(50, 7, A)) * 2
    tl = qn - lse(qn, temp)[:, None]
    pi = np.exp(tl / temp)
    assert np.abs(pi.sum(1) - 1).max() < 1e-12
    with np.errstate(divide="ignore", invalid="ignore"):
        by_log = np.where(pi > 0, pi * np.log(pi), 0.0)                 # (temp = 1e-3: pi underflows; 0 ln 0 = 0)
    lhs = (pi[:, None, :] * th).sum(2) - temp * by_log.sum(1)[:, None]
    rhs = (pi[:, None, :] * (th - qn[:, None, :])).sum(2) + lse(qn, temp)[:, None]
    assert np.abs(lhs - rhs).max() <= 1e-12
    out = miqn_target64(qn, qn, th, np.zeros(50, np.int64), np.zeros(50, F32), np.zeros(50, np.uint8), 1.0, temp, 0.0, 0.0)
    assert np.abs(out["V"] - rhs).max() <= 1e-12 and np.array_equal(out["T"], out["V"])


@pytest.mark.parametrize("temp", [1e-6, 0.03, 1.0])
@pytest.mark.parametrize("A", [2, 3, 8])
def test_a_gap_of_104_temp_makes_the_policy_one_hot_bit_for_bit(A, temp):
    """the float32 restatement with every gap of q' >= 104 temp: pi is exactly one-hot, every t_c finite (t = 0 at the maximum), no NaN,
    and V_j is theta(a*, j), bit for bit -- the hard target"""
    rng = np.random.default_rng(A + 7)
    B, Np = 40, 5
    gap = F32(104.0) * F32(temp) * F32(1.0 + 2.0 ** -10)
    best = rng.integers(0, A, B)
    qn = (rng.normal(size=(B, 1)) + np.zeros((B, A))).astype(F32)
    for b in range(B):
        for c in range(A):
            if c != best[b]:
                qn[b, c] = F32(qn[b, best[b]] - gap * F32(1 + 3 * rng.random()))
        assert all(F32(qn[b, best[b]] - qn[b, c]) >= F32(104.0) * F32(temp) for c in range(A) if c != best[b])
    th = (rng.normal(size=(B, Np, A)) * 3).astype(F32)
    r = rng.choice(np.array([0.1, 3, -3], F32), B)
    t = (rng.random(B) < 0.3).astype(np.uint8)
    T, V, pi, tl, bonus = miqn_target32(qn, qn, th, best, r, t, GAMMA, temp, 0.0, -1.0)
    assert np.isfinite(T).all() and np.isfinite(V).all() and np.isfinite(tl).all() and np.isfinite(pi).all()
    onehot = np.zeros((B, A), F32)
    onehot[np.arange(B), best] = 1
    assert np.array_equal(pi, onehot) and (tl[np.arange(B), best] == 0).all() and (tl <= 0).all()
    want = th[np.arange(B), :, best]
    assert np.array_equal(V.view(np.uint32), (want + F32(0)).view(np.uint32))
    rd = np.where(r == F32(0.1), 0.1, r.astype(np.float64))
    hard = np.where(t[:, None] != 0, rd[:, None], rd[:, None] + GAMMA * want.astype(np.float64)).astype(F32)
    assert np.array_equal(T, hard) and not bonus.any()                # alpha = 0: the IQN target with double_q = 0


def test_the_worked_bonus_values_are_munchausen_dqns():
    """include/fbdqn.h's worked bonus values of the Munchausen-DQN block, through both restatements"""
    th = np.zeros((1, 1, 2))
    for qs, a, want in (((1.5, 1.5), 0, -0.9 * 0.03 * np.log(2)), ((0.0, 2.0), 0, -0.9), ((0.0, 2.0), 1, 0.0)):
        o = miqn_target64(np.zeros((1, 2)), np.array([qs]), th, [a], [0.0], [1], GAMMA, 0.03, 0.9, -1.0)
        assert abs(o["bonus"][0] - want) < 1e-7 and abs(o["T"][0, 0] - want) < 1e-7       # the bonus reaches a terminal transition's target
        b32 = miqn_target32(np.zeros((1, 2)), np.array([qs]), th, [a], [0.0], [1], GAMMA, 0.03, 0.9, -1.0)[4]
        assert abs(float(b32[0]) - want) < 1e-6


# ================================================================================================================ the bound
@pytest.mark.parametrize("temp,alpha,l0", PARAMS)
def test_conditioning_bound_on_the_gpu_tests_inputs(oracle, temp, alpha, l0):
    """the inputs of tests/test_gpu_miqn.py's first shape at B = 32: the float32 restatement on float32 roundings of the float64 Qbar and
    theta, and again on inputs moved by +-Q_ATOL with the worst signs (q' up where d_c is largest and down where it is smallest, theta
    and q with random signs), against the float64 target under tol_bj.  Only Q_ATOL enters the tolerance"""
    from tests.test_gpu_miqn import ref_inputs
    from tests.test_gpu_iqn import SHAPES
    s, a, r, s2, t, tau, taup, qn, qs, th = ref_inputs(oracle, SHAPES[0], 32, False)
    ref = miqn_target64(qn, qs, th, a, r, t, GAMMA, temp, alpha, l0)
    tol = miqn_tol(ref["S"], temp)
    T32 = miqn_target32(qn, qs, th, a, r, t, GAMMA, temp, alpha, l0)[0]
    ratio = np.abs(T32 - ref["T"]) / tol
    print(f"temp={temp}: S in [{ref['S'].min():.3e}, {ref['S'].max():.3e}], tol in [{tol.min():.3e}, {tol.max():.3e}]; fp32 restatement on rounded inputs: "
          f"largest |T32 - T64| / tol {ratio.max():.3e}")
    assert (ratio <= 1).all()
    rng = np.random.default_rng(32)
    worst = 0.0
    for j in range(th.shape[1]):                                         # the worst signs are those of tau'_j's own d
        d = th[:, j, :] - qn
        sg = np.where(d >= np.median(d, 1, keepdims=True), 1.0, -1.0)
        for flip in (1.0, -1.0):
            qn_p = qn + flip * sg * Q_ATOL
            th_p = th + rng.choice([-1.0, 1.0], th.shape) * Q_ATOL
            qs_p = qs + rng.choice([-1.0, 1.0], qs.shape) * Q_ATOL
            Tp = miqn_target32(qn_p, qs_p, th_p, a, r, t, GAMMA, temp, alpha, l0)[0]
            rj = np.abs(Tp[:, j] - ref["T"][:, j]) / tol[:, j]
            worst = max(worst, rj.max())
            assert (rj <= 1).all(), (j, flip)
    print(f"temp={temp}: inputs moved by +-Q_ATOL with the worst signs: largest |T32 - T64| / tol {worst:.3e}")


# ================================================================================================================ Python refusals
def test_check_munchausen():
    from dqnflappybird_amd import veciqn
    assert len(inspect.signature(veciqn.check_args).parameters) == 18          # the CLI and the tests call it positionally
    assert veciqn.check_munchausen(False, 0.03, 0.9, -1.0) == (False, float(F32(0.03)), float(F32(0.9)), -1.0)
    assert veciqn.check_munchausen(np.bool_(True), 1, 0, 0)[0] is True and veciqn.check_munchausen(False, 0.03, 0.9, -1.0, True)[0] is False
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="munchausen must be True or False"):
            veciqn.check_munchausen(bad, 0.03, 0.9, -1.0)
    for kw, msg in ((dict(temp=0.0), "temp must be finite and > 0"), (dict(temp=float("nan")), "temp must be finite and > 0"),
                    (dict(temp=float("inf")), "temp must be finite and > 0"), (dict(alpha=1.5), "alpha must be in \\[0, 1\\]"),
                    (dict(alpha=-0.1), "alpha must be in \\[0, 1\\]"), (dict(clip=0.5), "clip \\(l0\\) must be finite and <= 0"),
                    (dict(clip=float("-inf")), "clip \\(l0\\) must be finite and <= 0")):
        args = {**dict(temp=0.03, alpha=0.9, clip=-1.0), **kw}
        for on in (True, False):
            with pytest.raises(ValueError, match=msg):
                veciqn.check_munchausen(on, args["temp"], args["alpha"], args["clip"])
        with pytest.raises(ValueError, match=msg):                       # ... before anything touches the GPU
            veciqn.VecIQN(32, munchausen=True, **kw)
    with pytest.raises(ValueError, match="munchausen=True with double_q=True"):
        veciqn.check_munchausen(True, 0.03, 0.9, -1.0, True)
    with pytest.raises(ValueError, match="munchausen=True with double_q=True"):
        veciqn.VecIQN(32, munchausen=True, double_q=True)
    with pytest.raises(ValueError, match="munchausen must be True or False"):
        veciqn.VecIQN(32, munchausen=1)
    with pytest.raises(ValueError, match="batch 64 > n_envs 32"):              # the other checks come first
        veciqn.VecIQN(32, munchausen=True, double_q=True, batch=64)
    sig = inspect.signature(veciqn.VecIQN.__init__).parameters
    assert [sig[k].default for k in ("munchausen", "temp", "alpha", "clip")] == [False, 0.03, 0.9, -1.0]


def test_the_binding_declares_the_two_calls():
    from dqnflappybird_amd import _lib as L
    import ctypes as C
    assert L.SIGNATURES["fb_qnet_set_iqn_munchausen"] == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float]
    assert L.SIGNATURES["fb_qnet_get_iqn_munchausen"] == [C.c_void_p] * 5
    text = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "int fb_qnet_set_iqn_munchausen(fb_qnet_t h, int on, float temp, float alpha, float clip_lo);" in text
    assert "int fb_qnet_get_iqn_munchausen(fb_qnet_t h, int *on_host, float *temp_host, float *alpha_host, float *clip_lo_host);" in text
    assert text.index("fb_qnet_create_iqn_dueling(int") < text.index("Munchausen IQN (M-IQN") < text.index("int fb_qnet_set_iqn_munchausen")


def test_checkpoints_record_the_target(tmp_path):
    from dqnflappybird_amd.veciqn import VecIQN
    files = {}
    for kind, kw in (("old", {}), ("off", dict(munchausen=np.array([0.0, 0.03, 0.9, -1.0]))), ("on", dict(munchausen=np.array([1.0, 0.5, 0.9, -1.0])))):
        files[kind] = str(tmp_path / f"{kind}.npz")
        np.savez(files[kind], head=np.array(["iqn"]), online=np.zeros(3, np.float32), scalars=np.array([0, 7, 2, 1, 128, 0, 1, 1, 0, 1], np.int64),
                 iqn=np.array([8, 8, 32, 1.0, 1.0]), **kw)

    def mk(mu, temp=0.5):
        v = VecIQN.__new__(VecIQN)
        v.__dict__.update(prioritized=False, dueling=False, munchausen=mu, temp=temp, alpha=0.9, clip=-1.0, n=2, batch=1, fc_width=128, n_step=1, seed=7,
                          n_tau=8, n_tau_next=8, n_tau_act=32, kappa=1.0)
        return v
    with pytest.raises(ValueError, match="written by a VecIQN with the Munchausen target, this VecIQN has the hard one \\(munchausen=False\\)"):
        mk(False).load(files["on"])
    for kind in ("old", "off"):                                          # a file without the key is the hard target's
        with pytest.raises(ValueError, match="written by a VecIQN with the hard target, this VecIQN has the Munchausen one \\(munchausen=True\\)"):
            mk(True).load(files[kind])
    with pytest.raises(ValueError, match="was trained with munchausen \\(temp, alpha, clip\\) = \\(0.5, 0.9, -1.0\\), this VecIQN has \\(0.25, 0.9, -1.0\\)"):
        mk(True, 0.25).load(files["on"])
    for v, kind in ((mk(False), "old"), (mk(False), "off"), (mk(True), "on")):        # a match gets past the check (and ends at the stub's missing net)
        with pytest.raises(AttributeError, match="no attribute 'net'"):
            v.load(files[kind])


def test_evaluate_ignores_the_key():
    src = open(os.path.join(ROOT, "dqnflappybird_amd", "evaluate.py")).read()
    assert "munchausen" not in src                                       # greedy play is unchanged: the checkpoint reader never asks


# ================================================================================================================ the command line
@pytest.mark.parametrize("argv,msg", [
    (["--model", "rainbowiqn", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model rainbowiqn"),
    (["--model", "ddqn", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model ddqn"),
    (["--model", "mdqn", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model mdqn"),
    (["--model", "qrdqn", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model qrdqn"),
    (["--model", "rainbow", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model rainbow"),
    (["--model", "sac", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model sac"),
    (["--model", "a2c", "--vec", "32", "--munchausen"], "--munchausen needs --model iqn or --model iqnper, not --model a2c"),
    (["--model", "iqn", "--munchausen"], "--model iqn needs --vec"),
    (["--model", "iqn", "--vec", "32", "--munchausen", "--double"], "--munchausen with --double"),
    (["--model", "iqn", "--vec", "32", "--munchausen", "--tau", "0"], "--tau must be finite and > 0"),
    (["--model", "iqnper", "--vec", "32", "--munchausen", "--alpha", "2"], "alpha must be in [0, 1]"),
    (["--model", "iqnper", "--vec", "32", "--munchausen", "--clip", "1"], "clip (l0) must be finite and <= 0"),
    (["--model", "iqn", "--vec", "32", "--munchausen", "--noisy"], "--noisy is not an option of --model iqn"),
    (["--model", "iqn", "--vec", "32", "--tau", "0.1"], "--tau / --alpha / --clip is not an option of --model iqn"),
    (["--model", "iqnper", "--vec", "32", "--alpha", "0.5"], "--tau / --alpha / --clip is not an option of --model iqnper"),
    (["--model", "rainbowiqn", "--vec", "32", "--clip", "-1"], "--tau / --alpha / --clip is not an option of --model rainbowiqn"),
])
def test_cli_munchausen_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr


def test_cli_passes_munchausen_to_the_loop():
    from dqnflappybird_amd.FlappyBirdDQN import build_parser, iqn_kwargs
    parser = build_parser()
    for model, per in (("iqn", False), ("iqnper", True)):
        kw = iqn_kwargs(parser.parse_args(["--model", model, "--vec", "64", "--munchausen"]), parser)
        assert kw["munchausen"] is True and (kw["temp"], kw["alpha"], kw["clip"]) == (float(F32(0.03)), float(F32(0.9)), -1.0)
        assert kw["prioritized"] is per and kw["double_q"] is False
        kw = iqn_kwargs(parser.parse_args(["--model", model, "--vec", "64", "--munchausen", "--tau", "0.5", "--alpha", "0.25", "--clip", "-2",
                                           "--dueling", "--n-step", "3", "--cvar", "0.5", "--polyak", "0.01", "--max-grad-norm", "5"]), parser)
        assert (kw["temp"], kw["alpha"], kw["clip"]) == (0.5, 0.25, -2.0) and kw["dueling"] is True and kw["n_step"] == 3 and kw["cvar"] == 0.5
        kw = iqn_kwargs(parser.parse_args(["--model", model, "--vec", "64"]), parser)
        assert not {"munchausen", "temp", "alpha", "clip"} & set(kw)          # without the flag the models stay what they are
