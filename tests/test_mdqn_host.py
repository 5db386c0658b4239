"""Munchausen-DQN (include/fbdqn.h: FB_ALGO_MDQN / FB_ALGO_MDQN_PER) without a GPU: the float64 restatement of the target the GPU tests
compare the kernels with (np_mdqn_target: the stable log-sum-exp form the header pins) against the paper's own form -- the explicit
softmax pi = softmax(q / tau), V = sum_c pi_c (q_c - tau ln pi_c) and the bonus alpha max(tau ln pi_a, l0) -- evaluated in 60-digit
decimal arithmetic, where exp(+-2000) neither overflows nor underflows; the header's hand cases; the ABI declarations; and every
refusal the Python layers make before anything touches the GPU."""
import ctypes
import decimal
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU, ALPHA, CLIP = 0.03, 0.9, -1.0


def np_lse(x, tau):
    """lse_tau over the last axis in float64: m + tau log sum exp((x - m) / tau)"""
    x = np.asarray(x, np.float64)
    m = x.max(-1)
    return m + tau * np.log(np.exp((x - m[..., None]) / tau).sum(-1))


def np_mdqn_target(q_s, q_s2, a, R, done, Gamma, tau=TAU, alpha=ALPHA, clip=CLIP):
    """the target of include/fbdqn.h in float64.  q_s = q-(s, .), q_s2 = q-(s', .) [B, A]; a, R, done [B]; Gamma the bootstrap discount.
    -> (y, bonus, V), each [B]"""
    q_s, q_s2 = np.asarray(q_s, np.float64), np.asarray(q_s2, np.float64)
    a = np.asarray(a, np.int64)
    R = np.asarray(R, np.float64)
    m = q_s.max(1)
    logpi = (q_s[np.arange(len(a)), a] - m) - tau * np.log(np.exp((q_s - m[:, None]) / tau).sum(1))      # tau ln pi-(a|s)
    bonus = alpha * np.maximum(logpi, clip)
    V = np_lse(q_s2, tau)
    y = (R + bonus) + np.where(np.asarray(done).astype(bool), 0.0, Gamma * V)
    return y, bonus, V


def paper_form(q_s, q_s2, a, R, done, Gamma, tau, alpha, clip):
    """one sample in the paper's form (eq. 2 of Vieillard et al.), 60 significant digits"""
    D = decimal.Decimal
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        t = D(repr(float(tau)))

        def softmax(q):
            e = [(D(repr(float(x))) / t).exp() for x in q]
            z = sum(e)
            return [x / z for x in e]

        pi_s, pi_s2 = softmax(q_s), softmax(q_s2)
        tlnpi = t * pi_s[a].ln()
        bonus = D(repr(float(alpha))) * max(tlnpi, D(repr(float(clip))))
        V = sum(p * (D(repr(float(x))) - t * p.ln()) for p, x in zip(pi_s2, q_s2))
        y = D(repr(float(R))) + bonus + (D(0) if done else D(repr(float(Gamma))) * V)
        return float(y), float(bonus), float(V)


@pytest.mark.parametrize("gap", [0.0, 0.5, 50.0, 2000.0])
@pytest.mark.parametrize("tau,alpha,clip", [(TAU, ALPHA, CLIP), (0.1, 0.5, -0.25), (1.0, 1.0, -1000.0)])
def test_stable_form_equals_the_papers_form(gap, tau, alpha, clip):
    """q gaps of 0 .. 2000 tau between the actions; at 50 tau the runner-up's probability is 2e-22, at 2000 tau the naive float64 form
    overflows (exp(q / tau)) or underflows to log(0)"""
    rng = np.random.default_rng(int(gap) + int(1000 * tau))
    for A in (1, 2, 3, 8):
        B = 12
        q_s = rng.normal(size=(B, A)) * tau
        q_s2 = rng.normal(size=(B, A)) * tau
        if A > 1:
            q_s[np.arange(B), rng.integers(0, A, B)] += gap * tau
            q_s2[np.arange(B), rng.integers(0, A, B)] -= gap * tau
        q_s += 3.0
        q_s2 -= 2.0
        a = rng.integers(0, A, B)
        R = rng.choice([0.1, 3.0, -3.0], B)
        done = rng.integers(0, 2, B)
        Gamma = 0.99 ** 3
        y, bonus, V = np_mdqn_target(q_s, q_s2, a, R, done, Gamma, tau, alpha, clip)
        assert np.all(bonus <= 0) and np.all(bonus >= alpha * clip)
        for b in range(B):
            y0, bonus0, V0 = paper_form(q_s[b], q_s2[b], int(a[b]), R[b], int(done[b]), Gamma, tau, alpha, clip)
            scale = max(1.0, abs(V0), gap * tau)
            assert abs(V[b] - V0) <= 1e-13 * scale, (A, b, V[b], V0)
            assert abs(bonus[b] - bonus0) <= 1e-13 * scale, (A, b, bonus[b], bonus0)
            assert abs(y[b] - y0) <= 1e-13 * scale, (A, b, y[b], y0)


def test_the_naive_form_fails_where_the_stable_one_does_not():
    q = np.array([[0.0, 2000 * TAU]])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        naive = TAU * np.log(np.exp(q / TAU).sum(1))
        naive_neg = TAU * np.log(np.exp(-q[:, ::-1] / TAU - 800.0).sum(1))
    assert not np.isfinite(naive).all() and not np.isfinite(naive_neg).all()
    assert np_lse(q, TAU)[0] == 2000 * TAU and np_lse(-q - 800 * TAU, TAU)[0] == -800 * TAU


def test_the_headers_hand_cases():
    one = lambda q_s, a, R=0.1, done=0, q_s2=(0.0, 0.0): [float(v[0]) for v in np_mdqn_target([q_s], [q_s2], [a], [R], [done], 0.99)]
    for c in (0.0, 1.5, -7.25):
        for a in (0, 1):
            assert abs(one((c, c), a)[1] - (-ALPHA * TAU * np.log(2.0))) < 1e-15
    assert one((0.0, 2.0), 0)[1] == -0.9                         # tau ln pi = -2 - tiny: clipped at l0 = -1
    b1 = one((0.0, 2.0), 1)[1]
    assert b1 == 0.0 and abs(b1) < 1e-20                         # -alpha tau log1p(exp(-66.7)) = -0
    y, bonus, V = one((0.0, 2.0), 0, R=3.0, done=1, q_s2=(5.0, 6.0))
    assert y == 3.0 + bonus == 3.0 - 0.9                         # done: y = R + bonus, the bootstrap is dropped and the bonus is not
    y, bonus, V = one((0.0, 2.0), 0, R=3.0, done=0, q_s2=(5.0, 5.0))
    assert abs(V - (5.0 + TAU * np.log(2.0))) < 1e-15 and abs(y - (3.0 - 0.9 + 0.99 * V)) < 1e-15


def test_one_action_gives_natures_target():
    rng = np.random.default_rng(3)
    q_s, q_s2 = rng.normal(size=(64, 1)) * 5, rng.normal(size=(64, 1)) * 5
    R = rng.choice([0.1, 3.0, -3.0], 64)
    done = rng.integers(0, 2, 64)
    y, bonus, V = np_mdqn_target(q_s, q_s2, np.zeros(64, np.int64), R, done, 0.99)
    assert not bonus.any() and np.array_equal(V, q_s2[:, 0])
    assert np.array_equal(y, np.where(done == 1, R, R + 0.99 * q_s2.max(1)))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_and_binding_declare_the_mdqn_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("#define FB_ALGO_MDQN 14", "#define FB_ALGO_MDQN_PER 15",
                 "int fb_qnet_set_munchausen(fb_qnet_t h, float tau, float alpha, float clip_lo);",
                 "int fb_qnet_get_munchausen(fb_qnet_t h, float *tau_host, float *alpha_host, float *clip_lo_host);",
                 "ONLY THE FIRST step's"):
        assert decl in hdr, decl
    assert (L.ALGO_MDQN, L.ALGO_MDQN_PER) == (14, 15) and L.MDQN_DEFAULTS == (0.03, 0.9, -1.0)
    f, vp = ctypes.c_float, ctypes.c_void_p
    assert L.SIGNATURES["fb_qnet_set_munchausen"] == [vp, f, f, f]
    assert L.SIGNATURES["fb_qnet_get_munchausen"] == [vp, vp, vp, vp]
    lib = L.lib()                                                # (binds both symbols: a stale library raises here)
    assert lib.fb_qnet_set_munchausen(None, 0.03, 0.9, -1.0) == -1 and "NULL" in lib.fb_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_algo_tables_and_value_checks():
    from dqnflappybird_amd import vec, vecbrain
    assert vec.ALGOS["mdqn"] == 14 and vec.ALGOS["mdqnper"] == 15
    assert "mdqnper" in vec.WEIGHTED_ALGOS and "mdqn" not in vec.WEIGHTED_ALGOS and set(vec.WEIGHTED_ALGOS) > set(vec.PRIORITIZED_ALGOS)
    assert "mdqnper" in vecbrain.PER_ALGOS and "mdqn" not in vecbrain.PER_ALGOS
    for algo in ("mdqn", "mdqnper"):
        assert vecbrain.MEAN_LOSS[algo] and algo in vecbrain.TARGET_SYNC
    assert vecbrain.HipVecBackend.mdqn is True
    assert vec.check_munchausen(0.03, 0.9, -1.0) == tuple(float(np.float32(x)) for x in (0.03, 0.9, -1.0))
    assert vec.check_munchausen(5, 0, 0) == (5.0, 0.0, 0.0) and vec.check_munchausen(1e-3, 1, -100) == (float(np.float32(1e-3)), 1.0, -100.0)
    for args, msg in (((0.0, 0.9, -1.0), "tau"), ((-0.03, 0.9, -1.0), "tau"), ((float("nan"), 0.9, -1.0), "tau"), ((float("inf"), 0.9, -1.0), "tau"),
                      ((0.03, -0.1, -1.0), "alpha"), ((0.03, 1.5, -1.0), "alpha"), ((0.03, float("nan"), -1.0), "alpha"),
                      ((0.03, 0.9, 0.5), "clip"), ((0.03, 0.9, float("-inf")), "clip"), ((0.03, 0.9, float("nan")), "clip")):
        with pytest.raises(ValueError, match=msg):
            vec.check_munchausen(*args)


@pytest.mark.parametrize("kw,msg", [
    (dict(algo="mdqn", tau=0.0), "tau must be finite and > 0"),
    (dict(algo="mdqnper", alpha=1.5), "alpha must be in \\[0, 1\\]"),
    (dict(algo="mdqn", clip=0.1), "clip \\(l0\\) must be finite and <= 0"),
    (dict(algo="mdqn", arch="c51"), "scalar heads: arch must be 'plain' or 'dueling'"),
    (dict(algo="mdqnper", arch="qrdueling"), "scalar heads: arch must be 'plain' or 'dueling'"),
    (dict(algo="mdqn", noisy=True), "not with the Munchausen-DQN algo 'mdqn'"),
    (dict(algo="mdqn", n_step=17), "n_step must be in 1..16"),
    (dict(algo="mdqn"), "cpu-oracle \\(tests only\\) backend has no Munchausen-DQN \\(mdqn\\): algo 'mdqn' needs it"),
    (dict(algo="mdqnper", arch="dueling", world=2), "backend has no Munchausen-DQN \\(mdqn\\): algo 'mdqnper' needs it"),
])
def test_vecbrain_refusals_on_a_backend_without_the_mdqn_flag(kw, msg):
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    assert not hasattr(CpuVecBackend, "mdqn")
    with pytest.raises(ValueError, match=msg):
        VecBrain(16, backend=CpuVecBackend(), **kw)


def test_checkpoint_key_round_trip_and_named_refusals(tmp_path):
    from dqnflappybird_amd.vecbrain import check_checkpoint_munchausen
    from dqnflappybird_amd.vec import check_munchausen
    mine = check_munchausen(TAU, ALPHA, CLIP)
    paths = {}
    for name, kw in (("same", dict(munchausen=np.array(mine, np.float64))),
                     ("other", dict(munchausen=np.array(check_munchausen(0.1, 0.5, -0.25), np.float64))),
                     ("scalar", dict())):
        paths[name] = str(tmp_path / f"{name}.npz")
        np.savez(paths[name], online=np.zeros(3, np.float32), **kw)
    z = {k: np.load(p) for k, p in paths.items()}
    assert tuple(z["same"]["munchausen"].tolist()) == mine                   # float32-rounded values survive the float64 array exactly
    check_checkpoint_munchausen(z["same"], mine, "x")
    check_checkpoint_munchausen(z["scalar"], mine, "x")                      # no key: any scalar-head checkpoint loads
    check_checkpoint_munchausen(z["other"], None, "x")                       # another scalar algo does not read the key
    with pytest.raises(ValueError, match="checkpoint x was trained with munchausen \\(tau, alpha, clip\\) = \\(0.10000000149011612, 0.5, -0.25\\), "
                                         "this VecBrain has \\(0.029999999329447746, 0.8999999761581421, -1.0\\)"):
        check_checkpoint_munchausen(z["other"], mine, "x")
    with pytest.raises(ValueError, match="munchausen"):
        check_checkpoint_munchausen(z["same"], check_munchausen(TAU, ALPHA, -0.5), "x")


@pytest.mark.parametrize("argv,msg", [
    (["--model", "mdqn"], "--model mdqn needs --vec"),
    (["--model", "mdqnper"], "--model mdqnper needs --vec"),
    (["--model", "mdqn", "--vec", "16", "--noisy"], "--noisy needs a C51 model"),
    (["--model", "mdqn", "--vec", "16", "--tau", "0"], "tau must be finite and > 0"),
    (["--model", "mdqnper", "--vec", "16", "--alpha", "2"], "alpha must be in [0, 1]"),
    (["--model", "mdqn", "--vec", "16", "--clip", "1"], "clip (l0) must be finite and <= 0"),
    (["--model", "ddqn", "--vec", "16", "--tau", "0.1"], "--tau / --alpha / --clip need a Munchausen model"),
])
def test_cli_mdqn_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr
