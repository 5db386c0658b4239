"""Initial priorities from acting-time TD errors (include/fbdqn.h FB_PER_INIT_TD), the parts decided without a GPU: the invariants of
the NumPy restatement the GPU tests compare the tree with (tests/primecases.py), the refusals of VecBrain, of the command line and of
VecReplay's own argument checks, the checkpoint key rules, and the ABI binding."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.cpu_backend import CpuVecBackend
from tests.primecases import P_MAX, P_MIN, FastTree, PrimedMemory, priority, td_delta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the restatement
def test_priority_range_and_hand_worked_values():
    d = np.array([0.0, 1e-9, 0.5, 0.99, 0.990001, 1.0, 6.0, 1e30], np.float32)
    p = priority(d)
    assert p.dtype == np.float32 and (p >= P_MIN).all() and (p <= P_MAX).all()
    assert p[0] == P_MIN == np.float32(np.float64(np.float32(0.01)) ** np.float64(np.float32(0.6)))
    assert (p[3:] == 1.0).all()                              # delta + 0.01f >= 1 in float32 from 0.99 on: abs_err_upper
    assert p[2] == np.float32(np.float64(np.float32(0.5) + np.float32(0.01)) ** np.float64(np.float32(0.6)))
    assert (np.diff(p) >= 0).all()


def test_a_done_row_ignores_q_and_the_other_rows_do_not():
    rng = np.random.default_rng(0)
    N, A = 64, 3
    R = rng.choice(np.array([0.1, 1.0, -1.0], np.float32), N)
    done = (rng.random(N) < 0.5).astype(np.uint8)
    rec = rng.normal(size=N).astype(np.float32)
    q1, q2 = rng.normal(size=(N, A)).astype(np.float32), rng.normal(size=(N, A)).astype(np.float32) + 5
    d1, d2 = td_delta(R, done, q1, rec, 0.99), td_delta(R, done, q2, rec, 0.99)
    assert done.any() and not done.all()
    assert np.array_equal(d1[done == 1], d2[done == 1]) and (d1[done == 0] != d2[done == 0]).all()
    assert np.array_equal(d1[done == 1], np.abs(R.astype(np.float64) - rec.astype(np.float64)).astype(np.float32)[done == 1])
    e = 3                                                    # one row by hand: product, then sum, then the difference, in float64
    while done[e]:
        e += 1
    y = float(R[e]) + 0.99 * float(q1[e].max())
    assert d1[e] == np.float32(abs(y - float(rec[e])))


@pytest.mark.parametrize("N,cap,n", [(5, 40, 1), (8, 64, 3), (64, 1000, 3)])
def test_restated_tree_invariants(N, cap, n):
    """after every prime and every push: the root is the sequential sum of the nodes one level down (a left + right tree: of its two
    children), every inner node is left + right, max / min heaps agree with the filled leaves, and primed leaves lie in [0.01^0.6, 1]"""
    rng = np.random.default_rng(N)
    mem = PrimedMemory(cap, N, n, 0.99)
    for S in range(2 * ((cap + N - 1) // N) + n + 3):
        q = rng.normal(size=(N, 2)).astype(np.float32)
        mem.prime(q, rng.integers(0, 2, N))
        assert (mem.last_p is not None) == (S >= n)
        for _ in range(2):                                   # ... behind the prime, then behind the push
            t = mem.t
            if t.size:
                assert t.tree[0] == t.tree[1] + t.tree[2] if cap > 1 else True
                acc = 0.0
                for v in t.level_sums(1):
                    acc += v
                assert t.tree[0] == acc
                inner = np.arange(cap - 1)
                assert np.array_equal(t.tree[inner], t.tree[2 * inner + 1] + t.tree[2 * inner + 2])
                filled = [d + cap - 1 for d in range(t.size)]
                assert t.maxt[0] == t.tree[filled].max() and t.mint[0] == t.tree[filled].min()
            if mem.last_p is not None:
                assert (mem.last_p >= P_MIN).all() and (mem.last_p <= P_MAX).all()
                if _ == 0:
                    assert np.array_equal(t.tree[t.last_stored(N)], mem.last_p.astype(np.float64))
            if _ == 0:
                mem.push(rng.choice(np.array([0.1, 1.0, -1.0], np.float32), N), (rng.random(N) < 0.2).astype(np.uint8))
    assert mem.t.size == cap and mem.S * N > 2 * cap         # wrapped twice


def test_restatement_falls_back_without_the_record():
    rng = np.random.default_rng(1)
    N, cap, n = 4, 32, 3
    mem = PrimedMemory(cap, N, n, 0.9)
    primed = []
    for S in range(12):
        if S == 7:
            mem.clear_record()                               # a mode switch / a load without the record
        mem.prime(rng.normal(size=(N, 2)).astype(np.float32), rng.integers(0, 2, N))
        primed.append(mem.last_p is not None)
        mem.push(np.ones(N, np.float32), np.zeros(N, np.uint8))
    assert primed == [False] * 3 + [True] * 4 + [False] * 3 + [True] * 2


def test_fast_tree_store_is_max_p():
    t = FastTree(6)
    assert t.store(4) == 1.0 and t.tree[0] == 4.0 and t.mint[0] == 1.0
    t.set_leaves(t.last_stored(4)[:2], [0.25, 0.5])
    assert t.tree[0] == 2.75 and t.maxt[0] == 1.0 and t.mint[0] == 0.25
    assert t.store(4) == 1.0 and t.size == 6 and t.pointer == 2      # wrapped: slots 4, 5, 0, 1 -- the two primed leaves are overwritten
    assert t.tree[0] == 6.0 and t.mint[0] == 1.0


# ------------------------------------------------------------------ VecBrain
class Created(Exception):
    pass


class WithInit(CpuVecBackend):
    name = "stand-in with per_priority_init"
    per_one_step = per_n_step = double_per = mdqn = c51 = qr = True
    per_priority_init = True

    def replay(self, capacity, n_envs, prioritized, n_step=1, gamma=None):
        raise Created(capacity, n_envs, prioritized, n_step, gamma)


class WithoutInit(WithInit):
    name = "stand-in without per_priority_init"
    per_priority_init = False


class WithoutOneStep(WithInit):
    name = "stand-in without per_one_step"
    per_one_step = False


def test_vecbrain_refusals_by_name():
    from dqnflappybird_amd.vecbrain import VecBrain
    kw = dict(capacity=64, priority_init="td")
    with pytest.raises(ValueError, match="per_priority_init") as ei:
        VecBrain(4, algo="per", backend=CpuVecBackend(), **kw)
    assert "cpu-oracle" in str(ei.value)
    with pytest.raises(ValueError, match="per_priority_init") as ei:
        VecBrain(4, algo="doubleper", backend=WithoutInit(), **kw)
    assert "stand-in without per_priority_init" in str(ei.value)
    with pytest.raises(ValueError, match="per_one_step.*primed inside it") as ei:      # (the composed-calls fallback of step() never primes)
        VecBrain(4, algo="per", backend=WithoutOneStep(), **kw)
    assert "stand-in without per_one_step" in str(ei.value)
    with pytest.raises(ValueError, match="mdqnper.*soft value"):
        VecBrain(4, algo="mdqnper", backend=WithInit(), **kw)
    for algo in ("dqn", "nature", "double", "c51per", "c51doubleper", "qrper", "qrdoubleper", "mdqn", "c51"):
        with pytest.raises(ValueError, match=f"priority_init='td' needs algo 'per' or 'doubleper'.*{algo}"):
            VecBrain(4, algo=algo, backend=WithInit(), **kw)
    with pytest.raises(ValueError, match="priority_init='td': data parallel is not supported"):
        VecBrain(4, algo="per", world=2, backend=WithInit(), **kw)
    with pytest.raises(ValueError, match="priority_init must be one of"):
        VecBrain(4, algo="per", backend=WithInit(), capacity=64, priority_init="mean")
    for algo in ("per", "doubleper"):                        # accepted: the brain goes on to ask for its memory
        with pytest.raises(Created) as ei:
            VecBrain(4, algo=algo, n_step=3, gamma=0.95, backend=WithInit(), **kw)
        assert ei.value.args == (64, 4, True, 3, 0.95)
    with pytest.raises(Created):                             # 'max' asks nothing of the backend
        VecBrain(4, algo="per", backend=WithoutInit(), capacity=64)


def test_the_hip_backend_declares_the_capability_and_the_cpu_one_does_not():
    from dqnflappybird_amd.vecbrain import HipVecBackend
    assert HipVecBackend.per_priority_init is True
    assert not getattr(CpuVecBackend, "per_priority_init", False)


def test_checkpoint_key_rules():
    from dqnflappybird_amd.vecbrain import check_checkpoint_priority_init

    class Z(dict):
        files = property(lambda self: list(self))

    old, new = Z(scalars=np.zeros(4)), Z(priority_init=np.array(["td"]))
    check_checkpoint_priority_init(old, "max", "ck")          # a file without the key loads as 'max'
    check_checkpoint_priority_init(new, "td", "ck")
    with pytest.raises(ValueError, match="ck was written with priority_init = 'max', this VecBrain has priority_init = 'td'"):
        check_checkpoint_priority_init(old, "td", "ck")
    with pytest.raises(ValueError, match="ck was written with priority_init = 'td', this VecBrain has priority_init = 'max'"):
        check_checkpoint_priority_init(new, "max", "ck")


def test_vecreplay_checks_its_arguments_before_the_device():
    """refused in Python before any device call: these run on an object that never reached the library"""
    from dqnflappybird_amd.vec import PRIORITY_INITS, VecReplay
    assert PRIORITY_INITS == ("max", "td")
    rep = object.__new__(VecReplay)
    with pytest.raises(ValueError, match="priority_init must be one of"):
        rep.set_priority_init("mean")


# ------------------------------------------------------------------ the command line
def cli(*argv):
    return subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN", *argv], cwd=ROOT, capture_output=True, text=True,
                          timeout=120)


@pytest.mark.parametrize("model", ["dqn", "ddqn", "duelingdqn", "mdqnper", "c51per", "rainbow", "qrdqnper", "iqnper", "sacper", "a2c"])
def test_cli_refuses_td_on_every_other_model_by_name(model):
    p = cli("--model", model, "--vec", "8", "--steps", "1", "--priority-init", "td")
    assert p.returncode == 2, (p.stdout, p.stderr)
    assert f"--priority-init td needs --model prioritydqn | doubleper, not --model {model}" in p.stderr


def test_cli_refuses_td_without_vec_and_an_unknown_value():
    p = cli("--model", "prioritydqn", "--steps", "1", "--priority-init", "td")
    assert p.returncode == 2 and "--priority-init td needs --vec" in p.stderr
    p = cli("--model", "prioritydqn", "--vec", "8", "--priority-init", "mean")
    assert p.returncode == 2 and "invalid choice" in p.stderr


def test_cli_hands_the_setting_to_vecbrain():
    import argparse
    from dqnflappybird_amd.FlappyBirdDQN import build_parser, priority_init_kwargs
    parser = build_parser()
    for model in ("prioritydqn", "doubleper"):
        args = parser.parse_args(["--model", model, "--vec", "8", "--priority-init", "td"])
        assert priority_init_kwargs(args, parser) == dict(priority_init="td")
    assert priority_init_kwargs(parser.parse_args(["--model", "prioritydqn", "--vec", "8"]), parser) == {}
    assert priority_init_kwargs(parser.parse_args(["--model", "dqn", "--vec", "8", "--priority-init", "max"]), parser) == {}
    assert isinstance(parser, argparse.ArgumentParser)


# ------------------------------------------------------------------ the binding
def test_the_calls_are_declared_and_bound():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "#define FB_PER_INIT_MAX 0" in hdr and "#define FB_PER_INIT_TD 1" in hdr
    assert "int fb_replay_prime_priorities(fb_replay_t h, const float *q, const uint8_t *actions, int n_actions, void *stream);" in hdr
    assert (L.PER_INIT_MAX, L.PER_INIT_TD) == (0, 1)
    assert L.SIGNATURES["fb_replay_prime_priorities"] == [L._vp, L._vp, L._vp, L._i, L._vp]
    assert L.SIGNATURES["fb_replay_set_priority_init"] == [L._vp, L._i]


def test_the_tools_offer_the_setting():
    for tool, flag in (("time_prime.py", "--envs"), ("per_census.py", "--steps"), ("learn_curve.py", "--priority-init")):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool), "--help"], cwd=ROOT, capture_output=True, text=True,
                           timeout=120)
        assert p.returncode == 0 and flag in p.stdout, (tool, p.stderr)
