"""Prioritized memories with n-step returns, the parts decided before anything touches a GPU: VecBrain's backend capability check
(per_n_step) with stand-in backends, how VecBrain asks the backend for the memory, VecReplay's argument checks, and the ABI binding."""
import os
import subprocess
import sys

import pytest

from tests.cpu_backend import CpuVecBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Created(Exception):
    """raised by the stand-in backends' replay(): VecBrain has asked for its memory -- with these arguments"""


class NoPerNStep(CpuVecBackend):
    name = "stand-in without per_n_step"


class WithPerNStep(CpuVecBackend):
    name = "stand-in with per_n_step"
    per_n_step = True

    def replay(self, capacity, n_envs, prioritized, n_step=1, gamma=None):
        raise Created(capacity, n_envs, prioritized, n_step, gamma)


def test_backend_without_the_capability_refuses_per_n_step():
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(ValueError, match="uniform replay only") as ei:
        VecBrain(4, algo="per", n_step=3, capacity=64, backend=NoPerNStep())
    assert "stand-in without per_n_step" in str(ei.value)


def test_backend_with_the_capability_creates_the_memory_with_n():
    from dqnflappybird_amd.vecbrain import VecBrain
    with pytest.raises(Created) as ei:
        VecBrain(4, algo="per", n_step=3, capacity=64, gamma=0.95, backend=WithPerNStep())
    assert ei.value.args == (64, 4, True, 3, 0.95)
    with pytest.raises(Created) as ei:                       # n = 1: the memory of old, created as before
        VecBrain(4, algo="per", capacity=64, backend=WithPerNStep())
    assert ei.value.args == (64, 4, True, 1, None)
    with pytest.raises(Created) as ei:                       # uniform memories keep the n-step view (set_n_step after creation)
        VecBrain(4, algo="dqn", n_step=3, capacity=64, backend=WithPerNStep())
    assert ei.value.args == (64, 4, False, 1, None)
    with pytest.raises(ValueError, match="1..16"):
        VecBrain(4, algo="per", n_step=17, backend=WithPerNStep())


def test_the_hip_backend_declares_the_capability():
    import inspect
    from dqnflappybird_amd.vecbrain import HipVecBackend
    assert HipVecBackend.per_n_step is True
    params = inspect.signature(HipVecBackend.replay).parameters
    assert "n_step" in params and "gamma" in params


@pytest.mark.parametrize("kw,msg", [(dict(n_step=0, gamma=0.99), "1..16"), (dict(n_step=17, gamma=0.99), "1..16"),
                                    (dict(n_step=3), "gamma"), (dict(capacity=11, n_step=3, gamma=0.99), "capacity 11 < n_step")])
def test_vecreplay_checks_its_n_step_arguments_before_the_device(kw, msg):
    """refused in Python before any device call (so these run without a GPU), prioritized or not"""
    from dqnflappybird_amd.vec import VecReplay
    for prioritized in (True, False):
        args = dict(dict(capacity=100, n_envs=4, prioritized=prioritized), **kw)
        with pytest.raises(ValueError, match=msg):
            VecReplay(**args)


def test_the_creation_call_is_declared_and_bound():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert "int fb_replay_create_nstep(int64_t capacity, int n_envs, int kind, int n, double gamma, fb_replay_t *out);" in hdr
    assert L.SIGNATURES["fb_replay_create_nstep"] == [L._i64, L._i, L._i, L._i, L._d, L._vp]


def test_time_nstep_offers_the_prioritized_memory():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "time_nstep.py"), "--help"], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0 and "--per-mode" in p.stdout and "per" in p.stdout, p.stderr
