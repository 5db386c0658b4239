"""What the four vectorised loops refuse, print and save on the host, pinned to a record.

The `host` part of tests/golden/loop_record.json was written ONCE, with the code of commit 97ae14e -- before the loops' shared host code
(checkpoint core, foreign-head refusal, log line tail, device-world construction, scalar argument checks, VecBrain's argument resolution)
was written once.  It is a record, not a reference to regenerate: that refactor, and every later one of the Python layer, must reproduce
every text, every precedence between two wrong arguments, every log line and every checkpoint array, compared with plain equality.
`python -m tests.test_loop_record_host --record [PATH]` writes it (no GPU); tests/test_gpu_loop_record.py holds the `gpu` part.

- Constructor refusals: per class an ordered grid of constructions -> str(e) of the ValueError, or "accepted".  "accepted" means the
  construction got as far as creating the envs (VecGameState, or the backend's env factory, which these cases replace by a marker), so
  the record also pins that every refusal comes before that point.  VecBrain's grid runs on the CPU stand-in, on the default HIP
  backend and on stub backends that lack one capability flag each.
- load() refusals: crafted .npz files loaded into Class.__new__(Class) objects that carry only the attributes load reads up to that
  refusal (an earlier read of another attribute would be an AttributeError here), the temp directory written as <dir>.
- VecBrain on the CPU stand-in (algos dqn, nature, per): the lines of run(6, log_every=3), every array of the checkpoint as
  (dtype, shape, SHA-256), then a fresh object that loads it, the lines of run(2, log_every=1) and its checkpoint.

The --record run, and only it, also checks coverage: it lists every `raise ValueError` of __init__, check_* and load in the four
modules with ast, and fails unless the traceback of some recorded refusal names each of them; the record stores the count.
"""
import ast
import contextlib
import hashlib
import io
import json
import os
import sys

import numpy as np
import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_record.json")
MODULES = ("vecbrain", "veciqn", "vecsac", "vecac")
FLAGS = ("c51", "c51_dueling", "c51_noisy", "acting_noise_env", "qr", "mdqn", "double_per", "huber", "grad_clip", "polyak", "per_one_step",
         "per_n_step")
NAN, INF = float("nan"), float("inf")


class Reached(Exception):
    """a construction passed every refusal and asked for its envs"""


def _reached(*a, **k):
    raise Reached()


@contextlib.contextmanager
def no_device_world():
    """VecGameState -> the marker: what the three single-GPU loops and the HIP backend create first"""
    from dqnflappybird_amd import vec
    real, vec.VecGameState = vec.VecGameState, _reached
    try:
        yield
    finally:
        vec.VecGameState = real


class _Obj:
    def seed(self, *a):
        pass


class _NStepObj(_Obj):
    def set_n_step(self, *a):
        pass


def stub_backend(lacking=None, name="stub", world=None):
    """a backend with every capability flag but `lacking`; its env factory is the marker, unless world = 'nonstep' / 'nstep': envs and
    a memory without / with an n-step view, and the net factory is the marker"""
    ns = {f: f != lacking for f in FLAGS}
    if name is not None:
        ns["name"] = name
    ns["env"] = _reached if world is None else (lambda self, n, seed: _Obj())
    ns["replay"] = lambda self, *a, **k: (_Obj if world == "nonstep" else _NStepObj)()
    ns["net"] = _reached
    return type("StubBackend", (), ns)()


def backend(key):
    if key == "cpu":
        from tests.cpu_backend import CpuVecBackend
        return CpuVecBackend()
    if key == "hip":
        return None
    if key == "stub":
        return stub_backend()
    if key == "stub-noname":
        return stub_backend("huber", name=None)
    if key in ("stub-nonstep", "stub-nstep"):
        return stub_backend(world=key[5:])
    return stub_backend(key[5:])


# ---------------------------------------------------------------- the constructor grids, in order
def _flag_cases():
    """per capability flag the arguments that need it: on the stub that lacks it, then on the full stub"""
    needs = [("acting_noise_env", dict(algo="c51", noisy=True, acting_noise="env")), ("huber", dict(huber=1.0)), ("grad_clip", dict(max_grad_norm=1.0)),
             ("polyak", dict(polyak=0.1)), ("double_per", dict(algo="doubleper")), ("per_one_step", dict(algo="doubleper")),
             ("mdqn", dict(algo="mdqn")), ("per_one_step", dict(algo="mdqnper")), ("mdqn", dict(algo="mdqnper")), ("qr", dict(algo="qr")),
             ("per_one_step", dict(algo="qrper")), ("per_one_step", dict(algo="qr")), ("c51", dict(algo="c51")),
             ("c51_dueling", dict(algo="c51", arch="c51dueling")), ("c51_dueling", dict(algo="c51")), ("per_one_step", dict(algo="c51per")),
             ("c51_noisy", dict(algo="c51", noisy=True)), ("c51_noisy", dict(algo="c51")), ("per_n_step", dict(algo="per", n_step=3)),
             ("per_n_step", dict(algo="per")), ("per_n_step", dict(algo="dqn", n_step=3))]
    out = []
    for flag, kw in needs:
        out.append((f"stub-{flag}", kw))
        out.append(("stub", kw))
    return out


BRAIN_CASES = [
    ("cpu", {}), ("cpu", dict(algo="nature")), ("cpu", dict(acting_noise="both")), ("cpu", dict(acting_noise="env")),
    ("cpu", dict(acting_noise="both", n_step=0)), ("cpu", dict(n_step=0)), ("cpu", dict(n_step=17)), ("cpu", dict(n_step=0, huber=-1.0)),
    ("cpu", dict(algo="c51", noisy=True, acting_noise="env")), ("cpu", dict(huber=-1.0)), ("cpu", dict(huber=NAN)), ("cpu", dict(algo="c51", huber=1.0)),
    ("cpu", dict(algo="qr", huber=0.5, max_grad_norm=-1.0)), ("cpu", dict(huber=1.0)), ("cpu", dict(huber=1.0, max_grad_norm=-1.0)),
    ("cpu", dict(max_grad_norm=-1.0)), ("cpu", dict(max_grad_norm=-1.0, polyak=2.0)), ("cpu", dict(polyak=2.0)), ("cpu", dict(polyak=NAN)),
    ("cpu", dict(max_grad_norm=1.0)), ("cpu", dict(max_grad_norm=1.0, polyak=2.0)), ("cpu", dict(polyak=0.1)), ("cpu", dict(polyak=0.1, algo="doubleper")),
    ("cpu", dict(algo="doubleper", arch="c51")), ("cpu", dict(algo="doubleper", arch="c51", noisy=True)), ("cpu", dict(algo="doubleper", noisy=True)),
    ("cpu", dict(algo="doubleper")), ("cpu", dict(algo="mdqn", tau=0.0)), ("cpu", dict(algo="mdqn", tau=0.0, arch="c51")), ("cpu", dict(algo="mdqn", alpha=2.0)),
    ("cpu", dict(algo="mdqn", clip=1.0)), ("cpu", dict(algo="mdqn", arch="c51")), ("cpu", dict(algo="mdqnper", noisy=True)), ("cpu", dict(algo="mdqn")),
    ("cpu", dict(algo="qr", arch="dueling")), ("cpu", dict(algo="qr", arch="dueling", world=2)), ("cpu", dict(algo="qr", world=2)),
    ("cpu", dict(algo="qrper", world=2, noisy=True)), ("cpu", dict(algo="qrdouble", noisy=True)), ("cpu", dict(algo="qr")), ("cpu", dict(arch="qr")),
    ("cpu", dict(algo="per", arch="qrdueling", noisy=True)), ("cpu", dict(algo="c51", arch="dueling")), ("cpu", dict(algo="c51double", world=2)),
    ("cpu", dict(algo="c51")), ("cpu", dict(noisy=True)), ("cpu", dict(noisy=True, arch="c51dueling")), ("cpu", dict(arch="c51dueling")),
    ("cpu", dict(algo="nature", arch="c51dueling", n_step=3)), ("cpu", dict(n_step=3)), ("cpu", dict(algo="per", n_step=3)),
    ("hip", {}), ("hip", dict(algo="c51doubleper", arch="c51dueling", noisy=True, acting_noise="env", n_step=3)),
    ("hip", dict(algo="qrdoubleper", arch="qrdueling")), ("hip", dict(algo="mdqnper", arch="dueling", huber=1.0, max_grad_norm=10, polyak=0.01)),
    ("hip", dict(algo="doubleper", arch="dueling", n_step=3)), ("hip", dict(algo="per", n_step=3)), ("hip", dict(algo="dqn", n_step=16)),
    ("hip", dict(acting_noise="env")), ("hip", dict(n_step=17)), ("hip", dict(algo="qr", huber=1.0)), ("hip", dict(huber=INF)),
    ("hip", dict(algo="qr", n_quantiles=1)), ("hip", dict(algo="qr", n_quantiles=65)), ("hip", dict(algo="qr", kappa=0.0)),
    ("hip", dict(algo="qrper", arch="c51")), ("hip", dict(algo="qr", world=2, n_quantiles=1)), ("hip", dict(algo="c51", n_atoms=1)),
    ("hip", dict(algo="c51", n_atoms=65)), ("hip", dict(algo="c51", v_min=10.0, v_max=-10.0)), ("hip", dict(algo="c51per", arch="qr")),
    ("hip", dict(algo="c51", arch="qrdueling")), ("hip", dict(algo="c51", noisy=True, sigma0=-1.0)), ("hip", dict(algo="mdqn", tau=NAN)),
    ("hip", dict(algo="mdqn", arch="qr")), ("hip", dict(algo="doubleper", arch="qr")), ("hip", dict(algo="double", noisy=True)),
    ("hip", dict(algo="double", arch="c51dueling")), ("hip", dict(algo="double", arch="c51")),
    ("stub-noname", dict(huber=1.0)), ("stub-noname", dict(huber=0.0)),
] + _flag_cases() + [
    ("stub-nonstep", dict(n_step=3)), ("stub-nonstep", dict(algo="c51", n_step=3, noisy=True, sigma0=-1.0)), ("stub-nonstep", dict(algo="per", n_step=3)),
    ("stub-nonstep", dict(algo="c51", noisy=True, sigma0=-1.0)), ("stub-nonstep", dict(algo="c51", noisy=True, sigma0=NAN)),
    ("stub-nstep", dict(n_step=3)), ("stub-nstep", dict(algo="c51", n_step=3, noisy=True, sigma0=-1.0)), ("stub-nstep", dict(algo="c51", noisy=True)),
]

IQN_CASES = [
    {}, dict(n_envs=0), dict(n_envs=0, batch=0), dict(batch=0), dict(batch=257), dict(batch=8), dict(batch=8, n_tau=0), dict(n_tau=0), dict(n_tau=1.5),
    dict(n_tau_next=65), dict(n_tau_act=65), dict(kappa=0.0), dict(cvar=0.0), dict(cvar=1.5), dict(cvar=0.5), dict(kappa=0.0, n_step=0), dict(n_step=0),
    dict(n_step=17), dict(n_step=0, polyak=2.0), dict(polyak=2.0), dict(polyak=2.0, replace_target_iter=0), dict(replace_target_iter=0), dict(observe=-1),
    dict(observe=1, n_step=3), dict(observe=2, n_step=3), dict(observe=-1, explore=0), dict(explore=0), dict(initial_epsilon=0.5, final_epsilon=0.6),
    dict(initial_epsilon=1.5), dict(final_epsilon=-0.1), dict(explore=0, gamma=1.5), dict(gamma=1.5), dict(gamma=NAN), dict(gamma=2.0, lr=0.0), dict(lr=0.0),
    dict(lr=INF), dict(lr=0.0, capacity=4), dict(capacity=4), dict(capacity=8, n_step=3, observe=2), dict(capacity=8), dict(capacity=4, max_grad_norm=-1.0),
    dict(max_grad_norm=-1.0), dict(max_grad_norm=-1.0, prioritized=1), dict(prioritized=1), dict(prioritized=None, dueling="yes"), dict(dueling="yes"),
    dict(dueling=0, munchausen=1), dict(munchausen=1), dict(munchausen=1, temp=0.0), dict(temp=0.0), dict(temp=NAN, alpha=2.0), dict(alpha=2.0),
    dict(clip=1.0), dict(clip=1.0, munchausen=True, double_q=True), dict(munchausen=True, double_q=True), dict(munchausen=False, double_q=True),
    dict(munchausen=True), dict(prioritized=True, dueling=True, double_q=True, n_step=3, cvar=0.5, max_grad_norm=10),
]

SAC_CASES = [
    {}, dict(n_envs=0), dict(n_envs=0, batch=0), dict(batch=0), dict(batch=257), dict(batch=8), dict(batch=8, alpha=0.0), dict(alpha=0.0), dict(alpha=NAN),
    dict(target_entropy=INF), dict(alpha_lr=-1.0), dict(alpha_lr=-1.0, polyak=2.0), dict(polyak=2.0), dict(polyak=0.0), dict(polyak=2.0, observe=-1),
    dict(observe=-1), dict(observe=-1, gamma=-0.1), dict(gamma=-0.1), dict(gamma=NAN), dict(gamma=2.0, lr=0.0), dict(lr=0.0), dict(lr=NAN),
    dict(lr=0.0, capacity=4), dict(capacity=4), dict(capacity=8), dict(capacity=4, max_grad_norm=-1.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=INF),
    dict(alpha_lr=1e-3, max_grad_norm=10),
]

AC_CASES = [
    {}, dict(algo="ppo"), dict(algo="trpo"), dict(algo="trpo", n_envs=0), dict(n_envs=0), dict(n_envs=0, rollout=0), dict(rollout=0), dict(rollout=129),
    dict(rollout=0, gamma=2.0), dict(gamma=2.0), dict(gamma=2.0, gae_lambda=2.0), dict(gae_lambda=2.0), dict(gae_lambda=NAN, value_coef=-1.0),
    dict(value_coef=-1.0), dict(value_coef=-1.0, entropy_coef=-1.0), dict(entropy_coef=-1.0), dict(entropy_coef=INF, max_grad_norm=-1.0),
    dict(max_grad_norm=-1.0), dict(max_grad_norm=-1.0, algo="ppo", epochs=0), dict(algo="ppo", epochs=0), dict(epochs=0, minibatches=0),
    dict(algo="ppo", epochs=0, minibatches=0), dict(algo="ppo", minibatches=0), dict(algo="ppo", minibatches=3), dict(algo="ppo", minibatches=8),
    dict(algo="ppo", minibatches=3, clip_eps=0.0), dict(algo="ppo", clip_eps=0.0), dict(algo="ppo", clip_eps=0.0, value_clip=-1.0),
    dict(algo="ppo", value_clip=-1.0), dict(algo="ppo", value_clip=-1.0, capacity=4), dict(capacity=4), dict(capacity=16), dict(capacity=4, lr=0.0),
    dict(lr=0.0), dict(lr=NAN), dict(algo="ppo", epochs=2, minibatches=2, value_clip=0.2, max_grad_norm=0.5),
]


def case_name(kw, be=None):
    text = ",".join(f"{k}={v!r}" for k, v in kw.items())
    return text if be is None else f"[{be}] {text}"


def construct(cls, kw, be=None):
    """-> ('accepted' or the refusal's text, the refusal or None)"""
    if cls == "VecBrain":
        from dqnflappybird_amd.vecbrain import VecBrain
        make = lambda: VecBrain(**{**dict(n_envs=2, batch=2, capacity=16, observe=2, seed=3, fc_width=128), **kw}, backend=backend(be))
    elif cls == "VecIQN":
        from dqnflappybird_amd.veciqn import VecIQN
        make = lambda: VecIQN(**{**dict(n_envs=4, batch=4, fc_width=128, seed=3, n_tau=2, n_tau_next=2, n_tau_act=4), **kw})
    elif cls == "VecSAC":
        from dqnflappybird_amd.vecsac import VecSAC
        make = lambda: VecSAC(**{**dict(n_envs=4, batch=4, fc_width=128, seed=3), **kw})
    else:
        from dqnflappybird_amd.vecac import VecActorCritic
        make = lambda: VecActorCritic(**{**dict(n_envs=4, rollout=2, fc_width=128, seed=3), **kw})
    try:
        with no_device_world():
            make()
    except Reached:
        pass
    except ValueError as e:
        return str(e), e
    return "accepted", None


def constructor_cases():
    """[(class, case name, arguments, backend key or None)] in the recorded order"""
    out = [("VecBrain", case_name(kw, be), kw, be) for be, kw in BRAIN_CASES]
    for cls, cases in (("VecIQN", IQN_CASES), ("VecSAC", SAC_CASES), ("VecActorCritic", AC_CASES)):
        out += [(cls, case_name(kw), kw, None) for kw in cases]
    return out


def run_constructors(errors=None):
    out = {}
    for cls, name, kw, be in constructor_cases():
        text, e = construct(cls, kw, be)
        out.setdefault(cls, []).append([name, text])
        if errors is not None and e is not None:
            errors.append(e)
    return out


# ---------------------------------------------------------------- load() refusals
Z = lambda *x: np.array(x, np.int64)
F = lambda *x: np.array(x, np.float64)
S = lambda x: np.array([x])
BRAIN_ATTRS = ("world", "n_step", "quantiles", "arch", "support", "noisy", "sigma0", "munchausen", "huber")       # in the order load reads them
IQN_ATTRS = ("prioritized", ("n", "batch", "fc_width", "n_step"), "seed", ("n_tau", "n_tau_next", "n_tau_act", "kappa"), "dueling", "munchausen",
             ("temp", "alpha", "clip"))
SAC_ATTRS = (("n", "batch", "fc_width"), "seed")
AC_ATTRS = ("algo", ("n", "T", "fc_width"), "seed")
BRAIN_SELF = dict(world=1, n_step=1, quantiles=None, arch="plain", support=None, noisy=False, sigma0=None, munchausen=None, huber=0.0)
IQN_SELF = dict(prioritized=False, n=4, batch=4, fc_width=128, n_step=1, seed=3, n_tau=2, n_tau_next=2, n_tau_act=4, kappa=1.0, dueling=False,
                munchausen=False, temp=0.03, alpha=0.9, clip=-1.0)
IQN_FILE = dict(head=S("iqn"), scalars=Z(0, 3, 4, 4, 128, 2, 100, 1, 0, 500), iqn=F(2, 2, 4, 1.0, 1.0))
SAC_SELF = dict(n=4, batch=4, fc_width=128, seed=3)
AC_SELF = dict(algo="a2c", n=4, T=2, fc_width=128, seed=3)
SC = Z(0, 0, 1, 3)                                           # a VecBrain file's scalars: timeStep, onlineTimeStep, world, seed
C51 = dict(support=F(51, -10, 10))
QR = dict(head=S("qr"), quantiles=F(51, 1.0))

# (class, case, the file's arrays, how many of the class's attribute groups the object carries, the attributes that differ from *_SELF)
LOAD_CASES = [
    ("VecBrain", "ac head", dict(head=S("ac"), scalars=SC), 1, {}),
    ("VecBrain", "sac head", dict(head=S("sac"), scalars=SC), 1, {}),
    ("VecBrain", "iqn head", dict(head=S("iqn"), scalars=SC), 1, {}),
    ("VecBrain", "world", dict(scalars=Z(0, 0, 2, 3)), 1, {}),
    ("VecBrain", "world, old file", dict(scalars=Z(0, 0)), 1, dict(world=2)),
    ("VecBrain", "n_step", dict(scalars=SC, n_step=Z(3)), 2, {}),
    ("VecBrain", "n_step, old file", dict(scalars=SC), 2, dict(n_step=3)),
    ("VecBrain", "qr file, scalar brain", dict(scalars=SC, **QR), 4, {}),
    ("VecBrain", "scalar file, qr brain", dict(scalars=SC), 4, dict(quantiles=(51, 1.0), arch="qr")),
    ("VecBrain", "c51 file, qr brain", dict(scalars=SC, **C51), 4, dict(quantiles=(51, 1.0), arch="qr")),
    ("VecBrain", "qr file, qrdueling brain", dict(scalars=SC, **QR), 4, dict(quantiles=(51, 1.0), arch="qrdueling")),
    ("VecBrain", "quantiles", dict(scalars=SC, **QR), 4, dict(quantiles=(32, 1.0), arch="qr")),
    ("VecBrain", "kappa", dict(scalars=SC, **QR), 4, dict(quantiles=(51, 0.5), arch="qr")),
    ("VecBrain", "scalar file, c51 brain", dict(scalars=SC), 5, dict(arch="c51", support=(51, -10.0, 10.0))),
    ("VecBrain", "c51 file, scalar brain", dict(scalars=SC, **C51), 5, {}),
    ("VecBrain", "support", dict(scalars=SC, **C51), 5, dict(arch="c51", support=(11, -10.0, 10.0))),
    ("VecBrain", "c51 file, c51dueling brain", dict(scalars=SC, **C51), 5, dict(arch="c51dueling", support=(51, -10.0, 10.0))),
    ("VecBrain", "c51dueling file, c51 brain", dict(scalars=SC, head=S("c51dueling"), **C51), 5, dict(arch="c51", support=(51, -10.0, 10.0))),
    ("VecBrain", "noisy file", dict(scalars=SC, noisy=Z(1), sigma0=F(0.5), **C51), 7, dict(arch="c51", support=(51, -10.0, 10.0))),
    ("VecBrain", "noisy brain", dict(scalars=SC, **C51), 7, dict(arch="c51", support=(51, -10.0, 10.0), noisy=True, sigma0=0.5)),
    ("VecBrain", "munchausen", dict(scalars=SC, munchausen=F(0.03, 0.9, -1.0)), 8, dict(munchausen=(0.05, 0.9, -1.0))),
    ("VecBrain", "huber file", dict(scalars=SC, huber=F(1.0)), 9, {}),
    ("VecBrain", "huber brain", dict(scalars=SC), 9, dict(huber=1.0)),
    ("VecBrain", "munchausen and huber", dict(scalars=SC, munchausen=F(0.03, 0.9, -1.0), huber=F(1.0)), 9, dict(munchausen=(0.03, 0.5, -1.0))),
    ("VecIQN", "sac head", dict(head=S("sac")), 0, {}),
    ("VecIQN", "ac head", dict(head=S("ac")), 0, {}),
    ("VecIQN", "no head", dict(scalars=SC), 0, {}),
    ("VecIQN", "c51 head", dict(scalars=SC, **C51), 0, {}),
    ("VecIQN", "qr head", dict(scalars=SC, **QR), 0, {}),
    ("VecIQN", "prioritized file", dict(IQN_FILE, prioritized=Z(1)), 1, {}),
    ("VecIQN", "prioritized loop, old file", IQN_FILE, 1, dict(prioritized=True)),
    ("VecIQN", "n_envs", IQN_FILE, 2, dict(n=8)),
    ("VecIQN", "n_step", dict(IQN_FILE, scalars=Z(0, 3, 4, 4, 128, 2, 100, 3, 0, 500)), 2, {}),
    ("VecIQN", "seed", IQN_FILE, 3, dict(seed=4)),
    ("VecIQN", "n_tau", IQN_FILE, 4, dict(n_tau=8)),
    ("VecIQN", "kappa", IQN_FILE, 4, dict(kappa=0.5)),
    ("VecIQN", "dueling file", dict(IQN_FILE, dueling=Z(1)), 5, {}),
    ("VecIQN", "dueling loop, old file", IQN_FILE, 5, dict(dueling=True)),
    ("VecIQN", "munchausen file", dict(IQN_FILE, munchausen=F(1.0, 0.03, 0.9, -1.0)), 6, {}),
    ("VecIQN", "munchausen loop, old file", IQN_FILE, 6, dict(munchausen=True)),
    ("VecIQN", "munchausen values", dict(IQN_FILE, munchausen=F(1.0, 0.03, 0.9, -1.0)), 7, dict(munchausen=True, temp=0.05)),
    ("VecSAC", "iqn head", dict(head=S("iqn")), 0, {}),
    ("VecSAC", "ac head", dict(head=S("ac")), 0, {}),
    ("VecSAC", "no head", dict(scalars=SC), 0, {}),
    ("VecSAC", "c51 head", dict(scalars=SC, **C51), 0, {}),
    ("VecSAC", "batch", dict(head=S("sac"), scalars=Z(0, 3, 4, 2, 128, 2)), 1, {}),
    ("VecSAC", "seed", dict(head=S("sac"), scalars=Z(0, 4, 4, 4, 128, 2)), 2, {}),
    ("VecActorCritic", "iqn head", dict(head=S("iqn")), 0, {}),
    ("VecActorCritic", "sac head", dict(head=S("sac")), 0, {}),
    ("VecActorCritic", "no head", dict(scalars=SC), 0, {}),
    ("VecActorCritic", "qr head", dict(scalars=SC, **QR), 0, {}),
    ("VecActorCritic", "ppo file, a2c loop", dict(head=S("ac"), ppo=F(4, 4, 0.2, 0.0, 1.0), scalars=Z(0, 0, 0, 3, 4, 2, 128)), 1, {}),
    ("VecActorCritic", "a2c file, ppo loop", dict(head=S("ac"), scalars=Z(0, 0, 0, 3, 4, 2, 128)), 1, dict(algo="ppo")),
    ("VecActorCritic", "rollout", dict(head=S("ac"), scalars=Z(0, 0, 0, 3, 4, 5, 128)), 2, {}),
    ("VecActorCritic", "seed", dict(head=S("ac"), scalars=Z(0, 0, 0, 4, 4, 2, 128)), 3, {}),
]


def bare(cls, groups, changed):
    """Class.__new__(Class) carrying the first `groups` attribute groups of what its load reads"""
    from dqnflappybird_amd.vecac import VecActorCritic
    from dqnflappybird_amd.vecbrain import VecBrain
    from dqnflappybird_amd.veciqn import VecIQN
    from dqnflappybird_amd.vecsac import VecSAC
    klass, attrs, mine = {"VecBrain": (VecBrain, BRAIN_ATTRS, BRAIN_SELF), "VecIQN": (VecIQN, IQN_ATTRS, IQN_SELF), "VecSAC": (VecSAC, SAC_ATTRS, SAC_SELF),
                          "VecActorCritic": (VecActorCritic, AC_ATTRS, AC_SELF)}[cls]
    obj = klass.__new__(klass)
    names = [n for g in attrs[:groups] for n in ((g,) if isinstance(g, str) else g)]
    assert set(changed) <= set(names), (cls, changed, names)
    obj.__dict__.update({n: changed.get(n, mine[n]) for n in names})
    return obj


def run_loads(tmp, errors=None):
    out = {}
    for i, (cls, case, arrays, groups, changed) in enumerate(LOAD_CASES):
        path = os.path.join(str(tmp), f"case{i}.npz")
        np.savez(path, online=np.zeros(3, np.float32), **arrays)
        obj = bare(cls, groups, changed)
        before = dict(obj.__dict__)
        try:
            obj.load(path)
            text = "accepted"
        except ValueError as e:
            text = str(e).replace(str(tmp), "<dir>")
            if errors is not None:
                errors.append(e)
        assert obj.__dict__ == before, f"{cls} {case}: a refused load changed the object"
        out.setdefault(cls, []).append([case, text])
    return out


# ---------------------------------------------------------------- VecBrain on the CPU stand-in
CPU_ALGOS = ("dqn", "nature", "per")
CPU_KW = dict(n_envs=4, batch=4, capacity=64, observe=2, seed=3)


def digests(path):
    """{key: [dtype, shape, SHA-256 of the bytes]} of every array of a checkpoint"""
    z = np.load(path)
    return {k: [str(z[k].dtype), list(z[k].shape), hashlib.sha256(np.ascontiguousarray(z[k]).tobytes()).hexdigest()] for k in z.files}


def lines_of(run, *a, **k):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        run(*a, **k)
    return buf.getvalue().splitlines()


def run_and_resume(make, tmp, name, steps, log_every, more, more_every):
    """the four things a loop case records: the lines of run(steps, log_every), its checkpoint, the lines a fresh object prints over
    `more` steps after loading it, and that object's checkpoint"""
    a = make()
    out = {"lines": lines_of(a.run, steps, log_every=log_every)}
    first, second = os.path.join(str(tmp), f"{name}.npz"), os.path.join(str(tmp), f"{name}.resumed.npz")
    a.save(first)
    out["checkpoint"] = digests(first)
    b = make()
    b.load(first)
    out["resumed_lines"] = lines_of(b.run, more, log_every=more_every)
    b.save(second)
    out["resumed_checkpoint"] = digests(second)
    return out


def run_cpu_brain(algo, tmp):
    from dqnflappybird_amd.vecbrain import VecBrain
    from tests.cpu_backend import CpuVecBackend
    try:
        return run_and_resume(lambda: VecBrain(algo=algo, backend=CpuVecBackend(), **CPU_KW), tmp, algo, 6, 3, 2, 1)
    except Exception as e:                                   # (recorded like any other answer: the stand-in has no prioritized memory)
        return {"raises": f"{type(e).__name__}: {e}"}


# ---------------------------------------------------------------- the tests
@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)["host"]


def same_as_recorded(what, got, want):
    got = json.loads(json.dumps(got))
    assert [c for c, _ in got] == [c for c, _ in want], f"{what}: the cases run and the recorded ones differ"
    wrong = [(c, g, w) for (c, g), (_, w) in zip(got, want) if g != w]
    for c, g, w in wrong[:10]:
        print(f"{what} {c}:\n  got      {g}\n  recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases of {what} answer differently from the record"
    refused = sum(1 for _, g in got if g != "accepted")
    print(f"{what}: {len(got)} cases, {refused} refused")
    return refused


@pytest.fixture(scope="module")
def constructed():
    return run_constructors()


@pytest.mark.parametrize("cls", ["VecBrain", "VecIQN", "VecSAC", "VecActorCritic"])
def test_constructor_refuses_as_recorded(table, constructed, cls):
    refused = same_as_recorded(f"{cls}()", constructed[cls], table["constructors"][cls])
    assert 0 < refused < len(constructed[cls])


def test_load_refuses_as_recorded(table, tmp_path):
    got = run_loads(tmp_path)
    assert sorted(got) == sorted(table["loads"])
    for cls in got:
        assert same_as_recorded(f"{cls}.load", got[cls], table["loads"][cls]) == len(got[cls])


@pytest.mark.parametrize("algo", CPU_ALGOS)
def test_cpu_brain_prints_and_saves_as_recorded(table, tmp_path, algo):
    got = json.loads(json.dumps(run_cpu_brain(algo, tmp_path)))
    want = table["cpu_brain"][algo]
    assert sorted(got) == sorted(want)
    for part in got:
        assert got[part] == want[part], f"VecBrain({algo!r}) on the CPU stand-in: {part} differs from the record"


# ---------------------------------------------------------------- recording
def raise_sites():
    """every `raise ValueError` in __init__, check_* and load of the four modules -> {(module file, first line, last line)}"""
    import dqnflappybird_amd
    sites = set()
    for mod in MODULES:
        path = os.path.join(os.path.dirname(dqnflappybird_amd.__file__), mod + ".py")
        with open(path) as f:
            tree = ast.parse(f.read())
        for fn in ast.walk(tree):
            if isinstance(fn, ast.FunctionDef) and (fn.name in ("__init__", "load") or fn.name.startswith("check_")):
                for node in ast.walk(fn):
                    if isinstance(node, ast.Raise) and isinstance(node.exc, ast.Call) and getattr(node.exc.func, "id", None) == "ValueError":
                        sites.add((os.path.realpath(path), node.lineno, node.end_lineno))
    return sites


def sites_named(errors, sites):
    hit = set()
    for e in errors:
        tb = e.__traceback__
        while tb is not None:
            path, line = os.path.realpath(tb.tb_frame.f_code.co_filename), tb.tb_lineno
            hit |= {s for s in sites if s[0] == path and s[1] <= line <= s[2]}
            tb = tb.tb_next
    return hit


def merge_record(path, part, rec):
    whole = {}
    if os.path.exists(path):
        with open(path) as f:
            whole = json.load(f)
    whole[part] = rec
    with open(path, "w") as f:
        json.dump(whole, f, indent=0, sort_keys=True)
        f.write("\n")


def record(path):
    import tempfile
    errors = []
    with tempfile.TemporaryDirectory() as tmp:
        rec = {"constructors": run_constructors(errors), "loads": run_loads(tmp, errors), "cpu_brain": {a: run_cpu_brain(a, tmp) for a in CPU_ALGOS}}
    sites = raise_sites()
    missed = sorted(sites - sites_named(errors, sites))
    for s in missed:
        print(f"not reached: {os.path.basename(s[0])}:{s[1]}")
    if missed:
        sys.exit(f"{len(missed)} of {len(sites)} raise sites are reached by no recorded refusal")
    rec["raise_sites"] = len(sites)
    merge_record(path, "host", rec)
    for part in ("constructors", "loads"):
        for cls, cases in rec[part].items():
            print(f"{part} {cls}: {len(cases)} cases, {sum(1 for _, t in cases if t != 'accepted')} refused")
    print(f"cpu_brain: {', '.join(f'{a}: {sorted(v)}' for a, v in rec['cpu_brain'].items())}")
    print(f"{len(sites)} raise sites, all reached -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_loop_record_host --record [PATH]")
