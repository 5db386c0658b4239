"""What IQN costs: us per fb_iqn_step against fb_vec_step of 'qr' (a QR net, N = 51) and of 'double' (a plain net) under the one-stream
schedule (fb_vec_step_set_schedule(0)) at the same env count; us per train step alone (exported gradient) of the three; and us per
acting forward (act_nib) of an IQN net against a plain net's, which should differ by nothing: the fold is refreshed behind Adam, not
on the acting path.  The prioritized forms run beside them on prioritized memories of the same capacity: fb_iqn_per_step and fb_vec_step
of 'qrper' -- over the uniform step they pay Memory.store's tree part, Memory.sample and Memory.batch_update.  The dueling IQN net
(arch 'iqndueling') has a row beside every IQN row: its train step forms the effective column in place and splits the head's gradient,
its acting path is the same plain head over the fold.  Munchausen IQN (QNet.set_iqn_munchausen, the paper's (0.03, 0.9, -1)) has a row
beside the plain IQN rows: the same three slices, an all-columns theta of the target net and one more plain head inside the loss launch.
--noisy times noisy IQN instead (QNet arch 'iqnduelingnoisy'): fb_iqn_per_step of the dueling net on a prioritized 3-step memory, non-noisy
against noisy with the shared acting sample against noisy with per-env acting noise, their train steps alone, and act_nib against
act_nib_env_noise.

    python tools/time_iqn.py [--noisy] [--envs 256,1024,4096] [--batch 32] [--steps 300] [--warmup 100] [--repeats 5] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.  Every pipeline is warmed up, then --repeats rounds of --steps timed
calls, the configurations alternated within each round, in one process.  Reported: the median and the spread of the rounds.  The
yardstick for a difference is the dependent empty launch (tools/mb/mb_launch, run as a child process first).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd import _lib as L  # noqa: E402
from dqnflappybird_amd.vec import (IQN_ALL_ARCHS as IQN_ARCHS, IqnPerStep, IqnStep, QNet, VecGameState, VecReplay, VecStep, iqn_per_train_from_replay,  # noqa: E402
                                   iqn_train_from_replay, train_from_replay)
from tools.time_a2c import launch_floor, timed  # noqa: E402

MIQN = "munchausen"                                 # (in a config's name: the IQN net of that row has the Munchausen target on)
CONFIGS = {"fb_iqn_step (N 8, N' 8, K 32)": ("iqn", None), "fb_iqn_step munchausen": ("iqn", None), "fb_iqn_step dueling": ("iqndueling", None),
           "fb_iqn_per_step (N 8, N' 8, K 32)": ("iqn", "per"), "fb_iqn_per_step munchausen": ("iqn", "per"),
           "fb_iqn_per_step dueling": ("iqndueling", "per"), "fb_vec_step qr (N 51)": ("qr", "qr"),
           "fb_vec_step qrper (N 51)": ("qr", "qrper"), "fb_vec_step double": ("plain", "double")}
ENV_NOISE = "per-env"                               # (in a config's name: the noisy net of that row acts with per-env noise)
NOISY_CONFIGS = {"fb_iqn_per_step dueling n 3": ("iqndueling", "per"), "fb_iqn_per_step dueling n 3 noisy shared": ("iqnduelingnoisy", "per"),
                 "fb_iqn_per_step dueling n 3 noisy per-env": ("iqnduelingnoisy", "per")}
CAPACITY = 1_000_000


def pipeline(n_envs, arch, algo, batch, munchausen=False, n_step=1, env_noise=False):
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, arch, max_batch=max(n_envs, 256))
    if munchausen:
        net.set_iqn_munchausen(True)
    if env_noise:
        net.set_acting_noise("env")
    per = algo in ("per", "qrper")                   # (a prioritized memory: the numpy generator, the reference-order tree)
    rep = VecReplay(CAPACITY, n_envs, prioritized=per, n_step=n_step, gamma=0.99)
    rep.seed(3, None if per else "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    net.set_hparams(lr=1e-6)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    step = (IqnPerStep if per else IqnStep)(env, rep, net, batch, 0.99) if arch in IQN_ARCHS else VecStep(env, rep, net, batch, algo, 0.99)
    p = dict(env=env, net=net, rep=rep, step=step, arch=arch, algo=algo, per=per, k=0)
    for _ in range(n_step - 1):                     # (an n-step memory: the first n - 1 steps only store)
        step(0.1, seed=2, step=p["k"], train=False)
        p["k"] += 1
    return p


def one(p):
    p["step"](0.1, seed=2, step=p["k"], train=True)
    p["k"] += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,1024,4096")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    ap.add_argument("--noisy", action="store_true", help="the noisy IQN configurations (dueling net, prioritized 3-step memory) instead of the others")
    a = ap.parse_args()
    configs, n_step = (NOISY_CONFIGS, 3) if a.noisy else (CONFIGS, 1)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        def row(what, n, config, v):
            emit(f"  {what:13s} {n:5d}  {config:42s} {statistics.median(v):10.1f} {min(v):9.1f} {max(v):9.1f}  us")

        def rounds(fns, warm):
            for fn in fns.values():
                for _ in range(warm):
                    fn()
            res = {c: [] for c in fns}
            for _ in range(a.repeats):
                for c, fn in fns.items():
                    res[c].append(timed(fn, a.steps))
            return res

        emit(f"# tools/time_iqn.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        floor = launch_floor()                   # (a child process of its own, before this one holds much of the GPU)
        if isinstance(floor, str):
            emit(f"# empty dependent launch: {floor}")
        else:
            for shape, us in floor:
                emit(f"# empty dependent launch (tools/mb/mb_launch, {shape}): {us:.2f} us per launch")
        L.check(L.lib().fb_vec_step_set_schedule(0), "fb_vec_step_set_schedule")      # the one-stream order: what fb_iqn_step runs in
        emit("#  what           envs  config                             median       min       max")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {c: pipeline(n_envs, arch, algo, a.batch, MIQN in c, n_step, ENV_NOISE in c) for c, (arch, algo) in configs.items()}
            for c, v in rounds({c: (lambda p=p: one(p)) for c, p in pipes.items()}, a.warmup).items():
                row("loop step", n_envs, c, v)
            idx = (torch.arange(a.batch, dtype=torch.int64) * 7).cuda()
            grads = {c: torch.zeros(p["net"].n_params, dtype=torch.float32, device="cuda") for c, p in pipes.items()}

            leaf, ones = idx + (CAPACITY - 1), torch.ones(a.batch, dtype=torch.float32, device="cuda")      # (a prioritized memory is read at its leaves)

            def train_fn(c, p):
                if p["arch"] in IQN_ARCHS and p["per"]:
                    return lambda: iqn_per_train_from_replay(p["rep"], p["net"], leaf, ones, 0.99, seed=2, step=1, flat_grad=grads[c])
                if p["arch"] in IQN_ARCHS:
                    return lambda: iqn_train_from_replay(p["rep"], p["net"], idx, 0.99, seed=2, step=1, flat_grad=grads[c])
                if p["per"]:
                    return lambda: train_from_replay(p["rep"], p["net"], p["algo"], leaf, 0.99, flat_grad=grads[c], isw=ones, want_abs_err=True)
                return lambda: train_from_replay(p["rep"], p["net"], p["algo"], idx, 0.99, flat_grad=grads[c])
            for c, v in rounds({c: train_fn(c, p) for c, p in pipes.items()}, 20).items():
                row(f"train B={a.batch}", n_envs, c.replace("fb_iqn_per_step", "iqn per").replace("fb_iqn_step", "iqn").replace("fb_vec_step ", ""), v)
            if a.noisy:                              # the acting forward alone: the fold's head, or the per-env path (restored behind it)
                act = {c: (lambda p=p: p["net"].act_nib_env_noise(p["env"].nib, 0.0, seed=2, step=3)) if ENV_NOISE in c else
                          (lambda p=p: p["net"].act_nib(p["env"].nib, 0.0, seed=2, step=3)) for c, p in pipes.items()}
                for c, v in rounds(act, 20).items():
                    row("act", n_envs, "act_nib_env_noise" if ENV_NOISE in c else "act_nib, noisy net" if "noisy" in c else "act_nib, non-noisy net", v)
                reset = {c: (lambda p=p: p["net"].reset_noise(0, 2, 3)) for c, p in pipes.items() if "noisy shared" in c}
                for c, v in rounds(reset, 20).items():
                    row("reset_noise", n_envs, "draw + rebuild + fold", v)
                del pipes, grads, act, reset
                torch.cuda.synchronize()
                continue
            act = {c: (lambda p=p: p["net"].act_nib(p["env"].nib, 0.1, seed=2, step=3)) for c, p in pipes.items()
                   if p["arch"] in IQN_ARCHS + ("plain",) and not p["per"] and MIQN not in c}
            for c, v in rounds(act, 20).items():
                row("act_nib", n_envs, "dueling iqn net (folded head)" if "dueling" in c else "iqn net (folded head)" if "iqn" in c else "plain net", v)
            del pipes, grads, act
            torch.cuda.synchronize()
        L.check(L.lib().fb_vec_step_set_schedule(1), "fb_vec_step_set_schedule")


if __name__ == "__main__":
    main()
