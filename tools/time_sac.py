"""What discrete SAC costs: us per fb_sac_step against fb_vec_step of 'double' on a dueling net under the one-stream schedule
(fb_vec_step_set_schedule(0)) at the same env count, and us per SAC train step (exported gradient) against 'double's with flat_grad.

    python tools/time_sac.py [--envs 1024,4096] [--batch 32] [--steps 300] [--warmup 100] [--repeats 5] [--per] [--n-step K] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.

loop step: SacStep (policy head, push + sample and the soft target update as launches of their own, rho = 0.005) and VecStep('double',
train=True) on a dueling net (head and push riding in the env launch), 512 / 2 nets, one pipeline each, warmed up, then --repeats
rounds of --steps timed steps, the two alternated within each round.  The yardstick for a difference is the dependent empty launch:
the tool runs tools/mb/mb_launch (building it from tools/mb/mb_launch.hip if the binary is missing) as a child process first.
train step: vec.sac_train_from_replay(flat_grad) and vec.train_from_replay('double', flat_grad) at --batch on the memories the steps
filled, the same alternation.  Reported: the median and the spread of the rounds.
--per: fb_sac_per_step on a prioritized memory of the same capacity (n = 1 and, with --n-step K > 1, n = K as well) runs beside them in
the same rounds, and vec.sac_per_train_from_replay beside the two train steps.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd import _lib as L  # noqa: E402
from dqnflappybird_amd.vec import (QNet, SacPerStep, SacStep, VecGameState, VecReplay, VecStep, sac_per_train_from_replay,  # noqa: E402
                                   sac_train_from_replay, train_from_replay)
from tools.time_a2c import launch_floor, timed  # noqa: E402


CAPACITY = 1_000_000


def pipeline(n_envs, arch, batch, per_n=0):
    """per_n > 0: a prioritized memory made with that n (the numpy generator, the reference-order tree) and fb_sac_per_step"""
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, arch, max_batch=max(n_envs, 256))
    rep = VecReplay(CAPACITY, n_envs, prioritized=True, n_step=per_n, gamma=0.99) if per_n else VecReplay(CAPACITY, n_envs)
    rep.seed(3, None if per_n else "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    net.set_hparams(lr=1e-6)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    if per_n:
        step = SacPerStep(env, rep, net, batch, 0.99, 0.005)
    else:
        step = SacStep(env, rep, net, batch, 0.99, 0.005) if arch == "sac" else VecStep(env, rep, net, batch, "double", 0.99)
    return dict(env=env, net=net, rep=rep, step=step, arch=arch, k=0, per_n=per_n)


def one(p):
    if p["arch"] == "sac":
        p["step"](seed=2, step=p["k"], train=p["k"] >= p["per_n"] - 1)      # (an n-step memory: n pushes before the first draw)
    else:
        p["step"](0.1, seed=2, step=p["k"], train=True)
    p["k"] += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1024,4096")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--per", action="store_true", help="also time fb_sac_per_step / sac_per_train_from_replay on a prioritized memory")
    ap.add_argument("--n-step", type=int, default=1, help="--per: also at this n (> 1)")
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        def row(what, n, config, v):
            emit(f"  {what:13s} {n:5d}  {config:28s} {statistics.median(v):10.1f} {min(v):9.1f} {max(v):9.1f}  us")

        emit(f"# tools/time_sac.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        floor = launch_floor()                   # (a child process of its own, before this one holds much of the GPU)
        if isinstance(floor, str):
            emit(f"# empty dependent launch: {floor}")
        else:
            for shape, us in floor:
                emit(f"# empty dependent launch (tools/mb/mb_launch, {shape}): {us:.2f} us per launch")
        L.check(L.lib().fb_vec_step_set_schedule(0), "fb_vec_step_set_schedule")      # the one-stream order: what fb_sac_step runs in
        emit("#  what           envs  config                           median       min       max")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {"fb_sac_step (rho 0.005)": pipeline(n_envs, "sac", a.batch), "fb_vec_step double/dueling": pipeline(n_envs, "dueling", a.batch)}
            for n in ([1] + ([a.n_step] if a.n_step > 1 else [])) if a.per else []:
                pipes[f"fb_sac_per_step n={n}"] = pipeline(n_envs, "sac", a.batch, per_n=n)
            for p in pipes.values():
                for _ in range(a.warmup):
                    one(p)
            res = {c: [] for c in pipes}
            for _ in range(a.repeats):
                for c, p in pipes.items():
                    res[c].append(timed(lambda: one(p), a.steps))
            for c, v in res.items():
                row("loop step", n_envs, c, v)
            sp, dp = pipes["fb_sac_step (rho 0.005)"], pipes["fb_vec_step double/dueling"]
            idx = (torch.arange(a.batch, dtype=torch.int64) * 7).cuda()
            g_s = torch.zeros(sp["net"].n_params, dtype=torch.float32, device="cuda")
            g_d = torch.zeros(dp["net"].n_params, dtype=torch.float32, device="cuda")
            steps = {"sac (3 slices, 3 heads)": lambda: sac_train_from_replay(sp["rep"], sp["net"], idx, 0.99, flat_grad=g_s),
                     "double (3 slices)": lambda: train_from_replay(dp["rep"], dp["net"], "double", idx, 0.99, flat_grad=g_d)}
            if a.per:
                pp = pipes["fb_sac_per_step n=1"]
                leaf, ones = idx + (CAPACITY - 1), torch.ones(a.batch, dtype=torch.float32, device="cuda")      # (a prioritized memory is read at its leaves)
                g_p = torch.zeros(pp["net"].n_params, dtype=torch.float32, device="cuda")
                steps["sac per (weights, priority)"] = lambda: sac_per_train_from_replay(pp["rep"], pp["net"], leaf, ones, 0.99, flat_grad=g_p)
            for fn in steps.values():
                for _ in range(20):
                    fn()
            rc = {c: [] for c in steps}
            for _ in range(a.repeats):
                for c, fn in steps.items():
                    rc[c].append(timed(fn, a.steps))
            for c, v in rc.items():
                row(f"train B={a.batch}", n_envs, c, v)
            del pipes, sp, dp, steps
            torch.cuda.synchronize()
        L.check(L.lib().fb_vec_step_set_schedule(1), "fb_vec_step_set_schedule")


if __name__ == "__main__":
    main()
