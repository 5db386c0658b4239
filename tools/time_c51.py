"""What a C51 head costs: µs per fb_vec_step of a C51 net against the plain (nature) head, and µs per train step of fb_train_steps.

    python tools/time_c51.py [--envs 256,1024,4096] [--atoms 51] [--steps 300] [--warmup 300] [--repeats 5] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.

fb_vec_step: one pipeline per (envs, head) -- VecStep with B = 32 and a 1 M-slot uniform memory, the bench's own shape -- warmed up,
then --repeats rounds of --steps timed steps, the heads alternated within each round.  The nature head is timed under both
schedules (a C51 net always takes the one-stream order: include/fbdqn.h), the C51 head under the one it takes.
fb_train_steps: train-only, 10 steps per call on a memory filled by the warm-up, B = 32, the same alternation.
Reported: the median and the spread of the rounds' µs per step.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd import _lib as L  # noqa: E402
from dqnflappybird_amd.vec import QNet, TrainSteps, VecGameState, VecReplay, VecStep  # noqa: E402


def pipeline(n_envs, head, atoms, cap, batch=32, gamma=0.99):
    env = VecGameState(n_envs, seed=1)
    if head == "c51":
        net, algo = QNet(2, 512, "c51", max_batch=max(n_envs, batch), n_atoms=atoms), "c51"
    else:
        net, algo = QNet(2, 512, "plain", max_batch=max(n_envs, batch)), "nature"
    rep = VecReplay(cap, n_envs)
    rep.seed(3, "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return dict(net=net, rep=rep, algo=algo, step=VecStep(env, rep, net, batch, algo, gamma), k=0)


def timed_vec(p, k):
    step = p["step"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(0.01, seed=2, step=p["k"] + i, train=True)
    torch.cuda.synchronize()
    p["k"] += k
    return (time.perf_counter() - t0) / k * 1e6


def timed_train(ts, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        ts(10)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (10 * calls) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,1024,4096")
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/time_c51.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit("#  what          envs  head     schedule   median_us   min_us   max_us")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {h: pipeline(n_envs, h, a.atoms, a.capacity) for h in ("nature", "c51")}
            for p in pipes.values():
                for i in range(a.warmup):
                    p["step"](0.01, seed=2, step=p["k"], train=i >= 4)
                    p["k"] += 1
            res = {("nature", 1): [], ("nature", 0): [], ("c51", 0): []}
            for _ in range(a.repeats):
                for head, sched in res:
                    L.check(L.lib().fb_vec_step_set_schedule(sched), "schedule")
                    res[(head, sched)].append(timed_vec(pipes[head], a.steps))
            L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
            for (head, sched), v in res.items():
                emit(f"  fb_vec_step  {n_envs:5d}  {head:7s}  {'split' if sched else 'one':8s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
            if n_envs == 1024:                   # train-only, on the memories the warm-up filled
                tss = {h: TrainSteps(p["rep"], p["net"], 32, p["algo"], 0.99) for h, p in pipes.items()}
                for ts in tss.values():
                    ts(10)
                rt = {h: [] for h in tss}
                for _ in range(a.repeats):
                    for h, ts in tss.items():
                        rt[h].append(timed_train(ts, max(1, a.steps // 10)))
                for h, v in rt.items():
                    emit(f"  train_steps  {32:5d}  {h:7s}  {'-':8s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
            del pipes
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
