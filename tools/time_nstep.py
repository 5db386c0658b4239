"""What n-step returns cost per vector step: µs per fb_vec_step at n = 1, 3, 5, under the split schedule and on one stream.

    python tools/time_nstep.py [--configs 1024:plain,4096:dueling] [--ns 1,3,5] [--steps 300] [--warmup 400] [--repeats 5] [--out FILE]
                               [--algo nature|per] [--per-mode exact|fast]

Rows go to stdout, and are appended to --out when one is given.

One pipeline per (envs, arch, n): VecStep (nature, B = 32, a 1 M-slot memory, the bench's own shape) warmed up for --warmup steps, then
--repeats rounds of --steps timed steps under each schedule (fb_vec_step_set_schedule 1 / 0), alternated.  Reported per schedule: the
median and the spread of the rounds' µs per step; for the split schedule also the fraction of minibatches that started beside their
env step (split_stats: clean / issued over the timed steps).
--algo per: a prioritized memory created with n-step returns (VecReplay(prioritized=True, n_step=n)) in --per-mode; fb_vec_step
never takes the split schedule for it, so one schedule is timed, and the pipelines of all n are built first and timed in turn within
every round (each round times every n once), so that drift of the machine falls on all of them alike.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd import _lib as L  # noqa: E402
from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402


def pipeline(n_envs, arch, n, cap, batch=32, gamma=0.99, algo="nature", per_mode="exact"):
    per = algo == "per"
    env, net = VecGameState(n_envs, seed=1), QNet(2, 512, arch, max_batch=max(n_envs, batch))
    rep = VecReplay(cap, n_envs, prioritized=per, n_step=n if per else 1, gamma=gamma)
    if per:
        rep.seed(3, "numpy"); rep.set_per_mode(per_mode)
    else:
        rep.seed(3, "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    if n > 1 and not per:
        rep.set_n_step(n, gamma)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return net, VecStep(env, rep, net, batch, algo, gamma)


def main_per(a, emit):
    """--algo per: every n's pipeline, timed in turn within each round (one schedule: the prioritized step never splits)"""
    emit("#  envs arch     n  per_mode   median_us   min_us   max_us")
    for cfg in a.configs.split(","):
        n_envs, arch = cfg.split(":")
        n_envs = int(n_envs)
        ns = [int(x) for x in a.ns.split(",")]
        pipes = {n: pipeline(n_envs, arch, n, a.capacity, algo="per", per_mode=a.per_mode) for n in ns}
        for n, (_, step) in pipes.items():
            for i in range(a.warmup):
                step(0.01, seed=2, step=i, train=i >= max(4, n))      # (a prioritized n-step memory trains from its n-th push on)
        k0 = a.warmup
        res = {n: [] for n in ns}
        for _ in range(a.repeats):
            for n, (_, step) in pipes.items():
                res[n].append(timed(step, a.steps, k0))
            k0 += a.steps
        for n in ns:
            v = res[n]
            emit(f"  {n_envs:5d} {arch:8s} {n:2d}  {a.per_mode:8s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
        del pipes
        torch.cuda.synchronize()


def timed(step, k, k0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(0.01, seed=2, step=k0 + i, train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="1024:plain,4096:dueling")
    ap.add_argument("--ns", default="1,3,5")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    ap.add_argument("--algo", default="nature", choices=["nature", "per"])
    ap.add_argument("--per-mode", default="exact", choices=["exact", "fast"], help="--algo per: how the SumTree is kept")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/time_nstep.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        if a.algo == "per":
            main_per(a, emit)
            return
        emit("#  envs arch     n  schedule   median_us   min_us   max_us   clean_fraction")
        for cfg in a.configs.split(","):
            n_envs, arch = cfg.split(":")
            n_envs = int(n_envs)
            for n in [int(x) for x in a.ns.split(",")]:
                net, step = pipeline(n_envs, arch, n, a.capacity)
                L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
                k0 = 0
                for i in range(a.warmup):
                    step(0.01, seed=2, step=k0, train=i >= 4)
                    k0 += 1
                res = {1: [], 0: []}
                clean = issued = 0
                for _ in range(a.repeats):
                    for sched in (1, 0):
                        L.check(L.lib().fb_vec_step_set_schedule(sched), "schedule")
                        i0, c0 = net.split_stats()
                        res[sched].append(timed(step, a.steps, k0))
                        k0 += a.steps
                        i1, c1 = net.split_stats()
                        if sched:
                            issued += i1 - i0; clean += c1 - c0
                L.check(L.lib().fb_vec_step_set_schedule(1), "schedule")
                for sched in (1, 0):
                    v = res[sched]
                    cf = f"{clean / issued:.3f}" if sched and issued else "-"
                    emit(f"  {n_envs:5d} {arch:8s} {n:2d}  {'split' if sched else 'one':8s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}   {cf}")
                del step, net
                torch.cuda.synchronize()


if __name__ == "__main__":
    main()
