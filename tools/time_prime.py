"""What initial priorities from acting-time TD errors cost per vector step: µs per fb_vec_step (algo per, B = 32, a 1 M-slot
prioritized memory in the fast mode) with priority_init 'max' against 'td' (include/fbdqn.h FB_PER_INIT_TD).

    python tools/time_prime.py [--envs 1024,4096] [--inits max,td] [--n-step 1] [--steps 300] [--warmup 400] [--repeats 5] [--out FILE]

One pipeline per (envs, init), all built and warmed up first; every round times each of them once, in turn, so that drift of the
machine falls on all of them alike.  Reported: the median, minimum and maximum of the rounds' µs per step, and for 'td' the
difference of the medians.  The 'max' leg never calls the new setting: its code path is the one of before it existed (what
tools/time_nstep.py --algo per --per-mode fast --ns 1 times).  'td' adds the prime launch, behind the env launch (the acting head
keeps riding in it).  Rows go to stdout, and are appended to --out when one is given.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402


def pipeline(n_envs, init, n, cap, batch=32, gamma=0.99):
    env, net = VecGameState(n_envs, seed=1), QNet(2, 512, "plain", max_batch=max(n_envs, batch))
    rep = VecReplay(cap, n_envs, prioritized=True, n_step=n, gamma=gamma)
    rep.seed(3, "numpy"); rep.set_per_mode("fast")
    if init == "td":
        rep.set_priority_init("td", gamma)
    net.init_params(5, which=0); net.init_params(6, which=1)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return VecStep(env, rep, net, batch, "per", gamma)


def timed(step, k, k0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(0.01, seed=2, step=k0 + i, train=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1024,4096")
    ap.add_argument("--inits", default="max,td")
    ap.add_argument("--n-step", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=400)
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
        emit(f"# tools/time_prime.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit("#  envs  n  init   median_us   min_us   max_us   td - max (medians)")
        inits = a.inits.split(",")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {init: pipeline(n_envs, init, a.n_step, a.capacity) for init in inits}
            for step in pipes.values():
                for i in range(a.warmup):
                    step(0.01, seed=2, step=i, train=i >= max(4, a.n_step))
            k0 = a.warmup
            res = {init: [] for init in inits}
            for _ in range(a.repeats):
                for init, step in pipes.items():
                    res[init].append(timed(step, a.steps, k0))
                k0 += a.steps
            for init in inits:
                v = res[init]
                extra = f"   {statistics.median(v) - statistics.median(res['max']):+.1f}" if init == "td" and "max" in res else ""
                emit(f"  {n_envs:5d} {a.n_step:2d}  {init:4s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}{extra}")
            del pipes
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
