"""What the Huber loss and the double target with prioritized replay cost: µs per fb_vec_step of 'double' against 'double' with
delta = 1 (uniform memory; the split schedule where 'double' takes it) and of 'per' against 'doubleper' against 'doubleper' with
delta = 1 (prioritized memory: two forward slices against three).

    python tools/time_huber.py [--envs 256,1024,4096] [--steps 300] [--warmup 300] [--repeats 5] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.

One pipeline per (envs, config) -- VecStep on the plain 512 / 2 net with B = 32 and a 1 M-slot memory -- warmed up, then --repeats rounds
of --steps timed steps, the configs alternated within each round.  Reported: the median and the spread of the rounds' µs per step; the
spread of the unchanged configs ('double', 'per') is the yardstick for the differences.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402

# config -> (algo, prioritized memory, delta)
CONFIGS = {"double": ("double", False, 0.0), "double+huber": ("double", False, 1.0), "per": ("per", True, 0.0),
           "doubleper": ("doubleper", True, 0.0), "doubleper+huber": ("doubleper", True, 1.0)}


def pipeline(n_envs, config, cap, batch=32, gamma=0.99):
    algo, per, delta = CONFIGS[config]
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, "plain", max_batch=max(n_envs, batch))
    rep = VecReplay(cap, n_envs, prioritized=per)
    rep.seed(3, "numpy" if per else "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    net.set_huber(delta)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return dict(net=net, rep=rep, step=VecStep(env, rep, net, batch, algo, gamma), k=0)


def timed_vec(p, k):
    step = p["step"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(0.01, seed=2, step=p["k"] + i, train=True)
    torch.cuda.synchronize()
    p["k"] += k
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,1024,4096")
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
        emit(f"# tools/time_huber.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit("#  what          envs  config            median_us   min_us   max_us")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {c: pipeline(n_envs, c, a.capacity) for c in CONFIGS}
            for p in pipes.values():
                for i in range(a.warmup):
                    p["step"](0.01, seed=2, step=p["k"], train=i >= 4)
                    p["k"] += 1
            res = {c: [] for c in pipes}
            for _ in range(a.repeats):
                for c in res:
                    res[c].append(timed_vec(pipes[c], a.steps))
            for c, v in res.items():
                emit(f"  fb_vec_step  {n_envs:5d}  {c:16s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
            for c in ("double", "double+huber"):
                issued, clean = pipes[c]["net"].split_stats()
                emit(f"#   {c}: split schedule on {issued} of {pipes[c]['k']} steps, {clean} minibatches beside their env step")
            del pipes
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
