"""What noisy layers add to a Rainbow step: µs per fb_vec_step of rainbow (c51doubleper on the dueling C51 head, prioritized memory,
3-step returns), of rainbow + noisy (the same on a noisy net: two noise draws and materialisations, sigma's gradient, Adam over
[mu | sigma]) and of rainbow + noisy acting with per-env noise (rainbow_noisy_env: mu materialised for acting, sigma's fc1 GEMM on the
scaled activations, the per-env noisy head).

    python tools/time_c51_noisy.py [--envs 256,1024,4096] [--configs rainbow,rainbow_noisy,rainbow_noisy_env] [--atoms 51] [--steps 300]
                                   [--warmup 300] [--repeats 5] [--per-mode exact] [--out FILE]

One pipeline per (envs, config): VecStep with B = 32 and a 1 M-slot memory, warmed up, then --repeats rounds of --steps timed steps,
the configs alternated within each round; epsilon 0 for both.  Reported: the median and the spread of the rounds' µs per step.  Rows
go to stdout, and are appended to --out (profiles/c51_noisy_time.txt unless another file, or '', is given).
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402

CONFIGS = {"rainbow": (False, "shared"), "rainbow_noisy": (True, "shared"), "rainbow_noisy_env": (True, "env")}      # name -> (noisy, acting noise)
ALGO, ARCH, N_STEP = "c51doubleper", "c51dueling", 3


def pipeline(n_envs, noisy, acting, atoms, cap, per_mode, batch=32, gamma=0.99):
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, ARCH, max_batch=max(n_envs, batch), n_atoms=atoms, noisy=noisy)
    if noisy:
        net.set_acting_noise(acting)
    rep = VecReplay(cap, n_envs, prioritized=True, n_step=N_STEP, gamma=gamma)
    rep.set_per_mode(per_mode)
    rep.seed(3, "numpy")
    net.init_params(5, which=0); net.init_params(6, which=1)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return dict(step=VecStep(env, rep, net, batch, ALGO, gamma), k=0)


def timed_vec(p, k):
    step = p["step"]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(k):
        step(0.0, seed=2, step=p["k"] + i, train=True)
    torch.cuda.synchronize()
    p["k"] += k
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,1024,4096")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="comma-separated subset of " + ", ".join(CONFIGS))
    ap.add_argument("--atoms", type=int, default=51)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--per-mode", default="exact", choices=("exact", "fast"))
    ap.add_argument("--out", default="profiles/c51_noisy_time.txt", help="also append the rows to this file ('' = stdout only)")
    a = ap.parse_args()
    configs = {name: CONFIGS[name] for name in a.configs.split(",")}
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/time_c51_noisy.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit(f"# {ALGO} on the {ARCH} head, n = {N_STEP}, B = 32, prioritized/{a.per_mode}, epsilon 0")
        emit("#  what          envs  config          median_us   min_us   max_us")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {name: pipeline(n_envs, noisy, acting, a.atoms, a.capacity, a.per_mode) for name, (noisy, acting) in configs.items()}
            for p in pipes.values():
                for i in range(a.warmup):
                    p["step"](0.0, seed=2, step=p["k"], train=i >= 4)
                    p["k"] += 1
            res = {name: [] for name in configs}
            for _ in range(a.repeats):
                for name in configs:
                    res[name].append(timed_vec(pipes[name], a.steps))
            for name, v in res.items():
                emit(f"  fb_vec_step  {n_envs:5d}  {name:14s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
            del pipes
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
