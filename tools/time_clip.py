"""What gradient clipping and soft target updates cost: µs per fb_vec_step of 'double' (uniform memory; the split schedule where it
applies) and 'doubleper' (prioritized memory) on the dueling 512 / 2 head with B = 32, in four settings each: off, the norm limit on, soft
target updates on (one fb_qnet_soft_sync_target behind every step), and both.

    python tools/time_clip.py [--envs 256,1024,4096] [--steps 300] [--warmup 300] [--repeats 5] [--max-grad-norm 10] [--polyak 0.005] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.

One pipeline at a time: each round builds a fresh pipeline per setting -- VecStep with a 1 M-slot memory -- warms it up, times --steps steps
and drops it, the four settings following each other within a round and the rounds repeating the sequence (off, clip, polyak, both, off,
...), so that drift shows in every setting alike.  Not several pipelines alive at once, as tools/time_huber.py has them: a prioritized
memory keeps a side stream of its own, and with two or more of them in one process one pipeline -- any of them, 'off' included -- ran
~500 µs per step slower (two of the process's streams on one hardware queue; what csrc/fb_common.hip's fb_streams_concurrent is
about).  A training process has one pipeline.  Reported: the median and the spread of the rounds' µs per step; the 'off' rows are the
yardstick.  A clipped step is the exporting step + two clip launches + fb_qnet_apply_adam's launch on one stream: it gives up the fused
chain's in-launch Adam and, for 'double', the split schedule (the split_stats lines say how many steps took it); the last clip's (norm,
scale) is printed so that a limit that never acts is seen as such.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402

ALGOS = {"double": False, "doubleper": True}              # algo -> prioritized memory
SETTINGS = ("off", "clip", "polyak", "clip+polyak")


def pipeline(n_envs, algo, setting, cap, G, rho, batch=32, gamma=0.99):
    per = ALGOS[algo]
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, "dueling", max_batch=max(n_envs, batch))
    rep = VecReplay(cap, n_envs, prioritized=per)
    rep.seed(3, "numpy" if per else "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    if "clip" in setting:
        net.set_max_grad_norm(G)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    return dict(net=net, rep=rep, step=VecStep(env, rep, net, batch, algo, gamma), k=0, rho=rho if "polyak" in setting else 0.0)


def one(p, train=True):
    p["step"](0.01, seed=2, step=p["k"], train=train)
    if train and p["rho"]:
        p["net"].soft_sync_target(p["rho"])
    p["k"] += 1


def timed_vec(p, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        one(p)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,1024,4096")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--max-grad-norm", type=float, default=10.0)
    ap.add_argument("--polyak", type=float, default=0.005)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/time_clip.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}  (max_grad_norm {a.max_grad_norm:g}, polyak {a.polyak:g})")
        emit("#  what          envs  algo       setting        median_us   min_us   max_us")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            for algo in ALGOS:
                res, notes = {s: [] for s in SETTINGS}, {}
                for _ in range(a.repeats):
                    for s in SETTINGS:
                        p = pipeline(n_envs, algo, s, a.capacity, a.max_grad_norm, a.polyak)
                        for i in range(a.warmup):
                            one(p, train=i >= 4)
                        res[s].append(timed_vec(p, a.steps))
                        issued, clean = p["net"].split_stats()
                        norm, scale = p["net"].grad_norm()
                        notes[s] = (f"#   {algo} {s}: split schedule on {issued} of {p['k']} steps ({clean} minibatches beside their env step); "
                                    f"last clip: norm {norm:.4g}, scale {scale:.4g}")
                        del p
                        torch.cuda.synchronize()
                for s, v in res.items():
                    emit(f"  fb_vec_step  {n_envs:5d}  {algo:9s}  {s:12s} {statistics.median(v):10.1f} {min(v):8.1f} {max(v):8.1f}")
                for s in SETTINGS:
                    emit(notes[s])


if __name__ == "__main__":
    main()
