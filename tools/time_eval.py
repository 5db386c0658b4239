"""Measure on-device evaluation (fb_eval_run).

  python tools/time_eval.py [--reps 5] [--quick]

1. all-live eval step time at 256 / 1024 / 4096 / 8192 envs (episodes = 64, so no env finishes inside the timed steps: every row is
   live), next to fb_vec_step(train=0) on one stream at the same N, both in this process; median and spread over --reps runs;
2. eval env-steps/s of those runs;
3. the heavy-tail run: a VecBrain (1024 envs, nature, lr 1e-5, 500 k-slot replay) trained for --train-steps vector steps
   (one train step each: profiles/r04_learning.txt has this configuration past a mean score of 100 at ~1.05 M), saved, its online net
   evaluated at 4096 envs x 1 episode capped at 100 000 steps: wall time, score distribution, acting rows launched / live rows,
   and the composed act_nib + frame_step Python loop over the same 4096 envs (same records) for comparison.
--quick: section 1 at 1024 envs only, no heavy-tail run (the kernel-statistics run under rocprofv3 uses it).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dqnflappybird_amd import _lib as L  # noqa: E402
from dqnflappybird_amd.evaluate import Evaluator, evaluate, qnet_from_checkpoint  # noqa: E402
from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay, VecStep  # noqa: E402


def vec_step_us(n, steps, net):
    env, replay = VecGameState(n, seed=1), VecReplay(max(4 * n * 8, 50_000), n)
    env.track_state()
    env.observe()
    replay.reset(env.frame_bits)
    st = VecStep(env, replay, net, 32, "dqn", 0.99)
    for i in range(8):
        st(0.0, seed=0, step=i, train=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        st(0.0, seed=0, step=8 + i, train=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def eval_step_us(n, steps, net, ev):
    ev.run(net, n, episodes=64, max_steps=32)                 # warm-up
    r = ev.run(net, n, episodes=64, max_steps=steps)
    assert r.truncated_count == n, "an env finished inside the timed steps: the rows were not all live"
    return r.wall_s / steps * 1e6, r.env_steps / r.wall_s


def composed_loop(net, n, max_steps, env_seed=0):
    env = VecGameState(n, seed=env_seed)
    nib = env.track_state()
    env.observe()
    done = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 0
    while steps < max_steps:
        a = net.act_nib(nib, 0.0)
        _, _, term, _ = env.frame_step(a, want_u8=False)
        done |= term.bool()
        steps += 1
        if steps % 32 == 0 and bool(done.all()):            # (the same one-sync-per-32-steps budget as fb_eval_run)
            break
    torch.cuda.synchronize()
    return time.perf_counter() - t0, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--train-steps", type=int, default=1_200_000)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    L.require_gpu()
    torch.cuda.set_device(0)
    print(f"# device {torch.cuda.get_device_name(0)}; eval chunk = 32 vector steps per live-count read", flush=True)
    Ns = [1024] if a.quick else [256, 1024, 4096, 8192]
    print("# 1-2. all-live step: fb_eval_run (trunk + fc1 + eval step per vector step, one sync per 32) vs fb_vec_step(train=0), "
          f"{a.steps} steps, median [min, max] of {a.reps} runs", flush=True)
    for n in Ns:
        net = QNet(2, 512, "plain", max_batch=(n + 2) // 3)
        net.init_params(seed=0)
        ev = Evaluator(n)
        e_us, v_us, rate = [], [], []
        for _ in range(a.reps):
            t, r = eval_step_us(n, a.steps, net, ev)
            e_us.append(t); rate.append(r)
            v_us.append(vec_step_us(n, a.steps, net))
        f = lambda x: f"{np.median(x):8.1f} [{min(x):.1f}, {max(x):.1f}]"
        print(f"N {n:5d}  eval_step_us {f(e_us)}  vec_step_train0_us {f(v_us)}  eval_env_steps_per_s {np.median(rate):.4g}", flush=True)
    if a.quick:
        return
    print(f"# 3. heavy tail: VecBrain(1024, nature, lr 1e-5) trained {a.train_steps} vector steps "
          f"(one train step each, {a.train_steps * 1024 / 1e9:.2f} G env-steps), then 4096 envs x 1 episode, cap 100000 steps", flush=True)
    from dqnflappybird_amd.vecbrain import VecBrain
    b = VecBrain(1024, algo="nature", observe=1000, capacity=500_000)
    b.net.set_hparams(lr=1e-5)
    t0 = time.perf_counter()
    b.run(a.train_steps, log_every=0)
    torch.cuda.synchronize()
    print(f"train wall_s {time.perf_counter() - t0:.2f}  training-env episodes {int(b.stats[0])} mean score "
          f"{int(b.stats[1]) / max(int(b.stats[0]), 1):.3f}", flush=True)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "ckpt.npz")
        b.save(path)
        net = qnet_from_checkpoint(path, max_batch=1366)      # (the composed loop's act_nib takes all 4096 envs in one call)
    walls = []
    for i in range(a.reps):
        r = evaluate(net, 4096, 1, max_steps=100_000)
        walls.append(r.wall_s)
    print(r.summary())
    print(f"eval wall_s median {np.median(walls):.3f} [{min(walls):.3f}, {max(walls):.3f}] over {a.reps} runs; "
          f"rows launched / live rows {r.rows_per_live_row:.3f} ({r.rows_launched} / {r.env_steps}); compactions {r.compactions}")
    q = np.percentile(r.score, [0, 10, 25, 50, 75, 90, 99, 100])
    print("score quantiles 0/10/25/50/75/90/99/100: " + " ".join(f"{v:.0f}" for v in q))
    print("length quantiles 0/50/90/99/100: " + " ".join(f"{v:.0f}" for v in np.percentile(r.length, [0, 50, 90, 99, 100])))
    cw, cs = composed_loop(net, 4096, r.steps + 32)
    print(f"composed act_nib + frame_step loop over the same 4096 envs: wall_s {cw:.3f} for {cs} vector steps "
          f"(eval: {np.median(walls):.3f} s, {r.steps} steps): ratio {cw / np.median(walls):.2f}", flush=True)


if __name__ == "__main__":
    main()
