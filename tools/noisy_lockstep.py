"""How much the envs of a noisy net act in lockstep: on a fresh VecBrain (rainbow: c51doubleper on the dueling C51 head, n = 3, noisy),
per vector step the fraction of envs that flap and the spread across envs of Q(flap) - Q(noop) as the step acts on it, for the shared
acting noise (one sample per step for all envs) and the per-env one.

    python tools/noisy_lockstep.py [--envs 1024] [--steps 200] [--seed 1] [--modes shared,env] [--out FILE]

The Q values are the acting forward's own: before each step the same call fb_vec_step makes (act_nib after the step's reset_noise(0),
or act_nib_env_noise), and its actions are checked against the step's.  The first steps of a fresh brain do not train (observe 1000),
so they show the initial net's behaviour.  Rows go to stdout and are appended to --out (profiles/c51_noisy_env_lockstep.txt unless
another file, or '', is given).
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vecbrain import VecBrain  # noqa: E402


def measure(mode, n_envs, steps, seed):
    vb = VecBrain(n_envs, algo="c51doubleper", arch="c51dueling", capacity=1_000_000, seed=seed, n_step=3, noisy=True, acting_noise=mode)
    flap, spread, mean = [], [], []
    for _ in range(steps):
        key = vb.seed + vb.rank
        if mode == "env":
            a, q = vb.net.act_nib_env_noise(vb.nib, vb.epsilon, seed=key, step=vb.timeStep, want_q=True)
        else:
            vb.net.reset_noise(0, key, vb.timeStep)          # (fb_vec_step draws the same sample first)
            a, q = vb.net.act_nib(vb.nib, vb.epsilon, seed=key, step=vb.timeStep, want_q=True)
        a, d = a.clone(), (q[:, 1] - q[:, 0]).double()
        vb.step()
        assert torch.equal(a, vb.one_step.actions), "the measured forward is not the step's"
        flap.append(a.double().mean().item())
        spread.append(d.std().item())
        mean.append(d.mean().item())
    del vb
    torch.cuda.synchronize()
    return flap, spread, mean


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--modes", default="shared,env")
    ap.add_argument("--out", default="profiles/c51_noisy_env_lockstep.txt", help="also append the rows to this file ('' = stdout only)")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/noisy_lockstep.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit(f"# fresh VecBrain, rainbow + noisy (sigma0 0.5), {a.envs} envs, seed {a.seed}, its first {a.steps} steps; d = Q(flap) - Q(noop) per env")
        for mode in a.modes.split(","):
            flap, spread, mean = measure(mode, a.envs, a.steps, a.seed)
            lock = sum(1 for f in flap if f in (0.0, 1.0))
            near = sum(1 for f in flap if f <= 0.05 or f >= 0.95)
            emit(f"  acting noise {mode:6s}: flap fraction over all steps {statistics.mean(flap):.3f}; steps where every env took the same action "
                 f"{lock} / {len(flap)}, >= 95 % the same {near} / {len(flap)}")
            emit(f"  acting noise {mode:6s}: spread of d across the envs of a step (std): median {statistics.median(spread):.4f}, "
                 f"range {min(spread):.4f} - {max(spread):.4f}; mean of d over the envs: std over the steps {statistics.pstdev(mean):.4f}")
            emit(f"  acting noise {mode:6s}: flap fraction of the first 12 steps " + " ".join(f"{f:.2f}" for f in flap[:12]))


if __name__ == "__main__":
    main()
