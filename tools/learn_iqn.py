"""Does the IQN loop LEARN?  One seeded VecIQN run: the windowed score and the loss, then a greedy evaluate() on fresh games.  One seed
says that the loop runs and learns, not how well.  The QR run to set beside it is tools/learn_curve.py --algo qr at the same envs, lr,
steps and seed.

    python tools/learn_iqn.py [--envs 1024] [--lr 1e-5] [--steps 2000000] [--window 50000] [--explore 1000000] [--n-step 1] [--double]
                              [--per] [--dueling] [--munchausen [--temp 0.03] [--alpha 0.9] [--clip -1]] [--cvar 1.0] [--eval-envs 4096]
                              [--sigma0 S [--acting-noise shared|env]]
                              [--seed 1] [--budget-s S] [--out FILE]

Every `window` steps the device stats buffer (episodes ended, score sum, score max, pipes passed: kept by the env kernel) is read and
zeroed, so each row is the window's own figure.  Rows go to stdout, and are appended to --out when one is given.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from dqnflappybird_amd.veciqn import VecIQN  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--steps", type=int, default=2_000_000)
    ap.add_argument("--window", type=int, default=50_000)
    ap.add_argument("--explore", type=int, default=1_000_000)
    ap.add_argument("--n-step", type=int, default=1)
    ap.add_argument("--double", action="store_true")
    ap.add_argument("--per", action="store_true", help="train from a prioritized memory (VecIQN(prioritized=True))")
    ap.add_argument("--dueling", action="store_true", help="the dueling IQN net (VecIQN(dueling=True))")
    ap.add_argument("--munchausen", action="store_true", help="the Munchausen target (VecIQN(munchausen=True)); not with --double")
    ap.add_argument("--temp", type=float, default=0.03, help="--munchausen: the softmax temperature")
    ap.add_argument("--alpha", type=float, default=0.9, help="--munchausen: the scale of the log-policy bonus")
    ap.add_argument("--clip", type=float, default=-1.0, help="--munchausen: the bonus's lower clip l0")
    ap.add_argument("--cvar", type=float, default=1.0)
    ap.add_argument("--sigma0", type=float, default=None, help="noisy fc1 and head layers at this sigma0 (VecIQN(noisy=True)): epsilon 0")
    ap.add_argument("--acting-noise", choices=("shared", "env"), default="shared", help="--sigma0: one acting sample for all envs, or one per env")
    ap.add_argument("--eval-envs", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--budget-s", type=float, default=0.0, help="stop the run after this many seconds (0 = run all its steps)")
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        emit(f"# tools/learn_iqn.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        v = VecIQN(a.envs, lr=a.lr, seed=a.seed, explore=a.explore, n_step=a.n_step, double_q=a.double, cvar=a.cvar, capacity=1_000_000,
                   prioritized=a.per, dueling=a.dueling, munchausen=a.munchausen, temp=a.temp, alpha=a.alpha, clip=a.clip,
                   **(dict(noisy=True, sigma0=a.sigma0, acting_noise=a.acting_noise) if a.sigma0 is not None else {}))
        emit(f"# envs {a.envs}  batch {v.batch}  (N, N', K) ({v.n_tau}, {v.n_tau_next}, {v.n_tau_act})  kappa {v.kappa:g}  cvar {v.cvar:g}  "
             f"double_q {v.double_q}  prioritized {v.prioritized}  dueling {v.dueling}  n_step {v.n_step}  observe {v.observe}  lr {v.lr:g}  seed {a.seed}"
             + (f"  munchausen (temp, alpha, clip) ({v.temp:g}, {v.alpha:g}, {v.clip:g})" if v.munchausen else "")
             + (f"  noisy sigma0 {v.sigma0:g} acting_noise {v.acting_noise}" if v.noisy else ""))
        emit("#   env_steps  train_steps  episodes  mean_score  max_score  pipes/episode       loss   epsilon   steps/s")
        t0 = t_run = time.time()
        v.stats.zero_()
        for k in range(1, a.steps + 1):
            loss = v.step()
            if k % a.window == 0 or k == a.steps:
                ep, ssum, smax, pipes = v.stats.tolist()
                v.stats.zero_()
                v.net.check_range()
                now = time.time()
                emit(f"  {k * a.envs:11d} {max(0, k - v.observe - 1):12d} {ep:9d} {ssum / max(ep, 1):11.3f} {smax:10d} {pipes / max(ep, 1):14.3f} "
                     f"{loss.item():10.4g} {v.epsilon:9.5f} {a.window / (now - t0):9.0f}")
                t0 = now
                if a.budget_s and now - t_run > a.budget_s:
                    emit(f"# stopped after {k} steps: the time budget of {a.budget_s:g} s is spent")
                    break
        if a.eval_envs:
            res = v.evaluate(n_envs=a.eval_envs, episodes=1)
            emit(f"# greedy evaluate() on {a.eval_envs} fresh games: mean score {res.score.mean():.3f}, median {float(np.median(res.score)):.1f}, "
                 f"max {int(res.score.max())}, mean length {res.length.mean():.1f}")
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
