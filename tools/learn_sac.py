"""Does the SAC loop LEARN?  One seeded VecSAC run per setting: the windowed score, the policy's entropy and the temperature, then a
greedy evaluate() on fresh games.  One seed says that the loop runs and learns, not how well.

    python tools/learn_sac.py [--envs 1024] [--steps 60000] [--window 5000] [--alpha-lrs 0,1e-4] [--eval-envs 4096] [--seed 0] [--out FILE]
                              [--budget-s S  (stop a run after S seconds of wall time)] [--per] [--n-step K] [--lrs 1e-4]

Every `window` steps the device stats buffer (episodes ended, score sum, score max, pipes passed: kept by the env kernel) is read and
zeroed, so each row is the window's own figure.  Rows go to stdout, and are appended to --out when one is given.
--per: a prioritized memory (VecSAC(prioritized=True)); --n-step K with it: K-step returns.  --lrs: Adam's learning rates, one run per
(lr, alpha_lr) pair.  A run's last row reports, over 256 live env states, the mean gap between the two actions' min(Q1, Q2) and
between their logits, beside alpha: whether the actions' values differ by more than the temperature.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vecsac import VecSAC  # noqa: E402


def q_gap(sac, rows=256):
    """mean |min(Q1, Q2)(s, 1) - min(Q1, Q2)(s, 0)| and mean |z_1 - z_0| over the newest states of the first `rows` envs"""
    s = sac.replay.current_state()[:rows].contiguous()
    z, q1, q2 = sac.net.forward_sac(s)
    q = torch.minimum(q1, q2)
    return (q[:, 1] - q[:, 0]).abs().mean().item(), (z[:, 1] - z[:, 0]).abs().mean().item()


def run(n_envs, steps, window, alpha_lr, seed, eval_envs, budget_s, emit, per=False, n_step=1, lr=1e-4):
    sac = VecSAC(n_envs, alpha_lr=alpha_lr, seed=seed, lr=lr, prioritized=per, n_step=n_step)
    emit(f"# envs {n_envs}  batch {sac.batch}  alpha {sac.alpha:g}  target_entropy {sac.target_entropy:g}  alpha_lr {sac.alpha_lr:g}  "
         f"polyak {sac.polyak:g}  observe {sac.observe}  lr {sac.lr:g}  seed {seed}  memory {'prioritized' if per else 'uniform'}  n_step {n_step}")
    emit("#   env_steps  episodes  mean_score  max_score  pipes/episode    q_loss  policy_loss   entropy     alpha   steps/s")
    t0 = t_run = time.time()
    sac.stats.zero_()
    for k in range(1, steps + 1):
        losses = sac.step()
        if k % window == 0 or k == steps:
            tot, q1, q2, lpi, ent, alpha = losses.tolist()
            ep, ssum, smax, pipes = sac.stats.tolist()
            sac.stats.zero_()
            sac.net.check_range()
            now = time.time()
            emit(f"  {k * n_envs:11d} {ep:9d} {ssum / max(ep, 1):11.3f} {smax:10d} {pipes / max(ep, 1):14.3f} {q1 + q2:9.4g} {lpi:12.4g} "
                 f"{ent:9.4f} {alpha:9.5f} {window / (now - t0):9.0f}")
            t0 = now
            if budget_s and now - t_run > budget_s:
                emit(f"# stopped after {k} steps: the time budget of {budget_s:g} s is spent")
                break
    gap, zgap = q_gap(sac, min(256, n_envs))
    emit(f"# at the end, over {min(256, n_envs)} live states: mean |min Q(s, 1) - min Q(s, 0)| {gap:.5g}, mean |z_1 - z_0| {zgap:.5g}, alpha {sac.net.sac()[0]:.5g}")
    if eval_envs:
        res = sac.evaluate(n_envs=eval_envs, episodes=1)
        emit(f"# greedy evaluate() on {eval_envs} fresh games: mean score {res.score.mean():.3f}, median {float(__import__('numpy').median(res.score)):.1f}, "
             f"max {int(res.score.max())}, mean length {res.length.mean():.1f}")
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=60000)
    ap.add_argument("--window", type=int, default=5000)
    ap.add_argument("--alpha-lrs", default="0,1e-4")
    ap.add_argument("--eval-envs", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--budget-s", type=float, default=0.0)
    ap.add_argument("--per", action="store_true", help="train from a prioritized memory")
    ap.add_argument("--n-step", type=int, default=1, help="--per: learn from K-step returns")
    ap.add_argument("--lrs", default="1e-4", help="Adam's learning rates, comma separated")
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        emit(f"# tools/learn_sac.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        for lr in [float(x) for x in a.lrs.split(",")]:
            for alr in [float(x) for x in a.alpha_lrs.split(",")]:
                run(a.envs, a.steps, a.window, alr, a.seed, a.eval_envs, a.budget_s, emit, a.per, a.n_step, lr)


if __name__ == "__main__":
    main()
