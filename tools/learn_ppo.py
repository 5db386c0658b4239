"""Does the vectorised PPO learn this game?  One seeded VecActorCritic(algo="ppo") run: the windowed mean score, then evaluate() on fresh
greedy games.  tools/learn_a2c.py with PPO's options; its rows carry env_steps, so the two curves compare per env step.

    python tools/learn_ppo.py [--envs 1024] [--rollout 5] [--updates 30000] [--window 1000] [--lr 1e-4] [--gamma 0.99] [--gae-lambda 0.95]
                              [--value-coef 0.5] [--entropy-coef 0.01] [--max-grad-norm 0] [--epochs 4] [--minibatches 4] [--clip-eps 0.2]
                              [--value-clip 0] [--no-adv-norm] [--adv-norm-scope minibatch] [--target-kl X] [--anneal-lr] [--seed 1] [--budget-s S] [--eval-envs 4096] [--eval-max-steps 100000] [--out FILE]

Every `window` updates the device stats buffer (episodes ended, score sum, score max, pipes passed: kept by the env kernel) is read and
zeroed, so each row is the window's own figure.  Rows go to stdout and to --out as they are produced.  Reported, not gated: nothing here
sets a target score, and no test reads these figures.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vecac import VecActorCritic  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--rollout", type=int, default=5)
    ap.add_argument("--updates", type=int, default=30000)
    ap.add_argument("--window", type=int, default=1000)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    ap.add_argument("--value-coef", type=float, default=0.5)
    ap.add_argument("--entropy-coef", type=float, default=0.01)
    ap.add_argument("--max-grad-norm", type=float, default=0.0)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--clip-eps", type=float, default=0.2)
    ap.add_argument("--value-clip", type=float, default=0.0)
    ap.add_argument("--no-adv-norm", action="store_true")
    ap.add_argument("--adv-norm-scope", default="rollout", help="rollout | minibatch")
    ap.add_argument("--target-kl", type=float, default=None, help="stop an update's epochs above 1.5 X of mean approximate KL (default: off)")
    ap.add_argument("--anneal-lr", action="store_true", help="the learning rate falls linearly to 0 over --updates")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--budget-s", type=float, default=0.0, help="stop after this many seconds of training (0 = run all updates)")
    ap.add_argument("--eval-envs", type=int, default=4096)
    ap.add_argument("--eval-max-steps", type=int, default=100_000, help="evaluate(): vector steps after which running games are truncated")
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        ac = VecActorCritic(a.envs, rollout=a.rollout, gamma=a.gamma, gae_lambda=a.gae_lambda, value_coef=a.value_coef, entropy_coef=a.entropy_coef,
                            max_grad_norm=a.max_grad_norm, seed=a.seed, lr=a.lr, algo="ppo", epochs=a.epochs, minibatches=a.minibatches,
                            clip_eps=a.clip_eps, value_clip=a.value_clip, normalize_adv=not a.no_adv_norm, adv_norm_scope=a.adv_norm_scope,
                            target_kl=a.target_kl, anneal_lr=a.anneal_lr, total_updates=a.updates if a.anneal_lr else None)
        emit(f"# tools/learn_ppo.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit(f"# envs {ac.n}  rollout {ac.T}  samples/update {ac.n * ac.T}  lr {ac.lr:g}  gamma {ac.gamma:g}  lambda {ac.gae_lambda:g}  value_coef {ac.value_coef:g}  "
             f"entropy_coef {ac.entropy_coef:g}  max_grad_norm {ac.max_grad_norm:g}  seed {ac.seed}  rewards 0.1 / 3 / -3 (the reference's)")
        emit(f"# ppo: epochs {ac.epochs}  minibatches {ac.minibatches} (of {ac.n * ac.T // ac.minibatches})  clip_eps {ac.clip_eps:g}  value_clip {ac.value_clip:g}  "
             f"normalize_adv {ac.normalize_adv}  ({ac.epochs * ac.minibatches} Adam steps per update)")
        emit(f"# ppo options: adv_norm_scope {ac.adv_norm_scope}  target_kl {ac.target_kl:g}  anneal_lr {ac.anneal_lr} (over {ac.total_updates})  one_call {ac.one_call}")
        emit("#     updates   env_steps  episodes  mean_score  max_score  pipes/episode  policy_loss  value_loss   entropy  clip_frac  approx_kl  env_steps/s  epochs/update")
        t0 = t_win = time.perf_counter()
        scores, done = [], 0
        while done < a.updates:
            k = min(a.window, a.updates - done)
            epochs_run = 0
            for _ in range(k):
                losses = ac.update()
                epochs_run += ac.epochs_run
            done += k
            tot, lpi, lv, ent, cf, kl = losses.tolist()              # (synchronises; the last update's last epoch)
            ep, ssum, smax, pipes = ac.stats.tolist()
            ac.stats.zero_()
            ac.net.check_range()
            now = time.perf_counter()
            scores.append(ssum / max(ep, 1))
            emit(f"  {done:10d} {done * ac.T * ac.n:11d} {ep:9d} {scores[-1]:11.3f} {smax:10d} {pipes / max(ep, 1):14.3f} {lpi:12.4g} {lv:11.4g} {ent:9.4f} {cf:10.4f} {kl:10.3g} "
                 f"{k * ac.T * ac.n / (now - t_win):12.0f} {epochs_run / k:14.3f}")
            t_win = now
            if a.budget_s and now - t0 > a.budget_s:
                emit(f"# stopped after {now - t0:.0f} s (--budget-s {a.budget_s:g}) at {done} of {a.updates} updates")
                break
        emit(f"# summary: mean score first window {scores[0]:.3f}, best window {max(scores):.3f}, last window {scores[-1]:.3f}")
        swings = [abs(b - x) for x, b in zip(scores, scores[1:])]
        if swings:
            drops = [(x - b) / x for x, b in zip(scores, scores[1:]) if b < x]
            emit(f"# window-to-window swing |score[i+1] - score[i]|: mean {sum(swings) / len(swings):.3f}, max {max(swings):.3f} over {len(swings)} steps; "
                 f"{len(drops)} of them fall, by {max(drops, default=0.0):.1%} of the earlier window at most")
        if a.eval_envs > 0:
            res = ac.evaluate(n_envs=a.eval_envs, episodes=1, max_steps=a.eval_max_steps)
            emit(f"# evaluate() on {a.eval_envs} games, argmax of the policy: {res.summary()}")


if __name__ == "__main__":
    main()
