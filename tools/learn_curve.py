"""Does the vectorised loop LEARN?  

Every kernel of the loop is parity-checked against the oracle; what kernel-level parity cannot see is the plumbing between them in the
vectorised form -- reward / terminal routing through the replay ring, the target-sync timing, the epsilon schedule, the frame stack
across episode ends.  A score curve can.  The reference's own evidence is logs_bird/eval_images/mean.png (mean episode score 60 .. 135 after
2 - 4 M single-env steps, BrainDQNNature.py:149-197); no target score is set here, only "clearly above the untrained policy's".

    python tools/learn_curve.py [--envs 16,1024] [--lrs 1e-6,1e-5] [--steps 2000000] [--window 50000] [--algo nature] [--out FILE]
                                [--n-step K] [--eval-envs 4096] [--algo c51|c51double|c51per|c51doubleper --atoms 51 --vmin -10 --vmax 10]
                                [--algo qr|qrdouble|qrper|qrdoubleper --quantiles 51 --kappa 1]
                                [--algo mdqn|mdqnper --tau 0.03 --alpha 0.9 --clip -1]
                                [--algo doubleper] [--huber D  (any scalar algo: the Huber loss's delta)]
                                [--max-grad-norm G  (clip the gradient's global norm; the rows then carry the last step's norm and scale)]
                                [--polyak RHO  (soft target updates after every train step, no periodic copy)]
                                [--priority-init td  (--algo per | doubleper: new leaves at their acting-time |TD error|, not the tree's maximum)]

One VecBrain run per (envs, lr); one train step per loop step once onlineTimeStep > OBSERVE, as in the reference.  Every `window`
steps the device stats buffer (episodes ended, score sum, score max, pipes passed: kept by the env kernel) is read and zeroed, so each
row is the window's own figure, not a running average.  Rows go to stdout and to --out as they are produced.
--n-step K trains from K-step returns (VecBrain(n_step=K); with --algo per / c51per / c51doubleper a prioritized memory created with K-step returns); the summary gives the train steps at which the windowed mean score first
passed 1 / 10 / 100, and --eval-envs M (> 0) ends each run with VecBrain.evaluate() on M fresh greedy games.  --noisy gives a C51 algo's
net noisy layers (epsilon 0 unless --initial-epsilon says otherwise), and --acting-noise env makes such a net act with independent noise per env.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vecbrain import VecBrain  # noqa: E402


def run(n_envs, lr, steps, window, algo, arch, seed, out, budget_s, explore, n_step=1, eval_envs=0, support=(51, -10.0, 10.0), noisy=False,
        initial_epsilon=None, acting_noise="shared", quantiles=(51, 1.0), munchausen=(0.03, 0.9, -1.0), huber=0.0, max_grad_norm=0.0,
        polyak=0.0, priority_init="max"):
    vb = VecBrain(n_envs, algo=algo, arch=arch, capacity=1_000_000, seed=seed, explore=explore, n_step=n_step,
                  n_atoms=support[0], v_min=support[1], v_max=support[2], noisy=noisy, initial_epsilon=initial_epsilon,
                  acting_noise=acting_noise, n_quantiles=quantiles[0], kappa=quantiles[1], tau=munchausen[0], alpha=munchausen[1],
                  clip=munchausen[2], huber=huber, max_grad_norm=max_grad_norm, polyak=polyak, priority_init=priority_init)
    vb.net.set_hparams(lr=lr)
    head = f"# envs {n_envs}  algo {algo}/{arch}  n_step {n_step}  lr {lr:g}  batch {vb.batch}  observe {vb.observe}  explore {vb.explore}  eps {vb.initial_epsilon} -> {vb.final_epsilon}  {f'soft target updates, rho {vb.polyak:g}' if vb.polyak else 'target never synced (PER: the reference agent never syncs it)' if algo == 'per' else f'target sync / {vb.replace_target_iter}'}"
    if vb.support:
        head += f"  support {vb.support[0]} atoms on [{vb.support[1]:g}, {vb.support[2]:g}]"
    if vb.quantiles:
        head += f"  {vb.quantiles[0]} quantiles, kappa {vb.quantiles[1]:g}"
    if vb.munchausen:
        head += f"  munchausen tau {vb.munchausen[0]:g} alpha {vb.munchausen[1]:g} clip {vb.munchausen[2]:g}"
    if vb.huber:
        head += f"  huber delta {vb.huber:g}"
    if vb.max_grad_norm:
        head += f"  max_grad_norm {vb.max_grad_norm:g}"
    if vb.priority_init != "max":
        head += f"  priority_init {vb.priority_init} (fast tree)"
    if vb.noisy:
        head += f"  noisy (sigma0 {vb.sigma0:g}, acting noise {vb.acting_noise})"
    cols = "#   train_steps   env_steps  epsilon  episodes  mean_score  max_score  pipes/episode      loss   steps/s"
    if vb.max_grad_norm:
        cols += "  grad_norm  clip_scale"
    for f in (sys.stdout, out):
        print(head, file=f); print(cols, file=f); f.flush()
    t_run = time.perf_counter()
    done = 0
    rows = []
    while done < steps:
        n = min(window, steps - done)
        t0 = time.perf_counter()
        vb.run(n, log_every=0)
        ep, ssum, smax, pipes = vb.stats.tolist()            # (the host sync of the window)
        dt = time.perf_counter() - t0
        vb.stats.zero_()
        done += n
        loss = vb.last_loss.item() if vb.last_loss is not None else float("nan")
        trained = max(0, vb.onlineTimeStep - vb.observe - 1)
        row = (trained, done * n_envs, vb.epsilon, ep, ssum / max(ep, 1), smax, pipes / max(ep, 1), loss, n / dt)
        rows.append(row)
        line = f"  {row[0]:13d} {row[1]:11d}  {row[2]:7.5f} {row[3]:9d}  {row[4]:10.3f} {row[5]:10d}  {row[6]:13.3f} {row[7]:9.4g} {row[8]:9.0f}"
        if vb.max_grad_norm:                                 # (the window's last train step; synchronous, once per window)
            gn, gc = vb.net.grad_norm()
            line += f" {gn:10.4g}  {gc:10.4g}"
        for f in (sys.stdout, out):
            print(line, file=f); f.flush()
        if budget_s and time.perf_counter() - t_run > budget_s:
            for f in (sys.stdout, out):
                print(f"# stopped at the time budget of {budget_s} s", file=f); f.flush()
            break
    assert vb.env.error_count() == 0
    issued, clean = vb.net.split_stats() if hasattr(vb.net, "split_stats") else (0, 0)      # (raises if a wait between the two streams of the split schedule gave up)
    first = rows[0][4]
    best = max(r[4] for r in rows)
    last = sum(r[4] for r in rows[-3:]) / len(rows[-3:])
    passed = {lvl: next((r[0] for r in rows if r[4] > lvl), None) for lvl in (1, 10, 100)}
    cross = ", ".join(f"> {lvl}: {'never' if v is None else v}" for lvl, v in passed.items())
    for f in (sys.stdout, out):
        print(f"# summary envs {n_envs} n_step {n_step} lr {lr:g}: mean score first window {first:.3f}, best window {best:.3f}, last three windows {last:.3f}, max score of the run {max(r[5] for r in rows)}; split schedule: {issued} steps, {clean} minibatches beside their env step", file=f)
        print(f"# windowed mean score first passed (train steps): {cross}", file=f)
        f.flush()
    if eval_envs:
        res = vb.evaluate(n_envs=eval_envs)
        for f in (sys.stdout, out):
            print(f"# evaluate() on {eval_envs} games: mean {res.mean_score:.3f} median {res.median_score:.1f} max {res.max_score}  ({res.summary()})", file=f)
            f.flush()
    for f in (sys.stdout, out):
        print("", file=f)
    del vb
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="16,1024")
    ap.add_argument("--lrs", default="1e-6,1e-5")
    ap.add_argument("--steps", type=int, default=2_000_000)
    ap.add_argument("--window", type=int, default=50_000)
    ap.add_argument("--algo", default="nature")
    ap.add_argument("--arch", default="plain")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--explore", type=int, default=1_000_000)
    ap.add_argument("--n-step", type=int, default=1)
    ap.add_argument("--atoms", type=int, default=51, help="--algo c51 / c51double / c51per / c51doubleper: atoms of the support")
    ap.add_argument("--quantiles", type=int, default=51, help="--algo qr / qrdouble / qrper / qrdoubleper: the number of quantiles")
    ap.add_argument("--kappa", type=float, default=1.0, help="QR algos: the quantile Huber loss's threshold")
    ap.add_argument("--tau", type=float, default=0.03, help="--algo mdqn / mdqnper: the softmax temperature")
    ap.add_argument("--alpha", type=float, default=0.9, help="--algo mdqn / mdqnper: the scale of the log-policy bonus")
    ap.add_argument("--clip", type=float, default=-1.0, help="--algo mdqn / mdqnper: the bonus's lower clip")
    ap.add_argument("--huber", type=float, default=0.0, help="scalar algos: the Huber loss's delta (0 = the squared loss)")
    ap.add_argument("--max-grad-norm", type=float, default=0.0, help="clip the gradient's global norm to this before Adam (0 = no clipping)")
    ap.add_argument("--polyak", type=float, default=0.0, help="soft target updates with this rate after every train step, no periodic copy (0 = off)")
    ap.add_argument("--priority-init", choices=("max", "td"), default="max", help="--algo per / doubleper: a new transition's priority (VecBrain(priority_init=...))")
    ap.add_argument("--vmin", type=float, default=-10.0)
    ap.add_argument("--vmax", type=float, default=10.0)
    ap.add_argument("--eval-envs", type=int, default=0, help="end each run with VecBrain.evaluate() on this many games (0 = no evaluation)")
    ap.add_argument("--budget-s", type=float, default=0.0, help="stop a run after this many seconds (0 = run all its steps)")
    ap.add_argument("--noisy", action="store_true", help="a C51 algo's net with noisy fc1 and head layers (VecBrain(noisy=True))")
    ap.add_argument("--initial-epsilon", type=float, default=None, help="the epsilon schedule's start (default: VecBrain's, 0 when --noisy)")
    ap.add_argument("--acting-noise", choices=("shared", "env"), default="shared", help="--noisy: one noise sample per step for all envs, or per env")
    ap.add_argument("--out", default="gpurun_out/learning.txt")
    a = ap.parse_args()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "a") as out:
        print(f"# tools/learn_curve.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}", file=out)
        for n_envs in [int(x) for x in a.envs.split(",")]:
            for lr in [float(x) for x in a.lrs.split(",")]:
                run(n_envs, lr, a.steps, a.window, a.algo, a.arch, a.seed, out, a.budget_s, a.explore, a.n_step, a.eval_envs, (a.atoms, a.vmin, a.vmax),
                    a.noisy, a.initial_epsilon, a.acting_noise, (a.quantiles, a.kappa), (a.tau, a.alpha, a.clip), a.huber, a.max_grad_norm, a.polyak,
                    a.priority_init)


if __name__ == "__main__":
    main()
