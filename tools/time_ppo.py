"""What PPO costs: µs per 256-sample ring-fed PPO chunk against the A2C chunk (the same trunk and backward; the loss launch differs), µs per
fb_ac_permute and fb_ac_normalize_adv at T N = 5120 and 131 072, and the whole PPO update at 1024 envs x T = 5 with the defaults
(4 epochs x 4 minibatches of 1280 = 80 chunks, 16 Adam steps), then that update chunk by chunk (one_call=False) beside each epoch as one
host call (one_call=True), beside per-minibatch advantage normalisation and beside the per-epoch read of target_kl, the four alternated
within every round in one process.

    python tools/time_ppo.py [--steps 300] [--warmup 50] [--repeats 5] [--parent DIR] [--out FILE]
    python tools/time_ppo.py --chunk-row --root DIR          (what --parent runs: the A2C chunk row alone, on the tree at DIR)

Rows go to stdout, and are appended to --out when one is given.

--parent DIR: a built checkout of the parent commit.  The A2C chunk row of tools/time_a2c.py (vec.ac_train_from_replay at B = 256 with
flat_grad, on a memory 1024 envs filled) is then measured on that tree and on this one in child processes of their own, alternated
P N N P, so that the A2C chunk of this tree can be judged against the parent's own round-to-round spread in the same session.
Reported: the median and the spread of the rounds.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, N, B = 5, 1024, 256


def timed(torch, fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def rollout(vec, torch):
    """an actor-critic net and a memory that holds one rollout of 1024 envs x T = 5 -> (net, replay, the last 256 positions)"""
    env = vec.VecGameState(N, seed=1)
    net = vec.QNet(2, 512, "ac", max_batch=N)
    rep = vec.VecReplay((T + 2) * N, N)
    rep.seed(3, "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    step = vec.AcRolloutStep(env, rep, net, T)
    for k in range(2 * T):
        step(k % T, seed=2, step=k)
    idx = (len(rep) - B + torch.arange(B, dtype=torch.int64)).cuda()
    return net, rep, idx, (env, step)


def chunk_row(a):
    """the A2C chunk row of tools/time_a2c.py on the tree at a.root: one line 'a2c-chunk median min max' (us)"""
    sys.path.insert(0, a.root)
    import torch
    from dqnflappybird_amd import vec
    assert os.path.abspath(vec.__file__).startswith(os.path.abspath(a.root) + os.sep), vec.__file__
    net, rep, idx, keep = rollout(vec, torch)
    adv, ret = torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
    g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
    fn = lambda: vec.ac_train_from_replay(rep, net, idx, adv, ret, n_total=T * N, flat_grad=g)
    for _ in range(a.warmup):
        fn()
    v = [timed(torch, fn, a.steps) for _ in range(a.repeats)]
    print(f"a2c-chunk {statistics.median(v):.2f} {min(v):.2f} {max(v):.2f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its A2C chunk row beside this tree's")
    ap.add_argument("--chunk-row", action="store_true", help="print the A2C chunk row of the tree at --root and exit")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.chunk_row:
        return chunk_row(a)
    sys.path.insert(0, ROOT)
    import torch
    from dqnflappybird_amd import vec
    from dqnflappybird_amd.vecac import VecActorCritic
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        def row(what, n, config, v, unit="us"):
            emit(f"  {what:13s} {n:7d}  {config:30s} {statistics.median(v):10.1f} {min(v):9.1f} {max(v):9.1f}  {unit}")

        emit(f"# tools/time_ppo.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        if a.parent:                              # (child processes first, before this one holds much of the GPU)
            emit("# the A2C chunk (ac_train_from_replay, B = 256, flat_grad), one child process per row, parent and this tree alternated")
            emit("#  tree       median       min       max   us")
            for name, root in (("parent", a.parent), ("this", ROOT), ("this", ROOT), ("parent", a.parent)):
                cmd = [sys.executable, os.path.join(ROOT, "tools", "time_ppo.py"), "--chunk-row", "--root", os.path.abspath(root), "--steps", str(a.steps),
                       "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
                res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=os.path.abspath(root))
                if res.returncode != 0:
                    raise SystemExit(f"{' '.join(cmd)} failed with {res.returncode}:\n{res.stderr[-2000:]}")
                f = [x for x in res.stdout.splitlines() if x.startswith("a2c-chunk")][-1].split()
                emit(f"  {name:8s} {float(f[1]):10.2f} {float(f[2]):9.2f} {float(f[3]):9.2f}")
        emit("#  what             n     config                             median       min       max")
        net, rep, idx, keep = rollout(vec, torch)
        adv, ret = torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
        lpo, vo = torch.full((B,), -0.69, device="cuda") + 0.05 * torch.randn(B, device="cuda"), ret + 0.3 * torch.randn(B, device="cuda")
        sel = torch.randperm(B).cuda()
        g = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        chunks = {"a2c chunk": lambda: vec.ac_train_from_replay(rep, net, idx, adv, ret, n_total=T * N, flat_grad=g),
                  "ppo chunk": lambda: vec.ppo_train_from_replay(rep, net, idx, adv, ret, lpo, vo, n_total=T * N, flat_grad=g),
                  "ppo chunk, sel": lambda: vec.ppo_train_from_replay(rep, net, idx, adv, ret, lpo, vo, sel=sel, n_total=T * N, flat_grad=g, check_sel=False)}
        for fn in chunks.values():
            for _ in range(a.warmup):
                fn()
        res = {c: [] for c in chunks}
        for _ in range(a.repeats):
            for c, fn in chunks.items():
                res[c].append(timed(torch, fn, a.steps))
        for c, v in res.items():
            row("train B=256", B, c + " (ring-fed, flat_grad)", v)
        for n in (5120, 131072):
            x = torch.randn(n, device="cuda")
            y, perm = torch.empty_like(x), torch.empty(n, dtype=torch.int64, device="cuda")
            draw = [0]

            def permute():
                draw[0] += 1
                vec.ac_permute(n, 1, draw[0], out=perm)
            small = {"fb_ac_permute": permute, "fb_ac_normalize_adv": lambda: vec.ac_normalize_adv(x, out=y)}
            for c, fn in small.items():
                for _ in range(a.warmup):
                    fn()
                row("rollout op", n, c, [timed(torch, fn, a.steps) for _ in range(a.repeats)])
        del net, rep, keep
        torch.cuda.synchronize()
        for algo in ("a2c", "ppo"):
            ac = VecActorCritic(N, rollout=T, seed=1, algo=algo)
            for _ in range(10):
                ac.update()
            ups = [timed(torch, ac.update, max(1, a.steps // 10)) for _ in range(a.repeats)]
            what = "T=5: 5 steps, 20 chunks, 1 Adam" if algo == "a2c" else "T=5: 5 steps, 4x4x5 chunks, 16 Adam"
            row(f"{algo} update", N, what, ups)
            row(f"{algo} update", N, "env steps per second", [T * N / (u * 1e-6) for u in ups], unit="1/s")
            del ac
            torch.cuda.synchronize()
        # the PPO update's four forms in ONE process, alternated within each round (target_kl = 1e9 reads after every epoch and never stops)
        forms = {"one_call=False (composed)": dict(one_call=False), "one_call=True": dict(one_call=True),
                 "one_call, adv_norm_scope=minibatch": dict(adv_norm_scope="minibatch"), "one_call, target_kl (3 reads)": dict(target_kl=1e9)}
        acs = {c: VecActorCritic(N, rollout=T, seed=1, algo="ppo", **kw) for c, kw in forms.items()}
        for ac in acs.values():
            for _ in range(10):
                ac.update()
        res = {c: [] for c in acs}
        for _ in range(a.repeats):
            for c, ac in acs.items():
                res[c].append(timed(torch, ac.update, max(1, a.steps // 10)))
        for c, v in res.items():
            row("ppo update", N, c, v)


if __name__ == "__main__":
    main()
