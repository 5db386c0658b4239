"""What A2C costs: µs per fb_ac_rollout_step against fb_vec_step(train = 0) at the same env count, µs per 256-sample ring-fed A2C chunk
(exported gradient) against the 'double' train step at B = 256 with flat_grad, and the whole update at 1024 envs x T = 5.

    python tools/time_a2c.py [--envs 1024,4096] [--steps 300] [--warmup 100] [--repeats 5] [--out FILE]

Rows go to stdout, and are appended to --out when one is given.

rollout step: AcRolloutStep on an actor-critic net (policy head and replay push as launches of their own) and VecStep(train=False) on a
plain net (head and push riding in the env launch), one pipeline each, warmed up, then --repeats rounds of --steps timed steps, the
two alternated within each round.  The yardstick for the difference is two dependent empty launches: the tool runs tools/mb/mb_launch
(building it from tools/mb/mb_launch.hip if the binary is missing) as a child process first and reports its one-workgroup rows.
chunk: vec.ac_train_from_replay(flat_grad) and vec.train_from_replay('double', flat_grad) at B = 256 on the memories the rollout
filled, the same alternation.  update: VecActorCritic(1024, rollout=5).update(), env steps per second = 5 x 1024 / the update's time.
Reported: the median and the spread of the rounds.
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from dqnflappybird_amd.vec import (AcRolloutStep, QNet, VecGameState, VecReplay, VecStep, ac_train_from_replay,  # noqa: E402
                                   train_from_replay)
from dqnflappybird_amd.vecac import VecActorCritic  # noqa: E402

T = 5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launch_floor():
    """us per dependent launch of a kernel that does next to nothing, one workgroup (tools/mb/mb_launch.hip) -> [(shape, us)], or a reason"""
    exe, src = os.path.join(ROOT, "tools", "mb", "mb_launch"), os.path.join(ROOT, "tools", "mb", "mb_launch.hip")
    try:
        if not os.path.exists(exe):
            subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", src, "-o", exe], check=True, capture_output=True, timeout=300)
        out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    except (OSError, subprocess.SubprocessError) as e:
        return f"not measured ({type(e).__name__}: {e})"
    rows = []
    for line in out.splitlines():
        f = line.split()
        if line.startswith("G") and f[1] == "1" and f[6] == "0" and f[4] in ("64", "256"):       # G 1 x T 64 | 256, no LDS
            rows.append((f"G 1 x T {f[4]}", float(f[line.split().index(":") + 1])))
    return rows or "not measured (no one-workgroup row in tools/mb/mb_launch's output)"


def pipeline(n_envs, arch):
    env = VecGameState(n_envs, seed=1)
    net = QNet(2, 512, arch, max_batch=max(n_envs, 256))
    rep = VecReplay((T + 2) * n_envs if arch == "ac" else 1_000_000, n_envs)
    rep.seed(3, "cpython")
    net.init_params(5, which=0); net.init_params(6, which=1)
    env.track_state(); env.observe(); rep.reset(env.frame_bits)
    step = AcRolloutStep(env, rep, net, T) if arch == "ac" else VecStep(env, rep, net, 32, "double", 0.99)
    return dict(env=env, net=net, rep=rep, step=step, arch=arch, k=0)


def one(p):
    if p["arch"] == "ac":
        p["step"](p["k"] % T, seed=2, step=p["k"])
    else:
        p["step"](0.0, seed=2, step=p["k"], train=False)
    p["k"] += 1


def timed(fn, k):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / k * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="1024,4096")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()

        def row(what, n, config, v, unit="us"):
            emit(f"  {what:13s} {n:5d}  {config:22s} {statistics.median(v):10.1f} {min(v):9.1f} {max(v):9.1f}  {unit}")

        emit(f"# tools/time_a2c.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        floor = launch_floor()                   # (a child process of its own, before this one holds much of the GPU)
        if isinstance(floor, str):
            emit(f"# empty dependent launch: {floor}")
        else:
            for shape, us in floor:
                emit(f"# empty dependent launch (tools/mb/mb_launch, {shape}): {us:.2f} us per launch, two of them {2 * us:.2f} us")
        emit("#  what           envs  config                     median       min       max")
        for n_envs in [int(x) for x in a.envs.split(",")]:
            pipes = {"fb_ac_rollout_step": pipeline(n_envs, "ac"), "fb_vec_step(train=0)": pipeline(n_envs, "plain")}
            for p in pipes.values():
                for _ in range(a.warmup):
                    one(p)
            res = {c: [] for c in pipes}
            for _ in range(a.repeats):
                for c, p in pipes.items():
                    res[c].append(timed(lambda: one(p), a.steps))
            for c, v in res.items():
                row("rollout step", n_envs, c, v)
            if n_envs == 1024:                   # the chunk, on the memories the steps above filled
                B = 256
                acp, dqp = pipes["fb_ac_rollout_step"], pipes["fb_vec_step(train=0)"]
                idx_ac = (len(acp["rep"]) - B + torch.arange(B, dtype=torch.int64)).cuda()
                idx_dq = torch.arange(B, dtype=torch.int64).cuda() * 7
                adv, ret = torch.randn(B, device="cuda"), torch.randn(B, device="cuda")
                g_ac = torch.zeros(acp["net"].n_params, dtype=torch.float32, device="cuda")
                g_dq = torch.zeros(dqp["net"].n_params, dtype=torch.float32, device="cuda")
                chunks = {"a2c chunk (1 slice)": lambda: ac_train_from_replay(acp["rep"], acp["net"], idx_ac, adv, ret, n_total=T * 1024, flat_grad=g_ac),
                          "double (3 slices)": lambda: train_from_replay(dqp["rep"], dqp["net"], "double", idx_dq, 0.99, flat_grad=g_dq)}
                for fn in chunks.values():
                    for _ in range(20):
                        fn()
                rc = {c: [] for c in chunks}
                for _ in range(a.repeats):
                    for c, fn in chunks.items():
                        rc[c].append(timed(fn, a.steps))
                for c, v in rc.items():
                    row("train B=256", B, c, v)
            del pipes
            torch.cuda.synchronize()
        ac = VecActorCritic(1024, rollout=T, seed=1)
        for _ in range(20):
            ac.update()
        ups = [timed(ac.update, max(1, a.steps // 5)) for _ in range(a.repeats)]
        row("update", 1024, f"T={T}: 5 steps, 20 chunks", ups)
        row("update", 1024, "env steps per second", [T * 1024 / (u * 1e-6) for u in ups], unit="1/s")


if __name__ == "__main__":
    main()
