"""How many leaves of the prioritized tree hold a TD-based priority?  ("Initial priorities from acting-time TD
errors".)

    python tools/per_census.py [--envs 1024] [--steps 5000] [--inits max,td] [--n-step 1] [--capacity 1000000] [--out FILE]

Runs fb_vec_step (algo per, B = 32, the fast tree) for --steps steps per setting and then takes the census of the filled leaves:
  by value       MEASURED: the share of leaves whose value on the device differs from the tree's maximum, the max_p a store writes.
                 A lower bound of the leaves with a TD-based priority: a |TD error| of 0.99 or more gives p = 1 = max_p as well (a
                 crash's transition usually does).
  by schedule    DERIVED on the host, not observed: a leaf counts when something other than Memory.store is due to have written it
                 last -- it was sampled (Memory.batch_update; the sampled indices of every step are kept and replayed against the
                 store schedule) at or after the step of its last store, or -- 'td' -- a prime followed that store, which holds for
                 every store but the newest by construction (1 - N / capacity).  It says what the by-value figure is a lower bound of.
Rows go to stdout, and are appended to --out when one is given.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from time_prime import pipeline  # noqa: E402


def census(n_envs, init, n, cap, steps, batch=32):
    step = pipeline(n_envs, init, n, cap, batch)
    rep = step.replay
    drawn = []
    first_train = max(4, n)
    for i in range(steps):
        step(0.01, seed=2, step=i, train=i >= first_train)
        if i >= first_train:
            drawn.append(step.idx.clone())
    tree, pointer, size, _ = rep.per_state()
    leaves = tree[cap - 1:cap - 1 + size]
    max_p = leaves.max()
    by_value = float((leaves != max_p).mean())
    # the store schedule: push S (1-based) stores N leaves when S >= n, store number k = S - n covers data slots (k N + e) mod cap
    stores = steps - n + 1
    last_store = np.full(cap, -1, np.int64)                  # the loop step (0-based) whose push stored the slot last
    for k in range(max(0, stores - (cap + n_envs - 1) // n_envs - 1), stores):
        last_store[(k * n_envs + np.arange(n_envs)) % cap] = k + n - 1
    assert pointer == (stores * n_envs) % cap and size == min(stores * n_envs, cap)
    last_draw = np.full(cap, -1, np.int64)
    if drawn:
        idx = torch.stack(drawn).cpu().numpy() - (cap - 1)       # [steps trained, B] data slots
        at = np.repeat(np.arange(first_train, steps), batch).reshape(idx.shape)
        np.maximum.at(last_draw, idx.ravel(), at.ravel())
    filled = last_store >= 0
    touched = last_draw >= last_store
    if init == "td":
        touched |= last_store < steps - 1                    # due a prime from the step behind its store (assumed, not observed)
    by_prov = float(touched[filled].mean())
    return size, float(max_p), by_prov, by_value


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5000)
    ap.add_argument("--inits", default="max,td")
    ap.add_argument("--n-step", type=int, default=1)
    ap.add_argument("--capacity", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="also append the rows to this file")
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out if a.out else os.devnull, "a") as out:
        def emit(line):
            for f in (sys.stdout, out):
                print(line, file=f); f.flush()
        emit(f"# tools/per_census.py on {torch.cuda.get_device_name(0)}: {' '.join(sys.argv[1:])}")
        emit("#  envs  n  init    steps  filled_leaves   max_p   value != max_p (measured)   by schedule (derived)")
        for init in a.inits.split(","):
            size, max_p, prov, val = census(a.envs, init, a.n_step, a.capacity, a.steps)
            emit(f"  {a.envs:5d} {a.n_step:2d}  {init:4s} {a.steps:8d} {size:14d} {max_p:7.4f} {100 * val:23.3f} % {100 * prov:21.3f} %")
            torch.cuda.synchronize()


if __name__ == "__main__":
    main()
