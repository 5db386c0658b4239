"""What the four vectorised loops print and save on the GPU, pinned to a record.

The `gpu` part of tests/golden/loop_record.json was written ONCE, with the code of commit 97ae14e -- before the loops' shared host code
was written once (tests/test_loop_record_host.py tells what that covers, and holds the `host` part).  It is a record, not a reference to
regenerate: a refactor of the Python layer must reproduce every log line and every checkpoint array of every case, compared with plain
equality.  The loops repeat bit for bit (no atomics, a fixed summation order), so the digests are reproducible on one kind of GPU (the
record's: MI355X); the record was written twice, in two processes, and the two files were identical.
`python -m tests.test_gpu_loop_record --record [PATH]` writes it (needs the GPU).

Per case: the lines of run(), every array of the checkpoint as (dtype, shape, SHA-256), then a fresh object that loads it, the lines it
prints while it goes on, and its checkpoint.  Everything is tiny: fc_width 128, 4 envs, batch 4, capacity 64, observe 2, seed 3; 8 steps
with a line every 4, then 4 more with a line every 2 (VecActorCritic: rollout 2, 3 updates, then 2 more, a line each).  VecBrain's cases
write every optional checkpoint key between them, and the cases with max_grad_norm print the GRAD_NORM / CLIP_SCALE suffix.
"""
import json
import sys

import pytest

from tests.test_loop_record_host import TABLE, merge_record, run_and_resume

pytestmark = pytest.mark.gpu
RING = dict(n_envs=4, batch=4, capacity=64, observe=2, seed=3, fc_width=128)
TAUS = dict(n_tau=2, n_tau_next=2, n_tau_act=4)
CASES = {
    "brain-nature": ("VecBrain", dict(algo="nature")),
    "brain-per-3step": ("VecBrain", dict(algo="per", n_step=3)),
    "brain-rainbow": ("VecBrain", dict(algo="c51doubleper", arch="c51dueling", noisy=True, n_step=3, n_atoms=11)),
    "brain-qrdoubleper": ("VecBrain", dict(algo="qrdoubleper", arch="qrdueling", n_quantiles=8)),
    "brain-mdqn": ("VecBrain", dict(algo="mdqn", arch="dueling", huber=1.0, max_grad_norm=10, polyak=0.01)),
    "iqn": ("VecIQN", dict(TAUS)),
    "iqn-rainbow": ("VecIQN", dict(TAUS, prioritized=True, dueling=True, double_q=True, n_step=3, cvar=0.5, max_grad_norm=10)),
    "iqn-munchausen": ("VecIQN", dict(TAUS, munchausen=True, polyak=0.01)),
    "sac": ("VecSAC", dict(alpha_lr=0)),
    "sac-alpha-clip": ("VecSAC", dict(alpha_lr=1e-3, max_grad_norm=10)),
    "a2c": ("VecActorCritic", dict(algo="a2c")),
    "ppo": ("VecActorCritic", dict(algo="ppo", epochs=2, minibatches=2, value_clip=0.2, max_grad_norm=0.5)),
}


def make(cls, kw):
    if cls == "VecBrain":
        from dqnflappybird_amd.vecbrain import VecBrain
        return VecBrain(**RING, **kw)
    if cls == "VecIQN":
        from dqnflappybird_amd.veciqn import VecIQN
        return VecIQN(**RING, **kw)
    if cls == "VecSAC":
        from dqnflappybird_amd.vecsac import VecSAC
        return VecSAC(**RING, **kw)
    from dqnflappybird_amd.vecac import VecActorCritic
    return VecActorCritic(n_envs=4, rollout=2, capacity=64, seed=3, fc_width=128, **kw)


def run_case(name, tmp):
    cls, kw = CASES[name]
    steps = (3, 1, 2, 1) if cls == "VecActorCritic" else (8, 4, 4, 2)
    return run_and_resume(lambda: make(cls, kw), tmp, name, *steps)


@pytest.fixture(scope="module")
def device():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)["gpu"]


def test_the_record_holds_these_cases(table):
    assert sorted(table) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_loop_prints_and_saves_as_recorded(device, table, tmp_path, name):
    got = json.loads(json.dumps(run_case(name, tmp_path)))
    want = table[name]
    assert sorted(got) == sorted(want)
    for part in ("lines", "resumed_lines"):
        print("\n".join(got[part]))
        assert got[part] == want[part], f"{name}: {part} differ from the record"
    for part in ("checkpoint", "resumed_checkpoint"):
        assert sorted(got[part]) == sorted(want[part]), f"{name}: the keys of the {part} differ from the record"
        wrong = [k for k in got[part] if got[part][k] != want[part][k]]
        assert not wrong, f"{name}: the arrays {wrong} of the {part} differ from the record"


def record(path):
    import tempfile
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory() as tmp:
        rec = {name: run_case(name, tmp) for name in CASES}
    merge_record(path, "gpu", rec)
    for name, r in rec.items():
        print(f"{name}: {len(r['lines'])} + {len(r['resumed_lines'])} lines, {len(r['checkpoint'])} arrays: {' '.join(sorted(r['checkpoint']))}")
        print("  " + r["lines"][-1])
    print(f"{len(rec)} cases -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_gpu_loop_record --record [PATH]")
