"""What every ring-fed entry point answers to every (net, memory, algo) combination, pinned to a recorded table.

tests/golden/refusals.json holds (return code, fb_last_error text) of each call below -- (0, "") for an accepted one -- as the library
answered BEFORE the host-side checks of these entry points were folded into shared functions (fb_check_algo and its kin, fb_common.h).
The table is a record, not a reference to regenerate: a refactor of the checks must reproduce every code and every text.
`python -m tests.test_gpu_refusals --record [PATH]` writes it (needs the GPU).

The matrix: 9 nets (plain, dueling, C51, dueling C51, noisy C51, QR, AC, SAC, IQN at fc_width 128, the smallest action count their
constructor takes, max_batch 4) x 3 memories (uniform, prioritized, uniform with a 3-step view; capacity 64, 2 envs, six pushes) x
every algo of vec.ALGOS plus -1 and 99, through each entry point that takes an algo; the same nets and memories through the entry
points that take none; and per entry point a NULL buffer, an n_envs mismatch, a batch above max_batch and a gamma that is outside
[0, 1] or not the memory's.  Accepted calls run a real step at batch 2.  After every refused call the memory's size and push count and
both nets' parameters are what they were.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refusals.json")
FC, MAXB, N, B, CAP, GAMMA = 128, 4, 2, 2, 64, 0.99
NETS = {"plain": ("plain", 1, {}), "dueling": ("dueling", 1, {}), "c51": ("c51", 1, {}), "c51dueling": ("c51dueling", 1, {}),
        "c51noisy": ("c51", 1, {"noisy": True}), "qr": ("qr", 1, {}), "ac": ("ac", 1, {}), "sac": ("sac", 2, {}), "iqn": ("iqn", 2, {})}
MEMS = ("uniform", "per", "uniform3")
ALGO_ENTRIES = ("fb_qnet_train_step", "fb_train_from_replay", "fb_train_steps", "fb_vec_step", "fb_vec_step_dp")
PLAIN_ENTRIES = ("fb_ac_train_from_replay", "fb_ppo_train_from_replay", "fb_sac_train_from_replay", "fb_iqn_train_from_replay", "fb_sac_step",
                 "fb_iqn_step", "fb_ac_rollout_step")
ARG_CASES = ("null", "n_envs", "batch", "gamma")
# the (net, memory, algo) each entry point's argument cases start from: a combination it accepts
HOME = {"fb_qnet_train_step": ("plain", "uniform3", "dqn"), "fb_train_from_replay": ("plain", "uniform3", "dqn"),
        "fb_train_steps": ("plain", "uniform3", "dqn"), "fb_vec_step": ("plain", "uniform3", "dqn"), "fb_vec_step_dp": ("plain", "uniform3", "dqn"),
        "fb_ac_train_from_replay": ("ac", "uniform", None), "fb_ppo_train_from_replay": ("ac", "uniform", None),
        "fb_sac_train_from_replay": ("sac", "uniform", None), "fb_iqn_train_from_replay": ("iqn", "uniform3", None),
        "fb_sac_step": ("sac", "uniform", None), "fb_iqn_step": ("iqn", "uniform3", None), "fb_ac_rollout_step": ("ac", "uniform", None)}


def algo_ids():
    from dqnflappybird_amd.vec import ALGOS
    ids = dict(sorted(ALGOS.items(), key=lambda kv: kv[1]))
    ids.update({"minus1": -1, "ninety9": 99})
    return ids


class World:
    """the nets, the memories (each with an env of its own) and one set of buffers, sized for the largest batch any case passes"""

    def __init__(self, torch):
        from dqnflappybird_amd import _lib as L
        from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay
        self.torch, self.L, self.lib = torch, L, L.lib()
        self.nets = {}
        for k, (name, (arch, A, kw)) in enumerate(NETS.items()):
            net = QNet(A, FC, arch, max_batch=MAXB, **kw)
            net.init_params(seed=k + 1)
            net.sync_target()
            self.nets[name] = net
        self.envs, self.mems = {}, {}
        for k, name in enumerate(MEMS):
            env = VecGameState(N, seed=k + 1)
            env.track_state()
            env.observe()
            rep = VecReplay(CAP, N, prioritized=name == "per")
            rep.seed(k + 1)
            rep.reset(env.frame_bits)
            act = torch.zeros(N, dtype=torch.uint8, device="cuda")
            for t in range(6):
                act[:] = t % 3 == 0
                _, rew, term, _ = env.frame_step(act)
                rep.push(env.frame_bits, act, rew, term)
            if name == "uniform3":
                rep.set_n_step(3, GAMMA)
            self.envs[name], self.mems[name] = env, rep
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        R = 8                                      # rows: above every batch passed (MAXB + 1), twice over for fb_train_steps' two index buffers
        self.idx, self.s, self.s2 = z(2 * R, torch.int64), z((R, 80, 80, 4), torch.uint8), z((R, 80, 80, 4), torch.uint8)
        self.a, self.r, self.t = z(R, torch.uint8), z(R, torch.float32), z(R, torch.uint8)
        self.isw, self.isw64, self.abs_err = torch.ones(R, dtype=torch.float32, device="cuda"), z(R, torch.float64), z(R, torch.float32)
        self.adv, self.loss, self.actions = z(R, torch.float32), z(8, torch.float32), z(N, torch.uint8)
        self.value, self.logp = z((2, N), torch.float32), z((1, N), torch.float32)
        self.s[:B] = self.mems["uniform"].current_state()
        self.s2[:B] = self.mems["uniform3"].current_state()

    def sample(self, mem):
        """B legitimate indices of the memory in self.idx (deque positions, or tree indices of the prioritized one)"""
        idx, _ = self.mems[mem].sample(B)
        self.idx[:B] = idx

    def snapshot(self, net, mem):
        out = [net.store_params(w).clone() for w in (0, 1)]
        if mem is not None:
            blob = np.asarray(self.mems[mem].state_blob())
            out += [len(self.mems[mem]), int(blob[24:32].view(np.int64)[0])]      # (ReplayBlobHeader: the push counter)
        return out

    def same(self, x, y):
        return self.torch.equal(x[0], y[0]) and self.torch.equal(x[1], y[1]) and x[2:] == y[2:]

    def call(self, entry, netname, mem, algo, case=None):
        """one call -> (rc, text); the four argument cases change one argument of the call"""
        L, lib, p = self.L, self.lib, self.L.ptr
        net, rep, env = self.nets[netname], self.mems[mem], self.envs[mem]
        null, batch = case == "null", MAXB + 1 if case == "batch" else B
        n_envs = N + 1 if case == "n_envs" else N
        gamma = GAMMA if case != "gamma" else 0.5 if rep.n_step[0] > 1 else 1.5
        loss = None if null else p(self.loss)
        d = lambda x: x.data_ptr()
        sb = L.StepBuffers(d(env.nib), d(self.actions), d(env.frame_bits), d(env.reward), d(env.terminal), d(env.score), d(self.idx), d(self.s),
                           d(self.s2), d(self.a), d(self.t), d(self.r), None if null else d(self.loss), None, d(self.isw64), d(self.isw),
                           d(self.abs_err))
        self.sample(mem)
        before = self.snapshot(net, None if entry == "fb_qnet_train_step" else mem)
        if entry == "fb_qnet_train_step":
            rc = lib.fb_qnet_train_step(net.h, algo, batch, p(self.s), p(self.a), p(self.r), p(self.s2), p(self.t), p(self.isw), gamma, loss,
                                        p(self.abs_err), None, None, None)
        elif entry == "fb_train_from_replay":
            rc = lib.fb_train_from_replay(rep.h, net.h, algo, batch, p(self.idx), p(self.isw), p(self.a), p(self.r), p(self.t), gamma, loss,
                                          p(self.abs_err), None, None)
        elif entry == "fb_train_steps":
            rc = lib.fb_train_steps(rep.h, net.h, algo, batch, 1, p(self.idx), p(self.s), p(self.s2), p(self.a), p(self.r), p(self.t), loss, gamma, None)
        elif entry == "fb_vec_step":
            rc = lib.fb_vec_step(env.h, rep.h, net.h, C.byref(sb), n_envs, algo, batch, 0.1, 3, 5, 1, gamma, None)
        elif entry == "fb_vec_step_dp":
            rc = lib.fb_vec_step_dp(None, env.h, rep.h, net.h, C.byref(sb), n_envs, algo, batch, 0.1, 3, 5, 1, gamma, 0, None)
        elif entry == "fb_ac_train_from_replay":
            rc = lib.fb_ac_train_from_replay(rep.h, net.h, batch, p(self.idx), p(self.adv), p(self.adv), batch, p(self.a), loss, None, None)
        elif entry == "fb_ppo_train_from_replay":
            rc = lib.fb_ppo_train_from_replay(rep.h, net.h, batch, p(self.idx), None, p(self.adv), p(self.adv), p(self.adv), p(self.adv), batch,
                                              p(self.a), loss, None, None)
        elif entry == "fb_sac_train_from_replay":
            rc = lib.fb_sac_train_from_replay(rep.h, net.h, batch, p(self.idx), p(self.a), p(self.r), p(self.t), gamma, loss, None, None, None)
        elif entry == "fb_iqn_train_from_replay":
            rc = lib.fb_iqn_train_from_replay(rep.h, net.h, 0, batch, p(self.idx), p(self.a), p(self.r), p(self.t), None, None, 3, 5, gamma, loss,
                                              None, None, None)
        elif entry == "fb_sac_step":
            rc = lib.fb_sac_step(env.h, rep.h, net.h, C.byref(sb), n_envs, batch, 3, 5, 1, gamma, 0.005, None)
        elif entry == "fb_iqn_step":
            rc = lib.fb_iqn_step(env.h, rep.h, net.h, C.byref(sb), n_envs, 0, batch, 0.1, 3, 5, 1, gamma, None)
        elif entry == "fb_ac_rollout_step":
            rb = L.AcRolloutBuffers(d(env.nib), d(self.actions), d(env.frame_bits), d(self.r), d(self.t), d(env.score), d(self.value),
                                    None if null else d(self.logp), 1)
            rc = lib.fb_ac_rollout_step(env.h, rep.h, net.h, C.byref(rb), n_envs, 3, 5, 0, None)
        else:
            raise KeyError(entry)
        text = "" if rc == 0 else lib.fb_last_error().decode()
        self.torch.cuda.synchronize()
        if rc != 0:
            assert self.same(self.snapshot(net, None if entry == "fb_qnet_train_step" else mem), before), (
                f"{entry} refused ({netname}, {mem}, algo {algo}, case {case}: {text!r}) and left the memory's counters or the net's parameters changed")
        return rc, text


def run_entry(world, entry):
    """every case of one entry point -> {case key: [rc, text]}"""
    out = {}
    if entry in ALGO_ENTRIES:
        for net in NETS:
            for mem in MEMS:
                for name, algo in algo_ids().items():
                    out[f"{net}|{mem}|{name}"] = list(world.call(entry, net, mem, algo))
    else:
        for net in NETS:
            for mem in MEMS:
                out[f"{net}|{mem}"] = list(world.call(entry, net, mem, None))
    net, mem, algo = HOME[entry]
    for case in ARG_CASES:
        out[f"arg|{case}"] = list(world.call(entry, net, mem, None if algo is None else algo_ids()[algo], case))
    return out


@pytest.fixture(scope="module")
def world():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return World(torch)


@pytest.fixture(scope="module")
def table():
    with open(TABLE) as f:
        return json.load(f)


@pytest.mark.parametrize("entry", ALGO_ENTRIES + PLAIN_ENTRIES)
def test_entry_point_answers_as_recorded(world, table, entry):
    want = {k: table["answers"][i] for k, i in table["cases"][entry].items()}
    got = run_entry(world, entry)
    assert sorted(got) == sorted(want), "the matrix and the recorded table list different cases"
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    for k, (g, w) in list(wrong.items())[:10]:
        print(f"{entry} {k}: got {g}, recorded {w}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases of {entry} answer differently from the record"
    accepted = sum(1 for v in got.values() if v[0] == 0)
    print(f"{entry}: {len(got)} cases, {accepted} accepted")
    assert 0 < accepted < len(got) or entry == "fb_vec_step_dp" and accepted == 0


def record(path):
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    world = World(torch)
    answers, cases = [], {}
    for entry in ALGO_ENTRIES + PLAIN_ENTRIES:
        cases[entry] = {}
        for k, v in run_entry(world, entry).items():
            if v not in answers:
                answers.append(v)
            cases[entry][k] = answers.index(v)
    with open(path, "w") as f:
        json.dump({"answers": answers, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(c) for c in cases.values())} cases, {len(answers)} distinct answers -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_gpu_refusals --record [PATH]")
