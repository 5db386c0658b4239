"""What the six SAC training entry points answer, and what their accepted calls compute and leave behind, pinned to a record.

tests/golden/sac_record.json was written ONCE, with the library of commit f1a040f -- before SAC's uniform and prioritized calls were folded
onto one train path (fb_qnet.hip), one ring-fed call (fb_sac.hip) and the step functions it shares with IQN (fb_common.hip).  It is a
record, not a reference to regenerate: that refactor, and every later one of the host side, must reproduce every return code, every
fb_last_error text and every digest.  The kernels have no atomics and a fixed summation order, so the digests are reproducible on one
kind of GPU (the record's: MI355X).  `python -m tests.test_gpu_sac_record --record [PATH]` writes it (needs the GPU).

Everything is tiny, the shapes of tests/test_gpu_family_record.py: fc_width 128, max_batch 4, 2 envs, capacity 64, six pushes, batch 2,
2 actions.

- Entry points: fb_qnet_sac_train_step, fb_qnet_sac_per_train_step, fb_sac_train_from_replay, fb_sac_per_train_from_replay, fb_sac_step,
  fb_sac_per_step.
- The matrix: the nets {plain, iqn, sac with alpha_lr = 0, sac with alpha_lr > 0 (the temperature's Adam element runs)} times the memories
  {uniform, uniform with a 3-step view, prioritized, prioritized made with n_step = 3 after six pushes, after two (fewer than n: the
  ring-fed training call is refused; the step, which pushes first, is accepted) and after one (a training step is refused, a store-only
  one accepted)}; the two steps with train 0 and 1.
- Per entry point: every handle and every required buffer NULL in turn (the steps with train 0 and 1: what a store-only step requires
  differs between the two), n_envs 3, batch 5, gamma 1.5 and a gamma that is not the memory's, flat_grad set (both sac nets), and for the
  steps rho in {-0.1, 0, 0.005, 1, 1.5, NaN} with train 0 and 1.
- After a refused call the memory's size and push counter and both nets' parameters are what they were.
- Digests: an accepted case starts from a defined state -- seeded online and target nets, zeroed Adam slots, fb_qnet_set_sac freshly
  applied, the memory and its env restored from a saved blob -- so no case depends on the order of the others.  SHA-256 of the bytes of
  loss f32[6], q_target, abs_err, a / r / t, idx, isw / isw32, actions, flat_grad, the online AND the target parameters after the call
  (the soft update shows), the five words of fb_qnet_get_sac_state and the memory's state blob (the push counter; a prioritized memory's
  tree after the priorities' update).
"""
import ctypes as C
import hashlib
import json
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sac_record.json")
FC, MAXB, N, B, CAP, GAMMA, RHO = 128, 4, 2, 2, 64, 0.99, 0.005
NAN = float("nan")

NETS = {"plain": ("plain", None), "iqn": ("iqn", None), "sac0": ("sac", 0.0), "sac1": ("sac", 0.01)}      # name -> (arch, alpha_lr)
MEMS = {"uniform": (False, 1, 6), "uniform3": (False, 1, 6), "per": (True, 1, 6), "per3": (True, 3, 6), "per3short": (True, 3, 2),
        "per3one": (True, 3, 1)}      # (prioritized, n at creation, pushes)
NET_ENTRIES = ("fb_qnet_sac_train_step", "fb_qnet_sac_per_train_step")
RING_ENTRIES = ("fb_sac_train_from_replay", "fb_sac_per_train_from_replay")
STEP_ENTRIES = ("fb_sac_step", "fb_sac_per_step")
PER_ENTRIES = ("fb_qnet_sac_per_train_step", "fb_sac_per_train_from_replay", "fb_sac_per_step")
ENTRIES = NET_ENTRIES + RING_ENTRIES + STEP_ENTRIES
RHOS = (-0.1, 0.0, RHO, 1.0, 1.5, NAN)
ENV_BUFFERS = ("nib", "actions", "frame_bits", "reward", "terminal", "score")


def nullable(entry):
    """the handles and required buffers of an entry point, each passed as NULL in turn"""
    weights = ("isw", "abs_err") if entry in PER_ENTRIES else ()
    if entry in NET_ENTRIES:
        return ("net", "s", "a", "r", "s2", "t", "loss") + weights
    if entry in RING_ENTRIES:
        return ("replay", "net", "idx", "a", "r", "t", "loss") + weights
    return ("env", "replay", "net", "b") + ENV_BUFFERS + ("idx", "a", "r", "t", "loss") + (("isw", "isw32", "abs_err") if weights else ())


def sha(x):
    if hasattr(x, "detach"):
        x = x.detach().contiguous().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


class World:
    """the nets, the memories (each with an env of its own) and one set of buffers, sized for the largest batch any case passes"""

    def __init__(self, torch):
        from dqnflappybird_amd import _lib as L
        from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay
        self.torch, self.L, self.lib = torch, L, L.lib()
        self.nets, self.seeds = {}, {}
        for k, (name, (arch, _)) in enumerate(NETS.items()):
            net = QNet(2, FC, arch, max_batch=MAXB, **(dict(n_tau=2, n_tau_next=2, n_tau_act=4) if arch == "iqn" else {}))
            net.set_hparams(lr=1e-3, eps=1e-4)     # (an update whose size depends on the gradient's, not on its sign alone)
            self.nets[name], self.seeds[name] = net, k + 1
        self.envs, self.mems, self.saved, self.fixed_idx = {}, {}, {}, {}
        for k, (name, (prioritized, n, pushes)) in enumerate(MEMS.items()):
            env = VecGameState(N, seed=k + 1)
            env.track_state()
            env.observe()
            rep = VecReplay(CAP, N, prioritized=prioritized, n_step=n, gamma=GAMMA if n > 1 else None)
            rep.seed(k + 1)
            rep.reset(env.frame_bits)
            act = torch.zeros(N, dtype=torch.uint8, device="cuda")
            for t in range(pushes):
                act[:] = t % 3 == 0
                _, rew, term, _ = env.frame_step(act)
                rep.push(env.frame_bits, act, rew, term)
            if name == "uniform3":
                rep.set_n_step(3, GAMMA)
            self.envs[name], self.mems[name] = env, rep
            # B legitimate indices (deque positions, or tree indices of a prioritized one); the short memories' trees are empty and every
            # call on them that would read the caller's idx is refused: they borrow per3's
            self.fixed_idx[name] = self.fixed_idx["per3"] if pushes < n else rep.sample(B)[0].clone()
            torch.cuda.synchronize()
            self.saved[name] = (rep.state_blob().copy(), env.get_state().copy(), env.nib.clone(), env.frame_bits.clone(), env.reward.clone(),
                                env.terminal.clone(), env.score.clone())
        self.dirty = set(self.nets)                # nets / memories an accepted call has moved: put back before the next call on them
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        R = 16                                     # rows: above every batch (MAXB + 1) and every env count (N + 1) passed
        self.idx, self.s, self.s2 = z(R, torch.int64), z((R, 80, 80, 4), torch.uint8), z((R, 80, 80, 4), torch.uint8)
        self.a, self.r, self.t = z(R, torch.uint8), z(R, torch.float32), z(R, torch.uint8)
        self.isw_in, self.isw64, self.isw32, self.abs_err = z(R, torch.float32), z(R, torch.float64), z(R, torch.float32), z(R, torch.float32)
        self.isw_in[:] = 0.5 + 0.25 * torch.arange(R, device="cuda")
        self.loss, self.y, self.actions = z(8, torch.float32), z(R, torch.float32), z(R, torch.uint8)
        self.flat_grad = z(max(net.n_params for net in self.nets.values()), torch.float32)
        self.s[:B] = self.mems["uniform"].current_state()
        self.s2[:B] = self.mems["uniform3"].current_state()
        self.s[B:] = self.s[:B].repeat(R // B - 1, 1, 1, 1)
        self.ga, self.gr, self.gt = z(R, torch.uint8), z(R, torch.float32), z(R, torch.uint8)      # the gathered calls' a / r / t
        self.ga[1::2] = 1
        self.gr[:] = 0.1 + 0.9 * (torch.arange(R, device="cuda") % 2)
        self.gt[1::2] = 1

    # -- defined states
    def fresh(self, netname, mem):
        """the state every case starts from, for what an accepted call has moved since"""
        torch, lib, L = self.torch, self.lib, self.L
        if netname in self.dirty:
            net = self.nets[netname]
            net.init_params(seed=self.seeds[netname])
            net.sync_target()
            net.init_params(seed=self.seeds[netname] + 100, which=L.NET_TARGET)      # (a target of its own: the target slice and the soft update show)
            zero = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            net.set_adam_state(zero, zero, np.array([0.9, 0.999], np.float32))
            if net.arch == "sac":
                assert lib.fb_qnet_set_sac(net.h, 0.2, 0.98 * math.log(2.0), NETS[netname][1]) == 0
            self.dirty.discard(netname)
        if mem is not None and mem in self.dirty:
            blob, state, nib, bits, rew, term, score = self.saved[mem]
            env, rep = self.envs[mem], self.mems[mem]
            torch.cuda.synchronize()
            rep.load_state_blob(blob)
            if mem == "uniform3":
                rep.set_n_step(3, GAMMA)
            env.set_state(state)
            env.nib.copy_(nib), env.frame_bits.copy_(bits), env.reward.copy_(rew), env.terminal.copy_(term), env.score.copy_(score)
            self.dirty.discard(mem)
        for x in (self.idx, self.loss, self.y, self.abs_err, self.a, self.r, self.t, self.isw64, self.isw32, self.actions, self.flat_grad):
            x.zero_()

    def snapshot(self, netname, mem):
        out = [self.nets[netname].store_params(w).clone() for w in (0, 1)]
        if mem is not None:
            blob = np.asarray(self.mems[mem].state_blob())
            out += [len(self.mems[mem]), int(blob[24:32].view(np.int64)[0])]      # (ReplayBlobHeader: the push counter)
        return out

    def same(self, x, y):
        return self.torch.equal(x[0], y[0]) and self.torch.equal(x[1], y[1]) and x[2:] == y[2:]

    def finish(self, rc, what, netname, mem, before):
        """(rc, text, digests of an accepted call's outputs or None); a refused call has left everything as it was"""
        text = "" if rc == 0 else self.lib.fb_last_error().decode()
        self.torch.cuda.synchronize()
        if rc != 0:
            assert self.same(self.snapshot(netname, mem), before), f"{what} refused ({text!r}) and left the memory's counters or the net's parameters changed"
            return [rc, text, None]
        self.dirty.update(x for x in (netname, mem) if x is not None)
        net = self.nets[netname]
        out = {"loss": self.loss[:6], "q_target": self.y[:B], "abs_err": self.abs_err[:B], "a": self.a[:B], "r": self.r[:B], "t": self.t[:B],
               "idx": self.idx[:B], "isw": self.isw64[:B], "isw32": self.isw32[:B], "actions": self.actions[:N], "flat_grad": self.flat_grad,
               "params": net.store_params(0), "target_params": net.store_params(1), "sac_state": net.sac_state()}
        if mem is not None:
            out["memory"] = self.mems[mem].state_blob()
        return [rc, text, {k: sha(v) for k, v in out.items()}]

    # -- one call of an entry point.  null: the handle or buffer passed as NULL; the other keywords change one argument each
    def call(self, entry, netname, mem, train=1, null=None, batch=B, n_envs=N, gamma=GAMMA, rho=RHO, flat_grad=False):
        L, lib = self.L, self.lib
        net = self.nets[netname]
        self.fresh(netname, mem)
        if mem is not None and entry in RING_ENTRIES:
            self.idx[:B] = self.fixed_idx[mem]
        before = self.snapshot(netname, mem)
        rep, env = (self.mems[mem], self.envs[mem]) if mem is not None else (None, None)
        p = lambda name, x: None if null == name else L.ptr(x)
        h = lambda name, obj: None if null == name else obj.h
        fg = L.ptr(self.flat_grad) if flat_grad else None
        if entry in NET_ENTRIES:
            head = (h("net", net), batch, p("s", self.s), p("a", self.ga), p("r", self.gr), p("s2", self.s2), p("t", self.gt))
            if entry == "fb_qnet_sac_train_step":
                rc = lib.fb_qnet_sac_train_step(*head, gamma, p("loss", self.loss), L.ptr(self.y), fg, None)
            else:
                rc = lib.fb_qnet_sac_per_train_step(*head, p("isw", self.isw_in), gamma, p("loss", self.loss), p("abs_err", self.abs_err), L.ptr(self.y),
                                                    fg, None)
        elif entry in RING_ENTRIES:
            head = (h("replay", rep), h("net", net), batch, p("idx", self.idx))
            art = (p("a", self.a), p("r", self.r), p("t", self.t), gamma, p("loss", self.loss))
            if entry == "fb_sac_train_from_replay":
                rc = lib.fb_sac_train_from_replay(*head, *art, L.ptr(self.y), fg, None)
            else:
                rc = lib.fb_sac_per_train_from_replay(*head, p("isw", self.isw_in), *art, p("abs_err", self.abs_err), L.ptr(self.y), fg, None)
        else:
            d = lambda name, x: None if null == name else x.data_ptr()
            sb = L.StepBuffers(d("nib", env.nib), d("actions", self.actions), d("frame_bits", env.frame_bits), d("reward", env.reward),
                               d("terminal", env.terminal), d("score", env.score), d("idx", self.idx), self.s.data_ptr(), self.s2.data_ptr(),
                               d("a", self.a), d("t", self.t), d("r", self.r), d("loss", self.loss), self.flat_grad.data_ptr() if flat_grad else None,
                               d("isw", self.isw64), d("isw32", self.isw32), d("abs_err", self.abs_err))
            rc = getattr(lib, entry)(h("env", env), h("replay", rep), h("net", net), None if null == "b" else C.byref(sb), n_envs, batch, 3, 5, train,
                                     gamma, rho, None)
        return self.finish(rc, f"{entry} ({netname}, {mem}, train {train}, null {null}, batch {batch}, n_envs {n_envs}, gamma {gamma}, rho {rho})",
                           netname, mem, before)


def run_entry(w, entry):
    """every case of one entry point -> {case key: [rc, text, digests or None]}"""
    out = {}
    step = entry in STEP_ENTRIES
    trains = (0, 1) if step else (1,)
    for net in NETS:
        for mem in (MEMS if entry not in NET_ENTRIES else (None,)):
            for train in trains:
                out[f"{net}|{mem}|train={train}"] = w.call(entry, net, mem, train)
    home = None if entry in NET_ENTRIES else "per3" if entry in PER_ENTRIES else "uniform"
    for train in trains:
        for name in nullable(entry):
            out[f"arg|{name}=NULL|train={train}"] = w.call(entry, "sac0", home, train, null=name)
        out[f"arg|batch=5|train={train}"] = w.call(entry, "sac0", home, train, batch=MAXB + 1)
        for gamma in (1.5, 0.5):
            out[f"arg|gamma={gamma}|train={train}"] = w.call(entry, "sac0", home, train, gamma=gamma)
        for net in ("sac0", "sac1"):
            out[f"arg|flat_grad|{net}|train={train}"] = w.call(entry, net, home, train, flat_grad=True)
        if step:
            out[f"arg|n_envs=3|train={train}"] = w.call(entry, "sac0", home, train, n_envs=N + 1)
            for rho in RHOS:
                out[f"arg|rho={rho!r}|train={train}"] = w.call(entry, "sac0", home, train, rho=rho)
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


def recorded(table, entry):
    """the entry point's cases as run_entry returns them: answers and digests are stored once each"""
    out = {}
    for k, i in table["cases"][entry].items():
        rc, text, dig = table["answers"][i]
        out[k] = [rc, text, None if dig is None else {name: table["digests"][j] for name, j in dig.items()}]
    return out


@pytest.mark.parametrize("entry", ENTRIES)
def test_sac_entry_point_answers_and_computes_as_recorded(world, table, entry):
    got, want = json.loads(json.dumps(run_entry(world, entry))), recorded(table, entry)
    assert sorted(got) == sorted(want), f"{entry}: the cases run and the recorded ones differ"
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    for k, (g, r) in list(wrong.items())[:10]:
        print(f"{entry} {k}:\n  got      {g}\n  recorded {r}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases of {entry} answer differently from the record"
    accepted = sum(1 for v in got.values() if v[0] == 0)
    print(f"{entry}: {len(got)} cases, {accepted} accepted")
    assert 0 < accepted < len(got)


def record(path):
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    world = World(torch)
    digests, answers, cases = [], [], {}

    def index(pool, v):
        if v not in pool:
            pool.append(v)
        return pool.index(v)
    for entry in ENTRIES:
        cases[entry] = {}
        for k, (rc, text, dig) in run_entry(world, entry).items():
            cases[entry][k] = index(answers, [rc, text, None if dig is None else {name: index(digests, d) for name, d in dig.items()}])
        print(f"{entry}: {len(cases[entry])} cases, {sum(1 for i in cases[entry].values() if answers[i][0] == 0)} accepted")
    with open(path, "w") as f:
        json.dump({"digests": digests, "answers": answers, "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"recorded {sum(len(c) for c in cases.values())} cases, {len(answers)} distinct answers, {len(digests)} distinct digests -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_gpu_sac_record --record [PATH]")
