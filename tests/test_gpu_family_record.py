"""What the net creators and the IQN entry points answer, and what the accepted IQN / SAC / A2C / PPO steps compute, pinned to a record.

tests/golden/family_record.json was written ONCE, with the library of commit cc9f0a5 -- before the host wiring of the net families was
folded (one creation spec, one allocation list, typed launchers of fb_ac.hip / fb_sac.hip / fb_iqn.hip, one IQN path under the uniform
and the prioritized calls).  It is a record, not a reference to regenerate: that refactor, and every later one of the host side, must
reproduce every return code, every fb_last_error text, every getter value and every digest.  The kernels have no atomics and a fixed
summation order, so the digests are reproducible on one kind of GPU (the record's: MI355X).
`python -m tests.test_gpu_family_record --record [PATH]` writes it (needs the GPU).

Everything is tiny: fc_width 128, max_batch 4, 2 envs, capacity 64, six pushes, batch 2, n_tau = n_tau_next = 2, n_tau_act = 4.

- Creators: each of the nine fb_qnet_create* with `out` NULL, every shared bound (fc_width, n_actions, max_batch), every arch -1..10 where
  it takes one, the family's own refusals, and one accepted creation; of an accepted creation fb_qnet_num_params, fb_qnet_is_noisy and
  what every getter answers (so a setting that creation passes on is seen to arrive).
- IQN entry points: the ten calls over the nets {plain, sac, iqn, iqndueling, iqn with Munchausen on}, the memories {uniform,
  prioritized, uniform with a 3-step view} and double_q in {0, 1, 2}, plus per entry a NULL buffer, an n_envs mismatch, batch 5, a
  gamma outside [0, 1] or not the memory's, and isw / abs_err NULL for the prioritized calls.  After a refused call the memory's size and
  push counter and both nets' parameters are what they were.
- Digests: an accepted case starts from a defined state -- init_params(seed), sync_target, then a target net initialised with a seed of
  its own (so that double_q and the target slices show), zeroed Adam slots, beta powers reset, the memory and its env as they were after
  the six pushes -- so no case depends on the order of the others.  SHA-256 of the bytes of the
  loss, T (q_target), abs_err, a / r / t (each where produced) and the online parameters after the step.  The same for one accepted
  step each of fb_sac_train_from_replay, fb_ac_train_from_replay and fb_ppo_train_from_replay.
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
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "family_record.json")
FC, MAXB, N, B, CAP, GAMMA = 128, 4, 2, 2, 64, 0.99
NT, NTA = 2, 4
NAN = float("nan")

# ---------------------------------------------------------------- creators
# name -> the arguments in call order (`out` follows them); ACCEPTED: what the accepted creation passes
CREATORS = {
    "fb_qnet_create": ("arch", "fc_width", "n_actions", "max_batch"),
    "fb_qnet_create_c51": ("fc_width", "n_actions", "n_atoms", "v_min", "v_max", "max_batch"),
    "fb_qnet_create_c51_dueling": ("fc_width", "n_actions", "n_atoms", "v_min", "v_max", "max_batch"),
    "fb_qnet_create_c51_noisy": ("arch", "fc_width", "n_actions", "n_atoms", "v_min", "v_max", "sigma0", "max_batch"),
    "fb_qnet_create_qr": ("arch", "fc_width", "n_actions", "n_quantiles", "kappa", "max_batch"),
    "fb_qnet_create_ac": ("fc_width", "n_actions", "max_batch"),
    "fb_qnet_create_sac": ("fc_width", "n_actions", "max_batch"),
    "fb_qnet_create_iqn": ("fc_width", "n_actions", "n_tau", "n_tau_next", "n_tau_act", "kappa", "max_batch"),
    "fb_qnet_create_iqn_dueling": ("fc_width", "n_actions", "n_tau", "n_tau_next", "n_tau_act", "kappa", "max_batch"),
}
ACCEPTED = dict(fc_width=FC, n_actions=2, max_batch=MAXB, n_atoms=51, v_min=-10.0, v_max=10.0, sigma0=0.5, n_quantiles=32, kappa=1.0,
                n_tau=NT, n_tau_next=NT, n_tau_act=NTA)
ACCEPTED_ARCH = {"fb_qnet_create": 0, "fb_qnet_create_c51_noisy": 2, "fb_qnet_create_qr": 4}
GETTERS = {
    "fb_qnet_get_support": (C.c_int, C.c_float, C.c_float),
    "fb_qnet_get_quantiles": (C.c_int, C.c_float),
    "fb_qnet_get_iqn": (C.c_int, C.c_int, C.c_int, C.c_float, C.c_float),
    "fb_qnet_get_iqn_munchausen": (C.c_int, C.c_float, C.c_float, C.c_float),
    "fb_qnet_get_sac": (C.c_float, C.c_float, C.c_float),
    "fb_qnet_get_ac": (C.c_float, C.c_float),
    "fb_qnet_get_ppo": (C.c_float, C.c_float),
    "fb_qnet_get_huber": (C.c_float,),
    "fb_qnet_get_munchausen": (C.c_float, C.c_float, C.c_float),
}


def creator_cases(names):
    """case name -> the arguments it changes (`out`: None = a NULL out)"""
    cases = {"accepted": {}, "out=NULL": {"out": None}}

    def add(**kw):
        cases[",".join(f"{k}={v!r}" for k, v in kw.items())] = kw
    for v in (0, 100, 4224):
        add(fc_width=v)
    for v in (0, 1, 9):
        add(n_actions=v)
    for v in (0, 2 ** 20 + 1):
        add(max_batch=v)
    if "arch" in names:
        for v in range(-1, 11):
            add(arch=v)
    if "n_atoms" in names:
        add(n_atoms=1), add(n_atoms=129), add(n_actions=4, n_atoms=51), add(v_min=10.0, v_max=10.0), add(v_min=20.0), add(v_min=NAN), add(v_max=NAN)
    if "sigma0" in names:
        add(sigma0=-0.5), add(sigma0=NAN)
    if "kappa" in names:
        add(kappa=0.0), add(kappa=NAN)
    if "n_quantiles" in names:
        add(n_quantiles=1), add(n_actions=8, n_quantiles=32)
    for k in ("n_tau", "n_tau_next", "n_tau_act"):
        if k in names:
            add(**{k: 0}), add(**{k: 65})
    return cases


def net_props(lib, h):
    """what an accepted creation left in the handle, as the library's own getters tell it"""
    n = C.c_int64()
    out = {"fb_qnet_num_params": [lib.fb_qnet_num_params(h, C.byref(n)), n.value], "fb_qnet_is_noisy": lib.fb_qnet_is_noisy(h)}
    for name, types in GETTERS.items():
        vals = [t() for t in types]
        rc = getattr(lib, name)(h, *[C.byref(v) for v in vals])
        out[name] = [rc, [v.value for v in vals] if rc == 0 else lib.fb_last_error().decode()]
    return out


def run_creator(lib, creator):
    """every case of one creator -> {case: [rc, text, props or None]}; every created net is destroyed"""
    names, out = CREATORS[creator], {}
    for case, change in creator_cases(names).items():
        args = dict(ACCEPTED, arch=ACCEPTED_ARCH.get(creator))
        args.update(change)
        h = C.c_void_p()
        rc = getattr(lib, creator)(*[args[k] for k in names], None if "out" in change else C.byref(h))
        text = "" if rc == 0 else lib.fb_last_error().decode()
        out[case] = [rc, text, net_props(lib, h) if rc == 0 else None]
        if rc == 0:
            assert lib.fb_qnet_destroy(h) == 0
    return out


# ---------------------------------------------------------------- the IQN entry points
NETS = {"plain": ("plain", {}), "sac": ("sac", {}), "iqn": ("iqn", {}), "iqndueling": ("iqndueling", {}), "iqnmu": ("iqn", {})}
IQN_KW = dict(n_tau=NT, n_tau_next=NT, n_tau_act=NTA)
MEMS = ("uniform", "per", "uniform3")
NET_ENTRIES = ("fb_qnet_iqn_train_step", "fb_qnet_iqn_per_train_step")                                    # (net, double_q)
MEM_ENTRIES = ("fb_iqn_train_from_replay", "fb_iqn_per_train_from_replay", "fb_iqn_step", "fb_iqn_per_step")      # (net, memory, double_q)
STEP_ENTRIES = ("fb_iqn_step", "fb_iqn_per_step")
PER_ENTRIES = ("fb_qnet_iqn_per_train_step", "fb_iqn_per_train_from_replay", "fb_iqn_per_step")
OTHER_ENTRIES = ("fb_qnet_forward_iqn", "fb_qnet_set_iqn_risk", "fb_qnet_set_iqn_munchausen", "fb_iqn_draw_taus")
FAMILY_STEPS = "one_step_of_sac_ac_ppo"
ENTRIES = NET_ENTRIES + MEM_ENTRIES + OTHER_ENTRIES
MU_CASES = ((1, 0.03, 0.9, -1.0), (0, 0.03, 0.9, -1.0), (2, 0.03, 0.9, -1.0), (1, 0.0, 0.9, -1.0), (1, NAN, 0.9, -1.0), (1, 0.03, 1.5, -1.0),
            (1, 0.03, 0.9, 0.5), (1, 0.05, 0.5, -2.0))


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


class World:
    """the nets, the memories (each with an env of its own) and one set of buffers, sized for the largest batch any case passes"""

    def __init__(self, torch):
        from dqnflappybird_amd import _lib as L
        from dqnflappybird_amd.vec import QNet, VecGameState, VecReplay
        self.torch, self.L, self.lib = torch, L, L.lib()
        self.nets, self.seeds = {}, {}
        for k, (name, (arch, kw)) in enumerate(dict(NETS, ac=("ac", {})).items()):
            net = QNet(2, FC, arch, max_batch=MAXB, **(IQN_KW if arch.startswith("iqn") else {}), **kw)
            net.set_hparams(lr=1e-3, eps=1e-4)     # (an update whose size depends on the gradient's, not on its sign alone)
            self.nets[name], self.seeds[name] = net, k + 1
        self.envs, self.mems, self.saved, self.fixed_idx = {}, {}, {}, {}
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
            self.fixed_idx[name] = rep.sample(B)[0].clone()      # B legitimate indices (deque positions, or tree indices of the prioritized one)
            torch.cuda.synchronize()
            self.saved[name] = (rep.state_blob().copy(), env.get_state().copy(), env.nib.clone(), env.frame_bits.clone(), env.reward.clone(),
                                env.terminal.clone(), env.score.clone())
        self.dirty = set(self.nets)                # nets / memories an accepted call has moved: put back before the next call on them
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
        R = 16                                     # rows: above every batch passed (MAXB + 1) and every forward's (3 MAXB + 1)
        self.idx, self.s, self.s2 = z(R, torch.int64), z((R, 80, 80, 4), torch.uint8), z((R, 80, 80, 4), torch.uint8)
        self.a, self.r, self.t = z(R, torch.uint8), z(R, torch.float32), z(R, torch.uint8)
        self.isw, self.isw64, self.abs_err = z(R, torch.float32), z(R, torch.float64), z(R, torch.float32)
        self.isw[:] = 0.5 + 0.25 * torch.arange(R, device="cuda")
        self.loss, self.y, self.actions = z(8, torch.float32), z((R, NT), torch.float32), z(N, torch.uint8)
        self.tau, self.theta, self.draw = z((R, NTA), torch.float32), z((R, NTA, 2), torch.float32), z((2, 2), torch.float32)
        self.tau[:] = (torch.arange(R * NTA, device="cuda").reshape(R, NTA) % 7 + 0.5) / 7.5
        self.adv, self.ret, self.logp, self.val = z(R, torch.float32), z(R, torch.float32), z(R, torch.float32), z(R, torch.float32)
        self.adv[:] = 0.5 - 0.25 * torch.arange(R, device="cuda")
        self.ret[:] = 0.1 * torch.arange(R, device="cuda")
        self.logp[:] = -0.7 + 0.05 * torch.arange(R, device="cuda")
        self.val[:] = 0.05 * torch.arange(R, device="cuda")
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
            net.init_params(seed=self.seeds[netname] + 100, which=L.NET_TARGET)      # (a target of its own: double_q and the target slices show)
            zero = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
            net.set_adam_state(zero, zero, np.array([0.9, 0.999], np.float32))
            if net.arch.startswith("iqn"):
                assert lib.fb_qnet_set_iqn_risk(net.h, 1.0) == 0
                assert lib.fb_qnet_set_iqn_munchausen(net.h, int(netname == "iqnmu"), 0.03, 0.9, -1.0) == 0
            if net.arch == "sac":
                assert lib.fb_qnet_set_sac(net.h, 0.2, 0.98 * math.log(2.0), 0.0) == 0
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
        for x in (self.loss, self.y, self.abs_err, self.a, self.r, self.t, self.theta, self.draw):
            x.zero_()

    def sample(self, mem):
        """the memory's B indices in self.idx (drawn once, when it was filled: every case starts from that memory)"""
        self.idx[:B] = self.fixed_idx[mem]

    def snapshot(self, netname, mem):
        out = [self.nets[netname].store_params(w).clone() for w in (0, 1)]
        if mem is not None:
            blob = np.asarray(self.mems[mem].state_blob())
            out += [len(self.mems[mem]), int(blob[24:32].view(np.int64)[0])]      # (ReplayBlobHeader: the push counter)
        return out

    def same(self, x, y):
        return self.torch.equal(x[0], y[0]) and self.torch.equal(x[1], y[1]) and x[2:] == y[2:]

    def finish(self, rc, what, netname, mem, before, digest):
        """(rc, text, digests of an accepted call's outputs or None); a refused call has left everything as it was"""
        text = "" if rc == 0 else self.lib.fb_last_error().decode()
        self.torch.cuda.synchronize()
        if rc != 0:
            assert self.same(self.snapshot(netname, mem), before), f"{what} refused ({text!r}) and left the memory's counters or the net's parameters changed"
            return [rc, text, None]
        self.dirty.update(x for x in (netname, mem) if x is not None)
        out = {k: sha(v) for k, v in digest.items()}
        out["params"] = sha(self.nets[netname].store_params(0))
        return [rc, text, out]

    # -- one call of a train / step entry point; the argument cases change one argument
    def call(self, entry, netname, mem, dq, case=None):
        L, lib, p = self.L, self.lib, self.L.ptr
        net = self.nets[netname]
        self.fresh(netname, mem)
        if mem is not None:
            self.sample(mem)
        before = self.snapshot(netname, mem)
        rep, env = (self.mems[mem], self.envs[mem]) if mem is not None else (None, None)
        batch = MAXB + 1 if case == "batch" else B
        n_envs = N + 1 if case == "n_envs" else N
        gamma = GAMMA if case != "gamma" else 0.5 if rep is not None and rep.n_step[0] > 1 else 1.5
        loss = None if case == "null" else p(self.loss)
        isw = None if case == "isw" else p(self.isw)
        ae = None if case == "abs_err" else p(self.abs_err)
        if entry == "fb_qnet_iqn_train_step":
            rc = lib.fb_qnet_iqn_train_step(net.h, dq, batch, p(self.s), p(self.ga), p(self.gr), p(self.s2), p(self.gt), None, None, 3, 5, gamma, loss,
                                            p(self.y), None, None)
            digest = {"loss": self.loss, "T": self.y[:B]}
        elif entry == "fb_qnet_iqn_per_train_step":
            rc = lib.fb_qnet_iqn_per_train_step(net.h, dq, batch, p(self.s), p(self.ga), p(self.gr), p(self.s2), p(self.gt), isw, None, None, 3, 5,
                                                gamma, loss, ae, p(self.y), None, None)
            digest = {"loss": self.loss, "T": self.y[:B], "abs_err": self.abs_err[:B]}
        elif entry == "fb_iqn_train_from_replay":
            rc = lib.fb_iqn_train_from_replay(rep.h, net.h, dq, batch, p(self.idx), p(self.a), p(self.r), p(self.t), None, None, 3, 5, gamma, loss,
                                              p(self.y), None, None)
            digest = {"loss": self.loss, "T": self.y[:B], "a": self.a[:B], "r": self.r[:B], "t": self.t[:B]}
        elif entry == "fb_iqn_per_train_from_replay":
            rc = lib.fb_iqn_per_train_from_replay(rep.h, net.h, dq, batch, p(self.idx), isw, p(self.a), p(self.r), p(self.t), None, None, 3, 5, gamma,
                                                  loss, ae, p(self.y), None, None)
            digest = {"loss": self.loss, "T": self.y[:B], "abs_err": self.abs_err[:B], "a": self.a[:B], "r": self.r[:B], "t": self.t[:B]}
        elif entry in STEP_ENTRIES:
            d = lambda x: x.data_ptr()
            sb = L.StepBuffers(d(env.nib), d(self.actions), d(env.frame_bits), d(env.reward), d(env.terminal), d(env.score), d(self.idx), d(self.s),
                               d(self.s2), d(self.a), d(self.t), d(self.r), None if case == "null" else d(self.loss), None, d(self.isw64),
                               None if case == "isw" else d(self.isw), None if case == "abs_err" else d(self.abs_err))
            rc = getattr(lib, entry)(env.h, rep.h, net.h, C.byref(sb), n_envs, dq, batch, 0.1, 3, 5, 1, gamma, None)
            digest = {"loss": self.loss, "a": self.a[:B], "r": self.r[:B], "t": self.t[:B], "actions": self.actions}
            if entry == "fb_iqn_per_step":
                digest["abs_err"] = self.abs_err[:B]
        else:
            raise KeyError(entry)
        return self.finish(rc, f"{entry} ({netname}, {mem}, double_q {dq}, case {case})", netname, mem, before, digest)

    # -- the entry points that take neither a memory nor double_q
    def forward_iqn(self, netname, which=0, batch=B, M=NTA, null=None):
        p, net = self.L.ptr, self.nets[netname]
        self.fresh(netname, None)
        before = self.snapshot(netname, None)
        arg = lambda name, x: None if null == name else p(x)
        rc = self.lib.fb_qnet_forward_iqn(net.h, which, arg("states", self.s), batch, arg("tau", self.tau), M, arg("theta", self.theta), None)
        out = self.finish(rc, f"fb_qnet_forward_iqn ({netname})", netname, None, before, {"theta": self.theta[:B]})
        self.dirty.discard(netname)                # (a forward moves nothing)
        return out

    def setter(self, entry, netname, *args):
        """fb_qnet_set_iqn_risk / _munchausen -> (rc, text, what the getter answers afterwards)"""
        lib, net = self.lib, self.nets[netname]
        self.fresh(netname, None)
        before = self.snapshot(netname, None)
        rc = getattr(lib, entry)(net.h, *args)
        out = self.finish(rc, f"{entry} ({netname}, {args})", netname, None, before, {})
        if rc == 0:
            getter = "fb_qnet_get_iqn" if entry == "fb_qnet_set_iqn_risk" else "fb_qnet_get_iqn_munchausen"
            vals = [t() for t in GETTERS[getter]]
            assert getattr(lib, getter)(net.h, *[C.byref(v) for v in vals]) == 0
            out[2] = {"get": [v.value for v in vals], "fold_q": sha(net.forward(self.s[:B]))}
        return out


def run_entry(w, entry):
    """every case of one entry point -> {case key: [rc, text, digests or None]}"""
    out, lib, p = {}, w.lib, w.L.ptr
    if entry in NET_ENTRIES + MEM_ENTRIES:
        mems = MEMS if entry in MEM_ENTRIES else (None,)
        for net in NETS:
            for mem in mems:
                for dq in (0, 1, 2):
                    out[f"{net}|{mem}|{dq}"] = w.call(entry, net, mem, dq)
        home = None if entry in NET_ENTRIES else "per" if entry in PER_ENTRIES else "uniform3"
        cases = ("null", "batch", "gamma") + (("n_envs",) if entry in STEP_ENTRIES else ()) + (("isw", "abs_err") if entry in PER_ENTRIES else ())
        for case in cases:
            out[f"arg|{case}"] = w.call(entry, "iqn", home, 0, case)
    elif entry == "fb_qnet_forward_iqn":
        for net in NETS:
            for which in (0, 1, 2):
                out[f"{net}|{which}"] = w.forward_iqn(net, which)
        for null in ("states", "tau", "theta"):
            out[f"arg|{null}=NULL"] = w.forward_iqn("iqn", null=null)
        for M in (0, 1, 65):
            out[f"arg|M={M}"] = w.forward_iqn("iqn", M=M)
        out["arg|batch"] = w.forward_iqn("iqn", batch=3 * MAXB + 1)
        out["arg|handle=NULL"] = [lib.fb_qnet_forward_iqn(None, 0, p(w.s), B, p(w.tau), NTA, p(w.theta), None), lib.fb_last_error().decode(), None]
    elif entry == "fb_qnet_set_iqn_risk":
        for net in NETS:
            for eta in (1.0, 0.5, 0.0, 1.5, NAN):
                out[f"{net}|{eta!r}"] = w.setter(entry, net, eta)
        out["arg|handle=NULL"] = [lib.fb_qnet_set_iqn_risk(None, 1.0), lib.fb_last_error().decode(), None]
    elif entry == "fb_qnet_set_iqn_munchausen":
        for net in NETS:
            for args in MU_CASES:
                out[f"{net}|{args!r}"] = w.setter(entry, net, *args)
        out["arg|handle=NULL"] = [lib.fb_qnet_set_iqn_munchausen(None, 1, 0.03, 0.9, -1.0), lib.fb_last_error().decode(), None]
    elif entry == "fb_iqn_draw_taus":
        for batch, n, which, null in ((2, 2, 0, False), (2, 2, 1, False), (2, 2, 2, False), (0, 2, 0, False), (2 ** 20 + 1, 2, 0, False), (2, 0, 0, False),
                                      (2, 65, 0, False), (2, 2, 0, True)):
            w.draw.zero_()
            rc = lib.fb_iqn_draw_taus(batch, n, 3, 5, which, None if null else p(w.draw), None)
            w.torch.cuda.synchronize()
            out[f"{batch}|{n}|{which}|{'NULL' if null else 'out'}"] = [rc, "" if rc == 0 else lib.fb_last_error().decode(), {"tau": sha(w.draw)} if rc == 0 else None]
    else:
        raise KeyError(entry)
    return out


def run_family_steps(w):
    """one accepted ring-fed step of the SAC, the A2C and the PPO call on the one-step uniform memory -> {call: [rc, text, digests]}"""
    lib, p, out = w.lib, w.L.ptr, {}
    for entry, netname in (("fb_sac_train_from_replay", "sac"), ("fb_ac_train_from_replay", "ac"), ("fb_ppo_train_from_replay", "ac")):
        net, rep = w.nets[netname], w.mems["uniform"]
        w.fresh(netname, "uniform")
        w.sample("uniform")
        before = w.snapshot(netname, "uniform")
        if entry == "fb_sac_train_from_replay":
            rc = lib.fb_sac_train_from_replay(rep.h, net.h, B, p(w.idx), p(w.a), p(w.r), p(w.t), GAMMA, p(w.loss), p(w.y), None, None)
            digest = {"loss": w.loss, "T": w.y.reshape(-1)[:B], "a": w.a[:B], "r": w.r[:B], "t": w.t[:B]}
        elif entry == "fb_ac_train_from_replay":
            rc = lib.fb_ac_train_from_replay(rep.h, net.h, B, p(w.idx), p(w.adv), p(w.ret), B, p(w.a), p(w.loss), None, None)
            digest = {"loss": w.loss, "a": w.a[:B]}
        else:
            rc = lib.fb_ppo_train_from_replay(rep.h, net.h, B, p(w.idx), None, p(w.adv), p(w.ret), p(w.logp), p(w.val), B, p(w.a), p(w.loss), None, None)
            digest = {"loss": w.loss, "a": w.a[:B]}
        out[entry] = w.finish(rc, entry, netname, "uniform", before, digest)
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


def same_as_recorded(what, got, want):
    got = json.loads(json.dumps(got))              # (tuples and NaN-free floats as the record holds them)
    assert sorted(got) == sorted(want), f"{what}: the cases run and the recorded ones differ"
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    for k, (g, r) in list(wrong.items())[:10]:
        print(f"{what} {k}:\n  got      {g}\n  recorded {r}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases of {what} answer differently from the record"
    accepted = sum(1 for v in got.values() if v[0] == 0)
    print(f"{what}: {len(got)} cases, {accepted} accepted")
    return accepted


@pytest.mark.parametrize("creator", list(CREATORS))
def test_creator_answers_as_recorded(world, table, creator):
    accepted = same_as_recorded(creator, run_creator(world.lib, creator), table["creators"][creator])
    assert accepted >= 1


@pytest.mark.parametrize("entry", ENTRIES)
def test_iqn_entry_point_answers_and_computes_as_recorded(world, table, entry):
    got = run_entry(world, entry)
    accepted = same_as_recorded(entry, got, table["entries"][entry])
    assert 0 < accepted < len(got)


def test_one_step_of_sac_ac_ppo_computes_as_recorded(world, table):
    accepted = same_as_recorded(FAMILY_STEPS, run_family_steps(world), table[FAMILY_STEPS])
    assert accepted == 3


def record(path):
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    world = World(torch)
    rec = {"creators": {c: run_creator(world.lib, c) for c in CREATORS}, "entries": {e: run_entry(world, e) for e in ENTRIES},
           FAMILY_STEPS: run_family_steps(world)}
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    count = lambda d: (len(d), sum(1 for v in d.values() if v[0] == 0))
    for part in ("creators", "entries"):
        for name, cases in rec[part].items():
            print(f"{name}: {count(cases)[0]} cases, {count(cases)[1]} accepted")
    print(f"{FAMILY_STEPS}: {count(rec[FAMILY_STEPS])} -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_gpu_family_record --record [PATH]")
