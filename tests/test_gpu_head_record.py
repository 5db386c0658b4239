"""What the head, acting and train-step kernels of the net families compute, pinned to a record, and the one epsilon rule of all families.

tests/golden/head_record.json was written ONCE, on an MI355X, with the library of commit c2a3a46 -- the parent of the commit that moved
the families' shared device code (the row head, Adam's tick, the row-to-slice lookup) into csrc/fb_head.h and csrc/fb_policy.h.  It is a
record, not a reference to regenerate: that refactor, and every later one of this device code (the policy draw and the gradient tile's
prologue still stand once per family), must reproduce every digest.  The kernels have no atomics and a fixed summation order, so the digests are reproducible on one kind
of GPU (the record's: MI355X).  `FB_LIB=<that commit's libfbdqn.so> python -m tests.test_gpu_head_record --record [PATH]` writes it.

tests/test_gpu_family_record.py covers train steps at 2 actions and fc_width 128 only; this record covers the acting and forward kernels
too, both action templates -- 2 (AT = 2) and 3 (AT = MAXA, masked columns live) -- and fc_width 128 (one round of the row head, lanes
32 .. 63 idle) and 512 (two rounds).  Head and acting calls take 5 rows (one full and one partial workgroup of 4 waves); train steps take
batches of 3 and 17 (the gradient tile's prologue strides the samples by 16: at 17 its row 0 takes a second turn).

- Every case starts from a defined state: init_params(seed), sync_target, a target net initialised with a seed of its own, zeroed Adam
  slots, beta powers reset, the family's settings.  The states come from a seeded env, every other input from a formula.
- Digests: SHA-256 of the raw bytes of every output -- logits / values / log-probabilities / actions / theta / Q of the head calls; of the
  train steps the loss words, the target, abs_err, the exported flat_grad, the beta powers, and the online parameters after a fused step.
  The exported-gradient form runs twice in a row without an apply in between: the second pass re-uses Adam's tick (ticks == applies).
- The epsilon rule: on nets whose head parameters are zero every action has the same Q, so the greedy pick is the FIRST maximum, 0; the
  Philox word of (seed, row, step) is computed here on the host, and the plain, C51, QR and IQN nets must take the random branch on the
  same rows and draw the same action there.
- The policy draw: on actor-critic and SAC nets with zero heads the logits tie, greedy acting must take action 0, and a sampled action
  must be the one the host's Philox word and the float32 cumulative sum of 1 / A give, on both nets.
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
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_record.json")
SHAPES = [(2, 128), (3, 128), (2, 512), (3, 512)]          # (actions, fc_width)
ROWS, BATCHES, NENV, MAXB, GAMMA = 5, (3, 17), 17, 32, 0.99
SEED, STEP = 4, 5                                          # rows 1, 2, 4 of 5 take the random branch at epsilon 0.5, rows 0 and 3 do not
NT, NTN, NTA = 3, 2, 4                                     # n_tau, n_tau_next, n_tau_act
F32 = np.float32
NET_KW = {"c51": dict(n_atoms=21, v_min=-5.0, v_max=5.0), "qr": dict(n_quantiles=16, kappa=1.0),
          "iqn": dict(n_tau=NT, n_tau_next=NTN, n_tau_act=NTA), "iqndueling": dict(n_tau=NT, n_tau_next=NTN, n_tau_act=NTA)}
NETS = ("ac", "sac", "iqn", "iqndueling", "plain", "c51", "qr")
ACT_NETS = ("plain", "c51", "qr", "iqn")                   # the families of the epsilon rule


def sha(t):
    a = t if isinstance(t, np.ndarray) else t.detach().contiguous().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def philox(k0, k1, c0, c1, c2, c3):
    """Philox4x32-10 as csrc/fb_common.h writes it -> (x, y, z, w)"""
    M = 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & M, p1 & M, ((p0 >> 32) ^ c3 ^ k1) & M, p0 & M
        k0, k1 = (k0 + 0x9E3779B9) & M, (k1 + 0xBB67AE85) & M
    return c0, c1, c2, c3


def eps_draw(row, epsilon, A, seed=SEED, step=STEP):
    """the epsilon rule on the host: (random branch taken, randrange(A)'s draw) of `row` on FB_STREAM_EPS = 1"""
    o = philox(seed & 0xFFFFFFFF, seed >> 32, row, step & 0xFFFFFFFF, 1, step >> 32)
    u = F32(o[0] >> 8) * F32(2.0 ** -24)
    return bool(u <= F32(epsilon)), (o[1] * A) >> 32


class World:
    """the inputs every case shares: 17 states s / s' and 5 nibble states of a seeded env, and the per-sample arrays"""

    def __init__(self, torch):
        from dqnflappybird_amd import _lib as L
        from dqnflappybird_amd.vec import VecGameState, VecReplay
        self.torch, self.L, self.lib = torch, L, L.lib()
        env = VecGameState(NENV, seed=1)
        env.track_state()
        env.observe()
        rep = VecReplay(512, NENV)
        rep.seed(1)
        rep.reset(env.frame_bits)
        act = torch.zeros(NENV, dtype=torch.uint8, device="cuda")
        for t in range(6):
            act[:] = t % 3 == 0
            act[t::4] ^= 1                         # (the envs do not all fly the same path)
            _, rew, term, _ = env.frame_step(act)
            rep.push(env.frame_bits, act, rew, term)
            if t == 3:
                self.s = rep.current_state().clone()
        self.s2 = rep.current_state().clone()
        self.nib = env.nib[:ROWS].clone()
        self.env, self.rep = env, rep
        self.idx = rep.sample(NENV)[0].clone()     # legitimate positions of the memory, for the ring-fed PPO call
        i = torch.arange(NENV, device="cuda")
        f = lambda x: x.to(torch.float32)
        self.r, self.t = f(0.1 + 0.9 * (i % 2)), (i % 3 == 0).to(torch.uint8)
        self.adv, self.ret = f(0.5 - 0.25 * (i % 5)), f(0.1 * i)
        self.logp, self.val, self.isw = f(-0.7 + 0.05 * (i % 7)), f(0.05 * i), f(0.5 + 0.25 * (i % 4))
        self.sel = ((i * 7 + 3) % NENV).to(torch.int64)
        self.tau = f((torch.arange(ROWS * NTA, device="cuda").reshape(ROWS, NTA) % 7 + 0.5) / 7.5).contiguous()
        torch.cuda.synchronize()

    def net(self, arch, A, FC):
        from dqnflappybird_amd.vec import QNet
        net = QNet(A, FC, arch, max_batch=MAXB, **NET_KW.get(arch, {}))
        net.set_hparams(lr=1e-3, eps=1e-4)         # (an update whose size depends on the gradient's, not on its sign alone)
        return net

    def fresh(self, net, seed, mu=False):
        """the state every case starts from"""
        torch, L = self.torch, self.L
        net.init_params(seed=seed)
        net.sync_target()
        net.init_params(seed=seed + 100, which=L.NET_TARGET)      # (a target of its own: double_q and the target rows show)
        zero = torch.zeros(net.n_params, dtype=torch.float32, device="cuda")
        net.set_adam_state(zero, zero, np.array([0.9, 0.999], F32))
        if net.arch.startswith("iqn"):
            net.set_iqn_risk(1.0)
            net.set_iqn_munchausen(bool(mu), 0.03, 0.9, -1.0)
        if net.arch == "sac":
            net.set_sac(0.2, 0.98 * math.log(net.A), 1e-3)       # alpha_lr > 0: the fused step makes the temperature's step too
        if net.arch == "ac":
            net.set_ac(0.5, 0.01)
            net.set_ppo(0.2, 0.3)

    def actions(self, A, B):
        return (self.torch.arange(B, device="cuda") % A).to(self.torch.uint8)


def digests(**outs):
    return {k: sha(v) for k, v in outs.items() if v is not None}


def head_cases(w, nets, A):
    """the forward and acting calls on 5 rows -> {case: {output: digest}}"""
    torch, L, lib, p = w.torch, w.L, w.lib, w.L.ptr
    s, nib, out = w.s[:ROWS], w.nib, {}
    for k, name in enumerate(NETS):
        w.fresh(nets[name], k + 1)
    ac, sac = nets["ac"], nets["sac"]
    z, v = ac.forward_ac(s)
    out["ac|forward_ac"] = digests(logits=z, value=v)
    out["ac|value_only"] = digests(value=ac.act_policy_nib(nib, SEED, STEP, value_only=True))
    for net in (ac, sac):
        for greedy in (False, True):
            for logits in (False, True):
                r = net.act_policy_nib(nib, SEED, STEP, greedy=greedy, want_logits=logits)
                out[f"{net.arch}|act_policy|greedy={greedy}|logits={logits}"] = digests(actions=r[0], value=r[1], logp=r[2], logits=r[3] if logits else None)
    for greedy in (0, 1):                          # SAC's acting call with the action alone (what fb_sac_step asks for)
        a = torch.full((ROWS,), 255, dtype=torch.uint8, device="cuda")
        assert lib.fb_qnet_act_policy_nib(sac.h, p(nib), ROWS, SEED, STEP, greedy, p(a), None, None, None, L.current_stream()) == 0
        out[f"sac|act_policy|greedy={bool(greedy)}|actions only"] = digests(actions=a)
    for which in (L.NET_ONLINE, L.NET_TARGET):
        zz, q1, q2 = sac.forward_sac(s, which)
        out[f"sac|forward_sac|{which}"] = digests(logits=zz, q1=q1, q2=q2)
        for name in ("iqn", "iqndueling"):
            out[f"{name}|forward_iqn|{which}"] = digests(theta=nets[name].forward_iqn(s, w.tau, which))
    for name in ACT_NETS:
        for eps in (0.0, 0.5, 1.0):
            a, q = nets[name].act_nib(nib, eps, SEED, STEP, want_q=True)
            out[f"{name}|act_nib|{eps}"] = digests(actions=a, q=q)
    return out


def twice_exported(w, net, step):
    """two gradient passes in a row into flat_grad, no apply in between: the second re-uses Adam's tick"""
    g = w.torch.zeros(net.n_params, dtype=w.torch.float32, device="cuda")
    out = {}
    for n in (1, 2):
        g.zero_()
        res = step(g)
        out.update({f"{k}{n}": v for k, v in digests(**res, flat_grad=g, pows=net.adam_state()[2]).items()})
    return out


def train_cases(w, nets, A, B):
    """the train steps at batch B -> {case: {output: digest}}"""
    torch, L, lib, p = w.torch, w.L, w.lib, w.L.ptr
    s, s2, r, t, a = w.s[:B], w.s2[:B], w.r[:B], w.t[:B], w.actions(A, B)
    adv, ret, lp, vo, isw = w.adv[:B], w.ret[:B], w.logp[:B], w.val[:B], w.isw[:B]
    out, ac, sac = {}, nets["ac"], nets["sac"]
    params = lambda net: net.store_params(0)
    steps = {"ac": lambda g: dict(loss=ac.ac_train_step(s, a, adv, ret, flat_grad=g)),
             "ppo": lambda g: dict(loss=ac.ppo_train_step(s, a, adv, ret, lp, vo, flat_grad=g))}
    for name, step in steps.items():
        w.fresh(ac, 1)
        out[f"{name}|fused|{B}"] = digests(**step(None), params=params(ac), pows=ac.adam_state()[2])
        w.fresh(ac, 1)
        out[f"{name}|exported|{B}"] = twice_exported(w, ac, step)
    for sel in (None, w.sel[:B] % B):              # the ring-fed PPO call: the rollout's buffers read at b, or at sel[b]
        w.fresh(ac, 1)
        loss, a_out = torch.zeros(6, dtype=torch.float32, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
        rc = lib.fb_ppo_train_from_replay(w.rep.h, ac.h, B, p(w.idx[:B]), p(sel), p(adv), p(ret), p(lp), p(vo), B, p(a_out), p(loss), None, L.current_stream())
        assert rc == 0, lib.fb_last_error().decode()
        out[f"ppo|ring|sel={sel is not None}|{B}"] = digests(loss=loss, a=a_out, params=params(ac))
    sac_step = lambda g: dict(zip(("loss", "T"), sac.sac_train_step(s, a, r, s2, t, GAMMA, flat_grad=g)))
    w.fresh(sac, 2)
    out[f"sac|fused|{B}"] = digests(**sac_step(None), params=params(sac), temperature=sac.sac_state())
    w.fresh(sac, 2)
    out[f"sac|exported|{B}"] = twice_exported(w, sac, sac_step)
    for k, (name, mu) in enumerate((("iqn", False), ("iqndueling", False), ("iqn", True))):
        net = nets[name]
        for dq in (False,) if mu else (False, True):       # (Munchausen refuses double_q)
            key = f"{name}{'|mu' if mu else ''}|dq={dq}|{B}"
            uni = lambda g: dict(zip(("loss", "T"), net.iqn_train_step(s, a, r, s2, t, GAMMA, dq, seed=SEED, step=STEP, flat_grad=g)))
            per = lambda g: dict(zip(("loss", "abs_err", "T"), net.iqn_per_train_step(s, a, r, s2, t, isw, GAMMA, dq, seed=SEED, step=STEP, flat_grad=g)))
            for form, step in (("uniform", uni), ("per", per)):
                w.fresh(net, 3 + k, mu)
                out[f"{key}|{form}|fused"] = digests(**step(None), params=params(net))
            w.fresh(net, 3 + k, mu)
            out[f"{key}|uniform|exported"] = twice_exported(w, net, uni)
    return out


def run_shape(w, A, FC):
    nets = {name: w.net(name, A, FC) for name in NETS}
    out = head_cases(w, nets, A)
    for B in BATCHES:
        out.update(train_cases(w, nets, A, B))
    w.torch.cuda.synchronize()
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


@pytest.mark.parametrize("A,FC", SHAPES)
def test_heads_and_train_steps_compute_as_recorded(world, table, A, FC):
    got, want = run_shape(world, A, FC), table[f"A={A}|FC={FC}"]
    assert sorted(got) == sorted(want), "the cases run and the recorded ones differ"
    wrong = {k: sorted(o for o in got[k] if got[k][o] != want[k].get(o)) for k in got if got[k] != want[k]}
    for k, outs in list(wrong.items())[:20]:
        print(f"A={A} FC={FC} {k}: differs from the record in {outs}")
    assert not wrong, f"{len(wrong)} of {len(got)} cases compute other bits than the record"
    print(f"A={A} FC={FC}: {len(got)} cases, {sum(len(v) for v in got.values())} digests")


@pytest.mark.parametrize("A", (2, 3))
def test_every_family_takes_the_first_maximum_and_the_same_epsilon_draw(world, A):
    torch, FC = world.torch, 128
    plain = world.net("plain", A, FC)
    trunk = plain.n_params - FC * A - A            # conv1 .. b_fc1: everything behind it is a family's head
    want = [eps_draw(row, 0.5, A) for row in range(ROWS)]
    assert {b for b, _ in want} == {False, True} and any(b and d != 0 for b, d in want), "the seed must show both branches and a draw other than 0"
    seen = {}
    for k, name in enumerate(ACT_NETS):
        net = plain if name == "plain" else world.net(name, A, FC)
        world.fresh(net, k + 1)
        flat = net.store_params(0)
        flat[trunk:] = 0.0                         # every action the same Q: more than one maximum in every row
        net.load_params(flat)
        for eps in (0.0, 0.5, 1.0):
            a, q = net.act_nib(world.nib, eps, SEED, STEP, want_q=True)
            a, q = a.cpu().numpy().tolist(), q.cpu().numpy()
            assert (q == q[:, :1]).all(), f"{name}: the Q row is not constant"
            draws = [eps_draw(row, eps, A) for row in range(ROWS)]
            assert a == [d if b else 0 for b, d in draws], f"{name} at epsilon {eps}: {a}, the host's Philox word gives {draws}"
            seen[name, eps] = a
    for eps in (0.0, 0.5, 1.0):
        assert len({tuple(seen[name, eps]) for name in ACT_NETS}) == 1
    assert seen["plain", 0.0] == [0] * ROWS and seen["plain", 0.5] != seen["plain", 1.0]


@pytest.mark.parametrize("A", (2, 3))
def test_both_policy_draws_take_the_first_maximum_and_the_same_sampled_action(world, A):
    """tied logits (zero heads) on an actor-critic and a SAC net: greedy acting takes action 0; a sampled action is the first c whose
    cumulated float32 probability exceeds the host's Philox word on FB_STREAM_POLICY = 8, the same on both nets"""
    FC = 128
    trunk = world.net("plain", A, FC).n_params - FC * A - A
    p = F32(1.0) / (F32(1.0) * F32(A))             # softmax of equal logits: e_c = 1, s = A
    want = []
    for row in range(ROWS):
        o = philox(SEED & 0xFFFFFFFF, SEED >> 32, row, STEP & 0xFFFFFFFF, 8, STEP >> 32)
        u, cum, act = F32(o[0] >> 8) * F32(2.0 ** -24), F32(0.0), A - 1
        for c in range(A):
            cum = F32(cum + p)
            if u < cum:
                act = c
                break
        want.append(act)
    assert len(set(want)) > 1, "the seed must show more than one sampled action"
    for k, name in enumerate(("ac", "sac")):
        net = world.net(name, A, FC)
        world.fresh(net, k + 1)
        flat = net.store_params(0)
        flat[trunk:] = 0.0
        net.load_params(flat)
        a, _, logp, z = net.act_policy_nib(world.nib, SEED, STEP, greedy=True, want_logits=True)
        assert (z == 0).all().item() and a.cpu().tolist() == [0] * ROWS, f"{name}: greedy acting on tied logits took {a.cpu().tolist()}"
        assert np.allclose(logp.cpu().numpy(), -math.log(A), atol=1e-6)
        a = net.act_policy_nib(world.nib, SEED, STEP, greedy=False)[0]
        assert a.cpu().tolist() == want, f"{name}: sampled {a.cpu().tolist()}, the host's Philox word gives {want}"


def record(path):
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    world = World(torch)
    rec = {f"A={A}|FC={FC}": run_shape(world, A, FC) for A, FC in SHAPES}
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    for k, v in rec.items():
        print(f"{k}: {len(v)} cases, {sum(len(o) for o in v.values())} digests")
    print(f"library {_lib.LIB_PATH} -> {path}")


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        record(sys.argv[2] if len(sys.argv) > 2 else TABLE)
    else:
        sys.exit("usage: python -m tests.test_gpu_head_record --record [PATH]")
