"""What the vectorised loops (VecBrain, VecIQN, VecSAC, VecActorCritic) share on the host, written once: the checkpoint core, the refusal
of another loop's file, the score and clip pieces of the log line and, for the three loops of one net on one GPU, the construction of
the device world and evaluate().  Every loop keeps its own step() / update(), its own settings and its own checkpoint keys.
"""


def npz_path(path):
    """the file np.savez writes for `path`"""
    return path if str(path).endswith(".npz") else str(path) + ".npz"


def to_device(x):
    """a checkpoint's array -> a tensor on the GPU"""
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


# ------------------------------------------------------------------ checkpoints
LOCAL_ARRAYS = ("env_state", "nib", "stats", "replay")       # of core_arrays: what differs per rank where a loop runs data parallel


def checkpoint_head(z):
    """the head a checkpoint holds: its recorded `head`, else 'c51' where it records a support, else 'scalar'"""
    if "head" in z.files:
        return str(z["head"][0])
    return "c51" if "support" in z.files else "scalar"


def refuse_foreign_head(z, path, foreign):
    """the "this file belongs to another loop" refusal -> the checkpoint's head.  foreign(head): what the message says after
    "checkpoint {path} holds " where the head is another loop's, a false value where this loop loads it"""
    head = checkpoint_head(z)
    told = foreign(head)
    if told:
        raise ValueError(f"checkpoint {path} holds {told}")
    return head


def core_arrays(net, env, nib, stats, replay):
    """what every loop's checkpoint holds: both nets and Adam's slots (net None: left out -- VecBrain's ranks > 0 write their local
    state only), every env's state, the agents' frame stacks (nib None, a backend that tracks none: left out), the stats and the memory"""
    import numpy as np
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    out = {}
    if net is not None:
        m, v, pows = net.adam_state()
        out.update(online=host(net.store_params(0)), target=host(net.store_params(1)), adam_m=host(m), adam_v=host(v),
                   beta_pows=np.asarray(pows, np.float32))
    out.update(env_state=env.get_state(), stats=host(stats), replay=replay.state_blob())
    if nib is not None:
        out["nib"] = host(nib)
    return out


def restore_core(z, net, env, nib, stats, replay, dev, local=None):
    """the inverse of core_arrays from an opened checkpoint; dev: array -> what the net and the tracked buffers take;
    local: the file that holds the envs, frame stacks, stats and memory where that is not z (VecBrain at world > 1)"""
    zl = z if local is None else local
    net.load_params(z["online"], 0)
    net.load_params(z["target"], 1)
    net.set_adam_state(dev(z["adam_m"]), dev(z["adam_v"]), z["beta_pows"])
    env.set_state(zl["env_state"])
    if nib is not None:
        nib.copy_(dev(zl["nib"]))
    stats[...] = dev(zl["stats"])
    replay.load_state_blob(zl["replay"])


# ------------------------------------------------------------------ the log line
def score_text(net, stats):
    """GAME_TIMES ... PIPES of a log line.  Reading the stats is the only host sync of a loop, once per log line; at the same sync an
    activation beyond the two-plane fp16 range raises (check_range)"""
    ep, ssum, smax, pipes = stats.tolist()
    if hasattr(net, "check_range"):
        net.check_range()
    return f"GAME_TIMES {ep} / MEAN_SCORE {ssum / max(ep, 1):.3f} / MAX_SCORE {smax} / PIPES {pipes}"


def clip_text(net, max_grad_norm):
    """the log line's suffix under gradient clipping: the last train step's norm and scale (a synchronous read, at the log cadence only)"""
    if not max_grad_norm:
        return ""
    norm, scale = net.grad_norm()
    return f" / GRAD_NORM {norm:.6g} / CLIP_SCALE {scale:.6g}"


# ------------------------------------------------------------------ one net, one GPU
class DeviceLoop:
    """What VecIQN, VecSAC and VecActorCritic share.  A subclass checks its arguments, sets n, seed, fc_width, capacity, gamma, lr and
    max_grad_norm, calls _build_world and binds its step; its save() / load() add their own keys around _save / _restore."""

    def _build_world(self, arch, max_batch, setup, target_seed=None, prioritized=False, n_step=1, **net_kw):
        """env, replay, net, nib and stats, from nothing to the first observation.  setup(net): the family's own setters;
        target_seed None: the target net starts as a copy of the online net, else from a draw of its own;
        prioritized: a prioritized memory (its n fixed at creation); n_step > 1 on a uniform one: its n-step view"""
        from .vec import QNet, VecGameState, VecReplay
        self.env = VecGameState(self.n, seed=self.seed)
        if prioritized:
            self.replay = VecReplay(self.capacity, self.n, prioritized=True, n_step=n_step, gamma=self.gamma)
        else:
            self.replay = VecReplay(self.capacity, self.n)
        self.replay.seed(self.seed)
        if n_step > 1 and not prioritized:
            self.replay.set_n_step(n_step, self.gamma)
        self.net = QNet(2, self.fc_width, arch, max_batch=max_batch, **net_kw)
        self.net.set_hparams(lr=self.lr)
        setup(self.net)
        if self.max_grad_norm:
            self.net.set_max_grad_norm(self.max_grad_norm)
        self.net.init_params(seed=self.seed, which=0)
        if target_seed is None:
            self.net.sync_target()
        else:
            self.net.init_params(seed=target_seed, which=1)
        self.nib = self.env.track_state()
        self.env.observe()
        self.replay.reset(self.env.frame_bits)
        self.stats = self.env.track_stats()

    def evaluate(self, n_envs=4096, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0):
        """Greedy play of n_envs fresh games with the net as it stands (dqnflappybird_amd.evaluate): the argmax of the policy, or of
        IQN's folded head under the net's risk setting.  Changes nothing the training that follows reads"""
        from .evaluate import evaluate
        return evaluate(self.net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed)

    def _save(self, path, head, **own):
        import numpy as np
        np.savez(npz_path(path), head=np.array([head]), **core_arrays(self.net, self.env, self.nib, self.stats, self.replay), **own)

    def _restore(self, z):
        restore_core(z, self.net, self.env, self.nib, self.stats, self.replay, to_device)
