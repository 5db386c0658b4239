"""VecSAC: discrete soft actor-critic (Haarnoja et al. 2018; Christodoulou 2019) on the vectorised loop, entirely device resident.

    step:  sample the policy for N envs -> frame_step -> store + draw a minibatch           (vec.SacStep, ONE host call)
           -> [after `observe` steps] the SAC train step on the minibatch, read from the replay ring in place:
              soft target from the target net's two Q heads, both critic losses, the actor's loss, [the temperature's Adam step]
           -> target <- target + polyak (online - target)

One net (a policy head and two Q heads on the shared trunk), one GPU, a uniform memory; include/fbdqn.h pins the semantics, DESIGN.md
section 18 the schedule.  The policy is stochastic: there is no epsilon; evaluate() plays its argmax.

prioritized=True: a prioritized memory (its n fixed at creation) and vec.SacPerStep -- store -> Memory.sample -> the SAC step with the
importance weights on both critic terms -> Memory.batch_update with the mean |critic error|, still one host call.  n_step > 1 (on the
prioritized memory only): the critics' target bootstraps from the state n steps on with gamma^n, on the ring's plain n-step return.
"""
import numpy as np

from .vecloop import DeviceLoop, clip_text, npz_path, refuse_foreign_head, score_text

SAC_HEAD = "sac"                                             # what a checkpoint of this class records as its head


def check_args(n_envs, batch, alpha, target_entropy, alpha_lr, polyak, observe, gamma, lr, max_grad_norm, capacity):
    """every argument check of VecSAC that needs no GPU -> the checked values"""
    from .vec import check_gamma, check_lr, check_max_grad_norm, check_n_envs, check_observe, check_polyak, check_ring_batch, check_sac, ring_capacity
    n = check_n_envs(n_envs)
    b = check_ring_batch(batch, n)
    a, h, alr = check_sac(alpha, target_entropy, alpha_lr, 2)
    rho = check_polyak(polyak, allow_off=True)
    ob = check_observe(observe)
    g, l = check_gamma(gamma), check_lr(lr)
    cap = ring_capacity(capacity, n)
    if cap < 2 * n:
        raise ValueError(f"capacity {cap} < 2 x n_envs = {2 * n}")
    return n, b, a, h, alr, rho, ob, g, l, check_max_grad_norm(max_grad_norm), cap


def check_replay(prioritized, n_step, n_envs, observe, capacity):
    """VecSAC's memory settings, checked apart from check_args (whose positional parameters stay as they are) and behind it (n_envs,
    observe, capacity: its checked values) -> (prioritized, n_step)"""
    from . import _lib as L
    if not isinstance(prioritized, (bool, np.bool_)):
        raise ValueError(f"prioritized must be True or False, got {prioritized!r}")
    ns = int(n_step)
    if not 1 <= ns <= L.NSTEP_MAX:
        raise ValueError(f"n_step must be in 1..{L.NSTEP_MAX}, got {n_step}")
    if ns > 1 and not prioritized:
        raise ValueError(f"n_step = {ns} needs prioritized=True: n-step SAC runs on the prioritized memory only (a uniform n-step view is "
                         "served by VecReplay.gather and QNet.sac_train_step with gamma^n)")
    if observe < ns - 1:
        raise ValueError(f"observe must be >= n_step - 1 = {ns - 1}: the first n_step - 1 steps only store (no n-step transition is complete yet), got {observe}")
    if capacity < max(2, ns) * n_envs:
        raise ValueError(f"capacity {capacity} < max(2, n_step) x n_envs = {max(2, ns) * n_envs}")
    return bool(prioritized), ns


def replay_kind(prioritized):
    return "prioritized" if prioritized else "uniform"


class VecSAC(DeviceLoop):
    prioritized, n_step = False, 1                           # (a uniform loop at n-step 1 unless __init__ says otherwise)

    def __init__(self, n_envs, batch=32, alpha=0.2, target_entropy=None, alpha_lr=0.0, polyak=0.005, observe=100, gamma=0.99, lr=1e-4,
                 max_grad_norm=0, fc_width=512, seed=0, capacity=None, prioritized=False, n_step=1):
        """n_envs games; every step trains one minibatch of `batch` transitions (<= n_envs, <= 256) once `observe` steps have filled
        the memory.  alpha: the temperature (its start when alpha_lr > 0, which learns it towards the entropy target_entropy, default
        0.98 ln 2); polyak: the soft target update's rate per step (0 = never); lr is Adam's; max_grad_norm=G > 0 clips the gradient's
        global norm; capacity: the memory's (default max(65536, 8 n_envs)).  prioritized: train from a prioritized memory (importance-
        weighted critic losses, the mean |critic error| as the priority); n_step > 1, with prioritized only: n-step returns, the first
        n_step - 1 steps store only."""
        (self.n, self.batch, self.alpha, self.target_entropy, self.alpha_lr, self.polyak, self.observe, self.gamma, self.lr, self.max_grad_norm,
         self.capacity) = check_args(n_envs, batch, alpha, target_entropy, alpha_lr, polyak, observe, gamma, lr, max_grad_norm, capacity)
        self.prioritized, self.n_step = check_replay(prioritized, n_step, self.n, self.observe, self.capacity)
        self.seed = int(seed)
        self.fc_width = int(fc_width)
        self._build_world("sac", max(self.n, self.batch), lambda net: net.set_sac(self.alpha, self.target_entropy, self.alpha_lr),
                          prioritized=self.prioritized, n_step=self.n_step)
        self._bind()
        self.timeStep = 0                                    # env steps per env so far: the key of the policy's draws

    def _bind(self):
        from .vec import SacPerStep, SacStep
        self.one_step = (SacPerStep if self.prioritized else SacStep)(self.env, self.replay, self.net, self.batch, self.gamma, self.polyak)
        self.losses = self.one_step.loss

    def step(self):
        """one vector step -> the six loss numbers f32[6] (device): total, Q1's, Q2's, the actor's, the entropy, alpha.  (observe >=
        n_step - 1: the steps before an n-step transition is complete are among the store-only ones)"""
        self.one_step(seed=self.seed, step=self.timeStep, train=self.timeStep >= self.observe)
        self.timeStep += 1
        return self.losses

    # ------------------------------------------------------------------ checkpoint / resume
    def save(self, path):
        """everything the loop needs to continue bit for bit: the nets, Adam, the temperature's five words, every env's state and frame
        stack, the stats, the memory (with its generator), the counters and the settings; `head` = 'sac' tells the file from the other
        loops'; a prioritized loop adds `prioritized` and `n_step` (and its memory's blob holds the tree) -- a uniform one's file is key
        for key what it was before the prioritized loop existed, and a file without the two keys is a uniform one's at n-step 1"""
        own = dict(prioritized=np.array([1], np.int64), n_step=np.array([self.n_step], np.int64)) if self.prioritized else {}
        self._save(path, SAC_HEAD, sac_state=self.net.sac_state(),
                   scalars=np.array([self.timeStep, self.seed, self.n, self.batch, self.fc_width, self.observe], np.int64),
                   sac=np.array([self.gamma, self.target_entropy, self.alpha_lr, self.polyak, self.max_grad_norm, self.lr], np.float64), **own)

    def load(self, path):
        """the inverse of save(), into a VecSAC made with the same n_envs, batch, fc_width, capacity, seed, memory kind (prioritized or
        not) and n_step; the settings of the file replace this object's"""
        import torch
        z = np.load(npz_path(path))
        refuse_foreign_head(z, path, lambda head: head != SAC_HEAD and f"a {head} head (another loop's), this is a VecSAC (head {SAC_HEAD!r})")
        per = bool(int(z["prioritized"][0])) if "prioritized" in z.files else False
        if per != self.prioritized:
            raise ValueError(f"checkpoint {path} was written by a VecSAC with a {replay_kind(per)} memory, this VecSAC has a "
                             f"{replay_kind(self.prioritized)} one (prioritized={self.prioritized})")
        ns = int(z["n_step"][0]) if "n_step" in z.files else 1
        if ns != self.n_step:
            raise ValueError(f"checkpoint {path} was written with n_step = {ns}, this VecSAC has n_step = {self.n_step}")
        sc = [int(x) for x in z["scalars"]]
        if (sc[2], sc[3], sc[4]) != (self.n, self.batch, self.fc_width):
            raise ValueError(f"checkpoint {path} was written with (n_envs, batch, fc_width) = {tuple(sc[2:5])}, this VecSAC has "
                             f"{(self.n, self.batch, self.fc_width)}")
        if sc[1] != self.seed:
            raise ValueError(f"checkpoint {path} was written with seed {sc[1]}, this VecSAC has seed {self.seed} (the envs' pipe-gap "
                             "streams are keyed by it)")
        self._restore(z)
        self.gamma, self.target_entropy, self.alpha_lr, self.polyak, self.max_grad_norm, self.lr = (float(x) for x in z["sac"])
        self.net.set_hparams(lr=self.lr)
        self.net.set_max_grad_norm(self.max_grad_norm)
        st = np.asarray(z["sac_state"], np.float32)
        self.net.set_sac(float(np.exp(st[0])), self.target_entropy, self.alpha_lr)
        self.net.set_sac_state(st)                           # (the five words as they were: log alpha is not re-derived)
        self.alpha = self.net.sac()[0]
        self.observe = sc[5]
        self.timeStep = sc[0]
        self._bind()
        torch.cuda.synchronize()

    def run(self, steps, log_every=1000):
        for i in range(steps):
            losses = self.step()
            if log_every and (i + 1) % log_every == 0:
                tot, q1, q2, lpi, ent, alpha = losses.tolist()   # the only host sync of the loop, once per log line
                score, clip = score_text(self.net, self.stats), clip_text(self.net, self.max_grad_norm)
                print(f"TIMESTEP {self.timeStep} / ENVS {self.n} / Q_LOSS {q1 + q2:.6g} / POLICY_LOSS {lpi:.6g} / ENTROPY {ent:.6g} / "
                      f"ALPHA {alpha:.6g} / {score} / LOSS {tot:.6g}{clip}", flush=True)
