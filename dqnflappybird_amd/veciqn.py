"""VecIQN: implicit quantile networks (Dabney, Ostrovski, Silver & Munos 2018) on the vectorised loop, entirely device resident.

    step:  epsilon-greedy on the folded head for N envs -> frame_step -> store + draw a minibatch      (vec.IqnStep, ONE host call)
           -> [after `observe` steps] the IQN train step on the minibatch, read from the replay ring in place:
              a* from the folded head of the target (or, double_q, the online) net, the target quantiles at sampled tau', the online
              quantiles at sampled tau, the pairwise quantile Huber loss
           -> the target net: copied every replace_target_iter steps, or target += polyak (online - target) every train step

One net, one GPU, a uniform memory at any n-step view; include/fbdqn.h pins the semantics, DESIGN.md section 19 the design.  Acting costs
what a plain net's does: the mean over the acting grid of tau folds into the head (QNet.set_iqn_risk scales the grid: CVaR).

prioritized=True: a prioritized memory (its n fixed at creation) and vec.IqnPerStep -- store -> Memory.sample -> the IQN step with the
importance weights -> Memory.batch_update with the per-sample loss, still one host call.  With double_q and n_step = 3: "Rainbow-IQN"
without the dueling and the noisy head.

dueling=True: the dueling IQN net (QNet arch 'iqndueling': value and advantage quantile streams, one effective column per action) in the
same loops; with prioritized, double_q and n_step = 3 this is Rainbow-IQN without noisy nets.

munchausen=True: Munchausen IQN (Vieillard, Pietquin & Geist 2020) -- the target becomes the soft value under softmax(Qbar- / temp) of the
target net plus the clipped log-policy bonus alpha max(temp ln pi-(a|s), clip) on the reward (QNet.set_iqn_munchausen); everything else,
the memory kinds, the dueling net, n-step returns and CVaR acting included, is unchanged.  It has no greedy next action: double_q is refused.

noisy=True: noisy IQN (Fortunato et al. 2018) -- fc1 and the head layers are factorised Gaussian layers at sigma0 (QNet archs 'iqnnoisy' /
'iqnduelingnoisy'), the step draws the nets' noise, and the epsilon schedule defaults to 0.  acting_noise='shared': one sample per step for
all envs; 'env': independent noise per env when acting.  With prioritized, dueling, double_q and n_step = 3: full Rainbow-IQN (Toromanoff et
al. 2019).
"""
import numpy as np

from .vecloop import DeviceLoop, clip_text, npz_path, refuse_foreign_head, score_text

IQN_HEAD = "iqn"                                             # what a checkpoint of this class records as its head


def check_args(n_envs, batch, n_tau, n_tau_next, n_tau_act, kappa, cvar, n_step, polyak, replace_target_iter, observe, explore, initial_epsilon,
               final_epsilon, gamma, lr, max_grad_norm, capacity):
    """every argument check of VecIQN that needs no GPU -> the checked values"""
    from . import _lib as L
    from .vec import check_gamma, check_iqn, check_lr, check_max_grad_norm, check_n_envs, check_observe, check_polyak, check_ring_batch, ring_capacity
    ex, ns, rti = int(explore), int(n_step), int(replace_target_iter)
    n = check_n_envs(n_envs)
    b = check_ring_batch(batch, n)
    N, Np, K, ka, eta = check_iqn(n_tau, n_tau_next, n_tau_act, kappa, cvar, 2)
    if not 1 <= ns <= L.NSTEP_MAX:
        raise ValueError(f"n_step must be in 1..{L.NSTEP_MAX}, got {n_step}")
    rho = check_polyak(polyak, allow_off=True)
    if rti < 1:
        raise ValueError(f"replace_target_iter must be >= 1, got {replace_target_iter}")
    ob = check_observe(observe)
    if ob < ns - 1:
        raise ValueError(f"observe must be >= n_step - 1 = {ns - 1}: the first n_step - 1 steps only store (no n-step transition is complete yet), got {observe}")
    if ex < 1:
        raise ValueError(f"explore must be >= 1, got {explore}")
    e0, e1 = float(initial_epsilon), float(final_epsilon)
    if not (0.0 <= e1 <= e0 <= 1.0):
        raise ValueError(f"the epsilon schedule needs 0 <= final_epsilon <= initial_epsilon <= 1, got {initial_epsilon} -> {final_epsilon}")
    g, l = check_gamma(gamma), check_lr(lr)
    cap = ring_capacity(capacity, n)
    if cap < max(2, ns) * n:
        raise ValueError(f"capacity {cap} < max(2, n_step) x n_envs = {max(2, ns) * n}")
    return n, b, N, Np, K, ka, eta, ns, rho, rti, ob, ex, e0, e1, g, l, check_max_grad_norm(max_grad_norm), cap


def check_prioritized(prioritized):
    """VecIQN's `prioritized` setting, checked apart from check_args (whose positional parameters stay as they are) -> bool"""
    if not isinstance(prioritized, (bool, np.bool_)):
        raise ValueError(f"prioritized must be True or False, got {prioritized!r}")
    return bool(prioritized)


def check_dueling(dueling):
    """VecIQN's `dueling` setting, checked apart from check_args (whose positional parameters stay as they are) -> bool"""
    if not isinstance(dueling, (bool, np.bool_)):
        raise ValueError(f"dueling must be True or False, got {dueling!r}")
    return bool(dueling)


def check_munchausen(munchausen, temp, alpha, clip, double_q=False):
    """VecIQN's Munchausen settings, checked apart from check_args (whose positional parameters stay as they are) -> (on, temp, alpha, l0);
    the three values are checked whether or not the target is on (the net holds them either way)"""
    from .vec import check_munchausen as check_values
    if not isinstance(munchausen, (bool, np.bool_)):
        raise ValueError(f"munchausen must be True or False, got {munchausen!r}")
    try:
        t, a, c = check_values(temp, alpha, clip)
    except ValueError as e:
        raise ValueError(str(e).replace("tau must", "temp must")) from None
    if munchausen and double_q:
        raise ValueError("munchausen=True with double_q=True: the Munchausen target is a soft value over all actions and has no greedy next action "
                         "for the online net to choose")
    return bool(munchausen), t, a, c


def check_noisy(noisy, sigma0, acting_noise):
    """VecIQN's noisy-net settings, checked apart from check_args (whose positional parameters stay as they are) -> (noisy, sigma0,
    acting_noise); sigma0 is checked whether or not the layers are on"""
    from .vec import ACTING_NOISE_MODES, check_sigma0
    if not isinstance(noisy, (bool, np.bool_)):
        raise ValueError(f"noisy must be True or False, got {noisy!r}")
    try:
        s0 = check_sigma0(sigma0)
    except (TypeError, ValueError):
        raise ValueError(f"sigma0 must be finite and >= 0, got {sigma0!r}") from None
    if acting_noise not in ACTING_NOISE_MODES:
        raise ValueError(f"acting_noise must be 'shared' or 'env', got {acting_noise!r}")
    if acting_noise == "env" and not noisy:
        raise ValueError("acting_noise='env' needs a noisy net (noisy=True)")
    return bool(noisy), s0, acting_noise


def net_kind(noisy):
    return "a noisy net" if noisy else "a non-noisy net"


def iqn_arch(dueling, noisy):
    """the QNet arch of a VecIQN's net"""
    return ("iqnduelingnoisy" if dueling else "iqnnoisy") if noisy else ("iqndueling" if dueling else "iqn")


def target_kind(munchausen):
    return "Munchausen" if munchausen else "hard"


def head_kind(dueling):
    return "dueling" if dueling else "plain"


def replay_kind(prioritized):
    return "prioritized" if prioritized else "uniform"


class VecIQN(DeviceLoop):
    noisy, sigma0, acting_noise = False, 0.5, "shared"       # (what __init__ sets per instance: a loop without noisy layers)

    def __init__(self, n_envs, batch=32, double_q=False, n_step=1, n_tau=8, n_tau_next=8, n_tau_act=32, kappa=1.0, cvar=1.0, polyak=0.0,
                 replace_target_iter=500, observe=1000, explore=1_000_000, initial_epsilon=None, final_epsilon=0.0, gamma=0.99, lr=1e-6,
                 max_grad_norm=0, fc_width=512, seed=0, capacity=None, prioritized=False, dueling=False,
                 munchausen=False, temp=0.03, alpha=0.9, clip=-1.0, noisy=False, sigma0=0.5, acting_noise="shared"):
        """n_envs games; every step trains one minibatch of `batch` transitions (<= n_envs, <= 256) once more than `observe` steps have
        filled the memory.  n_tau / n_tau_next: the tau sampled per transition for the online / target quantiles; n_tau_act: the acting
        grid; kappa: the quantile Huber threshold; cvar = eta in (0, 1]: act on CVaR_eta (1 = the mean).  double_q: a* from the online
        net.  n_step > 1: n-step returns.  The epsilon schedule (observe / explore / initial / final) and the periodic target copy are
        VecBrain's; polyak > 0 replaces the copy by soft updates; lr is Adam's; max_grad_norm=G > 0 clips the gradient's global norm.
        prioritized: train from a prioritized memory (importance-weighted loss, the per-sample loss as the priority).
        dueling: the dueling IQN net (value and advantage quantile streams) instead of the plain one.
        munchausen: the Munchausen target with the softmax temperature temp, the bonus's scale alpha and its lower clip (not with double_q).
        noisy: noisy fc1 and head layers, sigma initialised to sigma0 / sqrt(fan_in); the exploration comes from the noise, so
        initial_epsilon defaults to 0 (0.03 without noise); an explicit initial_epsilon is honoured.  acting_noise: 'shared' -- one noise
        sample per step for all envs -- or 'env': independent noise per env when acting (training is the same in both)."""
        if initial_epsilon is None:                          # (noisy itself is checked below, behind the checks of before)
            initial_epsilon = 0.0 if isinstance(noisy, (bool, np.bool_)) and noisy else 0.03
        (self.n, self.batch, self.n_tau, self.n_tau_next, self.n_tau_act, self.kappa, self.cvar, self.n_step, self.polyak, self.replace_target_iter,
         self.observe, self.explore, self.initial_epsilon, self.final_epsilon, self.gamma, self.lr, self.max_grad_norm, self.capacity) = check_args(
            n_envs, batch, n_tau, n_tau_next, n_tau_act, kappa, cvar, n_step, polyak, replace_target_iter, observe, explore, initial_epsilon,
            final_epsilon, gamma, lr, max_grad_norm, capacity)
        self.prioritized = check_prioritized(prioritized)
        self.dueling = check_dueling(dueling)
        self.munchausen, self.temp, self.alpha, self.clip = check_munchausen(munchausen, temp, alpha, clip, bool(double_q))
        self.noisy, self.sigma0, self.acting_noise = check_noisy(noisy, sigma0, acting_noise)
        self.double_q = bool(double_q)
        self.seed = int(seed)
        self.fc_width = int(fc_width)
        self.epsilon = self.initial_epsilon
        noisy_kw = dict(sigma0=self.sigma0) if self.noisy else {}
        self._build_world(iqn_arch(self.dueling, self.noisy), max(self.n, self.batch), self._setup_net, prioritized=self.prioritized,
                          n_step=self.n_step, n_tau=self.n_tau, n_tau_next=self.n_tau_next, n_tau_act=self.n_tau_act, kappa=self.kappa, **noisy_kw)
        self._bind()
        self.timeStep = 0                                    # env steps per env so far: the key of the epsilon and tau draws

    def _setup_net(self, net):
        if self.cvar != 1.0:
            net.set_iqn_risk(self.cvar)
        if self.munchausen:                                  # (off: the net is never touched)
            net.set_iqn_munchausen(True, self.temp, self.alpha, self.clip)
        if self.acting_noise == "env":                       # (the fused step reads it: act with per-env noise, draw the online sample after)
            net.set_acting_noise("env")

    def _bind(self):
        from .vec import IqnPerStep, IqnStep
        self.one_step = (IqnPerStep if self.prioritized else IqnStep)(self.env, self.replay, self.net, self.batch, self.gamma, self.double_q)
        self.loss = self.one_step.loss

    def step(self):
        """one vector step -> the loss f32[1] (device)"""
        if self.timeStep < self.n_step - 1:                  # no n-step transition is complete yet: store without drawing a minibatch
            if self.noisy and self.acting_noise == "shared":   # (the fused step's order: the online sample in front of acting ...)
                self.net.reset_noise(0, self.seed, self.timeStep)
            if self.acting_noise == "env":
                actions = self.net.act_nib_env_noise(self.nib, self.epsilon, seed=self.seed, step=self.timeStep)
                self.net.reset_noise(0, self.seed, self.timeStep)      # (... or, per-env acting, behind it)
            else:
                actions = self.net.act_nib(self.nib, self.epsilon, seed=self.seed, step=self.timeStep)
            _, reward, terminal, _ = self.env.frame_step(actions, want_u8=False)
            self.replay.push(self.env.frame_bits, actions, reward, terminal)
            self.timeStep += 1
            return self.loss
        training = self.timeStep > self.observe
        if training and not self.polyak and self.timeStep % self.replace_target_iter == 0:
            self.net.sync_target()                           # (acting reads the online net only: the same as syncing before training)
        self.one_step(self.epsilon, seed=self.seed, step=self.timeStep, train=training)
        if self.epsilon > self.final_epsilon and training:
            self.epsilon -= (self.initial_epsilon - self.final_epsilon) / self.explore
        if training and self.polyak:
            self.net.soft_sync_target(self.polyak)
        self.timeStep += 1
        return self.loss

    def _last_noise(self):
        """the online sample the last step left: drawn at (seed, timeStep - 1); mean mode before the first step"""
        if self.timeStep > 0:
            self.net.reset_noise(0, self.seed, self.timeStep - 1)
        else:
            self.net.mean_noise(0)

    def evaluate(self, n_envs=4096, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0, noise="mean"):
        """DeviceLoop.evaluate; a noisy net plays with its mean weights (noise='sample': one sample keyed by act_seed), and its online
        sample of the last step is put back afterwards"""
        from .evaluate import evaluate
        res = evaluate(self.net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed, noise=noise)
        if self.noisy:
            self._last_noise()
        return res

    # ------------------------------------------------------------------ checkpoint / resume
    def save(self, path):
        """everything the loop needs to continue bit for bit: the nets, Adam, every env's state and frame stack, the stats, the memory
        (with its generator and, prioritized, its tree), the counters, epsilon and the settings; `head` = 'iqn' tells the file from the
        other loops', `prioritized` the memory's kind (a file without the key is a uniform one's), `dueling` the net's (without the key: a plain IQN net's),
        `munchausen` = (on, temp, alpha, clip) the target's (without the key: the hard target); a noisy net adds `noisy`, `sigma0` and
        `acting_noise` (without them: not noisy), and its nets and Adam slots hold [mu | sigma]"""
        own = {}
        if self.noisy:
            own = dict(noisy=np.array([1], np.int64), sigma0=np.array([self.sigma0], np.float64), acting_noise=np.array([self.acting_noise]))
        self._save(path, IQN_HEAD, **own,
                   scalars=np.array([self.timeStep, self.seed, self.n, self.batch, self.fc_width, self.observe, self.explore, self.n_step,
                                     int(self.double_q), self.replace_target_iter], np.int64),
                   iqn=np.array([self.n_tau, self.n_tau_next, self.n_tau_act, self.kappa, self.cvar], np.float64),
                   prioritized=np.array([int(self.prioritized)], np.int64), dueling=np.array([int(self.dueling)], np.int64),
                   munchausen=np.array([float(self.munchausen), self.temp, self.alpha, self.clip], np.float64),
                   settings=np.array([self.gamma, self.polyak, self.max_grad_norm, self.lr, self.epsilon, self.initial_epsilon, self.final_epsilon],
                                     np.float64))

    def load(self, path):
        """the inverse of save(), into a VecIQN made with the same n_envs, batch, fc_width, n_step, (n_tau, n_tau_next, n_tau_act, kappa),
        capacity, seed, memory kind (prioritized or not), head kind (dueling or not) and target (munchausen or not, and its temp, alpha,
        clip) and noisy layers (noisy or not, sigma0, acting_noise); the other settings of the file replace this object's"""
        import torch
        z = np.load(npz_path(path))
        refuse_foreign_head(z, path, lambda head: head != IQN_HEAD and f"a {head} head (another loop's), this is a VecIQN (head {IQN_HEAD!r})")
        per = bool(int(z["prioritized"][0])) if "prioritized" in z.files else False
        if per != self.prioritized:
            raise ValueError(f"checkpoint {path} was written by a VecIQN with a {replay_kind(per)} memory, this VecIQN has a "
                             f"{replay_kind(self.prioritized)} one (prioritized={self.prioritized})")
        sc = [int(x) for x in z["scalars"]]
        if (sc[2], sc[3], sc[4], sc[7]) != (self.n, self.batch, self.fc_width, self.n_step):
            raise ValueError(f"checkpoint {path} was written with (n_envs, batch, fc_width, n_step) = {(sc[2], sc[3], sc[4], sc[7])}, this "
                             f"VecIQN has {(self.n, self.batch, self.fc_width, self.n_step)}")
        if sc[1] != self.seed:
            raise ValueError(f"checkpoint {path} was written with seed {sc[1]}, this VecIQN has seed {self.seed} (the envs' pipe-gap "
                             "streams are keyed by it)")
        q = [float(x) for x in z["iqn"]]
        mine = (self.n_tau, self.n_tau_next, self.n_tau_act, self.kappa)
        if (int(q[0]), int(q[1]), int(q[2]), q[3]) != mine:
            raise ValueError(f"checkpoint {path} was written with (n_tau, n_tau_next, n_tau_act, kappa) = {(int(q[0]), int(q[1]), int(q[2]), q[3])}, "
                             f"this VecIQN has {mine}")
        du = bool(int(z["dueling"][0])) if "dueling" in z.files else False
        if du != self.dueling:
            raise ValueError(f"checkpoint {path} was written by a VecIQN with a {head_kind(du)} IQN head, this VecIQN has a "
                             f"{head_kind(self.dueling)} one (dueling={self.dueling})")
        mu = [float(x) for x in z["munchausen"]] if "munchausen" in z.files else [0.0]
        if bool(mu[0]) != self.munchausen:
            raise ValueError(f"checkpoint {path} was written by a VecIQN with the {target_kind(bool(mu[0]))} target, this VecIQN has the "
                             f"{target_kind(self.munchausen)} one (munchausen={self.munchausen})")
        if self.munchausen and tuple(mu[1:]) != (self.temp, self.alpha, self.clip):
            raise ValueError(f"checkpoint {path} was trained with munchausen (temp, alpha, clip) = {tuple(mu[1:])}, this VecIQN has "
                             f"{(self.temp, self.alpha, self.clip)}")
        nz = bool(int(z["noisy"][0])) if "noisy" in z.files else False
        if nz != self.noisy:
            raise ValueError(f"checkpoint {path} holds {net_kind(nz)}, this VecIQN has {net_kind(self.noisy)} (noisy={self.noisy}: the parameter "
                             "vectors differ)")
        if self.noisy:
            s0, an = float(z["sigma0"][0]), str(z["acting_noise"][0])
            if s0 != self.sigma0:
                raise ValueError(f"checkpoint {path} was written with sigma0 = {s0}, this VecIQN has sigma0 = {self.sigma0}")
            if an != self.acting_noise:
                raise ValueError(f"checkpoint {path} was written with acting_noise = {an!r}, this VecIQN has acting_noise = {self.acting_noise!r}")
        self._restore(z)
        self.gamma, self.polyak, self.max_grad_norm, self.lr, self.epsilon, self.initial_epsilon, self.final_epsilon = (float(x) for x in z["settings"])
        self.cvar = q[4]
        self.net.set_hparams(lr=self.lr)
        self.net.set_max_grad_norm(self.max_grad_norm)
        self.net.set_iqn_risk(self.cvar)
        self.observe, self.explore, self.double_q, self.replace_target_iter = sc[5], sc[6], bool(sc[8]), sc[9]
        self.timeStep = sc[0]
        if self.noisy:
            self._last_noise()
        self._bind()
        torch.cuda.synchronize()

    def run(self, steps, log_every=1000):
        for i in range(steps):
            loss = self.step()
            if log_every and (i + 1) % log_every == 0:
                score, clip = score_text(self.net, self.stats), clip_text(self.net, self.max_grad_norm)
                print(f"TIMESTEP {self.timeStep} / ENVS {self.n} / EPSILON {self.epsilon:.6f} / {score} / LOSS {loss.item():.6g}{clip}", flush=True)
