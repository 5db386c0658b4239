"""VecActorCritic: synchronous advantage actor-critic (A2C), or PPO on the same rollout, on the vectorised loop, entirely device resident.

    update:  T x [sample the policy for N envs -> frame_step -> store]   (AcRolloutStep, one host call each)
             -> V(s_T) with the weights the rollout acted with -> GAE (vec.ac_gae)
             -> the T N fresh transitions in ring-fed chunks of <= 256 (vec.ac_train_from_replay), gradients summed
             -> [clip the sum] -> Adam, once

    algo="ppo" replaces the last two lines: [normalise the advantages (vec.ac_normalize_adv)] -> K epochs x [a fresh permutation of
             the T N transitions (vec.ac_permute) -> M minibatches x [ring-fed chunks of <= 256 read through the permutation
             (vec.ppo_train_from_replay), gradients summed -> [clip] -> Adam]]
    one_call=True runs each epoch's M minibatches as ONE host call (vec.ppo_epoch: the same calls in the same order, composed in the
             library); it carries the three stabilisers: adv_norm_scope='minibatch' (every minibatch's advantages normalised over the
             minibatch), target_kl (no further epoch once an epoch's mean approximate KL exceeds 1.5 target_kl) and anneal_lr (Adam's
             learning rate falls linearly to 0 over total_updates)

The replay memory is not sampled: its frame ring is the rollout's state store (the newest T N deque positions are the rollout,
in the order of the flattened [T, N] buffers), so no state is ever copied.  One net, one GPU; include/fbdqn.h pins the
semantics, DESIGN.md section 16 the schedule (section 17: PPO).  The reference's actor-critic (BrainActorCritic.py: one env, one episode, a second
network as the critic) stays what --model actorcritic runs; this is the batched algorithm its capacity is for.
"""
import numpy as np

from .vecloop import DeviceLoop, clip_text, npz_path, refuse_foreign_head, score_text

ALGOS = ("a2c", "ppo")                                       # what VecActorCritic(algo=...) takes
AC_HEAD = "ac"                                               # what a checkpoint of this class records as its head
CHUNK = 256                                                  # samples per ring-fed train chunk (the train step's limit)
ADV_NORM_SCOPES = ("rollout", "minibatch")                   # what VecActorCritic(adv_norm_scope=...) takes
KL_STOP_FACTOR = 1.5                                         # an epoch's mean approximate KL above this times target_kl ends the update
PPO_OPTS_OFF = ("rollout", 0.0, False, 0)                    # (adv_norm_scope, target_kl, anneal_lr, total_updates) of a checkpoint without `ppo_opts`


def rollout_indices(size, rollout, n_envs):
    """the deque positions of the rollout's T N transitions in a memory that holds `size` (its newest ones), in the order of the
    flattened [T, N] buffers: position j names (t, e) = divmod(total - size + j, N) (csrc/fb_gather.h)"""
    tn = int(rollout) * int(n_envs)
    if size < tn:
        raise ValueError(f"the memory holds {size} transitions, fewer than the rollout's {tn}")
    return size - tn + np.arange(tn, dtype=np.int64)


def check_args(n_envs, rollout, gamma, gae_lambda, value_coef, entropy_coef, max_grad_norm):
    """every argument check of VecActorCritic that needs no GPU -> the checked values"""
    from .vec import check_ac, check_gae, check_max_grad_norm, check_n_envs, check_rollout
    n = check_n_envs(n_envs)
    T = check_rollout(rollout)
    g, l = check_gae(gamma, gae_lambda)
    cv, ce = check_ac(value_coef, entropy_coef)
    return n, T, g, l, cv, ce, check_max_grad_norm(max_grad_norm)


def check_ppo_args(n_envs, rollout, epochs, minibatches, clip_eps, value_clip):
    """every argument check of VecActorCritic(algo='ppo') that needs no GPU -> (epochs, minibatches, clip_eps, value_clip)"""
    from .vec import check_ppo
    k, m, tn = int(epochs), int(minibatches), int(rollout) * int(n_envs)
    if k < 1:
        raise ValueError(f"epochs must be >= 1, got {epochs}")
    if m < 1 or tn % m:
        raise ValueError(f"minibatches must be >= 1 and divide rollout x n_envs = {tn}, got {minibatches}")
    return (k, m) + check_ppo(clip_eps, value_clip)


def check_ppo_options(adv_norm_scope="rollout", target_kl=None, anneal_lr=False, total_updates=None, one_call=None, normalize_adv=True):
    """every check of VecActorCritic(algo='ppo')'s stabilisers that needs no GPU -> (adv_norm_scope, target_kl, anneal_lr,
    total_updates, one_call): target_kl 0.0 = off (None and 0), total_updates 0 = none given, one_call resolved (None: True exactly
    when one of the three is on; adv_norm_scope='minibatch' is on only while normalize_adv is)"""
    if adv_norm_scope not in ADV_NORM_SCOPES:
        raise ValueError(f"adv_norm_scope must be one of {ADV_NORM_SCOPES}, got {adv_norm_scope!r}")
    kl = 0.0 if target_kl is None else float(target_kl)
    if not (np.isfinite(kl) and kl >= 0.0):
        raise ValueError(f"target_kl must be finite and >= 0 (None or 0 = off), got {target_kl}")
    total = 0 if total_updates is None else int(total_updates)
    if total_updates is not None and total < 1:
        raise ValueError(f"total_updates must be >= 1, got {total_updates}")
    anneal = bool(anneal_lr)
    if anneal and total < 1:
        raise ValueError("anneal_lr needs total_updates >= 1: the learning rate falls to 0 over that many updates")
    on = [name for name, x in (("adv_norm_scope='minibatch'", adv_norm_scope == "minibatch" and normalize_adv), ("target_kl", kl > 0.0),
                               ("anneal_lr", anneal)) if x]
    if on and one_call is not None and not one_call:
        raise ValueError(f"{' / '.join(on)} need one_call=True: one_call=False is the composed update, which has none of them")
    return adv_norm_scope, kl, anneal, total, bool(on) if one_call is None else bool(one_call)


def annealed_lr(lr, update, total_updates):
    """Adam's learning rate before update `update` (0-based) of a run annealed over total_updates: max(0, lr (1 - u / total)), float64"""
    return max(0.0, float(lr) * (1.0 - float(update) / float(total_updates)))


def check_ppo_opts_match(path, saved, mine):
    """a checkpoint's (adv_norm_scope, target_kl, anneal_lr, total_updates) against this object's: the first that differs is refused by name"""
    for name, a, b in zip(("adv_norm_scope", "target_kl", "anneal_lr", "total_updates"), saved, mine):
        if a != b:
            raise ValueError(f"checkpoint {path} was written with {name} = {a!r}, this VecActorCritic has {name} = {b!r}")


class VecActorCritic(DeviceLoop):
    def __init__(self, n_envs, rollout=5, gamma=0.99, gae_lambda=0.95, value_coef=0.5, entropy_coef=0.01, max_grad_norm=0.0, fc_width=512,
                 seed=0, lr=1e-4, capacity=None, algo="a2c", epochs=4, minibatches=4, clip_eps=0.2, value_clip=0.0, normalize_adv=True,
                 adv_norm_scope="rollout", target_kl=None, anneal_lr=False, total_updates=None, one_call=None):
        """n_envs games, `rollout` steps per update (1..128), GAE(gamma, gae_lambda), loss = mean(L_pi + value_coef L_v - entropy_coef H)
        over the rollout's rollout x n_envs samples, max_grad_norm=G > 0 clips the summed gradient's global norm before Adam, lr is
        Adam's (the other hyper-parameters are the library's TF defaults).  capacity: the memory's, at least (rollout + 2) n_envs (the
        default); it only has to hold the rollout.
        algo='ppo': each rollout trains `epochs` passes of `minibatches` shuffled minibatches (it must divide rollout x n_envs), an Adam
        step each, under the ratio clip clip_eps and the value clip value_clip (0 = off); normalize_adv: the rollout's advantages to
        mean 0, standard deviation 1 first.  algo='a2c' reads none of the five.
        algo='ppo' only, all off by default: adv_norm_scope='minibatch' (read while normalize_adv is True): every minibatch is normalised
        over itself, and the rollout-wide normalisation is not applied; target_kl=X > 0: after every epoch but the last, that epoch's
        mean approximate KL (ONE float read from the device) above 1.5 X ends the update; anneal_lr with total_updates=U >= 1: before
        update u Adam's learning rate is max(0, lr (1 - u / U)).  one_call: each epoch as one host call (vec.ppo_epoch) instead of the
        chunk-by-chunk loop; None = True exactly when one of the three is on, which need it."""
        if algo not in ALGOS:
            raise ValueError(f"algo must be one of {ALGOS}, got {algo!r}")
        self.algo = algo
        self.n, self.T, self.gamma, self.gae_lambda, self.value_coef, self.entropy_coef, self.max_grad_norm = check_args(
            n_envs, rollout, gamma, gae_lambda, value_coef, entropy_coef, max_grad_norm)
        self.normalize_adv = bool(normalize_adv)
        if algo == "ppo":
            self.epochs, self.minibatches, self.clip_eps, self.value_clip = check_ppo_args(self.n, self.T, epochs, minibatches, clip_eps, value_clip)
            self.adv_norm_scope, self.target_kl, self.anneal_lr, self.total_updates, self.one_call = check_ppo_options(
                adv_norm_scope, target_kl, anneal_lr, total_updates, one_call, self.normalize_adv)
        else:                                                # (A2C reads none of them: the net keeps the library's defaults)
            from .vec import PPO_DEFAULTS
            self.epochs, self.minibatches, self.clip_eps, self.value_clip = (1, 1) + PPO_DEFAULTS
            self.adv_norm_scope, self.target_kl, self.anneal_lr, self.total_updates, self.one_call = PPO_OPTS_OFF + (False,)
        need = (self.T + 2) * self.n
        self.capacity = need if capacity is None else int(capacity)
        if self.capacity < need:
            raise ValueError(f"capacity {self.capacity} < (rollout + 2) x n_envs = {need}: the memory's ring is the rollout's state store")
        import torch
        from .vec import AcRolloutStep, check_lr
        self.lr = check_lr(lr)
        self.seed = int(seed)
        self.fc_width = int(fc_width)
        self._build_world("ac", max(self.n, CHUNK), self._setup_net, target_seed=self.seed + 1)      # (the target net exists in every net; A2C never reads it)
        self.roll = AcRolloutStep(self.env, self.replay, self.net, self.T)
        self.grad = torch.zeros(self.net.n_params, dtype=torch.float32, device="cuda")
        self.chunk_grad = torch.zeros_like(self.grad)
        self.losses = torch.zeros(6 if self.algo == "ppo" else 4, dtype=torch.float32, device="cuda")
        self.perm = torch.zeros(self.T * self.n, dtype=torch.int64, device="cuda") if self.algo == "ppo" else None
        self.epochs_run = self.epochs                        # epochs of the last update (fewer under target_kl)
        if self.one_call:                                    # what vec.ppo_epoch fills: the minibatches' loss rows, the chunk's actions
            self.loss_rows = torch.zeros((self.minibatches, 6), dtype=torch.float32, device="cuda")
            self.a_out = torch.zeros(CHUNK, dtype=torch.uint8, device="cuda")
            self.epoch_mean = torch.zeros(6, dtype=torch.float32, device="cuda")
            self.adv_mb = None                               # ... and a minibatch's normalised advantages, made when first needed
        self.timeStep = 0                                    # env steps per env so far: the key of the policy's draws
        self.updates = 0
        self.pushes = 0                                      # pushes since the reset: len(replay) without a device sync
        self._idx_for = None

    def _setup_net(self, net):
        net.set_ac(self.value_coef, self.entropy_coef)
        if self.algo == "ppo":
            net.set_ppo(self.clip_eps, self.value_clip)

    def _mb_norm(self):
        return self.normalize_adv and self.adv_norm_scope == "minibatch"

    def _indices(self):
        import torch
        size = min(self.pushes * self.n, self.capacity)
        if self._idx_for != size:                            # (constant once the memory is full)
            self._idx = torch.from_numpy(rollout_indices(size, self.T, self.n)).cuda()
            self._idx_for = size
        return self._idx

    def collect(self):
        """the rollout: T steps of the N envs with the current policy, V(s_T), GAE -> (adv, ret), float32[T N] each, in the order of the
        flattened [T, N] buffers (self.roll holds the rollout's rewards, terminals, values and log-probabilities)"""
        from .vec import ac_gae
        for t in range(self.T):
            self.roll(t, seed=self.seed, step=self.timeStep)
            self.timeStep += 1
            self.pushes += 1
        self.net.act_policy_nib(self.nib, value=self.roll.value[self.T], value_only=True)      # V(s_T), the pre-update weights
        adv, ret = ac_gae(self.roll.reward, self.roll.terminal, self.roll.value, self.gamma, self.gae_lambda)
        return adv.view(-1), ret.view(-1)

    def update(self):
        """one update: the rollout, the advantages, then A2C's chunks and one Adam step -> the update's four loss numbers f32[4], or
        PPO's epochs of minibatches, an Adam step each -> the last epoch's six loss numbers f32[6], its minibatches' mean (device)"""
        from .vec import ac_train_from_replay
        adv, ret = self.collect()
        idx, tn = self._indices(), self.T * self.n
        if self.algo == "ppo":
            if self.anneal_lr:                               # (no state beyond the update counter; set_hparams waits for the device)
                self.net.set_hparams(lr=annealed_lr(self.lr, self.updates, self.total_updates))
            return (self._ppo_epochs_one_call if self.one_call else self._ppo_epochs)(idx, adv, ret, tn)
        self.grad.zero_()
        self.losses.zero_()
        for k in range(0, tn, CHUNK):
            e = min(k + CHUNK, tn)
            loss, _ = ac_train_from_replay(self.replay, self.net, idx[k:e], adv[k:e], ret[k:e], n_total=tn, flat_grad=self.chunk_grad)
            self.grad += self.chunk_grad
            self.losses += loss
        if self.max_grad_norm:
            self.net.clip_grad(self.grad)
        self.net.apply_adam(self.grad)
        self.updates += 1
        return self.losses

    def _ppo_epochs(self, idx, adv, ret, tn):
        """K epochs over the rollout: epoch e shuffles with the permutation of draw updates K + e (no state beyond the counter); a
        minibatch is tn / M consecutive elements of it, read in ring-fed chunks of <= 256: the states at idx[0] + perm, the rollout's
        advantages, returns, log-probabilities and values at perm"""
        from .vec import ac_normalize_adv, ac_permute, ppo_train_from_replay
        if self.normalize_adv:
            ac_normalize_adv(adv, out=adv)
        logp, value = self.roll.logp.view(-1), self.roll.value[:self.T].view(-1)
        mb = tn // self.minibatches
        for e in range(self.epochs):
            perm = ac_permute(tn, self.seed, self.updates * self.epochs + e, out=self.perm)
            pos = perm + idx[:1]                             # (the rollout's deque positions are consecutive: rollout_indices)
            last = e == self.epochs - 1
            if last:
                self.losses.zero_()
            for lo in range(0, tn, mb):
                self.grad.zero_()
                for k in range(lo, lo + mb, CHUNK):
                    hi = min(k + CHUNK, lo + mb)
                    loss, _ = ppo_train_from_replay(self.replay, self.net, pos[k:hi], adv, ret, logp, value, sel=perm[k:hi], n_total=mb,
                                                    flat_grad=self.chunk_grad, check_sel=False)      # (a permutation's slice)
                    self.grad += self.chunk_grad
                    if last:
                        self.losses += loss
                if self.max_grad_norm:
                    self.net.clip_grad(self.grad)
                self.net.apply_adam(self.grad)
        self.losses /= self.minibatches
        self.updates += 1
        return self.losses

    def _ppo_epochs_one_call(self, idx, adv, ret, tn):
        """_ppo_epochs with each epoch as one host call (vec.ppo_epoch): one torch op per epoch, for pos.  The returned six numbers are the
        last epoch RUN's, formed as _ppo_epochs forms them: the running sum of its chunks' numbers (vec.ppo_epoch_sum) over the
        minibatch count, so with every option off they are _ppo_epochs' bits.  target_kl: after every epoch but the last its mean
        approximate KL (epoch_mean[5], the mean of the minibatches' rows) is read, one float, and above 1.5 target_kl the remaining
        epochs are skipped -- their permutation draws stay unused, so the draw of epoch e of update u is u K + e whatever was skipped"""
        from .vec import ac_normalize_adv, ac_permute, ppo_epoch, ppo_epoch_sum
        mb_norm = self._mb_norm()
        if self.normalize_adv and not mb_norm:
            ac_normalize_adv(adv, out=adv)
        if mb_norm and self.adv_mb is None:
            self.adv_mb = adv.new_zeros(tn)
        logp, value = self.roll.logp.view(-1), self.roll.value[:self.T].view(-1)
        for e in range(self.epochs):
            perm = ac_permute(tn, self.seed, self.updates * self.epochs + e, out=self.perm)
            pos = perm + idx[:1]                             # (the rollout's deque positions are consecutive: rollout_indices)
            ppo_epoch(self.replay, self.net, pos, perm, adv, ret, logp, value, self.minibatches, self.grad, self.chunk_grad, self.loss_rows,
                      self.epoch_mean, a_out=self.a_out, adv_scratch=self.adv_mb if mb_norm else None, check_sel=False)      # (a permutation)
            self.epochs_run = e + 1
            if self.target_kl and e < self.epochs - 1 and self.epoch_mean[5].item() > KL_STOP_FACTOR * self.target_kl:
                break
        ppo_epoch_sum(self.net, self.losses)
        self.losses /= self.minibatches
        self.updates += 1
        return self.losses

    # ------------------------------------------------------------------ checkpoint / resume
    def save(self, path):
        """everything the loop needs to continue bit for bit: the nets, Adam, every env's state and frame stack, the stats, the memory,
        the counters and the A2C settings; `head` = 'ac' tells the file from a VecBrain's, and a PPO run adds its settings as `ppo`
        (epochs, minibatches, clip_eps, value_clip, normalize_adv): the permutations have no state beyond the update counter.  With a
        stabiliser on it also adds `ppo_opts` (adv_norm_scope as its index in ADV_NORM_SCOPES, target_kl, anneal_lr, total_updates);
        a file without that key is a run with all of them off"""
        extra = {}
        if self.algo == "ppo":
            extra["ppo"] = np.array([self.epochs, self.minibatches, self.clip_eps, self.value_clip, float(self.normalize_adv)], np.float64)
            opts = (self.adv_norm_scope, self.target_kl, self.anneal_lr, self.total_updates)
            if opts != PPO_OPTS_OFF:                         # (with every stabiliser off the file is the one of before, key for key)
                extra["ppo_opts"] = np.array([float(ADV_NORM_SCOPES.index(opts[0])), opts[1], float(opts[2]), float(opts[3])], np.float64)
        self._save(path, AC_HEAD, scalars=np.array([self.timeStep, self.updates, self.pushes, self.seed, self.n, self.T, self.fc_width], np.int64),
                   ac=np.array([self.gamma, self.gae_lambda, self.value_coef, self.entropy_coef, self.max_grad_norm, self.lr], np.float64), **extra)

    def load(self, path):
        """the inverse of save(), into a VecActorCritic made with the same n_envs, rollout, fc_width, capacity and seed (the envs' pipe-gap
        streams are keyed by the seed they were created with); the A2C settings of the file replace this object's.  PPO's stabilisers
        do not: a file whose `ppo_opts` differ from this object's is refused by the option's name"""
        import torch
        z = np.load(npz_path(path))
        refuse_foreign_head(z, path, lambda head: head != AC_HEAD and f"a {head} head (a VecBrain's), this is a VecActorCritic (head {AC_HEAD!r})")
        kind = "ppo" if "ppo" in z.files else "a2c"
        if kind != self.algo:
            raise ValueError(f"checkpoint {path} holds {'a PPO' if kind == 'ppo' else 'an A2C'} run, this VecActorCritic runs "
                             f"algo={self.algo!r}")
        sc = [int(x) for x in z["scalars"]]
        if (sc[4], sc[5], sc[6]) != (self.n, self.T, self.fc_width):
            raise ValueError(f"checkpoint {path} was written with (n_envs, rollout, fc_width) = {tuple(sc[4:7])}, this VecActorCritic has "
                             f"{(self.n, self.T, self.fc_width)}")
        if sc[3] != self.seed:
            raise ValueError(f"checkpoint {path} was written with seed {sc[3]}, this VecActorCritic has seed {self.seed} (the envs' pipe-gap "
                             "streams are keyed by it)")
        if self.algo == "ppo":                               # (a file without the key: every stabiliser off)
            saved = PPO_OPTS_OFF
            if "ppo_opts" in z.files:
                sc_, kl, an, tot = (float(x) for x in z["ppo_opts"])
                saved = (ADV_NORM_SCOPES[int(sc_)], kl, bool(an), int(tot))
            check_ppo_opts_match(path, saved, (self.adv_norm_scope, self.target_kl, self.anneal_lr, self.total_updates))
            if bool(z["ppo"][4]) and saved[0] == "minibatch" and not self.one_call:      # (the file's normalize_adv replaces this object's)
                raise ValueError(f"checkpoint {path} normalises its advantages per minibatch, which needs one_call=True; this VecActorCritic "
                                 f"was made with normalize_adv={self.normalize_adv} and one_call={self.one_call}")
        self._restore(z)
        self.gamma, self.gae_lambda, self.value_coef, self.entropy_coef, self.max_grad_norm, self.lr = (float(x) for x in z["ac"])
        self.net.set_ac(self.value_coef, self.entropy_coef)
        self.net.set_hparams(lr=self.lr)
        self.net.set_max_grad_norm(self.max_grad_norm)
        if self.algo == "ppo":
            k, m, eps, vclip, norm = (float(x) for x in z["ppo"])
            self.epochs, self.minibatches, self.clip_eps, self.value_clip = check_ppo_args(self.n, self.T, int(k), int(m), eps, vclip)
            self.normalize_adv = bool(norm)
            self.net.set_ppo(self.clip_eps, self.value_clip)
        self.timeStep, self.updates, self.pushes = sc[0], sc[1], sc[2]
        self._idx_for = None
        torch.cuda.synchronize()

    def run(self, updates, log_every=100):
        for i in range(updates):
            losses = self.update()
            if log_every and (i + 1) % log_every == 0:
                tot, lpi, lv, ent, *more = losses.tolist()       # the only host sync of the loop, once per log line
                score, clip = score_text(self.net, self.stats), clip_text(self.net, self.max_grad_norm)
                if more:                                         # PPO
                    clip += f" / CLIP_FRAC {more[0]:.6g} / APPROX_KL {more[1]:.6g}"
                    if self.one_call:
                        clip += f" / EPOCHS {self.epochs_run}"
                print(f"TIMESTEP {self.timeStep} / ENVS {self.n} / POLICY_LOSS {lpi:.6g} / VALUE_LOSS {lv:.6g} / ENTROPY {ent:.6g} / "
                      f"{score} / LOSS {tot:.6g}{clip}", flush=True)
