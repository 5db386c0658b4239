"""VecBrain: the reference's training loop (FlappyBirdDQN.py:72-76 + Brain*.setPerception) for N
envs per GPU, entirely device resident: no tensor leaves HBM between getAction and the Adam update.

    step:  currentState (A1) -> getAction for N envs (A2) -> frame_step (E*, P1 fused) -> store (R1/R4)
           -> sample (R1/R4) -> gather (R2) -> _trainQNetwork (Q*) [-> all-reduce over ranks]

Host-side schedule follows the reference: training starts once onlineTimeStep > OBSERVE, epsilon
decays by (INITIAL - FINAL) / EXPLORE per step after that, Nature/Double sync the target net when
timeStep % 500 == 0, PER never does (the reference agent's quirk, kept for algo 'per' only); C51 and C51 with prioritized
replay ('c51per' / 'c51doubleper') sync every replace_target_iter steps.  arch='c51dueling' gives any of the C51 algos the dueling
C51 head (Rainbow's, with 'c51doubleper' and n-step returns: FlappyBirdDQN.py --model rainbow).  noisy=True gives a C51 algo's net
noisy fc1 and head layers (NoisyNet; with arch='c51dueling', 'c51doubleper' and n-step returns: full Rainbow, --model rainbow --noisy):
fb_vec_step draws the nets' noise every step, and the epsilon schedule defaults to 0.  QR-DQN ('qr', 'qrdouble', 'qrper',
'qrdoubleper') trains a quantile head (arch 'qr', or 'qrdueling' for its dueling form) on one GPU and syncs as C51 does.  Munchausen-DQN ('mdqn',
'mdqnper' with prioritized replay) trains the scalar heads ('plain' or 'dueling') with a soft bootstrap and a clipped log-policy bonus
(tau, alpha, clip; include/fbdqn.h), syncs its target net every replace_target_iter steps and runs data parallel as 'double' / 'per' do.
'doubleper' is Double-DQN's target on a prioritized memory (with arch='dueling' and n_step: Rainbow without the distributional head); it
syncs as 'double' and runs data parallel as 'per'.  huber=delta > 0 gives every scalar algo the Huber (clipped-error) loss.
max_grad_norm=G > 0 clips the flat gradient's global norm to G before Adam (every algo and head; data parallel: behind the reduction);
polyak=rho > 0 replaces the periodic target copy by target += rho (online - target) after every train step.
"""
from . import dist as fdist
from .vecloop import LOCAL_ARRAYS, checkpoint_head, clip_text, core_arrays, npz_path, refuse_foreign_head, restore_core, score_text, to_device

MEAN_LOSS = {"dqn": False, "nature": True, "double": True, "per": True, "c51": True, "c51double": True, "c51per": True, "c51doubleper": True,
             "qr": True, "qrdouble": True, "qrper": True, "qrdoubleper": True, "mdqn": True, "mdqnper": True, "doubleper": True}
C51_ALGOS = ("c51", "c51double")                             # distributional Q-learning (include/fbdqn.h)
C51_PER_ALGOS = ("c51per", "c51doubleper")                   # ... with prioritized replay: weighted loss, KL priorities
QR_ALGOS = ("qr", "qrdouble")                                # quantile regression (QR-DQN; include/fbdqn.h)
QR_PER_ALGOS = ("qrper", "qrdoubleper")                      # ... with prioritized replay: weighted loss, l_b priorities
MDQN_ALGOS = ("mdqn", "mdqnper")                             # Munchausen-DQN on the scalar heads (include/fbdqn.h)
PER_ALGOS = ("per",) + C51_PER_ALGOS + QR_PER_ALGOS + ("mdqnper", "doubleper")      # algos with a prioritized memory
TARGET_SYNC = ("nature", "double", "doubleper") + C51_ALGOS + C51_PER_ALGOS + QR_ALGOS + QR_PER_ALGOS + MDQN_ALGOS   # algos whose target net is synced every replace_target_iter steps
SCALAR_ALGOS = ("dqn", "nature", "double", "per", "doubleper") + MDQN_ALGOS      # the TD algos of the scalar heads: what huber applies to
C51_HEADS = ("c51", "c51dueling")                            # the heads a C51 algo trains (arch; 'plain' means 'c51')
QR_HEADS = ("qr", "qrdueling")                               # the heads a QR algo trains (arch; 'plain' means 'qr')


class HipVecBackend:
    """What VecBrain computes with: the HIP library through vec.py.  (tests/cpu_backend.py holds a CPU stand-in with the
    same five factories, so that the rank logic below -- seed offsets, gradient averaging, target-sync placement -- runs
    in the world-size-2 gloo tests without a GPU; the product never uses anything else than this class.)"""
    name = "hip-gfx950"
    per_one_step = True                                      # fb_vec_step runs the prioritized step too (store, Memory.sample, train, batch_update)
    per_n_step = True                                        # prioritized memories with n-step returns (replay(..., n_step, gamma))
    per_priority_init = True                                 # new leaves at their acting-time |TD error| (replay.set_priority_init('td'), primed inside step())

    def env(self, n_envs, seed):
        from .vec import VecGameState
        return VecGameState(n_envs, seed=seed)

    def replay(self, capacity, n_envs, prioritized, n_step=1, gamma=None):
        """n_step > 1: the memory has n-step returns from its creation (the way a prioritized memory gets them)"""
        from .vec import VecReplay
        return VecReplay(capacity, n_envs, prioritized=prioritized, n_step=n_step, gamma=gamma)

    c51 = True                                               # distributional nets (net(..., support=(n_atoms, v_min, v_max)))
    c51_dueling = True                                       # ... with the dueling C51 head as well (net(..., arch='c51dueling', support=...))
    c51_noisy = True                                         # ... and noisy C51 nets (net(..., support=..., noisy=True, sigma0=s))
    acting_noise_env = True                                  # ... which can act with noise per env (net.set_acting_noise('env'))
    qr = True                                                # quantile nets (net(..., arch='qr' | 'qrdueling', quantiles=(n_quantiles, kappa)))
    mdqn = True                                              # Munchausen-DQN: algos 'mdqn' / 'mdqnper' in step(), net.set_munchausen(tau, alpha, clip)
    double_per = True                                        # algo 'doubleper' in step(): Double-DQN's target on a prioritized memory
    huber = True                                             # the Huber loss on the scalar heads: net.set_huber(delta)
    grad_clip = True                                         # global-norm gradient clipping: net.set_max_grad_norm(G), clip_grad, grad_norm
    polyak = True                                            # soft target updates: net.soft_sync_target(rho)

    def net(self, actions, fc_width, arch, max_batch, support=None, noisy=False, sigma0=0.5, quantiles=None):
        from .vec import QNet
        if quantiles is not None:
            return QNet(actions, fc_width, arch, max_batch=max_batch, n_quantiles=quantiles[0], kappa=quantiles[1])
        if support is not None:
            return QNet(actions, fc_width, arch if arch in C51_HEADS else "c51", max_batch=max_batch, n_atoms=support[0], v_min=support[1],
                        v_max=support[2], noisy=noisy, sigma0=sigma0)
        return QNet(actions, fc_width, arch, max_batch=max_batch)

    def step(self, env, replay, net, batch, algo, gamma, flat_grad, dist=None, mean_loss=False):
        from .vec import VecStep
        return VecStep(env, replay, net, batch, algo, gamma, flat_grad=flat_grad, dist=dist, mean_loss=mean_loss)

    def native(self, rank, world):
        """the library's own RCCL communicator (dist.NativeDP): with it the whole data-parallel step -- all-reduce and Adam included --
        is the one host call fb_vec_step_dp.  Opt-in (FB_DP_NATIVE=1, dist.native_wanted); otherwise torch.distributed's all-reduce
        sits between the step and Adam.  NativeDP() itself makes the ranks agree: it either succeeds on every rank or raises
        NativeUnavailable on every rank (fallback, all alike); a failure after its id exchange is fatal and propagates."""
        import torch.distributed as tdist
        if not fdist.native_wanted() or not tdist.is_initialized() or tdist.get_backend() != "nccl":
            return None
        try:
            return fdist.NativeDP(rank, world)
        except fdist.NativeUnavailable:
            return None

    def zeros(self, n):
        import torch
        return torch.zeros(n, dtype=torch.float32, device="cuda")

    def to_device(self, x):
        return to_device(x)

    def synchronize(self):
        import torch
        torch.cuda.synchronize()

    def train_from_replay(self, replay, net, algo, idx, isw, gamma, flat_grad, want_abs_err):
        """minibatch assembly + train step from the sampled indices on, without gathered copies -> (loss, abs_err or None)"""
        from .vec import train_from_replay
        out = train_from_replay(replay, net, algo, idx, gamma, flat_grad, isw=isw, want_abs_err=want_abs_err)
        return out[0], (out[4] if want_abs_err else None)

    def reducer(self, net, flat_grad, mean_loss):
        """-> callable that all-reduces flat_grad over the ranks: one collective; with FB_DP_OVERLAP=1 two, the large one overlapped
        with the conv backward (dist.OverlappedAllReduce -- off by default, see its docstring)"""
        import os
        if os.environ.get("FB_DP_OVERLAP", "0") == "1":
            return fdist.OverlappedAllReduce(net, flat_grad, mean_loss)
        return lambda: fdist.allreduce_gradients(flat_grad, mean_loss)


# the heads of the other loops' checkpoints -> what load() answers to one ("checkpoint <path> holds ...")
OTHER_LOOPS = {"ac": "an ac head (a VecActorCritic's), this is a VecBrain: load it with dqnflappybird_amd.vecac.VecActorCritic",
               "sac": "a sac head (a VecSAC's), this is a VecBrain: load it with dqnflappybird_amd.vecsac.VecSAC",
               "iqn": "an iqn head (a VecIQN's), this is a VecBrain: load it with dqnflappybird_amd.veciqn.VecIQN"}


def check_checkpoint_head(z, head, path):
    """a C51 checkpoint's head kind must be this brain's ('c51' or 'c51dueling'; checkpoints that record none hold a C51 head)"""
    saved = str(z["head"][0]) if "head" in z.files else "c51"
    if saved != head:
        raise ValueError(f"checkpoint {path} holds a {saved} head, this VecBrain has a {head} head (C51 and dueling C51 parameters "
                         "do not convert)")


def check_checkpoint_quantiles(z, quantiles, head, path):
    """a QR checkpoint goes into a QR brain with the same head, N and kappa only, and a QR brain takes a QR checkpoint only (C51 and
    N = 51 QR heads have the same parameter count: the recorded head is what tells them apart)"""
    saved_head = checkpoint_head(z)
    saved_qr = saved_head in QR_HEADS
    if saved_qr and quantiles is None:
        raise ValueError(f"checkpoint {path} holds a {saved_head} (QR) head, this VecBrain has a {head} head (QR and other parameters "
                         "do not convert)")
    if not saved_qr and quantiles is not None:
        raise ValueError(f"checkpoint {path} holds a {saved_head} head, this VecBrain has a {head} (QR) head (QR and other parameters "
                         "do not convert)")
    if quantiles is None:
        return
    if saved_head != head:
        raise ValueError(f"checkpoint {path} holds a {saved_head} head, this VecBrain has a {head} head (QR and dueling QR parameters "
                         "do not convert)")
    n, k = z["quantiles"].tolist()
    if (int(n), float(k)) != (int(quantiles[0]), float(quantiles[1])):
        raise ValueError(f"checkpoint {path} was trained with (n_quantiles, kappa) = ({int(n)}, {float(k)}), this VecBrain has "
                         f"({int(quantiles[0])}, {float(quantiles[1])})")


def check_checkpoint_munchausen(z, munchausen, path):
    """a Munchausen-DQN brain takes a checkpoint trained with its own (tau, alpha, l0), or one that records none (any scalar-head
    checkpoint: the parameters are the same net's); a brain of another algo does not read the key"""
    if munchausen is None or "munchausen" not in z.files:
        return
    saved = tuple(float(x) for x in z["munchausen"].tolist())
    if saved != tuple(float(x) for x in munchausen):
        raise ValueError(f"checkpoint {path} was trained with munchausen (tau, alpha, clip) = {saved}, this VecBrain has "
                         f"{tuple(float(x) for x in munchausen)}")


def check_checkpoint_huber(z, huber, path):
    """a checkpoint's nets were trained with the Huber delta it records (no key: 0, the squared loss -- every checkpoint of before the
    setting, and every one a brain with delta = 0 writes: save() records the key only when delta > 0, so such a checkpoint is the file
    it was before the setting existed); a scalar-head brain takes one trained with its own delta only.  Distributional brains (huber None) do not read the key"""
    if huber is None:
        return
    saved = float(z["huber"][0]) if "huber" in z.files else 0.0
    if saved != float(huber):
        raise ValueError(f"checkpoint {path} was trained with huber (delta) = {saved}, this VecBrain has huber = {float(huber)}")


def checkpoint_optimiser(z):
    """(max_grad_norm, polyak) a checkpoint records -- 0.0 where it records none: every checkpoint of before the settings, and every one a
    brain with the setting off writes.  Optimiser settings, like the learning rate: load() reports them (VecBrain.checkpoint_optimiser)
    and refuses nothing -- a run may be continued with another limit or rate"""
    return tuple(float(z[k][0]) if k in z.files else 0.0 for k in ("max_grad_norm", "polyak"))


def check_checkpoint_noisy(z, noisy, sigma0, path):
    """a checkpoint's net must be noisy exactly when this brain's is (checkpoints that record nothing hold a non-noisy net)"""
    saved = bool(z["noisy"][0]) if "noisy" in z.files else False
    if saved != bool(noisy):
        kind = lambda b: "a noisy net" if b else "a non-noisy net"
        raise ValueError(f"checkpoint {path} holds {kind(saved)}, this VecBrain has {kind(noisy)} (noisy=True / False: the parameter "
                         "vectors [mu | sigma] and [mu] do not convert)")


def check_checkpoint_support(z, support, path):
    """a checkpoint's head must be this brain's: C51 with the same support (n_atoms, v_min, v_max), or a scalar head on both sides"""
    saved = tuple(z["support"].tolist()) if "support" in z.files else None
    if saved is None and support is not None:
        raise ValueError(f"checkpoint {path} holds a scalar-head net, this VecBrain trains a C51 net (support {support})")
    if saved is not None and support is None:
        raise ValueError(f"checkpoint {path} holds a C51 net (support {saved}), this VecBrain has a scalar head")
    if saved is not None and (int(saved[0]), float(saved[1]), float(saved[2])) != (int(support[0]), float(support[1]), float(support[2])):
        raise ValueError(f"checkpoint {path} was trained on the support {saved} (n_atoms, v_min, v_max), this VecBrain has {tuple(support)}")


def backend_name(be):
    return getattr(be, 'name', type(be).__name__)


def require(be, flag, text):
    """the capability test: a backend that does not offer `flag` refuses: 'the <name> backend <text>'"""
    if not getattr(be, flag, False):
        raise ValueError(f"the {backend_name(be)} backend {text}")


def resolve_args(be, algo, arch, world, n_step, noisy, acting_noise, initial_epsilon, n_atoms, v_min, v_max, n_quantiles, kappa, tau, alpha, clip,
                 huber, max_grad_norm, polyak):
    """every refusal of VecBrain(...) that needs none of the backend's factories, in the order they fire (arguments, then what the backend
    `be` offers, per head family) -> (arch, support, quantiles, munchausen, huber, max_grad_norm, polyak, initial_epsilon) as the brain
    holds them: the head's own arch; None for what the algo does not have (huber: None on the distributional heads, which neither set
    nor record it).  sigma0 is checked where the noisy net is made."""
    from .vec import check_huber, check_max_grad_norm, check_munchausen, check_polyak, check_quantiles, check_support
    if acting_noise not in ("shared", "env"):
        raise ValueError(f"acting_noise must be 'shared' or 'env', got {acting_noise!r}")
    if acting_noise == "env" and not noisy:
        raise ValueError("acting_noise='env' needs a noisy net (noisy=True)")
    if initial_epsilon is None:
        initial_epsilon = 0.0 if noisy else 0.03
    if not 1 <= n_step <= 16:
        raise ValueError(f"n_step must be in 1..16, got {n_step}")
    if acting_noise == "env":
        require(be, "acting_noise_env", "has no per-env acting noise (acting_noise_env): acting_noise='env' needs it")
    support = quantiles = munchausen = None
    delta = check_huber(huber)
    if algo not in SCALAR_ALGOS:
        if delta > 0.0:
            raise ValueError(f"huber = {huber}: the Huber loss is offered on the scalar heads only ({', '.join(SCALAR_ALGOS)}), not with "
                             f"algo {algo!r} (QR has its own kappa)")
        delta = None
    elif delta > 0.0:
        require(be, "huber", f"has no Huber loss (huber): huber = {huber} needs it")
    limit = check_max_grad_norm(max_grad_norm)
    rho = check_polyak(polyak, allow_off=True)
    if limit > 0.0:
        require(be, "grad_clip", f"has no gradient clipping (grad_clip): max_grad_norm = {max_grad_norm} needs it")
    if rho > 0.0:
        require(be, "polyak", f"has no soft target updates (polyak): polyak = {polyak} needs it")
    one_step = f"has no one-call prioritized step (per_one_step): algo {algo!r} needs it"
    if algo == "doubleper":
        if arch not in ("plain", "dueling"):
            raise ValueError(f"algo {algo!r} trains the scalar heads: arch must be 'plain' or 'dueling', not {arch!r}")
        if noisy:
            raise ValueError(f"noisy=True: noisy layers are offered on the C51 heads only, not with algo {algo!r}")
        require(be, "double_per", f"has no Double-DQN with prioritized replay (double_per): algo {algo!r} needs it")
        require(be, "per_one_step", one_step)
    if algo in MDQN_ALGOS:
        munchausen = check_munchausen(tau, alpha, clip)
        if arch not in ("plain", "dueling"):
            raise ValueError(f"algo {algo!r} (Munchausen-DQN) trains the scalar heads: arch must be 'plain' or 'dueling', not {arch!r}")
        if noisy:
            raise ValueError(f"noisy=True: noisy layers are offered on the C51 heads only, not with the Munchausen-DQN algo {algo!r}")
        require(be, "mdqn", f"has no Munchausen-DQN (mdqn): algo {algo!r} needs it")
        if algo == "mdqnper":
            require(be, "per_one_step", one_step)
    elif algo in QR_ALGOS + QR_PER_ALGOS:
        if arch not in ("plain",) + QR_HEADS:
            raise ValueError(f"algo {algo!r} builds a QR head on the plain trunk: arch {arch!r} is not one (dueling QR is arch='qrdueling')")
        if world > 1:
            raise ValueError(f"algo {algo!r}: data-parallel QR is not supported (world = {world}; one GPU only)")
        if noisy:
            raise ValueError(f"noisy=True: noisy layers are offered on the C51 heads only, not with the QR algo {algo!r}")
        require(be, "qr", "has no QR nets")
        if algo in QR_PER_ALGOS:
            require(be, "per_one_step", one_step)
        quantiles = check_quantiles(n_quantiles, kappa)
        arch = "qrdueling" if arch == "qrdueling" else "qr"
    elif arch in QR_HEADS:
        raise ValueError(f"arch {arch!r} is a QR head: it trains with a QR algo ('qr', 'qrdouble', 'qrper', 'qrdoubleper'), not {algo!r}")
    elif algo in C51_ALGOS + C51_PER_ALGOS:
        if arch not in ("plain",) + C51_HEADS:
            raise ValueError(f"algo {algo!r} builds a C51 head on the plain trunk: arch {arch!r} is not one "
                             f"(dueling C51 is arch='c51dueling')")
        if world > 1:
            raise ValueError(f"algo {algo!r}: data-parallel C51 is not supported (world = {world}; one GPU only)")
        require(be, "c51", "has no C51 nets")
        if arch == "c51dueling":
            require(be, "c51_dueling", "has no dueling C51 nets")
        if algo in C51_PER_ALGOS:
            require(be, "per_one_step", one_step)
        if noisy:
            require(be, "c51_noisy", "has no noisy C51 nets")
        support = check_support(n_atoms, v_min, v_max)
        arch = "c51dueling" if arch == "c51dueling" else "c51"
    elif noisy:
        raise ValueError(f"noisy=True: noisy layers are offered on the C51 heads only, which train with a C51 algo ('c51', 'c51double', "
                         f"'c51per', 'c51doubleper'), not {algo!r}")
    elif arch == "c51dueling":
        raise ValueError(f"arch {arch!r} is a C51 head: it trains with a C51 algo ('c51', 'c51double', 'c51per', 'c51doubleper'), "
                         f"not {algo!r}")
    if n_step > 1 and algo in PER_ALGOS:
        require(be, "per_n_step", f"offers n-step returns on uniform replay only: algo {algo!r} takes n_step = 1 there")
    return arch, support, quantiles, munchausen, delta, limit, rho, initial_epsilon


PRIORITY_INIT_ALGOS = ("per", "doubleper")                   # ... which the acting Q-values give for a max target on a scalar head only


def check_priority_init(be, algo, world, priority_init):
    """the refusals of VecBrain(priority_init=...), before anything touches the GPU -> the setting.  'td' (Ape-X initial priorities,
    include/fbdqn.h fb_replay_set_priority_init): algo 'per' / 'doubleper', one rank, a backend with per_priority_init and the one-call
    prioritized step that issues the prime (per_one_step: the composed-calls fallback of step() never primes)"""
    from .vec import PRIORITY_INITS
    if priority_init not in PRIORITY_INITS:
        raise ValueError(f"priority_init must be one of {PRIORITY_INITS}, got {priority_init!r}")
    if priority_init == "max":
        return priority_init
    if algo == "mdqnper":
        raise ValueError(f"priority_init='td' is not offered with algo {algo!r}: its target is a soft value, not the max the acting Q-values give")
    if algo not in PRIORITY_INIT_ALGOS:
        raise ValueError(f"priority_init='td' needs algo 'per' or 'doubleper' (|TD| of a scalar head's max target), not {algo!r}")
    if world > 1:
        raise ValueError(f"priority_init='td': data parallel is not supported (world = {world}; one GPU only)")
    require(be, "per_priority_init", "has no TD initial priorities (per_priority_init): priority_init='td' needs it")
    require(be, "per_one_step", "has no one-call prioritized step (per_one_step): priority_init='td' is primed inside it")
    return priority_init


def check_checkpoint_priority_init(z, priority_init, path):
    """a checkpoint's memory was filled under the setting it records (no key: 'max' -- every checkpoint of before the setting, and every
    one a 'max' brain writes); a brain takes one written under its own setting only"""
    saved = str(z["priority_init"][0]) if "priority_init" in z.files else "max"
    if saved != priority_init:
        raise ValueError(f"checkpoint {path} was written with priority_init = {saved!r}, this VecBrain has priority_init = {priority_init!r}")


class VecBrain:
    def __init__(self, n_envs, algo="dqn", arch="plain", batch=32, capacity=1_000_000, fc_width=512, seed=0,
                 observe=1000, explore=1_000_000, initial_epsilon=None, final_epsilon=0.0, gamma=0.99,
                 replace_target_iter=500, sampler=None, rank=0, world=1, backend=None, n_step=1, n_atoms=51, v_min=-10.0, v_max=10.0,
                 noisy=False, sigma0=0.5, acting_noise="shared", n_quantiles=51, kappa=1.0, tau=0.03, alpha=0.9, clip=-1.0, huber=0.0,
                 max_grad_norm=0.0, polyak=0.0, priority_init="max"):
        """n_step > 1: learn from n-step returns (include/fbdqn.h: the uniform replay's n-step view, fb_replay_set_n_step; a prioritized
        memory created with n-step returns, fb_replay_create_nstep, on a backend with per_n_step).
        algo 'c51' / 'c51double': distributional Q-learning on n_atoms atoms over [v_min, v_max] (one GPU, uniform replay, plain trunk);
        'c51per' / 'c51doubleper': the same with prioritized replay (importance-weighted loss, KL priorities; n_step at creation).
        arch='c51dueling' (C51 algos only): the dueling C51 head -- value and advantage distributions (include/fbdqn.h).
        noisy=True (C51 algos only): noisy fc1 and head layers, sigma initialised to sigma0 / sqrt(fan_in); the exploration comes from
        the noise, so initial_epsilon defaults to 0 (0.03 without noise, the reference's); an explicit initial_epsilon is honoured.
        acting_noise (noisy nets): 'shared' -- one noise sample per step for all envs -- or 'env': independent noise per env when acting
        (include/fbdqn.h); training is the same in both, and checkpoints do not record it.
        algo 'qr' / 'qrdouble' / 'qrper' / 'qrdoubleper': QR-DQN with n_quantiles quantiles and the quantile Huber loss's kappa (one GPU,
        any n_step; the PER forms on a prioritized memory), on arch 'qr' ('plain' means it) or 'qrdueling'; no noisy QR nets.
        algo 'mdqn' / 'mdqnper': Munchausen-DQN on arch 'plain' or 'dueling' -- the target is a soft (log-sum-exp, temperature tau)
        bootstrap plus alpha x the log-policy of the taken action, clipped below at clip (include/fbdqn.h); 'mdqnper' on a prioritized
        memory; any n_step (only the first step's bonus is added), world > 1 as 'double' / 'per'; tau / alpha / clip are ignored otherwise.
        algo 'doubleper': 'double''s target (a* from the online net, its value from the target net) with 'per''s weighted loss and
        priorities, on a prioritized memory; arch 'plain' or 'dueling', any n_step, world > 1 as 'per'.
        huber=delta > 0 (scalar algos only -- 'dqn', 'nature', 'double', 'per', 'doubleper', 'mdqn', 'mdqnper'): the Huber loss, d^2 inside
        |d| <= delta and delta (2 |d| - delta) outside (include/fbdqn.h); 0 = the squared loss.  Checkpoints record it.
        max_grad_norm=G > 0 (every algo and head): the flat gradient is scaled by G / max(norm, G) before Adam (tf.clip_by_global_norm;
        include/fbdqn.h); world > 1: the reduced gradient is clipped, so every rank applies the same scale.  run() logs the last norm.
        polyak=rho in (0, 1] (every algo): after every train step target += rho (online - target) (net.soft_sync_target), and the hard
        copy every replace_target_iter steps is dropped.  This gives the 'per' family -- 'per', whose target net the reference agent never
        syncs, included -- a moving target.  Both are optimiser settings: checkpoints record them, load() does not refuse another value.
        priority_init='td' (algo 'per' / 'doubleper', world 1): a new transition's leaf gets the |TD error| of the Q-values computed to act
        (Ape-X; include/fbdqn.h fb_replay_prime_priorities) one step after its store instead of waiting at the tree's maximum to be
        sampled; the memory runs in its fast mode.  'max': the reference's Memory.store.  Checkpoints record it."""
        n_step, noisy, be = int(n_step), bool(noisy), backend or HipVecBackend()
        self.priority_init = check_priority_init(be, algo, world, priority_init)
        (arch, self.support, self.quantiles, self.munchausen, self.huber, self.max_grad_norm, self.polyak, initial_epsilon) = resolve_args(
            be, algo, arch, world, n_step, noisy, acting_noise, initial_epsilon, n_atoms, v_min, v_max, n_quantiles, kappa, tau, alpha, clip, huber,
            max_grad_norm, polyak)                           # (every refusal but the two below comes before anything touches the GPU)
        from .vec import bootstrap_gamma
        self.be = be
        self.n, self.algo, self.batch, self.gamma = n_envs, algo, batch, gamma
        self.n_step = n_step
        self.boot_gamma = bootstrap_gamma(gamma, n_step)     # Gamma = gamma^n as the running product
        self.rank, self.world = rank, world
        self.observe, self.explore = observe, explore
        self.epsilon, self.initial_epsilon, self.final_epsilon = initial_epsilon, initial_epsilon, final_epsilon
        self.replace_target_iter = replace_target_iter
        self.seed = seed
        # the world: envs, memory, nets
        self.env = be.env(n_envs, seed + 1000003 * rank)     # envs shard by rank: every rank plays its own games
        if n_step > 1 and algo in PER_ALGOS:                 # ... into its own replay shard (a prioritized one gets n at creation)
            self.replay = be.replay(capacity, n_envs, True, n_step=n_step, gamma=gamma)
        else:
            self.replay = be.replay(capacity, n_envs, algo in PER_ALGOS)
        self.replay.seed(seed + rank, sampler)
        if n_step > 1 and algo not in PER_ALGOS:             # (only then: a backend without n-step memories keeps working at n = 1)
            if not hasattr(self.replay, "set_n_step"):
                raise ValueError(f"the {backend_name(be)} backend's replay has no n-step view (n_step = {n_step})")
            self.replay.set_n_step(n_step, gamma)
        if self.priority_init == "td":                       # (the level-wise tree: the reference has no update order for this store)
            self.replay.set_per_mode("fast")
            self.replay.set_priority_init("td", gamma)
        self.arch = arch
        self.noisy = noisy
        self.sigma0 = None
        if noisy:
            from .vec import check_sigma0
            self.sigma0 = check_sigma0(sigma0)
            self.net = be.net(2, fc_width, arch, max(n_envs, batch), support=self.support, noisy=True, sigma0=self.sigma0)
        elif self.quantiles:
            self.net = be.net(2, fc_width, arch, max(n_envs, batch), quantiles=self.quantiles)
        else:
            self.net = be.net(2, fc_width, arch, max(n_envs, batch), support=self.support) if self.support else be.net(2, fc_width, arch, max(n_envs, batch))
        if self.munchausen:
            self.net.set_munchausen(*self.munchausen)
        if self.huber:
            self.net.set_huber(self.huber)
        if self.max_grad_norm:
            self.net.set_max_grad_norm(self.max_grad_norm)
        self.acting_noise = acting_noise
        if acting_noise == "env":
            self.net.set_acting_noise("env")                 # (fb_vec_step reads it: act with per-env noise, draw the online sample after)
        self.net.init_params(seed=seed, which=0)             # the same draw on every rank
        self.net.init_params(seed=seed + 1, which=1)
        if world > 1:                                        # replicas start from rank 0's parameters, bit for bit
            for which in (0, 1):
                flat = self.net.store_params(which)
                fdist.broadcast_params(flat, src=0)
                self.net.load_params(flat, which)
        self.grad = be.zeros(self.net.n_params) if world > 1 else None
        # one all-reduce of the flat gradient per train step (the HIP backend can split it in two: dist.OverlappedAllReduce)
        self.reduce = None
        if self.grad is not None:
            mk = getattr(be, "reducer", None)
            self.reduce = mk(self.net, self.grad, MEAN_LOSS[algo]) if mk else (lambda: fdist.allreduce_gradients(self.grad, MEAN_LOSS[algo]))
        self.timeStep = 0
        self.onlineTimeStep = 0
        self.nib = self.env.track_state()                    # currentState of every env, maintained by the env kernel
        self.env.observe()
        self.replay.reset(self.env.frame_bits)
        self.stats = self.env.track_stats()                  # [episodes, score sum, score max, pipes passed], kept by the env kernel
        self.last_loss = None
        self.dtype = "f32"
        # the step: the whole of it is one host call (fb_vec_step): uniform replay with the head, random.sample and the Memory append riding in the
        # env launch; prioritized replay with store -> Memory.sample -> weighted train -> batch_update as launches of the same call
        self.native = None
        if self.grad is not None and algo not in PER_ALGOS and hasattr(be, "native"):
            self.native = be.native(rank, world)
        if algo in PER_ALGOS and not getattr(be, "per_one_step", False):
            self.one_step = None                             # (a backend without the fused prioritized step: the separate calls below)
        elif self.native is not None:
            self.one_step = be.step(self.env, self.replay, self.net, batch, algo, gamma, self.grad, dist=self.native, mean_loss=MEAN_LOSS[algo])
        else:
            self.one_step = be.step(self.env, self.replay, self.net, batch, algo, gamma, self.grad)

    def _hard_sync_due(self):
        """the periodic target copy, unless soft updates replace it"""
        return not self.polyak and self.algo in TARGET_SYNC and self.timeStep % self.replace_target_iter == 0

    def _apply_reduced(self):
        """data parallel without the library's communicator: all-reduce, clip the reduced gradient (the net never clips an exported one), Adam"""
        self.reduce()
        if self.max_grad_norm:
            self.net.clip_grad(self.grad)
        self.net.apply_adam(self.grad)

    def train_step(self, idx=None):
        if self._hard_sync_due():
            self.net.sync_target()
        isw = None
        if idx is None:
            idx, isw = self.replay.sample(self.batch)
        if hasattr(self.be, "train_from_replay") and self.batch <= 256:
            # the conv trunk reads the sampled transitions' frame bits in the ring: no gather launch, no u8 copies
            loss, abs_err = self.be.train_from_replay(self.replay, self.net, self.algo, idx, isw, self.gamma, self.grad, self.algo in PER_ALGOS)
        else:
            s, a, r, s2, t = self.replay.gather(idx)
            loss, abs_err, _ = self.net.train_step(self.algo, s, a, r, s2, t, isw=isw, gamma=self.boot_gamma, flat_grad=self.grad,
                                                   want_aux=self.algo in PER_ALGOS)
        if self.grad is not None:
            self._apply_reduced()
        if self.algo in PER_ALGOS:
            self.replay.update_priorities(idx, abs_err=abs_err)
        if self.polyak:
            self.net.soft_sync_target(self.polyak)
        self.last_loss = loss

    def step(self):
        if self.one_step is not None:
            training = self.onlineTimeStep > self.observe
            if training and self._hard_sync_due():
                self.net.sync_target()                       # acting reads the online net only: same result as syncing before training
            self.one_step(self.epsilon, seed=self.seed + self.rank, step=self.timeStep, train=training)
            if self.epsilon > self.final_epsilon and self.onlineTimeStep > self.observe:
                self.epsilon -= (self.initial_epsilon - self.final_epsilon) / self.explore
            if training:
                if self.grad is not None and self.native is None:      # (fb_vec_step_dp has reduced, clipped and applied already)
                    self._apply_reduced()
                if self.polyak:
                    self.net.soft_sync_target(self.polyak)
                self.last_loss = self.one_step.loss
            self.timeStep += 1
            self.onlineTimeStep += 1
            return
        actions = self.net.act_nib(self.nib, self.epsilon, seed=self.seed + self.rank, step=self.timeStep)
        if self.epsilon > self.final_epsilon and self.onlineTimeStep > self.observe:
            self.epsilon -= (self.initial_epsilon - self.final_epsilon) / self.explore
        _, reward, terminal, _ = self.env.frame_step(actions, want_u8=False)
        training = self.onlineTimeStep > self.observe
        idx = None
        if training and self.algo not in PER_ALGOS:          # store + random.sample in one launch (same indices)
            idx = self.replay.push_sample(self.env.frame_bits, actions, reward, terminal, self.batch)
        else:
            self.replay.push(self.env.frame_bits, actions, reward, terminal)
        if training:
            self.train_step(idx)
        self.timeStep += 1
        self.onlineTimeStep += 1

    def evaluate(self, n_envs=4096, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0, noise="mean"):
        """Greedy play of n_envs fresh games with the online net as it stands (dqnflappybird_amd.evaluate): changes nothing the
        training that follows reads -- nets, Adam, envs, frame stacks, stats, replay, the step counters.  A noisy net plays with its
        mean weights (noise='sample': one sample keyed by act_seed); its online sample is put back afterwards (the last step's draw)."""
        from .evaluate import evaluate
        res = evaluate(self.net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed, noise=noise)
        if self.noisy:                                       # (fb_vec_step drew the online noise at (seed + rank, timeStep - 1) last)
            if self.timeStep > 0:
                self.net.reset_noise(0, self.seed + self.rank, self.timeStep - 1)
            else:
                self.net.mean_noise(0)
        return res

    def set_dtype(self, dtype="f32"):
        """'bf16' = BASELINE.json configs[2]'s arithmetic for acting AND training (fp32 master weights / Adam); 'f32' = default."""
        self.net.set_inference_dtype(dtype)
        self.net.set_train_dtype(dtype)
        self.dtype = dtype

    # ------------------------------------------------------------------ checkpoint / resume of the WHOLE loop
    def _local_path(self, path):
        """where this rank's LOCAL state goes: `<path>.rank<r>.npz` (envs, frame stacks, replay shard and stats differ per rank)"""
        base = str(path)[:-4] if str(path).endswith(".npz") else str(path)
        return f"{base}.rank{self.rank}.npz"

    def save(self, path):
        """Everything the device-resident loop needs to continue bit for bit: both nets + Adam slots (what the reference saves,
        BrainDQN.py:227-233), the three scalars, AND what it forgets (:176-192): the replay memory (frame ring, a / r / t, sampler
        generator, SumTree), onlineTimeStep, every env's state and the agents' frame stacks.

        world = 1: one file, `path`.  world > 1: the REPLICATED part (nets, Adam, scalars -- bit-identical on every rank) is written by
        rank 0 alone to `path`; every rank writes its own envs / frame stacks / replay shard / stats to `<path>.rank<r>.npz`.  (All ranks
        writing `path` -- round 3 -- overwrote each other's rank-local state.)  A barrier closes the call: when it returns on any rank,
        every file of the checkpoint is complete."""
        import numpy as np
        shared = core_arrays(self.net if self.rank == 0 else None, self.env, self.nib, self.stats, self.replay)
        local = {k: shared.pop(k) for k in LOCAL_ARRAYS if k in shared}
        if self.rank == 0:
            shared.update(scalars=np.array([self.timeStep, self.onlineTimeStep, self.world, self.seed], np.int64),
                          epsilon=np.array([self.epsilon], np.float64), n_step=np.array([self.n_step], np.int64))
            if self.support is not None:                     # (scalar-head checkpoints carry no support)
                shared["support"] = np.array(self.support, np.float64)
                shared["head"] = np.array([self.arch])       # 'c51' or 'c51dueling' (checkpoints without it: 'c51')
            if self.quantiles is not None:                   # QR: the head ('qr' / 'qrdueling') and (N, kappa)
                shared["head"] = np.array([self.arch])
                shared["quantiles"] = np.array(self.quantiles, np.float64)
            if self.munchausen is not None:                  # Munchausen-DQN: (tau, alpha, l0) the nets were trained with
                shared["munchausen"] = np.array(self.munchausen, np.float64)
            if self.huber:                                   # the Huber delta the nets were trained with (no key: 0, the squared loss)
                shared["huber"] = np.array([self.huber], np.float64)
            if self.max_grad_norm:                           # optimiser settings (no key: 0 = off), recorded like huber's: only when on
                shared["max_grad_norm"] = np.array([self.max_grad_norm], np.float64)
            if self.polyak:
                shared["polyak"] = np.array([self.polyak], np.float64)
            if self.priority_init == "td":                   # (no key: 'max'; world 1 only) with the record of acting-time Q-values
                rows, first, last = self.replay.prime_state()
                shared.update(priority_init=np.array(["td"]), prime_rows=rows, prime_span=np.array([first, last], np.int64))
            if self.noisy:                                   # online / target / Adam hold [mu | sigma] (checkpoints without it: not noisy)
                shared["noisy"] = np.array([1], np.int64)
                shared["sigma0"] = np.array([self.sigma0], np.float64)
        if self.world == 1:
            np.savez(npz_path(path), **shared, **local)
            return
        np.savez(self._local_path(path), **local)
        if self.rank == 0:
            np.savez(npz_path(path), **shared)
        fdist.barrier()

    def load(self, path):
        """the inverse of save(); at world > 1 every rank reads the replicated part from `path` and its own `<path>.rank<r>.npz`
        (the world size must be the one the checkpoint was written with: the shards are rank-local)."""
        import numpy as np
        z = np.load(npz_path(path))
        refuse_foreign_head(z, path, OTHER_LOOPS.get)        # (an actor-critic net has the dueling net's parameter count: the head tells)
        saved_world = int(z["scalars"][2]) if len(z["scalars"]) > 2 else 1
        if saved_world != self.world:
            raise ValueError(f"checkpoint {path} was written by {saved_world} rank(s), this job has {self.world}")
        saved_n = int(z["n_step"][0]) if "n_step" in z.files else 1          # (checkpoints from before n-step returns: one-step)
        if saved_n != self.n_step:
            raise ValueError(f"checkpoint {path} was trained with n_step = {saved_n}, this VecBrain has n_step = {self.n_step}")
        check_checkpoint_quantiles(z, self.quantiles, self.arch, path)
        check_checkpoint_support(z, self.support, path)
        if self.support is not None:
            check_checkpoint_head(z, self.arch, path)
        check_checkpoint_noisy(z, self.noisy, self.sigma0, path)
        check_checkpoint_munchausen(z, self.munchausen, path)
        check_checkpoint_huber(z, self.huber, path)
        check_checkpoint_priority_init(z, self.priority_init, path)
        # (max_grad_norm / polyak: optimiser settings, like the learning rate -- this brain's own values go on, whatever the file records)
        self.checkpoint_optimiser = checkpoint_optimiser(z)
        zl = np.load(self._local_path(path)) if self.world > 1 else z
        dev = self.be.to_device if hasattr(self.be, "to_device") else np.ascontiguousarray
        restore_core(z, self.net, self.env, self.nib, self.stats, self.replay, dev, local=zl)
        if self.priority_init == "td":                       # (behind the memory's blob, which clears the record)
            self.replay.load_prime_state(z["prime_rows"], *z["prime_span"].tolist())
        self.timeStep, self.onlineTimeStep = int(z["scalars"][0]), int(z["scalars"][1])
        if len(z["scalars"]) > 3:
            self.seed = int(z["scalars"][3])                     # the key of the acting (epsilon-greedy) stream: (seed + rank, timeStep)
        self.epsilon = float(z["epsilon"][0])
        if hasattr(self.be, "synchronize"):
            self.be.synchronize()

    def run(self, steps, log_every=100):
        for i in range(steps):
            self.step()
            if log_every and (i + 1) % log_every == 0:
                loss = self.last_loss.item() if self.last_loss is not None else float("nan")
                score = score_text(self.net, self.stats)
                if hasattr(self.net, "split_stats"):
                    self.net.split_stats()                       # (at the same sync: a wait between the two streams of fb_vec_step's split schedule that gave up raises)
                clip = clip_text(self.net, self.max_grad_norm)
                print(f"TIMESTEP {self.timeStep} / ENVS {self.n} / EPSILON {self.epsilon:.6f} / {score} / LOSS {loss:.6g}{clip}", flush=True)
