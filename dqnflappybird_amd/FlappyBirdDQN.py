"""Drop-in for FlappyBirdDQN.py of the reference (driver :25-82): `--model` dispatch, `preprocess`,
and the getAction -> frame_step -> preprocess -> setPerception loop, on the MI355X.

    python -m dqnflappybird_amd.FlappyBirdDQN --model dqn [--steps N] [--quiet]
    python -m dqnflappybird_amd.FlappyBirdDQN --model dqn --vec 1024 --steps N      (vectorised loop)
    python -m dqnflappybird_amd.FlappyBirdDQN --model dqn --vec 1024 --n-step 3     (... learning from 3-step returns)
    python -m dqnflappybird_amd.FlappyBirdDQN --model c51 --vec 1024                (distributional C51, vectorised loop only)
    python -m dqnflappybird_amd.FlappyBirdDQN --model c51per --vec 1024 --n-step 3  (C51 + prioritized replay + 3-step returns;
                                                                                       c51doubleper: with the double target)
    python -m dqnflappybird_amd.FlappyBirdDQN --model rainbow --vec 1024 --n-step 3 (the same with the dueling C51 head: Rainbow
                                                                                       without noisy nets)
    python -m dqnflappybird_amd.FlappyBirdDQN --model rainbow --vec 1024 --n-step 3 --noisy   (full Rainbow: noisy fc1 and head
                                                                                       layers, epsilon 0; --noisy takes any C51 model)
    python -m dqnflappybird_amd.FlappyBirdDQN --model qrdqn --vec 1024               (QR-DQN: quantile head, quantile Huber loss;
                                                                                       qrdqnper: with prioritized replay; qrrainbow:
                                                                                       dueling QR head, double target, PER; --n-quantiles,
                                                                                       --kappa)
    python -m dqnflappybird_amd.FlappyBirdDQN --model mdqn --vec 1024 [--tau 0.03 --alpha 0.9 --clip -1] [--n-step K]
                                                                                      (Munchausen-DQN on the scalar head: soft bootstrap +
                                                                                       clipped log-policy bonus; mdqnper: prioritized replay)
    python -m dqnflappybird_amd.FlappyBirdDQN --model doubleper --vec 1024 [--n-step K] [--huber 1]
                                                                                      (Double-DQN's target with prioritized replay on the scalar
                                                                                       head; --huber D: the Huber loss on any scalar-head model)
    python -m dqnflappybird_amd.FlappyBirdDQN --model doubleper --vec 1024 --n-step 3 --max-grad-norm 10 --polyak 0.005
                                                                                      (any --vec model: clip the gradient's global norm to G;
                                                                                       soft target updates with rate RHO after every train step
                                                                                       in place of the periodic copy)
    python -m dqnflappybird_amd.FlappyBirdDQN --model rainbow --vec 1024 --n-step 3 --noisy --acting-noise env
                                                                                      (... acting with independent noise per env)
    python -m dqnflappybird_amd.FlappyBirdDQN --model rainbowiqn --dueling --vec 1024 --n-step 3 --sigma0 0.5 --acting-noise env
                                                                                      (full Rainbow-IQN: noisy fc1 and head layers on the
                                                                                       IQN net at sigma0 0.5, epsilon 0; --sigma0 takes any IQN model)

`actorcritic` / `policygradient` are out of scope (broken in the reference).
"""
import argparse

import numpy as np

from . import _lib as L


def preprocess(observ, _env=[None]):
    """cv2.resize(observ, (80, 80)) -> COLOR_BGR2GRAY -> threshold(1, 255) (reference :31-34) as one
    HIP kernel; observ is the array3d frame u8[288,512,3]."""
    import ctypes as C
    import torch
    from .vec import VecGameState
    if _env[0] is None:
        _env[0] = VecGameState(1)
    rgb = torch.from_numpy(np.ascontiguousarray(observ, np.uint8)).cuda()
    out = torch.empty((80, 80), dtype=torch.uint8, device="cuda")
    L.check(L.lib().fb_preprocess_rgb(_env[0].h, L.ptr(rgb), 1, L.ptr(out), L.current_stream()), "fb_preprocess_rgb")
    return np.reshape(out.cpu().numpy(), (80, 80, 1))


def model_class(name):
    from .BrainDQN import BrainDQN
    from .BrainDQNNature import BrainDQNNature
    from .BrainDoubleDQN import BrainDoubleDQN
    from .BrainDuelingDQN_CC import BrainDuelingDQN
    from .BrainPrioritizedReplyDQN import BrainPrioritizedReplyDQN
    from .BrainActorCritic import BrainDQNActorCritic
    from .BrainPolicyGradient import BrainPolicyGradient
    table = {"dqn": BrainDQN, "ddqn": BrainDoubleDQN, "dqnnature": BrainDQNNature, "duelingdqn": BrainDuelingDQN,
             "prioritydqn": BrainPrioritizedReplyDQN, "actorcritic": BrainDQNActorCritic, "policygradient": BrainPolicyGradient}
    if name not in table:
        print("invalid model!")
        raise SystemExit(1)
    return table[name]


def playFlappyBird(model, steps=None, verbose=True):
    from .game import wrapped_flappy_bird as game
    brain = model_class(model)(2, 'bird', verbose=verbose)
    flappyBird = game.GameState()
    action0 = np.array([1, 0])
    observation0, reward0, terminal, curScore = flappyBird.frame_step(action0)
    observation0 = preprocess(observation0).reshape(80, 80)
    brain.setInitState(observation0)
    n = 0
    while steps is None or n < steps:
        action = brain.getAction()
        nextObserv, reward, terminal, curScore = flappyBird.frame_step(action)
        nextObserv = preprocess(nextObserv)
        brain.setPerception(nextObserv, action, reward, terminal, curScore)
        n += 1
    return brain


def optimiser_kwargs(args, parser):
    """--max-grad-norm / --polyak as VecBrain's keywords; bad values and a missing --vec are parser errors, before anything touches the GPU"""
    kw = {}
    if args.max_grad_norm is None and args.polyak is None:
        return kw
    if not args.vec:
        parser.error("--max-grad-norm / --polyak need --vec: the single-env agents are the reference's, which neither clip nor update softly")
    from .vec import check_max_grad_norm, check_polyak
    try:
        if args.max_grad_norm is not None:
            kw["max_grad_norm"] = check_max_grad_norm(args.max_grad_norm)
        if args.polyak is not None:
            kw["polyak"] = check_polyak(args.polyak, allow_off=True)
    except ValueError as e:
        parser.error(str(e))
    return kw


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--model")
    parser.add_argument("--steps", type=int, default=None)
    parser.add_argument("--quiet", action="store_true")
    parser.add_argument("--vec", type=int, default=0, help="run N vectorised envs (device-resident loop)")
    parser.add_argument("--n-step", type=int, default=1, help="learn from K-step returns (--vec, uniform replay; --model iqnper | rainbowiqn | sacper: prioritized; "
                                                                      "1 = the reference's one-step TD)")
    parser.add_argument("--priority-init", choices=("max", "td"), default=None, help="--model prioritydqn | doubleper with --vec: a new transition's priority -- "
                        "max (the default: the tree's maximum, the reference's) or td (the |TD error| of the Q-values computed to act, Ape-X)")
    parser.add_argument("--noisy", action="store_true", help="noisy fc1 and head layers, epsilon 0 (--model c51 | c51per | c51doubleper | rainbow, --vec)")
    parser.add_argument("--acting-noise", choices=("shared", "env"), default="shared",
                        help="--noisy / --sigma0: act with one noise sample for all envs (shared, the default) or independent noise per env (env)")
    parser.add_argument("--sigma0", type=float, default=None, metavar="S",
                        help="--model iqn | iqnper | rainbowiqn: noisy fc1 and head layers at sigma0 = S (0.5 is Fortunato et al.'s), epsilon 0; "
                             "--model rainbowiqn --dueling --n-step 3 --sigma0 0.5 --acting-noise env is full Rainbow-IQN")
    parser.add_argument("--n-quantiles", type=int, default=None, help="QR models: the number of quantiles N (default 51)")
    parser.add_argument("--kappa", type=float, default=None, help="QR models and --model iqn: the quantile Huber loss's threshold (default 1)")
    parser.add_argument("--n-tau", type=int, default=None, help="--model iqn: quantile fractions sampled per transition for the online net N (default 8)")
    parser.add_argument("--n-tau-target", type=int, default=None, help="--model iqn: quantile fractions sampled for the target N' (default 8)")
    parser.add_argument("--n-tau-act", type=int, default=None, help="--model iqn: the acting grid K (default 32)")
    parser.add_argument("--cvar", type=float, default=None, help="--model iqn: act on CVaR_ETA, 0 < ETA <= 1 (default 1 = the mean)")
    parser.add_argument("--double", action="store_true", help="--model iqn | iqnper: the greedy next action from the online net (Double-DQN's target; --model rainbowiqn sets it)")
    parser.add_argument("--dueling", action="store_true", help="--model iqn | iqnper | rainbowiqn: the dueling IQN net (value and advantage quantile streams); "
                                                                "--model rainbowiqn --dueling --n-step 3 is Rainbow-IQN without noisy nets")
    parser.add_argument("--munchausen", action="store_true", help="--model iqn | iqnper: Munchausen IQN -- the soft target and the log-policy bonus "
                                                                   "(--tau, --alpha, --clip as for mdqn; not with --double)")
    parser.add_argument("--tau", type=float, default=None, help="--model mdqn | mdqnper, --munchausen: the softmax temperature (default 0.03)")
    parser.add_argument("--alpha", type=float, default=None, help="--model mdqn | mdqnper, --munchausen: the scale of the log-policy bonus (default 0.9); "
                                                                   "--model sac: the temperature (default 0.2)")
    parser.add_argument("--clip", type=float, default=None, help="--model mdqn | mdqnper, --munchausen: the bonus's lower clip l0 (default -1)")
    parser.add_argument("--huber", type=float, default=None, help="scalar-head models with --vec: the Huber loss's delta (default 0 = the squared loss)")
    parser.add_argument("--max-grad-norm", type=float, default=None, help="--vec: clip the gradient's global norm to G before Adam (default 0 = no clipping)")
    parser.add_argument("--polyak", type=float, default=None, help="--vec: soft target updates, target += RHO (online - target) after every train step, "
                                                                    "in place of the periodic copy (default 0 = off)")
    parser.add_argument("--rollout", type=int, default=None, help="--model a2c: env steps per update T (default 5, at most 128)")
    parser.add_argument("--gae-lambda", type=float, default=None, help="--model a2c: lambda of the generalised advantage estimate (default 0.95)")
    parser.add_argument("--value-coef", type=float, default=None, help="--model a2c: the value loss's coefficient (default 0.5)")
    parser.add_argument("--entropy-coef", type=float, default=None, help="--model a2c: the entropy bonus's coefficient (default 0.01)")
    parser.add_argument("--epochs", type=int, default=None, help="--model ppo: passes over each rollout K (default 4)")
    parser.add_argument("--minibatches", type=int, default=None, help="--model ppo: minibatches per pass M, a divisor of rollout x envs (default 4)")
    parser.add_argument("--clip-eps", type=float, default=None, help="--model ppo: the probability ratio is clipped to [1 - E, 1 + E] (default 0.2)")
    parser.add_argument("--value-clip", type=float, default=None, help="--model ppo: clip the value around the rollout's by C (default 0 = off)")
    parser.add_argument("--no-adv-norm", action="store_true", help="--model ppo: do not normalise the rollout's advantages")
    parser.add_argument("--adv-norm-scope", default=None, help="--model ppo: normalise the advantages over the rollout (the default) or over every minibatch")
    parser.add_argument("--target-kl", type=float, default=None, help="--model ppo: stop an update's epochs once an epoch's mean approximate KL exceeds "
                                                                       "1.5 X (default 0 = off)")
    parser.add_argument("--anneal-lr", action="store_true", help="--model ppo: the learning rate falls linearly to 0 over the run's --steps updates")
    parser.add_argument("--target-entropy", type=float, default=None, help="--model sac | sacper: the entropy the learned temperature aims at (default 0.98 ln 2)")
    parser.add_argument("--alpha-lr", type=float, default=None, help="--model sac | sacper: the temperature's learning rate (default 0 = --alpha stays fixed)")
    return parser


SAC_MODELS = ("sac", "sacper")                           # sacper: SAC on a prioritized memory, which also takes --n-step


def sac_kwargs(args, parser):
    """--model sac's (sacper's: the same, and --n-step) options as VecSAC's keywords (--alpha is the temperature there, default 0.2);
    everything is refused here, by name, before anything touches the GPU"""
    given = [n for n, v in (("--target-entropy", args.target_entropy), ("--alpha-lr", args.alpha_lr)) if v is not None]
    if args.model not in SAC_MODELS:
        if given:
            parser.error(f"{' / '.join(given)} need --model sac, not --model {args.model}")
        return None
    per = args.model == "sacper"
    if not args.vec:
        parser.error(f"--model {args.model} needs --vec: discrete soft actor-critic runs in the vectorised loop only")
    for name, on in (("--noisy", args.noisy), ("--n-step", args.n_step != 1 and not per), ("--huber", args.huber is not None),
                     ("--tau / --clip", args.tau is not None or args.clip is not None),
                     ("--n-quantiles / --kappa", args.n_quantiles is not None or args.kappa is not None)):
        if on:
            parser.error(f"{name} is not an option of --model {args.model} (--alpha, --target-entropy, --alpha-lr, --polyak, --max-grad-norm"
                         f"{', --n-step' if per else ''} are)"
                         + (" -- n-step SAC runs on the prioritized memory: --model sacper --n-step K" if name == "--n-step" else ""))
    from .vecsac import check_args, check_replay
    kw = dict(alpha=0.2 if args.alpha is None else args.alpha, target_entropy=args.target_entropy, alpha_lr=0.0 if args.alpha_lr is None else args.alpha_lr,
              polyak=0.005 if args.polyak is None else args.polyak, max_grad_norm=0.0 if args.max_grad_norm is None else args.max_grad_norm)
    try:
        checked = check_args(args.vec, min(32, args.vec), kw["alpha"], kw["target_entropy"], kw["alpha_lr"], kw["polyak"], 100, 0.99, 1e-4,
                             kw["max_grad_norm"], None)
        if per:
            check_replay(True, args.n_step, checked[0], checked[6], checked[10])
    except ValueError as e:
        parser.error(str(e))
    kw["batch"] = min(32, args.vec)
    if per:                                              # (--model sac: VecSAC's keywords are the ones of before)
        kw.update(prioritized=True, n_step=args.n_step)
    return kw


IQN_MODELS = ("iqn", "iqnper", "rainbowiqn")             # iqnper: IQN on a prioritized memory; rainbowiqn: iqnper with --double; --dueling: the dueling net in each


def iqn_kwargs(args, parser):
    """--model iqn's (iqnper's, rainbowiqn's: the same) options as VecIQN's keywords; everything is refused here, by name, before anything
    touches the GPU"""
    given = [n for n, v in (("--n-tau", args.n_tau), ("--n-tau-target", args.n_tau_target), ("--n-tau-act", args.n_tau_act), ("--cvar", args.cvar),
                            ("--double", args.double or None), ("--dueling", args.dueling or None)) if v is not None]
    if args.munchausen and args.model not in ("iqn", "iqnper"):      # (rainbowiqn sets --double, which the soft target has no use for)
        parser.error(f"--munchausen needs --model iqn or --model iqnper, not --model {args.model}"
                     + (" (its --double target chooses a greedy next action; the Munchausen target has none)" if args.model == "rainbowiqn" else
                        " (Munchausen-DQN on the scalar heads is --model mdqn | mdqnper)"))
    if args.model not in IQN_MODELS:
        if given:
            parser.error(f"{' / '.join(given)} need --model iqn, not --model {args.model}")
        if args.sigma0 is not None:
            parser.error(f"--sigma0 needs an IQN model ({', '.join(IQN_MODELS)}), not --model {args.model}"
                         + (" (its noisy layers are --noisy, at sigma0 0.5)" if args.model in ("c51", "c51per", "c51doubleper", "rainbow") else ""))
        return None
    if not args.vec:
        parser.error(f"--model {args.model} needs --vec: implicit quantile networks run in the vectorised loop only")
    for name, on in (("--noisy", args.noisy), ("--huber", args.huber is not None), ("--n-quantiles", args.n_quantiles is not None),
                     ("--tau / --alpha / --clip", not args.munchausen and (args.tau is not None or args.alpha is not None or args.clip is not None))):
        if on:
            parser.error(f"{name} is not an option of --model {args.model} (--n-tau, --n-tau-target, --n-tau-act, --kappa, --cvar, --double, --n-step, "
                         "--polyak, --max-grad-norm are)")
    if args.acting_noise != "shared" and args.sigma0 is None:
        parser.error(f"--acting-noise {args.acting_noise} needs --noisy (the IQN models' noisy layers: --sigma0 S)")
    from .veciqn import check_args
    kw = dict(batch=min(32, args.vec), double_q=args.double or args.model == "rainbowiqn", n_step=args.n_step, n_tau=8 if args.n_tau is None else args.n_tau,
              n_tau_next=8 if args.n_tau_target is None else args.n_tau_target, n_tau_act=32 if args.n_tau_act is None else args.n_tau_act,
              kappa=1.0 if args.kappa is None else args.kappa, cvar=1.0 if args.cvar is None else args.cvar,
              polyak=0.0 if args.polyak is None else args.polyak, max_grad_norm=0.0 if args.max_grad_norm is None else args.max_grad_norm)
    try:
        check_args(args.vec, kw["batch"], kw["n_tau"], kw["n_tau_next"], kw["n_tau_act"], kw["kappa"], kw["cvar"], kw["n_step"], kw["polyak"], 500, 1000,
                   1_000_000, 0.03, 0.0, 0.99, 1e-6, kw["max_grad_norm"], None)
    except ValueError as e:
        parser.error(str(e))
    kw["prioritized"] = args.model != "iqn"
    if args.sigma0 is not None:                          # (without the flag VecIQN's keywords are the ones of before)
        from .veciqn import check_noisy
        try:
            _, s0, an = check_noisy(True, args.sigma0, args.acting_noise)
        except ValueError as e:
            parser.error(str(e).replace("sigma0 must", "--sigma0 must"))
        kw.update(noisy=True, sigma0=s0, acting_noise=an)
    if args.dueling:                                     # (without the flag VecIQN's keywords are the ones of before)
        kw["dueling"] = True
    if args.munchausen:                                  # (the same; --tau is the softmax temperature, VecIQN's `temp`)
        from .veciqn import check_munchausen
        try:
            _, t, a, c = check_munchausen(True, 0.03 if args.tau is None else args.tau, 0.9 if args.alpha is None else args.alpha,
                                          -1.0 if args.clip is None else args.clip, kw["double_q"])
        except ValueError as e:
            parser.error(str(e).replace("munchausen=True with double_q=True", "--munchausen with --double").replace("temp must", "--tau must"))
        kw.update(munchausen=True, temp=t, alpha=a, clip=c)
    return kw


def a2c_kwargs(args, parser):
    """--model a2c's and --model ppo's options as VecActorCritic's keywords; everything is refused here, before anything touches the GPU"""
    given = [n for n, v in (("--rollout", args.rollout), ("--gae-lambda", args.gae_lambda), ("--value-coef", args.value_coef),
                            ("--entropy-coef", args.entropy_coef)) if v is not None]
    ppo_given = [n for n, v in (("--epochs", args.epochs), ("--minibatches", args.minibatches), ("--clip-eps", args.clip_eps),
                                ("--value-clip", args.value_clip), ("--no-adv-norm", args.no_adv_norm or None),
                                ("--adv-norm-scope", args.adv_norm_scope), ("--target-kl", args.target_kl), ("--anneal-lr", args.anneal_lr or None))
                 if v is not None]
    if ppo_given and args.model != "ppo":
        parser.error(f"{' / '.join(ppo_given)} need --model ppo, not --model {args.model}")
    if args.model not in ("a2c", "ppo"):
        if given:
            parser.error(f"{' / '.join(given)} need --model a2c, not --model {args.model}")
        return None
    if not args.vec:
        parser.error(f"--model {args.model} needs --vec: the advantage actor-critic runs in the vectorised loop only")
    for name, on in (("--noisy", args.noisy), ("--n-step", args.n_step != 1), ("--huber", args.huber is not None), ("--polyak", args.polyak is not None),
                     ("--tau / --alpha / --clip", args.tau is not None or args.alpha is not None or args.clip is not None),
                     ("--n-quantiles / --kappa", args.n_quantiles is not None or args.kappa is not None)):
        if on:
            parser.error(f"{name} is not an option of --model {args.model} (--rollout, --gae-lambda, --value-coef, --entropy-coef, --max-grad-norm"
                         f"{', --epochs, --minibatches, --clip-eps, --value-clip, --no-adv-norm, --adv-norm-scope, --target-kl, --anneal-lr' if args.model == 'ppo' else ''} are)")
    from .vecac import check_args, check_ppo_args, check_ppo_options
    kw = dict(rollout=5 if args.rollout is None else args.rollout, gae_lambda=0.95 if args.gae_lambda is None else args.gae_lambda,
              value_coef=0.5 if args.value_coef is None else args.value_coef, entropy_coef=0.01 if args.entropy_coef is None else args.entropy_coef,
              max_grad_norm=0.0 if args.max_grad_norm is None else args.max_grad_norm)
    try:
        check_args(args.vec, kw["rollout"], 0.99, kw["gae_lambda"], kw["value_coef"], kw["entropy_coef"], kw["max_grad_norm"])
        if args.model == "ppo":
            kw.update(algo="ppo", epochs=4 if args.epochs is None else args.epochs, minibatches=4 if args.minibatches is None else args.minibatches,
                      clip_eps=0.2 if args.clip_eps is None else args.clip_eps, value_clip=0.0 if args.value_clip is None else args.value_clip,
                      normalize_adv=not args.no_adv_norm)
            check_ppo_args(args.vec, kw["rollout"], kw["epochs"], kw["minibatches"], kw["clip_eps"], kw["value_clip"])
            if args.adv_norm_scope is not None:              # (without the three flags VecActorCritic's keywords are the ones of before)
                kw["adv_norm_scope"] = args.adv_norm_scope
            if args.target_kl is not None:
                kw["target_kl"] = args.target_kl
            if args.anneal_lr:                               # (--steps is the run's length in updates: the schedule's end)
                kw.update(anneal_lr=True, total_updates=args.steps or 1000)
            check_ppo_options(kw.get("adv_norm_scope", "rollout"), kw.get("target_kl"), kw.get("anneal_lr", False), kw.get("total_updates"), None,
                              kw["normalize_adv"])
    except ValueError as e:
        parser.error(str(e))
    return kw


PRIORITY_INIT_MODELS = ("prioritydqn", "doubleper")      # the models whose acting Q-values give a stored transition's |TD error|


def priority_init_kwargs(args, parser):
    """--priority-init -> VecBrain's keyword; every other model refuses td by name (before anything touches the GPU)"""
    if args.priority_init is None:
        return {}
    if args.priority_init == "td":
        if args.model not in PRIORITY_INIT_MODELS:
            parser.error(f"--priority-init td needs --model {' | '.join(PRIORITY_INIT_MODELS)}, not --model {args.model}")
        if not args.vec:
            parser.error("--priority-init td needs --vec: the single-env agents are the reference's, which store at the tree's maximum")
    return dict(priority_init=args.priority_init) if args.vec and args.model in PRIORITY_INIT_MODELS else {}


def main():
    parser = build_parser()
    args = parser.parse_args()
    pkw = priority_init_kwargs(args, parser)             # (refused before anything touches the GPU)
    okw = optimiser_kwargs(args, parser)                 # (refused before anything touches the GPU)
    akw = a2c_kwargs(args, parser)
    skw = sac_kwargs(args, parser)
    ikw = iqn_kwargs(args, parser)
    if ikw is not None:                                  # implicit quantile networks: a class of its own, one GPU
        from .veciqn import VecIQN
        VecIQN(args.vec, **ikw).run(args.steps or 1000, log_every=0 if args.quiet else 100)
        return
    if skw is not None:                                  # the off-policy stochastic-policy learner: a class of its own, one GPU
        from .vecsac import VecSAC
        VecSAC(args.vec, **skw).run(args.steps or 1000, log_every=0 if args.quiet else 100)
        return
    if akw is not None:                                  # the on-policy learner: a class of its own, one GPU (--steps: updates)
        from .vecac import VecActorCritic
        VecActorCritic(args.vec, **akw).run(args.steps or 1000, log_every=0 if args.quiet else 100)
        return
    qr_models = ("qrdqn", "qrdqnper", "qrrainbow")
    md_models = ("mdqn", "mdqnper")
    scalar_models = ("dqn", "ddqn", "dqnnature", "duelingdqn", "prioritydqn", "doubleper") + md_models
    if args.model == "doubleper":                        # (refused before anything touches the GPU)
        if not args.vec:
            parser.error("--model doubleper needs --vec: Double-DQN with prioritized replay runs in the vectorised loop only")
        if args.noisy:
            parser.error(f"--noisy needs a C51 model (c51, c51per, c51doubleper, rainbow), not --model {args.model}")
    hkw = {}
    if args.huber is not None:                           # (refused before anything touches the GPU)
        if not args.vec:
            parser.error("--huber needs --vec: the single-env agents are the reference's, with its squared loss")
        if args.model not in scalar_models:
            parser.error(f"--huber needs a scalar-head model ({', '.join(scalar_models)}), not --model {args.model}")
        from .vec import check_huber
        try:
            hkw = dict(huber=check_huber(args.huber))
        except ValueError as e:
            parser.error(str(e))
    if args.model in md_models:                          # (refused before anything touches the GPU)
        if not args.vec:
            parser.error(f"--model {args.model} needs --vec: Munchausen-DQN runs in the vectorised loop only")
        if args.noisy:
            parser.error(f"--noisy needs a C51 model (c51, c51per, c51doubleper, rainbow), not --model {args.model}")
        from .vec import MDQN_DEFAULTS, check_munchausen
        try:
            mkw = dict(zip(("tau", "alpha", "clip"), check_munchausen(*(d if v is None else v for v, d in
                                                                       zip((args.tau, args.alpha, args.clip), MDQN_DEFAULTS)))))
        except ValueError as e:
            parser.error(str(e))
    elif args.tau is not None or args.alpha is not None or args.clip is not None:
        parser.error(f"--tau / --alpha / --clip need a Munchausen model ({', '.join(md_models)}), not --model {args.model}")
    if args.model in qr_models:                          # (refused before anything touches the GPU)
        if not args.vec:
            parser.error(f"--model {args.model} needs --vec: QR-DQN runs in the vectorised loop only")
        if args.noisy:
            parser.error(f"--noisy needs a C51 model (c51, c51per, c51doubleper, rainbow), not --model {args.model}")
        from .vec import check_quantiles
        try:
            check_quantiles(51 if args.n_quantiles is None else args.n_quantiles, 1.0 if args.kappa is None else args.kappa)
        except ValueError as e:
            parser.error(str(e))
    elif args.n_quantiles is not None or args.kappa is not None:
        parser.error(f"--n-quantiles / --kappa need a QR model ({', '.join(qr_models)}), not --model {args.model}")
    if args.acting_noise != "shared" and not args.noisy:      # (refused before anything touches the GPU)
        parser.error(f"--acting-noise {args.acting_noise} needs --noisy")
    if args.noisy:                                       # (refused before anything touches the GPU)
        if args.model not in ("c51", "c51per", "c51doubleper", "rainbow"):
            parser.error(f"--noisy needs a C51 model (c51, c51per, c51doubleper, rainbow), not --model {args.model}")
        if not args.vec:
            parser.error("--noisy needs --vec: noisy nets run in the vectorised loop only")
    if args.model in ("c51", "c51per", "c51doubleper", "rainbow") and not args.vec:    # (not reference agents: the single-env dispatch stays the reference's)
        parser.error(f"--model {args.model} needs --vec: distributional C51 runs in the vectorised loop only")
    if args.n_step != 1:                                 # (refused before anything touches the GPU)
        if not 1 <= args.n_step <= L.NSTEP_MAX:
            parser.error(f"--n-step must be in 1..{L.NSTEP_MAX}")
        if not args.vec:
            parser.error("--n-step needs --vec: the single-env agents are the reference's one-step algorithms")
        if args.model == "prioritydqn":
            parser.error("--n-step on this command line needs uniform replay: prioritydqn takes --n-step 1 here "
                         "(prioritized replay with n-step returns is VecBrain(algo='per', n_step=K))")
    if args.vec:
        # one process per GPU (python -m torch.distributed.run --nproc-per-node N -m dqnflappybird_amd.FlappyBirdDQN ...):
        # --vec envs PER RANK, rank-local replay, one RCCL all-reduce of the flat gradient per train step
        from . import dist as fdist
        from .vecbrain import VecBrain
        rank, _, world = fdist.init()
        if args.model in ("actorcritic", "policygradient"):
            raise SystemExit("--vec runs the DQN family; the actor-critic / policy-gradient agents are single-env (as in the reference)")
        algo = {"dqn": "dqn", "ddqn": "nature", "dqnnature": "nature", "duelingdqn": "nature", "prioritydqn": "per", "c51": "c51",
                "c51per": "c51per", "c51doubleper": "c51doubleper", "rainbow": "c51doubleper", "qrdqn": "qr", "qrdqnper": "qrper",
                "qrrainbow": "qrdoubleper", "mdqn": "mdqn", "mdqnper": "mdqnper", "doubleper": "doubleper"}[args.model]
        arch = "c51dueling" if args.model == "rainbow" else "plain"      # rainbow: dueling C51 head, double target, prioritized replay
        qkw = {}
        if args.model in qr_models:                      # qrrainbow: dueling QR head, double target, prioritized replay
            arch = "qrdueling" if args.model == "qrrainbow" else "qr"
            qkw = dict(n_quantiles=51 if args.n_quantiles is None else args.n_quantiles, kappa=1.0 if args.kappa is None else args.kappa)
        if args.model in md_models:
            qkw = mkw
        vb = VecBrain(args.vec, algo=algo, arch=arch, rank=rank, world=world, n_step=args.n_step, noisy=args.noisy,
                      acting_noise=args.acting_noise, **qkw, **hkw, **okw, **pkw)
        vb.run(args.steps or 1000, log_every=0 if (args.quiet or rank) else 100)
    else:
        playFlappyBird(args.model, args.steps, verbose=not args.quiet)


if __name__ == '__main__':
    main()
