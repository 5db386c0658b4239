"""On-device policy evaluation: greedy (or epsilon-greedy) play of many fresh games with a fixed net (fb_eval_run, include/fbdqn.h).

    from dqnflappybird_amd.evaluate import evaluate
    res = evaluate(net, n_envs=4096, episodes=1)        # net: vec.QNet (VecBrain.net); its online parameters, read only
    print(res.summary())

    python -m dqnflappybird_amd.evaluate CHECKPOINT.npz --envs 4096 --episodes 1

The loop runs on the device: the acting forward, the head, the game step and the episode records stay in HBM; the host reads one
live-env count every 32 vector steps and the records once at the end.  Envs that have finished their episodes are compacted away,
so a few long games do not keep every row of the acting forward busy.
"""
import argparse
import ctypes as C
import time

import numpy as np

from . import _lib as L


class EvalResult:
    """score / length (int32) and truncated (uint8) arrays [n_envs, episodes]: the records of fb_eval_run.  length == 0 marks an
    episode that was never reached; truncated == 1 one the step cap cut (score and length so far).  The statistics are taken over
    every recorded episode (completed and truncated)."""

    def __init__(self, score, length, truncated, steps, wall_s, rows_launched=0, compactions=0):
        self.score, self.length, self.truncated = score, length, truncated
        self.steps, self.wall_s = int(steps), float(wall_s)
        self.rows_launched, self.compactions = int(rows_launched), int(compactions)
        rec = length > 0
        s = score[rec].astype(np.float64)
        self.episodes = int(rec.sum())
        self.env_steps = int(length.sum(dtype=np.int64))          # every frame_step belongs to exactly one recorded episode
        self.truncated_count = int(truncated.sum())
        have = s.size > 0
        self.mean_score = float(s.mean()) if have else float("nan")
        self.median_score = float(np.median(s)) if have else float("nan")
        self.p10_score = float(np.percentile(s, 10)) if have else float("nan")
        self.p90_score = float(np.percentile(s, 90)) if have else float("nan")
        self.max_score = int(s.max()) if have else 0
        self.mean_length = float(length[rec].mean()) if have else float("nan")
        self.env_steps_per_s = self.env_steps / self.wall_s if self.wall_s > 0 else float("nan")

    @property
    def rows_per_live_row(self):
        """acting rows launched / env-steps actually taken (1.0 = no row was ever stepped for a finished env)"""
        return self.rows_launched / self.env_steps if self.env_steps else float("nan")

    def summary(self):
        n = self.score.shape[0]
        return (f"EVAL ENVS {n} / EPISODES {self.episodes} / TRUNCATED {self.truncated_count} / MEAN_SCORE {self.mean_score:.3f} / "
                f"MEDIAN {self.median_score:.1f} / P10 {self.p10_score:.1f} / P90 {self.p90_score:.1f} / MAX_SCORE {self.max_score} / "
                f"MEAN_LENGTH {self.mean_length:.1f} / STEPS {self.steps} / ENV_STEPS {self.env_steps} / "
                f"ENV_STEPS_PER_S {self.env_steps_per_s:.4g} / WALL_S {self.wall_s:.3f}")


class Evaluator:
    """An fb_eval handle for up to max_envs games (its own env states, nibble ping-pong buffers, maps and counters)."""

    def __init__(self, max_envs):
        import torch
        L.require_gpu()
        self.max_envs = int(max_envs)
        self.h = C.c_void_p()
        blob = L.sprite_blob()
        L.check(L.lib().fb_eval_create(self.max_envs, blob, len(blob), C.byref(self.h)), "fb_eval_create")
        self._torch = torch

    def __del__(self):
        try:
            if getattr(self, "h", None) and self.h.value:
                L.lib().fb_eval_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def run(self, net, n_envs, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0):
        torch = self._torch
        n, e = int(n_envs), int(episodes)
        shape = (max(n, 1), max(e, 1))
        score = torch.empty(shape, dtype=torch.int32, device="cuda")
        length = torch.empty(shape, dtype=torch.int32, device="cuda")
        trunc = torch.empty(shape, dtype=torch.uint8, device="cuda")
        steps = C.c_int64()
        t0 = time.perf_counter()
        L.check(L.lib().fb_eval_run(self.h, net.h, n, e, int(max_steps), float(epsilon), int(env_seed), int(act_seed),
                                    L.ptr(score), L.ptr(length), L.ptr(trunc), C.byref(steps), L.current_stream()), "fb_eval_run")
        wall = time.perf_counter() - t0                      # (fb_eval_run returns synchronised)
        rows, comp = C.c_int64(), C.c_int64()
        L.check(L.lib().fb_eval_stats(self.h, C.byref(rows), C.byref(comp)), "fb_eval_stats")
        return EvalResult(score.cpu().numpy(), length.cpu().numpy(), trunc.cpu().numpy(), steps.value, wall, rows.value, comp.value)


NOISE_MODES = ("mean", "sample")


def evaluate(net, n_envs, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0, noise="mean"):
    """Play `episodes` episodes in each of n_envs fresh games (env e = env e of VecGameState(n_envs, env_seed)) with the online
    parameters of `net` (vec.QNet, in its current inference dtype), at most max_steps vector steps.  A noisy net plays with its mean
    weights (noise='mean': mu), or noise='sample' with one sample of its online noise keyed by (act_seed, step 0); either leaves
    the net's online sample set that way.  -> EvalResult."""
    if not 1 <= int(n_envs) <= L.EVAL_MAX_ENVS:               # (the library checks it too; this keeps the handle's size sane)
        raise ValueError(f"evaluate: n_envs={n_envs} outside 1..{L.EVAL_MAX_ENVS}")
    if noise not in NOISE_MODES:
        raise ValueError(f"evaluate: noise must be one of {NOISE_MODES}, got {noise!r}")
    if getattr(net, "noisy", False):
        net.reset_noise(L.NET_ONLINE, int(act_seed), 0, mean=noise == "mean")
    elif noise != "mean":
        raise ValueError("evaluate: noise='sample' needs a noisy net")
    return Evaluator(n_envs).run(net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed)


def qnet_from_checkpoint(path, fc_width=512, dtype="f32", max_batch=1024):
    """The online net of a VecBrain.save or VecActorCritic.save checkpoint (an actor-critic net by its recorded head 'ac'; plain or dueling, told apart by the parameter count; C51 by its recorded support, and
    C51 or dueling C51 by its recorded head -- 'c51' where none is recorded; a noisy net by its recorded `noisy` / `sigma0`, in mean
    mode; a QR net by its recorded `quantiles` and head).  max_batch sizes the net's
    workspace: evaluation runs its acting forward in passes of up to 3 * max_batch rows."""
    from .vec import QNet
    z = np.load(path if str(path).endswith(".npz") else str(path) + ".npz")
    online = np.ascontiguousarray(z["online"], np.float32)
    if "head" in z.files and str(z["head"][0]) == "ac":      # an actor-critic net (VecActorCritic): greedy play is the policy's argmax
        net = QNet(2, fc_width, "ac", max_batch=max_batch)
        if net.n_params != online.size:
            raise ValueError(f"{path}: {online.size} online parameters do not match an actor-critic net of width {fc_width}")
        if dtype != "f32":
            raise ValueError(f"{path}: an actor-critic net computes in f32 only (dtype {dtype!r})")
        net.load_params(online, 0)
        return net
    if "head" in z.files and str(z["head"][0]) == "sac":     # a SAC net (VecSAC): greedy play is the policy's argmax
        net = QNet(2, fc_width, "sac", max_batch=max_batch)
        if net.n_params != online.size:
            raise ValueError(f"{path}: {online.size} online parameters do not match a SAC net of width {fc_width}")
        if dtype != "f32":
            raise ValueError(f"{path}: a SAC net computes in f32 only (dtype {dtype!r})")
        net.load_params(online, 0)
        return net
    if "head" in z.files and str(z["head"][0]) == "iqn":     # an IQN net (VecIQN): greedy play on the folded head, under the file's risk setting
        n_tau, n_tau_next, n_tau_act, kappa, cvar = z["iqn"].tolist()
        dueling = bool(int(z["dueling"][0])) if "dueling" in z.files else False      # (a file without the key: a plain IQN net)
        noisy = "noisy" in z.files and bool(z["noisy"][0])                           # (... nor `noisy`: not noisy; a noisy net starts in mean mode)
        from .veciqn import iqn_arch
        kw = dict(sigma0=float(z["sigma0"][0])) if noisy else {}
        net = QNet(2, fc_width, iqn_arch(dueling, noisy), max_batch=max_batch, n_tau=int(n_tau), n_tau_next=int(n_tau_next), n_tau_act=int(n_tau_act), kappa=kappa, **kw)
        if net.n_params != online.size:
            raise ValueError(f"{path}: {online.size} online parameters do not match {'a dueling' if dueling else 'an'} {'noisy ' if noisy else ''}IQN net of width {fc_width}")
        if dtype != "f32":
            raise ValueError(f"{path}: an IQN net computes in f32 only (dtype {dtype!r})")
        net.load_params(online, 0)
        net.set_iqn_risk(cvar)
        return net
    if "quantiles" in z.files:                               # a QR net (VecBrain records its head and (N, kappa))
        n_q, kappa = z["quantiles"].tolist()
        head = str(z["head"][0])
        if head not in ("qr", "qrdueling"):
            raise ValueError(f"{path}: unknown QR head {head!r}")
        net = QNet(2, fc_width, head, max_batch=max_batch, n_quantiles=int(n_q), kappa=kappa)
        if net.n_params != online.size:
            raise ValueError(f"{path}: {online.size} online parameters do not match a {head} net of width {fc_width} and {int(n_q)} quantiles")
        net.load_params(online, 0)
        net.set_inference_dtype(dtype)
        return net
    if "support" in z.files:                                 # a C51 net (VecBrain records its support)
        n_atoms, v_min, v_max = z["support"].tolist()
        head = str(z["head"][0]) if "head" in z.files else "c51"
        if head not in ("c51", "c51dueling"):
            raise ValueError(f"{path}: unknown C51 head {head!r}")
        noisy = "noisy" in z.files and bool(z["noisy"][0])
        kw = dict(noisy=True, sigma0=float(z["sigma0"][0])) if noisy else {}
        net = QNet(2, fc_width, head, max_batch=max_batch, n_atoms=int(n_atoms), v_min=v_min, v_max=v_max, **kw)
        if net.n_params != online.size:
            raise ValueError(f"{path}: {online.size} online parameters do not match a {'noisy ' if noisy else ''}{head} net of width "
                             f"{fc_width} and {int(n_atoms)} atoms")
        net.load_params(online, 0)
        net.set_inference_dtype(dtype)
        return net
    for arch in ("plain", "dueling"):
        net = QNet(2, fc_width, arch, max_batch=max_batch)
        if net.n_params == online.size:
            net.load_params(online, 0)
            net.set_inference_dtype(dtype)
            return net
    raise ValueError(f"{path}: {online.size} online parameters match neither a plain nor a dueling net of width {fc_width}")


def main(argv=None):
    ap = argparse.ArgumentParser(description="evaluate the online net of a VecBrain checkpoint on the GPU")
    ap.add_argument("checkpoint")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--episodes", type=int, default=1)
    ap.add_argument("--max-steps", type=int, default=100_000)
    ap.add_argument("--epsilon", type=float, default=0.0)
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32")
    ap.add_argument("--fc-width", type=int, default=512)
    ap.add_argument("--env-seed", type=int, default=0)
    ap.add_argument("--act-seed", type=int, default=0)
    ap.add_argument("--noise", choices=NOISE_MODES, default="mean", help="noisy nets: play with the mean weights, or one noise sample keyed by --act-seed")
    a = ap.parse_args(argv)
    net = qnet_from_checkpoint(a.checkpoint, a.fc_width, a.dtype)
    res = evaluate(net, a.envs, a.episodes, a.max_steps, a.epsilon, a.env_seed, a.act_seed, noise=a.noise)
    print(res.summary(), flush=True)
    return res


if __name__ == "__main__":
    main()
