"""VecSAC: discrete soft actor-critic (Haarnoja et al. 2018; Christodoulou 2019) on the vectorised loop, entirely device resident.

    step:  sample the policy for N envs -> frame_step -> store + draw a minibatch           (vec.SacStep, ONE host call)
           -> [after `observe` steps] the SAC train step on the minibatch, read from the replay ring in place:
              soft target from the target net's two Q heads, both critic losses, the actor's loss, [the temperature's Adam step]
           -> target <- target + polyak (online - target)

One net (a policy head and two Q heads on the shared trunk), one GPU, a uniform memory; include/fbdqn.h pins the semantics, DESIGN.md
section 18 the schedule.  The policy is stochastic: there is no epsilon; evaluate() plays its argmax.
"""
import numpy as np

SAC_HEAD = "sac"                                             # what a checkpoint of this class records as its head


def check_args(n_envs, batch, alpha, target_entropy, alpha_lr, polyak, observe, gamma, lr, max_grad_norm, capacity):
    """every argument check of VecSAC that needs no GPU -> the checked values"""
    from .vec import check_max_grad_norm, check_polyak, check_sac
    n, b, ob = int(n_envs), int(batch), int(observe)
    if n < 1:
        raise ValueError(f"n_envs must be >= 1, got {n_envs}")
    if not 1 <= b <= 256:
        raise ValueError(f"batch must be in 1..256, got {batch}")
    if b > n:
        raise ValueError(f"batch {b} > n_envs {n}: every step draws a minibatch, the first from one push of n_envs transitions")
    a, h, alr = check_sac(alpha, target_entropy, alpha_lr, 2)
    rho = check_polyak(polyak, allow_off=True)
    if ob < 0:
        raise ValueError(f"observe must be >= 0, got {observe}")
    g, l = float(gamma), float(lr)
    if not (np.isfinite(g) and 0.0 <= g <= 1.0):
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    if not (np.isfinite(l) and l > 0.0):
        raise ValueError(f"lr must be finite and > 0, got {lr}")
    cap = max(65536, 8 * n) if capacity is None else int(capacity)
    if cap < 2 * n:
        raise ValueError(f"capacity {cap} < 2 x n_envs = {2 * n}")
    return n, b, a, h, alr, rho, ob, g, l, check_max_grad_norm(max_grad_norm), cap


class VecSAC:
    def __init__(self, n_envs, batch=32, alpha=0.2, target_entropy=None, alpha_lr=0.0, polyak=0.005, observe=100, gamma=0.99, lr=1e-4,
                 max_grad_norm=0, fc_width=512, seed=0, capacity=None):
        """n_envs games; every step trains one minibatch of `batch` transitions (<= n_envs, <= 256) once `observe` steps have filled
        the memory.  alpha: the temperature (its start when alpha_lr > 0, which learns it towards the entropy target_entropy, default
        0.98 ln 2); polyak: the soft target update's rate per step (0 = never); lr is Adam's; max_grad_norm=G > 0 clips the gradient's
        global norm; capacity: the memory's (default max(65536, 8 n_envs))."""
        (self.n, self.batch, self.alpha, self.target_entropy, self.alpha_lr, self.polyak, self.observe, self.gamma, self.lr, self.max_grad_norm,
         self.capacity) = check_args(n_envs, batch, alpha, target_entropy, alpha_lr, polyak, observe, gamma, lr, max_grad_norm, capacity)
        from .vec import QNet, SacStep, VecGameState, VecReplay
        self.seed = int(seed)
        self.fc_width = int(fc_width)
        self.env = VecGameState(self.n, seed=self.seed)
        self.replay = VecReplay(self.capacity, self.n)
        self.replay.seed(self.seed)
        self.net = QNet(2, self.fc_width, "sac", max_batch=max(self.n, self.batch))
        self.net.set_hparams(lr=self.lr)
        self.net.set_sac(self.alpha, self.target_entropy, self.alpha_lr)
        if self.max_grad_norm:
            self.net.set_max_grad_norm(self.max_grad_norm)
        self.net.init_params(seed=self.seed, which=0)
        self.net.sync_target()
        self.nib = self.env.track_state()
        self.env.observe()
        self.replay.reset(self.env.frame_bits)
        self.stats = self.env.track_stats()
        self.one_step = SacStep(self.env, self.replay, self.net, self.batch, self.gamma, self.polyak)
        self.losses = self.one_step.loss
        self.timeStep = 0                                    # env steps per env so far: the key of the policy's draws

    def step(self):
        """one vector step -> the six loss numbers f32[6] (device): total, Q1's, Q2's, the actor's, the entropy, alpha"""
        self.one_step(seed=self.seed, step=self.timeStep, train=self.timeStep >= self.observe)
        self.timeStep += 1
        return self.losses

    def evaluate(self, n_envs=4096, episodes=1, max_steps=100_000, epsilon=0.0, env_seed=0, act_seed=0):
        """Greedy play (the policy's argmax) of n_envs fresh games with the net as it stands (dqnflappybird_amd.evaluate): changes
        nothing the training that follows reads"""
        from .evaluate import evaluate
        return evaluate(self.net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed)

    # ------------------------------------------------------------------ checkpoint / resume
    @staticmethod
    def _npz(path):
        return path if str(path).endswith(".npz") else str(path) + ".npz"

    def save(self, path):
        """everything the loop needs to continue bit for bit: the nets, Adam, the temperature's five words, every env's state and frame
        stack, the stats, the memory (with its generator), the counters and the settings; `head` = 'sac' tells the file from the other
        loops'"""
        host = lambda t: t.cpu().numpy()
        m, v, pows = self.net.adam_state()
        np.savez(self._npz(path), head=np.array([SAC_HEAD]), online=host(self.net.store_params(0)), target=host(self.net.store_params(1)),
                 adam_m=host(m), adam_v=host(v), beta_pows=np.asarray(pows, np.float32), sac_state=self.net.sac_state(),
                 scalars=np.array([self.timeStep, self.seed, self.n, self.batch, self.fc_width, self.observe], np.int64),
                 sac=np.array([self.gamma, self.target_entropy, self.alpha_lr, self.polyak, self.max_grad_norm, self.lr], np.float64),
                 env_state=self.env.get_state(), nib=host(self.nib), stats=host(self.stats), replay=self.replay.state_blob())

    def load(self, path):
        """the inverse of save(), into a VecSAC made with the same n_envs, batch, fc_width, capacity and seed; the settings of the file
        replace this object's"""
        import torch
        from .vec import SacStep
        from .vecbrain import checkpoint_head
        z = np.load(self._npz(path))
        head = checkpoint_head(z)
        if head != SAC_HEAD:
            raise ValueError(f"checkpoint {path} holds a {head} head (another loop's), this is a VecSAC (head {SAC_HEAD!r})")
        sc = [int(x) for x in z["scalars"]]
        if (sc[2], sc[3], sc[4]) != (self.n, self.batch, self.fc_width):
            raise ValueError(f"checkpoint {path} was written with (n_envs, batch, fc_width) = {tuple(sc[2:5])}, this VecSAC has "
                             f"{(self.n, self.batch, self.fc_width)}")
        if sc[1] != self.seed:
            raise ValueError(f"checkpoint {path} was written with seed {sc[1]}, this VecSAC has seed {self.seed} (the envs' pipe-gap "
                             "streams are keyed by it)")
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        self.net.load_params(z["online"], 0)
        self.net.load_params(z["target"], 1)
        self.net.set_adam_state(dev(z["adam_m"]), dev(z["adam_v"]), z["beta_pows"])
        self.gamma, self.target_entropy, self.alpha_lr, self.polyak, self.max_grad_norm, self.lr = (float(x) for x in z["sac"])
        self.net.set_hparams(lr=self.lr)
        self.net.set_max_grad_norm(self.max_grad_norm)
        st = np.asarray(z["sac_state"], np.float32)
        self.net.set_sac(float(np.exp(st[0])), self.target_entropy, self.alpha_lr)
        self.net.set_sac_state(st)                           # (the five words as they were: log alpha is not re-derived)
        self.alpha = self.net.sac()[0]
        self.observe = sc[5]
        self.env.set_state(z["env_state"])
        self.nib.copy_(dev(z["nib"]))
        self.stats[...] = dev(z["stats"])
        self.replay.load_state_blob(z["replay"])
        self.timeStep = sc[0]
        self.one_step = SacStep(self.env, self.replay, self.net, self.batch, self.gamma, self.polyak)
        self.losses = self.one_step.loss
        torch.cuda.synchronize()

    def run(self, steps, log_every=1000):
        for i in range(steps):
            losses = self.step()
            if log_every and (i + 1) % log_every == 0:
                tot, q1, q2, lpi, ent, alpha = losses.tolist()   # the only host sync of the loop, once per log line
                ep, ssum, smax, pipes = self.stats.tolist()
                self.net.check_range()
                clip = ""
                if self.max_grad_norm:
                    norm, scale = self.net.grad_norm()
                    clip = f" / GRAD_NORM {norm:.6g} / CLIP_SCALE {scale:.6g}"
                print(f"TIMESTEP {self.timeStep} / ENVS {self.n} / Q_LOSS {q1 + q2:.6g} / POLICY_LOSS {lpi:.6g} / ENTROPY {ent:.6g} / "
                      f"ALPHA {alpha:.6g} / GAME_TIMES {ep} / MEAN_SCORE {ssum / max(ep, 1):.3f} / MAX_SCORE {smax} / PIPES {pipes} / "
                      f"LOSS {tot:.6g}{clip}", flush=True)
