"""Vectorised front end of the HIP hot path: N envs / N-env replay / Q-network as torch-ROCm
tensors over the C ABI (include/fbdqn.h).  PyTorch is plumbing here (device memory, streams,
torch.distributed); every computation is a kernel of libfbdqn.so.

Reference counterparts:
    VecGameState  -> game/wrapped_flappy_bird.py GameState, N at a time, preprocess fused in
    VecReplay     -> BrainDQN.replayMemory (deque) / BrainPrioritizedReplyDQN.Memory
    QNet          -> BrainDQN._createQNetwork / _trainQNetwork and the variants' versions
"""
import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _dev_check(*tensors):
    for t in tensors:
        if t is not None and not (t.is_cuda and t.is_contiguous()):
            raise ValueError("tensors handed to the HIP path must be contiguous CUDA(ROCm) tensors")


def _check_states(name, x, rows=None):
    """`name` must be uint8[B,80,80,4] (rows: with that B)"""
    if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (80, 80, 4) or (rows is not None and x.shape[0] != rows):
        raise ValueError(f"{name} must be uint8[B,80,80,4]")


class VecGameState:
    """N independent Flappy Bird games on the GPU (game/wrapped_flappy_bird.py:58-183)."""

    def __init__(self, n_envs, seed=0, device="cuda"):
        L.require_gpu()
        self.n = int(n_envs)
        self.device = torch.device(device)
        self.h = C.c_void_p()
        blob = L.sprite_blob()
        L.check(L.lib().fb_env_create(self.n, seed, 0, blob, len(blob), C.byref(self.h)), "fb_env_create")
        dev = self.device
        self.frames = torch.empty((self.n, 80, 80), dtype=torch.uint8, device=dev)
        self.frame_bits = torch.empty((self.n, 100), dtype=torch.int64, device=dev)
        self.reward = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.terminal = torch.empty(self.n, dtype=torch.uint8, device=dev)
        self.score = torch.empty(self.n, dtype=torch.int32, device=dev)

    def __del__(self):
        try:                                     # at interpreter shutdown the module globals may already be gone
            if getattr(self, "h", None) and self.h.value:
                L.lib().fb_env_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def reset(self):
        L.check(L.lib().fb_env_reset(self.h, L.current_stream()), "fb_env_reset")

    def frame_step(self, actions, want_u8=True, frame_bits=None):
        """actions: uint8[N] (0 = nothing, 1 = flap).  Returns (frames u8[N,80,80] or None,
        reward f32[N], terminal u8[N], score i32[N]); the packed frame is in self.frame_bits
        (or in `frame_bits` when given, e.g. a replay-ring slot)."""
        _dev_check(actions, frame_bits)
        if actions.dtype != torch.uint8 or actions.numel() != self.n:
            raise ValueError("actions must be uint8[N]")
        fb = self.frame_bits if frame_bits is None else frame_bits
        L.check(L.lib().fb_env_step(self.h, L.ptr(actions), L.ptr(self.frames) if want_u8 else None, L.ptr(fb),
                                    L.ptr(self.reward), L.ptr(self.terminal), L.ptr(self.score),
                                    L.current_stream()), "fb_env_step")
        return (self.frames if want_u8 else None), self.reward, self.terminal, self.score

    def track_state(self):
        """Keep the agents' 4-frame stacks on the device in nibble form (fb_env_set_nib_buffer); returns the
        u8[N, FB_NIB_STRIDE] tensor (conv1's SAME padding included, include/fbdqn.h) that QNet.act_nib consumes.
        Call before observe()."""
        self.nib = torch.zeros((self.n, L.NIB_STRIDE), dtype=torch.uint8, device=self.device)
        L.check(L.lib().fb_env_set_nib_buffer(self.h, L.ptr(self.nib)), "fb_env_set_nib_buffer")
        return self.nib

    def track_stats(self):
        """Device-side episode counters (fb_env_set_stats_buffer): returns the int64[4] tensor
        [episodes ended, sum of their scores, max score, pipes passed]; read it whenever you log."""
        self.stats = torch.zeros(4, dtype=torch.int64, device=self.device)
        L.check(L.lib().fb_env_set_stats_buffer(self.h, L.ptr(self.stats)), "fb_env_set_stats_buffer")
        return self.stats

    def observe(self):
        L.check(L.lib().fb_env_observe(self.h, L.ptr(self.frames), L.ptr(self.frame_bits), L.current_stream()),
                "fb_env_observe")
        return self.frames

    def get_state(self):
        out = np.empty((self.n, 16), np.int32)
        L.check(L.lib().fb_env_get_state(self.h, L.ptr(out)), "fb_env_get_state")
        return out

    def set_state(self, state):
        state = np.ascontiguousarray(state, np.int32)
        assert state.shape == (self.n, 16)
        L.check(L.lib().fb_env_set_state(self.h, L.ptr(state)), "fb_env_set_state")

    def set_gap_tape(self, tape):
        if tape is None:
            L.check(L.lib().fb_env_set_gap_tape(self.h, None, 0), "fb_env_set_gap_tape")
            return
        tape = np.ascontiguousarray(tape, np.int8)
        assert tape.ndim == 2 and tape.shape[0] == self.n
        L.check(L.lib().fb_env_set_gap_tape(self.h, L.ptr(tape), tape.shape[1]), "fb_env_set_gap_tape")

    def render_full(self, env_id=0):
        out = torch.empty((288, 512, 3), dtype=torch.uint8, device=self.device)
        L.check(L.lib().fb_env_render_full(self.h, env_id, L.ptr(out), L.current_stream()), "fb_env_render_full")
        return out

    def error_count(self):
        v = C.c_int64()
        L.check(L.lib().fb_env_error_count(self.h, C.byref(v)), "fb_env_error_count")
        return v.value


class VecReplay:
    """Replay memory in HBM for N envs (BrainDQN.py:36,69-72,197-201;
    BrainPrioritizedReplyDQN.py:32-151).  Frames are stored once, 1 bit per pixel."""

    def __init__(self, capacity, n_envs=1, prioritized=False, device="cuda", n_step=1, gamma=None):
        """n_step > 1: n-step returns from the first push (fb_replay_create_nstep; 1 <= n_step <= 16, capacity >= n_step * n_envs,
        gamma required).  The only way to give a PRIORITIZED memory n-step returns: its tree stores each transition once it is
        complete, so n is fixed at creation (include/fbdqn.h).  A uniform memory created so equals one given set_n_step(n_step, gamma)."""
        self.h = C.c_void_p()
        n_step = int(n_step)
        if not 1 <= n_step <= L.NSTEP_MAX:
            raise ValueError(f"n_step must be in 1..{L.NSTEP_MAX}, got {n_step}")
        if n_step > 1 and gamma is None:
            raise ValueError(f"an n-step memory (n_step = {n_step}) needs the gamma of its returns")
        if int(capacity) < n_step * int(n_envs):
            raise ValueError(f"capacity {int(capacity)} < n_step x n_envs = {n_step * int(n_envs)}")
        L.require_gpu()
        self.capacity, self.n, self.prioritized = int(capacity), int(n_envs), bool(prioritized)
        self.device = torch.device(device)
        kind = L.REPLAY_PER if prioritized else L.REPLAY_UNIFORM
        if n_step == 1:
            L.check(L.lib().fb_replay_create(self.capacity, self.n, kind, C.byref(self.h)), "fb_replay_create")
        else:
            L.check(L.lib().fb_replay_create_nstep(self.capacity, self.n, kind, n_step, float(gamma), C.byref(self.h)),
                    "fb_replay_create_nstep")
        self._buf = {}

    def __del__(self):
        try:                                     # at interpreter shutdown the module globals may already be gone
            if getattr(self, "h", None) and self.h.value:
                L.lib().fb_replay_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def seed(self, seed, rng=None):
        """rng: 'cpython' (random.seed), 'numpy' (np.random.seed) or 'philox'."""
        kind = {"cpython": L.RNG_CPYTHON, "philox": L.RNG_PHILOX, "numpy": L.RNG_NUMPY}[
            rng or ("numpy" if self.prioritized else "cpython")]
        L.check(L.lib().fb_replay_seed(self.h, kind, seed), "fb_replay_seed")

    @staticmethod
    def _split(frames):
        """u8[N,80,80] -> (frames, None); int64[N,100] packed bits -> (None, bits)."""
        _dev_check(frames)
        if frames.dtype == torch.uint8:
            return frames, None
        if frames.dtype == torch.int64:
            return None, frames
        raise ValueError("frames must be uint8[N,80,80] or int64[N,100] (packed)")

    def reset(self, first_frames):
        f, b = self._split(first_frames)
        L.check(L.lib().fb_replay_reset(self.h, L.ptr(f), L.ptr(b), L.current_stream()), "fb_replay_reset")

    def push(self, next_frames, actions, rewards, terminals):
        f, b = self._split(next_frames)
        _dev_check(actions, rewards, terminals)
        L.check(L.lib().fb_replay_push(self.h, L.ptr(f), L.ptr(b), L.ptr(actions), L.ptr(rewards), L.ptr(terminals),
                                       L.current_stream()), "fb_replay_push")

    def push_sample(self, next_frames, actions, rewards, terminals, batch):
        """push(...) then sample(batch) of a uniform memory in one launch (fb_replay_push_sample) -> idx int64[B]."""
        if self.prioritized:
            raise ValueError("push_sample is for uniform memories (PER needs the importance weights: push + sample)")
        f, b = self._split(next_frames)
        _dev_check(actions, rewards, terminals)
        idx = self._get(f"idx{batch}", (batch,), torch.int64)
        L.check(L.lib().fb_replay_push_sample(self.h, L.ptr(f), L.ptr(b), L.ptr(actions), L.ptr(rewards), L.ptr(terminals),
                                              batch, L.ptr(idx), L.current_stream()), "fb_replay_push_sample")
        return idx

    def _get(self, name, shape, dtype):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._buf[name] = t
        return t

    def current_state(self):
        out = self._get("cur", (self.n, 80, 80, 4), torch.uint8)
        L.check(L.lib().fb_replay_current_state(self.h, L.ptr(out), L.current_stream()), "fb_replay_current_state")
        return out

    def sample(self, batch, uniforms=None, out=None):
        """-> idx int64[B] (deque positions, or SumTree indices for PER), isw float64[B] or None.
        `out`: an int64[B] device tensor to receive the indices (default: a buffer reused by every call)."""
        idx = self._get(f"idx{batch}", (batch,), torch.int64) if out is None else out
        _dev_check(idx)
        isw = self._get(f"isw{batch}", (batch,), torch.float64) if self.prioritized else None
        _dev_check(uniforms)
        L.check(L.lib().fb_replay_sample(self.h, batch, L.ptr(uniforms), L.ptr(idx), L.ptr(isw), L.current_stream()),
                "fb_replay_sample")
        return idx, isw

    def gather(self, idx):
        B = idx.numel()
        s = self._get(f"s{B}", (B, 80, 80, 4), torch.uint8)
        s2 = self._get(f"s2{B}", (B, 80, 80, 4), torch.uint8)
        a = self._get(f"a{B}", (B,), torch.uint8)
        r = self._get(f"r{B}", (B,), torch.float32)
        t = self._get(f"t{B}", (B,), torch.uint8)
        L.check(L.lib().fb_replay_gather(self.h, B, L.ptr(idx), L.ptr(s), L.ptr(s2), L.ptr(a), L.ptr(r), L.ptr(t),
                                         L.current_stream()), "fb_replay_gather")
        return s, a, r, s2, t

    def update_priorities(self, idx, abs_err=None, priorities=None):
        _dev_check(idx, abs_err, priorities)
        L.check(L.lib().fb_replay_update_priorities(self.h, idx.numel(), L.ptr(idx), L.ptr(abs_err), L.ptr(priorities),
                                                    L.current_stream()), "fb_replay_update_priorities")

    def set_per_mode(self, mode="exact"):
        """'exact' (reference-order running sums, bit-identical tree) or 'fast' (level-wise recomputation)."""
        L.check(L.lib().fb_replay_set_per_mode(self.h, {"exact": L.PER_EXACT, "fast": L.PER_FAST}[mode]),
                "fb_replay_set_per_mode")

    def set_priority_init(self, mode="max", gamma=None):
        """Which priority a new transition's leaf gets: 'max' (the tree's maximum, the reference's Memory.store) or 'td' (the |TD error|
        of the Q-values the actor computed, written one step later by prime(); fb_replay_set_priority_init: a prioritized memory in the
        fast mode only).  Switching clears the record of acting-time Q-values.  gamma: the one-step discount of those TD errors on an
        n = 1 memory (0.99 until set; an n-step memory uses its own, and a gamma given here must equal it)."""
        if mode not in PRIORITY_INITS:
            raise ValueError(f"priority_init must be one of {PRIORITY_INITS}, got {mode!r}")
        L.check(L.lib().fb_replay_set_priority_init(self.h, {"max": L.PER_INIT_MAX, "td": L.PER_INIT_TD}[mode]),
                "fb_replay_set_priority_init")
        if gamma is not None:
            L.check(L.lib().fb_replay_set_prime_gamma(self.h, float(gamma)), "fb_replay_set_prime_gamma")

    @property
    def priority_init(self):
        v = C.c_int()
        L.check(L.lib().fb_replay_get_priority_init(self.h, C.byref(v)), "fb_replay_get_priority_init")
        return PRIORITY_INITS[v.value]

    def prime(self, q, actions):
        """fb_replay_prime_priorities: q float32[N,A] = Q(s, .) of the current states and the actions uint8[N] taken there, once per
        step between the acting forward and the push.  The leaves the last push stored get the priority of their |TD error| (when the
        record holds their Q(s_t, a_t)), then q[e, actions[e]] is recorded."""
        _dev_check(q, actions)
        if q.dtype != torch.float32 or q.dim() != 2 or q.shape[0] != self.n or not q.is_contiguous():
            raise ValueError(f"q must be a contiguous float32[{self.n}, A] tensor")
        if actions.dtype != torch.uint8 or actions.numel() != self.n:
            raise ValueError(f"actions must be uint8[{self.n}]")
        L.check(L.lib().fb_replay_prime_priorities(self.h, L.ptr(q), L.ptr(actions), int(q.shape[1]), L.current_stream()),
                "fb_replay_prime_priorities")

    def prime_state(self):
        """(rows float32[n + 1, N], first, last): the record of acting-time Q-values and the push counts of the oldest and newest rows
        held (-1, -1: none).  With state_blob() it is what a resumed 'td' memory needs to continue bit for bit."""
        rows = np.empty((self.n_step[0] + 1, self.n), np.float32)
        first, last = C.c_int64(), C.c_int64()
        L.check(L.lib().fb_replay_get_prime_state(self.h, L.ptr(rows), rows.size, C.byref(first), C.byref(last)),
                "fb_replay_get_prime_state")
        return rows, first.value, last.value

    def load_prime_state(self, rows, first, last):
        rows = np.ascontiguousarray(rows, np.float32)
        L.check(L.lib().fb_replay_set_prime_state(self.h, L.ptr(rows), rows.size, int(first), int(last)), "fb_replay_set_prime_state")

    def set_n_step(self, n, gamma):
        """View the memory with n-step returns (fb_replay_set_n_step; uniform memories, 1 <= n <= 16, capacity >= n * n_envs): sample /
        gather / the ring-fed train calls then see (s_t, a_t, R, s_{t+n}, done) and bootstrap with gamma^n.  n = 1 restores the one-step
        memory.  Nothing stored changes; the training calls on it must be given this gamma.  A prioritized memory's n is fixed at
        creation (VecReplay(..., prioritized=True, n_step=K, gamma=g)): this raises for it."""
        L.check(L.lib().fb_replay_set_n_step(self.h, int(n), float(gamma)), "fb_replay_set_n_step")

    @property
    def n_step(self):
        """(n, gamma) of the memory's view; (1, 0.0) for the one-step memory."""
        n, g = C.c_int(), C.c_double()
        L.check(L.lib().fb_replay_get_n_step(self.h, C.byref(n), C.byref(g)), "fb_replay_get_n_step")
        return n.value, g.value

    @property
    def population(self):
        """transitions sample() draws from.  Uniform: deque positions, len(memory) less the (n - 1) * n_envs newest an n-step view
        cannot complete yet.  Prioritized: the tree's filled leaves, min(C, capacity) with C = max(0, pushes - n + 1) * n_envs
        completed transitions stored since the reset (len(memory) at n = 1)."""
        if self.prioritized:
            return self.per_state(want_tree=False)[2]
        return max(0, len(self) - (self.n_step[0] - 1) * self.n)

    def __len__(self):
        v = C.c_int64()
        L.check(L.lib().fb_replay_size(self.h, C.byref(v)), "fb_replay_size")
        return v.value

    def state_blob(self):
        """The whole memory as one numpy uint8 blob (fb_replay_save_state): frame ring, a / r / t rows, counters, sampler
        generator, SumTree heaps -- what a resumed run needs to continue the index stream bit for bit."""
        n = C.c_size_t()
        L.check(L.lib().fb_replay_state_bytes(self.h, C.byref(n)), "fb_replay_state_bytes")
        blob = np.empty(n.value, np.uint8)
        L.check(L.lib().fb_replay_save_state(self.h, L.ptr(blob), n.value), "fb_replay_save_state")
        return blob

    def load_state_blob(self, blob):
        blob = np.ascontiguousarray(blob, np.uint8)
        L.check(L.lib().fb_replay_load_state(self.h, L.ptr(blob), blob.size), "fb_replay_load_state")

    def per_state(self, want_tree=True):
        tree = np.empty(2 * self.capacity - 1, np.float64) if want_tree else None
        ptr_, size, beta = C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib().fb_replay_per_tree(self.h, L.ptr(tree), C.byref(ptr_), C.byref(size), C.byref(beta)),
                "fb_replay_per_tree")
        return tree, ptr_.value, size.value, beta.value


ALGOS = {"dqn": L.ALGO_DQN, "nature": L.ALGO_NATURE, "double": L.ALGO_DOUBLE, "per": L.ALGO_PER, "pg": L.ALGO_PG,
         "c51": L.ALGO_C51, "c51double": L.ALGO_C51_DOUBLE, "c51per": L.ALGO_C51_PER, "c51doubleper": L.ALGO_C51_DOUBLE_PER,
         "qr": L.ALGO_QR, "qrdouble": L.ALGO_QR_DOUBLE, "qrper": L.ALGO_QR_PER, "qrdoubleper": L.ALGO_QR_DOUBLE_PER,
         "mdqn": L.ALGO_MDQN, "mdqnper": L.ALGO_MDQN_PER, "doubleper": L.ALGO_DOUBLE_PER}
C51_ALGOS = ("c51", "c51double")                            # C51 on a uniform memory
C51_PER_ALGOS = ("c51per", "c51doubleper")                  # C51 on a prioritized memory (weighted loss, KL priorities)
QR_ALGOS = ("qr", "qrdouble")                               # QR-DQN on a uniform memory
QR_PER_ALGOS = ("qrper", "qrdoubleper")                     # QR-DQN on a prioritized memory (weighted loss, l_b priorities)
PER_ALGOS = ("per",) + C51_PER_ALGOS                        # the scalar and C51 algos that take a prioritized memory
PRIORITIZED_ALGOS = PER_ALGOS + QR_PER_ALGOS                # the algos of before Munchausen-DQN that take a prioritized memory
MDQN_ALGOS = ("mdqn",)                                      # Munchausen-DQN on a uniform memory (scalar heads; include/fbdqn.h)
MDQN_PER_ALGOS = ("mdqnper",)                               # Munchausen-DQN on a prioritized memory (FB_ALGO_PER's weights and |TD errors|)
DOUBLE_PER_ALGOS = ("doubleper",)                           # Double-DQN's target on a prioritized memory (scalar heads; include/fbdqn.h)
WEIGHTED_ALGOS = PRIORITIZED_ALGOS + MDQN_PER_ALGOS + DOUBLE_PER_ALGOS     # every algo that takes a prioritized memory and its importance weights
PRIORITY_INITS = ("max", "td")                             # a new leaf's priority: the tree's maximum, or the acting-time |TD error| (VecReplay.set_priority_init)
SCALAR_ALGOS = ("dqn", "nature", "double", "per", "mdqn", "mdqnper", "doubleper")      # the TD algos of the scalar heads: what the Huber loss applies to
MDQN_DEFAULTS = L.MDQN_DEFAULTS                             # (tau, alpha, l0) of a new scalar net
C51_DEFAULT_SUPPORT = (51, -10.0, 10.0)                  # n_atoms, v_min, v_max
C51_ARCHS = ("c51", "c51dueling")                         # distributional heads: C51, and the dueling C51 head (Rainbow's)
QR_ARCHS = ("qr", "qrdueling")                            # quantile heads: QR-DQN, and its dueling form
QR_DEFAULT_QUANTILES = (51, 1.0)                          # n_quantiles, kappa (include/fbdqn.h; the size of C51's default head)
ACTING_NOISE_MODES = ("shared", "env")                  # noisy nets: one noise sample for all envs when acting, or one per env
NOISY_DEFAULT_SIGMA0 = 0.5                                # noisy nets: sigma = sigma0 / sqrt(fan_in) at init (Fortunato et al.)
AC_ARCH = "ac"                                            # advantage actor-critic: V and the policy's logits on the shared trunk (include/fbdqn.h)
AC_DEFAULTS = L.AC_DEFAULTS                               # (value_coef, entropy_coef) of a new actor-critic net
AC_MAX_ROLLOUT = 128                                      # the longest rollout VecActorCritic takes
PPO_DEFAULTS = L.PPO_DEFAULTS                             # (clip_eps, value_clip) of a new actor-critic net
SAC_ARCH = "sac"                                          # discrete soft actor-critic: a policy head and two Q heads (include/fbdqn.h)
SAC_DEFAULTS = L.SAC_DEFAULTS                             # (alpha, target_entropy / ln A, alpha_lr) of a new SAC net
IQN_ARCH = "iqn"                                          # implicit quantile network: the plain layout and a cosine embedding (include/fbdqn.h)
IQN_DUELING_ARCH = "iqndueling"                           # its dueling form: value and advantage quantile streams, one effective column per action
IQN_ARCHS = (IQN_ARCH, IQN_DUELING_ARCH)                  # what every IQN call takes
IQN_DEFAULTS = L.IQN_DEFAULTS                             # (n_tau, n_tau_next, n_tau_act, kappa) of a new IQN net
IQN_NOISY_ARCHS = ("iqnnoisy", "iqnduelingnoisy")         # noisy IQN: fc1 and the head layers are factorised Gaussian layers (include/fbdqn.h)
IQN_ALL_ARCHS = IQN_ARCHS + IQN_NOISY_ARCHS               # what every IQN call takes
IQN_DUELING_ARCHS = (IQN_DUELING_ARCH, "iqnduelingnoisy")


def check_sigma0(sigma0):
    """the sigma0 check of fb_qnet_create_c51_noisy, on the host (-> float32-rounded float)"""
    s = float(np.float32(sigma0))
    if not (np.isfinite(s) and s >= 0.0):
        raise ValueError(f"sigma0 must be finite and >= 0, got {sigma0}")
    return s


def noise_size(fc_width, actions, n_atoms, arch):
    """the length of a noisy net's f(eps) vector (fb_qnet_get_noise): per layer fan_in + fan_out -- fc1, then the head's layer(s)"""
    fc = int(fc_width)
    if arch in IQN_NOISY_ARCHS:                  # (scalar layers: FC -> A, and the dueling net's V layer FC -> 1 in front of it; n_atoms is not read)
        return 1600 + fc + (fc + 1 if arch in IQN_DUELING_ARCHS else 0) + fc + int(actions)
    an = int(actions) * int(n_atoms)
    return 1600 + fc + (fc + int(n_atoms) if arch == "c51dueling" else 0) + fc + an


def check_support(n_atoms, v_min, v_max, actions=2):
    """the argument checks of fb_qnet_create_c51, on the host (-> (n_atoms, v_min, v_max) as int, float32-rounded floats)"""
    n_atoms = int(n_atoms)
    if not 2 <= n_atoms <= L.C51_MAX_ATOMS:
        raise ValueError(f"n_atoms must be in 2..{L.C51_MAX_ATOMS}, got {n_atoms}")
    if int(actions) * n_atoms > 128:
        raise ValueError(f"actions x n_atoms must be <= 128, got {int(actions)} x {n_atoms}")
    v_min, v_max = float(np.float32(v_min)), float(np.float32(v_max))
    if not (np.isfinite(v_min) and np.isfinite(v_max) and v_min < v_max):
        raise ValueError(f"the support needs finite v_min < v_max, got [{v_min}, {v_max}]")
    return n_atoms, v_min, v_max


def check_quantiles(n_quantiles, kappa, actions=2):
    """the argument checks of fb_qnet_create_qr, on the host (-> (n_quantiles, kappa) as int, float32-rounded float)"""
    n = int(n_quantiles)
    if not 2 <= n <= L.C51_MAX_ATOMS:
        raise ValueError(f"n_quantiles must be in 2..{L.C51_MAX_ATOMS}, got {n}")
    if int(actions) * n > 128:
        raise ValueError(f"actions x n_quantiles must be <= 128, got {int(actions)} x {n}")
    k = float(np.float32(kappa))
    if not (np.isfinite(k) and k > 0.0):
        raise ValueError(f"kappa must be finite and > 0, got {kappa}")
    return n, k


def check_munchausen(tau, alpha, clip):
    """the argument checks of fb_qnet_set_munchausen, on the host (-> (tau, alpha, l0) as float32-rounded floats)"""
    t, a, c = (float(np.float32(x)) for x in (tau, alpha, clip))
    if not (np.isfinite(t) and t > 0.0):
        raise ValueError(f"tau must be finite and > 0, got {tau}")
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], got {alpha}")
    if not (np.isfinite(c) and c <= 0.0):
        raise ValueError(f"clip (l0) must be finite and <= 0, got {clip}")
    return t, a, c


def check_ac(value_coef, entropy_coef):
    """the argument checks of fb_qnet_set_ac, on the host (-> (value_coef, entropy_coef) as float32-rounded floats)"""
    with np.errstate(over="ignore"):
        cv, ce = float(np.float32(value_coef)), float(np.float32(entropy_coef))
    if not (np.isfinite(cv) and cv >= 0.0):
        raise ValueError(f"value_coef must be finite and >= 0, got {value_coef}")
    if not (np.isfinite(ce) and ce >= 0.0):
        raise ValueError(f"entropy_coef must be finite and >= 0, got {entropy_coef}")
    return cv, ce


def check_ppo(clip_eps, value_clip):
    """the argument checks of fb_qnet_set_ppo, on the host (-> (clip_eps, value_clip) as float32-rounded floats; value_clip 0 = off)"""
    with np.errstate(over="ignore"):
        e, c = float(np.float32(clip_eps)), float(np.float32(value_clip))
    if not (np.isfinite(e) and e > 0.0):
        raise ValueError(f"clip_eps must be finite and > 0, got {clip_eps}")
    if not (np.isfinite(c) and c >= 0.0):
        raise ValueError(f"value_clip must be finite and >= 0, got {value_clip}")
    return e, c


def check_sac(alpha, target_entropy, alpha_lr, actions=2):
    """the argument checks of fb_qnet_set_sac, on the host (-> (alpha, target_entropy, alpha_lr) as float32-rounded floats);
    target_entropy None: the library's default, 0.98 ln(actions) in float32"""
    if not 2 <= int(actions) <= 8:
        raise ValueError(f"actions must be in 2..8 for a SAC net, got {actions}")
    if target_entropy is None:
        target_entropy = np.float32(SAC_DEFAULTS[1]) * np.log(np.float32(int(actions)))
    with np.errstate(over="ignore"):
        a, h, lr = (float(np.float32(x)) for x in (alpha, target_entropy, alpha_lr))
    if not (np.isfinite(a) and a > 0.0):
        raise ValueError(f"alpha must be finite and > 0, got {alpha}")
    if not np.isfinite(h):
        raise ValueError(f"target_entropy must be finite, got {target_entropy}")
    if not (np.isfinite(lr) and lr >= 0.0):
        raise ValueError(f"alpha_lr must be finite and >= 0 (0 = a fixed temperature), got {alpha_lr}")
    return a, h, lr


def check_iqn(n_tau, n_tau_next, n_tau_act, kappa, eta=1.0, actions=2):
    """the argument checks of fb_qnet_create_iqn and fb_qnet_set_iqn_risk, on the host
    (-> (n_tau, n_tau_next, n_tau_act, kappa, eta), the floats float32-rounded)"""
    if not 2 <= int(actions) <= 8:
        raise ValueError(f"actions must be in 2..8 for an IQN net, got {actions}")
    ns = []
    for name, v in (("n_tau", n_tau), ("n_tau_next", n_tau_next), ("n_tau_act", n_tau_act)):
        if int(v) != v or not 1 <= int(v) <= 64:
            raise ValueError(f"{name} must be an integer in 1..64, got {v}")
        ns.append(int(v))
    with np.errstate(over="ignore"):
        k, e = float(np.float32(kappa)), float(np.float32(eta))
    if not (np.isfinite(k) and k > 0.0):
        raise ValueError(f"kappa must be finite and > 0, got {kappa}")
    if not (np.isfinite(e) and 0.0 < e <= 1.0):
        raise ValueError(f"the risk setting eta (CVaR level) must be in (0, 1], got {eta}")
    return ns[0], ns[1], ns[2], k, e


def check_gae(gamma, gae_lambda):
    """the argument checks of fb_ac_gae, on the host (-> (gamma, lambda) as floats)"""
    g, l = float(gamma), float(gae_lambda)
    if not (np.isfinite(g) and 0.0 <= g <= 1.0):
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    if not (np.isfinite(l) and 0.0 <= l <= 1.0):
        raise ValueError(f"gae_lambda must be in [0, 1], got {gae_lambda}")
    return g, l


def check_rollout(rollout):
    """the rollout length of VecActorCritic / AcRolloutStep (-> int in 1..AC_MAX_ROLLOUT)"""
    t = int(rollout)
    if not 1 <= t <= AC_MAX_ROLLOUT:
        raise ValueError(f"rollout must be in 1..{AC_MAX_ROLLOUT}, got {rollout}")
    return t


def check_huber(delta):
    """the argument check of fb_qnet_set_huber, on the host (-> delta as a float32-rounded float; 0 = the squared loss)"""
    with np.errstate(over="ignore"):                   # (a value beyond float32's range is infinite as the float the library takes)
        d = float(np.float32(delta))
    if not (np.isfinite(d) and d >= 0.0):
        raise ValueError(f"huber (delta) must be finite and >= 0, got {delta}")
    return d


def check_max_grad_norm(g):
    """the argument check of fb_qnet_set_max_grad_norm, on the host (-> the limit as a float32-rounded float; 0 = no clipping)"""
    with np.errstate(over="ignore"):                   # (a value beyond float32's range is infinite as the float the library takes)
        v = float(np.float32(g))
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"max_grad_norm must be finite and >= 0, got {g}")
    return v


def check_polyak(rho, allow_off=False):
    """the argument check of fb_qnet_soft_sync_target, on the host (-> rho as a float32-rounded float in (0, 1]); allow_off: 0 passes
    as well (VecBrain's "no soft updates")"""
    v = float(np.float32(rho))
    if allow_off and v == 0.0:
        return 0.0
    if not (0.0 < v <= 1.0):                           # (NaN fails both comparisons)
        raise ValueError(f"polyak (rho) must be in (0, 1]{' or 0 = off' if allow_off else ''}, got {rho}")
    return v


def check_n_envs(n_envs):
    """the env count of a vectorised loop (-> int >= 1)"""
    n = int(n_envs)
    if n < 1:
        raise ValueError(f"n_envs must be >= 1, got {n_envs}")
    return n


def check_ring_batch(batch, n_envs):
    """the minibatch of a loop that trains from the ring every step (-> int in 1..256, at most n_envs)"""
    b = int(batch)
    if not 1 <= b <= 256:
        raise ValueError(f"batch must be in 1..256, got {batch}")
    if b > n_envs:
        raise ValueError(f"batch {b} > n_envs {n_envs}: every step draws a minibatch, the first from one push of n_envs transitions")
    return b


def check_observe(observe):
    """the steps a loop only stores before it trains (-> int >= 0)"""
    ob = int(observe)
    if ob < 0:
        raise ValueError(f"observe must be >= 0, got {observe}")
    return ob


def check_gamma(gamma):
    """a loop's discount (-> float in [0, 1])"""
    g = float(gamma)
    if not (np.isfinite(g) and 0.0 <= g <= 1.0):
        raise ValueError(f"gamma must be in [0, 1], got {gamma}")
    return g


def check_lr(lr):
    """Adam's learning rate (-> finite float > 0)"""
    l = float(lr)
    if not (np.isfinite(l) and l > 0.0):
        raise ValueError(f"lr must be finite and > 0, got {lr}")
    return l


def ring_capacity(capacity, n_envs):
    """the capacity of a ring-fed loop's memory (-> int; None: max(65536, 8 n_envs))"""
    return max(65536, 8 * n_envs) if capacity is None else int(capacity)


def bootstrap_gamma(gamma, n):
    """Gamma = g_n of the n-step return (g_0 = 1, g_{k+1} = g_k * gamma in float64): the discount an n-step target bootstraps with,
    and what QNet.train_step takes on a minibatch gathered from an n-step memory.  gamma itself at n = 1."""
    if int(n) == 1:
        return float(gamma)
    g = 1.0
    for _ in range(int(n)):
        g *= float(gamma)
    return g


class QNet:
    """The reference Q-network (BrainDQN.py:119-163) with forward, backward and TF-Adam as HIP
    kernels.  `arch='dueling'` builds the head of BrainDuelingDQN.py:78-86."""

    ARCHS = ("plain", "dueling") + C51_ARCHS + QR_ARCHS + (AC_ARCH, SAC_ARCH, IQN_ARCH, IQN_DUELING_ARCH) + IQN_NOISY_ARCHS

    def __init__(self, actions=2, fc_width=512, arch="plain", max_batch=32, device="cuda", n_atoms=C51_DEFAULT_SUPPORT[0],
                 v_min=C51_DEFAULT_SUPPORT[1], v_max=C51_DEFAULT_SUPPORT[2], noisy=False, sigma0=NOISY_DEFAULT_SIGMA0,
                 n_quantiles=QR_DEFAULT_QUANTILES[0], kappa=QR_DEFAULT_QUANTILES[1], n_tau=IQN_DEFAULTS[0], n_tau_next=IQN_DEFAULTS[1],
                 n_tau_act=IQN_DEFAULTS[2]):
        """arch='c51': the distributional head of include/fbdqn.h (n_atoms atoms on [v_min, v_max]; the support args are ignored otherwise);
        arch='c51dueling': the dueling C51 head (value and advantage distributions, include/fbdqn.h) on the same support.
        arch='qr' / 'qrdueling': the quantile head of QR-DQN (n_quantiles quantiles, quantile Huber loss with threshold kappa; include/fbdqn.h)
        and its dueling form; n_quantiles / kappa are ignored otherwise.
        noisy=True (C51 archs only): factorised Gaussian noisy fc1 and head layers, sigma initialised to sigma0 / sqrt(fan_in); the flat
        vector is [mu | sigma], and the net starts in mean mode (reset_noise, noise; include/fbdqn.h)
        arch='ac': an advantage actor-critic net -- the dueling net's parameters read raw, V = h . W_v + b_v and the policy's logits
        h . W_pi + b_pi (include/fbdqn.h); forward / act / act_nib / evaluation treat the logits as the Q values
        arch='sac': a discrete soft actor-critic net -- the policy's logits h . W_pi + b_pi and two Q heads (2 <= actions <= 8;
        include/fbdqn.h); forward / act / act_nib / evaluation treat the logits as the Q values
        arch='iqn': an implicit quantile network -- theta(s, a; tau) through a cosine embedding of tau; trains on n_tau / n_tau_next sampled
        tau with the quantile Huber loss (kappa), acts on the mean over a grid of n_tau_act tau (scaled by set_iqn_risk's eta), which
        forward / act / act_nib / evaluation return as the Q values (2 <= actions <= 8; include/fbdqn.h)
        arch='iqndueling': the dueling IQN net -- W_v b_v W_a b_a where W_q b_q stand, theta = V(tau) + Adv_a(tau) - mean_a' Adv_a'(tau) read as
        one effective column per action; every IQN call takes it (include/fbdqn.h)
        arch='iqnnoisy' / 'iqnduelingnoisy': the noisy forms of the two -- fc1 and the head layers (W_q b_q; dueling: the V and the advantage
        layer) are factorised Gaussian layers at sigma0, the tau embedding stays deterministic; .noisy is True, the noise calls and every IQN
        call take it (include/fbdqn.h).  noisy=True stays the C51 archs' keyword"""
        if arch not in self.ARCHS:
            raise ValueError(f"arch must be one of {self.ARCHS}, got {arch!r}")
        self.noisy = bool(noisy)
        self.sigma0 = None
        self.acting_noise = "shared"
        if arch in IQN_NOISY_ARCHS:                  # (noisy by name: noisy=True says nothing more)
            self.sigma0 = check_sigma0(sigma0)
        elif self.noisy:
            if arch not in C51_ARCHS:
                raise ValueError(f"noisy layers are offered on the C51 heads only ({C51_ARCHS}), not arch {arch!r}")
            self.sigma0 = check_sigma0(sigma0)
        if arch in C51_ARCHS:
            n_atoms, v_min, v_max = check_support(n_atoms, v_min, v_max, actions)
        if arch in QR_ARCHS:
            n_quantiles, kappa = check_quantiles(n_quantiles, kappa, actions)
        if arch in IQN_ALL_ARCHS:
            n_tau, n_tau_next, n_tau_act, kappa, _ = check_iqn(n_tau, n_tau_next, n_tau_act, kappa, 1.0, actions)
        L.require_gpu()
        self.A, self.FC, self.max_batch = int(actions), int(fc_width), int(max_batch)
        self.dueling = arch == "dueling"
        self.arch = arch
        self.device = torch.device(device)
        self.h = C.c_void_p()
        if arch in IQN_NOISY_ARCHS:
            self.noisy = True
            L.check(L.lib().fb_qnet_create_iqn_noisy(1 if arch in IQN_DUELING_ARCHS else 0, self.FC, self.A, n_tau, n_tau_next, n_tau_act, kappa,
                                                     self.sigma0, self.max_batch, C.byref(self.h)), "fb_qnet_create_iqn_noisy")
        elif self.noisy:
            L.check(L.lib().fb_qnet_create_c51_noisy(L.ARCH_C51 if arch == "c51" else L.ARCH_C51_DUELING, self.FC, self.A, n_atoms, v_min, v_max,
                                                     self.sigma0, self.max_batch, C.byref(self.h)), "fb_qnet_create_c51_noisy")
        elif arch == "c51":
            L.check(L.lib().fb_qnet_create_c51(self.FC, self.A, n_atoms, v_min, v_max, self.max_batch, C.byref(self.h)), "fb_qnet_create_c51")
        elif arch == "c51dueling":
            L.check(L.lib().fb_qnet_create_c51_dueling(self.FC, self.A, n_atoms, v_min, v_max, self.max_batch, C.byref(self.h)),
                    "fb_qnet_create_c51_dueling")
        elif arch == IQN_ARCH:
            L.check(L.lib().fb_qnet_create_iqn(self.FC, self.A, n_tau, n_tau_next, n_tau_act, kappa, self.max_batch, C.byref(self.h)),
                    "fb_qnet_create_iqn")
        elif arch == IQN_DUELING_ARCH:
            L.check(L.lib().fb_qnet_create_iqn_dueling(self.FC, self.A, n_tau, n_tau_next, n_tau_act, kappa, self.max_batch, C.byref(self.h)),
                    "fb_qnet_create_iqn_dueling")
        elif arch == SAC_ARCH:
            L.check(L.lib().fb_qnet_create_sac(self.FC, self.A, self.max_batch, C.byref(self.h)), "fb_qnet_create_sac")
        elif arch == AC_ARCH:
            L.check(L.lib().fb_qnet_create_ac(self.FC, self.A, self.max_batch, C.byref(self.h)), "fb_qnet_create_ac")
        elif arch in QR_ARCHS:
            L.check(L.lib().fb_qnet_create_qr(L.ARCH_QR if arch == "qr" else L.ARCH_QR_DUELING, self.FC, self.A, n_quantiles, kappa,
                                              self.max_batch, C.byref(self.h)), "fb_qnet_create_qr")
        else:
            L.check(L.lib().fb_qnet_create(L.ARCH_DUELING if self.dueling else L.ARCH_PLAIN, self.FC, self.A, self.max_batch,
                                           C.byref(self.h)), "fb_qnet_create")
        n = C.c_int64()
        L.check(L.lib().fb_qnet_num_params(self.h, C.byref(n)), "fb_qnet_num_params")
        self.n_params = n.value
        self._buf = {}

    def __del__(self):
        try:                                     # at interpreter shutdown the module globals may already be gone
            if getattr(self, "h", None) and self.h.value:
                L.lib().fb_qnet_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    def _get(self, name, shape, dtype):
        t = self._buf.get(name)
        if t is None or tuple(t.shape) != tuple(shape):
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._buf[name] = t
        return t

    # -- parameters -----------------------------------------------------------------
    def init_params(self, seed=0, which=L.NET_ONLINE):
        L.check(L.lib().fb_qnet_init_params(self.h, which, seed, L.current_stream()), "fb_qnet_init_params")

    def load_params(self, flat, which=L.NET_ONLINE):
        if not torch.is_tensor(flat):
            flat = torch.from_numpy(np.ascontiguousarray(flat, np.float32)).to(self.device)
        _dev_check(flat)
        if flat.dtype != torch.float32 or flat.numel() != self.n_params:
            raise ValueError(f"expected float32[{self.n_params}]")
        L.check(L.lib().fb_qnet_load_params(self.h, which, L.ptr(flat), L.current_stream()), "fb_qnet_load_params")
        torch.cuda.current_stream().synchronize()     # `flat` may be a temporary

    def store_params(self, which=L.NET_ONLINE):
        out = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_store_params(self.h, which, L.ptr(out), L.current_stream()), "fb_qnet_store_params")
        return out

    def set_hparams(self, lr=1e-6, beta1=0.9, beta2=0.999, eps=1e-8):
        L.check(L.lib().fb_qnet_set_hparams(self.h, lr, beta1, beta2, eps), "fb_qnet_set_hparams")

    def overflow_count(self, reset=False):
        """waves that split an ACTIVATION beyond the two-plane fp16 range (|x| >= 32768, include/fbdqn.h) since creation / the last
        reset: 0 = every forward / train step so far computed in range.  Synchronous (one device word)."""
        v = C.c_int64()
        L.check(L.lib().fb_qnet_overflow_count(self.h, int(bool(reset)), C.byref(v)), "fb_qnet_overflow_count")
        return v.value

    def split_stats(self):
        """(steps fb_vec_step issued with the train step on its own stream, how many of those started beside their env step)."""
        a, b = C.c_int64(), C.c_int64()
        L.check(L.lib().fb_qnet_split_stats(self.h, C.byref(a), C.byref(b)), "fb_qnet_split_stats")
        return a.value, b.value

    def check_range(self):
        """raise FbError if a launch of this net met an activation beyond the fp32-equivalent path's range (its results are then
        inf / NaN / wrong where TensorFlow's fp32 would have carried on)"""
        n = self.overflow_count()
        if n:
            raise L.FbError(f"{n} wave(s) of the Q-network's fp32-equivalent (two-plane fp16) kernels met an activation of magnitude >= 32768: "
                            "those Q-values / gradients are not to be trusted.  Use set_inference_dtype('bf16') / set_train_dtype('bf16') "
                            "(fp32's exponent range) for this net, or rescale its weights (include/fbdqn.h, fb_qnet_overflow_count).")

    def set_inference_dtype(self, dtype="f32"):
        """'f32' (default) or 'bf16': arithmetic of forward / act / act_nib on >= 256 states (BASELINE config 3)."""
        L.check(L.lib().fb_qnet_set_inference_dtype(self.h, {"f32": L.DTYPE_F32, "bf16": L.DTYPE_BF16}[dtype]),
                "fb_qnet_set_inference_dtype")

    def set_train_dtype(self, dtype="f32"):
        """'f32' (default) or 'bf16': arithmetic of train_step (bf16 operands, fp32 accumulation, fp32 master weights + Adam)."""
        L.check(L.lib().fb_qnet_set_train_dtype(self.h, {"f32": L.DTYPE_F32, "bf16": L.DTYPE_BF16}[dtype]), "fb_qnet_set_train_dtype")

    def adam_state(self):
        m = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        v = torch.empty_like(m)
        pows = np.empty(2, np.float32)
        L.check(L.lib().fb_qnet_get_adam_state(self.h, L.ptr(m), L.ptr(v), L.ptr(pows)), "fb_qnet_get_adam_state")
        return m, v, pows

    def set_adam_state(self, m, v, pows):
        pows = np.ascontiguousarray(pows, np.float32)
        _dev_check(m, v)
        L.check(L.lib().fb_qnet_set_adam_state(self.h, L.ptr(m), L.ptr(v), L.ptr(pows)), "fb_qnet_set_adam_state")

    def sync_target(self):
        L.check(L.lib().fb_qnet_sync_target(self.h, L.current_stream()), "fb_qnet_sync_target")

    def soft_sync_target(self, rho):
        """target <- target + rho (online - target) over the flat vector (fb_qnet_soft_sync_target; [mu | sigma] of a noisy net), with
        everything derived from the target's parameters rebuilt behind it; rho in (0, 1], rho = 1 is sync_target itself"""
        L.check(L.lib().fb_qnet_soft_sync_target(self.h, check_polyak(rho), L.current_stream()), "fb_qnet_soft_sync_target")

    # -- gradient clipping by global norm --------------------------------------------
    def set_max_grad_norm(self, g):
        """the limit G of the flat gradient's norm (fb_qnet_set_max_grad_norm): 0 = off; G > 0: train_step / train_from_replay / VecStep
        without flat_grad scale the gradient by G / max(norm, G) before Adam, and a data-parallel step clips behind its reduction.
        An exported gradient (flat_grad) stays unclipped: clip_grad does it"""
        L.check(L.lib().fb_qnet_set_max_grad_norm(self.h, check_max_grad_norm(g)), "fb_qnet_set_max_grad_norm")

    @property
    def max_grad_norm(self):
        g = C.c_float()
        L.check(L.lib().fb_qnet_get_max_grad_norm(self.h, C.byref(g)), "fb_qnet_get_max_grad_norm")
        return g.value

    def clip_grad(self, flat_grad):
        """clip float32[n_params] in place to the net's limit (fb_qnet_clip_grad); with the limit 0 it only records the norm"""
        _dev_check(flat_grad)
        if flat_grad.dtype != torch.float32 or flat_grad.numel() != self.n_params:
            raise ValueError(f"expected float32[{self.n_params}]")
        L.check(L.lib().fb_qnet_clip_grad(self.h, L.ptr(flat_grad), L.current_stream()), "fb_qnet_clip_grad")

    def grad_norm(self):
        """(norm, scale) of the net's last clip (fb_qnet_grad_norm); synchronous: read it when you log, not per step"""
        n, c = C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_grad_norm(self.h, C.byref(n), C.byref(c)), "fb_qnet_grad_norm")
        return n.value, c.value

    # -- Munchausen-DQN (scalar heads) -----------------------------------------------
    def set_munchausen(self, tau=MDQN_DEFAULTS[0], alpha=MDQN_DEFAULTS[1], clip=MDQN_DEFAULTS[2]):
        """(tau, alpha, l0) of algos 'mdqn' / 'mdqnper' (fb_qnet_set_munchausen): the softmax temperature, the bonus's scale and its
        lower clip; refused on a C51 / QR net and for values outside their ranges, before anything changes"""
        L.check(L.lib().fb_qnet_set_munchausen(self.h, float(tau), float(alpha), float(clip)), "fb_qnet_set_munchausen")

    def munchausen(self):
        """the net's current (tau, alpha, l0) (fb_qnet_get_munchausen)"""
        t, a, c = C.c_float(), C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_munchausen(self.h, C.byref(t), C.byref(a), C.byref(c)), "fb_qnet_get_munchausen")
        return t.value, a.value, c.value

    # -- Huber loss (scalar heads) ------------------------------------------------------
    def set_huber(self, delta):
        """the Huber (clipped-error) loss's delta of every scalar TD algo (fb_qnet_set_huber): d^2 inside |d| <= delta, delta (2 |d| -
        delta) outside, the gradient through clamp(d, -delta, delta); 0 = off, the squared loss.  Refused on a C51 / QR / noisy net
        and for a NaN, infinite or negative delta, before anything changes"""
        L.check(L.lib().fb_qnet_set_huber(self.h, float(delta)), "fb_qnet_set_huber")

    def huber(self):
        """the net's current delta (fb_qnet_get_huber); 0 = the squared loss"""
        d = C.c_float()
        L.check(L.lib().fb_qnet_get_huber(self.h, C.byref(d)), "fb_qnet_get_huber")
        return d.value

    # -- advantage actor-critic (arch='ac') -------------------------------------------
    def _need_ac(self, what):
        if self.arch != AC_ARCH:
            raise ValueError(f"{what} needs an actor-critic net (QNet(..., arch='ac'))")

    def set_ac(self, value_coef=AC_DEFAULTS[0], entropy_coef=AC_DEFAULTS[1]):
        """the A2C loss's coefficients (fb_qnet_set_ac): loss = mean(L_pi + value_coef L_v - entropy_coef H); both finite and >= 0"""
        self._need_ac("set_ac")
        cv, ce = check_ac(value_coef, entropy_coef)
        L.check(L.lib().fb_qnet_set_ac(self.h, cv, ce), "fb_qnet_set_ac")

    def ac(self):
        """the net's current (value_coef, entropy_coef) (fb_qnet_get_ac)"""
        self._need_ac("ac")
        cv, ce = C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_ac(self.h, C.byref(cv), C.byref(ce)), "fb_qnet_get_ac")
        return cv.value, ce.value

    def forward_ac(self, states):
        """u8 states -> (logits f32[B, A], value f32[B]) of the online net (fb_qnet_forward_ac)"""
        self._need_ac("forward_ac")
        _dev_check(states)
        _check_states("states", states)
        B = states.shape[0]
        z = torch.empty((B, self.A), dtype=torch.float32, device=self.device)
        v = torch.empty(B, dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_forward_ac(self.h, L.ptr(states), B, L.ptr(z), L.ptr(v), L.current_stream()), "fb_qnet_forward_ac")
        return z, v

    def act_policy_nib(self, nib_states, seed=0, step=0, greedy=False, want_logits=False, value=None, logp=None, actions=None, value_only=False):
        """sample an action per env from the policy (fb_qnet_act_policy_nib; the draw is keyed (seed, step, row), greedy: the first argmax)
        -> (actions u8[n], value f32[n], logp f32[n][, logits f32[n, A]]).  value / logp / actions: tensors to write into (a rollout
        buffer's row).  value_only: no action and no draw -> value alone (the bootstrap V(s_T))"""
        if self.arch != SAC_ARCH:
            self._need_ac("act_policy_nib")
        _dev_check(nib_states, value, logp, actions)
        if nib_states.dtype != torch.uint8 or nib_states.dim() != 2 or nib_states.shape[1] != L.NIB_STRIDE:
            raise ValueError(f"nib_states must be uint8[n,{L.NIB_STRIDE}] (VecGameState.track_state())")
        n = nib_states.shape[0]
        for name, t, dt in (("value", value, torch.float32), ("logp", logp, torch.float32), ("actions", actions, torch.uint8)):
            if t is not None and (t.dtype != dt or t.numel() != n):
                raise ValueError(f"{name} must be {dt}[{n}]")
        value = torch.empty(n, dtype=torch.float32, device=self.device) if value is None else value
        if value_only:
            L.check(L.lib().fb_qnet_act_policy_nib(self.h, L.ptr(nib_states), n, int(seed), int(step), 0, None, L.ptr(value), None, None,
                                                   L.current_stream()), "fb_qnet_act_policy_nib")
            return value
        actions = torch.empty(n, dtype=torch.uint8, device=self.device) if actions is None else actions
        logp = torch.empty(n, dtype=torch.float32, device=self.device) if logp is None else logp
        z = torch.empty((n, self.A), dtype=torch.float32, device=self.device) if want_logits else None
        L.check(L.lib().fb_qnet_act_policy_nib(self.h, L.ptr(nib_states), n, int(seed), int(step), int(bool(greedy)), L.ptr(actions), L.ptr(value),
                                               L.ptr(logp), L.ptr(z), L.current_stream()), "fb_qnet_act_policy_nib")
        return (actions, value, logp, z) if want_logits else (actions, value, logp)

    def ac_train_step(self, s, a, adv, ret, n_total=None, flat_grad=None):
        """one A2C step on <= 256 gathered states (fb_qnet_ac_train_step): n_total = the whole update's sample count (default: this
        chunk's).  flat_grad=None applies Adam; a float32[n_params] tensor receives the chunk's gradient instead.
        -> loss f32[4] (device): the chunk's share of (total, policy, value, entropy)"""
        self._need_ac("ac_train_step")
        _dev_check(s, a, adv, ret, flat_grad)
        _check_states("s", s)
        B = s.shape[0]
        check_ac_batch(B, a, adv, ret, n_total, flat_grad, self.n_params)
        loss = torch.zeros(4, dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_ac_train_step(self.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(ret), int(n_total or B), L.ptr(loss),
                                              L.ptr(flat_grad), L.current_stream()), "fb_qnet_ac_train_step")
        return loss

    def set_ppo(self, clip_eps=PPO_DEFAULTS[0], value_clip=PPO_DEFAULTS[1]):
        """PPO's clip ranges (fb_qnet_set_ppo): the ratio is clipped to [1 - clip_eps, 1 + clip_eps]; value_clip > 0 clips the value
        around the rollout's, 0 = off.  The loss's coefficients are set_ac's"""
        self._need_ac("set_ppo")
        e, c = check_ppo(clip_eps, value_clip)
        L.check(L.lib().fb_qnet_set_ppo(self.h, e, c), "fb_qnet_set_ppo")

    def ppo(self):
        """the net's current (clip_eps, value_clip) (fb_qnet_get_ppo)"""
        self._need_ac("ppo")
        e, c = C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_ppo(self.h, C.byref(e), C.byref(c)), "fb_qnet_get_ppo")
        return e.value, c.value

    def ppo_train_step(self, s, a, adv, ret, logp_old, value_old, n_total=None, flat_grad=None):
        """one PPO step on <= 256 gathered states (fb_qnet_ppo_train_step): logp_old / value_old are the rollout's log-probabilities
        and values, n_total = the minibatch's sample count (default: this chunk's).  flat_grad as for ac_train_step.
        -> loss f32[6] (device): the chunk's share of (total, policy, value, entropy, clip fraction, approximate KL)"""
        self._need_ac("ppo_train_step")
        _dev_check(s, a, adv, ret, logp_old, value_old, flat_grad)
        _check_states("s", s)
        B = s.shape[0]
        check_chunk(B, a, n_total, flat_grad, self.n_params)
        check_ppo_batch(B, None, adv, ret, logp_old, value_old)
        loss = torch.zeros(6, dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_ppo_train_step(self.h, B, L.ptr(s), L.ptr(a), L.ptr(adv), L.ptr(ret), L.ptr(logp_old), L.ptr(value_old),
                                               int(n_total or B), L.ptr(loss), L.ptr(flat_grad), L.current_stream()), "fb_qnet_ppo_train_step")
        return loss

    # -- discrete soft actor-critic (arch='sac') ---------------------------------------
    def _need_sac(self, what):
        if self.arch != SAC_ARCH:
            raise ValueError(f"{what} needs a SAC net (QNet(..., arch='sac'))")

    def set_sac(self, alpha=SAC_DEFAULTS[0], target_entropy=None, alpha_lr=SAC_DEFAULTS[2]):
        """the temperature alpha, the target entropy (None: 0.98 ln A) and the temperature's learning rate, 0 = fixed (fb_qnet_set_sac);
        writes log alpha and clears the temperature's Adam state"""
        self._need_sac("set_sac")
        a, h, lr = check_sac(alpha, target_entropy, alpha_lr, self.A)
        L.check(L.lib().fb_qnet_set_sac(self.h, a, h, lr), "fb_qnet_set_sac")

    def sac(self):
        """the net's current (alpha, target_entropy, alpha_lr) (fb_qnet_get_sac); synchronous"""
        self._need_sac("sac")
        a, h, lr = C.c_float(), C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_sac(self.h, C.byref(a), C.byref(h), C.byref(lr)), "fb_qnet_get_sac")
        return a.value, h.value, lr.value

    def sac_state(self):
        """(log alpha, m, v, beta1 power, beta2 power) as float32[5] on the host (fb_qnet_get_sac_state); synchronous"""
        self._need_sac("sac_state")
        w = np.empty(5, np.float32)
        L.check(L.lib().fb_qnet_get_sac_state(self.h, L.ptr(w)), "fb_qnet_get_sac_state")
        return w

    def set_sac_state(self, state):
        self._need_sac("set_sac_state")
        w = np.ascontiguousarray(state, np.float32)
        if w.shape != (5,):
            raise ValueError("the temperature state is float32[5]: (log alpha, m, v, beta1 power, beta2 power)")
        L.check(L.lib().fb_qnet_set_sac_state(self.h, L.ptr(w)), "fb_qnet_set_sac_state")

    def forward_sac(self, states, which=L.NET_ONLINE):
        """u8 states -> (logits, q1, q2), each f32[B, A], of the online or the target net (fb_qnet_forward_sac)"""
        self._need_sac("forward_sac")
        _dev_check(states)
        _check_states("states", states)
        B = states.shape[0]
        z, q1, q2 = (torch.empty((B, self.A), dtype=torch.float32, device=self.device) for _ in range(3))
        L.check(L.lib().fb_qnet_forward_sac(self.h, int(which), L.ptr(states), B, L.ptr(z), L.ptr(q1), L.ptr(q2), L.current_stream()),
                "fb_qnet_forward_sac")
        return z, q1, q2

    def _sac_train_step(self, what, s, a, r, s2, t, isw, gamma, flat_grad, want_target):
        """sac_train_step, and with `what` == 'sac_per_train_step' its prioritized form (isw in, abs_err out)
        -> (loss f32[6], q_target f32[B] or None, abs_err f32[B] or None)"""
        weighted = what == "sac_per_train_step"
        self._need_sac(what)
        _dev_check(s, a, r, s2, t, isw, flat_grad)
        for name, x in (("s", s), ("s2", s2)):
            _check_states(name, x, s.shape[0])
        B = s.shape[0]
        check_sac_batch(B, a, r, t, flat_grad, self.n_params)
        if weighted:
            check_isw(B, isw)
        loss = torch.zeros(6, dtype=torch.float32, device=self.device)
        ae = torch.empty(B, dtype=torch.float32, device=self.device) if weighted else None
        y = torch.empty(B, dtype=torch.float32, device=self.device) if want_target else None
        batch = (self.h, B, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t))
        out = (L.ptr(y), L.ptr(flat_grad), L.current_stream())
        if weighted:
            L.check(L.lib().fb_qnet_sac_per_train_step(*batch, L.ptr(isw), float(gamma), L.ptr(loss), L.ptr(ae), *out), "fb_qnet_sac_per_train_step")
        else:
            L.check(L.lib().fb_qnet_sac_train_step(*batch, float(gamma), L.ptr(loss), *out), "fb_qnet_sac_train_step")
        return loss, y, ae

    def sac_train_step(self, s, a, r, s2, t, gamma=0.99, flat_grad=None, want_target=True):
        """one SAC step on <= 256 gathered transitions (fb_qnet_sac_train_step).  flat_grad=None applies Adam (and, with alpha_lr > 0,
        the temperature's step); a float32[n_params] tensor receives the gradient instead.
        -> (loss f32[6]: total, mean d1^2, mean d2^2, mean L_pi, mean entropy, the alpha used; q_target f32[B] or None)"""
        return QNet._sac_train_step(self, "sac_train_step", s, a, r, s2, t, None, gamma, flat_grad, want_target)[:2]

    def sac_per_train_step(self, s, a, r, s2, t, isw, gamma=0.99, flat_grad=None, want_target=True):
        """sac_train_step with importance weights isw f32[B] (fb_qnet_sac_per_train_step): both critic terms and their gradients are
        weighted by w_b, the actor term, the entropy and the temperature's step are not; abs_err[b] = 0.5 (|d1| + |d2|), without the
        weight, is the priority.  isw = 1 gives sac_train_step's bits.  On n-step transitions gamma is the bootstrap's gamma^n.
        -> (loss f32[6], q_target f32[B] or None, abs_err f32[B])"""
        return QNet._sac_train_step(self, "sac_per_train_step", s, a, r, s2, t, isw, gamma, flat_grad, want_target)

    # -- implicit quantile networks (arch='iqn') -----------------------------------------
    def _need_iqn(self, what):
        if self.arch not in IQN_ALL_ARCHS:
            raise ValueError(f"{what} needs an IQN net (QNet(..., arch='iqn'))")

    def set_iqn_risk(self, eta=1.0):
        """act under CVaR_eta: the acting grid becomes eta (2 i + 1) / (2 K); 1 = risk neutral (fb_qnet_set_iqn_risk); synchronous"""
        self._need_iqn("set_iqn_risk")
        e = check_iqn(1, 1, 1, 1.0, eta, self.A)[4]
        L.check(L.lib().fb_qnet_set_iqn_risk(self.h, e), "fb_qnet_set_iqn_risk")

    def set_iqn_munchausen(self, on, temp=MDQN_DEFAULTS[0], alpha=MDQN_DEFAULTS[1], clip=MDQN_DEFAULTS[2]):
        """Munchausen IQN on / off and its (temp, alpha, l0) (fb_qnet_set_iqn_munchausen): the IQN train steps issued after it form the soft
        target with the log-policy bonus; on refuses double_q.  temp is Munchausen-DQN's tau (tau is the quantile fraction here)"""
        self._need_iqn("set_iqn_munchausen")
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"on must be True or False, got {on!r}")
        L.check(L.lib().fb_qnet_set_iqn_munchausen(self.h, int(on), float(temp), float(alpha), float(clip)), "fb_qnet_set_iqn_munchausen")

    def iqn_munchausen(self):
        """the net's (on, temp, alpha, l0) (fb_qnet_get_iqn_munchausen)"""
        self._need_iqn("iqn_munchausen")
        o, t, a, c = C.c_int(), C.c_float(), C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_iqn_munchausen(self.h, C.byref(o), C.byref(t), C.byref(a), C.byref(c)), "fb_qnet_get_iqn_munchausen")
        return bool(o.value), t.value, a.value, c.value

    def iqn(self):
        """the net's (n_tau, n_tau_next, n_tau_act, kappa, eta) (fb_qnet_get_iqn)"""
        self._need_iqn("iqn")
        n, m, k, ka, e = C.c_int(), C.c_int(), C.c_int(), C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_iqn(self.h, C.byref(n), C.byref(m), C.byref(k), C.byref(ka), C.byref(e)), "fb_qnet_get_iqn")
        return n.value, m.value, k.value, ka.value, e.value

    def forward_iqn(self, states, tau, which=L.NET_ONLINE):
        """u8 states [B,80,80,4], tau f32[B, M] (1 <= M <= 64) -> theta f32[B, M, A] of the online or the target net (fb_qnet_forward_iqn)"""
        self._need_iqn("forward_iqn")
        _dev_check(states, tau)
        _check_states("states", states)
        B = states.shape[0]
        if tau.dtype != torch.float32 or tau.dim() != 2 or tau.shape[0] != B or not 1 <= tau.shape[1] <= 64 or not tau.is_contiguous():
            raise ValueError("tau must be a contiguous float32[B, M] with 1 <= M <= 64")
        M = tau.shape[1]
        theta = torch.empty((B, M, self.A), dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_forward_iqn(self.h, int(which), L.ptr(states), B, L.ptr(tau), M, L.ptr(theta), L.current_stream()),
                "fb_qnet_forward_iqn")
        return theta

    def _iqn_train_step(self, what, s, a, r, s2, t, isw, gamma, double_q, tau, tau_next, seed, step, flat_grad, want_target):
        """iqn_train_step, and with `what` == 'iqn_per_train_step' its prioritized form (isw in, abs_err out)
        -> (loss f32[1], abs_err f32[B] or None, q_target f32[B, n_tau_next] or None)"""
        weighted = what == "iqn_per_train_step"
        self._need_iqn(what)
        _dev_check(s, a, r, s2, t, isw, flat_grad, tau, tau_next)
        for name, x in (("s", s), ("s2", s2)):
            _check_states(name, x, s.shape[0])
        B = s.shape[0]
        N, Np = self.iqn()[:2]
        check_iqn_batch(B, a, r, t, tau, tau_next, N, Np, flat_grad, self.n_params)
        if weighted:
            check_isw(B, isw)
        loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        ae = torch.empty(B, dtype=torch.float32, device=self.device) if weighted else None
        y = torch.empty((B, Np), dtype=torch.float32, device=self.device) if want_target else None
        batch = (self.h, int(bool(double_q)), B, L.ptr(s), L.ptr(a), L.ptr(r), L.ptr(s2), L.ptr(t))
        draws = (L.ptr(tau), L.ptr(tau_next), int(seed), int(step), float(gamma), L.ptr(loss))
        out = (L.ptr(y), L.ptr(flat_grad), L.current_stream())
        if weighted:
            L.check(L.lib().fb_qnet_iqn_per_train_step(*batch, L.ptr(isw), *draws, L.ptr(ae), *out), "fb_qnet_iqn_per_train_step")
        else:
            L.check(L.lib().fb_qnet_iqn_train_step(*batch, *draws, *out), "fb_qnet_iqn_train_step")
        return loss, ae, y

    def iqn_train_step(self, s, a, r, s2, t, gamma=0.99, double_q=False, tau=None, tau_next=None, seed=0, step=0, flat_grad=None,
                       want_target=True):
        """one IQN step on <= 256 gathered transitions (fb_qnet_iqn_train_step).  tau f32[B, n_tau] / tau_next f32[B, n_tau_next], or None:
        the draws of (seed, step) (iqn_draw_taus).  flat_grad=None applies Adam; a float32[n_params] tensor receives the gradient instead.
        -> (loss f32[1], q_target f32[B, n_tau_next] or None)"""
        loss, _, y = self._iqn_train_step("iqn_train_step", s, a, r, s2, t, None, gamma, double_q, tau, tau_next, seed, step, flat_grad, want_target)
        return loss, y

    def iqn_per_train_step(self, s, a, r, s2, t, isw, gamma=0.99, double_q=False, tau=None, tau_next=None, seed=0, step=0, flat_grad=None,
                           want_target=True):
        """iqn_train_step with importance weights isw f32[B] (fb_qnet_iqn_per_train_step): the loss is mean_b w_b l_b, the gradient that of
        l_b / B times w_b; abs_err[b] = l_b, without the weight, is the priority.  isw = 1 gives iqn_train_step's bits.
        -> (loss f32[1], abs_err f32[B], q_target f32[B, n_tau_next] or None)"""
        return self._iqn_train_step("iqn_per_train_step", s, a, r, s2, t, isw, gamma, double_q, tau, tau_next, seed, step, flat_grad, want_target)

    # -- noise (noisy nets) ---------------------------------------------------------
    def _need_noisy(self, what):
        if not self.noisy:
            raise ValueError(f"{what} needs a noisy net (QNet(..., noisy=True))")

    def reset_noise(self, which=L.NET_ONLINE, seed=0, step=0, mean=False):
        """draw net `which`'s noise at (seed, step) (fb_qnet_reset_noise), or mean=True: zero noise, the effective weights are mu"""
        self._need_noisy("reset_noise")
        L.check(L.lib().fb_qnet_reset_noise(self.h, int(which), int(seed), int(step), L.NOISE_MEAN if mean else L.NOISE_SAMPLE,
                                            L.current_stream()), "fb_qnet_reset_noise")

    def mean_noise(self, which=L.NET_ONLINE):
        """mean mode for net `which`: zero noise"""
        self.reset_noise(which, mean=True)

    def set_acting_noise(self, mode="shared"):
        """the noise fb_vec_step acts with (fb_qnet_set_acting_noise): 'shared' -- the online net's current sample, one for all envs
        (the default) -- or 'env': independent noise per env (act_nib_env_noise); training is the same in both"""
        self._need_noisy("set_acting_noise")
        if mode not in ACTING_NOISE_MODES:
            raise ValueError(f"acting noise must be one of {ACTING_NOISE_MODES}, got {mode!r}")
        L.check(L.lib().fb_qnet_set_acting_noise(self.h, L.ACT_NOISE_PER_ENV if mode == "env" else L.ACT_NOISE_SHARED),
                "fb_qnet_set_acting_noise")
        self.acting_noise = mode

    @property
    def noise_size(self):
        if not self.noisy:
            return 0
        return noise_size(self.FC, self.A, 0 if self.arch in IQN_NOISY_ARCHS else self.support[0], self.arch)

    def noise(self, which=L.NET_ONLINE):
        """net `which`'s current f(eps) vector, float32[noise_size] on the device (per layer: f(eps_in), then f(eps_out))"""
        self._need_noisy("noise")
        out = torch.empty(self.noise_size, dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_get_noise(self.h, int(which), L.ptr(out)), "fb_qnet_get_noise")
        return out

    @property
    def support(self):
        """(n_atoms, v_min, v_max) of a C51 net (fb_qnet_get_support), None for a scalar head"""
        n, lo, hi = C.c_int(), C.c_float(), C.c_float()
        L.check(L.lib().fb_qnet_get_support(self.h, C.byref(n), C.byref(lo), C.byref(hi)), "fb_qnet_get_support")
        return (n.value, lo.value, hi.value) if n.value else None

    def quantiles(self):
        """(n_quantiles, kappa) of a QR net (fb_qnet_get_quantiles), None for any other head"""
        n, k = C.c_int(), C.c_float()
        L.check(L.lib().fb_qnet_get_quantiles(self.h, C.byref(n), C.byref(k)), "fb_qnet_get_quantiles")
        return (n.value, k.value) if n.value else None

    def atoms(self):
        """the support values z_i = v_min + i * dz as float32 (the device's arithmetic), or None"""
        sup = self.support
        if sup is None:
            return None
        n, lo, hi = sup
        dz = (np.float32(hi) - np.float32(lo)) / np.float32(n - 1)
        return np.float32(lo) + np.arange(n, dtype=np.float32) * np.float32(dz)

    # -- compute --------------------------------------------------------------------
    def forward_dist(self, states, which=L.NET_ONLINE):
        """C51 nets: the return distributions p f32[B, A, n_atoms] of u8 states (fb_qnet_forward_dist)"""
        _dev_check(states)
        sup = self.support
        if sup is None:
            raise ValueError("forward_dist needs a C51 net (arch='c51' or 'c51dueling')")
        B = states.shape[0]
        _check_states("states", states)
        p = torch.empty((B, self.A, sup[0]), dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_forward_dist(self.h, which, L.ptr(states), B, L.ptr(p), L.current_stream()), "fb_qnet_forward_dist")
        return p

    def forward_quantiles(self, states, which=L.NET_ONLINE):
        """QR nets: the quantiles theta f32[B, A, n_quantiles] of u8 states (fb_qnet_forward_quantiles)"""
        _dev_check(states)
        qs = self.quantiles()
        if qs is None:
            raise ValueError("forward_quantiles needs a QR net (arch='qr' or 'qrdueling')")
        B = states.shape[0]
        _check_states("states", states)
        th = torch.empty((B, self.A, qs[0]), dtype=torch.float32, device=self.device)
        L.check(L.lib().fb_qnet_forward_quantiles(self.h, which, L.ptr(states), B, L.ptr(th), L.current_stream()), "fb_qnet_forward_quantiles")
        return th

    def forward(self, states, which=L.NET_ONLINE):
        _dev_check(states)
        B = states.shape[0]
        _check_states("states", states)
        q = self._get(f"q{B}", (B, self.A), torch.float32)
        L.check(L.lib().fb_qnet_forward(self.h, which, L.ptr(states), B, L.ptr(q), L.current_stream()), "fb_qnet_forward")
        return q

    def act(self, states, epsilon, seed=0, step=0, want_q=False):
        _dev_check(states)
        n = states.shape[0]
        actions = self._get(f"act{n}", (n,), torch.uint8)
        q = self._get(f"qa{n}", (n, self.A), torch.float32) if want_q else None
        L.check(L.lib().fb_qnet_act(self.h, L.ptr(states), n, float(epsilon), seed, step, L.ptr(actions), L.ptr(q),
                                    L.current_stream()), "fb_qnet_act")
        return (actions, q) if want_q else actions

    def act_nib(self, nib_states, epsilon, seed=0, step=0, want_q=False):
        """getAction for N envs straight from VecGameState.track_state()'s nibble states."""
        _dev_check(nib_states)
        n = nib_states.shape[0]
        actions = self._get(f"act{n}", (n,), torch.uint8)
        q = self._get(f"qa{n}", (n, self.A), torch.float32) if want_q else None
        L.check(L.lib().fb_qnet_act_nib(self.h, L.ptr(nib_states), n, float(epsilon), seed, step, L.ptr(actions), L.ptr(q),
                                        L.current_stream()), "fb_qnet_act_nib")
        return (actions, q) if want_q else actions

    def act_nib_env_noise(self, nib_states, epsilon, seed=0, step=0, want_q=False):
        """act_nib with independent noise per env (fb_qnet_act_nib_env_noise): env e acts through mu + sigma * its own noise, drawn
        at (seed, step); the net's own samples and parameters stay as they were"""
        self._need_noisy("act_nib_env_noise")
        _dev_check(nib_states)
        n = nib_states.shape[0]
        actions = self._get(f"act{n}", (n,), torch.uint8)
        q = self._get(f"qa{n}", (n, self.A), torch.float32) if want_q else None
        L.check(L.lib().fb_qnet_act_nib_env_noise(self.h, L.ptr(nib_states), n, float(epsilon), int(seed), int(step), L.ptr(actions), L.ptr(q),
                                                  L.current_stream()), "fb_qnet_act_nib_env_noise")
        return (actions, q) if want_q else actions

    def train_step(self, algo, s, a, r, s2, t, isw=None, gamma=0.99, flat_grad=None, want_aux=True):
        """One _trainQNetwork step.  Returns (loss f32[1], abs_err f32[B], q_target f32[B]) device tensors.
        flat_grad=None applies Adam; a float32[n_params] tensor receives the gradients instead."""
        _dev_check(s, a, r, s2, t, isw, flat_grad)
        B = s.shape[0]
        loss = self._get("loss", (1,), torch.float32)
        ae = self._get(f"ae{B}", (B,), torch.float32) if want_aux else None
        y = self._get(f"y{B}", (B,), torch.float32) if want_aux else None
        if isw is not None and isw.dtype != torch.float32:
            isw = isw.to(torch.float32)          # ISWeights is fed to a float32 placeholder
        L.check(L.lib().fb_qnet_train_step(self.h, ALGOS[algo] if isinstance(algo, str) else algo, B, L.ptr(s), L.ptr(a),
                                           L.ptr(r), L.ptr(s2), L.ptr(t), L.ptr(isw), float(gamma), L.ptr(loss), L.ptr(ae),
                                           L.ptr(y), L.ptr(flat_grad), L.current_stream()), "fb_qnet_train_step")
        return loss, ae, y

    def pg_step(self, states, actions, weights, n_total=None, flat_grad=None):
        """One policy-gradient step (FB_ALGO_PG) on <= 128 states: loss = sum over them of softmax_cross_entropy(logits, action) x
        weight / n_total (n_total defaults to the chunk size = a plain mean).  flat_grad=None applies Adam; a float32[n_params] tensor
        receives the chunk's gradient instead (episodes longer than 128: add the chunks' gradients, then apply_adam once).
        -> loss f32[1] (device)."""
        B = states.shape[0]
        zeros = self._get(f"pgt{B}", (B,), torch.uint8)
        zeros.zero_()
        loss, _, _ = self.train_step("pg", states, actions, weights, states, zeros, gamma=float(n_total or B), flat_grad=flat_grad, want_aux=False)
        return loss

    def apply_adam(self, flat_grad):
        _dev_check(flat_grad)
        L.check(L.lib().fb_qnet_apply_adam(self.h, L.ptr(flat_grad), L.current_stream()), "fb_qnet_apply_adam")


def train_from_replay(replay, net, algo, idx, gamma=0.99, flat_grad=None, isw=None, want_abs_err=False):
    """replay.gather(idx) + net.train_step(...) without the gathered copies (fb_train_from_replay): the conv trunk reads the sampled
    transitions' 1-bit frames in the ring directly.  Same results as the two calls (batch <= 256).  Prioritized replay: idx are the
    SumTree leaf indices of replay.sample, isw its importance weights; want_abs_err returns |TD error| for update_priorities.
    An n-step memory (replay.set_n_step) is read as (s, a, R, s', done) and bootstrapped with gamma^n; gamma must be the memory's.
    -> (loss f32[1], a u8[B], r f32[B], t u8[B][, abs_err f32[B]]) on the device."""
    if (replay.prioritized or algo in WEIGHTED_ALGOS) and isw is None:
        raise ValueError("the prioritized step needs the importance weights (isw)")
    _dev_check(idx, flat_grad, isw)
    B, dev = int(idx.numel()), idx.device
    a = torch.empty(B, dtype=torch.uint8, device=dev); r = torch.empty(B, dtype=torch.float32, device=dev)
    t = torch.empty(B, dtype=torch.uint8, device=dev); loss = torch.zeros(1, dtype=torch.float32, device=dev)
    ae = torch.empty(B, dtype=torch.float32, device=dev) if want_abs_err else None
    if isw is not None and isw.dtype != torch.float32:
        isw = isw.to(torch.float32)                      # ISWeights is fed to a float32 placeholder
    L.check(L.lib().fb_train_from_replay(replay.h, net.h, ALGOS[algo], B, L.ptr(idx), L.ptr(isw), L.ptr(a), L.ptr(r), L.ptr(t), float(gamma),
                                         L.ptr(loss), L.ptr(ae), L.ptr(flat_grad), L.current_stream()),
            "fb_train_from_replay")
    return (loss, a, r, t, ae) if want_abs_err else (loss, a, r, t)


def _check_flat_grad(flat_grad, n_params):
    if flat_grad is not None and (flat_grad.dtype != torch.float32 or flat_grad.numel() != n_params):
        raise ValueError(f"flat_grad must be float32[{n_params}]")


def check_chunk(B, a, n_total, flat_grad, n_params):
    """what the A2C and the PPO training calls check alike, on the host: the chunk's size, its actions, n_total, the gradient buffer"""
    if not 1 <= B <= 256:
        raise ValueError(f"an A2C chunk holds 1..256 samples, got {B}")
    if a is not None and (a.dtype != torch.uint8 or a.numel() != B):
        raise ValueError(f"a must be uint8[{B}]")
    if n_total is not None and int(n_total) < B:
        raise ValueError(f"n_total = {n_total} must be the whole update's sample count (>= the chunk's {B})")
    _check_flat_grad(flat_grad, n_params)


def check_ac_batch(B, a, adv, ret, n_total, flat_grad, n_params):
    """the shape checks of the two A2C training calls, on the host"""
    check_chunk(B, a, n_total, flat_grad, n_params)
    for name, t in (("adv", adv), ("ret", ret)):
        if t.dtype != torch.float32 or t.numel() != B:
            raise ValueError(f"{name} must be float32[{B}]")


def check_sac_batch(B, a, r, t, flat_grad, n_params, what="a SAC batch"):
    """the shape checks of the SAC training calls, on the host"""
    if not 1 <= B <= 256:
        raise ValueError(f"{what} holds 1..256 samples, got {B}")
    for name, x, dt in (("a", a, torch.uint8), ("r", r, torch.float32), ("t", t, torch.uint8)):
        if x is not None and (x.dtype != dt or x.numel() != B):
            raise ValueError(f"{name} must be {dt}[{B}]")
    _check_flat_grad(flat_grad, n_params)


def check_iqn_batch(B, a, r, t, tau, tau_next, n_tau, n_tau_next, flat_grad, n_params):
    """the shape checks of the two IQN training calls, on the host: check_sac_batch's, with the two tau tensors in front of flat_grad"""
    check_sac_batch(B, a, r, t, None, n_params, "an IQN batch")
    for name, x, n in (("tau", tau, n_tau), ("tau_next", tau_next, n_tau_next)):
        if x is not None and (x.dtype != torch.float32 or tuple(x.shape) != (B, n) or not x.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous float32[{B}, {n}]")
    _check_flat_grad(flat_grad, n_params)


def check_isw(B, isw):
    """the shape check of the prioritized IQN and SAC calls' importance weights, on the host"""
    if isw is None or isw.dtype != torch.float32 or tuple(isw.shape) != (B,) or not isw.is_contiguous():
        raise ValueError(f"isw must be a contiguous float32[{B}] (the prioritized step needs the importance weights)")


def _ring_call(name, replay, net, arch, need, reads, idx, n_loss, *tensors, prioritized=False):
    """what the four *_train_from_replay calls of the newer families begin with: the net's arch, a uniform memory (prioritized=True: a
    prioritized one), device tensors, idx's dtype -> (B, dev, a u8[B], loss f32[n_loss]), the last two for the library to fill"""
    if net.arch not in (arch if isinstance(arch, tuple) else (arch,)):
        raise ValueError(f"{name} needs {need}")
    if prioritized and not replay.prioritized:
        raise ValueError(f"{name} {reads} a prioritized memory only")
    if replay.prioritized and not prioritized:
        raise ValueError(f"{name} {reads} a uniform memory only")
    _dev_check(idx, *tensors)
    if idx.dtype != torch.int64:
        raise ValueError("idx must be int64[B]")
    B, dev = int(idx.numel()), idx.device
    return B, dev, torch.empty(B, dtype=torch.uint8, device=dev), torch.zeros(n_loss, dtype=torch.float32, device=dev)


def iqn_draw_taus(batch, n, seed=0, step=0, which=0, device="cuda"):
    """the tau the IQN train step draws for (seed, step) when it is given none (fb_iqn_draw_taus; stateless): float32[batch, n], strictly
    inside (0, 1); which 0: the online tau, 1: the target's tau'"""
    if not 1 <= int(batch) <= (1 << 20) or not 1 <= int(n) <= 64 or which not in (0, 1):
        raise ValueError(f"iqn_draw_taus: batch in 1..2^20, n in 1..64, which 0 or 1 (got {batch}, {n}, {which})")
    L.require_gpu()
    out = torch.empty((int(batch), int(n)), dtype=torch.float32, device=device)
    L.check(L.lib().fb_iqn_draw_taus(int(batch), int(n), int(seed), int(step), int(which), L.ptr(out), L.current_stream()), "fb_iqn_draw_taus")
    return out


def _iqn_train_from_replay(name, replay, net, idx, isw, gamma, double_q, tau, tau_next, seed, step, flat_grad, want_target):
    """iqn_train_from_replay, and with `name` == 'iqn_per_train_from_replay' its prioritized form (a prioritized memory, isw in, abs_err out)
    -> (loss f32[1], a u8[B], r f32[B], t u8[B], q_target f32[B, n_tau_next] or None, abs_err f32[B] or None)"""
    weighted = name == "iqn_per_train_from_replay"
    B, dev, a, loss = _ring_call(name, replay, net, IQN_ALL_ARCHS, "an IQN net (QNet(..., arch='iqn'))", "trains from", idx, 1, flat_grad, tau, tau_next, isw,
                                 prioritized=weighted)
    N, Np = net.iqn()[:2]
    check_iqn_batch(B, None, None, None, tau, tau_next, N, Np, flat_grad, net.n_params)
    if weighted:
        check_isw(B, isw)
    r, t = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    ae = torch.empty(B, dtype=torch.float32, device=dev) if weighted else None
    y = torch.empty((B, Np), dtype=torch.float32, device=dev) if want_target else None
    batch = (replay.h, net.h, int(bool(double_q)), B, L.ptr(idx))
    art = (L.ptr(a), L.ptr(r), L.ptr(t), L.ptr(tau), L.ptr(tau_next), int(seed), int(step), float(gamma), L.ptr(loss))
    out = (L.ptr(y), L.ptr(flat_grad), L.current_stream())
    if weighted:
        L.check(L.lib().fb_iqn_per_train_from_replay(*batch, L.ptr(isw), *art, L.ptr(ae), *out), "fb_iqn_per_train_from_replay")
    else:
        L.check(L.lib().fb_iqn_train_from_replay(*batch, *art, *out), "fb_iqn_train_from_replay")
    return loss, a, r, t, y, ae


def iqn_train_from_replay(replay, net, idx, gamma=0.99, double_q=False, tau=None, tau_next=None, seed=0, step=0, flat_grad=None,
                          want_target=False):
    """QNet.iqn_train_step on the transitions at the deque positions idx of a uniform memory (any n-step view; gamma must be the memory's),
    read from its frame ring in place (fb_iqn_train_from_replay)
    -> (loss f32[1], a u8[B], r f32[B], t u8[B][, q_target f32[B, n_tau_next]])"""
    loss, a, r, t, y, _ = _iqn_train_from_replay("iqn_train_from_replay", replay, net, idx, None, gamma, double_q, tau, tau_next, seed, step, flat_grad,
                                                 want_target)
    return (loss, a, r, t, y) if want_target else (loss, a, r, t)


def iqn_per_train_from_replay(replay, net, idx, isw, gamma=0.99, double_q=False, tau=None, tau_next=None, seed=0, step=0, flat_grad=None,
                              want_target=False):
    """QNet.iqn_per_train_step on the transitions at the SumTree leaves idx of a prioritized memory (any n-step view; gamma must be the
    memory's), read from its frame ring in place (fb_iqn_per_train_from_replay); isw f32[B]: replay.sample's importance weights
    -> (loss f32[1], a u8[B], r f32[B], t u8[B][, q_target f32[B, n_tau_next]], abs_err f32[B])"""
    loss, a, r, t, y, ae = _iqn_train_from_replay("iqn_per_train_from_replay", replay, net, idx, isw, gamma, double_q, tau, tau_next, seed, step,
                                                  flat_grad, want_target)
    return (loss, a, r, t, y, ae) if want_target else (loss, a, r, t, ae)


def _sac_train_from_replay(name, replay, net, idx, isw, gamma, flat_grad, want_target):
    """sac_train_from_replay, and with `name` == 'sac_per_train_from_replay' its prioritized form (a prioritized memory, isw in, abs_err out)
    -> (loss f32[6], a u8[B], r f32[B], t u8[B], q_target f32[B] or None, abs_err f32[B] or None)"""
    weighted = name == "sac_per_train_from_replay"
    B, dev, a, loss = _ring_call(name, replay, net, SAC_ARCH, "a SAC net (QNet(..., arch='sac'))", "trains from", idx, 6, flat_grad, isw, prioritized=weighted)
    check_sac_batch(B, None, None, None, flat_grad, net.n_params)
    if weighted:
        check_isw(B, isw)
    r, t = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
    ae = torch.empty(B, dtype=torch.float32, device=dev) if weighted else None
    y = torch.empty(B, dtype=torch.float32, device=dev) if want_target else None
    batch = (replay.h, net.h, B, L.ptr(idx))
    art = (L.ptr(a), L.ptr(r), L.ptr(t), float(gamma), L.ptr(loss))
    out = (L.ptr(y), L.ptr(flat_grad), L.current_stream())
    if weighted:
        L.check(L.lib().fb_sac_per_train_from_replay(*batch, L.ptr(isw), *art, L.ptr(ae), *out), "fb_sac_per_train_from_replay")
    else:
        L.check(L.lib().fb_sac_train_from_replay(*batch, *art, *out), "fb_sac_train_from_replay")
    return loss, a, r, t, y, ae


def sac_train_from_replay(replay, net, idx, gamma=0.99, flat_grad=None, want_target=False):
    """QNet.sac_train_step on the transitions at the deque positions idx of a uniform memory at n-step 1, read from its frame ring in
    place (fb_sac_train_from_replay) -> (loss f32[6], a u8[B], r f32[B], t u8[B][, q_target f32[B]])"""
    loss, a, r, t, y, _ = _sac_train_from_replay("sac_train_from_replay", replay, net, idx, None, gamma, flat_grad, want_target)
    return (loss, a, r, t, y) if want_target else (loss, a, r, t)


def sac_per_train_from_replay(replay, net, idx, isw, gamma=0.99, flat_grad=None, want_target=False):
    """QNet.sac_per_train_step on the transitions at the SumTree leaves idx of a prioritized memory (at the n it was made with; gamma
    must be the memory's), read from its frame ring in place (fb_sac_per_train_from_replay); isw f32[B]: replay.sample's importance
    weights -> (loss f32[6], a u8[B], r f32[B], t u8[B][, q_target f32[B]], abs_err f32[B])"""
    loss, a, r, t, y, ae = _sac_train_from_replay("sac_per_train_from_replay", replay, net, idx, isw, gamma, flat_grad, want_target)
    return (loss, a, r, t, y, ae) if want_target else (loss, a, r, t, ae)


def ac_gae(reward, terminal, value, gamma=0.99, gae_lambda=0.95):
    """generalised advantage estimation on the device (fb_ac_gae): reward f32[T, N], terminal u8[T, N], value f32[T + 1, N] (row T: the
    bootstrap V(s_T)) -> (adv f32[T, N], ret f32[T, N]); float64 arithmetic in the order include/fbdqn.h pins"""
    g, l = check_gae(gamma, gae_lambda)
    _dev_check(reward, terminal, value)
    if reward.dim() != 2 or reward.dtype != torch.float32:
        raise ValueError("reward must be float32[T,N]")
    T, N = reward.shape
    if terminal.dtype != torch.uint8 or tuple(terminal.shape) != (T, N):
        raise ValueError(f"terminal must be uint8[{T},{N}]")
    if value.dtype != torch.float32 or tuple(value.shape) != (T + 1, N):
        raise ValueError(f"value must be float32[{T + 1},{N}] (row T: the bootstrap value)")
    adv, ret = torch.empty_like(reward), torch.empty_like(reward)
    L.check(L.lib().fb_ac_gae(L.ptr(reward), L.ptr(terminal), L.ptr(value), T, N, g, l, L.ptr(adv), L.ptr(ret), L.current_stream()), "fb_ac_gae")
    return adv, ret


def ac_train_from_replay(replay, net, idx, adv, ret, n_total=None, flat_grad=None):
    """QNet.ac_train_step on the transitions at the deque positions idx of a uniform memory, read from its frame ring in place
    (fb_ac_train_from_replay) -> (loss f32[4], a u8[B]: the ring's actions)"""
    B, _, a, loss = _ring_call("ac_train_from_replay", replay, net, AC_ARCH, "an actor-critic net (QNet(..., arch='ac'))", "reads the rollout from", idx, 4,
                               adv, ret, flat_grad)
    check_ac_batch(B, None, adv, ret, n_total, flat_grad, net.n_params)
    L.check(L.lib().fb_ac_train_from_replay(replay.h, net.h, B, L.ptr(idx), L.ptr(adv), L.ptr(ret), int(n_total or B), L.ptr(a), L.ptr(loss),
                                            L.ptr(flat_grad), L.current_stream()), "fb_ac_train_from_replay")
    return loss, a


def check_ppo_batch(B, sel, adv, ret, logp_old, value_old):
    """the shape checks PPO's training calls add to check_ac_batch's: without sel the four buffers hold the chunk's B samples, with sel
    (int64[B]) they are the rollout's, of one length, read at sel[b]"""
    if sel is not None and (sel.dtype != torch.int64 or sel.numel() != B):
        raise ValueError(f"sel must be int64[{B}]")
    n = B if sel is None else int(adv.numel())
    if n < 1:
        raise ValueError("adv is empty")
    for name, t in (("adv", adv), ("ret", ret), ("logp_old", logp_old), ("value_old", value_old)):
        if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32[{n}]")


def ppo_train_from_replay(replay, net, idx, adv, ret, logp_old, value_old, sel=None, n_total=None, flat_grad=None, check_sel=True):
    """QNet.ppo_train_step on the transitions at the deque positions idx of a uniform memory, read from its frame ring in place
    (fb_ppo_train_from_replay).  sel int64[B]: sample b reads adv / ret / logp_old / value_old (the rollout's flattened buffers, one
    length) at sel[b].  The library takes sel as it comes (its ABI carries no length), so sel is checked against the buffers here.
    THAT CHECK IS A HOST SYNC ON EVERY CALL WITH sel (it reads sel back from the device and waits for the stream): a loop, or anyone
    who times this call, passes check_sel=False, which is safe for a sel that is in range by construction (a permutation's slice:
    VecActorCritic, tools/time_ppo.py).  -> (loss f32[6], a u8[B]: the ring's actions)"""
    B, _, a, loss = _ring_call("ppo_train_from_replay", replay, net, AC_ARCH, "an actor-critic net (QNet(..., arch='ac'))", "reads the rollout from", idx, 6,
                               sel, adv, ret, logp_old, value_old, flat_grad)
    check_chunk(B, None, n_total, flat_grad, net.n_params)
    check_ppo_batch(B, sel, adv, ret, logp_old, value_old)
    if sel is not None and check_sel and not bool(((sel >= 0) & (sel < adv.numel())).all()):      # (reads sel back: one host sync)
        raise ValueError(f"sel must lie in 0..{adv.numel() - 1}, the rollout buffers' positions")
    L.check(L.lib().fb_ppo_train_from_replay(replay.h, net.h, B, L.ptr(idx), L.ptr(sel), L.ptr(adv), L.ptr(ret), L.ptr(logp_old), L.ptr(value_old),
                                             int(n_total or B), L.ptr(a), L.ptr(loss), L.ptr(flat_grad), L.current_stream()),
            "fb_ppo_train_from_replay")
    return loss, a


def ac_normalize_adv(adv, out=None):
    """the rollout's advantages to mean 0 and standard deviation 1 on the device (fb_ac_normalize_adv: float64, the order
    include/fbdqn.h pins) -> out (a new tensor of adv's shape; out=adv normalises in place)"""
    _dev_check(adv, out)
    if adv.dtype != torch.float32 or adv.numel() < 1 or not adv.is_contiguous():
        raise ValueError("adv must be a contiguous, non-empty float32 tensor")
    out = torch.empty_like(adv) if out is None else out
    if out.dtype != torch.float32 or out.numel() != adv.numel() or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32[{adv.numel()}]")
    L.check(L.lib().fb_ac_normalize_adv(L.ptr(adv), int(adv.numel()), L.ptr(out), L.current_stream()), "fb_ac_normalize_adv")
    return out


def ac_permute(n, seed=0, draw=0, out=None, device="cuda"):
    """a permutation of range(n) as int64[n] on the device, a function of (n, seed, draw) alone (fb_ac_permute: a keyed Feistel
    network over Philox, cycle-walked; no state)"""
    n = int(n)
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"n must be in 1..2^31 - 1, got {n}")
    _dev_check(out)
    out = torch.empty(n, dtype=torch.int64, device=device) if out is None else out
    if out.dtype != torch.int64 or out.numel() != n or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous int64[{n}]")
    L.check(L.lib().fb_ac_permute(n, int(seed) & (2 ** 64 - 1), int(draw) & (2 ** 64 - 1), L.ptr(out), L.current_stream()), "fb_ac_permute")
    return out


def _check_sel(sel, n, check_sel):
    """sel int64, inside buffers of n elements (check_sel: read back from the device, ONE HOST SYNC, as ppo_train_from_replay's)"""
    if sel.dtype != torch.int64 or sel.numel() < 1:
        raise ValueError("sel must be a non-empty int64 tensor")
    if check_sel and not bool(((sel >= 0) & (sel < n)).all()):
        raise ValueError(f"sel must lie in 0..{n - 1}, the rollout buffers' positions")


def ac_normalize_adv_sel(adv, sel, out, check_sel=True):
    """the advantages adv[sel] (one minibatch) to mean 0 and standard deviation 1 over themselves, written to out[sel]
    (fb_ac_normalize_adv_sel: float64, the order include/fbdqn.h pins); the other positions of out are not written, and out is not adv.
    sel int64[n]: distinct positions (a permutation's slice); check_sel=False skips the range check's host sync -> out"""
    _dev_check(adv, sel, out)
    if adv.dtype != torch.float32 or adv.numel() < 1:
        raise ValueError("adv must be a contiguous, non-empty float32 tensor")
    if out.dtype != torch.float32 or out.numel() != adv.numel():
        raise ValueError(f"out must be a contiguous float32[{adv.numel()}]")
    _check_sel(sel, adv.numel(), check_sel)
    L.check(L.lib().fb_ac_normalize_adv_sel(L.ptr(adv), L.ptr(sel), int(sel.numel()), L.ptr(out), L.current_stream()), "fb_ac_normalize_adv_sel")
    return out


def ac_grad_accumulate(acc, chunk, first):
    """acc = (0 if first else acc) + chunk on the device, one fp32 add per element (fb_ac_grad_accumulate): what acc.zero_() and
    acc += chunk give, in one launch -> acc"""
    _dev_check(acc, chunk)
    if acc.dtype != torch.float32 or chunk.dtype != torch.float32 or acc.numel() != chunk.numel() or acc.numel() < 1:
        raise ValueError("acc and chunk must be non-empty float32 tensors of one length")
    L.check(L.lib().fb_ac_grad_accumulate(L.ptr(acc), L.ptr(chunk), int(acc.numel()), int(bool(first)), L.current_stream()), "fb_ac_grad_accumulate")
    return acc


def ppo_epoch(replay, net, pos, sel, adv, ret, logp_old, value_old, minibatches, grad, chunk_grad, loss_rows, epoch_mean, a_out=None,
              adv_scratch=None, check_sel=True):
    """one PPO epoch as one host call (fb_ppo_epoch): `minibatches` consecutive minibatches of pos / sel (int64[n]: the ring positions and
    the rollout-buffer indices of the epoch's n transitions), each read in ring-fed chunks of <= 256 whose gradients are summed into grad
    (chunk_grad: the chunk's), clipped if the net clips, and applied by Adam.  adv_scratch (float32 of adv's size, not adv): every
    minibatch's advantages are normalised over the minibatch into it first.  loss_rows float32[minibatches, 6] receives the minibatches'
    six loss numbers, epoch_mean float32[6] their mean.  Bit for bit the composed calls (ppo_train_from_replay, ac_grad_accumulate,
    QNet.clip_grad, QNet.apply_adam); nothing is read back.  check_sel as for ppo_train_from_replay -> (epoch_mean, a_out u8[256])"""
    if net.arch != AC_ARCH:
        raise ValueError("ppo_epoch needs an actor-critic net (QNet(..., arch='ac'))")
    if replay.prioritized:
        raise ValueError("ppo_epoch reads the rollout from a uniform memory only")
    _dev_check(pos, sel, adv, ret, logp_old, value_old, grad, chunk_grad, loss_rows, epoch_mean, a_out, adv_scratch)
    n, m = int(pos.numel()), int(minibatches)
    if pos.dtype != torch.int64 or n < 1:
        raise ValueError("pos must be a non-empty int64 tensor")
    if sel.numel() != n:
        raise ValueError(f"sel must be int64[{n}]")
    if m < 1 or n % m:
        raise ValueError(f"minibatches must be >= 1 and divide the epoch's {n} transitions, got {minibatches}")
    check_ppo_batch(n, sel, adv, ret, logp_old, value_old)
    _check_sel(sel, adv.numel(), check_sel)
    _check_flat_grad(grad, net.n_params)
    _check_flat_grad(chunk_grad, net.n_params)
    if adv_scratch is not None and (adv_scratch.dtype != torch.float32 or adv_scratch.numel() != adv.numel()):
        raise ValueError(f"adv_scratch must be a contiguous float32[{adv.numel()}]")
    if loss_rows.dtype != torch.float32 or loss_rows.numel() != 6 * m:
        raise ValueError(f"loss_rows must be float32[{m}, 6]")
    if epoch_mean.dtype != torch.float32 or epoch_mean.numel() != 6:
        raise ValueError("epoch_mean must be float32[6]")
    a_out = torch.empty(256, dtype=torch.uint8, device=pos.device) if a_out is None else a_out
    if a_out.dtype != torch.uint8 or a_out.numel() < 256:
        raise ValueError("a_out must be uint8[256]")
    L.check(L.lib().fb_ppo_epoch(replay.h, net.h, n, m, L.ptr(pos), L.ptr(sel), L.ptr(adv), L.ptr(ret), L.ptr(logp_old), L.ptr(value_old),
                                 int(adv_scratch is not None), L.ptr(adv_scratch), L.ptr(grad), L.ptr(chunk_grad), L.ptr(a_out), L.ptr(loss_rows),
                                 L.ptr(epoch_mean), L.current_stream()), "fb_ppo_epoch")
    return epoch_mean, a_out


def ppo_epoch_sum(net, out):
    """the running sum of the chunks' six loss numbers over the net's last ppo_epoch, in the order one accumulator fed chunk by chunk
    adds them (fb_ppo_epoch_sum), into out float32[6] -> out"""
    if net.arch != AC_ARCH:
        raise ValueError("ppo_epoch_sum needs an actor-critic net (QNet(..., arch='ac'))")
    _dev_check(out)
    if out.dtype != torch.float32 or out.numel() != 6:
        raise ValueError("out must be float32[6]")
    L.check(L.lib().fb_ppo_epoch_sum(net.h, L.ptr(out), L.current_stream()), "fb_ppo_epoch_sum")
    return out


class AcRolloutStep:
    """One step of an A2C rollout as a single host call (fb_ac_rollout_step): sample the policy (value and log-probability into row
    `slot` of the rollout buffers) -> frame_step (reward / terminal into row `slot`) -> store.  The results of QNet.act_policy_nib,
    VecGameState.frame_step and VecReplay.push in that order; the pointers are bound once."""

    def __init__(self, env, replay, net, rollout):
        if net.arch != AC_ARCH:
            raise ValueError("AcRolloutStep needs an actor-critic net (QNet(..., arch='ac'))")
        if replay.prioritized:
            raise ValueError("AcRolloutStep stores the rollout in a uniform memory only")
        if getattr(env, "nib", None) is None:
            raise ValueError("call env.track_state() first: the acting path reads the env kernel's nibble states")
        self.T = check_rollout(rollout)
        self.env, self.replay, self.net = env, replay, net
        dev, N = env.device, env.n
        self.actions = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.reward = torch.zeros((self.T, N), dtype=torch.float32, device=dev)
        self.terminal = torch.zeros((self.T, N), dtype=torch.uint8, device=dev)
        self.value = torch.zeros((self.T + 1, N), dtype=torch.float32, device=dev)      # (row T: the bootstrap value, the caller's)
        self.logp = torch.zeros((self.T, N), dtype=torch.float32, device=dev)
        p = lambda x: x.data_ptr()
        self.buf = L.AcRolloutBuffers(p(env.nib), p(self.actions), p(env.frame_bits), p(self.reward), p(self.terminal), p(env.score),
                                      p(self.value), p(self.logp), self.T)

    def __call__(self, slot, seed=0, step=0):
        """-> actions uint8[N] (device); row `slot` of reward / terminal / value / logp is written"""
        L.check(L.lib().fb_ac_rollout_step(self.env.h, self.replay.h, self.net.h, C.byref(self.buf), self.env.n, int(seed), int(step), int(slot),
                                           L.current_stream()), "fb_ac_rollout_step")
        return self.actions


def _bind_step(self, name, arch, need, env, replay, net, batch, gamma, flat_grad, n_loss, prioritized=False):
    """what SacStep, SacPerStep, IqnStep and IqnPerStep set up alike: the checks, the step's own tensors (loss: f32[n_loss]) and the bound pointers;
    prioritized: a prioritized memory instead of a uniform one, and Memory.sample's weights (f64 and f32) and abs_err beside them"""
    if net.arch not in (arch if isinstance(arch, tuple) else (arch,)):
        raise ValueError(f"{name} needs {need}")
    if prioritized and not replay.prioritized:
        raise ValueError(f"{name} trains from a prioritized memory only")
    if replay.prioritized and not prioritized:
        raise ValueError(f"{name} trains from a uniform memory only")
    if getattr(env, "nib", None) is None:
        raise ValueError("call env.track_state() first: the acting path reads the env kernel's nibble states")
    if not 1 <= int(batch) <= 256:
        raise ValueError(f"batch must be in 1..256, got {batch}")
    _dev_check(flat_grad)
    self.env, self.replay, self.net = env, replay, net
    self.batch, self.gamma, self.flat_grad = int(batch), float(gamma), flat_grad
    dev, B = env.device, self.batch
    self.actions = torch.zeros(env.n, dtype=torch.uint8, device=dev)
    self.idx = torch.zeros(B, dtype=torch.int64, device=dev)
    self.a = torch.empty(B, dtype=torch.uint8, device=dev)
    self.r = torch.empty(B, dtype=torch.float32, device=dev)
    self.t = torch.empty(B, dtype=torch.uint8, device=dev)
    self.loss = torch.zeros(n_loss, dtype=torch.float32, device=dev)
    self.isw = torch.zeros(B, dtype=torch.float64, device=dev) if prioritized else None
    self.isw32 = torch.zeros(B, dtype=torch.float32, device=dev) if prioritized else None
    self.abs_err = torch.zeros(B, dtype=torch.float32, device=dev) if prioritized else None
    p = lambda x: None if x is None else x.data_ptr()
    self.buf = L.StepBuffers(p(env.nib), p(self.actions), p(env.frame_bits), p(env.reward), p(env.terminal), p(env.score),
                             p(self.idx), None, None, p(self.a), p(self.t), p(self.r), p(self.loss), p(flat_grad),
                             p(self.isw), p(self.isw32), p(self.abs_err))


class SacStep:
    """One whole step of the SAC loop as a single host call (fb_sac_step): sample the policy -> frame_step -> store + sample the
    minibatch -> (train) the SAC step from the ring -> (polyak > 0) the soft target update.  The results of the separate calls in that
    order; the pointers are bound once."""
    entry, prioritized = "fb_sac_step", False

    def __init__(self, env, replay, net, batch=32, gamma=0.99, polyak=0.005, flat_grad=None):
        _bind_step(self, type(self).__name__, SAC_ARCH, "a SAC net (QNet(..., arch='sac'))", env, replay, net, batch, gamma, flat_grad, 6,
                   prioritized=self.prioritized)
        self.rho = check_polyak(polyak, allow_off=True)

    def __call__(self, seed=0, step=0, train=True):
        """-> actions uint8[N] (device); rewards / terminals / scores are the env's tensors, the six loss numbers are self.loss"""
        L.check(getattr(L.lib(), self.entry)(self.env.h, self.replay.h, self.net.h, C.byref(self.buf), self.env.n, self.batch, int(seed), int(step),
                                            int(bool(train)), self.gamma, self.rho, L.current_stream()), self.entry)
        return self.actions


class SacPerStep(SacStep):
    """SacStep on a prioritized memory (fb_sac_per_step): sample the policy -> frame_step -> store -> (train) Memory.sample -> the
    weighted SAC step from the ring -> Memory.batch_update with 0.5 (|d1| + |d2|) -> (polyak > 0) the soft target update, all in line on
    one stream.  The results of the separate calls in that order; it owns idx, isw (f64), isw32 and abs_err (as the loss left it).  On a
    memory made with n_step > 1 a training step needs n pushes at its draw: the first n - 1 steps are store-only (train=False)."""
    entry, prioritized = "fb_sac_per_step", True


class _IqnStep:
    """what IqnStep and IqnPerStep are: the pointers bound once, and one host call per step (`entry`; prioritized: the kind of memory it takes)"""
    entry, prioritized = None, False

    def __init__(self, env, replay, net, batch=32, gamma=0.99, double_q=False, flat_grad=None):
        _bind_step(self, type(self).__name__, IQN_ALL_ARCHS, "an IQN net (QNet(..., arch='iqn'))", env, replay, net, batch, gamma, flat_grad, 1,
                   prioritized=self.prioritized)
        self.double_q = bool(double_q)

    def __call__(self, epsilon=0.0, seed=0, step=0, train=True):
        """-> actions uint8[N] (device); rewards / terminals / scores are the env's tensors, the loss is self.loss"""
        L.check(getattr(L.lib(), self.entry)(self.env.h, self.replay.h, self.net.h, C.byref(self.buf), self.env.n, int(self.double_q), self.batch,
                                            float(epsilon), int(seed), int(step), int(bool(train)), self.gamma, L.current_stream()), self.entry)
        return self.actions


class IqnStep(_IqnStep):
    """One whole step of the IQN loop as a single host call (fb_iqn_step): epsilon-greedy on the folded head -> frame_step -> store +
    sample the minibatch -> (train) the IQN step from the ring, its tau drawn from (seed, step).  The results of the separate calls in
    that order; the pointers are bound once."""
    entry = "fb_iqn_step"


class IqnPerStep(_IqnStep):
    """IqnStep on a prioritized memory (fb_iqn_per_step): epsilon-greedy on the folded head -> frame_step -> store -> (train) Memory.sample
    -> the weighted IQN step from the ring -> Memory.batch_update with the per-sample loss, all in line on one stream.  The results of the
    separate calls in that order; it owns idx, isw (f64), isw32 and abs_err (l_b as the loss left it)."""
    entry, prioritized = "fb_iqn_per_step", True


class TrainSteps:
    """n x (random.sample -> minibatch -> _trainQNetwork) on a uniform memory that is not being pushed to, as one host call
    (fb_train_steps): the separate calls' results, with the next step's random.sample riding in the conv3 backward launch.  On an
    n-step memory gamma must be the memory's (the steps bootstrap with gamma^n)."""

    def __init__(self, replay, net, batch=32, algo="dqn", gamma=0.99):
        if replay.prioritized or algo in WEIGHTED_ALGOS:
            raise ValueError("TrainSteps is for uniform replay (PER needs the importance weights: use the separate calls)")
        self.replay, self.net, self.batch, self.algo, self.gamma = replay, net, batch, ALGOS[algo], float(gamma)
        dev, B = replay.device, batch
        self.idx = torch.zeros(2 * B, dtype=torch.int64, device=dev)     # two buffers, used alternately
        self.s = torch.empty((B, 80, 80, 4), dtype=torch.uint8, device=dev)
        self.s2 = torch.empty((B, 80, 80, 4), dtype=torch.uint8, device=dev)
        self.a = torch.empty(B, dtype=torch.uint8, device=dev)
        self.r = torch.empty(B, dtype=torch.float32, device=dev)
        self.t = torch.empty(B, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)

    def __call__(self, n_steps=1):
        L.check(L.lib().fb_train_steps(self.replay.h, self.net.h, self.algo, self.batch, int(n_steps), L.ptr(self.idx), L.ptr(self.s),
                                       L.ptr(self.s2), L.ptr(self.a), L.ptr(self.r), L.ptr(self.t), L.ptr(self.loss), self.gamma,
                                       L.current_stream()), "fb_train_steps")
        return self.loss


class VecStep:
    """One whole step of the vectorised loop (FlappyBirdDQN.py:72-76 for N envs) as a single
    host call, fb_vec_step: getAction -> frame_step -> store + sample -> minibatch -> _trainQNetwork (prioritized memories: ->
    Memory.batch_update as well).
    The same C-ABI calls in the same order as the separate VecGameState / VecReplay / QNet methods (identical
    results); the pointers are bound once, so the interpreter spends one ctypes call per step instead of five."""

    def __init__(self, env, replay, net, batch=32, algo="dqn", gamma=0.99, flat_grad=None, dist=None, mean_loss=False):
        """flat_grad: export the gradient instead of applying Adam (data parallel; the caller all-reduces and calls net.apply_adam).
        dist: a dist.NativeDP -- then the call is fb_vec_step_dp: the step, the all-reduce of flat_grad through the library's own
        RCCL communicator (overlapped with the conv backward) and Adam, all in the one host call; mean_loss divides by the world size."""
        if algo in C51_ALGOS and replay.prioritized:
            raise ValueError(f"algo {algo!r} trains from a uniform memory only (prioritized replay with C51 is not supported)")
        if algo in C51_ALGOS + C51_PER_ALGOS and dist is not None:
            raise ValueError(f"algo {algo!r}: data-parallel C51 is not supported (one GPU only)")
        if algo in QR_ALGOS and replay.prioritized:
            raise ValueError(f"algo {algo!r} trains from a uniform memory only (QR with prioritized replay is 'qrper' / 'qrdoubleper')")
        if algo in QR_ALGOS + QR_PER_ALGOS and dist is not None:
            raise ValueError(f"algo {algo!r}: data-parallel QR is not supported (one GPU only)")
        if replay.prioritized != (algo in WEIGHTED_ALGOS):
            raise ValueError(f"algos {WEIGHTED_ALGOS} go with a prioritized memory, every other algo with a uniform one (algo {algo!r})")
        if dist is not None and flat_grad is None:
            raise ValueError("VecStep(dist=...) needs the flat_grad buffer the gradient is reduced in")
        self.dist, self.mean_loss = dist, int(bool(mean_loss))
        if getattr(env, "nib", None) is None:
            raise ValueError("call env.track_state() first: the acting path reads the env kernel's nibble states")
        _dev_check(flat_grad)
        self.env, self.replay, self.net = env, replay, net
        self.batch, self.algo, self.gamma, self.flat_grad = batch, ALGOS[algo], float(gamma), flat_grad
        dev, B = env.device, batch
        self.actions = torch.zeros(env.n, dtype=torch.uint8, device=dev)
        self.idx = torch.zeros(B, dtype=torch.int64, device=dev)
        self.s = torch.empty((B, 80, 80, 4), dtype=torch.uint8, device=dev)
        self.s2 = torch.empty((B, 80, 80, 4), dtype=torch.uint8, device=dev)
        self.a = torch.empty(B, dtype=torch.uint8, device=dev)
        self.r = torch.empty(B, dtype=torch.float32, device=dev)
        self.t = torch.empty(B, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        per = algo in WEIGHTED_ALGOS                       # Memory.sample's weights (f64, and as the float32 placeholder takes them), |TD errors|
        self.isw = torch.zeros(B, dtype=torch.float64, device=dev) if per else None
        self.isw32 = torch.zeros(B, dtype=torch.float32, device=dev) if per else None
        self.abs_err = torch.zeros(B, dtype=torch.float32, device=dev) if per else None
        p = lambda x: None if x is None else x.data_ptr()
        self.buf = L.StepBuffers(p(env.nib), p(self.actions), p(env.frame_bits), p(env.reward), p(env.terminal), p(env.score),
                                 p(self.idx), p(self.s), p(self.s2), p(self.a), p(self.t), p(self.r), p(self.loss), p(flat_grad),
                                 p(self.isw), p(self.isw32), p(self.abs_err))

    def __call__(self, epsilon, seed=0, step=0, train=True):
        """-> actions uint8[N] (device); rewards / terminals / scores are the env's tensors, loss is self.loss."""
        if self.dist is not None:
            L.check(L.lib().fb_vec_step_dp(self.dist.handle, self.env.h, self.replay.h, self.net.h, C.byref(self.buf), self.env.n, self.algo,
                                           self.batch, float(epsilon), int(seed), int(step), int(bool(train)), self.gamma, self.mean_loss,
                                           L.current_stream()), "fb_vec_step_dp")
            return self.actions
        L.check(L.lib().fb_vec_step(self.env.h, self.replay.h, self.net.h, C.byref(self.buf), self.env.n, self.algo, self.batch,
                                    float(epsilon), int(seed), int(step), int(bool(train)), self.gamma, L.current_stream()),
                "fb_vec_step")
        return self.actions
