"""ctypes binding of libfbdqn.so (include/fbdqn.h).

The HIP library is the product: there is no CPU fallback.  `lib()` raises if the
shared object is missing, and `require_gpu()` raises if no MI355X is visible, so a
GPU box can never silently run anything else.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FB_LIB") or os.path.join(_HERE, "libfbdqn.so")      # FB_LIB: an ablation / tuning build (tools/)
ASSET_BLOB = os.path.join(_HERE, "assets", "sprites.bin")

FB_OK = 0
REPLAY_UNIFORM, REPLAY_PER = 0, 1
RNG_CPYTHON, RNG_PHILOX, RNG_NUMPY = 0, 1, 2
ARCH_PLAIN, ARCH_DUELING, ARCH_C51, ARCH_C51_DUELING = 0, 1, 2, 3
NET_ONLINE, NET_TARGET = 0, 1
ALGO_DQN, ALGO_NATURE, ALGO_DOUBLE, ALGO_PER, ALGO_PG = 0, 1, 2, 3, 4
ALGO_C51, ALGO_C51_DOUBLE = 5, 6
ALGO_C51_PER, ALGO_C51_DOUBLE_PER = 7, 8                # C51 with prioritized replay (include/fbdqn.h)
C51_MAX_ATOMS = 64                                    # include/fbdqn.h FB_C51_MAX_ATOMS
ARCH_QR, ARCH_QR_DUELING = 4, 5                       # quantile-regression heads (include/fbdqn.h)
ALGO_QR, ALGO_QR_DOUBLE, ALGO_QR_PER, ALGO_QR_DOUBLE_PER = 9, 10, 11, 12
ALGO_MDQN, ALGO_MDQN_PER = 14, 15                     # Munchausen-DQN on the scalar heads (include/fbdqn.h)
MDQN_DEFAULTS = (0.03, 0.9, -1.0)                     # (tau, alpha, l0) of a new scalar net: the paper's
ALGO_DOUBLE_PER = 16                                  # Double-DQN's target on a prioritized memory (include/fbdqn.h)
ARCH_AC = 6                                           # advantage actor-critic: the dueling layout read raw (include/fbdqn.h)
AC_DEFAULTS = (0.5, 0.01)                             # (value_coef, entropy_coef) of a new actor-critic net
ARCH_SAC = 7                                          # discrete soft actor-critic: a policy head and two Q heads (include/fbdqn.h)
SAC_DEFAULTS = (0.2, 0.98, 0.0)                       # (alpha, target_entropy / ln A, alpha_lr) of a new SAC net
ARCH_IQN = 8                                          # implicit quantile network: the plain layout and a cosine embedding (include/fbdqn.h)
ARCH_IQN_DUELING = 9                                  # its dueling form: W_v b_v W_a b_a read as one effective column per action (include/fbdqn.h)
IQN_DEFAULTS = (8, 8, 32, 1.0)                        # (n_tau, n_tau_next, n_tau_act, kappa) of a new IQN net; its risk setting eta starts at 1
IQN_COS = 64                                          # include/fbdqn.h FB_IQN_COS
PPO_DEFAULTS = (0.2, 0.0)                             # (clip_eps, value_clip) of a new actor-critic net; value_clip 0 = off
NOISE_SAMPLE, NOISE_MEAN = 0, 1                       # include/fbdqn.h FB_NOISE_* (fb_qnet_reset_noise)
ACT_NOISE_SHARED, ACT_NOISE_PER_ENV = 0, 1            # include/fbdqn.h FB_ACT_NOISE_* (fb_qnet_set_acting_noise)
DTYPE_F32, DTYPE_BF16 = 0, 1
PER_EXACT, PER_FAST = 0, 1
PER_INIT_MAX, PER_INIT_TD = 0, 1
NIB_PITCH, NIB_ROWS, NIB_STRIDE = 44, 84, 3712       # include/fbdqn.h FB_NIB_*
EVAL_MAX_ENVS, EVAL_MAX_EPISODES = 65536, 64         # include/fbdqn.h FB_EVAL_MAX_*
NSTEP_MAX = 16                                        # include/fbdqn.h FB_NSTEP_MAX

_vp, _i, _i64, _u64, _f, _d, _sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_size_t

# name -> argtypes; every symbol include/fbdqn.h declares (tests/test_capi_symbols.py checks the match)
SIGNATURES = {
    "fb_last_error": [],
    "fb_version": [],
    "fb_device_count": [],
    "fb_debug_abort_backtrace": [],
    "fb_env_create": [_i, _u64, C.c_uint32, _vp, _sz, _vp],
    "fb_env_destroy": [_vp],
    "fb_env_reset": [_vp, _vp],
    "fb_env_step": [_vp] * 8,
    "fb_env_observe": [_vp] * 4,
    "fb_env_get_state": [_vp, _vp],
    "fb_env_set_state": [_vp, _vp],
    "fb_env_set_gap_tape": [_vp, _vp, _i],
    "fb_env_render_full": [_vp, _i, _vp, _vp],
    "fb_env_error_count": [_vp, _vp],
    "fb_env_set_nib_buffer": [_vp, _vp],
    "fb_env_set_stats_buffer": [_vp, _vp],
    "fb_preprocess_rgb": [_vp, _vp, _i, _vp, _vp],
    "fb_replay_create": [_i64, _i, _i, _vp],
    "fb_replay_destroy": [_vp],
    "fb_replay_seed": [_vp, _i, _u64],
    "fb_replay_reset": [_vp, _vp, _vp, _vp],
    "fb_replay_push": [_vp] * 7,
    "fb_replay_push_sample": [_vp] * 6 + [_i, _vp, _vp],
    "fb_replay_current_state": [_vp, _vp, _vp],
    "fb_replay_sample": [_vp, _i, _vp, _vp, _vp, _vp],
    "fb_replay_gather": [_vp, _i] + [_vp] * 7,
    "fb_replay_profile_gather": [_vp, _i] + [_vp] * 6 + [_i, _vp],
    "fb_replay_update_priorities": [_vp, _i, _vp, _vp, _vp, _vp],
    "fb_replay_set_per_mode": [_vp, _i],
    "fb_replay_set_priority_init": [_vp, _i],
    "fb_replay_get_priority_init": [_vp, _vp],
    "fb_replay_set_prime_gamma": [_vp, _d],
    "fb_replay_get_prime_gamma": [_vp, _vp],
    "fb_replay_prime_priorities": [_vp, _vp, _vp, _i, _vp],
    "fb_replay_get_prime_state": [_vp, _vp, _sz, _vp, _vp],
    "fb_replay_set_prime_state": [_vp, _vp, _sz, _i64, _i64],
    "fb_replay_set_n_step": [_vp, _i, _d],
    "fb_replay_get_n_step": [_vp, _vp, _vp],
    "fb_replay_create_nstep": [_i64, _i, _i, _i, _d, _vp],
    "fb_replay_size": [_vp, _vp],
    "fb_replay_per_tree": [_vp] * 5,
    "fb_replay_state_bytes": [_vp, _vp],
    "fb_replay_save_state": [_vp, _vp, _sz],
    "fb_replay_load_state": [_vp, _vp, _sz],
    "fb_qnet_create": [_i, _i, _i, _i, _vp],
    "fb_qnet_create_c51": [_i, _i, _i, _f, _f, _i, _vp],
    "fb_qnet_create_c51_dueling": [_i, _i, _i, _f, _f, _i, _vp],
    "fb_qnet_create_c51_noisy": [_i, _i, _i, _i, _f, _f, _f, _i, _vp],
    "fb_qnet_is_noisy": [_vp],
    "fb_qnet_reset_noise": [_vp, _i, _u64, _u64, _i, _vp],
    "fb_qnet_get_noise": [_vp, _i, _vp],
    "fb_qnet_set_acting_noise": [_vp, _i],
    "fb_qnet_act_nib_env_noise": [_vp, _vp, _i, _f, _u64, _u64, _vp, _vp, _vp],
    "fb_qnet_get_support": [_vp] * 4,
    "fb_qnet_forward_dist": [_vp, _i, _vp, _i, _vp, _vp],
    "fb_qnet_create_qr": [_i, _i, _i, _i, _f, _i, _vp],
    "fb_qnet_get_quantiles": [_vp, _vp, _vp],
    "fb_qnet_forward_quantiles": [_vp, _i, _vp, _i, _vp, _vp],
    "fb_qnet_set_munchausen": [_vp, _f, _f, _f],
    "fb_qnet_get_munchausen": [_vp, _vp, _vp, _vp],
    "fb_qnet_set_huber": [_vp, _f],
    "fb_qnet_get_huber": [_vp, _vp],
    "fb_qnet_set_max_grad_norm": [_vp, _f],
    "fb_qnet_get_max_grad_norm": [_vp, _vp],
    "fb_qnet_clip_grad": [_vp, _vp, _vp],
    "fb_qnet_grad_norm": [_vp, _vp, _vp],
    "fb_qnet_soft_sync_target": [_vp, _f, _vp],
    "fb_qnet_create_ac": [_i, _i, _i, _vp],
    "fb_qnet_set_ac": [_vp, _f, _f],
    "fb_qnet_get_ac": [_vp, _vp, _vp],
    "fb_qnet_forward_ac": [_vp, _vp, _i, _vp, _vp, _vp],
    "fb_qnet_act_policy_nib": [_vp, _vp, _i, _u64, _u64, _i, _vp, _vp, _vp, _vp, _vp],
    "fb_ac_gae": [_vp, _vp, _vp, _i, _i, _d, _d, _vp, _vp, _vp],
    "fb_qnet_ac_train_step": [_vp, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "fb_ac_train_from_replay": [_vp, _vp, _i, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fb_ac_rollout_step": [_vp, _vp, _vp, _vp, _i, _u64, _u64, _i, _vp],
    "fb_qnet_set_ppo": [_vp, _f, _f],
    "fb_qnet_get_ppo": [_vp, _vp, _vp],
    "fb_qnet_ppo_train_step": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp],
    "fb_ppo_train_from_replay": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp],
    "fb_ac_normalize_adv": [_vp, _i64, _vp, _vp],
    "fb_ac_permute": [_i64, _u64, _u64, _vp, _vp],
    "fb_ac_normalize_adv_sel": [_vp, _vp, _i64, _vp, _vp],
    "fb_ac_grad_accumulate": [_vp, _vp, _i64, _i, _vp],
    "fb_ppo_epoch": [_vp, _vp, _i64, _i] + [_vp] * 6 + [_i] + [_vp] * 7,
    "fb_ppo_epoch_sum": [_vp, _vp, _vp],
    "fb_qnet_create_sac": [_i, _i, _i, _vp],
    "fb_qnet_set_sac": [_vp, _f, _f, _f],
    "fb_qnet_get_sac": [_vp, _vp, _vp, _vp],
    "fb_qnet_get_sac_state": [_vp, _vp],
    "fb_qnet_set_sac_state": [_vp, _vp],
    "fb_qnet_forward_sac": [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp],
    "fb_qnet_sac_train_step": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp],
    "fb_sac_train_from_replay": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp],
    "fb_sac_step": [_vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _i, _d, _f, _vp],
    "fb_qnet_sac_per_train_step": [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp],
    "fb_sac_per_train_from_replay": [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp, _vp],
    "fb_sac_per_step": [_vp, _vp, _vp, _vp, _i, _i, _u64, _u64, _i, _d, _f, _vp],
    "fb_qnet_create_iqn": [_i, _i, _i, _i, _i, _f, _i, _vp],
    "fb_qnet_create_iqn_dueling": [_i, _i, _i, _i, _i, _f, _i, _vp],
    "fb_qnet_create_iqn_noisy": [_i, _i, _i, _i, _i, _i, _f, _f, _i, _vp],
    "fb_qnet_set_iqn_risk": [_vp, _f],
    "fb_qnet_get_iqn": [_vp, _vp, _vp, _vp, _vp, _vp],
    "fb_qnet_set_iqn_munchausen": [_vp, _i, _f, _f, _f],
    "fb_qnet_get_iqn_munchausen": [_vp, _vp, _vp, _vp, _vp],
    "fb_qnet_forward_iqn": [_vp, _i, _vp, _i, _vp, _i, _vp, _vp],
    "fb_iqn_draw_taus": [_i, _i, _u64, _u64, _i, _vp, _vp],
    "fb_qnet_iqn_train_step": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _d, _vp, _vp, _vp, _vp],
    "fb_iqn_train_from_replay": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _d, _vp, _vp, _vp, _vp],
    "fb_iqn_step": [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64, _u64, _i, _d, _vp],
    "fb_qnet_iqn_per_train_step": [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _d, _vp, _vp, _vp, _vp, _vp],
    "fb_iqn_per_train_from_replay": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _u64, _u64, _d, _vp, _vp, _vp, _vp, _vp],
    "fb_iqn_per_step": [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64, _u64, _i, _d, _vp],
    "fb_qnet_destroy": [_vp],
    "fb_qnet_num_params": [_vp, _vp],
    "fb_qnet_init_params": [_vp, _i, _u64, _vp],
    "fb_qnet_load_params": [_vp, _i, _vp, _vp],
    "fb_qnet_store_params": [_vp, _i, _vp, _vp],
    "fb_qnet_get_adam_state": [_vp] * 4,
    "fb_qnet_set_adam_state": [_vp] * 4,
    "fb_qnet_set_hparams": [_vp, _f, _f, _f, _f],
    "fb_qnet_set_inference_dtype": [_vp, _i],
    "fb_qnet_overflow_count": [_vp, _i, _vp],
    "fb_qnet_split_stats": [_vp, _vp, _vp],
    "fb_vec_step_set_schedule": [_i],
    "fb_qnet_set_train_dtype": [_vp, _i],
    "fb_qnet_forward": [_vp, _i, _vp, _i, _vp, _vp],
    "fb_qnet_act": [_vp, _vp, _i, _f, _u64, _u64, _vp, _vp, _vp],
    "fb_qnet_act_nib": [_vp, _vp, _i, _f, _u64, _u64, _vp, _vp, _vp],
    "fb_qnet_train_step": [_vp, _i, _i] + [_vp] * 6 + [_d] + [_vp] * 5,
    "fb_qnet_apply_adam": [_vp, _vp, _vp],
    "fb_train_steps": [_vp, _vp, _i, _i, _i] + [_vp] * 7 + [_d, _vp],
    "fb_qnet_sync_target": [_vp, _vp],
    "fb_qnet_profile_kernel": [_vp, _i, _i, _i, _i] + [_vp] * 7,
    "fb_dist_probe": [C.c_char_p],
    "fb_dist_unique_id": [C.c_char_p, _vp],
    "fb_dist_create": [C.c_char_p, _i, _i, _vp],
    "fb_dist_destroy": [_vp],
    "fb_dist_set_overlap": [_vp, _i],
    "fb_vec_step_dp": [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64, _u64, _i, _d, _i, _vp],
    "fb_dist_reduce_apply": [_vp, _vp, _vp, _i, _vp],
    "fb_dist_grad_event": [_vp],
    "fb_dist_all_reduce": [_vp, _vp, _i64, _vp],
    "fb_qnet_set_grad_event": [_vp, _vp],
    "fb_qnet_grad_split": [_vp],
    "fb_train_from_replay": [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp],
    "fb_profile_ring_kernel": [_vp, _vp, _i, _i, _i, _i] + [_vp] * 6,
    "fb_qnet_kernel_name": [_i],
    "fb_vec_step": [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _u64, _u64, _i, _d, _vp],
    "fb_eval_create": [_i, _vp, _sz, _vp],
    "fb_eval_destroy": [_vp],
    "fb_eval_run": [_vp, _vp, _i, _i, _i64, _f, _u64, _u64, _vp, _vp, _vp, _vp, _vp],
    "fb_eval_stats": [_vp, _vp, _vp],
    "fb_eval_q": [_vp, _vp, _i, _vp, _vp],
}


class StepBuffers(C.Structure):
    """fb_step_buffers (include/fbdqn.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("nib", "actions", "frame_bits", "reward", "terminal", "score", "idx", "s", "s2", "a", "t",
                                           "r", "loss", "flat_grad", "isw", "isw32", "abs_err")]


class AcRolloutBuffers(C.Structure):
    """fb_ac_rollout_buffers (include/fbdqn.h)"""
    _fields_ = [(n, C.c_void_p) for n in ("nib", "actions", "frame_bits", "reward", "terminal", "score", "value", "logp")] + [("slots", C.c_int)]


_lib = None


class FbError(RuntimeError):
    pass


def lib():
    """Load libfbdqn.so; fail loudly when it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FbError(f"{LIB_PATH} is missing: build it with `make -C dqnflappybird_amd/csrc` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
        # PyTorch-ROCm bundles its own libamdhip64 (soname libamdhip64.so.7, same as /opt/rocm's).
        # Import torch FIRST so that the process has ONE HIP runtime and libfbdqn.so binds to it;
        # loading /opt/rocm's copy first leaves torch without devices ("No HIP GPUs are available").
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            fn = getattr(L, name)      # AttributeError = stale library: rebuild it
            fn.argtypes = args
            fn.restype = C.c_char_p if name in ("fb_last_error", "fb_qnet_kernel_name") else C.c_int64 if name == "fb_qnet_grad_split" else C.c_void_p if name in ("fb_dist_create", "fb_dist_grad_event") else None if name == "fb_dist_destroy" else C.c_int
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != FB_OK:
        msg = lib().fb_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(f"{what}: {msg}")
        raise FbError(f"{what} failed ({rc}): {msg}")


def require_gpu():
    n = lib().fb_device_count()
    if n <= 0:
        raise FbError("no HIP device visible: the MI355X path cannot run (there is no CPU fallback): "
                      + lib().fb_last_error().decode("utf-8", "replace"))
    return n


def sprite_blob():
    with open(ASSET_BLOB, "rb") as f:
        return f.read()


def ptr(t):
    """device/host pointer of a torch tensor / numpy array / None as c_void_p."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        return C.c_void_p(t.data_ptr())
    return t.ctypes.data_as(C.c_void_p)


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
