"""PPO's one-call epoch and its stabilisers (include/fbdqn.h: fb_ppo_epoch and its block) without a GPU: np_normalize_sel, the numpy
restatement of fb_ac_normalize_adv_sel that tests/test_gpu_ppo_epoch.py compares the kernel with bit for bit; the annealing schedule;
every refusal the Python layers make before anything touches the GPU; the header's text; the checkpoint key's defaults."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_ac_host import ROOT
from tests.test_ppo_host import _two_level_sum, np_normalize

NAN, INF = float("nan"), float("inf")


def np_normalize_sel(adv, sel, out):
    """fb_ac_normalize_adv_sel in numpy, operation for operation (float64, the header's order applied to j): out[sel[j]] receives the
    normalised adv[sel[j]], every other position of out stays -> out"""
    adv, sel = np.asarray(adv, np.float32).ravel(), np.asarray(sel, np.int64)
    x = adv[sel].astype(np.float64)
    n = np.float64(len(x))
    mean = _two_level_sum(x) / n
    d = x - mean
    sd = np.sqrt(_two_level_sum(d * d) / n)
    out[sel] = ((x - mean) / (sd + np.float64(1e-8))).astype(np.float32)
    return out


def shuffled_subset(n, seed):
    """(a float32 buffer of 2 n + 3 elements, n distinct positions of it in a shuffled order)"""
    rng = np.random.default_rng(seed)
    size = 2 * n + 3
    return (rng.normal(size=size) * 3 + 1.5).astype(np.float32), rng.permutation(size)[:n].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- the normaliser
@pytest.mark.parametrize("n", [2, 255, 256, 257, 1280])
def test_np_normalize_sel_against_plain_float64(n):
    """the two-level order is a float64 sum like any other: mean and sd within 1e-12 relative of numpy's pairwise ones (the values are
    O(1) with mean 1.5, so the sums carry no cancellation), and the normalised values with them"""
    adv, sel = shuffled_subset(n, n)
    x = adv[sel].astype(np.float64)
    mean = _two_level_sum(x) / n
    sd = np.sqrt(_two_level_sum((x - mean) ** 2) / n)
    assert abs(mean - x.mean()) <= 1e-12 * abs(x.mean()) and abs(sd - x.std()) <= 1e-12 * x.std()
    sentinel = np.float32(-77.0)
    out = np_normalize_sel(adv, sel, np.full(adv.shape, sentinel, np.float32))
    plain = (x - x.mean()) / (x.std() + 1e-8)
    np.testing.assert_allclose(out[sel].astype(np.float64), plain, rtol=1e-6, atol=1e-6)      # (float32 rounding of the result)
    g = ((x - mean) / (sd + 1e-8))
    np.testing.assert_allclose(g, plain, rtol=1e-12, atol=1e-12)
    rest = np.ones(len(adv), bool)
    rest[sel] = False
    assert rest.sum() == n + 3 and (out[rest] == sentinel).all() and out.dtype == np.float32


def test_np_normalize_sel_of_one_element_is_zero():
    adv, sel = shuffled_subset(1, 0)
    out = np_normalize_sel(adv, sel, np.full(adv.shape, np.float32(9.0)))
    assert out[sel[0]] == 0.0 and (np.delete(out, sel[0]) == 9.0).all()


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1300])
def test_identity_selection_is_the_rollout_normaliser(n):
    rng = np.random.default_rng(n)
    x = (rng.normal(size=n) * 3 + 1.5).astype(np.float32)
    got = np_normalize_sel(x, np.arange(n), np.zeros(n, np.float32))
    assert np.array_equal(got, np_normalize(x))


# ---------------------------------------------------------------------------------------------------------------- annealing
def test_annealing_schedule():
    from dqnflappybird_amd.vecac import annealed_lr
    lr, total = 2.5e-4, 7
    assert annealed_lr(lr, 0, total) == lr
    assert annealed_lr(lr, 1, total) == lr * (1.0 - 1.0 / 7.0)
    assert annealed_lr(lr, total - 1, total) == lr * (1.0 - 6.0 / 7.0) and 0.0 < annealed_lr(lr, total - 1, total) < lr / 6.9
    assert annealed_lr(lr, total, total) == 0.0 and annealed_lr(lr, total + 5, total) == 0.0
    assert annealed_lr(1e-3, 3, 4) == 1e-3 * 0.25 and annealed_lr(1e-3, 0, 1) == 1e-3 and annealed_lr(1e-3, 1, 1) == 0.0
    v = [annealed_lr(lr, u, total) for u in range(total + 1)]
    assert all(a > b for a, b in zip(v, v[1:])) and isinstance(v[1], float)


# ---------------------------------------------------------------------------------------------------------------- Python refusals
def test_check_ppo_options_values():
    from dqnflappybird_amd.vecac import PPO_OPTS_OFF, check_ppo_options
    assert check_ppo_options() == PPO_OPTS_OFF + (False,)
    assert check_ppo_options("rollout", None, False, None, None) == ("rollout", 0.0, False, 0, False)
    assert check_ppo_options(target_kl=0) == ("rollout", 0.0, False, 0, False)                      # 0 and None: off
    assert check_ppo_options(one_call=True) == ("rollout", 0.0, False, 0, True)
    assert check_ppo_options(one_call=False) == ("rollout", 0.0, False, 0, False)
    assert check_ppo_options("minibatch") == ("minibatch", 0.0, False, 0, True)
    assert check_ppo_options("minibatch", normalize_adv=False) == ("minibatch", 0.0, False, 0, False)      # not read: not on
    assert check_ppo_options(target_kl=0.02) == ("rollout", 0.02, False, 0, True)
    assert check_ppo_options(anneal_lr=True, total_updates=10) == ("rollout", 0.0, True, 10, True)
    assert check_ppo_options(total_updates=10) == ("rollout", 0.0, False, 10, False)
    assert check_ppo_options("minibatch", 0.02, True, 1, True) == ("minibatch", 0.02, True, 1, True)


@pytest.mark.parametrize("kw,msg", [
    (dict(adv_norm_scope="epoch"), "adv_norm_scope must be one of"),
    (dict(adv_norm_scope=None), "adv_norm_scope must be one of"),
    (dict(target_kl=-0.01), "target_kl must be finite and >= 0"),
    (dict(target_kl=NAN), "target_kl must be finite and >= 0"),
    (dict(target_kl=INF), "target_kl must be finite and >= 0"),
    (dict(anneal_lr=True), "anneal_lr needs total_updates >= 1"),
    (dict(anneal_lr=True, total_updates=0), "total_updates must be >= 1, got 0"),
    (dict(total_updates=-3), "total_updates must be >= 1, got -3"),
    (dict(target_kl=0.02, one_call=False), "target_kl need one_call=True"),
    (dict(adv_norm_scope="minibatch", one_call=False), "adv_norm_scope='minibatch' need one_call=True"),
    (dict(anneal_lr=True, total_updates=5, one_call=False), "anneal_lr need one_call=True"),
    (dict(adv_norm_scope="minibatch", target_kl=1.0, one_call=False), "adv_norm_scope='minibatch' / target_kl need one_call=True"),
])
def test_check_ppo_options_refusals(kw, msg):
    from dqnflappybird_amd.vecac import VecActorCritic, check_ppo_options
    with pytest.raises(ValueError, match=msg):
        check_ppo_options(**kw)
    with pytest.raises(ValueError, match=msg):                   # ... and the constructor, before anything touches the GPU
        VecActorCritic(16, algo="ppo", **kw)


def test_check_ppo_args_keeps_its_signature():
    import inspect
    from dqnflappybird_amd.vecac import check_ppo_args
    assert list(inspect.signature(check_ppo_args).parameters) == ["n_envs", "rollout", "epochs", "minibatches", "clip_eps", "value_clip"]


@pytest.mark.parametrize("argv,msg", [
    (["--model", "ppo", "--vec", "16", "--adv-norm-scope", "epoch"], "adv_norm_scope must be one of"),
    (["--model", "ppo", "--vec", "16", "--target-kl", "-1"], "target_kl must be finite and >= 0"),
    (["--model", "ppo", "--vec", "16", "--target-kl", "nan"], "target_kl must be finite and >= 0"),
    (["--model", "ppo", "--vec", "16", "--anneal-lr", "--steps", "-2"], "total_updates must be >= 1, got -2"),
    (["--model", "a2c", "--vec", "16", "--target-kl", "0.02"], "--target-kl need --model ppo, not --model a2c"),
    (["--model", "a2c", "--vec", "16", "--anneal-lr"], "--anneal-lr need --model ppo, not --model a2c"),
    (["--model", "dqn", "--vec", "16", "--adv-norm-scope", "minibatch"], "--adv-norm-scope need --model ppo, not --model dqn"),
    (["--model", "sac", "--vec", "16", "--target-kl", "0.02", "--anneal-lr"], "--target-kl / --anneal-lr need --model ppo, not --model sac"),
    (["--model", "iqn", "--vec", "16", "--adv-norm-scope", "minibatch", "--anneal-lr"], "--adv-norm-scope / --anneal-lr need --model ppo, not --model iqn"),
    (["--model", "ppo", "--target-kl", "0.02"], "--model ppo needs --vec"),
])
def test_cli_refusals(argv, msg):
    out = subprocess.run([sys.executable, "-m", "dqnflappybird_amd.FlappyBirdDQN"] + argv, cwd=ROOT, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 2
    assert msg in out.stderr


# ---------------------------------------------------------------------------------------------------------------- ABI
OLD_PPO_NOT_OFFERED = " *   not offered data-parallel PPO, bf16, per-minibatch advantage normalisation, KL early stopping, annealing, recurrent policies. */\n"


def test_header_and_binding_declare_the_epoch_abi():
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    for decl in ("int fb_ac_normalize_adv_sel(const float *adv, const int64_t *sel, int64_t n, float *out, void *stream);",
                 "int fb_ac_grad_accumulate(float *acc, const float *chunk, int64_t n, int first, void *stream);",
                 "int fb_ppo_epoch(fb_replay_t replay, fb_qnet_t net, int64_t n, int minibatches, const int64_t *pos, const int64_t *sel, const float *adv,",
                 "float *loss_rows /*f32[minibatches][6]*/, float *epoch_mean /*f32[6]*/, void *stream);",
                 "int fb_ppo_epoch_sum(fb_qnet_t net, float *sum /*[dev] f32[6]*/, void *stream);", "in ascending order over ALL chunks of the epoch",
                 "out[sel[j]] = (float)(((double)adv[sel[j]] - mean) / (sd + 1e-8))", "out == adv is refused",
                 "acc[i] = (first ? 0.f : acc[i]) + chunk[i]", "epoch_mean[c] = (sum_m loss_rows[m][c], ascending m from 0.f) / (float)minibatches",
                 "no host synchronisation, no host read", "Data-parallel PPO, bf16 and recurrent policies stay not"):
        assert decl in hdr, decl
    # PPO's own block stands word for word, in front of the new one
    assert OLD_PPO_NOT_OFFERED in hdr and hdr.index(OLD_PPO_NOT_OFFERED) < hdr.index("PPO: one epoch as one host call")
    old = hdr[hdr.index("/* ------------------------------------------------------------------ PPO (Schulman et al. 2017)"):hdr.index("PPO: one epoch as one host call")]
    for text in ("normalise   fb_ac_normalize_adv, per rollout, in double", "out may be adv.  1 <= n < 2^31",
                 "int fb_ac_normalize_adv(const float *adv, int64_t n, float *out, void *stream);",
                 "int fb_ac_permute(int64_t n, uint64_t seed, uint64_t draw, int64_t *out, void *stream);"):
        assert text in old, text
    i, i64, vp = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert L.SIGNATURES["fb_ac_normalize_adv_sel"] == [vp, vp, i64, vp, vp]
    assert L.SIGNATURES["fb_ac_grad_accumulate"] == [vp, vp, i64, i, vp]
    assert L.SIGNATURES["fb_ppo_epoch"] == [vp, vp, i64, i, vp, vp, vp, vp, vp, vp, i, vp, vp, vp, vp, vp, vp, vp]
    assert L.SIGNATURES["fb_ppo_epoch_sum"] == [vp, vp, vp]
    lib = L.lib()                                                # (binds every symbol: a stale library raises here)
    err = lambda: lib.fb_last_error().decode()
    assert lib.fb_ppo_epoch_sum(None, None, None) == -1 and "fb_ppo_epoch_sum: NULL" in err()
    assert lib.fb_ac_normalize_adv_sel(None, None, 4, None, None) == -1 and "fb_ac_normalize_adv_sel: NULL" in err()
    assert lib.fb_ac_grad_accumulate(None, None, 4, 1, None) == -1 and "fb_ac_grad_accumulate: NULL" in err()
    assert lib.fb_ppo_epoch(*([None, None, 4, 1] + [None] * 6 + [0] + [None] * 7)) == -1 and "fb_ppo_epoch: NULL" in err()


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def bare_ppo(**kw):
    """VecActorCritic.__new__ with what load reads up to the options' refusal"""
    from dqnflappybird_amd.vecac import PPO_OPTS_OFF, VecActorCritic
    v = VecActorCritic.__new__(VecActorCritic)
    v.algo, v.n, v.T, v.fc_width, v.seed = "ppo", 16, 4, 512, 0
    v.adv_norm_scope, v.target_kl, v.anneal_lr, v.total_updates = PPO_OPTS_OFF
    for k, x in kw.items():
        setattr(v, k, x)
    return v


def test_checkpoint_key_defaults_and_mismatches(tmp_path):
    from dqnflappybird_amd.vecac import ADV_NORM_SCOPES, PPO_OPTS_OFF
    assert PPO_OPTS_OFF == ("rollout", 0.0, False, 0) and ADV_NORM_SCOPES == ("rollout", "minibatch")
    old, new = str(tmp_path / "old.npz"), str(tmp_path / "new.npz")
    base = dict(head=np.array(["ac"]), ppo=np.array([4, 4, 0.2, 0.0, 1.0]), scalars=np.array([0, 0, 1, 0, 16, 4, 512], np.int64))
    np.savez(old, **base)                                        # a file of before: no `ppo_opts`
    np.savez(new, ppo_opts=np.array([1.0, 0.02, 1.0, 500.0]), **base)
    # an old file into an object with an option on: refused by the option's name, against the all-off defaults
    for kw, msg in ((dict(adv_norm_scope="minibatch"), "was written with adv_norm_scope = 'rollout', this VecActorCritic has adv_norm_scope = 'minibatch'"),
                    (dict(target_kl=0.02), "was written with target_kl = 0.0, this VecActorCritic has target_kl = 0.02"),
                    (dict(anneal_lr=True, total_updates=9), "was written with anneal_lr = False, this VecActorCritic has anneal_lr = True"),
                    (dict(total_updates=9), "was written with total_updates = 0, this VecActorCritic has total_updates = 9")):
        with pytest.raises(ValueError, match=msg):
            bare_ppo(**kw).load(old)
    # a new file into objects that differ in one option each
    on = dict(adv_norm_scope="minibatch", target_kl=0.02, anneal_lr=True, total_updates=500)
    for kw, msg in ((dict(adv_norm_scope="rollout"), "adv_norm_scope = 'minibatch', this VecActorCritic has adv_norm_scope = 'rollout'"),
                    (dict(target_kl=0.0), "target_kl = 0.02, this VecActorCritic has target_kl = 0.0"),
                    (dict(anneal_lr=False), "anneal_lr = True, this VecActorCritic has anneal_lr = False"),
                    (dict(total_updates=400), "total_updates = 500, this VecActorCritic has total_updates = 400")):
        with pytest.raises(ValueError, match=msg):
            bare_ppo(**{**on, **kw}).load(new)
    # the file's normalize_adv replaces the object's: per-minibatch normalisation cannot arrive in an object on the chunk-by-chunk path
    with pytest.raises(ValueError, match="normalises its advantages per minibatch, which needs one_call=True"):
        bare_ppo(**on, normalize_adv=False, one_call=False).load(new)
    # matching options pass the check: load goes on to restore the net, which a bare object has none of
    with pytest.raises(AttributeError, match="net"):
        bare_ppo().load(old)
    with pytest.raises(AttributeError, match="net"):
        bare_ppo(**on, normalize_adv=True, one_call=True).load(new)
