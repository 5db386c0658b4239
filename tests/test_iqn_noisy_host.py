"""Noisy IQN, the host side (include/fbdqn.h: fb_qnet_create_iqn_noisy): the layout of [mu | sigma] and of the noise vector, the float64
identity behind the per-env head -- the grid mean of theta under one env's effective weights is the folded mu logit plus the noise term
the header states -- the header block's key sentences, the command line's accepted and refused forms, and VecIQN's argument checks.
tests/test_gpu_iqn_noisy.py imports the helpers."""
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_iqn_dueling_host import as_iqn, iqnd_bounds
from tests.test_iqn_host import E, F32, head_parts, iqn_bounds, pre64, qbar_from_h, tau_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUNK = 77984                                # W_fc1's first entry: sigma covers the vector from here to W_e's first entry


def mu_bounds(fc, A, dueling):
    return {n: (lo, hi) for n, lo, hi in (iqnd_bounds if dueling else iqn_bounds)(fc, A)}


def n_mu(fc, A, dueling):
    return mu_bounds(fc, A, dueling)["b_e"][1]


def noisy_end(fc, A, dueling):
    """where sigma's range [TRUNK, .) ends: the first entry of W_e"""
    return mu_bounds(fc, A, dueling)["W_e"][0]


def n_total(fc, A, dueling):
    return n_mu(fc, A, dueling) + noisy_end(fc, A, dueling) - TRUNK


def layers(fc, A, dueling):
    """[(w, fan_in, fan_out, ein, eout)] of the noisy layers in flat order -- fc1, (the V layer,) the Q / advantage layer -- and nz"""
    b = mu_bounds(fc, A, dueling)
    shapes = [(TRUNK, 1600, fc)] + ([(b["W_v"][0], fc, 1), (b["W_a"][0], fc, A)] if dueling else [(b["W_q"][0], fc, A)])
    out, e = [], 0
    for w, fi, fo in shapes:
        out.append((w, fi, fo, e, e + fi))
        e += fi + fo
    return out, e


def factors(nz, fc, A, dueling, dtype=np.float64):
    """e(q) for q in [TRUNK, noisy_end): f(eps_out_j) f(eps_in_i) for a weight, f(eps_out_j) for a bias; dtype float32: the device's product"""
    nz = np.asarray(nz, dtype)
    parts = []
    for w, fi, fo, ein, eout in layers(fc, A, dueling)[0]:
        parts += [(nz[None, eout:eout + fo] * nz[ein:ein + fi, None]).ravel(), nz[eout:eout + fo]]
    e = np.concatenate(parts)
    assert e.size == noisy_end(fc, A, dueling) - TRUNK and e.dtype == dtype
    return e


def effective(P, nz, fc, A, dueling):
    """float64 torch: the effective parameters (the net's mu layout) of a master vector P = [mu | sigma], differentiable in P"""
    n, ne = n_mu(fc, A, dueling), noisy_end(fc, A, dueling)
    P = torch.as_tensor(P, dtype=torch.float64)
    assert P.numel() == n_total(fc, A, dueling)
    return torch.cat([P[:TRUNK], P[TRUNK:ne] + P[n:] * torch.as_tensor(factors(nz, fc, A, dueling)), P[ne:n]])


def as_plain(p_eff, fc, A, dueling):
    """the IQN-layout view (effective columns) the restatements of tests/test_iqn_host.py read"""
    return as_iqn(p_eff, fc, A) if dueling else p_eff


def rand_master(rng, fc, A, dueling, scale=0.05):
    return torch.tensor(rng.normal(size=n_total(fc, A, dueling)) * scale)


# ---------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("fc,A", [(128, 2), (384, 3), (128, 8)])
def test_layout_and_noise_size(fc, A):
    from dqnflappybird_amd import vec
    for du, arch, plain_arch in ((False, "iqnnoisy", "iqn"), (True, "iqnduelingnoisy", "iqndueling")):
        ls, nz = layers(fc, A, du)
        assert nz == vec.noise_size(fc, A, 0, arch) == (1600 + fc) + ((fc + 1) if du else 0) + (fc + A)
        assert [l[0] for l in ls] == sorted(l[0] for l in ls) and ls[0][:3] == (TRUNK, 1600, fc) and ls[-1][1:3] == (fc, A)
        for (w, fi, fo, _, _), nxt in zip(ls, ls[1:] + [(noisy_end(fc, A, du),)]):
            assert w + (fi + 1) * fo == nxt[0]                       # W[fin][fout], b[fout], then the next layer: consecutive up to W_e
        assert n_total(fc, A, du) == n_mu(fc, A, du) + sum((fi + 1) * fo for _, fi, fo, _, _ in ls)
        assert noisy_end(fc, A, du) == n_mu(fc, A, du) - (E + 1) * fc   # W_e b_e have no sigma
    assert vec.IQN_NOISY_ARCHS == ("iqnnoisy", "iqnduelingnoisy") and vec.IQN_ARCHS == ("iqn", "iqndueling")
    assert all(a in vec.QNet.ARCHS for a in vec.IQN_NOISY_ARCHS)
    # the C51 sizes are what they were
    assert vec.noise_size(512, 2, 51, "c51") == 1600 + 512 + 512 + 102 and vec.noise_size(512, 2, 51, "c51dueling") == 1600 + 512 + 512 + 51 + 512 + 102


def test_factors_and_effective():
    fc, A = 128, 3
    rng = np.random.default_rng(0)
    for du in (False, True):
        ls, nz = layers(fc, A, du)
        e = rng.normal(size=nz)
        P = rand_master(rng, fc, A, du)
        n, ne = n_mu(fc, A, du), noisy_end(fc, A, du)
        eff = effective(P, e, fc, A, du)
        assert eff.numel() == n and torch.equal(eff[:TRUNK], P[:TRUNK]) and torch.equal(eff[ne:], P[ne:n])
        w, fi, fo, ein, eout = ls[-1]
        i, j = 7, A - 1                                              # one weight and one bias of the last layer, spelled out
        q = w + i * fo + j
        assert abs(eff[q].item() - (P[q] + P[n + q - TRUNK] * e[ein + i] * e[eout + j]).item()) < 1e-15
        q = w + fi * fo + j
        assert abs(eff[q].item() - (P[q] + P[n + q - TRUNK] * e[eout + j]).item()) < 1e-15
        assert torch.equal(effective(P, np.zeros(nz), fc, A, du), P[:n])            # mean mode: mu
        f32 = factors(e.astype(F32), fc, A, du, F32)
        assert np.abs(f32 - factors(e.astype(F32), fc, A, du)).max() < 1e-5


# ---------------------------------------------------------------------------------------------------------------- the identity
def noise_terms(P, e, h, phibar, fc, A, dueling):
    """the header's noise term per column, float64: f(eo_a) (sum_k phibar_k sigma_W[k, a] f(ei_k) h_k + sigma_b[a]) of the Q / advantage
    layer and, dueling, the same over the V layer; -> [B, A]"""
    n = n_mu(fc, A, dueling)
    sig = lambda q0, cnt: P[n + q0 - TRUNK:n + q0 - TRUNK + cnt]
    out = []
    for w, fi, fo, ein, eout in layers(fc, A, dueling)[0][1:]:
        sW, sb = sig(w, fi * fo).view(fi, fo), sig(w + fi * fo, fo)
        ei, eo = torch.as_tensor(e[ein:ein + fi]), torch.as_tensor(e[eout:eout + fo])
        out.append(eo * ((h * phibar * ei) @ sW + sb))
    if not dueling:
        return out[0]
    nV, nA = out
    return nV + nA - nA.mean(1, keepdim=True)


@pytest.mark.parametrize("eta", [1.0, 0.25])
@pytest.mark.parametrize("K", [1, 32])
@pytest.mark.parametrize("dueling", [False, True])
def test_the_per_env_identity(dueling, K, eta):
    """the grid mean of theta under one env's effective weights == the folded mu logit + the noise term, in float64, as tightly as
    tests/test_iqn_host.py::test_the_fold_identity holds"""
    fc, A = 128, 3
    rng = np.random.default_rng(3 + K)
    P = rand_master(rng, fc, A, dueling)
    P[n_mu(fc, A, dueling):] = P[n_mu(fc, A, dueling):].abs()
    e = rng.normal(size=layers(fc, A, dueling)[1])
    h = torch.tensor(np.abs(rng.normal(size=(6, fc))))             # (env e's fc1 activations: its own noise is already in them)
    mu = as_plain(P[:n_mu(fc, A, dueling)], fc, A, dueling)
    eff = as_plain(effective(P, e, fc, A, dueling), fc, A, dueling)
    want = qbar_from_h(eff, h, K, eta, fc, A)                        # the mean over the acting grid of theta under the effective weights
    phi = F.relu(pre64(mu, tau_grid(K, eta), fc, A))                 # (W_e b_e are mu's: deterministic)
    if K > 1:
        assert (phi == 0).any() and (phi > 0).any()
    phibar = phi.mean(0)
    Wq, bq, _, _ = head_parts(mu, fc, A)
    folded = h @ (phibar[:, None] * Wq) + bq                         # the mu logit over the mu fold
    got = folded + noise_terms(P, e, h, phibar, fc, A, dueling)
    assert (got - folded).abs().max().item() > 1e-3                  # the noise term is far above the bound
    assert (got - want).abs().max().item() < 1e-14
    zero = torch.cat([P[:n_mu(fc, A, dueling)], torch.zeros(noisy_end(fc, A, dueling) - TRUNK, dtype=torch.float64)])
    assert noise_terms(zero, e, h, phibar, fc, A, dueling).abs().max().item() == 0      # sigma = 0: the mu logit alone


# ---------------------------------------------------------------------------------------------------------------- ABI and header
def test_header_and_binding_declare_the_noisy_iqn_abi():
    import ctypes as C
    from dqnflappybird_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "fbdqn.h")).read()
    assert ("int fb_qnet_create_iqn_noisy(int dueling, int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, float sigma0,\n"
            "                             int max_batch, fb_qnet_t *out);") in hdr
    assert L.SIGNATURES["fb_qnet_create_iqn_noisy"] == [C.c_int] * 6 + [C.c_float, C.c_float, C.c_int, C.c_void_p]
    block = hdr[hdr.index("noisy IQN (Fortunato et al. 2018"):hdr.index("int fb_qnet_create_iqn_noisy(")]
    for word in ("supersedes the \"not offered ... noisy IQN\" lines", "The conv trunk and the tau embedding W_e b_e stay deterministic",
                 "sits at n_mu + q - OFF_WF1", "fb_qnet_num_params = n_mu + (off.we - OFF_WF1)", "sigma = sigma0 / sqrt(fan_in) per layer",
                 "nz = (1600 + FC) + (FC + A); dueling:", "(1600 + FC) + (FC + 1) + (FC + A)", "(element, step_lo, 6, 2 step_hi + net)",
                 "A new net is in mean mode", "the IQN fold follows each rebuild", "g[n_mu + q - OFF_WF1] = g[q] e(q)",
                 "mu trains bit for bit as the non-noisy IQN net", "counter (e nz + k, step_lo, 7, step_hi)",
                 "h_k = relu((mu partials + b_k) + f(eo_k) (t_k + sigma_b_k))",
                 "Qbar_e(a) = [b_q[a] + sum_k phibar_k W_q^mu[k, a] h_k] + f(eo_a) (sum_k phibar_k sigma_W[k, a] f(ei_k) h_k + sigma_b[a])",
                 "nV + nA_a - (1/A) sum_c nA_c", "At sigma = 0 the call is mean-mode fb_qnet_act_nib", "The call reads no net's sample",
                 "fb_qnet_act_nib_env_noise(seed, step) -> env step -> store / sample -> fb_qnet_reset_noise(0) -> fb_qnet_reset_noise(1)",
                 "The tau draws (stream 10) are unchanged", "n nz >= 2^32"):
        assert word in block, word
    # the older blocks keep their lines (other host tests read them)
    assert hdr.count("not offered noisy IQN, bf16, data parallel, riders, the split schedule; Munchausen with double_q.") == 2
    assert "not offered prioritized replay, dueling or noisy IQN" in hdr
    common = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_common.h")).read()
    assert "struct IqnFoldNzArgs : IqnFoldArgs { float *pbar; };" in common and "int fb_qnet_env_noise_fc1(" in common
    iqn = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_iqn.hip")).read()
    qnet = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_qnet.hip")).read()
    assert "void iqn_env_noise_head_kernel(" in iqn and "iqn_env_noise_head_kernel" not in qnet          # the new kernels: fb_iqn.hip's code object


# ---------------------------------------------------------------------------------------------------------------- VecIQN's checks
def test_check_noisy_and_the_keywords():
    from dqnflappybird_amd import veciqn
    assert len(inspect.signature(veciqn.check_args).parameters) == 18          # the CLI and the tests call it positionally
    assert veciqn.check_noisy(False, 0.5, "shared") == (False, 0.5, "shared")
    assert veciqn.check_noisy(np.bool_(True), 0, "env") == (True, 0.0, "env")
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="noisy must be True or False"):
            veciqn.check_noisy(bad, 0.5, "shared")
        with pytest.raises(ValueError, match="noisy must be True or False"):
            veciqn.VecIQN(32, noisy=bad)
    for bad in (-0.1, float("nan"), float("inf"), "x"):
        for on in (True, False):
            with pytest.raises(ValueError, match="sigma0 must be finite and >= 0"):
                veciqn.check_noisy(on, bad, "shared")
        with pytest.raises(ValueError, match="sigma0 must be finite and >= 0"):     # ... before anything touches the GPU
            veciqn.VecIQN(32, noisy=True, sigma0=bad)
    for bad in ("per-env", "", None, 1):
        with pytest.raises(ValueError, match="acting_noise must be 'shared' or 'env'"):
            veciqn.VecIQN(32, noisy=True, acting_noise=bad)
    with pytest.raises(ValueError, match="acting_noise='env' needs a noisy net \\(noisy=True\\)"):
        veciqn.VecIQN(32, acting_noise="env")
    with pytest.raises(ValueError, match="batch 64 > n_envs 32"):              # the other checks come first
        veciqn.VecIQN(32, noisy=True, sigma0=-1.0, batch=64)
    sig = inspect.signature(veciqn.VecIQN.__init__).parameters
    assert list(sig)[-3:] == ["noisy", "sigma0", "acting_noise"]              # the new keywords come last
    assert [sig[k].default for k in ("noisy", "sigma0", "acting_noise")] == [False, 0.5, "shared"]
    assert veciqn.iqn_arch(False, False) == "iqn" and veciqn.iqn_arch(True, False) == "iqndueling"
    assert veciqn.iqn_arch(False, True) == "iqnnoisy" and veciqn.iqn_arch(True, True) == "iqnduelingnoisy"


def test_checkpoints_record_the_noisy_layers(tmp_path):
    from dqnflappybird_amd.veciqn import VecIQN
    base = dict(head=np.array(["iqn"]), online=np.zeros(3, np.float32), scalars=np.array([0, 7, 2, 1, 128, 0, 1, 1, 0, 1], np.int64),
                iqn=np.array([8, 8, 32, 1.0, 1.0]))
    noisy = lambda s0, an: dict(noisy=np.array([1], np.int64), sigma0=np.array([s0]), acting_noise=np.array([an]))
    files = {}
    for kind, kw in (("old", {}), ("noisy", noisy(0.5, "shared")), ("env", noisy(0.5, "env")), ("s1", noisy(1.0, "shared"))):
        files[kind] = str(tmp_path / f"{kind}.npz")
        np.savez(files[kind], **base, **kw)

    def mk(nz, s0=0.5, an="shared"):
        v = VecIQN.__new__(VecIQN)
        v.__dict__.update(prioritized=False, dueling=False, munchausen=False, n=2, batch=1, fc_width=128, n_step=1, seed=7, n_tau=8, n_tau_next=8,
                          n_tau_act=32, kappa=1.0, noisy=nz, sigma0=s0, acting_noise=an)
        return v
    with pytest.raises(ValueError, match="holds a noisy net, this VecIQN has a non-noisy net \\(noisy=False"):
        mk(False).load(files["noisy"])
    with pytest.raises(ValueError, match="holds a non-noisy net, this VecIQN has a noisy net \\(noisy=True"):      # a file without the keys: not noisy
        mk(True).load(files["old"])
    with pytest.raises(ValueError, match="was written with sigma0 = 1.0, this VecIQN has sigma0 = 0.5"):
        mk(True).load(files["s1"])
    with pytest.raises(ValueError, match="was written with acting_noise = 'env', this VecIQN has acting_noise = 'shared'"):
        mk(True).load(files["env"])
    with pytest.raises(ValueError, match="was written with acting_noise = 'shared', this VecIQN has acting_noise = 'env'"):
        mk(True, an="env").load(files["noisy"])


# ---------------------------------------------------------------------------------------------------------------- the command line
def cli(argv):
    from dqnflappybird_amd.FlappyBirdDQN import build_parser, iqn_kwargs
    parser = build_parser()
    return iqn_kwargs(parser.parse_args(argv), parser)


@pytest.mark.parametrize("argv,msg", [
    (["--model", "iqn", "--vec", "32", "--noisy"], "--noisy is not an option of --model iqn"),
    (["--model", "rainbowiqn", "--vec", "32", "--sigma0", "0.5", "--noisy"], "--noisy is not an option of --model rainbowiqn"),
    (["--model", "rainbow", "--vec", "32", "--sigma0", "0.5"], "--sigma0 needs an IQN model (iqn, iqnper, rainbowiqn), not --model rainbow"),
    (["--model", "ddqn", "--vec", "32", "--sigma0", "0.5"], "--sigma0 needs an IQN model (iqn, iqnper, rainbowiqn), not --model ddqn"),
    (["--model", "qrdqn", "--vec", "32", "--sigma0", "0.5"], "--sigma0 needs an IQN model"),
    (["--model", "sac", "--vec", "32", "--sigma0", "0.5"], "--sigma0 needs an IQN model"),
    (["--model", "a2c", "--vec", "32", "--sigma0", "0.5"], "--sigma0 needs an IQN model"),
    (["--model", "iqn", "--sigma0", "0.5"], "--model iqn needs --vec"),
    (["--model", "iqn", "--vec", "32", "--sigma0", "-1"], "--sigma0 must be finite and >= 0"),
    (["--model", "iqnper", "--vec", "32", "--sigma0", "nan"], "--sigma0 must be finite and >= 0"),
    (["--model", "iqn", "--vec", "32", "--acting-noise", "env"], "--acting-noise env needs --noisy"),
    (["--model", "rainbowiqn", "--vec", "32", "--sigma0", "0.5", "--acting-noise", "per-env"], "invalid choice"),
])
def test_cli_refusals(argv, msg, capsys):
    with pytest.raises(SystemExit) as ex:
        cli(argv)
    assert ex.value.code == 2 and msg in capsys.readouterr().err


def test_cli_passes_sigma0_to_the_loop():
    for model, per, dq in (("iqn", False, False), ("iqnper", True, False), ("rainbowiqn", True, True)):
        kw = cli(["--model", model, "--vec", "64", "--sigma0", "0.5"])
        assert kw["noisy"] is True and kw["sigma0"] == 0.5 and kw["acting_noise"] == "shared" and kw["prioritized"] is per and kw["double_q"] is dq
        kw = cli(["--model", model, "--vec", "64", "--sigma0", "0", "--acting-noise", "env"])
        assert kw["noisy"] is True and kw["sigma0"] == 0.0 and kw["acting_noise"] == "env"
        kw = cli(["--model", model, "--vec", "64"])
        assert not {"noisy", "sigma0", "acting_noise"} & set(kw)      # without the flag VecIQN's keywords are the ones of before
    kw = cli(["--model", "rainbowiqn", "--dueling", "--vec", "64", "--n-step", "3", "--sigma0", "0.5", "--acting-noise", "env"])      # full Rainbow-IQN
    assert (kw["noisy"], kw["dueling"], kw["prioritized"], kw["double_q"], kw["n_step"], kw["acting_noise"]) == (True, True, True, True, 3, "env")
    assert cli(["--model", "rainbow", "--vec", "64", "--noisy"]) is None          # the C51 models keep --noisy
