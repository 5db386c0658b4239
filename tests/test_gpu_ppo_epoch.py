"""PPO's one-call epoch on the GPU (include/fbdqn.h: fb_ppo_epoch and its block; kernels: csrc/fb_ac.hip).  Everything here is bit for
bit: fb_ac_normalize_adv_sel against the numpy restatement of tests/test_ppo_epoch_host.py, fb_ac_grad_accumulate against torch's own
zero_() and +=, fb_ppo_epoch against the calls it composes (vec.ppo_train_from_replay, QNet.clip_grad, QNet.apply_adam, torch adds --
never against itself), and VecActorCritic's new options against loops written out in the test from those calls."""
import numpy as np
import pytest

from tests.test_gpu_ac import loop_state, net_state, same_loop, same_state
from tests.test_ppo_epoch_host import np_normalize_sel, shuffled_subset

pytestmark = pytest.mark.gpu
FC = 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    from dqnflappybird_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return torch


def bits(t):
    """a float32 tensor's bit patterns (so that NaN equals NaN and -0 differs from +0)"""
    import torch
    return t.contiguous().view(torch.int32)


# ================================================================================================================ fb_ac_normalize_adv_sel
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1280])
def test_normalize_adv_sel_is_the_restatement(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_normalize_adv_sel
    adv, sel = shuffled_subset(n, 100 + n)
    sentinel = np.float32(-77.0)
    want = np_normalize_sel(adv, sel, np.full(adv.shape, sentinel, np.float32))
    out = torch.full((len(adv),), float(sentinel), dtype=torch.float32, device="cuda")
    d_adv = torch.from_numpy(adv).cuda()
    got = ac_normalize_adv_sel(d_adv, torch.from_numpy(sel).cuda(), out)
    assert got is out and np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    rest = np.ones(len(adv), bool)
    rest[sel] = False
    assert rest.sum() == n + 3 and (out.cpu().numpy()[rest] == sentinel).all()      # unselected positions keep the sentinel
    assert np.array_equal(d_adv.cpu().numpy(), adv)                                  # adv is read only


@pytest.mark.parametrize("n", [1, 257, 1280])
def test_normalize_adv_sel_identity_is_normalize_adv(torch_cuda, n):
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_normalize_adv, ac_normalize_adv_sel
    adv = torch.from_numpy(shuffled_subset(n, n)[0][:n].copy()).cuda()
    whole = ac_normalize_adv(adv)
    out = ac_normalize_adv_sel(adv, torch.arange(n, dtype=torch.int64, device="cuda"), torch.zeros_like(adv))
    assert torch.equal(bits(out), bits(whole))


def test_normalize_adv_sel_refusals(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import ac_normalize_adv_sel
    adv = torch.randn(40, device="cuda")
    keep = adv.clone()
    sel = torch.arange(8, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="out must not be adv"):
        ac_normalize_adv_sel(adv, sel, adv)
    with pytest.raises(ValueError, match="sel must lie in 0..39"):
        ac_normalize_adv_sel(adv, sel + 33, torch.zeros_like(adv))
    with pytest.raises(ValueError, match=r"out must be a contiguous float32\[40\]"):
        ac_normalize_adv_sel(adv, sel, torch.zeros(39, device="cuda"))
    lib, out = L.lib(), torch.zeros_like(adv)
    assert lib.fb_ac_normalize_adv_sel(L.ptr(adv), L.ptr(sel), 0, L.ptr(out), None) == -1 and "out of range" in lib.fb_last_error().decode()
    assert lib.fb_ac_normalize_adv_sel(L.ptr(adv), L.ptr(sel), 1 << 31, L.ptr(out), None) == -1
    assert lib.fb_ac_normalize_adv_sel(L.ptr(adv), None, 8, L.ptr(out), None) == -1 and "NULL argument" in lib.fb_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(adv, keep) and not out.any()


# ================================================================================================================ fb_ac_grad_accumulate
def n_params():
    from dqnflappybird_amd.vec import QNet
    return QNet(2, FC, "ac", max_batch=256).n_params


@pytest.mark.parametrize("n", [1, 255, 257, "params"])
@pytest.mark.parametrize("offset", [0, 1])
def test_grad_accumulate_is_zero_and_add(torch_cuda, n, offset):
    """first = 1 over a stale accumulator, then two more chunks: torch's zero_() and += bit for bit.  The first chunk holds a -0 (which
    becomes +0), a NaN and an Inf; the stale accumulator holds NaNs that must not come through.  offset 1: buffers 4 bytes off a
    16-byte boundary (the kernel's one-element form); 255 and 257 leave a tail of 3 and of 1 behind the float4 part"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_grad_accumulate
    n = n_params() if n == "params" else n
    g = torch.Generator(device="cpu").manual_seed(n + offset)
    chunks = [(torch.randn(n + offset, generator=g) * 10.0 ** float(k - 1)).cuda()[offset:] for k in range(3)]
    special = [-0.0, float("nan"), float("inf"), float("-inf")][:min(4, n)]
    for k, v in enumerate(special):
        chunks[0][(k * 97) % n if n > 4 else k] = v
    assert all(c.data_ptr() % 16 == 4 * offset for c in chunks)
    stale = torch.full((n + offset,), float("nan"), device="cuda")[offset:]
    stale[n // 2:] = 3.5
    want = stale.clone()
    want.zero_()
    acc = stale.clone() if offset == 0 else torch.cat([torch.zeros(offset, device="cuda"), stale])[offset:]
    assert acc.data_ptr() % 16 == 4 * offset
    keep = [c.clone() for c in chunks]
    for k, c in enumerate(chunks):
        want += c
        assert ac_grad_accumulate(acc, c, first=k == 0) is acc
        assert torch.equal(bits(acc), bits(want)), (n, offset, k)
        if k == 0:                                                # position 0 held the -0: 0.f + -0 = +0; the stale NaNs are gone
            got = acc.cpu().numpy()
            assert got[0] == 0.0 and not np.signbit(got[0]) and np.isnan(got).sum() == (1 if n > 4 else 0)
            assert n <= 4 or (np.isinf(got).sum() == 2 and np.isnan(got[97]))
    for c, c0 in zip(chunks, keep):
        assert torch.equal(bits(c), bits(c0))                     # the chunks are read only


def test_grad_accumulate_minus_zero_and_refusals(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import ac_grad_accumulate
    c = torch.tensor([-0.0, -0.0, 1.0, -0.0, -0.0], device="cuda")
    acc = torch.full((5,), -1.0, device="cuda")
    ac_grad_accumulate(acc, c, first=True)
    assert not np.signbit(acc.cpu().numpy()).any() and acc.tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    ac_grad_accumulate(acc, c, first=False)
    assert acc.tolist() == [0.0, 0.0, 2.0, 0.0, 0.0] and not np.signbit(acc.cpu().numpy()).any()      # (+0) + (-0) = +0
    with pytest.raises(ValueError, match="one length"):
        ac_grad_accumulate(acc, c[:4], first=True)
    lib = L.lib()
    assert lib.fb_ac_grad_accumulate(L.ptr(acc), L.ptr(acc), 5, 1, None) == -1 and "acc must not be chunk" in lib.fb_last_error().decode()
    assert lib.fb_ac_grad_accumulate(L.ptr(acc), L.ptr(c), 0, 1, None) == -1 and lib.fb_ac_grad_accumulate(L.ptr(acc), None, 5, 1, None) == -1
    torch.cuda.synchronize()
    assert acc.tolist() == [0.0, 0.0, 2.0, 0.0, 0.0]


# ================================================================================================================ fb_ppo_epoch
def make_loop(n_envs, T, epochs=2, minibatches=1, **kw):
    from dqnflappybird_amd.vecac import VecActorCritic
    return VecActorCritic(n_envs, rollout=T, algo="ppo", epochs=epochs, minibatches=minibatches, seed=4, **{**dict(fc_width=FC), **kw})


def rollout_of(ac):
    """a fresh rollout of the loop -> (idx0, adv, ret, logp, value), the buffers flattened [T N]"""
    adv, ret = ac.collect()
    return ac._indices()[:1], adv, ret, ac.roll.logp.view(-1), ac.roll.value[:ac.T].view(-1)


def composed_epoch(torch, ac, perm, pos, adv, ret, logp, value, mb_norm, scratch):
    """one epoch from the existing calls and torch adds, as VecActorCritic._ppo_epochs composes it; per-minibatch normalisation is
    fb_ac_normalize_adv on the minibatch's gathered advantages (element j of its sums is the minibatch's element j), scattered back
    -> (loss_rows [M, 6], epoch_mean [6], the last chunk's actions, the running sum over all chunks [6])"""
    from dqnflappybird_amd.vec import ac_normalize_adv, ppo_train_from_replay
    tn, M = perm.numel(), ac.minibatches
    mb = tn // M
    rows = torch.zeros((M, 6), dtype=torch.float32, device="cuda")
    run = torch.zeros(6, dtype=torch.float32, device="cuda")
    a = None
    for m, lo in enumerate(range(0, tn, mb)):
        src = adv
        if mb_norm:
            sel = perm[lo:lo + mb]
            scratch[sel] = ac_normalize_adv(adv[sel].contiguous())
            src = scratch
        ac.grad.zero_()
        for k in range(lo, lo + mb, 256):
            hi = min(k + 256, lo + mb)
            loss, a = ppo_train_from_replay(ac.replay, ac.net, pos[k:hi], src, ret, logp, value, sel=perm[k:hi], n_total=mb,
                                            flat_grad=ac.chunk_grad, check_sel=False)
            ac.grad += ac.chunk_grad
            rows[m] += loss
            run += loss
        if ac.max_grad_norm:
            ac.net.clip_grad(ac.grad)
        ac.net.apply_adam(ac.grad)
    mean = torch.zeros(6, dtype=torch.float32, device="cuda")
    for m in range(M):
        mean += rows[m]
    return rows, mean / torch.tensor(float(M), dtype=torch.float32, device="cuda"), a, run


EPOCH_CASES = [(16, 3, 4, {}), (64, 4, 1, {}), (52, 5, 1, {}), (128, 5, 2, {}), (128, 5, 2, dict(max_grad_norm=0.5)), (52, 5, 1, dict(fc_width=512))]


@pytest.mark.parametrize("mb_norm", [0, 1])
@pytest.mark.parametrize("n_envs,T,M,kw", EPOCH_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_ppo_epoch_is_the_composed_calls(torch_cuda, n_envs, T, M, kw, mb_norm):
    """two epochs in a row on two equal loops, one through fb_ppo_epoch, one composed: parameters, Adam's m, v and beta powers, the
    summed gradient, loss_rows, epoch_mean and a_out after each.  mb = T N / M is 12 (one short chunk), 256 (one full chunk),
    260 (256 + 4) and 320 (256 + 64)"""
    torch = torch_cuda
    from dqnflappybird_amd.vec import ac_permute, ppo_epoch, ppo_epoch_sum
    one, ref = make_loop(n_envs, T, minibatches=M, lr=1e-3, **kw), make_loop(n_envs, T, minibatches=M, lr=1e-3, **kw)
    tn = n_envs * T
    ro, rr = rollout_of(one), rollout_of(ref)
    assert all(torch.equal(x, y) for x, y in zip(ro, rr))
    rows = torch.full((M, 6), 7.0, dtype=torch.float32, device="cuda")                 # (stale: the first chunk of a row starts from 0)
    mean, a_out = torch.full((6,), 7.0, dtype=torch.float32, device="cuda"), torch.zeros(256, dtype=torch.uint8, device="cuda")
    scratch = [torch.full((tn,), -5.0, dtype=torch.float32, device="cuda") for _ in range(2)]
    start = net_state(one.net)
    run = ppo_epoch_sum(one.net, torch.full((6,), 7.0, dtype=torch.float32, device="cuda"))
    assert not run.any()                                                               # zeros before the first epoch
    for e in range(2):
        perm = ac_permute(tn, 4, e)
        pos = perm + ro[0]
        got = ppo_epoch(one.replay, one.net, pos, perm, *ro[1:], M, one.grad, one.chunk_grad, rows, mean, a_out=a_out,
                        adv_scratch=scratch[0] if mb_norm else None, check_sel=False)
        assert got[0] is mean and got[1] is a_out
        w_rows, w_mean, w_a, w_run = composed_epoch(torch, ref, perm, pos, *rr[1:], mb_norm, scratch[1])
        assert torch.equal(bits(ppo_epoch_sum(one.net, run)), bits(w_run)), e           # one accumulator over all chunks
        print(f"epoch {e}: mean {mean.tolist()} / {w_mean.tolist()}")
        assert torch.equal(bits(rows), bits(w_rows)) and torch.equal(bits(mean), bits(w_mean)), e
        assert torch.equal(a_out[:w_a.numel()], w_a) and torch.equal(bits(one.grad), bits(ref.grad)), e
        assert same_state(torch, net_state(one.net), net_state(ref.net)), e
        if mb_norm:
            assert torch.equal(bits(scratch[0]), bits(scratch[1])) and not (scratch[0] == -5.0).any()
    assert torch.isfinite(mean).all() and not same_state(torch, net_state(one.net), start)
    assert all(torch.equal(x, y) for x, y in zip(ro[1:], rr[1:]))                      # the rollout buffers are read only
    if kw.get("max_grad_norm"):
        assert one.net.grad_norm() == ref.net.grad_norm() and 0.0 < one.net.grad_norm()[1] <= 1.0
    assert one.net.overflow_count() == 0


def test_ppo_epoch_refusals_leave_everything_as_it_was(torch_cuda):
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    from dqnflappybird_amd.vec import QNet, VecReplay, ppo_epoch, ppo_epoch_sum
    lib = L.lib()
    ac = make_loop(16, 3, minibatches=4)
    idx0, adv, ret, logp, value = rollout_of(ac)
    tn = 48
    perm = torch.randperm(tn, device="cuda")
    pos = perm + idx0
    rows, mean = torch.full((4, 6), 7.0, device="cuda"), torch.full((6,), 7.0, device="cuda")
    a_out, scratch = torch.zeros(256, dtype=torch.uint8, device="cuda"), torch.zeros(tn, device="cuda")
    blob, before = np.asarray(ac.replay.state_blob()).copy(), net_state(ac.net)
    err = lambda: lib.fb_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return (np.array_equal(np.asarray(ac.replay.state_blob()), blob) and same_state(torch, net_state(ac.net), before)
                and bool((rows == 7.0).all()) and bool((mean == 7.0).all()) and not scratch.any() and not ac.grad.any())

    def call(replay=ac.replay.h, net=ac.net.h, n=tn, M=4, norm=0, **ptrs):
        t = dict(pos=pos, sel=perm, adv=adv, ret=ret, logp=logp, value=value, scratch=None, grad=ac.grad, chunk=ac.chunk_grad, a=a_out, rows=rows,
                 mean=mean)
        t.update(ptrs)
        p = {k: L.ptr(v) for k, v in t.items()}
        return lib.fb_ppo_epoch(replay, net, n, M, p["pos"], p["sel"], p["adv"], p["ret"], p["logp"], p["value"], norm, p["scratch"], p["grad"],
                                p["chunk"], p["a"], p["rows"], p["mean"], None)

    for name in ("pos", "sel", "adv", "ret", "logp", "value", "grad", "chunk", "a", "rows", "mean"):
        assert call(**{name: None}) == -1 and "fb_ppo_epoch: NULL argument" in err(), name
    assert call(replay=None) == -1 and call(net=None) == -1
    for M in (0, -1, 5, 7):
        assert call(M=M) == -1 and "minibatches must be >= 1 and divide n = 48" in err(), M
    assert call(n=0, M=1) == -1 and "out of range" in err()
    assert call(norm=1) == -1 and "mb_adv_norm needs adv_scratch" in err()
    assert call(norm=1, scratch=adv) == -1 and "adv_scratch must not be adv" in err()
    assert call(chunk=ac.grad) == -1 and "grad must not be chunk_grad" in err()
    with pytest.raises(ValueError, match="adv_scratch must not be adv"):
        ppo_epoch(ac.replay, ac.net, pos, perm, adv, ret, logp, value, 4, ac.grad, ac.chunk_grad, rows, mean, adv_scratch=adv, check_sel=False)
    with pytest.raises(ValueError, match="minibatches must be >= 1 and divide the epoch's 48"):
        ppo_epoch(ac.replay, ac.net, pos, perm, adv, ret, logp, value, 5, ac.grad, ac.chunk_grad, rows, mean, check_sel=False)
    with pytest.raises(ValueError, match="sel must lie in 0..47"):
        ppo_epoch(ac.replay, ac.net, pos, perm + 1, adv, ret, logp, value, 4, ac.grad, ac.chunk_grad, rows, mean)
    with pytest.raises(ValueError, match=r"loss_rows must be float32\[4, 6\]"):
        ppo_epoch(ac.replay, ac.net, pos, perm, adv, ret, logp, value, 4, ac.grad, ac.chunk_grad, rows[:3], mean, check_sel=False)
    assert untouched()
    # what fb_ppo_train_from_replay refuses: an n-step view, a prioritized memory, a net that is not an actor-critic net, a chunk above max_batch
    ac.replay.set_n_step(3, 0.99)
    assert call() == -1 and "3-step view" in err()
    ac.replay.set_n_step(1, 0.99)
    per = VecReplay(2000, 16, prioritized=True)
    assert call(replay=per.h) == -1 and "uniform memory only" in err()
    with pytest.raises(ValueError, match="uniform memory only"):
        ppo_epoch(per, ac.net, pos, perm, adv, ret, logp, value, 4, ac.grad, ac.chunk_grad, rows, mean, check_sel=False)
    for arch in ("plain", "dueling"):
        q = QNet(2, FC, arch, max_batch=32)
        q.init_params(1)
        qb = net_state(q)
        assert call(net=q.h) == -1 and "not an actor-critic net (fb_qnet_create_ac)" in err(), arch
        with pytest.raises(ValueError, match="needs an actor-critic net"):
            ppo_epoch(ac.replay, q, pos, perm, adv, ret, logp, value, 4, ac.grad, ac.chunk_grad, rows, mean, check_sel=False)
        assert lib.fb_ppo_epoch_sum(q.h, L.ptr(mean), None) == -1 and "not an actor-critic net" in err()
        with pytest.raises(ValueError, match="needs an actor-critic net"):
            ppo_epoch_sum(q, mean)
        assert same_state(torch, net_state(q), qb)
    assert lib.fb_ppo_epoch_sum(ac.net.h, None, None) == -1 and lib.fb_ppo_epoch_sum(None, L.ptr(mean), None) == -1 and "NULL argument" in err()
    assert not ppo_epoch_sum(ac.net, torch.ones(6, device="cuda")).any()                # no refused call moved the running sum
    small = QNet(2, FC, "ac", max_batch=8)                       # (the same parameter count: ac.grad fits)
    small.init_params(1)
    sb = net_state(small)
    assert call(net=small.h) == -1 and "exceeds min(max_batch, 256)" in err()
    assert same_state(torch, net_state(small), sb) and untouched()
    # ... and after all of that the call still runs
    assert call() == 0
    torch.cuda.synchronize()
    assert not same_state(torch, net_state(ac.net), before) and torch.isfinite(mean).all() and not (rows == 7.0).any()


# ================================================================================================================ VecActorCritic
_off = {}


def off_pair(torch):
    """3 updates at (128 envs, T 5, 2 epochs, 2 minibatches: mb 320, chunks 256 + 64), one_call False and True from one seed, run once
    -> (the two loops, their returned losses)"""
    if not _off:
        a, b = make_loop(128, 5, minibatches=2, one_call=False), make_loop(128, 5, minibatches=2, one_call=True)
        _off["v"] = (a, b, [a.update().clone() for _ in range(3)], [b.update().clone() for _ in range(3)])
    return _off["v"]


def test_one_call_with_every_option_off_keeps_the_composed_state(torch_cuda):
    """parameters, Adam's m, v and beta powers (and the envs, the memory, the counters) bit for bit"""
    torch = torch_cuda
    a, b, _, _ = off_pair(torch)
    assert (a.one_call, b.one_call, make_loop(16, 3).one_call) == (False, True, False)
    assert same_loop(torch, loop_state(a), loop_state(b))
    assert b.epochs_run == 2 and a.updates == b.updates == 3


def test_one_call_with_every_option_off_returns_the_composed_losses(torch_cuda):
    """the returned six numbers bit for bit, at mb = 320: two chunks per minibatch, where the order of the additions shows.  The
    chunk-by-chunk loop adds the last epoch's chunks c_mk into ONE running sum, ((c00 + c01) + c10) + c11, and divides by M; the
    one-call loop returns fb_ppo_epoch_sum, the same running sum kept on the device, over M -- not epoch_mean, whose pinned order is rows
    first, (c00 + c01) + (c10 + c11), and which differs from it by up to 16 units of the last place here"""
    torch = torch_cuda
    _, b, la, lb = off_pair(torch)
    for u, (x, y) in enumerate(zip(la, lb)):
        print(f"update {u}: composed {x.tolist()}\n          one call {y.tolist()}  ulp differences {(bits(x) - bits(y)).tolist()}")
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(la, lb))
    print(f"epoch_mean {b.epoch_mean.tolist()}")
    torch.testing.assert_close(b.epoch_mean, lb[2], rtol=1e-5, atol=1e-8)      # (the other order of the same additions)


def kl_reference(torch, ref, target_kl):
    """one update of `ref` (a one_call=False loop) written out from the existing calls, with the early-stopping rule applied to the
    same device number -> (epochs run, the last epoch's mean)"""
    from dqnflappybird_amd.vec import ac_normalize_adv, ac_permute
    idx0, adv, ret, logp, value = rollout_of(ref)
    ac_normalize_adv(adv, out=adv)
    tn, ran, mean = ref.T * ref.n, 0, None
    for e in range(ref.epochs):
        perm = ac_permute(tn, ref.seed, ref.updates * ref.epochs + e)
        _, mean, _, _ = composed_epoch(torch, ref, perm, perm + idx0, adv, ret, logp, value, 0, None)
        ran = e + 1
        if e < ref.epochs - 1 and mean[5].item() > 1.5 * target_kl:
            break
    ref.updates += 1
    return ran, mean


@pytest.mark.parametrize("target_kl,epochs_run", [(1e9, 4), (1e-9, 1)])
def test_early_stopping_is_the_reference_loop(torch_cuda, capsys, target_kl, epochs_run):
    """lr 1e-3, 4 epochs x 4 minibatches, 64 envs x T 4, two updates: an Adam step at that lr moves the policy by far more than 1.5e-9 in
    KL, so the tight target stops after one epoch -- which the reference loop, reading the same device number, must say too"""
    torch = torch_cuda
    kw = dict(epochs=4, minibatches=4, lr=1e-3)
    ref, got = make_loop(64, 4, one_call=False, **kw), make_loop(64, 4, target_kl=target_kl, **kw)
    assert got.one_call and got.target_kl == target_kl
    for u in range(2):
        ran, mean = kl_reference(torch, ref, target_kl)
        losses = got.update()
        print(f"update {u} target_kl {target_kl:g}: reference ran {ran} epochs, approximate KL {mean[5].item():.3g}; the loop ran {got.epochs_run}")
        assert ran == epochs_run and got.epochs_run == epochs_run
        assert torch.equal(bits(losses), bits(mean))
        assert same_loop(torch, loop_state(got), loop_state(ref))
    capsys.readouterr()
    got.run(1, log_every=1)
    line = capsys.readouterr().out
    assert f"/ EPOCHS {epochs_run}" in line and "APPROX_KL" in line
    ref.run(1, log_every=1)                                      # the composed path's line is the one of before
    assert "EPOCHS" not in capsys.readouterr().out


def test_annealing_is_set_hparams_with_the_formula(torch_cuda):
    torch = torch_cuda
    lr, total = 1e-3, 4
    a, b = make_loop(64, 4, minibatches=2, lr=lr, anneal_lr=True, total_updates=total), make_loop(64, 4, minibatches=2, lr=lr, one_call=True)
    flat = make_loop(64, 4, minibatches=2, lr=lr, one_call=True)
    for u in range(3):
        b.net.set_hparams(lr=max(0.0, lr * (1.0 - u / total)))
        la, lb = a.update().clone(), b.update().clone()
        flat.update()
        assert torch.equal(bits(la), bits(lb)) and same_loop(torch, loop_state(a), loop_state(b)), u
    assert not same_loop(torch, loop_state(a), loop_state(flat)) and a.lr == lr       # the schedule did something; the base rate stays
    # at and past total_updates the rate is 0: Adam's moments move, the parameters do not
    a.update()
    p = a.net.store_params(0).clone()
    a.update()
    assert a.updates == 5 and torch.equal(a.net.store_params(0), p)


def test_checkpoints_with_the_options(torch_cuda, tmp_path):
    torch = torch_cuda
    on = dict(minibatches=2, lr=1e-3, adv_norm_scope="minibatch", target_kl=2e-4, anneal_lr=True, total_updates=6)
    straight = make_loop(64, 4, epochs=3, **on)
    ls = [straight.update().clone() for _ in range(4)]
    ran = []
    c = make_loop(64, 4, epochs=3, **on)
    for _ in range(2):
        c.update()
        ran.append(c.epochs_run)
    path = str(tmp_path / "opts.npz")
    c.save(path)
    z = np.load(path)
    assert z["ppo_opts"].tolist() == [1.0, 2e-4, 1.0, 6.0] and z["ppo"].tolist()[:2] == [3.0, 2.0]
    resumed = make_loop(64, 4, epochs=3, **on)
    resumed.load(path)
    assert same_loop(torch, loop_state(resumed), loop_state(c))
    for u in (2, 3):
        assert torch.equal(bits(resumed.update()), bits(ls[u])), u
        ran.append(resumed.epochs_run)
    print(f"epochs run per update: {ran}")
    assert min(ran) < 3                                          # (some update stopped early: the resumed run has unused draws behind it)
    assert same_loop(torch, loop_state(resumed), loop_state(straight))
    # a mismatch is refused by name, and changes nothing
    for kw, msg in ((dict(adv_norm_scope="rollout"), "adv_norm_scope = 'minibatch', this VecActorCritic has adv_norm_scope = 'rollout'"),
                    (dict(target_kl=None), "target_kl = 0.0002, this VecActorCritic has target_kl = 0.0"),
                    (dict(total_updates=7), "total_updates = 6, this VecActorCritic has total_updates = 7"),
                    (dict(anneal_lr=False, total_updates=None), "anneal_lr = True, this VecActorCritic has anneal_lr = False")):
        other = make_loop(64, 4, epochs=3, **{**on, **kw})
        st = loop_state(other)
        with pytest.raises(ValueError, match=msg):
            other.load(path)
        assert same_loop(torch, loop_state(other), st)
    # a file as the code before this key wrote it (every option off: no key) loads with the options off, into either path
    plain = make_loop(64, 4, epochs=3, minibatches=2, lr=1e-3)
    plain.update()
    old = str(tmp_path / "old.npz")
    plain.save(old)
    assert "ppo_opts" not in np.load(old).files and "ppo" in np.load(old).files
    for one_call in (False, True):
        into = make_loop(64, 4, epochs=3, minibatches=2, lr=1e-3, one_call=one_call)
        into.load(old)
        assert same_loop(torch, loop_state(into), loop_state(plain))
        assert (into.adv_norm_scope, into.target_kl, into.anneal_lr, into.total_updates) == ("rollout", 0.0, False, 0)
    with pytest.raises(ValueError, match="was written with adv_norm_scope = 'rollout', this VecActorCritic has adv_norm_scope = 'minibatch'"):
        make_loop(64, 4, epochs=3, **on).load(old)
