"""tests/kinkfree.py on the host: the per-sample rejection that gives tests/test_gpu_kinkfree_grads.py its minibatches.  Determinism,
the margin of what it returns (alone and as a batch), the accepted shares at the three nets it was measured on, and the additivity
of the oracle's backward pass over the samples, which is what makes a per-sample margin enough."""
import numpy as np
import pytest

from tests import kinkfree
from tests.test_gpu_qnet import trained_like_params
from tests.test_oracle_qnet import rand_states, tensor_bounds

NETS = [(512, 2, False), (128, 1, True), (384, 3, True)]


def trunk_of(oracle, fc, A, dueling, seed=1):
    return trained_like_params(oracle, oracle.qcfg(fc, A, dueling), seed)


def test_deterministic_in_seed(oracle):
    p = trunk_of(oracle, 128, 1, True)
    a, na = kinkfree.kink_free_states(oracle, p, 128, 40, seed=7)
    b, nb = kinkfree.kink_free_states(oracle, p, 128, 40, seed=7)
    c, _ = kinkfree.kink_free_states(oracle, p, 128, 40, seed=8)
    assert a.shape == (40, 80, 80, 4) and a.dtype == np.uint8
    assert np.array_equal(a, b) and na == nb and not np.array_equal(a, c)
    # a shorter request is a prefix of a longer one: tests take prefixes of one pool
    d, _ = kinkfree.kink_free_states(oracle, p, 128, 9, seed=7)
    assert np.array_equal(d, a[:9])


@pytest.mark.parametrize("fc,A,dueling", NETS)
def test_margin_and_accepted_share(oracle, fc, A, dueling):
    """every returned state clears the threshold alone and in the batch (under the net's own config too, not only the dummy head's),
    rejected candidates exist and do not, and the share accepted is the one measured with the oracle (0.96 at 1e-4) -- the helper's
    own assertion asks for 0.8"""
    p = trunk_of(oracle, fc, A, dueling)
    picked = []
    s, drawn = kinkfree.kink_free_states(oracle, p, fc, kinkfree.POOL, seed=fc + A, picked=picked)
    assert len(s) == kinkfree.POOL == len(picked) and picked[-1] == drawn - 1
    share = kinkfree.POOL / drawn
    print(f"kink-free share fc={fc} A={A} dueling={dueling}: {kinkfree.POOL}/{drawn} = {share:.3f}")
    assert kinkfree.MIN_SHARE_RANDOM <= share <= 1.0
    assert 0.9 < share < 1.0                                  # (measured: 0.963 / 0.968 / 0.967)
    for b in range(0, kinkfree.POOL, 17):
        assert kinkfree.margin_of(oracle, p, fc, s[b:b + 1]) > kinkfree.MARGIN, b
    cfg = oracle.qcfg(fc, A, dueling)
    oracle.forward(p, cfg, s)
    assert oracle.last_margin() > kinkfree.MARGIN
    # the candidates it passed over are the same stream's, and sit inside the margin
    rng = np.random.default_rng(fc + A)
    cand = np.concatenate([rand_states(rng, 1) for _ in range(drawn)])
    assert np.array_equal(cand[picked], s)
    rejected = np.setdiff1d(np.arange(drawn), picked)
    assert len(rejected) > 0
    for k in rejected[:4]:
        assert kinkfree.margin_of(oracle, p, fc, cand[k:k + 1]) <= kinkfree.MARGIN


def test_source_candidates_and_the_share_floor(oracle):
    """a source is asked once per candidate and `picked` names the ones taken; a source that mostly fails is refused"""
    p = trunk_of(oracle, 128, 1, True)
    rng = np.random.default_rng(3)
    seen = []

    def source():
        seen.append(rand_states(rng, 1)[0])
        return seen[-1]

    picked = []
    s, drawn = kinkfree.kink_free_states(oracle, p, 128, 20, seed=None, source=source, nonzero=True, picked=picked)
    assert drawn == len(seen) and np.array_equal(np.stack(seen)[picked], s)
    with pytest.raises(AssertionError, match="accepted"):
        kinkfree.kink_free_states(oracle, p, 128, 20, seed=0, margin=0.05)


def test_pool_is_built_once(oracle):
    p = trunk_of(oracle, 128, 1, True)
    a, n = kinkfree.pool(oracle, p, 128, seed=5)
    b, _ = kinkfree.pool(oracle, p.copy(), 128, seed=5)
    assert a is b and len(a) == kinkfree.POOL and not a.flags.writeable
    q = p.copy()
    q[0] += 1.0
    assert kinkfree.pool(oracle, q, 128, seed=5)[0] is not a


def test_backward_is_additive_over_the_samples(oracle):
    """oracle.backward on the batch == the float64 sum of the 256 single-sample passes, to 1e-6 relative: no term couples two samples,
    so a batch of states that are kink-free one by one is a kink-free batch"""
    fc, A, dueling = 384, 3, True
    cfg = oracle.qcfg(fc, A, dueling)
    p = trunk_of(oracle, fc, A, dueling)
    s, _ = kinkfree.pool(oracle, p, fc, seed=fc + A)
    B = len(s)
    rng = np.random.default_rng(1)
    dq = (rng.standard_normal((B, A)) / B).astype(np.float32)
    q, acts = oracle.forward(p, cfg, s, keep=True)
    g = oracle.backward(p, cfg, s, acts, dq)
    total = np.zeros(g.size, np.float64)
    for b in range(B):
        qb, ab = oracle.forward(p, cfg, s[b:b + 1], keep=True)
        assert np.array_equal(qb[0], q[b])
        total += oracle.backward(p, cfg, s[b:b + 1], ab, dq[b:b + 1])
    for name, lo, hi in tensor_bounds(fc, A, "dueling"):
        np.testing.assert_allclose(g[lo:hi], total[lo:hi], rtol=1e-6, atol=1e-6 * np.abs(total[lo:hi]).max(), err_msg=name)
