"""Kink-free minibatches of any size, for gradient checks that compare every element.

A gradient through a ReLU or a max-pool is only comparable between two arithmetics away from the kinks: a unit whose input sits
within rounding distance of 0 (or a pool winner within rounding distance of its runner-up) takes another mask on the device than in
the float64-accumulating oracle, and its whole contribution differs.  The oracle reports the smallest such distance of a forward
pass (oracle.last_margin), as the minimum over the samples of the batch: the margin is a property of ONE SAMPLE.  Rejecting whole
batches (as the small-batch tests do) stops working near B = 100; rejecting samples one by one costs ~1 / 0.96 oracle forwards per
accepted state at margin 1e-4, at any batch size, and every prefix of an accepted pool is kink-free too.

Only the trunk (conv1 .. fc1) has kinks, and it depends only on the fc1 width: the margin is taken through an oracle config of that
width with a one-column dummy head, so the same helper serves the scalar, C51, QR, dueling and noisy nets (a noisy net: pass the
effective fc1 weights mu + sigma (.) e).  Only the states the gradient flows through need a margin; the next states s' do not.

Not a conftest and not a test module: imported by tests/test_kinkfree_host.py and tests/test_gpu_kinkfree_grads.py."""
import zlib

import numpy as np

from tests.test_oracle_qnet import rand_states

MARGIN = 1e-4            # tests/test_gpu_qnet.py::Q_ATOL, the project's bound on device-versus-oracle outputs
MIN_SHARE_RANDOM = 0.8   # accepted / drawn must reach these: the oracle alone gives 0.96 (random states) and 0.95 (game frames) at 1e-4
MIN_SHARE_FRAMES = 0.5
POOL = 256


def trunk_size(fc):
    """the flat vector up to the head's first entry (conv1 .. b_fc1)"""
    return 77984 + 1600 * fc + fc


def trunk_params(oracle, p_trunk, fc):
    """(oracle config, float32 parameters) of the width-fc trunk under a one-action zero head"""
    n = trunk_size(fc)
    p_trunk = np.asarray(p_trunk)
    assert p_trunk.ndim == 1 and p_trunk.size >= n, (p_trunk.shape, n)
    cfg = oracle.qcfg(fc, 1, False)
    p = np.zeros(oracle.nparams(cfg), np.float32)
    p[:n] = p_trunk[:n]
    return cfg, p


def margin_of(oracle, p_trunk, fc, states, nonzero=False):
    """the oracle's kink margin of a batch of states (its minimum over the samples) under the trunk"""
    cfg, p = trunk_params(oracle, p_trunk, fc)
    oracle.forward(p, cfg, states)
    return float(oracle.last_margin(nonzero=nonzero))


def kink_free_states(oracle, p_trunk, fc, n, seed, margin=MARGIN, source=None, nonzero=False, picked=None):
    """-> (u8[n, 80, 80, 4], candidates drawn): n states whose oracle margin under the net's online trunk p_trunk (a flat parameter
    vector; only its first trunk_size(fc) entries are read) exceeds `margin`, each candidate judged alone.

    Candidates come one at a time from rand_states under default_rng(seed), or from source(), a callable that returns one candidate
    u8[80, 80, 4] per call (seed is then unused; game frames: nonzero=True leaves the exact ties of pool windows over identical
    pixels out, as tests/test_gpu_shims.py does).  picked: a list that receives the ordinal numbers of the accepted candidates, for
    a source that has to know which of its draws were taken.  Asserts that the accepted share is not small: a helper that threw
    most of the data away would be hiding something."""
    cfg, p = trunk_params(oracle, p_trunk, fc)
    rng = np.random.default_rng(seed)
    out = np.empty((n, 80, 80, 4), np.uint8)
    got = drawn = 0
    floor = MIN_SHARE_RANDOM if source is None else MIN_SHARE_FRAMES
    while got < n:
        assert drawn < 64 or got >= floor * drawn * 0.5, f"accepted {got} of {drawn} candidates at margin {margin}"
        s = rand_states(rng, 1) if source is None else np.ascontiguousarray(source(), np.uint8).reshape(1, 80, 80, 4)
        oracle.forward(p, cfg, s)
        if oracle.last_margin(nonzero=nonzero) > margin:
            out[got] = s[0]
            got += 1
            if picked is not None:
                picked.append(drawn)
        drawn += 1
    assert got >= floor * drawn, f"accepted {got} of {drawn} candidates at margin {margin}: below the share of {floor}"
    return out, drawn


_pools = {}


def pool(oracle, p_trunk, fc, seed, margin=MARGIN):
    """the shared pool of POOL kink-free random states of one (trunk, fc): built on first use, then handed out read-only, so the
    rejection cost is paid once per net.  Tests take prefixes.  -> (states, drawn)"""
    n = trunk_size(fc)
    key = (fc, zlib.crc32(np.ascontiguousarray(p_trunk[:n]).tobytes()), seed, margin)
    if key not in _pools:
        s, drawn = kink_free_states(oracle, p_trunk, fc, POOL, seed, margin)
        s.setflags(write=False)
        _pools[key] = (s, drawn)
    return _pools[key]
