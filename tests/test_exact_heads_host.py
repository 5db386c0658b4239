"""The constructed head biases of tests/test_gpu_exact_heads.py, host side.  A head whose weight matrix is all zero gives theta (or
logits, or Q) that are its biases, for every state, on every path: fmaf(x, 0, acc) leaves acc.  Here: the builders of those biases
(shared with the GPU tests), and the check that what the GPU tests then expect is exact in fp32 -- the sums a wave forms over the
quantiles agree bit for bit in forward, reversed and pairwise (butterfly) order and equal the float64 sum, 1 / N is a power of two, and
the dueling fold's v + (a - sum_a / A) is exact for the integer biases and power-of-two action counts chosen."""
import numpy as np
import pytest

from tests.test_oracle_qnet import tensor_bounds
from tests.test_qr_host import np_qr_loss

HEAD0 = lambda fc: 77984 + 1600 * fc + fc                        # W_fc2's first entry (tests/test_gpu_c51.py::head0)
KINDS = ("plain", "dueling", "c51", "c51dueling", "noisy-c51", "noisy-c51dueling", "qr", "qrdueling")
N_DIST = 16                                                      # atoms / quantiles of the tie nets: A N = 128 at A = 8


def arch_of(kind):
    return kind.split("-")[-1]


def layout(kind):
    """tests/test_oracle_qnet.py::tensor_bounds's name for the head's layout"""
    return {"qr": "c51", "qrdueling": "c51dueling"}.get(arch_of(kind), arch_of(kind))


def with_head(p, fc, A, kind, N, b, b_v=None):
    """the flat vector p with every head weight (and, for a noisy net's [mu | sigma], every sigma) zero and the head's biases set:
    b [A, N] ([A] on a scalar head), b_v [N] ([1]) on a dueling head"""
    out = np.array(p, np.float32)
    out[HEAD0(fc):] = 0.0
    for name, lo, hi in tensor_bounds(fc, A, layout(kind), N)[8:]:
        if name in ("b_q", "b_head", "b_adv"):
            out[lo:hi] = np.asarray(b, np.float32).ravel()
        elif name == "b_v":
            out[lo:hi] = np.asarray(b_v, np.float32).ravel()
    return out


def fold32(b_v, b_a):
    """c51d_fold_kernel's b_eff in float32, in its order: v + (a - (sum over the actions, 0 .. A-1 in turn) / A)"""
    b_v, b_a = np.asarray(b_v, np.float32), np.asarray(b_a, np.float32)
    sm = np.zeros(b_a.shape[1], np.float32)
    for q in range(b_a.shape[0]):
        sm = sm + b_a[q]
    return b_v[None, :] + (b_a - sm[None, :] / np.float32(b_a.shape[0]))


def level_rows(kind, levels, N=N_DIST):
    """-> (b, b_v): head biases that give action a a Q growing with levels[a], and bit-identical rows to actions of equal level.
    Scalar heads: Q = the level.  QR: the level plus an integer ramp.  C51: logits level / 4 x the atom's index (an exponential tilt
    towards the high atoms: the expectation grows with the level).  Dueling heads add a value stream common to all actions."""
    lv = np.asarray(levels, np.float32)
    arch = arch_of(kind)
    if arch in ("plain", "dueling"):
        return lv, (np.float32([1.0]) if arch == "dueling" else None)
    i = np.arange(N, dtype=np.float32)
    b = lv[:, None] + (i - N // 2)[None, :] if arch.startswith("qr") else 0.25 * lv[:, None] * i[None, :]
    return b.astype(np.float32), ((i % 3).astype(np.float32) if arch.endswith("dueling") else None)


def tie_patterns(A):
    """levels per action with exact ties: all actions; at A >= 3 a tie of 1 and 2 below action 0 and above it; at A = 8 ties at the end"""
    pats = [[0] * A, [3] * A]
    if A >= 3:
        pats += [[2, 1, 1] + [0] * (A - 3), [0, 1, 1] + [-1] * (A - 3)]
    if A == 8:
        pats += [[0] * 6 + [5, 5], [1, 0, 0, 0, 2, 0, 2, 2]]
    return pats


def shaped_rows(levels, N=4):
    """QR rows of equal integer sums and different shapes: action a holds levels[a] + (a + 1) x [-3, -1, 1, 3] (N = 4)"""
    assert N == 4
    return np.float32([[lv + (a + 1) * k for k in (-3, -1, 1, 3)] for a, lv in enumerate(levels)])


def distinct_rows(A, N):
    """target rows that differ per action at O(1): action a holds 2 a + an integer ramp"""
    return np.float32([[2 * a + i - N // 2 for i in range(N)] for a in range(A)])


def sums32(x):
    """the float32 sum of x in forward, reversed and pairwise (the wave butterfly's) order"""
    x = np.asarray(x, np.float32)
    f = np.float32(0)
    for v in x:
        f = np.float32(f + v)
    r = np.float32(0)
    for v in x[::-1]:
        r = np.float32(r + v)
    y = np.concatenate([x, np.zeros(64 - len(x), np.float32)])
    while len(y) > 1:
        y = (y[: len(y) // 2] + y[len(y) // 2:]).astype(np.float32)
    return f, r, y[0]


def expected_qr(th_on, th_sel, th_tg, a, r, t, gamma, kappa, w=None):
    """float64, from the definitions of include/fbdqn.h with np.argmax's first maximum: -> (loss, l_b [B], dl/dtheta [A, N] summed over
    the batch and divided by B, the same with |.| of every term, a*)"""
    th_on, th_sel, th_tg = (np.asarray(x, np.float64) for x in (th_on, th_sel, th_tg))
    B = len(a)
    astar = int(np.argmax(th_sel.mean(1)))
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    lb, g, gabs = np.zeros(B), np.zeros_like(th_on), np.zeros_like(th_on)
    for b in range(B):
        T = float(r[b]) + gamma * (1.0 - float(t[b])) * th_tg[astar]
        lb[b], gb = np_qr_loss(th_on[a[b]], T, kappa)
        g[a[b]] += w[b] * gb / B
        gabs[a[b]] += np.abs(w[b] * gb) / B
    return float((w * lb).mean()), lb, g, gabs, astar


# ---------------------------------------------------------------------------------------------------------------- exactness
def exact_theta_rows():
    rows = []
    for N in (2, 4, 16, 64):
        rows += [np.arange(N, dtype=np.float32) - N // 2 + lv for lv in (-1, 0, 3, 100)]
    rows += list(shaped_rows([0, 0, 0, 0, 5, 5, -2, 1]))
    rows += list(distinct_rows(8, 16)) + list(distinct_rows(3, 2))
    for A in (2, 8):
        b, b_v = level_rows("qrdueling", [0, 1, 1, -1, 2, 2, 0, 3][:A])
        rows += list(fold32(b_v, b)) + list(fold32(np.arange(4) % 3, shaped_rows([1, 1, 0, 0, 2, 2, 2, -3][:A])))
    return rows


def test_the_sums_of_the_constructed_quantiles_are_exact_in_any_order():
    rows = exact_theta_rows()
    assert len(rows) > 50
    for x in rows:
        N = len(x)
        assert N & (N - 1) == 0                                  # 1 / N is a power of two: the mean is one exact scaling
        want = np.asarray(x, np.float64).sum()
        f, r, p = sums32(x)
        assert f == r == p == want and float(np.float32(want)) == want
        assert float(np.float32(f) * np.float32(1.0 / N)) == want / N


def test_the_dueling_fold_is_exact_for_the_chosen_biases():
    for A in (2, 8):
        cases = [level_rows("qrdueling", lv[:A]) for lv in ([0, 1, 1, -1, 2, 2, 0, 3], [3] * 8, [0] * 6 + [5, 5])]
        cases += [(shaped_rows(lv[:A]), np.arange(4) % 3) for lv in ([1, 1, 0, 0, 2, 2, 2, -3], [0] * 8)]
        for b, b_v in cases:
            b64, v64 = np.asarray(b, np.float64), np.asarray(b_v, np.float64)
            want = v64[None, :] + b64 - b64.mean(0, keepdims=True)
            got = fold32(b_v, b)
            assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    # the scalar dueling head: V + (A_a - mean_a A_a) with integer levels and A = 2 or 8
    for lv in tie_patterns(2) + tie_patterns(8):
        lv32 = np.float32(lv)
        mean = np.float32(0)
        for v in lv32:
            mean = np.float32(mean + v)
        mean = np.float32(mean / np.float32(len(lv)))
        q = np.float32(1.0) + (lv32 - mean)
        assert np.array_equal(q.astype(np.float64), 1.0 + np.asarray(lv, np.float64) - np.mean(lv))


def test_tied_rows_are_bit_identical_and_the_levels_order_the_expectations():
    """what the tie tests rely on for every kind, at any A (the dueling mean at A = 3 need not be exact: tied actions subtract the
    same number from the same number): equal levels -> identical bias rows; a higher level -> a higher Q by a wide margin"""
    for kind in KINDS:
        for A in (2, 3, 8):
            for lv in tie_patterns(A):
                b, b_v = level_rows(kind, lv)
                for x in range(A):
                    for y in range(A):
                        assert (lv[x] == lv[y]) == bool(np.array_equal(b[x], b[y]))
                if "c51" in kind:
                    lg = np.asarray(b, np.float64) + (0.0 if b_v is None else np.asarray(b_v, np.float64)[None, :])
                    p = np.exp(lg - lg.max(1, keepdims=True))
                    q = (p / p.sum(1, keepdims=True) * np.linspace(-10.0, 10.0, N_DIST)).sum(1)
                elif "qr" in kind:
                    q = np.asarray(b, np.float64).mean(1)
                else:
                    q = np.asarray(b, np.float64)
                for x in range(A):
                    for y in range(A):
                        if lv[x] > lv[y]:
                            assert q[x] > q[y] + 0.25, (kind, lv)


def test_the_worked_case_and_the_kinks_on_the_lattice():
    """the values the device cases use are exact in fp32 and their expected results are the header's"""
    loss, lb, g, _, astar = expected_qr([[9, 9], [0, 1], [7, 8]], [[-4, -2], [0, 5], [-3, 1]], [[-4, -2], [0, 5], [-3, 1]],
                                        [1, 1], [0.5, 0.5], [0, 0], 0.5, 1.0)
    assert astar == 1 and loss == 0.90625 and np.array_equal(g[1], [-0.1875, -0.3125]) and not g[0].any() and not g[2].any()
    for v in (0.90625, 0.1875, 0.3125, 0.90625 * 256, 0.1875 / 256, 0.3125 / 256):
        assert float(np.float32(v)) == v
    for k in (0.5, 1.0, 2.0):                                    # |u| = kappa on every pair: terminal, T = r = +-k
        for sign in (1.0, -1.0):
            loss, _, g, _, _ = expected_qr([[0, 0], [5, 5]], [[0, 0], [0, 0]], [[1e30, 1e30], [1e30, 1e30]], [0], [sign * k], [1], 0.5, k)
            assert loss == pytest.approx(0.5 * k) and np.allclose(g[0], [-0.25, -0.75] if sign > 0 else [0.75, 0.25]) and not g[1].any()
