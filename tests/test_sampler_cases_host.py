"""tests/samplecases.py on the host: the logging generator leaves CPython's stream alone, and what the case list covers.

The census totals are CONDITIONS on the list, computed from CPython's `random` alone (no kernel result is read or modelled): if the
list stopped putting draws on the block edge, into the last 63 words of a block, onto repeated candidates or on either side of
setsize, the GPU sweep (tests/test_gpu_sampler_sweep.py) would pass vacuously.

With seed 7, the 150 cases and 40 draws per case (6000 draws) the reference gives
    pool 1200, set 4800, cross 1313, tail_start 340, opt_ok 1705, opt_short 674, opt_dup 181, dup_same 975, dup_cross 1028,
    regen_in_pool 240;
    cross per k: 0 at k = 1, 5, 6, then 18, 18, 26, 61, 64, 67, 85, 86, 132, 211, 271, 274 at k = 21 .. 256.
A setsize restated with its second step at k = 23 instead of 22 puts the (n = 277, k = 22) case on the set path: pool drops by 40,
the step list reads [6, 23, 86], and the logged words replayed on that path no longer give CPython's sample
(test_a_wrong_setsize_is_rejected)."""
import os
import random
import re
from collections import Counter

import pytest

from tests import samplecases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = dict(pool=1000, cross=500, tail_start=100, opt_ok=500, opt_short=200, opt_dup=50, dup_same=300, dup_cross=300, regen_in_pool=100)
SEED7_TOTALS = dict(pool=1200, set=4800, cross=1313, tail_start=340, opt_ok=1705, opt_short=674, opt_dup=181, dup_same=975, dup_cross=1028,
                    regen_in_pool=240)


def sampler_constant(name):
    """a `constexpr int NAME = value` of csrc/fb_sampler.h, read from the header"""
    text = open(os.path.join(ROOT, "dqnflappybird_amd", "csrc", "fb_sampler.h")).read()
    m = re.search(r"\b%s\s*=\s*(\d+)\s*[,;]" % re.escape(name), text)
    assert m, f"{name} not found in fb_sampler.h"
    return int(m.group(1))


@pytest.fixture(scope="module")
def totals():
    return S.census_all()


def test_case_list_is_the_one_the_sweep_documents():
    assert len(S.CASES) == 150 and len(set(S.CASES)) == 150 and len(S.CASES) * S.DRAWS == 6000
    assert S.KS == (1, 5, 6, 21, 22, 32, 63, 64, 65, 85, 86, 128, 200, 255, 256)
    for k in S.KS:
        s = S.setsize(k)
        assert S.sizes(k) == (k, s, s + 1, 2 * s + 3, 4099, 65536, 65537, 1_000_000, 1_048_575, 1_048_576)
        assert k <= s                            # n = k, the whole population, is a pool-path case
    assert all(n >= k for n, k in S.CASES)
    assert max(n for n, _ in S.CASES) < 2 ** 22  # what fb_replay_create takes
    assert sum(len(ks) for ks in S.by_n().values()) == 150


def test_setsize_steps_where_cpython_puts_them():
    """21 up to k = 5, then 21 + 4 ** ceil(log(3k, 4)): steps exactly at 6, 22 and 86, and the largest value fits the kernel's pool"""
    want = {k: 21 if k <= 5 else 85 if k <= 21 else 277 if k <= 85 else 1045 for k in range(1, 257)}
    got = {k: S.setsize(k) for k in range(1, 257)}
    assert got == want
    assert sorted(set(got.values())) == [21, 85, 277, 1045]
    assert [k for k in range(2, 257) if got[k] != got[k - 1]] == [6, 22, 86]
    assert S.setsize(256) <= sampler_constant("FB_SAMPLE_POOL") == 1100
    assert sampler_constant("FB_SAMPLE_MAXB") == 256 == max(S.KS)
    # the set path's table holds at most 256 selected values and one window of 64 more
    assert sampler_constant("FB_SAMPLE_TAB") >= 2 * (256 + S.WINDOW)


def test_setsize_decides_the_path_like_random_sample_does():
    """the helper's pool / set split is the one Lib/random.py makes: sample() replayed by hand from the word log, on the path the
    helper's setsize names, consumes exactly the logged words and gives CPython's sample"""
    for n, k in S.CASES:
        r = S.LoggingRandom(S.SEED)
        for _ in range(3):
            del r.log[:]
            want = r.sample(range(n), k)
            assert S.replay(r.log, n, k, pool=n <= S.setsize(k)) == want, (n, k)


def test_logging_generator_leaves_the_stream_alone(oracle):
    """every case: the logging subclass draws what random.Random draws; the oracle's PyRandom.sample draws the same and ends every
    draw on the word the log ends on (its block index == the census's word offset mod 624), and both go on with the same word"""
    for seed in (S.SEED, S.SEED_WIDE):
        for n, k in S.CASES:
            if seed == S.SEED_WIDE and k not in (64, 65, 256):
                continue
            _, samples, offsets = S.census(seed, n, k)
            assert samples == S.expected(seed, n, k), (seed, n, k)
            o = oracle.PyRandom(seed)
            for want, off in zip(samples, offsets):
                assert o.sample(n, k).tolist() == want, (seed, n, k)
                assert o.s.idx % S.BLOCK == off % S.BLOCK, (seed, n, k)
            r = random.Random(seed)
            for _ in range(S.DRAWS):
                r.sample(range(n), k)
            assert o.getrandbits(32) == r.getrandbits(32), (seed, n, k)


def test_every_draw_is_on_exactly_one_path(totals):
    total, _ = totals
    assert total["pool"] + total["set"] == 6000
    small = sum(S.DRAWS for n, k in S.CASES if k <= S.WINDOW and n > S.setsize(k))
    assert total["opt_ok"] + total["opt_dup"] + total["opt_short"] == small == 2560


def test_case_list_reaches_every_branch_often_enough(totals):
    total, cross = totals
    print("census, seed", S.SEED, {e: total[e] for e in S.EVENTS})
    print("cross per k", {k: cross[k] for k in S.KS})
    report = f"totals {dict(total)}, cross per k {dict(cross)}"
    for event, floor in FLOORS.items():
        assert total[event] >= floor, f"{event} = {total[event]} < {floor}: {report}"
    for k in S.KS:
        if k >= 21:
            assert cross[k] >= 10, f"k = {k}: cross = {cross[k]} < 10: {report}"
    if S.SEED == 7:
        assert {e: total[e] for e in SEED7_TOTALS} == SEED7_TOTALS, report
        assert cross[21] == 18 and [cross[k] for k in S.KS] == sorted(cross[k] for k in S.KS), report


def test_window_bookkeeping_on_hand_made_logs():
    """draw_events on logs small enough to read: block edge, tail start, the three outcomes of the first window, both kinds of repeat"""
    n, k, bits = 1000, 3, 10
    log = lambda *vals: [(bits, v) for v in vals]
    assert S.draw_events(0, log(1, 2, 3), n, k) == {"set", "opt_ok"}
    assert S.draw_events(0, log(1, 1001, 2, 3), n, k) == {"set", "opt_ok"}                    # a rejected word is no candidate
    assert S.draw_events(0, log(1, 1, 2, 3), n, k) == {"set", "opt_dup", "dup_same"}
    assert S.draw_events(0, log(1, 2, 3, 3)[:3], n, k) == {"set", "opt_ok"}
    assert S.draw_events(622, log(1, 2, 3), n, k) == {"set", "cross", "tail_start", "opt_short"}
    assert S.draw_events(622, log(1, 2, 1, 3), n, k) == {"set", "cross", "tail_start", "opt_short", "dup_cross"}
    assert S.draw_events(623, log(1, 2, 2, 3), n, k) == {"set", "cross", "tail_start", "opt_short", "dup_same"}
    assert S.draw_events(624, log(1, 2, 3), n, k) == {"set", "opt_ok"}                        # a draw that STARTS on the edge crosses nothing
    assert S.draw_events(560, log(1, 2, 3), n, k) == {"set", "opt_ok"}                        # 64 words left: a full window
    assert S.draw_events(561, log(1, 2, 3), n, k) == {"set", "tail_start", "opt_ok"}
    assert S.windows(600, 100) == [(0, 24, 24), (24, 88, 64), (88, 100, 64)]
    assert S.draw_events(0, log(1, 2, 3), 20, k) == {"pool", "regen_in_pool"}
    assert S.draw_events(5, log(1, 2, 3), 20, k) == {"pool"}
    assert S.draw_events(623, log(1, 2, 3), 20, k) == {"pool", "cross", "regen_in_pool"}
    assert S.draw_events(0, log(*range(70)), n, 70) == {"set"}                                # k > 64: no optimistic path to classify


def test_a_wrong_setsize_is_rejected():
    """the second step at k = 23 instead of 22: the restatement test's condition fails, and the census moves -- the cases at
    n = setsize and setsize + 1 are there to see exactly this"""
    def wrong(k):
        return 85 if k == 22 else S.setsize(k)

    assert [k for k in range(2, 257) if wrong(k) != wrong(k - 1)] == [6, 23, 86]          # (what the restatement test would see)
    # the one case of the list it reclassifies: n = setsize(22), which CPython samples through the pool
    assert [(n, k) for n, k in S.CASES if (n <= S.setsize(k)) != (n <= wrong(k))] == [(277, 22)]
    right, moved = totals_of(S.setsize), totals_of(wrong)
    print("census with the step at 23", {e: moved[e] for e in S.EVENTS})
    assert right["pool"] - moved["pool"] == S.DRAWS == moved["set"] - right["set"]
    # and the stream itself gives the wrong class away: replayed on the set path, the log does not give CPython's sample
    r = S.LoggingRandom(S.SEED)
    want = r.sample(range(277), 22)
    assert 277 > wrong(22) and S.replay(r.log, 277, 22, pool=False) != want == S.replay(r.log, 277, 22, pool=True)


def totals_of(size):
    total = Counter()
    for n, k in S.CASES:
        if k == 22:                              # (the only k the two differ on)
            total.update(S.census(S.SEED, n, k, size=size)[0])
    return total
