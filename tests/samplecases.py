"""The replay samplers' case list, and a census of what CPython's own stream does on it.

`random.sample(range(n), k)` on the device is one piece of lock-step wave code (csrc/fb_sampler.h, sample_cpython_body): an
optimistic ballot path for k <= 64, a loop over windows of up to 64 state words with a hash table of the selected values, a
word-serial pool path for n <= setsize, and MT19937 regeneration at the 624-word block edge in the middle of any of these.
CASES puts a k on either side of every step of setsize, of the optimistic path's limit and of the 64-lane register slots, and
an n on either side of the pool / set switch and of the steps of n.bit_length().

census() is a statement about the CPython stream alone: it logs every word a `sample()` call consumes and counts, from the log
and the word offset since seeding, how often the stream puts a draw where that control flow branches.  It neither reads nor
models a kernel result; tests/test_sampler_cases_host.py holds the totals to floors, so that a later edit of the list cannot
hollow out the GPU sweep (tests/test_gpu_sampler_sweep.py)."""
import random
from collections import Counter
from math import ceil, log

SEED = 7
SEED_WIDE = 2 ** 40 + 7                  # a two-word init_by_array key
DRAWS = 40
KS = (1, 5, 6, 21, 22, 32, 63, 64, 65, 85, 86, 128, 200, 255, 256)
BLOCK = 624                              # MT19937 state words; the device's index starts at 624, so the first draw regenerates
WINDOW = 64                              # one wave
EVENTS = ("pool", "set", "cross", "tail_start", "opt_ok", "opt_dup", "opt_short", "dup_same", "dup_cross", "regen_in_pool")


def setsize(k):
    """Lib/random.py, sample(): the population size up to which the pool path is taken"""
    s = 21
    if k > 5:
        s += 4 ** ceil(log(k * 3, 4))
    return s


def sizes(k):
    s = setsize(k)
    return (k, s, s + 1, 2 * s + 3, 4099, 65536, 65537, 1_000_000, 1_048_575, 1_048_576)


CASES = tuple((n, k) for k in KS for n in sizes(k))


def by_n(cases=CASES):
    """{n: [k, ...]} -- one memory per n serves every k drawn from it"""
    out = {}
    for n, k in cases:
        out.setdefault(n, []).append(k)
    return out


class LoggingRandom(random.Random):
    """random.Random that logs (bits, value) of every getrandbits call; a call of at most 32 bits is one MT19937 word.  Overriding
    getrandbits alone keeps _randbelow on its getrandbits form, which is what random.Random itself uses."""

    def __init__(self, seed):
        self.log = []
        super().__init__(seed)

    def getrandbits(self, k):
        v = super().getrandbits(k)
        self.log.append((k, v))
        return v


def expected(seed, n, k, draws=DRAWS):
    """the `draws` consecutive random.sample(range(n), k) after random.seed(seed)"""
    r = random.Random(seed)
    return [r.sample(range(n), k) for _ in range(draws)]


def replay(log, n, k, pool):
    """Lib/random.py's sample() run by hand on a word log, on the path `pool` names -> the sample, or None where the log is not what
    that path would have consumed (words left over, or too few)"""
    vals, out = iter(log), []
    try:
        if pool:
            left = list(range(n))
            for i in range(k):
                v = next(vals)[1]
                while v >= n - i:
                    v = next(vals)[1]
                out.append(left[v])
                left[v] = left[n - i - 1]
        else:
            taken = set()
            for _ in range(k):
                v = next(vals)[1]
                while v >= n or v in taken:
                    v = next(vals)[1]
                taken.add(v)
                out.append(v)
    except StopIteration:
        return None
    return out if next(vals, None) is None else None


def get_leaf(tree, v):
    """SumTree.get_leaf (BrainPrioritizedReplyDQN.py:85-100) on a flat heap -> tree index of the leaf"""
    i = 0
    while 2 * i + 1 < len(tree):
        l = 2 * i + 1
        if v <= tree[l]:
            i = l
        else:
            v -= tree[l]
            i = l + 1
    return i


def windows(start, words):
    """the consecutive chunks of min(64, words left in the block) words from word offset `start`, as (lo, hi) into the draw's log"""
    out, lo = [], 0
    while lo < words:
        left = BLOCK - (start + lo) % BLOCK
        hi = min(words, lo + min(WINDOW, left))
        out.append((lo, hi, min(WINDOW, left)))
        lo = hi
    return out


def draw_events(start, log, n, k, size=setsize):
    """the events of one draw that began `start` words after seeding and consumed the words of `log`"""
    ev = set()
    words = len(log)
    assert all(bits <= 32 for bits, _ in log) and words >= 1
    crosses = start // BLOCK != (start + words - 1) // BLOCK
    if crosses:
        ev.add("cross")
    if n <= size(k):
        ev.add("pool")
        if crosses or start % BLOCK == 0:
            ev.add("regen_in_pool")
        return ev
    ev.add("set")
    if BLOCK - start % BLOCK < WINDOW:
        ev.add("tail_start")
    win = windows(start, words)
    seen = set()
    for w, (lo, hi, full) in enumerate(win):
        cand = [v for _, v in log[lo:hi] if v < n]
        if len(set(cand)) < len(cand):
            ev.add("dup_same")
        if seen & set(cand):
            ev.add("dup_cross")
        seen |= set(cand)
        if w == 0 and k <= WINDOW:
            # a log that ends inside the first window completed the sample there; one that goes on either ran out of candidates
            # (fewer than k in the whole window) or met a repeat among the first k
            if len(cand) < k:
                assert hi - lo == full
                ev.add("opt_short")
            else:
                ev.add("opt_ok" if len(set(cand[:k])) == k else "opt_dup")
    return ev


def census(seed, n, k, draws=DRAWS, size=setsize):
    """-> (Counter of EVENTS over `draws` consecutive sample(range(n), k) after one seed, the samples, the word offset after each)"""
    r = LoggingRandom(seed)
    r.log.clear()
    count, samples, offsets, start = Counter(), [], [], 0
    for _ in range(draws):
        samples.append(r.sample(range(n), k))
        log = r.log[:]
        r.log.clear()
        count.update(draw_events(start, log, n, k, size))
        start += len(log)
        offsets.append(start)
    return count, samples, offsets


def census_all(seed=SEED, cases=CASES, draws=DRAWS, size=setsize):
    """-> (Counter over the whole list, {k: `cross` summed over that k's cases})"""
    total, cross = Counter(), Counter()
    for n, k in cases:
        c = census(seed, n, k, draws, size)[0]
        total.update(c)
        cross[k] += c["cross"]
    return total, cross
