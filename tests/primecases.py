"""A NumPy restatement of include/fbdqn.h's FB_PER_INIT_TD (fb_replay_prime_priorities), shared by tests/test_prime_host.py and
tests/test_gpu_prime.py: the |TD error| and the priority of a stored transition from the acting-time Q-values, with the header's
float and double steps, and a prioritized tree kept the FB_PER_FAST way -- every inner node left + right in float64, with the max and
min heaps alongside -- driven by stores at max_p, primes and batch_updates."""
import numpy as np

P_EXP = np.float64(np.float32(0.6))                          # (double)0.6f: Memory.alpha as the kernels hold it
P_MIN, P_MAX = np.float32(np.float64(np.float32(0.01)) ** P_EXP), np.float32(1.0)


def priority(delta):
    """Memory.batch_update's formula as per_update_fast_kernel has it: (float)pow((double)min(delta + 0.01f, 1.0f), (double)0.6f)"""
    delta = np.asarray(delta, np.float32)
    c = np.minimum(delta + np.float32(0.01), np.float32(1.0)).astype(np.float32)
    return np.power(c.astype(np.float64), P_EXP).astype(np.float32)


def td_delta(R, done, q, rec, Gamma):
    """R f32[N], done u8[N]: the ring's n-step read; q f32[N, A]: Q(s', .) of the bootstrap state; rec f32[N]: the recorded Q(s, a);
    Gamma: the bootstrap discount.  y = done ? R : R + Gamma * max_a q in float64 (product, then sum); -> (float)|y - (double)rec|"""
    R, q, rec = np.asarray(R, np.float32), np.asarray(q, np.float32), np.asarray(rec, np.float32)
    m = q.max(axis=1).astype(np.float64)
    y = np.where(np.asarray(done) != 0, R.astype(np.float64), R.astype(np.float64) + np.float64(Gamma) * m)
    return np.abs(y - rec.astype(np.float64)).astype(np.float32)


class FastTree:
    """SumTree + max / min heaps as array heaps of 2 cap - 1 nodes (leaf of data slot d: d + cap - 1), every touched inner node
    recomputed from its two children, deepest first"""

    def __init__(self, cap):
        self.cap, n = cap, 2 * cap - 1
        self.tree, self.maxt, self.mint = np.zeros(n), np.zeros(n), np.full(n, np.inf)
        self.pointer = self.size = 0

    def _refresh(self, leaves):
        nodes = set()
        for i in leaves:
            while i > 0:
                i = (i - 1) >> 1
                if i in nodes:
                    break
                nodes.add(i)
        for i in sorted(nodes, reverse=True):                # (children have larger indices than their parent)
            l, r = 2 * i + 1, 2 * i + 2
            self.tree[i] = self.tree[l] + self.tree[r]
            self.maxt[i] = max(self.maxt[l], self.maxt[r])
            self.mint[i] = min(self.mint[l], self.mint[r])

    def set_leaves(self, leaves, p):
        """leaves: heap indices; p: their values, later duplicates win"""
        leaves = [int(i) for i in leaves]
        for i, v in zip(leaves, np.asarray(p, np.float64)):
            self.tree[i] = self.maxt[i] = self.mint[i] = v
        self._refresh(leaves)

    def last_stored(self, N):
        """heap indices of the N leaves the last store wrote, in env order"""
        return [(self.pointer - N + e) % self.cap + self.cap - 1 for e in range(N)]

    def store(self, N):
        """Memory.store of N transitions: max_p (1.0 on an empty tree) into the next N data slots"""
        max_p = self.maxt[0] if self.maxt[0] != 0 else 1.0
        leaves = [(self.pointer + e) % self.cap + self.cap - 1 for e in range(N)]
        self.pointer, self.size = (self.pointer + N) % self.cap, min(self.size + N, self.cap)
        self.set_leaves(leaves, np.full(N, max_p))
        return max_p

    def level_sums(self, depth):
        """the values of the nodes at `depth` (root = 0), left to right"""
        return self.tree[(1 << depth) - 1:(1 << (depth + 1)) - 1]


class PrimedMemory:
    """The record of acting-time Q-values over a FastTree and a host copy of the pushed rows: prime(q, actions) then push(rew, term),
    once per step, as fb_vec_step orders them on a FB_PER_INIT_TD memory"""

    def __init__(self, cap, N, n, gamma):
        from tests.test_nstep_host import nstep_return
        self._ret = nstep_return
        self.t, self.N, self.n, self.gamma = FastTree(cap), N, n, gamma
        self.rews, self.terms, self.rec = [], [], {}
        self.last_delta = self.last_p = None

    @property
    def S(self):
        return len(self.rews)

    def clear_record(self):
        self.rec = {}

    def prime(self, q, actions):
        S, n, N = self.S, self.n, self.N
        q = np.asarray(q, np.float32)
        self.last_delta = self.last_p = None
        if S >= n and all(k in self.rec for k in range(S - n, S)):
            R, done, G = self._ret(np.stack(self.rews[S - n:S]), np.stack(self.terms[S - n:S]), self.gamma)
            self.last_delta = td_delta(R, done, q, self.rec[S - n], G)
            self.last_p = priority(self.last_delta)
            self.t.set_leaves(self.t.last_stored(N), self.last_p)
        if S - 1 not in self.rec:                            # (a gap: what was recorded before it is not consecutive)
            self.rec = {}
        self.rec[S] = q[np.arange(N), np.asarray(actions, np.int64)].copy()

    def push(self, rew, term):
        self.rews.append(np.asarray(rew, np.float32)); self.terms.append(np.asarray(term, np.uint8))
        if self.S >= self.n:
            self.t.store(self.N)
