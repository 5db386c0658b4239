// Minibatch assembly from the packed frame ring -- device code shared by the replay kernels (fb_replay.hip) and the ring-fed
// train trunk (fb_qnet.hip).  Included inside each translation unit's anonymous namespace.
#pragma once

__device__ __forceinline__ size_t fb_frame_off(const FbGatherCtx &P, long long f, int e) {
    if (f < 0) f = 0;                                   // setInitState: the first frame four times
    return ((size_t)(f % P.t_f) * P.n_envs + e) * 100;
}

// Where transition `j` of a sampled minibatch lives: (tt, e) = (time slot, env) of its frame t; its window is frames tt - 3 .. tt + 1 of
// env e.  j is a deque position (uniform memory, 0 = oldest) or a SumTree leaf index (prioritized memory); an index outside the
// filled part raises the memory's error flag (when `flag`) and reads transition 0.
__device__ __forceinline__ void fb_ring_locate(const FbGatherCtx &P, long long steps, long long j, bool flag, long long &tt, int &e) {
    const long long total = steps * P.n_envs;
    long long g;
    if (P.kind == FB_REPLAY_PER) {
        // (n-step memory: the tree has received C = max(0, steps - n + 1) N stores, one per COMPLETED transition; C = total at n = 1)
        const long long cs = steps - (P.nstep - 1), C = cs > 0 ? cs * P.n_envs : 0;
        long long d = j - (P.cap - 1);
        if (d < 0 || d >= P.cap || d >= C) { if (flag) *P.error = 1; d = 0; }
        g = C > 0 ? d + P.cap * ((C - 1 - d) / P.cap) : 0;      // newest transition living in data slot d (empty tree: transition 0)
    } else {
        const long long size = total < P.cap ? total : P.cap;
        // (n-step view: the newest (n - 1) x N positions are not complete yet -- their frame t + n has not been pushed)
        if (j < 0 || j >= size - (long long)(P.nstep - 1) * P.n_envs) { if (flag) *P.error = 1; j = 0; }
        g = total - size + j;                       // deque position j, 0 = oldest
    }
    tt = g / P.n_envs; e = (int)(g - tt * P.n_envs);
}

// The n-step return of transition (tt, e) of a memory viewed with n = P.nstep > 1 steps (include/fbdqn.h fb_replay_set_n_step):
// m = n, or k + 1 for the first k < n with term[tt + k] = 1; R = (float) sum_{k < m} g_k * (double) rew[tt + k], ascending k, g_0 = 1,
// g_{k+1} = g_k * gamma; done = some term[tt + k] = 1, k < n.  All n row loads are issued before any of them is used.  Rows tt .. tt + n - 1
// are n consecutive time slots: slot (tt % t_f) + k wraps at most once because n <= FB_NSTEP_MAX and cap >= n * N give t_f >= n + 6.
__device__ __forceinline__ void fb_nstep_return(const FbGatherCtx &P, long long tt, int e, float &R, uint8_t &done) {
    const int n = P.nstep, s0 = (int)(tt % P.t_f);
    float rw[FB_NSTEP_MAX];
    uint8_t tm[FB_NSTEP_MAX];
#pragma unroll
    for (int k = 0; k < FB_NSTEP_MAX; k++) {
        rw[k] = 0.0f; tm[k] = 0;
        if (k < n) {
            const int sk = s0 + k < P.t_f ? s0 + k : s0 + k - P.t_f;
            const size_t mo = (size_t)sk * P.n_envs + e;
            rw[k] = P.rew[mo]; tm[k] = P.term[mo];
        }
    }
    double acc = 0.0, g = 1.0;
    bool stop = false;
#pragma unroll
    for (int k = 0; k < FB_NSTEP_MAX; k++) {
        if (k < n && !stop) {
            acc += g * (double)rw[k];
            g *= P.gamma;
            stop = tm[k] != 0;
        }
    }
    R = (float)acc; done = stop ? 1 : 0;
}

// One thread expands 4 pixels x 4 stacked frames = 16 contiguous bytes of s (and of s').
__device__ __forceinline__ uint32_t expand4(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, int q) {
    return (((n0 >> q) & 1u) * 0xFFu) | (((n1 >> q) & 1u) * 0xFF00u) | (((n2 >> q) & 1u) * 0xFF0000u) |
           (((n3 >> q) & 1u) * 0xFF000000u);
}

// thread tid of B * 1600: sample tid / 1600, 16-byte chunk tid % 1600 of s (and of s')
template <bool CURRENT>
__device__ __forceinline__ void gather_body(const FbGatherCtx &P, long long steps, int B, const long long *__restrict__ idx,
                                            uint4 *__restrict__ s, uint4 *__restrict__ s2, uint8_t *__restrict__ a,
                                            float *__restrict__ r, uint8_t *__restrict__ t, long long tid) {
    // `steps` (pushes so far) comes by value from the host's mirror: one dependent global round trip less than reading
    // ReplayDev::steps here
    if (tid >= (long long)B * 1600) return;
    const int b = (int)(tid / 1600), chunk = (int)(tid - (long long)b * 1600);
    long long tt; int e;
    if (CURRENT) { tt = steps; e = b; }
    else fb_ring_locate(P, steps, idx[b], chunk == 0, tt, e);
    const int p = chunk * 4, w = p >> 6, sh = p & 63;
    uint32_t n[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        if (CURRENT && k == 4) { n[k] = 0; break; }
        n[k] = (uint32_t)(P.bits[fb_frame_off(P, tt - 3 + k, e) + w] >> sh) & 0xFu;
    }
    uint4 o;
    o.x = expand4(n[0], n[1], n[2], n[3], 0); o.y = expand4(n[0], n[1], n[2], n[3], 1);
    o.z = expand4(n[0], n[1], n[2], n[3], 2); o.w = expand4(n[0], n[1], n[2], n[3], 3);
    s[tid] = o;
    if (!CURRENT) {
        if (P.nstep > 1) {                              // n-step view: s' = frames tt + n - 3 .. tt + n (n[4] went unused)
#pragma unroll
            for (int k = 1; k < 5; k++) n[k] = (uint32_t)(P.bits[fb_frame_off(P, tt + P.nstep - 4 + k, e) + w] >> sh) & 0xFu;
        }
        o.x = expand4(n[1], n[2], n[3], n[4], 0); o.y = expand4(n[1], n[2], n[3], n[4], 1);
        o.z = expand4(n[1], n[2], n[3], n[4], 2); o.w = expand4(n[1], n[2], n[3], n[4], 3);
        s2[tid] = o;
        if (chunk == 0) {
            const size_t mo = (size_t)(tt % P.t_f) * P.n_envs + e;
            a[b] = P.act[mo];
            if (P.nstep > 1) fb_nstep_return(P, tt, e, r[b], t[b]);
            else { r[b] = P.rew[mo]; t[b] = P.term[mo]; }
        }
    }
}
