// fb_iqn.hip -- implicit quantile networks (IQN) on the replay ring: the kernels of an FB_ARCH_IQN net and the fb_iqn_* entry points, as a
// code object of their own (fb_qnet.hip routes to the launchers below and gets no kernel: a kernel added to ITS code object moves the others).
// include/fbdqn.h pins the semantics.  Parameters behind b_fc1: W_q b_q (the plain head's place), then the embedding W_e[64][FC] b_e[FC];
// theta(tau)_a = b_q[a] + sum_k (h_k phi_k(tau)) W_q[k, a], phi_k = relu(b_e[k] + sum_j cos(pi j tau) W_e[j, k]).
//   iqn_fold_kernel   phibar over the acting grid and the fold block [b_fc1 | phibar * W_q | b_q] of one net: what every forward-only path reads
//   iqn_head_kernel   theta at the caller's tau (fb_qnet_forward_iqn); one workgroup per state
//   iqn_loss_kernel   training, launch 1 of 2: per sample a*, the target quantiles, theta, the pairwise quantile Huber loss, d theta, then the
//                     dhf row, the W_q-gradient row, the embedding's pre-activation gradients and the cosine rows; one workgroup per sample.
//                     Its PW instantiations are the prioritized form: importance weights in, the per-sample loss out as the priority; its MU
//                     instantiations form the Munchausen target (a soft policy over the target net's Qbar, no a*) in place of the hard one
//   iqn_grad_kernel   training, launch 2 of 2: per 16 fc1 units the gradients of b_fc1, W_q, W_e, b_e; workgroup 0: b_q, the loss, Adam's tick
// Behind them run fc1_bwd_big_kernel, the conv backward and Adam of fb_qnet.hip, unchanged.
// A dueling net (FB_ARCH_IQN_DUELING; the DU instantiations): W_v b_v W_a b_a where W_q b_q stood, read as the effective column
// We[k, a] = (W_v[k] + W_a[k, a]) - m_k, be[a] (iqn_eff), formed in place wherever W_q b_q is read; the fold block keeps the plain layout;
// the gradient kernel splits the column gradients into W_v / b_v (the thread group bg == 8) and W_a / b_a.  DU = false: the statements of before.
// A lane owns a unit k and keeps W_e[:, k] in 64 registers; the cosine rows sit in LDS and are read as broadcasts; phi is recomputed in the
// backward pass instead of stored.
#include "fb_common.h"
#include <math.h>

namespace {
#include "fb_head.h"
#include "fb_policy.h"

constexpr int IQN_MAXB = 256;        // the train step's batch limit (fb_qnet.hip MAXTB)
constexpr int IQN_E = FB_IQN_COS;    // cosines of the embedding
constexpr int IQN_MAXT = 64;         // most tau per state in any call

// c_j(tau): formed in double, rounded once (a float32 argument of up to 198 rad would cost 1e-5)
__device__ __forceinline__ float iqn_cos(int j, float tau) { return (float)cos(M_PI * (double)j * (double)tau); }
// the tau of a Philox word: exact in float32, strictly inside (0, 1)
__device__ __forceinline__ float iqn_tau_of(uint32_t w) { return (float)(2u * (w >> 9) + 1u) * (1.0f / 16777216.0f); }
__device__ __forceinline__ float iqn_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi, int b, int i, bool target) {
    const fb_u4 o = fb_philox(seed_lo, seed_hi, (uint32_t)(b * 64 + i), step_lo, FB_STREAM_TAU, step_hi);
    return iqn_tau_of(target ? o.y : o.x);
}

// the fc1 activation of unit k of state `row` from the partial sums hf[ks][stot][FC]: ac_units4's sums and order, one unit
__device__ __forceinline__ float iqn_unit(const float *__restrict__ hf, int stot, int nks, int FC, const float *__restrict__ P, int bf1, int row, int k) {
    float v = hf[(size_t)row * FC + k];
#pragma unroll
    for (int ks = 1; ks < FC1_KS; ks++) {
        const float t = hf[((size_t)(ks < nks ? ks : 0) * stot + row) * FC + k];
        v += ks < nks ? t : 0.f;
    }
    return fmaxf(v + P[bf1 + k], 0.f);
}

// a dueling net's effective entries of one row: out[a] = (v[0] + row[a]) - (sum_{c < A} row[c]) / (float)A, the sum over ascending c from 0.f
// (include/fbdqn.h pins it).  v / row: W_v[k] / W_a[k, :], or b_v / b_a.  A + 1 loads, none under a branch: c >= A reads column 0 (dropped)
template <int AT>
__device__ __forceinline__ void iqn_eff(const float *__restrict__ v, const float *__restrict__ row, int A, float (&out)[AT]) {
    float wa[AT], s = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) wa[a] = row[a < A ? a : 0];
#pragma unroll
    for (int a = 0; a < AT; a++) s += a < A ? wa[a] : 0.f;
    const float m = s / (float)A, wv = v[0];
#pragma unroll
    for (int a = 0; a < AT; a++) out[a] = (wv + wa[a]) - m;
}
// entry `col` (< A) of the same, without indexing the registers
template <int AT>
__device__ __forceinline__ float iqn_eff_col(const float *__restrict__ v, const float *__restrict__ row, int A, int col) {
    float e[AT];
    iqn_eff<AT>(v, row, A, e);
    float r = e[0];
#pragma unroll
    for (int a = 1; a < AT; a++) r = a == col ? e[a] : r;
    return r;
}

// Munchausen IQN (include/fbdqn.h), from the finished Qbar rows of the target net, qn = Qbar-(s', .) and qs = Qbar-(s, .), in fp32 over
// ascending c: the soft policy at s', pi_c = e_c / S' with e_c = expf((qn_c - m') / temp), and t_c = (qn_c - m') - temp logf(S') (= temp ln pi_c,
// never formed as a log of pi_c: finite when e_c underflows); the bonus alpha max((qs_a - m) - temp logf(S), l0) is mdqn_target's
// expression (fb_qnet.hip).  Entries c >= A are masked by selects (pi_c = 0, t_c = 0)
template <int AT>
__device__ __forceinline__ void iqn_mu_policy(const float (&qn)[AT], const float (&qs)[AT], int A, int a_b, float temp, float alpha, float clip,
                                              float (&pi)[AT], float (&tl)[AT], float &bonus) {
    float mn = qn[0], ms = qs[0], qa = qs[0];
#pragma unroll
    for (int c = 1; c < AT; c++) { mn = c < A ? fmaxf(mn, qn[c]) : mn; ms = c < A ? fmaxf(ms, qs[c]) : ms; qa = c == a_b ? qs[c] : qa; }
    float e[AT], sn = 0.f, ss = 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) { e[c] = c < A ? expf((qn[c] - mn) / temp) : 0.f; sn += e[c]; ss += c < A ? expf((qs[c] - ms) / temp) : 0.f; }
    const float ln = temp * logf(sn);
#pragma unroll
    for (int c = 0; c < AT; c++) { pi[c] = e[c] / sn; tl[c] = c < A ? (qn[c] - mn) - ln : 0.f; }
    bonus = alpha * fmaxf((qa - ms) - temp * logf(ss), clip);
}

// the cosine rows of the taus tq[0 .. M) into ct[M][64] (both LDS), by the whole workgroup; the caller synchronises
__device__ __forceinline__ void iqn_cos_rows(const float *tq, int M, float *ct, int tid, int nthreads) {
    for (int q = tid; q < M * IQN_E; q += nthreads) ct[q] = iqn_cos(q & 63, tq[q >> 6]);
}

// theta of state `row` at the M taus whose cosine rows are ct[M][64] (LDS), by a workgroup of 256: out[m * NC + c] (LDS) for the columns
// c < NC -- NC = 1: the one column `col`; else the columns 0 .. NC - 1 (c >= A: column 0, never read).  Thread t owns the units t, t + 256,
// ...: it holds W_e[:, k], forms pre (fmaf over ascending j from b_e[k]), g = h_k * relu(pre) and g * W_q[k, c]; a wave sums its 64 units
// by the xor butterfly and its lane 0 adds the rounds up in order in part[wave][m][c]; out = b_q[c] + (((p_0 + p_1) + p_2) + p_3).
// part: LDS, 4 * M * NC floats.  Ends behind a barrier: out is complete.  No load under a branch (a thread past FC reads unit 0, h = 0).
// DU: a dueling net (AT: its action template), We[k, c] / be[c] where W_q[k, c] / b_q[c] stand
// WHO: a tag that gives a second caller of one (NC, AT, DU) a function of its own; the code is the same (the Munchausen loss passes 1: with
// iqn_head_kernel's instantiation shared between two kernels, the compiler ordered two scalar instructions of the head kernel differently)
template <int NC, int AT, bool DU, int WHO = 0>
__device__ __forceinline__ void iqn_theta(const float *__restrict__ hf, int stot, int nks, int FC, int A, const float *__restrict__ P, const NetOff &off,
                                          const IqnOff &io, int row, int col, const float *ct, int M, float *part, float *out) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < 4 * M * NC; q += 256) part[q] = 0.f;
    __syncthreads();
    for (int k0 = 0; k0 < FC; k0 += 256) {
        const bool ok = k0 + tid < FC;
        const int k = ok ? k0 + tid : 0;
        float w[IQN_E], wq[NC];
#pragma unroll
        for (int j = 0; j < IQN_E; j++) w[j] = P[io.we + j * FC + k];
        if constexpr (DU) {
            if constexpr (NC == 1) wq[0] = iqn_eff_col<AT>(P + off.wv + k, P + off.wq + k * A, A, col);
            else { static_assert(NC == AT, "all columns"); iqn_eff<AT>(P + off.wv + k, P + off.wq + k * A, A, wq); }
        } else {
#pragma unroll
            for (int c = 0; c < NC; c++) wq[c] = P[off.wq + k * A + (NC == 1 ? col : (c < A ? c : 0))];
        }
        const float be = P[io.be + k], hk = iqn_unit(hf, stot, nks, FC, P, off.bf1, row, k), h = ok ? hk : 0.f;
        for (int m = 0; m < M; m++) {
            float pre = be;
#pragma unroll
            for (int j = 0; j < IQN_E; j++) pre = fmaf(ct[m * IQN_E + j], w[j], pre);
            const float g = h * fmaxf(pre, 0.f);
#pragma unroll
            for (int c = 0; c < NC; c++) {
                float v = g * wq[c];
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) part[(wave * M + m) * NC + c] += v;
            }
        }
    }
    __syncthreads();
    for (int q = tid; q < M * NC; q += 256) {
        const int c = q % NC;
        float bq;
        if constexpr (DU) bq = iqn_eff_col<AT>(P + off.bv, P + off.bq, A, NC == 1 ? col : (c < A ? c : 0));
        else bq = P[off.bq + (NC == 1 ? col : (c < A ? c : 0))];
        out[q] = bq + (((part[q] + part[M * NC + q]) + part[2 * M * NC + q]) + part[3 * M * NC + q]);
    }
    __syncthreads();
}

// ---- the fold of one net: 128 units per workgroup (FC % 128 == 0), a thread per unit
// DU: [b_fc1 | phibar_k * We[k, a] | be[a]], the same plain layout
// NZ, a noisy net (fb_qnet_create_iqn_noisy): phibar_k itself is left in F.pbar[k] as well, for the per-env head below.  NZ = false: the
// statements and the argument block of before
template <bool DU, bool NZ = false>
__global__ __launch_bounds__(128) void iqn_fold_kernel(std::conditional_t<NZ, IqnFoldNzArgs, IqnFoldArgs> F) {
    __shared__ float ct[IQN_MAXT * IQN_E];
    __shared__ float tq[IQN_MAXT];
    const int tid = threadIdx.x, k = blockIdx.x * 128 + tid, K = F.K, FC = F.FC, A = F.A;
    if (tid < K) tq[tid] = (float)((double)F.eta * (double)(2 * tid + 1) / (double)(2 * K));
    __syncthreads();
    iqn_cos_rows(tq, K, ct, tid, 128);
    __syncthreads();
    float w[IQN_E];
#pragma unroll
    for (int j = 0; j < IQN_E; j++) w[j] = F.P[F.io.we + j * FC + k];
    const float be = F.P[F.io.be + k], bf = F.P[F.off.bf1 + k];
    float bq;
    [[maybe_unused]] float we[MAXA];                              // (DU: the unit's effective row, every load issued up front: this launch is latency)
    if constexpr (DU) {
        iqn_eff<MAXA>(F.P + F.off.wv + k, F.P + F.off.wq + k * A, A, we);
        bq = iqn_eff_col<MAXA>(F.P + F.off.bv, F.P + F.off.bq, A, k < A ? k : 0);
    } else {
        bq = F.P[F.off.bq + (k < A ? k : 0)];
    }
    float sm = 0.f;
    for (int i = 0; i < K; i++) {
        float pre = be;
#pragma unroll
        for (int j = 0; j < IQN_E; j++) pre = fmaf(ct[i * IQN_E + j], w[j], pre);
        sm += fmaxf(pre, 0.f);
    }
    const float pb = sm / (float)K;
    if constexpr (NZ) F.pbar[k] = pb;
    F.fold[k] = bf;
    if constexpr (DU) {
#pragma unroll
        for (int a = 0; a < MAXA; a++)
            if (a < A) F.fold[FC + k * A + a] = pb * we[a];
    } else {
        for (int a = 0; a < A; a++) F.fold[FC + k * A + a] = pb * F.P[F.off.wq + k * A + a];
    }
    if (k < A) F.fold[FC + FC * A + k] = bq;
}

// ---- per-env acting noise on a noisy IQN net (fb_qnet_act_nib_env_noise, include/fbdqn.h): the scalar head of env e under ITS effective
// weights, from the fc1 stage's two sets of partial sums.  One wave per env, eight envs per workgroup (env_noise_head_kernel's pattern,
// fb_qnet.hip): the head's rows are the same for every env, so the workgroup stages the rows of 256 units -- the mu fold's, sigma's Q /
// advantage layer's, (dueling) sigma's V layer's, and phibar -- in LDS at a time, coalesced, and each wave runs its chains from there.
// Lane l owns the units 4 l .. 4 l + 3 of a stage, which is head_one_t's dealing (fb_head.h): the mu logit b_q[a] + sum_k h_k F[k, a] is
// formed with that function's sums, in its order, so that sigma = 0 gives fb_qnet_act_nib's bits.  h_k = relu((mu partials + b_k) +
// f(eo_k) (t_k + sigma_b_k)); the noise term of a layer, f(eo_a) (sum_k sigma_W[k, a] (h_k f(ei_k) phibar_k) + sigma_b[a]), is added
// behind the mu logit -- dueling: nV + nA_a - (1/A) sum_c nA_c.  Draw k of env e: fb_qnet.hip's env_noise_f, Philox(key = seed, counter =
// (e nz + k, step_lo, FB_STREAM_ENV_NOISE, step_hi)).  Plain stores, no atomics; no load under a branch (clamped addresses, masked values).
// A draw is Philox, a logarithm and a full-range cosine: unrolled twelve times per stage it cost 256 VGPRs and scratch at AT = 8.  So a
// thread forms its draws of a stage in ONE rolled loop and parks them in LDS words only it reads (dr: no barrier needed), and the FMA
// chains read them back
__device__ __forceinline__ float iqn_env_noise_f(uint32_t seed_lo, uint32_t seed_hi, uint32_t c0, uint32_t step_lo, uint32_t step_hi) {
    const fb_u4 r = fb_philox(seed_lo, seed_hi, c0, step_lo, FB_STREAM_ENV_NOISE, step_hi);
    const float u1 = ((r.x >> 8) + 1) * (1.0f / 16777216.0f), u2 = (r.y >> 8) * (1.0f / 16777216.0f);
    const float z = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    return copysignf(sqrtf(fabsf(z)), z);
}
constexpr int IEN_WAVES = 8, IEN_UC = 256;      // envs per workgroup; units per stage (one round of head_one_t)
template <int AT, bool DU>
__global__ __launch_bounds__(64 * IEN_WAVES) void iqn_env_noise_head_kernel(IqnEnvNoiseArgs H) {
    constexpr int T = 64 * IEN_WAVES, PER = (IEN_UC * AT + T - 1) / T;
    __shared__ __attribute__((aligned(16))) float lm[IEN_UC * AT];      // the mu fold's rows [unit][A]
    __shared__ __attribute__((aligned(16))) float ls[IEN_UC * AT];      // sigma's Q / advantage rows [unit][A]
    __shared__ float lv[DU ? IEN_UC : 1], lp[IEN_UC];                   // sigma's V row; phibar
    constexpr int ND = DU ? 12 : 8;                                     // a thread's parked draws: 2 or 3 kinds x 4 units
    __shared__ float dr[ND * T];
    const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.x * IEN_WAVES + (tid >> 6);
    const bool live = row < H.n;
    const int smp = live ? row : H.n - 1;                        // (a wave past n stages and waits with the others, stores nothing)
    const int A = AT == MAXA ? H.A : AT, FC = H.FC;
    const int key = H.key_of ? H.key_of[smp] : smp;
    const uint32_t base = (uint32_t)key * (uint32_t)H.nz;
    auto draw = [&](int k) { return iqn_env_noise_f(H.seed_lo, H.seed_hi, base + (uint32_t)k, H.step_lo, H.step_hi); };
    float acc[AT], ns[AT], nv = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) { acc[a] = 0.f; ns[a] = 0.f; }
    for (int k0 = 0; k0 < FC; k0 += IEN_UC) {
        const int cu = min(IEN_UC, FC - k0), cq = cu * A;          // this stage's units (FC % 128 == 0: 128 or 256) and row entries
        const float *__restrict__ gm = H.F + H.foff.wq + (size_t)k0 * A, *__restrict__ gs = H.sig + H.off.wq + (size_t)k0 * A;
        float tm[PER], ts[PER];
#pragma unroll
        for (int r = 0; r < PER; r++) { const int i = min(tid + r * T, cq - 1); tm[r] = gm[i]; ts[r] = gs[i]; }
        const int iu = min(tid, cu - 1);
        const float tp = H.pbar[k0 + iu], tv = DU ? H.sig[H.off.wv + k0 + iu] : 0.f;
        // this lane's four units: fc1's mu sum (head_one_t's), sigma's t sum, the two biases
        const bool ok = 4 * lane < cu;
        const int j0 = k0 + (ok ? 4 * lane : 0);
        float4 t[FC1_KS], tt[FC1_KS];
#pragma unroll
        for (int ks = 0; ks < FC1_KS; ks++) {
            t[ks] = sel4(ks < H.nks, *reinterpret_cast<const float4 *>(H.hf + ((size_t)(ks < H.nks ? ks : 0) * H.stot + smp) * FC + j0));
            tt[ks] = sel4(ks < H.nkt, *reinterpret_cast<const float4 *>(H.ht + ((size_t)(ks < H.nkt ? ks : 0) * H.stot + smp) * FC + j0));
        }
        const float4 bv = *reinterpret_cast<const float4 *>(H.F + H.foff.bf1 + j0);
        float sb[4];
#pragma unroll
        for (int e = 0; e < 4; e++) sb[e] = H.sig[H.off.bf1 + j0 + e];
        float4 v = t[0], u = tt[0];
#pragma unroll
        for (int ks = 1; ks < FC1_KS; ks++) {
            v.x += t[ks].x; v.y += t[ks].y; v.z += t[ks].z; v.w += t[ks].w;
            u.x += tt[ks].x; u.y += tt[ks].y; u.z += tt[ks].z; u.w += tt[ks].w;
        }
        const float pre[4] = {v.x + bv.x, v.y + bv.y, v.z + bv.z, v.w + bv.w}, tu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll 1
        for (int i = 0; i < ND; i++) {                 // f(eo) of fc1, f(ei) of the Q / advantage layer, (dueling) f(ei) of the V layer
            const int kind = i >> 2, off = kind == 0 ? H.e_fc1_out : kind == 1 ? H.e_q_in : H.e_v_in;
            dr[i * T + tid] = draw(off + j0 + (i & 3));
        }
        __syncthreads();                                          // (the previous stage's rows are no longer read)
#pragma unroll
        for (int r = 0; r < PER; r++) { const int i = tid + r * T; if (i < cq) { lm[i] = tm[r]; ls[i] = ts[r]; } }
        if (tid < cu) { lp[tid] = tp; if (DU) lv[tid] = tv; }
        __syncthreads();
        if (ok) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int kl = 4 * lane + e;
                const float x = fmaxf(pre[e] + dr[e * T + tid] * (tu[e] + sb[e]), 0.f);
                const float xp = x * lp[kl], xq = xp * dr[(4 + e) * T + tid];
#pragma unroll
                for (int a = 0; a < AT; a++) {
                    const int o = kl * A + (a < A ? a : 0);
                    acc[a] = fmaf(x, lm[o], acc[a]);              // (columns a >= A are never read)
                    ns[a] = fmaf(xq, ls[o], ns[a]);
                }
                if (DU) nv = fmaf(xp * dr[(8 + e) * T + tid], lv[kl], nv);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < AT; a++)
        for (int o = 32; o > 0; o >>= 1) { acc[a] += __shfl_xor(acc[a], o); ns[a] += __shfl_xor(ns[a], o); }
    if (DU) for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o);
    // f(eo) of the Q / advantage layer's columns, then of the V layer's one: ONE draw per lane -- lane a < AT column a's, lane AT the V
    // layer's (the lanes behind it repeat that one) -- handed round by shuffles
    const float dout = draw(lane < AT ? H.e_q_out + (lane < A ? lane : 0) : H.e_v_out);
    float qv[AT], nq[AT], mean = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) {
        const int c = a < A ? a : 0;
        qv[a] = a < A ? acc[a] + H.F[H.foff.bq + c] : 0.f;
        nq[a] = __shfl(dout, a) * (ns[a] + H.sig[H.off.bq + c]);
        if (a < A) mean += nq[a];
    }
    if (DU) {
        mean /= (float)A;
        const float vn = __shfl(dout, AT) * (nv + H.sig[H.off.bv]);
#pragma unroll
        for (int a = 0; a < AT; a++) qv[a] += (vn + nq[a]) - mean;
    } else {
#pragma unroll
        for (int a = 0; a < AT; a++) qv[a] += nq[a];
    }
    if (lane == 0 && live) {                                      // (head_one_t's)
#pragma unroll
        for (int a = 0; a < AT; a++) if (a < A) H.q[(size_t)smp * A + a] = qv[a];
        int best = 0;
#pragma unroll
        for (int a = 1; a < AT; a++) if (a < A && qv[a] > qv[best]) best = a;
        const fb_u4 o = fb_philox(H.seed_lo, H.seed_hi, (uint32_t)key, H.step_lo, H.stream, H.step_hi);
        const float u = (float)(o.x >> 8) * (1.0f / 16777216.0f);
        if (u <= H.epsilon) best = (int)(((unsigned long long)o.y * (unsigned)A) >> 32);
        H.actions[smp] = (uint8_t)best;
    }
}

// ---- fb_qnet_forward_iqn: one workgroup per state
template <int AT, bool DU>
__global__ __launch_bounds__(256) void iqn_head_kernel(IqnHeadArgs H) {
    __shared__ float ct[IQN_MAXT * IQN_E];
    __shared__ float part[4 * IQN_MAXT * AT];
    __shared__ float out[IQN_MAXT * AT];
    __shared__ float tq[IQN_MAXT];
    const int tid = threadIdx.x, row = blockIdx.x, M = H.M, A = AT == MAXA ? H.A : AT;
    const float t = H.tau[(size_t)row * M + (tid < M ? tid : 0)];
    if (tid < M) tq[tid] = t;
    __syncthreads();
    iqn_cos_rows(tq, M, ct, tid, 256);
    __syncthreads();
    iqn_theta<AT, AT, DU>(H.hf, H.stot, H.nks, H.FC, A, H.P, H.off, H.io, row, 0, ct, M, part, out);
    for (int q = tid; q < M * AT; q += 256) {
        const int m = q / AT, c = q - m * AT;
        if (c < A) H.theta[((size_t)row * M + m) * A + c] = out[q];
    }
}

// ---- training, launch 1 of 2: one workgroup per sample.  Rows b / B + b / 2 B + b of the fc1 partial sums: s and s' through the online
// net, s' through the target net.  dl[b][4]: the action read, sum_i d theta_i, l_b, 0.
// PW, the prioritized form (fb_qnet_iqn_per_train_step): w_b = isw[b] is multiplied into d theta_i LAST, dl[b][2] takes w_b l_b and
// abs_err[b] the unweighted l_b (the priority); w = 1 leaves the bits of the uniform form.
// DU, a dueling net: theta, T and the backward's column through We / be; a* over the fold with ITS offsets (L.foff, the plain layout's).
// MU, Munchausen IQN (include/fbdqn.h): no a*.  q' = Qbar-(s', .) and q = Qbar-(s, .) are the plain head over the TARGET net's fold at rows
// 2 B + b and L.srow0 + b; theta-(s', c; tau'_j) of EVERY column c comes from one all-columns iqn_theta (the bits of the one-column calls);
// thread j < N' forms V_j = sum_c pi_c (theta_cj - t_c) and T_j = (float)((R + bonus) + (done ? 0 : Gamma V_j)).  From theta of the online
// column on it is the code of the other instantiations.  MU = false: the statements of before
template <int AT, bool PW, bool DU, bool MU>
__global__ __launch_bounds__(256) void iqn_loss_kernel(IqnLossMuArgs L) {
    __shared__ float ct[2 * IQN_MAXT * IQN_E];                    // the cosine rows of tau (N of them), then of tau' (N')
    __shared__ float part[4 * IQN_MAXT * (MU ? AT : 1)];
    [[maybe_unused]] __shared__ float tall[MU ? IQN_MAXT * AT : 1];      // (MU: theta-(s', c; tau'_j) at [j * AT + c])
    __shared__ float tq[2 * IQN_MAXT];
    __shared__ float th[IQN_MAXT], tg[IQN_MAXT], dth[IQN_MAXT], rowl[IQN_MAXT];
    const int tid = threadIdx.x, lane = tid & 63, b = blockIdx.x;
    const int A = AT == MAXA ? L.A : AT, FC = L.FC, B = L.B, N = L.N, Np = L.Np;
    {   // tau_i at tid < N, tau'_j behind them: the caller's, or the draws of (seed, step).  No load under a branch: without the caller's array a valid word is read and dropped
        const bool nx = tid >= N;
        const int cnt = nx ? Np : N, i0 = nx ? tid - N : tid, i = i0 < cnt ? i0 : cnt - 1;
        const float *src = nx ? L.tau_next : L.tau;
        const float given = *(src ? src + (size_t)b * cnt + i : L.rew + b);
        const float drawn = iqn_draw(L.seed_lo, L.seed_hi, L.step_lo, L.step_hi, b, i, nx);
        if (tid < N + Np) tq[tid] = src ? given : drawn;
    }
    __syncthreads();
    iqn_cos_rows(tq, N + Np, ct, tid, 256);
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;   // (an action past the head reads the last one: stays in bounds)
    const float rf = L.rew[b];
    const bool done = L.term[b] != 0;
    [[maybe_unused]] float wb = 1.f;
    if constexpr (PW) wb = L.isw[b];
    // Qbar of a row: the shared row head over the fold L.F, whose layout is the plain one (a dueling net: ITS offsets, L.foff).  Written as
    // calls under `if constexpr`: behind a lambda the loss kernels' instructions were ordered differently
    if constexpr (MU) {
        // the two Qbar rows of the target net (every wave, every lane forms the same bits), then the soft policy at s' and the bonus at (s, a)
        float qn[AT], qs[AT];
        if constexpr (DU) {
            row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.foff, L.arow0 + b, lane, qn);
            row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.foff, L.srow0 + b, lane, qs);
        } else {
            row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.off, L.arow0 + b, lane, qn);
            row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.off, L.srow0 + b, lane, qs);
        }
        float pi[AT], tl[AT], bonus;
        iqn_mu_policy<AT>(qn, qs, A, ab, L.temp, L.alpha, L.clip_lo, pi, tl, bonus);
        __syncthreads();
        iqn_theta<AT, AT, DU, 1>(L.hf, L.stot, L.nks, FC, A, L.P1, L.off, L.io, 2 * B + b, 0, ct + N * IQN_E, Np, part, tall);
        const int j = tid < Np ? tid : 0;                         // (no load under a branch: a thread past N' reads row 0 and drops it)
        float V = 0.f;
#pragma unroll
        for (int c = 0; c < AT; c++) { const float p = pi[c] * (tall[j * AT + c] - tl[c]); V += c < A ? p : 0.f; }
        if (tid < Np) {
            const double r = (rf == 0.1f ? 0.1 : (double)rf) + (double)bonus;      // (the convention of every target here; the bonus on terminal samples too)
            const float T = (float)(done ? r : r + L.gamma * (double)V);
            tg[tid] = T;
            if (L.t_out) L.t_out[(size_t)b * Np + tid] = T;
        }
    } else {
        // a*: the first maximum of the plain head over the fold (every wave forms the same bits)
        float qa[AT];
        if constexpr (DU) row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.foff, L.arow0 + b, lane, qa);
        else row_head<AT, false, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.F, L.off, L.arow0 + b, lane, qa);
        int as = 0;
        float qbest = qa[0];
#pragma unroll
        for (int c = 1; c < AT; c++) { const bool up = c < A && qa[c] > qbest; as = up ? c : as; qbest = up ? qa[c] : qbest; }
        __syncthreads();
        iqn_theta<1, AT, DU>(L.hf, L.stot, L.nks, FC, A, L.P1, L.off, L.io, 2 * B + b, as, ct + N * IQN_E, Np, part, tg);
        if (tid < Np) {
            const double r = rf == 0.1f ? 0.1 : (double)rf;       // (the convention of every target here)
            const float T = (float)(done ? r : r + L.gamma * (double)tg[tid]);
            tg[tid] = T;
            if (L.t_out) L.t_out[(size_t)b * Np + tid] = T;
        }
    }
    iqn_theta<1, AT, DU>(L.hf, L.stot, L.nks, FC, A, L.P0, L.off, L.io, b, ab, ct, N, part, th);      // (its first barrier orders tg's stores too)
    if (tid < N) {                                                // the pairwise quantile Huber loss of row i, j ascending
        const float kap = L.kappa, ti = tq[tid], thi = th[tid];
        float l = 0.f, g = 0.f;
        for (int j = 0; j < Np; j++) {
            const float u = tg[j] - thi, au = fabsf(u), w = fabsf(ti - (u < 0.f ? 1.f : 0.f));
            const float hub = au <= kap ? 0.5f * u * u : kap * (au - 0.5f * kap);
            l += (w * hub) / kap;
            g += (w * fminf(fmaxf(u, -kap), kap)) / kap;
        }
        rowl[tid] = l;
        if constexpr (PW) dth[tid] = ((-(g / (float)Np)) / (float)B) * wb;
        else dth[tid] = (-(g / (float)Np)) / (float)B;
    }
    __syncthreads();
    if (tid == 0) {
        float l = 0.f, sd = 0.f;
        for (int i = 0; i < N; i++) { l += rowl[i]; sd += dth[i]; }
        if constexpr (PW) {
            const float lb = l / (float)Np;
            *reinterpret_cast<float4 *>(L.dl + (size_t)b * 4) = make_float4((float)ab, sd, wb * lb, 0.f);
            L.abs_err[b] = lb;
        } else {
            *reinterpret_cast<float4 *>(L.dl + (size_t)b * 4) = make_float4((float)ab, sd, l / (float)Np, 0.f);
        }
    }
    for (int q = tid; q < N * IQN_E; q += 256) L.ctab[(size_t)b * N * IQN_E + q] = ct[q];
    // backward: phi recomputed per unit; s_k = sum_i d theta_i phi_ik
    for (int k0 = 0; k0 < FC; k0 += 256) {
        const bool ok = k0 + tid < FC;
        const int k = ok ? k0 + tid : 0;
        float w[IQN_E];
#pragma unroll
        for (int j = 0; j < IQN_E; j++) w[j] = L.P0[L.io.we + j * FC + k];
        float wq;
        if constexpr (DU) wq = iqn_eff_col<AT>(L.P0 + L.off.wv + k, L.P0 + L.off.wq + k * A, A, ab);
        else wq = L.P0[L.off.wq + k * A + ab];
        const float be = L.P0[L.io.be + k], h = iqn_unit(L.hf, L.stot, L.nks, FC, L.P0, L.off.bf1, b, k);
        float s = 0.f;
        for (int i = 0; i < N; i++) {
            float pre = be;
#pragma unroll
            for (int j = 0; j < IQN_E; j++) pre = fmaf(ct[i * IQN_E + j], w[j], pre);
            const float d = dth[i];
            s = fmaf(d, fmaxf(pre, 0.f), s);
            if (ok) L.dpre[((size_t)b * N + i) * FC + k] = pre > 0.f ? (d * h) * wq : 0.f;
        }
        if (ok) {
            L.gw[(size_t)b * FC + k] = h * s;
            L.dhf[(size_t)b * FC + k] = h > 0.f ? wq * s : 0.f;
        }
    }
}

// ---- training, launch 2 of 2: one workgroup per 16 fc1 units (sac_grad_kernel's grid): b_fc1's gradient and the tile's maximum |dhf|
// (fc1_bwd_big_kernel's pre-scale); thread (unit jl, column c < 8) walks the samples in order for W_q's column c, which takes sample b's
// row when a_b = c, else 0; then thread (unit jl, cosines 4 g .. 4 g + 3) walks the rows (b, i) in order for W_e, the threads of g = 0
// for b_e as well.  Workgroup 0 also sums b_q and the loss the same way and ticks Adam.
// DU, a dueling net: with H_kc the column sum above and G_k = sum_b gw[b, k] (ascending b, walked beside it), dW_a[k, c] = H_kc - G_k / (float)A;
// the thread group bg == 8 (idle otherwise: A <= 8) walks G_k again for dW_v[k] = G_k; b_a / b_v the same way from dl[b][1]
template <bool DU>
__global__ __launch_bounds__(256) void iqn_grad_kernel(IqnGradArgs L) {
    __shared__ float dlt[IQN_MAXB * 4];
    __shared__ float xt[IQN_MAXB * 16];
    __shared__ float part[16][16];
    __shared__ float wmax[4];
    const int tid = threadIdx.x, B = L.B, FC = L.FC, A = L.A, j00 = blockIdx.x * 16;
    for (int k = tid; k < B * 4; k += 256) dlt[k] = L.dl[k];
    for (int k = tid; k < B * 16; k += 256) xt[k] = L.gw[(size_t)(k >> 4) * FC + j00 + (k & 15)];
    const int jl = tid & 15, bg = tid >> 4;
    // (the gradient tile's prologue: fb_ac.hip's ac_grad_kernel says why each gradient kernel carries these statements itself)
    float sm = 0.f, mx = 0.f;
    for (int b = bg; b < B; b += 16) { const float d = L.dhf[(size_t)b * FC + j00 + jl]; sm += d; mx = fmaxf(mx, fabsf(d)); }
    part[bg][jl] = sm;
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    if ((tid & 63) == 0) wmax[tid >> 6] = mx;
    __syncthreads();
    if (tid == 0) L.gmax[blockIdx.x] = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
    if (bg == 0) {
        float v = part[0][jl];
#pragma unroll
        for (int q = 1; q < 16; q++) v += part[q][jl];
        L.grad[L.off.bf1 + j00 + jl] = v;
    }
    const int c = bg;
    const bool live = c < A;                                      // (A <= 8: the columns sit in bg < 8)
    float acc = 0.f, gb = 0.f;
    [[maybe_unused]] float gk = 0.f, gs = 0.f;                   // (DU: G_k and sum_b dl[b][1])
    if (live) {
        for (int b = 0; b < B; b++) {
            const bool hit = (int)dlt[b * 4] == c;
            acc += hit ? xt[b * 16 + jl] : 0.f;
            gb += hit ? dlt[b * 4 + 1] : 0.f;
            if constexpr (DU) { gk += xt[b * 16 + jl]; gs += dlt[b * 4 + 1]; }
        }
        if constexpr (DU) L.grad[L.off.wq + (size_t)(j00 + jl) * A + c] = acc - gk / (float)A;
        else L.grad[L.off.wq + (size_t)(j00 + jl) * A + c] = acc;
    }
    if constexpr (DU) {
        if (bg == 8) {
            for (int b = 0; b < B; b++) { gk += xt[b * 16 + jl]; gs += dlt[b * 4 + 1]; }
            L.grad[L.off.wv + j00 + jl] = gk;
        }
    }
    {
        const int R = B * L.N;
        const float *dp = L.dpre + j00 + jl;
        const float4 *cp = reinterpret_cast<const float4 *>(L.ctab) + bg;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, be = 0.f;
#pragma unroll 8
        for (int r = 0; r < R; r++) {
            const float d = dp[(size_t)r * FC];
            const float4 cv = cp[(size_t)r * (IQN_E / 4)];
            a0 = fmaf(cv.x, d, a0); a1 = fmaf(cv.y, d, a1); a2 = fmaf(cv.z, d, a2); a3 = fmaf(cv.w, d, a3);
            be += d;
        }
        float *gwe = L.grad + L.io.we + (size_t)(bg * 4) * FC + j00 + jl;
        gwe[0] = a0; gwe[FC] = a1; gwe[2 * (size_t)FC] = a2; gwe[3 * (size_t)FC] = a3;
        if (bg == 0) L.grad[L.io.be + j00 + jl] = be;
    }
    if (blockIdx.x != 0) return;
    if constexpr (DU) {
        if (jl == 0 && live) L.grad[L.off.bq + c] = gb - gs / (float)A;
        if (jl == 0 && bg == 8) L.grad[L.off.bv] = gs;
    } else {
        if (jl == 0 && live) L.grad[L.off.bq + c] = gb;
    }
    if (tid == 0) {
        float t = 0.f;
        for (int b = 0; b < B; b++) t += dlt[b * 4 + 2];
        L.loss[0] = t / (float)B;
        FbAdamHead &ad = *L.adam;
        if (L.tick && ad.ticks == ad.applies) {                  // (adam_tick's statements, fb_head.h: called, it costs the DU kernel 2 VGPRs, 64 for 62)
            ad.alpha = ad.lr * sqrtf(1.f - ad.b2pow) / (1.f - ad.b1pow);
            ad.b1pow *= ad.b1; ad.b2pow *= ad.b2;
            ad.ticks += 1;
        }
    }
}

__global__ __launch_bounds__(256) void iqn_draw_kernel(long long total, int n, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo, uint32_t step_hi,
                                                       int which, float *out) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int b = (int)(q / n), i = (int)(q - (long long)b * n);
    out[q] = iqn_draw(seed_lo, seed_hi, step_lo, step_hi, b, i, which != 0);
}

// the loss launch of either kind of net (L.dueling), with the hard or the Munchausen target (L.mu), at the head's action template and the prioritized form
template <int AT, bool PW>
void launch_loss(hipStream_t st, const IqnLossMuArgs &L) {
    with_bool(L.dueling != 0, [&](auto du) { with_bool(L.mu != 0, [&](auto mu) {
        hipLaunchKernelGGL((iqn_loss_kernel<AT, PW, decltype(du)::value, decltype(mu)::value>), dim3(L.B), dim3(256), 0, st, L);
    }); });
}
}  // namespace

void fb_iqn_launch_fold(hipStream_t st, const IqnFoldArgs &F) {
    with_bool(F.dueling != 0, [&](auto du) { hipLaunchKernelGGL(iqn_fold_kernel<decltype(du)::value>, dim3(F.FC / 128), dim3(128), 0, st, F); });
}

void fb_iqn_launch_fold_noisy(hipStream_t st, const IqnFoldNzArgs &F) {
    with_bool(F.dueling != 0, [&](auto du) { hipLaunchKernelGGL((iqn_fold_kernel<decltype(du)::value, true>), dim3(F.FC / 128), dim3(128), 0, st, F); });
}

void fb_iqn_launch_env_noise_head(hipStream_t st, const IqnEnvNoiseArgs &H) {
    with_actions(H.A, [&](auto a) {
        with_bool(H.dueling != 0, [&](auto du) {
            hipLaunchKernelGGL((iqn_env_noise_head_kernel<decltype(a)::value, decltype(du)::value>), dim3((H.n + IEN_WAVES - 1) / IEN_WAVES), dim3(64 * IEN_WAVES),
                               0, st, H);
        });
    });
}

void fb_iqn_launch_head(hipStream_t st, const IqnHeadArgs &H) {
    with_actions(H.A, [&](auto a) {
        with_bool(H.dueling != 0, [&](auto du) {
            hipLaunchKernelGGL((iqn_head_kernel<decltype(a)::value, decltype(du)::value>), dim3(H.rows), dim3(256), 0, st, H);
        });
    });
}

void fb_iqn_launch_loss(hipStream_t st, const IqnLossMuArgs &L) {
    with_actions(L.A, [&](auto a) {           // (isw set: the prioritized form, which also writes abs_err)
        with_bool(L.isw != nullptr, [&](auto pw) {
            launch_loss<decltype(a)::value, decltype(pw)::value>(st, L);
        });
    });
}

void fb_iqn_launch_grad(hipStream_t st, const IqnGradArgs &L) {
    with_bool(L.dueling != 0, [&](auto du) { hipLaunchKernelGGL(iqn_grad_kernel<decltype(du)::value>, dim3(L.FC / 16), dim3(256), 0, st, L); });
}

extern "C" int fb_iqn_draw_taus(int batch, int n, uint64_t seed, uint64_t step, int which, float *tau_out, void *stream) {
    FB_REQUIRE(tau_out, "fb_iqn_draw_taus: tau_out is NULL");
    FB_REQUIRE(batch >= 1 && batch <= (1 << 20), "fb_iqn_draw_taus: batch %d outside 1..2^20", batch);
    FB_REQUIRE(n >= 1 && n <= IQN_MAXT, "fb_iqn_draw_taus: n %d outside 1..%d", n, IQN_MAXT);
    FB_REQUIRE(which == 0 || which == 1, "fb_iqn_draw_taus: which must be 0 (online) or 1 (target)");
    const long long total = (long long)batch * n;
    hipLaunchKernelGGL(iqn_draw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, fb_stream(stream), total, n, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)step, (uint32_t)(step >> 32), which, tau_out);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

// the checks of the two uniform ring-fed IQN calls on the memory: a uniform one, at any n-step view, whose gamma the caller's is
static int iqn_check_memory(fb_replay_t replay, double gamma, const char *who) {
    FB_REQUIRE(!fb_replay_is_prioritized(replay), "%s: IQN trains from a uniform memory only (prioritized replay is not offered)", who);
    return fb_replay_check_gamma(replay, gamma, who);
}
// ... and of the two prioritized ones: a prioritized one, at any n-step view (fb_check_per_memory)
static int iqn_per_check_memory(fb_replay_t replay, double gamma, int pushes_ahead, const char *who) {
    return fb_check_per_memory(replay, gamma, pushes_ahead, who, "fb_iqn_train_from_replay / fb_iqn_step");
}

// fb_iqn_train_from_replay (isw / abs_err NULL) and fb_iqn_per_train_from_replay (both set: the weights in, l_b out) behind their
// NULL-argument checks: the net, the memory of the call's kind, the train step's own checks, then the step on the ring
static int iqn_train_from_replay(const char *who, fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, const float *isw,
                                 uint8_t *a_out, float *r_out, uint8_t *t_out, const float *tau, const float *tau_next, uint64_t seed, uint64_t step,
                                 double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(fb_qnet_is_iqn(net), "%s: not an IQN net (fb_qnet_create_iqn)", who);
    int rc = isw ? iqn_per_check_memory(replay, gamma, 0, who) : iqn_check_memory(replay, gamma, who);
    if (rc != FB_OK) return rc;
    rc = fb_qnet_iqn_check_train(net, double_q, batch, gamma, who);
    if (rc != FB_OK) return rc;
    FbRingSrc ring;
    rc = fb_ring_src_fresh(replay, net, batch, idx, a_out, r_out, t_out, &ring, stream);
    if (rc != FB_OK) return rc;
    return fb_qnet_iqn_train_ring(net, double_q, batch, &ring, isw, tau, tau_next, seed, step, fb_replay_bootstrap_gamma(replay, gamma), loss, abs_err,
                                  q_target, flat_grad, stream, who);
}

extern "C" int fb_iqn_train_from_replay(fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, uint8_t *a_out, float *r_out,
                                        uint8_t *t_out, const float *tau, const float *tau_next, uint64_t seed, uint64_t step, double gamma, float *loss,
                                        float *q_target, float *flat_grad, void *stream) {
    const char *who = "fb_iqn_train_from_replay";
    FB_REQUIRE(replay && net && idx && a_out && r_out && t_out && loss, "%s: NULL argument", who);
    return iqn_train_from_replay(who, replay, net, double_q, batch, idx, nullptr, a_out, r_out, t_out, tau, tau_next, seed, step, gamma, loss, nullptr,
                                 q_target, flat_grad, stream);
}

extern "C" int fb_iqn_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, const float *isw,
                                            uint8_t *a_out, float *r_out, uint8_t *t_out, const float *tau, const float *tau_next, uint64_t seed,
                                            uint64_t step, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    const char *who = "fb_iqn_per_train_from_replay";
    FB_REQUIRE(replay && net && idx && a_out && r_out && t_out && loss, "%s: NULL argument", who);
    FB_REQUIRE(isw && abs_err, "%s: the prioritized step needs the importance weights (isw) and abs_err", who);
    return iqn_train_from_replay(who, replay, net, double_q, batch, idx, isw, a_out, r_out, t_out, tau, tau_next, seed, step, gamma, loss, abs_err,
                                 q_target, flat_grad, stream);
}

// fb_iqn_step and fb_iqn_per_step (fb_common.h, the fused steps): the checks, epsilon-greedy on the folded head, the env step, the store
// and the train call
static int iqn_step(const char *who, bool prioritized, fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q,
                    int batch, float epsilon, uint64_t seed, uint64_t step, int train, double gamma, void *stream) {
    int rc = fb_check_step_buffers(env, replay, net, b, train, prioritized, who);
    if (rc != FB_OK) return rc;
    FB_REQUIRE(fb_qnet_is_iqn(net), "%s: not an IQN net (fb_qnet_create_iqn)", who);
    // (a prioritized n-step memory samples after this step's push: it needs n pushes by then)
    rc = prioritized ? iqn_per_check_memory(replay, gamma, train ? 1 : -1, who) : iqn_check_memory(replay, gamma, who);
    if (rc == FB_OK) rc = fb_check_step_handles(env, replay, net, n_envs, who);
    if (rc == FB_OK) rc = fb_qnet_iqn_check_train(net, double_q, batch, gamma, who);
    // a noisy net (include/fbdqn.h, fb_vec_step's order).  Shared mode: the online net's sample of this step is drawn before acting, which
    // reads it through the fold.  Per-env mode: the acting forward draws per env from mu and sigma, and the online sample is drawn behind
    // the store (it also rebuilds what that forward left at mu).  The target net's sample is drawn in front of the train step
    const bool noisy = fb_qnet_is_noisy(net) != 0, env_noise = noisy && fb_qnet_acting_noise(net) == FB_ACT_NOISE_PER_ENV;
    if (rc == FB_OK && env_noise) rc = fb_qnet_check_env_noise(net, n_envs, who);
    if (rc != FB_OK) return rc;
    if (noisy && !env_noise) rc = fb_qnet_reset_noise(net, 0, seed, step, FB_NOISE_SAMPLE, stream);
    if (rc == FB_OK)
        rc = env_noise ? fb_qnet_act_nib_env_noise_keep(net, b->nib, n_envs, epsilon, seed, step, b->actions, nullptr, stream)
                       : fb_qnet_act_nib(net, b->nib, n_envs, epsilon, seed, step, b->actions, nullptr, stream);
    if (rc == FB_OK) rc = fb_env_step(env, b->actions, nullptr, b->frame_bits, b->reward, b->terminal, b->score, stream);
    if (rc != FB_OK) return rc;
    bool online_drawn = !env_noise;
    rc = fb_step_store_train(replay, b, batch, train, prioritized, stream, [&](const float *isw, float *abs_err) {
        int rn = FB_OK;
        if (env_noise) { rn = fb_qnet_reset_noise(net, 0, seed, step, FB_NOISE_SAMPLE, stream); online_drawn = true; }
        if (rn == FB_OK && noisy) rn = fb_qnet_reset_noise(net, 1, seed, step, FB_NOISE_SAMPLE, stream);
        if (rn != FB_OK) return rn;
        return iqn_train_from_replay(who, replay, net, double_q, batch, b->idx, isw, b->a, b->r, b->t, nullptr, nullptr, seed, step, gamma, b->loss, abs_err,
                                     nullptr, b->flat_grad, stream);
    });
    if (rc == FB_OK && !online_drawn) rc = fb_qnet_reset_noise(net, 0, seed, step, FB_NOISE_SAMPLE, stream);      // (a store-only step in the per-env mode)
    return rc;
}

extern "C" int fb_iqn_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q, int batch, float epsilon,
                           uint64_t seed, uint64_t step, int train, double gamma, void *stream) {
    return iqn_step("fb_iqn_step", false, env, replay, net, b, n_envs, double_q, batch, epsilon, seed, step, train, gamma, stream);
}

extern "C" int fb_iqn_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q, int batch,
                               float epsilon, uint64_t seed, uint64_t step, int train, double gamma, void *stream) {
    return iqn_step("fb_iqn_per_step", true, env, replay, net, b, n_envs, double_q, batch, epsilon, seed, step, train, gamma, stream);
}
