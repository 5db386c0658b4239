// fb_ac.hip -- advantage actor-critic (A2C) on the batched envs: the kernels of an FB_ARCH_AC net and the fb_ac_* entry points, as a code
// object of their own (fb_qnet.hip routes to the launchers below and gets no kernel: a kernel added to ITS code object moves the others).
// include/fbdqn.h pins the semantics.  Head parameters in the dueling layout, read raw: V = h . W_v + b_v, logits = h . W_pi + b_pi.
//   ac_head_kernel    acting: logits, V, the sampled (or greedy) action and its log-probability; one wave per state
//   ac_gae_kernel     the advantage scan; one thread per env, t = T-1 .. 0
//   ac_loss_kernel    training, launch 1 of 2: per sample logits / V, the loss terms, dz, dV, the dhf row and the activation row
//   ac_grad_kernel    training, launch 2 of 2: per 16 fc1 units the gradients of b_fc1, W_v, W_pi; workgroup 0: b_v, b_pi, the loss, Adam's tick
// and PPO on the same rollout (fb_qnet_ppo_train_step, fb_ppo_train_from_replay, fb_ac_normalize_adv, fb_ac_permute):
//   ppo_loss_kernel     ac_loss_kernel's place in the train step: the clipped-surrogate policy term, the (clipped) value term, two more loss terms
//   ac_adv_norm_kernel  the rollout's advantages to mean 0, standard deviation 1; ONE workgroup, float64, a pinned order
//   ac_permute_kernel   a stateless keyed permutation of [0, n): a Feistel network over Philox, cycle-walked; one thread per element
// and one PPO epoch as one host call (fb_ppo_epoch, fb_ppo_epoch_sum, fb_ac_normalize_adv_sel, fb_ac_grad_accumulate):
//   ac_adv_norm_sel_kernel  ac_adv_norm_kernel over the elements a selection names (one minibatch); ONE workgroup, the same pinned order
//   ac_grad_accum_kernel    acc = (first ? 0 : acc) + chunk over the flat gradient, float4 where aligned; workgroup 0 may add the chunk's six
//                           loss numbers to the minibatch's row, and to the epoch's running sum, in the same launch
//   ppo_epoch_mean_kernel   the epoch's six numbers: the minibatches' rows added in ascending order, divided by their count
// Behind them run fc1_bwd_big_kernel, the conv backward and Adam of fb_qnet.hip, unchanged.
#include "fb_common.h"
#include <math.h>

namespace {
#include "fb_head.h"
#include "fb_policy.h"

constexpr int AC_MAXB = 256;         // the train step's batch limit (fb_qnet.hip MAXTB)

template <int AT>
__global__ __launch_bounds__(256) void ac_head_kernel(AcHeadArgs H) {
    const int lane = threadIdx.x & 63, smp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (smp >= H.rows) return;                                   // (wave-uniform)
    const int A = AT == MAXA ? H.A : AT;
    float z[AT], V;
    row_head<AT, true, const NetOff &>(H.hf, H.stot, H.nks, H.FC, A, H.P, H.off, smp, lane, z, &V);
    if (lane != 0) return;
    H.value[smp] = V;
    if (H.logits) {
#pragma unroll
        for (int c = 0; c < AT; c++) if (c < A) H.logits[(size_t)smp * A + c] = z[c];
    }
    if (!H.actions) return;
    float p[AT], lp[AT], m, s;
    ac_softmax<AT>(z, A, p, lp, m, s);
    // The policy draw: greedy takes the first maximum; otherwise word x of Philox(seed, (smp, step) on FB_STREAM_POLICY) gives u and the
    // action is the first c with u < p_0 + .. + p_c, A - 1 when rounding leaves none; then logp of the action.  fb_sac.hip's sac_head_kernel
    // holds the same statements.  They are not one function: inlined from a header, these statements index lp[] through 8 KiB of LDS at
    // AT = MAXA, and a form that indexes nothing changed sac_head_kernel<2>'s instructions, whose step then could not be shown no slower
    int act = 0;
    if (H.greedy) {
#pragma unroll
        for (int c = 1; c < AT; c++) if (c < A && z[c] > z[act]) act = c;
    } else {
        const fb_u4 o = fb_philox(H.seed_lo, H.seed_hi, (uint32_t)smp, H.step_lo, FB_STREAM_POLICY, H.step_hi);
        const float u = (float)(o.x >> 8) * (1.0f / 16777216.0f);
        float cum = 0.f;
        bool found = false;
        act = A - 1;
#pragma unroll
        for (int c = 0; c < AT; c++) {
            cum += p[c];
            if (c < A && !found && u < cum) { act = c; found = true; }
        }
    }
    H.actions[smp] = (uint8_t)act;
    if (H.logp) {
        float l = lp[0];
#pragma unroll
        for (int c = 1; c < AT; c++) l = c == act ? lp[c] : l;
        H.logp[smp] = l;
    }
}

// ---- generalised advantage estimation, one thread per env: every load and store of a time slot is contiguous across the envs.
// Everything in double, in the order include/fbdqn.h pins (no contraction: the build has -ffp-contract=off).
__global__ __launch_bounds__(256) void ac_gae_kernel(const float *__restrict__ rew, const uint8_t *__restrict__ term, const float *__restrict__ val,
                                                     int T, int N, double gamma, double gl, float *__restrict__ adv, float *__restrict__ ret) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= N) return;
    double A = 0.0, vn = (double)val[(size_t)T * N + e];
    for (int t = T - 1; t >= 0; t--) {
        const size_t k = (size_t)t * N + e;
        const float rf = rew[k];
        const bool nd = term[k] == 0;
        const double v = (double)val[k];
        const double r = rf == 0.1f ? 0.1 : (double)rf;
        const double x = nd ? gamma * vn : 0.0;
        const double d = (r + x) - v;
        A = d + (nd ? gl * A : 0.0);
        adv[k] = (float)A;
        ret[k] = (float)(A + v);
        vn = v;
    }
}

// ---- training, launch 1 of 2: one wave per sample (c51_loss_kernel's grid).  dl[b][16]: dz_c at c < 8, dV at 8, the loss terms
// L_pi, L_v, H at 9 .. 11.  Every lane holds the same logits, so the softmax, the loss and dz need no further exchange; the dhf and xs rows
// are written four units per lane.
template <int AT>
__global__ __launch_bounds__(256) void ac_loss_kernel(AcLossArgs L) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;                                        // (wave-uniform)
    const int A = AT == MAXA ? L.A : AT, FC = L.FC;
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;  // (an action past the head reads the last one: stays in bounds)
    const float adv = L.adv[b], ret = L.ret[b];
    float z[AT], V, p[AT], lp[AT], m, s;
    row_head<AT, true, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.P, L.off, b, lane, z, &V);
    ac_softmax<AT>(z, A, p, lp, m, s);
    float H = 0.f, lpa = lp[0];
#pragma unroll
    for (int c = 0; c < AT; c++) { H -= c < A ? p[c] * lp[c] : 0.f; lpa = c == ab ? lp[c] : lpa; }
    const float dv = V - ret;
    float dz[AT];
#pragma unroll
    for (int c = 0; c < AT; c++)
        dz[c] = c < A ? (adv * (p[c] - (c == ab ? 1.f : 0.f)) + L.ce * p[c] * (lp[c] + H)) / L.nt : 0.f;
    const float dV = (2.f * L.cv * dv) / L.nt;
    float o = lane == 8 ? dV : lane == 9 ? -adv * lpa : lane == 10 ? dv * dv : lane == 11 ? H : 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) o = lane == c ? dz[c] : o;
    if (lane < 16) L.dl[(size_t)b * 16 + lane] = o;
    for (int j0 = 4 * lane; j0 < FC; j0 += 256) {
        float x4[4], w[4][AT], wv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int a = 0; a < AT; a++) w[e][a] = L.P[L.off.wq + (j0 + e) * A + (a < A ? a : 0)];
            wv[e] = L.P[L.off.wv + j0 + e];
        }
        ac_units4(L.hf, L.stot, L.nks, FC, L.P, L.off.bf1, b, j0, x4);
        float d4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float dh = dV * wv[e];
#pragma unroll
            for (int a = 0; a < AT; a++) dh = fmaf(dz[a], w[e][a], dh);      // (dz of a >= A is 0)
            d4[e] = x4[e] > 0.f ? dh : 0.f;
        }
        *reinterpret_cast<float4 *>(L.dhf + (size_t)b * FC + j0) = make_float4(d4[0], d4[1], d4[2], d4[3]);
        *reinterpret_cast<float4 *>(L.xs + (size_t)b * FC + j0) = make_float4(x4[0], x4[1], x4[2], x4[3]);
    }
}

// ---- PPO's loss (include/fbdqn.h), ac_loss_kernel's grid and outputs: dl[b][16] holds dz at 0 .. 7, dV at 8, L_pi / L_v / H at 9 .. 11
// and the two terms PPO adds, 1{r outside [1 - eps, 1 + eps]} at 12 and (r - 1) - log r at 13.  Every lane holds the same logits, so
// the ratio and both clips are wave-uniform arithmetic: no exchange.  SEL: the rollout's four buffers are read at sel[b] (one 8-byte
// load per wave) instead of at b -- a template argument, so that no load sits under a branch.
template <int AT, bool SEL>
__global__ __launch_bounds__(256) void ppo_loss_kernel(PpoLossArgs Q) {
    const AcLossArgs &L = Q.a;
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;                                        // (wave-uniform)
    const int A = AT == MAXA ? L.A : AT, FC = L.FC;
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;  // (an action past the head reads the last one: stays in bounds)
    const long long k = SEL ? Q.sel[b] : (long long)b;
    const float adv = L.adv[k], ret = L.ret[k], lpo = Q.logp_old[k], vo = Q.value_old[k];
    float z[AT], V, p[AT], lp[AT], m, s;
    row_head<AT, true, const NetOff &>(L.hf, L.stot, L.nks, FC, A, L.P, L.off, b, lane, z, &V);
    ac_softmax<AT>(z, A, p, lp, m, s);
    float H = 0.f, lpa = lp[0];
#pragma unroll
    for (int c = 0; c < AT; c++) { H -= c < A ? p[c] * lp[c] : 0.f; lpa = c == ab ? lp[c] : lpa; }
    const float lr = lpa - lpo, r = expf(lr), lo = 1.f - Q.eps, hi = 1.f + Q.eps;
    const float s1 = r * adv, s2 = fminf(fmaxf(r, lo), hi) * adv;
    const float lpi = -fminf(s1, s2), w = s1 <= s2 ? s1 : 0.f;   // (the clipped branch is flat in r: no gradient)
    const float e1 = V - ret, d = V - vo, q1 = e1 * e1;
    const bool plain = Q.vclip == 0.f || fabsf(d) <= Q.vclip;   // the exact unclipped branch: vo + d is never formed
    const float e2 = (vo + copysignf(Q.vclip, d)) - ret, q2 = e2 * e2;
    const float lv = plain ? q1 : fmaxf(q1, q2);
    const float dV = plain || q1 >= q2 ? (2.f * L.cv * e1) / L.nt : 0.f;
    float dz[AT];
#pragma unroll
    for (int c = 0; c < AT; c++)
        dz[c] = c < A ? (w * (p[c] - (c == ab ? 1.f : 0.f)) + L.ce * p[c] * (lp[c] + H)) / L.nt : 0.f;
    float o = lane == 8 ? dV : lane == 9 ? lpi : lane == 10 ? lv : lane == 11 ? H : lane == 12 ? (r < lo || r > hi ? 1.f : 0.f)
              : lane == 13 ? (r - 1.f) - lr : 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) o = lane == c ? dz[c] : o;
    if (lane < 16) L.dl[(size_t)b * 16 + lane] = o;
    for (int j0 = 4 * lane; j0 < FC; j0 += 256) {               // the dhf and activation rows, as ac_loss_kernel writes them
        float x4[4], wq[4][AT], wv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int a = 0; a < AT; a++) wq[e][a] = L.P[L.off.wq + (j0 + e) * A + (a < A ? a : 0)];
            wv[e] = L.P[L.off.wv + j0 + e];
        }
        ac_units4(L.hf, L.stot, L.nks, FC, L.P, L.off.bf1, b, j0, x4);
        float d4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float dh = dV * wv[e];
#pragma unroll
            for (int a = 0; a < AT; a++) dh = fmaf(dz[a], wq[e][a], dh);     // (dz of a >= A is 0)
            d4[e] = x4[e] > 0.f ? dh : 0.f;
        }
        *reinterpret_cast<float4 *>(L.dhf + (size_t)b * FC + j0) = make_float4(d4[0], d4[1], d4[2], d4[3]);
        *reinterpret_cast<float4 *>(L.xs + (size_t)b * FC + j0) = make_float4(x4[0], x4[1], x4[2], x4[3]);
    }
}

// ---- the rollout's advantages to mean 0 and standard deviation 1, in double, in the order include/fbdqn.h pins: ONE workgroup; thread t
// sums the elements i = t (mod 256) in ascending order, thread 0 adds the 256 partial sums in ascending t.  out may be adv: an element
// is read and written by the same thread, and the last read of a pass sits in front of a barrier.
__global__ __launch_bounds__(256) void ac_adv_norm_kernel(const float *adv, long long n, float *out) {
    __shared__ double part[256];
    __shared__ double stat[2];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (long long i = t; i < n; i += 256) acc += (double)adv[i];
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double S = 0.0;
        for (int q = 0; q < 256; q++) S += part[q];
        stat[0] = S / (double)n;
    }
    __syncthreads();
    const double mean = stat[0];
    acc = 0.0;
    for (long long i = t; i < n; i += 256) { const double d = (double)adv[i] - mean; acc += d * d; }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double S = 0.0;
        for (int q = 0; q < 256; q++) S += part[q];
        stat[1] = sqrt(S / (double)n);
    }
    __syncthreads();
    const double den = stat[1] + 1e-8;
    for (long long i = t; i < n; i += 256) out[i] = (float)(((double)adv[i] - mean) / den);
}

// ---- ac_adv_norm_kernel over a selection: element j of the sums is adv[sel[j]], and out is written at sel[j] only.  out is not adv (the
// host refuses it): a minibatch normalised in place would be normalised again in the next epoch.  sel holds distinct positions inside
// adv / out by the caller's contract (a slice of a permutation), as ppo_loss_kernel's sel.
__global__ __launch_bounds__(256) void ac_adv_norm_sel_kernel(const float *__restrict__ adv, const long long *__restrict__ sel, long long n,
                                                              float *__restrict__ out) {
    __shared__ double part[256];
    __shared__ double stat[2];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (long long j = t; j < n; j += 256) acc += (double)adv[sel[j]];
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double S = 0.0;
        for (int q = 0; q < 256; q++) S += part[q];
        stat[0] = S / (double)n;
    }
    __syncthreads();
    const double mean = stat[0];
    acc = 0.0;
    for (long long j = t; j < n; j += 256) { const double d = (double)adv[sel[j]] - mean; acc += d * d; }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double S = 0.0;
        for (int q = 0; q < 256; q++) S += part[q];
        stat[1] = sqrt(S / (double)n);
    }
    __syncthreads();
    const double den = stat[1] + 1e-8;
    for (long long j = t; j < n; j += 256) { const long long k = sel[j]; out[k] = (float)(((double)adv[k] - mean) / den); }
}

// ---- the sum of an update's chunk gradients: acc[i] = (first ? 0 : acc[i]) + chunk[i], one fp32 add per element (0.f + x on a first
// chunk: a -0 becomes +0, as zero_() and += give it).  V4: both pointers 16-byte aligned -- thread i takes float4 i of the n / 4 whole
// ones, the next n % 4 threads one tail element each; otherwise one element per thread.  row != NULL: workgroup 0 adds the chunk's six
// loss numbers to the minibatch's row under the same rule (fb_ppo_epoch), so that a chunk costs one launch here, not two; and to run, the
// epoch's running sum over ALL its chunks (first_run: the epoch's first chunk), which is what a loop that adds every chunk's numbers to
// one accumulator holds -- the rows' sum is another order of the same additions.
template <bool V4>
__global__ __launch_bounds__(256) void ac_grad_accum_kernel(float *__restrict__ acc, const float *__restrict__ chunk, long long n, int first,
                                                            float *__restrict__ row, float *__restrict__ run, int first_run,
                                                            const float *__restrict__ six) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (V4) {
        const long long n4 = n >> 2, k = 4 * n4 + (i - n4);
        if (i < n4) {
            const float4 c = reinterpret_cast<const float4 *>(chunk)[i];
            float4 a = reinterpret_cast<const float4 *>(acc)[i];
            if (first) a = make_float4(0.f, 0.f, 0.f, 0.f);
            reinterpret_cast<float4 *>(acc)[i] = make_float4(a.x + c.x, a.y + c.y, a.z + c.z, a.w + c.w);
        } else if (k < n) {
            acc[k] = (first ? 0.f : acc[k]) + chunk[k];
        }
    } else if (i < n) {
        acc[i] = (first ? 0.f : acc[i]) + chunk[i];
    }
    if (row && blockIdx.x == 0 && threadIdx.x < 6) {
        const float x = six[threadIdx.x];
        row[threadIdx.x] = (first ? 0.f : row[threadIdx.x]) + x;
        run[threadIdx.x] = (first_run ? 0.f : run[threadIdx.x]) + x;
    }
}

// ---- the epoch's six numbers: thread c adds rows[m][c] in ascending m from 0.f and divides by the count
__global__ __launch_bounds__(64) void ppo_epoch_mean_kernel(const float *__restrict__ rows, int minibatches, float *__restrict__ mean) {
    const int c = threadIdx.x;
    if (c >= 6) return;
    float s = 0.f;
    for (int m = 0; m < minibatches; m++) s += rows[m * 6 + c];
    mean[c] = s / (float)minibatches;
}

// ---- a keyed permutation of [0, n) without state: element i -> the cycle-walked image of i under a 4-round Feistel network on k = 2 half
// bits, (L, R) <- (R, L ^ (F_r(R) & mask)), F_r(R) = word r of Philox4x32-10(key = seed, counter = (R, draw_lo, FB_STREAM_PERM, draw_hi)).
// The network is a bijection of [0, 2^k), so walking it until the value is below n is a bijection of [0, n) (the walk of an i < n comes
// back to i at the latest); 2^k < 4 n: fewer than 4 walks on average.
__global__ __launch_bounds__(256) void ac_permute_kernel(long long n, uint32_t seed_lo, uint32_t seed_hi, uint32_t draw_lo, uint32_t draw_hi, int half,
                                                         long long *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t mask = (1u << half) - 1u;
    uint32_t x = (uint32_t)i;
    do {
        uint32_t Lh = x >> half, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const fb_u4 o = fb_philox(seed_lo, seed_hi, R, draw_lo, FB_STREAM_PERM, draw_hi);
            const uint32_t F = r == 0 ? o.x : r == 1 ? o.y : r == 2 ? o.z : o.w;
            const uint32_t nr = Lh ^ (F & mask);
            Lh = R; R = nr;
        }
        x = (Lh << half) | R;
    } while ((long long)x >= n);
    out[i] = (long long)x;
}

// ---- training, launch 2 of 2: one workgroup per 16 fc1 units (c51_grad_kernel's grid): b_fc1's gradient and the tile's maximum |dhf|
// (fc1_bwd_big_kernel's pre-scale), then thread (unit jl, column c) walks the samples in order: c < A is W_pi's column c, c = 8 is W_v.
// Workgroup 0 also sums b_pi, b_v and the loss terms the same way (nterms: A2C's three, or PPO's five), forms the loss numbers and ticks Adam.
// The prologue -- thread group bg sums dhf[b][j00 + jl] over b = bg, bg + 16, ..; the 16 partial sums are added in ascending bg into b_fc1's
// gradient; max |dhf| goes to gmax; one barrier, which also publishes dlt / xt -- stands in sac_grad_kernel and iqn_grad_kernel too,
// statement for statement.  As one shared function it kept every kernel's registers but moved instructions (one in this kernel, one in
// sac_grad_kernel, a few in iqn_grad_kernel), and step times within a microsecond of the parent's could not be shown to be no slower
// (profiles/device_helpers_family_times.txt).
__global__ __launch_bounds__(256) void ac_grad_kernel(AcGradArgs L) {
    __shared__ float dlt[AC_MAXB * 16];
    __shared__ float xt[AC_MAXB * 16];
    __shared__ float part[16][16];
    __shared__ float wmax[4];
    __shared__ float lsum[5];
    const int tid = threadIdx.x, B = L.B, FC = L.FC, A = L.A, j00 = blockIdx.x * 16;
    for (int k = tid; k < B * 16; k += 256) { dlt[k] = L.dl[k]; xt[k] = L.xs[(size_t)(k >> 4) * FC + j00 + (k & 15)]; }
    const int jl = tid & 15, bg = tid >> 4;
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
    const int c = bg, cc = c < A || c == 8 ? c : 0;              // (idle columns walk column 0 and store nothing)
    float acc = 0.f, gb = 0.f;
    for (int b = 0; b < B; b++) {
        const float w = dlt[b * 16 + cc];
        gb += w;
        acc = fmaf(xt[b * 16 + jl], w, acc);
    }
    if (c < A) L.grad[L.off.wq + (size_t)(j00 + jl) * A + c] = acc;
    if (c == 8) L.grad[L.off.wv + j00 + jl] = acc;
    if (blockIdx.x != 0) return;
    if (jl == 0 && c < A) L.grad[L.off.bq + c] = gb;
    if (jl == 0 && c == 8) L.grad[L.off.bv] = gb;
    if (jl == 1 && c >= 9 && c < 9 + L.nterms) {                 // (otherwise idle threads: the loss terms, samples in order)
        float t = 0.f;
        for (int b = 0; b < B; b++) t += dlt[b * 16 + c];
        lsum[c - 9] = t / L.nt;
    }
    __syncthreads();
    if (tid == 0) {
        L.loss[1] = lsum[0]; L.loss[2] = lsum[1]; L.loss[3] = lsum[2];
        L.loss[0] = (lsum[0] + L.cv * lsum[1]) - L.ce * lsum[2];
        if (L.nterms == 5) { L.loss[4] = lsum[3]; L.loss[5] = lsum[4]; }      // PPO: the clip fraction and the approximate KL
        adam_tick(L.adam, L.tick);
    }
}

}  // namespace

void fb_ac_launch_head(hipStream_t st, const AcHeadArgs &H) {
    with_actions(H.A, [&](auto a) { hipLaunchKernelGGL(ac_head_kernel<decltype(a)::value>, dim3((H.rows + 3) / 4), dim3(256), 0, st, H); });
}

void fb_ac_launch_loss(hipStream_t st, const AcLossArgs &L) {
    with_actions(L.A, [&](auto a) { hipLaunchKernelGGL(ac_loss_kernel<decltype(a)::value>, dim3((L.B + 3) / 4), dim3(256), 0, st, L); });
}

void fb_ac_launch_ppo_loss(hipStream_t st, const PpoLossArgs &Q) {
    const dim3 grid((Q.a.B + 3) / 4);
    with_actions(Q.a.A, [&](auto a) {
        if (Q.sel) hipLaunchKernelGGL((ppo_loss_kernel<decltype(a)::value, true>), grid, dim3(256), 0, st, Q);
        else hipLaunchKernelGGL((ppo_loss_kernel<decltype(a)::value, false>), grid, dim3(256), 0, st, Q);
    });
}

void fb_ac_launch_grad(hipStream_t st, const AcGradArgs &L) {
    hipLaunchKernelGGL(ac_grad_kernel, dim3(L.FC / 16), dim3(256), 0, st, L);
}

extern "C" int fb_ac_gae(const float *reward, const uint8_t *terminal, const float *value, int T, int N, double gamma, double lambda, float *adv,
                         float *ret, void *stream) {
    FB_REQUIRE(reward && terminal && value && adv && ret, "fb_ac_gae: NULL argument");
    FB_REQUIRE(T >= 1 && N >= 1 && ((long long)T + 1) * N < (1LL << 31), "fb_ac_gae: T = %d, N = %d out of range", T, N);
    FB_REQUIRE(isfinite(gamma) && gamma >= 0.0 && gamma <= 1.0, "fb_ac_gae: gamma must be in [0, 1] (got %g)", gamma);
    FB_REQUIRE(isfinite(lambda) && lambda >= 0.0 && lambda <= 1.0, "fb_ac_gae: lambda must be in [0, 1] (got %g)", lambda);
    hipLaunchKernelGGL(ac_gae_kernel, dim3((N + 255) / 256), dim3(256), 0, fb_stream(stream), reward, terminal, value, T, N, gamma, gamma * lambda, adv, ret);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

// what the two ring-fed AC training calls do between their NULL checks and their train step: the net's kind, the memory's (uniform, n-step
// 1), the batch and n_total, then the minibatch described in the ring (r / t go to the net's scratch rows)
static int ac_ring_src(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, int64_t n_total, uint8_t *a_out, FbRingSrc *ring, const char *who,
                       void *stream) {
    FB_REQUIRE(fb_qnet_is_ac(net), "%s: not an actor-critic net (fb_qnet_create_ac)", who);
    int rc = fb_check_uniform_n1(replay, who, "the rollout is read from a uniform memory only", "the rollout is read");
    if (rc == FB_OK) rc = fb_qnet_ac_check_train(net, batch, n_total, who);
    if (rc != FB_OK) return rc;
    float *r_scr; uint8_t *t_scr;
    fb_qnet_ac_scratch(net, &r_scr, &t_scr);
    return fb_ring_src_fresh(replay, net, batch, idx, a_out, r_scr, t_scr, ring, stream);
}

extern "C" int fb_ac_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *adv, const float *ret,
                                       int64_t n_total, uint8_t *a_out, float *loss, float *flat_grad, void *stream) {
    FB_REQUIRE(replay && net && idx && adv && ret && a_out && loss, "fb_ac_train_from_replay: NULL argument");
    FbRingSrc ring;
    const int rc = ac_ring_src(replay, net, batch, idx, n_total, a_out, &ring, "fb_ac_train_from_replay", stream);
    if (rc != FB_OK) return rc;
    return fb_qnet_ac_train_ring(net, batch, &ring, adv, ret, n_total, loss, flat_grad, stream);
}

extern "C" int fb_ppo_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const int64_t *sel, const float *adv,
                                        const float *ret, const float *logp_old, const float *value_old, int64_t n_total, uint8_t *a_out,
                                        float *loss, float *flat_grad, void *stream) {
    FB_REQUIRE(replay && net && idx && adv && ret && logp_old && value_old && a_out && loss, "fb_ppo_train_from_replay: NULL argument");
    FbRingSrc ring;
    const int rc = ac_ring_src(replay, net, batch, idx, n_total, a_out, &ring, "fb_ppo_train_from_replay", stream);
    if (rc != FB_OK) return rc;
    return fb_qnet_ppo_train_ring(net, batch, &ring, sel, adv, ret, logp_old, value_old, n_total, loss, flat_grad, stream);
}

extern "C" int fb_ac_normalize_adv(const float *adv, int64_t n, float *out, void *stream) {
    FB_REQUIRE(adv && out, "fb_ac_normalize_adv: NULL argument");
    FB_REQUIRE(n >= 1 && n < (1LL << 31), "fb_ac_normalize_adv: n = %lld out of range", (long long)n);
    hipLaunchKernelGGL(ac_adv_norm_kernel, dim3(1), dim3(256), 0, fb_stream(stream), adv, (long long)n, out);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_ac_normalize_adv_sel(const float *adv, const int64_t *sel, int64_t n, float *out, void *stream) {
    FB_REQUIRE(adv && sel && out, "fb_ac_normalize_adv_sel: NULL argument");
    FB_REQUIRE(out != adv, "fb_ac_normalize_adv_sel: out must not be adv (a minibatch normalised in place would be normalised again in the next epoch)");
    FB_REQUIRE(n >= 1 && n < (1LL << 31), "fb_ac_normalize_adv_sel: n = %lld out of range", (long long)n);
    hipLaunchKernelGGL(ac_adv_norm_sel_kernel, dim3(1), dim3(256), 0, fb_stream(stream), adv, reinterpret_cast<const long long *>(sel), (long long)n, out);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

// acc = (first ? 0 : acc) + chunk, and with row the same rule over the six loss numbers (fb_ppo_epoch's chunk)
static void launch_grad_accum(hipStream_t st, float *acc, const float *chunk, long long n, int first, float *row, float *run, int first_run,
                              const float *six) {
    if ((((uintptr_t)acc | (uintptr_t)chunk) & 15) == 0) {
        const long long threads = (n >> 2) + (n & 3);
        hipLaunchKernelGGL(ac_grad_accum_kernel<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, acc, chunk, n, first, row, run, first_run, six);
    } else {
        hipLaunchKernelGGL(ac_grad_accum_kernel<false>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, acc, chunk, n, first, row, run, first_run, six);
    }
}

extern "C" int fb_ac_grad_accumulate(float *acc, const float *chunk, int64_t n, int first, void *stream) {
    FB_REQUIRE(acc && chunk, "fb_ac_grad_accumulate: NULL argument");
    FB_REQUIRE(acc != chunk, "fb_ac_grad_accumulate: acc must not be chunk");
    FB_REQUIRE(n >= 1 && n < (1LL << 31), "fb_ac_grad_accumulate: n = %lld out of range", (long long)n);
    launch_grad_accum(fb_stream(stream), acc, chunk, (long long)n, first != 0, nullptr, nullptr, 0, nullptr);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

// One PPO epoch as the calls VecActorCritic composes, in their order, on `stream` (include/fbdqn.h).  Everything any of them refuses is
// refused here first, so that nothing is launched and no host-side state of the net moves before a refusal.  The chunk's six numbers
// land in epoch_mean, which the last launch then overwrites with the epoch's.
extern "C" int fb_ppo_epoch(fb_replay_t replay, fb_qnet_t net, int64_t n, int minibatches, const int64_t *pos, const int64_t *sel, const float *adv,
                            const float *ret, const float *logp_old, const float *value_old, int mb_adv_norm, float *adv_scratch, float *grad,
                            float *chunk_grad, uint8_t *a_out, float *loss_rows, float *epoch_mean, void *stream) {
    const char *who = "fb_ppo_epoch";
    FB_REQUIRE(replay && net && pos && sel && adv && ret && logp_old && value_old && grad && chunk_grad && a_out && loss_rows && epoch_mean,
               "fb_ppo_epoch: NULL argument");
    FB_REQUIRE(n >= 1 && n < (1LL << 31), "fb_ppo_epoch: n = %lld out of range", (long long)n);
    FB_REQUIRE(minibatches >= 1 && n % minibatches == 0, "fb_ppo_epoch: minibatches must be >= 1 and divide n = %lld (got %d)", (long long)n, minibatches);
    FB_REQUIRE(!mb_adv_norm || adv_scratch, "fb_ppo_epoch: mb_adv_norm needs adv_scratch (f32 of the rollout buffers' size)");
    FB_REQUIRE(!mb_adv_norm || adv_scratch != adv, "fb_ppo_epoch: adv_scratch must not be adv (a minibatch normalised in place would be normalised "
               "again in the next epoch)");
    FB_REQUIRE(grad != chunk_grad, "fb_ppo_epoch: grad must not be chunk_grad");
    FB_REQUIRE(fb_qnet_is_ac(net), "%s: not an actor-critic net (fb_qnet_create_ac)", who);
    int rc = fb_check_uniform_n1(replay, who, "the rollout is read from a uniform memory only", "the rollout is read");
    if (rc != FB_OK) return rc;
    const int64_t mb = n / minibatches;
    rc = fb_qnet_ac_check_train(net, (int)(mb < AC_MAXB ? mb : AC_MAXB), mb, who);
    if (rc != FB_OK) return rc;
    const bool clip = fb_qnet_max_grad_norm(net) > 0.f;
    FB_REQUIRE(!clip || ((uintptr_t)grad & 15) == 0, "fb_ppo_epoch: grad must be 16-byte aligned (the net clips it)");
    int64_t np = 0;
    rc = fb_qnet_num_params(net, &np);
    if (rc != FB_OK) return rc;
    hipStream_t st = fb_stream(stream);
    for (int m = 0; m < minibatches; m++) {
        const int64_t lo = (int64_t)m * mb;
        if (mb_adv_norm) {
            rc = fb_ac_normalize_adv_sel(adv, sel + lo, mb, adv_scratch, stream);
            if (rc != FB_OK) return rc;
        }
        for (int64_t k = lo; k < lo + mb; k += AC_MAXB) {
            const int b = (int)(lo + mb - k < AC_MAXB ? lo + mb - k : AC_MAXB);
            rc = fb_ppo_train_from_replay(replay, net, b, pos + k, sel + k, mb_adv_norm ? adv_scratch : adv, ret, logp_old, value_old, mb, a_out,
                                          epoch_mean, chunk_grad, stream);
            if (rc != FB_OK) return rc;
            launch_grad_accum(st, grad, chunk_grad, (long long)np, k == lo, loss_rows + (size_t)m * 6, fb_qnet_ppo_sum(net), k == 0, epoch_mean);
        }
        if (clip) {
            rc = fb_qnet_clip_grad(net, grad, stream);
            if (rc != FB_OK) return rc;
        }
        rc = fb_qnet_apply_adam(net, grad, stream);
        if (rc != FB_OK) return rc;
    }
    hipLaunchKernelGGL(ppo_epoch_mean_kernel, dim3(1), dim3(64), 0, st, loss_rows, minibatches, epoch_mean);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_ppo_epoch_sum(fb_qnet_t net, float *sum, void *stream) {
    FB_REQUIRE(net && sum, "fb_ppo_epoch_sum: NULL argument");
    FB_REQUIRE(fb_qnet_is_ac(net), "fb_ppo_epoch_sum: not an actor-critic net (fb_qnet_create_ac)");
    FB_CHECK_HIP(hipMemcpyAsync(sum, fb_qnet_ppo_sum(net), 6 * sizeof(float), hipMemcpyDeviceToDevice, fb_stream(stream)));
    return FB_OK;
}

extern "C" int fb_ac_permute(int64_t n, uint64_t seed, uint64_t draw, int64_t *out, void *stream) {
    FB_REQUIRE(out, "fb_ac_permute: NULL argument");
    FB_REQUIRE(n >= 1 && n < (1LL << 31), "fb_ac_permute: n = %lld out of range (1 <= n < 2^31)", (long long)n);
    int k = 2;
    while ((1LL << k) < n) k += 2;               // the smallest even bit count with 2^k >= n
    hipLaunchKernelGGL(ac_permute_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fb_stream(stream), (long long)n, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)draw, (uint32_t)(draw >> 32), k / 2, reinterpret_cast<long long *>(out));
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_ac_rollout_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_ac_rollout_buffers *b, int n_envs, uint64_t seed,
                                  uint64_t step, int slot, void *stream) {
    FB_REQUIRE(env && replay && net && b, "fb_ac_rollout_step: NULL handle");
    FB_REQUIRE(b->nib && b->actions && b->frame_bits && b->reward && b->terminal && b->score && b->value && b->logp, "fb_ac_rollout_step: NULL buffer");
    FB_REQUIRE(fb_qnet_is_ac(net), "fb_ac_rollout_step: not an actor-critic net (fb_qnet_create_ac)");
    FB_REQUIRE(!fb_replay_is_prioritized(replay), "fb_ac_rollout_step: the rollout is stored in a uniform memory only");
    int rc = fb_check_step_handles(env, replay, net, n_envs, "fb_ac_rollout_step");
    if (rc != FB_OK) return rc;
    FB_REQUIRE(slot >= 0 && slot < b->slots, "fb_ac_rollout_step: slot %d outside the buffers' %d rows", slot, b->slots);
    // (every argument check of the three calls below is made above -- handles, buffers, the net's kind and row count, the env counts --
    // so nothing is launched and no push is counted before a refusal)
    const size_t o = (size_t)slot * n_envs;
    rc = fb_qnet_act_policy_nib(net, b->nib, n_envs, seed, step, 0, b->actions, b->value + o, b->logp + o, nullptr, stream);
    if (rc != FB_OK) return rc;
    rc = fb_env_step(env, b->actions, nullptr, b->frame_bits, b->reward + o, b->terminal + o, b->score, stream);
    if (rc != FB_OK) return rc;
    return fb_replay_push(replay, nullptr, b->frame_bits, b->actions, b->reward + o, b->terminal + o, stream);
}
