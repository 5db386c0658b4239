// fb_sac.hip -- discrete soft actor-critic (SAC) on the replay ring: the kernels of an FB_ARCH_SAC net and the fb_sac_* entry points, as a
// code object of their own (fb_qnet.hip routes to the launchers below and gets no kernel: a kernel added to ITS code object moves the others).
// include/fbdqn.h pins the semantics.  Head parameters behind b_fc1, read raw: W_pi b_pi (the plain head's place), W_q1 b_q1, W_q2 b_q2;
// z = h . W_pi + b_pi, Q_i = h . W_qi + b_qi.
//   sac_head_kernel   acting / forward: logits, Q1, Q2, the soft state value, the sampled (or greedy) action and its log-probability; one wave per state
//   sac_loss_kernel   training, launch 1 of 2: per sample the soft target, both critic errors, the actor term, dz / dQ, the dhf row and the activation row.
//                     Its PW instantiations are the prioritized form: importance weights into the critic terms, the mean |critic error| out as the priority
//   sac_grad_kernel   training, launch 2 of 2: per 16 fc1 units the gradients of b_fc1, W_pi, W_q1, W_q2; workgroup 0: the head biases, the six
//                     loss numbers, Adam's tick and the temperature update
// Behind them run fc1_bwd_big_kernel, the conv backward and Adam of fb_qnet.hip, unchanged.
#include "fb_common.h"
#include <math.h>

namespace {
#include "fb_head.h"
#include "fb_policy.h"

constexpr int SAC_MAXB = 256;        // the train step's batch limit (fb_qnet.hip MAXTB)

// the soft state value sum_c p_c (min(Q1_c, Q2_c) - alpha log p_c), ascending c, float32
template <int AT>
__device__ __forceinline__ float sac_soft_value(const float (&p)[AT], const float (&lp)[AT], const float (&q1)[AT], const float (&q2)[AT], int A, float alpha) {
    float V = 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) V += c < A ? p[c] * (fminf(q1[c], q2[c]) - alpha * lp[c]) : 0.f;
    return V;
}

template <int AT>
__global__ __launch_bounds__(256) void sac_head_kernel(SacHeadArgs H) {
    const int lane = threadIdx.x & 63, smp = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (smp >= H.rows) return;                                   // (wave-uniform)
    const int A = AT == MAXA ? H.A : AT;
    const float alpha = expf(H.sw[0]);
    float z[AT], q1[AT], q2[AT];
    row_head<AT>(H.hf, H.stot, H.nks, H.FC, A, H.P, HeadOff{H.off.bf1, H.off.wq, H.off.bq}, smp, lane, z);
    const bool needq = H.value || H.q1 || H.q2;                  // (kernel-uniform)
#pragma unroll
    for (int c = 0; c < AT; c++) { q1[c] = 0.f; q2[c] = 0.f; }
    if (needq) {
        row_head<AT>(H.hf, H.stot, H.nks, H.FC, A, H.P, HeadOff{H.off.bf1, H.so.wq1, H.so.bq1}, smp, lane, q1);
        row_head<AT>(H.hf, H.stot, H.nks, H.FC, A, H.P, HeadOff{H.off.bf1, H.so.wq2, H.so.bq2}, smp, lane, q2);
    }
    if (lane != 0) return;
#pragma unroll
    for (int c = 0; c < AT; c++) if (c < A) {
        if (H.logits) H.logits[(size_t)smp * A + c] = z[c];
        if (H.q1) H.q1[(size_t)smp * A + c] = q1[c];
        if (H.q2) H.q2[(size_t)smp * A + c] = q2[c];
    }
    if (!H.actions && !H.value) return;
    float p[AT], lp[AT], m, s;
    ac_softmax<AT>(z, A, p, lp, m, s);
    if (H.value) H.value[smp] = sac_soft_value<AT>(p, lp, q1, q2, A, alpha);
    if (!H.actions) return;
    int act = 0;
    if (H.greedy) {                                              // first maximum
#pragma unroll
        for (int c = 1; c < AT; c++) if (c < A && z[c] > z[act]) act = c;
    } else {                                                     // the draw pinned for an actor-critic net (fb_ac.hip)
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

// ---- training, launch 1 of 2: one wave per sample.  Rows b / B + b / 2 B + b of the fc1 partial sums: s and s' through the online net, s'
// through the target net.  Every lane holds the same heads, so the target, both losses and the gradients need no further exchange.
// dl[b][16]: dz_c at c < 8, dQ1(s, a) at 8, dQ2(s, a) at 9, d1^2 / d2^2 / L_pi / H at 10 .. 13, the action at 14, the alpha used at 15.
// PW, the prioritized form (fb_qnet_sac_per_train_step; SacPerLossArgs): w_b = isw[b] is multiplied LAST into dQ1 / dQ2 and into slots 10 / 11
// -- the dhf row and both critics' gradients pick it up through dQ_i -- and abs_err[b] takes 0.5 (|d1| + |d2|), unweighted (the priority);
// dz, L_pi and H stay unweighted.  w = 1 leaves the bits of the uniform form.  w_b is loaded once the six heads are formed: nothing of it
// is live across them, and the load is wave-uniform.
template <int AT, bool PW>
__global__ __launch_bounds__(256) void sac_loss_kernel(std::conditional_t<PW, SacPerLossArgs, SacLossArgs> L) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;                                        // (wave-uniform)
    const int A = AT == MAXA ? L.A : AT, FC = L.FC, B = L.B;
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;  // (an action past the head reads the last one: stays in bounds)
    const float rf = L.rew[b];
    const bool tb = L.term[b] != 0;
    const float alpha = expf(L.sw[0]);
    float z[AT], q1[AT], q2[AT], p[AT], lp[AT], m, s;
    // s' first: the policy from the online net (row B + b), both critics from the target net (row 2 B + b)
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P0, HeadOff{L.off.bf1, L.off.wq, L.off.bq}, B + b, lane, z);
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P1, HeadOff{L.off.bf1, L.so.wq1, L.so.bq1}, 2 * B + b, lane, q1);
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P1, HeadOff{L.off.bf1, L.so.wq2, L.so.bq2}, 2 * B + b, lane, q2);
    ac_softmax<AT>(z, A, p, lp, m, s);
    const float Vn = sac_soft_value<AT>(p, lp, q1, q2, A, alpha);
    const double r = rf == 0.1f ? 0.1 : (double)rf;              // (the convention of every target here)
    const float y = (float)(tb ? r : r + L.gamma * (double)Vn);
    // s: all three heads of the online net
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P0, HeadOff{L.off.bf1, L.off.wq, L.off.bq}, b, lane, z);
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P0, HeadOff{L.off.bf1, L.so.wq1, L.so.bq1}, b, lane, q1);
    row_head<AT>(L.hf, L.stot, L.nks, FC, A, L.P0, HeadOff{L.off.bf1, L.so.wq2, L.so.bq2}, b, lane, q2);
    ac_softmax<AT>(z, A, p, lp, m, s);
    float q1a = q1[0], q2a = q2[0];
#pragma unroll
    for (int c = 1; c < AT; c++) { q1a = c == ab ? q1[c] : q1a; q2a = c == ab ? q2[c] : q2a; }
    const float Bf = (float)B, d1 = q1a - y, d2 = q2a - y;
    float dq1 = (2.f * d1) / Bf, dq2 = (2.f * d2) / Bf, wb = 1.f;
    if constexpr (PW) {
        wb = L.isw[b];
        dq1 *= wb; dq2 *= wb;
        if (lane == 0) L.abs_err[b] = 0.5f * (fabsf(d1) + fabsf(d2));
    }
    const auto weighted = [&](float v) { if constexpr (PW) return v * wb; else return v; };      // (the uniform form: the statement of before)
    float f[AT], Lpi = 0.f, H = 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) {
        f[c] = alpha * lp[c] - fminf(q1[c], q2[c]);              // (min Q is a constant of the actor term)
        Lpi += c < A ? p[c] * f[c] : 0.f;
        H -= c < A ? p[c] * lp[c] : 0.f;
    }
    float dz[AT];
#pragma unroll
    for (int c = 0; c < AT; c++) dz[c] = c < A ? (p[c] * (f[c] - Lpi)) / Bf : 0.f;
    float o = lane == 8 ? dq1 : lane == 9 ? dq2 : lane == 10 ? weighted(d1 * d1) : lane == 11 ? weighted(d2 * d2) : lane == 12 ? Lpi : lane == 13 ? H
              : lane == 14 ? (float)ab : alpha;
#pragma unroll
    for (int c = 0; c < AT; c++) o = lane == c ? dz[c] : o;
    if (lane < 16) L.dl[(size_t)b * 16 + lane] = o;
    if (lane == 0 && L.y_out) L.y_out[b] = y;
    for (int j0 = 4 * lane; j0 < FC; j0 += 256) {
        float x4[4], w[4][AT], w1[4], w2[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int a = 0; a < AT; a++) w[e][a] = L.P0[L.off.wq + (j0 + e) * A + (a < A ? a : 0)];
            w1[e] = L.P0[L.so.wq1 + (j0 + e) * A + ab];
            w2[e] = L.P0[L.so.wq2 + (j0 + e) * A + ab];
        }
        ac_units4(L.hf, L.stot, L.nks, FC, L.P0, L.off.bf1, b, j0, x4);
        float d4[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float dh = dq1 * w1[e];
            dh = fmaf(dq2, w2[e], dh);
#pragma unroll
            for (int a = 0; a < AT; a++) dh = fmaf(dz[a], w[e][a], dh);       // (dz of a >= A is 0)
            d4[e] = x4[e] > 0.f ? dh : 0.f;
        }
        *reinterpret_cast<float4 *>(L.dhf + (size_t)b * FC + j0) = make_float4(d4[0], d4[1], d4[2], d4[3]);
        *reinterpret_cast<float4 *>(L.xs + (size_t)b * FC + j0) = make_float4(x4[0], x4[1], x4[2], x4[3]);
    }
}

// ---- training, launch 2 of 2: one workgroup per 16 fc1 units (ac_grad_kernel's grid): b_fc1's gradient and the tile's maximum |dhf|
// (fc1_bwd_big_kernel's pre-scale), then thread (unit jl, column c) walks the samples in order, twice: first c < 8 is W_pi's column c and
// c >= 8 W_q1's column c - 8, then c < 8 is W_q2's column c.  A critic's column c takes sample b's dQ_i when a_b = c, else 0.
// Workgroup 0 also sums b_pi, b_q1, b_q2 and the four loss terms the same way, forms the six loss numbers, ticks Adam and -- when the step
// applies Adam itself and alpha_lr > 0 -- makes the temperature's own Adam step on log alpha (include/fbdqn.h), on one thread.
__global__ __launch_bounds__(256) void sac_grad_kernel(SacGradArgs L) {
    __shared__ float dlt[SAC_MAXB * 16];
    __shared__ float xt[SAC_MAXB * 16];
    __shared__ float part[16][16];
    __shared__ float wmax[4];
    __shared__ float lsum[4];
    const int tid = threadIdx.x, B = L.B, FC = L.FC, A = L.A, j00 = blockIdx.x * 16;
    for (int k = tid; k < B * 16; k += 256) { dlt[k] = L.dl[k]; xt[k] = L.xs[(size_t)(k >> 4) * FC + j00 + (k & 15)]; }
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
    const int c = bg, col = c & 7;
    const bool live = col < A;
    float acc = 0.f, gb = 0.f;
    if (c < 8) {                                                 // W_pi's column c (idle columns walk column 0 and store nothing)
        const int cc = live ? col : 0;
        for (int b = 0; b < B; b++) {
            const float w = dlt[b * 16 + cc];
            gb += w;
            acc = fmaf(xt[b * 16 + jl], w, acc);
        }
        if (live) L.grad[L.off.wq + (size_t)(j00 + jl) * A + col] = acc;
    } else {                                                     // W_q1's column c - 8
        for (int b = 0; b < B; b++) {
            const float w = (int)dlt[b * 16 + 14] == col ? dlt[b * 16 + 8] : 0.f;
            gb += w;
            acc = fmaf(xt[b * 16 + jl], w, acc);
        }
        if (live) L.grad[L.so.wq1 + (size_t)(j00 + jl) * A + col] = acc;
    }
    float acc2 = 0.f, gb2 = 0.f;
    if (c < 8) {                                                 // W_q2's column c
        for (int b = 0; b < B; b++) {
            const float w = (int)dlt[b * 16 + 14] == col ? dlt[b * 16 + 9] : 0.f;
            gb2 += w;
            acc2 = fmaf(xt[b * 16 + jl], w, acc2);
        }
        if (live) L.grad[L.so.wq2 + (size_t)(j00 + jl) * A + col] = acc2;
    }
    if (blockIdx.x != 0) return;
    if (jl == 0 && live) {
        if (c < 8) { L.grad[L.off.bq + col] = gb; L.grad[L.so.bq2 + col] = gb2; }
        else L.grad[L.so.bq1 + col] = gb;
    }
    if (jl == 1 && c >= 10 && c < 14) {                          // (otherwise idle threads: the loss terms, samples in order)
        float t = 0.f;
        for (int b = 0; b < B; b++) t += dlt[b * 16 + c];
        lsum[c - 10] = t / (float)B;
    }
    __syncthreads();
    if (tid == 0) {
        L.loss[1] = lsum[0]; L.loss[2] = lsum[1]; L.loss[3] = lsum[2]; L.loss[4] = lsum[3];
        L.loss[0] = (lsum[0] + lsum[1]) + lsum[2];
        L.loss[5] = dlt[15];                                     // the alpha the loss kernel used
        adam_tick(L.adam, L.tick);
        const FbAdamHead &ad = *L.adam;
        if (L.temp) {                                            // one element of the net's TF-style Adam on log alpha, its own beta powers
            float la = L.sw[0], mm = L.sw[1], vv = L.sw[2], p1 = L.sw[3], p2 = L.sw[4];
            const float g = lsum[3] - L.target_entropy;
            const float at = L.alpha_lr * sqrtf(1.f - p2) / (1.f - p1);
            p1 *= ad.b1; p2 *= ad.b2;
            mm += (g - mm) * (1.f - ad.b1); vv += (g * g - vv) * (1.f - ad.b2);
            la -= (mm * at) / (sqrtf(vv) + ad.eps);
            L.sw[0] = la; L.sw[1] = mm; L.sw[2] = vv; L.sw[3] = p1; L.sw[4] = p2;
        }
    }
}

}  // namespace

void fb_sac_launch_head(hipStream_t st, const SacHeadArgs &H) {
    with_actions(H.A, [&](auto a) { hipLaunchKernelGGL(sac_head_kernel<decltype(a)::value>, dim3((H.rows + 3) / 4), dim3(256), 0, st, H); });
}

void fb_sac_launch_loss(hipStream_t st, const SacLossArgs &L) {
    with_actions(L.A, [&](auto a) { hipLaunchKernelGGL((sac_loss_kernel<decltype(a)::value, false>), dim3((L.B + 3) / 4), dim3(256), 0, st, L); });
}

void fb_sac_launch_per_loss(hipStream_t st, const SacPerLossArgs &L) {
    with_actions(L.A, [&](auto a) { hipLaunchKernelGGL((sac_loss_kernel<decltype(a)::value, true>), dim3((L.B + 3) / 4), dim3(256), 0, st, L); });
}

void fb_sac_launch_grad(hipStream_t st, const SacGradArgs &L) {
    hipLaunchKernelGGL(sac_grad_kernel, dim3(L.FC / 16), dim3(256), 0, st, L);
}

// the memory of the two uniform ring-fed SAC calls: a uniform one at n-step 1
static int sac_check_memory(fb_replay_t replay, const char *who) {
    return fb_check_uniform_n1(replay, who, "SAC trains from a uniform memory only (prioritized replay is not offered)", "SAC reads it");
}
// ... and of the two prioritized ones: a prioritized one, at the n it was made with (fb_check_per_memory)
static int sac_per_check_memory(fb_replay_t replay, double gamma, int pushes_ahead, const char *who) {
    return fb_check_per_memory(replay, gamma, pushes_ahead, who, "fb_sac_train_from_replay / fb_sac_step");
}

// fb_sac_train_from_replay (isw / abs_err NULL) and fb_sac_per_train_from_replay (both set: the weights in, the priority out) behind their
// NULL-argument checks: the net, the memory of the call's kind, the train step's own checks, then the step on the ring
static int sac_train_from_replay(const char *who, fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *isw, uint8_t *a_out,
                                 float *r_out, uint8_t *t_out, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(fb_qnet_is_sac(net), "%s: not a SAC net (fb_qnet_create_sac)", who);
    int rc = isw ? sac_per_check_memory(replay, gamma, 0, who) : sac_check_memory(replay, who);
    if (rc != FB_OK) return rc;
    rc = fb_qnet_sac_check_train(net, batch, gamma, who);
    if (rc != FB_OK) return rc;
    FbRingSrc ring;
    rc = fb_ring_src_fresh(replay, net, batch, idx, a_out, r_out, t_out, &ring, stream);
    if (rc != FB_OK) return rc;
    return fb_qnet_sac_train_ring(net, batch, &ring, isw, fb_replay_bootstrap_gamma(replay, gamma), loss, abs_err, q_target, flat_grad, stream, who);
}

extern "C" int fb_sac_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, uint8_t *a_out, float *r_out, uint8_t *t_out,
                                        double gamma, float *loss, float *q_target, float *flat_grad, void *stream) {
    const char *who = "fb_sac_train_from_replay";
    FB_REQUIRE(replay && net && idx && a_out && r_out && t_out && loss, "%s: NULL argument", who);
    return sac_train_from_replay(who, replay, net, batch, idx, nullptr, a_out, r_out, t_out, gamma, loss, nullptr, q_target, flat_grad, stream);
}

extern "C" int fb_sac_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *isw, uint8_t *a_out, float *r_out,
                                            uint8_t *t_out, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    const char *who = "fb_sac_per_train_from_replay";
    FB_REQUIRE(replay && net && idx && a_out && r_out && t_out && loss, "%s: NULL argument", who);
    FB_REQUIRE(isw && abs_err, "%s: the prioritized step needs the importance weights (isw) and abs_err", who);
    return sac_train_from_replay(who, replay, net, batch, idx, isw, a_out, r_out, t_out, gamma, loss, abs_err, q_target, flat_grad, stream);
}

// fb_sac_step and fb_sac_per_step (fb_common.h, the fused steps): the checks, the policy's draw, the env step, the store and the train
// call, the soft target update
static int sac_step(const char *who, bool prioritized, fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch,
                    uint64_t seed, uint64_t step, int train, double gamma, float rho, void *stream) {
    int rc = fb_check_step_buffers(env, replay, net, b, train, prioritized, who);
    if (rc != FB_OK) return rc;
    FB_REQUIRE(fb_qnet_is_sac(net), "%s: not a SAC net (fb_qnet_create_sac)", who);
    // (a prioritized n-step memory samples after this step's push: it needs n pushes by then)
    rc = prioritized ? sac_per_check_memory(replay, gamma, train ? 1 : -1, who) : sac_check_memory(replay, who);
    if (rc == FB_OK) rc = fb_check_step_handles(env, replay, net, n_envs, who);
    if (rc == FB_OK) rc = fb_qnet_sac_check_train(net, batch, gamma, who);
    if (rc != FB_OK) return rc;
    FB_REQUIRE(rho >= 0.f && rho <= 1.f, "%s: rho must be in [0, 1] (0 = no target update; got %g)", who, (double)rho);
    rc = fb_qnet_act_policy_nib(net, b->nib, n_envs, seed, step, 0, b->actions, nullptr, nullptr, nullptr, stream);
    if (rc == FB_OK) rc = fb_env_step(env, b->actions, nullptr, b->frame_bits, b->reward, b->terminal, b->score, stream);
    if (rc == FB_OK) rc = fb_step_store_train(replay, b, batch, train, prioritized, stream, [&](const float *isw, float *abs_err) {
        return sac_train_from_replay(who, replay, net, batch, b->idx, isw, b->a, b->r, b->t, gamma, b->loss, abs_err, nullptr, b->flat_grad, stream);
    });
    return rc != FB_OK || rho <= 0.f ? rc : fb_qnet_soft_sync_target(net, rho, stream);
}

extern "C" int fb_sac_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch, uint64_t seed, uint64_t step,
                           int train, double gamma, float rho, void *stream) {
    return sac_step("fb_sac_step", false, env, replay, net, b, n_envs, batch, seed, step, train, gamma, rho, stream);
}

extern "C" int fb_sac_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch, uint64_t seed,
                               uint64_t step, int train, double gamma, float rho, void *stream) {
    return sac_step("fb_sac_per_step", true, env, replay, net, b, n_envs, batch, seed, step, train, gamma, rho, stream);
}
