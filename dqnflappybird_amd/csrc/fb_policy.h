// Device helpers of the side code objects, fb_ac.hip (A2C / PPO), fb_sac.hip (discrete SAC) and fb_iqn.hip (IQN): the fc1 activations of
// four units, the pinned float32 softmax and the linear head of one state.  Included inside each of those translation units' anonymous
// namespace, behind fb_head.h.
#pragma once

// the fc1 activations of units j0 .. j0 + 3 of state smp from the partial sums hf[ks][stot][FC]: head_one_t's loads, sums and order
__device__ __forceinline__ void ac_units4(const float *__restrict__ hf, int stot, int nks, int FC, const float *__restrict__ P, int bf1, int smp, int j0,
                                          float (&x4)[4]) {
    float4 t[FC1_KS];
#pragma unroll
    for (int ks = 0; ks < FC1_KS; ks++)
        t[ks] = sel4(ks < nks, *reinterpret_cast<const float4 *>(hf + ((size_t)(ks < nks ? ks : 0) * stot + smp) * FC + j0));
    const float4 bv = *reinterpret_cast<const float4 *>(P + bf1 + j0);
    float4 v = t[0];
#pragma unroll
    for (int ks = 1; ks < FC1_KS; ks++) { v.x += t[ks].x; v.y += t[ks].y; v.z += t[ks].z; v.w += t[ks].w; }
    x4[0] = fmaxf(v.x + bv.x, 0.f); x4[1] = fmaxf(v.y + bv.y, 0.f); x4[2] = fmaxf(v.z + bv.z, 0.f); x4[3] = fmaxf(v.w + bv.w, 0.f);
}

// softmax of the A logits in float32, ascending c (include/fbdqn.h): p, log p, the maximum m and s = sum_c exp(z_c - m)
template <int AT>
__device__ __forceinline__ void ac_softmax(const float (&z)[AT], int A, float (&p)[AT], float (&lp)[AT], float &m, float &s) {
    m = z[0];
#pragma unroll
    for (int c = 1; c < AT; c++) m = c < A ? fmaxf(m, z[c]) : m;
    float e[AT];
    s = 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) { e[c] = c < A ? expf(z[c] - m) : 0.f; s += e[c]; }
    const float lse = m + logf(s);
#pragma unroll
    for (int c = 0; c < AT; c++) { p[c] = e[c] / s; lp[c] = z[c] - lse; }
}

// ONE linear head of state smp on every lane of the wave (xor butterfly: the same bits everywhere): out[c] = h . W[:, c] + b[c], W at
// off.wq, b at off.bq; VAL: also *V = h . w_v + b_v, the value column at off.wv / off.bv, walked beside the others.  OFF: how the caller hands the
// offsets over decides where the compiler reads them, and with that the registers of the AT = MAXA kernels -- fb_ac.hip and fb_iqn.hip
// name `const NetOff &` (read where used: the parent's streams), fb_sac.hip passes a HeadOff by value (read at the call, as its
// heads always were; by reference sac_head_kernel<8> takes 170 VGPRs for 123).  Formed exactly as head_one_t forms the
// plain head's outputs -- a lane takes 4 consecutive units per round, fmaf in unit order, then the butterfly, then the bias -- so over
// W_q / b_q (or a fold block) these are the very bits fb_qnet_forward returns.  The heads of a state are formed one after another (one
// weight tile live at a time: no spill at AT = MAXA).  No load under a branch: columns a >= A read column 0 and are never used.
struct HeadOff { int bf1, wq, bq; };
template <int AT, bool VAL = false, class OFF>
__device__ __forceinline__ void row_head(const float *__restrict__ hf, int stot, int nks, int FC, int A, const float *__restrict__ P, OFF off,
                                         int smp, int lane, float (&out)[AT], float *V = nullptr) {
    static_assert(std::is_same<OFF, const NetOff &>::value || std::is_same<OFF, HeadOff>::value, "name `const NetOff &`, or pass a HeadOff");
    constexpr int NA = VAL ? AT + 1 : AT;
    float acc[NA], bq[AT];
#pragma unroll
    for (int a = 0; a < NA; a++) acc[a] = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) bq[a] = P[off.bq + (a < A ? a : 0)];
    [[maybe_unused]] float bv = 0.f;
    if constexpr (VAL) bv = P[off.bv];
    for (int j0 = 4 * lane; j0 < FC; j0 += 256) {
        float x4[4], w[4][AT];
        [[maybe_unused]] float wv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int a = 0; a < AT; a++) w[e][a] = P[off.wq + (j0 + e) * A + (a < A ? a : 0)];
            if constexpr (VAL) wv[e] = P[off.wv + j0 + e];
        }
        ac_units4(hf, stot, nks, FC, P, off.bf1, smp, j0, x4);
#pragma unroll
        for (int e = 0; e < 4; e++) {
#pragma unroll
            for (int a = 0; a < AT; a++) acc[a] = fmaf(x4[e], w[e][a], acc[a]);
            if constexpr (VAL) acc[AT] = fmaf(x4[e], wv[e], acc[AT]);
        }
    }
#pragma unroll
    for (int a = 0; a < NA; a++)
        for (int o = 32; o > 0; o >>= 1) acc[a] += __shfl_xor(acc[a], o);
#pragma unroll
    for (int a = 0; a < AT; a++) out[a] = a < A ? acc[a] + bq[a] : 0.f;
    if constexpr (VAL) *V = acc[AT] + bv;
}
