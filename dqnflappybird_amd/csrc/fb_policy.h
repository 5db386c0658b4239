// Device helpers of the two policy-head code objects, fb_ac.hip (A2C / PPO) and fb_sac.hip (discrete SAC): the fc1 activations of four
// units and the pinned float32 softmax.  Included inside each of those translation units' anonymous namespace, behind fb_head.h.
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
