// fb_qnet.hip -- the DQN Q-network, its losses, backward pass and TF-style Adam on gfx950.
//
// Reference semantics (paths relative to the reference checkout):
//   network        BrainDQN.py:119-155  conv 8x8/4 SAME + relu -> max_pool 2x2/2 -> conv 4x4/2 SAME + relu
//                                       -> conv 3x3/1 SAME + relu -> NHWC flatten -> fc 1600xFC + relu -> fc FCxA
//   dueling head   BrainDuelingDQN.py:78-86
//   getAction      BrainDQN.py:99-116
//   targets/loss   BrainDQN.py:159-162,210-215; BrainDQNNature.py:118-119,164-175;
//                  BrainDoubleDQN.py:51-61; BrainPrioritizedReplyDQN.py:247-251
//   optimizer      BrainDQN.py:163 -> TF ApplyAdam (m += (g-m)(1-b1); v += (g*g-v)(1-b2);
//                  var -= m*alpha/(sqrt(v)+eps); alpha = lr*sqrt(1-b2^t)/(1-b1^t))
//
// Every layer is an implicit GEMM on the fp32-input matrix instruction v_mfma_f32_32x32x2_f32
// (exact fp32 FMA chain, same rate as the vector ALU but one wave per SIMD saturates it, which is
// what a batch of 32 needs).  One workgroup owns one 32x32 output tile; its waves split the
// reduction dimension and are summed through LDS in a fixed order, so every result is bit
// reproducible (no atomics anywhere).  DESIGN.md "Q-network kernels" has the tile tables.
#include <math.h>
#include <stdlib.h>
#include "fb_common.h"

// ablation switches of the small-batch fc1 kernels (tools/time_train.py against -DFK_ABL=n / -DBW_ABL=n builds; 0 = the product)
#ifndef FK_ABL
#define FK_ABL 0
#endif
#ifndef BW_ABL
#define BW_ABL 0
#endif

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int OFF_W1 = 0, OFF_B1 = 8192, OFF_W2 = 8224, OFF_B2 = 40992, OFF_W3 = 41056, OFF_B3 = 77920,
              OFF_WF1 = 77984;
constexpr int CONV_PARAMS = OFF_WF1;         // everything in front of W_fc1
#include "fb_head.h"               // MAXA, FC1_KS, sel4, head_one
#include "fb_sampler.h"            // the replay sampler can ride in the conv3 backward launch (fb_train_steps)
#include "fb_gather.h"             // the ring readers of the ring-fed train trunk
constexpr int MAXTB = 256;


struct Slice { const float *params; const uint8_t *states; int s_off, count; const uint16_t *w1s; int fshift; };    // fshift: ring-fed plans, 0 = s, 1 = s'
struct Slices { Slice s[3]; int rb; };    // rb: bf16 training (fb_qnet_set_train_dtype): GEMM operands are rounded to bf16

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// D layout of the 32x32 tile: lane -> column (lane & 31), register r -> row
__device__ __forceinline__ int drow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// body(r, row) for the 16 accumulator rows of this lane that exist (row < limit).  A whole tile takes the straight-line
// path: a guard per row would put every store (and the load feeding it) in its own basic block, and hipcc then waits
// vmcnt(0) before each one -- 16 serialised write round trips at the end of every kernel.
template <class F>
__device__ __forceinline__ void for_rows(int base, int limit, int lane, F body) {
    if (base + 32 <= limit) {
#pragma unroll
        for (int r = 0; r < 16; r++) body(r, base + drow(r, lane));
    } else {
#pragma unroll
        for (int r = 0; r < 16; r++) { const int row = base + drow(r, lane); if (row < limit) body(r, row); }
    }
}

// Sum the accumulators of the first NW waves of a workgroup (>= 8 waves) and run the epilogue, with the work dealt out:
// every contributing wave parks its 16 rows in LDS (red: NW * 16 * 64 floats), then wave k < 8 adds the NW partials
// of rows 2k and 2k + 1 -- in wave order w = 0, 1, .., the same chain of fp32 adds a single reducing wave would run, so
// the result is bit-identical -- and calls body(sum, r, base + drow(r)) for them.  Rows at or past `limit` are skipped
// (whole tiles take the unguarded path, see for_rows).  One wave used to do all 16 x (NW - 1) adds and all 16 stores while
// the others idled.
template <int NW, class F>
__device__ __forceinline__ void reduce_rows(const f32x16 &acc, float *red, int wave, int lane, int base, int limit, F body) {
    if (wave < NW) {
#pragma unroll
        for (int r = 0; r < 16; r++) red[(wave * 16 + r) * 64 + lane] = acc[r];
    }
    __syncthreads();
    if (wave >= 8) return;
    float v[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int r = 2 * wave + q;
        v[q] = red[r * 64 + lane];
#pragma unroll
        for (int w = 1; w < NW; w++) v[q] += red[(w * 16 + r) * 64 + lane];
    }
    if (base + 32 <= limit) {
#pragma unroll
        for (int q = 0; q < 2; q++) body(v[q], 2 * wave + q, base + drow(2 * wave + q, lane));
    } else {
#pragma unroll
        for (int q = 0; q < 2; q++) { const int row = base + drow(2 * wave + q, lane); if (row < limit) body(v[q], 2 * wave + q, row); }
    }
}

// Loads are never placed under a branch: hipcc waits vmcnt(0) at the join and the loads of one wave serialise into
// dependent round trips.  The caller passes a VALID address also for a padding lane; the value is zeroed by a select.
// pins a loaded value in a register where it stands: without it LLVM sinks a load into the (even wave-uniform) branch
// that uses it, which brings the vmcnt(0)-per-load behaviour back
__device__ __forceinline__ void keep(float &x) { asm volatile("" : "+v"(x)); }
// bf16 training: an operand as the nearest bf16 number (products of two such are exact in the fp32 accumulation)
__device__ __forceinline__ float rbf(float x, bool rb) { return rb ? (float)(__bf16)x : x; }
__device__ __forceinline__ void keep(int &x) { asm volatile("" : "+v"(x)); }

// ================================================================== forward
// ---- conv1 on the fp16 matrix cores, exactly.
// conv1's input is u8 (in practice 0 / 255): every u8 value is exact in fp16.  Each fp32 weight is carried as two fp16 numbers
// w = h + l / 4096 (split2x2 below), so sum_k x_k * w_k = sum_k x_k*h_k + (sum_k x_k*l_k) / 4096 with every product exact in the
// fp32 accumulation inside v_mfma_f32_32x32x16_f16 -- two matrix instructions per 16 k, and they leave the vector ALU free for the
// u8 -> fp16 conversion.  K = 256 = 8 ky x 2 chunks of 16 (4 pixels x 4 frames = 16 contiguous bytes).
// The split weights live in w1s[part][ky][kq][h][co][8] (fp16), refreshed whenever the parameters change.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ uint32_t f32_to_bf16_rn(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// x = hi + mid + lo exactly, each a bf16 (round to nearest even at every step)
__device__ __forceinline__ void split3(float x, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
    hi = f32_to_bf16_rn(x);
    const float r1 = x - __uint_as_float(hi << 16);
    mid = f32_to_bf16_rn(r1);
    lo = f32_to_bf16_rn(r1 - __uint_as_float(mid << 16));
}

// the same split for two values at once on the hardware converter (v_cvt_pk_bf16_f32, round to nearest even):
// each output word packs the two bf16 (x0 in the low half)
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split3x2(float x0, float x1, uint32_t &hi, uint32_t &mid, uint32_t &lo) {
    const f32x2 x = {x0, x1};
    const bf16x2 h = __builtin_convertvector(x, bf16x2);
    const f32x2 r1 = x - __builtin_convertvector(h, f32x2);
    const bf16x2 m = __builtin_convertvector(r1, bf16x2);
    const f32x2 r2 = r1 - __builtin_convertvector(m, f32x2);
    const bf16x2 l = __builtin_convertvector(r2, bf16x2);
    hi = __builtin_bit_cast(uint32_t, h); mid = __builtin_bit_cast(uint32_t, m); lo = __builtin_bit_cast(uint32_t, l);
}

// ---- fp32 as TWO fp16 numbers.  x = h + l / 4096 with h = fp16(x) and l = fp16((x - h) * 4096), both rounded to nearest:
// |x - h| <= 2^-12 |x| and the second rounding leaves 2^-12 of that, so the pair carries x to 2^-24 relative -- fp32's own
// precision (2 x 11 significand bits plus the two roundings' sign bits) -- FOR 2^-14 <= |x| < 65504, fp16's normal range; the
// scale keeps l in h's exponent range instead of fp16's subnormals.  (Gradient operands are brought into that range by an exact
// power-of-two pre-scale, see pow2_scale below.)  A product a * w is then ah*wh + (ah*wl + al*wh) / 4096 + (al*wl) / 2^24: every fp16 x fp16 product is
// exact in the MFMA's fp32 accumulator, the last term is below one fp32 rounding and is dropped.  THREE v_mfma_f32_32x32x16_f16
// per 16 k (one into the main accumulator, two into a second one that is folded in with an exact power-of-two scale at the end)
// replace the SIX bf16 products of the hi/mid/lo split this path used before (three bf16 planes, 8 bits each) at the same
// accuracy: half the matrix cycles, two operand planes instead of three.  (Range: |x| must stay below 65504, fp16's maximum;
// the reference network's activations are O(1..100).)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
constexpr float F16_LO_SCALE = 4096.f, F16_LO_UNSCALE = 1.f / 4096.f;
__device__ __forceinline__ void split2x2(float x0, float x1, uint32_t &hi, uint32_t &lo) {
    const f32x2 x = {x0, x1};
    const f16x2 h = __builtin_convertvector(x, f16x2);
    const f32x2 r = (x - __builtin_convertvector(h, f32x2)) * F16_LO_SCALE;
    const f16x2 l = __builtin_convertvector(r, f16x2);
    hi = __builtin_bit_cast(uint32_t, h); lo = __builtin_bit_cast(uint32_t, l);
}
__device__ __forceinline__ f32x16 mfma_h(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_b(uint4 a, uint4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
constexpr uint32_t F16_255 = 0x5BF8u;        // 255.0 as fp16 (a lit pixel)

// ---- range of the two-plane form, and the power-of-two pre-scale that keeps GRADIENT operands inside it.
// The 2^-24 above holds while |x| >= 2^-14 (6.1e-5), fp16's smallest normal number: below it h is subnormal, the pair degrades
// linearly towards an ABSOLUTE error floor of ~7e-12, and values above 65504 overflow.  Weights and activations of this network live
// well inside that range (and a weight below 6e-5 still only errs by 7e-12 absolute, 1e-9 of a typical weight).  Gradients do not:
// with the mean losses (/ B, PER also x isw) and the reference's sigma = 0.01 weights, dh3 / dh2 / dp1 are 1e-6 .. 1e-8 throughout a
// run.  Every gradient operand is therefore multiplied by an exact power of two S before the split -- chosen from the maximum
// magnitude of the operand block (one sample, or one group of 16 samples, or the whole dhf matrix), so that the maximum lands in
// [2^10, 2^11) -- and the accumulator is multiplied by 1 / S in the epilogue, next to F16_LO_UNSCALE: both exact, so the result is
// that of unscaled arithmetic with operands of full two-plane precision.  Elements more than 2^24 below their block's maximum lose
// precision progressively; they are below one fp32 rounding of the sums the maximum takes part in.
struct Pow2 { float s, inv; };
__device__ __forceinline__ Pow2 pow2_scale(float maxabs) {
    const int e = (int)((__float_as_uint(maxabs) >> 23) & 255u);      // biased exponent (0: zero / subnormal maximum)
    int sb = 264 - e;                                                  // 127 + (10 - (e - 127))
    sb = sb < 2 ? 2 : (sb > 252 ? 252 : sb);                           // S and 1 / S both normal fp32 numbers
    Pow2 r;
    r.s = __uint_as_float((uint32_t)sb << 23); r.inv = __uint_as_float((uint32_t)(254 - sb) << 23);
    return r;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
// maximum over the workgroup's first NW waves of a per-thread non-negative value: one LDS word per wave (sx[0 .. NW)), written here,
// read after the caller's barrier by wg_max_read
__device__ __forceinline__ void wg_max_write(float v, float *sx, int wave, int lane) {
    v = wave_max(v);
    if (lane == 0) sx[wave] = v;
}
template <int NW>
__device__ __forceinline__ float wg_max_read(const float *sx) {
    float m = sx[0];
#pragma unroll
    for (int w = 1; w < NW; w++) m = fmaxf(m, sx[w]);
    return m;
}

// ---- range guard of the two-plane form for ACTIVATIONS, which are split unscaled (a per-block scale like the gradients' would need the
// block's maximum before the producing epilogue can store): h = fp16(x) overflows from 65520 on, and l = fp16((x - h) * 4096) already
// from |x| >= 32768 on (half an ulp of h is 16 there, times 4096 = 65536).  The guaranteed range is therefore |x| < 32768 (FB_F16_RANGE).
// The reference network's activations are O(1 .. 100) with its sigma = 0.01 weights and stay far inside; a net loaded from outside
// (tf_bundle.py) need not.  TF's fp32 would carry on; this path would turn into inf / NaN -- or, worse, into a finite wrong number behind
// the next relu.  So every site that splits an activation notes |x| >= FB_F16_RANGE, and a wave that saw one bumps the net's overflow
// word (AdamDev::ovf): fb_qnet_overflow_count reports it, VecBrain / the Brain classes raise on it.  It is the only atomic in the
// library and sits on the failure path only.  bf16 (NS = 1, FB_DTYPE_BF16) has fp32's exponent range: no guard, and the way out.
constexpr float FB_F16_RANGE = 32768.f;
__device__ __forceinline__ bool out_of_f16_range(float a, float b, float c, float d) { return fmaxf(fmaxf(fabsf(a), fabsf(b)), fmaxf(fabsf(c), fabsf(d))) >= FB_F16_RANGE; }
// (call where every lane of the wave is active)
__device__ __forceinline__ void note_overflow(bool bad, unsigned *ctr) {
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && (threadIdx.x & 63) == 0 && ctr) atomicAdd(ctr, 1u);
}

// W_conv1 in that form: w1s[part][ky][kq][h][co][8] fp16, part 0 = h, part 1 = l (conv1's u8 input is exact in fp16, so conv1 needs
// only x*wh and x*wl: two MFMAs per 16 k)
__device__ __forceinline__ void split_w1(const float w, int idx /* flat index in W_conv1[8][8][4][32] */, uint16_t *__restrict__ w1s) {
    const int co = idx & 31, f = (idx >> 5) & 3, kx = (idx >> 7) & 7, ky = idx >> 10;
    const int kq = kx >> 2, h = (kx >> 1) & 1, j = (kx & 1) * 4 + f;
    const _Float16 hh = (_Float16)w;
    const _Float16 ll = (_Float16)((w - (float)hh) * F16_LO_SCALE);
    const size_t o = ((((size_t)ky * 2 + kq) * 2 + h) * 32 + co) * 8 + j;
    w1s[o] = __builtin_bit_cast(uint16_t, hh); w1s[8192 + o] = __builtin_bit_cast(uint16_t, ll);
}

// (runs whenever the host replaced a net's parameters: it also bumps that net's parameter version, see AdamDev)
__global__ void w1_split_kernel(const float *__restrict__ params, uint16_t *__restrict__ w1s, unsigned *__restrict__ pver) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < 8192) split_w1(params[OFF_W1 + idx], idx, w1s);
    if (idx == 0 && pver) *pver += 1;
}

// 8 bytes -> 8 fp16 (exact: every u8 value has <= 8 significant bits)
__device__ __forceinline__ uint4 u8x8_to_f16(uint2 v) {
    uint4 o;
    const f32x2 p0 = {(float)(v.x & 255u), (float)((v.x >> 8) & 255u)}, p1 = {(float)((v.x >> 16) & 255u), (float)(v.x >> 24)};
    const f32x2 p2 = {(float)(v.y & 255u), (float)((v.y >> 8) & 255u)}, p3 = {(float)((v.y >> 16) & 255u), (float)(v.y >> 24)};
    o.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(p0, f16x2)); o.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(p1, f16x2));
    o.z = __builtin_bit_cast(uint32_t, __builtin_convertvector(p2, f16x2)); o.w = __builtin_bit_cast(uint32_t, __builtin_convertvector(p3, f16x2));
    return o;
}
__device__ __forceinline__ uint4 nib_lut_entry(unsigned t) {   // byte t = 2 pixels x 4 frames (bit 4*px + f) -> the 8 k-values of one lane
    uint4 e;
    e.x = ((t >> 0) & 1u) * F16_255 | ((t >> 1) & 1u) * (F16_255 << 16);
    e.y = ((t >> 2) & 1u) * F16_255 | ((t >> 3) & 1u) * (F16_255 << 16);
    e.z = ((t >> 4) & 1u) * F16_255 | ((t >> 5) & 1u) * (F16_255 << 16);
    e.w = ((t >> 6) & 1u) * F16_255 | ((t >> 7) & 1u) * (F16_255 << 16);
    return e;
}

// conv1 8x8x4->32 stride 4 SAME(2,2) + bias + relu + max_pool 2x2; one wave per tile of 8 pooled pixels x 4
// window positions (the pool is a max over 4 accumulator registers of one lane), 32 fp16 MFMAs per tile.
// NIB = false: states are u8[n][80][80][4] (the reference's layout).  NIB = true (acting path): states are
// the env kernel's running "nibble state" (SAME-padded, FB_NIB_* in include/fbdqn.h): one byte = 2 horizontally adjacent pixels x the
// last 4 frames (bit 4*px + f), which is exactly the 8 k-values one lane feeds to one MFMA, so the whole
// bf16x8 operand comes out of a 256-entry LDS table with one ds_read_b128 -- no u8 -> bf16 conversion, and
// the 25.6 KB/env currentState expansion (its own launch before) disappears.
constexpr int WSP_W2 = 0, WSP_W3 = 64 * 3 * 64, WSP_WF1 = WSP_W3 + 72 * 3 * 64;     // uint4 offsets inside wsp

// Item space of the re-split: one item = 8 weights -> one 16-byte entry in each of the three planes.
//   [0, 4096)                W_conv2 forward   wsp[WSP_W2 ]: [k8 = (tap, ci / 8)][plane][co]          (k = tap * 32 + ci)
//   [4096, 8704)             W_conv3 forward   wsp[WSP_W3 ]: [k8 = (tap, ci / 8)][plane][co]
//   [8704, 8704 + 200 FC)    W_fc1             wsp[WSP_WF1]: [k8][plane][unit]
//   then 4608 + 4096 items   the conv weights TRANSPOSED for the data gradients (conv32_bx_kernel):
//                            wsp[W3T]: [tap * 8 + co / 8][plane][ci (64)], wsp[W2T]: [tap * 8 + co / 8][plane][ci (32)]   (8 consecutive co)
constexpr int IT_CONV = 64 * 64 + 72 * 64;
__host__ __device__ __forceinline__ int wsp_w3t(int FC) { return WSP_WF1 + (200 + 4) * 3 * FC; }      // (+ 4: fc1_sp_kernel over-reads a chunk)
__host__ __device__ __forceinline__ int wsp_w2t(int FC) { return wsp_w3t(FC) + 72 * 3 * 64; }
__host__ __device__ __forceinline__ int wsp_total(int FC) { return wsp_w2t(FC) + 128 * 3 * 32; }
__host__ __device__ __forceinline__ int wsplit_items(int FC) { return 2 * IT_CONV + 200 * FC; }
// item of the conv-only job (forward + transposed conv planes, no fc1): q in [0, 2 IT_CONV)
__device__ __forceinline__ int conv_item(int q, int FC) { return q < IT_CONV ? q : q + 200 * FC; }

// 8 weights -> the item's entry in each of the three planes (by value: an array filled in two branches becomes an alloca that hipcc
// "promotes" to LDS -- 36 KB of it in conv1_sp_kernel, which slowed that kernel from 18 to 30 us)
__device__ __forceinline__ void wsplit_store(uint4 *__restrict__ o, int pstride, float w0, float w1, float w2, float w3, float w4, float w5, float w6, float w7) {
    // plane 0: fp16 h, plane 1: fp16 l (split2x2), plane 2: the weight rounded to bf16 (bf16 mode, FB_DTYPE_BF16)
    uint4 hi, lo, bh;
    uint32_t m_, l_;
    split2x2(w0, w1, hi.x, lo.x); split2x2(w2, w3, hi.y, lo.y); split2x2(w4, w5, hi.z, lo.z); split2x2(w6, w7, hi.w, lo.w);
    split3x2(w0, w1, bh.x, m_, l_); split3x2(w2, w3, bh.y, m_, l_); split3x2(w4, w5, bh.z, m_, l_); split3x2(w6, w7, bh.w, m_, l_);
    o[0] = hi; o[pstride] = lo; o[2 * pstride] = bh;
}

__device__ __forceinline__ void wsplit_item(const float *__restrict__ params, uint4 *__restrict__ wsp, int FC, int id) {
    const int t0 = IT_CONV + 200 * FC;
    if (id < t0) {                                                       // k-strided gather: W[k8 * 8 + e][col]
        const float *W; uint4 *out; int N;
        if (id < 64 * 64) { W = params + OFF_W2; out = wsp + WSP_W2; N = 64; }
        else if (id < IT_CONV) { id -= 64 * 64; W = params + OFF_W3; out = wsp + WSP_W3; N = 64; }
        else { id -= IT_CONV; W = params + OFF_WF1; out = wsp + WSP_WF1; N = FC; }
        const int k8 = id / N, col = id - k8 * N;
        const float *c0 = W + (size_t)(k8 * 8) * N + col;
        wsplit_store(out + (size_t)k8 * 3 * N + col, N, c0[0], c0[(size_t)N], c0[(size_t)2 * N], c0[(size_t)3 * N], c0[(size_t)4 * N], c0[(size_t)5 * N],
                     c0[(size_t)6 * N], c0[(size_t)7 * N]);
    } else {                                                             // transposed: 8 consecutive co of one (tap, ci)
        id -= t0;
        if (id >= IT_CONV) return;
        const float *src; uint4 *o; int pstride;
        if (id < 72 * 64) { const int kk = id >> 6, ci = id & 63; src = params + OFF_W3 + ((kk >> 3) * 64 + ci) * 64 + (kk & 7) * 8; o = wsp + wsp_w3t(FC) + kk * 3 * 64 + ci; pstride = 64; }
        else { id -= 72 * 64; const int kk = id >> 5, ci = id & 31; src = params + OFF_W2 + ((kk >> 3) * 32 + ci) * 64 + (kk & 7) * 8; o = wsp + wsp_w2t(FC) + kk * 3 * 32 + ci; pstride = 32; }
        const float4 x = reinterpret_cast<const float4 *>(src)[0], y = reinterpret_cast<const float4 *>(src)[1];
        wsplit_store(o, pstride, x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w);
    }
}

// stand-alone re-split (the acting forward normally does it inside its conv1 launch): only when the versions differ
__global__ void wsplit_kernel(const float *__restrict__ params, uint4 *__restrict__ wsp, int FC, const unsigned *__restrict__ pver,
                              const unsigned *__restrict__ wver) {
    if (*pver == *wver) return;
    wsplit_item(params, wsp, FC, blockIdx.x * blockDim.x + threadIdx.x);
}

// (the launch also re-splits W_conv2 / W_conv3 of a net whose parameters changed since its planes were built -- conv23_t_kernel, the
// next launch, reads them -- a few items per thread in front of the tile work, decided on the device like conv1_sp_kernel does)
struct SplitJob { const float *params[2]; uint4 *wsp[2]; const unsigned *pver[2], *wverc[2]; int FC; };

template <bool NIB>
__global__ __launch_bounds__(256) void conv1_pool_kernel(Slices sl, float *__restrict__ p1, uint8_t *__restrict__ amax, SplitJob job) {
    __shared__ uint4 lut[NIB ? 256 : 1];
    if (blockIdx.z == 0) {
#pragma unroll
        for (int n = 0; n < 2; n++)
            if (job.pver[n] && *job.pver[n] != *job.wverc[n])
                for (int q = blockIdx.x * 256 + threadIdx.x; q < 2 * IT_CONV; q += gridDim.x * 256) wsplit_item(job.params[n], job.wsp[n], job.FC, conv_item(q, job.FC));
    }
    if (NIB) {
        lut[threadIdx.x] = nib_lut_entry(threadIdx.x);       // element j = 4*px + f  <->  bit j of the byte
        __syncthreads();
    }
    const Slice s = sl.s[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, i = lane & 31, j = lane & 31;
    const int npool = s.count * 100, tile = blockIdx.x * 4 + wave;
    if (tile * 8 >= npool) return;
    const int P = tile * 8 + (i >> 2), pos = i & 3;
    const int b = P / 100, rem = P - b * 100, py = rem / 10, px = rem - py * 10;
    const int oy = 2 * py + (pos >> 1), ox = 2 * px + (pos & 1);
    const int bs = P < npool ? b : 0;        // the last tile's pixels past the slice read state 0 (zeroed by the select), as conv1_sp_kernel's do: b = count lies past the caller's states
    const uint4 *WB = reinterpret_cast<const uint4 *>(s.w1s) + hl * 32 + j;      // [part][ky][kq][h][co] x 16 B
    f32x16 acc = {0}, acl = {0};
#pragma unroll 2
    for (int ky = 0; ky < 8; ky++) {
        const int iy = oy * 4 + ky - 2;
        const bool rowok = P < npool && iy >= 0 && iy < 80;
        const uint8_t *row = NIB ? s.states + (size_t)bs * FB_NIB_STRIDE + ((rowok ? iy : 0) + 2) * FB_NIB_PITCH + 4
                                 : s.states + (((size_t)bs * 80 + (rowok ? iy : 0)) * 80) * 4;
#pragma unroll
        for (int kq = 0; kq < 2; kq++) {
            const int ix = ox * 4 - 2 + 4 * kq + 2 * hl;         // even: the pixel pair is inside or outside together
            const bool ok = rowok && ix >= 0 && ix < 80;
            uint4 A;
            const int ixc = ok ? ix : 0;                         // a valid address for the padding taps too; zeroed by a select
            if (NIB) {
                const unsigned idx = row[ixc >> 1];
                A = lut[ok ? idx : 0u];                          // entry 0 = all zero = the SAME padding
            } else {
                const uint2 v = *reinterpret_cast<const uint2 *>(row + (size_t)ixc * 4);
                A = u8x8_to_f16(make_uint2(ok ? v.x : 0u, ok ? v.y : 0u));
            }
            acc = mfma_h(A, WB[((0 * 8 + ky) * 2 + kq) * 64], acc);
            acl = mfma_h(A, WB[((1 * 8 + ky) * 2 + kq) * 64], acl);
        }
    }
    const float bias = s.params[OFF_B1 + j];
#pragma unroll
    for (int r = 0; r < 16; r++) acc[r] = fmaf(acl[r], F16_LO_UNSCALE, acc[r]);      // x*wh + (x*wl) / 4096: exact scale, one rounding
#pragma unroll
    for (int g = 0; g < 4; g++) {
        float bv = fmaxf(acc[4 * g] + bias, 0.f);
        int best = 0;
#pragma unroll
        for (int q = 1; q < 4; q++) {
            const float v = fmaxf(acc[4 * g + q] + bias, 0.f);
            if (v > bv) { bv = v; best = q; }
        }
        const int Pp = tile * 8 + 2 * g + hl;
        if (Pp < npool) {
            const size_t o = ((size_t)s.s_off * 100 + Pp) * 32 + j;
            p1[o] = bv; amax[o] = (uint8_t)best;
        }
    }
}

// ---- two-plane fp16 path (>= 256 states: the acting path, and the forward part of large training batches).
// An fp32 value is carried as the two fp16 numbers h + l / 4096 described above (split2x2), so an fp32 product a*w is
// ah*wh + (ah*wl + al*wh) / 4096 (+ al*wl / 2^24, below one fp32 rounding, dropped): three v_mfma_f32_32x32x16_f16
// (3 x 32 cycles per 16 k), each product exact in the MFMA's fp32 accumulator, replace eight v_mfma_f32_32x32x2_f32
// (8 x 64 cycles) while leaving the vector ALU to the address arithmetic.  NS = 1: one bf16 plane (the bf16 mode).
// Activations travel between the layers as two fp16 planes (one bf16 plane in bf16 mode) [plane][row][channel]; the weights are
// re-split whenever the parameters changed: wsp[k/8][plane][N] x 8 halves (16 B).
// NS = 3: the fp32-equivalent path; NS = 1 uses the bf16 plane only = plain bf16 arithmetic.
// conv1 of that path on u8 states (the acting path's nibble states go through conv23_sp_kernel<., 5, true> instead).  The small-batch
// kernel's wave re-reads all 32 KB of split weights for every tile (400 MB of L1/L2 traffic at 1024 states); here a workgroup parks them
// in LDS once and its waves walk over tiles, the next tile's input bytes in flight while the current one is in the MFMAs.  The vector
// ALU is the scarce unit here (32 MFMAs per tile leave room for ~170 vector instructions): the 2x2 pool is a max over four registers of
// a lane, and a quad transpose hands every lane 4 consecutive channels of one pooled pixel for an 8-byte store per plane (512 B per
// wave, contiguous).
// One workgroup of 12 waves per CU (3 per SIMD, <= 168 VGPRs): one copy of the weights per CU, and 12800 tiles over
// 3072 waves leave every SIMD 12 or 13 tiles (640 workgroups of 4 waves left some CUs with 3 workgroups = 15 tiles
// per SIMD and others with 2).  When the step changed the parameters every thread first re-splits at most one
// 8-weight item of W_conv2 / W_conv3 / W_fc1 for the kernels that follow (wsplit_item) -- no launch of its own.
#ifndef FB_C1_WAVES
#define FB_C1_WAVES 12
#endif
constexpr int C1_WAVES = FB_C1_WAVES;
// 4 x 4 transpose inside every quad of lanes: lane l ends with v[c] = (lane c's v[l]).  Two butterfly stages (partners
// l ^ 1, then l ^ 2), 16 vector instructions.
__device__ __forceinline__ float dpp_x1(float v) { const int x = __float_as_int(v); return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false)); }
__device__ __forceinline__ float dpp_x2(float v) { const int x = __float_as_int(v); return __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false)); }
__device__ __forceinline__ void quad_transpose(float (&v)[4], int l) {
    const bool b0 = l & 1, b1 = l & 2;
    const float r01 = dpp_x1(b0 ? v[0] : v[1]), r23 = dpp_x1(b0 ? v[2] : v[3]);
    const float x0 = b0 ? r01 : v[0], x1 = b0 ? v[1] : r01, x2 = b0 ? r23 : v[2], x3 = b0 ? v[3] : r23;
    const float ra = dpp_x2(b1 ? x0 : x2), rb = dpp_x2(b1 ? x1 : x3);
    v[0] = b1 ? ra : x0; v[1] = b1 ? rb : x1; v[2] = b1 ? x2 : ra; v[3] = b1 ? x3 : rb;
}

// Training on >= 256 states runs its forward through these kernels too: `side` then names up to two further state blocks (the
// minibatch's s and s' are separate buffers: state b lives in block b / per) and the fp32 copies the backward pass reads -- the
// pooled activations and the position of each pool's maximum (first maximum, like conv1_pool_kernel).
struct C1Side { const uint8_t *st1, *st2; int per; float *p1; uint8_t *amax; };

__global__ __launch_bounds__(64 * C1_WAVES) void conv1_sp_kernel(Slice s, const uint8_t *__restrict__ zeros, uint16_t *__restrict__ p1s,
                                                                  size_t p1plane, int nsplit, uint4 *__restrict__ wsp, int FC,
                                                                  const unsigned *__restrict__ pver, const unsigned *__restrict__ wver, C1Side side,
                                                                  unsigned *__restrict__ ovf) {
    __shared__ uint4 wl[2 * 16 * 64];
    const int bid = blockIdx.x, nblk = gridDim.x;
    // this workgroup's weight copy goes out first, the re-split items' loads right behind it (one round trip, not two)
    // (named registers: as an array hipcc "promoted" the staging copy to LDS -- 36 KB more per workgroup and 18 -> 30 us)
    constexpr int WQ = 2 * 16 * 64, NT = 64 * C1_WAVES;
    static_assert(WQ <= 3 * NT, "three staging registers per thread cover the weight copy");
    const uint4 *w1g = reinterpret_cast<const uint4 *>(s.w1s);
    const int wq0 = threadIdx.x, wq1 = threadIdx.x + NT, wq2 = threadIdx.x + 2 * NT;
    const uint4 wc0 = w1g[wq0 < WQ ? wq0 : 0], wc1 = w1g[wq1 < WQ ? wq1 : 0], wc2 = w1g[wq2 < WQ ? wq2 : 0];
    // the parameters changed since wsp was split (decided here, on the device: a replayed hipGraph takes the same decision a
    // live call would); the conv2+conv3 launch that follows records the new version
    if (pver && *pver != *wver) {
        const int items = wsplit_items(FC);
        for (int id = blockIdx.x * (64 * C1_WAVES) + threadIdx.x; id < items; id += gridDim.x * (64 * C1_WAVES)) wsplit_item(s.params, wsp, FC, id);
    }
    if (wq0 < WQ) wl[wq0] = wc0;
    if (wq1 < WQ) wl[wq1] = wc1;
    if (wq2 < WQ) wl[wq2] = wc2;
    __syncthreads();
    typedef uint2 Raw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, j = lane & 31, pp = j >> 2, pos = j & 3;
    const int npool = s.count * 100, ntiles = (npool + 7) / 8, stride = nblk * C1_WAVES;
    const float bias = s.params[OFF_B1 + j];
    auto fetch = [&](int tile, Raw (&raw)[16]) {
        const int P0 = tile * 8 + pp, P = P0 < npool ? P0 : 0;       // rows past the end compute on state 0 and are not stored
        int b = P / 100;
        const int rem = P - b * 100, py = rem / 10, px = rem - py * 10;
        const int oy = 2 * py + (pos >> 1), ox = 2 * px + (pos & 1);
        const uint8_t *sbase = s.states;
        if (side.per) { const int blk = b / side.per; b -= blk * side.per; sbase = blk == 0 ? s.states : blk == 1 ? side.st1 : side.st2; }
#pragma unroll
        for (int ky = 0; ky < 8; ky++) {
            const int iy = oy * 4 + ky - 2;
            const bool rowok = P < npool && iy >= 0 && iy < 80;
            const uint8_t *row = sbase + (((size_t)b * 80 + (rowok ? iy : 0)) * 80) * 8 / 2;
#pragma unroll
            for (int kq = 0; kq < 2; kq++) {
                const int ix = ox * 4 - 2 + 4 * kq + 2 * hl;
                const bool ok = rowok && ix >= 0 && ix < 80;
                // padding taps read the zero page: no branch, so no vmcnt(0) at a join
                raw[ky * 2 + kq] = *reinterpret_cast<const uint2 *>(ok ? row + (size_t)ix * 4 : zeros);
            }
        }
    };
    // tile -> wave, wave-major: tile = wave * nblk + bid (+ k * stride).  12 800 tiles over 3 072 waves leave 512 waves a fifth tile; in
    // workgroup-major order those were all 12 waves of 43 workgroups (15 tiles on each of their SIMDs against 12 elsewhere: the launch
    // lasted as long as those CUs), now they are waves 0 and 1 of every workgroup (13 tiles on two SIMDs of every CU).
    int tile = wave * nblk + bid;
    if (tile >= ntiles) return;
    Raw cur[16], nxt[16];
    fetch(tile, cur);
    bool bad = false;
    for (; tile < ntiles; tile += stride) {
        if (tile + stride < ntiles) fetch(tile + stride, nxt);
        int z;                                   // opaque 0: keeps the 48 weight fragments in LDS (re-read per tile)
        asm volatile("s_mov_b32 %0, 0" : "=s"(z));      // instead of hoisted into 192 registers at one wave per SIMD
        const uint4 *wlz = wl + z;
        f32x16 acc = {0}, acl = {0};
#pragma unroll
        for (int c = 0; c < 16; c++) {
            const uint4 A = u8x8_to_f16(cur[c]);
            acc = mfma_h(A, wlz[(0 * 16 + c) * 64 + lane], acc);
            acl = mfma_h(A, wlz[(1 * 16 + c) * 64 + lane], acl);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) acc[r] = fmaf(acl[r], F16_LO_UNSCALE, acc[r]);
        // D[row = 4 * pixel + window position][col = channel]: register r of a lane is window position r & 3 of pooled pixel
        // 2 * (r >> 2) + hl for channel j, so the 2x2 max-pool is a max over 4 registers; relu(max + bias) (monotone, so equal
        // to the max of the relu'd values).  The quad transpose then gives lane l of quad q pixel 2 * l + hl, channels 4q..4q+3.
        float o4[4];
#pragma unroll
        for (int g = 0; g < 4; g++) o4[g] = fmaxf(fmaxf(fmaxf(acc[4 * g], acc[4 * g + 1]), fmaxf(acc[4 * g + 2], acc[4 * g + 3])) + bias, 0.f);
        float am4[4] = {0.f, 0.f, 0.f, 0.f};
        if (side.amax) {                             // argmax of relu(x + bias) over the window, first maximum (conv1_pool_kernel's rule)
#pragma unroll
            for (int g = 0; g < 4; g++) {
                float bv = fmaxf(acc[4 * g] + bias, 0.f);
                int best = 0;
#pragma unroll
                for (int q = 1; q < 4; q++) { const float v = fmaxf(acc[4 * g + q] + bias, 0.f); if (v > bv) { bv = v; best = q; } }
                am4[g] = __int_as_float(best);
            }
            quad_transpose(am4, j & 3);
        }
        quad_transpose(o4, j & 3);
        const int Pp = tile * 8 + 2 * (j & 3) + hl;
        if (side.p1 && Pp < npool) {
            const size_t so = ((size_t)s.s_off * 100 + Pp) * 32 + 4 * (j >> 2);
            *reinterpret_cast<float4 *>(side.p1 + so) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            *reinterpret_cast<uint32_t *>(side.amax + so) = (uint32_t)__float_as_int(am4[0]) | (uint32_t)__float_as_int(am4[1]) << 8 |
                                                             (uint32_t)__float_as_int(am4[2]) << 16 | (uint32_t)__float_as_int(am4[3]) << 24;
        }
        uint32_t hi[2], lo[2], m_, l_;
        if (nsplit == 3) { split2x2(o4[0], o4[1], hi[0], lo[0]); split2x2(o4[2], o4[3], hi[1], lo[1]); bad |= out_of_f16_range(o4[0], o4[1], o4[2], o4[3]); }      // fp16 h / l planes
        else { split3x2(o4[0], o4[1], hi[0], m_, l_); split3x2(o4[2], o4[3], hi[1], m_, l_); lo[0] = lo[1] = 0u; }     // one bf16 plane
        if (Pp < npool) {
            uint16_t *o = p1s + ((size_t)s.s_off * 100 + Pp) * 32 + 4 * (j >> 2);
            *reinterpret_cast<uint2 *>(o) = make_uint2(hi[0], hi[1]);
            if (nsplit == 3) *reinterpret_cast<uint2 *>(o + p1plane) = make_uint2(lo[0], lo[1]);
        }
#pragma unroll
        for (int q = 0; q < 16; q++) cur[q] = nxt[q];
    }
    note_overflow(bad, ovf);
}

// conv2 + conv3 of that path in ONE kernel, five states per workgroup (125 of its 128 MFMA rows).  A 10x10x32
// conv2 input is 12.8 KB as two fp16 planes: the five of them are copied into LDS once, in full cache lines,
// and both convolutions gather their im2col fragments from LDS (ds_read_b128) -- the 4x (conv2) and 9x (conv3)
// re-reads of the input and the fragment-shaped 16-byte global loads (64 cache lines per wave instruction) are gone,
// and conv2's output never leaves the CU.  Only the weights stream: 34 chunks of 32 k (16 conv2 taps, 18 conv3
// half taps) through a 3-slot LDS ring, fetched two chunks ahead.  Operands are swapped (D = W^T x A^T) so that a
// lane owns 4 consecutive channels of one pixel per register quad: 8-byte plane stores instead of 2-byte ones.
// LDS images are piece-rotated / XOR-swizzled so that the 16-lane groups of a ds_read_b128 spread over the banks.
struct C23Args {
    const uint16_t *p1s; size_t pl1;         // conv2 input planes [3][n*100][32]
    const uint4 *w;                          // split weights: conv2 chunks 0..15, conv3 chunks 16..33 (wsp + WSP_W2)
    const float *b2, *b3;
    uint16_t *a3s; size_t pl3;               // conv3 output planes [3][n*25][64]
    int n;
    const unsigned *pver; unsigned *wver;    // whole forward plans: the conv1 launch in front re-split the weights if these differed
    unsigned *wverc;                         // (the conv part's own version word, see AdamDev)
    float *h2o, *h3o;                        // training: fp32 copies of conv2's / conv3's output rows [n*25][64] for the backward pass, or NULL
    // C1 = true (the acting path on nibble states): conv1 + pool of the workgroup's states run HERE, in front of conv2 -- their output
    // goes straight into conv2's LDS image and never sees HBM (p1s / pl1 unused)
    const uint8_t *nib; const uint16_t *w1s; const float *b1;
    const float *params; uint4 *wsp; int FC;  // ... and the riding re-split of W_fc1's planes for the fc1 launch that follows (pver != wver)
    unsigned *ovf;                           // the net's overflow word (note_overflow)
    unsigned long long *round_flag; unsigned long long round_val; int round_blk;      // split schedule (or NULL): workgroup round_blk stores round_val on arrival
};

#ifndef C23_NO_LDSR
#define C23_NO_LDSR 0
#endif
#ifndef C23_NO_W
#define C23_NO_W 0
#endif
#ifndef C23_NO_BAR
#define C23_NO_BAR 0
#endif
#ifndef C23_NO_MFMA
#define C23_NO_MFMA 0
#endif
#ifndef C23_EXIT
#define C23_EXIT 0
#endif
// SPW = states per workgroup (5: 125 of the 128 MFMA rows; every launch takes 5).
// C1 = true: THE ACTING TRUNK -- conv1 + pool of the SPW states run in this kernel too, on the SAME-padded nibble states (one byte = 2
// pixels x 4 frames; the MFMA operand is a 256-entry table lookup, as in conv1_pool_kernel<true>): 8 waves x 6-7 tiles of 8 pooled pixels,
// each wave holding all 32 weight fragments of W_conv1's two planes in REGISTERS for its tiles (conv1_sp_kernel re-reads them from LDS
// for every tile: 32 KB of LDS reads per tile, 2.4 MB per CU -- that kernel is as much LDS- as MFMA-bound), and the pooled output is
// split straight into conv2's LDS image: the 13 + 13 MB of fp16 planes a separate conv1 launch would write and this kernel read back,
// and one launch boundary, are gone.  The nibble images, the table and the staged conv1 weights live where the weight ring and the exchange
// area will be (both idle until conv2 starts).
template <int NS, int SPW = 5, bool C1 = false>
__global__ __launch_bounds__(512) void conv23_sp_kernel(C23Args a) {
    // NS = 3: fp32-equivalent arithmetic on two fp16 planes (h, l; three products per step); NS = 1: one bf16 plane
    constexpr int NPL = NS == 3 ? 2 : 1, P0 = NS == 3 ? 0 : 2;             // operand planes in use / first weight plane of wsp
    constexpr int IN_P = SPW * 400, C2_P = SPW * 200, ZOFF = NPL * IN_P, RING = ZOFF + 16, RSZ = 4 * NPL * 64, XCH = RING + 6 * RSZ;   // uint4 units
    constexpr int NOWN = 17;                 // chunks per wave group
    constexpr int NIB_U4 = FB_NIB_STRIDE / 16, NIBO = RING, LUTO = RING + SPW * NIB_U4;      // (C1) nibble images and table inside the ring area
    static_assert(FB_NIB_STRIDE % 16 == 0 && SPW * NIB_U4 + 256 <= 6 * RSZ, "the conv1 front end borrows the weight ring");
    __shared__ uint4 smem[XCH + 2048];
    // EIGHT waves: wave group g = wave >> 2 takes the chunks of parity g (conv2 taps 2 i + g, then conv3 half taps 2 k + g) for the same
    // four 32-row tiles, so every SIMD holds two waves (w and w + 4) whose LDS reads, ring writes and barrier waits hide behind each
    // other's MFMAs -- with four waves (one per SIMD) a chunk took MFMA + LDS + barrier + ring time end to end (0.40 us against 0.21 us
    // of MFMAs; ablation builds -DC23_NO_*).  The two partial sums per output meet through LDS once per convolution; each wave then
    // finishes the channel tile ct = g.
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, w4 = wave & 3, grp = wave >> 2, hl = lane >> 5, j = lane & 31;
    const int s0 = blockIdx.x * SPW, ml = w4 * 32 + j;
    if (!C1 && a.wver && blockIdx.x == 0 && threadIdx.x == 0) { *a.wver = *a.pver; *a.wverc = *a.pver; }
    if (C1 && a.round_flag && (int)blockIdx.x == a.round_blk && threadIdx.x == 0) fb_flag_store(a.round_flag, a.round_val);
    const int bl = ml / 25, rem = ml - bl * 25, oy = rem / 5, ox = rem - oy * 5;
    const bool rowok = ml < SPW * 25;
    int nloc = a.n - s0; if (nloc > SPW) nloc = SPW;
    const int ringp = RING + grp * 3 * RSZ;  // this group's three ring slots
    // weight staging registers: named members, no arrays (hipcc otherwise parks them in LDS / scratch)
    struct BSt { uint4 v0, v1; };
    auto srcB = [&](int i, int q) {          // own chunk i = chunk 2 i + grp of the weight stream
        const int e = w4 + 4 * q, k8 = e / NPL, pl = e - k8 * NPL;
        return a.w + (size_t)(2 * i + grp) * 768 + (k8 * 3 + P0 + pl) * 64 + lane;
    };
    auto loadB = [&](int i) {                // by value throughout: a reference into a lambda defeats SROA (staging lands in LDS)
        BSt r;
        r.v0 = *srcB(i, 0);
        if (NPL == 2) r.v1 = *srcB(i, 1); else r.v1 = r.v0;
        return r;
    };
    auto storeB = [&](int slot, const BSt r) {
        uint4 *d = smem + ringp + slot * RSZ + w4 * 64 + lane;
        d[0] = r.v0;
        if (NPL == 2) d[256] = r.v1;
    };
    BSt bstA = loadB(0), bstB = loadB(1);
    bool bad = false;                        // an activation beyond the two-plane range was split (note_overflow at the end)
    if constexpr (C1) {
        // ---- conv1 + bias + relu + 2x2 max pool of the workgroup's states, into conv2's LDS image
        // W_fc1's planes for the fc1 launch that follows, if the parameters moved since they were split (decided on the device; the fc1
        // launch records the new version): at most one 8-weight item per thread, requested first
        if (a.pver && *a.pver != *a.wver)
            for (int id = IT_CONV + blockIdx.x * 512 + threadIdx.x; id < IT_CONV + 200 * a.FC; id += gridDim.x * 512) wsplit_item(a.params, a.wsp, a.FC, id);
        const uint4 *w1g = reinterpret_cast<const uint4 *>(a.w1s);
        const uint4 wc0 = w1g[threadIdx.x], wc1 = w1g[threadIdx.x + 512], wc2 = w1g[threadIdx.x + 1024], wc3 = w1g[threadIdx.x + 1536];
        const uint4 *ng = reinterpret_cast<const uint4 *>(a.nib + (size_t)s0 * FB_NIB_STRIDE);
        const int i0 = threadIdx.x, i1 = threadIdx.x + 512, i2 = threadIdx.x + 1024;      // (SPW * NIB_U4 = 1160 entries at SPW = 5: three per thread)
        static_assert(SPW * NIB_U4 <= 1536, "at most three image entries per thread");
        const uint4 n0 = ng[i0 < nloc * NIB_U4 ? i0 : 0], n1 = ng[i1 < nloc * NIB_U4 ? i1 : 0];
        uint4 n2 = make_uint4(0u, 0u, 0u, 0u);
        if constexpr (SPW * NIB_U4 > 1024) n2 = ng[i2 < nloc * NIB_U4 ? i2 : 0];
        smem[XCH + threadIdx.x] = wc0; smem[XCH + threadIdx.x + 512] = wc1; smem[XCH + threadIdx.x + 1024] = wc2; smem[XCH + threadIdx.x + 1536] = wc3;
        if (i0 < SPW * NIB_U4) smem[NIBO + i0] = i0 < nloc * NIB_U4 ? n0 : make_uint4(0u, 0u, 0u, 0u);
        if (i1 < SPW * NIB_U4) smem[NIBO + i1] = i1 < nloc * NIB_U4 ? n1 : make_uint4(0u, 0u, 0u, 0u);
        if constexpr (SPW * NIB_U4 > 1024) { if (i2 < SPW * NIB_U4) smem[NIBO + i2] = i2 < nloc * NIB_U4 ? n2 : make_uint4(0u, 0u, 0u, 0u); }
        if (threadIdx.x < 256) smem[LUTO + threadIdx.x] = nib_lut_entry(threadIdx.x);
        if (threadIdx.x < 16) smem[ZOFF + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
        if (nloc < SPW)                          // the last workgroup of a count that SPW does not divide: rows of absent states compute on zeros
            for (int i = threadIdx.x; i < NPL * IN_P; i += 512) smem[i] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        // this wave's copy of the 16 h-plane weight fragments ([c = (ky, kq)][lane]) stays in REGISTERS for all its tiles; the 16 l-plane
        // fragments are re-read from LDS per tile (all 32 in registers, 128 VGPRs, spill beside what the conv2 / conv3 pipeline holds)
        uint4 Wf[16];
#pragma unroll
        for (int c = 0; c < 16; c++) Wf[c] = smem[XCH + c * 64 + lane];
        const uint8_t *nibl = reinterpret_cast<const uint8_t *>(smem + NIBO);
        const uint4 *lut = smem + LUTO;
        const float bias1 = a.b1[j];
        const int npool = nloc * 100, ntile = (npool + 7) >> 3;
        for (int tile = wave; tile < ntile; tile += 8) {
            const int P = tile * 8 + (j >> 2), pos = j & 3, Pc = P < npool ? P : 0;
            const int st = Pc / 100, r100 = Pc - st * 100, py = r100 / 10, px = r100 - py * 10, poy = 2 * py + (pos >> 1), pox = 2 * px + (pos & 1);
            // the image carries conv1's SAME padding: every tap is base + ky * pitch + 2 * kq (include/fbdqn.h FB_NIB_*)
            const uint8_t *base = nibl + st * FB_NIB_STRIDE + (4 * poy) * FB_NIB_PITCH + 3 + 2 * pox + hl;
            unsigned raw[16];
#pragma unroll
            for (int c = 0; c < 16; c++) raw[c] = base[(c >> 1) * FB_NIB_PITCH + 2 * (c & 1)];
            f32x16 c1a = {0}, c1l = {0};
            int z;                                   // opaque 0: keeps the l-plane fragments in LDS (re-read per tile) instead of hoisted into registers
            asm volatile("s_mov_b32 %0, 0" : "=s"(z));
            const uint4 *wl1 = smem + XCH + 16 * 64 + lane + z;
#pragma unroll
            for (int h8 = 0; h8 < 2; h8++) {
                uint4 A[8];
#pragma unroll
                for (int c = 0; c < 8; c++) A[c] = lut[P < npool ? raw[8 * h8 + c] : 0u];
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    c1a = mfma_h(A[c], Wf[8 * h8 + c], c1a);
                    c1l = mfma_h(A[c], wl1[(8 * h8 + c) * 64], c1l);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) c1a[r] = fmaf(c1l[r], F16_LO_UNSCALE, c1a[r]);      // x*wh + (x*wl) / 4096: exact scale, one rounding
#pragma unroll
            for (int g = 0; g < 4; g++) {
                // register r of a lane = window position r & 3 of pooled pixel 2 * (r >> 2) + hl, channel j: the pool is a max over four
                // registers; relu(max + bias) == max of the relu'd values (monotone)
                const float bv = fmaxf(fmaxf(fmaxf(c1a[4 * g], c1a[4 * g + 1]), fmaxf(c1a[4 * g + 2], c1a[4 * g + 3])) + bias1, 0.f);
                const int Pp = tile * 8 + 2 * g + hl;
                if (Pp < npool) {
                    uint16_t *d = reinterpret_cast<uint16_t *>(smem + Pp * 4 + (((j >> 3) + (Pp >> 2)) & 3)) + (j & 7);
                    if constexpr (NS == 3) {
                        const _Float16 hh = (_Float16)bv, ll = (_Float16)((bv - (float)hh) * F16_LO_SCALE);
                        d[0] = __builtin_bit_cast(uint16_t, hh); d[IN_P * 8] = __builtin_bit_cast(uint16_t, ll);
                        bad |= bv >= FB_F16_RANGE;
                    } else d[0] = (uint16_t)f32_to_bf16_rn(bv);
                }
            }
        }
        __syncthreads();                         // the image is complete, and every wave is done with the ring area
    } else
    {   // the five input images, plane by plane; piece q of pixel pix lands on piece (q + (pix >> 2)) & 3
        uint4 t[NPL][4];
#pragma unroll
        for (int p = 0; p < NPL; p++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int q = threadIdx.x + 512 * r;
                const bool ok = q < nloc * 400;
                t[p][r] = make_uint4(0u, 0u, 0u, 0u);
                if (ok) t[p][r] = reinterpret_cast<const uint4 *>(a.p1s + p * a.pl1 + (size_t)s0 * 3200)[q];
            }
#pragma unroll
        for (int p = 0; p < NPL; p++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int q = threadIdx.x + 512 * r, pix = q >> 2;
                if (q < IN_P) smem[p * IN_P + pix * 4 + ((q + (pix >> 2)) & 3)] = t[p][r];
            }
        if (threadIdx.x < 16) smem[ZOFF + threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
    }
    // Software pipeline (everything by value -- a reference into a lambda defeats SROA): while the 12 MFMAs of own chunk
    // i run on fragments already in registers, the fragments of chunk i + 1 are read from LDS into a second
    // register set, the staged weights of chunk i + 2 go into ring slot (i + 2) % 3 and the global loads of chunk
    // i + 4 are issued; one barrier per chunk (= per pair of chunks of the weight stream).
    struct Fr { uint4 A[2][NPL]; uint4 W[2][2][NPL]; };
    auto readW = [&](int i, Fr f) {
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int ct = 0; ct < 2; ct++)
#pragma unroll
                for (int p = 0; p < NPL; p++) f.W[s][ct][p] = smem[ringp + (i % 3) * RSZ + ((2 * s + hl) * NPL + p) * 64 + ct * 32 + j];
        return f;
    };
    auto readA = [&](auto aidx, Fr f) {          // aidx(s, p) -> LDS index of this lane's activation fragment
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int p = 0; p < NPL; p++) f.A[s][p] = smem[aidx(s, p)];
        return f;
    };
    // acc: the h*h products; acl: h*l + l*h, folded in with the exact factor 1 / 4096 in the epilogue (NS = 3 only)
    f32x16 acc[2] = {{0}, {0}}, acl[2] = {{0}, {0}};
    auto compute = [&](const Fr f) {
        // NB the MFMA intrinsics are pure: nothing but a data dependence orders them.  Without the ordered use of the
        // accumulators at the head of each FB_STEP hipcc hoists them across the barrier to right behind the LDS reads that
        // produce their operands (reads -> wait -> MFMA: no prefetch distance at all)
#pragma unroll
        for (int s = 0; s < 2; s++)
#pragma unroll
            for (int ct = 0; ct < 2; ct++) {
                if constexpr (NS == 3) {
                    acl[ct] = mfma_h(f.W[s][ct][0], f.A[s][1], acl[ct]);
                    acl[ct] = mfma_h(f.W[s][ct][1], f.A[s][0], acl[ct]);
                    acc[ct] = mfma_h(f.W[s][ct][0], f.A[s][0], acc[ct]);
                } else acc[ct] = mfma_b(f.W[s][ct][0], f.A[s][0], acc[ct]);
            }
    };
    auto a2 = [&](int c) {                       // conv2 chunk c = tap (ky, kx), 32 channels
        const int iy = 2 * oy + (c >> 2) - 1, ix = 2 * ox + (c & 3) - 1;
        const bool ok = rowok && iy >= 0 && iy < 10 && ix >= 0 && ix < 10;
        const int pix = bl * 100 + iy * 10 + ix, hl_ = hl;
        return [=](int s, int p) { return ok ? p * IN_P + pix * 4 + ((2 * s + hl_ + (pix >> 2)) & 3) : ZOFF; };
    };
    auto a3 = [&](int c) {                       // conv3 chunk c = half a tap (ky, kx), channels 32 * (c & 1) ..
        const int cell = c >> 1, ky = cell / 3, kx = cell - 3 * ky, iy = oy + ky - 1, ix = ox + kx - 1;
        const bool ok = rowok && iy >= 0 && iy < 5 && ix >= 0 && ix < 5;
        const int pix = bl * 25 + iy * 5 + ix, hl_ = hl;
        return [=](int s, int p) { return ok ? p * C2_P + pix * 8 + ((4 * (c & 1) + 2 * s + hl_) ^ ((pix >> 1) & 7)) : ZOFF; };
    };
    storeB(0, bstA); bstA = loadB(2);
    __syncthreads();
    storeB(1, bstB); bstB = loadB(3);
    Fr cur = {};
    cur = readA(a2(grp), readW(0, cur));
    __syncthreads();
    if (C23_EXIT == 1) { if (cur.A[0][0].x == 0x12345u && cur.W[0][0][0].y == 77u) a.a3s[0] = 1; return; }
#define FB_STEP(i, ST, AIDX_NEXT, HAVE_A)                                                                         \
    {                                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        asm volatile("" : "+a"(acc[0]), "+a"(acc[1]), "+a"(acl[0]), "+a"(acl[1]));     /* see compute(): chunk i's MFMAs stay behind chunk i - 1's barrier */ \
        Fr nx = cur;                                                                                                   \
        if ((i) + 1 < NOWN && !C23_NO_LDSR) { nx = readW((i) + 1, nx); if (HAVE_A) nx = readA(AIDX_NEXT, nx); }        \
        compute(cur);                                                                                                  \
        if ((i) + 2 < NOWN && !C23_NO_W) { storeB(((i) + 2) % 3, ST); if ((i) + 4 < NOWN) ST = loadB((i) + 4); }       \
        /* issue order inside the chunk: one LDS read / ring write / global load behind each MFMA, so that the LDS pipe   \
           and the MFMA pipe run side by side instead of in two phases that the per-chunk barrier keeps in lock step */ \
        /* (12 MFMAs, 12 LDS reads, 2 ring writes, 2 global loads per chunk at NS = 3) */ \
        _Pragma("unroll") for (int i_ = 0; i_ < 8; i_++) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); } \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; i_++) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x200, 1, 0); } \
        _Pragma("unroll") for (int i_ = 0; i_ < 2; i_++) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x100, 1, 0); __builtin_amdgcn_sched_group_barrier(0x020, 1, 0); } \
        if (!C23_NO_BAR) __syncthreads();                                                                              \
        cur = nx;                                                                                                      \
    }
    // The two groups' partial sums of a convolution meet here: every wave parks the channel tile it does NOT finish (ct = 1 - grp) in the
    // exchange area and, after a barrier, adds its partner's share of the tile it does finish (ct = grp).  Then relu(sum + bias) of this
    // lane's 16 channels x 1 pixel, split, handed to put(plane, piece 0..7, 8-byte half).
    float *xch = reinterpret_cast<float *>(smem + XCH);
    auto epilogue = [&](const float *__restrict__ bias, float *__restrict__ side, auto put) {
        f32x16 mine, other;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float v0 = NS == 3 ? fmaf(acl[0][r], F16_LO_UNSCALE, acc[0][r]) : acc[0][r];
            const float v1 = NS == 3 ? fmaf(acl[1][r], F16_LO_UNSCALE, acc[1][r]) : acc[1][r];
            mine[r] = grp ? v1 : v0; other[r] = grp ? v0 : v1;
            acc[0][r] = 0.f; acc[1][r] = 0.f; acl[0][r] = 0.f; acl[1][r] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < 16; r++) xch[(wave * 16 + r) * 64 + lane] = other[r];
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; r++) mine[r] += xch[((wave ^ 4) * 16 + r) * 64 + lane];
        const int ct = grp;
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + ct * 32 + 8 * g + 4 * hl);
            const float o0 = fmaxf(mine[4 * g] + bv.x, 0.f), o1 = fmaxf(mine[4 * g + 1] + bv.y, 0.f), o2 = fmaxf(mine[4 * g + 2] + bv.z, 0.f),
                        o3 = fmaxf(mine[4 * g + 3] + bv.w, 0.f);
            uint32_t h0, l0, h1, l1, m_;
            if constexpr (NS == 3) { split2x2(o0, o1, h0, l0); split2x2(o2, o3, h1, l1); bad |= out_of_f16_range(o0, o1, o2, o3); }
            else { split3x2(o0, o1, h0, m_, l0); split3x2(o2, o3, h1, m_, l1); }
            put(0, ct * 4 + g, make_uint2(h0, h1));
            if (NS == 3) put(1, ct * 4 + g, make_uint2(l0, l1));
            if (side && rowok && bl < nloc)
                *reinterpret_cast<float4 *>(side + ((size_t)s0 * 25 + ml) * 64 + ct * 32 + 8 * g + 4 * hl) = make_float4(o0, o1, o2, o3);
        }
    };
    // ---- conv2: own chunks 0 .. 7 = taps 2 i + grp
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        FB_STEP(i, bstA, a2(2 * (i + 1) + grp), true);
        FB_STEP(i + 1, bstB, a2(2 * (i + 2) + grp), i + 2 < 8);       // conv3's activations do not exist yet
    }
    // its output pixel ml (= bl * 25 + oy * 5 + ox), 64 channels = 8 pieces, piece q on q ^ ((ml >> 1) & 7); aliases the input
    // images, which every wave has finished reading (barrier at the end of the last chunk)
    epilogue(a.b2, a.h2o, [&](int p, int piece, uint2 v) {
        if (rowok) reinterpret_cast<uint2 *>(smem + p * C2_P + ml * 8 + (piece ^ ((ml >> 1) & 7)))[hl] = v;
    });
    __syncthreads();
    if (C23_EXIT == 2) { if (smem[threadIdx.x].x == 0x12345u) a.a3s[0] = 1; return; }
    // ---- conv3: own chunks 8 .. 16 = half taps 2 k + grp (the first one's weight fragments are already in `cur`)
    cur = readA(a3(grp), cur);
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        FB_STEP(8 + k, bstA, a3(2 * (k + 1) + grp), true);
        FB_STEP(8 + k + 1, bstB, a3(2 * (k + 2) + grp), true);
    }
    FB_STEP(16, bstA, a3(0), false);
#undef FB_STEP
    epilogue(a.b3, a.h3o, [&](int p, int piece, uint2 v) {
        if (rowok && bl < nloc)
            *reinterpret_cast<uint2 *>(a.a3s + p * a.pl3 + ((size_t)s0 * 25 + ml) * 64 + piece * 8 + 4 * hl) = v;
    });
    if constexpr (NS == 3) note_overflow(bad && rowok && bl < nloc, a.ovf);      // (rows of absent states compute on garbage-free zeros anyway)
}

// conv2 + conv3 for SMALL batches (training, and any forward below 256 states): one workgroup per state, the same two-plane fp16
// arithmetic as conv23_sp_kernel (three MFMAs per fp32 product; NS = 1: one bf16 plane).  The two stand-alone fp32-MFMA kernels
// (round 1's conv2_kernel, conv3_kernel) were two launches of ~6.5 + 7.5 us whose matrix work is under a microsecond: what they wait for is
// the launch, a cold read of what the previous launch wrote, a 32-deep chain of 64-cycle fp32 MFMAs and an LDS reduction -- twice.
// Here conv1's pooled output of ONE state (12.8 KB fp32) is split into planes in LDS once, conv2's output never leaves the CU, and
// the 17 weight chunks of 64 k (8 for conv2's 16 taps x 32 channels, 9 for conv3's taps x 64 channels) go from L2 straight into the
// registers of the one wave that uses them.  8 waves = 2 channel tiles x 4 k-steps of a chunk; the four k partial sums per tile are
// added through LDS in a fixed order.
// fp32 side outputs h2 / h3 feed the backward kernels and fc1.  Operands swapped as in conv23_sp_kernel (D = W^T x A^T): a lane owns
// 4 consecutive channels of one pixel per register quad.
struct C23T {
    Slices sl;
    const float *p1; float *h2, *h3;
    const uint4 *w[3];                       // per slice: split weights of its net (wsp + WSP_W2)
    const unsigned *pver[2]; unsigned *wverc[2];     // the launch in front re-split W_conv2 / W_conv3 of a stale net: record it
    // RING = true (the whole conv trunk of a replay minibatch in this launch, fb_vec_step): the states come straight out of the frame
    // ring as bits, conv1 + pool run here too (p1o / amax: its fp32 side outputs for the backward pass, rows of slice 0)
    FbRingSrc ring; float *p1o; uint8_t *amax; unsigned long long *ring_fo;
    uint16_t *a3s; size_t pl3;               // conv3's output as planes too ([plane][row * 25 + pixel][64]) when fc1_sp_kernel follows, or NULL
    unsigned *ovf;                           // the net's overflow word (note_overflow)
};

// RING = true: conv1 of the state in front of conv2 + conv3, fed from the replay's 1-bit frame ring.  The workgroup locates its
// transition (index -> time slot, env), turns the four 800-byte frames of its state into the SAME-padded nibble image the acting conv1
// uses (one byte = 2 pixels x 4 frames, include/fbdqn.h FB_NIB_*) in LDS, and runs conv1_pool_kernel's tile loop on it: 13 tiles of 8
// pooled pixels over 8 waves, the operand a 256-entry table lookup.  The pooled output goes into conv2's LDS planes directly (and, for
// the online pass over s, as fp32 + pool positions to global for the backward kernels).  What this replaces: the gather launch with its
// 51 KB per transition of u8 expansion, and the conv1 launch.
#ifndef C23T_EXIT
#define C23T_EXIT 0
#endif
// W16 (ring-fed, small batches): sixteen waves per workgroup -- conv1's 13 tiles in ONE round instead of two; waves 8 .. 15 leave after it
// NST (ring-fed, a memory viewed with n > 1 steps, fb_replay_set_n_step): the s' slices read frames tt + n - 3 .. tt + n (their fshift is n,
// set on the host), and the workgroup that writes a / r / t forms the n-step return: lanes 0 .. n - 1 of wave 0 load row tt + k each (all
// n loads in flight at once), a ballot finds the first terminal and the rewards are summed through shuffles in ascending k
// (fb_nstep_return's arithmetic); lane 0 writes.  NST = false is the one-step kernel as it was.
template <int NS, bool RING, bool W16 = false, bool NST = false>
__global__ __launch_bounds__(W16 ? 1024 : 512) __attribute__((amdgpu_waves_per_eu(4))) void conv23_t_kernel(C23T a) {      // <= 128 registers: two workgroups per CU
    constexpr int NPL = NS == 3 ? 2 : 1, P0 = NS == 3 ? 0 : 2;
    constexpr int IN_P = 400, C2_P = 200, C2O = NPL * IN_P, ZOFF = C2O + NPL * C2_P, RED = ZOFF + 16;
    __shared__ uint4 smem[RED + 2048];
    __shared__ uint4 lut[RING ? 256 : 1];
    __shared__ uint32_t nibw[RING ? FB_NIB_STRIDE / 4 : 1];
    __shared__ unsigned long long fo[4];
    float *red = reinterpret_cast<float *>(smem + RED);
    const Slice s = a.sl.s[blockIdx.y];
    if ((int)blockIdx.x >= s.count) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, j = lane & 31, ct = wave & 1, kq = wave >> 1;
    const size_t row = (size_t)s.s_off + blockIdx.x;
    const uint4 *w = a.w[blockIdx.y];
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid < 2 && a.wverc[tid]) *a.wverc[tid] = *a.pver[tid];
    // Every weight fragment is used by exactly ONE wave (tile ct, k-step kq of chunk c): no sharing, so no LDS staging -- the wave reads
    // its two 512-byte row segments per plane straight from L2, three chunks ahead, and the chunk loop needs no barrier at all
    // (an LDS ring here cost a write, a read and a workgroup barrier per chunk for nothing).
    struct WF { uint4 v[NPL]; };
    auto loadW = [&](int c) {
        WF r;
#pragma unroll
        for (int p = 0; p < NPL; p++) r.v[p] = w[((size_t)(8 * c + 2 * kq + hl) * 3 + P0 + p) * 64 + ct * 32 + j];
        return r;
    };
    WF w0 = {}, w1 = {}, w2 = {};
    if (!W16 || wave < 8) { w0 = loadW(0); w1 = loadW(1); w2 = loadW(2); }
    bool bad = false;                        // an activation beyond the two-plane range was split (note_overflow)
    if constexpr (!RING) {   // the state's conv2 input: 100 pixels x 32 channels fp32 -> planes; piece q (8 channels) of pixel pix lands on (q + (pix >> 2)) & 3
        float4 t[2];
#pragma unroll
        for (int r = 0; r < 2; r++) { const int i = tid + 512 * r; t[r] = reinterpret_cast<const float4 *>(a.p1 + row * 3200)[i < 800 ? i : 0]; }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = tid + 512 * r, pix = i >> 3, q8 = i & 7;
            uint32_t h0, l0, h1, l1, m_;
            if constexpr (NS == 3) { split2x2(t[r].x, t[r].y, h0, l0); split2x2(t[r].z, t[r].w, h1, l1); bad |= out_of_f16_range(t[r].x, t[r].y, t[r].z, t[r].w); }
            else { split3x2(t[r].x, t[r].y, h0, m_, l0); split3x2(t[r].z, t[r].w, h1, m_, l1); }
            if (i < 800) {
                uint2 *d = reinterpret_cast<uint2 *>(smem + pix * 4 + (((q8 >> 1) + (pix >> 2)) & 3)) + (q8 & 1);
                d[0] = make_uint2(h0, h1);
                if (NS == 3) d[2 * IN_P] = make_uint2(l0, l1);          // plane 1: IN_P uint4 further
            }
        }
        if (tid < 16) smem[ZOFF + tid] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        // conv1's weight planes (32 KB) go into LDS once, into the reduction area conv2 / conv3 only need later: read from L2 fragment by
        // fragment inside the tile loop they cost a dependent round trip per pair of taps (4.8 us for the 13 tiles; named registers, see
        // conv1_sp_kernel)
        const uint4 *w1g = reinterpret_cast<const uint4 *>(s.w1s);
        const int t5 = tid & 511;                                             // (W16: threads 512 .. 1023 repeat the first half's copies)
        const uint4 wc0 = w1g[t5], wc1 = w1g[t5 + 512], wc2 = w1g[t5 + 1024], wc3 = w1g[t5 + 1536];
        // ---- where the state lives: frames tt - 3 + fshift .. of env e (four threads, one frame offset each)
        if constexpr (!NST) {
            if (tid < 4) {
                long long tt; int e;
                fb_ring_locate(a.ring.c, a.ring.steps, a.ring.idx[blockIdx.x], tid == 0 && blockIdx.y == 0, tt, e);
                const unsigned long long o = fb_frame_off(a.ring.c, tt - 3 + s.fshift + tid, e);
                fo[tid] = o;
                if (blockIdx.y == 0) {
                    a.ring_fo[blockIdx.x * 4 + tid] = o;                   // conv1's weight-gradient kernel builds its image from the same frames
                    if (tid == 0) {
                        const size_t mo = (size_t)(tt % a.ring.c.t_f) * a.ring.c.n_envs + e;
                        a.ring.a[blockIdx.x] = a.ring.c.act[mo]; a.ring.r[blockIdx.x] = a.ring.c.rew[mo]; a.ring.t[blockIdx.x] = a.ring.c.term[mo];
                    }
                }
            }
        } else {
            if (tid < FB_NSTEP_MAX) {                                      // (lanes of wave 0)
                long long tt; int e;
                fb_ring_locate(a.ring.c, a.ring.steps, a.ring.idx[blockIdx.x], tid == 0 && blockIdx.y == 0, tt, e);
                if (tid < 4) {
                    const unsigned long long o = fb_frame_off(a.ring.c, tt - 3 + s.fshift + tid, e);
                    fo[tid] = o;
                    if (blockIdx.y == 0) a.ring_fo[blockIdx.x * 4 + tid] = o;
                }
                if (blockIdx.y == 0) {
                    // lane k < n: row tt + k (rows are consecutive time slots, wrapping at most once: t_f >= n + 6); lanes past n read row tt
                    const FbGatherCtx &c = a.ring.c;
                    const int n = c.nstep, k = tid < n ? tid : 0, s0 = (int)(tt % c.t_f), sk = s0 + k < c.t_f ? s0 + k : s0 + k - c.t_f;
                    const size_t mo = (size_t)sk * c.n_envs + e;
                    const float rw = c.rew[mo];
                    const unsigned long long tmask = __ballot(tid < n && c.term[mo] != 0);
                    if (tid == 0) a.ring.a[blockIdx.x] = c.act[mo];
                    const int m = tmask ? __builtin_ctzll(tmask) + 1 : n;       // (uniform) the first terminal ends the sum
                    double acc = 0.0, g = 1.0;
                    for (int q = 0; q < m; q++) { acc += g * (double)__shfl(rw, q); g *= c.gamma; }
                    if (tid == 0) { a.ring.r[blockIdx.x] = (float)acc; a.ring.t[blockIdx.x] = tmask ? 1 : 0; }
                }
            }
        }
        if (tid < 256) lut[tid] = nib_lut_entry(tid);
        if (tid >= 256 && tid - 256 < FB_NIB_STRIDE / 16) reinterpret_cast<uint4 *>(nibw)[tid - 256] = make_uint4(0u, 0u, 0u, 0u);
        if (tid < 16) smem[ZOFF + tid] = make_uint4(0u, 0u, 0u, 0u);
        if (tid < 512) { smem[RED + tid] = wc0; smem[RED + tid + 512] = wc1; smem[RED + tid + 1024] = wc2; smem[RED + tid + 1536] = wc3; }
        __syncthreads();
        // ---- nibble image: group gi = 8 pixels of one row = one byte of each frame -> four nibble bytes (pixel pairs), one 4-byte store
        const uint8_t *fb = reinterpret_cast<const uint8_t *>(a.ring.c.bits);
        uint32_t fbyte[2][4];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int gi = t5 + 512 * r, gc = gi < 800 ? gi : 0;
#pragma unroll
            for (int f = 0; f < 4; f++) fbyte[r][f] = fb[fo[f] * 8 + gc];
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int gi = t5 + 512 * r, y = gi / 10, g = gi - y * 10;
            uint32_t o = 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int f = 0; f < 4; f++) {
                    const uint32_t t2 = (fbyte[r][f] >> (2 * q)) & 3u;           // pixels 2q, 2q + 1 of the group in frame f
                    o |= ((t2 & 1u) | ((t2 & 2u) << 3)) << (8 * q + f);            // bit 4 * px + f of nibble byte q
                }
            if (gi < 800 && tid < 512) nibw[((y + 2) * FB_NIB_PITCH + 4 + 4 * g) >> 2] = o;
        }
        __syncthreads();
        if (C23T_EXIT == 1) { if (nibw[tid] == 0x12345u) a.h2[0] = 1.f; return; }
        // ---- conv1 + bias + relu + 2x2 max pool (conv1_pool_kernel's tile loop on the LDS image): tiles wave, wave + 8 of 13
        const uint8_t *nib = reinterpret_cast<const uint8_t *>(nibw);
        const uint4 *WB = smem + RED + lane;                                          // [part][ky][kq][h][co] x 16 B
        const float bias = s.params[OFF_B1 + j];
        for (int tile = wave; tile < 13; tile += W16 ? 16 : 8) {
            const int P = tile * 8 + (j >> 2), pos = j & 3;
            const int py = P / 10, px = P - py * 10, oy = 2 * py + (pos >> 1), ox = 2 * px + (pos & 1);
            f32x16 acc = {0}, acl = {0};
            // the image carries conv1's SAME padding: every tap is base + ky * pitch + 2 * kq -- all 16 byte reads go out first, then the
            // 16 table reads, then the MFMAs (two LDS latencies per tile instead of two per pair of taps)
            const uint8_t *base = nib + (4 * (P < 100 ? oy : 0)) * FB_NIB_PITCH + 3 + 2 * (P < 100 ? ox : 0) + hl;
            unsigned raw[16];
#pragma unroll
            for (int c = 0; c < 16; c++) raw[c] = base[(c >> 1) * FB_NIB_PITCH + 2 * (c & 1)];
#pragma unroll
            for (int h8 = 0; h8 < 2; h8++) {                             // (two halves: 16 operands at once cost 132 registers, one too many
                uint4 A[8];                                              //  for two workgroups per CU at 256 samples)
#pragma unroll
                for (int c = 0; c < 8; c++) A[c] = lut[P < 100 ? raw[8 * h8 + c] : 0u];
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    acc = mfma_h(A[c], WB[(0 * 16 + 8 * h8 + c) * 64], acc);
                    acl = mfma_h(A[c], WB[(1 * 16 + 8 * h8 + c) * 64], acl);
                }
            }
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = fmaf(acl[r], F16_LO_UNSCALE, acc[r]);      // x*wh + (x*wl) / 4096: exact scale, one rounding
#pragma unroll
            for (int g = 0; g < 4; g++) {
                float bv = fmaxf(acc[4 * g] + bias, 0.f);
                int best = 0;
#pragma unroll
                for (int q = 1; q < 4; q++) {
                    const float v = fmaxf(acc[4 * g + q] + bias, 0.f);
                    if (v > bv) { bv = v; best = q; }
                }
                const int Pp = tile * 8 + 2 * g + hl;
                if (Pp < 100) {
                    if (blockIdx.y == 0) { const size_t o = (row * 100 + Pp) * 32 + j; a.p1o[o] = bv; a.amax[o] = (uint8_t)best; }
                    uint16_t *d = reinterpret_cast<uint16_t *>(smem + Pp * 4 + (((j >> 3) + (Pp >> 2)) & 3)) + (j & 7);
                    if constexpr (NS == 3) {
                        const _Float16 hh = (_Float16)bv, ll = (_Float16)((bv - (float)hh) * F16_LO_SCALE);
                        d[0] = __builtin_bit_cast(uint16_t, hh); d[IN_P * 8] = __builtin_bit_cast(uint16_t, ll);
                        bad |= bv >= FB_F16_RANGE;
                    } else d[0] = (uint16_t)f32_to_bf16_rn(bv);
                }
            }
        }
    }
    __syncthreads();
    if (W16 && wave >= 8) { if constexpr (NS == 3) note_overflow(bad, a.ovf); return; }                    // (their part -- conv1's tiles 8 .. 12 -- is done; s_barrier only counts the waves that are left)
    if (RING && C23T_EXIT == 2) { if (smem[tid].x == 0x12345u) a.h2[0] = 1.f; return; }
    const int oy = j / 5, ox = j - oy * 5;
    const bool rowok = j < 25;
    f32x16 acc = {0}, acl = {0};
    // the four k partial sums of each channel tile, added in k order; wave (ct', q) finishes registers 4q .. 4q + 3 of tile ct': channels
    // ct' * 32 + 8 q + 4 hl .. + 3 of pixel j
    auto finish = [&](const float *__restrict__ bias, float *__restrict__ out, bool planes) {
#pragma unroll
        for (int r = 0; r < 16; r++) red[((kq * 2 + ct) * 16 + r) * 64 + lane] = NS == 3 ? fmaf(acl[r], F16_LO_UNSCALE, acc[r]) : acc[r];
        __syncthreads();
        const int ctp = wave & 1, q = wave >> 1;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            v[e] = red[((0 * 2 + ctp) * 16 + 4 * q + e) * 64 + lane];
#pragma unroll
            for (int k = 1; k < 4; k++) v[e] += red[((k * 2 + ctp) * 16 + 4 * q + e) * 64 + lane];
        }
        const int ch = ctp * 32 + 8 * q + 4 * hl;
        const float4 bv = *reinterpret_cast<const float4 *>(bias + ch);
        v[0] = fmaxf(v[0] + bv.x, 0.f); v[1] = fmaxf(v[1] + bv.y, 0.f); v[2] = fmaxf(v[2] + bv.z, 0.f); v[3] = fmaxf(v[3] + bv.w, 0.f);
        if (rowok) *reinterpret_cast<float4 *>(out + (row * 25 + j) * 64 + ch) = make_float4(v[0], v[1], v[2], v[3]);
        if ((planes || a.a3s) && rowok) {
            uint32_t h0, l0, h1, l1, m_;
            if constexpr (NS == 3) { split2x2(v[0], v[1], h0, l0); split2x2(v[2], v[3], h1, l1); bad |= out_of_f16_range(v[0], v[1], v[2], v[3]); }
            else { split3x2(v[0], v[1], h0, m_, l0); split3x2(v[2], v[3], h1, m_, l1); }
            if (planes) {
                uint2 *d = reinterpret_cast<uint2 *>(smem + C2O + j * 8 + ((ctp * 4 + q) ^ ((j >> 1) & 7))) + hl;
                d[0] = make_uint2(h0, h1);
                if (NS == 3) d[2 * C2_P] = make_uint2(l0, l1);
            } else {
                uint16_t *d = a.a3s + (row * 25 + j) * 64 + ch;
                *reinterpret_cast<uint2 *>(d) = make_uint2(h0, h1);
                if (NS == 3) *reinterpret_cast<uint2 *>(d + a.pl3) = make_uint2(l0, l1);
            }
        }
#pragma unroll
        for (int r = 0; r < 16; r++) { acc[r] = 0.f; acl[r] = 0.f; }
    };
#pragma unroll
    for (int c = 0; c < 17; c++) {
        // this wave's k-step of chunk c: 16 k = two 8-k pieces (lane halves)
        int aidx[2];
        if (c < 8) {                                                     // conv2: chunk = taps 2c, 2c + 1 x 32 channels
            const int tap = 2 * c + (kq >> 1), iy = 2 * oy + (tap >> 2) - 1, ix = 2 * ox + (tap & 3) - 1, pix = iy * 10 + ix;
            const bool ok = rowok && iy >= 0 && iy < 10 && ix >= 0 && ix < 10;
#pragma unroll
            for (int p = 0; p < NPL; p++) aidx[p] = ok ? p * IN_P + pix * 4 + ((((kq & 1) * 2 + hl) + (pix >> 2)) & 3) : ZOFF;
        } else {                                                         // conv3: chunk = tap c - 8 x 64 channels
            const int tap = c - 8, ky = tap / 3, iy = oy + ky - 1, ix = ox + (tap - 3 * ky) - 1, pix = iy * 5 + ix;
            const bool ok = rowok && iy >= 0 && iy < 5 && ix >= 0 && ix < 5;
#pragma unroll
            for (int p = 0; p < NPL; p++) aidx[p] = ok ? C2O + p * C2_P + pix * 8 + ((2 * kq + hl) ^ ((pix >> 1) & 7)) : ZOFF;
        }
        uint4 A[NPL];
#pragma unroll
        for (int p = 0; p < NPL; p++) A[p] = smem[aidx[p]];
        const WF W = w0;
        w0 = w1; w1 = w2;
        if (c + 3 < 17) w2 = loadW(c + 3);
        if constexpr (NS == 3) {
            acl = mfma_h(W.v[0], A[1], acl);
            acl = mfma_h(W.v[1], A[0], acl);
            acc = mfma_h(W.v[0], A[0], acc);
        } else acc = mfma_b(W.v[0], A[0], acc);
        if (c == 7) { finish(s.params + OFF_B2, a.h2, true); __syncthreads(); }      // conv2 done: its output becomes conv3's LDS image
    }
    finish(s.params + OFF_B3, a.h3, false);
    if constexpr (NS == 3) note_overflow(bad, a.ovf);
}

// fc1 of that path: hfp[ks] = A[M x 1600] x W[1600 x N] over a quarter of K.  One workgroup = 128 rows x 64 columns x
// 12 or 13 chunks of 32 k (grid z = 4 slices: exactly 256 workgroups at 1024 states and N = 512).  Both operands go
// through LDS: the activation chunk is fetched as 64-byte row segments (4 lanes per row, not one 16-byte fragment
// per lane from 64 different lines) into a piece-rotated image, the weight chunk as in conv23_sp_kernel; same
// software pipeline (fragments of chunk c + 1 read while chunk c is in the MFMAs, chunk c + 2 written to its ring
// slot, chunk c + 4 in flight from global).  A slice with only 12 chunks runs its 13th on the zero page.
constexpr int FC1_SP_KS = 4;
struct Fc1Args { const uint16_t *ain; size_t aplane; const uint16_t *zeros; const uint4 *w; float *hfp; int stot, M, N;
                 const unsigned *pver; unsigned *wver;          // (behind the fused acting trunk, which re-split W_fc1's planes if they were stale: record it)
                 const uint4 *w2; int m_split;                  // rows from m_split on (a multiple of the 128-row tile) take the weights w2: the target net's slices in the same launch
                 const float *hp_src; float *hp_dst; int hp_n;      // the fused acting forward: the parameters its head will read (b_fc1 on), copied for it here
                 unsigned long long *set_flag; unsigned long long set_val; };   // split schedule (or NULL): this launch has started, so the trunk in front of it has retired

// ablation switch (tools/abl_forward.sh; 0 = the product): 1 no global loads inside the chunk loop, 2 no MFMAs, 3 no ring writes / fragment
// reads (no LDS traffic in the loop), 4 no output stores
#ifndef FC1_ABL
#define FC1_ABL 0
#endif
template <int NS>
__global__ __launch_bounds__(256) void fc1_sp_kernel(Fc1Args a) {
    constexpr int NPL = NS == 3 ? 2 : 1, P0 = NS == 3 ? 0 : 2;                   // as in conv23_sp_kernel
    constexpr int ASZ = NPL * 512, BSZ = 4 * NPL * 64, SLOT = ASZ + BSZ;         // uint4 units
    __shared__ uint4 smem[3 * SLOT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, j = lane & 31;
    if (a.wver && blockIdx.x == 0 && threadIdx.x == 0) *a.wver = *a.pver;
    if (a.hp_dst) { const int i = blockIdx.x * 256 + threadIdx.x; if (i < a.hp_n) a.hp_dst[i] = a.hp_src[i]; }
    if (a.set_flag && blockIdx.x == 0 && threadIdx.x == 0) fb_flag_store(a.set_flag, a.set_val);
    // XCD-aware tile order (consecutive workgroup ids go round the 8 XCDs, each with its own 4 MB L2): XCD x takes K slice
    // x & 3 and the column tiles of half x >> 2, for every row tile -- 0.6 MB of weights + 2.4 MB of activations per L2
    // instead of all 4.9 MB of weights behind each one (row-tile-major order: 49 MB through the fabric per 1024 states)
    const int xcd = blockIdx.x & 7, w = blockIdx.x >> 3, nth = a.N >> 7;          // nth = column tiles per half
    const int ks = xcd & 3, m0 = (w / nth) * 128, n0 = ((xcd >> 2) * nth + w % nth) * 64;
    const int cbase = ks * 12 + (ks < 2 ? ks : 2), count = ks < 2 ? 13 : 12;
    // staging registers as named members (arrays here end up in LDS / scratch: hipcc does not scalarise them)
    struct St { uint4 a0, a1, a2, a3, b0, b1; };
    // per-thread source pointers, fixed for the whole K loop: chunk c of the activations is an immediate offset
    // (64 B per chunk), the weight pointers advance by one chunk per load() (load() is called in chunk order).
    // Rows past M are clamped to the last row (computed, never stored); a slice with 12 chunks still LOADS a 13th
    // (the buffers are padded by one chunk) but skips its MFMAs.
    const int r0 = min(m0 + (int)(threadIdx.x >> 2), a.M - 1), r1 = min(m0 + 64 + (int)(threadIdx.x >> 2), a.M - 1);
    const uint16_t *pa0 = a.ain + (size_t)r0 * 1600 + (size_t)cbase * 32 + (threadIdx.x & 3) * 8;
    const uint16_t *pa1 = a.ain + (size_t)r1 * 1600 + (size_t)cbase * 32 + (threadIdx.x & 3) * 8;
    auto ldA = [&](int c, int p, int i) { return *reinterpret_cast<const uint4 *>((i ? pa1 : pa0) + p * a.aplane + c * 32); };
    const uint4 *wsel = a.w2 && m0 >= a.m_split ? a.w2 : a.w;
    auto pbq = [&](int q) {
        const int e = wave + 4 * q, k8 = e / NPL, pl = e - k8 * NPL;
        return wsel + ((size_t)(cbase * 4 + k8) * 3 + P0 + pl) * a.N + n0 + lane;
    };
    const uint4 *pb0 = pbq(0), *pb1 = pbq(NPL == 2 ? 1 : 0);
    const size_t bstep = (size_t)12 * a.N;
    auto ldB = [&](int c, int q) {
        (void)c;
        const uint4 *&pb = q == 0 ? pb0 : pb1;
        const uint4 v = *pb;
        pb += bstep;
        return v;
    };
    auto load = [&](int c) {
        St r;
        r.a0 = ldA(c, 0, 0); r.a1 = ldA(c, 0, 1); r.b0 = ldB(c, 0);
        if (NPL == 2) { r.a2 = ldA(c, 1, 0); r.a3 = ldA(c, 1, 1); r.b1 = ldB(c, 1); }
        else { r.a2 = r.a0; r.a3 = r.a0; r.b1 = r.b0; }
        return r;
    };
    auto stA_ = [&](int slot, int p, int i, const uint4 v) {
        const int q = threadIdx.x + 256 * i, row = q >> 2;
        smem[slot * SLOT + p * 512 + row * 4 + ((q + (row >> 2)) & 3)] = v;
    };
    auto store = [&](int slot, const St r) {
        stA_(slot, 0, 0, r.a0); stA_(slot, 0, 1, r.a1);
        uint4 *d = smem + slot * SLOT + ASZ + wave * 64 + lane;
        d[0] = r.b0;
        if (NPL == 2) { stA_(slot, 1, 0, r.a2); stA_(slot, 1, 1, r.a3); d[256] = r.b1; }
    };
    struct Fr { uint4 A[NPL]; uint4 W[2][NPL]; };         // the fragments of ONE k-step (16 k) of a chunk
    const int row = wave * 32 + j;
    auto readF = [&](int slot, int s) {
        Fr f;
#pragma unroll
        for (int p = 0; p < NPL; p++) {
            f.A[p] = smem[slot * SLOT + p * 512 + row * 4 + ((2 * s + hl + (row >> 2)) & 3)];
#pragma unroll
            for (int ct = 0; ct < 2; ct++) f.W[ct][p] = smem[slot * SLOT + ASZ + ((2 * s + hl) * NPL + p) * 64 + ct * 32 + j];
        }
        return f;
    };
    f32x16 acc[2] = {{0}, {0}}, acl[2] = {{0}, {0}};       // h*h products; h*l + l*h (folded in at the end, x 1 / 4096)
    auto compute = [&](const Fr f) {
        if (FC1_ABL == 2) { acc[0][0] += __uint_as_float(f.A[0].x ^ f.W[0][0].y ^ f.W[1][NPL - 1].z ^ f.A[NPL - 1].w); return; }
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            if constexpr (NS == 3) {
                acl[ct] = mfma_h(f.A[1], f.W[ct][0], acl[ct]);
                acl[ct] = mfma_h(f.A[0], f.W[ct][1], acl[ct]);
                acc[ct] = mfma_h(f.A[0], f.W[ct][0], acc[ct]);
            } else acc[ct] = mfma_b(f.A[0], f.W[ct][0], acc[ct]);
        }
    };
    St stA = load(0), stB = load(1);
    store(0, stA); stA = load(2);
    __syncthreads();
    store(1, stB); stB = load(3);
    Fr cur = readF(0, 0);
    __syncthreads();
    // half-chunk software pipeline: the fragments of the next k-step are read while the 12 MFMAs of this one run
#define FB_STEP(cc, ST)                                                                                    \
    {                                                                                                          \
        const Fr f1 = FC1_ABL == 3 ? cur : readF((cc) % 3, 1);                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        compute(cur);                                                                                          \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        const Fr nx = FC1_ABL == 3 ? cur : readF(((cc) + 1) % 3, 0);                                           \
        if ((cc) + 2 < 13) { if (FC1_ABL != 3) store(((cc) + 2) % 3, ST); if ((cc) + 4 < 13 && FC1_ABL != 1) ST = load((cc) + 4); }              \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        compute(f1);                                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                                     \
        __syncthreads();                                                                                       \
        cur = nx;                                                                                              \
    }
#pragma unroll
    for (int c = 0; c < 12; c += 2) { FB_STEP(c, stA); FB_STEP(c + 1, stB); }
    if (count > 12) { compute(cur); compute(readF(0, 1)); }            // chunk 12 sits in ring slot 12 % 3
#undef FB_STEP
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
        for_rows(m0 + wave * 32, a.M, lane, [&](int r, int mr) {
            if (FC1_ABL == 4 && acc[ct][r] != 12345.f) return;
            a.hfp[((size_t)ks * a.stot + mr) * a.N + n0 + ct * 32 + j] = NS == 3 ? fmaf(acl[ct][r], F16_LO_UNSCALE, acc[ct][r]) : acc[ct][r];
        });
}

// relu(bias + sum of the fc1 partials) for one (sample, unit)
__device__ __forceinline__ float fc1_out(const float *__restrict__ hfp, int stot, int FC, int smp, int jj, float bias, int nks) {
    float v = hfp[(size_t)smp * FC + jj], t[FC1_KS];
#pragma unroll
    for (int ks = 1; ks < FC1_KS; ks++) {                        // loads in flight together, none under a branch
        const float x = hfp[((size_t)(ks < nks ? ks : 0) * stot + smp) * FC + jj];
        t[ks] = ks < nks ? x : 0.f;
    }
#pragma unroll
    for (int ks = 1; ks < FC1_KS; ks++) v += t[ks];              // fixed order; + 0.f is exact
    return fmaxf(v + bias, 0.f);
}

// fc2 / dueling head (+ epsilon-greedy action for the acting path); one wave per sample
struct HeadArgs { Slices sl; int nslices; HeadCore c; };

__global__ __launch_bounds__(256) void head_kernel(HeadArgs H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = nullptr;
    const int smp = slice_row(H.sl, H.nslices, blockIdx.x * 4 + wave, P);
    if (smp < 0) return;
    head_one(H.c, P, smp, lane);
}

// ================================================================== loss + head backward
// Device-resident optimizer / parameter-version state.  Everything that decides WHAT a later launch has to do lives here and
// not in the host handle, so a step replayed from a captured hipGraph leaves the same state behind as a live one:
//   ticks / applies   Adam step counter bookkeeping: the loss kernel advances beta1^t / beta2^t (a "tick") only when the previous
//                     tick has been consumed by an Adam update (ticks == applies); the Adam kernel marks it consumed
//   pver / wver       version of the parameters of net 0 / 1 (bumped by whatever writes them: Adam, init, load, target sync) and
//                     the version the fp16 planes of W_conv2 / W_conv3 / W_fc1 (wsp) were split from; the acting forward
//                     compares the two ON THE DEVICE and re-splits when they differ.  wverc: the same for the W_conv2 / W_conv3 part
//                     alone, which is all the small-batch conv2+conv3 kernel needs (conv23_t_kernel; a train-only loop re-splits 70 K
//                     weights per step, not 890 K)
// The Adam scalars and the tick bookkeeping are the base FbAdamHead (fb_common.h): what the side code objects see of this struct
struct AdamDev : FbAdamHead { unsigned pver[2], wver[2], wverc[2];
                              unsigned ovf; };      // ovf: waves that split an activation beyond FB_F16_RANGE (note_overflow)
static_assert(sizeof(AdamDev) == sizeof(FbAdamHead) + 7 * sizeof(unsigned), "AdamDev is its base, then its own 7 words: no padding between them");

// Munchausen-DQN (include/fbdqn.h): the net's (tau, alpha, l0).  MD instantiations of the two scalar loss bodies read the THIRD slice
// (rows 2B ..: s through the target net) whatever L.algo says, and L.algo names the loss's form alone there: FB_ALGO_NATURE (FB_ALGO_MDQN)
// or FB_ALGO_PER (FB_ALGO_MDQN_PER).  The other instantiations are what they were before the parameter existed.
struct MdPar { float tau, alpha, clip; };
// V = lse_tau(q-(s', .)) and the bonus alpha max(tau ln pi-(a|s), l0) from the finished Q rows qn = q-(s', .), q3 = q-(s, .); entries
// c >= A are masked by selects.  One action: the sums are exp(0) = 1, log(1) = 0, so V = qn[0] and the bonus 0 exactly.
template <int AT, int NQ>
__device__ __forceinline__ void mdqn_target(const float (&qn)[NQ], const float (&q3)[NQ], int A, int a_b, const MdPar &M, float &V, float &bonus) {
    float mn = qn[0], m3 = q3[0], qa = q3[0];
#pragma unroll
    for (int c = 1; c < AT; c++) { mn = c < A ? fmaxf(mn, qn[c]) : mn; m3 = c < A ? fmaxf(m3, q3[c]) : m3; qa = c == a_b ? q3[c] : qa; }
    float sn = 0.f, s3 = 0.f;
#pragma unroll
    for (int c = 0; c < AT; c++) { sn += c < A ? expf((qn[c] - mn) / M.tau) : 0.f; s3 += c < A ? expf((q3[c] - m3) / M.tau) : 0.f; }
    V = mn + M.tau * logf(sn);
    bonus = M.alpha * fmaxf((qa - m3) - M.tau * logf(s3), M.clip);
}

// The scalar loss's two later options (include/fbdqn.h), template parameters of the two loss bodies like MD:
//   DP  FB_ALGO_DOUBLE_PER: Double's target (a* = the online net's first maximum over s', the value from the third slice: s' through the
//       target net) whatever L.algo says, and L.algo = FB_ALGO_PER names the loss's form (weighted by isw, a mean)
//   HU  the Huber (clipped-error) loss with the net's delta > 0: l(d) = d^2 inside |d| <= delta, delta (2 |d| - delta) outside; the
//       gradient takes clamp(d, -delta, delta) where the squared loss takes d.  Inside the zone both are the squared loss's own
//       expressions (w * d * d and -scale * w * d with the clamp returning d itself), so they agree with it bit for bit.
// No load and no branch: selects on values the body holds already.
template <bool HU>
__device__ __forceinline__ float td_clamp(float d, float delta) { if constexpr (HU) return fminf(fmaxf(d, -delta), delta); else return d; }
template <bool HU>
__device__ __forceinline__ float td_term(float w, float d, float delta) {
    const float sq = w * d * d;
    if constexpr (HU) { const float ad = fabsf(d); return ad <= delta ? sq : w * (delta * (2.f * ad - delta)); } else return sq;
}

struct LossArgs {
    int algo, B, FC, A, dueling;
    NetOff off;
    const float *params;            // online
    const float *q;                 // [3B][A] workspace
    const float *hf; int stot, nks; // fc1 partials [nks][stot][FC]; rows 0..B-1 = s through the online net
    const uint8_t *act; const float *rew; const uint8_t *term; const float *isw;
    double gamma;
    float *grad, *dhf, *loss, *abs_err, *y_out;
    float *gmax;                    // [FC / 16]: every workgroup's maximum |dhf| (fc1_bwd_big_kernel derives its operand pre-scale from them)
    AdamDev *adam; int tick;
};

// (Large batches only: small ones get all of this inside fc1_bwd2_kernel.)
// grid = FC / 16 workgroups.  Every workgroup recomputes the B targets (cheap), workgroup 0 also publishes
// loss / abs_err / y, the output-bias gradients and the Adam tick.  Thread (jl, bg) owns unit j and every
// 16th sample; the 16 partial sums per unit are added in a fixed order.  (64 units x 4 sample groups per workgroup
// meant 8 workgroups, each thread walking 64 samples in 8 dependent rounds of loads: 13.8 us at B = 256.)
// ONE round trip to memory: the unit's parameters and the fc1 partial sums of its first 8 samples (all of them at
// B <= 32) are requested at the top, together with the Q values / rewards / actions of the target computation --
// nothing is loaded behind the barrier, and no load sits under a branch (clamped addresses + selects; AT = the
// number of actions at compile time, MAXA = read it from L.A).
template <int AT, bool MD = false, bool DP = false, bool HU = false>
__device__ __forceinline__ void loss_head_body(const LossArgs &L, float (*dadv)[MAXA], float *dv, float *lterm, float (*part)[16][MAXA + 2], float *wmax, const MdPar M = MdPar{},
                                               const float delta = 0.f) {
    const int tid = threadIdx.x, B = L.B, A = AT == MAXA ? L.A : AT;
    const bool lead = blockIdx.x == 0;
    const float *P = L.params;
    const int jl = tid & 15, bg = tid >> 4, jj = blockIdx.x * 16 + jl;
    // ---- everything this thread needs from memory
    float gw[AT], wrow[AT], gv = 0.f, gb = 0.f, dmax = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) { gw[a] = 0.f; wrow[a] = P[L.off.wq + jj * A + (a < A ? a : 0)]; }
    float wvj = P[(L.dueling ? L.off.wv : L.off.bf1) + jj];
    const float bias = P[L.off.bf1 + jj];
    float hv[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int b = bg + 16 * u;
        hv[u] = fc1_out(L.hf, L.stot, L.FC, b < B ? b : bg, jj, bias, L.nks);
    }
    const int tb = tid < B ? tid : 0;                            // threads past the batch recompute sample 0 and store nothing
    const bool dbl = DP || L.algo == FB_ALGO_DOUBLE;
    float qsv[AT], qnv[AT], q3v[AT];
#pragma unroll
    for (int a = 0; a < AT; a++) {
        const int ac = a < A ? a : 0;
        qsv[a] = L.q[(size_t)tb * A + ac];
        qnv[a] = L.q[(size_t)(B + tb) * A + ac];                 // DQN: online(s'); Nature/PER: target(s'); Double: online(s')
        q3v[a] = L.q[(size_t)((MD || dbl ? 2 * B : 0) + tb) * A + ac]; // Double only: target(s'); Munchausen (MD): target(s)
    }
    const float rf = L.rew[tb];
    const int termb = L.term[tb], a_b = L.act[tb];
    float isw = L.isw ? L.isw[tb] : 1.f;                         // (a kernel argument decides: uniform branch, taken by PER alone)
#pragma unroll
    for (int a = 0; a < AT; a++) { keep(wrow[a]); keep(qsv[a]); keep(qnv[a]); keep(q3v[a]); }
    keep(wvj);
#pragma unroll
    for (int u = 0; u < 8; u++) keep(hv[u]);
    if (!L.dueling) wvj = 0.f;
    if (L.algo != FB_ALGO_PER) isw = 1.f;
    // ---- targets
    {
        float sel;
        if (dbl) {                                               // BrainDoubleDQN.py:51-54
            int am = 0;
#pragma unroll
            for (int a = 1; a < AT; a++) if (a < A && qnv[a] > qnv[am]) am = a;
            sel = q3v[0];
#pragma unroll
            for (int a = 1; a < AT; a++) sel = a == am ? q3v[a] : sel;
        } else {
            sel = qnv[0];
#pragma unroll
            for (int a = 1; a < AT; a++) sel = a < A ? fmaxf(sel, qnv[a]) : sel;
        }
        // BrainDQN.py:210-215: python float64 arithmetic on the rewards 0.1 / 3 / -3, then fed as float32
        double r = rf == 0.1f ? 0.1 : (double)rf;
        if constexpr (MD) {                                      // Munchausen: the soft bootstrap, and the log-policy bonus on the reward
            float bonus;
            mdqn_target<AT>(qnv, q3v, A, a_b, M, sel, bonus);
            r += (double)bonus;
        }
        const double yd = termb ? r : r + L.gamma * (double)sel;
        const float y = (float)yd;
        float qe = qsv[0];
#pragma unroll
        for (int a = 1; a < AT; a++) qe = a == a_b ? qsv[a] : qe;
        const float d = y - qe;                                  // q_eval = reduce_sum(Q * onehot)
        const float w = isw;
        const float scale = L.algo == FB_ALGO_DQN ? 2.f : 2.f / (float)B;     // sum vs mean
        const float g = -scale * w * td_clamp<HU>(d, delta);     // dLoss/dQ[b][a_b]
        if (tid < B) {
            lterm[tid] = td_term<HU>(w, d, delta);
            if (lead && L.abs_err) L.abs_err[tid] = fabsf(d);
            if (lead && L.y_out) L.y_out[tid] = y;
            if (L.dueling) {
                dv[tid] = g;
#pragma unroll
                for (int a = 0; a < AT; a++) dadv[tid][a] = (a == a_b ? g : 0.f) - g / (float)A;
            } else {
                dv[tid] = 0.f;
#pragma unroll
                for (int a = 0; a < AT; a++) dadv[tid][a] = a == a_b ? g : 0.f;
            }
        }
    }
    __syncthreads();
    if (lead && tid == 0) {
        float s = 0.f;
        for (int b = 0; b < B; b++) s += lterm[b];
        *L.loss = L.algo == FB_ALGO_DQN ? s : s / (float)B;
        adam_tick(L.adam, L.tick);
    }
    if (lead && tid >= 64 && tid < 64 + A) { const int a = tid - 64; float s = 0.f; for (int b = 0; b < B; b++) s += dadv[b][a]; L.grad[L.off.bq + a] = s; }
    if (lead && tid == 128 && L.dueling) { float s = 0.f; for (int b = 0; b < B; b++) s += dv[b]; L.grad[L.off.bv] = s; }
    // 8 samples per round: their 8 x nks partial sums are requested together (the first round's at the top of the kernel);
    // the arithmetic and its order per sample are unchanged
    for (int b0 = bg; b0 < B; b0 += 128) {
        if (b0 != bg) {
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int b = b0 + 16 * u;
                hv[u] = fc1_out(L.hf, L.stot, L.FC, b < B ? b : bg, jj, bias, L.nks);
            }
#pragma unroll
            for (int u = 0; u < 8; u++) keep(hv[u]);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int b = b0 + 16 * u;
            if (b < B) {
                const float h = hv[u];
                float d = dv[b] * wvj;
#pragma unroll
                for (int a = 0; a < AT; a++) if (a < A) { d = fmaf(dadv[b][a], wrow[a], d); gw[a] = fmaf(h, dadv[b][a], gw[a]); }
                gv = fmaf(h, dv[b], gv);
                const float dh = h > 0.f ? d : 0.f;
                L.dhf[(size_t)b * L.FC + jj] = dh;
                dmax = fmaxf(dmax, fabsf(dh));
                gb += dh;
            }
        }
    }
#pragma unroll
    for (int a = 0; a < AT; a++) part[bg][jl][a] = gw[a];
    part[bg][jl][MAXA] = gv; part[bg][jl][MAXA + 1] = gb;
    wg_max_write(dmax, wmax, tid >> 6, tid & 63);
    __syncthreads();
    if (tid == 0) L.gmax[blockIdx.x] = wg_max_read<4>(wmax);
    if (bg == 0) {
        auto total = [&](int c) {
            float v = part[0][jl][c];
#pragma unroll
            for (int g = 1; g < 16; g++) v += part[g][jl][c];
            return v;
        };
#pragma unroll
        for (int a = 0; a < AT; a++)
            if (a < A) L.grad[L.off.wq + jj * A + a] = total(a);
        if (L.dueling) L.grad[L.off.wv + jj] = total(MAXA);
        L.grad[L.off.bf1 + jj] = total(MAXA + 1);
    }
}

__global__ __launch_bounds__(256) void loss_head_kernel(LossArgs L) {
    __shared__ float dadv[MAXTB][MAXA];
    __shared__ float dv[MAXTB];
    __shared__ float lterm[MAXTB];
    __shared__ float part[16][16][MAXA + 2];
    __shared__ float wmax[4];
    if (L.A == 2) loss_head_body<2>(L, dadv, dv, lterm, part, wmax);
    else loss_head_body<MAXA>(L, dadv, dv, lterm, part, wmax);
}
// ... with the Munchausen target (FB_ALGO_MDQN / _PER): a kernel of its own, so that loss_head_kernel stays the code it was
__global__ __launch_bounds__(256) void loss_head_md_kernel(LossArgs L, MdPar M) {
    __shared__ float dadv[MAXTB][MAXA];
    __shared__ float dv[MAXTB];
    __shared__ float lterm[MAXTB];
    __shared__ float part[16][16][MAXA + 2];
    __shared__ float wmax[4];
    if (L.A == 2) loss_head_body<2, true>(L, dadv, dv, lterm, part, wmax, M);
    else loss_head_body<MAXA, true>(L, dadv, dv, lterm, part, wmax, M);
}
// ... with FB_ALGO_DOUBLE_PER's target (DP) and / or the Huber loss (HU), on either target: the options are compile-time flags of one
// extended kernel, instantiated for the four combinations the host asks for (loss_stage), so that the two kernels above stay the code
// they were and no net with delta = 0 pays for a clamp
template <bool DP, bool HU, bool MD>
__global__ __launch_bounds__(256) void loss_head_x_kernel(LossArgs L, MdPar M, float delta) {
    __shared__ float dadv[MAXTB][MAXA];
    __shared__ float dv[MAXTB];
    __shared__ float lterm[MAXTB];
    __shared__ float part[16][16][MAXA + 2];
    __shared__ float wmax[4];
    if (L.A == 2) loss_head_body<2, MD, DP, HU>(L, dadv, dv, lterm, part, wmax, M, delta);
    else loss_head_body<MAXA, MD, DP, HU>(L, dadv, dv, lterm, part, wmax, M, delta);
}

// fb_qnet_apply_adam on gradients that no fb_qnet_train_step ticked for (guarded on the device, so it is safe to launch always)
__global__ void adam_tick_kernel(AdamDev *ad) { adam_tick(ad, 1); }
__global__ void bump_pver_kernel(AdamDev *ad, int which) { ad->pver[which] += 1; }
__global__ void mark_split_kernel(AdamDev *ad, int which) { ad->wver[which] = ad->pver[which]; ad->wverc[which] = ad->pver[which]; }

// ================================================================== distributional (C51) head: acting, evaluation and training
// include/fbdqn.h pins the semantics.  logits[a][i] = relu(h_fc1) . W[:, a N + i] + b[a N + i], p = softmax_i, Q[a] = sum_i z_i p[a][i].
// One wave per state.  Lane i holds atom i of EVERY action (register a = action a): the softmax of an action, its Q and the projection
// are then whole-wave reductions, and the loads of one weight row are contiguous across the lanes.  Lanes >= N read the clamped column
// N - 1 and are masked by selects: no load sits under a branch (head_one_t's rule).
struct C51Sup { int N; float vmin, vmax, dz; };
__device__ __forceinline__ float rdlane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ float wave_sum(float v) {          // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// the logits of state `row` (fc1 partial sums hf[nks][stot][FC]) through the head parameters P: 64 units per round, each unit's
// activation broadcast from the lane that computed it (v_readlane: a scalar operand of the FMAs)
template <int AT>
__device__ __forceinline__ void c51_logits(const float *__restrict__ hf, int stot, int nks, int FC, const float *__restrict__ P, const NetOff &off,
                                           int A, int N, int row, int lane, float (&lg)[AT]) {
    const int AN = A * N, il = lane < N ? lane : N - 1;
#pragma unroll
    for (int a = 0; a < AT; a++) lg[a] = 0.f;
    for (int j0 = 0; j0 < FC; j0 += 64) {                         // (FC % 128 == 0)
        const float x = fc1_out(hf, stot, FC, row, j0 + lane, P[off.bf1 + j0 + lane], nks);
        const float *__restrict__ w = P + off.wq + (size_t)j0 * AN + il;
#pragma unroll 8
        for (int k = 0; k < 64; k++) {
            const float xs = rdlane(x, k);
#pragma unroll
            for (int a = 0; a < AT; a++) lg[a] = fmaf(xs, w[(size_t)k * AN + (a < A ? a : 0) * N], lg[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < AT; a++) lg[a] += P[off.bq + (a < A ? a : 0) * N + il];
}
// softmax of one action's logits over the N atoms: p on this lane (0 past N), and the log of the normaliser (max + log sum)
__device__ __forceinline__ float c51_softmax(float lg, bool on, float &lse) {
    const float m = wave_max(on ? lg : -INFINITY);
    const float e = on ? expf(lg - m) : 0.f;
    const float s = wave_sum(e);
    lse = m + logf(s);
    return e / s;
}
template <int AT>
__device__ __forceinline__ void c51_q(const float (&lg)[AT], bool on, float z, float (&qv)[AT]) {
#pragma unroll
    for (int a = 0; a < AT; a++) {
        float lse;
        qv[a] = wave_sum(c51_softmax(lg[a], on, lse) * z);
    }
}

// acting / evaluation head of ONE state: Q = E[Z], argmax (first maximum) and head_one_t's epsilon rule, bit for bit the same draws
struct C51Core {
    const float *hf; int stot, nks; float *q, *probs; int FC, A; NetOff off; C51Sup sup;      // probs: f32[row][A][N] or NULL
    uint8_t *actions; float epsilon; uint32_t seed_lo, seed_hi, step_lo, step_hi;
    const int32_t *key_of; uint32_t stream;      // epsilon counter: key_of[row] on `stream` (fb_eval_run), or the row on FB_STREAM_EPS
};
// QR (qr_head_kernel, a QR net): lg holds the quantiles theta, Q = (1/N) sum_i theta_i, and `probs` receives theta
template <int AT, bool QR = false>
__device__ __forceinline__ void c51_head_one(const C51Core &C, const float *__restrict__ P, int smp, int lane) {
    const int A = AT == MAXA ? C.A : AT, N = C.sup.N;
    const bool on = lane < N;
    const int key = C.key_of ? C.key_of[smp] : smp;
    float lg[AT], qv[AT];
    c51_logits<AT>(C.hf, C.stot, C.nks, C.FC, P, C.off, A, N, smp, lane, lg);
    const float z = C.sup.vmin + (float)(on ? lane : 0) * C.sup.dz;
    if constexpr (QR) {
        float *row = C.probs ? C.probs + (size_t)smp * A * N + lane : nullptr;
#pragma unroll
        for (int a = 0; a < AT; a++) {
            if (row && on && a < A) row[a * N] = lg[a];
            qv[a] = wave_sum(on ? lg[a] : 0.f) * (1.f / (float)N);
        }
    } else if (C.probs) {                                                // (a kernel argument decides: uniform branch)
        float *row = C.probs + (size_t)smp * A * N + lane;
#pragma unroll
        for (int a = 0; a < AT; a++) {
            float lse;
            const float p = c51_softmax(lg[a], on, lse);
            if (on && a < A) row[a * N] = p;
            qv[a] = wave_sum(p * z);
        }
    } else c51_q<AT>(lg, on, z, qv);
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < AT; a++) if (a < A) C.q[(size_t)smp * A + a] = qv[a];
        if (C.actions) {                                         // BrainDQN.py:103-108
            int best = 0;
#pragma unroll
            for (int a = 1; a < AT; a++) if (a < A && qv[a] > qv[best]) best = a;           // np.argmax: first maximum
            const fb_u4 o = fb_philox(C.seed_lo, C.seed_hi, (uint32_t)key, C.step_lo, C.stream, C.step_hi);
            const float u = (float)(o.x >> 8) * (1.0f / 16777216.0f);                      // random.random()
            if (u <= C.epsilon) best = (int)(((unsigned long long)o.y * (unsigned)A) >> 32);   // randrange(A)
            C.actions[smp] = (uint8_t)best;
        }
    }
}
// params != NULL: every row reads that copy of the head parameters (fb_eval_run: the one the fused acting forward's fc1 launch took)
struct C51HeadArgs { Slices sl; int nslices; const float *params; C51Core c; };
template <int AT>
__global__ __launch_bounds__(256) void c51_head_kernel(C51HeadArgs H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = nullptr;
    const int smp = slice_row(H.sl, H.nslices, blockIdx.x * 4 + wave, P);
    if (smp < 0) return;
    c51_head_one<AT>(H.c, H.params ? H.params : P, smp, lane);
}
// the QR head (a QR net): c51_head_kernel's layout and slices, Q = the mean of the quantiles
template <int AT>
__global__ __launch_bounds__(256) void qr_head_kernel(C51HeadArgs H) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *P = nullptr;
    const int smp = slice_row(H.sl, H.nslices, blockIdx.x * 4 + wave, P);
    if (smp < 0) return;
    c51_head_one<AT, true>(H.c, H.params ? H.params : P, smp, lane);
}

// ---- training, launch 1 of 2: one wave per sample.  Rows of hf: s (online net, 0 .. B-1), s' through p_next (B ..), and for
// FB_ALGO_C51_DOUBLE s' through the target net (2B ..).  Forms a* and the target distribution, projects it onto the support
// (m, a deterministic gather: lane i adds up, in order j = 0 .. N-1, what atom j sends it -- no atomics), the sample's loss term, the
// logit gradient (p - m) / B of the taken action (dl[b][64]), and from it the fc1 pre-activation gradient row dhf[b][FC] (and the
// activation row xs[b][FC] the second launch reads).
struct C51LossArgs {
    int algo, B, FC, A, nks, stot; NetOff off; C51Sup sup;
    const float *p_on, *p_next, *p_tgt;
    const float *hf; const uint8_t *act; const float *rew; const uint8_t *term; double gamma;
    float *dl, *xs, *lterm, *dhf;
    const float *isw; float *abs_err;                            // PW only: importance weights f32[B]; priorities f32[B] out or NULL
};
// PW (FB_ALGO_C51_PER / _DOUBLE_PER): the loss term and the logit gradient are weighted by isw[b] -- g = ((p - m) / B) * w, so that
// dhf, the second launch's gradients and the loss all carry the weight and w = 1 gives the unweighted results bit for bit -- and the
// sample's priority max(0, KL(m || p)) goes to abs_err[b].  (L.algo: the target's form only, FB_ALGO_C51 or FB_ALGO_C51_DOUBLE.)
template <int AT, bool PW = false>
__global__ __launch_bounds__(256) void c51_loss_kernel(C51LossArgs L) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;                                        // (wave-uniform)
    const int A = AT == MAXA ? L.A : AT, N = L.sup.N, B = L.B, FC = L.FC;
    const bool on = lane < N;
    const float vmin = L.sup.vmin, vmax = L.sup.vmax, dz = L.sup.dz;
    const float z = vmin + (float)(on ? lane : 0) * dz;
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;  // (an action past the head reads the last one: stays in bounds)
    const float r = L.rew[b];
    const int done = L.term[b];
    float ls[AT], ln[AT], lt[AT];
    c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_on, L.off, A, N, b, lane, ls);
    c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_next, L.off, A, N, B + b, lane, ln);
    if (L.algo == FB_ALGO_C51_DOUBLE) c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_tgt, L.off, A, N, 2 * B + b, lane, lt);
    else {
#pragma unroll
        for (int a = 0; a < AT; a++) lt[a] = ln[a];
    }
    // a* = argmax_a Q(s', a) of p_next's distribution (C51: the target net, double: the online net), first maximum
    float qn[AT];
    c51_q<AT>(ln, on, z, qn);
    int best = 0;
#pragma unroll
    for (int a = 1; a < AT; a++) if (a < A && qn[a] > qn[best]) best = a;
    float d = lt[0], la = ls[0];
#pragma unroll
    for (int a = 1; a < AT; a++) { d = a == best ? lt[a] : d; la = a == ab ? ls[a] : la; }
    float lse_n, lse_s;
    const float pn = c51_softmax(d, on, lse_n);                  // the target distribution p(s', a*)
    // projection of Tz_j = clamp(R + Gamma (1 - done) z_j, vmin, vmax) onto the support
    const float G = done ? 0.f : (float)L.gamma;
    float tz = r + G * z;
    tz = fminf(fmaxf(tz, vmin), vmax);
    float bj = (tz - vmin) / dz;
    bj = fminf(fmaxf(bj, 0.f), (float)(N - 1));                  // ((vmax - vmin) / dz may round past N - 1)
    float m = 0.f;
    for (int j = 0; j < N; j++) {
        const float pj = rdlane(pn, j), bb = rdlane(bj, j);
        const float lf = floorf(bb), uf = ceilf(bb);
        const int l = (int)lf, u = (int)uf;
        const float wl = l == u ? pj : pj * (uf - bb), wu = pj * (bb - lf);   // l == u: the whole mass stays on the atom
        m += lane == l ? wl : 0.f;
        m += lane == u && u != l ? wu : 0.f;
    }
    // loss -sum_i m_i log_softmax(logits(s, a_b))_i and its logit gradient (p - m) / B
    const float ps = c51_softmax(la, on, lse_s);
    float lossb = wave_sum(on ? -m * (la - lse_s) : 0.f);
    float g = on ? (ps - m) / (float)B : 0.f;
    if constexpr (PW) {
        // KL(m || p) = sum_i m_i (log m_i - log p_i) over the atoms with m_i > 0 (log m_i through a select: no branch around it)
        const float w = L.isw[b];
        const bool pos = on && m > 0.f;
        const float kl = wave_sum(pos ? m * (logf(pos ? m : 1.f) - (la - lse_s)) : 0.f);
        if (L.abs_err && lane == 0) L.abs_err[b] = fmaxf(kl, 0.f);
        lossb *= w;
        g *= w;
    }
    L.dl[(size_t)b * 64 + lane] = g;
    if (lane == 0) L.lterm[b] = lossb;
    const int AN = A * N;
    for (int j0 = 0; j0 < FC; j0 += 64) {
        const int j = j0 + lane;
        const float x = fc1_out(L.hf, L.stot, FC, b, j, L.p_on[L.off.bf1 + j], L.nks);
        const float *__restrict__ w = L.p_on + L.off.wq + (size_t)j * AN + ab * N;
        float dh = 0.f;
        for (int i = 0; i < N; i++) dh = fmaf(rdlane(g, i), w[i], dh);
        L.dhf[(size_t)b * FC + j] = x > 0.f ? dh : 0.f;
        L.xs[(size_t)b * FC + j] = x;
    }
}

// ---- QR training, launch 1 of 2 (include/fbdqn.h): c51_loss_kernel's grid and rows, one wave per sample, lane i = quantile i of every
// action.  Forms a* (the first maximum of the mean of p_next's quantiles), the targets T_j = R + Gamma (1 - done) theta_target(s', a*)_j,
// then the pairwise quantile Huber loss: lane i walks j = 0 .. N-1 in order with T_j broadcast by v_readlane (deterministic, no atomics).
// dl[b][64] = dl_b/dtheta / B on the taken action, and the dhf / xs rows exactly as c51_loss_kernel's tail: c51_grad_kernel /
// c51d_grad_kernel follow unchanged.  PW (FB_ALGO_QR_PER / _DOUBLE_PER): the loss term and dl carry isw[b] (g = (dl_b / B) * w), the
// priority abs_err[b] = l_b does not.  (L.algo: the target's form only, FB_ALGO_QR or FB_ALGO_QR_DOUBLE.)
struct QRLossArgs {
    int algo, B, FC, A, N, nks, stot; NetOff off; float kappa;
    const float *p_on, *p_next, *p_tgt;
    const float *hf; const uint8_t *act; const float *rew; const uint8_t *term; double gamma;
    float *dl, *xs, *lterm, *dhf;
    const float *isw; float *abs_err;                            // PW only: importance weights f32[B]; priorities f32[B] out or NULL
};
template <int AT, bool PW = false>
__global__ __launch_bounds__(256) void qr_loss_kernel(QRLossArgs L) {
    const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= L.B) return;                                        // (wave-uniform)
    const int A = AT == MAXA ? L.A : AT, N = L.N, B = L.B, FC = L.FC;
    const bool on = lane < N;
    const float kappa = L.kappa, invN = 1.f / (float)N;
    const int a_raw = L.act[b], ab = a_raw < A ? a_raw : A - 1;  // (an action past the head reads the last one: stays in bounds)
    const float r = L.rew[b];
    const int done = L.term[b];
    float ts[AT], tn[AT], tt[AT];
    c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_on, L.off, A, N, b, lane, ts);
    c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_next, L.off, A, N, B + b, lane, tn);
    if (L.algo == FB_ALGO_QR_DOUBLE) c51_logits<AT>(L.hf, L.stot, L.nks, FC, L.p_tgt, L.off, A, N, 2 * B + b, lane, tt);
    else {
#pragma unroll
        for (int a = 0; a < AT; a++) tt[a] = tn[a];
    }
    // a* = argmax_a of the mean quantile of p_next (QR: the target net, double: the online net), first maximum
    float qn[AT];
#pragma unroll
    for (int a = 0; a < AT; a++) qn[a] = wave_sum(on ? tn[a] : 0.f) * invN;
    int best = 0;
#pragma unroll
    for (int a = 1; a < AT; a++) if (a < A && qn[a] > qn[best]) best = a;
    float d = tt[0], th = ts[0];
#pragma unroll
    for (int a = 1; a < AT; a++) { d = a == best ? tt[a] : d; th = a == ab ? ts[a] : th; }
    const float T = done ? r : r + (float)L.gamma * d;           // target quantile j on lane j
    const float tau = (float)(2 * lane + 1) / (float)(2 * N);
    float ls = 0.f, gs = 0.f;
    for (int j = 0; j < N; j++) {
        const float u = rdlane(T, j) - th, au = fabsf(u);
        const float wt = fabsf(tau - (u < 0.f ? 1.f : 0.f));
        const float hub = au <= kappa ? 0.5f * u * u : kappa * (au - 0.5f * kappa);
        ls += wt * hub / kappa;
        gs += wt * fminf(fmaxf(u, -kappa), kappa) / kappa;
    }
    const float lb = wave_sum(on ? ls : 0.f) * invN;             // l_b
    float lossb = lb;
    float g = on ? (-gs * invN) / (float)B : 0.f;
    if constexpr (PW) {
        const float w = L.isw[b];
        if (L.abs_err && lane == 0) L.abs_err[b] = lb;
        lossb *= w;
        g *= w;
    }
    L.dl[(size_t)b * 64 + lane] = g;
    if (lane == 0) L.lterm[b] = lossb;
    const int AN = A * N;
    for (int j0 = 0; j0 < FC; j0 += 64) {
        const int j = j0 + lane;
        const float x = fc1_out(L.hf, L.stot, FC, b, j, L.p_on[L.off.bf1 + j], L.nks);
        const float *__restrict__ w = L.p_on + L.off.wq + (size_t)j * AN + ab * N;
        float dh = 0.f;
        for (int i = 0; i < N; i++) dh = fmaf(rdlane(g, i), w[i], dh);
        L.dhf[(size_t)b * FC + j] = x > 0.f ? dh : 0.f;
        L.xs[(size_t)b * FC + j] = x;
    }
}

// ---- training, launch 2 of 2: one workgroup per 16 fc1 units (grid FC / 16, the grid of loss_head_kernel): b_fc1's gradient and the
// tile's maximum |dhf| (gmax: fc1_bwd_big_kernel's pre-scale), then W_fc2's gradient for those units -- thread (c, ug) owns column c
// of units 8 ug .. 8 ug + 7 and walks the samples in order -- and, in workgroup 0, b_fc2's gradient, the loss and the Adam tick.
// DUEL (c51d_grad_kernel, a dueling C51 net): the tile's W_eff / b_eff gradients go through LDS and unfold into the net's own head
// (L.off: W_v b_v W_a b_a), dW_v[:, i] = sum_a dW_eff[:, a N + i], dW_a = dW_eff - (1/A) sum_a' dW_eff[:, a' N + i] -- N + A N <= 192
// columns per unit, walked by the whole workgroup.
struct C51GradArgs { int B, FC, A, N; NetOff off; const float *dl, *xs, *lterm, *dhf; const uint8_t *act; float *grad, *loss, *gmax; AdamDev *adam; int tick; };
template <bool DUEL>
__device__ __forceinline__ void c51_grad_body(const C51GradArgs &L) {
    __shared__ float dlt[MAXTB * 64];
    __shared__ float xt[MAXTB * 16];
    __shared__ int at[MAXTB];
    __shared__ float part[16][16];
    __shared__ float wmax[4];
    const int tid = threadIdx.x, B = L.B, FC = L.FC, j00 = blockIdx.x * 16;
    for (int k = tid; k < B * 64; k += 256) dlt[k] = L.dl[k];
    for (int k = tid; k < B * 16; k += 256) xt[k] = L.xs[(size_t)(k >> 4) * FC + j00 + (k & 15)];
    for (int k = tid; k < B; k += 256) at[k] = L.act[k] < L.A ? L.act[k] : L.A - 1;
    const int jl = tid & 15, bg = tid >> 4;
    float s = 0.f, mx = 0.f;
    for (int b = bg; b < B; b += 16) { const float d = L.dhf[(size_t)b * FC + j00 + jl]; s += d; mx = fmaxf(mx, fabsf(d)); }
    part[bg][jl] = s;
    wg_max_write(mx, wmax, tid >> 6, tid & 63);
    __syncthreads();
    if (tid == 0) L.gmax[blockIdx.x] = wg_max_read<4>(wmax);
    if (bg == 0) {
        float v = part[0][jl];
#pragma unroll
        for (int q = 1; q < 16; q++) v += part[q][jl];
        L.grad[L.off.bf1 + j00 + jl] = v;
    }
    const int AN = L.A * L.N, c = tid & 127, ug = tid >> 7;
    const int cc = c < AN ? c : 0, ac = cc / L.N, ic = cc - ac * L.N;
    float acc[8], gb = 0.f;
#pragma unroll
    for (int u = 0; u < 8; u++) acc[u] = 0.f;
    for (int b = 0; b < B; b++) {
        const float w = at[b] == ac ? dlt[b * 64 + ic] : 0.f;
        gb += w;
#pragma unroll
        for (int u = 0; u < 8; u++) acc[u] = fmaf(xt[b * 16 + ug * 8 + u], w, acc[u]);
    }
    if constexpr (DUEL) {
        constexpr int ES = 129;                                  // (row stride of the exchange: 16 x 129 + 128 floats in dlt's space)
        float *ge = dlt, *gbe = dlt + 16 * ES;
        __syncthreads();                                         // (every thread is through dlt)
        if (c < AN) {
#pragma unroll
            for (int u = 0; u < 8; u++) ge[(ug * 8 + u) * ES + c] = acc[u];
            if (ug == 0) gbe[c] = gb;
        }
        __syncthreads();
        const int N = L.N, A = L.A, W = N + AN;                  // output columns of a unit: dW_v (N), then dW_a (A N)
        for (int k = tid; k < 16 * W; k += 256) {
            const int u = k / W, col = k - u * W, i = col < N ? col : (col - N) % N;
            const float *e = ge + u * ES;
            float sm = 0.f;
            for (int q = 0; q < A; q++) sm += e[q * N + i];
            if (col < N) L.grad[L.off.wv + (size_t)(j00 + u) * N + col] = sm;
            else L.grad[L.off.wq + (size_t)(j00 + u) * AN + (col - N)] = e[col - N] - sm / (float)A;
        }
        if (blockIdx.x == 0 && tid < W) {
            const int i = tid < N ? tid : (tid - N) % N;
            float sm = 0.f;
            for (int q = 0; q < A; q++) sm += gbe[q * N + i];
            if (tid < N) L.grad[L.off.bv + tid] = sm;
            else L.grad[L.off.bq + (tid - N)] = gbe[tid - N] - sm / (float)A;
        }
    } else if (c < AN) {
#pragma unroll
        for (int u = 0; u < 8; u++) L.grad[L.off.wq + (size_t)(j00 + ug * 8 + u) * AN + c] = acc[u];
        if (blockIdx.x == 0 && ug == 0) L.grad[L.off.bq + c] = gb;
    }
    if (blockIdx.x == 0 && tid == 0) {
        float t = 0.f;
        for (int b = 0; b < B; b++) t += L.lterm[b];
        *L.loss = t / (float)B;
        if (L.tick && L.adam->ticks == L.adam->applies) {        // (adam_tick's statements: calling it here reorders this kernel)
            AdamDev &ad = *L.adam;
            ad.alpha = ad.lr * sqrtf(1.f - ad.b2pow) / (1.f - ad.b1pow);
            ad.b1pow *= ad.b1; ad.b2pow *= ad.b2;
            ad.ticks += 1;
        }
    }
}
__global__ __launch_bounds__(256) void c51_grad_kernel(C51GradArgs L) { c51_grad_body<false>(L); }
__global__ __launch_bounds__(256) void c51d_grad_kernel(C51GradArgs L) { c51_grad_body<true>(L); }

// ---- dueling C51 (FB_ARCH_C51_DUELING): V_i + Adv_{a,i} - (1/A) sum_a' Adv_{a',i} is linear in h, so the head folds into an effective
// C51 head, W_eff[:, a N + i] = W_v[:, i] + (W_a[:, a N + i] - (1/A) sum_a' W_a[:, a' N + i]) and b_eff likewise, and every C51 kernel
// above reads it unchanged.  heff = [b_fc1 | W_eff | b_eff]: the C51 layout from b_fc1 on (the net's hoff), refolded whenever the
// net's parameters change.
struct C51dFoldArgs { const float *p; float *heff; NetOff off; int FC, A, N; };
__global__ __launch_bounds__(256) void c51d_fold_kernel(C51dFoldArgs F) {
    const int AN = F.A * F.N, k = blockIdx.x * 256 + threadIdx.x;
    if (k >= F.FC + (F.FC + 1) * AN) return;
    if (k < F.FC) { F.heff[k] = F.p[F.off.bf1 + k]; return; }
    const int kk = k - F.FC, row = kk / AN, c = kk - row * AN, a = c / F.N, i = c - a * F.N;
    const bool bias = row == F.FC;                               // (the last row: b_eff)
    const float *wa = F.p + (bias ? F.off.bq : F.off.wq + row * AN) + i;
    const float v = F.p[bias ? F.off.bv + i : F.off.wv + row * F.N + i];
    float sm = 0.f;
    for (int q = 0; q < F.A; q++) sm += wa[q * F.N];
    F.heff[k] = v + (wa[a * F.N] - sm / (float)F.A);
}

// ---- noisy C51 nets (include/fbdqn.h): fc1 and every head layer are factorised Gaussian layers.  The master vector of a net is
// [mu | sigma]: mu in the net's own layout (n floats), then sigma of every parameter from W_fc1 on (sigma of q at n + q - OFF_WF1).  What
// every other kernel reads is the effective vector of the same layout as mu, materialised after each change of mu, sigma or the noise:
// the trunk copied, q >= OFF_WF1 as mu + sigma * e(q), e(q) = f(eps_out_j) f(eps_in_i) for a weight, f(eps_out_j) for a bias.
// Layer l: W[fin][fout] at w, then b[fout]; the layers are consecutive from OFF_WF1 on (fc1, then the head's one or two).  The noise
// vector of a net: per layer f(eps_in)[fin] at ein, then f(eps_out)[fout] at eout.
struct NoisyLayer { int w, fin, fout, ein, eout; float sig; };      // sig: the initial sigma, sigma0 / sqrt(fin)
struct NoisyNet { NoisyLayer l[3]; int nl, n, nz; };
__device__ __forceinline__ NoisyLayer noisy_layer(const NoisyNet &N, int q) {      // (selects, no dynamic index: no scratch)
    NoisyLayer L = N.l[0];
    if (N.nl > 1 && q >= N.l[1].w) L = N.l[1];
    if (N.nl > 2 && q >= N.l[2].w) L = N.l[2];
    return L;
}
__device__ __forceinline__ float noisy_factor(const NoisyNet &N, const float *__restrict__ nz, int q) {
    const NoisyLayer L = noisy_layer(N, q);
    const int r = q - L.w, i = r / L.fout, j = r - i * L.fout;
    const float fo = nz[L.eout + j];
    return i < L.fin ? fo * nz[L.ein + i] : fo;                  // (row fin: the bias)
}

// one draw of a net's noise vector: element k of net `which` at (seed, step) is z = Box-Muller of Philox(key = seed, counter = (k,
// step_lo, FB_STREAM_NOISE, 2 step_hi + which)), the formula of init_params_kernel without its truncation, stored as f(z) =
// sign(z) sqrt|z|.  mean: zeros (the effective weights are mu exactly)
__global__ __launch_bounds__(256) void noise_draw_kernel(float *__restrict__ nz, int len, uint32_t seed_lo, uint32_t seed_hi, uint32_t step_lo,
                                                         uint32_t c3, int mean) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= len) return;
    float f = 0.f;
    if (!mean) {
        const fb_u4 r = fb_philox(seed_lo, seed_hi, (uint32_t)k, step_lo, FB_STREAM_NOISE, c3);
        const float u1 = ((r.x >> 8) + 1) * (1.0f / 16777216.0f), u2 = (r.y >> 8) * (1.0f / 16777216.0f);
        const float z = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        f = copysignf(sqrtf(fabsf(z)), z);
    }
    nz[k] = f;
}

// the effective parameters of a net from q0 on (0: the trunk changed as well).  ad (or NULL): a new parameter version for the W_fc1
// planes the forward re-splits, the conv planes staying current if they were
// ne: the end of the noisy range [OFF_WF1, ne) -- N.n, but for an IQN net, whose W_e b_e behind it have no sigma and are copied as the trunk is
struct NoisyMat { const float *mst; float *eff; const float *nz; NoisyNet N; int q0, which; AdamDev *ad; int ne; };
__global__ __launch_bounds__(256) void noisy_mat_kernel(NoisyMat a) {
    if (a.ad && blockIdx.x == 0 && threadIdx.x == 0) {
        const unsigned v = a.ad->pver[a.which];
        if (a.ad->wverc[a.which] == v) a.ad->wverc[a.which] = v + 1;
        a.ad->pver[a.which] = v + 1;
    }
    const int q = a.q0 + blockIdx.x * 256 + threadIdx.x;
    if (q >= a.N.n) return;
    const float mu = a.mst[q];
    if (q < OFF_WF1 || q >= a.ne) { a.eff[q] = mu; return; }
    const float s = a.mst[a.N.n + q - OFF_WF1], e = noisy_factor(a.N, a.nz, q);
    a.eff[q] = s == 0.f || e == 0.f ? mu : fmaf(s, e, mu);           // (exactly mu without noise)
}

// sigma's gradient, behind every gradient of the effective parameters: g[n + q - OFF_WF1] = g[q] e(q)
__global__ __launch_bounds__(256) void noisy_sgrad_kernel(float *__restrict__ g, const float *__restrict__ nz, NoisyNet N, int ne) {
    const int q = OFF_WF1 + blockIdx.x * 256 + threadIdx.x;
    if (q >= ne) return;
    g[N.n + q - OFF_WF1] = g[q] * noisy_factor(N, nz, q);
}

// sigma's initial values, sigma0 / sqrt(fan_in) per layer (weights and biases)
__global__ __launch_bounds__(256) void noisy_sigma_init_kernel(float *__restrict__ p, NoisyNet N, int ne) {
    const int q = OFF_WF1 + blockIdx.x * 256 + threadIdx.x;
    if (q >= ne) return;
    p[N.n + q - OFF_WF1] = noisy_layer(N, q).sig;
}

// ---- per-env acting noise (fb_qnet_act_nib_env_noise, include/fbdqn.h): env e acts through mu + sigma (.) (f(eps_out_e) x f(eps_in_e))
// on fc1 and every head layer.  The mu part is the acting forward as it stands (mu materialised into params[0] for the call); what the
// noise adds: fc1's sigma term t[e][j] = sum_k sigma_W[k][j] f(eps_in_e,k) x[e][k] as a second fc1_sp_kernel launch over split planes of
// sigma_W_fc1 and of the scaled activations x (.) f(eps_in_e), and per-env noisy head logits (env_noise_head_kernel).
// Element k of env e at (seed, step): noise_draw_kernel's u1 / u2 / z / f(z) from Philox(key = seed, counter = (e nz + k, step_lo,
// FB_STREAM_ENV_NOISE, step_hi)).
__device__ __forceinline__ float env_noise_f(uint32_t seed_lo, uint32_t seed_hi, uint32_t c0, uint32_t step_lo, uint32_t step_hi) {
    const fb_u4 r = fb_philox(seed_lo, seed_hi, c0, step_lo, FB_STREAM_ENV_NOISE, step_hi);
    const float u1 = ((r.x >> 8) + 1) * (1.0f / 16777216.0f), u2 = (r.y >> 8) * (1.0f / 16777216.0f);
    const float z = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
    return copysignf(sqrtf(fabsf(z)), z);
}

// sigma_W_fc1 (sig: a base with sig + OFF_WF1 = sigma_W_fc1) into W_fc1's plane layout at wsp + WSP_WF1 (wsplit_item's fc1 items), unless
// *seen says they were built at the current Adam count (AdamDev::applies: every Adam update of the online net moves it; init / load
// reset *seen).  env_noise_scale_kernel, the next launch, records the count
__global__ __launch_bounds__(256) void env_noise_sigsplit_kernel(const float *__restrict__ sig, uint4 *__restrict__ wsp, int FC, const AdamDev *ad,
                                                                const int *seen) {
    if (*seen == ad->applies) return;
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id < 200 * FC) wsplit_item(sig, wsp, FC, IT_CONV + id);
}

// x (.) f(eps_in_e) of fc1 for every (env e < n, k < 1600), split as two fp16 planes ([plane][e][1600], plane stride pl) for
// fc1_sp_kernel.  x: conv3's output, from its two planes a3 (>= 256 states) or in fp32 from h3.  Two k per thread
struct EnvScale { const uint16_t *a3; const float *h3; size_t pl; uint16_t *out; int n, nz; uint32_t seed_lo, seed_hi, step_lo, step_hi;
                  const AdamDev *ad; int *seen; unsigned *ovf; };
__global__ __launch_bounds__(256) void env_noise_scale_kernel(EnvScale a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.seen = a.ad->applies;
    const int id = blockIdx.x * 256 + threadIdx.x, e = min(id / 800, a.n - 1), k = 2 * (id - (id / 800) * 800);
    const bool on = id < a.n * 800;
    const size_t o = (size_t)e * 1600 + k;
    float x0, x1;
    if (a.a3) {
        const uint32_t hi = *reinterpret_cast<const uint32_t *>(a.a3 + o), lo = *reinterpret_cast<const uint32_t *>(a.a3 + a.pl + o);
        const f32x2 h = __builtin_convertvector(__builtin_bit_cast(f16x2, hi), f32x2), l = __builtin_convertvector(__builtin_bit_cast(f16x2, lo), f32x2);
        x0 = fmaf(l.x, F16_LO_UNSCALE, h.x); x1 = fmaf(l.y, F16_LO_UNSCALE, h.y);
    } else { x0 = a.h3[o]; x1 = a.h3[o + 1]; }
    const uint32_t c = (uint32_t)e * (uint32_t)a.nz + (uint32_t)k;
    const float y0 = x0 * env_noise_f(a.seed_lo, a.seed_hi, c, a.step_lo, a.step_hi), y1 = x1 * env_noise_f(a.seed_lo, a.seed_hi, c + 1u, a.step_lo, a.step_hi);
    uint32_t hi, lo;
    split2x2(y0, y1, hi, lo);
    if (on) { *reinterpret_cast<uint32_t *>(a.out + o) = hi; *reinterpret_cast<uint32_t *>(a.out + a.pl + o) = lo; }
    note_overflow(on && out_of_f16_range(y0, y1, 0.f, 0.f), a.ovf);
}

// the per-env noisy head: one wave per env, c51_head_one's layout (lane i = atom i of every action).  h_j = relu((mu partials + b_j) +
// f(eps_out_j) (t_j + sigma_b_j)); the mu logits exactly as c51_logits forms them (P, hoff: the folded head for dueling C51), then each
// head layer's noise term f(eps_out_o) (sum_j sigma_W[j][o] f(eps_in_j) h_j + sigma_b_o) -- dueling C51: V_n + A_n - mean_a A_n per atom --
// added after it; softmax, Q, argmax and epsilon as c51_head_one.  sig: sigma of mu entry q at sig[q] (off: the net's own layout).
struct EnvNoiseHead {
    const float *hf, *ht; int stot, nks;     // mu fc1 partials [nks][stot][FC], sigma's t partials [FC1_SP_KS][stot][FC]
    const float *P; NetOff hoff; const float *sig; NetOff off; NoisyNet N;
    int n, FC, A; C51Sup sup; float *q; uint8_t *actions; float epsilon; uint32_t seed_lo, seed_hi, step_lo, step_hi;
    const int32_t *key_of; uint32_t stream;  // epsilon counter and noise: key_of[row] (or the row), epsilon on `stream`
};
// Eight envs per workgroup, one wave each.  The head's weights are the same for every env: the workgroup stages KC rows of the mu
// head, of sigma's Q / advantage layer and (dueling) of sigma's V layer in LDS at a time -- coalesced loads, one round trip per stage --
// and each wave runs its FMA chains from there (a wave that reads the rows from global memory itself waits on a round trip every few k)
constexpr int ENH_WAVES = 8;
template <int AT> struct EnhLds { static constexpr int KC = AT == 2 ? 64 : 16, PER = (KC * AT * 64 + 511) / 512, PERV = (KC * 64 + 511) / 512; };
template <int AT, bool DUEL>
__global__ __launch_bounds__(64 * ENH_WAVES) void env_noise_head_kernel(EnvNoiseHead H) {
    constexpr int KC = EnhLds<AT>::KC, PER = EnhLds<AT>::PER, PERV = EnhLds<AT>::PERV, WQ = KC * AT * 64;
    __shared__ float lw[2 * WQ + (DUEL ? KC * 64 : 0)];          // [mu rows | sigma rows | sigma V rows], row pitch AN (V: N)
    const int tid = threadIdx.x, lane = tid & 63, row = blockIdx.x * ENH_WAVES + (tid >> 6);
    const bool live = row < H.n;
    const int smp = live ? row : H.n - 1;                        // (a wave past n stages and waits with the others, stores nothing)
    const int A = AT == MAXA ? H.A : AT, N = H.sup.N, AN = A * N, il = lane < N ? lane : N - 1, FC = H.FC;
    const bool on = lane < N;
    const int key = H.key_of ? H.key_of[smp] : smp;
    const uint32_t base = (uint32_t)key * (uint32_t)H.N.nz;
    auto draw = [&](int k) { return env_noise_f(H.seed_lo, H.seed_hi, base + (uint32_t)k, H.step_lo, H.step_hi); };
    const NoisyLayer L0 = H.N.l[0], LV = H.N.l[1], LQ = H.N.l[DUEL ? 2 : 1];      // fc1, (V,) the Q / advantage layer
    float lg[AT], ns[AT], nv = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) { lg[a] = 0.f; ns[a] = 0.f; }
    float x = 0.f, xq = 0.f, xv = 0.f;
    for (int k0 = 0; k0 < FC; k0 += KC) {
        // rows k0 .. k0 + KC of the three matrices (contiguous: KC AN, KC AN, KC N floats): the loads go out first, none under a branch
        const int cq = KC * AN, cv = KC * N;
        const float *__restrict__ gm = H.P + H.hoff.wq + (size_t)k0 * AN, *__restrict__ gq = H.sig + H.off.wq + (size_t)k0 * AN;
        const float *__restrict__ gv = H.sig + H.off.wv + (size_t)k0 * N;
        float tm[PER], tq[PER], tv[DUEL ? PERV : 1];
#pragma unroll
        for (int r = 0; r < PER; r++) { const int i = min(tid + r * 512, cq - 1); tm[r] = gm[i]; tq[r] = gq[i]; }
        if (DUEL) {
#pragma unroll
            for (int r = 0; r < PERV; r++) tv[r] = gv[min(tid + r * 512, cv - 1)];
        }
        if (k0 % 64 == 0) {                                       // this wave's fc1 activations of units k0 .. k0 + 63 (lane = unit)
            const int j = k0 + lane;
            float v = H.hf[(size_t)smp * FC + j], t[FC1_KS];            // (fc1_out's sum, before its relu)
#pragma unroll
            for (int ks = 1; ks < FC1_KS; ks++) {
                const float y = H.hf[((size_t)(ks < H.nks ? ks : 0) * H.stot + smp) * FC + j];
                t[ks] = ks < H.nks ? y : 0.f;
            }
#pragma unroll
            for (int ks = 1; ks < FC1_KS; ks++) v += t[ks];
            const float pre = v + H.P[H.hoff.bf1 + j];
            float tt = H.ht[(size_t)smp * FC + j];
#pragma unroll
            for (int ks = 1; ks < FC1_SP_KS; ks++) tt += H.ht[((size_t)ks * H.stot + smp) * FC + j];
            x = fmaxf(pre + draw(L0.eout + j) * (tt + H.sig[H.off.bf1 + j]), 0.f);
            xq = x * draw(LQ.ein + j);
            xv = DUEL ? x * draw(LV.ein + j) : 0.f;
        }
        __syncthreads();                                          // (the previous stage's rows are no longer read)
#pragma unroll
        for (int r = 0; r < PER; r++) { const int i = tid + r * 512; if (i < cq) { lw[i] = tm[r]; lw[WQ + i] = tq[r]; } }
        if (DUEL) {
#pragma unroll
            for (int r = 0; r < PERV; r++) { const int i = tid + r * 512; if (i < cv) lw[2 * WQ + i] = tv[r]; }
        }
        __syncthreads();
        const int kl = k0 % 64;                                   // (the stage's first unit among the lanes of x)
#pragma unroll 8
        for (int k = 0; k < KC; k++) {                            // c51_logits' order of the mu sums: unit by unit
            const float xs = rdlane(x, kl + k), xqs = rdlane(xq, kl + k);
#pragma unroll
            for (int a = 0; a < AT; a++) {
                const int o = k * AN + (a < A ? a : 0) * N + il;
                lg[a] = fmaf(xs, lw[o], lg[a]);
                ns[a] = fmaf(xqs, lw[WQ + o], ns[a]);
            }
            if (DUEL) nv = fmaf(rdlane(xv, kl + k), lw[2 * WQ + k * N + il], nv);
        }
    }
#pragma unroll
    for (int a = 0; a < AT; a++) lg[a] += H.P[H.hoff.bq + (a < A ? a : 0) * N + il];
    float nq[AT], mean = 0.f;
#pragma unroll
    for (int a = 0; a < AT; a++) {
        const int o = (a < A ? a : 0) * N + il;
        nq[a] = draw(LQ.eout + o) * (ns[a] + H.sig[H.off.bq + o]);
        if (a < A) mean += nq[a];
    }
    if (DUEL) {
        mean /= (float)A;
        const float vn = draw(LV.eout + il) * (nv + H.sig[H.off.bv + il]);
#pragma unroll
        for (int a = 0; a < AT; a++) lg[a] += (vn + nq[a]) - mean;
    } else {
#pragma unroll
        for (int a = 0; a < AT; a++) lg[a] += nq[a];
    }
    float qv[AT];
    const float z = H.sup.vmin + (float)(on ? lane : 0) * H.sup.dz;
    c51_q<AT>(lg, on, z, qv);
    if (lane == 0 && live) {                                      // (c51_head_one's)
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

// ================================================================== fc1 + loss, small batches (training, < 256 states)
// fc1 with the WHOLE reduction in one workgroup.  Round 1's fc1_kernel split K = 1600 over 5 workgroups, which leaves five partial
// sums per unit that only a further launch can add up -- so Q (and with it the loss and every gradient) sat two launches
// behind fc1 (head_kernel, loss_head_kernel).  Here one workgroup owns a 16 x 16 output tile for all of K (its 8 waves split K
// and are summed through LDS in wave order), so it can finish what depends on the complete sums: it stores the pre-activation
// sums (slot 0 of the partial-sum buffer: nks = 1 for head_kernel / the env rider) and the tile's share of the head,
// qpart[row][tile][a] = sum over its 16 units of relu(sum + bias) * W_q[unit][a] (slot A: the same with W_v, dueling) -- row-major: the
// FC / 16 shares of one Q value are consecutive (fc1_bwd2_kernel's 16 lanes per row read 2 cache lines, not 16: with [tile][row] every
// workgroup of that launch spent ~2.5 us touching 3 000 lines for 36 KB of shares).
// fc1_bwd2_kernel adds the FC / 16 shares per row in its prologue: two launches and two round trips fewer per train step.
// The activation rows go through LDS (each wave stages its own 16 x 200 slice with 16-byte coalesced loads: a fragment-shaped
// global load would touch 64 cache lines per instruction); the weight columns are read directly (4 rows x 64 B per
// instruction).  v_mfma_f32_16x16x4_f32, two accumulators (40-cycle dependent latency against a 32-cycle issue interval).
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct FkArgs { Slices sl; const float *h3; float *hf; float *qpart; int FC, A, dueling, stot; NetOff off; };
constexpr int FK_ROW = 204;                   // LDS row stride of a wave's 16 x 200 slice (floats): conflict-free ds_read_b64

__global__ __launch_bounds__(512) void fc1_fk_kernel(FkArgs a) {
    __shared__ float ast[8 * 16 * FK_ROW];
    __shared__ float red[8 * 4 * 64];
    const Slice s = a.sl.s[blockIdx.z];
    const int M = s.count, m0 = blockIdx.x * 16, n0 = blockIdx.y * 16;
    if (m0 >= M) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
    const int kw = wave * 200;                                           // this wave's K range
    // weight column of this lane: k = kw + 50 g + t for MFMA t (lane group g supplies k index g of every step; A uses the same map)
    const float *bcol = s.params + OFF_WF1 + (size_t)(kw + 50 * g) * a.FC + n0 + r;
    float bv[50];
#pragma unroll
    for (int t = 0; t < 50; t++) bv[t] = bcol[(size_t)(FK_ABL == 2 ? 0 : t) * a.FC];
    // the head's parameters of this lane's unit (the epilogue's shares): requested with everything else, not behind the reduction
    float hb = s.params[a.off.bf1 + n0 + r], hw[MAXA + 1];
#pragma unroll
    for (int c = 0; c < MAXA; c++) hw[c] = s.params[a.off.wq + (n0 + r) * a.A + (c < a.A ? c : 0)];
    hw[MAXA] = s.params[(a.dueling ? a.off.wv : a.off.bf1) + n0 + r];
    // stage the activation slice: 16 rows x 50 float4; rows past the slice are clamped (computed, never stored)
    float *mine = ast + wave * 16 * FK_ROW;
    float4 st[13];
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const int idx = lane + 64 * i, row = idx < 800 ? idx / 50 : 0, c4 = idx < 800 ? idx - row * 50 : 0;
        const int mr = m0 + row < M ? m0 + row : M - 1;
        st[i] = *reinterpret_cast<const float4 *>(a.h3 + (size_t)(s.s_off + mr) * 1600 + kw + 4 * (FK_ABL == 3 ? 0 : c4));
    }
#pragma unroll
    for (int i = 0; i < 13; i++) {
        const int idx = lane + 64 * i, row = idx / 50, c4 = idx - row * 50;
        if (idx < 800) *reinterpret_cast<float4 *>(mine + row * FK_ROW + 4 * c4) = st[i];
    }
    __builtin_amdgcn_wave_barrier();                                     // the slice is this wave's own: no workgroup barrier
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const float *arow = mine + r * FK_ROW + 50 * g;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    float2 av[25];                                                       // every LDS read goes out before the first MFMA: the chain
#pragma unroll                                                           // must not wait for one read per step
    for (int t = 0; t < 25; t++) av[t] = *reinterpret_cast<const float2 *>(arow + 2 * t);
#pragma unroll
    for (int t = 0; t < 25; t++) { keep(av[t].x); keep(av[t].y); }
#pragma unroll
    for (int t = 0; t < (FK_ABL == 1 ? 1 : 25); t++) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(rbf(av[t].x, a.sl.rb), rbf(bv[2 * t], a.sl.rb), acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(rbf(av[t].y, a.sl.rb), rbf(bv[2 * t + 1], a.sl.rb), acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) red[(wave * 4 + q) * 64 + lane] = acc0[q] + acc1[q];
    __syncthreads();
    if (threadIdx.x >= 256) return;
    // thread (reg, lane) of the 16 x 16 tile: D[row = 4 (lane >> 4) + reg][col = lane & 15]; the 8 wave partials in wave order
    const int reg = threadIdx.x >> 6, row = 4 * g + reg, col = r, mr = m0 + row, unit = n0 + col;
    float v = red[reg * 64 + lane];
#pragma unroll
    for (int w = 1; w < 8; w++) v += red[(w * 4 + reg) * 64 + lane];
    const bool live = mr < M;
    const size_t srow = (size_t)s.s_off + (live ? mr : M - 1);
    if (live) a.hf[srow * a.FC + unit] = v;                              // pre-activation sum (bias and relu belong to the consumer)
    if (!a.qpart || FK_ABL == 4) return;
    const float h = fmaxf(v + hb, 0.f);
    const int qs = a.A + 1;
    float *qo = a.qpart + (srow * (size_t)gridDim.y + blockIdx.y) * qs;
#pragma unroll
    for (int c = 0; c <= MAXA; c++) {                                    // A columns of W_q (+ W_v for the dueling head)
        // (fully unrolled, static indices into hw: a loop the compiler cannot unroll turns hw into an alloca that hipcc parks in LDS)
        if (c < a.A || (c == a.A && a.dueling)) {                        // wave-uniform; no load inside
            float x = h * (c == a.A ? hw[MAXA] : hw[c]);
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) x += __shfl_xor(x, o, 16);   // over the tile's 16 units, fixed tree
            if (col == 0 && live) qo[c] = x;
        }
    }
}

// Loss + head backward + fc1 backward in ONE launch.  Every workgroup first rebuilds the B targets from the qpart shares (cheap:
// FC / 16 shares per Q value), i.e. what loss_head_kernel computed once and handed on through global memory; then the first n_dx
// workgroups compute a 32 x 32 tile of dh3 (they need dhf of their 32 rows for all units: rebuilt from the fc1 sums into LDS), the
// others eight 32 x 32 tiles of dW_fc1 in one 32-unit column block (dhf of all B rows for those 32 units).  The head's own
// gradients (W_q, b_q, W_v, b_v, b_fc1) come from the first dW workgroup of every column block; loss / abs_err / y and the Adam
// tick from workgroup 0.  Same arithmetic per element as loss_head_kernel + the fp32-MFMA fc1 backward it replaced.
struct Bw1Args {
    int algo, B, FC, A, dueling, stot, n_dx, rb;
    NetOff off;
    const float *params, *pnext, *ptarget;   // online net; the nets slice 1 (s') and slice 2 (Double: s' again) went through
    const float *hf, *qpart, *h3;
    const uint8_t *act; const float *rew; const uint8_t *term; const float *isw;
    double gamma;
    float *grad, *dh3, *loss, *abs_err, *y_out;
    AdamDev *adam; int tick;
    FbGate gate;                             // split schedule: the launch does not retire before the acting trunk on the other stream has (fb_gate_workgroup)
};
constexpr int BW_DX_ROW = 4;                 // + floats of padding per dhf row in LDS (dX role): conflict-free ds_read_b128
constexpr int BW_DW_ROW = 36;                // dhf row stride in LDS (dW role)

// DX: the role is a template argument and the kernel branches ONCE, at the top, into one of two straight-line bodies (a role branch
// around the pre-loads would put a vmcnt(0) join between them and the prologue's own loads)
template <int AT, bool DX, bool MD = false, bool DP = false, bool HU = false>
__device__ __forceinline__ void fc1_bwd2_body(const Bw1Args &L, float *smem, const MdPar M = MdPar{}, const float delta = 0.f) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = L.B, FC = L.FC, A = AT == MAXA ? L.A : AT;
    const float *P = L.params;
    float (*dadv)[MAXA] = reinterpret_cast<float (*)[MAXA]>(smem);                  // [MAXTB][MAXA]
    float *dv = smem + MAXTB * MAXA, *lterm = dv + MAXTB, *dadv2 = lterm + MAXTB, *big = dadv2 + 2 * MAXTB;     // big: role dependent
    // (dadv2: the two-action plain head's dA as packed pairs [b][2], 16-byte aligned per two rows)
    const bool lead = blockIdx.x == 0;
    const bool dbl = DP || L.algo == FB_ALGO_DOUBLE;
    const bool row3 = MD || dbl;                 // a third slice at rows 2B ..: Double's s' through the target net, Munchausen's (MD) s through it
    const int qs = A + 1, ntile = FC >> 4;
    // ---- role of this workgroup, and EVERY global load its body needs, issued before the target computation: the fc1 sums, the
    // unit parameters, the W_fc1 runs / h3 operands depend on nothing computed here, so the kernel makes one round trip to memory,
    // not three (shares -> dhf inputs -> MFMA operands)
    constexpr bool dx_role = DX;
    const int mt = dx_role ? blockIdx.x / 50 : 0, t2 = dx_role ? 0 : blockIdx.x - L.n_dx, nt = t2 / 7, kg = t2 - nt * 7;
    const int kt = dx_role ? blockIdx.x - mt * 50 : kg * 8 + wave;
    auto unit_params = [&](int n, float &bias, float (&wq)[AT], float &wv) {
        bias = P[L.off.bf1 + n];
        wv = P[(L.dueling ? L.off.wv : L.off.bf1) + n];
#pragma unroll
        for (int c = 0; c < AT; c++) wq[c] = P[L.off.wq + n * A + (c < A ? c : 0)];
    };
    float pre_hf[32], pre_bias, pre_wq[AT], pre_wv, pre_a[16];
    float4 pre_w[8];
    if constexpr (DX) {
        const int ch = FC < 512 ? FC : 512, n = tid < ch ? tid : 0;
#pragma unroll
        for (int q = 0; q < 32; q++) { const int bq_ = mt * 32 + q; pre_hf[q] = L.hf[(size_t)(bq_ < B ? bq_ : 0) * FC + n]; }
        unit_params(n, pre_bias, pre_wq, pre_wv);
        const int kh = ch / 16, nbeg = wave * (ch / 8) + (lane >> 5) * kh;
        const float *brun = P + OFF_WF1 + (size_t)(kt * 32 + (lane & 31)) * FC + nbeg;
#pragma unroll
        for (int q = 0; q < 8; q++) pre_w[q] = *reinterpret_cast<const float4 *>(brun + (4 * q < kh ? 4 * q : 0));
#pragma unroll
        for (int q = 0; q < 16; q++) pre_a[q] = 0.f;
        // relu'(h3) of the two output rows this wave finishes (reduce_rows deals rows 2 wave, 2 wave + 1 to wave < 8): requested now, not
        // behind the reduction at the very end of the longest role of this launch
#pragma unroll
        for (int q = 0; q < 2; q++) { const int mr = mt * 32 + drow(2 * (wave & 7) + q, lane); pre_a[q] = L.h3[(size_t)(mr < B ? mr : 0) * 1600 + kt * 32 + (lane & 31)]; }
    } else {
        const int c = tid & 31;
#pragma unroll
        for (int q = 0; q < 2; q++) { const int b = (tid >> 5) + 16 * q; pre_hf[q] = L.hf[(size_t)(b < B ? b : 0) * FC + nt * 32 + c]; }
#pragma unroll
        for (int q = 2; q < 32; q++) pre_hf[q] = 0.f;
        unit_params(nt * 32 + c, pre_bias, pre_wq, pre_wv);
        const int ktc = kt < 50 ? kt : 0;
#pragma unroll
        for (int t = 0; t < 16; t++) { const int b = 2 * t + (lane >> 5); pre_a[t] = L.h3[(size_t)(b < B ? b : 0) * 1600 + ktc * 32 + (lane & 31)]; }
#pragma unroll
        for (int q = 0; q < 8; q++) pre_w[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    // ---- targets: thread (b = tid >> 4, j = tid & 15) adds the shares of tiles j, j + 16, .. ; 16-lane tree; lane j == 0 finishes
    // No load under a branch and no load inside a loop of unknown trip count (hipcc waits vmcnt(0) at every such join: the first
    // version of this prologue made ~10 dependent round trips): the head biases of the three nets and the shares of the first two
    // tiles per lane (all of them for FC <= 512) are requested up front from clamped addresses and masked by selects.
    float bqs[AT], bqn[AT], bq3[AT];
#pragma unroll
    for (int c = 0; c < AT; c++) { const int cc = c < A ? c : 0; bqs[c] = L.params[L.off.bq + cc]; bqn[c] = L.pnext[L.off.bq + cc]; bq3[c] = L.ptarget[L.off.bq + cc]; }
    const int bvo = L.dueling ? L.off.bv : L.off.bq;
    float bvs = L.params[bvo], bvn = L.pnext[bvo], bv3 = L.ptarget[bvo];
    for (int b0 = 0; b0 < (BW_ABL == 1 ? 0 : B); b0 += 32) {
        const int b = b0 + (tid >> 4), j = tid & 15, bc = b < B ? b : 0;
        // the transition's reward / terminal / action ride with the shares
        float rf = L.rew[bc], isw = L.isw ? L.isw[bc] : 1.f;
        int termb = L.term[bc], a_b = L.act[bc];
        float x0[2][AT + 1], x1[2][AT + 1], x2[2][AT + 1];
#pragma unroll
        for (int u = 0; u < 2; u++) {
            const int tile = j + 16 * u, tc = tile < ntile ? tile : 0;
            const float *q0 = L.qpart + ((size_t)bc * ntile + tc) * qs;
            const size_t rs = (size_t)ntile * qs;                        // one row of shares
#pragma unroll
            for (int c = 0; c <= AT; c++) {
                const int cc = c < qs ? c : 0;
                x0[u][c] = q0[cc]; x1[u][c] = q0[(size_t)B * rs + cc]; x2[u][c] = q0[(size_t)(row3 ? 2 * B : 0) * rs + cc];
            }
        }
        keep(rf); keep(isw); keep(termb); keep(a_b);
        float qsv[AT + 1], qnv[AT + 1], q3v[AT + 1];
#pragma unroll
        for (int c = 0; c <= AT; c++) {
            keep(x0[0][c]); keep(x1[0][c]); keep(x2[0][c]); keep(x0[1][c]); keep(x1[1][c]); keep(x2[1][c]);
            // (FC = 128: 8 tiles, so lanes j >= 8 have no first share -- tc = 0 would count tile 0 again)
            const bool on = c < A || (c == A && L.dueling), on0 = on && j < ntile, on1 = on && j + 16 < ntile;
            qsv[c] = (on0 ? x0[0][c] : 0.f) + (on1 ? x0[1][c] : 0.f);
            qnv[c] = (on0 ? x1[0][c] : 0.f) + (on1 ? x1[1][c] : 0.f);
            q3v[c] = (on0 ? x2[0][c] : 0.f) + (on1 ? x2[1][c] : 0.f);
        }
        for (int tile = j + 32; tile < ntile; tile += 16) {              // FC > 512 only
            const float *q0 = L.qpart + ((size_t)bc * ntile + tile) * qs;
            const size_t rs = (size_t)ntile * qs;
#pragma unroll
            for (int c = 0; c <= AT; c++) {
                const int cc = c < qs ? c : 0;
                const bool on = c < A || (c == A && L.dueling);
                const float y0 = q0[cc], y1 = q0[(size_t)B * rs + cc], y2 = q0[(size_t)(row3 ? 2 * B : 0) * rs + cc];
                qsv[c] += on ? y0 : 0.f; qnv[c] += on ? y1 : 0.f; q3v[c] += on ? y2 : 0.f;
            }
        }
#pragma unroll
        for (int c = 0; c <= AT; c++)
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) { qsv[c] += __shfl_xor(qsv[c], o, 16); qnv[c] += __shfl_xor(qnv[c], o, 16); q3v[c] += __shfl_xor(q3v[c], o, 16); }
        // every lane finishes (no branch); only lane j == 0 of a live row publishes.  The V share sits in column A of the shares;
        // with AT == MAXA that index is a run-time one: select it out
        float vs = 0.f, vn = 0.f, v3 = 0.f;
#pragma unroll
        for (int c = 0; c <= AT; c++) { vs = c == A ? qsv[c] : vs; vn = c == A ? qnv[c] : vn; v3 = c == A ? q3v[c] : v3; }
        // biases / dueling combine (BrainDuelingDQN.py:78-86) like head_one, with the head parameters of the net each slice went
        // through: s -> online; s' -> online (DQN, Double's argmax) or target; Double's third slice -> target
        auto fin = [&](float (&qv)[AT + 1], float vshare, const float (&bq)[AT], float bvv) {
            float mean = 0.f;
#pragma unroll
            for (int c = 0; c < AT; c++) { qv[c] = c < A ? qv[c] + bq[c] : 0.f; mean += c < A ? qv[c] : 0.f; }
            const float V = vshare + bvv;
            mean /= (float)A;
#pragma unroll
            for (int c = 0; c < AT; c++) qv[c] = L.dueling ? V + (qv[c] - mean) : qv[c];
        };
        fin(qsv, vs, bqs, bvs);
        fin(qnv, vn, bqn, bvn);
        fin(q3v, v3, bq3, bv3);
        float sel;
        {
            int am = 0;                                              // BrainDoubleDQN.py:51-54
#pragma unroll
            for (int c = 1; c < AT; c++) if (c < A && qnv[c] > qnv[am]) am = c;
            float seld = q3v[0], selm = qnv[0];
#pragma unroll
            for (int c = 1; c < AT; c++) { seld = c == am ? q3v[c] : seld; selm = c < A ? fmaxf(selm, qnv[c]) : selm; }
            sel = dbl ? seld : selm;
        }
        if (L.algo != FB_ALGO_PER) isw = 1.f;
        // BrainDQN.py:210-215: python float64 arithmetic on the rewards 0.1 / 3 / -3, then fed as float32
        double rr = rf == 0.1f ? 0.1 : (double)rf;
        if constexpr (MD) {                                          // Munchausen: the soft bootstrap, and the log-policy bonus on the reward
            float bonus;
            mdqn_target<AT>(qnv, q3v, A, a_b, M, sel, bonus);
            rr += (double)bonus;
        }
        const double yd = termb ? rr : rr + L.gamma * (double)sel;
        const float y = (float)yd;
        float qe = qsv[0];
#pragma unroll
        for (int c = 1; c < AT; c++) qe = c == a_b ? qsv[c] : qe;
        const float d = y - qe;                                      // q_eval = reduce_sum(Q * onehot)
        const float scale = L.algo == FB_ALGO_DQN ? 2.f : 2.f / (float)B;     // sum vs mean
        const float gq = -scale * isw * td_clamp<HU>(d, delta);      // dLoss/dQ[b][a_b]
        // FB_ALGO_PG (BrainPolicyGradient.py:96-100; the actor of BrainActorCritic.py:96-100): Q(s) are LOGITS; loss = mean over
        // gamma (= the number of samples of the whole batch this chunk belongs to) of softmax_cross_entropy(logits, action) x weight,
        // the weight arriving where the rewards do.  dLoss/dlogit[c] = (softmax[c] - onehot[c]) x weight / N; these sum to 0 over c,
        // so a dueling head's V receives nothing and its advantages the same values.
        const bool pg = L.algo == FB_ALGO_PG;
        float pgp[AT], pgl;
        {
            float mx = qsv[0], se = 0.f;
#pragma unroll
            for (int c = 1; c < AT; c++) mx = c < A ? fmaxf(mx, qsv[c]) : mx;
#pragma unroll
            for (int c = 0; c < AT; c++) { pgp[c] = c < A ? expf(qsv[c] - mx) : 0.f; se += pgp[c]; }
#pragma unroll
            for (int c = 0; c < AT; c++) pgp[c] /= se;
            pgl = logf(se) - (qe - mx);                              // -log softmax[a_b]
        }
        const float pgw = rf / (float)L.gamma;
        if (j == 0 && b < B) {
            lterm[b] = pg ? pgl * pgw : td_term<HU>(isw, d, delta);
            if (lead && L.abs_err) L.abs_err[b] = fabsf(d);
            if (lead && L.y_out) L.y_out[b] = y;
            dv[b] = L.dueling && !pg ? gq : 0.f;
#pragma unroll
            for (int c = 0; c < AT; c++) dadv[b][c] = pg ? (pgp[c] - (c == a_b ? 1.f : 0.f)) * pgw : (c == a_b ? gq : 0.f) - (L.dueling ? gq / (float)A : 0.f);
            if (AT == 2) { dadv2[2 * b] = dadv[b][0]; dadv2[2 * b + 1] = dadv[b][1]; }
        }
    }
#pragma unroll
    for (int q = 0; q < 32; q++) keep(pre_hf[q]);
#pragma unroll
    for (int q = 0; q < 16; q++) keep(pre_a[q]);
#pragma unroll
    for (int q = 0; q < 8; q++) { keep(pre_w[q].x); keep(pre_w[q].y); keep(pre_w[q].z); keep(pre_w[q].w); }
    __syncthreads();
    if (lead && tid == 0) {
        float sum = 0.f;
        for (int b = 0; b < B; b++) sum += lterm[b];
        *L.loss = L.algo == FB_ALGO_DQN || L.algo == FB_ALGO_PG ? sum : sum / (float)B;       // (PG: the 1 / N is in every term)
        adam_tick(L.adam, L.tick);
    }
    if (lead && tid >= 64 && tid < 64 + A) { const int c = tid - 64; float sum = 0.f; for (int b = 0; b < B; b++) sum += dadv[b][c]; L.grad[L.off.bq + c] = sum; }
    if (lead && tid == 128 && L.dueling) { float sum = 0.f; for (int b = 0; b < B; b++) sum += dv[b]; L.grad[L.off.bv] = sum; }
    // dhf[b][n] = relu'(fc1) * (dV * W_v[n] + sum_a dA[a] * W_q[n][a]) from a pre-loaded fc1 sum and the unit's parameters
    auto dhf_of = [&](int b, float hfv, float bias, const float (&wq)[AT], float wv, float &hout) {
        const float v = hfv + bias;
        float d = L.dueling ? dv[b] * wv : 0.f;
#pragma unroll
        for (int c = 0; c < AT; c++) if (c < A) d = fmaf(dadv[b][c], wq[c], d);
        hout = fmaxf(v, 0.f);
        return v > 0.f ? d : 0.f;
    };
    const int hl = lane >> 5, i = lane & 31, jj = lane & 31;
    if constexpr (DX) {
        // ---- dh3[b][k] = (h3 > 0) * sum_n dhf[b][n] * W_fc1[k][n]: rows mt*32.., k tile kt; n in chunks of <= 512 units that the 8
        // waves split (each lane half a run of ch / 16 units).  Thread n of a chunk rebuilds column n of dhf for the 32 rows.
        const int RS = 512 + BW_DX_ROW;
        float *dh = big, *red = big + 32 * RS;
        f32x16 acc = {0};
        for (int nc = 0; nc < FC; nc += 512) {
            const int ch = FC - nc < 512 ? FC - nc : 512;
            if (nc) {                                                // (FC > 512 only: later chunks load inside the loop)
                __syncthreads();
                const int n = nc + (tid < ch ? tid : 0);
#pragma unroll
                for (int q = 0; q < 32; q++) { const int bq_ = mt * 32 + q; pre_hf[q] = L.hf[(size_t)(bq_ < B ? bq_ : 0) * FC + n]; }
                unit_params(n, pre_bias, pre_wq, pre_wv);
                const int kh = ch / 16, nbeg = wave * (ch / 8) + hl * kh;
                const float *brun = P + OFF_WF1 + (size_t)(kt * 32 + jj) * FC + nc + nbeg;
#pragma unroll
                for (int q = 0; q < 8; q++) pre_w[q] = *reinterpret_cast<const float4 *>(brun + (4 * q < kh ? 4 * q : 0));
            }
            if (tid < ch && BW_ABL != 2) {
                if (AT == 2 && !L.dueling) {
                    // two-action plain head: d = dA[b][0] * W_q[n][0] + dA[b][1] * W_q[n][1]; the 32 rows' (dA0, dA1) pairs arrive as 16
                    // broadcast ds_read_b128, all in flight, instead of 64 dependent scalar reads
                    float4 da[16];
#pragma unroll
                    for (int q = 0; q < 16; q++) da[q] = *reinterpret_cast<const float4 *>(dadv2 + 2 * (mt * 32 + 2 * q < MAXTB - 1 ? mt * 32 + 2 * q : 0));
                    float o[32];
#pragma unroll
                    for (int q = 0; q < 16; q++) {
                        const float v0 = pre_hf[2 * q] + pre_bias, v1 = pre_hf[2 * q + 1] + pre_bias;
                        const float d0 = fmaf(da[q].y, pre_wq[1], fmaf(da[q].x, pre_wq[0], 0.f)), d1 = fmaf(da[q].w, pre_wq[1], fmaf(da[q].z, pre_wq[0], 0.f));
                        o[2 * q] = (v0 > 0.f && mt * 32 + 2 * q < B) ? d0 : 0.f;
                        o[2 * q + 1] = (v1 > 0.f && mt * 32 + 2 * q + 1 < B) ? d1 : 0.f;
                    }
#pragma unroll
                    for (int q = 0; q < 32; q++) dh[q * RS + tid] = o[q];
                } else {
#pragma unroll
                    for (int q = 0; q < 32; q++) {
                        float hv;
                        dh[q * RS + tid] = mt * 32 + q < B ? dhf_of(mt * 32 + q, pre_hf[q], pre_bias, pre_wq, pre_wv, hv) : 0.f;
                    }
                }
            }
            __syncthreads();
            const int kh = ch / 16, nbeg = wave * (ch / 8) + hl * kh;
            const float *arun = dh + i * RS + nbeg;
            float4 xa[8];
#pragma unroll
            for (int q = 0; q < 8; q++) xa[q] = *reinterpret_cast<const float4 *>(arun + (4 * q < kh ? 4 * q : 0));
#pragma unroll
            for (int q = 0; q < 8; q++) { keep(xa[q].x); keep(xa[q].y); keep(xa[q].z); keep(xa[q].w); }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                if (4 * q < kh && BW_ABL != 3) {
                    const float4 x = xa[q], w = pre_w[q];
                    const bool rb = L.rb;
                    acc = mfma(rbf(x.x, rb), rbf(w.x, rb), acc); acc = mfma(rbf(x.y, rb), rbf(w.y, rb), acc);
                    acc = mfma(rbf(x.z, rb), rbf(w.z, rb), acc); acc = mfma(rbf(x.w, rb), rbf(w.w, rb), acc);
                }
            }
        }
        reduce_rows<8>(acc, red, wave, lane, mt * 32, B, [&](float v, int r, int mr) {
            const size_t o = (size_t)mr * 1600 + kt * 32 + jj;
            L.dh3[o] = BW_ABL == 4 ? v : (((r & 1) ? pre_a[1] : pre_a[0]) > 0.f ? v : 0.f);
        });
        return;
    }
    if (BW_ABL == 5) return;
    // ---- dW_fc1[k][n] = sum_b h3[b][k] * dhf[b][n]: column block nt (32 units), k tiles kg*8 + wave; + the head's gradients
    float *dh = big, *hh = big + MAXTB * BW_DW_ROW;                       // dhf and relu(fc1) of all B rows, 32 units
    {
        const int c = tid & 31;
#pragma unroll
        for (int q = 0; q < 2; q++) {
            const int b = (tid >> 5) + 16 * q;
            if (b < B) { float hv; dh[b * BW_DW_ROW + c] = dhf_of(b, pre_hf[q], pre_bias, pre_wq, pre_wv, hv); hh[b * BW_DW_ROW + c] = hv; }
        }
        for (int b = (tid >> 5) + 32; b < B; b += 16) {                 // B > 32: the rest of the rows (loads inside the loop)
            float hv;
            dh[b * BW_DW_ROW + c] = dhf_of(b, L.hf[(size_t)b * FC + nt * 32 + c], pre_bias, pre_wq, pre_wv, hv);
            hh[b * BW_DW_ROW + c] = hv;
        }
    }
    __syncthreads();
    if (kt < 50) {
        f32x16 acc = {0};
#pragma unroll
        for (int t = 0; t < 16; t++) {                                   // samples 0..31: A operands pre-loaded at the top
            const int b = 2 * t + hl;
            const float w = dh[(b < B ? b : 0) * BW_DW_ROW + jj];
            acc = mfma(b < B ? rbf(pre_a[t], L.rb) : 0.f, b < B ? rbf(w, L.rb) : 0.f, acc);
        }
#pragma unroll 4
        for (int t = 16; t < (B + 1) / 2; t++) {
            const int b = 2 * t + hl, bc = b < B ? b : 0;
            const float x = L.h3[(size_t)bc * 1600 + kt * 32 + i], w = dh[bc * BW_DW_ROW + jj];
            acc = mfma(b < B ? rbf(x, L.rb) : 0.f, b < B ? rbf(w, L.rb) : 0.f, acc);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) L.grad[OFF_WF1 + (size_t)(kt * 32 + drow(r, lane)) * FC + nt * 32 + jj] = acc[r];
    }
    if (kg != 0) return;
    // head gradients of units nt*32 .. +32: thread (c = tid & 31, part = tid >> 5) sums b = part, part + 16, ..; 16 parts in order
    float *part = hh + MAXTB * BW_DW_ROW;                                 // [16][32][AT + 2]
    {
        const int c = tid & 31, pt = tid >> 5;
        float gw[AT], gv = 0.f, gb = 0.f;
#pragma unroll
        for (int q = 0; q < AT; q++) gw[q] = 0.f;
        for (int b = pt; b < B; b += 16) {
            const float h = hh[b * BW_DW_ROW + c];
#pragma unroll
            for (int q = 0; q < AT; q++) if (q < A) gw[q] = fmaf(h, dadv[b][q], gw[q]);
            gv = fmaf(h, dv[b], gv);
            gb += dh[b * BW_DW_ROW + c];
        }
        float *po = part + (pt * 32 + c) * (AT + 2);
#pragma unroll
        for (int q = 0; q < AT; q++) po[q] = gw[q];
        po[AT] = gv; po[AT + 1] = gb;
    }
    __syncthreads();
    if (tid < 32) {
        const int n = nt * 32 + tid;
        float acc[AT + 2];
#pragma unroll
        for (int q = 0; q < AT + 2; q++) acc[q] = part[tid * (AT + 2) + q];
        for (int pt = 1; pt < 16; pt++)
#pragma unroll
            for (int q = 0; q < AT + 2; q++) acc[q] += part[(pt * 32 + tid) * (AT + 2) + q];
#pragma unroll
        for (int q = 0; q < AT; q++) if (q < A) L.grad[L.off.wq + n * A + q] = acc[q];
        if (L.dueling) L.grad[L.off.wv + n] = acc[AT];
        L.grad[L.off.bf1 + n] = acc[AT + 1];
    }
}

constexpr int BW_LDS_COMMON = MAXTB * MAXA + 4 * MAXTB;
constexpr int BW_LDS_DX = 32 * (512 + BW_DX_ROW) + 8 * 16 * 64, BW_LDS_DW = 2 * MAXTB * BW_DW_ROW + 16 * 32 * (MAXA + 2);
constexpr int BW_LDS = BW_LDS_COMMON + (BW_LDS_DX > BW_LDS_DW ? BW_LDS_DX : BW_LDS_DW);        // 27 264 floats = 109 KB

__global__ __launch_bounds__(512) void fc1_bwd2_kernel(Bw1Args L) {
    __shared__ float smem_bw[BW_LDS];
    if (fb_gate_workgroup(L.gate)) return;
    const bool dx = (int)blockIdx.x < L.n_dx;
    if (L.A == 2) { if (dx) fc1_bwd2_body<2, true>(L, smem_bw); else fc1_bwd2_body<2, false>(L, smem_bw); }
    else { if (dx) fc1_bwd2_body<MAXA, true>(L, smem_bw); else fc1_bwd2_body<MAXA, false>(L, smem_bw); }
}
// ... with the Munchausen target (FB_ALGO_MDQN / _PER): a kernel of its own, so that fc1_bwd2_kernel stays the code it was
__global__ __launch_bounds__(512) void fc1_bwd2_md_kernel(Bw1Args L, MdPar M) {
    __shared__ float smem_bw[BW_LDS];
    if (fb_gate_workgroup(L.gate)) return;
    const bool dx = (int)blockIdx.x < L.n_dx;
    if (L.A == 2) { if (dx) fc1_bwd2_body<2, true, true>(L, smem_bw, M); else fc1_bwd2_body<2, false, true>(L, smem_bw, M); }
    else { if (dx) fc1_bwd2_body<MAXA, true, true>(L, smem_bw, M); else fc1_bwd2_body<MAXA, false, true>(L, smem_bw, M); }
}
// ... with FB_ALGO_DOUBLE_PER's target (DP) and / or the Huber loss (HU): the extended kernel, as loss_head_x_kernel (the split
// schedule's gate workgroup included)
template <bool DP, bool HU, bool MD>
__global__ __launch_bounds__(512) void fc1_bwd2_x_kernel(Bw1Args L, MdPar M, float delta) {
    __shared__ float smem_bw[BW_LDS];
    if (fb_gate_workgroup(L.gate)) return;
    const bool dx = (int)blockIdx.x < L.n_dx;
    if (L.A == 2) { if (dx) fc1_bwd2_body<2, true, MD, DP, HU>(L, smem_bw, M, delta); else fc1_bwd2_body<2, false, MD, DP, HU>(L, smem_bw, M, delta); }
    else { if (dx) fc1_bwd2_body<MAXA, true, MD, DP, HU>(L, smem_bw, M, delta); else fc1_bwd2_body<MAXA, false, MD, DP, HU>(L, smem_bw, M, delta); }
}

#ifdef FB_QNET_X_TU
// fb_qnet_x.hip compiles this file up to here: the two extended kernels are instantiated in THAT translation unit, and so live in a code
// object of their own.  The code object of this file then holds exactly the kernels it held before the options existed, at the offsets
// they had -- a kernel added here moves every other one (the descriptors in front of the text grow), and the train chain's
// conv23_t_kernel and adam_fused_kernel measured 0.2 us slower each for that alone (profiles/huber_bench_parent_vs_new.txt).  The
// launchers take the argument structs as bytes: both units compile the same definitions above.
//
// Global-norm gradient clipping and the soft target update (include/fbdqn.h) live here for the same reason.
//   grad_sumsq_kernel   CLIP_WGS workgroups over the flat gradient, whatever its length: thread t of workgroup w squares the float4s
//                       w * 256 + t, + CLIP_WGS * 256, ... in float64 and adds them in that order; the workgroup adds its 256 sums in a
//                       fixed tree (clip_tree) and stores ONE float64 partial.  The n % 4 elements behind the last float4 go to the first
//                       threads of workgroup 0, behind their own range.  No atomics: the partials do not depend on timing
//   grad_clip_kernel    every workgroup adds the CLIP_WGS partials in the same tree, so all of them hold the same norm = (float) sqrt(sum)
//                       and c = G / max(norm, G) (c = 1 for G = 0 and for a norm that is not finite), and scales the float4s grad_sumsq's
//                       workgroup of the same index read; with c == 1 it stores nothing.  Workgroup 0 records (norm, c)
//   target_lerp_kernel  t += rho * (o - t) in fp32 over the whole master vector in one launch, float4 wide, the n % 4 tail by workgroup 0
constexpr int CLIP_WGS = 256;
__device__ __forceinline__ double clip_tree(double v, double *sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    return sh[0];
}
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float *__restrict__ g, long long n, double *__restrict__ part) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    const long long n4 = n >> 2;
    double acc = 0.0;
    for (long long q = (long long)blockIdx.x * 256 + tid; q < n4; q += (long long)CLIP_WGS * 256) {
        const float4 v = reinterpret_cast<const float4 *>(g)[q];
        acc += (double)v.x * (double)v.x; acc += (double)v.y * (double)v.y; acc += (double)v.z * (double)v.z; acc += (double)v.w * (double)v.w;
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) { const double x = (double)g[(n4 << 2) + tid]; acc += x * x; }
    const double s = clip_tree(acc, sh);
    if (tid == 0) part[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void grad_clip_kernel(float *__restrict__ g, long long n, const double *__restrict__ part, float G, float *__restrict__ out) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    static_assert(CLIP_WGS == 256, "one partial per thread");
    const float norm = (float)sqrt(clip_tree(part[tid], sh));
    // (a NaN norm fails both comparisons, an infinite one the second: c = 1.  The quotient of two floats, formed in float64 and rounded
    // once more, is the correctly rounded fp32 quotient)
    const bool on = G > 0.f && norm > G && norm <= 3.402823466e38f;
    const float c = on ? (float)((double)G / (double)norm) : 1.f;
    if (blockIdx.x == 0 && tid == 0) { out[0] = norm; out[1] = c; }
    if (c == 1.f) return;
    const long long n4 = n >> 2;
    for (long long q = (long long)blockIdx.x * 256 + tid; q < n4; q += (long long)CLIP_WGS * 256) {
        float4 v = reinterpret_cast<float4 *>(g)[q];
        v.x *= c; v.y *= c; v.z *= c; v.w *= c;
        reinterpret_cast<float4 *>(g)[q] = v;
    }
    if (blockIdx.x == 0 && tid < (int)(n & 3)) g[(n4 << 2) + tid] *= c;
}
__global__ __launch_bounds__(256) void target_lerp_kernel(float *__restrict__ t, const float *__restrict__ o, long long n, float rho) {
    const long long n4 = n >> 2, q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q < n4) {
        float4 a = reinterpret_cast<float4 *>(t)[q];
        const float4 b = reinterpret_cast<const float4 *>(o)[q];
        a.x += rho * (b.x - a.x); a.y += rho * (b.y - a.y); a.z += rho * (b.z - a.z); a.w += rho * (b.w - a.w);
        reinterpret_cast<float4 *>(t)[q] = a;
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) { const long long i = (n4 << 2) + threadIdx.x; t[i] += rho * (o[i] - t[i]); }
}
}  // namespace
void fb_qnet_launch_clip_x(hipStream_t st, float *g, long long n, double *part, float G, float *out) {
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(CLIP_WGS), dim3(256), 0, st, (const float *)g, n, part);
    hipLaunchKernelGGL(grad_clip_kernel, dim3(CLIP_WGS), dim3(256), 0, st, g, n, (const double *)part, G, out);
}
void fb_qnet_launch_target_lerp_x(hipStream_t st, float *t, const float *o, long long n, float rho) {
    hipLaunchKernelGGL(target_lerp_kernel, dim3((unsigned)(((n >> 2) + 255) / 256 > 0 ? ((n >> 2) + 255) / 256 : 1)), dim3(256), 0, st, t, o, n, rho);
}
void fb_qnet_launch_loss_head_x(int dp, int hu, int md, unsigned grid, hipStream_t st, const void *largs, const void *mdpar, float delta) {
    LossArgs L; MdPar M;
    memcpy(&L, largs, sizeof(L)); memcpy(&M, mdpar, sizeof(M));
    const dim3 g(grid), b(256);
    if (dp && hu) hipLaunchKernelGGL((loss_head_x_kernel<true, true, false>), g, b, 0, st, L, M, delta);
    else if (dp) hipLaunchKernelGGL((loss_head_x_kernel<true, false, false>), g, b, 0, st, L, M, 0.f);
    else if (hu && md) hipLaunchKernelGGL((loss_head_x_kernel<false, true, true>), g, b, 0, st, L, M, delta);
    else hipLaunchKernelGGL((loss_head_x_kernel<false, true, false>), g, b, 0, st, L, M, delta);
}
void fb_qnet_launch_fc1_bwd2_x(int dp, int hu, int md, unsigned grid, hipStream_t st, const void *largs, const void *mdpar, float delta) {
    Bw1Args L; MdPar M;
    memcpy(&L, largs, sizeof(L)); memcpy(&M, mdpar, sizeof(M));
    const dim3 g(grid), b(512);
    if (dp && hu) hipLaunchKernelGGL((fc1_bwd2_x_kernel<true, true, false>), g, b, 0, st, L, M, delta);
    else if (dp) hipLaunchKernelGGL((fc1_bwd2_x_kernel<true, false, false>), g, b, 0, st, L, M, 0.f);
    else if (hu && md) hipLaunchKernelGGL((fc1_bwd2_x_kernel<false, true, true>), g, b, 0, st, L, M, delta);
    else hipLaunchKernelGGL((fc1_bwd2_x_kernel<false, true, false>), g, b, 0, st, L, M, delta);
}
#else
// ================================================================== backward
// conv weight (+ bias) gradients: dW[(cell, ci)][co] = sum_m X[m @ cell][ci] * dY[m][co], db[co] = sum_m dY[m][co].
// One workgroup = one 32(ci) x 32(co) tile of one kernel cell; its 8 waves and the gridDim.y slabs split
// the reduction over output pixels m (each wave: one or two chunks of 16 MFMAs whose 32 operand loads are
// all issued before the first MFMA).  The last CO/32 workgroups of a launch are "bias tiles": their A
// operand is 1 in row 0, so row 0 of the tile is the column sum of dY.  Slabs are summed by
// slab_reduce_kernel in a fixed order.
template <int LAYER> struct DwGeom;
template <> struct DwGeom<2> { static constexpr int OH = 5, OW = 5, IH = 10, IW = 10, CI = 32, CO = 64, K = 4, S = 2, P = 1, WOFF = OFF_W2, BOFF = OFF_B2, CELLS = 16, CIT = 1; };
template <> struct DwGeom<3> { static constexpr int OH = 5, OW = 5, IH = 5, IW = 5, CI = 64, CO = 64, K = 3, S = 1, P = 1, WOFF = OFF_W3, BOFF = OFF_B3, CELLS = 9, CIT = 2; };

template <int LAYER>
__device__ __forceinline__ void conv_dw_body(int bx, int zslab, int nz, float *red, int B, const float *__restrict__ x,
                                             const float *__restrict__ dy, float *__restrict__ slabs, size_t slab_stride, bool rb = false) {
    using G = DwGeom<LAYER>;
    constexpr int COT = G::CO / 32, WTILES = G::CELLS * G::CIT * COT, OPIX = G::OH * G::OW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, i = lane & 31, j = lane & 31;
    const bool bias_tile = bx >= WTILES;
    int tile = bias_tile ? 0 : bx;
    const int cot = bias_tile ? bx - WTILES : tile % COT;
    tile /= COT;
    const int cit = tile % G::CIT, cell = tile / G::CIT;
    const int ky = cell / G::K, kx = cell - ky * G::K;
    const int M = B * OPIX, parts = nz * 8;
    int per = (M + parts - 1) / parts; per += per & 1;
    const int mbeg = wave < 8 ? (zslab * 8 + wave) * per : M;        // a 9th wave (merged launches) stays idle
    const int mend = mbeg + per < M ? mbeg + per : M;
    f32x16 acc = {0};
    for (int c0 = mbeg; c0 < mend; c0 += 32) {
        // every load of the chunk is issued unconditionally from a clamped (valid) address -- 48 loads in flight instead
        // of 48 dependent round trips -- pinned (keep), and only then masked by selects
        float a[16], bb[16], dv[16], xv[16];
        bool mok[16], in[16];
        // position c0 of the chunk is wave-uniform: its (sample, oy, ox) come from scalar divisions once; the 32 positions
        // of the chunk then only carry an offset d < 32 through two small mul-shift quotients (exact for the ranges that
        // can occur: OW = 5, d + ox0 < 64, oy0 + q < 32) instead of two 32-bit divisions per position and lane
        const int c0s = __builtin_amdgcn_readfirstlane(c0);
        const int b0 = c0s / OPIX, rem0 = c0s - b0 * OPIX, oy0 = rem0 / G::OW, ox0 = rem0 - oy0 * G::OW;
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int m0 = c0s + 2 * t + hl;
            mok[t] = m0 < mend;
            const int d = mok[t] ? 2 * t + hl : 0;                  // rows past the end recompute position c0 (valid) and are masked
            const int m = c0s + d;
            const int xs = ox0 + d, q = (xs * 205) >> 10, ox = xs - q * G::OW;
            const int ys = oy0 + q, qq = (ys * 205) >> 10, oy = ys - qq * G::OH, b = b0 + qq;
            const int iy = oy * G::S + ky - G::P;
            dv[t] = dy[(uint32_t)m * (uint32_t)G::CO + (uint32_t)(cot * 32 + j)];
            const int ix = ox * G::S + kx - G::P;
            in[t] = iy >= 0 && iy < G::IH && ix >= 0 && ix < G::IW;
            xv[t] = x[(((uint32_t)b * G::IH + (uint32_t)(in[t] ? iy : 0)) * G::IW + (uint32_t)(in[t] ? ix : 0)) * G::CI + (uint32_t)(cit * 32 + i)];
        }
        // the pins take the RAW loaded values (a conversion between a load and its pin drags the load down to the pin),
        // behind a scheduling fence
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 16; t++) { keep(dv[t]); keep(xv[t]); }
#pragma unroll
        for (int t = 0; t < 16; t++) {
            bb[t] = mok[t] ? dv[t] : 0.f;
            a[t] = bias_tile ? (mok[t] && i == 0 ? 1.f : 0.f) : (mok[t] && in[t] ? xv[t] : 0.f);
        }
#pragma unroll
        for (int t = 0; t < 16; t++) acc = mfma(rbf(a[t], rb), rbf(bb[t], rb), acc);
    }
    float *o = slabs + zslab * slab_stride;
    reduce_rows<8>(acc, red, wave, lane, 0, 32, [&](float v, int, int row32) {
        if (bias_tile) {
            if (row32 == 0) o[G::BOFF + cot * 32 + j] = v;                           // row 0 = column sums
        } else {
            const int row = cell * G::CI + cit * 32 + row32;
            o[G::WOFF + (size_t)row * G::CO + cot * 32 + j] = v;
        }
    });
}

// ---- conv3 and conv2 data gradients of ONE sample in one workgroup, on the transposed two-plane weights (every batch size:
// B = 256 is one workgroup per CU).
// dh3 (25 x 64) -> dh2 = relu2' * conv3^T(dh3) -> dp1 = relu1' * conv2^T(dh2), everything between the first load and the last store in
// LDS: the mirror image of conv23_t_kernel.  17 weight chunks of 64 k through the same 3-slot ring:
//   (weight fragments come straight from L2 into the one wave that uses them)
//   conv3^T: 9 chunks = taps, k = 64 output channels; 8 waves = 2 input-channel tiles x 4 k-steps;
//   conv2^T: stride 2 means input pixel (iy, ix) only meets taps with ky = iy + 1, kx = ix + 1 (mod 2): the 100 input pixels fall into
//            4 parity classes of 25 with 4 live taps each.  8 chunks = (which of the class's two ky, which kx, which half of the 64
//            output channels), each holding that tap of EVERY class; 8 waves = 4 classes x 2 k-steps.
// Side outputs dh2 / dp1 (fp32) feed the weight-gradient tiles of the next launch.
struct BxArgs { const float *dh3, *h2, *p1; float *dh2, *dp1; const uint4 *w3t, *w2t; };

template <int NS> struct BxLds { static constexpr int NPL = NS == 3 ? 2 : 1, U4 = 2 * NPL * 200 + 16 + 2048 + 4; };      // uint4 units (+ 4: the per-wave maxima of the gradient pre-scale)

// MODE 0: the launch's own role (dh2 / dp1 go to global memory for the weight-gradient launches that follow: batches > 64).
// MODE 1 / 2 (conv_bw_kernel, batches <= 64: the chain is the first part of a workgroup that goes on to weight gradients of ITS sample):
//   1  the whole chain; dp1 goes to `ldsout` (LDS of the caller, outside smem) as fp32 [100 pixels][32 channels];
//      `hook` runs behind the first barrier that follows the planes' first writes (the caller's LDS work that must follow ITS zeroing)
//   2  conv3^T only; dh2 goes to `ldsout` as fp32 [25 pixels][64 channels]
// Nothing is written to global memory in modes 1 / 2, and the caller places the barrier behind the LDS result.
struct NoHook { __device__ __forceinline__ void operator()() const {} };
template <int NS, int MODE = 0, class Hook = NoHook>
__device__ __forceinline__ void conv32_bx_body(const BxArgs &a, int b, uint4 *smem, float *ldsout = nullptr, Hook hook = Hook()) {
    constexpr int NPL = NS == 3 ? 2 : 1, P0 = NS == 3 ? 0 : 2;
    constexpr int C2_P = 200, D2O = NPL * C2_P, ZOFF = 2 * NPL * C2_P, RED = ZOFF + 16;
    constexpr int NCH = MODE == 2 ? 9 : 17;                                 // weight chunks this mode walks
    float *red = reinterpret_cast<float *>(smem + RED);
    float *sx = red + 8192;                                              // 8 + 8 words: per-wave maxima of dh3, then of dh2 (pow2_scale)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, j = lane & 31;
    const bool rowok = j < 25;
    // weight fragments: one wave per fragment, straight from L2, three chunks ahead (see conv23_t_kernel)
    struct WF { uint4 v[NPL]; };
    auto loadW = [&](int cc) {
        WF r;
        if (cc < 9) {                                                    // conv3^T: rows 8 cc + 2 kq + hl of W3T, columns of tile ct
            const int ct = wave & 1, kq = wave >> 1;
#pragma unroll
            for (int p = 0; p < NPL; p++) r.v[p] = a.w3t[((size_t)(8 * cc + 2 * kq + hl) * 3 + P0 + p) * 64 + ct * 32 + j];
        } else {                                                         // conv2^T: this class's tap (a2, b2), co half coh, k-step ks
            const int c2 = cc - 9, a2 = c2 >> 2, b2 = (c2 >> 1) & 1, coh = c2 & 1, cls = wave & 3, ks = wave >> 2;
            const int tap = ((((cls >> 1) + 1) & 1) + 2 * a2) * 4 + (((cls & 1) + 1) & 1) + 2 * b2;
#pragma unroll
            for (int p = 0; p < NPL; p++) r.v[p] = a.w2t[((size_t)(tap * 8 + coh * 4 + 2 * ks + hl) * 3 + P0 + p) * 32 + j];
        }
        return r;
    };
    // (PF chunks ahead.  A chunk is ~100 ns of work and an L2 round trip 600 - 800: at three ahead the loop waits for the weight stream --
    // 290 KB per chain, 1.9 us at a CU's 64 B / clock, the floor of this chain; conv_bw_kernel's roles go four ahead (five would pass 128 registers: one workgroup per CU).  Static indices
    // of a fully unrolled loop: registers, no alloca.)
    constexpr int PF = MODE == 0 ? 3 : 4;
    WF wq[PF];
#pragma unroll
    for (int q = 0; q < PF; q++) wq[q] = loadW(q);
    // roles of the two finishing passes, and the masks they need (requested now)
    const int ctA = wave & 1, qA = wave >> 1, chA = ctA * 32 + 8 * qA + 4 * hl;                 // conv3^T: channels chA .. + 3 of pixel j
    const float4 m2 = *reinterpret_cast<const float4 *>(a.h2 + ((size_t)b * 25 + (rowok ? j : 0)) * 64 + chA);
    const int clsB = wave & 3, halfB = wave >> 2, qy = j / 5, qx = j - qy * 5;
    const int pixB = ((clsB >> 1) + 2 * qy) * 10 + (clsB & 1) + 2 * qx, ciB = 16 * halfB + 4 * hl;   // conv2^T: channels ciB.. and ciB + 8..
    const float *p1p = a.p1 + ((size_t)b * 100 + (rowok && MODE != 2 ? pixB : 0)) * 32 + ciB;
    const float4 m1a = reinterpret_cast<const float4 *>(p1p)[0], m1b = reinterpret_cast<const float4 *>(p1p)[2];
    // The sample's gradients are tiny (1e-6 .. 1e-8 with a mean loss): the two-plane fp16 operands get an exact power-of-two pre-scale
    // from the sample's own maximum |dh3| (S3) and, further down, |dh2| (S2); 1 / S is folded back where a sum leaves the matrix
    // instruction (pow2_scale).  bf16 (NS = 1) has fp32's exponent range and needs none.
    Pow2 S3 = {1.f, 1.f}, S2 = {1.f, 1.f};
    {   // dh3 of the sample -> planes [25 pixels][8 pieces of 8 channels], piece q on q ^ ((pix >> 1) & 7)
        const int i = tid < 400 ? tid : 0, pix = i >> 4, q16 = i & 15;
        float4 t = reinterpret_cast<const float4 *>(a.dh3 + (size_t)b * 1600)[i];
        if constexpr (NS == 3) {
            wg_max_write(fmaxf(fmaxf(fabsf(t.x), fabsf(t.y)), fmaxf(fabsf(t.z), fabsf(t.w))), sx, wave, lane);
            __syncthreads();
            S3 = pow2_scale(wg_max_read<8>(sx));
            t.x *= S3.s; t.y *= S3.s; t.z *= S3.s; t.w *= S3.s;
        }
        uint32_t h0, l0, h1, l1, m_;
        if constexpr (NS == 3) { split2x2(t.x, t.y, h0, l0); split2x2(t.z, t.w, h1, l1); }
        else { split3x2(t.x, t.y, h0, m_, l0); split3x2(t.z, t.w, h1, m_, l1); }
        if (tid < 400) {
            uint2 *d = reinterpret_cast<uint2 *>(smem + pix * 8 + ((q16 >> 1) ^ ((pix >> 1) & 7))) + (q16 & 1);
            d[0] = make_uint2(h0, h1);
            if (NS == 3) d[2 * C2_P] = make_uint2(l0, l1);
        }
        if (tid < 16) smem[ZOFF + tid] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    hook();
    f32x16 acc = {0}, acl = {0};
    auto park = [&](int slot) {
#pragma unroll
        for (int r = 0; r < 16; r++) red[(slot * 16 + r) * 64 + lane] = NS == 3 ? fmaf(acl[r], F16_LO_UNSCALE, acc[r]) : acc[r];
#pragma unroll
        for (int r = 0; r < 16; r++) { acc[r] = 0.f; acl[r] = 0.f; }
        __syncthreads();
    };
    const int iyA = j / 5, ixA = j - iyA * 5;
#pragma unroll
    for (int cc = 0; cc < NCH; cc++) {
        int aidx[NPL];
        if (cc < 9) {                                                    // conv3^T, tap cc: output pixel = input pixel + 1 - tap
            const int kq = wave >> 1, ky = cc / 3, oy = iyA + 1 - ky, ox = ixA + 1 - (cc - 3 * ky), pix = oy * 5 + ox;
            const bool ok = rowok && oy >= 0 && oy < 5 && ox >= 0 && ox < 5;
#pragma unroll
            for (int p = 0; p < NPL; p++) aidx[p] = ok ? p * C2_P + pix * 8 + ((2 * kq + hl) ^ ((pix >> 1) & 7)) : ZOFF;
        } else {                                                         // conv2^T, this class's tap (a2, b2), co half coh, k-step ks
            const int c2 = cc - 9, a2 = c2 >> 2, b2 = (c2 >> 1) & 1, coh = c2 & 1, ks = wave >> 2;
            const int py = clsB >> 1, px = clsB & 1, ky = ((py + 1) & 1) + 2 * a2, kx = ((px + 1) & 1) + 2 * b2;
            const int ty = py + 2 * qy + 1 - ky, tx = px + 2 * qx + 1 - kx, oy = ty >> 1, ox = tx >> 1, pix = oy * 5 + ox;
            const bool ok = rowok && ty >= 0 && tx >= 0 && oy < 5 && ox < 5;
#pragma unroll
            for (int p = 0; p < NPL; p++) aidx[p] = ok ? D2O + p * C2_P + pix * 8 + ((coh * 4 + 2 * ks + hl) ^ ((pix >> 1) & 7)) : ZOFF;
        }
        uint4 A[NPL];
#pragma unroll
        for (int p = 0; p < NPL; p++) A[p] = smem[aidx[p]];
        const WF W = wq[cc % PF];
        if (cc + PF < NCH) wq[cc % PF] = loadW(cc + PF);
        if constexpr (NS == 3) {
            acl = mfma_h(W.v[0], A[1], acl);
            acl = mfma_h(W.v[1], A[0], acl);
            acc = mfma_h(W.v[0], A[0], acc);
        } else acc = mfma_b(W.v[0], A[0], acc);
        if (cc == 8) {
            // dh2: the four k partial sums per channel tile in k order, masked by relu2 (h2 > 0); fp32 out + planes for conv2^T
            park((wave >> 1) * 2 + (wave & 1));
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                v[e] = red[((0 * 2 + ctA) * 16 + 4 * qA + e) * 64 + lane];
#pragma unroll
                for (int k = 1; k < 4; k++) v[e] += red[((k * 2 + ctA) * 16 + 4 * qA + e) * 64 + lane];
            }
            v[0] = m2.x > 0.f ? v[0] : 0.f; v[1] = m2.y > 0.f ? v[1] : 0.f; v[2] = m2.z > 0.f ? v[2] : 0.f; v[3] = m2.w > 0.f ? v[3] : 0.f;
            if constexpr (MODE == 2) {                                   // the chain ends here: dh2 (true value) as fp32 in LDS
                if (rowok) *reinterpret_cast<float4 *>(ldsout + j * 64 + chA) = make_float4(v[0] * S3.inv, v[1] * S3.inv, v[2] * S3.inv, v[3] * S3.inv);
                return;
            }
            if constexpr (NS == 3) {
                // v = S3 * dh2.  Its planes get their own scale from the sample's maximum (the lanes of rows >= 25 hold sums over the
                // zero page: 0); what goes to memory is the true value
                wg_max_write(rowok ? fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3]))) : 0.f, sx + 8, wave, lane);
                __syncthreads();
                S2 = pow2_scale(wg_max_read<8>(sx + 8));
            }
            if (rowok) {
                if constexpr (MODE == 0) *reinterpret_cast<float4 *>(a.dh2 + ((size_t)b * 25 + j) * 64 + chA) = make_float4(v[0] * S3.inv, v[1] * S3.inv, v[2] * S3.inv, v[3] * S3.inv);
                if constexpr (NS == 3) { v[0] *= S2.s; v[1] *= S2.s; v[2] *= S2.s; v[3] *= S2.s; }
                uint32_t h0, l0, h1, l1, m_;
                if constexpr (NS == 3) { split2x2(v[0], v[1], h0, l0); split2x2(v[2], v[3], h1, l1); }
                else { split3x2(v[0], v[1], h0, m_, l0); split3x2(v[2], v[3], h1, m_, l1); }
                uint2 *d = reinterpret_cast<uint2 *>(smem + D2O + j * 8 + ((ctA * 4 + qA) ^ ((j >> 1) & 7))) + hl;
                d[0] = make_uint2(h0, h1);
                if (NS == 3) d[2 * C2_P] = make_uint2(l0, l1);
            }
            __syncthreads();                                             // dh2's planes are complete before conv2^T reads them
        }
    }
    // dp1: the two k-step partial sums per class, masked by relu1 through the pool (p1 > 0)
    park((wave >> 2) * 4 + (wave & 3));
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; e++) v[e] = (red[((0 * 4 + clsB) * 16 + 8 * halfB + e) * 64 + lane] + red[((1 * 4 + clsB) * 16 + 8 * halfB + e) * 64 + lane]) * S2.inv * S3.inv;
    if (rowok) {
        float *o = MODE == 1 ? ldsout + pixB * 32 + ciB : a.dp1 + ((size_t)b * 100 + pixB) * 32 + ciB;
        reinterpret_cast<float4 *>(o)[0] = make_float4(m1a.x > 0.f ? v[0] : 0.f, m1a.y > 0.f ? v[1] : 0.f, m1a.z > 0.f ? v[2] : 0.f, m1a.w > 0.f ? v[3] : 0.f);
        reinterpret_cast<float4 *>(o)[2] = make_float4(m1b.x > 0.f ? v[4] : 0.f, m1b.y > 0.f ? v[5] : 0.f, m1b.z > 0.f ? v[6] : 0.f, m1b.w > 0.f ? v[7] : 0.f);
    }
}

// ---- fc1 backward of a LARGE batch (256 samples; small ones: fc1_bwd2_kernel) on the fp16 matrix instruction, one wave per 32 x 32
// tile, operands split into two fp16 planes (NS = 3; NS = 1: rounded to bf16, one product) on the fly from fp32 rows that stay L2 resident
// (dhf 0.5 MB, h3 1.6 MB, W_fc1 3.3 MB) -- no staging, no reduction between waves, and the loads of four k-steps in flight while the
// previous four are in the MFMAs.  (The fp32-input MFMA version of this launch took 35 us at B = 256: two scalar loads in front of
// every 64-cycle MFMA, 32 dependent round trips per wave.)
//   data gradient    dh3[b][i] = (h3[b][i] > 0) * sum_n dhf[b][n] * W_fc1[i][n]: both operands are K-contiguous rows, 8 floats per lane
//   weight gradient  dW[i][n]  = sum_b h3[b][i] * dhf[b][n]: the reduction runs over samples, a lane gathers its 8 k-values with 8
//                    loads (each one coalesced across the 32 lanes of a half)
struct FragF { float4 a0, a1, b0, b1; };                // one k-step of one lane: 8 values of each operand
__device__ __forceinline__ float4 mul4(float4 v, float s) { return make_float4(v.x * s, v.y * s, v.z * s, v.w * s); }
// GA: which operand is the gradient (dhf) -- it is multiplied by the power of two `gs` before the split (pow2_scale), the caller folds
// 1 / gs back
template <int NS, bool GA>
__device__ __forceinline__ void mma_frag(FragF f, f32x16 &acc, f32x16 &acl, float gs, bool &bad) {
    if constexpr (NS == 3) {
        if constexpr (!GA) bad |= fmaxf(fmaxf(fmaxf(fabsf(f.a0.x), fabsf(f.a0.y)), fmaxf(fabsf(f.a0.z), fabsf(f.a0.w))), fmaxf(fmaxf(fabsf(f.a1.x), fabsf(f.a1.y)), fmaxf(fabsf(f.a1.z), fabsf(f.a1.w)))) >= FB_F16_RANGE;      // a = h3, an activation split unscaled
        if constexpr (GA) { f.a0 = mul4(f.a0, gs); f.a1 = mul4(f.a1, gs); } else { f.b0 = mul4(f.b0, gs); f.b1 = mul4(f.b1, gs); }
        uint4 ah, al, bh, bl;
        split2x2(f.a0.x, f.a0.y, ah.x, al.x); split2x2(f.a0.z, f.a0.w, ah.y, al.y); split2x2(f.a1.x, f.a1.y, ah.z, al.z); split2x2(f.a1.z, f.a1.w, ah.w, al.w);
        split2x2(f.b0.x, f.b0.y, bh.x, bl.x); split2x2(f.b0.z, f.b0.w, bh.y, bl.y); split2x2(f.b1.x, f.b1.y, bh.z, bl.z); split2x2(f.b1.z, f.b1.w, bh.w, bl.w);
        acl = mfma_h(ah, bl, acl);
        acl = mfma_h(al, bh, acl);
        acc = mfma_h(ah, bh, acc);
    } else {
        uint4 ah, bh; uint32_t m_, l_;
        split3x2(f.a0.x, f.a0.y, ah.x, m_, l_); split3x2(f.a0.z, f.a0.w, ah.y, m_, l_); split3x2(f.a1.x, f.a1.y, ah.z, m_, l_); split3x2(f.a1.z, f.a1.w, ah.w, m_, l_);
        split3x2(f.b0.x, f.b0.y, bh.x, m_, l_); split3x2(f.b0.z, f.b0.w, bh.y, m_, l_); split3x2(f.b1.x, f.b1.y, bh.z, m_, l_); split3x2(f.b1.z, f.b1.w, bh.w, m_, l_);
        acc = mfma_b(ah, bh, acc);
    }
}
// One workgroup per 32 x 32 tile, its 8 waves split the reduction (K = FC units for the data gradient, K = B samples for the weight
// gradient) and add their partial tiles through LDS in wave order (reduce_rows): a wave's chain is ONE group of loads, all in flight
// together, and a handful of MFMAs.  (One wave per tile walked 32 k-steps with a prefetch distance of one: 20 us at B = 256, the same in
// bf16 -- latency, not arithmetic; the fp32-MFMA kernel before that took 35 us.)
// KX / KW: k-steps per wave of the two roles as compile-time constants (FC / 128, B / 128), 0 = run-time counts.
template <int NS, int KX, int KW>
__global__ __launch_bounds__(512) void fc1_bwd_big_kernel(int n_dx, const float *__restrict__ params, const float *__restrict__ h3,
                                                          const float *__restrict__ dhf, float *__restrict__ dh3,
                                                          float *__restrict__ grad, int B, int FC, const float *__restrict__ gmax, unsigned *__restrict__ ovf) {
    __shared__ float red[8 * 16 * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, r = lane & 31;
    const int tile = blockIdx.x;
    f32x16 acc = {0}, acl = {0};
    bool bad = false;
    // pre-scale of the gradient operand: the maximum |dhf| of the whole matrix, from the loss kernel's per-workgroup maxima (FC / 16 <= 256
    // words: four per lane); requested here, consumed behind the fragment loads
    float gm = 0.f;
    {
        const int nm = FC >> 4;
        float g4[4];
#pragma unroll
        for (int q = 0; q < 4; q++) g4[q] = gmax[lane + 64 * q < nm ? lane + 64 * q : 0];
#pragma unroll
        for (int q = 0; q < 4; q++) gm = fmaxf(gm, g4[q]);
    }
    if (tile < n_dx) {
        const int mt = tile / 50, it = tile - mt * 50, m = mt * 32 + r;
        const int per = KX ? KX : FC / 128, k0 = wave * per;
        const float4 *pa = reinterpret_cast<const float4 *>(dhf + (size_t)(m < B ? m : 0) * FC + 8 * hl) + k0 * 4;
        const float4 *pb = reinterpret_cast<const float4 *>(params + OFF_WF1 + (size_t)(it * 32 + r) * FC + 8 * hl) + k0 * 4;
        auto ld = [&](int ks) { return FragF{pa[ks * 4], pa[ks * 4 + 1], pb[ks * 4], pb[ks * 4 + 1]}; };      // k-step k0 + ks: units 16 (k0 + ks) + 8 hl ..
        if constexpr (KX > 0) {
            FragF f[KX];
#pragma unroll
            for (int q = 0; q < KX; q++) f[q] = ld(q);
            const Pow2 G = pow2_scale(wave_max(gm));
#pragma unroll
            for (int q = 0; q < KX; q++) mma_frag<NS, true>(f[q], acc, acl, G.s, bad);
            if constexpr (NS == 3) {
#pragma unroll
                for (int q = 0; q < 16; q++) acc[q] = fmaf(acl[q], F16_LO_UNSCALE, acc[q]) * G.inv;
            }
        } else {
            const Pow2 G = pow2_scale(wave_max(gm));
            for (int q = 0; q < per; q++) mma_frag<NS, true>(ld(q), acc, acl, G.s, bad);
            if constexpr (NS == 3) {
#pragma unroll
                for (int q = 0; q < 16; q++) acc[q] = fmaf(acl[q], F16_LO_UNSCALE, acc[q]) * G.inv;
            }
        }
        reduce_rows<8>(acc, red, wave, lane, mt * 32, B, [&](float v, int, int mr) {
            const size_t o = (size_t)mr * 1600 + it * 32 + r;
            dh3[o] = h3[o] > 0.f ? v : 0.f;
        });
        return;
    }
    const int t = tile - n_dx, nt_n = FC / 32;
    const int it = t / nt_n, nt = t - it * nt_n;
    const float *pa = h3 + it * 32 + r, *pb = dhf + nt * 32 + r;
    const int per = KW ? KW : ((B + 15) / 16 + 7) / 8, k0 = wave * per;
    auto ld = [&](int ks) {                              // k-step k0 + ks: samples 16 (k0 + ks) + 8 hl .. + 7 (past the batch: row 0, zeroed)
        const int b0 = 16 * (k0 + ks) + 8 * hl;
        float a[8], bb[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const bool ok = b0 + j < B;
            const size_t bc = ok ? b0 + j : 0;
            const float x = pa[bc * 1600], y = pb[bc * FC];
            a[j] = ok ? x : 0.f; bb[j] = ok ? y : 0.f;
        }
        return FragF{make_float4(a[0], a[1], a[2], a[3]), make_float4(a[4], a[5], a[6], a[7]), make_float4(bb[0], bb[1], bb[2], bb[3]),
                     make_float4(bb[4], bb[5], bb[6], bb[7])};
    };
    const Pow2 G = pow2_scale(wave_max(gm));
    if constexpr (KW > 0) {
        FragF f[KW];
#pragma unroll
        for (int q = 0; q < KW; q++) f[q] = ld(q);
#pragma unroll
        for (int q = 0; q < KW; q++) mma_frag<NS, false>(f[q], acc, acl, G.s, bad);
    } else {
        for (int q = 0; q < per; q++) mma_frag<NS, false>(ld(q), acc, acl, G.s, bad);
    }
    if constexpr (NS == 3) {
#pragma unroll
        for (int q = 0; q < 16; q++) acc[q] = fmaf(acl[q], F16_LO_UNSCALE, acc[q]) * G.inv;
        note_overflow(bad, ovf);
    }
    reduce_rows<8>(acc, red, wave, lane, 0, 32, [&](float v, int, int row32) {
        grad[OFF_WF1 + (size_t)(it * 32 + row32) * FC + nt * 32 + r] = v;
    });
}

// TF ApplyAdam on four consecutive parameters (the one definition both Adam paths use)
__device__ __forceinline__ void adam4(float4 &P, float4 &Mv, float4 &V, const float4 Gv, float alpha, float omb1, float omb2, float eps) {
#define FB_ADAM1(c)                                  \
    Mv.c += (Gv.c - Mv.c) * omb1;                    \
    V.c += (Gv.c * Gv.c - V.c) * omb2;               \
    P.c -= (Mv.c * alpha) / (sqrtf(V.c) + eps);
    FB_ADAM1(x) FB_ADAM1(y) FB_ADAM1(z) FB_ADAM1(w)
#undef FB_ADAM1
}

// W_fc1 is 91 % of the parameters and its gradient is complete once the fc1 backward launch has run, while the launches
// that follow (conv3 / conv2 / conv1 backward) neither read W_fc1 nor fill more than ~200 of the 256 CUs, and wait on
// latency rather than on HBM.  Its Adam update therefore rides as extra workgroups at the END of the conv3 backward
// launch (float4 range [q0, q1) of the flat parameter vector); adam_fused_kernel at the end of the step skips that range.
struct AdamSpan { float *p, *m, *v; const float *g; const AdamDev *ad; int q0, q1; };
__device__ __forceinline__ void adam_span_body(int blk, int nblk, const AdamSpan a) {
    const float alpha = a.ad->alpha, omb1 = 1.f - a.ad->b1, omb2 = 1.f - a.ad->b2, eps = a.ad->eps;
    for (int q = a.q0 + blk * (int)blockDim.x + (int)threadIdx.x; q < a.q1; q += nblk * (int)blockDim.x) {
        float4 P = reinterpret_cast<float4 *>(a.p)[q], Mv = reinterpret_cast<float4 *>(a.m)[q], V = reinterpret_cast<float4 *>(a.v)[q];
        adam4(P, Mv, V, reinterpret_cast<const float4 *>(a.g)[q], alpha, omb1, omb2, eps);
        reinterpret_cast<float4 *>(a.p)[q] = P; reinterpret_cast<float4 *>(a.m)[q] = Mv; reinterpret_cast<float4 *>(a.v)[q] = V;
    }
}

// ---- conv1's weight gradient on the fp16 matrix cores, one sample per workgroup.
// dW1[(ky, kx, ci)][co] = sum over output pixels of x[4 oy + ky - 2][4 ox + kx - 2][ci] * dY[oy][ox][co], dY = the pooled gradient routed to
// each pool's maximum.  x is u8 -- exact in fp16 -- so with dY as two fp16 planes (split2x2) the products are exact and TWO
// v_mfma_f32_32x32x16_f16 per 16 pixels and weight-row tile replace the eight fp32 MFMAs (4x the cycles each) of the tiled kernel this replaced;
// more important at these sizes, the operands come out of LDS at fixed offsets instead of through per-pixel address arithmetic
// (that kernel spent ~750 vector instructions per 32 pixels and wave):
//   * the sample's 80 x 80 x 4 bytes are copied once into a zero-padded LDS image [84][100][4] (conv1's SAME padding + slack for the
//     padded pixel groups; rows of 416 bytes, pixel 0 at byte 16), so tap (ky, kx, ci) of 8 consecutive output pixels is 8 byte reads at base + 16 j;
//   * output rows are cut into 3 groups of 8 pixels (20 = 8 + 8 + 4, the last group padded with dY = 0): a lane's 8 k-values never
//     wrap a row; 30 MFMA steps per sample instead of 25;
//   * dY's fragments are the same for all 8 weight-row tiles (ky): each wave builds those of 4 steps (pool routing, split, bias sum)
//     into LDS, then wave ky walks all 30 steps.
// One slab per workgroup (two per sample), summed by the Adam kernel, through slab_fold_kernel when there are more than zmax.
constexpr int DW1_IMG_W = 104, DW1_IMG_H = 84, DW1_IMG = DW1_IMG_H * DW1_IMG_W * 4;      // bytes; 4 zero pixels left of column 0 (16-byte rows), 2 zero rows above
constexpr int DW1_STEPS = 30;

// NSP workgroups per sample (each takes 30 / NSP consecutive steps and writes its own slab: small batches want more than B workgroups)
template <int NSP> struct Dw1Lds { static constexpr int U4 = DW1_IMG / 16 + (DW1_STEPS / NSP) * 2 * 64 + 64 + 4; };      // uint4 units (+ 4: per-wave maxima of the gradient pre-scale)

// RING: the sample's image comes out of the replay's 1-bit frames (four frame offsets per sample in ring_fo, left by the trunk kernel)
struct Dw1Ring { const unsigned long long *bits, *fo; };
template <int NSP, bool RING = false>
__device__ __forceinline__ void conv1_dw2_body(int blk, const uint8_t *__restrict__ states, const float *__restrict__ dp1,
                                               const uint8_t *__restrict__ amax, float *__restrict__ slabs, size_t slab_stride, uint4 *pool,
                                               Dw1Ring ring = Dw1Ring{nullptr, nullptr}) {
    constexpr int SW = DW1_STEPS / NSP, PU = (SW + 7) / 8;       // steps of this workgroup; fragment-building rounds per wave
    uint4 *img4 = pool, *bfr = pool + DW1_IMG / 16;
    float (*bsum)[32] = reinterpret_cast<float (*)[32]>(bfr + SW * 2 * 64);
    float *sx = reinterpret_cast<float *>(bfr + SW * 2 * 64 + 64);      // per-wave maxima of |dY| (pow2_scale)
    const int b = blk / NSP, part = blk - b * NSP, s0 = part * SW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, c = lane & 31;
    uint8_t *img = reinterpret_cast<uint8_t *>(img4);
    // ---- this wave's share of the dY fragments: local steps wave, wave + 8, .. ; lane (c, hl) holds pixels (group 2 st + hl, ox0 .. ox0 + 7) of
    // channel c: 4 pooled pixels, each feeding the two window positions of its row.  All loads first.
    float dv[PU][4];
    int am[PU][4];
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int ls = wave + 8 * u, g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = (ox0 >> 1) + q;
            const bool ok = ls < SW && px < 10;
            const uint32_t po = ((uint32_t)b * 100u + (uint32_t)(ok ? (oy >> 1) * 10 + px : 0)) * 32u + (uint32_t)c;
            dv[u][q] = dp1[po]; am[u][q] = amax[po];
        }
    }
    {   // dY is a gradient (1e-7 .. 1e-9 in the reference's regime): its fp16 planes are built from S1 * dY, S1 a power of two from this
        // workgroup's maximum |dY| (pow2_scale); the maxima meet through LDS behind the barrier that follows the image's zeroing
        float m = 0.f;
#pragma unroll
        for (int u = 0; u < PU; u++)
#pragma unroll
            for (int q = 0; q < 4; q++) m = fmaxf(m, wave + 8 * u < SW ? fabsf(dv[u][q]) : 0.f);
        wg_max_write(m, sx, wave, lane);
    }
    // ---- the padded image: zero everything, then the 80 rows of 320 bytes
    // (named registers, not an array: hipcc parked a 4-entry uint4 array in scratch memory here)
    uint4 pxa, pxb, pxc, pxd;
    if constexpr (!RING) {
        const uint4 *sp = reinterpret_cast<const uint4 *>(states + (size_t)b * 25600);
        pxa = sp[tid]; pxb = sp[tid + 512]; pxc = sp[tid + 1024]; pxd = sp[tid + 1536 < 1600 ? tid + 1536 : 0];
    } else {
        // chunk i = 4 pixels x 4 frames: a nibble of each frame's bit row, expanded to 0 / 255 bytes (what the gather would have written)
        const unsigned long long f0 = ring.fo[b * 4], f1 = ring.fo[b * 4 + 1], f2 = ring.fo[b * 4 + 2], f3 = ring.fo[b * 4 + 3];
        auto chunk = [&](int i) {
            const int pp = (i < 1600 ? i : 0) * 4, w = pp >> 6, sh = pp & 63;
            const uint32_t n0 = (uint32_t)(ring.bits[f0 + w] >> sh) & 0xFu, n1 = (uint32_t)(ring.bits[f1 + w] >> sh) & 0xFu,
                           n2 = (uint32_t)(ring.bits[f2 + w] >> sh) & 0xFu, n3 = (uint32_t)(ring.bits[f3 + w] >> sh) & 0xFu;
            return make_uint4(expand4(n0, n1, n2, n3, 0), expand4(n0, n1, n2, n3, 1), expand4(n0, n1, n2, n3, 2), expand4(n0, n1, n2, n3, 3));
        };
        pxa = chunk(tid); pxb = chunk(tid + 512); pxc = chunk(tid + 1024); pxd = chunk(tid + 1536);
    }
    for (int i = tid; i < DW1_IMG / 16; i += 512) img4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    {
        auto put = [&](int i, const uint4 v) {                                       // 20 uint4 (4 pixels x 4 frames each) per image row
            const int row = i / 20, col4 = i - row * 20;
            if (i < 1600) *reinterpret_cast<uint4 *>(img + ((row + 2) * DW1_IMG_W + 4 + 4 * col4) * 4) = v;
        };
        put(tid, pxa); put(tid + 512, pxb); put(tid + 1024, pxc); put(tid + 1536, pxd);
    }
    const Pow2 S1 = pow2_scale(wg_max_read<8>(sx));
    float bs = 0.f;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int ls = wave + 8 * u, g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
        float v[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool ok = ls < SW && (ox0 >> 1) + q < 10;
            const int pos = (oy & 1) * 2;
            v[2 * q] = ok && am[u][q] == pos ? dv[u][q] : 0.f;
            v[2 * q + 1] = ok && am[u][q] == pos + 1 ? dv[u][q] : 0.f;
        }
        uint4 fh, fl;
        split2x2(v[0] * S1.s, v[1] * S1.s, fh.x, fl.x); split2x2(v[2] * S1.s, v[3] * S1.s, fh.y, fl.y);
        split2x2(v[4] * S1.s, v[5] * S1.s, fh.z, fl.z); split2x2(v[6] * S1.s, v[7] * S1.s, fh.w, fl.w);
        if (ls < SW) { bfr[(ls * 2 + 0) * 64 + lane] = fh; bfr[(ls * 2 + 1) * 64 + lane] = fl; }
#pragma unroll
        for (int q = 0; q < 8; q++) bs += v[q];
    }
    bs += __shfl_xor(bs, 32);
    if (hl == 0) bsum[wave][c] = bs;
    __syncthreads();
    // ---- wave ky: weight rows (ky, kx, ci) = lane & 31; tap byte of pixel j of its group at tap0 + 16 j.  Image row 4 oy + ky (= input row
    // 4 oy + ky - 2, two zero rows on top), column 4 ox + kx + 2 (= input column 4 ox + kx - 2, four zero pixels on the left).  The LDS
    // reads of step st + 1 are issued before the MFMAs of step st (they return in order: the wait for step st leaves them in flight).
    const int ky = wave, kx = c >> 2, ci = c & 3;
    const uint8_t *tapk = img + (ky * DW1_IMG_W + kx + 2) * 4 + ci;
    struct Ops { uint32_t x[8]; uint4 bh, bl; };
    auto fetch = [&](int ls) {
        const int g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
        const uint8_t *tap = tapk + ((4 * oy) * DW1_IMG_W + 4 * ox0) * 4;
        Ops o;
#pragma unroll
        for (int jq = 0; jq < 8; jq++) o.x[jq] = tap[16 * jq];
        o.bh = bfr[(ls * 2 + 0) * 64 + lane]; o.bl = bfr[(ls * 2 + 1) * 64 + lane];
        return o;
    };
    f32x16 acc = {0}, acl = {0};
    Ops cur = fetch(0);
#pragma unroll
    for (int ls = 0; ls < SW; ls++) {
        Ops nxt = cur;
        if (ls + 1 < SW) nxt = fetch(ls + 1);
        uint4 A;
        {
            const f32x2 p0 = {(float)cur.x[0], (float)cur.x[1]}, p1 = {(float)cur.x[2], (float)cur.x[3]};      // u8 -> fp16 is exact
            const f32x2 p2 = {(float)cur.x[4], (float)cur.x[5]}, p3 = {(float)cur.x[6], (float)cur.x[7]};
            A.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(p0, f16x2)); A.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(p1, f16x2));
            A.z = __builtin_bit_cast(uint32_t, __builtin_convertvector(p2, f16x2)); A.w = __builtin_bit_cast(uint32_t, __builtin_convertvector(p3, f16x2));
        }
        acc = mfma_h(A, cur.bh, acc);
        acl = mfma_h(A, cur.bl, acl);
        cur = nxt;
    }
    float *o = slabs + (size_t)blk * slab_stride;
#pragma unroll
    for (int r = 0; r < 16; r++) o[OFF_W1 + (ky * 32 + drow(r, lane)) * 32 + c] = fmaf(acl[r], F16_LO_UNSCALE, acc[r]) * S1.inv;
    if (wave == 0 && hl == 0) {
        float sum = bsum[0][c];
#pragma unroll
        for (int w = 1; w < 8; w++) sum += bsum[w][c];
        o[OFF_B1 + c] = sum;
    }
}

// ---- the conv backward of any batch in two launches (after fc1_bwd2_kernel / fc1_bwd_big_kernel; large batches add conv_dwg_kernel):
//   conv_bx_kernel    B workgroups run the per-sample data-gradient chain (conv32_bx_body); beside them the conv3 weight-gradient tiles
//                     (they need dh3 and h2 only), W_fc1's Adam span and, in fb_train_steps, the next step's random.sample
//   conv_dw21_kernel  the conv2 weight-gradient tiles (dh2 is complete now) and conv1's (dp1), side by side
template <int NS>
__global__ __launch_bounds__(512) void conv_bx_kernel(BxArgs bx, int B, int nz, float *__restrict__ slabs, size_t slab_stride, int n_adam,
                                                      AdamSpan span, FbSampleRider rider, int rb) {
    // one LDS pool for whichever role the workgroup has (separate static arrays would add up: with 134 KB per workgroup the ~400 Adam
    // workgroups of this launch went one per CU)
    __shared__ uint4 pool[BxLds<NS>::U4];
    static_assert(BxLds<NS>::U4 * 16 >= FB_SAMPLE_LDS_WORDS * 4 && BxLds<NS>::U4 >= 2048, "the riders borrow the pool");
    const int rid = rider.k ? 1 : 0, bid = (int)blockIdx.x - rid;
    if (bid < 0) {
        uint32_t *sw = reinterpret_cast<uint32_t *>(pool);
        if (threadIdx.x < 64) sample_cpython_body(rider.ctx, rider.k, rider.setsize, rider.out, sw, reinterpret_cast<int *>(sw + 624));
        return;
    }
    if (bid < B) { conv32_bx_body<NS>(bx, bid, pool); return; }
    const int t = bid - B;
    if (t < 38 * nz) {
        float *red = reinterpret_cast<float *>(pool);
        conv_dw_body<3>(t % 38, t / 38, nz, red, B, bx.h2, bx.dh3, slabs, slab_stride, rb);
        return;
    }
    adam_span_body(t - 38 * nz, n_adam, span);
}

template <int NSP, bool RING>
__global__ __launch_bounds__(512) void conv_dw21_kernel(int nz, int B, const float *__restrict__ p1, const float *__restrict__ dh2,
                                                        const uint8_t *__restrict__ states, const float *__restrict__ dp1,
                                                        const uint8_t *__restrict__ amax, float *__restrict__ slabs, size_t slab_stride,
                                                        float *__restrict__ slabs1, size_t stride1, int rb, Dw1Ring ring, FbGate gate) {
    if (fb_gate_workgroup(gate)) return;
    const int n2 = 34 * nz;                       // (slabs1 / stride1: where conv1's slabs go -- the common slab set, or the fold buffer)
    __shared__ uint4 pool[Dw1Lds<NSP>::U4];
    static_assert(Dw1Lds<NSP>::U4 >= 2048, "the conv2 tiles borrow the pool");
    if ((int)blockIdx.x < n2) {
        float *red = reinterpret_cast<float *>(pool);
        conv_dw_body<2>(blockIdx.x % 34, blockIdx.x / 34, nz, red, B, p1, dh2, slabs, slab_stride, rb);
        return;
    }
    if ((int)blockIdx.x < n2 + NSP * B) conv1_dw2_body<NSP, RING>((int)blockIdx.x - n2, states, dp1, amax, slabs1, stride1, pool, ring);
}

// ==================================================================================================================================
// ---- the conv backward of a SMALL batch (B <= 64) in ONE launch: conv_bw_kernel.
// conv_bx_kernel -> conv_dw21_kernel is a grid-wide seam only because the weight-gradient tiles above reduce over SAMPLES inside a tile,
// so every tile needs every sample's dh2 / dp1.  Per sample nothing crosses workgroups: dW3 of sample b needs dh3[b] and h2[b]; dW2 needs
// dh2[b] (the first half of b's data-gradient chain) and p1[b]; dW1 needs dp1[b] (the whole chain) and b's frames.  So sample b gets FOUR
// workgroups that share nothing and each write their own slab rows (Adam adds the B slabs in slab order, as it already does for conv1):
//   C1 x 2        the whole chain (conv32_bx_body, dp1 kept in LDS) -> conv1's weight gradient of half the output rows (conv1_dw2_body's
//                 arithmetic; its LDS image of the sample is built while the chain's first loads are in flight)     -> slabs 2b, 2b + 1
//   W2 x BW_NW2   conv3^T only (dh2 kept in LDS) -> its share of the 32 tiles of dW2[tap][ci][co] = sum over the 25 output pixels,
//                 fp32 MFMA from LDS-resident fp32 operands                                                          -> slab b
//   W3 x BW_NW3   no chain at all -> its share of the 36 tiles of dW3 likewise                                       -> slab b
// The chain is computed 2 + BW_NW2 times per sample -- on CUs that the old launches left idle (B = 32: 192 workgroups + the Adam span
// on 256 CUs) -- which is what lets every role start at once and removes the launch boundary between chain and tiles.  A tile costs a
// wave ~1.4 us (13 dependent 64-cycle MFMAs behind 26 LDS reads): with one workgroup per layer (4 - 5 tiles per wave) the tile roles,
// not the chain, set the launch's length (13 us alone against 9.3 for the chain; profiles/r04_notes.md), hence the split.
// dh2 / dp1 never go to global memory.  W_fc1's Adam span and fb_train_steps' sampler ride as in conv_bx_kernel.
constexpr int BW1_ROWS = 44, BW1_IMG_U4 = BW1_ROWS * DW1_IMG_W * 4 / 16;      // the image rows one half needs: 4 oy + ky, oy in [10 part, 10 part + 10)
constexpr int BW_NW2 = 2, BW_NW3 = 2, BW_WGS = 2 + BW_NW2 + BW_NW3;            // workgroups per sample
constexpr int BW_AUX_U4 = 1200, BW_DP1_U4 = 800;                             // aux: C1's image (1144) | W2's p1 + dh2 (800 + 400) | W3's dh3 + h2 (400 + 400)
template <int NS> struct BwLds { static constexpr int CH = BxLds<NS>::U4, U4 = CH + BW_AUX_U4 + BW_DP1_U4; };
static_assert(BW1_IMG_U4 <= BW_AUX_U4, "C1's image lives in the aux area");

// per-sample weight-gradient tiles from LDS-resident fp32 operands: xs[IH * IW][CI], dys[25][64]; wave w takes tiles w, w + 8, ..;
// k = output pixel, 13 steps of v_mfma_f32_32x32x2_f32 (lane half hl supplies pixel 2 t + hl; pixel 25 is padding)
#ifndef DWT_ABL
#define DWT_ABL 0
#endif
template <int LAYER>
__device__ __forceinline__ void dw_sample_tiles(const float *xs, const float *dys, float *__restrict__ o, bool rb, int sub, int nsub) {
    using G = DwGeom<LAYER>;
    constexpr int NT = DWT_ABL == 3 ? 8 : G::CELLS * G::CIT * 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane >> 5, i = lane & 31;
    for (int tile = wave + 8 * sub; tile < NT; tile += 8 * nsub) {          // workgroup `sub` of the `nsub` that share the sample's tiles
        const int cot = tile & 1, cit = G::CIT == 2 ? (tile >> 1) & 1 : 0, cell = tile / (2 * G::CIT), ky = cell / G::K, kx = cell - ky * G::K;
        float a[13], bb[13];
#pragma unroll
        for (int t = 0; t < 13; t++) {
            const int m = 2 * t + hl;
            const int oy = hl ? (2 * t + 1) / 5 : (2 * t) / 5, ox = hl ? (2 * t + 1) % 5 : (2 * t) % 5;
            const bool ok = t < 12 || hl == 0;
            const int iy = oy * G::S + ky - G::P, ix = ox * G::S + kx - G::P;
            const bool in = ok && iy >= 0 && iy < G::IH && ix >= 0 && ix < G::IW;
            const float xv = xs[(in ? iy * G::IW + ix : 0) * G::CI + cit * 32 + i], dv = dys[(ok ? m : 0) * 64 + cot * 32 + i];
            a[t] = in ? xv : 0.f; bb[t] = ok ? dv : 0.f;
        }
        f32x16 acc = {0};
        if (DWT_ABL == 1) { float sm = 0.f;
#pragma unroll
            for (int t = 0; t < 13; t++) sm += a[t] * bb[t];
#pragma unroll
            for (int r = 0; r < 16; r++) acc[r] = sm; }
        else {
#pragma unroll
        for (int t = 0; t < 13; t++) acc = mfma(rbf(a[t], rb), rbf(bb[t], rb), acc);
        }
        if (DWT_ABL == 2) { if (acc[0] == 12345.f) o[0] = acc[3]; continue; }
#pragma unroll
        for (int r = 0; r < 16; r++) o[G::WOFF + (size_t)(cell * G::CI + cit * 32 + drow(r, lane)) * G::CO + cot * 32 + i] = acc[r];
    }
}
// db[co] = sum over the 25 pixels of dys[pix][co], in pixel order
__device__ __forceinline__ void dw_sample_bias(const float *dys, float *__restrict__ ob) {
    if (threadIdx.x < 64) {
        float sum = dys[threadIdx.x];
#pragma unroll
        for (int m = 1; m < 25; m++) sum += dys[m * 64 + threadIdx.x];
        ob[threadIdx.x] = sum;
    }
}

// what conv1's weight-gradient half asks of global memory, requested before the chain: the pool positions of its dY fragments and its
// 840 image chunks (4 pixels x 4 frames each; part p needs input rows [40 p - 2, 40 p + 42) of the 80)
struct Bw1Pre { int am[2][4]; uint4 pxa, pxb; };
template <bool RING>
__device__ __forceinline__ Bw1Pre bw1_request(int b, int part, const uint8_t *__restrict__ states, const uint8_t *__restrict__ amax, Dw1Ring ring) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, c = lane & 31, s0 = part * 15;
    Bw1Pre r;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int ls = wave + 8 * u, g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = (ox0 >> 1) + q;
            const bool ok = ls < 15 && px < 10;
            r.am[u][q] = amax[((uint32_t)b * 100u + (uint32_t)(ok ? (oy >> 1) * 10 + px : 0)) * 32u + (uint32_t)c];
        }
    }
    const int i0 = part ? 760 : 0, ia = i0 + tid, ib = i0 + (tid < 328 ? 512 + tid : 0);
    if constexpr (!RING) {
        const uint4 *sp = reinterpret_cast<const uint4 *>(states + (size_t)b * 25600);
        r.pxa = sp[ia]; r.pxb = sp[ib];
    } else {
        const unsigned long long f0 = ring.fo[b * 4], f1 = ring.fo[b * 4 + 1], f2 = ring.fo[b * 4 + 2], f3 = ring.fo[b * 4 + 3];
        auto chunk = [&](int i) {
            const int pp = i * 4, w = pp >> 6, sh = pp & 63;
            const uint32_t n0 = (uint32_t)(ring.bits[f0 + w] >> sh) & 0xFu, n1 = (uint32_t)(ring.bits[f1 + w] >> sh) & 0xFu,
                           n2 = (uint32_t)(ring.bits[f2 + w] >> sh) & 0xFu, n3 = (uint32_t)(ring.bits[f3 + w] >> sh) & 0xFu;
            return make_uint4(expand4(n0, n1, n2, n3, 0), expand4(n0, n1, n2, n3, 1), expand4(n0, n1, n2, n3, 2), expand4(n0, n1, n2, n3, 3));
        };
        r.pxa = chunk(ia); r.pxb = chunk(ib);
    }
    return r;
}
// the chunks into the (zeroed) image: local row = input row + 2 - 40 part, 16-byte column 1 + chunk column
__device__ __forceinline__ void bw1_put(const Bw1Pre &pre, int part, uint4 *img4) {
    const int tid = threadIdx.x, i0 = part ? 760 : 0;
    auto put = [&](int i, const uint4 v) {
        const int row = i / 20, col4 = i - row * 20;
        img4[((row + 2 - 40 * part) * DW1_IMG_W + 4 + 4 * col4) / 4] = v;
    };
    put(i0 + tid, pre.pxa);
    if (tid < 328) put(i0 + 512 + tid, pre.pxb);
}
// conv1_dw2_body<2>'s arithmetic from the fragments on: dY = dp1 (LDS, fp32 [100][32]) routed to the pool maxima, two fp16 planes behind a
// power-of-two pre-scale from this workgroup's maximum; wave ky walks the 15 steps.  bfr: 15 x 2 x 64 + 64 + 4 uint4 (the chain's dead `red`).
__device__ __forceinline__ void bw1_main(int blk, int part, const Bw1Pre &pre, const float *dp1s, const uint4 *img4, uint4 *bfr,
                                         float *__restrict__ slabs, size_t slab_stride) {
    constexpr int SW = 15, PU = 2;
    float (*bsum)[32] = reinterpret_cast<float (*)[32]>(bfr + SW * 2 * 64);
    float *sx = reinterpret_cast<float *>(bfr + SW * 2 * 64 + 64);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, c = lane & 31, s0 = part * SW;
    const uint8_t *img = reinterpret_cast<const uint8_t *>(img4);
    float dv[PU][4];
    float m = 0.f;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int ls = wave + 8 * u, g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int px = (ox0 >> 1) + q;
            const bool ok = ls < SW && px < 10;
            dv[u][q] = dp1s[(ok ? (oy >> 1) * 10 + px : 0) * 32 + c];
            m = fmaxf(m, ls < SW ? fabsf(dv[u][q]) : 0.f);
        }
    }
    wg_max_write(m, sx, wave, lane);
    __syncthreads();
    const Pow2 S1 = pow2_scale(wg_max_read<8>(sx));
    float bs = 0.f;
#pragma unroll
    for (int u = 0; u < PU; u++) {
        const int ls = wave + 8 * u, g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
        float v[8];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool ok = ls < SW && (ox0 >> 1) + q < 10;
            const int pos = (oy & 1) * 2;
            v[2 * q] = ok && pre.am[u][q] == pos ? dv[u][q] : 0.f;
            v[2 * q + 1] = ok && pre.am[u][q] == pos + 1 ? dv[u][q] : 0.f;
        }
        uint4 fh, fl;
        split2x2(v[0] * S1.s, v[1] * S1.s, fh.x, fl.x); split2x2(v[2] * S1.s, v[3] * S1.s, fh.y, fl.y);
        split2x2(v[4] * S1.s, v[5] * S1.s, fh.z, fl.z); split2x2(v[6] * S1.s, v[7] * S1.s, fh.w, fl.w);
        if (ls < SW) { bfr[(ls * 2 + 0) * 64 + lane] = fh; bfr[(ls * 2 + 1) * 64 + lane] = fl; }
#pragma unroll
        for (int q = 0; q < 8; q++) bs += v[q];
    }
    bs += __shfl_xor(bs, 32);
    if (hl == 0) bsum[wave][c] = bs;
    __syncthreads();
    const int ky = wave, kx = c >> 2, ci = c & 3;
    const uint8_t *tapk = img + ((ky - 40 * part) * DW1_IMG_W + kx + 2) * 4 + ci;
    struct Ops { uint32_t x[8]; uint4 bh, bl; };
    auto fetch = [&](int ls) {
        const int g = 2 * (s0 + ls) + hl, oy = g / 3, ox0 = (g - 3 * oy) * 8;
        const uint8_t *tap = tapk + ((4 * oy) * DW1_IMG_W + 4 * ox0) * 4;
        Ops o;
#pragma unroll
        for (int jq = 0; jq < 8; jq++) o.x[jq] = tap[16 * jq];
        o.bh = bfr[(ls * 2 + 0) * 64 + lane]; o.bl = bfr[(ls * 2 + 1) * 64 + lane];
        return o;
    };
    f32x16 acc = {0}, acl = {0};
    Ops cur = fetch(0);
#pragma unroll
    for (int ls = 0; ls < SW; ls++) {
        Ops nxt = cur;
        if (ls + 1 < SW) nxt = fetch(ls + 1);
        uint4 A;
        {
            const f32x2 p0 = {(float)cur.x[0], (float)cur.x[1]}, p1 = {(float)cur.x[2], (float)cur.x[3]};      // u8 -> fp16 is exact
            const f32x2 p2 = {(float)cur.x[4], (float)cur.x[5]}, p3 = {(float)cur.x[6], (float)cur.x[7]};
            A.x = __builtin_bit_cast(uint32_t, __builtin_convertvector(p0, f16x2)); A.y = __builtin_bit_cast(uint32_t, __builtin_convertvector(p1, f16x2));
            A.z = __builtin_bit_cast(uint32_t, __builtin_convertvector(p2, f16x2)); A.w = __builtin_bit_cast(uint32_t, __builtin_convertvector(p3, f16x2));
        }
        acc = mfma_h(A, cur.bh, acc);
        acl = mfma_h(A, cur.bl, acl);
        cur = nxt;
    }
    float *o = slabs + (size_t)blk * slab_stride;
#pragma unroll
    for (int r = 0; r < 16; r++) o[OFF_W1 + (ky * 32 + drow(r, lane)) * 32 + c] = fmaf(acl[r], F16_LO_UNSCALE, acc[r]) * S1.inv;
    if (wave == 0 && hl == 0) {
        float sum = bsum[0][c];
#pragma unroll
        for (int w = 1; w < 8; w++) sum += bsum[w][c];
        o[OFF_B1 + c] = sum;
    }
}

// ablation switch (tools/abl_build.sh + tools/time_train_ring.py; 0 = the product): 1 C1 stops behind the chain, 2 W2 stops behind its
// chain, 3 W3 returns at once, 4 no Adam span, 5 C1 returns at once, 6 every role but the Adam span returns at once, 7 / 8 / 9 only W3 / W2 / C1 (+ the span), 10 / 11 only C1's / W2's chain
#ifndef CBW_ABL
#define CBW_ABL 0
#endif
template <int NS, bool RING>
__global__ __launch_bounds__(512) void conv_bw_kernel(BxArgs bx, int B, float *__restrict__ slabs, size_t slab_stride, float *__restrict__ slabs1,
                                                      size_t stride1, const uint8_t *__restrict__ states, const uint8_t *__restrict__ amax, Dw1Ring ring,
                                                      int n_adam, AdamSpan span, FbSampleRider rider, int rb, FbGate gate) {
    __shared__ uint4 pool[BwLds<NS>::U4];
    if (fb_gate_workgroup(gate)) return;
    static_assert(BwLds<NS>::U4 * 16 >= FB_SAMPLE_LDS_WORDS * 4, "the sampler rider borrows the pool");
    uint4 *aux = pool + BwLds<NS>::CH;
    float *dp1s = reinterpret_cast<float *>(aux + BW_AUX_U4);
    const int rid = rider.k ? 1 : 0, bid = (int)blockIdx.x - rid, tid = threadIdx.x;
    if (bid < 0) {
        uint32_t *sw = reinterpret_cast<uint32_t *>(pool);
        if (tid < 64) sample_cpython_body(rider.ctx, rider.k, rider.setsize, rider.out, sw, reinterpret_cast<int *>(sw + 624));
        return;
    }
    if (bid < 2 * B) {                                                       // C1: chain -> half of conv1's weight gradient
        if (CBW_ABL == 5 || CBW_ABL == 6 || CBW_ABL == 7 || CBW_ABL == 8 || CBW_ABL == 11) return;
        const int b = bid >> 1, part = bid & 1;
        const Bw1Pre pre = bw1_request<RING>(b, part, states, amax, ring);
        for (int i = tid; i < BW1_IMG_U4; i += 512) aux[i] = make_uint4(0u, 0u, 0u, 0u);
        conv32_bx_body<NS, 1>(bx, b, pool, dp1s);
        // the image's chunks hang on TWO dependent round trips (frame offsets -> bits): placed behind the chain, whose barriers have long
        // ordered them behind the zeroing, they never hold it up (as a hook behind the chain's second barrier they did); bw1_main's own
        // two barriers order them in front of the first tap read
        bw1_put(pre, part, aux);
        __syncthreads();                                                     // dp1 complete; the chain's reduction area is free
        if (CBW_ABL == 1 || CBW_ABL == 10) { if (dp1s[tid] == 12345.f) slabs1[0] = 1.f; return; }
        bw1_main(bid, part, pre, dp1s, aux, pool + (BwLds<NS>::CH - 2048 - 4), slabs1, stride1);
        return;
    }
    if (bid < (2 + BW_NW2) * B) {                                            // W2: conv3^T -> its share of dW2 (+ db2)
        if (CBW_ABL == 6 || CBW_ABL == 7 || CBW_ABL == 9 || CBW_ABL == 10) return;
        const int b = (bid - 2 * B) / BW_NW2, sub = (bid - 2 * B) - b * BW_NW2;
        float *p1s = reinterpret_cast<float *>(aux), *dys = p1s + 3200;
        const float4 *src = reinterpret_cast<const float4 *>(bx.p1 + (size_t)b * 3200);
        const float4 xa = src[tid], xb = src[tid < 288 ? 512 + tid : 0];
        reinterpret_cast<float4 *>(p1s)[tid] = xa;
        if (tid < 288) reinterpret_cast<float4 *>(p1s)[512 + tid] = xb;
        conv32_bx_body<NS, 2>(bx, b, pool, dys);
        __syncthreads();
        float *o = slabs + (size_t)b * slab_stride;
        if (CBW_ABL == 2 || CBW_ABL == 11) { if (dys[tid] == 12345.f) o[0] = 1.f; return; }
        dw_sample_tiles<2>(p1s, dys, o, rb, sub, BW_NW2);
        if (sub == BW_NW2 - 1) dw_sample_bias(dys, o + OFF_B2);                // (the workgroup with the fewest tiles)
        return;
    }
    if (bid < BW_WGS * B) {                                                  // W3: its share of dW3 (+ db3) from dh3 and h2 alone
        if (CBW_ABL == 3 || CBW_ABL == 6 || CBW_ABL == 8 || CBW_ABL == 9 || CBW_ABL == 10 || CBW_ABL == 11) return;
        const int b = (bid - (2 + BW_NW2) * B) / BW_NW3, sub = (bid - (2 + BW_NW2) * B) - b * BW_NW3;
        float *dys = reinterpret_cast<float *>(aux), *xs = dys + 1600;
        const int q = tid < 400 ? tid : 0;
        const float4 d = reinterpret_cast<const float4 *>(bx.dh3 + (size_t)b * 1600)[q], x = reinterpret_cast<const float4 *>(bx.h2 + (size_t)b * 1600)[q];
        if (tid < 400) { reinterpret_cast<float4 *>(dys)[tid] = d; reinterpret_cast<float4 *>(xs)[tid] = x; }
        __syncthreads();
        float *o = slabs + (size_t)b * slab_stride;
        dw_sample_tiles<3>(xs, dys, o, rb, sub, BW_NW3);
        if (sub == BW_NW3 - 1) dw_sample_bias(dys, o + OFF_B3);
        return;
    }
    if (CBW_ABL == 4) return;
    adam_span_body(bid - BW_WGS * B, n_adam, span);
}

// ---- conv3 / conv2 weight gradients of a LARGE batch (B a multiple of 16): one workgroup per group of 16 samples and 32 x 32 tile of
// (input channel, output channel) [conv2: and per parity class of input pixels], on the fp16 matrix instruction with the SAMPLES as the
// reduction dimension of one MFMA: dW[tap][ci][co] = sum over pixels of ( sum over the 16 samples of x[b][pixel + tap][ci] * dY[b][pixel][co] ),
// so with both operands parked in LDS as planes [pixel][channel][16 samples] every fragment is ONE 16-byte read at a computed address
// -- no im2col gather -- and a (tap, pixel) pair is one MFMA step (three products; NS = 1: one bf16 product).  Each workgroup reads its
// 16 samples' x and dY once (13 MB from L2 per layer at B = 256; the tiled fp32-MFMA kernels re-read them per tile: ~60 MB per layer,
// 950 + 850 workgroups that each ran one 16-MFMA chunk per wave) and walks all its taps: conv3 9 taps over 8 waves (wave 0 takes the
// two corner taps 0 and 8), conv2 the 4 taps that meet its parity class x 2 halves of the pixels.  One slab per sample group.
template <int NS> struct DwgLds {
    static constexpr int NPL = NS == 3 ? 2 : 1, PLH = 25 * 32 * 16;             // halves per plane of one operand
    static constexpr int U4 = 2 * NPL * PLH / 8 + 64 + 128 + 2048 + 4;           // + a zero page (1 KB) + bias partials (512 floats) + the reduction area (8 x 16 x 64 floats) + per-wave maxima (pre-scale)
};

// LAYER 3: blk = (group, ci tile, co tile); LAYER 2: blk = (group, parity class, co tile)
template <int NS, int LAYER>
__device__ __forceinline__ void conv_dwg_body(int blk, const float *__restrict__ x, const float *__restrict__ dy, float *__restrict__ slabs,
                                              size_t slab_stride, uint4 *pool, unsigned *ovf) {
    constexpr int NPL = DwgLds<NS>::NPL, PLH = DwgLds<NS>::PLH, ZERO = 2 * NPL * PLH;      // (halves)
    uint16_t *X = reinterpret_cast<uint16_t *>(pool), *DY = X + NPL * PLH;
    float *part = reinterpret_cast<float *>(pool + 2 * NPL * PLH / 8 + 64);
    float *red = part + 512;
    float *sx = red + 8192;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hl = lane >> 5, r = lane & 31;
    const int cot = blk & 1, mid = LAYER == 3 ? (blk >> 1) & 1 : (blk >> 1) & 3, g = LAYER == 3 ? blk >> 2 : blk >> 3;
    const int py = mid >> 1, px = mid & 1;                                   // (LAYER 2: the parity class)
    // ---- the group's operands into LDS as planes [pixel][channel][16 samples].  Item = (pixel, channel, PAIR of samples): two scalar
    // loads (a half wave reads 32 consecutive channels = 128 B), one packed 4-byte write per plane; lanes of a write are 32 B apart
    // (4-way bank conflicts; float4 loads with 2-byte writes measured 32-way and made this kernel slower than the tiles it replaces).
    // Wave-item w = (pixel w % 25, pair quartet w / 25); lane (channel r, hl): sample pair w / 25 + 4 hl.
    float xa[13], xb[13], ya[13], yb[13];
#pragma unroll
    for (int q = 0; q < 13; q++) {
        const int w = wave + 8 * q, wc = w < 100 ? w : 0, pos = wc % 25, bp = wc / 25 + 4 * hl;
        const size_t s0 = (size_t)g * 16 + 2 * bp;
        size_t xo;
        if (LAYER == 3) xo = (s0 * 25 + pos) * 64 + mid * 32 + r;
        else { const int qy = pos / 5, qx = pos - qy * 5; xo = (s0 * 100 + (py + 2 * qy) * 10 + px + 2 * qx) * 32 + r; }
        const size_t yo = (s0 * 25 + pos) * 64 + cot * 32 + r;
        xa[q] = x[xo]; xb[q] = x[xo + (LAYER == 3 ? 1600 : 3200)];
        ya[q] = dy[yo]; yb[q] = dy[yo + 1600];
    }
    if (tid < 64) pool[2 * NPL * PLH / 8 + tid] = make_uint4(0u, 0u, 0u, 0u);
    // dY is a gradient: its two fp16 planes are built from SY * dY, SY a power of two from the maximum |dY| of this workgroup's operand
    // block (16 samples x 25 pixels x 32 channels), folded back in fold() (pow2_scale); x is an activation and needs none
    Pow2 SY = {1.f, 1.f};
    if constexpr (NS == 3) {
        float m = 0.f;
#pragma unroll
        for (int q = 0; q < 13; q++) m = fmaxf(m, wave + 8 * q < 100 ? fmaxf(fabsf(ya[q]), fabsf(yb[q])) : 0.f);
        wg_max_write(m, sx, wave, lane);
        __syncthreads();
        SY = pow2_scale(wg_max_read<8>(sx));
    }
    float bs = 0.f;
    bool bad = false;                                                          // x is an activation, split unscaled: range guard (note_overflow)
#pragma unroll
    for (int q = 0; q < 13; q++) {
        const int w = wave + 8 * q, pos = w % 25, bp = w / 25 + 4 * hl;
        if (w < 100) {
            const int o = (pos * 32 + r) * 16 + 2 * bp;
            uint32_t h0, l0, h1, l1, m_;
            if constexpr (NS == 3) { split2x2(xa[q], xb[q], h0, l0); split2x2(ya[q] * SY.s, yb[q] * SY.s, h1, l1); bad |= fmaxf(fabsf(xa[q]), fabsf(xb[q])) >= FB_F16_RANGE; }
            else { split3x2(xa[q], xb[q], h0, m_, l0); split3x2(ya[q], yb[q], h1, m_, l1); }
            *reinterpret_cast<uint32_t *>(X + o) = h0; *reinterpret_cast<uint32_t *>(DY + o) = h1;
            if (NS == 3) { *reinterpret_cast<uint32_t *>(X + PLH + o) = l0; *reinterpret_cast<uint32_t *>(DY + PLH + o) = l1; }
            bs += ya[q] + yb[q];
        }
    }
    part[tid] = bs;                                                            // (all items of a thread share its channel r: 512 % 64 == 0)
    if constexpr (NS == 3) note_overflow(bad, ovf);
    __syncthreads();
    float *o = slabs + (size_t)g * slab_stride;
    if (mid == 0 && tid < 32) {                                                // bias gradient of the co tile: column sums of dY, fixed order
        float sum = 0.f;
        for (int k = 0; k < 16; k++) sum += part[tid + 32 * k];
        o[(LAYER == 3 ? OFF_B3 : OFF_B2) + cot * 32 + tid] = sum;
    }
    // fragment of pixel `pos` (pos < 0: the zero page -- a tap that falls off the image; no branch, so the 25 steps unroll and their LDS
    // reads run ahead of the MFMAs)
    auto frag = [&](const uint16_t *base, int p, int pos) {
        return *reinterpret_cast<const uint4 *>(pos < 0 ? X + ZERO + 8 * hl : base + p * PLH + (pos * 32 + r) * 16 + 8 * hl);
    };
    f32x16 acc = {0}, acl = {0};
    auto step = [&](int xpos, int pix) {
        if constexpr (NS == 3) {
            const uint4 ah = frag(X, 0, xpos), al = frag(X, 1, xpos), bh = frag(DY, 0, pix), bl = frag(DY, 1, pix);
            acl = mfma_h(ah, bl, acl); acl = mfma_h(al, bh, acl); acc = mfma_h(ah, bh, acc);
        } else acc = mfma_b(frag(X, 0, xpos), frag(DY, 0, pix), acc);
    };
    auto fold = [&]() {
        if constexpr (NS == 3) {
#pragma unroll
            for (int q = 0; q < 16; q++) acc[q] = fmaf(acl[q], F16_LO_UNSCALE, acc[q]) * SY.inv;
        }
    };
    if constexpr (LAYER == 3) {
        // wave w: tap w over all 25 pixels, plus pixels 3 w .. 3 w + 2 (wave 7: .. 24) of the ninth tap into a second accumulator pair whose
        // eight partial sums meet through LDS (one wave doing two whole taps made the workgroup wait for it: 50 steps against 25)
        {
            const int ky = wave / 3, kx = wave - 3 * ky;
#pragma unroll
            for (int pix = 0; pix < 25; pix++) {
                const int oy = pix / 5, ox = pix - oy * 5, iy = oy + ky - 1, ix = ox + kx - 1;
                step(iy >= 0 && iy < 5 && ix >= 0 && ix < 5 ? iy * 5 + ix : -1, pix);
            }
            fold();
#pragma unroll
            for (int q = 0; q < 16; q++) o[OFF_W3 + (size_t)((wave * 64 + mid * 32 + drow(q, lane)) * 64) + cot * 32 + r] = acc[q];
        }
#pragma unroll
        for (int q = 0; q < 16; q++) { acc[q] = 0.f; acl[q] = 0.f; }
#pragma unroll
        for (int k = 0; k < 4; k++) {                                          // tap 8 = (ky, kx) = (2, 2): input pixel (oy + 1, ox + 1)
            const int pix = 3 * wave + k, pc = pix < 25 ? pix : 0, oy = pc / 5, ox = pc - oy * 5;
            const bool mine = k < 3 || wave == 7;
            step(mine && pix < 25 && oy < 4 && ox < 4 ? (oy + 1) * 5 + ox + 1 : -1, pc);
        }
        fold();
        reduce_rows<8>(acc, red, wave, lane, 0, 32, [&](float v, int, int row32) {
            o[OFF_W3 + (size_t)((8 * 64 + mid * 32 + row32) * 64) + cot * 32 + r] = v;
        });
    } else {
        // wave w: tap (a, b2) = w & 3 of the class, pixels [13 * (w >> 2), ..): the two halves meet through LDS
        const int t4 = wave & 3, a2 = t4 >> 1, b2 = t4 & 1, half = wave >> 2;
        const int ky = ((py + 1) & 1) + 2 * a2, kx = ((px + 1) & 1) + 2 * b2;
#pragma unroll
        for (int k = 0; k < 13; k++) {
            const int pix = half * 13 + k, pc = pix < 25 ? pix : 0;
            const int oy = pc / 5, ox = pc - oy * 5, qy = oy + a2 - py, qx = ox + b2 - px;
            step(pix < 25 && qy >= 0 && qy < 5 && qx >= 0 && qx < 5 ? qy * 5 + qx : -1, pc);
        }
        fold();
        if (half) {
#pragma unroll
            for (int q = 0; q < 16; q++) red[(t4 * 16 + q) * 64 + lane] = acc[q];
        }
        __syncthreads();
        if (!half) {
#pragma unroll
            for (int q = 0; q < 16; q++)
                o[OFF_W2 + (size_t)(((ky * 4 + kx) * 32 + drow(q, lane)) * 64) + cot * 32 + r] = acc[q] + red[(t4 * 16 + q) * 64 + lane];
        }
    }
}

template <int NS>
__global__ __launch_bounds__(512) void conv_dwg_kernel(int n3, const float *__restrict__ h2, const float *__restrict__ dh3, const float *__restrict__ p1,
                                                       const float *__restrict__ dh2, float *__restrict__ slabs, size_t slab_stride, unsigned *__restrict__ ovf) {
    __shared__ uint4 pool[DwgLds<NS>::U4];
    if ((int)blockIdx.x < n3) conv_dwg_body<NS, 3>(blockIdx.x, h2, dh3, slabs, slab_stride, pool, ovf);
    else conv_dwg_body<NS, 2>(blockIdx.x - n3, p1, dh2, slabs, slab_stride, pool, ovf);
}

// Large batches: conv1's weight gradient reduces over B x 400 output pixels; with at most zmax = 64 slabs a wave would
// walk up to 7 chunks one after the other (94 us at B = 256).  It is cut into up to 4 x 64 sub-slabs instead (one chunk
// per wave again) and this kernel folds groups of 4 into the 64 slabs the Adam kernel sums, in a fixed order.
constexpr int CONV1_PARAMS = OFF_W2;       // W_conv1 + b_conv1 open a slab
__global__ void slab_fold_kernel(const float *__restrict__ sub, int nsub, int fold, float *__restrict__ slabs, size_t slab_stride) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
    if (idx >= CONV1_PARAMS) return;
    float v = 0.f;
    for (int q0 = 0; q0 < fold; q0 += 4) {               // four loads in flight at a time, added in slab order
        float x[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int z = s * fold + q0 + q;
            const bool ok = q0 + q < fold && z < nsub;
            x[q] = sub[(size_t)(ok ? z : 0) * CONV1_PARAMS + idx];
            x[q] = ok ? x[q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) v += x[q];
    }
    slabs[s * slab_stride + idx] = v;
}

// The conv gradient of float4 `q4` = the sum of its z <= 64 slabs in ONE canonical order that both consumers use (adam_fused_kernel of
// the fused step, slab_reduce_kernel of the gradient-exporting one), so the two forms stay bit-identical:
//     chunk c = (((0 + s[16 c]) + s[16 c + 1]) + ..) over its <= 16 slabs, in slab order;      G = ((C0 + C1) + C2) + C3   (absent chunks: + 0)
// A chunk is sixteen loads in flight at once from clamped addresses, masked by selects; the chunks are independent, so the Adam kernel
// gives each to its own lane (per-sample slabs: z = 32 / 64 is one round trip there, not two / four; thirty-two loads in flight on
// ONE lane -- 168 registers -- took that kernel from 7.3 to 12.0 us in situ, profiles/r04_notes.md).
constexpr int SLAB_CHUNK = 16;                // (four chunks: zmax = 64 slabs)
__device__ __forceinline__ float4 slab_chunk4(const float *__restrict__ slabs, size_t slab_stride, long long q4, int z, int c) {
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), t[SLAB_CHUNK];
    const int s0 = c * SLAB_CHUNK;
#pragma unroll
    for (int q = 0; q < SLAB_CHUNK; q++) t[q] = *reinterpret_cast<const float4 *>(slabs + (size_t)(s0 + q < z ? s0 + q : 0) * slab_stride + q4 * 4);
#pragma unroll
    for (int q = 0; q < SLAB_CHUNK; q++) {
        const bool ok = s0 + q < z;
        g.x += ok ? t[q].x : 0.f; g.y += ok ? t[q].y : 0.f; g.z += ok ? t[q].z : 0.f; g.w += ok ? t[q].w : 0.f;
    }
    return g;
}
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 slab_combine4(float4 c0, float4 c1, float4 c2, float4 c3) { return add4(add4(add4(c0, c1), c2), c3); }
// (one thread, chunk after chunk: the gradient-exporting path's slab_reduce_kernel)
__device__ __forceinline__ float4 slab_sum4(const float *__restrict__ slabs, size_t slab_stride, long long q4, int z) {
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 c0 = slab_chunk4(slabs, slab_stride, q4, z, 0);
    const float4 c1 = z > SLAB_CHUNK ? slab_chunk4(slabs, slab_stride, q4, z, 1) : zero;
    const float4 c2 = z > 2 * SLAB_CHUNK ? slab_chunk4(slabs, slab_stride, q4, z, 2) : zero;
    const float4 c3 = z > 3 * SLAB_CHUNK ? slab_chunk4(slabs, slab_stride, q4, z, 3) : zero;
    return slab_combine4(c0, c1, c2, c3);
}

// sum the reduction slabs of the conv weight + bias gradients into the flat gradient (fixed order)
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float *__restrict__ slabs, size_t slab_stride, int z1, int z2, int z3,
                                   float *__restrict__ grad) {
    const int q4 = blockIdx.x * blockDim.x + threadIdx.x, idx = q4 * 4;
    if (idx >= CONV_PARAMS) return;
    const int z = idx < OFF_W2 ? z1 : (idx < OFF_W3 ? z2 : z3);
    reinterpret_cast<float4 *>(grad)[q4] = slab_sum4(slabs, slab_stride, q4, z);
}
static_assert(OFF_W2 % 4 == 0 && OFF_W3 % 4 == 0 && CONV_PARAMS % 4 == 0, "slab regions are float4 aligned");

// TF ApplyAdam, fp32, float4 wide: THE Adam launch -- of the fused step (single GPU: the conv gradients are still spread over the
// reduction slabs and are summed here, in the canonical order above; W_fc1 has been updated by the AdamSpan riding in the conv backward
// launch and is skipped: tail0) and of fb_qnet_apply_adam (data parallel: a complete flat gradient, no slabs, tail0 = the start of W_fc1).
// adam4 per element either way, dealt out so that the update of W_conv2 / W_conv3 leaves their split planes behind (forward
// [k / 8][plane][co] and transposed [tap * 8 + co / 8][plane][ci], what wsplit_item builds) the way the update of W_conv1 always has
// (split_w1).  INVARIANT this establishes: the conv planes of a net are current after every library call that writes its parameters
// (Adam here; init / load / target sync re-split eagerly) -- so the kernels that read them in the launch they run in (the ring-fed
// train trunk conv23_t_kernel<ring>, the fused acting trunk) need no launch in front of them.  W_fc1's planes stay stale (wver): only
// the >= 256-state forward reads them, and the launch in front of its fc1 re-splits them on sight.
//   workgroups [0, 64)      W_conv2, one tile of 8 k-rows x 64 co each (128 float4): TWO lanes per float4, lane c sums the slab chunks c and
//                           c + 2 (the launch is a chain of dependent round trips -- P / m / v and the chunks all leave in the first one);
//                           update, park the new values in LDS, emit the 64 forward entries and the 8 x 8 transposed entries (8 weights
//                           each, three planes)
//   workgroups [64, 136)    W_conv3 likewise (72 tiles)
//   then n_rest             everything else from tail0 on: W_conv1 + b_conv1 (W_conv1's planes via split_w1), b_conv2, b_conv3, [W_fc1,]
//                           b_fc1 and the head; `lanes` (4 with slabs: one chunk per lane; 1 without) lanes per float4
constexpr int ADAMF_T2 = 64, ADAMF_T3 = 72;
struct AdamFused {
    float *p, *m, *v; const float *g; long long n; AdamDev *ad;
    const float *slabs; size_t slab_stride; int z1, z2, z3;
    uint16_t *w1s; uint4 *wsp; int FC;
    int tail0;                       // first float4 behind W_fc1
    int n_rest;                      // workgroups of the third role
    int lanes;                       // lanes per float4 in the third role: 4 (slab mode: a chunk each) or 1
    // split schedule (or NULL): the launch does not retire before the other stream's env step has (whatever the caller puts on this stream
    // next may read the env step's outputs).  (That stream's fc1 launch -- which reads the conv planes and biases this launch rewrites,
    // records the version word and copies the head's parameters -- has retired: the conv backward launch's gate workgroup waited for it.)
    FbSplitFlags *split; unsigned long long split_val;
};
__device__ __forceinline__ float4 shfl4(float4 v, int src) { return make_float4(__shfl(v.x, src), __shfl(v.y, src), __shfl(v.z, src), __shfl(v.w, src)); }
__global__ __launch_bounds__(256) void adam_fused_kernel(AdamFused a) {
    __shared__ float tile[8][68];
    const int bid = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float alpha = a.ad->alpha, omb1 = 1.f - a.ad->b1, omb2 = 1.f - a.ad->b2, eps = a.ad->eps;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (bid < ADAMF_T2 + ADAMF_T3) {
        const bool l3 = bid >= ADAMF_T2;
        const int k0 = 8 * (l3 ? bid - ADAMF_T2 : bid), woff = l3 ? OFF_W3 : OFF_W2, CI = l3 ? 64 : 32, z = l3 ? a.z3 : a.z2;
        const int f = tid >> 1, c = tid & 1, kr = f >> 4, c4 = f & 15;
        const long long q = (woff + (k0 + kr) * 64 + 4 * c4) >> 2;
        float4 P = reinterpret_cast<float4 *>(a.p)[q], Mv = reinterpret_cast<float4 *>(a.m)[q], V = reinterpret_cast<float4 *>(a.v)[q];
        float4 Gv;
        if (z > 0) {
            // lane c: chunks c and c + 2; the pair exchanges them and both add in the canonical order
            const float4 ca = slab_chunk4(a.slabs, a.slab_stride, q, z, c);
            const float4 cb = z > 2 * SLAB_CHUNK ? slab_chunk4(a.slabs, a.slab_stride, q, z, c + 2) : zero;
            const float4 oa = shfl4(ca, lane ^ 1), ob = shfl4(cb, lane ^ 1);
            Gv = c == 0 ? slab_combine4(ca, oa, cb, ob) : slab_combine4(oa, ca, ob, cb);
        } else Gv = reinterpret_cast<const float4 *>(a.g)[q];
        adam4(P, Mv, V, Gv, alpha, omb1, omb2, eps);
        if (c == 0) {
            reinterpret_cast<float4 *>(a.p)[q] = P; reinterpret_cast<float4 *>(a.m)[q] = Mv; reinterpret_cast<float4 *>(a.v)[q] = V;
            *reinterpret_cast<float4 *>(&tile[kr][4 * c4]) = P;
        }
        __syncthreads();
        if (tid < 64) {                                                  // forward planes: entry (k8, col) = weights W[8 k8 .. 8 k8 + 7][col]
            const int col = tid;
            uint4 *o = a.wsp + (l3 ? WSP_W3 : WSP_W2) + (size_t)(k0 / 8) * 3 * 64 + col;
            wsplit_store(o, 64, tile[0][col], tile[1][col], tile[2][col], tile[3][col], tile[4][col], tile[5][col], tile[6][col], tile[7][col]);
        } else if (tid < 128) {                                          // transposed planes: entry (tap * 8 + co / 8, ci) = 8 consecutive co of row (tap, ci)
            const int r = (tid - 64) >> 3, co8 = tid & 7, tap = k0 / CI, ci = k0 - tap * CI + r;
            uint4 *o = a.wsp + (l3 ? wsp_w3t(a.FC) : wsp_w2t(a.FC)) + (size_t)(tap * 8 + co8) * 3 * CI + ci;
            const float *t = &tile[r][8 * co8];
            wsplit_store(o, CI, t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7]);
        }
        return;
    }
    // the rest, as consecutive float4 ranges of the flat vector: [0, OFF_W2) [OFF_B2, OFF_W3) [OFF_B3, OFF_WF1) [tail0 * 4, n)
    const int n0 = OFF_W2 / 4, n1 = (OFF_W3 - OFF_B2) / 4, n2 = (OFF_WF1 - OFF_B3) / 4;
    const long long n4 = a.n >> 2, nq = n0 + n1 + n2 + (n4 - a.tail0);
    const int L = a.lanes, per = 256 / L, c = tid & (L - 1);              // L lanes per float4 (a power of two); lane c: slab chunk c
    for (long long base = (long long)(bid - ADAMF_T2 - ADAMF_T3) * per; base < nq; base += (long long)a.n_rest * per) {
        const long long qq = base + tid / L;
        const bool live = qq < nq;
        const long long qc = live ? qq : 0;
        long long q; int z;
        if (qc < n0) { q = qc; z = a.z1; }
        else if (qc < n0 + n1) { q = OFF_B2 / 4 + (qc - n0); z = a.z2; }
        else if (qc < n0 + n1 + n2) { q = OFF_B3 / 4 + (qc - n0 - n1); z = a.z3; }
        else { q = a.tail0 + (qc - n0 - n1 - n2); z = 0; }
        float4 P = reinterpret_cast<float4 *>(a.p)[q], Mv = reinterpret_cast<float4 *>(a.m)[q], V = reinterpret_cast<float4 *>(a.v)[q];
        float4 Gv;
        if (L == 4) {
            // (z is uniform over the four lanes of an item; the shuffles run for every lane of the wave)
            const float4 mine = z > c * SLAB_CHUNK ? slab_chunk4(a.slabs, a.slab_stride, q, z, c) : zero;
            const int l0 = lane & ~3;
            const float4 c0 = shfl4(mine, l0), c1 = shfl4(mine, l0 + 1), c2 = shfl4(mine, l0 + 2), c3 = shfl4(mine, l0 + 3);
            Gv = z > 0 ? slab_combine4(c0, c1, c2, c3) : reinterpret_cast<const float4 *>(a.g)[q];
        } else Gv = z > 0 ? slab_sum4(a.slabs, a.slab_stride, q, z) : reinterpret_cast<const float4 *>(a.g)[q];
        adam4(P, Mv, V, Gv, alpha, omb1, omb2, eps);
        if (live && c == 0) {
            reinterpret_cast<float4 *>(a.p)[q] = P; reinterpret_cast<float4 *>(a.m)[q] = Mv; reinterpret_cast<float4 *>(a.v)[q] = V;
            if (q * 4 < OFF_B1) {                                        // W_conv1 changed: refresh its two fp16 planes
                const int idx = (int)q * 4;
                split_w1(P.x, idx, a.w1s); split_w1(P.y, idx + 1, a.w1s); split_w1(P.z, idx + 2, a.w1s); split_w1(P.w, idx + 3, a.w1s);
            }
        }
    }
    // the update consumes the pending tick and makes a new parameter version, of which the conv planes are current (nothing in this
    // launch reads these words)
    if (bid == ADAMF_T2 + ADAMF_T3 && tid == 0) { a.ad->applies = a.ad->ticks; a.ad->pver[0] += 1; a.ad->wverc[0] = a.ad->pver[0]; }
    if (bid == ADAMF_T2 + ADAMF_T3 && tid < (int)(a.n & 3)) {
        const long long q = (n4 << 2) + tid;
        float mm = a.m[q], vv = a.v[q];
        mm += (a.g[q] - mm) * omb1; vv += (a.g[q] * a.g[q] - vv) * omb2;
        a.p[q] -= (mm * alpha) / (sqrtf(vv) + eps);
        a.m[q] = mm; a.v[q] = vv;
    }
    if (a.split && bid == ADAMF_T2 + ADAMF_T3 && tid == 0) fb_flag_wait(&a.split->env_done, a.split_val, &a.split->timeouts[4]);
}

// tf.truncated_normal(stddev=0.01) weights, 0.01 biases (BrainDQN.py:123-152)
__global__ void init_params_kernel(float *__restrict__ p, long long n, NetOff off, int FC, int A, int dueling,
                                   uint32_t seed_lo, uint32_t seed_hi) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool bias = (i >= OFF_B1 && i < OFF_W2) || (i >= OFF_B2 && i < OFF_W3) || (i >= OFF_B3 && i < OFF_WF1) ||
                (i >= off.bf1 && i < off.bf1 + FC) || (i >= off.bq && i < off.bq + A) || (dueling && i == off.bv);
    if (bias) { p[i] = 0.01f; return; }
    for (uint32_t ctr = 0;; ctr++) {
        const fb_u4 r = fb_philox(seed_lo, seed_hi, (uint32_t)i, ctr, FB_STREAM_INIT, 0u);
        const float u1 = ((r.x >> 8) + 1) * (1.0f / 16777216.0f), u2 = (r.y >> 8) * (1.0f / 16777216.0f);
        const float z = sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
        if (fabsf(z) <= 2.f) { p[i] = 0.01f * z; return; }
    }
}

}  // namespace

#ifndef FB_ADAM_GRID
#define FB_ADAM_GRID 1024
#endif
constexpr int ADAM_GRID = FB_ADAM_GRID;

// ================================================================== host side
#include <vector>
struct fb_qnet {
    std::vector<void *> allocs;      // every device buffer qnet_create allocated, as its alloc() recorded it: what fb_qnet_destroy frees
    int arch, FC, A, max_batch;
    long long n;
    NetOff off;
    float *params[2], *adam_m, *adam_v, *grad, *slabs;
    float *slabs1;                   // conv1 sub-slabs of large batches (slab_fold_kernel), NULL when max_batch never needs them
    uint16_t *w1s[2];                // W_conv1 as two fp16 planes (h, l), [2][8192]
    uint4 *wsp[2];                   // planes (fp16 h, fp16 l, bf16) of W_conv2, W_conv3, W_fc1 and of the transposed conv weights
    uint16_t *zeros;                 // 256 B of zeros (padding source of the plane kernels)
    uint16_t *a1s, *a3s;             // activation planes of that path: conv1 out [2][S*3200], conv3 out [2][S*1600] fp16 (one bf16 plane in bf16 mode)
    int nsplit;                      // 3 = fp32-equivalent (default), 1 = bf16 inference
    int nsplit_train;                // the same for training (fb_qnet_set_train_dtype): 1 = bf16 operands, fp32 accumulation + master weights
    bool adam_ticked;                // host-side hint only (eager calls): the last train step left a tick pending for fb_qnet_apply_adam;
                                     // the truth is AdamDev::ticks / applies on the device
    AdamDev *adam;
    // workspace for 3 * max_batch samples
    float *p1, *h2, *h3, *hf, *q;
    float *qpart;                    // small-batch training: per 16-unit tile shares of the head, [S][FC/16][A + 1]
    unsigned long long *ring_fo;     // ring-fed training: the four frame offsets of every sample's state s, [max_batch][4]
    hipEvent_t grad_ev;              // fb_qnet_set_grad_event: recorded behind the fc1 backward launch of a gradient-exporting step, or NULL
    hipEvent_t grad_ev_recorded;     // the event the last gradient-exporting step did record (fb_qnet_take_grad_event_recorded)
    uint8_t *amax;
    float *dhf, *dh3, *dh2, *dp1;
    float *gmax;                     // large batches: the loss kernel's per-workgroup maxima of |dhf| (gradient pre-scale of fc1_bwd_big_kernel), [FC / 16]
    int zmax;
    // the fused acting forward's OWN fc1 partial sums and its copy of the parameters the head reads (b_fc1 on: [n - off.bf1], taken by the
    // fc1 launch): a train step running beside it on another stream (fb_vec_step's split schedule) shares none of its buffers and may
    // start its Adam launch as soon as that fc1 launch is through
    float *hf_act, *hp_act;
    FbSplitCtx *split;               // fb_qnet_split_ctx
    C51Sup sup;                      // C51 nets: the support (sup.N = 0: a scalar head); QR nets: sup.N = n_quantiles, the rest 0
    float kappa;                     // QR nets: the quantile Huber loss's threshold
    MdPar md;                        // scalar nets: Munchausen-DQN's (tau, alpha, l0) (fb_qnet_set_munchausen)
    float huber;                     // scalar nets: the Huber loss's delta; 0 = the squared loss (fb_qnet_set_huber)
    float *c51_dl, *c51_xs, *c51_lt; // C51 training: logit gradients [max_batch][64], fc1 activations of s [max_batch][FC], loss terms [max_batch]
    // what the C51 head / loss / eval kernels read: hoff (the C51 layout; = off but for a dueling C51 net) from head_base(params[w]).
    // A dueling C51 net (FB_ARCH_C51_DUELING): heff[w] = [b_fc1 | W_eff | b_eff], the folded head of params[w] (c51d_fold_kernel)
    NetOff hoff;
    float *heff[2];
    // a noisy C51 net (fb_qnet_create_c51_noisy): mst[w] = [mu | sigma] (ntot floats: what Adam updates, load / store / sync move);
    // params[w] is then the EFFECTIVE vector (n floats, mu + sigma * noise, noisy_mat_kernel) every forward / backward kernel reads.
    // nz[w]: the net's current f(eps) sample (nnet.nz floats; zeros = mean mode).  Other nets: ntot = n, mst / nz NULL
    bool noisy;
    long long ntot;
    NoisyNet nnet;
    float *mst[2], *nz[2];
    // per-env acting noise (fb_qnet_act_nib_env_noise; noisy nets only): the mode fb_vec_step acts in (FB_ACT_NOISE_*); nz_zero: a zero
    // noise vector (mu materialised for the call); wsig: sigma_W_fc1 as W_fc1's planes (wsig + WSP_WF1), built at the Adam count *sig_seen;
    // a3n: the scaled activations' planes (a3s's shape); ht: sigma's fc1 partials (hf_act's shape)
    int act_noise;
    float *nz_zero, *ht;
    uint4 *wsig;
    uint16_t *a3n;
    int *sig_seen;
    bool split_adam_pending;         // a split step exported its gradient: the fb_qnet_apply_adam that completes it takes over the Adam launch's waits
    // global-norm gradient clipping (fb_qnet_set_max_grad_norm): G, 0 = off; clip_part: grad_sumsq_kernel's float64 partials, one per
    // workgroup; clip_out: (norm, c) of the last fb_qnet_clip_grad
    float max_grad_norm;
    double *clip_part;
    float *clip_out;
    // an actor-critic net (FB_ARCH_AC, fb_qnet_create_ac; kernels: fb_ac.hip): (c_v, c_e) of fb_qnet_set_ac; ac_dl: the loss kernel's
    // per-sample row [max_batch][16]; ac_xs: fc1 activations of s [max_batch][FC]; ac_r / ac_t: the rows the ring-fed trunk fills beside the actions
    float ac_cv, ac_ce;
    float ppo_eps, ppo_vclip;        // PPO's clip ranges (fb_qnet_set_ppo): the ratio's epsilon, the value clip (0 = off)
    float *ac_dl, *ac_xs, *ac_r;
    uint8_t *ac_t;
    // a SAC net (FB_ARCH_SAC, fb_qnet_create_sac; kernels: fb_sac.hip): the two Q heads behind the plain layout's W_pi b_pi; the target
    // entropy and the temperature's learning rate (fb_qnet_set_sac); sac_w: [dev] (log alpha, m, v, beta1 power, beta2 power).  The loss
    // kernel's per-sample row and the activations of s live in ac_dl / ac_xs
    SacOff sac_off;
    float sac_hbar, sac_alr;
    float *sac_w;
    // an IQN net (FB_ARCH_IQN, fb_qnet_create_iqn; kernels: fb_iqn.hip): the embedding W_e b_e behind the plain layout; N, N', K and the risk
    // setting eta (kappa: the field above).  heff[w] = [b_fc1 | phibar * W_q | b_q], the fold of params[w] every forward-only path reads as a
    // plain net's head (iqn_fold_kernel; refolded wherever a dueling C51 net's head is).  Training: the loss kernel's per-sample row in ac_dl
    // ([.][4]), the W_q-gradient rows in ac_xs, the embedding's pre-activation gradients [Bt N][FC] and the cosine rows [Bt N][64]
    IqnOff iqn_off;
    int iqn_n, iqn_np, iqn_k;
    float iqn_eta;
    float *iqn_dpre, *iqn_ctab;
    // a dueling IQN net (FB_ARCH_IQN_DUELING, fb_qnet_create_iqn_dueling): off is the DUELING layout (W_v b_v W_a b_a), then W_e b_e; its fold
    // heff[w] = [b_fc1 | phibar * We | be] keeps the PLAIN layout, whose offsets are hoff: what reads head_base() as a plain net takes hoff
    // Munchausen IQN (fb_qnet_set_iqn_munchausen): on / off and (temp, alpha, l0); read by the IQN train plans alone
    int iqn_mu;
    MdPar iqn_md;
    // an actor-critic net: [dev] f32[6], the running sum of the last fb_ppo_epoch's chunk loss numbers (fb_ppo_epoch_sum).  Last, so that
    // every field above keeps the place it had
    float *ppo_sum;
    // a noisy IQN net (fb_qnet_create_iqn_noisy): fc1 and the head layers are noisy as a noisy C51 net's (mst / nz / nnet above;
    // iqn_off.we = noisy_end: W_e b_e have no sigma).  iqn_pbar[w]: phibar[FC] of net w's acting grid, left by the noisy fold launch for the per-env head
    // noisy_end: where the noisy range [OFF_WF1, noisy_end) of any noisy net ends.  (Behind every field of before)
    float *iqn_pbar[2];
    int noisy_end;
};

static NetOff make_off(int FC, int A, int dueling) {      // A: the head's columns (C51: actions x atoms)
    NetOff o;
    o.bf1 = OFF_WF1 + 1600 * FC;
    int p = o.bf1 + FC;
    if (dueling) { o.wv = p; o.bv = p + FC; p = o.bv + 1; } else { o.wv = 0; o.bv = 0; }
    o.wq = p; o.bq = p + FC * A; o.n = o.bq + A;
    return o;
}

// a dueling C51 net: the trunk, W_fc1 b_fc1, then W_v[FC, N] b_v[N] W_a[FC, A N] b_a[A N] (wq / bq: the advantage head)
static NetOff make_off_c51d(int FC, int A, int N) {
    NetOff o;
    o.bf1 = OFF_WF1 + 1600 * FC;
    o.wv = o.bf1 + FC; o.bv = o.wv + FC * N;
    o.wq = o.bv + N; o.bq = o.wq + FC * A * N; o.n = o.bq + A * N;
    return o;
}
// a folded head: a dueling C51 or dueling QR net (the same layout and fold)
static bool is_c51d(const fb_qnet *h) { return h->arch == FB_ARCH_C51_DUELING || h->arch == FB_ARCH_QR_DUELING; }
static bool is_qr(const fb_qnet *h) { return h->arch == FB_ARCH_QR || h->arch == FB_ARCH_QR_DUELING; }
// an actor-critic net: the dueling layout read raw (W_v b_v: V; W_pi b_pi at wq / bq: the logits, which the plain head reads as "Q")
static bool is_ac(const fb_qnet *h) { return h->arch == FB_ARCH_AC; }
// a SAC net: the plain layout (W_pi b_pi at wq / bq: the logits, which the plain head reads as "Q"), then W_q1 b_q1 W_q2 b_q2
static bool is_sac(const fb_qnet *h) { return h->arch == FB_ARCH_SAC; }
// an IQN net: the plain layout (W_q b_q at wq / bq), then W_e b_e; forward-only paths read the plain head over its fold, heff[w]
static bool is_iqn(const fb_qnet *h) { return h->arch == FB_ARCH_IQN || h->arch == FB_ARCH_IQN_DUELING; }
// a dueling IQN net: the dueling layout (W_v b_v, W_a b_a at wq / bq), then W_e b_e; its fold is a plain net's, read with hoff
static bool is_iqnd(const fb_qnet *h) { return h->arch == FB_ARCH_IQN_DUELING; }
// the parameters the C51 kernels read, with h->hoff, for the net whose parameters are `params` (a virtual base for a dueling C51 net:
// hoff.bf1 lands on heff[w][0], as the acting forward's hp_act copy is read)
static const float *head_base(const fb_qnet *h, const float *params) {
    if (!is_c51d(h) && !is_iqn(h)) return params;
    return h->heff[params == h->params[1] ? 1 : 0] - h->off.bf1;
}
// refold a dueling C51 net's head after its parameters changed (no-op for other nets)
static void c51d_fold(fb_qnet *h, int which, hipStream_t st) {
    if (is_iqn(h)) {                             // (an IQN net: phibar over the acting grid and its fold block, fb_iqn.hip)
        const IqnFoldArgs F{h->params[which], h->heff[which], h->FC, h->A, h->iqn_k, h->off, h->iqn_off, h->iqn_eta, is_iqnd(h) ? 1 : 0};
        if (h->noisy) fb_iqn_launch_fold_noisy(st, IqnFoldNzArgs{F, h->iqn_pbar[which]});      // (... and phibar itself, for the per-env head)
        else fb_iqn_launch_fold(st, F);
        return;
    }
    if (!is_c51d(h)) return;
    const C51dFoldArgs F{h->params[which], h->heff[which], h->off, h->FC, h->A, h->sup.N};
    const int tot = h->FC + (h->FC + 1) * h->A * h->sup.N;
    hipLaunchKernelGGL(c51d_fold_kernel, dim3((tot + 255) / 256), dim3(256), 0, st, F);
}

// the vector Adam updates and load / store / sync move: [mu | sigma] of a noisy net, the parameters themselves otherwise
static float *master(const fb_qnet *h, int which) { return h->noisy ? h->mst[which] : h->params[which]; }
// a noisy net: rebuild params[which] from its master vector and noise, from q0 on (0 after a change of mu's trunk); bump: a new parameter
// version (noise only: the conv planes stay current).  No-op for other nets
static void noisy_materialise(fb_qnet *h, int which, int q0, bool bump, hipStream_t st) {
    if (!h->noisy) return;
    const NoisyMat a{h->mst[which], h->params[which], h->nz[which], h->nnet, q0, which, bump ? h->adam : nullptr, h->noisy_end};
    hipLaunchKernelGGL(noisy_mat_kernel, dim3((unsigned)((h->n - q0 + 255) / 256)), dim3(256), 0, st, a);
}
// a noisy net whose online sigma the host replaced (init / load): the per-env acting path's sigma_W_fc1 planes are stale
static void env_noise_invalidate(fb_qnet *h, int which, hipStream_t st) {
    if (h->noisy && which == 0) (void)hipMemsetD32Async((hipDeviceptr_t)h->sig_seen, -1, 1, st);
}
// a noisy net: sigma's gradient into g[n ..) from the effective parameters' gradient in g[OFF_WF1, n)
static void noisy_sgrad(fb_qnet *h, float *g, hipStream_t st) {
    if (!h->noisy) return;
    hipLaunchKernelGGL(noisy_sgrad_kernel, dim3((unsigned)((h->noisy_end - OFF_WF1 + 255) / 256)), dim3(256), 0, st, g, (const float *)h->nz[0], h->nnet, h->noisy_end);
}

// What a net is made from.  Every fb_qnet_create* checks its arguments, fills one of these and hands it to qnet_create; nothing reaches the
// handle by another way.  The fields a family does not have stay zero
struct NetSpec {
    int arch, fc_width, n_actions, max_batch;
    C51Sup sup;                      // C51 nets: the support
    int n_quantiles;                 // QR nets: N
    float kappa;                     // QR and IQN nets: the quantile Huber loss's threshold
    bool noisy; float sigma0;        // noisy C51 / IQN nets (fb_qnet_create_c51_noisy / _iqn_noisy): finite sigma0 >= 0
    int n_tau, n_tau_next, n_tau_act;      // IQN nets: N, N', K
};
static NetSpec net_spec(int arch, int fc_width, int n_actions, int max_batch) {
    NetSpec s{};
    s.arch = arch; s.fc_width = fc_width; s.n_actions = n_actions; s.max_batch = max_batch;
    return s;
}
static int qnet_create(const NetSpec &s, fb_qnet_t *out);

// The checks every creator makes, `fn` naming it in the message.  They stand at three places of a creator's order (the first failing check
// decides the text): `out` in front of everything, fc_width and n_actions (min_actions: the family's lower bound, 1 or 2) in front of the
// family's own checks, max_batch behind them
enum { CREATE_OUT = 1, CREATE_SHAPE = 2, CREATE_BATCH = 4, CREATE_ALL = 7 };
static int check_create(const char *fn, const NetSpec &s, int min_actions, const fb_qnet_t *out, int which = CREATE_ALL) {
    if (which & CREATE_OUT) FB_REQUIRE(out, "%s: out is NULL", fn);
    if (which & CREATE_SHAPE) {
        FB_REQUIRE(s.fc_width >= 128 && s.fc_width <= 4096 && s.fc_width % 128 == 0, "%s: fc_width must be a multiple of 128", fn);
        FB_REQUIRE(s.n_actions >= min_actions && s.n_actions <= MAXA, "%s: n_actions must be in %d..%d", fn, min_actions, MAXA);
    }
    if (which & CREATE_BATCH) FB_REQUIRE(s.max_batch >= 1 && s.max_batch <= (1 << 20), "%s: max_batch out of range", fn);
    return FB_OK;
}

extern "C" int fb_qnet_create(int arch, int fc_width, int n_actions, int max_batch, fb_qnet_t *out) {
    const NetSpec s = net_spec(arch, fc_width, n_actions, max_batch);
    if (const int rc = check_create("fb_qnet_create", s, 1, out, CREATE_OUT)) return rc;
    FB_REQUIRE(arch != FB_ARCH_C51, "fb_qnet_create: a C51 net is made by fb_qnet_create_c51 (it needs the support)");
    FB_REQUIRE(arch != FB_ARCH_C51_DUELING, "fb_qnet_create: a dueling C51 net is made by fb_qnet_create_c51_dueling (it needs the support)");
    FB_REQUIRE(arch != FB_ARCH_QR && arch != FB_ARCH_QR_DUELING, "fb_qnet_create: a QR net is made by fb_qnet_create_qr (it needs N and kappa)");
    FB_REQUIRE(arch != FB_ARCH_AC, "fb_qnet_create: an actor-critic net is made by fb_qnet_create_ac");
    FB_REQUIRE(arch != FB_ARCH_SAC, "fb_qnet_create: a SAC net is made by fb_qnet_create_sac");
    FB_REQUIRE(arch != FB_ARCH_IQN, "fb_qnet_create: an IQN net is made by fb_qnet_create_iqn (it needs N, N', K and kappa)");
    FB_REQUIRE(arch == FB_ARCH_PLAIN || arch == FB_ARCH_DUELING, "fb_qnet_create: arch must be 0 or 1");
    if (const int rc = check_create("fb_qnet_create", s, 1, out, CREATE_SHAPE | CREATE_BATCH)) return rc;
    return qnet_create(s, out);
}

// the checks of fb_qnet_create_c51 / _c51_dueling / _c51_noisy, before any allocation (`fn` names the caller in the message)
static int c51_create(const char *fn, int arch, int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, fb_qnet_t *out,
                      bool noisy, float sigma0) {
    NetSpec s = net_spec(arch, fc_width, n_actions, max_batch);
    if (const int rc = check_create(fn, s, 1, out, CREATE_OUT | CREATE_SHAPE)) return rc;
    FB_REQUIRE(n_atoms >= 2 && n_atoms <= FB_C51_MAX_ATOMS, "%s: n_atoms=%d outside 2..%d", fn, n_atoms, FB_C51_MAX_ATOMS);
    FB_REQUIRE(n_actions * n_atoms <= 128, "%s: n_actions * n_atoms = %d exceeds 128", fn, n_actions * n_atoms);
    FB_REQUIRE(isfinite(v_min) && isfinite(v_max) && v_min < v_max, "%s: the support needs finite v_min < v_max (got %g, %g)",
               fn, (double)v_min, (double)v_max);
    if (const int rc = check_create(fn, s, 1, out, CREATE_BATCH)) return rc;
    const float dz = (v_max - v_min) / (float)(n_atoms - 1);
    FB_REQUIRE(isfinite(dz) && dz > 0.f, "%s: the atom spacing (v_max - v_min) / (n_atoms - 1) is not a positive finite float", fn);
    s.sup = C51Sup{n_atoms, v_min, v_max, dz}; s.noisy = noisy; s.sigma0 = sigma0;
    return qnet_create(s, out);
}

extern "C" int fb_qnet_create_c51(int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, fb_qnet_t *out) {
    return c51_create("fb_qnet_create_c51", FB_ARCH_C51, fc_width, n_actions, n_atoms, v_min, v_max, max_batch, out, false, 0.f);
}

extern "C" int fb_qnet_create_c51_dueling(int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, fb_qnet_t *out) {
    return c51_create("fb_qnet_create_c51_dueling", FB_ARCH_C51_DUELING, fc_width, n_actions, n_atoms, v_min, v_max, max_batch, out, false, 0.f);
}

extern "C" int fb_qnet_create_c51_noisy(int arch, int fc_width, int n_actions, int n_atoms, float v_min, float v_max, float sigma0, int max_batch,
                                        fb_qnet_t *out) {
    FB_REQUIRE(out, "fb_qnet_create_c51_noisy: out is NULL");
    FB_REQUIRE(arch == FB_ARCH_C51 || arch == FB_ARCH_C51_DUELING, "fb_qnet_create_c51_noisy: arch must be FB_ARCH_C51 (2) or FB_ARCH_C51_DUELING (3), "
               "got %d (noisy layers are offered on the C51 heads only)", arch);
    FB_REQUIRE(isfinite(sigma0) && sigma0 >= 0.f, "fb_qnet_create_c51_noisy: sigma0 must be finite and >= 0 (got %g)", (double)sigma0);
    return c51_create("fb_qnet_create_c51_noisy", arch, fc_width, n_actions, n_atoms, v_min, v_max, max_batch, out, true, sigma0);
}

extern "C" int fb_qnet_create_qr(int arch, int fc_width, int n_actions, int n_quantiles, float kappa, int max_batch, fb_qnet_t *out) {
    const char *fn = "fb_qnet_create_qr";
    NetSpec s = net_spec(arch, fc_width, n_actions, max_batch);
    if (const int rc = check_create(fn, s, 1, out, CREATE_OUT)) return rc;
    FB_REQUIRE(arch == FB_ARCH_QR || arch == FB_ARCH_QR_DUELING, "%s: arch must be FB_ARCH_QR (4) or FB_ARCH_QR_DUELING (5), got %d", fn, arch);
    if (const int rc = check_create(fn, s, 1, out, CREATE_SHAPE)) return rc;
    FB_REQUIRE(n_quantiles >= 2 && n_quantiles <= FB_C51_MAX_ATOMS, "%s: n_quantiles=%d outside 2..%d", fn, n_quantiles, FB_C51_MAX_ATOMS);
    FB_REQUIRE(n_actions * n_quantiles <= 128, "%s: n_actions * n_quantiles = %d exceeds 128", fn, n_actions * n_quantiles);
    FB_REQUIRE(isfinite(kappa) && kappa > 0.f, "%s: kappa must be finite and > 0 (got %g)", fn, (double)kappa);
    if (const int rc = check_create(fn, s, 1, out, CREATE_BATCH)) return rc;
    s.n_quantiles = n_quantiles; s.kappa = kappa;
    return qnet_create(s, out);
}

extern "C" int fb_qnet_create_ac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out) {
    const NetSpec s = net_spec(FB_ARCH_AC, fc_width, n_actions, max_batch);
    if (const int rc = check_create("fb_qnet_create_ac", s, 1, out)) return rc;
    return qnet_create(s, out);
}

extern "C" int fb_qnet_create_sac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out) {
    const NetSpec s = net_spec(FB_ARCH_SAC, fc_width, n_actions, max_batch);
    if (const int rc = check_create("fb_qnet_create_sac", s, 2, out)) return rc;
    return qnet_create(s, out);
}

// the checks of fb_qnet_create_iqn / _iqn_dueling, before any allocation (`fn` names the caller in the message)
static int iqn_create(const char *fn, int arch, int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch,
                      fb_qnet_t *out, bool noisy = false, float sigma0 = 0.f) {
    NetSpec s = net_spec(arch, fc_width, n_actions, max_batch);
    if (const int rc = check_create(fn, s, 2, out, CREATE_OUT | CREATE_SHAPE)) return rc;
    s.noisy = noisy; s.sigma0 = sigma0;
    FB_REQUIRE(n_tau >= 1 && n_tau <= 64, "%s: n_tau=%d outside 1..64", fn, n_tau);
    FB_REQUIRE(n_tau_next >= 1 && n_tau_next <= 64, "%s: n_tau_next=%d outside 1..64", fn, n_tau_next);
    FB_REQUIRE(n_tau_act >= 1 && n_tau_act <= 64, "%s: n_tau_act=%d outside 1..64", fn, n_tau_act);
    FB_REQUIRE(isfinite(kappa) && kappa > 0.f, "%s: kappa must be finite and > 0 (got %g)", fn, (double)kappa);
    if (const int rc = check_create(fn, s, 2, out, CREATE_BATCH)) return rc;
    s.n_tau = n_tau; s.n_tau_next = n_tau_next; s.n_tau_act = n_tau_act; s.kappa = kappa;
    return qnet_create(s, out);
}

extern "C" int fb_qnet_create_iqn(int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch, fb_qnet_t *out) {
    return iqn_create("fb_qnet_create_iqn", FB_ARCH_IQN, fc_width, n_actions, n_tau, n_tau_next, n_tau_act, kappa, max_batch, out);
}

extern "C" int fb_qnet_create_iqn_dueling(int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch,
                                          fb_qnet_t *out) {
    return iqn_create("fb_qnet_create_iqn_dueling", FB_ARCH_IQN_DUELING, fc_width, n_actions, n_tau, n_tau_next, n_tau_act, kappa, max_batch, out);
}

// a noisy IQN net (include/fbdqn.h): fb_qnet_create_iqn's checks, then sigma0's, before any allocation
extern "C" int fb_qnet_create_iqn_noisy(int dueling, int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, float sigma0,
                                        int max_batch, fb_qnet_t *out) {
    const char *fn = "fb_qnet_create_iqn_noisy";
    FB_REQUIRE(out, "%s: out is NULL", fn);
    FB_REQUIRE(dueling == 0 || dueling == 1, "%s: dueling must be 0 or 1 (got %d)", fn, dueling);
    FB_REQUIRE(isfinite(sigma0) && sigma0 >= 0.f, "%s: sigma0 must be finite and >= 0 (got %g)", fn, (double)sigma0);
    return iqn_create(fn, dueling ? FB_ARCH_IQN_DUELING : FB_ARCH_IQN, fc_width, n_actions, n_tau, n_tau_next, n_tau_act, kappa, max_batch, out, true, sigma0);
}

static int sac_write_words(fb_qnet *h, float alpha);

// the noise layers of a noisy net: fc1 (1600 -> FC), then the head's (C51: FC -> A N; dueling C51: FC -> N, FC -> A N; IQN: FC -> A; dueling
// IQN: FC -> 1, FC -> A)
static NoisyNet make_noisy(const NetOff &o, int arch, int FC, int A, int N, float sigma0) {
    NoisyNet nn;
    memset(&nn, 0, sizeof(nn));
    auto add = [&](int w, int fin, int fout) {
        NoisyLayer &L = nn.l[nn.nl++];
        L.w = w; L.fin = fin; L.fout = fout; L.ein = nn.nz; L.eout = nn.nz + fin; nn.nz += fin + fout;
        L.sig = (float)((double)sigma0 / sqrt((double)fin));
    };
    add(OFF_WF1, 1600, FC);
    if (arch == FB_ARCH_C51_DUELING) add(o.wv, FC, N);
    if (arch == FB_ARCH_IQN_DUELING) add(o.wv, FC, 1);
    add(o.wq, FC, N ? A * N : A);
    nn.n = o.n;
    return nn;
}

static int qnet_create(const NetSpec &s, fb_qnet_t *out) {
    const int arch = s.arch, fc_width = s.fc_width, n_actions = s.n_actions, max_batch = s.max_batch;
    const C51Sup sup = s.n_quantiles ? C51Sup{s.n_quantiles, 0.f, 0.f, 0.f} : s.sup;      // (fb_qnet::sup: a QR net keeps N there)
    fb_qnet *h = new fb_qnet();                  // (value-initialised: every field zero)
    h->md = MdPar{0.03f, 0.9f, -1.f};            // Munchausen-DQN, the paper's values (read by FB_ALGO_MDQN / _PER on a scalar net alone)
    h->ac_cv = 0.5f; h->ac_ce = 0.01f;           // A2C's value and entropy coefficients (read on an actor-critic net alone)
    h->ppo_eps = 0.2f; h->ppo_vclip = 0.f;       // PPO's clip ranges (read by the PPO train steps of an actor-critic net alone)
    h->arch = arch; h->FC = fc_width; h->A = n_actions; h->max_batch = max_batch; h->sup = sup; h->kappa = s.kappa;
    h->off = is_c51d(h) ? make_off_c51d(fc_width, n_actions, sup.N)
                        : make_off(fc_width, sup.N ? n_actions * sup.N : n_actions, arch == FB_ARCH_DUELING || arch == FB_ARCH_AC || arch == FB_ARCH_IQN_DUELING);
    if (is_sac(h)) {                             // (the plain layout, then the two Q heads: off.n covers them)
        h->sac_off.wq1 = h->off.n; h->sac_off.bq1 = h->sac_off.wq1 + fc_width * n_actions;
        h->sac_off.wq2 = h->sac_off.bq1 + n_actions; h->sac_off.bq2 = h->sac_off.wq2 + fc_width * n_actions;
        h->off.n = h->sac_off.bq2 + n_actions;
        h->sac_hbar = 0.98f * logf((float)n_actions); h->sac_alr = 0.f;
    }
    if (is_iqn(h)) {                             // (the plain or the dueling layout, then the embedding: off.n covers it)
        h->iqn_off.we = h->off.n; h->iqn_off.be = h->iqn_off.we + FB_IQN_COS * fc_width;
        h->off.n = h->iqn_off.be + fc_width;
        h->iqn_n = s.n_tau; h->iqn_np = s.n_tau_next; h->iqn_k = s.n_tau_act; h->iqn_eta = 1.f;
        h->iqn_mu = 0; h->iqn_md = MdPar{0.03f, 0.9f, -1.f};      // (Munchausen IQN: off, the paper's values)
    }
    h->hoff = is_c51d(h) ? make_off(fc_width, n_actions * sup.N, 0) : is_iqnd(h) ? make_off(fc_width, n_actions, 0) : h->off;      // (a dueling IQN net: its fold's)
    h->n = h->off.n;
    h->noisy = s.noisy;
    h->noisy_end = is_iqn(h) ? h->iqn_off.we : (int)h->n;      // (where sigma's range [OFF_WF1, .) ends: an IQN net's W_e b_e have none)
    h->ntot = h->noisy ? h->n + h->noisy_end - OFF_WF1 : h->n;
    if (h->noisy) h->nnet = make_noisy(h->off, arch, fc_width, n_actions, sup.N, s.sigma0);
    h->zmax = 64;
    const size_t S = (size_t)3 * max_batch, nb = sizeof(float) * (size_t)h->n, nbt = sizeof(float) * (size_t)h->ntot;
    hipError_t e = hipSuccess;
    auto alloc = [&](auto **p, size_t bytes) {   // zeroed device memory, recorded in h->allocs
        void *q = nullptr;
        if (e == hipSuccess) e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return;
        h->allocs.push_back(q);
        *p = static_cast<std::remove_reference_t<decltype(**p)> *>(q);
        e = hipMemset(q, 0, bytes);
    };
    alloc(&h->params[0], nb); alloc(&h->params[1], nb);
    alloc(&h->adam_m, nbt); alloc(&h->adam_v, nbt); alloc(&h->grad, nbt);
    if (h->noisy) for (int w = 0; w < 2; w++) { alloc(&h->mst[w], nbt); alloc(&h->nz[w], sizeof(float) * (size_t)h->nnet.nz); }      // (zero noise: mean mode)
    if (h->noisy) {
        alloc(&h->nz_zero, sizeof(float) * (size_t)h->nnet.nz);
        alloc(&h->wsig, sizeof(uint4) * (size_t)wsp_w3t(fc_width));
        alloc(&h->a3n, S * 1600 * 6 + 256);
        alloc(&h->ht, S * fc_width * 4 * FC1_SP_KS);
        alloc(&h->sig_seen, sizeof(int));
        if (is_iqn(h)) for (int w = 0; w < 2; w++) alloc(&h->iqn_pbar[w], sizeof(float) * (size_t)fc_width);
        if (e == hipSuccess) e = hipMemset(h->sig_seen, 0xff, sizeof(int));      // (no planes yet)
    }
    alloc(&h->slabs, sizeof(float) * (size_t)h->zmax * CONV_PARAMS);
    if (2 * max_batch > h->zmax) alloc(&h->slabs1, sizeof(float) * (size_t)2 * (max_batch < MAXTB ? max_batch : MAXTB) * CONV1_PARAMS);      // two sub-slabs per sample
    alloc(&h->adam, sizeof(AdamDev));
    alloc(&h->w1s[0], 3 * 8192 * 2); alloc(&h->w1s[1], 3 * 8192 * 2);
    const size_t wsp_bytes = (size_t)wsp_total(fc_width) * sizeof(uint4);
    alloc(&h->wsp[0], wsp_bytes); alloc(&h->wsp[1], wsp_bytes);
    h->nsplit = 3; h->nsplit_train = 3;
    alloc(&h->zeros, 256);
    alloc(&h->a1s, S * 3200 * 6); alloc(&h->a3s, S * 1600 * 6 + 256);
    alloc(&h->p1, S * 3200 * 4); alloc(&h->amax, S * 3200);
    alloc(&h->h2, S * 1600 * 4); alloc(&h->h3, S * 1600 * 4);
    alloc(&h->hf, S * fc_width * 4 * FC1_KS); alloc(&h->q, S * MAXA * 4);
    alloc(&h->qpart, (size_t)(fc_width / 16) * S * (MAXA + 1) * 4);
    alloc(&h->ring_fo, (size_t)max_batch * 4 * sizeof(unsigned long long));
    const size_t Bm = max_batch;
    alloc(&h->dhf, Bm * fc_width * 4); alloc(&h->dh3, Bm * 1600 * 4);
    alloc(&h->dh2, Bm * 1600 * 4); alloc(&h->dp1, Bm * 3200 * 4);
    alloc(&h->gmax, (size_t)(fc_width / 16) * 4);
    alloc(&h->hf_act, S * fc_width * 4 * FC1_SP_KS); alloc(&h->hp_act, sizeof(float) * (size_t)(h->n - h->off.bf1));
    if (sup.N) { alloc(&h->c51_dl, Bm * 64 * 4); alloc(&h->c51_xs, Bm * fc_width * 4); alloc(&h->c51_lt, Bm * 4); }
    if (is_c51d(h) || is_iqn(h)) for (int w = 0; w < 2; w++) alloc(&h->heff[w], sizeof(float) * (size_t)(h->hoff.n - h->off.bf1));
    if (is_ac(h)) {
        const size_t Bt = Bm < MAXTB ? Bm : MAXTB;
        alloc(&h->ac_dl, Bt * 16 * 4); alloc(&h->ac_xs, Bt * fc_width * 4); alloc(&h->ac_r, Bt * 4); alloc(&h->ac_t, Bt);
        alloc(&h->ppo_sum, 6 * 4);
    }
    if (is_sac(h)) {
        const size_t Bt = Bm < MAXTB ? Bm : MAXTB;
        alloc(&h->ac_dl, Bt * 16 * 4); alloc(&h->ac_xs, Bt * fc_width * 4); alloc(&h->sac_w, 8 * 4);
    }
    if (is_iqn(h)) {                             // (sized by the train step's batch limit, not by max_batch: that is the env count)
        const size_t Bt = Bm < MAXTB ? Bm : MAXTB;
        alloc(&h->ac_dl, Bt * 4 * 4); alloc(&h->ac_xs, Bt * fc_width * 4);
        alloc(&h->iqn_dpre, Bt * h->iqn_n * fc_width * 4); alloc(&h->iqn_ctab, Bt * h->iqn_n * FB_IQN_COS * 4);
    }
    alloc(&h->clip_part, sizeof(double) * 256); alloc(&h->clip_out, sizeof(float) * 2);
    if (e == hipSuccess) { const float one = 1.f; e = hipMemcpy(h->clip_out + 1, &one, sizeof(one), hipMemcpyHostToDevice); }      // (no clip yet: norm 0, c 1)
    int rc = e == hipSuccess ? FB_OK : fb_set_error(e == hipErrorOutOfMemory ? FB_ERR_NOMEM : FB_ERR_HIP, "fb_qnet_create: %s", hipGetErrorString(e));
    if (rc == FB_OK) {   // wsp has never been split: parameter versions start ahead of the split versions
        AdamDev a; memset(&a, 0, sizeof(a));
        a.pver[0] = a.pver[1] = 1;
        if (hipMemcpy(h->adam, &a, sizeof(a), hipMemcpyHostToDevice) != hipSuccess) rc = fb_set_error(FB_ERR_HIP, "fb_qnet_create: hipMemcpy failed");
    }
    if (rc == FB_OK) rc = fb_qnet_set_hparams(h, 1e-6f, 0.9f, 0.999f, 1e-8f);
    if (rc == FB_OK && is_sac(h)) rc = sac_write_words(h, 0.2f);      // (behind fb_qnet_set_hparams: the beta powers start at the net's betas)
    if (rc != FB_OK) { fb_qnet_destroy(h); return rc; }                // the single failure exit: whatever was allocated is freed from the same list
    *out = h;
    return FB_OK;
}

extern "C" int fb_qnet_destroy(fb_qnet_t h) {
    if (!h) return FB_OK;
    if (h->split) {
        FbSplitCtx *c = h->split;
        if (c->tstream) { (void)hipStreamSynchronize(c->tstream); (void)hipStreamDestroy(c->tstream); }
        if (c->f) (void)hipFree(c->f);
        delete c;
    }
    for (void *p : h->allocs) (void)hipFree(p);
    delete h;
    return FB_OK;
}

__global__ void flag_wait_kernel(const unsigned long long *flag, unsigned long long v, unsigned *timeouts) { if (threadIdx.x == 0) fb_flag_wait(flag, v, timeouts); }
__global__ void flag_set_kernel(unsigned long long *flag, unsigned long long v) { fb_flag_store(flag, v); }

FbSplitCtx *fb_qnet_split_ctx(fb_qnet_t h) {
    if (!h) return nullptr;
    if (h->split) return h->split->tstream ? h->split : nullptr;
    FbSplitCtx *c = new FbSplitCtx();
    memset(c, 0, sizeof(*c));
    h->split = c;                                // (kept even when incomplete: tstream == NULL means "tried, unavailable")
    int lo = 0, hi = 0;
    bool ok = hipMalloc((void **)&c->f, sizeof(FbSplitFlags)) == hipSuccess && hipMemset(c->f, 0, sizeof(FbSplitFlags)) == hipSuccess;
    hipStream_t ts = nullptr;
    ok = ok && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hipStreamCreateWithPriority(&ts, hipStreamNonBlocking, lo) == hipSuccess;      // (lowest: the train chain beside it is the critical one)
    if (!ok) { (void)hipGetLastError(); return nullptr; }
    c->tstream = ts;
    return c;
}

int fb_split_probe(FbSplitCtx *c, void *stream) {
    if (!c || !c->tstream) return 0;
    if (c->probed_stream == stream && c->seq > 0) return c->probed_ok;
    int lo = 0, hi = 0, ok = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) return 0;
    c->tstream = fb_side_stream_beside(reinterpret_cast<hipStream_t>(stream), lo, c->tstream, &ok);
    c->probed_stream = stream; c->probed_ok = ok;
    return ok;
}

int fb_split_wait(const FbSplitCtx *c, const unsigned long long *flag, unsigned long long v, void *stream) {
    hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, fb_stream(stream), flag, v, &c->f->timeouts[1]);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

int fb_split_set(const FbSplitCtx *, unsigned long long *flag, unsigned long long v, void *stream) {
    hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(1), 0, fb_stream(stream), flag, v);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_split_stats(fb_qnet_t h, int64_t *steps_host, int64_t *clean_host) {
    FB_REQUIRE(h && steps_host && clean_host, "fb_qnet_split_stats: NULL argument");
    *steps_host = 0; *clean_host = 0;
    if (!h->split || !h->split->tstream) return FB_OK;
    FB_CHECK_HIP(hipDeviceSynchronize());
    unsigned v[8] = {0};
    FB_CHECK_HIP(hipMemcpy(v, &h->split->f->clean_count, sizeof(v), hipMemcpyDeviceToHost));
    FB_REQUIRE(!(v[1] | v[2] | v[3] | v[4] | v[5] | v[6]), "fb_qnet_split_stats: waits between the two chains of the split schedule gave up after 1 s (the draw %u, the side stream's entry %u, "
               "the fc1 backward launch's gate %u, the conv backward launch's gate %u, the Adam launch's last wait %u): the results of those steps are not to be trusted", v[1], v[2], v[3], v[4], v[5]);
    *steps_host = (int64_t)h->split->seq; *clean_host = (int64_t)v[0];
    return FB_OK;
}

extern "C" int fb_qnet_num_params(fb_qnet_t h, int64_t *n_host) {
    FB_REQUIRE(h && n_host, "fb_qnet_num_params: NULL argument");
    *n_host = h->ntot;
    return FB_OK;
}

extern "C" int fb_qnet_set_hparams(fb_qnet_t h, float lr, float beta1, float beta2, float eps) {
    FB_REQUIRE(h, "fb_qnet_set_hparams: NULL handle");
    FB_CHECK_HIP(hipDeviceSynchronize());
    AdamDev a;
    FB_CHECK_HIP(hipMemcpy(&a, h->adam, sizeof(a), hipMemcpyDeviceToHost));
    const bool fresh = a.b1 == 0.f && a.b2 == 0.f;
    a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
    if (fresh) { a.b1pow = beta1; a.b2pow = beta2; a.alpha = 0.f; }      // beta1_power / beta2_power initial values
    FB_CHECK_HIP(hipMemcpy(h->adam, &a, sizeof(a), hipMemcpyHostToDevice));
    return FB_OK;
}

extern "C" int fb_qnet_overflow_count(fb_qnet_t h, int reset, int64_t *count_host) {
    FB_REQUIRE(h && count_host, "fb_qnet_overflow_count: NULL argument");
    FB_CHECK_HIP(hipDeviceSynchronize());
    unsigned v = 0;
    FB_CHECK_HIP(hipMemcpy(&v, &h->adam->ovf, sizeof(v), hipMemcpyDeviceToHost));
    if (reset && v) { const unsigned z = 0; FB_CHECK_HIP(hipMemcpy(&h->adam->ovf, &z, sizeof(z), hipMemcpyHostToDevice)); }
    *count_host = (int64_t)v;
    return FB_OK;
}

extern "C" int fb_qnet_set_inference_dtype(fb_qnet_t h, int dtype) {
    FB_REQUIRE(h && (dtype == FB_DTYPE_F32 || dtype == FB_DTYPE_BF16), "fb_qnet_set_inference_dtype: dtype must be FB_DTYPE_F32 or FB_DTYPE_BF16");
    FB_REQUIRE(!(is_ac(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_inference_dtype: an actor-critic net computes in FB_DTYPE_F32 only");
    FB_REQUIRE(!(is_sac(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_inference_dtype: a SAC net computes in FB_DTYPE_F32 only");
    FB_REQUIRE(!(is_iqn(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_inference_dtype: an IQN net computes in FB_DTYPE_F32 only");
    h->nsplit = dtype == FB_DTYPE_BF16 ? 1 : 3;
    return FB_OK;
}

extern "C" int fb_qnet_set_train_dtype(fb_qnet_t h, int dtype) {
    FB_REQUIRE(h && (dtype == FB_DTYPE_F32 || dtype == FB_DTYPE_BF16), "fb_qnet_set_train_dtype: dtype must be FB_DTYPE_F32 or FB_DTYPE_BF16");
    FB_REQUIRE(!(is_ac(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_train_dtype: an actor-critic net trains in FB_DTYPE_F32 only");
    FB_REQUIRE(!(is_sac(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_train_dtype: a SAC net trains in FB_DTYPE_F32 only");
    FB_REQUIRE(!(is_iqn(h) && dtype == FB_DTYPE_BF16), "fb_qnet_set_train_dtype: an IQN net trains in FB_DTYPE_F32 only");
    h->nsplit_train = dtype == FB_DTYPE_BF16 ? 1 : 3;
    return FB_OK;
}

// The host replaced a net's parameters (init, load, target sync): bring its split planes up to date right away.  The forward kernels
// would do it on their own (AdamDev::pver / wver), except the ring-fed conv trunk (conv23_t_kernel<., true>), which has no launch in front
// of it that could; these are rare events, the launch costs nothing that matters.
static void resplit_now(fb_qnet *h, int which, hipStream_t st) {
    const int items = wsplit_items(h->FC);
    hipLaunchKernelGGL(wsplit_kernel, dim3((items + 255) / 256), dim3(256), 0, st, h->params[which], h->wsp[which], h->FC,
                       (const unsigned *)&h->adam->pver[which], (const unsigned *)&h->adam->wver[which]);
    hipLaunchKernelGGL(mark_split_kernel, dim3(1), dim3(1), 0, st, h->adam, which);
}

extern "C" int fb_qnet_init_params(fb_qnet_t h, int which, uint64_t seed, void *stream) {
    FB_REQUIRE(h && (which == 0 || which == 1), "fb_qnet_init_params: bad argument");
    hipLaunchKernelGGL(init_params_kernel, dim3((unsigned)((h->n + 255) / 256)), dim3(256), 0, fb_stream(stream),
                       master(h, which), h->n, h->off, h->FC, h->sup.N ? h->A * h->sup.N : h->A, h->arch == FB_ARCH_DUELING || is_c51d(h) || is_ac(h) || is_iqnd(h), (uint32_t)seed,
                       (uint32_t)(seed >> 32));
    if (is_c51d(h)) {                            // (init_params_kernel's dueling bias is one entry: b_v has N)
        const float b = 0.01f;
        uint32_t bits;
        memcpy(&bits, &b, 4);
        FB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(master(h, which) + h->off.bv), (int)bits, (size_t)h->sup.N, fb_stream(stream)));
    }
    if (is_sac(h)) {                             // (the Q heads' weights drew as every weight does, keyed by their own index; their biases)
        const float b = 0.01f;
        uint32_t bits;
        memcpy(&bits, &b, 4);
        FB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->params[which] + h->sac_off.bq1), (int)bits, (size_t)h->A, fb_stream(stream)));
        FB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->params[which] + h->sac_off.bq2), (int)bits, (size_t)h->A, fb_stream(stream)));
    }
    if (is_iqn(h)) {                             // (W_e drew as every weight does; b_e = 1: a fresh net has phi ~ 1 and starts as the plain net)
        const float b = 1.0f;
        uint32_t bits;
        memcpy(&bits, &b, 4);
        FB_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(master(h, which) + h->iqn_off.be), (int)bits, (size_t)h->FC, fb_stream(stream)));
    }
    if (h->noisy)                                // (mu as the plain net's, then sigma0 / sqrt(fan_in))
        hipLaunchKernelGGL(noisy_sigma_init_kernel, dim3((unsigned)((h->noisy_end - OFF_WF1 + 255) / 256)), dim3(256), 0, fb_stream(stream), h->mst[which], h->nnet, h->noisy_end);
    noisy_materialise(h, which, 0, false, fb_stream(stream));
    env_noise_invalidate(h, which, fb_stream(stream));
    c51d_fold(h, which, fb_stream(stream));
    hipLaunchKernelGGL(w1_split_kernel, dim3(32), dim3(256), 0, fb_stream(stream), h->params[which], h->w1s[which], &h->adam->pver[which]);
    resplit_now(h, which, fb_stream(stream));
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_load_params(fb_qnet_t h, int which, const float *flat, void *stream) {
    FB_REQUIRE(h && flat && (which == 0 || which == 1), "fb_qnet_load_params: bad argument");
    FB_CHECK_HIP(hipMemcpyAsync(master(h, which), flat, sizeof(float) * (size_t)h->ntot, hipMemcpyDeviceToDevice, fb_stream(stream)));
    noisy_materialise(h, which, 0, false, fb_stream(stream));
    env_noise_invalidate(h, which, fb_stream(stream));
    hipLaunchKernelGGL(w1_split_kernel, dim3(32), dim3(256), 0, fb_stream(stream), h->params[which], h->w1s[which], &h->adam->pver[which]);
    c51d_fold(h, which, fb_stream(stream));
    resplit_now(h, which, fb_stream(stream));
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_store_params(fb_qnet_t h, int which, float *flat, void *stream) {
    FB_REQUIRE(h && flat && (which == 0 || which == 1), "fb_qnet_store_params: bad argument");
    FB_CHECK_HIP(hipMemcpyAsync(flat, master(h, which), sizeof(float) * (size_t)h->ntot, hipMemcpyDeviceToDevice, fb_stream(stream)));
    return FB_OK;
}

extern "C" int fb_qnet_get_adam_state(fb_qnet_t h, float *m, float *v, float *beta_pows_host) {
    FB_REQUIRE(h, "fb_qnet_get_adam_state: NULL handle");
    FB_CHECK_HIP(hipDeviceSynchronize());
    const size_t nb = sizeof(float) * (size_t)h->ntot;
    if (m) FB_CHECK_HIP(hipMemcpy(m, h->adam_m, nb, hipMemcpyDeviceToDevice));
    if (v) FB_CHECK_HIP(hipMemcpy(v, h->adam_v, nb, hipMemcpyDeviceToDevice));
    if (beta_pows_host) {
        AdamDev a;
        FB_CHECK_HIP(hipMemcpy(&a, h->adam, sizeof(a), hipMemcpyDeviceToHost));
        beta_pows_host[0] = a.b1pow; beta_pows_host[1] = a.b2pow;
    }
    return FB_OK;
}

extern "C" int fb_qnet_set_adam_state(fb_qnet_t h, const float *m, const float *v, const float *beta_pows_host) {
    FB_REQUIRE(h, "fb_qnet_set_adam_state: NULL handle");
    FB_CHECK_HIP(hipDeviceSynchronize());
    const size_t nb = sizeof(float) * (size_t)h->ntot;
    if (m) FB_CHECK_HIP(hipMemcpy(h->adam_m, m, nb, hipMemcpyDeviceToDevice));
    if (v) FB_CHECK_HIP(hipMemcpy(h->adam_v, v, nb, hipMemcpyDeviceToDevice));
    if (beta_pows_host) {
        AdamDev a;
        FB_CHECK_HIP(hipMemcpy(&a, h->adam, sizeof(a), hipMemcpyDeviceToHost));
        a.b1pow = beta_pows_host[0]; a.b2pow = beta_pows_host[1];
        FB_CHECK_HIP(hipMemcpy(h->adam, &a, sizeof(a), hipMemcpyHostToDevice));
    }
    return FB_OK;
}

// ------------------------------------------------------------------ launch plan
// Every kernel of a forward / train step, individually addressable so that bench.py can time one
// kernel on the caller's stream (fb_qnet_profile_kernel) with exactly the launch geometry the real
// step uses.  `only` < 0 launches the whole plan.
enum KernelId {
    K_CONV1 = 0, K_CONV2, K_CONV3, K_FC1, K_HEAD, K_LOSS, K_FC1_BWD, K_CONV3_BWD, K_CONV2_BWD, K_CONV1_DW, K_SLAB, K_ADAM,
    K_COUNT
};

struct Plan {
    Slices sl; int ns;                       // forward slices
    bool nib;                                // states are the env's nibble state (acting path)
    uint8_t *actions; float epsilon; uint64_t seed, step;
    bool train;                              // forward only when false
    int algo, B; const uint8_t *s, *a, *t; const float *r, *isw; double gamma;
    float *loss, *abs_err, *y, *G; bool apply_adam, tick;
    FbHeadRider *head_rider;                 // acting path: describe the head work instead of launching it (fb_vec_step)
    const FbSampleRider *sample_rider;       // train plan: random.sample for the next step rides in the conv3 backward launch
    const FbRingSrc *ring;                   // the minibatch lives in the replay's frame ring (no gathered copies): conv trunk in one launch
    // the split schedule (fb_common.hip).  Acting plan: the fc1 launch stores trunk_done.  Train plan: gate workgroups in the fc1 backward
    // launch (trunk_done) and the conv backward launch (fc1_done), the Adam launch's last thread waits for env_done
    const FbSplitCtx *split;
    // fb_eval_run / fb_eval_q: the fused acting trunk (five states per workgroup) at ANY state count, so that a state's Q values do not
    // depend on how many other states share the launch (the small-batch kernels below 256 states round differently)
    bool any_rows;
    float *probs;                            // C51 forward plans: the head also writes the probabilities f32[row][A][N] (fb_qnet_forward_dist)
    bool no_head;                            // C51 / IQN forward plans: conv1 .. fc1 only (fb_qnet_act_nib_env_noise launches its own head)
    // an actor-critic net.  Forward plans with ac_value set: the policy head (fb_ac.hip) instead of the plain one -- value f32[rows], logits
    // f32[rows][A] / logp f32[rows] or NULL, p.actions NULL: no action; ac_greedy: the first maximum instead of a draw.  Train plans: the
    // advantages, the returns and n_total (p.r / p.isw / p.gamma stay unset)
    float *ac_value, *ac_logits, *ac_logp; int ac_greedy;
    const float *ac_adv, *ac_ret; float ac_nt;
    // a PPO train plan of an actor-critic net: the clipped-surrogate loss instead of A2C's; the rollout's log-probabilities and values;
    // ppo_sel (or NULL): where sample b reads ac_adv / ac_ret / ppo_logp / ppo_value
    bool ppo; const float *ppo_logp, *ppo_value; const long long *ppo_sel;
    // a SAC net.  Forward plans with policy_head set: the SAC head (fb_sac.hip) instead of the plain one -- ac_value (or NULL) the soft state
    // value, ac_logits / ac_logp as above, sac_q1 / sac_q2 f32[rows][A] or NULL.  Train plans: three slices as FB_ALGO_DOUBLE's, p.r / p.t /
    // p.gamma / p.y as a scalar step's; sac_temp: the temperature update runs (the CALLER exports nothing and alpha_lr > 0)
    bool policy_head; float *sac_q1, *sac_q2; bool sac_temp;
    // an IQN net.  Forward plans with iqn_theta set: theta f32[rows][iqn_m][A] at iqn_tau instead of the plain head over the fold.  Train
    // plans: three slices as FB_ALGO_DOUBLE's; iqn_tau / iqn_tau_next (or NULL: the draws of p.seed / p.step), iqn_double: a* from the online net;
    // p.y: T f32[B][N'] or NULL
    // iqn_mu: the Munchausen target (the net's setting when the plan was made): the slice at rows B .. is s through the TARGET net
    const float *iqn_tau, *iqn_tau_next; int iqn_m; float *iqn_theta; bool iqn_double, iqn_mu;
};

// (IntTag, with_bool, with_actions: fb_head.h)  nsp: the operands' planes, 3 = fp32-equivalent, 1 = bf16
template <class F> static void with_nsp(int nsp, F f) { if (nsp == 3) f(IntTag<3>{}); else f(IntTag<1>{}); }

template <class T> static void put_seed_words(T &c, uint64_t seed, uint64_t step) {      // the four words the head kernels take
    c.seed_lo = (uint32_t)seed; c.seed_hi = (uint32_t)(seed >> 32);
    c.step_lo = (uint32_t)step; c.step_hi = (uint32_t)(step >> 32);
}

// What the stages of a plan share: where it runs and the values derived from the plan.  run_plan below is the sequence of the stages.
struct PlanCtx {
    int only; hipStream_t st;                // `only` < 0: the whole plan; else the launches of that KernelId alone
    int maxc, total;                         // states of the largest slice / of all slices
    bool big, trunk, fused, c51, ac, sac, iqn; // ac: the loss is fb_ac.hip's, fb_sac.hip's or fb_iqn.hip's two launches (an actor-critic, SAC or IQN net)
    bool state_trunk;                        // gathered states through conv1_pool + conv23_t with planes, then large_pass's fc1 alone (plan_ctx)
    int nsp, stot; size_t pl1, pl2;          // stot: rows of the workspace; pl1 / pl2: its plane pitch after conv1 / conv2, conv3
};
static bool runs(const PlanCtx &c, int id) { return c.only < 0 || c.only == id; }      // the launches of KernelId `id` are part of this run

static PlanCtx plan_ctx(const fb_qnet *h, const Plan &p, int only, hipStream_t st) {
    PlanCtx c{only, st, 0, 0};
    for (int z = 0; z < p.ns; z++) { if (p.sl.s[z].count > c.maxc) c.maxc = p.sl.s[z].count; c.total += p.sl.s[z].count; }
    // >= 256 samples in a slice: thousands of tiles, one wave per tile (no K split); below: K split over waves
    // >= 256 states per slice: the LDS-staged two-plane-fp16 kernels (conv1_sp / conv23_sp / fc1_sp).  Forward-only plans take
    // them with one slice; TRAINING plans run them in passes, one per run of consecutive slices that go through the same net
    // (DQN: s and s' in one pass; Nature / PER: s online, s' target; Double: s, s' online + s' target), with fp32 side outputs
    // (pooled conv1 + pool positions, conv2, conv3) for the backward kernels.  nsp: 3 = fp32-equivalent, 1 = bf16 operands.
    c.big = c.maxc >= 256 || p.any_rows;
    c.nsp = p.train ? h->nsplit_train : h->nsplit;
    c.stot = 3 * h->max_batch; c.pl1 = (size_t)c.stot * 3200; c.pl2 = (size_t)c.stot * 1600;
    c.trunk = p.ring != nullptr;                 // ring-fed minibatch (any batch size): the whole conv trunk per state in one launch
    // the acting path on nibble states (forward-only plans of one slice): conv1 + conv2 + conv3 in ONE launch
    // (conv23_sp_kernel<., 5, true>), five states per workgroup.  Its fc1 partial sums are in hf_act, its head parameters in hp_act
    c.fused = c.big && p.nib && !p.train && !c.trunk && p.ns == 1;
    c.c51 = h->sup.N > 0;
    c.sac = is_sac(h);
    c.iqn = is_iqn(h);
    c.ac = is_ac(h) || c.sac || c.iqn;
    // an actor-critic train step on 256 GATHERED states: the per-state conv trunk of the smaller batches, writing conv3's planes, then
    // fc1_sp -- the arithmetic of the ring-fed form (ring_trunk), so that the two forms of an A2C chunk agree bit for bit at every size
    // (the large-batch trunk sums conv2 / conv3 in another order).  The ring-fed form is the one the A2C loop runs
    c.state_trunk = c.ac && p.train && c.big && !c.trunk;
    return c;
}

// small batches: conv2 + conv3 in one launch on the split planes (conv23_t_kernel); the conv1 launch in front re-splits the conv
// weights of every net of the plan whose parameters moved (decided on the device), the conv2+conv3 launch records it
static C23T trunk_args(fb_qnet *h, const Plan &p, const PlanCtx &c, SplitJob *job) {      // job: conv1_pool_kernel's
    C23T c23t;
    memset(job, 0, sizeof(*job)); memset(&c23t, 0, sizeof(c23t));
    job->FC = h->FC;
    c23t.sl = p.sl; c23t.p1 = h->p1; c23t.h2 = h->h2; c23t.h3 = h->h3; c23t.ovf = &h->adam->ovf;
    for (int z = 0; z < p.ns; z++) {
        const int which = p.sl.s[z].params == h->params[1] ? 1 : 0;
        c23t.w[z] = h->wsp[which] + WSP_W2;
        if (c.only < 0) {
            job->params[which] = h->params[which]; job->wsp[which] = h->wsp[which];
            job->pver[which] = &h->adam->pver[which]; job->wverc[which] = &h->adam->wverc[which];
            c23t.pver[which] = &h->adam->pver[which]; c23t.wverc[which] = &h->adam->wverc[which];
        }
    }
    return c23t;
}

// the ring-fed trunk: conv1 + pool + conv2 + conv3 of every state in ONE launch
static void ring_trunk(fb_qnet *h, const Plan &p, const PlanCtx &c) {
    SplitJob job;                                     // (unused here: the ring-fed trunk has no conv1_pool launch in front of it)
    C23T c23t = trunk_args(h, p, c, &job);
    if (c.big) { c23t.a3s = h->a3s; c23t.pl3 = c.pl2; }     // >= 256 states per slice: fc1_sp_kernel follows and reads conv3's output as planes
    c23t.ring = *p.ring; c23t.p1o = h->p1; c23t.amax = h->amax; c23t.ring_fo = h->ring_fo;
    const bool w16 = c.maxc * p.ns <= 256;            // at most one workgroup per CU anyway: spend the idle SIMD slots on conv1's second round
    const bool nst = p.ring->c.nstep > 1;             // n-step view: the same kernels with the n-step return (NST)
    with_nsp(c.nsp, [&](auto ns) { with_bool(w16, [&](auto w) { with_bool(nst, [&](auto nv) {
        constexpr bool W16 = decltype(w)::value;
        hipLaunchKernelGGL((conv23_t_kernel<decltype(ns)::value, true, W16, decltype(nv)::value>), dim3(c.maxc, p.ns), dim3(W16 ? 1024 : 512), 0, c.st, c23t);
    }); }); });
}

// one large-batch pass, conv1_sp -> conv23_sp -> fc1_sp (behind the ring-fed trunk fc1 alone), from slice *z to the next pass's first
static int large_pass(fb_qnet *h, const Plan &p, const PlanCtx &c, int *z) {
    const int z0 = *z;
    int z1 = z0 + 1;
    while (z1 < p.ns && p.sl.s[z1].params == p.sl.s[z0].params && p.sl.s[z1].count == p.sl.s[z0].count && p.sl.s[z1].s_off == p.sl.s[z1 - 1].s_off + p.sl.s[z1 - 1].count) z1++;
    const Slice s0 = p.sl.s[z0];
    const int which = s0.params == h->params[1] ? 1 : 0, row0 = s0.s_off, rows = s0.count * (z1 - z0);
    // stale split weights are refreshed by the leading workgroups of the conv1 launch, decided on the device from
    // AdamDev::pver / wver (a single profiled kernel never re-splits: fb_qnet_profile_kernel brings wsp up to date once)
    const unsigned *pver = c.only < 0 ? &h->adam->pver[which] : nullptr;
    unsigned *wver = c.only < 0 ? &h->adam->wver[which] : nullptr;
    Slice sl = s0;
    sl.count = rows;
    C1Side side;
    memset(&side, 0, sizeof(side));
    if (z1 - z0 > 1) { side.per = s0.count; side.st1 = p.sl.s[z0 + 1].states; side.st2 = z1 - z0 > 2 ? p.sl.s[z0 + 2].states : p.sl.s[z0 + 1].states; }
    if (p.train) { side.p1 = h->p1; side.amax = h->amax; }
    const int t1p = (rows * 100 + 7) / 8, gsp = min(256, (t1p + C1_WAVES - 1) / C1_WAVES);      // one 12-wave workgroup per CU, the waves stride over the tiles
    if (!c.trunk && !c.state_trunk && !c.fused && runs(c, K_CONV1))
        hipLaunchKernelGGL(conv1_sp_kernel, dim3(gsp), dim3(64 * C1_WAVES), 0, c.st, sl, (const uint8_t *)h->zeros, h->a1s, c.pl1, c.nsp, h->wsp[which], h->FC, pver, (const unsigned *)wver, side, &h->adam->ovf);
    C23Args c23{h->a1s + (size_t)row0 * 3200, c.pl1, h->wsp[which] + WSP_W2, s0.params + OFF_B2, s0.params + OFF_B3, h->a3s + (size_t)row0 * 1600, c.pl2, rows, pver, wver, c.only < 0 ? &h->adam->wverc[which] : nullptr,
                p.train ? h->h2 + (size_t)row0 * 1600 : nullptr, p.train ? h->h3 + (size_t)row0 * 1600 : nullptr,
                s0.states, s0.w1s, s0.params + OFF_B1, s0.params, h->wsp[which], h->FC, &h->adam->ovf};
    Fc1Args af{h->a3s + (size_t)row0 * 1600, c.pl2, h->zeros, h->wsp[which] + WSP_WF1, (c.fused ? h->hf_act : h->hf) + (size_t)row0 * h->FC, c.stot, rows, h->FC,
               c.fused ? pver : nullptr, c.fused ? wver : nullptr, nullptr, 0,
               c.fused ? head_base(h, s0.params) + h->off.bf1 : nullptr, c.fused ? h->hp_act : nullptr, c.fused ? (int)(h->hoff.n - h->off.bf1) : 0,
               c.fused && p.split && c.only < 0 ? &p.split->f->trunk_done : nullptr, p.split ? p.split->seq : 0};
    // behind the ring-fed trunk the groups only differ in fc1's weights: when the next group (the target net's slices) follows this
    // one row for row and starts on a tile boundary, ONE fc1 launch takes both (two launches of 128 + 64 workgroups each left
    // half the chip idle twice: 8.9 + 8.5 us at B = 256 against one of 192)
    if (c.trunk && z1 < p.ns && rows % 128 == 0) {
        int z2 = z1 + 1;
        while (z2 < p.ns && p.sl.s[z2].params == p.sl.s[z1].params && p.sl.s[z2].s_off == p.sl.s[z2 - 1].s_off + p.sl.s[z2 - 1].count) z2++;
        const Slice sn = p.sl.s[z1];
        if (z2 == p.ns && sn.s_off == row0 + rows && sn.params != s0.params) {
            int rows2 = 0;
            for (int z = z1; z < z2; z++) rows2 += p.sl.s[z].count;
            af.w2 = h->wsp[sn.params == h->params[1] ? 1 : 0] + WSP_WF1; af.m_split = rows; af.M = rows + rows2;
            z1 = z2;
        }
    }
    *z = z1;
    // five states per workgroup (125 of the 128 MFMA rows; 1024 envs = 205 workgroups: alone it costs what four per workgroup on
    // all 256 CUs cost, and in the split schedule the fifth of the chip it leaves is where the train chain runs beside it)
    const dim3 gc((rows + 4) / 5), gf(((af.M + 127) / 128) * (h->FC / 64) * FC1_SP_KS);    // FC % 128 == 0 (fb_qnet_create)
    // split schedule, more than one round of trunk workgroups (one per CU, 256 CUs) with a partial last round: that round's first
    // workgroup says when it has been placed -- the train chain on the other stream starts then (fb_sampler.h)
    if (c.fused && p.split && c.only < 0 && gc.x > 256 && gc.x % 256 != 0) { c23.round_flag = &p.split->f->last_round; c23.round_val = p.split->seq; c23.round_blk = (int)(gc.x / 256) * 256; }
    with_nsp(c.nsp, [&](auto ns) {
        if (!c.trunk && !c.state_trunk && runs(c, K_CONV2))      // fused: conv1 .. conv3; else conv3 rides in conv2's launch
            with_bool(c.fused, [&](auto fu) { hipLaunchKernelGGL((conv23_sp_kernel<decltype(ns)::value, 5, decltype(fu)::value>), gc, dim3(512), 0, c.st, c23); });
        if (runs(c, K_FC1)) hipLaunchKernelGGL(fc1_sp_kernel<decltype(ns)::value>, gf, dim3(256), 0, c.st, af);
    });
    // the fc1 launch copies one head parameter per thread: a distributional head (C51 / QR, A N columns) can outgrow a small
    // launch's threads, and the rest of the copy follows it on the same stream (these nets take the one-stream order)
    if (c.fused && (c.only < 0 || c.only == K_FC1) && (long long)af.hp_n > (long long)gf.x * 256) {
        const size_t done = (size_t)gf.x * 256;
        FB_CHECK_HIP(hipMemcpyAsync(h->hp_act + done, af.hp_src + done, sizeof(float) * ((size_t)af.hp_n - done), hipMemcpyDeviceToDevice, c.st));
    }
    return FB_OK;
}

// the small-batch forward: conv1_pool -> conv23_t (behind the ring-fed trunk neither) -> fc1_fk
// small batches: the whole K per workgroup (fc1_fk_kernel), which lets training skip the head and loss launches
// planes: conv3's output as planes too (fc1_sp_kernel follows: a gathered actor-critic batch of 256, run_plan)
static void small_trunk(fb_qnet *h, const Plan &p, const PlanCtx &c, bool planes) {
    SplitJob job;
    C23T c23t = trunk_args(h, p, c, &job);
    if (planes) { c23t.a3s = h->a3s; c23t.pl3 = c.pl2; }
    const int t1 = (c.maxc * 100 + 7) / 8;
    if (runs(c, K_CONV1))
        with_bool(p.nib, [&](auto nib) { hipLaunchKernelGGL(conv1_pool_kernel<decltype(nib)::value>, dim3((t1 + 3) / 4, 1, p.ns), dim3(256), 0, c.st, p.sl, h->p1, h->amax, job); });
    if (runs(c, K_CONV2))                                // (conv3 rides in the same launch)
        with_nsp(c.nsp, [&](auto ns) { hipLaunchKernelGGL((conv23_t_kernel<decltype(ns)::value, false>), dim3(c.maxc, p.ns), dim3(512), 0, c.st, c23t); });
}

static void small_forward(fb_qnet *h, const Plan &p, const PlanCtx &c) {
    if (!c.trunk) small_trunk(h, p, c, false);
    if (runs(c, K_FC1)) {
        FkArgs fa;
        fa.sl = p.sl; fa.h3 = h->h3; fa.hf = h->hf; fa.qpart = p.train && !c.c51 && !c.ac ? h->qpart : nullptr; fa.FC = h->FC; fa.A = h->A;      // (C51 / actor-critic: the head is the loss launches' own work)
        fa.dueling = h->arch == FB_ARCH_DUELING; fa.stot = c.stot; fa.off = h->off;
        hipLaunchKernelGGL(fc1_fk_kernel, dim3((c.maxc + 15) / 16, h->FC / 16, p.ns), dim3(512), 0, c.st, fa);
    }
}

static void launch_dist_head(const fb_qnet *h, const C51HeadArgs &H, int rows, hipStream_t st) {      // (C51 / QR; one wave per row)
    with_actions(h->A, [&](auto a) {
        if (is_qr(h)) hipLaunchKernelGGL(qr_head_kernel<decltype(a)::value>, dim3((rows + 3) / 4), dim3(256), 0, st, H);
        else hipLaunchKernelGGL(c51_head_kernel<decltype(a)::value>, dim3((rows + 3) / 4), dim3(256), 0, st, H);
    });
}

// the head: launched on its own, or described into the rider (p.head_rider) for the launch that carries it
static void head_stage(fb_qnet *h, const Plan &p, const PlanCtx &c) {
    auto shared = [&](auto &H) {                 // the fields every head's struct has: where fc1's partial sums are and the head's shape
        H.hf = c.fused ? h->hf_act : h->hf; H.stot = c.stot; H.nks = c.big ? FC1_SP_KS : 1; H.FC = h->FC; H.A = h->A;
    };
    auto core = [&](auto &C) {                   // ... and what C51Core and HeadCore add to them (hoff: = off but for a folded head, whose layout is plain)
        shared(C); C.q = h->q; C.off = h->hoff; C.actions = p.actions; C.epsilon = p.epsilon;
        put_seed_words(C, p.seed, p.step);
    };
    // the heads of fb_ac.hip / fb_sac.hip / fb_iqn.hip, each a launch of its own over all rows.  P: the net's parameters (act_copy: of a
    // fused acting forward the copy its fc1 launch took)
    auto side = [&](auto &H, bool act_copy) {
        memset(&H, 0, sizeof(H));
        shared(H); H.rows = c.total; H.off = h->off; H.P = act_copy && c.fused ? h->hp_act - h->off.bf1 : p.sl.s[0].params;
    };
    auto policy = [&](auto &H) {                 // what an actor-critic and a SAC head put out alike
        side(H, true);
        H.logits = p.ac_logits; H.value = p.ac_value; H.logp = p.ac_logp; H.actions = p.actions; H.greedy = p.ac_greedy;
        put_seed_words(H, p.seed, p.step);
    };
    if (c.c51 && !p.train && !p.no_head && runs(c, K_HEAD)) {           // C51: the distributional head (stand-alone launch only; no env rider)
        C51HeadArgs H;
        H.sl = p.sl; H.nslices = p.ns; H.params = nullptr;
        for (int z = 0; z < p.ns; z++) H.sl.s[z].params = head_base(h, p.sl.s[z].params);      // (a dueling C51 net: its folded head)
        C51Core &C = H.c;
        core(C); C.probs = p.probs; C.sup = h->sup; C.key_of = nullptr; C.stream = FB_STREAM_EPS;
        if (p.head_rider) {                          // fb_eval_run: describe the work (fb_qnet_c51_eval_head launches it)
            memset(p.head_rider, 0, sizeof(*p.head_rider));
            p.head_rider->c.hf = C.hf; p.head_rider->c.stot = c.stot; p.head_rider->c.nks = C.nks;
            p.head_rider->params = c.fused ? h->hp_act - h->off.bf1 : H.sl.s[0].params;
        } else launch_dist_head(h, H, c.total, c.st);
    }
    if (c.sac && !p.train && p.policy_head && runs(c, K_HEAD)) {       // a SAC net's head (fb_sac.hip)
        SacHeadArgs H;
        policy(H);
        H.so = h->sac_off; H.sw = h->sac_w; H.q1 = p.sac_q1; H.q2 = p.sac_q2;
        fb_sac_launch_head(c.st, H);
        return;
    }
    if (c.iqn && !p.train && p.iqn_theta && runs(c, K_HEAD)) {         // an IQN net's theta at the caller's tau (fb_iqn.hip)
        IqnHeadArgs H;
        side(H, false);
        H.M = p.iqn_m; H.io = h->iqn_off; H.dueling = is_iqnd(h) ? 1 : 0; H.tau = p.iqn_tau; H.theta = p.iqn_theta;
        fb_iqn_launch_head(c.st, H);
        return;
    }
    if (c.ac && !c.sac && !c.iqn && !p.train && p.ac_value && runs(c, K_HEAD)) {  // an actor-critic net's policy head (fb_ac.hip)
        AcHeadArgs H;
        policy(H);
        fb_ac_launch_head(c.st, H);
        return;
    }
    // (an actor-critic net without ac_value: the plain head over W_pi b_pi, the logits as "Q"; its train plans: the loss launches' own work)
    if (!c.c51 && !p.no_head && !(p.train && (c.ac || !c.big)) && runs(c, K_HEAD)) {    // (small-batch training gets Q from fc1_fk_kernel's shares instead)
        HeadArgs H;
        H.sl = p.sl; H.nslices = p.ns;
        for (int z = 0; z < p.ns; z++) H.sl.s[z].params = head_base(h, p.sl.s[z].params);      // (an IQN net: its fold; every scalar net: its parameters)
        HeadCore &C = H.c;
        core(C); C.dueling = h->arch == FB_ARCH_DUELING;
        // (the rider of a fused acting forward reads the head's parameters from the copy that forward's fc1 launch took: b_fc1 on)
        if (p.head_rider) { p.head_rider->c = C; p.head_rider->params = c.fused ? h->hp_act - h->off.bf1 : H.sl.s[0].params; p.head_rider->on = 1; p.head_rider->on_arrival = nullptr; p.head_rider->arrival_val = 0; }   // rides in the env launch
        else hipLaunchKernelGGL(head_kernel, dim3((c.total + 3) / 4), dim3(256), 0, c.st, H);
    }
}

// the loss.  Scalar: large batches only (small ones: fc1_bwd2_kernel's own work).  C51: per-sample distribution / projection / dhf, then
// the per-unit reductions; QR: per-sample targets / quantile Huber loss / dhf, then C51's per-unit reductions
static void loss_stage(fb_qnet *h, const Plan &p, const PlanCtx &c) {
    const int B = p.B, FC = h->FC;
    auto shared = [&](auto &L) {                 // the fields every family's loss struct has: the shapes, fc1's partial sums of the slices, the actions, dhf out
        L.B = B; L.FC = FC; L.A = h->A; L.stot = c.stot; L.nks = c.big ? FC1_SP_KS : 1; L.hf = h->hf; L.act = p.a; L.dhf = h->dhf;
    };
    auto transition = [&](auto &L) { L.rew = p.r; L.term = p.t; L.gamma = p.gamma; };      // ... and those of every loss that bootstraps
    // the losses of fb_ac.hip / fb_sac.hip / fb_iqn.hip: the net's own layout, the per-sample row in ac_dl
    auto side = [&](auto &L) { memset(&L, 0, sizeof(L)); shared(L); L.off = h->off; L.dl = h->ac_dl; };
    FbAdamHead *const adam_head = h->adam;
    if (c.iqn) {                                 // IQN: per-sample a* / T / theta / loss / d theta / dhf, then the per-unit reductions (fb_iqn.hip)
        IqnLossMuArgs L;                         // (IqnLossArgs, then Munchausen's fields: all zero = the hard target)
        side(L); transition(L);
        // a* from the target net's fold at its rows of s' (2 B ..), or (double_q) from the online net's at B ..  Munchausen: both Qbar rows over
        // the TARGET net's fold, s at rows B .., s' at rows 2 B .. (iqn_train)
        const bool tgt = p.iqn_mu || !p.iqn_double;
        L.P0 = h->params[0]; L.P1 = h->params[1]; L.F = head_base(h, h->params[tgt ? 1 : 0]); L.arow0 = tgt ? 2 * B : B;
        L.N = h->iqn_n; L.Np = h->iqn_np; L.io = h->iqn_off; L.kappa = h->kappa;
        L.tau = p.iqn_tau; L.tau_next = p.iqn_tau_next;
        put_seed_words(L, p.seed, p.step);
        L.gw = h->ac_xs; L.dpre = h->iqn_dpre; L.ctab = h->iqn_ctab; L.t_out = p.y;
        L.isw = p.isw; L.abs_err = p.abs_err;    // (both set: the prioritized form; the uniform calls leave both NULL)
        L.foff = h->hoff; L.dueling = is_iqnd(h) ? 1 : 0;       // (L.F is a fold: the plain layout's offsets, whatever the net's)
        if (p.iqn_mu) { L.mu = 1; L.temp = h->iqn_md.tau; L.alpha = h->iqn_md.alpha; L.clip_lo = h->iqn_md.clip; L.srow0 = B; }
        fb_iqn_launch_loss(c.st, L);
        const IqnGradArgs gA{B, FC, h->A, h->iqn_n, h->off, h->iqn_off, h->ac_dl, h->ac_xs, h->dhf, h->iqn_dpre, h->iqn_ctab, p.G, p.loss, h->gmax,
                             adam_head, p.tick, is_iqnd(h) ? 1 : 0};
        fb_iqn_launch_grad(c.st, gA);
        return;
    }
    if (c.sac) {                                 // SAC: per-sample target / losses / dz / dQ / dhf, then the per-unit reductions (fb_sac.hip)
        SacPerLossArgs L;                        // (SacLossArgs, then the prioritized form's two fields)
        side(L); transition(L);
        L.P0 = h->params[0]; L.P1 = h->params[1]; L.so = h->sac_off; L.sw = h->sac_w; L.xs = h->ac_xs; L.y_out = p.y;
        L.isw = p.isw; L.abs_err = p.abs_err;    // (both set: the prioritized form; the uniform calls leave both NULL and launch the kernel of before)
        if (p.isw) fb_sac_launch_per_loss(c.st, L);
        else fb_sac_launch_loss(c.st, L);
        const SacGradArgs gA{B, FC, h->A, h->off, h->sac_off, h->ac_dl, h->ac_xs, h->dhf, p.G, p.loss, h->gmax, adam_head,
                             p.tick, h->sac_w, h->sac_hbar, h->sac_alr, p.sac_temp ? 1 : 0};
        fb_sac_launch_grad(c.st, gA);
        return;
    }
    if (c.ac) {                                  // actor-critic: per-sample loss / dz / dV / dhf, then the per-unit reductions (fb_ac.hip)
        AcLossArgs L;
        side(L);
        L.P = h->params[0]; L.adv = p.ac_adv; L.ret = p.ac_ret; L.nt = p.ac_nt; L.cv = h->ac_cv; L.ce = h->ac_ce; L.xs = h->ac_xs;
        if (p.ppo) fb_ac_launch_ppo_loss(c.st, PpoLossArgs{L, p.ppo_sel, p.ppo_logp, p.ppo_value, h->ppo_eps, h->ppo_vclip});
        else fb_ac_launch_loss(c.st, L);
        const AcGradArgs gA{B, FC, h->A, h->off, h->ac_dl, h->ac_xs, h->dhf, p.ac_nt, h->ac_cv, h->ac_ce, p.G, p.loss, h->gmax,
                            adam_head, p.tick, p.ppo ? 5 : 3};
        fb_ac_launch_grad(c.st, gA);
        return;
    }
    if (!c.c51) {                                // (large batches only, run_plan: nks is fc1_sp_kernel's 4 K slices)
        LossArgs L;
        shared(L); transition(L);
        L.algo = p.algo; L.dueling = h->arch == FB_ARCH_DUELING; L.off = h->off;
        L.params = h->params[0]; L.q = h->q; L.isw = p.isw;
        L.grad = p.G; L.loss = p.loss; L.abs_err = p.abs_err; L.y_out = p.y; L.gmax = h->gmax;
        // data-parallel path: the loss kernel advances the Adam step counter as well (once per fb_qnet_apply_adam), so the
        // apply needs no launch of its own for it
        // (at most one tick per Adam update: guarded on the device by AdamDev::ticks / applies)
        L.adam = h->adam; L.tick = p.tick;
        const bool dp = p.algo == FB_ALGO_DOUBLE_PER, hu = h->huber > 0.f, md = is_mdqn_algo(p.algo);
        if (md) L.algo = p.algo == FB_ALGO_MDQN_PER ? FB_ALGO_PER : FB_ALGO_NATURE;      // (L.algo: the loss's form alone)
        if (dp) L.algo = FB_ALGO_PER;
        const dim3 grid(FC / 16);
        // (delta = 0 and an older algo: the kernels and arguments of before the options existed)
        if (dp || hu) fb_qnet_launch_loss_head_x(dp, hu, md, grid.x, c.st, &L, &h->md, h->huber);      // (the extended kernel: fb_qnet_x.hip's code object)
        else if (md) hipLaunchKernelGGL(loss_head_md_kernel, grid, dim3(256), 0, c.st, L, h->md);
        else hipLaunchKernelGGL(loss_head_kernel, grid, dim3(256), 0, c.st, L);
        return;
    }
    const bool pw = is_per_algo(p.algo);         // (prioritized: weighted loss; the priorities are KL (C51) / l_b (QR))
    auto dist = [&](auto &L) {                   // the fields C51LossArgs and QRLossArgs have in common
        shared(L); transition(L); L.off = h->hoff;
        L.p_on = head_base(h, h->params[0]); L.p_next = head_base(h, p.sl.s[1].params);
        L.p_tgt = head_base(h, p.ns > 2 ? p.sl.s[2].params : p.sl.s[1].params);
        L.dl = h->c51_dl; L.xs = h->c51_xs; L.lterm = h->c51_lt;
        L.isw = pw ? p.isw : nullptr; L.abs_err = pw ? p.abs_err : nullptr;
    };
    with_actions(h->A, [&](auto a) { with_bool(pw, [&](auto w) {
        if (is_qr(h)) {
            QRLossArgs L;
            dist(L);
            L.algo = is_double_qr(p.algo) ? FB_ALGO_QR_DOUBLE : FB_ALGO_QR; L.N = h->sup.N; L.kappa = h->kappa;
            hipLaunchKernelGGL((qr_loss_kernel<decltype(a)::value, decltype(w)::value>), dim3((B + 3) / 4), dim3(256), 0, c.st, L);
        } else {
            C51LossArgs L;
            dist(L);
            L.algo = is_double_c51(p.algo) ? FB_ALGO_C51_DOUBLE : FB_ALGO_C51; L.sup = h->sup;
            hipLaunchKernelGGL((c51_loss_kernel<decltype(a)::value, decltype(w)::value>), dim3((B + 3) / 4), dim3(256), 0, c.st, L);
        }
    }); });
    const C51GradArgs gA{B, FC, h->A, h->sup.N, h->off, h->c51_dl, h->c51_xs, h->c51_lt, h->dhf, p.a, p.G, p.loss, h->gmax, h->adam, p.tick};
    if (is_c51d(h)) hipLaunchKernelGGL(c51d_grad_kernel, dim3(FC / 16), dim3(256), 0, c.st, gA);      // (gA.off: W_v b_v W_a b_a)
    else hipLaunchKernelGGL(c51_grad_kernel, dim3(FC / 16), dim3(256), 0, c.st, gA);
}

// the fc1 backward.  Small scalar batches: head, loss and fc1's gradients in one launch (fc1_bwd2_kernel); else fc1's gradients from dhf
static void fc1_backward(fb_qnet *h, const Plan &p, const PlanCtx &c) {
    const int B = p.B, FC = h->FC;
    if (!c.big && !c.c51 && !c.ac) {
        const int ndx1 = ((B + 31) / 32) * 50;
        Bw1Args L;
        L.algo = p.algo; L.B = B; L.FC = FC; L.A = h->A; L.dueling = h->arch == FB_ARCH_DUELING; L.stot = c.stot; L.n_dx = ndx1; L.off = h->off;
        L.params = h->params[0]; L.pnext = p.sl.s[1].params; L.ptarget = p.ns > 2 ? p.sl.s[2].params : p.sl.s[1].params;
        L.hf = h->hf; L.qpart = h->qpart; L.h3 = h->h3; L.act = p.a; L.rew = p.r; L.term = p.t; L.isw = p.isw; L.gamma = p.gamma;
        L.grad = p.G; L.dh3 = h->dh3; L.loss = p.loss; L.abs_err = p.abs_err; L.y_out = p.y;
        L.adam = h->adam; L.tick = p.tick; L.rb = h->nsplit_train == 1;       // bf16 training: operands rounded to bf16
        L.gate = p.split && c.only < 0 ? FbGate{&p.split->f->trunk_done, p.split->seq, &p.split->f->timeouts[2]} : FbGate{nullptr, 0, nullptr};
        const dim3 grid(ndx1 + (FC / 32) * 7 + (L.gate.flag ? 1 : 0));
        const bool dp = p.algo == FB_ALGO_DOUBLE_PER, hu = h->huber > 0.f, md = is_mdqn_algo(p.algo);
        if (md) L.algo = p.algo == FB_ALGO_MDQN_PER ? FB_ALGO_PER : FB_ALGO_NATURE;      // (L.algo: the loss's form alone)
        if (dp) L.algo = FB_ALGO_PER;
        // (delta = 0 and an older algo: the kernels and arguments of before the options existed)
        if (dp || hu) fb_qnet_launch_fc1_bwd2_x(dp, hu, md, grid.x, c.st, &L, &h->md, h->huber);       // (the extended kernel: fb_qnet_x.hip's code object)
        else if (md) hipLaunchKernelGGL(fc1_bwd2_md_kernel, grid, dim3(512), 0, c.st, L, h->md);
        else hipLaunchKernelGGL(fc1_bwd2_kernel, grid, dim3(512), 0, c.st, L);
        return;
    }
    const int ndx = ((B + 31) / 32) * 50, ntile = ndx + 50 * (FC / 32);        // one workgroup per 32 x 32 tile, data-gradient tiles first
    const bool std_shape = FC == 512 && B == 256;      // the shapes this path sees (MAXTB = 256): fully unrolled instantiation
    with_nsp(h->nsplit_train, [&](auto ns) { with_bool(std_shape, [&](auto s) {
        hipLaunchKernelGGL((fc1_bwd_big_kernel<decltype(ns)::value, decltype(s)::value ? 4 : 0, decltype(s)::value ? 2 : 0>), dim3(ntile), dim3(512), 0, c.st,
                           ndx, h->params[0], h->h3, h->dhf, h->dh3, p.G, B, FC, (const float *)h->gmax, &h->adam->ovf);
    }); });
}

struct SlabCounts { int z1, z3; };           // slabs the conv backward left of conv1's / conv3's weight gradient (conv2's: as conv3's)
// the conv backward in its three shapes: conv_bw (small batches, one launch); conv_bx + conv_dw21; those two with conv_dwg between them
static SlabCounts conv_backward(fb_qnet *h, const Plan &p, const PlanCtx &c, int span0, int span1) {
    const int B = p.B, FC = h->FC, rbt = h->nsplit_train == 1;       // bf16 training: operands rounded to bf16
    // slabs: one chunk of <= 16 MFMAs (32 output pixels) per wave where the slab budget allows it
    int z3 = min((B * 25 + 255) / 256, h->zmax);
    const size_t ss = CONV_PARAMS;
    const AdamSpan span{master(h, 0), h->adam_m, h->adam_v, p.G, h->adam, span0, span1};
    // split schedule: the fc1 backward launch has waited for the acting trunk on the other stream (its gate workgroup), so W_fc1's Adam
    // span may ride in the launches below; the last of them waits for that stream's fc1 launch, so the Adam launch may follow
    const FbGate gate_fc1 = p.split && c.only < 0 ? FbGate{&p.split->f->fc1_done, p.split->seq, &p.split->f->timeouts[3]} : FbGate{nullptr, 0, nullptr};
    const FbSampleRider srider = p.sample_rider ? *p.sample_rider : FbSampleRider{};
    // [data-gradient chain per sample + conv3 dW + W_fc1's Adam] and [conv2 dW + conv1 dW] (see conv_bx_kernel)
    // conv1's weight gradient: two workgroups per sample, each with its own slab (2 B slabs); more than zmax of them are written
    // to the sub-slab buffer and folded into zmax slabs afterwards, in a fixed order
    const bool fold1 = 2 * B > h->zmax;
    const int fold = (2 * B + h->zmax - 1) / h->zmax;
    const int z1 = fold1 ? (2 * B + fold - 1) / fold : 2 * B;
    const int n_adam5 = (span1 - span0 + 511) / 512;
    const BxArgs bx{h->dh3, h->h2, h->p1, h->dh2, h->dp1, h->wsp[0] + wsp_w3t(FC), h->wsp[0] + wsp_w2t(FC)};
    const Dw1Ring dr{p.ring ? p.ring->c.bits : nullptr, h->ring_fo};
    float *s1 = fold1 ? h->slabs1 : h->slabs;
    const size_t st1 = fold1 ? (size_t)CONV1_PARAMS : ss;
    // large batches (multiples of 16): conv3's and conv2's weight gradients per group of 16 samples in a launch of their own
    // (conv_dwg_kernel) instead of as 38 + 34 tiles per slab inside the two launches below; one slab per group
    const bool dwg = c.big && B % 16 == 0;
    const int zt3 = dwg ? 0 : z3, zt2 = zt3;
    // small batches: the whole conv backward per sample in ONE launch (conv_bw_kernel); one conv2 / conv3 slab per sample
    const bool bw = !c.big && B <= h->zmax;
    // split schedule: W_fc1's Adam span rides in the next launch, and the acting trunk running beside this step on another stream
    // re-splits W_fc1's planes from those very parameters in its first microseconds
    if (bw) {
        z3 = B;
        const dim3 g(BW_WGS * B + n_adam5 + (srider.k ? 1 : 0) + (gate_fc1.flag ? 1 : 0));
        if (runs(c, K_CONV3_BWD)) with_nsp(h->nsplit_train, [&](auto ns) { with_bool(p.ring != nullptr, [&](auto r) {
            hipLaunchKernelGGL((conv_bw_kernel<decltype(ns)::value, decltype(r)::value>), g, dim3(512), 0, c.st,
                               bx, B, h->slabs, ss, s1, st1, p.s, (const uint8_t *)h->amax, dr, n_adam5, span, srider, rbt, gate_fc1);
        }); });
    } else {
        const dim3 g3(B + 38 * zt3 + n_adam5 + (srider.k ? 1 : 0)), g2(34 * zt2 + 2 * B + (gate_fc1.flag ? 1 : 0));
        if (runs(c, K_CONV3_BWD)) with_nsp(h->nsplit_train, [&](auto ns) {
            hipLaunchKernelGGL(conv_bx_kernel<decltype(ns)::value>, g3, dim3(512), 0, c.st, bx, B, zt3, h->slabs, ss, n_adam5, span, srider, rbt);
        });
        if (dwg) {
            z3 = B / 16;                                 // (conv2's slab count follows it)
            const int n3 = z3 * 4, n2 = z3 * 8;
            if (runs(c, K_CONV2_BWD)) with_nsp(h->nsplit_train, [&](auto ns) {
                hipLaunchKernelGGL(conv_dwg_kernel<decltype(ns)::value>, dim3(n3 + n2), dim3(512), 0, c.st, n3, h->h2, h->dh3, h->p1, h->dh2, h->slabs, ss, &h->adam->ovf);
            });
        }
        if (runs(c, K_CONV2_BWD)) with_bool(p.ring != nullptr, [&](auto r) {
            hipLaunchKernelGGL((conv_dw21_kernel<2, decltype(r)::value>), g2, dim3(512), 0, c.st,
                               zt2, B, h->p1, h->dh2, p.s, h->dp1, h->amax, h->slabs, ss, s1, st1, rbt, dr, gate_fc1);
        });
    }
    if (fold1 && runs(c, K_CONV2_BWD)) hipLaunchKernelGGL(slab_fold_kernel, dim3((CONV1_PARAMS + 255) / 256, z1), dim3(256), 0, c.st, h->slabs1, 2 * B, fold, h->slabs, ss);
    return SlabCounts{z1, z3};
}

// data-parallel path: the caller needs the complete flat gradient; fused path: Adam sums the slabs itself
static void reduce_or_adam(fb_qnet *h, const Plan &p, const PlanCtx &c, SlabCounts z, int span1) {
    if (p.split && c.only < 0) h->split_adam_pending = !p.apply_adam;
    if (!p.apply_adam && runs(c, K_SLAB)) hipLaunchKernelGGL(slab_reduce_kernel, dim3((CONV_PARAMS / 4 + 255) / 256), dim3(256), 0, c.st, h->slabs, (size_t)CONV_PARAMS, z.z1, z.z3, z.z3, p.G);
    if (c.only < 0) noisy_sgrad(h, p.G, c.st);   // (a noisy net: sigma's gradient, from the gradient of the effective W_fc1 b_fc1 and head)
    // split schedule: the Adam launch rewrites the conv planes / biases the acting trunk reads and the parameters its fc1 launch copies for the head
    if (p.apply_adam && runs(c, K_ADAM)) {
        AdamFused af;
        af.p = master(h, 0); af.m = h->adam_m; af.v = h->adam_v; af.g = p.G; af.n = h->ntot; af.ad = h->adam;
        af.slabs = h->slabs; af.slab_stride = CONV_PARAMS; af.z1 = z.z1; af.z2 = af.z3 = z.z3;
        af.w1s = h->w1s[0]; af.wsp = h->wsp[0]; af.FC = h->FC; af.tail0 = span1;
        const long long nrest4 = OFF_W2 / 4 + (OFF_W3 - OFF_B2) / 4 + (OFF_WF1 - OFF_B3) / 4 + (h->ntot / 4 - span1);
        af.lanes = 4;                                    // slab mode: one chunk of <= 16 slabs per lane
        af.split = p.split && c.only < 0 ? p.split->f : nullptr; af.split_val = p.split ? p.split->seq : 0;
        af.n_rest = (int)((nrest4 * af.lanes + 255) / 256);
        hipLaunchKernelGGL(adam_fused_kernel, dim3(ADAMF_T2 + ADAMF_T3 + af.n_rest), dim3(256), 0, c.st, af);
        noisy_materialise(h, 0, 0, false, c.st);
        c51d_fold(h, 0, c.st);
    }
}

static int run_plan(fb_qnet *h, const Plan &p, int only, hipStream_t st) {
    const PlanCtx c = plan_ctx(h, p, only, st);
    if (c.trunk && runs(c, K_CONV2)) ring_trunk(h, p, c);
    if (c.state_trunk) small_trunk(h, p, c, true);
    if (c.big) {
        for (int z = 0; z < p.ns;) {
            const int rc = large_pass(h, p, c, &z);
            if (rc != FB_OK) return rc;
        }
    } else small_forward(h, p, c);
    head_stage(h, p, c);
    if (p.train) {
        // exactly one of the launches that tick the Adam step counter -- the QR, C51 and scalar loss, fc1_bwd2_kernel -- is in a
        // plan when only < 0, and p.tick is false whenever only >= 0
        if (p.tick) h->adam_ticked = !p.apply_adam;              // stays pending until fb_qnet_apply_adam consumes it
        if ((c.c51 || c.ac || c.big) && runs(c, K_LOSS)) loss_stage(h, p, c);
        if (runs(c, K_FC1_BWD)) fc1_backward(h, p, c);
        // data-parallel path: from here on G[CONV_PARAMS ..) -- W_fc1, b_fc1, the head: 91 % of the bytes -- is final; the caller's side
        // stream can start reducing it while the conv backward below still runs (fb_qnet_set_grad_event)
        if (!p.apply_adam && only < 0) {
            h->grad_ev_recorded = nullptr;
            if (h->grad_ev) { FB_CHECK_HIP(hipEventRecord(h->grad_ev, st)); h->grad_ev_recorded = h->grad_ev; }
        }
        // fused single-GPU update: W_fc1's Adam rides in the conv backward launch below (AdamSpan), beside the conv data-gradient chain
        // (measured, profiles/r03_notes.md: splitting it between that launch and the conv weight gradients' costs the same ~3.5 us in all
        // -- the span is HBM traffic at ~6.5 TB/s and what it slows is the latency-bound chains beside it, wherever it rides); the
        // data-parallel path exports the gradient instead
        const int span0 = OFF_WF1 / 4, span1 = p.apply_adam ? (OFF_WF1 + 1600 * h->FC) / 4 : span0;
        reduce_or_adam(h, p, c, conv_backward(h, p, c, span0, span1), span1);
    }
    FB_LAUNCH_CHECK();
    return FB_OK;
}

static Plan forward_plan(fb_qnet *h, int which, const uint8_t *states, int n) {
    Plan p; memset(&p, 0, sizeof(p));
    p.sl.s[0] = Slice{h->params[which], states, 0, n, h->w1s[which], 0};
    p.ns = 1;
    return p;
}

static bool rows_ok(const fb_qnet *h, int n) { return n >= 1 && n <= 3 * h->max_batch; }      // the rows of a plan fit the workspace
static int copy_q(fb_qnet *h, int n, float *q, hipStream_t st) {      // the Q values of the n rows the last plan ran, to the caller (q may be NULL)
    if (q) FB_CHECK_HIP(hipMemcpyAsync(q, h->q, sizeof(float) * (size_t)n * h->A, hipMemcpyDeviceToDevice, st));
    return FB_OK;
}

extern "C" int fb_qnet_forward(fb_qnet_t h, int which, const uint8_t *states, int batch, float *q, void *stream) {
    FB_REQUIRE(h && states && q && (which == 0 || which == 1), "fb_qnet_forward: bad argument");
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward: batch %d exceeds 3*max_batch", batch);
    int rc = run_plan(h, forward_plan(h, which, states, batch), -1, fb_stream(stream));
    if (rc != FB_OK) return rc;
    return copy_q(h, batch, q, fb_stream(stream));
}

// fb_qnet_act / fb_qnet_act_nib behind their argument checks (nib: the states are the env's nibble state)
static int act_states(fb_qnet *h, const uint8_t *states, bool nib, int n, float epsilon, uint64_t seed, uint64_t step, uint8_t *actions, float *q,
                      hipStream_t st) {
    Plan p = forward_plan(h, 0, states, n);
    p.nib = nib;
    p.actions = actions; p.epsilon = epsilon; p.seed = seed; p.step = step;
    int rc = run_plan(h, p, -1, st);
    if (rc != FB_OK) return rc;
    return copy_q(h, n, q, st);
}

extern "C" int fb_qnet_act(fb_qnet_t h, const uint8_t *states, int n, float epsilon, uint64_t seed, uint64_t step,
                           uint8_t *actions, float *q, void *stream) {
    FB_REQUIRE(h && states && actions, "fb_qnet_act: NULL argument");
    FB_REQUIRE(rows_ok(h, n), "fb_qnet_act: n %d exceeds 3*max_batch", n);
    return act_states(h, states, false, n, epsilon, seed, step, actions, q, fb_stream(stream));
}

extern "C" int fb_qnet_act_nib(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                               uint8_t *actions, float *q, void *stream) {
    FB_REQUIRE(h && nib_states && actions, "fb_qnet_act_nib: NULL argument");
    FB_REQUIRE(rows_ok(h, n), "fb_qnet_act_nib: n %d exceeds 3*max_batch", n);
    return act_states(h, nib_states, true, n, epsilon, seed, step, actions, q, fb_stream(stream));
}

int fb_qnet_num_actions(fb_qnet_t h) { return h ? h->A : 0; }
const float *fb_qnet_acting_q(fb_qnet_t h) { return h ? h->q : nullptr; }      // f32[n][A] of the rows the last plan ran
int fb_qnet_is_c51(fb_qnet_t h) { return h && h->sup.N > 0 && !is_qr(h); }
int fb_qnet_is_qr(fb_qnet_t h) { return h && is_qr(h); }
int fb_qnet_is_dist(fb_qnet_t h) { return h && h->sup.N > 0; }
int fb_qnet_is_ac(fb_qnet_t h) { return h && is_ac(h); }
int fb_qnet_is_sac(fb_qnet_t h) { return h && is_sac(h); }
int fb_qnet_is_iqn(fb_qnet_t h) { return h && is_iqn(h); }
extern "C" int fb_qnet_is_noisy(fb_qnet_t h) { return h && h->noisy ? 1 : 0; }

extern "C" int fb_qnet_reset_noise(fb_qnet_t h, int which, uint64_t seed, uint64_t step, int mode, void *stream) {
    FB_REQUIRE(h && (which == 0 || which == 1), "fb_qnet_reset_noise: bad argument");
    FB_REQUIRE(h->noisy, "fb_qnet_reset_noise: not a noisy net (fb_qnet_create_c51_noisy)");
    FB_REQUIRE(mode == FB_NOISE_SAMPLE || mode == FB_NOISE_MEAN, "fb_qnet_reset_noise: mode must be FB_NOISE_SAMPLE or FB_NOISE_MEAN (got %d)", mode);
    hipStream_t st = fb_stream(stream);
    hipLaunchKernelGGL(noise_draw_kernel, dim3((h->nnet.nz + 255) / 256), dim3(256), 0, st, h->nz[which], h->nnet.nz, (uint32_t)seed, (uint32_t)(seed >> 32),
                       (uint32_t)step, (uint32_t)(step >> 32) * 2u + (uint32_t)which, mode == FB_NOISE_MEAN ? 1 : 0);
    noisy_materialise(h, which, OFF_WF1, true, st);      // (the trunk is mu: unchanged)
    c51d_fold(h, which, st);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_get_noise(fb_qnet_t h, int which, float *out) {
    FB_REQUIRE(h && out && (which == 0 || which == 1), "fb_qnet_get_noise: bad argument");
    FB_REQUIRE(h->noisy, "fb_qnet_get_noise: not a noisy net (fb_qnet_create_c51_noisy)");
    FB_CHECK_HIP(hipDeviceSynchronize());
    FB_CHECK_HIP(hipMemcpy(out, h->nz[which], sizeof(float) * (size_t)h->nnet.nz, hipMemcpyDefault));
    return FB_OK;
}

extern "C" int fb_qnet_set_acting_noise(fb_qnet_t h, int mode) {
    FB_REQUIRE(h, "fb_qnet_set_acting_noise: NULL handle");
    FB_REQUIRE(h->noisy, "fb_qnet_set_acting_noise: not a noisy net (fb_qnet_create_c51_noisy)");
    FB_REQUIRE(mode == FB_ACT_NOISE_SHARED || mode == FB_ACT_NOISE_PER_ENV,
               "fb_qnet_set_acting_noise: mode must be FB_ACT_NOISE_SHARED or FB_ACT_NOISE_PER_ENV (got %d)", mode);
    h->act_noise = mode;
    return FB_OK;
}
int fb_qnet_acting_noise(fb_qnet_t h) { return h && h->noisy ? h->act_noise : FB_ACT_NOISE_SHARED; }

int fb_qnet_check_env_noise(fb_qnet_t h, int n, const char *who) {
    FB_REQUIRE(h, "%s: NULL handle", who);
    FB_REQUIRE(h->noisy, "%s: per-env acting noise needs a noisy net (fb_qnet_create_c51_noisy)", who);
    FB_REQUIRE(h->nsplit == 3, "%s: per-env acting noise takes FB_DTYPE_F32 inference only (the net is set to FB_DTYPE_BF16)", who);
    FB_REQUIRE(rows_ok(h, n), "%s: n %d exceeds 3*max_batch", who, n);
    FB_REQUIRE((unsigned long long)n * (unsigned long long)h->nnet.nz < (1ull << 32), "%s: n * nz = %d * %d must stay below 2^32 (the noise counter)",
               who, n, h->nnet.nz);
    return FB_OK;
}

// the fc1 stage of the per-env acting forward (include/fbdqn.h), shared by the C51 and the IQN path: mu into params[0] (zero noise) and
// its fold, the acting forward's conv1 .. fc1 on it, then the noise: sigma_W_fc1's planes (when sigma moved), the scaled activations'
// planes, sigma's fc1 GEMM (fc1_sp_kernel, unchanged).  *o: where the head that follows finds the two sets of fc1 partial sums
int fb_qnet_env_noise_fc1(fb_qnet_t h, const uint8_t *nib_states, int n, uint64_t seed, uint64_t step, FbEnvNoiseFc1 *o, void *stream) {
    hipStream_t st = fb_stream(stream);
    const NoisyMat mu{h->mst[0], h->params[0], h->nz_zero, h->nnet, OFF_WF1, 0, h->adam, h->noisy_end};
    hipLaunchKernelGGL(noisy_mat_kernel, dim3((unsigned)((h->n - OFF_WF1 + 255) / 256)), dim3(256), 0, st, mu);
    c51d_fold(h, 0, st);
    Plan p = forward_plan(h, 0, nib_states, n);
    p.nib = true; p.no_head = true;
    const int rc = run_plan(h, p, -1, st);
    if (rc != FB_OK) return rc;
    const bool sp = n >= 256;                    // (run_plan's: the fused two-plane trunk + fc1_sp_kernel, else the small-batch kernels)
    const int FC = h->FC, stot = 3 * h->max_batch;
    const size_t pl2 = (size_t)stot * 1600;
    const float *sig = h->mst[0] + h->n - OFF_WF1;      // (sigma of mu entry q at sig[q])
    hipLaunchKernelGGL(env_noise_sigsplit_kernel, dim3((unsigned)((200 * FC + 255) / 256)), dim3(256), 0, st, sig, h->wsig, FC, (const AdamDev *)h->adam,
                       (const int *)h->sig_seen);
    EnvScale es{sp ? h->a3s : nullptr, sp ? nullptr : h->h3, pl2, h->a3n, n, h->nnet.nz, 0, 0, 0, 0, h->adam, h->sig_seen, &h->adam->ovf};
    put_seed_words(es, seed, step);
    hipLaunchKernelGGL(env_noise_scale_kernel, dim3((unsigned)(((long long)n * 800 + 255) / 256)), dim3(256), 0, st, es);
    const Fc1Args af{h->a3n, pl2, h->zeros, h->wsig + WSP_WF1, h->ht, stot, n, FC, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0};
    hipLaunchKernelGGL(fc1_sp_kernel<3>, dim3(((n + 127) / 128) * (FC / 64) * FC1_SP_KS), dim3(256), 0, st, af);
    o->hf = sp ? h->hf_act : h->hf; o->ht = h->ht; o->stot = stot; o->nks = sp ? FC1_SP_KS : 1; o->nkt = FC1_SP_KS; o->sig = sig;
    return FB_OK;
}

// the per-env acting forward: the fc1 stage above, then the per-env noisy head -- a C51 net's (env_noise_head_kernel) or an IQN net's
// (fb_iqn.hip).  restore: rebuild params[0] (and the folded head) from the net's own sample -- the same launches that built them
static int act_env_noise(fb_qnet *h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step, uint8_t *actions, float *q,
                         bool restore, hipStream_t st) {
    FB_REQUIRE(h && nib_states && actions, "fb_qnet_act_nib_env_noise: NULL argument");
    int rc = fb_qnet_check_env_noise(h, n, "fb_qnet_act_nib_env_noise");
    if (rc != FB_OK) return rc;
    FbEnvNoiseFc1 f1;
    rc = fb_qnet_env_noise_fc1(h, nib_states, n, seed, step, &f1, st);
    if (rc != FB_OK) return rc;
    const int FC = h->FC;
    if (is_iqn(h)) {
        IqnEnvNoiseArgs H;
        memset(&H, 0, sizeof(H));
        H.hf = f1.hf; H.ht = f1.ht; H.stot = f1.stot; H.nks = f1.nks; H.nkt = f1.nkt; H.sig = f1.sig;
        H.F = head_base(h, h->params[0]); H.foff = h->hoff; H.off = h->off; H.pbar = h->iqn_pbar[0];
        H.n = n; H.FC = FC; H.A = h->A; H.nz = h->nnet.nz; H.dueling = is_iqnd(h) ? 1 : 0;
        const NoisyLayer LV = h->nnet.l[1], LQ = h->nnet.l[h->nnet.nl - 1];
        H.e_fc1_out = h->nnet.l[0].eout; H.e_v_in = LV.ein; H.e_v_out = LV.eout; H.e_q_in = LQ.ein; H.e_q_out = LQ.eout;
        H.q = h->q; H.actions = actions; H.epsilon = epsilon;
        put_seed_words(H, seed, step); H.key_of = nullptr; H.stream = FB_STREAM_EPS;
        fb_iqn_launch_env_noise_head(st, H);
    } else {
        EnvNoiseHead H;
        H.hf = f1.hf; H.ht = f1.ht; H.stot = f1.stot; H.nks = f1.nks;
        H.P = head_base(h, h->params[0]); H.hoff = h->hoff; H.sig = f1.sig; H.off = h->off; H.N = h->nnet;
        H.n = n; H.FC = FC; H.A = h->A; H.sup = h->sup; H.q = h->q; H.actions = actions; H.epsilon = epsilon;
        put_seed_words(H, seed, step); H.key_of = nullptr; H.stream = FB_STREAM_EPS;
        with_actions(h->A, [&](auto a) { with_bool(is_c51d(h), [&](auto d) {
            hipLaunchKernelGGL((env_noise_head_kernel<decltype(a)::value, decltype(d)::value>), dim3((n + ENH_WAVES - 1) / ENH_WAVES), dim3(64 * ENH_WAVES), 0, st, H);
        }); });
    }
    if (restore) {
        noisy_materialise(h, 0, OFF_WF1, true, st);
        c51d_fold(h, 0, st);
    }
    FB_LAUNCH_CHECK();
    return copy_q(h, n, q, st);
}

extern "C" int fb_qnet_act_nib_env_noise(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                                         uint8_t *actions, float *q, void *stream) {
    return act_env_noise(h, nib_states, n, epsilon, seed, step, actions, q, true, fb_stream(stream));
}
int fb_qnet_act_nib_env_noise_keep(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                                   uint8_t *actions, float *q, void *stream) {
    return act_env_noise(h, nib_states, n, epsilon, seed, step, actions, q, false, fb_stream(stream));
}

extern "C" int fb_qnet_get_support(fb_qnet_t h, int *n_atoms_host, float *v_min_host, float *v_max_host) {
    FB_REQUIRE(h && n_atoms_host && v_min_host && v_max_host, "fb_qnet_get_support: NULL argument");
    *n_atoms_host = is_qr(h) ? 0 : h->sup.N; *v_min_host = h->sup.vmin; *v_max_host = h->sup.vmax;      // (a QR net: no support)
    return FB_OK;
}

extern "C" int fb_qnet_set_munchausen(fb_qnet_t h, float tau, float alpha, float clip_lo) {
    FB_REQUIRE(h, "fb_qnet_set_munchausen: NULL handle");
    FB_REQUIRE(h->sup.N == 0, "fb_qnet_set_munchausen: Munchausen-DQN trains the scalar heads only, not a C51 / QR net");
    FB_REQUIRE(!is_ac(h), "fb_qnet_set_munchausen: Munchausen-DQN trains the scalar Q heads only, not an actor-critic net");
    FB_REQUIRE(!is_sac(h), "fb_qnet_set_munchausen: Munchausen-DQN trains the scalar Q heads only, not a SAC net");
    FB_REQUIRE(!is_iqn(h), "fb_qnet_set_munchausen: Munchausen-DQN trains the scalar Q heads only, not an IQN net (its loss has its own kappa)");
    FB_REQUIRE(isfinite(tau) && tau > 0.f, "fb_qnet_set_munchausen: tau must be finite and > 0 (got %g)", (double)tau);
    FB_REQUIRE(alpha >= 0.f && alpha <= 1.f, "fb_qnet_set_munchausen: alpha must be in [0, 1] (got %g)", (double)alpha);
    FB_REQUIRE(isfinite(clip_lo) && clip_lo <= 0.f, "fb_qnet_set_munchausen: the clip l0 must be finite and <= 0 (got %g)", (double)clip_lo);
    h->md = MdPar{tau, alpha, clip_lo};
    return FB_OK;
}

extern "C" int fb_qnet_get_munchausen(fb_qnet_t h, float *tau_host, float *alpha_host, float *clip_lo_host) {
    FB_REQUIRE(h, "fb_qnet_get_munchausen: NULL handle");
    FB_REQUIRE(h->sup.N == 0, "fb_qnet_get_munchausen: Munchausen-DQN trains the scalar heads only, not a C51 / QR net");
    FB_REQUIRE(!is_ac(h), "fb_qnet_get_munchausen: Munchausen-DQN trains the scalar Q heads only, not an actor-critic net");
    FB_REQUIRE(!is_sac(h), "fb_qnet_get_munchausen: Munchausen-DQN trains the scalar Q heads only, not a SAC net");
    FB_REQUIRE(!is_iqn(h), "fb_qnet_get_munchausen: Munchausen-DQN trains the scalar Q heads only, not an IQN net (its loss has its own kappa)");
    if (tau_host) *tau_host = h->md.tau;
    if (alpha_host) *alpha_host = h->md.alpha;
    if (clip_lo_host) *clip_lo_host = h->md.clip;
    return FB_OK;
}

extern "C" int fb_qnet_set_huber(fb_qnet_t h, float delta) {
    FB_REQUIRE(h, "fb_qnet_set_huber: NULL handle");
    FB_REQUIRE(h->sup.N == 0, "fb_qnet_set_huber: the Huber loss is a setting of the scalar heads only, not of a C51 / QR / noisy net (QR has its own kappa)");
    FB_REQUIRE(!is_ac(h), "fb_qnet_set_huber: the Huber loss is a setting of the scalar Q heads only, not of an actor-critic net");
    FB_REQUIRE(!is_sac(h), "fb_qnet_set_huber: the Huber loss is a setting of the scalar Q heads only, not of a SAC net");
    FB_REQUIRE(!is_iqn(h), "fb_qnet_set_huber: the Huber loss is a setting of the scalar Q heads only, not of an IQN net (its loss has its own kappa)");
    FB_REQUIRE(isfinite(delta) && delta >= 0.f, "fb_qnet_set_huber: delta must be finite and >= 0 (0 = the squared loss; got %g)", (double)delta);
    h->huber = delta;
    return FB_OK;
}

extern "C" int fb_qnet_get_huber(fb_qnet_t h, float *delta_host) {
    FB_REQUIRE(h && delta_host, "fb_qnet_get_huber: NULL argument");
    FB_REQUIRE(h->sup.N == 0, "fb_qnet_get_huber: the Huber loss is a setting of the scalar heads only, not of a C51 / QR / noisy net (QR has its own kappa)");
    FB_REQUIRE(!is_ac(h), "fb_qnet_get_huber: the Huber loss is a setting of the scalar Q heads only, not of an actor-critic net");
    FB_REQUIRE(!is_sac(h), "fb_qnet_get_huber: the Huber loss is a setting of the scalar Q heads only, not of a SAC net");
    FB_REQUIRE(!is_iqn(h), "fb_qnet_get_huber: the Huber loss is a setting of the scalar Q heads only, not of an IQN net (its loss has its own kappa)");
    *delta_host = h->huber;
    return FB_OK;
}

extern "C" int fb_qnet_get_quantiles(fb_qnet_t h, int *n_quantiles_host, float *kappa_host) {
    FB_REQUIRE(h && n_quantiles_host && kappa_host, "fb_qnet_get_quantiles: NULL argument");
    *n_quantiles_host = is_qr(h) ? h->sup.N : 0; *kappa_host = is_qr(h) ? h->kappa : 0.f;
    return FB_OK;
}

extern "C" int fb_qnet_forward_quantiles(fb_qnet_t h, int which, const uint8_t *states, int batch, float *theta, void *stream) {
    FB_REQUIRE(h && states && theta && (which == 0 || which == 1), "fb_qnet_forward_quantiles: bad argument");
    FB_REQUIRE(is_qr(h), "fb_qnet_forward_quantiles: not a QR net (fb_qnet_create_qr)");
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward_quantiles: batch %d exceeds 3*max_batch", batch);
    Plan p = forward_plan(h, which, states, batch);
    p.probs = theta;                             // (the QR head writes theta there)
    return run_plan(h, p, -1, fb_stream(stream));
}

extern "C" int fb_qnet_forward_dist(fb_qnet_t h, int which, const uint8_t *states, int batch, float *probs, void *stream) {
    FB_REQUIRE(h && states && probs && (which == 0 || which == 1), "fb_qnet_forward_dist: bad argument");
    FB_REQUIRE(h->sup.N > 0 && !is_qr(h), "fb_qnet_forward_dist: not a C51 net (fb_qnet_create_c51; a QR net: fb_qnet_forward_quantiles)");
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward_dist: batch %d exceeds 3*max_batch", batch);
    Plan p = forward_plan(h, which, states, batch);
    p.probs = probs;
    return run_plan(h, p, -1, fb_stream(stream));
}

// fb_eval_run on a C51 net: the head fb_qnet_eval_trunk described (hd->c.hf / stot / nks, hd->params), with the caller's q / actions /
// epsilon / seeds in hd->c, keyed by key_of[row] on FB_STREAM_EVAL -- as the env launch's head rider keys a scalar net's draws
int fb_qnet_c51_eval_head(fb_qnet_t h, const FbHeadRider *hd, int n, const int32_t *key_of, void *stream) {
    FB_REQUIRE(h && hd && key_of && h->sup.N > 0, "fb_qnet_c51_eval_head: bad argument");
    C51HeadArgs H;
    memset(&H, 0, sizeof(H));
    H.sl.s[0] = Slice{hd->params, nullptr, 0, n, nullptr, 0}; H.nslices = 1; H.params = hd->params;
    C51Core &C = H.c;
    C.hf = hd->c.hf; C.stot = hd->c.stot; C.nks = hd->c.nks; C.q = hd->c.q; C.probs = nullptr; C.FC = h->FC; C.A = h->A;
    C.off = h->hoff; C.sup = h->sup; C.actions = hd->c.actions; C.epsilon = hd->c.epsilon;
    C.seed_lo = hd->c.seed_lo; C.seed_hi = hd->c.seed_hi; C.step_lo = hd->c.step_lo; C.step_hi = hd->c.step_hi;
    C.key_of = key_of; C.stream = FB_STREAM_EVAL;
    launch_dist_head(h, H, n, fb_stream(stream));
    FB_LAUNCH_CHECK();
    return FB_OK;
}
int fb_qnet_max_rows(fb_qnet_t h) { return h ? 3 * h->max_batch : 0; }
hipStream_t fb_qnet_side_stream(fb_qnet_t h) { return h && h->split ? h->split->tstream : nullptr; }

int fb_qnet_eval_trunk(fb_qnet_t h, const uint8_t *nib_states, int n, FbHeadRider *head, void *stream) {
    FB_REQUIRE(h && nib_states && head, "fb_qnet_eval_trunk: NULL argument");
    FB_REQUIRE(rows_ok(h, n), "fb_qnet_eval_trunk: n %d exceeds 3*max_batch", n);
    Plan p = forward_plan(h, 0, nib_states, n);
    p.nib = true; p.any_rows = true;
    p.head_rider = head;
    return run_plan(h, p, -1, fb_stream(stream));
}

extern "C" int fb_eval_q(fb_qnet_t h, const uint8_t *nib_states, int n, float *q, void *stream) {
    FB_REQUIRE(h && nib_states && q, "fb_eval_q: NULL argument");
    FB_REQUIRE(rows_ok(h, n), "fb_eval_q: n %d exceeds 3*max_batch", n);
    Plan p = forward_plan(h, 0, nib_states, n);
    p.nib = true; p.any_rows = true;
    int rc = run_plan(h, p, -1, fb_stream(stream));
    if (rc != FB_OK) return rc;
    return copy_q(h, n, q, fb_stream(stream));
}

int fb_qnet_check_step(fb_qnet_t h, int n_envs, int train_batch) {
    FB_REQUIRE(h, "fb_vec_step: NULL net");
    FB_REQUIRE(n_envs >= 1 && n_envs <= 3 * h->max_batch, "fb_vec_step: %d envs exceed 3*max_batch of the net", n_envs);
    FB_REQUIRE(train_batch < 0 || (train_batch >= 1 && train_batch <= h->max_batch && train_batch <= MAXTB),
               "fb_vec_step: batch %d exceeds min(max_batch, %d)", train_batch, MAXTB);
    return FB_OK;
}

int fb_qnet_act_nib_rider(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t *actions, FbHeadRider *head, void *stream, const FbSplitCtx *split) {
    FB_REQUIRE(h && nib_states && actions && head, "fb_qnet_act_nib_rider: NULL argument");
    FB_REQUIRE(h->sup.N == 0, "fb_qnet_act_nib_rider: a C51 or QR net's head does not ride in the env launch");
    FB_REQUIRE(rows_ok(h, n), "fb_qnet_act_nib: n %d exceeds 3*max_batch", n);
    Plan p = forward_plan(h, 0, nib_states, n);
    p.nib = true;
    p.actions = actions; p.epsilon = epsilon; p.seed = seed; p.step = step;
    p.head_rider = head;
    p.split = split;
    return run_plan(h, p, -1, fb_stream(stream));
}

extern "C" int fb_qnet_apply_adam(fb_qnet_t h, const float *flat_grad, void *stream) {
    FB_REQUIRE(h && flat_grad, "fb_qnet_apply_adam: NULL argument");
    hipStream_t st = fb_stream(stream);
    // gradients that did not come from fb_qnet_train_step need their own tick.  The kernel checks on the device whether one is
    // pending; the host-side hint only saves the launch in eager mode (under stream capture the hint describes capture time, not
    // replay time, so the guarded kernel always goes in)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(st, &cap);
    if (!h->adam_ticked || cap != hipStreamCaptureStatusNone) hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(1), 0, st, h->adam);
    h->adam_ticked = false;
    AdamFused af;
    af.p = master(h, 0); af.m = h->adam_m; af.v = h->adam_v; af.g = flat_grad; af.n = h->ntot; af.ad = h->adam;
    af.slabs = nullptr; af.slab_stride = 0; af.z1 = af.z2 = af.z3 = 0;
    af.w1s = h->w1s[0]; af.wsp = h->wsp[0]; af.FC = h->FC; af.tail0 = OFF_WF1 / 4;
    af.n_rest = ADAM_GRID; af.lanes = 1;
    // (the update that completes a split step: its stores wait for that step's acting forward, and it does not retire before that step's env launch)
    af.split = h->split_adam_pending && h->split && h->split->tstream ? h->split->f : nullptr; af.split_val = af.split ? h->split->seq : 0;
    h->split_adam_pending = false;
    hipLaunchKernelGGL(adam_fused_kernel, dim3(ADAMF_T2 + ADAMF_T3 + af.n_rest), dim3(256), 0, st, af);
    noisy_materialise(h, 0, 0, false, st);
    c51d_fold(h, 0, st);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_set_grad_event(fb_qnet_t h, void *event) {
    FB_REQUIRE(h, "fb_qnet_set_grad_event: NULL handle");
    h->grad_ev = (hipEvent_t)event;
    return FB_OK;
}

void *fb_qnet_get_grad_event(fb_qnet_t h) { return h ? (void *)h->grad_ev : nullptr; }
void *fb_qnet_take_grad_event_recorded(fb_qnet_t h) {
    if (!h) return nullptr;
    void *e = (void *)h->grad_ev_recorded;
    h->grad_ev_recorded = nullptr;
    return e;
}

extern "C" int64_t fb_qnet_grad_split(fb_qnet_t h) { return h ? (int64_t)CONV_PARAMS : 0; }

extern "C" int fb_qnet_sync_target(fb_qnet_t h, void *stream) {
    FB_REQUIRE(h, "fb_qnet_sync_target: NULL handle");
    FB_CHECK_HIP(hipMemcpyAsync(master(h, 1), master(h, 0), sizeof(float) * (size_t)h->ntot, hipMemcpyDeviceToDevice, fb_stream(stream)));
    FB_CHECK_HIP(hipMemcpyAsync(h->w1s[1], h->w1s[0], 3 * 8192 * 2, hipMemcpyDeviceToDevice, fb_stream(stream)));
    hipLaunchKernelGGL(bump_pver_kernel, dim3(1), dim3(1), 0, fb_stream(stream), h->adam, 1);
    noisy_materialise(h, 1, 0, false, fb_stream(stream));      // (with the target net's own noise)
    resplit_now(h, 1, fb_stream(stream));
    c51d_fold(h, 1, fb_stream(stream));
    FB_LAUNCH_CHECK();
    return FB_OK;
}

// target <- target + rho (online - target) over the master vector; then everything derived from the target's parameters is rebuilt from
// the new values, in fb_qnet_load_params' order (W_conv1's planes through w1_split_kernel, which also makes the new parameter version)
extern "C" int fb_qnet_soft_sync_target(fb_qnet_t h, float rho, void *stream) {
    FB_REQUIRE(h, "fb_qnet_soft_sync_target: NULL handle");
    FB_REQUIRE(rho > 0.f && rho <= 1.f, "fb_qnet_soft_sync_target: rho must be in (0, 1] (got %g)", (double)rho);
    if (rho == 1.f) return fb_qnet_sync_target(h, stream);
    hipStream_t st = fb_stream(stream);
    fb_qnet_launch_target_lerp_x(st, master(h, 1), master(h, 0), h->ntot, rho);
    noisy_materialise(h, 1, 0, false, st);       // (with the target net's own noise)
    hipLaunchKernelGGL(w1_split_kernel, dim3(32), dim3(256), 0, st, h->params[1], h->w1s[1], &h->adam->pver[1]);
    c51d_fold(h, 1, st);
    resplit_now(h, 1, st);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_set_max_grad_norm(fb_qnet_t h, float g) {
    FB_REQUIRE(h, "fb_qnet_set_max_grad_norm: NULL handle");
    FB_REQUIRE(isfinite(g) && g >= 0.f, "fb_qnet_set_max_grad_norm: the norm limit must be finite and >= 0 (0 = no clipping; got %g)", (double)g);
    h->max_grad_norm = g;
    return FB_OK;
}

extern "C" int fb_qnet_get_max_grad_norm(fb_qnet_t h, float *g_host) {
    FB_REQUIRE(h && g_host, "fb_qnet_get_max_grad_norm: NULL argument");
    *g_host = h->max_grad_norm;
    return FB_OK;
}

float fb_qnet_max_grad_norm(fb_qnet_t h) { return h ? h->max_grad_norm : 0.f; }

extern "C" int fb_qnet_clip_grad(fb_qnet_t h, float *flat_grad, void *stream) {
    FB_REQUIRE(h && flat_grad, "fb_qnet_clip_grad: NULL argument");
    FB_REQUIRE(((uintptr_t)flat_grad & 15) == 0, "fb_qnet_clip_grad: flat_grad must be 16-byte aligned");
    fb_qnet_launch_clip_x(fb_stream(stream), flat_grad, h->ntot, h->clip_part, h->max_grad_norm, h->clip_out);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

extern "C" int fb_qnet_grad_norm(fb_qnet_t h, float *norm_host, float *scale_host) {
    FB_REQUIRE(h, "fb_qnet_grad_norm: NULL handle");
    FB_CHECK_HIP(hipDeviceSynchronize());
    float v[2] = {0.f, 1.f};
    FB_CHECK_HIP(hipMemcpy(v, h->clip_out, sizeof(v), hipMemcpyDeviceToHost));
    if (norm_host) *norm_host = v[0];
    if (scale_host) *scale_host = v[1];
    return FB_OK;
}

// a whole train step.  A net with a norm limit whose caller exports nothing: the exporting step into the net's own gradient buffer, the
// clip, then fb_qnet_apply_adam's launch -- those three public calls, so their results bit for bit (loss, abs_err, q_target: the step's)
static int run_train(fb_qnet *h, Plan &p, void *stream) {
    if (!(p.apply_adam && h->max_grad_norm > 0.f)) return run_plan(h, p, -1, fb_stream(stream));
    p.apply_adam = false;                        // (p.G is h->grad already)
    const hipEvent_t ev = h->grad_ev;            // (nobody reduces this export: no event)
    h->grad_ev = nullptr;
    int rc = run_plan(h, p, -1, fb_stream(stream));
    h->grad_ev = ev;
    if (rc == FB_OK) rc = fb_qnet_clip_grad(h, h->grad, stream);
    if (rc == FB_OK) rc = fb_qnet_apply_adam(h, h->grad, stream);
    return rc;
}

// a train step on gathered states: only a batch of >= 256 reads W_fc1's planes (fc1_sp_kernel), which Adam leaves stale (fb_ring_src_fresh's
// rule for the ring-fed calls)
static int run_train_gathered(fb_qnet *h, Plan &p, int B, void *stream) {
    const int rc = B >= 256 ? fb_qnet_refresh_planes(h, stream) : FB_OK;
    return rc != FB_OK ? rc : run_train(h, p, stream);
}

// what every train plan ends with: where the gradient goes and who applies Adam, the ring, and its n-step view (s' = frames tt + n - 3 .. tt + n)
static void plan_train_tail(fb_qnet *h, Plan &p, float *flat_grad, const FbRingSrc *ring) {
    p.G = flat_grad ? flat_grad : h->grad;
    p.apply_adam = flat_grad == nullptr; p.tick = true;
    p.ring = ring;
    if (ring && ring->c.nstep > 1)
        for (int z = 0; z < p.ns; z++) if (p.sl.s[z].fshift) p.sl.s[z].fshift = ring->c.nstep;
}

// the two checks the training calls of every family share, `who` in the message
static int check_batch(fb_qnet *h, int B, const char *who) {
    FB_REQUIRE(B >= 1 && B <= h->max_batch && B <= MAXTB, "%s: batch %d exceeds min(max_batch, %d)", who, B, MAXTB);
    return FB_OK;
}
static int check_gamma01(double gamma, const char *who) {
    FB_REQUIRE(isfinite(gamma) && gamma >= 0.0 && gamma <= 1.0, "%s: gamma must be in [0, 1] (got %g)", who, gamma);
    return FB_OK;
}

static int train_plan(fb_qnet *h, int algo, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                      const uint8_t *t, const float *isw, double gamma, float *loss, float *abs_err, float *q_target,
                      float *flat_grad, Plan *out, const FbRingSrc *ring = nullptr) {
    FB_REQUIRE(h && a && r && t && loss && (ring || (s && s2)), "fb_qnet_train_step: NULL argument");
    FB_REQUIRE((algo >= 0 && algo <= FB_ALGO_QR_DOUBLE_PER) || is_mdqn_algo(algo) || algo == FB_ALGO_DOUBLE_PER, "fb_qnet_train_step: unknown algo %d", algo);
    FB_REQUIRE(!is_ac(h), "fb_qnet_train_step: an actor-critic net trains through fb_qnet_ac_train_step / fb_ac_train_from_replay only (got algo %d)", algo);
    FB_REQUIRE(!is_sac(h), "fb_qnet_train_step: a SAC net trains through fb_qnet_sac_train_step / fb_sac_train_from_replay only (got algo %d)", algo);
    FB_REQUIRE(!is_iqn(h), "fb_qnet_train_step: an IQN net trains through fb_qnet_iqn_train_step / fb_iqn_train_from_replay only (got algo %d)", algo);
    {
        const bool c51a = is_c51_algo(algo), qra = is_qr_algo(algo);
        FB_REQUIRE(c51a == (h->sup.N > 0 && !is_qr(h)), c51a ? "fb_qnet_train_step: algo %d (C51) needs a C51 net (fb_qnet_create_c51)"
                                                : "fb_qnet_train_step: a C51 net trains with FB_ALGO_C51, FB_ALGO_C51_PER, FB_ALGO_C51_DOUBLE_PER "
                                                  "or FB_ALGO_C51_DOUBLE only (got algo %d)", algo);
        FB_REQUIRE(qra == is_qr(h), qra ? "fb_qnet_train_step: algo %d (QR) needs a QR net (fb_qnet_create_qr)"
                                        : "fb_qnet_train_step: a QR net trains with FB_ALGO_QR, FB_ALGO_QR_DOUBLE, FB_ALGO_QR_PER or "
                                          "FB_ALGO_QR_DOUBLE_PER only (got algo %d)", algo);
    }
    if (const int rb = check_batch(h, B, "fb_qnet_train_step")) return rb;
    FB_REQUIRE(algo != FB_ALGO_PG || (B <= 128 && !ring && gamma >= (double)B), "fb_qnet_train_step: FB_ALGO_PG takes chunks of <= 128 gathered states and gamma = the whole batch's sample count (>= %d)", B);
    FB_REQUIRE(!is_per_algo(algo) || isw, "fb_qnet_train_step: PER needs isw (algo %d)", algo);
    FB_REQUIRE(algo != FB_ALGO_PG || !(h->huber > 0.f), "fb_qnet_train_step: FB_ALGO_PG has no TD error to clip: the net's Huber delta is %g, set it to 0 (fb_qnet_set_huber)", (double)h->huber);
    Plan p; memset(&p, 0, sizeof(p));
    // forward: s through the online net, s' through the net(s) the algorithm asks for
    p.ns = 2;
    p.sl.s[0] = Slice{h->params[0], s, 0, B, h->w1s[0], 0};
    if (algo == FB_ALGO_DQN || algo == FB_ALGO_PG) p.sl.s[1] = Slice{h->params[0], s2, B, B, h->w1s[0], 1};               // BrainDQN.py:205 (same net); PG: s2 is forwarded and ignored
    else if (algo == FB_ALGO_DOUBLE || algo == FB_ALGO_DOUBLE_PER || is_double_c51(algo) || is_double_qr(algo)) { p.sl.s[1] = Slice{h->params[0], s2, B, B, h->w1s[0], 1}; p.sl.s[2] = Slice{h->params[1], s2, 2 * B, B, h->w1s[1], 1}; p.ns = 3; }
    else p.sl.s[1] = Slice{h->params[1], s2, B, B, h->w1s[1], 1};                                // target net (Nature, PER, C51, C51_PER, Munchausen)
    if (is_mdqn_algo(algo)) { p.sl.s[2] = Slice{h->params[1], s, 2 * B, B, h->w1s[1], 0}; p.ns = 3; }     // Munchausen: s through the target net as well (the log-policy bonus)
    p.sl.rb = h->nsplit_train == 1;
    p.train = true; p.algo = algo; p.B = B; p.s = s; p.a = a; p.r = r; p.t = t; p.isw = isw; p.gamma = gamma;
    p.loss = loss; p.abs_err = abs_err; p.y = q_target;
    plan_train_tail(h, p, flat_grad, ring);
    *out = p;
    return FB_OK;
}

int fb_qnet_train_step_ring(fb_qnet_t h, int algo, int B, const FbRingSrc *ring, const float *isw, double gamma, float *loss, float *abs_err,
                            float *flat_grad, void *stream, const FbSampleRider *rider, const FbSplitCtx *split) {
    FB_REQUIRE(h && ring && ring->idx && ring->a && ring->r && ring->t, "fb_qnet_train_step_ring: NULL argument");
    Plan p;
    int rc = train_plan(h, algo, B, nullptr, ring->a, ring->r, nullptr, ring->t, isw, gamma, loss, abs_err, nullptr, flat_grad, &p, ring);
    if (rc != FB_OK) return rc;
    p.sample_rider = rider;
    p.split = split;
    return run_train(h, p, stream);
}

// both nets in one launch (blockIdx.y = net; every thread checks its net's versions) + one marking launch
__global__ void wsplit_both_kernel(const float *__restrict__ p0, const float *__restrict__ p1, uint4 *__restrict__ w0, uint4 *__restrict__ w1, int FC,
                                   const AdamDev *__restrict__ ad) {
    const int n = blockIdx.y;
    if (ad->pver[n] == ad->wver[n]) return;
    wsplit_item(n ? p1 : p0, n ? w1 : w0, FC, blockIdx.x * blockDim.x + threadIdx.x);
}
__global__ void mark_split_both_kernel(AdamDev *ad) {
    const int n = threadIdx.x;
    if (n < 2) { ad->wver[n] = ad->pver[n]; ad->wverc[n] = ad->pver[n]; }
}

int fb_qnet_refresh_planes(fb_qnet_t h, void *stream) {
    FB_REQUIRE(h, "fb_qnet_refresh_planes: NULL handle");
    const int items = wsplit_items(h->FC);
    hipLaunchKernelGGL(wsplit_both_kernel, dim3((items + 255) / 256, 2), dim3(256), 0, fb_stream(stream), h->params[0], h->params[1], h->wsp[0], h->wsp[1],
                       h->FC, (const AdamDev *)h->adam);      // (returns at once for a net whose versions agree)
    hipLaunchKernelGGL(mark_split_both_kernel, dim3(1), dim3(64), 0, fb_stream(stream), h->adam);
    FB_LAUNCH_CHECK();
    return FB_OK;
}

int fb_qnet_profile_ring(fb_qnet_t h, int kernel, int reps, int algo, int B, const FbRingSrc *ring, float *loss, void *stream) {
    FB_REQUIRE(h && ring && kernel >= 0 && kernel < K_COUNT && reps >= 1, "fb_qnet_profile_ring: bad argument");
    FB_REQUIRE(!is_per_algo(algo), "fb_qnet_profile_ring: uniform memories only");
    Plan p;
    int rc = train_plan(h, algo, B, nullptr, ring->a, ring->r, nullptr, ring->t, nullptr, 0.99, loss, nullptr, nullptr, nullptr, &p, ring);
    if (rc != FB_OK) return rc;
    p.tick = false;
    rc = fb_qnet_refresh_planes(h, stream);
    for (int i = 0; i < reps && rc == FB_OK; i++) rc = run_plan(h, p, kernel, fb_stream(stream));
    return rc;
}

extern "C" int fb_qnet_train_step(fb_qnet_t h, int algo, int B, const uint8_t *s, const uint8_t *a, const float *r,
                                  const uint8_t *s2, const uint8_t *t, const float *isw, double gamma, float *loss,
                                  float *abs_err, float *q_target, float *flat_grad, void *stream) {
    Plan p;
    int rc = train_plan(h, algo, B, s, a, r, s2, t, isw, gamma, loss, abs_err, q_target, flat_grad, &p);
    if (rc != FB_OK) return rc;
    return run_train(h, p, stream);
}

// ---- advantage actor-critic (include/fbdqn.h; kernels: fb_ac.hip)
extern "C" int fb_qnet_set_ac(fb_qnet_t h, float value_coef, float entropy_coef) {
    FB_REQUIRE(h, "fb_qnet_set_ac: NULL handle");
    FB_REQUIRE(is_ac(h), "fb_qnet_set_ac: not an actor-critic net (fb_qnet_create_ac)");
    FB_REQUIRE(isfinite(value_coef) && value_coef >= 0.f, "fb_qnet_set_ac: value_coef must be finite and >= 0 (got %g)", (double)value_coef);
    FB_REQUIRE(isfinite(entropy_coef) && entropy_coef >= 0.f, "fb_qnet_set_ac: entropy_coef must be finite and >= 0 (got %g)", (double)entropy_coef);
    h->ac_cv = value_coef; h->ac_ce = entropy_coef;
    return FB_OK;
}

extern "C" int fb_qnet_get_ac(fb_qnet_t h, float *value_coef_host, float *entropy_coef_host) {
    FB_REQUIRE(h, "fb_qnet_get_ac: NULL handle");
    FB_REQUIRE(is_ac(h), "fb_qnet_get_ac: not an actor-critic net (fb_qnet_create_ac)");
    if (value_coef_host) *value_coef_host = h->ac_cv;
    if (entropy_coef_host) *entropy_coef_host = h->ac_ce;
    return FB_OK;
}

extern "C" int fb_qnet_forward_ac(fb_qnet_t h, const uint8_t *states, int batch, float *logits, float *value, void *stream) {
    FB_REQUIRE(h && states && logits && value, "fb_qnet_forward_ac: NULL argument");
    FB_REQUIRE(is_ac(h), "fb_qnet_forward_ac: not an actor-critic net (fb_qnet_create_ac)");
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward_ac: batch %d exceeds 3*max_batch", batch);
    Plan p = forward_plan(h, 0, states, batch);
    p.ac_value = value; p.ac_logits = logits;
    return run_plan(h, p, -1, fb_stream(stream));
}

extern "C" int fb_qnet_act_policy_nib(fb_qnet_t h, const uint8_t *nib_states, int n, uint64_t seed, uint64_t step, int greedy, uint8_t *actions,
                                      float *value, float *logp, float *logits, void *stream) {
    FB_REQUIRE(h && nib_states && (value || is_sac(h)), "fb_qnet_act_policy_nib: NULL argument");
    FB_REQUIRE(is_ac(h) || is_sac(h), "fb_qnet_act_policy_nib: not an actor-critic or SAC net (fb_qnet_create_ac / fb_qnet_create_sac)");
    FB_REQUIRE(actions || !logp, "fb_qnet_act_policy_nib: logp needs actions");
    FB_REQUIRE(rows_ok(h, n), "fb_qnet_act_policy_nib: n %d exceeds 3*max_batch", n);
    Plan p = forward_plan(h, 0, nib_states, n);
    p.nib = true;
    p.actions = actions; p.seed = seed; p.step = step;
    p.ac_value = value; p.ac_logits = logits; p.ac_logp = logp; p.ac_greedy = greedy != 0;
    p.policy_head = true;
    return run_plan(h, p, -1, fb_stream(stream));
}

int fb_qnet_ac_check_train(fb_qnet_t h, int B, int64_t n_total, const char *who) {
    FB_REQUIRE(h && is_ac(h), "%s: not an actor-critic net (fb_qnet_create_ac)", who);
    if (const int rb = check_batch(h, B, who)) return rb;
    FB_REQUIRE(n_total >= (int64_t)B && n_total <= (int64_t)1 << 40, "%s: n_total %lld must be the whole update's sample count (>= the batch %d)", who, (long long)n_total, B);
    return FB_OK;
}

void fb_qnet_ac_scratch(fb_qnet_t h, float **r, uint8_t **t) { *r = h->ac_r; *t = h->ac_t; }
float *fb_qnet_ppo_sum(fb_qnet_t h) { return h->ppo_sum; }

// the train plan of an actor-critic net: ONE slice, s through the online net
static Plan ac_train_plan(fb_qnet *h, int B, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret, int64_t n_total, float *loss,
                          float *flat_grad, const FbRingSrc *ring) {
    Plan p; memset(&p, 0, sizeof(p));
    p.ns = 1;
    p.sl.s[0] = Slice{h->params[0], s, 0, B, h->w1s[0], 0};
    p.train = true; p.algo = -1; p.B = B; p.s = s; p.a = a; p.ac_adv = adv; p.ac_ret = ret; p.ac_nt = (float)n_total;
    p.loss = loss;
    plan_train_tail(h, p, flat_grad, ring);
    return p;
}

extern "C" int fb_qnet_ac_train_step(fb_qnet_t h, int B, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret, int64_t n_total,
                                     float *loss, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && adv && ret && loss, "fb_qnet_ac_train_step: NULL argument");
    const int rc = fb_qnet_ac_check_train(h, B, n_total, "fb_qnet_ac_train_step");
    if (rc != FB_OK) return rc;
    Plan p = ac_train_plan(h, B, s, a, adv, ret, n_total, loss, flat_grad, nullptr);
    return run_train_gathered(h, p, B, stream);
}

int fb_qnet_ac_train_ring(fb_qnet_t h, int B, const FbRingSrc *ring, const float *adv, const float *ret, int64_t n_total, float *loss,
                          float *flat_grad, void *stream) {
    FB_REQUIRE(h && ring && ring->idx && ring->a && adv && ret && loss, "fb_ac_train_from_replay: NULL argument");
    const int rc = fb_qnet_ac_check_train(h, B, n_total, "fb_ac_train_from_replay");
    if (rc != FB_OK) return rc;
    Plan p = ac_train_plan(h, B, nullptr, ring->a, adv, ret, n_total, loss, flat_grad, ring);
    return run_train(h, p, stream);
}

// ---- PPO on an actor-critic net (include/fbdqn.h; kernels: fb_ac.hip): A2C's plan with the clipped-surrogate loss launch
extern "C" int fb_qnet_set_ppo(fb_qnet_t h, float clip_eps, float value_clip) {
    FB_REQUIRE(h, "fb_qnet_set_ppo: NULL handle");
    FB_REQUIRE(is_ac(h), "fb_qnet_set_ppo: not an actor-critic net (fb_qnet_create_ac)");
    FB_REQUIRE(isfinite(clip_eps) && clip_eps > 0.f, "fb_qnet_set_ppo: clip_eps must be finite and > 0 (got %g)", (double)clip_eps);
    FB_REQUIRE(isfinite(value_clip) && value_clip >= 0.f, "fb_qnet_set_ppo: value_clip must be finite and >= 0 (got %g)", (double)value_clip);
    h->ppo_eps = clip_eps; h->ppo_vclip = value_clip;
    return FB_OK;
}

extern "C" int fb_qnet_get_ppo(fb_qnet_t h, float *clip_eps_host, float *value_clip_host) {
    FB_REQUIRE(h, "fb_qnet_get_ppo: NULL handle");
    FB_REQUIRE(is_ac(h), "fb_qnet_get_ppo: not an actor-critic net (fb_qnet_create_ac)");
    if (clip_eps_host) *clip_eps_host = h->ppo_eps;
    if (value_clip_host) *value_clip_host = h->ppo_vclip;
    return FB_OK;
}

static Plan ppo_train_plan(fb_qnet *h, int B, const uint8_t *s, const uint8_t *a, const int64_t *sel, const float *adv, const float *ret,
                           const float *logp_old, const float *value_old, int64_t n_total, float *loss, float *flat_grad, const FbRingSrc *ring) {
    Plan p = ac_train_plan(h, B, s, a, adv, ret, n_total, loss, flat_grad, ring);
    p.ppo = true; p.ppo_logp = logp_old; p.ppo_value = value_old; p.ppo_sel = reinterpret_cast<const long long *>(sel);
    return p;
}

extern "C" int fb_qnet_ppo_train_step(fb_qnet_t h, int B, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret,
                                      const float *logp_old, const float *value_old, int64_t n_total, float *loss, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && adv && ret && logp_old && value_old && loss, "fb_qnet_ppo_train_step: NULL argument");
    const int rc = fb_qnet_ac_check_train(h, B, n_total, "fb_qnet_ppo_train_step");
    if (rc != FB_OK) return rc;
    Plan p = ppo_train_plan(h, B, s, a, nullptr, adv, ret, logp_old, value_old, n_total, loss, flat_grad, nullptr);
    return run_train_gathered(h, p, B, stream);
}

int fb_qnet_ppo_train_ring(fb_qnet_t h, int B, const FbRingSrc *ring, const int64_t *sel, const float *adv, const float *ret,
                           const float *logp_old, const float *value_old, int64_t n_total, float *loss, float *flat_grad, void *stream) {
    FB_REQUIRE(h && ring && ring->idx && ring->a && adv && ret && logp_old && value_old && loss, "fb_ppo_train_from_replay: NULL argument");
    const int rc = fb_qnet_ac_check_train(h, B, n_total, "fb_ppo_train_from_replay");
    if (rc != FB_OK) return rc;
    Plan p = ppo_train_plan(h, B, nullptr, ring->a, sel, adv, ret, logp_old, value_old, n_total, loss, flat_grad, ring);
    return run_train(h, p, stream);
}

// ---- discrete soft actor-critic (include/fbdqn.h; kernels: fb_sac.hip)
// (log alpha, m, v, beta1 power, beta2 power) <- (logf(alpha), 0, 0, the net's beta1, beta2); synchronous
static int sac_write_words(fb_qnet *h, float alpha) {
    FB_CHECK_HIP(hipDeviceSynchronize());
    AdamDev a;
    FB_CHECK_HIP(hipMemcpy(&a, h->adam, sizeof(a), hipMemcpyDeviceToHost));
    const float w[8] = {logf(alpha), 0.f, 0.f, a.b1, a.b2, 0.f, 0.f, 0.f};
    FB_CHECK_HIP(hipMemcpy(h->sac_w, w, sizeof(w), hipMemcpyHostToDevice));
    return FB_OK;
}

extern "C" int fb_qnet_set_sac(fb_qnet_t h, float alpha, float target_entropy, float alpha_lr) {
    FB_REQUIRE(h, "fb_qnet_set_sac: NULL handle");
    FB_REQUIRE(is_sac(h), "fb_qnet_set_sac: not a SAC net (fb_qnet_create_sac)");
    FB_REQUIRE(isfinite(alpha) && alpha > 0.f, "fb_qnet_set_sac: alpha must be finite and > 0 (got %g)", (double)alpha);
    FB_REQUIRE(isfinite(target_entropy), "fb_qnet_set_sac: target_entropy must be finite (got %g)", (double)target_entropy);
    FB_REQUIRE(isfinite(alpha_lr) && alpha_lr >= 0.f, "fb_qnet_set_sac: alpha_lr must be finite and >= 0 (0 = a fixed temperature; got %g)", (double)alpha_lr);
    const int rc = sac_write_words(h, alpha);
    if (rc != FB_OK) return rc;
    h->sac_hbar = target_entropy; h->sac_alr = alpha_lr;
    return FB_OK;
}

extern "C" int fb_qnet_get_sac_state(fb_qnet_t h, float *state_host) {
    FB_REQUIRE(h && state_host, "fb_qnet_get_sac_state: NULL argument");
    FB_REQUIRE(is_sac(h), "fb_qnet_get_sac_state: not a SAC net (fb_qnet_create_sac)");
    FB_CHECK_HIP(hipDeviceSynchronize());
    FB_CHECK_HIP(hipMemcpy(state_host, h->sac_w, 5 * sizeof(float), hipMemcpyDeviceToHost));
    return FB_OK;
}

extern "C" int fb_qnet_set_sac_state(fb_qnet_t h, const float *state_host) {
    FB_REQUIRE(h && state_host, "fb_qnet_set_sac_state: NULL argument");
    FB_REQUIRE(is_sac(h), "fb_qnet_set_sac_state: not a SAC net (fb_qnet_create_sac)");
    FB_REQUIRE(isfinite(state_host[0]), "fb_qnet_set_sac_state: log alpha must be finite (got %g)", (double)state_host[0]);
    FB_CHECK_HIP(hipDeviceSynchronize());
    FB_CHECK_HIP(hipMemcpy(h->sac_w, state_host, 5 * sizeof(float), hipMemcpyHostToDevice));
    return FB_OK;
}

extern "C" int fb_qnet_get_sac(fb_qnet_t h, float *alpha_host, float *target_entropy_host, float *alpha_lr_host) {
    FB_REQUIRE(h, "fb_qnet_get_sac: NULL handle");
    FB_REQUIRE(is_sac(h), "fb_qnet_get_sac: not a SAC net (fb_qnet_create_sac)");
    if (alpha_host) {
        float w[5];
        const int rc = fb_qnet_get_sac_state(h, w);
        if (rc != FB_OK) return rc;
        *alpha_host = expf(w[0]);
    }
    if (target_entropy_host) *target_entropy_host = h->sac_hbar;
    if (alpha_lr_host) *alpha_lr_host = h->sac_alr;
    return FB_OK;
}

extern "C" int fb_qnet_forward_sac(fb_qnet_t h, int which, const uint8_t *states, int batch, float *logits, float *q1, float *q2, void *stream) {
    FB_REQUIRE(h && states && logits && q1 && q2 && (which == 0 || which == 1), "fb_qnet_forward_sac: bad argument");
    FB_REQUIRE(is_sac(h), "fb_qnet_forward_sac: not a SAC net (fb_qnet_create_sac)");
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward_sac: batch %d exceeds 3*max_batch", batch);
    Plan p = forward_plan(h, which, states, batch);
    p.policy_head = true; p.ac_logits = logits; p.sac_q1 = q1; p.sac_q2 = q2;
    return run_plan(h, p, -1, fb_stream(stream));
}

int fb_qnet_sac_check_train(fb_qnet_t h, int B, double gamma, const char *who) {
    FB_REQUIRE(h && is_sac(h), "%s: not a SAC net (fb_qnet_create_sac)", who);
    if (const int rb = check_batch(h, B, who)) return rb;
    return check_gamma01(gamma, who);
}

// the train plan a SAC and an IQN net share: FB_ALGO_DOUBLE's three slices -- s and s' through the online net, s' through the target net
static Plan three_slice_plan(fb_qnet *h, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t, double gamma,
                             float *loss, float *q_target, float *flat_grad, const FbRingSrc *ring) {
    Plan p; memset(&p, 0, sizeof(p));
    p.ns = 3;
    p.sl.s[0] = Slice{h->params[0], s, 0, B, h->w1s[0], 0};
    p.sl.s[1] = Slice{h->params[0], s2, B, B, h->w1s[0], 1};
    p.sl.s[2] = Slice{h->params[1], s2, 2 * B, B, h->w1s[1], 1};
    p.train = true; p.algo = -1; p.B = B; p.s = s; p.a = a; p.r = r; p.t = t; p.gamma = gamma;
    p.loss = loss; p.y = q_target;
    plan_train_tail(h, p, flat_grad, ring);
    return p;
}

// The SAC train step behind every entry point's NULL-argument checks (`who`: the one the messages name): gathered states (ring NULL) or the
// ring-fed form; isw / abs_err both set: the prioritized form, the same plan with the importance weights in and the priority out (the loss
// launch's weighted instantiation, fb_sac.hip), else both NULL.  The temperature update runs when the CALLER exports nothing and alpha_lr > 0
// (the uniform ring-fed call takes a memory at n-step 1 only, the prioritized one the memory's n: fb_sac.hip)
static int sac_train(const char *who, fb_qnet *h, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,
                     const FbRingSrc *ring, const float *isw, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    const int rc = fb_qnet_sac_check_train(h, B, gamma, who);
    if (rc != FB_OK) return rc;
    Plan p = three_slice_plan(h, B, s, a, r, s2, t, gamma, loss, q_target, flat_grad, ring);
    p.sac_temp = flat_grad == nullptr && h->sac_alr > 0.f;
    p.isw = isw; p.abs_err = abs_err;
    return ring ? run_train(h, p, stream) : run_train_gathered(h, p, B, stream);
}

extern "C" int fb_qnet_sac_train_step(fb_qnet_t h, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,
                                      double gamma, float *loss, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && r && s2 && t && loss, "fb_qnet_sac_train_step: NULL argument");
    return sac_train("fb_qnet_sac_train_step", h, B, s, a, r, s2, t, nullptr, nullptr, gamma, loss, nullptr, q_target, flat_grad, stream);
}

extern "C" int fb_qnet_sac_per_train_step(fb_qnet_t h, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,
                                          const float *isw, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && r && s2 && t && loss, "fb_qnet_sac_per_train_step: NULL argument");
    FB_REQUIRE(isw && abs_err, "fb_qnet_sac_per_train_step: the prioritized step needs the importance weights (isw) and abs_err");
    return sac_train("fb_qnet_sac_per_train_step", h, B, s, a, r, s2, t, nullptr, isw, gamma, loss, abs_err, q_target, flat_grad, stream);
}

int fb_qnet_sac_train_ring(fb_qnet_t h, int B, const FbRingSrc *ring, const float *isw, double gamma, float *loss, float *abs_err, float *q_target,
                           float *flat_grad, void *stream, const char *who) {
    FB_REQUIRE(h && ring && ring->idx && ring->a && ring->r && ring->t && loss && !isw == !abs_err, "%s: NULL argument", who);
    return sac_train(who, h, B, nullptr, ring->a, ring->r, nullptr, ring->t, ring, isw, gamma, loss, abs_err, q_target, flat_grad, stream);
}

// ---- implicit quantile networks (include/fbdqn.h; kernels: fb_iqn.hip)
extern "C" int fb_qnet_set_iqn_risk(fb_qnet_t h, float eta) {
    FB_REQUIRE(h, "fb_qnet_set_iqn_risk: NULL handle");
    FB_REQUIRE(is_iqn(h), "fb_qnet_set_iqn_risk: not an IQN net (fb_qnet_create_iqn)");
    FB_REQUIRE(isfinite(eta) && eta > 0.f && eta <= 1.f, "fb_qnet_set_iqn_risk: eta must be in (0, 1] (got %g)", (double)eta);
    FB_CHECK_HIP(hipDeviceSynchronize());        // (whatever still reads the folds of the old eta)
    h->iqn_eta = eta;
    c51d_fold(h, 0, nullptr); c51d_fold(h, 1, nullptr);
    FB_LAUNCH_CHECK();
    FB_CHECK_HIP(hipDeviceSynchronize());
    return FB_OK;
}

extern "C" int fb_qnet_get_iqn(fb_qnet_t h, int *n_tau_host, int *n_tau_next_host, int *n_tau_act_host, float *kappa_host, float *eta_host) {
    FB_REQUIRE(h, "fb_qnet_get_iqn: NULL handle");
    FB_REQUIRE(is_iqn(h), "fb_qnet_get_iqn: not an IQN net (fb_qnet_create_iqn)");
    if (n_tau_host) *n_tau_host = h->iqn_n;
    if (n_tau_next_host) *n_tau_next_host = h->iqn_np;
    if (n_tau_act_host) *n_tau_act_host = h->iqn_k;
    if (kappa_host) *kappa_host = h->kappa;
    if (eta_host) *eta_host = h->iqn_eta;
    return FB_OK;
}

// Munchausen IQN: a host-side setting the train plans made after it read (fb_qnet_set_huber's pattern)
extern "C" int fb_qnet_set_iqn_munchausen(fb_qnet_t h, int on, float temp, float alpha, float clip_lo) {
    FB_REQUIRE(h, "fb_qnet_set_iqn_munchausen: NULL handle");
    FB_REQUIRE(is_iqn(h), "fb_qnet_set_iqn_munchausen: not an IQN net (fb_qnet_create_iqn; a scalar net takes fb_qnet_set_munchausen)");
    FB_REQUIRE(on == 0 || on == 1, "fb_qnet_set_iqn_munchausen: on must be 0 or 1 (got %d)", on);
    FB_REQUIRE(isfinite(temp) && temp > 0.f, "fb_qnet_set_iqn_munchausen: temp must be finite and > 0 (got %g)", (double)temp);
    FB_REQUIRE(alpha >= 0.f && alpha <= 1.f, "fb_qnet_set_iqn_munchausen: alpha must be in [0, 1] (got %g)", (double)alpha);
    FB_REQUIRE(isfinite(clip_lo) && clip_lo <= 0.f, "fb_qnet_set_iqn_munchausen: the clip l0 must be finite and <= 0 (got %g)", (double)clip_lo);
    h->iqn_mu = on;
    h->iqn_md = MdPar{temp, alpha, clip_lo};
    return FB_OK;
}

extern "C" int fb_qnet_get_iqn_munchausen(fb_qnet_t h, int *on_host, float *temp_host, float *alpha_host, float *clip_lo_host) {
    FB_REQUIRE(h, "fb_qnet_get_iqn_munchausen: NULL handle");
    FB_REQUIRE(is_iqn(h), "fb_qnet_get_iqn_munchausen: not an IQN net (fb_qnet_create_iqn; a scalar net takes fb_qnet_get_munchausen)");
    if (on_host) *on_host = h->iqn_mu;
    if (temp_host) *temp_host = h->iqn_md.tau;
    if (alpha_host) *alpha_host = h->iqn_md.alpha;
    if (clip_lo_host) *clip_lo_host = h->iqn_md.clip;
    return FB_OK;
}

extern "C" int fb_qnet_forward_iqn(fb_qnet_t h, int which, const uint8_t *states, int batch, const float *tau, int M, float *theta, void *stream) {
    FB_REQUIRE(h && states && tau && theta && (which == 0 || which == 1), "fb_qnet_forward_iqn: bad argument");
    FB_REQUIRE(is_iqn(h), "fb_qnet_forward_iqn: not an IQN net (fb_qnet_create_iqn)");
    FB_REQUIRE(M >= 1 && M <= 64, "fb_qnet_forward_iqn: M %d outside 1..64", M);
    FB_REQUIRE(rows_ok(h, batch), "fb_qnet_forward_iqn: batch %d exceeds 3*max_batch", batch);
    Plan p = forward_plan(h, which, states, batch);
    p.iqn_tau = tau; p.iqn_m = M; p.iqn_theta = theta;
    return run_plan(h, p, -1, fb_stream(stream));
}

int fb_qnet_iqn_check_train(fb_qnet_t h, int double_q, int B, double gamma, const char *who) {
    FB_REQUIRE(h && is_iqn(h), "%s: not an IQN net (fb_qnet_create_iqn)", who);
    FB_REQUIRE(double_q == 0 || double_q == 1, "%s: double_q must be 0 or 1 (got %d)", who, double_q);
    FB_REQUIRE(!(h->iqn_mu && double_q), "%s: double_q = 1 on a net with Munchausen on (fb_qnet_set_iqn_munchausen): the soft target has no a* to choose", who);
    if (const int rb = check_batch(h, B, who)) return rb;
    return check_gamma01(gamma, who);
}

// The IQN train step behind every entry point's NULL-argument checks (`who`: the one the messages name): gathered states (ring NULL) or the
// ring-fed form; isw / abs_err both set: the prioritized form, the same plan with the importance weights in and the per-sample loss out
// (the loss launch's weighted instantiation, fb_iqn.hip), else both NULL
static int iqn_train(const char *who, fb_qnet *h, int double_q, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                     const uint8_t *t, const FbRingSrc *ring, const float *isw, const float *tau, const float *tau_next, uint64_t seed, uint64_t step,
                     double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    const int rc = fb_qnet_iqn_check_train(h, double_q, B, gamma, who);
    if (rc != FB_OK) return rc;
    Plan p = three_slice_plan(h, B, s, a, r, s2, t, gamma, loss, q_target, flat_grad, ring);
    p.iqn_tau = tau; p.iqn_tau_next = tau_next; p.iqn_double = double_q != 0; p.seed = seed; p.step = step;
    p.isw = isw; p.abs_err = abs_err;
    // Munchausen: the online net's s' slice is read by double_q alone, which is refused with it; its rows take s through the TARGET net
    // (fshift 0: plan_train_tail has left it alone), as FB_ALGO_MDQN's third slice does.  Both target slices are consecutive: one pass
    if (h->iqn_mu) { p.iqn_mu = true; p.sl.s[1] = Slice{h->params[1], s, B, B, h->w1s[1], 0}; }
    return ring ? run_train(h, p, stream) : run_train_gathered(h, p, B, stream);
}

extern "C" int fb_qnet_iqn_train_step(fb_qnet_t h, int double_q, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                                      const uint8_t *t, const float *tau, const float *tau_next, uint64_t seed, uint64_t step, double gamma,
                                      float *loss, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && r && s2 && t && loss, "fb_qnet_iqn_train_step: NULL argument");
    return iqn_train("fb_qnet_iqn_train_step", h, double_q, B, s, a, r, s2, t, nullptr, nullptr, tau, tau_next, seed, step, gamma, loss, nullptr, q_target,
                     flat_grad, stream);
}

extern "C" int fb_qnet_iqn_per_train_step(fb_qnet_t h, int double_q, int B, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                                          const uint8_t *t, const float *isw, const float *tau, const float *tau_next, uint64_t seed, uint64_t step,
                                          double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream) {
    FB_REQUIRE(h && s && a && r && s2 && t && loss, "fb_qnet_iqn_per_train_step: NULL argument");
    FB_REQUIRE(isw && abs_err, "fb_qnet_iqn_per_train_step: the prioritized step needs the importance weights (isw) and abs_err");
    return iqn_train("fb_qnet_iqn_per_train_step", h, double_q, B, s, a, r, s2, t, nullptr, isw, tau, tau_next, seed, step, gamma, loss, abs_err, q_target,
                     flat_grad, stream);
}

int fb_qnet_iqn_train_ring(fb_qnet_t h, int double_q, int B, const FbRingSrc *ring, const float *isw, const float *tau, const float *tau_next,
                           uint64_t seed, uint64_t step, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream,
                           const char *who) {
    FB_REQUIRE(h && ring && ring->idx && ring->a && ring->r && ring->t && loss && !isw == !abs_err, "%s: NULL argument", who);
    return iqn_train(who, h, double_q, B, nullptr, ring->a, ring->r, nullptr, ring->t, ring, isw, tau, tau_next, seed, step, gamma, loss, abs_err, q_target,
                     flat_grad, stream);
}

// Measurement aid for bench.py: launch ONE kernel of the train-step plan (`kernel` = KernelId, see
// fb_qnet_kernel_name) `reps` times with the real launch geometry.  It re-runs that kernel on the
// workspace a preceding fb_qnet_train_step left behind; the Adam tick is disabled, and for K_ADAM
// the step is applied `reps` times, so call it on a scratch network only.
extern "C" int fb_qnet_profile_kernel(fb_qnet_t h, int kernel, int reps, int algo, int B, const uint8_t *s, const uint8_t *a,
                                      const float *r, const uint8_t *s2, const uint8_t *t, float *loss, void *stream) {
    FB_REQUIRE(kernel >= 0 && kernel < K_COUNT && reps >= 1, "fb_qnet_profile_kernel: bad kernel id / reps");
    Plan p;
    int rc = FB_OK;
    if (algo < 0) {                              // the acting forward: one slice of B states through the online net
        FB_REQUIRE(h && s && B >= 1 && B <= 3 * h->max_batch && kernel <= K_HEAD, "fb_qnet_profile_kernel: bad forward request");
        p = forward_plan(h, 0, s, B);
        p.nib = algo == -2;                      // -2: `s` is the env kernel's nibble state
    } else rc = train_plan(h, algo, B, s, a, r, s2, t, nullptr, 0.99, loss, nullptr, nullptr, nullptr, &p);
    if (rc != FB_OK) return rc;
    p.tick = false;
    for (int n = 0; n < 2; n++) resplit_now(h, n, fb_stream(stream));      // bring both nets' split planes up to date once, outside the timed launches
    for (int i = 0; i < reps; i++) { rc = run_plan(h, p, kernel, fb_stream(stream)); if (rc != FB_OK) return rc; }
    return FB_OK;
}

extern "C" const char *fb_qnet_kernel_name(int kernel) {
    // the launches of the SMALL-batch plans (what bench.py profiles at B = 32); ids that are no launch of their own there time as ~0:
    // conv3 rides in conv23_t_kernel, head / loss in fc1_fk_kernel / fc1_bwd2_kernel, every conv weight gradient in conv_bw_kernel
    // (batches of 65 .. 255 run conv_bx_kernel + conv_dw21_kernel under the same two ids)
    static const char *names[K_COUNT] = {"conv1_pool_kernel", "conv23_t_kernel", "(conv3: in conv23_t)", "fc1_fk_kernel", "head_kernel",
                                         "(loss: in fc1_bwd2)", "fc1_bwd2_kernel", "conv_bw_kernel", "(conv2 / conv1 dW: in conv_bw)",
                                         "(conv1 dW: in conv_bw)", "slab_reduce_kernel", "adam_fused_kernel"};
    return kernel >= 0 && kernel < K_COUNT ? names[kernel] : "";
}
#endif  // FB_QNET_X_TU
