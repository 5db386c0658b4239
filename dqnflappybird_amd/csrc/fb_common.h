// Shared host/device helpers of libfbdqn.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <type_traits>
#include "../../include/fbdqn.h"

// ---------------------------------------------------------------- errors
extern thread_local char fb_err_buf[512];
int fb_set_error(int code, const char *fmt, ...);

#define FB_CHECK_HIP(expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fb_set_error(FB_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                           \
    } while (0)

#define FB_REQUIRE(cond, ...)                                          \
    do {                                                               \
        if (!(cond)) return fb_set_error(FB_ERR_INVALID, __VA_ARGS__); \
    } while (0)

#define FB_LAUNCH_CHECK() FB_CHECK_HIP(hipGetLastError())

static inline hipStream_t fb_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// ---------------------------------------------------------------- algo families (include/fbdqn.h)
static inline bool is_c51_algo(int algo) {          // trains a C51 net
    return algo == FB_ALGO_C51 || algo == FB_ALGO_C51_DOUBLE || algo == FB_ALGO_C51_PER || algo == FB_ALGO_C51_DOUBLE_PER;
}
static inline bool is_double_c51(int algo) { return algo == FB_ALGO_C51_DOUBLE || algo == FB_ALGO_C51_DOUBLE_PER; }     // a* online
static inline bool is_qr_algo(int algo) {           // trains a QR net
    return algo == FB_ALGO_QR || algo == FB_ALGO_QR_DOUBLE || algo == FB_ALGO_QR_PER || algo == FB_ALGO_QR_DOUBLE_PER;
}
static inline bool is_double_qr(int algo) { return algo == FB_ALGO_QR_DOUBLE || algo == FB_ALGO_QR_DOUBLE_PER; }       // a* online
static inline bool is_per_algo(int algo) {          // prioritized memory, importance weights, |TD error| / priority out
    return algo == FB_ALGO_PER || algo == FB_ALGO_C51_PER || algo == FB_ALGO_C51_DOUBLE_PER || algo == FB_ALGO_QR_PER ||
           algo == FB_ALGO_QR_DOUBLE_PER || algo == FB_ALGO_MDQN_PER || algo == FB_ALGO_DOUBLE_PER;
}
static inline bool is_mdqn_algo(int algo) { return algo == FB_ALGO_MDQN || algo == FB_ALGO_MDQN_PER; }      // Munchausen target, a scalar net
static inline bool is_scalar_algo(int algo) { return (algo >= FB_ALGO_DQN && algo <= FB_ALGO_PER) || is_mdqn_algo(algo) || algo == FB_ALGO_DOUBLE_PER; }      // the scalar-head algos the ring-fed calls take

// Hand-offs between kernels of two streams through device words (fb_vec_step's split schedule).  A word only ever grows (the step
// number).  Stores and polls are relaxed agent-scope atomics (they go to the coherent level, past the XCD's own L2); a reader that goes
// on to READ what the other kernel wrote adds fb_flag_acquire() -- the L2s of the eight XCDs are not coherent with each other inside a
// launch -- and the writer of such data stores the word from a kernel BEHIND the one that wrote the data (its end-of-kernel release has
// written the data back).  Waits are bounded: after ~1 s a wave counts a timeout and goes on, so none can spin forever.
__device__ __forceinline__ unsigned long long fb_flag_load(const unsigned long long *flag) { return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fb_flag_store(unsigned long long *flag, unsigned long long v) { __hip_atomic_store(flag, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fb_flag_acquire() { __atomic_thread_fence(__ATOMIC_ACQUIRE); }
// A launch's GATE workgroup: one extra workgroup at the end of the grid whose first thread does nothing but wait for a word -- so the
// launch does not retire, and the next launch on its stream does not start, before the other stream's kernel has.  One wave spins; the
// kernels behind the gate never do (waves that spin must not hold what the kernels they wait for need: a launch whose every workgroup
// waited for the acting trunk to retire kept that trunk, which wants whole SIMDs, from ever being placed).
struct FbGate { const unsigned long long *flag; unsigned long long val; unsigned *timeouts; };      // flag == NULL: no gate workgroup in the grid
__device__ __forceinline__ void fb_flag_wait(const unsigned long long *flag, unsigned long long v, unsigned *timeouts);
__device__ __forceinline__ bool fb_gate_workgroup(const FbGate &g) {          // true: this workgroup was the gate (it has waited; return)
    if (!g.flag || blockIdx.x != gridDim.x - 1) return false;
    if (threadIdx.x == 0) fb_flag_wait(g.flag, g.val, g.timeouts);
    return true;
}
__device__ __forceinline__ void fb_flag_wait(const unsigned long long *flag, unsigned long long v, unsigned *timeouts) {
    if (fb_flag_load(flag) >= v) return;
    const long long t0 = wall_clock64();
    while (fb_flag_load(flag) < v) {
        __builtin_amdgcn_s_sleep(8);
        if (wall_clock64() - t0 > 100000000LL) { atomicAdd(timeouts, 1u); break; }      // (100 MHz counter)
    }
}

// ---------------------------------------------------------------- Philox4x32-10
// This framework's own counter-based stream (the reference has a single env and
// a single shared MT19937): key = seed, counter = (entity id, draw counter, stream id, 0).
#define FB_STREAM_GAP 0u      // pipe gaps, random.randint(0,7)   game/wrapped_flappy_bird.py:212
#define FB_STREAM_EPS 1u      // epsilon-greedy                     BrainDQN.py:103-104
#define FB_STREAM_SAMPLE 2u   // uniform replay (FB_RNG_PHILOX)
#define FB_STREAM_PER 3u      // PER segment uniforms (FB_RNG_PHILOX)
#define FB_STREAM_INIT 4u     // truncated-normal weight init
#define FB_STREAM_EVAL 5u     // epsilon-greedy of fb_eval_run, counter = (env id, eval step): never the training acting stream
#define FB_STREAM_NOISE 6u    // noisy nets' factorised noise, counter = (element, step_lo, 6, 2 step_hi + net) (fb_qnet_reset_noise)
#define FB_STREAM_ENV_NOISE 7u  // per-env acting noise of noisy nets, counter = (env * nz + element, step_lo, 7, step_hi) (fb_qnet_act_nib_env_noise)
#define FB_STREAM_POLICY 8u   // the policy's action draw of an actor-critic net, counter = (row, step_lo, 8, step_hi) (fb_qnet_act_policy_nib)
#define FB_STREAM_PERM 9u     // the round function of PPO's minibatch permutation, counter = (R, draw_lo, 9, draw_hi) (fb_ac_permute)
#define FB_STREAM_TAU 10u     // IQN's quantile fractions, counter = (b * 64 + i, step_lo, 10, step_hi); .x online, .y target (fb_iqn_draw_taus)

struct fb_u4 { uint32_t x, y, z, w; };

__host__ __device__ static inline fb_u4 fb_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1,
                                                  uint32_t c2, uint32_t c3) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return fb_u4{c0, c1, c2, c3};
}

// ---------------------------------------------------------------- MT19937 (device side)
// CPython `random` / numpy legacy RandomState share this generator; state lives in HBM
// (625 words: mt[624], idx) and is advanced by a single wave.
struct FbMT { uint32_t mt[624]; uint32_t idx; };

// what a draw needs: the generator, the population size n = len(memory) at the time of the call, an error flag
// gate (split schedule of fb_vec_step, or NULL): the draw is that step's first launch on the caller's stream (it stores c_entry = gate_val
// on arrival) and the gate of the train chain behind it: it does not retire before the env step its minibatch depends on has (the
// previous step's when none of the drawn positions is >= newest_from, else this step's own)
struct FbSplitFlags;
struct FbSampleCtx { FbMT *mt; int *error; long long n; FbSplitFlags *gate; unsigned long long gate_val; long long newest_from; int wait_last_round; };
// random.sample(range(n), k) -> out[k] as a rider of another module's launch (fb_sampler.h; k == 0: no rider)
struct FbSampleRider { FbSampleCtx ctx; int k; long long setsize; long long *out; };
// fc2 / dueling head + epsilon-greedy action of one state from the fc1 partial sums (fb_head.h): the acting path's last
// kernel, which fb_vec_step lets ride in the env step launch (every env workgroup computes its own action first).
struct NetOff { int bf1, wv, bv, wq, bq, n; };
struct HeadCore {
    const float *hf; int stot, nks; float *q; int FC, A, dueling; NetOff off;
    uint8_t *actions; float epsilon; uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
// on_arrival (split schedule, or NULL): a word the launch that carries the rider stores when it arrives -- the launch in front of it (the
// acting forward's fc1 launch) has retired then
struct FbHeadRider { HeadCore c; const float *params; int on; unsigned long long *on_arrival; unsigned long long arrival_val; };
// fb_eval_run's step launch (fb_env.hip, env_kernel<true, true>): the launch walks rows of the evaluation's compacted buffers, env_of maps
// a row to its env id (the key of its gap and epsilon streams); per-env counters and the records are indexed by env id, so compaction
// moves only the row-indexed state, nibble image and map
struct FbEvalRider {
    const int32_t *env_of;                     // [rows of the launch]
    int32_t *ep_k, *ep_len;                    // [env] episodes ended / frame_steps of the running episode
    int32_t *score, *length; uint8_t *trunc;   // [env][episodes] records (caller owned)
    int episodes;
    unsigned *live;                            // envs that have not ended `episodes` episodes yet
    unsigned long long *done_step;             // the latest vector step (1-based) at which an env ended its last episode
    unsigned long long step;                   // this launch's vector step (0-based)
};
// What a kernel needs of the replay's frame ring to read transitions from it (fb_gather.h)
// nstep / gamma: the memory's n-step view (fb_replay_set_n_step; nstep = 1: the one-step transition, gamma unused)
struct FbGatherCtx {
    long long cap; int n_envs, t_f, kind;
    const unsigned long long *bits; const uint8_t *act; const float *rew; const uint8_t *term; int *error;
    int nstep; double gamma;
};
// A sampled minibatch described by where it lives in the frame ring instead of by gathered copies: the train step's first kernel reads
// the 1-bit frames itself (no gather launch, no u8 expansion) and fills a / r / t (u8 / f32 / u8 [B], [dev]) for the loss.
struct FbRingSrc { FbGatherCtx c; long long steps; const long long *idx; uint8_t *a; float *r; uint8_t *t; };
int fb_replay_ring_src(fb_replay_t h, int batch, const int64_t *idx, uint8_t *a, float *r, uint8_t *t, FbRingSrc *out);
// fb_qnet_train_step on such a minibatch (isw / abs_err: the prioritized step's importance weights in, |TD errors| out; else NULL).  The split conv planes of both nets must be current: true
// after an acting forward of >= 256 states in the same stream order (fb_vec_step), which is the only caller.
// rider: random.sample for the NEXT step in the conv3 backward launch (fb_train_steps), or NULL.
// split (the split schedule's train chain, or NULL): the fc1 backward launch gets a gate workgroup waiting for trunk_done (W_fc1's Adam span
// rides in the launch behind it), the conv backward launch one waiting for fc1_done (the Adam launch follows), and the Adam launch's
// last thread waits for env_done
int fb_qnet_train_step_ring(fb_qnet_t h, int algo, int batch, const FbRingSrc *ring, const float *isw, double gamma, float *loss,
                            float *abs_err, float *flat_grad, void *stream, const FbSampleRider *rider = nullptr, const struct FbSplitCtx *split = nullptr);
// The split schedule of fb_vec_step (fb_common.hip): the train step of a vector step on a stream of its own BESIDE the acting forward and
// the env step -- both read the weights the previous step's Adam left; only the replay push connects them, and only when the minibatch
// holds one of the transitions this very step appends (the sampler decides that on the device and opens `gate` itself when it does not).
struct FbSplitFlags {                          // [dev], one word per 64 bytes; each holds the number of the last step that reached the point
    unsigned long long c_entry, p0[7];         // the caller's stream has reached this step's first launch (the draw): all it held before is done
    unsigned long long trunk_done, p2[7];      // the acting trunk has retired (stored by the fc1 launch behind it)
    unsigned long long fc1_done, p3[7];        // the acting forward's fc1 launch has retired
    unsigned long long env_done, p4[7];        // the env step (with the push and the head riding in it) has retired
    unsigned long long last_round, p8[7];      // (acting trunks of more than one round of workgroups) the first workgroup of the LAST round has been placed
    unsigned clean_count;                      // minibatches that started beside their env step
    unsigned timeouts[7];                      // waits that gave up (must stay 0), per site: 0 the draw (env_done) 1 the side stream's entry (c_entry) 2 the fc1 backward launch's gate (trunk_done) 3 the conv backward launch's gate (fc1_done) 4 the Adam launch's last wait (env_done)
};
struct FbSplitCtx {
    hipStream_t tstream;                       // the side stream: acting forward + env step (the train chain stays on the caller's stream)
    FbSplitFlags *f;
    unsigned long long seq;                    // steps issued so far
    // HIP multiplexes streams onto a few hardware queues and promises no concurrency between two streams: on a shared queue a kernel
    // that waits for a word a LATER launch stores would sit in front of it until its time-out.  So the pair (side stream, caller's
    // stream) shakes hands once, both ways, with 20 ms waits, before the schedule is used with it (fb_split_probe)
    const void *probed_stream; int probed_ok;
};
int fb_split_probe(FbSplitCtx *ctx, void *stream);      // 1: the side stream and `stream` make progress independently of each other (synchronises both, once per stream)
// HIP deals a process's streams out over a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) in turn and promises no concurrency
// between two of them: a side stream that lands on its caller's queue runs IN LINE with it (the prioritized memory's run-ahead tree work
// then cost configs[3] 680 us per step instead of 260), and a kernel on it that polls a word a later launch of the caller's stream
// stores would wait until its time-out.  fb_streams_concurrent: a hand-shake both ways with 20 ms waits (synchronises both streams);
// fb_side_stream_beside: `current` if it passes, else up to six fresh non-blocking streams of that priority (`current` is destroyed
// when it is replaced); *ok says whether the stream returned passes.
int fb_streams_concurrent(hipStream_t side, hipStream_t caller);
hipStream_t fb_side_stream_beside(hipStream_t caller, int priority, hipStream_t current, int *ok);
FbSplitCtx *fb_qnet_split_ctx(fb_qnet_t h);    // created on first use; NULL when the runtime lacks stream memory operations (the caller falls back)
// random.sample(range(n after the coming push), batch) -> idx on `stream`, opening ctx->gate at ctx->seq when the draw is clean; 1 when launched
// wait_last_round: the draw also waits until the acting trunk on the side stream has placed the first workgroup of its last round
int fb_replay_sample_gated(fb_replay_t h, int batch, int64_t *idx, const FbSplitCtx *ctx, void *stream, int wait_last_round = 0);
// one-wave launches on `stream`: wait until *flag >= v (bounded) / *flag = v behind whatever the stream holds
int fb_split_wait(const FbSplitCtx *ctx, const unsigned long long *flag, unsigned long long v, void *stream);
int fb_split_set(const FbSplitCtx *ctx, unsigned long long *flag, unsigned long long v, void *stream);
int fb_qnet_refresh_planes(fb_qnet_t h, void *stream);      // re-split whichever net's planes are stale (decided on the device)
int fb_qnet_profile_ring(fb_qnet_t h, int kernel, int reps, int algo, int batch, const FbRingSrc *ring, float *loss, void *stream);
// Memory append as a rider of the env step: every env workgroup stores its new frame / action / reward / terminal straight
// into the ring slot of the coming push (bits: slot of env 0's frame, +100 words per env; act / rew / term: row of the
// step, +1 per env; bits == NULL: no rider).  steps_dev receives steps_new (the device mirror of the push counter).
struct FbPushRider { unsigned long long *bits; uint8_t *act; float *rew; uint8_t *term; long long *steps_dev; long long steps_new; };
// library-internal (C++ linkage): the env step with the replay sampler as an extra workgroup, and the replay side of it
int fb_env_step_rider(fb_env_t h, const uint8_t *actions, uint8_t *frames, uint64_t *frame_bits, float *reward, uint8_t *terminal,
                      int32_t *score, const FbSampleRider *rider, const FbPushRider *push, const FbHeadRider *head, void *stream);
int fb_qnet_num_actions(fb_qnet_t h);
int fb_qnet_is_c51(fb_qnet_t h);              // 1: a C51 net (fb_qnet_create_c51 / _c51_dueling / _c51_noisy)
int fb_qnet_is_qr(fb_qnet_t h);               // 1: a QR net (fb_qnet_create_qr)
// 1: a distributional head (C51 or QR): the head is its own launch (no env rider, the one-stream order of fb_vec_step)
int fb_qnet_is_dist(fb_qnet_t h);
// the extended scalar loss kernels (FB_ALGO_DOUBLE_PER / Huber), instantiated in fb_qnet_x.hip: a code object of their own (see fb_qnet.hip).
// largs / mdpar: fb_qnet.hip's LossArgs (Bw1Args) and MdPar, as bytes
void fb_qnet_launch_loss_head_x(int dp, int hu, int md, unsigned grid, hipStream_t st, const void *largs, const void *mdpar, float delta);
void fb_qnet_launch_fc1_bwd2_x(int dp, int hu, int md, unsigned grid, hipStream_t st, const void *largs, const void *mdpar, float delta);
// global-norm gradient clipping and the soft target update, in the same code object: grad_sumsq_kernel + grad_clip_kernel over g[n] (part:
// 256 float64 partials, out: (norm, c)); target_lerp_kernel, t += rho (o - t) over n floats.  fb_qnet_max_grad_norm: the net's limit, 0 = off
void fb_qnet_launch_clip_x(hipStream_t st, float *g, long long n, double *part, float G, float *out);
void fb_qnet_launch_target_lerp_x(hipStream_t st, float *t, const float *o, long long n, float rho);
float fb_qnet_max_grad_norm(fb_qnet_t h);
// fb_eval_run on a distributional (C51 or QR) net: launch the head fb_qnet_eval_trunk described in *hd (q / actions / epsilon / seeds filled in by the caller),
// epsilon draws keyed key_of[row] on FB_STREAM_EVAL; the eval step launch then reads the actions (its head rider stays off)
int fb_qnet_c51_eval_head(fb_qnet_t h, const FbHeadRider *hd, int n, const int32_t *key_of, void *stream);
// fb_eval_run's acting forward: conv1 .. fc1 of n nibble states (1 <= n <= 3 * max_batch) through the fused two-plane trunk at ANY n (the
// acting path switches to the small-batch kernels below 256 states), the head described in *head for the eval step launch
int fb_qnet_eval_trunk(fb_qnet_t h, const uint8_t *nib_states, int n, FbHeadRider *head, void *stream);
int fb_qnet_max_rows(fb_qnet_t h);            // 3 * max_batch: the most states one acting forward takes
hipStream_t fb_qnet_side_stream(fb_qnet_t h); // the split schedule's side stream if the net has one, else NULL (never creates it)
void *fb_qnet_get_grad_event(fb_qnet_t h);                 // the event fb_qnet_set_grad_event installed, or NULL
// the event the LAST gradient-exporting train step recorded behind its fc1 backward launch (NULL: none was recorded); reading clears it
void *fb_qnet_take_grad_event_recorded(fb_qnet_t h);
// argument checks fb_vec_step makes BEFORE any counter moves or any launch goes out (0 = fine, else the error code with
// fb_last_error set): the batch the train step would reject / the env count the acting forward would reject
int fb_qnet_check_step(fb_qnet_t h, int n_envs, int train_batch);
// noisy nets' acting noise (include/fbdqn.h): the mode fb_qnet_set_acting_noise set (FB_ACT_NOISE_SHARED for any other net); the checks
// fb_qnet_act_nib_env_noise makes for n states (FB_OK, else the error code with fb_last_error set); that call without its final restore of
// the online net's effective parameters (fb_vec_step: the fb_qnet_reset_noise(0) behind it rebuilds them anyway)
int fb_qnet_acting_noise(fb_qnet_t h);
int fb_qnet_check_env_noise(fb_qnet_t h, int n, const char *who);
int fb_qnet_act_nib_env_noise_keep(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                                   uint8_t *actions, float *q, void *stream);
// ---- advantage actor-critic (FB_ARCH_AC): the kernels live in fb_ac.hip, a code object of their own; fb_qnet.hip fills these structs and
// hands them to the launchers below.  P: the net's parameters (or the fused acting forward's copy, hp_act - off.bf1); off: the dueling
// layout, wv / bv = W_v b_v, wq / bq = W_pi b_pi
struct FbAdamHead { float b1pow, b2pow, alpha, lr, b1, b2, eps, pad; int ticks, applies; };      // the base of fb_qnet.hip's AdamDev
struct AcHeadArgs {
    const float *hf, *P; int stot, nks, FC, A, rows; NetOff off;
    float *logits, *value, *logp; uint8_t *actions;              // logits f32[rows][A] or NULL; logp or NULL; actions NULL: no action (forward_ac)
    int greedy; uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
struct AcLossArgs {
    const float *hf, *P; int stot, nks, FC, A, B; NetOff off;
    const uint8_t *act; const float *adv, *ret; float nt, cv, ce;      // nt = (float)n_total
    float *dl, *xs, *dhf;                                        // dl f32[B][16]: dz, dV, the loss terms (fb_ac.hip)
};
// PPO's loss launch (ppo_loss_kernel): A2C's arguments, the clip ranges, and the rollout's buffers read at sel[b] (sel NULL: at b)
struct PpoLossArgs {
    AcLossArgs a;
    const long long *sel; const float *logp_old, *value_old; float eps, vclip;
};
// nterms: the loss terms of dl's columns 9 .. 9 + nterms - 1 that workgroup 0 sums: 3 for A2C (loss f32[4]), 5 for PPO (loss f32[6])
struct AcGradArgs { int B, FC, A; NetOff off; const float *dl, *xs, *dhf; float nt, cv, ce; float *grad, *loss, *gmax; FbAdamHead *adam; int tick; int nterms; };
void fb_ac_launch_head(hipStream_t st, const AcHeadArgs &H);
void fb_ac_launch_loss(hipStream_t st, const AcLossArgs &L);
void fb_ac_launch_ppo_loss(hipStream_t st, const PpoLossArgs &Q);
void fb_ac_launch_grad(hipStream_t st, const AcGradArgs &L);
int fb_qnet_is_ac(fb_qnet_t h);               // 1: an actor-critic net (fb_qnet_create_ac)
// the checks of the two AC training calls (batch, n_total), `who` in the message; the scratch r / t rows the ring-fed trunk fills beside
// a_out; the ring-fed AC train step behind fb_ac_train_from_replay's checks
int fb_qnet_ac_check_train(fb_qnet_t h, int batch, int64_t n_total, const char *who);
void fb_qnet_ac_scratch(fb_qnet_t h, float **r, uint8_t **t);
float *fb_qnet_ppo_sum(fb_qnet_t h);          // [dev] f32[6] of an actor-critic net: fb_ppo_epoch's running sum of the chunks' loss numbers
int fb_qnet_ac_train_ring(fb_qnet_t h, int batch, const FbRingSrc *ring, const float *adv, const float *ret, int64_t n_total, float *loss,
                          float *flat_grad, void *stream);
// the ring-fed PPO train step behind fb_ppo_train_from_replay's checks (sel NULL: the four buffers are read at b)
int fb_qnet_ppo_train_ring(fb_qnet_t h, int batch, const FbRingSrc *ring, const int64_t *sel, const float *adv, const float *ret,
                           const float *logp_old, const float *value_old, int64_t n_total, float *loss, float *flat_grad, void *stream);
// ---- discrete soft actor-critic (FB_ARCH_SAC): the kernels live in fb_sac.hip, a code object of their own; fb_qnet.hip fills these structs
// and hands them to the launchers below.  off: the PLAIN layout, wq / bq = W_pi b_pi; so: the two Q heads behind it.  sw: the net's
// temperature words (log alpha, m, v, beta1 power, beta2 power)
struct SacOff { int wq1, bq1, wq2, bq2; };
struct SacHeadArgs {
    const float *hf, *P; int stot, nks, FC, A, rows; NetOff off; SacOff so; const float *sw;
    float *logits, *value, *logp, *q1, *q2; uint8_t *actions;    // each f32 output or NULL; actions NULL: no action (forward_sac)
    int greedy; uint32_t seed_lo, seed_hi, step_lo, step_hi;
};
struct SacLossArgs {
    const float *hf, *P0, *P1; int stot, nks, FC, A, B; NetOff off; SacOff so; const float *sw;      // P0 / P1: the online / target parameters
    const uint8_t *act, *term; const float *rew; double gamma;
    float *dl, *xs, *dhf, *y_out;                                // dl f32[B][16] (fb_sac.hip); y_out f32[B] or NULL
};
// What the prioritized loss launch takes: SacLossArgs and, behind its last field, isw / abs_err, both f32[B], both set (the weights in,
// 0.5 (|d1| + |d2|) out).  The uniform launch keeps SacLossArgs, so its kernels are the ones of before the prioritized form existed
struct SacPerLossArgs : SacLossArgs { const float *isw; float *abs_err; };
// temp: the temperature update runs (alpha_lr > 0 and the step applies Adam itself)
struct SacGradArgs { int B, FC, A; NetOff off; SacOff so; const float *dl, *xs, *dhf; float *grad, *loss, *gmax; FbAdamHead *adam; int tick;
                     float *sw; float target_entropy, alpha_lr; int temp; };
void fb_sac_launch_head(hipStream_t st, const SacHeadArgs &H);
void fb_sac_launch_loss(hipStream_t st, const SacLossArgs &L);
void fb_sac_launch_per_loss(hipStream_t st, const SacPerLossArgs &L);
void fb_sac_launch_grad(hipStream_t st, const SacGradArgs &L);
int fb_qnet_is_sac(fb_qnet_t h);              // 1: a SAC net (fb_qnet_create_sac)
// the checks of the SAC training calls, `who` in the message; the ring-fed SAC train step behind the checks of `who` -- fb_sac_train_from_replay
// (isw / abs_err NULL), or fb_sac_per_train_from_replay, the prioritized form (isw / abs_err f32[batch], both non-NULL).  gamma: the
// bootstrap's discount
int fb_qnet_sac_check_train(fb_qnet_t h, int batch, double gamma, const char *who);
int fb_qnet_sac_train_ring(fb_qnet_t h, int batch, const FbRingSrc *ring, const float *isw, double gamma, float *loss, float *abs_err, float *q_target,
                           float *flat_grad, void *stream, const char *who);
// ---- implicit quantile networks (FB_ARCH_IQN): the kernels live in fb_iqn.hip, a code object of their own; fb_qnet.hip fills these structs
// and hands them to the launchers below.  off: the PLAIN layout (wq / bq = W_q b_q); io: the embedding behind it, W_e[64][FC] b_e[FC].
// A fold block is [b_fc1 | phibar * W_q | b_q]: the plain layout from b_fc1 on, so `block - off.bf1` is read as a plain net's parameters
struct IqnOff { int we, be; };
// A dueling IQN net (FB_ARCH_IQN_DUELING; `dueling` = 1, the last field of every struct below): off is the DUELING layout (wv / bv = W_v b_v,
// wq / bq = W_a b_a) and the kernels read the effective column We[k, a] = (W_v[k] + W_a[k, a]) - m_k, be[a] where W_q b_q stood; the fold block
// keeps the plain layout, [b_fc1 | phibar * We | be], and IqnLossArgs::foff holds ITS offsets (the plain layout's; = off for a plain IQN net)
struct IqnFoldArgs { const float *P; float *fold; int FC, A, K; NetOff off; IqnOff io; float eta; int dueling; };
// theta f32[rows][M][A] at tau f32[rows][M]
struct IqnHeadArgs { const float *hf, *P; int stot, nks, FC, A, rows, M; NetOff off; IqnOff io; const float *tau; float *theta; int dueling; };
// P0 / P1: the online / target parameters; F: the fold block (minus off.bf1) of the net that chooses a* -- online (double_q) or target --
// and arow0 the first of its rows of hf (B or 2 B).  tau / tau_next NULL: the draws of (seed, step)
struct IqnLossArgs {
    const float *hf, *P0, *P1, *F; int arow0, stot, nks, FC, A, B, N, Np; NetOff off; IqnOff io; float kappa;
    const uint8_t *act, *term; const float *rew; double gamma; const float *tau, *tau_next;
    uint32_t seed_lo, seed_hi, step_lo, step_hi;
    float *dl, *gw, *dhf, *dpre, *ctab, *t_out;                  // dl f32[B][4]; gw f32[B][FC]; dpre f32[B N][FC]; ctab f32[B N][64]; t_out f32[B][Np] or NULL
    // isw / abs_err, the prioritized form: both f32[B], both set (the weights in, l_b out); else both NULL.  foff: the offsets F is read with
    const float *isw; float *abs_err; NetOff foff; int dueling;
};
// What the loss launch takes (fb_iqn_launch_loss's parameter type): IqnLossArgs and, behind its last field, Munchausen IQN's five (fb_qnet_set_iqn_munchausen).  mu = 1: F is the
// TARGET net's fold, arow0 = 2 B (s') and srow0 = B the first row of the slice that holds s through the target net; (temp, alpha, clip_lo)
// the net's.  mu = 0: none of the five is read
struct IqnLossMuArgs : IqnLossArgs { int mu; float temp, alpha, clip_lo; int srow0; };
struct IqnGradArgs { int B, FC, A, N; NetOff off; IqnOff io; const float *dl, *gw, *dhf, *dpre, *ctab; float *grad, *loss, *gmax; FbAdamHead *adam; int tick; int dueling; };
// ---- noisy IQN nets (fb_qnet_create_iqn_noisy, include/fbdqn.h).  The fold launch's noisy variant takes IqnFoldArgs and, behind its last
// field, pbar f32[FC]: phibar of the acting grid, which the per-env head scales sigma's head rows by (the plain launch keeps IqnFoldArgs)
struct IqnFoldNzArgs : IqnFoldArgs { float *pbar; };
// the fc1 stage of the per-env acting forward (fb_qnet.hip, the C51 and the IQN path alike): behind the argument checks it materialises
// mu into the online net's effective vector, refolds, runs conv1 .. fc1 of the n nibble states and sigma's fc1 GEMM over the per-env scaled
// activations.  *o: the mu fc1 partials hf[nks][stot][FC], sigma's t partials ht[FC1_SP_KS][stot][FC], sig with sigma of mu entry q at sig[q]
struct FbEnvNoiseFc1 { const float *hf, *ht, *sig; int stot, nks, nkt; };      // nkt: the t partials (fb_qnet.hip's FC1_SP_KS)
int fb_qnet_env_noise_fc1(fb_qnet_t h, const uint8_t *nib_states, int n, uint64_t seed, uint64_t step, FbEnvNoiseFc1 *o, void *stream);
// the per-env scalar head (iqn_env_noise_head_kernel).  F / foff: the MU fold block (minus off.bf1) and its plain offsets; sig / off: sigma in
// the net's own layout; nz and the e_* offsets: the noise vector's length and where fc1's eps_out, the V layer's and the Q / advantage
// layer's eps_in / eps_out start in it; key_of (or NULL: the row) keys the noise and the epsilon draw, the latter on `stream`
struct IqnEnvNoiseArgs {
    const float *hf, *ht; int stot, nks, nkt;
    const float *F; NetOff foff; const float *sig; NetOff off; const float *pbar;
    int n, FC, A, nz, e_fc1_out, e_v_in, e_v_out, e_q_in, e_q_out;
    float *q; uint8_t *actions; float epsilon; uint32_t seed_lo, seed_hi, step_lo, step_hi;
    const int32_t *key_of; uint32_t stream; int dueling;
};
void fb_iqn_launch_fold_noisy(hipStream_t st, const IqnFoldNzArgs &F);
void fb_iqn_launch_env_noise_head(hipStream_t st, const IqnEnvNoiseArgs &H);
void fb_iqn_launch_fold(hipStream_t st, const IqnFoldArgs &F);
void fb_iqn_launch_head(hipStream_t st, const IqnHeadArgs &H);
void fb_iqn_launch_loss(hipStream_t st, const IqnLossMuArgs &L);
void fb_iqn_launch_grad(hipStream_t st, const IqnGradArgs &L);
int fb_qnet_is_iqn(fb_qnet_t h);              // 1: an IQN net (fb_qnet_create_iqn, fb_qnet_create_iqn_dueling)
// the checks of the IQN training calls, `who` in the message; the ring-fed IQN train step behind the checks of `who` -- fb_iqn_train_from_replay
// (isw / abs_err NULL), or fb_iqn_per_train_from_replay, the prioritized form (isw / abs_err f32[batch], both non-NULL).  gamma: the
// bootstrap's discount
int fb_qnet_iqn_check_train(fb_qnet_t h, int double_q, int batch, double gamma, const char *who);
int fb_qnet_iqn_train_ring(fb_qnet_t h, int double_q, int batch, const FbRingSrc *ring, const float *isw, const float *tau, const float *tau_next,
                           uint64_t seed, uint64_t step, double gamma, float *loss, float *abs_err, float *q_target, float *flat_grad, void *stream,
                           const char *who);
// ---- the refusal rules of the ring-fed entry points (fb_common.hip): made before any counter moves or any launch; FB_OK, else the error
// code with fb_last_error naming `who`
int fb_check_q_net(fb_qnet_t net, const char *who, bool steps);       // no AC / SAC / IQN net (steps: `who` steps the envs too)
int fb_check_algo(fb_replay_t replay, fb_qnet_t net, int algo, const char *who, bool takes_per = true);       // algo against net and memory
int fb_check_step_handles(fb_env_t env, fb_replay_t replay, fb_qnet_t net, int n_envs, const char *who);      // n_envs: the handles', <= 3 * max_batch
// a uniform memory ("%s: `uniform_only`") at n-step 1 ("... `reads` at n-step 1 only")
int fb_check_uniform_n1(fb_replay_t replay, const char *who, const char *uniform_only, const char *reads);
// fb_replay_ring_src, and W_fc1's planes re-split where the batch reads them (>= 256): what a ring-fed train call does behind its checks
int fb_ring_src_fresh(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, uint8_t *a, float *r, uint8_t *t, FbRingSrc *ring, void *stream);
// the memory of the prioritized SAC and IQN calls (include/fbdqn.h: calls of their own, the memory's kind never switches what a call does;
// `uniform_calls` names the family's uniform ones): a prioritized one, whose gamma the caller's is and whose tree holds a leaf once
// `pushes_ahead` more pushes are counted (pushes_ahead < 0: a store-only step, which samples nothing)
int fb_check_per_memory(fb_replay_t replay, double gamma, int pushes_ahead, const char *who, const char *uniform_calls);
int fb_env_num_envs(fb_env_t h);
int fb_replay_num_envs(fb_replay_t h);
int fb_replay_is_prioritized(fb_replay_t h);
// n-step memories (fb_replay_set_n_step): the gamma a ring-fed training call was given must be the memory's (FB_OK, else FB_ERR_INVALID
// with fb_last_error naming `who`); the discount its bootstrap then takes is Gamma = gamma^n (the running product), `gamma` itself at n = 1
int fb_replay_check_gamma(fb_replay_t h, double gamma, const char *who);
// prioritized n-step memories (fb_replay_create_nstep): FB_ERR_STATE (fb_last_error naming `who`) when the tree will still be empty
// once `pushes_ahead` more pushes are counted -- fewer than n pushes since the reset; FB_OK for every other memory
int fb_replay_check_complete(fb_replay_t h, int pushes_ahead, const char *who);
double fb_replay_bootstrap_gamma(fb_replay_t h, double gamma);
// FB_PER_INIT_TD memories (fb_replay_set_priority_init): the setting; at n = 1 the gamma a step trains with must be the one the memory
// forms its TD priorities with (FB_ERR_INVALID naming `who` otherwise; FB_OK for every other memory); the online net's acting output
int fb_replay_priority_init(fb_replay_t h);
int fb_replay_check_prime_gamma(fb_replay_t h, double gamma, const char *who);
// fb_replay_prime_priorities between fb_replay_begin_push_rider (the push is counted) and fb_replay_finish_push (its leaves are stored)
int fb_replay_prime_before_finish(fb_replay_t h, const float *q, const uint8_t *actions, int n_actions, void *stream);
const float *fb_qnet_acting_q(fb_qnet_t h);
int fb_replay_update_priorities_keep(fb_replay_t h, int batch, const int64_t *idx, const float *abs_err, void *stream);       // in line, abs_err left untouched (fb_vec_step)
int fb_replay_update_priorities_ahead(fb_replay_t h, int batch, const int64_t *idx, const float *abs_err, void *stream);      // batch_update on the side stream (see fb_replay.hip); 1 when issued
int fb_replay_per_store_ahead(fb_replay_t h, void *stream);
int fb_replay_sample_ahead(fb_replay_t h, int batch, int64_t *idx, double *isw, float *isw32, void *stream);      // Memory.sample behind that store, on the same stream; 1 when issued      // the tree part of the coming push, ahead of it on a side stream (see fb_replay.hip)
int fb_env_can_carry_head(fb_env_t h);        // 1 when an env workgroup of the step launch has a wave per env it walks (<= 4 envs per workgroup)
// fb_qnet_act_nib without its last launch: conv1 .. fc1 are launched, *head describes the head_kernel work left over
// split (or NULL): the split schedule's context -- the fc1 launch stores trunk_done on arrival (the trunk in front of it has retired)
int fb_qnet_act_nib_rider(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                          uint8_t *actions, FbHeadRider *head, void *stream, const FbSplitCtx *split = nullptr);
// the rider for the frame / scalar part of "fb_replay_push" (returns 1, fills *push and COUNTS the push: the env launch that carries it
// must follow, and fb_replay_finish_push behind that launch: Memory.store's tree update of a prioritized memory -- joined if it ran
// ahead on the side stream, launched otherwise; nothing for a uniform memory)
int fb_replay_begin_push_rider(fb_replay_t h, FbPushRider *push);
int fb_replay_finish_push(fb_replay_t h, void *stream);
// fb_replay_sample that also leaves the importance weights as float32 (the loss's placeholder type), or NULL
int fb_replay_sample_f32(fb_replay_t h, int batch, const double *uniforms, int64_t *idx, double *isw, float *isw32, void *stream);
// the rider for "fb_replay_push; fb_replay_sample(batch) -> idx" (memory as it will be after `pushes_ahead` more pushes).  Returns 1 and
// fills *rider for a uniform memory with the CPython generator, 0 when the sampler cannot ride (PER, other generators).
int fb_replay_sample_rider(fb_replay_t h, int batch, int64_t *idx, FbSampleRider *rider, int pushes_ahead = 1);
void fb_mt_init_genrand_host(FbMT *s, uint32_t seed);
void fb_mt_init_by_array_host(FbMT *s, const uint32_t *key, int n);
// ---- the fused steps of the replay-fed families (fb_sac_step, fb_iqn_step and their prioritized forms): check -> act -> fb_env_step ->
// fb_step_store_train.  Every argument check of the calls a step makes is made before the first launch, so nothing is launched and no
// push is counted before a refusal.
// fb_check_step_buffers: what a step begins with, the handles and the buffers it writes.  The uniform step's push samples into b->idx
// whether it trains or not; the prioritized one draws, and needs idx and the weights' buffers, only when it trains
int fb_check_step_buffers(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int train, bool prioritized, const char *who);
// what a step ends with (the soft update of SAC aside): the store and, when it trains, the family's ring-fed train call
// train_call(isw, abs_err) -- uniform: fb_replay_push_sample, train_call(NULL, NULL); prioritized: Memory.store -> Memory.sample -> the
// weighted loss -> Memory.batch_update, in line on `stream` at every env count; abs_err stays as the loss left it
template <class TrainCall>
static inline int fb_step_store_train(fb_replay_t replay, const fb_step_buffers *b, int batch, int train, bool prioritized, void *stream, TrainCall train_call) {
    if (!prioritized) {
        const int rc = fb_replay_push_sample(replay, nullptr, b->frame_bits, b->actions, b->reward, b->terminal, batch, b->idx, stream);
        return rc != FB_OK || !train ? rc : train_call(nullptr, nullptr);
    }
    int rc = fb_replay_push(replay, nullptr, b->frame_bits, b->actions, b->reward, b->terminal, stream);
    if (rc != FB_OK || !train) return rc;
    rc = fb_replay_sample_f32(replay, batch, nullptr, b->idx, b->isw, b->isw32, stream);
    if (rc == FB_OK) rc = train_call(b->isw32, b->abs_err);
    return rc != FB_OK ? rc : fb_replay_update_priorities_keep(replay, batch, b->idx, b->abs_err, stream);
}
