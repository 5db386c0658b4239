/*
 * include/fbdqn.h -- C ABI of libfbdqn.so, the MI355X (gfx950) Flappy-Bird DQN hot path.
 *
 * This is the drop-in boundary.  The reference (angela000/DQNFlappyBird) is pure
 * Python and has no FFI layer of its own; its boundary is the duck-typed surface
 * FlappyBirdDQN.py uses (GameState.frame_step, Brain.getAction / setPerception).
 * Each entry point below names the reference function it stands behind
 * (paths relative to the reference checkout); the modules under dqnflappybird_amd/ bind them
 * with ctypes and re-creates the reference's class surface on top.
 *
 * Conventions
 *   - every pointer marked [dev] is device memory owned by the CALLER (e.g.
 *     torch.Tensor.data_ptr()); the library never frees caller memory;
 *   - [host] pointers are ordinary host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); every
 *     call is asynchronous on it unless documented otherwise; nothing here
 *     allocates or synchronises inside the step functions, so a caller may
 *     capture them into a hipGraph;
 *   - return value: 0 = FB_OK, negative = error; fb_last_error() gives the text
 *     (thread-local).  No C++ exception crosses the boundary;
 *   - one handle per GPU; handles are not thread-safe; distinct handles are
 *     independent.
 *
 * Environment variables libfbdqn.so reads: diagnostics only, neither selects a code path nor changes a result:
 *   FB_ABORT_LOG=path         file the SIGABRT hook appends the native back-trace to (fb_debug_abort_backtrace)
 *   FB_SIDE_PROBE_DEBUG=1     print what the side-stream checks measured (fb_streams_concurrent, csrc/fb_common.hip) to stderr
 * The Python side reads FB_LIB (another build of this library), FB_DP_NATIVE / FB_DP_OVERLAP (which data-parallel path, dist.py).
 * Modes that DO change results (FB_PER_FAST, the train dtype, pipelined acting) are API calls below, never variables.
 */
#ifndef FBDQN_H
#define FBDQN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FB_OK 0
#define FB_ERR_INVALID (-1)      /* bad argument / shape */
#define FB_ERR_HIP (-2)          /* a HIP runtime call failed */
#define FB_ERR_NOMEM (-3)
#define FB_ERR_STATE (-4)        /* call order (e.g. sample before enough pushes) */

const char *fb_last_error(void);
int fb_version(void);
/* number of visible HIP devices, or a negative error; used by the shim to fail loudly */
int fb_device_count(void);
/* Diagnostics: install a SIGABRT handler that writes the aborting thread's native call stack to stderr -- and to the file the
 * environment variable FB_ABORT_LOG names, if set: a test runner may have captured descriptor 2 -- before the previous handler
 * runs (the GPU runtimes abort() on fatal errors, not always with a message).  Idempotent. */
int fb_debug_abort_backtrace(void);

/* ------------------------------------------------------------------ environment
 * N independent games stepped per launch, render + 80x80 preprocess fused in.
 *   GameState.__init__    game/wrapped_flappy_bird.py:59-85
 *   GameState.frame_step  game/wrapped_flappy_bird.py:87-183
 *   getRandomPipe         game/wrapped_flappy_bird.py:208-221
 *   checkCrash/pixelCollision  :244-300
 *   flappy_bird_utils.load/getHitmask  game/flappy_bird_utils.py:16-124 (-> sprite blob)
 *   preprocess            FlappyBirdDQN.py:31-34
 */
typedef struct fb_env *fb_env_t;

#define FB_ENV_STATE_INTS 16     /* layout of one env in get/set_state, see below */

/* sprite_blob: the packed sprites (tools/make_assets.py layout, 57 756 bytes) [host]. */
int fb_env_create(int n_envs, uint64_t seed, uint32_t flags, const void *sprite_blob, size_t blob_bytes,
                  fb_env_t *out);
int fb_env_destroy(fb_env_t h);
/* GameState.__init__ for every env (draws two pipe gaps each). */
int fb_env_reset(fb_env_t h, void *stream);
/* frame_step for every env.
 *   actions   [dev] u8[N]      0 = do nothing, 1 = flap (index of the one-hot's 1); any other
 *                              value is the reference's ValueError: the env is left untouched
 *                              and counted in fb_env_error_count()
 *   frames    [dev] u8[N,80,80] or NULL: preprocess(image_data) = {0,255}, [x_small][y_small]
 *   frame_bits[dev] u64[N,100] or NULL: the same frame, 1 bit per pixel (bit i of the row-major
 *                              pixel index i lives in word i/64, bit i%64)
 *   reward    [dev] f32[N]     0.1 / 3 / -3
 *   terminal  [dev] u8[N]
 *   score     [dev] i32[N]     score_return (captured before the reset on a crash)
 */
int fb_env_step(fb_env_t h, const uint8_t *actions, uint8_t *frames, uint64_t *frame_bits, float *reward,
                uint8_t *terminal, int32_t *score, void *stream);
/* Observation of the current state without stepping (used for the very first frame only by
 * tests; the reference obtains it with a do-nothing frame_step, FlappyBirdDQN.py:65-66). */
int fb_env_observe(fb_env_t h, uint8_t *frames, uint64_t *frame_bits, void *stream);
/* Parity / checkpoint access; synchronous.  i32[N][16] [host]:
 *   0 playery 1 velY 2 playerIndex 3 loopIter 4 basex 5 score 6 nPipes
 *   7..9 pipe x 10..12 pipe gap index (0..7) 13 PLAYER_INDEX_GEN phase 14 rng counter 15 tape cursor */
int fb_env_get_state(fb_env_t h, int32_t *state_host);
/* fb_env_set_state refuses (FB_ERR_INVALID) a wing pose outside 0..2, a basex outside {0,-4,..,-44}, a gap index outside 0..7 and a
 * pipe count outside 1..3; it does not check the rest.  The domain the step and the observation are specified and tested on
 * (tests/test_gpu_env_sweep.py: equal to the oracle env at every point of it) is what play reaches, for every integer pipe x:
 *   playery 0..379 (at or below 380 the step has crashed and reset; the observation's bird rows cover y < 384 from a table and
 *   fall back to the per-pixel path outside, and the ground-only columns 63..79 assume the bird never lies below y = 403),
 *   velY -9..10, loopIter 0..29, phase 0..3, nPipes 2..3 with pipe x ascending and slots >= nPipes zero (a step may leave 1 pipe
 *   behind when it removes the first of 2; a third pipe only exists while the first is at x <= 4), rng counter / tape cursor >= 0. */
int fb_env_set_state(fb_env_t h, const int32_t *state_host);
/* Replace the Philox pipe-gap stream by an explicit tape of random.randint(0,7) results
 * (i8[N][tape_len], [host], copied); tape_len = 0 switches back to Philox. Synchronous. */
int fb_env_set_gap_tape(fb_env_t h, const int8_t *tape_host, int tape_len);
/* pygame.surfarray.array3d of one env: u8[288,512,3] [dev] (debug / parity). */
int fb_env_render_full(fb_env_t h, int env_id, uint8_t *rgb, void *stream);
/* Register (or clear with NULL) a caller-owned buffer u8[N][FB_NIB_STRIDE] [dev] that every following fb_env_observe /
 * fb_env_step keeps equal to the agent's 4-frame stack (BrainDQN.py:68,238-239) in "nibble" form: one byte = two
 * horizontally adjacent pixels, bit 4*px + f = frame f of the stack (f = 3 newest).  The image is stored with conv1's
 * SAME padding around it, so that the acting conv1 reads every tap at a fixed offset from one base address with no
 * bounds check: FB_NIB_ROWS rows of FB_NIB_PITCH bytes = [4 zero bytes][40 bytes: pixels 0..79 of the row]; image row r
 * is buffer row r + 2 (two zero rows above, two below; the right-hand padding of a row is the zero prefix of the next),
 * i.e. pixels (r, 2q), (r, 2q+1) live in byte (r + 2) * FB_NIB_PITCH + 4 + q.  observe zeroes the padding and fills all
 * four frames with the observation (setInitState); a step shifts and appends.  fb_qnet_act_nib consumes it, which
 * removes the currentState expansion from the acting path.  Synchronous. */
#define FB_NIB_PITCH 44
#define FB_NIB_ROWS 84
#define FB_NIB_STRIDE 3712      /* 84 * 44 = 3696, + 16 so that the last row's right-hand taps stay inside */
int fb_env_set_nib_buffer(fb_env_t h, uint8_t *nib_states);
/* Register (or clear with NULL) a caller-owned u64[4] [dev] that every following fb_env_step updates with atomics:
 * [0] episodes ended (the reference's gameTimes, BrainDQN.py:92), [1] sum and [2] maximum of their scores
 * (score_every_episode, :94), [3] pipes passed (reward 3 events).  The vectorised loop reads it back whenever it
 * logs, instead of syncing per step.  The caller zeroes it.  Synchronous. */
int fb_env_set_stats_buffer(fb_env_t h, uint64_t *stats);
/* number of invalid actions seen so far (synchronous). */
int fb_env_error_count(fb_env_t h, int64_t *count_host);
/* preprocess() of FlappyBirdDQN.py:31-34 (cv2.resize -> BGR2GRAY -> threshold) for frames the caller
 * holds as array3d images: rgb u8[n,288,512,3] [dev] -> out u8[n,80,80] [dev].  The fused env step
 * never needs it; it exists so that `preprocess(observ)` stays a drop-in. */
int fb_preprocess_rgb(fb_env_t h, const uint8_t *rgb, int n_frames, uint8_t *out, void *stream);

/* ------------------------------------------------------------------ replay memory
 * HBM ring of single frames (1 bit / pixel: preprocess only emits 0 or 255) + per-transition
 * action / reward / terminal; a transition is the 5-frame window (s = t-3..t, s' = t-2..t+1).
 *   deque store / popleft     BrainDQN.py:36,69-72      (REPLAY_MEMORY = 50000, :26)
 *   frame stack               BrainDQN.py:68,238-239    (newest last, never reset)
 *   random.sample             BrainDQN.py:197
 *   minibatch assembly        BrainDQN.py:198-201
 *   SumTree / Memory          BrainPrioritizedReplyDQN.py:32-151
 */
typedef struct fb_replay *fb_replay_t;

#define FB_REPLAY_UNIFORM 0
#define FB_REPLAY_PER 1

#define FB_RNG_CPYTHON 0         /* MT19937 + Lib/random.py: bit-exact random.sample(range(n), B) */
#define FB_RNG_PHILOX 1          /* counter based, with replacement, fully parallel */
#define FB_RNG_NUMPY 2           /* MT19937 legacy np.random.seed(int): Memory.sample's uniform() */

int fb_replay_create(int64_t capacity, int n_envs, int kind, fb_replay_t *out);
int fb_replay_destroy(fb_replay_t h);
int fb_replay_seed(fb_replay_t h, int rng_kind, uint64_t seed);          /* synchronous */
/* setInitState: the first observation becomes all four frames of every env's stack. */
int fb_replay_reset(fb_replay_t h, const uint8_t *frames /*[dev] u8[N,80,80] or NULL*/,
                    const uint64_t *frame_bits /*[dev] u64[N,100] or NULL*/, void *stream);
/* setPerception's store: one transition per env (env order = deque order within a step).
 * Exactly one of frames / frame_bits is given (the NEXT observation).  The handle counts pushes on
 * the host (the kernels receive the step index by value), so a push must not be replayed from a captured
 * hipGraph, and a captured fb_replay_gather / fb_replay_current_state addresses the memory as it was filled at
 * capture time (fine for replaying train steps on a memory that is not being pushed to; sample / train have no
 * such restriction). */
int fb_replay_push(fb_replay_t h, const uint8_t *frames, const uint64_t *frame_bits, const uint8_t *actions,
                   const float *rewards, const uint8_t *terminals, void *stream);
/* fb_replay_push followed by fb_replay_sample(batch) of a uniform memory, in one launch: identical results
 * (the sample depends on the memory's size after the push, not on the pushed data; same RNG consumption),
 * but the single-wave sampler runs beside the copy instead of after it.  idx i64[batch] [dev].  For a
 * prioritized memory or a non-CPython RNG it simply performs the two calls in a row (isw is not returned:
 * use the separate calls for PER). */
int fb_replay_push_sample(fb_replay_t h, const uint8_t *frames, const uint64_t *frame_bits, const uint8_t *actions,
                          const float *rewards, const uint8_t *terminals, int batch, int64_t *idx, void *stream);
/* currentState of every env: u8[N,80,80,4] [dev] (newest frame last). */
int fb_replay_current_state(fb_replay_t h, uint8_t *states, void *stream);
/* Uniform: idx = deque positions (0 = oldest) exactly as random.sample(range(len), B).
 * PER: idx = SumTree tree indices (b_idx of Memory.sample), isw = ISWeights[:,0] (f64),
 *      uniforms = B doubles in [0,1) [dev] replacing np.random.uniform's stream, or NULL. */
int fb_replay_sample(fb_replay_t h, int batch, const double *uniforms, int64_t *idx, double *isw, void *stream);
/* s, s2: u8[B,80,80,4]; a: u8[B]; r: f32[B]; t: u8[B]  (all [dev]) */
int fb_replay_gather(fb_replay_t h, int batch, const int64_t *idx, uint8_t *s, uint8_t *s2, uint8_t *a,
                     float *r, uint8_t *t, void *stream);
/* Measurement aid (bench.py roofline): fb_replay_gather launched `reps` times back to back on `stream`. */
int fb_replay_profile_gather(fb_replay_t h, int batch, const int64_t *idx, uint8_t *s, uint8_t *s2, uint8_t *a, float *r,
                             uint8_t *t, int reps, void *stream);
/* Memory.batch_update(tree_idx, abs_errors): abs_err f32[B] [dev] is updated in place (+= 0.01)
 * like the reference does; priorities_or_null f32[B] [dev] injects the p values instead of
 * computing (min(|e|+0.01, 1))^0.6 on the device. */
int fb_replay_update_priorities(fb_replay_t h, int batch, const int64_t *idx, float *abs_err,
                                const float *priorities_or_null, void *stream);
/* How the SumTree is maintained (prioritized memories only):
 *   FB_PER_EXACT (default) the reference's running sums in the reference's update order: tree bytes and sampled
 *                indices bit-identical to BrainPrioritizedReplyDQN.SumTree (the parity mode); Memory.store of
 *                N envs costs N ordered tree walks
 *   FB_PER_FAST  every touched node recomputed as left + right, level by level: order independent, same values
 *                up to fp64 rounding of the sums, ~20x faster stores for thousands of envs.  Switch only while the
 *                memory is empty or between steps; the tree stays valid in both modes. */
#define FB_PER_EXACT 0
#define FB_PER_FAST 1
int fb_replay_set_per_mode(fb_replay_t h, int mode);
/* Which priority a NEW transition's leaf gets (prioritized memories only):
 *   FB_PER_INIT_MAX (default) the tree's maximum, the reference's Memory.store: a leaf gets a TD-based priority only once it has been
 *                sampled and trained on.  With this setting every call is what it was before the setting existed.
 *   FB_PER_INIT_TD  the |TD error| the actor can form from the Q-values it computed to act (Ape-X, Horgan et al. 2018).  Accepted on a
 *                prioritized memory in FB_PER_FAST with capacity >= n_envs only: the reference has no such operation, so FB_PER_EXACT has
 *                no update order to reproduce.  A uniform memory, a FB_PER_EXACT memory, capacity < n_envs: FB_ERR_INVALID before anything
 *                is allocated.  While it is on, fb_replay_set_per_mode(FB_PER_EXACT) and fb_replay_load_state of a FB_PER_EXACT blob are
 *                FB_ERR_INVALID.  The store itself is unchanged (fb_replay_push writes max_p); the leaves are rewritten one step later by
 * fb_replay_prime_priorities(h, q f32[N,A] [dev], actions u8[N] [dev], n_actions, stream), issued once per step AFTER the acting forward
 *   has produced q = Q(s_S, .) and the actions a_S for the current state (S = pushes since the reset) and BEFORE push S + 1.  In this order:
 *   1. Prime -- only if push S stored N leaves (S >= n) and the record holds rec[t] for their time slot t = S - n.  For env e
 *        y     = done ? R : R + Gamma * max_a q[e,a]      in float64 (product, then sum: no fused multiply-add); (R, done) is the ring's
 *                n-step read of transition (t, e) exactly as fb_replay_gather delivers it (n = 1: the row itself), Gamma = gamma^n as
 *                the running product of the memory's gamma; at n = 1, where the memory holds no discount, the value of
 *                fb_replay_set_prime_gamma (0.99, the reference's GAMMA, until set)
 *        delta = (float)|y - (double)rec[t][e]|
 *        p     = (float)pow((double)min(delta + 0.01f, 1.0f), (double)0.6f)            Memory.batch_update's formula
 *      and the leaf of data slot (data_pointer - N + e) mod capacity -- the leaves push S stored, in env order -- becomes p in the sum,
 *      max and min heaps; every ancestor is recomputed level by level as in FB_PER_FAST.  No atomics and no reductions: the tree is a
 *      function of its leaves alone.  A leaf among them that step S's fb_replay_update_priorities already updated IS OVERWRITTEN by
 *      its acting-time value.  Otherwise (the first n calls after a reset, after a switch of the setting, after fb_replay_load_state
 *      without fb_replay_set_prime_state, after a step without this call) the leaves keep their max_p.
 *   2. Record -- rec[S][e] = q[e, actions[e]] in a ring of n + 1 rows of f32[N] the memory owns (an action >= n_actions raises the
 *      memory's index error, reported by fb_replay_size, and records q[e,0]).
 *   FB_ERR_INVALID: a memory that is not FB_PER_INIT_TD, NULL q / actions, n_actions outside 1..256.
 * fb_replay_set_priority_init and fb_replay_reset clear the record.  fb_replay_get_prime_state / _set_prime_state read and write the
 * record ([host] f32[(n + 1) * N], `floats` must say so) and the two counters first / last (the push counts of the oldest and newest
 * consecutive rows held, -1 / -1 = none); synchronous; with them behind fb_replay_save_state / fb_replay_load_state a checkpoint resumes
 * bit for bit.  The memory's state blob keeps its format.
 * fb_vec_step on a FB_PER_INIT_TD memory issues the call itself (see there). */
#define FB_PER_INIT_MAX 0
#define FB_PER_INIT_TD 1
int fb_replay_set_priority_init(fb_replay_t h, int mode);
int fb_replay_get_priority_init(fb_replay_t h, int *mode_host);
int fb_replay_set_prime_gamma(fb_replay_t h, double gamma);       /* n-step memory: must equal the memory's gamma */
int fb_replay_get_prime_gamma(fb_replay_t h, double *gamma_host);
int fb_replay_prime_priorities(fb_replay_t h, const float *q, const uint8_t *actions, int n_actions, void *stream);
int fb_replay_get_prime_state(fb_replay_t h, float *rows_host, size_t floats, int64_t *first_host, int64_t *last_host);
int fb_replay_set_prime_state(fb_replay_t h, const float *rows_host, size_t floats, int64_t first, int64_t last);
/* n-step returns (Ape-X / R2D2 style) as a different READ of the same ring -- nothing new is stored, the state blob is unchanged.
 * With n steps and discount gamma, transition t of env e (the deque position j of the one-step memory, see below) is
 *   s      frames t-3 .. t of env e (as at n = 1), a = act[t]
 *   R      m = n, or k + 1 for the first k < n with term[t+k] = 1;  R = (float) sum_{k<m} g_k * (double) rew[t+k], summed in ascending k,
 *          g_0 = 1.0, g_{k+1} = g_k * gamma in double (rounded to float once)
 *   done   1 iff some term[t+k] = 1, k < n
 *   s'     frames t+n-3 .. t+n of env e, always (when done the target masks it out)
 *   target y = done ? R : R + Gamma * maxQ'(s') in float64, Gamma = g_n: the one-step formula with (r, term, gamma) -> (R, done, Gamma);
 *          Double / dueling unchanged.
 * Population: after S pushes transition t is complete once frame t+n exists (t <= S-n): the sampleable population is the oldest
 * min(len, cap) - (n-1) * N deque positions, and deque position j names the same transition as at n = 1.  random.sample (CPython
 * generator, bit-exact against random.sample(range(population), B)) and the Philox sampler draw over that population; an index beyond
 * it is an out-of-range index for fb_replay_gather / fb_train_from_replay.  fb_replay_size stays len(memory).
 * Split schedule of fb_vec_step: the only transitions whose data the coming push writes (frame S+1, row S) are those of time slot S+1-n,
 * the NEWEST N positions of the post-push n-step population -- so the gated draw's dirty rule "some index >= population - N" stays exact.
 * fb_replay_set_n_step: uniform memories only, 1 <= n <= FB_NSTEP_MAX, capacity >= n * n_envs; anything else is FB_ERR_INVALID and
 *   changes nothing.  n = 1 restores the one-step memory exactly (gamma is then ignored).  A host-side setting read by the calls issued
 *   after it: a hipGraph captured earlier keeps the value it was captured with.
 * Ring-fed training calls on an n > 1 memory (fb_vec_step, fb_vec_step_dp, fb_train_from_replay, fb_train_steps) take `gamma` = the
 * memory's gamma (anything else is FB_ERR_INVALID before any counter moves or any launch) and bootstrap with Gamma; fb_replay_gather
 * returns (s, a, R, s', done); fb_qnet_train_step on gathered tensors is unchanged -- pass it Gamma.
 * fb_replay_get_n_step: the current (n, gamma) [host] (gamma = 0 at n = 1), for both kinds.
 *
 * Prioritized memories with n-step returns (Ape-X: a prioritized memory fed with COMPLETED transitions).  n is fixed at creation
 * (fb_replay_create_nstep): the ring size and the tree's contents both depend on it from the first push.  N = n_envs, cap = capacity,
 * S = pushes since the last reset.
 *   Stores   push S completes the N transitions of time slot S - n; Memory.store's tree part of push S stores exactly those N leaves
 *            (max priority, env order, the reference's operations, every store path and mode unchanged).  Pushes 1 .. n-1 after a reset
 *            store nothing.  After S pushes the tree has received C = max(0, S - n + 1) * N stores: its bytes, data_pointer, size and
 *            beta are those of the reference's Memory after C store calls (FB_PER_EXACT bit for bit), i.e. those of an n = 1
 *            prioritized memory of the same cap and N after S - n + 1 pushes.
 *   Leaves   leaf d (data slot d) names the newest complete transition living in slot d: g = d + cap * floor((C - 1 - d) / cap),
 *            (t, e) = divmod(g, N); valid iff d < min(C, cap) (an index beyond that raises the memory's error flag as at n = 1).
 *   Reads    as in the uniform n-step view above: (s, a, R, s', done) of transition t, the target bootstrapped with Gamma; importance
 *            weights, beta and batch_update are unchanged (the |TD errors| written back are those of the n-step target).
 *   Population  min(C, cap): the tree always holds up to cap complete transitions (the uniform n-step population is
 *            min(S N, cap) - (n-1) N instead).  fb_replay_size stays len(memory) = min(S N, cap); fb_replay_per_tree's size is min(C, cap).
 *   Ring     cap complete transitions reach n - 1 time slots further back than at n = 1: the ring keeps T_f = ceil(cap / N) + n + 5 time
 *            slots (ceil(cap / N) + 6 at n = 1, as fb_replay_create), (n - 1) * N * 806 bytes more.  The state blob records T_f, so a blob
 *            of a prioritized memory with another n is refused by fb_replay_load_state.
 *   Order    fb_replay_sample before n pushes since the reset is FB_ERR_STATE (the tree is empty), and so is fb_vec_step(train = 1)
 *            or fb_train_from_replay when fewer than n pushes will exist when it samples; both before any launch.
 * fb_replay_create_nstep: fb_replay_create with n-step returns from the start.  Uniform memories: fb_replay_create followed by
 *   fb_replay_set_n_step.  Prioritized memories: the memory above (fb_replay_set_n_step refuses them).  1 <= n <= FB_NSTEP_MAX and
 *   capacity >= n * n_envs, else FB_ERR_INVALID and nothing is allocated.  n = 1 is fb_replay_create exactly (gamma ignored). */
#define FB_NSTEP_MAX 16
int fb_replay_set_n_step(fb_replay_t h, int n, double gamma);
int fb_replay_get_n_step(fb_replay_t h, int *n_host, double *gamma_host);
int fb_replay_create_nstep(int64_t capacity, int n_envs, int kind, int n, double gamma, fb_replay_t *out);
/* host-side queries (synchronous): len(replayMemory); PER: tree copy f64[2*cap-1] [host] */
int fb_replay_size(fb_replay_t h, int64_t *size_host);
int fb_replay_per_tree(fb_replay_t h, double *tree_host, int64_t *data_pointer, int64_t *size, double *beta);
/* Checkpoint of the memory -- what the reference forgets (BrainDQN.py:176-192,227-233 save the network and three scalars; a
 * resumed run observes for OBSERVE steps again).  One opaque [host] blob of fb_replay_state_bytes() bytes holds the frame ring, the
 * action / reward / terminal rows, the counters, the sampler's generator state and the SumTree heaps: after fb_replay_load_state
 * into a memory created with the same capacity / env count / kind, sample / gather / push continue bit for bit.  Synchronous. */
int fb_replay_state_bytes(fb_replay_t h, size_t *bytes_host);
int fb_replay_save_state(fb_replay_t h, void *blob_host, size_t bytes);
int fb_replay_load_state(fb_replay_t h, const void *blob_host, size_t bytes);

/* ------------------------------------------------------------------ Q network
 *   network        BrainDQN.py:119-155 (conv 8x8/4 -> pool -> conv 4x4/2 -> conv 3x3/1 -> fc -> A)
 *   dueling head   BrainDuelingDQN.py:78-86
 *   getAction      BrainDQN.py:99-116
 *   _trainQNetwork BrainDQN.py:195-223, BrainDQNNature.py:149-182, BrainDoubleDQN.py:37-68,
 *                  BrainPrioritizedReplyDQN.py:277-315
 *   Adam           BrainDQN.py:163 (tf.train.AdamOptimizer(1e-6))
 *   target sync    BrainDQNNature.py:107-111,151-152
 * Flat fp32 parameter order = the reference's variable creation order:
 *   W_conv1[8,8,4,32] b[32] W_conv2[4,4,32,64] b[64] W_conv3[3,3,64,64] b[64] W_fc1[1600,FC] b[FC]
 *   then  W_fc2[FC,A] b[A]            (plain)
 *   or    W_v[FC,1] b_v[1] W_a[FC,A] b_a[A]   (dueling)
 *   or    W_fc2[FC,A*N] b[A*N]        (C51, below)
 *   or    W_v[FC,N] b_v[N] W_a[FC,A*N] b_a[A*N]   (dueling C51, below)
 */
typedef struct fb_qnet *fb_qnet_t;

#define FB_ARCH_PLAIN 0
#define FB_ARCH_DUELING 1
#define FB_NET_ONLINE 0
#define FB_NET_TARGET 1
#define FB_ALGO_DQN 0            /* BrainDQN: target from the same net, loss = sum */
#define FB_ALGO_NATURE 1         /* BrainDQNNature: frozen target net, loss = mean */
#define FB_ALGO_DOUBLE 2         /* BrainDoubleDQN.trainQNetwork: argmax online, value target, mean */
#define FB_ALGO_PER 3            /* BrainPrioritizedReplyDQN: target net, mean(ISW * sq), abs_errors */
/* Policy gradient (BrainPolicyGradient.py:96-100; the actor of BrainActorCritic.py:96-100): the net's outputs are LOGITS,
 * loss = mean over N samples of softmax_cross_entropy(logits, action) x weight.  In fb_qnet_train_step: r = the weights (what the
 * reference feeds as tf_rewards / td_error), gamma = N as a double -- a batch larger than 128 (one whole episode) goes in chunks of
 * <= 128 that export their gradient (flat_grad), the caller adds them up and calls fb_qnet_apply_adam once; s2 / t are ignored (pass
 * s / zeros), abs_err / q_target are not meaningful; loss = this chunk's share of the mean.  Not available through fb_vec_step. */
#define FB_ALGO_PG 4

/* ------------------------------------------------------------------ distributional Q-learning (C51, Bellemare, Dabney & Munos 2017)
 * A C51 net (FB_ARCH_C51, fb_qnet_create_c51) has the plain trunk and fc1, then the head  W_fc2[FC, A*N] b[A*N]  (N = n_atoms; column
 * a*N + i is atom i of action a; fb_qnet_init_params: the same truncated-normal weights / 0.01 biases).
 *   support     z_i = v_min + i * dz, dz = (v_max - v_min) / (N - 1), fixed at creation; 2 <= N <= 64, A * N <= 128, v_min < v_max finite
 *   head        logits[b][a][i] = relu(h_fc1[b]) . W[:, a*N + i] + b[a*N + i],  p[b][a][.] = softmax_i(logits[b][a][.]),
 *               Q[b][a] = sum_i z_i p[b][a][i].  fb_qnet_forward / _act / _act_nib / fb_eval_q / fb_eval_run return that Q; acting
 *               and evaluation take its argmax (first maximum) and the plain net's epsilon rule (same Philox draws)
 *   target      a* = argmax_a Q(s', a) of the target net (FB_ALGO_C51) or of the online net (FB_ALGO_C51_DOUBLE, Rainbow); the
 *               distribution p' = p_target(s', a*)
 *   projection  Tz_j = clamp(R + Gamma (1 - done) z_j, v_min, v_max), b_j = (Tz_j - v_min) / dz (then clamped to [0, N-1]),
 *               l = floor(b_j), u = ceil(b_j): m_l += p'_j (u - b_j), m_u += p'_j (b_j - l); when l == u, m_l += p'_j.
 *               Gamma = gamma^n as DESIGN.md section 10 forms it (n-step memories work unchanged)
 *   loss        mean_b -sum_i m_i log_softmax(logits[b][a_b])_i, fp32, targets constant; dLoss/dlogits = (p - m) / B on the taken
 *               action, 0 elsewhere.  abs_err / q_target of fb_qnet_train_step are not written.
 * Accepted: fb_qnet_train_step, fb_train_from_replay, fb_train_steps and fb_vec_step with a UNIFORM memory, 1 <= B <= min(max_batch,
 * 256), any n, fused Adam or flat_grad.  FB_ERR_INVALID before any launch or counter change: a C51 algo on another net or another
 * algo on a C51 net, a prioritized memory (FB_ALGO_C51_PER below takes one), fb_vec_step_dp.  fb_vec_step runs the one-stream schedule with the head as its own launch.
 * fb_qnet_forward_dist: the probabilities p (f32[B][A][N], [dev]) of `which` net for u8 states, 1 <= B <= 3 * max_batch. */
#define FB_ARCH_C51 2
#define FB_ALGO_C51 5
#define FB_ALGO_C51_DOUBLE 6
/* C51 with prioritized replay (Rainbow without dueling / noisy nets).  Two algos of their own: the memory's kind never switches what
 * FB_ALGO_C51 / _DOUBLE do (those keep refusing a prioritized memory).
 *   FB_ALGO_C51_PER        target as FB_ALGO_C51,        a PRIORITIZED memory only
 *   FB_ALGO_C51_DOUBLE_PER target as FB_ALGO_C51_DOUBLE, a PRIORITIZED memory only
 * Support, projection and Gamma = gamma^n exactly as above.  With the importance weights w_b (isw, f32[B], required: the float32 form
 * of Memory.sample's ISWeights, what FB_ALGO_PER reads):
 *   loss        (1/B) sum_b w_b CE_b,  CE_b = -sum_i m_i log p_i(s_b, a_b)  (the reference PER agent's mean(ISW * sq), with CE for sq)
 *   gradient    dLoss/dlogits = ((p - m) / B) * w_b on the taken action, formed in that order: with w = 1 the results are FB_ALGO_C51's
 *               (_DOUBLE's) bit for bit
 *   abs_err[b]  (when non-NULL) the priority max(0, KL_b), KL_b = sum_i [m_i > 0] m_i (log m_i - log p_i) in fp32, no w_b factor (the
 *               Rainbow paper's choice: KL goes to 0 as the fit improves, CE only to H(m) -- up to log 2 for mass split over two atoms).
 *               Memory.batch_update is unchanged, min(err + 0.01, 1)^0.6; early in training KL ~ log N - H(m) (~3 for 51 atoms), so
 *               priorities sit at the clip 1 until the head fits.  q_target is not written.
 * Accepted: fb_qnet_train_step (a C51 net, isw), fb_train_from_replay (isw, a prioritized memory) and fb_vec_step (isw / isw32 / abs_err
 * buffers): FB_ALGO_PER's path there (sample ahead, ring-fed train from 256 envs, batch_update ahead or in line), the head as its own
 * launch, the one-stream schedule.  FB_ERR_INVALID before any launch or counter change: fb_train_steps (no weights), fb_vec_step_dp, a
 * uniform memory, a scalar net, no isw. */
#define FB_ALGO_C51_PER 7
#define FB_ALGO_C51_DOUBLE_PER 8
#define FB_C51_MAX_ATOMS 64
int fb_qnet_create_c51(int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, fb_qnet_t *out);
/* Dueling C51 (the Rainbow paper's dueling distributional head; Rainbow without noisy nets).  A dueling C51 net (FB_ARCH_C51_DUELING,
 * fb_qnet_create_c51_dueling: the same arguments and support checks as fb_qnet_create_c51, made before any allocation) has the plain
 * trunk and fc1, then two heads that read the same h = relu(h_fc1):
 *   value       V_i = h . W_v[:, i] + b_v[i]                                  W_v[FC, N] b_v[N]
 *   advantage   Adv[a][i] = h . W_a[:, a*N + i] + b_a[a*N + i]                W_a[FC, A*N] b_a[A*N] (column a*N + i: atom i of action a)
 *   logits      logits[a][i] = V_i + Adv[a][i] - (1/A) sum_a' Adv[a'][i]
 * Flat order: the trunk, W_fc1 b_fc1, then W_v b_v W_a b_a (FC 512, N 51, A 2: 78 489 head parameters).  fb_qnet_init_params: the same
 * truncated-normal weights, 0.01 for all N entries of b_v and the other biases.  Softmax, Q, acting / evaluation, the target, the
 * projection, the loss, the KL priorities and every entry point are exactly the C51 ones above (all four C51 algos; fb_qnet_is_c51,
 * fb_qnet_get_support and fb_qnet_forward_dist as for a C51 net); refused as for a C51 net: a scalar algo, fb_vec_step_dp, and
 * fb_qnet_create with arch 2 or 3.
 * (The head is linear: the library folds it into an effective C51 head, W_eff[:, a*N + i] = W_v[:, i] + W_a[:, a*N + i] - (1/A)
 * sum_a' W_a[:, a'*N + i], whenever the net's parameters change -- init, load, target sync, every Adam update -- and its gradients
 * unfold from that head's.  The results agree with the formulas above to float rounding, not bit for bit.) */
#define FB_ARCH_C51_DUELING 3
int fb_qnet_create_c51_dueling(int fc_width, int n_actions, int n_atoms, float v_min, float v_max, int max_batch, fb_qnet_t *out);
/* Noisy C51 nets (NoisyNet, Fortunato et al. 2018: with the dueling C51 head, the double target, prioritized replay and n-step returns,
 * full Rainbow).  A noisy net is a C51 (arch 2) or dueling C51 (arch 3) net whose fully connected layers are factorised Gaussian noisy
 * layers: fc1 and every head layer (W_fc2 b for C51; W_v b_v and W_a b_a, two separate layers, for dueling C51).  The conv trunk stays
 * deterministic.  Made by fb_qnet_create_c51_noisy (arch 2 or 3, the support checks of fb_qnet_create_c51, sigma0 finite and >= 0; all
 * before any allocation).
 *   layer       y = (mu_W + sigma_W (.) (f(eps_out) x f(eps_in))) . x + mu_b + sigma_b (.) f(eps_out),  f(z) = sign(z) sqrt|z|
 *               (W[in][out] as everywhere here: sigma_W[i][j] multiplies f(eps_in_i) f(eps_out_j)); eps_in has fan_in entries, eps_out fan_out
 *   layout      the flat vector (fb_qnet_num_params, load / store_params, flat_grad, fb_qnet_apply_adam, the Adam state, fb_qnet_sync_target)
 *               is [mu | sigma]: mu in the net's C51 / dueling C51 layout above, unchanged, then sigma in the same tensor order from W_fc1
 *               on (sigma_W_fc1 sigma_b_fc1, then the sigma of each head tensor): sigma of mu entry q sits at n_mu + q - 77984
 *               (n_mu = the non-noisy net's count; FC 512, 51 atoms, A 2: 950 022 + 872 038 for C51, 976 185 + 898 201 for dueling C51)
 *   init        fb_qnet_init_params: mu exactly as the non-noisy net's (the same Philox draws), then sigma = sigma0 / sqrt(fan_in) for the
 *               weights and the biases of each layer (fan_in 1600 for fc1, FC for the head layers), in float64 rounded to float
 *   noise       each net (online 0, target 1) holds a current sample: the vector f(eps) of nz floats, per layer in the order above f(eps_in)
 *               [fan_in] then f(eps_out)[fan_out] (nz = 1600 + FC + FC + A*N for C51, 1600 + FC + FC + N + FC + A*N for dueling C51: 2 726 and 3 289
 *               at FC 512, 51 atoms, A 2).
 *               FB_NOISE_SAMPLE at (seed, step): element k of net w is z = sqrt(-2 log u1) cos(2 pi u2) (no truncation; fp32 logf / cosf),
 *               u1 = ((r.x >> 8) + 1) / 2^24, u2 = (r.y >> 8) / 2^24, r = Philox4x32-10(key = (seed_lo, seed_hi), counter = (k, step_lo,
 *               FB_STREAM_NOISE = 6, 2 step_hi + w)), stored as f(z); the online and target nets draw independent vectors for the same key.
 *               FB_NOISE_MEAN: every element 0, so the effective weights are mu exactly.  A new net is in mean mode.  Only
 *               fb_qnet_reset_noise and fb_vec_step change a sample; forward, act, act_nib, forward_dist, fb_eval_q, fb_eval_run,
 *               fb_qnet_train_step and fb_train_from_replay use the current one and never resample.  fb_qnet_get_noise copies a net's
 *               current f(eps) (nz floats, host or device memory; synchronous).  Init, load, sync and Adam keep each net's sample.
 *   gradient    G = the loss gradient of the effective weights: d/dmu = G, d/dsigma_W[i][j] = G[i][j] f(eps_in_i) f(eps_out_j),
 *               d/dsigma_b[j] = G_b[j] f(eps_out_j); TF Adam with the net's hyper-parameters updates all of [mu | sigma].  The online
 *               prediction and the double target's a* use the online net's sample, the target distribution the target net's sample.
 *   fb_vec_step on a noisy net: before acting, fb_qnet_reset_noise(net 0, seed, step); before the train step (train != 0),
 *               fb_qnet_reset_noise(net 1, seed, step); acting and the train step of the call share the online sample (one sample per
 *               net per step for all envs, not one per env); epsilon-greedy as passed (0 for Rainbow).  Bit for bit the composed calls
 *               reset_noise(0) -> act_nib -> env step (+ push / sample) -> reset_noise(1) -> train, for all four C51 algos, both memories, any n.
 *   refused     FB_ERR_INVALID before any launch or counter change: a scalar arch, fb_vec_step_dp, fb_train_steps (no per-step noise key);
 *               fb_qnet_reset_noise / fb_qnet_get_noise on a net that is not noisy.  (The TF bundle export refuses it in Python.)
 * (The library keeps an effective vector mu + sigma (.) noise per net, rebuilt after every change of mu, sigma or the noise -- init, load,
 * sync, Adam, reset -- which every forward and backward kernel reads; sigma's gradient is formed from the effective one's.) */
#define FB_NOISE_SAMPLE 0
#define FB_NOISE_MEAN 1
int fb_qnet_create_c51_noisy(int arch, int fc_width, int n_actions, int n_atoms, float v_min, float v_max, float sigma0, int max_batch,
                             fb_qnet_t *out);
int fb_qnet_is_noisy(fb_qnet_t h);                                                      /* 1: a noisy net, 0: not (or NULL) */
int fb_qnet_reset_noise(fb_qnet_t h, int which, uint64_t seed, uint64_t step, int mode, void *stream);
int fb_qnet_get_noise(fb_qnet_t h, int which, float *out);
/* Per-env acting noise (noisy nets only).  The default, FB_ACT_NOISE_SHARED, is the behaviour above: acting reads the online net's
 * current sample, one for all envs.  FB_ACT_NOISE_PER_ENV draws independent noise per env when acting; training is the same in both modes.
 *   acting      for env (row) e, Q comes from the weights mu + sigma (.) (f(eps_out_e) x f(eps_in_e)) on fc1 and on every head layer (W_fc2 b
 *               for C51; W_v b_v and W_a b_a, separately, for dueling C51), the layer formula, f, the per-layer order (f(eps_in)[fan_in] then
 *               f(eps_out)[fan_out]) and nz of the shared sample; the conv trunk stays deterministic.  Softmax, Q, argmax (first maximum) and
 *               epsilon (the same FB_STREAM_EPS draws) are the C51 head's.
 *   draw        element k of env e at (seed, step): z and f(z) formed as FB_NOISE_SAMPLE's from r = Philox4x32-10(key = (seed_lo, seed_hi),
 *               counter = (e nz + k, step_lo, FB_STREAM_ENV_NOISE = 7, step_hi)); the online net only (no target-net draws).  n nz >= 2^32
 *               is refused (more than ~1.3 M envs).
 *   mu, sigma   from the master vector [mu | sigma].  The call never reads the net's current sample and leaves both nets' samples,
 *               effective vectors, folded heads, parameters and Adam state as they were.
 *   where       each noise term is added after the mu sum it perturbs: fc1 unit j = relu((sum of the mu partials + b_j) + f(eps_out_j)
 *               (t_j + sigma_b_j)), t_j = sum_k sigma_W[k][j] f(eps_in_k) x_k; a head logit = (the mu logit) + its noise term, for
 *               dueling C51 V_n + A_n - mean_a A_n per atom.  With sigma = 0, per-env acting is acting in mean mode bit for bit.
 *   refused     FB_ERR_INVALID before any launch or counter change: a net that is not noisy, a bad mode, per-env mode with
 *               FB_DTYPE_BF16 inference (fb_qnet_act_nib_env_noise and fb_vec_step).
 *   fb_qnet_act_nib_env_noise: fb_qnet_act_nib's arguments and n range (1 <= n <= 3 max_batch), q f32[n][A] or NULL.
 *   fb_vec_step on a noisy net in FB_ACT_NOISE_PER_ENV mode: bit for bit the composed calls fb_qnet_act_nib_env_noise(seed, step) ->
 *               env step (+ push / sample) -> reset_noise(0, FB_NOISE_SAMPLE, seed, step) -> (train != 0) reset_noise(1, ...) -> train, for
 *               all four C51 algos, both memories, any n: the step still leaves the online sample (seed, step) in place.
 *   fb_qnet_set_acting_noise sets the mode fb_vec_step reads (a net starts in FB_ACT_NOISE_SHARED); fb_eval_run is not affected. */
#define FB_ACT_NOISE_SHARED 0
#define FB_ACT_NOISE_PER_ENV 1
int fb_qnet_set_acting_noise(fb_qnet_t h, int mode);
int fb_qnet_act_nib_env_noise(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                              uint8_t *actions, float *q, void *stream);
int fb_qnet_get_support(fb_qnet_t h, int *n_atoms_host, float *v_min_host, float *v_max_host);      /* n_atoms = 0: not a C51 net */
int fb_qnet_forward_dist(fb_qnet_t h, int which, const uint8_t *states, int batch, float *probs, void *stream);

/* ------------------------------------------------------------------ quantile regression (QR-DQN, Dabney, Rowland, Bellemare & Munos 2018)
 * A QR net keeps the plain trunk and fc1; its head has the C51 head's shape (N = n_quantiles, column a*N + i is quantile i of action a):
 *   FB_ARCH_QR          W_fc2[FC, A*N] b[A*N]
 *   FB_ARCH_QR_DUELING  W_v[FC, N] b_v[N] W_a[FC, A*N] b_a[A*N]; theta[a][i] = V_i + Adv[a][i] - (1/A) sum_a' Adv[a'][i], as dueling C51
 * 2 <= N <= 64, A * N <= 128, kappa finite and > 0, all checked by fb_qnet_create_qr before any allocation.  fb_qnet_init_params makes the
 * same draws as the C51 net of the same shape and seed (equal parameters bit for bit).
 *   quantiles   theta[b][a][i] = relu(h_fc1[b]) . W[:, a*N + i] + b[a*N + i] (through the folded head for the dueling form)
 *   midpoints   tau_i = (2i + 1) / (2N)
 *   Q           Q[b][a] = (1/N) sum_i theta[b][a][i]: what fb_qnet_forward / _act / _act_nib / fb_eval_q / fb_eval_run return; acting and
 *               evaluation take its first maximum and the plain net's epsilon rule (same Philox draws)
 *   target      a* = argmax_a Q(s', a) of the target net (FB_ALGO_QR) or of the online net (FB_ALGO_QR_DOUBLE); the quantiles always come
 *               from the target net: T_j = R + Gamma (1 - done) theta_target(s', a*)_j.  No clamp, no projection; Gamma = gamma^n as DESIGN.md
 *               section 10 forms it (n-step memories work unchanged)
 *   loss        u_ij = T_j - theta_i (the taken action a_b, targets constant), L_k(u) = u^2 / 2 if |u| <= k else k (|u| - k / 2),
 *               rho_ij = |tau_i - 1{u_ij < 0}| L_k(u_ij) / k, l_b = (1/N) sum_i sum_j rho_ij, loss = mean_b l_b in fp32
 *   gradient    dl_b/dtheta_i = -(1/N) sum_j |tau_i - 1{u_ij < 0}| clamp(u_ij, -k, k) / k on the taken action (0 elsewhere), divided by B.
 *               Lane i sums over j = 0 .. N-1 in that order: deterministic, no atomics.  abs_err / q_target are not written (uniform algos).
 *   worked case N = 2, k = 1, theta = [0, 1], T = [0.5, 3]: l = 0.90625, dl/dtheta = [-0.1875, -0.3125]
 *   prioritized FB_ALGO_QR_PER (target as FB_ALGO_QR) and FB_ALGO_QR_DOUBLE_PER (target as _DOUBLE) take a prioritized memory and isw only:
 *               loss = (1/B) sum_b w_b l_b; gradient = (that of l_b / B) * w_b, formed in that order (w = 1 gives the uniform algo's results
 *               bit for bit); abs_err[b] = l_b, without the weight (>= 0).  Memory.batch_update is unchanged.
 * FB_ALGO_QR / _DOUBLE take a uniform memory only.  The target net syncs as for C51.  Every entry point that takes a C51 net takes a QR
 * net with a QR algo, but for these: FB_ERR_INVALID before any launch or counter change for a QR algo on another net or another algo on a
 * QR net, fb_vec_step_dp, fb_qnet_forward_dist, noisy / per-env acting noise calls; fb_qnet_create refuses archs 4 and 5;
 * fb_qnet_get_support reports n_atoms = 0.
 * fb_qnet_get_quantiles: N and kappa of a QR net (n = 0 for any other net).  fb_qnet_forward_quantiles: theta (f32[B][A][N], [dev]) of
 * `which` net for u8 states, 1 <= B <= 3 * max_batch. */
#define FB_ARCH_QR 4
#define FB_ARCH_QR_DUELING 5
#define FB_ALGO_QR 9
#define FB_ALGO_QR_DOUBLE 10
#define FB_ALGO_QR_PER 11
#define FB_ALGO_QR_DOUBLE_PER 12
int fb_qnet_create_qr(int arch, int fc_width, int n_actions, int n_quantiles, float kappa, int max_batch, fb_qnet_t *out);
int fb_qnet_get_quantiles(fb_qnet_t h, int *n_quantiles_host, float *kappa_host);
int fb_qnet_forward_quantiles(fb_qnet_t h, int which, const uint8_t *states, int batch, float *theta, void *stream);

/* ------------------------------------------------------------------ Munchausen-DQN (Vieillard, Pietquin & Geist, NeurIPS 2020)
 * Two algos on the SCALAR heads (FB_ARCH_PLAIN and FB_ARCH_DUELING; the dueling combine happens before anything below): the Q head, the
 * squared TD loss, epsilon-greedy acting and evaluation are FB_ALGO_NATURE's; only the target differs.  With the net's parameters
 * (tau, alpha, l0) and, for a vector x with m = max_c x_c,  lse_tau(x) = m + tau log sum_c exp((x_c - m) / tau):
 *   forward     q(s, .) from the online net; q-(s, .) and q-(s', .) from the TARGET net: three slices, s online, s' target, s target
 *   bonus       alpha max(tau ln pi-(a|s), l0),  tau ln pi-(a|s) = (q-(s, a) - m) - tau log sum_c exp((q-(s, c) - m) / tau)  (<= 0), m = max q-(s, .)
 *   V           lse_tau(q-(s', .))  (= sum_c pi-(c|s') (q-(s', c) - tau ln pi-(c|s')), pi- = softmax(q- / tau))
 *   target      y = (R + bonus) + (done ? 0 : Gamma V): bonus and V in fp32 (expf / logf), R and the sums in float64 as the other scalar
 *               algos form theirs (R = 0.1f reads as 0.1), rounded to float once.  The bonus is added on terminal transitions too.
 *               Gamma = gamma^n as DESIGN.md section 10 forms it; on an n-step memory R is the n-step return and ONLY THE FIRST step's
 *               bonus (that of (s, a)) is added -- the memory stores no state between s and s' to form the others from
 *   loss        mean_b w_b (y_b - q(s_b, a_b))^2, the gradient through q(s, a) only: exactly FB_ALGO_NATURE's (FB_ALGO_MDQN, w = 1) or
 *               FB_ALGO_PER's (FB_ALGO_MDQN_PER, w = isw) with this y; abs_err = |y - q(s, a)|, q_target = y
 *   A = 1       lse_tau(x) = x + tau log(1) = x and the bonus is alpha max(0 - tau log(1), l0) = 0: FB_ALGO_MDQN on a one-action net gives
 *               FB_ALGO_NATURE's loss, y and gradient bit for bit
 *   worked      tau 0.03, alpha 0.9, l0 -1: q-(s) = (c, c) -> bonus -alpha tau ln 2 = -0.018715...; q-(s) = (0, 2) -> -0.9 for a = 0
 *               (clipped), -0 for a = 1
 * FB_ALGO_MDQN takes a uniform memory, FB_ALGO_MDQN_PER a prioritized one and isw, as FB_ALGO_PER does.  FB_ALGO_MDQN is accepted
 * wherever FB_ALGO_DOUBLE is (fb_qnet_train_step, fb_train_from_replay, fb_train_steps, fb_vec_step on the schedule FB_ALGO_DOUBLE takes
 * at that shape, flat_grad, fb_vec_step_dp, FB_DTYPE_BF16 training), FB_ALGO_MDQN_PER wherever FB_ALGO_PER is.  FB_ERR_INVALID before any
 * launch or counter change: these algos on a C51 / QR / noisy net (and a C51 / QR algo on a scalar net, as before), a prioritized memory
 * for FB_ALGO_MDQN, a uniform memory or no isw for FB_ALGO_MDQN_PER.  The target net syncs as for FB_ALGO_NATURE (the caller's call).
 * fb_qnet_set_munchausen: the net's (tau, alpha, l0); a new scalar net holds (0.03, 0.9, -1), the paper's.  FB_ERR_INVALID before
 *   anything changes: tau not finite or <= 0, alpha outside [0, 1], l0 not finite or > 0, a C51 / QR net.  A host-side setting read by
 *   the calls issued after it (a hipGraph captured earlier keeps the values it was captured with).
 * fb_qnet_get_munchausen: the current values [host] (any of the pointers may be NULL); FB_ERR_INVALID on a C51 / QR net. */
/* (13 is no algo and stays refused as unknown by every entry point: callers and tests have used it as the first number past the QR algos) */
#define FB_ALGO_MDQN 14
#define FB_ALGO_MDQN_PER 15
int fb_qnet_set_munchausen(fb_qnet_t h, float tau, float alpha, float clip_lo);
int fb_qnet_get_munchausen(fb_qnet_t h, float *tau_host, float *alpha_host, float *clip_lo_host);

/* ------------------------------------------------------------------ Huber (clipped-error) loss and Double-DQN with prioritized replay
 * Two additions to the SCALAR heads (FB_ARCH_PLAIN and FB_ARCH_DUELING), both on the target / loss side alone: the forward, the dueling
 * combine, acting, evaluation and everything behind dLoss/dq(s, a) (fc1 / conv backward, Adam) are what they were.
 *
 * Huber loss: a per-net setting, delta (fb_qnet_set_huber).  A new scalar net holds delta = 0 = off: the squared TD loss of the algos
 * above, through the kernels of before the setting existed.  delta finite and > 0 turns it on for FB_ALGO_DQN, _NATURE, _DOUBLE, _PER,
 * _MDQN, _MDQN_PER and _DOUBLE_PER, in fb_qnet_train_step, fb_train_from_replay, fb_train_steps, fb_vec_step (both schedules),
 * fb_vec_step_dp, with flat_grad and in FB_DTYPE_BF16 training.  With d = y - q(s, a) and w the importance weight (1 for the uniform algos):
 *   loss term   w l(d),  l(d) = d^2 for |d| <= delta, else delta (2 |d| - delta): TWICE the textbook Huber loss, so that it IS the d^2 of
 *               the squared loss inside the zone; value and slope are continuous at |d| = delta (delta^2 and 2 delta).  Formed in fp32 as
 *               (w * d) * d inside, w * (delta * (2 |d| - delta)) outside; summed (FB_ALGO_DQN) or averaged over the batch as before
 *   gradient    dLoss/dq(s, a) = -scale w clamp(d, -delta, delta), scale as before (2 for FB_ALGO_DQN's sum, 2 / B for the means), formed as
 *               ((-scale) * w) * clamp: for |d| <= delta (|d| = delta included: the quadratic branch) loss term and gradient are bit for
 *               bit the squared loss's, and so delta = 1e30 gives the results of delta = 0
 *   abs_err     |d|, NOT clipped (the prioritized memory clips its priorities itself); q_target = y, unchanged
 *   worked      delta 1, B 2, a mean loss, d = (0.5, -3): terms (0.25, 5), loss 2.625, dLoss/dq = (-0.5, +1.0)
 * fb_qnet_set_huber: FB_ERR_INVALID before anything changes: delta NaN, infinite or < 0; a C51 / QR / noisy net (QR has its own kappa).
 *   A host-side setting read by the calls issued after it (a hipGraph captured earlier keeps the value it was captured with).
 * fb_qnet_get_huber: the current delta [host]; FB_ERR_INVALID on a C51 / QR / noisy net.
 * FB_ALGO_PG has no TD error: on a net whose delta is > 0 it is refused (FB_ERR_INVALID) before anything is launched.
 *
 * FB_ALGO_DOUBLE_PER: Double-DQN's target on a prioritized memory ("Rainbow minus the distributional head" with FB_ARCH_DUELING and
 * n-step returns).
 *   forward     three slices as FB_ALGO_DOUBLE: s online, s' online, s' target
 *   target      a* = the FIRST maximum of the online net's q(s', .) (a later action wins only if strictly greater), y = R + (done ? 0 :
 *               Gamma q-(s', a*)), formed exactly as FB_ALGO_DOUBLE forms it: float64 sums, R = 0.1f read as 0.1, rounded to float once
 *   loss        mean_b isw_b l(d_b), gradient, abs_err = |d| and q_target = y exactly as FB_ALGO_PER with that y
 *   hence       with isw == 1 its loss, y and gradient are FB_ALGO_DOUBLE's bit for bit; on a one-action net (a* = 0, target net's value)
 *               everything is FB_ALGO_PER's bit for bit
 * Accepted wherever FB_ALGO_PER is: a prioritized memory (n-step ones included) and isw only, fb_qnet_train_step, fb_train_from_replay,
 * fb_vec_step on FB_ALGO_PER's schedule (sample ahead on the memory's side stream, ring-fed training from 256 envs), flat_grad,
 * fb_vec_step_dp, FB_DTYPE_BF16 training.  FB_ERR_INVALID before any launch or counter change, as for FB_ALGO_PER: fb_train_steps,
 * a uniform memory, no isw, a C51 / QR / noisy net.  The target net syncs as for FB_ALGO_DOUBLE (the caller's call). */
/* (16 is the next number after the Munchausen algos; 13 stays no algo) */
#define FB_ALGO_DOUBLE_PER 16
int fb_qnet_set_huber(fb_qnet_t h, float delta);
int fb_qnet_get_huber(fb_qnet_t h, float *delta_host);

/* ------------------------------------------------------------------ global-norm gradient clipping and soft (Polyak) target updates
 * Two optimiser-side settings, both off in a new net; with them off every path, kernel and result is what it was.
 *
 * Clipping (tf.clip_by_global_norm; the dueling paper, Rainbow and QR-DQN clip to 10): a per-net limit G (fb_qnet_set_max_grad_norm).
 *   norm        sqrt(sum_q g[q]^2) over the WHOLE flat gradient (fb_qnet_num_params floats: every tensor of the flat order, for a noisy net
 *               sigma's part included).  Squares and sums in float64, in a fixed order (a fixed grid, per-thread strides, a fixed tree per
 *               workgroup, the workgroups' partials in a fixed tree; no atomics): two calls on equal gradients give equal bits.  The sum's
 *               square root is rounded to fp32 once
 *   scale       c = G / max(norm, G) in fp32 from that norm, g[q] <- g[q] * c.  norm <= G: c is exactly 1.0f and nothing is stored, the
 *               gradient stays bit for bit.  A norm that is not finite (an inf or NaN entry): c = 1, the gradient goes on as it would
 *               without clipping and the recorded norm shows it.  G = 0: the norm is computed and recorded, the gradient untouched (the
 *               diagnostic use: fb_qnet_clip_grad on an exported gradient of a net that does not clip)
 *   worked      g = (3, 4), G = 2.5: norm 5, c 0.5, g <- (1.5, 2)
 * fb_qnet_set_max_grad_norm: G = 0 (a new net) off, finite G > 0 on; negative, NaN or infinite: FB_ERR_INVALID before anything changes.
 *   Every arch.  A host-side setting read by the calls issued after it (a hipGraph captured earlier keeps the value it was captured with).
 * fb_qnet_clip_grad: the two launches above on flat_grad ([dev] f32[fb_qnet_num_params], 16-byte aligned, in place) with the net's G, on
 *   `stream`; capturable.  The net keeps (norm, c) of its last call in two device words.
 * fb_qnet_grad_norm: those two words [host] (either pointer may be NULL); SYNCHRONOUS, for the log cadence.  (0, 1) before any clip.
 * Where a net with G > 0 clips:
 *   flat_grad == NULL   fb_qnet_train_step, fb_train_from_replay, fb_vec_step: the step runs as the exporting step into the net's own
 *                       gradient buffer, then fb_qnet_clip_grad, then fb_qnet_apply_adam's launch: parameters, both Adam slots and the beta
 *                       powers are those of the three public calls composed by hand, bit for bit; loss / abs_err / q_target are the
 *                       (unclipped) step's.  The fused chain's in-launch Adam (W_fc1's span in the conv backward, the slab-summing Adam
 *                       launch) is not taken
 *   flat_grad != NULL   the gradient is exported UNCLIPPED, as before: the caller reduces it, then clips (fb_qnet_clip_grad) or hands it
 *                       to fb_dist_reduce_apply / fb_vec_step_dp, which clip behind the reduction and the averaging, before Adam
 *   fb_vec_step         takes the one-stream order (as for C51 / QR nets); the split schedule's Adam hand-over is never armed
 *   fb_train_steps      FB_ERR_INVALID before any launch or counter change (as for a noisy net)
 *   FB_ALGO_PG          callers sum their chunk gradients and call fb_qnet_apply_adam: they clip the sum with fb_qnet_clip_grad first
 *   fb_qnet_apply_adam  never clips by itself.
 *
 * Soft target update: fb_qnet_soft_sync_target(rho): target <- target + rho * (online - target) in fp32 (formed in that order, no fused
 * multiply-add) over the vector fb_qnet_sync_target copies ([mu | sigma] of a noisy net), one launch.
 *   rho         in (0, 1]; 0, negative, > 1 or NaN: FB_ERR_INVALID before any launch.  rho == 1 IS fb_qnet_sync_target (bit-identical)
 *   afterwards  on `stream`, everything derived from the target's parameters is rebuilt from the NEW values, as fb_qnet_load_params does
 *               (not copied from the online net): W_conv1's fp16 planes, a new parameter version, a noisy net's effective vector with the
 *               target's own current sample, the split planes, a dueling distributional net's folded head.  The online net, both noise
 *               samples and the Adam state are untouched.  Every arch; capturable. */
int fb_qnet_set_max_grad_norm(fb_qnet_t h, float g);
int fb_qnet_get_max_grad_norm(fb_qnet_t h, float *g_host);
int fb_qnet_clip_grad(fb_qnet_t h, float *flat_grad, void *stream);
int fb_qnet_grad_norm(fb_qnet_t h, float *norm_host, float *scale_host);
int fb_qnet_soft_sync_target(fb_qnet_t h, float rho, void *stream);

/* ------------------------------------------------------------------ advantage actor-critic (A2C, Mnih et al. 2016, synchronous form)
 * The on-policy learner of the vectorised loop: N envs make T steps with the current policy, and ALL T N fresh transitions train one
 * update.  (The reference's BrainPolicyGradient / BrainActorCritic are one env, one episode, a critic that is a second network trained
 * online at batch 1: FB_ALGO_PG stands behind those.  This is the batched algorithm, with a shared trunk.)
 * An AC net (FB_ARCH_AC, fb_qnet_create_ac) has the trunk and fc1 of every net and the DUELING net's head parameters, layout and order,
 *   W_v[FC,1] b_v[1] W_pi[FC,A] b_pi[A]   (fb_qnet_num_params and fb_qnet_init_params' draws are the dueling net's of that shape)
 * read RAW, with h = relu(h_fc1):  V(s) = h . W_v + b_v,  logits z(s) = h . W_pi + b_pi.  There is no dueling combine.
 *   acting      fb_qnet_forward / _act / _act_nib / fb_eval_run / fb_eval_q treat the LOGITS as the Q values (the plain head over W_pi b_pi):
 *               greedy play is the policy's argmax, epsilon as for a plain net.  fb_qnet_forward_ac returns (z, V) -- z the very bits
 *               fb_qnet_forward returns.  The target net (FB_NET_TARGET) exists and is unused by A2C
 *   policy      float32, ascending c:  m = max_c z_c, e_c = expf(z_c - m), p_c = e_c / sum e,  log p_c = z_c - (m + logf(sum e))
 *   sampling    fb_qnet_act_policy_nib, row r at (seed, step): u = (o.x >> 8) * 2^-24, o = Philox4x32-10(key = (seed_lo, seed_hi), counter =
 *               (r, step_lo, FB_STREAM_POLICY = 8, step_hi)); the action is the smallest c with u < sum_{c' <= c} p_c' (a running float32 sum),
 *               A - 1 if there is none; logp = log p_a.  greedy != 0: the first maximum of z, no draw.  A = 1: action 0, logp 0
 *   advantages  fb_ac_gae (generalised advantage estimation, Schulman et al. 2016) over reward f32[T,N], terminal u8[T,N], value f32[T+1,N]
 *               (row T: the bootstrap V(s_T)), per env, t = T-1 .. 0, everything in double:
 *                 r = (rew == 0.1f) ? 0.1 : (double)rew   (the convention of every target here);  nd = !terminal[t]
 *                 x = nd ? gamma * (double)v[t+1] : 0;  delta = (r + x) - (double)v[t];  A = delta + (nd ? gl * A : 0),  gl = gamma * lambda
 *                 adv[t] = (float)A;  ret[t] = (float)(A + (double)v[t])
 *               0 <= gamma, lambda <= 1.  lambda = 1: the discounted return less V; lambda = 0: the one-step TD error
 *   loss        per sample b of a chunk, N_tot = n_total (the whole update's sample count), c_v / c_e the net's coefficients, fp32:
 *                 L_pi = -adv_b log p_{a_b}   (adv is a constant)      L_v = (V_b - ret_b)^2      H = -sum_c p_c log p_c
 *                 loss = (1 / N_tot) sum_b (L_pi + c_v L_v - c_e H)
 *                 dLoss/dz_c = (adv_b (p_c - 1{c = a_b}) + c_e p_c (log p_c + H)) / N_tot       dLoss/dV = (2 c_v (V_b - ret_b)) / N_tot
 *               loss[0..3] = the chunk's share of {total, sum L_pi / N_tot, sum L_v / N_tot, sum H / N_tot}; sums over b in ascending order,
 *               no atomics: equal inputs give equal bits
 *   training    fb_qnet_ac_train_step on gathered states, fb_ac_train_from_replay on ring positions (the ring-fed trunk; a UNIFORM memory
 *               at n-step 1; a_out receives the ring's actions): 1 <= batch <= min(max_batch, 256), n_total >= batch.  flat_grad NULL:
 *               Adam at once (with the net's gradient clipping, as fb_qnet_train_step).  flat_grad != NULL: the chunk's gradient is
 *               exported only -- the caller sums the chunks of an update, clips the sum with fb_qnet_clip_grad if it wants, and calls
 *               fb_qnet_apply_adam once, as FB_ALGO_PG callers do.  s is forwarded once (one slice)
 *   rollout     the replay ring is the rollout's state store: after T fb_ac_rollout_step calls the newest T N deque positions,
 *               idx = len - T N + k, are the transitions in the order of the flattened [T,N] buffers (position j -> g = total - size + j,
 *               (t, e) = divmod(g, N)).  fb_ac_rollout_step(slot) = fb_qnet_act_policy_nib (value / logp written at row `slot`) ->
 *               fb_env_step (reward / terminal written at row `slot`) -> fb_replay_push: three calls in that order on `stream`,
 *               their results bit for bit.  No riders, no split schedule.  It pushes: not capturable for replay, like fb_vec_step
 *   refused     FB_ERR_INVALID before any launch or counter change: on an AC net every FB_ALGO_* of fb_qnet_train_step / fb_train_from_replay /
 *               fb_train_steps / fb_vec_step / fb_vec_step_dp, fb_qnet_set_huber / _get_huber, fb_qnet_set_munchausen / _get_munchausen,
 *               FB_DTYPE_BF16 for inference or training; fb_qnet_create with arch 6 and fb_qnet_create_c51_noisy with it (no noisy AC net);
 *               every fb_qnet_*_ac / fb_ac_* call below on a net that is not an AC net.
 *   not offered data-parallel A2C, bf16, riders or the split schedule for the rollout step, noisy or distributional critics.  (PPO on the
 *               same rollout: the block below.)
 * fb_qnet_set_ac / fb_qnet_get_ac: (c_v, c_e), 0.5 and 0.01 in a new net; both finite and >= 0.  A host-side setting read by the calls issued
 *   after it. */
#define FB_ARCH_AC 6
typedef struct {
    uint8_t *nib;                                   /* u8[N,FB_NIB_STRIDE]: the buffer given to fb_env_set_nib_buffer */
    uint8_t *actions;                               /* u8[N] out */
    uint64_t *frame_bits;                           /* u64[N,100] out */
    float *reward; uint8_t *terminal;               /* f32[slots,N], u8[slots,N]: row `slot` out */
    int32_t *score;                                 /* i32[N] out */
    float *value, *logp;                            /* f32[slots (+1),N], f32[slots,N]: row `slot` out */
    int slots;                                      /* rows of reward / terminal / value / logp (the rollout length T) */
} fb_ac_rollout_buffers;
int fb_qnet_create_ac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out);
int fb_qnet_set_ac(fb_qnet_t h, float value_coef, float entropy_coef);
int fb_qnet_get_ac(fb_qnet_t h, float *value_coef_host, float *entropy_coef_host);
/* states u8[B,80,80,4] -> logits f32[B,A], value f32[B]; 1 <= B <= 3 * max_batch; the online net */
int fb_qnet_forward_ac(fb_qnet_t h, const uint8_t *states, int batch, float *logits, float *value, void *stream);
/* the acting forward of fb_qnet_act_nib (the small-batch kernels below 256 states, the fused trunk from 256 on), then the policy head as
 * a launch of its own.  actions u8[n] or NULL (NULL: logits / value only, no draw), value f32[n], logp f32[n] or NULL, logits f32[n,A] or NULL */
int fb_qnet_act_policy_nib(fb_qnet_t h, const uint8_t *nib_states, int n, uint64_t seed, uint64_t step, int greedy, uint8_t *actions,
                           float *value, float *logp, float *logits, void *stream);
int fb_ac_gae(const float *reward, const uint8_t *terminal, const float *value, int T, int N, double gamma, double lambda, float *adv,
              float *ret, void *stream);
int fb_qnet_ac_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret, int64_t n_total,
                          float *loss, float *flat_grad, void *stream);
int fb_ac_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *adv, const float *ret,
                            int64_t n_total, uint8_t *a_out, float *loss, float *flat_grad, void *stream);
int fb_ac_rollout_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_ac_rollout_buffers *b, int n_envs, uint64_t seed,
                       uint64_t step, int slot, void *stream);

/* ------------------------------------------------------------------ PPO (Schulman et al. 2017) on the actor-critic rollout
 * The clipped-surrogate update on an AC net: the rollout, V(s_T) and fb_ac_gae as for A2C, then K epochs of shuffled minibatches over the
 * SAME T N transitions, each an Adam step.  One GPU, fp32, a uniform memory at n-step 1, as A2C.  z, V, p, log p, H are formed exactly
 * as in the A2C block; a is the batch's action (the ring's in the ring-fed call); an action >= A reads action A - 1.
 *   settings    fb_qnet_set_ppo / fb_qnet_get_ppo: (clip_eps, value_clip), 0.2 and 0 in a new AC net; clip_eps finite and > 0, value_clip
 *               finite and >= 0 (0 = the value term is not clipped).  Host-side settings read by the calls issued after them, like
 *               fb_qnet_set_ac, whose (c_v, c_e) PPO reads too
 *   loss        per sample b of a chunk, N_tot = n_total (the MINIBATCH's sample count), fp32, eps = clip_eps:
 *                 lr = log p_a - logp_old      r = expf(lr)      lo = 1 - eps      hi = 1 + eps
 *                 s1 = r adv      s2 = fminf(fmaxf(r, lo), hi) adv      L_pi = -fminf(s1, s2)      w = (s1 <= s2) ? s1 : 0
 *                 dLoss/dz_c = (w (p_c - 1{c = a}) + c_e p_c (log p_c + H)) / N_tot
 *                 e1 = V - ret      d = V - value_old
 *                 value_clip == 0 or |d| <= value_clip:   L_v = e1^2      dLoss/dV = 2 c_v e1 / N_tot      (value_old + d is never formed)
 *                 otherwise:  e2 = (value_old + copysignf(value_clip, d)) - ret      L_v = fmaxf(e1^2, e2^2)
 *                             dLoss/dV = (e1^2 >= e2^2) ? 2 c_v e1 / N_tot : 0
 *               loss[0..5] = the chunk's share of {total = L_pi + c_v L_v - c_e H, sum L_pi / N_tot, sum L_v / N_tot, sum H / N_tot,
 *               clip fraction = sum 1{r < lo or r > hi} / N_tot, approximate KL = sum ((r - 1) - lr) / N_tot}; sums over b in ascending
 *               order, no atomics: equal inputs give equal bits
 *   training    fb_qnet_ppo_train_step on gathered states, fb_ppo_train_from_replay on ring positions idx (as fb_ac_train_from_replay):
 *               1 <= batch <= min(max_batch, 256), n_total >= batch; adv, ret, logp_old, value_old f32; loss f32[6]; flat_grad as for A2C
 *               (NULL: Adam at once, with the net's clipping; else the chunk's gradient is exported only).  sel (ring-fed call) i64[batch]
 *               or NULL: sample b reads adv, ret, logp_old and value_old at sel[b] (NULL: at b), so a shuffled minibatch reads the
 *               flattened [T N] rollout buffers in place; the caller keeps every sel[b] inside them
 *   normalise   fb_ac_normalize_adv, per rollout, in double: thread t of ONE 256-thread workgroup sums the elements i = t (mod 256) in
 *               ascending i (from 0.0), one thread adds the 256 partial sums in ascending t: S; mean = S / n; the same two-level sum of
 *               (x - mean)^2: Q; sd = sqrt(Q / n); out[i] = (float)(((double)x_i - mean) / (sd + 1e-8)).  out may be adv.  1 <= n < 2^31
 *   shuffle     fb_ac_permute(n, seed, draw, out): out i64[n] is a permutation of [0, n), a function of (n, seed, draw) alone.  k = the
 *               smallest even bit count with 2^k >= n (k >= 2), half = k / 2, mask = 2^half - 1, x = (L << half) | R; four Feistel
 *               rounds r = 0 .. 3: (L, R) <- (R, L ^ (F_r(R) & mask)), F_r(R) = word r (x, y, z, w) of Philox4x32-10(key = (seed_lo,
 *               seed_hi), counter = (R, draw_lo, FB_STREAM_PERM = 9, draw_hi)); out[i] = the first value below n of i's images under
 *               repeated application (cycle walking: the network is a bijection of [0, 2^k), and 2^k < 4 n).  1 <= n < 2^31
 *   refused     FB_ERR_INVALID before any launch or counter change: fb_qnet_set_ppo / _get_ppo / fb_qnet_ppo_train_step /
 *               fb_ppo_train_from_replay on a net that is not an AC net; a prioritized or n-step memory; the batch and n_total rules above
 *   not offered data-parallel PPO, bf16, per-minibatch advantage normalisation, KL early stopping, annealing, recurrent policies. */
int fb_qnet_set_ppo(fb_qnet_t h, float clip_eps, float value_clip);
int fb_qnet_get_ppo(fb_qnet_t h, float *clip_eps_host, float *value_clip_host);
int fb_qnet_ppo_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *adv, const float *ret,
                           const float *logp_old, const float *value_old, int64_t n_total, float *loss /*f32[6]*/, float *flat_grad, void *stream);
int fb_ppo_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const int64_t *sel, const float *adv,
                             const float *ret, const float *logp_old, const float *value_old, int64_t n_total, uint8_t *a_out,
                             float *loss /*f32[6]*/, float *flat_grad, void *stream);
int fb_ac_normalize_adv(const float *adv, int64_t n, float *out, void *stream);
int fb_ac_permute(int64_t n, uint64_t seed, uint64_t draw, int64_t *out, void *stream);

/* ------------------------------------------------------------------ PPO: one epoch as one host call, and per-minibatch advantage normalisation
 * Of the block above's "not offered" items this one offers per-minibatch advantage normalisation (fb_ac_normalize_adv_sel, fb_ppo_epoch's
 * mb_adv_norm) in the library, and gives the loop above it what KL early stopping and annealing need: fb_ppo_epoch leaves the epoch's mean
 * approximate KL in epoch_mean[5], which a caller reads between two epochs to stop (there is no device-side gate on Adam), and annealing is
 * fb_qnet_set_hparams between two updates (VecActorCritic: target_kl, anneal_lr).  Data-parallel PPO, bf16 and recurrent policies stay not
 * offered.
 *   normalise   fb_ac_normalize_adv_sel(adv, sel, n, out), per MINIBATCH: the statistics over the n selected elements x_j = adv[sel[j]],
 *               j < n, only; in double, fb_ac_normalize_adv's two-level order applied to j: thread t of ONE 256-thread workgroup sums
 *               j = t (mod 256) in ascending j (from 0.0), one thread adds the 256 partial sums in ascending t: S; mean = S / n; the same
 *               two-level sum of (x_j - mean)^2: Q; sd = sqrt(Q / n); out[sel[j]] = (float)(((double)adv[sel[j]] - mean) / (sd + 1e-8)).
 *               Positions of out that sel does not name are not written.  out == adv is refused: an element normalised in one epoch would
 *               be normalised again in the next.  The sel[j] are distinct and inside adv / out by the caller's contract (a slice of a
 *               permutation), as fb_ppo_train_from_replay's sel.  1 <= n < 2^31.  Vector stores only, no atomics
 *   accumulate  fb_ac_grad_accumulate(acc, chunk, n, first): acc[i] = (first ? 0.f : acc[i]) + chunk[i], one fp32 add per element: what
 *               zeroing acc and adding the chunks one by one gives (a -0 of a first chunk becomes +0; NaN and Inf pass through; with
 *               first != 0 the old acc is not read).  Any n in 1 <= n < 2^31, any alignment; acc != chunk
 *   epoch       fb_ppo_epoch: ONE PPO epoch over n transitions; pos[k] is element k's ring position, sel[k] its index into the rollout
 *               buffers adv, ret, logp_old, value_old.  With mb = n / minibatches, for each minibatch m in ascending order:
 *                 1. mb_adv_norm != 0: fb_ac_normalize_adv_sel(adv, sel + m mb, mb, adv_scratch); the chunks of this minibatch then read
 *                    adv_scratch in place of adv
 *                 2. for every chunk of <= 256 consecutive elements k .. of the minibatch, in ascending order:
 *                    fb_ppo_train_from_replay(replay, net, chunk size, pos + k, sel + k, adv or adv_scratch, ret, logp_old, value_old,
 *                    n_total = mb, a_out, the chunk's six numbers, chunk_grad); then fb_ac_grad_accumulate(grad, chunk_grad,
 *                    fb_qnet_num_params, first = the minibatch's first chunk); then loss_rows[m][c] = (first ? 0.f : loss_rows[m][c]) +
 *                    the chunk's number c, c = 0 .. 5: the chunks' numbers added in fp32, from 0, in ascending chunk order
 *                 3. the net's max_grad_norm > 0: fb_qnet_clip_grad(net, grad)
 *                 4. fb_qnet_apply_adam(net, grad)
 *               afterwards epoch_mean[c] = (sum_m loss_rows[m][c], ascending m from 0.f) / (float)minibatches.  The whole call is, bit for
 *               bit, the composed calls above on `stream`: parameters, Adam state, grad, a_out (the last chunk's actions).  It launches
 *               only: no host synchronisation, no host read.  (On the way epoch_mean holds each chunk's six numbers.)
 *   running sum fb_ppo_epoch_sum(net, sum): sum [dev] f32[6] receives the net's running sum of its LAST fb_ppo_epoch -- the chunks' number c
 *               added in fp32, from 0.f, in ascending order over ALL chunks of the epoch, minibatch after minibatch (zeros before the
 *               first epoch): what a caller that adds every chunk's six numbers to one accumulator holds, as VecActorCritic's
 *               chunk-by-chunk loop does.  The rows' sum behind epoch_mean is another order of the same additions and differs from it in
 *               the last places wherever a minibatch has more than one chunk.  A copy on `stream`; an AC net only
 *   refused     FB_ERR_INVALID before any launch or counter change: everything fb_ppo_train_from_replay refuses (a net that is not an AC
 *               net, a prioritized or n-step memory, a chunk above max_batch); NULL arguments (adv_scratch may be NULL without mb_adv_norm);
 *               n outside 1 <= n < 2^31; minibatches < 1 or not dividing n; mb_adv_norm without adv_scratch or with adv_scratch == adv;
 *               grad == chunk_grad; a grad that is not 16-byte aligned on a net that clips */
int fb_ac_normalize_adv_sel(const float *adv, const int64_t *sel, int64_t n, float *out, void *stream);
int fb_ac_grad_accumulate(float *acc, const float *chunk, int64_t n, int first, void *stream);
int fb_ppo_epoch_sum(fb_qnet_t net, float *sum /*[dev] f32[6]*/, void *stream);
int fb_ppo_epoch(fb_replay_t replay, fb_qnet_t net, int64_t n, int minibatches, const int64_t *pos, const int64_t *sel, const float *adv,
                 const float *ret, const float *logp_old, const float *value_old, int mb_adv_norm, float *adv_scratch /*f32[rollout size] or NULL*/,
                 float *grad /*f32[num_params]*/, float *chunk_grad /*f32[num_params]*/, uint8_t *a_out /*u8[256]*/,
                 float *loss_rows /*f32[minibatches][6]*/, float *epoch_mean /*f32[6]*/, void *stream);

/* ------------------------------------------------------------------ discrete soft actor-critic (SAC; Haarnoja et al. 2018, Christodoulou 2019)
 * The off-policy learner of a STOCHASTIC policy: a policy head and two Q heads on the shared trunk, trained from the replay memory with an
 * entropy bonus whose temperature alpha is fixed or learned.  One GPU, fp32, a uniform memory at n-step 1.
 * A SAC net (FB_ARCH_SAC, fb_qnet_create_sac; 2 <= A <= 8) has the trunk and fc1 of every net, then three heads read RAW:
 *   W_pi[FC,A] b_pi[A] W_q1[FC,A] b_q1[A] W_q2[FC,A] b_q2[A]      (W_pi b_pi where a plain net of that shape has its head)
 * with h = relu(h_fc1):  z = h . W_pi + b_pi,  Q1 = h . W_q1 + b_q1,  Q2 = h . W_q2 + b_q2.
 *   init        fb_qnet_init_params: element i of the flat vector draws as in every net -- a weight from Philox counter (i, ctr, FB_STREAM_INIT, 0)
 *               under the seed, a bias 0.01 -- so the trunk, fc1 and W_pi b_pi are the plain net's of that seed bit for bit, and the two Q
 *               heads, keyed by their own indices, differ from each other
 *   acting      fb_qnet_forward / _act / _act_nib / fb_eval_run / fb_eval_q treat the LOGITS as the Q values (the plain head over W_pi b_pi):
 *               greedy play is argmax pi.  fb_qnet_forward_sac returns (z, Q1, Q2) of the online or the target net -- z the very bits
 *               fb_qnet_forward returns.  fb_qnet_act_policy_nib takes a SAC net as well: softmax, draw, greedy rule, logp and logits as
 *               pinned for an AC net; value may be NULL, else it receives the soft state value, float32, ascending c from 0:
 *                 V = sum_c p_c * (fminf(Q1_c, Q2_c) - alpha * log p_c)
 *   settings    fb_qnet_set_sac(alpha, target_entropy, alpha_lr): alpha finite > 0, target_entropy finite, alpha_lr finite >= 0; 0.2,
 *               0.98f * logf(A) and 0 in a new net; alpha_lr = 0: a fixed temperature.  The net holds five device words (log alpha, m, v,
 *               pow1, pow2); set writes (logf(alpha), 0, 0, beta1, beta2) with the net's betas at that time.  fb_qnet_get_sac returns
 *               expf(log alpha); fb_qnet_get_sac_state / _set_sac_state move the five words (checkpoints).  All four are synchronous.
 *               Every kernel reads alpha = expf(log alpha) on the device
 *   train step  per sample b, fp32, sums over c ascending from 0, alpha the value the previous step left; ' marks s':
 *                 p', lp' = softmax(z(s'; online))       Q1', Q2' from the TARGET net       V' as the soft state value above
 *                 r = (R == 0.1f) ? 0.1 : (double)R      y = (float)(t ? r : r + gamma * (double)V')      (no gradient through y)
 *                 d_i = Q_i(s, a) - y       L_q = d_1^2 + d_2^2       dLoss/dQ_i(s, a) = (2 d_i) / B, the other columns 0
 *                 p, lp = softmax(z(s))     f_c = alpha * lp_c - fminf(Q1_c(s), Q2_c(s))  (min Q a constant)     L_pi = sum_c p_c f_c
 *                 H = -sum_c p_c lp_c       dLoss/dz_c = (p_c (f_c - L_pi)) / B       (the actor's gradient enters the shared trunk)
 *               loss[0..5]: m1 = (sum_b d_1^2) / B, m2 likewise, mp = (sum_b L_pi) / B, mh = (sum_b H) / B, sums over b ascending;
 *               loss = {(m1 + m2) + mp, m1, m2, mp, mh, the alpha used}.  No atomics: equal inputs give equal bits.
 *               an action >= A reads A - 1.  1 <= batch <= min(max_batch, 256); 0 <= gamma <= 1.  q_target f32[batch] (y) or NULL.
 *               flat_grad and the net's max_grad_norm as in fb_qnet_train_step.  fb_qnet_sac_train_step takes gathered states,
 *               fb_sac_train_from_replay ring positions (a_out / r_out / t_out receive the ring's a, r, t); the two agree bit for bit
 *   temperature when alpha_lr > 0 and the caller exports nothing (flat_grad NULL), behind the net's Adam tick, on one thread, b1 / b2 / eps the net's:
 *                 g = mh - target_entropy        at = alpha_lr * sqrtf(1 - pow2) / (1 - pow1)        pow1 *= b1   pow2 *= b2
 *                 m += (g - m) * (1 - b1)        v += (g * g - v) * (1 - b2)        log alpha -= (m * at) / (sqrtf(v) + eps)
 *               An exporting step and fb_qnet_apply_adam leave the five words alone
 *   loop step   fb_sac_step = fb_qnet_act_policy_nib (sampled; no value / logp) -> fb_env_step -> fb_replay_push_sample(batch) -> if train:
 *               fb_sac_train_from_replay (b->loss f32[6], b->flat_grad) -> if rho > 0: fb_qnet_soft_sync_target(rho); those calls in that
 *               order on `stream`, their results bit for bit.  No riders, no split schedule; it pushes: not capturable, like fb_vec_step
 *   refused     FB_ERR_INVALID before any launch or counter change: on a SAC net every FB_ALGO_* of fb_qnet_train_step / fb_train_from_replay /
 *               fb_train_steps / fb_vec_step / fb_vec_step_dp, the A2C and PPO calls, fb_qnet_set_huber / _get_huber, fb_qnet_set_munchausen /
 *               _get_munchausen, FB_DTYPE_BF16 for inference or training; fb_qnet_create with arch 7 and fb_qnet_create_c51_noisy with it;
 *               the SAC calls below on a net that is not a SAC net; a prioritized or n-step memory; the batch, gamma and settings rules above
 *   not offered data-parallel SAC, bf16, prioritized replay, n-step returns, noisy or distributional critics, riders or the split schedule. */
#define FB_ARCH_SAC 7
int fb_qnet_create_sac(int fc_width, int n_actions, int max_batch, fb_qnet_t *out);
int fb_qnet_set_sac(fb_qnet_t h, float alpha, float target_entropy, float alpha_lr);
int fb_qnet_get_sac(fb_qnet_t h, float *alpha_host, float *target_entropy_host, float *alpha_lr_host);
int fb_qnet_get_sac_state(fb_qnet_t h, float *state_host /*f32[5]*/);
int fb_qnet_set_sac_state(fb_qnet_t h, const float *state_host /*f32[5]*/);
/* states u8[B,80,80,4] -> logits, q1, q2 f32[B,A]; 1 <= B <= 3 * max_batch; which: FB_NET_ONLINE / FB_NET_TARGET */
int fb_qnet_forward_sac(fb_qnet_t h, int which, const uint8_t *states, int batch, float *logits, float *q1, float *q2, void *stream);
int fb_qnet_sac_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,
                           double gamma, float *loss /*f32[6]*/, float *q_target, float *flat_grad, void *stream);
int fb_sac_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, uint8_t *a_out, float *r_out, uint8_t *t_out,
                             double gamma, float *loss /*f32[6]*/, float *q_target, float *flat_grad, void *stream);

/* ------------------------------------------------------------------ prioritized SAC and n-step returns (Schaul et al. 2016; Horgan et al. 2018, Ape-X)
 * The SAC step above on a PRIORITIZED memory (fb_replay_create / fb_replay_create_nstep with prioritized = 1), as calls of their own: the
 * memory's kind never switches what a call does, and the uniform calls above keep refusing a prioritized memory and an n-step view.
 * Everything not named here is the uniform step's, formula for formula.  With w_b = isw[b] (Memory.sample's importance weights, float32):
 *   critics     targets, d_1 and d_2 unchanged.  dLoss/dQ_i(s, a) = ((2 d_i) / B) * w_b; the terms summed into m1 / m2 are (d_i * d_i) * w_b.
 *               w is multiplied LAST in both, so w_b = 1 for every b gives the uniform step's bits in every output.  The weights are not
 *               validated on the device, as in the other prioritized steps.  The dhf row takes the weight through dQ_i
 *   actor, temperature   NOT weighted: L_pi, H, dLoss/dz_c and the temperature's Adam step (driven by mh, the unweighted mean entropy) are the
 *               uniform step's.  The importance weights correct the critic's TD expectation under the skewed draw; the policy-improvement
 *               step holds under any state distribution, and leaving it alone keeps the temperature's dynamics those of the uniform step
 *   priority    abs_err[b] = 0.5f * (fabsf(d_1) + fabsf(d_2)), written UNWEIGHTED, in FB_ALGO_PER's |TD error| unit: the memory's own
 *               (min(|e| + 0.01, 1))^0.6 applies unchanged (fb_replay_update_priorities)
 *   n-step      on a prioritized memory made with n > 1 the ring delivers (R, done) and s' = the state n steps on:
 *                 y = done ? R : R + Gamma * V'(s'),   Gamma = gamma^n as the memory forms it, R as r above
 *               R is the ring's plain n-step return: the intermediate steps carry NO entropy bonus (the soft value enters at the bootstrap
 *               alone).  fb_sac_per_train_from_replay's gamma must be the memory's; fb_qnet_sac_per_train_step, the gathered call,
 *               takes Gamma from the caller.  The two agree bit for bit
 *   loop step   fb_sac_per_step: every argument check of every call below comes first -- nothing is launched and no push is counted before a
 *               refusal -- then, in this order on `stream`: fb_qnet_act_policy_nib (sampled) -> fb_env_step -> fb_replay_push -> if train:
 *               fb_replay_sample_f32, fb_sac_per_train_from_replay on b->isw32 / b->abs_err, fb_replay_update_priorities with abs_err left as
 *               the loss wrote it -> if rho > 0: fb_qnet_soft_sync_target(rho).  Each result is bit for bit that of the separate calls.
 *               A training step before n pushes exist at its draw returns FB_ERR_STATE before any launch; train = 0 is a store-only step
 *   refused     FB_ERR_INVALID before any launch or counter change: a net that is not a SAC net; a uniform memory; NULL isw or abs_err; the
 *               batch, gamma and rho rules of the uniform calls
 *   not offered uniform n-step SAC through the ring (the gathered route serves it: fb_replay_gather on an n-step view, then
 *               fb_qnet_sac_train_step with Gamma); data-parallel SAC, bf16, noisy or distributional critics, riders, the split schedule; a
 *               weighted actor term. */
int fb_qnet_sac_per_train_step(fb_qnet_t h, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2, const uint8_t *t,
                               const float *isw /*f32[B]*/, double gamma, float *loss /*f32[6]*/, float *abs_err /*f32[B]*/,
                               float *q_target, float *flat_grad, void *stream);
int fb_sac_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int batch, const int64_t *idx, const float *isw, uint8_t *a_out,
                                 float *r_out, uint8_t *t_out, double gamma, float *loss, float *abs_err, float *q_target,
                                 float *flat_grad, void *stream);

/* ------------------------------------------------------------------ implicit quantile networks (IQN; Dabney, Ostrovski, Silver & Munos 2018)
 * The step after QR-DQN: the net learns the whole quantile function theta(s, a; tau), trains on sampled tau and can act under a distorted
 * risk measure (CVaR).  One GPU, fp32, a uniform memory at any n-step view.
 * An IQN net (FB_ARCH_IQN, fb_qnet_create_iqn; 2 <= A <= 8; 1 <= n_tau N, n_tau_next N', n_tau_act K <= 64; kappa finite > 0, all checked
 * before any allocation) has the PLAIN layout, then the embedding of FB_IQN_COS = 64 cosines (E):
 *   trunk, W_fc1, b_fc1, W_q[FC,A], b_q[A], W_e[E,FC], b_e[FC]      (W_q b_q where a plain net has its head; one flat vector for Adam,
 *                                                                     load / store / sync and the clip)
 *   init        fb_qnet_init_params draws every weight by its own index, as in every net: the trunk, fc1 and W_q b_q are the plain net's of that
 *               seed bit for bit, W_e draws like any weight.  b_e is filled with 1.0, NOT 0.01: a fresh net has phi ~ 1 and starts as the plain
 *               net of its seed; the dependence on tau is learned
 *   theta       h = relu(h_fc1).  c_j(tau) = (float)cos(M_PI * (double)j * (double)tau), j = 0 .. 63 (formed in double, rounded once);
 *               pre_k(tau) = b_e[k] + sum_j c_j W_e[j,k], fmaf over ascending j from b_e[k];  phi_k = relu(pre_k);
 *               theta(tau)_a = b_q[a] + sum_k (h_k phi_k) W_q[k,a]   (the order of the sum over k is the kernel's: fixed, no atomics)
 *   greedy Q    the net holds a risk setting eta (fb_qnet_set_iqn_risk, 0 < eta <= 1, 1 in a new net): CVaR_eta through tau -> eta tau.
 *               tauhat_i = (float)((double)eta * (2 i + 1) / (2 K)), i < K;  phibar_k = (sum_i phi_k(tauhat_i)) / (float)K, float32, ascending i;
 *               Wt_q[k,a] = phibar_k * W_q[k,a];  Qbar(s, .) = the plain head over (b_fc1, Wt_q, b_q) -- the mean of theta over the grid,
 *               since theta is linear in phi.  fb_qnet_forward / _act / _act_nib / fb_eval_run / fb_eval_q return Qbar of the online or the
 *               target net with the plain net's first-maximum rule, epsilon rule and Philox draws.  The fold (b_fc1, Wt_q, b_q) of a net is
 *               rebuilt by one small launch behind everything that changes its parameters or eta: Adam (fused or fb_qnet_apply_adam),
 *               fb_qnet_load_params, _init_params, _sync_target, _soft_sync_target, fb_qnet_set_iqn_risk (on the default stream, then
 *               synchronised).  fb_qnet_is_dist is 0: for acting purposes an IQN net is a plain net
 *   forward_iqn theta f32[B][M][A] of the online or target net at the caller's tau f32[B][M]; 1 <= M <= 64, 1 <= B <= 3 * max_batch
 *   tau draws   fb_iqn_draw_taus(batch, n, seed, step, which, out f32[batch][n]), stateless: o = Philox(key = seed, counter = (b * 64 + i,
 *               step_lo, FB_STREAM_TAU = 10, step_hi)); tau = (float)(2 * (w >> 9) + 1) * 2^-24 with w = o.x for which = 0 (online) and
 *               o.y for which = 1 (target): exact in float32, strictly inside (0, 1)
 *   train step  per sample b, fp32 unless said otherwise:
 *                 a* = the first maximum of Qbar(s', .) of the TARGET net (double_q = 0) or the online net (double_q = 1)
 *                 r = (R == 0.1f) ? 0.1 : (double)R      T_j = (float)(done ? r : r + gamma * (double)theta_tgt(s', a*; tau'_j)), j < N'
 *                 theta_i = theta(s, a_b; tau_i), i < N      u_ij = T_j - theta_i      w_ij = |tau_i - 1{u_ij < 0}|
 *                 L(u) = u^2 / 2 if |u| <= kappa else kappa (|u| - kappa / 2)
 *                 l_b = (sum_i (sum_j (w_ij L(u_ij)) / kappa)) / N'        j ascending inside, i ascending outside
 *                 dl_b/dtheta_i = (-(sum_j (w_ij clamp(u_ij, -kappa, kappa)) / kappa) / N') / B       j ascending; T is a constant
 *               loss[0] = (sum_b l_b) / B over ascending b.  Gradients reach W_q and b_q (the taken action's column), W_e, b_e, and through
 *               dhf fc1 and the trunk; every sum runs in a fixed order with no atomics: equal inputs give equal bits.
 *               tau f32[B][N] / tau_next f32[B][N'] are the caller's, or NULL: the draws above from (seed, step), which 0 / 1, bit for bit.
 *               an action >= A reads A - 1.  1 <= batch <= min(max_batch, 256); 0 <= gamma <= 1 (an n-step memory: fb_iqn_train_from_replay
 *               wants the memory's gamma and bootstraps with Gamma = gamma^n as every ring-fed call; fb_qnet_iqn_train_step takes the
 *               discount of the bootstrap itself).  q_target f32[B][N'] (T) or NULL.  flat_grad, the Adam tick and the net's max_grad_norm
 *               as in fb_qnet_sac_train_step.  The gathered and the ring-fed call agree bit for bit
 *   loop step   fb_iqn_step = fb_qnet_act_nib(epsilon) -> fb_env_step -> fb_replay_push_sample(batch) -> if train: fb_iqn_train_from_replay
 *               (tau from (seed, step); b->loss f32[1], b->flat_grad); those calls in that order on `stream`, after every check of all of
 *               them, their results bit for bit.  It pushes: not capturable
 *   refused     FB_ERR_INVALID before any launch or counter change: on an IQN net every FB_ALGO_* of fb_qnet_train_step / fb_train_from_replay /
 *               fb_train_steps / fb_vec_step / fb_vec_step_dp, the A2C, PPO and SAC calls, fb_qnet_set_huber / _get_huber, _set_munchausen /
 *               _get_munchausen, the noise calls, fb_qnet_forward_dist / _forward_quantiles, FB_DTYPE_BF16; fb_qnet_create with arch 8; the
 *               IQN calls on a net that is not an IQN net; a prioritized memory
 *   not offered prioritized replay, dueling or noisy IQN, bf16, data parallel, riders of the train step, the split schedule. */
#define FB_ARCH_IQN 8
#define FB_IQN_COS 64
int fb_qnet_create_iqn(int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch, fb_qnet_t *out);
int fb_qnet_set_iqn_risk(fb_qnet_t h, float eta);
int fb_qnet_get_iqn(fb_qnet_t h, int *n_tau_host, int *n_tau_next_host, int *n_tau_act_host, float *kappa_host, float *eta_host);
int fb_qnet_forward_iqn(fb_qnet_t h, int which, const uint8_t *states, int batch, const float *tau /*f32[B][M]*/, int M,
                        float *theta /*f32[B][M][A]*/, void *stream);
int fb_iqn_draw_taus(int batch, int n, uint64_t seed, uint64_t step, int which, float *tau_out /*f32[batch][n]*/, void *stream);
int fb_qnet_iqn_train_step(fb_qnet_t h, int double_q, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                           const uint8_t *t, const float *tau, const float *tau_next, uint64_t seed, uint64_t step, double gamma,
                           float *loss /*f32[1]*/, float *q_target, float *flat_grad, void *stream);
int fb_iqn_train_from_replay(fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, uint8_t *a_out, float *r_out,
                             uint8_t *t_out, const float *tau, const float *tau_next, uint64_t seed, uint64_t step, double gamma,
                             float *loss /*f32[1]*/, float *q_target, float *flat_grad, void *stream);
/* ------------------------------------------------------------------ prioritized IQN: the three calls above with importance weights
 * Calls of their own -- the memory's kind never switches what one of the three calls above does, they keep refusing a prioritized memory.
 * With double_q = 1 on an n-step prioritized memory (fb_replay_create_nstep) this is the non-dueling "Rainbow-IQN" configuration.
 *   train step  fb_qnet_iqn_per_train_step (gathered) / fb_iqn_per_train_from_replay (ring-fed; idx are SumTree leaf indices): the IQN train
 *               step above -- a*, T, the tau draws, theta, l_b unchanged -- with w_b = isw[b]:
 *                 dl_b/dtheta_i = ((-(sum_j ...) / N') / B) * w_b      the weight multiplied LAST, as FB_ALGO_QR_PER forms it
 *                 loss[0] = (sum_b w_b l_b) / B over ascending b       abs_err[b] = l_b, WITHOUT the weight (>= 0): the priority
 *               w = 1 gives the uniform call's loss, T and gradient bit for bit.  isw / abs_err f32[batch], both required.  No atomics: equal
 *               inputs give equal bits.  The gathered and the ring-fed call agree bit for bit; an n-step memory as above (the memory's gamma,
 *               Gamma = gamma^n)
 *   loop step   fb_iqn_per_step = fb_qnet_act_nib(epsilon) -> fb_env_step -> fb_replay_push -> if train: fb_replay_sample into b->idx / b->isw /
 *               b->isw32 -> fb_iqn_per_train_from_replay(b->isw32, tau from (seed, step), b->loss, b->abs_err, b->flat_grad) ->
 *               Memory.batch_update(b->idx, b->abs_err); those calls in that order on `stream`, after every check of all of them, their
 *               results bit for bit.  Memory.batch_update runs IN LINE at every env count: no side stream, no sample-ahead, no riders (what
 *               fb_vec_step's prioritized step does from 4096 envs on is not done here).  When it returns b->abs_err holds l_b as the loss
 *               left it, as fb_vec_step's prioritized step leaves |TD error| (see fb_step_buffers).  It pushes: not capturable
 *   refused     FB_ERR_INVALID before any launch, push or counter change: a uniform memory; a net that is not an IQN net; NULL isw / abs_err
 *               (a training fb_iqn_per_step: b->isw, b->isw32, b->abs_err); the batch, double_q and gamma rules above; an n_envs that is
 *               not the handles'.  FB_ERR_STATE: an n-step prioritized memory whose tree is still empty when the step would sample. */
int fb_qnet_iqn_per_train_step(fb_qnet_t h, int double_q, int batch, const uint8_t *s, const uint8_t *a, const float *r, const uint8_t *s2,
                               const uint8_t *t, const float *isw /*f32[B]*/, const float *tau, const float *tau_next, uint64_t seed,
                               uint64_t step, double gamma, float *loss /*f32[1]*/, float *abs_err /*f32[B]*/, float *q_target,
                               float *flat_grad, void *stream);
int fb_iqn_per_train_from_replay(fb_replay_t replay, fb_qnet_t net, int double_q, int batch, const int64_t *idx, const float *isw /*f32[B]*/,
                                 uint8_t *a_out, float *r_out, uint8_t *t_out, const float *tau, const float *tau_next, uint64_t seed,
                                 uint64_t step, double gamma, float *loss /*f32[1]*/, float *abs_err /*f32[B]*/, float *q_target,
                                 float *flat_grad, void *stream);
/* ------------------------------------------------------------------ dueling IQN: value and advantage quantile streams
 * The linear dueling head of this code base (V and the advantages read straight off fc1, BrainDuelingDQN.py:78-86) on the quantile function:
 * both streams share g_k(tau) = h_k phi_k(tau), so the combine V(tau) + Adv_a(tau) - mean_a' Adv_a'(tau) is ONE effective column per action.
 * A dueling IQN net (FB_ARCH_IQN_DUELING, fb_qnet_create_iqn_dueling: fb_qnet_create_iqn's arguments and checks, before any allocation) has
 * the DUELING layout, then the embedding:
 *   trunk, W_fc1, b_fc1, W_v[FC,1], b_v[1], W_a[FC,A], b_a[A], W_e[E,FC], b_e[FC]      (one flat vector for Adam, load / store / sync, the clip)
 *   init        every weight by its own index: the part up to b_a is the FB_ARCH_DUELING net of that seed bit for bit (b_v = 0.01); b_e = 1.0
 *   forward     all float32:
 *                 m_k     = (sum_{c<A} W_a[k,c]) / (float)A            ascending c from 0.f
 *                 We[k,a] = (W_v[k] + W_a[k,a]) - m_k
 *                 be[a]   = (b_v + b_a[a]) - (sum_c b_a[c]) / (float)A      ascending c from 0.f
 *                 theta(tau)_a = be[a] + sum_k (h_k phi_k(tau)) We[k,a]     IQN's sum over k, unchanged
 *               theta, T, a* and the loss are IQN's with We / be where W_q / b_q stand (formed in place wherever they are read)
 *   greedy Q    the fold block stays in the PLAIN layout, [b_fc1 | phibar_k * We[k,a] | be[a]]: for acting a dueling IQN net is a plain net
 *               over its fold, as an IQN net is; no acting kernel is its own.  The fold is rebuilt wherever an IQN net's is.
 *               fb_qnet_is_dist is 0
 *   gradients   with gw[b,k] the taken column's gradient row of sample b, as IQN forms it:
 *                 G_k = sum_b gw[b,k]   H_kc = sum_{b: a_b = c} gw[b,k]   (both over ascending b)
 *                 dW_v[k] = G_k         dW_a[k,c] = H_kc - G_k / (float)A
 *               b_v and b_a the same way from dl_b = sum_i dl_b/dtheta_i.  W_e, b_e, b_fc1, the trunk, the loss and the Adam tick as IQN's.
 *               No atomics: equal inputs give equal bits
 *   calls       every fb_qnet_*iqn* and fb_iqn_* call above, the prioritized ones and both loop steps included, takes either kind of net and
 *               refuses what it refused; fb_qnet_create with arch 9 is refused
 *   not offered noisy IQN, bf16, data parallel, riders, the split schedule; Munchausen with double_q. */
#define FB_ARCH_IQN_DUELING 9
int fb_qnet_create_iqn_dueling(int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, int max_batch, fb_qnet_t *out);
/* ------------------------------------------------------------------ Munchausen IQN (M-IQN; Vieillard, Pietquin & Geist 2020, section 4)
 * Munchausen-DQN's soft bootstrap and log-policy bonus on IQN's target.  A setting of an IQN net (either arch): off in a new net, which
 * then holds (temp, alpha, l0) = (0.03, 0.9, -1).  `temp` is Munchausen-DQN's tau; tau is the quantile fraction everywhere in IQN.  Off: every
 * call is what it was, bit for bit.  On, for sample b of every IQN training call (gathered, ring-fed, the prioritized ones, both loop steps):
 *   forward     three slices still: s through the online net, s through the TARGET net (where s' through the online net stood: only
 *               double_q read it), s' through the target net
 *   Qbar rows   q' = Qbar-(s', .) and q = Qbar-(s, .): the plain head over the TARGET net's fold block, the bits fb_qnet_forward(FB_NET_TARGET)
 *               returns and the acting path would read.  The net's CVaR eta is IN them (the fold's grid is eta tauhat): the soft policy is
 *               over what the agent acts on
 *   policy      at s', float32, ascending c:  m' = max_c q'_c;  e_c = expf((q'_c - m') / temp);  S' = sum_c e_c (from 0.f);  pi_c = e_c / S';
 *               t_c = (q'_c - m') - temp * logf(S')   (= temp ln pi_c; never formed as a log of pi_c, so finite when e_c underflows to 0)
 *   soft value  V_j = sum_c pi_c * (theta_tgt(s', c; tau'_j) - t_c), j < N': ascending c from 0.f, a multiply then an add (no fma); theta_tgt
 *               of every column has the bits the one-column form of the hard target gives it
 *   bonus       alpha * fmaxf((q_a - m) - temp * logf(S), l0),  m = max_c q_c, S = sum_c expf((q_c - m) / temp), a = the stored action (one
 *               >= A reads A - 1): Munchausen-DQN's expression over q
 *   target      T_j = (float)((r + (double)bonus) + (done ? 0 : gamma * (double)V_j)), r = (R == 0.1f) ? 0.1 : (double)R, float64, rounded
 *               once.  The bonus is added on terminal transitions too.  An n-step memory: R is the n-step return, gamma the bootstrap's
 *               Gamma = gamma^n, and only the first step's bonus (that of (s, a)) exists -- Munchausen-DQN's rules
 *   unchanged   theta_i, u_ij, the loss, dl_b/dtheta_i, abs_err = l_b, the priority convention, the importance weight multiplied last, the
 *               tau draws, q_target = T, the gradient kernel and everything behind it.  There is no a*, no argmax anywhere
 *   limits      temp -> 0 with alpha = 0: once every gap of q' is >= 104 temp, pi is exactly one-hot, t = 0 there, and T, the loss and the
 *               gradient are the hard target's (double_q = 0) bit for bit.  l0 = 0: the bonus is exactly 0 (its argument is <= 0)
 * fb_qnet_set_iqn_munchausen: FB_ERR_INVALID before anything changes: a net that is not an IQN net, on not 0 / 1, temp not finite or <= 0,
 *   alpha outside [0, 1], l0 not finite or > 0.  A host-side setting read by the calls issued after it.
 * fb_qnet_get_iqn_munchausen: the current values [host] (any of the pointers may be NULL); FB_ERR_INVALID on a net that is not an IQN net.
 * fb_qnet_set_munchausen / _get_munchausen keep refusing an IQN net.
 *   refused     FB_ERR_INVALID before any launch, push or counter change: double_q = 1 in any IQN training call or loop step on a net with
 *               the setting on (the soft target has no a* for the online net to choose)
 *   not offered noisy IQN, bf16, data parallel, riders, the split schedule; Munchausen with double_q. */
int fb_qnet_set_iqn_munchausen(fb_qnet_t h, int on, float temp, float alpha, float clip_lo);
int fb_qnet_get_iqn_munchausen(fb_qnet_t h, int *on_host, float *temp_host, float *alpha_host, float *clip_lo_host);
/* ------------------------------------------------------------------ noisy IQN (Fortunato et al. 2018 on the IQN net; with the dueling head,
 * prioritized replay and n-step returns: Rainbow-IQN, Toromanoff et al. 2019)
 *
 * This block supersedes the "not offered ... noisy IQN" lines of the four IQN blocks above.
 * A noisy IQN net is an IQN (arch 8) or dueling IQN (arch 9) net whose fc1 (1600 -> FC) and head layers are factorised Gaussian layers, as a
 * noisy C51 net's.  Plain head: W_q b_q, FC -> A.  Dueling head: the V layer FC -> 1 and the advantage layer FC -> A, separate layers with
 * separate noise.  The conv trunk and the tau embedding W_e b_e stay deterministic.
 *   made by     fb_qnet_create_iqn_noisy(dueling 0 / 1, ...): fb_qnet_create_iqn's checks plus sigma0 finite and >= 0, before any allocation.
 *               fb_qnet_create_c51_noisy with arch 8 / 9, fb_qnet_create(8 | 9, ...) and the noise calls on a non-noisy net keep their refusals
 *   layout      the master vector is [mu | sigma].  mu is the net's IQN layout, unchanged: n_mu = the non-noisy net's count.  sigma covers the
 *               entries q in [OFF_WF1, off.we) -- W_fc1 b_fc1 and the head; W_e b_e have no sigma -- and sits at n_mu + q - OFF_WF1.
 *               fb_qnet_num_params = n_mu + (off.we - OFF_WF1).  Load, store, flat_grad, the Adam state, both target syncs, the soft sync and
 *               the global-norm clip cover the whole vector
 *   init        mu is the non-noisy net's bits for the same seed (b_e = 1.0 is kept); sigma = sigma0 / sqrt(fan_in) per layer, weights and biases
 *   noise       per layer, in the layout's order: f(eps_in)[fan_in], then f(eps_out)[fan_out].  nz = (1600 + FC) + (FC + A); dueling:
 *               (1600 + FC) + (FC + 1) + (FC + A).  The draws are those of FB_NOISE_SAMPLE / FB_NOISE_MEAN above: Philox stream 6, counter
 *               (element, step_lo, 6, 2 step_hi + net).  A new net is in mean mode
 *   effective   params[w] = mu + sigma (.) e on [OFF_WF1, off.we), mu elsewhere; rebuilt behind every change (init, load, both syncs, the
 *               fused Adam, fb_qnet_apply_adam, fb_qnet_reset_noise), and the IQN fold follows each rebuild.  So every forward-only path
 *               (fb_qnet_act_nib, fb_eval_run, fb_eval_q, the env launch's head rider, fb_qnet_forward, fb_qnet_forward_iqn) sees the current
 *               sample; the shared mode has no acting kernel of its own
 *   gradient    the IQN kernels yield the effective weights' gradient, which is mu's; sigma's is g[n_mu + q - OFF_WF1] = g[q] e(q); W_e b_e
 *               gradients pass through untouched.  In mean mode sigma's gradient is 0 and mu trains bit for bit as the non-noisy IQN net
 *   per-env     FB_ACT_NOISE_PER_ENV, fb_qnet_act_nib_env_noise's draws: stream 7, counter (e nz + k, step_lo, 7, step_hi).  fc1 as documented
 *               for C51: h_k = relu((mu partials + b_k) + f(eo_k) (t_k + sigma_b_k)).  Plain head:
 *                 Qbar_e(a) = [b_q[a] + sum_k phibar_k W_q^mu[k, a] h_k] + f(eo_a) (sum_k phibar_k sigma_W[k, a] f(ei_k) h_k + sigma_b[a])
 *               The bracket is the mu logit over the mu fold, with the plain head's arithmetic; the noise term is added after it.  phibar is
 *               the acting grid's mean embedding (K points, risk eta) from mu's W_e b_e: theta is linear in phi and the noise does not depend
 *               on tau, so this is exactly the grid mean of theta under env e's effective weights.  Dueling: the noise term of column a is
 *               nV + nA_a - (1/A) sum_c nA_c, nV and nA_c formed as the plain head's noise term over the V and advantage layers' own sigma and
 *               noise.  epsilon-greedy is fb_qnet_act_nib's, on the same Philox stream.  At sigma = 0 the call is mean-mode fb_qnet_act_nib
 *               bit for bit, actions and Q.  The call reads no net's sample and leaves samples, effective vectors, folds, parameters and Adam
 *               state as they were
 *   steps       fb_iqn_step / fb_iqn_per_step on a noisy net are bit for bit the composed public calls.  Shared mode: fb_qnet_reset_noise(0,
 *               SAMPLE, seed, step) -> fb_qnet_act_nib -> env step -> store / sample -> fb_qnet_reset_noise(1, ...) -> train.  Per-env mode:
 *               fb_qnet_act_nib_env_noise(seed, step) -> env step -> store / sample -> fb_qnet_reset_noise(0) -> fb_qnet_reset_noise(1) ->
 *               train (fb_vec_step's order).  The tau draws (stream 10) are unchanged.  double_q, n-step, prioritized replay, CVaR, Polyak,
 *               gradient clipping and Munchausen compose
 *   takes it    fb_qnet_is_noisy, _reset_noise, _get_noise, _set_acting_noise, _act_nib_env_noise; every fb_qnet_iqn_* / fb_iqn_* call,
 *               fb_qnet_set_iqn_risk and fb_qnet_set_iqn_munchausen
 *   refused     before any launch or counter change: fb_vec_step*, fb_train_steps, FB_DTYPE_BF16, data parallel, the scalar / C51 / QR algos,
 *               n nz >= 2^32 in the per-env call
 *   not offered noisy QR / scalar / SAC nets, one launch for draw + rebuild + fold, the split schedule, riders. */
int fb_qnet_create_iqn_noisy(int dueling, int fc_width, int n_actions, int n_tau, int n_tau_next, int n_tau_act, float kappa, float sigma0,
                             int max_batch, fb_qnet_t *out);

int fb_qnet_create(int arch, int fc_width, int n_actions, int max_batch, fb_qnet_t *out);
int fb_qnet_destroy(fb_qnet_t h);
int fb_qnet_num_params(fb_qnet_t h, int64_t *n_host);
/* tf.truncated_normal(stddev=0.01) weights, 0.01 biases, for `which` net. */
int fb_qnet_init_params(fb_qnet_t h, int which, uint64_t seed, void *stream);
int fb_qnet_load_params(fb_qnet_t h, int which, const float *flat /*[dev]*/, void *stream);
int fb_qnet_store_params(fb_qnet_t h, int which, float *flat /*[dev]*/, void *stream);
/* Adam slots m, v (f32[n] [dev]) and beta powers ([host] f32[2]); synchronous. */
int fb_qnet_get_adam_state(fb_qnet_t h, float *m, float *v, float *beta_pows_host);
int fb_qnet_set_adam_state(fb_qnet_t h, const float *m, const float *v, const float *beta_pows_host);
int fb_qnet_set_hparams(fb_qnet_t h, float lr, float beta1, float beta2, float eps);
/* Arithmetic of the forward-only path on >= 256 states (fb_qnet_forward / fb_qnet_act / fb_qnet_act_nib):
 *   FB_DTYPE_F32  (default) fp32-equivalent: every fp32 product as three fp16 MFMA products of two planes (x = h + l/4096).  The
 *                 pair carries x to 2^-24 relative for 2^-14 <= |x| < 65504 (fp16's normal range): weights and activations of this
 *                 network live there; gradient operands (1e-6 .. 1e-9 in the reference's regime) are brought there by an exact
 *                 power-of-two pre-scale taken from the operand block's maximum, folded back in the epilogue (csrc/fb_qnet.hip
 *                 pow2_scale; tests/test_gpu_qnet.py::test_train_step_gradients_in_the_reference_regime)
 *   FB_DTYPE_BF16 plain bf16 inference (config 3 of BASELINE.json: "bf16"): activations and weights rounded to
 *                 bf16, fp32 accumulation.  Training and batches < 256 always compute in fp32. */
#define FB_DTYPE_F32 0
#define FB_DTYPE_BF16 1
int fb_qnet_set_inference_dtype(fb_qnet_t h, int dtype);
/* Range guard of FB_DTYPE_F32.  ACTIVATIONS are split into their two fp16 planes unscaled, so the form is exact only for
 * |x| < FB_F16_RANGE = 32768 (h overflows from 65520 on, l already from 32768 on).  TensorFlow's fp32 (BrainDQN.py:119-155) has no such
 * limit; the reference network's activations are O(1 .. 100) and stay far inside, a net loaded from outside need not.  Every kernel that
 * splits an activation (acting trunk, training trunk, the large-batch weight-gradient kernels) therefore counts the waves that met
 * |x| >= FB_F16_RANGE in a device word instead of silently producing inf / NaN (or a finite wrong number behind the next relu):
 *   fb_qnet_overflow_count -> [host] the count since creation / the last reset (synchronous; 0 = every result so far is in range).
 * A non-zero count means: the Q-values / gradients of those launches are NOT to be trusted; switch the net to FB_DTYPE_BF16 (fp32's
 * exponent range) or rescale its weights.  VecBrain.run and the Brain* classes raise on it at their log cadence. */
int fb_qnet_overflow_count(fb_qnet_t h, int reset, int64_t *count_host);
/* Arithmetic of fb_qnet_train_step (BASELINE.json configs[2]: "bf16"):
 *   FB_DTYPE_F32  (default) fp32: the fc1 GEMMs of small batches on the fp32-input matrix instruction, everything else on two-plane fp16
 *                 (as above, gradient operands pre-scaled)
 *   FB_DTYPE_BF16 bf16 training: every GEMM operand (activations, weights, incoming gradients; conv1's u8 input is exact anyway)
 *                 is rounded to bf16, products accumulate in fp32, the master weights and both Adam slots stay fp32.  Gradients
 *                 then agree with fp32 ones to a few per cent per tensor (tests/test_gpu_configs.py states the bound). */
int fb_qnet_set_train_dtype(fb_qnet_t h, int dtype);
/* QValue.eval: states u8[B,80,80,4] -> q f32[B,A] */
int fb_qnet_forward(fb_qnet_t h, int which, const uint8_t *states, int batch, float *q, void *stream);
/* getAction for N envs: forward + epsilon-greedy (Philox stream 1, counter = step).
 *   epsilon f32 by value; actions u8[N] out; q f32[N,A] out or NULL */
int fb_qnet_act(fb_qnet_t h, const uint8_t *states, int n, float epsilon, uint64_t seed, uint64_t step,
                uint8_t *actions, float *q, void *stream);
/* One _trainQNetwork step on a gathered minibatch.
 *   isw f32[B] (PER) or NULL; loss f32[1]; abs_err f32[B] or NULL; q_target f32[B] or NULL (all [dev])
 *   flat_grad NULL : gradients are applied with Adam at once (single GPU)
 *   flat_grad [dev] f32[n_params]: gradients are only written there (data parallel: all-reduce
 *             them, then fb_qnet_apply_adam) */
/* fb_qnet_act on the env kernel's nibble states u8[n][FB_NIB_STRIDE] (fb_env_set_nib_buffer) */
int fb_qnet_act_nib(fb_qnet_t h, const uint8_t *nib_states, int n, float epsilon, uint64_t seed, uint64_t step,
                    uint8_t *actions, float *q, void *stream);
int fb_qnet_train_step(fb_qnet_t h, int algo, int batch, const uint8_t *s, const uint8_t *a, const float *r,
                       const uint8_t *s2, const uint8_t *t, const float *isw, double gamma, float *loss,
                       float *abs_err, float *q_target, float *flat_grad, void *stream);
int fb_qnet_apply_adam(fb_qnet_t h, const float *flat_grad, void *stream);
/* Data parallel, all-reduce off the critical path: a step that exports its gradient (flat_grad != NULL; fb_qnet_train_step,
 * fb_vec_step, fb_train_from_replay) records `event` (a hipEvent_t, or NULL to switch this off) on its stream right behind the
 * fc1 backward launch.  From that point flat_grad[fb_qnet_grad_split() ..) -- W_fc1, b_fc1 and the head, 91 % of the bytes -- is
 * final: reduce it on a side stream that waits for the event while the conv backward (3 more launches) still runs, reduce the
 * small front part [0, fb_qnet_grad_split()) on the step's stream afterwards, join, fb_qnet_apply_adam. */
int fb_qnet_set_grad_event(fb_qnet_t h, void *event);
int64_t fb_qnet_grad_split(fb_qnet_t h);
int fb_qnet_sync_target(fb_qnet_t h, void *stream);
/* Measurement aid (bench.py roofline): re-launch ONE kernel of the train-step plan `reps` times on
 * `stream` with the geometry the real step uses, on the workspace a preceding fb_qnet_train_step
 * of the same shape left behind.  Kernel ids count from 0; fb_qnet_kernel_name() returns "" past the
 * last one.  algo = -1 / -2 selects the acting forward (batch states as u8 / as nibble states).  The Adam kernel really updates the parameters: use a scratch network. */
int fb_qnet_profile_kernel(fb_qnet_t h, int kernel, int reps, int algo, int batch, const uint8_t *s, const uint8_t *a,
                           const float *r, const uint8_t *s2, const uint8_t *t, float *loss, void *stream);
const char *fb_qnet_kernel_name(int kernel);

/* ------------------------------------------------------------------ one whole step of the vectorised loop
 * FlappyBirdDQN.py:72-76 for N envs in ONE call: getAction (fb_qnet_act_nib) -> frame_step
 * (fb_env_step, packed frames) -> store + random.sample (fb_replay_push_sample) -> minibatch (fb_replay_gather)
 * -> _trainQNetwork (fb_qnet_train_step).  The results of exactly those calls in that order on `stream`.  It saves the
 * host's per-call overhead between launches (the GPU otherwise idles ~15 us per step waiting for the interpreter) and
 * four launches: the head of the acting forward (fc2 + epsilon-greedy action), random.sample and the Memory append
 * ride inside the env step launch (uniform memory, CPython generator, <= 2048 envs and 2 actions for the head; anything
 * else keeps its own launch), bit-identical to the separate calls.
 * With >= 256 envs the step skips the gather launch as well: the train step's first kernel reads the sampled
 * transitions' 1-bit frames in the ring itself (fb_train_from_replay below) -- same results, b->s / b->s2 stay untouched.
 * A prioritized memory (BrainPrioritizedReplyDQN.py:277-329) runs store -> Memory.sample -> train with the importance weights ->
 * Memory.batch_update in the same call (fb_replay_push, fb_replay_sample, fb_train_from_replay, fb_replay_update_priorities: no riders).
 * All pointers [dev], caller owned; nib is the buffer given to fb_env_set_nib_buffer.  train = 0 stops after the
 * store (the reference's OBSERVE phase).  flat_grad as in fb_qnet_train_step (data parallel: all-reduce it, then
 * fb_qnet_apply_adam).
 * A prioritized memory set to FB_PER_INIT_TD (fb_replay_set_priority_init): the call issues fb_replay_prime_priorities itself, on the online
 * net's acting output (f32 in either inference dtype) -- act (fb_qnet_act_nib) -> prime -> env step -> push, its store at max_p ->
 * Memory.sample -> train -> Memory.batch_update: the results of exactly those calls in that order, and at sampling time only the N newest
 * leaves are still at max_p.  (Inside the call the acting head still rides in the env launch and the prime launch sits behind it, in front
 * of the push's tree part: the env launch writes nothing the prime reads.)  Refused with FB_ERR_INVALID before any launch or counter change on such a memory: FB_ALGO_MDQN_PER (its target is not a max);
 * every C51 / QR / noisy algo and net (their priorities are losses, not |TD| of means); at n = 1 a gamma that is not the memory's
 * fb_replay_set_prime_gamma; fb_vec_step_dp; fb_sac_per_step, fb_iqn_per_step and their training calls.
 *
 * hipGraph capture.  State that decides what a launch does lives on the device (parameter / plane versions, Adam's step counter, the
 * sampler's generator, SumTree pointer / size, beta), so a captured call replays correctly -- with ONE exception: the replay memory's
 * push counter also has a host-side mirror (it is passed by value into the launches that address the frame ring), so a captured
 * launch that pushes or addresses the ring is only valid while the memory holds the number of pushes it held at capture time.
 *   capturable, replayable any number of times:  fb_qnet_forward / _act / _act_nib, fb_qnet_train_step, fb_qnet_apply_adam,
 *       fb_qnet_sync_target, fb_env_step, fb_replay_sample, fb_replay_update_priorities, and -- on a memory that is NOT pushed to
 *       between capture and the last replay -- fb_replay_gather, fb_train_from_replay and fb_train_steps (what bench.py's
 *       train-only leg does: fb_train_steps(10) in one graph)
 *   NOT capturable for replay:  fb_replay_push / _push_sample, fb_vec_step, fb_vec_step_dp (they advance the push counter: a replay
 *       would write the same ring slot again and sample a memory of the captured size); synchronous calls (get / set state, seeds,
 *       hyper-parameters, checkpoints) synchronise the device and must stay outside a capture. */
typedef struct {
    uint8_t *nib;                                   /* u8[N,FB_NIB_STRIDE] */
    uint8_t *actions;                               /* u8[N] out */
    uint64_t *frame_bits;                           /* u64[N,100] out */
    float *reward; uint8_t *terminal; int32_t *score;   /* [N] out */
    int64_t *idx;                                   /* i64[B] out */
    uint8_t *s, *s2, *a, *t; float *r;              /* gathered minibatch: u8[B,80,80,4] x2, u8[B], u8[B], f32[B] */
    float *loss;                                    /* f32[1] out */
    float *flat_grad;                               /* f32[n_params] or NULL */
    /* prioritized replay (algo = FB_ALGO_PER, FB_ALGO_DOUBLE_PER, FB_ALGO_MDQN_PER, the C51 and QR _PER algos; fb_iqn_per_step, fb_sac_per_step) only, else NULL: Memory.sample's importance weights as it returns them (f64[B]) and as the
     * float32 placeholder takes them (f32[B]), and the |TD errors| Memory.batch_update receives (f32[B]).
     * With the reference-order tree and 4096 envs or more Memory.batch_update of a step runs on the memory's own side stream, beside the NEXT step's acting
     * forward (its result is first needed by that step's Memory.store, which follows it there): idx and abs_err are read after
     * fb_vec_step has returned and must stay valid -- and unwritten by the caller -- until the next call on this memory.  Whichever
     * form Memory.batch_update takes (side stream or in line), abs_err holds |TD error| as the loss left it when fb_vec_step returns
     * (fb_replay_update_priorities, the stand-alone call, adds its 0.01 in place as the reference does,
     * BrainPrioritizedReplyDQN.py:147).  Any later call that touches the memory's tree joins that stream first. */
    double *isw; float *isw32; float *abs_err;
} fb_step_buffers;
/* The split schedule.  For a uniform memory with the CPython generator, 256 <= n_envs <= 8192, batch < 256, a 2-action net and a stream
 * that is not being captured, fb_vec_step keeps the train step on `stream` and puts the acting forward and the env step on a stream of the
 * net's own BESIDE it: in the reference's loop both read the weights the previous step's Adam left (FlappyBirdDQN.py:72-76), and the
 * minibatch depends on the env step only when it holds one of the n_envs transitions this very step appends -- the draw decides that on
 * the device and then waits for the env step itself (~3 % of the steps at 1024 envs / 1 M slots).  The two chains hand over through
 * device words that kernels store and single waves poll; every wait is bounded at 1 s and counted.  Results are those of the
 * one-stream order bit for bit.
 * On return everything the step produced is ordered on `stream`, so callers need not know -- with one exception: a step that exports
 * its gradient (flat_grad) is completed by fb_qnet_apply_adam / fb_dist_reduce_apply on the same stream, and only behind THAT call is
 * `stream` ordered behind the step's env launch (actions, rewards, terminals, scores, frame bits).
 * The first call with a given `stream` checks that the net's side stream really runs beside it (HIP may map both to one hardware queue
 * or pipe): it synchronises both streams a few times, ~1 ms, once; if no side stream passes, the step stays on one stream.
 *   fb_qnet_split_stats -> [host] steps issued that way / how many of their minibatches started beside the env step (synchronous);
 *                          FB_ERR_INVALID with the per-site counts if any wait between the chains gave up. */
int fb_qnet_split_stats(fb_qnet_t net, int64_t *steps_host, int64_t *clean_host);
/* Process-wide choice of the above (both schedules give the same results): split = 0 keeps every later fb_vec_step on one stream,
 * 1 (the default) takes the split schedule where it applies. */
int fb_vec_step_set_schedule(int split);
int fb_vec_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int algo, int batch,
                float epsilon, uint64_t seed, uint64_t step, int train, double gamma, void *stream);
/* The vector step of a SAC net (the SAC block above pins it): of *b it reads nib, actions, frame_bits, reward, terminal, score, idx, and for a
 * training step a, r, t, loss (f32[6]) and flat_grad (or NULL). */
int fb_sac_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch, uint64_t seed, uint64_t step,
                int train, double gamma, float rho, void *stream);
/* The vector step of a SAC net on a prioritized memory (the prioritized SAC block above pins it): the buffers fb_sac_step reads (idx for a
 * training step only), and for a training step isw, isw32 and abs_err as well. */
int fb_sac_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int batch, uint64_t seed, uint64_t step,
                    int train, double gamma, float rho, void *stream);
/* The vector step of an IQN net (the IQN block above pins it): of *b it reads nib, actions, frame_bits, reward, terminal, score, idx, and for a
 * training step a, r, t, loss (f32[1]) and flat_grad (or NULL). */
int fb_iqn_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q, int batch, float epsilon,
                uint64_t seed, uint64_t step, int train, double gamma, void *stream);
/* The vector step of an IQN net on a prioritized memory (the prioritized IQN block above pins it): the buffers fb_iqn_step reads, and for a
 * training step isw, isw32 and abs_err as well. */
int fb_iqn_per_step(fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int double_q, int batch, float epsilon,
                    uint64_t seed, uint64_t step, int train, double gamma, void *stream);

/* fb_replay_gather + fb_qnet_train_step WITHOUT the gathered copies (BrainDQN.py:197-223 from the indices on): the minibatch is
 * described by its indices, the conv trunk reads the replay's 1-bit frames directly (5 x 800 B per transition instead of writing and
 * re-reading 51 KB of u8 expansion) and fills a, r, t (u8 / f32 / u8 [batch], [dev] out).  Bit-identical to the two separate calls.
 * batch <= 256.  isw f32[batch] (the prioritized step's importance weights, idx then are SumTree leaf indices) or NULL; abs_err f32[batch]
 * out (|TD error|, for fb_replay_update_priorities) or NULL; flat_grad as in fb_qnet_train_step. */
int fb_train_from_replay(fb_replay_t replay, fb_qnet_t net, int algo, int batch, const int64_t *idx, const float *isw, uint8_t *a, float *r,
                         uint8_t *t, double gamma, float *loss, float *abs_err, float *flat_grad, void *stream);
/* Measurement aid: kernel `kernel` (ids of fb_qnet_kernel_name) of that step's plan, `reps` times, like fb_qnet_profile_kernel. */
int fb_profile_ring_kernel(fb_replay_t replay, fb_qnet_t net, int kernel, int reps, int algo, int batch, const int64_t *idx, uint8_t *a,
                           float *r, uint8_t *t, float *loss, void *stream);

/* ------------------------------------------------------------------ data parallel: one process per GPU, RCCL over xGMI
 * The only exchange between ranks is the all-reduce of the flat gradient between the backward pass and Adam (envs and replay shards are
 * rank-local).  fb_vec_step_dp = fb_vec_step(flat_grad) + that all-reduce + fb_qnet_apply_adam in one call, with RCCL called directly
 * on the step's own stream (no detour through another library's stream).  Optionally (fb_dist_set_overlap) in two pieces: the W_fc1 /
 * head part of the gradient (91 % of the bytes, final behind the fc1 backward launch) on a side stream while the conv backward still
 * runs, the conv part on the step's stream, then a join and Adam -- the same sums as one all-reduce of the whole vector.  mean_loss != 0 divides by the world size afterwards (the mean losses of
 * BrainDQNNature.py:119 / BrainPrioritizedReplyDQN.py:251; BrainDQN's sum loss, BrainDQN.py:162, is a plain sum).
 * Set-up: rank 0 calls fb_dist_unique_id, hands the 128 bytes to every rank by whatever channel the launcher has (the Python side
 * broadcasts them, dqnflappybird_amd/dist.py), every rank calls fb_dist_create (collective: ncclCommInitRank) with its HIP device current.
 * librccl_path: the librccl.so the process already holds (a Python host's framework usually bundles one), or NULL for the default search. */
typedef struct fb_dist *fb_dist_t;
/* rank-local, non-collective: 0 when this process can load RCCL and resolve its symbols.  Every rank calls it (and rank 0
 * fb_dist_unique_id) BEFORE the ranks agree to take this path; once the id has been exchanged a failure of fb_dist_create on one
 * rank leaves its peers inside ncclCommInitRank, so from there on a failure must end the job, not fall back. */
int fb_dist_probe(const char *librccl_path);
int fb_dist_unique_id(const char *librccl_path, uint8_t *id128 /*[host] out*/);
fb_dist_t fb_dist_create(const char *librccl_path, int rank, int world, const uint8_t *id128 /*[host]*/);
void fb_dist_destroy(fb_dist_t d);
/* 0 (default): one all-reduce of the whole gradient on the step's stream; 1: the two-piece schedule described above.  Every cross-stream
 * dependency costs 5-8 us on this hardware, so the two-piece schedule only pays when the 3.3 MB all-reduce takes longer than ~20 us. */
int fb_dist_set_overlap(fb_dist_t d, int overlap);
int fb_vec_step_dp(fb_dist_t d, fb_env_t env, fb_replay_t replay, fb_qnet_t net, const fb_step_buffers *b, int n_envs, int algo,
                   int batch, float epsilon, uint64_t seed, uint64_t step, int train, double gamma, int mean_loss, void *stream);
/* The reduction + Adam alone, for a gradient some other call exported (fb_qnet_train_step, fb_train_from_replay) after
 * fb_qnet_set_grad_event(net, fb_dist_grad_event(d)). */
int fb_dist_reduce_apply(fb_dist_t d, fb_qnet_t net, float *flat_grad /*[dev]*/, int mean_loss, void *stream);
void *fb_dist_grad_event(fb_dist_t d);
/* The collective alone: sum all-reduce of buf[count] (f32, [dev], in place) over the communicator, on `stream`.  For measurement
 * (bench.py config.allreduce_us) and for callers that schedule their own step. */
int fb_dist_all_reduce(fb_dist_t d, float *buf, int64_t count, void *stream);

/* n_steps x (fb_replay_sample -> fb_replay_gather -> fb_qnet_train_step) on a uniform memory in ONE call, same results: each step
 * trains from the replay's frame ring as fb_train_from_replay does (no gather), only the first draw is a launch of its own, and the
 * draw of step i + 1 rides in step i's conv3 backward launch (CPython generator; other generators keep their launches).
 * idx: i64[2 * batch] [dev], two buffers used alternately (step i: idx + (i & 1) * batch); a, r, t, loss as in fb_train_from_replay;
 * s, s2 must not be NULL but are not written. */
int fb_train_steps(fb_replay_t replay, fb_qnet_t net, int algo, int batch, int n_steps, int64_t *idx, uint8_t *s, uint8_t *s2,
                   uint8_t *a, float *r, uint8_t *t, float *loss, double gamma, void *stream);

/* ------------------------------------------------------------------ evaluation: greedy play of many games with a fixed net
 * What it evaluates: the reference's play loop (FlappyBirdDQN.py:72-76) with getAction (BrainDQN.py:99-116) at a fixed epsilon and
 * no training.  fb_eval_run(ev, net, n_envs, episodes, max_steps, epsilon, env_seed, act_seed, ...):
 *   start    env e (0 <= e < n_envs) starts as env e of fb_env_create(n_envs, env_seed, ...) does (gap stream keyed (env_seed, e)),
 *            its first frame stack as fb_env_observe leaves it;
 *   step     every live env takes the epsilon-greedy action of the net's ONLINE parameters (its inference dtype, plain or dueling)
 *            and makes one frame_step.  epsilon = 0: the argmax of the Q values fb_qnet_act_nib computes for that state (same tie
 *            rule).  epsilon > 0: fb_qnet_act's rule (uniform <= epsilon, then a uniform action) on a stream of its own, keyed
 *            (act_seed, env id, eval step) -- never the training acting stream, independent of the row an env occupies;
 *   records  when env e ends its k-th episode: score[e][k] = the score_return fb_env_step reports, length[e][k] = its frame_steps
 *            (the crashing one included), truncated[e][k] = 0.  After `episodes` episodes the env takes no more steps;
 *   stop     when every env is finished or after max_steps vector steps.  An env still running then records its in-progress
 *            episode (score and frame_steps so far, truncated = 1) if it has made a step of it.  Entries never reached keep
 *            length = 0 (score 0, truncated 0).  *steps_host = the vector steps taken;
 *   effects  none on anything a later training call reads (net parameters, target, Adam, step counter, env handles, replay,
 *            split schedule); the acting forward may re-split the net's inference planes of the same parameters (bit-identical).
 * score / length: i32[n_envs][episodes], truncated: u8[n_envs][episodes], [dev] caller owned.  1 <= n_envs <= min(FB_EVAL_MAX_ENVS,
 * the handle's max_envs), 1 <= episodes <= FB_EVAL_MAX_EPISODES, max_steps >= 1, 0 <= epsilon <= 1, a 2-action net: anything else is
 * FB_ERR_INVALID before any launch.
 * SYNCHRONOUS and NOT capturable: the work goes on `stream` behind what it holds (and behind the net's side stream, if it has one),
 * the call reads a live-env count through pinned memory once per 32 vector steps and returns with `stream` synchronised.  The
 * acting forward runs in passes of <= 3 * max_batch rows (the net's acting capacity).
 * fb_eval_stats: acting rows launched and compactions of the last fb_eval_run (host counters, no sync).
 * fb_eval_q: the Q values (f32[n][A], [dev]) of the acting forward fb_eval_run uses, for n nibble states (1 <= n <= 3 * max_batch):
 * the fused trunk at every n, so a state's Q values do not depend on n or on its row. */
#define FB_EVAL_MAX_ENVS 65536
#define FB_EVAL_MAX_EPISODES 64
typedef struct fb_eval *fb_eval_t;
int fb_eval_create(int max_envs, const void *sprite_blob, size_t blob_bytes, fb_eval_t *out);
int fb_eval_destroy(fb_eval_t ev);
int fb_eval_run(fb_eval_t ev, fb_qnet_t net, int n_envs, int episodes, int64_t max_steps, float epsilon, uint64_t env_seed,
                uint64_t act_seed, int32_t *score, int32_t *length, uint8_t *truncated, int64_t *steps_host, void *stream);
int fb_eval_stats(fb_eval_t ev, int64_t *rows_launched_host, int64_t *compactions_host);
int fb_eval_q(fb_qnet_t net, const uint8_t *nib_states, int n, float *q, void *stream);

#ifdef __cplusplus
}
#endif
#endif
