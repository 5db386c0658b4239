"""State-space sweeps of the env kernel against the oracle env (oracle/fbo_env.c).

The env kernel (csrc/fb_env.hip) restates the game through tables: 64-bit hit masks for the collision test, pre-rendered pipe and bird
rows for the observation, a per-pixel path only for rows where bird and pipe meet.  A trajectory visits a thin thread of the states
those tables serve; the lattices here enumerate them.  Every lattice names its POST-step target and builds the pre-state that reaches
it in one frame_step: with action 0, velY = -1 and loopIter = 0 the step leaves y and the wing pose alone and moves every pipe by 4.

A sweep holds the same states twice: as a numpy structured array of np.dtype(oracle.Env), which the oracle steps in place, element by
element (oracle_step) or renders (oracle_frames), and in the device's i32[N,16] layout (include/fbdqn.h, fb_env_get_state).  seed,
env id (the env's index inside its device chunk of at most CHUNK envs), the gap stream's counter and the wing generator's phase are
set alike on both sides: a crash resets the env, and both sides then draw the same two Philox gaps.

Not a conftest and not a test module: imported by tests/test_env_sweep_host.py and tests/test_gpu_env_sweep.py."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from oracle import oracle as O
from tests.test_gpu_env import dev_state_to_snapshot  # noqa: F401  (the per-env form of device_snapshot; the host test ties the two)

ENV = np.dtype(O.Env)
CHUNK = 32768                  # envs per VecGameState: above the step launch's 2048 workgroups, so a workgroup's first-env and strided-env paths both run
SEED = 0x5EED_0BAD_CAFE        # key of every chunk's gap stream (both halves non-zero)
PLAYERX, BIRD_W, BIRD_H, PIPE_W, PIPE_H, GAP = 57, 34, 24, 52, 320, 100

A_Y, A_X, A_GAPS, A_WINGS = np.arange(380), np.arange(6, 91), np.arange(8), np.arange(3)
A_SHAPE = (len(A_Y), len(A_X), len(A_GAPS), len(A_WINGS))

Sweep = namedtuple("Sweep", "envs dev actions coords")       # coords: dict of per-state int arrays naming the lattice point
Stepped = namedtuple("Stepped", "sweep post reward terminal score")


# ----------------------------------------------------------------------------- the oracle over arrays
def _fn(name, *argtypes):
    """a private prototype of an oracle function (the shared CDLL's argtypes stay as oracle.py set them)"""
    return C.CFUNCTYPE(C.c_int, *argtypes)((name, O.lib()))


def oracle_step(envs, actions):
    """fbo_env_step on every element of `envs`, in place -> (reward f32[n], terminal u8[n], score i32[n])"""
    assert envs.dtype == ENV and envs.flags.c_contiguous and envs.flags.writeable and len(actions) == len(envs)
    n = len(envs)
    step = _fn("fbo_env_step", C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)
    rew, term, score = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32)
    e0, r0, t0, s0, sz = envs.ctypes.data, rew.ctypes.data, term.ctypes.data, score.ctypes.data, ENV.itemsize
    for i, a in enumerate(np.asarray(actions).tolist()):
        if step(e0 + sz * i, a, r0 + 4 * i, t0 + 4 * i, s0 + 4 * i) != 0:
            raise ValueError("Multiple input actions!")
    return rew, term.astype(np.uint8), score


def oracle_frames(envs):
    """fbo_env_frame80 of every element -> u8[n,80,80]"""
    assert envs.dtype == ENV and envs.flags.c_contiguous
    out = np.empty((len(envs), 80, 80), np.uint8)
    frame = _fn("fbo_env_frame80", C.c_void_p, C.c_void_p)
    e0, o0 = envs.ctypes.data, out.ctypes.data
    for i in range(len(envs)):
        frame(e0 + ENV.itemsize * i, o0 + 6400 * i)
    return out


def oracle_render_full(envs):
    """fbo_env_render_full of every element -> u8[n,288,512,3]"""
    assert envs.dtype == ENV and envs.flags.c_contiguous
    out = np.empty((len(envs), 288, 512, 3), np.uint8)
    render = _fn("fbo_env_render_full", C.c_void_p, C.c_void_p)
    for i in range(len(envs)):
        render(envs.ctypes.data + ENV.itemsize * i, out.ctypes.data + out[0].nbytes * i)
    return out


def oracle_snapshot_each(envs):
    """fbo_env_snapshot, one call per element -> i32[n,16] (what snapshot() must equal)"""
    assert envs.dtype == ENV and envs.flags.c_contiguous
    out = np.empty((len(envs), 16), np.int32)
    snap = _fn("fbo_env_snapshot", C.c_void_p, C.c_void_p)
    for i in range(len(envs)):
        snap(envs.ctypes.data + ENV.itemsize * i, out.ctypes.data + 64 * i)
    return out


def pack_frames(frames):
    """u8[n,80,80] -> the kernel's frame_bits i64[n,100], as tests/test_gpu_env.py packs one frame"""
    return np.packbits(frames.reshape(len(frames), 6400) != 0, axis=1, bitorder="little").view(np.int64)


# ----------------------------------------------------------------------------- layouts
def _snapshot(y, fields7, n_pipes, pipe_x, pipe_gap):
    out = np.zeros((len(y), 16), np.int32)
    out[:, 0] = y
    out[:, 1:7] = fields7
    live = np.arange(3)[None, :] < n_pipes[:, None]
    gy = 100 + 10 * pipe_gap
    out[:, 7:10] = np.where(live, pipe_x, -9999)
    out[:, 10:13] = np.where(live, gy - PIPE_H, 0)
    out[:, 13:16] = np.where(live, gy + GAP, 0)
    return out


def snapshot(envs):
    """Env array -> i32[n,16] in the snapshot layout of fbo_env_snapshot / the fixtures, without a per-element call"""
    f = np.stack([envs[k] for k in ("vely", "player_index", "loop_iter", "basex", "score", "n_pipes")], axis=1)
    return _snapshot(envs["playery"].astype(np.int32), f, envs["n_pipes"], envs["pipe_x"], envs["pipe_gap"])


def device_snapshot(st):
    """device i32[n,16] -> the same snapshot layout: dev_state_to_snapshot of tests/test_gpu_env.py for all envs at once"""
    st = np.asarray(st, np.int32)
    return _snapshot(st[:, 0], st[:, 1:7], st[:, 6], st[:, 7:10], st[:, 10:13])


def device_state(envs):
    """Env array -> the device's i32[n,16] (include/fbdqn.h); word 15, the tape cursor, stays 0: the sweeps draw from Philox"""
    st = np.zeros((len(envs), 16), np.int32)
    st[:, 0] = envs["playery"].astype(np.int32)
    for w, k in enumerate(("vely", "player_index", "loop_iter", "basex", "score", "n_pipes"), start=1):
        st[:, w] = envs[k]
    st[:, 7:10], st[:, 10:13] = envs["pipe_x"], envs["pipe_gap"]
    st[:, 13], st[:, 14] = envs["cyc_pos"], envs["rng_ctr"].astype(np.int32)
    return st


def post_state_mismatch(dev_post, orc_post):
    """bool[n]: the device's post-step state differs from the oracle's -- the snapshot's 16 words (dead pipe slots are not state: the
    oracle leaves the removed pipe's values behind, the kernel zeroes them), the wing generator's phase, the gap counter, the unused
    tape cursor"""
    bad = (device_snapshot(dev_post) != snapshot(orc_post)).any(axis=1)
    bad |= (dev_post[:, 13] != orc_post["cyc_pos"]) | (dev_post[:, 14] != orc_post["rng_ctr"].astype(np.int32)) | (dev_post[:, 15] != 0)
    return bad


# ----------------------------------------------------------------------------- state builders
def build(coords, y, vely, wing, loop_iter, basex, cyc_pos, score, n_pipes, pipe_x, pipe_gap, rng_ctr, action):
    """Every argument broadcasts to the number of states n (pipe_x / pipe_gap to [n,3]; slots >= n_pipes must be 0)."""
    pipe_x, pipe_gap = np.asarray(pipe_x), np.asarray(pipe_gap)
    n = max([np.size(v) for v in (y, vely, wing, loop_iter, basex, cyc_pos, score, n_pipes, rng_ctr, action)] + [pipe_x.size // 3, pipe_gap.size // 3])
    envs = np.zeros(n, ENV)
    envs["playery"], envs["vely"], envs["player_index"], envs["loop_iter"] = y, vely, wing, loop_iter
    envs["basex"], envs["cyc_pos"], envs["score"], envs["n_pipes"] = basex, cyc_pos, score, n_pipes
    envs["pipe_x"], envs["pipe_gap"] = pipe_x, pipe_gap
    envs["seed_lo"], envs["seed_hi"] = SEED & 0xFFFFFFFF, SEED >> 32
    envs["env_id"], envs["rng_ctr"] = np.arange(n) % CHUNK, rng_ctr
    live = np.arange(3)[None, :] < envs["n_pipes"][:, None]
    assert ((envs["n_pipes"] >= 2) & (envs["n_pipes"] <= 3)).all() and not envs["pipe_x"][~live].any() and not envs["pipe_gap"][~live].any()
    assert (envs["playery"] >= 0).all() and (envs["playery"] < 380).all() and (envs["pipe_gap"] >= 0).all() and (envs["pipe_gap"] < 8).all()
    assert (envs["basex"] <= 0).all() and (envs["basex"] > -48).all() and (envs["basex"] % 4 == 0).all()
    actions = np.broadcast_to(np.asarray(action, np.uint8), (n,)).copy()
    coords = {k: np.broadcast_to(np.asarray(v), (n,)) for k, v in coords.items()}
    return Sweep(envs, device_state(envs), actions, coords)


def reach(coords, y, wing, pipe_x_post, pipe_gap, n_pipes=2, basex=0):
    """The pre-states that reach the target (y, wing, pipe x) in one frame_step: action 0, velY -1 -> 0, loopIter 0 -> 1 (no wing
    change), every live pipe 4 further right.  Score, wing-generator phase and gap counter vary with the index so that neither side
    can pass with a constant."""
    pipe_x_post = np.asarray(pipe_x_post)
    n = pipe_x_post.size // 3
    i = np.arange(n)
    live = np.arange(3)[None, :] < np.broadcast_to(np.asarray(n_pipes), (n,))[:, None]
    return build(coords, y, -1, wing, 0, basex, i % 4, i % 7, n_pipes, np.where(live, pipe_x_post.reshape(n, 3) + 4, 0), pipe_gap,
                 2 + 2 * (i % 5), 0)


def lattice_a():
    """A. Collision, exhaustive: target y 0..379 x first pipe's x 6..90 (every x at which its rectangle overlaps the bird's columns
    57..90) x gap index x wing pose; the second pipe 144 further right with another gap."""
    y, x, g, w = (v.reshape(-1) for v in np.meshgrid(A_Y, A_X, A_GAPS, A_WINGS, indexing="ij"))
    px = np.stack([x, x + 144, np.zeros_like(x)], axis=1)
    pg = np.stack([g, (g + 3) % 8, np.zeros_like(g)], axis=1)
    return reach(dict(y=y, x=x, gap=g, wing=w), y, w, px, pg)


def _safe_y(g):
    return 100 + 10 * g + 38         # the middle of the gap: 38 free rows above and below the bird


def lattice_b():
    """B. Dynamics.  (1) pre-state y 0..379 x velY -9..10 x action, pipes far from the bird: ceiling clamp, flap rule, velocity cap,
    the ground boundary at 379 / 380.  (2) a fixed-seed sample of 4096 of those x loopIter 0..29, with the wing generator's 4 phases
    and the 12 basex values running through the sample (every (loopIter, phase, basex) occurs).  (3) pipe bookkeeping, bird safe in
    the gap: first pipe's pre-step x 56..-56 at 2 pipes (score window 45..48 after the step, spawn window 1..4, removal below -52)
    and 4..-56 at 3 pipes (a third pipe only exists once the first has reached the spawn window) with the third pipe at the two
    reachable residues x0 + 294 / x0 + 296, x every gap index x action."""
    y, v, a = (q.reshape(-1) for q in np.meshgrid(np.arange(380), np.arange(-9, 11), np.arange(2), indexing="ij"))
    n1 = len(y)
    far_x, far_g = np.array([[200, 344, 0]]), np.array([[2, 6, 0]])
    i = np.arange(n1)
    parts = [dict(y=y, vely=v, action=a, loop_iter=np.full(n1, 2), cyc_pos=i % 4, basex=-4 * (i % 12), n_pipes=np.full(n1, 2),
                  pipe_x=np.repeat(far_x, n1, 0), pipe_gap=np.repeat(far_g, n1, 0))]
    pick = np.sort(np.random.default_rng(20261019).choice(n1, 4096, replace=False))
    s, li = (q.reshape(-1) for q in np.meshgrid(np.arange(4096), np.arange(30), indexing="ij"))
    parts.append(dict(y=y[pick][s], vely=v[pick][s], action=a[pick][s], loop_iter=li, cyc_pos=s % 4, basex=-4 * ((s // 4) % 12),
                      n_pipes=np.full(len(s), 2), pipe_x=np.repeat(far_x, len(s), 0), pipe_gap=np.repeat(far_g, len(s), 0)))
    rows = []
    for x0 in range(56, -57, -1):
        for g in range(8):
            for act in (0, 1):
                rows.append((x0, g, act, 2, 0))
                if x0 <= 4:
                    rows += [(x0, g, act, 3, x0 + 294), (x0, g, act, 3, x0 + 296)]
    x0, g, act, npipes, x2 = np.array(rows).T
    n3 = len(x0)
    i = np.arange(n3)
    parts.append(dict(y=_safe_y(g), vely=np.zeros(n3, int), action=act, loop_iter=i % 30, cyc_pos=i % 4, basex=-4 * (i % 12), n_pipes=npipes,
                      pipe_x=np.stack([x0, x0 + 144, x2], 1), pipe_gap=np.stack([g, np.where(g < 7, g + 1, 6), np.where(npipes == 3, (g + 5) % 8, 0)], 1)))      # (a neighbouring gap: the bird also clears the second pipe, which reaches its columns at x0 <= -54)
    f = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    n = len(f["y"])
    i = np.arange(n)
    part = np.repeat(np.arange(3), [len(p["y"]) for p in parts])
    return build(dict(part=part, y=f["y"], vely=f["vely"], action=f["action"], loop_iter=f["loop_iter"], x0=f["pipe_x"][:, 0], n_pipes=f["n_pipes"]),
                 f["y"], f["vely"], i % 3, f["loop_iter"], f["basex"], f["cyc_pos"], i % 7, f["n_pipes"], f["pipe_x"], f["pipe_gap"],
                 2 + 2 * (i % 5), f["action"])


def lattice_c():
    """C. Pipe render tables: first pipe's target x 298..-56 x gap index, bird at y 244 with wing = x mod 3.  Right of x = 0 two
    pipes (the step itself spawns the third at x 1..4); from x = 0 down three, the third at the two reachable residues (the step
    removes the first below -52)."""
    x, g = (q.reshape(-1) for q in np.meshgrid(np.arange(298, -57, -1), np.arange(8), indexing="ij"))
    three = x <= 0
    px = np.stack([x, x + 144, np.where(three, x + 294 + 2 * (g & 1), 0)], 1)
    pg = np.stack([g, (g + 3) % 8, np.where(three, (g + 5) % 8, 0)], 1)
    return reach(dict(x=x, gap=g), 244, x % 3, px, pg, n_pipes=np.where(three, 3, 2), basex=-4 * (np.arange(len(x)) % 12))


def lattice_d():
    """D. Bird render table: y 0..379 x wing pose, no pipe over the bird's rows (pipes at x 150 and 294)."""
    y, w = (q.reshape(-1) for q in np.meshgrid(np.arange(380), np.arange(3), indexing="ij"))
    n = len(y)
    return reach(dict(y=y, wing=w), y, w, np.repeat([[150, 294, 0]], n, 0), np.repeat([[1, 5, 0]], n, 0), basex=-4 * (np.arange(n) % 12))


def lattice_e():
    """E. Slow rows (bird and pipe in the same observation rows): a fixed-seed sample of 3000 non-crashing and 1000 crashing states of
    lattice A (a crash yields the reset frame), crossed cyclically with the 12 basex values."""
    a = stepped("A")
    rng = np.random.default_rng(20261020)
    alive, dead = np.flatnonzero(a.terminal == 0), np.flatnonzero(a.terminal != 0)
    pick = np.concatenate([np.sort(rng.choice(alive, 3000, replace=False)), np.sort(rng.choice(dead, 1000, replace=False))])
    c = {k: v[pick] for k, v in a.sweep.coords.items()}
    x, g = c["x"], c["gap"]
    px = np.stack([x, x + 144, np.zeros_like(x)], 1)
    pg = np.stack([g, (g + 3) % 8, np.zeros_like(g)], 1)
    return reach(c, c["y"], c["wing"], px, pg, basex=-4 * (np.arange(len(pick)) % 12))


LATTICES = dict(A=lattice_a, B=lattice_b, C=lattice_c, D=lattice_d, E=lattice_e)


@functools.lru_cache(maxsize=None)
def stepped(name):
    """The lattice and the oracle's one step on it, computed once per process and read-only from then on."""
    sweep = LATTICES[name]()
    post = sweep.envs.copy()
    rew, term, score = oracle_step(post, sweep.actions)
    for arr in (sweep.envs, sweep.dev, sweep.actions, post, rew, term, score):
        arr.flags.writeable = False
    return Stepped(sweep, post, rew, term, score)


@functools.lru_cache(maxsize=None)
def stepped_frames(name):
    """the oracle's 80x80 frame of every post-step state of a lattice, packed like the kernel's frame_bits"""
    bits = pack_frames(oracle_frames(stepped(name).post))
    bits.flags.writeable = False
    return bits


# ----------------------------------------------------------------------------- coverage, from the oracle alone
def rect_overlap_a():
    """bool[n] over lattice A's targets: the bird's rectangle overlaps a pipe rectangle (pygame's clip is non-empty).  The first
    pipe's columns x..x+51 meet the bird's 57..90 at every x of the lattice and the second pipe's never do, so only the rows decide:
    the upper pipe ends above gapY, the lower one starts at gapY + 100."""
    c = stepped("A").sweep.coords
    gy = 100 + 10 * c["gap"]
    assert ((c["x"] < PLAYERX + BIRD_W) & (c["x"] + PIPE_W > PLAYERX) & (c["x"] + 144 >= PLAYERX + BIRD_W)).all()
    return (c["y"] < gy) | (c["y"] + BIRD_H > gy + GAP)


@functools.lru_cache(maxsize=None)
def resize_taps():
    """(xo[80], yo[80]): the first of the two source rows (game x) / source columns (game y) that cv2.resize reads for every output
    row / column, from impulse responses of the oracle's preprocess (tests/test_oracle_env.py::test_resize_taps_match_survey_probe:
    light one source line, see which output lines answer)."""
    xo, yo = np.full(80, -1), np.full(80, -1)
    for sx in range(288):
        img = np.zeros((288, 512, 3), np.uint8)
        img[sx] = 255
        for r in np.flatnonzero(O.preprocess(img).any(axis=1)):
            if xo[r] < 0:
                xo[r] = sx
    for sy in range(512):
        img = np.zeros((288, 512, 3), np.uint8)
        img[:, sy] = 255
        for c in np.flatnonzero(O.preprocess(img).any(axis=0)):
            if yo[c] < 0:
                yo[c] = sy
    assert (xo >= 0).all() and (yo >= 0).all()
    return xo, yo


def bird_rows():
    """bool[80]: observation rows with a source row among the bird's columns 57..90"""
    xo, _ = resize_taps()
    return (xo + 1 >= PLAYERX) & (xo < PLAYERX + BIRD_W)


def pipe_table_cover(envs):
    """bool[8 gaps, 53 dx, 5 phases]: the pre-rendered pipe rows that the frames of `envs` use.  An observation row r with first
    source row xo[r] meets a live pipe at x when dx = xo[r] - x + 1 lies in 0..52 (one of its two source rows is a pipe column); its
    tap weights repeat every 5 rows (3.6 * 5 = 18 source rows), which is the phase.  Rows that also meet the bird are left out: they
    are rendered per pixel (lattice E), not from the table."""
    xo, _ = resize_taps()
    assert (xo[5:] == xo[:-5] + 18).all()
    cover = np.zeros((8, PIPE_W + 1, 5), bool)
    for r in np.flatnonzero(~bird_rows()):
        for i in range(3):
            dx = xo[r] - envs["pipe_x"][:, i] + 1
            m = (i < envs["n_pipes"]) & (dx >= 0) & (dx <= PIPE_W)
            cover[envs["pipe_gap"][m, i], dx[m], r % 5] = True
    return cover


def slow_row_cover(envs):
    """int[80]: in how many of `envs` observation row r meets the bird and a live pipe"""
    xo, _ = resize_taps()
    count = np.zeros(80, int)
    for r in np.flatnonzero(bird_rows()):
        m = np.zeros(len(envs), bool)
        for i in range(3):
            dx = xo[r] - envs["pipe_x"][:, i] + 1
            m |= (i < envs["n_pipes"]) & (dx >= 0) & (dx <= PIPE_W)
        count[r] = m.sum()
    return count
