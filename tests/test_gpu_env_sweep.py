"""The env kernel over whole lattices of states (tests/envsweep.py) against the oracle env, bit for bit: the collision masks on every
(y, pipe x, gap, wing) at which bird and pipe rectangles overlap, the step's dynamics and pipe bookkeeping, and the observation's
pre-rendered pipe rows, bird rows and per-pixel rows on every table entry.  tests/test_env_sweep_host.py checks, from the oracle
alone, that the lattices reach those states.  Per chunk of at most 32 768 envs: set_state, one frame_step, read back."""
import numpy as np
import pytest

from tests import envsweep as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def env_of(torch_cuda):
    """VecGameState by env count, shared by the chunks of a lattice and by the tests (one holds a u8 frame buffer per env)"""
    from dqnflappybird_amd.vec import VecGameState
    made = {}

    def get(n):
        if n not in made:
            made[n] = VecGameState(n, seed=S.SEED)
        return made[n]
    yield get
    made.clear()


def step_on_device(torch, env_of, sweep):
    """one frame_step of every state of the sweep -> (post-step device states, reward, terminal, score)"""
    n = len(sweep.envs)
    post, rew = np.empty((n, 16), np.int32), np.empty(n, np.float32)
    term, score = np.empty(n, np.uint8), np.empty(n, np.int32)
    for lo in range(0, n, S.CHUNK):
        hi = min(n, lo + S.CHUNK)
        env = env_of(hi - lo)
        env.set_state(sweep.dev[lo:hi])
        env.frame_step(torch.from_numpy(sweep.actions[lo:hi].copy()).cuda(), want_u8=False)
        post[lo:hi] = env.get_state()
        rew[lo:hi], term[lo:hi], score[lo:hi] = env.reward.cpu().numpy(), env.terminal.cpu().numpy(), env.score.cpu().numpy()
        assert env.error_count() == 0
    print(f"stepped {n} states in {-(-n // S.CHUNK)} chunk(s): {int(term.sum())} crashes, {int((rew == np.float32(3.0)).sum())} scoring")
    return post, rew, term, score


def assert_outcomes_equal(s, post, rew, term, score):
    """reward, terminal, score and the full post-step state of every env == the oracle's; the first few lattice points that differ
    are reported with both outcomes"""
    bad = (rew != s.reward) | (term != s.terminal) | (score != s.score) | S.post_state_mismatch(post, s.post)
    if bad.any():
        lines = []
        for i in np.flatnonzero(bad)[:8]:
            at = {k: int(v[i]) for k, v in s.sweep.coords.items()}
            lines.append(f"{at}: kernel (reward, terminal, score) = {(float(rew[i]), int(term[i]), int(score[i]))}, oracle "
                         f"{(float(s.reward[i]), int(s.terminal[i]), int(s.score[i]))}\n    kernel state {post[i].tolist()}\n"
                         f"    oracle snapshot {S.snapshot(s.post[i:i + 1])[0].tolist()} phase {int(s.post['cyc_pos'][i])} counter {int(s.post['rng_ctr'][i])}")
        pytest.fail(f"{int(bad.sum())} of {len(bad)} states differ from the oracle:\n" + "\n".join(lines))


def test_collision_lattice(torch_cuda, env_of):
    """A: all 775 200 targets y 0..379 x pipe x 6..90 x gap x wing, 76 % of them crashes (then both sides reset and draw the same
    two gaps), 27 424 with overlapping rectangles and no opaque pixels in common -- the states the 64-bit row masks, the reversed
    upper-pipe mask and the shift d = 57 - x decide."""
    s = S.stepped("A")
    assert_outcomes_equal(s, *step_on_device(torch_cuda, env_of, s.sweep))


def test_dynamics_lattice(torch_cuda, env_of):
    """B: y x velY x action (ceiling, flap, velocity cap, ground at 379 / 380), loopIter x wing phase x basex, and the pipe list's
    spawn / removal / score windows at 2 and 3 pipes."""
    s = S.stepped("B")
    assert_outcomes_equal(s, *step_on_device(torch_cuda, env_of, s.sweep))


def unpack_bits(bits):
    """frame_bits i64[n,100] -> bool[n,80,80]"""
    return np.unpackbits(np.ascontiguousarray(bits).view(np.uint8).reshape(len(bits), 800), axis=1, bitorder="little").reshape(-1, 80, 80) != 0


def assert_bits_equal(s, got, want, what):
    bad = (got != want).any(axis=1)
    if bad.any():
        lines = []
        for i in np.flatnonzero(bad)[:6]:
            px = np.argwhere(unpack_bits(got[i:i + 1])[0] != unpack_bits(want[i:i + 1])[0])
            lines.append(f"{ {k: int(v[i]) for k, v in s.sweep.coords.items()} } terminal {int(s.terminal[i])}: {len(px)} pixels, first (row, column) {px[:6].tolist()}")
        pytest.fail(f"{what}: {int(bad.sum())} of {len(bad)} frames differ from the oracle's:\n" + "\n".join(lines))


def check_frames(torch, name):
    """frame_bits of the step == the oracle's 80x80 frame of every post-step state (the reset frame after a crash); the u8 frames,
    observe() on the post-step state and the nibble image's newest frame say the same."""
    from dqnflappybird_amd.vec import VecGameState
    from tests.test_gpu_shims import unpack_nib
    s, want = S.stepped(name), S.stepped_frames(name)
    n = len(s.post)
    assert n <= S.CHUNK
    env = VecGameState(n, seed=S.SEED)
    nib = env.track_state()
    acts = torch.from_numpy(s.sweep.actions.copy()).cuda()
    env.set_state(s.sweep.dev)
    env.observe()                                           # the agent's stack: four copies of the pre-step observation
    before = env.frame_bits.cpu().numpy()
    assert_bits_equal(s, before, S.pack_frames(S.oracle_frames(s.sweep.envs)), f"{name}: observe() before the step")
    env.frame_step(acts, want_u8=False)
    step_bits = env.frame_bits.clone()
    assert_outcomes_equal(s, env.get_state(), env.reward.cpu().numpy(), env.terminal.cpu().numpy(), env.score.cpu().numpy())
    assert_bits_equal(s, step_bits.cpu().numpy(), want, f"{name}: frame_step")
    for lo in range(0, n, 512):                             # newest frame in every nibble's top bit, the pre-step one below it
        stack = unpack_nib(nib[lo:lo + 512]) != 0
        assert np.array_equal(stack[..., 3], unpack_bits(want[lo:lo + 512])), lo
        assert all(np.array_equal(stack[..., f], unpack_bits(before[lo:lo + 512])) for f in range(3)), lo
    env.frame_bits.zero_()
    frames = env.observe()                                  # observe() of the post-step state writes the frame the step wrote
    assert torch.equal(env.frame_bits, step_bits)
    assert np.array_equal(frames.cpu().numpy(), unpack_bits(want) * np.uint8(255))
    assert np.array_equal(unpack_nib(nib[:512]) != 0, np.repeat(unpack_bits(want[:512])[..., None], 4, axis=-1))      # (setInitState: four copies)
    env.set_state(s.sweep.dev)                              # the same step again, u8 frames wanted
    env.frames.fill_(7)
    frames, _, _, _ = env.frame_step(acts, want_u8=True)
    assert np.array_equal(frames.cpu().numpy(), unpack_bits(want) * np.uint8(255)) and torch.equal(env.frame_bits, step_bits)
    assert env.error_count() == 0


def test_frames_pipe_tables(torch_cuda):
    """C: first pipe at every x 298..-56 x gap, two and three pipes: every (gap, dx, row phase) entry of the pre-rendered pipe rows."""
    check_frames(torch_cuda, "C")


def test_frames_bird_table(torch_cuda):
    """D: bird at every y 0..379 x wing with its rows free of pipes: every entry and shift of the pre-rendered bird rows."""
    check_frames(torch_cuda, "D")


def test_frames_slow_rows(torch_cuda):
    """E: 3000 surviving and 1000 crashing states of A, every basex: bird and pipe in the same observation rows (per-pixel path)."""
    check_frames(torch_cuda, "E")


def render_states():
    """48 states: every basex (i % 12) and wing (i % 3); 12 each with the bird's rectangle over the upper pipe, over the lower pipe,
    with three pipes (the first partly off screen), and in free flight from the ceiling to the ground."""
    i = np.arange(48)
    kind, k, g = i // 12, i % 12, i % 8
    gy = 100 + 10 * g
    y = np.choose(kind, [gy - 12, gy + S.GAP - 12, gy + 38, np.minimum(k * 35, 379)])
    x0 = np.choose(kind, [40 + 3 * k, 40 + 3 * k, -10 - 4 * k, np.full(48, 150)])
    three = kind == 2
    px = np.stack([x0, x0 + 144, np.where(three, x0 + 294, 0)], 1)
    pg = np.stack([g, (g + 3) % 8, np.where(three, (g + 5) % 8, 0)], 1)
    return S.build(dict(i=i), y, 0, i % 3, i % 30, -4 * k, i % 4, i % 7, np.where(three, 3, 2), px, pg, 2, 0)


def test_render_full_on_swept_states(torch_cuda, env_of):
    sw = render_states()
    want = S.oracle_render_full(sw.envs)
    env = env_of(48)
    env.set_state(sw.dev)
    for e in range(48):
        got = env.render_full(e).cpu().numpy()
        assert np.array_equal(got, want[e]), (sw.dev[e].tolist(), np.argwhere((got != want[e]).any(axis=-1))[:5].tolist())


@pytest.mark.parametrize("n_frames", [1, 3, 17])
def test_preprocess_batches(torch_cuda, oracle, env_of, n_frames):
    """fb_preprocess_rgb on batches (the preprocess shim only ever passes one frame): oracle full renders and uint8 noise, mixed;
    every output frame == oracle.preprocess of that frame, and nothing is written behind the batch."""
    torch = torch_cuda
    from dqnflappybird_amd import _lib as L
    renders = S.oracle_render_full(render_states().envs[(n_frames + 5 * np.arange(n_frames)) % 48])
    rng = np.random.default_rng(n_frames)
    batch = np.stack([renders[f] if f % 2 == 0 else rng.integers(0, 256, (288, 512, 3), dtype=np.uint8) for f in range(n_frames)])
    rgb = torch.from_numpy(batch).cuda()
    out = torch.full((n_frames + 1, 80, 80), 7, dtype=torch.uint8, device="cuda")
    L.check(L.lib().fb_preprocess_rgb(env_of(48).h, L.ptr(rgb), n_frames, L.ptr(out), L.current_stream()), "fb_preprocess_rgb")
    got = out.cpu().numpy()
    for f in range(n_frames):
        assert np.array_equal(got[f], oracle.preprocess(batch[f])), f
    assert (got[n_frames] == 7).all()
