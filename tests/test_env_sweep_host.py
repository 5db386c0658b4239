"""tests/envsweep.py on the host: the vectorised layouts against the oracle's own, and what the lattices cover.

The coverage figures are CONDITIONS on the sweeps, computed from the oracle alone (no kernel, no kernel table is read): if a lattice
stopped reaching the states where the env kernel's bit masks and pre-rendered rows matter, the GPU sweeps would pass vacuously."""
import numpy as np

from tests import envsweep as S


def test_lattice_sizes_and_domain():
    """Lattice A has exactly 775 200 states; every pre-state is in the domain fb_env_set_state documents (build() asserts it) and
    every post-step y stays in 0..379."""
    sizes = {n: len(S.stepped(n).post) for n in "ABCDE"}
    print("lattice sizes", sizes)
    assert sizes == dict(A=775200, B=15200 + 4096 * 30 + 3760, C=355 * 8, D=1140, E=4000)
    for n in "ABCDE":
        s = S.stepped(n)
        assert s.sweep.envs.dtype == S.ENV and S.ENV.itemsize == 104 and s.sweep.dev.shape == (sizes[n], 16) and s.sweep.dev.dtype == np.int32
        assert (s.post["playery"] >= 0).all() and (s.post["playery"] < 380).all() and (s.post["playery"] == np.floor(s.post["playery"])).all()
        assert (s.sweep.envs["env_id"] == np.arange(sizes[n]) % S.CHUNK).all()
    a = S.stepped("A")
    c = a.sweep.coords
    ok = a.terminal == 0                         # the targets are reached: a surviving state IS its lattice point
    assert (a.post["playery"][ok] == c["y"][ok]).all() and (a.post["pipe_x"][ok, 0] == c["x"][ok]).all()
    assert (a.post["player_index"][ok] == c["wing"][ok]).all() and (a.post["pipe_gap"][ok, 0] == c["gap"][ok]).all()


def test_builders_are_deterministic():
    for name in "BCDE":
        one, two = S.LATTICES[name](), S.LATTICES[name]()
        assert one.envs.tobytes() == two.envs.tobytes() and np.array_equal(one.dev, two.dev) and np.array_equal(one.actions, two.actions)
        assert one.envs.tobytes() == S.stepped(name).sweep.envs.tobytes()
    assert S.lattice_a().envs.tobytes() == S.stepped("A").sweep.envs.tobytes()


def test_vectorised_snapshot_equals_the_oracles():
    """snapshot() == fbo_env_snapshot per element on every state of B (before and after the step: dead pipe slots, removed and
    spawned pipes) and on a sample of A; device_snapshot(device_state()) is the same thing, and equals dev_state_to_snapshot."""
    b, a = S.stepped("B"), S.stepped("A")
    pick = np.sort(np.random.default_rng(3).choice(len(a.post), 20000, replace=False))
    for envs in (b.sweep.envs, b.post, a.sweep.envs[pick], a.post[pick]):
        envs = np.ascontiguousarray(envs)
        want = S.oracle_snapshot_each(envs)
        assert np.array_equal(S.snapshot(envs), want)
        dev = S.device_state(envs)
        live = np.arange(3)[None, :] < envs["n_pipes"][:, None]
        dev[:, 7:10][~live] = 0; dev[:, 10:13][~live] = 0          # (what the kernel leaves in a dead slot)
        assert np.array_equal(S.device_snapshot(dev), want)
        for i in range(0, len(envs), 97):
            assert np.array_equal(S.dev_state_to_snapshot(dev[i]), want[i])
        assert np.array_equal(dev[:, 13], envs["cyc_pos"]) and np.array_equal(dev[:, 14], envs["rng_ctr"].astype(np.int32))
    assert np.array_equal(b.sweep.dev, S.device_state(b.sweep.envs))
    assert not S.post_state_mismatch(S.device_state(b.post), b.post).any()
    wrong = S.device_state(b.post[:8])
    wrong[3, 14] += 1; wrong[5, 8] += 1
    assert S.post_state_mismatch(wrong, b.post[:8]).tolist() == [False, False, False, True, False, True, False, False]


def test_collision_lattice_reaches_the_states_where_the_masks_matter():
    a = S.stepped("A")
    term = (a.terminal != 0).reshape(S.A_SHAPE)
    overlap_alive = int((S.rect_overlap_a() & (a.terminal == 0)).sum())
    wing_cells = int((term.min(axis=-1) != term.max(axis=-1)).sum())
    scoring = int((a.reward == np.float32(3.0)).sum())              # a crash overrides the 3: these score and live
    by, bx = int((term[1:] != term[:-1]).sum()), int((term[:, 1:] != term[:, :-1]).sum())
    print(f"lattice A: {term.mean():.4f} crash, {overlap_alive} rect-overlap-without-crash, {wing_cells} wing-dependent cells, "
          f"{scoring} scoring, {by} / {bx} crash boundaries along y / x")
    assert overlap_alive >= 27000 and wing_cells >= 500 and scoring >= 7000 and by >= 4000 and bx >= 11000
    assert set(np.unique(a.reward).tolist()) == {float(np.float32(v)) for v in (-3.0, 0.1, 3.0)}
    # a crash resets onto the env's own Philox stream: both gaps drawn, from the counter the state carried
    dead = a.terminal != 0
    assert (a.post["rng_ctr"][dead] == a.sweep.envs["rng_ctr"][dead] + 2).all() and (a.post["rng_ctr"][~dead] == a.sweep.envs["rng_ctr"][~dead]).all()
    assert len(np.unique(a.post["pipe_gap"][dead, :2], axis=0)) == 64


def test_dynamics_lattice_reaches_every_rule():
    b = S.stepped("B")
    c, pre, post = b.sweep.coords, b.sweep.envs, b.post
    one = c["part"] == 0
    alive = b.terminal == 0
    assert (post["playery"][one & alive] == 0).sum() > 50                          # the ceiling clamp
    assert (one & (c["vely"] == 10) & alive & (post["vely"] == 10)).any()          # the velocity cap
    assert (one & (c["action"] == 1) & alive & (post["vely"] == -9)).any()         # a flap
    for y, v, dies in ((369, 10, False), (370, 10, True), (379, 0, False), (379, 1, True)):      # the ground: y + velY reaches 380
        m = one & (c["y"] == y) & (c["vely"] == v - 1) & (c["action"] == 0)
        assert m.sum() == 1 and bool(b.terminal[m][0]) == dies, (y, v)
    two = c["part"] == 1
    combos = np.unique(np.stack([pre["loop_iter"][two], pre["cyc_pos"][two], pre["basex"][two]], 1), axis=0)
    assert len(combos) == 30 * 4 * 12
    assert set(np.unique(post["player_index"][two & alive]).tolist()) == {0, 1, 2} and len(np.unique(post["basex"][two])) == 12
    three = (c["part"] == 2) & alive
    assert three.sum() == (c["part"] == 2).sum()                                   # the bird sits in the gap: bookkeeping is what differs
    x0, n_pre, n_post = c["x0"][three], c["n_pipes"][three], post["n_pipes"][three]
    assert ((n_post == 3) & (n_pre == 2)).sum() == 4 * 16 and set(x0[(n_post == 3) & (n_pre == 2)].tolist()) == {5, 6, 7, 8}     # spawn at post x 1..4
    assert set(x0[n_post < n_pre].tolist()) == set(range(-56, -48))                # removal below -52
    assert set(x0[b.reward[three] == np.float32(3.0)].tolist()) == {49, 50, 51, 52}                                              # score at post x 45..48
    assert set(post["pipe_x"][three & (b.sweep.envs["n_pipes"] == 3)][:, 2].tolist()) >= {290, 292} and (n_post >= 1).all() and (n_post <= 3).all()


def test_render_lattices_index_every_table_entry():
    """C-E together use every (gap, dx, phase) entry of the pre-rendered pipe rows and every (wing, y) of the bird table; E puts the
    bird and a pipe into every one of the bird's observation rows."""
    xo, yo = S.resize_taps()
    assert xo[:4].tolist() == [1, 4, 8, 12] and yo[:4].tolist() == [2, 9, 15, 21]             # (test_resize_taps_match_survey_probe)
    assert (yo[5:] == yo[:-5] + 32).all() and yo[62] + 1 < 404 <= yo[63]                       # columns 63.. see the ground only
    cover = np.zeros((8, 53, 5), bool)
    for n in "CDE":
        cover |= S.pipe_table_cover(S.stepped(n).post)
    assert cover.all(), np.argwhere(~cover)[:5]
    assert S.pipe_table_cover(S.stepped("C").post).all()                                       # ... C alone does, as it is meant to
    d = S.stepped("D")
    assert not d.terminal.any() and not S.slow_row_cover(d.post).any()                         # bird rows free of pipes: the table path
    seen = np.zeros((3, 380), bool)
    seen[d.post["player_index"], d.post["playery"].astype(int)] = True
    assert seen.all()
    e = S.stepped("E")
    alive = e.terminal == 0
    assert alive.sum() == 3000 and S.bird_rows().sum() == 9
    slow = S.slow_row_cover(np.ascontiguousarray(e.post[alive]))
    assert (slow[S.bird_rows()] >= 1000).all(), slow
    assert len(np.unique(e.post["basex"])) == 12 and len(np.unique(e.post["basex"][~alive])) == 1      # (a reset puts basex back to 0)
    total = sum(len(S.stepped(n).post) for n in "CDE")
    assert 7500 <= total <= 8500
