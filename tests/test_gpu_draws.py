"""The distribution of every random draw the device makes.

The parity tests prove that the device draws what the oracle draws; the oracle restates the same counter RNG, so an error in the design of
a draw passes them.  Here the draws are read back from the device -- setup rows and placements from export_state(), pool rows and first
movers from start_index / player, actions from the logged actions and their masks, playout results -- and held against what the reference
means by them: np.random.choice over the setup table, random.shuffle of the setup cells, np.random.randint over the pool, a uniformly
random valid action; and against independence across players, games, turns, envs, seeds, env_id_offsets and streams.

Every chi-squared is held below the 0.999 quantile for its degrees of freedom and printed with it (pytest -s).  The RNG is a counter RNG:
every figure is a fixed number.  The keys -- seeds 0, 1, 7, 0xC0FFEE, env_id_offset 0, 1 << 20, 1 << 40 -- were fixed before the first
run; a statistic above its quantile is not answered by another key (tests/draw_stats.py).  The same statistics run
on the oracle's functions and reject eight deliberately broken samplers in tests/test_draws_cpu.py."""
import numpy as np
import pytest

from tests import draw_stats as ds

pytestmark = pytest.mark.gpu

N = ds.N_KEYS
KEYS = [(s, o) for s in ds.SEEDS for o in ds.OFFSETS]


def _env(name, n, seed, offset, **kw):
    from stratego_env_amd.vec_env import VecStrategoEnv
    kw.setdefault('placement', 'plain')
    return VecStrategoEnv(name, n, seed=seed, env_id_offset=offset, **kw)


def _own_side_maps(env):
    """-> both players' own-side setup cells, uint8 [N, U, C] each (player -1's board rotated back by 180 degrees)."""
    import torch
    st, _ = env.export_state()
    U = env.variant.initial_state_usable_rows
    p1 = st[:, 0, :U, :].to(torch.uint8).cpu().numpy()
    p2 = torch.flip(st[:, 1], dims=(1, 2))[:, :U, :].to(torch.uint8).cpu().numpy()
    del st
    return p1, p2


# ---- a. the setup table -------------------------------------------------------------------------------------------------------------------
_TABLE = {}
_ROWS = {}


def _table():
    if not _TABLE:
        from stratego_env_amd import setups as S
        table = S.load_setup_table('barrage')
        canonical, lookup = ds.table_rows(table)
        _TABLE.update(table=table, canonical=canonical, lookup=lookup)
    return _TABLE['table'], _TABLE['canonical'], _TABLE['lookup']


def _setup_rows(seed, offset, games=1):
    """The (canonical) table rows of both players in the first `games` games of 65,536 Barrage envs; computed once per key."""
    key = (seed, offset)
    if key not in _ROWS or len(_ROWS[key]) < games:
        _, _, lookup = _table()
        env = _env('barrage', N, seed, offset, human_inits=True, auto_reset=False)
        out, numbers = [], []
        for j in range(games):
            env.reset()
            numbers.append(env.env_info()[:, 1].cpu().numpy())
            out.append(ds.setup_rows_from_maps(*_own_side_maps(env), lookup))
        for j in range(1, games):
            assert np.array_equal(numbers[j], numbers[0] + j), "every reset() starts the env's next game"
        env.close()
        _ROWS[key] = out
    return _ROWS[key]


@pytest.mark.parametrize('seed,offset', KEYS)
def test_setup_table_rows_are_uniform_and_the_players_independent(seed, offset):
    """np.random.choice twice (util.py:313-314): a table row that occurs m times has probability m / S; the index binned into 16 equal
    ranges; the margins of both players, their 16 x 16 joint, and env g against env g + 1."""
    _, canonical, _ = _table()
    (i1, i2), = _setup_rows(seed, offset)[:1]
    tag = 'setup table, seed %#x offset %#x: ' % (seed, offset)
    ds.check(tag + 'margin +1', ds.setup_margin_stat(i1, canonical))
    ds.check(tag + 'margin -1', ds.setup_margin_stat(i2, canonical))
    ds.check(tag + 'player +1 x player -1', ds.setup_joint_stat(i1, i2, len(canonical)))
    ds.check(tag + 'env g x env g + 1', ds.setup_joint_stat(i1[0::2], i1[1::2], len(canonical)))


@pytest.mark.parametrize('a,b', [((0, 0), (1, 0)), ((0, 0), (0, 1 << 20)), ((0, 0), (0, 1 << 40)), ((1, 1 << 20), (1, 0)),
                                 ((0, 0), (1 << 32, 0)), ((7, 1 << 40), (7 + (1 << 32), 1 << 40))],
                         ids=['seed0-seed1', 'offset0-offset2^20', 'offset0-offset2^40', 'seed1-offset2^20-offset0', 'seed0-seed2^32', 'seed7-seed7+2^32'])
def test_setup_rows_of_another_seed_or_offset_are_other_draws(a, b):
    """Another seed, the same seed with another env_id_offset, and the seeds s and s + (1 << 32): fewer than 1 % of the envs get the same
    pair of rows, and the 16 x 16 joint of the two runs is independent."""
    _, canonical, _ = _table()
    (a1, a2), = _setup_rows(*a)[:1]
    (b1, b2), = _setup_rows(*b)[:1]
    same = float(((a1 == b1) & (a2 == b2)).mean())
    print('seed %#x offset %#x against seed %#x offset %#x: %.4f %% of the envs draw the same pair' % (a + b + (100 * same,)))
    assert same < 0.01
    ds.check('setup rows of the two runs, player +1', ds.setup_joint_stat(a1, b1, len(canonical)))
    ds.check('setup rows of the two runs, player -1', ds.setup_joint_stat(a2, b2, len(canonical)))


def test_setup_rows_of_consecutive_games_are_independent():
    _, canonical, _ = _table()
    (i1, i2), (j1, j2) = _setup_rows(0xC0FFEE, 1 << 20, games=2)
    assert float(((i1 == j1) & (i2 == j2)).mean()) < 0.01
    ds.check('setup table, game j x game j + 1, player +1', ds.setup_joint_stat(i1, j1, len(canonical)))
    ds.check('setup table, game j x game j + 1, player -1', ds.setup_joint_stat(i2, j2, len(canonical)))


# ---- b. random placements -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,seed,offset', [('micro', 0, 0), ('tiny', 1, 1 << 20), ('fives', 7, 1 << 40), ('barrage', 0xC0FFEE, 0)])
def test_random_placements_are_uniform_shuffles(name, seed, offset):
    """random.shuffle of the setup cells, pieces filled in piece-code order (util.py:13-30): every cell holds every piece type with
    probability piece_counts / n, the two players' flags are independent, consecutive games are, and on the boards whose arrangements can
    be enumerated (24, 24, 120) every one appears with equal frequency."""
    env = _env(name, N, seed, offset, human_inits=False, auto_reset=False)
    v = env.variant
    n = v.initial_state_usable_rows * v.columns
    env.reset()
    m1, m2 = (m.reshape(N, n) for m in _own_side_maps(env))
    for pl, m in ((1, m1), (-1, m2)):
        assert np.array_equal(np.sort(m, axis=1), np.broadcast_to(np.sort(np.concatenate([np.zeros(n - v.pieces_per_side, dtype=np.uint8),
                              np.repeat(np.arange(1, 13, dtype=np.uint8), v.piece_counts)])), (N, n))), "every placement holds the variant's pieces"
    for k, st in ds.placement_stats(v.piece_counts, m1, m2, name + ': ').items():
        ds.check(k, st)
    if ds.n_arrangements(v.piece_counts, n) <= 120:
        for pl, m in ((1, m1), (-1, m2)):
            seen, worlds, st = ds.arrangement_stat(v.piece_counts, m)
            print('%s player %+d: %d of %d arrangements' % (name, pl, seen, worlds))
            assert seen == worlds
            ds.check('%s: arrangements of player %+d' % (name, pl), st)
    env.reset()
    k1, k2 = (m.reshape(N, n) for m in _own_side_maps(env))
    assert float(((k1 == m1).all(1) & (k2 == m2).all(1)).mean()) < (0.01 if n > 4 else 0.02)       # (4 cells: 1 / 576 of the pairs repeat by chance)
    flag = lambda m: np.argmax(m == 11, axis=1)
    ds.check(name + ': flag +1 of game j x game j + 1', ds.chi2_independence(ds.two_way(flag(m1), flag(k1), n, n)))
    ds.check(name + ': flag -1 of game j x game j + 1', ds.chi2_independence(ds.two_way(flag(m2), flag(k2), n, n)))
    env.close()


# ---- c. start pools -----------------------------------------------------------------------------------------------------------------------
def test_start_pool_rows_and_first_movers():
    """np.random.randint over the pool and a fair coin for the first mover (maenv:519-527), per game: 16 distinguishable records on Micro,
    first_player='random', auto-reset; the rows and first movers of the first four games of every env."""
    from stratego_env_amd.config import VARIANTS
    from tests.pool_roots import make_pool
    n_pool, games, chunk = 16, 4, 32
    states, players = make_pool(VARIANTS['micro'], 2, n=n_pool)
    assert len({s.tobytes() for s in states}) == n_pool
    env = _env('micro', N, 1, 1 << 40, auto_reset=True, human_inits=False)
    env.set_start_states(states, players, first_player='random', restart_clock=True)
    env.reset()
    rows, first = [env.start_index.cpu().numpy().copy()], [env.player.cpu().numpy().copy()]
    env.sample_valid_actions()
    traj = env.alloc_trajectory(chunk)
    done, row_at, first_at = [], [], []
    for _ in range(3):                                             # (a Micro game lasts at most 20 moves: three restarts within 61 steps)
        env.rollout_trajectory(chunk, traj, emit_obs=False)
        done.append(traj['done'].cpu().numpy() != 0)
        row_at.append(traj['start_index'].cpu().numpy())
        first_at.append(traj['player'].cpu().numpy())
    env.close()
    done, row_at, first_at = (np.concatenate(x) for x in (done, row_at, first_at))                 # [steps, N]
    nth = np.cumsum(done, axis=0)
    assert (nth[-1] >= games - 1).all()
    cols = np.arange(N)
    for j in range(1, games):
        at = np.argmax(nth >= j, axis=0)                           # the step of the env's j-th restart: its slot holds the new game
        assert done[at, cols].all()
        rows.append(row_at[at, cols]); first.append(first_at[at, cols])
    rows, first = np.stack(rows, axis=1), np.stack(first, axis=1)
    assert ((rows >= 0) & (rows < n_pool)).all() and np.isin(first, (1, -1)).all()
    for k, st in ds.pool_stats(rows, first, n_pool, 'start pool: ').items():
        ds.check(k, st)


# ---- d. action draws ------------------------------------------------------------------------------------------------------------------------
def _trajectory_pit(env, slots, rs):
    """`slots` rollout steps into a trajectory buffer -> (u float [N, slots]: the PIT of every logged action in its mask, NaN for a mover without
    a move; same_game bool [N, slots - 1])."""
    import torch
    n = env.num_envs
    env.reset()
    env.sample_valid_actions()
    traj = env.alloc_trajectory(slots)
    env.rollout_trajectory(slots, traj)
    kind = env.last_launch_kind
    u = np.full((n, slots), np.nan)
    for t in range(slots):
        m = traj['mask'][t].reshape(n, -1) != 0
        a = traj['actions'][t].long()
        total = m.sum(1)
        inside = (a >= 0) & (a < m.shape[1])
        safe = torch.where(inside, a, torch.zeros_like(a))
        k = torch.cumsum(m, dim=1).gather(1, safe[:, None])[:, 0] - 1
        valid = inside & m.gather(1, safe[:, None])[:, 0]
        has = total > 0
        assert bool(valid[has].all()), "every drawn action is valid"
        has, k, total = has.cpu().numpy(), k.cpu().numpy(), total.cpu().numpy()
        u[has, t] = ds.pit(k[has], total[has], rs)
    assert int(traj['invalid_action'].sum()) == 0
    same_game = (traj['done'][1:].cpu().numpy() == 0).T
    print('%d of %d steps have a mover with a move, %d of %d step pairs stay in one game' % ((~np.isnan(u)).sum(), u.size, same_game.sum(), same_game.size))
    return u, same_game, kind


@pytest.mark.parametrize('name,n,seed,offset,multi', [('barrage', 4096, 7, 1 << 20, True), ('micro', N, 0xC0FFEE, 1 << 40, True),
                                                      ('barrage', 4096, 0, 0, False), ('micro', N, 1, 1 << 20, False)],
                         ids=['barrage-multi-step', 'micro-lane-multi-step', 'barrage-per-step', 'micro-per-step'])
def test_logged_actions_are_uniform_over_the_valid_ones(name, n, seed, offset, multi):
    """A uniformly random valid action (maenv:830-834) at every step of a 32-slot trajectory: from mask[t] and actions[t] the rank k of the
    action among the `total` valid ones; every action is valid; the randomised PIT u = (k + U) / total is uniform (16 bins); turn t and
    t + 1 of one game are independent (4 x 4), env g and g + 1 at one step are.  Barrage plays the wave-per-game multi-step kernel, Micro
    the lane multi-step kernel, and with sgx_set_multi_step off the per-step kernels draw."""
    from stratego_env_amd import _lib
    env = _env(name, n, seed, offset, auto_reset=True)
    if not multi:
        env.set_multi_step(False)
    u, same_game, kind = _trajectory_pit(env, 32, np.random.RandomState(11))
    want = {('barrage', True): (_lib.LAUNCH_MULTI_STEP_WAVE,), ('micro', True): (_lib.LAUNCH_MULTI_STEP,),
            ('barrage', False): (_lib.LAUNCH_WAVE,), ('micro', False): (_lib.LAUNCH_WAVE, _lib.LAUNCH_LANE)}[(name, multi)]
    assert kind in want, (name, multi, kind)
    env.close()
    tag = '%s, %s: ' % (name, {0: 'wave per step', 1: 'lane per step', 2: 'lane multi-step', 3: 'wave multi-step'}[kind])
    for k, st in ds.action_stats(u, tag, same_game).items():
        ds.check(k, st)


# ---- e. the stand-alone sampler -------------------------------------------------------------------------------------------------------------
def test_standalone_sampler_is_uniform_over_the_valid_actions():
    """sgx_sample_valid on 65,536 Barrage games in one position (the fixed maps of tests/test_gpu_choose_actions.py's softmax test): the
    equal-logits test ties the chooser to this sampler; this ties the sampler to uniform."""
    import torch
    env = _env('barrage', N, 7, 0, auto_reset=False, human_inits=False)
    m1 = np.zeros((10, 10), dtype=np.int8)
    m1[3, 0], m1[3, 4], m1[3, 5], m1[2, 2], m1[0, 0], m1[1, 1], m1[3, 9], m1[2, 8] = 2, 2, 3, 9, 11, 12, 1, 10
    maps = torch.from_numpy(np.broadcast_to(m1, (N, 10, 10)).copy())
    env.reset(maps, maps)
    mask0 = env.mask[0].reshape(-1).cpu().numpy()
    valid = np.flatnonzero(mask0)
    assert len(valid) >= 10 and bool((env.mask.reshape(N, -1) == env.mask[0].reshape(1, -1)).all())
    got = env.sample_valid_actions().cpu().numpy()
    env.close()
    assert np.isin(got, valid).all()
    rank = np.searchsorted(valid, got)
    ds.check('sgx_sample_valid over %d valid actions' % len(valid), ds.chi2_uniform(rank, len(valid)))
    ds.check('sgx_sample_valid, env g x env g + 1', ds.chi2_independence(ds.two_way(rank[0::2], rank[1::2], len(valid), len(valid))))


def test_standalone_sampler_takes_one_variate_per_key():
    """The draws of one key at two totals: sgx_sample_valid on the same 65,536 Micro games with 12 and with 16 valid actions (the first
    actions of the mask, so that the action is its rank).  The rule takes k = floor(v total) from the high half of one draw: the pair is
    the two quantisations of one uniform variate, 24 possible cells of 192 (ds.quantisation_joint_stat).  A sampler that is uniform at
    every total but takes the draw another way -- the low half through a modulo -- has the same margins and another joint
    (tests/test_draws_cpu.py::test_teeth_low_half_modulo_12)."""
    import torch
    env = _env('micro', N, 7, 1 << 20, auto_reset=False, human_inits=False)
    env.reset()
    A = env.R * env.Cc * env.K
    ks = []
    for total in (12, 16):
        mask = torch.from_numpy(ds.first_valid_mask(N, A, total)).to(env.device)
        out = torch.full((N,), -7, dtype=torch.int32, device=env.device)
        ks.append(env.sample_valid_actions(mask=mask, out=out).cpu().numpy())
        assert ((ks[-1] >= 0) & (ks[-1] < total)).all()
        ds.check('sgx_sample_valid, %d valid actions' % total, ds.chi2_uniform(ks[-1], total))
    env.close()
    ds.check('sgx_sample_valid of one key at 12 and 16 valid actions', ds.quantisation_joint_stat(ks[0], 12, ks[1], 16))


# ---- f. playouts ----------------------------------------------------------------------------------------------------------------------------
def test_playouts_of_two_draws_and_the_rollout_are_independent():
    """sgx_playout from 65,536 copies of one Micro root under draws 0 and 1, and rollout_steps from the same root with the same seed and
    env ids: the 3 x 3 tables of results (win / loss / draw for player +1) are independent -- another draw is another game, and the playout
    stream is not the action stream (draw 0 stands where the rollout's game number 0 stands)."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    seed, offset = 7, 1 << 20
    root = _env('micro', 1, 5, 0, auto_reset=False, human_inits=False)
    root.reset()
    st, pl = root.export_state()
    index = torch.zeros(N, dtype=torch.int32, device=root.device)
    pool = PackedStates('micro', N, seed=seed, env_id_offset=offset)
    results = []
    for draw in (0, 1):
        res = pool.playout(root, src_index=index, draw=draw)
        assert pool.last_launch_kind == _lib.LAUNCH_PLAYOUT
        assert bool(res.done.all())
        results.append(res.reward[:, 0].cpu().numpy())
    pool.close()
    env = _env('micro', N, seed, offset, auto_reset=False, human_inits=False)
    env.reset()
    env.import_state(st.expand(N, -1, -1, -1).contiguous(), pl.expand(N).contiguous())
    info = env.env_info().cpu().numpy()
    assert (info[:, 1] == 0).all() and (info[:, 0] == 0).all(), "game number 0, turn 0: the key of the playouts' draw 0"
    env.rollout_steps(env.variant.max_turns + 1, emit_obs=False, emit_mask=False)      # (no auto-reset: a finished game stays finished)
    assert bool((env.env_info()[:, 2] != 0).all()), "every rollout game is over"
    final, _ = env.export_state()
    results.append(final[:, 5, 0, 2].cpu().numpy().astype(np.float32))               # the winner; 0 for a tie and for a max-turn ending
    env.close(); root.close()
    cat = [np.where(r > 0, 0, np.where(r < 0, 1, 2)) for r in results]
    for r in cat:
        print('win / loss / draw for player +1:', np.bincount(r, minlength=3).tolist())
    same = float((cat[0] == cat[1]).mean())
    ds.check('playout draw 0 x draw 1', ds.chi2_independence(ds.two_way(cat[0], cat[1], 3, 3)))
    ds.check('playout draw 0 x rollout', ds.chi2_independence(ds.two_way(cat[0], cat[2], 3, 3)))
    ds.check('playout draw 1 x rollout', ds.chi2_independence(ds.two_way(cat[1], cat[2], 3, 3)))
    assert same < 0.99
