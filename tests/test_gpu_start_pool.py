"""Start pools on the GPU (sgx_set_start_pool, VecStrategoEnv.set_start_states / set_curriculum): every game start that would sample a
setup loads a pool record instead -- in reset() and in every kernel that restarts games, in the middle of multi-step launches too.

The oracle is stepped alongside (tests/test_start_pool_cpu.PoolFollower plays the rule on OracleEnv alone) and every slot of every launch
is compared: mask, observation, reward, done, player, ending_invalid, the drawn action and start_index.  Buffers are poisoned before
every call.  The number of restarts must equal the follower's and reach the floor of the case (tests/test_start_pool_cpu.CASES)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS
from tests.helpers import GOLDEN, general_states
from tests.step_checks import _host, _multi_kinds, _poison
from tests.pool_roots import START_POOL_CASES as CASES, G0, POOL_N, SEED, PoolFollower, make_pool

pytestmark = pytest.mark.gpu
CHUNK = 64


def _env(v, n, states, players, restart_clock, first_player='stored', **kw):
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv(v, n, seed=SEED, env_id_offset=G0, auto_reset=True, **kw)
    env.set_start_states(states, players, first_player=first_player, restart_clock=restart_clock)
    assert env.start_pool_size == len(states)
    return env


def _current(env, both=False, decode=False):
    h = {'mask': (env.decode_mask() if decode else env.mask).cpu().numpy(), 'obs': (env.decode_obs() if decode else env.obs).cpu().numpy(),
         'player': env.player.cpu().numpy(), 'start_index': env.start_index.cpu().numpy()}
    if both:
        h['fobs'] = env.fobs.cpu().numpy()
    return h


def _decode_slot(env, traj, s):
    """compact outputs: the contract tensors of slot s"""
    keep = (env.obs, env.mask)
    env.obs, env.mask = traj['obs'][s], traj['mask'][s]
    try:
        return env.decode_obs().cpu().numpy(), env.decode_mask().cpu().numpy()
    finally:
        env.obs, env.mask = keep


def _rollout_against_follower(name, n, steps, pool_steps, restart_clock, floor, kw=None, first_player='stored', multi=True, emit_obs=True, v=None,
                              pool=None):
    import torch
    kw = dict(kw or {})
    v = v or VARIANTS[name]
    both, original, compact = bool(kw.get('full_obs')), kw.get('obs_channel_mode') == 'original', bool(kw.get('compact_outputs'))
    states, players = pool if pool is not None else make_pool(v, pool_steps)
    fo = PoolFollower(v, n, states, players, restart_clock, random_first=first_player == 'random', both=both, original=original, with_obs=emit_obs)
    env = _env(v, n, states, players, restart_clock, first_player, **kw)
    if not multi:
        env.set_multi_step(False)
    env.reset()
    fo.check_current(_current(env, both, compact))
    env.sample_valid_actions()
    traj = env.alloc_trajectory(CHUNK)
    assert tuple(traj['start_index'].shape) == (CHUNK, n) and traj['start_index'].dtype == torch.int32
    done_seen = 0
    for at in range(0, steps, CHUNK):
        now = min(CHUNK, steps - at)
        acts = env.next_actions.cpu().numpy().copy()
        _poison(traj)
        env.rollout_trajectory(now, traj, emit_obs=emit_obs)
        if multi and not original:
            assert env.last_launch_kind in _multi_kinds(), (name, 'the test must not pass on the per-step kernel')
        elif not multi:
            assert env.last_launch_kind not in _multi_kinds()
        if not emit_obs:
            assert bool(torch.isnan(traj['obs']).all())
        h = _host(traj)
        for s in range(now):
            slot = {k: a[s] for k, a in h.items()}
            if compact:
                slot['obs'], slot['mask'] = _decode_slot(env, traj, s)
            if not emit_obs:
                slot.pop('obs')
            fo.step(acts, slot, tag=(name, 'call at', at, 'slot', s))
            acts = h['actions'][s]
        done_seen += int(h['done'][:now].sum())
        assert env.start_index.data_ptr() == traj['start_index'][now - 1].data_ptr()
    st, pl = env.export_state()
    assert np.array_equal(st.cpu().numpy(), np.stack([oe.state for oe in fo.oenvs])), (name, 'final states')
    assert np.array_equal(pl.cpu().numpy(), np.asarray([oe.player for oe in fo.oenvs], dtype=np.int8))
    assert done_seen == fo.restarts, (name, 'restarts', done_seen, fo.restarts)
    assert fo.restarts >= floor, (name, fo.restarts, floor)
    env.close()
    return fo


@pytest.mark.parametrize('name', list(CASES))
def test_every_slot_of_multi_step_launches_equals_the_oracle(name):
    n, steps, pool_steps, restart, floor = CASES[name]
    _rollout_against_follower(name, n, steps, pool_steps, restart, floor)


def test_one_launch_per_step():
    _rollout_against_follower('barrage', 48, 256, 41, True, 5, multi=False)


def test_one_launch_per_step_lane_kernel():
    _rollout_against_follower('micro', 130, 96, 7, True, 300, multi=False)


# (floors of the per-kind cases: the follower ends 59 games in 48 x 640 steps with this pool, 0.0019 per env-step -- 48 x 256 steps expect
#  23; the floor is a third of that, and the exact count is compared with the follower anyway)
def test_full_obs():
    _rollout_against_follower('barrage', 48, 256, 41, True, 8, kw={'full_obs': True})


def test_original_channels():
    _rollout_against_follower('barrage', 48, 256, 41, True, 8, kw={'obs_channel_mode': 'original'})


def test_compact_outputs():
    _rollout_against_follower('barrage', 48, 256, 41, True, 8, kw={'compact_outputs': True})


def test_no_observation_half_wave_kind():
    _rollout_against_follower('barrage', 45, 256, 41, True, 5, emit_obs=False)


def test_random_first_player():
    fo = _rollout_against_follower('barrage', 48, 256, 41, True, 5, first_player='random')
    assert fo.first_movers == {1, -1}


def test_random_first_player_lane_kernels():
    fo = _rollout_against_follower('micro', 130, 128, 7, True, 500, first_player='random')
    assert fo.first_movers == {1, -1}


def test_a_trajectory_without_per_slot_results():
    """alloc_trajectory(results=False) with a pool set: no per-slot start_index; the env's own start_index [N] follows the last step."""
    name, n = 'short_barrage', 64
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    fo = PoolFollower(v, n, states, players, True)
    env = _env(v, n, states, players, True)
    env.reset()
    fo.check_current(_current(env))
    env.sample_valid_actions()
    traj = env.alloc_trajectory(32, results=False)
    assert 'start_index' not in traj and 'reward' not in traj
    own = env.start_index
    for call in range(8):
        _poison(traj)
        own.fill_(-12345)
        env.rollout_trajectory(32, traj)
        assert env.last_launch_kind in _multi_kinds() and env.start_index is own
        h = _host(traj)
        for s in range(32):
            slot = {'obs': h['obs'][s], 'mask': h['mask'][s], 'actions': h['actions'][s]}
            if s == 31:
                slot.update(start_index=own.cpu().numpy(), player=env.player.cpu().numpy(), done=env.done.cpu().numpy())
            fo.step(None, slot, tag=('no results', call, s))
    assert fo.restarts >= 40, fo.restarts          # (203 endings in 64 x 320 steps with this pool: 256 steps expect 160)
    env.close()


def test_a_ring_of_three_sets():
    """rollout_steps(3, ring=True): one multi-step launch writes the three sets in turn; the per-step results are the last step's."""
    name, n = 'barrage', 48
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    fo = PoolFollower(v, n, states, players, True)
    env = _env(v, n, states, players, True)
    env.reset()
    fo.check_current(_current(env))
    env.alloc_output_ring(3, tune=False)
    env.sample_valid_actions()
    for call in range(86):
        first = env._ring_pos
        for k in range(3):
            env._ring[k][0].fill_(float('nan'))
            env._ring[k][1].fill_(0x5A)
        env.start_index.fill_(-12345)
        env.rollout_steps(3, ring=True)
        assert env.last_launch_kind in _multi_kinds()
        for i in range(3):
            obs, mask, _ = env._ring[(first + i) % 3]
            slot = {'obs': obs.cpu().numpy(), 'mask': mask.cpu().numpy()}
            if i == 2:
                slot.update(done=env.done.cpu().numpy(), reward=env.reward.cpu().numpy(), player=env.player.cpu().numpy(),
                            ending_invalid=env.ending_invalid.cpu().numpy(), start_index=env.start_index.cpu().numpy(),
                            actions=env.next_actions.cpu().numpy())
            fo.step(None, slot, tag=('ring', call, i))
    assert fo.restarts >= 5
    env.close()


def test_step_sync_with_four_envs():
    """sgx_step_sync on 4 games: single_kernel_pool (one workgroup per game)."""
    import torch
    name, n = 'short_barrage', 4
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    fo = PoolFollower(v, n, states, players, True)
    env = _env(v, n, states, players, True)
    env.reset()
    fo.check_current(_current(env))
    for t in range(400):
        acts = np.asarray([fo.drawn(e) for e in range(n)], dtype=np.int32)
        env.obs.fill_(float('nan')); env.mask.fill_(0x5A); env.start_index.fill_(-12345)
        env.step_sync(torch.from_numpy(acts))
        fo.step(acts, {'obs': env.obs.cpu().numpy(), 'mask': env.mask.cpu().numpy(), 'done': env.done.cpu().numpy(), 'reward': env.reward.cpu().numpy(),
                       'player': env.player.cpu().numpy(), 'ending_invalid': env.ending_invalid.cpu().numpy(),
                       'invalid_action': env.invalid_action.cpu().numpy(), 'start_index': env.start_index.cpu().numpy()}, tag=('sync', t))
    assert fo.restarts >= 3, fo.restarts
    env.close()


def test_a_board_of_more_than_256_cells():
    """17 x 16 = 272 cells (10-bit cell indices, records staged in a loop), 4 envs; the pool keeps its clock and sits a few moves before
    max_turns, so games end and restart all the time."""
    from tests.boards import CUSTOM
    v = CUSTOM['c17x16']
    pool = make_pool(v, v.max_turns - 6, n=12)
    _rollout_against_follower('c17x16', 4, 96, None, False, 20, v=v, pool=pool)


# ---- reset() ----------------------------------------------------------------------------------------------------------------------
def test_reset_draws_from_the_pool_and_env_select_touches_only_the_selected():
    import torch
    name, n = 'barrage', 96
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    fo = PoolFollower(v, n, states, players, False)
    env = _env(v, n, states, players, False)
    env.reset()
    fo.check_current(_current(env))
    assert len(set(env.start_index.cpu().numpy().tolist())) > 8
    sel = np.zeros(n, dtype=np.uint8)
    sel[[0, 3, 17, 64, 95]] = 1
    before = env.export_state()[0].cpu().numpy()
    for e in np.flatnonzero(sel):
        fo.start(int(e))
    env.reset(env_select=torch.from_numpy(sel))
    fo.check_current(_current(env), 'env_select')
    after = env.export_state()[0].cpu().numpy()
    assert np.array_equal(after[sel == 0], before[sel == 0])
    assert np.array_equal(after, np.stack([oe.state for oe in fo.oenvs]))
    env.close()


def test_explicit_maps_override_the_pool():
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, n = 'barrage', 16
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    env = _env(v, n, states, players, False)
    env.reset()
    cv = orc.make_cvariant(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, v.initial_state_usable_rows)
    maps = [orc.sample_setup(cv, 5, e, 0) for e in range(n)]
    m1 = np.stack([m[0] for m in maps]).astype(np.int8)
    m2 = np.stack([m[1] for m in maps]).astype(np.int8)
    env.reset(m1, m2)
    twin = VecStrategoEnv(name, n, seed=SEED, env_id_offset=G0, auto_reset=True)
    twin.reset(m1, m2)
    assert env.obs.cpu().numpy().tobytes() == twin.obs.cpu().numpy().tobytes() and bool((env.mask == twin.mask).all())
    assert np.array_equal(env.export_state()[0].cpu().numpy(), twin.export_state()[0].cpu().numpy())
    assert bool((env.start_index == -1).all())
    env.close(); twin.close()


def test_the_curriculum_fixture_batched():
    import os
    from stratego_env_amd.vec_env import VecStrategoEnv
    path = os.path.join(GOLDEN, 'curriculum_barrage.npz')
    with np.load(path) as z:
        table, winners = z['state'].astype(np.int64), z['winner'].reshape(-1)
    assert len(table) == 8
    n = 256
    env = VecStrategoEnv('barrage', n, seed=SEED, env_id_offset=G0, auto_reset=True)
    env.set_curriculum(path)
    assert env.start_pool_size == 8
    env.reset()
    idx = env.start_index.cpu().numpy()
    assert idx.min() >= 0 and idx.max() < 8 and len(set(idx.tolist())) == 8
    st, pl = env.export_state()
    st, pl = st.cpu().numpy(), pl.cpu().numpy()
    for e in range(n):
        want = table[idx[e]].copy()
        want[5, 0, 0], want[5, 1, 0] = 0, 1000
        assert np.array_equal(st[e], want), (e, idx[e])
        p = -1 if orc.rng_below(orc.rng(SEED, G0 + e, 0, 4, 1), 2) == 1 else 1
        assert pl[e] == p
    assert set(pl.tolist()) == {1, -1}
    assert np.array_equal(env.start_winner.cpu().numpy(), winners[idx].astype(np.int8))
    # ... and the positions play: a multi-step rollout with restarts from the table
    env.sample_valid_actions()
    env.rollout_steps(64)
    assert env.last_launch_kind in _multi_kinds() and int(env.invalid_action.sum()) == 0
    idx2 = env.start_index.cpu().numpy()
    assert idx2.min() >= 0 and idx2.max() < 8
    assert np.array_equal(env.start_winner.cpu().numpy(), winners[idx2].astype(np.int8))
    env.close()


def test_clearing_the_pool_restores_sampled_setups_byte_for_byte():
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, n = 'barrage', 64
    v = VARIANTS[name]
    states, players = make_pool(v, 41)
    a = _env(v, n, states, players, True)
    a.clear_start_states()
    assert a.start_pool_size == 0 and a.start_index is None
    b = VecStrategoEnv(name, n, seed=SEED, env_id_offset=G0, auto_reset=True)
    trajs = []
    for env in (a, b):
        env.reset()
        env.sample_valid_actions()
        traj = env.alloc_trajectory(64)
        assert 'start_index' not in traj
        _poison(traj)
        env.rollout_trajectory(64, traj)
        trajs.append(traj)
    for k in trajs[1]:
        assert trajs[0][k].cpu().numpy().tobytes() == trajs[1][k].cpu().numpy().tobytes(), k
    assert np.array_equal(a.export_state()[0].cpu().numpy(), b.export_state()[0].cpu().numpy())
    a.close(); b.close()


# ---- refusals: ValueError / SGX_EINVAL before anything is launched -------------------------------------------------------------------
def test_refusals():
    from stratego_env_amd import _lib
    from stratego_env_amd.vec_env import VecStrategoEnv
    name = 'tiny'
    v = VARIANTS[name]
    states, players = make_pool(v, 9)
    env = VecStrategoEnv(name, 32, seed=SEED, env_id_offset=G0, auto_reset=True)
    # a finished game
    bad = states.copy()
    bad[5][5, 0, 1] = 1
    bad[5][5, 0, 2] = 1
    with pytest.raises(ValueError, match=r'over'):
        env.set_start_states(bad, players)
    assert env.start_pool_size == 0
    import torch
    pool_bad = VecStrategoEnv(name, len(bad), outputs=False, human_inits=False)            # ... and straight at the C ABI: the message names the record
    pool_bad.import_state_checked(bad, players, torch.zeros(len(bad), dtype=torch.uint8, device=env.device))
    rc = env._L.sgx_set_start_pool(env._h, pool_bad._h, len(bad), 0)
    assert rc == -1 and b'record 5 ' in env._L.sgx_last_error(), env._L.sgx_last_error()
    pool_bad.close()
    # a state the packed record cannot carry
    gs, gp = general_states(name, 6, np.random.RandomState(3))
    gs[:, 5, 0, 1] = 0
    with pytest.raises(ValueError, match=r'sanitised'):
        env.set_start_states(gs, gp)
    # a pool of another board
    other = VecStrategoEnv('micro', 8, outputs=False, human_inits=False)
    other.reset()
    with pytest.raises(ValueError):
        env.set_start_states(other)
    # n_pool = 0 / more than the pool holds, straight at the C ABI
    pool = VecStrategoEnv(name, 8, outputs=False, human_inits=False)
    pool.reset()
    for n_pool in (0, 9, -1):
        rc = env._L.sgx_set_start_pool(env._h, pool._h, n_pool, 0)
        assert rc == -1 and b'n_pool' in env._L.sgx_last_error(), (n_pool, rc)
    assert env._L.sgx_set_start_pool(env._h, pool._h, 8, 64) == -1
    assert env.start_pool_size == 0
    # ... and the env still plays sampled setups
    env.reset()
    env.sample_valid_actions()
    env.rollout_steps(8)
    assert int(env.invalid_action.sum()) == 0
    # the pool is a COPY: closing the source leaves it usable
    env.set_start_states(pool)
    pool.close(); other.close()
    env.reset()
    env.sample_valid_actions()
    env.rollout_steps(40)
    assert int(env.invalid_action.sum()) == 0 and int(env.start_index.min()) >= 0 and int(env.start_index.max()) < 8
    env.close()


# ---- guard bands ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,n', [('barrage', 45), ('micro', 130), ('fives', 33)])
def test_start_index_is_written_inside_its_extent_only(name, n):
    import torch
    from tests.guard_bands import Arena
    from stratego_env_amd import _lib
    v = VARIANTS[name]
    states, players = make_pool(v, CASES[name][2])
    env = _env(v, n, states, players, True)
    dev = env.device
    si = Arena('start_index', (n,), torch.int32, 4, dev)
    env.start_index = si.t
    _lib.check(env._L.sgx_set_start_index_out(env._h, C.c_void_p(si.t.data_ptr())), env._L)

    def settle(what):
        torch.cuda.synchronize(dev)
        si.check_guards(what)
        si.check_written(what)
        assert int(si.t.min()) >= 0 and int(si.t.max()) < POOL_N
        si.poison()
    env.reset()
    settle('reset')
    sel = torch.zeros(n, dtype=torch.uint8)
    rows = [1, n // 2, n - 1]
    sel[rows] = 1
    env.reset(env_select=sel)
    torch.cuda.synchronize(dev)
    si.check_guards('env_select')
    si.check_written('env_select', rows=rows)
    env.reset()
    settle('reset again')
    env.sample_valid_actions()
    env.rollout_step()
    settle('step')
    env.rollout_steps(40)
    settle('rollout_steps')
    env.set_multi_step(False)
    env.rollout_steps(3)
    settle('per-step rollout')
    env.set_multi_step(True)
    # the trajectory's start_index: [T, N] between guards
    T = 24
    traj = env.alloc_trajectory(T)
    ts = Arena('traj start_index', (T, n), torch.int32, 8, dev)
    traj['start_index'] = ts.t
    for steps, first in ((T, 0), (7, 20), (1, 3)):
        ts.poison()
        env.rollout_trajectory(steps, traj, first_slot=first)
        torch.cuda.synchronize(dev)
        ts.check_guards(('traj', steps, first))
        si.check_guards(('traj', steps, first))
        si.check_untouched(('traj', steps, first))
        slots = [(first + i) % T for i in range(steps)]
        ts.check_written(('traj', steps, first), rows=slots)
        assert int(ts.t[slots].min()) >= 0 and int(ts.t[slots].max()) < POOL_N
    env.close()
