"""Start pools (sgx_set_start_pool): the C ABI's new symbols, and -- oracle only, no GPU -- the rule every game start follows while a
pool is set, played by a follower that the GPU tests (tests/test_gpu_start_pool.py) compare every slot of a multi-step launch with.

The rule (include/stratego_mi355x.h): game `game_no` of env `e` starts from pool record j = rng_below(rng(seed, env_id_offset + e, game_no,
stream 4, 0), n_pool) -- whole: boards, never-moved flags, clock, recent moves, captures -- with the record's mover, or, with a random
first player, -1 when rng_below(rng(..., stream 4, 1), 2) == 1 else +1; restart_clock puts turn = 0 and max_turns = the variant's.

The adequacy test makes sure the inputs of the GPU tests end enough games for those tests to mean something: a floor per case, taken
from the counts measured on the oracle with exactly these inputs (table in CASES)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import setups as S
from stratego_env_amd.config import VARIANTS

MASK, POBS, FOBS = 'valid_actions_mask', 'partial_observation', 'full_observation'
STREAM_POOL = 4
SEED, G0 = 0xC0FFEE, 4100
POOL_SEED, POOL_G0, POOL_N = 0x51A7, 900, 24

#        board            envs steps pool_steps restart_clock  floor    (endings measured on the oracle: 2,711 / 1,230 / 123 / 203 / 59 / 16)
CASES = {'micro': (130, 160, 7, True, 1000),
         'tiny': (100, 256, 9, True, 500),
         'fives': (33, 180, 15, True, 60),
         'short_barrage': (64, 320, 41, True, 100),
         'barrage': (48, 640, 41, True, 30),
         'short_standard': (16, 384, 150, False, 8)}


def cvariant_of(v):
    table = S.load_setup_table(v.human_inits) if getattr(v, 'human_inits', None) else None
    return orc.make_cvariant(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, v.initial_state_usable_rows, setups=table)


def make_pool(v, pool_steps, n=POOL_N, seed=POOL_SEED, g0=POOL_G0):
    """The final positions of `n` oracle rollouts of `pool_steps` steps, and their movers."""
    r = orc.rollout_ex(cvariant_of(v), seed, g0, n, pool_steps, want_states=True)
    return r['states'], r['info'][:, 3].astype(np.int8)


class PoolFollower:
    """The start-pool rule on OracleEnv alone.  step() plays one step of every game (auto-reset from the pool) and, given the host copy of
    a slot of GPU outputs, compares whatever tensors it holds."""

    def __init__(self, v, n, states, players, restart_clock, random_first=False, both=False, original=False, seed=SEED, g0=G0, with_obs=True):
        self.v, self.n, self.seed, self.g0 = v, n, seed, g0
        self.states, self.players = np.asarray(states), np.asarray(players)
        self.restart_clock, self.random_first, self.both, self.with_obs = restart_clock, random_first, both, with_obs
        mode = 'both_observations' if both else 'partially_observable'
        self.oenvs = [orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, observation_mode=mode,
                                    obs_channel_mode='original' if original else 'extended') for _ in range(n)]
        self.start_index = np.full(n, -1, dtype=np.int32)
        self.restarts, self.steps, self.touched = 0, 0, set()
        self.first_movers = set()
        self.cur = [None] * n
        for e, oe in enumerate(self.oenvs):
            oe.game_no = -1                # (a fresh handle's counter: the first game a reset starts is number 0)
            self.start(e)

    def start(self, e):
        """the env's next game: from the pool"""
        oe = self.oenvs[e]
        oe.game_no += 1
        g = self.g0 + e
        j = orc.rng_below(orc.rng(self.seed, g, oe.game_no, STREAM_POOL, 0), len(self.states))
        st = self.states[j].copy()
        if self.restart_clock:
            st[5, 0, 0], st[5, 1, 0] = 0, self.v.max_turns
        p = int(self.players[j])
        if self.random_first:
            p = -1 if orc.rng_below(orc.rng(self.seed, g, oe.game_no, STREAM_POOL, 1), 2) == 1 else 1
        o = oe.reset(initial_state_override=st, first_player_override=p)
        self.start_index[e] = j
        self.touched.add(int(j))
        self.first_movers.add(p)
        self.cur[e] = o[p]
        return o

    def drawn(self, e):
        oe = self.oenvs[e]
        return orc.sample_action(self.cur[e][MASK].astype(np.uint8), self.seed, self.g0 + e, oe.game_no, int(oe.state[5, 0, 0]))

    def check_current(self, h, tag='reset'):
        """the outputs of the CURRENT position of every env (after a reset): h = {'obs', 'mask', 'player', 'start_index'[, 'fobs']}"""
        for e, oe in enumerate(self.oenvs):
            o = self.cur[e]
            if 'start_index' in h:
                assert h['start_index'][e] == self.start_index[e], (tag, e, 'start_index')
            assert h['player'][e] == oe.player, (tag, e, 'player')
            assert np.array_equal(o[MASK], h['mask'][e]), (tag, e, 'mask')
            if 'obs' in h:
                assert o[POBS].tobytes() == h['obs'][e].tobytes(), (tag, e, 'observation')
            if 'fobs' in h:
                assert o[FOBS].tobytes() == h['fobs'][e].tobytes(), (tag, e, 'full observation')

    def step(self, acts=None, h=None, tag=''):
        """One step of every game with the actions acts[e] (default: the draw).  h: host arrays of ONE slot, [N, ...] each -- any of mask,
        obs, fobs, reward, done, player, invalid_action, ending_invalid, actions, start_index; compared where present."""
        h = h or {}
        for e, oe in enumerate(self.oenvs):
            a = self.drawn(e) if acts is None else int(acts[e])
            t = (tag, 'step', self.steps, 'env', e)
            o, rew, done, info = oe.step({oe.player: a})              # (the draws are valid actions: the oracle never raises here)
            if 'invalid_action' in h:
                assert h['invalid_action'][e] == 0, t
            if 'done' in h:
                assert bool(h['done'][e]) == done['__all__'], t + ('done',)
            if done['__all__']:
                self.restarts += 1
                if 'reward' in h:
                    assert (h['reward'][e, 0], h['reward'][e, 1]) == (rew[1], rew[-1]), t + ('reward',)
                if 'ending_invalid' in h:
                    assert bool(h['ending_invalid'][e]) == info[1]['game_result_was_invalid'], t + ('ending_invalid',)
                o = self.start(e)
            else:
                if 'reward' in h:
                    assert h['reward'][e, 0] == 0 and h['reward'][e, 1] == 0, t + ('reward',)
                if 'ending_invalid' in h:
                    assert h['ending_invalid'][e] == 0, t
                self.cur[e] = o[oe.player]
            p = oe.player
            if 'player' in h:
                assert h['player'][e] == p, t + ('player',)
            if 'start_index' in h:
                assert h['start_index'][e] == self.start_index[e], t + ('start_index', int(h['start_index'][e]), int(self.start_index[e]))
            if 'mask' in h:
                assert np.array_equal(self.cur[e][MASK], h['mask'][e]), t + ('mask',)
            if 'obs' in h and self.with_obs:
                assert self.cur[e][POBS].tobytes() == h['obs'][e].tobytes(), t + ('observation',)
            if 'fobs' in h:
                assert self.cur[e][FOBS].tobytes() == h['fobs'][e].tobytes(), t + ('full observation',)
            if 'actions' in h:
                assert h['actions'][e] == self.drawn(e), t + ('drawn action',)
        self.steps += 1


def follower_for(name, **kw):
    n, steps, pool_steps, restart, floor = CASES[name]
    v = VARIANTS[name]
    states, players = make_pool(v, pool_steps)
    return PoolFollower(v, n, states, players, restart, **kw), steps, floor


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_start_pool_symbols():
    from stratego_env_amd import _lib
    L = _lib.load()
    for sym in ('sgx_set_start_pool', 'sgx_set_start_index_out', 'sgx_start_pool_size'):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert L.sgx_abi_version() == _lib.ABI_VERSION == 15
    assert (_lib.POOL_RANDOM_FIRST_PLAYER, _lib.POOL_RESTART_CLOCK) == (1, 2)
    assert L.sgx_start_pool_size(None) == 0


def test_set_start_pool_fails_loudly_without_a_handle():
    """No device here, so no handle can exist: every entry point of the feature says so instead of touching anything."""
    from stratego_env_amd import _lib
    L = _lib.load()
    rc = L.sgx_set_start_pool(None, None, 0, 0)
    assert rc < 0 and b'sgx_set_start_pool' in L.sgx_last_error()
    rc = L.sgx_set_start_index_out(None, None)
    assert rc < 0 and b'sgx_set_start_index_out' in L.sgx_last_error()
    with pytest.raises(_lib.SgxError):
        _lib.check(L.sgx_set_start_pool(None, None, 1, 0), L)


# ---- input adequacy, oracle only --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_the_inputs_end_enough_games(name):
    """The follower alone, actions from the counter RNG like a rollout: the number of games that end (and restart from the pool) must
    reach the floor of the case -- the GPU test has to reproduce the follower's count exactly."""
    fo, steps, floor = follower_for(name)
    assert len(fo.states) == POOL_N
    for _ in range(steps):
        fo.step()
    print('%s: %d endings in %d x %d steps, %d of %d pool entries touched' % (name, fo.restarts, fo.n, steps, len(fo.touched), POOL_N))
    assert fo.restarts >= floor, (name, fo.restarts, floor)
    assert all(0 <= j < POOL_N for j in fo.touched)
