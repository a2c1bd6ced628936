"""Weighted playouts (sgx_playout_weighted) without a GPU: the binding and the host-side refusals, the numpy restatement of the rule
(tests/weighted_playout_rule.py, what the device kernel is held to bit for bit in tests/test_gpu_weighted_playout.py) against the two
consequences the rule promises -- a constant table plays sgx_playout's games, a weight of 0 is never drawn next to a positive one --, the
two views, the distribution of the first move, and the ready-made tables of stratego_env_amd.playout_policies."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib, playout_policies as pol
from stratego_env_amd.config import VARIANTS
from tests import draw_stats as ds, playout_rule as pr, weighted_playout_rule as wr
from tests.pool_roots import sampled_states
from tests.tables import _p16, attacks_only_table, third_zero_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAME_SETS = ['micro', 'tiny', 'fives']


def test_the_binding():
    assert 'sgx_playout_weighted' in _lib.EXPORTED_SYMBOLS
    assert _lib.LAUNCH_PLAYOUT_WEIGHTED == 7 and _lib.PLAYOUT_SEE_ALL == 1
    assert _lib.ABI_VERSION == 15                       # an addition within v15: no struct or signature of the existing ABI changed
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    assert re.search(r'#define SGX_LAUNCH_PLAYOUT_WEIGHTED 7\b', hdr) and re.search(r'#define SGX_PLAYOUT_SEE_ALL 1\b', hdr)
    assert re.search(r'#define SGX_ABI_VERSION 15\b', hdr)


def test_the_library_refuses_on_the_host():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_playout_weighted.argtypes) == 8
    w = pol.uniform()
    io = _lib.SgxPlayoutIO(None, None, None, None, None, 0, 0)
    # a NULL handle is SGX_EINVAL with a message, whatever else is passed
    assert L.sgx_playout_weighted(None, None, None, io, _p16(w), 0, 0, None) == -1
    assert b'sgx_playout_weighted' in L.sgx_last_error() and b'NULL' in L.sgx_last_error()
    # the table and the policy flags are looked at before the handles are (so no device is needed to get these refusals): a NULL table, an
    # entry of 4096 (the first offender's indices named), unknown policy bits
    assert L.sgx_playout_weighted(None, None, None, io, None, 0, 0, None) == -1
    assert b'weights is NULL' in L.sgx_last_error()
    bad = pol.uniform()
    bad[2, 7, 9] = 4096
    bad[3, 1, 1] = 5000
    assert L.sgx_playout_weighted(None, None, None, io, _p16(bad), 0, 0, None) == -1
    assert b'weights[2][7][9] = 4096' in L.sgx_last_error(), L.sgx_last_error()
    for flags in (2, 4, -1):
        assert L.sgx_playout_weighted(None, None, None, io, _p16(w), flags, 0, None) == -1
        assert b'policy_flags' in L.sgx_last_error()


def test_the_python_side_checks_the_table():
    from stratego_env_amd.procedural_env import playout_weights
    w = playout_weights(np.full(wr.SHAPE, 7, dtype=np.int64))
    assert w.dtype == np.uint16 and w.flags['C_CONTIGUOUS'] and w.shape == wr.SHAPE and (w == 7).all()
    import torch
    assert np.array_equal(playout_weights(torch.full(wr.SHAPE, 9, dtype=torch.int32)), np.full(wr.SHAPE, 9))
    assert np.array_equal(playout_weights(np.full(wr.SHAPE, 3).transpose(0, 1, 2)[:, :, ::1]), np.full(wr.SHAPE, 3))
    for bad in (np.zeros((4, 13, 13), dtype=np.int32), np.zeros(wr.SHAPE, dtype=np.float32)):
        with pytest.raises(ValueError):
            playout_weights(bad)
    for value, idx in ((4096, (1, 2, 3)), (-1, (3, 12, 13))):
        t = np.ones(wr.SHAPE, dtype=np.int64)
        t[idx] = value
        with pytest.raises(ValueError) as ei:
            playout_weights(t)
        assert 'weights[%d][%d][%d]' % idx in str(ei.value)


@pytest.fixture(scope='module')
def uniform_games():
    """playout_rule.playout of every sampled root of every game set, once: {name: [(root, mover, result)]}"""
    return {name: [(st, mover, pr.playout(name, st, mover, seed=0x5EED, g=si, draw=2)) for si, (st, mover) in enumerate(sampled_states(name))]
            for name in GAME_SETS}


@pytest.mark.parametrize('name', GAME_SETS)
@pytest.mark.parametrize('c', [1, 7, 4095])
def test_a_constant_table_plays_the_uniform_games(name, c, uniform_games):
    """floor(floor(h c n / 2^32) / c) = floor(h n / 2^32): with w_i = c the first prefix sum above x is that of move floor(x / c)."""
    table = np.full(wr.SHAPE, c, dtype=np.uint16)
    for see_all in (False, True):
        for si, (st, mover, want) in enumerate(uniform_games[name]):
            got = wr.playout(name, st, mover, 0x5EED, si, 2, table, see_all)
            where = (name, c, see_all, si)
            assert np.array_equal(got[0], want[0]) and got[1] == want[1], where
            assert got[2].tobytes() == want[2].tobytes() and got[3:6] == want[3:6], where
            assert got[6] == 0 and got[7] == want[5], where                 # every position played had W > 0


@pytest.mark.parametrize('name', GAME_SETS)
def test_a_weight_of_zero_is_never_drawn_next_to_a_positive_one(name):
    table = third_zero_table()
    assert 0.2 < float((table == 0).mean()) < 0.4
    zero = pos = 0
    for see_all in (False, True):
        for si, (st, mover) in enumerate(sampled_states(name)):
            trace = []
            out = wr.playout(name, st, mover, 3, si, 1, table, see_all, trace=trace)
            assert out[6] + out[7] == len(trace) == out[5]
            for w, k in trace:
                if w.sum() > 0:
                    assert w[k] > 0, (name, si)
                    pos += 1
                else:
                    zero += 1
    assert pos > 0
    # a table that weighs attacks only: most positions offer none (W == 0, the uniform draw), some do (W > 0, and then an attack is played)
    table = attacks_only_table()
    n_zero = n_pos = 0
    for si, (st, mover) in enumerate(sampled_states(name)):
        trace = []
        out = wr.playout(name, st, mover, 3, si, 1, table, trace=trace)
        n_zero, n_pos = n_zero + out[6], n_pos + out[7]
        for w, k in trace:
            assert w.sum() == 0 or w[k] == 5
    assert n_zero > 0 and n_pos > 0, (name, n_zero, n_pos)


def _all_revealed(st):
    return not ((st[3] == 13).any() or (st[4] == 13).any())


@pytest.mark.parametrize('name', GAME_SETS)
def test_the_two_views(name):
    """The public view indexes the table with 13 where see_all indexes it with the true type: with a table that tells them apart the two
    views play different games from a root with unrevealed opponents, and the same game from a root where everything is revealed."""
    table = third_zero_table(1)
    differ = revealed_roots = 0
    for si, (st, mover) in enumerate(sampled_states(name)):
        over = orc.OracleRules(VARIANTS[name].rows, VARIANTS[name].columns).get_game_ended(st, 1) != 0
        a = wr.playout(name, st, mover, 8, si, 0, table, False)
        b = wr.playout(name, st, mover, 8, si, 0, table, True)
        same = np.array_equal(a[0], b[0]) and a[5] == b[5]
        if _all_revealed(st):
            revealed_roots += 1
            assert same, (name, si)
        elif not over:
            differ += int(not same)
    assert differ > 0, name
    print(name, 'roots with everything revealed among the samples:', revealed_roots)        # (the assertion above covers them when there are any)


def test_the_first_move_follows_the_weights():
    """One Fives root, 65,536 slots, the first move: counts against w_i / W, by the rejection rule of the other draws (draw_stats.check);
    the same statistic rejects a sampler that ignores the weights."""
    name = 'fives'
    table = third_zero_table(2)
    st, mover = sampled_states(name)[16]                                   # 13 valid moves, two of them of weight 0 under this table
    env = pr._env(name)
    obs = env.reset(initial_state_override=np.asarray(st, dtype=np.int64), first_player_override=int(mover))
    valid = np.flatnonzero(np.asarray(obs[env.player][env.MASK]).reshape(-1))
    w = wr.move_weights(name, st, mover, valid, table)
    W, n = int(w.sum()), len(w)
    assert n >= 6 and (w > 0).sum() >= 4 and (w == 0).any(), w
    g = np.arange(ds.N_KEYS)
    r = ds.np_rng(11, g, 5, ds.STREAM_PLAYOUT, int(st[5, 0, 0]))
    picks = np.searchsorted(np.cumsum(w), ds.np_rng_below(r, W), side='right')
    for i in range(0, ds.N_KEYS, 4099):                                   # the vectorised draw is the rule's
        assert picks[i] == wr.pick(orc.rng(11, int(g[i]), 5, ds.STREAM_PLAYOUT, int(st[5, 0, 0])), w)[0]
    expected = ds.N_KEYS * w / W
    ds.check('first move against w / W', ds.chi2_fit(np.bincount(picks, minlength=n), expected))
    assert np.bincount(picks, minlength=n)[w == 0].sum() == 0
    ignorant = ds.np_rng_below(r, n)                                       # the uniform sampler
    chi2, limit = ds.report('a sampler that ignores the weights', ds.chi2_fit(np.bincount(ignorant, minlength=n), expected))
    assert chi2 > limit


def test_playout_policies_from_reward_matrix():
    u = pol.uniform()
    assert u.dtype == np.uint16 and u.shape == wr.SHAPE and (u == 1).all()
    z = pol.from_reward_matrix(np.zeros((13, 13)))
    assert z.dtype == np.uint16 and z.shape == wr.SHAPE and (z == 64).all()
    assert (pol.from_reward_matrix(np.zeros((13, 14)), scale=9) == 9).all()
    # monotone in the reward, for every direction factor and temperature tried
    r = np.linspace(-3, 3, 13 * 14).reshape(13, 14)
    for temperature in (0.5, 1.0, 4.0):
        w = pol.from_reward_matrix(r, temperature=temperature, direction=(3, 1, 2, 2)).astype(np.int64)
        assert (np.diff(w.reshape(4, -1), axis=1) >= 0).all()
        assert w[0].max() > w[0].min()
        assert (w[0] >= w[1]).all() and (w[2] == w[3]).all()
    # clipped at both ends, rounded to the nearest
    big = pol.from_reward_matrix(np.full((13, 14), 50.0))
    assert (big == 4095).all()
    assert (pol.from_reward_matrix(np.full((13, 14), -50.0)) == 0).all()
    assert (pol.from_reward_matrix(np.full((13, 14), np.log(2.4)), scale=1) == 2).all() and (pol.from_reward_matrix(np.full((13, 14), np.log(2.6)), scale=1) == 3).all()
    # a [13][13] matrix: the unknown column takes the empty cell's reward
    m = np.zeros((13, 13)); m[:, 0] = 1.0
    w = pol.from_reward_matrix(m)
    assert (w[:, :, 13] == w[:, :, 0]).all() and (w[:, :, 0] > w[:, :, 1]).all()
    for bad in (dict(reward_matrix=np.zeros((12, 13))), dict(reward_matrix=np.zeros((13, 13)), temperature=0),
                dict(reward_matrix=np.zeros((13, 13)), direction=(1, 1, 1))):
        with pytest.raises(ValueError):
            pol.from_reward_matrix(**bad)


def _oracle_attack(ru, attacker, defender):
    """+1 / 0 / -1: what the oracle's get_next_state makes of `attacker` (player +1) moving onto `defender` (player -1) on a 5x5 board"""
    st = ru.create_initial_state(np.zeros((5, 5)), np.zeros((5, 5)), np.zeros((5, 5)), 100)
    st[0, 0, 0] = 11; st[3, 0, 0] = 13
    st[0, 1, 1] = attacker; st[3, 1, 1] = 13
    st[1, 2, 1] = defender; st[4, 2, 1] = 13
    if defender != 11:
        st[1, 4, 4] = 11; st[4, 4, 4] = 13
    nxt, _ = ru.get_next_state(st, 1, ru.get_action_1d_index_from_positions(1, 1, 2, 1))
    mine, theirs = int(nxt[0, 2, 1]), int(nxt[1, 2, 1])
    assert (mine, theirs) in ((attacker, 0), (0, 0), (0, defender))
    return 1 if mine else (0 if not theirs else -1)


def test_capture_biased_follows_the_combat_rule():
    ru = orc.OracleRules(5, 5)
    for variant in (None, 'barrage', 'standard', 'fives'):
        for forward in (1, 2, 5):
            w = pol.capture_biased(variant, forward=forward).astype(np.int64)
            assert w.shape == wr.SHAPE and w.max() <= 4095
            for t in range(1, 11):
                for d in range(1, 13):
                    outcome = _oracle_attack(ru, t, d)
                    assert outcome == pol.attack_outcome(t, d), (t, d)
                    for direction in range(4):
                        quiet, attack = w[direction, t, 0], w[direction, t, d]
                        if outcome > 0:
                            assert attack > quiet, (variant, direction, t, d)
                        elif outcome < 0:
                            assert attack < quiet, (variant, direction, t, d)
                assert (w[0, t] == forward * w[1, t]).all() and (w[1, t] == w[2, t]).all() and (w[2, t] == w[3, t]).all()
            # weight(win) > weight(quiet move) > weight(loss) as single numbers too
            assert w[1, 10, 9] > w[1, 10, 0] > w[1, 9, 10] > 0
