"""Playouts (sgx_playout) without a GPU: the binding, and the numpy restatement of the rule (tests/playout_rule.py, what the device
kernel is held to bit for bit in tests/test_gpu_playout.py) checked against the oracle's rules on roots taken from the golden games."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib
from stratego_env_amd.config import VARIANTS
from tests import playout_rule as pr
from tests.pool_roots import sampled_states

GAME_SETS = ['micro', 'tiny', 'fives']


def test_the_binding():
    assert C.sizeof(_lib.SgxPlayoutIO) == 48
    offsets = {name: getattr(_lib.SgxPlayoutIO, name).offset for name, _ in _lib.SgxPlayoutIO._fields_}
    assert offsets == {'reward_dev': 0, 'done_dev': 8, 'ending_invalid_dev': 16, 'player_dev': 24, 'length_dev': 32, 'max_steps': 40, 'flags': 44}
    assert 'sgx_playout' in _lib.EXPORTED_SYMBOLS
    assert _lib.LAUNCH_PLAYOUT == 4
    assert _lib.ABI_VERSION == 15                       # no struct or signature of the existing ABI changed


def test_the_library_exports_the_entry_point():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_playout.argtypes) == 6
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message
    assert L.sgx_playout(None, None, None, None, 0, None) != 0
    assert b'NULL' in L.sgx_last_error()


@pytest.mark.parametrize('name', GAME_SETS)
def test_a_playout_ends_its_game(name):
    v = VARIANTS[name]
    ru = orc.OracleRules(v.rows, v.columns)
    roots = sampled_states(name)
    assert len(roots) >= 6
    finished_roots = 0
    for si, (st, mover) in enumerate(roots):
        turn = int(st[5, 0, 0])
        root_over = ru.get_game_ended(st, 1) != 0
        finished_roots += int(root_over)
        final, player, reward, done, ending_invalid, length = pr.playout(name, st, mover, seed=0x5EED, g=si, draw=0)
        where = (name, si)
        assert done == 1, where
        assert ru.get_game_ended(final, 1) != 0, where
        if root_over:                                   # a root that is over: length 0 and its own result
            assert length == 0 and np.array_equal(final, st) and player == mover, where
            inv = ru.get_game_result_is_invalid(st)
            assert ending_invalid == int(inv), where
            want = (0.0, 0.0) if inv else (ru.get_game_ended(st, 1), ru.get_game_ended(st, -1))
            assert reward.tolist() == [np.float32(want[0]), np.float32(want[1])], where
        else:
            assert 1 <= length <= v.max_turns - turn, where
            assert int(final[5, 0, 0]) == turn + length, where
        assert ending_invalid == int(ru.get_game_result_is_invalid(final)), where
        if ending_invalid:
            assert reward.tolist() == [0.0, 0.0], where
        else:
            assert reward[0] == np.float32(ru.get_game_ended(final, 1)) and reward[1] == np.float32(ru.get_game_ended(final, -1)), where
    assert finished_roots > 0                           # (sampled_states keeps every game's last position)


@pytest.mark.parametrize('name', GAME_SETS)
def test_max_steps_three_is_three_next_states(name):
    v = VARIANTS[name]
    ru = orc.OracleRules(v.rows, v.columns)
    checked = 0
    for si, (st, mover) in enumerate(sampled_states(name)):
        if ru.get_game_ended(st, 1) != 0:
            continue
        final, player, reward, done, ending_invalid, length = pr.playout(name, st, mover, seed=3, g=si, draw=7, max_steps=3)
        # the same three moves through get_next_state: spatial action in the mover's perspective -> absolute 1-D index
        cur, pl, n = np.asarray(st, dtype=np.int64), int(mover), 0
        while n < 3 and ru.get_game_ended(cur, 1) == 0:
            mask = ru.get_valid_moves_as_spatial_mask(ru.get_state_from_player_perspective(cur, pl), 1).reshape(-1)     # maenv:452-454
            valid = np.flatnonzero(mask)
            k = orc.rng_below(orc.rng(3, si, 7, pr.STREAM_PLAYOUT, int(cur[5, 0, 0])), len(valid))
            spatial = np.unravel_index(int(valid[k]), (v.rows, v.columns, ru.K))
            a = ru.get_action_1d_index_from_player_perspective(ru.get_action_1d_index_from_spatial_index(tuple(int(x) for x in spatial)), pl)
            cur, pl = ru.get_next_state(cur, pl, int(a))
            n += 1
        assert length == n and np.array_equal(final, cur) and player == pl, (name, si)
        over = ru.get_game_ended(cur, 1) != 0
        assert done == int(over), (name, si)
        if not over:                                    # cut off: nothing to report
            assert reward.tolist() == [0.0, 0.0] and ending_invalid == 0, (name, si)
        checked += 1
    assert checked >= 5


def test_the_key_selects_the_game():
    name = 'fives'
    st, mover = sampled_states(name, 1)[1]
    games = set()
    for seed, g, draw in ((0, 0, 0), (0, 0, 1), (0, 0, 1 << 40), (0, 1, 0), (0, 2, 0), (1, 0, 0)):
        final, player, reward, done, ending_invalid, length = pr.playout(name, st, mover, seed, g, draw)
        games.add((final.tobytes(), length))
        again = pr.playout(name, st, mover, seed, g, draw)                 # the same key gives the same game
        assert np.array_equal(again[0], final) and again[5] == length and again[2].tobytes() == reward.tobytes()
    assert len(games) >= 4                              # draw, slot and seed all enter the key
    # two draws and two slots of one root differ somewhere
    a = pr.playout(name, st, mover, 5, 0, 0)
    assert not np.array_equal(a[0], pr.playout(name, st, mover, 5, 0, 1)[0]) or not np.array_equal(a[0], pr.playout(name, st, mover, 5, 1, 0)[0])


def test_the_batch_gathers_like_the_device_call():
    name = 'micro'
    roots = sampled_states(name)
    states = np.stack([s for s, _ in roots])
    players = np.asarray([p for _, p in roots], dtype=np.int8)
    idx = np.asarray([2, 2, 0, 1, 2], dtype=np.int32)
    out, out_players, reward, done, ending_invalid, length = pr.playout_batch(name, states, players, 9, 100, 4, idx, max_steps=5)
    assert out.shape == (5,) + states.shape[1:] and reward.dtype == np.float32 and length.dtype == np.int32
    for i, s in enumerate(idx):
        one = pr.playout(name, states[s], int(players[s]), 9, 100 + i, 4, 5)
        assert np.array_equal(out[i], one[0]) and out_players[i] == one[1] and length[i] == one[5] and done[i] == one[3]
