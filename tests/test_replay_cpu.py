"""Replay (sgx_replay) without a GPU: the binding, and the numpy restatement of the rule (tests/replay_rule.py, what the device
kernel is held to bit for bit in tests/test_gpu_replay.py) checked against the golden games recorded from the reference."""
import ctypes as C

import numpy as np
import pytest

from stratego_env_amd import _lib
from tests import replay_rule as rr
from tests.helpers import load_games, oracle_env

GAME_SETS = ['micro', 'tiny', 'fives']


def test_the_binding():
    assert C.sizeof(_lib.SgxReplayIO) == 104
    offsets = {name: getattr(_lib.SgxReplayIO, name).offset for name, _ in _lib.SgxReplayIO._fields_}
    assert offsets == {'actions_dev': 0, 'lengths_dev': 8, 'applied_dev': 16, 'consumed_dev': 24, 'stop_dev': 32, 'reward_dev': 40,
                       'done_dev': 48, 'ending_invalid_dev': 56, 'player_dev': 64, 'game_stride': 72, 'step_stride': 80,
                       'actions_elems': 88, 'max_len': 96, 'flags': 100}
    assert 'sgx_replay' in _lib.EXPORTED_SYMBOLS
    assert (_lib.REPLAY_SKIP_INVALID, _lib.REPLAY_ACTIONS_1D, _lib.REPLAY_ALLOW_OSCILLATION) == (1, 2, 4)
    assert _lib.LAUNCH_REPLAY == 5
    assert _lib.ABI_VERSION == 15                       # no struct or signature of the existing ABI changed


def test_the_library_exports_the_entry_point():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_replay.argtypes) == 5
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message that names the call
    assert L.sgx_replay(None, None, None, None, None) != 0
    assert b'sgx_replay' in L.sgx_last_error()


def _games(name):
    """-> (g, [(root state, list, errors)] per game): the root is what env.reset(p1_map, p2_map) gives."""
    g = load_games(name)
    off = g['offsets']
    env = oracle_env(name)
    out = []
    for gi in range(len(off) - 1):
        env.reset(g['p1_maps'][gi].astype(np.int64), g['p2_maps'][gi].astype(np.int64))
        out.append((env.state.copy(), g['actions'][off[gi]:off[gi + 1]].astype(np.int32), g['errors'][off[gi]:off[gi + 1]].astype(bool)))
    return g, out


@pytest.mark.parametrize('name', GAME_SETS)
def test_skip_mode_reaches_the_recorded_final_states(name):
    g, games = _games(name)
    total_errors = 0
    for gi, (root, acts, errs) in enumerate(games):
        final, player, reward, done, ending_invalid, applied, consumed, stop = rr.replay(name, root, 1, acts, skip_invalid=True)
        where = (name, gi)
        assert np.array_equal(final, g['final_states'][gi].astype(np.int64)), where
        assert consumed == len(acts) and applied == len(acts) - int(errs.sum()) and stop == rr.STOP_EXHAUSTED, where
        assert done == int(bool(g['finished'][gi])), where
        if done:
            assert ending_invalid == int(bool(g['ending_invalid'][gi])), where
            last = g['offsets'][gi] + int(np.flatnonzero(~errs)[-1])
            assert tuple(reward) == tuple(np.float32(x) for x in g['rewards'][last]), where
        total_errors += int(errs.sum())
    assert total_errors > 0                             # (these sets were recorded with invalid actions among the moves)


@pytest.mark.parametrize('name', GAME_SETS)
def test_stop_mode_ends_at_the_first_invalid_entry(name):
    g, games = _games(name)
    env = oracle_env(name)
    stopped = 0
    for gi, (root, acts, errs) in enumerate(games):
        final, player, reward, done, ending_invalid, applied, consumed, stop = rr.replay(name, root, 1, acts)
        where = (name, gi)
        if not errs.any():
            assert stop == rr.STOP_EXHAUSTED and consumed == len(acts), where
            assert np.array_equal(final, g['final_states'][gi].astype(np.int64)), where
            continue
        k = int(np.flatnonzero(errs)[0])
        assert stop == rr.STOP_INVALID and consumed == k and applied == k, where
        # the oracle's position after that prefix
        env.reset(initial_state_override=root, first_player_override=1)
        for a in acts[:k]:
            env.step({env.player: int(a)})
        assert np.array_equal(final, env.state) and player == env.player, where
        stopped += 1
    assert stopped > 0


@pytest.mark.parametrize('name', GAME_SETS)
def test_entries_after_the_end_of_the_game_are_not_read(name):
    g, games = _games(name)
    checked = 0
    for gi, (root, acts, errs) in enumerate(games):
        if not g['finished'][gi]:
            continue
        longer = np.concatenate([acts, np.asarray([0, -1, 3, 1 << 30], dtype=np.int32)])
        for skip in (True, False):
            if errs.any() and not skip:
                continue
            final, player, reward, done, ending_invalid, applied, consumed, stop = rr.replay(name, root, 1, longer, skip_invalid=skip)
            assert stop == rr.STOP_GAME_OVER and consumed == len(acts) and done == 1, (name, gi, skip)
            assert np.array_equal(final, g['final_states'][gi].astype(np.int64)), (name, gi, skip)
        checked += 1
    assert checked > 0


@pytest.mark.parametrize('name', GAME_SETS)
def test_a_replay_in_two_parts_is_the_replay(name):
    g, games = _games(name)
    for gi, (root, acts, errs) in enumerate(games[:24]):
        whole = rr.replay(name, root, 1, acts, skip_invalid=True)
        for k in sorted({0, 1, len(acts) // 2, len(acts)}):
            first = rr.replay(name, root, 1, acts[:k], skip_invalid=True)
            second = rr.replay(name, first[0], first[1], acts[k:], skip_invalid=True)
            assert np.array_equal(second[0], whole[0]) and second[1] == whole[1], (name, gi, k)
            assert second[2].tobytes() == whole[2].tobytes() and second[3:5] == whole[3:5], (name, gi, k)
            assert first[5] + second[5] == whole[5] and first[6] + second[6] == whole[6], (name, gi, k)


def test_the_batch_gathers_like_the_device_call():
    name = 'micro'
    g, games = _games(name)
    states = np.stack([r for r, _, _ in games[:3]])
    players = np.ones(3, dtype=np.int8)
    idx = np.asarray([2, 2, 0, 1], dtype=np.int32)
    L = 6
    acts = np.full((4, L), -1, dtype=np.int32)
    for i, s in enumerate(idx):
        a = games[s][1][:L]
        acts[i, :len(a)] = a
    lengths = np.asarray([6, 2, 0, 9], dtype=np.int32)              # (9: clamped to the width of the tensor)
    out = rr.replay_batch(name, states, players, acts, lengths, idx, skip_invalid=True)
    assert out[0].shape == (4,) + states.shape[1:] and out[5].dtype == np.int32 and out[7].dtype == np.uint8
    for i, s in enumerate(idx):
        one = rr.replay(name, states[s], 1, acts[i], int(lengths[i]), skip_invalid=True)
        assert np.array_equal(out[0][i], one[0]) and out[1][i] == one[1] and out[5][i] == one[5] and out[6][i] == one[6] and out[7][i] == one[7]
    assert out[6][2] == 0 and np.array_equal(out[0][2], states[0])   # a list of length 0: the root
