"""Piece origins (sgx_set_replay_origins) without a GPU: known answers of the rule's numpy restatement (tests/origins_rule.py,
what the tracked replay kernel is held to bit for bit in tests/test_gpu_origins.py) on hand-built positions, its invariants over the golden
games of every variant, chaining, beliefs.follow, and the ABI."""
import os
import re

import numpy as np
import pytest

from stratego_env_amd import _lib, beliefs
from tests import origins_rule as orr
from tests.helpers import load_games, oracle_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ['barrage', 'standard', 'micro', 'tiny', 'fives', 'medium', 'octa_barrage', 'short_barrage', 'short_standard', 'standard2']
SGX_EINVAL = -1
FLAG, SCOUT = 11, 2


# ---- known answers on the 4x4 board ('tiny': no obstacles).  Cells are absolute, r * 4 + c; player +1 moves first -------------------------
def _position(p1, p2):
    """{(r, c): type} per player, absolute coordinates -> the reference state env.reset builds from the two own-side maps"""
    env = oracle_env('tiny')
    m1, m2 = np.zeros((4, 4), dtype=np.int64), np.zeros((4, 4), dtype=np.int64)
    for (r, c), t in p1.items():
        m1[r, c] = t
    for (r, c), t in p2.items():
        m2[3 - r, 3 - c] = t                                          # player -1's map is in its own perspective
    env.reset(m1, m2)
    state = env.state.copy()
    for (r, c), t in p1.items():
        assert state[0, r, c] == t
    for (r, c), t in p2.items():
        assert state[1, r, c] == t
    return state


def _a(sr, sc, er, ec):
    return oracle_env('tiny').rules.get_action_1d_index_from_positions(sr, sc, er, ec)


def _labels(state, actions, **kw):
    lab, final, player, m, c, stop = orr.replay_tracked('tiny', state, 1, np.asarray(actions, dtype=np.int32), actions_1d=True, **kw)
    return lab, m, c, stop


def _want(p1, p2):
    """{cell: label} per player -> int16 [2, 16], -1 elsewhere"""
    w = np.full((2, 16), -1, dtype=np.int16)
    for q, d in enumerate((p1, p2)):
        for cell, v in d.items():
            w[q, cell] = v
    return w


BASE1, BASE2 = {(0, 0): FLAG}, {(3, 3): FLAG}


def test_start_labels_are_the_cells_of_the_pieces():
    s = _position({**BASE1, (1, 1): 5}, {**BASE2, (2, 2): 6})
    lab, m, c, stop = _labels(s, [])
    assert (m, c, stop) == (0, 0, 0)
    assert np.array_equal(lab, _want({0: 0, 5: 5}, {15: 15, 10: 10}))


def test_a_move_to_an_empty_cell_carries_the_label():
    s = _position({**BASE1, (1, 1): 5}, {**BASE2, (2, 2): 6})
    lab, m, c, stop = _labels(s, [_a(1, 1, 2, 1)])
    assert m == 1
    assert np.array_equal(lab, _want({0: 0, 9: 5}, {15: 15, 10: 10}))


def test_a_won_attack_carries_the_movers_label_and_drops_the_defenders():
    s = _position({**BASE1, (1, 1): 6}, {**BASE2, (2, 1): 4, (2, 3): 5})
    lab, m, c, stop = _labels(s, [_a(1, 1, 2, 1)])
    assert m == 1
    assert np.array_equal(lab, _want({0: 0, 9: 5}, {15: 15, 11: 11}))


def test_a_lost_attack_drops_the_movers_label_only():
    s = _position({**BASE1, (1, 1): 4, (1, 3): 5}, {**BASE2, (2, 1): 6})
    lab, m, c, stop = _labels(s, [_a(1, 1, 2, 1)])
    assert m == 1
    assert np.array_equal(lab, _want({0: 0, 7: 7}, {15: 15, 9: 9}))


def test_a_drawn_attack_drops_both_labels():
    s = _position({**BASE1, (1, 1): 5, (1, 3): 5}, {**BASE2, (2, 1): 5, (2, 3): 5})
    lab, m, c, stop = _labels(s, [_a(1, 1, 2, 1)])
    assert m == 1
    assert np.array_equal(lab, _want({0: 0, 7: 7}, {15: 15, 11: 11}))


def test_a_long_scout_move_carries_the_label():
    s = _position({**BASE1, (0, 2): SCOUT}, {**BASE2, (2, 1): 5})
    lab, m, c, stop = _labels(s, [_a(0, 2, 3, 2)])
    assert m == 1
    assert np.array_equal(lab, _want({0: 0, 14: 2}, {15: 15, 9: 9}))


def test_a_flag_capture_is_a_won_attack_and_later_entries_are_not_applied():
    s = _position({**BASE1, (2, 3): 5}, {**BASE2, (2, 1): 5})
    capture = _a(2, 3, 3, 3)
    want = _want({0: 0, 15: 11}, {9: 9})
    lab, m, c, stop = _labels(s, [capture])
    assert m == 1 and np.array_equal(lab, want)
    # entries after the end of the game: a move of the piece that is still there is not read
    lab, m, c, stop = _labels(s, [capture, _a(2, 1, 1, 1), _a(3, 3, 3, 2)], skip_invalid=True)
    assert (m, c, stop) == (1, 1, 1) and np.array_equal(lab, want)


def test_a_skipped_or_refused_entry_changes_nothing():
    s = _position({**BASE1, (1, 1): 5}, {**BASE2, (2, 2): 6})
    start = _want({0: 0, 5: 5}, {15: 15, 10: 10})
    bad = _a(0, 0, 1, 0)                                              # the flag does not move
    lab, m, c, stop = _labels(s, [bad, _a(1, 1, 2, 1)], skip_invalid=True)
    assert (m, c, stop) == (1, 2, 0)
    assert np.array_equal(lab, _want({0: 0, 9: 5}, {15: 15, 10: 10}))
    lab, m, c, stop = _labels(s, [bad, _a(1, 1, 2, 1)])
    assert (m, c, stop) == (0, 0, 2) and np.array_equal(lab, start)


def test_given_labels_are_carried_verbatim():
    s = _position({**BASE1, (1, 1): 5}, {**BASE2, (2, 2): 6})
    given = (np.arange(32).reshape(2, 16) * 1000 - 16000).astype(np.int16)   # what empty cells hold is ignored
    given[0, 5], given[1, 10] = -1, -32768
    lab, m, c, stop = _labels(s, [_a(1, 1, 2, 1), _a(2, 2, 1, 2)], origin_in=given)
    assert m == 2
    assert np.array_equal(lab, _want({0: given[0, 0], 9: -1}, {15: given[1, 15], 6: -32768}))


# ---- the golden games of every variant, played whole with identity labels ------------------------------------------------------------------
def _golden(name):
    g = load_games(name)
    off = g['offsets']
    env = oracle_env(name)
    for gi in range(len(off) - 1):
        env.reset(g['p1_maps'][gi].astype(np.int64), g['p2_maps'][gi].astype(np.int64))
        yield gi, env.state.copy(), g['actions'][off[gi]:off[gi + 1]].astype(np.int32), g['final_states'][gi].astype(np.int64)


def check_invariants(lab, start, final, where):
    """the three invariants of identity labels: a label exactly where a piece is, no label twice, and the piece is of the type that started
    on the cell its label names"""
    for q in range(2):
        occ = final[q].reshape(-1) != 0
        assert np.array_equal(lab[q] != -1, occ), where
        ids = lab[q][occ]
        assert len(set(ids.tolist())) == len(ids), where
        assert np.array_equal(final[q].reshape(-1)[occ], start[q].reshape(-1)[ids]), where


@pytest.mark.parametrize('name', GOLDEN)
def test_invariants_over_the_golden_games(name):
    moved = 0
    for gi, root, acts, want_final in _golden(name):
        lab, final, player, m, c, stop = orr.replay_tracked(name, root, 1, acts, skip_invalid=True)
        assert np.array_equal(final, want_final), (name, gi)
        check_invariants(lab, root, final, (name, gi))
        moved += int((lab != orr.start_labels(root)).any())
    assert moved > 0


@pytest.mark.parametrize('name', ['micro', 'fives', 'barrage'])
def test_two_halves_chained_through_origins_in_equal_one_pass(name):
    rs = np.random.RandomState(3)
    for gi, root, acts, _ in list(_golden(name))[:6]:
        cells = root[0].size
        for given in (None, rs.randint(-32768, 32768, size=(2, cells)).astype(np.int16)):
            if given is not None:
                given[0, ::3] = -1                                     # -1 is a label like any other
            whole = orr.replay_tracked(name, root, 1, acts, skip_invalid=True, origin_in=given)
            k = len(acts) // 2
            first = orr.replay_tracked(name, root, 1, acts[:k], skip_invalid=True, origin_in=given)
            second = orr.replay_tracked(name, first[1], first[2], acts[k:], skip_invalid=True, origin_in=first[0])
            assert np.array_equal(second[0], whole[0]) and np.array_equal(second[1], whole[1]), (name, gi)
            if given is not None:
                occ = np.stack([whole[1][q].reshape(-1) != 0 for q in range(2)])
                assert set(whole[0][occ].tolist()) <= set(given.reshape(-1).tolist())
                assert (whole[0][~occ] == -1).all()


# ---- beliefs.follow ------------------------------------------------------------------------------------------------------------------------------
def _follow_loops(prior, origins):
    n, _, cells = origins.shape
    out = np.zeros((n, 2, 12, cells), dtype=prior.dtype)
    for i in range(n):
        for p in range(2):
            for c in range(cells):
                o = int(origins[i, p, c])
                if 0 <= o < cells:
                    out[i, p, :, c] = (prior[p] if prior.ndim == 3 else prior[i, p])[:, o]
    return out


def test_follow_against_a_triple_loop():
    rs = np.random.RandomState(5)
    n, cells = 7, 25
    origins = rs.randint(-3, cells + 3, size=(n, 2, cells)).astype(np.int16)
    origins[0, 0, 0], origins[0, 1, 1] = -32768, 32767
    for shape in ((2, 12, cells), (n, 2, 12, cells)):
        prior = rs.randint(0, 4096, size=shape).astype(np.uint16)
        got = beliefs.follow(prior, origins)
        assert got.dtype == prior.dtype and got.shape == (n, 2, 12, cells)
        assert np.array_equal(got, _follow_loops(prior, origins))
    with pytest.raises(ValueError):
        beliefs.follow(np.zeros((2, 12, cells + 1), dtype=np.uint16), origins)
    with pytest.raises(ValueError):
        beliefs.follow(np.zeros((2, 12, cells), dtype=np.uint16), origins[:, 0])


def _one_hot(state):
    """uint16 [2, 12, cells]: 4095 where that player has that type on that cell"""
    cells = state[0].size
    t = np.zeros((2, 12, cells), dtype=np.uint16)
    for q in range(2):
        own = state[q].reshape(-1)
        occ = np.flatnonzero(own)
        t[q, own[occ] - 1, occ] = 4095
    return t


def test_a_one_hot_prior_on_the_start_followed_through_a_game_is_one_hot_on_the_end():
    for name in ('fives', 'barrage'):
        for gi, root, acts, _ in list(_golden(name))[:4]:
            lab, final, player, m, c, stop = orr.replay_tracked(name, root, 1, acts, skip_invalid=True)
            assert m > 0
            got = beliefs.follow(_one_hot(root), lab[None])
            assert np.array_equal(got[0], _one_hot(final)), (name, gi)


def test_follow_on_torch_tensors_equals_numpy():
    import torch
    rs = np.random.RandomState(6)
    n, cells = 5, 12
    origins = rs.randint(-2, cells + 2, size=(n, 2, cells)).astype(np.int16)
    for shape in ((2, 12, cells), (n, 2, 12, cells)):
        prior = rs.randint(0, 4096, size=shape).astype(np.int32)
        got = beliefs.follow(torch.from_numpy(prior), torch.from_numpy(origins))
        assert got.dtype == torch.int32 and np.array_equal(got.numpy(), beliefs.follow(prior, origins))


# ---- ABI (these fail on a library without the feature) ---------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    return _lib.load()


def test_the_library_exports_both_symbols(lib):
    assert 'sgx_set_replay_origins' in _lib.EXPORTED_SYMBOLS and 'sgx_replay_origins_set' in _lib.EXPORTED_SYMBOLS
    assert len(lib.sgx_set_replay_origins.argtypes) == 3 and len(lib.sgx_replay_origins_set.argtypes) == 1
    assert lib.sgx_replay_origins_set(None) == 0
    assert _lib.LAUNCH_REPLAY_TRACKED == 8 and _lib.ABI_VERSION == 15 and lib.sgx_abi_version() == 15


def test_the_setter_refuses_under_its_own_name(lib):
    assert lib.sgx_set_replay_origins(None, None, 4096) == SGX_EINVAL
    assert b'sgx_set_replay_origins' in lib.sgx_last_error() and b'NULL' in lib.sgx_last_error()
    for in_ptr, out_ptr, which in ((None, 4096 + 2, b'origin_out_dev'), (4096 + 1, 4096, b'origin_in_dev'), (4096 + 2, 8192, b'origin_in_dev')):
        assert lib.sgx_set_replay_origins(None, in_ptr, out_ptr) == SGX_EINVAL
        msg = lib.sgx_last_error()
        assert b'sgx_set_replay_origins' in msg and which in msg and b'4-byte aligned' in msg, msg


def test_the_headers_contract_names_both_pointers():
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    start = hdr.index('/* Alignment of device pointers.')
    contract = hdr[start:hdr.index('*/', start)]
    line = re.search(r'^ \*   sgx_set_replay_origins\s+(.*)$', contract, re.M)
    assert line and 'origin_in_dev' in line.group(1) and 'origin_out_dev' in line.group(1) and re.search(r'\b4\b', line.group(1))
    assert re.search(r'#define SGX_LAUNCH_REPLAY_TRACKED 8\b', hdr) and re.search(r'#define SGX_ABI_VERSION 15\b', hdr)
    # the setter is not on the header's list of entry points that wait for the device
    waits = hdr[hdr.index('the entry points that wait for the device are'):hdr.index('every other entry point returns once its work is enqueued')]
    assert 'sgx_set_replay_origins' not in waits
