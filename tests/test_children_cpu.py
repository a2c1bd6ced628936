"""Expand all (sgx_count_moves / sgx_expand_all) without a GPU: the numpy restatement of the rule (tests/children_rule.py, what
the device kernels are held to bit for bit in tests/test_gpu_children.py) against the reference's own masks along recorded games, the binding,
and the new kernels' resources read from the shipped library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from stratego_env_amd import _lib
from tests import children_rule as cr
from tests.helpers import load_expanded, oracle_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPANDED = ['barrage', 'octa_barrage', 'medium', 'fives', 'tiny', 'micro']


@pytest.mark.parametrize('name', EXPANDED)
def test_the_rule_against_the_golden_masks(name):
    """At every position of the recorded games: the rule's action list is flatnonzero of the reference's mask (empty where that is the no-op
    only), the child of the recorded action is the oracle's next position, and the last one is the recorded final state."""
    ex = load_expanded(name)
    n_games = len([k for k in ex if k.endswith('_actions')])
    env = oracle_env(name)
    noop = env.K - 1
    positions = empty = 0
    for gi in range(n_games):
        pre = 'g%d_' % gi
        masks, slot_player, actions = ex[pre + 'masks'], ex[pre + 'slot_player'], ex[pre + 'actions']
        env.reset(ex[pre + 'p1_map'].astype(np.int64), ex[pre + 'p2_map'].astype(np.int64))
        slot = 0                                           # the golden slot that holds the mover's mask at the current position
        for k in range(len(actions) + 1):
            where = (name, gi, k)
            assert slot_player[slot] == env.player, where
            golden = np.flatnonzero(masks[slot].reshape(-1))
            got = cr.moves(name, env.state, env.player)
            if golden.tolist() == [noop]:
                assert len(got) == 0, where
                empty += 1
            else:
                assert np.array_equal(got, golden), where
            positions += 1
            if k == len(actions):
                break
            a = int(actions[k])
            state, player = env.state.copy(), env.player
            obs, rew, done, info = env.step({env.player: a})
            if a in got.tolist():
                c_state, c_player, c_reward, c_done, c_ei = cr.child(name, state, player, a)
                assert np.array_equal(c_state, env.state) and c_player == env.player, where
                assert c_done == int(bool(done['__all__'])) == int(bool(ex[pre + 'dones'][k])), where
                if c_done:
                    assert tuple(c_reward) == tuple(np.float32(x) for x in ex[pre + 'rewards'][k]), where
                    assert c_ei == int(bool(info[1]['game_result_was_invalid'])), where
                else:
                    assert not c_reward.any() and c_ei == 0, where
                one_d = cr.action_1d(name, a, player)
                ns, npl = env.rules.get_next_state(state, player, one_d)
                assert np.array_equal(ns, env.state) and int(npl) == env.player, where
            else:
                assert a == noop and len(got) == 0, where         # (the no-op of a mover without a move: valid, but never a child)
            # the next mover's mask among the slots this step added
            slot = _mover_slot(ex[pre + 'slot_player'], ex[pre + 'dones'], k + 1, env.player)
        assert np.array_equal(env.state, ex[pre + 'final_state'].astype(np.int64)), (name, gi)
    assert positions > n_games
    ended = sum(int(bool(ex['g%d_dones' % gi][-1])) for gi in range(n_games))
    assert empty >= ended, "every recorded ending is a position without a child"


def test_a_finished_game_has_no_child():
    """the recorded final states of finished games (tests/golden/games_*.npz): no move, whoever is asked"""
    from tests.helpers import load_games
    seen = 0
    for name in ('micro', 'tiny'):
        g = load_games(name)
        for gi in np.flatnonzero(g['finished'])[:16]:
            final = g['final_states'][gi].astype(np.int64)
            for player in (1, -1):
                assert len(cr.moves(name, final, player)) == 0, (name, gi, player)
                assert len(cr.root_children(name, final, player)['action']) == 0
            seen += 1
    assert seen > 0


def _mover_slot(slot_player, dones, k, mover):
    """the golden slot of the mover's mask at the position after k steps: slot 0 is the initial position, every step adds one slot (the next
    mover's) or, when it ended the game, two (both players', +1 first)"""
    if k == 0:
        return 0
    base = 1 + sum(2 if dones[j] else 1 for j in range(k - 1))
    if not dones[k - 1]:
        return base
    return base if slot_player[base] == mover else base + 1


def test_the_binding():
    assert C.sizeof(_lib.SgxChildrenIO) == 88
    offsets = {name: getattr(_lib.SgxChildrenIO, name).offset for name, _ in _lib.SgxChildrenIO._fields_}
    assert offsets == {'offsets_dev': 0, 'parent_dev': 8, 'action_dev': 16, 'reward_dev': 24, 'done_dev': 32, 'ending_invalid_dev': 40,
                       'player_dev': 48, 'n_roots': 56, 'first_child': 64, 'n_children': 72, 'flags': 80, 'reserved': 84}
    # ... and the header's struct, member by member in the same order
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    body = re.search(r'typedef struct sgx_children_io \{(.*?)\} sgx_children_io;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    members = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            members += [m.strip().lstrip('*') for m in re.sub(r'^(const\s+)?\w+\s+', '', decl).split(',')]
    assert members == [name for name, _ in _lib.SgxChildrenIO._fields_]
    assert 'sgx_count_moves' in _lib.EXPORTED_SYMBOLS and 'sgx_expand_all' in _lib.EXPORTED_SYMBOLS
    assert _lib.CHILDREN_ACTIONS_1D == 1 and _lib.LAUNCH_CHILDREN == 6
    assert re.search(r'#define SGX_LAUNCH_CHILDREN 6\b', hdr) and re.search(r'#define SGX_CHILDREN_ACTIONS_1D 1\b', hdr)
    assert _lib.ABI_VERSION == 15                       # no struct or signature of the existing ABI changed


def test_the_library_exports_the_entry_points():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_count_moves.argtypes) == 6 and len(L.sgx_expand_all.argtypes) == 5
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message that names the call
    assert L.sgx_count_moves(None, None, 0, None, None, None) == -1
    assert b'sgx_count_moves' in L.sgx_last_error()
    assert L.sgx_expand_all(None, None, None, None, None) == -1
    assert b'sgx_expand_all' in L.sgx_last_error()


def test_the_new_kernels_use_no_scratch_memory(tmp_path):
    """count_kernel and children_kernel on every board of the reference, in every games-per-wave variant the library holds, and the three scan
    kernels: no scratch memory (read from the shipped library)."""
    from tests.step_checks import _kernel_resources
    res = _kernel_resources(tmp_path)
    boards = {(10, 10), (15, 15), (8, 8), (6, 6), (5, 5), (4, 4), (3, 4)}
    for kernel in ('12count_kernel', '15children_kernel'):
        seen = set()
        for name, r in res.items():
            m = re.search(kernel + r'ILi(\d+)ELi(\d+)ELi(\d+)E', name)
            if not m:
                continue
            assert r['scratch'] == 0, (name, r)
            seen.add((int(m.group(1)), int(m.group(2))))
        assert seen == boards, (kernel, seen)
    scans = [name for name in res if re.search(r'scan_(sums|bases|offsets)_kernel', name)]
    assert len(scans) == 3
    for name in scans:
        assert res[name]['scratch'] == 0, (name, res[name])
