"""sgx_step_vs without a GPU: the ABI pins and the host-side refusals that need no device, and the numpy restatement of the rule
(tests/step_vs_rule.py, what the device kernel is held to bit for bit in tests/test_gpu_step_vs.py) against the rule's own promises -- a
constant table draws the uniform k-th valid move, a weight of 0 is never taken next to a positive one, the bot never moves twice, a
finished root is a copy, a refused action leaves the position alone and the bot still, without actions only the bot's slots move -- and
against tests/replay_rule.py: replaying [agent action, reply] from the root gives the same final state."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib, playout_policies as pol
from stratego_env_amd.config import VARIANTS
from tests import replay_rule as rr, step_vs_rule as sv, weighted_playout_rule as wr
from tests.pool_roots import VALID, agent_actions, sampled_states
from tests.tables import third_zero_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAME_SETS = ['micro', 'tiny', 'fives']


def _over(name, st):
    v = VARIANTS[name]
    return orc.OracleRules(v.rows, v.columns).get_game_ended(np.asarray(st, dtype=np.int64), 1) != 0


def test_the_binding():
    assert 'sgx_step_vs' in _lib.EXPORTED_SYMBOLS
    assert _lib.LAUNCH_STEP_VS == 9 and _lib.VS_SEE_ALL == 1 and (_lib.VS_MOVED_AGENT, _lib.VS_MOVED_BOT) == (1, 2)
    assert (sv.MOVED_AGENT, sv.MOVED_BOT) == (1, 2)
    assert _lib.ABI_VERSION == 15                       # an addition within v15: no struct or signature of the existing ABI changed
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    assert re.search(r'#define SGX_LAUNCH_STEP_VS 9\b', hdr) and re.search(r'#define SGX_VS_SEE_ALL 1\b', hdr)
    assert re.search(r'#define SGX_VS_MOVED_AGENT 1\b', hdr) and re.search(r'#define SGX_VS_MOVED_BOT\s+2\b', hdr)
    assert re.search(r'#define SGX_ABI_VERSION 15\b', hdr)
    assert re.search(r'\bint sgx_step_vs\(sgx_env \*dst, sgx_env \*src, const int32_t \*src_index_dev, const sgx_vs_io \*io,', hdr)
    # STREAM_REPLY = 8, a stream of its own, in the device code and in the rule
    layout = open(os.path.join(ROOT, 'stratego_env_amd', 'csrc', 'sgx_layout.h')).read()
    assert re.search(r'STREAM_REPLY = 8\b', layout) and sv.STREAM_REPLY == 8
    streams = dict(re.findall(r'(STREAM_[A-Z0-9_]+) = (\d+)', re.search(r'enum \{ STREAM_SETUP[^}]*\}', layout).group(0)))
    assert len(set(streams.values())) == len(streams) == 9
    # sgx_vs_io: the header's members in the header's order are the ctypes struct's, 9 pointers + 2 int32 = 80 bytes
    body = re.search(r'typedef struct sgx_vs_io \{(.*?)\} sgx_vs_io;', hdr, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    members = []
    for decl in body.split(';'):
        names = re.findall(r'\*?\s*(\w+)\s*(?:,|$)', decl.strip())
        members += [n for n in names if n]
    assert members == [f[0] for f in _lib.SgxVsIO._fields_], members
    assert C.sizeof(_lib.SgxVsIO) == 80
    assert [f[1] for f in _lib.SgxVsIO._fields_] == [C.c_void_p] * 9 + [C.c_int32] * 2


def test_the_library_refuses_on_the_host():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_step_vs.argtypes) == 7
    p16 = lambda w: w.ctypes.data_as(C.POINTER(C.c_uint16))
    w = pol.uniform()
    io = _lib.SgxVsIO(None, None, None, None, None, None, None, None, None, 1, 0)
    # the table is looked at before the handles are (so no device is needed to get these refusals)
    assert L.sgx_step_vs(None, None, None, io, None, 0, None) == -1
    assert b'sgx_step_vs' in L.sgx_last_error() and b'weights is NULL' in L.sgx_last_error()
    bad = pol.uniform()
    bad[2, 7, 9] = 4096
    assert L.sgx_step_vs(None, None, None, io, p16(bad), 0, None) == -1
    assert b'sgx_step_vs: weights[2][7][9] = 4096' in L.sgx_last_error(), L.sgx_last_error()
    assert L.sgx_step_vs(None, None, None, io, p16(w), 0, None) == -1
    assert b'sgx_step_vs' in L.sgx_last_error() and b'NULL' in L.sgx_last_error()


@pytest.fixture(scope='module')
def stepped():
    """Every sampled root of every game set through the rule once, for both sides, with a seeded mix of agent actions and the random table:
    {name: [(root, mover, side, action, kind, result, trace)]}"""
    table = third_zero_table()
    out = {}
    for name in GAME_SETS:
        roots = sampled_states(name)
        states, players = [s for s, _ in roots], [p for _, p in roots]
        actions, kinds = agent_actions(name, states, players, seed=4)
        rows = []
        for si, (st, mover) in enumerate(roots):
            for side in (1, -1):
                trace = []
                res = sv.step_vs(name, st, mover, int(actions[si]), side, 0x5EED, si, 3, table, see_all=bool(si & 1), trace=trace)
                rows.append((st, mover, side, int(actions[si]), int(kinds[si]), res, trace))
        out[name] = rows
    return out


@pytest.mark.parametrize('name', GAME_SETS)
def test_the_promises_of_the_rule(name, stepped):
    seen = {'agent+bot': 0, 'bot only': 0, 'refused': 0, 'over': 0, 'ended by the agent': 0, 'weighted': 0}
    for st, mover, side, action, kind, res, trace in stepped[name]:
        final, player, reward, done, ending_invalid, invalid, moved, reply = res
        st = np.asarray(st, dtype=np.int64)
        turn0, turn1 = int(st[5, 0, 0]), int(final[5, 0, 0])
        if _over(name, st):                                                 # a finished root is a copy, whatever the action
            assert np.array_equal(final, st) and player == mover and done == 1 and (invalid, moved, reply) == (0, 0, -1)
            seen['over'] += 1
            continue
        if invalid:                                                         # a refused action: the position stays, the bot stays still
            assert mover == side and kind != VALID
            assert np.array_equal(final, st) and player == mover and (moved, reply, done) == (0, -1, 0)
            seen['refused'] += 1
            continue
        assert (mover == side) == bool(moved & sv.MOVED_AGENT)
        assert kind == VALID or mover != side                               # (where the bot is to move the action is not looked at)
        # never two bot moves: the turn counter advanced by one per mover that moved
        assert turn1 - turn0 == bin(moved).count('1') and len(trace) <= 1
        assert (reply >= 0) == bool(moved & sv.MOVED_BOT)
        if not done:
            assert player == side and (moved & sv.MOVED_BOT)                # the agent is to move again
        elif not (moved & sv.MOVED_BOT):
            seen['ended by the agent'] += 1
        for valid, w, k in trace:                                           # weight 0 is never taken while another move has weight
            assert valid[k] == reply
            assert w.sum() == 0 or w[k] > 0
            seen['weighted'] += int(w.sum() > 0)
        seen['agent+bot' if moved == 3 else 'bot only'] += int(moved >= 2)
    print(name, seen)
    assert seen['agent+bot'] and seen['bot only'] and seen['refused'] and seen['weighted']


@pytest.mark.parametrize('name', GAME_SETS)
@pytest.mark.parametrize('c', [1, 7, 4095])
def test_a_constant_table_draws_the_uniform_kth_move(name, c):
    table = np.full(wr.SHAPE, c, dtype=np.uint16)
    drawn = 0
    for si, (st, mover) in enumerate(sampled_states(name)):
        if _over(name, st):
            continue
        valid = sv.valid_actions(name, st, mover)
        r = orc.rng(9, 100 + si, 1 << 40, sv.STREAM_REPLY, int(np.asarray(st)[5, 0, 0]))
        want = int(valid[orc.rng_below(r, len(valid))])
        for see_all in (False, True):
            res = sv.step_vs(name, st, mover, None, -mover, 9, 100 + si, 1 << 40, table, see_all)
            assert res[7] == want and res[6] == sv.MOVED_BOT, (name, c, si)
            drawn += 1
    assert drawn > 0


@pytest.mark.parametrize('name', GAME_SETS)
def test_without_actions_only_the_bots_slots_move(name):
    roots = sampled_states(name)
    states, players = np.stack([np.asarray(s, dtype=np.int64) for s, _ in roots]), np.asarray([p for _, p in roots], dtype=np.int8)
    sides = np.where(np.arange(len(roots)) % 3 == 0, -1, 1).astype(np.int8)
    out, out_p, reward, done, ending_invalid, invalid, moved, reply = sv.step_vs_batch(name, states, players, None, sides, 2, 50, 7, third_zero_table(1))
    bots = 0
    for i in range(len(roots)):
        if players[i] != sides[i] and not _over(name, states[i]):
            assert moved[i] == sv.MOVED_BOT and reply[i] >= 0 and int(out[i][5, 0, 0]) == int(states[i][5, 0, 0]) + 1
            bots += 1
        else:
            assert moved[i] == 0 and reply[i] == -1 and np.array_equal(out[i], states[i]) and out_p[i] == players[i]
        assert invalid[i] == 0
    assert 0 < bots < len(roots)
    # the batch keys slot i with env_id_offset + i and reads root index[i]
    index = np.random.RandomState(1).randint(0, len(roots), size=9)
    got = sv.step_vs_batch(name, states, players, None, -1, 2, 50, 7, third_zero_table(1), index=index)
    for i, s in enumerate(index):
        one = sv.step_vs(name, states[s], int(players[s]), None, -1, 2, 50 + i, 7, third_zero_table(1))
        assert np.array_equal(got[0][i], one[0]) and got[7][i] == one[7] and got[6][i] == one[6]


@pytest.mark.parametrize('name', GAME_SETS)
def test_replaying_the_two_actions_gives_the_final_state(name, stepped):
    replayed = 0
    for st, mover, side, action, kind, res, trace in stepped[name]:
        final, player, reward, done, ending_invalid, invalid, moved, reply = res
        lst = ([action] if moved & sv.MOVED_AGENT else []) + ([reply] if moved & sv.MOVED_BOT else [])
        got = rr.replay(name, st, mover, lst)
        assert np.array_equal(got[0], final) and got[1] == player, (name, side, action)
        assert got[2].tobytes() == reward.tobytes() and got[3:5] == (done, ending_invalid)
        assert got[5] == got[6] == len(lst)                                # every entry was applied
        replayed += len(lst)
    assert replayed > 0


