"""sgx_step_vs / PackedStates.step_vs / VecStrategoEnv.step_vs / VsBotVecEnv on the GPU: records and all seven outputs bit for bit against the
numpy restatement of the rule on the oracle (tests/step_vs_rule.py, which tests/test_step_vs_cpu.py holds to the rule's promises) on boards
of four, two and one game per wave, a board with more channels than lanes and one with wide cells; a restatement-free check (T calls in
place, then sgx_replay of the logged actions reproduces the records); NULL outputs, a ragged batch and guard bands, the in-place call
against the two-handle call, the refusals (all host-side), a dst with a start pool, two tables on one stream; and the wrapper env.
The stream contract of sgx_step_vs is the row `step-vs` of the one table of stream cases (tests/stream_cases.py, run by
tests/test_gpu_streams.py).

Roots, N_SRC, KEYS and DRAWS are the weighted playout tests' (tests/pool_roots.py); a test restates at most two moves per slot."""
import itertools

import numpy as np
import pytest

from stratego_env_amd import playout_policies as pol
from tests import pool_roots as tp, step_vs_rule as sv, tables as tb
from tests.guard_bands import Arena, pool_output_sweep
from tests.pool_roots import STEP_VS_OUT_SPECS as OUT_SPECS, agent_actions

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1
N_SRC, KEYS, DRAWS, TABLES = tp.N_SRC, tp.KEYS, tp.DRAWS, tb.TABLES
OUTS = ('reward', 'done', 'ending_invalid', 'player', 'invalid_action', 'moved', 'reply_action')
# every value of every axis (table, view, agent) on each board; their whole cross product on the boards whose restatement is cheap
SMALL = ('micro', 'fives', 'medium', 'octa_barrage', 'barrage')


def _results(res):
    return {k: tp._np(getattr(res, k)) for k in OUTS}


def _sides(kind, n):
    """agent = +1, -1, or a mixed int8 [n]"""
    return kind if kind != 'mixed' else np.where(np.random.RandomState(8).randint(0, 2, size=n) == 0, -1, 1).astype(np.int8)


def _compare(variant, pool, res, states, players, actions, sides, seed, offset, draw, table, see_all, index, where):
    """the pool's records and the seven result tensors against the restatement; -> the restatement's (invalid, moved, done)"""
    want = dict(zip(('state', 'players') + OUTS[:3] + OUTS[4:], sv.step_vs_batch(variant, states, players, actions, sides, seed, offset, draw, table,
                                                                                 see_all, index)))
    want['player'] = want['players']
    got = _results(res)
    for k in OUTS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (where, k, got[k].tolist(), want[k].tolist())
    got_s, got_p = pool.unpack()
    assert np.array_equal(tp._np(got_s), want['state']), where
    assert np.array_equal(tp._np(got_p), want['players']), where
    return want['invalid_action'], want['moved'], want['done']


def _roots_with_finished(name):
    """tp._board_roots as a pool of N_SRC records; where the rollout left no finished game among them (the large boards), slots 0 .. 3 take the
    ends of uniform playouts of their own games.  -> (pool, states, players, finished)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    v = tp._board(name)
    env, states, players, finished = tp._board_roots(name, tp.WEIGHTED_CASES[name][0])
    pool = PackedStates(v, N_SRC)
    pool.copy_from(env)
    if not finished.any():
        ends = PackedStates(v, N_SRC, seed=1)
        res = ends.playout(env)
        assert bool(res.done[:4].all())
        four = torch.arange(4, dtype=torch.int32, device='cuda')
        pool.copy_from(ends, src_index=four, dst_index=four)
        ends.close()
        states_t, players_t = pool.unpack()
        states, players = tp._np(states_t), tp._np(players_t)
        finished = tp._np(pool._vec.env_info()[:, 2]) != 0
    env.close()
    return pool, states, players, finished


@pytest.mark.parametrize('name', ['micro', 'fives', 'medium', 'octa_barrage', 'barrage', 'standard2', 'c3x40', 'c32x32'])
def test_bit_exact_against_the_restatement(name):
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    v = tp._board(name)
    env, states, players, finished = _roots_with_finished(name)
    assert finished.any() and not finished.all(), "both finished and unfinished roots"
    before_t = env.unpack()
    n = 61
    shared = int(np.flatnonzero(~finished)[0])
    idx = np.random.RandomState(5).randint(0, N_SRC, size=n).astype(np.int32)
    idx[:20] = shared                                                      # 20 slots of one root: wave-mates that take different ways
    idx_t = torch.from_numpy(idx).cuda()
    acts = {'gathered': agent_actions(v, states, players, idx, seed=1)[0], 'identity': agent_actions(v, states, players, None, seed=2)[0]}
    combos = list(itertools.product(TABLES, (False, True), (1, -1, 'mixed')))
    if name not in SMALL:
        combos = [(t, bool(j & 1), (1, -1, 'mixed')[j % 3]) for j, t in enumerate(list(TABLES) * 2)]
    seen = {'refused': 0, 'over': 0, 'bot only': 0, 'agent and bot': 0, 'agent only': 0}
    ways_of_the_shared_root = set()
    pools = {}
    for j, (tname, see_all, agent) in enumerate(combos):
        seed, offset = KEYS[j % len(KEYS)]
        draw = DRAWS[j % len(DRAWS)]
        for kind, pool_n, index, index_t in (('gathered', n, idx, idx_t), ('identity', N_SRC, None, None)):
            if (kind, seed) not in pools:
                pools[kind, seed] = PackedStates(v, pool_n, seed=seed, env_id_offset=offset)
            pool = pools[kind, seed]
            sides = _sides(agent, pool_n)
            agent_arg = agent if agent != 'mixed' else torch.from_numpy(sides).cuda()
            res = pool.step_vs(env, torch.from_numpy(acts[kind]).cuda(), agent_arg, TABLES[tname], see_all=see_all, draw=draw, src_index=index_t)
            assert pool.last_launch_kind == _lib.LAUNCH_STEP_VS == 9
            where = (name, seed, tname, see_all, agent, draw, kind)
            invalid, moved, done = _compare(v, pool, res, states, players, acts[kind], sides, seed, offset, draw, TABLES[tname], see_all, index, where)
            root_over = finished[index] if index is not None else finished
            seen['refused'] += int(invalid.sum())
            seen['over'] += int(root_over.sum())
            seen['bot only'] += int((moved == sv.MOVED_BOT).sum())
            seen['agent and bot'] += int((moved == 3).sum())
            seen['agent only'] += int((moved == sv.MOVED_AGENT).sum())
            # every slot that is not over and was not refused has its agent to move
            live = (done == 0) & (invalid == 0)
            assert np.array_equal(tp._np(res.player)[live], np.broadcast_to(sides, (pool_n,))[live]), where
            if index is not None:
                ways_of_the_shared_root |= set(zip(invalid[:20].tolist(), moved[:20].tolist()))
    for pool in pools.values():
        pool.close()
    after_t = env.unpack()
    assert torch.equal(after_t[0], before_t[0]) and torch.equal(after_t[1], before_t[1])           # src untouched
    print(name, seen, 'ways of the shared root', sorted(ways_of_the_shared_root))
    assert seen['refused'] and seen['over'] and seen['bot only'] and seen['agent and bot']
    assert len(ways_of_the_shared_root) >= 3, "wave-mates on one root: refused, agent and bot, bot only"
    env.close()


@pytest.mark.parametrize('name,T', [('barrage', 12), ('micro', 6)])
def test_in_place_calls_replay_to_the_same_records(name, T):
    """No restatement: T in-place calls on a live env without restarts, then sgx_replay of the interleaved logged (agent, reply) actions
    from the snapshot reproduces the records."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    n = 96
    env = VecStrategoEnv(name, n, seed=21, env_id_offset=300, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(3, emit_obs=False, emit_mask=False)                  # (movers of both colours among the roots)
    snap = env.snapshot()
    sides = torch.from_numpy(_sides('mixed', n)).cuda()
    table = TABLES['random']
    log = torch.full((n, 2 * T), -1, dtype=torch.int32, device='cuda')
    length = torch.zeros((n,), dtype=torch.int64, device='cuda')
    rows = torch.arange(n, device='cuda')
    refused = replies = 0
    for t in range(T):
        env.observe(emit_obs=False)
        actions = env.sample_valid_actions().clone()
        actions[t % 7::7] = -1 - t                                         # some refused actions in every call
        res = env.step_vs(actions, sides, table, see_all=bool(t & 1), draw=t)
        for bit, values in ((sv.MOVED_AGENT, actions), (sv.MOVED_BOT, res.reply_action)):
            took = (res.moved & bit) != 0
            log[rows[took], length[took]] = values[took]
            length += took
        live = (res.done == 0) & (res.invalid_action == 0)
        assert torch.equal(res.player[live], sides[live]), (name, t)
        assert bool((res.moved[res.invalid_action != 0] == 0).all())
        refused += int(res.invalid_action.sum())
        replies += int(((res.moved & sv.MOVED_BOT) != 0).sum())
    assert refused > 0 and replies > n
    pool = PackedStates(name, n)
    rep = pool.replay(snap, log, lengths=length.to(torch.int32))
    assert torch.equal(rep.applied.long(), length) and int(rep.stop.max()) <= 1
    for got, want in zip(pool.unpack(), env.export_state()):
        assert torch.equal(got, want)
    assert torch.equal(pool._vec.env_info()[:, [0, 2, 3]], env.env_info()[:, [0, 2, 3]])
    for x in (pool, snap, env):
        x.close()


def _vs_io(_lib, ptrs, actions, agent_dev, agent=1, flags=0):
    return _lib.SgxVsIO(actions, agent_dev, ptrs['reward'], ptrs['done'], ptrs['ending_invalid'], ptrs['player'], ptrs['invalid_action'],
                        ptrs['moved'], ptrs['reply_action'], agent, flags)


def test_null_outputs_a_ragged_batch_and_guard_bands():
    """n = 37 is no multiple of the 16 games of a Fives workgroup.  (The records are the library's own allocation: they are compared with
    the restatement's, like every pool-to-pool test does.)"""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'fives', 37
    env, states, players, finished = tp._board_roots(name, tp.WEIGHTED_CASES[name][0], n=n)
    pool = PackedStates(name, n, seed=2, env_id_offset=7)
    vec = pool._vec
    L = vec._L
    table = TABLES['random']
    actions = agent_actions(name, states, players, None, seed=3)[0]
    sides = _sides('mixed', n)
    want = dict(zip(('state', 'player') + OUTS[:3] + OUTS[4:], sv.step_vs_batch(name, states, players, actions, sides, 2, 7, 5, table, True)))

    def guarded_inputs(byte_phase, word_phase):
        ins = {'actions': Arena('actions', (n,), torch.int32, word_phase, vec.device), 'agent': Arena('agent', (n,), torch.int8, byte_phase, vec.device)}
        ins['actions'].t.copy_(torch.from_numpy(actions))
        ins['agent'].t.copy_(torch.from_numpy(sides))
        return ins

    def call(ptrs, ins):
        io = _vs_io(_lib, ptrs, ins['actions'].t.data_ptr(), ins['agent'].t.data_ptr(), 0, _lib.VS_SEE_ALL)
        return L.sgx_step_vs(vec._h, env._h, None, io, tb._p16(table), 5, vec._stream())

    def after_call(ins, skip):
        if skip is None:
            for a in ins.values():
                a.check_guards('sgx_step_vs')
            assert np.array_equal(ins['actions'].host(), actions) and np.array_equal(ins['agent'].host(), sides)       # inputs only read
        assert np.array_equal(tp._np(pool.unpack()[0]), want['state'])

    pool_output_sweep(OUT_SPECS, vec.device, guarded_inputs, call, want, 'sgx_step_vs', after_call)
    pool.close(); env.close()


def test_in_place_equals_the_two_handle_call_and_null_actions():
    import torch
    name, n = 'barrage', 40
    env, states, players, finished = tp._board_roots(name, 200, n=n)
    twin = tp._pool_from(env, name, n)
    dst = tp._pool_from(None, name, n)
    actions = torch.from_numpy(agent_actions(name, states, players, None, seed=6)[0]).cuda()
    table = pol.capture_biased(name)
    for acts, agent in ((actions, 1), (actions, -1), (None, 1), (None, -1)):
        a = dst.step_vs(twin, acts, agent, table, draw=4)                  # pool to pool
        b = twin.step_vs(twin, acts, agent, table, draw=4)                 # in place: the live-env call
        for k in OUTS:
            assert torch.equal(getattr(a, k), getattr(b, k)), (k, agent)
        for x, y in zip(dst.unpack(), twin.unpack()):
            assert torch.equal(x, y)
        if acts is None:                                                   # the bot opens where it is its turn, every other slot is a copy
            assert not bool((a.moved & sv.MOVED_AGENT).any()) and not bool(a.invalid_action.any())
    with pytest.raises(ValueError):
        twin.step_vs(twin, actions, 1, table, src_index=torch.zeros(n, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        twin.step_vs(twin, actions, 0, table)
    for x in (twin, dst, env):
        x.close()


def test_refusals_are_host_side_and_a_start_pool_is_accepted():
    """Every refusal is SGX_EINVAL with its message under this function's name; dst, src and the poisoned outputs keep what they held.  A dst
    with a start pool is accepted, plays what a dst without one plays, and its pool draws do not move."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'barrage', 16
    env, states, players, _ = tp._board_roots(name, 30, n=n)
    a, b = tp._pool_from(env, name, n), tp._pool_from(env, name, n)
    foreign, small = PackedStates('standard', n), PackedStates(name, n // 2)
    L = a._vec._L
    stream = a._vec._stream()
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    outs = {k: torch.full((n, w) if w > 1 else (n,), 77, dtype=getattr(torch, t), device='cuda') for k, w, t in OUT_SPECS}
    actions = torch.from_numpy(agent_actions(name, states, players, None, seed=9)[0]).cuda()
    actions2 = torch.cat([actions, actions])
    good = pol.capture_biased(name)

    def io(agent=1, flags=0, agent_dev=None, actions_off=0, offs=()):
        ptrs = {k: t.data_ptr() + (dict(offs).get(k, 0)) for k, t in outs.items()}
        return _vs_io(_lib, ptrs, actions2.data_ptr() + actions_off, agent_dev, agent, flags)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in ('sgx_step_vs',) + words), msg

    def call(dst, src, index, io_, table=good):
        return L.sgx_step_vs(dst, src, index, io_, None if table is None else tb._p16(table), 0, stream)

    ah, bh = a._vec._h, b._vec._h
    refused(call(ah, foreign._vec._h, None, io()), 'different variants')
    refused(call(ah, ah, idx.data_ptr(), io()), 'race')
    refused(call(ah, small._vec._h, None, io()), 'at least as many envs')
    for agent in (0, 2, -2):
        refused(call(ah, bh, None, io(agent=agent)), 'agent')
    for flags in (2, 3, 1 << 20, -1):
        refused(call(ah, bh, None, io(flags=flags)), 'flags')
    refused(call(ah, bh, idx.data_ptr() + 2, io()), 'src_index_dev', '4-byte aligned')
    refused(call(ah, bh, None, io(actions_off=2)), 'actions_dev', '4-byte aligned')
    refused(call(ah, bh, None, io(offs=(('reward', 2),))), 'reward_dev', '4-byte aligned')
    refused(call(ah, bh, None, io(offs=(('reply_action', 1),))), 'reply_action_dev', '4-byte aligned')
    refused(call(None, bh, None, io()), 'NULL')
    refused(call(ah, bh, None, None), 'NULL')
    refused(call(ah, bh, None, io(), table=None), 'weights is NULL')
    bad = good.copy()
    bad[1, 10, 13] = 4096
    refused(call(ah, bh, None, io(), table=bad), 'weights[1][10][13] = 4096')
    with pytest.raises(ValueError):
        a.step_vs(b, actions, 1, bad)
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 77).all()), k                                    # nothing ran
    for pool in (a, b):
        got_s, got_p = pool.unpack()
        assert np.array_equal(tp._np(got_s), states) and np.array_equal(tp._np(got_p), players)
    # an agent outside {+1, -1} is not looked at when agent_dev is given; a dst with a start pool is accepted
    sides = torch.from_numpy(_sides('mixed', n)).cuda()
    plain = a.step_vs(b, actions, sides, good, draw=3)
    plain_s = [t.clone() for t in a.unpack()]
    fresh = tp._pool_from(None, name, n)
    a.copy_from(b)
    assert L.sgx_set_start_pool(ah, fresh._vec._h, n, 0) == 0, L.sgx_last_error()
    start_index = torch.full((n,), -5, dtype=torch.int32, device='cuda')
    assert L.sgx_set_start_index_out(ah, start_index.data_ptr()) == 0
    assert call(ah, bh, None, io(agent=0, agent_dev=sides.data_ptr())) == 0, L.sgx_last_error()
    res = a.step_vs(b, actions, sides, good, draw=3)
    for k in OUTS:
        assert torch.equal(getattr(res, k), getattr(plain, k)), k
    for x, y in zip(a.unpack(), plain_s):
        assert torch.equal(x, y)
    assert bool((start_index == -5).all()), "the call writes no start index"
    assert torch.equal(a._vec.env_info()[:, 1], b._vec.env_info()[:, 1]), "no game was restarted: the game numbers, and so the pool draws, are unmoved"
    assert L.sgx_set_start_index_out(ah, None) == 0 and L.sgx_set_start_pool(ah, None, 0, 0) == 0
    for x in (a, b, foreign, small, fresh, env):
        x.close()


def test_two_tables_on_one_stream():
    """The table is read before the call returns: the host overwrites the first call's table before the second call, nothing is
    synchronised in between, and each pool holds the positions of its own table."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates, StepVsResult
    name, n = 'fives', N_SRC
    env, states, players, finished = tp._board_roots(name, tp.WEIGHTED_CASES[name][0])
    first, second = PackedStates(name, n, seed=4, env_id_offset=9), PackedStates(name, n, seed=4, env_id_offset=9)
    L = first._vec._L
    res = [StepVsResult.empty(n, 'cuda') for _ in range(2)]
    actions = torch.from_numpy(agent_actions(name, states, players, None, seed=5)[0]).cuda()
    ios = [_vs_io(_lib, {k: getattr(r, k).data_ptr() for k in OUTS}, actions.data_ptr(), None, -1, 0) for r in res]
    buf = TABLES['attacks'].copy()
    stream = first._vec._stream()
    assert second._vec._stream().value == stream.value                     # one stream for both calls
    assert L.sgx_step_vs(first._vec._h, env._h, None, ios[0], tb._p16(buf), 6, stream) == 0, L.sgx_last_error()
    buf[:] = TABLES['forward']                                             # the first call's table is gone
    assert L.sgx_step_vs(second._vec._h, env._h, None, ios[1], tb._p16(buf), 6, stream) == 0, L.sgx_last_error()
    buf[:] = 0
    torch.cuda.synchronize()
    acts = tp._np(actions)
    _compare(name, first, res[0], states, players, acts, -1, 4, 9, 6, TABLES['attacks'], False, None, 'first')
    _compare(name, second, res[1], states, players, acts, -1, 4, 9, 6, TABLES['forward'], False, None, 'second')
    assert not torch.equal(res[0].reply_action, res[1].reply_action), "the two tables reply differently"
    first.close(); second.close(); env.close()


def _follow(vs, variant, g, seed, steps_log):
    """env g of a VsBotVecEnv run through the oracle with step_vs_rule, move for move; steps_log: per step (state before, mover, action,
    side, draw, state after the move call, done of that step)."""
    for st, mover, action, side, draw, after, done, reply in steps_log:
        got = sv.step_vs(variant, st, mover, action, side, seed, g, draw, vs.weights, vs.see_all)
        assert np.array_equal(got[0], after) and got[3] == done and got[7] == reply, g


@pytest.mark.parametrize('name,n,steps', [('micro', 256, 40), ('barrage', 64, 10)])
def test_the_wrapper_env(name, n, steps):
    import torch
    from stratego_env_amd.vs_env import VsBotVecEnv
    seed, follow = 0xBEEF, 5

    def run(record):
        vs = VsBotVecEnv(name, n, agent='random', seed=seed, human_inits=False, placement='plain', env_id_offset=40)
        env = vs.env
        obs, mask = vs.reset()
        trace, steps_log = [], []
        games = env.env_info()[:, 1].clone()
        finished = 0
        assert bool((env.player == vs.agent)[env.env_info()[:, 2] == 0].all())
        for t in range(steps):
            actions = env.sample_valid_actions().clone()
            if t % 5 == 4:
                actions[::9] = -3                                          # refused where the game is running
            sides_before = vs.agent.clone()
            if record:
                st, pl = env.export_state()
                before = (tp._np(st[follow]), int(pl[follow]), int(actions[follow]), int(sides_before[follow]), vs._draw)
                twin = env.snapshot()
                moved = twin.step_vs(actions, sides_before, vs.weights, see_all=vs.see_all, draw=vs._draw)
                steps_log.append(before + (tp._np(twin.export_state()[0][follow]), int(moved.done[follow]), int(moved.reply_action[follow])))
                twin.close()
            obs, mask, reward, done, info = vs.step(actions)
            # obs and mask are observe() of the records; every running game has its agent to move
            obs2, mask2 = obs.clone(), mask.clone()
            env.observe()
            assert torch.equal(env.obs, obs2) and torch.equal(env.mask, mask2)
            info_t = env.env_info()
            running = info_t[:, 2] == 0
            assert torch.equal(env.player[running], vs.agent[running])
            # reward is the agent's column (of the side it had in the game that ended)
            raw = vs._res.reward
            assert torch.equal(reward, torch.where(sides_before > 0, raw[:, 0], raw[:, 1]))
            assert bool((reward[done == 0] == 0).all())
            # a restarted env has a new game number, and stands at turn 1 where the bot opened it
            restarted = done != 0
            assert torch.equal(info_t[:, 1], games + restarted.to(games.dtype))
            opened = restarted & (vs._open.moved != 0)
            assert bool((info_t[opened, 0] == 1).all()) and bool((info_t[restarted & ~opened, 0] == 0).all())
            assert bool((vs._open.moved[~restarted] == 0).all()), "the opening call moves fresh games only"
            games = info_t[:, 1].clone()
            finished += int(restarted.sum())
            trace.append((actions.clone(), reward.clone(), done.clone(), info['reply_action'].clone(), info['invalid_action'].clone(), vs.agent.clone()))
        final = [t.clone() for t in env.export_state()]
        if record:
            _follow(vs, name, 40 + follow, seed, steps_log)
        vs.close()
        return trace, final, finished

    a, fa, finished = run(True)
    b, fb, _ = run(False)
    for x, y in zip(a, b):                                                 # two runs with the same seed are identical
        assert all(torch.equal(p, q) for p, q in zip(x, y))
    assert all(torch.equal(p, q) for p, q in zip(fa, fb))
    assert sum(int(x[4].sum()) for x in a) > 0
    if name == 'micro':
        assert finished > n, "many restarts"


def test_the_example_counts_add_up():
    from stratego_env_amd.examples.vs_bot_eval import evaluate
    for kind in ('uniform', 'policy'):
        r = evaluate('micro', 128, 30, kind, side='random', seed=3)
        assert r['finished'] > 0 and r['wins'] + r['losses'] + r['ties'] == r['finished'], r
        assert r['invalid'] == 0, r
