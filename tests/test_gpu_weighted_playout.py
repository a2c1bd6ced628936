"""sgx_playout_weighted / PackedStates.playout(weights=...) on the GPU: a constant table plays sgx_playout's games byte for byte; seeded random,
attacks-only and forward-only tables reproduce the numpy restatement of the rule on the oracle (tests/weighted_playout_rule.py, which
tests/test_weighted_playout_cpu.py holds to the rule's promises) bit for bit in both views, on boards of four, two and one game per wave, a
board with more channels than lanes and one with wide cells; ragged batches, the in-place call and the int64 API, NULL outputs and guard
bands, the refusals (all host-side, before any launch), two tables on one stream, and the PIMC example with a biased policy.

Roots are taken as tests/test_gpu_playout.py takes them (tests/pool_roots.py: rollouts without auto-reset, its rollout lengths); the caps
keep the restated moves of a test under about 60,000."""
import numpy as np
import pytest

from stratego_env_amd import playout_policies as pol
from tests import pool_roots as tp, weighted_playout_rule as wr
from tests.guard_bands import pool_output_sweep
from tests.boards import _board
from tests.pool_roots import N_SRC, WEIGHTED_CASES, _board_roots, _sample_states
from tests.tables import TABLES, _p16

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1


def _compare(variant, pool, res, states, players, seed, offset, draw, table, see_all, index, max_steps, where):
    """the pool's final states and the five result tensors against the restatement; -> (lengths, W == 0 positions, W > 0 positions)"""
    want_s, want_p, want_r, want_d, want_e, want_l, n_zero, n_pos = wr.playout_batch(variant, states, players, seed, offset, draw, table, see_all,
                                                                                      index, max_steps)
    got = tp._playout_results(res)
    print(where, 'lengths', want_l.tolist())
    assert np.array_equal(got['length'], want_l), where
    assert got['reward'].tobytes() == want_r.tobytes(), where
    assert np.array_equal(got['done'], want_d) and np.array_equal(got['ending_invalid'], want_e), where
    assert np.array_equal(got['player'], want_p), where
    got_s, got_p = pool.unpack()
    assert np.array_equal(tp._np(got_s), want_s), where
    assert np.array_equal(tp._np(got_p), want_p), where
    return want_l, int(n_zero.sum()), int(n_pos.sum())


@pytest.mark.parametrize('name', ['micro', 'fives', 'medium', 'barrage', 'standard2', 'c3x40', 'c20x20', 'c32x32'])
def test_a_constant_table_plays_the_games_of_sgx_playout(name):
    """the same pool key and draw: records and all five results byte for byte, no restatement needed"""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    v = _board(name)
    env, states, players, finished = _board_roots(name, WEIGHTED_CASES[name][0])
    assert not finished.all()
    n = 61
    idx_t = torch.from_numpy(np.random.RandomState(5).randint(0, N_SRC, size=n).astype(np.int32)).cuda()
    played = 0
    for seed, offset in tp.KEYS:
        for pool_n, index_t in ((n, idx_t), (N_SRC, None)):
            plain = PackedStates(v, pool_n, seed=seed, env_id_offset=offset)
            weighted = PackedStates(v, pool_n, seed=seed, env_id_offset=offset)
            for draw, c, see_all, max_steps in ((0, 1, False, 0), (1, 7, True, 0), (1 << 40, 4095, False, 9)):
                want = plain.playout(env, src_index=index_t, max_steps=max_steps, draw=draw)
                assert plain.last_launch_kind == _lib.LAUNCH_PLAYOUT
                got = weighted.playout(env, src_index=index_t, max_steps=max_steps, draw=draw, weights=np.full(wr.SHAPE, c), see_all=see_all)
                assert weighted.last_launch_kind == _lib.LAUNCH_PLAYOUT_WEIGHTED
                where = (name, seed, draw, c, see_all, max_steps)
                for k, t in tp._playout_results(want).items():
                    assert tp._playout_results(got)[k].tobytes() == t.tobytes(), (where, k)
                ws, wp = weighted.unpack()
                ps, pp = plain.unpack()
                assert torch.equal(ws, ps) and torch.equal(wp, pp), where
                played += int(want.length.sum())
            plain.close(); weighted.close()
    assert played > 0
    env.close()


@pytest.mark.parametrize('name', ['micro', 'fives', 'medium', 'octa_barrage', 'barrage', 'standard2', 'c3x40'])
def test_bit_exact_against_the_restatement(name):
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    v = _board(name)
    steps, caps = WEIGHTED_CASES[name]
    env, states, players, finished = _board_roots(name, steps)
    assert not finished.all()
    before_t = env.export_state()
    n = 61
    shared = int(np.flatnonzero(~finished)[0])
    idx = np.random.RandomState(5).randint(0, N_SRC, size=n).astype(np.int32)
    idx[:20] = shared
    idx_t = torch.from_numpy(idx).cuda()
    moves, zero, pos, wave_mates_differ = 0, 0, 0, False
    for seed, offset in tp.KEYS:
        gathered = PackedStates(v, n, seed=seed, env_id_offset=offset)
        identity = PackedStates(v, N_SRC, seed=seed, env_id_offset=offset)
        for tname, table in TABLES.items():
            for see_all in (False, True):
                for draw, max_steps in zip(tp.DRAWS, caps):
                    for pool, index, index_t in ((gathered, idx, idx_t), (identity, None, None)):
                        res = pool.playout(env, src_index=index_t, max_steps=max_steps, draw=draw, weights=table, see_all=see_all)
                        assert pool.last_launch_kind == _lib.LAUNCH_PLAYOUT_WEIGHTED
                        where = (name, seed, tname, see_all, max_steps, draw, 'gathered' if index is not None else 'identity')
                        lengths, z, p = _compare(v, pool, res, states, players, seed, offset, draw, table, see_all, index, max_steps, where)
                        moves, zero, pos = moves + int(lengths.sum()), zero + z, pos + p
                        if index is None:
                            wave_mates_differ |= bool((lengths[0::2] != lengths[1::2]).any())
        gathered.close(); identity.close()
    after_t = env.export_state()
    assert torch.equal(after_t[0], before_t[0]) and torch.equal(after_t[1], before_t[1])           # src untouched
    print(name, 'restated moves', moves, 'positions with W == 0', zero, 'with W > 0', pos)
    assert zero > 0 and pos > 0, "both the uniform fall-back (W == 0) and the weighted draw (W > 0) were played"
    assert wave_mates_differ, "two games that share a wave (slots 2j, 2j + 1) ended at different lengths"
    assert moves < 60000
    env.close()


@pytest.mark.parametrize('name', ['fives', 'medium'])
def test_ragged_batches(name):
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    env, states, players, finished = _board_roots(name, WEIGHTED_CASES[name][0])
    wg = tp.GAMES_PER_WORKGROUP[name]
    rs = np.random.RandomState(3)
    table = TABLES['random']
    for n in (1, wg - 1, wg, wg + 1, 251):
        idx = rs.randint(0, N_SRC, size=n).astype(np.int32)
        pool = PackedStates(name, n, seed=11, env_id_offset=5)
        res = pool.playout(env, src_index=torch.from_numpy(idx).cuda(), max_steps=12, draw=n, weights=table, see_all=bool(n & 1))
        _compare(name, pool, res, states, players, 11, 5, n, table, bool(n & 1), idx, 12, (name, n))
        pool.close()
    env.close()


def test_in_place_and_the_int64_api():
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    table = TABLES['forward']
    for name, max_steps, see_all in (('fives', 0, True), ('barrage', 9, False)):
        n = 40
        states, players = _sample_states(name, n, np.random.RandomState(13))           # along golden games, terminal states included
        pe = BatchedStrategoProceduralEnv(name, n)
        src = pe.pack(states, players)
        assert int(src.sanitised.sum()) == 0
        dst = pe.new_packed(n)
        res = dst.playout(src, max_steps=max_steps, draw=3, weights=table, see_all=see_all)                # pool to pool
        want_l, _, _ = _compare(name, dst, res, states, players, 0, 0, 3, table, see_all, None, max_steps, (name, 'pool to pool'))
        assert (want_l == 0).any() and (want_l > 0).any()
        pool_s, pool_r = tp._np(dst.unpack()[0]), tp._playout_results(res)
        res2 = src.playout(src, max_steps=max_steps, draw=3, weights=table, see_all=see_all)               # in place
        assert np.array_equal(tp._np(src.unpack()[0]), pool_s)
        for k, val in tp._playout_results(res2).items():
            assert val.tobytes() == pool_r[k].tobytes(), (name, k)
        with pytest.raises(ValueError):
            src.playout(src, src_index=torch.zeros(n, dtype=torch.int32, device='cuda'), weights=table)
        with pytest.raises(ValueError):
            dst.playout(src, weights=np.full(wr.SHAPE, 4096))
        # int64 in, int64 out; a CPU tensor as the table
        res3, final, final_players = pe.playout(states, players, max_steps=max_steps, draw=3, return_states=True,
                                                weights=torch.from_numpy(table.astype(np.int32)), see_all=see_all)
        for k, val in tp._playout_results(res3).items():
            assert val.tobytes() == pool_r[k].tobytes(), (name, k)
        assert final.dtype == torch.int64 and np.array_equal(tp._np(final), pool_s)
        assert np.array_equal(tp._np(final_players), pool_r['player'])
        for x in (src, dst, pe):
            x.close()


def test_null_outputs_and_guard_bands():
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'fives', 37
    env, states, players, finished = _board_roots(name, WEIGHTED_CASES[name][0], n=n)
    pool = PackedStates(name, n, seed=2, env_id_offset=7)
    vec = pool._vec
    L = vec._L
    table = TABLES['random']
    want = dict(zip(('state', 'player', 'reward', 'done', 'ending_invalid', 'length'), wr.playout_batch(name, states, players, 2, 7, 5, table, True)))

    def call(ptrs, ins):
        io = _lib.SgxPlayoutIO(ptrs['reward'], ptrs['done'], ptrs['ending_invalid'], ptrs['player'], ptrs['length'], 0, 0)
        return L.sgx_playout_weighted(vec._h, env._h, None, io, _p16(table), _lib.PLAYOUT_SEE_ALL, 5, vec._stream())

    def after_call(ins, skip):
        if skip is None:
            assert np.array_equal(tp._np(pool.unpack()[0]), want['state'])

    pool_output_sweep(tp.PLAYOUT_OUT_SPECS, vec.device, lambda byte_phase, word_phase: {}, call, want, 'sgx_playout_weighted', after_call)
    pool.close(); env.close()


def test_refusals_are_host_side():
    """Every refusal is SGX_EINVAL with its message under this function's name; dst, src and the outputs keep what they held."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'barrage', 16
    env, states, players, _ = _board_roots(name, 30, n=n)
    a, b = tp._pool_from(env, name, n), tp._pool_from(env, name, n)
    foreign = PackedStates('standard', n)
    small = PackedStates(name, n // 2)
    L = a._vec._L
    stream = a._vec._stream()
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    outs = {k: torch.full((n, w) if w > 1 else (n,), 77, dtype=getattr(torch, t), device='cuda') for k, w, t in tp.PLAYOUT_OUT_SPECS}
    good = pol.capture_biased(name)

    def io(max_steps=0, flags=0, reward_off=0, length_off=0):
        return _lib.SgxPlayoutIO(outs['reward'].data_ptr() + reward_off, outs['done'].data_ptr(), outs['ending_invalid'].data_ptr(),
                                 outs['player'].data_ptr(), outs['length'].data_ptr() + length_off, max_steps, flags)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in ('sgx_playout_weighted',) + words), msg

    def call(dst, src, index, io_, table=good, policy=0):
        return L.sgx_playout_weighted(dst, src, index, io_, None if table is None else _p16(table), policy, 0, stream)

    ah, bh = a._vec._h, b._vec._h
    refused(call(ah, foreign._vec._h, None, io()), 'different variants')
    refused(call(ah, ah, idx.data_ptr(), io()), 'race')
    refused(call(ah, small._vec._h, None, io()), 'at least as many envs')
    refused(call(ah, bh, None, io(max_steps=-1)), 'max_steps')
    for flags in (1, 2, -1):
        refused(call(ah, bh, None, io(flags=flags)), 'flags')
    refused(call(ah, bh, idx.data_ptr() + 2, io()), 'src_index_dev', '4-byte aligned')
    refused(call(ah, bh, None, io(reward_off=2)), 'reward_dev', '4-byte aligned')
    refused(call(ah, bh, None, io(length_off=1)), 'length_dev', '4-byte aligned')
    refused(call(None, bh, None, io()), 'NULL')
    refused(call(ah, bh, None, None), 'NULL')
    refused(call(ah, bh, None, io(), table=None), 'weights is NULL')
    bad = good.copy()
    bad[1, 10, 13] = 4096
    refused(call(ah, bh, None, io(), table=bad), 'weights[1][10][13] = 4096')
    for policy in (2, 3, 1 << 20, -1):
        refused(call(ah, bh, None, io(), policy=policy), 'policy_flags')
    with pytest.raises(ValueError):
        a.playout(b, weights=bad)
    fresh = tp._pool_from(None, name, n)
    assert L.sgx_set_start_pool(ah, fresh._vec._h, n, 0) == 0, L.sgx_last_error()
    refused(call(ah, bh, None, io()), 'start pool')
    assert L.sgx_set_start_pool(ah, None, 0, 0) == 0
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 77).all()), k                                    # nothing ran
    for pool in (a, b):
        got_s, got_p = pool.unpack()
        assert np.array_equal(tp._np(got_s), states) and np.array_equal(tp._np(got_p), players)
    # ... and the same call without a fault goes through
    assert call(ah, bh, None, io(max_steps=2), policy=_lib.PLAYOUT_SEE_ALL) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    assert not bool((outs['length'] == 77).any())
    for x in (a, b, foreign, small, fresh, env):
        x.close()


def test_two_tables_on_one_stream():
    """The table is read before the call returns: the host overwrites the first call's table before the second call, nothing is
    synchronised in between, and each pool holds the games of its own table."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'fives', N_SRC
    env, states, players, finished = _board_roots(name, WEIGHTED_CASES[name][0])
    first, second = PackedStates(name, n, seed=4, env_id_offset=9), PackedStates(name, n, seed=4, env_id_offset=9)
    L = first._vec._L
    res = [[torch.empty((n, 2), dtype=torch.float32, device='cuda'), torch.empty((n,), dtype=torch.uint8, device='cuda'),
            torch.empty((n,), dtype=torch.uint8, device='cuda'), torch.empty((n,), dtype=torch.int8, device='cuda'),
            torch.empty((n,), dtype=torch.int32, device='cuda')] for _ in range(2)]
    ios = [_lib.SgxPlayoutIO(*[t.data_ptr() for t in r], 0, 0) for r in res]
    buf = TABLES['attacks'].copy()
    stream = first._vec._stream()
    assert second._vec._stream().value == stream.value                     # one stream for both calls
    assert L.sgx_playout_weighted(first._vec._h, env._h, None, ios[0], _p16(buf), 0, 6, stream) == 0, L.sgx_last_error()
    buf[:] = TABLES['forward']                                             # the first call's table is gone
    assert L.sgx_playout_weighted(second._vec._h, env._h, None, ios[1], _p16(buf), 0, 6, stream) == 0, L.sgx_last_error()
    buf[:] = 0
    torch.cuda.synchronize()
    from stratego_env_amd.procedural_env import PlayoutResult
    a = _compare(name, first, PlayoutResult(*res[0]), states, players, 4, 9, 6, TABLES['attacks'], False, None, 0, 'first')
    b = _compare(name, second, PlayoutResult(*res[1]), states, players, 4, 9, 6, TABLES['forward'], False, None, 0, 'second')
    assert not np.array_equal(a[0], b[0]) or not torch.equal(first.unpack()[0], second.unpack()[0]), "the two tables play different games"
    first.close(); second.close(); env.close()


def test_pimc_example_with_a_biased_policy():
    import torch
    from stratego_env_amd.examples.pimc_move_chooser import choose_moves
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, B, W = 'fives', 8, 4
    env = VecStrategoEnv(name, B, seed=9, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(6, emit_obs=False, emit_mask=False)
    states_t, players_t = env.export_state()
    table = pol.capture_biased(name)
    actions, values = choose_moves(env, W, draw=1, seed=4, weights=table)
    pe = BatchedStrategoProceduralEnv(name, B)
    mask = pe.get_valid_moves_as_1d_mask(states_t, players_t) != 0
    assert bool(mask.any(dim=1).all())
    assert bool(mask[torch.arange(B, device=mask.device), actions].all()), "every chosen action is valid in its game"
    assert torch.equal(torch.isfinite(values), mask)
    assert bool((values[mask].abs() <= 1).all())
    again, values_again = choose_moves(env, W, draw=1, seed=4, weights=table)              # the same seeds give the same choices
    assert torch.equal(again, actions) and torch.equal(values_again, values)
    _, uniform_values = choose_moves(env, W, draw=1, seed=4)
    assert not torch.equal(uniform_values, values), "the biased playouts are other games than the uniform ones"
    _, public_values = choose_moves(env, W, draw=1, seed=4, weights=table, see_all=False)
    assert torch.equal(torch.isfinite(public_values), mask)
    after = env.export_state()
    assert torch.equal(after[0], states_t) and torch.equal(after[1], players_t)            # the root env's records are unchanged
    pe.close(); env.close()
