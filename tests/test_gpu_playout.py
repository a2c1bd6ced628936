"""sgx_playout / PackedStates.playout on the GPU: bit for bit the numpy restatement of the rule on the oracle (tests/playout_rule.py, which
tests/test_playout_cpu.py holds against the oracle's rules) on every compiled-in board size and two generic ones, ragged batches, the in-place
call and the int64 API, NULL outputs and guard bands, the refusals (all host-side, before any launch) and the PIMC example.

Roots are rollouts WITHOUT auto-reset from random setups (human_inits=False), so a game that has ended stays a finished root; the rollout
lengths below leave some of the 24 games finished and some not (the oracle plays the same rollouts on the CPU: that is how they were chosen),
and every test asserts the mix it relies on.  The restated moves of a test stay under about 60,000."""

import numpy as np
import pytest

from tests import playout_rule as pr
from tests.boards import CUSTOM
from tests.guard_bands import pool_arenas, pool_output_sweep
from tests.pool_roots import CASES, DRAWS, GAMES_PER_WORKGROUP, KEYS, N_SRC, PLAYOUT_OUT_SPECS, _np, _playout_results, _pool_from, _roots, _sample_states

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1


def _compare(variant, pool, res, states, players, seed, offset, draw, index, max_steps, where):
    """the pool's final states and the five result tensors against the restatement; -> the restatement's lengths"""
    want_s, want_p, want_r, want_d, want_e, want_l = pr.playout_batch(variant, states, players, seed, offset, draw, index, max_steps)
    got = _playout_results(res)
    print(where, 'lengths', want_l.tolist())
    assert np.array_equal(got['length'], want_l), where
    assert got['reward'].tobytes() == want_r.tobytes(), where
    assert np.array_equal(got['done'], want_d) and np.array_equal(got['ending_invalid'], want_e), where
    assert np.array_equal(got['player'], want_p), where
    got_s, got_p = pool.unpack()
    assert np.array_equal(_np(got_s), want_s), where
    assert np.array_equal(_np(got_p), want_p), where
    return want_l


@pytest.mark.parametrize('name', list(CASES))
def test_bit_exact_against_the_restatement(name):
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    steps, caps, shared = CASES[name]
    env, states, players, finished = _roots(name, steps)
    assert finished.any() and not finished.all(), "both finished and unfinished roots"
    assert not finished[shared]
    before_t = env.export_state()
    n = 61
    idx = np.random.RandomState(5).randint(0, N_SRC, size=n).astype(np.int32)
    idx[:20] = shared
    idx_t = torch.from_numpy(idx).cuda()
    moves, shared_lengths_differ, wave_mates_differ = 0, False, False
    for seed, offset in KEYS:
        gathered = PackedStates(name, n, seed=seed, env_id_offset=offset)
        identity = PackedStates(name, N_SRC, seed=seed, env_id_offset=offset)
        for max_steps in caps:
            for draw in DRAWS:
                for pool, index, index_t in ((gathered, idx, idx_t), (identity, None, None)):
                    res = pool.playout(env, src_index=index_t, max_steps=max_steps, draw=draw)
                    assert pool.last_launch_kind == _lib.LAUNCH_PLAYOUT
                    where = (name, seed, max_steps, draw, 'gathered' if index is not None else 'identity')
                    lengths = _compare(name, pool, res, states, players, seed, offset, draw, index, max_steps, where)
                    moves += int(lengths.sum())
                    if index is not None:
                        shared_lengths_differ |= len(set(lengths[:20].tolist())) >= 2
                    else:
                        wave_mates_differ |= bool((lengths[0::2] != lengths[1::2]).any())
        gathered.close(); identity.close()
    after_t = env.export_state()
    assert torch.equal(after_t[0], before_t[0]) and torch.equal(after_t[1], before_t[1])           # src untouched
    assert shared_lengths_differ, "the 20 slots of one root played games of at least two lengths"
    assert wave_mates_differ, "two games that share a wave (slots 2j, 2j + 1) ended at different lengths"
    print(name, 'restated moves', moves)
    assert moves < 60000
    env.close()


@pytest.mark.parametrize('name', list(GAMES_PER_WORKGROUP))
def test_ragged_batches(name):
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    steps = CASES[name][0]
    env, states, players, finished = _roots(name, steps)
    wg = GAMES_PER_WORKGROUP[name]
    rs = np.random.RandomState(3)
    for n in (1, wg - 1, wg, wg + 1, 251):
        idx = rs.randint(0, N_SRC, size=n).astype(np.int32)
        pool = PackedStates(name, n, seed=11, env_id_offset=5)
        res = pool.playout(env, src_index=torch.from_numpy(idx).cuda(), draw=n)
        _compare(name, pool, res, states, players, 11, 5, n, idx, 0, (name, n))
        pool.close()
    env.close()


def test_in_place_and_the_int64_api():
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv, PackedStates
    for name, max_steps in (('fives', 0), ('barrage', 9)):
        n = 40
        states, players = _sample_states(name, n, np.random.RandomState(13))           # along golden games, terminal states included
        pe = BatchedStrategoProceduralEnv(name, n)
        src = pe.pack(states, players)
        assert int(src.sanitised.sum()) == 0
        dst = pe.new_packed(n)
        res = dst.playout(src, max_steps=max_steps, draw=3)                             # pool to pool
        want_l = _compare(name, dst, res, states, players, 0, 0, 3, None, max_steps, (name, 'pool to pool'))
        assert (want_l == 0).any() and (want_l > 0).any()
        pool_s, pool_r = _np(dst.unpack()[0]), _playout_results(res)
        res2 = src.playout(src, max_steps=max_steps, draw=3)                            # in place
        assert np.array_equal(_np(src.unpack()[0]), pool_s)
        for k, v in _playout_results(res2).items():
            assert v.tobytes() == pool_r[k].tobytes(), (name, k)
        with pytest.raises(ValueError):
            src.playout(src, src_index=torch.zeros(n, dtype=torch.int32, device='cuda'))
        # int64 in, int64 out
        res3 = pe.playout(states, players, max_steps=max_steps, draw=3)
        for k, v in _playout_results(res3).items():
            assert v.tobytes() == pool_r[k].tobytes(), (name, k)
        res4, final, final_players = pe.playout(states, players, max_steps=max_steps, draw=3, return_states=True)
        assert final.dtype == torch.int64 and np.array_equal(_np(final), pool_s)
        assert np.array_equal(_np(final_players), pool_r['player']) and np.array_equal(_np(res4.length), want_l)
        # value_for: a column for +-1, per slot for a tensor
        assert torch.equal(res3.value_for(1), res3.reward[:, 0]) and torch.equal(res3.value_for(-1), res3.reward[:, 1])
        pl = torch.from_numpy(players).cuda()
        assert torch.equal(res3.value_for(pl), torch.where(pl > 0, res3.reward[:, 0], res3.reward[:, 1]))
        for x in (src, dst, pe):
            x.close()


def test_null_outputs_and_guard_bands():
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'fives', 37
    steps = CASES[name][0]
    env, states, players, finished = _roots(name, steps, n=n)
    pool = PackedStates(name, n, seed=2, env_id_offset=7)
    vec = pool._vec
    L = vec._L
    want = dict(zip(('state', 'player', 'reward', 'done', 'ending_invalid', 'length'), pr.playout_batch(name, states, players, 2, 7, 5)))

    def call(ptrs, ins=None):
        io = _lib.SgxPlayoutIO(ptrs['reward'], ptrs['done'], ptrs['ending_invalid'], ptrs['player'], ptrs['length'], 0, 0)
        return L.sgx_playout(vec._h, env._h, None, io, 5, vec._stream())

    def after_call(ins, skip):
        if skip is None:
            assert np.array_equal(_np(pool.unpack()[0]), want['state'])

    # the five tensors between guard bands, at every phase the contract allows; then each result pointer NULL in turn: the others are still right
    pool_output_sweep(PLAYOUT_OUT_SPECS, vec.device, lambda byte_phase, word_phase: {}, call, want, 'sgx_playout', after_call)
    # the phases the contract refuses: SGX_EINVAL, nothing launched
    for bad, phase in (('reward', 1), ('reward', 2), ('length', 2), ('length', 3)):
        ar = pool_arenas(PLAYOUT_OUT_SPECS, n, vec.device)
        ptrs = {k: a.t.data_ptr() for k, a in ar.items()}
        ptrs[bad] += phase
        assert call(ptrs) == SGX_EINVAL
        assert ('%s_dev' % bad).encode() in L.sgx_last_error() and b'4-byte aligned' in L.sgx_last_error()
        torch.cuda.synchronize()
        for a in ar.values():
            a.check_guards('sgx_playout')
            a.check_untouched('sgx_playout')
    pool.close(); env.close()


def test_refusals_are_host_side():
    """Every refusal is SGX_EINVAL with its message; dst, src and the outputs keep what they held."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    name, n = 'barrage', 16
    env, states, players, _ = _roots(name, 30, n=n)
    a, b = _pool_from(env, name, n), _pool_from(env, name, n)
    foreign = PackedStates('standard', n)
    small = PackedStates(name, n // 2)
    L = a._vec._L
    stream = a._vec._stream()
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    outs = {k: torch.full((n, w) if w > 1 else (n,), 77, dtype=getattr(torch, t), device='cuda') for k, w, t in PLAYOUT_OUT_SPECS}

    def io(max_steps=0, flags=0, reward_off=0, length_off=0):
        return _lib.SgxPlayoutIO(outs['reward'].data_ptr() + reward_off, outs['done'].data_ptr(), outs['ending_invalid'].data_ptr(),
                                 outs['player'].data_ptr(), outs['length'].data_ptr() + length_off, max_steps, flags)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in words), msg

    ah, bh = a._vec._h, b._vec._h
    refused(L.sgx_playout(ah, foreign._vec._h, None, io(), 0, stream), 'different variants')
    with pytest.raises(_lib.SgxError):
        a.playout(foreign)
    refused(L.sgx_playout(ah, ah, idx.data_ptr(), io(), 0, stream), 'sgx_playout', 'race')
    with pytest.raises(ValueError):
        a.playout(a, src_index=idx[:n])
    refused(L.sgx_playout(ah, small._vec._h, None, io(), 0, stream), 'at least as many envs')
    refused(L.sgx_playout(ah, bh, None, io(max_steps=-1), 0, stream), 'max_steps')
    with pytest.raises(_lib.SgxError):
        a.playout(b, max_steps=-3)
    for flags in (1, 2, -1):
        refused(L.sgx_playout(ah, bh, None, io(flags=flags), 0, stream), 'flags')
    refused(L.sgx_playout(ah, bh, idx.data_ptr() + 2, io(), 0, stream), 'src_index_dev', '4-byte aligned')
    refused(L.sgx_playout(ah, bh, None, io(reward_off=2), 0, stream), 'reward_dev', '4-byte aligned')
    refused(L.sgx_playout(ah, bh, None, io(length_off=1), 0, stream), 'length_dev', '4-byte aligned')
    refused(L.sgx_playout(None, bh, None, io(), 0, stream), 'NULL')
    refused(L.sgx_playout(ah, bh, None, None, 0, stream), 'NULL')
    # a dst with a start pool set (the pool: the unfinished games of a fresh env)
    fresh = _pool_from(None, name, n)
    assert L.sgx_set_start_pool(ah, fresh._vec._h, n, 0) == 0, L.sgx_last_error()
    refused(L.sgx_playout(ah, bh, None, io(), 0, stream), 'start pool')
    assert L.sgx_set_start_pool(ah, None, 0, 0) == 0
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == 77).all()), k                                    # nothing ran
    for pool in (a, b):
        got_s, got_p = pool.unpack()
        assert np.array_equal(_np(got_s), states) and np.array_equal(_np(got_p), players)
    # ... and the same call without a fault goes through
    assert L.sgx_playout(ah, bh, None, io(max_steps=2), 0, stream) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    assert not bool((outs['length'] == 77).any())
    for x in (a, b, foreign, small, fresh, env):
        x.close()


@pytest.mark.parametrize('name', ['c7x7', 'c12x12'])
def test_generic_geometries(name):
    """boards outside the reference's variants run the same kernel from their own library: 7x7 (two games per wave), 12x12 (one)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    v = CUSTOM[name]
    n = 16
    env = VecStrategoEnv(v, n, seed=23, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(40, emit_obs=False, emit_mask=False)
    states, players = (_np(t) for t in env.export_state())
    idx = np.random.RandomState(1).randint(0, n, size=n).astype(np.int32)
    pool = PackedStates(v, n, seed=6, env_id_offset=3)
    for index in (None, idx):
        res = pool.playout(env, src_index=None if index is None else torch.from_numpy(index).cuda(), max_steps=12, draw=2)
        _compare(v, pool, res, states, players, 6, 3, 2, index, 12, (name, index is not None))
    pool.close(); env.close()


def test_pimc_example_runs():
    import torch
    from stratego_env_amd.examples.pimc_move_chooser import choose_moves
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, B, W = 'fives', 8, 4
    env = VecStrategoEnv(name, B, seed=9, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(6, emit_obs=False, emit_mask=False)
    states_t, players_t = env.export_state()
    actions, values = choose_moves(env, W, draw=1, seed=4)
    pe = BatchedStrategoProceduralEnv(name, B)
    mask = pe.get_valid_moves_as_1d_mask(states_t, players_t) != 0
    assert bool(mask.any(dim=1).all())                                     # (six moves into a Fives game nobody is stuck)
    assert bool(mask[torch.arange(B, device=mask.device), actions].all()), "every chosen action is valid in its game"
    assert torch.equal(torch.isfinite(values), mask)
    assert bool((values[mask].abs() <= 1).all())
    again, values_again = choose_moves(env, W, draw=1, seed=4)              # the same seeds give the same choices
    assert torch.equal(again, actions) and torch.equal(values_again, values)
    after = env.export_state()
    assert torch.equal(after[0], states_t) and torch.equal(after[1], players_t)            # the root env's records are unchanged
    pe.close(); env.close()
