"""sgx_determinize_weighted / PackedStates.determinize(..., beliefs=...) on the GPU: bit for bit the numpy restatement of the rule
(tests/determinize_weighted_rule.py, which tests/test_determinize_weighted_cpu.py holds against the oracle's rules and its exact distribution)
on every compiled-in board size, the source left alone, the consequences the header promises, outputs and table between guard bands, the
refusals (all host-side, before any launch) and the PIMC example with a setup prior."""
import numpy as np
import pytest

from stratego_env_amd.config import VARIANTS
from tests import determinize_weighted_rule as wr
from tests.pool_roots import _live_env, _np
from tests.tables import chi2_against, fives_samples, one_hot_truth, skewed_fives_table, third_zero_belief

pytestmark = pytest.mark.gpu

BOARDS = ['standard', 'barrage', 'standard2', 'octa_barrage', 'medium', 'fives', 'tiny', 'micro']     # 10x10, 10x10, 15x15 (four slices), 8x8, 6x6, 5x5, 4x4, 3x4
DRAWS = (0, 1, 1 << 40)
SGX_EINVAL = -1


def _tables(cells, n_src):
    """The table kinds of the bit-exact test: (name, int64 numpy table, shared?)."""
    rs = np.random.RandomState(23)
    big = rs.randint(0, 65536, size=(2, 12, cells))                        # entries above 4095: the clamp
    big[rs.random_sample(big.shape) < 0.25] = 0
    big_each = rs.randint(0, 65536, size=(n_src, 2, 12, cells))
    big_each[rs.random_sample(big_each.shape) < 0.4] = 0
    return [('shared, a third zero', third_zero_belief(cells, seed=1).astype(np.int64), True),
            ('per record, a third zero', third_zero_belief(cells, seed=2, shape=(n_src, 2, 12, cells)).astype(np.int64), False),
            ('shared, entries to 65,535', big.astype(np.int64), True),
            ('all zero', np.zeros((2, 12, cells), dtype=np.int64), True),
            ('per record, entries to 65,535', big_each.astype(np.int64), False)]


@pytest.mark.parametrize('name', BOARDS)
def test_bit_exact_against_the_restatement(name):
    """Identity and gathered src_index (many slots from one root), observer 0 / +1 / -1, three draws, two seeds and a non-zero env_id_offset
    on dst, shared and per-record tables with zeros, with entries above 4095 and all zero, a live VecStrategoEnv after a rollout as src;
    hidden[] and off_belief[] are the restatement's and src is byte-identical afterwards."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    v = VARIANTS[name]
    cells = v.rows * v.columns
    n_src, n = 24, 64
    env = _live_env(name, n_src, min(60, v.max_turns - 3), seed=17)
    states_t, players_t = env.export_state()
    states, players = _np(states_t), _np(players_t)
    rs = np.random.RandomState(5)
    idx = rs.randint(0, n_src, size=n).astype(np.int32)
    idx[:20] = 3                                                           # many worlds of one root
    idx_t = torch.from_numpy(idx).cuda()
    tables = _tables(cells, n_src)
    tables_t = [torch.from_numpy(t.astype(np.int32)).cuda() for _, t, _ in tables]
    combo = fell_back = 0
    for seed, offset in ((0, 0), (0xABCDEF0123, 1000)):
        gathered = PackedStates(name, n, seed=seed, env_id_offset=offset)
        identity = PackedStates(name, n_src, seed=seed, env_id_offset=offset)
        for observer in (0, 1, -1):
            for draw in DRAWS:
                kind, table, shared = tables[combo % len(tables)]
                table_t = tables_t[combo % len(tables)]
                combo += 1
                for pool, index, index_t in ((gathered, idx, idx_t), (identity, None, None)):
                    hidden, off = pool.determinize(env, src_index=index_t, observer=observer, draw=draw, beliefs=table_t,
                                                   return_off_belief=True, validate=False)
                    got, got_players = pool.unpack()
                    want, want_hidden, want_off = wr.determinize_weighted_batch(states, players, observer, table, seed, offset, draw, index)
                    where = (name, seed, observer, draw, kind, 'gathered' if index is not None else 'identity')
                    assert np.array_equal(_np(hidden), want_hidden), where
                    assert np.array_equal(_np(off), want_off), where
                    assert np.array_equal(_np(got), want), where
                    assert np.array_equal(_np(got_players), players if index is None else players[index]), where
                    assert int(want_hidden.min()) >= 0, where                # (positions from play are consistent)
                    if kind == 'all zero':
                        assert np.array_equal(want_off, want_hidden), where  # every draw took the fallback
                    fell_back += int(want_off.sum())
        gathered.close(); identity.close()
    assert fell_back > 0
    after_t, after_players_t = env.export_state()
    assert torch.equal(after_t, states_t) and torch.equal(after_players_t, players_t)       # src untouched
    env.close()


@pytest.mark.parametrize('name', ['c20x20', 'c32x32'])
def test_bit_exact_on_boards_of_many_slices(name):
    """The per-geometry libraries share the kernel: 20 x 20 (seven 64-cell slices, player -1's pieces in slices 5 and 6) and 32 x 32 (sixteen
    slices = the most a lane's bit fields hold; player -1's pieces in slices 14 and 15), 40 pieces of all twelve types per side."""
    import torch
    from stratego_env_amd import config
    from stratego_env_amd.procedural_env import PackedStates
    from tests.boards import CUSTOM
    config.VARIANTS[name] = CUSTOM[name]
    try:
        v = CUSTOM[name]
        cells = v.rows * v.columns
        n_src, n = 6, 16
        env = _live_env(name, n_src, 40, seed=12)
        states, players = (_np(t) for t in env.export_state())
        idx = np.random.RandomState(3).randint(0, n_src, size=n).astype(np.int32)
        idx_t = torch.from_numpy(idx).cuda()
        pool = PackedStates(name, n, seed=5, env_id_offset=77)
        tables = _tables(cells, n_src)
        for k, observer in enumerate((0, 1, -1)):
            for kind, table, shared in (tables[k], tables[3]):
                hidden, off = pool.determinize(env, src_index=idx_t, observer=observer, draw=k, beliefs=torch.from_numpy(table.astype(np.int32)).cuda(),
                                               return_off_belief=True, validate=False)
                want, want_hidden, want_off = wr.determinize_weighted_batch(states, players, observer, table, 5, 77, k, idx)
                assert np.array_equal(_np(hidden), want_hidden) and np.array_equal(_np(off), want_off), (name, observer, kind)
                assert np.array_equal(_np(pool.unpack()[0]), want), (name, observer, kind)
                assert int(want_hidden.min()) >= 20, (name, observer, kind)          # (40 pieces a side, 40 moves in: most are still hidden)
        assert np.array_equal(_np(env.export_state()[0]), states)
        pool.close(); env.close()
    finally:
        config.VARIANTS.pop(name, None)


def test_in_place_and_the_int64_api():
    """dst == src with a NULL index works in place; BatchedStrategoProceduralEnv.determinize on reference-layout states equals the packed
    path and the restatement; hidden_dev and off_belief_dev are nullable; the Python checks of `beliefs`."""
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from tests.pool_roots import _sample_states
    for name in ('barrage', 'tiny'):
        v = VARIANTS[name]
        cells = v.rows * v.columns
        n = 48
        states, players = _sample_states(name, n, np.random.RandomState(13))
        pe = BatchedStrategoProceduralEnv(name, n)
        shared = third_zero_belief(cells, seed=4)
        each = third_zero_belief(cells, seed=5, shape=(n, 2, 12, cells))
        for observer, draw, table in ((0, 0, shared), (1, 3, each), (-1, 1 << 40, shared)):
            want, want_hidden, want_off = wr.determinize_weighted_batch(states, players, observer, table, 0, 0, draw)
            table_t = torch.from_numpy(table.astype(np.int64)).cuda()
            pool = pe.pack(states, players)
            assert int(pool.sanitised.sum()) == 0
            hidden, off = pool.determinize(pool, observer=observer, draw=draw, beliefs=table_t, return_off_belief=True)       # in place
            assert np.array_equal(_np(hidden), want_hidden) and np.array_equal(_np(off), want_off), (name, observer, draw)
            assert np.array_equal(_np(pool.unpack()[0]), want), (name, observer, draw)
            pool.close()
            got, got_hidden, got_off = pe.determinize(states, players, observer=observer, draw=draw, beliefs=table, return_off_belief=True)
            assert got.dtype == torch.int64 and got_hidden.dtype == torch.int32 and got_off.dtype == torch.int32
            assert np.array_equal(_np(got), want) and np.array_equal(_np(got_hidden), want_hidden) and np.array_equal(_np(got_off), want_off)
            got2, hidden2 = pe.determinize(states, players, observer=observer, draw=draw, beliefs=table)
            assert np.array_equal(_np(got2), want) and np.array_equal(_np(hidden2), want_hidden)
        # both outputs nullable at the C ABI
        pool, other = pe.pack(states, players), pe.new_packed()
        vec = other._vec
        t16 = torch.from_numpy(shared.astype(np.int16)).cuda()
        assert vec._L.sgx_determinize_weighted(vec._h, pool._vec._h, None, 0, t16.data_ptr(), 0, 6, None, None, vec._stream()) == 0
        assert np.array_equal(_np(other.unpack()[0]), wr.determinize_weighted_batch(states, players, 0, shared, 0, 0, 6)[0])
        # beliefs=None is the uniform call; the Python layer refuses what it can see
        from tests import determinize_rule as dr
        assert np.array_equal(_np(other.determinize(pool, draw=2)), dr.determinize_batch(states, players, 0, 0, 0, 2)[1])
        with pytest.raises(ValueError):
            other.determinize(pool, beliefs=torch.ones((2, 12, cells), device='cuda'))                      # floats: round them yourself
        with pytest.raises(ValueError):
            other.determinize(pool, beliefs=torch.ones((2, 11, cells), dtype=torch.int32, device='cuda'))
        with pytest.raises(ValueError):
            other.determinize(pool, beliefs=torch.full((2, 12, cells), 4096, dtype=torch.int32, device='cuda'))
        with pytest.raises(ValueError):
            other.determinize(pool, beliefs=torch.full((2, 12, cells), -1, dtype=torch.int32, device='cuda'))
        with pytest.raises(ValueError):
            other.determinize(pool, return_off_belief=True)
        for x in (pool, other, pe):
            x.close()


@pytest.mark.parametrize('name', ['barrage', 'standard2', 'micro'])
def test_one_hot_truth_returns_the_record_and_a_constant_table_keeps_the_keys(name):
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    v = VARIANTS[name]
    cells = v.rows * v.columns
    n_src, n = 24, 64
    env = _live_env(name, n_src, min(40, v.max_turns - 3), seed=6)
    states_t, players_t = env.export_state()
    states = _np(states_t)
    truth = np.stack([one_hot_truth(s) for s in states])
    idx = torch.from_numpy(np.random.RandomState(1).randint(0, n_src, size=n).astype(np.int32)).cuda()
    pool = PackedStates(name, n, seed=4, env_id_offset=9)
    for observer in (0, 1, -1):
        hidden, off = pool.determinize(env, src_index=idx, observer=observer, draw=8, beliefs=torch.from_numpy(truth.astype(np.int32)).cuda(),
                                       return_off_belief=True)
        got, got_players = pool.unpack()
        assert torch.equal(got, states_t[idx.long()]) and torch.equal(got_players, players_t[idx.long()])       # bit for bit
        assert int(off.sum()) == 0 and int(hidden.min()) >= 0
    # a constant table: the worlds differ from the roots, the observer's information-set key does not
    root_keys = env.state_keys(idx, observer=0)
    hidden = pool.determinize(env, src_index=idx, observer=0, draw=8, beliefs=torch.full((2, 12, cells), 9, dtype=torch.int32, device='cuda'))
    assert torch.equal(pool.state_keys(observer=0), root_keys)
    changed = (pool.unpack()[0] != states_t[idx.long()]).flatten(1).any(dim=1)
    if name == 'barrage':                       # (standard2 hides three pieces of one type and a flag, micro two pieces: most deals are the root)
        assert float(changed.float().mean()) > 0.5
        assert not torch.equal(pool.state_keys(), env.state_keys(idx))                                         # (the state keys do differ)
    pool.close(); env.close()


def test_an_inconsistent_record_is_copied_unchanged():
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from tests.helpers import _blank_state, _put
    n = 4
    states = []
    for bad_type, moved in ((12, True), (11, True), (12, False), (11, False)):
        st = _blank_state(5, 5, VARIANTS['fives'].max_turns, 4)
        _put(st, -1, 0, 0, 4); _put(st, -1, 0, 1, 5)
        _put(st, -1, 2, 2, bad_type, moved=moved)
        _put(st, -1, 0, 3, 11 if bad_type == 12 else 6)
        _put(st, 1, 4, 0, 11); _put(st, 1, 4, 1, 7, moved=True)
        states.append(st)
    states = np.stack(states)
    players = np.ones(n, dtype=np.int8)
    table = third_zero_belief(25, seed=8)
    pe = BatchedStrategoProceduralEnv('fives', n)
    got, hidden, off = pe.determinize(states, players, observer=1, draw=9, beliefs=table, return_off_belief=True)
    want, want_hidden, want_off = wr.determinize_weighted_batch(states, players, 1, table, 0, 0, 9)
    assert want_hidden.tolist() == [-1, -1, 4, 4] and want_off[:2].tolist() == [0, 0]
    assert np.array_equal(_np(hidden), want_hidden) and np.array_equal(_np(off), want_off) and np.array_equal(_np(got), want)
    assert np.array_equal(_np(got)[:2], states[:2])
    pe.close()


@pytest.mark.parametrize('kind', ['constant', 'skewed'])
def test_65536_samples_of_the_fives_position(kind):
    """The distribution case of tests/test_determinize_weighted_cpu.py on the device: one root fanned out over 65,536 slots by a src_index
    of zeros, bit-exact against the restatement's samples -- so the chi-squared is the CPU test's."""
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv, PackedStates
    from tests.pool_roots import fives_position
    st, worlds = fives_position()
    n = 65536
    table = np.full((2, 12, 25), 7, dtype=np.uint16) if kind == 'constant' else skewed_fives_table()
    want_layers, want_off = fives_samples(kind)
    pe = BatchedStrategoProceduralEnv('fives', 1)
    src = pe.pack(st[None], np.ones(1, dtype=np.int8))
    assert int(src.sanitised.sum()) == 0
    dst = PackedStates('fives', n, seed=0)
    hidden, off = dst.determinize(src, src_index=torch.zeros(n, dtype=torch.int32, device='cuda'), observer=1, draw=0, beliefs=table,
                                  return_off_belief=True)
    got = dst.unpack()[0]
    assert bool((hidden == 5).all())
    layers = _np(got[:, 1].reshape(n, 25))
    assert np.array_equal(layers, want_layers)
    assert np.array_equal(_np(off), want_off)
    keep = [l for l in range(34) if l != 1]
    assert bool((got[:, keep] == torch.from_numpy(st[keep]).cuda()[None]).all())
    stat, df, pooled, impossible = chi2_against(layers, wr.world_probabilities(st, 1, 1, table))
    assert impossible == 0 and pooled <= 0.05 and stat < wr.chi2_quantile_999(df)
    for x in (src, dst, pe):
        x.close()


@pytest.mark.parametrize('name', ['barrage', 'fives'])
def test_outputs_and_table_between_guard_bands(name):
    """hidden_dev, off_belief_dev and the belief table at every 4-byte phase between guard bands (tests/test_gpu_guard_bands.py), n = 37 so
    that the last workgroup is partial: no byte outside the outputs is written, every element inside is, and the table and its bands are
    what they were.  (dst's records are the library's own allocation: they are held to the restatement byte for byte instead.)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from tests.guard_bands import Arena, I32_PHASES
    v = VARIANTS[name]
    cells = v.rows * v.columns
    n = 37
    env = _live_env(name, n, 25, seed=4)
    states, players = (_np(t) for t in env.export_state())
    pool = PackedStates(name, n, seed=2, env_id_offset=7)
    vec = pool._vec
    for k, phase in enumerate(I32_PHASES):
        shared = k % 2 == 0
        table = third_zero_belief(cells, seed=30 + k, shape=(2, 12, cells) if shared else (n, 2, 12, cells))
        ar_h = Arena('hidden', (n,), torch.int32, phase, vec.device)
        ar_o = Arena('off_belief', (n,), torch.int32, I32_PHASES[(k + 1) % 4], vec.device)
        ar_b = Arena('belief', table.shape, torch.int16, I32_PHASES[(k + 2) % 4], vec.device)
        table_t = torch.from_numpy(table.astype(np.int16)).to(vec.device)
        ar_b.t.copy_(table_t)
        rc = vec._L.sgx_determinize_weighted(vec._h, env._h, None, 0, ar_b.t.data_ptr(), 0 if shared else 2 * 12 * cells, 5,
                                             ar_h.t.data_ptr(), ar_o.t.data_ptr(), vec._stream())
        assert rc == 0, vec._L.sgx_last_error()
        torch.cuda.synchronize()
        for ar in (ar_h, ar_o, ar_b):
            ar.check_guards('sgx_determinize_weighted')
        ar_h.check_written('sgx_determinize_weighted')
        ar_o.check_written('sgx_determinize_weighted')
        assert torch.equal(ar_b.t, table_t)
        want, want_hidden, want_off = wr.determinize_weighted_batch(states, players, 0, table, 2, 7, 5)
        assert np.array_equal(ar_h.host(), want_hidden) and np.array_equal(ar_o.host(), want_off)
        assert np.array_equal(_np(pool.unpack()[0]), want)
    assert np.array_equal(_np(env.export_state()[0]), states)
    pool.close(); env.close()


def test_refusals_are_host_side():
    """SGX_EINVAL with a message under the function's name and nothing launched: what sgx_determinize refuses, a NULL table, bad strides,
    misaligned pointers; the outputs keep their poison, and the same call without the fault goes through."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    n, cells = 16, 100
    a = PackedStates('barrage', n)
    b = PackedStates('barrage', n)
    foreign = PackedStates('standard', n)
    small = PackedStates('barrage', n // 2)
    L = a._vec._L
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    hidden = torch.full((n + 1,), 77, dtype=torch.int32, device='cuda')
    off = torch.full((n + 1,), 77, dtype=torch.int32, device='cuda')
    T = 2 * 12 * cells
    table = torch.ones((n * (T + 2) + 2,), dtype=torch.int16, device='cuda')     # (room for every stride the test passes, and for the off-by-2 pointer)
    stream = a._vec._stream()

    def call(dst=a, src=b, index=None, observer=0, belief=table.data_ptr(), stride=0, hid=hidden.data_ptr(), ob=off.data_ptr()):
        return L.sgx_determinize_weighted(None if dst is None else dst._vec._h, None if src is None else src._vec._h, index, observer, belief, stride, 0,
                                          hid, ob, stream)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in ('sgx_determinize_weighted',) + words), msg

    refused(call(src=a, index=idx.data_ptr()), 'race')
    refused(call(src=foreign), 'different variants')
    for observer in (2, -2, 13):
        refused(call(observer=observer), 'observer')
    refused(call(src=small), 'at least as many envs')
    refused(call(dst=None), 'NULL')
    refused(call(belief=None), 'belief_dev is NULL')
    for stride in (-2, -T, 1, T + 1, 2, T - 2):
        refused(call(stride=stride), 'belief_stride')
    refused(call(index=idx.data_ptr() + 2), 'src_index_dev', '4-byte aligned')
    refused(call(belief=table.data_ptr() + 2), 'belief_dev', '4-byte aligned')
    refused(call(hid=hidden.data_ptr() + 1), 'hidden_dev', '4-byte aligned')
    refused(call(ob=off.data_ptr() + 2), 'off_belief_dev', '4-byte aligned')
    with pytest.raises(ValueError):
        a.determinize(a, src_index=idx[:n], beliefs=table[:T].view(2, 12, cells))
    with pytest.raises(_lib.SgxError):
        a.determinize(foreign, beliefs=table[:T].view(2, 12, cells))
    torch.cuda.synchronize()
    assert bool((hidden == 77).all()) and bool((off == 77).all())          # nothing ran
    # the same calls without the fault: in place without an index, strides 0, T and T + 2, an index
    assert call(src=a) == 0
    for stride in (0, T, T + 2):
        assert call(stride=stride) == 0, L.sgx_last_error()
    assert call(index=idx.data_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((hidden[:n] == 0).all()) and bool((off[:n] == 0).all()) and int(hidden[n]) == 77 and int(off[n]) == 77      # (empty pools: nothing hidden)
    for x in (a, b, foreign, small):
        x.close()


def test_the_pimc_example_with_a_setup_prior():
    import torch
    from stratego_env_amd.beliefs import setup_prior
    from stratego_env_amd.examples.pimc_move_chooser import choose_moves
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv('barrage', 8, seed=1, auto_reset=False)
    env.reset()
    env.rollout_steps(6)
    prior = setup_prior('barrage')
    actions, values = choose_moves(env, n_worlds=2, max_steps=40, beliefs=prior)
    again, values_again = choose_moves(env, n_worlds=2, max_steps=40, beliefs=prior)
    assert torch.equal(actions, again) and torch.equal(values, values_again)
    pool = PackedStates('barrage', 8)
    pool.copy_from(env)
    mask = pool.valid_moves_as_1d_mask() != 0
    assert bool((actions >= 0).all())
    assert bool(mask[torch.arange(8, device=mask.device), actions].all())
    assert bool((torch.isfinite(values) == mask).all())
    pool.close(); env.close()
