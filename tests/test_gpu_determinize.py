"""sgx_determinize / PackedStates.determinize on the GPU: bit for bit the numpy restatement of the rule (tests/determinize_rule.py, which
tests/test_determinize_cpu.py holds against the oracle's rules) on every compiled-in board size, the source left alone, well-formed records,
the refusals (all host-side, before any launch) and one large run with the invariants checked on the device."""
import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS
from tests import determinize_rule as dr
from tests.pool_roots import _live_env, _np

pytestmark = pytest.mark.gpu

BOARDS = ['standard', 'barrage', 'standard2', 'octa_barrage', 'medium', 'fives', 'tiny', 'micro']     # 10x10, 10x10, 15x15, 8x8, 6x6, 5x5, 4x4, 3x4
DRAWS = (0, 1, 1 << 40)
SGX_EINVAL = -1


@pytest.mark.parametrize('name', BOARDS)
def test_bit_exact_against_the_restatement(name):
    """Identity and gathered src_index (many slots from one root), observer 0 / +1 / -1, three draws, two seeds and a non-zero env_id_offset
    on dst, a live VecStrategoEnv after a rollout as src; hidden[] is the restatement's count and src is byte-identical afterwards."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    v = VARIANTS[name]
    n_src, n = 24, 64
    env = _live_env(name, n_src, min(60, v.max_turns - 3), seed=17)        # games at different depths: auto-reset restarts the short ones
    states_t, players_t = env.export_state()
    states, players = _np(states_t), _np(players_t)
    rs = np.random.RandomState(5)
    idx = rs.randint(0, n_src, size=n).astype(np.int32)
    idx[:20] = 3                                                           # many worlds of one root
    idx_t = torch.from_numpy(idx).cuda()
    moved_hidden = 0
    for seed, offset in ((0, 0), (0xABCDEF0123, 1000)):
        gathered = PackedStates(name, n, seed=seed, env_id_offset=offset)
        identity = PackedStates(name, n_src, seed=seed, env_id_offset=offset)
        for observer in (0, 1, -1):
            for draw in DRAWS:
                for pool, index, index_t in ((gathered, idx, idx_t), (identity, None, None)):
                    hidden = pool.determinize(env, src_index=index_t, observer=observer, draw=draw)
                    got, got_players = pool.unpack()
                    want, want_hidden = dr.determinize_batch(states, players, observer, seed, offset, draw, index)
                    where = (name, seed, observer, draw, 'gathered' if index is not None else 'identity')
                    assert np.array_equal(_np(hidden), want_hidden), where
                    assert np.array_equal(_np(got), want), where
                    assert np.array_equal(_np(got_players), players if index is None else players[index]), where
                    assert int(want_hidden.min()) >= 0, where                # (positions from play are consistent)
        gathered.close(); identity.close()
    for e in range(n_src):                                                 # the shuffle had moved cells to deal with somewhere
        _, A, B, I, M = dr.hidden_lists(states[e], players[e], 0)
        moved_hidden += len(B)
    after_t, after_players_t = env.export_state()
    assert torch.equal(after_t, states_t) and torch.equal(after_players_t, players_t)       # src untouched
    if name in ('standard', 'barrage', 'octa_barrage', 'standard2'):
        assert moved_hidden > 0
    env.close()


@pytest.mark.parametrize('name', ['barrage', 'fives'])
def test_hidden_counts_land_between_guard_bands(name):
    """hidden_dev at every int32 phase between guard bands (tests/test_gpu_guard_bands.py): no byte outside it is written, every element
    inside is."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from tests.guard_bands import Arena, I32_PHASES
    n = 37
    env = _live_env(name, n, 25, seed=4)
    states, players = (_np(t) for t in env.export_state())
    pool = PackedStates(name, n, seed=2, env_id_offset=7)
    vec = pool._vec
    for phase in I32_PHASES:
        ar = Arena('hidden', (n,), torch.int32, phase, vec.device)
        rc = vec._L.sgx_determinize(vec._h, env._h, None, 0, 5, ar.t.data_ptr(), vec._stream())
        assert rc == 0, vec._L.sgx_last_error()
        torch.cuda.synchronize()
        ar.check_guards('sgx_determinize')
        ar.check_written('sgx_determinize')
        want, want_hidden = dr.determinize_batch(states, players, 0, 2, 7, 5)
        assert np.array_equal(ar.host(), want_hidden)
        assert np.array_equal(_np(pool.unpack()[0]), want)
    # hidden_dev is nullable
    assert vec._L.sgx_determinize(vec._h, env._h, None, 0, 6, None, vec._stream()) == 0
    assert np.array_equal(_np(pool.unpack()[0]), dr.determinize_batch(states, players, 0, 2, 7, 6)[0])
    pool.close(); env.close()


@pytest.mark.parametrize('name', ['barrage', 'tiny', 'fives'])
def test_determinized_records_are_well_formed(name):
    """Every determinized record expands like any other: a random valid action played pool to pool gives the oracle's get_next_state of
    the unpacked world (the pattern of test_packed_states_expand_equals_get_next_state)."""
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    v = VARIANTS[name]
    n_src, n = 32, 96
    env = _live_env(name, n_src, 11, seed=21)
    pe = BatchedStrategoProceduralEnv(name, n)
    worlds = pe.new_packed(seed=8)
    idx = torch.from_numpy(np.random.RandomState(2).randint(0, n_src, size=n).astype(np.int32)).cuda()
    hidden = worlds.determinize(env, src_index=idx, observer=0, draw=4)
    assert int(hidden.min()) >= 0
    ws, wp = worlds.unpack()
    masks = pe.get_valid_moves_as_1d_mask(ws, wp)
    acts = torch.multinomial((masks != 0).float(), 1).squeeze(1).to(torch.int32)
    children = pe.new_packed()
    valid, child_players = children.expand(worlds, acts)
    assert bool(valid.all())
    cs, cp = children.unpack()
    ru = orc.OracleRules(v.rows, v.columns)
    ws_h, wp_h, cs_h, cp_h, acts_h = _np(ws), _np(wp), _np(cs), _np(cp), _np(acts)
    for e in range(n):
        want, want_player = ru.get_next_state(ws_h[e], int(wp_h[e]), int(acts_h[e]))
        assert np.array_equal(cs_h[e], want), (name, e)
        assert int(cp_h[e]) == want_player and int(_np(child_players)[e]) == want_player
    for x in (env, pe, worlds, children):
        x.close()


def test_in_place_and_the_int64_api():
    """dst == src with a NULL index works in place; BatchedStrategoProceduralEnv.determinize on reference-layout states (terminal ones
    included) equals the packed path and the restatement."""
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from tests.pool_roots import _sample_states
    for name in ('barrage', 'tiny'):
        n = 48
        states, players = _sample_states(name, n, np.random.RandomState(13))
        pe = BatchedStrategoProceduralEnv(name, n)
        for observer, draw in ((0, 0), (1, 3), (-1, 1 << 40)):
            want, want_hidden = dr.determinize_batch(states, players, observer, 0, 0, draw)
            pool = pe.pack(states, players)
            assert int(pool.sanitised.sum()) == 0
            hidden = pool.determinize(pool, observer=observer, draw=draw)                       # in place
            assert np.array_equal(_np(hidden), want_hidden) and np.array_equal(_np(pool.unpack()[0]), want), (name, observer, draw)
            pool.close()
            got, got_hidden = pe.determinize(states, players, observer=observer, draw=draw)     # int64 in, int64 out
            assert got.dtype == torch.int64 and got_hidden.dtype == torch.int32
            assert np.array_equal(_np(got), want) and np.array_equal(_np(got_hidden), want_hidden), (name, observer, draw)
        pe.close()


def test_an_inconsistent_record_is_copied_unchanged():
    import torch
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
    pe = BatchedStrategoProceduralEnv('fives', n)
    got, hidden = pe.determinize(states, players, observer=1, draw=9)
    want, want_hidden = dr.determinize_batch(states, players, 1, 0, 0, 9)
    assert want_hidden.tolist() == [-1, -1, 4, 4]
    assert np.array_equal(_np(hidden), want_hidden) and np.array_equal(_np(got), want)
    assert np.array_equal(_np(got)[:2], states[:2])
    pe.close()


def test_refusals_are_host_side():
    """SGX_EINVAL with a message and nothing launched: in-place with an index, a foreign variant, a bad observer, a misaligned index."""
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    n = 16
    a = PackedStates('barrage', n)
    b = PackedStates('barrage', n)
    foreign = PackedStates('standard', n)
    L = a._vec._L
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    hidden = torch.full((n,), 77, dtype=torch.int32, device='cuda')
    stream = a._vec._stream()

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(L.sgx_determinize(a._vec._h, a._vec._h, idx.data_ptr(), 0, 0, hidden.data_ptr(), stream), 'sgx_determinize', 'race')
    with pytest.raises(ValueError):
        a.determinize(a, src_index=idx[:n])
    refused(L.sgx_determinize(a._vec._h, foreign._vec._h, None, 0, 0, hidden.data_ptr(), stream), 'different variants')
    with pytest.raises(_lib.SgxError):
        a.determinize(foreign)
    for observer in (2, -2, 13):
        refused(L.sgx_determinize(a._vec._h, b._vec._h, None, observer, 0, hidden.data_ptr(), stream), 'observer')
    with pytest.raises(_lib.SgxError):
        a.determinize(b, observer=2)
    refused(L.sgx_determinize(a._vec._h, b._vec._h, idx.data_ptr() + 2, 0, 0, hidden.data_ptr(), stream), 'src_index_dev', '4-byte aligned')
    refused(L.sgx_determinize(a._vec._h, b._vec._h, None, 0, 0, hidden.data_ptr() + 1, stream), 'hidden_dev', '4-byte aligned')
    small = PackedStates('barrage', n // 2)
    refused(L.sgx_determinize(a._vec._h, small._vec._h, None, 0, 0, None, stream), 'at least as many envs')
    refused(L.sgx_determinize(None, b._vec._h, None, 0, 0, None, stream), 'NULL')
    torch.cuda.synchronize()
    assert bool((hidden == 77).all())                                      # nothing ran
    for x in (a, b, foreign, small):
        x.close()


def test_65536_barrage_records_mid_rollout():
    """One large launch; the invariants of a sampled world checked vectorised on the device."""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    n = 65536
    env = _live_env('barrage', n, 60, seed=3)
    s0, p0 = env.export_state()
    pool = PackedStates('barrage', n, seed=9, env_id_offset=1 << 20)
    hidden = pool.determinize(env, observer=0, draw=2)
    s1, p1 = pool.unpack()
    assert torch.equal(p1, p0)
    opp = (p0 == 1).long()                                                  # layer of the opponent's pieces: 1 for mover +1, else 0
    ar = torch.arange(n, device=s0.device)
    layer = torch.arange(34, device=s0.device)
    other = layer[None, :] != opp[:, None]                                  # [n, 34]: every layer but the opponent's pieces
    assert bool(((s1 == s0).flatten(2).all(dim=2) | ~other).all())
    t0, t1 = s0[ar, opp].flatten(1), s1[ar, opp].flatten(1)                 # the opponent's pieces before / after
    po, still = s0[ar, 3 + opp].flatten(1), s0[ar, 32 + opp].flatten(1)
    hid = (t0 != 0) & (po == 13)
    assert torch.equal(hidden.long(), hid.sum(dim=1))
    assert bool((hidden > 0).all())
    assert bool((t1[~hid] == t0[~hid]).all())                               # revealed and empty cells untouched
    z = torch.zeros_like(t0)
    assert torch.equal(torch.where(hid, t1, z).sort(dim=1).values, torch.where(hid, t0, z).sort(dim=1).values)   # the same types per record
    assert not bool((hid & (still == 0) & ((t1 == 11) | (t1 == 12))).any())                                       # flag / bombs on never-moved cells
    assert not bool((hid & (t1 == 0)).any())
    changed = (t1 != t0).any(dim=1)
    assert float(changed.float().mean()) > 0.9
    assert bool((hid & (still == 0)).any())                                 # moved hidden cells took part
    # the same key gives the same worlds, another draw other ones; the live env is what it was
    again = PackedStates('barrage', n, seed=9, env_id_offset=1 << 20)
    again.determinize(env, observer=0, draw=2)
    assert torch.equal(again.unpack()[0], s1)
    again.determinize(env, observer=0, draw=3)
    s2 = again.unpack()[0]
    assert float((s2[ar, opp].flatten(1) != t1).any(dim=1).float().mean()) > 0.9
    assert torch.equal(env.export_state()[0], s0)
    # a handful of records against the restatement
    pick = [0, 1, 4097, 32768, 65535]
    s0_h, p0_h, s1_h = _np(s0[pick]), _np(p0[pick]), _np(s1[pick])
    for k, e in enumerate(pick):
        want, want_hidden = dr.determinize(s0_h[k], int(p0_h[k]), 0, 9, (1 << 20) + e, 2)
        assert np.array_equal(s1_h[k], want) and int(hidden[e]) == want_hidden
    for x in (env, pool, again):
        x.close()
