"""sgx_state_keys / state_keys on the GPU: bit for bit the numpy restatement of the rule (tests/keys_rule.py, which tests/test_keys_cpu.py
holds against its known answers and against the oracle's positions) applied to the unpacked states -- every compiled-in board size, a wide
board, chained capture events, ragged sizes, guard bands, the refusals (host-side, before any launch), the library's own calls
(determinize, expand_all, copy_from), the int64 API and the example.

Roots are made as tests/test_gpu_playout.py makes them: rollouts without auto-reset, so finished games stay finished roots."""
import numpy as np
import pytest

from tests import keys_rule as kr
from tests.pool_roots import CASES, N_SRC, _np, _roots

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1
VIEWS = (None, 0, 1, -1)                                 # observer: None = the state key


def _want(states, players, observer, clock, wide):
    """the rule on unpacked states, as the int64 the Python classes return: [n], or [n, 2] with wide"""
    w0 = kr.as_int64(kr.keys(states, players, observer=observer, clock=clock, word=0))
    if not wide:
        return w0
    return np.stack([w0, kr.as_int64(kr.keys(states, players, observer=observer, clock=clock, word=1))], axis=1)


def _all_views(src, states, players, index, where):
    """every view, both flags and both widths of `src` against the rule; -> the calls made"""
    import torch
    index_t = None if index is None else torch.from_numpy(np.asarray(index, dtype=np.int32)).cuda()
    s, p = (states, players) if index is None else (states[index], players[index])
    calls = 0
    for observer in VIEWS:
        for clock in (True, False):
            for wide in (False, True):
                got = src.state_keys(index_t, observer=observer, clock=clock, wide=wide)
                assert got.dtype == torch.int64 and tuple(got.shape) == ((len(s), 2) if wide else (len(s),))
                assert np.array_equal(_np(got), _want(s, p, observer, clock, wide)), (where, observer, clock, wide)
                calls += 1
    return calls


@pytest.mark.parametrize('name', list(CASES))
def test_bit_exact_against_the_rule(name):
    import torch
    steps, _, shared = CASES[name]
    env, states, players, finished = _roots(name, steps)
    assert finished.any() and not finished.all(), "both finished and unfinished roots"
    kind = env.last_launch_kind
    idx = np.random.RandomState(5).randint(0, N_SRC, size=61).astype(np.int32)
    idx[:20] = shared
    assert _all_views(env, states, players, None, (name, 'identity')) == 16
    assert _all_views(env, states, players, idx, (name, 'gathered')) == 16
    for observer in VIEWS:
        got = _np(env.state_keys(torch.from_numpy(idx).cuda(), observer=observer, wide=True))
        assert (got[:20] == got[0]).all(), "the 20 slots of one root have one key"
    # different positions have different keys (24 roots: a collision would be a 2^-55 event)
    assert len(set(_np(env.state_keys()).tolist())) == len({(s.tobytes(), int(p)) for s, p in zip(states, players)})
    after = env.export_state()
    assert np.array_equal(_np(after[0]), states) and np.array_equal(_np(after[1]), players)         # src is only read
    assert env.last_launch_kind == kind                                                           # ... and its launch kind left alone
    env.close()


# 256 threads per workgroup, Geo::LPG lanes per record: micro (3x4) four records per wave, fives (5x5) two -- there the lane groups of a
# partly filled wave leave while their wave mates go on to the exchange and the store --, barrage (10x10) one
@pytest.mark.parametrize('name,per_workgroup', [('micro', 16), ('fives', 8), ('barrage', 4)])
def test_ragged_sizes(name, per_workgroup):
    import torch
    env, states, players, _ = _roots(name, CASES[name][0])
    L = env._L
    for n in sorted({1, 2, 3, 5, per_workgroup - 1, per_workgroup, per_workgroup + 1, N_SRC - 1}):      # (2, 3, 5: inside a wave of several records)
        index = np.arange(n, dtype=np.int32)[::-1].copy()
        for wide in (False, True):
            got = env.state_keys(torch.from_numpy(index).cuda(), observer=0, wide=wide)
            assert np.array_equal(_np(got), _want(states[index], players[index], 0, True, wide)), (name, n, wide)
        # the NULL index with n below the handle's envs: records 0 .. n-1, nothing behind them
        out = torch.full((N_SRC,), 77, dtype=torch.int64, device='cuda')
        assert L.sgx_state_keys(env._h, None, n, 2, 0, out.data_ptr(), env._stream()) == 0, L.sgx_last_error()
        got = _np(out)
        assert np.array_equal(got[:n], _want(states[:n], players[:n], None, True, False)) and (got[n:] == 77).all(), (name, n)
    out = torch.full((4, 2), 77, dtype=torch.int64, device='cuda')
    for flags in (0, 2):
        assert L.sgx_state_keys(env._h, None, 0, 2, flags, out.data_ptr(), env._stream()) == 0, L.sgx_last_error()      # n == 0: no launch
    assert tuple(env.state_keys(torch.zeros(0, dtype=torch.int32)).shape) == (0,)
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    env.close()


def test_a_wide_board():
    """20 x 20: 10-bit cell indices, 32-bit capture events, a record of several KiB walked in a loop"""
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests.boards import CUSTOM
    v = CUSTOM['c20x20']
    n = 6
    env = VecStrategoEnv(v, n, seed=23, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(300, emit_obs=False, emit_mask=False)
    states, players = (_np(t) for t in env.export_state())
    assert (states[:, 8:32] != 0).any() and (states[:, 6:8] != 0).any(), "capture events and recent moves are present"
    _all_views(env, states, players, None, 'c20x20')
    _all_views(env, states, players, np.asarray([5, 0, 0, 3, 2], dtype=np.int32), 'c20x20 gathered')
    env.close()


def test_chained_capture_events():
    """many66 (nine scouts a side): a count beyond 8 on one cell is several events of one key in the record and ONE feature, the sum, in the key"""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests.boards import MANY_PIECES as CUSTOM
    v = CUSTOM['many66']
    counts = (7, 8, 9, 16, 17)
    n = len(counts)
    states = np.zeros((n, 34, 6, 6), dtype=np.int64)
    for e, c in enumerate(counts):
        st = states[e]
        st[5, 1, 0], st[5, 0, 0] = v.max_turns, 10
        st[0, 2, 0] = 2; st[3, 2, 0] = 13
        st[1, 3, 0] = 12; st[4, 3, 0] = 13; st[33, 3, 0] = 1
        st[0, 0, 5] = 11; st[3, 0, 5] = 13; st[32, 0, 5] = 1
        st[1, 5, 5] = 11; st[4, 5, 5] = 13; st[33, 5, 5] = 1
        st[1, 5, 0] = 3; st[4, 5, 0] = 13
        st[7 + 2, 3, 0] = c                                      # c scouts of player +1 captured on one cell
        st[19 + 3, 1, 1] = 11                                    # and 11 miners of player -1 on another
    players = np.asarray([1, -1, 1, -1, 1], dtype=np.int8)
    env = VecStrategoEnv(v, n, seed=3, outputs=False)
    san = torch.zeros(n, dtype=torch.uint8, device=env.device)
    env.import_state_checked(states, players, san)
    assert int(san.sum()) == 0
    back, back_players = (_np(t) for t in env.export_state())
    assert np.array_equal(back, states) and np.array_equal(back_players, players)
    _all_views(env, states, players, None, 'many66')
    _all_views(env, states, players, np.asarray([4, 4, 1, 3, 0, 2, 2], dtype=np.int32), 'many66 gathered')
    assert len(set(_np(env.state_keys()).tolist())) == n
    env.close()


@pytest.mark.parametrize('name', ['fives', 'barrage'])
def test_with_the_librarys_own_calls(name):
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    env, states, players, finished = _roots(name, CASES[name][0])
    pool = PackedStates(name, N_SRC, seed=9, env_id_offset=100)
    changed = 0
    for draw, observer in ((0, 0), (1, 1), (2, -1)):
        root_keys = _np(env.state_keys(observer=observer, wide=True))
        hidden = _np(pool.determinize(env, observer=observer, draw=draw))
        assert (hidden >= 0).all()
        assert np.array_equal(_np(pool.state_keys(observer=observer, wide=True)), root_keys), (name, draw, observer)      # one information set
        worlds, world_players = (_np(t) for t in pool.unpack())
        assert np.array_equal(world_players, players)
        differs = (worlds != states).reshape(N_SRC, -1).any(axis=1)
        for clock in (True, False):
            same_key = _np(pool.state_keys(clock=clock)) == _np(env.state_keys(clock=clock))
            assert np.array_equal(same_key, ~differs), (name, draw, observer, clock)                                   # the state key moves exactly with the state
        _all_views(pool, worlds, world_players, None, (name, 'worlds', draw))
        changed += int(differs.sum())
    assert changed > 0, "some world differs from its root"
    pool.copy_from(env)
    for observer in VIEWS:
        assert torch.equal(pool.state_keys(observer=observer, wide=True), env.state_keys(observer=observer, wide=True))
    # all children of the roots
    _, offsets = env.count_moves()
    total = int(offsets[-1])
    assert total > N_SRC
    kids = PackedStates(name, total + 3)
    res = kids.expand_all(env)
    assert int((res.parent >= 0).sum()) == total
    child_states, child_players = (_np(t)[:total] for t in kids.unpack())
    index = np.arange(total, dtype=np.int32)
    for observer in VIEWS:
        for clock in (True, False):
            got = _np(kids.state_keys(torch.from_numpy(index).cuda(), observer=observer, clock=clock))
            assert np.array_equal(got, _want(child_states, child_players, observer, clock, False)), (name, 'children', observer, clock)
    for x in (kids, pool, env):
        x.close()


@pytest.mark.parametrize('name', ['fives', 'barrage'])          # two records per wave / one
def test_guard_bands(name):
    import torch
    from tests.guard_bands import Arena
    env, states, players, _ = _roots(name, CASES[name][0])
    L = env._L
    idx = np.random.RandomState(2).randint(0, N_SRC, size=37).astype(np.int32)
    idx_t = torch.from_numpy(idx).cuda()
    for n, index, index_t in ((N_SRC - 3, None, None), (37, idx, idx_t)):
        s, p = (states[:n], players[:n]) if index is None else (states[index], players[index])
        for wide, phases in ((False, (0, 8, 24, 1016)), (True, (0, 16, 48, 1008))):
            for phase in phases:
                a = Arena('keys', (n + 5, 2) if wide else (n + 5,), torch.int64, phase, env.device)
                assert L.sgx_state_keys(env._h, None if index_t is None else index_t.data_ptr(), n, 2, 2 if wide else 0, a.t.data_ptr(), env._stream()) == 0, \
                    L.sgx_last_error()
                torch.cuda.synchronize()
                a.check_guards('sgx_state_keys')
                a.check_written('sgx_state_keys', rows=list(range(n)))                  # the five rows past n keep the poison
                assert np.array_equal(a.host()[:n], _want(s, p, None, True, wide)), (n, wide, phase)
    env.close()


def test_refusals_are_host_side():
    """Every refusal is SGX_EINVAL with a message that names the call; the output keeps what it held."""
    import torch
    name, n = 'barrage', 16
    env, states, players, _ = _roots(name, 30, n=n)
    L, h, stream = env._L, env._h, env._stream()
    out = torch.full((n + 2, 2), 77, dtype=torch.int64, device='cuda')
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert 'sgx_state_keys' in msg and all(w in msg for w in words), msg

    refused(L.sgx_state_keys(None, None, n, 2, 0, out.data_ptr(), stream), 'handle', 'NULL')
    refused(L.sgx_state_keys(h, None, n, 2, 0, None, stream), 'keys_dev', 'NULL')
    refused(L.sgx_state_keys(h, None, -1, 2, 0, out.data_ptr(), stream), 'n must be')
    refused(L.sgx_state_keys(h, None, n + 1, 2, 0, out.data_ptr(), stream), 'n must not exceed')
    for view in (-2, 3, 13):
        refused(L.sgx_state_keys(h, None, n, view, 0, out.data_ptr(), stream), 'view')
    for flags in (4, 8, -1):
        refused(L.sgx_state_keys(h, None, n, 2, flags, out.data_ptr(), stream), 'flag')
    refused(L.sgx_state_keys(h, None, n, 2, 0, out.data_ptr() + 4, stream), 'keys_dev', '8-byte aligned')
    refused(L.sgx_state_keys(h, None, n, 2, 2, out.data_ptr() + 8, stream), 'keys_dev', '16-byte aligned')
    refused(L.sgx_state_keys(h, idx.data_ptr() + 2, n, 2, 0, out.data_ptr(), stream), 'src_index_dev', '4-byte aligned')
    with pytest.raises(ValueError):
        env.state_keys(observer=2)
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                                 # nothing ran
    # ... and the same calls without a fault go through (keys_dev at + 8 bytes is fine for the narrow key)
    assert L.sgx_state_keys(h, idx.data_ptr() + 4, n, 2, 0, out.data_ptr() + 8, stream) == 0, L.sgx_last_error()
    got = _np(out).reshape(-1)
    assert (got[1:1 + n] == _want(states[:1], players[:1], None, True, False)[0]).all() and got[0] == 77 and (got[1 + n:] == 77).all()
    env.close()


def test_the_int64_api_and_the_known_answers():
    """BatchedStrategoProceduralEnv.state_keys on int64 states: the rule, and on the 3x4 state of the header the known answers themselves"""
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    name = 'fives'
    env, states, players, _ = _roots(name, CASES[name][0])
    pe = BatchedStrategoProceduralEnv(name, N_SRC)
    for observer in VIEWS:
        for clock, wide in ((True, False), (False, True)):
            got = pe.state_keys(states, players, observer=observer, clock=clock, wide=wide)
            assert np.array_equal(_np(got), _want(states, players, observer, clock, wide)), (observer, clock, wide)
    got = pe.state_keys(states[:5], players[:5])                                    # fewer states than the batch size
    assert np.array_equal(_np(got), _want(states[:5], players[:5], None, True, False))
    twice, twice_players = np.concatenate([states, states[::-1]]), np.concatenate([players, players[::-1]])      # ... and more
    assert np.array_equal(_np(pe.state_keys(twice, twice_players, observer=0)), _want(twice, twice_players, 0, True, False))
    # a state the packed record cannot carry (three recent-move cells of one player): the key is that of the state the record holds, strict
    # raises, and last_sanitised -- the flags of the calls that import into the env's own handle -- is not written, whatever n is
    bad = twice.copy()
    bad[3, 6] = 0
    bad[3, 6, 0, :3] = -1
    pe.last_sanitised.fill_(5)
    packed = pe.pack(bad, twice_players)
    assert _np(packed.sanitised).tolist() == [0, 0, 0, 1] + [0] * (len(bad) - 4)
    held, held_players = (_np(t) for t in packed.unpack())
    packed.close()
    assert not np.array_equal(held[3], bad[3]) and np.array_equal(held[4:], bad[4:])
    assert np.array_equal(_np(pe.state_keys(bad, twice_players)), _want(held, held_players, None, True, False))
    assert np.array_equal(_np(pe.state_keys(bad[:7], twice_players[:7])), _want(held[:7], held_players[:7], None, True, False))
    assert bool((pe.last_sanitised == 5).all())
    pe.strict = True
    for m in (7, len(bad)):
        with pytest.raises(ValueError):
            pe.state_keys(bad[:m], twice_players[:m])
    assert np.array_equal(_np(pe.state_keys(twice, twice_players)), _want(twice, twice_players, None, True, False))      # clean states pass under strict
    pe.close(); env.close()
    # the known answers on the device: the 3x4 state of the rule's text (no obstacles: 'micro' without its lake is a custom 3x4)
    from stratego_env_amd.config import custom_variant
    v = custom_variant(3, 4, max_turns=50, piece_counts=(0, 2, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0), name='keys3x4')
    pe = BatchedStrategoProceduralEnv(v, 2)
    pe.strict = True
    s = kr.known_answer_state()
    both = np.stack([s, s])
    movers = np.asarray([1, -1], dtype=np.int8)
    for what, (kw, plus, minus) in kr.KNOWN_ANSWERS.items():
        word = kw.get('word', 0)
        got = _np(pe.state_keys(both, movers, observer=kw.get('observer'), clock=kw.get('clock', True), wide=True))[:, word]
        assert got.view(np.uint64).tolist() == [plus, minus], what
    t = s.copy()
    t[1, 2, 3], t[1, 2, 0] = 10, 11
    for what, (kw, answer) in kr.SWAPPED_HIDDEN.items():
        got = _np(pe.state_keys(np.stack([t, t]), np.asarray([1, 1], dtype=np.int8), observer=kw.get('observer')))
        assert got.view(np.uint64).tolist() == [answer, answer], what
    pe.close()
    v3 = custom_variant(3, 3, max_turns=0, piece_counts=(0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0), name='keys3x3')
    pe = BatchedStrategoProceduralEnv(v3, 1)
    got = _np(pe.state_keys(np.zeros((1, 34, 3, 3), dtype=np.int64), np.asarray([1], dtype=np.int8)))
    assert got.view(np.uint64).tolist() == [kr.ZERO_3X3_STATE_KEY]
    pe.close()


def _rule_levels(name, states, players, depth):
    """-> per depth: (paths, the set of (state with turn count and max turns zeroed, mover)) by the children rule on the CPU"""
    from tests import children_rule as cr

    def ident(s, p):
        z = s.copy()
        z[5, 0, 0] = z[5, 1, 0] = 0
        return (z.tobytes(), int(p))

    frontier = [(s, int(p)) for s, p in zip(states, players)]
    levels = [(len(frontier), {ident(s, p) for s, p in frontier})]
    for d in range(depth):
        nxt = []
        for s, p in frontier:
            for a in cr.moves(name, s, p):
                nxt.append(cr.child(name, s, p, a)[:2])
        frontier = nxt
        levels.append((len(frontier), {ident(s, p) for s, p in frontier}))
    return levels


@pytest.mark.parametrize('name', ['micro', 'tiny'])
def test_unique_positions_example(name):
    from stratego_env_amd.examples.perft import perft
    from stratego_env_amd.examples.unique_positions import unique_positions
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv(name, 4, seed=3, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    states, players = (_np(t) for t in env.export_state())
    levels = _rule_levels(name, states, players, 2)
    positions, distinct = unique_positions(env, 2, capacity=7)                     # (several windows per level)
    print(name, 'positions', positions, 'distinct', distinct)
    assert positions == perft(env, 2, capacity=7)[0] == [n for n, _ in levels]
    assert distinct == [len(s) for _, s in levels]
    assert unique_positions(env, 2, capacity=100000) == (positions, distinct)
    assert unique_positions(env, 0) == (positions[:1], distinct[:1])
    assert np.array_equal(_np(env.export_state()[0]), states)
    env.close()
