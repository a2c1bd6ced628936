"""sgx_count_moves / sgx_expand_all / PackedStates.expand_all on the GPU: bit for bit the numpy restatement of the rule on the oracle
(tests/children_rule.py, which tests/test_children_cpu.py holds against the reference's recorded masks) on every compiled-in board size and a
generic one; windows, long root lists on both sides of every boundary of the offsets scan, offsets that do not belong to the roots, NULL
outputs and guard bands, the refusals (all host-side, before any launch), the int64 API and the perft example.

Roots are made exactly as tests/test_gpu_playout.py makes them (24 games, seed 17, no auto-reset, its per-board rollout lengths): finished and
unfinished games on every board; every test asserts the mix it relies on.  Every root's children are restated once per board and shared."""

import numpy as np
import pytest

from tests import children_rule as cr
from tests.pool_roots import CASES, GAMES_PER_WORKGROUP, N_SRC, _np, _pool_from, _roots

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1
# the geometry of the offsets scan (sgx_children.h): SCAN_BLOCK counts per workgroup of the first and third pass; the second pass is one
# workgroup that walks the block sums in chunks of SCAN_BLOCK, so a "full second level" is SCAN_BLOCK * SCAN_BLOCK roots
SCAN_BLOCK = 256
SCAN_LEVEL2 = SCAN_BLOCK * SCAN_BLOCK
SCAN_LENGTHS = (SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SCAN_LEVEL2 - 1, SCAN_LEVEL2, SCAN_LEVEL2 + 1, 70001)
RESULTS = ('reward', 'done', 'ending_invalid', 'player')

_restated = {}


def _setup(name, n=N_SRC):
    """-> (env, states, players, per_root): the roots of tests/test_gpu_playout.py and the cache of their restated children"""
    env, states, players, finished = _roots(name, CASES[name][0], n=n)
    per_root = _restated.setdefault((name, n), {})
    return env, states, players, per_root


def _got(pool, res, m):
    """what a call left in the first m slots: the result tensors and the records"""
    st, pl = pool.unpack()
    out = {k: _np(getattr(res, k))[:m] for k in ('parent', 'action') + RESULTS}
    out['state'], out['record_player'] = _np(st)[:m], _np(pl)[:m]
    return out


def _same(got, want, where, action_key='action'):
    n = len(want['parent'])
    assert np.array_equal(got['parent'][:n], want['parent']), where
    assert np.array_equal(got['action'][:n], want[action_key]), where
    assert got['reward'][:n].tobytes() == want['reward'].tobytes(), where
    for k in ('done', 'ending_invalid', 'player'):
        assert np.array_equal(got[k][:n], want[k]), (where, k)
    assert np.array_equal(got['state'][:n], want['state']), where
    assert np.array_equal(got['record_player'][:n], want['player']), where


def _mix(ch, parent):
    counts = ch.counts
    assert (counts == 0).any(), "a root without a child"
    assert len(set(counts[counts > 0].tolist())) >= 2, "two different non-zero counts"
    m = len(parent) // 2 * 2
    assert (parent[0:m:2] != parent[1:m:2]).any(), "two wave-mates (slots 2j, 2j + 1) with different roots"


@pytest.mark.parametrize('name', list(CASES))
def test_bit_exact_against_the_restatement(name):
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    env, states, players, per_root = _setup(name)
    before_t = env.export_state()
    idx = np.random.RandomState(5).randint(0, N_SRC, size=61).astype(np.int32)
    shared = CASES[name][2]
    idx[:20] = shared
    restated = 0
    for index in (idx, None):
        index_t = None if index is None else torch.from_numpy(index).cuda()
        ch = cr.Children(name, states, players, index, per_root)
        want = ch.window()
        restated += ch.total
        counts, offsets = env.count_moves(index_t)
        assert counts.dtype == torch.int32 and offsets.dtype == torch.int64
        assert np.array_equal(_np(counts), ch.counts) and np.array_equal(_np(offsets), ch.offsets), (name, index is None)
        _mix(ch, want['parent'])
        if index is not None:
            assert ch.counts[0] > 0 and (want['parent'][:ch.counts[0] * 20] < 20).all()           # the shared root's children, 20 times over
        pool = PackedStates(name, ch.total)
        for actions_1d in (False, True):
            for given in (offsets, None):
                res = pool.expand_all(env, src_index=index_t, offsets=given, actions_1d=actions_1d)
                assert pool.last_launch_kind == _lib.LAUNCH_CHILDREN
                assert int(res.total) == ch.total and np.array_equal(_np(res.offsets), ch.offsets)
                _same(_got(pool, res, ch.total), want, (name, index is None, actions_1d), 'action_1d' if actions_1d else 'action')
        pool.close()
    after_t = env.export_state()
    assert torch.equal(after_t[0], before_t[0]) and torch.equal(after_t[1], before_t[1])           # src untouched
    print(name, 'restated children', restated)
    assert restated < 20000
    env.close()


@pytest.mark.parametrize('name', list(GAMES_PER_WORKGROUP))
def test_windows_tile_the_single_call(name):
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    env, states, players, per_root = _setup(name)
    ch = cr.Children(name, states, players, None, per_root)
    want = ch.window()
    _mix(ch, want['parent'])
    total, wg = ch.total, GAMES_PER_WORKGROUP[name]
    _, offsets = env.count_moves()
    whole = PackedStates(name, total)
    single = _got(whole, whole.expand_all(env, offsets=offsets), total)
    _same(single, want, (name, 'single'))
    straddles = False
    for w in (1, wg - 1, wg, wg + 1, 251):
        pool = PackedStates(name, w)
        parts = {k: [] for k in single}
        for first in range(0, total, w):
            m = min(w, total - first)
            res = pool.expand_all(env, offsets=offsets, first_child=first)              # (the last window reaches past total)
            st, pl = pool.unpack()
            for k, t in (('parent', res.parent), ('action', res.action), ('reward', res.reward), ('done', res.done),
                         ('ending_invalid', res.ending_invalid), ('player', res.player), ('state', st), ('record_player', pl)):
                parts[k].append(t[:m].clone())
            if m < w:
                assert bool((res.parent[m:] == -1).all()) and bool((res.action[m:] == -1).all()), (name, w)
            last = first + m - 1
            a, b = want['parent'][first], want['parent'][last]
            straddles |= bool(a != b and first > ch.offsets[a] and last < ch.offsets[b + 1] - 1)
        for k, v in parts.items():
            assert _np(torch.cat(v)).tobytes() == single[k].tobytes(), (name, w, k)
        pool.close()
    assert straddles, "a window that starts inside one root's children and ends inside another's"
    # a window past the total over known records: the tail keeps them
    w = wg + 3
    pool = PackedStates(name, w)
    filler = int(np.flatnonzero(ch.counts > 0)[0])
    pool.copy_from(env, src_index=torch.full((w,), filler, dtype=torch.int32, device='cuda'))
    res = pool.expand_all(env, offsets=offsets, first_child=total - 3)
    got = _got(pool, res, w)
    tail = ch.window(total - 3, 3)
    _same({k: v[:3] for k, v in got.items()}, tail, (name, 'tail window'))
    assert (got['parent'][3:] == -1).all() and (got['action'][3:] == -1).all()
    assert np.array_equal(got['state'][3:], np.repeat(states[filler][None], w - 3, axis=0))
    # ... and one wholly past it
    res = pool.expand_all(env, offsets=offsets, first_child=total + 5)
    assert bool((res.parent == -1).all()) and bool((res.action == -1).all())
    assert np.array_equal(_np(pool.unpack()[0]), got['state'])
    pool.close(); whole.close(); env.close()


@pytest.mark.parametrize('name', ['micro', 'short_barrage'])
def test_many_roots_and_the_scan(name):
    """root lists on both sides of every boundary of the scan (four and two games per wave: 16 and 32 lanes search the offsets)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    env, states, players, per_root = _setup(name)
    base = cr.Children(name, states, players, None, per_root)
    _mix(base, base.window()['parent'])
    rs = np.random.RandomState(8)
    pool = PackedStates(name, 251)
    for n in SCAN_LENGTHS:
        idx = rs.randint(0, N_SRC, size=n).astype(np.int32)
        idx_t = torch.from_numpy(idx).cuda()
        counts, offsets = env.count_moves(idx_t)
        want_offsets = np.concatenate([[0], np.cumsum(base.counts[idx].astype(np.int64))])
        assert np.array_equal(_np(counts), base.counts[idx]), (name, n)
        assert np.array_equal(_np(offsets), want_offsets), (name, n)
        if n != SCAN_LENGTHS[-1]:
            continue
        # three windows of the longest list: at the start, across the root where a scan block AND the second chunk of the second pass
        # start, at the end
        ch = cr.Children(name, states, players, idx, per_root)
        boundary = SCAN_LEVEL2
        across = int(ch.offsets[boundary]) - 100
        assert across > 0 and across + 251 <= ch.total
        for first in (0, across, ch.total - 251):
            res = pool.expand_all(env, src_index=idx_t, offsets=offsets, first_child=first)
            want = ch.window(first, 251)
            assert len(want['parent']) == 251
            if first == across:
                assert want['parent'][0] < boundary <= want['parent'][-1]
            _same(_got(pool, res, 251), want, (name, n, first))
    pool.close(); env.close()


def test_offsets_that_do_not_belong_to_the_roots():
    """offsets built from doubled counts: ranks at or past a root's true count are no-child slots, every other slot is the child it names"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    name = 'fives'
    env, states, players, per_root = _setup(name)
    ch = cr.Children(name, states, players, None, per_root)
    _mix(ch, ch.window()['parent'])
    doubled = np.concatenate([[0], np.cumsum(2 * ch.counts.astype(np.int64))])
    total2 = int(doubled[-1])
    pool = PackedStates(name, total2)
    filler = int(np.flatnonzero(ch.counts == 0)[0])
    pool.copy_from(env, src_index=torch.full((total2,), filler, dtype=torch.int32, device='cuda'))
    res = pool.expand_all(env, offsets=torch.from_numpy(doubled).cuda())
    got = _got(pool, res, total2)
    root = np.searchsorted(doubled, np.arange(total2), side='right') - 1
    rank = np.arange(total2) - doubled[root]
    real = rank < ch.counts[root]
    assert real.sum() == ch.total and (~real).sum() == ch.total
    assert (got['parent'][~real] == -1).all() and (got['action'][~real] == -1).all()
    assert np.array_equal(got['state'][~real], np.repeat(states[filler][None], ch.total, axis=0))
    want = ch.window()                                       # (the real slots, in order, are all children in order)
    _same({k: v[real] for k, v in got.items()}, want, 'doubled offsets')
    # garbage: decreasing, negative and huge entries -- every slot is a child of some root in range or no child at all
    n = pool.n
    for junk in (np.arange(N_SRC + 1)[::-1] * 7, np.full(N_SRC + 1, -5), np.asarray([0] + [1 << 62] * N_SRC), np.asarray([1 << 40] * N_SRC + [1 << 41])):
        res = pool.expand_all(env, offsets=torch.from_numpy(np.ascontiguousarray(junk, dtype=np.int64)).cuda())
        parent, action = _np(res.parent), _np(res.action)
        assert ((parent >= -1) & (parent < N_SRC)).all() and ((action == -1) == (parent == -1)).all()
    pool.close(); env.close()


OUT_SPECS = (('parent', 1, 'int32'), ('action', 1, 'int32'), ('reward', 2, 'float32'), ('done', 1, 'uint8'), ('ending_invalid', 1, 'uint8'),
             ('player', 1, 'int8'))


def test_null_outputs_and_guard_bands():
    import torch
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    from tests.guard_bands import Arena, pool_arenas
    name = 'fives'
    env, states, players, per_root = _setup(name)
    ch = cr.Children(name, states, players, None, per_root)
    n, extra, first = 37, 6, 11
    assert ch.total >= first + n
    want = ch.window(first, n)
    pool = PackedStates(name, n + extra)
    filler = int(np.flatnonzero(ch.counts == 0)[0])
    vec = pool._vec
    L = vec._L
    counts_a = Arena('counts', (N_SRC,), torch.int32, 4, vec.device)
    offsets_a = Arena('offsets', (N_SRC + 1,), torch.int64, 16, vec.device)
    assert L.sgx_count_moves(env._h, None, N_SRC, counts_a.t.data_ptr(), offsets_a.t.data_ptr(), vec._stream()) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    for a, w in ((counts_a, ch.counts), (offsets_a, ch.offsets)):
        a.check_guards('sgx_count_moves'); a.check_written('sgx_count_moves')
        assert a.host().tobytes() == w.tobytes()
    offsets_a.poison()
    assert L.sgx_count_moves(env._h, None, N_SRC, None, offsets_a.t.data_ptr(), vec._stream()) == 0, L.sgx_last_error()     # counts NULL
    torch.cuda.synchronize()
    offsets_a.check_guards('sgx_count_moves')
    assert offsets_a.host().tobytes() == ch.offsets.tobytes()

    def arenas(byte_phase, word_phase):
        return pool_arenas(OUT_SPECS, n, vec.device, byte_phase, word_phase)

    def call(ptrs):
        pool.copy_from(env, src_index=torch.full((n + extra,), filler, dtype=torch.int32, device='cuda'))
        io = _lib.SgxChildrenIO(offsets_a.t.data_ptr(), ptrs['parent'], ptrs['action'], ptrs['reward'], ptrs['done'], ptrs['ending_invalid'],
                                ptrs['player'], N_SRC, first, n, 0, 0)
        return L.sgx_expand_all(vec._h, env._h, None, io, vec._stream())

    def records_ok():
        st = _np(pool.unpack()[0])
        assert np.array_equal(st[:n], want['state'])
        assert np.array_equal(st[n:], np.repeat(states[filler][None], extra, axis=0)), "records beyond n_children are untouched"

    for byte_phase, word_phase in ((0, 0), (1, 4), (3, 12), (13, 8)):
        ar = arenas(byte_phase, word_phase)
        assert call({k: a.t.data_ptr() for k, a in ar.items()}) == 0, L.sgx_last_error()
        torch.cuda.synchronize()
        for k, a in ar.items():
            a.check_guards('sgx_expand_all')
            a.check_written('sgx_expand_all')
            assert a.host().tobytes() == want[k].tobytes(), (k, byte_phase, word_phase)
        offsets_a.check_guards('sgx_expand_all')
        records_ok()
    # each result pointer NULL in turn: the others are still right
    for skip in [k for k, _, _ in OUT_SPECS]:
        ar = arenas(0, 0)
        assert call({k: (None if k == skip else a.t.data_ptr()) for k, a in ar.items()}) == 0, L.sgx_last_error()
        torch.cuda.synchronize()
        for k, a in ar.items():
            a.check_guards('sgx_expand_all')
            if k == skip:
                a.check_untouched('sgx_expand_all')
            else:
                assert a.host().tobytes() == want[k].tobytes(), (k, 'without', skip)
        records_ok()
    # ... and all of them NULL: the records alone
    assert call({k: None for k, _, _ in OUT_SPECS}) == 0, L.sgx_last_error()
    records_ok()
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
    L = a._vec._L
    stream = a._vec._stream()
    ah, bh = a._vec._h, b._vec._h
    idx = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    counts, offsets = b.count_moves()
    offs2 = torch.cat([offsets, offsets])                                  # (room for an offset view at + 8 bytes)
    outs = {'parent': torch.full((n,), 77, dtype=torch.int32, device='cuda'), 'action': torch.full((n,), 77, dtype=torch.int32, device='cuda'),
            'reward': torch.full((n, 2), 77.0, device='cuda'), 'done': torch.full((n,), 77, dtype=torch.uint8, device='cuda'),
            'ending_invalid': torch.full((n,), 77, dtype=torch.uint8, device='cuda'), 'player': torch.full((n,), 77, dtype=torch.int8, device='cuda')}

    def io(offsets_ptr=offsets.data_ptr(), n_roots=n, first=0, n_children=n, flags=0, off=None):
        p = {k: t.data_ptr() for k, t in outs.items()}
        if off:
            p[off[0]] += off[1]
        return _lib.SgxChildrenIO(offsets_ptr, p['parent'], p['action'], p['reward'], p['done'], p['ending_invalid'], p['player'],
                                  n_roots, first, n_children, flags, 0)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(L.sgx_expand_all(None, bh, None, io(), stream), 'sgx_expand_all', 'NULL')
    refused(L.sgx_expand_all(ah, None, None, io(), stream), 'NULL')
    refused(L.sgx_expand_all(ah, bh, None, None, stream), 'NULL')
    refused(L.sgx_expand_all(ah, foreign._vec._h, None, io(), stream), 'different variants')
    refused(L.sgx_expand_all(ah, ah, None, io(), stream), 'src == dst')
    with pytest.raises(ValueError):
        a.expand_all(a)
    refused(L.sgx_expand_all(ah, bh, None, io(n_children=n + 1), stream), 'n_children')
    with pytest.raises(_lib.SgxError):
        a.expand_all(b, n=n + 1)
    for kw in ({'n_roots': -1}, {'n_children': -1}, {'first': -1}):
        refused(L.sgx_expand_all(ah, bh, None, io(**kw), stream), 'negative')
    refused(L.sgx_expand_all(ah, bh, None, io(n_roots=n + 1), stream), 'n_roots')
    for flags in (2, 4, -1):
        refused(L.sgx_expand_all(ah, bh, None, io(flags=flags), stream), 'flag')
    refused(L.sgx_expand_all(ah, bh, None, io(offsets_ptr=None), stream), 'offsets_dev', 'NULL')
    refused(L.sgx_expand_all(ah, bh, None, io(offsets_ptr=offs2.data_ptr() + 8), stream), 'offsets_dev', '16-byte aligned')
    refused(L.sgx_expand_all(ah, bh, idx.data_ptr() + 2, io(), stream), 'src_index_dev', '4-byte aligned')
    for k in ('parent', 'action', 'reward'):
        refused(L.sgx_expand_all(ah, bh, None, io(off=(k, 2)), stream), k + '_dev', '4-byte aligned')
    # sgx_count_moves
    sink_c, sink_o = torch.full((n + 1,), 77, dtype=torch.int32, device='cuda'), torch.full((n + 3,), 77, dtype=torch.int64, device='cuda')
    refused(L.sgx_count_moves(None, None, n, sink_c.data_ptr(), sink_o.data_ptr(), stream), 'sgx_count_moves', 'NULL')
    refused(L.sgx_count_moves(bh, None, n, sink_c.data_ptr(), None, stream), 'offsets_dev', 'NULL')
    refused(L.sgx_count_moves(bh, None, -1, sink_c.data_ptr(), sink_o.data_ptr(), stream), 'n_roots')
    refused(L.sgx_count_moves(bh, None, n + 1, sink_c.data_ptr(), sink_o.data_ptr(), stream), 'n_roots')
    refused(L.sgx_count_moves(bh, None, n, sink_c.data_ptr(), sink_o.data_ptr() + 8, stream), 'offsets_dev', '16-byte aligned')
    refused(L.sgx_count_moves(bh, None, n, sink_c.data_ptr() + 2, sink_o.data_ptr(), stream), 'counts_dev', '4-byte aligned')
    refused(L.sgx_count_moves(bh, idx.data_ptr() + 1, n, sink_c.data_ptr(), sink_o.data_ptr(), stream), 'src_index_dev', '4-byte aligned')
    # a dst with a start pool set (the pool: the unfinished games of a fresh env)
    fresh = _pool_from(None, name, n)
    assert L.sgx_set_start_pool(ah, fresh._vec._h, n, 0) == 0, L.sgx_last_error()
    refused(L.sgx_expand_all(ah, bh, None, io(), stream), 'start pool')
    assert L.sgx_set_start_pool(ah, None, 0, 0) == 0
    torch.cuda.synchronize()
    for k, t in list(outs.items()) + [('counts', sink_c), ('offsets', sink_o)]:
        assert bool((t == 77).all()), k                                    # nothing ran
    for pool in (a, b):
        got_s, got_p = pool.unpack()
        assert np.array_equal(_np(got_s), states) and np.array_equal(_np(got_p), players)
    # the no-ops: n_roots == 0 writes offsets[0] = 0 and nothing else; n_children == 0 launches nothing
    assert L.sgx_count_moves(bh, None, 0, None, sink_o.data_ptr(), stream) == 0, L.sgx_last_error()
    assert _np(sink_o).tolist() == [0] + [77] * (n + 2)
    assert L.sgx_expand_all(ah, bh, None, io(n_children=0), stream) == 0, L.sgx_last_error()
    assert L.sgx_expand_all(ah, bh, None, io(offsets_ptr=sink_o.data_ptr(), n_roots=0), stream) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    assert bool((outs['parent'] == -1).all()) and bool((outs['action'] == -1).all()) and bool((outs['done'] == 77).all())       # (no root: no child)
    assert np.array_equal(_np(a.unpack()[0]), states)
    # ... and the same call without a fault goes through
    assert L.sgx_expand_all(ah, bh, None, io(), stream) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    assert int(offsets[-1]) >= n and not bool((outs['parent'] == -1).any()) and not bool((outs['done'] == 77).any())
    for x in (a, b, foreign, fresh, env):
        x.close()


def test_a_generic_geometry():
    """a board outside the reference's variants runs the same kernels from its own library: 7x7 (two games per wave)"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tests.boards import CUSTOM
    v = CUSTOM['c7x7']
    n = 16
    env = VecStrategoEnv(v, n, seed=23, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.rollout_steps(40, emit_obs=False, emit_mask=False)
    states, players = (_np(t) for t in env.export_state())
    idx = np.random.RandomState(1).randint(0, n, size=n).astype(np.int32)
    per_root = {}
    for index in (None, idx):
        index_t = None if index is None else torch.from_numpy(index).cuda()
        ch = cr.Children(v, states, players, index, per_root)
        assert ch.total > 0
        counts, offsets = env.count_moves(index_t)
        assert np.array_equal(_np(counts), ch.counts) and np.array_equal(_np(offsets), ch.offsets)
        pool = PackedStates(v, ch.total + 2)
        for actions_1d in (False, True):
            res = pool.expand_all(env, src_index=index_t, actions_1d=actions_1d)
            got = _got(pool, res, ch.total + 2)
            _same(got, ch.window(), ('c7x7', index is None, actions_1d), 'action_1d' if actions_1d else 'action')
            assert (got['parent'][ch.total:] == -1).all()
        pool.close()
    env.close()


def test_the_int64_api():
    """BatchedStrategoProceduralEnv.expand_all against get_next_state over get_valid_moves_as_1d_mask: the same set of (parent, action,
    child), in the documented order, through windows of a scratch pool smaller than the number of children"""
    import torch
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    name = 'fives'
    env, states, players, per_root = _setup(name)
    ch = cr.Children(name, states, players, None, per_root)
    pe = BatchedStrategoProceduralEnv(name, N_SRC)
    assert ch.total > 2 * N_SRC, "several windows"
    children, child_players, parent, action = pe.expand_all(states, players)
    assert children.dtype == torch.int64 and tuple(children.shape) == (ch.total,) + states.shape[1:]
    want = ch.window()
    assert np.array_equal(_np(parent), want['parent']) and np.array_equal(_np(action), want['action_1d'])       # the documented order
    assert np.array_equal(_np(children), want['state']) and np.array_equal(_np(child_players), want['player'])
    # the way it replaces: the 1-D mask, nonzero, get_next_state batch by batch
    mask = pe.get_valid_moves_as_1d_mask(states, players) != 0
    mask[:, -1] = False                                                   # the no-op is never a child
    finished = _np(pe.get_game_ended(states, players)) != 0
    pa = _np(torch.nonzero(mask))
    pa = pa[~finished[pa[:, 0]]]
    assert len(pa) == ch.total
    old = {}
    for k0 in range(0, len(pa), N_SRC):
        part = pa[k0:k0 + N_SRC]
        m = len(part)
        pad = np.concatenate([part, np.repeat(part[:1], N_SRC - m, axis=0)])
        ns, npl, ok = pe.get_next_state(states[pad[:, 0]], players[pad[:, 0]], pad[:, 1])
        assert bool(ok.all())
        for (p, a), s, q in zip(part, _np(ns)[:m], _np(npl)[:m]):
            old[(int(p), int(a))] = (s.tobytes(), int(q))
    new = {(int(p), int(a)): (s.tobytes(), int(q)) for p, a, s, q in zip(_np(parent), _np(action), _np(children), _np(child_players))}
    assert new == old
    pe.close(); env.close()


def _rule_perft(name, states, players, depth):
    nodes = [len(states)] + [0] * depth
    frontier = [(s, int(p)) for s, p in zip(states, players)]
    for d in range(depth):
        nxt = []
        for s, p in frontier:
            for a in cr.moves(name, s, p):
                if d + 1 < depth:
                    cs, cp = cr.child(name, s, p, a)[:2]
                    nxt.append((cs, cp))
                nodes[d + 1] += 1
        frontier = nxt
    return nodes


@pytest.mark.parametrize('name', ['micro', 'tiny'])
def test_perft_example(name):
    from stratego_env_amd.examples.perft import perft
    from stratego_env_amd.vec_env import VecStrategoEnv
    env = VecStrategoEnv(name, 5, seed=3, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    states, players = (_np(t) for t in env.export_state())
    want = _rule_perft(name, states, players, 3)
    nodes, windows = perft(env, 3, capacity=7)
    print(name, 'perft', nodes, 'windows', windows)
    assert nodes == want
    assert max(windows) > 1, "a level that needed several windows"
    assert perft(env, 3, capacity=100000)[0] == want
    assert perft(env, 1, capacity=1)[0] == want[:2] and perft(env, 0)[0] == want[:1]
    after = env.export_state()
    assert np.array_equal(_np(after[0]), states)
    env.close()
