"""sgx_set_leaf_values on the GPU: with a table set on dst, sgx_playout, sgx_playout_weighted, sgx_replay and sgx_expand_all report the leaf
values of every position that is not over -- bit for bit the restatement (the playout / weighted / replay / children rule modules as they are,
the rewards of the slots that are not over then replaced by tests/leaf_values_rule.py on the final states), in both views -- and nothing else
changes: every other output and every record is what the same call writes with the table cleared.  Off means off, wave-mates, the setter's
semantics (two tables on one stream, the refusals, guard bands; the gated stream is the row `playout-leaf-values` of tests/stream_cases.py)
and what it is for: a greedy one-ply choice and a truncated PIMC that see a capture.

Roots are taken as tests/test_gpu_playout.py takes them (tests/pool_roots.py: rollouts without auto-reset, its rollout lengths and caps), so
finished and unfinished roots mix; the two boards outside its table get roots from three rollouts -- to the max-turn ending, one move short
of it, and a short one -- so that every cap leaves slots cut off and slots finished (counted per cap over the launches of a test: on Micro
one weighted launch finishes all of its 29 games within 7 moves).  The table is random int16 over the full range with distinct entries: a
wrong cell, row or view cannot cancel."""
import ctypes as C

import numpy as np
import pytest

from tests import children_rule as cr, leaf_values_rule as lv, playout_rule as pr, pool_roots as tp, replay_rule as rr, weighted_playout_rule as wr
from tests.boards import _board
from tests.pool_roots import _np
from tests.tables import third_zero_table

pytestmark = pytest.mark.gpu

SGX_EINVAL = -1
N_SRC = tp.N_SRC
SEED, OFFSET = 0xABCDEF0123, 1000
# no sum of at most 2 x 80 pieces of 32,768 reaches this limit: the sums themselves are compared; SMALL clamps nearly every one
LIMIT, DENOM = (1 << 24) - 5, (1 << 24) - 3
SMALL_LIMIT, SMALL_DENOM = 9000, 9001
WEIGHTS = third_zero_table(0)
# board -> (variant name or key of a custom table, half-wave setting of dst or None)
BOARDS = {'micro': ('micro', None), 'tiny': ('tiny', None), 'fives': ('fives', None), 'medium': ('medium', None), 'octa_barrage': ('octa_barrage', None),
          'barrage-one-game-per-wave': ('barrage', False), 'barrage-two-games-per-wave': ('barrage', True), 'standard2': ('standard2', None),
          'c20x20': ('c20x20', None), 'many66': ('many66', None)}
# the boards outside tests/pool_roots.py's CASES: (the steps of three rollouts of eight games -- to the max-turn ending, one move
# short of it, and a short one --, caps)
THREE_ROLLOUTS = {'c20x20': ((400, 399, 40), (1, 7)), 'many66': ((120, 119, 30), (1, 7))}


def _cells(v):
    from stratego_env_amd.config import get_variant
    v = v if hasattr(v, 'rows') else get_variant(v)
    return v.rows * v.columns


def _table(cells, seed=7):
    return (np.random.RandomState(seed).permutation(65536)[:2 * 14 * cells] - 32768).astype(np.int16).reshape(2, 14, cells)


class Roots:
    """N_SRC roots of a board on the device (`src`: a live env or a pool) and on the host (states, players, finished), and the caps"""

    def __init__(self, board):
        from stratego_env_amd.procedural_env import PackedStates
        key, self.half_wave = BOARDS[board]
        self.v = v = _board(key)
        self.owned = []
        if key in tp.CASES:
            steps, caps, _ = tp.CASES[key]
            self.src, self.states, self.players, self.finished = tp._roots(v, steps)
            assert self.finished.any() and not self.finished.all(), "both finished and unfinished roots"
            self.caps = tuple(c for c in caps if c)                    # (0 = to the end cuts nobody off)
            self.owned.append(self.src)
        else:
            import torch
            rollouts, self.caps = THREE_ROLLOUTS[key]
            third = N_SRC // 3
            self.src = PackedStates(v, N_SRC)
            for k, steps in enumerate(rollouts):
                env = tp._roots(v, steps, n=third, seed=17 + k)[0]
                self.src.copy_from(env, dst_index=np.arange(k * third, (k + 1) * third, dtype=np.int32))
                torch.cuda.synchronize()
                env.close()
            st, pl = self.src.unpack()
            self.states, self.players = _np(st), _np(pl)
            self.finished = self.states[:, 5, 0, 1] != 0
            assert self.finished[:third].all() and not self.finished[2 * third:].all()
            self.owned.append(self.src)
        self.cells = _cells(v)
        self.table = _table(self.cells)

    def pool(self, n, seed=SEED, offset=OFFSET):
        from stratego_env_amd.procedural_env import PackedStates
        p = PackedStates(self.v, n, seed=seed, env_id_offset=offset)
        if self.half_wave is not None:
            p._vec.set_half_wave(self.half_wave)
        self.owned.append(p)
        return p

    def close(self):
        for x in self.owned:
            x.close()


def _outputs(res, keys):
    return {k: _np(getattr(res, k)) for k in keys}


def _records(pool):
    st, pl = pool.unpack()
    return _np(st), _np(pl)


def _check_against_cleared(got, off, got_rec, off_rec, where):
    """every output but the rewards, and the records, are what the cleared call wrote"""
    for k in off:
        if k != 'reward':
            assert got[k].tobytes() == off[k].tobytes(), (where, k)
    assert np.array_equal(got_rec[0], off_rec[0]) and np.array_equal(got_rec[1], off_rec[1]), where


PLAYOUT_KEYS = ('reward', 'done', 'ending_invalid', 'player', 'length')


@pytest.mark.parametrize('board', list(BOARDS))
def test_playouts_bit_exact_against_the_restatement(board):
    import torch
    R = Roots(board)
    n = 29
    idx = np.random.RandomState(5).randint(0, N_SRC, size=n).astype(np.int32)
    idx_t = torch.from_numpy(idx).cuda()
    gathered, identity, in_place = R.pool(n), R.pool(N_SRC), R.pool(N_SRC)
    moves, cut_off, finished = 0, {c: 0 for c in R.caps}, {c: 0 for c in R.caps}
    for weighted in (False, True):
        kw = dict(weights=WEIGHTS, see_all=False) if weighted else {}
        for draw, cap in zip(tp.DRAWS, R.caps):
            for pool, index, index_t in ((gathered, idx, idx_t), (identity, None, None), (in_place, None, None)):
                where = (board, 'weighted' if weighted else 'uniform', cap, 'gathered' if index is not None else 'in place' if pool is in_place else 'identity')

                def run():
                    if pool is in_place:
                        pool.copy_from(R.src)
                        return pool.playout(pool, max_steps=cap, draw=draw, **kw)
                    return pool.playout(R.src, src_index=index_t, max_steps=cap, draw=draw, **kw)

                if pool is not in_place:                                    # (the in-place call plays the identity call's games)
                    if weighted:
                        want = wr.playout_batch(R.v, R.states, R.players, SEED, OFFSET, draw, WEIGHTS, False, index, cap)[:6]
                    else:
                        want = pr.playout_batch(R.v, R.states, R.players, SEED, OFFSET, draw, index, cap)
                    moves += int(want[5].sum())
                want_s, want_p, want_r, want_d, want_e, want_l = want
                cut_off[cap] += int((want_d == 0).sum())
                finished[cap] += int((want_d == 1).sum())
                pool.clear_leaf_values()
                off, off_rec = _outputs(run(), PLAYOUT_KEYS), _records(pool)
                assert off['reward'].tobytes() == want_r.tobytes() and np.array_equal(off['length'], want_l) and np.array_equal(off_rec[0], want_s), where
                for see_all in (False, True):
                    pool.set_leaf_values(R.table, LIMIT, DENOM, see_all=see_all)
                    assert pool.leaf_values_set
                    got, got_rec = _outputs(run(), PLAYOUT_KEYS), _records(pool)
                    expected = lv.apply(want_r, want_d, want_s, R.table, LIMIT, DENOM, see_all)
                    print(where, 'see_all' if see_all else 'public', 'cut off', int((want_d == 0).sum()), 'of', len(want_d))
                    assert got['reward'].tobytes() == expected.tobytes(), (where, see_all)
                    assert (want_d != 0).all() or (expected[want_d == 0] != 0).any()
                    _check_against_cleared(got, off, got_rec, off_rec, (where, see_all))
    st, pl = (R.src.unpack() if hasattr(R.src, 'unpack') else R.src.export_state())
    assert np.array_equal(_np(st), R.states) and np.array_equal(_np(pl), R.players)            # src untouched
    print(board, 'restated moves', moves, 'cut off per cap', cut_off, 'finished per cap', finished)
    assert all(cut_off[c] > 0 and finished[c] > 0 for c in R.caps), "every max_steps used leaves slots cut off and slots finished"
    R.close()


REPLAY_KEYS = ('reward', 'done', 'ending_invalid', 'player', 'applied', 'consumed', 'stop')
CHILD_KEYS = ('reward', 'done', 'ending_invalid', 'player', 'parent', 'action')


@pytest.mark.parametrize('board', list(BOARDS))
def test_replay_and_expand_all_bit_exact_against_the_restatement(board):
    import torch
    from stratego_env_amd.config import get_variant
    R = Roots(board)
    v = R.v if hasattr(R.v, 'rows') else get_variant(R.v)
    n, L = 29, 5
    rs = np.random.RandomState(8)
    idx = rs.randint(0, N_SRC, size=n).astype(np.int32)
    idx[:4] = np.flatnonzero(~R.finished)[:1]                                 # (slots 0..3 share an unfinished root)
    idx_t = torch.from_numpy(idx).cuda()
    # a short list per slot: a valid move of the root first (where it has one), then entries that are mostly invalid and passed over
    n_actions = R.cells * (2 * (v.rows - 1) + 2 * (v.columns - 1) + 1)
    lists = rs.randint(0, n_actions, size=(n, L)).astype(np.int32)
    for i, s in enumerate(idx):
        m = cr.moves(R.v, R.states[s], int(R.players[s]))
        if len(m):
            lists[i, 0] = m[i % len(m)]
    lengths = (np.arange(n) % (L + 1)).astype(np.int32)
    lists_t, lengths_t = torch.from_numpy(lists).cuda(), torch.from_numpy(lengths).cuda()
    pool = R.pool(n)
    for what, acts, acts_t, lens, lens_t in (('max_len 0', np.zeros((n, 0), dtype=np.int32), torch.empty((n, 0), dtype=torch.int32, device='cuda'), None, None),
                                             ('short list', lists, lists_t, lengths, lengths_t)):
        want_s, want_p, want_r, want_d, want_e, want_a, want_c, want_stop = rr.replay_batch(R.v, R.states, R.players, acts, lens, idx, skip_invalid=True)
        assert (want_d == 0).any() and (want_d == 1).any(), (board, what)
        if what == 'short list':
            assert (want_a > 0).any(), "some entries were applied"
        run = lambda: pool.replay(R.src, acts_t, lengths=lens_t, src_index=idx_t, skip_invalid=True)
        pool.clear_leaf_values()
        off, off_rec = _outputs(run(), REPLAY_KEYS), _records(pool)
        assert off['reward'].tobytes() == want_r.tobytes() and np.array_equal(off['applied'], want_a) and np.array_equal(off_rec[0], want_s), (board, what)
        for limit, denom in ((LIMIT, DENOM), (SMALL_LIMIT, SMALL_DENOM)):
            for see_all in (False, True):
                pool.set_leaf_values(R.table, limit, denom, see_all=see_all)
                got, got_rec = _outputs(run(), REPLAY_KEYS), _records(pool)
                expected = lv.apply(want_r, want_d, want_s, R.table, limit, denom, see_all)
                assert got['reward'].tobytes() == expected.tobytes(), (board, what, limit, see_all)
                _check_against_cleared(got, off, got_rec, off_rec, (board, what, limit, see_all))
                if what == 'max_len 0':                                        # evaluate() is this call; in place it scores the pool's own records
                    assert _np(pool.evaluate(R.src, src_index=idx_t)).tobytes() == expected.tobytes()
                    assert _np(pool.evaluate()).tobytes() == expected.tobytes()
                    assert np.array_equal(_records(pool)[0], want_s)
        clamped = np.abs(lv.batch_scores(want_s[want_d == 0], R.table)) > SMALL_LIMIT
        assert clamped.any(), "the small limit clamps"
    # expand_all: the children of eight roots, two windows of a small pool
    some = np.concatenate([np.flatnonzero(~R.finished)[::3][:6], np.flatnonzero(R.finished)[:2]]).astype(np.int32)
    some_t = torch.from_numpy(some).cuda()
    ch = cr.Children(R.v, R.states, R.players, some)
    assert ch.total >= 4
    m = (ch.total + 1) // 2 + 1                                                # the second window ends in slots without a child
    kids = R.pool(m)
    prev = _records(kids)
    offsets = R.src.count_moves(some_t)[1]
    saw_open = saw_over = False
    for first in (0, m):
        w = ch.window(first, m)
        k = len(w['parent'])
        assert k > 0 and (first == 0 or k < m)
        run = lambda: kids.expand_all(R.src, src_index=some_t, offsets=offsets, first_child=first)
        kids.clear_leaf_values()
        off, off_rec = _outputs(run(), CHILD_KEYS), _records(kids)
        assert np.array_equal(off['parent'][:k], w['parent']) and (off['parent'][k:] == -1).all() and off['reward'][:k].tobytes() == w['reward'].tobytes()
        assert np.array_equal(off_rec[0][:k], w['state']) and np.array_equal(off_rec[0][k:], prev[0][k:])
        saw_open |= bool((w['done'] == 0).any())
        saw_over |= bool((w['done'] == 1).any())
        for see_all in (False, True):
            kids.set_leaf_values(R.table, LIMIT, DENOM, see_all=see_all)
            res = run()
            got, got_rec = _outputs(res, CHILD_KEYS), _records(kids)
            expected = lv.apply(w['reward'], w['done'], w['state'], R.table, LIMIT, DENOM, see_all)
            assert got['reward'][:k].tobytes() == expected.tobytes(), (board, first, see_all)
            for key in CHILD_KEYS[1:]:
                assert got[key][:k].tobytes() == off[key][:k].tobytes(), (board, first, see_all, key)
            assert (got['parent'][k:] == -1).all() and (got['action'][k:] == -1).all()
            assert np.array_equal(got_rec[0], off_rec[0]) and np.array_equal(got_rec[1], off_rec[1])   # (slots without a child keep their records)
        prev = off_rec
    assert saw_open, "children whose game goes on"
    print(board, 'children', ch.total, 'finished children seen', saw_over)
    R.close()


def test_off_means_off():
    """set then cleared = never set, byte for byte; sgx_step on a live env and sgx_expand into a pool with a table report the reference's rewards"""
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    R = Roots('fives')
    T = R.table
    idx_t = torch.from_numpy(np.random.RandomState(2).randint(0, N_SRC, size=N_SRC).astype(np.int32)).cuda()
    never, cleared = R.pool(N_SRC), R.pool(N_SRC)
    cleared.set_leaf_values(T, LIMIT, DENOM)
    assert cleared.leaf_values_set and not never.leaf_values_set
    cleared.clear_leaf_values()
    assert not cleared.leaf_values_set
    cleared.clear_leaf_values()                                                # (clearing twice is fine)
    empty = torch.empty((N_SRC, 0), dtype=torch.int32, device='cuda')
    offsets = R.src.count_moves(idx_t)[1]
    calls = (('playout', PLAYOUT_KEYS, lambda p: p.playout(R.src, src_index=idx_t, max_steps=3, draw=4)),
             ('weighted', PLAYOUT_KEYS, lambda p: p.playout(R.src, src_index=idx_t, max_steps=3, draw=4, weights=WEIGHTS)),
             ('replay', REPLAY_KEYS, lambda p: p.replay(R.src, empty, src_index=idx_t)),
             ('expand_all', CHILD_KEYS, lambda p: p.expand_all(R.src, src_index=idx_t, offsets=offsets, first_child=5)))
    for what, keys, call in calls:
        a, b = call(never), call(cleared)
        torch.cuda.synchronize()
        valid = slice(None)
        if what == 'expand_all':                                               # (slots without a child are not written: compare the written ones)
            assert torch.equal(a.parent, b.parent)
            valid = _np(a.parent) >= 0
            assert valid.any()
        for k in keys:
            assert _np(getattr(a, k))[valid].tobytes() == _np(getattr(b, k))[valid].tobytes(), (what, k)
        ra, rb = _records(never), _records(cleared)
        assert np.array_equal(ra[0][valid], rb[0][valid]) and np.array_equal(ra[1][valid], rb[1][valid]), what
        if what != 'expand_all':
            open_ = _np(a.done) == 0
            assert open_.any() and (_np(a.reward)[open_] == 0).all(), "without a table a position that is not over reports 0, 0"
    with pytest.raises(ValueError):
        never.evaluate()
    # sgx_expand into a pool with a table: the step's rewards, 0, 0 where the game goes on
    with_table = R.pool(N_SRC)
    with_table.set_leaf_values(T, LIMIT, DENOM, see_all=True)
    plain = R.pool(N_SRC)
    acts = []
    for s in range(N_SRC):
        m = cr.moves(R.v, R.states[s], int(R.players[s]))
        acts.append(cr.action_1d(R.v, m[0], int(R.players[s])) if len(m) else 0)
    acts_t = torch.tensor(acts, dtype=torch.int32, device='cuda')
    for p in (with_table, plain):
        p.expand(R.src if isinstance(R.src, PackedStates) else _as_pool(R, R.src), acts_t)
    torch.cuda.synchronize()
    assert _np(with_table._vec.reward).tobytes() == _np(plain._vec.reward).tobytes()
    open_ = _np(with_table._vec.done) == 0
    assert open_.any() and (_np(with_table._vec.reward)[open_] == 0).all()
    assert np.array_equal(_records(with_table)[0], _records(plain)[0])
    # sgx_step on a live env that has a table set: the reference's rewards
    from stratego_env_amd.vec_env import VecStrategoEnv
    live = [VecStrategoEnv('fives', 16, seed=3, auto_reset=False, human_inits=False, placement='plain') for _ in range(2)]
    L = live[0]._L
    assert L.sgx_set_leaf_values(live[0]._h, T.ctypes.data_as(C.c_void_p), LIMIT, DENOM, 0) == 0, L.sgx_last_error()
    assert L.sgx_leaf_values_set(live[0]._h) == 1 and L.sgx_leaf_values_set(live[1]._h) == 0 and L.sgx_leaf_values_set(None) == 0
    for e in live:
        e.reset()
        e.sample_valid_actions()
        for _ in range(12):
            e.rollout_step()
    torch.cuda.synchronize()
    for k in ('reward', 'done', 'obs', 'mask'):
        assert torch.equal(getattr(live[0], k), getattr(live[1], k)), k
    assert bool((live[0].reward[live[0].done == 0] == 0).all())
    for e in live:
        e.close()
    R.close()


def _as_pool(R, env):
    from stratego_env_amd.procedural_env import PackedStates
    p = PackedStates(R.v, N_SRC)
    p.copy_from(env)
    R.owned.append(p)
    return p


@pytest.mark.parametrize('board', ['micro', 'fives', 'barrage-two-games-per-wave'])
def test_wave_mates_get_their_own_values(board):
    """two slots of one wave, one finished and one cut off: the finished one keeps its result, the other gets its value"""
    R = Roots(board)
    pool = R.pool(N_SRC)
    pool.set_leaf_values(R.table, LIMIT, DENOM, see_all=True)
    per_wave = {'micro': 4, 'fives': 2, 'barrage-two-games-per-wave': 2}[board]
    pairs = 0
    for draw, cap in zip(tp.DRAWS, R.caps):
        res = pool.playout(R.src, max_steps=cap, draw=draw)
        want_s, want_p, want_r, want_d, want_e, want_l = pr.playout_batch(R.v, R.states, R.players, SEED, OFFSET, draw, None, cap)
        expected = lv.apply(want_r, want_d, want_s, R.table, LIMIT, DENOM, True)
        got = _np(res.reward)
        for w0 in range(0, N_SRC, per_wave):
            d = want_d[w0:w0 + per_wave]
            if (d == 0).any() and (d == 1).any():
                pairs += 1
                assert got[w0:w0 + per_wave].tobytes() == expected[w0:w0 + per_wave].tobytes(), (board, cap, w0)
        assert got.tobytes() == expected.tobytes()
    assert pairs > 0, "a wave with a finished and a cut-off slot occurred"
    R.close()


def test_setter_semantics_and_refusals():
    """replacing the table between two launches on one stream gives each launch its own; the refusals change nothing"""
    import torch
    R = Roots('fives')
    T1, T2 = R.table, _table(R.cells, seed=99)
    pool_a, pool_b = R.pool(N_SRC), R.pool(N_SRC)
    L, h = pool_a._vec._L, pool_a._vec._h
    assert L.sgx_leaf_values_set(h) == 0
    want = pr.playout_batch(R.v, R.states, R.players, SEED, OFFSET, 3, None, 4)
    want_s, _, want_r, want_d = want[0], want[1], want[2], want[3]
    pool_a.set_leaf_values(T1, LIMIT, DENOM)
    res1 = pool_a.playout(R.src, max_steps=4, draw=3)                          # (no synchronisation of the test's between the launch ...
    pool_a.set_leaf_values(T2, 5000, 70000, see_all=True)                     #  ... and the setter, which waits for it itself)
    res2 = pool_a.playout(R.src, max_steps=4, draw=3)
    assert _np(res1.reward).tobytes() == lv.apply(want_r, want_d, want_s, T1, LIMIT, DENOM, False).tobytes()
    assert _np(res2.reward).tobytes() == lv.apply(want_r, want_d, want_s, T2, 5000, 70000, True).tobytes()
    # the table is a setting of the handle: copies do not carry it, and the caller's array is free after the call
    pool_b.copy_from(pool_a)
    assert not pool_b.leaf_values_set
    scribble = T2.copy()
    pool_b.set_leaf_values(scribble, 5000, 70000, see_all=True)
    scribble[:] = 0
    assert _np(pool_b.playout(R.src, max_steps=4, draw=3).reward).tobytes() == _np(res2.reward).tobytes()
    # the refusals: SGX_EINVAL with the function's name, the setting stays what it was
    p16 = T1.ctypes.data_as(C.c_void_p)

    def refused(rc, *words):
        assert rc == SGX_EINVAL
        msg = L.sgx_last_error().decode()
        assert 'sgx_set_leaf_values' in msg and all(w in msg for w in words), msg

    refused(L.sgx_set_leaf_values(None, p16, 1, 1, 0), 'NULL')
    for limit, denom in ((0, 1), (2, 1), (1, 0), (1, (1 << 24) + 1), (-3, 7), ((1 << 24) + 1, (1 << 24) + 1)):
        refused(L.sgx_set_leaf_values(h, p16, limit, denom, 0), 'limit')
    for flags in (2, 4, -1, 3):
        refused(L.sgx_set_leaf_values(h, p16, 1, 1, flags), 'flag')
    assert L.sgx_leaf_values_set(h) == 1
    assert _np(pool_a.playout(R.src, max_steps=4, draw=3).reward).tobytes() == _np(res2.reward).tobytes()
    for bad in (np.zeros((2, 14, R.cells + 1), dtype=np.int16), np.zeros((2, 14, R.cells), dtype=np.float32), np.full((2, 14, R.cells), 40000)):
        with pytest.raises(ValueError):
            pool_a.set_leaf_values(bad, 1, 1)
    with pytest.raises(ValueError):
        pool_a.set_leaf_values(T1, 2, 1)
    assert _np(pool_a.playout(R.src, max_steps=4, draw=3).reward).tobytes() == _np(res2.reward).tobytes()
    # NULL clears and ignores the other arguments; limit == denom == 2^24 and 1, 1 are accepted
    assert L.sgx_set_leaf_values(h, None, -5, -5, 77) == 0 and L.sgx_leaf_values_set(h) == 0
    for limit, denom in ((1 << 24, 1 << 24), (1, 1)):
        assert L.sgx_set_leaf_values(h, p16, limit, denom, 1) == 0, L.sgx_last_error()
        assert _np(pool_a.playout(R.src, max_steps=4, draw=3).reward).tobytes() == lv.apply(want_r, want_d, want_s, T1, limit, denom, True).tobytes()
    R.close()


def test_guard_bands_only_the_rewards_differ():
    """the five result tensors of a playout between guard bands, table off and on: reward is the only one whose bytes differ, nothing
    outside the payloads is written, and a NULL reward pointer writes nothing more"""
    import torch
    from stratego_env_amd import _lib
    from tests.guard_bands import pool_arenas
    R = Roots('fives')
    n = N_SRC
    pool = R.pool(n)
    vec = pool._vec
    L = vec._L
    src_h = R.src._h if hasattr(R.src, '_h') else R.src._vec._h

    def arenas(byte_phase, word_phase):
        return pool_arenas(tp.PLAYOUT_OUT_SPECS, n, vec.device, byte_phase, word_phase)

    def call(ptrs):
        io = _lib.SgxPlayoutIO(ptrs['reward'], ptrs['done'], ptrs['ending_invalid'], ptrs['player'], ptrs['length'], 3, 0)
        return L.sgx_playout(vec._h, src_h, None, io, 5, vec._stream())

    want = pr.playout_batch(R.v, R.states, R.players, SEED, OFFSET, 5, None, 3)
    expected = lv.apply(want[2], want[3], want[0], R.table, LIMIT, DENOM, False)
    for byte_phase, word_phase in ((0, 0), (1, 4), (3, 12)):
        host = {}
        for on in (False, True):
            if on:
                pool.set_leaf_values(R.table, LIMIT, DENOM)
            else:
                pool.clear_leaf_values()
            ar = arenas(byte_phase, word_phase)
            assert call({k: a.t.data_ptr() for k, a in ar.items()}) == 0, L.sgx_last_error()
            torch.cuda.synchronize()
            for k, a in ar.items():
                a.check_guards('sgx_playout with leaf values')
                a.check_written('sgx_playout with leaf values')
            host[on] = {k: a.host() for k, a in ar.items()}
        differ = [k for k in host[True] if host[True][k].tobytes() != host[False][k].tobytes()]
        assert differ == ['reward'], differ
        assert host[True]['reward'].tobytes() == expected.tobytes() and host[False]['reward'].tobytes() == want[2].tobytes()
    ar = arenas(0, 0)                                                          # (the table is still set)
    assert call({k: (None if k == 'reward' else a.t.data_ptr()) for k, a in ar.items()}) == 0, L.sgx_last_error()
    torch.cuda.synchronize()
    for k, a in ar.items():
        a.check_guards('sgx_playout with leaf values')
        if k == 'reward':
            a.check_untouched('sgx_playout with leaf values')
        else:
            assert a.host().tobytes() == host[True][k].tobytes(), k
    R.close()


def _capture_position():
    """fives, +1 to move: its major stands next to a REVEALED sergeant of -1 (a capture) and has quiet moves too; flags in the corners"""
    s = np.zeros((34, 5, 5), dtype=np.int64)
    s[0, 0, 0], s[0, 2, 2], s[0, 0, 4] = 11, 7, 4             # +1: flag, major, sergeant
    s[1, 4, 4], s[1, 2, 3], s[1, 4, 0] = 11, 4, 6             # -1: flag, sergeant (revealed, right of the major), captain
    s[3, 0, 0], s[3, 2, 2], s[3, 0, 4] = 13, 13, 13
    s[4, 4, 4], s[4, 2, 3], s[4, 4, 0] = 13, 4, 13
    s[32, 0, 0] = s[32, 0, 4] = 1
    s[33, 4, 4] = s[33, 4, 0] = 1
    s[5, 0, 0], s[5, 1, 0] = 10, 60                           # turn 10 of 60
    return s


def test_meaning_the_capture_is_seen():
    """greedy one-ply with material and see-all picks the capture; PIMC cut off after two moves values it highest with a leaf table and
    values every action the same (0) without one -- the hole in the parent commit"""
    import torch
    from stratego_env_amd import leaf_values as lvb
    from stratego_env_amd.examples.greedy_one_ply import greedy_moves
    from stratego_env_amd.examples.pimc_move_chooser import choose_moves
    from stratego_env_amd.procedural_env import BatchedStrategoProceduralEnv
    from stratego_env_amd.vec_env import VecStrategoEnv
    name, B = 'fives', 4
    s = _capture_position()
    pe = BatchedStrategoProceduralEnv(name, B)
    states = torch.from_numpy(np.stack([s] * B)).cuda()
    players = torch.ones(B, dtype=torch.int8, device='cuda')
    capture = int(pe.get_action_1d_index_from_positions(2, 2, 2, 3))
    mask = pe.get_valid_moves_as_1d_mask(states, players) != 0
    assert bool(mask[0, capture]) and int(mask[0].sum()) > 3, "the capture and quiet moves are valid"
    table = lvb.material(name)
    limit = denom = 2 * lvb.side_total(name)
    roots = pe.pack(states, players)
    assert int(roots.sanitised.sum()) == 0
    actions, values = greedy_moves(roots, table, limit - 1, denom, see_all=True)
    assert actions.tolist() == [capture] * B
    env = VecStrategoEnv(name, B, seed=1, auto_reset=False, human_inits=False, placement='plain')
    env.reset()
    env.import_state(states, players)
    chosen, val = choose_moves(env, n_worlds=4, draw=2, seed=5, max_steps=2, leaf=(table, limit - 1, denom))
    finite = torch.isfinite(val[0])
    assert torch.equal(finite, mask[0])
    assert chosen.tolist() == [capture] * B
    assert bool((val[0][finite] < val[0, capture]).sum() == int(finite.sum()) - 1), "the capture has the highest value, strictly"
    _, blind = choose_moves(env, n_worlds=4, draw=2, seed=5, max_steps=2, leaf=None)
    assert len(set(blind[0][finite].tolist())) == 1, "without leaf values a truncated playout says nothing"
    roots.close(); pe.close(); env.close()
