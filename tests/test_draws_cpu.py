"""The distribution of every random draw of the build, on the CPU.

The GPU tests hold the kernels to the oracle bit for bit, and the oracle restates the same counter RNG: an error in the DESIGN of a draw
(a shuffle bound, a key that forgets the game number, a seed cut to 32 bits) would be restated faithfully on both sides.  Here the
statistics of tests/test_gpu_draws.py run (a) on the oracle's own restated functions (so_rng, so_rng_below, so_sample_setup,
so_sample_action), 65,536 keys each, so that a defect can be located without a GPU, and (b) on deliberately broken samplers written in
numpy in this file, each of which its statistic must reject: a statistic that lets its broken sampler pass is not sharp enough.

Every chi-squared is held below (teeth: above) the 0.999 quantile for its degrees of freedom and printed with it.  The RNG is a counter
RNG: every figure is a fixed number."""
import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import setups as S
from stratego_env_amd.config import VARIANTS
from tests import draw_stats as ds
from tests.helpers import oracle_cvariant

N = ds.N_KEYS
KEYS = [(s, o) for s in ds.SEEDS for o in ds.OFFSETS]
G = np.arange(N, dtype=np.uint64)


def _ids(offset):
    return G + np.uint64(offset)


# ---- the numpy restatement the broken samplers are variations of ------------------------------------------------------------------------
def test_numpy_rng_is_the_oracles():
    rs = np.random.RandomState(0)
    for i in range(4096):
        seed = int(rs.randint(0, 1 << 62)) * 4 + int(rs.randint(0, 4)) if i % 2 else int(rs.choice(ds.SEEDS))
        g = int(rs.randint(0, 1 << 20)) + int(rs.choice(ds.OFFSETS))
        j, stream, t = int(rs.randint(0, 1 << 40)), int(rs.randint(0, 7)), int(rs.randint(0, 3000))
        r = orc.rng(seed, g, j, stream, t)
        assert int(ds.np_rng(seed, g, j, stream, t)[0]) == r
        n = int(rs.randint(1, 5000))
        assert int(ds.np_rng_below(np.asarray([r], dtype=np.uint64), n)[0]) == orc.rng_below(r, n)


def test_the_one_seed_difference_that_shifts_env_ids():
    """A limit of the key, stated in include/stratego_mi355x.h: the first mix takes seed + phi * (g + 1), so (seed, g) and (seed + phi,
    g - 1) name the same stream -- and no other seed difference tried here does."""
    phi, m64 = 0x9E3779B97F4A7C15, (1 << 64) - 1
    for seed in ds.SEEDS:
        for g in (1, 77, (1 << 20) + 5, (1 << 40) + 9):
            for stream in range(7):
                r = orc.rng(seed, g, 3, stream, 11)
                assert orc.rng((seed + phi) & m64, g - 1, 3, stream, 11) == r
                for other in (seed + 1, seed + (1 << 32), (seed + phi + 1) & m64, (seed - phi) & m64):
                    assert orc.rng(other, g - 1, 3, stream, 11) != r and orc.rng(other, g, 3, stream, 11) != r


def test_numpy_shuffle_is_the_oracles():
    for name in ('micro', 'tiny', 'fives', 'barrage'):
        v = VARIANTS[name]
        n = v.initial_state_usable_rows * v.columns
        cv = oracle_cvariant(name)
        g = np.arange(50, dtype=np.uint64) + np.uint64(1 << 40)
        m1 = ds.placement_maps(ds.np_shuffle(7, g, 3, ds.STREAM_SHUFFLE_P1, n), v.piece_counts)
        m2 = ds.placement_maps(ds.np_shuffle(7, g, 3, ds.STREAM_SHUFFLE_P2, n), v.piece_counts)
        for e in range(50):
            o1, o2 = orc.sample_setup(cv, 7, int(g[e]), 3)
            assert np.array_equal(o1.reshape(-1)[:n], m1[e]) and np.array_equal(o2.reshape(-1)[:n], m2[e])


# ---- (a) the oracle's own functions -------------------------------------------------------------------------------------------------------
def test_raw_draws_of_the_oracle():
    """so_rng / so_rng_below themselves: the draw below 16 is uniform, the low half of the draw as well, the two halves are independent,
    and neighbouring keys (env, game, counter, stream, seed) give independent draws."""
    r = np.asarray([orc.rng(7, g, 0, ds.STREAM_ACTION, 0) for g in range(N)], dtype=np.uint64)
    hi = np.asarray([orc.rng_below(int(x), 16) for x in r])
    assert np.array_equal(hi, ds.np_rng_below(r, 16))
    ds.check('so_rng_below 16', ds.chi2_uniform(hi, 16))
    lo = ((r & np.uint64(0xFFFFFFFF)) >> np.uint64(28)).astype(np.int64)
    ds.check('low half, 16 bins', ds.chi2_uniform(lo, 16))
    ds.check('high half x low half', ds.chi2_independence(ds.two_way(hi, lo, 16, 16)))
    for what, other in (('env g + 1', lambda g: orc.rng(7, g + 1, 0, ds.STREAM_ACTION, 0)), ('game j + 1', lambda g: orc.rng(7, g, 1, ds.STREAM_ACTION, 0)),
                        ('counter t + 1', lambda g: orc.rng(7, g, 0, ds.STREAM_ACTION, 1)), ('playout stream', lambda g: orc.rng(7, g, 0, ds.STREAM_PLAYOUT, 0)),
                        ('seed + 1', lambda g: orc.rng(8, g, 0, ds.STREAM_ACTION, 0)), ('seed + 2^32', lambda g: orc.rng(7 + (1 << 32), g, 0, ds.STREAM_ACTION, 0))):
        r2 = np.asarray([other(g) for g in range(N)], dtype=np.uint64)
        assert (r2 == r).mean() < 0.01
        ds.check('draw x draw of ' + what, ds.chi2_independence(ds.two_way(hi, ds.np_rng_below(r2, 16), 16, 16)))


def _table():
    table = S.load_setup_table('barrage')
    canonical, lookup = ds.table_rows(table)
    return table, canonical, lookup


def _oracle_setup_rows(cv, lookup, seed, offset, j, U):
    p1 = np.zeros((N, U, 10), dtype=np.uint8)
    p2 = np.zeros((N, U, 10), dtype=np.uint8)
    for e in range(N):
        m1, m2 = orc.sample_setup(cv, seed, offset + e, j)
        p1[e], p2[e] = m1[:U], m2[:U]
    return ds.setup_rows_from_maps(p1, p2, lookup)


def test_setup_table_draws_of_the_oracle():
    """so_sample_setup with the shipped Barrage table, seed 0xC0FFEE, env ids from 1 << 40: margins, the pair, and game 0 against game 1."""
    table, canonical, lookup = _table()
    Sn = len(table)
    v = VARIANTS['barrage']
    cv = oracle_cvariant('barrage', setups=table)
    seed, offset = 0xC0FFEE, 1 << 40
    i1, i2 = _oracle_setup_rows(cv, lookup, seed, offset, 0, v.initial_state_usable_rows)
    # the rows the restated draws name (canonical: a row that occurs m times counts at its first occurrence)
    want1 = canonical[ds.np_rng_below(ds.np_rng(seed, _ids(offset), 0, ds.STREAM_SETUP, 0), Sn)]
    want2 = canonical[ds.np_rng_below(ds.np_rng(seed, _ids(offset), 0, ds.STREAM_SETUP, 1), Sn)]
    assert np.array_equal(i1, want1) and np.array_equal(i2, want2)
    ds.check('setup margin +1', ds.setup_margin_stat(i1, canonical))
    ds.check('setup margin -1', ds.setup_margin_stat(i2, canonical))
    ds.check('setup pair 16 x 16', ds.setup_joint_stat(i1, i2, Sn))
    j1, _ = _oracle_setup_rows(cv, lookup, seed, offset, 1, v.initial_state_usable_rows)
    assert (j1 == i1).mean() < 0.01
    ds.check('setup game 0 x game 1', ds.setup_joint_stat(i1, j1, Sn))


def _np_setup(seed, offset, j=0, table_rows=None, canonical=None, p2_counter=1):
    Sn = len(canonical)
    i1 = canonical[ds.np_rng_below(ds.np_rng(seed, _ids(offset), j, ds.STREAM_SETUP, 0), Sn)]
    i2 = canonical[ds.np_rng_below(ds.np_rng(seed, _ids(offset), j, ds.STREAM_SETUP, p2_counter), Sn)]
    return i1, i2


@pytest.mark.parametrize('seed,offset', KEYS)
def test_setup_table_draws_at_every_key(seed, offset):
    """The restated arithmetic (held against so_sample_setup above) at all twelve (seed, offset) pairs of the GPU test."""
    table, canonical, lookup = _table()
    Sn = len(table)
    i1, i2 = _np_setup(seed, offset, canonical=canonical)
    tag = 'seed %#x offset %#x ' % (seed, offset)
    ds.check(tag + 'margin +1', ds.setup_margin_stat(i1, canonical))
    ds.check(tag + 'margin -1', ds.setup_margin_stat(i2, canonical))
    ds.check(tag + 'pair', ds.setup_joint_stat(i1, i2, Sn))
    ds.check(tag + 'env g x g + 1', ds.setup_joint_stat(i1[0::2], i1[1::2], Sn))
    for what, (s2, o2, j2) in (('seed + 1', (seed + 1, offset, 0)), ('seed + 2^32', (seed + (1 << 32), offset, 0)), ('game 1', (seed, offset, 1)),
                               ('offset + 2^20', (seed, offset + (1 << 20), 0)), ('offset + 2^40', (seed, offset + (1 << 40), 0))):
        k1, k2 = _np_setup(s2, o2, j2, canonical=canonical)
        assert ((k1 == i1) & (k2 == i2)).mean() < 0.01
        ds.check(tag + 'x ' + what, ds.setup_joint_stat(i1, k1, Sn))


def _oracle_placements(name, seed, offset, j=0):
    v = VARIANTS[name]
    n = v.initial_state_usable_rows * v.columns
    cv = oracle_cvariant(name)
    m1 = np.zeros((N, n), dtype=np.int64)
    m2 = np.zeros((N, n), dtype=np.int64)
    for e in range(N):
        a, b = orc.sample_setup(cv, seed, offset + e, j)
        m1[e], m2[e] = a.reshape(-1)[:n], b.reshape(-1)[:n]
    return m1, m2


@pytest.mark.parametrize('name,seed,offset', [('micro', 0, 0), ('tiny', 1, 1 << 20), ('fives', 7, 1 << 40)])
def test_random_placements_of_the_oracle(name, seed, offset):
    m1, m2 = _oracle_placements(name, seed, offset)
    for k, st in ds.placement_stats(VARIANTS[name].piece_counts, m1, m2, name + ' ').items():
        ds.check(k, st)
    for pl, m in ((1, m1), (-1, m2)):
        seen, worlds, st = ds.arrangement_stat(VARIANTS[name].piece_counts, m)
        print('%s player %+d: %d of %d arrangements' % (name, pl, seen, worlds))
        assert seen == worlds
        ds.check('%s arrangements %+d' % (name, pl), st)


def test_random_placements_barrage_numpy():
    """40 cells, 8 pieces: the restated shuffle (held against so_sample_setup above)."""
    v = VARIANTS['barrage']
    g = _ids(0)
    m1 = ds.placement_maps(ds.np_shuffle(0xC0FFEE, g, 0, ds.STREAM_SHUFFLE_P1, 40), v.piece_counts)
    m2 = ds.placement_maps(ds.np_shuffle(0xC0FFEE, g, 0, ds.STREAM_SHUFFLE_P2, 40), v.piece_counts)
    for k, st in ds.placement_stats(v.piece_counts, m1, m2, 'barrage ').items():
        ds.check(k, st)


def _np_pool(seed, offset, games, n_pool, key_game=True, first_counter=1):
    j = np.arange(games, dtype=np.uint64)[None, :] * np.uint64(1 if key_game else 0)
    g = _ids(offset)[:, None]
    rows = ds.np_rng_below(ds.np_rng(seed, g, j, ds.STREAM_POOL, 0), n_pool)
    first = np.where(ds.np_rng_below(ds.np_rng(seed, g, j, ds.STREAM_POOL, first_counter), 2) == 1, -1, 1)
    return rows, first


@pytest.mark.parametrize('seed,offset', [(0, 1 << 20), (0xC0FFEE, 0)])
def test_start_pool_draws(seed, offset):
    """pool_index / pool_first_player (sgx_layout.h; the oracle has no start pool: so_rng / so_rng_below carry the rule, as in
    tests/test_start_pool_cpu.py): 16 rows, four consecutive games."""
    rows, first = _np_pool(seed, offset, 4, 16)
    for e in range(0, N, 4099):
        for j in range(4):
            assert rows[e, j] == orc.rng_below(orc.rng(seed, offset + e, j, ds.STREAM_POOL, 0), 16)
            assert first[e, j] == (-1 if orc.rng_below(orc.rng(seed, offset + e, j, ds.STREAM_POOL, 1), 2) == 1 else 1)
    for k, st in ds.pool_stats(rows, first, 16).items():
        ds.check(k, st)


def test_action_draws_of_the_oracle():
    """so_sample_action on masks of 1 .. 40 valid actions out of 64, four consecutive turns of 65,536 games, and the same keys on the
    playout stream: the action is valid, its PIT is uniform, and turns, envs and the two streams are independent."""
    rs = np.random.RandomState(1)
    T, A = 4, 64
    seed, offset = 7, 1 << 20
    masks = np.zeros((T, N, A), dtype=np.uint8)
    totals = rs.randint(1, 41, size=(T, N))
    for t in range(T):
        order = np.argsort(rs.random_sample((N, A)), axis=1)
        masks[t] = (np.argsort(order, axis=1) < totals[t][:, None]).astype(np.uint8)
    acts = np.zeros((T, N), dtype=np.int64)
    for t in range(T):
        for e in range(N):
            acts[t, e] = orc.sample_action(masks[t, e], seed, offset + e, 0, 10 + t)
    u = np.zeros((N, T))
    k0 = None
    for t in range(T):
        k, total, valid = ds.ranks_in_masks(masks[t], acts[t])
        assert valid.all() and np.array_equal(total, totals[t])
        assert np.array_equal(k, ds.np_rng_below(ds.np_rng(seed, _ids(offset), 0, ds.STREAM_ACTION, 10 + t), total))
        u[:, t] = ds.pit(k, total, rs)
        k0 = (k, total) if t == 0 else k0
    for name, st in ds.action_stats(u).items():
        ds.check(name, st)
    kp = ds.np_rng_below(ds.np_rng(seed, _ids(offset), 0, ds.STREAM_PLAYOUT, 10), k0[1])
    ds.check('PIT action x playout stream', ds.pit_pair_stat(u[:, 0], ds.pit(kp, k0[1], rs)))
    # one key at two totals: the two quantisations of one variate (with the first `total` actions valid the action is its rank)
    m12, m16 = ds.first_valid_mask(1, A, 12)[0], ds.first_valid_mask(1, A, 16)[0]
    k12 = np.asarray([orc.sample_action(m12, seed, offset + e, 0, 10) for e in range(N)])
    k16 = np.asarray([orc.sample_action(m16, seed, offset + e, 0, 10) for e in range(N)])
    ds.check('so_sample_action of one key at 12 and 16 valid actions', ds.quantisation_joint_stat(k12, 12, k16, 16))


# ---- (b) teeth: every broken sampler lands above the threshold ----------------------------------------------------------------------------
def _rejected(name, stat):
    chi2, limit = ds.report('BROKEN ' + name, stat)
    assert chi2 > limit, (name, 'the statistic lets this broken sampler pass', chi2, limit)


def _np_actions(seed, offset, totals, rs, key_turn=True, below=None):
    T = totals.shape[1]
    u = np.zeros(totals.shape)
    for t in range(T):
        r = ds.np_rng(seed, _ids(offset), 0, ds.STREAM_ACTION, 10 + (t if key_turn else 0))
        k = ds.np_rng_below(r, totals[:, t]) if below is None else below(r, totals[:, t])
        u[:, t] = ds.pit(k, totals[:, t], rs)
    return u


def test_teeth_sattolo_shuffle():
    """rng_below(r, i) in place of rng_below(r, i + 1): no piece stays where the list had it, only cyclic orders appear."""
    for name in ('micro', 'tiny', 'fives', 'barrage'):
        v = VARIANTS[name]
        n = v.initial_state_usable_rows * v.columns
        good = ds.placement_maps(ds.np_shuffle(3, G, 0, ds.STREAM_SHUFFLE_P1, n), v.piece_counts)
        ds.check(name + ' cells x types', ds.cell_by_type_stat(good, v.piece_counts))
        bad = ds.placement_maps(ds.np_shuffle(3, G, 0, ds.STREAM_SHUFFLE_P1, n, bound=0), v.piece_counts)
        _rejected(name + ' Sattolo, cells x types', ds.cell_by_type_stat(bad, v.piece_counts))
    seen, worlds, st = ds.arrangement_stat(VARIANTS['micro'].piece_counts, ds.placement_maps(ds.np_shuffle(3, G, 0, ds.STREAM_SHUFFLE_P1, 4, bound=0), VARIANTS['micro'].piece_counts))
    assert seen < worlds
    _rejected('micro Sattolo, arrangements (%d of %d)' % (seen, worlds), st)


def test_teeth_both_players_on_one_stream():
    v = VARIANTS['tiny']
    m1 = ds.placement_maps(ds.np_shuffle(3, G, 0, ds.STREAM_SHUFFLE_P1, 4), v.piece_counts)
    m2 = ds.placement_maps(ds.np_shuffle(3, G, 0, ds.STREAM_SHUFFLE_P1, 4), v.piece_counts)          # (should be STREAM_SHUFFLE_P2)
    _rejected('player -1 shuffles with the stream of player +1', ds.placement_stats(v.piece_counts, m1, m2)['flag +1 x flag -1'])
    _, canonical, _ = _table()
    i1, i2 = _np_setup(0, 0, canonical=canonical, p2_counter=0)                                   # (should be counter 1)
    _rejected('player -1 draws the setup with the counter of player +1', ds.setup_joint_stat(i1, i2, len(canonical)))
    rows, first = _np_pool(0, 0, 4, 16, first_counter=0)
    _rejected('the first mover draws with the counter of the pool row', ds.pool_stats(rows, first, 16)['pool row x first mover'])


def test_teeth_game_number_left_out():
    rows, first = _np_pool(0, 0, 4, 16, key_game=False)
    st = ds.pool_stats(rows, first, 16)
    _rejected('game number left out, pool rows', st['pool row of game j x game j + 1'])
    _rejected('game number left out, first movers', st['first mover of game j x game j + 1'])
    _, canonical, _ = _table()
    i1, _ = _np_setup(0, 0, 0, canonical=canonical)
    k1, _ = _np_setup(0, 0, 0, canonical=canonical)                                               # (game 1 drawn with j = 0)
    _rejected('game number left out, setups', ds.setup_joint_stat(i1, k1, len(canonical)))


def test_teeth_turn_left_out():
    rs = np.random.RandomState(2)
    totals = rs.randint(1, 41, size=(N, 4))
    for name, st in ds.action_stats(_np_actions(7, 0, totals, rs)).items():
        ds.check('control ' + name, st)
    _rejected('turn left out of the key', ds.action_stats(_np_actions(7, 0, totals, rs, key_turn=False))['PIT turn t x t + 1'])


def test_teeth_env_id_offset_left_out():
    _, canonical, _ = _table()
    i1, i2 = _np_setup(1, 0, canonical=canonical)
    k1, k2 = _np_setup(1, 0, canonical=canonical)                                                 # (the rank at offset 1 << 20 keyed without it)
    assert ((i1 == k1) & (i2 == k2)).mean() >= 0.01
    _rejected('env_id_offset left out of the key', ds.setup_joint_stat(i1, k1, len(canonical)))


def test_teeth_seed_masked_to_32_bits():
    _, canonical, _ = _table()
    s = 7
    i1, i2 = _np_setup(s & 0xFFFFFFFF, 0, canonical=canonical)
    k1, k2 = _np_setup((s + (1 << 32)) & 0xFFFFFFFF, 0, canonical=canonical)
    assert ((i1 == k1) & (i2 == k2)).mean() >= 0.01
    _rejected('seed masked to 32 bits', ds.setup_joint_stat(i1, k1, len(canonical)))


def test_teeth_modulo_of_a_draw_below_16():
    """k % total of a draw below 16: with 12 valid actions the first four are twice as likely."""
    rs = np.random.RandomState(4)
    totals = np.full((N, 4), 12)
    u = _np_actions(7, 0, totals, rs, below=lambda r, total: ds.np_rng_below(r, 16) % total)
    _rejected('k % total of a draw below 16', ds.action_stats(u)['PIT margin'])


def test_teeth_low_half_modulo_12():
    """rng_below fed the low half of the draw through r % n, n = 12.

    Read as "the low half, a 32-bit value, handed to rng_below" the sampler is the constant 0 ((r >> 32) of a 32-bit value) and every
    statistic rejects it.

    Read as `k = (r & 0xFFFFFFFF) % n` it is uniform at every n: both halves of the draw leave the same 64-bit finaliser and 2^32 = 4
    (mod 12) makes the modulo's bias 1 part in 10^9.  No margin and no joint across keys sees it (65,536 keys, seed 7, statistic against
    its 0.999 quantile: 12-cell margin 12.8 / 31.4, PIT margin 10.1 / 37.8, PIT turn t x t + 1 17.3 / 28.1, PIT env g x g + 1 13.1 / 28.1,
    even the low-half draw x the rule's draw of the same key, 12 x 12: 115.2 / 174.9): those statistics alone were not sharp enough.
    What tells it from the rule is the joint of the draws of ONE key at two totals (ds.quantisation_joint_stat): the rule's k = floor(v n)
    makes (k at 12, k at 16) the two quantisations of one variate, 24 possible cells of 192; `low half % n` fills the 48 cells with
    k12 = k16 (mod 4) instead.  The rule passes it here, on so_sample_action (test_action_draws_of_the_oracle) and on sgx_sample_valid
    (tests/test_gpu_draws.py)."""
    zeros = ds.np_rng_below(ds.np_rng(7, G, 0, ds.STREAM_ACTION, 10) & np.uint64(0xFFFFFFFF), 12)
    _rejected('rng_below handed the low half', ds.chi2_uniform(zeros, 12))
    rs = np.random.RandomState(5)
    totals = np.full((N, 4), 12)

    def low(r, total):
        return ((r & np.uint64(0xFFFFFFFF)) % np.asarray(total).astype(np.uint64)).astype(np.int64)
    r = ds.np_rng(7, G, 0, ds.STREAM_ACTION, 10)
    k_low, k_rule = low(r, 12), ds.np_rng_below(r, 12)
    blind = dict(ds.action_stats(_np_actions(7, 0, totals, rs, below=low)))
    blind['12-cell margin'] = ds.chi2_uniform(k_low, 12)
    blind['low-half draw x the rule\'s draw'] = ds.chi2_independence(ds.two_way(k_low, k_rule, 12, 12))
    for name, st in blind.items():
        ds.report('(blind to it) low half % 12, ' + name, st)
    ds.check('control: the rule at 12 and 16', ds.quantisation_joint_stat(k_rule, 12, ds.np_rng_below(r, 16), 16))
    _rejected('low half % n at 12 and 16', ds.quantisation_joint_stat(k_low, 12, low(r, 16), 16))
