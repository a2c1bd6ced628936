"""Statistics for the distribution tests of the on-device random draws (tests/test_draws_cpu.py, tests/test_gpu_draws.py).  Plain numpy,
test infrastructure only; never imported by the product package.

Every chi-squared is held below the 0.999 quantile for its degrees of freedom (tests/determinize_rule.chi2_quantile_999).  The RNG is a
counter RNG, so every statistic is a fixed number for a fixed key: nothing here is flaky.

`np_rng` / `np_rng_below` restate the counter RNG for arrays of keys.  tests/test_draws_cpu.py holds them against the oracle's `so_rng` /
`so_rng_below`; the deliberately broken samplers of the teeth test are variations of them."""
import numpy as np

from tests.determinize_rule import chi2_quantile_999

MIN_EXPECTED = 5.0
SEEDS = (0, 1, 7, 0xC0FFEE)                      # the keys of the GPU tests, fixed before any of them ran
OFFSETS = (0, 1 << 20, 1 << 40)
N_KEYS = 65536

STREAM_SETUP, STREAM_ACTION, STREAM_SHUFFLE_P1, STREAM_SHUFFLE_P2, STREAM_POOL, STREAM_DETERMINIZE, STREAM_PLAYOUT = range(7)

_M64 = (1 << 64) - 1


# ---- the counter RNG for arrays of keys ----------------------------------------------------------------------------------------------
def _u64(x):
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.asarray(int(x) & _M64, dtype=np.uint64)


def _sm_fin(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_rng(seed, g, j, stream, t):
    """sgx_rng / so_rng for arrays: every argument an int or an integer array (broadcast); -> uint64 array."""
    with np.errstate(over='ignore'):
        seed, g, j, stream, t = (np.atleast_1d(_u64(x)) for x in (seed, g, j, stream, t))
        h = _sm_fin(seed + np.uint64(0x9E3779B97F4A7C15) * (g + np.uint64(1)))
        ctr = (stream << np.uint64(32)) | (t & np.uint64(0xFFFFFFFF))
        return _sm_fin(h ^ (j * np.uint64(0xD1B54A32D192ED03) + ctr * np.uint64(0x8CB92BA72F3D8DD7) + np.uint64(0x2545F4914F6CDD1D)))


def np_rng_below(r, n):
    """rng_below / so_rng_below for arrays: the high half of the draw scaled into [0, n)."""
    return (((_u64(r) >> np.uint64(32)) * _u64(n)) >> np.uint64(32)).astype(np.int64)


def np_shuffle(seed, g, j, stream, n, bound=1):
    """The Fisher-Yates of the random placement for arrays of keys -> int64 [len(g), n], row = the shuffled list loc[] of cells.
    bound=1 is the rule (swap loc[i] with loc[rng_below(r, i + 1)]); bound=0 draws below i: Sattolo's algorithm, a broken sampler."""
    g = np.atleast_1d(np.asarray(g))
    rows = np.arange(len(g))
    loc = np.tile(np.arange(n, dtype=np.int64), (len(g), 1))
    for i in range(n - 1, 0, -1):
        k = np_rng_below(np_rng(seed, g, j, stream, i), i + bound)
        a, b = loc[rows, i].copy(), loc[rows, k].copy()
        loc[rows, i], loc[rows, k] = b, a
    return loc


def placement_maps(loc, piece_counts):
    """loc int64 [N, n] -> the own-side map over the n setup cells, int64 [N, n]: pieces in piece-code order go to loc[0], loc[1], ..."""
    types = np.repeat(np.arange(1, 13), np.asarray(piece_counts))
    maps = np.zeros(loc.shape, dtype=np.int64)
    rows = np.arange(loc.shape[0])
    for q, t in enumerate(types):
        maps[rows, loc[:, q]] = t
    return maps


# ---- chi-squared ---------------------------------------------------------------------------------------------------------------------
def merge_cells(observed, expected, min_expected=MIN_EXPECTED):
    """Merge cells, smallest expectation first, until every expectation is >= min_expected -> (observed, expected) of the merged cells.
    A cell with expectation 0 must be empty; it is dropped (an observation in it makes the statistic infinite: chi2_fit)."""
    o = np.asarray(observed, dtype=np.float64).reshape(-1)
    e = np.asarray(expected, dtype=np.float64).reshape(-1)
    order = np.argsort(e, kind='stable')
    mo, me, co, ce = [], [], 0.0, 0.0
    for i in order:
        co, ce = co + o[i], ce + e[i]
        if ce >= min_expected:
            mo.append(co); me.append(ce)
            co = ce = 0.0
    if ce > 0 or co > 0:                                  # a tail below the minimum joins the last cell
        if not mo:
            mo.append(0.0); me.append(0.0)
        mo[-1] += co; me[-1] += ce
    return np.asarray(mo), np.asarray(me)


def chi2_fit(observed, expected):
    """Pearson chi-squared of a count table against expected counts (same total), cells merged until every expectation is >= 5
    -> (chi2, degrees of freedom, 0.999 quantile)."""
    o = np.asarray(observed, dtype=np.float64).reshape(-1)
    e = np.asarray(expected, dtype=np.float64).reshape(-1)
    assert o.shape == e.shape and abs(o.sum() - e.sum()) <= 1e-6 * max(1.0, e.sum()), "observed and expected counts of the same total"
    impossible = float(o[e <= 0].sum())
    o, e = merge_cells(o[e > 0], e[e > 0])
    df = len(e) - 1
    assert df >= 1, "a table of one cell tests nothing"
    chi2 = float((((o - e) ** 2) / e).sum())
    if impossible:
        chi2 = float('inf')
    return chi2, df, chi2_quantile_999(df)


def chi2_uniform(values, cells):
    """values: integers in [0, cells) -> chi2_fit of their counts against the uniform distribution."""
    values = np.asarray(values, dtype=np.int64).reshape(-1)
    counts = np.bincount(values, minlength=cells)
    assert len(counts) == cells
    return chi2_fit(counts, np.full(cells, len(values) / cells))


def two_way(a, b, na, nb):
    """Count table [na, nb] of the integer pairs (a, b)."""
    a, b = np.asarray(a, dtype=np.int64).reshape(-1), np.asarray(b, dtype=np.int64).reshape(-1)
    assert a.shape == b.shape and (a >= 0).all() and (a < na).all() and (b >= 0).all() and (b < nb).all()
    return np.bincount(a * nb + b, minlength=na * nb).reshape(na, nb)


def chi2_independence(table):
    """Pearson chi-squared of a two-way count table against the product of its margins.  Rows / columns are merged, smallest margin first,
    until every expectation is >= 5 -> (chi2, degrees of freedom (rows - 1)(columns - 1), 0.999 quantile)."""
    t = np.asarray(table, dtype=np.float64)
    assert t.ndim == 2
    t = t[t.sum(1) > 0][:, t.sum(0) > 0]
    while True:
        n, r, c = t.sum(), t.sum(1), t.sum(0)
        e = np.outer(r, c) / n
        if e.min() >= MIN_EXPECTED or (t.shape[0] <= 2 and t.shape[1] <= 2):
            break
        # the smallest margin, relative to its axis, is the one to merge into its next smallest neighbour
        merge_rows = t.shape[0] > 2 and (t.shape[1] <= 2 or r.min() / n <= c.min() / n)
        if not merge_rows:
            t = t.T
        m = t.sum(1)
        i, k = np.argsort(m, kind='stable')[:2]
        t[k] += t[i]
        t = np.delete(t, i, axis=0)
        if not merge_rows:
            t = t.T
    assert e.min() >= MIN_EXPECTED, "a two-way table this thin tests nothing (smallest expectation %.2f)" % e.min()
    df = (t.shape[0] - 1) * (t.shape[1] - 1)
    assert df >= 1, "a table with one row or one column tests nothing"
    return float((((t - e) ** 2) / e).sum()), df, chi2_quantile_999(df)


# ---- the randomised probability-integral transform -----------------------------------------------------------------------------------
def pit(k, total, rs):
    """Draw k of `total` equally likely values -> u = (k + U) / total with U from the host RandomState `rs`: exactly uniform on [0, 1)
    under a uniform draw, whatever `total` is."""
    k, total = np.asarray(k, dtype=np.float64), np.asarray(total, dtype=np.float64)
    assert (total >= 1).all() and (k >= 0).all() and (k < total).all()
    return (k + rs.random_sample(k.shape)) / total


def bins(u, n):
    """u in [0, 1) -> bin index in [0, n)."""
    return np.minimum((np.asarray(u) * n).astype(np.int64), n - 1)


def report(name, stat):
    """Print a statistic with its limit (like tests/test_determinize_cpu.py) and return (chi2, limit)."""
    chi2, df, limit = stat
    print("%s: chi2 %.1f, df %d (0.999 quantile %.1f), ratio %.2f" % (name, chi2, df, limit, chi2 / limit))
    return chi2, limit


def check(name, stat):
    chi2, limit = report(name, stat)
    assert chi2 < limit, (name, chi2, limit)
    return chi2


# ---- decoding draws from states ------------------------------------------------------------------------------------------------------
def table_rows(table):
    """The setup table uint8 [S, U*C] -> (canonical int64 [S]: the first row equal to row i, lookup {row bytes: canonical index}).  A row that
    occurs m times is drawn with probability m / S; its draws are all counted at its first occurrence."""
    lookup, canonical = {}, np.zeros(len(table), dtype=np.int64)
    for i, row in enumerate(np.ascontiguousarray(table, dtype=np.uint8)):
        canonical[i] = lookup.setdefault(row.tobytes(), i)
    return canonical, lookup


def setup_rows_from_maps(p1_rows, p2_rows, lookup):
    """Own-side back rows uint8 [N, U, C] of both players (row 0 = the player's own back row) -> the table rows (canonical) they came from:
    p1_map[r][c] = s1[(U-1-r)*C + c], p2_map[r][c] = s2[(U-1-r)*C + (C-1-c)]."""
    s1 = np.ascontiguousarray(np.asarray(p1_rows, dtype=np.uint8)[:, ::-1, :]).reshape(len(p1_rows), -1)
    s2 = np.ascontiguousarray(np.asarray(p2_rows, dtype=np.uint8)[:, ::-1, ::-1]).reshape(len(p2_rows), -1)
    return (np.asarray([lookup[r.tobytes()] for r in s1], dtype=np.int64), np.asarray([lookup[r.tobytes()] for r in s2], dtype=np.int64))


def own_side_rows(states01, usable_rows):
    """Layers 0 / 1 of reference-layout states, [N, 2, R, C] -> both players' own-side back rows [N, U, C] (player -1's board is the
    180 degree rotation of its own-side map: create_initial_state)."""
    s = np.asarray(states01)
    return s[:, 0, :usable_rows, :], s[:, 1, ::-1, ::-1][:, :usable_rows, :]


def setup_bin_expectation(canonical, n, n_bins=16):
    """Expected counts of `n` draws over `n_bins` equal ranges of the (canonical) table index."""
    S = len(canonical)
    return np.bincount(canonical * n_bins // S, minlength=n_bins) * (n / S)


def setup_bins(index, S, n_bins=16):
    return np.asarray(index, dtype=np.int64) * n_bins // S


def arrangement_ids(maps):
    """maps int [N, n] -> (id per row, number of distinct ids seen): every distinct arrangement gets a number in order of first appearance
    of its sorted byte string."""
    m = np.ascontiguousarray(np.asarray(maps, dtype=np.uint8))
    uniq, inv = np.unique(m, axis=0, return_inverse=True)
    return inv.reshape(-1), len(uniq)


def n_arrangements(piece_counts, n_cells):
    """Number of arrangements of the multiset of pieces (and empty cells) over n_cells."""
    from math import factorial
    counts = [int(c) for c in piece_counts if c] + [n_cells - int(sum(piece_counts))]
    out = factorial(n_cells)
    for c in counts:
        out //= factorial(c)
    return out


def cell_by_type_stat(maps, piece_counts):
    """maps int [N, n] own-side cells -> Pearson chi-squared of the cell x piece type table (type 0 = empty) against piece_counts / n per
    cell.  Every game puts one type on every cell and every piece on one cell, so both margins of the table are fixed: a cell's variance
    is N p (1 - p) with the multinomial's covariances on BOTH axes, the sum X has mean n (T - 1) for T types present, and X (n - 1) / n is
    chi-squared with (n - 1)(T - 1) degrees of freedom.  -> (X (n - 1) / n, df, 0.999 quantile)."""
    maps = np.asarray(maps, dtype=np.int64)
    N, n = maps.shape
    counts = np.stack([np.bincount(maps[:, c], minlength=13) for c in range(n)]).astype(np.float64)            # [n, 13]
    p = np.concatenate([[n - sum(piece_counts)], np.asarray(piece_counts, dtype=np.float64)]) / n
    assert counts[:, p == 0].sum() == 0, "a piece type the variant does not have"
    present = p > 0
    e = np.tile(p[present] * N, (n, 1))
    assert e.min() >= MIN_EXPECTED
    df = (n - 1) * (int(present.sum()) - 1)
    x = float((((counts[:, present] - e) ** 2) / e).sum()) * (n - 1) / n
    return x, df, chi2_quantile_999(df)


# ---- the composite statistics both test files use --------------------------------------------------------------------------------------
def setup_margin_stat(index, canonical):
    """Canonical table indices of N draws, binned into 16 equal ranges, against the table's own multiplicities."""
    return chi2_fit(np.bincount(setup_bins(index, len(canonical)), minlength=16), setup_bin_expectation(canonical, len(index)))


def setup_joint_stat(index_a, index_b, S):
    """16 x 16 joint of two binned table indices against the product of its margins."""
    return chi2_independence(two_way(setup_bins(index_a, S), setup_bins(index_b, S), 16, 16))


def pit_margin_stat(u):
    return chi2_uniform(bins(u, 16), 16)


def pit_pair_stat(u_a, u_b):
    """4 x 4 joint of two PIT values against the product of its margins."""
    return chi2_independence(two_way(bins(u_a, 4), bins(u_b, 4), 4, 4))


def quantisation_joint_stat(k_a, n_a, k_b, n_b):
    """The draws of ONE key below n_a and below n_b.  The rule takes both from the high half of the same draw, k = floor(v n), so the pair is
    the two quantisations of one uniform variate v: with L = lcm(n_a, n_b), segment s of L equal segments of [0, 1) gives the cell
    (s n_a // L, s n_b // L) with probability 1 / L (several segments may share a cell), and every other cell of the n_a x n_b table is impossible.  -> chi2_fit of the
    joint table against that.  (A sampler that is uniform at every n but takes the draw another way -- the low half, a modulo -- has the
    right margins and the wrong joint.)"""
    L = int(np.lcm(n_a, n_b))
    k_a = np.asarray(k_a).reshape(-1)
    expected = np.zeros((n_a, n_b))
    for s in range(L):
        expected[s * n_a // L, s * n_b // L] += len(k_a) / L
    return chi2_fit(two_way(k_a, k_b, n_a, n_b), expected)


def first_valid_mask(n_rows, n_actions, total):
    """uint8 [n_rows, n_actions] with the first `total` actions valid: the rank of a drawn action is the action itself."""
    m = np.zeros((n_rows, n_actions), dtype=np.uint8)
    m[:, :total] = 1
    return m


def ranks_in_masks(mask, actions):
    """mask [N, A] (non-zero = valid), actions int [N] -> (k: the rank of the action among the valid ones, total, valid: the action is in
    the mask) as int64 / bool arrays [N]."""
    m = np.asarray(mask).reshape(len(actions), -1) != 0
    a = np.asarray(actions, dtype=np.int64)
    rows = np.arange(len(a))
    inside = (a >= 0) & (a < m.shape[1])
    safe = np.where(inside, a, 0)
    total = m.sum(1).astype(np.int64)
    k = np.cumsum(m, axis=1)[rows, safe].astype(np.int64) - 1
    return k, total, inside & m[rows, safe]


def placement_stats(piece_counts, m1, m2, tag=''):
    """The statistics of a random placement: own-side maps int [N, n] of both players -> {name: (chi2, df, limit)}."""
    n = m1.shape[1]
    out = {tag + 'cells x types +1': cell_by_type_stat(m1, piece_counts), tag + 'cells x types -1': cell_by_type_stat(m2, piece_counts),
           tag + 'flag +1 x flag -1': chi2_independence(two_way(np.argmax(m1 == 11, axis=1), np.argmax(m2 == 11, axis=1), n, n))}
    return out


def arrangement_stat(piece_counts, maps):
    """maps int [N, n] -> (arrangements seen, arrangements there are, chi2_fit of their counts against the uniform distribution)."""
    worlds = n_arrangements(piece_counts, maps.shape[1])
    ids, seen = arrangement_ids(maps)
    counts = np.concatenate([np.bincount(ids), np.zeros(worlds - seen)])
    return seen, worlds, chi2_fit(counts, np.full(worlds, len(maps) / worlds))


def pool_stats(rows, first, n_pool, tag=''):
    """rows int [N, J], first (+1 / -1) [N, J]: the pool rows and first movers of J consecutive games of N envs."""
    out = {tag + 'pool row margin': chi2_uniform(rows, n_pool),
           tag + 'pool row of game j x game j + 1': chi2_independence(two_way(rows[:, :-1], rows[:, 1:], n_pool, n_pool)),
           tag + 'pool row x first mover': chi2_independence(two_way(rows, (first < 0).astype(np.int64), n_pool, 2)),
           tag + 'first mover against one half': chi2_uniform((first < 0).astype(np.int64), 2),
           tag + 'first mover of game j x game j + 1': chi2_independence(two_way(first[:, :-1] < 0, first[:, 1:] < 0, 2, 2))}
    return out


def action_stats(u, tag='', same_game=None):
    """u float [N, T]: the PIT of the action drawn at T consecutive steps of N envs (NaN where there is none); same_game bool [N, T - 1]:
    steps t and t + 1 belong to one game (None: all do)."""
    ok = ~np.isnan(u)
    pair_t = ok[:, :-1] & ok[:, 1:]
    if same_game is not None:
        pair_t &= np.asarray(same_game, dtype=bool)
    pair_g = ok[0::2] & ok[1::2]
    return {tag + 'PIT margin': pit_margin_stat(u[ok]),
            tag + 'PIT turn t x t + 1': pit_pair_stat(u[:, :-1][pair_t], u[:, 1:][pair_t]),
            tag + 'PIT env g x g + 1': pit_pair_stat(u[0::2][pair_g], u[1::2][pair_g])}
