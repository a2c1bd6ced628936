"""Belief-weighted determinization (sgx_determinize_weighted) without a GPU: the binding, the numpy restatement of the rule
(tests/determinize_weighted_rule.py, what the device kernel is held to bit for bit in tests/test_gpu_determinize_weighted.py) against the
oracle's rules and the consequences the header promises, its exact distribution, and the tables of stratego_env_amd.beliefs."""
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib, beliefs as bl, setups as S
from stratego_env_amd.config import VARIANTS
from tests import determinize_weighted_rule as wr
from tests.helpers import _blank_state, _put
from tests.pool_roots import fives_position, sampled_states
from tests.tables import chi2_against, fives_samples, one_hot_truth, skewed_fives_table, third_zero_belief

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAME_SETS = ['barrage', 'standard', 'standard2', 'octa_barrage', 'medium', 'fives', 'tiny', 'micro']      # every board size
DRAWS = (0, 1, 1 << 40)


def test_the_binding():
    from stratego_env_amd import build as hip_build
    assert 'sgx_determinize_weighted' in _lib.EXPORTED_SYMBOLS
    assert _lib.ABI_VERSION == 15 and _lib.BELIEF_WEIGHT_MAX == 4095
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    assert re.search(r'\bint sgx_determinize_weighted\(', hdr) and re.search(r'#define SGX_ABI_VERSION 15\b', hdr)
    assert re.search(r'#define SGX_BELIEF_WEIGHT_MAX 4095\b', hdr)
    layout = open(os.path.join(ROOT, 'stratego_env_amd', 'csrc', 'sgx_layout.h')).read()
    assert re.search(r'STREAM_DETERMINIZE_WEIGHTED = 7\b', layout) and wr.STREAM_DETERMINIZE_WEIGHTED == 7
    hip_build.build()
    L = _lib.load()
    assert L.sgx_abi_version() == 15
    assert len(L.sgx_determinize_weighted.argtypes) == 10
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message
    assert L.sgx_determinize_weighted(None, None, None, 0, None, 0, 0, None, None, None) == -1
    assert b'sgx_determinize_weighted' in L.sgx_last_error() and b'NULL' in L.sgx_last_error()


@pytest.mark.parametrize('name', GAME_SETS)
def test_the_rule_against_the_oracle(name):
    v = VARIANTS[name]
    cells = v.rows * v.columns
    ru = orc.OracleRules(v.rows, v.columns)
    states = sampled_states(name, n_games=2, every=7)
    assert len(states) >= 4
    table = third_zero_belief(cells, seed=11)
    changed = fell_back = 0
    for si, (st, mover) in enumerate(states):
        truth = one_hot_truth(st)
        for observer in (1, -1, 0):
            o = observer if observer else mover
            opp = 1 if o == 1 else 0
            pobs = ru.get_partially_observable_observation_extended_channels(st, o)
            mask = ru.get_valid_moves_as_1d_mask(st, o)
            hid = (st[opp] != 0) & (st[3 + opp] == 13)
            for draw in DRAWS:
                out, hidden, off = wr.determinize_weighted(st, mover, observer, table, seed=0x5EED, g=si, draw=draw)
                where = (name, si, observer, draw)
                keep = [l for l in range(34) if l != opp]
                assert np.array_equal(out[keep], st[keep]), where                                     # only pieces[opp] changes
                assert hidden == int(hid.sum()), where
                assert np.array_equal(out[opp][~hid], st[opp][~hid]), where
                assert sorted(out[opp][hid].tolist()) == sorted(st[opp][hid].tolist()), where       # the multiset is preserved
                assert not np.any(np.isin(out[opp], (11, 12)) & hid & (st[32 + opp] == 0)), where    # flag / bombs on never-moved cells
                w = np.minimum(table[opp].astype(np.int64), 4095)
                flat = out[opp].reshape(-1)
                zero_pairs = sum(1 for c in np.flatnonzero(hid.reshape(-1)) if w[flat[c] - 1][c] == 0)
                assert off == zero_pairs, where                                                       # off_belief = dealt (t, cell) pairs of weight 0
                assert ru.get_partially_observable_observation_extended_channels(out, o).tobytes() == pobs.tobytes(), where
                assert ru.get_valid_moves_as_1d_mask(out, o).tobytes() == mask.tobytes(), where
                changed += int(not np.array_equal(out[opp], st[opp]))
                fell_back += off
            # the table that is one-hot on the truth returns the state
            out, hidden, off = wr.determinize_weighted(st, mover, observer, truth, seed=1, g=si, draw=3)
            assert np.array_equal(out, st) and off == 0 and hidden == int(hid.sum()), (name, si, observer)
    assert changed > 0                       # (the deal does something)
    if name in ('barrage', 'standard', 'octa_barrage'):
        assert changed > len(states) and fell_back > 0


def test_a_zero_weight_is_never_taken_next_to_a_positive_one():
    """Every draw of every deal, re-walked: the instance sequence is public, so the test can replay free / candidates from the result."""
    st, _ = fives_position()
    table = skewed_fives_table()
    w = table[1].astype(np.int64)
    for g in range(400):
        out, hidden, off = wr.determinize_weighted(st, 1, 1, table, 9, g, 0)
        flat = out[1].reshape(-1)
        free = [0, 1, 2, 3, 9]
        zero_taken = 0
        for t in (11, 7, 6, 5, 4):
            cell = [c for c in free if flat[c] == t][0]
            cand = [c for c in free if c != 9] if t == 11 else free
            if w[t - 1][cell] == 0:
                assert all(w[t - 1][c] == 0 for c in cand), (g, t)
                zero_taken += 1
            free.remove(cell)
        assert zero_taken == off


def test_a_flag_or_bomb_on_a_moved_hidden_cell_is_refused():
    for bad_type in (11, 12):
        for observer in (1, -1):
            st = _blank_state(5, 5, 60, 4)
            opp = -observer
            _put(st, opp, 0, 0, 4)
            _put(st, opp, 0, 1, 5)
            _put(st, opp, 2, 2, bad_type, moved=True)
            _put(st, opp, 0, 3, 11 if bad_type == 12 else 6)
            _put(st, observer, 4, 0, 11)
            _put(st, observer, 4, 1, 7, moved=True)
            out, hidden, off = wr.determinize_weighted(st, observer, observer, third_zero_belief(25), 0, 0, 5)
            assert hidden == -1 and off == 0 and np.array_equal(out, st)


def test_the_batch_form_indexes_tables_by_source_record():
    states = sampled_states('fives', n_games=1, every=3)[:4]
    st = np.stack([s for s, _ in states])
    movers = np.asarray([m for _, m in states])
    tables = third_zero_belief(25, seed=2, shape=(4, 2, 12, 25))
    idx = np.asarray([3, 0, 3, 1, 2, 2])
    out, hidden, off = wr.determinize_weighted_batch(st, movers, 0, tables, 5, 100, 2, idx)
    for i, s in enumerate(idx):
        w1, h1, o1 = wr.determinize_weighted(st[s], int(movers[s]), 0, tables[s], 5, 100 + i, 2)
        assert np.array_equal(out[i], w1) and hidden[i] == h1 and off[i] == o1
    out2, _, _ = wr.determinize_weighted_batch(st, movers, 0, tables[1], 5, 100, 2, idx)          # one table for all
    assert np.array_equal(out2[3], out[3]) and not np.array_equal(out2, out)


# ---- the distribution ------------------------------------------------------------------------------------------------------------------
def test_the_vectorised_sampler_is_the_rule():
    st, _ = fives_position()
    for kind in ('constant', 'skewed'):
        table = np.full((2, 12, 25), 7, dtype=np.uint16) if kind == 'constant' else skewed_fives_table()
        layers, off = fives_samples(kind)
        for g in list(range(300)) + [4097, 65535]:
            out, hidden, o1 = wr.determinize_weighted(st, 1, 1, table, 0, g, 0)
            assert hidden == 5 and np.array_equal(out[1].reshape(-1), layers[g]) and o1 == off[g], (kind, g)


def test_a_constant_table_samples_uniformly():
    """65,536 samples of the 96 worlds of the Fives position; Pearson's chi-squared against uniform must stay below the 0.999 quantile
    for 95 degrees of freedom (143.4).  The RNG is a counter RNG, so the statistic is a fixed number.  Obtained: 101.5, every world seen."""
    st, worlds = fives_position()
    layers, off = fives_samples('constant')
    probs = wr.world_probabilities(st, 1, 1, np.full((2, 12, 25), 7, dtype=np.uint16))
    assert len(probs) == worlds >= 90 and all(p == probs[next(iter(probs))] for p in probs.values())       # the rule IS uniform
    assert sum(probs.values()) == 1
    stat, df, pooled, impossible = chi2_against(layers, probs)
    limit = wr.chi2_quantile_999(df)
    print("constant table: %d worlds, chi2 %.1f (0.999 quantile for %d degrees of freedom %.1f)" % (len(probs), stat, df, limit))
    assert df == worlds - 1 and pooled == 0 and impossible == 0
    assert len({row.tobytes() for row in layers}) == worlds
    assert stat < limit
    assert int(off.sum()) == 0


def test_a_skewed_table_samples_the_exact_distribution():
    """The same 65,536 slots with skewed_fives_table(): chi-squared against world_probabilities (exact fractions), every world of expected
    count >= 5 a cell, the rest pooled into one cell that may hold at most 5 % of the mass; a world of probability 0 is never seen.
    Obtained: 46 worlds of probability > 0, 32 of them with an expected count >= 5, the other 14 (0.04 % of the mass: the flag on the cell
    of weight 1 in 1,101) pooled; chi-squared 24.6 against the 0.999 quantile 62.6 for 32 degrees of freedom."""
    st, worlds = fives_position()
    table = skewed_fives_table()
    layers, off = fives_samples('skewed')
    probs = wr.world_probabilities(st, 1, 1, table)
    assert sum(probs.values()) == 1
    assert 10 <= len(probs) < worlds                        # the zeros rule worlds out
    stat, df, pooled, impossible = chi2_against(layers, probs)
    limit = wr.chi2_quantile_999(df)
    print("skewed table: %d possible worlds, %d degrees of freedom, pooled mass %.4f, chi2 %.1f (0.999 quantile %.1f)"
          % (len(probs), df, pooled, stat, limit))
    assert impossible == 0
    assert pooled <= 0.05
    assert df >= 10
    assert stat < limit
    # the 4 is dealt last onto the one cell that is left: its weight there is 0 in this table, and off_belief says so for every world
    assert bool((off == 1).all())


# ---- stratego_env_amd.beliefs ------------------------------------------------------------------------------------------------------------
def test_uniform_and_from_probabilities():
    for name in ('barrage', 'fives', 'standard2'):
        v = VARIANTS[name]
        u = bl.uniform(name)
        assert u.shape == (2, 12, v.rows * v.columns) == bl.shape(name) and u.dtype == np.uint16 and bool((u == 1).all())
    p = np.zeros((3, 2, 12, 9))
    p[0, 0, 0, :4] = [1.0, 0.5, 1e-9, 0.0]                 # max -> 4095; half of it -> 2047.5 -> 2048 (halves up); tiny stays 1; 0 stays 0
    p[0, 1, 5, 2] = 0.25                                   # every [12, cells] block is scaled on its own
    p[1, 0, 11, 8] = 4095.0                                # (a scale of exactly 1: the halves below are exact in floating point)
    p[1, 0, 2, 1] = 1000.25                                # -> 1000
    p[1, 0, 2, 2] = 1000.5                                 # -> 1001: halves go up
    w = bl.from_probabilities(p)
    assert w.shape == p.shape and w.dtype == np.uint16
    assert w[0, 0, 0, :4].tolist() == [4095, 2048, 1, 0]
    assert w[0, 1, 5, 2] == 4095 and w[1, 0, 11, 8] == 4095
    assert w[1, 0, 2, 1] == 1000 and w[1, 0, 2, 2] == 1001
    assert int(w[2].max()) == 0 and int(w[1, 1].max()) == 0                  # a block of zeros stays zeros
    assert int(w.max()) <= bl.WEIGHT_MAX and np.array_equal(w > 0, p > 0)
    rs = np.random.RandomState(0)
    q = rs.random_sample((2, 12, 100)) * (rs.random_sample((2, 12, 100)) < 0.7)
    wq = bl.from_probabilities(q)
    assert np.array_equal(wq > 0, q > 0) and int(wq[0].max()) == 4095 and int(wq[1].max()) == 4095
    assert np.abs(wq[0].astype(np.float64) - np.maximum(q[0] / q[0].max() * 4095, (q[0] > 0) * 1.0)).max() <= 0.5 + 1e-9      # the nearest integer, or lifted to 1
    for bad in (np.full((2, 12, 9), -1.0), np.full((2, 12, 9), np.nan), np.zeros((2, 11, 9)), np.zeros((12, 9))):
        with pytest.raises(ValueError):
            bl.from_probabilities(bad)


@pytest.mark.parametrize('name', ['barrage', 'standard'])
def test_setup_prior_counts_what_the_oracle_deals(name):
    """beliefs.setup_counts against every row of the shipped table run through the oracle's game creation (row i dealt to both players),
    and setup_prior's scaling, fill and zeros."""
    v = VARIANTS[name]
    R, C, U = v.rows, v.columns, v.initial_state_usable_rows
    cells = R * C
    table = S.load_setup_table(name)
    ru = orc.OracleRules(R, C)
    ob = v.obstacle_map().astype(np.int64)
    want = np.zeros((2, 13, cells), dtype=np.int64)
    ar = np.arange(cells)
    for row in table:
        m1, m2 = S.own_side_maps(row, row, R, C, U)
        st = ru.create_initial_state(ob, m1, m2, v.max_turns)
        for p in range(2):
            want[p, st[p].reshape(-1), ar] += 1
    counts = bl.setup_counts(name)
    assert counts.shape == (2, 12, cells) and np.array_equal(counts, want[:, 1:])
    assert int(counts.sum()) == 2 * len(table) * int(sum(v.piece_counts))
    prior = bl.setup_prior(name)
    assert prior.shape == (2, 12, cells) and prior.dtype == np.uint16 and int(prior.max()) == 4095
    for p in range(2):
        inside = np.zeros(cells, dtype=bool)
        inside[:U * C] = True
        if p == 1:
            inside = inside[::-1]
        top = int(counts[p].max())
        scaled = (2 * 4095 * counts[p] + top) // (2 * top)
        scaled = np.where(counts[p] > 0, np.maximum(scaled, 1), 0)
        assert int(counts[p][:, ~inside].sum()) == 0                        # nobody sets up outside the setup rows
        assert np.array_equal(prior[p][:, inside], scaled[:, inside])
        assert int(prior[p].max()) == 4095
        assert int(prior[p][10:, ~inside].max()) == 0                       # flag and bomb: weight 0 outside the setup rows
        for t in range(1, 11):
            mean = max(1, int(np.floor(scaled[t - 1, inside].sum() / inside.sum() + 0.5)))
            assert bool((prior[p][t - 1, ~inside] == mean).all()), (p, t)
    # player -1's string is mirrored left to right before its side is turned by 180 degrees: what is left is the board flipped top to bottom
    assert np.array_equal(prior[1].reshape(12, R, C)[:, ::-1, :], prior[0].reshape(12, R, C))
