"""Determinization (sgx_determinize) without a GPU: the numpy restatement of the rule (tests/determinize_rule.py, what the device
kernel is held to bit for bit in tests/test_gpu_determinize.py) checked against the oracle's rules along the golden games, its uniformity
over the consistent worlds, and the binding."""
import collections

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib
from stratego_env_amd import build as hip_build
from stratego_env_amd.config import VARIANTS
from tests import determinize_rule as dr
from tests.helpers import _blank_state, _put
from tests.pool_roots import fives_position, sampled_states

GAME_SETS = ['barrage', 'standard', 'octa_barrage', 'fives', 'micro']
DRAWS = (0, 1, 1 << 40)


@pytest.mark.parametrize('name', GAME_SETS)
def test_sampled_worlds_look_the_same_to_the_observer(name):
    v = VARIANTS[name]
    ru = orc.OracleRules(v.rows, v.columns)
    states = sampled_states(name)
    assert len(states) >= 6
    changed = 0
    for si, (st, mover) in enumerate(states):
        for observer in (1, -1, 0):
            o = observer if observer else mover
            opp = 1 if o == 1 else 0
            pobs = ru.get_partially_observable_observation_extended_channels(st, o)
            pobs_orig = ru.get_partially_observable_observation(st, o)
            mask = ru.get_valid_moves_as_1d_mask(st, o)
            for draw in DRAWS:
                out, hidden = dr.determinize(st, mover, observer, seed=0x5EED, g=si, draw=draw)
                where = (name, si, observer, draw)
                # every layer but the opponent's pieces is what it was
                keep = [l for l in range(34) if l != opp]
                assert np.array_equal(out[keep], st[keep]), where
                hid = (st[opp] != 0) & (st[3 + opp] == 13)
                assert hidden == int(hid.sum()), where
                assert np.array_equal(out[opp][~hid], st[opp][~hid]), where                          # revealed cells and empty cells untouched
                assert sorted(out[opp][hid].tolist()) == sorted(st[opp][hid].tolist()), where       # the same types, dealt again
                assert not np.any(np.isin(out[opp], (11, 12)) & hid & (st[32 + opp] == 0)), where    # no flag / bomb on a moved cell
                # the observer cannot tell the world from the real one: observation (extended and original channels) and valid moves
                assert ru.get_partially_observable_observation_extended_channels(out, o).tobytes() == pobs.tobytes(), where
                assert ru.get_partially_observable_observation(out, o).tobytes() == pobs_orig.tobytes(), where
                assert ru.get_valid_moves_as_1d_mask(out, o).tobytes() == mask.tobytes(), where
                changed += int(not np.array_equal(out[opp], st[opp]))
    assert changed > len(states)             # (the shuffle does something)


def test_observer_zero_is_the_mover_and_the_key_selects_the_world():
    st, mover = sampled_states('barrage', 1)[2]
    a, _ = dr.determinize(st, mover, 0, 7, 3, 0)
    b, _ = dr.determinize(st, mover, mover, 7, 3, 0)
    assert np.array_equal(a, b)
    worlds = {dr.determinize(st, mover, 1, seed, g, draw)[0][1].tobytes() for seed in (0, 1) for g in (0, 1, 2) for draw in (0, 1, 1 << 40)}
    assert len(worlds) > 6                  # seed, slot and draw all enter the key
    assert np.array_equal(dr.determinize(st, mover, 1, 7, 3, 5)[0], dr.determinize(st, mover, 1, 7, 3, 5)[0])


def test_inconsistent_states_are_returned_unchanged():
    R = C = 5
    for bad_type in (11, 12):
        for observer in (1, -1):
            st = _blank_state(R, C, 60, 4)
            opp = -observer
            _put(st, opp, 0, 0, 4)
            _put(st, opp, 0, 1, 5)
            _put(st, opp, 2, 2, bad_type, moved=True)          # a hidden flag / bomb on a moved cell: play cannot produce it
            _put(st, opp, 0, 3, 11 if bad_type == 12 else 6)
            _put(st, observer, 4, 0, 11)
            _put(st, observer, 4, 1, 7, moved=True)
            for draw in DRAWS:
                out, hidden = dr.determinize(st, observer, observer, 0, 0, draw)
                assert hidden == -1 and np.array_equal(out, st)
            # the same piece REVEALED is not hidden and does not make the state inconsistent
            st[3 + (0 if opp == 1 else 1), 2, 2] = bad_type
            out, hidden = dr.determinize(st, observer, observer, 0, 0, 0)
            assert hidden == 3


def barrage_like_position():
    """10 x 10, observer +1: seven hidden opponent pieces {1, 2, 2, 3, 9, flag, bomb}, five never moved and two moved:
    5 * 4 cells for flag and bomb, 5! / 2! ways for the rest = 1,200 worlds."""
    st = _blank_state(10, 10, VARIANTS['barrage'].max_turns, 40)
    for c, t in ((0, 11), (2, 2), (3, 12), (7, 9), (9, 1)):
        _put(st, -1, 0, c, t)
    _put(st, -1, 2, 4, 2, moved=True)
    _put(st, -1, 3, 8, 3, moved=True)
    _put(st, -1, 1, 1, 10, known=True, moved=True)             # a revealed piece takes no part
    for c, t in ((0, 11), (1, 12), (5, 10), (6, 2)):
        _put(st, 1, 9, c, t)
    return st, 1200


def chi2_over(st, worlds, keys):
    """Pearson chi-squared of the worlds sampled for `keys` = (seed, g, draw) triples against the uniform distribution over `worlds`."""
    counts = collections.Counter()
    for seed, g, draw in keys:
        out, hidden = dr.determinize(st, 1, 1, seed, g, draw)
        assert hidden > 0
        assert not np.any(np.isin(out[1], (11, 12)) & (st[33] == 0))
        counts[out[1].tobytes()] += 1
    n = sum(counts.values())
    e = n / worlds
    return len(counts), sum((c - e) ** 2 / e for c in counts.values()) + (worlds - len(counts)) * e


N_DRAWS = 65536


@pytest.mark.parametrize('case', ['fives_slots_seed0', 'fives_slots_seed1', 'fives_slots_seed7', 'fives_draws_seed3', 'barrage_like_slots_seed0'])
def test_the_rule_is_uniform_over_the_consistent_worlds(case):
    """65,536 samples each; every world must appear and Pearson's chi-squared must stay below the 0.999 quantile for worlds - 1 degrees of
    freedom (Wilson-Hilferty: 143.4 for 95, 1,356.1 for 1,199).  The RNG is a counter RNG, so the statistic is a fixed number.  Obtained:
      Fives (96 worlds), slots 0..65,535, draw 0:  seed 0: 94.7   seed 1: 83.9   seed 7: 89.9
      Fives, seed 3, slot 0, draws 0..65,535:      74.6
      Barrage-like (1,200 worlds), seed 0, slots:  1,216.6
    (the statistic depends on the order of the cell and type lists, not on where the cells are)."""
    if case.startswith('fives'):
        st, worlds = fives_position()
    else:
        st, worlds = barrage_like_position()
    if 'draws' in case:
        keys = [(3, 0, d) for d in range(N_DRAWS)]
    else:
        seed = int(case.rsplit('seed', 1)[1])
        keys = [(seed, g, 0) for g in range(N_DRAWS)]
    seen, chi2 = chi2_over(st, worlds, keys)
    limit = dr.chi2_quantile_999(worlds - 1)
    print("%s: %d of %d worlds, chi2 %.1f (0.999 quantile %.1f)" % (case, seen, worlds, chi2, limit))
    assert seen == worlds
    assert chi2 < limit


def test_wilson_hilferty_quantiles():
    # tabulated 0.999 quantiles: df 100: 149.449, df 1000: 1143.917 (the approximation is good to 0.1 % from a few dozen degrees on)
    assert abs(dr.chi2_quantile_999(100) - 149.449) < 0.15
    assert abs(dr.chi2_quantile_999(1000) - 1143.917) < 1.2


def test_the_library_exports_the_entry_point():
    assert 'sgx_determinize' in _lib.EXPORTED_SYMBOLS
    hip_build.build()
    L = _lib.load()
    assert hasattr(L, 'sgx_determinize')
    assert L.sgx_determinize.argtypes is not None and len(L.sgx_determinize.argtypes) == 7
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message
    assert L.sgx_determinize(None, None, None, 0, 0, None, None) != 0
    assert b'NULL' in L.sgx_last_error()
