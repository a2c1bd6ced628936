"""Boards and setup tables the tests share (support code, no tests): the test-only variants of sizes and piece counts the reference has no
variant for, the setup table of a variant, and an int64 state from two setup maps."""
import numpy as np

from stratego_env_amd import config, setups as S
from stratego_env_amd.config import VARIANTS, custom_variant


def registered(variants):
    """The body of a test module's autouse fixture (`yield from registered(CUSTOM)`): the shared checkers look variants up by name, so
    the test-only names are in config.VARIANTS for the duration of a test (the product takes the Variant objects themselves)."""
    config.VARIANTS.update(variants)
    yield
    for k in variants:
        config.VARIANTS.pop(k, None)


#                                                        spy scout miner sgt lt cpt maj col gen mar flag bomb
CUSTOM = {
    'c3x3': custom_variant(3, 3, max_turns=24, piece_counts=(0, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0), name='c3x3'),
    'c7x7': custom_variant(7, 7, max_turns=150, obstacle_locations=((3, 1), (3, 5)),
                           piece_counts=(1, 2, 1, 0, 1, 1, 0, 1, 0, 1, 1, 2), initial_state_usable_rows=2, name='c7x7'),
    'c9x5': custom_variant(9, 5, max_turns=200, obstacle_locations=((4, 2),),
                           piece_counts=(1, 3, 2, 1, 1, 1, 1, 0, 1, 1, 1, 2), initial_state_usable_rows=3, name='c9x5'),
    'c12x12': custom_variant(12, 12, max_turns=300, obstacle_locations=((5, 2), (6, 2), (5, 3), (6, 3), (5, 8), (6, 8), (5, 9), (6, 9)),
                             piece_counts=(1, 8, 5, 4, 4, 4, 3, 2, 1, 1, 1, 6), initial_state_usable_rows=4, name='c12x12'),
    'c3x40': custom_variant(3, 40, max_turns=120, piece_counts=(1, 6, 2, 1, 1, 1, 1, 1, 1, 1, 1, 3), name='c3x40'),   # K = 83 > 64 lanes
    # more than 256 cells: 10-bit cell indices in the packed record (uint32 capture events, 6-bit recent-move codes), templates read from
    # global memory, records staged in a loop
    'c20x20': custom_variant(20, 20, max_turns=400, obstacle_locations=((9, 4), (10, 4), (9, 5), (10, 5), (9, 14), (10, 14), (9, 15), (10, 15)),
                             piece_counts=(1, 8, 5, 4, 4, 4, 3, 2, 1, 1, 1, 6), initial_state_usable_rows=3, name='c20x20'),
    'c32x32': custom_variant(32, 32, max_turns=250, obstacle_locations=((15, 7), (16, 7), (15, 24), (16, 24)),      # SGX_MAX_CELLS
                             piece_counts=(1, 8, 5, 4, 4, 4, 3, 2, 1, 1, 1, 6), initial_state_usable_rows=2, name='c32x32'),
    'c17x16': custom_variant(17, 16, max_turns=300, obstacle_locations=((8, 3), (8, 12)),
                             piece_counts=(1, 6, 3, 2, 2, 2, 2, 1, 1, 1, 1, 4), initial_state_usable_rows=2, name='c17x16'),
}


#                                                                    spy scout miner sgt lt cpt maj col gen mar flag bomb
MANY_PIECES = {
    'many66': custom_variant(6, 6, max_turns=120, piece_counts=(0, 9, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1), initial_state_usable_rows=2, name='many66'),
    'many88': custom_variant(8, 8, max_turns=160, obstacle_locations=((3, 2), (4, 5)), piece_counts=(1, 12, 2, 0, 0, 0, 0, 0, 0, 1, 1, 3),
                             initial_state_usable_rows=3, name='many88'),
}


def _board(name):
    """what the product takes for a board of these tests: the name of a variant of the main library, or the Variant of a test-only board"""
    return CUSTOM.get(name) or MANY_PIECES.get(name) or name


def _table(name):
    v = VARIANTS[name]
    return S.load_setup_table(v.human_inits) if v.human_inits else None


def _state_from_maps(name, m1, m2):
    from oracle import oracle as orc
    v = VARIANTS[name]
    ob = np.zeros((v.rows, v.columns), dtype=np.int64)
    for r, c in v.obstacle_locations:
        ob[r, c] = 1
    return orc.OracleRules(v.rows, v.columns).create_initial_state(ob, m1.astype(np.int64), m2.astype(np.int64), v.max_turns)
