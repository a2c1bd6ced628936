"""The leaf-value rule (tests/leaf_values_rule.py) against known answers worked by hand, its int32 headroom, the table builders of
stratego_env_amd.leaf_values and the host-side refusals of the Python layer.  No GPU: the device side is tests/test_gpu_leaf_values.py."""
import numpy as np
import pytest

from stratego_env_amd import leaf_values as lvb
from stratego_env_amd.config import VARIANTS
from stratego_env_amd.procedural_env import leaf_scale, leaf_table
from tests import leaf_values_rule as lv


def test_known_answers_in_both_views_for_both_players():
    s, T = lv.known_answer_state(), lv.known_answer_table()
    for see_all in (False, True):
        assert lv.scores(s, T, see_all) == lv.KNOWN_SCORES[see_all], see_all
        assert lv.batch_scores(s[None], T, see_all).tolist() == [list(lv.KNOWN_SCORES[see_all])]
    # the public view: the two values are each player's own estimate, not negatives of each other
    p1, m1 = lv.KNOWN_SCORES[False]
    assert p1 == 3907 and m1 == 3607
    v = lv.values(s[None], T, 1 << 20, 1 << 20)
    assert v.dtype == np.float32 and v.tobytes() == np.asarray([[3907 / 1048576, 3607 / 1048576]], dtype=np.float32).tobytes()


def test_the_perspective_turn_of_player_minus_one():
    """the same piece on the same ABSOLUTE cell is worth T[0][t][cell] to +1 and T[0][t][cells - 1 - cell] to -1"""
    T = np.zeros((2, 14, 9), dtype=np.int16)
    T[0, 5] = np.arange(9) * 7 + 1                     # asymmetric in the cell
    T[1, 13] = -(np.arange(9) * 11 + 3)
    for cell in range(9):
        s = np.zeros((34, 3, 3), dtype=np.int64)
        s.reshape(34, 9)[0, cell] = 5
        s.reshape(34, 9)[3, cell] = 13
        # +1 owns it: mine(+1) at `cell`; -1 sees an unknown piece of +1's at +1's perspective cell = `cell`
        assert lv.scores(s, T) == (7 * cell + 1, 11 * cell + 3)
        s = np.zeros((34, 3, 3), dtype=np.int64)
        s.reshape(34, 9)[1, cell] = 5
        s.reshape(34, 9)[4, cell] = 13
        assert lv.scores(s, T) == (11 * (8 - cell) + 3, 7 * (8 - cell) + 1)
        assert lv.scores(s, T, see_all=True) == (0, 7 * (8 - cell) + 1)        # row T[1][5] is zero


def test_rows_never_read():
    s, T = lv.known_answer_state(), lv.known_answer_table().copy()
    want = {v: lv.scores(s, T, v) for v in (False, True)}
    T[:, 0] = 12345
    T[0, 13] = -12345
    for v in (False, True):
        assert lv.scores(s, T, v) == want[v] and tuple(lv.batch_scores(s[None], T, v)[0]) == want[v]


def test_the_clamp_and_limit_equal_denom():
    s, T = lv.known_answer_state(), lv.known_answer_table()
    # S = (3907, 3607): below, at and above the limit; one float32 division
    assert lv.values(s[None], T, 3907, 4000).tolist() == [[np.float32(3907) / np.float32(4000), np.float32(3607) / np.float32(4000)]]
    assert lv.values(s[None], T, 3700, 4000).tolist() == [[np.float32(3700) / np.float32(4000), np.float32(3607) / np.float32(4000)]]
    assert lv.values(s[None], T, 100, 100).tolist() == [[1.0, 1.0]]                       # limit = denom: a leaf may reach a win's value
    assert lv.values(s[None], -T.astype(np.int64), 100, 100).tolist() == [[-1.0, -1.0]]
    assert lv.values(s[None], T, 1, 1 << 24).tolist() == [[2.0 ** -24, 2.0 ** -24]]
    # apply: only the rows of slots that are not over change
    reward = np.asarray([[1, -1], [0, 0], [1e-4, 1e-4]], dtype=np.float32)
    got = lv.apply(reward, [1, 0, 1], np.stack([s, s, s]), T, 3700, 4000)
    assert got[0].tolist() == [1, -1] and got[2].tobytes() == reward[2].tobytes()
    assert got[1].tolist() == [np.float32(3700) / np.float32(4000), np.float32(3607) / np.float32(4000)]


def test_int32_headroom_at_1024_cells():
    """every cell holds a piece of each side's layers and every entry is extreme: |S| = 2 * 1024 * 32768 = 2^26 fits int32"""
    s = np.zeros((34, 32, 32), dtype=np.int64)
    s[0] = 3; s[1] = 4; s[3] = 13; s[4] = 13
    T = np.zeros((2, 14, 1024), dtype=np.int16)
    T[0] = -32768
    T[1] = 32767
    for see_all in (False, True):
        sc = lv.batch_scores(s[None], T, see_all)
        assert sc.tolist() == [[-1024 * 32768 - 1024 * 32767] * 2]
        assert abs(int(sc[0, 0])) < 1 << 31
    T[0], T[1] = 32767, -32768
    assert lv.scores(s, T) == (1024 * 32767 + 1024 * 32768,) * 2
    assert lv.values(s[None], T, 1 << 24, 1 << 24).tolist() == [[1.0, 1.0]]


def test_the_batch_form_is_the_definition():
    rs = np.random.RandomState(4)
    n, R, C = 12, 4, 5
    s = np.zeros((n, 34, R, C), dtype=np.int64)
    for l, hi in ((0, 13), (1, 13), (3, 14), (4, 14)):
        s[:, l] = rs.randint(0, hi, size=(n, R, C)) * (rs.rand(n, R, C) < 0.5)
    T = (rs.permutation(65536)[:2 * 14 * R * C] - 32768).astype(np.int16).reshape(2, 14, R * C)
    for see_all in (False, True):
        assert lv.batch_scores(s, T, see_all).tolist() == [list(lv.scores(x, T, see_all)) for x in s]


def test_material_builder():
    v = VARIANTS['barrage']
    t = lvb.material('barrage')
    assert t.shape == (2, 14, 100) and t.dtype == np.int16
    vals = np.asarray(lvb.DEFAULT_VALUES)
    assert (t[0, 1:13] == vals[1:, None]).all() and (t[1, 1:13] == vals[1:, None]).all()
    assert (t[:, 0] == 0).all() and (t[0, 13] == 0).all()
    mean = int(np.rint(sum(n * vals[k] for k, n in enumerate(v.piece_counts, start=1)) / sum(v.piece_counts)))
    assert (t[1, 13] == mean).all()
    assert lvb.side_total('barrage') == sum(n * vals[k] for k, n in enumerate(v.piece_counts, start=1))
    assert (lvb.material(v, unknown=7)[1, 13] == 7).all()
    custom = lvb.material('fives', values=list(range(13)))
    assert (custom[0, 1:13, 3] == np.arange(1, 13)).all()
    with pytest.raises(ValueError):
        lvb.material('fives', values=[1.5] * 13)
    with pytest.raises(ValueError):
        lvb.material('fives', values=[0] * 11 + [40000, 0])
    # a side that has lost nothing and sees nothing of the other is worth the difference of total and unknown-mean, on any state
    s = np.zeros((34, 10, 10), dtype=np.int64)
    s[0, 0, :8] = [11, 10, 9, 3, 2, 2, 1, 12]
    s[3, 0, :8] = 13
    sc = lv.scores(s, t)
    assert sc == (lvb.side_total('barrage'), -8 * mean)


def test_advance_and_piece_square_builders():
    base = lvb.material('fives')
    t = lvb.with_advance(base, 3)
    rows = np.arange(25) // 5
    assert (t[0, 1:11] - base[0, 1:11] == 3 * rows).all() and (t[1, 1:11] - base[1, 1:11] == 3 * rows).all()
    assert (t[1, 13] - base[1, 13] == 3 * rows).all()
    assert (t[:, 11:13] == base[:, 11:13]).all() and (t[:, 0] == 0).all() and (t[0, 13] == 0).all()
    wide = lvb.with_advance(lvb.material('micro'), 2, rows=3)                  # 3 x 4: not square
    assert (wide[0, 2] - lvb.material('micro')[0, 2] == 2 * (np.arange(12) // 4)).all()
    with pytest.raises(ValueError):
        lvb.with_advance(lvb.material('micro'), 2)                             # sqrt(12) does not divide
    with pytest.raises(ValueError):
        lvb.with_advance(base, 20000)
    # a scout that advances is worth more to its owner, whoever the owner is: the perspective turn
    for layer, cell_far, cell_near in ((0, 22, 2), (1, 2, 22)):
        far, near = np.zeros((34, 5, 5), dtype=np.int64), np.zeros((34, 5, 5), dtype=np.int64)
        far.reshape(34, 25)[layer, cell_far] = 2
        near.reshape(34, 25)[layer, cell_near] = 2
        col = 0 if layer == 0 else 1
        assert lv.scores(far, t)[col] - lv.scores(near, t)[col] == 3 * 4
    mine, theirs = np.arange(12 * 9).reshape(12, 9), -np.arange(13 * 9).reshape(13, 9)
    ps = lvb.from_piece_square(mine, theirs)
    assert (ps[0, 1:13] == mine).all() and (ps[1, 1:14] == theirs).all() and (ps[:, 0] == 0).all() and (ps[0, 13] == 0).all()
    assert (lvb.from_piece_square(mine, theirs[:12])[1, 13] == 0).all()
    for bad in ((mine[:11], theirs), (mine, theirs[:, :8]), (mine.astype(float), theirs), (mine * 1000, theirs)):
        with pytest.raises(ValueError):
            lvb.from_piece_square(*bad)


def test_python_side_refusals():
    good = np.zeros((2, 14, 25), dtype=np.int64)
    assert leaf_table(good, 25).dtype == np.int16 and leaf_table(good, 25).flags['C_CONTIGUOUS']
    import torch
    assert leaf_table(torch.zeros((2, 14, 25), dtype=torch.int32), 25).shape == (2, 14, 25)
    for bad in (np.zeros((2, 14, 24), dtype=np.int64), np.zeros((2, 13, 25), dtype=np.int64), np.zeros((14, 25), dtype=np.int64),
                np.zeros((2, 14, 25), dtype=np.float32)):
        with pytest.raises(ValueError):
            leaf_table(bad, 25)
    for v in (32768, -32769):
        t = good.copy()
        t[1, 13, 24] = v
        with pytest.raises(ValueError) as ei:
            leaf_table(t, 25)
        assert 'table[1][13][24]' in str(ei.value)
    t = good.copy()
    t[0, 0, 0], t[1, 1, 1] = 32767, -32768
    assert leaf_table(t, 25)[0, 0, 0] == 32767 and leaf_table(t, 25)[1, 1, 1] == -32768
    assert leaf_scale(1, 1) == (1, 1) and leaf_scale(5, 1 << 24) == (5, 1 << 24)
    for limit, denom in ((0, 1), (2, 1), (1, 0), (1, (1 << 24) + 1), (-1, 5)):
        with pytest.raises(ValueError):
            leaf_scale(limit, denom)
