"""tests/choose_rule.py checked without a GPU: that its acceptance set is the rule (equal logits against the oracle's sampler, the weights
against float64 softmax), that it is sharp enough to hold a kernel (the share of games with more than one acceptable answer, per case
the GPU file runs), that its random cases exercise exp2 at all, and that it rejects every broken rule of choose_rule.MUTANTS on the
same inputs the GPU tests feed the kernel.  Also the argument check of VecStrategoEnv.choose_actions, on plain descriptions."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from tests import choose_rule as cr

SEED, OFFSET = 99, 3
CPU_BOARDS = list(cr.BOARDS)


def _r64(n, salt):
    games, turns = cr.synthetic_keys(n, salt)
    return cr.draws(SEED, OFFSET, games, turns), games, turns


def _r32(r64):
    return [r >> 32 for r in r64]


def test_the_fused_multiply_add_is_rounded_once():
    """fma_x against exact rational arithmetic: random operands, and sums placed exactly half way between two float32 plus or minus a
    product too small for float64 to keep (where rounding the float64 sum again would go the wrong way)."""
    rs = np.random.RandomState(1)
    d = -np.abs(rs.standard_normal(4000) * 10).astype(np.float32)
    scales = np.asarray([1.4426950408889634, 28.853901, 0.20609929, 4.8e-39, 1.4426951e30], dtype=np.float32)
    mx = np.float32(0.0)
    ties = []
    for k in range(1, 200):                       # 23 - t with t = (2k + 1) * 2^-20: half way between two float32 of [16, 32) (ulp 2^-19)
        ties.append(-(2 * k + 1) * 2.0 ** -20)
    for scale in scales:
        x = cr.fma_x(d, mx, scale)
        for i in range(0, d.size, 7):
            exact = Fraction(float(d[i])) * Fraction(float(scale)) + 23
            want = _round_to_float32(exact)
            assert float(x[i]) == want, (float(d[i]), float(scale), float(x[i]), want)
    # products d * scale = tie * (1 +- 2^-40): d = tie (exact in float32), scale = 1 +- tiny is not a float32, so build them from factors
    for t in ties:
        for dd, sc in ((np.float32(t * 2.0 ** 30), np.float32(2.0 ** -30)), (np.float32(t), np.float32(1.0 + 2.0 ** -23)),
                       (np.float32(t), np.float32(1.0 - 2.0 ** -24))):
            x = cr.fma_x(np.asarray([dd], dtype=np.float32), mx, sc)
            want = _round_to_float32(Fraction(float(dd)) * Fraction(float(sc)) + 23)
            assert float(x[0]) == want, (t, float(dd), float(sc))


def _round_to_float32(q):
    """Round a Fraction to the nearest float32, ties to even, exactly."""
    if q == 0:
        return 0.0
    sign = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    k = a / ulp
    f = k.numerator // k.denominator
    rem = k - f
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and f % 2 == 1):
        f += 1
    return sign * float(f * ulp)


@pytest.mark.parametrize('board', ['micro', 'fives', 'medium', 'barrage'])
def test_equal_logits_are_the_uniform_sampler(board):
    """Equal logits: one acceptable answer, the floor(r32 * n_valid / 2^32)-th valid action -- so_sample_action's with the same key."""
    n = 64
    na = cr.n_actions(board)
    lg = cr.gen_logits(board, 'equal', n)
    r64, games, turns = _r64(n, 1)
    for fam in ('sparse', 'all', 'alternate', 'lone'):
        mask = cr.gen_mask(board, fam, n, SEED)
        for e in range(n):
            acc = cr.accept(lg[e], mask[e], r64[e] >> 32, 0.7)
            valid = np.flatnonzero(mask[e])
            k = ((r64[e] >> 32) * valid.size) >> 32
            assert acc == {int(valid[k])}, (board, fam, e)
            assert orc.sample_action(mask[e], SEED, OFFSET + e, int(games[e]), int(turns[e])) == int(valid[k])
            assert cr.play(lg[e], mask[e], r64[e], 0.7) == int(valid[k])
    assert cr.accept(lg[0], np.zeros(na, dtype=np.uint8), 5, 1.0) == {-1}


@pytest.mark.parametrize('board', ['micro', 'fives', 'barrage', 'c12x12'])
def test_the_intervals_bracket_softmax(board):
    """hi / total_lo and lo / total_hi bracket float64 softmax over the valid actions within n_valid * 2^-23 per action: the rule IS the
    reference's chooser (softmax of logits / T over the valid actions) up to the 23-bit fixed point, on sparse and dense masks."""
    n = 6
    for sigma in cr.SIGMAS:
        for temperature in (0.05, 1.0, 7.0):
            for fam in ('sparse', 'all'):
                mask = cr.gen_mask(board, fam, n, SEED)
                lg = cr.gen_logits(board, 'normal', n, SEED, sigma)
                for e in range(n):
                    lo, hi = cr.intervals(lg[e], mask[e], temperature)
                    valid = mask[e] != 0
                    z = lg[e].astype(np.float64) / np.float64(np.float32(temperature))
                    z = np.where(valid, z, -np.inf)
                    p = np.exp(z - z.max())
                    p /= p.sum()
                    tol = int(valid.sum()) * 2.0 ** -23
                    up, dn = hi / float(lo.sum()), lo / float(hi.sum())
                    assert (up + tol >= p).all() and (dn - tol <= p).all(), (board, sigma, temperature, fam, e)
                    assert (up - dn <= 8 * tol + 8 * 2.0 ** -23).all()        # ... and it is a tight bracket, not a trivial one
                    assert not hi[~valid].any()


def _all_cases():
    return cr.RANDOM_CASES + cr.EXACT_CASES + cr.SPECIAL_CASES


@pytest.mark.parametrize('board', CPU_BOARDS)
def test_ambiguity_cap_and_nontrivial_inputs(board):
    """Per (board, case, batch size) of the GPU file: the share of games with more than one acceptable answer, from the rule alone, is at
    most 5 %; exact cases have none; and in the normal-logits cases at the temperatures of EXP2_TEMPERATURES at least 90 % of the games
    have two or more valid actions with different positive weights (at T = 0 and 1e-30 every weight under the maximum's is 0, at 3e38
    every weight is 2^23, at T = 0.05 with sigma 4 the runner-up of a sparse mask is usually under 2^-23: those cases pin the ends of
    the rule, not exp2)."""
    worst, shares, reseeded = {}, {}, 0
    for n in cr.batch_sizes(board):
        r32 = _r32(_r64(n, n)[0])
        for case in _all_cases():
            lg, mask, temperature, sets, first = cr.settled_inputs(board, case, n, SEED, r32)
            share = cr.ambiguity_share(sets)
            worst[case[0]] = max(worst.get(case[0], 0.0), first)
            reseeded += first > cr.AMBIGUITY_CAP
            many = sum(1 for s in sets if len(s) > 1)
            assert many <= cr.AMBIGUITY_CAP * n, (board, case[0], n, share)
            if case in cr.EXACT_CASES:
                assert many == 0, (board, case[0], n)
            if case[1] == 'normal' and n == max(cr.batch_sizes(board)):
                nt = cr.nontrivial_share(lg, mask, temperature)
                shares[case[0]] = round(nt, 3)
                if (case[2], case[3]) in cr.EXP2_TEMPERATURES:
                    assert nt >= 0.9, (board, case[0], n, nt)
    # (shown with pytest -s)
    print('\n[choose ambiguity] %s: worst share per case: %s' % (board, {k: round(v, 4) for k, v in worst.items() if v} or 'none ambiguous'))
    print('[choose ambiguity] %s: %d (case, batch size) pairs moved to another seed' % (board, reseeded))
    print('[choose exp2 share] %s: 1.0 at T in {1, 7} and 0.0 at T in {0, 1e-30, 3e38} except %s' % (board, {k: v for k, v in shares.items() if 0.0 < v < 1.0} or 'none'))


# ---- broken rules ----------------------------------------------------------------------------------------------------------------------
_SPREAD = [c for c in cr.RANDOM_CASES if c[3] in (1.0, 7.0, 3e38)] + \
          [c for c in cr.EXACT_CASES if c[1] in ('ties', 'equal') or (c[1] == 'two_level' and c[4] in ('own', 'all', 'alternate'))]
_ALL_LIVE = [c for c in _all_cases() if c[4] != 'empty']


def _applies(mutant, board):
    """The cases in which a broken rule must be caught, with the reason it cannot be caught elsewhere.  -> [(case, row or None)]."""
    rows = cr.row_sizes(board)
    na = cr.n_actions(board)
    if mutant in ('descending', 'low_half'):         # needs two actions with positive weight: not argmax, not a lone action
        return [(c, None) for c in _SPREAD]
    if mutant == 'shift31':                          # a draw in the upper half finds no action at all: every case with a live game
        return [(c, None) for c in _ALL_LIVE]
    if mutant == 'max_over_invalid':                 # argmax over a sparse mask: the global maximum is invalid (at T > 0 it only rescales every weight)
        return [(c, None) for c in cr.RANDOM_CASES if c[3] in (0.0, 1e-30) and c[4] == 'own']
    if mutant == 'temperature_multiplies':
        return [(c, None) for c in cr.RANDOM_CASES if c[3] != 1.0]
    if mutant == 'nan_is_zero':                      # (at T = 0 a NaN read as 0.0 is never the maximum of 2 * N(0, 1) logits)
        return [(c, None) for c in cr.SPECIAL_CASES if c[3] == 1.0]
    if mutant == 'no_shortcut':                      # 0 * inf = NaN: without the shortcut argmax has no weight at all
        return [(c, None) for c in _ALL_LIVE if c[3] == 0.0]
    if mutant == 'row_total_31bit':                  # a row of 256 weights of 2^23
        return [(c, 256) for c in _all_cases() if 256 in rows and c[4] == 'all' and (c[1] == 'equal' or (c[1] == 'normal' and c[3] == 3e38))]
    if mutant == 'before_dropped':
        return [(c, r) for c in _SPREAD for r in rows if na > r]
    if mutant == 'partial_row_skipped':
        return [(c, r) for c in cr.EXACT_CASES if c[4] == 'lone' for r in rows if na % r]
    return []                                        # scan_ge, round_nearest, bits22: only with a chosen draw (below); padding: its own case


@pytest.mark.parametrize('board', ['micro', 'fives', 'medium'])
@pytest.mark.parametrize('mutant', [m for m in cr.MUTANTS if m not in ('scan_ge', 'round_nearest', 'bits22', 'padding_honoured')])
def test_broken_rules_are_rejected_on_the_shared_inputs(mutant, board):
    """Each broken rule, played as if it were the kernel on the generators' inputs with the counter RNG's draws, gives an answer outside
    accept() in at least one game of every case it applies to (_applies says which, and why not the others).  Shares of games outside
    accept(), 64 games per case, minimum .. maximum over the applicable cases (printed by this test), micro / fives / medium:
      descending              0.531 .. 1.000 / 0.531 .. 1.000 / 0.625 .. 1.000   (20 cases)
      low_half                0.484 .. 1.000 / 0.453 .. 1.000 / 0.516 .. 1.000   (20)
      shift31                 0.484 .. 1.000 on all three                        (37)
      max_over_invalid        0.688 .. 0.766 / 0.906 .. 0.922 / 0.953 .. 0.984   (4)
      temperature_multiplies  0.859 .. 1.000 / 0.906 .. 1.000 / 0.922 .. 1.000   (20)
      nan_is_zero             0.141 .. 0.172 / 0.141 .. 0.156 / 0.094 .. 0.094   (2)
      no_shortcut             1.000 on all three                                 (8: the T = 0 cases)
      row_total_31bit         - / - / 1.000                                      (3: a 256-action row of 2^23 weights needs 64 lanes)
      before_dropped          0.203 .. 0.859 / 0.375 .. 0.922 / 0.344 .. 0.891   (40 / 20 / 40: per row size)
      partial_row_skipped     0.328 / 0.422 / 0.250 .. 0.484                     (the lone-action masks, per row size with a partial row)
    scan_ge, round_nearest, bits22: test_rules_that_only_a_chosen_draw_can_tell_apart; padding_honoured: test_padding_bits_are_not_actions."""
    n = 64
    r64 = _r64(n, 5)[0]
    cases = _applies(mutant, board)
    if mutant == 'row_total_31bit' and board != 'medium':
        assert not cases                               # 16 / 32 lanes per game: a row total is at most 2^29 / 2^30
        return
    assert cases, (mutant, board)
    shares = []
    for case, row in cases:
        lg, mask, temperature = cr.case_inputs(board, case, n, SEED)
        out = 0
        for e in range(n):
            got = cr.play(lg[e], mask[e], r64[e], temperature, mutant=mutant, row=row)
            want = cr.accept(lg[e], mask[e], r64[e] >> 32, temperature)
            assert cr.play(lg[e], mask[e], r64[e], temperature) in want            # the rule itself is always inside
            out += got not in want
        assert out >= 1, (mutant, board, case[0], row)
        shares.append(out / n)
    print('\n[choose mutants] %-22s %-6s rejected in %d cases, share of games %.3f .. %.3f' % (mutant, board, len(cases), min(shares), max(shares)))


@pytest.mark.parametrize('board', ['micro', 'fives', 'medium', 'barrage'])
def test_padding_bits_are_not_actions(board):
    """The bit-mask packer with every padding bit set: the rule ignores them; a rule that honours them answers an action >= NA."""
    n = 32
    na = cr.n_actions(board)
    r64 = _r64(n, 9)[0]
    lg, mask, temperature = cr.case_inputs(board, cr.EXACT_CASES[0], n, SEED)
    words = cr.pack_bits(mask, padding=True)
    assert words.shape == (n, cr.compact_words(na)) and words.dtype == np.int32
    allbits = cr.unpack_bits(words)
    assert np.array_equal(allbits[:, :na], mask) and allbits[:, na:].all() and allbits.shape[1] > na
    assert np.array_equal(cr.unpack_bits(cr.pack_bits(mask), na), mask) and not cr.unpack_bits(cr.pack_bits(mask))[:, na:].any()
    out = 0
    for e in range(n):
        want = cr.accept(lg[e], mask[e], r64[e] >> 32, temperature)
        assert len(want) == 1 and max(want) < na
        got = cr.play(lg[e], mask[e], r64[e], temperature, mutant='padding_honoured', padded_valid=allbits[e])
        out += got not in want
    assert out >= 1


@pytest.mark.parametrize('board', ['micro', 'fives', 'barrage'])
def test_rules_that_only_a_chosen_draw_can_tell_apart(board):
    """`>=` for `>` in the scan, weights rounded to nearest, 22 bits: against the rule these move a draw by at most ~NA / 2^24 in total
    variation (every total holds the maximum's 2^23), so the counter RNG's draws would need thousands of games per case to show them.
    With the draw CHOSEN (unit weights, a target inside them) the acceptance set has one member and rejects all three in every game:
    the set is sharp enough; it is the device API that offers no way to set a draw."""
    n = 16
    lg, mask, temperature, r64 = cr.crafted(board, 'unit_head', n)
    for e in range(n):
        want = cr.accept(lg[e], mask[e], r64[e] >> 32, temperature)
        assert want == {10 + 3 * e} == {cr.play(lg[e], mask[e], r64[e], temperature)}
        for mutant in ('scan_ge', 'round_nearest', 'bits22'):
            assert cr.play(lg[e], mask[e], r64[e], temperature, mutant=mutant) not in want, (mutant, e)


def test_the_dropped_shortcut_at_a_positive_temperature():
    """The maximum weighing 2^23 - 1 instead of 2^23 moves a target only where total - target > total^2 / 2^32 (about 16,900 weights
    from the end): the 32x32 board, the maximum first, a chosen draw behind it."""
    lg, mask, temperature, r64 = cr.crafted('c32x32', 'unit_tail', 3)
    for e in range(3):
        want = cr.accept(lg[e], mask[e], r64[e] >> 32, temperature)
        assert len(want) == 1 and cr.play(lg[e], mask[e], r64[e], temperature) in want
        assert cr.play(lg[e], mask[e], r64[e], temperature, mutant='no_shortcut') not in want


def test_geometry_of_the_path_table():
    """ChooseGeo restated: the rows and the register cache of every board of the path table."""
    want = {'micro': (132, (3, True), (9, True)), 'tiny': (208, (4, True), (13, True)), 'c3x3': (81, None, (6, True)),
            'fives': (425, None, (14, True)), 'medium': (756, (3, True), (12, True)), 'barrage': (3700, (15, True), (58, True)),
            'standard2': (12825, None, (201, False)), 'c12x12': (6480, (26, False), (102, False)), 'c32x32': (128000, (500, False), (2000, False))}
    for board, (na, v4, v1) in want.items():
        assert (cr.n_actions(board), cr.geo(board, 4), cr.geo(board, 1)) == (na, v4, v1), board


# ---- the wrapper's argument check ------------------------------------------------------------------------------------------------------
def test_choose_actions_argument_check():
    import torch
    from stratego_env_amd.vec_env import check_choose_tensors
    n, na, words = 8, 208, 8
    dev, cpu = torch.device('cuda', 0), torch.device('cpu')
    ok_out = (torch.int32, dev, n, True)
    assert check_choose_tensors(n, na, words, dev, (torch.uint8, dev, n * na, True), ok_out) is False
    assert check_choose_tensors(n, na, words, dev, (torch.bool, dev, n * na, True), ok_out) is False
    assert check_choose_tensors(n, na, words, dev, (torch.int32, dev, n * words, True), ok_out) is True
    bad = [
        ((torch.uint8, cpu, n * na, True), ok_out),                           # a host mask
        ((torch.uint8, torch.device('cuda', 1), n * na, True), ok_out),       # another device
        ((torch.uint8, dev, n * na, False), ok_out),                          # a transposed view
        ((torch.int64, dev, n * na, True), ok_out),                           # wrong dtypes
        ((torch.int8, dev, n * na, True), ok_out),
        ((torch.float32, dev, n * na, True), ok_out),
        ((torch.uint8, dev, n * na - 1, True), ok_out),                       # wrong sizes
        ((torch.uint8, dev, n * words, True), ok_out),
        ((torch.int32, dev, n * na, True), ok_out),                           # an int32 tensor that is not the bit mask
        ((torch.int32, dev, n * words - 1, True), ok_out),
        ((torch.uint8, dev, n * na, True), (torch.int32, cpu, n, True)),
        ((torch.uint8, dev, n * na, True), (torch.int32, dev, n, False)),
        ((torch.uint8, dev, n * na, True), (torch.int64, dev, n, True)),
        ((torch.uint8, dev, n * na, True), (torch.int32, dev, n - 1, True)),
        ((torch.uint8, dev, n * na, True), (torch.int32, dev, n + 1, True)),
    ]
    for mask, out in bad:
        with pytest.raises(ValueError):
            check_choose_tensors(n, na, words, dev, mask, out)
