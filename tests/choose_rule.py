"""The chooser's rule (sgx_choose_actions, stratego_env_amd/csrc/sgx_choose.h) restated in numpy, with an acceptance set DERIVED from
the accuracy of the device's exp2f instead of fitted to it.  Plain numpy / Python: no torch, no GPU.  Test infrastructure (the draws
come from oracle/); never imported by the product package.

The rule.  Invalid actions and NaN logits count as -inf; mx = the float32 maximum; no action above -inf: the answer is -1.
scale = +inf for temperature 0, else float32(log2 e) / float32(T) (what the host computes); d = float32(l - mx);
x = d * scale + 23 rounded ONCE to float32 (the kernel's fmaf); weight = floor(exp2f(x)), exactly 2^23 where l == mx and exactly 0
where x is -inf or NaN; total = the sum; target = floor(r32 * total / 2^32); the answer is the first action in ascending order whose
running sum exceeds target.

The acceptance set.  Everything above is exact integer or correctly rounded float32 arithmetic except exp2f.  With w* = 2^x (float64)
the device weight is floor(v) for some v within E_ULP float32 ulps of w*, clipped to [0, 2^23]: an interval [lo, hi] per action.
From the running sums of the two ends and the two targets, action a can be the answer of SOME admissible rounding only if hi[a] > 0,
cum_lo[a] - lo[a] <= target_hi and cum_hi[a] > target_lo (accept()): a superset of what any admissible exp2f can give, and exactly
one action where every weight is 0 or 2^23.

E_ULP = 2.  The ROCm install this was written against ships no HIP math accuracy table (no document under its tree names exp2f), so
2 is a fallback bound chosen beforehand, NOT a measurement of the kernel: v_exp_f32 is specified to 1 ulp and the library's exp2f adds
a range scaling that is exact.  It is never to be adjusted to make a failing comparison pass.

The input generators below are deterministic functions of (board, case, seed); the GPU tests (tests/test_gpu_choose_paths.py) and the
CPU tests with the broken rules (tests/test_choose_cpu.py) call the same ones, so both see the same logits and masks.  The one input a
CPU test cannot have is the env's own mask: `sparse` (25-60 valid actions, what a position offers) stands in for it there."""
import numpy as np

BITS = 23
ONE = 1 << BITS
E_ULP = 2
LOG2E = np.float32(1.4426950408889634)
STREAM_ACTION = 1

TEMPERATURES = (0.0, 1e-30, 0.05, 1.0, 7.0, 3e38)
SIGMAS = (1.0, 4.0)

# ---- the boards of the path table ------------------------------------------------------------------------------------------------
# name: (rows, columns, lanes per game).  Lanes per game is Geo::LPG of sgx_layout.h: 16 up to 16 cells, 32 up to 32, else 64.
BOARDS = {
    'micro': (3, 4, 16), 'tiny': (4, 4, 16), 'c3x3': (3, 3, 16), 'fives': (5, 5, 32), 'medium': (6, 6, 64), 'barrage': (10, 10, 64),
    'standard2': (15, 15, 64), 'c12x12': (12, 12, 64), 'c32x32': (32, 32, 64),
}
CACHE_LIMIT = 72            # ChooseGeo::CACHE: ROWS * VEC <= 72 keeps the game's logits in registers
WAVES = 4                   # ChooseGeo::WAVES: waves per workgroup
MAX_GAMES = {'c32x32': 5, 'c12x12': 20, 'standard2': 40}


def n_actions(board):
    R, C, _ = BOARDS[board]
    return R * C * (2 * (R - 1) + 2 * (C - 1) + 1)


def lanes(board):
    return BOARDS[board][2]


def geo(board, vec):
    """ChooseGeo restated -> (rows, cached), or None where the board has no such kernel (VEC 4 needs NA % 4 == 0)."""
    na, lpg = n_actions(board), lanes(board)
    if vec == 4 and na % 4:
        return None
    nch = (na + vec - 1) // vec
    rows = (nch + lpg - 1) // lpg
    return rows, rows * vec <= CACHE_LIMIT


def games_per_workgroup(board):
    return WAVES * (64 // lanes(board))


def row_sizes(board):
    """Actions per row of the kernels the board has: LPG * VEC."""
    return [lanes(board) * vec for vec in (4, 1) if geo(board, vec)]


def compact_words(na):
    """sgx_compact_mask_words: Geo::MB_WORDS."""
    return (((na + 31) // 32 + 1) + 3) & ~3


def batch_sizes(board):
    """1, one workgroup's games - 1 / + 0 / + 1, a prime near 200 -- capped for the big boards."""
    g = games_per_workgroup(board)
    cap = MAX_GAMES.get(board, 211)
    return sorted({min(n, cap) for n in (1, g - 1, g, g + 1, 211)})


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def host_scale(temperature):
    with np.errstate(over='ignore', divide='ignore'):
        return np.float32(np.inf) if temperature == 0 else LOG2E / np.float32(temperature)


def masked(logits, valid):
    """float32 logits with invalid actions and NaN at -inf, and their float32 maximum."""
    lg = np.asarray(logits, dtype=np.float32)
    l = np.where(np.asarray(valid, dtype=bool) & ~np.isnan(lg), lg, np.float32(-np.inf)).astype(np.float32)
    return l, (l.max() if l.size else np.float32(-np.inf))


def fma_x(l, mx, scale):
    """float32(d * scale + 23) with ONE rounding, d = float32(l - mx): the product of two float32 is exact in float64, the sum is taken
    with its rounding error (two-sum), and the error decides the one case in which rounding the float64 sum to float32 would round
    twice: a sum that lands exactly half way between two float32."""
    with np.errstate(invalid='ignore', over='ignore'):
        d = (l - mx).astype(np.float32)
        p = d.astype(np.float64) * np.float64(scale)                       # exact: 24 + 24 significant bits
        s = p + 23.0
        fin = np.isfinite(p)
        bb = s - p
        err = np.where(fin, (p - (s - bb)) + (23.0 - bb), 0.0)              # p + 23 == s + err exactly
        x = s.astype(np.float32)
        xd = x.astype(np.float64)
        other = np.nextafter(x, np.where(s > xd, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
        tie = fin & (err != 0) & (xd != s) & ((xd + other.astype(np.float64)) * 0.5 == s)
        if tie.any():
            up = np.maximum(x, other)
            dn = np.minimum(x, other)
            x = np.where(tie, np.where(err > 0, up, dn), x).astype(np.float32)
    return x


def exact_weights(l, mx, scale):
    """w* = 2^x in float64 per action (2^23 where l == mx, 0 where x is -inf or NaN) and the mask of the l == mx actions."""
    top = l == mx
    x = fma_x(l, mx, scale)
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        w = np.exp2(x.astype(np.float64))
    w = np.where(np.isnan(w), 0.0, w)
    return np.where(top, float(ONE), w), top


def intervals(logits, valid, temperature, e_ulp=E_ULP):
    """-> (lo, hi) int64 [NA]: the weights any admissible exp2f can give; None for a game without a drawable action."""
    l, mx = masked(logits, valid)
    if mx == -np.inf:
        return None
    w, top = exact_weights(l, mx, host_scale(temperature))
    _, e = np.frexp(w)                                                    # w = m * 2^e, 0.5 <= m < 1: float32 ulp = 2^(e - 24)
    slack = e_ulp * np.ldexp(1.0, e - 24)
    lo = np.floor(np.clip(w - slack, 0.0, float(ONE))).astype(np.int64)
    hi = np.floor(np.clip(w + slack, 0.0, float(ONE))).astype(np.int64)
    dead = w == 0.0
    lo = np.where(top, ONE, np.where(dead, 0, lo))
    hi = np.where(top, ONE, np.where(dead, 0, hi))
    return lo, hi


def accept_from(lo, hi, r32):
    cum_lo, cum_hi = np.cumsum(lo), np.cumsum(hi)
    target_lo = (int(r32) * int(cum_lo[-1])) >> 32
    target_hi = (int(r32) * int(cum_hi[-1])) >> 32
    ok = (hi > 0) & (cum_lo - lo <= target_hi) & (cum_hi > target_lo)
    return set(np.flatnonzero(ok).tolist())


def accept(logits, mask_valid, r32, temperature):
    """The set of answers the kernel may give for one game (see the module docstring)."""
    iv = intervals(logits, mask_valid, temperature)
    if iv is None:
        return {-1}
    return accept_from(iv[0], iv[1], r32)


def accept_batch(logits, valid, r32, temperature):
    return [accept(logits[e], valid[e], r32[e], temperature) for e in range(len(logits))]


def ambiguity_share(sets):
    return sum(1 for s in sets if len(s) > 1) / max(1, len(sets))


# ---- the rule "played" (one admissible rounding: exp2 in float64), with the switches of the broken rules -------------------------------
NOT_WRITTEN = -2            # a broken rule under which no lane of the kernel would write an answer

MUTANTS = ('scan_ge', 'descending', 'low_half', 'shift31', 'max_over_invalid', 'temperature_multiplies', 'nan_is_zero', 'round_nearest',
           'bits22', 'no_shortcut', 'row_total_31bit', 'before_dropped', 'partial_row_skipped', 'padding_honoured')


def play(logits, valid, r64, temperature, mutant=None, row=None, padded_valid=None):
    """The answer of the rule for one game; r64 = the whole 64-bit draw (r32 is its high half).  mutant: one of MUTANTS, the rule broken
    in that one way.  row = actions per row (LPG * VEC) for the broken rules that depend on the rows; padded_valid = the validity of
    every bit of the game's bit-mask words (padding included) for 'padding_honoured' (logits beyond NA read as 0.0)."""
    lg = np.asarray(logits, dtype=np.float32)
    valid = np.asarray(valid, dtype=bool)
    na = lg.size
    if mutant == 'padding_honoured':
        lg = np.concatenate([lg, np.zeros(padded_valid.size - na, dtype=np.float32)])
        valid = np.asarray(padded_valid, dtype=bool)
    if mutant == 'partial_row_skipped':
        valid = valid.copy()
        valid[(na // row) * row:] = False
    if mutant == 'nan_is_zero':
        lg = np.where(np.isnan(lg), np.float32(0.0), lg)
    l, mx = masked(lg, valid)
    if mutant == 'max_over_invalid':
        mx = masked(lg, np.ones_like(valid))[1]
    if mx == -np.inf:
        return -1
    if mutant == 'temperature_multiplies':
        with np.errstate(over='ignore'):
            scale = LOG2E * np.float32(temperature)
    else:
        scale = host_scale(temperature)
    w, top = exact_weights(l, mx, scale)
    if mutant == 'round_nearest':
        wi = np.floor(w + 0.5).astype(np.int64)
    elif mutant == 'bits22':
        wi = np.floor(w * 0.5).astype(np.int64)
    else:
        wi = np.floor(w).astype(np.int64)
    if mutant == 'no_shortcut':
        wi = np.where(top, ONE - 1, wi)                                    # floor(exp2(23) * (1 - 2^-24)) in float32 arithmetic: 2^23 - 1
        if not np.isfinite(scale):                                        # 0 * inf: without the shortcut the maximum's x is NaN
            wi = np.where(top, 0, wi)
    if mutant == 'descending':
        wi = wi[::-1]
    n = wi.size
    if mutant == 'row_total_31bit':
        pad = (-n) % row
        rows = np.concatenate([wi, np.zeros(pad, dtype=np.int64)]).reshape(-1, row).sum(axis=1) & 0x7FFFFFFF
        total = int(rows.sum())
    else:
        total = int(wi.sum())
    if total == 0:                                                        # (the kernel answers -1 only where mx is -inf)
        return NOT_WRITTEN
    draw = (int(r64) & 0xFFFFFFFF) if mutant == 'low_half' else (int(r64) >> 32)
    target = (draw * total) >> (31 if mutant == 'shift31' else 32)
    cum = np.cumsum(wi)
    if mutant == 'row_total_31bit':                                       # the row is found from the truncated totals, the lane from the true weights
        before, jr = 0, -1
        for j, t in enumerate(rows.tolist()):
            if before + t > target:
                jr = j
                break
            before += t
        if jr < 0:
            return NOT_WRITTEN
        inc = before + np.cumsum(wi[jr * row:(jr + 1) * row])
        hit = np.flatnonzero(inc > target)
        return jr * row + int(hit[0]) if hit.size else NOT_WRITTEN
    if mutant == 'before_dropped':
        jr = int(np.argmax(cum > target)) // row if cum[-1] > target else -1
        if jr < 0:
            return NOT_WRITTEN
        hit = np.flatnonzero(np.cumsum(wi[jr * row:(jr + 1) * row]) > target)
        return jr * row + int(hit[0]) if hit.size else NOT_WRITTEN
    hit = cum >= target if mutant == 'scan_ge' else cum > target
    if not hit.any():
        return NOT_WRITTEN
    a = int(np.argmax(hit))
    return n - 1 - a if mutant == 'descending' else a


# ---- generators --------------------------------------------------------------------------------------------------------------------
def _rs(board, case, seed):
    import zlib
    return np.random.RandomState((zlib.crc32(('%s/%s' % (board, case)).encode()) + 7919 * int(seed)) & 0x7FFFFFFF)


def lone_positions(board):
    """Where a lone valid action goes: 0, NA - 1, and for every row size of the board's kernels the last action of row j and the first
    of row j + 1 for j = 0 and the last whole row, and the middle of the final partial row."""
    na = n_actions(board)
    pos = [0, na - 1]
    for row in row_sizes(board):
        jl = na // row                                                    # whole rows
        for j in sorted({0, jl - 1} - {-1}):
            pos += [p for p in ((j + 1) * row - 1, (j + 1) * row) if p < na]
        if na % row:
            pos.append(jl * row + (na - jl * row) // 2)
    out = []
    for p in pos:
        if p not in out:
            out.append(p)
    return out


MASK_FAMILIES = ('sparse', 'all', 'alternate', 'lone', 'empty')


def gen_mask(board, family, n, seed=0, rot=0):
    """uint8 [n, NA].  'lone': game e has the single valid action lone_positions(board)[(e + rot) % len]."""
    na = n_actions(board)
    m = np.zeros((n, na), dtype=np.uint8)
    if family == 'all':
        m[:] = 1
    elif family == 'alternate':
        m[:, (np.arange(na) + seed) % 2 == 0] = 1
    elif family == 'lone':
        pos = lone_positions(board)
        for e in range(n):
            m[e, pos[(e + rot) % len(pos)]] = 1
    elif family == 'sparse':
        rs = _rs(board, 'sparse', seed)
        for e in range(n):
            k = int(rs.randint(25, 61))
            m[e, rs.choice(na, size=min(k, na), replace=False)] = 1
    elif family != 'empty':
        raise ValueError(family)
    return m


def stripes(lg):
    """The special-value pattern: NaN and -inf stripes everywhere, +inf stripes in every fifth game."""
    lg[:, ::7] = np.nan
    lg[:, 3::11] = -np.inf
    lg[::5, 5::13] = np.inf
    return lg


def gen_logits(board, family, n, seed=0, sigma=1.0, valid=None):
    """float32 [n, NA].  normal: sigma * N(0, 1); special: the same with the stripes; two_level: 0 or -1000; ties: 3-7 equal maxima among
    the valid actions of `valid`, everything else at least 40 below (weight 0 at temperature 1: the answer is exact); equal: 0.25;
    dead: -inf and NaN only."""
    na = n_actions(board)
    rs = _rs(board, '%s/%g' % (family, sigma), seed)
    if family == 'equal':
        return np.full((n, na), 0.25, dtype=np.float32)
    if family == 'dead':
        lg = np.full((n, na), -np.inf, dtype=np.float32)
        lg[:, ::2] = np.nan
        return lg
    if family == 'two_level':
        return np.where(rs.rand(n, na) < 0.5, np.float32(0.0), np.float32(-1000.0)).astype(np.float32)
    lg = (rs.standard_normal((n, na)) * sigma).astype(np.float32)
    if family == 'normal':
        return lg
    if family == 'special':
        return stripes(lg)
    if family == 'ties':
        lg = (-40.0 - np.abs(lg)).astype(np.float32)
        for e in range(n):
            cand = np.flatnonzero(valid[e]) if valid is not None else np.arange(na)
            if cand.size:
                k = min(int(rs.randint(3, 8)), cand.size)
                lg[e, rs.choice(cand, size=k, replace=False)] = np.float32(1.5)
        return lg
    raise ValueError(family)


def pack_bits(mask_u8, padding=False):
    """The compact mask: bit a & 31 of word a >> 5, compact_words(NA) int32 words per game; padding=True sets every bit beyond NA."""
    m = np.asarray(mask_u8) != 0
    n, na = m.shape
    words = compact_words(na)
    bits = np.full((n, words * 32), bool(padding))
    bits[:, :na] = m
    w = (bits.reshape(n, words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    return w.astype(np.uint32).view(np.int32)


def unpack_bits(words, na=None):
    w = np.ascontiguousarray(words).view(np.uint32)
    bits = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1).astype(np.uint8)
    return bits if na is None else bits[:, :na]


def draws(seed, env_id_offset, games, turns):
    """The whole 64-bit draw of the counter RNG for env e in game games[e] at turn turns[e] (r32 = draw >> 32)."""
    from oracle import oracle as orc
    return [orc.rng(int(seed), int(env_id_offset) + e, int(games[e]), STREAM_ACTION, int(turns[e])) for e in range(len(games))]


def synthetic_keys(n, salt):
    """(games, turns) for a CPU run: what a few steps of a batch of envs would show."""
    e = np.arange(n)
    return (e * 7 + salt) % 5, (e * 3 + salt) % 40


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------
# (name, logits family, sigma, temperature, mask family); mask family 'own' = the env's mask on the GPU, 'sparse' on the CPU
RANDOM_CASES = [('normal s%g T%g %s' % (s, t, m), 'normal', s, t, m) for s in SIGMAS for t in TEMPERATURES for m in ('own', 'all')]
EXACT_CASES = ([('two_level %s' % m, 'two_level', 1.0, 1.0, m) for m in ('own', 'all', 'alternate', 'lone', 'empty')] +
               [('ties T%g %s' % (t, m), 'ties', 1.0, t, m) for t in (0.0, 1.0) for m in ('own', 'all')] +
               [('equal all', 'equal', 1.0, 0.7, 'all')])
SPECIAL_CASES = [('special T%g %s' % (t, m), 'special', 2.0, t, m) for t in (1.0, 0.0) for m in ('own', 'all')]
# (sigma, T) at which a normal-logits case must exercise exp2 in at least 90 % of its games.  Not the others: at T = 0 and 1e-30 every
# weight under the maximum's is 0 and at 3e38 every weight is 2^23 by construction (they pin the two ends of the rule), and at T = 0.05
# the runner-up of 25-60 valid actions is under 2^-23 of the maximum in 7-25 % of the games at sigma 1 and in 60 % at sigma 4.
EXP2_TEMPERATURES = ((1.0, 1.0), (1.0, 7.0), (4.0, 1.0), (4.0, 7.0))
AMBIGUITY_CAP = 0.05


def case_inputs(board, case, n, seed, own_mask=None, rot=0):
    """-> (logits float32 [n, NA], mask uint8 [n, NA], temperature) of a case; own_mask = the env's mask where the case asks for it
    (None: the sparse stand-in)."""
    name, family, sigma, temperature, mfam = case
    if mfam == 'own':
        mask = own_mask if own_mask is not None else gen_mask(board, 'sparse', n, seed)
    else:
        mask = gen_mask(board, mfam, n, seed, rot)
    return gen_logits(board, family, n, seed, sigma, valid=mask), mask, temperature


def settled_inputs(board, case, n, seed, r32, own_mask=None, rot=0, tries=12):
    """case_inputs at the first of the seeds seed, seed + 1000, ... at which the share of games with more than one acceptable answer is
    within AMBIGUITY_CAP -- decided by the rule alone, before any answer of a kernel exists.  (The cap bites on the dense masks of the
    largest boards: 128,000 valid actions of similar weight leave 3-7 % of the games with two acceptable neighbours, and a batch of
    five games has no room for one.)  -> (logits, mask, temperature, acceptance sets, the share at the first seed)."""
    first = None
    for k in range(tries):
        lg, mask, temperature = case_inputs(board, case, n, seed + 1000 * k, own_mask, rot)
        sets = accept_batch(lg, mask, r32, temperature)
        first = ambiguity_share(sets) if first is None else first
        if sum(1 for s in sets if len(s) > 1) <= AMBIGUITY_CAP * n:
            return lg, mask, temperature, sets, first
    raise AssertionError("no seed of %d keeps %s / %s within the ambiguity cap" % (tries, board, case[0]))


def mixed_inputs(board, n, seed, rot, own_mask=None):
    """Mixed waves: game e has an empty mask if (e + rot) % 3 == 0, only -inf / NaN logits if == 1, and is live otherwise."""
    lg, mask, temperature = case_inputs(board, ('mixed', 'normal', 1.0, 1.0, 'own'), n, seed, own_mask)
    mask = mask.copy()
    kind = (np.arange(n) + rot) % 3
    mask[kind == 0] = 0
    lg[kind == 1] = gen_logits(board, 'dead', int((kind == 1).sum()))
    return lg, mask, temperature, kind


def crafted(board, kind, n):
    """CPU only: cases whose DRAW is chosen, which the device API does not allow (a draw is keyed by seed, env, game and turn).  They
    show that the acceptance set itself tells a broken rule from the rule where the counter RNG's draws would need ~2^23 / NA games to.
    Temperature float32(log2 e) makes scale exactly 1, so a logit of -22.25 below the maximum weighs 2^0.75 = 1.68...: 1 truncated, 2
    rounded, 0 at 22 bits, and far enough from an integer for the interval to be [1, 1].
    unit_head: every action valid, the maximum LAST, target 10 + 3e inside the unit weights before it.
    unit_tail: the maximum FIRST, the target (NA - 1) / 2 + 3e unit weights behind it, and of the draws with that target the largest.
    -> (logits, mask, temperature, r64 list)."""
    na = n_actions(board)
    lg = np.full((n, na), -22.25, dtype=np.float32)
    mask = np.ones((n, na), dtype=np.uint8)
    total = ONE + na - 1
    r64 = []
    for e in range(n):
        if kind == 'unit_head':
            lg[e, na - 1] = 0.0
            t = 10 + 3 * e
            r32 = -((-t << 32) // total)                                  # the smallest draw whose target is t
        else:
            lg[e, 0] = 0.0
            t = ONE + (na - 1) // 2 + 3 * e
            r32 = (((t + 1) << 32) - 1) // total                         # the largest
        assert 0 <= r32 < 1 << 32 and (r32 * total) >> 32 == t and t < total
        r64.append((r32 << 32) | 0x9E3779B9)
    return lg, mask, float(LOG2E), r64


def nontrivial_share(logits, valid, temperature):
    """The share of games with two or more valid actions whose weights are positive and different."""
    hits = 0
    for e in range(len(logits)):
        l, mx = masked(logits[e], valid[e])
        if mx == -np.inf:
            continue
        w = np.floor(exact_weights(l, mx, host_scale(temperature))[0])
        hits += np.unique(w[w > 0]).size >= 2
    return hits / max(1, len(logits))
