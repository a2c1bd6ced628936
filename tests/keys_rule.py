"""The position-key rule (sgx_state_keys) restated in numpy on the reference's int64 [34,R,C] states: what the device kernel
must reproduce bit for bit.  Test infrastructure; never imported by the product package.

The key of a position is the SplitMix finaliser of the XOR of one hash per feature of the state: every non-zero (layer, cell, value) outside
the obstacle layer, the scalar layer and -- for an information-set key -- the true pieces of the observer's opponent; the scalars, the mover
and the observer, hashed whether zero or not.  `key` is the definition, entry by entry; `keys` is the same arithmetic on whole arrays (the
tests hold one against the other) for batches."""
import numpy as np

M64 = (1 << 64) - 1


def sm_fin(z):
    z &= M64
    z ^= z >> 30; z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27; z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


SALT = (0x5347584B45595330, 0x5347584B45595331)   # word 0 / word 1 ("SGXKEYS0" / "SGXKEYS1")
GOLD = 0x9E3779B97F4A7C15


def feat(word, slot, value):                       # value: two's complement, low 32 bits
    w = ((slot & 0xFFFFFFFF) << 32) | (value & 0xFFFFFFFF)
    return sm_fin(SALT[word] + GOLD * (w + 1))


def key(state, player, observer=None, clock=True, word=0):
    """observer None = state key; +1 / -1 = that player's information set; 0 = the mover's"""
    L, R, C = state.shape
    skip = {2, 5}                                  # obstacles (constant per variant), scalars (below)
    if observer is not None:
        obs = player if observer == 0 else observer
        skip.add(1 if obs == 1 else 0)             # the TRUE pieces of the observer's opponent
    x = 0
    for l in range(34):
        if l in skip: continue
        for cell in range(R * C):
            v = int(state[l, cell // C, cell % C])
            if v: x ^= feat(word, l * 1024 + cell, v)
    sc = [int(state[5,0,1]), int(state[5,0,2]), int(state[5,1,1]), int(player)]   # game over, winner, ending invalid, mover
    if clock: sc += [int(state[5,0,0]), int(state[5,1,0])]                        # turn count, max turns
    for i, v in enumerate(sc):
        x ^= feat(word, 5 * 1024 + i, v)           # scalar features are hashed whether zero or not
    if observer is not None:
        x ^= feat(word, 5 * 1024 + 6, obs)
    return sm_fin(x)


def known_answer_state():
    """the 3x4 state of the known answers (include/stratego_mi355x.h gives the rule; the answers were computed with `key`)"""
    s = np.zeros((34, 3, 4), dtype=np.int64)
    s[0, 0, 1], s[0, 0, 2] = 11, 2
    s[1, 2, 3], s[1, 2, 0] = 11, 10
    s[3, 0, 1], s[3, 0, 2] = 13, 2
    s[4, 2, 3], s[4, 2, 0] = 13, 13
    s[32, 0, 1] = 1
    s[33, 2, 3] = s[33, 2, 0] = 1
    s[6, 0, 2], s[6, 1, 2] = -1, 1
    s[9, 1, 1] = 2
    s[5, 0, 0], s[5, 1, 0] = 7, 50
    return s


# (arguments of key) -> (answer for player +1, answer for player -1)
KNOWN_ANSWERS = {
    'state key': (dict(), 0x57a8b3c530c10805, 0x4abb9aee14fae68f),
    'word 1': (dict(word=1), 0xffa55259982c32e6, 0x9857728de2befe00),
    'no clock': (dict(clock=False), 0xf464de7ffe726ede, 0xc0fcb7d37ea16ecc),
    'observer +1': (dict(observer=1), 0xd78b1c91fc25daff, 0x75a5e6b1cacbaa60),
    'observer -1': (dict(observer=-1), 0xde5b56795eeedaca, 0x50a3ec072a8672d9),
    'observer 0 (mover)': (dict(observer=0), 0xd78b1c91fc25daff, 0x50a3ec072a8672d9),
}
SWAPPED_HIDDEN = {'state key': (dict(), 0x64175b8e326ffc8a), 'observer +1': (dict(observer=1), 0xd78b1c91fc25daff),
                  'observer -1': (dict(observer=-1), 0x27e7c1f2c4f8ef22)}          # layer 1: (2,3)=10, (2,0)=11, mover +1
ZERO_3X3_STATE_KEY = 0x5cc2158e381d6d68            # all-zero 3x3 state, mover +1


# ---- the same rule on whole arrays (uint64 arithmetic wraps like the masks above) ------------------------------------------------------------
def _fin(z):
    z = z.astype(np.uint64)
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _feat(word, slot, value):
    w = (np.asarray(slot).astype(np.uint64) << np.uint64(32)) | (np.asarray(value).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF))
    return _fin(np.uint64(SALT[word]) + np.uint64(GOLD) * (w + np.uint64(1)))


def keys(states, players, observer=None, clock=True, word=0):
    """states int64 [n,34,R,C], players [n] -> uint64 [n]: key(states[i], players[i], ...) for every i"""
    states = np.asarray(states, dtype=np.int64)
    players = np.asarray(players).astype(np.int64).reshape(-1)
    n, L, R, C = states.shape
    with np.errstate(over='ignore'):
        flat = states.reshape(n, L, R * C)
        slot = (np.arange(L)[:, None] * 1024 + np.arange(R * C)[None, :])[None]
        h = np.where(flat != 0, _feat(word, np.broadcast_to(slot, flat.shape), flat), np.uint64(0))
        use = np.ones((n, L), dtype=bool)
        use[:, 2] = use[:, 5] = False
        obs = None
        if observer is not None:
            obs = players if observer == 0 else np.full(n, int(observer), dtype=np.int64)
            use[np.arange(n), np.where(obs == 1, 1, 0)] = False
        h = np.where(use[:, :, None], h, np.uint64(0))
        x = np.bitwise_xor.reduce(h.reshape(n, -1), axis=1)
        sc = [states[:, 5, 0, 1], states[:, 5, 0, 2], states[:, 5, 1, 1], players]
        if clock:
            sc += [states[:, 5, 0, 0], states[:, 5, 1, 0]]
        for i, v in enumerate(sc):
            x = x ^ _feat(word, np.full(n, 5 * 1024 + i), v)
        if obs is not None:
            x = x ^ _feat(word, np.full(n, 5 * 1024 + 6), obs)
        return _fin(x)


def as_int64(k):
    """the bit pattern of uint64 keys as the int64 the Python classes return"""
    return np.asarray(k, dtype=np.uint64).view(np.int64)
