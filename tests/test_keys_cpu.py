"""Position keys (sgx_state_keys) without a GPU: the numpy restatement of the rule (tests/keys_rule.py, what the device kernel
is held to bit for bit in tests/test_gpu_keys.py) against its known answers, its properties on oracle positions -- equal keys exactly for
equal positions, for equal information sets -- and the binding."""
import collections
import re
import os

import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd import _lib
from stratego_env_amd.config import VARIANTS
from tests import determinize_rule as dr
from tests import keys_rule as kr
from tests.helpers import oracle_cvariant, oracle_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARDS = ['micro', 'fives', 'barrage']
N_POSITIONS = 300
STRIDE = {'barrage': 4}


def test_known_answers():
    s = kr.known_answer_state()
    for what, (kw, plus, minus) in kr.KNOWN_ANSWERS.items():
        assert kr.key(s, 1, **kw) == plus and kr.key(s, -1, **kw) == minus, what
        assert kr.keys(np.stack([s, s]), [1, -1], **kw).tolist() == [plus, minus], what          # the array form is the same rule
    t = s.copy()
    t[1, 2, 3], t[1, 2, 0] = 10, 11                          # player -1's two hidden pieces swapped
    for what, (kw, answer) in kr.SWAPPED_HIDDEN.items():
        assert kr.key(t, 1, **kw) == answer == int(kr.keys(t[None], [1], **kw)[0]), what
    assert kr.key(np.zeros((34, 3, 3), dtype=np.int64), 1) == kr.ZERO_3X3_STATE_KEY
    assert kr.as_int64([plus]).dtype == np.int64 and int(kr.as_int64([0xffa55259982c32e6])[0]) < 0     # the bit pattern, as int64


_positions_cache = {}


def positions(name):
    """(states [n,34,R,C], movers [n]) along oracle games played to their end with random valid moves from a fixed seed: every STRIDE-th
    position of a game and its final one (every position on the small boards; a Barrage game lasts hundreds of moves); the last N_POSITIONS
    collected, so that they end with a finished game; computed once per board"""
    if name in _positions_cache:
        return _positions_cache[name]
    rs = np.random.RandomState(1234)
    cv = oracle_cvariant(name)
    stride = STRIDE.get(name, 1)
    states, movers = [], []
    g = 0
    while len(states) < N_POSITIONS:
        env = oracle_env(name)
        obs = env.reset(initial_state_override=orc.reset_state(cv, 4242, g, 0))
        g += 1
        states.append(env.state.copy()); movers.append(env.player)
        for t in range(1, VARIANTS[name].max_turns + 2):      # (the max-turn ending closes every game: a count bounds the loop)
            p = env.player
            a = int(rs.choice(np.flatnonzero(obs[p]['valid_actions_mask'].reshape(-1))))
            obs, rew, done, info = env.step({p: a})
            if done['__all__'] or t % stride == 0:
                states.append(env.state.copy()); movers.append(env.player)
            if done['__all__']:
                break
        assert done['__all__'], (name, g)
    out = (np.stack(states[-N_POSITIONS:]), np.asarray(movers[-N_POSITIONS:], dtype=np.int64))
    finished = out[0][:, 5, 0, 1] != 0
    assert finished.any() and not finished.all(), "finished and unfinished games are among the positions"
    _positions_cache[name] = out
    return out


def _partition(labels):
    groups = collections.defaultdict(list)
    for i, l in enumerate(labels):
        groups[l].append(i)
    return sorted(groups.values())


@pytest.mark.parametrize('name', BOARDS)
def test_equal_keys_exactly_for_equal_positions(name):
    states, movers = positions(name)
    # the positions, each once more under the other mover, once with another turn count and once with another max turns: pairs that differ in
    # the mover only, in the clock only
    other_turn, other_max = states.copy(), states.copy()
    other_turn[:, 5, 0, 0] += 2
    other_max[:, 5, 1, 0] += 10
    s = np.concatenate([states, states, other_turn, other_max, states])
    p = np.concatenate([movers, -movers, movers, movers, movers])
    by_state = _partition([(x.tobytes(), int(q)) for x, q in zip(s, p)])
    assert len(by_state) < len(s), "some positions are equal"
    for word in (0, 1):
        assert _partition(kr.keys(s, p, word=word).tolist()) == by_state, (name, word)
    no_clock = s.copy()
    no_clock[:, 5, 0, 0] = no_clock[:, 5, 1, 0] = 0
    by_no_clock = _partition([(x.tobytes(), int(q)) for x, q in zip(no_clock, p)])
    assert len(by_no_clock) < len(by_state)
    for word in (0, 1):
        assert _partition(kr.keys(s, p, clock=False, word=word).tolist()) == by_no_clock, (name, word)
    # the entry-by-entry definition agrees with the array form on real positions
    for i in (0, len(states) // 2, len(states) - 1):
        for kw in (dict(), dict(observer=0), dict(observer=1, clock=False, word=1), dict(observer=-1)):
            assert kr.key(states[i], int(movers[i]), **kw) == int(kr.keys(states[i:i + 1], movers[i:i + 1], **kw)[0]), (name, i, kw)


@pytest.mark.parametrize('name', BOARDS)
def test_information_sets(name):
    v = VARIANTS[name]
    ru = orc.OracleRules(v.rows, v.columns)
    states, movers = positions(name)
    pick = np.linspace(0, len(states) - 1, 24).astype(int)
    moved = 0
    for observer in (1, -1, 0):
        worlds, world_movers, roots = [], [], []
        for si in pick:
            st, mover = states[si], int(movers[si])
            worlds.append(st); world_movers.append(mover); roots.append(si)
            for draw in (0, 1, 2):
                w, hidden = dr.determinize(st, mover, observer, seed=0x5EED, g=int(si), draw=draw)
                assert hidden >= 0
                worlds.append(w); world_movers.append(mover); roots.append(si)
        worlds, world_movers, roots = np.stack(worlds), np.asarray(world_movers), np.asarray(roots)
        info = kr.keys(worlds, world_movers, observer=observer)
        info1 = kr.keys(worlds, world_movers, observer=observer, word=1)
        state_keys = kr.keys(worlds, world_movers)
        for si in pick:
            sel = np.flatnonzero(roots == si)
            assert len(set(info[sel].tolist())) == 1 and len(set(info1[sel].tolist())) == 1, (name, observer, si)     # one information set
            for j in sel[1:]:
                differs = not np.array_equal(worlds[j], worlds[sel[0]])
                assert (state_keys[j] != state_keys[sel[0]]) == differs, (name, observer, si)
                moved += int(differs)
        # inside one key group the observer's raw partial observation is one observation
        for group in _partition(info.tolist()):
            seen = set()
            for j in group:
                o = int(world_movers[j]) if observer == 0 else observer
                seen.add((o, ru.get_partially_observable_observation_extended_channels(worlds[j], o).tobytes()))
            assert len(seen) == 1, (name, observer, group)
    assert moved > 0, "some world differs from its root"


@pytest.mark.parametrize('name', BOARDS)
def test_every_included_layer_moves_the_key_and_the_excluded_one_does_not(name):
    states, movers = positions(name)
    st, mover = states[len(states) // 3], int(movers[len(states) // 3])
    R, C = st.shape[1:]
    for observer in (None, 1, -1, 0):
        obs = None if observer is None else (mover if observer == 0 else observer)
        excluded = {2} | (set() if obs is None else {1 if obs == 1 else 0})
        base = [kr.key(st, mover, observer=observer, word=w) for w in (0, 1)]
        for l in range(34):
            cells = [(0, 0), (R - 1, C - 1)] if l != 5 else [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)]
            for r, c in cells:
                t = st.copy()
                t[l, r, c] += 1
                got = [kr.key(t, mover, observer=observer, word=w) for w in (0, 1)]
                if l in excluded:
                    assert got == base, (name, observer, l)
                else:
                    assert got[0] != base[0] and got[1] != base[1], (name, observer, l, r, c)
        # a scalar cell the rule does not name is not part of it; the mover and the observer are
        t = st.copy()
        t[5, R - 1, C - 1] += 1
        assert kr.key(t, mover, observer=observer) == base[0]
        assert kr.key(st, -mover, observer=observer) != base[0]
    assert len({kr.key(st, mover, observer=o) for o in (None, 1, -1)}) == 3
    # without the clock turn count and max turns are out, everything else is in
    t = st.copy()
    t[5, 0, 0] += 1; t[5, 1, 0] += 1
    assert kr.key(t, mover, clock=False) == kr.key(st, mover, clock=False) and kr.key(t, mover) != kr.key(st, mover)


def test_the_binding():
    assert 'sgx_state_keys' in _lib.EXPORTED_SYMBOLS
    assert (_lib.KEYS_VIEW_STATE, _lib.KEYS_NO_CLOCK, _lib.KEYS_WIDE) == (2, 1, 2)
    hdr = open(os.path.join(ROOT, 'include', 'stratego_mi355x.h')).read()
    assert re.search(r'#define SGX_KEYS_VIEW_STATE 2\b', hdr) and re.search(r'#define SGX_KEYS_NO_CLOCK 1\b', hdr) and re.search(r'#define SGX_KEYS_WIDE\s+2\b', hdr)
    assert re.search(r'int sgx_state_keys\(sgx_env \*src, const int32_t \*src_index_dev, int64_t n, int32_t view, int32_t flags, uint64_t \*keys_dev, void \*stream\);', hdr)
    assert _lib.ABI_VERSION == 15                       # no struct or signature of the existing ABI changed
    # the constants of the rule, as the header states them
    for const in ('0xBF58476D1CE4E5B9', '0x94D049BB133111EB', '0x9E3779B97F4A7C15', '0x5347584B45595330', '0x5347584B45595331'):
        assert const in hdr, const


def test_the_library_exports_the_entry_point():
    from stratego_env_amd import build as hip_build
    hip_build.build()
    L = _lib.load()
    assert len(L.sgx_state_keys.argtypes) == 7
    # refusals are host-side and need no device: a NULL handle is SGX_EINVAL with a message that names the call
    assert L.sgx_state_keys(None, None, 0, 2, 0, None, None) == -1
    assert b'sgx_state_keys' in L.sgx_last_error()


def test_the_new_kernels_use_no_scratch_memory_and_no_lds(tmp_path):
    """keys_kernel on every board of the reference, both key widths: no scratch memory, no LDS (read from the shipped library)"""
    from tests.step_checks import _kernel_resources
    res = _kernel_resources(tmp_path)
    seen = set()
    for name, r in res.items():
        m = re.search(r'11keys_kernelILi(\d+)ELi(\d+)ELb([01])E', name)
        if not m:
            continue
        assert r['scratch'] == 0 and r['lds'] == 0, (name, r)
        seen.add((int(m.group(1)), int(m.group(2)), int(m.group(3))))
    boards = {(10, 10), (15, 15), (8, 8), (6, 6), (5, 5), (4, 4), (3, 4)}
    assert seen == {(r, c, w) for r, c in boards for w in (0, 1)}, seen
