"""Guard bands (support code, no tests): the arena -- guard | payload | guard around every output tensor of a call --, the oracle stepped
alongside a guarded env, and the sweep of the pool-to-pool result tensors.  tests/test_gpu_guard_bands.py has the construction in full;
every pool-to-pool file runs pool_output_sweep on its own entry point.  Nothing here touches the GPU at import."""
import numpy as np
import pytest

from oracle import oracle as orc
from stratego_env_amd.config import VARIANTS
from tests.boards import _table
from tests.helpers import FOBS, MASK, POBS, oracle_cvariant

GUARD = 4096
GUARD_WORD = (0xAD, 0xDE, 0xC0, 0x7F)        # float32 0x7FC0DEAD: a NaN
POISON_WORD = (0x5A, 0x5A, 0xA5, 0x7F)       # float32 0x7FA55A5A: another one
U8_PHASES = (0, 1, 2, 3, 4, 5, 12, 13, 15, 127, 1023)
F32_ODD_PHASES = (0, 4, 8, 12, 124, 1020)    # odd boards: every float phase
F32_QUAD_PHASES = (0, 16, 112, 1008)         # boards with a multiple of 4 cells: 16-byte aligned (4, 8, 12 are SGX_EINVAL)
I32_PHASES = (0, 4, 8, 12)
OUTPUTS = ('obs', 'fobs', 'mask', 'reward', 'done', 'player', 'invalid_action', 'ending_invalid', 'final_obs', 'final_fobs', 'next_actions')


# ---- the arena ---------------------------------------------------------------------------------------------------------------------
class Arena:
    """guard | payload | guard.  `t` is the payload as a tensor of `dtype` and `shape`, `phase` bytes past a 1 KiB boundary."""

    def __init__(self, name, shape, dtype, phase, device):
        import torch
        self.name, self.shape, self.dtype, self.phase = name, tuple(int(x) for x in shape), dtype, int(phase)
        self.item = torch.empty((), dtype=dtype).element_size()
        assert self.phase % self.item == 0, "a tensor view needs its natural alignment: exactly the contract's minimum"
        self.nbytes = int(np.prod(self.shape)) * self.item
        self.game_bytes = self.nbytes // self.shape[0]
        total = GUARD + self.phase + self.nbytes + GUARD
        raw = torch.empty(total + 1024, dtype=torch.uint8, device=device)
        off = (-raw.data_ptr()) % 1024
        self.buf = raw[off:off + total]
        assert self.buf.data_ptr() % 1024 == 0
        self.lo, self.hi = GUARD + self.phase, GUARD + self.phase + self.nbytes
        idx = torch.arange(total, device=device) % 4
        self.guard_pat = torch.tensor(GUARD_WORD, dtype=torch.uint8, device=device)[idx]
        self.poison_pat = torch.tensor(POISON_WORD, dtype=torch.uint8, device=device)[idx[self.lo:self.hi]]
        self.buf.copy_(self.guard_pat)
        self.t = self.buf[self.lo:self.hi].view(dtype).view(self.shape)
        assert self.t.data_ptr() % 1024 == self.phase % 1024
        self.poison()

    def poison(self):
        self.buf[self.lo:self.hi].copy_(self.poison_pat)

    def check_guards(self, what=''):
        import torch
        if torch.equal(self.buf[:self.lo], self.guard_pat[:self.lo]) and torch.equal(self.buf[self.hi:], self.guard_pat[self.hi:]):
            return
        bad = torch.nonzero(self.buf != self.guard_pat_with_payload()).flatten().cpu().numpy()
        rel = [int(b) - self.lo for b in bad]
        games = sorted({min(max(r // self.game_bytes, 0), self.shape[0] - 1) for r in rel})
        left = torch.nonzero(self.unwritten().view(self.shape[0], -1))
        pytest.fail("%s: %s (phase %d): %d guard bytes overwritten, payload-relative offsets %s ... %s (payload is %d bytes, negative = before it); games %s; "
                    "%d payload elements still hold the poison%s"
                    % (what, self.name, self.phase, len(rel), rel[:6], rel[-3:], self.nbytes, games[:8], len(left),
                       (', first: game-row %d element %d' % tuple(int(x) for x in left[0])) if len(left) else ''))

    def guard_pat_with_payload(self):
        g = self.guard_pat.clone()
        g[self.lo:self.hi] = self.buf[self.lo:self.hi]
        return g

    def unwritten(self):
        """bool per ELEMENT: it still holds the poison (an element, not a byte: a legitimate 0x5A inside an action is no poison)"""
        same = self.buf[self.lo:self.hi] == self.poison_pat
        return same.view(-1, self.item).all(dim=1).view(self.shape)

    def check_written(self, what='', rows=None):
        """every element (of the games `rows`, default all) has been written; rows given: the OTHER games keep the poison"""
        import torch
        u = self.unwritten().view(self.shape[0], -1)
        if rows is None:
            left = u
        else:
            sel = torch.zeros(self.shape[0], dtype=torch.bool, device=u.device)
            sel[torch.as_tensor(rows, dtype=torch.long, device=u.device)] = True
            left = u[sel]
            assert bool(u[~sel].all()), "%s: %s: a game outside the call's selection was written" % (what, self.name)
        if bool(left.any()):
            g, i = [int(x) for x in torch.nonzero(left)[0]]
            pytest.fail("%s: %s (phase %d): %d elements still hold the poison, first at game-row %d element %d (of %d per game)"
                        % (what, self.name, self.phase, int(left.sum()), g, i, u.shape[1]))

    def check_untouched(self, what=''):
        assert bool(self.unwritten().all()), "%s: %s was written by a call that must not touch it" % (what, self.name)

    def host(self):
        return self.t.cpu().numpy()


def _phase_set(k, quad):
    """The phases of one call's tensors: they differ from each other and move through the lists at different strides."""
    f = F32_QUAD_PHASES if quad else F32_ODD_PHASES
    u = U8_PHASES
    return {'obs': f[k % len(f)], 'fobs': f[(k + 1) % len(f)], 'final_obs': f[(k + 2) % len(f)], 'final_fobs': f[(k + 3) % len(f)],
            'mask': u[k % 11], 'done': u[(k + 3) % 11], 'player': u[(k + 5) % 11], 'invalid_action': u[(k + 7) % 11], 'ending_invalid': u[(k + 9) % 11],
            'reward': (0, 4)[k % 2], 'next_actions': I32_PHASES[(k + 1) % 4]}


def _swap_outputs(env, phases, names=OUTPUTS):
    """Replace the env's output tensors (read through data_ptr() on every call) by arena views; returns {name: Arena}."""
    ar = {}
    for k in names:
        t = getattr(env, k)
        if t is None:
            continue
        ar[k] = Arena(k, t.shape, t.dtype, phases.get(k, 0), env.device)
        setattr(env, k, ar[k].t)
    return ar


def _load_actions(env, acts):
    """the rollout calls play env.next_actions (in / out): a fresh arena gets the actions the chain stands at"""
    import torch
    env.next_actions.copy_(torch.from_numpy(np.ascontiguousarray(acts, dtype=np.int32)))


def _sync(env):
    import torch
    torch.cuda.synchronize(env.device)


def _guards(arenas, what):
    for a in arenas.values():
        a.check_guards(what)


# ---- the oracle, stepped alongside ---------------------------------------------------------------------------------------------------
class Oracle:
    """`n` oracle games that mirror a VecStrategoEnv(seed, env_id_offset=g0); step(acts) plays one step and returns what every output
    tensor must hold afterwards (the same bookkeeping as tests/step_checks.py: check_step_vs_oracle)."""

    def __init__(self, name, seed, g0, n, auto_reset=True, channel_mode='extended'):
        v = VARIANTS[name]
        self.name, self.v, self.seed, self.g0, self.n, self.auto_reset = name, v, seed, g0, n, auto_reset
        self.cv = oracle_cvariant(name, setups=_table(name))
        self.envs = []
        for e in range(n):
            oe = orc.OracleEnv(v.rows, v.columns, v.max_turns, v.obstacle_locations, v.piece_counts, observation_mode='both_observations',
                               obs_channel_mode=channel_mode)
            oe.reset(initial_state_override=orc.reset_state(self.cv, seed, g0 + e, 0))
            oe.game_no = 0
            self.envs.append(oe)
        self.cur = [oe._obs(1) for oe in self.envs]
        self.finished = [False] * n
        self.games_done = 0

    def drawn(self, e):
        oe = self.envs[e]
        return orc.sample_action(self.cur[e][MASK].astype(np.uint8), self.seed, self.g0 + e, oe.game_no, int(oe.state[5, 0, 0]))

    def current(self):
        return {'mask': np.stack([c[MASK] for c in self.cur]).astype(np.uint8), 'obs': np.stack([c[POBS] for c in self.cur]),
                'fobs': np.stack([c[FOBS] for c in self.cur]), 'player': np.asarray([oe.player for oe in self.envs], dtype=np.int8),
                'next_actions': np.asarray([self.drawn(e) for e in range(self.n)], dtype=np.int32)}

    def step(self, acts):
        n = self.n
        x = {'invalid_action': np.zeros(n, np.uint8), 'done': np.zeros(n, np.uint8), 'ending_invalid': np.zeros(n, np.uint8),
             'reward': np.zeros((n, 2), np.float32), 'final': {}, 'legal': np.ones(n, bool)}
        for e, oe in enumerate(self.envs):
            try:
                if self.finished[e]:
                    raise ValueError
                o, rew, done, info = oe.step({oe.player: int(acts[e])})
            except ValueError:
                x['invalid_action'][e], x['done'][e], x['legal'][e] = 1, (1 if self.finished[e] else 0), False
                continue
            if done['__all__']:
                self.games_done += 1
                x['done'][e] = 1
                x['reward'][e] = (rew[1], rew[-1])
                x['ending_invalid'][e] = 1 if info[1]['game_result_was_invalid'] else 0
                x['final'][e] = (o[1], o[-1])
                if self.auto_reset:
                    oe.game_no += 1
                    o = oe.reset(initial_state_override=orc.reset_state(self.cv, self.seed, self.g0 + e, oe.game_no))
                else:
                    self.finished[e] = True
            self.cur[e] = o[oe.player]
        x.update(self.current())
        return x

    def states(self):
        return np.stack([oe.state for oe in self.envs]), np.asarray([oe.player for oe in self.envs], dtype=np.int8)


def _compare(ar, x, what, emit_obs=True):
    """(3): the payloads against the oracle's step `x`.  Rewards / the max-turn flag of a REFUSED action are not the oracle's to say (it
    raises): those rows are only required to be written."""
    h = {k: a.host() for k, a in ar.items()}
    legal = x['legal'] if 'legal' in x else np.ones(len(x['player']), bool)
    for k in ('mask', 'player', 'next_actions', 'done', 'invalid_action'):
        if k in h and k in x:
            assert np.array_equal(h[k], x[k]), (what, k, 'first differing game', int(np.flatnonzero((h[k] != x[k]).reshape(len(x[k]), -1).any(1))[0]))
    for k in ('reward', 'ending_invalid'):
        if k in h and k in x:
            assert np.array_equal(h[k][legal], x[k][legal]), (what, k)
    for k in ('obs', 'fobs'):
        if emit_obs and k in h and h[k].dtype == np.float32:
            assert h[k].tobytes() == x[k].tobytes(), (what, k, 'first differing game',
                                                      int(np.flatnonzero((h[k].view(np.uint32) != x[k].view(np.uint32)).reshape(len(x[k]), -1).any(1))[0]))
    for k, key in (('final_obs', POBS), ('final_fobs', FOBS)):
        if k in h:
            for e, (o1, o2) in x.get('final', {}).items():
                assert h[k][e, 0].tobytes() == o1[key].tobytes() and h[k][e, 1].tobytes() == o2[key].tobytes(), (what, k, e)


def _written_after_step(ar, x, what, emit_obs=True, emit_mask=True):
    for k, a in ar.items():
        if k in ('final_obs', 'final_fobs'):
            a.check_written(what, rows=sorted(x['final'].keys()))            # terminal steps only; the other games' slots stay untouched
        elif (k in ('obs', 'fobs') and not emit_obs) or (k == 'mask' and not emit_mask):
            a.check_untouched(what)
        else:
            a.check_written(what)


def _make(name, n, seed=None, g0=500, channel_mode='extended', **kw):
    from stratego_env_amd.vec_env import VecStrategoEnv
    seed = 0x6A4D0000 + 131 * len(name) + n if seed is None else seed
    env = VecStrategoEnv(name, n, seed=seed, env_id_offset=g0, placement='plain', obs_channel_mode=channel_mode, **kw)
    return env, Oracle(name, seed, g0, n, auto_reset=kw.get('auto_reset', False), channel_mode=channel_mode)


def _play(ora, acts, n):
    """n oracle steps, each playing what the one before drew; returns the per-step expectations"""
    xs = []
    for _ in range(n):
        xs.append(ora.step(acts))
        acts = xs[-1]['next_actions'].copy()
    return xs


# ---- the sweep of a pool-to-pool call's result tensors -------------------------------------------------------------------------------
POOL_PHASES = ((0, 0), (1, 4), (3, 12), (13, 0))      # (byte phase of the uint8 / int8 tensors, byte phase of the float32 / int32 tensors)


def pool_arenas(specs, n, device, byte_phase=0, word_phase=0):
    """{name: Arena} for the output specs (name, width, dtype name) of a pool-to-pool call, [n, width] or [n] each"""
    import torch
    return {k: Arena(k, (n, w) if w > 1 else (n,), getattr(torch, t), word_phase if t in ('float32', 'int32') else byte_phase, device)
            for k, w, t in specs}


def pool_output_sweep(specs, device, make_inputs, call, want, what, after_call):
    """The result tensors of a pool-to-pool call between guard bands: at the four phase pairs of POOL_PHASES every guard holds, every
    element is written and the bytes are `want`'s; then each result pointer NULL in turn: every guard holds, the skipped tensor keeps
    its poison and the others are still right.
    specs: (name, width, dtype name) per output, [n, width] or [n]; want: {name: host array}, its rows give n.
    make_inputs(byte_phase, word_phase) -> whatever guarded inputs the call reads ({} for none);
    call(ptrs, ins) -> rc, ptrs = {name: data pointer or None}; it raises or returns non-zero on a refusal, which fails the sweep with
    the library's message (`what` is the entry point's name as its messages and these ones carry it);
    after_call(ins, skip): the file's own checks of the records and the inputs after every call (synchronised); skip is None in the
    phase sweep, else the name of the output that was NULL."""
    import torch
    from stratego_env_amd import _lib
    n = len(want[specs[0][0]])

    def run(ar, ins, skip=None):
        rc = call({k: (None if k == skip else a.t.data_ptr()) for k, a in ar.items()}, ins)
        assert rc == 0, (what, rc, _lib.load().sgx_last_error())
        torch.cuda.synchronize()

    for byte_phase, word_phase in POOL_PHASES:
        ar, ins = pool_arenas(specs, n, device, byte_phase, word_phase), make_inputs(byte_phase, word_phase)
        run(ar, ins)
        for k, a in ar.items():
            a.check_guards(what)
            a.check_written(what)
            assert a.host().tobytes() == want[k].tobytes(), (k, byte_phase, word_phase)
        after_call(ins, None)
    for skip in [k for k, _, _ in specs]:
        ar, ins = pool_arenas(specs, n, device), make_inputs(0, 0)
        run(ar, ins, skip)
        for k, a in ar.items():
            a.check_guards(what)
            if k == skip:
                a.check_untouched(what)
            else:
                assert a.host().tobytes() == want[k].tobytes(), (k, 'without', skip)
        after_call(ins, skip)
