"""sgx_choose_actions on every kernel path, every answer compared with the interval-exact rule of tests/choose_rule.py (accept()).

The paths.  The host (stratego_mi355x.hip, sgx_choose_actions) launches choose_kernel<R, C, VEC, BITS>: VEC = 4 where NA % 4 == 0, the
logits are 16-byte and the mask 4-byte aligned, else VEC = 1; BITS for the int32 bit mask.  ChooseGeo (sgx_choose.h) gives the rest:
a row is one chunk of VEC actions per lane of the game, ROWS = ceil(ceil(NA / VEC) / LPG), and CACHE = ROWS * VEC <= 72 keeps the
game's logits in registers -- without it the per-row totals go through LDS and the search is a loop of its own.  LPG (sgx_layout.h) is
16 lanes per game up to 16 cells, 32 up to 32 cells, 64 above; a workgroup is 4 waves = 4 * 64 / LPG games.

    board             NA       lanes/game          VEC 4 rows     VEC 1 rows
    micro 3x4         132      16 (4 games/wave)   3, cached      9, cached
    tiny 4x4          208      16                  4, cached      13, cached
    c3x3              81       16                  -              6, cached
    fives 5x5         425      32 (2 games/wave)   -              14, cached
    medium 6x6        756      64                  3, cached      12, cached
    barrage 10x10     3,700    64                  15, cached     58, cached
    standard2 15x15   12,825   64                  -              201, LDS
    c12x12            6,480    64                  26, LDS        102, LDS
    c32x32            128,000  64                  500, LDS       2,000, LDS

(tests/test_choose_cpu.py::test_geometry_of_the_path_table holds the restatement in choose_rule.geo to this table.)

Every case below runs at every alignment: logits at 0 / 4 / 8 / 12 bytes off a 16-byte boundary x byte masks at 0 .. 3 bytes off (VEC 4
only at 0 / 0), and the bit mask at every logits alignment; misaligned tensors are views into a larger one.  The bit mask is the env's
own compact mask where the case uses the env's mask, else choose_rule.pack_bits.  The acceptance sets depend on (logits, mask, draw,
temperature) only, so they are computed once per case and shared by its 20 launches; and because the kernel's sums are integers, the 20
launches must also agree with EACH OTHER exactly (the header's promise: a draw depends on nothing but logits, mask, seed, game, turn).
Batch sizes: 1, one workgroup's games - 1 / + 0 / + 1, 211; at most 5 / 20 / 40 games on c32x32 / c12x12 / standard2.  The envs run
with env_id_offset != 0 and are stepped between the cases, so turns and game numbers differ."""
import numpy as np
import pytest

from tests import choose_rule as cr
from tests.boards import _board

pytestmark = pytest.mark.gpu

SEED, OFFSET = 99, 3
POISON = -7
TOY = ('micro', 'tiny', 'c3x3', 'fives')


class _Runner:
    """One env of n games and the launches of one case at every alignment."""

    def __init__(self, board, n):
        import torch
        from stratego_env_amd.vec_env import VecStrategoEnv
        self.torch, self.board, self.n, self.na = torch, board, n, cr.n_actions(board)
        self.env = VecStrategoEnv(_board(board), n, seed=SEED, env_id_offset=OFFSET, auto_reset=True, compact_outputs=True)
        assert self.env.R * self.env.Cc * self.env.K == self.na and self.env.compact_mask_words == cr.compact_words(self.na)
        self.env.reset()
        self.advance(3)
        dev = self.env.device
        self._lg = [torch.empty(n * self.na + 4, dtype=torch.float32, device=dev) for _ in range(4)]
        self._mb = [torch.empty(n * self.na + 4, dtype=torch.uint8, device=dev) for _ in range(4)]
        self._mw = [torch.empty(n * cr.compact_words(self.na) + 1, dtype=torch.int32, device=dev) for _ in range(2)]
        self.launches = 0

    def advance(self, steps=1):
        for _ in range(steps):
            self.env.sample_valid_actions()
            self.env.step(self.env.next_actions)
        info = self.env.env_info().cpu().numpy()
        self.r64 = cr.draws(SEED, OFFSET, info[:, 1], info[:, 0])
        self.r32 = [r >> 32 for r in self.r64]
        self.own = self.env.decode_mask().reshape(self.n, -1).cpu().numpy()
        assert np.array_equal(cr.unpack_bits(self.env.mask.cpu().numpy(), self.na), self.own)     # the packer's layout is the env's

    def run(self, lg, mask, temperature, own_bits=False, padding=False, kinds=('bytes', 'bits')):
        """-> int32 [launches, n]: the kernel's answers at every alignment of the logits and of the byte mask, and with the bit mask."""
        torch, n, na = self.torch, self.n, self.na
        dev = self.env.device
        lgs, mbs, mws = [], [], []
        src = torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32)).reshape(-1).to(dev)
        msrc = torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).reshape(-1).to(dev)
        wsrc = self.env.mask.reshape(-1) if own_bits else torch.from_numpy(cr.pack_bits(mask, padding=padding)).reshape(-1).to(dev)
        for k in range(4):
            self._lg[k].fill_(float('nan'))
            v = self._lg[k][k:k + n * na]
            v.copy_(src)
            assert v.data_ptr() % 16 == 4 * k
            lgs.append(v.view(n, na))
            self._mb[k].fill_(1)
            m = self._mb[k][k:k + n * na]
            m.copy_(msrc)
            assert m.data_ptr() % 4 == k
            mbs.append(m.view(n, na))
        for k in range(2):
            self._mw[k].fill_(-1)
            w = self._mw[k][k:k + wsrc.numel()]
            w.copy_(wsrc)
            mws.append(w.view(n, -1))
        combos = ([(lgs[a], mbs[b]) for a in range(4) for b in range(4)] if 'bytes' in kinds else []) + \
                 ([(lgs[a], mws[a % 2]) for a in range(4)] if 'bits' in kinds else [])
        got = []
        for l, m in combos:
            out = torch.full((n,), POISON, dtype=torch.int32, device=dev)
            res = self.env.choose_actions(l, temperature=temperature, mask=m, out=out)
            assert res is out
            got.append(out)
        self.launches += len(combos)
        return torch.stack(got).cpu().numpy()

    def close(self):
        self.env.close()


def _check(board, case_name, n, got, sets, mask, lg):
    """Every launch's answer for every game: written, inside the acceptance set, a valid action below NA; all launches agree."""
    na = mask.shape[1]
    assert (got != POISON).all(), (board, case_name, n, 'an entry of out was not written')
    assert (got == got[0]).all(), (board, case_name, n, 'the paths disagree', np.argwhere(got != got[0])[:4].tolist())
    for e in range(n):
        a = int(got[0, e])
        assert a in sets[e], (board, case_name, n, e, a, sorted(sets[e])[:6])
        assert -1 <= a < na
        if a >= 0:
            assert mask[e, a] != 0 and not np.isnan(lg[e, a]) and lg[e, a] != -np.inf


def _run_cases(board, cases, exact=False):
    launches = 0
    for n in cr.batch_sizes(board):
        run = _Runner(board, n)
        try:
            for ci, case in enumerate(cases):
                rots = range(0, len(cr.lone_positions(board)), n) if case[4] == 'lone' else (0,)
                for rot in rots:
                    lg, mask, temperature, sets, first = cr.settled_inputs(board, case, n, SEED + ci, run.r32, own_mask=run.own, rot=rot)
                    many = sum(1 for s in sets if len(s) > 1)
                    assert many <= cr.AMBIGUITY_CAP * n, (board, case[0], n)                # the cap, on the inputs actually used
                    if exact:
                        assert many == 0, (board, case[0], n)
                    got = run.run(lg, mask, temperature, own_bits=case[4] == 'own')
                    _check(board, case[0], n, got, sets, mask, lg)
                    if case[1] == 'equal':                                               # a row total of 2^31 on 64 lanes, 2^40 in all on 32x32
                        want = [(r * cr.n_actions(board)) >> 32 for r in run.r32]
                        assert got[0].tolist() == want, (board, n)
                    if temperature == 0.0:
                        for e in range(n):
                            if got[0, e] >= 0:
                                assert lg[e, got[0, e]] == np.nanmax(np.where(mask[e] != 0, lg[e], -np.inf)), (board, case[0], e)
                run.advance()
            launches += run.launches
        finally:
            run.close()
    return launches


@pytest.mark.parametrize('sigma', cr.SIGMAS)
@pytest.mark.parametrize('board', list(cr.BOARDS))
def test_random_logits_on_every_path(board, sigma):
    """Normal logits x sigma at T in {0, 1e-30, 0.05, 1, 7, 3e38} with the env's mask and the all-valid mask: every answer of every
    launch is in accept(), is a valid action and is below NA."""
    assert _run_cases(board, [c for c in cr.RANDOM_CASES if c[2] == sigma]) > 0


@pytest.mark.parametrize('board', list(cr.BOARDS))
def test_exact_cases_on_every_path(board):
    """One acceptable answer, so equality: two-level logits {0, -1000} with every mask family (the env's, all valid, alternate, a lone
    valid action at 0, NA - 1, either side of the first and the last whole row's boundaries and inside the final partial row, empty),
    3-7 planted ties of the maximum at T = 0 and T = 1, equal logits with every action valid (action floor(r32 * NA / 2^32))."""
    assert _run_cases(board, cr.EXACT_CASES, exact=True) > 0


@pytest.mark.parametrize('board', list(cr.BOARDS))
def test_special_values_on_every_path(board):
    """NaN / -inf / +inf stripes: NaN and -inf are never chosen, +inf wins (checked through accept() and _check)."""
    assert _run_cases(board, cr.SPECIAL_CASES) > 0


@pytest.mark.parametrize('board', list(cr.BOARDS))
def test_padding_bits_of_the_bit_mask_are_not_actions(board):
    """Every bit beyond NA set in the packed mask: the answers are those without them, never an action >= NA."""
    case = cr.EXACT_CASES[0]
    for n in cr.batch_sizes(board):
        run = _Runner(board, n)
        try:
            lg, mask, temperature, sets, _ = cr.settled_inputs(board, case, n, SEED, run.r32, own_mask=run.own)
            assert all(len(s) == 1 for s in sets)
            got = run.run(lg, mask, temperature, padding=True, kinds=('bits',))
            _check(board, 'padding', n, got, sets, mask, lg)
        finally:
            run.close()


@pytest.mark.parametrize('board', TOY)
def test_mixed_waves(board):
    """Boards with 2 or 4 games per wave: game e has an empty mask if (e + rot) % 3 == 0, only -inf / NaN logits if == 1, and is live
    otherwise -- for rot = 0, 1, 2, so a live game sits in every slot of a wave next to games that left early -- in batches that end
    inside a wave and inside a workgroup.  Dead games get exactly -1, live games the rule's answer; every entry of the poisoned `out`
    is written."""
    for n in cr.batch_sizes(board):
        run = _Runner(board, n)
        try:
            for rot in range(3):
                lg, mask, temperature, kind = cr.mixed_inputs(board, n, SEED + rot, rot, own_mask=run.own)
                sets = cr.accept_batch(lg, mask, run.r32, temperature)
                assert all(sets[e] == {-1} for e in range(n) if kind[e] != 2) and all(-1 not in sets[e] for e in range(n) if kind[e] == 2)
                assert sum(1 for s in sets if len(s) > 1) <= cr.AMBIGUITY_CAP * n
                got = run.run(lg, mask, temperature)
                _check(board, 'mixed rot %d' % rot, n, got, sets, mask, lg)
                run.advance()
        finally:
            run.close()


def test_the_wrapper_refuses_what_it_cannot_pass_on():
    """choose_actions raises before any launch -- only with inputs that stay inside their own allocation even if it did not: a
    transposed [NA, N] byte mask, an int64 tensor of N * NA elements, an int64 `out` of N entries."""
    import torch
    from stratego_env_amd.vec_env import VecStrategoEnv
    n = 8
    env = VecStrategoEnv('tiny', n, seed=1)
    env.reset()
    na = env.R * env.Cc * env.K
    lg = torch.zeros((n, na), device=env.device)
    out = torch.full((n,), POISON, dtype=torch.int32, device=env.device)
    transposed = torch.ones((na, n), dtype=torch.uint8, device=env.device).t()
    assert transposed.shape == (n, na) and not transposed.is_contiguous()
    for bad in (transposed, torch.ones((n, na), dtype=torch.int64, device=env.device)):
        with pytest.raises(ValueError):
            env.choose_actions(lg, mask=bad, out=out)
    with pytest.raises(ValueError):
        env.choose_actions(lg, out=torch.full((n,), POISON, dtype=torch.int64, device=env.device))
    torch.cuda.synchronize()
    assert bool((out == POISON).all())                                  # nothing was launched
    assert bool((env.choose_actions(lg, mask=env.mask.bool(), out=out) >= 0).all())      # bool bytes are bytes
    env.close()
