"""What the weighted sampler of sgx_playout_weighted costs per move, and what a biased policy does to the games, on the roots of
tools/playout_bench.py: 65,536 Barrage records (a) fresh from reset() and (b) 100 rollout steps into their games.

Legs, interleaved in one process, HIP events around each launch, REPEATS repetitions after a warm-up of one each (median and min .. max):
  uniform    sgx_playout.
  constant   sgx_playout_weighted with the constant table: the same games and the same number of moves as `uniform` (the tool checks the
             lengths), so (constant - uniform) / moves played is the sampler's cost per move.
  biased     playout_policies.capture_biased in the public view, and with SGX_PLAYOUT_SEE_ALL: ms, mean length, moves/s, the share of
             decisive endings (somebody won) and of move-limit endings.
    python tools/weighted_playout_bench.py [variant ...]

    python tools/weighted_playout_bench.py --ab OTHER_LIBRARY [--rounds 3] [variant ...]
sgx_playout of this build against another build of the library (the parent commit's) on the same roots: every round starts one process per
library, alternating (SGX_LIB_PATH + SGX_ALLOW_FOREIGN_BUILD=1; a library older than sgx_playout_weighted loads for this leg), each timing
REPEATS launches per root set; all repetitions of a library are pooled into its median and spread."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DEPTH, REPEATS = 65536, 100, 7
NEW_SYMBOL = 'sgx_playout_weighted'


def _allow_older_library():
    """a library built before sgx_playout_weighted existed may be bound for the legs that never call it"""
    import types
    from stratego_env_amd import _lib
    _lib.EXPORTED_SYMBOLS = tuple(s for s in _lib.EXPORTED_SYMBOLS if s != NEW_SYMBOL)
    bind = _lib._bind

    def bind_older(L):
        if not hasattr(L, NEW_SYMBOL):
            setattr(L, NEW_SYMBOL, types.SimpleNamespace())
        return bind(L)
    _lib._bind = bind_older


def _timed(torch, fn):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)                                            # ms


def _root_sets(name):
    """-> [(case, roots PackedStates)]"""
    from stratego_env_amd import _lib
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    out = []
    for case, depth in (('fresh', 0), ('%d steps in' % DEPTH, DEPTH)):
        env = VecStrategoEnv(name, N, seed=9, auto_reset=True, placement='plain')
        env.reset()
        if depth:
            env.rollout_steps(depth, emit_obs=False, emit_mask=False)
        roots = PackedStates(name, N)
        L = roots._vec._L
        _lib.check(L.sgx_copy_envs(roots._vec._h, None, env._h, None, N, roots._vec._stream()), L)
        env.close()
        out.append((case, roots))
    return out


def _spread(ts):
    t = sorted(ts)
    return "median %.2f ms (min %.2f, max %.2f, n %d)" % (t[len(t) // 2], t[0], t[-1], len(t))


def leg_uniform(names):
    """one process of the --ab run: times of sgx_playout with whatever library SGX_LIB_PATH names -> one JSON line"""
    if os.environ.get('SGX_ALLOW_FOREIGN_BUILD') == '1':
        _allow_older_library()
    import torch
    from stratego_env_amd.procedural_env import PackedStates
    out = {}
    for name in names:
        for case, roots in _root_sets(name):
            dst = PackedStates(name, N, seed=1)
            dst.playout(roots, draw=0)
            out['%s, %s' % (name, case)] = [_timed(torch, lambda: dst.playout(roots, draw=r + 1)) for r in range(REPEATS)]
            dst.close(); roots.close()
    print('LEG ' + json.dumps(out), flush=True)


def ab(other, rounds, names):
    here = {}
    for r in range(rounds):
        for tag, lib in (('other', other), ('this', None)):
            env = dict(os.environ)
            if lib:
                env.update(SGX_LIB_PATH=lib, SGX_ALLOW_FOREIGN_BUILD='1')
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--leg-uniform'] + names, env=env, capture_output=True, text=True, timeout=600)
            line = [l for l in p.stdout.splitlines() if l.startswith('LEG ')]
            if p.returncode != 0 or not line:
                sys.stdout.write(p.stdout + p.stderr)
                raise SystemExit("the %s leg of round %d failed (exit status %d)" % (tag, r, p.returncode))
            for case, ts in json.loads(line[0][4:]).items():
                here.setdefault(case, {}).setdefault(tag, []).extend(ts)
    for case, both in here.items():
        med = {k: sorted(v)[len(v) // 2] for k, v in both.items()}
        print("sgx_playout %-22s other library: %s" % (case, _spread(both['other'])), flush=True)
        print("sgx_playout %-22s this build:    %s; this - other = %+.2f ms by the medians; the other library's own repetitions span %.2f ms"
              % (case, _spread(both['this']), med['this'] - med['other'], max(both['other']) - min(both['other'])), flush=True)


def main():
    args = sys.argv[1:]
    names = [a for i, a in enumerate(args) if not a.startswith('--') and (i == 0 or args[i - 1] not in ('--ab', '--rounds'))] or ['barrage']
    if '--leg-uniform' in args:
        return leg_uniform(names)
    if '--ab' in args:
        rounds = int(args[args.index('--rounds') + 1]) if '--rounds' in args else 3
        return ab(os.path.abspath(args[args.index('--ab') + 1]), rounds, names)
    import torch
    from stratego_env_amd import build as hip_build, playout_policies as pol
    from stratego_env_amd.procedural_env import PackedStates
    from tools.kernel_notes import kernel_notes

    for name in names:
        biased = pol.capture_biased(name)
        legs = (('uniform', None, False), ('constant', pol.uniform(), False), ('biased public', biased, False), ('biased see_all', biased, True))
        for case, roots in _root_sets(name):
            dst = PackedStates(name, N, seed=1)
            res, ts = {}, {k: [] for k, _, _ in legs}

            def run(leg, draw):
                k, table, see_all = leg
                res[k] = dst.playout(roots, draw=draw, weights=table, see_all=see_all)

            for leg in legs:                                               # warm-up, and every leg plays every game to its end
                run(leg, 0)
                assert bool(res[leg[0]].done.all())
            for r in range(REPEATS):
                for leg in legs:
                    ts[leg[0]].append(_timed(torch, lambda: run(leg, r + 1)))
            assert torch.equal(res['uniform'].length, res['constant'].length) and torch.equal(res['uniform'].reward, res['constant'].reward), \
                "the constant table plays the uniform games"
            med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
            for k, _, _ in legs:
                length = res[k].length.double()
                moves = float(length.sum())
                decisive = float(((res[k].reward[:, 0].abs() == 1)).double().mean())
                print("%-9s %6d records, %-12s %-15s %s; length mean %.1f; %.2f G moves/s; decisive endings %.3f, move-limit endings %.3f"
                      % (name, N, case, k, _spread(ts[k]), float(length.mean()), moves / med[k] / 1e6, decisive,
                         float(res[k].ending_invalid.double().mean())), flush=True)
            moves = float(res['uniform'].length.double().sum())
            print("%-9s %6d records, %-12s sampler: (constant - uniform) / moves = (%.2f - %.2f) ms / %.3g moves = %.3f ns per move of the pool (%.1f %% of the uniform launch)"
                  % (name, N, case, med['constant'], med['uniform'], moves, (med['constant'] - med['uniform']) * 1e6 / moves,
                     100.0 * (med['constant'] - med['uniform']) / med['uniform']), flush=True)
            dst.close(); roots.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'playout' in kname:
            print("%-78s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:78], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
