"""sgx_playout to the end of the game against the way the same outcomes were obtained before it existed, on the same roots.

Workload: 65,536 Barrage records (a) fresh from reset() and (b) 100 rollout steps into their games, and the same for Standard.
  playout   one sgx_playout launch, pool to pool, max_steps = 0; rewards, lengths and the final records written.
  baseline  sgx_copy_envs of the roots into a scratch handle (auto_reset=False), the mask-only observe and the draw of the first action that a
            handle needs after a copy, then rollout_steps(max_turns, emit_obs=False, emit_mask=False); the rewards are in `reward` afterwards.
            (A finished game stays unchanged under the no-op and keeps reporting its result, so every wave plays all max_turns steps.)
The two run interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; min and median are
printed together with every repetition, then the playout length distribution (mean, p50, p99, max) and mean length / max_turns: the share
of the baseline's steps that do work.  The two sides draw their moves from different RNG streams, so they play different games of the same
distribution from the same roots; the tool checks that both leave every game finished and prints both win rates.
    python tools/playout_bench.py [variant ...] [--cpu-work-ratio]
--cpu-work-ratio: no GPU -- the oracle plays the rule (tests/playout_rule.py) from 64 fresh roots per variant and prints mean length / max_turns."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DEPTH, REPEATS = 65536, 100, 5


def cpu_work_ratio(names, n=64):
    import numpy as np
    from oracle import oracle as orc
    from stratego_env_amd.config import VARIANTS
    from tests import playout_rule as pr
    from tests.helpers import oracle_cvariant
    for name in names:
        v = VARIANTS[name]
        cv = oracle_cvariant(name)
        states = np.stack([orc.reset_state(cv, 9, g, 0) for g in range(n)])
        length = pr.playout_batch(name, states, np.ones(n, dtype=np.int8), 1, 0, 0)[5]
        print("%-9s oracle, %d fresh roots (random setups): playout length mean %.1f, p50 %d, max %d of max_turns %d: work ratio %.3f"
              % (name, n, length.mean(), np.percentile(length, 50), length.max(), v.max_turns, length.mean() / v.max_turns), flush=True)


def main():
    names = [a for a in sys.argv[1:] if not a.startswith('--')] or ['barrage', 'standard']
    if '--cpu-work-ratio' in sys.argv:
        return cpu_work_ratio(names)
    import torch
    from stratego_env_amd import _lib, build as hip_build
    from stratego_env_amd.config import VARIANTS
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tools.kernel_notes import kernel_notes

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                            # ms

    for name in names:
        max_turns = VARIANTS[name].max_turns
        for case, depth in (('fresh', 0), ('%d steps in' % DEPTH, DEPTH)):
            env = VecStrategoEnv(name, N, seed=9, auto_reset=True, placement='plain')
            env.reset()
            if depth:
                env.rollout_steps(depth, emit_obs=False, emit_mask=False)
            roots = PackedStates(name, N)
            L = roots._vec._L
            _lib.check(L.sgx_copy_envs(roots._vec._h, None, env._h, None, N, roots._vec._stream()), L)
            env.close()
            dst = PackedStates(name, N, seed=1)
            scratch = VecStrategoEnv(name, N, seed=1, auto_reset=False, human_inits=False, placement='plain')
            out = {}

            def playout():
                out['res'] = dst.playout(roots, draw=out.get('n', 0))
                out['n'] = out.get('n', 0) + 1

            def baseline():
                _lib.check(L.sgx_copy_envs(scratch._h, None, roots._vec._h, None, N, scratch._stream()), L)
                scratch.observe(emit_obs=False)
                scratch.sample_valid_actions()
                scratch._next_actions_fresh = True
                scratch.rollout_steps(max_turns, emit_obs=False, emit_mask=False)

            playout(); baseline()                                           # warm-up, and both work
            assert bool(out['res'].done.all()) and bool(scratch.done.all()), "both sides play every game to its end"
            ts = {'playout': [], 'baseline': []}
            for _ in range(REPEATS):
                ts['playout'].append(timed(playout))
                ts['baseline'].append(timed(baseline))
            res = out['res']
            length = res.length.float()
            q = lambda p: float(torch.quantile(length, p))
            for k in ('playout', 'baseline'):
                t = sorted(ts[k])
                print("%-9s %6d records, %-12s %-8s %s ms (min %.2f, median %.2f)" % (name, N, case, k, " / ".join("%.2f" % x for x in ts[k]), t[0], t[len(t) // 2]), flush=True)
            print("%-9s %6d records, %-12s baseline / playout: %.2fx by the minima, %.2fx by the medians" % (
                name, N, case, min(ts['baseline']) / min(ts['playout']), sorted(ts['baseline'])[REPEATS // 2] / sorted(ts['playout'])[REPEATS // 2]), flush=True)
            print("%-9s %6d records, %-12s playout length mean %.1f, p50 %.0f, p99 %.0f, max %d; max_turns %d, of which the baseline plays all: work ratio %.3f (turn of the roots: mean %.1f)"
                  % (name, N, case, float(length.mean()), q(0.5), q(0.99), int(length.max()), max_turns, float(length.mean()) / max_turns,
                     float(roots._vec.env_info()[:, 0].float().mean())), flush=True)
            print("%-9s %6d records, %-12s player +1 wins: playout %.3f, baseline %.3f; max-turn endings: %.3f, %.3f" % (
                name, N, case, float((res.reward[:, 0] == 1).float().mean()), float((scratch.reward[:, 0] == 1).float().mean()),
                float(res.ending_invalid.float().mean()), float(scratch.ending_invalid.float().mean())), flush=True)
            for x in (roots, dst, scratch):
                x.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'playout_kernel' in kname:
            print("%-70s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:70], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
