"""What tracking piece origins costs (sgx_set_replay_origins), on the workload of tools/replay_bench.py: 65,536 games from reset()
(setups from the variant's table), T = 200 recorded actions per game, both layouts of the action tensor.
  plain dense / [T][N]      sgx_replay without the setting, this build
  parent dense / [T][N]     the same call in the PARENT commit's library (--parent-lib PATH: a build of the parent's sources), on the same start
                            records (the same seeded reset) and the same log -- the baseline: the untracked kernel is the code it was
  tracked dense / [T][N]    sgx_replay with the setting: the same games, and int16 [N][2][cells] labels
  follow                    beliefs.follow(setup_prior, labels) on the device -> one int16 [2][12][cells] table per record
  determinize(followed)     sgx_determinize_weighted with those per-record tables (belief_stride > 0)
All run interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; every repetition, the median and
min ... max are printed.  The tool checks that all replays leave the same records and that the tracked ones leave the same labels.
    python tools/origins_bench.py [variant] [--games N] [--steps T] [--parent-lib PATH]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, REPEATS = 65536, 200, 7
NEW_SYMBOLS = ('sgx_set_replay_origins', 'sgx_replay_origins_set')


def load_parent(path):
    """The parent commit's library under this package's binding: it lacks the two entry points this commit adds, which no untracked call
    reaches; they are bound to this build's so that the binding is complete."""
    from stratego_env_amd import _lib
    raw, here = C.CDLL(path), C.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        try:
            getattr(raw, sym)
        except AttributeError:
            setattr(raw, sym, getattr(here, sym))
    L = _lib._bind(raw)
    assert L.sgx_abi_version() == _lib.ABI_VERSION
    L.build_id = L.sgx_build_id().decode('ascii', 'replace')
    _lib._libs[path] = L
    return L


def main():
    import torch
    from stratego_env_amd import beliefs, build as hip_build
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tools.kernel_notes import kernel_notes
    args = sys.argv[1:]
    opts = {'--games': N, '--steps': T, '--parent-lib': None}
    for k in opts:
        if k in args:
            opts[k] = args[args.index(k) + 1]
    skip = {args.index(k) + 1 for k in opts if k in args}
    name = next((a for i, a in enumerate(args) if not a.startswith('--') and i not in skip), 'barrage')
    n, steps, parent = int(opts['--games']), int(opts['--steps']), opts['--parent-lib']

    def timed(fn):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)                                            # ms

    env = VecStrategoEnv(name, n, seed=9, auto_reset=False, placement='plain')
    env.reset()
    start, dst, worlds = PackedStates(name, n), PackedStates(name, n), PackedStates(name, n, seed=1)
    start.copy_from(env)
    log = torch.empty((steps, n), dtype=torch.int32, device=env.device)      # [T][N]
    for t in range(steps):
        over = env.env_info()[:, 2] != 0
        drawn = env.sample_valid_actions()
        log[t] = torch.where(over, torch.full_like(drawn, -1), drawn)       # (a finished game: an entry no replay reads)
        env.step(log[t], emit_obs=False)
    want = env.export_state()[0]
    played = env.env_info()[:, 0].float()
    dense = log.T.contiguous()                                               # [N][T]
    out = {}
    kinds = [('plain dense', lambda: out.__setitem__('pd', dst.replay(start, dense))),
             ('plain [T][N]', lambda: out.__setitem__('pt', dst.replay(start, log.T)))]
    if parent:
        load_parent(parent)
        p_env = VecStrategoEnv(name, n, seed=9, auto_reset=False, placement='plain', lib_path=parent)
        p_env.reset()                                                        # the same seeded reset: the same start records
        p_start = VecStrategoEnv(name, n, human_inits=False, outputs=False, lib_path=parent)
        p_dst = VecStrategoEnv(name, n, human_inits=False, outputs=False, lib_path=parent)
        p_env.snapshot(out=p_start)
        kinds += [('parent dense', lambda: p_dst.replay(p_start, dense)), ('parent [T][N]', lambda: p_dst.replay(p_start, log.T))]
    kinds += [('tracked dense', lambda: out.__setitem__('td', dst.replay(start, dense, track_origins=True))),
              ('tracked [T][N]', lambda: out.__setitem__('tt', dst.replay(start, log.T, track_origins=True)))]
    prior = None
    if name in ('barrage', 'standard'):
        prior = torch.from_numpy(beliefs.setup_prior(name).astype('int16')).to(env.device)
        kinds += [('follow', lambda: out.__setitem__('f', beliefs.follow(prior, out['td'].origins))),
                  ('determinize(followed)', lambda: out.__setitem__('h', worlds.determinize(dst, observer=0, draw=3, beliefs=out['f'], validate=False)))]
    # warm-up, and every way reaches the same records
    for k, fn in kinds:
        fn()
        if k.startswith(('plain', 'tracked')):
            assert torch.equal(dst.unpack()[0], want), k
        if k.startswith('parent'):
            assert torch.equal(p_dst.export_state()[0], want), k
    assert torch.equal(out['td'].origins, out['tt'].origins)
    assert torch.equal(out['pd'].applied.float(), played) and torch.equal(out['td'].applied, out['pd'].applied)
    ts = {k: [] for k, _ in kinds}
    for _ in range(REPEATS):
        for k, fn in kinds:
            ts[k].append(timed(fn))
    moves = float(played.sum())
    lab = out['td'].origins.long()
    cells = lab.shape[2]
    walked = (lab >= 0) & (lab != torch.arange(cells, device=lab.device))
    print("%s, %d games, %d recorded actions per game; moves applied per replay: %.0f (mean %.1f per game); pieces left %d, of them off their start cell %d"
          % (name, n, steps, moves, moves / n, int((lab >= 0).sum()), int(walked.sum())), flush=True)
    med = lambda k: sorted(ts[k])[REPEATS // 2]
    for k, _ in kinds:
        print("%-22s %s ms (median %.3f, min %.3f ... max %.3f)" % (k, " / ".join("%.3f" % x for x in ts[k]), med(k), min(ts[k]), max(ts[k])), flush=True)
    for lay in ('dense', '[T][N]'):
        line = "%-7s tracked / plain %.3fx" % (lay, med('tracked ' + lay) / med('plain ' + lay))
        if parent:
            line += "; plain / parent %.3fx; tracked / parent %.3fx" % (med('plain ' + lay) / med('parent ' + lay), med('tracked ' + lay) / med('parent ' + lay))
        print(line + " (medians)", flush=True)
    for x in (start, dst, worlds, env):
        x.close()
    if parent:
        for x in (p_env, p_start, p_dst):
            x.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'replay_kernel' in kname and ('ILi10ELi10ELi' in kname):
            print("%-84s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:84], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
