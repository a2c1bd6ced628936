"""count_moves + expand_all against the way all children of a batch of nodes were obtained before them, on the same roots.

Workload: 65,536 Barrage roots, 100 rollout steps after reset() (setups from the variant's table, no auto-reset); all their children, written
window after window into ONE pool of a fixed capacity.
  (a) count        sgx_count_moves alone: the counts and their int64 offsets
  (b) expand_all   sgx_expand_all over all children, in windows of the pool (offsets from (a), not timed again)
  (c) mask way     what it replaces, with calls the parent commit has: the 1-D mask of every root (sgx_observe, SGX_STEP_MASK_1D),
                   nonzero() (a host synchronisation), the parent / action index tensors, sgx_expand over the same windows
  (d) expand       sgx_expand alone on the (parent, action) pairs of (c), already on the device: the given-action kernel, the yardstick
                   of the child kernel, which regenerates the root's mask and takes the k-th entry on top of it
The four run interleaved in one process, HIP events around each, REPEATS repetitions after a warm-up of one each; every repetition, min and
median are printed, then children/s by the median and the ratios (b)/(d) and (c)/((a)+(b)).  The tool checks that (b) and (c) make the same
multiset of children per root.
    python tools/children_bench.py [variant] [--games N] [--steps T] [--capacity C]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, T, CAPACITY, REPEATS = 65536, 100, 262144, 5


def main():
    import torch
    from stratego_env_amd import build as hip_build
    from stratego_env_amd.procedural_env import PackedStates
    from stratego_env_amd.vec_env import VecStrategoEnv
    from tools.kernel_notes import kernel_notes
    args = sys.argv[1:]
    name = next((a for a in args if not a.startswith('--') and not a.isdigit()), 'barrage')
    n = int(args[args.index('--games') + 1]) if '--games' in args else N
    steps = int(args[args.index('--steps') + 1]) if '--steps' in args else T
    cap = int(args[args.index('--capacity') + 1]) if '--capacity' in args else CAPACITY

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
    env.rollout_steps(steps, emit_obs=False, emit_mask=False)
    roots, dst = PackedStates(name, n), PackedStates(name, cap)
    roots.copy_from(env)
    env.close()
    dev = roots.device
    out = {}

    def count():
        out['counts'], out['offsets'] = roots.count_moves()

    count()
    total = int(out['offsets'][-1])
    firsts = list(range(0, total, cap))

    def expand_all():
        for first in firsts:
            out['children'] = dst.expand_all(roots, offsets=out['offsets'], first_child=first)

    def pairs():
        mask = roots.valid_moves_as_1d_mask()
        nz = torch.nonzero(mask[:, :-1])                                    # (the no-op entry is no child; a host synchronisation)
        m = nz.shape[0]
        pad = len(range(0, m, cap)) * cap - m                               # sgx_expand fills the whole pool: the last window is padded
        parent = torch.cat([nz[:, 0].to(torch.int32), torch.zeros(pad, dtype=torch.int32, device=dev)])
        action = torch.cat([nz[:, 1].to(torch.int32), torch.full((pad,), mask.shape[1] - 1, dtype=torch.int32, device=dev)])
        out['pairs'] = (parent, action, m)

    def expand():
        parent, action, m = out['pairs']
        for first in range(0, m, cap):
            dst.expand(roots, action[first:first + cap], parent_index=parent[first:first + cap])

    def mask_way():
        pairs()
        expand()

    # warm-up, and both ways make the same children: per root the same number, and the same multiset of records in the first window
    expand_all()
    mask_way()
    parent, action, m = out['pairs']
    assert m == total, "the mask way and count_moves agree about the number of children"
    assert torch.equal(torch.bincount(parent[:m].long(), minlength=n).to(torch.int32), out['counts'])
    chk = PackedStates(name, min(8192, total))                              # (a small pool: its int64 export is what gets compared)
    w, width = chk.n, roots._vec.variant.action_size
    res = chk.expand_all(roots, offsets=out['offsets'], first_child=0, actions_1d=True)
    key_new = res.parent.long() * width + res.action.long()
    rec_new = chk.unpack()[0][torch.argsort(key_new)]
    chk.expand(roots, action[:w], parent_index=parent[:w])
    key_old = parent[:w].long() * width + action[:w].long()
    rec_old = chk.unpack()[0][torch.argsort(key_old)]
    # (both windows hold the children of the same leading roots; compare up to the last whole root)
    whole = int(out['offsets'][int(res.parent[w - 1])]) if w < total else w
    assert torch.equal(torch.sort(key_new)[0][:whole], torch.sort(key_old)[0][:whole]), "the same (parent, action) pairs"
    assert torch.equal(rec_new[:whole], rec_old[:whole]), "the same children"
    chk.close()

    kinds = (('(a) count', count), ('(b) expand_all', expand_all), ('(c) mask way', mask_way), ('(d) expand', expand))
    ts = {k: [] for k, _ in kinds}
    for _ in range(REPEATS):
        for k, fn in kinds:
            ts[k].append(timed(fn))
    print("%s, %d roots %d rollout steps after reset(), %d children (mean %.1f per root, %d roots without one), %d windows of a pool of %d"
          % (name, n, steps, total, total / n, int((out['counts'] == 0).sum()), len(firsts), cap), flush=True)
    med = lambda k: sorted(ts[k])[REPEATS // 2]
    for k, _ in kinds:
        t = sorted(ts[k])
        per = n if k == '(a) count' else total
        print("%-15s %s ms (min %.3f, median %.3f; %.3f G %s/s by the median)" % (k, " / ".join("%.3f" % x for x in ts[k]), t[0], med(k), per / med(k) / 1e6,
                                                                                 'roots' if k == '(a) count' else 'children'), flush=True)
    print("(b) / (d): %.2fx per child; (c) / ((a) + (b)): %.2fx (medians)"
          % (med('(b) expand_all') / med('(d) expand'), med('(c) mask way') / (med('(a) count') + med('(b) expand_all'))), flush=True)
    for x in (roots, dst):
        x.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'count_kernel' in kname or 'children_kernel' in kname or 'scan_' in kname:
            print("%-70s vgpr %3d sgpr %3d scratch %4d lds %6d" % (kname[:70], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
