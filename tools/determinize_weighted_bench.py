"""sgx_determinize_weighted next to sgx_determinize on the same roots: 65,536 Barrage and 65,536 Standard records taken 100 rollout steps
into their games; the uniform call (the baseline: its kernel is the parent commit's), the weighted call with the constant table
(beliefs.uniform) and with beliefs.setup_prior, each with one table for all records, and the setup prior once more as one table per
record (stride 2 * 12 * cells).  The calls run interleaved in one process, 100 launches each per repetition after a warm-up, five
repetitions, HIP-event time; min / median and every repetition are printed.  Ends with the kernels' register / LDS / scratch figures
(tools/kernel_notes.py).
    python tools/determinize_weighted_bench.py [variant ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from stratego_env_amd import _lib, beliefs, build as hip_build  # noqa: E402
from stratego_env_amd.procedural_env import PackedStates  # noqa: E402
from stratego_env_amd.vec_env import VecStrategoEnv  # noqa: E402
from tools.kernel_notes import kernel_notes  # noqa: E402

N, DEPTH, LAUNCHES, REPEATS = 65536, 100, 100, 5


def timed(fn, k):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(k):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / k


def main():
    names = sys.argv[1:] or ['barrage', 'standard']
    for name in names:
        env = VecStrategoEnv(name, N, seed=9, auto_reset=True, placement='plain')
        env.reset()
        env.rollout_steps(DEPTH)
        src, dst = PackedStates(name, N), PackedStates(name, N, seed=1)
        L, s, d = dst._vec._L, src._vec._h, dst._vec._h
        stream = dst._vec._stream()
        _lib.check(L.sgx_copy_envs(s, None, env._h, None, N, stream), L)
        env.close()
        dev = dst.device
        hidden = torch.empty((N,), dtype=torch.int32, device=dev)
        off = torch.empty((N,), dtype=torch.int32, device=dev)
        const = torch.from_numpy(beliefs.uniform(name).astype(np.int16)).to(dev)
        prior = torch.from_numpy(beliefs.setup_prior(name).astype(np.int16)).to(dev)
        each = prior[None].expand(N, -1, -1, -1).contiguous()                # one table per record: N x 2 x 12 x cells x 2 B
        T = prior.numel()

        def weighted(table, stride):
            return lambda i: L.sgx_determinize_weighted(d, s, None, 0, table.data_ptr(), stride, i, hidden.data_ptr(), off.data_ptr(), stream)
        calls = (('sgx_determinize', lambda i: L.sgx_determinize(d, s, None, 0, i, hidden.data_ptr(), stream)),
                 ('weighted, constant table', weighted(const, 0)),
                 ('weighted, setup prior', weighted(prior, 0)),
                 ('weighted, prior per record', weighted(each, T)))
        for _, fn in calls:                                                 # warm-up, and every call works
            for i in range(20):
                _lib.check(fn(i), L)
        ts = {k: [] for k, _ in calls}
        for _ in range(REPEATS):
            for k, fn in calls:
                ts[k].append(timed(fn, LAUNCHES))
        rec = dst._vec.record_bytes
        for k, _ in calls:
            t = sorted(ts[k])
            print("%-9s %6d records of %4d B, %d steps in   %-27s min %.1f / median %.1f us per launch (%s)   %.2f G records/s"
                  % (name, N, rec, DEPTH, k, t[0], t[REPEATS // 2], " ".join("%.1f" % x for x in ts[k]), N / t[REPEATS // 2] * 1e-3), flush=True)
        _lib.check(weighted(prior, 0)(0), L)
        torch.cuda.synchronize()
        print("%-9s hidden cells dealt per record: mean %.1f, max %d; setup prior: %.2f %% of the records with a piece on a weight-0 cell; table %d B"
              % (name, float(hidden.float().mean()), int(hidden.max()), 100.0 * float((off > 0).float().mean()), 2 * T), flush=True)
        src.close(); dst.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'determinize' in kname:
            print("%-70s vgpr %3d sgpr %3d scratch %4d static lds %6d (+ dynamic: 4 x (record + 3 / 2 bytes per cell, cells rounded to 64))"
                  % (kname[:70], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
