"""sgx_determinize next to the two calls it sits between on the same pools: sgx_copy_envs (the pure record-traffic floor: read a record,
write a record) and sgx_expand (a full env.step() on the same traffic).  65,536 Barrage and 65,536 Standard records taken 100 rollout steps
into their games; the three calls run interleaved, 200 launches each per repeat after a warm-up, three repeats, HIP-event time; every
repeat is printed, so the spread is what the lines show.  Ends with the kernel's register / LDS / scratch figures (tools/kernel_notes.py).
    python tools/determinize_bench.py [variant ...]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from stratego_env_amd import _lib, build as hip_build  # noqa: E402
from stratego_env_amd.procedural_env import PackedStates  # noqa: E402
from stratego_env_amd.vec_env import VecStrategoEnv  # noqa: E402
from tools.kernel_notes import kernel_notes  # noqa: E402

N, DEPTH, LAUNCHES, REPEATS = 65536, 100, 200, 3


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
        acts = env.next_actions.clone()                                     # a valid spatial action of every record's mover
        src, dst = PackedStates(name, N), PackedStates(name, N, seed=1)
        L, s, d = dst._vec._L, src._vec._h, dst._vec._h
        stream = dst._vec._stream()
        _lib.check(L.sgx_copy_envs(s, None, env._h, None, N, stream), L)
        env.close()
        hidden = torch.empty((N,), dtype=torch.int32, device=dst.device)
        io = dst._vec._fill_io(acts, False, False, False, 0)
        io.auto_reset = 0
        io.mask_dev = None
        calls = (('sgx_copy_envs', lambda i: L.sgx_copy_envs(d, None, s, None, N, stream)),
                 ('sgx_determinize', lambda i: L.sgx_determinize(d, s, None, 0, i, hidden.data_ptr(), stream)),
                 ('sgx_expand', lambda i: L.sgx_expand(d, s, None, C.byref(io), stream)))
        for _, fn in calls:                                                 # warm-up, and every call works
            for i in range(20):
                _lib.check(fn(i), L)
        ts = {k: [] for k, _ in calls}
        for _ in range(REPEATS):
            for k, fn in calls:
                ts[k].append(timed(fn, LAUNCHES))
        assert int(dst._vec.invalid_action.sum()) == 0
        L.sgx_determinize(d, s, None, 0, 0, hidden.data_ptr(), stream)
        rec = dst._vec.record_bytes
        for k, _ in calls:
            med = sorted(ts[k])[REPEATS // 2]
            print("%-9s %6d records of %4d B, %d steps in   %-16s %s us per launch (median %.1f, spread %.1f)   %.2f G records/s   %.2f TB/s read + written"
                  % (name, N, rec, DEPTH, k, " / ".join("%.1f" % t for t in ts[k]), med, max(ts[k]) - min(ts[k]), N / med * 1e-3, 2 * N * rec / med * 1e-6), flush=True)
        print("%-9s hidden cells shuffled per record: mean %.1f, max %d" % (name, float(hidden.float().mean()), int(hidden.max())), flush=True)
        src.close(); dst.close()
    for kname, r in sorted(kernel_notes(hip_build.LIB_PATH).items()):
        if 'determinize_kernel' in kname or 'copy_records_kernel' in kname:
            print("%-70s vgpr %3d sgpr %3d scratch %4d static lds %6d (determinize: + 4 x (record + 3 bytes per cell, rounded to 64) dynamic)"
                  % (kname[:70], r['vgpr'], r['sgpr'], r['scratch'], r['lds']), flush=True)


if __name__ == '__main__':
    main()
