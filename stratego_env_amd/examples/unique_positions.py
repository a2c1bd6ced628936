"""unique positions: how many DIFFERENT positions lie d moves below the current positions of an env's games -- perft counts move paths, and
two paths may meet in one position (a transposition).  An example of position keys (state_keys) on top of the level-by-level walk of
examples/perft.py:

    positions[d] = the paths of length d (perft's nodes), distinct[d] = the different positions among their ends, by the state key
    WITHOUT the clock: turn count and max turns stay out, every other layer of the state and the mover go in.

The walk is perft's: count_moves -> expand_all in windows of pools of a fixed capacity.  Each window's keys (8 bytes per position) are kept
on the device, the positions themselves are overwritten by the next window; a level's distinct count is torch.unique over its keys.  Unlike
perft the deepest level is written too: its positions are what gets a key.

    python -m stratego_env_amd.examples.unique_positions [variant] [--games N] [--depth D] [--capacity C]
"""
import argparse

import torch

from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def unique_positions(env, depth, capacity=4096):
    """env: a live VecStrategoEnv (only read).  -> (positions, distinct): positions[d] = paths of length d below the env's games,
    distinct[d] = the different positions they end in (no-clock state keys)."""
    depth, capacity = int(depth), int(capacity)
    if depth < 0 or capacity < 1:
        raise ValueError("depth must be >= 0 and capacity >= 1")
    keys = [[env.state_keys(clock=False)]] + [[] for _ in range(depth)]
    pools = [PackedStates(env.variant, capacity, device=env.device) for _ in range(depth)]

    def descend(src, n, level):
        """the records [0, n) of src are positions at depth `level`"""
        index = None if n == src.num_envs else torch.arange(n, dtype=torch.int32, device=env.device)
        _, offsets = src.count_moves(index)
        total = int(offsets[-1])                          # the window's one synchronisation
        dst = pools[level]
        for first in range(0, total, capacity):
            m = min(capacity, total - first)
            dst.expand_all(src, src_index=index, offsets=offsets, first_child=first, n=m)
            keys[level + 1].append(dst.state_keys(index=None if m == capacity else torch.arange(m, dtype=torch.int32, device=env.device), clock=False))
            if level + 1 < depth:
                descend(dst._vec, m, level + 1)

    try:
        if depth > 0:
            descend(env, env.num_envs, 0)
        positions = [sum(int(k.numel()) for k in level) for level in keys]
        distinct = [int(torch.unique(torch.cat(level)).numel()) if level else 0 for level in keys]
    finally:
        for p in pools:
            p.close()
    return positions, distinct


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('variant', nargs='?', default='barrage')
    ap.add_argument('--games', type=int, default=4)
    ap.add_argument('--depth', type=int, default=3)
    ap.add_argument('--capacity', type=int, default=65536)
    ap.add_argument('--seed', type=int, default=0)
    a = ap.parse_args()
    env = VecStrategoEnv(a.variant, a.games, seed=a.seed, auto_reset=False, human_inits=False)
    env.reset()
    positions, distinct = unique_positions(env, a.depth, a.capacity)
    for d, (n, u) in enumerate(zip(positions, distinct)):
        print('depth %d: %d positions, %d distinct' % (d, n, u))
    env.close()


if __name__ == '__main__':
    main()
