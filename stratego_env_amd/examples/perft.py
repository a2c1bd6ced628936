"""perft: how many positions lie d moves below the current positions of an env's games, for d = 0 .. depth -- the classic check of a move
generator, here as an example of level-by-level tree walking with count_moves / expand_all on packed records.

    nodes[0] = the games, nodes[d + 1] = the sum of the valid moves of all positions at depth d (a finished game and a mover without a move
    have none).

The frontier lives in pools of a fixed capacity, whatever the size of a level: a level with more positions than a pool holds is walked in
windows (expand_all's first_child), each window being counted -- and, above the last level, expanded in turn -- before the next one overwrites
it.  The deepest level is only counted, never written, so depth 3 ping-pongs between two pools; every further level takes one more.  The
only synchronisation is the one integer per window that says how many children there are.

    python -m stratego_env_amd.examples.perft [variant] [--games N] [--depth D] [--capacity C]
"""
import argparse

import torch

from stratego_env_amd.procedural_env import PackedStates
from stratego_env_amd.vec_env import VecStrategoEnv


def perft(env, depth, capacity=4096):
    """env: a live VecStrategoEnv (only read).  -> (nodes, windows): nodes[d] = positions at depth d below the env's games, windows[d] = the
    expand_all calls that wrote level d (0 for level 0 and for the deepest level, which is only counted)."""
    depth, capacity = int(depth), int(capacity)
    if depth < 0 or capacity < 1:
        raise ValueError("depth must be >= 0 and capacity >= 1")
    nodes, windows = [env.num_envs] + [0] * depth, [0] * (depth + 1)
    pools = [PackedStates(env.variant, capacity, device=env.device) for _ in range(max(depth - 1, 0))]

    def descend(src, n, level):
        """the records [0, n) of src are positions at depth `level`"""
        index = None if n == src.num_envs else torch.arange(n, dtype=torch.int32, device=env.device)
        _, offsets = src.count_moves(index)
        total = int(offsets[-1])                          # the window's one synchronisation
        nodes[level + 1] += total
        if level + 1 == depth:
            return
        dst = pools[level]
        for first in range(0, total, capacity):
            m = min(capacity, total - first)
            dst.expand_all(src, src_index=index, offsets=offsets, first_child=first, n=m)
            windows[level + 1] += 1
            descend(dst._vec, m, level + 1)

    try:
        if depth > 0:
            descend(env, env.num_envs, 0)
    finally:
        for p in pools:
            p.close()
    return nodes, windows


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
    nodes, windows = perft(env, a.depth, a.capacity)
    for d, (n, w) in enumerate(zip(nodes, windows)):
        print('depth %d: %d positions%s' % (d, n, ' (%d windows)' % w if w else ''))
    env.close()


if __name__ == '__main__':
    main()
