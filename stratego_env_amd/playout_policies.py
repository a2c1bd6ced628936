"""Weight tables for weighted playouts (PackedStates.playout(..., weights=...), sgx_playout_weighted).  Host only, plain numpy.

A table is uint16 [4, 13, 14], read as weights[direction][moving piece type][what stands on the target cell], every entry in [0, 4095]:
  direction  0 = forward (the mover's perspective +r: towards the opponent's setup rows), 1 = backward, 2 / 3 = sideways (+c / -c);
  piece      the mover's true type 1..10 (rows 0, 11 = flag and 12 = bomb never move and are never read);
  target     0 = an empty cell, 1..12 = a piece of that type, 13 = a piece the mover has not identified (never read with see_all=True,
             which looks at the opponent's true type).
A move is drawn with probability weight / (sum of the weights of all valid moves); a weight of 0 is never drawn while another valid move
has a positive weight, and where every valid move has weight 0 the draw is uniform."""
import numpy as np

from .config import get_variant

SHAPE = (4, 13, 14)
WEIGHT_MAX = 4095
SPY, SCOUT, MINER, MARSHAL, FLAG, BOMB, UNKNOWN = 1, 2, 3, 10, 11, 12, 13


def uniform(weight=1):
    """Every move the same weight: plays, bit for bit, the games of the unweighted playout (any constant >= 1 does)."""
    if not 1 <= int(weight) <= WEIGHT_MAX:
        raise ValueError("weight must be in [1, %d]" % WEIGHT_MAX)
    return np.full(SHAPE, int(weight), dtype=np.uint16)


def from_reward_matrix(reward_matrix, temperature=1.0, direction=(1, 1, 1, 1), scale=64):
    """A softmax policy over the reference's move heuristic: reward_matrix[moved type, target type] as
    get_heuristic_rewards_from_move takes it, [13][13] or [13][14] (column 13 = a target of unknown type; a [13][13] matrix gives it the
    reward of column 0, an empty cell's).
    -> weights[dir][t][d] = clip(round(scale * direction[dir] * exp(reward[t][d] / temperature)), 0, 4095) as uint16 [4, 13, 14].
    Rounding is numpy's np.rint: to the nearest integer, halves to the even one -- so a product below 0.5 becomes weight 0 (never drawn
    while another move has weight), and exactly 0.5 does too.  Products above 4095 are clipped: raise the temperature or lower the scale
    to keep the ratios."""
    r = np.asarray(reward_matrix, dtype=np.float64)
    if r.shape not in ((13, 13), (13, 14)):
        raise ValueError("reward_matrix must be [13][13] or [13][14] = [moved type][target type] (got %s)" % (tuple(r.shape),))
    if not temperature > 0:
        raise ValueError("temperature must be positive")
    d = np.asarray(direction, dtype=np.float64)
    if d.shape != (4,) or (d < 0).any():
        raise ValueError("direction must be four factors >= 0: forward, backward, +c, -c")
    if r.shape[1] == 13:
        r = np.concatenate([r, r[:, :1]], axis=1)
    with np.errstate(over='ignore'):
        w = float(scale) * d[:, None, None] * np.exp(r / float(temperature))[None, :, :]
    return np.clip(np.rint(w), 0, WEIGHT_MAX).astype(np.uint16)


def attack_outcome(attacker, defender):
    """+1 the attacker wins (the flag's capture included), 0 both are removed, -1 the attacker is lost: the combat rule for an attacker
    1..10 on a defender 1..12."""
    if attacker == MINER and defender == BOMB:
        return 1
    if attacker == SPY and defender == MARSHAL:
        return 1
    if defender == FLAG:
        return 1
    if defender == BOMB:
        return -1
    if attacker == defender:
        return 0
    return 1 if attacker > defender else -1


def capture_biased(variant=None, forward=2, win=16, tie=3, quiet=4, loss=1, unknown=4):
    """A ready-made table from the combat rule: a winning attack weighs `win`, a quiet move (onto an empty cell) `quiet`, an even
    exchange `tie`, a losing attack `loss`, an attack on a piece of unknown type `unknown`; forward moves weigh `forward` times that.
    win > quiet > loss keeps the order the name promises.  `variant` (a name or a Variant; None = any) is only checked to exist: the
    combat rule, and so the table, is the same on every board."""
    if not (win > quiet > loss >= 0):
        raise ValueError("capture_biased wants win > quiet > loss >= 0")
    if variant is not None:
        get_variant(variant)
    w = np.zeros(SHAPE, dtype=np.int64)
    for t in range(1, 11):
        w[:, t, 0] = quiet
        w[:, t, UNKNOWN] = unknown
        for d in range(1, 13):
            o = attack_outcome(t, d)
            w[:, t, d] = win if o > 0 else tie if o == 0 else loss
    w[0] *= int(forward)
    if w.max() > WEIGHT_MAX:
        raise ValueError("a weight exceeds %d" % WEIGHT_MAX)
    return w.astype(np.uint16)
