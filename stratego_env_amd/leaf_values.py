"""Leaf-value tables (PackedStates.set_leaf_values, sgx_set_leaf_values).  Host only, plain numpy.

A table is int16 [2, 14, cells], read as table[half][piece][cell]:
  half   0 = "mine": the worth of an own piece of true type 1..12 (rows 0 and 13 are never read);
         1 = "theirs": the worth of an opponent's piece as the player sees it, 1..12 = a revealed type, 13 = a piece not identified yet
             (never read with see_all=True, which looks at the opponent's true type); row 0 is never read;
  cell   r * columns + c in the perspective of the piece's OWNER: row 0 is the owner's back row, the last row the far side of the
         board, for either player.
A position that is not over is worth clamp(mine - theirs, -limit, limit) / denom to a player.  `denom` is the caller's: the sum of a
side's piece values (side_total) keeps a material-only table inside +-1."""
import numpy as np

from .config import get_variant

ROWS = 14
SPY, SCOUT, MINER, MARSHAL, FLAG, BOMB, UNKNOWN = 1, 2, 3, 10, 11, 12, 13
# Default worth of a piece by type, index = type code (0 unused): the ranks by their number, doubled from the general up (the two pieces a
# side cannot replace), the spy as much as a captain-to-major (it is the marshal's only attacker), the miner above its rank (bombs), the
# bomb like a lieutenant-to-captain, the flag far above everything else together -- so that no exchange is worth the flag.
DEFAULT_VALUES = (0, 45, 15, 35, 20, 30, 40, 50, 65, 90, 140, 1000, 40)


def _variant(variant):
    return variant if hasattr(variant, 'piece_counts') else get_variant(variant)


def _values(values):
    v = np.asarray(DEFAULT_VALUES if values is None else values)
    if v.shape != (13,) or v.dtype.kind not in 'iu':
        raise ValueError("values must be 13 integers, index = piece type code 1..12 (entry 0 is not read)")
    return v.astype(np.int64)


def side_total(variant, values=None):
    """The sum of the values of one side's pieces: a `denom` that keeps a material-only table inside +-1."""
    v, vals = _variant(variant), _values(values)
    return int(sum(int(n) * int(vals[t]) for t, n in enumerate(v.piece_counts, start=1)))


def _checked(table):
    if table.min() < -32768 or table.max() > 32767:
        raise ValueError("an entry leaves int16: scale the values down")
    return table.astype(np.int16)


def material(variant, values=None, unknown=None):
    """Piece values alone, the same on every cell: table[0][t][:] = table[1][t][:] = values[t] for t in 1..12 and table[1][13][:] =
    unknown.  values: 13 integers indexed by type code (default DEFAULT_VALUES: spy 45, scout 15, miner 35, sergeant 20, lieutenant 30,
    captain 40, major 50, colonel 65, general 90, marshal 140, flag 1000, bomb 40); unknown: the worth of a piece not identified yet
    (default: the mean value of the variant's piece multiset, rounded to the nearest integer, halves to even)."""
    v, vals = _variant(variant), _values(values)
    counts = np.asarray(v.piece_counts, dtype=np.int64)
    if unknown is None:
        unknown = int(np.rint((counts * vals[1:]).sum() / max(int(counts.sum()), 1)))
    t = np.zeros((2, ROWS, v.rows * v.columns), dtype=np.int64)
    t[:, 1:13, :] = vals[1:, None]
    t[1, UNKNOWN, :] = int(unknown)
    return _checked(t)


def with_advance(table, per_row, rows=None):
    """`table` plus a bonus for how far a MOVABLE piece has advanced: per_row * r on perspective row r (r = 0 the owner's back row), added
    to the rows of types 1..10 of both halves and to "theirs" 13 (an unidentified piece may be movable; flags and bombs stay put).
    rows: the board's rows (default: the square root of the cell count, for square boards).  -> a new int16 table."""
    t = np.asarray(table).astype(np.int64)
    if t.ndim != 3 or t.shape[:2] != (2, ROWS):
        raise ValueError("table must have shape [2, 14, cells]")
    cells = t.shape[2]
    if rows is None:
        rows = int(round(cells ** 0.5))
        if rows * rows != cells:
            raise ValueError("%d cells are not a square board: pass rows=" % cells)
    rows = int(rows)
    if rows < 1 or cells % rows:
        raise ValueError("rows must divide the table's %d cells" % cells)
    bonus = int(per_row) * (np.arange(cells) // (cells // rows))
    t[:, 1:11, :] += bonus
    t[1, UNKNOWN, :] += bonus
    return _checked(t)


def from_piece_square(mine, theirs):
    """Two piece-square arrays -> a table.  mine: integers [12, cells] or [13, cells] for the own types 1..12 (a 13th row is refused:
    an own piece is never unknown); theirs: [12, cells] (unknown pieces weigh 0) or [13, cells] (row 12 = a piece not identified)."""
    m, th = np.asarray(mine), np.asarray(theirs)
    if m.dtype.kind not in 'iu' or th.dtype.kind not in 'iu':
        raise ValueError("piece-square arrays must have an integer dtype: round them yourself")
    if m.ndim != 2 or m.shape[0] != 12:
        raise ValueError("mine must have shape [12, cells]: one row per own piece type 1..12")
    if th.ndim != 2 or th.shape[0] not in (12, 13) or th.shape[1] != m.shape[1]:
        raise ValueError("theirs must have shape [12, cells] or [13, cells] with mine's cells")
    t = np.zeros((2, ROWS, m.shape[1]), dtype=np.int64)
    t[0, 1:13] = m
    t[1, 1:1 + th.shape[0]] = th
    return _checked(t)
