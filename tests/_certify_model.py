"""TEST INFRASTRUCTURE: the table-certification criterion (include/sst.h,
sst_table_certify) restated in numpy, independent of the engine.

pair(r, m) is the 2-bit cell of mass m in row r: bits 2 * (C - 1 - m % C) of
word (r, m // C), bit0 low, bit1 the "left" bit.  Expected, reading only the
given words:
  row 0: pair(0, 0) = 3, every other cell 0
  row r >= 1: bit0(r, m) = [pair(r - 1, m) != 0]
              bit1(r, m) = [m >= w_r and pair(r, m - w_r) != 0]
Columns below the last must equal the expected word; the last column must be
expected & ((full << 2k) & full) for one k in [0, C] shared by all rows.
"""
import numpy as np

DT = {4: np.uint8, 8: np.uint16, 16: np.uint32, 32: np.uint64}


def certifiable(masses, C):
    return all(m >= C for m in masses[1:])


def _full(C):
    return (1 << (2 * C)) - 1


def _cells_set(x, C):
    alt = np.uint64(0x5555555555555555 & _full(C))
    return (x | (x >> np.uint64(1))) & alt


def _shifted(row, by):
    """out[c] = row[c - by], 0 where c - by < 0."""
    out = np.zeros_like(row)
    if by < len(row):
        out[by:] = row[:len(row) - by]
    return out


def expected_words(words, masses, C):
    """The unmasked expected word of every position, uint64[n_rows, n_cols]."""
    x = np.asarray(words).astype(np.uint64)
    full = np.uint64(_full(C))
    exp = np.zeros_like(x)
    exp[0, 0] = np.uint64(3 << (2 * C - 2))
    for r in range(1, x.shape[0]):
        step, shift = divmod(int(masses[r]), C)
        left = _cells_set(_shifted(x[r], step), C) >> np.uint64(2 * shift)
        if shift:
            left |= (_cells_set(_shifted(x[r], step + 1), C) << np.uint64(2 * (C - shift))) & full
        exp[r] = _cells_set(x[r - 1], C) | (left << np.uint64(1))
    return exp


def admissible_k(word, expected, C):
    """The k in [0, C] with word == expected & ((full << 2k) & full)."""
    full = _full(C)
    return {k for k in range(C + 1) if int(word) == int(expected) & ((full << (2 * k)) & full)}


def first_violation(words, masses, C):
    """None when the words pass, else (row, column) of the lowest row-major
    violation.  In the last column a row violates when no k fits it and every
    row above it."""
    x = np.asarray(words).astype(np.uint64)
    exp = expected_words(x, masses, C)
    last = x.shape[1] - 1
    found = []
    bad = np.argwhere(x[:, :last] != exp[:, :last])
    if len(bad):
        found.append((int(bad[0][0]), int(bad[0][1])))
    run = set(range(C + 1))
    for r in range(x.shape[0]):
        run &= admissible_k(x[r, last], exp[r, last], C)
        if not run:
            found.append((r, last))
            break
    return min(found) if found else None


def flip(words, row, col, bit):
    out = np.array(words, copy=True)
    out[row, col] ^= out.dtype.type(1 << bit)
    return out


def flip_left(words, C, row, col, cell=None):
    """A copy with the left bit of one cell of word (row, col) flipped, and the
    cell's index.  The cell keeps pair != 0 (its bit0 is set), so the upload
    check bit0(r + 1, m) == any(r, m) still holds; in the last row any cell
    does.  `cell`: that cell (mass % C), else the first that qualifies."""
    x = np.asarray(words)
    cells = range(C) if cell is None else [cell]
    for j in cells:
        if row == x.shape[0] - 1 or (int(x[row, col]) >> (2 * (C - 1 - j))) & 1:
            return flip(x, row, col, 2 * (C - 1 - j) + 1), j
    raise AssertionError(f"word ({row}, {col}) has no cell to flip")


def stray_last_column_bit(words, masses, C):
    """A copy with one left bit set in the last column outside the closure: the
    first cell of the last row's last word when its expected pair is 0 (every
    mask but the all-zero one keeps that cell)."""
    x = np.asarray(words)
    r, last = x.shape[0] - 1, x.shape[1] - 1
    assert not (int(expected_words(x, masses, C)[r, last]) >> (2 * C - 2)) & 3, "cell is inside the closure"
    return flip(x, r, last, 2 * C - 1)
