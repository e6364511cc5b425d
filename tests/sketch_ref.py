"""The count sketch pinned in include/flcodec.h, restated in float64 numpy on the oracle's Philox: the cell and sign of
an element, the table of a vector, the weighted sum of tables and the median-of-rows estimate."""
import functools

import numpy as np

from oracle.compressors_ref import philox4x32_10

T = 1024
U = 2.0 ** -24


def philox_group(group, seed, counter):
    g = np.asarray(group, np.uint64)
    return philox4x32_10((g & np.uint64(0xFFFFFFFF)).astype(np.uint32), (g >> np.uint64(32)).astype(np.uint32),
                         np.uint32(counter & 0xFFFFFFFF), np.uint32(counter >> 32),
                         np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))


def cells(idx, cols, seed, rows=5):
    """(cell [k, rows] within a row's ``cols`` cells, sign [k, rows] of +-1.0) of the elements ``idx``."""
    i = np.asarray(idx, np.int64)
    NT = cols // T
    q, p, o, g = i // cols, (i % cols) // T, i % T, i // T
    x, y, _, _ = philox_group(q, seed, 0x100)
    A, B = (x.astype(np.int64) | 1) % NT, y.astype(np.int64) % NT
    # the table tile tau that receives source tile p: the one with (A tau + B) mod NT == p, by search
    tau = np.argmax((A[:, None] * np.arange(NT)[None, :] + B[:, None]) % NT == p[:, None], axis=1)
    cell, sign = np.empty((i.size, rows), np.int64), np.empty((i.size, rows))
    for j in range(rows):
        x, y, _, _ = philox_group(g, seed, 0x200 + j)
        a, b = (x.astype(np.int64) | 1) % T, y.astype(np.int64) % T
        cell[:, j] = T * tau + (a * o + b) % T
        w = np.stack(philox_group(i >> 7, seed, 0x300 + j), 1)[np.arange(i.size), (i >> 5) & 3]
        sign[:, j] = 1.0 - 2.0 * ((w >> (i & 31).astype(np.uint32)) & np.uint32(1))
    return cell, sign


@functools.lru_cache(maxsize=4)
def all_cells(n, cols, seed):
    """``cells`` of every element of an ``n``-vector, all five rows (row j does not depend on the row count)."""
    return cells(np.arange(n), cols, seed)


def encode(x, rows, cols, seed):
    """(S, M): the table of ``x`` and, per cell, the sum of |x_i| over its contributors (the error bounds' scale)."""
    x = np.asarray(x, np.float64)
    cell, sign = all_cells(x.size, cols, seed)
    S, M = np.zeros((rows, cols)), np.zeros((rows, cols))
    for j in range(rows):
        np.add.at(S[j], cell[:, j], sign[:, j] * x)
        np.add.at(M[j], cell[:, j], np.abs(x))
    return S, M


def fold(tables, weights):
    """(S-bar as the device rounds it: fp32(w_0 S_0), then fmaf(w_c, S_c, .), sum_c |w_c S_c|) of fp32 tables."""
    w = [np.float64(np.float32(v)) for v in weights]
    s = (w[0] * tables[0].astype(np.float64)).astype(np.float32)
    mag = np.abs(w[0] * tables[0].astype(np.float64))
    for wc, t in zip(w[1:], tables[1:]):
        s = (wc * t.astype(np.float64) + s.astype(np.float64)).astype(np.float32)  # (exact before the one rounding at
        mag += np.abs(wc * t.astype(np.float64))                                  # the tests' magnitudes)
    return s, mag


def estimate(S, n, cols, seed):
    """(median over the rows of s_j(i) S[j][cell_j(i)], those per-row values [n, rows]) for i < n."""
    rows = S.shape[0]
    cell, sign = all_cells(n, cols, seed)
    vals = sign[:, :rows] * np.asarray(S, np.float64)[np.arange(rows)[None, :], cell[:, :rows]]
    return np.median(vals, axis=1), vals


def planted(seed, n=50_000, count=8):
    """(x, the planted indices): ``count`` coordinates of +-100 among unit Gaussians."""
    g = np.random.default_rng(seed)
    x = g.standard_normal(n).astype(np.float32)
    idx = np.sort(g.choice(n, count, replace=False))
    x[idx] = 100.0 * g.choice([-1.0, 1.0], count)
    return x, idx
