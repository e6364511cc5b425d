"""The numpy model of top-k by magnitude, built from ``oracle.compressors_ref`` functions applied to ``|x|``.

Definition: for a vector ``x`` of length ``d`` and ``0 < K < d`` the kept index set is exactly the
set the signed select keeps on ``|x|`` — ``ref.topk_kept(np.abs(x), K)[0]``: a NaN of either sign is the largest
magnitude, ``-0 == +0``, ``+v`` and ``-v`` tie, and among the entries tied with the K-th largest magnitude the highest
indices are kept — and the kept values are ``x[kept]`` with their own signs.  ``K <= 0`` or ``K >= d`` copies ``x``.
The stacked pipeline's second stage (standard dithering, p = inf) is the oracle's own, run on the kept values.
"""

from __future__ import annotations

from typing import Callable, Tuple

import numpy as np

from oracle import compressors_ref as ref

F32 = np.float32


def kept(x: np.ndarray, K: int, fast: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(ascending kept indices, x[kept]); ``fast``: the O(n) select of the same set."""
    idx = (ref.topk_kept_select if fast else ref.topk_kept)(np.abs(x), K)[0]
    return idx, x[idx]


def topk(x: np.ndarray, K: int) -> np.ndarray:
    """The dense result: x on the kept set, +0 elsewhere; a copy of x for K <= 0 or K >= d."""
    if not 0 < K < len(x):
        return x.copy()
    out = np.zeros_like(x)
    idx, vals = kept(x, K, fast=len(x) > 4096 and x.dtype == np.float32)  # (the O(n) select's keys are float32)
    out[idx] = vals
    return out


def stacked(x: np.ndarray, K: int, s: int, u_of: Callable[[np.ndarray], np.ndarray], fast: bool = False):
    """Top-k by magnitude, then the oracle's standard dithering (p = inf) of the K-sparse vector: (dense out, kept
    idx, codes (sign << 7 | level), norm), as ``ref.stacked`` returns them for the signed pipeline."""
    idx, vals = kept(x, K, fast)
    y = np.zeros_like(x)
    y[idx] = vals
    pn = F32(np.max(np.abs(y))) if len(y) else F32(0)
    out, _, _, lvl_idx = ref.dither(y, ref.standard_levels(s), pn, u_of)
    codes = (lvl_idx[idx] | (np.signbit(vals).astype(np.int64) << 7)) * (vals != 0)
    return out, idx, codes.astype(np.uint8), pn


def flip_signs(x: np.ndarray, seed: int) -> np.ndarray:
    """``x`` with about half of its sign bits flipped (seeded): ``|x'|`` equals ``|x|`` bit for bit."""
    g = np.random.default_rng(seed)
    bits = np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else np.uint64).copy()
    top = bits.dtype.type(1) << bits.dtype.type(8 * bits.dtype.itemsize - 1)
    bits[g.random(len(x)) < 0.5] ^= top
    return bits.view(x.dtype)
