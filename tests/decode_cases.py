"""A numpy model of the dense decoders and the hand-built wire streams they are pinned on.

The model restates the wire descriptions of include/flcodec.h — flc_sparse_decode[_tiled], flc_stacked_decode[_tiled],
flc_quant_decode, flc_natural_decode and the float64 forms flc_quant_decode_f64 / flc_natural_decode_f64 — with the
oracle's own level tables (oracle.compressors_ref.standard_levels / natural_levels) and the exact fused multiply-add of
oracle.server_steps_exact (proved against rational arithmetic in tests/test_step_cases.py).  tests/test_decode_cases.py
anchors it to the reference's arithmetic (ref.dither, ref.natural, ref.stacked, ref.topk and their float64 forms);
tests/test_gpu_decode_edges.py holds the kernels to it bit for bit.

Every stream built here is well formed: ascending unique indices below n, codes whose level is at most s, natural
fields 1..277 (float64: 1..2098) or the two special codes.  Nothing here needs a GPU.
"""

from __future__ import annotations

from typing import Iterator, List, Optional, Tuple

import numpy as np

from oracle import compressors_ref as ref
from oracle.server_steps_exact import fma_exact

F32, F64 = np.float32, np.float64
TILE = 1024  # FLC_TILE
FLT_MAX = float(np.finfo(F32).max)
DBL_MAX = float(np.finfo(F64).max)
STD, NAT = 0, 1  # FLC_Q_STANDARD_DITHER, FLC_Q_NATURAL_DITHER

# every n % 4 (6 and 1026 are the sizes with n % 4 == 2), one tile, two tiles, odd and even tile counts
SIZES = [1, 3, 4, 5, 6, 1023, 1024, 1025, 1026, 2047, 2048, 2049, 3073, 4097, 5 * 1024 + 3, 70_001]
LARGE_N = 2**20 + 5  # k = n: flc_tile_index takes its grid-stride path (k + 1 > 2048 x 256), every tile is full
TILE_COUNTS = [63, 64, 65, 128, 129, 1024]
LEVELS = [1, 2, 7, 49, 98, 103, 107, 127]
NORMS = [1.0, 3e-39, FLT_MAX, 2.3e-3, 0.0, -1.0, float("inf"), float("nan")]
NORMS64 = [1.0, 5e-324, DBL_MAX, 2.3e-3, 0.0, -1.0, float("inf"), float("nan")]
WEIGHTS = [1.0, 0.37, -1.5, 3e-39, 0.0, -0.0, float("inf"), float("nan")]
NAT_FIELDS = (1, 277)     # 2^(field - 150): 2^-149 .. 2^127
NAT_FIELDS64 = (1, 2098)  # 2^(field - 1075): 2^-1074 .. 2^1023
VALUE_EDGES = [0.0, -0.0, 1e-40, -3e-41, float("inf"), float("-inf"), float("nan"), FLT_MAX, -FLT_MAX, 2.0**-149,
               -(2.0**-126)]


def scale_dk(d: int, k: int) -> float:
    """fp32(D / K), rand-k's scale (compressors.py:289-291)."""
    return float(F32(d / k))


SCALES = [1.0, scale_dk(70_001, 700)]  # (100.00142...: not a power of two)


# ------------------------------------------------------------------------------------------------ value functions
def level_table(kind: int, s: int) -> np.ndarray:
    return ref.standard_levels(s) if kind == STD else ref.natural_levels(s)


def norm_regular(norm, fmax: float = FLT_MAX) -> np.ndarray:
    """0 < norm <= the format's largest finite number (NaN compares false)."""
    norm = np.asarray(norm)
    with np.errstate(invalid="ignore"):
        return (norm > 0) & (norm <= fmax)


def quant_values(codes, kind: int, s: int, bits: int, norm) -> np.ndarray:
    """fp32(fp32(lv[level]) * sign) * norm for code = sign << (bits - 1) | level; under a norm that is not regular code
    0 gives +0 and every other code NaN.  ``norm`` is a scalar or an array of ``codes``' shape (fp32)."""
    codes = np.asarray(codes).astype(np.int64)
    level, sign = codes & ((1 << (bits - 1)) - 1), codes >> (bits - 1)
    assert level.max(initial=0) <= s and sign.max(initial=0) <= 1, "not wire: a level above s"
    lv32 = level_table(kind, s).astype(F32)
    norm = np.broadcast_to(np.asarray(norm, dtype=F32), codes.shape)
    with np.errstate(all="ignore"):
        sv = lv32[level] * np.where(sign == 1, F32(-1), F32(1))
        v = sv * norm
    irregular = np.where(codes == 0, F32(0), F32(np.nan))
    return np.where(norm_regular(norm), v, irregular).astype(F32)


def quant_values64(codes, kind: int, s: int, norm, bits: int = 8) -> np.ndarray:
    """The float64 form (flc_quant_decode_f64): (lv[level] * sign) * norm in fp64, the same rule for a norm that is
    not a positive finite double."""
    codes = np.asarray(codes).astype(np.int64)
    level, sign = codes & ((1 << (bits - 1)) - 1), codes >> (bits - 1)
    assert level.max(initial=0) <= s and sign.max(initial=0) <= 1, "not wire: a level above s"
    norm = np.broadcast_to(np.asarray(norm, dtype=F64), codes.shape)
    with np.errstate(all="ignore"):
        v = (level_table(kind, s)[level] * np.where(sign == 1, -1.0, 1.0)) * norm
    irregular = np.where(codes == 0, 0.0, np.nan)
    return np.where(norm_regular(norm, DBL_MAX), v, irregular).astype(F64)


def _natural(codes, bias: int, fields: Tuple[int, int], dtype) -> np.ndarray:
    codes = np.asarray(codes).astype(np.int64)
    field, sign = codes & 0x7FFF, codes >> 15
    special = (codes == 0) | (codes == 0x7FFF)
    assert np.all(special | ((field >= fields[0]) & (field <= fields[1]))), "not wire: a field out of range"
    with np.errstate(all="ignore"):
        v = np.ldexp(1.0, np.where(special, bias, field) - bias) * np.where(sign == 1, -1.0, 1.0)
    v = np.where(codes == 0, 0.0, np.where(codes == 0x7FFF, np.nan, v))
    return v.astype(dtype)  # (a power of two inside the format's range: the cast is exact)


def natural_values(codes) -> np.ndarray:
    """0 -> +0, 0x7fff -> NaN, else +-2^(field - 150), field 1..277 (flc_natural_decode)."""
    return _natural(codes, 150, NAT_FIELDS, F32)


def natural_values64(codes) -> np.ndarray:
    """0 -> +0, 0x7fff -> NaN, else +-2^(field - 1075) (flc_natural_decode_f64)."""
    return _natural(codes, 1075, NAT_FIELDS64, F64)


# ------------------------------------------------------------------------------------------------------ code tables
def quant_codes(s: int, bits: int) -> np.ndarray:
    """Every valid code of a packet with ``s`` levels: both signs of every level 0..s, sign with level 0 included."""
    assert 1 <= s <= (1 << (bits - 1)) - 1
    lv = np.arange(s + 1, dtype=np.int64)
    return np.concatenate([lv, lv | (1 << (bits - 1))]).astype(np.uint8)


def natural_codes(fields: Tuple[int, int] = NAT_FIELDS) -> np.ndarray:
    f = np.arange(fields[0], fields[1] + 1, dtype=np.int64)
    return np.concatenate([[0, 0x7FFF], f, f | 0x8000]).astype(np.uint16)


def cycled(table: np.ndarray, count: int, start: int = 0) -> np.ndarray:
    """``count`` entries of ``table`` in turn, from position ``start``."""
    return table[(np.arange(count, dtype=np.int64) + start) % len(table)]


# -------------------------------------------------------------------------------------------------------- packing
def pack(codes, bits: int) -> np.ndarray:
    """Element i of the flat batch at bit offset i * bits, little-endian within a byte: ceil(n * bits / 8) bytes."""
    flat = np.asarray(codes).astype(np.uint8).reshape(-1)
    assert bits in (2, 4, 8) and flat.max(initial=0) < (1 << bits)
    per = 8 // bits
    padded = np.zeros(-(-len(flat) // per) * per, dtype=np.uint8)
    padded[:len(flat)] = flat
    out = np.zeros(len(padded) // per, dtype=np.uint8)
    for j in range(per):
        out |= padded[j::per] << np.uint8(j * bits)
    return out


def unpack(buf, n: int, bits: int) -> np.ndarray:
    buf = np.asarray(buf, dtype=np.uint8)
    bit = np.arange(n, dtype=np.int64) * bits
    return ((buf[bit >> 3] >> (bit & 7).astype(np.uint8)) & np.uint8((1 << bits) - 1)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- dense assembly
def sparse_dense(n: int, idx, val, scale: float = 1.0) -> np.ndarray:
    """dense[idx[j]] = fl(scale * val[j]), +0 elsewhere."""
    dense = np.zeros(n, dtype=F32)
    with np.errstate(all="ignore"):
        dense[np.asarray(idx, dtype=np.int64)] = F32(scale) * np.asarray(val, dtype=F32)
    return dense


def stacked_dense(n: int, idx, codes, s: int, norm) -> np.ndarray:
    """The code value (standard dithering, 8-bit codes, the packet's one norm) at idx[j], +0 elsewhere."""
    dense = np.zeros(n, dtype=F32)
    dense[np.asarray(idx, dtype=np.int64)] = quant_values(codes, STD, s, 8, F32(norm))
    return dense


def weighted(dense: np.ndarray, weight: float, accumulate: bool, out0: Optional[np.ndarray] = None) -> np.ndarray:
    """The output rule of the sparse, stacked and natural decodes over the whole vector:
    accumulate ? fma(weight, dense, out) : (weight != 1 ? fl(weight * dense) : dense)."""
    w = F32(weight)
    if accumulate:
        return fma_exact(w, dense, out0, F32)
    if w != F32(1):  # (NaN != 1)
        with np.errstate(all="ignore"):
            return (w * dense).astype(F32)
    return dense.copy()


def row_weighted(v: np.ndarray, row_w: Optional[np.ndarray], accumulate: bool,
                 out0: Optional[np.ndarray] = None) -> np.ndarray:
    """flc_quant_decode's rule on a [rows, d] batch:
    accumulate ? fma(row_w ? row_w[r] : 1, v, out) : (row_w ? fl(row_w[r] * v) : v)."""
    w = None if row_w is None else np.asarray(row_w, dtype=F32).reshape(-1, 1)
    if accumulate:
        return fma_exact(F32(1) if w is None else np.broadcast_to(w, v.shape), v, out0, F32)
    if w is None:
        return v.copy()
    with np.errstate(all="ignore"):
        return (w * v).astype(F32)


def tile_pointers(idx, n: int) -> np.ndarray:
    """tiles[t] = first j with idx[j] >= t * TILE, t = 0 .. ceil(n / TILE)."""
    ntiles = -(-n // TILE)
    return np.searchsorted(np.asarray(idx, dtype=np.int64), np.arange(ntiles + 1, dtype=np.int64) * TILE,
                           side="left").astype(np.uint32)


# ---------------------------------------------------------------------------------------------------- the streams
def _tile_span(n: int, t: int) -> Tuple[int, int]:
    return t * TILE, min((t + 1) * TILE, n)


def _in_tile(n: int, t: int, count: int, g: np.random.Generator) -> np.ndarray:
    """``count`` ascending indices of tile t, its first and last element among them when count >= 2."""
    lo, hi = _tile_span(n, t)
    assert 1 <= count <= hi - lo
    if count == 1:
        return np.array([lo], dtype=np.int64)
    inner = lo + 1 + np.sort(g.choice(hi - lo - 2, size=count - 2, replace=False)) if count > 2 else []
    return np.concatenate([[lo], inner, [hi - 1]]).astype(np.int64)


def streams(n: int) -> Iterator[Tuple[int, np.ndarray, str]]:
    """Every occupancy that fits n, as (n, ascending unique int64 indices, label).  The labels:
    k0, first, last, edges, tile<c> (one tile with exactly c entries, its neighbours empty), pair (two adjacent full
    tiles of one wave's pair), lasttile (every element of the last tile and nothing else), full (k = n), p1, p33."""
    g = np.random.default_rng(1_000_003 * n + 17)
    ntiles = -(-n // TILE)
    yield n, np.zeros(0, dtype=np.int64), "k0"
    yield n, np.array([0], dtype=np.int64), "first"
    yield n, np.array([n - 1], dtype=np.int64), "last"
    if n >= TILE + 1:
        e = np.arange(TILE, n, TILE, dtype=np.int64)
        yield n, np.sort(np.concatenate([e - 1, e])), "edges"
    for c in TILE_COUNTS:
        for t in (1, 0):  # (tile 1 has a neighbour on both sides when there are three tiles)
            lo, hi = _tile_span(n, t)
            if t < ntiles and hi - lo >= c:
                yield n, _in_tile(n, t, c, g), f"tile{c}"
                break
    if n >= 2 * TILE:
        t = 2 if n >= 4 * TILE else 0  # (tiles 2t and 2t + 1 share a wave)
        yield n, np.arange(t * TILE, (t + 2) * TILE, dtype=np.int64), "pair"
    if ntiles >= 2:
        yield n, np.arange((ntiles - 1) * TILE, n, dtype=np.int64), "lasttile"
    yield n, np.arange(n, dtype=np.int64), "full"
    if n >= 100:
        yield n, np.sort(g.choice(n, size=n // 100, replace=False)).astype(np.int64), "p1"
    if n >= 3:
        yield n, np.sort(g.choice(n, size=n // 3, replace=False)).astype(np.int64), "p33"


def large_stream() -> Tuple[int, np.ndarray, str]:
    return LARGE_N, np.arange(LARGE_N, dtype=np.int64), "full"


def all_streams() -> List[Tuple[int, np.ndarray, str]]:
    return [st for n in SIZES for st in streams(n)]


def sparse_values(k: int, seed: int) -> np.ndarray:
    """k kept values: ordinary ones mixed with +-0, +-denormals, +-inf, NaN and +-FLT_MAX (every 13th entry takes one
    edge value; ``seed`` moves the pattern, so a k = 1 stream meets them in turn)."""
    v = (np.random.default_rng(seed).standard_normal(k) * 1e-2).astype(F32)
    for i, e in enumerate(VALUE_EDGES):
        v[(i + seed) % 13::13] = F32(e)
    return v


def stacked_codes(k: int, s: int, start: int = 0) -> np.ndarray:
    """k code bytes cycling over every valid byte of a packet with ``s`` levels."""
    return cycled(quant_codes(s, 8), k, start)


def seed_acc(n: int, seed: int) -> np.ndarray:
    """An accumulator with -0, +-inf, NaN and denormal lanes among ordinary values (as _seed_acc of
    tests/test_gpu_sparse_wire.py lays them out)."""
    a = (np.random.default_rng(seed).standard_normal(n) * 1e-2).astype(F32)
    for i, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"), 0.0, 1e-40, -2e-42)):
        a[i::11][: max(1, n // 50)] = F32(v)
    return a
