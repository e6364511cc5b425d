"""Inputs and numpy models for bucketed dithering (flc_bucket_encode / _encode_round / _decode and the four
``*_bucket_*`` folds) where its kernels can go wrong.  CPU only: no torch, no device.

edge_message     one message whose buckets are the decision-edge vectors of tests/quant_cases.py (p a margin's width
                 from the element's own Philox uniform, y a margin's width from a level), bucket b under the norm
                 NORMS32[(b + rot) % len]: neighbours run from 3e-42 to FLT_MAX, x[lo] = +-norm makes that norm the
                 bucket's max |x|, the message spans three 4096-element blocks and ends in a short bucket.
l2_norm_model    the summation order include/flcodec.h promises for p = 2: a per-lane fp64 chain over 8 elements, a
                 balanced tree over min(B / 8, 64) adjacent lanes, then the bucket's waves in order.
l2_message       general buckets with a 2^+-20 spread of scales, the special buckets (a subnormal norm, an overflow to
                 inf, a norm just below FLT_MAX, NaN, inf) and, for B >= 2048, a bucket whose fp32 norm depends on the
                 wave order (tie_bucket).
handbuilt_record a record laid out as flc_bucket_wire_layout describes, every code of the format under bucket norms
                 that alternate regular and irregular values (-0, -1, -inf, ...), the padding filled with a sentinel;
                 its decode is tests/decode_cases.quant_values with each element's bucket norm.

tests/test_bucket_cases.py anchors all of this on the CPU; tests/test_gpu_bucket_edges.py holds the kernels to it."""

from __future__ import annotations

import functools

import numpy as np

from tests import bucket_ref as br
from tests import decode_cases as dc
from tests import quant_cases as qc

F32, F64 = np.float32, np.float64
STD, NAT = 0, 1
ALL_B = (64, 128, 256, 512, 1024, 2048, 4096)
TAILS = ("one", "six", "nearly")  # 1, 6 and B - 3 elements in the last bucket
BLOCK = 4096  # elements per block of bucket_encode_kernel
SEED, CTR = 0x1234_5678_9ABC, 77
FLT_MAX = np.finfo(F32).max
PAD = 0xA5  # the sentinel byte of a hand-built record's padding


def tail_len(tail: str, B: int) -> int:
    return {"one": 1, "six": 6, "nearly": B - 3}[tail]


def rotation(kind: int, B: int, i: int):
    """The (tail, rot) of level index i at this bucket size: over a kind's levels each (B, tail) pair occurs."""
    return TAILS[(ALL_B.index(B) + i) % 3], i + kind


def norms_of(kind: int):
    return qc.NORMS32 if kind == STD else qc.NORMS_NAT32


def levels_of(kind: int):
    return qc.LEVELS_STD if kind == STD else qc.LEVELS_NAT


# ------------------------------------------------------------------------------------------------ decision edges
@functools.lru_cache(maxsize=64)
def edge_message(kind: int, s: int, B: int, tail: str, rot: int, seed: int = SEED, counter: int = CTR):
    """(x, norms, codes (one per element, unpacked), decode, nnz): every norm of the kind's table on a whole bucket,
    n >= 2 * 4096 + B, then ``tail_len(tail, B)`` more elements; the expectation is ref.dither per slice under that
    slice's norm with the uniform of the element's index in the whole message (bucket_ref.bucket_philox)."""
    table = norms_of(kind)
    whole = max(len(table), -(-(2 * BLOCK + B) // B))
    n = whole * B + tail_len(tail, B)
    g = np.random.default_rng([kind, s, B, TAILS.index(tail), rot, seed & 0xFFFF, counter])
    build = qc.std_edge_case if kind == STD else qc.nat_dither_edge_case
    x = np.empty(n, dtype=F32)
    norms = np.empty(-(-n // B), dtype=F32)
    for b, (lo, hi) in enumerate(br.slices(n, B)):
        norms[b] = table[(b + rot) % len(table)]
        x[lo:hi] = build(s, norms[b], hi - lo, seed, counter, g, at=np.arange(lo, hi))
    out, codes, nnz = br.bucket_philox(x, kind, s, B, norms, seed, counter)
    for a in (x, norms, out, codes):
        a.setflags(write=False)
    return x, norms, codes, out, nnz


# ------------------------------------------------------------------------------------------------ the p = 2 norm
def bucket_sums(x: np.ndarray, B: int, reverse_waves: bool = False) -> np.ndarray:
    """The fp64 sum of squares of every bucket in the documented order (``reverse_waves``: the waves of a bucket of
    B >= 1024 taken last to first — not the documented order; the CPU test uses it to show that tie_bucket tells the
    two apart)."""
    n = len(x)
    nb = -(-n // B)
    v = np.zeros(nb * B, dtype=F64)  # (elements past n count as +0)
    v[:n] = x.astype(F64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = (v * v).reshape(nb, B // 8, 8)  # (exact: 48 significant bits)
        ss = np.zeros((nb, B // 8), dtype=F64)
        for j in range(8):  # the lane's chain over its 8 elements, in index order from 0.0
            ss = ss + sq[:, :, j]
        width = min(B // 8, 64)
        t = ss.reshape(nb, -1, width)  # [bucket, wave of the bucket, lane]
        while t.shape[2] > 1:  # xor 1, 2, 4, ...: a + b on both partners
            t = t[:, :, 0::2] + t[:, :, 1::2]
        t = t[:, :, 0]
        if B < 1024:
            return t[:, 0]
        if reverse_waves:
            t = t[:, ::-1]
        r = np.zeros(nb, dtype=F64)
        for w in range(t.shape[1]):
            r = r + t[:, w]
        return r


def l2_norm_model(x: np.ndarray, B: int, reverse_waves: bool = False) -> np.ndarray:
    """float32(sqrt(S)) per bucket, S by bucket_sums."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(bucket_sums(x, B, reverse_waves)).astype(F32)


def tie_bucket(B: int) -> np.ndarray:
    """A bucket of B >= 2048 elements whose fp32 norm depends on the wave order.  With T = 1 + 2^-24, the midpoint of
    the floats 1 and 1 + 2^-23, wave 0 sums to T^2 = 1 + 2^-23 + 2^-48 exactly in any order (1, two 2^-12 and sixteen
    2^-26, each in a lane of its own) and every later wave to 2^-53, half an fp64 ulp of T^2 (two 2^-27).  In wave
    order each half ulp is a tie that rounds to the even T^2: S = T^2, sqrt = T, and fp32(T) is a tie that rounds to
    the even 1.0.  Last to first the later waves add up first (1.5 or 3.5 ulps): S = T^2 + 2 or 4 ulps, sqrt > T, and
    the norm is 1 + 2^-23.  (For B = 1024 there are two waves, and a + b = b + a.)"""
    assert B >= 2048
    x = np.zeros(B, dtype=F32)
    x[0] = 1.0
    x[8], x[16] = 2.0**-12, -(2.0**-12)
    x[24:24 + 16 * 8:8] = 2.0**-26
    for w in range(1, B // 512):
        x[w * 512 + 40] = 2.0**-27
        x[w * 512 + 333] = -(2.0**-27)
    return x


def general_buckets(B: int, count: int, seed: int) -> np.ndarray:
    """Normal data times 2^k, k uniform in [-20, 20]: squares 2^80 apart inside one bucket, zeros and -0 among them."""
    g = np.random.default_rng([B, count, seed])
    n = B * count
    x = (g.standard_normal(n) * np.ldexp(1.0, g.integers(-20, 21, n))).astype(F32)
    x[g.random(n) < 0.03] = 0.0
    x[5::97] = -0.0
    return x


SPECIAL = ("subnormal", "overflow", "below_max", "nan", "inf")


@functools.lru_cache(maxsize=None)
def l2_message(B: int):
    """(x, {name: bucket index}): general buckets over three blocks, the special buckets each between two general ones
    for B < 4096 (so that bucket isolation is part of the comparison), the tie bucket for B >= 2048, and a tail of
    B - 3."""
    lead = -(-(2 * BLOCK + B) // B)
    parts, where = [general_buckets(B, lead, 1)], {}

    def add(name, bucket):
        where[name] = sum(len(p) for p in parts) // B
        parts.append(bucket.astype(F32))
        if B < BLOCK:  # (B = 4096 keeps the message under 50 k elements: its special buckets are neighbours)
            parts.append(general_buckets(B, 1, 10 + len(where)))

    add("subnormal", np.full(B, 2.0**-149))
    add("overflow", np.where(np.arange(B) % 2 == 0, FLT_MAX, -FLT_MAX))
    # sqrt(B) v just below FLT_MAX (every element v: S = B v^2 is exact up to the fp64 roundings of the order)
    v = F32(float(FLT_MAX) / np.sqrt(B) * (1.0 - 2.0**-20))
    add("below_max", np.where(np.arange(B) % 3, v, -v))
    nanb = general_buckets(B, 1, 3).copy()
    nanb[B // 2 + 1] = np.nan
    add("nan", nanb)
    infb = general_buckets(B, 1, 4).copy()
    infb[B - 1] = -np.inf
    add("inf", infb)
    if B >= 2048:
        add("tie", tie_bucket(B))
    parts.append(general_buckets(B, 1, 5)[:B - 3])
    x = np.concatenate(parts).astype(F32)
    x.setflags(write=False)
    return x, where


# ------------------------------------------------------------------------------------------------ hand-built records
# regular and irregular norms in turn: every irregular one has a regular neighbour (decode_cases.NORMS and -0, -inf,
# 2^-149)
RECORD_NORMS = tuple(F32(v) for v in (0.0, 1.0, -1.0, 3e-39, float("inf"), FLT_MAX, float("nan"), 2.3e-3, -0.0,
                                      2.0**-149, float("-inf")))
assert {repr(float(F32(v))) for v in dc.NORMS} <= {repr(float(v)) for v in RECORD_NORMS}
RECORD_SIZES = ("1", "6", "B-1", "B", "B+6", "1026", "4096+B+2", "3*4096+5")


def record_size(name: str, B: int) -> int:
    return {"1": 1, "6": 6, "B-1": B - 1, "B": B, "B+6": B + 6, "1026": 1026, "4096+B+2": BLOCK + B + 2,
            "3*4096+5": 3 * BLOCK + 5}[name]


def wire_layout(n: int, bits: int, B: int):
    """(record bytes, byte offset of the codes): include/flcodec.h's flc_bucket_wire_layout — nb fp32 norms, the codes
    from the next 16-B boundary, the record a multiple of 256 B."""
    nb = -(-n // B)
    codes = -(-4 * nb // 16) * 16
    return -(-(codes + (n * bits + 7) // 8) // 256) * 256, codes


def handbuilt_record(kind: int, s: int, bits: int, B: int, n: int, start: int):
    """(record bytes, norms, codes (one per element), decoded values).  Element e has code
    quant_codes(s, bits)[(e + start) % ...]: both signs of every level 0..s; bucket b has norm
    RECORD_NORMS[(b + start) % 11].  Every byte outside the two fields is PAD, and so are the unused high bits of a
    partly used last code byte.  The values are quant_values under each element's bucket norm: nrm > 0 && nrm <=
    FLT_MAX, else +0 for code 0 and NaN for every other code."""
    nb = -(-n // B)
    codes = dc.cycled(dc.quant_codes(s, bits), n, start)
    norms = np.array([RECORD_NORMS[(b + start) % len(RECORD_NORMS)] for b in range(nb)], dtype=F32)
    stride, off = wire_layout(n, bits, B)
    rec = np.full(stride, PAD, dtype=np.uint8)
    rec[:4 * nb] = norms.view(np.uint8)
    packed = dc.pack(codes, bits)
    used = (n * bits) % 8
    if used:
        packed[-1] |= np.uint8((PAD >> used) << used)
    rec[off:off + len(packed)] = packed
    values = dc.quant_values(codes, kind, s, bits, np.repeat(norms, B)[:n])
    return rec, norms, codes, values


def fold_chain(values, weights, start: np.ndarray) -> np.ndarray:
    """The ordered chain of the record folds: acc = fmaf(w_c, v_c, acc) over the records in order."""
    acc = np.array(start, dtype=F32)
    for v, w in zip(values, weights):
        acc = dc.fma_exact(F32(w), v, acc, F32)
    return acc
