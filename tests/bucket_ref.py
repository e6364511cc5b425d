"""Numpy model of bucketed dithering, built only from oracle.compressors_ref: the dithering rule (``dither``) with
the level tables (``standard_levels`` / ``natural_levels``) run per slice of ``B`` consecutive elements with that
slice's norm, the uniforms from one stream (``compat_stream`` / ``python_random_stream`` in index order across the
slices, or ``philox_stream`` at the element's index in the whole message)."""

from __future__ import annotations

import math

import numpy as np

from oracle import compressors_ref as ref

STD, NATD = 0, 1


def levels_of(kind, s: int) -> np.ndarray:
    return ref.standard_levels(s) if kind in ("std", STD) else ref.natural_levels(s)


def code_bits(s: int) -> int:
    b = 1 + int(math.ceil(math.log2(s + 1)))
    return next(c for c in (2, 4, 8) if b <= c)


def slices(n: int, B: int):
    return [(lo, min(lo + B, n)) for lo in range(0, n, B)]


def bucket_compat(x: np.ndarray, kind: str, s: int, B: int, pnorms: np.ndarray, u_of=None):
    """The slice-wise compressVector with the global ``random`` stream (or ``u_of``): (out, send, nnz)."""
    u_of = u_of or ref.python_random_stream()
    lv = levels_of(kind, s)
    out = np.zeros_like(x)
    nnz = 0
    for b, (lo, hi) in enumerate(slices(len(x), B)):
        o, nz, _, _ = ref.dither(x[lo:hi], lv, np.float32(pnorms[b]), u_of)
        out[lo:hi] = o
        nnz += nz
    per = (1.0 + np.ceil(math.log2(s))) / 32.0
    send = len(pnorms) + nnz * per if kind == "std" else len(x) * per
    return out, send, nnz


def bucket_philox(x: np.ndarray, kind, s: int, B: int, pnorms: np.ndarray, seed: int, ctr: int):
    """Philox mode: (out, codes as one uint32 per element, nnz); element e of the message on uniform e."""
    n = len(x)
    lv = levels_of(kind, s)
    bits = code_bits(s)
    out = np.zeros_like(x)
    codes = np.zeros(n, dtype=np.uint32)
    u_all = ref.philox_uniforms(n, seed, ctr)
    nnz = 0
    for b, (lo, hi) in enumerate(slices(n, B)):
        xs = x[lo:hi]
        nrm = np.float32(pnorms[b])
        o, nz, ci, li = ref.dither(xs, lv, nrm, lambda idx, lo=lo: u_all[idx + lo])
        nnz += nz
        sign = np.signbit(xs).astype(np.uint32) << (bits - 1)
        if nrm > 0 and np.isfinite(nrm):
            out[lo:hi] = o
            codes[lo:hi] = np.where(xs != 0, sign | li.astype(np.uint32), 0)
        else:  # a norm of 0, +-inf or NaN: code 0 for x == 0, code 1 otherwise; decodes to +0 / NaN
            codes[lo:hi] = (xs != 0).astype(np.uint32)
            out[lo:hi] = np.where(xs != 0, np.float32(np.nan), np.float32(0))
    return out, codes, nnz


def pack(codes: np.ndarray, bits: int) -> np.ndarray:
    """Element i at bit offset i * bits, little-endian within a byte."""
    n = len(codes)
    per = 8 // bits
    padded = np.zeros(-(-n // per) * per, dtype=np.uint32)
    padded[:n] = codes
    by = np.zeros(len(padded) // per, dtype=np.uint32)
    for j in range(per):
        by |= padded[j::per] << (j * bits)
    return by.astype(np.uint8)


def unpack(by: np.ndarray, n: int, bits: int) -> np.ndarray:
    per = 8 // bits
    b = by.astype(np.uint32)
    out = np.zeros(len(b) * per, dtype=np.uint32)
    for j in range(per):
        out[j::per] = (b >> (j * bits)) & ((1 << bits) - 1)
    return out[:n]


def decode(codes: np.ndarray, kind, s: int, B: int, pnorms: np.ndarray) -> np.ndarray:
    """v = fp32(fp32(level) * sign) * norm[e // B]; under a norm that is not positive and finite: +0 / NaN."""
    bits = code_bits(s)
    lv = levels_of(kind, s).astype(np.float32)
    n = len(codes)
    nrm = np.repeat(np.asarray(pnorms, dtype=np.float32), B)[:n]
    lvl = codes & ((1 << (bits - 1)) - 1)
    neg = (codes >> (bits - 1)) & 1
    sv = np.where(neg == 1, -lv[lvl], lv[lvl]).astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (sv * nrm).astype(np.float32)
    bad = ~((nrm > 0) & np.isfinite(nrm))
    v[bad] = np.where(codes[bad] == 0, np.float32(0), np.float32(np.nan))
    return v
