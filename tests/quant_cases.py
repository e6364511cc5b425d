"""Inputs that put the elements of a dithering / natural quantizer call on the edges of its per-element decision, and
float32 numpy restatements of the two fp32 fast paths of the standard dithering.  CPU only: no torch, no device.

The decision of compressors.py:344-353 is "lower level iff u < p" with p = (lv[j+1] - y) / (lv[j+1] - lv[j]) and
y = |x| / norm.  Random inputs leave |u - p| ~ 1/3 and y ~ 1/(2s) from a level; every element here is built from its
own Philox uniform u_i so that p lands a chosen offset from u_i, or y a chosen offset from a level, the offsets being
the margins of the kernels' fast paths (1e-4, 5e-5, 3e-5), the error bound their comments claim (2.4e-5), 1e-9 and 0.
The natural compressor (pt = 2 - mantissa, exact) gets pt = u_i to the last mantissa bit and one ulp either side.

The oracle (oracle/compressors_ref.py) is the only reference of the device tests; the mirrors below exist so the CPU
test can show which path each element of the catalogue takes, and that a narrower margin would decide some wrongly."""

import functools
import math

import numpy as np

from oracle import compressors_ref as ref

F32, F64 = np.float32, np.float64

LEVELS_STD = (1, 2, 3, 7, 10, 100, 127)
LEVELS_NAT = (2, 4, 8)
# (3.7e-37 / 3.8e-37: fp32(127 / norm) overflows / does not; >= 8.6e37: fp32(1 / norm) is subnormal)
NORMS32 = tuple(F32(v) for v in (1.0, 0.75, 3.1e-3, 1.1754944e-38, 1e-38, 3e-42, 3.7e-37, 3.8e-37, 8.6e37, 1e38,
                                 3.4028235e38))
NORMS_NAT32 = tuple(F32(v) for v in (1.0, 3.1e-3, 3e-42, 1.1754944e-38, 3.4028235e38))
NORMS64 = (1.0, 0.75, 2.0**-1074, 1e-310, 2.0**-1022, 1e300, 1.7976931348623157e308)
# the kernels' margins, the error bound of quant.hip's comment, and two offsets far inside them
OFFSETS = np.array([0.0, 1e-9, -1e-9, 2.4e-5, -2.4e-5, 3e-5, -3e-5, 5e-5, -5e-5, 1e-4, -1e-4])
NEAR_POW2_EXPONENTS = tuple(sorted({sg * f for sg in (1, -1) for f in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 127,
                                                                         128, 129, 600, 1000)}
                                   | {0, -1022, 1023, -1074, -1073, -1060, -1030, -1023}))


# ------------------------------------------------------------------------------------------------- uniforms
def words_at(idx, seed, counter):
    """The uint32 Philox word of each element index (word e & 3 of counter group e >> 2): u = word * 2^-32 is
    ref.philox_uniforms_at."""
    e = np.asarray(idx, dtype=np.uint64)
    grp = e >> np.uint64(2)
    w = ref.philox4x32_10(
        (grp & np.uint64(0xFFFFFFFF)).astype(np.uint32), (grp >> np.uint64(32)).astype(np.uint32),
        np.uint32(counter & 0xFFFFFFFF), np.uint32((counter >> 32) & 0xFFFFFFFF),
        np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    return np.stack(w, axis=1)[np.arange(len(e)), (e & np.uint64(3)).astype(np.int64)].astype(np.uint32)


def words(n, seed, counter):
    return words_at(np.arange(n, dtype=np.uint64), seed, counter)


def uniforms(w):
    return w.astype(F64) * 2.0**-32


# ------------------------------------------------------------------------------------------- dithering, fp32 / fp64
def _edge_y(lv, u, g, extra_on_levels):
    """y* in [0, 1] of each element from its uniform: a third with p = u + off, a third each with y an offset (in
    bracket widths: off / s for the standard levels) from the lower / upper level of a uniformly drawn bracket;
    ``extra_on_levels``: every 16th element exactly on a nonzero level instead."""
    n, s = len(u), len(lv) - 1
    j = g.integers(0, s, n)
    off = OFFSETS[g.integers(0, len(OFFSETS), n)]
    kind = g.permutation(n) % 3
    lo, hi = lv[j], lv[j + 1]
    y = np.where(kind == 0, hi - (u + off) * (hi - lo), np.where(kind == 1, lo, hi) + off * (hi - lo))
    if extra_on_levels:
        on = np.arange(n) % 16 == 5
        y[on] = hi[on]
    else:
        on = np.zeros(n, dtype=bool)
    return np.clip(y, 0.0, 1.0), on


def _finish(y, on, norm, g, ftype, itype):
    """x = ftype(y * norm) moved by -2 .. +2 ulps (not the ``on`` elements), |x| <= norm, random signs,
    x[0] = +-norm."""
    norm = ftype(norm)
    with np.errstate(over="ignore", under="ignore"):
        mag = (y * F64(norm)).astype(ftype) if ftype is F32 else ftype(y) * norm
    mag = np.minimum(mag, norm)
    bits = mag.view(itype).astype(np.int64) + np.where(on, 0, g.integers(-2, 3, len(y)))
    bits = np.clip(bits, 0, int(np.array([norm]).view(itype)[0]))
    x = bits.astype(itype).view(ftype).copy()
    x[0] = norm
    return np.where(g.random(len(y)) < 0.5, -x, x).astype(ftype)


def std_edge_case(s, norm, n, seed, counter, g, at=None):
    """float32 vector for standard dithering with ``s`` levels and the given norm; element i is built from the
    uniform of index ``at[i]`` (default i)."""
    u = uniforms(words_at(np.arange(n) if at is None else at, seed, counter))
    y, on = _edge_y(ref.standard_levels(s), u, g, False)
    return _finish(y, on, norm, g, F32, np.uint32)


def nat_dither_edge_case(s, norm, n, seed, counter, g, at=None):
    """The same for the natural levels [0, 2^-(s-1), ..., 1/2, 1]: the brackets include [0, 2^-(s-1)] (elements below
    the lowest level), and every 16th element sits exactly on a power of two."""
    u = uniforms(words_at(np.arange(n) if at is None else at, seed, counter))
    y, on = _edge_y(ref.natural_levels(s), u, g, True)
    return _finish(y, on, norm, g, F32, np.uint32)


def std_edge_case64(s, norm, n, seed, counter, g):
    """std_edge_case in float64 (y = |x| / norm, p and the ulp moves all in fp64), for quant64_code."""
    u = uniforms(words(n, seed, counter))
    y, on = _edge_y(ref.standard_levels(s), u, g, False)
    return _finish(y, on, norm, g, F64, np.uint64)


# --------------------------------------------------------------------------------------------- natural compressor
def _natural_case(n, seed, counter, g, mant_bits, exps, specials, ftype):
    """|x| = (2 - pt) * 2^f with pt = u_i rounded to ``mant_bits`` bits, and that -1 / +1 ulp; an element whose u_i
    has no bits below 2^-mant_bits always gets pt == u_i (the strict < then takes the upper power)."""
    w = words(n, seed, counter).astype(np.uint64)
    drop = 32 - mant_bits  # bits of the word below the mantissa's last place (negative: the word is coarser)
    q = ((w + (np.uint64(1) << np.uint64(drop - 1))) >> np.uint64(drop)).astype(np.int64) if drop > 0 \
        else w.astype(np.int64) << (-drop)
    exact = (w & np.uint64((1 << max(drop, 0)) - 1)) == 0
    off = g.integers(-1, 2, n)
    if drop > 0:
        off = np.where(exact, 0, off)
    q = np.clip(q + off, 1, 1 << mant_bits)
    m = 2.0 - q.astype(F64) * 2.0**-mant_bits  # exact: a multiple of 2^-mant_bits in [1, 2)
    f = np.asarray(exps, dtype=np.int64)[g.integers(0, len(exps), n)]
    with np.errstate(under="ignore"):
        x = np.ldexp(m, f).astype(ftype)  # (a subnormal keeps the mantissa bits it has room for)
    x = np.where(g.random(n) < 0.5, -x, x).astype(ftype)
    sp = np.asarray(specials, dtype=ftype)
    sp = np.concatenate([sp, -sp])
    x[1:1 + len(sp)] = sp  # (index 0 keeps a generic element; the last, ragged group stays generic too)
    pt_eq_u = q.astype(F64) * 2.0**-mant_bits == uniforms(w.astype(np.uint32))
    pt_eq_u[1:1 + len(sp)] = False
    return x, pt_eq_u & (np.abs(x) >= np.finfo(ftype).tiny)


def natural_edge_case(n, seed, counter, g):
    """float32 vector for the natural compressor and the mask of its normal elements with pt == u exactly."""
    fmax = np.finfo(F32).max
    below = np.nextafter(fmax, F32(0), dtype=F32)
    specials = [fmax, below, np.nextafter(below, F32(0), dtype=F32), np.finfo(F32).tiny, 2.0**-149, 2.0**-148,
                3 * 2.0**-149, 2.0**-127, 1.0, 2.0**127, 2.0**-126, 0.5, 2.0, 2.0**64, 2.0**-64]
    exps = [-149, -148, -140, -130, -127, -126, -125, -1, 0, 1, 23, 24, 64, 126, 127] + list(range(-126, 128, 7))
    return _natural_case(n, seed, counter, g, 23, exps, specials, F32)


def natural_edge_case64(n, seed, counter, g):
    """The same in float64 (pt a multiple of 2^-52: every u_i is one, so a third of the elements have pt == u_i)."""
    fmax = np.finfo(F64).max
    below = np.nextafter(fmax, 0.0)
    specials = [fmax, below, np.nextafter(below, 0.0), np.finfo(F64).tiny, 2.0**-1074, 2.0**-1073, 3 * 2.0**-1074,
                2.0**-1023, 1.0, 2.0**1023, 2.0**600, 0.5, 2.0, 3.0]
    exps = [-1074, -1073, -1060, -1030, -1023, -1022, -1021, -1, 0, 1, 52, 53, 600, 1022, 1023] + \
        list(range(-1022, 1024, 61))
    return _natural_case(n, seed, counter, g, 52, exps, specials, F64)


def near_pow2_case64():
    """The doubles around every power of two 2^f of NEAR_POW2_EXPONENTS where math.log2 may round onto the integer:
    2^f (1 + j 2^-52), j = 0 .. J_f, and 2^f (1 - j 2^-53), j = 1 .. J_f, J_f = 64 (|f| + 2) — four times the width
    W = (|f| + 2) 2^-48 of natural64_code's log2 branch, so both sides of its switch are present.  Returns (x, u):
    signs alternate, and u[i] is one of 0, delta_i (|x_i| = 2^f (1 +- delta_i)) and 1 - 2^-53 — the decision depends
    on the rounding of log2 only for u < 2 delta."""
    parts = []
    for f in NEAR_POW2_EXPONENTS:
        J = 64 * (abs(f) + 2)
        j = np.arange(0, J + 1, dtype=F64)
        up = np.ldexp(1.0 + j * 2.0**-52, f)
        dn = np.ldexp(1.0 - j[1:] * 2.0**-53, f)
        v = np.concatenate([dn[::-1], up])
        parts.append(np.unique(v[v > 0]))  # (subnormals: the representable ones, once each)
    a = np.concatenate(parts)
    m, e = np.frexp(a)
    delta = np.where(m < 0.75, 2.0 * m - 1.0, 1.0 - m)  # exact
    i = np.arange(len(a))
    u = np.where(i % 3 == 0, 0.0, np.where(i % 3 == 1, delta, 1.0 - 2.0**-53))
    x = np.where(i % 2 == 0, a, -a)
    assert len(x) < 2_000_000
    return x, u


def log2_correctly_rounded(a):
    """Correctly rounded log2 of positive doubles, through ``decimal`` at 60 digits: a = 2^F (1 + d) with d exact;
    log1p(d) by its series while |d| < 1e-9 (the next term is below 1e-54), by Decimal.ln otherwise."""
    import decimal

    ctx = decimal.Context(prec=60)
    D = decimal.Decimal
    ln2 = ctx.ln(D(2))
    half, third, quarter = D(1) / D(2), ctx.divide(D(1), D(3)), D(1) / D(4)
    m, e = np.frexp(np.asarray(a, dtype=F64))
    hi = m >= 0.75
    F = np.where(hi, e, e - 1).tolist()
    d = np.where(hi, m - 1.0, 2.0 * m - 1.0).tolist()
    out = []
    for Fi, di in zip(F, d):
        dd = D(di)
        if abs(di) < 1e-9:
            l1p = ctx.multiply(dd, ctx.subtract(D(1), ctx.multiply(dd, ctx.subtract(half, ctx.multiply(
                dd, ctx.subtract(third, ctx.multiply(dd, quarter)))))))
        else:
            l1p = ctx.ln(ctx.add(D(1), dd))
        out.append(float(ctx.add(D(Fi), ctx.divide(l1p, ln2))))
    return np.array(out)


@functools.lru_cache(maxsize=None)
def host_log2_survey():
    """Host math.log2 against the correctly rounded log2 over near_pow2_case64 (read by the CPU and the device test):
    ``decides`` = floor and ceil agree on every element and the two are equal wherever either is an integer — all the
    oracle takes from math.log2; ``off`` = elements where they differ at all, ``max_ulps`` = by how much;
    ``on_integer`` = non-powers of two whose math.log2 is an integer."""
    x, _ = near_pow2_case64()
    a = np.abs(x)
    host = np.array([math.log2(v) for v in a.tolist()])
    exact = log2_correctly_rounded(a)
    integral = (host == np.rint(host)) | (exact == np.rint(exact))
    decides = bool(np.array_equal(np.floor(host), np.floor(exact)) and np.array_equal(np.ceil(host), np.ceil(exact))
                   and np.array_equal(host[integral], exact[integral]))
    off = host != exact
    ulps = np.abs(host[off] - exact[off]) / np.spacing(np.abs(exact[off]))
    m, _ = np.frexp(a)
    return {"decides": decides, "off": int(off.sum()), "max_ulps": float(ulps.max()) if off.any() else 0.0,
            "on_integer": int(((host == np.rint(host)) & (m != 0.5)).sum()), "n": int(a.size)}


# ------------------------------------------------------------------------------------------------ mirrors
def fast_std_mirror(x, norm, s, w, margins=(1e-4, 5e-5)):
    """quant.hip's 8-element group path and topk.hip's code_of, in float32: t' = |x| * fp32(s / norm), p' = ceil(t') -
    t', u' = fp32(word) * 2^-32.  Returns (level, decided): decided where t' clears ``margins[0]`` from both integers
    and |u' - p'| clears ``margins[1]`` (an overflowed s / norm decides nothing: every comparison with NaN fails)."""
    m0, m1 = F32(margins[0]), F32(margins[1])
    with np.errstate(all="ignore"):
        rs = F32(s) / F32(norm)
        t = np.abs(x.astype(F32)) * rs
        jf = np.ceil(t)
        pf = jf - t
        uf = w.astype(F32) * F32(2.0**-32)
        ok = (pf > m0) & (t - (jf - F32(1)) > m0) & (np.abs(uf - pf) > m1) & (x != 0)
        lvl = np.where(ok, jf, 0).astype(np.int64) - (ok & (uf < pf))
    return lvl, ok


def dither_level_mirror(y, s, u, margins=(1e-4, 3e-5)):
    """flc_device.hpp's dither_level<0> fast path on y = fp32(|x| / norm) and the fp64 uniform u."""
    m0, m1 = F32(margins[0]), F32(margins[1])
    with np.errstate(all="ignore"):
        t = y.astype(F32) * F32(s)
        jf = np.ceil(t)
        pf = jf - t
        uf = u.astype(F32)
        ok = (pf > m0) & (t - (jf - F32(1)) > m0) & (np.abs(uf - pf) > m1)
        lvl = np.where(ok, jf, 0).astype(np.int64) - (ok & (uf < pf))
    return lvl, ok
