"""Inputs that put the server optimiser steps (FedOpt's adaptive tail, FedDR's combine, FedDyn's and pFedMe's folds) on
the edges of their arithmetic, and the mutants those inputs must tell from the stepwise reference
(oracle/server_steps_exact.py).  CPU only: numpy, no torch, no device.

Every vector has N = 4,133 elements: one full 4,096-element model_fold chunk plus a 37-element remainder, N % 4 = 1.
The blocks of ``fedopt_case`` (in order; ``BLOCKS[dtype]`` maps their names to slices):

    cross     16 x 16 special values of delta and |v|: +-0, +-inf, NaN, the smallest subnormal, the smallest normal, a
              value whose square overflows, 1e+-20, +-1, and deltas whose squares are subnormal or underflow to zero
    negv      v = -0 and v < 0
    ties      yogi: v == fl(delta^2) exactly, both nextafter neighbours, and delta = v = 0
    near      v within a factor 16 of delta^2
    nearomb   v within a factor 16 of (1 - beta2) * delta^2 (a fused and an unfused adam update differ)
    vzero     v = 0 with delta = 0, delta != 0, and delta != 0 with delta^2 = 0 (tau = 0: 0/0 and x/0)
    bigtheta  theta so large that the update is under half an ulp
    cancel    theta = -update (of one optimiser each)
    lrunder   lr * delta underflows to a subnormal or to zero
    subn      delta^2 and v subnormal
    gauss     the distribution of the other tests: delta ~ N(0, 1e-3), v in [1e-6, 1e-4]

A mutant is the stepwise reference with one deliberate departure; ``differing`` counts the lanes that tell them apart.
"""

import functools

import numpy as np

from oracle import server_steps_exact as sx

F32, F64 = np.float32, np.float64
N = 4133
SPLIT = (4133 - 1030 - 7, 1030, 7)  # the three-tensor cut of the flat vectors for the folds that take a model
SIZES3 = (4133, 1030, 7)  # three tensors of a model_fold call
LR, BETA2, TAUS = 0.01, 0.99, (1e-3, 0.0)
OPTS = sx.OPTS
TEETH = 32

_TINY = {F32: 2.0**-149, F64: 2.0**-1074}
_MIN = {F32: 2.0**-126, F64: 2.0**-1022}
_HUGE = {F32: 3e38, F64: 1.5e308}
# delta whose square is subnormal / underflows to zero
_SQ_SUB = {F32: 2.0**-63, F64: 2.0**-520}
_SQ_ZERO = {F32: 2.0**-75, F64: 2.0**-540}


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == F32 else np.uint64)


def differing(a, b):
    """Lanes that differ: one side NaN and the other not, or two non-NaN values of different bit patterns (a NaN's
    payload and sign are not pinned; +-0 and +-inf are)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    an, bn = np.isnan(a), np.isnan(b)
    return (an != bn) | (~an & ~bn & (bits_of(a) != bits_of(b)))


def same(a, b) -> bool:
    return not bool(differing(a, b).any())


def lane_class(a):
    """0 finite nonzero, 1 +0, 2 -0, 3 +inf, 4 -inf, 5 NaN."""
    a = np.asarray(a)
    c = np.zeros(a.shape, dtype=np.int8)
    c[(a == 0) & ~np.signbit(a)] = 1
    c[(a == 0) & np.signbit(a)] = 2
    c[np.isposinf(a)] = 3
    c[np.isneginf(a)] = 4
    c[np.isnan(a)] = 5
    return c


def _specials(dt):
    t, m, h = _TINY[dt], _MIN[dt], _HUGE[dt]
    d = [0.0, -0.0, np.inf, -np.inf, np.nan, t, m, h, 1e20, 1e-20, 1.0, -1.0, _SQ_SUB[dt], _SQ_ZERO[dt], -_SQ_ZERO[dt],
         -3 * t]
    v = [0.0, np.inf, np.nan, t, m, h, 1e20, 1e-20, 1.0, _SQ_SUB[dt] ** 2, 5 * t, 4.0, 0.25, m * 0.5, 1e-6, 3.0]
    assert len(d) == 16 and len(v) == 16
    return np.array(d, dtype=dt), np.array(v, dtype=dt)


@functools.lru_cache(maxsize=None)
def _fedopt_case(dtype_name: str):
    dt = np.dtype(dtype_name).type
    rng = np.random.RandomState(20240 + (dt is F64))
    th_parts, d_parts, v_parts, names = [], [], [], []

    def add(name, d, v, th=None):
        d, v = np.asarray(d, dtype=dt), np.asarray(v, dtype=dt)
        assert d.shape == v.shape and d.ndim == 1
        if th is None:
            th = (rng.randn(d.size) * 1e-2).astype(dt)
        th_parts.append(np.asarray(th, dtype=dt))
        d_parts.append(d)
        v_parts.append(v)
        names.append((name, d.size))

    with np.errstate(all="ignore"):
        sd, sv = _specials(dt)
        add("cross", np.repeat(sd, 16), np.tile(sv, 16))
        add("negv", [0.0, 1e-3, -0.0, 1e-3, 0.0, 1e-3, 0.0, -1e-3],
            [-0.0, -0.0, -0.0, -1.0, -1e-30, -1e-30, -np.inf, -_TINY[dt]])
        # yogi ties: v == fl(d^2), its neighbours, and both zero
        d = (rng.randn(48) * 1e-3).astype(dt)
        d[:4] = np.array([1.0, -3.0, 2.0**-10, 1e-3], dtype=dt)
        sq = d * d
        add("ties", np.concatenate([d, d, d, np.array([0.0, -0.0, 0.0, -0.0], dtype=dt)]),
            np.concatenate([sq, np.nextafter(sq, dt(np.inf)), np.nextafter(sq, dt(0)),
                            np.array([0.0, 0.0, -0.0, -0.0], dtype=dt)]))
        d = (rng.randn(256) * 1e-3).astype(dt)
        add("near", d, (d * d) * (2.0 ** rng.uniform(-4, 4, 256)).astype(dt))
        # (with beta2 = 0.99 the two terms of adam's update are of one size where v is near delta^2 / 100: there the
        # rounding of fl((1 - beta2) * delta^2), which the fma does not make, reaches v's last bit)
        d = (rng.randn(256) * 1e-3).astype(dt)
        add("nearomb", d, (d * d) * dt(1.0 - BETA2) * (2.0 ** rng.uniform(-4, 4, 256)).astype(dt))
        z = _SQ_ZERO[dt]  # (delta != 0 whose square is zero: v stays 0, and tau = 0 divides lr * delta by zero)
        d = [0.0, -0.0] * 4 + list(rng.randn(8) * 1e-3) + [z, -z, z / 2, -z / 2, z / 8, -z / 8, z / 64, -z / 64]
        add("vzero", np.array(d, dtype=dt), np.zeros(24, dtype=dt))
        d = (rng.randn(32) * 1e-3).astype(dt)
        big = [1e6, -1e6, 3e7, 1e12] if dt is F32 else [1e15, -1e15, 3e16, 1e22]
        add("bigtheta", d, rng.uniform(1e-6, 1e-4, 32).astype(dt), th=np.array(big * 8, dtype=dt))
        # theta = -update: 16 lanes for each adaptive optimiser (tau = 1e-3)
        d = (rng.randn(48) * 1e-3).astype(dt)
        v = rng.uniform(1e-6, 1e-4, 48).astype(dt)
        th = np.zeros(48, dtype=dt)
        for i, opt in enumerate(("adagrad", "yogi", "adam")):
            sl = slice(16 * i, 16 * i + 16)
            th[sl] = -sx.fedopt_step(opt, th[sl], d[sl], v[sl], LR, BETA2, TAUS[0], dt)[0]
        add("cancel", d, v, th=th)
        lo = 2.0 ** rng.uniform(-8, 12, 64) * _TINY[dt]
        add("lrunder", (lo * rng.choice([-1.0, 1.0], 64)).astype(dt), rng.uniform(1e-12, 1e-10, 64).astype(dt),
            th=(rng.randn(64) * 1e-2 * (rng.rand(64) < 0.5)).astype(dt))  # (half the lanes theta = 0: the bits survive)
        d = (_SQ_SUB[dt] * 2.0 ** rng.uniform(-8, -0.5, 96) * rng.choice([-1.0, 1.0], 96)).astype(dt)
        v = (_TINY[dt] * 2.0 ** rng.uniform(0, 20, 96)).astype(dt)
        v[::5] = 0
        add("subn", d, v)
        rest = N - sum(k for _, k in names)
        add("gauss", rng.randn(rest) * 1e-3, rng.uniform(1e-6, 1e-4, rest))
    blocks, off = {}, 0
    for name, k in names:
        blocks[name] = slice(off, off + k)
        off += k
    assert off == N
    out = tuple(np.concatenate(p) for p in (th_parts, d_parts, v_parts))
    for a in out:
        a.setflags(write=False)
    return out + (blocks,)


def fedopt_case(dtype=F32):
    """(theta, delta, v) of N elements, read-only."""
    return _fedopt_case(np.dtype(dtype).name)[:3]


def blocks(dtype=F32):
    return _fedopt_case(np.dtype(dtype).name)[3]


# --------------------------------------------------------------------------------------------------------- FedDR
# (num_clients 3, eta 0.01: cx = 3/4 and cy = 1/4 are exact, so |t| == pc can be placed exactly; num_clients 10 rounds
# both products)
FEDDR_PARAMS = ({"alpha": 0.3, "cx": 0.75, "cy": 0.25, "pc": 0.0075}, {"alpha": 1.9, "cx": 10 / 11, "cy": 1 / 11,
                                                                       "pc": 0.1 * 10 / 11})
PROXES = (sx.PROX_NONE, sx.PROX_L1, sx.PROX_SCALE)


@functools.lru_cache(maxsize=None)
def _feddr_case(dtype_name: str):
    """(theta, y, x_til): N lanes.  With FEDDR_PARAMS[0]: 64 lanes of |t| == pc and its neighbours, 64 of t = -0 and
    64 of t = +0, 96 NaN lanes (a NaN operand, inf - inf, 0 * inf); specials crossed; gaussians around the threshold."""
    dt = np.dtype(dtype_name).type
    rng = np.random.RandomState(77 + (dt is F64))
    p = FEDDR_PARAMS[0]
    pc = dt(p["pc"])
    tiny = _TINY[dt]
    th, y, x = [], [], []

    def add(t_, y_, x_):
        th.append(np.asarray(t_, dtype=dt))
        y.append(np.asarray(y_, dtype=dt))
        x.append(np.asarray(x_, dtype=dt))

    with np.errstate(all="ignore"):
        # theta == y keeps y; x = 0: t = fl(y / 4) = +-pc exactly, and one ulp either side
        edge = np.array([pc, -pc, np.nextafter(pc, dt(1)), np.nextafter(pc, dt(0)), -np.nextafter(pc, dt(1)),
                         -np.nextafter(pc, dt(0)), 2 * pc, -2 * pc] * 8, dtype=dt) * dt(4)
        add(edge, edge, np.zeros(64))
        # t = -0 needs both products -0 (x = -0; cy * y' underflowing from below): y = -0 with theta one subnormal
        # step below it (alpha * (theta - y) rounds to -0), or theta == y one or two steps below zero (y' = y, and
        # y' / 4 rounds to -0: under half a step, and the tie to even)
        kind = np.arange(64) % 3
        add(np.where(kind == 0, -tiny, np.where(kind == 1, -tiny, -2 * tiny)),
            np.where(kind == 0, -0.0, np.where(kind == 1, -tiny, -2 * tiny)), np.full(64, -0.0))
        add(np.zeros(64), np.zeros(64), np.where(rng.rand(64) < 0.5, 0.0, -0.0))  # t = +0
        nan = np.full(32, np.nan)
        g = rng.randn(32) * 1e-2
        add(np.concatenate([nan, g, g]), np.concatenate([g, nan, g]), np.concatenate([g, g, nan]))
        add(np.full(16, np.inf), np.full(16, np.inf), g[:16])  # theta - y = inf - inf
        add(g[:16], np.full(16, np.inf), np.full(16, -np.inf))  # cx * x + cy * y = -inf + inf
        sd, _ = _specials(dt)
        add(np.repeat(sd, 16), np.tile(sd, 16), np.tile(np.roll(sd, 5), 16))
        rest = N - sum(a.size for a in th)
        add(rng.randn(rest) * 2e-2, rng.randn(rest) * 2e-2, rng.randn(rest) * 1e-2)
    out = tuple(np.concatenate(a) for a in (th, y, x))
    assert all(a.size == N for a in out)
    for a in out:
        a.setflags(write=False)
    return out


def feddr_case(dtype=F32):
    return _feddr_case(np.dtype(dtype).name)


# ------------------------------------------------------------------------------------------------ message vectors
@functools.lru_cache(maxsize=None)
def messages(count: int, n: int = N, seed: int = 0):
    """``count`` fp32 message vectors of n elements with edge lanes among gaussians (+-0, +-inf, NaN, subnormals,
    values whose weighted sum cancels), read-only."""
    rng = np.random.RandomState(1000 + 31 * count + seed)
    out = []
    edges = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0**-149, -(2.0**-140), 3e38, -3e38, 1e-30, 1.0], dtype=F32)
    for m in range(count):
        x = (rng.randn(n) * 1e-3).astype(F32)
        pos = rng.permutation(n)[: max(1, n // 12)]
        x[pos] = edges[rng.randint(0, len(edges), pos.size)]
        if m and n > 40:
            x[7:40:3] = -out[0][7:40:3]  # cancels the first message's value under equal weights
        x.setflags(write=False)
        out.append(x)
    return tuple(out)


def cut(flat, sizes):
    ts, off = [], 0
    for k in sizes:
        ts.append(flat[off:off + k])
        off += k
    assert off == len(flat)
    return ts


# --------------------------------------------------------------------------------------------------------- mutants
def _wide(dt):
    return F64 if dt is F32 else np.longdouble


def _flush(x, dt):
    return np.where(np.abs(x) < dt(_MIN[dt]), np.copysign(dt(0), x), x)


def _fedopt_mutant(kind, opt, theta, delta, v, lr, beta2, tau, dt):
    """fedopt_step with one departure (``kind``); the rest is the stepwise reference's text."""
    lrs, b2, omb, nomb, taus = sx.fedopt_scalars(lr, beta2, tau, dt)
    th, d, vi = (np.asarray(a, dtype=dt) for a in (theta, delta, v))
    with np.errstate(all="ignore"):
        d2 = d * d
        if kind == "flush_subnormals":
            d2, vi = _flush(d2, dt), _flush(vi, dt)
        if opt == "adagrad":
            vi = sx.fma_exact(d, d, vi, dt) if kind == "adagrad_contracted" else vi + d2
        elif opt == "yogi":
            diff = vi - d2
            sg = sx._sign(diff)
            if kind == "yogi_sign0_plus":
                sg = np.where(diff == 0, dt(1), sg)
            elif kind == "yogi_sign0_minus":
                sg = np.where(diff == 0, dt(-1), sg)
            vi = vi + (nomb * d2) * sg
        else:
            vi = (omb * d2) + (vi * b2) if kind == "adam_unfused" else sx.fma_exact(omb, d2, vi * b2, dt)
        if kind == "den_rounded_once":
            w = _wide(dt)
            den = (np.sqrt(vi.astype(w)) + w(taus)).astype(dt)
        else:
            den = np.sqrt(vi) + taus
        if kind == "lr_times_quotient":
            th = th + lrs * (d / den)
        elif kind == "times_reciprocal":
            th = th + (lrs * d) * (dt(1) / den)
        else:
            th = th + (lrs * d) / den
    return th, vi


_ADAPTIVE = ("adagrad", "yogi", "adam")
# name -> the optimisers whose text the departure changes
FEDOPT_MUTANTS = {
    "adam_unfused": ("adam",), "adagrad_contracted": ("adagrad",), "yogi_sign0_plus": ("yogi",),
    "yogi_sign0_minus": ("yogi",), "lr_times_quotient": _ADAPTIVE, "times_reciprocal": _ADAPTIVE,
    "den_rounded_once": _ADAPTIVE, "flush_subnormals": _ADAPTIVE,
}


def mutant_taus(name):
    """The tau values at which the mutant is a departure at all.  ``den_rounded_once`` is none at tau = 0: the
    denominator is then sqrt(v) alone, and a square root taken in a wider type and rounded is the correctly rounded
    square root again (from 2p + 2 bits always; fp32 through fp64 has them), so the two texts compute one value."""
    return TAUS[:1] if name == "den_rounded_once" else TAUS


def fedopt_mutant(name, opt, theta, delta, v, tau, dtype=F32):
    assert opt in FEDOPT_MUTANTS[name]
    dt = np.dtype(dtype).type
    return _fedopt_mutant(name, opt, theta, delta, v, LR, BETA2, tau, dt)


def feddr_mutant(name, theta, y, x_til, p, dtype=F32):
    """FedDR's L1 prox with ``clamp_drops_nan`` (max(m, 0) returning 0 for a NaN m) or ``sign_of_minus_zero``
    (sign(-0) = -1)."""
    dt = np.dtype(dtype).type
    th, yo, xt = (np.asarray(t, dtype=dt) for t in (theta, y, x_til))
    with np.errstate(all="ignore"):
        yn = sx.fma_exact(dt(p["alpha"]), th - yo, yo, dt)
        t = dt(p["cx"]) * xt + dt(p["cy"]) * yn
        m = np.abs(t) - dt(p["pc"])
        sg = sx._sign(t)
        if name == "clamp_drops_nan":
            m = np.where(m > 0, m, dt(0))
        else:
            m = np.where(m < 0, dt(0), m)
        if name == "sign_of_minus_zero":
            sg = np.where((t == 0) & np.signbit(t), dt(-1), sg)
        return sg * m, yn


FEDDR_MUTANTS = ("clamp_drops_nan", "sign_of_minus_zero")
