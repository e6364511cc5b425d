"""GPU parity of flc_avg_and_gradient_dense_records (wire.hip dense_fold_records_kernel<KIND, BITS, PairIO>) against
the chain it replaces — every record decoded densely (flc_quant_decode / flc_natural_decode), then
flc_avg_and_gradients — bit for bit over the whole backing buffers, so the guard elements before and after every tensor
must be untouched: every code format, tile edges and sub-byte tails, the record, parameter-source and tensor chains,
weights, parameters and norms at their edge values, and the gradients-only form."""

import ctypes

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests.test_gpu_dense_wire import (FORMATS, NATD, NATURAL, STD, WEIGHTS, _block, _cut, _decode, _fid, _seed_acc,
                                       _splits, _with_norms)

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
THREE = [(STD, 4, 7), (NATD, 8, 127), (NATURAL, 16, 0)]
GAP = 4  # guard elements between consecutive tensors (a multiple of 4: every tensor keeps its contiguous cut's alignment)
SENTINEL = 7.5  # the gradient buffer's guards (finite, so an overwrite by anything — a NaN included — shows)


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1)


def _spread(base, lead, sizes):
    """Tensor t at ``lead + start_t + GAP * t`` of ``base``: the contiguous cut's alignment, with guards between."""
    ts, off = [], lead
    for m in sizes:
        ts.append(base[off:off + m])
        off += m + GAP
    return ts


def _span(n, lead, sizes):
    return lead + n + GAP * len(sizes) + 3


def _state(n, lead, sizes, seed):
    """(parameter buffer, its tensors, gradient buffer, its tensors): the parameters with -0, +-inf and NaN lanes, the
    gradient tensors NaN (the chain starts at +0, not at the stored value) between finite guards."""
    span = _span(n, lead, sizes)
    pbase = _seed_acc(span, seed)
    gbase = torch.full((span,), SENTINEL, device="cuda")
    gs = _spread(gbase, lead, sizes)
    for g in gs:
        g.fill_(float("nan"))
    return pbase, _spread(pbase, lead, sizes), gbase, gs


def _layouts(n):
    """(label, sizes, lead): one tensor; the unaligned split cut one element in; seventeen tensors (two tensor launches)
    cut one element in, and the same split aligned (every fourth tensor takes the float4 path)."""
    out = []
    for name, sizes in _splits(n).items():
        out.append((name, sizes, 0 if name == "one" else 1))
        if name == "seventeen":
            out.append(("seventeen_aligned", sizes, 0))
    return out


def _run(fmt, n, recs, psrc_seed):
    """The entry against decode-then-flc_avg_and_gradients for every layout, with and without parameter sources."""
    from fl_sim_amd import _lib

    kind, bits, s = fmt
    m = len(recs)
    wg = [WEIGHTS[c % len(WEIGHTS)] for c in range(m)]
    wp = [WEIGHTS[(c + 2) % len(WEIGHTS)] for c in range(m)]
    dec_flat = [_decode(r, kind, bits, s, n) for r in recs]  # the reference's decoded vectors, made once
    g = torch.Generator(device="cuda").manual_seed(psrc_seed)
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    fl = lambda v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    rptr = ptr(recs)
    for label, sizes, lead in _layouts(n):
        T = len(sizes)
        sz = (ctypes.c_int64 * T)(*sizes)
        psrc_flat = [torch.randn(n + lead, generator=g, device="cuda")[lead:] for _ in range(m)]
        psrc = ptr([t for f in psrc_flat for t in _cut(f, sizes)])
        dec = ptr([t for f in dec_flat for t in _cut(f, sizes)])
        for inertia in (0.1, 0.0):
            pa, ta, ga, gta = _state(n, lead, sizes, 11 * n + m)
            pb, tb, gb, gtb = _state(n, lead, sizes, 11 * n + m)
            _lib.call("flc_avg_and_gradient_dense_records", ptr(ta), ptr(gta), psrc, rptr, fl(wp), fl(wg), m, n, kind, s,
                      bits, sz, T, inertia, None)
            _lib.call("flc_avg_and_gradients", ptr(tb), ptr(gtb), psrc, dec, fl(wp), fl(wg), m, sz, T, inertia, None)
            torch.cuda.synchronize()
            assert gc.same_bits(_bits(pa), _bits(pb)), (label, inertia, "parameters")
            assert gc.same_bits(_bits(ga), _bits(gb)), (label, inertia, "gradients")
            fresh_g = _state(n, lead, sizes, 11 * n + m)[2]
            guards = torch.isfinite(fresh_g)
            assert gc.same_bits(_bits(ga[guards]), _bits(fresh_g[guards])), (label, "gradient guards")
        # update_gradients alone: param_srcs NULL, the parameters (given or not) keep their bits
        for give_params in (True, False):
            pa, ta, ga, gta = _state(n, lead, sizes, 11 * n + m)
            _lib.call("flc_avg_and_gradient_dense_records", ptr(ta) if give_params else None, ptr(gta), None, rptr, None,
                      fl(wg), m, n, kind, s, bits, sz, T, 0.1, None)
            torch.cuda.synchronize()
            assert gc.same_bits(_bits(pa), _bits(_state(n, lead, sizes, 11 * n + m)[0])), (label, "parameters untouched")
            assert gc.same_bits(_bits(ga), _bits(gb)), (label, "gradients alone")


@pytest.mark.parametrize("n,m", [(4097, 3), (70001, 10)])
@pytest.mark.parametrize("fmt", FORMATS, ids=_fid)
def test_every_format_equals_decode_then_avg_and_gradients(fmt, n, m):
    """All eleven formats; at 70001 the records' norms at their edge values (0, +inf, NaN, a subnormal)."""
    kind, bits, s = fmt
    block = _block(kind, bits, s, n)
    wires = _with_norms(block, kind, bits, n, m) if n == 70001 else block[:m]
    _run(fmt, n, [wires[r] for r in range(m)], n + m)
    # the inputs do hold the -0 decode: a code that is the sign bit alone (natural dithering with 127 levels has its
    # first level at 2^-126 of the norm, below every input here)
    if kind != NATURAL and not (kind == NATD and s > 30):
        dec = _bits(_decode(block[0], kind, bits, s, n))
        assert (dec.view(np.uint32) == 0x80000000).any() and (dec.view(np.uint32) == 0).any()


@pytest.mark.parametrize("m", [17, 65])
@pytest.mark.parametrize("fmt", THREE, ids=_fid)
def test_chained_launches_equal_the_chain(fmt, m):
    """17 messages: the parameter sources take two launches, the second without records.  65: the records take two
    launches and the sources five, three of which carry sources only; without sources both record launches carry
    records only."""
    kind, bits, s = fmt
    n = 4097
    block = _block(kind, bits, s, n)
    _run(fmt, n, [block[r] for r in range(m)], n + m)


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025])
@pytest.mark.parametrize("fmt", THREE, ids=_fid)
def test_tile_borders_and_tails(fmt, n):
    """A partial last group, a code word reaching into the record's padding, and exact tile borders."""
    kind, bits, s = fmt
    block = _block(kind, bits, s, n)
    _run(fmt, n, [block[r] for r in range(3)], n)


def test_rejects_bad_arguments_on_the_device():
    from fl_sim_amd import _lib, codec

    n = 5000
    stride, _ = codec.dense_wire_layout(n, STD, 4)
    rec = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    g = torch.ones(n, device="cuda")
    one = (ctypes.c_float * 1)(1.0)
    with pytest.raises(_lib.FlcError, match="hold"):
        _lib.call("flc_avg_and_gradient_dense_records", None, (P * 1)(g.data_ptr()), None, (P * 1)(rec.data_ptr()), None,
                  one, 1, n, STD, 7, 4, (ctypes.c_int64 * 1)(n - 1), 1, 0.0, None)
    with pytest.raises(_lib.FlcError, match="aligned"):
        _lib.call("flc_avg_and_gradient_dense_records", None, (P * 1)(g.data_ptr()), None, (P * 1)(rec.data_ptr() + 8),
                  None, one, 1, n, STD, 7, 4, (ctypes.c_int64 * 1)(n), 1, 0.0, None)
    with pytest.raises(_lib.FlcError, match="does not fit"):
        _lib.call("flc_avg_and_gradient_dense_records", None, (P * 1)(g.data_ptr()), None, (P * 1)(rec.data_ptr()), None,
                  one, 1, n, STD, 8, 4, (ctypes.c_int64 * 1)(n), 1, 0.0, None)
    torch.cuda.synchronize()
    assert bool((g == 1).all())  # (nothing launched)
