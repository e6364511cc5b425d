"""The scaled-sign codec on the device: encode / decode against plain numpy (np.signbit; math.fsum(|x|) / m per
bucket), the four sign-record folds against flc_sign_decode + their dense counterparts, one round through the mixin."""

import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from fl_sim_amd import _lib as lib, codec
from oracle.server_steps_exact import fma_exact
from tests import golden_cases as gc

pytestmark = pytest.mark.gpu

F32 = np.float32
_dev = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731  (a copy: the cached references are read-only)


def _decoded(scales, neg, n, B):
    per = np.repeat(scales, B or n)[:n]
    return np.where(neg, -per, per).astype(F32)


@functools.lru_cache(maxsize=None)
def _case(cls, n, B):
    """(x, scales, bits) of the numpy reference; computed once per case and never written to."""
    g = np.random.default_rng(1000 * n + B + (cls == "exact"))
    if cls == "exact":  # integer multiples of 2^-12 below 2^12: every fp64 partial sum is exact in any order
        x = (g.integers(-(1 << 24) + 1, 1 << 24, n).astype(np.float64) * 2.0 ** -12).astype(F32)
        x[g.random(n) < 0.1] = 0.0
        x[g.random(n) < 0.1] = -0.0
        if B and n > B:  # an all-zero bucket of both zeros
            x[B:2 * B] = np.where(g.random(min(B, n - B)) < 0.5, F32(0.0), F32(-0.0))
    else:  # normal fp32 values over 40 binades
        x = (g.standard_normal(n) * 2.0 ** g.integers(-20, 21, n)).astype(F32)
    w = B or n
    scales = np.array([F32(np.float64(math.fsum(np.abs(x[lo:lo + w]).astype(np.float64).tolist())) / x[lo:lo + w].size)
                       for lo in range(0, n, w)], dtype=F32)
    bits = np.packbits(np.signbit(x), bitorder="little")
    for a in (x, scales, bits):
        a.setflags(write=False)
    return x, scales, bits


def _encode(x, B, inplace=False):
    xd = _dev(x)
    res = xd if inplace else torch.empty_like(xd)
    rec, out = codec.sign_encode(xd, B, decode=True, residual=res)
    sv, bv = codec.sign_wire_views(rec, x.size, B)
    return sv.cpu().numpy(), bv.cpu().numpy(), out.cpu().numpy(), res.cpu().numpy()


@pytest.mark.parametrize("B", [0, 64, 512, 1024, 4096])
@pytest.mark.parametrize("n", [1, 7, 9, 63, 65, 513, 4095, 4097, 70001])
@pytest.mark.parametrize("cls", ["exact", "general"])
def test_encode(cls, n, B):
    """Bits exact; exact class: scales (hence out, residual) bit-equal; general class: each scale the reference's or an
    adjacent fp32 (an fp64 sum of m <= 70001 terms is within m * 2^-53 relative of exact: at most one fp32 step).  Both:
    out is +- the record's own scale, residual fp32(x - out); the in-place run and a rerun give the same bytes."""
    x, scales, bits = _case(cls, n, B)
    sc, bt, out, res = _encode(x, B)
    assert np.array_equal(bt, bits)
    if cls == "exact":
        assert gc.same_bits(sc, scales)
    else:
        assert np.all((sc == scales) | (sc == np.nextafter(scales, F32(np.inf))) | (sc == np.nextafter(scales, F32(-np.inf))))
    assert gc.same_bits(out, _decoded(sc, np.signbit(x), n, B)) and gc.same_bits(res, (x - out).astype(F32))
    for again in (_encode(x, B, inplace=True), _encode(x, B)):
        assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(again, (sc, bt, out, res)))


def _handbuilt(n, B, seed):
    """(record bytes, decoded values) of a record written in numpy: random bits, scales of both signs and zero."""
    g = np.random.default_rng(seed)
    total, off = codec.sign_wire_layout(n, B)
    scales = (g.integers(-40, 41, -(-n // B) if B else 1) / 16.0).astype(F32)
    bits = g.integers(0, 256, (n + 7) // 8, dtype=np.uint8)
    rec = g.integers(0, 256, total, dtype=np.uint8)  # (the padding is never interpreted)
    rec[:scales.nbytes] = scales.view(np.uint8)
    rec[off["bits"]:off["bits"] + bits.size] = bits
    return rec, _decoded(scales, np.unpackbits(bits, bitorder="little")[:n].astype(bool), n, B)


@pytest.mark.parametrize("weight,accumulate", [(1.0, False), (-0.75, False), (0.3, True), (1.0, True)])
@pytest.mark.parametrize("n,B", [(9, 0), (4097, 0), (4097, 512), (70001, 4096)])
def test_decode_of_a_handbuilt_record(n, B, weight, accumulate):
    rec, v = _handbuilt(n, B, n + B)
    acc0 = (np.random.default_rng(n).standard_normal(n + 8)).astype(F32)
    out = _dev(acc0)
    codec.sign_decode(_dev(rec), n, B, out=out[:n], weight=weight, accumulate=accumulate)
    want = fma_exact(F32(weight), v, acc0[:n], F32) if accumulate else F32(weight) * v
    assert gc.same_bits(out.cpu().numpy(), np.concatenate([want, acc0[n:]]))  # (nothing written past n)


FOLD_N = 4097  # the folds
SIZES = [5, 257, 521, 1023, FOLD_N - 1806]  # tensor boundaries inside a bucket and off every multiple of 4
WEIGHTS = [0.5, -1.25, 0.0, 1.0, -0.001, 3.0]
_cut =lambda flat: list(torch.split(flat, SIZES))  # noqa: E731
_ptrs = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731


def _state(count, seed, shift=1):
    """``count`` flat fp32 vectors ``shift`` elements into one buffer (1: no tensor is 16-B aligned but by accident)."""
    span = FOLD_N + 3
    base = torch.randn(count * span, generator=torch.Generator().manual_seed(seed)).cuda()
    return base, [base[k * span + shift:k * span + shift + FOLD_N] for k in range(count)]


@functools.lru_cache(maxsize=None)
def _round(R, B):
    """(records [R, stride] on the device, their flc_sign_decode vectors, weights)."""
    recs = _dev(np.stack([_handbuilt(FOLD_N, B, 31 * R + c)[0] for c in range(R)]))
    dec = [codec.sign_decode(recs[c], FOLD_N, B, out=torch.zeros(FOLD_N, device="cuda")) for c in range(R)]
    return recs, dec, [WEIGHTS[c % len(WEIGHTS)] for c in range(R)]


@pytest.mark.parametrize("B", [0, 512])
@pytest.mark.parametrize("R", [1, 3, 17, 65])  # (across the 16-record batch and the 64-record launch chain)
@pytest.mark.parametrize("form", ["wires", "groups", "fedopt_avg", "fedopt_adam", "gradient"])
def test_folds_equal_decode_then_dense(form, R, B):
    recs, dec, w = _round(R, B)
    n, T, wf = FOLD_N, len(SIZES), (ctypes.c_float * R)(*w)
    rptr, sz = _ptrs(list(recs)), (ctypes.c_int64 * T)(*SIZES)
    res = []
    for fused in (True, False):
        if form == "wires":  # (flc_fold_*_wires take a 16-B aligned out: spans of 4100 floats)
            base, (a, b) = _state(2, R, shift=0)
            for out, accumulate in ((a, 0), (b, 1)):
                if fused:
                    lib.call("flc_fold_sign_wires", recs.data_ptr(), recs.shape[1], (ctypes.c_int32 * R)(*range(R)),
                             wf, R, n, B, accumulate, out.data_ptr(), None)
                else:
                    codec.weighted_sum(out, dec, w, 2 if accumulate else 1)
        elif form == "groups":  # groups 0 and 2 share the records in turn, group 1 stays idle
            base, flats = _state(3, R)
            gof = [0 if c % 3 else 2 for c in range(R)]
            if fused:
                lib.call("flc_fold_sign_record_groups", rptr, wf, (ctypes.c_int32 * R)(*gof), R, n, B,
                         _ptrs([t for f in flats for t in _cut(f)]), 3, sz, T, None)
            for g in () if fused else (0, 2):
                mem = [c for c in range(R) if gof[c] == g]
                for t, dst in enumerate(_cut(flats[g]) if mem else []):
                    codec.weighted_sum(dst, [_cut(dec[c])[t] for c in mem], [w[c] for c in mem], 2)
        elif form.startswith("fedopt"):
            opt, beta0, lr, beta2, tau = (("avg", 0.0, 1.0, 1.0, 1.0) if form == "fedopt_avg" else
                                          ("adam", 0.9, 0.01, 0.99, 1e-3))
            base, (theta, delta, v) = _state(3, R)
            v.abs_().add_(1e-6)
            th, dl, vv = _cut(theta), _cut(delta), (_cut(v) if opt != "avg" else None)
            if fused:
                lib.call("flc_fedopt_fold_sign_records", rptr, wf, R, n, B, _ptrs(dl), _ptrs(th),
                         _ptrs(vv) if vv else None, sz, T, beta0, lib.FLC_OPT[opt], lr, beta2, tau, None)
            else:
                codec.model_fold(dl, [_cut(d) for d in dec], w, 0, beta0, theta=th, v=vv, opt=opt, lr=lr, beta2=beta2,
                                 tau=tau)
        else:
            base, (params, grads) = _state(2, R)
            _, psrc_flat = _state(R, R + 1)
            args = (_ptrs(_cut(params)), _ptrs(_cut(grads)), _ptrs([t for f in psrc_flat for t in _cut(f)]),
                    rptr if fused else _ptrs([t for d in dec for t in _cut(d)]), (ctypes.c_float * R)(*w[::-1]), wf, R)
            if fused:
                lib.call("flc_avg_and_gradient_sign_records", *args, n, B, sz, T, 0.25, None)
            else:
                lib.call("flc_avg_and_gradients", *args, sz, T, 0.25, None)
        torch.cuda.synchronize()
        res.append(base.cpu().numpy())
    assert gc.same_bits(res[0], res[1])


def test_fedopt_round_with_records_and_feedback_equals_the_decoded_round():
    """Three clients with ``wire_records`` and ``error_feedback``: every message carries the sign record, and the
    server's model and every client's memory equal those of the same round with ``wire_records`` off."""
    from fl_sim_amd import SignCompressor
    from tests.test_gpu_round import build_round

    shapes = [(64, 3, 3), (4096,), (300, 77)]
    n = sum(int(np.prod(sh)) for sh in shapes)
    got = {}
    for wire in (True, False):
        s, clients = build_round(shapes, "avg", "cuda", n_clients=3)
        for c in clients:
            c.compressors, c.error_feedback, c.wire_records = [SignCompressor(n, bucket=512)], True, wire
            c.communicate(s)
        msgs = [m["delta_parameters"] for m in s._received_messages]
        if wire:
            assert all(d.kind == "sign" and d.nbytes == codec.sign_wire_layout(n, 512)[0] for d in msgs)
            assert all(c.compressors[0].last_need_to_send_advance == -(-n // 512) + n / 32.0 for c in clients)
        s.update()
        assert not wire or all(d._flat is None for d in msgs)  # (folded from the records, never decoded)
        got[wire] = ([p.detach().cpu().numpy().ravel() for p in s.model.parameters()]
                     + [c.error_memory("delta_parameters").value().cpu().numpy() for c in clients])
    assert all(gc.same_bits(a, b) for a, b in zip(got[True], got[False])) and all(e.any() for e in got[True][-3:])
