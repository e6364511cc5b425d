"""Bucketed dithering on the edges (gfx950): flc_bucket_encode / _encode_round / _decode, the four ``*_bucket_*`` folds
and Compressor(bucket=B) against the catalogue and numpy models of tests/bucket_cases.py (anchored on the CPU by
tests/test_bucket_cases.py), at every bucket size from 64 to 4096.  The encoder on messages whose every element stands a
margin's width from its decision, neighbouring buckets under norms from 3e-42 to FLT_MAX; the p = 2 norms bit for bit
against the documented summation order, a subnormal norm, an overflow to inf and a bucket whose fp32 norm depends on
the wave order; the decoder and the folds on hand-built records with negative, -0, -inf and NaN norms next to regular
ones, every code of the format, n % 4 == 2 and a sentinel in the padding.  Everything bit for bit (any NaN equals any
NaN); codes and counts as integers."""

import ctypes
import functools
import pickle

import numpy as np
import pytest
import torch

from tests import bucket_cases as bc
from tests import bucket_ref as br
from tests import decode_cases as dc
from tests import golden_cases as gc
from tests import quant_cases as qc

pytestmark = pytest.mark.gpu
F32 = np.float32
STD, NAT = bc.STD, bc.NAT
INF, L2 = 0, 2
SENTINEL = 12345.0
GUARD = 64
P = ctypes.c_void_p


def _codec():
    from fl_sim_amd import codec

    return codec


def _lib():
    from fl_sim_amd import _lib

    return _lib


def _dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the catalogue's arrays are read-only)


def _record(n, kind, bits, B, rows=None):
    """A PAD-filled record (or [rows, stride] block) and its layout, which is the catalogue's."""
    stride, off = _codec().bucket_wire_layout(n, kind, bits, B)
    assert (stride, off["codes"]) == bc.wire_layout(n, bits, B) and off["norms"] == 0
    shape = (stride,) if rows is None else (rows, stride)
    return torch.full(shape, bc.PAD, dtype=torch.uint8, device="cuda"), off["codes"]


def _fields(rec, n, bits, B, off):
    """(norms, unpacked codes) of a record on the host, after checking that its padding still holds PAD."""
    r = rec.cpu().numpy()
    nb, nbytes = -(-n // B), (n * bits + 7) // 8
    assert (r[4 * nb:off] == bc.PAD).all() and (r[off + nbytes:] == bc.PAD).all(), "the record's padding was written"
    return r[:4 * nb].view(F32), dc.unpack(r[off:off + nbytes], n, bits)


def _check_codes(got, want, x, tag):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (tag, "codes", bad.size, [(int(i), float(x[i]), int(got[i]), int(want[i])) for i in bad[:5]])


def _same_norms(got, want):
    return gc.same_bits(np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32))


# ------------------------------------------------------------------------------------------------ 1. decision edges
EDGE_LEVELS = [(STD, s, i) for i, s in enumerate(qc.LEVELS_STD)] + [(NAT, s, i) for i, s in enumerate(qc.LEVELS_NAT)]


@pytest.mark.parametrize("B", bc.ALL_B)
@pytest.mark.parametrize("kind,s,i", EDGE_LEVELS, ids=[f"{'std' if k == STD else 'nat'}{s}" for k, s, _ in EDGE_LEVELS])
def test_encode_on_the_decision_edges(kind, s, i, B):
    """p = inf and given norms against the catalogue, the decode of the record, the padding, and the round form over 3
    and over 65 messages (a chained launch), each message with its own seed and counter."""
    codec = _codec()
    tail, rot = bc.rotation(kind, B, i)
    bits = br.code_bits(s)
    keys = [(bc.SEED + c, bc.CTR + 7 * c) for c in range(3)]
    msgs = [bc.edge_message(kind, s, B, tail, rot + c, *keys[c]) for c in range(3)]
    n = len(msgs[0][0])
    assert all(len(m[0]) == n for m in msgs)
    xd = [_dev(m[0]) for m in msgs]
    singles = []
    for c, (x, norms, codes, out, nnz) in enumerate(msgs):
        tag = (kind, s, B, tail, c)
        rec, off = _record(n, kind, bits, B)
        _, got_nnz, got_out = codec.bucket_encode(xd[c], kind, s, B, np.inf, *keys[c], record=rec, want_nnz=True,
                                                  decode=True)
        nv, cv = _fields(rec, n, bits, B, off)
        assert np.array_equal(nv.view(np.uint32), norms.view(np.uint32)), (tag, "norms")
        _check_codes(cv, codes, x, tag)
        assert gc.same_bits(got_out.cpu().numpy(), out), (tag, "out")
        assert int(got_nnz.item()) == nnz, (tag, "nnz")
        singles.append(rec)
        if c == 0:  # the same message under given norms, and the record decoded
            rec2, _ = _record(n, kind, bits, B)
            _, nnz2, out2 = codec.bucket_encode(xd[0], kind, s, B, np.inf, *keys[0], record=rec2, norms=_dev(norms),
                                                want_nnz=True, decode=True)
            assert torch.equal(rec2, rec) and int(nnz2.item()) == nnz, (tag, "given norms")
            assert gc.same_bits(out2.cpu().numpy(), out), (tag, "given norms, out")
            assert gc.same_bits(codec.bucket_decode(rec, n, kind, s, bits, B).cpu().numpy(), out), (tag, "decode")
    # the round form: 3 messages, then 65 (message c = message c % 3 under its own seed and counter)
    recs, _ = _record(n, kind, bits, B, rows=3)
    counts = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    codec.bucket_encode_round(xd, kind, s, bits, B, INF, [k[0] for k in keys], [k[1] for k in keys],
                              [recs[c] for c in range(3)], counts=[counts[c:c + 1] for c in range(3)])
    assert torch.equal(recs, torch.stack(singles)) and counts.tolist() == [m[4] for m in msgs]
    C = 65
    seeds = [bc.SEED + c % 3 + 11 * (c // 3) for c in range(C)]
    ctrs = [bc.CTR + 7 * (c % 3) + 1000 * (c // 3) for c in range(C)]
    assert (seeds[:3], ctrs[:3]) == ([k[0] for k in keys], [k[1] for k in keys])
    recs, _ = _record(n, kind, bits, B, rows=C)
    codec.bucket_encode_round([xd[c % 3] for c in range(C)], kind, s, bits, B, INF, seeds, ctrs,
                              [recs[c] for c in range(C)])
    each, _ = _record(n, kind, bits, B, rows=C)
    for c in range(3, C):
        codec.bucket_encode(xd[c % 3], kind, s, B, np.inf, seeds[c], ctrs[c], record=each[c])
    each[:3] = torch.stack(singles)
    assert torch.equal(recs, each)
    assert not torch.equal(recs[0], recs[3]) and not torch.equal(recs[64], recs[61])


# ------------------------------------------------------------------------------------------------ 2. the p = 2 norm
@pytest.mark.parametrize("B", bc.ALL_B)
def test_p2_norms_follow_the_documented_order(B):
    codec = _codec()
    x, where = bc.l2_message(B)
    n = len(x)
    model = bc.l2_norm_model(x, B)
    xd = _dev(x)
    mask8 = 127
    for kind, s in ((STD, 127), (NAT, 8), (STD, 1)):
        bits = br.code_bits(s)
        tag = (B, kind, s)
        rec, off = _record(n, kind, bits, B)
        _, nnz, out = codec.bucket_encode(xd, kind, s, B, 2, bc.SEED, bc.CTR, record=rec, want_nnz=True, decode=True)
        nv, cv = _fields(rec, n, bits, B, off)
        bad = [(b, float(nv[b]), float(model[b])) for b in range(len(model))
               if not _same_norms(nv[b:b + 1], model[b:b + 1])]
        assert not bad, (tag, "norms (bucket, got, model)", bad[:5], {k: v for k, v in where.items()})
        want_out, want_codes, want_nnz = br.bucket_philox(x, kind, s, B, nv, bc.SEED, bc.CTR)
        _check_codes(cv, want_codes, x, tag)
        assert gc.same_bits(out.cpu().numpy(), want_out), (tag, "out")
        assert int(nnz.item()) == want_nnz
        assert gc.same_bits(codec.bucket_decode(rec, n, kind, s, bits, B).cpu().numpy(), want_out), (tag, "decode")
        # the special buckets
        sub = where["subnormal"]
        assert 0 < nv[sub] < np.finfo(F32).tiny, (tag, "the subnormal norm was flushed")
        if s == 127:  # ordinary codes: y = 1 / sqrt(B) lies between two levels above 0, not the 0 / 1 of "no norm"
            assert int((cv[sub * B:(sub + 1) * B] & mask8).max()) > 1
        for name in ("overflow", "nan", "inf"):
            b = where[name]
            assert np.isnan(nv[b]) if name == "nan" else np.isposinf(nv[b])
            xs = x[b * B:(b + 1) * B]
            assert np.array_equal(cv[b * B:(b + 1) * B], (xs != 0).astype(np.uint8)), (tag, name, "code 0 / code 1")
        assert np.isfinite(nv[where["below_max"]]) and nv[where["below_max"]] > F32(0.99) * bc.FLT_MAX


@pytest.mark.parametrize("B", bc.ALL_B)
def test_p2_norm_does_not_depend_on_the_position(B):
    """The same bucket contents at bucket 0, in a later wave, in later blocks, in messages of different n and in a
    round of three messages: one norm, the model's."""
    codec = _codec()
    x, where = bc.l2_message(B)
    picks = [0, where["subnormal"], where["below_max"]] + ([where["tie"]] if B >= 2048 else [])
    contents = [x[b * B:(b + 1) * B] for b in picks]
    want = [bc.l2_norm_model(c, B)[0] for c in contents]
    kind, s, bits = STD, 7, 4
    per_block = bc.BLOCK // B
    places = [[1 + k for k in range(len(contents))],  # block 0 (B < 4096: a later wave or sub-wave group)
              [per_block + 1 + 2 * k for k in range(len(contents))],  # from block 1 on, every other bucket
              [2 * per_block + 3 + k for k in range(len(contents))]]
    nb = max(max(p) for p in places) + 2
    n = nb * B - 5
    msgs = []
    for m, place in enumerate(places):
        y = bc.general_buckets(B, nb, 100 + m)[:n].copy()
        for c, b in zip(contents, place):
            y[b * B:(b + 1) * B] = c
        msgs.append(_dev(y))
    got = []
    for m, place in enumerate(places):
        rec, off = _record(n, kind, bits, B)
        codec.bucket_encode(msgs[m], kind, s, B, 2, 5, m, record=rec)
        got.append(_fields(rec, n, bits, B, off)[0][place])
    recs, off = _record(n, kind, bits, B, rows=3)
    codec.bucket_encode_round(msgs, kind, s, bits, B, L2, [5, 5, 5], [0, 1, 2], [recs[m] for m in range(3)])
    for m, place in enumerate(places):
        got.append(_fields(recs[m], n, bits, B, off)[0][place])
    for c in contents:  # alone, and first in a message of B + 1 elements
        for extra in (0, 1):
            y = np.concatenate([c, np.ones(extra, dtype=F32)])
            rec, off = _record(B + extra, kind, bits, B)
            codec.bucket_encode(_dev(y), kind, s, B, 2, 5, 9, record=rec)
            nv = _fields(rec, B + extra, bits, B, off)[0]
            assert _same_norms(nv[:1], bc.l2_norm_model(c, B)[:1]), (B, "alone", extra)
    for g in got:
        assert _same_norms(g, np.array(want, dtype=F32)), (B, [float(v) for v in g], [float(v) for v in want])


# ------------------------------------------------------------------------------------------------ 3. the decoder
LEVELS_OF_BITS = {2: (1, 1), 4: (7, 5), 8: (127, 100)}


def _levels(bits, B, kind):
    return LEVELS_OF_BITS[bits][(bc.ALL_B.index(B) + kind) % 2]


class _View:
    """``out``: n elements 16 B into a buffer of sentinels, holding ``start`` (or sentinels)."""

    def __init__(self, n, start=None):
        self.buf = torch.full((4 + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.out = self.buf[4:4 + n]
        if start is not None:
            self.out.copy_(torch.from_numpy(start))
        self.n = n

    def result(self, what):
        host = self.buf.cpu().numpy()
        assert (host[:4] == SENTINEL).all() and (host[4 + self.n:] == SENTINEL).all(), f"a write outside out: {what}"
        return host[4:4 + self.n]


def _decode(rec, n, kind, s, bits, B, weight, acc0, what):
    view = _View(n, acc0)
    _codec().bucket_decode(rec, n, kind, s, bits, B, out=view.out, weight=weight, accumulate=acc0 is not None)
    return view.result(what)


@pytest.mark.parametrize("B", bc.ALL_B)
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("kind", [STD, NAT])
def test_decode_of_handbuilt_records(kind, bits, B):
    """Plain, under each weight, and accumulating under each weight onto an accumulator with -0, +-inf, NaN and
    denormal lanes; nothing is written past n.  A record of one bucket meets every norm of the cycle."""
    s = _levels(bits, B, kind)
    for i, name in enumerate(bc.RECORD_SIZES):
        n = bc.record_size(name, B)
        start = bc.ALL_B.index(B) + 3 * i + bits
        starts = [start] if n > B else [start + k for k in range(len(bc.RECORD_NORMS))]
        acc0 = dc.seed_acc(n, n + bits)
        for k, st in enumerate(starts):
            rec, _, _, values = bc.handbuilt_record(kind, s, bits, B, n, st)
            drec = _dev(rec)
            tag = (kind, s, bits, B, n, st)
            assert gc.same_bits(_decode(drec, n, kind, s, bits, B, 1.0, None, tag), values), (tag, "plain")
            if k:
                continue
            for w in dc.WEIGHTS:
                assert gc.same_bits(_decode(drec, n, kind, s, bits, B, w, None, tag),
                                    dc.weighted(values, w, False)), (tag, "weight", w)
                assert gc.same_bits(_decode(drec, n, kind, s, bits, B, w, acc0, tag),
                                    dc.weighted(values, w, True, acc0)), (tag, "accumulate", w)
            assert torch.equal(drec.cpu(), torch.from_numpy(rec))  # (the record is only read)


# ------------------------------------------------------------------------------------------------ 4. the folds
FOLD_FORMATS = [(STD, 7, 4), (NAT, 127, 8), (STD, 1, 2), (NAT, 5, 4), (STD, 127, 8), (NAT, 1, 2), (STD, 100, 8)]
FOLD_WEIGHTS = [1.0, 0.37, -1.5, 3e-39, 0.0, -0.0, 0.125, -0.77]
FOLD_R = [1, 3, 17, 65]


def _fold_format(B, R):
    return FOLD_FORMATS[(bc.ALL_B.index(B) + FOLD_R.index(R)) % len(FOLD_FORMATS)]


@functools.lru_cache(maxsize=8)
def _fold_round(B, R, n):
    """R hand-built records of one format: (format, [R + 3, stride] host block, slots, weights, decoded values).
    Three records get norms of their own; beyond that the records share their norms (start + 11 c), so that the
    buckets with a regular norm carry numbers through the whole chain, and differ in their codes."""
    kind, s, bits = _fold_format(B, R)
    rows = R + 3
    slots = [(7 * c + 2) % rows for c in range(R)]  # not consecutive, not ascending
    assert len(set(slots)) == R
    stride, _ = bc.wire_layout(n, bits, B)
    block = np.full((rows, stride), bc.PAD, dtype=np.uint8)
    values = []
    for c in range(R):
        start = 1 + c if R <= 3 else 1 + len(bc.RECORD_NORMS) * c
        rec, _, _, v = bc.handbuilt_record(kind, s, bits, B, n, start)
        block[slots[c]] = rec
        values.append(v)
    weights = [FOLD_WEIGHTS[(c + R) % len(FOLD_WEIGHTS)] for c in range(R)]
    return (kind, s, bits), block, slots, weights, values


def _fold_sizes(B):
    return [6, bc.BLOCK + B + 2]


def _tensor_sizes(n, B):
    """Tensor boundaries inside a bucket and not on a multiple of 4."""
    if n < 16:
        return [5, n - 5]
    cuts = [5, B // 2 + 1, B + 9, 1023]
    return cuts + [n - sum(cuts)]


def _cut(flat, sizes):
    out, off = [], 0
    for m in sizes:
        out.append(flat[off:off + m])
        off += m
    return out


def _seeded(n, seed, count):
    """``count`` flat vectors of n elements one element into a buffer (no tensor 16-B aligned but by accident)."""
    span = (n + 1 + 3) // 4 * 4
    base = torch.cat([_dev(dc.seed_acc(span, seed + k)) for k in range(count)])
    return base, [base[k * span + 1:k * span + 1 + n] for k in range(count)]


def _ptrs(ts):
    return (P * len(ts))(*[t.data_ptr() for t in ts])


def _floats(v):
    return (ctypes.c_float * len(v))(*v)


@pytest.mark.parametrize("B", bc.ALL_B)
@pytest.mark.parametrize("R", FOLD_R)
def test_fold_bucket_wires_and_groups_against_the_ordered_chain(R, B):
    lib = _lib()
    for n in _fold_sizes(B):
        (kind, s, bits), block, slots, weights, values = _fold_round(B, R, n)
        wires = _dev(block)
        for accumulate in (0, 1):
            acc0 = dc.seed_acc(n, 3 * n + R)
            view = _View(n, acc0)  # (accumulate 0: the stored values are not read)
            lib.call("flc_fold_bucket_wires", wires.data_ptr(), wires.shape[1], (ctypes.c_int32 * R)(*slots),
                     _floats(weights), R, n, kind, s, bits, B, accumulate, view.out.data_ptr(), None)
            torch.cuda.synchronize()
            want = bc.fold_chain(values, weights, acc0 if accumulate else np.zeros(n, dtype=F32))
            assert gc.same_bits(view.result((B, R, n)), want), (B, R, n, kind, s, bits, "wires", accumulate)
        assert torch.equal(wires.cpu(), torch.from_numpy(block))
        # the grouped fold: groups 0 and 2 share the records in turn, group 1 stays idle
        G, sizes = 3, _tensor_sizes(n, B)
        T = len(sizes)
        gof = [0 if c % 3 else 2 for c in range(R)]
        base, flats = _seeded(n, 7 * n + R, G)
        start = [f.cpu().numpy() for f in flats]
        dptr = [t.data_ptr() for g in range(G) for t in _cut(flats[g], sizes)]
        lib.call("flc_fold_bucket_record_groups", (P * R)(*[wires[sl].data_ptr() for sl in slots]), _floats(weights),
                 (ctypes.c_int32 * R)(*gof), R, n, kind, s, bits, B, (P * (G * T))(*dptr), G,
                 (ctypes.c_int64 * T)(*sizes), T, None)
        torch.cuda.synchronize()
        fresh, _ = _seeded(n, 7 * n + R, G)
        want_base = fresh.cpu().numpy()
        span = len(want_base) // G
        for g in range(G):
            mem = [c for c in range(R) if gof[c] == g]
            want_base[g * span + 1:g * span + 1 + n] = bc.fold_chain([values[c] for c in mem],
                                                                     [weights[c] for c in mem], start[g])
        assert gc.same_bits(base.cpu().numpy(), want_base), (B, R, n, kind, s, bits, "groups")


@pytest.mark.parametrize("B", bc.ALL_B)
@pytest.mark.parametrize("R", FOLD_R)
def test_fedopt_and_gradient_folds_against_decode_then_dense(R, B):
    """flc_fedopt_fold_bucket_records (avg and adam) against flc_model_fold, flc_avg_and_gradient_bucket_records
    against flc_avg_and_gradients, both on the modelled decodes of the same records."""
    lib, codec = _lib(), _codec()
    for n in _fold_sizes(B):
        (kind, s, bits), block, slots, weights, values = _fold_round(B, R, n)
        wires = _dev(block)
        rptr = (P * R)(*[wires[sl].data_ptr() for sl in slots])
        sizes = _tensor_sizes(n, B)
        T = len(sizes)
        sz = (ctypes.c_int64 * T)(*sizes)
        dec = [_dev(v) for v in values]
        for opt, beta0, lr, beta2, tau in (("avg", 0.0, 1.0, 1.0, 1.0), ("adam", 0.9, 0.01, 0.99, 1e-3)):
            res = []
            for fused in (True, False):
                base, (theta, delta, v) = _seeded(n, 11 * n + R, 3)
                v.abs_().add_(1e-6)
                th, dl, vv = _cut(theta, sizes), _cut(delta, sizes), _cut(v, sizes)
                if fused:
                    lib.call("flc_fedopt_fold_bucket_records", rptr, _floats(weights), R, n, kind, s, bits, B,
                             _ptrs(dl), _ptrs(th), _ptrs(vv) if opt != "avg" else None, sz, T, beta0,
                             lib.FLC_OPT[opt], lr, beta2, tau, None)
                else:
                    codec.model_fold(dl, [_cut(d, sizes) for d in dec], weights, 0, beta0, theta=th,
                                     v=vv if opt != "avg" else None, opt=opt, lr=lr, beta2=beta2, tau=tau)
                torch.cuda.synchronize()
                res.append(base.cpu().numpy())
            assert gc.same_bits(res[0], res[1]), (B, R, n, kind, s, bits, "fedopt", opt)
        res = []
        wp = [FOLD_WEIGHTS[(c + 2) % len(FOLD_WEIGHTS)] for c in range(R)]
        g = torch.Generator(device="cuda").manual_seed(n + R)
        psrc_flat = [torch.randn(n + 1, generator=g, device="cuda")[1:] for _ in range(R)]
        psrc = _ptrs([t for f in psrc_flat for t in _cut(f, sizes)])
        for fused in (True, False):
            base, (params, grads) = _seeded(n, 13 * n + R, 2)
            pt, gt = _cut(params, sizes), _cut(grads, sizes)
            if fused:
                lib.call("flc_avg_and_gradient_bucket_records", _ptrs(pt), _ptrs(gt), psrc, rptr, _floats(wp),
                         _floats(weights), R, n, kind, s, bits, B, sz, T, 0.25, None)
            else:
                gsrc = _ptrs([t for d in dec for t in _cut(d, sizes)])
                lib.call("flc_avg_and_gradients", _ptrs(pt), _ptrs(gt), psrc, gsrc, _floats(wp), _floats(weights), R,
                         sz, T, 0.25, None)
            torch.cuda.synchronize()
            res.append(base.cpu().numpy())
        assert gc.same_bits(res[0], res[1]), (B, R, n, kind, s, bits, "avg_and_gradient")
        span = len(res[0]) // 2  # the gradients are the ordered chain from +0 of the modelled decodes
        assert gc.same_bits(res[0][span + 1:span + 1 + n], bc.fold_chain(values, weights, np.zeros(n, dtype=F32)))


def test_bucket_folds_refuse_what_the_header_lists():
    lib = _lib()
    n, B = 5000, 256
    (kind, s, bits) = (STD, 7, 4)
    rec, _, _, _ = bc.handbuilt_record(kind, s, bits, B, n, 1)
    wires = _dev(rec).reshape(1, -1)
    out = torch.ones(n, device="cuda")
    one, slot = _floats([1.0]), (ctypes.c_int32 * 1)(0)
    sz = (ctypes.c_int64 * 1)(n)
    calls = {
        "flc_fold_bucket_wires": lambda f, b: (wires.data_ptr(), wires.shape[1], slot, one, 1, n, f, s, bits, b, 1,
                                               out.data_ptr(), None),
        "flc_fedopt_fold_bucket_records": lambda f, b: (_ptrs([wires]), one, 1, n, f, s, bits, b, _ptrs([out]), None,
                                                        None, sz, 1, 0.0, 0, 1.0, 0.0, 0.0, None),
        "flc_avg_and_gradient_bucket_records": lambda f, b: (None, _ptrs([out]), None, _ptrs([wires]), None, one, 1, n,
                                                             f, s, bits, b, sz, 1, 0.0, None),
        "flc_fold_bucket_record_groups": lambda f, b: (_ptrs([wires]), one, slot, 1, n, f, s, bits, b, _ptrs([out]), 1,
                                                       sz, 1, None),
    }
    for name, args in calls.items():
        for bad in (0, 32, 96, 8192, -64):
            with pytest.raises(lib.FlcError, match="bucket"):
                lib.call(name, *args(kind, bad))
        with pytest.raises(lib.FlcError, match="format"):
            lib.call(name, *args(lib.FLC_WIRE_NATURAL, B))
    torch.cuda.synchronize()
    assert bool((out == 1).all())  # (nothing launched)


# ------------------------------------------------------------------------------------------------ 5. the compressor
@pytest.mark.parametrize("B", [128, 256, 1024, 2048])
@pytest.mark.parametrize("kind,s,i", [(STD, 7, 3), (NAT, 4, 1)])
def test_compressor_with_a_bucket_on_the_decision_edges(kind, s, i, B):
    from fl_sim_amd import Compressor

    c = Compressor("q", rng="philox", seed=99, bucket=B)
    nc = None
    if kind == STD:
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(s, nc, p=np.inf)
    else:
        c.makeNaturalDitheringFP32(s, B, p=np.inf)
    seed, ctr = pickle.loads(pickle.dumps(c)).philox.next()
    tail, rot = bc.rotation(kind, B, i)
    x, norms, codes, out, nnz = bc.edge_message(kind, s, B, tail, rot, seed, ctr)
    got = c.compressVector(_dev(x)).cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint32) != out.view(np.uint32))
    assert bad.size == 0, (bad.size, [(int(j), float(x[j]), float(got[j]), float(out[j])) for j in bad[:5]])
    n, nb = len(x), len(norms)
    per = (1.0 + np.ceil(np.log2(s))) / 32.0
    assert c.last_input_advance == n == c.total_input_components
    assert c.really_need_to_send_components == (nb + nnz * per if kind == STD else n * per)
    if nc is not None:
        assert nc.total_input_components == nb == nc.really_need_to_send_components
