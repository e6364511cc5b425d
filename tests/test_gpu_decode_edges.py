"""The dense decoders — flc_sparse_decode[_tiled], flc_stacked_decode[_tiled], flc_quant_decode, flc_natural_decode,
flc_quant_decode_f64, flc_natural_decode_f64 and flc_tile_index — against the numpy model of tests/decode_cases.py
(anchored to the reference's arithmetic by tests/test_decode_cases.py) on hand-built, well-formed streams, bit for bit:
every tile occupancy from k = 0 to k = n, every valid code under regular and irregular norms, the listed weights,
scales and edge-valued accumulators, and the extent of every write (``out`` is a 16-B-aligned view inside a buffer of
sentinels).  Non-accumulating decodes write into NaN, so an element that is never written shows.  The tiled,
non-accumulating decode runs twice in a row: its tile order alternates from call to call, so one of the two calls ran
ascending and the other descending."""

import ctypes

import numpy as np
import pytest
import torch

from tests import decode_cases as dc
from tests import golden_cases as gc
from tests import golden_f64

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SENTINEL = 12345.0
GUARD = 64  # sentinel elements after the view (4 before it: the view stays 16-B aligned)
FLC_EINVAL, FLC_EWORKSPACE = 1, 3


def _call(name, *args):
    from fl_sim_amd import _lib

    _lib.call(name, *args)


def _st():
    from fl_sim_amd import codec

    return codec._stream(torch.device("cuda"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _View:
    """``out``: n elements at offset 16 B of a buffer filled with a finite sentinel, holding ``start`` (or NaN)."""

    def __init__(self, n, start=None, dtype=torch.float32):
        lead = 4 if dtype == torch.float32 else 2
        self.buf = torch.full((lead + n + GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.out = self.buf[lead:lead + n]
        assert self.out.data_ptr() % 16 == 0
        if start is None:
            self.out.fill_(float("nan"))
        else:
            self.out.copy_(torch.from_numpy(start))
        self.lead, self.n = lead, n

    def result(self, what):
        """The view's contents, after checking that both sides of it are unchanged."""
        host = self.buf.cpu().numpy()
        assert (host[:self.lead] == SENTINEL).all() and (host[self.lead + self.n:] == SENTINEL).all(), \
            f"a write outside out: {what}"
        return host[self.lead:self.lead + self.n]


class _Stream:
    """One index stream on the device with its tile pointers from flc_tile_index (checked against the model)."""

    def __init__(self, n, idx, label):
        self.n, self.k, self.label, self.idx = n, len(idx), label, idx
        self.d_idx = _dev(idx.astype(np.int32))
        ntiles = -(-n // dc.TILE)
        tbuf = torch.full((ntiles + 1 + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        _call("flc_tile_index", self.d_idx.data_ptr(), self.k, n, tbuf.data_ptr(), _st())
        host = tbuf.cpu().numpy()
        assert (host[ntiles + 1:] == 0x5A5A5A5A).all(), ("tile pointers written past ceil(n / TILE) + 1", n, label)
        assert np.array_equal(host[:ntiles + 1].view(np.uint32), dc.tile_pointers(idx, n)), (n, label)
        self.d_tiles = tbuf[:ntiles + 1]
        from fl_sim_amd import codec

        self.ws_bytes = codec._ws_size(torch.device("cuda"), "flc_sparse_decode_workspace_size", n)
        self.d_ws = torch.zeros(max(self.ws_bytes, 16), dtype=torch.uint8, device="cuda")

    def sparse(self, d_val, scale, weight, acc0, tiled):
        view = _View(self.n, acc0)
        if tiled:
            _call("flc_sparse_decode_tiled", self.d_idx.data_ptr(), d_val.data_ptr(), self.k, scale, self.n, weight,
                  int(acc0 is not None), view.out.data_ptr(), self.d_tiles.data_ptr(), _st())
        else:
            _call("flc_sparse_decode", self.d_idx.data_ptr(), d_val.data_ptr(), self.k, scale, self.n, weight,
                  int(acc0 is not None), view.out.data_ptr(), self.d_ws.data_ptr(), self.ws_bytes, _st())
        return view.result((self.n, self.label, "sparse", tiled))

    def stacked(self, d_codes, s, d_norm, weight, acc0, tiled):
        view = _View(self.n, acc0)
        if tiled:
            _call("flc_stacked_decode_tiled", self.d_idx.data_ptr(), d_codes.data_ptr(), self.k, s, d_norm.data_ptr(),
                  self.n, weight, int(acc0 is not None), view.out.data_ptr(), self.d_tiles.data_ptr(), _st())
        else:
            _call("flc_stacked_decode", self.d_idx.data_ptr(), d_codes.data_ptr(), self.k, s, d_norm.data_ptr(),
                  self.n, weight, int(acc0 is not None), view.out.data_ptr(), self.d_ws.data_ptr(), self.ws_bytes,
                  _st())
        return view.result((self.n, self.label, "stacked", tiled))


def _check_decodes(run, dense, weight, acc0, what, untiled_acc=True):
    """``run(weight, acc0 or None, tiled)`` against the output rule: the tiled plain decode twice in a row (both tile
    orders), the tiled accumulating one, and the untiled forms."""
    plain = dc.weighted(dense, weight, False)
    for call in (1, 2):
        assert gc.same_bits(run(weight, None, True), plain), (what, weight, "tiled", call)
    assert gc.same_bits(run(weight, None, False), plain), (what, weight, "untiled")
    acc = dc.weighted(dense, weight, True, acc0)
    assert gc.same_bits(run(weight, acc0, True), acc), (what, weight, "tiled, accumulate")
    if untiled_acc:
        assert gc.same_bits(run(weight, acc0, False), acc), (what, weight, "untiled, accumulate")


# --------------------------------------------------------------------------------------------------- sparse decode
@pytest.mark.parametrize("n", dc.SIZES)
def test_sparse_decode_on_every_occupancy(n):
    """Every (n, occupancy) stream at weight 1 with both scales and at weight -1.5."""
    acc0 = dc.seed_acc(n, 7 * n + 1)
    for i, (_, idx, label) in enumerate(dc.streams(n)):
        st = _Stream(n, idx, label)
        val = dc.sparse_values(st.k, i)
        d_val = _dev(val)
        for scale, weight in ((dc.SCALES[0], 1.0), (dc.SCALES[1], 1.0), (dc.SCALES[1], -1.5)):
            dense = dc.sparse_dense(n, idx, val, scale)
            _check_decodes(lambda w, a, t: st.sparse(d_val, scale, w, a, t), dense, weight, acc0, (n, label, scale))


@pytest.mark.parametrize("weight", dc.WEIGHTS, ids=[repr(w) for w in dc.WEIGHTS])
def test_sparse_decode_under_every_weight(weight):
    for n, want in ((4097, "p33"), (5 * 1024 + 3, "full"), (1026, "edges"), (3, "last")):
        idx = next(ix for _, ix, label in dc.streams(n) if label == want)
        st = _Stream(n, idx, want)
        val = dc.sparse_values(st.k, 5)
        d_val = _dev(val)
        acc0 = dc.seed_acc(n, n)
        for scale in dc.SCALES:
            dense = dc.sparse_dense(n, idx, val, scale)
            _check_decodes(lambda w, a, t: st.sparse(d_val, scale, w, a, t), dense, weight, acc0, (n, want, scale))


# -------------------------------------------------------------------------------------------------- stacked decode
def _norm_id(v):
    return repr(float(F32(v)))


@pytest.mark.parametrize("n", dc.SIZES)
def test_stacked_decode_on_every_occupancy(n):
    """Every (n, occupancy) stream under every norm of the list; the packet's levels and the weight (1 or 0.37) move
    with the stream and the norm."""
    acc0 = dc.seed_acc(n, 3 * n + 2)
    for i, (_, idx, label) in enumerate(dc.streams(n)):
        st = _Stream(n, idx, label)
        for j, norm in enumerate(dc.NORMS):
            s = dc.LEVELS[(i + j) % len(dc.LEVELS)]
            codes = dc.stacked_codes(st.k, s, start=i + 3 * j)
            d_codes, d_norm = _dev(codes), _dev(np.array([norm], dtype=F32))
            dense = dc.stacked_dense(n, idx, codes, s, norm)
            _check_decodes(lambda w, a, t: st.stacked(d_codes, s, d_norm, w, a, t), dense, 1.0 if j % 2 == 0 else 0.37,
                           acc0, (n, label, s, norm), untiled_acc=j % 4 == 1)


@pytest.mark.parametrize("s", dc.LEVELS)
def test_stacked_decode_of_every_code_under_every_norm_and_weight(s):
    """Both signs of every level 0..s (sign with level 0 and the top level among them) under each norm of the list,
    the weights taken in turn so that every (norm, weight) pair of the two lists is met over the eight packets."""
    for n, want in ((4097, "p33"), (2049, "full")):
        idx = next(ix for _, ix, label in dc.streams(n) if label == want)
        st = _Stream(n, idx, want)
        assert st.k >= 2 * (s + 1)
        codes = dc.stacked_codes(st.k, s, start=s)
        assert set(codes.tolist()) == set(dc.quant_codes(s, 8).tolist())
        d_codes = _dev(codes)
        acc0 = dc.seed_acc(n, s)
        for j, norm in enumerate(dc.NORMS):
            d_norm = _dev(np.array([norm], dtype=F32))
            dense = dc.stacked_dense(n, idx, codes, s, norm)
            for weight in (dc.WEIGHTS[(j + s) % 8], dc.WEIGHTS[(j + s + 3) % 8]):
                _check_decodes(lambda w, a, t: st.stacked(d_codes, s, d_norm, w, a, t), dense, weight, acc0,
                               (n, want, s, norm))


def test_stacked_decode_under_every_norm_times_every_weight():
    n, s = 3073, 107
    idx = next(ix for _, ix, label in dc.streams(n) if label == "p33")
    st = _Stream(n, idx, "p33")
    codes = dc.stacked_codes(st.k, s)
    d_codes = _dev(codes)
    acc0 = dc.seed_acc(n, 9)
    for norm in dc.NORMS:
        d_norm = _dev(np.array([norm], dtype=F32))
        dense = dc.stacked_dense(n, idx, codes, s, norm)
        for weight in dc.WEIGHTS:
            _check_decodes(lambda w, a, t: st.stacked(d_codes, s, d_norm, w, a, t), dense, weight, acc0, (norm, weight),
                           untiled_acc=False)


@pytest.mark.parametrize("k", [1, 5, 15])
def test_stacked_decode_reads_a_packed_wire_record_filled_by_hand(k):
    """k < 16: the record's codes field is 16 bytes, of which the decode may use the first k only (the rest hold 0xAB,
    no valid code of a 49-level packet)."""
    from fl_sim_amd import codec

    n, s = 4097, 49
    idx = np.sort(np.random.default_rng(k).choice(n, size=k, replace=False)).astype(np.int64)
    idx[-1] = n - 1
    stride, _ = codec.stacked_wire_layout(n, k)
    record = torch.full((stride,), 0xAB, dtype=torch.uint8, device="cuda")
    pkt = codec.wire_packet(record, n, k, s)
    assert pkt.codes.numel() == 16 and pkt.idx.numel() == k
    codes = dc.stacked_codes(k, s, start=s)  # (s, 128 | 0, 128 | 1, ..: the top level, then sign with level 0)
    pkt.idx.copy_(_dev(idx.astype(np.int32)))
    pkt.codes[:k].copy_(_dev(codes))
    pkt.norm.copy_(_dev(np.array([2.3e-3], dtype=F32)))
    _call("flc_tile_index", pkt.idx.data_ptr(), k, n, pkt.tiles.data_ptr(), _st())
    assert np.array_equal(pkt.tiles.cpu().numpy().view(np.uint32), dc.tile_pointers(idx, n))
    dense = dc.stacked_dense(n, idx, codes, s, 2.3e-3)
    acc0 = dc.seed_acc(n, k)
    for weight in (1.0, -1.5):
        for call in (1, 2):
            view = _View(n)
            codec.stacked_decode(pkt, out=view.out, weight=weight)
            assert gc.same_bits(view.result("record"), dc.weighted(dense, weight, False)), (weight, call)
        view = _View(n, acc0)
        codec.stacked_decode(pkt, out=view.out, weight=weight, accumulate=True)
        assert gc.same_bits(view.result("record"), dc.weighted(dense, weight, True, acc0)), weight


# ---------------------------------------------------------------------------------------------- the large stream
def test_the_large_stream_fills_every_tile():
    """n = 2^20 + 5 with k = n: flc_tile_index strides its grid (k + 1 > 2048 x 256 threads), every tile is full."""
    n, idx, label = dc.large_stream()
    st = _Stream(n, idx, label)
    acc0 = dc.seed_acc(n, 1)
    val = dc.sparse_values(n, 2)
    d_val = _dev(val)
    dense = dc.sparse_dense(n, idx, val, dc.SCALES[1])
    _check_decodes(lambda w, a, t: st.sparse(d_val, dc.SCALES[1], w, a, t), dense, 0.37, acc0, "sparse")
    s = 103
    codes = dc.stacked_codes(n, s)
    d_codes = _dev(codes)
    for norm, weight in ((2.3e-3, 1.0), (float("nan"), -1.5)):
        d_norm = _dev(np.array([norm], dtype=F32))
        dense = dc.stacked_dense(n, idx, codes, s, norm)
        _check_decodes(lambda w, a, t: st.stacked(d_codes, s, d_norm, w, a, t), dense, weight, acc0, ("stacked", norm),
                       untiled_acc=False)


# ------------------------------------------------------------------------------------------------ flc_quant_decode
QUANT_SHAPES = [(1, 1), (1, 7), (1, 8), (1, 9), (1, 70_001), (3, 5), (5, 3), (7, 1), (4, 1023), (3, 4097)]
QUANT_LEVELS = {2: [1], 4: list(range(1, 8)), 8: dc.LEVELS}


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("kind", [dc.STD, dc.NAT], ids=["standard", "natural"])
def test_quant_decode_of_every_code_on_every_shape(kind, bits):
    """Every valid code cycled over the flat batch (rows begin mid-byte at bits 2 and 4 when d * bits % 8 != 0, and
    rows shorter than 8 share a group), per-row norms from the list (regular and irregular rows alternate), with and
    without row weights, plain and accumulating; the code buffer holds exactly ceil(rows * d * bits / 8) bytes."""
    for s in QUANT_LEVELS[bits]:
        table = dc.quant_codes(s, bits)
        for si, (rows, d) in enumerate(QUANT_SHAPES):
            n = rows * d
            codes = dc.cycled(table, n, start=s + si).reshape(rows, d)
            if n >= len(table):
                assert set(codes.reshape(-1).tolist()) == set(table.tolist())
            norms = np.array([dc.NORMS[(r + s + si) % 8] for r in range(rows)], dtype=F32)
            row_w = np.array([dc.WEIGHTS[(r + 3 * s + si) % 8] for r in range(rows)], dtype=F32)
            packed = dc.pack(codes, bits)
            assert len(packed) == -(-n * bits // 8)
            d_codes, d_norms, d_w = _dev(packed), _dev(norms), _dev(row_w)
            assert d_codes.numel() == len(packed)
            v = dc.quant_values(codes, kind, s, bits, norms.reshape(-1, 1))
            acc0 = dc.seed_acc(n, n + s).reshape(rows, d)
            for w_host, w_dev in ((None, None), (row_w, d_w)):
                for a0 in (None, acc0):
                    view = _View(n, None if a0 is None else a0.reshape(-1))
                    _call("flc_quant_decode", d_codes.data_ptr(), rows, d, kind, s, bits, d_norms.data_ptr(),
                          None if w_dev is None else w_dev.data_ptr(), int(a0 is not None), view.out.data_ptr(), _st())
                    want = dc.row_weighted(v, w_host, a0 is not None, a0).reshape(-1)
                    assert gc.same_bits(view.result((kind, bits, s, rows, d)), want), \
                        (kind, bits, s, rows, d, w_host is not None, a0 is not None)


# ---------------------------------------------------------------------------------------------- flc_natural_decode
@pytest.mark.parametrize("n", [1, 7, 8, 9, 4097, 70_001])
def test_natural_decode_of_every_code(n):
    table = dc.natural_codes()
    starts = [0] if n >= len(table) else list(range(0, len(table), n))  # (a short vector walks the table)
    acc0 = dc.seed_acc(n, n + 5)
    for start in starts:
        codes = dc.cycled(table, n, start)
        d_codes = _dev(codes.view(np.int16))
        dense = dc.natural_values(codes)
        weights = dc.WEIGHTS if start == 0 else [1.0]
        for weight in weights:
            for a0 in (None, acc0) if start == 0 else (None,):
                view = _View(n, a0)
                _call("flc_natural_decode", d_codes.data_ptr(), n, weight, int(a0 is not None), view.out.data_ptr(),
                      _st())
                want = dc.weighted(dense, weight, a0 is not None, a0)
                assert gc.same_bits(view.result(("natural", n)), want), (n, start, weight, a0 is not None)


# -------------------------------------------------------------------------------------------------- float64 forms
@pytest.mark.parametrize("n", [1, 5, 4097])
def test_natural_decode_f64_of_every_code(n):
    table = dc.natural_codes(dc.NAT_FIELDS64)
    for start in range(0, len(table), n if n > 5 else 419):
        codes = dc.cycled(table, n, start)
        d_codes = _dev(codes.view(np.int16))
        view = _View(n, dtype=torch.float64)
        _call("flc_natural_decode_f64", d_codes.data_ptr(), n, view.out.data_ptr(), _st())
        assert golden_f64.same_bits(view.result(("natural64", n)), dc.natural_values64(codes)), (n, start)


@pytest.mark.parametrize("kind", [dc.STD, dc.NAT], ids=["standard", "natural"])
def test_quant_decode_f64_of_every_code_and_level_count(kind):
    """Every s in 1..127 and every valid code: the top level is pinned to 1 where s * (1 / s) != 1 in fp64 (s = 49,
    98, 103, 107), the other levels are i * (1 / s), not i / s.  Every (s, n, norm) that differs is reported."""
    bad = []
    for s in range(1, 128):
        table = dc.quant_codes(s, 8)
        for n in (1, 5, 4097):
            norms = dc.NORMS64 if n == 4097 else [dc.NORMS64[(s + n) % 8], dc.NORMS64[3]]
            for j, norm in enumerate(norms):
                codes = dc.cycled(table, n, start=s + j if n == 4097 else s - 1 + j * (s + 1))
                d_codes, d_norm = _dev(codes), _dev(np.array([norm], dtype=F64))
                view = _View(n, dtype=torch.float64)
                _call("flc_quant_decode_f64", d_codes.data_ptr(), n, kind, s, d_norm.data_ptr(), view.out.data_ptr(),
                      _st())
                want = dc.quant_values64(codes, kind, s, norm)
                if not golden_f64.same_bits(view.result(("quant64", s, n)), want):
                    bad.append((s, n, norm))
    assert not bad, (f"levels that differ: {sorted({b[0] for b in bad})}", bad)


# ------------------------------------------------------------------------------------------------------ refusals
def test_decoders_refuse_before_they_launch():
    """Host-side checks (nothing is launched: the pointers are never dereferenced)."""
    from fl_sim_amd import _lib

    lib = _lib.load()
    err = lambda: lib.flc_last_error().decode()  # noqa: E731
    A, B, C, T, W = 4096, 8192, 12288, 16384, 20480  # (16-B aligned, non-null)
    n, k = 4097, 3
    need = _lib.size("flc_sparse_decode_workspace_size", n)
    assert need >= (-(-n // dc.TILE) + 1) * 4
    exact = (-(-n // dc.TILE) + 1) * 4  # (what the decode itself asks of a workspace)
    # an out that is not 16-B aligned
    assert lib.flc_sparse_decode(A, B, k, 1.0, n, 1.0, 0, C + 4, W, need, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_sparse_decode(A, B, k, 1.0, n, 1.0, 1, C + 8, W, need, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_sparse_decode_tiled(A, B, k, 1.0, n, 1.0, 0, C + 4, T, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_stacked_decode(A, B, k, 127, C, n, 1.0, 0, T + 12, W, need, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_stacked_decode_tiled(A, B, k, 127, C, n, 1.0, 1, T + 4, W, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_quant_decode(A, 1, n, 0, 127, 8, B, None, 0, C + 4, None) == FLC_EINVAL and "aligned" in err()
    assert lib.flc_natural_decode(A, n, 1.0, 0, C + 4, None) == FLC_EINVAL and "aligned" in err()
    # levels outside [1, 127], levels that do not fit the bits
    for levels in (0, -1, 128, 255):
        assert lib.flc_stacked_decode(A, B, k, levels, C, n, 1.0, 0, T, W, need, None) == FLC_EINVAL and "levels" in err()
        assert lib.flc_stacked_decode_tiled(A, B, k, levels, C, n, 1.0, 0, T, W, None) == FLC_EINVAL and "levels" in err()
        assert lib.flc_quant_decode(A, 1, n, 0, levels, 8, B, None, 0, C, None) == FLC_EINVAL and "levels" in err()
        assert lib.flc_quant_decode_f64(A, n, 0, levels, B, C, None) == FLC_EINVAL and "levels" in err()
    for levels, bits in ((2, 2), (8, 4), (127, 4), (1, 3), (1, 16)):
        assert lib.flc_quant_decode(A, 1, n, 1, levels, bits, B, None, 0, C, None) == FLC_EINVAL
        assert "levels" in err() or "bits" in err()
    # a decode workspace one byte short
    for acc in (0, 1):
        assert lib.flc_sparse_decode(A, B, k, 1.0, n, 1.0, acc, C, W, exact - 1, None) == FLC_EWORKSPACE
        assert "workspace" in err()
        assert lib.flc_stacked_decode(A, B, k, 127, C, n, 1.0, acc, T, W, exact - 1, None) == FLC_EWORKSPACE
        assert lib.flc_sparse_decode(A, B, k, 1.0, n, 1.0, acc, C, None, need, None) == FLC_EWORKSPACE
    # n >= 2^31
    big = ctypes.c_int64(1 << 31)
    assert lib.flc_tile_index(A, k, big, T, None) == FLC_EINVAL and "2^31" in err()
    assert lib.flc_sparse_decode(A, B, k, 1.0, big, 1.0, 0, C, W, 1 << 40, None) == FLC_EINVAL and "2^31" in err()
    assert lib.flc_sparse_decode_tiled(A, B, k, 1.0, big, 1.0, 0, C, T, None) == FLC_EINVAL and "2^31" in err()
    assert lib.flc_stacked_decode(A, B, k, 127, C, big, 1.0, 0, T, W, 1 << 40, None) == FLC_EINVAL and "2^31" in err()
    assert lib.flc_stacked_decode_tiled(A, B, k, 127, C, big, 1.0, 0, T, W, None) == FLC_EINVAL and "2^31" in err()
