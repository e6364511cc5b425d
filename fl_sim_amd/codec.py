"""Device-side functional API over the C ABI: torch tensors in HBM in, torch tensors out.

Every function here launches hand-written gfx950 kernels from ``libflcodec.so`` on the current HIP
stream of the tensor's device; none of them synchronises the stream.  Tensors must be fp32, on a HIP
device and contiguous (non-contiguous or misaligned inputs are copied once).  This module is the
plumbing under :class:`fl_sim_amd.compressors.Compressor` and :mod:`fl_sim_amd.aggregation`; bench.py
drives it directly for the device-resident measurement.
"""

from __future__ import annotations

import collections.abc as _abc
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import call

_WS: Dict[Tuple[int, int, str], torch.Tensor] = {}


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(device: torch.device) -> int:
    """The raw handle of ``device``'s current stream (torch's C accessor when present: building a Stream object per
    call cost a few microseconds of host time on every launch of the small configs)."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(device.index if device.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(device).cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev_f32(x: torch.Tensor, name: str = "x") -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise TypeError(f"{name} must be a torch tensor on a HIP device (got {type(x).__name__}"
                        f"{'' if not isinstance(x, torch.Tensor) else ' on ' + str(x.device)})")
    if x.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {x.dtype}); the codec path is fp32")
    if not x.is_contiguous() or x.data_ptr() % 16 != 0:
        x = x.contiguous().clone()
    return x


TILE = 1024  # FLC_TILE (include/flcodec.h)


_WS_SIZE: Dict[tuple, int] = {}


def _ws_size(device: torch.device, name: str, *args) -> int:
    """A workspace-size entry point's result for ``device`` (the size functions read the current device's CU count,
    so the query runs with ``device`` current), memoised per device: one ctypes call fewer per encode."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, name) + args
    v = _WS_SIZE.get(key)
    if v is None:
        with torch.cuda.device(idx):
            v = _WS_SIZE[key] = _lib.size(name, *args)
    return v


def workspace(device: torch.device, nbytes: int, kind: str) -> torch.Tensor:
    """Zero-initialised workspace, cached per (device, stream, kind) and grown on demand."""
    key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device), kind)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(max(int(nbytes), 256), dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


def code_bits(levels: int) -> int:
    """Bits per element of the dithering wire: sign + ceil(log2(levels + 1)), rounded up to 2/4/8."""
    b = 1 + int(math.ceil(math.log2(levels + 1)))
    for c in (2, 4, 8):
        if b <= c:
            return c
    raise ValueError(f"levels={levels} does not fit an 8-bit code (at most 127 levels)")


# ----------------------------------------------------------------------------------------------- dither
@dataclass
class QuantPacket:
    """Wire of the dense dithering codec: per-row fp32 norm + packed ``bits``-bit codes."""

    codes: torch.Tensor
    norms: torch.Tensor
    rows: int
    d: int
    kind: int
    levels: int
    bits: int
    nnz: Optional[torch.Tensor] = None

    @property
    def nbytes(self) -> int:
        return self.codes.numel() + 4 * self.rows


def quant_norm(x2d: torch.Tensor, p: float = math.inf) -> torch.Tensor:
    x2d = _dev_f32(x2d)
    rows, d = x2d.shape
    pk = _lib.FLC_NORM_INF if math.isinf(p) else (_lib.FLC_NORM_L2 if p == 2 else None)
    if pk is None:
        raise ValueError(f"p must be inf or 2 (got {p})")
    norms = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    nb = _ws_size(x2d.device, "flc_quant_workspace_size", rows, d)
    ws = workspace(x2d.device, nb, "quant")
    call("flc_quant_norm", _p(x2d), rows, d, pk, _p(norms), _p(ws), ws.numel(), _stream(x2d.device))
    return norms


def count_consumers(x2d: torch.Tensor, norms: Optional[torch.Tensor]) -> torch.Tensor:
    """Device int64 scalar: the number of uniforms the reference draws for this batch."""
    x2d = _dev_f32(x2d)
    rows, d = x2d.shape
    out = torch.empty(1, dtype=torch.int64, device=x2d.device)
    call("flc_count_consumers", _p(x2d), rows, d, _p(norms), _p(out), _stream(x2d.device))
    return out


def quant_encode(x2d: torch.Tensor, kind: int, levels: int, norms: torch.Tensor, seed: int = 0, counter: int = 0,
                 compat_u: Optional[torch.Tensor] = None, want_nnz: bool = True) -> QuantPacket:
    x2d = _dev_f32(x2d)
    rows, d = x2d.shape
    bits = code_bits(levels)
    nbytes = (rows * d * bits + 7) // 8
    codes = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=x2d.device)
    nnz = torch.empty(rows, dtype=torch.int64, device=x2d.device) if want_nnz else None
    if compat_u is not None and compat_u.dtype != torch.float64:
        raise TypeError("compat_u must be float64")
    nb = _ws_size(x2d.device, "flc_quant_workspace_size", rows, d)
    ws = workspace(x2d.device, nb, "quant")
    call("flc_quant_encode", _p(x2d), rows, d, kind, levels, bits, _p(norms), seed, counter, _p(compat_u),
         _p(codes), _p(nnz), _p(ws), ws.numel(), _stream(x2d.device))
    return QuantPacket(codes, norms, rows, d, kind, levels, bits, nnz)


def quant_encode_decode(x2d: torch.Tensor, kind: int, levels: int, norms: torch.Tensor, seed: int = 0,
                        counter: int = 0, compat_u: Optional[torch.Tensor] = None, want_nnz: bool = True,
                        out: Optional[torch.Tensor] = None) -> Tuple[QuantPacket, torch.Tensor]:
    """quant_encode and quant_decode in one pass (flc_quant_encode_decode): the same codes, and the decoded batch
    computed from each code as it is made.  Returns (packet, decoded [rows, d])."""
    x2d = _dev_f32(x2d)
    rows, d = x2d.shape
    bits = code_bits(levels)
    codes = torch.empty(max((rows * d * bits + 7) // 8, 1), dtype=torch.uint8, device=x2d.device)
    nnz = torch.empty(rows, dtype=torch.int64, device=x2d.device) if want_nnz else None
    if out is None:
        out = torch.empty(rows, d, dtype=torch.float32, device=x2d.device)
    if compat_u is not None and compat_u.dtype != torch.float64:
        raise TypeError("compat_u must be float64")
    ws = workspace(x2d.device, _ws_size(x2d.device, "flc_quant_workspace_size", rows, d), "quant")
    call("flc_quant_encode_decode", _p(x2d), rows, d, kind, levels, bits, _p(norms), seed, counter, _p(compat_u),
         _p(codes), _p(nnz), _p(out), _p(ws), ws.numel(), _stream(x2d.device))
    return QuantPacket(codes, norms, rows, d, kind, levels, bits, nnz), out


def quant_encode_auto(x2d: torch.Tensor, kind: int, levels: int, p: float = math.inf, seed: int = 0, counter: int = 0,
                      want_nnz: bool = False, decode: bool = True):
    """Philox mode with the norm included (flc_quant_encode_auto): norm, encode and (``decode``) the decoded batch in
    two launches for rows of >= 2048 elements.  Returns (packet, decoded or None)."""
    x2d = _dev_f32(x2d)
    rows, d = x2d.shape
    pk = _lib.FLC_NORM_INF if math.isinf(p) else (_lib.FLC_NORM_L2 if p == 2 else None)
    if pk is None:
        raise ValueError(f"p must be inf or 2 (got {p})")
    bits = code_bits(levels)
    codes = torch.empty(max((rows * d * bits + 7) // 8, 1), dtype=torch.uint8, device=x2d.device)
    norms = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    nnz = torch.empty(rows, dtype=torch.int64, device=x2d.device) if want_nnz else None
    out = torch.empty(rows, d, dtype=torch.float32, device=x2d.device) if decode else None
    ws = workspace(x2d.device, _ws_size(x2d.device, "flc_quant_workspace_size", rows, d), "quant")
    call("flc_quant_encode_auto", _p(x2d), rows, d, kind, levels, bits, pk, seed, counter, _p(codes), _p(norms),
         _p(nnz), _p(out), _p(ws), ws.numel(), _stream(x2d.device))
    _after_encode(x2d.device, ("quant",))
    return QuantPacket(codes, norms, rows, d, kind, levels, bits, nnz), out


def quant_decode(pkt: QuantPacket, out: Optional[torch.Tensor] = None, row_weights: Optional[torch.Tensor] = None,
                 accumulate: bool = False) -> torch.Tensor:
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an out tensor")
        out = torch.empty(pkt.rows, pkt.d, dtype=torch.float32, device=pkt.codes.device)
    call("flc_quant_decode", _p(pkt.codes), pkt.rows, pkt.d, pkt.kind, pkt.levels, pkt.bits, _p(pkt.norms),
         _p(row_weights), int(accumulate), _p(out), _stream(out.device))
    return out


# ---------------------------------------------------------------------------------------------- natural
def natural_encode(x: torch.Tensor, seed: int = 0, counter: int = 0, compat_u: Optional[torch.Tensor] = None,
                   want_nnz: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    x = _dev_f32(x).reshape(-1)
    n = x.numel()
    codes = torch.empty(n, dtype=torch.int16, device=x.device)
    nnz = torch.empty(1, dtype=torch.int64, device=x.device) if want_nnz else None
    nb = _ws_size(x.device, "flc_natural_workspace_size", n)
    ws = workspace(x.device, nb, "natural")
    call("flc_natural_encode", _p(x), n, seed, counter, _p(compat_u), _p(codes), _p(nnz), _p(ws), ws.numel(),
         _stream(x.device))
    return codes, nnz


def natural_decode(codes: torch.Tensor, n: int, out: Optional[torch.Tensor] = None, weight: float = 1.0,
                   accumulate: bool = False) -> torch.Tensor:
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=codes.device)
    call("flc_natural_decode", _p(codes), n, weight, int(accumulate), _p(out), _stream(out.device))
    return out


# ---------------------------------------------------------------------------------------- dense records
_DENSE_LAYOUT: Dict[tuple, tuple] = {}


def dense_wire_layout(n: int, fmt: int, bits: int):
    """(record bytes, {"norm", "codes"} byte offsets) of a dense record (flc_dense_wire_layout): a dithering
    quantizer's norm and ``bits``-bit codes (``fmt`` FLC_Q_STANDARD_DITHER / FLC_Q_NATURAL_DITHER, bits 2, 4 or 8), or
    the natural compressor's uint16 codes (``fmt`` FLC_WIRE_NATURAL, bits 16), as one contiguous record."""
    import ctypes

    key = (int(n), int(fmt), int(bits))
    r = _DENSE_LAYOUT.get(key)
    if r is None:
        off = (ctypes.c_int64 * 2)()
        total = _lib.size("flc_dense_wire_layout", key[0], key[1], key[2], ctypes.cast(off, ctypes.c_void_p))
        if total == 0:
            raise ValueError(f"bad dense record shape n={n}, format={fmt}, bits={bits}")
        r = _DENSE_LAYOUT[key] = (int(total), {"norm": int(off[0]), "codes": int(off[1])})
    return r


def dense_wire_views(record: torch.Tensor, n: int, fmt: int, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(norm, codes) views into a dense record (a contiguous uint8 HIP tensor of at least
    ``dense_wire_layout(n, fmt, bits)[0]`` bytes, 16-B aligned): the fp32 norm and the uint8 code stream, or the
    natural compressor's int16 codes."""
    stride, off = dense_wire_layout(n, fmt, bits)
    if record.dtype != torch.uint8 or record.device.type != "cuda" or not record.is_contiguous():
        raise TypeError("a wire record is a contiguous uint8 HIP tensor")
    rec = record.reshape(-1)
    if rec.numel() < stride or rec.data_ptr() % 16 != 0:
        raise ValueError(f"a dense record needs {stride} bytes, 16-B aligned")
    norm = rec[off["norm"]:off["norm"] + 4].view(torch.float32)
    if fmt == _lib.FLC_WIRE_NATURAL:
        return norm, rec[off["codes"]:off["codes"] + 2 * n].view(torch.int16)
    return norm, rec[off["codes"]:off["codes"] + (n * bits + 7) // 8]


def dense_record_decode(record: torch.Tensor, n: int, fmt: int, levels: int, bits: int,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The decoded flat vector of a dense record (flc_quant_decode / flc_natural_decode on its views)."""
    norm, codes = dense_wire_views(record, n, fmt, bits)
    if fmt == _lib.FLC_WIRE_NATURAL:
        return natural_decode(codes, n, out=out)
    pkt = QuantPacket(codes, norm, 1, n, fmt, levels, bits)
    return quant_decode(pkt, out=None if out is None else out.reshape(1, n)).reshape(n)


def quant_encode_round(xs: Sequence[torch.Tensor], kind: int, levels: int, bits: int, norm_p: int,
                       seeds: Sequence[int], counters: Sequence[int], records, counts=None) -> None:
    """A round's dithering messages in one call (flc_quant_encode_round, philox mode, norm included): message c — the
    flat fp32 vector ``xs[c]``, all of one size on one device — is encoded with its own Philox
    ``(seeds[c], counters[c])`` into the dense record ``records[c]`` (its norm and codes views, dense_wire_views),
    bit-identical to ``flc_quant_encode_auto`` of that vector alone.  ``records``: a ``[C, >= stride]`` uint8 block
    or a sequence of C records; ``norm_p``: FLC_NORM_INF or FLC_NORM_L2; ``counts``: None, or one one-element device
    int64 tensor per message (a contiguous ``[C]`` tensor also) that receives the message's count of nonzero
    elements."""
    C = len(xs)
    if C == 0:
        return
    n, dev = xs[0].numel(), xs[0].device
    xp = _batch_ptrs(xs, n, dev) if dev.type == "cuda" else None
    if xp is None:  # (the slow path: checks with messages, copies of misaligned inputs)
        xs = [_dev_f32(x).reshape(-1) for x in xs]
        if any(x.numel() != n or x.device != dev for x in xs):
            raise ValueError("a round encode takes messages of one size on one device")
        xp = [x.data_ptr() for x in xs]
    _quant_round_call("flc_quant_encode_round", xp, n, dev, kind, levels, bits, norm_p, seeds, counters, records,
                      counts)


def quant_encode_residual_round(mems: Sequence[torch.Tensor], kind: int, levels: int, bits: int, norm_p: int,
                                seeds: Sequence[int], counters: Sequence[int], records, counts=None) -> None:
    """:func:`quant_encode_round` with error feedback in the encode's own pass (flc_quant_encode_residual_round):
    message c's input is the error memory ``mems[c]``, holding ``a``; the records, norms and counts are those of
    ``quant_encode_round(mems, ...)`` bit for bit, and each memory is left holding ``a − decode(records[c])`` — what
    ``dense_record_decode`` into a fresh vector and :func:`ef_residual_dense` leave — with no decode, no temporary and
    no further launch.  The memories are written in place, so nothing is copied for them: each must be a contiguous,
    16-B aligned float32 tensor of one size on one HIP device, and no two may share elements."""
    C = len(mems)
    if C == 0:
        return
    if not isinstance(mems[0], torch.Tensor) or mems[0].device.type != "cuda":
        raise TypeError("the memories must be float32 tensors on a HIP device")
    n, dev = mems[0].numel(), mems[0].device
    ep = _batch_ptrs(mems, n, dev)
    if ep is None:
        raise ValueError("the memories must be contiguous, 16-B aligned float32 tensors of one size on one device")
    _quant_round_call("flc_quant_encode_residual_round", ep, n, dev, kind, levels, bits, norm_p, seeds, counters,
                      records, counts)


def _quant_round_call(entry: str, xp: List[int], n: int, dev, kind: int, levels: int, bits: int, norm_p: int, seeds,
                      counters, records, counts) -> None:
    """The record views, tables and workspace of a round's quantizer encode, then the call (``entry``: the plain or
    the residual form; ``xp``: the messages' input pointers)."""
    import ctypes

    C = len(xp)
    if len(seeds) != C or len(counters) != C:
        raise ValueError("one seed and one counter per message")
    if isinstance(records, torch.Tensor) and records.dim() == 2:  # one record block: the rows' views by arithmetic
        stride, off = dense_wire_layout(n, kind, bits)
        if records.shape[0] != C or records.shape[1] % 16 or records.device != dev:
            raise ValueError(f"records must be a [{C}, >= {stride}] uint8 block (16-B rows) on {dev}")
        dense_wire_views(records[0], n, kind, bits)  # (dtype, size and alignment, checked on one row for all)
        bases = [records.data_ptr() + c * records.shape[1] for c in range(C)]
        nps, cps = [b + off["norm"] for b in bases], [b + off["codes"] for b in bases]
    else:
        if len(records) != C:
            raise ValueError("one record per message")
        views = [dense_wire_views(r, n, kind, bits) for r in records]
        if any(r.device != dev for r in records):
            raise ValueError(f"the records must be on {dev}")
        nps, cps = [v[0].data_ptr() for v in views], [v[1].data_ptr() for v in views]
    ctr, cnt = _round_args(C, dev, 0, counters, counts)
    P = ctypes.c_void_p * C
    vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    ws = workspace(dev, _ws_size(dev, "flc_quant_encode_round_workspace_size", n, C), "quant_round")
    call(entry, vp(P(*xp)), C, n, kind, levels, bits, norm_p,
         vp((ctypes.c_uint64 * C)(*[int(s_) for s_ in seeds])), vp(ctr), vp(P(*cps)), vp(P(*nps)), vp(cnt), _p(ws),
         ws.numel(), _stream(dev))


def natural_encode_round(xs: Sequence[torch.Tensor], seeds: Sequence[int], counters: Sequence[int], records) -> None:
    """A round's natural-compressor messages in one call (flc_natural_encode_round, philox mode): message c — the flat
    fp32 vector ``xs[c]``, all of one size on one device — is encoded with its own Philox ``(seeds[c], counters[c])``
    into the codes view of the dense record ``records[c]`` (dense_wire_views with FLC_WIRE_NATURAL), bit-identical to
    ``flc_natural_encode`` of that vector alone.  ``records``: a ``[C, >= stride]`` uint8 block or a sequence of C
    records.  One launch per 64 messages, no workspace."""
    C = len(xs)
    if C == 0:
        return
    n, dev = xs[0].numel(), xs[0].device
    xp = _batch_ptrs(xs, n, dev) if dev.type == "cuda" else None
    if xp is None:  # (the slow path: checks with messages, copies of misaligned inputs)
        xs = [_dev_f32(x).reshape(-1) for x in xs]
        if any(x.numel() != n or x.device != dev for x in xs):
            raise ValueError("a round encode takes messages of one size on one device")
        xp = [x.data_ptr() for x in xs]
    _natural_round_call("flc_natural_encode_round", xp, n, dev, seeds, counters, records)


def natural_encode_residual_round(mems: Sequence[torch.Tensor], seeds: Sequence[int], counters: Sequence[int],
                                  records) -> None:
    """:func:`natural_encode_round` with error feedback in the encode's own pass (flc_natural_encode_residual_round):
    message c's input is the error memory ``mems[c]``, holding ``a``; the records are those of
    ``natural_encode_round(mems, ...)`` bit for bit, and each memory is left holding ``a − decode(records[c])`` — what
    ``dense_record_decode`` into a fresh vector and :func:`ef_residual_dense` leave — with no decode, no temporary and
    no further launch.  The memories are written in place, so nothing is copied for them: each must be a contiguous,
    16-B aligned float32 tensor of one size on one HIP device, and no two may share elements."""
    C = len(mems)
    if C == 0:
        return
    if not isinstance(mems[0], torch.Tensor) or mems[0].device.type != "cuda":
        raise TypeError("the memories must be float32 tensors on a HIP device")
    n, dev = mems[0].numel(), mems[0].device
    ep = _batch_ptrs(mems, n, dev)
    if ep is None:
        raise ValueError("the memories must be contiguous, 16-B aligned float32 tensors of one size on one device")
    _natural_round_call("flc_natural_encode_residual_round", ep, n, dev, seeds, counters, records)


def _natural_round_call(entry: str, xp: List[int], n: int, dev, seeds, counters, records) -> None:
    """The code views and tables of a round's natural-compressor encode, then the call (``entry``: the plain or the
    residual form; ``xp``: the messages' input pointers).  The record-view arithmetic of :func:`_quant_round_call`."""
    import ctypes

    C = len(xp)
    if len(seeds) != C or len(counters) != C:
        raise ValueError("one seed and one counter per message")
    fmt = _lib.FLC_WIRE_NATURAL
    if isinstance(records, torch.Tensor) and records.dim() == 2:  # one record block: the rows' views by arithmetic
        stride, off = dense_wire_layout(n, fmt, 16)
        if records.shape[0] != C or records.shape[1] % 16 or records.device != dev:
            raise ValueError(f"records must be a [{C}, >= {stride}] uint8 block (16-B rows) on {dev}")
        dense_wire_views(records[0], n, fmt, 16)  # (dtype, size and alignment, checked on one row for all)
        cps = [records.data_ptr() + c * records.shape[1] + off["codes"] for c in range(C)]
    else:
        if len(records) != C:
            raise ValueError("one record per message")
        views = [dense_wire_views(r, n, fmt, 16) for r in records]
        if any(r.device != dev for r in records):
            raise ValueError(f"the records must be on {dev}")
        cps = [v[1].data_ptr() for v in views]
    P = ctypes.c_void_p * C
    U = ctypes.c_uint64 * C
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    call(entry, vp(P(*xp)), C, n, vp(U(*[int(s_) for s_ in seeds])), vp(U(*[int(t) for t in counters])), vp(P(*cps)),
         _stream(dev))


# --------------------------------------------------------------------------------------- bucket records
BUCKET_SIZES = (64, 128, 256, 512, 1024, 2048, 4096)
_BUCKET_LAYOUT: Dict[tuple, tuple] = {}


def _norm_kind(p) -> int:
    if isinstance(p, int) and p in (_lib.FLC_NORM_INF, _lib.FLC_NORM_L2):
        return p
    if math.isinf(p):
        return _lib.FLC_NORM_INF
    if p == 2:
        return _lib.FLC_NORM_L2
    raise ValueError(f"p must be inf or 2 (got {p})")


def bucket_wire_layout(n: int, fmt: int, bits: int, bucket: int):
    """(record bytes, {"norms", "codes"} byte offsets) of a bucket record (flc_bucket_wire_layout): the
    ``ceil(n / bucket)`` fp32 norms of a bucketed dithering quantizer, then its ``bits``-bit codes."""
    import ctypes

    key = (int(n), int(fmt), int(bits), int(bucket))
    r = _BUCKET_LAYOUT.get(key)
    if r is None:
        off = (ctypes.c_int64 * 2)()
        total = _lib.size("flc_bucket_wire_layout", key[0], key[1], key[2], key[3], ctypes.cast(off, ctypes.c_void_p))
        if total == 0:
            raise ValueError(f"bad bucket record shape n={n}, format={fmt}, bits={bits}, bucket={bucket}")
        r = _BUCKET_LAYOUT[key] = (int(total), {"norms": int(off[0]), "codes": int(off[1])})
    return r


def bucket_wire_views(record: torch.Tensor, n: int, fmt: int, bits: int, bucket: int):
    """(norms, codes) views into a bucket record (a contiguous uint8 HIP tensor of at least
    ``bucket_wire_layout(...)[0]`` bytes, 16-B aligned): the per-bucket fp32 norms and the uint8 code stream."""
    stride, off = bucket_wire_layout(n, fmt, bits, bucket)
    if record.dtype != torch.uint8 or record.device.type != "cuda" or not record.is_contiguous():
        raise TypeError("a wire record is a contiguous uint8 HIP tensor")
    rec = record.reshape(-1)
    if rec.numel() < stride or rec.data_ptr() % 16 != 0:
        raise ValueError(f"a bucket record needs {stride} bytes, 16-B aligned")
    nb = (n + bucket - 1) // bucket
    return (rec[off["norms"]:off["norms"] + 4 * nb].view(torch.float32),
            rec[off["codes"]:off["codes"] + (n * bits + 7) // 8])


def bucket_encode(x: torch.Tensor, kind: int, levels: int, bucket: int, p=math.inf, seed: int = 0, counter: int = 0,
                  record: Optional[torch.Tensor] = None, norms: Optional[torch.Tensor] = None,
                  want_nnz: bool = False, decode: bool = False):
    """One message as a bucket record in one launch that reads ``x`` once (flc_bucket_encode, philox mode): the
    dithering quantizer applied to every ``bucket`` consecutive elements with that bucket's own norm.  ``norms``: given
    per-bucket norms (``ceil(n / bucket)`` floats) used instead of the device's.  Returns
    ``(record, nnz or None, decoded or None)``; ``record`` is allocated when not given."""
    x = _dev_f32(x).reshape(-1)
    n, dev = x.numel(), x.device
    bits = code_bits(levels)
    stride, _ = bucket_wire_layout(n, kind, bits, bucket)
    if record is None:
        record = torch.empty(stride, dtype=torch.uint8, device=dev)
    nv, cv = bucket_wire_views(record, n, kind, bits, bucket)
    if norms is not None:
        if norms.numel() != nv.numel():
            raise ValueError(f"{nv.numel()} bucket norms expected (got {norms.numel()})")
        nv.copy_(norms.reshape(-1).to(device=dev, dtype=torch.float32))
    nnz = torch.empty(1, dtype=torch.int64, device=dev) if want_nnz else None
    out = torch.empty(n, dtype=torch.float32, device=dev) if decode else None
    call("flc_bucket_encode", _p(x), n, kind, levels, bits, bucket, _norm_kind(p), int(norms is not None), seed,
         counter, _p(nv), _p(cv), _p(nnz), _p(out), _stream(dev))
    return record, nnz, out


def bucket_encode_round(xs: Sequence[torch.Tensor], kind: int, levels: int, bits: int, bucket: int, norm_p: int,
                        seeds: Sequence[int], counters: Sequence[int], records, counts=None,
                        norms_given: bool = False) -> None:
    """A round's messages as bucket records in one launch per 64 messages (flc_bucket_encode_round): message c — the
    flat fp32 vector ``xs[c]``, all of one size on one device — is encoded with its own Philox
    ``(seeds[c], counters[c])`` into ``records[c]``, bit-identical to :func:`bucket_encode` of that vector alone.
    ``records``: a ``[C, >= stride]`` uint8 block or a sequence of C records; ``counts``: None, or one one-element
    device int64 tensor per message (a contiguous ``[C]`` tensor also)."""
    import ctypes

    C = len(xs)
    if C == 0:
        return
    if len(seeds) != C or len(counters) != C:
        raise ValueError("one seed and one counter per message")
    xs = [_dev_f32(x).reshape(-1) for x in xs]
    n, dev = xs[0].numel(), xs[0].device
    if any(x.numel() != n or x.device != dev for x in xs):
        raise ValueError("a round encode takes messages of one size on one device")
    if len(records) != C:
        raise ValueError("one record per message")
    views = [bucket_wire_views(r, n, kind, bits, bucket) for r in records]
    if counts is not None and len(counts) != C:
        raise ValueError("one count slot per message")
    P, U = ctypes.c_void_p * C, ctypes.c_uint64 * C
    vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    cnt = None if counts is None else P(*[c.data_ptr() for c in counts])
    call("flc_bucket_encode_round", vp(P(*[x.data_ptr() for x in xs])), C, n, kind, levels, bits, bucket,
         _norm_kind(norm_p), int(norms_given), vp(U(*[int(s_) for s_ in seeds])), vp(U(*[int(t) for t in counters])),
         vp(P(*[v[0].data_ptr() for v in views])), vp(P(*[v[1].data_ptr() for v in views])), vp(cnt), _stream(dev))


def bucket_decode(record: torch.Tensor, n: int, kind: int, levels: int, bits: int, bucket: int,
                  out: Optional[torch.Tensor] = None, weight: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """The decoded flat vector of a bucket record (flc_bucket_decode): ``v = fp32(fp32(level) * sign) * norm[e // B]``;
    ``out = fmaf(weight, v, out)`` when accumulating, ``weight * v`` otherwise."""
    nv, cv = bucket_wire_views(record, n, kind, bits, bucket)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an out tensor")
        out = torch.empty(n, dtype=torch.float32, device=record.device)
    call("flc_bucket_decode", _p(cv), n, kind, levels, bits, bucket, _p(nv), float(weight), int(accumulate), _p(out),
         _stream(out.device))
    return out


def fold_dense_wires(wires: torch.Tensor, slots: Sequence[int], weights: Sequence[float], n: int, fmt: int,
                     levels: int, bits: int, out: Optional[torch.Tensor] = None,
                     accumulate: bool = False) -> torch.Tensor:
    """``out = (accumulate ? out : 0) + Σ_c weights[c] · decode(wires[slots[c]])`` in client order, one pass
    (flc_fold_dense_wires).  ``wires``: a [records, stride] uint8 HIP tensor of dense records."""
    import ctypes

    if wires.dtype != torch.uint8 or wires.dim() != 2 or not wires.is_contiguous() or wires.device.type != "cuda":
        raise TypeError("wires must be a contiguous [records, stride] uint8 HIP tensor")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an out tensor")
        out = torch.empty(n, dtype=torch.float32, device=wires.device)
    m = len(slots)
    call("flc_fold_dense_wires", _p(wires), wires.shape[1], (ctypes.c_int32 * m)(*[int(s) for s in slots]),
         (ctypes.c_float * m)(*[float(w) for w in weights]), m, n, fmt, levels, bits, int(accumulate), _p(out),
         _stream(wires.device))
    return out


# ------------------------------------------------------------------------------------------------ top-k
# FLC_TOPK_CHECK=1: read the persistent encoder's sticky error word after every top-k / stacked encode
# (one host synchronisation per call) and raise if a call lost co-residency (include/flcodec.h)
TOPK_CHECK = os.environ.get("FLC_TOPK_CHECK", "0") not in ("", "0")
TOPK_ERRORS = {1: "digit not found", 2: "count mismatch", 4: "exchange spin timeout"}
_TOPK_KINDS = ("topk", "topk_batch")  # single-client and batched encoder workspaces (never shared)
# every workspace kind whose kernels run a grid exchange, and the entry point reading its sticky error word
_STATUS_FN = {"topk": "flc_topk_status", "topk_batch": "flc_topk_status", "quant": "flc_quant_status",
              "f64": "flc_f64_status"}


def _status(device: torch.device, kinds: Sequence[str], reset: bool = True) -> int:
    err = 0
    for kind in kinds:
        key = (device.index if device.index is not None else torch.cuda.current_device(), _stream(device), kind)
        ws = _WS.get(key)
        if ws is None:
            continue
        out = torch.empty(1, dtype=torch.int64, device=device)
        call(_STATUS_FN[kind], _p(ws), _p(out), int(reset), _stream(device))
        err |= int(out.item())
    return err


def topk_status(device: Optional[torch.device] = None, reset: bool = True) -> int:
    """The sticky error word of the top-k workspace of ``device``'s current stream (0 = every encode since
    the last reset was exact).  Synchronises that stream."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return _status(device, _TOPK_KINDS, reset)


def quant_status(device: Optional[torch.device] = None, reset: bool = True) -> int:
    """The sticky error word of the one-launch quantizer's workspace (quant_fused_kernel's grid exchange) of
    ``device``'s current stream; 0 = every call since the last reset had all its blocks resident."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    return _status(device, ("quant",), reset)


def topk_status_all(reset: bool = True) -> Dict[Tuple[int, int], int]:
    """{(device, stream): error word} of every cached workspace whose kernels run a grid exchange (the top-k
    encoders, the one-launch quantizer).  Synchronises each device first and reads on its current stream (the stream
    a workspace was used on may be gone)."""
    res: Dict[Tuple[int, int], int] = {}
    for (dev, stream, kind), ws in list(_WS.items()):
        if kind not in _STATUS_FN:
            continue
        d = torch.device("cuda", dev)
        torch.cuda.synchronize(d)
        out = torch.empty(1, dtype=torch.int64, device=d)
        call(_STATUS_FN[kind], _p(ws), _p(out), int(reset), _stream(d))
        res[(dev, stream)] = res.get((dev, stream), 0) | int(out.item())
    return res


_PLAN_FIELDS = ("S", "rank_lo", "rank_hi", "take_all", "G", "M", "ovf", "list_cap", "compact", "cap", "list_all",
                "hist_bits", "fast_rank", "chunk", "cus")  # FLC_PLAN_* (include/flcodec.h)
_SEL_FIELDS = ("call", "err", "C", "fallback", "T", "maxkey", "rounds", "t_lo", "t_hi", "need", "ties", "strict",
               "sample_path")  # FLC_SEL_*


def topk_select_plan(n: int, k: int, clients: int = 0, cus: int = 0) -> dict:
    """The numbers the select will use for a call over ``n`` elements keeping ``k`` (flc_topk_select_plan): sample
    size and ranks, blocks and elements per block, overflow slots, list capacities.  ``clients`` = 0: the
    single-client encoders, >= 1: the batched ones.  ``cus`` = 0 reads the current device's CU count; with
    ``cus`` > 0 no device is touched."""
    import ctypes

    out = (ctypes.c_int64 * 16)()
    call("flc_topk_select_plan", int(n), int(k), int(clients), int(cus), out)
    return {f: int(out[i]) for i, f in enumerate(_PLAN_FIELDS)}


def topk_select_stats(device: Optional[torch.device] = None, kind: str = "topk", client: int = 0) -> dict:
    """What the last select on the cached ``kind`` workspace ("topk": the single-client encoders, "topk_batch": the
    batched ones, ``client`` its place in the launch) of ``device``'s current stream did (flc_topk_select_stats):
    ``sample_path`` (0 fast pick, 1 general pick, 2 take-all), the floor / ceiling keys ``t_lo`` / ``t_hi``, the
    candidates admitted ``C``, ``fallback``, histogram ``rounds``, the k-th largest key ``T``, ``need`` / ``ties`` /
    ``strict`` and ``maxkey``.  Synchronises the stream."""
    import ctypes

    if kind not in _TOPK_KINDS:
        raise ValueError(f"kind must be one of {_TOPK_KINDS}")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    ws = _WS.get((device.index if device.index is not None else torch.cuda.current_device(), _stream(device), kind))
    if ws is None:
        raise RuntimeError(f"no {kind!r} workspace on this device and stream yet: run an encode first")
    out = (ctypes.c_uint64 * 16)()
    call("flc_topk_select_stats", _p(ws), ws.numel(), int(client), out, _stream(device))
    return {f: int(out[i]) for i, f in enumerate(_SEL_FIELDS)}


def _after_encode(device: torch.device, kinds: Sequence[str] = _TOPK_KINDS) -> None:
    """FLC_TOPK_CHECK: read the sticky error word of the workspaces ``kinds`` (one host synchronisation) and raise
    if a grid-exchange launch lost co-residency; its output would be wrong."""
    if TOPK_CHECK:
        err = _status(device, kinds)
        if err:
            bits = ", ".join(v for b, v in TOPK_ERRORS.items() if err & b)
            what = {("quant",): "quantizer", ("f64",): "float64 top-k select"}.get(tuple(kinds), "top-k encode")
            raise _lib.FlcError(f"{what} lost co-residency or failed ({bits}); its output may be wrong")


ORDER_SIGNED, ORDER_MAGNITUDE = 0, 1  # FLC_ORDER_* (include/flcodec.h)


def _order(order) -> int:
    """A select's order as FLC_ORDER_*: ``ORDER_SIGNED`` / ``"signed"`` (the reference's rule, compressors.py:293-296:
    the k largest signed values) or ``ORDER_MAGNITUDE`` / ``"magnitude"`` (the k largest |x|, each kept value x's
    own)."""
    if isinstance(order, str):
        if order not in ("signed", "magnitude"):
            raise ValueError(f"order must be 'signed' or 'magnitude' (got {order!r})")
        return ORDER_MAGNITUDE if order == "magnitude" else ORDER_SIGNED
    o = int(order)
    if o not in (ORDER_SIGNED, ORDER_MAGNITUDE):
        raise ValueError(f"order must be ORDER_SIGNED or ORDER_MAGNITUDE (got {order!r})")
    return o


def _call_ord(name: str, order: int, k_pos: int, *args) -> None:
    """``name`` in the signed order; otherwise its ``_ord`` form, which takes ``order`` after k (argument ``k_pos``)."""
    if order == ORDER_SIGNED:
        call(name, *args)
    else:
        call(name + "_ord", *args[:k_pos + 1], order, *args[k_pos + 1:])


def _tiles(n: int, device: torch.device) -> torch.Tensor:
    """CSR tile pointers over FLC_TILE-output tiles (include/flcodec.h)."""
    return torch.empty((n + TILE - 1) // TILE + 1, dtype=torch.int32, device=device)


def topk_encode(x: torch.Tensor, k: int, with_tiles: bool = False, order=ORDER_SIGNED):
    """Kept set of the reference Top-K (k largest signed values): (idx int32 ascending, val fp32), plus the
    tile pointers of idx when ``with_tiles`` (emitted by the encoder, saving the decoder an index pass).
    ``order=ORDER_MAGNITUDE``: the k largest |x| instead (:func:`_order`); ``val`` stays ``x[idx]``, signs included."""
    order = _order(order)
    x = _dev_f32(x).reshape(-1)
    n = x.numel()
    idx = torch.empty(k, dtype=torch.int32, device=x.device)
    val = torch.empty(k, dtype=torch.float32, device=x.device)
    tiles = _tiles(n, x.device) if with_tiles else None
    ws = workspace(x.device, _ws_size(x.device, "flc_topk_workspace_size", n, k), "topk")
    _call_ord("flc_topk_encode_tiled", order, 2, _p(x), n, k, _p(idx), _p(val), _p(tiles), _p(ws), ws.numel(),
              _stream(x.device))
    _after_encode(x.device)
    return (idx, val, tiles) if with_tiles else (idx, val)


def topk_encode_batch(xs: Sequence[torch.Tensor], k: int, with_tiles: bool = False, order=ORDER_SIGNED):
    """The top-k of many clients' flat deltas (one size) in one launch (flc_topk_encode_batch): entry c equals
    ``topk_encode(xs[c], k, with_tiles, order)``."""
    import ctypes

    order = _order(order)
    xs = [_dev_f32(x).reshape(-1) for x in xs]
    C = len(xs)
    if C == 0:
        return []
    n, dev = xs[0].numel(), xs[0].device
    if any(x.numel() != n or x.device != dev for x in xs):
        raise ValueError("a batched encode takes clients of one size on one device")
    ntl = (n + TILE - 1) // TILE + 1
    idx = torch.empty(C, k, dtype=torch.int32, device=dev)
    val = torch.empty(C, k, dtype=torch.float32, device=dev)
    tiles = torch.empty(C, ntl, dtype=torch.int32, device=dev) if with_tiles else None
    P = ctypes.c_void_p * C
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    ws = workspace(dev, _ws_size(dev, "flc_topk_encode_batch_workspace_size", n, k, C), "topk_batch")
    _call_ord("flc_topk_encode_batch", order, 3, vp(P(*[x.data_ptr() for x in xs])), C, n, k,
              vp(P(*[idx.data_ptr() + 4 * k * c for c in range(C)])),
              vp(P(*[val.data_ptr() + 4 * k * c for c in range(C)])),
              vp(P(*[tiles.data_ptr() + 4 * ntl * c for c in range(C)])) if with_tiles else None, _p(ws), ws.numel(),
              _stream(dev))
    _after_encode(dev)
    rows = zip(idx.unbind(0), val.unbind(0), tiles.unbind(0) if with_tiles else [None] * C)
    return [(i_, v_, t_) if with_tiles else (i_, v_) for i_, v_, t_ in rows]


def sparse_decode(idx: torch.Tensor, val: torch.Tensor, n: int, scale: float = 1.0, out: Optional[torch.Tensor] = None,
                  weight: float = 1.0, accumulate: bool = False, tiles: Optional[torch.Tensor] = None) -> torch.Tensor:
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=val.device)
    if tiles is not None:
        call("flc_sparse_decode_tiled", _p(idx), _p(val), idx.numel(), scale, n, weight, int(accumulate), _p(out),
             _p(tiles), _stream(out.device))
        return out
    ws = workspace(out.device, _ws_size(out.device, "flc_sparse_decode_workspace_size", n), "decode")
    call("flc_sparse_decode", _p(idx), _p(val), idx.numel(), scale, n, weight, int(accumulate), _p(out), _p(ws),
         ws.numel(), _stream(out.device))
    return out


@dataclass
class StackedPacket:
    """Wire of the stacked codec: ascending int32 indices, 8-bit (sign | level) codes, fp32 norm; plus the
    encoder-emitted tile pointers of the indices (CSR over 1024-output tiles), the decoder's index."""

    idx: torch.Tensor
    codes: torch.Tensor
    norm: torch.Tensor
    n: int
    levels: int
    tiles: Optional[torch.Tensor] = None

    @property
    def nbytes(self) -> int:
        return 5 * self.idx.numel() + 4 + (4 * self.tiles.numel() if self.tiles is not None else 0)


class PacketBatch(_abc.Sequence):
    """The packets of a batched encode (one row per client of four [clients, ...] blocks), made on demand: packet c
    is ``StackedPacket(idx[c], codes[c], norm[c], n, levels, tiles[c])``.  A round of many small clients would
    otherwise spend more host time building views than the GPU spends encoding (4 views x 100 clients)."""

    def __init__(self, idx, codes, norm, tiles, n: int, levels: int):
        self.idx, self.codes, self.norm, self.tiles, self.n, self.levels = idx, codes, norm, tiles, n, levels

    def __len__(self) -> int:
        return self.idx.shape[0]

    def __getitem__(self, c):
        if isinstance(c, slice):
            return [self[i] for i in range(*c.indices(len(self)))]
        if c < 0:
            c += len(self)
        if not 0 <= c < len(self):
            raise IndexError(c)
        return StackedPacket(self.idx[c], self.codes[c], self.norm[c], self.n, self.levels,
                             None if self.tiles is None else self.tiles[c])


def _batch_ptrs(xs: Sequence[torch.Tensor], n: int, dev: torch.device) -> Optional[List[int]]:
    """The clients' data pointers when every one is a contiguous, 16-B aligned fp32 tensor of n elements on `dev`
    (one lean pass: the batch may hold hundreds of clients); None otherwise."""
    f32, di = torch.float32, dev.index
    out = []
    for x in xs:
        if not (isinstance(x, torch.Tensor) and x.dtype is f32 and x.numel() == n and x.is_contiguous()
                and x.get_device() == di):
            return None
        p = x.data_ptr()
        if p & 15:
            return None
        out.append(p)
    return out


_WIRE_LAYOUT = {}


def stacked_wire_layout(n: int, k: int):
    """(record bytes, {"norm", "idx", "codes", "tiles"} byte offsets) of the packed stacked wire
    (flc_stacked_wire_layout): one contiguous record per client whose layout depends on (n, k) only."""
    import ctypes

    key = (int(n), int(k))
    r = _WIRE_LAYOUT.get(key)
    if r is None:
        off = (ctypes.c_int64 * 4)()
        total = _lib.size("flc_stacked_wire_layout", int(n), int(k), ctypes.cast(off, ctypes.c_void_p))
        if total == 0:
            raise ValueError(f"bad wire shape n={n}, k={k}")
        r = (int(total), dict(zip(("norm", "idx", "codes", "tiles"), (int(v) for v in off))))
        _WIRE_LAYOUT[key] = r
    return r


def wire_packet(record: torch.Tensor, n: int, k: int, levels: int = 127) -> StackedPacket:
    """The StackedPacket whose tensors are views into one packed wire record (a uint8 HIP tensor of at least
    ``stacked_wire_layout(n, k)[0]`` bytes, 16-B aligned)."""
    stride, off = stacked_wire_layout(n, k)
    if record.dtype != torch.uint8 or record.device.type != "cuda" or not record.is_contiguous():
        raise TypeError("a wire record is a contiguous uint8 HIP tensor")
    rec = record.reshape(-1)
    if rec.numel() < stride or rec.data_ptr() % 16 != 0:
        raise ValueError(f"a wire record needs {stride} bytes, 16-B aligned")
    ntiles = (n + TILE - 1) // TILE + 1
    return StackedPacket(rec[off["idx"]:off["idx"] + 4 * k].view(torch.int32),
                         rec[off["codes"]:off["codes"] + max(k, 16)],
                         rec[off["norm"]:off["norm"] + 4].view(torch.float32), int(n), int(levels),
                         rec[off["tiles"]:off["tiles"] + 4 * ntiles].view(torch.int32))


def stacked_encode(x: torch.Tensor, k: int, levels: int = 127, seed: int = 0, counter: int = 0,
                   with_tiles: bool = True, wire: Optional[torch.Tensor] = None,
                   out: Optional[StackedPacket] = None, order=ORDER_SIGNED) -> StackedPacket:
    """Stacked top-k -> 8-bit dithering encode.  ``wire``: a packed wire record (see :func:`wire_packet`) to write
    the packet into; the returned packet's tensors are then views of it.  ``out``: a packet of the same (n, k) whose
    tensors are overwritten (no allocation per call); it is returned.  ``order``: the top-k stage's selection order
    (:func:`_order`); the packet, its decode and every fold are the same either way."""
    order = _order(order)
    x = _dev_f32(x).reshape(-1)
    n = x.numel()
    if out is not None:
        if out.n != n or out.idx.numel() != k or out.idx.device != x.device or (with_tiles and out.tiles is None):
            raise ValueError("`out` must be a packet of the same n and k on the input's device")
        idx, codes, norm, tiles = out.idx, out.codes, out.norm, out.tiles if with_tiles else None
    elif wire is not None:
        if wire.device != x.device:
            raise ValueError("the wire record must be on the input's device")
        pk = wire_packet(wire, n, k, levels)
        idx, codes, norm, tiles = pk.idx, pk.codes, pk.norm, pk.tiles
    else:
        idx = torch.empty(k, dtype=torch.int32, device=x.device)
        codes = torch.empty(max(k, 16), dtype=torch.uint8, device=x.device)
        norm = torch.empty(1, dtype=torch.float32, device=x.device)
        tiles = _tiles(n, x.device) if with_tiles else None
    ws = workspace(x.device, _ws_size(x.device, "flc_topk_workspace_size", n, k), "topk")
    _call_ord("flc_stacked_encode_tiled", order, 2, _p(x), n, k, levels, seed, counter, None, _p(idx), _p(codes),
              _p(norm), _p(tiles), _p(ws), ws.numel(), _stream(x.device))
    _after_encode(x.device)
    return StackedPacket(idx, codes, norm, n, levels, tiles)


def _round_args(C: int, dev, counter: int, counters, counts):
    """The per-client Philox counters and count destinations of a round encode (flc_stacked_encode[_delta]_round) as
    ctypes arrays: ``counters`` (None: ``counter`` for every client) and ``counts`` (None: no counts) — a contiguous
    device int64 tensor of C elements, or a sequence of C one-element device int64 tensors."""
    import ctypes

    ctr = [int(counter)] * C if counters is None else [int(t) for t in counters]
    if len(ctr) != C:
        raise ValueError("one counter per client")
    cp = None
    if counts is not None:
        if isinstance(counts, torch.Tensor):
            if counts.dtype != torch.int64 or counts.numel() != C or not counts.is_contiguous() or counts.device != dev:
                raise ValueError(f"counts must be a contiguous int64 tensor of {C} elements on {dev}")
            ptrs = [counts.data_ptr() + 8 * c for c in range(C)]
        else:
            counts = list(counts)
            if len(counts) != C or any(t.dtype != torch.int64 or t.numel() != 1 or t.device != dev for t in counts):
                raise ValueError(f"counts must be {C} one-element int64 tensors on {dev}")
            ptrs = [t.data_ptr() for t in counts]
        cp = (ctypes.c_void_p * C)(*ptrs)
    return (ctypes.c_uint64 * C)(*ctr), cp


def stacked_encode_batch(xs: Sequence[torch.Tensor], k: int, levels: int = 127, seeds: Sequence[int] = (),
                         counter: int = 0, with_tiles: bool = True, wires=None, counters: Optional[Sequence[int]] = None,
                         counts=None, order=ORDER_SIGNED) -> Optional[Sequence[StackedPacket]]:
    """The stacked encode of many clients' flat deltas (all of one size) in one launch (flc_stacked_encode_batch):
    packet c equals ``stacked_encode(xs[c], k, levels, seeds[c], counter)`` bit for bit.  ``wires``: the packed wire
    records to write into — a ``[clients, >= stride]`` uint8 tensor (then nothing is returned: the records are the
    output) or a list of one record per client (the packets returned are views of them).  ``counters``: one Philox
    counter per client in place of ``counter``; ``counts``: a device int64 tensor ``[clients]`` (or a list of
    one-element ones) that receives each packet's number of kept entries with a nonzero (or NaN) value — either keyword
    takes the call through flc_stacked_encode_round, whose encode makes the counts itself, and so does
    ``order=ORDER_MAGNITUDE`` (one order for the whole call, :func:`_order`)."""
    import ctypes

    order = _order(order)
    C = len(xs)
    if C == 0:
        return []
    x0 = xs[0]
    n, dev = x0.numel(), x0.device
    xp = _batch_ptrs(xs, n, dev) if dev.type == "cuda" else None
    if xp is None:  # (the slow path: checks with messages, copies of misaligned inputs)
        xs = [_dev_f32(x).reshape(-1) for x in xs]
        if any(x.numel() != n or x.device != dev for x in xs):
            raise ValueError("a batched encode takes clients of one size on one device")
        xp = [x.data_ptr() for x in xs]
    seeds = list(seeds) if len(seeds) else [0] * C
    if len(seeds) != C:
        raise ValueError("one seed per client")
    P = ctypes.c_void_p * C
    stride, off = stacked_wire_layout(n, k)
    pks = None
    if isinstance(wires, torch.Tensor):  # one [C, >= stride] record block: pointers by arithmetic
        if (wires.dtype != torch.uint8 or wires.dim() != 2 or wires.shape[0] != C or wires.shape[1] < stride
                or not wires.is_contiguous() or wires.device != dev or wires.data_ptr() % 16 or wires.shape[1] % 16):
            raise ValueError(f"records must be a contiguous [{C}, >= {stride}] uint8 block (16-B rows) on {dev}")
        rs = wires.shape[1]
        bases = [wires.data_ptr() + c * rs for c in range(C)]
        ptr = {f: P(*[b + off[f] for b in bases]) for f in ("idx", "codes", "norm", "tiles")}
    else:
        if wires is not None:
            if len(wires) != C:
                raise ValueError("one wire record per client")
            pks = [wire_packet(r, n, k, levels) for r in wires]
            ptr = {"idx": P(*[p.idx.data_ptr() for p in pks]), "codes": P(*[p.codes.data_ptr() for p in pks]),
                   "norm": P(*[p.norm.data_ptr() for p in pks]), "tiles": P(*[p.tiles.data_ptr() for p in pks])}
        else:  # one block per field, the packets its rows (views made in one unbind each)
            ntl = (n + TILE - 1) // TILE + 1
            kc = max(k, 16)
            idx = torch.empty(C, k, dtype=torch.int32, device=dev)
            codes = torch.empty(C, kc, dtype=torch.uint8, device=dev)
            norm = torch.empty(C, 1, dtype=torch.float32, device=dev)
            tiles = torch.empty(C, ntl, dtype=torch.int32, device=dev) if with_tiles else None
            pks = PacketBatch(idx, codes, norm, tiles, n, levels)
            b = {f: t.data_ptr() for f, t in (("idx", idx), ("codes", codes), ("norm", norm))}
            ptr = {"idx": P(*[b["idx"] + 4 * k * c for c in range(C)]),
                   "codes": P(*[b["codes"] + kc * c for c in range(C)]),
                   "norm": P(*[b["norm"] + 4 * c for c in range(C)]),
                   "tiles": P(*[tiles.data_ptr() + 4 * ntl * c for c in range(C)]) if with_tiles else None}
    ws = workspace(dev, _ws_size(dev, "flc_stacked_encode_batch_workspace_size", n, k, C), "topk_batch")
    vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    if counters is None and counts is None and order == ORDER_SIGNED:
        call("flc_stacked_encode_batch", vp(P(*xp)), C, n, k, levels,
             vp((ctypes.c_uint64 * C)(*[int(s_) for s_ in seeds])), counter, vp(ptr["idx"]), vp(ptr["codes"]),
             vp(ptr["norm"]), vp(ptr["tiles"]), _p(ws), ws.numel(), _stream(dev))
    else:
        ctr, cp = _round_args(C, dev, counter, counters, counts)
        _call_ord("flc_stacked_encode_round", order, 3, vp(P(*xp)), C, n, k, levels,
                  vp((ctypes.c_uint64 * C)(*[int(s_) for s_ in seeds])), vp(ctr), vp(ptr["idx"]), vp(ptr["codes"]),
                  vp(ptr["norm"]), vp(ptr["tiles"]), vp(cp), _p(ws), ws.numel(), _stream(dev))
    _after_encode(dev)
    return pks


def stacked_encode_delta_batch(local_params: Sequence[Sequence[torch.Tensor]], global_params: Sequence[torch.Tensor],
                               k: int, levels: int = 127, seeds: Sequence[int] = (), counter: int = 0,
                               counters: Optional[Sequence[int]] = None, counts=None,
                               order=ORDER_SIGNED) -> "PacketBatch":
    """The delta-fused stacked encode of a round's clients in one launch (flc_stacked_encode_delta_batch): client c's
    delta ``cat([l - g for l, g in zip(local_params[c], global_params)])`` (the global model shared by every client),
    packet c equal to ``stacked_encode_delta(local_params[c], global_params, k, levels, seeds[c], counter)``.
    ``counters`` / ``counts`` / ``order``: as in :func:`stacked_encode_batch` (flc_stacked_encode_delta_round)."""
    import ctypes

    order = _order(order)
    C = len(local_params)
    if C == 0:
        return []
    ok = lambda t: t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 4 == 0  # noqa: E731
    gs = [t if ok(t) else t.contiguous().float() for t in global_params]
    ls = [[t if ok(t) else t.contiguous().float() for t in lp] for lp in local_params]
    m = len(gs)
    if m == 0 or any(len(lp) != m for lp in ls):
        raise ValueError("every client has one local tensor per global tensor, at least one")
    dev = gs[0].device
    for lp in ls:
        for a, b in zip(lp, gs):
            if a.numel() != b.numel() or a.device != dev or b.device != dev or dev.type != "cuda":
                raise ValueError("local and global tensors must be HIP tensors of matching sizes on one device")
    n = sum(t.numel() for t in gs)
    seeds = list(seeds) if len(seeds) else [0] * C
    if len(seeds) != C:
        raise ValueError("one seed per client")
    ntl = (n + TILE - 1) // TILE + 1
    kc = max(k, 16)
    idx = torch.empty(C, k, dtype=torch.int32, device=dev)
    codes = torch.empty(C, kc, dtype=torch.uint8, device=dev)
    norm = torch.empty(C, 1, dtype=torch.float32, device=dev)
    tiles = torch.empty(C, ntl, dtype=torch.int32, device=dev)
    P = ctypes.c_void_p
    vp = lambda a: ctypes.cast(a, P)  # noqa: E731
    ws = workspace(dev, _ws_size(dev, "flc_stacked_encode_delta_batch_workspace_size", n, k, C, m), "topk_batch")
    if counters is None and counts is None and order == ORDER_SIGNED:
        name, ctr, cnt = "flc_stacked_encode_delta_batch", (counter,), ()
    else:
        ca, cp = _round_args(C, dev, counter, counters, counts)
        name, ctr, cnt = "flc_stacked_encode_delta_round", (vp(ca),), (None if cp is None else vp(cp),)
    _call_ord(name, order, 5, vp((P * (C * m))(*[t.data_ptr() for lp in ls for t in lp])),
              vp((P * m)(*[t.data_ptr() for t in gs])), vp((ctypes.c_int64 * m)(*[t.numel() for t in gs])), m, C, k,
              levels, vp((ctypes.c_uint64 * C)(*[int(s_) for s_ in seeds])), *ctr,
              vp((P * C)(*[idx.data_ptr() + 4 * k * c for c in range(C)])),
              vp((P * C)(*[codes.data_ptr() + kc * c for c in range(C)])),
              vp((P * C)(*[norm.data_ptr() + 4 * c for c in range(C)])),
              vp((P * C)(*[tiles.data_ptr() + 4 * ntl * c for c in range(C)])), *cnt, _p(ws), ws.numel(), _stream(dev))
    _after_encode(dev)
    return PacketBatch(idx, codes, norm, tiles, n, levels)


def stacked_encode_delta(local_params: Sequence[torch.Tensor], global_params: Sequence[torch.Tensor], k: int,
                         levels: int = 127, seed: int = 0, counter: int = 0,
                         wire: Optional[torch.Tensor] = None, order=ORDER_SIGNED) -> StackedPacket:
    """The stacked encode of the client delta ``cat([l - g for l, g in zip(local, global)])`` with the delta formed in
    the encoder's read pass (flc_stacked_encode_delta): the flat delta is never written.  Same packet as
    ``stacked_encode(delta_flatten(local, global), ...)``.  ``wire``: a packed wire record to write into (the packet's
    tensors are then views of it, see :func:`wire_packet`).  ``order``: as in :func:`stacked_encode` (by magnitude:
    |local - global|)."""
    import ctypes

    order = _order(order)
    ls = [t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 4 == 0) else t.contiguous().float()
          for t in local_params]
    gs = [t if (t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 4 == 0) else t.contiguous().float()
          for t in global_params]
    if len(ls) != len(gs) or not ls:
        raise ValueError("one global tensor per local tensor, at least one")
    for a, b in zip(ls, gs):
        if a.numel() != b.numel() or a.device != b.device or a.device.type != "cuda":
            raise ValueError("local and global tensors must be HIP tensors of matching sizes")
    dev = ls[0].device
    n = sum(t.numel() for t in ls)
    m = len(ls)
    lp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in ls])
    gp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in gs])
    sz = (ctypes.c_int64 * m)(*[t.numel() for t in ls])
    if wire is not None:
        if wire.device != dev:
            raise ValueError("the wire record must be on the tensors' device")
        pk = wire_packet(wire, n, k, levels)
        idx, codes, norm, tiles = pk.idx, pk.codes, pk.norm, pk.tiles
    else:
        idx = torch.empty(k, dtype=torch.int32, device=dev)
        codes = torch.empty(max(k, 16), dtype=torch.uint8, device=dev)
        norm = torch.empty(1, dtype=torch.float32, device=dev)
        tiles = _tiles(n, dev)
    ws = workspace(dev, _ws_size(dev, "flc_stacked_encode_delta_workspace_size", n, k, m), "topk")
    _call_ord("flc_stacked_encode_delta", order, 4, ctypes.cast(lp, ctypes.c_void_p), ctypes.cast(gp, ctypes.c_void_p),
              ctypes.cast(sz, ctypes.c_void_p), m, k, levels, seed, counter, _p(idx), _p(codes), _p(norm), _p(tiles),
              _p(ws), ws.numel(), _stream(dev))
    _after_encode(dev)
    return StackedPacket(idx, codes, norm, n, levels, tiles)


def stacked_decode(pkt: StackedPacket, out: Optional[torch.Tensor] = None, weight: float = 1.0,
                   accumulate: bool = False) -> torch.Tensor:
    if out is None:
        out = torch.empty(pkt.n, dtype=torch.float32, device=pkt.idx.device)
    if pkt.tiles is not None:
        call("flc_stacked_decode_tiled", _p(pkt.idx), _p(pkt.codes), pkt.idx.numel(), pkt.levels, _p(pkt.norm), pkt.n,
             weight, int(accumulate), _p(out), _p(pkt.tiles), _stream(out.device))
        return out
    ws = workspace(out.device, _ws_size(out.device, "flc_sparse_decode_workspace_size", pkt.n), "decode")
    call("flc_stacked_decode", _p(pkt.idx), _p(pkt.codes), pkt.idx.numel(), pkt.levels, _p(pkt.norm), pkt.n, weight,
         int(accumulate), _p(out), _p(ws), ws.numel(), _stream(out.device))
    return out


# ------------------------------------------------------------------------- sparse records (top-k / rand-k wire)
_SPARSE_LAYOUT = {}


def sparse_wire_layout(n: int, k: int):
    """(record bytes, {"idx", "val", "tiles"} byte offsets) of a sparse record (flc_sparse_wire_layout): the top-k /
    rand-k wire — ascending int32 indices, the decoded fp32 values, tile pointers — as one contiguous record whose
    layout depends on (n, k) only."""
    import ctypes

    key = (int(n), int(k))
    r = _SPARSE_LAYOUT.get(key)
    if r is None:
        off = (ctypes.c_int64 * 3)()
        total = _lib.size("flc_sparse_wire_layout", key[0], key[1], ctypes.cast(off, ctypes.c_void_p))
        if total == 0:
            raise ValueError(f"bad sparse record shape n={n}, k={k}")
        r = _SPARSE_LAYOUT[key] = (int(total), dict(zip(("idx", "val", "tiles"), (int(v) for v in off))))
    return r


def sparse_wire_views(record: torch.Tensor, n: int, k: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(idx, val, tiles) views into a sparse record (a contiguous uint8 HIP tensor of at least
    ``sparse_wire_layout(n, k)[0]`` bytes, 16-B aligned)."""
    stride, off = sparse_wire_layout(n, k)
    if record.dtype != torch.uint8 or record.device.type != "cuda" or not record.is_contiguous():
        raise TypeError("a wire record is a contiguous uint8 HIP tensor")
    rec = record.reshape(-1)
    if rec.numel() < stride or rec.data_ptr() % 16 != 0:
        raise ValueError(f"a sparse record needs {stride} bytes, 16-B aligned")
    ntiles = (n + TILE - 1) // TILE + 1
    return (rec[off["idx"]:off["idx"] + 4 * k].view(torch.int32), rec[off["val"]:off["val"] + 4 * k].view(torch.float32),
            rec[off["tiles"]:off["tiles"] + 4 * ntiles].view(torch.int32))


def sparse_record_decode(record: torch.Tensor, n: int, k: int, out: Optional[torch.Tensor] = None,
                         weight: float = 1.0, accumulate: bool = False) -> torch.Tensor:
    """The decoded flat vector of a sparse record (flc_sparse_decode_tiled on its views, scale 1)."""
    idx, val, tiles = sparse_wire_views(record, n, k)
    return sparse_decode(idx, val, n, 1.0, out=out, weight=weight, accumulate=accumulate, tiles=tiles)


def topk_encode_record(x: torch.Tensor, k: int, record: torch.Tensor, order=ORDER_SIGNED) -> torch.Tensor:
    """The top-k of the flat vector ``x`` (``order``: as in :func:`topk_encode`) written into the sparse record
    ``record`` (flc_topk_encode_tiled with the three pointers inside it)."""
    order = _order(order)
    x = _dev_f32(x).reshape(-1)
    n = x.numel()
    idx, val, tiles = sparse_wire_views(record, n, k)
    ws = workspace(x.device, _ws_size(x.device, "flc_topk_workspace_size", n, k), "topk")
    _call_ord("flc_topk_encode_tiled", order, 2, _p(x), n, k, _p(idx), _p(val), _p(tiles), _p(ws), ws.numel(),
              _stream(x.device))
    _after_encode(x.device)
    return record


def topk_encode_records(xs: Sequence[torch.Tensor], k: int, records: torch.Tensor,
                        order=ORDER_SIGNED) -> torch.Tensor:
    """A round's top-k messages in one call (flc_topk_encode_batch): row c of the ``[C, >= stride]`` uint8 block
    ``records`` (16-B rows) takes the sparse record of the flat fp32 vector ``xs[c]`` — all of one size on one device —
    equal to ``topk_encode_record(xs[c], k, records[c], order)``."""
    import ctypes

    order = _order(order)
    C = len(xs)
    if C == 0:
        return records
    n, dev = xs[0].numel(), xs[0].device
    xp = _batch_ptrs(xs, n, dev) if dev.type == "cuda" else None
    if xp is None:
        xs = [_dev_f32(x).reshape(-1) for x in xs]
        if any(x.numel() != n or x.device != dev for x in xs):
            raise ValueError("a batched encode takes clients of one size on one device")
        xp = [x.data_ptr() for x in xs]
    stride, off = sparse_wire_layout(n, k)
    if not (isinstance(records, torch.Tensor) and records.dim() == 2 and records.shape[0] == C
            and records.shape[1] % 16 == 0 and records.device == dev):
        raise ValueError(f"records must be a [{C}, >= {stride}] uint8 block (16-B rows) on {dev}")
    sparse_wire_views(records[0], n, k)  # (dtype, size and alignment, checked on one row for all)
    bases = [records.data_ptr() + c * records.shape[1] for c in range(C)]
    P = ctypes.c_void_p * C
    vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
    ws = workspace(dev, _ws_size(dev, "flc_topk_encode_batch_workspace_size", n, k, C), "topk_batch")
    with torch.cuda.device(dev):
        _call_ord("flc_topk_encode_batch", order, 3, vp(P(*xp)), C, n, k, vp(P(*[b + off["idx"] for b in bases])),
                  vp(P(*[b + off["val"] for b in bases])), vp(P(*[b + off["tiles"] for b in bases])), _p(ws),
                  ws.numel(), _stream(dev))
    _after_encode(dev)
    return records


def sparse_gather(x: torch.Tensor, idx: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[j] = fp32(scale) * x[idx[j]]`` (flc_sparse_gather): rand-k's kept values, bit-equal to what
    ``randk_apply`` scatters; ``out``: a sparse record's val view."""
    x = _dev_f32(x).reshape(-1)
    k = idx.numel()
    if out is None:
        out = torch.empty(k, dtype=torch.float32, device=x.device)
    call("flc_sparse_gather", _p(x), x.numel(), _p(idx), k, scale, _p(out), _stream(x.device))
    return out


def fold_sparse_wires(wires: torch.Tensor, slots: Sequence[int], weights: Sequence[float], n: int, k: int,
                      out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """``out = (accumulate ? out : 0) + Σ_c weights[c] · decode(wires[slots[c]])`` in client order, one pass
    (flc_fold_sparse_wires).  ``wires``: a [records, stride] uint8 HIP tensor of sparse records."""
    import ctypes

    if wires.dtype != torch.uint8 or wires.dim() != 2 or not wires.is_contiguous() or wires.device.type != "cuda":
        raise TypeError("wires must be a contiguous [records, stride] uint8 HIP tensor")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an out tensor")
        out = torch.empty(n, dtype=torch.float32, device=wires.device)
    m = len(slots)
    call("flc_fold_sparse_wires", _p(wires), wires.shape[1], (ctypes.c_int32 * m)(*[int(s) for s in slots]),
         (ctypes.c_float * m)(*[float(w) for w in weights]), m, n, k, int(accumulate), _p(out), _stream(wires.device))
    return out


def stacked_fold_wires(wires: torch.Tensor, slots: Sequence[int], weights: Sequence[float], n: int, k: int,
                       levels: int = 127, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """Server fold of many clients' packed wires in one pass (flc_stacked_fold_wires):
    ``out = (out if accumulate else +0)``, then ``out = fmaf(weights[c], decode(wires[slots[c]]), out)`` for c in
    order — bit-identical to zeroing ``out`` and calling ``stacked_decode(..., weight, accumulate=True)`` per client.
    ``wires``: uint8 HIP tensor [records, stride] (or flat, records of ``stacked_wire_layout(n, k)[0]`` bytes)."""
    import ctypes

    stride, _ = stacked_wire_layout(n, k)
    if wires.dtype != torch.uint8 or wires.device.type != "cuda" or not wires.is_contiguous():
        raise TypeError("wires must be a contiguous uint8 HIP tensor")
    if wires.dim() == 2:
        stride = wires.shape[1]
    nrec = wires.numel() // stride
    if len(slots) != len(weights) or not slots:
        raise ValueError("one weight per slot, at least one")
    if min(slots) < 0 or max(slots) >= nrec:
        raise ValueError(f"slots must index the {nrec} records")
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs an out tensor")
        out = torch.empty(n, dtype=torch.float32, device=wires.device)
    elif out.device != wires.device or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n:
        raise ValueError(f"out must be a contiguous fp32 tensor of {n} elements on {wires.device}")
    m = len(slots)
    sl = (ctypes.c_int32 * m)(*[int(v) for v in slots])
    wt = (ctypes.c_float * m)(*[float(v) for v in weights])
    call("flc_stacked_fold_wires", _p(wires), stride, ctypes.cast(sl, ctypes.c_void_p), ctypes.cast(wt, ctypes.c_void_p),
         m, n, k, levels, int(accumulate), _p(out), _stream(out.device))
    return out


# -------------------------------------------------------------------------------------- adaptive random
ADAPTIVE_ERRORS = {1: "probabilities contain NaN", 2: "probabilities do not sum to 1"}


def adaptive_prepare(x: torch.Tensor) -> torch.Tensor:
    """First half of the adaptive random compressor (compressors.py:297-301): S = sum|x| in numpy's order,
    p = |x| / S, and the speculated runs of the fp64 cumsum.  Returns numpy's check as a device int32:
    0 = ok, 1 = NaN in p, 2 = p does not sum to 1 (see ADAPTIVE_ERRORS).  No uniform is consumed.  A float64 x
    runs the float64 form (S and p in fp64, flc_adaptive_prepare_f64)."""
    f64 = isinstance(x, torch.Tensor) and x.dtype == torch.float64
    x = (_dev_f64(x) if f64 else _dev_f32(x)).reshape(-1)
    n = x.numel()
    if n == 0:
        raise ValueError("'a' cannot be empty unless no samples are taken")
    status = torch.empty(1, dtype=torch.int32, device=x.device)
    ws = workspace(x.device, _ws_size(x.device, "flc_adaptive_workspace_size", n), "adaptive")
    call("flc_adaptive_prepare_f64" if f64 else "flc_adaptive_prepare", _p(x), n, _p(status), _p(ws), ws.numel(),
         _stream(x.device))
    return status


def adaptive_select(x: torch.Tensor, u: float, out: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Second half, after :func:`adaptive_prepare` on the same stream: the exact sequential cdf,
    ``searchsorted(u, side='right')`` and the dense output (zeros, out[ind] = x[ind]).
    Returns (out, index as a device int64)."""
    f64 = isinstance(x, torch.Tensor) and x.dtype == torch.float64
    x = (_dev_f64(x) if f64 else _dev_f32(x)).reshape(-1)
    n = x.numel()
    if out is None:
        out = torch.empty(n, dtype=x.dtype, device=x.device)
    index = torch.empty(1, dtype=torch.int64, device=x.device)
    ws = workspace(x.device, _ws_size(x.device, "flc_adaptive_workspace_size", n), "adaptive")
    call("flc_adaptive_select_f64" if f64 else "flc_adaptive_select", _p(x), n, float(u), _p(index), _p(out), _p(ws),
         ws.numel(), _stream(x.device))
    return out, index


def adaptive_stats(x: torch.Tensor) -> dict:
    """Diagnostics of the last :func:`adaptive_select` on x's workspace (host sync): special chunks, special maps
    taken, chunks re-run sequentially, and whether the exact sequential chain ran instead."""
    x = x.reshape(-1)
    n = x.numel()
    ws = workspace(x.device, _ws_size(x.device, "flc_adaptive_workspace_size", n), "adaptive")
    st = torch.empty(4, dtype=torch.int32, device=x.device)
    call("flc_adaptive_stats", _p(ws), ws.numel(), n, _p(st), _stream(x.device))
    s = [int(v) for v in st.cpu()]
    return {"special": s[0], "taken": s[1], "reruns": s[2], "sequential": s[3]}


# ------------------------------------------------------------------------------------------------- misc
def copy(x: torch.Tensor) -> torch.Tensor:
    x = _dev_f32(x)
    out = torch.empty_like(x)
    call("flc_copy", _p(x), x.numel(), _p(out), _stream(x.device))
    return out


def scale_div(x: torch.Tensor, p: float) -> torch.Tensor:
    x = _dev_f32(x)
    out = torch.empty_like(x)
    call("flc_scale_div", _p(x), x.numel(), p, _p(out), _stream(x.device))
    return out


def randk_indices(n: int, k: int, seed: int, counter: int, device: torch.device) -> torch.Tensor:
    """Rand-K's index set in philox mode, on the device: the k largest of n Philox keys (flc_randk_keys + the top-k
    encoder), int32 ascending.  k >= n gives every index (the reference's ``S[:K]`` of a full permutation)."""
    if k >= n:
        return torch.arange(n, dtype=torch.int32, device=device)
    if k <= 0:
        return torch.empty(0, dtype=torch.int32, device=device)
    keys = torch.empty(n, dtype=torch.float32, device=device)
    call("flc_randk_keys", n, seed, counter, _p(keys), _stream(device))
    idx, _ = topk_encode(keys, k)
    return idx


def randk_apply(x: torch.Tensor, idx: torch.Tensor, scale: float) -> torch.Tensor:
    x = _dev_f32(x).reshape(-1)
    out = torch.empty_like(x)
    call("flc_randk_apply", _p(x), x.numel(), _p(idx), idx.numel(), scale, _p(out), _stream(x.device))
    return out


def weighted_sum(dst: torch.Tensor, srcs: Sequence[torch.Tensor], weights: Sequence[float], init_mode: int,
                 beta: float = 0.0) -> torch.Tensor:
    """dst = {dst*beta | 0 | dst} then dst = fmaf(w_m, src_m, dst) for each message in order."""
    import ctypes

    f64 = dst.dtype == torch.float64  # float64 models: the fold in fp64, the weights kept double (flc_weighted_sum_f64)
    if dst.device.type != "cuda" or dst.dtype not in (torch.float32, torch.float64) or not dst.is_contiguous():
        raise TypeError("dst must be a contiguous fp32 or fp64 HIP tensor")
    n = dst.numel()
    srcs = [(_dev_f64 if f64 else _dev_f32)(s, "src") for s in srcs]
    for s in srcs:
        if s.numel() != n:
            raise ValueError("every source must have dst's number of elements")
    ptrs = (ctypes.c_void_p * max(len(srcs), 1))(*[s.data_ptr() for s in srcs])
    ws = ((ctypes.c_double if f64 else ctypes.c_float) * max(len(srcs), 1))(*[float(w) for w in weights])
    call("flc_weighted_sum_f64" if f64 else "flc_weighted_sum", ctypes.cast(ptrs, ctypes.c_void_p),
         ctypes.cast(ws, ctypes.c_void_p), len(srcs), n, init_mode, float(beta), _p(dst), _stream(dst.device))
    return dst


MODEL_FOLD_MAX_SRC = 16


_MODEL_FOLD_OP: list = []


def _model_fold_op():
    """torch.ops.flcodec.model_fold_ when libflcodec_torch.so is built (the same C-ABI call, its per-tensor checks in
    C++), else None (the ctypes path below)."""
    if not _MODEL_FOLD_OP:
        op = None
        try:
            from . import load_torch_ops

            load_torch_ops()
            op = torch.ops.flcodec.model_fold_
        except (ImportError, OSError, RuntimeError, AttributeError):
            op = None
        _MODEL_FOLD_OP.append(op)
    return _MODEL_FOLD_OP[0]


def _flcfold_entry(cell: list, name: str):
    """fl_sim_amd._flcfold.<name> (csrc/pyfold.cpp: the C-ABI call on Python lists of tensors, no dispatcher boxing)
    when built, else None (the ctypes path); a missing module and a missing entry both count as not built.  Looked up
    once: ``cell`` is the entry's module-level one-element cache, empty until then.  The cells stay module attributes
    because the tests force the ctypes path by replacing one (``monkeypatch.setattr(codec, "_PYFOLD", [None])``)."""
    if not cell:
        try:
            from . import _flcfold

            cell.append(getattr(_flcfold, name))
        except (ImportError, AttributeError):
            cell.append(None)
    return cell[0]


_PYFOLD: list = []
_PYSRV: list = []
_PYPAIR: list = []
_PYRECS: list = []
_PYDRECS: list = []
_PYSRECS: list = []
_PYMRECS: list = []
_PYGROUPS: list = []
_PYGRECS: list = []
_PYGDRECS: list = []
_PYGSRECS: list = []
_PYFLAT: list = []
_PYROUND: list = []
_PYDELTA: list = []
_PYEF: list = []


def _pyfold():
    """_flcfold.model_fold (the fold on lists of tensors, more than 16 messages in chained launches), or None."""
    return _flcfold_entry(_PYFOLD, "model_fold")


def _pysrv():
    """_flcfold.server_fold (flc_model_fold_server on lists of tensors, at most 16 messages), or None."""
    return _flcfold_entry(_PYSRV, "server_fold")


def _pypair():
    """_flcfold.avg_and_gradients (flc_avg_and_gradients on lists of tensors and message mappings), or None."""
    return _flcfold_entry(_PYPAIR, "avg_and_gradients")


def _pyrecs():
    """_flcfold.fold_records (flc_fedopt_fold_records on lists, one C call), or None."""
    return _flcfold_entry(_PYRECS, "fold_records")


def _pydrecs():
    """_flcfold.fold_dense_records (flc_fedopt_fold_dense_records on lists, one C call), or None."""
    return _flcfold_entry(_PYDRECS, "fold_dense_records")


def _pysrecs():
    """_flcfold.fold_sparse_records (flc_fedopt_fold_sparse_records on lists, one C call), or None."""
    return _flcfold_entry(_PYSRECS, "fold_sparse_records")


def _pymrecs():
    """_flcfold.fold_mixed_records (flc_fedopt_fold_mixed_records on lists, one C call), or None."""
    return _flcfold_entry(_PYMRECS, "fold_mixed_records")


def _pygroups():
    """_flcfold.fold_record_groups (flc_fold_record_groups on lists, one C call), or None."""
    return _flcfold_entry(_PYGROUPS, "fold_record_groups")


def _pygrecs():
    """_flcfold.avg_and_gradient_records (flc_avg_and_gradient_records on lists, one C call), or None."""
    return _flcfold_entry(_PYGRECS, "avg_and_gradient_records")


def _pygdrecs():
    """_flcfold.avg_and_gradient_dense_records (flc_avg_and_gradient_dense_records on lists, one C call), or None."""
    return _flcfold_entry(_PYGDRECS, "avg_and_gradient_dense_records")


def _pygsrecs():
    """_flcfold.avg_and_gradient_sparse_records (flc_avg_and_gradient_sparse_records on lists, one C call), or None."""
    return _flcfold_entry(_PYGSRECS, "avg_and_gradient_sparse_records")


def _pyflat():
    """_flcfold.delta_flat (a new flat delta, flc_delta_flatten, one C call), or None."""
    return _flcfold_entry(_PYFLAT, "delta_flat")


def _pyround():
    """_flcfold.stacked_records_round (the round's stacked encode into a record block, one Philox counter per
    message, the send counts made by the encode; one C call), or None."""
    return _flcfold_entry(_PYROUND, "stacked_records_round")


def _pydelta():
    """_flcfold.stacked_delta_record (the delta-fused stacked encode into a wire record and the send count, one C
    call), or None."""
    return _flcfold_entry(_PYDELTA, "stacked_delta_record")


def _pyef():
    """_flcfold.ef_accumulate (flc_ef_accumulate on lists of tensors, one C call), or None."""
    return _flcfold_entry(_PYEF, "ef_accumulate")


def model_fold_server(theta: Sequence[torch.Tensor], aux: Sequence[torch.Tensor],
                      srcs: Sequence[Sequence[torch.Tensor]], weights: Sequence[float], kind: str, fold: bool = True,
                      init_mode: int = 0, inertia: float = 0.0, c: float = 0.0) -> None:
    """FedDyn's / pFedMe's server update of a whole model in one launch (flc_model_fold_server): ``kind`` "feddyn"
    (aux = h; c = -mu / num_clients) or "pfedme" (aux = the saved model when ``fold`` is False; c = beta).  ``srcs[m]``
    is message m's tensor list, at most 16 messages; every tensor a contiguous fp32 tensor on theta's device."""
    import ctypes

    nt, ns = len(theta), len(srcs)
    if ns > MODEL_FOLD_MAX_SRC:
        raise ValueError(f"model_fold_server takes at most {MODEL_FOLD_MAX_SRC} messages")
    if len(aux) != nt or len(weights) != ns or any(len(m) != nt for m in srcs):
        raise ValueError("one aux tensor per model tensor, one weight per message, one tensor per model tensor each")
    if nt == 0:
        return
    f32, dev = torch.float32, theta[0].get_device()
    sizes = [t.numel() for t in theta]

    def ptrs(ts):
        out = []
        for t, n in zip(ts, sizes):
            if not (t.is_cuda and t.dtype is f32 and t.is_contiguous() and t.get_device() == dev and t.numel() == n):
                raise TypeError("model_fold_server: contiguous fp32 HIP tensors of the model's sizes on one device")
            out.append(t.data_ptr())
        return out

    sp = [q for m in srcs for q in ptrs(m)]
    P = ctypes.c_void_p
    vp = lambda a: ctypes.cast(a, P)  # noqa: E731
    call("flc_model_fold_server", vp((P * nt)(*ptrs(theta))), vp((P * nt)(*ptrs(aux))), vp((P * max(len(sp), 1))(*sp)),
         vp((ctypes.c_float * max(ns, 1))(*[float(w) for w in weights])), ns, vp((ctypes.c_int64 * nt)(*sizes)), nt,
         {"feddyn": _lib.FLC_SRV_FEDDYN, "pfedme": _lib.FLC_SRV_PFEDME}[kind], int(bool(fold)), int(init_mode),
         float(inertia), float(c), _stream(theta[0].device))


def model_fold(dsts: Sequence[torch.Tensor], srcs: Sequence[Sequence[torch.Tensor]], weights: Sequence[float],
               init_mode: int, beta: float = 0.0, theta: Optional[Sequence[torch.Tensor]] = None,
               v: Optional[Sequence[torch.Tensor]] = None, opt: str = "avg", lr: float = 1.0, beta2: float = 0.0,
               tau: float = 0.0) -> None:
    """A whole model in one launch (flc_model_fold): per tensor t, ``weighted_sum(dsts[t], [s[t] for s in srcs],
    weights, init_mode, beta)`` and, with ``theta``, ``fedopt_step(theta[t], dsts[t], v[t], opt, lr, beta2, tau)``.
    ``srcs[m]`` is message m's list of tensors (all on the dsts' device); at most 16 messages.  The checks are one
    lean pass per tensor: a model update is ~100 tensors, and per-tensor Python costs more than the kernel."""
    import ctypes

    nt, ns = len(dsts), len(srcs)
    pf = _pyfold()
    if pf is not None:  # every tensor checked in C before anything is launched; > 16 messages chained
        pf(dsts, srcs, None, weights, int(init_mode), float(beta), theta, v, _lib.FLC_OPT[opt], float(lr), float(beta2),
           float(tau))
        return
    if ns > MODEL_FOLD_MAX_SRC:
        raise ValueError(f"model_fold takes at most {MODEL_FOLD_MAX_SRC} messages")
    if nt == 0:
        return
    op = _model_fold_op()
    if op is not None:  # the checks and the pointer tables in C++ (torch_ops.cpp): one dispatcher call
        if any(len(msg) != nt for msg in srcs):
            raise ValueError("every message has one tensor per model tensor")
        if len(weights) != ns:
            raise ValueError("one weight per message")
        op(list(dsts), [t for msg in srcs for t in msg], [float(w) for w in weights], int(init_mode), float(beta),
           [] if theta is None else list(theta), [] if v is None else list(v), _lib.FLC_OPT[opt], float(lr),
           float(beta2), float(tau))
        return
    f32 = torch.float32
    dev = dsts[0].get_device()

    def ptrs(ts, what):
        out = []
        for t in ts:
            if not (t.is_cuda and t.dtype is f32 and t.is_contiguous() and t.get_device() == dev):
                raise TypeError(f"{what} tensors must be contiguous fp32 HIP tensors on one device")
            out.append(t.data_ptr())
        return out

    if len(weights) != ns:
        raise ValueError("one weight per message")
    sizes = [t.numel() for t in dsts]
    for what, ts in (("theta", theta), ("v", v)):
        if ts is not None and (len(ts) != nt or any(t.numel() != n for t, n in zip(ts, sizes))):
            raise ValueError(f"{what} must have one tensor per model tensor, of the model tensors' sizes")
    dp = ptrs(dsts, "model")
    sp = []
    for msg in srcs:
        if len(msg) != nt:
            raise ValueError("every message has one tensor per model tensor")
        for a, n in zip(msg, sizes):
            if a.numel() != n:
                raise ValueError("message tensors must match the model tensors' sizes")
        sp.extend(ptrs(msg, "message"))
    P = ctypes.c_void_p
    vp = lambda a: ctypes.cast(a, P)  # noqa: E731
    call("flc_model_fold", vp((P * nt)(*dp)), vp((P * max(len(sp), 1))(*sp)),
         vp((ctypes.c_float * max(ns, 1))(*weights)), ns, vp((ctypes.c_int64 * nt)(*sizes)), nt, int(init_mode),
         float(beta), None if theta is None else vp((P * nt)(*ptrs(theta, "model"))),
         None if v is None else vp((P * nt)(*ptrs(v, "model"))), _lib.FLC_OPT[opt], float(lr), float(beta2),
         float(tau), torch.cuda.current_stream(dev).cuda_stream)


def fedopt_step(theta: torch.Tensor, delta: torch.Tensor, v: Optional[torch.Tensor], opt: str, lr: float,
                beta2: float, tau: float) -> None:
    dt = theta.dtype
    for t, name in ((theta, "theta"), (delta, "delta"), (v, "v")):
        if t is None:
            continue
        if t.device.type != "cuda" or t.dtype != dt or dt not in (torch.float32, torch.float64) or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous HIP tensor of theta's dtype (fp32 or fp64)")
        if t.numel() != theta.numel():
            raise ValueError("theta, delta and v must have the same number of elements")
    call("flc_fedopt_step_f64" if dt == torch.float64 else "flc_fedopt_step", _p(theta), _p(delta), _p(v),
         theta.numel(), _lib.FLC_OPT[opt], float(lr), float(beta2), float(tau), _stream(theta.device))


def feddr_combine(theta: torch.Tensor, y: torch.Tensor, x_til: torch.Tensor, alpha: float, cx: float, cy: float,
                  prox: int, prox_c: float) -> None:
    """y = fmaf(alpha, theta - y, y); theta = prox(cx * x_til + cy * y), in place (flc_feddr_combine)."""
    dt = theta.dtype
    for t, name in ((theta, "theta"), (y, "y"), (x_til, "x_til")):
        if t.device.type != "cuda" or t.dtype != dt or dt not in (torch.float32, torch.float64) or not t.is_contiguous():
            raise TypeError(f"{name} must be a contiguous HIP tensor of theta's dtype (fp32 or fp64)")
        if t.numel() != theta.numel():
            raise ValueError("theta, y and x_til must have the same number of elements")
    call("flc_feddr_combine_f64" if dt == torch.float64 else "flc_feddr_combine", _p(theta), _p(y), _p(x_til),
         theta.numel(), float(alpha), float(cx), float(cy), int(prox), float(prox_c), _stream(theta.device))


def delta_flatten(local_params: Sequence[torch.Tensor], global_params: Sequence[torch.Tensor],
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The flat client delta ``cat([l - g for l, g in zip(local, global)])`` in one pass (flc_delta_flatten):
    FedOptClient.communicate's clone + ``add_(alpha=-1)`` (_fedopt.py:294-297) fused with the flatten the codec
    input needs.  Returns ``out`` (allocated when None)."""
    import ctypes

    ls = [_dev_f32(t, "local") for t in local_params]
    gs = [_dev_f32(t, "global") for t in global_params]
    if len(ls) != len(gs):
        raise ValueError("one global tensor per local tensor")
    for a, b in zip(ls, gs):
        if a.numel() != b.numel() or a.device != b.device:
            raise ValueError("local and global tensors must match in size and device")
    total = sum(t.numel() for t in ls)
    dev = ls[0].device if ls else (out.device if out is not None else torch.device("cuda"))
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    elif out.device.type != "cuda" or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != total:
        raise ValueError(f"out must be a contiguous fp32 HIP tensor of {total} elements")
    m = max(len(ls), 1)
    lp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in ls])
    gp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in gs])
    sz = (ctypes.c_int64 * m)(*[t.numel() for t in ls])
    call("flc_delta_flatten", ctypes.cast(lp, ctypes.c_void_p), ctypes.cast(gp, ctypes.c_void_p),
         ctypes.cast(sz, ctypes.c_void_p), len(ls), _p(out), _stream(dev))
    return out


# ---------------------------------------------------------------------------------------- error feedback
def _ef_memory(e: torch.Tensor, name: str = "e") -> torch.Tensor:
    """An error-feedback memory is written in place: a contiguous fp32 HIP tensor as it is (never a copy)."""
    if not isinstance(e, torch.Tensor) or e.device.type != "cuda" or e.dtype != torch.float32 or not e.is_contiguous():
        raise TypeError(f"{name} must be a contiguous float32 tensor on a HIP device")
    return e


def _ef_input(t: torch.Tensor, name: str) -> torch.Tensor:
    """A read-only operand of the feedback kernels: contiguous fp32 on a HIP device, any 4-B alignment."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise TypeError(f"{name} must be a torch tensor on a HIP device")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype}); the codec path is fp32")
    return t if t.is_contiguous() else t.contiguous()


def ef_accumulate(local_params: Sequence[torch.Tensor], global_params: Optional[Sequence[torch.Tensor]],
                  e: torch.Tensor) -> torch.Tensor:
    """``e += cat([l - g ...])`` in place (``global_params`` None: ``e += cat(local)``) — flc_ef_accumulate, the
    accumulate of an error-feedback message into the client's memory.  Returns ``e``."""
    import ctypes

    e = _ef_memory(e)
    ls = [_ef_input(t, "local") for t in local_params]
    gs = None if global_params is None else [_ef_input(t, "global") for t in global_params]
    if gs is not None and len(ls) != len(gs):
        raise ValueError("one global tensor per local tensor")
    for a, b in zip(ls, gs if gs is not None else ls):
        if a.numel() != b.numel() or a.device != e.device or b.device != e.device:
            raise ValueError("local and global tensors must match in size and lie on the memory's device")
    if sum(t.numel() for t in ls) != e.numel():
        raise ValueError(f"the memory holds {e.numel()} elements, the tensors {sum(t.numel() for t in ls)}")
    m = max(len(ls), 1)
    lp = (ctypes.c_void_p * m)(*[t.data_ptr() for t in ls])
    gp = None if gs is None else ctypes.cast((ctypes.c_void_p * m)(*[t.data_ptr() for t in gs]), ctypes.c_void_p)
    sz = (ctypes.c_int64 * m)(*[t.numel() for t in ls])
    with torch.cuda.device(e.device):
        call("flc_ef_accumulate", ctypes.cast(lp, ctypes.c_void_p), gp, ctypes.cast(sz, ctypes.c_void_p), len(ls),
             _p(e), _stream(e.device))
    return e


def ef_residual_round(records: Sequence[torch.Tensor], memories: Sequence[torch.Tensor], n: int, k: int,
                      levels: int) -> None:
    """``memories[c][idx] -= decode(records[c])`` at every record's kept entries, all clients in one launch
    (flc_ef_residual_round): the residual ``e' = a − c`` of a round's stacked records, ``a`` held in the memories."""
    import ctypes

    if len(records) != len(memories):
        raise ValueError("one memory per record")
    if not records:
        return
    dev = memories[0].device
    stride, _ = stacked_wire_layout(n, k) if k > 0 else (0, None)
    for r, e in zip(records, memories):
        _ef_memory(e, "a memory")
        if e.numel() != n or e.device != dev:
            raise ValueError(f"every memory holds n = {n} elements on one device")
        if r.dtype != torch.uint8 or r.device != dev or not r.is_contiguous() or r.numel() < stride:
            raise ValueError(f"a wire record is a contiguous uint8 tensor of at least {stride} bytes on the memories' "
                             "device")
    C = len(records)
    rp = (ctypes.c_void_p * C)(*[r.data_ptr() for r in records])
    ep = (ctypes.c_void_p * C)(*[e.data_ptr() for e in memories])
    with torch.cuda.device(dev):
        call("flc_ef_residual_round", ctypes.cast(rp, ctypes.c_void_p), ctypes.cast(ep, ctypes.c_void_p), C, int(n),
             int(k), int(levels), _stream(dev))


def ef_residual_sparse_round(records: Sequence[torch.Tensor], memories: Sequence[torch.Tensor], n: int, k: int) -> None:
    """``memories[c][idx] -= val`` at every sparse record's kept entries, all clients in one launch
    (flc_ef_residual_sparse_round): the residual ``e' = a − c`` of a round's top-k / rand-k records."""
    import ctypes

    if len(records) != len(memories):
        raise ValueError("one memory per record")
    if not records:
        return
    dev = memories[0].device
    stride, _ = sparse_wire_layout(n, k)
    for r, e in zip(records, memories):
        _ef_memory(e, "a memory")
        if e.numel() != n or e.device != dev:
            raise ValueError(f"every memory holds n = {n} elements on one device")
        if r.dtype != torch.uint8 or r.device != dev or not r.is_contiguous() or r.numel() < stride:
            raise ValueError(f"a wire record is a contiguous uint8 tensor of at least {stride} bytes on the memories' "
                             "device")
    C = len(records)
    rp = (ctypes.c_void_p * C)(*[r.data_ptr() for r in records])
    ep = (ctypes.c_void_p * C)(*[e.data_ptr() for e in memories])
    with torch.cuda.device(dev):
        call("flc_ef_residual_sparse_round", ctypes.cast(rp, ctypes.c_void_p), ctypes.cast(ep, ctypes.c_void_p), C,
             int(n), int(k), _stream(dev))


def ef_residual_dense(e: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """``e -= c`` in place (flc_ef_residual_dense): the residual of a message that carries its decoded flat vector."""
    e = _ef_memory(e)
    c = _ef_input(c, "c")
    if c.numel() != e.numel() or c.device != e.device:
        raise ValueError("c must hold the memory's element count on its device")
    with torch.cuda.device(e.device):
        call("flc_ef_residual_dense", _p(e), _p(c), e.numel(), _stream(e.device))
    return e


# ---------------------------------------------------------------------------------------- float64 inputs
# The reference runs every compressor on whatever dtype x has (compressors.py:267-410); these are the float64 forms
# (f64.hip): a float64 HIP vector in, a float64 HIP vector out.  Uniforms as for float32 (compat_u: one double per
# consumer in index order, else Philox at the element's index).
def _dev_f64(x: torch.Tensor, name: str = "x") -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise TypeError(f"{name} must be a torch tensor on a HIP device")
    if x.dtype != torch.float64:
        raise TypeError(f"{name} must be float64 (got {x.dtype})")
    x = x.reshape(-1)
    if not x.is_contiguous() or x.data_ptr() % 16 != 0:
        x = x.contiguous().clone()
    return x


def _ws64(x: torch.Tensor, k: int = 0) -> torch.Tensor:
    return workspace(x.device, _ws_size(x.device, "flc_f64_workspace_size", x.numel(), int(k)), "f64")


def copy_f64(x: torch.Tensor) -> torch.Tensor:
    x = _dev_f64(x)
    out = torch.empty_like(x)
    call("flc_copy_f64", _p(x), x.numel(), _p(out), _stream(x.device))
    return out


def scale_div_f64(x: torch.Tensor, p: float) -> torch.Tensor:
    x = _dev_f64(x)
    out = torch.empty_like(x)
    call("flc_scale_div_f64", _p(x), x.numel(), float(p), _p(out), _stream(x.device))
    return out


def randk_apply_f64(x: torch.Tensor, idx: torch.Tensor, scale: float) -> torch.Tensor:
    x = _dev_f64(x)
    idx = idx.to(device=x.device, dtype=torch.int32).contiguous()
    out = torch.empty_like(x)
    call("flc_randk_apply_f64", _p(x), x.numel(), _p(idx), idx.numel(), float(scale), _p(out), _stream(x.device))
    return out


def count_consumers_f64(x: torch.Tensor, norm: Optional[torch.Tensor]) -> torch.Tensor:
    """Device int64 scalar: the uniforms the reference draws (natural: norm None, x != 0; dithering: with the norm)."""
    x = _dev_f64(x)
    out = torch.empty(1, dtype=torch.int64, device=x.device)
    ws = _ws64(x)
    call("flc_count_consumers_f64", _p(x), x.numel(), _p(norm), _p(out), _p(ws), ws.numel(), _stream(x.device))
    return out


def natural_f64(x: torch.Tensor, seed: int = 0, counter: int = 0, compat_u: Optional[torch.Tensor] = None,
                want_codes: bool = False) -> Tuple[Optional[torch.Tensor], torch.Tensor]:
    """Natural compression of a float64 vector: (codes or None, decoded float64 vector)."""
    x = _dev_f64(x)
    n = x.numel()
    codes = torch.empty(n, dtype=torch.int16, device=x.device) if want_codes else None
    out = torch.empty_like(x)
    ws = _ws64(x)
    call("flc_natural_f64", _p(x), n, seed, counter, _p(compat_u), _p(codes), _p(out), _p(ws), ws.numel(),
         _stream(x.device))
    return codes, out


def natural_decode_f64(codes: torch.Tensor, n: int) -> torch.Tensor:
    out = torch.empty(n, dtype=torch.float64, device=codes.device)
    call("flc_natural_decode_f64", _p(codes), n, _p(out), _stream(out.device))
    return out


def quant_norm_f64(x: torch.Tensor, p: float = math.inf) -> torch.Tensor:
    x = _dev_f64(x)
    pk = _lib.FLC_NORM_INF if math.isinf(p) else (_lib.FLC_NORM_L2 if p == 2 else None)
    if pk is None:
        raise ValueError(f"p must be inf or 2 (got {p})")
    norm = torch.empty(1, dtype=torch.float64, device=x.device)
    ws = _ws64(x)
    call("flc_quant_norm_f64", _p(x), x.numel(), pk, _p(norm), _p(ws), ws.numel(), _stream(x.device))
    return norm


def quant_f64(x: torch.Tensor, kind: int, levels: int, norm: torch.Tensor, seed: int = 0, counter: int = 0,
              compat_u: Optional[torch.Tensor] = None, want_codes: bool = False, want_nnz: bool = False):
    """Standard / natural dithering of a float64 vector with the given float64 norm (a 1-element device tensor):
    (8-bit codes or None, decoded float64 vector, nnz or None)."""
    x = _dev_f64(x)
    n = x.numel()
    if norm.dtype != torch.float64 or norm.device != x.device:
        raise TypeError("norm must be a float64 tensor on x's device")
    if compat_u is not None and compat_u.dtype != torch.float64:
        raise TypeError("compat_u must be float64")
    codes = torch.empty(n, dtype=torch.uint8, device=x.device) if want_codes else None
    nnz = torch.empty(1, dtype=torch.int64, device=x.device) if want_nnz else None
    out = torch.empty_like(x)
    ws = _ws64(x)
    call("flc_quant_f64", _p(x), n, kind, levels, _p(norm), seed, counter, _p(compat_u), _p(codes), _p(out), _p(nnz),
         _p(ws), ws.numel(), _stream(x.device))
    return codes, out, nnz


def quant_decode_f64(codes: torch.Tensor, n: int, kind: int, levels: int, norm: torch.Tensor) -> torch.Tensor:
    out = torch.empty(n, dtype=torch.float64, device=codes.device)
    call("flc_quant_decode_f64", _p(codes), n, kind, levels, _p(norm), _p(out), _stream(out.device))
    return out


def topk_dense_f64(x: torch.Tensor, k: int, order=ORDER_SIGNED) -> torch.Tensor:
    """out = x on the k largest elements (ties: the highest indices), +0 elsewhere; 0 < k < n.  ``order``: as in
    :func:`topk_encode` (by magnitude: the k largest |x|)."""
    order = _order(order)
    x = _dev_f64(x)
    out = torch.empty_like(x)
    ws = _ws64(x, k)
    _call_ord("flc_topk_dense_f64", order, 2, _p(x), x.numel(), int(k), _p(out), _p(ws), ws.numel(), _stream(x.device))
    _after_encode(x.device, ("f64",))
    return out



def topk_stats_f64(x: torch.Tensor, k: int) -> dict:
    """What the last ``topk_dense_f64(x, k)`` on x's workspace did (flc_topk_stats_f64; synchronises the stream):
    ``fb`` (1: the K-th key came from the exact passes over x), ``err``, ``T``, ``need``, ``ties``, ``ithr``,
    ``nbin``, and that call's band geometry ``S``, ``r_lo``, ``r_hi``, ``on``, ``sample`` (the sample size cap)."""
    import ctypes

    x = x.reshape(-1)
    ws = _ws64(x, k)
    out = (ctypes.c_int64 * 16)()
    call("flc_topk_stats_f64", _p(ws), ws.numel(), x.numel(), int(k), out, _stream(x.device))
    names = ("fb", "err", "nbin", "T", "need", "ties", "ithr", "S", "r_lo", "r_hi", "on", "sample")
    d = {f: int(out[i]) for i, f in enumerate(names)}
    d["T"] &= (1 << 64) - 1
    return d
