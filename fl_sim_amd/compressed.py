"""The codec's call site: a FedOpt round whose client messages carry a compressed delta.

The reference never calls its compressors (``.coveragerc:16-17``; the only caller is
``test/test_compressors.py:12-15``), so the call site is new.  Its meaning is fixed by the round fixtures
(``tests/golden/gen_golden.py`` ``gen_round``), composed from the reference's own pieces:

* client — ``FedOptClient.communicate`` (``_fedopt.py:295-308``) forms ``delta_j = θ_local_j − θ_global_j``; the
  flattened delta goes through ``Compressor.compressVector`` (``compressors.py:267-410``): one compressor, or the
  stacked pipeline TopK then standard dithering (p = ∞) of the K-sparse result; the decoded vector, reshaped to the
  model's tensors, is the message's ``delta_parameters``;
* server — ``FedOptServer.update`` (``_fedopt.py:196-240``) folds the round.

What runs here instead:

* :class:`CompressedFedOptClientMixin` — ``communicate`` forms the delta on the device.  With the stacked pipeline the
  message carries the client's packed wire record (``flc_stacked_wire_layout``: 5 B per kept entry + tile pointers)
  instead of the dense delta; in philox mode the delta is formed inside the encoder's read
  (``flc_stacked_encode_delta``), in compat mode the pipeline is composed from the top-k encode and the dithering
  encode of the kept values with the interpreter's ``random`` stream, exactly as the reference consumes it.  Any other
  compressor runs through the drop-in ``Compressor`` on the device and the message carries the decoded delta —
  unless ``wire_records`` is on (looked up on the client, then on its config; ``wire=True`` on
  :func:`compress_delta` / :func:`compress_tensors`; off by default) and the compressor list is one float32 standard
  dithering (identical norm compressor), natural dithering or natural compressor (:func:`dense_wire_codec`): the
  message then carries the quantizer's own wire as a dense record (``flc_dense_wire_layout``: the fp32 norm and the
  packed 2-, 4- or 8-bit codes, or one uint16 per element), written by the compressor's encoder straight into the
  record with nothing decoded, the RNG streams and send statistics advancing as ``compressVector`` advances them.
  In philox mode a dithering quantizer's records of up to 2^20 elements (device norm, p = ∞ or 2; with error feedback
  only under ``FLC_EF_DENSE_DEFER=1``, :data:`EF_DENSE_DEFER`) are deferred like the stacked ones: the round's messages are encoded by one ``flc_quant_encode_round`` when a record
  or a statistic is first read (:func:`deferred_dense_stats` counts these batches).
  With ``sparse_records`` on (a switch of its own, looked up the same way; ``sparse=True`` on the three compress
  functions; off by default) a compressor list that is one float32 top-k or rand-k compressor with 0 < K < n whose
  record is smaller than 4·n bytes (:func:`sparse_wire_codec`) sends its sparse record (``flc_sparse_wire_layout``:
  the ascending kept indices, their decoded fp32 values — rand-k's already ``D / K · x`` — and the tile pointers: 8 B
  per kept entry), written by ``flc_topk_encode_tiled`` (rand-k: the index set as today — the reference's ``np.random``
  shuffle prefix sorted on the host, or the K largest Philox keys — then ``flc_sparse_gather``), the RNG streams and
  send statistics advancing as ``compressVector`` advances them.  Top-k draws no random numbers, so in any
  ``rng_mode`` its records of up to 2^24 elements are deferred: one ``flc_topk_encode_batch`` writes the round's
  records (:func:`deferred_sparse_stats` counts these batches); rand-k encodes at once.
  Either way ``delta_parameters`` is a :class:`CompressedDelta`: a sequence of per-tensor tensors that decodes itself
  on first access, so any server — the reference's own ``update`` included — reads it unchanged.
* ``aggregation.fedopt_update`` (and :class:`~fl_sim_amd.aggregation.FedOptUpdateMixin`) recognises a round of stacked
  records and runs :func:`fold_records`: ONE launch per 64 clients decodes every record, folds it into δ in message
  order and applies the server optimiser's step (``flc_fedopt_fold_records``) — the records are read once, δ, θ (and
  v) read and written once; bit-identical to decoding each record and running the reference's update.  A round of
  dense records of one (n, format, levels, bits) (:func:`dense_record_round`) takes the same functions
  (``flc_fedopt_fold_dense_records``; for SCAFFOLD and IFCA ``flc_fold_dense_record_groups``): the server reads the
  codes, 1/4 to 1/16 of the dense bytes; the variance-reduced servers' ``gradients`` as dense records take
  ``flc_avg_and_gradient_dense_records``.  A round of sparse records of one (n, k) (:func:`sparse_round`) takes them
  too (``flc_fedopt_fold_sparse_records``, ``flc_fold_sparse_record_groups``, and for the variance-reduced servers'
  ``gradients`` ``flc_avg_and_gradient_sparse_records``).  A mixed round reads each message as its decoded tensors —
  unless ``FLC_MIXED_FOLD=1`` (:data:`MIXED_FOLD`, off by default): then a round whose messages differ in codec, one
  decoded vector among them included (:func:`mixed_round`), is folded in one pass with every record read by its own
  descriptor (``flc_fedopt_fold_mixed_records``, ``flc_fold_mixed_record_groups``,
  ``flc_avg_and_gradient_mixed_records``), on device-resident servers.
  The folds are written once per server form — :func:`fold_records` (FedOpt), :func:`fold_gradient_records` (the
  variance-reduced servers), :func:`fold_record_groups` (SCAFFOLD, IFCA) — and each serves every kind of round:
  :func:`record_round` and its three parts are one classifier (one of these kinds, one ``codec_key``),
  ``_record_entries`` is the one place that knows a uniform kind's shape arguments, C names and one-call ``_flcfold``
  entries, ``_server_ok`` the one check of the server tensors, and ``mixed=True`` (the ``fold_mixed_*`` names) swaps
  the kind's shape for the per-record descriptor columns of ``_mixed_tables``.

The compressors' send statistics advance as ``compressVector`` advances them (``compressors.py:406-408``), per stage.

The variance-reduced algorithms (FedProx, FedPD, ProxSkip, pFedMac with ``config.vr``) send ``parameters`` and
``gradients`` (fedprox/_fedprox.py:208-217, fedpd/_fedpd.py:252-275, proxskip/_proxskip.py:265-276,
pfedmac/_pfedmac.py:203-212).  Their call site compresses the gradients only — the stochastic half of the message, and
the one whose server fold starts from +0 (``tests/golden/gen_golden_vr_codec.py`` fixes the meaning the same way):

* :class:`CompressedGradientsClientMixin` — runs the client's own ``communicate`` and sends the ``gradients`` of the
  message it appended through :func:`compress_tensors` (everything :func:`compress_delta` does, nothing subtracted);
* ``aggregation.avg_parameters_and_gradients`` / ``update_gradients`` (and the ``VRUpdateMixin`` family) recognise a
  round of stacked, dense or sparse records (:func:`record_round`) and run :func:`fold_gradient_records`: every record
  decoded and folded into the gradients and the dense parameters folded into the model in one
  ``flc_avg_and_gradient_records`` pass (``flc_avg_and_gradient_dense_records`` /
  ``flc_avg_and_gradient_sparse_records`` by the records' kind).

SCAFFOLD and IFCA send deltas (scaffold/_scaffold.py:210-222: ``parameters_delta`` and ``control_variates_delta``;
ifca/_ifca.py:228-240: ``delta_parameters`` and a ``cluster_id``), and their servers accumulate each message in place
into one of several destinations (θ and c; the message's cluster centre):

* :class:`CompressedSCAFFOLDClientMixin` / :class:`CompressedIFCAClientMixin` — ``communicate`` with every delta sent
  through :func:`compress_delta` (``tests/golden/gen_golden_delta_codec.py`` fixes the meaning);
* ``aggregation.scaffold_update`` / ``ifca_update`` recognise a round of stacked records and run
  :func:`fold_record_groups`: every destination's records decoded and folded in ONE ``flc_fold_record_groups`` pass
  (grid = tiles × groups).

Error feedback (``fl_sim_amd/feedback.py``; ``tests/golden/gen_golden_ef.py`` fixes the meaning): with
``error_feedback`` truthy on the client or its config, every client mixin keeps one
:class:`~fl_sim_amd.feedback.ErrorMemory` ``e`` per message vector (``client.error_memory(key)``) and sends the message
of ``a = e + (local − cached)``; the memory takes ``a − c``.  :func:`compress_delta` / :func:`compress_tensors` take
the memory as ``feedback=``: ``flc_ef_accumulate`` writes ``a`` into it in place, the memory tensor is the deferred
batch item's flat input (no snapshot), and after the batch's ``flc_stacked_encode_round`` has succeeded one
``flc_ef_residual_round`` subtracts what the round's records carry at their K kept entries (a batch whose encode raised
stays pending with its memories holding ``a``; a memory still waiting in a batch when its client communicates again
has that batch run first).  The immediate stacked paths encode the memory and run the residual with one client; any
other compressor chain runs on the memory's values, then ``flc_ef_residual_dense`` (with ``wire`` on, on the decoded
dense record, which the message does not keep — or, with ``FLC_EF_DENSE_DEFER=1`` (:data:`EF_DENSE_DEFER`, off by
default), a dithering quantizer's dense-record message waits in the round's batch with the memory as its flat input and
one ``flc_quant_encode_residual_round`` writes the records and the residuals in the encode's own pass).  A sparse record's residual is K entries too
(``flc_ef_residual_sparse_round``: once per deferred batch after its encode succeeded, with one client on the immediate
paths).  ``feedback=None`` is the path above, untouched.
"""

from __future__ import annotations

import collections.abc as _abc
import ctypes
import functools
import math
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, codec
from ._lib import FLC_NORM_INF, FLC_NORM_L2, FLC_Q_NATURAL_DITHER, FLC_Q_STANDARD_DITHER, FLC_WIRE_NATURAL
from . import rng as _rng
from .compressors import Compressor, CompressorType
from .feedback import ErrorFeedbackClientMixin, ErrorMemory


_MSG_CLS: list = []


def client_message_class():
    """The reference's ``ClientMessage`` (nodes.py:1537-1557) when ``fl_sim`` is importable (``Server._update``
    asserts the type, nodes.py:767-770), else a dict subclass with the same constructor.  Looked up once per process
    (a failing import costs ~80 us, and ``communicate`` runs once per client per round)."""
    if not _MSG_CLS:
        try:
            from fl_sim.nodes import ClientMessage as ref_cls  # type: ignore
        except Exception:  # fl_sim absent (or its dependencies: torch_ecg, ...)
            ref_cls = ClientMessage
        _MSG_CLS.append(ref_cls)
    return _MSG_CLS[0]


class ClientMessage(dict):
    """Stand-in for the reference's ``ClientMessage`` (nodes.py:1537-1557) when ``fl_sim`` is not importable."""

    __name__ = "ClientMessage"

    def __init__(self, client_id: int, train_samples: int, metrics: dict, **kwargs) -> None:
        super().__init__(client_id=client_id, train_samples=train_samples, metrics=metrics, **kwargs)


class CompressedDelta(_abc.Sequence):
    """A client's compressed model delta as its message carries it.

    ``kind == "stacked"``: the packed wire record of the stacked codec (top-k ascending int32 indices, 8-bit
    sign | level codes, the kept set's norm, tile pointers); ``kind == "sparse"`` (``sparse=True``): the sparse record
    of a top-k or rand-k compressor (ascending int32 indices, the decoded fp32 values, tile pointers); ``kind == "quant"`` / ``"natural"`` (``wire=True``): the
    dense record of a dithering quantizer (its norm and packed ``bits``-bit codes) or of the natural compressor (one
    uint16 per element), ``format`` being flc_dense_wire_layout's; ``kind == "bucket"`` (``wire=True`` with a bucket
    size): the bucket record of a bucketed dithering quantizer (one norm per ``bucket`` elements, then the packed codes;
    flc_bucket_wire_layout); ``kind == "dense"``: the decoded flat delta.
    Indexing gives tensor ``j`` of the model's shapes (the decoded values, one flat decode on first access), so code
    written for a list of delta tensors reads it unchanged."""

    def __init__(self, shapes: Sequence[torch.Size], device: torch.device, n: int, *, record=None, k: int = 0,
                 levels: int = 0, flat: Optional[torch.Tensor] = None, batch: Optional["_Batch"] = None,
                 format: Optional[int] = None, bits: int = 0, sparse: bool = False, bucket: int = 0):
        self.shapes = [torch.Size(s) for s in shapes]
        self.device = device
        self.n = int(n)
        self._record, self.k, self.levels = record, int(k), int(levels)
        self._batch = batch  # (a deferred encode: the record is made by the batch's launch on first access)
        self.format, self.bits = format, int(bits)
        self.bucket = int(bucket)  # a bucket record's bucket size (flc_bucket_wire_layout), else 0
        if format is not None and self.bucket:
            self.kind = "bucket"
        elif format is not None:
            self.kind = "natural" if format == FLC_WIRE_NATURAL else "quant"
        elif sparse:  # (a top-k / rand-k record, flc_sparse_wire_layout(n, k): levels 0, no format)
            self.kind = "sparse"
        else:
            self.kind = "stacked" if record is not None or batch is not None else "dense"
        self._flat = flat
        self._views: Optional[List[torch.Tensor]] = None

    @property
    def record(self) -> Optional[torch.Tensor]:
        """The packed wire record (stacked, sparse, quant, natural), or None (dense)."""
        if self._batch is not None:
            self._batch.run()
        return self._record

    @property
    def codec_key(self) -> tuple:
        """What a round's records must share to be folded together."""
        return (self.kind, self.n, self.k, self.levels, self.format, self.bits, self.bucket)

    def __getstate__(self):
        """A copied or pickled message carries its record (a deferred encode runs first); a dense record travels
        without the decoded vector, which the copy decodes again when it is read."""
        if self._batch is not None:
            self._batch.run()
        d = self.__dict__.copy()
        d["_batch"] = None
        if self.kind in ("quant", "natural", "bucket"):
            d["_flat"] = d["_views"] = None
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.__dict__.setdefault("bucket", 0)  # (a delta pickled before bucket records existed)

    @property
    def nbytes(self) -> int:
        """Bytes the message carries for the delta (the wire record, or the dense fp32 vector)."""
        return int(self.record.numel()) if self.record is not None else 4 * self.n

    def flat(self) -> torch.Tensor:
        """The decoded flat delta (flc_stacked_decode_tiled, flc_sparse_decode_tiled, flc_quant_decode or
        flc_natural_decode of the record, once)."""
        if self._flat is None:
            if self.kind == "bucket":
                self._flat = codec.bucket_decode(self.record, self.n, self.format, self.levels, self.bits, self.bucket)
            elif self.kind in ("quant", "natural"):
                self._flat = codec.dense_record_decode(self.record, self.n, self.format, self.levels, self.bits)
            elif self.kind == "sparse":
                self._flat = codec.sparse_record_decode(self.record, self.n, self.k)
            else:
                self._flat = codec.stacked_decode(codec.wire_packet(self.record, self.n, self.k, self.levels))
        return self._flat

    def tensors(self) -> List[torch.Tensor]:
        if self._views is None:
            f, out, off = self.flat(), [], 0
            for s in self.shapes:
                m = s.numel()
                out.append(f[off:off + m].view(s))
                off += m
            self._views = out
        return self._views

    def __len__(self) -> int:
        return len(self.shapes)

    def __getitem__(self, j):
        return self.tensors()[j]

    def __iter__(self):
        return iter(self.tensors())


def stacked_pipeline(compressors: Sequence[Compressor]) -> Optional[Tuple[int, int]]:
    """(K, levels) when ``compressors`` is the stacked pipeline the packed wire carries: a TopK compressor, then a
    float32 standard-dithering compressor with p = ∞ and 1..127 levels; else None."""
    if len(compressors) != 2:
        return None
    tk, sd = compressors
    if not (isinstance(tk, Compressor) and isinstance(sd, Compressor)):
        return None
    if tk.compressorType != CompressorType.TOPK_COMPRESSOR:
        return None
    if sd.compressorType != CompressorType.STANDARD_DITHERING_FP32 or not math.isinf(sd.p) or not 1 <= sd.s <= 127:
        return None
    return int(tk.K), int(sd.s)


def pipeline_order(compressors: Sequence[Compressor]) -> int:
    """The selection order (``codec.ORDER_*``) a compressor list's top-k stage runs in: ``codec.ORDER_MAGNITUDE`` when
    its first compressor is a top-k made with ``magnitude=True`` — alone, or heading the stacked pipeline of
    :func:`stacked_pipeline` — else ``codec.ORDER_SIGNED`` (the reference's rule, compressors.py:293-296).  The order
    changes which entries a record holds, never the record: layouts, folds and residuals are the same."""
    if not compressors:
        return codec.ORDER_SIGNED
    tk = compressors[0]
    if isinstance(tk, Compressor) and tk.compressorType == CompressorType.TOPK_COMPRESSOR and tk.magnitude:
        return codec.ORDER_MAGNITUDE
    return codec.ORDER_SIGNED


def _ptrs(ts: Sequence[torch.Tensor]):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _fp32_on(ts: Sequence[torch.Tensor], dev: torch.device) -> List[torch.Tensor]:
    out = []
    for t in ts:
        t = t.detach()
        if t.device != dev:
            t = t.to(dev)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 4:
            t = t.contiguous().float()
        out.append(t)
    return out


def _norm_kind(p) -> Optional[int]:
    """The device norm of a dithering compressor's ``p``: FLC_NORM_INF, FLC_NORM_L2, or None (any other p)."""
    return FLC_NORM_INF if math.isinf(p) else (FLC_NORM_L2 if p == 2 else None)


@functools.lru_cache(maxsize=None)
def _code_fraction(s: int):
    """What one dithered element adds to the send count, in fp32 elements: its sign and one of ``s`` levels in
    1 + ceil(log2 s) of 32 bits (compressors.py:365 / 404).  Remembered per ``s``: it is asked once per message, and
    numpy's ceil of a scalar costs more than the rest of the enqueue."""
    return (1.0 + np.ceil(math.log2(s))) / 32.0


def _norm_stage_send(sd: Compressor, norm: torch.Tensor) -> float:
    """The norm compressor's pass over the one-element norm vector (compressors.py:334-337) and the send count it
    contributes; an identical norm compressor (the reference's usual one) is advanced without reading the norm back."""
    nc = sd.vectorNormCompressor
    if _identical(nc):
        nc._finish(1, 1)
    else:
        nc.compressVector(np.array([np.float32(norm.item())]))
    return nc.last_need_to_send_advance


def compress_delta(local: Sequence[torch.Tensor], cached: Sequence[torch.Tensor],
                   compressors: Sequence[Compressor], feedback: Optional[ErrorMemory] = None,
                   wire: bool = False, sparse: bool = False, bucket: int = 0) -> CompressedDelta:
    """The client's compressed delta ``compressors(cat(local − cached))`` (see the module docstring); every compressor's
    RNG stream and send statistics advance as its own ``compressVector`` call would advance them.  ``feedback``: the
    client's :class:`~fl_sim_amd.feedback.ErrorMemory` ``e`` for this vector — the message is then that of the input
    ``a = e + (local − cached)`` and the memory takes ``a − c`` (error feedback; None: nothing remembered).  ``wire``:
    one float32 dithering quantizer or natural compressor (:func:`dense_wire_codec`) sends its dense record — the norm
    and the packed codes — instead of the decoded vector; any other compressor list is sent as without it.  ``sparse``:
    one top-k or rand-k compressor (:func:`sparse_wire_codec`) sends its sparse record — the kept indices, their decoded
    values and the tile pointers — instead of the decoded vector; any other compressor list is sent as without it.
    ``bucket`` (a power of two in [64, 4096]; 0: the compressor's own ``bucket``): a float32 dithering quantizer
    quantizes every ``bucket`` consecutive elements under that bucket's own norm (``Compressor.bucket``); with ``wire``
    the message carries the bucket record (``kind == "bucket"``), without it the decoded vector."""
    if feedback is not None:
        return _compress_feedback(list(local), cached, compressors, feedback, wire, sparse, bucket)
    return _compress(list(local), cached, compressors, wire, sparse, bucket)


def compress_tensors(tensors: Sequence[torch.Tensor], compressors: Sequence[Compressor],
                     feedback: Optional[ErrorMemory] = None, wire: bool = False,
                     sparse: bool = False, bucket: int = 0) -> CompressedDelta:
    """``compressors(cat(tensors))`` — :func:`compress_delta` with nothing subtracted (a client's gradient list): the
    stacked pipeline gives a packed record, any other compressor the decoded flat vector (``wire``: a dithering
    quantizer's or the natural compressor's dense record; ``sparse``: a top-k or rand-k compressor's sparse record);
    the compressors' RNG streams
    and send statistics advance alike, and in philox mode a deferred message joins the round's batched encode with the
    flat vector as its snapshot.  ``feedback``: as for :func:`compress_delta` (``a = e + cat(tensors)``); ``bucket``
    likewise."""
    if feedback is not None:
        return _compress_feedback(list(tensors), None, compressors, feedback, wire, sparse, bucket)
    return _compress(list(tensors), None, compressors, wire, sparse, bucket)


def dense_wire_codec(compressors: Sequence[Compressor]) -> Optional[Tuple[int, int, int]]:
    """(format, levels, bits) of the dense record ``compressors`` sends with ``wire`` on — one float32 compressor:
    standard dithering with an identical norm compressor and 1..127 levels, natural dithering with 1..127 levels (the
    code width is ``codec.code_bits(s)``; any p), or the natural compressor (uint16 codes) — else None."""
    if len(compressors) != 1 or not isinstance(compressors[0], Compressor):
        return None
    c = compressors[0]
    t = c.compressorType
    if t == CompressorType.NATURAL_COMPRESSOR_FP32:
        return FLC_WIRE_NATURAL, 0, 16
    if t == CompressorType.STANDARD_DITHERING_FP32:
        if not (_identical(c.vectorNormCompressor) and 1 <= c.s <= 127):
            return None
        return FLC_Q_STANDARD_DITHER, int(c.s), codec.code_bits(int(c.s))
    if t == CompressorType.NATURAL_DITHERING_FP32 and 1 <= c.s <= 127:
        return FLC_Q_NATURAL_DITHER, int(c.s), codec.code_bits(int(c.s))
    return None


def _dense_record(x: torch.Tensor, shapes, n: int, comp: Compressor, dc: Tuple[int, int, int], dev) -> CompressedDelta:
    """The dense record of the flat fp32 vector ``x`` under ``comp``: the codes written straight into the record by the
    compressor's own encoder, nothing decoded.  The RNG streams and send statistics advance exactly as
    ``comp.compressVector(x)`` advances them (compressors.py:302-325, 327-404): compat mode draws the interpreter's
    ``random`` stream for the consuming elements; philox mode takes one ``philox.next()`` and leaves a standard
    dithering's nonzero count in the compressor's pending slab, so nothing synchronises."""
    fmt, s, bits = dc
    x = codec._dev_f32(x).reshape(-1)
    stride, _ = codec.dense_wire_layout(n, fmt, bits)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    norm, codes = codec.dense_wire_views(rec, n, fmt, bits)
    st = codec._stream(dev)
    compat = comp.rng_mode == "compat"
    if fmt == FLC_WIRE_NATURAL:
        seed, ctr = comp.philox.next()
        u = None
        if compat:
            u = comp._uniforms(int(codec.count_consumers(x.reshape(1, n), None).item()), dev)
        ws = codec.workspace(dev, codec._ws_size(dev, "flc_natural_workspace_size", n), "natural")
        _lib.call("flc_natural_encode", x.data_ptr(), n, seed, ctr, codec._p(u), codes.data_ptr(), None, ws.data_ptr(),
                  ws.numel(), st)
        comp._finish(n, 9.0 / 32.0 * n)  # compressors.py:325
        return CompressedDelta(shapes, dev, n, record=rec, levels=0, format=fmt, bits=bits)
    std = fmt == FLC_Q_STANDARD_DITHER
    per = _code_fraction(s)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", 1, n), "quant")
    host_norm = None
    if comp._wants_host_norm(device_input=True):  # the reference's np.linalg.norm (compressors.py:332 / 372)
        host_norm = comp._reference_norm(x.detach().cpu().numpy())
        norm.copy_(torch.tensor([host_norm], dtype=torch.float32), non_blocking=True)
    seed, ctr = comp.philox.next()
    if not compat:
        cnt = comp._count_slot(dev) if std else None
        if host_norm is None:  # norm and encode together (the record's norm field is the encode's norms output)
            pk = _norm_kind(comp.p)
            if pk is None:
                raise ValueError(f"p must be inf or 2 (got {comp.p})")
            _lib.call("flc_quant_encode_auto", x.data_ptr(), 1, n, fmt, s, bits, pk, seed, ctr, codes.data_ptr(),
                      norm.data_ptr(), codec._p(cnt), None, ws.data_ptr(), ws.numel(), st)
            codec._after_encode(dev, ("quant",))
        else:
            _lib.call("flc_quant_encode", x.data_ptr(), 1, n, fmt, s, bits, norm.data_ptr(), seed, ctr, None,
                      codes.data_ptr(), codec._p(cnt), ws.data_ptr(), ws.numel(), st)
        if std:
            comp._finish_pending(n, cnt, _norm_stage_send(comp, None), per)
        else:
            comp._finish(n, n * per)
        return CompressedDelta(shapes, dev, n, record=rec, levels=s, format=fmt, bits=bits)
    if host_norm is None:
        pk = _norm_kind(comp.p)
        if pk is None:
            raise ValueError(f"p must be inf or 2 (got {comp.p})")
        _lib.call("flc_quant_norm", x.data_ptr(), 1, n, pk, norm.data_ptr(), ws.data_ptr(), ws.numel(), st)
    consumers = int(codec.count_consumers(x.reshape(1, n), norm).item())
    comp._check_bracket(float(norm.item()), consumers)
    u = comp._uniforms(consumers, dev)
    nnz = torch.empty(1, dtype=torch.int64, device=dev) if std else None
    _lib.call("flc_quant_encode", x.data_ptr(), 1, n, fmt, s, bits, norm.data_ptr(), seed, ctr, u.data_ptr(),
              codes.data_ptr(), codec._p(nnz), ws.data_ptr(), ws.numel(), st)
    if std:
        base = _norm_stage_send(comp, None)
        nz = int(nnz.item())
        comp._finish(n, base + nz * per if nz else base)
    else:
        comp._finish(n, n * per)
    return CompressedDelta(shapes, dev, n, record=rec, levels=s, format=fmt, bits=bits)


_DITHER_F32 = (CompressorType.STANDARD_DITHERING_FP32, CompressorType.NATURAL_DITHERING_FP32)


def _bucket_of(compressors: Sequence[Compressor], bucket: int) -> int:
    """The bucket size a message of ``compressors`` is quantized with: ``bucket`` (the client's ``quant_bucket``), or
    the one compressor's own ``bucket``; 0 unless the list is one float32 dithering quantizer."""
    if len(compressors) != 1 or not isinstance(compressors[0], Compressor):
        return 0
    c = compressors[0]
    if c.compressorType not in _DITHER_F32:
        return 0
    B = int(bucket or c.bucket or 0)
    if B and B not in codec.BUCKET_SIZES:
        raise ValueError(f"bucket must be 0 or a power of two in [64, 4096] (got {B})")
    return B


class _bucketed:
    """``comp.bucket = B`` for the length of a ``compressVector`` call (the message's bucket size on a compressor
    whose own is another)."""

    def __init__(self, comp: Compressor, B: int):
        self.comp, self.B = comp, B

    def __enter__(self):
        self.old = self.comp.bucket
        self.comp.bucket = self.B

    def __exit__(self, *exc):
        self.comp.bucket = self.old


def _bucket_stats(comp: Compressor, n: int, B: int, std: bool, cnt) -> None:
    """The send statistics of the slice-wise compressVector calls (Compressor._compress_bucketed's), with a standard
    dithering's nonzero count still on the device in ``cnt``: nb norms through the identical norm compressor, then one
    code fraction per nonzero element; natural dithering: n code fractions."""
    per = _code_fraction(comp.s)
    if not std:
        comp._finish(n, n * per)
        return
    nb = -(-n // B)
    nc = comp.vectorNormCompressor
    nc.last_input_advance = 1
    nc.last_need_to_send_advance = 1
    nc.total_input_components += nb
    nc.really_need_to_send_components += nb
    comp._finish_pending(n, cnt, nb, per)


def _bucket_record(x: torch.Tensor, shapes, n: int, comp: Compressor, dc: Tuple[int, int, int], B: int,
                   dev) -> CompressedDelta:
    """The bucket record of the flat fp32 vector ``x`` under ``comp`` with bucket size ``B``, encoded at once.  Philox
    mode: one flc_bucket_encode (the norms from the device, or — ``norm_mode`` "reference" — the host's per-slice
    ``np.linalg.norm``), the nonzero count left in the compressor's pending slab.  Compat mode: the existing per-row
    entry points over the ``[n // B, B]`` head and the tail, as ``Compressor._compress_bucketed`` composes them, with
    flc_quant_encode writing each piece's codes at its place in the record's code stream (a whole bucket's codes start
    16-B aligned) and the interpreter's draws consumed in index order."""
    fmt, s, bits = dc
    x = codec._dev_f32(x).reshape(-1)
    std = fmt == FLC_Q_STANDARD_DITHER
    if comp.rng_mode == "philox":
        pk = _norm_kind(comp.p)
        if pk is None:
            raise ValueError(f"p must be inf or 2 (got {comp.p})")
        given = None
        if comp._wants_host_norm(device_input=True):
            with _bucketed(comp, B):
                given = torch.from_numpy(comp._reference_norm(x.detach().cpu().numpy())).to(dev)
        seed, ctr = comp.philox.next()
        cnt = comp._count_slot(dev) if std else None
        stride, _ = codec.bucket_wire_layout(n, fmt, bits, B)
        rec = torch.empty(stride, dtype=torch.uint8, device=dev)
        nv, cv = codec.bucket_wire_views(rec, n, fmt, bits, B)
        if given is not None:
            nv.copy_(given)
        _lib.call("flc_bucket_encode", x.data_ptr(), n, fmt, s, bits, B, pk, int(given is not None), seed, ctr,
                  nv.data_ptr(), cv.data_ptr(), codec._p(cnt), None, codec._stream(dev))
        _bucket_stats(comp, n, B, std, cnt)
        return CompressedDelta(shapes, dev, n, record=rec, levels=s, format=fmt, bits=bits, bucket=B)
    pk = _norm_kind(comp.p)
    given = None
    if comp._wants_host_norm(device_input=True):
        with _bucketed(comp, B):
            given = torch.from_numpy(comp._reference_norm(x.detach().cpu().numpy())).to(dev)
    elif pk is None:
        raise ValueError(f"p must be inf or 2 (got {comp.p})")
    seed, ctr = comp.philox.next()
    stride, _ = codec.bucket_wire_layout(n, fmt, bits, B)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    nv, cv = codec.bucket_wire_views(rec, n, fmt, bits, B)
    if given is not None:
        nv.copy_(given)
    st = codec._stream(dev)
    pieces = [(lo, min(65535, n // B - lo // B), B) for lo in range(0, (n // B) * B, 65535 * B)]
    if n % B:
        pieces.append(((n // B) * B, 1, n % B))
    nnz_total = 0
    for lo, rows, d in pieces:
        x2 = x[lo:lo + rows * d].reshape(rows, d)
        nrm = nv[lo // B:lo // B + rows]
        ws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", rows, d), "quant")
        if given is None:
            _lib.call("flc_quant_norm", x2.data_ptr(), rows, d, pk, nrm.data_ptr(), ws.data_ptr(), ws.numel(), st)
        consumers = int(codec.count_consumers(x2, nrm).item())
        for r in (nrm == 0).nonzero().reshape(-1).tolist():  # (a p = 2 norm that underflowed: the reference fails)
            comp._check_bracket(0.0, int(torch.count_nonzero(x2[r]).item()))
        u = comp._uniforms(consumers, dev)
        nnz = torch.empty(rows, dtype=torch.int64, device=dev) if std else None
        _lib.call("flc_quant_encode", x2.data_ptr(), rows, d, fmt, s, bits, nrm.data_ptr(), seed, ctr, u.data_ptr(),
                  cv.data_ptr() + lo * bits // 8, codec._p(nnz), ws.data_ptr(), ws.numel(), st)
        if std:
            nnz_total += int(nnz.sum().item())
    per = _code_fraction(s)
    if std:
        nb = -(-n // B)
        nc = comp.vectorNormCompressor
        nc.last_input_advance = 1
        nc.last_need_to_send_advance = 1
        nc.total_input_components += nb
        nc.really_need_to_send_components += nb
        comp._finish(n, nb + nnz_total * per)
    else:
        comp._finish(n, n * per)
    return CompressedDelta(shapes, dev, n, record=rec, levels=s, format=fmt, bits=bits, bucket=B)


def sparse_wire_codec(compressors: Sequence[Compressor], n: Optional[int] = None) -> Optional[int]:
    """``K`` of the sparse record ``compressors`` sends with ``sparse`` on for a float32 vector of ``n`` elements
    (default: the compressor's own ``D``) — one top-k or rand-k compressor (compressors.py:284-296) with 0 < K < n (a
    rand-k: built for that n) whose record, ``flc_sparse_wire_layout(n, K)``, is smaller than the vector's 4·n bytes —
    else None: the message is then sent as without the option (a top-k with K <= 0 or K >= n copies,
    compressors.py:293-296)."""
    if len(compressors) != 1 or not isinstance(compressors[0], Compressor):
        return None
    c = compressors[0]
    t = c.compressorType
    if t not in (CompressorType.TOPK_COMPRESSOR, CompressorType.RANDK_COMPRESSOR):
        return None
    if n is None:
        n = getattr(c, "D", None)
    try:
        n, K = int(n), int(c.K)
    except (TypeError, ValueError):
        return None
    if K != c.K or not 0 < K < n or n >= 1 << 31:
        return None
    if t == CompressorType.RANDK_COMPRESSOR and int(c.D) != n:
        return None
    if codec.sparse_wire_layout(n, K)[0] >= 4 * n:
        return None
    return K


def _all_f32(local, cached) -> bool:
    """Every tensor of the message is float32 (the sparse record is the float32 form: a float64 model keeps today's
    message)."""
    return all(t.dtype is torch.float32 for t in local) and (
        cached is None or all(t.dtype is torch.float32 for t in cached))


def _sparse_record(x: torch.Tensor, shapes, n: int, comp: Compressor, K: int, dev) -> CompressedDelta:
    """The sparse record of the flat fp32 vector ``x`` under the top-k or rand-k compressor ``comp``, written by the
    encoders straight into the record, nothing decoded.  The RNG streams and send statistics advance exactly as
    ``comp.compressVector(x)`` advances them (compressors.py:284-296): top-k draws nothing; rand-k takes the
    reference's ``np.random`` shuffle prefix (compat; sorted ascending on the host — the indices are unique, so the
    decoded vector does not depend on their order) or one ``philox.next()`` (the K largest Philox keys, ascending,
    with their tile pointers), then ``flc_sparse_gather`` writes ``fp32(D / K) * x[idx]``."""
    x = codec._dev_f32(x).reshape(-1)
    stride, _ = codec.sparse_wire_layout(n, K)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    if comp.compressorType == CompressorType.TOPK_COMPRESSOR:
        codec.topk_encode_record(x, K, rec, order=comp.order)  # compressors.py:293-296 (or by magnitude)
        comp._finish(n, comp.K)
        return CompressedDelta(shapes, dev, n, record=rec, k=K, sparse=True)
    idx, val, tiles = codec.sparse_wire_views(rec, n, K)
    st = codec._stream(dev)
    if comp.rng_mode == "compat":  # compressors.py:285-288: the reference's own permutation, on the host
        S = np.sort(_rng.numpy_shuffle_prefix(comp.D, comp.K)).astype(np.int32)
        idx.copy_(torch.from_numpy(S))
        _lib.call("flc_tile_index", idx.data_ptr(), K, n, tiles.data_ptr(), st)
    else:  # the K largest of n Philox keys: the top-k encoder on the keys writes idx and tiles (val: the keys, replaced)
        seed, ctr = comp.philox.next()
        keys = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.call("flc_randk_keys", n, seed, ctr, keys.data_ptr(), st)
        codec.topk_encode_record(keys, K, rec)
    codec.sparse_gather(x, idx, float(np.float32(comp.D / comp.K)), out=val)  # compressors.py:289-291
    comp._finish(n, comp.K)
    return CompressedDelta(shapes, dev, n, record=rec, k=K, sparse=True)


def _flatten(ts: Sequence[torch.Tensor], dev: torch.device) -> torch.Tensor:
    """cat(ts) as a new flat fp32 vector on ``dev`` (a snapshot: the tensors may change before a deferred encode)."""
    return torch.cat([t.reshape(-1) for t in _fp32_on(ts, dev)])


def _compress(local: List[torch.Tensor], cached: Optional[Sequence[torch.Tensor]],
              compressors: Sequence[Compressor], wire: bool = False, sparse: bool = False,
              bucket: int = 0) -> CompressedDelta:
    """``compressors(cat(local − cached))``, or (``cached`` None) ``compressors(cat(local))``."""
    dev = local[0].device if local[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    shapes = [t.shape for t in local]
    n = sum(t.numel() for t in local)
    pipe = stacked_pipeline(compressors)
    seed_ctr = None
    if pipe is not None and 0 < pipe[0] < n and compressors[1].rng_mode == "philox":
        # the common case in one C call, the tensors as they are (model parameters on the device): the record and the
        # send count made by _flcfold.stacked_delta_record; a tensor it does not take (host-resident, not fp32 or not
        # contiguous) falls through to the converted call below with the same Philox (seed, counter)
        seed_ctr = compressors[1].philox.next()
        if DEFER_ENCODE and n <= _DEFER_MAX_N and _identical(compressors[1].vectorNormCompressor):
            r = _deferred(local, cached, shapes, n, pipe[0], pipe[1], compressors[0], compressors[1], dev, seed_ctr)
            if r is not None:
                return r
        r = None if cached is None else _stacked_fast(local, cached, shapes, n, pipe[0], pipe[1], compressors[0],
                                                      compressors[1], dev, seed_ctr)
        if r is not None:
            return r
    out = None
    if cached is None:
        out = _flatten(local, dev)
        if pipe is not None and 0 < pipe[0] < n:
            return _stacked(out, None, shapes, n, pipe[0], pipe[1], compressors[0], compressors[1], dev, seed_ctr)
    elif pipe is None or not 0 < pipe[0] < n:
        snap = codec._pyflat()
        if snap is not None:
            try:  # the flat delta in one C call (the tensors as they are: contiguous fp32 on one device)
                out = snap(local, cached)
            except TypeError:
                pass
            if out is not None and out.device != dev:
                out = None
    if out is None:
        ls, gs = _fp32_on(local, dev), _fp32_on(cached, dev)
        if pipe is not None and 0 < pipe[0] < n:
            return _stacked(ls, gs, shapes, n, pipe[0], pipe[1], compressors[0], compressors[1], dev, seed_ctr)
        out = codec.delta_flatten(ls, gs)
    dc = dense_wire_codec(compressors) if wire else None
    B = _bucket_of(compressors, bucket)
    if B and dc is not None and out.dtype == torch.float32:  # a bucket record: one norm per B elements, then the codes
        if DEFER_ENCODE and n <= _DEFER_BUCKET_MAX_N:
            r = _defer_bucket(out, shapes, n, compressors[0], dc, B, dev)  # (out: a new vector, the snapshot)
            if r is not None:
                return r
        return _bucket_record(out, shapes, n, compressors[0], dc, B, dev)
    if B:
        dc = None  # (a bucketed quantizer never sends the whole-vector dense record)
    if dc is not None:  # the quantizer's own wire as the message: codes written into the record, nothing decoded
        if DEFER_ENCODE and n <= _DEFER_DENSE_MAX_N and dc[0] != FLC_WIRE_NATURAL:
            r = _defer_dense(out, shapes, n, compressors[0], dc, dev)  # (out: a new vector, the snapshot)
            if r is not None:
                return r
        if NATURAL_DEFER and DEFER_ENCODE and dc[0] == FLC_WIRE_NATURAL and n <= _DEFER_NATURAL_MAX_N:
            r = _defer_natural(out, shapes, n, compressors[0], dev)
            if r is not None:
                return r
        return _dense_record(out, shapes, n, compressors[0], dc, dev)
    K = sparse_wire_codec(compressors, n) if sparse and _all_f32(local, cached) else None
    if K is not None:  # the sparsifier's own wire as the message: (idx, val, tiles) written into the record
        if DEFER_ENCODE and n <= _DEFER_MAX_N and compressors[0].compressorType == CompressorType.TOPK_COMPRESSOR:
            return _defer_sparse(out, shapes, n, K, compressors[0], dev, None)  # (out: a new vector, the snapshot)
        return _sparse_record(out, shapes, n, compressors[0], K, dev)
    if B:  # the bucketed compressVector's decoded vector
        with _bucketed(compressors[0], B):
            return CompressedDelta(shapes, dev, n, flat=compressors[0].compressVector(out))
    for comp in compressors:  # the drop-in compressors on the device, in order
        out = comp.compressVector(out)
    return CompressedDelta(shapes, dev, n, flat=out)


def _accumulate(local: List[torch.Tensor], cached: Optional[Sequence[torch.Tensor]], e: torch.Tensor, dev) -> None:
    """``e += cat(local − cached)`` in place (flc_ef_accumulate): one C call on the tensors as they are, or — a tensor
    it does not take (host-resident, not fp32 or not contiguous) — on their converted copies."""
    fast = codec._pyef()
    if fast is not None:
        try:
            fast(local, cached, e)
            return
        except TypeError:
            pass  # (nothing launched)
    codec.ef_accumulate(_fp32_on(local, dev), None if cached is None else _fp32_on(cached, dev), e)


def _compress_feedback(local: List[torch.Tensor], cached: Optional[Sequence[torch.Tensor]],
                       compressors: Sequence[Compressor], mem: ErrorMemory, wire: bool = False,
                       sparse: bool = False, bucket: int = 0) -> CompressedDelta:
    """:func:`_compress` of ``a = e + (local − cached)`` with the memory ``e`` of ``mem`` as the encoders' flat input,
    then ``e = a − c`` (fl_sim_amd/feedback.py): the K-entry residual of a stacked record (after the batched encode
    when the message is deferred), the K-entry residual of a sparse record likewise (flc_ef_residual_sparse_round),
    the dense one of any other compressor's decoded vector."""
    dev = local[0].device if local[0].is_cuda else torch.device("cuda", torch.cuda.current_device())
    shapes = [t.shape for t in local]
    n = sum(t.numel() for t in local)
    if mem.n != n:
        raise ValueError(f"the error memory holds {mem.n} elements, the message {n}")
    if mem.device != dev:
        raise ValueError(f"the error memory is on {mem.device}, the encode on {dev}")
    mem._settle()  # (the memory's earlier message still waits in a batch: that batch runs first)
    e = mem._acquire()
    _accumulate(local, cached, e, dev)
    pipe = stacked_pipeline(compressors)
    if pipe is not None and 0 < pipe[0] < n:
        tk, sd = compressors
        seed_ctr = None
        if sd.rng_mode == "philox":
            seed_ctr = sd.philox.next()
            if DEFER_ENCODE and n <= _DEFER_MAX_N and _identical(sd.vectorNormCompressor):
                return _defer(e, shapes, n, pipe[0], pipe[1], tk, sd, dev, seed_ctr, mem)
        d = _stacked(e, None, shapes, n, pipe[0], pipe[1], tk, sd, dev, seed_ctr)
        codec.ef_residual_round([d._record], [e], n, pipe[0], pipe[1])
        return d
    dc = dense_wire_codec(compressors) if wire else None
    B = _bucket_of(compressors, bucket)
    if B:  # bucketed: encoded at once from the memory's values, then the plain dense residual of the decoded record
        if dc is not None:
            d = _bucket_record(e, shapes, n, compressors[0], dc, B, dev)
        else:
            with _bucketed(compressors[0], B):
                d = CompressedDelta(shapes, dev, n, flat=compressors[0].compressVector(e))
        codec.ef_residual_dense(e, d.flat())
        return d
    if dc is not None:  # the message carries the record; the memory takes a − decode(record) (these quantizers are
        # unbiased: the plain dense residual) — from the round's batched encode itself with EF_DENSE_DEFER on
        if (EF_DENSE_DEFER and DEFER_ENCODE and n <= _DEFER_EF_DENSE_MAX_N and dc[0] != FLC_WIRE_NATURAL
                and _all_f32(local, cached)):  # (the messages _compress defers, no others)
            r = _defer_dense(e, shapes, n, compressors[0], dc, dev, mem)
            if r is not None:
                return r
        if (NATURAL_DEFER and DEFER_ENCODE and dc[0] == FLC_WIRE_NATURAL and n <= _DEFER_EF_NATURAL_MAX_N
                and _all_f32(local, cached)):  # (the messages _compress defers, no others)
            r = _defer_natural(e, shapes, n, compressors[0], dev, mem)
            if r is not None:
                return r
        d = _dense_record(e, shapes, n, compressors[0], dc, dev)
        codec.ef_residual_dense(e, codec.dense_record_decode(d._record, n, dc[0], dc[1], dc[2]))
        return d
    K = sparse_wire_codec(compressors, n) if sparse and _all_f32(local, cached) else None
    if K is not None:  # the memory is the encoder's input; it takes a − c at the record's K kept entries
        if DEFER_ENCODE and n <= _DEFER_MAX_N and compressors[0].compressorType == CompressorType.TOPK_COMPRESSOR:
            return _defer_sparse(e, shapes, n, K, compressors[0], dev, mem)
        d = _sparse_record(e, shapes, n, compressors[0], K, dev)
        codec.ef_residual_sparse_round([d._record], [e], n, K)
        return d
    out = e
    for comp in compressors:  # the drop-in compressors on the device, in order (each returns a new vector)
        out = comp.compressVector(out)
    if out is e or out.data_ptr() == e.data_ptr():  # (no compressor: the message carries a itself, e becomes +0)
        out = e.clone()
    codec.ef_residual_dense(e, out)
    return CompressedDelta(shapes, dev, n, flat=out)


# Deferred encodes (philox mode, the stacked pipeline, an identical norm compressor, models up to 16 M parameters).
# A model-sized encode is all fixed latency on the GPU — ~44 us per message at configs[0] (417,482 parameters), most of
# it the persistent select's grid exchanges — so a round's messages are encoded together: `communicate` flattens the
# client's delta (a snapshot: the model may change before the encode runs) and fixes its Philox (seed, counter) and
# send-count slot, and the first access to any of the round's records — or to a statistic of their compressors —
# encodes them all in one launch chain (flc_stacked_encode_round: each client's select on its share of the CUs with
# the message's own (seed, counter) — sampled clients' compressors have advanced differently, so a round's counters
# differ — records bit-identical to the per-message encodes; the select also counts the dithering stage's nonzero
# inputs into the message's slot, so no count launch follows).  FLC_DEFER_ENCODE=0 encodes every message when it is
# made (the one-C-call form).  deferred_stats() counts the batched encodes run and their messages.
DEFER_ENCODE = os.environ.get("FLC_DEFER_ENCODE", "1") != "0"
_DEFER_MAX_N = 1 << 24
_DEFER_MAX_PENDING = 64
_DEFER_MAX_BATCHES = 16


_STATS = {"batches": 0, "messages": 0}
_DENSE_STATS = {"batches": 0, "messages": 0}
_SPARSE_STATS = {"batches": 0, "messages": 0}


def _read_stats(stats: dict, reset: bool) -> dict:
    out = dict(stats)
    if reset:
        stats.update(batches=0, messages=0)
    return out


def deferred_stats(reset: bool = False) -> dict:
    """``{"batches": batched encodes run, "messages": messages they encoded}`` since import or since the last
    ``deferred_stats(reset=True)`` (which returns the figures up to then)."""
    return _read_stats(_STATS, reset)


def deferred_dense_stats(reset: bool = False) -> dict:
    """:func:`deferred_stats` for the dense records' batched encodes (flc_quant_encode_round, flc_natural_encode_round
    and their residual forms), counted apart."""
    return _read_stats(_DENSE_STATS, reset)


def deferred_sparse_stats(reset: bool = False) -> dict:
    """:func:`deferred_stats` for the sparse records' batched encodes (flc_topk_encode_batch), counted apart."""
    return _read_stats(_SPARSE_STATS, reset)


class _Item(NamedTuple):
    """One waiting message of a batch."""

    delta: "CompressedDelta"  # the message's delta, which takes its record when the batch has encoded
    flat: torch.Tensor  # the encoder's input: a snapshot of the flat vector, or the error memory's tensor
    seed: int  # the message's Philox seed ...
    counter: int  # ... and counter
    count: Optional[torch.Tensor]  # the send-count slot the encode writes (None: the count does not depend on the data)
    comp: Optional[Compressor]  # the compressor owning that slot
    stream: torch.cuda.Stream  # the stream the flat vector was written on ...
    handle: int  # ... and its handle
    mem: Optional[ErrorMemory]  # the error memory whose tensor ``flat`` is, or None


class _Batch:
    """The waiting messages of one (device, n, k, levels, order): a round's stacked records, encoded together (a signed
    and a magnitude message never share a launch: a batched encode runs in one selection order).  The stream
    handling around the encode is shared with :class:`_DenseBatch`, which replaces :meth:`_encode_rows`."""

    stats = _STATS

    def __init__(self, key):
        self.key = key
        self.items: List[_Item] = []

    def run(self) -> None:
        if _PENDING.get(self.key) is self:
            del _PENDING[self.key]
        items, self.items = self.items, []
        if not items:
            return
        try:
            self._encode(items)
        except BaseException:
            self.items = items + self.items  # (left pending: the next access tries again and raises again)
            _PENDING.setdefault(self.key, self)
            raise

    def _encode(self, items) -> None:
        dev = torch.device("cuda", self.key[0])
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream(dev)
            ch = cur.cuda_stream
            for st in {it.handle: it.stream for it in items if it.handle != ch}.values():  # (other streams' deltas)
                cur.wait_stream(st)
            rows = self._encode_rows(items, dev)
            self.stats["batches"] += 1
            self.stats["messages"] += len(items)
            for it, r in zip(items, rows):
                if it.handle != ch:
                    it.flat.record_stream(cur)
                    if it.comp is not None:
                        it.comp._note_slab_stream(cur)  # (the count was written on this stream, not the slot's own)
                if it.mem is not None:
                    it.mem._written(cur)
                it.delta._record, it.delta._batch = r, None

    def _encode_rows(self, items, dev):
        """The items' records, encoded on ``dev``'s current stream: the rows of one ``[C, stride]`` block."""
        _, n, k, levels, order = self.key
        stride, _ = codec.stacked_wire_layout(n, k)
        C = len(items)
        recs = torch.empty(C, stride, dtype=torch.uint8, device=dev)
        flats = [it.flat for it in items]
        seeds, ctrs, cnts = [it.seed for it in items], [it.counter for it in items], [it.count for it in items]
        fast = codec._pyround()
        if fast is not None:  # one C call: the encode's launch chain fills the count slots too
            ws = codec.workspace(dev, codec._ws_size(dev, "flc_stacked_encode_batch_workspace_size", n, k, C),
                                 "topk_batch")
            fast(flats, seeds, ctrs, k, levels, recs, cnts, ws, order)
        else:
            codec.stacked_encode_batch(flats, k, levels, seeds=seeds, counters=ctrs, counts=cnts, wires=recs,
                                       order=order)
        codec._after_encode(dev)
        rows = recs.unbind(0)
        fed = [(r, it.mem) for it, r in zip(items, rows) if it.mem is not None]
        if fed:  # error feedback: e = a − c at the records' kept entries, one launch for the round (an encode
            # that raised never gets here: the memories then still hold a, and the retry encodes the same a)
            codec.ef_residual_round([r for r, _ in fed], [m._e for _, m in fed], n, k, levels)
        return rows


# Deferred dense records (philox mode, `wire` on, one standard or natural dithering with p = inf or 2 and the device
# norm, no error feedback).  The per-message flc_quant_encode_auto of a model-sized vector is all fixed latency too, so
# these messages wait like the stacked ones — the flat delta snapshotted, the Philox (seed, counter) and the count slot
# fixed at `communicate` — and one flc_quant_encode_round (two launches per 64 messages, each message with its own
# (seed, counter), record and count slot) writes the round's records, bit-identical to the per-message encodes.
# The same switch (FLC_DEFER_ENCODE) and pending bounds as the stacked batches, which share _PENDING with these; the
# size bound is the dense kind's own: measured (profiles/dense_record_defer.json), ten messages' batched encode takes
# 60 us against 124 us of per-message encodes at 417,482 elements and 95 against 128 us at 1 M, but 157 against 136 us
# at 2 M and 248 against 137 us for eight messages of 4 M — past ~1.5 M elements the per-message call's one-launch
# form, which reads the vector once, beats two streaming launches — so larger messages keep the immediate path.
_DEFER_DENSE_MAX_N = 1 << 20

# With error feedback such a message is encoded at once — flc_ef_accumulate, flc_quant_encode_auto, a dense decode into
# a fresh vector and flc_ef_residual_dense — unless FLC_EF_DENSE_DEFER=1 (EF_DENSE_DEFER, off by default): then it
# waits like the others with the error memory's tensor as the encoder's input, in a batch of its own kind (the key's
# last element), and one flc_quant_encode_residual_round writes the round's records and leaves every memory holding
# a − decode(record) from the encode's own pass: nothing decoded, no temporary, no further launch.  Records, memories,
# statistics and counters are bit-identical to the immediate path's.  The size bound is this kind's own: the immediate
# chain makes three more dense passes per message than without feedback, so the batched form wins further up —
# measured (profiles/ef_dense_round.json, encodes only), ten messages take 72 us against 316 us at 417,482 elements,
# 104 against 316 us at 1 M and 163 against 319 us at 2 M; eight messages of 4 M take 253 against 289 us, the ranges
# apart in one run and touching in another, and of 8 M 482 against 467 us.  The bound is the largest size at which the
# ranges stayed apart in every run.
EF_DENSE_DEFER = os.environ.get("FLC_EF_DENSE_DEFER", "0") == "1"
_DEFER_EF_DENSE_MAX_N = 2_000_000


class _DenseBatch(_Batch):
    """The waiting dense-record messages of one (device, "quant", n, format, levels, bits, norm_p, feedback); an
    item's count slot and compressor are None for natural dithering, whose send count does not depend on the data.
    In a feedback batch every item's ``flat`` is its error memory's tensor."""

    stats = _DENSE_STATS

    def _encode_rows(self, items, dev):
        _, _, n, fmt, levels, bits, pk, fed = self.key
        stride, _ = codec.dense_wire_layout(n, fmt, bits)
        recs = torch.empty(len(items), stride, dtype=torch.uint8, device=dev)
        rows = recs.unbind(0)
        # error feedback: the encode's own pass leaves e = a − decode(record) in the memories.  The call is the last
        # thing here that can raise: a batch that failed has written no memory, and the retry encodes the same a
        encode = codec.quant_encode_residual_round if fed else codec.quant_encode_round
        encode([it.flat for it in items], fmt, levels, bits, pk, [it.seed for it in items],
               [it.counter for it in items], recs,
               [it.count for it in items] if fmt == FLC_Q_STANDARD_DITHER else None)
        return rows


# Deferred bucket records (philox mode, `wire` on, a bucket size, the device norms, no error feedback): the messages
# wait like the dense ones and one flc_bucket_encode_round — one launch per 64 messages, each message with its own
# (seed, counter), record and count slot — writes the round's records, bit-identical to the per-message
# flc_bucket_encode.  The same switch (FLC_DEFER_ENCODE) and pending bounds; deferred_bucket_stats() counts them apart.
_DEFER_BUCKET_MAX_N = 1 << 20
_BUCKET_STATS = {"batches": 0, "messages": 0}


def deferred_bucket_stats(reset: bool = False) -> dict:
    """:func:`deferred_stats` for the bucket records' batched encodes (flc_bucket_encode_round), counted apart."""
    return _read_stats(_BUCKET_STATS, reset)


class _BucketBatch(_Batch):
    """The waiting bucket-record messages of one (device, "bucket", n, format, levels, bits, bucket, norm_p); an item's
    count slot and compressor are None for natural dithering."""

    stats = _BUCKET_STATS

    def _encode_rows(self, items, dev):
        _, _, n, fmt, levels, bits, B, pk = self.key
        stride, _ = codec.bucket_wire_layout(n, fmt, bits, B)
        recs = torch.empty(len(items), stride, dtype=torch.uint8, device=dev)
        rows = recs.unbind(0)
        codec.bucket_encode_round([it.flat for it in items], fmt, levels, bits, B, pk, [it.seed for it in items],
                                  [it.counter for it in items], rows,
                                  [it.count for it in items] if fmt == FLC_Q_STANDARD_DITHER else None)
        return rows


def _defer_bucket(x: torch.Tensor, shapes, n: int, comp: Compressor, dc: Tuple[int, int, int], B: int,
                  dev) -> Optional[CompressedDelta]:
    """The bucket-record message of the flat vector ``x`` (a snapshot) joins the round's batched encode; the Philox
    stream and the send statistics advance here exactly as :func:`_bucket_record` advances them.  None (nothing
    advanced: the immediate path takes the message) outside philox mode with the device norm of p = inf or 2."""
    fmt, s, bits = dc
    if comp.rng_mode != "philox" or comp._wants_host_norm(device_input=True):
        return None
    pk = _norm_kind(comp.p)
    if pk is None or x.dtype != torch.float32 or x.device != dev:
        return None
    x = codec._dev_f32(x).reshape(-1)
    std = fmt == FLC_Q_STANDARD_DITHER
    st = torch.cuda.current_stream(dev)
    cnt = comp._count_slot(dev, st) if std else None  # (before the batch is looked up, as in _defer)
    b = _waiting(_BucketBatch, (dev.index, "bucket", n, fmt, s, bits, B, pk))
    seed, ctr = comp.philox.next()
    d = CompressedDelta(shapes, dev, n, levels=s, batch=b, format=fmt, bits=bits, bucket=B)
    _bucket_stats(comp, n, B, std, cnt)
    return _enqueue(b, _Item(d, x, seed, ctr, cnt, comp if std else None, st, st.cuda_stream, None))


# Deferred natural-compressor records (philox mode, `wire` on, the natural compressor's uint16 wire), behind
# FLC_NATURAL_DEFER=1 (NATURAL_DEFER, off by default).  The compressor has no norm, so a round is one streaming launch
# per 64 messages with no workspace (flc_natural_encode_round), each message with its own (seed, counter) and record,
# bit-identical to the per-message flc_natural_encode.  With error feedback the message waits in a batch of its own
# kind (the key's last element) with the error memory's tensor as the encoder's input, and one
# flc_natural_encode_residual_round writes the round's records and leaves every memory holding a − decode(record) from
# the encode's own pass — the immediate chain's flc_natural_decode into a fresh vector and flc_ef_residual_dense are not
# run.  Records, memories, statistics and counters are bit-identical to the immediate path's.  The same switch
# (FLC_DEFER_ENCODE) and pending bounds as the other batches, which share _PENDING with these.  The size bounds are
# measured (profiles/natural_defer_round.json, encodes only, two runs, device events): each is the largest size at which
# the round call's min–max range lay below the per-message chain's in both runs.  One streaming launch has no mid-size
# dip like the dithering round's two: ten plain messages take 37 us against 81 us at 417,482 elements and eight take
# 107 against 133 us at 8 M (at 16 M 178 against 198 us, the ranges touching in one run); with feedback ten take 40
# against 254 us at 417,482 and eight 244 against 567 us at 16 M, apart in both runs at every size.
NATURAL_DEFER = os.environ.get("FLC_NATURAL_DEFER", "0") == "1"
_DEFER_NATURAL_MAX_N = 8_000_000
_DEFER_EF_NATURAL_MAX_N = 16_000_000


class _NaturalBatch(_Batch):
    """The waiting natural-compressor messages of one (device, "natural", n, feedback); an item has no count slot and
    no compressor (the send count is 9/32 n whatever the data).  In a feedback batch every item's ``flat`` is its error
    memory's tensor."""

    stats = _DENSE_STATS

    def _encode_rows(self, items, dev):
        _, _, n, fed = self.key
        stride, _ = codec.dense_wire_layout(n, FLC_WIRE_NATURAL, 16)
        recs = torch.empty(len(items), stride, dtype=torch.uint8, device=dev)
        rows = recs.unbind(0)
        # error feedback: the encode's own pass leaves e = a − decode(record) in the memories.  The call is the last
        # thing here that can raise: a batch that failed has written no memory, and the retry encodes the same a
        encode = codec.natural_encode_residual_round if fed else codec.natural_encode_round
        encode([it.flat for it in items], [it.seed for it in items], [it.counter for it in items], recs)
        return rows


# Deferred sparse records (`sparse` on, one top-k compressor, any rng_mode: top-k draws no random numbers).  The
# model-sized select is the same fixed latency as the stacked pipeline's, so these messages wait like the stacked ones
# — the flat delta snapshotted (or the error memory's tensor itself), the send statistics advanced at `communicate` —
# and one flc_topk_encode_batch writes the round's records into the rows of one block, equal to the per-message
# flc_topk_encode_tiled.  The same switch (FLC_DEFER_ENCODE), size bound and pending bounds as the stacked batches.
# Rand-k keeps the immediate path.
class _SparseBatch(_Batch):
    """The waiting top-k messages of one (device, "sparse", n, K, order); an item has no Philox state and no count
    slot."""

    stats = _SPARSE_STATS

    def _encode_rows(self, items, dev):
        _, _, n, k, order = self.key
        stride, _ = codec.sparse_wire_layout(n, k)
        recs = torch.empty(len(items), stride, dtype=torch.uint8, device=dev)
        codec.topk_encode_records([it.flat for it in items], k, recs, order=order)
        rows = recs.unbind(0)
        fed = [(r, it.mem) for it, r in zip(items, rows) if it.mem is not None]
        if fed:  # error feedback: e = a − c at the records' kept entries, one launch for the round, after the encode
            # succeeded (an encode that raised never gets here: the memories then still hold a)
            codec.ef_residual_sparse_round([r for r, _ in fed], [m._e for _, m in fed], n, k)
        return rows


_PENDING: dict = {}


def _run_pending() -> None:
    """Every deferred encode now (before a compressor's pending send counts are read)."""
    for b in list(_PENDING.values()):
        b.run()


Compressor._before_read = staticmethod(_run_pending)


def _deferred(local, cached, shapes, n: int, K: int, s: int, tk: Compressor, sd: Compressor, dev,
              seed_ctr) -> Optional[CompressedDelta]:
    snap = codec._pyflat()
    if cached is None:  # (nothing subtracted: the flat vector itself)
        flat = _flatten(local, dev)
    else:
        try:
            flat = snap(local, cached) if snap is not None else codec.delta_flatten(local, cached)
        except TypeError:  # (host-resident, non-contiguous or non-fp32 tensors: converted first)
            flat = codec.delta_flatten(_fp32_on(local, dev), _fp32_on(cached, dev))
    if flat.device != dev:
        return None
    return _defer(flat, shapes, n, K, s, tk, sd, dev, seed_ctr, None)


def _waiting(cls, key) -> "_Batch":
    """The waiting batch under ``key``, made (of class ``cls``) when there is none."""
    b = _PENDING.get(key)
    if b is None:
        b = _PENDING[key] = cls(key)
    return b


def _enqueue(b: "_Batch", item: _Item) -> CompressedDelta:
    """``item`` joins the waiting batch ``b``; its delta.  A full batch is encoded at once, and with too many batches
    waiting all of them are."""
    b.items.append(item)
    if item.mem is not None:
        item.mem._batch = b
    if len(b.items) >= _DEFER_MAX_PENDING:
        b.run()
    elif len(_PENDING) > _DEFER_MAX_BATCHES:  # (messages nobody reads: the waiting deltas stay bounded)
        _run_pending()
    return item.delta


def _defer(flat: torch.Tensor, shapes, n: int, K: int, s: int, tk: Compressor, sd: Compressor, dev, seed_ctr,
           mem: Optional[ErrorMemory]) -> CompressedDelta:
    """The message of the flat vector ``flat`` joins the round's batched encode (``mem``: ``flat`` is that error
    memory's tensor, which takes the residual once the batch has encoded)."""
    st = torch.cuda.current_stream(dev)
    # the slot before the batch is looked up: a full slab is read back, running the batches.  With the slot in hand the
    # compressors' pending lists have room, so the _finish calls below read nothing back and run no batch: they come
    # before the item is appended only so that the append and the bounds sit in one place (_enqueue)
    cnt = sd._count_slot(dev, st)
    b = _waiting(_Batch, (dev.index, n, K, s, tk.order))
    d = CompressedDelta(shapes, dev, n, k=K, levels=s, batch=b)
    tk._finish(n, tk.K)
    sd._finish_pending(n, cnt, _norm_stage_send(sd, None), _code_fraction(sd.s))
    return _enqueue(b, _Item(d, flat, seed_ctr[0], seed_ctr[1], cnt, sd, st, st.cuda_stream, mem))


def _defer_dense(x: torch.Tensor, shapes, n: int, comp: Compressor, dc: Tuple[int, int, int],
                 dev, mem: Optional[ErrorMemory] = None) -> Optional[CompressedDelta]:
    """The dense-record message of the flat vector ``x`` (a snapshot, or — ``mem`` — that error memory's tensor, which
    the batched encode leaves holding the residual) joins the round's batched quantizer encode; the Philox stream and
    the send statistics advance here exactly as :func:`_dense_record` advances them.  None (nothing advanced: the
    immediate path takes the message) outside philox mode with the device norm of p = inf or 2 on a float32 vector."""
    fmt, s, bits = dc
    if comp.rng_mode != "philox" or comp._wants_host_norm(device_input=True):
        return None
    pk = _norm_kind(comp.p)
    if pk is None or x.dtype != torch.float32 or x.device != dev:
        return None
    if mem is None:
        x = codec._dev_f32(x).reshape(-1)
    elif x.dim() != 1 or not x.is_contiguous() or x.data_ptr() % 16:  # (written in place: never a copy)
        return None
    std = fmt == FLC_Q_STANDARD_DITHER
    st = torch.cuda.current_stream(dev)
    cnt = comp._count_slot(dev, st) if std else None  # (before the batch is looked up and the _finish calls, as in _defer)
    b = _waiting(_DenseBatch, (dev.index, "quant", n, fmt, s, bits, pk, mem is not None))
    seed, ctr = comp.philox.next()
    d = CompressedDelta(shapes, dev, n, levels=s, batch=b, format=fmt, bits=bits)
    if std:
        comp._finish_pending(n, cnt, _norm_stage_send(comp, None), _code_fraction(s))
    else:
        comp._finish(n, n * _code_fraction(s))
    return _enqueue(b, _Item(d, x, seed, ctr, cnt, comp if std else None, st, st.cuda_stream, mem))


def _defer_natural(x: torch.Tensor, shapes, n: int, comp: Compressor, dev,
                   mem: Optional[ErrorMemory] = None) -> Optional[CompressedDelta]:
    """The natural-compressor message of the flat vector ``x`` (a snapshot, or — ``mem`` — that error memory's tensor,
    which the batched encode leaves holding the residual) joins the round's batched encode; the Philox stream and the
    send statistics advance here exactly as :func:`_dense_record` advances them (compressors.py:302-325).  None
    (nothing advanced: the immediate path takes the message) outside philox mode on a float32 vector."""
    if comp.rng_mode != "philox" or x.dtype != torch.float32 or x.device != dev:
        return None
    if mem is None:
        x = codec._dev_f32(x).reshape(-1)
    elif x.dim() != 1 or not x.is_contiguous() or x.data_ptr() % 16:  # (written in place: never a copy)
        return None
    st = torch.cuda.current_stream(dev)
    b = _waiting(_NaturalBatch, (dev.index, "natural", n, mem is not None))
    seed, ctr = comp.philox.next()
    d = CompressedDelta(shapes, dev, n, levels=0, batch=b, format=FLC_WIRE_NATURAL, bits=16)
    comp._finish(n, 9.0 / 32.0 * n)  # compressors.py:325
    return _enqueue(b, _Item(d, x, seed, ctr, None, None, st, st.cuda_stream, mem))


def _defer_sparse(flat: torch.Tensor, shapes, n: int, K: int, tk: Compressor, dev,
                  mem: Optional[ErrorMemory]) -> CompressedDelta:
    """The top-k message of the flat vector ``flat`` (a snapshot, or — ``mem`` — that error memory's tensor, which
    takes the residual once the batch has encoded) joins the round's batched top-k encode; the send statistics advance
    here as ``compressVector`` advances them (compressors.py:293-296)."""
    st = torch.cuda.current_stream(dev)
    b = _waiting(_SparseBatch, (dev.index, "sparse", n, K, tk.order))
    d = CompressedDelta(shapes, dev, n, k=K, batch=b, sparse=True)
    tk._finish(n, tk.K)
    return _enqueue(b, _Item(d, flat, 0, 0, None, None, st, st.cuda_stream, mem))


def _stacked_fast(local, cached, shapes, n: int, K: int, s: int, tk: Compressor, sd: Compressor, dev,
                  seed_ctr) -> Optional[CompressedDelta]:
    """The philox-mode stacked message in one C call (None: the extension is absent or a tensor needs converting)."""
    fast = codec._pydelta()
    if fast is None:
        return None
    stride, _ = codec.stacked_wire_layout(n, K)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    cnt = sd._count_slot(dev)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_stacked_encode_delta_workspace_size", n, K, len(local)), "topk")
    try:
        fast(local, cached, K, s, seed_ctr[0], seed_ctr[1], rec, cnt, ws, tk.order)
    except TypeError:
        return None  # (nothing launched)
    codec._after_encode(dev)
    tk._finish(n, tk.K)
    nc = sd.vectorNormCompressor
    base = _norm_stage_send(sd, None if _identical(nc) else codec.wire_packet(rec, n, K, s).norm)
    sd._finish_pending(n, cnt, base, _code_fraction(sd.s))
    return CompressedDelta(shapes, dev, n, record=rec, k=K, levels=s)


def _identical(nc) -> bool:
    return isinstance(nc, Compressor) and nc.compressorType == CompressorType.IDENTICAL


def _stacked(ls, gs, shapes, n: int, K: int, s: int, tk: Compressor, sd: Compressor, dev,
             seed_ctr=None) -> CompressedDelta:
    """The stacked message of ``cat(ls − gs)``, or (``gs`` None) of the flat vector ``ls``."""
    stride, _ = codec.stacked_wire_layout(n, K)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    pk = codec.wire_packet(rec, n, K, s)
    per = _code_fraction(sd.s)
    seed, ctr = seed_ctr if seed_ctr is not None else sd.philox.next()
    if sd.rng_mode == "philox":
        # the delta formed inside the encoder's read; the dithering stage's nonzero count stays on the device
        if gs is None:
            codec.stacked_encode(ls, K, s, seed, ctr, wire=rec, order=tk.order)
            cnt = sd._count_slot(dev)
            _lib.call("flc_count_nonzero_at_batch", _ptrs([ls]), _ptrs([pk.idx]), 1, n, K, _ptrs([cnt]),
                      codec._stream(dev))
        else:
            codec.stacked_encode_delta(ls, gs, K, s, seed, ctr, wire=rec, order=tk.order)
            cnt = sd._count_slot(dev)
            _lib.call("flc_delta_count_nonzero_at", _ptrs(ls), _ptrs(gs),
                      (ctypes.c_int64 * len(ls))(*[t.numel() for t in ls]), len(ls), pk.idx.data_ptr(), K,
                      cnt.data_ptr(), codec._stream(dev))
        tk._finish(n, tk.K)
        base = _norm_stage_send(sd, pk.norm)
        sd._finish_pending(n, cnt, base, per)
        return CompressedDelta(shapes, dev, n, record=rec, k=K, levels=s)
    # compat: TopK (compressors.py:293-296), then standard dithering of the K-sparse vector (327-365) whose nonzero
    # elements, in index order, are the kept values: one random.random() per consuming kept value
    x = ls if gs is None else codec.delta_flatten(ls, gs)
    val = torch.empty(K, dtype=torch.float32, device=dev)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_topk_workspace_size", n, K), "topk")
    st = codec._stream(dev)
    codec._call_ord("flc_topk_encode_tiled", tk.order, 2, x.data_ptr(), n, K, pk.idx.data_ptr(), val.data_ptr(),
                    pk.tiles.data_ptr(), ws.data_ptr(), ws.numel(), st)
    codec._after_encode(dev)
    tk._finish(n, tk.K)
    row = val.reshape(1, K)
    qws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", 1, K), "quant")
    _lib.call("flc_quant_norm", row.data_ptr(), 1, K, FLC_NORM_INF, pk.norm.data_ptr(), qws.data_ptr(), qws.numel(), st)
    consumers = int(codec.count_consumers(row, pk.norm).item())
    u = sd._uniforms(consumers, dev)
    nnz = torch.empty(1, dtype=torch.int64, device=dev)
    _lib.call("flc_quant_encode", row.data_ptr(), 1, K, FLC_Q_STANDARD_DITHER, s, 8, pk.norm.data_ptr(), seed, ctr,
              u.data_ptr() if consumers else None, pk.codes.data_ptr(), nnz.data_ptr(), qws.data_ptr(), qws.numel(), st)
    base = _norm_stage_send(sd, pk.norm)
    nz = int(nnz.item())
    sd._finish(n, base + nz * per if nz else base)
    return CompressedDelta(shapes, dev, n, record=rec, k=K, levels=s)


_RECORD_KINDS = ("stacked", "quant", "natural", "sparse", "bucket")


def _round_deltas(messages: Sequence, key: str, kinds: Tuple[str, ...]) -> Optional[List[CompressedDelta]]:
    """The messages' compressed deltas under ``key`` when there are messages, every one carries a
    :class:`CompressedDelta` of one of ``kinds`` and all share one ``codec_key``, else None."""
    if not messages:
        return None
    ds = []
    for m in messages:
        d = m.get(key) if isinstance(m, dict) else None
        if not isinstance(d, CompressedDelta) or d.kind not in kinds:
            return None
        ds.append(d)
    key0 = ds[0].codec_key
    for d in ds:
        if d.codec_key != key0:
            return None
    return ds


def stacked_round(messages: Sequence, key: str = "delta_parameters") -> Optional[List[CompressedDelta]]:
    """The messages' compressed deltas when every one is a stacked record of one (n, k, levels), else None."""
    return _round_deltas(messages, key, ("stacked",))


def dense_record_round(messages: Sequence, key: str = "delta_parameters") -> Optional[List[CompressedDelta]]:
    """The messages' compressed deltas when every one is a dense record (``kind`` "quant" or "natural") of one
    (n, format, levels, bits), else None (a mixed round: each message then decodes itself)."""
    return _round_deltas(messages, key, ("quant", "natural"))


def sparse_round(messages: Sequence, key: str = "delta_parameters") -> Optional[List[CompressedDelta]]:
    """The messages' compressed deltas when every one is a sparse record (``kind`` "sparse") of one (n, k), else None
    (a mixed round: each message then decodes itself)."""
    return _round_deltas(messages, key, ("sparse",))


def record_round(messages: Sequence, key: str = "delta_parameters") -> Optional[List[CompressedDelta]]:
    """:func:`stacked_round`, :func:`dense_record_round` or :func:`sparse_round`: a round the record folds take, else
    None."""
    return _round_deltas(messages, key, _RECORD_KINDS)


class _Entries(NamedTuple):
    """One uniform record kind's entry points, by server form (the FedOpt fold, the variance-reduced servers'
    gradient fold, the grouped fold): the C names, and the ``codec._py*`` accessor of the form's one-call ``_flcfold``
    entry (None: the form has none for this kind)."""

    fedopt: str
    gradient: str
    groups: str
    py_fedopt: object
    py_gradient: object
    py_groups: object


def _entries(infix: str, *accessors) -> _Entries:
    return _Entries(f"flc_fedopt_fold_{infix}records", f"flc_avg_and_gradient_{infix}records",
                    f"flc_fold_{infix}record_groups", *accessors)


_STACKED = _entries("", codec._pyrecs, codec._pygrecs, codec._pygroups)
_SPARSE = _entries("sparse_", codec._pysrecs, codec._pygsrecs, None)
_DENSE = _entries("dense_", codec._pydrecs, codec._pygdrecs, None)
_BUCKET = _entries("bucket_", lambda: None, lambda: None, None)  # (the C entries; no one-call _flcfold form)
_MIXED = _entries("mixed_", codec._pymrecs, None, None)  # (a mixed_round: every record by its own descriptor)


def _record_entries(d0: CompressedDelta) -> Tuple[tuple, _Entries]:
    """(shape, entries) of a uniform round of ``d0``'s records — the one place that knows a kind's entry points.
    ``shape`` is what every entry of the kind takes after the record count: (n, k, levels) of stacked records, (n, k)
    of sparse ones, (n, format, levels, bits) of dense ones, (n, format, levels, bits, bucket) of bucket ones."""
    if d0.kind == "sparse":
        return (d0.n, d0.k), _SPARSE
    if d0.kind == "bucket":
        return (d0.n, d0.format, d0.levels, d0.bits, d0.bucket), _BUCKET
    if d0.kind in ("quant", "natural"):
        return (d0.n, d0.format, d0.levels, d0.bits), _DENSE
    return (d0.n, d0.k, d0.levels), _STACKED


# Mixed rounds.  A round whose messages do not share one codec_key — another K, another bit width, another record
# kind, or one client that sends its decoded vector — is declined by record_round, and every message then decodes
# itself (4·n bytes written per message, read back by the dense fold).  With FLC_MIXED_FOLD=1 such a round is folded in
# one pass over the messages as they are: every record carries its own descriptor (flc_record_kind, k, format, levels,
# bits) and a decoded vector is read as a flat fp32 record (flc_fedopt_fold_mixed_records, flc_fold_mixed_record_groups,
# flc_avg_and_gradient_mixed_records), bit-identical to the per-message path.  Off by default; uniform rounds take the
# uniform folds either way.  mixed_fold_stats() counts the mixed folds run and their messages.
MIXED_FOLD = os.environ.get("FLC_MIXED_FOLD", "0") == "1"
_MIXED_STATS = {"folds": 0, "messages": 0}
_REC_STACKED, _REC_SPARSE, _REC_DENSE, _REC_FLAT = (_lib.FLC_REC_STACKED, _lib.FLC_REC_SPARSE, _lib.FLC_REC_DENSE,
                                                     _lib.FLC_REC_FLAT)


def mixed_fold_stats(reset: bool = False) -> dict:
    """``{"folds": mixed one-pass folds run, "messages": messages they folded}`` since import or since the last
    ``mixed_fold_stats(reset=True)`` (which returns the figures up to then)."""
    out = dict(_MIXED_STATS)
    if reset:
        _MIXED_STATS.update(folds=0, messages=0)
    return out


def _folded(messages: int, mixed: bool) -> bool:
    """A fold has run (True); a mixed one is counted."""
    if mixed:
        _MIXED_STATS["folds"] += 1
        _MIXED_STATS["messages"] += messages
    return True


def mixed_round(messages: Sequence, key: str = "delta_parameters") -> Optional[List[CompressedDelta]]:
    """The messages' compressed deltas when :data:`MIXED_FOLD` is on and the round is one the mixed fold takes and the
    uniform folds do not: every message carries a :class:`CompressedDelta` of one ``n`` under ``key``, at least one is
    a record, they do not all share one ``codec_key``, and every decoded (``"dense"``) one holds a float32 flat vector;
    else None."""
    if not MIXED_FOLD or not messages:
        return None
    ds = []
    for m in messages:
        d = m.get(key) if isinstance(m, dict) else None
        if not isinstance(d, CompressedDelta):
            return None
        ds.append(d)
    d0 = ds[0]
    if any(d.n != d0.n for d in ds) or all(d.kind in ("dense", "bucket") for d in ds):
        return None
    if all(d.codec_key == d0.codec_key for d in ds):
        return None
    if any(d.kind == "dense" and not (isinstance(d._flat, torch.Tensor) and d._flat.dtype is torch.float32
                                      and d._flat.numel() == d.n) for d in ds):
        return None
    return ds


def _mixed_tables(deltas: Sequence[CompressedDelta], dev: torch.device, records=None):
    """What the mixed entry points read of ``deltas`` on ``dev``: (tensors, kinds, ks, formats, levels, bits) — a
    record's bytes (a deferred one is encoded by this read), a decoded message's flat fp32 vector; tensors elsewhere
    (or not 16-B aligned) are copied.  ``records``: the records where they were staged (None entries: the delta's own)."""
    ts, kinds, ks, fmts, lvs, bits = [], [], [], [], [], []
    for i, d in enumerate(deltas):
        if d.kind == "dense":
            t, desc = d._flat, (_REC_FLAT, 0, 0, 0, 0)
        elif d.kind == "bucket":  # (not in the mixed fold's descriptor tables: read as its decoded vector)
            t, desc = d.flat(), (_REC_FLAT, 0, 0, 0, 0)
        else:
            t = d.record
            desc = ((_REC_STACKED, d.k, 0, d.levels, 0) if d.kind == "stacked" else
                    (_REC_SPARSE, d.k, 0, 0, 0) if d.kind == "sparse" else
                    (_REC_DENSE, 0, d.format, d.levels, d.bits))
        if records is not None and records[i] is not None:
            t = records[i]
        t = t.detach()
        if t.device != dev:
            t = t.to(dev)
        if not t.is_contiguous() or t.data_ptr() % 16:
            t = t.clone(memory_format=torch.contiguous_format)
        ts.append(t)
        for col, x in zip((kinds, ks, fmts, lvs, bits), desc):
            col.append(int(x))
    return ts, kinds, ks, fmts, lvs, bits


def _mixed_ctypes(kinds, ks, fmts, lvs, bits):
    m = len(kinds)
    i32 = lambda xs: (ctypes.c_int32 * m)(*xs)  # noqa: E731
    return i32(kinds), (ctypes.c_int64 * m)(*ks), i32(fmts), i32(lvs), i32(bits)


def _round_records(deltas: Sequence[CompressedDelta], dev: torch.device, mixed: bool, records=None):
    """(the round's records on ``dev``, what the C entries take after the record count, the entries) — a uniform
    round's shape, or a mixed round's ``n`` and descriptor columns.  ``records``: the records where they were staged
    (None, or None entries: the deltas' own); records elsewhere are moved."""
    if mixed:
        recs, *cols = _mixed_tables(deltas, dev, records)
        return recs, (deltas[0].n, *_mixed_ctypes(*cols)), _MIXED
    recs = [d.record if records is None or records[i] is None else records[i] for i, d in enumerate(deltas)]
    return ([r if r.device == dev else r.to(dev) for r in recs], *_record_entries(deltas[0]))


def _server_ok(groups: Sequence[Sequence[torch.Tensor]], n: int, distinct: bool = False) -> Optional[torch.device]:
    """The HIP device of server tensor lists that are, list by list, contiguous fp32 tensors of one device holding the
    first list's element counts, ``n`` in all — with ``distinct``, no non-empty tensor in two places; else None."""
    first = list(groups[0]) if groups else []
    if not first or not isinstance(first[0], torch.Tensor) or not first[0].is_cuda:
        return None
    dev = first[0].device
    seen = set()
    for g in groups:
        if len(g) != len(first) or any(not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev
                                            and t.dtype is torch.float32 and t.is_contiguous()
                                            and t.numel() == f.numel()) for t, f in zip(g, first)):
            return None
        if distinct:
            ptrs = [t.data_ptr() for t in g if t.numel()]
            if len(seen.intersection(ptrs)) or len(set(ptrs)) != len(ptrs):
                return None
            seen.update(ptrs)
    return dev if sum(t.numel() for t in first) == n else None


def fold_records(deltas: Sequence[CompressedDelta], weights: Sequence[float], delta_params: Sequence[torch.Tensor],
                 theta: Optional[Sequence[torch.Tensor]], v: Optional[Sequence[torch.Tensor]], beta0: float,
                 opt: str = "avg", lr: float = 1.0, beta2: float = 0.0, tau: float = 0.0, mixed: bool = False) -> bool:
    """``δ = β0·δ + Σ_c w_c·decode(record_c)`` in message order, then (``theta``) the server optimiser's step — one
    ``flc_fedopt_fold_records`` pass (``flc_fedopt_fold_dense_records`` / ``flc_fedopt_fold_sparse_records`` by the
    records' kind; ``mixed``, a :func:`mixed_round`: ``flc_fedopt_fold_mixed_records``, every message by its own
    codec).  False (nothing launched) when the server tensors are not contiguous fp32 tensors of one HIP device
    holding the records' element count (the caller then takes the dense path)."""
    dps = list(delta_params)
    groups = [dps] + ([list(theta)] if theta is not None else []) + ([list(v)] if v is not None else [])
    th, vv = groups[1] if theta is not None else None, groups[-1] if v is not None else None
    n = deltas[0].n
    ws = [float(w) for w in weights]
    step = (float(beta0), _lib.FLC_OPT[opt], float(lr), float(beta2), float(tau))
    if mixed:  # (the descriptor tables are built on the server's device: its check comes first)
        dev = _server_ok(groups, n)
        if dev is None:
            return False
        recs, *cols = _mixed_tables(deltas, dev)
        shape, entries = (n, *cols), _MIXED
    else:
        shape, entries = _record_entries(deltas[0])
        recs = [d.record for d in deltas]
    fast = entries.py_fedopt()
    if fast is not None and dps:
        try:  # one C call: every tensor checked in place; TypeError: nothing launched, the checks below decide
            fast(recs, ws, *shape, dps, th, vv, *step)
            return _folded(len(recs), mixed)
        except TypeError:
            pass
    if mixed:
        shape = (n, *_mixed_ctypes(*cols))
    else:
        dev = _server_ok(groups, n)
        if dev is None:
            return False
        recs = [r if r.device == dev else r.to(dev) for r in recs]
    m, T = len(recs), len(dps)
    with torch.cuda.device(dev):
        _lib.call(entries.fedopt, _ptrs(recs), (ctypes.c_float * m)(*ws), m, *shape, _ptrs(dps),
                  _ptrs(th) if th is not None else None, _ptrs(vv) if vv is not None else None,
                  (ctypes.c_int64 * T)(*[t.numel() for t in dps]), T, *step, codec._stream(dev))
    return _folded(m, mixed)


def fold_gradient_records(deltas: Sequence[CompressedDelta], w_grads: Sequence[float], grads: Sequence[torch.Tensor],
                          params: Optional[Sequence[torch.Tensor]] = None,
                          param_srcs: Optional[Sequence[Sequence[torch.Tensor]]] = None,
                          w_params: Optional[Sequence[float]] = None, inertia: float = 0.0,
                          records: Optional[Sequence[torch.Tensor]] = None, mixed: bool = False) -> bool:
    """``grads = Σ_m w_grads[m]·decode(record_m)`` from +0 in message order and, with ``params``,
    ``θ = θ·inertia + Σ_m w_params[m]·param_srcs[m]`` — one ``flc_avg_and_gradient_records`` pass (``params`` None:
    ``update_gradients`` alone; ``flc_avg_and_gradient_sparse_records`` / ``flc_avg_and_gradient_dense_records`` by
    the records' kind; ``mixed``, a :func:`mixed_round`: ``flc_avg_and_gradient_mixed_records``).  ``records``: the
    messages' records where they were staged (default: the deltas' own).  False (nothing launched) when a tensor is
    not a contiguous fp32 tensor of the gradients' HIP device holding the records' element count (the caller then
    takes the dense path); records and parameter sources elsewhere are moved."""
    gs = list(grads)
    n, m = deltas[0].n, len(deltas)
    ps = srcs = None
    if params is not None:
        ps = [p.data if isinstance(p, torch.nn.Parameter) else p for p in params]
    dev = _server_ok([gs] + ([ps] if ps is not None else []), n)
    if dev is None:
        return False
    if ps is not None:
        srcs = [[t.detach() if t.device == dev else t.detach().to(dev) for t in r] for r in param_srcs]
        if len(srcs) != m or _server_ok([gs] + srcs, n) is None:
            return False
    recs, shape, entries = _round_records(deltas, dev, mixed, records)
    T = len(gs)
    fl = lambda ws: (ctypes.c_float * m)(*[float(w) for w in ws])  # noqa: E731
    with torch.cuda.device(dev):
        _lib.call(entries.gradient, _ptrs(ps) if ps is not None else None, _ptrs(gs),
                  _ptrs([t for r in srcs for t in r]) if srcs is not None else None, _ptrs(recs),
                  fl(w_params) if ps is not None else None, fl(w_grads), m, *shape,
                  (ctypes.c_int64 * T)(*[g.numel() for g in gs]), T, float(inertia), codec._stream(dev))
    return _folded(m, mixed)


def fold_record_groups(groups: Sequence[Tuple[Sequence[CompressedDelta], Sequence[float], Sequence[torch.Tensor]]],
                       records: Optional[Sequence[Optional[Sequence[torch.Tensor]]]] = None,
                       mixed: bool = False) -> bool:
    """For every ``(deltas, weights, dst_tensors)`` of ``groups``: ``dst += Σ_c w_c·decode(record_c)`` in place, in
    the group's message order (``add_parameters``' accumulation) — all groups in one ``flc_fold_record_groups`` pass
    (``flc_fold_sparse_record_groups`` / ``flc_fold_dense_record_groups`` by the records' kind; ``mixed``:
    ``flc_fold_mixed_record_groups``, the messages differing in codec within a group or between groups).
    A group without deltas is left alone.  ``records[g]``: group ``g``'s records where they were staged (default: the
    deltas' own).  False (nothing launched) when the records are not of one codec and shape (``mixed``: of one n), or
    a destination tensor is not a contiguous fp32 tensor of one HIP device, or the groups' tensors do not all hold the
    records' element counts tensor by tensor, or two groups share a destination (the caller then takes the dense
    path); records on another device are moved."""
    recs_of = list(records) if records is not None else [None] * len(groups)
    live = [(list(ds), [float(w) for w in ws], [p.data if isinstance(p, torch.nn.Parameter) else p for p in dst], rs)
            for (ds, ws, dst), rs in zip(groups, recs_of) if len(ds)]
    if not live:
        return True
    d0 = live[0][0][0]
    if mixed:
        if any(d.n != d0.n for ds, _, _, _ in live for d in ds):
            return False
    elif d0.kind == "dense" or any(d.codec_key != d0.codec_key for ds, _, _, _ in live for d in ds):
        return False
    if any(len(ws) != len(ds) or (rs is not None and len(rs) != len(ds)) for ds, ws, _, rs in live):
        return False
    shape, entries = ((), _MIXED) if mixed else _record_entries(d0)
    fast = entries.py_groups() if entries.py_groups is not None else None  # (stacked records only)
    if fast is not None:
        try:  # one C call: every tensor checked in place; TypeError: nothing launched, the checks below decide
            fast([[d.record for d in ds] if rs is None else rs for ds, _, _, rs in live],
                 [ws for _, ws, _, _ in live], [dst for _, _, dst, _ in live], *shape)
            return True
        except TypeError:
            pass
    dev = _server_ok([dst for _, _, dst, _ in live], d0.n, distinct=True)
    if dev is None:
        return False
    ds = [d for g, _, _, _ in live for d in g]
    staged = [r for g, _, _, rs in live for r in (rs if rs is not None else [None] * len(g))]
    recs, shape, _ = _round_records(ds, dev, mixed, staged)
    ws = [w for _, g, _, _ in live for w in g]
    gof = [i for i, (g, _, _, _) in enumerate(live) for _ in g]
    m, T = len(recs), len(live[0][2])
    with torch.cuda.device(dev):
        _lib.call(entries.groups, _ptrs(recs), (ctypes.c_float * m)(*ws), (ctypes.c_int32 * m)(*gof), m, *shape,
                  _ptrs([t for _, _, dst, _ in live for t in dst]), len(live),
                  (ctypes.c_int64 * T)(*[t.numel() for t in live[0][2]]), T, codec._stream(dev))
    return _folded(m, mixed)


def fold_mixed_records(deltas: Sequence[CompressedDelta], weights: Sequence[float],
                       delta_params: Sequence[torch.Tensor], theta: Optional[Sequence[torch.Tensor]],
                       v: Optional[Sequence[torch.Tensor]], beta0: float, opt: str = "avg", lr: float = 1.0,
                       beta2: float = 0.0, tau: float = 0.0) -> bool:
    """:func:`fold_records` for a :func:`mixed_round`: every message by its own codec, one
    ``flc_fedopt_fold_mixed_records`` pass."""
    return fold_records(deltas, weights, delta_params, theta, v, beta0, opt, lr, beta2, tau, mixed=True)


def fold_mixed_record_groups(groups: Sequence[Tuple[Sequence[CompressedDelta], Sequence[float],
                                                    Sequence[torch.Tensor]]]) -> bool:
    """:func:`fold_record_groups` for groups whose messages differ in codec, within a group or between groups: one
    ``flc_fold_mixed_record_groups`` pass."""
    return fold_record_groups(groups, mixed=True)


def fold_mixed_gradient_records(deltas: Sequence[CompressedDelta], w_grads: Sequence[float],
                                grads: Sequence[torch.Tensor], params: Optional[Sequence[torch.Tensor]] = None,
                                param_srcs: Optional[Sequence[Sequence[torch.Tensor]]] = None,
                                w_params: Optional[Sequence[float]] = None, inertia: float = 0.0) -> bool:
    """:func:`fold_gradient_records` for a :func:`mixed_round` of gradients: one
    ``flc_avg_and_gradient_mixed_records`` pass."""
    return fold_gradient_records(deltas, w_grads, grads, params, param_srcs, w_params, inertia, mixed=True)


def _compressors_of(node, name: str = "compressors") -> List[Compressor]:
    cs = getattr(node, name, None)
    if cs is None:
        cs = getattr(getattr(node, "config", None), name, None)
    if cs is None:
        return []
    return [cs] if isinstance(cs, Compressor) else list(cs)


def _wire_records(node) -> bool:
    """``wire_records`` looked up on the client, then on its config (as ``error_feedback`` is); absent or false: the
    dithering quantizers and the natural compressor send their decoded vectors."""
    v = getattr(node, "wire_records", None)
    if v is None:
        v = getattr(getattr(node, "config", None), "wire_records", None)
    return bool(v)


def _quant_bucket(node) -> int:
    """``quant_bucket`` looked up on the client, then on its config (as ``wire_records`` is); absent or 0: the
    dithering quantizers scale the whole vector by one norm (or by their own ``Compressor.bucket``)."""
    v = getattr(node, "quant_bucket", None)
    if v is None:
        v = getattr(getattr(node, "config", None), "quant_bucket", None)
    return int(v or 0)


def _sparse_records(node) -> bool:
    """``sparse_records`` looked up on the client, then on its config (as ``wire_records`` is); absent or false: the
    top-k and rand-k compressors send their decoded vectors."""
    v = getattr(node, "sparse_records", None)
    if v is None:
        v = getattr(getattr(node, "config", None), "sparse_records", None)
    return bool(v)


class CompressedFedOptClientMixin(ErrorFeedbackClientMixin):
    """Mix in before the reference's ``FedOptClient`` (``class C(CompressedFedOptClientMixin, FedOptClient)``):
    ``communicate`` (_fedopt.py:295-308) sends the delta through the client's compressors (``self.compressors``, or
    ``self.config.compressors``: one :class:`~fl_sim_amd.compressors.Compressor` or a sequence applied in order; none
    sends the plain delta).  The server side is :class:`~fl_sim_amd.aggregation.FedOptUpdateMixin`, which folds a
    round of stacked records in one pass (or any reference server, which reads the message's delta unchanged).
    ``self.error_feedback`` (or ``self.config.error_feedback``) truthy: error feedback through the memory
    ``self.error_memory("delta_parameters")`` (fl_sim_amd/feedback.py)."""

    def communicate(self, target) -> None:
        # (the parameters as they are: the codec only reads them, and every converting path detaches first)
        params = list(self.model.parameters())
        delta = compress_delta(params, self._cached_parameters, _compressors_of(self),
                               self._feedback_for("delta_parameters", params), wire=_wire_records(self),
                               sparse=_sparse_records(self), bucket=_quant_bucket(self))
        target._received_messages.append(
            client_message_class()(
                **{
                    "client_id": self.client_id,
                    "delta_parameters": delta,
                    "train_samples": len(self.train_loader.dataset),
                    "metrics": self._metrics,
                }
            )
        )


class CompressedSCAFFOLDClientMixin(ErrorFeedbackClientMixin):
    """Mix in before the reference's ``SCAFFOLDClient`` (``class C(CompressedSCAFFOLDClientMixin, SCAFFOLDClient)``):
    ``communicate`` (scaffold/_scaffold.py:210-222) sends ``parameters_delta`` through the client's ``compressors`` and
    ``control_variates_delta`` through its ``control_compressors`` (each looked up on the client, then on its config:
    one :class:`~fl_sim_amd.compressors.Compressor` or a sequence applied in order; a missing set sends that vector as
    the reference does), in that order, then applies the reference's side effects (the control variates take the
    updated ones, which are released).  In philox mode with the stacked pipeline both records join the round's one
    batched encode, each with its own counter; the deferred encode reads a snapshot of the flat delta taken here, so
    overwriting the control variates afterwards is safe.  The server side is
    :class:`~fl_sim_amd.aggregation.SCAFFOLDUpdateMixin`, which folds both vectors' records in one pass (or any
    reference server: the compressed deltas read as lists of tensors).  With ``error_feedback`` the two vectors keep
    two memories, ``self.error_memory("parameters_delta")`` and ``self.error_memory("control_variates_delta")``."""

    def communicate(self, target) -> None:
        cs, ccs = _compressors_of(self), _compressors_of(self, "control_compressors")
        params = list(self.model.parameters())
        if cs:
            pd = compress_delta(params, self._cached_parameters, cs, self._feedback_for("parameters_delta", params),
                                wire=_wire_records(self), sparse=_sparse_records(self), bucket=_quant_bucket(self))
        else:
            pd = [mp.detach().sub(cp) for mp, cp in zip(params, self._cached_parameters)]
        if ccs:
            ucvs = list(self._updated_control_variates)
            cd = compress_delta(ucvs, self._control_variates, ccs, self._feedback_for("control_variates_delta", ucvs),
                                wire=_wire_records(self), sparse=_sparse_records(self), bucket=_quant_bucket(self))
        else:
            cd = [ucv.sub(cv) for ucv, cv in zip(self._updated_control_variates, self._control_variates)]
        target._received_messages.append(
            client_message_class()(
                **{
                    "client_id": self.client_id,
                    "parameters_delta": pd,
                    "control_variates_delta": cd,
                    "train_samples": len(self.train_loader.dataset),
                    "metrics": self._metrics,
                }
            )
        )
        for cv, ucv in zip(self._control_variates, self._updated_control_variates):
            cv.copy_(ucv)
        del self._updated_control_variates  # free memory
        self._updated_control_variates = None


class CompressedIFCAClientMixin(ErrorFeedbackClientMixin):
    """Mix in before the reference's ``IFCAClient`` (``class C(CompressedIFCAClientMixin, IFCAClient)``):
    ``communicate`` (ifca/_ifca.py:228-240) sends the delta through the client's compressors
    (:class:`CompressedFedOptClientMixin`'s message) and the client's ``cluster_id`` beside it.  The server side is
    :class:`~fl_sim_amd.aggregation.IFCAUpdateMixin`, which folds every cluster's records in one pass (or any
    reference server).  ``error_feedback``: as for :class:`CompressedFedOptClientMixin`."""

    def communicate(self, target) -> None:
        params = list(self.model.parameters())
        delta = compress_delta(params, self._cached_parameters, _compressors_of(self),
                               self._feedback_for("delta_parameters", params), wire=_wire_records(self),
                               sparse=_sparse_records(self), bucket=_quant_bucket(self))
        target._received_messages.append(
            client_message_class()(
                **{
                    "client_id": self.client_id,
                    "cluster_id": self.cluster_id,
                    "delta_parameters": delta,
                    "train_samples": len(self.train_loader.dataset),
                    "metrics": self._metrics,
                }
            )
        )


def compress_message_gradients(message, compressors: Sequence[Compressor], feedback=None, wire: bool = False,
                               sparse: bool = False, bucket: int = 0) -> None:
    """Replace ``message["gradients"]`` (a list of tensors) with the :class:`CompressedDelta` made from them
    (:func:`compress_tensors`); no compressors, no gradients or gradients already compressed: the message as it is.
    ``feedback``: the client's error memory for the vector, or a callable that makes it from the gradient list (called
    only when a message is compressed), or None."""
    gs = message.get("gradients")
    if not compressors or gs is None or isinstance(gs, CompressedDelta) or len(gs) == 0:
        return
    gs = list(gs)
    message["gradients"] = compress_tensors(gs, compressors, feedback(gs) if callable(feedback) else feedback, wire,
                                            sparse, bucket)


class CompressedGradientsClientMixin(ErrorFeedbackClientMixin):
    """Mix in before the reference's ``FedProxClient``, ``FedPDClient``, ``ProxSkipClient`` or ``pFedMacClient``
    (``class C(CompressedGradientsClientMixin, FedProxClient)``): the client's own ``communicate``
    (fedprox/_fedprox.py:208-217, fedpd/_fedpd.py:252-275, proxskip/_proxskip.py:265-276, pfedmac/_pfedmac.py:203-212)
    runs as it is, and the ``gradients`` of every message it appended (``config.vr``) go through the client's
    compressors (``self.gradient_compressors``, or ``self.config.gradient_compressors``: one
    :class:`~fl_sim_amd.compressors.Compressor` or a sequence applied in order; none leaves the message unchanged).
    A client that skips the round appends nothing, so nothing is compressed and no compressor advances; ``parameters``
    stay as the reference sends them.  The server side is :class:`~fl_sim_amd.aggregation.VRUpdateMixin`, which folds a
    round of stacked, dense or sparse records and the dense parameters in one pass (or any reference server: the
    compressed gradients read as a list of tensors).  With ``error_feedback`` the gradients go through the memory
    ``self.error_memory("gradients")``; a client that skips the round touches no memory."""

    def communicate(self, target) -> None:
        received = target._received_messages
        before = len(received)
        super().communicate(target)
        cs = _compressors_of(self, "gradient_compressors")
        if not cs:
            return
        for m in target._received_messages[before if target._received_messages is received else 0:]:
            if isinstance(m, dict) and "gradients" in m:
                compress_message_gradients(m, cs, lambda gs: self._feedback_for("gradients", gs), _wire_records(self),
                                           _sparse_records(self), _quant_bucket(self))
