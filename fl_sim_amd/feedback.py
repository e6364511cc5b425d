"""Error feedback for the compressed client messages: a per-client residual memory for biased compressors.

The call site's headline compressor (top-k 1 % then 8-bit dithering) is biased (``Compressor.is_biased``): every round
it drops 99 % of the update's coordinates.  Error feedback keeps what was not sent and adds it to the next round's
message.  For one client and one message vector, with memory ``e`` (flat fp32, ``n`` elements, zero at the start)::

    a  = fp32(e + fp32(local − cached))     # a gradient list: a = fp32(e + x)
    c  = compressors(a)                     # Compressor.compressVector (compressors.py:267-410), applied in order
    e' = fp32(a − c)

The message is exactly what :func:`~fl_sim_amd.compressed.compress_delta` sends for the input ``a`` (a packed stacked
record, or the decoded flat vector), with the same statistics and RNG advance; the server side does not change.

:class:`ErrorMemory` owns ``e``.  It *is* the flat input of the encoders: ``flc_ef_accumulate`` writes ``a`` into it in
place, the (deferred, batched) stacked encode reads it, and ``flc_ef_residual_round`` subtracts what the round's records
carry at their K kept entries — ``e'`` equals ``a`` everywhere else bit for bit, so no dense pass follows the encode.
A dithering quantizer's dense record changes every element; there the batched encode itself
(``flc_quant_encode_residual_round``, opt-in: ``compressed.EF_DENSE_DEFER``) stores ``a − decode(code)`` back to the
positions it read, so again nothing is decoded and no pass follows.
A NaN or inf that enters the memory stays there, as the expression says; :meth:`ErrorMemory.reset` is the way out.
"""

from __future__ import annotations

from typing import Optional

import torch


class ErrorMemory:
    """The residual memory of one client and one message vector: ``n`` fp32 elements on HIP device ``device``,
    allocated zeroed on first use.  Pass it as ``feedback=`` to :func:`~fl_sim_amd.compressed.compress_delta` /
    :func:`~fl_sim_amd.compressed.compress_tensors`.

    While a deferred batched encode still reads the memory (and owes it the residual), the tensor holds ``a``;
    :meth:`value` and :meth:`reset` run that encode first.  The memory remembers the stream that wrote it last; a
    call on another stream waits for that stream before it touches the tensor."""

    def __init__(self, n: int, device=None):
        self.n = int(n)
        if self.n < 0:
            raise ValueError("an error memory holds n >= 0 elements")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise ValueError("an error memory lives on a HIP device (the encode's device)")
        self.device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self._e: Optional[torch.Tensor] = None
        self._stream = None  # the torch stream that wrote the tensor last
        self._batch = None   # the pending batched encode that reads the tensor and owes it a residual

    def _settle(self) -> None:
        """Run the pending batched encode that still owes this memory its residual (it raises what the encode
        raises; the memory then still holds ``a`` and stays pending)."""
        b = self._batch
        if b is not None:
            b.run()

    def _acquire(self) -> torch.Tensor:
        """The tensor, for a write on the current stream of the memory's device: allocated on first use; the current
        stream first waits for the stream that wrote it last, and becomes the last writer."""
        cur = torch.cuda.current_stream(self.device)
        if self._e is None:
            with torch.cuda.device(self.device):
                self._e = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        elif self._stream is not None and self._stream.cuda_stream != cur.cuda_stream:
            cur.wait_stream(self._stream)
            self._e.record_stream(cur)
        self._stream = cur
        return self._e

    def _written(self, stream) -> None:
        """A batched encode applied the residual on ``stream``."""
        self._batch = None
        self._stream = stream

    def value(self) -> torch.Tensor:
        """The memory tensor ``e`` (not a copy), after any pending deferred encode that still owes it a residual has
        run; ordered after the memory's last write on the current stream."""
        self._settle()
        return self._acquire()

    def reset(self) -> None:
        """Zero the memory (after running pending work): forgets every residual, a NaN or inf included."""
        self._settle()
        self._acquire().zero_()

    def __repr__(self) -> str:
        return f"ErrorMemory(n={self.n}, device={self.device}, pending={self._batch is not None})"


def feedback_enabled(node) -> bool:
    """``error_feedback`` looked up on the client, then on its config; absent or false: off."""
    v = getattr(node, "error_feedback", None)
    if v is None:
        v = getattr(getattr(node, "config", None), "error_feedback", None)
    return bool(v)


class ErrorFeedbackClientMixin:
    """The memories of a compressed client: one :class:`ErrorMemory` per message vector, kept on the client and made
    when the vector is first sent with ``error_feedback`` on."""

    def error_memory(self, key: str) -> Optional[ErrorMemory]:
        """The :class:`ErrorMemory` of message vector ``key`` (``"delta_parameters"``, ``"gradients"``,
        ``"parameters_delta"``, ``"control_variates_delta"``), or None when that vector has not been sent with error
        feedback on."""
        return getattr(self, "_error_memories", {}).get(key)

    def _feedback_for(self, key: str, tensors) -> Optional[ErrorMemory]:
        """The memory ``key`` for a message made of ``tensors`` (None: feedback off)."""
        if not feedback_enabled(self):
            return None
        mems = self.__dict__.setdefault("_error_memories", {})
        m = mems.get(key)
        if m is None:
            ts = list(tensors)
            t0 = ts[0]
            dev = t0.device if t0.is_cuda else torch.device("cuda", torch.cuda.current_device())
            m = mems[key] = ErrorMemory(sum(t.numel() for t in ts), dev)
        return m
