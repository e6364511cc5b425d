"""Error feedback restated for the tests (the meaning of fl_sim_amd/feedback.py) as a loop around the oracle's
compressors: for one client with memory ``e`` (fp32, zero at the start), per round

    a  = fp32(e + x)          x = fp32(local − cached), or the flat gradient list
    c  = compressors(a)       oracle.round_ref.compress (compat) / oracle.compressors_ref.stacked (philox)
    e' = fp32(a − c)

in numpy float32 arithmetic (one rounding per operation).  Pinned by tests/golden/ef_codec.npz
(tests/test_ef_oracle.py)."""

from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

from oracle import compressors_ref as ref
from oracle import round_ref


def accumulate(e: np.ndarray, x: np.ndarray) -> np.ndarray:
    a = e + np.ascontiguousarray(x, dtype=np.float32)
    assert a.dtype == np.float32
    return a


class CompatClient:
    """One client's memory and accumulated send statistics under the compat RNG (the global streams; the caller seeds
    them and runs the clients of a round in order)."""

    def __init__(self, codec: str, n: int):
        self.codec, self.e = codec, np.zeros(n, dtype=np.float32)
        self.sent: List[float] = []
        self.inputs: List[float] = []
        self.last: List[float] = []

    def round(self, x: np.ndarray) -> np.ndarray:
        """The decoded vector ``c`` the round's message carries; the memory becomes ``a − c``."""
        a = accumulate(self.e, x)
        out, sends, ins = round_ref.compress(self.codec, a)
        c = np.ascontiguousarray(out, dtype=np.float32)
        self.e = a - c
        if not self.sent:
            self.sent, self.inputs = [0.0] * len(sends), [0.0] * len(ins)
        self.sent = [s + float(v) for s, v in zip(self.sent, sends)]
        self.inputs = [s + float(v) for s, v in zip(self.inputs, ins)]
        self.last = [float(v) for v in sends]
        return c

    def stats_row(self) -> List[float]:
        """As tests/golden/gen_golden_ef.py stores it: sent per stage, inputs per stage, last send per stage."""
        return self.sent + self.inputs + self.last


def philox_round(e: np.ndarray, x: np.ndarray, K: int, levels: int, seed: int,
                 counter: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.float32]:
    """One philox-mode round of the stacked pipeline: (c, e', kept indices, codes, norm) for the memory ``e`` and the
    round's flat input ``x`` with the dithering stage's Philox (seed, counter)."""
    a = accumulate(e, x)
    c, kept, codes, norm = ref.stacked(a, K, levels, ref.philox_stream(seed, counter, a.shape[0]), fast=True)
    c = np.ascontiguousarray(c, dtype=np.float32)
    return c, a - c, kept, codes, norm


def record_fields(d) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(idx, codes, norm) of a stacked CompressedDelta's record, on the host."""
    from fl_sim_amd import codec

    pk = codec.wire_packet(d.record, d.n, d.k, d.levels)
    return pk.idx.cpu().numpy().astype(np.int64), pk.codes[:d.k].cpu().numpy(), pk.norm.cpu().numpy()[0]


def flat_of(tensors: Sequence) -> np.ndarray:
    import torch

    return torch.cat([t.detach().reshape(-1).cpu() for t in tensors]).numpy()
