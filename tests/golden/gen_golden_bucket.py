#!/usr/bin/env python3
"""Fixture for bucketed dithering: ``tests/golden/bucket_codec.npz``.

With bucket size ``B`` the compressor's result on a vector of ``n`` elements is the reference's own
``Compressor.compressVector`` (compressors.py:327-404) applied to the consecutive slices ``x[0:B], x[B:2B], ...`` in
index order on ONE compressor object, the outputs concatenated; the last slice may be short.  The reference is run from
its sources at ``REF`` (none of its text is kept here).  Each case seeds ``random``, makes one reference compressor —
standard dithering with an identical norm compressor, or natural dithering with ``dInput = B`` — and calls it on every
slice.  Stored per case ``<kind><s>_p<p>_B<B>_n<n>``: ``|out`` the concatenated output, ``|pnorm`` the per-bucket
``np.linalg.norm``, ``|stats`` (the compressor's ``really_need_to_send_components`` and ``total_input_components``,
then the norm compressor's, zeros for natural dithering) and ``|next_random`` (the next ``random.random()``); the inputs
once per size as ``x_n<n>`` (5 % exact zeros and a few ``-0.0``).

The constants and inputs below import without the reference; only ``main`` needs it.
"""

from __future__ import annotations

import random
import sys
from pathlib import Path
from typing import Any, Dict

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from tests.golden.gen_golden import OUT, REF, load_reference_compressors, make_input  # noqa: E402

BUCKET_KINDS = (("std", 1), ("std", 7), ("std", 10), ("natd", 3), ("natd", 8))
BUCKET_PS = (np.inf, 2)
BUCKET_SIZES = (64, 512)
BUCKET_NS = (64, 1000, 5000)


def bucket_cases():
    for kind, s in BUCKET_KINDS:
        for p in BUCKET_PS:
            for B in BUCKET_SIZES:
                for n in BUCKET_NS:
                    yield kind, s, p, B, n


def bucket_key(kind: str, s: int, p: float, B: int, n: int) -> str:
    return f"{kind}{s}_p{'inf' if np.isinf(p) else int(p)}_B{B}_n{n}"


def bucket_seed(kind: str, s: int, p: float, B: int, n: int) -> int:
    return 2100 + 97 * BUCKET_KINDS.index((kind, s)) + 31 * BUCKET_PS.index(p) + 7 * BUCKET_SIZES.index(B) + n % 13


def bucket_input(n: int) -> np.ndarray:
    """Seeded input of n elements (the global streams are not touched): 5 % exact zeros, every 97th element -0.0."""
    x = make_input(n, 41)
    x[5::97] = -0.0
    return x


def gen_bucket() -> None:
    ref = load_reference_compressors()
    store: Dict[str, Any] = {}
    for n in BUCKET_NS:
        store[f"x_n{n}"] = bucket_input(n)
    for kind, s, p, B, n in bucket_cases():
        key = bucket_key(kind, s, p, B, n)
        x = bucket_input(n)
        random.seed(bucket_seed(kind, s, p, B, n))
        comp = ref.Compressor()
        nc = None
        if kind == "std":
            nc = ref.Compressor("norm")
            nc.makeIdenticalCompressor()
            comp.makeStandardDitheringFP32(s, nc, p=p)
        else:
            comp.makeNaturalDitheringFP32(s, B, p=p)
        outs, norms = [], []
        for lo in range(0, n, B):
            sl = x[lo:lo + B]
            norms.append(np.linalg.norm(sl, p))
            o = comp.compressVector(sl)
            c = np.ascontiguousarray(o, dtype=np.float32)
            assert np.array_equal(c.astype(np.asarray(o).dtype), o)  # (nothing lost in fp32)
            outs.append(c)
        store[key + "|out"] = np.concatenate(outs)
        store[key + "|pnorm"] = np.array(norms, dtype=np.float32)
        assert all(np.float32(v) == v for v in norms)
        store[key + "|stats"] = np.array(
            [float(comp.really_need_to_send_components), float(comp.total_input_components),
             float(nc.really_need_to_send_components) if nc else 0.0,
             float(nc.total_input_components) if nc else 0.0], dtype=np.float64)
        store[key + "|next_random"] = np.array(random.random())
    np.savez_compressed(OUT / "bucket_codec.npz", **store)
    print("bucket_codec.npz:", len(store), "arrays")


def main() -> int:
    if not REF.exists():
        print("reference not present; nothing to do", file=sys.stderr)
        return 1
    gen_bucket()
    return 0


if __name__ == "__main__":
    sys.exit(main())
