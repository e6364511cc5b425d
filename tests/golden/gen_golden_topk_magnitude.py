#!/usr/bin/env python3
"""Fixture for top-k by magnitude: ``tests/golden/topk_magnitude.npz``.

Top-k by magnitude keeps the index set the reference's own TopK compressor (compressors.py:293-296) keeps on ``|x|``,
and each kept value is ``x``'s own.  The reference is run from its sources at ``REF`` (none of its text is kept here):
its TopK compressor on ``np.abs(x)`` gives the kept mask.  The inputs have pairwise distinct non-zero magnitudes and
mixed signs, so the reference's unstable argsort has no ties to resolve.  For the stacked pipeline the reference's
standard dithering (identical norm compressor, p = inf) then runs on ``x * mask`` with ``random`` seeded per case.

Stored: the inputs once per size as ``x_n<n>``; per ``n<n>_K<K>`` the mask ``|mask`` (uint8); per
``n<n>_K<K>_s<s>`` the output ``|out``, ``|stats`` (the dithering compressor's ``really_need_to_send_components`` and
``total_input_components``, then the norm compressor's) and ``|next_random`` (the next ``random.random()``).

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

MAG_NS = (7, 1000, 5000)
MAG_LEVELS = (1, 7, 10)


def mag_ks(n: int):
    return (1, n // 100 or 3, n - 1)


def mag_cases():
    for n in MAG_NS:
        for K in mag_ks(n):
            yield n, K


def mag_key(n: int, K: int) -> str:
    return f"n{n}_K{K}"


def mag_seed(n: int, K: int, s: int) -> int:
    return 3300 + 101 * MAG_NS.index(n) + 17 * mag_ks(n).index(K) + s


def mag_input(n: int) -> np.ndarray:
    """Seeded input of n elements (the global streams are not touched): no zeros, mixed signs, distinct magnitudes."""
    x = make_input(n, 54, zero_frac=0.0)  # (seed 54: the first with no two equal magnitudes at every size)
    assert np.all(x != 0) and len(np.unique(np.abs(x))) == n and (x < 0).any() and (x > 0).any()
    return x


def gen_topk_magnitude() -> None:
    ref = load_reference_compressors()
    store: Dict[str, Any] = {}
    for n in MAG_NS:
        store[f"x_n{n}"] = mag_input(n)
    for n, K in mag_cases():
        x = mag_input(n)
        tk = ref.Compressor()
        tk.makeTopKCompressor(K, n)
        mask = np.asarray(tk.compressVector(np.abs(x))) != 0
        assert int(mask.sum()) == K  # (no zero magnitudes: the kept entries are the nonzero ones)
        store[mag_key(n, K) + "|mask"] = mask.astype(np.uint8)
        for s in MAG_LEVELS:
            random.seed(mag_seed(n, K, s))
            nc = ref.Compressor("norm")
            nc.makeIdenticalCompressor()
            sd = ref.Compressor()
            sd.makeStandardDitheringFP32(s, nc, p=np.inf)
            o = sd.compressVector(x * mask)
            c = np.ascontiguousarray(o, dtype=np.float32)
            assert np.array_equal(c.astype(np.asarray(o).dtype), o)  # (nothing lost in fp32)
            key = f"{mag_key(n, K)}_s{s}"
            store[key + "|out"] = c
            store[key + "|stats"] = np.array(
                [float(sd.really_need_to_send_components), float(sd.total_input_components),
                 float(nc.really_need_to_send_components), float(nc.total_input_components)], dtype=np.float64)
            store[key + "|next_random"] = np.array(random.random())
    np.savez_compressed(OUT / "topk_magnitude.npz", **store)
    print("topk_magnitude.npz:", len(store), "arrays")


def main() -> int:
    if not REF.exists():
        print("reference not present; nothing to do", file=sys.stderr)
        return 1
    gen_topk_magnitude()
    return 0


if __name__ == "__main__":
    sys.exit(main())
