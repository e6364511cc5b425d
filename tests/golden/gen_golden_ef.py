#!/usr/bin/env python3
"""Fixture for error feedback at the codec's call site: ``tests/golden/ef_codec.npz``.

The reference never compresses a message (see ``gen_golden.py``, ``gen_round``) and has no error feedback; the meaning
is fixed in fl_sim_amd/feedback.py and composed here around the reference's own compressor, run from its sources at
``REF`` (none of its text is kept here).  For one client with memory ``e`` (fp32, zero at the start), per round::

    a  = fp32(e + fp32(local − cached))      # numpy float32 arithmetic, one rounding per operation
    c  = compressors(a)                      # Compressor.compressVector (compressors.py:267-410), applied in order
    e' = fp32(a − c)

``EF_CLIENTS`` clients × ``EF_ROUNDS`` rounds; one compressor set per client, kept across the rounds (its send
statistics accumulate); every round's models come from ``ef_inputs`` (a seeded ``torch.Generator``: the global streams
are not touched); ``random`` / ``np.random`` are seeded once per case (``ef_seed``) and consumed in client order within
a round.  Stored per case ``ef_<codec>_<tag>``: ``c<round>_<client>`` (the decoded vector each message carries) and
``e<client>`` (the final memories) as SHA-256, the small shape also in full; ``stats`` (per client, after the last
round: every stage's ``really_need_to_send_components``, then every stage's ``total_input_components``, then every
stage's ``last_need_to_send_advance``); ``next_random`` / ``next_np`` (the streams' next draws).

The constants and inputs below import without the reference; only ``main`` needs it.
"""

from __future__ import annotations

import random
import sys
from pathlib import Path
from typing import Any, Dict

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from tests.golden.gen_golden import (CONFIG1_SHAPES, OUT, REF, SMALL_SHAPES, load_reference_compressors,  # noqa: E402
                                     make_model, reference_round_compressors, sha)

EF_CODECS = ("stacked10", "topk", "std8inf", "natural")
EF_CLIENTS = 4
EF_ROUNDS = 3
EF_TAGS = {"small": SMALL_SHAPES, "config1": CONFIG1_SHAPES}
# input seed at which the K-th largest value of every a = e + delta (every codec, client and round, both shapes) is
# unique, so the reference's unstable argsort (compressors.py:294-295, over the signed values) has no choice among
# ties: main asserts it
EF_INPUT_SEED = 130


def ef_key(codec: str, tag: str) -> str:
    return f"ef_{codec}_{tag}"


def ef_seed(codec: str, tag: str) -> int:
    """The case's seed of both global streams.  (As for ``round_seed``: the natural compressor compares its draw with
    an fp32 probability, in float32 under numpy 2 and in float64 under the reference's pinned numpy < 2; a draw within
    half an fp32 ulp below the probability would make the two disagree.  tests/test_ef_oracle.py, which follows
    numpy < 2, reproduces the fixture bit for bit, so no draw of these seeds falls there.)"""
    return 1300 + 11 * EF_CODECS.index(codec) + (0 if tag == "small" else 1)


def ef_inputs(shapes):
    """(cached, locals_): the model every client trains from, and ``locals_[r][i]``: client i's model after round
    r's training — cached plus noise, so a round's delta is ``locals_[r][i] − cached``."""
    cached = [p.detach().clone() for p in make_model(shapes, 70).parameters()]
    g = torch.Generator().manual_seed(EF_INPUT_SEED)
    locals_ = [[[t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached] for _ in range(EF_CLIENTS)]
               for _ in range(EF_ROUNDS)]
    return cached, locals_


def flat_delta(local, cached) -> np.ndarray:
    """fp32(local − cached), flattened (FedOptClient.communicate's delta, _fedopt.py:294-297)."""
    return torch.cat([(lo - c).reshape(-1) for lo, c in zip(local, cached)]).numpy()


def gen_ef() -> None:
    ref = load_reference_compressors()
    store: Dict[str, Any] = {}
    for tag, shapes in EF_TAGS.items():
        full = tag == "small"
        cached, locals_ = ef_inputs(shapes)
        D = sum(int(np.prod(s)) for s in shapes)
        K = D // 100

        def put(key, flat):
            store[key + "|sha"] = np.array(sha(flat))
            if full:
                store[key + "|out"] = flat

        for codec in EF_CODECS:
            key = ef_key(codec, tag)
            seed = ef_seed(codec, tag)
            random.seed(seed)
            np.random.seed(seed)
            comps = [reference_round_compressors(ref, codec, D) for _ in range(EF_CLIENTS)]
            mem = [np.zeros(D, dtype=np.float32) for _ in range(EF_CLIENTS)]
            for r in range(EF_ROUNDS):
                for i in range(EF_CLIENTS):
                    a = mem[i] + flat_delta(locals_[r][i], cached)
                    assert a.dtype == np.float32
                    srt = np.sort(a)
                    assert srt[-K] != srt[-K - 1] and srt[-K] != srt[-K + 1], "a tie at the top-k threshold"
                    out = a
                    for comp in comps[i]:
                        out = comp.compressVector(out)
                    c = np.ascontiguousarray(out, dtype=np.float32)
                    assert np.array_equal(c.astype(np.asarray(out).dtype), out)  # (nothing lost in fp32)
                    mem[i] = a - c
                    put(f"{key}|c{r}_{i}", c)
            for i in range(EF_CLIENTS):
                put(f"{key}|e{i}", mem[i])
            store[key + "|stats"] = np.array(
                [[float(x.really_need_to_send_components) for x in cs] + [float(x.total_input_components) for x in cs]
                 + [float(x.last_need_to_send_advance) for x in cs] for cs in comps], dtype=np.float64)
            store[key + "|next_random"] = np.array(random.random())
            store[key + "|next_np"] = np.array(np.random.random_sample())
    np.savez_compressed(OUT / "ef_codec.npz", **store)
    print("ef_codec.npz:", len(store), "arrays")


def main() -> int:
    if not REF.exists():
        print("reference not present; nothing to do", file=sys.stderr)
        return 1
    torch.set_num_threads(1)
    gen_ef()
    return 0


if __name__ == "__main__":
    sys.exit(main())
