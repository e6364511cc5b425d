"""Pin the oracle to the reference's SCAFFOLD and IFCA rounds with compressed deltas (tests/golden/delta_codec.npz,
gen_golden_delta_codec.py: the algorithm's own client ``communicate`` -> ``Compressor.compressVector`` on every
flattened delta -> the algorithm's own server ``update``, run from the reference's sources): ``round_ref.compress`` on
the flattened deltas, then ``aggregation_ref.scaffold_update`` / ``ifca_update`` — θ, c and the centres bit for bit
(small) or by SHA-256 (config1), the ``client_ids`` lists, every client's send statistics and both global streams in
lock-step.  And ``compressed.stacked_round`` on SCAFFOLD's two keys, from hand-built messages.  CPU only."""

import random

import numpy as np
import pytest
import torch

from oracle import aggregation_ref as agg_ref
from oracle import round_ref
from tests import golden_cases as gc
from tests.golden.gen_golden import CONFIG1_SHAPES, SCAFFOLD_CFG, SMALL_SHAPES
from tests.golden.gen_golden_delta_codec import (DELTA_ALGS, DELTA_CODECS, delta_codec_key, delta_codec_seed,
                                                 ifca_codec_inputs, scaffold_codec_inputs)

DC = np.load(f"{gc.GOLDEN}/delta_codec.npz", allow_pickle=False)


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()


def same(key, field, ts):
    a = flat(ts)
    if f"{key}|{field}|out" in DC.files:
        return gc.same_bits(a, DC[f"{key}|{field}|out"])
    return gc.sha(a) == str(DC[f"{key}|{field}|sha"])


def compressed_delta(codec, local, cached, row):
    """The reference client's delta (``local - cached`` per tensor) through the oracle's codec, reshaped."""
    deltas = [a.sub(b) for a, b in zip(local, cached)]
    out, sends, ins = round_ref.compress(codec, flat(deltas))
    row += sends + ins
    out_t = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))
    ts, off = [], 0
    for d in deltas:
        ts.append(out_t[off:off + d.numel()].reshape(d.shape).clone())
        off += d.numel()
    return ts


def test_fixture_holds_every_case():
    keys = {k.split("|")[0] for k in DC.files}
    want = {delta_codec_key(a, c, tag) for a in DELTA_ALGS for c in DELTA_CODECS for tag in ("small", "config1")}
    assert keys == want
    for k in want:
        fields = {f.split("|")[1] for f in DC.files if f.startswith(k + "|")}
        if "_scaffold_" in k:
            assert fields == {"theta", "cv", "stats", "next_random", "next_np"}
            assert (f"{k}|theta|out" in DC.files) == (f"{k}|cv|out" in DC.files) == k.endswith("_small")
            assert DC[f"{k}|stats"].shape[0] == 10
        else:
            assert fields == {f"center{c}" for c in range(4)} | {f"ids{c}" for c in range(4)} | {
                "stats", "next_random", "next_np"}
            assert all((f"{k}|center{c}|out" in DC.files) == k.endswith("_small") for c in range(4))
            assert DC[f"{k}|stats"].shape[0] == 10


@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("codec", DELTA_CODECS)
def test_scaffold_oracle_matches_reference(codec, tag):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    theta, cvs, clients = scaffold_codec_inputs(shapes)
    key = delta_codec_key("scaffold", codec, tag)
    gc.seed_all(delta_codec_seed("scaffold", codec, tag))
    msgs, stats = [], []
    for src in clients:
        row = []
        pd = compressed_delta(codec, src["local"], src["cached"], row)  # parameters_delta first
        cd = compressed_delta(codec, src["ucv"], src["cv"], row)
        msgs.append({"client_id": src["client_id"], "parameters_delta": pd, "control_variates_delta": cd})
        stats.append(row)
    assert random.random() == float(DC[key + "|next_random"])
    assert np.random.random_sample() == float(DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), DC[key + "|stats"])
    agg_ref.scaffold_update(theta, cvs, msgs, SCAFFOLD_CFG["lr"], SCAFFOLD_CFG["num_clients"])
    assert same(key, "theta", theta)
    assert same(key, "cv", cvs)


@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("codec", DELTA_CODECS)
def test_ifca_oracle_matches_reference(codec, tag):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    centers, clients = ifca_codec_inputs(shapes)
    key = delta_codec_key("ifca", codec, tag)
    gc.seed_all(delta_codec_seed("ifca", codec, tag))
    msgs, stats = [], []
    for src in clients:
        row = []
        d = compressed_delta(codec, src["local"], src["cached"], row)
        msgs.append({"client_id": src["client_id"], "cluster_id": src["cluster_id"], "delta_parameters": d})
        stats.append(row)
    assert random.random() == float(DC[key + "|next_random"])
    assert np.random.random_sample() == float(DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), DC[key + "|stats"])
    before1 = flat(centers[1]["center_model_params"]).copy()
    agg_ref.ifca_update(centers, msgs, 4)
    for c in range(4):
        assert same(key, f"center{c}", centers[c]["center_model_params"]), c
        assert centers[c]["client_ids"] == DC[f"{key}|ids{c}"].tolist(), c
    assert gc.same_bits(flat(centers[1]["center_model_params"]), before1)  # (the idle cluster)


def test_stacked_round_on_the_scaffold_keys():
    """None for a mixed or a dense round (and for another key), the list for a uniform stacked round — per key."""
    from fl_sim_amd import compressed

    shapes, dev = [torch.Size((3, 2)), torch.Size((4,))], torch.device("cpu")

    def rec(k=2, levels=10, n=10):
        return compressed.CompressedDelta(shapes, dev, n, record=torch.zeros(256, dtype=torch.uint8), k=k, levels=levels)

    dense = compressed.CompressedDelta(shapes, dev, 10, flat=torch.zeros(10))
    plain = [torch.zeros(3, 2), torch.zeros(4)]
    msgs = [{"parameters_delta": rec(), "control_variates_delta": rec(k=3)} for _ in range(3)]
    for key in ("parameters_delta", "control_variates_delta"):
        got = compressed.stacked_round(msgs, key)
        assert got is not None and [id(d) for d in got] == [id(m[key]) for m in msgs]
    assert compressed.stacked_round(msgs) is None  # (no delta_parameters in these messages)
    half = [{"parameters_delta": rec(), "control_variates_delta": plain} for _ in range(3)]
    assert compressed.stacked_round(half, "parameters_delta") is not None
    assert compressed.stacked_round(half, "control_variates_delta") is None
    one_dense = msgs + [{"parameters_delta": dense, "control_variates_delta": rec(k=3)}]
    assert compressed.stacked_round(one_dense, "parameters_delta") is None
    assert compressed.stacked_round(one_dense, "control_variates_delta") is not None
    assert compressed.stacked_round(msgs + [{"parameters_delta": rec(levels=8), "control_variates_delta": rec(k=3)}],
                                    "parameters_delta") is None
    # the call site's entry points exist beside the FedOpt and gradient ones
    assert callable(compressed.fold_record_groups)
    assert hasattr(compressed, "CompressedSCAFFOLDClientMixin") and hasattr(compressed, "CompressedIFCAClientMixin")
    assert "flc_fold_record_groups" in __import__("fl_sim_amd._lib", fromlist=["SIGNATURES"]).SIGNATURES
