"""Pin the oracle to the reference's variance-reduced round with compressed gradients (tests/golden/vr_codec.npz,
gen_golden_vr_codec.py: the algorithm's own client ``communicate`` -> ``Compressor.compressVector`` on the flattened
gradients -> the algorithm's own server ``update``, run from the reference's sources): ``round_ref.compress`` on the
flattened gradients, then ``aggregation_ref.avg_parameters`` / ``update_gradients`` — θ and the gradients bit for bit
(small) or by SHA-256 (config1), every client's send statistics and both global streams in lock-step.  And
``compressed.stacked_round`` on a gradients round, from hand-built messages.  CPU only."""

import random

import numpy as np
import pytest
import torch

from oracle import aggregation_ref as agg_ref
from oracle import round_ref
from tests import golden_cases as gc
from tests.golden.gen_golden import CONFIG1_SHAPES, PFEDMAC_BETA, SMALL_SHAPES, VR_SERVERS, vr_inputs
from tests.golden.gen_golden_vr_codec import VR_CODEC_MSGS, VR_CODECS, vr_codec_key, vr_codec_seed

VRC = np.load(f"{gc.GOLDEN}/vr_codec.npz", allow_pickle=False)


def flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).numpy()


def same(key, field, ts):
    a = flat(ts)
    if f"{key}|{field}|out" in VRC.files:
        return gc.same_bits(a, VRC[f"{key}|{field}|out"])
    return gc.sha(a) == str(VRC[f"{key}|{field}|sha"])


def test_fixture_holds_every_case():
    keys = {k.split("|")[0] for k in VRC.files}
    want = {vr_codec_key(s, c, nm, tag) for s in VR_SERVERS for c in VR_CODECS for nm in VR_CODEC_MSGS
            for tag in ("small", "config1")}
    assert keys == want
    for k in want:
        assert (f"{k}|theta|out" in VRC.files) == k.endswith("_small")


@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("nm", VR_CODEC_MSGS)
@pytest.mark.parametrize("codec", VR_CODECS)
@pytest.mark.parametrize("name", list(VR_SERVERS))
def test_vr_codec_oracle_matches_reference(name, codec, nm, tag):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    params, msgs = vr_inputs(shapes, nm)
    key = vr_codec_key(name, codec, nm, tag)
    gc.seed_all(vr_codec_seed(name, codec, nm, tag))
    stats = []
    for m in msgs:
        out, sends, ins = round_ref.compress(codec, flat(m["gradients"]))
        out_t = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))
        gs, off = [], 0
        for g in m["gradients"]:
            gs.append(out_t[off:off + g.numel()].reshape(g.shape).clone())
            off += g.numel()
        m["gradients"] = gs
        stats.append(sends + ins)
    assert random.random() == float(VRC[key + "|next_random"])
    assert np.random.random_sample() == float(VRC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), VRC[key + "|stats"])
    agg_ref.avg_parameters(params, msgs, inertia=1 - PFEDMAC_BETA if name == "pfedmac" else 0.0)
    assert same(key, "theta", params)
    assert same(key, "grad", agg_ref.update_gradients(params, msgs))


def test_stacked_round_on_gradients():
    """None for a mixed or a dense round (and for another key), the list for a uniform stacked round."""
    from fl_sim_amd import compressed

    shapes, dev = [torch.Size((3, 2)), torch.Size((4,))], torch.device("cpu")

    def rec(k=2, levels=10, n=10):
        return compressed.CompressedDelta(shapes, dev, n, record=torch.zeros(256, dtype=torch.uint8), k=k, levels=levels)

    dense = compressed.CompressedDelta(shapes, dev, 10, flat=torch.zeros(10))
    msgs = [{"gradients": rec(), "parameters": []} for _ in range(3)]
    got = compressed.stacked_round(msgs, key="gradients")
    assert got is not None and [id(d) for d in got] == [id(m["gradients"]) for m in msgs]
    assert compressed.stacked_round(msgs) is None  # (no delta_parameters in these messages)
    assert compressed.stacked_round([], key="gradients") is None
    assert compressed.stacked_round(msgs + [{"gradients": dense}], key="gradients") is None
    assert compressed.stacked_round(msgs + [{"gradients": [torch.zeros(3, 2), torch.zeros(4)]}], key="gradients") is None
    assert compressed.stacked_round([{"gradients": dense}] * 2, key="gradients") is None
    assert compressed.stacked_round(msgs + [{"parameters": []}], key="gradients") is None
    for other in (rec(k=3), rec(levels=8)):
        assert compressed.stacked_round(msgs + [{"gradients": other}], key="gradients") is None
    # the mixin's compressor lookup and entry points exist beside the FedOpt ones
    assert callable(compressed.compress_tensors) and callable(compressed.compress_message_gradients)
    assert callable(compressed.fold_gradient_records)
    assert hasattr(compressed, "CompressedGradientsClientMixin")
