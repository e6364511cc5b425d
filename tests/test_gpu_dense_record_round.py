"""The codec's call site with ``wire_records`` on: the dithering quantizers and the natural compressor send their dense
records (flc_dense_wire_layout) and the servers fold the records (flc_fedopt_fold_dense_records,
flc_fold_dense_record_groups) — against the reference's own rounds (tests/golden/round_codec.npz, delta_codec.npz,
vr_codec.npz, ef_codec.npz: the fixtures that pin the same rounds with the option off), bit for bit, on a device- and a
host-resident server, with every compressor's send statistics and both global streams in lock-step; philox mode
against the same messages with the option off; pickling, fallbacks, error feedback."""

import copy
import pickle
import random
import types

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import test_gpu_delta_codec as tdc
from tests import test_gpu_vr_codec as tvr
from tests.golden.gen_golden import (CONFIG1_SHAPES, ROUND_OPTS, SMALL_SHAPES, VR_SERVERS, round_inputs, round_seed,
                                     vr_inputs)
from tests.golden.gen_golden_delta_codec import (delta_codec_key, delta_codec_seed, ifca_codec_inputs,
                                                 scaffold_codec_inputs)
from tests.golden.gen_golden_ef import EF_CLIENTS, EF_ROUNDS, EF_TAGS, ef_inputs, ef_key, ef_seed
from tests.golden.gen_golden_vr_codec import vr_codec_key, vr_codec_seed
from tests.test_gpu_round import _check_adaptive_tail, _fields, _same, build_round, make_compressors

pytestmark = pytest.mark.gpu
KINDS = ("quant", "natural")
WIRE = {"std8inf": (0, 8, 8), "std4p2": (0, 4, 4), "natural": (2, 0, 16)}  # codec -> (format, levels, bits)


def _n(shapes):
    return sum(int(np.prod(sh)) for sh in shapes)


def _is_record(d, codec, D):
    """The message carries the codec's dense record and nothing else."""
    from fl_sim_amd import _lib
    from fl_sim_amd.compressed import CompressedDelta

    fmt, s, bits = WIRE[codec]
    size = _lib.size("flc_dense_wire_layout", D, fmt, bits, None)
    code_bytes = 2 * D if fmt == 2 else (D * bits + 7) // 8
    assert size == (16 + code_bytes + 255) // 256 * 256 and size < 4 * D  # (the byte ratio: bits / 32 of 4n, + header)
    return (isinstance(d, CompressedDelta) and d.kind == ("natural" if codec == "natural" else "quant")
            and d.kind in KINDS and (d.format, d.levels, d.bits) == (fmt, s, bits) and d.nbytes == size
            and d.record.numel() == size and d._flat is None)


@pytest.fixture(autouse=True)
def _no_leftovers():
    from fl_sim_amd import compressed

    compressed._run_pending()  # (messages earlier tests left waiting)
    yield
    compressed._run_pending()


# ------------------------------------------------------------------------------ 1. compat mode against the reference
@pytest.mark.parametrize("server", ["device", "host"])
@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("opt", list(ROUND_OPTS))
@pytest.mark.parametrize("codec", list(WIRE))
def test_fedopt_round_with_records_matches_reference(codec, opt, tag, server):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    rec = _fields(f"round_{codec}_{opt}_{tag}")
    s, clients = build_round(shapes, opt, "cuda" if server == "device" else "cpu")
    D = _n(shapes)
    stats = []
    gc.seed_all(round_seed(codec, opt, tag))
    for i, c in enumerate(clients):
        c.compressors = make_compressors(codec, D)
        if i % 2:  # (the two places the option is looked up)
            c.wire_records = True
        else:
            c.config = types.SimpleNamespace(wire_records=True)
        c.communicate(s)
        stats.append([float(x.last_need_to_send_advance) for x in c.compressors]
                     + [float(x.total_input_components) for x in c.compressors])
    assert random.random() == float(rec["next_random"])
    assert np.random.random_sample() == float(rec["next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), rec["stats"])
    msgs = s._received_messages
    assert all(_is_record(m["delta_parameters"], codec, D) for m in msgs)
    s.update()
    assert all(m["delta_parameters"]._flat is None for m in msgs)  # (the server never made a dense vector)
    assert _same(rec, "delta", s.delta_parameters)
    if opt == "avg":
        assert _same(rec, "theta", list(s.model.parameters()))
    else:
        _check_adaptive_tail(codec, opt, tag, shapes, s)
    if server == "host":
        assert all(p.is_cpu for p in s.model.parameters())


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_scaffold_round_with_records_matches_reference(codec, tag, where):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    D = _n(shapes)
    theta, cvs, clients = scaffold_codec_inputs(shapes)
    key = delta_codec_key("scaffold", codec, tag)
    s = tdc._scaffold_server(theta, cvs, where)
    stats = []
    gc.seed_all(delta_codec_seed("scaffold", codec, tag))
    for src in clients:
        c = tdc._scaffold_client(src, (codec, codec), D)
        c.config.wire_records = True
        c.communicate(s)
        stats.append(tdc._stats(c.compressors) + tdc._stats(c.config.control_compressors))
    assert random.random() == float(tdc.DC[key + "|next_random"])
    assert np.random.random_sample() == float(tdc.DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tdc.DC[key + "|stats"])
    got = s._received_messages
    assert len(got) == 10 and all(_is_record(m[k], codec, D) for m in got for k in tdc.KEYS)
    s.update()
    assert all(m[k]._flat is None for m in got for k in tdc.KEYS)  # (the grouped fold read the records)
    assert tdc._same(key, "theta", list(s.model.parameters()))
    assert tdc._same(key, "cv", s._control_variates)
    dev = "cuda" if where == "device" else "cpu"
    assert all(p.device.type == dev for p in list(s.model.parameters()) + list(s._control_variates))


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tag", ["small", "config1"])
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_ifca_round_with_records_matches_reference(codec, tag, where):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    D = _n(shapes)
    centers, clients = ifca_codec_inputs(shapes)
    key = delta_codec_key("ifca", codec, tag)
    s = tdc._ifca_server(centers, where)
    stats = []
    gc.seed_all(delta_codec_seed("ifca", codec, tag))
    for src in clients:
        c = tdc._ifca_client(src, codec, D)
        c.wire_records = True
        c.communicate(s)
        stats.append(tdc._stats(c.compressors))
    assert random.random() == float(tdc.DC[key + "|next_random"])
    assert np.random.random_sample() == float(tdc.DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tdc.DC[key + "|stats"])
    got = s._received_messages
    assert all(_is_record(m["delta_parameters"], codec, D) for m in got)
    s.update()
    assert all(m["delta_parameters"]._flat is None for m in got)
    dev = "cuda" if where == "device" else "cpu"
    for c in range(4):
        assert tdc._same(key, f"center{c}", s._cluster_centers[c]["center_model_params"]), c
        assert s._cluster_centers[c]["client_ids"] == tdc.DC[f"{key}|ids{c}"].tolist(), c
        assert all(p.device.type == dev for p in s._cluster_centers[c]["center_model_params"])
    tdc._assert_same(s._cluster_centers[1]["center_model_params"], centers[1]["center_model_params"])  # (idle)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_vr_round_with_gradient_records_falls_back_and_matches_reference(codec, where):
    """The variance-reduced servers have no record fold for these codecs: the message carries the record and the server
    reads it as the list of decoded tensors."""
    name, tag, nm = "fedprox", "small", 10
    assert name in VR_SERVERS
    shapes = SMALL_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, nm)
    key = vr_codec_key(name, codec, nm, tag)
    s = tvr._server(name, params, where)
    stats = []
    gc.seed_all(vr_codec_seed(name, codec, nm, tag))
    for src in msgs:
        c = tvr._client(src)
        c.gradient_compressors = make_compressors(codec, D)
        c.wire_records = True
        c.communicate(s)
        stats.append([float(x.last_need_to_send_advance) for x in c.gradient_compressors]
                     + [float(x.total_input_components) for x in c.gradient_compressors])
    assert random.random() == float(tvr.VRC[key + "|next_random"])
    assert np.random.random_sample() == float(tvr.VRC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tvr.VRC[key + "|stats"])
    got = s._received_messages
    assert len(got) == nm and all(_is_record(m["gradients"], codec, D) for m in got)
    s.update()
    assert tvr._same(key, "theta", list(s.model.parameters()))
    assert tvr._same(key, "grad", [p.grad for p in s.model.parameters()])


@pytest.mark.parametrize("tag", list(EF_TAGS))
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_error_feedback_with_records_matches_the_reference(codec, tag):
    """Error feedback with ``wire`` on: the messages and memories of the option off (tests/golden/ef_codec.npz pins
    those), the message carrying the record."""
    from fl_sim_amd.compressed import compress_delta
    from fl_sim_amd.feedback import ErrorMemory
    from tests.test_gpu_ef_round import EF, _cuda
    from tests.test_gpu_ef_round import _same as ef_same

    shapes = EF_TAGS[tag]
    cached, locals_ = ef_inputs(shapes)
    n, key = _n(shapes), ef_key(codec, tag)
    dc = _cuda(cached)
    comps = [make_compressors(codec, n) for _ in range(EF_CLIENTS)]
    mems = [ErrorMemory(n, "cuda") for _ in range(EF_CLIENTS)]
    gc.seed_all(ef_seed(codec, tag))
    for r in range(EF_ROUNDS):
        for i in range(EF_CLIENTS):
            d = compress_delta(_cuda(locals_[r][i]), dc, comps[i], feedback=mems[i], wire=True)
            assert _is_record(d, codec, n)
            assert ef_same(f"{key}|c{r}_{i}", d.flat().cpu().numpy()), (r, i)
    for i in range(EF_CLIENTS):
        assert ef_same(f"{key}|e{i}", mems[i].value().cpu().numpy()), i
    stats = [[float(x.really_need_to_send_components) for x in cs] + [float(x.total_input_components) for x in cs]
             + [float(x.last_need_to_send_advance) for x in cs] for cs in comps]
    assert np.array_equal(np.array(stats, dtype=np.float64), EF[key + "|stats"])
    assert random.random() == float(EF[key + "|next_random"])
    assert np.random.random_sample() == float(EF[key + "|next_np"])


# ------------------------------------------------------------------------------------------------ 2. philox mode
def _philox_compressor(codec, D, seed):
    from fl_sim_amd import Compressor

    if codec == "natd7":
        c = Compressor(rng="philox", seed=seed)
        c.makeNaturalDitheringFP32(7, D)
        return [c]
    if codec == "std1inf":
        c = Compressor(rng="philox", seed=seed)
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(1, nc, np.inf)
        return [c]
    return make_compressors(codec, D, rng="philox", seed=seed)


def _stat_tuple(c):
    return (c.total_input_components, c.last_input_advance, c.really_need_to_send_components,
            c.last_need_to_send_advance, c.philox.counter)


@pytest.mark.parametrize("codec", ["std8inf", "std4p2", "std1inf", "natd7", "natural"])
def test_philox_records_equal_the_dense_messages(codec):
    """Two sets of identically seeded compressors, ``wire`` off and on, three messages each: the decoded records are
    the dense messages, the statistics and Philox counters agree, and the record's codes are ``Compressor.encode``'s
    packet for the same (seed, counter)."""
    from fl_sim_amd import codec as C
    from fl_sim_amd.compressed import compress_delta

    shapes = CONFIG1_SHAPES if codec in ("std8inf", "natural") else SMALL_SHAPES
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 3)
    D = _n(shapes)
    glob = [t.cuda() for t in theta]
    off, on, enc = (_philox_compressor(codec, D, 77) for _ in range(3))
    for i in range(3):
        loc = [t.cuda() for t in locals_[i]]
        a = compress_delta(loc, glob, off)
        b = compress_delta(loc, glob, on, wire=True)
        assert a.kind == "dense" and b.kind in KINDS and b._flat is None and b.nbytes < a.nbytes
        x = C.delta_flatten(loc, glob)
        pkt = enc[0].encode(x)
        norm, codes = C.dense_wire_views(b.record, D, b.format, b.bits)
        if codec == "natural":
            assert np.array_equal(codes.cpu().numpy(), pkt.cpu().numpy())
        else:
            assert (pkt.kind, pkt.levels, pkt.bits) == (b.format, b.levels, b.bits)
            assert np.array_equal(codes.cpu().numpy(), pkt.codes[:codes.numel()].cpu().numpy())
            assert gc.same_bits(norm.cpu().numpy(), pkt.norms.cpu().numpy())
        assert gc.same_bits(b.flat().cpu().numpy(), a.flat().cpu().numpy())
        assert [tuple(t.shape) for t in b] == [tuple(sh) for sh in shapes]  # list(delta): the model's tensors
        assert gc.same_bits(torch.cat([t.reshape(-1) for t in b]).cpu().numpy(), a.flat().cpu().numpy())
    assert _stat_tuple(off[0]) == _stat_tuple(on[0])
    assert enc[0].philox.counter == on[0].philox.counter


def test_philox_communicate_reads_nothing_back(monkeypatch):
    """``communicate`` with ``wire_records`` on in philox mode performs no device-to-host read: the standard
    dithering's nonzero counts wait in the compressor's device slab until a statistic is first read."""
    from fl_sim_amd import Compressor

    shapes = SMALL_SHAPES
    D = _n(shapes)
    s, clients = build_round(shapes, "avg", "cuda")
    comps = make_compressors("std8inf", D, rng="philox", seed=5)
    want = make_compressors("std8inf", D, rng="philox", seed=5)
    reads = []
    for name in ("item", "tolist", "cpu", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name,
                            lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n) if self.is_cuda else None,
                                                                     _o(self, *a, **k))[1])
    flushes = []
    orig_flush = Compressor._flush
    monkeypatch.setattr(Compressor, "_flush", lambda self: (flushes.append(bool(self.__dict__.get("_pending"))),
                                                            orig_flush(self))[1])
    for c in clients:
        c.compressors, c.wire_records = comps, True
        c.communicate(s)
    assert not reads and not any(flushes)  # (nothing read back, no pending count folded)
    pend = comps[0].__dict__["_pending"]
    slab = comps[0].__dict__["_slab"]
    assert len(pend) == len(clients)
    assert all(cnt.data_ptr() == slab.data_ptr() + 8 * i for i, (cnt, _, _) in enumerate(pend))
    monkeypatch.undo()
    total = comps[0].really_need_to_send_components  # (the first read folds the slab)
    assert comps[0].__dict__.get("_pending") is None
    for c in clients:  # the same messages, the option off
        c.compressors, c.wire_records = want, False
        c.communicate(s)
    assert total == want[0].really_need_to_send_components
    assert comps[0].last_need_to_send_advance == want[0].last_need_to_send_advance
    a, b = s._received_messages[:len(clients)], s._received_messages[len(clients):]
    for x, y in zip(a, b):
        assert gc.same_bits(x["delta_parameters"].flat().cpu().numpy(), y["delta_parameters"].flat().cpu().numpy())


# ------------------------------------------------------------------------------------- 3. the message as an object
@pytest.mark.parametrize("codec", ["std4p2", "natural"])
def test_message_pickles_as_its_record(codec):
    from fl_sim_amd.compressed import compress_delta

    shapes = CONFIG1_SHAPES
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 1)
    D = _n(shapes)
    gc.seed_all(4)
    d = compress_delta([t.cuda() for t in locals_[0]], [t.cuda() for t in theta], make_compressors(codec, D), wire=True)
    dense = d.flat().cpu().numpy()  # (decoded before it is pickled: the copy still travels as the record)
    blob = pickle.dumps(d)
    assert len(blob) <= d.nbytes + 1024 and d.nbytes < 4 * D
    for x in (pickle.loads(blob), copy.deepcopy(d)):
        assert x.kind == d.kind and x._flat is None and x.nbytes == d.nbytes
        assert np.array_equal(x.record.cpu().numpy(), d.record.cpu().numpy())
        assert gc.same_bits(x.flat().cpu().numpy(), dense)
        assert [tuple(t.shape) for t in x] == [tuple(sh) for sh in shapes]


def test_option_off_is_unchanged():
    """Without the option (the default, and ``wire_records`` false) these codecs send their decoded vectors."""
    shapes = SMALL_SHAPES
    D = _n(shapes)
    s, clients = build_round(shapes, "avg", "cuda")
    gc.seed_all(1)
    for i, c in enumerate(clients[:3]):
        c.compressors = make_compressors("std8inf", D)
        if i == 1:
            c.wire_records = False
        if i == 2:
            c.config = types.SimpleNamespace(wire_records=0)
        c.communicate(s)
    assert all(m["delta_parameters"].kind == "dense" and m["delta_parameters"].nbytes == 4 * D
               for m in s._received_messages)
    from fl_sim_amd.compressed import dense_record_round, record_round

    assert dense_record_round(s._received_messages) is None and record_round(s._received_messages) is None


def test_codecs_without_a_record_ignore_the_option():
    """``wire`` on with a compressor list that has no dense record: the existing path, byte for byte."""
    from fl_sim_amd.compressed import compress_delta

    shapes = SMALL_SHAPES
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 1)
    D = _n(shapes)
    loc, glob = [t.cuda() for t in locals_[0]], [t.cuda() for t in theta]
    for codec, kind in (("topk", "dense"), ("stacked10", "stacked"), ("randk", "dense")):
        out = []
        for wire in (False, True):
            gc.seed_all(9)
            d = compress_delta(loc, glob, make_compressors(codec, D), wire=wire)
            assert d.kind == kind
            out.append(d.flat().cpu().numpy())
        assert gc.same_bits(out[0], out[1]), codec


def test_mixed_round_falls_back_to_per_message_decoding():
    """One stacked message among quantizer records (and records of two widths): no record round, every message decodes
    itself, and the update equals the update from the decoded messages."""
    from fl_sim_amd import aggregation as agg
    from fl_sim_amd.compressed import dense_record_round, record_round, stacked_round

    shapes = SMALL_SHAPES
    D = _n(shapes)
    s, clients = build_round(shapes, "adam", "cuda")
    gc.seed_all(2)
    for i, c in enumerate(clients):
        c.compressors = make_compressors("stacked10" if i == 0 else "std4p2" if i == 5 else "std8inf", D)
        c.wire_records = True
        c.communicate(s)
    msgs = s._received_messages
    assert [m["delta_parameters"].kind for m in msgs] == ["stacked"] + ["quant"] * 9
    assert stacked_round(msgs) is None and dense_record_round(msgs) is None and record_round(msgs) is None
    assert dense_record_round(msgs[1:5]) is not None and dense_record_round(msgs[1:]) is None  # (4 bits among 8)
    cfg = ROUND_OPTS["adam"]

    def state():
        theta, delta, v, _, _ = round_inputs(shapes, "adam")
        return [t.clone().cuda() for t in theta], [t.clone().cuda() for t in delta], [t.clone().cuda() for t in v]

    a, b = state(), state()
    agg.fedopt_update(a[0], a[1], a[2], msgs, "adam", cfg["lr"], cfg["betas"], cfg["tau"])
    decoded = [{"delta_parameters": [t.clone() for t in m["delta_parameters"]]} for m in msgs]
    agg.fedopt_update(b[0], b[1], b[2], decoded, "adam", cfg["lr"], cfg["betas"], cfg["tau"])
    for x, y in zip(a[0] + a[1] + a[2], b[0] + b[1] + b[2]):
        assert gc.same_bits(x.cpu().numpy().reshape(-1), y.cpu().numpy().reshape(-1))


def test_scaffold_sets_of_two_codecs_fold_separately():
    """``compressors`` 8-bit dithering and ``control_compressors`` natural: two record rounds of different codecs, each
    folded in a grouped pass of its own, equal to the update from the decoded messages."""
    from fl_sim_amd import aggregation as agg
    from tests.golden.gen_golden import SCAFFOLD_CFG

    shapes = SMALL_SHAPES
    D = _n(shapes)
    theta, cvs, clients = scaffold_codec_inputs(shapes)
    msgs = types.SimpleNamespace(_received_messages=[])
    gc.seed_all(32)
    for src in clients:
        c = tdc._scaffold_client(src, ("std8inf", "natural"), D)
        c.wire_records = True
        c.communicate(msgs)
    sent = msgs._received_messages
    assert sent[0]["parameters_delta"].kind == "quant" and sent[0]["control_variates_delta"].kind == "natural"
    pa, ca = [t.clone().cuda() for t in theta], [t.clone().cuda() for t in cvs]
    pb, cb = [t.clone().cuda() for t in theta], [t.clone().cuda() for t in cvs]
    agg.scaffold_update(pa, ca, sent, SCAFFOLD_CFG["lr"], SCAFFOLD_CFG["num_clients"])
    assert all(m[k]._flat is None for m in sent for k in tdc.KEYS)
    agg.scaffold_update(pb, cb, tdc._decoded(sent, tdc.KEYS), SCAFFOLD_CFG["lr"], SCAFFOLD_CFG["num_clients"])
    tdc._assert_same(pa + ca, pb + cb)
