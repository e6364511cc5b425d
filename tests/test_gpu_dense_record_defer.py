"""Deferred dense records: with ``wire`` on in philox mode a dithering quantizer's messages wait for one batched
flc_quant_encode_round.  A round with deferral on and the same round with ``DEFER_ENCODE`` off (the per-message
flc_quant_encode_auto) agree bit for bit — records, send statistics, Philox counters, the server's update — through
compress_delta, compress_tensors and the FedOpt, SCAFFOLD and IFCA client mixins; the batch runs when a record or a
statistic is first read; everything else stays on the immediate path."""

import pickle
import types

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import test_gpu_delta_codec as tdc
from tests.golden.gen_golden import CONFIG1_SHAPES, SMALL_SHAPES, round_inputs
from tests.golden.gen_golden_delta_codec import ifca_codec_inputs, scaffold_codec_inputs
from tests.test_gpu_round import build_round, make_compressors

pytestmark = pytest.mark.gpu
CODECS = ["std8inf", "std4p2", "natd7"]
SHAPES = {"small": SMALL_SHAPES, "config1": CONFIG1_SHAPES}


def _n(shapes):
    return sum(int(np.prod(sh)) for sh in shapes)


def _comps(codec, D, seed, rng="philox"):
    from fl_sim_amd import Compressor

    if codec == "natd7":
        c = Compressor(rng=rng, seed=seed)
        c.makeNaturalDitheringFP32(7, D)
        return [c]
    return make_compressors(codec, D, rng=rng, seed=seed)


def _stat(c):
    return (c.total_input_components, c.last_input_advance, c.really_need_to_send_components,
            c.last_need_to_send_advance, c.philox.counter)


def _rec(d):
    """(norm bits, code bytes) of a dense record (its padding is not part of the message)."""
    from fl_sim_amd import codec

    norm, codes = codec.dense_wire_views(d.record, d.n, d.format, d.bits)
    if d.kind == "natural":  # (the natural compressor's record has no norm: the field is never written)
        return np.zeros(1, np.int32), codes.cpu().numpy()
    return norm.view(torch.int32).cpu().numpy(), codes.cpu().numpy()


def _same_records(a, b):
    assert (a.kind, a.codec_key, a.nbytes, [tuple(s) for s in a.shapes]) == \
           (b.kind, b.codec_key, b.nbytes, [tuple(s) for s in b.shapes])
    (na, ca), (nb, cb) = _rec(a), _rec(b)
    return np.array_equal(na, nb) and np.array_equal(ca, cb)


def _flat(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts]).numpy()


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    from fl_sim_amd import compressed

    compressed._run_pending()  # (messages earlier tests left waiting)
    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    yield
    compressed._run_pending()


def _legs(run):
    """``run()`` with deferral off, then on; (immediate result, deferred result)."""
    from fl_sim_amd import compressed

    out = []
    for on in (False, True):
        compressed.DEFER_ENCODE = on
        out.append(run(on))
    compressed.DEFER_ENCODE = True
    return out


# ------------------------------------------------------------------------------ 1. deferred == immediate, bit for bit
@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("codec", CODECS)
def test_compress_delta_and_tensors(codec, tag):
    from fl_sim_amd.compressed import compress_delta, compress_tensors

    shapes = SHAPES[tag]
    D = _n(shapes)
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 4)
    glob = [t.cuda() for t in theta]
    locs = [[t.cuda() for t in loc] for loc in locals_]

    def run(on):
        comps = [_comps(codec, D, 40 + i) for i in range(2)]  # (two clients' compressors, advancing differently)
        ds = [compress_delta(locs[i], glob, comps[i % 2], wire=True) for i in range(4)]
        ds += [compress_tensors(locs[i], comps[0], wire=True) for i in range(2)]
        assert all((d._batch is not None) == on for d in ds)
        return ds, [_stat(c[0]) for c in comps]

    (a, sa), (b, sb) = _legs(run)
    assert sa == sb
    for x, y in zip(a, b):
        assert _same_records(x, y)
        assert y._batch is None and y._flat is None
    assert gc.same_bits(a[0].flat().cpu().numpy(), b[0].flat().cpu().numpy())


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("codec", CODECS)
def test_fedopt_round(codec, tag):
    shapes = SHAPES[tag]
    D = _n(shapes)

    def run(on):
        s, clients = build_round(shapes, "adam", "cuda")
        comps = [_comps(codec, D, 7 + i) for i in range(3)]  # (sampled clients share three compressor sets)
        for i, c in enumerate(clients):
            c.compressors, c.wire_records = comps[i % 3], True
            c.communicate(s)
        msgs = list(s._received_messages)
        assert all((m["delta_parameters"]._batch is not None) == on for m in msgs)
        s.update()
        assert all(m["delta_parameters"]._flat is None for m in msgs)  # (the record fold took the round)
        return msgs, [_stat(c[0]) for c in comps], _flat(list(s.model.parameters()) + s.delta_parameters)

    (ma, sa, ta), (mb, sb, tb) = _legs(run)
    assert sa == sb and gc.same_bits(ta, tb)
    assert all(_same_records(x["delta_parameters"], y["delta_parameters"]) for x, y in zip(ma, mb))


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("codec", CODECS)
def test_scaffold_round(codec, tag):
    """Both deltas of a client (its two compressor sets) join the round's batch, each with its own counter."""
    shapes = SHAPES[tag]
    D = _n(shapes)
    theta, cvs, clients = scaffold_codec_inputs(shapes)

    def run(on):
        s = tdc._scaffold_server(theta, cvs, "device")
        stats = []
        for i, src in enumerate(clients):
            c = tdc._scaffold_client(src)
            c.compressors, c.config.control_compressors = _comps(codec, D, 100 + i), _comps(codec, D, 200 + i)
            c.wire_records = True
            c.communicate(s)
            stats.append((c.compressors[0], c.config.control_compressors[0]))
        msgs = list(s._received_messages)
        assert all((m[k]._batch is not None) == on for m in msgs for k in tdc.KEYS)
        if on:
            assert len({id(m[k]._batch) for m in msgs for k in tdc.KEYS}) == 1  # (one batch for both vectors)
        s.update()
        assert all(m[k]._flat is None for m in msgs for k in tdc.KEYS)
        return msgs, [(_stat(a), _stat(b)) for a, b in stats], _flat(list(s.model.parameters()) + s._control_variates)

    (ma, sa, ta), (mb, sb, tb) = _legs(run)
    assert sa == sb and gc.same_bits(ta, tb)
    assert all(_same_records(x[k], y[k]) for x, y in zip(ma, mb) for k in tdc.KEYS)


@pytest.mark.parametrize("tag", list(SHAPES))
@pytest.mark.parametrize("codec", CODECS)
def test_ifca_round(codec, tag):
    shapes = SHAPES[tag]
    D = _n(shapes)
    centers, clients = ifca_codec_inputs(shapes)

    def run(on):
        s = tdc._ifca_server(centers, "device")
        comps = []
        for i, src in enumerate(clients):
            c = tdc._ifca_client(src)
            c.compressors, c.wire_records = _comps(codec, D, 300 + i), True
            c.communicate(s)
            comps.append(c.compressors[0])
        msgs = list(s._received_messages)
        assert all((m["delta_parameters"]._batch is not None) == on for m in msgs)
        s.update()
        assert all(m["delta_parameters"]._flat is None for m in msgs)
        return msgs, [_stat(c) for c in comps], _flat([p for c in range(4)
                                                        for p in s._cluster_centers[c]["center_model_params"]])

    (ma, sa, ta), (mb, sb, tb) = _legs(run)
    assert sa == sb and gc.same_bits(ta, tb)
    assert all(_same_records(x["delta_parameters"], y["delta_parameters"]) for x, y in zip(ma, mb))


# ------------------------------------------------------------------------------------------- 2. the batch's behaviour
def _round_of_ten(codec="std8inf", shapes=SMALL_SHAPES, seed=5):
    D = _n(shapes)
    s, clients = build_round(shapes, "avg", "cuda")
    comps = _comps(codec, D, seed)
    for c in clients:
        c.compressors, c.wire_records = comps, True
    return s, clients, comps


def test_ten_messages_wait_for_one_batch_and_nothing_is_read_back(monkeypatch):
    from fl_sim_amd import compressed

    s, clients, comps = _round_of_ten()
    assert len(clients) == 10
    before, dense_before = compressed.deferred_stats(), compressed.deferred_dense_stats(reset=True)
    assert sorted(dense_before) == ["batches", "messages"]
    reads = []
    for name in ("item", "tolist", "cpu", "numpy"):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name,
                            lambda self, *a, _o=orig, _n=name, **k: (reads.append(_n) if self.is_cuda else None,
                                                                     _o(self, *a, **k))[1])
    for c in clients:
        c.communicate(s)
    ds = [m["delta_parameters"] for m in s._received_messages]
    assert all(d._batch is not None and d._batch is ds[0]._batch and d._record is None for d in ds)
    assert not reads  # (nothing read back from the device)
    assert compressed.deferred_dense_stats() == {"batches": 0, "messages": 0}
    rec = ds[3].record  # the first access resolves all ten
    assert rec is not None and not reads
    monkeypatch.undo()
    assert all(d._batch is None and d._record is not None for d in ds) and not compressed._PENDING
    assert compressed.deferred_dense_stats() == {"batches": 1, "messages": 10}
    assert compressed.deferred_stats() == before  # (the stacked batches' counters are their own)
    base = ds[0]._record.data_ptr()
    assert all(d._record.data_ptr() == base + i * ds[0]._record.numel() for i, d in enumerate(ds))  # one block
    assert compressed.deferred_dense_stats(reset=True) == {"batches": 1, "messages": 10}
    assert compressed.deferred_dense_stats() == {"batches": 0, "messages": 0}


def test_two_sizes_or_two_level_counts_make_two_batches():
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_tensors

    g = torch.Generator(device="cuda").manual_seed(3)
    eight, four = _comps("std8inf", 5000, 1), _comps("std4p2", 5000, 1)
    two_sizes = [(m, eight) for m in (5000, 5000, 4999, 5000)]
    two_levels = [(5000, eight), (5000, four), (5000, eight), (5000, four)]
    for round_ in (two_sizes, two_levels):
        compressed.deferred_dense_stats(reset=True)
        ds = [compress_tensors([torch.randn(m, generator=g, device="cuda")], comps, wire=True) for m, comps in round_]
        assert len({id(d._batch) for d in ds}) == 2 and len(compressed._PENDING) == 2
        compressed._run_pending()
        assert all(d._batch is None and d._record is not None for d in ds)
        assert compressed.deferred_dense_stats() == {"batches": 2, "messages": 4}


def test_reading_a_statistic_runs_the_batch():
    from fl_sim_amd import compressed

    s, clients, comps = _round_of_ten()
    for c in clients[:4]:
        c.communicate(s)
    ds = [m["delta_parameters"] for m in s._received_messages]
    assert all(d._batch is not None for d in ds) and compressed._PENDING
    total = comps[0].really_need_to_send_components
    assert all(d._batch is None and d._record is not None for d in ds) and not compressed._PENDING
    compressed.DEFER_ENCODE = False
    s2, clients2, comps2 = _round_of_ten()
    for c in clients2[:4]:
        c.communicate(s2)
    assert total == comps2[0].really_need_to_send_components and _stat(comps[0]) == _stat(comps2[0])


def test_pickling_a_pending_message_runs_the_batch():
    s, clients, _ = _round_of_ten("std4p2")
    for c in clients[:3]:
        c.communicate(s)
    ds = [m["delta_parameters"] for m in s._received_messages]
    assert all(d._batch is not None for d in ds)
    x = pickle.loads(pickle.dumps(ds[1]))
    assert all(d._batch is None for d in ds)
    assert x._batch is None and _same_records(x, ds[1])
    assert gc.same_bits(x.flat().cpu().numpy(), ds[1].flat().cpu().numpy())


def test_the_record_is_of_the_model_at_communicate():
    """The flat delta is snapshotted at ``communicate``: a model changed afterwards does not change the record."""
    def run(on):
        s, clients, _ = _round_of_ten("natd7")
        out = []
        for c in clients[:3]:
            c.communicate(s)
            if on:
                with torch.no_grad():
                    for p in c.model.parameters():
                        p.mul_(-3.0).add_(1.0)
                    for t in c._cached_parameters:
                        t.zero_()
        return [m["delta_parameters"] for m in s._received_messages]

    a, b = _legs(run)
    assert all(_same_records(x, y) for x, y in zip(a, b))


def test_messages_flattened_on_a_second_stream():
    from fl_sim_amd.compressed import compress_delta

    shapes = CONFIG1_SHAPES
    D = _n(shapes)
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 3)
    glob = [t.cuda() for t in theta]
    locs = [[t.cuda() for t in loc] for loc in locals_]
    torch.cuda.synchronize()

    def run(on):
        comps = _comps("std4p2", D, 9)
        side = torch.cuda.Stream()
        ds = [compress_delta(locs[0], glob, comps, wire=True)]
        with torch.cuda.stream(side):
            busy = torch.ones(2048, 2048, device="cuda")
            for _ in range(20):  # (work queued ahead of the flatten on the side stream)
                busy = busy @ busy * 1e-4
            ds += [compress_delta(locs[i], glob, comps, wire=True) for i in (1, 2)]
        if not on:  # (the immediate encodes ran on the side stream; the batch orders itself after the flattens)
            torch.cuda.current_stream().wait_stream(side)
        recs = [_rec(d) for d in ds]  # (read on the default stream)
        torch.cuda.synchronize()
        return ds, recs, _stat(comps[0])

    (a, ra, sa), (b, rb, sb) = _legs(run)
    assert sa == sb
    for (na, ca), (nb, cb) in zip(ra, rb):
        assert np.array_equal(na, nb) and np.array_equal(ca, cb)


# ------------------------------------------------------------------------------------------- 3. the immediate path
def _one_message(comps, feedback=None):
    from fl_sim_amd.compressed import compress_delta

    theta, _, _, locals_, _ = round_inputs(SMALL_SHAPES, "avg", 1)
    return compress_delta([t.cuda() for t in locals_[0]], [t.cuda() for t in theta], comps, feedback, wire=True)


@pytest.mark.parametrize("case", ["error_feedback", "compat", "natural", "reference_norm"])
def test_these_messages_are_not_deferred(case):
    from fl_sim_amd import compressed
    from fl_sim_amd.feedback import ErrorMemory

    D = _n(SMALL_SHAPES)

    def run(on):
        gc.seed_all(6)
        if case == "natural":
            comps = make_compressors("natural", D, rng="philox", seed=2)
        elif case == "compat":
            comps = _comps("std8inf", D, 2, rng="compat")
        else:
            comps = _comps("std4p2", D, 2)
        if case == "reference_norm":
            comps[0].norm_mode = "reference"
        mem = ErrorMemory(D, "cuda") if case == "error_feedback" else None
        d = _one_message(comps, mem)
        assert d._batch is None and d._record is not None and not compressed._PENDING
        return d, _stat(comps[0]), None if mem is None else mem.value().cpu().numpy()

    before = compressed.deferred_dense_stats()
    (a, sa, ea), (b, sb, eb) = _legs(run)
    assert _same_records(a, b) and sa == sb
    assert ea is None or gc.same_bits(ea, eb)
    assert compressed.deferred_dense_stats() == before  # (no batched encode ran)


def test_a_message_past_the_size_bound_is_not_deferred(monkeypatch):
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_tensors

    assert compressed._DEFER_DENSE_MAX_N <= compressed._DEFER_MAX_N
    monkeypatch.setattr(compressed, "_DEFER_DENSE_MAX_N", 5000)
    g = torch.Generator(device="cuda").manual_seed(8)
    comps = _comps("std8inf", 5001, 3)
    at, past = (compress_tensors([torch.randn(m, generator=g, device="cuda")], comps, wire=True) for m in (5000, 5001))
    assert at._batch is not None and past._batch is None and past._record is not None


def test_the_switch_off_encodes_every_message_at_once():
    """``FLC_DEFER_ENCODE=0`` (``compressed.DEFER_ENCODE`` false): every message encoded when it is made."""
    from fl_sim_amd import compressed

    before = compressed.deferred_dense_stats()
    compressed.DEFER_ENCODE = False
    s, clients, comps = _round_of_ten()
    for c in clients:
        c.communicate(s)
    ds = [m["delta_parameters"] for m in s._received_messages]
    assert all(d._batch is None and d._record is not None for d in ds) and not compressed._PENDING
    assert compressed.deferred_dense_stats() == before
