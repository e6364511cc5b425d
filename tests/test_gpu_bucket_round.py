"""Bucket records at the codec's call site (compress_delta / compress_tensors with ``wire`` and ``bucket``) and in the
server folds (flc_fedopt_fold_bucket_records, flc_avg_and_gradient_bucket_records, flc_fold_bucket_record_groups,
flc_fold_bucket_wires), bit for bit against decoding every record (flc_bucket_decode) and running today's dense path;
FedAvg also against oracle/aggregation_ref on the numpy-decoded records; the deferred round encode against the
immediate one; mixed rounds, pickling and error feedback."""

import ctypes
import pickle

import numpy as np
import pytest
import torch

from oracle import aggregation_ref
from tests import bucket_ref as br
from tests.golden.gen_golden import CONFIG1_SHAPES, SMALL_SHAPES

pytestmark = pytest.mark.gpu

STD, NATD = 0, 1


def _n(shapes):
    return sum(int(np.prod(s)) for s in shapes)


def _model(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(s, generator=g) * scale).cuda() for s in shapes]


def _comp(kind, s, p=np.inf, seed=0, bucket=0, rng="philox"):
    from fl_sim_amd import Compressor

    c = Compressor("q", rng=rng, seed=seed, bucket=bucket, extended_levels=s > 10)
    if kind == STD:
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(s, nc, p=p)
    else:
        c.makeNaturalDitheringFP32(s, 512, p=p)
    return c


def _split(flat, shapes):
    out, off = [], 0
    for s in shapes:
        m = int(np.prod(s))
        out.append(flat[off:off + m].view(tuple(s)).clone())
        off += m
    return out


def _decoded(d, shapes):
    """The record decoded by flc_bucket_decode on a copy (the delta itself keeps no decoded vector)."""
    from fl_sim_amd import codec

    assert d.kind == "bucket"
    return _split(codec.bucket_decode(d.record.clone(), d.n, d.format, d.levels, d.bits, d.bucket), shapes)


def _numpy_decoded(d, shapes):
    from fl_sim_amd import codec

    nv, cv = codec.bucket_wire_views(d.record, d.n, d.format, d.bits, d.bucket)
    v = br.decode(br.unpack(cv.cpu().numpy(), d.n, d.bits), d.format, d.levels, d.bucket, nv.cpu().numpy())
    return _split(torch.from_numpy(v), shapes)


def _round(shapes, C, kind, s, B, p=np.inf, key_seed=100):
    """C bucket-record deltas of clients whose compressors have advanced differently (different counters)."""
    from fl_sim_amd.compressed import compress_delta

    cached = _model(shapes, 1)
    out = []
    for i in range(C):
        comp = _comp(kind, s, p, seed=key_seed + (i % 4))
        comp.philox.counter = 3 * i
        local = [c + d for c, d in zip(cached, _model(shapes, 10 + i, 1e-2))]
        out.append(compress_delta(local, cached, [comp], wire=True, bucket=B))
    assert all(d.kind == "bucket" and d.bucket == B for d in out)
    return out


def _fields(d):
    """The record's norms and codes (the padding behind them is never written)."""
    from fl_sim_amd import codec

    nv, cv = codec.bucket_wire_views(d.record, d.n, d.format, d.bits, d.bucket)
    return nv.view(torch.int32).clone(), cv.clone()


def _same_fields(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _same(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.fixture(autouse=True)
def _no_leftovers():
    from fl_sim_amd import compressed

    compressed._run_pending()
    yield
    compressed._run_pending()


# ------------------------------------------------------------------------------------------------ FedOpt
@pytest.mark.parametrize("shapes,C,opt,kind,s,B", [
    (SMALL_SHAPES, 4, "avg", STD, 127, 64), (SMALL_SHAPES, 70, "avg", NATD, 7, 512),
    (SMALL_SHAPES, 4, "adam", STD, 1, 256), (SMALL_SHAPES, 70, "adam", STD, 7, 4096),
    (CONFIG1_SHAPES, 4, "avg", STD, 127, 512)], ids=["avg4", "avg70", "adam4", "adam70", "config1"])
def test_fedopt_fold_equals_the_dense_path(shapes, C, opt, kind, s, B):
    from fl_sim_amd import aggregation

    deltas = _round(shapes, C, kind, s, B)
    step = (opt, 1.0, (0.0, 1.0), 0.0) if opt == "avg" else (opt, 0.1, (0.9, 0.99), 1e-3)
    res = []
    for form in ("records", "decoded"):
        theta, dl, v = _model(shapes, 2), _model(shapes, 3, 1e-2), [t.abs() for t in _model(shapes, 4, 1e-4)]
        msgs = [{"delta_parameters": d if form == "records" else _decoded(d, shapes), "train_samples": 10}
                for d in deltas]
        aggregation.fedopt_update(theta, dl, v, msgs, *step)
        res.append(theta + dl + v)
    assert all(d._flat is None for d in deltas)  # (the fold read the records: nothing was decoded)
    assert _same(res[0], res[1])
    if opt == "avg":
        theta, dl = [t.cpu() for t in _model(shapes, 2)], [t.cpu() for t in _model(shapes, 3, 1e-2)]
        msgs = [{"delta_parameters": _numpy_decoded(d, shapes), "train_samples": 10} for d in deltas]
        aggregation_ref.fedopt_update(theta, dl, None, msgs, "avg", 1.0, (0.0, 1.0), 0.0)
        n = len(shapes)
        assert _same([t.cpu() for t in res[0][:2 * n]], theta + dl)


# ------------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("C,kind,s,B", [(4, STD, 7, 64), (70, NATD, 127, 1024)])
def test_gradient_fold_equals_the_dense_path(C, kind, s, B):
    """A FedProx-shaped round: the parameters dense, the gradients bucket records."""
    from fl_sim_amd import aggregation
    from fl_sim_amd.compressed import compress_tensors

    shapes = SMALL_SHAPES
    grads = [compress_tensors(_model(shapes, 30 + i, 1e-2), [_comp(kind, s, seed=7 + i)], wire=True, bucket=B)
             for i in range(C)]
    assert all(g.kind == "bucket" for g in grads)
    res = []
    for form in ("records", "decoded"):
        mps = [torch.nn.Parameter(t) for t in _model(shapes, 2)]
        msgs = [{"parameters": _model(shapes, 50 + i), "gradients": g if form == "records" else _decoded(g, shapes),
                 "train_samples": 5 + i} for i, g in enumerate(grads)]
        got = aggregation.avg_parameters_and_gradients(mps, msgs, inertia=0.25)
        res.append([p.data for p in mps] + list(got))
    assert all(g._flat is None for g in grads)
    assert _same(res[0], res[1])


# ------------------------------------------------------------------------------------------------ groups
def test_scaffold_groups_equal_the_dense_path():
    from fl_sim_amd import aggregation

    shapes, C = SMALL_SHAPES, 6
    pd = _round(shapes, C, STD, 7, 128, key_seed=200)
    cd = _round(shapes, C, STD, 7, 128, key_seed=300)
    res = []
    for form in ("records", "decoded"):
        ps, cvs = _model(shapes, 2), _model(shapes, 5)
        msgs = [{"parameters_delta": a if form == "records" else _decoded(a, shapes),
                 "control_variates_delta": b if form == "records" else _decoded(b, shapes)} for a, b in zip(pd, cd)]
        aggregation.scaffold_update(ps, cvs, msgs, 0.5, 20)
        res.append(ps + cvs)
    assert all(d._flat is None for d in pd + cd)
    assert _same(res[0], res[1])


def test_ifca_groups_with_an_empty_cluster_equal_the_dense_path():
    from fl_sim_amd import aggregation

    shapes, C = SMALL_SHAPES, 7
    deltas = _round(shapes, C, NATD, 7, 2048, key_seed=400)
    cluster_of = [0, 2, 2, 0, 3, 2, 0]  # (cluster 1 stays idle)
    res = []
    for form in ("records", "decoded"):
        centers = {c: {"center_model_params": _model(shapes, 60 + c), "client_ids": []} for c in range(4)}
        msgs = [{"client_id": i, "cluster_id": cluster_of[i],
                 "delta_parameters": d if form == "records" else _decoded(d, shapes)} for i, d in enumerate(deltas)]
        aggregation.ifca_update(centers, msgs, 4)
        res.append([t for c in range(4) for t in centers[c]["center_model_params"]])
    assert all(d._flat is None for d in deltas)
    assert _same(res[0], res[1])
    assert _same(res[0][len(shapes):2 * len(shapes)], _model(shapes, 61))  # (the idle centre is untouched)


# ------------------------------------------------------------------------------------------------ the wire fold
@pytest.mark.parametrize("kind,s,B,n", [(STD, 127, 64, 4186), (NATD, 7, 512, 70001), (STD, 1, 4096, 12345)])
@pytest.mark.parametrize("accumulate", [False, True])
def test_fold_bucket_wires(kind, s, B, n, accumulate):
    from fl_sim_amd import _lib, codec

    bits = br.code_bits(s)
    stride, _ = codec.bucket_wire_layout(n, kind, bits, B)
    R = 6
    wires = torch.zeros(R, stride, dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(n)
    for r in range(R):
        x = (torch.randn(n, generator=g) * 1e-2).cuda()
        codec.bucket_encode(x, kind, s, B, np.inf, 11, r, record=wires[r])
    slots = [4, 0, 5, 2]  # (out of order; records 1 and 3 unused)
    weights = [0.5, -0.25, 0.0, 1.5]
    prev = (torch.randn(n, generator=g)).cuda()
    out = prev.clone()
    _lib.call("flc_fold_bucket_wires", wires.data_ptr(), stride, (ctypes.c_int32 * 4)(*slots),
              (ctypes.c_float * 4)(*weights), 4, n, kind, s, bits, B, int(accumulate), out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    want = prev.clone() if accumulate else torch.zeros(n, device="cuda")
    for sl, w in zip(slots, weights):
        codec.bucket_decode(wires[sl], n, kind, s, bits, B, out=want, weight=w, accumulate=True)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------------------------------------ deferred
def _stat_tuple(c):
    return (c.total_input_components, c.last_input_advance, c.really_need_to_send_components,
            c.last_need_to_send_advance, c.philox.counter)


@pytest.mark.parametrize("kind,s,p", [(STD, 7, np.inf), (NATD, 7, 2)])
def test_deferred_round_equals_the_immediate_encodes(kind, s, p, monkeypatch):
    from fl_sim_amd import compressed

    assert compressed.DEFER_ENCODE
    shapes, B, C = SMALL_SHAPES, 512, 5
    cached = _model(shapes, 1)
    locals_ = [[c + d for c, d in zip(cached, _model(shapes, 80 + i, 1e-2))] for i in range(C)]

    def run():
        comps = [_comp(kind, s, p, seed=500 + i) for i in range(C)]
        for i, c in enumerate(comps):
            c.philox.counter = 7 * i  # (sampled clients: the compressors have advanced differently)
        ds = [compressed.compress_delta(locals_[i], cached, [comps[i]], wire=True, bucket=B) for i in range(C)]
        return comps, ds

    compressed.deferred_bucket_stats(reset=True)
    comps, ds = run()
    assert all(d._batch is not None and d._record is None for d in ds)  # (waiting)
    recs = [_fields(d) for d in ds]
    assert compressed.deferred_bucket_stats() == {"batches": 1, "messages": C}
    stats = [_stat_tuple(c) for c in comps] + [_stat_tuple(c.vectorNormCompressor) for c in comps if kind == STD]
    monkeypatch.setattr(compressed, "DEFER_ENCODE", False)
    comps2, ds2 = run()
    assert all(d._batch is None and d._record is not None for d in ds2)
    assert compressed.deferred_bucket_stats() == {"batches": 1, "messages": C}
    assert all(_same_fields(a, _fields(d)) for a, d in zip(recs, ds2))
    assert stats == ([_stat_tuple(c) for c in comps2]
                     + [_stat_tuple(c.vectorNormCompressor) for c in comps2 if kind == STD])
    nb = -(-_n(shapes) // B)
    if kind == STD:
        assert all(c.vectorNormCompressor.total_input_components == nb for c in comps)


# ------------------------------------------------------------------------------------------------ fall-backs
@pytest.mark.parametrize("mixed_fold", [False, True])
def test_a_round_mixing_bucket_and_dense_records(mixed_fold, monkeypatch):
    from fl_sim_amd import aggregation, compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", mixed_fold)
    compressed.mixed_fold_stats(reset=True)
    shapes = SMALL_SHAPES
    cached = _model(shapes, 1)
    ds = []
    for i, B in enumerate([512, 0, 512, 0]):
        local = [c + d for c, d in zip(cached, _model(shapes, 90 + i, 1e-2))]
        ds.append(compressed.compress_delta(local, cached, [_comp(STD, 7, seed=600 + i)], wire=True, bucket=B))
    assert [d.kind for d in ds] == ["bucket", "quant", "bucket", "quant"]
    assert len({(d.n, d.format, d.levels, d.bits) for d in ds}) == 1 and compressed.record_round(
        [{"delta_parameters": d} for d in ds]) is None
    decoded = [_decoded(d, shapes) if d.kind == "bucket" else
               _split(pickle.loads(pickle.dumps(d)).flat(), shapes) for d in ds]
    res = []
    for form in ("records", "decoded"):
        theta, dl = _model(shapes, 2), _model(shapes, 3, 1e-2)
        msgs = [{"delta_parameters": d if form == "records" else t, "train_samples": 10} for d, t in zip(ds, decoded)]
        aggregation.fedopt_update(theta, dl, None, msgs, "avg", 1.0, (0.0, 1.0), 0.0)
        res.append(theta + dl)
    assert _same(res[0], res[1])
    assert compressed.mixed_fold_stats()["folds"] == (1 if mixed_fold else 0)


def test_a_pickled_batch_round_trips():
    from fl_sim_amd import compressed

    shapes = SMALL_SHAPES
    ds = _round(shapes, 4, STD, 7, 256, key_seed=700)
    assert all(d._batch is not None for d in ds)
    twins = [pickle.loads(pickle.dumps(d)) for d in ds]
    assert compressed.deferred_bucket_stats()["batches"] >= 1
    for d, t in zip(ds, twins):
        assert t.kind == "bucket" and t.bucket == 256 and t.codec_key == d.codec_key and t._flat is None
        assert t.nbytes == d.nbytes == d.record.numel() < 4 * d.n
        assert _same_fields(_fields(t), _fields(d))
        assert _same(list(t), _decoded(d, shapes))
        assert _same(list(d), list(t))


def test_wire_off_sends_the_bucketed_decoded_vector():
    from fl_sim_amd import compressed

    shapes = SMALL_SHAPES
    cached = _model(shapes, 1)
    local = [c + d for c, d in zip(cached, _model(shapes, 95, 1e-2))]
    a = compressed.compress_delta(local, cached, [_comp(STD, 7, seed=800)], wire=True, bucket=128)
    b = compressed.compress_delta(local, cached, [_comp(STD, 7, seed=800)], bucket=128)
    c = compressed.compress_delta(local, cached, [_comp(STD, 7, seed=800, bucket=128)], wire=True)
    assert a.kind == "bucket" and b.kind == "dense" and c.kind == "bucket"
    assert _same_fields(_fields(a), _fields(c))
    assert _same([b.flat()], [a.flat()])

    class Node:
        pass

    node = Node()
    assert compressed._quant_bucket(node) == 0
    node.config = type("Cfg", (), {"quant_bucket": 512})()
    assert compressed._quant_bucket(node) == 512
    node.quant_bucket = 64
    assert compressed._quant_bucket(node) == 64


# ------------------------------------------------------------------------------------------------ error feedback
@pytest.mark.parametrize("kind,s,B", [(STD, 7, 64), (NATD, 7, 512)])
def test_error_feedback_against_the_oracle(kind, s, B):
    """2 rounds x 3 clients: a = e + delta; c = bucket(a); e' = a - c, with the oracle's dithering rule per bucket."""
    from fl_sim_amd.compressed import compress_delta
    from fl_sim_amd.feedback import ErrorMemory

    shapes = SMALL_SHAPES
    n = _n(shapes)
    cached = _model(shapes, 1)
    comps = [_comp(kind, s, seed=900 + i) for i in range(3)]
    mems = [ErrorMemory(n, "cuda") for _ in range(3)]
    e = [np.zeros(n, dtype=np.float32) for _ in range(3)]
    for r in range(2):
        for i in range(3):
            local = [c + d for c, d in zip(cached, _model(shapes, 1000 + 10 * r + i, 1e-2))]
            delta = torch.cat([(lo - c).reshape(-1) for lo, c in zip(local, cached)]).cpu().numpy()
            d = compress_delta(local, cached, [comps[i]], feedback=mems[i], wire=True, bucket=B)
            assert d.kind == "bucket" and d._batch is None  # (not deferred)
            a = e[i] + delta
            pn = np.array([np.max(np.abs(a[lo:hi])) for lo, hi in br.slices(n, B)], dtype=np.float32)
            c, _, _ = br.bucket_philox(a, kind, s, B, pn, 900 + i, r)
            e[i] = a - c
            assert np.array_equal(d.flat().cpu().numpy().view(np.uint32), c.view(np.uint32)), (r, i)
            assert np.array_equal(mems[i].value().cpu().numpy().view(np.uint32), e[i].view(np.uint32)), (r, i)
