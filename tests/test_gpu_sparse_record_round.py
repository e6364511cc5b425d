"""The codec's call site with ``sparse_records`` on: the top-k and rand-k compressors send their sparse records
(flc_sparse_wire_layout) and the servers fold the records (flc_fedopt_fold_sparse_records,
flc_fold_sparse_record_groups, flc_avg_and_gradient_sparse_records) — against the reference's own rounds
(tests/golden/round_codec.npz, delta_codec.npz, vr_codec.npz, ef_codec.npz: the fixtures that pin the same rounds with
the option off), bit for bit, on a device- and a host-resident server, with every compressor's send statistics and both
global streams in lock-step; philox mode against the same messages with the option off and against the immediate
encodes; the deferred batch; pickling; fallbacks."""

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


def _n(shapes):
    return sum(int(np.prod(sh)) for sh in shapes)


def _is_record(d, D, K=None):
    """The message carries the sparse record of (D, K) and nothing else."""
    from fl_sim_amd import _lib
    from fl_sim_amd.compressed import CompressedDelta

    K = D // 100 if K is None else K
    size = _lib.size("flc_sparse_wire_layout", D, K, None)
    assert 0 < size < 4 * D
    return (isinstance(d, CompressedDelta) and d.kind == "sparse" and d.k == K and d.levels == 0 and d.format is None
            and d.nbytes == size and d.record.numel() == size and d._flat is None)


def _switch_on(c, i):
    if i % 2:  # (the two places the option is looked up)
        c.sparse_records = True
    else:
        cfg = getattr(c, "config", None)
        if cfg is None:
            c.config = types.SimpleNamespace(sparse_records=True)
        else:
            cfg.sparse_records = True


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
@pytest.mark.parametrize("codec", ["topk", "randk"])
def test_fedopt_round_with_records_matches_reference(codec, opt, tag, server):
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    rec = _fields(f"round_{codec}_{opt}_{tag}")
    s, clients = build_round(shapes, opt, "cuda" if server == "device" else "cpu")
    D = _n(shapes)
    stats = []
    gc.seed_all(round_seed(codec, opt, tag))
    for i, c in enumerate(clients):
        c.compressors = make_compressors(codec, D)
        _switch_on(c, i)
        c.communicate(s)
        stats.append([float(x.last_need_to_send_advance) for x in c.compressors]
                     + [float(x.total_input_components) for x in c.compressors])
    assert random.random() == float(rec["next_random"])
    assert np.random.random_sample() == float(rec["next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), rec["stats"])
    msgs = s._received_messages
    assert all(_is_record(m["delta_parameters"], D) for m in msgs)
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
def test_scaffold_round_with_records_matches_reference(tag, where):
    codec = "topk"
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    D = _n(shapes)
    theta, cvs, clients = scaffold_codec_inputs(shapes)
    key = delta_codec_key("scaffold", codec, tag)
    s = tdc._scaffold_server(theta, cvs, where)
    stats = []
    gc.seed_all(delta_codec_seed("scaffold", codec, tag))
    for i, src in enumerate(clients):
        c = tdc._scaffold_client(src, (codec, codec), D)
        _switch_on(c, i)
        c.communicate(s)
        stats.append(tdc._stats(c.compressors) + tdc._stats(c.config.control_compressors))
    assert random.random() == float(tdc.DC[key + "|next_random"])
    assert np.random.random_sample() == float(tdc.DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tdc.DC[key + "|stats"])
    got = s._received_messages
    assert len(got) == 10 and all(_is_record(m[k], D) for m in got for k in tdc.KEYS)
    s.update()
    assert all(m[k]._flat is None for m in got for k in tdc.KEYS)  # (the grouped fold read the records)
    assert tdc._same(key, "theta", list(s.model.parameters()))
    assert tdc._same(key, "cv", s._control_variates)
    dev = "cuda" if where == "device" else "cpu"
    assert all(p.device.type == dev for p in list(s.model.parameters()) + list(s._control_variates))


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tag", ["small", "config1"])
def test_ifca_round_with_records_matches_reference(tag, where):
    codec = "topk"
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    D = _n(shapes)
    centers, clients = ifca_codec_inputs(shapes)
    key = delta_codec_key("ifca", codec, tag)
    s = tdc._ifca_server(centers, where)
    stats = []
    gc.seed_all(delta_codec_seed("ifca", codec, tag))
    for i, src in enumerate(clients):
        c = tdc._ifca_client(src, codec, D)
        _switch_on(c, i)
        c.communicate(s)
        stats.append(tdc._stats(c.compressors))
    assert random.random() == float(tdc.DC[key + "|next_random"])
    assert np.random.random_sample() == float(tdc.DC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tdc.DC[key + "|stats"])
    got = s._received_messages
    assert all(_is_record(m["delta_parameters"], D) for m in got)
    s.update()
    assert all(m["delta_parameters"]._flat is None for m in got)
    dev = "cuda" if where == "device" else "cpu"
    for c in range(4):
        assert tdc._same(key, f"center{c}", s._cluster_centers[c]["center_model_params"]), c
        assert s._cluster_centers[c]["client_ids"] == tdc.DC[f"{key}|ids{c}"].tolist(), c
        assert all(p.device.type == dev for p in s._cluster_centers[c]["center_model_params"])
    tdc._assert_same(s._cluster_centers[1]["center_model_params"], centers[1]["center_model_params"])  # (idle)


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tag,nm", [("small", 10), ("config1", 10), ("small", 20)])
@pytest.mark.parametrize("name", list(VR_SERVERS))
def test_vr_round_with_gradient_records_matches_reference(name, tag, nm, where):
    codec = "topk"
    shapes = SMALL_SHAPES if tag == "small" else CONFIG1_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, nm)
    key = vr_codec_key(name, codec, nm, tag)
    s = tvr._server(name, params, where)
    stats = []
    gc.seed_all(vr_codec_seed(name, codec, nm, tag))
    for i, src in enumerate(msgs):
        c = tvr._client(src)
        c.gradient_compressors = make_compressors(codec, D)
        _switch_on(c, i)
        c.communicate(s)
        stats.append([float(x.last_need_to_send_advance) for x in c.gradient_compressors]
                     + [float(x.total_input_components) for x in c.gradient_compressors])
    assert random.random() == float(tvr.VRC[key + "|next_random"])
    assert np.random.random_sample() == float(tvr.VRC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tvr.VRC[key + "|stats"])
    got = s._received_messages
    assert len(got) == nm and all(_is_record(m["gradients"], D) for m in got)
    assert all(isinstance(m["parameters"], list) for m in got)  # (the parameters as the reference sends them)
    s.update()
    assert all(m["gradients"]._flat is None for m in got)  # (never decoded densely)
    assert tvr._same(key, "theta", list(s.model.parameters()))
    assert tvr._same(key, "grad", [p.grad for p in s.model.parameters()])
    dev = "cuda" if where == "device" else "cpu"
    assert all(p.device.type == dev and p.grad.device.type == dev for p in s.model.parameters())


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("tag", list(EF_TAGS))
def test_error_feedback_with_records_matches_the_reference(tag, defer, monkeypatch):
    """Error feedback with ``sparse`` on: the messages and memories of the option off (tests/golden/ef_codec.npz pins
    those), the message carrying the record, the memory taking the K-entry residual — after the round's batched encode
    (``defer``) or with one client."""
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_delta
    from fl_sim_amd.feedback import ErrorMemory
    from tests.test_gpu_ef_round import EF, _cuda
    from tests.test_gpu_ef_round import _same as ef_same

    monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
    codec = "topk"
    shapes = EF_TAGS[tag]
    cached, locals_ = ef_inputs(shapes)
    n, key = _n(shapes), ef_key(codec, tag)
    dc = _cuda(cached)
    comps = [make_compressors(codec, n) for _ in range(EF_CLIENTS)]
    mems = [ErrorMemory(n, "cuda") for _ in range(EF_CLIENTS)]
    compressed.deferred_sparse_stats(reset=True)
    gc.seed_all(ef_seed(codec, tag))
    for r in range(EF_ROUNDS):
        ds = [compress_delta(_cuda(locals_[r][i]), dc, comps[i], feedback=mems[i], sparse=True)
              for i in range(EF_CLIENTS)]
        for i, d in enumerate(ds):
            assert _is_record(d, n)
            assert ef_same(f"{key}|c{r}_{i}", d.flat().cpu().numpy()), (r, i)
    assert compressed.deferred_sparse_stats() == ({"batches": EF_ROUNDS, "messages": EF_ROUNDS * EF_CLIENTS} if defer
                                                  else {"batches": 0, "messages": 0})
    for i in range(EF_CLIENTS):
        assert ef_same(f"{key}|e{i}", mems[i].value().cpu().numpy()), i
    stats = [[float(x.really_need_to_send_components) for x in cs] + [float(x.total_input_components) for x in cs]
             + [float(x.last_need_to_send_advance) for x in cs] for cs in comps]
    assert np.array_equal(np.array(stats, dtype=np.float64), EF[key + "|stats"])
    assert random.random() == float(EF[key + "|next_random"])
    assert np.random.random_sample() == float(EF[key + "|next_np"])


# ------------------------------------------------------------------------------------------------ 2. philox mode
def _stat_tuple(c):
    return (c.total_input_components, c.last_input_advance, c.really_need_to_send_components,
            c.last_need_to_send_advance, c.philox.counter)


def _philox_round(codec, opt, shapes, sparse, n_clients=10, shared=False):
    """A philox-mode FedOpt round: (server, clients, the compressors)."""
    s, clients = build_round(shapes, opt, "cuda", n_clients)
    D = _n(shapes)
    comps = []
    one = make_compressors(codec, D, rng="philox", seed=31)
    for i, c in enumerate(clients):
        c.compressors = one if shared else make_compressors(codec, D, rng="philox", seed=31 + i)
        c.sparse_records = sparse
        comps.append(c.compressors[0])
        c.communicate(s)
    return s, clients, comps


@pytest.mark.parametrize("opt", list(ROUND_OPTS))
@pytest.mark.parametrize("codec", ["topk", "randk"])
def test_philox_records_on_equal_records_off(codec, opt):
    """The same round with the option on and off: identical θ, δ (and v), statistics and Philox counters; the records
    decode to the dense messages; a rand-k record's values are the scattered ones."""
    shapes = CONFIG1_SHAPES
    D = _n(shapes)
    a, _, ca = _philox_round(codec, opt, shapes, False)
    b, _, cb = _philox_round(codec, opt, shapes, True)
    assert all(m["delta_parameters"].kind == "dense" for m in a._received_messages)
    assert all(_is_record(m["delta_parameters"], D) for m in b._received_messages)
    assert [_stat_tuple(c) for c in ca] == [_stat_tuple(c) for c in cb]
    want = [m["delta_parameters"].flat().cpu().numpy() for m in a._received_messages]
    a.update()
    b.update()
    assert all(m["delta_parameters"]._flat is None for m in b._received_messages)
    for x, y in zip(list(a.model.parameters()) + a.delta_parameters + (a.v_parameters or []),
                    list(b.model.parameters()) + b.delta_parameters + (b.v_parameters or [])):
        assert gc.same_bits(x.detach().cpu().numpy().reshape(-1), y.detach().cpu().numpy().reshape(-1))
    for m, w in zip(b._received_messages, want):
        d = m["delta_parameters"]
        assert gc.same_bits(d.flat().cpu().numpy(), w)
        assert [tuple(t.shape) for t in d] == [tuple(sh) for sh in shapes]  # list(delta): the model's tensors
        idx = d.record[:4 * d.k].view(torch.int32).cpu().numpy()
        assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < D  # ascending, unique, in range


@pytest.mark.parametrize("n_msgs", [10, 70])
def test_deferred_round_encode_equals_the_immediate_encodes(n_msgs, monkeypatch):
    """One flc_topk_encode_batch for the round (70 messages: the pending bound runs a full batch of 64, the rest
    follow) against DEFER_ENCODE off: identical records, identical statistics."""
    from fl_sim_amd import compressed

    shapes = SMALL_SHAPES if n_msgs > 10 else CONFIG1_SHAPES
    D = _n(shapes)
    compressed.deferred_sparse_stats(reset=True)
    a, _, ca = _philox_round("topk", "avg", shapes, True, n_msgs)
    assert compressed.deferred_sparse_stats()["batches"] == (1 if n_msgs > 10 else 0)  # (nothing read yet)
    recs_a = [m["delta_parameters"].record.cpu().numpy() for m in a._received_messages]
    st = compressed.deferred_sparse_stats(reset=True)
    assert st == {"batches": 1 if n_msgs <= 64 else 2, "messages": n_msgs}
    assert compressed.deferred_stats()["batches"] >= 0 and compressed.deferred_dense_stats()["batches"] >= 0
    monkeypatch.setattr(compressed, "DEFER_ENCODE", False)
    b, _, cb = _philox_round("topk", "avg", shapes, True, n_msgs)
    assert compressed.deferred_sparse_stats() == {"batches": 0, "messages": 0}
    assert all(m["delta_parameters"]._batch is None for m in b._received_messages)
    recs_b = [m["delta_parameters"].record.cpu().numpy() for m in b._received_messages]
    assert all(_is_record(m["delta_parameters"], D) for m in a._received_messages + b._received_messages)
    for x, y in zip(recs_a, recs_b):  # (the three fields, not the padding between them)
        assert np.array_equal(_fields_of(x, D), _fields_of(y, D))
    assert [_stat_tuple(c) for c in ca] == [_stat_tuple(c) for c in cb]


def _fields_of(rec, D):
    """The record's three fields, without the padding between them."""
    from fl_sim_amd import codec

    K = D // 100
    _, off = codec.sparse_wire_layout(D, K)
    nt = (D + 1023) // 1024 + 1
    return np.concatenate([rec[off["idx"]:off["idx"] + 4 * K], rec[off["val"]:off["val"] + 4 * K],
                           rec[off["tiles"]:off["tiles"] + 4 * nt]])


def test_deferred_messages_survive_what_happens_before_the_read():
    """A model changed in place after its message (the batch reads a snapshot), a statistic read mid-round (top-k's
    send count does not depend on the encode: it is right at once and nothing runs), a record read mid-round (the
    waiting batch runs, a second one follows), one compressor shared by every client: the vectors of
    ``compressVector``."""
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_delta

    shapes = CONFIG1_SHAPES
    D = _n(shapes)
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 6)
    glob = [t.cuda() for t in theta]
    comp = make_compressors("topk", D, rng="philox", seed=3)
    compressed.deferred_sparse_stats(reset=True)
    ds, want = [], []
    for i in range(6):
        loc = [t.clone().cuda() for t in locals_[i]]
        want.append(comp[0].compressVector(torch.cat([(a - b).reshape(-1) for a, b in zip(loc, glob)])).cpu().numpy())
        ds.append(compress_delta(loc, glob, comp, sparse=True))
        assert ds[-1]._batch is not None  # (waiting)
        for t in loc:
            t.mul_(-3.0)  # the client goes on training: the message must not change
        if i == 2:
            assert comp[0].really_need_to_send_components == 6 * (D // 100)  # (3 messages, each counted twice here)
            assert comp[0].total_input_components == 6 * D and comp[0].last_need_to_send_advance == D // 100
            assert compressed.deferred_sparse_stats() == {"batches": 0, "messages": 0}
            assert _is_record(ds[0], D)  # (reads the record: the batch of the three runs)
            assert compressed.deferred_sparse_stats() == {"batches": 1, "messages": 3}
            assert all(d._batch is None for d in ds)
    assert compressed.deferred_sparse_stats() == {"batches": 1, "messages": 3}
    for d, w in zip(ds, want):
        assert gc.same_bits(d.flat().cpu().numpy(), w)
    assert compressed.deferred_sparse_stats() == {"batches": 2, "messages": 6}


@pytest.mark.parametrize("codec", ["topk", "randk"])
def test_message_pickles_as_its_record(codec):
    from fl_sim_amd.compressed import compress_delta

    shapes = CONFIG1_SHAPES
    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 1)
    D = _n(shapes)
    d = compress_delta([t.cuda() for t in locals_[0]], [t.cuda() for t in theta],
                       make_compressors(codec, D, rng="philox", seed=4), sparse=True)
    assert (d._batch is not None) == (codec == "topk")  # (a waiting top-k message: the copy runs the batch first)
    blob = pickle.dumps(d)
    assert d._batch is None and len(blob) <= d.nbytes + 1024 and d.nbytes < 4 * D
    dense = d.flat().cpu().numpy()
    for x in (pickle.loads(blob), copy.deepcopy(d)):
        assert x.kind == "sparse" and x.nbytes == d.nbytes and x.k == d.k and x._batch is None
        assert np.array_equal(x.record.cpu().numpy(), d.record.cpu().numpy())
        assert gc.same_bits(x.flat().cpu().numpy(), dense)
        assert [tuple(t.shape) for t in x] == [tuple(sh) for sh in shapes]


# ------------------------------------------------------------------------------------------------ 3. fallbacks
def _message(codec_or_comps, shapes, seed=9, dtype=torch.float32, **kw):
    from fl_sim_amd.compressed import compress_delta

    theta, _, _, locals_, _ = round_inputs(shapes, "avg", 1)
    D = _n(shapes)
    comps = make_compressors(codec_or_comps, D) if isinstance(codec_or_comps, str) else codec_or_comps
    gc.seed_all(seed)
    return compress_delta([t.to(dtype).cuda() for t in locals_[0]], [t.to(dtype).cuda() for t in theta], comps, **kw)


def test_option_off_is_unchanged():
    """Without the option (the default, ``sparse_records`` false, and ``wire_records`` alone) top-k and rand-k send
    their decoded vectors, byte for byte the message of ``compressVector``."""
    from fl_sim_amd.compressed import record_round, sparse_round

    shapes = SMALL_SHAPES
    D = _n(shapes)
    for codec in ("topk", "randk"):
        s, clients = build_round(shapes, "avg", "cuda")
        gc.seed_all(1)
        for i, c in enumerate(clients[:4]):
            c.compressors = make_compressors(codec, D)
            if i == 1:
                c.sparse_records = False
            if i == 2:
                c.config = types.SimpleNamespace(sparse_records=0)
            if i == 3:
                c.wire_records = True  # (the other switch: not these compressors')
            c.communicate(s)
        msgs = s._received_messages
        assert all(m["delta_parameters"].kind == "dense" and m["delta_parameters"].nbytes == 4 * D for m in msgs)
        assert sparse_round(msgs) is None and record_round(msgs) is None
        gc.seed_all(1)
        for c, m in zip(clients[:4], msgs):
            x = torch.cat([(p.detach() - q).reshape(-1) for p, q in zip(c.model.parameters(), c._cached_parameters)])
            want = make_compressors(codec, D)[0].compressVector(x)
            assert gc.same_bits(m["delta_parameters"].flat().cpu().numpy(), want.cpu().numpy())


def test_lists_without_a_sparse_record_ignore_the_option():
    """``sparse`` on with K = 0, K >= n, a record that would not be smaller than the vector, a float64 model, the
    stacked pipeline or a quantizer: the message of the option off, bit for bit."""
    from fl_sim_amd import Compressor

    shapes = SMALL_SHAPES
    D = _n(shapes)

    def topk(K):
        c = Compressor()
        c.makeTopKCompressor(K, D)
        return [c]

    cases = [(lambda: topk(0), "dense", {}), (lambda: topk(D), "dense", {}), (lambda: topk(D + 5), "dense", {}),
             (lambda: topk(D // 2), "dense", {}),  # 8 K + tile pointers >= 4 n
             (lambda: make_compressors("topk", D), "dense", dict(dtype=torch.float64)),
             (lambda: make_compressors("randk", D), "dense", dict(dtype=torch.float64)),
             (lambda: make_compressors("stacked10", D), "stacked", {}),
             (lambda: make_compressors("std8inf", D), "dense", {}),
             (lambda: make_compressors("natural", D), "dense", {})]
    for mk, kind, kw in cases:
        a = _message(mk(), shapes, **kw)
        b = _message(mk(), shapes, sparse=True, **kw)
        assert a.kind == b.kind == kind, (kind, kw)
        assert a.nbytes == b.nbytes
        assert gc.same_bits(a.flat().cpu().numpy(), b.flat().cpu().numpy())
    # the quantizers' records keep their own switch
    assert _message("std8inf", shapes, sparse=True, wire=True).kind == "quant"
    assert _message("topk", shapes, sparse=True, wire=True).kind == "sparse"
    assert _message("topk", shapes, wire=True).kind == "dense"


def test_mixed_round_falls_back_to_per_message_decoding():
    """A dense message, a stacked record and records of another K among the sparse records: no record round, every
    message decodes itself, and the update equals the update from the decoded messages."""
    from fl_sim_amd import Compressor
    from fl_sim_amd import aggregation as agg
    from fl_sim_amd.compressed import record_round, sparse_round, stacked_round

    shapes = SMALL_SHAPES
    D = _n(shapes)
    s, clients = build_round(shapes, "adam", "cuda")
    gc.seed_all(2)
    for i, c in enumerate(clients):
        c.compressors = make_compressors("stacked10" if i == 0 else "randk" if i == 3 else "topk", D)
        if i == 5:
            c.compressors = [Compressor()]
            c.compressors[0].makeTopKCompressor(D // 50, D)
        c.sparse_records = i != 7
        c.communicate(s)
    msgs = s._received_messages
    kinds = [m["delta_parameters"].kind for m in msgs]
    assert kinds == ["stacked"] + ["sparse"] * 6 + ["dense"] + ["sparse"] * 2
    assert stacked_round(msgs) is None and sparse_round(msgs) is None and record_round(msgs) is None
    assert sparse_round(msgs[1:5]) is not None and sparse_round(msgs[1:7]) is None  # (another K among them)
    assert record_round(msgs[1:5]) == [m["delta_parameters"] for m in msgs[1:5]]
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
