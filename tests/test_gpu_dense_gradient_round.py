"""The variance-reduced servers' call site with ``wire_records`` on: FedProx, FedPD, ProxSkip and pFedMac clients send
their ``gradients`` as dense records (flc_dense_wire_layout) and the servers fold the records beside the dense
parameters in one pass (flc_avg_and_gradient_dense_records), never decoding one — against the reference's own rounds
(tests/golden/vr_codec.npz: the fixture that pins the same rounds with the option off), bit for bit, on a device- and a
host-resident server, with the send statistics and both global streams in lock-step; philox mode against the same round
with the option off; both ways to the kernel (the one-C-call extension entries and ctypes), for dense and for sparse
records; mixed rounds, a model the launch does not take, error feedback."""

import random
import types

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import test_gpu_vr_codec as tvr
from tests.golden.gen_golden import CONFIG1_SHAPES, SMALL_SHAPES, VR_SERVERS, vr_inputs
from tests.golden.gen_golden_vr_codec import vr_codec_key, vr_codec_seed
from tests.test_gpu_dense_record_round import _is_record, _philox_compressor, _stat_tuple
from tests.test_gpu_round import make_compressors

pytestmark = pytest.mark.gpu


def _n(shapes):
    return sum(int(np.prod(sh)) for sh in shapes)


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1)


def _switch_on(c, i):
    if i % 2:  # (the two places the option is looked up)
        c.wire_records = True
    else:
        c.config.wire_records = True


@pytest.fixture(autouse=True)
def _no_leftovers():
    from fl_sim_amd import compressed

    compressed._run_pending()  # (messages earlier tests left waiting)
    yield
    compressed._run_pending()


def _compat_round(name, codec, tag, nm, where, switch=_switch_on):
    """The fixture's round with records on: (server, key); the streams and statistics are checked here."""
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
        switch(c, i)
        c.communicate(s)
        stats.append([float(x.last_need_to_send_advance) for x in c.gradient_compressors]
                     + [float(x.total_input_components) for x in c.gradient_compressors])
    assert random.random() == float(tvr.VRC[key + "|next_random"])
    assert np.random.random_sample() == float(tvr.VRC[key + "|next_np"])
    assert np.array_equal(np.array(stats, dtype=np.float64), tvr.VRC[key + "|stats"])
    assert len(s._received_messages) == nm
    return s, key, D


# ------------------------------------------------------------------------------ 1. compat mode against the reference
@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("tag,nm", [("small", 10), ("config1", 10), ("small", 20)])
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
@pytest.mark.parametrize("name", list(VR_SERVERS))
def test_vr_round_with_dense_gradient_records_matches_reference(name, codec, tag, nm, where):
    s, key, D = _compat_round(name, codec, tag, nm, where)
    got = s._received_messages
    assert all(_is_record(m["gradients"], codec, D) for m in got)
    assert all(isinstance(m["parameters"], list) for m in got)  # (the parameters as the reference sends them)
    s.update()
    assert all(m["gradients"]._flat is None for m in got)  # (never decoded densely)
    assert tvr._same(key, "theta", list(s.model.parameters()))
    assert tvr._same(key, "grad", [p.grad for p in s.model.parameters()])
    dev = "cuda" if where == "device" else "cpu"
    assert all(p.device.type == dev and p.grad.device.type == dev for p in s.model.parameters())


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_update_gradients_alone_folds_the_records(codec, where):
    """``update_gradients`` over such messages: the fixture's gradients, the parameters untouched, nothing decoded."""
    from fl_sim_amd import aggregation as agg

    s, key, D = _compat_round("fedprox", codec, "small", 10, where)
    got = s._received_messages
    ps = list(s.model.parameters())
    before = [p.detach().clone() for p in ps]
    grads = agg.update_gradients(ps, got)
    assert all(m["gradients"]._flat is None for m in got)
    assert tvr._same(key, "grad", grads) and tvr._same(key, "grad", [p.grad for p in ps])
    for p, p0 in zip(ps, before):
        assert torch.equal(p.detach().view(torch.int32), p0.view(torch.int32))
        assert p.grad.device == p.device and p.grad.shape == p.shape


# ------------------------------------------------------------------------------------------------ 2. philox mode
def _philox_fedprox(codec, wire, n_clients=10):
    shapes = CONFIG1_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, n_clients)
    s = tvr._server("fedprox", params, "device")
    comps = []
    for i, src in enumerate(msgs):
        c = tvr._client(src)
        c.gradient_compressors = _philox_compressor(codec, D, 500 + i)
        for _ in range(i % 3):  # (counters that differ between the clients)
            c.gradient_compressors[0].philox.next()
        c.wire_records = wire
        c.communicate(s)
        comps.append(c.gradient_compressors[0])
    return s, comps


@pytest.mark.parametrize("defer", [True, False])
@pytest.mark.parametrize("codec", ["std8inf", "std4p2", "natd7"])
def test_philox_records_on_equal_records_off(codec, defer, monkeypatch):
    """Two identically seeded sets of compressors, ``wire_records`` off and on, one FedProx round of 10 clients: θ,
    ``.grad``, the send statistics and the Philox counters bit for bit, with the round's encode deferred and not."""
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
    a, ca = _philox_fedprox(codec, False)
    b, cb = _philox_fedprox(codec, True)
    assert all(m["gradients"].kind == "dense" for m in a._received_messages)
    assert all(m["gradients"].kind == "quant" and m["gradients"].nbytes < 4 * m["gradients"].n
               for m in b._received_messages)
    a.update()
    b.update()
    assert all(m["gradients"]._flat is None for m in b._received_messages)
    assert [_stat_tuple(c) for c in ca] == [_stat_tuple(c) for c in cb]
    for x, y in zip(a.model.parameters(), b.model.parameters()):
        assert gc.same_bits(_bits(x), _bits(y)) and gc.same_bits(_bits(x.grad), _bits(y.grad))
    assert any(bool(p.grad.any()) for p in b.model.parameters())


# ------------------------------------------------------------------------------------- 3. both ways to the kernel
def _record_messages(kind, n_msgs=10):
    """A philox round's messages with dense (8-bit dithering) or sparse (top-k) gradient records, and the same messages
    with the gradients as their decoded tensors."""
    shapes = CONFIG1_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, n_msgs)
    s = types.SimpleNamespace(_received_messages=[])
    for i, src in enumerate(msgs):
        c = tvr._client(src)
        c.gradient_compressors = make_compressors("std8inf" if kind == "dense" else "topk", D, rng="philox", seed=70 + i)
        c.wire_records, c.sparse_records = kind == "dense", kind == "sparse"
        c.communicate(s)
    recs = s._received_messages
    assert all(m["gradients"].kind == ("quant" if kind == "dense" else "sparse") for m in recs)
    dense = []
    for m in recs:
        d = m["gradients"]
        flat = (_decode_dense(d) if kind == "dense" else _decode_sparse(d))
        gs, off = [], 0
        for sh in d.shapes:
            gs.append(flat[off:off + sh.numel()].view(sh))
            off += sh.numel()
        dense.append(dict(m, gradients=gs))
    assert all(m["gradients"]._flat is None for m in recs)  # (decoded beside the messages, not through them)
    return params, recs, dense


def _decode_dense(d):
    from fl_sim_amd import codec

    return codec.dense_record_decode(d.record, d.n, d.format, d.levels, d.bits)


def _decode_sparse(d):
    from fl_sim_amd import codec

    return codec.sparse_record_decode(d.record, d.n, d.k)


@pytest.mark.parametrize("ext", [True, False])
@pytest.mark.parametrize("kind", ["dense", "sparse"])
def test_one_c_call_and_ctypes_paths_give_the_same_bits(kind, ext, monkeypatch):
    """avg_parameters_and_gradients and update_gradients over a round of records through the one-C-call entry
    (_flcfold.avg_and_gradient_dense_records / avg_and_gradient_sparse_records) and (``ext`` False: as when the
    extension is not built) through ctypes, against the same calls over the decoded gradients."""
    from fl_sim_amd import aggregation as agg
    from fl_sim_amd import codec

    cell, accessor = ("_PYGDRECS", codec._pygdrecs) if kind == "dense" else ("_PYGSRECS", codec._pygsrecs)
    calls = []
    if ext:
        real = accessor()
        assert real is not None, "the _flcfold extension must be built"

        def spy(*a):
            r = real(*a)
            calls.append(1)  # (returned: the launch ran)
            return r

        monkeypatch.setattr(codec, cell, [spy])
    else:
        monkeypatch.setattr(codec, cell, [None])
        assert accessor() is None
    params, recs, dense = _record_messages(kind)
    a = [torch.nn.Parameter(t.clone().cuda()) for t in params]
    b = [torch.nn.Parameter(t.clone().cuda()) for t in params]
    ga = agg.avg_parameters_and_gradients(a, recs, True, 0.2)
    gb = agg.avg_parameters_and_gradients(b, dense, True, 0.2)
    assert all(m["gradients"]._flat is None for m in recs)
    for x, y, u, v in zip(a, b, ga, gb):
        assert gc.same_bits(_bits(x), _bits(y))
        assert gc.same_bits(_bits(u), _bits(v)) and gc.same_bits(_bits(x.grad), _bits(v))
        assert x.grad.device == x.device and x.grad.shape == x.shape
    if ext:
        assert len(calls) == 1
        base = a[0].grad.untyped_storage().data_ptr()
        off = a[0].grad.data_ptr()
        for x in a:  # the `.grad` views lie back to back in one flat buffer
            assert x.grad.untyped_storage().data_ptr() == base and x.grad.data_ptr() == off
            off += 4 * x.numel()
    before = [p.detach().clone() for p in a]
    ga = agg.update_gradients(a, recs)
    gb = agg.update_gradients(b, dense)
    assert all(m["gradients"]._flat is None for m in recs)
    assert len(calls) == (2 if ext else 0)
    for x, x0, u, v in zip(a, before, ga, gb):
        assert torch.equal(x.detach().view(torch.int32), x0.view(torch.int32))
        assert gc.same_bits(_bits(u), _bits(v)) and gc.same_bits(_bits(x.grad), _bits(v))


def test_the_extension_entries_raise_type_error_before_anything_runs():
    """The TypeError-means-nothing-launched rule of avg_and_gradient_records, for the two new entries."""
    from fl_sim_amd import _flcfold

    for kind in ("dense", "sparse"):
        params, recs, _ = _record_messages(kind, 3)
        d0 = recs[0]["gradients"]
        ps = [t.clone().cuda() for t in params]
        keep = [p.clone() for p in ps]
        ps[4] = ps[4].t().contiguous().t()  # (a non-contiguous model tensor)
        keep[4] = ps[4].clone()
        rs = [m["gradients"].record for m in recs]
        w = [1 / 3] * 3
        with pytest.raises(TypeError):
            if kind == "dense":
                _flcfold.avg_and_gradient_dense_records(ps, recs, rs, w, w, d0.n, d0.format, d0.levels, d0.bits, 0.0, True)
            else:
                _flcfold.avg_and_gradient_sparse_records(ps, recs, rs, w, w, d0.n, d0.k, 0.0, True)
        with pytest.raises(TypeError):  # a record on the host
            good = [t.clone().cuda() for t in params]
            host = [rs[0].cpu()] + rs[1:]
            if kind == "dense":
                _flcfold.avg_and_gradient_dense_records(good, recs, host, w, w, d0.n, d0.format, d0.levels, d0.bits, 0.0)
            else:
                _flcfold.avg_and_gradient_sparse_records(good, recs, host, w, w, d0.n, d0.k, 0.0)
        torch.cuda.synchronize()
        for p, k in zip(ps, keep):
            assert torch.equal(p, k) and p.grad is None


# ------------------------------------------------------------------------------------------------ 4. fallbacks
@pytest.mark.parametrize("how", ["records_off", "four_bits"])
def test_mixed_round_decodes_per_message(how):
    """One client with ``wire_records`` off among the record clients: the fixture's round (the message is the decoded
    vector of the same draws), through the per-message decode.  One client at 4 bits among 8-bit clients: no record
    round either, and the update equals the update from the decoded messages."""
    from fl_sim_amd import aggregation as agg
    from fl_sim_amd.compressed import dense_record_round, record_round

    if how == "records_off":
        def switch(c, i):
            c.wire_records = i != 3

        s, key, D = _compat_round("fedprox", "std8inf", "small", 10, "device", switch)
        got = s._received_messages
        assert [m["gradients"].kind for m in got] == ["quant"] * 3 + ["dense"] + ["quant"] * 6
        assert record_round(got, key="gradients") is None and dense_record_round(got, key="gradients") is None
        assert dense_record_round(got[:3], key="gradients") is not None
        s.update()
        assert all(m["gradients"]._flat is not None for m in got)  # (each message decoded itself)
        assert tvr._same(key, "theta", list(s.model.parameters()))
        assert tvr._same(key, "grad", [p.grad for p in s.model.parameters()])
        return
    shapes = SMALL_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, 10)
    sent = types.SimpleNamespace(_received_messages=[])
    gc.seed_all(12)
    for i, src in enumerate(msgs):
        c = tvr._client(src)
        c.gradient_compressors = make_compressors("std4p2" if i == 5 else "std8inf", D)
        c.wire_records = True
        c.communicate(sent)
    got = sent._received_messages
    assert all(m["gradients"].kind == "quant" for m in got) and got[5]["gradients"].bits == 4
    assert record_round(got, key="gradients") is None
    assert dense_record_round(got[:5], key="gradients") is not None
    a = [torch.nn.Parameter(t.clone().cuda()) for t in params]
    b = [torch.nn.Parameter(t.clone().cuda()) for t in params]
    decoded = [dict(m, gradients=[t.clone() for t in m["gradients"]]) for m in got]
    agg.avg_parameters_and_gradients(a, got, False, 0.0)
    agg.avg_parameters_and_gradients(b, decoded, False, 0.0)
    for x, y in zip(a, b):
        assert gc.same_bits(_bits(x), _bits(y)) and gc.same_bits(_bits(x.grad), _bits(y.grad))


def test_a_model_the_launch_does_not_take_gets_the_right_result():
    """A non-contiguous parameter: the one-pass launch does not take the model, the parameters are averaged on the dense
    path, and the round still gives the fixture's θ and gradients."""
    shapes = SMALL_SHAPES
    D = _n(shapes)
    params, msgs = vr_inputs(shapes, 10)
    key = vr_codec_key("fedprox", "std8inf", 10, "small")
    s = tvr._server("fedprox", params, "device")
    p4 = torch.nn.Parameter(params[4].clone().cuda().t().contiguous().t())
    assert p4.shape == params[4].shape and not p4.is_contiguous()
    s.model.register_parameter("p4", p4)
    gc.seed_all(vr_codec_seed("fedprox", "std8inf", 10, "small"))
    for src in msgs:
        c = tvr._client(src)
        c.gradient_compressors = make_compressors("std8inf", D)
        c.wire_records = True
        c.communicate(s)
    assert all(_is_record(m["gradients"], "std8inf", D) for m in s._received_messages)
    s.update()
    ps = list(s.model.parameters())
    assert not ps[4].is_contiguous()
    assert tvr._same(key, "theta", ps)
    assert tvr._same(key, "grad", [p.grad for p in ps])


# ------------------------------------------------------------------------------------------------ 5. error feedback
@pytest.mark.parametrize("codec", ["std8inf", "natural"])
def test_error_feedback_on_a_gradient_client_with_records(codec):
    """Two rounds of three gradient clients with ``error_feedback``, ``wire_records`` on against off: the same messages
    and the same memories, and the server's round from the records equals the round from the option-off messages."""
    from fl_sim_amd import aggregation as agg
    from fl_sim_amd.compressed import CompressedGradientsClientMixin

    shapes = SMALL_SHAPES
    D = _n(shapes)
    g = torch.Generator().manual_seed(91)
    params = [torch.randn(sh, generator=g) for sh in shapes]
    rounds = [[[torch.randn(sh, generator=g) * 1e-2 for sh in shapes] for _ in range(3)] for _ in range(2)]

    class Base:
        def communicate(self, target):
            target._received_messages.append({"client_id": self.cid, "parameters": self.params, "gradients": self.grads,
                                              "train_samples": 10 + self.cid})

    class Client(CompressedGradientsClientMixin, Base):
        pass

    def run(wire):
        clients = []
        for i in range(3):
            c = Client()
            c.cid = i
            c.config = types.SimpleNamespace(error_feedback=True, wire_records=wire,
                                             gradient_compressors=make_compressors(codec, D, rng="philox", seed=80 + i))
            c.params = [t.clone().cuda() for t in params]
            clients.append(c)
        sent, thetas = [], []
        for r in range(2):
            s = types.SimpleNamespace(_received_messages=[])
            for c, gs in zip(clients, rounds[r]):
                c.grads = [t.clone().cuda() for t in gs]
                c.communicate(s)
            sent.append(s._received_messages)
            th = [torch.nn.Parameter(t.clone().cuda()) for t in params]
            agg.avg_parameters_and_gradients(th, s._received_messages, True, 0.1)
            thetas.append(th)
        return clients, sent, thetas

    ca, sa, ta = run(False)
    cb, sb, tb = run(True)
    for r in range(2):
        assert all(m["gradients"].kind == "dense" for m in sa[r])
        assert all(_is_record(m["gradients"], codec, D) for m in sb[r])  # (the server folded the records)
        for x, y in zip(ta[r], tb[r]):
            assert gc.same_bits(_bits(x), _bits(y)) and gc.same_bits(_bits(x.grad), _bits(y.grad))
        for ma, mb in zip(sa[r], sb[r]):
            assert gc.same_bits(_bits(ma["gradients"].flat()), _bits(mb["gradients"].flat()))
    for x, y in zip(ca, cb):
        assert gc.same_bits(_bits(x.error_memory("gradients").value()), _bits(y.error_memory("gradients").value()))
        assert _stat_tuple(x.config.gradient_compressors[0]) == _stat_tuple(y.config.gradient_compressors[0])
