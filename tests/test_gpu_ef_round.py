"""Error feedback at the codec's call site (fl_sim_amd/feedback.py, compressed.py), bit for bit: compat mode against the
reference's own compressor (tests/golden/ef_codec.npz), philox mode against tests/ef_ref.py — deferred (the memory is
the batched encode's flat input, one K-entry residual launch per round) and immediate —, the ordering and retry rules
of the memories, and whole FedOpt and SCAFFOLD rounds through the mixins."""

import random
import types

import numpy as np
import pytest
import torch

from tests import ef_ref
from tests import golden_cases as gc
from tests.golden.gen_golden import CONFIG1_SHAPES, ROUND_OPTS, SCAFFOLD_CFG, SMALL_SHAPES, round_inputs, round_seed
from tests.golden.gen_golden_delta_codec import scaffold_codec_inputs
from tests.golden.gen_golden_ef import (EF_CLIENTS, EF_CODECS, EF_ROUNDS, EF_TAGS, ef_inputs, ef_key, ef_seed,
                                        flat_delta)
from tests.test_gpu_delta_codec import _scaffold_client, _scaffold_server
from tests.test_gpu_round import _fields, _record_fields, _same as _round_same, build_round, make_compressors

pytestmark = pytest.mark.gpu
EF = np.load(f"{gc.GOLDEN}/ef_codec.npz", allow_pickle=False)
LEVELS = 10


def _same(key, a):
    if key + "|out" in EF.files and not gc.same_bits(a, EF[key + "|out"]):
        return False
    return gc.sha(a) == str(EF[key + "|sha"])


def _cuda(ts):
    return [t.clone().cuda() for t in ts]


def _n(shapes):
    return sum(int(np.prod(s)) for s in shapes)


@pytest.fixture(autouse=True)
def _no_leftovers():
    from fl_sim_amd import compressed

    compressed._run_pending()  # (messages earlier tests left waiting)
    yield
    compressed._run_pending()


# ---------------------------------------------------------------------------------------- compat mode, the reference
@pytest.mark.parametrize("tag", list(EF_TAGS))
@pytest.mark.parametrize("codec", EF_CODECS)
def test_compat_rounds_match_the_reference(codec, tag):
    """4 clients × 3 rounds through compress_delta(feedback=...): every message (a record for the stacked pipeline,
    the decoded flat otherwise), the final memories, the accumulated statistics and both streams' positions."""
    from fl_sim_amd.compressed import compress_delta
    from fl_sim_amd.feedback import ErrorMemory

    shapes = EF_TAGS[tag]
    cached, locals_ = ef_inputs(shapes)
    n, key = _n(shapes), ef_key(codec, tag)
    dc = _cuda(cached)
    comps = [make_compressors(codec, n) for _ in range(EF_CLIENTS)]
    mems = [ErrorMemory(n, "cuda") for _ in range(EF_CLIENTS)]
    gc.seed_all(ef_seed(codec, tag))
    for r in range(EF_ROUNDS):
        for i in range(EF_CLIENTS):
            d = compress_delta(_cuda(locals_[r][i]), dc, comps[i], feedback=mems[i])
            assert d.kind == ("stacked" if codec == "stacked10" else "dense")
            if codec == "stacked10":
                assert d.nbytes < n
            else:
                assert d.flat().data_ptr() != mems[i].value().data_ptr()
            assert _same(f"{key}|c{r}_{i}", d.flat().cpu().numpy()), (r, i)
    for i in range(EF_CLIENTS):
        assert _same(f"{key}|e{i}", mems[i].value().cpu().numpy()), i
    stats = [[float(x.really_need_to_send_components) for x in cs] + [float(x.total_input_components) for x in cs]
             + [float(x.last_need_to_send_advance) for x in cs] for cs in comps]
    assert np.array_equal(np.array(stats, dtype=np.float64), EF[key + "|stats"])
    assert random.random() == float(EF[key + "|next_random"])
    assert np.random.random_sample() == float(EF[key + "|next_np"])


# ------------------------------------------------------------------------------------------- philox mode, the oracle
def _philox_rounds(shapes, defer, monkeypatch, n_clients=10, sampled=4, rounds=4, gradients=False):
    """Clients sampled ``sampled`` of ``n_clients`` per round (so their Philox counters differ within a round); per
    round: the records' fields, read after the round's last message.  Returns (records per round and sampled client,
    final memories, the sampling, the batches run)."""
    from fl_sim_amd import compressed
    from fl_sim_amd.feedback import ErrorMemory

    monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
    n = _n(shapes)
    g = torch.Generator().manual_seed(41)
    cached = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    dc = _cuda(cached)
    comps = [make_compressors("stacked10", n, rng="philox", seed=300 + i) for i in range(n_clients)]
    mems = [ErrorMemory(n, "cuda") for _ in range(n_clients)]
    pick = random.Random(5)
    compressed.deferred_stats(reset=True)
    recs, xs, who = [], [], []
    for r in range(rounds):
        ids = sorted(pick.sample(range(n_clients), sampled))
        ds, rx = [], []
        for i in ids:
            local = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached]
            if gradients:
                x = torch.cat([t.reshape(-1) for t in local]).numpy()
                ds.append(compressed.compress_tensors(_cuda(local), comps[i], feedback=mems[i]))
            else:
                x = flat_delta(local, cached)
                ds.append(compressed.compress_delta(_cuda(local), dc, comps[i], feedback=mems[i]))
            rx.append(x)
        recs.append([_record_fields(d) for d in ds])
        xs.append(rx)
        who.append(ids)
    return recs, [m.value().cpu().numpy() for m in mems], xs, who, compressed.deferred_stats()


def _oracle_rounds(n, xs, who, n_clients=10):
    K = n // 100
    e = [np.zeros(n, dtype=np.float32) for _ in range(n_clients)]
    ctr = [0] * n_clients
    out = []
    for rx, ids in zip(xs, who):
        row = []
        for x, i in zip(rx, ids):
            c, e[i], kept, codes, norm = ef_ref.philox_round(e[i], x, K, LEVELS, 300 + i, ctr[i])
            ctr[i] += 1
            row.append((c, kept, codes, norm))
        out.append(row)
    return out, e


@pytest.mark.parametrize("tag,gradients", [("small", False), ("config1", False), ("small", True)])
def test_philox_rounds_match_the_oracle_deferred_and_immediate(tag, gradients, monkeypatch):
    """4 of 10 clients per round for 4 rounds: records and memories identical deferred and immediate, and equal to
    the oracle's; deferred, one batched encode per round."""
    shapes = EF_TAGS[tag]
    n, K = _n(shapes), _n(shapes) // 100
    ra, ea, xs, who, sa = _philox_rounds(shapes, True, monkeypatch, gradients=gradients)
    rb, eb, xs_b, who_b, sb = _philox_rounds(shapes, False, monkeypatch, gradients=gradients)
    assert who == who_b and sa == {"batches": 4, "messages": 16} and sb == {"batches": 0, "messages": 0}
    assert len({tuple(w) for w in who}) > 1
    for r in range(4):
        for j in range(4):
            assert np.array_equal(ra[r][j], rb[r][j]), (r, j)
    for i in range(10):
        assert np.array_equal(ea[i].view(np.uint32), eb[i].view(np.uint32)), i
    want, e = _oracle_rounds(n, xs, who)
    for r in range(4):
        for j in range(4):
            c, kept, codes, norm = want[r][j]
            f = ra[r][j]  # norm (4 B), idx (4 K B), codes (K B), tiles
            assert np.array_equal(f[:4].view(np.float32), np.array([norm], dtype=np.float32)), (r, j)
            assert np.array_equal(f[4:4 + 4 * K].view(np.int32).astype(np.int64), kept), (r, j)
            assert np.array_equal(f[4 + 4 * K:4 + 5 * K], codes), (r, j)
    for i in range(10):
        assert gc.same_bits(ea[i], e[i]), i
    assert any(np.any(e[i]) for i in range(10))


def _one_client(shapes, seed=7, comp_seed=77):
    from fl_sim_amd.feedback import ErrorMemory

    n = _n(shapes)
    g = torch.Generator().manual_seed(seed)
    cached = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    locals_ = [[t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached] for _ in range(3)]
    return n, cached, locals_, _cuda(cached), make_compressors("stacked10", n, rng="philox", seed=comp_seed), \
        ErrorMemory(n, "cuda")


def test_zero_memory_sends_the_plain_record_then_differs():
    """Round 1 from a zero memory: the record of the same call without feedback, bit for bit; round 2 is not."""
    from fl_sim_amd.compressed import compress_delta

    n, cached, locals_, dc, comps, mem = _one_client(SMALL_SHAPES)
    plain = make_compressors("stacked10", n, rng="philox", seed=77)
    for r, equal in ((0, True), (1, False)):
        a = _record_fields(compress_delta(_cuda(locals_[r]), dc, comps, feedback=mem))
        b = _record_fields(compress_delta(_cuda(locals_[r]), dc, plain))
        assert np.array_equal(a, b) == equal, r
    assert comps[1].philox.counter == plain[1].philox.counter == 2  # (the same RNG advance)
    assert comps[0].total_input_components == plain[0].total_input_components == 2 * n


def test_two_messages_before_a_read_equal_two_sequential_rounds(monkeypatch):
    """A client that communicates again while its memory still waits in a batch: that batch runs first (one batch per
    message), and the memory equals two sequential rounds'."""
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    n, cached, locals_, dc, comps, mem = _one_client(SMALL_SHAPES)
    compressed.deferred_stats(reset=True)
    d0 = compressed.compress_delta(_cuda(locals_[0]), dc, comps, feedback=mem)
    assert d0._batch is not None and mem._batch is d0._batch
    d1 = compressed.compress_delta(_cuda(locals_[1]), dc, comps, feedback=mem)
    assert d0._batch is None and d1._batch is not None
    assert compressed.deferred_stats() == {"batches": 1, "messages": 1}
    e, K = np.zeros(n, dtype=np.float32), n // 100
    for r, d in enumerate((d0, d1)):
        c, e, kept, codes, norm = ef_ref.philox_round(e, flat_delta(locals_[r], cached), K, LEVELS, 77, r)
        assert gc.same_bits(d.flat().cpu().numpy(), c), r
    assert gc.same_bits(mem.value().cpu().numpy(), e)
    assert compressed.deferred_stats() == {"batches": 2, "messages": 2}


def test_value_mid_round_runs_the_batch_and_reset_zeroes(monkeypatch):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    n, cached, locals_, dc, comps, mem = _one_client(SMALL_SHAPES)
    d = compressed.compress_delta(_cuda(locals_[0]), dc, comps, feedback=mem)
    other = compressed.compress_delta(_cuda(locals_[1]), dc, make_compressors("stacked10", n, rng="philox", seed=78))
    assert d._batch is not None and other._batch is d._batch and compressed._PENDING
    v = mem.value()  # (runs the round's batch: the plain message's record is made too)
    assert d._batch is None and other._batch is None and not compressed._PENDING and mem._batch is None
    c, e, *_ = ef_ref.philox_round(np.zeros(n, dtype=np.float32), flat_delta(locals_[0], cached), n // 100, LEVELS, 77, 0)
    assert gc.same_bits(v.cpu().numpy(), e) and np.any(e)
    assert mem.value() is v
    d2 = compressed.compress_delta(_cuda(locals_[1]), dc, comps, feedback=mem)
    mem.reset()  # (after the pending work)
    assert d2._batch is None and not bool(mem.value().any())
    assert np.array_equal(mem.value().cpu().numpy().view(np.uint32), np.zeros(n, dtype=np.uint32))


def test_a_raised_encode_leaves_the_memory_for_the_retry(monkeypatch):
    """The batched encode raises once: the batch stays pending, the memory still holds a (no residual applied); the
    retry encodes the same a and applies the residual exactly once."""
    from fl_sim_amd import codec, compressed

    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    n, cached, locals_, dc, comps, mem = _one_client(SMALL_SHAPES)
    real = codec._pyround()
    assert real is not None
    calls = []

    def failing(*a):
        calls.append(1)
        if len(calls) == 1:
            raise RuntimeError("injected")
        return real(*a)

    monkeypatch.setattr(codec, "_pyround", lambda: failing)
    d = compressed.compress_delta(_cuda(locals_[0]), dc, comps, feedback=mem)
    x = flat_delta(locals_[0], cached)
    with pytest.raises(RuntimeError, match="injected"):
        d.record
    assert d._batch is not None and mem._batch is d._batch
    assert gc.same_bits(mem._e.cpu().numpy(), x)  # (a = 0 + x, untouched)
    c, e, *_ = ef_ref.philox_round(np.zeros(n, dtype=np.float32), x, n // 100, LEVELS, 77, 0)
    assert gc.same_bits(d.flat().cpu().numpy(), c)
    assert gc.same_bits(mem.value().cpu().numpy(), e) and len(calls) == 2


def test_memory_written_on_a_side_stream_and_encoded_on_another(monkeypatch):
    """The accumulate runs on a side stream behind a long fill; the batch is encoded (and the residual applied) on the
    default stream, and the next round's accumulate on a second side stream: each waits for the memory's last
    writer."""
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    n, cached, locals_, dc, comps, mem = _one_client(CONFIG1_SHAPES)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ds = []
    for r, s in enumerate((s1, s2)):
        ls = _cuda(locals_[r])
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            big = torch.empty(1 << 26, device="cuda")  # (a long fill ahead of the accumulate on that stream)
            big.fill_(1.0)
            ds.append(compressed.compress_delta(ls, dc, comps, feedback=mem))
        if r == 0:
            ds[0].record  # (encoded on the default stream)
    e, K = np.zeros(n, dtype=np.float32), n // 100
    for r in range(2):
        c, e, *_ = ef_ref.philox_round(e, flat_delta(locals_[r], cached), K, LEVELS, 77, r)
        assert gc.same_bits(ds[r].flat().cpu().numpy(), c), r
    assert gc.same_bits(mem.value().cpu().numpy(), e)


def test_seventy_messages_in_one_round(monkeypatch):
    """70 clients with a memory each, two rounds: a batch runs itself at 64 messages, the residual launch chains past
    32 clients; every record and memory equals the oracle's."""
    from fl_sim_amd import compressed
    from fl_sim_amd.feedback import ErrorMemory

    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    shapes, C = SMALL_SHAPES, 70
    n, K = _n(shapes), _n(shapes) // 100
    g = torch.Generator().manual_seed(43)
    cached = [torch.randn(s, generator=g) * 0.1 for s in shapes]
    dc = _cuda(cached)
    comps = [make_compressors("stacked10", n, rng="philox", seed=900 + i) for i in range(C)]
    mems = [ErrorMemory(n, "cuda") for _ in range(C)]
    e = [np.zeros(n, dtype=np.float32) for _ in range(C)]
    compressed.deferred_stats(reset=True)
    for r in range(2):
        locs = [[t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached] for _ in range(C)]
        ds = [compressed.compress_delta(_cuda(locs[i]), dc, comps[i], feedback=mems[i]) for i in range(C)]
        for i in range(C):
            c, e[i], *_ = ef_ref.philox_round(e[i], flat_delta(locs[i], cached), K, LEVELS, 900 + i, r)
            assert gc.same_bits(ds[i].flat().cpu().numpy(), c), (r, i)
    assert compressed.deferred_stats() == {"batches": 4, "messages": 140}
    for i in range(C):
        assert gc.same_bits(mems[i].value().cpu().numpy(), e[i]), i


@pytest.mark.parametrize("defer", [True, False])
def test_converted_inputs_give_the_same_records_and_memories(defer, monkeypatch):
    """A host-resident, non-contiguous or float64 model goes through the converting accumulate (the extension's call
    raises TypeError before anything is written): the same records and the same fp32 memory on the device."""
    from fl_sim_amd import compressed
    from fl_sim_amd.feedback import ErrorMemory

    monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
    g = torch.Generator().manual_seed(47)
    shapes = [(16, 1, 5, 5), (16,), (256, 37), (10,)]
    n = _n(shapes)
    glob = [torch.randn(sh, generator=g) for sh in shapes]
    locs = [[t + torch.randn(t.shape, generator=g) * 1e-2 for t in glob] for _ in range(2)]
    forms = {
        "device": lambda ls: ([t.cuda() for t in ls], [t.cuda() for t in glob]),
        "host": lambda ls: (ls, [t.cuda() for t in glob]),
        "noncontig": lambda ls: ([t.cuda() if i != 2 else t.cuda().t().contiguous().t() for i, t in enumerate(ls)],
                                 [t.cuda() for t in glob]),
        "float64": lambda ls: ([t.double().cuda() for t in ls], [t.cuda() for t in glob]),
    }
    got = {}
    for name, form in forms.items():
        comps = make_compressors("stacked10", n, rng="philox", seed=5)
        mem = ErrorMemory(n, "cuda")
        recs = [_record_fields(compressed.compress_delta(*form(ls), comps, feedback=mem)) for ls in locs]
        v = mem.value()
        assert v.dtype is torch.float32 and v.is_cuda
        got[name] = (recs, v.cpu().numpy(), comps[1].really_need_to_send_components, comps[1].philox.counter)
    e = np.zeros(n, dtype=np.float32)
    for r, ls in enumerate(locs):
        c, e, kept, *_ = ef_ref.philox_round(e, flat_delta(ls, glob), n // 100, LEVELS, 5, r)
    assert gc.same_bits(got["device"][1], e)
    for name in ("host", "noncontig", "float64"):  # (the float64 copies of fp32 values convert back exactly)
        assert all(np.array_equal(x, y) for x, y in zip(got[name][0], got["device"][0])), name
        assert np.array_equal(got[name][1].view(np.uint32), got["device"][1].view(np.uint32)), name
        assert got[name][2:] == got["device"][2:], name


def test_ifca_message_with_feedback():
    """CompressedIFCAClientMixin with ``error_feedback``: the FedOpt message plus ``cluster_id``, one memory."""
    from fl_sim_amd.compressed import CompressedIFCAClientMixin

    class Client(CompressedIFCAClientMixin):
        pass

    n, cached, locals_, dc, comps, _ = _one_client(SMALL_SHAPES)
    c = Client()
    c.client_id, c.cluster_id, c._metrics, c.error_feedback, c.compressors = 3, 2, {}, True, comps
    c.train_loader = types.SimpleNamespace(dataset=range(11))
    c._cached_parameters = dc
    c.model = torch.nn.Module()
    for j, t in enumerate(locals_[0]):
        c.model.register_parameter(f"p{j}", torch.nn.Parameter(t.clone().cuda()))
    s = types.SimpleNamespace(_received_messages=[])
    e = np.zeros(n, dtype=np.float32)
    for r in range(2):
        for p, t in zip(c.model.parameters(), locals_[r]):
            p.data.copy_(t)
        c.communicate(s)
        m = s._received_messages[-1]
        assert m["cluster_id"] == 2 and m["client_id"] == 3 and m["delta_parameters"].kind == "stacked"
        out, e, *_ = ef_ref.philox_round(e, flat_delta(locals_[r], cached), n // 100, LEVELS, 77, r)
        assert gc.same_bits(m["delta_parameters"].flat().cpu().numpy(), out), r
    assert gc.same_bits(c.error_memory("delta_parameters").value().cpu().numpy(), e)


def test_wrong_memory_raises():
    from fl_sim_amd.compressed import compress_delta, compress_tensors
    from fl_sim_amd.feedback import ErrorMemory

    n, cached, locals_, dc, comps, mem = _one_client(SMALL_SHAPES)
    with pytest.raises(ValueError, match="holds"):
        compress_delta(_cuda(locals_[0]), dc, comps, feedback=ErrorMemory(n + 1, "cuda"))
    with pytest.raises(ValueError, match="holds"):
        compress_tensors(_cuda(locals_[0]), comps, feedback=ErrorMemory(n - 1, "cuda"))
    with pytest.raises(ValueError):
        ErrorMemory(n, "cpu")
    assert comps[1].philox.counter == 0  # (nothing consumed)


# ------------------------------------------------------------------------------------------------ through the mixins
def _tensors(flat, shapes):
    ts, off = [], 0
    for sh in shapes:
        m = int(np.prod(sh))
        ts.append(torch.from_numpy(flat[off:off + m].copy()).view(sh))
        off += m
    return ts


@pytest.mark.parametrize("server", ["device", "host"])
def test_fedopt_rounds_with_feedback_match_the_oracle(server):
    """CompressedFedOptClientMixin with ``error_feedback`` (on the client or on its config) and FedOptUpdateMixin, two
    rounds on a device- and a host-resident server: δ and θ equal the oracle's messages folded by the reference's
    update restated; ``error_memory`` returns the memories."""
    from oracle import aggregation_ref as agg_ref

    shapes, opt = SMALL_SHAPES, "avg"
    n, K = _n(shapes), _n(shapes) // 100
    s, clients = build_round(shapes, opt, "cuda" if server == "device" else "cpu")
    theta, delta, v, locals_, sizes = round_inputs(shapes, opt)
    cached = [t.clone() for t in theta]
    cfg = ROUND_OPTS[opt]
    for i, c in enumerate(clients):
        c.compressors = make_compressors("stacked10", n, rng="philox", seed=100 + i)
        if i % 2:
            c.error_feedback = True
        else:
            c.config = types.SimpleNamespace(error_feedback=True)
        assert c.error_memory("delta_parameters") is None
    e = [np.zeros(n, dtype=np.float32) for _ in clients]
    g = torch.Generator().manual_seed(44)
    for r in range(2):
        msgs = []
        for i, c in enumerate(clients):
            if r:  # (the model moves on; the cached parameters stay)
                locals_[i] = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in locals_[i]]
                for p, t in zip(c.model.parameters(), locals_[i]):
                    p.data.copy_(t)
            c.communicate(s)
            out, e[i], *_ = ef_ref.philox_round(e[i], flat_delta(locals_[i], cached), K, LEVELS, 100 + i, r)
            msgs.append({"delta_parameters": _tensors(out, shapes)})
        assert all(m["delta_parameters"].kind == "stacked" for m in s._received_messages)
        s.update()
        assert all(m["delta_parameters"]._flat is None for m in s._received_messages)  # (never decoded densely)
        s._received_messages = []
        agg_ref.fedopt_update(theta, delta, v, msgs, opt, cfg["lr"], cfg["betas"], cfg["tau"])
        assert gc.same_bits(ef_ref.flat_of(s.delta_parameters), ef_ref.flat_of(delta)), r
        assert gc.same_bits(ef_ref.flat_of(list(s.model.parameters())), ef_ref.flat_of(theta)), r
    for i, c in enumerate(clients):
        assert gc.same_bits(c.error_memory("delta_parameters").value().cpu().numpy(), e[i]), i


def test_scaffold_rounds_with_two_memories_match_the_oracle():
    """CompressedSCAFFOLDClientMixin with ``error_feedback``: one memory for ``parameters_delta``, one for
    ``control_variates_delta``; two rounds through SCAFFOLDUpdateMixin equal the oracle composed with the reference's
    update restated."""
    from fl_sim_amd import compressed
    from oracle import aggregation_ref as agg_ref

    shapes = SMALL_SHAPES
    n, K = _n(shapes), _n(shapes) // 100
    theta, cvs, srcs = scaffold_codec_inputs(shapes)
    s = _scaffold_server(theta, cvs, "device")
    clients = [_scaffold_client(src, ("stacked10", "stacked10"), n, rng="philox", seed=500 + i)
               for i, src in enumerate(srcs)]
    keys = ("parameters_delta", "control_variates_delta")
    e = [{k: np.zeros(n, dtype=np.float32) for k in keys} for _ in clients]
    g = torch.Generator().manual_seed(45)
    compressed.deferred_stats(reset=True)
    for r in range(2):
        want = []
        for i, (c, src) in enumerate(zip(clients, srcs)):
            c.error_feedback = True
            if r:
                src["cv"] = src["ucv"]  # (the reference's side effect of the round before)
                src["local"] = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in src["local"]]
                src["ucv"] = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in src["cv"]]
                for p, t in zip(c.model.parameters(), src["local"]):
                    p.data.copy_(t)
                c._updated_control_variates = _cuda(src["ucv"])
            c.communicate(s)
            m = {}
            for k, a, b, seed in zip(keys, (src["local"], src["ucv"]), (src["cached"], src["cv"]),
                                     (500 + i, 1500 + i)):
                out, e[i][k], *_ = ef_ref.philox_round(e[i][k], flat_delta(a, b), K, LEVELS, seed, r)
                m[k] = _tensors(out, shapes)
            want.append(m)
        s.update()
        assert all(m[k].kind == "stacked" and m[k]._flat is None for m in s._received_messages for k in keys)
        s._received_messages = []
        agg_ref.scaffold_update(theta, cvs, want, SCAFFOLD_CFG["lr"], SCAFFOLD_CFG["num_clients"])
        assert gc.same_bits(ef_ref.flat_of(list(s.model.parameters())), ef_ref.flat_of(theta)), r
        assert gc.same_bits(ef_ref.flat_of(s._control_variates), ef_ref.flat_of(cvs)), r
    if compressed.DEFER_ENCODE:  # both vectors of every client in the round's one batch
        assert compressed.deferred_stats() == {"batches": 2, "messages": 40}
    for i, c in enumerate(clients):
        for k in keys:
            assert c.error_memory(k).n == n
            assert gc.same_bits(c.error_memory(k).value().cpu().numpy(), e[i][k]), (i, k)
        assert c.error_memory("parameters_delta") is not c.error_memory("control_variates_delta")
        assert c.error_memory("delta_parameters") is None


def test_gradient_mixin_keeps_one_memory_and_a_skipping_client_touches_none():
    """CompressedGradientsClientMixin with ``error_feedback``: the ``gradients`` of the message go through the memory
    ``"gradients"``; a client that skips its round appends nothing and touches no memory."""
    from fl_sim_amd.compressed import CompressedDelta, CompressedGradientsClientMixin

    shapes = SMALL_SHAPES
    n, K = _n(shapes), _n(shapes) // 100
    g = torch.Generator().manual_seed(46)

    class Base:
        def communicate(self, target):
            if self.skip:
                return
            target._received_messages.append({"client_id": 0, "parameters": self.params, "gradients": self.grads})

    class Client(CompressedGradientsClientMixin, Base):
        pass

    c = Client()
    c.config = types.SimpleNamespace(error_feedback=True,
                                     gradient_compressors=make_compressors("stacked10", n, rng="philox", seed=61))
    s = types.SimpleNamespace(_received_messages=[])
    c.params = [torch.randn(sh, generator=g).cuda() for sh in shapes]
    e = np.zeros(n, dtype=np.float32)
    sent = 0
    for r, skip in enumerate((False, True, False)):
        grads = [torch.randn(sh, generator=g) * 1e-2 for sh in shapes]
        c.grads, c.skip = _cuda(grads), skip
        before = None if c.error_memory("gradients") is None else c.error_memory("gradients").value().clone()
        c.communicate(s)
        if skip:
            assert len(s._received_messages) == sent
            assert torch.equal(c.error_memory("gradients").value().view(torch.int32), before.view(torch.int32))
            continue
        d = s._received_messages[-1]["gradients"]
        assert isinstance(d, CompressedDelta) and d.kind == "stacked"
        x = torch.cat([t.reshape(-1) for t in grads]).numpy()
        out, e, *_ = ef_ref.philox_round(e, x, K, LEVELS, 61, sent)
        assert gc.same_bits(d.flat().cpu().numpy(), out), r
        sent += 1
    assert gc.same_bits(c.error_memory("gradients").value().cpu().numpy(), e)


def test_feedback_off_is_the_untouched_path():
    """``feedback=None`` / ``error_feedback`` absent or false: round_codec.npz's stacked round (the reference's own)
    unchanged, and no memory is made."""
    shapes, codec, opt, tag = SMALL_SHAPES, "stacked10", "avg", "small"
    rec = _fields(f"round_{codec}_{opt}_{tag}")
    s, clients = build_round(shapes, opt, "cuda")
    n = _n(shapes)
    gc.seed_all(round_seed(codec, opt, tag))
    for i, c in enumerate(clients):
        c.compressors = make_compressors(codec, n)
        if i % 2:
            c.error_feedback = False
        c.communicate(s)
        assert c.error_memory("delta_parameters") is None
    assert random.random() == float(rec["next_random"])
    s.update()
    assert _round_same(rec, "delta", s.delta_parameters)
    assert _round_same(rec, "theta", list(s.model.parameters()))
