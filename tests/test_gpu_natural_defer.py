"""Deferred natural-compressor records (``compressed.NATURAL_DEFER``, off by default): with the switch on, a natural
compressor's ``wire`` message waits for the round's one flc_natural_encode_round — with error feedback, for one
flc_natural_encode_residual_round, which also leaves every memory holding ``a − decode(record)``.  Switch on against
switch off (the per-message encode; with feedback the chain encode, dense decode, dense residual) agree bit for bit —
records, memories, send statistics, Philox counters, the server's update — and the feedback round, composed from the
CPU oracle's natural compressor as tests/ef_ref.py composes the stacked pipeline, agrees with the oracle; everything
else stays on the immediate path."""

import numpy as np
import pytest
import torch

from tests import ef_ref
from tests import golden_cases as gc
from tests import test_gpu_delta_codec as tdc
from tests.golden.gen_golden import SMALL_SHAPES, round_inputs
from tests.golden.gen_golden_delta_codec import scaffold_codec_inputs
from tests.golden.gen_golden_ef import flat_delta
from tests.test_gpu_round import build_round, make_compressors

pytestmark = pytest.mark.gpu
CLIENTS, ROUNDS = 4, 3
SAMPLED = [(0, 1, 2, 3), (0, 2), (0, 1, 2, 3)]  # (round 2 samples two clients: the round-3 counters differ)
D = sum(int(np.prod(sh)) for sh in SMALL_SHAPES)


def _comps(seed, rng="philox"):
    return make_compressors("natural", D, rng=rng, seed=seed)


def _stat(c):
    return (c.total_input_components, c.last_input_advance, c.really_need_to_send_components,
            c.last_need_to_send_advance, c.philox.counter)


def _codes(d):
    """The code bytes of a natural record (its norm field and padding are not part of the message)."""
    from fl_sim_amd import codec

    assert d.kind == "natural" and d.format is not None and d.bits == 16 and d.levels == 0
    return codec.dense_wire_views(d.record, d.n, d.format, d.bits)[1].cpu().numpy()


def _same_records(a, b):
    assert (a.kind, a.codec_key, a.nbytes, [tuple(s) for s in a.shapes]) == \
           (b.kind, b.codec_key, b.nbytes, [tuple(s) for s in b.shapes])
    return np.array_equal(_codes(a), _codes(b))


def _flat(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts]).numpy()


def _mem_bits(mem):
    return mem.value().cpu().numpy().view(np.uint32).copy()


@pytest.fixture(autouse=True)
def _clean(monkeypatch):
    from fl_sim_amd import compressed

    compressed._run_pending()  # (messages earlier tests left waiting)
    monkeypatch.setattr(compressed, "DEFER_ENCODE", True)
    monkeypatch.setattr(compressed, "NATURAL_DEFER", False)
    yield
    compressed._run_pending()


def _legs(run):
    """``run(on)`` with the switch off, then on; (immediate result, deferred result)."""
    from fl_sim_amd import compressed

    out = []
    for on in (False, True):
        compressed.NATURAL_DEFER = on
        out.append(run(on))
    compressed.NATURAL_DEFER = False
    return out


# --------------------------------------------------------------------------------- 1. switch on == switch off == oracle
def _fedopt_rounds(opt, fb, on):
    """Four clients over three rounds through the FedOpt mixins (two of them sampled in round 2); per round the
    messages' code bytes and the server's θ and δ, then the memories and the compressors' statistics.  Also the flat
    inputs and the records' decoded vectors, for the oracle."""
    from fl_sim_amd import codec as flc, compressed

    s, clients = build_round(SMALL_SHAPES, opt, "cuda", n_clients=CLIENTS)
    theta, _, _, locals_, _ = round_inputs(SMALL_SHAPES, opt, CLIENTS)
    g = torch.Generator().manual_seed(91)
    for i, c in enumerate(clients):
        c.compressors, c.wire_records, c.error_feedback = _comps(40 + i), True, fb
    recs, decs, servers, xs = [], [], [], []
    for r in range(ROUNDS):
        before = compressed.deferred_dense_stats()
        for i in SAMPLED[r]:
            if r:  # (the model moves on; the cached parameters stay)
                locals_[i] = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in locals_[i]]
                for p, t in zip(clients[i].model.parameters(), locals_[i]):
                    p.data.copy_(t)
            clients[i].communicate(s)
        msgs = list(s._received_messages)
        ds = [m["delta_parameters"] for m in msgs]
        assert all((d._batch is not None) == on and (d._record is None) == on for d in ds)
        assert compressed.deferred_dense_stats() == before  # (nothing encoded in a batch yet)
        if on:
            assert len({id(d._batch) for d in ds}) == 1
            assert ds[0]._batch.key[1:] == ("natural", D, fb)
            if fb:
                assert all(clients[i].error_memory("delta_parameters")._batch is ds[0]._batch for i in SAMPLED[r])
        recs.append([_codes(d) for d in ds])  # the first read runs the round's batch
        after = compressed.deferred_dense_stats()
        assert after["batches"] - before["batches"] == (1 if on else 0)
        assert after["messages"] - before["messages"] == (len(ds) if on else 0)
        assert all(d._batch is None for d in ds)
        decs.append([flc.dense_record_decode(d.record, d.n, d.format, d.levels, d.bits).cpu().numpy() for d in ds])
        xs.append([flat_delta(locals_[i], theta) for i in SAMPLED[r]])
        s.update()
        assert all(d._flat is None for d in ds)  # (the record fold took the round)
        servers.append(_flat(list(s.model.parameters()) + s.delta_parameters))
        s._received_messages = []
    mems = [_mem_bits(c.error_memory("delta_parameters")) for c in clients] if fb else []
    return recs, servers, mems, [_stat(c.compressors[0]) for c in clients], xs, decs


def _oracle(a, seed, ctr):
    """The oracle's natural compressor on ``a`` with the message's Philox (seed, counter): the decoded vector."""
    from oracle import compressors_ref as ref

    u = ref.philox_uniforms(a.shape[0], seed, ctr)
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(ref.natural(a, lambda i: u[i])[0], dtype=np.float32)


@pytest.mark.parametrize("opt", ["avg", "adam"])
@pytest.mark.parametrize("fb", [False, True], ids=["plain", "feedback"])
def test_fedopt_rounds_on_equal_off_and_the_oracle(fb, opt):
    (ra, ta, ea, sa, xs, _), (rb, tb, eb, sb, _, decs) = _legs(lambda on: _fedopt_rounds(opt, fb, on))
    assert sa == sb
    assert len({st[-1] for st in sa}) == 2  # (Philox counters 3 and 2: the clients advanced differently)
    assert all(st[2] == pytest.approx(st[-1] * 9.0 / 32.0 * D, rel=1e-12) for st in sb)  # (compressors.py:325)
    for r in range(ROUNDS):
        assert gc.same_bits(ta[r], tb[r]), r
        for ca, cb in zip(ra[r], rb[r]):
            assert np.array_equal(ca, cb), r
    assert len(ea) == len(eb) == (CLIENTS if fb else 0)
    for i in range(len(ea)):
        assert np.array_equal(ea[i], eb[i]), i
    if opt != "avg":  # (the oracle's loop does not depend on the server's optimiser: once per form)
        return
    e = [np.zeros(D, dtype=np.float32) for _ in range(CLIENTS)]
    ctr = [0] * CLIENTS
    for r in range(ROUNDS):
        for j, i in enumerate(SAMPLED[r]):
            a = ef_ref.accumulate(e[i], xs[r][j]) if fb else np.ascontiguousarray(xs[r][j], dtype=np.float32)
            c = _oracle(a, 40 + i, ctr[i])
            assert gc.same_bits(decs[r][j], c), (r, i)
            if fb:
                e[i] = a - c
            ctr[i] += 1
    if fb:
        for i in range(CLIENTS):
            assert np.array_equal(eb[i], e[i].view(np.uint32)), i
        assert any(np.any(x) for x in e)


@pytest.mark.parametrize("fb", [False, True], ids=["plain", "feedback"])
def test_scaffold_two_deltas_land_in_one_batch(fb):
    from fl_sim_amd import compressed

    theta, cvs, srcs = scaffold_codec_inputs(SMALL_SHAPES)

    def run(on):
        s = tdc._scaffold_server(theta, cvs, "device")
        clients = []
        for i, src in enumerate(srcs):
            c = tdc._scaffold_client(src)
            c.compressors, c.config.control_compressors = _comps(100 + i), _comps(200 + i)
            c.wire_records, c.error_feedback = True, fb
            clients.append(c)
        before = compressed.deferred_dense_stats()
        for c in clients:
            c.communicate(s)
        msgs = list(s._received_messages)
        assert all((m[k]._batch is not None) == on for m in msgs for k in tdc.KEYS)
        if on:
            assert len({id(m[k]._batch) for m in msgs for k in tdc.KEYS}) == 1  # (one batch for both vectors)
        s.update()
        after = compressed.deferred_dense_stats()
        assert after["batches"] - before["batches"] == (1 if on else 0)
        assert after["messages"] - before["messages"] == (2 * len(clients) if on else 0)
        mems = []
        if fb:
            for c in clients:
                assert c.error_memory(tdc.KEYS[0]) is not c.error_memory(tdc.KEYS[1])
            mems = [_mem_bits(c.error_memory(k)) for c in clients for k in tdc.KEYS]
        stats = [(_stat(c.compressors[0]), _stat(c.config.control_compressors[0])) for c in clients]
        assert all(a[-1] == 1 and b[-1] == 1 for a, b in stats)  # (each compressor its own counter, advanced once)
        return msgs, stats, _flat(list(s.model.parameters()) + s._control_variates), mems

    (ma, sa, ta, ea), (mb, sb, tb, eb) = _legs(run)
    assert sa == sb and gc.same_bits(ta, tb)
    assert all(_same_records(x[k], y[k]) for x, y in zip(ma, mb) for k in tdc.KEYS)
    assert len(ea) == len(eb) and all(np.array_equal(x, y) for x, y in zip(ea, eb))
    assert not fb or any(x.any() for x in eb)


# ------------------------------------------------------------------------------------------ 2. the memory's own rules
def _one_client(seed=77, rng="philox"):
    from fl_sim_amd.feedback import ErrorMemory

    theta, _, _, locals_, _ = round_inputs(SMALL_SHAPES, "avg", 3)
    return ([t.cuda() for t in theta], [[t.cuda() for t in loc] for loc in locals_], _comps(seed, rng),
            ErrorMemory(D, "cuda"))


def test_a_raised_encode_leaves_the_memories_for_the_retry(monkeypatch):
    """The batched call raises once: the batch stays pending and the memory still holds a; the retry encodes the same
    a and applies the residual exactly once."""
    from fl_sim_amd import codec, compressed
    from fl_sim_amd.compressed import compress_delta

    glob, locs, comps, mem = _one_client()
    off_mem = _one_client()[3]
    want = compress_delta(locs[0], glob, _comps(77), off_mem, wire=True)  # (switch off: immediate)
    assert want._batch is None
    real, calls = codec.natural_encode_residual_round, []

    def failing(*a, **k):
        calls.append(1)
        if len(calls) == 1:
            raise RuntimeError("injected")
        return real(*a, **k)

    monkeypatch.setattr(codec, "natural_encode_residual_round", failing)
    compressed.NATURAL_DEFER = True
    d = compress_delta(locs[0], glob, comps, mem, wire=True)
    x = flat_delta([t.cpu() for t in locs[0]], [t.cpu() for t in glob])
    with pytest.raises(RuntimeError, match="injected"):
        d.record
    assert d._batch is not None and mem._batch is d._batch
    assert gc.same_bits(mem._e.cpu().numpy(), x)  # (a = 0 + x, untouched)
    assert _same_records(d, want) and len(calls) == 2
    assert np.array_equal(_mem_bits(mem), _mem_bits(off_mem)) and _mem_bits(mem).any()
    assert _stat(comps[0])[-1] == 1  # (the retry drew no further Philox counter)


def test_nothing_decodes_on_the_deferred_path(monkeypatch):
    """With the dense decode made to raise, a deferred feedback round still completes; the immediate chain needs it."""
    from fl_sim_amd import codec, compressed

    def boom(*a, **k):
        raise AssertionError("a dense record was decoded")

    monkeypatch.setattr(codec, "dense_record_decode", boom)

    def round_(on):
        compressed.NATURAL_DEFER = on
        s, clients = build_round(SMALL_SHAPES, "avg", "cuda", n_clients=CLIENTS)
        for i, c in enumerate(clients):
            c.compressors, c.wire_records, c.error_feedback = _comps(40 + i), True, True
            c.communicate(s)
        s.update()
        return [_mem_bits(c.error_memory("delta_parameters")) for c in clients]

    assert all(e.any() for e in round_(True))
    with pytest.raises(AssertionError, match="decoded"):
        round_(False)


def test_value_runs_the_memory_s_batch_and_no_other():
    from fl_sim_amd.compressed import compress_delta

    def run(on):
        glob, locs, comps, mem = _one_client()
        d = compress_delta(locs[0], glob, comps, mem, wire=True)
        other = compress_delta(locs[1], glob, _comps(78), None, wire=True)  # (a plain message: its own batch)
        assert (d._batch is not None) == on and (other._batch is not None) == on
        assert not on or other._batch is not d._batch  # (a feedback batch never mixes with a plain one)
        v = mem.value()
        assert d._batch is None and d._record is not None and mem._batch is None
        assert (other._batch is not None) == on  # (the memory's batch ran, no other)
        return d, other, v.cpu().numpy().view(np.uint32).copy(), _stat(comps[0])

    (a, oa, ea, sa), (b, ob, eb, sb) = _legs(run)
    assert _same_records(a, b) and _same_records(oa, ob) and np.array_equal(ea, eb) and eb.any() and sa == sb


# ------------------------------------------------------------------------------------------- 3. the immediate path
def test_the_switch_off_encodes_at_once():
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_delta

    assert compressed.NATURAL_DEFER is False  # (the fixture's value, which is the default's)
    assert compressed._DEFER_NATURAL_MAX_N <= compressed._DEFER_MAX_N
    assert compressed._DEFER_EF_NATURAL_MAX_N <= compressed._DEFER_MAX_N
    glob, locs, comps, mem = _one_client()
    before = compressed.deferred_dense_stats()
    for m in (None, mem):
        d = compress_delta(locs[0], glob, comps, m, wire=True)
        assert d._batch is None and d._record is not None and mem._batch is None and not compressed._PENDING
    assert compressed.deferred_dense_stats() == before


# (float64: a float64 model's feedback message — its plain message is deferred like any float32 flat vector, as the
# dithering quantizers' is)
@pytest.mark.parametrize("case,fb", [("defer_encode_off", False), ("defer_encode_off", True), ("compat", False),
                                     ("compat", True), ("float64", True)])
def test_these_messages_stay_immediate(case, fb, monkeypatch):
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_delta

    if case == "defer_encode_off":
        monkeypatch.setattr(compressed, "DEFER_ENCODE", False)

    def run(on):
        gc.seed_all(6)
        glob, locs, comps, mem = _one_client(2, "compat" if case == "compat" else "philox")
        if case == "float64":
            glob, locs = [t.double() for t in glob], [[t.double() for t in loc] for loc in locs]
        ds = []
        for r in range(2):
            d = compress_delta(locs[r], glob, comps, mem if fb else None, wire=True)
            assert d._batch is None and d._record is not None and mem._batch is None and not compressed._PENDING
            ds.append(d)
        return ds, _stat(comps[0]), _mem_bits(mem)

    before = compressed.deferred_dense_stats()
    (a, sa, ea), (b, sb, eb) = _legs(run)
    assert all(_same_records(x, y) for x, y in zip(a, b)) and sa == sb and np.array_equal(ea, eb)
    assert compressed.deferred_dense_stats() == before  # (no batched encode ran)


@pytest.mark.parametrize("fb", [False, True], ids=["plain", "feedback"])
def test_a_message_past_the_size_bound_stays_immediate(fb, monkeypatch):
    from fl_sim_amd import compressed
    from fl_sim_amd.compressed import compress_tensors
    from fl_sim_amd.feedback import ErrorMemory

    monkeypatch.setattr(compressed, "_DEFER_EF_NATURAL_MAX_N" if fb else "_DEFER_NATURAL_MAX_N", 5000)

    def run(on):
        g = torch.Generator(device="cuda").manual_seed(8)
        out = []
        for m in (5000, 5001):
            comps, mem = make_compressors("natural", m, rng="philox", seed=3), ErrorMemory(m, "cuda")
            d = compress_tensors([torch.randn(m, generator=g, device="cuda")], comps, mem if fb else None, wire=True)
            assert (d._batch is not None) == (on and m == 5000)
            out.append((d, _mem_bits(mem), _stat(comps[0])))
        return out

    a, b = _legs(run)
    for (da, ea, sa), (db, eb, sb) in zip(a, b):
        assert _same_records(da, db) and np.array_equal(ea, eb) and sa == sb
