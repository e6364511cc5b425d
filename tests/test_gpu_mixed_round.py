"""The call site of the mixed fold (FLC_MIXED_FOLD / compressed.MIXED_FOLD): rounds of 10 clients that each chose a
codec of their own — two stacked K, three dithering widths, the natural compressor, two top-k K as sparse records, and
one client that sends its decoded vector — through every server that folds records.  The same round runs with the
switch off (each message decodes itself: the behaviour without the feature) and on (one pass over the messages as they
are); the server's state must agree bit for bit."""

import types

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests import test_gpu_delta_codec as tdc
from tests import test_gpu_vr_codec as tvr
from tests.golden.gen_golden import SMALL_SHAPES, vr_inputs
from tests.golden.gen_golden_delta_codec import ifca_codec_inputs, scaffold_codec_inputs
from tests.test_gpu_round import build_round, make_compressors

pytestmark = pytest.mark.gpu

D = sum(int(np.prod(sh)) for sh in SMALL_SHAPES)
# client i's codec; "flat": std8inf with wire_records off (the message is the decoded vector)
CODECS = ("stacked10", "stacked20", "std8inf", "std4p2", "natd7", "natural", "topk", "topk40", "flat", "stacked10")
CONTROL = ("natural", "stacked10", "flat", "topk40", "std4p2", "stacked20", "std8inf", "natd7", "topk", "topk")
RECORD_KINDS = ("stacked", "sparse", "quant", "natural")


def _compressors(name, seed):
    from fl_sim_amd import Compressor

    def std(L):
        c = Compressor(rng="philox", seed=seed + 1, extended_levels=True)  # (levels above 10)
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(L, nc, np.inf)
        return c

    def topk(k):
        c = Compressor(rng="philox", seed=seed)
        c.makeTopKCompressor(k, D)
        return c

    if name == "stacked20":
        return [topk(D // 20), std(127)]
    if name == "topk40":
        return [topk(D // 40)]
    if name == "natd7":
        c = Compressor(rng="philox", seed=seed)
        c.makeNaturalDitheringFP32(7, D)
        return [c]
    return make_compressors("std8inf" if name == "flat" else name, D, rng="philox", seed=seed)


def _equip(node, name, seed, attr="compressors", on_config=False):
    setattr(node.config if on_config else node, attr, _compressors(name, seed))


def _flags(c, names):
    """wire_records / sparse_records on, unless one of the client's vectors is sent decoded (the switches are per
    client: such a client sends every vector decoded)."""
    c.wire_records = c.sparse_records = "flat" not in names


@pytest.fixture(autouse=True)
def _no_leftovers():
    from fl_sim_amd import compressed

    compressed._run_pending()
    yield
    compressed._run_pending()


def _bits(ts):
    return torch.cat([t.detach().reshape(-1).cpu() for t in ts]).numpy()


def _assert_same(a, b, what=""):
    assert gc.same_bits(_bits(a), _bits(b)), what


def _records_of(msgs, keys):
    return [m[k] for m in msgs for k in keys if m[k].kind in RECORD_KINDS]


def _check_switch(on, msgs, keys, before, after, folds=1):
    """On: the stats advanced and no record message decoded itself; off: the stats stand and every one did."""
    recs = _records_of(msgs, keys)
    assert len(recs) >= 8 * len(keys)
    if on:
        assert after["folds"] == before["folds"] + folds
        assert after["messages"] == before["messages"] + len(msgs) * len(keys)
        assert all(d._flat is None for d in recs)
    else:
        assert after == before
        assert all(d._flat is not None for d in recs)


# --------------------------------------------------------------------------------------------------------- FedOpt
def _fedopt_round(monkeypatch, on, opt, codecs=CODECS, spoil=False, check=True):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", on)
    s, clients = build_round(SMALL_SHAPES, opt, "cuda")
    if spoil:  # a server tensor the launch does not take: δ[4] as a transposed view
        t = s.delta_parameters[4]
        s.delta_parameters[4] = t.t().contiguous().t()
        assert not s.delta_parameters[4].is_contiguous() and torch.equal(s.delta_parameters[4], t)
    for i, c in enumerate(clients):
        c.config = types.SimpleNamespace()
        _equip(c, codecs[i], 100 + 10 * i)
        _flags(c, [codecs[i]])
        c.communicate(s)
    msgs = s._received_messages
    kinds = [m["delta_parameters"].kind for m in msgs]
    before = compressed.mixed_fold_stats()
    s.update()
    after = compressed.mixed_fold_stats()
    torch.cuda.synchronize()
    state = [list(s.model.parameters()), s.delta_parameters] + ([s.v_parameters] if s.v_parameters is not None else [])
    return state, msgs, kinds, before, after


@pytest.mark.parametrize("opt", ["avg", "adam"])
def test_fedopt_round_of_ten_codecs(monkeypatch, opt):
    from fl_sim_amd import compressed

    off, msgs_off, kinds, b0, a0 = _fedopt_round(monkeypatch, False, opt)
    assert kinds == ["stacked", "stacked", "quant", "quant", "quant", "natural", "sparse", "sparse", "dense", "stacked"]
    assert compressed.record_round(msgs_off) is None
    _check_switch(False, msgs_off, ["delta_parameters"], b0, a0)
    on, msgs_on, kinds_on, b1, a1 = _fedopt_round(monkeypatch, True, opt)
    assert kinds_on == kinds and compressed.mixed_round(msgs_on) is not None
    _check_switch(True, msgs_on, ["delta_parameters"], b1, a1)
    for x, y, what in zip(off, on, ("theta", "delta", "v")):
        _assert_same(x, y, what)


def test_uniform_round_takes_the_uniform_fold(monkeypatch):
    from fl_sim_amd import compressed

    for codec in ("stacked10", "std8inf", "topk"):
        off, _, _, _, _ = _fedopt_round(monkeypatch, False, "adam", [codec] * 10)
        on, msgs, kinds, before, after = _fedopt_round(monkeypatch, True, "adam", [codec] * 10)
        assert len(set(kinds)) == 1 and kinds[0] in RECORD_KINDS
        assert after == before  # (the mixed fold was not consulted)
        assert all(m["delta_parameters"]._flat is None for m in msgs)  # (the uniform record fold ran)
        for x, y in zip(off, on):
            _assert_same(x, y, codec)


def test_server_the_launch_does_not_take_falls_back(monkeypatch):
    off, _, _, _, _ = _fedopt_round(monkeypatch, False, "adam", spoil=True)
    on, msgs, _, before, after = _fedopt_round(monkeypatch, True, "adam", spoil=True)
    assert after == before  # (nothing folded by the mixed pass)
    assert all(m["delta_parameters"]._flat is not None for m in msgs)  # (each message decoded itself)
    for x, y, what in zip(off, on, ("theta", "delta", "v")):
        _assert_same(x, y, what)
    plain, _, _, _, _ = _fedopt_round(monkeypatch, False, "adam")
    for x, y, what in zip(plain, on, ("theta", "delta", "v")):
        _assert_same(x, y, what)  # (and the same values as the contiguous server's)


def test_deferred_batches_of_two_k_are_encoded_by_the_folds_first_read(monkeypatch):
    from fl_sim_amd import compressed

    assert compressed.DEFER_ENCODE
    monkeypatch.setattr(compressed, "MIXED_FOLD", True)
    s, clients = build_round(SMALL_SHAPES, "avg", "cuda")
    codecs = ("stacked10", "stacked20") * 5
    for i, c in enumerate(clients):
        c.config = types.SimpleNamespace()
        _equip(c, codecs[i], 100 + 10 * i)
        c.communicate(s)
    ds = [m["delta_parameters"] for m in s._received_messages]
    assert {d.k for d in ds} == {D // 100, D // 20}
    assert all(d._batch is not None and d._record is None for d in ds)  # (two batches wait, nothing encoded)
    assert len({id(d._batch) for d in ds}) == 2
    enc0, mix0 = compressed.deferred_stats(), compressed.mixed_fold_stats()
    s.update()
    enc1, mix1 = compressed.deferred_stats(), compressed.mixed_fold_stats()
    assert enc1["batches"] == enc0["batches"] + 2 and enc1["messages"] == enc0["messages"] + 10
    assert mix1["folds"] == mix0["folds"] + 1 and mix1["messages"] == mix0["messages"] + 10
    assert all(d._record is not None and d._flat is None for d in ds)
    on = [list(s.model.parameters()), s.delta_parameters]
    monkeypatch.setattr(compressed, "MIXED_FOLD", False)
    s2, clients2 = build_round(SMALL_SHAPES, "avg", "cuda")
    for i, c in enumerate(clients2):
        c.config = types.SimpleNamespace()
        _equip(c, codecs[i], 100 + 10 * i)
        c.communicate(s2)
    s2.update()
    for x, y in zip(on, [list(s2.model.parameters()), s2.delta_parameters]):
        _assert_same(x, y)


# ------------------------------------------------------------------------------------------------------- SCAFFOLD
def _scaffold_round(monkeypatch, on):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", on)
    theta, cvs, clients = scaffold_codec_inputs(SMALL_SHAPES)
    s = tdc._scaffold_server(theta, cvs, "device")
    for i, src in enumerate(clients):
        c = tdc._scaffold_client(src)
        _equip(c, CODECS[i], 300 + 10 * i)
        _equip(c, CONTROL[i], 700 + 10 * i, "control_compressors", on_config=True)
        _flags(c, [CODECS[i], CONTROL[i]])
        c.communicate(s)
    msgs = s._received_messages
    before = compressed.mixed_fold_stats()
    s.update()
    after = compressed.mixed_fold_stats()
    torch.cuda.synchronize()
    return [list(s.model.parameters()), s._control_variates], msgs, before, after


def test_scaffold_round_with_compressors_differing_per_client_and_per_vector(monkeypatch):
    from fl_sim_amd import compressed

    off, msgs_off, b0, a0 = _scaffold_round(monkeypatch, False)
    for key in tdc.KEYS:
        assert compressed.record_round(msgs_off, key) is None
        assert len({m[key].codec_key for m in msgs_off}) >= 6
    assert a0 == b0 and all(m[k]._flat is not None for m in msgs_off for k in tdc.KEYS)
    on, msgs_on, b1, a1 = _scaffold_round(monkeypatch, True)
    assert a1["folds"] == b1["folds"] + 1  # (θ's and c's messages in one launch)
    assert a1["messages"] == b1["messages"] + 20
    recs = _records_of(msgs_on, tdc.KEYS)
    assert len(recs) >= 12 and all(d._flat is None for d in recs)
    _assert_same(off[0], on[0], "theta")
    _assert_same(off[1], on[1], "control variates")


def test_scaffold_groups_of_two_uniform_codecs_fold_in_one_launch(monkeypatch):
    """θ's messages all stacked, c's all 8-bit: one launch per codec without the switch, one launch with it."""
    from fl_sim_amd import compressed

    def run(on):
        monkeypatch.setattr(compressed, "MIXED_FOLD", on)
        theta, cvs, clients = scaffold_codec_inputs(SMALL_SHAPES)
        s = tdc._scaffold_server(theta, cvs, "device")
        for i, src in enumerate(clients):
            c = tdc._scaffold_client(src)
            _equip(c, "stacked10", 300 + 10 * i)
            _equip(c, "std8inf", 700 + 10 * i, "control_compressors", on_config=True)
            _flags(c, [])
            c.communicate(s)
        before = compressed.mixed_fold_stats()
        s.update()
        after = compressed.mixed_fold_stats()
        assert all(m[k]._flat is None for m in s._received_messages for k in tdc.KEYS)  # (records folded either way)
        return [list(s.model.parameters()), s._control_variates], after["folds"] - before["folds"]

    off, f0 = run(False)
    on, f1 = run(True)
    assert (f0, f1) == (0, 1)
    _assert_same(off[0], on[0], "theta")
    _assert_same(off[1], on[1], "control variates")


# ----------------------------------------------------------------------------------------------------------- IFCA
def _ifca_round(monkeypatch, on):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", on)
    centers, clients = ifca_codec_inputs(SMALL_SHAPES)
    s = tdc._ifca_server(centers, "device")
    for i, src in enumerate(clients):
        c = tdc._ifca_client(src)
        _equip(c, CODECS[i], 500 + 10 * i)
        _flags(c, [CODECS[i]])
        c.communicate(s)
    msgs = s._received_messages
    before = compressed.mixed_fold_stats()
    s.update()
    after = compressed.mixed_fold_stats()
    torch.cuda.synchronize()
    return s._cluster_centers, msgs, before, after


def test_ifca_round_of_ten_codecs(monkeypatch):
    off, msgs_off, b0, a0 = _ifca_round(monkeypatch, False)
    _check_switch(False, msgs_off, ["delta_parameters"], b0, a0)
    on, msgs_on, b1, a1 = _ifca_round(monkeypatch, True)
    _check_switch(True, msgs_on, ["delta_parameters"], b1, a1)
    assert sorted(off) == sorted(on)
    for c in off:
        _assert_same(off[c]["center_model_params"], on[c]["center_model_params"], f"centre {c}")
        assert off[c]["client_ids"] == on[c]["client_ids"]


# ------------------------------------------------------------------------------------- the variance-reduced servers
def _vr_messages(monkeypatch, on):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", on)
    params, srcs = vr_inputs(SMALL_SHAPES, 10)
    s = tvr._server("fedprox", params, "device")
    for i, src in enumerate(srcs):
        c = tvr._client(src)
        _equip(c, CODECS[i], 900 + 10 * i, "gradient_compressors")
        _flags(c, [CODECS[i]])
        c.communicate(s)
    return s


def test_update_gradients_of_ten_codecs(monkeypatch):
    from fl_sim_amd import aggregation, compressed

    out = {}
    for on in (False, True):
        s = _vr_messages(monkeypatch, on)
        mps = list(s.model.parameters())
        theta0 = [p.detach().clone() for p in mps]
        before = compressed.mixed_fold_stats()
        grads = aggregation.update_gradients(mps, s._received_messages)
        after = compressed.mixed_fold_stats()
        torch.cuda.synchronize()
        _check_switch(on, s._received_messages, ["gradients"], before, after)
        assert all(p.grad.data_ptr() == g.data_ptr() for p, g in zip(mps, grads))
        _assert_same(mps, theta0, "the parameters are untouched")
        out[on] = grads
    _assert_same(out[False], out[True], "gradients")


def test_vr_server_round_of_ten_codecs(monkeypatch):
    from fl_sim_amd import compressed

    out = {}
    for on in (False, True):
        s = _vr_messages(monkeypatch, on)
        before = compressed.mixed_fold_stats()
        s.update()
        after = compressed.mixed_fold_stats()
        torch.cuda.synchronize()
        _check_switch(on, s._received_messages, ["gradients"], before, after)
        out[on] = [list(s.model.parameters()), [p.grad for p in s.model.parameters()]]
    _assert_same(out[False][0], out[True][0], "theta")
    _assert_same(out[False][1], out[True][1], "gradients")
