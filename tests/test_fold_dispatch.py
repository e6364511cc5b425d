"""The record folds' dispatch: which entry a round's records reach (the ``_flcfold`` one-call entries behind the
``codec._PY*`` cells, the C ABI through ``_lib.call``) and with exactly which arguments.  The entries are replaced by
recorders, so nothing is launched: the results are the other files' business, the routing is this one's."""

import ctypes

import pytest
import torch

SHAPES = [torch.Size((3, 2)), torch.Size((4,))]
N = 10
KINDS = ("stacked", "sparse", "quant", "natural")
# per kind: what follows n in the entries' shape arguments, the FedOpt / gradient / grouped cells, the C names' infix
SHAPE = {"stacked": (N, 2, 10), "sparse": (N, 3), "quant": (N, 0, 127, 8), "natural": (N, 2, 0, 16)}
CELL = {"stacked": ("_PYRECS", "_PYGRECS"), "sparse": ("_PYSRECS", "_PYGSRECS"), "quant": ("_PYDRECS", "_PYGDRECS"),
        "natural": ("_PYDRECS", "_PYGDRECS")}
INFIX = {"stacked": "", "sparse": "sparse_", "quant": "dense_", "natural": "dense_"}
CELLS = ("_PYRECS", "_PYDRECS", "_PYSRECS", "_PYMRECS", "_PYGROUPS", "_PYGRECS", "_PYGDRECS", "_PYGSRECS")
REC = {"stacked": 0, "sparse": 1, "quant": 2, "natural": 2, "flat": 3}  # flc_record_kind
OPT = {"avg": 0, "adagrad": 1, "yogi": 2, "adam": 3}


def _deltas(dev="cpu"):
    """tests/test_capi_mixed_fold.py's 10-element model: records of zero bytes, never read here."""
    from fl_sim_amd import compressed

    CD = compressed.CompressedDelta
    d = torch.device(dev)
    rec = lambda **kw: CD(SHAPES, d, kw.pop("n", N), record=torch.zeros(256, dtype=torch.uint8, device=d),  # noqa: E731
                          **kw)
    return dict(
        stacked=lambda **kw: rec(**{"k": 2, "levels": 10, **kw}),
        sparse=lambda **kw: rec(**{"k": 3, "sparse": True, **kw}),
        quant=lambda **kw: rec(**{"format": 0, "levels": 127, "bits": 8, **kw}),
        natural=lambda **kw: rec(format=2, bits=16, **kw),
        flat=lambda dtype=torch.float32, n=N: CD(SHAPES, d, n, flat=torch.zeros(n, dtype=dtype, device=d)),
    )


def _msgs(ds, key="delta_parameters"):
    return [{key: d, "train_samples": i + 1} for i, d in enumerate(ds)]


def _srv(dev="cpu"):
    return [torch.zeros(s, device=dev) for s in SHAPES]


class Recorder:
    def __init__(self, result=None, raises=None):
        self.calls, self.result, self.raises = [], result, raises

    def __call__(self, *args):
        self.calls.append(args)
        if self.raises is not None:
            raise self.raises
        return self.result


def _record_cells(monkeypatch, **kw):
    """Every record-fold cell replaced by a recorder of its own; {cell name: recorder}."""
    from fl_sim_amd import codec

    out = {}
    for name in CELLS:
        out[name] = Recorder(**kw)
        monkeypatch.setattr(codec, name, [out[name]])
    return out


def _only(recorders, name):
    assert [k for k, r in recorders.items() if r.calls] == [name]
    assert len(recorders[name].calls) == 1
    return recorders[name].calls[0]


def _same(got, want):
    """Two lists of tensors, object by object."""
    return len(got) == len(want) and all(a is b for a, b in zip(got, want))


# ----------------------------------------------------------------------------------------------------- without a GPU
@pytest.mark.parametrize("kind", KINDS)
def test_fold_records_calls_the_kinds_entry(monkeypatch, kind):
    from fl_sim_amd import compressed

    cells = _record_cells(monkeypatch)
    ds = [_deltas()[kind]() for _ in range(3)]
    dp, th, v = _srv(), _srv(), _srv()
    ws = [torch.tensor(0.25).item(), 1, 0.5]
    assert compressed.fold_records(ds, ws, dp, th, v, 0.5, "yogi", 0.1, 0.99, 1e-3) is True
    a = _only(cells, CELL[kind][0])
    assert len(a) == 2 + len(SHAPE[kind]) + 8
    assert _same(a[0], [d.record for d in ds])
    assert a[1] == [0.25, 1.0, 0.5] and all(type(w) is float for w in a[1])
    assert a[2:2 + len(SHAPE[kind])] == SHAPE[kind]
    rest = a[2 + len(SHAPE[kind]):]
    assert _same(rest[0], dp) and _same(rest[1], th) and _same(rest[2], v)
    assert rest[3:] == (0.5, OPT["yogi"], 0.1, 0.99, 1e-3)
    assert type(rest[3]) is float and type(rest[4]) is int

    cells = _record_cells(monkeypatch)  # the defaults, no θ, no v: FedAvg's δ alone
    assert compressed.fold_records(ds, ws, dp, None, None, 0) is True
    a = _only(cells, CELL[kind][0])
    assert a[2 + len(SHAPE[kind]) + 1:] == (None, None, 0.0, OPT["avg"], 1.0, 0.0, 0.0)


@pytest.mark.parametrize("kind", KINDS)
def test_fold_record_groups_calls_the_stacked_entry_only(monkeypatch, kind):
    from fl_sim_amd import compressed

    cells = _record_cells(monkeypatch)
    d = _deltas()
    g0, g1 = [d[kind](), d[kind]()], [d[kind]()]
    dst0, dst1 = _srv(), _srv()
    groups = [(g0, [0.5, 0.5], dst0), ([], [], _srv()), (g1, [1], dst1)]
    got = compressed.fold_record_groups(groups)
    if kind != "stacked":  # (no one-call entry: the ctypes path's checks decline host tensors)
        assert got is False and not any(r.calls for r in cells.values())
        return
    assert got is True
    a = _only(cells, "_PYGROUPS")
    assert len(a) == 6 and a[3:] == SHAPE["stacked"]
    assert len(a[0]) == 2 and _same(a[0][0], [x.record for x in g0]) and _same(a[0][1], [x.record for x in g1])
    assert a[1] == [[0.5, 0.5], [1]]
    assert len(a[2]) == 2 and _same(a[2][0], dst0) and _same(a[2][1], dst1)
    staged = [[torch.zeros(256, dtype=torch.uint8) for _ in g0], None, None]
    cells = _record_cells(monkeypatch)
    assert compressed.fold_record_groups(groups, staged) is True
    a = _only(cells, "_PYGROUPS")
    assert _same(a[0][0], staged[0]) and _same(a[0][1], [x.record for x in g1])


@pytest.mark.parametrize("kind", KINDS)
def test_an_entry_that_declines_leaves_host_tensors_to_the_caller(monkeypatch, kind):
    from fl_sim_amd import compressed

    cells = _record_cells(monkeypatch, raises=TypeError("not a HIP tensor"))
    ds = [_deltas()[kind]() for _ in range(2)]
    assert compressed.fold_records(ds, [0.5, 0.5], _srv(), _srv(), None, 0.0) is False
    _only(cells, CELL[kind][0])
    cells = _record_cells(monkeypatch, raises=TypeError("not a HIP tensor"))
    assert compressed.fold_record_groups([(ds, [0.5, 0.5], _srv())]) is False
    assert [k for k, r in cells.items() if r.calls] == (["_PYGROUPS"] if kind == "stacked" else [])
    assert compressed.fold_gradient_records(ds, [0.5, 0.5], _srv()) is False
    assert compressed.fold_record_groups([]) is True  # (no group with messages: nothing to do)


def _rounds():
    d = _deltas()
    return [
        [d["stacked"](), d["stacked"]()], [d["sparse"](), d["sparse"](), d["sparse"]()], [d["quant"]()],
        [d["natural"](), d["natural"]()], [d["quant"](), d["natural"]()], [d["stacked"](), d["stacked"](k=3)],
        [d["stacked"](), d["stacked"](levels=127)], [d["stacked"](), d["stacked"](n=11)],
        [d["sparse"](), d["sparse"](k=1)], [d["quant"](), d["quant"](levels=7, bits=4)],
        [d["quant"](), d["quant"](format=1)], [d["stacked"](), d["sparse"]()], [d["stacked"](), d["flat"]()],
        [d["flat"](), d["flat"]()], [d["flat"](), d["natural"](), d["flat"]()], [d["sparse"](), d["flat"](n=11)],
        [d["stacked"](), d["flat"](torch.float64)], [],
    ]


@pytest.mark.parametrize("on", (False, True))
def test_the_classifiers_agree_with_codec_key_equality(monkeypatch, on):
    from fl_sim_amd import compressed

    monkeypatch.setattr(compressed, "MIXED_FOLD", on)
    before = compressed.mixed_fold_stats()
    kinds_of = {compressed.stacked_round: ("stacked",), compressed.sparse_round: ("sparse",),
                compressed.dense_record_round: ("quant", "natural"),
                compressed.record_round: ("stacked", "sparse", "quant", "natural")}
    for ds in _rounds():
        for key in ("delta_parameters", "gradients"):
            msgs = _msgs(ds, key)
            one_key = bool(ds) and all(x.codec_key == ds[0].codec_key for x in ds)
            for fn, kinds in kinds_of.items():
                got = fn(msgs, key)
                if one_key and ds[0].kind in kinds:
                    assert got is not None and _same(got, ds)
                else:
                    assert got is None
                assert fn(msgs, "parameters_delta") is None  # (another key)
            flat_ok = all(x.kind != "dense" or x._flat.dtype is torch.float32 for x in ds)
            mixed = (on and bool(ds) and not one_key and all(x.n == ds[0].n for x in ds)
                     and any(x.kind != "dense" for x in ds) and flat_ok)
            got = compressed.mixed_round(msgs, key)
            assert (got is not None and _same(got, ds)) if mixed else got is None
    assert compressed.record_round(_msgs([_deltas()["stacked"]()]) + [{"delta_parameters": [torch.zeros(N)]}]) is None
    assert compressed.mixed_fold_stats() == before  # (recognising a round folds nothing)


# -------------------------------------------------------------------------------------------------------- on the GPU
def _vals(a):
    """A ctypes array as a list (pointers as integers); anything else as it is."""
    return list(a) if isinstance(a, ctypes.Array) else a


def _ptr_list(ts):
    return [t.data_ptr() for t in ts]


@pytest.fixture
def ctypes_calls(monkeypatch):
    """The ctypes path alone: every cell empty (None), ``_lib.call`` a recorder."""
    from fl_sim_amd import _lib, codec

    for name in CELLS:
        monkeypatch.setattr(codec, name, [None])
    rec = Recorder()
    monkeypatch.setattr(_lib, "call", rec)
    return rec


def _stream():
    from fl_sim_amd import codec

    return codec._stream(torch.device("cuda", 0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ctypes_fedopt_fold(ctypes_calls, kind):
    from fl_sim_amd import compressed

    ds = [_deltas("cuda:0")[kind]() for _ in range(3)]
    dp, th, v = _srv("cuda:0"), _srv("cuda:0"), _srv("cuda:0")
    before = compressed.mixed_fold_stats()
    assert compressed.fold_records(ds, [0.25, 1, 0.5], dp, th, v, 0.5, "adam", 0.1, 0.99, 1e-3) is True
    (a,) = ctypes_calls.calls
    s = len(SHAPE[kind])
    assert a[0] == f"flc_fedopt_fold_{INFIX[kind]}records" and len(a) == 4 + s + 11
    assert _vals(a[1]) == _ptr_list([d.record for d in ds]) and _vals(a[2]) == [0.25, 1.0, 0.5] and a[3] == 3
    assert a[4:4 + s] == SHAPE[kind]
    r = a[4 + s:]
    assert [_vals(x) for x in r[:3]] == [_ptr_list(dp), _ptr_list(th), _ptr_list(v)]
    assert _vals(r[3]) == [6, 4] and r[4:] == (2, 0.5, OPT["adam"], 0.1, 0.99, 1e-3, _stream())
    ctypes_calls.calls.clear()
    assert compressed.fold_records(ds, [1, 1, 1], dp, None, None, 0.0) is True
    (a,) = ctypes_calls.calls
    assert a[4 + s + 1:4 + s + 3] == (None, None) and a[4 + s + 5:-1] == (0.0, OPT["avg"], 1.0, 0.0, 0.0)
    assert compressed.mixed_fold_stats() == before


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ctypes_gradient_fold(ctypes_calls, kind):
    from fl_sim_amd import compressed

    ds = [_deltas("cuda:0")[kind]() for _ in range(2)]
    gs, ps = _srv("cuda:0"), _srv("cuda:0")
    srcs = [_srv("cuda:0"), _srv("cuda:0")]
    before = compressed.mixed_fold_stats()
    assert compressed.fold_gradient_records(ds, [0.25, 0.75], gs, ps, srcs, [0.5, 0.125], 0.25) is True
    (a,) = ctypes_calls.calls
    s = len(SHAPE[kind])
    assert a[0] == f"flc_avg_and_gradient_{INFIX[kind]}records" and len(a) == 8 + s + 4
    assert [_vals(x) for x in a[1:5]] == [_ptr_list(ps), _ptr_list(gs), _ptr_list(srcs[0] + srcs[1]),
                                          _ptr_list([d.record for d in ds])]
    assert _vals(a[5]) == [0.5, 0.125] and _vals(a[6]) == [0.25, 0.75] and a[7] == 2
    assert a[8:8 + s] == SHAPE[kind]
    assert _vals(a[8 + s]) == [6, 4] and a[9 + s:] == (2, 0.25, _stream())
    ctypes_calls.calls.clear()
    staged = [torch.zeros(256, dtype=torch.uint8, device="cuda:0") for _ in ds]
    assert compressed.fold_gradient_records(ds, [0.25, 0.75], gs, records=staged) is True  # (update_gradients alone)
    (a,) = ctypes_calls.calls
    assert (a[1], a[3], a[5]) == (None, None, None) and _vals(a[4]) == _ptr_list(staged) and a[-2] == 0.0
    assert compressed.mixed_fold_stats() == before


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_ctypes_grouped_fold(ctypes_calls, kind):
    from fl_sim_amd import compressed

    d = _deltas("cuda:0")
    g0, g1 = [d[kind](), d[kind]()], [d[kind]()]
    dst0, dst1 = _srv("cuda:0"), _srv("cuda:0")
    before = compressed.mixed_fold_stats()
    assert compressed.fold_record_groups([(g0, [0.5, 0.25], dst0), ([], [], _srv("cuda:0")), (g1, [1], dst1)]) is True
    (a,) = ctypes_calls.calls
    s = len(SHAPE[kind])
    assert a[0] == f"flc_fold_{INFIX[kind]}record_groups" and len(a) == 5 + s + 5
    assert _vals(a[1]) == _ptr_list([x.record for x in g0 + g1]) and _vals(a[2]) == [0.5, 0.25, 1.0]
    assert _vals(a[3]) == [0, 0, 1] and a[4] == 3 and a[5:5 + s] == SHAPE[kind]
    r = a[5 + s:]
    assert _vals(r[0]) == _ptr_list(dst0 + dst1) and r[1] == 2 and _vals(r[2]) == [6, 4] and r[3:] == (2, _stream())
    ctypes_calls.calls.clear()
    assert compressed.fold_record_groups([(g0, [0.5, 0.25], dst0), (g1, [1], dst0)]) is False  # a shared destination
    assert compressed.fold_record_groups([(g0, [0.5, 0.25], dst0), ([d[kind](n=11)], [1], dst1)]) is False
    assert not ctypes_calls.calls and compressed.mixed_fold_stats() == before


def _mixed(dev="cuda:0"):
    d = _deltas(dev)
    ds = [d["stacked"](), d["sparse"](), d["quant"](), d["natural"](), d["flat"]()]
    cols = [[REC[k] for k in ("stacked", "sparse", "quant", "natural", "flat")], [2, 3, 0, 0, 0], [0, 0, 0, 2, 0],
            [10, 0, 127, 0, 0], [0, 0, 8, 16, 0]]
    return ds, cols, _ptr_list([x.record for x in ds[:4]] + [ds[4]._flat])


@pytest.mark.gpu
def test_ctypes_mixed_folds(ctypes_calls):
    from fl_sim_amd import compressed

    ds, cols, recs = _mixed()
    dp, th, v = _srv("cuda:0"), _srv("cuda:0"), _srv("cuda:0")
    ws = [0.5, 1, -0.25, 0, 2]
    st = compressed.mixed_fold_stats()
    assert compressed.fold_mixed_records(ds, ws, dp, th, v, 0.5, "yogi", 0.1, 0.99, 1e-3) is True
    (a,) = ctypes_calls.calls
    assert a[0] == "flc_fedopt_fold_mixed_records" and len(a) == 21
    assert _vals(a[1]) == recs and _vals(a[2]) == [float(w) for w in ws] and a[3:5] == (5, N)
    assert [_vals(x) for x in a[5:10]] == cols
    assert [_vals(x) for x in a[10:14]] == [_ptr_list(dp), _ptr_list(th), _ptr_list(v), [6, 4]]
    assert a[14:] == (2, 0.5, OPT["yogi"], 0.1, 0.99, 1e-3, _stream())
    assert compressed.mixed_fold_stats() == {"folds": st["folds"] + 1, "messages": st["messages"] + 5}

    ctypes_calls.calls.clear()
    dst0, dst1 = _srv("cuda:0"), _srv("cuda:0")
    assert compressed.fold_mixed_record_groups([(ds[:2], ws[:2], dst0), ([], [], _srv("cuda:0")),
                                                (ds[2:], ws[2:], dst1)]) is True
    (a,) = ctypes_calls.calls
    assert a[0] == "flc_fold_mixed_record_groups" and len(a) == 16
    assert _vals(a[1]) == recs and _vals(a[2]) == [float(w) for w in ws] and _vals(a[3]) == [0, 0, 1, 1, 1]
    assert a[4:6] == (5, N) and [_vals(x) for x in a[6:11]] == cols
    assert _vals(a[11]) == _ptr_list(dst0 + dst1) and a[12] == 2 and _vals(a[13]) == [6, 4]
    assert a[14:] == (2, _stream())
    assert compressed.mixed_fold_stats() == {"folds": st["folds"] + 2, "messages": st["messages"] + 10}

    ctypes_calls.calls.clear()
    gs, ps = _srv("cuda:0"), _srv("cuda:0")
    srcs = [_srv("cuda:0") for _ in ds]
    wp = [0.2] * 5
    assert compressed.fold_mixed_gradient_records(ds, ws, gs, ps, srcs, wp, 0.25) is True
    (a,) = ctypes_calls.calls
    assert a[0] == "flc_avg_and_gradient_mixed_records" and len(a) == 18
    assert [_vals(x) for x in a[1:5]] == [_ptr_list(ps), _ptr_list(gs), _ptr_list([t for r in srcs for t in r]), recs]
    assert _vals(a[5]) == [pytest.approx(0.2)] * 5 and _vals(a[6]) == [float(w) for w in ws] and a[7:9] == (5, N)
    assert [_vals(x) for x in a[9:14]] == cols and _vals(a[14]) == [6, 4] and a[15:] == (2, 0.25, _stream())
    assert compressed.mixed_fold_stats() == {"folds": st["folds"] + 3, "messages": st["messages"] + 15}

    ctypes_calls.calls.clear()  # a fold that declines counts nothing
    assert compressed.fold_mixed_record_groups([(ds[:2], ws[:2], dst0), (ds[2:], ws[2:], dst0)]) is False
    assert compressed.fold_mixed_records(ds, ws, dp, _srv("cpu"), None, 0.0) is False
    assert not ctypes_calls.calls
    assert compressed.mixed_fold_stats() == {"folds": st["folds"] + 3, "messages": st["messages"] + 15}
    compressed._MIXED_STATS.update(st)


@pytest.mark.gpu
def test_one_call_mixed_fold(monkeypatch):
    from fl_sim_amd import codec, compressed

    cells = _record_cells(monkeypatch)
    ds, cols, recs = _mixed()
    dp, th = _srv("cuda:0"), _srv("cuda:0")
    st = compressed.mixed_fold_stats()
    assert compressed.fold_mixed_records(ds, [1, 2, 3, 4, 5], dp, th, None, 0.5, "avg", 0.1, 0.99, 1e-3) is True
    a = _only(cells, "_PYMRECS")
    assert _ptr_list(a[0]) == recs and a[1] == [1.0, 2.0, 3.0, 4.0, 5.0] and a[2] == N and list(a[3:8]) == cols
    assert _same(a[8], dp) and _same(a[9], th) and a[10] is None and a[11:] == (0.5, OPT["avg"], 0.1, 0.99, 1e-3)
    assert compressed.mixed_fold_stats() == {"folds": st["folds"] + 1, "messages": st["messages"] + 5}
    compressed._MIXED_STATS.update(st)
    assert codec._pymrecs() is cells["_PYMRECS"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_update_gradients_fast_path(monkeypatch, kind):
    from fl_sim_amd import aggregation

    cells = _record_cells(monkeypatch, result=("the gradients",))
    ds = [_deltas("cuda:0")[kind]() for _ in range(3)]
    msgs = _msgs(ds, "gradients")
    mps = _srv("cuda:0")
    assert aggregation.update_gradients(mps, msgs) == "the gradients"
    a = _only(cells, CELL[kind][1])
    s = len(SHAPE[kind])
    assert len(a) == 5 + s + 2
    assert _same(a[0], mps) and a[1] is None and _same(a[2], [d.record for d in ds]) and a[3] is None
    assert a[4] == [1 / 6, 2 / 6, 3 / 6] and a[5:5 + s] == SHAPE[kind] and a[5 + s:] == (0.0, True)

    cells = _record_cells(monkeypatch, result=("the gradients",))  # with the parameters: the messages themselves
    for m in msgs:
        m["parameters"] = _srv("cuda:0")
    assert aggregation.avg_parameters_and_gradients(mps, msgs, size_aware=True, inertia=0.5) == "the gradients"
    a = _only(cells, CELL[kind][1])
    assert a[1] is msgs and a[3] == [1 / 12, 2 / 12, 3 / 12] and a[4] == [1 / 6, 2 / 6, 3 / 6]
    assert a[5 + s:] == (0.5, True)
