"""Sparse records (flc_sparse_wire_layout) and the argument validation of their folds, of flc_sparse_gather and of
flc_ef_residual_sparse_round, which happens before anything touches the device, so it runs without one.  The pointers
are never dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
EINVAL = 1
TILE = 1024

NEW = ("flc_sparse_wire_layout", "flc_fold_sparse_wires", "flc_fedopt_fold_sparse_records",
       "flc_fold_sparse_record_groups", "flc_avg_and_gradient_sparse_records", "flc_sparse_gather",
       "flc_ef_residual_sparse_round")


def _lib():
    from fl_sim_amd import _lib as L

    return L


def test_symbols_exported():
    L = _lib()
    lib = L.load()
    for name in NEW:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.flc_abi_version() == 1
    from fl_sim_amd import _flcfold

    assert callable(_flcfold.fold_sparse_records)
    for old in ("fold_records", "fold_dense_records", "fold_record_groups", "avg_and_gradient_records"):
        assert callable(getattr(_flcfold, old))


def test_header_declares_the_new_entry_points():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "flcodec.h")).read()
    for name in NEW:
        assert name + "(" in text, name


@pytest.mark.parametrize("n,k", [(1, 1), (4097, 40), (70001, 700), (1000003, 333334)])
def test_layout(n, k):
    L = _lib()
    off = (ctypes.c_int64 * 3)(-1, -1, -1)
    total = L.size("flc_sparse_wire_layout", n, k, c(off))
    ntiles = (n + TILE - 1) // TILE + 1  # ceil(n / FLC_TILE) + 1 CSR pointers
    assert total > 0 and total % 256 == 0
    assert all(o >= 0 and o % 16 == 0 for o in off)  # every field 16-B aligned
    idx, val, tiles = off
    assert idx + 4 * k <= val and val + 4 * k <= tiles  # idx int32[k], val fp32[k], in that order, not overlapping
    assert tiles + 4 * ntiles <= total < tiles + 4 * ntiles + 256  # the tiles fit; less than one pad unit is added
    assert L.size("flc_sparse_wire_layout", n, k, None) == total  # (offsets are optional)
    from fl_sim_amd import codec

    assert codec.sparse_wire_layout(n, k) == (total, {"idx": idx, "val": val, "tiles": tiles})


def test_layout_is_smaller_than_the_dense_vector_at_one_percent():
    L = _lib()
    for n in (70001, 417482, 1000003):
        total = L.size("flc_sparse_wire_layout", n, n // 100, None)
        assert total < 4 * n and total < 8 * (n // 100) + 4 * ((n + TILE - 1) // TILE + 1) + 256 + 32


@pytest.mark.parametrize("n,k", [(0, 1), (-5, 1), (100, 0), (100, -1), (100, 101), (1, 2), (1 << 31, 5),
                                 (1 << 40, 5), ((1 << 31) + 5, 1 << 31)])
def test_layout_rejects(n, k):
    assert _lib().size("flc_sparse_wire_layout", n, k, None) == 0


def test_layout_just_below_the_limit():
    n = (1 << 31) - 1
    assert _lib().size("flc_sparse_wire_layout", n, n, None) > 8 * n


# ------------------------------------------------------------------------------------------------- the folds
def _wires(**kw):
    a = dict(wires=0x10000, stride=4096, slots=(ctypes.c_int32 * 2)(0, 1), weights=(ctypes.c_float * 2)(0.5, 1.0),
             n_wires=2, n=3000, k=30, accumulate=0, out=0x80000)
    a.update(kw)
    return (a["wires"], a["stride"], c(a["slots"]), c(a["weights"]), a["n_wires"], a["n"], a["k"], a["accumulate"],
            a["out"], None)


def _fedopt(**kw):
    a = dict(records=(P * 3)(256, 512, 768), weights=(ctypes.c_float * 3)(0.5, 1.0, -0.25), n_records=3, n=3000, k=30,
             delta=(P * 2)(0x10000, 0x20000), theta=(P * 2)(0x30000, 0x40000), v=(P * 2)(0x50000, 0x60000),
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2, opt=3)
    a.update(kw)
    return (c(a["records"]), c(a["weights"]), a["n_records"], a["n"], a["k"], c(a["delta"]), c(a["theta"]),
            c(a["v"]), c(a["sizes"]), a["n_tensors"], 0.5, a["opt"], 0.1, 0.99, 1e-3, None)


def _groups(**kw):
    a = dict(records=(P * 3)(256, 512, 768), weights=(ctypes.c_float * 3)(0.5, 1.0, -0.25),
             group_of=(ctypes.c_int32 * 3)(0, 2, 0), n_records=3, n=3000, k=30,
             dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x40000), n_groups=3,
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2)
    a.update(kw)
    return (c(a["records"]), c(a["weights"]), c(a["group_of"]), a["n_records"], a["n"], a["k"], c(a["dsts"]),
            a["n_groups"], c(a["sizes"]), a["n_tensors"], None)


def _pair(**kw):
    a = dict(params=(P * 2)(0x10000, 0x20000), grads=(P * 2)(0x30000, 0x40000),
             param_srcs=(P * 6)(0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000),
             grad_records=(P * 3)(256, 512, 768), w_params=(ctypes.c_float * 3)(0.3, 0.3, 0.4),
             w_grads=(ctypes.c_float * 3)(0.5, 1.0, -0.25), n_src=3, n=3000, k=30,
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2)
    a.update(kw)
    return (c(a["params"]), c(a["grads"]), None if a["param_srcs"] is None else c(a["param_srcs"]),
            c(a["grad_records"]), c(a["w_params"]), c(a["w_grads"]), a["n_src"], a["n"], a["k"], c(a["sizes"]),
            a["n_tensors"], 0.25, None)


def _gather(**kw):
    a = dict(x=0x10000, n=3000, idx=0x20000, k=30, val=0x30000)
    a.update(kw)
    return (a["x"], a["n"], a["idx"], a["k"], 1.5, a["val"], None)


def _residual(**kw):
    a = dict(records=(P * 2)(256, 512), es=(P * 2)(0x10000, 0x20000), n_clients=2, n=3000, k=30)
    a.update(kw)
    return (c(a["records"]), c(a["es"]), a["n_clients"], a["n"], a["k"], None)


K_BAD = {
    "k_zero": (dict(k=0), "k 0 outside [1, n = 3000]"),
    "k_above_n": (dict(k=3001), "k 3001 outside [1, n = 3000]"),
    "k_negative": (dict(k=-1), "bad arguments"),
    "k_too_large": (dict(k=1 << 31), "must be < 2^31"),
}
RECORD_BAD = {
    "null_record": (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "record_4_mod_16": (dict(records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"),
    "sizes_sum": (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
    "negative_size": (dict(sizes=(ctypes.c_int64 * 2)(-1, 3001)), "negative size for tensor 0"),
    "n_too_large": (dict(n=1 << 31, sizes=(ctypes.c_int64 * 2)(1 << 30, 1 << 30)), "must be < 2^31"),
    "n_zero": (dict(n=0), "bad arguments"),
    "no_tensors": (dict(n_tensors=0), "bad arguments"),
}
GROUP_BAD = {
    "group_below": (dict(group_of=(ctypes.c_int32 * 3)(0, -1, 0)), "record 1 names group -1 outside [0, 3)"),
    "group_above": (dict(group_of=(ctypes.c_int32 * 3)(0, 2, 3)), "record 2 names group 3 outside [0, 3)"),
    "shared_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x10000)),
                           "groups 0 and 2 share a destination"),
    "null_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0)), "null pointer for tensor 1 of group 2"),
    "no_groups": (dict(n_groups=0), "bad arguments"),
}
WIRES_BAD = {
    "null_wires": (dict(wires=None), "bad arguments"),
    "null_out": (dict(out=None), "bad arguments"),
    "wires_4_mod_16": (dict(wires=0x10004), "16-B aligned buffers required"),
    "out_4_mod_16": (dict(out=0x80004), "16-B aligned buffers required"),
    "short_stride": (dict(stride=256), "stride 256 < record size 512"),
    "stride_not_16": (dict(stride=4100), "not 16-B aligned"),
    "negative_slot": (dict(slots=(ctypes.c_int32 * 2)(0, -1)), "slot 1 is negative"),
    "n_too_large": (dict(n=1 << 31), "must be < 2^31"),
    "no_wires": (dict(n_wires=0), "bad arguments"),
}


def _check(fn, args, message):
    lib = _lib().load()
    assert getattr(lib, fn)(*args) == EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and fn in err, err


def test_record_size_of_the_validation_shape():
    """(3000, 30): idx 120 B -> val at 128, tiles at 256 (4 pointers) -> 512 B, the figure short_stride expects."""
    assert _lib().size("flc_sparse_wire_layout", 3000, 30, None) == 512


@pytest.mark.parametrize("case", list(K_BAD) + list(WIRES_BAD))
def test_fold_sparse_wires_validates_without_gpu(case):
    kw, message = (K_BAD.get(case) or WIRES_BAD[case])
    _check("flc_fold_sparse_wires", _wires(**kw), message)


@pytest.mark.parametrize("case", list(K_BAD) + list(RECORD_BAD))
def test_fedopt_fold_sparse_records_validates_without_gpu(case):
    kw, message = (K_BAD.get(case) or RECORD_BAD[case])
    _check("flc_fedopt_fold_sparse_records", _fedopt(**kw), message)


def test_fedopt_fold_sparse_records_more_checks():
    _check("flc_fedopt_fold_sparse_records", _fedopt(opt=7), "unknown optimiser 7")
    _check("flc_fedopt_fold_sparse_records", _fedopt(delta=(P * 2)(0x10000, 0)), "null pointer for tensor 1")
    _check("flc_fedopt_fold_sparse_records", _fedopt(theta=(P * 2)(0x30000, 0)), "null pointer for tensor 1")
    _check("flc_fedopt_fold_sparse_records", _fedopt(n_records=-1), "bad arguments")
    args = list(_fedopt())
    args[7] = None  # v missing under adam
    _check("flc_fedopt_fold_sparse_records", args, "v required")
    args = list(_fedopt())
    args[0] = None  # no record table
    _check("flc_fedopt_fold_sparse_records", args, "bad arguments")


@pytest.mark.parametrize("case", list(K_BAD) + list(RECORD_BAD) + list(GROUP_BAD))
def test_fold_sparse_record_groups_validates_without_gpu(case):
    kw, message = (K_BAD.get(case) or RECORD_BAD.get(case) or GROUP_BAD[case])
    _check("flc_fold_sparse_record_groups", _groups(**kw), message)


def test_fold_sparse_record_groups_without_records_is_a_no_op():
    """No record: nothing to fold, nothing launched (the tables are still checked)."""
    lib = _lib().load()
    assert lib.flc_fold_sparse_record_groups(*_groups(n_records=0)) == 0
    assert lib.flc_fold_sparse_record_groups(*_groups(n_records=0, k=0)) == EINVAL
    assert lib.flc_fold_sparse_record_groups(*_groups(n_records=0, sizes=(ctypes.c_int64 * 2)(1, 2))) == EINVAL


PAIR_BAD = {
    "null_record": (dict(grad_records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "record_4_mod_16": (dict(grad_records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"),
    "sizes_sum": (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
    "negative_size": (dict(sizes=(ctypes.c_int64 * 2)(-1, 3001)), "negative size for tensor 0"),
    "n_too_large": (dict(n=1 << 31), "must be < 2^31"),
    "no_sources": (dict(n_src=0), "bad arguments"),
    "null_gradient": (dict(grads=(P * 2)(0x30000, 0)), "null pointer for tensor 1"),
    "null_parameter": (dict(params=(P * 2)(0, 0x20000)), "null pointer for tensor 0"),
    "null_source": (dict(param_srcs=(P * 6)(0x50000, 0x60000, 0x70000, 0, 0x90000, 0xa0000)),
                    "null source 1 of tensor 1"),
}


@pytest.mark.parametrize("case", list(K_BAD) + list(PAIR_BAD))
def test_avg_and_gradient_sparse_records_validates_without_gpu(case):
    kw, message = (K_BAD.get(case) or PAIR_BAD[case])
    _check("flc_avg_and_gradient_sparse_records", _pair(**kw), message)


@pytest.mark.parametrize("kw", [dict(x=None), dict(idx=None), dict(val=None), dict(n=0), dict(k=-1)],
                         ids=lambda kw: next(iter(kw)))
def test_sparse_gather_validates_without_gpu(kw):
    _check("flc_sparse_gather", _gather(**kw), "bad arguments")


def test_sparse_gather_more_checks():
    _check("flc_sparse_gather", _gather(n=1 << 31), "must be < 2^31")
    _check("flc_sparse_gather", _gather(k=1 << 31), "must be < 2^31")
    assert _lib().load().flc_sparse_gather(*_gather(k=0, idx=None, val=None)) == 0  # nothing to gather


RESIDUAL_BAD = {
    "negative_clients": (dict(n_clients=-1), "bad arguments"),
    "negative_k": (dict(k=-1), "bad arguments"),
    "n_too_large": (dict(n=1 << 31), "must be < 2^31"),
    "k_above_n": (dict(k=3001), "k 3001 > n 3000"),
    "null_record": (dict(records=(P * 2)(256, 0)), "record 1 is null or not 16-B aligned"),
    "record_4_mod_16": (dict(records=(P * 2)(260, 512)), "record 0 is null or not 16-B aligned"),
    "null_memory": (dict(es=(P * 2)(0x10000, 0)), "null memory for client 1"),
    "shared_memory": (dict(es=(P * 2)(0x10000, 0x10000)), "clients 0 and 1 share a memory"),
}


@pytest.mark.parametrize("case", list(RESIDUAL_BAD))
def test_ef_residual_sparse_round_validates_without_gpu(case):
    kw, message = RESIDUAL_BAD[case]
    _check("flc_ef_residual_sparse_round", _residual(**kw), message)


def test_ef_residual_sparse_round_without_work_is_a_no_op():
    lib = _lib().load()
    assert lib.flc_ef_residual_sparse_round(*_residual(n_clients=0)) == 0
    assert lib.flc_ef_residual_sparse_round(*_residual(k=0)) == 0
    args = list(_residual())
    args[0] = None  # null tables with clients
    _check("flc_ef_residual_sparse_round", args, "bad arguments")


def test_the_stacked_entry_points_keep_their_messages():
    """The stacked folds share the host code the sparse ones extend: same checks, same texts, their own names."""
    lib = _lib().load()
    w = (ctypes.c_float * 2)(0.5, 1.0)
    s = (ctypes.c_int32 * 2)(0, 1)
    assert lib.flc_stacked_fold_wires(0x10000, 4096, c(s), c(w), 2, 3000, 30, 0, 0, 0x80000, None) == EINVAL
    assert "flc_stacked_fold_wires: levels must be in [1, 127]" in lib.flc_last_error().decode()
    assert lib.flc_stacked_fold_wires(0x10000, 4096, c(s), c(w), 2, 3000, 0, 127, 0, 0x80004, None) == EINVAL
    assert "flc_stacked_fold_wires: 16-B aligned buffers required" in lib.flc_last_error().decode()
    recs = (P * 3)(256, 512, 768)
    w3 = (ctypes.c_float * 3)(0.5, 1.0, -0.25)
    sz = (ctypes.c_int64 * 2)(1000, 2000)
    g = (P * 2)(0x30000, 0x40000)
    assert lib.flc_avg_and_gradient_records(None, c(g), None, c(recs), None, c(w3), 3, 3000, 30, 200, c(sz), 2, 0.0,
                                            None) == EINVAL
    assert "flc_avg_and_gradient_records: levels must be in [1, 127]" in lib.flc_last_error().decode()
    es = (P * 2)(0x10000, 0x20000)
    assert lib.flc_ef_residual_round(c((P * 2)(256, 512)), c(es), 2, 3000, 30, 0, None) == EINVAL
    assert "flc_ef_residual_round: levels must be in [1, 127]" in lib.flc_last_error().decode()


def test_opt_in_keywords_exist():
    """``sparse`` after ``wire`` on the three compress functions, off by default; the lists it selects."""
    import inspect

    from fl_sim_amd import compressed
    from fl_sim_amd.compressors import Compressor

    for f in (compressed.compress_delta, compressed.compress_tensors, compressed.compress_message_gradients):
        names = list(inspect.signature(f).parameters)
        assert names.index("sparse") == names.index("wire") + 1
        assert inspect.signature(f).parameters["sparse"].default is False

    def topk(k, d):
        t = Compressor("t")
        t.makeTopKCompressor(k, d)
        return t

    def randk(k, d):
        t = Compressor("r")
        t.makeRandKCompressor(k, d)
        return t

    sd = Compressor("q")
    ident = Compressor("n")
    ident.makeIdenticalCompressor()
    sd.makeStandardDitheringFP32(8, ident)
    sc = compressed.sparse_wire_codec
    assert sc([topk(700, 70001)]) == 700 and sc([randk(700, 70001)]) == 700
    assert sc([topk(700, 70001)], 70001) == 700 and sc([topk(700, 70001)], 500) is None  # K >= n
    assert sc([topk(0, 70001)]) is None and sc([topk(70001, 70001)]) is None and sc([topk(80000, 70001)]) is None
    assert sc([randk(700, 70001)], 70002) is None  # (a rand-k built for another length)
    assert sc([topk(30000, 70001)]) == 30000 and sc([topk(34000, 70001)]) == 34000
    assert sc([topk(35000, 70001)]) is None  # 8 K + the tile pointers reach 4 n: the record would not be smaller
    assert sc([topk(1, 40)]) is None  # (a 256-B record against 160 B)
    assert sc([topk(700, 70001), sd]) is None and sc([sd]) is None and sc([]) is None
    assert sc([topk(700, 70001), topk(700, 70001)]) is None
    assert compressed.dense_wire_codec([topk(700, 70001)]) is None  # (the other switch's records: not these)
    assert compressed.deferred_sparse_stats() == {"batches": 0, "messages": 0}
    assert compressed.sparse_round([]) is None
