"""Dense records (flc_dense_wire_layout) and the argument validation of their three folds, which happens before
anything touches the device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
EINVAL = 1

STD, NATD, NATURAL = 0, 1, 2  # FLC_Q_STANDARD_DITHER, FLC_Q_NATURAL_DITHER, FLC_WIRE_NATURAL
FORMATS = [(STD, 2), (STD, 4), (STD, 8), (NATD, 2), (NATD, 4), (NATD, 8), (NATURAL, 16)]
SIZES = [1, 3, 4, 1023, 1024, 1025, 70001]


def _lib():
    from fl_sim_amd import _lib as L

    return L


def test_symbols_exported():
    L = _lib()
    lib = L.load()
    for name in ("flc_dense_wire_layout", "flc_fold_dense_wires", "flc_fedopt_fold_dense_records",
                 "flc_fold_dense_record_groups"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert L.FLC_WIRE_NATURAL == NATURAL
    assert lib.flc_abi_version() == 1
    from fl_sim_amd import _flcfold

    assert callable(_flcfold.fold_dense_records)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt,bits", FORMATS)
def test_layout(n, fmt, bits):
    L = _lib()
    off = (ctypes.c_int64 * 2)(-1, -1)
    total = L.size("flc_dense_wire_layout", n, fmt, bits, c(off))
    code_bytes = 2 * n if fmt == NATURAL else (n * bits + 7) // 8
    assert total > 0 and total % 256 == 0
    assert off[1] % 16 == 0 and off[0] % 4 == 0
    assert off[0] + 4 <= off[1]  # the norm lies before the codes
    assert off[1] + code_bytes <= total < off[1] + code_bytes + 256  # the codes fit; less than one pad unit is added
    assert L.size("flc_dense_wire_layout", n, fmt, bits, None) == total  # (offsets are optional)
    if fmt != NATURAL:
        assert total <= 4 * n or n < 64  # 1/4 .. 1/16 of the dense bytes once the header is amortised
    from fl_sim_amd import codec

    assert codec.dense_wire_layout(n, fmt, bits) == (total, {"norm": off[0], "codes": off[1]})


@pytest.mark.parametrize("n,fmt,bits", [(100, STD, 1), (100, STD, 3), (100, STD, 16), (100, NATD, 0), (100, NATD, 16),
                                         (100, NATURAL, 8), (100, NATURAL, 2), (100, 3, 8), (100, -1, 8),
                                         (0, STD, 8), (-5, NATURAL, 16), (1 << 31, STD, 8), (1 << 31, NATURAL, 16),
                                         (1 << 40, NATD, 2)])
def test_layout_rejects(n, fmt, bits):
    assert _lib().size("flc_dense_wire_layout", n, fmt, bits, None) == 0


def test_layout_just_below_the_limit():
    assert _lib().size("flc_dense_wire_layout", (1 << 31) - 1, STD, 8, None) == (1 << 31) + 256


# ------------------------------------------------------------------------------------------------- the folds
def _wires(**kw):
    a = dict(wires=0x10000, stride=4096, slots=(ctypes.c_int32 * 2)(0, 1), weights=(ctypes.c_float * 2)(0.5, 1.0),
             n_wires=2, n=3000, format=STD, levels=7, bits=4, accumulate=0, out=0x80000)
    a.update(kw)
    return (a["wires"], a["stride"], c(a["slots"]), c(a["weights"]), a["n_wires"], a["n"], a["format"], a["levels"],
            a["bits"], a["accumulate"], a["out"], None)


def _fedopt(**kw):
    a = dict(records=(P * 3)(256, 512, 768), weights=(ctypes.c_float * 3)(0.5, 1.0, -0.25), n_records=3, n=3000,
             format=STD, levels=7, bits=4, delta=(P * 2)(0x10000, 0x20000), theta=(P * 2)(0x30000, 0x40000),
             v=(P * 2)(0x50000, 0x60000), sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2, opt=3)
    a.update(kw)
    return (c(a["records"]), c(a["weights"]), a["n_records"], a["n"], a["format"], a["levels"], a["bits"],
            c(a["delta"]), c(a["theta"]), c(a["v"]), c(a["sizes"]), a["n_tensors"], 0.5, a["opt"], 0.1, 0.99, 1e-3,
            None)


def _groups(**kw):
    a = dict(records=(P * 3)(256, 512, 768), weights=(ctypes.c_float * 3)(0.5, 1.0, -0.25),
             group_of=(ctypes.c_int32 * 3)(0, 2, 0), n_records=3, n=3000, format=STD, levels=7, bits=4,
             dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x40000), n_groups=3,
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2)
    a.update(kw)
    return (c(a["records"]), c(a["weights"]), c(a["group_of"]), a["n_records"], a["n"], a["format"], a["levels"],
            a["bits"], c(a["dsts"]), a["n_groups"], c(a["sizes"]), a["n_tensors"], None)


FORMAT_BAD = {
    "levels_8_in_4_bits": (dict(levels=8), "levels 8 does not fit 4-bit codes"),
    "levels_zero": (dict(levels=0), "levels 0 does not fit 4-bit codes"),
    "levels_2_in_2_bits": (dict(levels=2, bits=2), "levels 2 does not fit 2-bit codes"),
    "levels_128": (dict(levels=128, bits=8), "levels 128 does not fit 8-bit codes"),
    "bits_3": (dict(bits=3), "bits must be 2, 4 or 8"),
    "bits_16_dither": (dict(bits=16), "bits must be 2, 4 or 8"),
    "natural_8_bits": (dict(format=NATURAL, bits=8), "16 bits"),
    "unknown_format": (dict(format=3), "unknown format 3"),
}
RECORD_BAD = {
    "null_record": (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "record_4_mod_16": (dict(records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"),
    "sizes_sum": (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
    "n_too_large": (dict(n=1 << 31, sizes=(ctypes.c_int64 * 2)(1 << 30, 1 << 30)), "must be < 2^31"),
}
GROUP_BAD = {
    "group_below": (dict(group_of=(ctypes.c_int32 * 3)(0, -1, 0)), "record 1 names group -1 outside [0, 3)"),
    "group_above": (dict(group_of=(ctypes.c_int32 * 3)(0, 2, 3)), "record 2 names group 3 outside [0, 3)"),
    "shared_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x10000)),
                           "groups 0 and 2 share a destination"),
    "null_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0)), "null pointer for tensor 1 of group 2"),
}
WIRES_BAD = {
    "null_wires": (dict(wires=None), "bad arguments"),
    "wires_4_mod_16": (dict(wires=0x10004), "16-B aligned buffers required"),
    "out_4_mod_16": (dict(out=0x80004), "16-B aligned buffers required"),
    "short_stride": (dict(stride=1280), "stride 1280 < record size 1536"),
    "stride_not_16": (dict(stride=4100), "not 16-B aligned"),
    "negative_slot": (dict(slots=(ctypes.c_int32 * 2)(0, -1)), "slot 1 is negative"),
    "n_too_large": (dict(n=1 << 31), "must be < 2^31"),
    "no_wires": (dict(n_wires=0), "bad arguments"),
}


def _check(fn, args, message):
    lib = _lib().load()
    assert getattr(lib, fn)(*args) == EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and fn in err


@pytest.mark.parametrize("case", list(FORMAT_BAD) + list(WIRES_BAD))
def test_fold_dense_wires_validates_without_gpu(case):
    kw, message = (FORMAT_BAD.get(case) or WIRES_BAD[case])
    _check("flc_fold_dense_wires", _wires(**kw), message)


@pytest.mark.parametrize("case", list(FORMAT_BAD) + list(RECORD_BAD))
def test_fedopt_fold_dense_records_validates_without_gpu(case):
    kw, message = (FORMAT_BAD.get(case) or RECORD_BAD[case])
    _check("flc_fedopt_fold_dense_records", _fedopt(**kw), message)


def test_fedopt_fold_dense_records_more_checks():
    _check("flc_fedopt_fold_dense_records", _fedopt(opt=7), "unknown optimiser 7")
    _check("flc_fedopt_fold_dense_records", _fedopt(delta=(P * 2)(0x10000, 0)), "null pointer for tensor 1")
    args = list(_fedopt())
    args[9] = None  # v missing under adam
    _check("flc_fedopt_fold_dense_records", args, "v required")


@pytest.mark.parametrize("case", list(FORMAT_BAD) + list(RECORD_BAD) + list(GROUP_BAD))
def test_fold_dense_record_groups_validates_without_gpu(case):
    kw, message = (FORMAT_BAD.get(case) or RECORD_BAD.get(case) or GROUP_BAD[case])
    _check("flc_fold_dense_record_groups", _groups(**kw), message)


def test_fold_dense_record_groups_without_records_is_a_no_op():
    """No record: nothing to fold, nothing launched (the tables are still checked)."""
    L = _lib()
    lib = L.load()
    assert lib.flc_fold_dense_record_groups(*_groups(n_records=0)) == 0
    assert lib.flc_fold_dense_record_groups(*_groups(n_records=0, format=NATURAL, bits=16, levels=0)) == 0
    assert lib.flc_fold_dense_record_groups(*_groups(n_records=0, levels=8)) == EINVAL
    with pytest.raises(L.FlcError, match="levels"):
        L.call("flc_fold_dense_record_groups", *_groups(levels=200, bits=8))


def test_opt_in_keywords_exist():
    """``wire`` on compress_delta / compress_tensors, off by default; the record kinds it selects."""
    import inspect

    import numpy as np

    from fl_sim_amd import compressed
    from fl_sim_amd.compressors import Compressor

    for f in (compressed.compress_delta, compressed.compress_tensors):
        p = inspect.signature(f).parameters["wire"]
        assert p.default is False
    ident = Compressor("n")
    ident.makeIdenticalCompressor()

    def std(s, p=np.inf, nc=ident):
        q = Compressor("q")
        q.makeStandardDitheringFP32(s, nc, p)
        return q

    def natd(s):
        q = Compressor("q")
        q.makeNaturalDitheringFP32(s, 1000)
        return q

    nat = Compressor("q")
    nat.makeNaturalCompressorFP32()
    tk = Compressor("t")
    tk.makeTopKCompressor(10, 1000)
    dc = compressed.dense_wire_codec
    assert dc([std(1)]) == (STD, 1, 2) and dc([std(4)]) == (STD, 4, 4) and dc([std(7)]) == (STD, 7, 4)
    assert dc([std(8)]) == (STD, 8, 8) and dc([std(10, 2)]) == (STD, 10, 8)
    assert dc([natd(7)]) == (NATD, 7, 4) and dc([natd(100)]) == (NATD, 100, 8)
    assert dc([nat]) == (NATURAL, 0, 16)
    assert dc([std(4, nc=nat)]) is None  # (a norm compressor that is not the identical one)
    assert dc([tk]) is None and dc([tk, std(4)]) is None and dc([]) is None and dc([std(4), std(4)]) is None
    nat64 = Compressor("q")
    nat64.makeNaturalCompressorFP64()
    assert dc([nat64]) is None
