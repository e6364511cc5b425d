"""flc_avg_and_gradient_dense_records: the symbol through every binding layer, and its argument validation, which
happens before anything touches the device, so it runs without one.  The pointers are never dereferenced."""

import ctypes
import os

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
EINVAL = 1
FN = "flc_avg_and_gradient_dense_records"
STD, NATD, NATURAL = 0, 1, 2


def _lib():
    from fl_sim_amd import _lib as L

    return L


def _pair(**kw):
    a = dict(params=(P * 2)(0x10000, 0x20000), grads=(P * 2)(0x30000, 0x40000),
             param_srcs=(P * 6)(0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xa0000),
             grad_records=(P * 3)(256, 512, 768), w_params=(ctypes.c_float * 3)(0.3, 0.3, 0.4),
             w_grads=(ctypes.c_float * 3)(0.5, 1.0, -0.25), n_src=3, n=3000, format=STD, levels=127, bits=8,
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2)
    a.update(kw)
    opt = lambda p: None if p is None else c(p)  # noqa: E731
    return (opt(a["params"]), opt(a["grads"]), opt(a["param_srcs"]), opt(a["grad_records"]), opt(a["w_params"]),
            opt(a["w_grads"]), a["n_src"], a["n"], a["format"], a["levels"], a["bits"], opt(a["sizes"]),
            a["n_tensors"], 0.25, None)


def _check(args, message):
    lib = _lib().load()
    assert getattr(lib, FN)(*args) == EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and FN in err, err


def test_symbol_exported_registered_and_bound():
    L = _lib()
    lib = L.load()
    assert hasattr(lib, FN) and FN in L.SIGNATURES
    res, args = L.SIGNATURES[FN]
    assert res is ctypes.c_int and len(args) == 15
    assert args[7:11] == [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]  # n, format, levels, bits
    from fl_sim_amd import _flcfold, codec

    for name in ("avg_and_gradient_dense_records", "avg_and_gradient_sparse_records", "avg_and_gradient_records"):
        assert callable(getattr(_flcfold, name)), name
    assert codec._pygdrecs() is _flcfold.avg_and_gradient_dense_records
    assert codec._pygsrecs() is _flcfold.avg_and_gradient_sparse_records
    assert codec._pygrecs() is _flcfold.avg_and_gradient_records


def test_header_declares_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "flcodec.h")).read()
    assert "int " + FN + "(" in text
    at = text.index("int " + FN + "(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "nodes.py:1134-1180" in comment and "compressors.py:357" in comment  # the reference lines it replaces


BAD = {
    "format_3": (dict(format=3), "unknown format 3"),
    "bits_3": (dict(bits=3), "bits must be 2, 4 or 8 (got 3)"),
    "natural_bits_8": (dict(format=NATURAL, bits=8), "the natural compressor's codes have 16 bits (got 8)"),
    "levels_0": (dict(levels=0, bits=4), "levels 0 does not fit 4-bit codes"),
    "levels_8_at_4_bits": (dict(levels=8, bits=4), "levels 8 does not fit 4-bit codes"),
    "no_sources": (dict(n_src=0), "bad arguments"),
    "sizes_sum_below": (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
    "sizes_sum_above": (dict(sizes=(ctypes.c_int64 * 2)(1000, 2001)), "the tensors hold 3001 elements, the records 3000"),
    "null_record": (dict(grad_records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "record_8_mod_16": (dict(grad_records=(P * 3)(256, 512, 776)), "record 2 is null or not 16-B aligned"),
    "params_without_w_params": (dict(w_params=None), "bad arguments"),
    "null_gradient": (dict(grads=(P * 2)(0x30000, 0)), "null pointer for tensor 1"),
    "n_too_large": (dict(n=1 << 31, sizes=(ctypes.c_int64 * 2)(1 << 30, 1 << 30)), "must be < 2^31"),
    "n_far_too_large": (dict(n=1 << 40), "must be < 2^31"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_avg_and_gradient_dense_records_validates_without_gpu(case):
    kw, message = BAD[case]
    _check(_pair(**kw), message)


@pytest.mark.parametrize("fmt,levels,bits", [(STD, 1, 2), (NATD, 7, 4), (STD, 127, 8), (NATURAL, 0, 16)])
def test_the_codec_check_comes_before_the_tensor_checks_for_every_format(fmt, levels, bits):
    """A well-formed (format, levels, bits) passes check_dense_format, so the next finding is the one reported —
    also with ``param_srcs`` NULL (update_gradients alone), where ``params`` and ``w_params`` may be NULL."""
    bad_sizes = (ctypes.c_int64 * 2)(1000, 1999)
    _check(_pair(format=fmt, levels=levels, bits=bits, sizes=bad_sizes), "the tensors hold 2999 elements")
    _check(_pair(format=fmt, levels=levels, bits=bits, sizes=bad_sizes, param_srcs=None, params=None, w_params=None),
           "the tensors hold 2999 elements")


def test_a_null_gradient_tensor_of_size_zero_is_accepted_by_the_checks():
    """Only a tensor of non-zero size needs a pointer: with one, the next check (the records) is the one that fails."""
    _check(_pair(grads=(P * 2)(0, 0x40000), params=(P * 2)(0, 0x20000), sizes=(ctypes.c_int64 * 2)(0, 3000),
                 grad_records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned")


def test_the_stacked_and_sparse_entries_keep_their_checks():
    lib = _lib().load()
    recs = (P * 3)(256, 512, 768)
    w3 = (ctypes.c_float * 3)(0.5, 1.0, -0.25)
    sz = (ctypes.c_int64 * 2)(1000, 2000)
    g = (P * 2)(0x30000, 0x40000)
    assert lib.flc_avg_and_gradient_records(None, c(g), None, c(recs), None, c(w3), 3, 3000, 30, 200, c(sz), 2, 0.0,
                                            None) == EINVAL
    assert "flc_avg_and_gradient_records: levels must be in [1, 127]" in lib.flc_last_error().decode()
    assert lib.flc_avg_and_gradient_sparse_records(None, c(g), None, c(recs), None, c(w3), 3, 3000, 0, c(sz), 2, 0.0,
                                                   None) == EINVAL
    assert "flc_avg_and_gradient_sparse_records: k 0 outside [1, n = 3000]" in lib.flc_last_error().decode()
