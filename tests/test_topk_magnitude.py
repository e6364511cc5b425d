"""Top-k by magnitude, CPU side: the numpy model (tests/topk_magnitude_ref.py) against the fixture made by running the
reference's own compressors on ``|x|`` (tests/golden/topk_magnitude.npz), the host surface of the feature, and the
carry-over of the path catalogue (tests/select_cases.py): no case of it has a sign bit set, so flipping sign bits
leaves ``|x'| == x`` bit for bit and the signed select's preconditions on ``x`` are the magnitude select's on ``x'``."""

import ctypes
import os
import random

import numpy as np
import pytest

from fl_sim_amd import Compressor, _lib, codec, compressed
from oracle import compressors_ref as ref
from tests import select_cases as sc
from tests import topk_magnitude_ref as mref
from tests.golden import gen_golden_topk_magnitude as gen

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_magnitude.npz"))
FLC_EINVAL = 1  # include/flcodec.h
ORD_SYMBOLS = ("flc_topk_encode_tiled_ord", "flc_topk_encode_batch_ord", "flc_stacked_encode_tiled_ord",
               "flc_stacked_encode_delta_ord", "flc_stacked_encode_round_ord", "flc_stacked_encode_delta_round_ord",
               "flc_topk_dense_f64_ord")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------------------------------------ 1. the fixture
def test_fixture_holds_every_case():
    assert gen.MAG_NS == (7, 1000, 5000) and gen.MAG_LEVELS == (1, 7, 10)
    assert [gen.mag_ks(n) for n in gen.MAG_NS] == [(1, 3, 6), (1, 10, 999), (1, 50, 4999)]
    want = {f"x_n{n}" for n in gen.MAG_NS}
    for n, K in gen.mag_cases():
        want.add(gen.mag_key(n, K) + "|mask")
        for s in gen.MAG_LEVELS:
            want |= {f"{gen.mag_key(n, K)}_s{s}|{f}" for f in ("out", "stats", "next_random")}
    assert set(GOLD.files) == want
    for n in gen.MAG_NS:
        x = GOLD[f"x_n{n}"]
        assert np.array_equal(_bits(x), _bits(gen.mag_input(n)))
        assert np.all(x != 0) and np.unique(np.abs(x)).size == n and (x < 0).any() and (x > 0).any()


@pytest.mark.parametrize("n,K", list(gen.mag_cases()))
def test_model_reproduces_the_reference_kept_set(n, K):
    x = GOLD[f"x_n{n}"]
    mask = GOLD[gen.mag_key(n, K) + "|mask"].astype(bool)
    for fast in (False, True):
        idx, vals = mref.kept(x, K, fast)
        assert np.array_equal(idx, np.flatnonzero(mask)) and np.array_equal(_bits(vals), _bits(x[mask]))
    assert np.array_equal(_bits(mref.topk(x, K)), _bits(np.where(mask, x, np.float32(0))))
    assert (mref.kept(x, K)[1] < 0).any() or K == 1  # (mixed signs: the kept values keep their own)


@pytest.mark.parametrize("s", gen.MAG_LEVELS)
@pytest.mark.parametrize("n,K", list(gen.mag_cases()))
def test_model_reproduces_the_reference_stacked_pipeline(n, K, s):
    """Output, send statistics and the compat stream's position: one ``random.random()`` per non-zero kept entry, in
    index order."""
    x = GOLD[f"x_n{n}"]
    key = f"{gen.mag_key(n, K)}_s{s}"
    random.seed(gen.mag_seed(n, K, s))
    out, idx, codes, pn = mref.stacked(x, K, s, ref.python_random_stream())
    nxt = random.random()
    assert np.array_equal(_bits(out), _bits(GOLD[key + "|out"]))
    assert nxt == float(GOLD[key + "|next_random"])
    assert _bits(np.array([pn]))[0] == _bits(np.array([np.max(np.abs(x))], dtype=np.float32))[0]  # max|kept| = max|x|
    # the second stage alone, on the kept values: the oracle's standard dithering of the K-sparse vector
    y = mref.topk(x, K)
    random.seed(gen.mag_seed(n, K, s))
    out2, send, _ = ref.standard_dithering(y, s, np.inf, ref.python_random_stream())
    assert np.array_equal(_bits(out2), _bits(out))
    assert np.array_equal(GOLD[key + "|stats"], np.array([send, n, 1.0, 1.0]))
    assert np.array_equal(codes >> 7, np.signbit(x[idx]).astype(np.uint8))  # the code's sign bit: the value's own


# ------------------------------------------------------------------------------------------------ 2. host surface
def test_factory_default_and_names():
    c = Compressor()
    assert c.magnitude is False
    c.makeTopKCompressor(5, 100)
    assert c.magnitude is False and c.order == codec.ORDER_SIGNED
    assert c.name == "Top-K (K=5) Compressor" and c.fullName == "Top [K=5,D=100]"
    m = Compressor()
    m.makeTopKCompressor(5, 100, magnitude=True)
    assert m.magnitude is True and m.order == codec.ORDER_MAGNITUDE
    assert m.name == "Top-K by magnitude (K=5) Compressor" and m.fullName == "Top|x| [K=5,D=100]"
    assert m.is_biased == c.is_biased and m.w == c.w == 0.0 and m.compressorType == c.compressorType
    m.makeRandKCompressor(5, 100)  # every other factory leaves it False
    assert m.magnitude is False
    nc = Compressor("norm")
    nc.makeIdenticalCompressor()
    m.makeTopKCompressor(5, 100, magnitude=True)
    m.makeStandardDitheringFP32(8, nc)
    assert m.magnitude is False
    m.makeTopKCompressor(5, 100, True)
    m.makeNaturalDitheringFP32(8, 100)
    assert m.magnitude is False


def test_order_helper():
    tk, mk, sd, nc = Compressor(), Compressor(), Compressor(), Compressor("norm")
    nc.makeIdenticalCompressor()
    tk.makeTopKCompressor(5, 100)
    mk.makeTopKCompressor(5, 100, magnitude=True)
    sd.makeStandardDitheringFP32(8, nc)
    assert compressed.pipeline_order([tk]) == compressed.pipeline_order([tk, sd]) == codec.ORDER_SIGNED
    assert compressed.pipeline_order([mk]) == compressed.pipeline_order([mk, sd]) == codec.ORDER_MAGNITUDE
    assert compressed.pipeline_order([sd]) == compressed.pipeline_order([]) == codec.ORDER_SIGNED
    assert compressed.stacked_pipeline([mk, sd]) == compressed.stacked_pipeline([tk, sd]) == (5, 8)
    assert (codec.ORDER_SIGNED, codec.ORDER_MAGNITUDE) == (0, 1)
    assert codec._order("magnitude") == 1 and codec._order("signed") == 0 and codec._order(1) == 1
    for bad in (2, -1, "abs"):
        with pytest.raises(ValueError):
            codec._order(bad)


def test_ord_symbols_are_declared_and_exported():
    lib = _lib.load()
    assert lib.flc_abi_version() == 1
    for name in ORD_SYMBOLS:
        base = name[:-4]
        res, args = _lib.SIGNATURES[name]
        bres, bargs = _lib.SIGNATURES[base]
        assert res is ctypes.c_int and bres is ctypes.c_int
        kpos = max(i for i, a in enumerate(bargs[:6]) if a is ctypes.c_int64)  # k: the last int64 of the head
        assert list(args) == list(bargs[:kpos + 1]) + [ctypes.c_int] + list(bargs[kpos + 1:]), name
        assert hasattr(lib, name) and getattr(lib, name).argtypes == list(args)


def test_a_bad_order_is_rejected_before_any_launch():
    """FLC_EINVAL for an order that is neither 0 nor 1 (the arguments are otherwise well-formed host values; nothing is
    dereferenced or launched)."""
    lib = _lib.load()
    raw = ctypes.create_string_buffer(1024 + 16)  # scratch standing in for every pointer, 16-B aligned
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    one = (ctypes.c_void_p * 1)(p.value)
    op = ctypes.cast(one, ctypes.c_void_p)
    sz = ctypes.cast((ctypes.c_int64 * 1)(8), ctypes.c_void_p)
    for order in (2, -1):
        assert lib.flc_topk_encode_tiled_ord(p, 8, 2, order, p, p, None, p, 512, None) == FLC_EINVAL
        assert b"order" in lib.flc_last_error()
        assert lib.flc_topk_encode_batch_ord(op, 1, 8, 2, order, op, op, None, p, 512, None) == FLC_EINVAL
        assert lib.flc_stacked_encode_tiled_ord(p, 8, 2, order, 7, 0, 0, None, p, p, p, None, p, 512,
                                                None) == FLC_EINVAL
        assert lib.flc_stacked_encode_delta_ord(op, op, sz, 1, 2, order, 7, 0, 0, p, p, p, p, p, 512,
                                                None) == FLC_EINVAL
        assert lib.flc_stacked_encode_round_ord(op, 1, 8, 2, order, 7, p, p, op, op, op, None, None, p, 512,
                                                None) == FLC_EINVAL
        assert lib.flc_stacked_encode_delta_round_ord(op, op, sz, 1, 1, 2, order, 7, p, p, op, op, op, op, None, p, 512,
                                                      None) == FLC_EINVAL
        assert lib.flc_topk_dense_f64_ord(p, 8, 2, order, p, p, 512, None) == FLC_EINVAL
        assert b"order" in lib.flc_last_error()


# ------------------------------------------------------------------------------------------------ 3. the catalogue
CUS = 256


def plan_of(n, k, clients=0):
    return codec.topk_select_plan(n, k, clients, CUS)


SINGLE = sc.single_cases(plan_of)[0]
STORAGE = sc.storage_cases(plan_of)
CATALOGUE = {**SINGLE, **STORAGE}


def test_the_catalogue_is_the_27_cases():
    assert sorted(CATALOGUE) == sorted(sc.SINGLE_NAMES + sc.STORAGE_NAMES) and len(CATALOGUE) == 27


@pytest.mark.parametrize("name", sc.SINGLE_NAMES + sc.STORAGE_NAMES)
def test_catalogue_case_carries_over(name):
    case = CATALOGUE[name]()
    x = case.x
    assert not np.signbit(x).any(), name  # no negative element (no -0, no negative NaN either)
    xf = mref.flip_signs(x, 1234)
    assert np.signbit(xf).any() and not np.signbit(xf).all()
    assert np.array_equal(_bits(np.abs(xf)), _bits(x))  # |x'| == x bit for bit
    sc.precondition(case, plan_of(x.size, case.k))  # ... so x's precondition is the magnitude select's on x'
    idx, vals = mref.kept(xf, case.k, fast=True)
    assert np.array_equal(idx, ref.topk_kept_select(x, case.k)[0]) and np.array_equal(_bits(vals), _bits(xf[idx]))
