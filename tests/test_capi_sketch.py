"""Count-sketch records: layout, split rule, workspace and default sizes, the argument validation of the sketch entry
points (before anything touches the device, so it runs without one; the pointers are never dereferenced), and the
float64 reference's own recovery of planted coordinates with the seeds the device test uses."""

import ctypes

import numpy as np
import pytest

from fl_sim_amd import SketchCompressor, _lib as L, codec
from tests import sketch_ref as ref

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
RECOVERY_SEEDS = (1, 2, 3)


@pytest.mark.parametrize("n,rows,cols,total,splits,ws", [
    (1, 1, 4096, 16384, 1, 256), (8 * 4096, 3, 4096, 49152, 1, 256), (8 * 4096 + 1, 3, 4096, 49152, 2, 98304),
    (27 * 8192 + 3, 5, 8192, 163840, 4, 655360), (417_482, 5, 16384, 327680, 4, 1310720),
    (25_000_000, 5, 1 << 20, 20971520, 1, 256), (25_000_000, 5, 4096, 81920, 255, 255 * 81920),
])
def test_layout(n, rows, cols, total, splits, ws):
    off = (ctypes.c_int64 * 1)(-1)
    assert L.size("flc_sketch_wire_layout", n, rows, cols, c(off)) == total and off[0] == 0
    assert codec.sketch_wire_layout(n, rows, cols) == total
    assert L.load().flc_sketch_splits(n, cols) == splits
    assert L.size("flc_sketch_workspace_size", n, rows, cols) == ws


@pytest.mark.parametrize("D,rows,cols", [(1, 5, 4096), (163_839, 5, 4096), (163_840, 5, 8192), (417_482, 5, 16384),
                                         (417_482, 1, 65536), (25_000_000, 5, 1 << 20), (10 ** 9, 3, 1 << 20)])
def test_default_cols(D, rows, cols):
    comp = SketchCompressor(D, rows=rows)
    assert comp.cols == codec.sketch_cols(D, rows) == cols and comp.send_components() == rows * cols
    assert comp.is_biased and comp.compressorType == "SKETCH_COMPRESSOR"


@pytest.mark.parametrize("kw", [dict(rows=2), dict(rows=7), dict(cols=2048), dict(cols=5000), dict(cols=1 << 21),
                                dict(K=101), dict(D=0)])
def test_compressor_refuses(kw):
    with pytest.raises(ValueError):
        SketchCompressor(**{"D": 100, **kw})


@pytest.mark.parametrize("x", [np.zeros(100, np.float64), np.zeros(99, np.float32), np.zeros((10, 10), np.float32)])
def test_compress_vector_refuses_before_any_launch(x):
    with pytest.raises(ValueError):
        SketchCompressor(100).compressVector(x)


GOOD = dict(x=0x10000, n=70000, rows=3, cols=4096, record=0x30000, out=0x50000, ws=0x60000, ws_bytes=1 << 20,
            records=(P * 3)(256, 512, 768), n_records=3, u=0x70000, v=0x80000, idx=0x90000, k=5, cells=0xA0000)
W3 = (ctypes.c_float * 3)(0.5, 1.0, -0.25)
ARGS = {
    "flc_sketch_encode": lambda a: (a["x"], a["n"], a["rows"], a["cols"], 7, a["record"], a["out"], a["ws"],
                                    a["ws_bytes"], None),
    "flc_sketch_estimate": lambda a: (c(a["records"]), c(W3), a["n_records"], a["n"], a["rows"], a["cols"], 7,
                                      a["out"], None),
    "flc_sketch_fold": lambda a: (c(a["records"]), c(W3), a["n_records"], a["rows"], a["cols"], a["out"], None),
    "flc_sketch_state_step": lambda a: (c(a["records"]), c(W3), a["n_records"], a["rows"], a["cols"], 0.5, a["u"],
                                        a["v"], None),
    "flc_sketch_clear": lambda a: (a["idx"], a["k"], a["n"], a["rows"], a["cols"], 7, a["u"], a["v"], None),
    "flc_sketch_cells": lambda a: (a["idx"], a["k"], a["n"], a["rows"], a["cols"], 7, a["cells"], None),
}
TABLE_BAD = [(dict(rows=2), "rows 2 must be"), (dict(rows=0), "rows 0"), (dict(cols=2048), "cols 2048"),
             (dict(cols=4097), "cols 4097"), (dict(cols=1 << 21), "a power of two in")]
N_BAD = [(dict(n=0), "n must be in [1, 2^31)"), (dict(n=1 << 31), "2^31")]
REC_BAD = [(dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
           (dict(records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"), (dict(n_records=0), "no record")]
BAD = {
    "flc_sketch_encode": TABLE_BAD + N_BAD + [
        (dict(x=None), "null x or record"), (dict(record=None), "null x or record"), (dict(x=0x10004), "16-B aligned"),
        (dict(record=0x30008), "16-B aligned"), (dict(out=0x50004), "16-B aligned"), (dict(ws=None), "workspace"),
        (dict(ws_bytes=4096), "workspace 4096 < 147456"), (dict(ws=0x60010), "not 256-B aligned")],
    "flc_sketch_estimate": TABLE_BAD + N_BAD + REC_BAD + [
        (dict(out=None), "out is null"), (dict(out=0x50004), "out is null or not"), (dict(n_records=65), "at most 64")],
    "flc_sketch_fold": TABLE_BAD + REC_BAD + [(dict(out=None), "table is null"), (dict(out=0x50008), "table is null or")],
    "flc_sketch_state_step": TABLE_BAD + REC_BAD + [
        (dict(u=None), "u is null"), (dict(u=0x70004), "not 16-B aligned"), (dict(v=0x80004), "not 16-B aligned"),
        (dict(n_records=65), "at most 64")],
    "flc_sketch_clear": TABLE_BAD + N_BAD + [(dict(idx=None), "null idx"), (dict(k=-1), "k < 0"),
                                             (dict(u=None, v=None), "neither u nor v")],
    "flc_sketch_cells": TABLE_BAD + N_BAD + [(dict(idx=None), "null idx"), (dict(cells=None), "null cells")],
}


@pytest.mark.parametrize("fn,i", [(fn, i) for fn in ARGS for i in range(len(BAD[fn]))])
def test_refusals_without_gpu(fn, i):
    kw, message = BAD[fn][i]
    lib = L.load()
    assert getattr(lib, fn)(*ARGS[fn]({**GOOD, **kw})) == 1  # FLC_EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and fn in err


@pytest.mark.parametrize("n,rows,cols", [(0, 1, 4096), (1 << 31, 1, 4096), (100, 2, 4096), (100, 3, 2048),
                                         (100, 3, 6000), (100, 5, 1 << 21)])
def test_layout_and_workspace_reject(n, rows, cols):
    assert L.size("flc_sketch_wire_layout", n, rows, cols, None) == 0
    assert L.size("flc_sketch_workspace_size", n, rows, cols) == 0


@pytest.mark.parametrize("seed", RECOVERY_SEEDS)
def test_reference_recovers_planted(seed):
    """The hash itself, no device: the float64 sketch of 8 planted +-100 among 50 000 unit Gaussians (cols 8192,
    5 rows) gives them back as the 8 largest |estimate| — and bijective tile maps: no two elements of a chunk share a
    cell."""
    x, idx = ref.planted(seed)
    S, _ = ref.encode(x, 5, 8192, seed)
    est, _ = ref.estimate(S, x.size, 8192, seed)
    assert np.array_equal(np.sort(np.argsort(-np.abs(est))[:8]), idx)
    cell, _ = ref.all_cells(x.size, 8192, seed)
    assert all(np.unique(cell[q * 8192:(q + 1) * 8192, j]).size == min(8192, x.size - q * 8192)
               for q in range(7) for j in range(5))
