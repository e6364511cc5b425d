"""Low-rank records (flc_lowrank_wire_layout) and the argument validation of the low-rank entry points, which happens
before anything touches the device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

from fl_sim_amd import _lib as L, codec

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p


@pytest.mark.parametrize("n,cols,rank,q_off,total,ws", [
    (1, 256, 1, 16, 1280, 1280), (255, 256, 4, 16, 4352, 4352), (257, 256, 2, 16, 2304, 2304),
    (33 * 512 + 5, 512, 1, 144, 2304, 9 * 2048 + 256), (417482, 1024, 4, 6528, 23040, 102 * 16384 + 13056),
    (25_000_000, 1024, 4, 390640, 407040, 763 * 16384 + 97792),
])
def test_layout(n, cols, rank, q_off, total, ws):
    off = (ctypes.c_int64 * 2)(-1, -1)
    assert L.size("flc_lowrank_wire_layout", n, cols, rank, c(off)) == total and (off[0], off[1]) == (0, q_off)
    assert L.size("flc_lowrank_wire_layout", n, cols, rank, None) == total  # (offsets are optional)
    assert codec.lowrank_wire_layout(n, cols, rank) == (total, {"p": 0, "q": q_off})
    assert L.size("flc_lowrank_workspace_size", n, cols, rank) == ws


@pytest.mark.parametrize("D,cols", [(1, 256), (65536, 256), (65537, 512), (417482, 1024), (25_000_000, 1024)])
def test_default_cols(D, cols):
    assert codec.lowrank_cols(D) == cols


GOOD = dict(x=0x10000, n=3000, cols=256, rank=2, q=0x20000, record=0x30000, q_next=0x40000, out=0x50000,
            residual=None, ws=0x60000, ws_bytes=1 << 20, records=(P * 3)(256, 512, 768), n_records=3)
W3 = (ctypes.c_float * 3)(0.5, 1.0, -0.25)
ARGS = {
    "flc_lowrank_encode": lambda a: (a["x"], a["n"], a["cols"], a["rank"], a["q"], a["record"], a["q_next"], a["out"],
                                     a["residual"], a["ws"], a["ws_bytes"], None),
    "flc_lowrank_decode": lambda a: (a["record"], a["n"], a["cols"], a["rank"], 1.0, 0, a["out"], a["x"],
                                     a["residual"], None),
    "flc_fold_lowrank_records": lambda a: (c(a["records"]), c(W3), a["n_records"], a["n"], a["cols"], a["rank"], 0,
                                           a["out"], None),
}
SHAPE_BAD = [(dict(n=0), "n must be in [1, 2^31)"), (dict(n=1 << 31), "2^31"), (dict(cols=128), "cols 128 must be"),
             (dict(cols=768), "cols 768 must be"), (dict(cols=2048), "cols 2048"), (dict(rank=3), "rank 3"),
             (dict(rank=0), "rank 0"), (dict(rank=8), "rank 8")]
BAD = {
    "flc_lowrank_encode": [
        (dict(x=None), "null x, q or record"), (dict(q=None), "null x, q or record"),
        (dict(record=None), "null x, q or record"), (dict(x=0x10004), "must be 16-B aligned"),
        (dict(q=0x20008), "must be 16-B aligned"), (dict(record=0x30004), "must be 16-B aligned"),
        (dict(q_next=0x40004), "must be 16-B aligned"), (dict(out=0x50008), "must be 16-B aligned"),
        (dict(residual=0x50004), "must be 16-B aligned"), (dict(ws=None), "workspace"),
        (dict(ws_bytes=4096), "workspace 4096 < 6400"), (dict(ws=0x60010), "not 256-B aligned")],
    "flc_lowrank_decode": [
        (dict(record=None), "null record"), (dict(out=None), "neither out nor residual"),
        (dict(residual=0x50000, x=None), "residual without x"), (dict(out=0x50004), "must be 16-B aligned"),
        (dict(record=0x30008), "must be 16-B aligned"), (dict(residual=0x70004), "must be 16-B aligned")],
    "flc_fold_lowrank_records": [
        (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
        (dict(records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"),
        (dict(n_records=0), "no record"), (dict(out=None), "null records, weights or out"),
        (dict(out=0x50004), "out must be 16-B aligned")],
}


@pytest.mark.parametrize("fn,i", [(fn, i) for fn in ARGS for i in range(len(SHAPE_BAD) + len(BAD[fn]))])
def test_refusals_without_gpu(fn, i):
    kw, message = (SHAPE_BAD + BAD[fn])[i]
    lib = L.load()
    assert getattr(lib, fn)(*ARGS[fn]({**GOOD, **kw})) == 1  # FLC_EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and fn in err


@pytest.mark.parametrize("n,cols,rank", [(0, 256, 1), (1 << 31, 256, 1), (100, 128, 1), (100, 300, 2), (100, 256, 3)])
def test_layout_and_workspace_reject(n, cols, rank):
    assert L.size("flc_lowrank_wire_layout", n, cols, rank, None) == 0
    assert L.size("flc_lowrank_workspace_size", n, cols, rank) == 0
