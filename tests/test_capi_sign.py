"""Sign records (flc_sign_wire_layout) and the argument validation of the scaled-sign entry points, which happens
before anything touches the device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

from fl_sim_amd import _lib as L, codec

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p


@pytest.mark.parametrize("n,bucket,bits_off,total", [
    (1, 0, 16, 256), (1, 64, 16, 256), (1920, 0, 16, 256), (1921, 0, 16, 512), (4097, 512, 48, 768),
    (4097, 64, 272, 1024), (70001, 4096, 80, 8960), (70001, 0, 16, 8960), ((1 << 31) - 1, 0, 16, (1 << 28) + 256),
])
def test_layout(n, bucket, bits_off, total):
    off = (ctypes.c_int64 * 2)(-1, -1)
    assert L.size("flc_sign_wire_layout", n, bucket, c(off)) == total and (off[0], off[1]) == (0, bits_off)
    assert L.size("flc_sign_wire_layout", n, bucket, None) == total  # (offsets are optional)
    assert codec.sign_wire_layout(n, bucket) == (total, {"scales": 0, "bits": bits_off})
    assert L.size("flc_sign_workspace_size", n, bucket) == (0 if bucket else (8 * -(-n // 4096) + 255) // 256 * 256)


@pytest.mark.parametrize("n,bucket", [(0, 0), (-3, 64), (1 << 31, 0), (100, 32), (100, 96), (100, 8192), (100, -64)])
def test_layout_and_workspace_reject(n, bucket):
    assert L.size("flc_sign_wire_layout", n, bucket, None) == 0 and L.size("flc_sign_workspace_size", n, bucket) == 0


W3, DST = (ctypes.c_float * 3)(0.5, 1.0, -0.25), (P * 4)(0x10000, 0x20000, 0x30000, 0x40000)
GOOD = dict(x=0x10000, n=3000, bucket=512, scales=0x20000, bits=0x20020, out=0x30000, residual=None, ws=0x40000,
            ws_bytes=256, wires=0x10000, stride=4096, slots=(ctypes.c_int32 * 2)(0, 1), records=(P * 3)(256, 512, 768),
            sizes=(ctypes.c_int64 * 2)(1000, 2000))
ARGS = {  # the entry points' argument lists over one table of good values
    "flc_sign_encode": lambda a: (a["x"], a["n"], a["bucket"], a["scales"], a["bits"], a["out"], a["residual"],
                                  a["ws"], a["ws_bytes"], None),
    "flc_sign_decode": lambda a: (a["bits"], a["n"], a["bucket"], a["scales"], 1.0, 0, a["out"], None),
    "flc_fold_sign_wires": lambda a: (a["wires"], a["stride"], c(a["slots"]), c(W3), 2, a["n"], a["bucket"], 0,
                                      a["out"], None),
    "flc_fedopt_fold_sign_records": lambda a: (c(a["records"]), c(W3), 3, a["n"], a["bucket"], c(DST), None, None,
                                               c(a["sizes"]), 2, 0.5, 0, 0.1, 0.99, 1e-3, None),
    "flc_avg_and_gradient_sign_records": lambda a: (None, c(DST), None, c(a["records"]), None, c(W3), 3, a["n"],
                                                    a["bucket"], c(a["sizes"]), 2, 0.0, None),
    "flc_fold_sign_record_groups": lambda a: (c(a["records"]), c(W3), c((ctypes.c_int32 * 3)(0, 1, 0)), 3, a["n"],
                                              a["bucket"], c(DST), 2, c(a["sizes"]), 2, None),
}
SHAPE_BAD = [(dict(bucket=96), "bucket 96 is not 0 or a power of two in [64, 4096]"),  # every entry point
             (dict(bucket=8192), "bucket 8192 is not 0 or"), (dict(n=0), ""), (dict(n=1 << 31), "2^31")]
RECORD_BAD = [
    (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    (dict(records=(P * 3)(256, 512, 772)), "record 2 is null or not 16-B aligned"),
    (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
]
BAD = {
    "flc_sign_encode": [
        (dict(x=None), "null x, scales or bits"), (dict(scales=None), "null x, scales or bits"),
        (dict(bits=None), "null x, scales or bits"), (dict(x=0x10004), "must be 16-B aligned"),
        (dict(bits=0x20024), "must be 16-B aligned"), (dict(out=0x30008), "must be 16-B aligned"),
        (dict(residual=0x30004), "must be 16-B aligned"), (dict(bucket=0, ws=None), "workspace 256 < 256"),
        (dict(bucket=0, n=4096 * 40), "workspace 256 < 512"), (dict(bucket=0, ws=0x40004), "not 8-B aligned")],
    "flc_sign_decode": [
        (dict(bits=None), "null bits, scales or out"), (dict(scales=None), "null bits, scales or out"),
        (dict(out=None), "null bits, scales or out"), (dict(out=0x30004), "must be 16-B aligned"),
        (dict(bits=0x20028), "must be 16-B aligned")],
    "flc_fold_sign_wires": [
        (dict(wires=None), "bad arguments"), (dict(out=0x30004), "16-B aligned buffers required"),
        (dict(stride=256), "stride 256 < record size 512"), (dict(stride=256, bucket=0), "stride 256 < record size 512"),
        (dict(slots=(ctypes.c_int32 * 2)(0, -1)), "slot 1 is negative")],
    "flc_fedopt_fold_sign_records": RECORD_BAD,
    "flc_avg_and_gradient_sign_records": RECORD_BAD,
    "flc_fold_sign_record_groups": RECORD_BAD,
}


@pytest.mark.parametrize("fn,i", [(fn, i) for fn in ARGS for i in range(len(SHAPE_BAD) + len(BAD[fn]))])
def test_refusals_without_gpu(fn, i):
    kw, message = (SHAPE_BAD + BAD[fn])[i]
    lib = L.load()
    assert getattr(lib, fn)(*ARGS[fn]({**GOOD, **kw})) == 1  # FLC_EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and fn in err

