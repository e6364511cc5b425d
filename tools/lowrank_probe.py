"""The low-rank compressor on an MI355X (one JSON document, ``--out``, default profiles/lowrank_round.json; DESIGN.md
§3.3j quotes it), at n = 417,482 and 25,000,000 with rank 4 and the default cols:
(i) flc_lowrank_encode with ``residual`` in place, beside flc_sign_encode (whole-vector scale) with ``residual``;
(ii) flc_fold_lowrank_records over 10 records, beside 10 flc_lowrank_decode(accumulate) calls and beside
flc_fold_sign_wires over 10 sign records.  The legs alternate in one process; per leg the median and the range of
``--repeats`` repeats, each timing ``--calls`` calls with device events, microseconds per call.  The inputs are
whatever the previous call left in the caches: at the small size everything is L2 / MALL resident, at the large size
the vectors are not.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

RANK, RECORDS = 4, 10
SIZES = (417_482, 25_000_000)


def timed(legs, repeats, calls, warmup=3):
    us = {k: [] for k in legs}
    names = list(legs)
    for rep in range(repeats):
        for k in names[rep % len(names):] + names[:rep % len(names)]:
            for _ in range(warmup):
                legs[k]()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                legs[k]()
            e1.record()
            torch.cuda.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return us


def part(codec, _lib, dev, n, repeats, calls):
    g = torch.Generator(device=dev).manual_seed(n)
    cols = codec.lowrank_cols(n)
    m = -(-n // cols)
    st = codec._stream(dev)
    x = torch.randn(n, generator=g, device=dev) * 1e-2
    x0 = x.clone()
    q = torch.randn(cols, RANK, generator=g, device=dev)
    lbytes, sbytes = codec.lowrank_wire_layout(n, cols, RANK)[0], codec.sign_wire_layout(n, 0)[0]
    lrec = torch.zeros(lbytes, dtype=torch.uint8, device=dev)
    srec = torch.zeros(sbytes, dtype=torch.uint8, device=dev)
    sv, sb = codec.sign_wire_views(srec, n, 0)
    need = _lib.size("flc_lowrank_workspace_size", n, cols, RANK)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sneed = _lib.size("flc_sign_workspace_size", n, 0)
    sws = torch.empty(sneed, dtype=torch.uint8, device=dev)

    def lowrank_encode():  # (the memory shrinks call by call, as a client's does; the work does not depend on it)
        _lib.call("flc_lowrank_encode", x.data_ptr(), n, cols, RANK, q.data_ptr(), lrec.data_ptr(), None, None,
                  x.data_ptr(), ws.data_ptr(), need, st)

    def sign_encode():
        _lib.call("flc_sign_encode", x.data_ptr(), n, 0, sv.data_ptr(), sb.data_ptr(), None, x.data_ptr(),
                  sws.data_ptr(), sneed, st)

    enc = timed({"lowrank_encode_residual": lowrank_encode, "sign_encode_residual": sign_encode}, repeats, calls)

    # the fold's inputs: 10 encoded records of each kind
    lrecs, wires = [], torch.zeros(RECORDS * sbytes, dtype=torch.uint8, device=dev)
    for c in range(RECORDS):
        xc = x0 * (1 + 0.1 * c) + torch.randn(n, generator=g, device=dev) * 1e-3
        lrecs.append(codec.lowrank_encode(xc, q)[0])
        codec.sign_encode(xc, 0, record=wires[c * sbytes:(c + 1) * sbytes])
    out = torch.zeros(n, device=dev)
    ptrs = (ctypes.c_void_p * RECORDS)(*[r.data_ptr() for r in lrecs])
    wts = (ctypes.c_float * RECORDS)(*[0.1] * RECORDS)
    slots = (ctypes.c_int32 * RECORDS)(*range(RECORDS))
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def lowrank_fold():
        _lib.call("flc_fold_lowrank_records", cv(ptrs), cv(wts), RECORDS, n, cols, RANK, 0, out.data_ptr(), st)

    def lowrank_decodes():
        for c in range(RECORDS):
            _lib.call("flc_lowrank_decode", lrecs[c].data_ptr(), n, cols, RANK, 0.1, int(c > 0), out.data_ptr(), None,
                      None, st)

    def sign_fold():
        _lib.call("flc_fold_sign_wires", wires.data_ptr(), sbytes, cv(slots), cv(wts), RECORDS, n, 0, 0,
                  out.data_ptr(), st)

    fold = timed({"lowrank_fold_mfma": lowrank_fold, "lowrank_decode_x10": lowrank_decodes,
                  "sign_fold_wires": sign_fold}, repeats, calls)
    lowrank_fold()
    a = out.clone()
    lowrank_decodes()
    assert torch.allclose(a, out, rtol=1e-4, atol=1e-6), "the timed fold and the timed decodes disagree"

    doc = {"n": n, "cols": cols, "rows": m, "rank": RANK, "records": RECORDS,
           "record_bytes": {"lowrank": lbytes, "sign": sbytes, "decoded": 4 * n},
           "algorithmic_bytes": {
               "lowrank_encode_residual": 4 * n * 3 + 2 * need + lbytes,  # x twice, the residual, the partials twice
               "sign_encode_residual": 4 * n * 3 + sbytes,  # (bucket 0: x in the pass and in the scale launch)
               "lowrank_fold_mfma": 4 * n + RECORDS * lbytes,
               "lowrank_decode_x10": 4 * n * (2 * RECORDS - 1) + RECORDS * lbytes,
               "sign_fold_wires": 4 * n + RECORDS * sbytes}}
    for k, v in {**enc, **fold}.items():
        doc[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    return doc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "lowrank_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import _lib, codec

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"what": "the low-rank encode (with residual) beside the sign encode, and the MFMA fold of 10 records beside "
                   "10 accumulating decodes and the sign fold; device events, us per call (median, range of the "
                   "repeats); inputs as the previous call left them in the caches",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls,
           "sizes": [part(codec, _lib, dev, n, a.repeats, a.calls) for n in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
