"""The count sketch on an MI355X (one JSON document, ``--out``, default profiles/sketch_round.json; DESIGN.md §3.3k
quotes it), at n = 417,482 and 25,000,000 with 5 rows and the default cols:
(i) flc_sketch_encode (no estimate), beside flc_sign_encode (whole-vector scale, no residual), flc_lowrank_encode
(rank 4, no residual: two reads of x) and a stream copy of x (one read and one write of x on the same box);
(ii) flc_sketch_estimate over 10 records, beside 10 flc_lowrank_decode(accumulate) calls.
The legs alternate in one process; per leg the median and the range of ``--repeats`` repeats, each timing ``--calls``
calls with device events, microseconds per call.  The inputs are whatever the previous call left in the caches: at the
small size everything is L2 / MALL resident, at the large size the vectors are not.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROWS, RANK, RECORDS, SEED = 5, 4, 10, 2020
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
    cols, lcols = codec.sketch_cols(n, ROWS), codec.lowrank_cols(n)
    st = codec._stream(dev)
    x = torch.randn(n, generator=g, device=dev) * 1e-2
    y = torch.empty_like(x)
    q = torch.randn(lcols, RANK, generator=g, device=dev)
    kbytes, sbytes = codec.sketch_wire_layout(n, ROWS, cols), codec.sign_wire_layout(n, 0)[0]
    lbytes = codec.lowrank_wire_layout(n, lcols, RANK)[0]
    krec, srec, lrec = (torch.zeros(b, dtype=torch.uint8, device=dev) for b in (kbytes, sbytes, lbytes))
    sv, sb = codec.sign_wire_views(srec, n, 0)
    need = {k: _lib.size(f, *a) for k, f, a in (("k", "flc_sketch_workspace_size", (n, ROWS, cols)),
                                                ("s", "flc_sign_workspace_size", (n, 0)),
                                                ("l", "flc_lowrank_workspace_size", (n, lcols, RANK)))}
    ws = {k: torch.empty(b, dtype=torch.uint8, device=dev) for k, b in need.items()}

    def sketch_encode():
        _lib.call("flc_sketch_encode", x.data_ptr(), n, ROWS, cols, SEED, krec.data_ptr(), None, ws["k"].data_ptr(),
                  need["k"], st)

    def sign_encode():
        _lib.call("flc_sign_encode", x.data_ptr(), n, 0, sv.data_ptr(), sb.data_ptr(), None, None, ws["s"].data_ptr(),
                  need["s"], st)

    def lowrank_encode():
        _lib.call("flc_lowrank_encode", x.data_ptr(), n, lcols, RANK, q.data_ptr(), lrec.data_ptr(), None, None, None,
                  ws["l"].data_ptr(), need["l"], st)

    enc = timed({"sketch_encode": sketch_encode, "sign_encode": sign_encode, "lowrank_encode": lowrank_encode,
                 "stream_copy": lambda: y.copy_(x)}, repeats, calls)

    krecs, lrecs = [], []
    for c in range(RECORDS):
        xc = x * (1 + 0.1 * c) + torch.randn(n, generator=g, device=dev) * 1e-3
        krecs.append(codec.sketch_encode(xc, ROWS, cols, SEED)[0])
        lrecs.append(codec.lowrank_encode(xc, q)[0])
    out = torch.zeros(n, device=dev)
    ptrs = (ctypes.c_void_p * RECORDS)(*[r.data_ptr() for r in krecs])
    wts = (ctypes.c_float * RECORDS)(*[0.1] * RECORDS)
    cv = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731

    def sketch_estimate():
        _lib.call("flc_sketch_estimate", cv(ptrs), cv(wts), RECORDS, n, ROWS, cols, SEED, out.data_ptr(), st)

    def lowrank_decodes():
        for c in range(RECORDS):
            _lib.call("flc_lowrank_decode", lrecs[c].data_ptr(), n, lcols, RANK, 0.1, int(c > 0), out.data_ptr(), None,
                      None, st)

    est = timed({"sketch_estimate_10": sketch_estimate, "lowrank_decode_x10": lowrank_decodes}, repeats, calls)

    doc = {"n": n, "rows": ROWS, "cols": cols, "splits": _lib.load().flc_sketch_splits(n, cols), "records": RECORDS,
           "record_bytes": {"sketch": kbytes, "sign": sbytes, "lowrank": lbytes, "decoded": 4 * n},
           "algorithmic_bytes": {"sketch_encode": 4 * n + kbytes + (2 * need["k"] if need["k"] > 256 else 0),
                                 "stream_copy": 8 * n, "sketch_estimate_10": 4 * n + RECORDS * kbytes}}
    for k, v in {**enc, **est}.items():
        doc[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    return doc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sketch_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import _lib, codec

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"what": "the count-sketch encode beside the sign encode, the low-rank encode and a stream copy of x, and the "
                   "estimate of 10 records beside 10 accumulating low-rank decodes; device events, us per call "
                   "(median, range of the repeats); inputs as the previous call left them in the caches",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls,
           "sizes": [part(codec, _lib, dev, n, a.repeats, a.calls) for n in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
