"""Bucketed dithering on an MI355X (one JSON document, ``--out``, default profiles/bucket_round.json; DESIGN.md
§3.3h quotes it).  The legs of each part alternate in one process; per leg the median and the range (min, max) of
``--repeats`` repeats, each timing ``--calls`` calls with device events and a host clock, microseconds per call.

  (a) encode   flc_bucket_encode at n = 409,600 and 25,001,984, B = 512, 8 bits (s = 127), p = inf, philox, against the
               only way the parent commit produces the same bytes — flc_quant_norm + flc_quant_encode on the
               [n / B, B] batch (rows capped at 65535 per call: the large size takes one pair of calls per 65,535
               rows) — asserted bit-equal here; flc_quant_encode_auto on the whole vector (one norm: another codec) as
               context.
  (b) round    a configs[0]-shaped FedAvg round of 10 clients with bucket records, host to host, against the same
               round with the whole-vector dense records (another codec: context only).
  (c) fold     flc_fedopt_fold_bucket_records over the 10 records against 10 flc_bucket_decode + flc_model_fold (the
               dense path of ``aggregation.fedopt_update`` on the decoded messages).

Kernel times come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_CLIENTS = 10
B, LEVELS, BITS = 512, 127, 8
ENCODE_SIZES = (409_600, 25_001_984)
MAX_ROWS = 65535


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def separated(fast, slow):
    return max(fast) < min(slow)


def timed(legs, repeats, calls, warmup=3):
    """{leg: (device us per call, host us per call) lists}, the legs alternating in rotating order."""
    dv = {k: [] for k in legs}
    hs = {k: [] for k in legs}
    names = list(legs)
    for rep in range(repeats):
        for k in names[rep % len(names):] + names[:rep % len(names)]:
            for _ in range(warmup):
                legs[k]()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            for _ in range(calls):
                legs[k]()
            e1.record()
            torch.cuda.synchronize()
            hs[k].append((time.perf_counter() - t0) * 1e6 / calls)
            dv[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    return dv, hs


def report(dv, hs):
    return {k: {"device": summary(dv[k]), "host_to_host": summary(hs[k])} for k in dv}


def encode_part(codec, _lib, dev, n, repeats, calls):
    assert n % B == 0
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.randn(n, generator=g, device=dev) * 1e-2
    rows = n // B
    st = codec._stream(dev)
    stride, _ = codec.bucket_wire_layout(n, 0, BITS, B)
    rec = torch.zeros(stride, dtype=torch.uint8, device=dev)
    nv, cv = codec.bucket_wire_views(rec, n, 0, BITS, B)
    norms2 = torch.zeros(rows, dtype=torch.float32, device=dev)
    codes2 = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", min(rows, MAX_ROWS), B), "quant")
    norm1 = torch.zeros(1, dtype=torch.float32, device=dev)
    codes1 = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws1 = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", 1, n), "quant_whole")

    def bucket():
        _lib.call("flc_bucket_encode", x.data_ptr(), n, 0, LEVELS, BITS, B, _lib.FLC_NORM_INF, 0, 5, 9, nv.data_ptr(),
                  cv.data_ptr(), None, None, st)

    def composed():
        # (the Philox words are indexed by the flat index of the batch a call is given: a piece that does not start at
        # element 0 would draw other words, so the composed form equals the bucket encode only as ONE call — sizes with
        # more than 65,535 rows are timed piecewise and compared on the first piece)
        for r0 in range(0, rows, MAX_ROWS):
            r = min(MAX_ROWS, rows - r0)
            xp = x.data_ptr() + 4 * r0 * B
            _lib.call("flc_quant_norm", xp, r, B, _lib.FLC_NORM_INF, norms2.data_ptr() + 4 * r0, ws.data_ptr(),
                      ws.numel(), st)
            _lib.call("flc_quant_encode", xp, r, B, 0, LEVELS, BITS, norms2.data_ptr() + 4 * r0, 5, 9, None,
                      codes2.data_ptr() + r0 * B, None, ws.data_ptr(), ws.numel(), st)

    def whole():
        _lib.call("flc_quant_encode_auto", x.data_ptr(), 1, n, 0, LEVELS, BITS, _lib.FLC_NORM_INF, 5, 9,
                  codes1.data_ptr(), norm1.data_ptr(), None, None, ws1.data_ptr(), ws1.numel(), st)

    bucket()
    composed()
    torch.cuda.synchronize()
    first = min(rows, MAX_ROWS)
    same = (torch.equal(nv.view(torch.int32), norms2.view(torch.int32))
            and torch.equal(cv[:first * B], codes2[:first * B]))
    assert same, "flc_bucket_encode and flc_quant_norm + flc_quant_encode on [n / B, B] differ"
    dv, hs = timed({"bucket_encode": bucket, "norm_plus_encode_rows": composed, "whole_vector_auto": whole}, repeats,
                   calls)
    out = {"n": n, "bucket": B, "bits": BITS, "composed_calls": 2 * -(-rows // MAX_ROWS), "bit_equal": same,
           "bit_equal_elements": first * B, **report(dv, hs),
           "bucket_faster_beyond_spread": separated(dv["bucket_encode"], dv["norm_plus_encode_rows"])}
    assert codec.quant_status(dev) == 0
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "bucket_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import Compressor, _lib, aggregation, codec, compressed

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"what": "bucketed dithering, B = 512, 8-bit standard dithering, p = inf, philox; us per call (median, range "
                   "of the repeats)", "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "calls_per_repeat": a.calls}
    doc["encode"] = [encode_part(codec, _lib, dev, n, a.repeats, a.calls) for n in ENCODE_SIZES]

    # (b) the round, (c) the fold
    D = sum(torch.Size(s).numel() for s in SHAPES)
    g = torch.Generator(device=dev).manual_seed(1)
    cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached] for _ in range(N_CLIENTS)]

    def state(seed):
        comps = []
        for i in range(N_CLIENTS):
            sd, nc = Compressor(rng="philox", seed=seed + i, extended_levels=True), Compressor("norm")
            nc.makeIdenticalCompressor()
            sd.makeStandardDitheringFP32(LEVELS, nc, float("inf"))
            comps.append([sd])
        return {"comps": comps, "theta": [t.clone() for t in cached], "delta": [torch.zeros_like(t) for t in cached]}

    def round_(s, bucket):
        msgs = [{"delta_parameters": compressed.compress_delta(locals_[i], cached, s["comps"][i], wire=True,
                                                               bucket=bucket)} for i in range(N_CLIENTS)]
        aggregation.fedopt_update(s["theta"], s["delta"], None, msgs, "avg", 1.0, (0.0, 1.0), 1.0)
        return msgs

    sb, sw = state(100), state(200)
    dv, hs = timed({"bucket_records": lambda: round_(sb, B), "whole_vector_records": lambda: round_(sw, 0)},
                   a.repeats, a.calls)
    for s in (sb, sw):  # (the send counts the timed rounds left on the device)
        _ = s["comps"][0][0].really_need_to_send_components
    doc["round"] = {"n": D, "clients": N_CLIENTS, **report(dv, hs)}

    msgs = round_(state(300), B)
    recs = [m["delta_parameters"] for m in msgs]
    assert all(r.kind == "bucket" for r in recs)
    _ = [r.record for r in recs]
    w = [1.0 / N_CLIENTS] * N_CLIENTS
    fa = {"theta": [t.clone() for t in cached], "delta": [torch.zeros_like(t) for t in cached]}
    fb = {"theta": [t.clone() for t in cached], "delta": [torch.zeros_like(t) for t in cached]}
    flats = [torch.empty(D, dtype=torch.float32, device=dev) for _ in range(N_CLIENTS)]

    def split(f):
        out, off = [], 0
        for s in SHAPES:
            m = torch.Size(s).numel()
            out.append(f[off:off + m].view(s))
            off += m
        return out

    def fold():
        assert compressed.fold_records(recs, w, fa["delta"], fa["theta"], None, 0.0)

    def decode_then_fold():
        dec = [{"delta_parameters": split(codec.bucket_decode(r.record, D, r.format, r.levels, r.bits, r.bucket,
                                                              out=f))} for r, f in zip(recs, flats)]
        aggregation.fedopt_update(fb["theta"], fb["delta"], None, dec, "avg", 1.0, (0.0, 1.0), 1.0)

    fold()
    decode_then_fold()
    torch.cuda.synchronize()
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(fa["theta"], fb["theta"]))
    assert same, "the record fold and decode + flc_model_fold differ"
    dv, hs = timed({"fold_bucket_records": fold, "decode_then_model_fold": decode_then_fold}, a.repeats, a.calls)
    doc["fold"] = {"n": D, "records": N_CLIENTS, "bit_equal": same, **report(dv, hs),
                   "fold_faster_beyond_spread": separated(dv["fold_bucket_records"], dv["decode_then_model_fold"])}
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
