"""The scaled-sign encode on an MI355X (one JSON document, ``--out``, default profiles/sign_round.json; DESIGN.md
§3.3i quotes it): flc_sign_encode at B = 512 without ``out``, against flc_bucket_encode at 2 bits (s = 1, p = inf,
philox: the smallest code the project had), at n = 409,600 and 25,001,984.  The two legs alternate in one process; per
leg the median and the range of ``--repeats`` repeats, each timing ``--calls`` calls with device events, microseconds
per call.  A record, not a gate."""
import argparse
import json
import os
import statistics
import sys

import torch

B = 512
SIZES = (409_600, 25_001_984)


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
    x = torch.randn(n, generator=torch.Generator(device=dev).manual_seed(n), device=dev) * 1e-2
    st = codec._stream(dev)
    srec = torch.zeros(codec.sign_wire_layout(n, B)[0], dtype=torch.uint8, device=dev)
    sv, sb = codec.sign_wire_views(srec, n, B)
    brec = torch.zeros(codec.bucket_wire_layout(n, 0, 2, B)[0], dtype=torch.uint8, device=dev)
    nv, cv = codec.bucket_wire_views(brec, n, 0, 2, B)

    def sign():
        _lib.call("flc_sign_encode", x.data_ptr(), n, B, sv.data_ptr(), sb.data_ptr(), None, None, None, 0, st)

    def bucket2():
        _lib.call("flc_bucket_encode", x.data_ptr(), n, 0, 1, 2, B, _lib.FLC_NORM_INF, 0, 5, 9, nv.data_ptr(),
                  cv.data_ptr(), None, None, st)

    us = timed({"sign_encode": sign, "bucket_encode_2bit": bucket2}, repeats, calls)
    # the scales against torch's fp32 mean of |x| per bucket (a loose check that the timed call computed something)
    want = x.abs().view(-1, B).double().mean(1)
    assert torch.allclose(sv.double(), want, rtol=1e-6), "the timed encode's scales are off"
    out = {"n": n, "bucket": B, "algorithmic_bytes": {"sign_encode": n * (4 + 1 / 8 + 4 / B),
                                                      "bucket_encode_2bit": n * (4 + 1 / 4 + 4 / B)}}
    for k, v in us.items():
        out[k] = {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
    out["sign_slower_beyond_spread"] = min(us["sign_encode"]) > max(us["bucket_encode_2bit"])
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sign_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import _lib, codec

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"what": "flc_sign_encode (B = 512, no out) against flc_bucket_encode at 2 bits; device events, us per call "
                   "(median, range of the repeats)", "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
           "calls_per_repeat": a.calls, "encode": [part(codec, _lib, dev, n, a.repeats, a.calls) for n in SIZES]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
