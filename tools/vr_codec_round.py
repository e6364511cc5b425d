"""A variance-reduced server's round with compressed gradients, timed three ways (one JSON line; DESIGN.md quotes it
from profiles/vr_codec_round.json): 10 messages at configs[0]'s model (417,482 parameters), everything device-resident,
the gradients through the stacked pipeline (K = D/100, 10 levels, philox).

  a  dense gradients: aggregation.avg_parameters_and_gradients (flc_avg_and_gradients) — the uncompressed round
  b  the records without the fused kernel: every record decoded densely (flc_stacked_decode_tiled), then a
  c  the fused path: avg_parameters_and_gradients on the records (flc_avg_and_gradient_records)

Each repeat draws fresh gradients and encodes fresh records (outside the timed windows), then times `--calls` calls of
each leg, the legs in rotating order, a host clock around work that ends in a device synchronise.  Reported per leg:
the median over the repeats and their spread (min, max), microseconds per call.  On a tree without the fused entry
point (an older revision, for its own figure of a) c is null."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fl_sim_amd import aggregation as agg  # noqa: E402
from fl_sim_amd import codec, compressed  # noqa: E402

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_MSGS, LEVELS = 10, 10


def cut(flat):
    out, off = [], 0
    for s in SHAPES:
        m = torch.Size(s).numel()
        out.append(flat[off:off + m].view(s))
        off += m
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    K = D // 100
    g = torch.Generator(device=dev).manual_seed(1)
    theta = cut(torch.randn(D, generator=g, device=dev))
    psrc = [cut(torch.randn(D, generator=g, device=dev)) for _ in range(N_MSGS)]
    ts = [100 * (i + 1) + 7 * (i % 3) for i in range(N_MSGS)]
    stride, _ = codec.stacked_wire_layout(D, K)
    fused = hasattr(compressed, "fold_gradient_records")
    times = {"a": [], "b": [], "c": []}
    for rep in range(a.repeats):
        flats = [torch.randn(D, generator=g, device=dev) * 1e-3 for _ in range(N_MSGS)]
        recs = torch.empty(N_MSGS, stride, dtype=torch.uint8, device=dev)
        for i, f in enumerate(flats):
            codec.stacked_encode(f, K, LEVELS, seed=1000 * rep + i, counter=rep, wire=recs[i])
        pks = [codec.wire_packet(recs[i], D, K, LEVELS) for i in range(N_MSGS)]
        dense = [{"parameters": psrc[i], "gradients": cut(flats[i]), "train_samples": ts[i]} for i in range(N_MSGS)]
        rmsgs = [{"parameters": psrc[i], "train_samples": ts[i],
                  "gradients": compressed.CompressedDelta(SHAPES, dev, D, record=recs[i], k=K, levels=LEVELS)}
                 for i in range(N_MSGS)]

        def leg_a():
            agg.avg_parameters_and_gradients(theta, dense)

        def leg_b():
            agg.avg_parameters_and_gradients(
                theta, [{"parameters": psrc[i], "gradients": cut(codec.stacked_decode(pks[i])), "train_samples": ts[i]}
                        for i in range(N_MSGS)])

        def leg_c():
            agg.avg_parameters_and_gradients(theta, rmsgs)
            assert rmsgs[0]["gradients"]._flat is None  # (the records were not decoded densely)

        legs = [("a", leg_a), ("b", leg_b)] + ([("c", leg_c)] if fused else [])
        legs = legs[rep % len(legs):] + legs[:rep % len(legs)]
        for name, fn in legs:
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6 / a.calls)
    if fused:  # faster and different is not faster: the two record paths on the last repeat's inputs, bit for bit
        t1, t2 = [t.clone() for t in theta], [t.clone() for t in theta]
        g1 = agg.avg_parameters_and_gradients(t1, rmsgs)
        g2 = agg.avg_parameters_and_gradients(
            t2, [{"parameters": psrc[i], "gradients": cut(codec.stacked_decode(pks[i])), "train_samples": ts[i]}
                 for i in range(N_MSGS)])
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(t1 + g1, t2 + g2))
        assert same, "the fused path and the composition differ"

    def summary(v):
        return None if not v else {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                                   "max_us": round(max(v), 2)}

    print(json.dumps({"what": "vr round, compressed gradients: 10 messages x 417,482 parameters, K = D/100, 10 levels",
                      "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls,
                      "a_dense_avg_and_gradients": summary(times["a"]),
                      "b_decode_then_avg_and_gradients": summary(times["b"]),
                      "c_fused_records": summary(times["c"]), "fused_equals_composition": bool(fused) or None,
                      "record_bytes": stride, "dense_gradient_bytes": 4 * D}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
