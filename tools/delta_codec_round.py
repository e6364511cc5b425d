"""A SCAFFOLD server's round with compressed deltas, timed four ways (one JSON line; DESIGN.md quotes it from
profiles/delta_codec_round.json): 10 messages at configs[0]'s model (417,482 parameters), everything device-resident,
both deltas of every message through the stacked pipeline (K = D/100, 10 levels, philox).

  a  dense deltas: aggregation.scaffold_update on lists of tensors — the uncompressed round
  b  the records folded one destination at a time with the single-destination entry: flc_fedopt_fold_records with the
     destination as `delta`, beta0 = 1, theta = NULL, called twice (θ, then c)
  c  the grouped pass: aggregation.scaffold_update on the records (flc_fold_record_groups, θ and c in one launch);
     c_call is the bare C call, b's counterpart
  d  decode-then-fold: every record decoded densely (flc_stacked_decode_tiled), then a

Each repeat draws fresh deltas and encodes fresh records (outside the timed windows), then times `--calls` calls of
each leg, the legs in rotating order, a host clock around work that ends in a device synchronise.  Reported per leg:
the median over the repeats and their spread (min, max), microseconds per update.  On a tree without the grouped entry
point (an older revision, for its own figures of a and b) c is null.  `--only LEG` runs one leg (for a kernel trace)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fl_sim_amd import _lib  # noqa: E402
from fl_sim_amd import aggregation as agg  # noqa: E402
from fl_sim_amd import codec, compressed  # noqa: E402

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_MSGS, N_CLIENTS, LEVELS, LR = 10, 20, 10, 0.05
KEYS = ("parameters_delta", "control_variates_delta")
P = ctypes.c_void_p


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
    ap.add_argument("--only", choices=["a", "b", "c", "c_call", "d"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    K = D // 100
    g = torch.Generator(device=dev).manual_seed(1)
    theta, cvs = cut(torch.randn(D, generator=g, device=dev)), cut(torch.randn(D, generator=g, device=dev) * 1e-3)
    stride, _ = codec.stacked_wire_layout(D, K)
    grouped = hasattr(compressed, "fold_record_groups")
    T, m = len(SHAPES), N_MSGS
    sizes = (ctypes.c_int64 * T)(*[t.numel() for t in theta])
    ratio = (LR / N_MSGS, 1 / N_CLIENTS)
    times = {"a": [], "b": [], "c": [], "c_call": [], "d": []}
    for rep in range(a.repeats):
        flats = [[torch.randn(D, generator=g, device=dev) * 1e-3 for _ in range(N_MSGS)] for _ in KEYS]
        recs = torch.empty(2, N_MSGS, stride, dtype=torch.uint8, device=dev)
        for v in range(2):
            for i, f in enumerate(flats[v]):
                codec.stacked_encode(f, K, LEVELS, seed=1000 * rep + 100 * v + i, counter=rep, wire=recs[v, i])
        pks = [[codec.wire_packet(recs[v, i], D, K, LEVELS) for i in range(N_MSGS)] for v in range(2)]
        dense = [{KEYS[0]: cut(flats[0][i]), KEYS[1]: cut(flats[1][i])} for i in range(N_MSGS)]
        rmsgs = [{k: compressed.CompressedDelta(SHAPES, dev, D, record=recs[v, i], k=K, levels=LEVELS)
                  for v, k in enumerate(KEYS)} for i in range(N_MSGS)]
        st = codec._stream(dev)
        one = [((P * m)(*[recs[v, i].data_ptr() for i in range(m)]), (ctypes.c_float * m)(*[ratio[v]] * m),
                (P * T)(*[t.data_ptr() for t in (theta, cvs)[v]])) for v in range(2)]
        both = ((P * (2 * m))(*[recs[v, i].data_ptr() for v in range(2) for i in range(m)]),
                (ctypes.c_float * (2 * m))(*([ratio[0]] * m + [ratio[1]] * m)),
                (ctypes.c_int32 * (2 * m))(*([0] * m + [1] * m)),
                (P * (2 * T))(*[t.data_ptr() for t in theta + cvs]))

        def leg_a():
            agg.scaffold_update(theta, cvs, dense, LR, N_CLIENTS)

        def leg_b():
            for r, w, d in one:
                _lib.call("flc_fedopt_fold_records", r, w, m, D, K, LEVELS, d, None, None, sizes, T, 1.0, 0, 1.0, 0.0,
                          0.0, st)

        def leg_c():
            agg.scaffold_update(theta, cvs, rmsgs, LR, N_CLIENTS)
            assert rmsgs[0][KEYS[0]]._flat is None  # (the records were not decoded densely)

        def leg_c_call():
            _lib.call("flc_fold_record_groups", both[0], both[1], both[2], 2 * m, D, K, LEVELS, both[3], 2, sizes, T, st)

        def leg_d():
            agg.scaffold_update(theta, cvs, [{k: cut(codec.stacked_decode(pks[v][i])) for v, k in enumerate(KEYS)}
                                             for i in range(N_MSGS)], LR, N_CLIENTS)

        legs = [("a", leg_a), ("b", leg_b), ("d", leg_d)] + ([("c", leg_c), ("c_call", leg_c_call)] if grouped else [])
        if a.only is not None:
            legs = [x for x in legs if x[0] == a.only]
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
    same = None
    if grouped:  # faster and different is not faster: the record paths on the last repeat's inputs, bit for bit
        outs = []
        for fn in (leg_c, leg_d, leg_b, leg_c_call):
            saved = [t.clone() for t in theta + cvs]
            fn()
            torch.cuda.synchronize()
            outs.append([t.clone() for t in theta + cvs])
            for t, s in zip(theta + cvs, saved):
                t.copy_(s)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for o in outs[1:] for x, y in zip(outs[0], o))
        assert same, "the grouped pass, the per-destination folds and the composition differ"

    def summary(v):
        return None if not v else {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                                   "max_us": round(max(v), 2)}

    print(json.dumps({"what": "SCAFFOLD round, compressed deltas: 10 messages x 2 vectors x 417,482 parameters, "
                              "K = D/100, 10 levels",
                      "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls,
                      "a_dense_scaffold_update": summary(times["a"]),
                      "b_fedopt_fold_records_twice": summary(times["b"]),
                      "c_grouped_scaffold_update": summary(times["c"]),
                      "c_call_fold_record_groups": summary(times["c_call"]),
                      "d_decode_then_scaffold_update": summary(times["d"]), "record_paths_equal": same,
                      "record_bytes": stride, "dense_delta_bytes": 4 * D}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
