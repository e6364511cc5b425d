"""The client side of a compressed FedOpt round with and without error feedback, timed three ways (one JSON line;
DESIGN.md §3.4b quotes it from profiles/ef_round.json): configs[0]'s round — 10 clients × 417,482 parameters, the
stacked pipeline (K = D/100, 10 levels), philox, deferred batched encode, everything device-resident.  A round is the
10 ``communicate``-time calls plus the first access to a record (which runs the round's batched encode).

  a  feedback off: compress_delta(local, cached, compressors)
  b  feedback on: compress_delta(..., feedback=ErrorMemory) — the memory is the encoder's flat input, one
     flc_ef_residual_round launch after the batched encode
  c  feedback hand-built from the public pieces, as a user would without the feature: a = e + cat(local − cached) in
     torch, compress_tensors([a], compressors), c = CompressedDelta.flat() (a dense decode, and the client's encode at
     communicate time: the residual needs the record there), e = a − c

Each repeat times ``--calls`` rounds of each leg, the legs in rotating order inside one process, a host clock around
work that ends in a device synchronise.  Reported per leg: the median over the repeats and their spread (min, max),
microseconds per round.  ``--legs a --tree PATH`` runs leg a on another checkout's package and library (the parent
commit's, for the no-regression reading; a tree without fl_sim_amd.feedback has only leg a).  ``--residual-gib``
times flc_ef_residual_round alone on one headline-sized record (1 GiB of fp32, K = n/100) with device events."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_CLIENTS, LEVELS = 10, 10


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--residual-gib", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    from fl_sim_amd import Compressor, codec, compressed

    try:
        from fl_sim_amd.feedback import ErrorMemory
    except ImportError:
        ErrorMemory = None
    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.residual_gib:
        return residual_gib(codec, dev)
    legs = [x for x in a.legs.split(",") if x]
    if ErrorMemory is None:
        assert legs == ["a"], "this tree has no error feedback: leg a only"
    D = sum(torch.Size(s).numel() for s in SHAPES)
    K = D // 100
    g = torch.Generator(device=dev).manual_seed(1)
    cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached] for _ in range(N_CLIENTS)]

    def make(seed):
        out = []
        for i in range(N_CLIENTS):
            tk, sd, nc = Compressor(rng="philox", seed=seed + i), Compressor(rng="philox", seed=seed + i), \
                Compressor("norm")
            tk.makeTopKCompressor(K, D)
            nc.makeIdenticalCompressor()
            sd.makeStandardDitheringFP32(LEVELS, nc, float("inf"))
            out.append([tk, sd])
        return out

    def state(seed):
        return {"comps": make(seed), "mems": None if ErrorMemory is None else [ErrorMemory(D, dev)
                                                                                for _ in range(N_CLIENTS)],
                "hand": [torch.zeros(D, device=dev) for _ in range(N_CLIENTS)]}

    def leg_a(s):
        ds = [compressed.compress_delta(locals_[i], cached, s["comps"][i]) for i in range(N_CLIENTS)]
        ds[0].record
        return ds

    def leg_b(s):
        ds = [compressed.compress_delta(locals_[i], cached, s["comps"][i], feedback=s["mems"][i])
              for i in range(N_CLIENTS)]
        ds[0].record
        return ds

    def leg_c(s):
        ds = []
        for i in range(N_CLIENTS):
            x = torch.cat([(lo - c).reshape(-1) for lo, c in zip(locals_[i], cached)])
            acc = s["hand"][i] + x
            d = compressed.compress_tensors([acc], s["comps"][i])
            s["hand"][i] = acc - d.flat()
            ds.append(d)
        return ds

    fns = {"a": leg_a, "b": leg_b, "c": leg_c}
    states = {name: state(100 * (j + 1)) for j, name in enumerate(legs)}
    times = {name: [] for name in legs}
    compressed.deferred_stats(reset=True)
    for rep in range(a.repeats):
        order = legs[rep % len(legs):] + legs[:rep % len(legs)]
        for name in order:
            fn, s = fns[name], states[name]
            for _ in range(a.warmup):
                fn(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                fn(s)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6 / a.calls)
    for s in states.values():  # (the send counts the timed rounds left on the device)
        _ = s["comps"][0][1].really_need_to_send_components
    same = None
    if "b" in legs and "c" in legs:  # faster and different is not faster: two rounds from zero memories, bit for bit
        sb, sc = state(7), state(7)
        same = True
        for _ in range(2):
            rb, rc = leg_b(sb), leg_c(sc)
            for x, y in zip(rb, rc):
                same = same and torch.equal(x.flat().view(torch.int32), y.flat().view(torch.int32))
        for m, h in zip(sb["mems"], sc["hand"]):
            same = same and torch.equal(m.value().view(torch.int32), h.view(torch.int32))
        assert same, "the built-in feedback and the hand-built one differ"

    def summary(v):
        return None if not v else {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                                   "max_us": round(max(v), 2)}

    print(json.dumps({"what": "client side of a compressed FedOpt round: 10 clients x 417,482 parameters, K = D/100, "
                              "10 levels, philox, deferred",
                      "tree": a.label, "device": torch.cuda.get_device_name(0), "repeats": a.repeats,
                      "calls_per_repeat": a.calls,
                      "a_feedback_off": summary(times.get("a")), "b_feedback_on": summary(times.get("b")),
                      "c_feedback_by_hand": summary(times.get("c")), "b_equals_c": same}))
    return 0


def residual_gib(codec, dev) -> int:
    """flc_ef_residual_round on one record of a 1 GiB vector (n = 2^28, K = n/100 ≈ 2.7 M scattered 4-B updates)."""
    n = 1 << 28
    k = n // 100
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn(n, generator=g, device=dev) * 1e-2
    stride, _ = codec.stacked_wire_layout(n, k)
    rec = torch.empty(stride, dtype=torch.uint8, device=dev)
    codec.stacked_encode(x, k, LEVELS, seed=3, counter=0, wire=rec)
    e = x  # (the memory holds a)
    for _ in range(3):
        codec.ef_residual_round([rec], [e], n, k, LEVELS)
    torch.cuda.synchronize()
    ts = []
    for _ in range(20):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        codec.ef_residual_round([rec], [e], n, k, LEVELS)
        t1.record()
        t1.synchronize()
        ts.append(t0.elapsed_time(t1) * 1e3)
    print(json.dumps({"what": "flc_ef_residual_round, one record of a 1 GiB vector (device events around one call)",
                      "device": torch.cuda.get_device_name(0), "n": n, "k": k, "calls": len(ts),
                      "median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
                      "max_us": round(max(ts), 2), "dense_pass_bytes": 12 * n, "residual_bytes": 13 * k}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
