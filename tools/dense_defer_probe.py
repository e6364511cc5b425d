"""A FedAvg round whose clients send dense records, with each message encoded when it is made and with the round's
messages deferred to one batched encode (one JSON document, ``--out``, default profiles/dense_record_defer.json;
DESIGN.md §3.3c quotes it).  configs[0]'s round as tools/dense_record_probe.py runs it: 10 clients × 417,482
parameters, standard dithering p = ∞, philox, ``wire_records`` on, everything device-resident, at 8-bit codes
(s = 127) and 4-bit codes (s = 7).  A round is the 10 ``communicate``-time ``compress_delta`` calls and the server's
``fedopt_update`` (FedAvg: optimizer "avg", lr 1, betas (0, 1)), whose record fold reads the records — the deferred
leg's batch runs there.

  immediate  ``compressed.DEFER_ENCODE`` False: per message a flatten, a memset of the count slot and its own
             flc_quant_encode_auto (the behaviour before dense deferral existed)
  deferred   ``compressed.DEFER_ENCODE`` True: per message a flatten; one flc_quant_encode_round for the round

The legs are interleaved in one process, each repeated ``--repeats`` times in rotating order; a repeat times
``--calls`` rounds with a host clock (host to host, ending in a device synchronise) and with a pair of device events
around the same rounds.  Reported per leg: the median over the repeats and their spread (min, max), microseconds per
round.  Both legs must give θ bit for bit.

``encode``: the encode alone at larger messages — ``n_msgs`` flc_quant_encode_auto calls against one
flc_quant_encode_round on the same vectors, device events and host clock per round of messages — up to n = 25 M with 8
messages, where a message is far past fixed latency and batching is not expected to help."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_CLIENTS = 10
SETTINGS = {"std8_s127": 127, "std4_s7": 7}
ENCODE_POINTS = ((417_482, 10), (1_000_000, 10), (2_000_000, 10), (4_000_000, 8), (16_000_000, 8), (25_000_000, 8))


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def separated(fast, slow):
    """The faster leg's whole range lies below the slower leg's (their min-max ranges do not overlap)."""
    return max(fast) < min(slow)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--encode-calls", type=int, default=12)
    ap.add_argument("--no-encode-points", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "dense_record_defer.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import Compressor, aggregation, codec, compressed

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5 and a.calls >= 50
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    g = torch.Generator(device=dev).manual_seed(1)
    cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached] for _ in range(N_CLIENTS)]

    def make(levels, seed):
        out = []
        for i in range(N_CLIENTS):
            sd, nc = Compressor(rng="philox", seed=seed + i, extended_levels=True), Compressor("norm")
            nc.makeIdenticalCompressor()
            sd.makeStandardDitheringFP32(levels, nc, float("inf"))
            out.append([sd])
        return out

    def state(levels, seed):
        return {"comps": make(levels, seed), "theta": [t.clone() for t in cached],
                "delta": [torch.zeros_like(t) for t in cached]}

    def round_(s, defer):
        compressed.DEFER_ENCODE = defer
        msgs = [{"delta_parameters": compressed.compress_delta(locals_[i], cached, s["comps"][i], wire=True)}
                for i in range(N_CLIENTS)]
        aggregation.fedopt_update(s["theta"], s["delta"], None, msgs, "avg", 1.0, (0.0, 1.0), 1.0)
        return msgs

    doc = {"what": "FedAvg round, 10 clients x 417,482 parameters, standard dithering p = inf, philox, wire_records "
                   "on; immediate: DEFER_ENCODE False, deferred: DEFER_ENCODE True; us per round",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls, "n": D,
           "parent_commit_round_us": 381, "settings": {}}
    for name, levels in SETTINGS.items():
        legs = {"immediate": False, "deferred": True}
        states = {k: state(levels, 100 * (j + 1)) for j, k in enumerate(legs)}
        host = {k: [] for k in legs}
        devt = {k: [] for k in legs}
        compressed.deferred_dense_stats(reset=True)
        for rep in range(a.repeats):
            order = list(legs)[rep % 2:] + list(legs)[:rep % 2]
            for k in order:
                s = states[k]
                for _ in range(a.warmup):
                    round_(s, legs[k])
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.calls):
                    round_(s, legs[k])
                e1.record()
                torch.cuda.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e6 / a.calls)
                devt[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        for s in states.values():  # (the send counts the timed rounds left on the device)
            _ = s["comps"][0][0].really_need_to_send_components
        batches = compressed.deferred_dense_stats(reset=True)
        rounds = a.repeats * (a.warmup + a.calls)  # one batch per deferred round (a round in which the compressors'
        # 64-slot count slabs fill up is split: each read-back runs the messages waiting so far)
        assert batches["messages"] == N_CLIENTS * rounds and rounds <= batches["batches"] < 1.2 * rounds, batches
        # the two legs compute the same round: identically seeded compressors, three rounds each, bit for bit
        sa, sb = state(levels, 7), state(levels, 7)
        for _ in range(3):
            round_(sa, False)
            round_(sb, True)
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(sa["theta"], sb["theta"]))
        same = same and all(x[0].really_need_to_send_components == y[0].really_need_to_send_components
                            and x[0].philox.counter == y[0].philox.counter for x, y in zip(sa["comps"], sb["comps"]))
        assert same, "the deferred round and the immediate round differ"
        doc["settings"][name] = {
            "levels": levels, "bits": codec.code_bits(levels),
            "immediate": {"host_to_host": summary(host["immediate"]), "device": summary(devt["immediate"])},
            "deferred": {"host_to_host": summary(host["deferred"]), "device": summary(devt["deferred"])},
            "deferred_faster_beyond_spread": {"host_to_host": separated(host["deferred"], host["immediate"]),
                                              "device": separated(devt["deferred"], devt["immediate"])},
            "same_round": same}
    compressed.DEFER_ENCODE = True
    if not a.no_encode_points:
        doc["encode"] = [encode_point(codec, dev, n, m, levels, a.encode_calls)
                         for n, m in ENCODE_POINTS for levels in (127, 7)]
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


def encode_point(codec, dev, n, n_msgs, levels, calls):
    """``n_msgs`` flc_quant_encode_auto calls (each with its count slot's memset) against one flc_quant_encode_round."""
    from fl_sim_amd import _lib

    bits = codec.code_bits(levels)
    stride, off = codec.dense_wire_layout(n, 0, bits)
    g = torch.Generator(device=dev).manual_seed(3)
    xs = [torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(n_msgs)]
    recs = {k: torch.empty(n_msgs, stride, dtype=torch.uint8, device=dev) for k in ("each", "round")}
    cnts = {k: torch.zeros(n_msgs, dtype=torch.int64, device=dev) for k in ("each", "round")}
    seeds, ctrs = list(range(5, 5 + n_msgs)), list(range(n_msgs))
    st = codec._stream(dev)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", 1, n), "quant")
    views = [codec.dense_wire_views(recs["each"][c], n, 0, bits) for c in range(n_msgs)]

    def each():
        for c in range(n_msgs):
            norm, codes = views[c]
            _lib.call("flc_quant_encode_auto", xs[c].data_ptr(), 1, n, 0, levels, bits, _lib.FLC_NORM_INF, seeds[c],
                      ctrs[c], codes.data_ptr(), norm.data_ptr(), cnts["each"][c:c + 1].data_ptr(), None,
                      ws.data_ptr(), ws.numel(), st)

    def round_():
        codec.quant_encode_round(xs, 0, levels, bits, _lib.FLC_NORM_INF, seeds, ctrs, recs["round"], cnts["round"])

    out = {"n": n, "messages": n_msgs, "levels": levels, "bits": bits, "calls": calls}
    times = {}
    for name, fn in (("per_message", each), ("round", round_)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        dv, hs = [], []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            hs.append((time.perf_counter() - t0) * 1e6)
            dv.append(e0.elapsed_time(e1) * 1e3)
        times[name] = dv
        out[name] = {"device": summary(dv), "host_to_host": summary(hs)}
    cb = (n * bits + 7) // 8
    fields = ((off["norm"], off["norm"] + 4), (off["codes"], off["codes"] + cb))
    same = (all(torch.equal(recs["each"][:, lo:hi], recs["round"][:, lo:hi]) for lo, hi in fields)
            and torch.equal(cnts["each"], cnts["round"]))
    assert same, "the batched records and the per-message records differ"
    out["same_records"] = same
    out["round_faster_beyond_spread"] = separated(times["round"], times["per_message"])
    out["round_slower_beyond_spread"] = separated(times["per_message"], times["round"])
    assert codec.quant_status(dev) == 0
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.exit(main())
