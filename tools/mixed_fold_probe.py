"""The server update of a round whose clients chose different codecs, with the mixed one-pass fold off and on (one JSON
document, ``--out``, default profiles/mixed_fold_round.json; DESIGN.md §3.3f quotes it).  Device-resident FedAvg server
(optimizer "avg", lr 1, betas (0, 1)), philox mode, the records encoded before anything is timed; only
``aggregation.fedopt_update`` is timed.

  shape 1  configs[0]: 417,482 parameters in 8 tensors, 10 clients — five 8-bit (s = 127) and five 4-bit (s = 7)
           standard dithering records, in two orders: ``grouped`` (8, 8, 8, 8, 8, 4, 4, 4, 4, 4: two runs) and
           ``alternating`` (8, 4, 8, 4, ...: ten runs of one record)
  shape 2  25,000,000 parameters in one tensor, 8 records: four stacked (K = 1 %, 127 levels) and four 8-bit

  a  switch off: record_round declines the round, every message decodes itself (one launch and 4·n bytes written per
     message) and flc_model_fold reads the decoded vectors — what runs without FLC_MIXED_FOLD=1
  b  switch on: flc_fedopt_fold_mixed_records reads the messages as they are
  c  the ceiling: a uniform 8-bit round of as many records through flc_fedopt_fold_dense_records

A message keeps its decoded vector once it has decoded itself, so before every update of every leg the messages'
decoded vectors are dropped (two attribute stores per message): each update of leg a decodes again, as each round's
new messages would.  The legs alternate in one process, ``--repeats`` times in rotating order after a warm-up of the
shape; a repeat times ``--calls`` updates with the host clock (ending in a device synchronise) and with a pair of device
events around the same updates.  Reported per leg: the median over the repeats (min-max), microseconds per update.
Legs a and b are asserted bit-equal from one fresh server state.

``--root DIR`` imports the package from another checkout (with its built libraries) and ``--legs a`` runs one leg: the
switch-off path on the parent commit, for its own run-to-run spread."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main() -> int:
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--legs", default="a,b,c")
    ap.add_argument("--root", default=here)
    ap.add_argument("--out", default=os.path.join(here, "profiles", "mixed_fold_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from fl_sim_amd import Compressor, aggregation, compressed

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5 and a.calls >= 200
    legs = [x for x in a.legs.split(",") if x]
    assert set(legs) <= {"a", "b", "c"}
    assert "b" not in legs or hasattr(compressed, "MIXED_FOLD"), "this checkout has no mixed fold"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def dither(levels, seed):
        sd, nc = Compressor(rng="philox", seed=seed, extended_levels=True), Compressor("norm")
        nc.makeIdenticalCompressor()
        sd.makeStandardDitheringFP32(levels, nc, float("inf"))
        return [sd]

    def stacked(k, n, seed):
        tk = Compressor(rng="philox", seed=seed)
        tk.makeTopKCompressor(k, n)
        return [tk] + dither(127, seed + 1)

    def messages(shapes, codecs):
        """One pre-encoded message per entry of ``codecs`` ("std8", "std4", "stk1"), and the cached model."""
        g = torch.Generator(device=dev).manual_seed(1)
        n = sum(torch.Size(s).numel() for s in shapes)
        cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in shapes]
        msgs = []
        for i, name in enumerate(codecs):
            local = [t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached]
            comps = stacked(n // 100, n, 50 + 2 * i) if name == "stk1" else dither(127 if name == "std8" else 7, 50 + 2 * i)
            d = compressed.compress_delta(local, cached, comps, wire=True)
            assert d.record is not None and d.kind in ("quant", "stacked")
            msgs.append({"delta_parameters": d})
            del local
        torch.cuda.synchronize()
        return cached, msgs

    def state(cached):
        return {"theta": [t.clone() for t in cached], "delta": [torch.zeros_like(t) for t in cached]}

    def update(s, msgs, on):
        if hasattr(compressed, "MIXED_FOLD"):
            compressed.MIXED_FOLD = on
        for m in msgs:  # (a message that decoded itself keeps the vector: every update starts from the records)
            d = m["delta_parameters"]
            d._flat = d._views = None
        aggregation.fedopt_update(s["theta"], s["delta"], None, msgs, "avg", 1.0, (0.0, 1.0), 1.0)

    def measure(cached, rounds):
        """rounds: leg -> (messages, switch); the legs alternated, (host, device) microseconds per update."""
        states = {k: state(cached) for k in rounds}
        host = {k: [] for k in rounds}
        devt = {k: [] for k in rounds}
        for k, (msgs, on) in rounds.items():
            for _ in range(a.warmup):
                update(states[k], msgs, on)
        torch.cuda.synchronize()
        names = list(rounds)
        for rep in range(a.repeats):
            r = rep % len(names)
            for k in names[r:] + names[:r]:
                msgs, on = rounds[k]
                for _ in range(3):
                    update(states[k], msgs, on)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(a.calls):
                    update(states[k], msgs, on)
                e1.record()
                torch.cuda.synchronize()
                host[k].append((time.perf_counter() - t0) * 1e6 / a.calls)
                devt[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        return {k: {"host_to_host": summary(host[k]), "device": summary(devt[k])} for k in rounds}

    def same_round(cached, msgs):
        sa, sb = state(cached), state(cached)
        update(sa, msgs, False)
        update(sb, msgs, True)
        torch.cuda.synchronize()
        same = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                   for x, y in zip(sa["theta"] + sa["delta"], sb["theta"] + sb["delta"]))
        assert same, "the mixed fold and the per-message path differ"
        return same

    doc = {"what": "server update (fedopt_update, FedAvg) of a round of differing codecs; a switch off (every message "
                   "decodes itself), b switch on (flc_fedopt_fold_mixed_records), c a uniform 8-bit round through "
                   "flc_fedopt_fold_dense_records; us per update, median (min, max) over the repeats",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls,
           "legs": legs, "root": "this checkout" if os.path.abspath(a.root) == here else "another checkout",
           "shapes": {}}
    plans = {
        "configs0_grouped": (SHAPES, ["std8"] * 5 + ["std4"] * 5),
        "configs0_alternating": (SHAPES, ["std8", "std4"] * 5),
        "25M_stacked_and_8bit": ([(25_000_000,)], ["stk1"] * 4 + ["std8"] * 4),
    }
    for name, (shapes, codecs) in plans.items():
        cached, mixed = messages(shapes, codecs)
        rounds = {}
        if "a" in legs:
            rounds["a_switch_off"] = (mixed, False)
        if "b" in legs:
            rounds["b_switch_on"] = (mixed, True)
        if "c" in legs:
            rounds["c_uniform_8bit"] = (messages(shapes, ["std8"] * len(codecs))[1], True)
        entry = {"n": sum(torch.Size(s).numel() for s in shapes), "records": codecs,
                 "message_bytes": [m["delta_parameters"].nbytes for m in mixed]}
        entry.update(measure(cached, rounds))
        if "a" in legs and "b" in legs:
            entry["a_and_b_bit_equal"] = same_round(cached, mixed)
            ra, rb = entry["a_switch_off"], entry["b_switch_on"]
            entry["b_range_below_a_range"] = {k: rb[k]["max_us"] < ra[k]["min_us"] for k in ("host_to_host", "device")}
            stats = compressed.mixed_fold_stats()
            assert stats["folds"] > 0
        doc["shapes"][name] = entry
        del cached, mixed, rounds
        torch.cuda.empty_cache()
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
