"""A FedAvg round whose clients use the plain top-k compressor, with the sparse records off and on, the record fold
against the chain it replaces, and the round's batched encode against per-message encodes (one JSON document,
``--out``, default profiles/sparse_record_round.json; DESIGN.md §3.3d quotes it).  configs[0]'s round: 10 clients ×
417,482 parameters, K = n / 100, philox, everything device-resident.  A round is the 10 ``communicate``-time
``compress_delta`` calls and the server's ``fedopt_update`` (FedAvg: optimizer "avg", lr 1, betas (0, 1)).

  A  sparse off (the behaviour before the option existed): each message the decoded vector (a select, then a dense
     decode), the server's flc_model_fold
  B  sparse on: each message its record, the round's records written by one flc_topk_encode_batch, the server's
     flc_fedopt_fold_sparse_records

The legs are interleaved in one process, each repeated ``--repeats`` times in rotating order; a repeat times
``--calls`` rounds with a host clock (host to host, ending in a device synchronise) and with a pair of device events
around the same rounds (the device's time line from the first launch to the last).  Reported per leg: the median over
the repeats and their spread (min, max), microseconds per round, and the bytes a message carries.

``fold``: device events around flc_fedopt_fold_sparse_records alone, against the chain it replaces — every record
decoded with flc_sparse_decode_tiled into its own dense vector, then flc_model_fold with the step — at n = 417,482 with
10 records, each call on another of ``sets`` distinct record sets (and its own δ and θ) so that nothing is served from
the 256 MiB cache by the previous call.

``encode``: device events around one flc_topk_encode_batch of the 10 messages into a record block, against 10
flc_topk_encode_tiled calls into 10 records, the legs alternating."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_CLIENTS = 10


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fold-calls", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "sparse_record_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import Compressor, aggregation, codec, compressed

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    K = D // 100
    g = torch.Generator(device=dev).manual_seed(1)
    cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached] for _ in range(N_CLIENTS)]

    def make(seed):
        out = []
        for i in range(N_CLIENTS):
            tk = Compressor(rng="philox", seed=seed + i)
            tk.makeTopKCompressor(K, D)
            out.append([tk])
        return out

    def state(seed):
        return {"comps": make(seed), "theta": [t.clone() for t in cached],
                "delta": [torch.zeros_like(t) for t in cached]}

    def round_(s, sparse):
        msgs = [{"delta_parameters": compressed.compress_delta(locals_[i], cached, s["comps"][i], sparse=sparse)}
                for i in range(N_CLIENTS)]
        aggregation.fedopt_update(s["theta"], s["delta"], None, msgs, "avg", 1.0, (0.0, 1.0), 1.0)
        return msgs

    doc = {"what": "FedAvg round, 10 clients x 417,482 parameters, top-k 1 %, philox; A sparse records off, B on; "
                   "us per round",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls, "n": D, "k": K}
    legs = {"A": False, "B": True}
    states = {k: state(100 * (j + 1)) for j, k in enumerate(legs)}
    host = {k: [] for k in legs}
    devt = {k: [] for k in legs}
    nbytes = {}
    compressed.deferred_sparse_stats(reset=True)
    for rep in range(a.repeats):
        order = list(legs)[rep % 2:] + list(legs)[:rep % 2]
        for k in order:
            s = states[k]
            for _ in range(a.warmup):
                msgs = round_(s, legs[k])
            nbytes[k] = msgs[0]["delta_parameters"].nbytes
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
    st = compressed.deferred_sparse_stats()
    # the two legs compute the same round, bit for bit
    sa, sb = state(7), state(7)
    round_(sa, False)
    round_(sb, True)
    same = all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(sa["theta"], sb["theta"]))
    assert same, "the round with records and the round without differ"
    doc["round"] = {
        "A_sparse_off": {"host_to_host": summary(host["A"]), "device": summary(devt["A"]),
                         "message_bytes": nbytes["A"]},
        "B_sparse_on": {"host_to_host": summary(host["B"]), "device": summary(devt["B"]),
                        "message_bytes": nbytes["B"]},
        "batched_encodes_per_round_B": st["batches"] / max(1, st["messages"] // N_CLIENTS),
        "same_round": same}
    doc["fold"] = fold(codec, dev, D, K, N_CLIENTS, a.fold_calls, 16)
    doc["encode"] = encode(codec, dev, D, K, N_CLIENTS, a.fold_calls, a.repeats)
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


def fold(codec, dev, n, k, n_records, calls, sets):
    """flc_fedopt_fold_sparse_records (avg step) against decode-each-record + flc_model_fold, device events per call."""
    import ctypes

    from fl_sim_amd import _lib

    stride, _ = codec.sparse_wire_layout(n, k)
    g = torch.Generator(device=dev).manual_seed(3)
    recs = torch.empty(sets, n_records, stride, dtype=torch.uint8, device=dev)
    for si in range(sets):
        codec.topk_encode_records([torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(n_records)], k,
                                  recs[si])
    delta = [torch.zeros(n, device=dev) for _ in range(sets)]
    theta = [torch.zeros(n, device=dev) for _ in range(sets)]
    dense = [torch.empty(n, device=dev) for _ in range(n_records)]
    w = [1.0 / n_records] * n_records
    P = ctypes.c_void_p
    cw = (ctypes.c_float * n_records)(*w)
    one = (ctypes.c_int64 * 1)(n)
    st = codec._stream(dev)

    def fused(si):
        _lib.call("flc_fedopt_fold_sparse_records", (P * n_records)(*[recs[si, r].data_ptr() for r in range(n_records)]),
                  cw, n_records, n, k, (P * 1)(delta[si].data_ptr()), (P * 1)(theta[si].data_ptr()), None, one, 1, 0.0,
                  0, 1.0, 1.0, 1.0, st)

    def chain(si):
        for r in range(n_records):
            codec.sparse_record_decode(recs[si, r], n, k, out=dense[r])
        codec.model_fold([delta[si]], [[d] for d in dense], w, 0, 0.0, theta=[theta[si]], opt="avg", lr=1.0,
                         beta2=1.0, tau=1.0)

    out = {"n": n, "k": k, "records": n_records, "record_sets": sets, "calls": calls, "record_bytes": stride,
           "dense_bytes": 4 * n}
    for name, fn in (("fused", fused), ("chain", chain)):
        for i in range(sets):
            fn(i)
        torch.cuda.synchronize()
        ts = []
        for i in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(i % sets)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        out[name] = summary(ts)
    torch.cuda.synchronize()
    return out


def encode(codec, dev, n, k, n_msgs, calls, repeats):
    """One flc_topk_encode_batch of the round's messages against one flc_topk_encode_tiled per message: device events
    around ``calls`` rounds' worth, the two legs alternating, ``repeats`` times; us per round of messages."""
    stride, _ = codec.sparse_wire_layout(n, k)
    g = torch.Generator(device=dev).manual_seed(5)
    xs = [torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(n_msgs)]
    block = torch.empty(n_msgs, stride, dtype=torch.uint8, device=dev)
    single = [torch.empty(stride, dtype=torch.uint8, device=dev) for _ in range(n_msgs)]

    def batched():
        codec.topk_encode_records(xs, k, block)

    def per_message():
        for x, r in zip(xs, single):
            codec.topk_encode_record(x, k, r)

    legs = {"batched": batched, "per_message": per_message}
    ts = {name: [] for name in legs}
    for rep in range(repeats):
        order = list(legs)[rep % 2:] + list(legs)[:rep % 2]
        for name in order:
            fn = legs[name]
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32))  # (the three fields, not the padding)
               for c in range(n_msgs)
               for a, b in zip(codec.sparse_wire_views(block[c], n, k), codec.sparse_wire_views(single[c], n, k)))
    return {"n": n, "k": k, "messages": n_msgs, "calls_per_repeat": calls, "repeats": repeats,
            "batched": summary(ts["batched"]), "per_message": summary(ts["per_message"]), "same_records": same}


if __name__ == "__main__":
    sys.exit(main())
