"""A FedProx round whose clients send their gradients as dense records (``wire_records`` on, plain standard dithering),
with the server decoding every record and with the one-pass record fold, and the fold against the chain it replaces
(one JSON document, ``--out``, default profiles/dense_gradient_round.json; DESIGN.md §3.3e quotes it).  configs[0]'s
round: 10 clients × 417,482 parameters, p = ∞, philox, everything device-resident, at two settings: 8-bit codes
(s = 127) and 4-bit codes (s = 7).  A round is the 10 ``communicate``-time ``compress_message_gradients`` calls (records
on in both legs) and the server's ``avg_parameters_and_gradients``.

  A  the server does not recognise the gradient round (the behaviour before flc_avg_and_gradient_dense_records: the
     probe makes ``compressed.record_round`` answer as it did then — stacked and sparse rounds only), so every record
     decodes itself into its own 4n-byte vector (one flc_quant_decode per message) and flc_avg_and_gradients follows
  B  the server folds the records: one flc_avg_and_gradient_dense_records pass

The legs are interleaved in one process, each repeated ``--repeats`` times in rotating order; a repeat times
``--calls`` rounds with a host clock (host to host, ending in a device synchronise) and with a pair of device events
around the same rounds (the device's time line from the first launch to the last).  Reported per leg: the median over
the repeats and their spread (min, max), microseconds per round.  The probe asserts that θ and ``.grad`` of the two legs
are bit-identical.

``fold``: device events around flc_avg_and_gradient_dense_records alone, against the chain it replaces — every record
decoded with flc_quant_decode into its own dense vector, then flc_avg_and_gradients — at n = 417,482 with 10 records and
at n = 25 M with 8 records, each call on another of ``sets`` distinct record sets (and its own θ and gradient buffer)
so that nothing is served from the 256 MiB cache by the previous call (at 25 M the record sets together hold 600 MB of
8-bit codes, 300 MB of 4-bit codes).  Both sides read the same dense parameter sources."""
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


def summary(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fold-calls", type=int, default=24)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "dense_gradient_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import Compressor, aggregation, codec, compressed

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 4
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    g = torch.Generator(device=dev).manual_seed(1)
    theta0 = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in theta0] for _ in range(N_CLIENTS)]
    grads_ = [[torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in theta0] for _ in range(N_CLIENTS)]

    def make(levels, seed):
        out = []
        for i in range(N_CLIENTS):
            sd, nc = Compressor(rng="philox", seed=seed + i, extended_levels=True), Compressor("norm")
            nc.makeIdenticalCompressor()
            sd.makeStandardDitheringFP32(levels, nc, float("inf"))
            out.append([sd])
        return out

    def state(levels, seed):
        return {"comps": make(levels, seed), "theta": [torch.nn.Parameter(t.clone()) for t in theta0]}

    recognise = compressed.record_round

    def before(messages, key="delta_parameters"):  # (record_round as it was: no dense gradient round)
        if key == "gradients":
            return compressed.stacked_round(messages, key) or compressed.sparse_round(messages, key)
        return recognise(messages, key)

    def round_(s, fold):
        msgs = []
        for i in range(N_CLIENTS):
            m = {"parameters": locals_[i], "gradients": grads_[i], "train_samples": 10 + i}
            compressed.compress_message_gradients(m, s["comps"][i], None, True)
            msgs.append(m)
        compressed.record_round = recognise if fold else before
        try:
            aggregation.avg_parameters_and_gradients(s["theta"], msgs, False, 0.0)
        finally:
            compressed.record_round = recognise
        return msgs

    doc = {"what": "FedProx round, 10 clients x 417,482 parameters, gradients as dense records (standard dithering "
                   "p = inf, philox, wire_records on); A the server decodes every record then flc_avg_and_gradients, "
                   "B flc_avg_and_gradient_dense_records; us per round",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls, "n": D,
           "settings": {}}
    for name, levels in SETTINGS.items():
        legs = {"A": False, "B": True}
        states = {k: state(levels, 100 * (j + 1)) for j, k in enumerate(legs)}
        host = {k: [] for k in legs}
        devt = {k: [] for k in legs}
        decoded = {}
        nbytes = 0
        for rep in range(a.repeats):
            order = list(legs)[rep % 2:] + list(legs)[:rep % 2]
            for k in order:
                s = states[k]
                for _ in range(a.warmup):
                    msgs = round_(s, legs[k])
                decoded[k] = sum(m["gradients"]._flat is not None for m in msgs)
                nbytes = msgs[0]["gradients"].nbytes
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
        assert decoded == {"A": N_CLIENTS, "B": 0}, decoded  # A decoded every message, B none
        # the two legs compute the same round: identically seeded compressors, one round each, bit for bit
        sa, sb = state(levels, 7), state(levels, 7)
        round_(sa, False)
        round_(sb, True)
        same = all(torch.equal(x.detach().view(torch.int32), y.detach().view(torch.int32))
                   and torch.equal(x.grad.view(torch.int32), y.grad.view(torch.int32))
                   for x, y in zip(sa["theta"], sb["theta"]))
        assert same, "the round with the record fold and the round with the decodes differ"
        doc["settings"][name] = {
            "levels": levels, "bits": codec.code_bits(levels), "record_bytes": nbytes, "dense_bytes": 4 * D,
            "A_decode_then_fold": {"host_to_host": summary(host["A"]), "device": summary(devt["A"]),
                                   "messages_decoded": decoded["A"]},
            "B_record_fold": {"host_to_host": summary(host["B"]), "device": summary(devt["B"]),
                              "messages_decoded": decoded["B"]},
            "same_round": same}
    doc["fold"] = [fold(codec, dev, n, recs, levels, a.fold_calls, sets)
                   for n, recs, sets in ((D, 10, 16), (25_000_000, 8, 3)) for levels in (127, 7)]
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


def fold(codec, dev, n, n_records, levels, calls, sets):
    """flc_avg_and_gradient_dense_records against decode-each-record + flc_avg_and_gradients, device events per call."""
    import ctypes

    from fl_sim_amd import _lib

    bits = codec.code_bits(levels)
    stride, _ = codec.dense_wire_layout(n, 0, bits)
    g = torch.Generator(device=dev).manual_seed(3)
    recs = torch.empty(sets, n_records, stride, dtype=torch.uint8, device=dev)
    x = torch.empty(n, device=dev)
    st = codec._stream(dev)
    ws = codec.workspace(dev, codec._ws_size(dev, "flc_quant_workspace_size", 1, n), "quant")
    for si in range(sets):
        for r in range(n_records):
            x.normal_(generator=g).mul_(1e-2)
            norm, codes = codec.dense_wire_views(recs[si, r], n, 0, bits)
            _lib.call("flc_quant_encode_auto", x.data_ptr(), 1, n, 0, levels, bits, _lib.FLC_NORM_INF, 5, si * 64 + r,
                      codes.data_ptr(), norm.data_ptr(), None, None, ws.data_ptr(), ws.numel(), st)
    del x
    srcs = [torch.randn(n, generator=g, device=dev) for _ in range(n_records)]  # (the same bytes for both sides)
    theta = [torch.zeros(n, device=dev) for _ in range(sets)]
    grad = [torch.empty(n, device=dev) for _ in range(sets)]
    dense = [torch.empty(n, device=dev) for _ in range(n_records)]
    P = ctypes.c_void_p
    cw = (ctypes.c_float * n_records)(*([1.0 / n_records] * n_records))
    one = (ctypes.c_int64 * 1)(n)
    sp = (P * n_records)(*[t.data_ptr() for t in srcs])
    dp = (P * n_records)(*[t.data_ptr() for t in dense])

    def fused(si):
        _lib.call("flc_avg_and_gradient_dense_records", (P * 1)(theta[si].data_ptr()), (P * 1)(grad[si].data_ptr()), sp,
                  (P * n_records)(*[recs[si, r].data_ptr() for r in range(n_records)]), cw, cw, n_records, n, 0, levels,
                  bits, one, 1, 0.0, st)

    def chain(si):
        for r in range(n_records):
            norm, codes = codec.dense_wire_views(recs[si, r], n, 0, bits)
            _lib.call("flc_quant_decode", codes.data_ptr(), 1, n, 0, levels, bits, norm.data_ptr(), None, 0,
                      dense[r].data_ptr(), st)
        _lib.call("flc_avg_and_gradients", (P * 1)(theta[si].data_ptr()), (P * 1)(grad[si].data_ptr()), sp, dp, cw, cw,
                  n_records, one, 1, 0.0, st)

    out = {"n": n, "records": n_records, "levels": levels, "bits": bits, "record_sets": sets, "calls": calls,
           "record_bytes": stride, "dense_bytes": 4 * n}
    kept = {}
    for name, fn in (("fused", fused), ("chain", chain)):
        for i in range(sets):
            fn(i)
        torch.cuda.synchronize()
        kept[name] = grad[0].clone()
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
    assert torch.equal(kept["fused"].view(torch.int32), kept["chain"].view(torch.int32)), "the folds differ"
    return out


if __name__ == "__main__":
    sys.exit(main())
