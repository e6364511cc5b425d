"""The client side of a round whose clients send the natural compressor's dense records, with each message encoded when
it is made and with the round's messages deferred to one batched encode (one JSON document, ``--out``, default
profiles/natural_defer_round.json; DESIGN.md §3.3g quotes it).  configs[0]'s shape: 10 clients × 417,482 parameters,
the natural compressor, philox, ``wire_records`` on, everything device-resident, without and with ``error_feedback``.
A round is the 10 ``communicate``-time ``compress_delta`` calls (with feedback, each with the client's memory) and the
first access to a record — the deferred leg's batch runs there.

  off  ``compressed.NATURAL_DEFER`` False: per message its own flc_natural_encode; with feedback flc_ef_accumulate,
       flc_natural_encode, flc_natural_decode into a fresh vector and flc_ef_residual_dense
  on   ``compressed.NATURAL_DEFER`` True: one flc_natural_encode_round; with feedback flc_ef_accumulate per message and
       one flc_natural_encode_residual_round

The legs are interleaved in one process, each repeated ``--repeats`` times in rotating order; a repeat times
``--calls`` rounds with a host clock (host to host, ending in a device synchronise) and with a pair of device events
around the same rounds.  Reported per leg: the median over the repeats and their spread (min, max), microseconds per
round.  Both legs must give the same records, memories, statistics and counters bit for bit.

``--off-only --package-root DIR`` measures the off leg alone with the package found under ``DIR`` — a checkout of the
parent commit, which has no switch — and ``--parent FILE`` copies that run's figures into the document, so that the
code under test is not its own yardstick.  ``--second-run FILE`` copies another whole run of this probe into the
document (``second_run``): the size bounds rest on what held in every run.

``encode``: the encodes alone at larger messages, device events and host clock per round of messages — ``n_msgs`` times
the immediate call (plain: flc_natural_encode; feedback: flc_natural_encode, flc_natural_decode into a fresh vector,
flc_ef_residual_dense) against one round call on the same vectors, refilled before every timed call — up to n = 16 M
with 8 messages, where a message is far past fixed latency."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]
N_CLIENTS = 10
SETTINGS = {"plain": False, "feedback": True}
ENCODE_POINTS = ((417_482, 10), (1_000_000, 10), (2_000_000, 10), (4_000_000, 8), (8_000_000, 8), (16_000_000, 8))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--package-root", default=ROOT)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--second-run", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "natural_defer_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.package_root))
    from fl_sim_amd import Compressor, _lib, codec, compressed
    from fl_sim_amd.feedback import ErrorMemory

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    assert a.repeats >= 5 and a.calls >= 50
    assert a.off_only or hasattr(compressed, "NATURAL_DEFER"), "this package has no switch: --off-only"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    D = sum(torch.Size(s).numel() for s in SHAPES)
    g = torch.Generator(device=dev).manual_seed(1)
    cached = [torch.randn(s, generator=g, device=dev) * 0.1 for s in SHAPES]
    locals_ = [[t + torch.randn(t.shape, generator=g, device=dev) * 1e-2 for t in cached] for _ in range(N_CLIENTS)]

    def state(fb, seed):
        comps = []
        for i in range(N_CLIENTS):
            c = Compressor(rng="philox", seed=seed + i)
            c.makeNaturalCompressorFP32()
            comps.append([c])
        return {"comps": comps, "mems": [ErrorMemory(D, dev) if fb else None for _ in range(N_CLIENTS)]}

    def round_(s, on):
        if not a.off_only:
            compressed.NATURAL_DEFER = on
        ds = [compressed.compress_delta(locals_[i], cached, s["comps"][i], s["mems"][i], wire=True)
              for i in range(N_CLIENTS)]
        assert ds[0].record is not None  # the first access: the deferred leg's batch runs here
        return ds

    legs = {"off": False} if a.off_only else {"off": False, "on": True}
    doc = {"what": "client side of a round, 10 clients x 417,482 parameters, the natural compressor, philox, "
                   "wire_records on, without (plain) and with (feedback) error_feedback: ten compress_delta calls and "
                   "the first record access; off: NATURAL_DEFER False, on: NATURAL_DEFER True; us per round",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_repeat": a.calls, "n": D,
           "legs": list(legs), "settings": {}}
    for name, fb in SETTINGS.items():
        states = {k: state(fb, 100 * (j + 1)) for j, k in enumerate(legs)}
        host = {k: [] for k in legs}
        devt = {k: [] for k in legs}
        compressed.deferred_dense_stats(reset=True)
        for rep in range(a.repeats):
            order = list(legs)[rep % len(legs):] + list(legs)[:rep % len(legs)]
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
        batches = compressed.deferred_dense_stats(reset=True)
        rounds = a.repeats * (a.warmup + a.calls)  # (no count slots: exactly one batch per deferred round)
        want = {"batches": 0, "messages": 0} if a.off_only else {"batches": rounds, "messages": N_CLIENTS * rounds}
        assert batches == want, (batches, want)
        entry = {"error_feedback": fb}
        for k in legs:
            entry[k] = {"host_to_host": summary(host[k]), "device": summary(devt[k])}
        if not a.off_only:
            # the two legs compute the same rounds: identically seeded compressors, three rounds each, bit for bit
            sa, sb = state(fb, 7), state(fb, 7)
            same = True
            for _ in range(3):
                da, db = round_(sa, False), round_(sb, True)
                for x, y in zip(da, db):  # (the records' code field: the norm field and the padding are not the message)
                    vx, vy = (codec.dense_wire_views(d.record, d.n, d.format, d.bits)[1] for d in (x, y))
                    same = same and torch.equal(vx, vy)
            if fb:
                same = same and all(torch.equal(x.value().view(torch.int32), y.value().view(torch.int32))
                                    for x, y in zip(sa["mems"], sb["mems"]))
            same = same and all(x[0].really_need_to_send_components == y[0].really_need_to_send_components
                                and x[0].total_input_components == y[0].total_input_components
                                and x[0].philox.counter == y[0].philox.counter
                                for x, y in zip(sa["comps"], sb["comps"]))
            assert same, "the switch-on round and the switch-off round differ"
            entry["same_round"] = same
            entry["on_faster_beyond_spread"] = {"host_to_host": separated(host["on"], host["off"]),
                                                "device": separated(devt["on"], devt["off"])}
        doc["settings"][name] = entry
    if not a.off_only:
        compressed.NATURAL_DEFER = False
    if a.parent:
        with open(a.parent) as f:
            p = json.load(f)
        doc["parent_commit_off"] = {k: v["off"] for k, v in p["settings"].items()}
        for k, v in doc["settings"].items():
            if "on" in v:
                off = p["settings"][k]["off"]["host_to_host"]
                v["on_faster_than_parent_off_beyond_spread"] = v["on"]["host_to_host"]["max_us"] < off["min_us"]
                v["on_median_not_above_parent_off_median"] = v["on"]["host_to_host"]["median_us"] <= off["median_us"]
    if not a.no_encode_points and not a.off_only:
        doc["encode"] = [encode_point(_lib, codec, dev, n, m, fb, a.encode_calls)
                         for n, m in ENCODE_POINTS for fb in (False, True)]
    if a.second_run:  # (another run of this probe in the same session, kept whole beside this one)
        with open(a.second_run) as f:
            doc["second_run"] = json.load(f)
    text = json.dumps(doc, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)
    return 0


def encode_point(_lib, codec, dev, n, n_msgs, fb, calls):
    """``n_msgs`` times flc_natural_encode — with ``fb`` followed by flc_natural_decode into a fresh vector and
    flc_ef_residual_dense — against one flc_natural_encode_round / flc_natural_encode_residual_round, on vectors
    holding the same values."""
    fmt = _lib.FLC_WIRE_NATURAL
    stride, off = codec.dense_wire_layout(n, fmt, 16)
    g = torch.Generator(device=dev).manual_seed(3)
    src = [torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(n_msgs)]
    mems = {k: [torch.empty(n, device=dev) for _ in range(n_msgs)] for k in ("each", "round")}
    recs = {k: torch.zeros(n_msgs, stride, dtype=torch.uint8, device=dev) for k in ("each", "round")}
    seeds, ctrs = list(range(5, 5 + n_msgs)), list(range(n_msgs))
    st = codec._stream(dev)
    views = [codec.dense_wire_views(recs["each"][c], n, fmt, 16)[1] for c in range(n_msgs)]

    def each():
        for c in range(n_msgs):
            _lib.call("flc_natural_encode", mems["each"][c].data_ptr(), n, seeds[c], ctrs[c], None,
                      views[c].data_ptr(), None, None, 0, st)
            if fb:
                codec.ef_residual_dense(mems["each"][c], codec.dense_record_decode(recs["each"][c], n, fmt, 0, 16))

    def round_():
        (codec.natural_encode_residual_round if fb else codec.natural_encode_round)(mems["round"], seeds, ctrs,
                                                                                    recs["round"])

    out = {"n": n, "messages": n_msgs, "error_feedback": fb, "calls": calls}
    times = {}
    for name, fn in (("chain", each), ("round", round_)):
        key = "each" if name == "chain" else "round"
        dv, hs = [], []
        for i in range(calls + 3):  # (three untimed calls first)
            for m, x in zip(mems[key], src):  # the vectors hold a again (queued ahead of the first event)
                m.copy_(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                hs.append((time.perf_counter() - t0) * 1e6)
                dv.append(e0.elapsed_time(e1) * 1e3)
        times[name] = dv
        out[name] = {"device": summary(dv), "host_to_host": summary(hs)}
    lo, hi = off["codes"], off["codes"] + 2 * n
    same = (torch.equal(recs["each"][:, lo:hi], recs["round"][:, lo:hi])
            and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(mems["each"], mems["round"])))
    assert same, "the batched call and the per-message chain differ"
    out["same_records_and_memories"] = same
    out["round_faster_beyond_spread"] = separated(times["round"], times["chain"])
    out["round_slower_beyond_spread"] = separated(times["chain"], times["round"])
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    sys.exit(main())
