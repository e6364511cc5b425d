"""The robust fold on an MI355X (one JSON document, ``--out``, default profiles/robust_round.json; DESIGN.md §3.3l
quotes it), at n = 417,482 and 25,000,000 elements in one tensor, C = 10, 16, 32 and 64 messages:
flc_robust_fold (median, and trimmed mean with b = C // 10) with the fused FedAvg step, beside flc_model_fold (the mean
of the same messages with the same step, 16 messages per launch, chained), ``torch.stack(msgs).sort(0)`` -> slice ->
mean -> the delta update -> flc_fedopt_step, and a stream copy of the stacked messages (C n values read and written).
The legs alternate in one process; per leg the median and the range of ``--repeats`` repeats, each timing some calls
with device events, microseconds per call.  ``rate_gbs`` is the leg's algorithmic bytes over its median time: (C + 4) n
values for the folds (every message, delta and theta read, delta and theta written), 2 C n for the copy.  The inputs
are whatever the previous call left in the caches.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

SIZES = (417_482, 25_000_000)
CLIENTS = (10, 16, 32, 64)
BETA, LR = 0.9, 1.0


def timed(legs, repeats, calls, warmup):
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


def part(codec, _lib, dev, n, C, repeats, calls, warmup):
    g = torch.Generator(device=dev).manual_seed(n + C)
    msgs = [torch.randn(n, generator=g, device=dev) * 1e-2 for _ in range(C)]
    delta, theta = torch.zeros(n, device=dev), torch.randn(n, generator=g, device=dev)
    stacked = torch.stack(msgs)
    sink = torch.empty_like(stacked)
    st, b = codec._stream(dev), C // 10
    P = ctypes.c_void_p
    cv = lambda a: ctypes.cast(a, P)  # noqa: E731
    one = lambda t: cv((P * 1)(t.data_ptr()))  # noqa: E731
    dp, tp, sz = one(delta), one(theta), cv((ctypes.c_int64 * 1)(n))
    sp = cv((P * C)(*[m.data_ptr() for m in msgs]))
    chunks = [(cv((P * len(ms))(*[m.data_ptr() for m in ms])), cv((ctypes.c_float * len(ms))(*[(1 - BETA) / C] * len(ms))),
               len(ms)) for ms in (msgs[c:c + 16] for c in range(0, C, 16))]

    def robust(rule, trim):
        _lib.call("flc_robust_fold", dp, sp, C, sz, 1, rule, trim, 1 - BETA, 0, BETA, tp, None, 0, LR, 0.0, 0.0, st)

    def mean():
        for i, (ptrs, wts, cnt) in enumerate(chunks):
            last = i == len(chunks) - 1
            _lib.call("flc_model_fold", dp, ptrs, wts, cnt, sz, 1, 0 if i == 0 else 2, BETA, tp if last else None, None,
                      0, LR, 0.0, 0.0, st)

    def torch_sort():
        s = torch.stack(msgs).sort(0).values
        r = s[b:C - b].mean(0)
        delta.mul_(BETA).add_(r, alpha=1 - BETA)
        codec.fedopt_step(theta, delta, None, "avg", LR, 0.0, 0.0)

    us = timed({"robust_median": lambda: robust(0, 0), "robust_trimmed": lambda: robust(1, b), "model_fold_mean": mean,
                "torch_sort_trimmed": torch_sort, "stream_copy": lambda: sink.copy_(stacked)}, repeats, calls, warmup)
    doc = {"n": n, "clients": C, "trim": b}
    for k, v in us.items():
        med = statistics.median(v)
        nbytes = 8 * C * n if k == "stream_copy" else 4 * (C + 4) * n
        doc[k] = {"median_us": round(med, 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                  "rate_gbs": round(nbytes / med / 1e3, 1)}
    for k in ("robust_median", "robust_trimmed", "model_fold_mean"):
        doc[k]["fraction_of_copy_rate"] = round(doc[k]["rate_gbs"] / doc["stream_copy"]["rate_gbs"], 3)
    return doc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "robust_round.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from fl_sim_amd import _lib, codec

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rows = []
    for n in SIZES:
        for C in CLIENTS:
            rows.append(part(codec, _lib, dev, n, C, a.repeats, 20 if n < 1_000_000 else 3, 3 if n < 1_000_000 else 1))
            torch.cuda.empty_cache()
    doc = {"what": "flc_robust_fold (median; trimmed mean, b = C // 10) with the fused FedAvg step beside flc_model_fold "
                   "(the mean, chained past 16 messages), torch.stack().sort(0) -> slice -> mean -> update -> "
                   "flc_fedopt_step, and a stream copy of the stacked messages; device events, us per call (median, "
                   "range of the repeats); rate_gbs = algorithmic bytes / median time",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
