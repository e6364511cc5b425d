"""What selecting by magnitude costs, measured with device events (one JSON line; DESIGN.md §3.1d quotes it from
profiles/topk_magnitude.json).

  (a) the magnitude encode of x' against the signed encode of |x'|: the two have the same keys, the same floor and the
      same path, so any difference is the cost of the order alone.  Shapes: configs[2]'s plain top-k (25 M elements,
      K = 250,000) and the stacked encode at 2^28 elements (K = n / 100, 127 levels).
  (b) ``--signed-only --label NAME``: the signed legs alone, for a run against another build of the library (``FLC_LIB``,
      the parent commit's) in alternating processes; ``--merge`` folds those runs into the result and states whether
      this tree's signed legs lie inside the parent's own repeat-to-repeat range.

Each repeat times ``--calls`` calls of each leg between two device events, the legs alternating inside one process; every
call reads an input that is not resident from the previous calls (the inputs rotate over a pool larger than the
memory-side cache).  Reported per leg: the median over the repeats and their range, microseconds per call."""
import argparse
import glob
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("topk_25M", 25_000_000, 250_000, 8, False), ("stacked_2p28", 1 << 28, (1 << 28) // 100, 3, True))


def time_leg(fn, pool, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(calls):
        fn(pool[i % len(pool)], i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def summary(ts):
    return {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2),
            "repeats_us": [round(t, 2) for t in ts]}


def merge(out_dir, out):
    res = json.load(open(out))
    runs = [json.load(open(p)) for p in sorted(glob.glob(os.path.join(out_dir, "topk_magnitude_ab_*.json")))]
    ab = {}
    for shape in (s[0] for s in SHAPES):
        rows = {}
        for r in runs:
            rows.setdefault(r["label"], []).extend(r["shapes"][shape]["signed"]["repeats_us"])
        if set(rows) != {"parent", "tree"}:
            continue
        p, t = rows["parent"], rows["tree"]
        ab[shape] = {"parent": summary(p), "tree": summary(t),
                     "tree_inside_parent_range": bool(min(p) <= min(t) and max(t) <= max(p)),
                     "tree_median_inside_parent_range": bool(min(p) <= statistics.median(t) <= max(p))}
    res["signed_vs_parent"] = ab
    json.dump(res, open(out, "w"), indent=1)
    print(json.dumps(res))
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--signed-only", action="store_true")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_magnitude.json"))
    ap.add_argument("--merge", default=None, help="directory of the --signed-only runs to fold into --out")
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    assert a.repeats >= 5 and a.calls >= 30
    sys.path.insert(0, ROOT)
    from fl_sim_amd import codec

    assert torch.cuda.is_available(), "this measurement needs a HIP device"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls": a.calls, "label": a.label,
           "library": os.environ.get("FLC_LIB", "in-tree"), "shapes": {}}
    for name, n, k, pool_n, stacked in SHAPES:
        g = torch.Generator(device=dev).manual_seed(n % 1000)
        xs = [torch.randn(n, generator=g, device=dev) * 1e-3 for _ in range(pool_n)]  # x': mixed signs
        ab = [x.abs() for x in xs]  # |x'|: the signed select's input with the same keys
        if stacked:
            out = codec.stacked_encode(xs[0], k, 127, seed=1, counter=0)  # (a packet reused by every call: no allocation)
            signed = lambda x, i: codec.stacked_encode(x, k, 127, seed=1, counter=i, out=out)  # noqa: E731
            mag = None if a.signed_only else (
                lambda x, i: codec.stacked_encode(x, k, 127, seed=1, counter=i, out=out, order=codec.ORDER_MAGNITUDE))
        else:
            signed = lambda x, i: codec.topk_encode(x, k, with_tiles=True)  # noqa: E731
            mag = None if a.signed_only else (
                lambda x, i: codec.topk_encode(x, k, with_tiles=True, order=codec.ORDER_MAGNITUDE))
        legs = {"signed": (signed, ab)} if a.signed_only else {"magnitude": (mag, xs), "signed": (signed, ab)}
        if not a.signed_only:  # the two legs keep the same entries (checked once, outside the timed window)
            i1 = codec.topk_encode(xs[0], k, order=codec.ORDER_MAGNITUDE)[0]
            i2 = codec.topk_encode(ab[0], k)[0]
            assert torch.equal(i1, i2)
        times = {leg: [] for leg in legs}
        for fn, pool in legs.values():  # warm-up: code objects, workspaces
            time_leg(fn, pool, 5)
        for _ in range(a.repeats):
            for leg, (fn, pool) in legs.items():
                times[leg].append(time_leg(fn, pool, a.calls))
        assert codec.topk_status(dev) == 0
        row = {leg: summary(ts) for leg, ts in times.items()}
        if not a.signed_only:
            m, s = row["magnitude"], row["signed"]
            row["ranges_overlap"] = bool(m["min_us"] <= s["max_us"] and s["min_us"] <= m["max_us"])
            row["median_diff_us"] = round(m["median_us"] - s["median_us"], 2)
        row.update(n=n, k=k, pool=pool_n)
        res["shapes"][name] = row
        del xs, ab
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
