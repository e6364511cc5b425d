#!/usr/bin/env python3
"""The compressed round with sampled clients, as the reference runs it (nodes.py:741-751: a subset of the clients each
round): 100 clients at configs[0]'s model shapes, each with its own stacked pipeline (TopK 1 % -> standard dithering
s = 127, philox), a device-resident FedAvg server; every round 10 clients drawn by
``np.random.RandomState(seed).choice(100, 10, replace=False)`` communicate and the server updates.  Each client's
dithering compressor advances its Philox counter once per message, so from the second round on the sampled clients
carry different counters.  Beside it the lockstep round: the same 10 clients every round (equal counters).

Prints one JSON line: µs per round of both, and ``compressed.deferred_stats()`` of the sampled rounds where the
package has it.

    python tools/sampled_round.py [--rounds 200] [--warmup 5] [--seed 0]
"""

import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIG0_SHAPES = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (256, 1568), (256,), (10, 256), (10,)]  # 417,482
N_CLIENTS, PER_ROUND, LEVELS = 100, 10, 127


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.rounds < 200:
        ap.error("at least 200 timed rounds")

    from fl_sim_amd import Compressor, compressed
    from fl_sim_amd.aggregation import FedOptUpdateMixin
    from fl_sim_amd.compressed import CompressedFedOptClientMixin

    class _Client(CompressedFedOptClientMixin):
        pass

    class _Server(FedOptUpdateMixin):
        pass

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    d0 = sum(int(np.prod(s)) for s in CONFIG0_SHAPES)
    g = torch.Generator(device=dev).manual_seed(321)
    th0 = [torch.randn(sh, generator=g, device=dev) * 0.1 for sh in CONFIG0_SHAPES]
    cached = [t.clone() for t in th0]  # (the round's global model: every client's cached copy, only read)
    clients = []
    for i in range(N_CLIENTS):
        c = _Client()
        c.client_id, c._metrics = i, {}
        c.train_loader = types.SimpleNamespace(dataset=range(100 * (i % 10 + 1)))
        c.model = torch.nn.Module()
        for j, t in enumerate(th0):
            c.model.register_parameter(f"p{j}",
                                       torch.nn.Parameter(t + torch.randn(t.shape, generator=g, device=dev) * 1e-2))
        c._cached_parameters = cached
        clients.append(c)

    def pipeline(i):
        tk = Compressor(rng="philox", seed=i)
        tk.makeTopKCompressor(d0 // 100, d0)
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        sd = Compressor(rng="philox", seed=i, extended_levels=True)
        sd.makeStandardDitheringFP32(LEVELS, nc, np.inf)
        return [tk, sd]

    def server():
        s = _Server()
        s.model = torch.nn.Module()
        for j, t in enumerate(th0):
            s.model.register_parameter(f"p{j}", torch.nn.Parameter(t.clone()))
        s.delta_parameters = [torch.zeros_like(p) for p in s.model.parameters()]
        s.v_parameters = None
        s.config = types.SimpleNamespace(optimizer="avg", lr=1, betas=(0, 1), tau=1)
        return s

    stats = getattr(compressed, "deferred_stats", None)

    def measure(draws):
        """µs per round over draws[warmup:], every client starting from a fresh pipeline."""
        for c in clients:
            c.compressors = pipeline(c.client_id)
        s = server()

        def round_(chosen):
            s._received_messages = []
            for i in chosen:
                clients[i].communicate(s)
            s.update()

        for ch in draws[:a.warmup]:
            round_(ch)
        torch.cuda.synchronize()
        if stats is not None:
            stats(reset=True)
        t0 = time.perf_counter()
        for ch in draws[a.warmup:]:
            round_(ch)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt / (len(draws) - a.warmup) * 1e6, (stats(reset=True) if stats is not None else None)

    rs = np.random.RandomState(a.seed)
    total = a.warmup + a.rounds
    sampled = [rs.choice(N_CLIENTS, PER_ROUND, replace=False).tolist() for _ in range(total)]
    lockstep = [sampled[0]] * total
    us_s, st_s = measure(sampled)
    us_l, st_l = measure(lockstep)
    line = {"tool": "sampled_round", "clients": N_CLIENTS, "per_round": PER_ROUND, "params": d0,
            "rounds": a.rounds, "warmup": a.warmup, "seed": a.seed,
            "sampled_us_per_round": round(us_s, 1), "lockstep_us_per_round": round(us_l, 1)}
    if st_s is not None:
        line["deferred_stats_sampled"] = st_s
        line["deferred_stats_lockstep"] = st_l
    print(json.dumps(line))


if __name__ == "__main__":
    main()
