#!/usr/bin/env python3
"""Fixture for the codec's call site at SCAFFOLD and IFCA: ``tests/golden/delta_codec.npz``.

The reference never compresses a message (see ``gen_golden.py``, ``gen_round``), so the round's meaning is composed
from the reference's own pieces, all run from its sources at ``REF`` (none of its text is kept here):

* client — the algorithm's own ``communicate`` (scaffold/_scaffold.py:210-222: ``parameters_delta`` and
  ``control_variates_delta``, then the control variates take the updated ones; ifca/_ifca.py:228-240:
  ``delta_parameters`` and ``cluster_id``; ``ClientMessage`` = ``dict``) on a client holding ``scaffold_codec_inputs``'
  / ``ifca_codec_inputs``' tensors;
* codec — every flattened delta through ``Compressor.compressVector`` (compressors.py:267-410), a fresh compressor
  set per client and per vector; within a SCAFFOLD message ``parameters_delta`` before ``control_variates_delta``; the
  decoded vector, reshaped, put back into the message;
* server — the algorithm's own ``update`` (_scaffold.py:158-169 over ``Server.add_parameters``; _ifca.py:167-195).

The global ``random`` / ``np.random`` streams are seeded once per round (``delta_codec_seed``) and consumed in message
order.  Stored per case ``dc_<alg>_<codec>_<tag>``: SCAFFOLD ``theta`` and ``cv``, IFCA ``center<c>`` and ``ids<c>``
(SHA-256; the small shape also in full), ``stats`` (per client, per compressor set: the send of every stage, then the
input components of every stage), ``next_random`` / ``next_np`` (the streams' next draws after the round).

The constants and inputs below import without the reference; only ``main`` needs it.
"""

from __future__ import annotations

import random
import sys
import types
from pathlib import Path
from typing import Any, Dict

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[2]))

from tests.golden.gen_golden import (CONFIG1_SHAPES, IFCA_CLUSTER_OF, OUT, REF, SCAFFOLD_CFG, SMALL_SHAPES,  # noqa: E402
                                     compile_methods, ifca_inputs, load_reference_compressors,
                                     reference_round_compressors, scaffold_inputs, sha, variant_namespace)

DELTA_CODECS = ("stacked10", "topk", "std8inf", "natural")
DELTA_ALGS = ("scaffold", "ifca")
SCAFFOLD_MSGS = 10  # of SCAFFOLD_CFG["num_clients"] = 20 clients
# input seeds at which the K-th largest value of every delta is unique at both shapes (main asserts it)
SCAFFOLD_INPUT_SEED = 90
IFCA_INPUT_SEED = 91


def delta_codec_key(alg: str, codec: str, tag: str) -> str:
    return f"dc_{alg}_{codec}_{tag}"


def delta_codec_seed(alg: str, codec: str, tag: str) -> int:
    """The round's seed of both global streams."""
    return 1100 + 31 * DELTA_ALGS.index(alg) + 7 * DELTA_CODECS.index(codec) + (0 if tag == "small" else 1)


def scaffold_codec_inputs(shapes):
    """(server θ, server c, clients): every client trained from θ (its cached parameters) and holds control variates
    and updated control variates of its own."""
    theta, cvs, _ = scaffold_inputs(shapes)
    g = torch.Generator().manual_seed(SCAFFOLD_INPUT_SEED)
    clients = []
    for i in range(SCAFFOLD_MSGS):
        local = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in theta]
        cv = [torch.randn(sh, generator=g) * 1e-3 for sh in shapes]
        ucv = [c + torch.randn(c.shape, generator=g) * 1e-2 for c in cv]
        clients.append({"client_id": i, "train_samples": 100 * (i + 1) + 7 * (i % 3), "metrics": {},
                        "cached": [t.clone() for t in theta], "local": local, "cv": cv, "ucv": ucv})
    return theta, cvs, clients


def ifca_codec_inputs(shapes):
    """(cluster centres with the previous round's client ids, clients): client i trained from the centre of cluster
    IFCA_CLUSTER_OF[i]; cluster 1 receives no message."""
    centers, _ = ifca_inputs(shapes)
    g = torch.Generator().manual_seed(IFCA_INPUT_SEED)
    clients = []
    for i, c in enumerate(IFCA_CLUSTER_OF):
        cached = [t.clone() for t in centers[c]["center_model_params"]]
        local = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached]
        clients.append({"client_id": i, "cluster_id": c, "train_samples": 100 * (i + 1) + 7 * (i % 3), "metrics": {},
                        "cached": cached, "local": local})
    return centers, clients


def _compress_in_place(ref, codec: str, m: dict, key: str, stats: list) -> None:
    flat = torch.cat([d.reshape(-1) for d in m[key]]).numpy()
    # top-k keeps the K largest values (compressors.py:294-295, an unstable argsort): the K-th must be unique, or the
    # reference has a choice among ties
    srt = np.sort(flat)
    K = flat.size // 100
    assert srt[-K] != srt[-K - 1] and srt[-K] != srt[-K + 1], "a tie at the top-k threshold"
    out = flat
    comps = reference_round_compressors(ref, codec, flat.size)
    for comp in comps:
        out = comp.compressVector(out)
    stats += [float(comp.last_need_to_send_advance) for comp in comps]
    stats += [float(comp.total_input_components) for comp in comps]
    out_t = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))
    ts, off = [], 0
    for d in m[key]:
        ts.append(out_t[off:off + d.numel()].reshape(d.shape).clone())
        off += d.numel()
    m[key] = ts


def _client(src: dict, node) -> types.SimpleNamespace:
    c = types.SimpleNamespace(client_id=src["client_id"], _metrics=src["metrics"],
                              _cached_parameters=[t.clone() for t in src["cached"]],
                              train_loader=types.SimpleNamespace(dataset=list(range(src["train_samples"]))))
    c.model = torch.nn.Module()
    for j, t in enumerate(src["local"]):
        c.model.register_parameter(f"p{j}", torch.nn.Parameter(t.clone()))
    c.get_detached_model_parameters = types.MethodType(node["get_detached_model_parameters"], c)
    return c


def gen_delta_codec() -> None:
    ref = load_reference_compressors()
    ns = variant_namespace()
    srv = compile_methods("fl_sim/nodes.py", "Server", ("add_parameters",), ns)
    node = compile_methods("fl_sim/nodes.py", "Node", ("get_detached_model_parameters",), ns)
    cns = {**ns, "ClientMessage": dict}
    sc_upd = compile_methods("fl_sim/algorithms/scaffold/_scaffold.py", "SCAFFOLDServer", ("update",), ns)["update"]
    sc_comm = compile_methods("fl_sim/algorithms/scaffold/_scaffold.py", "SCAFFOLDClient", ("communicate",),
                              cns)["communicate"]
    if_upd = compile_methods("fl_sim/algorithms/ifca/_ifca.py", "IFCAServer", ("update",), ns)["update"]
    if_comm = compile_methods("fl_sim/algorithms/ifca/_ifca.py", "IFCAClient", ("communicate",), cns)["communicate"]
    store: Dict[str, Any] = {}
    for tag, shapes in (("small", SMALL_SHAPES), ("config1", CONFIG1_SHAPES)):
        full = tag == "small"

        def put(key, tensors):
            flat = torch.cat([t.detach().reshape(-1) for t in tensors]).numpy()
            store[key + "|sha"] = np.array(sha(flat))
            if full:
                store[key + "|out"] = flat

        for codec in DELTA_CODECS:
            # SCAFFOLD: 10 messages of 20 clients
            theta, cvs, clients = scaffold_codec_inputs(shapes)
            s = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(lr=SCAFFOLD_CFG["lr"]),
                                      _clients=list(range(SCAFFOLD_CFG["num_clients"])))
            s.model = torch.nn.Module()
            for i, t in enumerate(theta):
                s.model.register_parameter(f"p{i}", torch.nn.Parameter(t.clone()))
            s.add_parameters = types.MethodType(srv["add_parameters"], s)
            s._control_variates = [t.clone() for t in cvs]
            s._received_messages = []
            seed = delta_codec_seed("scaffold", codec, tag)
            random.seed(seed)
            np.random.seed(seed)
            stats = []
            for src in clients:
                c = _client(src, node)
                c._control_variates = [t.clone() for t in src["cv"]]
                c._updated_control_variates = [t.clone() for t in src["ucv"]]
                sc_comm(c, s)
                assert c._updated_control_variates is None
                assert all(torch.equal(a, b) for a, b in zip(c._control_variates, src["ucv"]))
                row: list = []
                _compress_in_place(ref, codec, s._received_messages[-1], "parameters_delta", row)
                _compress_in_place(ref, codec, s._received_messages[-1], "control_variates_delta", row)
                stats.append(row)
            sc_upd(s)
            key = delta_codec_key("scaffold", codec, tag)
            put(key + "|theta", list(s.model.parameters()))
            put(key + "|cv", s._control_variates)
            store[key + "|stats"] = np.array(stats, dtype=np.float64)
            store[key + "|next_random"] = np.array(random.random())
            store[key + "|next_np"] = np.array(np.random.random_sample())

            # IFCA: 4 clusters, cluster 1 idle this round
            centers, clients = ifca_codec_inputs(shapes)
            s = types.SimpleNamespace(device=torch.device("cpu"), config=types.SimpleNamespace(num_clusters=4))
            s._cluster_centers, s._received_messages = centers, []
            seed = delta_codec_seed("ifca", codec, tag)
            random.seed(seed)
            np.random.seed(seed)
            stats = []
            for src in clients:
                c = _client(src, node)
                c.cluster_id = src["cluster_id"]
                if_comm(c, s)
                row = []
                _compress_in_place(ref, codec, s._received_messages[-1], "delta_parameters", row)
                stats.append(row)
            if_upd(s)
            key = delta_codec_key("ifca", codec, tag)
            for c in range(4):
                put(f"{key}|center{c}", s._cluster_centers[c]["center_model_params"])
                store[f"{key}|ids{c}"] = np.array(s._cluster_centers[c]["client_ids"], dtype=np.int64)
            store[key + "|stats"] = np.array(stats, dtype=np.float64)
            store[key + "|next_random"] = np.array(random.random())
            store[key + "|next_np"] = np.array(np.random.random_sample())
    np.savez_compressed(OUT / "delta_codec.npz", **store)
    print("delta_codec.npz:", len(store), "arrays")


def main() -> int:
    if not REF.exists():
        print("reference not present; nothing to do", file=sys.stderr)
        return 1
    torch.set_num_threads(1)
    gen_delta_codec()
    return 0


if __name__ == "__main__":
    sys.exit(main())
