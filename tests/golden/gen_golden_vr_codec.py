#!/usr/bin/env python3
"""Fixture for the codec's call site at the variance-reduced algorithms: ``tests/golden/vr_codec.npz``.

The reference never compresses a message (see ``gen_golden.py``, ``gen_round``), so the round's meaning is composed
from the reference's own pieces, all run from its sources at ``REF`` (none of its text is kept here):

* client — the algorithm's own ``communicate`` (fedprox/_fedprox.py:208-217, fedpd/_fedpd.py:252-275,
  proxskip/_proxskip.py:265-276, pfedmac/_pfedmac.py:203-212; ``ClientMessage`` = ``dict``) on a client whose model
  holds ``vr_inputs``' parameters and, as ``.grad``, its gradients; with ``config.vr`` the message carries
  ``gradients``;
* codec — the flattened gradients through ``Compressor.compressVector`` (compressors.py:267-410), a fresh compressor
  set per client; the decoded vector, reshaped, put back as ``gradients``.  ``parameters`` stay as sent;
* server — the algorithm's own ``update`` over ``Server.avg_parameters`` / ``update_gradients`` (nodes.py:1134-1180).

The global ``random`` / ``np.random`` streams are seeded once per round (``vr_codec_seed``) and consumed client by
client in message order.  Stored per case ``vrc_<server>_<codec>_<messages>_<tag>``: ``theta`` and ``grad`` (SHA-256;
the small shape also in full), ``stats`` (per client: the send of every stage, then the input components of every
stage), ``next_random`` / ``next_np`` (the streams' next draws after the round).

The constants below import without the reference; only ``main`` needs it.
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

from tests.golden.gen_golden import (CONFIG1_SHAPES, OUT, PFEDMAC_BETA, REF, SMALL_SHAPES, VR_SERVERS,  # noqa: E402
                                     compile_methods, load_reference_compressors, reference_round_compressors, sha,
                                     variant_namespace, vr_inputs)

VR_CODECS = ("stacked10", "topk", "std8inf", "natural")
VR_CODEC_MSGS = (10, 20)
VR_CLIENTS = {name: (rel, cls.replace("Server", "Client")) for name, (rel, cls) in VR_SERVERS.items()}


def vr_codec_key(name: str, codec: str, nm: int, tag: str) -> str:
    return f"vrc_{name}_{codec}_{nm}_{tag}"


def vr_codec_seed(name: str, codec: str, nm: int, tag: str) -> int:
    """The round's seed of both global streams."""
    return (900 + 41 * list(VR_SERVERS).index(name) + 7 * VR_CODECS.index(codec) + (3 if nm == 20 else 0)
            + (0 if tag == "small" else 1))


def gen_vr_codec() -> None:
    ref = load_reference_compressors()
    ns = variant_namespace()
    srv = compile_methods("fl_sim/nodes.py", "Server", ("add_parameters", "avg_parameters", "update_gradients"), ns)
    node = compile_methods("fl_sim/nodes.py", "Node", ("get_detached_model_parameters",), ns)
    store: Dict[str, Any] = {}
    for tag, shapes in (("small", SMALL_SHAPES), ("config1", CONFIG1_SHAPES)):
        full = tag == "small"

        def put(key, tensors):
            flat = torch.cat([t.detach().reshape(-1) for t in tensors]).numpy()
            store[key + "|sha"] = np.array(sha(flat))
            if full:
                store[key + "|out"] = flat

        for name, (rel, cls) in VR_SERVERS.items():
            upd = compile_methods(rel, cls, ("update",), ns)["update"]
            comm = compile_methods(rel, VR_CLIENTS[name][1], ("communicate",), {**ns, "ClientMessage": dict})["communicate"]
            for codec in VR_CODECS:
                for nm in VR_CODEC_MSGS:
                    params, msgs = vr_inputs(shapes, nm)
                    s = types.SimpleNamespace(device=torch.device("cpu"), n_iter=0, _num_communications=0)
                    s.model = torch.nn.Module()
                    for i, t in enumerate(params):
                        s.model.register_parameter(f"p{i}", torch.nn.Parameter(t.clone()))
                    for fn_name, fn in srv.items():
                        setattr(s, fn_name, types.MethodType(fn, s))
                    s.config = types.SimpleNamespace(vr=True, beta=PFEDMAC_BETA)
                    s._received_messages = []
                    seed = vr_codec_seed(name, codec, nm, tag)
                    random.seed(seed)
                    np.random.seed(seed)
                    stats = []
                    for src in msgs:
                        c = types.SimpleNamespace(
                            client_id=src["client_id"], _metrics=src["metrics"],
                            _cached_parameters=[t.clone() for t in src["parameters"]],
                            train_loader=types.SimpleNamespace(dataset=list(range(src["train_samples"]))),
                            # every client communicates this round: FedPD's every-n-iterations pattern with n = 1,
                            # ProxSkip's pattern with a 1 at the server's iteration
                            config=types.SimpleNamespace(vr=True, stochastic=False, comm_freq=1, p=1.0),
                            communication_pattern=[1])
                        c.model = torch.nn.Module()
                        for j, (t, g) in enumerate(zip(src["parameters"], src["gradients"])):
                            p = torch.nn.Parameter(t.clone())
                            p.grad = g.clone()
                            c.model.register_parameter(f"p{j}", p)
                        c.get_detached_model_parameters = types.MethodType(node["get_detached_model_parameters"], c)
                        before = len(s._received_messages)
                        comm(c, s)
                        assert len(s._received_messages) == before + 1, "the client skipped the round"
                        m = s._received_messages[-1]
                        flat = torch.cat([g.reshape(-1) for g in m["gradients"]]).numpy()
                        # top-k keeps the K largest values (compressors.py:294-295, an unstable argsort): the K-th
                        # must be unique, or the reference has a choice among ties
                        srt = np.sort(flat)
                        K = flat.size // 100
                        assert srt[-K] != srt[-K - 1] and srt[-K] != srt[-K + 1], "a tie at the top-k threshold"
                        out = flat
                        comps = reference_round_compressors(ref, codec, flat.size)
                        for comp in comps:
                            out = comp.compressVector(out)
                        stats.append([float(comp.last_need_to_send_advance) for comp in comps]
                                     + [float(comp.total_input_components) for comp in comps])
                        out_t = torch.from_numpy(np.ascontiguousarray(out, dtype=np.float32))
                        gs, off = [], 0
                        for g in m["gradients"]:
                            gs.append(out_t[off:off + g.numel()].reshape(g.shape).clone())
                            off += g.numel()
                        m["gradients"] = gs
                    upd(s)
                    key = vr_codec_key(name, codec, nm, tag)
                    put(key + "|theta", list(s.model.parameters()))
                    put(key + "|grad", [p.grad for p in s.model.parameters()])
                    store[key + "|stats"] = np.array(stats, dtype=np.float64)
                    store[key + "|next_random"] = np.array(random.random())
                    store[key + "|next_np"] = np.array(np.random.random_sample())
    np.savez_compressed(OUT / "vr_codec.npz", **store)
    print("vr_codec.npz:", len(store), "arrays")


def main() -> int:
    if not REF.exists():
        print("reference not present; nothing to do", file=sys.stderr)
        return 1
    torch.set_num_threads(1)
    gen_vr_codec()
    return 0


if __name__ == "__main__":
    sys.exit(main())
