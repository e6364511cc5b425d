"""The server optimiser steps in every fold, bit for bit against the stepwise reference
(oracle/server_steps_exact.py) on the edge catalogue of tests/step_cases.py: flc_fedopt_step (fp32 / fp64),
flc_model_fold's three code paths (float4, the n % 4 tail, the unaligned scalar path; 0, 1, 3 and 17 messages), the
sparse, stacked and dense record folds (ModelIO::store's float4 and per-component paths), flc_feddr_combine,
flc_model_fold_server (FedDyn / pFedMe, the fold form and the !FOLD form of a chained round) and one pass through
aggregation.fedopt_update.  A NaN lane must be NaN on both sides (payload and sign not pinned); +-0, +-inf and every
finite value are exact.  tests/test_step_cases.py shows on the CPU that each documented way of getting the arithmetic
subtly wrong changes at least 32 lanes of these vectors."""

import ctypes

import numpy as np
import pytest
import torch

from oracle import server_steps_exact as sx
from tests import step_cases as sc

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
F32, F64 = np.float32, np.float64
STD, NATD, NATURAL = 0, 1, 2
PAD = 7.5  # the guard value around an unaligned view


def _np(t):
    return t.detach().cpu().numpy().reshape(-1).copy()


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def _assert_same(got, want, what):
    got = _np(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    bad = np.flatnonzero(sc.differing(got, want))
    assert bad.size == 0, (what, f"{bad.size} lanes differ", bad[:6].tolist(), got[bad[:6]].tolist(),
                           np.asarray(want)[bad[:6]].tolist())


class _Views:
    """Device tensors holding the given arrays: lead 0, each in an allocation of its own (16-B aligned); lead 1, a view
    one element into a guarded buffer (4-B aligned only)."""

    def __init__(self, arrays, lead):
        self.lead, self.bufs, self.ts = lead, [], []
        for a in arrays:
            n = a.size
            buf = torch.full((n + lead + 4,), PAD, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
            t = buf[lead:lead + n]
            t.copy_(torch.from_numpy(np.array(a, copy=True)))
            assert (t.data_ptr() % 16 == 0) == (lead == 0)
            self.bufs.append(buf)
            self.ts.append(t)

    def check_guards(self):
        for buf, t in zip(self.bufs, self.ts):
            g = _np(buf)
            assert np.all(g[:self.lead] == PAD) and np.all(g[self.lead + t.numel():] == PAD)


def _model_state(sizes):
    """theta, delta, v of a model of the given tensor sizes: tensor 0 is the whole catalogue, the others its leading
    lanes (the special-value cross product, the ties ...)."""
    th, d, v = sc.fedopt_case(F32)
    starts = [0, 0, 250][:len(sizes)]
    return [[a[s:s + n] for s, n in zip(starts, sizes)] for a in (th, d, v)]


# ------------------------------------------------------------------------------------------------ flc_fedopt_step
@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("opt", sc.OPTS)
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_fedopt_step(dt, opt, tau):
    from fl_sim_amd import codec

    th, d, v = sc.fedopt_case(dt)
    want_t, want_v = sx.fedopt_step(opt, th, d, v, sc.LR, sc.BETA2, tau, dt)
    g_t, g_d, g_v = _dev(th), _dev(d), _dev(v)
    codec.fedopt_step(g_t, g_d, None if opt == "avg" else g_v, opt, sc.LR, sc.BETA2, tau)
    torch.cuda.synchronize()
    _assert_same(g_t, want_t, "theta")
    _assert_same(g_d, d, "delta")
    _assert_same(g_v, v if opt == "avg" else want_v, "v")


# ------------------------------------------------------------------------------------------------ flc_model_fold
def _fold_plan(count):
    """(init_mode, beta0, weights): no message, delta as it stands (init 2); one message of weight 1 from +0 (init 1:
    the message's edge values land in delta exactly); 3 and 17 messages on delta * 0.9 (init 0)."""
    if count == 0:
        return 2, 0.0, []
    if count == 1:
        return 1, 0.0, [1.0]
    return 0, 0.9, [(1 - 0.9) / count] * count


@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("count", [0, 1, 3, 17])
@pytest.mark.parametrize("opt", sc.OPTS)
def test_model_fold_with_the_step(opt, count, lead, tau):
    from fl_sim_amd import codec

    sizes = sc.SIZES3
    th, d, v = _model_state(sizes)
    init, beta0, ws = _fold_plan(count)
    if count == 1:
        msgs = [d]  # the edge deltas themselves
    else:
        msgs = [sc.cut(m, sizes) for m in sc.messages(count, sum(sizes))]
    g_t, g_d, g_v = _Views(th, lead), _Views(d, lead), _Views(v, lead)
    g_m = [_Views(m, lead) for m in msgs]
    codec.model_fold(g_d.ts, [m.ts for m in g_m], ws, init, beta0, theta=g_t.ts, v=None if opt == "avg" else g_v.ts,
                     opt=opt, lr=sc.LR, beta2=sc.BETA2, tau=tau)
    torch.cuda.synchronize()
    for j in range(len(sizes)):
        want_d = sx.fold_chain(d[j], beta0, [m[j] for m in msgs], ws, init)
        want_t, want_v = sx.fedopt_step(opt, th[j], want_d, v[j], sc.LR, sc.BETA2, tau)
        _assert_same(g_d.ts[j], want_d, ("delta", j))
        _assert_same(g_t.ts[j], want_t, ("theta", j))
        _assert_same(g_v.ts[j], v[j] if opt == "avg" else want_v, ("v", j))
    for g in [g_t, g_d, g_v] + g_m:
        g.check_guards()
    for m, src in zip(g_m, msgs):  # (the messages are read only)
        for t, a in zip(m.ts, src):
            _assert_same(t, a, "message")


# ------------------------------------------------------------------------------------------------ the record folds
def _flat_state(lead):
    """theta, delta, v of the catalogue as three flat device buffers, each cut into sc.SPLIT (tensor borders inside a
    1,024-element tile; with lead 0 tensors 0 and 1 take the float4 path and tensor 2, starting 8 bytes off, the
    per-component one; with lead 1 every tensor does)."""
    arrs = sc.fedopt_case(F32)
    views = _Views(arrs, lead)
    return arrs, views, [sc.cut(t, sc.SPLIT) for t in views.ts]


def _ptrs(ts):
    return (P * len(ts))(*[t.data_ptr() for t in ts])


def _check_record_fold(call, decoded, ws, beta0, opt, tau, lead, delta0=None):
    """``call(delta, theta, v)`` runs the fused fold on the three-tensor state; expected: fold_chain over the decoded
    records, then fedopt_step."""
    (th, d, v), views, (t_t, t_d, t_v) = _flat_state(lead)
    if delta0 is not None:
        d = delta0
        views.ts[1].copy_(torch.from_numpy(np.array(d, copy=True)))
    call(t_d, t_t, None if opt == "avg" else t_v)
    torch.cuda.synchronize()
    want_d = sx.fold_chain(d, beta0, decoded, ws, 0)
    want_t, want_v = sx.fedopt_step(opt, th, want_d, v, sc.LR, sc.BETA2, tau)
    _assert_same(views.ts[1], want_d, "delta")
    _assert_same(views.ts[0], want_t, "theta")
    _assert_same(views.ts[2], v if opt == "avg" else want_v, "v")
    views.check_guards()


_SPARSE: dict = {}


def _sparse_records(form):
    """"place": three records that place the catalogue's deltas on their lanes (lane i in record i % 3; the third
    takes lane 1 again, with +0, to reach the common k).  "touch": three records of gaussian and edge values on lanes
    i % 7 == r, so lanes 3..6 mod 7 are named by no record."""
    from fl_sim_amd import _lib, codec

    if form not in _SPARSE:
        n = sc.N
        d = sc.fedopt_case(F32)[1]
        idxs, vals = [], []
        for r in range(3):
            if form == "place":
                idx = np.arange(r, n, 3)
                val = d[idx].copy()
                if r == 2:
                    idx, val = np.concatenate([[1], idx]), np.concatenate([[F32(0)], val])
            else:
                idx = np.arange(r, n, 7)
                val = sc.messages(3, n, seed=9)[r][idx].copy()
            idxs.append(idx)
            vals.append(val.astype(F32))
        k = len(idxs[0])
        assert all(len(i) == k for i in idxs)
        stride, _ = codec.sparse_wire_layout(n, k)
        wires = torch.full((3, stride), 0xAB, dtype=torch.uint8, device="cuda")
        for r in range(3):
            ri, rv, rt = codec.sparse_wire_views(wires[r], n, k)
            ri.copy_(torch.from_numpy(idxs[r].astype(np.int32)))
            rv.copy_(torch.from_numpy(vals[r]))
            _lib.call("flc_tile_index", ri.data_ptr(), k, n, rt.data_ptr(), codec._stream(wires.device))
        torch.cuda.synchronize()
        decoded = [_np(codec.sparse_record_decode(wires[r], n, k)) for r in range(3)]
        _SPARSE[form] = (wires, k, decoded)
    return _SPARSE[form]


@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("opt", sc.OPTS)
@pytest.mark.parametrize("form", ["place", "touch"])
def test_fedopt_fold_sparse_records(form, opt, lead, tau):
    from fl_sim_amd import _lib

    wires, k, decoded = _sparse_records(form)
    n = sc.N
    d = sc.fedopt_case(F32)[1]
    if form == "place":  # w = 1, beta0 = 0, delta0 = 0: delta becomes the records' values exactly
        ws, beta0, delta0 = [1.0, 1.0, 1.0], 0.0, np.zeros(n, dtype=F32)
        placed = sx.fold_chain(delta0, beta0, decoded, ws, 0)
        nz = d != 0
        assert sc.same(placed[nz], d[nz]) and np.all(placed[~nz] == 0)
    else:  # beta0 = 1: the edge values of delta0 on lanes the records name and on lanes they do not
        ws, beta0, delta0 = [1.0, 0.37, -1.5], 1.0, None

    def call(delta, theta, v):
        T = len(sc.SPLIT)
        _lib.call("flc_fedopt_fold_sparse_records", (P * 3)(*[wires[r].data_ptr() for r in range(3)]),
                  (ctypes.c_float * 3)(*ws), 3, n, k, _ptrs(delta), _ptrs(theta), None if v is None else _ptrs(v),
                  (ctypes.c_int64 * T)(*sc.SPLIT), T, beta0, _lib.FLC_OPT[opt], sc.LR, sc.BETA2, tau, None)

    _check_record_fold(call, decoded, ws, beta0, opt, tau, lead, delta0)


_STACKED: dict = {}


def _stacked_records():
    """Three stacked records (top-k + 127-level dithering) whose kept sets are the lanes i % 5 == r."""
    from fl_sim_amd import codec

    if not _STACKED:
        n = sc.N
        k = len(range(0, n, 5))
        stride, _ = codec.stacked_wire_layout(n, k)
        wires = torch.zeros(3, stride, dtype=torch.uint8, device="cuda")
        decoded = []
        for r in range(3):
            x = np.array(sc.messages(3, n, seed=11)[r], copy=True)
            x = np.where(np.abs(x) < 0.01, x, F32(1e-3)).astype(F32)  # (NaN, +-inf and the large values included)
            x[r::5] = np.where(np.abs(x[r::5]) < 1e-6, F32(1.0), x[r::5] * F32(1000))
            codec.stacked_encode(_dev(x), k, 127, seed=5 + r, counter=3, wire=wires[r])
            decoded.append(_np(codec.stacked_decode(codec.wire_packet(wires[r], n, k))))
        torch.cuda.synchronize()
        assert all(np.count_nonzero(dec) > k // 2 for dec in decoded)
        _STACKED["x"] = (wires, k, decoded)
    return _STACKED["x"]


@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("opt", sc.OPTS)
@pytest.mark.parametrize("beta0", [1.0, 0.9])
def test_fedopt_fold_stacked_records(beta0, opt, lead, tau):
    from fl_sim_amd import _lib

    wires, k, decoded = _stacked_records()
    ws = [1.0, 0.37, -1.5]

    def call(delta, theta, v):
        T = len(sc.SPLIT)
        _lib.call("flc_fedopt_fold_records", (P * 3)(*[wires[r].data_ptr() for r in range(3)]),
                  (ctypes.c_float * 3)(*ws), 3, sc.N, k, 127, _ptrs(delta), _ptrs(theta),
                  None if v is None else _ptrs(v), (ctypes.c_int64 * T)(*sc.SPLIT), T, beta0, _lib.FLC_OPT[opt], sc.LR,
                  sc.BETA2, tau, None)

    _check_record_fold(call, decoded, ws, beta0, opt, tau, lead)


DENSE_FORMATS = [(STD, 4, 7), (NATD, 8, 8), (NATURAL, 16, 0)]
_DENSE: dict = {}


def _dense_records(fmt):
    """Three dense records of inputs that are exactly zero on the even lanes (code 0 decodes to +0: fmaf(w, +0, a)
    leaves every a but -0 as it is)."""
    from fl_sim_amd import _lib, codec

    if fmt not in _DENSE:
        kind, bits, s = fmt
        n = sc.N
        stride, _ = codec.dense_wire_layout(n, kind, bits)
        wires = torch.full((3, stride), 0xAB, dtype=torch.uint8, device="cuda")
        st = codec._stream(wires.device)
        decoded = []
        for r in range(3):
            x = np.array(sc.messages(3, n, seed=13)[r], copy=True)
            x = np.where(np.abs(x) < 0.01, x, F32(2e-3)).astype(F32)  # (NaN, +-inf and the large values included)
            x[0::2] = 0
            xd = _dev(x)
            norm, codes = codec.dense_wire_views(wires[r], n, kind, bits)
            out = torch.empty(n, dtype=torch.float32, device="cuda")
            if kind == NATURAL:
                ws_ = codec.workspace(xd.device, codec._ws_size(xd.device, "flc_natural_workspace_size", n), "natural")
                _lib.call("flc_natural_encode", xd.data_ptr(), n, 7 + r, 3, None, codes.data_ptr(), None,
                          ws_.data_ptr(), ws_.numel(), st)
                _lib.call("flc_natural_decode", codes.data_ptr(), n, 1.0, 0, out.data_ptr(), st)
            else:
                ws_ = codec.workspace(xd.device, codec._ws_size(xd.device, "flc_quant_workspace_size", 1, n), "quant")
                _lib.call("flc_quant_norm", xd.data_ptr(), 1, n, _lib.FLC_NORM_INF, norm.data_ptr(), ws_.data_ptr(),
                          ws_.numel(), st)
                _lib.call("flc_quant_encode", xd.data_ptr(), 1, n, kind, s, bits, norm.data_ptr(), 7 + r, 3, None,
                          codes.data_ptr(), None, ws_.data_ptr(), ws_.numel(), st)
                _lib.call("flc_quant_decode", codes.data_ptr(), 1, n, kind, s, bits, norm.data_ptr(), None, 0,
                          out.data_ptr(), st)
            torch.cuda.synchronize()
            decoded.append(_np(out))
            assert np.all(decoded[-1][0::2] == 0) and np.count_nonzero(decoded[-1]) > n // 16
        _DENSE[fmt] = (wires, decoded)
    return _DENSE[fmt]


@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("opt", sc.OPTS)
@pytest.mark.parametrize("beta0", [1.0, 0.9])
@pytest.mark.parametrize("fmt", DENSE_FORMATS, ids=["std4s7", "natd8s8", "natural"])
def test_fedopt_fold_dense_records(fmt, beta0, opt, lead, tau):
    from fl_sim_amd import _lib

    kind, bits, s = fmt
    wires, decoded = _dense_records(fmt)
    ws = [1.0, 0.37, -1.5]

    def call(delta, theta, v):
        T = len(sc.SPLIT)
        _lib.call("flc_fedopt_fold_dense_records", (P * 3)(*[wires[r].data_ptr() for r in range(3)]),
                  (ctypes.c_float * 3)(*ws), 3, sc.N, kind, s, bits, _ptrs(delta), _ptrs(theta),
                  None if v is None else _ptrs(v), (ctypes.c_int64 * T)(*sc.SPLIT), T, beta0, _lib.FLC_OPT[opt], sc.LR,
                  sc.BETA2, tau, None)

    _check_record_fold(call, decoded, ws, beta0, opt, tau, lead)


# ------------------------------------------------------------------------------------------------ flc_feddr_combine
@pytest.mark.parametrize("params", [0, 1])
@pytest.mark.parametrize("prox", sc.PROXES, ids=["none", "l1", "scale"])
@pytest.mark.parametrize("dt", [F32, F64], ids=["f32", "f64"])
def test_feddr_combine(dt, prox, params):
    from fl_sim_amd import codec

    p = sc.FEDDR_PARAMS[params]
    pc = 1 / (1 + 2 * p["pc"]) if prox == sx.PROX_SCALE else p["pc"]
    th, y, x = sc.feddr_case(dt)
    want_t, want_y = sx.feddr_combine(th, y, x, p["alpha"], p["cx"], p["cy"], prox, pc, dt)
    if prox == sx.PROX_L1 and params == 0:  # the lanes the catalogue is for are there
        t = sx.feddr_combine(th, y, x, p["alpha"], p["cx"], p["cy"], sx.PROX_NONE, pc, dt)[0]
        assert (np.abs(t) == dt(pc)).sum() >= 16 and (t == 0).sum() >= 128 and np.isnan(t).sum() >= 96
    g_t, g_y, g_x = _dev(th), _dev(y), _dev(x)
    codec.feddr_combine(g_t, g_y, g_x, p["alpha"], p["cx"], p["cy"], prox, pc)
    torch.cuda.synchronize()
    _assert_same(g_y, want_y, "y")
    _assert_same(g_t, want_t, "theta")
    _assert_same(g_x, x, "x_til")


# ------------------------------------------------------------------------------------------------ FedDyn, pFedMe
def _server_state(sizes):
    n = sum(sizes)
    th0 = sc.messages(1, n, seed=5)[0]
    h = np.concatenate([sc.fedopt_case(F32)[1], sc.fedopt_case(F32)[1][:n - sc.N]])
    return sc.cut(th0, sizes), sc.cut(h, sizes)


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("count", [1, 3, 17])
def test_model_fold_server_feddyn(count, lead):
    from fl_sim_amd import codec

    sizes, c = sc.SIZES3, -0.1 / 10
    th0, h0 = _server_state(sizes)
    msgs = [sc.cut(m, sizes) for m in sc.messages(count, sum(sizes))]
    ws = [1 / count] * count
    g_t, g_h = _Views(th0, lead), _Views(h0, lead)
    g_m = [_Views(m, lead) for m in msgs]
    srcs = [m.ts for m in g_m]
    cap = codec.MODEL_FOLD_MAX_SRC
    if count <= cap:
        codec.model_fold_server(g_t.ts, g_h.ts, srcs, ws, "feddyn", True, 0, 0.0, c)
    else:  # h in chained launches against the unchanged model, then the chained average (aggregation.feddyn_update)
        for c0 in range(0, count, cap):
            codec.model_fold_server(g_t.ts, g_h.ts, srcs[c0:c0 + cap], ws[c0:c0 + cap], "feddyn", False, 0, 0.0, c)
        torch.cuda.synchronize()
        for j in range(len(sizes)):
            _assert_same(g_t.ts[j], th0[j], ("theta untouched", j))
        codec.model_fold(g_t.ts, srcs, ws, 0, 0.0)
    torch.cuda.synchronize()
    for j in range(len(sizes)):
        want_t, want_h = sx.server_fold("feddyn", th0[j], h0[j], [m[j] for m in msgs], ws, c)
        _assert_same(g_h.ts[j], want_h, ("h", count, j))
        _assert_same(g_t.ts[j], want_t, ("theta", count, j))
    for g in [g_t, g_h] + g_m:
        g.check_guards()


@pytest.mark.parametrize("lead", [0, 1], ids=["aligned", "offset4"])
@pytest.mark.parametrize("count", [0, 1, 3, 17])
def test_model_fold_server_pfedme(count, lead):
    from fl_sim_amd import codec

    sizes, beta = sc.SIZES3, 0.7
    th0, _ = _server_state(sizes)
    msgs = [sc.cut(m, sizes) for m in sc.messages(count, sum(sizes))]
    ws = [1 / count] * count if count else []  # (no message: the blend of the model with itself, init 2)
    g_t = _Views(th0, lead)
    g_m = [_Views(m, lead) for m in msgs]
    srcs = [m.ts for m in g_m]
    if count <= codec.MODEL_FOLD_MAX_SRC:
        codec.model_fold_server(g_t.ts, g_t.ts, srcs, ws, "pfedme", True, 0 if count else 2, 0.0, beta)
    else:  # the model saved, the chained average, then the blend alone (aggregation.pfedme_update)
        saved = _Views(th0, lead)
        codec.model_fold(g_t.ts, srcs, ws, 0, 0.0)
        codec.model_fold_server(g_t.ts, saved.ts, [], [], "pfedme", False, 2, 0.0, beta)
        torch.cuda.synchronize()
        for j in range(len(sizes)):
            _assert_same(saved.ts[j], th0[j], ("saved", j))
        saved.check_guards()
    torch.cuda.synchronize()
    for j in range(len(sizes)):
        want_t, _ = sx.server_fold("pfedme", th0[j], None, [m[j] for m in msgs], ws, beta, True, 0 if count else 2)
        _assert_same(g_t.ts[j], want_t, ("theta", count, j))
    for g in [g_t] + g_m:
        g.check_guards()


# ------------------------------------------------------------------------------------------------ the Python layer
@pytest.mark.parametrize("opt", sc.OPTS)
def test_fedopt_update_forms_the_scalars_as_the_reference_does(opt):
    """aggregation.fedopt_update on device tensors: alpha = (1 - beta1) / len(messages), lr, beta2, 1 - beta2 and tau
    reach the kernel as the reference's torch ops would cast them."""
    from fl_sim_amd import aggregation

    sizes = sc.SIZES3
    th, d, v = _model_state(sizes)
    beta1, count = 0.9, 3
    msgs = [sc.cut(m, sizes) for m in sc.messages(count, sum(sizes))]
    g_t, g_d, g_v = ([_dev(a) for a in grp] for grp in (th, d, v))
    messages = [{"delta_parameters": [_dev(a) for a in m], "train_samples": 10} for m in msgs]
    aggregation.fedopt_update(g_t, g_d, None if opt == "avg" else g_v, messages, opt, sc.LR, (beta1, sc.BETA2),
                              sc.TAUS[0])
    torch.cuda.synchronize()
    alpha = (1 - beta1) / count
    for j in range(len(sizes)):
        want_d = sx.fold_chain(d[j], beta1, [m[j] for m in msgs], [alpha] * count, 0)
        want_t, want_v = sx.fedopt_step(opt, th[j], want_d, v[j], sc.LR, sc.BETA2, sc.TAUS[0])
        _assert_same(g_d[j], want_d, ("delta", j))
        _assert_same(g_t[j], want_t, ("theta", j))
        _assert_same(g_v[j], v[j] if opt == "avg" else want_v, ("v", j))
