"""The contract of fl_sim_amd._flcfold (csrc/pyfold.cpp) on a device, entry by entry: which exception a tensor of
the wrong dtype, layout or size raises in each argument position, what a short, misaligned or mistyped record raises,
and that a rejected call launched and allocated nothing — every tensor of the call still holds, bit for bit, what it
held before, and no reference count moved (tests/pyfold_cases.py).  Every rejection here is made by the host checks,
before any launch.  The success paths are run once each for their reference counts and return values; what they
compute is the parity suites' business.  The model has a zero-element tensor and sizes that are no multiple of 4."""

import math

import pytest
import torch

from fl_sim_amd import _flcfold as fold
from fl_sim_amd import _lib, codec
from tests.pyfold_cases import FOLD, SRV, STEP, accepted, rejected, snapshot, unchanged

pytestmark = pytest.mark.gpu

SHAPES = [(5,), (0,), (3, 1)]
N, K, S = 8, 2, 127  # the flat model, the kept entries, the levels
FMT, BITS = _lib.FLC_Q_STANDARD_DITHER, 8


def dev(i=0):
    return torch.device("cuda", i)


def model(fill=1.0, d=None):
    d = d or dev()
    return [torch.arange(math.prod(s), dtype=torch.float32, device=d).reshape(s) + fill for s in SHAPES]


def bad_tensors(ts):
    """(kind, copy of the list ``ts`` with one tensor spoilt) for float64, non-contiguous and wrong-size tensors, in
    the first and the last position."""
    for i in (0, len(ts) - 1):
        t = ts[i]
        for kind, b in (("dtype", t.double()),
                        ("layout", torch.zeros(2 * t.numel(), device=t.device)[::2].reshape(t.shape)),
                        ("size", torch.zeros(t.numel() + 1, device=t.device))):
            assert kind != "layout" or not b.is_contiguous()
            out = list(ts)
            out[i] = b
            yield kind, out


def stride():
    return codec.stacked_wire_layout(N, K)[0]


def record(nbytes=None, offset=0):
    """An all-zero uint8 tensor of the record's size (or ``nbytes``), ``offset`` bytes into a 16-B aligned buffer."""
    nbytes = stride() if nbytes is None else nbytes
    r = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev())[offset:offset + nbytes]
    assert r.data_ptr() % 16 == offset % 16 and r.is_contiguous()
    return r


def bad_records():
    yield record(stride() - 1)  # one byte short
    yield record(offset=4)  # misaligned
    yield torch.zeros(stride(), dtype=torch.int8, device=dev())  # not uint8
    yield torch.zeros(stride(), dtype=torch.uint8)  # on the host


def stacked_ws(call, *a):
    return codec.workspace(dev(), codec._ws_size(dev(), call, *a), "topk_batch" if "batch" in call else "topk")


@pytest.fixture(scope="module")
def stacked_rec():
    """One valid stacked record of (N, K, S), made by stacked_delta_record — its success path."""
    loc, glo, r = model(3.0), model(1.0), record()
    cnt = torch.zeros(1, dtype=torch.int64, device=dev())
    ws = stacked_ws("flc_stacked_encode_delta_workspace_size", N, K, len(loc))
    assert accepted(fold.stacked_delta_record, loc, glo, K, S, 7, 1, r, cnt, ws) is None
    assert accepted(fold.stacked_delta_record, loc, glo, K, S, 7, 1, record(), None, ws) is None
    torch.cuda.synchronize()
    assert 0 <= int(cnt.item()) <= K
    return r


@pytest.fixture(scope="module")
def dense_rec():
    r = torch.zeros(codec.dense_wire_layout(N, FMT, BITS)[0], dtype=torch.uint8, device=dev())
    codec.quant_encode_round([torch.cat([t.reshape(-1) for t in model(2.0)])], FMT, S, BITS, _lib.FLC_NORM_INF, [7], [1],
                             [r])
    return r


def test_model_fold():
    d, m, th, v = model(), model(2.0), model(3.0), model(4.0)
    snap = snapshot(d, m, th, v)
    call = fold.model_fold
    tail = lambda th_, v_: (0, 0.0, th_, v_, 3, 1.0, 0.9, 1e-3)  # noqa: E731
    for kind, b in bad_tensors(d):  # (the model's sizes are the measure: a wrong one shows at the first message)
        exc, text = (ValueError, "message tensors must match") if kind == "size" else (TypeError, "model tensors")
        rejected(exc, text, call, b, [m], None, [0.5], *FOLD)
    for kind, b in bad_tensors(th):
        exc, text = (ValueError, "theta / v must match") if kind == "size" else (TypeError, "theta / v tensors")
        rejected(exc, text, call, d, [m], None, [0.5], *tail(b, v))
        rejected(exc, text, call, d, [m], None, [0.5], *tail(th, b))
    rejected(ValueError, "theta / v need one tensor", call, d, [m], None, [0.5], *tail(th[:2], v))
    rejected(TypeError, "theta / v must be sequences", call, d, [m], None, [0.5], *tail(5, v))
    for kind, b in bad_tensors(m):
        exc, text = (ValueError, "message tensors must match") if kind == "size" else (TypeError, "message tensors")
        rejected(exc, text, call, d, [m, b], None, [0.5, 0.5], *FOLD)
        rejected(exc, text, call, d, [{"p": m}, {"p": b}], "p", [0.5, 0.5], *FOLD)
    rejected(ValueError, "one tensor per model tensor", call, d, [m[:2]], None, [0.5], *FOLD)
    rejected(KeyError, "q", call, d, [{"p": m}], "q", [0.5], *FOLD)
    rejected(TypeError, "", call, d, [m], None, ["x"], *FOLD)  # (a weight that is no number)
    # two errors: theta is checked before the messages, a message's tensors in order
    rejected(TypeError, "theta / v tensors", call, d, [m[:2]], None, [0.5], *tail([t.double() for t in th], v))
    rejected(TypeError, "message tensors", call, d, [[m[0].double(), m[1], torch.zeros(4, device=dev())]], None, [0.5],
             *FOLD)
    unchanged(snap)
    assert accepted(call, d, [m, m], None, [0.5, 0.25], *FOLD) is None
    assert accepted(call, d, [{"p": m}] * 17, "p", [0.5] * 17, *tail(th, v)) is None  # (chained launches)


def test_server_fold():
    th, aux, m = model(), model(2.0), model(3.0)
    snap = snapshot(th, aux, m)
    call = fold.server_fold
    for kind, b in bad_tensors(th):
        exc, text = (ValueError, "aux tensors must match") if kind == "size" else (TypeError, "model tensors")
        rejected(exc, text, call, b, aux, [m], None, [0.5], *SRV)
    for kind, b in bad_tensors(aux):
        exc, text = (ValueError, "aux tensors must match") if kind == "size" else (TypeError, "aux tensors")
        rejected(exc, text, call, th, b, [m], None, [0.5], *SRV)
    for kind, b in bad_tensors(m):
        exc, text = (ValueError, "message tensors must match") if kind == "size" else (TypeError, "message tensors")
        rejected(exc, text, call, th, aux, [m, b], None, [0.5, 0.5], *SRV)
        rejected(exc, text, call, th, aux, [{"p": b}], "p", [0.5], *SRV)
    rejected(ValueError, "one tensor per model tensor", call, th, aux, [m[:2]], None, [0.5], *SRV)
    # two errors: theta and aux are checked tensor by tensor together, both before the messages
    rejected(TypeError, "aux tensors", call, th[:2] + [th[2].double()], [aux[0].double()] + aux[1:], [m[:2]], None,
             [0.5], *SRV)
    unchanged(snap)
    assert accepted(call, th, aux, [m, m], None, [0.5, 0.5], *SRV) is None


def _check_views(out, params, set_grad):
    views, flat = out
    assert isinstance(views, list) and flat.dtype == torch.float32 and flat.numel() == N and flat.device == params[0].device
    off = 0
    for v, p in zip(views, params):
        assert v.shape == p.shape
        assert v.numel() == 0 or v.data_ptr() == flat.data_ptr() + 4 * off  # (the view aliases the flat buffer)
        assert v.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        assert (p.grad is v) if set_grad else (p.grad is None)
        off += p.numel()


def test_avg_and_gradients():
    p, g = model(), model(9.0)
    msg = {"parameters": model(2.0), "gradients": model(3.0)}
    snap = snapshot(p, g, msg["parameters"], msg["gradients"])
    call = fold.avg_and_gradients
    for kind, b in bad_tensors(p):
        exc, text = (ValueError, "gradient buffers must match") if kind == "size" else (TypeError, "model tensors")
        rejected(exc, text, call, b, g, [msg], [0.5], [0.5], 0.0)
        exc, text = (ValueError, "message tensors must match") if kind == "size" else (TypeError, "model tensors")
        rejected(exc, text, call, b, None, [msg], [0.5], [0.5], 0.0, True)
    for kind, b in bad_tensors(g):
        exc, text = (ValueError, "gradient buffers must match") if kind == "size" else (TypeError, "gradient buffers")
        rejected(exc, text, call, p, b, [msg], [0.5], [0.5], 0.0)
    for key in ("parameters", "gradients"):
        for kind, b in bad_tensors(msg[key]):
            exc, text = (ValueError, "message tensors must match") if kind == "size" else (TypeError, "message tensors")
            rejected(exc, text, call, p, g, [msg, {**msg, key: b}], [0.5, 0.5], [0.5, 0.5], 0.0)
            rejected(exc, text, call, p, None, [{**msg, key: b}], [0.5], [0.5], 0.0, True)
    rejected(ValueError, "one tensor per model tensor", call, p, g, [{**msg, "gradients": model()[:2]}], [0.5], [0.5], 0.0)
    rejected(KeyError, "gradients", call, p, None, [{"parameters": msg["parameters"]}], [0.5], [0.5], 0.0, True)
    # two errors: a message's parameters are checked before its gradients
    rejected(TypeError, "message tensors", call, p, g,
             [{"parameters": [t.double() for t in msg["parameters"]], "gradients": model()[:2]}], [0.5], [0.5], 0.0)
    unchanged(snap)
    assert all(t.grad is None for t in p)  # (nothing was attached by a rejected set_grad call)
    assert accepted(call, p, g, [msg], [0.5], [0.5], 0.0) is None
    _check_views(accepted(call, p, None, [msg, msg], [0.5, 0.5], [0.5, 0.5], 0.0), p, False)
    _check_views(accepted(call, p, None, [msg], [0.5], [0.5], 0.0, False), p, False)
    out = accepted(call, p, None, [msg], [1.0], [1.0], 0.0, True)
    _check_views(out, p, True)
    torch.cuda.synchronize()
    assert torch.equal(out[1], torch.cat([t.reshape(-1) for t in msg["gradients"]]))


def test_stacked_delta_record(stacked_rec):
    loc, glo, r = model(3.0), model(1.0), record()
    cnt = torch.zeros(1, dtype=torch.int64, device=dev())
    ws = stacked_ws("flc_stacked_encode_delta_workspace_size", N, K, len(loc))
    snap = snapshot(loc, glo, r, cnt, stacked_rec)
    call = fold.stacked_delta_record
    for kind, b in bad_tensors(loc):
        exc, text = (ValueError, "matching sizes") if kind == "size" else (TypeError, "local / global tensors")
        rejected(exc, text, call, b, glo, K, S, 7, 1, r, cnt, ws)
        rejected(exc, text, call, loc, b, K, S, 7, 1, r, cnt, ws)
    bad = list(bad_records())
    for b in bad[:2]:
        rejected(ValueError, "smaller than the wire layout or not 16-B aligned", call, loc, glo, K, S, 7, 1, b, cnt, ws)
    for b in bad[2:] + [5]:
        rejected(TypeError, "the record must be", call, loc, glo, K, S, 7, 1, b, cnt, ws)
    for b in (cnt.int(), cnt[:0], cnt.cpu(), 5):
        rejected(TypeError, "count must be an int64", call, loc, glo, K, S, 7, 1, r, b, ws)
    for b in (ws.view(torch.int8), ws.cpu(), None):
        rejected(TypeError, "ws must be", call, loc, glo, K, S, 7, 1, r, cnt, b)
    # two errors: the record before the count before the workspace
    rejected(ValueError, "smaller than the wire layout", call, loc, glo, K, S, 7, 1, bad[0], cnt.int(), None)
    rejected(TypeError, "count must be an int64", call, loc, glo, K, S, 7, 1, r, cnt.int(), None)
    unchanged(snap)


def test_delta_flat():
    loc, glo = model(3.0), model(1.0)
    snap = snapshot(loc, glo)
    for kind, b in bad_tensors(loc):
        exc, text = (ValueError, "matching sizes") if kind == "size" else (TypeError, "local / global tensors")
        rejected(exc, text, fold.delta_flat, b, glo)
        rejected(exc, text, fold.delta_flat, loc, b)
    # two errors: the tensors in order
    rejected(TypeError, "local / global tensors", fold.delta_flat, [loc[0].double(), loc[1]], [glo[0], glo[0]])
    unchanged(snap)
    out = accepted(fold.delta_flat, loc, glo)
    assert out.shape == (N,) and out.dtype == torch.float32 and out.device == loc[0].device
    assert torch.equal(out, torch.full((N,), 2.0, device=dev()))
    e = torch.zeros(0, device=dev())
    out = accepted(fold.delta_flat, [e, e.reshape(0, 2)], [e, e.reshape(0, 2)])
    assert out.shape == (0,) and out.dtype == torch.float32 and out.device == e.device


def test_ef_accumulate():
    loc, glo, e = model(3.0), model(1.0), torch.ones(N, device=dev())
    snap = snapshot(loc, glo, e)
    call = fold.ef_accumulate
    for b in (e.double(), torch.zeros(2 * N, device=dev())[::2]):
        rejected(TypeError, "the memory must be", call, loc, glo, b)
    rejected(ValueError, "the memory must hold", call, loc, glo, torch.zeros(N + 1, device=dev()))
    rejected(ValueError, "the memory must hold", call, loc, None, torch.zeros(N - 1, device=dev()))
    for kind, b in bad_tensors(loc):
        exc, text = (ValueError, "matching sizes") if kind == "size" else (TypeError, "local / global tensors")
        rejected(exc, text, call, b, glo, e)
        rejected(exc, text, call, loc, b, e)
        if kind != "size":
            rejected(exc, text, call, b, None, e)
    rejected(TypeError, "local must be a sequence", call, 5, glo, e)
    rejected(TypeError, "global must be a sequence", call, loc, 5, e)
    rejected(ValueError, "one global tensor per local tensor", call, loc, glo[:2], e)
    rejected(ValueError, "one global tensor per local tensor", call, [], None, e)
    # two errors: the lists' sizes before the memory's
    rejected(ValueError, "matching sizes", call, loc, [glo[0], glo[1], glo[0]], torch.zeros(1, device=dev()))
    unchanged(snap)
    assert accepted(call, loc, glo, e) is None
    assert accepted(call, loc, None, e) is None
    assert torch.equal(e, 3.0 + torch.cat([t.reshape(-1) for t in loc]))


def test_stacked_records_round(stacked_rec):
    x = [torch.cat([a.reshape(-1) - b.reshape(-1) for a, b in zip(model(3.0), model(1.0))]) for _ in range(2)]
    r = torch.zeros(2, stride(), dtype=torch.uint8, device=dev())
    cnt = [torch.zeros(1, dtype=torch.int64, device=dev()) for _ in range(2)]
    ws = stacked_ws("flc_stacked_encode_batch_workspace_size", N, K, 2)
    snap = snapshot(x, r, cnt)
    call = fold.stacked_records_round
    for b in (x[1].double(), torch.zeros(2 * N, device=dev())[::2]):
        rejected(TypeError, "flat deltas must be", call, [x[0], b], [1, 2], [3, 4], K, S, r, cnt, ws)
    rejected(ValueError, "flat deltas must all have one size", call, [x[0], torch.zeros(N + 1, device=dev())], [1, 2],
             [3, 4], K, S, r, cnt, ws)
    for b in (cnt[1].int(), cnt[1][:0], cnt[1].cpu(), 5):
        rejected(TypeError, "counts must be int64", call, x, [1, 2], [3, 4], K, S, r, [cnt[0], b], ws)
    rejected(TypeError, "", call, x, [1, "x"], [3, 4], K, S, r, cnt, ws)  # (a seed that is no integer)
    rejected(TypeError, "records must be a uint8 HIP tensor", call, x, [1, 2], [3, 4], K, S, [r[0], r[1]], cnt, ws)
    block = "records must be a contiguous [clients"
    wide = torch.zeros(2, stride() + 8, dtype=torch.uint8, device=dev())
    for b in (torch.zeros(3, stride(), dtype=torch.uint8, device=dev()), wide, r.view(torch.int8), r.cpu(), r[0],
              wide[:, :stride()], r[:, :stride() - 16]):
        rejected(ValueError, block, call, x, [1, 2], [3, 4], K, S, b, cnt, ws)
    rejected(ValueError, "bad wire shape", call, [x[0][:0], x[1][:0]], [1, 2], [3, 4], 0, S, r, cnt, ws)
    for b in (ws.view(torch.int8), ws.cpu(), None):
        rejected(TypeError, "ws must be", call, x, [1, 2], [3, 4], K, S, r, cnt, b)
    # two errors: the deltas and counts before the block before the workspace
    rejected(TypeError, "counts must be int64", call, x, [1, 2], [3, 4], K, S, wide, [cnt[0], 5], None)
    rejected(ValueError, block, call, x, [1, 2], [3, 4], K, S, wide, cnt, None)
    unchanged(snap)
    assert accepted(call, x, [7, 7], [1, 1], K, S, r, cnt, ws) is None
    torch.cuda.synchronize()
    # (the same delta, seed and counter as the one-message record: the rows are that record)
    assert torch.equal(r[0], stacked_rec) and torch.equal(r[1], stacked_rec)


@pytest.mark.parametrize("dense", [False, True])
def test_fold_records(dense, stacked_rec, dense_rec):
    d, th, v = model(), model(2.0), model(3.0)
    good = dense_rec if dense else stacked_rec
    snap = snapshot(d, th, v, good)
    call = fold.fold_dense_records if dense else fold.fold_records
    shape = (N, FMT, S, BITS) if dense else (N, K, S)
    tail = lambda th_, v_: (th_, v_, 0.0, 3, 1.0, 0.9, 1e-3)  # noqa: E731
    for kind, b in bad_tensors(d):
        text = "do not hold the records' element count" if kind == "size" else "server tensors must be"
        rejected(TypeError, text, call, [good], [0.5], *shape, b, None, None, *STEP)
    for kind, b in bad_tensors(th):
        rejected(TypeError, "theta / v must match", call, [good], [0.5], *shape, d, *tail(b, v))
        rejected(TypeError, "theta / v must match", call, [good], [0.5], *shape, d, *tail(th, b))
    rejected(TypeError, "theta / v need one tensor", call, [good], [0.5], *shape, d, *tail(th[:2], v))
    rejected(TypeError, "theta / v must be sequences", call, [good], [0.5], *shape, d, *tail(th, 5))
    for b in bad_records():
        rejected(TypeError, "records must be 16-B aligned uint8", call, [good, b], [0.5, 0.5], *shape, d, None, None,
                 *STEP)
    rejected(TypeError, "", call, [good], ["x"], *shape, d, None, None, *STEP)  # (a weight that is no number)
    bad_shape = (N, FMT, S, 3) if dense else (N + 1, K, S)
    text = "bad wire shape" if dense else "do not hold the records' element count"
    rejected(ValueError if dense else TypeError, text, call, [good], [0.5], *bad_shape, d, None, None, *STEP)
    # two errors: the server tensors before theta before the records
    rejected(TypeError, "theta / v must match", call, [5], [0.5], *shape, d, *tail(th, [t.double() for t in v]))
    rejected(TypeError, "server tensors must be", call, [5], [0.5], *shape, [t.double() for t in d], *tail(5, 5))
    unchanged(snap)
    assert accepted(call, [good, good], [0.5, 0.25], *shape, d, None, None, *STEP) is None
    assert accepted(call, [good], [0.5], *shape, d, *tail(th, v)) is None


def test_fold_record_groups(stacked_rec):
    a, b2 = model(), model(2.0)
    good = stacked_rec
    snap = snapshot(a, b2, good)
    call = fold.fold_record_groups
    for kind, b in bad_tensors(a):
        text = "do not hold the records' element count" if kind == "size" else "server tensors must be"
        rejected(TypeError, text, call, [[good]], [[0.5]], [b], N, K, S)
        text = "must match the first group's sizes" if kind == "size" else "server tensors must be"
        rejected(TypeError, text, call, [[good], [good]], [[0.5], [0.5]], [b2, b], N, K, S)
    for b in bad_records():
        rejected(TypeError, "records must be 16-B aligned uint8", call, [[good], [good, b]], [[0.5], [0.5, 0.5]], [a, b2],
                 N, K, S)
    rejected(TypeError, "first group's number of tensors", call, [[good], [good]], [[0.5], [0.5]], [a, b2[:2]], N, K, S)
    rejected(ValueError, "one weight per record", call, [[good], [good]], [[0.5], []], [a, b2], N, K, S)
    rejected(TypeError, "", call, [[good]], [["x"]], [a], N, K, S)  # (a weight that is no number)
    # one destination tensor in two groups is refused; a zero-element tensor may be shared
    rejected(TypeError, "a server tensor in two places", call, [[good], [good]], [[0.5], [0.5]],
             [a, [b2[0], b2[1], a[2]]], N, K, S)
    rejected(TypeError, "a server tensor in two places", call, [[good], []], [[0.5], []], [a, a], N, K, S)
    # two errors: a group's tensors before its records, the groups in order
    rejected(TypeError, "server tensors must be", call, [[5], [good]], [[], [0.5]], [[t.double() for t in a], b2[:2]], N, K,
             S)
    rejected(TypeError, "records must be 16-B aligned uint8", call, [[5], [good]], [[0.5], [0.5]], [a, b2[:2]], N, K, S)
    unchanged(snap)
    assert accepted(call, [[good], [good, good]], [[0.5], [0.5, 0.25]], [a, [b2[0], a[1], b2[2]]], N, K, S) is None
    assert accepted(call, [[good], []], [[0.5], []], [a, b2], N, K, S) is None


def test_avg_and_gradient_records(stacked_rec):
    p, good = model(), stacked_rec
    msg = {"parameters": model(2.0)}
    snap = snapshot(p, msg["parameters"], good)
    call = fold.avg_and_gradient_records
    for kind, b in bad_tensors(p):
        text = "do not hold the records' element count" if kind == "size" else "model tensors must be"
        rejected(TypeError, text, call, b, [msg], [good], [0.5], [0.5], N, K, S, 0.0, True)
        rejected(TypeError, text, call, b, None, [good], None, [0.5], N, K, S, 0.0, True)
    for b in bad_records():
        rejected(TypeError, "records must be 16-B aligned uint8", call, p, [msg, msg], [good, b], [0.5, 0.5], [0.5, 0.5],
                 N, K, S, 0.0, True)
        rejected(TypeError, "records must be 16-B aligned uint8", call, p, None, [b], None, [0.5], N, K, S, 0.0, True)
    for kind, b in bad_tensors(msg["parameters"]):
        rejected(TypeError, "message tensors must be", call, p, [msg, {"parameters": b}], [good, good], [0.5, 0.5],
                 [0.5, 0.5], N, K, S, 0.0, True)
    rejected(TypeError, "one tensor per model tensor", call, p, [{"parameters": model()[:2]}], [good], [0.5], [0.5], N, K,
             S, 0.0, True)
    rejected(KeyError, "parameters", call, p, [{}], [good], [0.5], [0.5], N, K, S, 0.0, True)
    rejected(ValueError, "bad wire shape", call, [p[1]], None, [good], None, [0.5], 0, 0, S, 0.0, True)
    rejected(TypeError, "", call, p, None, [good], None, ["x"], N, K, S, 0.0, True)  # (a weight that is no number)
    # two errors: a message's record before its parameters, the model before both
    rejected(TypeError, "records must be 16-B aligned uint8", call, p, [{}], [5], [0.5], [0.5], N, K, S, 0.0, True)
    rejected(TypeError, "model tensors must be", call, [t.double() for t in p], [{}], [5], [0.5], [0.5], N, K, S, 0.0)
    unchanged(snap)
    assert all(t.grad is None for t in p)
    _check_views(accepted(call, p, [msg, msg], [good, good], [0.5, 0.5], [0.5, 0.5], N, K, S, 0.0), p, False)
    _check_views(accepted(call, p, None, [good], None, [0.5], N, K, S, 0.0, False), p, False)
    _check_views(accepted(call, p, [msg], [good], [0.5], [0.5], N, K, S, 0.0, True), p, True)
    q = model()
    _check_views(accepted(call, q, None, [good], None, [1.0], N, K, S, 0.0, True), q, True)
    unchanged((q, model()))  # (without messages the parameters are left untouched)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible devices")
def test_other_device_leaves_the_current_one():
    """A call on tensors of device 1 while device 0 is current runs there and leaves the current device at 0."""
    torch.cuda.set_device(0)
    d1 = dev(1)
    loc, glo, e = model(3.0, d1), model(1.0, d1), torch.zeros(N, device=d1)
    out = accepted(fold.delta_flat, loc, glo)
    assert torch.cuda.current_device() == 0 and out.device == d1
    assert accepted(fold.ef_accumulate, loc, glo, e) is None
    assert accepted(fold.model_fold, loc, [glo], None, [0.5], *FOLD) is None
    assert torch.cuda.current_device() == 0
    torch.cuda.synchronize(d1)
    assert torch.equal(out, torch.full((N,), 2.0, device=d1)) and torch.equal(e, out)
    # tensors of two devices in one call: refused
    rejected(TypeError, "local / global tensors", fold.delta_flat, loc, model(1.0))
    assert torch.cuda.current_device() == 0
