"""The count sketch (FetchSGD) on the device against the float64 numpy restatement in tests/sketch_ref.py: the one-pass
encode (an exact class bit for bit, a general class within the rounding bound of its sums), the estimate on hand-built
records, the server's state step and clear, recovery of planted coordinates, and FedAvg rounds through the mixins."""

import numpy as np
import pytest
import torch

from fl_sim_amd import SketchCompressor, codec
from tests import sketch_ref as ref
from tests.test_capi_sketch import RECOVERY_SEEDS

pytestmark = pytest.mark.gpu

U, T, SEED = ref.U, ref.T, 0x1234_5678_9ABC
# n: the tile and chunk edges, then the split rule's (8 chunks per split): the largest n with one split, the smallest
# with two (its last split a single element), and two splits of 8 and 5 chunks
SHAPES = [(r, c, n) for r in (1, 3, 5) for c in (4096, 8192)
          for n in (1, T - 1, T + 1, c - 1, c + 1, 3 * c + T + 5, 8 * c, 8 * c + 1, 13 * c + 3)]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _exact(got, want64):
    """Bit equality with the float64 reference, a zero's sign aside."""
    return _same_bits(np.asarray(got, np.float32) + np.float32(0), np.asarray(want64, np.float64) + 0.0)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


@pytest.mark.parametrize("cls", ["exact", "general"])
@pytest.mark.parametrize("rows,cols,n", SHAPES)
def test_encode(rows, cols, n, cls):
    g = np.random.default_rng(n + rows)
    x = (g.integers(-8, 9, n) if cls == "exact" else g.standard_normal(n)).astype(np.float32)
    assert codec._lib.load().flc_sketch_splits(n, cols) == (1 if n <= 8 * cols else 2)
    S, M = ref.encode(x, rows, cols, SEED)
    rec, est = codec.sketch_encode(_dev(x), rows, cols, SEED, estimate=True)
    got = codec.sketch_table(rec, rows, cols).cpu().numpy()
    again = codec.sketch_table(codec.sketch_encode(_dev(x), rows, cols, SEED)[0], rows, cols).cpu().numpy()
    assert _same_bits(got, again)  # (a rerun: identical bytes)
    if cls == "exact":  # every partial sum is exact in any order: this pins the tile map, the permutations, the signs
        assert _exact(got, S)
    else:
        err, bound = np.abs(got - S), (-(-n // cols) + 2) * U * M
        print(f"encode {rows}x{cols} n={n}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
        assert np.all(err <= bound)
    assert _exact(est.cpu().numpy(), ref.estimate(got, n, cols, SEED)[0])  # (out: the estimate of its own record)


@pytest.mark.parametrize("cls", ["exact", "general"])
@pytest.mark.parametrize("rows,cols,n,C", [(r, c, n, C) for r in (1, 3, 5) for c, n in ((4096, 3 * 4096 + T + 5),
                                                                                       (8192, 8192 - 1))
                                           for C in (1, 3, 10)] + [(5, 4096, 4096 + 1, 70), (3, 8192, 20000, 67)])
def test_estimate_of_handbuilt_records(rows, cols, n, C, cls):
    g = np.random.default_rng(n + 7 * C + rows)
    if cls == "exact":  # integer tables and power-of-two weights: every partial sum is exact
        tabs = [g.integers(-8, 9, (rows, cols)).astype(np.float32) for _ in range(C)]
        w = (2.0 ** g.integers(-2, 3, C) * g.choice([-1.0, 1.0], C)).astype(np.float32)
    else:
        tabs = [g.standard_normal((rows, cols)).astype(np.float32) for _ in range(C)]
        w = g.standard_normal(C).astype(np.float32)
    recs = [_dev(t) for t in tabs]
    got = codec.sketch_estimate(recs, w.tolist(), n, rows, cols, SEED).cpu().numpy()
    sbar64 = sum(np.float64(wc) * t.astype(np.float64) for wc, t in zip(w, tabs))
    want, _ = ref.estimate(sbar64, n, cols, SEED)
    if cls == "exact":
        assert _exact(got, want)
        return
    _, mags = ref.estimate(ref.fold(tabs, w)[1], n, cols, SEED)  # (|.| of the per-row magnitudes: the signs drop out)
    bound = (C + 1) * U * np.max(np.abs(mags), axis=1)  # a median moves no further than its worst argument
    print(f"estimate {rows}x{cols} n={n} C={C}: max err / bound = {np.max(np.abs(got - want) / bound):.3f}")
    assert np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("rho", [0.0, 0.5])
@pytest.mark.parametrize("rows", [1, 3, 5])
def test_state_step_and_clear(rows, rho):
    cols, n, C = 4096, 3 * 4096 + T + 5, 3  # (NT = 4; the kept indices span the first chunk boundary)
    g = np.random.default_rng(rows)
    tabs = [g.integers(-8, 9, (rows, cols)).astype(np.float32) for _ in range(C)]
    w = [0.5, 2.0, -1.0]
    u0, v0 = (g.integers(-16, 17, (rows, cols)).astype(np.float32) for _ in range(2))
    u, v = _dev(u0), _dev(v0)
    codec.sketch_state_step([_dev(t) for t in tabs], w, rows, cols, rho, u, v)
    u1 = rho * u0.astype(np.float64) + sum(wc * t.astype(np.float64) for wc, t in zip(w, tabs))
    v1 = v0 + u1
    assert _exact(u.cpu().numpy(), u1) and _exact(v.cpu().numpy(), v1)
    idx = np.array([5, cols - 2, cols - 1, cols, cols + 1, 2 * cols + 1500, n - 1], np.int32)
    cell, sign = ref.cells(idx, cols, SEED, rows)
    got_cell, got_neg = codec.sketch_cells(torch.from_numpy(idx).cuda(), n, rows, cols, SEED)
    assert np.array_equal(got_cell.cpu().numpy(), cell) and np.array_equal(got_neg.cpu().numpy(), sign < 0)
    codec.sketch_clear(torch.from_numpy(idx).cuda(), n, rows, cols, SEED, u, v)
    for j in range(rows):
        u1[j, cell[:, j]] = 0.0
        v1[j, cell[:, j]] = 0.0
    assert _exact(u.cpu().numpy(), u1) and _exact(v.cpu().numpy(), v1)


@pytest.mark.parametrize("seed", RECOVERY_SEEDS)
def test_recovers_planted_coordinates(seed):
    x, idx = ref.planted(seed)
    comp = SketchCompressor(x.size, rows=5, cols=8192, K=8, seed=seed)
    out = comp.compressVector(_dev(x)).cpu().numpy()
    assert np.array_equal(np.flatnonzero(out), idx) and comp.last_need_to_send_advance == 5 * 8192
    est = codec.sketch_encode(_dev(x), 5, 8192, seed, estimate=True)[1].cpu().numpy()
    assert np.array_equal(np.sort(np.argsort(-np.abs(est))[:8]), idx) and _same_bits(out[idx], est[idx])


@pytest.mark.parametrize("error", [False, True])
def test_fedavg_rounds_through_the_mixins(error):
    """Three clients with ``wire_records`` for two rounds: integer deltas with distinct planted coordinates, the
    server keeping ``sketch_k`` = their count; theta is the float64 restatement's, bit for bit."""
    from tests.test_gpu_round import build_round

    shapes = [(64, 3, 3), (4096,), (300, 77)]
    n = sum(int(np.prod(sh)) for sh in shapes)
    s, clients = build_round(shapes, "avg", "cuda", n_clients=3)
    s.sketch_k, s.sketch_error = 6, error
    for p in s.model.parameters():  # (an integer model: the first round's deltas are the integers drawn below)
        p.data = torch.round(p.data * 8)
    for c in clients:
        c._cached_parameters = [p.detach().clone() for p in s.model.parameters()]
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()  # noqa: E731
    for c in clients:
        c.compressors, c.wire_records = [SketchCompressor(n, rows=5, seed=SEED)], True
    rows, cols = 5, clients[0].compressors[0].cols
    g = np.random.default_rng(5)
    v = np.zeros((rows, cols), np.float32)
    for rnd in range(2):
        theta = flat(s.model.parameters()).astype(np.float64)
        s._received_messages, tabs = [], []
        for i, c in enumerate(clients):
            d = g.integers(-1, 2, n).astype(np.float32)
            d[g.choice(n // 3, 2, replace=False) + i * (n // 3)] = 192.0 * (i + 1) * (1 - 2 * (rnd & 1))
            off = 0
            for p, q in zip(c.model.parameters(), c._cached_parameters):
                p.data = q + torch.from_numpy(d[off:off + q.numel()]).cuda().view(q.shape)
                off += q.numel()
            d = flat(c.model.parameters()) - flat(c._cached_parameters)  # (the delta as fp32 forms it)
            tabs.append(ref.encode(d, rows, cols, SEED)[0].astype(np.float32))
            c.communicate(s)
        msgs = [m["delta_parameters"] for m in s._received_messages]
        assert all(d.kind == "sketch" and d.nbytes == 4 * rows * cols for d in msgs)
        assert all(_exact(codec.sketch_table(d.record, rows, cols).cpu().numpy(), t) for d, t in zip(msgs, tabs))
        s.update()
        assert all(d._flat is None for d in msgs)  # (added as tables, never estimated one by one)
        sbar = ref.fold(tabs, [np.float32(1 / 3)] * 3)[0]
        v = (v.astype(np.float64) + sbar).astype(np.float32) if error else sbar  # (rho = 0: u is S-bar)
        est, _ = ref.estimate(v, n, cols, SEED)
        keep = np.argsort(-np.abs(est))[:6]
        if error:
            cell, _ = ref.cells(keep, cols, SEED)
            for j in range(rows):
                v[j, cell[:, j]] = 0.0
            assert _exact(s._sketch_state.v.cpu().numpy(), v)
        else:
            assert s._sketch_state.u is None and s._sketch_state.v is None
        theta[keep] += est[keep]
        assert _exact(flat(s.model.parameters()), theta.astype(np.float32))
        for c in clients:
            c._cached_parameters = [p.detach().clone() for p in s.model.parameters()]
    clients[0].error_feedback = True
    with pytest.raises(ValueError, match="server's sketch"):
        clients[0].communicate(s)
