"""The low-rank (PowerSGD) compressor on the device against plain float64 numpy: the MFMA fold and the decode on
hand-built records (an exact class, bit for bit, and a general class within the rounding bound of their sums), the
one-pass encode, and one FedOpt round through the mixins."""

import numpy as np
import pytest
import torch

from fl_sim_amd import codec

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = [(cols, r, n) for cols in (256, 512, 1024) for r in (1, 2, 4)
          for n in (1, cols - 1, cols + 1, 33 * cols + 5, 1100 * cols - 3)]
# the largest errors measured on the device at SHAPES, times 4: the decoded vector in units of
# 2^-24 max|M| sqrt(cols) (6.04, the 2 x 512 Gaussian matrix at rank 4), P^T P - I in units of 2^-24 (1.53)
DECODED_UNITS, ORTHO_UNITS = 4 * 6.04, 4 * 1.53


def _record(P, Q, n, cols, r):
    total, off = codec.lowrank_wire_layout(n, cols, r)
    buf = np.zeros(total, np.uint8)
    for name, a in (("p", P), ("q", Q)):
        b = np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint8)
        buf[off[name]:off[name] + b.size] = b
    return torch.from_numpy(buf).cuda()


def _factors(g, cls, count, m, cols, r):
    if cls == "exact":  # small integers and power-of-two weights: every partial sum is exact in fp32 in any order
        return ([g.integers(-8, 9, (m, r)).astype(np.float32) for _ in range(count)],
                [g.integers(-8, 9, (cols, r)).astype(np.float32) for _ in range(count)],
                (2.0 ** g.integers(-2, 3, count) * g.choice([-1.0, 1.0], count)).astype(np.float32))
    return ([g.standard_normal((m, r)).astype(np.float32) for _ in range(count)],
            [g.standard_normal((cols, r)).astype(np.float32) for _ in range(count)],
            g.standard_normal(count).astype(np.float32))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _exact(got, want64):
    """Bit equality with the float64 reference, a zero's sign aside (a sum of -0 products is -0 or +0 by its order)."""
    return _same_bits(got + np.float32(0), want64 + 0.0)


@pytest.mark.parametrize("cls", ["exact", "general"])
@pytest.mark.parametrize("cols,r,n,C", [s + (C,) for s in SHAPES for C in (1, 3, 10)]
                         + [(256, 1, 33 * 256 + 5, 71), (512, 4, 512 + 1, 67)])  # (past 64 records: chained launches)
def test_fold(cols, r, n, C, cls):
    g = np.random.default_rng(n + 7 * C + r)
    m = -(-n // cols)
    Ps, Qs, w = _factors(g, cls, C, m, cols, r)
    recs = [_record(P, Q, n, cols, r) for P, Q in zip(Ps, Qs)]
    A = np.concatenate([np.float32(wc) * P for wc, P in zip(w, Ps)], 1).astype(np.float64)  # fp32(w_c P^), [m, K]
    B = np.concatenate(Qs, 1).astype(np.float64)
    ref, mag = (A @ B.T).reshape(-1)[:n], (np.abs(A) @ np.abs(B).T).reshape(-1)[:n]
    out0 = g.integers(-64, 65, n).astype(np.float32) if cls == "exact" else g.standard_normal(n).astype(np.float32)
    for acc in (False, True):
        want = ref + out0 if acc else ref
        got = [codec.fold_lowrank_records(recs, w.tolist(), n, cols, r, out=torch.from_numpy(out0).cuda(),
                                          accumulate=acc).cpu().numpy() for _ in range(2)]
        assert _same_bits(got[0], got[1])  # (a rerun: identical bytes)
        if cls == "exact":
            assert _exact(got[0], want)
        else:
            err, bound = np.abs(got[0] - want), (C * r + 3) * U * mag + (U * np.abs(out0) if acc else 0)
            print(f"fold {cols}x{r} n={n} C={C} acc={acc}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert np.all(err <= bound)


@pytest.mark.parametrize("cls", ["exact", "general"])
@pytest.mark.parametrize("cols,r,n", SHAPES)
def test_decode_of_a_handbuilt_record(cols, r, n, cls):
    g = np.random.default_rng(n + r)
    (P,), (Q,), (w,) = _factors(g, cls, 1, -(-n // cols), cols, r)
    rec = _record(P, Q, n, cols, r)
    v = (P.astype(np.float64) @ Q.astype(np.float64).T).reshape(-1)[:n]
    mag = (np.abs(P).astype(np.float64) @ np.abs(Q).astype(np.float64).T).reshape(-1)[:n]
    x = g.integers(-64, 65, n).astype(np.float32) if cls == "exact" else g.standard_normal(n).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    res = torch.empty_like(xd)
    plain = codec.lowrank_decode(rec, n, cols, r, weight=float(w), x=xd, residual=res).cpu().numpy()
    accum = codec.lowrank_decode(rec, n, cols, r, out=xd.clone(), weight=float(w), accumulate=True).cpu().numpy()
    inplace = xd.clone()
    codec.lowrank_decode(rec, n, cols, r, x=inplace, residual=inplace)
    assert _same_bits(inplace.cpu().numpy(), res.cpu().numpy())
    wants = (float(w) * v, float(w) * v + x, x - v)
    for got, want, extra in zip((plain, accum, res.cpu().numpy()), wants, (0, U * np.abs(x), U * np.abs(x - v))):
        if cls == "exact":
            assert _exact(got, want)
        else:  # r products and sums, the weight's rounding, the accumulate's (or the subtraction's)
            assert np.all(np.abs(got - want) <= (r + 3) * U * max(abs(float(w)), 1.0) * mag + extra)


def _reference(x, cols, Q):
    """The six steps in float64: (P^, Q', dropped, decoded)."""
    n, r = x.size, Q.shape[1]
    m = -(-n // cols)
    M = np.zeros(m * cols)
    M[:n] = x
    M = M.reshape(m, cols)
    P = M @ Q
    G = P.T @ P
    L, W, drop = np.zeros((r, r)), np.zeros((r, r)), np.zeros(r, bool)
    for k in range(r):
        d = G[k, k] - L[k, :k] @ L[k, :k]
        drop[k] = G[k, k] == 0 or d <= 2.0 ** -40 * G[k, k]
        if not drop[k]:
            L[k, k] = np.sqrt(d)
            L[k + 1:, k] = (G[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    for k in range(r):
        if not drop[k]:
            W[k, k] = 1 / L[k, k]
            for l in range(k):
                W[k, l] = -(L[k, l:k] @ W[l:k, l]) / L[k, k]
    Ph, Qn = P @ W.T, (M.T @ P) @ W.T
    return Ph, Qn, drop, (Ph @ Qn.T).reshape(-1)[:n]


def _encode(x, Q, **kw):
    qd = torch.from_numpy(Q.astype(np.float32)).cuda()
    qn = torch.empty_like(qd)
    rec, out = codec.lowrank_encode(torch.from_numpy(x).cuda(), qd, q_next=qn, decode=True, **kw)
    P, Qp = codec.lowrank_wire_views(rec, x.size, *Q.shape)
    return rec, out.cpu().numpy(), P.cpu().numpy().astype(np.float64), Qp.cpu().numpy(), qn.cpu().numpy()


@pytest.mark.parametrize("kind", ["lowrank", "gaussian"])
@pytest.mark.parametrize("cols,r,n", SHAPES)
def test_encode(cols, r, n, kind):
    g = np.random.default_rng(3 * n + r)
    m = -(-n // cols)
    if kind == "lowrank":  # (a) A B^T with small integers: rank <= r, so the decoded vector is the input
        A = g.integers(-4, 5, (m, r)).astype(np.float64)
        if m > 1 and n % cols:
            A[-1] = 0  # (the zero padding must not raise the rank: a short last row is a zero row)
        x = (A @ g.integers(-4, 5, (cols, r)).T).reshape(-1)[:n].astype(np.float32)
    else:
        x = g.standard_normal(n).astype(np.float32)
    Q = g.standard_normal((cols, r)).astype(np.float32)
    rec, out, P, Qp, qn = _encode(x, Q)
    _, _, drop, dec = _reference(x.astype(np.float64), cols, Q.astype(np.float64))
    unit = U * max(np.max(np.abs(x)), 1e-30) * np.sqrt(cols)
    e_dec, e_orth = np.max(np.abs(out - dec)) / unit, np.max(np.abs(P.T @ P - np.diag(~drop * 1.0))) / U
    print(f"encode {kind} {cols}x{r} n={n}: decoded {e_dec:.2f} units, orthonormality {e_orth:.2f} units")
    assert np.array_equal(~P.any(0), drop) and np.array_equal(~Qp.any(0), drop)
    assert e_dec <= DECODED_UNITS and e_orth <= ORTHO_UNITS
    if kind == "lowrank":
        assert np.max(np.abs(out - x)) <= DECODED_UNITS * unit
    assert _same_bits(qn[:, drop], Q[:, drop]) and _same_bits(qn[:, ~drop], Qp[:, ~drop])
    # (c) the residual is fp32(x - out), in place too, and a rerun gives the same bytes
    xd = torch.from_numpy(x).cuda()
    res = torch.empty_like(xd)
    _, out2, P2, Qp2, _ = _encode(x, Q, residual=res)
    codec.lowrank_encode(xd, torch.from_numpy(Q).cuda(), residual=xd)
    assert _same_bits(P, P2) and _same_bits(Qp, Qp2) and _same_bits(out, out2)
    assert _same_bits(res.cpu().numpy(), x - out)
    assert _same_bits(xd.cpu().numpy(), x - out)


@pytest.mark.parametrize("cols,n", [(256, 33 * 256 + 5), (1024, 1100 * 1024 - 3)])
def test_encode_drops_columns_without_nan(cols, n):
    g = np.random.default_rng(n)
    Q = g.integers(1, 4, (cols, 2)).astype(np.float32)
    m = -(-n // cols)
    u = g.integers(1, 4, m).astype(np.float64)
    u[-1] = 0
    rank1 = np.outer(u, g.integers(1, 4, cols)).reshape(-1)[:n].astype(np.float32)  # (P is exact: parallel columns)
    for x, dropped in ((np.zeros(n, np.float32), [True, True]), (rank1, [False, True])):
        rec, out, P, Qp, qn = _encode(x, Q)
        assert np.isfinite(out).all() and np.isfinite(P).all() and np.isfinite(Qp).all()
        assert np.array_equal(~P.any(0), dropped) and np.array_equal(~Qp.any(0), dropped)
        assert _same_bits(qn[:, dropped], Q[:, dropped]) and _same_bits(qn[:, ~np.array(dropped)], Qp[:, ~np.array(dropped)])
        assert np.max(np.abs(out - x)) <= DECODED_UNITS * U * np.max(np.abs(x)) * np.sqrt(cols)


def test_fedopt_rounds_with_records_and_feedback():
    """Three clients with ``wire_records`` and ``error_feedback`` for two rounds: the messages carry low-rank records,
    each memory is ``a - decode(record)`` bit for bit, the server's model is the float64 fold of the records within
    the fold's bound and the dense fold's own roundings, and avg_parameters (the decode fallback) agrees too."""
    from fl_sim_amd import LowRankCompressor, aggregation
    from tests.test_gpu_round import build_round

    shapes = [(64, 3, 3), (4096,), (300, 77)]
    n = sum(int(np.prod(sh)) for sh in shapes)
    s, clients = build_round(shapes, "avg", "cuda", n_clients=3)
    flat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()  # noqa: E731
    mem = [np.zeros(n, np.float32) for _ in clients]
    for c in clients:
        c.compressors, c.error_feedback, c.wire_records = [LowRankCompressor(n, rank=2, seed=c.client_id)], True, True
    cols = clients[0].compressors[0].cols
    for rnd in range(2):
        theta, delta = flat(s.model.parameters()).astype(np.float64), flat(s.delta_parameters).astype(np.float64)
        s._received_messages = []
        a = [(e + (flat(c.model.parameters()) - flat(c._cached_parameters))).astype(np.float32)
             for c, e in zip(clients, mem)]
        for c in clients:
            c.communicate(s)
        msgs = [m["delta_parameters"] for m in s._received_messages]
        assert all(d.kind == "lowrank" and d.nbytes == codec.lowrank_wire_layout(n, cols, 2)[0] for d in msgs)
        assert all(c.compressors[0].last_need_to_send_advance == (-(-n // cols) + cols) * 2 for c in clients)
        dec = [codec.lowrank_decode(d.record, n, cols, 2).cpu().numpy() for d in msgs]
        mem = [c.error_memory("delta_parameters").value().cpu().numpy() for c in clients]
        assert all(_same_bits(e, ai - di) for e, ai, di in zip(mem, a, dec))
        s.update()
        assert all(d._flat is None for d in msgs)  # (folded from the records, never decoded)
        avg = [torch.zeros(sh, device="cuda") for sh in shapes]
        aggregation.avg_parameters(avg, s._received_messages, key="delta_parameters")
        assert np.all(np.abs(flat(avg) - sum(d.astype(np.float64) for d in dec) / 3)
                      <= 4 * U * sum(np.abs(d) for d in dec) / 3)
        views = [[v.cpu().numpy().astype(np.float64) for v in codec.lowrank_wire_views(d.record, n, cols, 2)]
                 for d in msgs]
        alpha = np.float32(1 / 3)
        F = sum((np.float32(alpha) * P.astype(np.float32)).astype(np.float64) @ Q.T for P, Q in views).reshape(-1)[:n]
        mag = sum(np.abs(alpha * P) @ np.abs(Q).T for P, Q in views).reshape(-1)[:n]
        want = theta + (0 * delta + F)  # (avg: lr 1, betas (0, 1))
        bound = (3 * 2 + 3) * U * mag + U * np.abs(F) + U * np.abs(want)  # the fold, delta's and theta's roundings
        assert np.all(np.abs(flat(s.model.parameters()) - want) <= bound)
        for c in clients:  # the next round: the clients start from the server's model and move again
            c._cached_parameters = [p.detach().clone() for p in s.model.parameters()]
            for p, q in zip(c.model.parameters(), s.model.parameters()):
                p.data = q.detach() + 0.01 * torch.sin(p.detach() * (3 + c.client_id))
