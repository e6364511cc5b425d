"""flc_robust_fold on the device (the coordinate-wise median and trimmed mean, include/flcodec.h) against plain numpy:
the values mapped to their totalOrder keys, np.sort along the client axis, mapped back; the kept slice summed and
divided in float64.  Then the fused optimiser step against codec.fedopt_step, and a round through the mixin."""

import functools

import numpy as np
import pytest
import torch

from fl_sim_amd import codec
from oracle.server_steps_exact import fma_exact
from tests import golden_cases as gc

pytestmark = pytest.mark.gpu

F32, F64, U = np.float32, np.float64, 2.0 ** -24
SIZES = (1, 3, 1024, 1027, 4099)  # (tensor 3 is a view at a 4-byte offset, on the model and in every message)
CS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64]
PLANT = np.array([[-1e30, -np.inf, np.uint32(0xffc00001).view(F32)],  # below: .., -inf, a -NaN
                  [1e30, np.inf, np.uint32(0x7fffffff).view(F32)]], dtype=F32)  # above: .., +inf, the largest +NaN
RULES = [("median", 0, C) for C in CS] + [("trimmed_mean", b, C) for C in CS
                                          for b in sorted({0, 1, (C - 1) // 2}) if 2 * b < C]


def _sorted(X):  # along the client axis by the IEEE totalOrder key, a signed integer; the map is its own inverse
    k = np.ascontiguousarray(X).view(np.int32)
    k = np.sort(k ^ ((k >> 31) & 0x7fffffff), axis=0)
    return (k ^ ((k >> 31) & 0x7fffffff)).view(F32)


@functools.lru_cache(maxsize=None)
def _case(cls, rule, b, C, sizes=SIZES):
    """(X (C, n) over the concatenated tensors, r in float64, the bound on |got - r|, None where fp32(r) is exact)."""
    n, med = sum(sizes), rule == "median"
    g = np.random.default_rng(97 * C + 7 * b + med + 1000 * (cls == "exact") + len(sizes))
    X = g.standard_normal((C, n)).astype(F32)
    if cls == "exact":  # small integers and both zeros; outliers in at most q clients per side and coordinate
        X = g.integers(-8, 9, (C, n)).astype(F32)
        X[(X == 0) & (g.random((C, n)) < 0.5)] = -0.0
        q = (-(-C // 2) - 1) // 2 if med else b
        order = np.argsort(g.random((C, n)), axis=0)[:2 * q]  # (distinct clients per coordinate)
        for j, rows in enumerate(order):
            vals = np.where(g.random(n) < 0.6, PLANT[j // q][g.integers(0, 3, n)], X[rows, np.arange(n)])
            np.put_along_axis(X, rows[None], vals[None], 0)
    lo, hi = ((C - 1) // 2, C // 2 + 1) if med else (b, C - b)
    kept, m = _sorted(X)[lo:hi].astype(F64), hi - lo
    with np.errstate(all="ignore"):
        ref = functools.reduce(np.add, kept) / m if not med else 0.5 * kept[0] + 0.5 * kept[-1]
        bound = U * np.abs(ref) + (2.0 ** -149 if med else (m - 1) * U * np.abs(kept).sum(0) / m)
    X.setflags(write=False)
    return X, ref, None if (cls == "exact" or m == 1) else bound  # (one kept value: a selection, s / 1.0f)


def _upload(X, sizes=SIZES, fill=0.0):
    """One buffer, one copy: (model tensors filled with ``fill``, the messages' tensor lists); every tensor starts
    16-B aligned but tensor 3, which starts 4 bytes later."""
    offs = np.cumsum([0] + [(n + 8) // 4 * 4 for n in sizes])
    host = np.full((len(X) + 1, offs[-1]), fill, dtype=F32)
    views = [slice(o + (t == 3), o + (t == 3) + n) for t, (o, n) in enumerate(zip(offs, sizes))]
    for v, e, n in zip(views, np.cumsum((0,) + tuple(sizes)), sizes):
        host[1:, v] = X[:, e:e + n]
    dev = torch.from_numpy(host).cuda()
    rows = [[row[v] for v in views] for row in dev]
    return rows[0], rows[1:]


def _flat(ts):
    return torch.cat([t.detach().reshape(-1) for t in ts]).cpu().numpy()


@pytest.mark.parametrize("rule,b,C", RULES)
@pytest.mark.parametrize("cls", ["exact", "general"])
def test_fold_only(cls, rule, b, C):
    X, ref, bound = _case(cls, rule, b, C)
    dst, msgs = _upload(X, fill=7.0)
    codec.robust_fold(dst, msgs, rule, b, 1.0, 1)  # a = fmaf(1, r, +0)
    got = _flat(dst)
    if bound is None:
        assert gc.same_bits(got, ref.astype(F32) + F32(0.0))
    else:
        err = np.abs(got.astype(F64) - ref)
        print(f"{cls} {rule} b={b} C={C}: worst error / bound {np.max(err / bound):.3f}")
        assert np.all(err <= bound)
    codec.robust_fold(dst, msgs, rule, b, 1.0, 1)
    assert gc.same_bits(_flat(dst), got)  # a rerun: the same bytes
    if cls == "exact":  # from -0 the sum keeps r itself, a zero's sign included
        dst, msgs = _upload(X, fill=-0.0)
        codec.robust_fold(dst, msgs, rule, b, 1.0, 2)
        assert gc.same_bits(_flat(dst), ref.astype(F32))


@pytest.mark.parametrize("C", [10, 64])
def test_more_tensors_than_one_launch_holds(C):
    X, ref, _ = _case("exact", "trimmed_mean", 1, C, (5,) * 300)
    dst, msgs = _upload(X, (5,) * 300)
    codec.robust_fold(dst, msgs, "trimmed_mean", 1, 1.0, 1)
    assert gc.same_bits(_flat(dst), ref.astype(F32) + F32(0.0))


@pytest.mark.parametrize("opt", ["avg", "adagrad", "yogi", "adam"])
@pytest.mark.parametrize("rule,b", [("median", 0), ("trimmed_mean", 1)])
@pytest.mark.parametrize("C", [5, 16, 33])
def test_fused_step_equals_fold_then_fedopt_step(C, rule, b, opt):
    n, lr, beta2, tau = sum(SIZES), 0.03, 0.99, 1e-3
    rd, msgs = _upload(_case("general", rule, b, C)[0])
    codec.robust_fold(rd, msgs, rule, b, 1.0, 1)
    g = np.random.default_rng(C)
    state = np.stack([g.standard_normal(n), g.standard_normal(n), g.random(n) + 1e-3]).astype(F32)  # dst, theta, v
    a = fma_exact(F32(0.1), _flat(rd), state[0] * F32(0.9))
    want = [torch.from_numpy(x).cuda() for x in (a, state[1].copy(), state[2].copy())]
    codec.fedopt_step(want[1], want[0], None if opt == "avg" else want[2], opt, lr, beta2, tau)
    dst, theta, v = _upload(state)[1]
    codec.robust_fold(dst, msgs, rule, b, 0.1, 0, 0.9, theta=theta, v=None if opt == "avg" else v, opt=opt, lr=lr,
                      beta2=beta2, tau=tau)
    assert all(gc.same_bits(_flat(x), y.cpu().numpy()) for x, y in zip((dst, theta, v), want))


def _round(opt, where, **switches):
    """A FedOpt server of the small model and its ten messages: eight honest deltas, one all 1e30, one all NaN."""
    from tests.golden.gen_golden import SMALL_SHAPES
    from tests.test_gpu_round import build_round

    s, clients = build_round(SMALL_SHAPES, opt, where, n_clients=8)
    vars(s.config).update(switches)
    theta = [p.detach().cpu() for p in s.model.parameters()]
    deltas = [[(p.detach().cpu() - t).cuda() for p, t in zip(c.model.parameters(), theta)] for c in clients]
    deltas += [[torch.full(sh, val, device="cuda") for sh in SMALL_SHAPES] for val in (1e30, float("nan"))]
    s._received_messages = [{"delta_parameters": d, "train_samples": 1} for d in deltas]
    return s, clients


@pytest.mark.parametrize("where", ["cuda", "cpu"])
@pytest.mark.parametrize("opt", ["avg", "adam"])
@pytest.mark.parametrize("rule,trim,lo,hi", [("trimmed_mean", np.float32(0.2), 2, 8), ("median", 0, 4, 6)])
def test_round_through_the_mixin(rule, trim, lo, hi, opt, where):
    """theta against the whole update in float64.  With m kept values the delta d = fmaf(1 - b0, r, delta * b0) is off
    by at most (m + 2) u (|1 - b0| mean|kept| + |b0 delta|): the sum and the division, the scalars' casts, the product
    and the fma.  FedAvg adds lr times that and one rounding of theta.  Adam's lr d / (sqrt(v') + tau) moves by at most
    twice that over the denominator (through d, and d^2 under the root), plus 10 u of itself: its roundings and casts."""
    s, _ = _round(opt, where, robust=rule, robust_trim=trim)
    cfg, (b0, b2), m = s.config, s.config.betas, hi - lo
    th0, d0 = (_flat(ts).astype(F64) for ts in (s.model.parameters(), s.delta_parameters))
    kept = _sorted(np.stack([_flat(m_["delta_parameters"]) for m_ in s._received_messages])).astype(F64)[lo:hi]
    d = (1 - b0) * kept.mean(0) + b0 * d0
    upd = bound = cfg.lr * (m + 2) * U * ((1 - b0) * np.abs(kept).mean(0) + b0 * np.abs(d0))
    if opt == "avg":
        upd = cfg.lr * d
    else:
        den = np.sqrt(b2 * _flat(s.v_parameters).astype(F64) + (1 - b2) * d * d) + cfg.tau
        upd, bound = cfg.lr * d / den, 2 * bound / den + 10 * U * np.abs(cfg.lr * d / den)
    s.update()
    got = _flat(s.model.parameters())
    assert np.isfinite(got).all() and all(p.device.type == where for p in s.model.parameters())
    err, bound = np.abs(got - (th0 + upd)), bound + np.spacing(np.abs(got))
    print(f"{rule} {opt} {where}: worst error / bound {np.max(err / bound):.3f}")
    assert np.all(err <= bound)


def test_round_without_the_switch_is_not_finite_and_too_many_messages_raise():
    s, _ = _round("avg", "cuda")
    s.update()  # (the existing path, as it is: the mean takes the two faulty clients in)
    assert not any(torch.isfinite(p).all() for p in s.model.parameters())
    s, _ = _round("avg", "cuda", robust="median")
    s._received_messages = (s._received_messages * 7)[:65]
    with pytest.raises(ValueError, match="64"):
        s.update()


def test_round_of_sign_records_equals_the_fold_of_the_decoded_messages():
    from fl_sim_amd import SignCompressor

    s, clients = _round("adam", "cuda", robust="trimmed_mean", robust_trim=2)
    bad, s._received_messages = s._received_messages[8:], []
    for c in clients:
        c.compressors, c.wire_records = [SignCompressor(_flat(s.model.parameters()).size, bucket=64)], True
        c.communicate(s)
    assert all(m["delta_parameters"].kind == "sign" for m in s._received_messages)
    s._received_messages += bad
    cfg, state = s.config, (s.delta_parameters, list(s.model.parameters()), s.v_parameters)
    want = [[t.detach().clone() for t in ts] for ts in state]
    codec.robust_fold(want[0], [list(m["delta_parameters"]) for m in s._received_messages], "trimmed_mean", 2,
                      1 - cfg.betas[0], 0, cfg.betas[0], theta=want[1], v=want[2], opt="adam", lr=cfg.lr,
                      beta2=cfg.betas[1], tau=cfg.tau)
    s.update()
    assert all(gc.same_bits(_flat(got), _flat(exp)) for got, exp in zip(state, want))
