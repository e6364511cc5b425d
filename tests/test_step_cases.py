"""CPU checks of the server-step edge catalogue (tests/step_cases.py) and its exact reference
(oracle/server_steps_exact.py): ``fma_exact`` against rational arithmetic; the teeth condition (every mutant differs
from the reference on at least 32 lanes of the case vectors, so a kernel that made the mutant's mistake could not
pass tests/test_gpu_step_edges.py); and the stepwise reference against the torch-CPU restatement of the reference
(oracle/aggregation_ref.py) on the catalogue vectors themselves.  Everything without a square root — the fold, v,
FedDR, FedDyn, pFedMe — agrees with torch bit for bit.  FedOpt's theta divides by ``vp.sqrt() + tau`` and torch's CPU
sqrt is not correctly rounded: every lane is in the same class and finite lanes are within the tolerance the suite
documents for torch (1e-6 of the update + 1 ulp; 1e-14 in fp64), with one stated exception, the ``cancel`` block (see
test_stepwise_fedopt_against_torch_on_the_catalogue)."""

import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import server_steps_exact as sx
from tests import step_cases as sc

F32, F64 = np.float32, np.float64
DTYPES = [F32, F64]


# ------------------------------------------------------------------------------------------------------ fma_exact
def _check_fma(w, x, a, dt):
    got = sx.fma_exact(w, x, a, dt)
    assert got.dtype == dt
    for wi, xi, ai, gi in zip(w.tolist(), x.tolist(), a.tolist(), got.tolist()):
        want = sx.round_exact(Fraction(wi) * Fraction(xi) + Fraction(ai), dt)
        assert want == gi and math.copysign(1.0, want) == math.copysign(1.0, gi), (wi, xi, ai, gi, want)


def _triples(dt, count, seed, span=30):
    rng = np.random.RandomState(seed)
    mk = lambda: (rng.uniform(1, 2, count) * 2.0 ** rng.randint(-span, span + 1, count)  # noqa: E731
                  * rng.choice([-1.0, 1.0], count)).astype(dt)
    return mk(), mk(), mk()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_fma_exact_equals_rational_arithmetic_on_random_triples(dt):
    w, x, a = _triples(dt, 10_000, 1)
    _check_fma(w, x, a, dt)
    # products that nearly cancel the addend: a = -fl(w * x) and its neighbours (the result is the product's rounding
    # error, which a rounded product loses)
    w, x, _ = _triples(dt, 2_000, 2)
    p = w * x
    for a in (-p, -np.nextafter(p, dt(np.inf)), -np.nextafter(p, dt(-np.inf))):
        _check_fma(w, x, a, dt)


def test_fma_exact_resolves_the_double_rounding_tie():
    """w * x + a lies just below the midpoint of two fp32 values; its fp64 rounding lands on the midpoint, which then
    rounds up (to even): the naive route through fp64 gives a + 1 ulp, the exact result is a."""
    w = F32((1 + 2.0**-23) * 2.0**-24)
    x = F32(1 - 2.0**-23)
    a = F32(1 + 2.0**-23)
    naive = F32(F64(w) * F64(x) + F64(a))
    assert naive == np.nextafter(a, F32(2))
    assert sx.fma_exact(w, x, a, F32) == a
    assert sx.round_exact(Fraction(float(w)) * Fraction(float(x)) + Fraction(float(a)), F32) == float(a)
    # a family of them: odd-mantissa addends over several binades, the product just under / over half an ulp
    rng = np.random.RandomState(3)
    k = 2_000
    e = rng.randint(-20, 21, k)
    a = ((1 + (2 * rng.randint(0, 2**22, k) + 1) * 2.0**-23) * 2.0**e).astype(F32)
    half = (2.0**-24 * 2.0**e)
    for scale in (1 - 2.0**-23, 1 + 2.0**-23, 1.0):
        w = (half * (1 + 2.0**-23)).astype(F32)
        x = np.full(k, scale, dtype=F32)
        _check_fma(w, x, a, F32)
        _check_fma(-w, x, a, F32)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_fma_exact_in_the_subnormal_range_and_at_the_specials(dt):
    tiny, mn = sc._TINY[dt], sc._MIN[dt]
    rng = np.random.RandomState(4)
    k = 3_000
    w = (rng.uniform(1, 2, k) * rng.choice([-1.0, 1.0], k)).astype(dt)
    x = (mn * 2.0 ** rng.uniform(-30, 2, k)).astype(dt)
    a = (tiny * rng.randint(-40, 41, k)).astype(dt)
    _check_fma(w, x, a, dt)
    _check_fma(w * dt(0.5), np.full(k, tiny, dtype=dt), a, dt)  # products at and under half the smallest subnormal
    big = dt(sc._HUGE[dt])
    arr = lambda *vals: np.array(vals, dtype=dt)  # noqa: E731
    _check_fma(arr(big, big, -big), arr(2, 1.5, 3), arr(-big, big, big), dt)  # the product alone overflows
    z, inf, nan = dt(0), dt(np.inf), dt(np.nan)
    got = sx.fma_exact(arr(z, -z, z, inf, inf, nan, 1, 1), arr(1, 1, -1, z, 1, 1, 1, -1),
                       arr(-z, -z, z, 1, -inf, 1, -1, 1), dt)
    assert sc.lane_class(got).tolist() == [1, 2, 1, 5, 5, 5, 1, 1]


# ------------------------------------------------------------------------------------------------------ the cases
@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_case_vectors_hold_what_they_claim(dt):
    th, d, v = sc.fedopt_case(dt)
    b = sc.blocks(dt)
    assert th.size == d.size == v.size == sc.N == 4133 and sc.N % 4 == 1 and sum(sc.SPLIT) == sc.N
    with np.errstate(all="ignore"):
        d2 = d * d
        t = b["ties"]
        assert (v[t] == d2[t]).sum() >= 48 and (v[t] > d2[t]).sum() >= 40 and (v[t] < d2[t]).sum() >= 40
        sub = (d2 != 0) & (np.abs(d2) < sc._MIN[dt])
        assert sub.sum() >= 64 and ((d != 0) & (d2 == 0)).sum() >= 16
        assert ((v == 0) & np.signbit(v)).sum() >= 3 and (v < 0).sum() >= 4
        n = b["near"]
        assert np.all((v[n] >= d2[n] / 17) & (v[n] <= d2[n] * 17))
        lr_d = dt(sc.LR) * d[b["lrunder"]]
        assert ((lr_d == 0) | (np.abs(lr_d) < sc._MIN[dt])).all() and (lr_d == 0).any() and (lr_d != 0).any()
        # bigtheta: the update is under half an ulp, theta keeps its bits; cancel: theta' == 0
        for opt in ("adagrad", "yogi", "adam"):
            got = sx.fedopt_step(opt, th, d, v, sc.LR, sc.BETA2, sc.TAUS[0], dt)[0]
            assert sc.same(got[b["bigtheta"]], th[b["bigtheta"]])
        for i, opt in enumerate(("adagrad", "yogi", "adam")):
            sl = slice(b["cancel"].start + 16 * i, b["cancel"].start + 16 * i + 16)
            assert np.all(sx.fedopt_step(opt, th[sl], d[sl], v[sl], sc.LR, sc.BETA2, sc.TAUS[0], dt)[0] == 0)
        # tau = 0: 0/0 and x/0 lanes
        got = sx.fedopt_step("adagrad", th, d, v, sc.LR, sc.BETA2, 0.0, dt)[0][b["vzero"]]
        assert np.isnan(got).sum() >= 8 and np.isinf(got).sum() >= 4
    p = sc.FEDDR_PARAMS[0]
    tt, y, x = sc.feddr_case(dt)
    t = sx.feddr_combine(tt, y, x, p["alpha"], p["cx"], p["cy"], sx.PROX_NONE, p["pc"], dt)[0]
    pc = dt(p["pc"])
    assert (np.abs(t) == pc).sum() >= 16 and ((t == 0) & np.signbit(t)).sum() >= 64
    assert ((t == 0) & ~np.signbit(t)).sum() >= 64 and np.isnan(t).sum() >= 96


# ------------------------------------------------------------------------------------------------------ the teeth
_FEDOPT_TEETH = [(name, opt, tau) for name in sorted(sc.FEDOPT_MUTANTS) for opt in sc.FEDOPT_MUTANTS[name]
                 for tau in sc.mutant_taus(name)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name,opt,tau", _FEDOPT_TEETH)
def test_every_fedopt_mutant_differs_on_at_least_32_lanes(name, opt, tau, dt):
    """Every optimiser whose text the departure changes, at both tau values of the GPU tests (but for the one mutant
    that is no departure at tau = 0: step_cases.mutant_taus)."""
    th, d, v = sc.fedopt_case(dt)
    ref_t, ref_v = sx.fedopt_step(opt, th, d, v, sc.LR, sc.BETA2, tau, dt)
    mut_t, mut_v = sc.fedopt_mutant(name, opt, th, d, v, tau, dt)
    lanes = sc.differing(ref_t, mut_t) | sc.differing(ref_v, mut_v)
    assert lanes.sum() >= sc.TEETH, (name, opt, tau, int(lanes.sum()))


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", sc.FEDDR_MUTANTS)
def test_every_feddr_mutant_differs_on_at_least_32_lanes(name, dt):
    th, y, x = sc.feddr_case(dt)
    p = sc.FEDDR_PARAMS[0]
    ref_t, ref_y = sx.feddr_combine(th, y, x, p["alpha"], p["cx"], p["cy"], sx.PROX_L1, p["pc"], dt)
    mut_t, mut_y = sc.feddr_mutant(name, th, y, x, p, dt)
    assert sc.same(ref_y, mut_y)
    lanes = sc.differing(ref_t, mut_t)
    assert lanes.sum() >= sc.TEETH, (name, int(lanes.sum()))


def test_the_reference_is_its_own_zeroth_mutant():
    """The mutants' shared text with no departure is the reference: a difference counted above is the departure's."""
    for dt in DTYPES:
        th, d, v = sc.fedopt_case(dt)
        for opt in ("adagrad", "yogi", "adam"):
            for tau in sc.TAUS:
                a = sx.fedopt_step(opt, th, d, v, sc.LR, sc.BETA2, tau, dt)
                b = sc._fedopt_mutant("none", opt, th, d, v, sc.LR, sc.BETA2, tau, dt)
                assert sc.same(a[0], b[0]) and sc.same(a[1], b[1])


# ------------------------------------------------------------------------------------------------------ torch
def _tt(a):
    import torch

    return torch.from_numpy(np.array(a, copy=True))


def _against_torch(what, got, want, ref0=None, v_like=False, zero_or_finite=None):
    """Same class on every lane; finite lanes within the documented torch tolerance; the count in the message.
    ``zero_or_finite``: lanes on which a zero on one side may face a finite value on the other (still within the
    tolerance)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype
    cg, cw = sc.lane_class(got), sc.lane_class(want)
    num = (cg <= 2) & (cw <= 2)  # finite or zero on both sides
    strict = np.ones(got.shape, dtype=bool) if zero_or_finite is None else ~zero_or_finite
    bad = np.flatnonzero((cg != cw) & (strict | ~num))
    assert bad.size == 0, (what, "class differs on lanes", bad[:8].tolist(), got[bad[:8]], want[bad[:8]])
    diff = int(sc.differing(got, want).sum())
    f64 = got.dtype == F64
    if v_like:
        fin = (cg == 0) & (cw == 0)
        it = np.int64 if f64 else np.int32
        ulp = np.abs(got[fin].view(it).astype(np.int64) - want[fin].view(it).astype(np.int64))
        assert ulp.size == 0 or (ulp.max() <= 1 and (ulp > 0).mean() < 0.01), (what, f"{diff} lanes differ")
    else:
        g, w = got[num].astype(np.longdouble), want[num].astype(np.longdouble)
        upd = np.abs(w - ref0[num].astype(np.longdouble)) if ref0 is not None else np.abs(w)
        upd = np.where(np.isfinite(upd), upd, 0)
        rel = 1e-14 if f64 else 1e-6
        assert np.all(np.abs(g - w) <= rel * upd + np.spacing(np.abs(want[num]))), (what, f"{diff} lanes differ")
    return diff


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("opt", sc.OPTS)
def test_stepwise_fedopt_against_torch_on_the_catalogue(opt, tau, dt):
    """The catalogue's delta itself: no message and beta1 = 1, so torch's ``mul_(1.0)`` leaves every edge lane as it is
    (the ties, delta = +-0, delta^2 and lr * delta underflowing, x/0).  v has no sqrt in it and agrees bit for bit, so
    yogi's sign(0), the signed zeros and the subnormals are torch's.  theta divides by ``vp.sqrt() + tau`` and torch's
    CPU sqrt is not correctly rounded, hence the tolerance; on the ``cancel`` block, built so
    that theta' == 0 exactly under the IEEE square root, torch's last-bit-different denominator leaves ~1e-10 in place
    of the zero on a few lanes — there, and only there, a zero may face a finite value within the same tolerance."""
    from oracle import aggregation_ref as agg

    th, d, v = sc.fedopt_case(dt)
    e_t, e_v = sx.fedopt_step(opt, th, d, v, sc.LR, sc.BETA2, tau, dt)
    tt, td, tv = [_tt(th)], [_tt(d)], [_tt(v)]
    agg.fedopt_update(tt, td, None if opt == "avg" else tv, [], opt, sc.LR, (1.0, sc.BETA2), tau)
    assert sc.same(td[0].numpy(), d)
    if opt != "avg":
        n_v = int(sc.differing(e_v, tv[0].numpy()).sum())
        assert n_v == 0, f"v: {n_v} lanes differ"
    cancel = np.zeros(sc.N, dtype=bool)
    cancel[sc.blocks(dt)["cancel"]] = True
    _against_torch((opt, tau, "theta"), e_t, tt[0].numpy(), ref0=th, zero_or_finite=cancel)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("tau", sc.TAUS)
@pytest.mark.parametrize("opt", sc.OPTS)
def test_stepwise_fedopt_against_torch_after_a_fold(opt, tau, dt):
    """The fold in front (three messages on delta * 0.9), as a round runs it: the fma chain agrees bit for bit, the
    tail within the torch tolerance.  (The messages swamp the small-delta edges; the test above keeps them.)"""
    from oracle import aggregation_ref as agg

    th, d, v = sc.fedopt_case(dt)
    msgs = [np.asarray(m, dtype=dt) for m in sc.messages(3)]
    beta0 = 0.9
    w = (1 - beta0) / len(msgs)
    delta = sx.fold_chain(d, beta0, msgs, [w] * len(msgs), 0, dt)
    e_t, e_v = sx.fedopt_step(opt, th, delta, v, sc.LR, sc.BETA2, tau, dt)
    tt, td, tv = [_tt(th)], [_tt(d)], [_tt(v)]
    agg.fedopt_update(tt, td, None if opt == "avg" else tv, [{"delta_parameters": [_tt(m)]} for m in msgs], opt, sc.LR,
                      (beta0, sc.BETA2), tau)
    n_d = int(sc.differing(delta, td[0].numpy()).sum())
    assert n_d == 0, f"the fold is an fma chain on both sides: {n_d} lanes differ"
    if opt != "avg":
        _against_torch((opt, tau, "v"), e_v, tv[0].numpy(), v_like=True)
    _against_torch((opt, tau, "theta"), e_t, tt[0].numpy(), ref0=th)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("reg,prox", [("none", sx.PROX_NONE), ("l1", sx.PROX_L1), ("l2squared", sx.PROX_SCALE)])
@pytest.mark.parametrize("num_clients,eta,alpha", [(3, 0.01, 0.3), (10, 0.1, 1.9)])
def test_stepwise_feddr_against_torch(num_clients, eta, alpha, reg, prox, dt):
    """No sqrt is involved: bit for bit."""
    from oracle import aggregation_ref as agg

    th, y, x = sc.feddr_case(dt)
    coeff = eta * num_clients / (num_clients + 1)
    pc = 1 / (1 + 2 * coeff) if prox == sx.PROX_SCALE else coeff
    e_t, e_y = sx.feddr_combine(th, y, x, alpha, coeff / eta, 1 / (num_clients + 1), prox, pc, dt)
    tt, ty, tx = [_tt(th)], [_tt(y)], [_tt(x)]
    agg.feddr_update(tt, ty, tx, [], alpha, eta, num_clients, reg)
    for name, e, t in (("y", e_y, ty[0]), ("theta", e_t, tt[0])):
        n_diff = int(sc.differing(e, t.numpy()).sum())
        assert n_diff == 0, f"{reg} {name}: {n_diff} lanes differ"


def test_stepwise_feddyn_and_pfedme_against_torch():
    from oracle import aggregation_ref as agg

    th, h, _ = sc.fedopt_case(F32)
    for count in (1, 3, 17):
        msgs = sc.messages(count)
        w = [1 / count] * count
        tmsgs = [{"parameters": [_tt(m)], "train_samples": 1} for m in msgs]
        e_t, e_h = sx.server_fold("feddyn", th, h, msgs, w, -0.1 / 10)
        tt, thh = [_tt(th)], [_tt(h)]
        agg.feddyn_update(tt, thh, tmsgs, 0.1, 10)
        assert _against_torch(("feddyn", count, "h"), e_h, thh[0].numpy(), v_like=True) == 0
        assert _against_torch(("feddyn", count, "theta"), e_t, tt[0].numpy(), v_like=True) == 0
        e_t, _ = sx.server_fold("pfedme", th, None, msgs, w, 0.7)
        tt = [_tt(th)]
        agg.pfedme_update(tt, tmsgs, 0.7)
        assert _against_torch(("pfedme", count, "theta"), e_t, tt[0].numpy(), v_like=True) == 0
        # the !FOLD forms compute the same values in two steps
        avg = sx.fold_chain(th, 0.0, msgs, w, 0)
        assert sc.same(sx.server_fold("pfedme", avg, th, [], [], 0.7, fold=False)[0], e_t)
        assert sc.same(sx.server_fold("feddyn", th, h, msgs, w, -0.1 / 10, fold=False)[1], e_h)
