"""CPU checks of the path-directed select inputs (tests/select_cases.py) at the plan of a 256-CU device: every case's
class-level preconditions make its path unavoidable for any floor / ceiling the pick may choose, the numpy mirror of
the keys is the oracle's, and the oracle itself (oracle/compressors_ref.py) keeps exactly k entries on each input and
resolves ties of the K-th value towards the highest indices."""

import numpy as np
import pytest

from fl_sim_amd import codec
from oracle import compressors_ref as ref
from tests import select_cases as sc

CUS = 256


def plan_of(n, k, clients=0):
    return codec.topk_select_plan(n, k, clients, CUS)


SINGLE, N1, K1, N2 = sc.single_cases(plan_of)
STORAGE = sc.storage_cases(plan_of)


def _oracle_sane(x, k):
    idx, val = ref.topk_kept(x, k)
    assert idx.size == k and np.all(np.diff(idx) > 0)
    keys = sc.order_key(x)
    T = sc.kth_key(x, k)
    kept = np.zeros(x.size, bool)
    kept[idx] = True
    assert kept[keys > T].all() and not kept[keys < T].any()
    ties = np.flatnonzero(keys == T)
    need = k - int((keys > T).sum())
    assert 1 <= need <= ties.size
    assert np.array_equal(np.flatnonzero(kept & (keys == T)), ties[ties.size - need:])  # the highest indices
    i2, v2 = ref.topk_kept_select(x, k)
    assert np.array_equal(i2, idx) and np.array_equal(v2.view(np.uint32), val.view(np.uint32))


def test_key_mirror_matches_the_oracle_and_inverts():
    g = np.random.default_rng(0)
    x = g.standard_normal(10_000).astype(np.float32)
    x[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e-45, -1e-45]
    k = sc.order_key(x)
    assert np.array_equal(k, ref.order_keys(x))
    assert k[0] == k[1] == 0x80000000 and k[2] == sc.KEY_INF and k[4] == k[5] == sc.KEY_NAN
    fin = ~np.isnan(x)
    back = sc.key_value(k[fin])
    assert np.array_equal(sc.order_key(back), k[fin])
    assert np.array_equal(np.argsort(k[fin], kind="stable"), np.argsort(x[fin], kind="stable"))
    d = g.standard_normal(1000)
    d[:4] = [0.0, -0.0, np.nan, np.inf]
    k64 = sc.order_key64(d)
    assert k64[0] == k64[1] and k64[2] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert np.array_equal(np.argsort(k64[3:], kind="stable"), np.argsort(d[3:], kind="stable"))


def test_catalogue_names():
    assert sorted(SINGLE) == sorted(sc.SINGLE_NAMES) and sorted(STORAGE) == sorted(sc.STORAGE_NAMES)


def test_sample_positions():
    assert np.array_equal(sc.sample_positions(20_000, 20_000), np.arange(20_000))
    p = sc.sample_positions(N1, 32768)
    assert p.size == 32768 and np.all(np.diff(p) > 0) and 0 <= p[0] and p[-1] < N1
    assert p[0] == int(0.5 * N1 / 32768) and p[12345] == int(12345.5 * N1 / 32768)


def test_plan_shapes_the_cases_rely_on():
    p = plan_of(N1, K1)
    assert p["S"] < N1 and p["G"] > 3 and p["rank_hi"] > 0 and p["rank_lo"] <= p["fast_rank"] and p["compact"]
    assert p["M"] * (p["G"] - 1) < N1 < p["M"] * p["G"]  # a ragged last block
    assert plan_of(N1, N1 * 5 // 100)["rank_lo"] > p["fast_rank"]
    assert plan_of(20_000, 10_000)["S"] == 20_000 and not plan_of(20_000, 10_000)["take_all"]
    assert plan_of(20_000, 19_600)["take_all"] and plan_of(N1, N1 - 1)["take_all"]
    assert plan_of(N1, 1)["rank_hi"] == 0 and plan_of(N1, 40)["rank_hi"] == 0
    q = plan_of(N2, N2 // 100)
    assert q["M"] > q["cap"] and q["ovf"] == 0 and N2 == 2 * CUS * q["cap"] - 3
    b3, b2 = plan_of(70_001, 700, 3), plan_of(N1, K1, 2)
    assert b3["S"] == 4096 and b3["G"] * 3 <= CUS and b3["list_cap"] == min(256, b3["list_all"] // b3["G"])
    assert 4096 <= b2["S"] <= 32768 and b2["G"] * 2 <= CUS and not b2["compact"]


@pytest.mark.parametrize("name", sorted(SINGLE))
def test_single_case_reaches_its_path(name):
    case = SINGLE[name]()
    plan = plan_of(case.x.size, case.k)
    sc.precondition(case, plan)
    _oracle_sane(case.x, case.k)


@pytest.mark.parametrize("name", sorted(STORAGE))
def test_storage_case_reaches_its_path(name):
    case = STORAGE[name]()
    plan = plan_of(case.x.size, case.k)
    assert plan["M"] > plan["cap"]
    sc.precondition(case, plan)
    idx, _ = ref.topk_kept_select(case.x, case.k)  # (the stable argsort of 8 M elements runs in the GPU test)
    assert idx.size == case.k


def test_zero_tie_cuts():
    x, k_above, nt, cuts = sc.zero_tie_cuts(plan_of)
    zeros = np.flatnonzero(x == 0)
    assert zeros.size == nt and np.signbit(x[zeros]).any() and not np.signbit(x[zeros]).all()
    M = plan_of(N1, k_above)["M"]
    blocks = set((zeros // M).tolist())
    assert 0 in blocks and (N1 - 1) // M in blocks and any(z % M == M - 1 and z + 1 in zeros for z in zeros)
    for k, what in cuts:
        case = sc.Case(f"n_zero_ties_{what}", x, k, {"fallback": 0, "rerange": False, "rounds_one": True})
        sc.precondition(case, plan_of(N1, k))
        _oracle_sane(x, k)
        assert sc.kth_key(x, k) == 0x80000000


@pytest.mark.parametrize("n,k,clients", [(70_001, 700, 3), (70_001, 40, 3), (N1, K1, 2), (N1, 40, 2)])
def test_batched_cases_reach_their_paths(n, k, clients):
    for which in (("e",) if k == 40 else ("h", "l_over", "l_ctrl")):
        case = sc.batch_cases(lambda n_, k_: plan_of(n_, k_, clients), n, k, which)
        sc.precondition(case, plan_of(n, k, clients))
        _oracle_sane(case.x, k)


def test_planting_near_the_band_leaves_the_sample_alone():
    case = SINGLE["a_fast_compact"]()
    plan = plan_of(N1, K1)
    k_lo, k_hi = sc.sample_rank_keys(case.x, plan)
    pos = sc.sample_positions(N1, plan["S"])
    planted = sc.plant_near_band(case.x, K1, plan, k_lo - 100, k_hi + 100, 3)
    assert len(planted) == 10
    for key, y in planted:
        assert np.array_equal(y[pos].view(np.uint32), case.x[pos].view(np.uint32))
        assert sc.kth_key(y, K1) == key and int((sc.order_key(y) == key).sum()) == 64
        assert int((sc.order_key(y) > key).sum()) == K1 - 32


def test_float64_cases():
    n, sample = 1 << 20, 16384
    cases = sc.f64_cases(n, sample)
    assert {c[0] for c in cases} == {"g", "i", "j", "n"}
    for name, (x, k, fb) in cases.items():
        exp, _ = ref.topk(x, k)
        assert fb in (0, 1), name
        keys = sc.order_key64(x)
        T = np.partition(keys, n - k)[n - k]
        kept = (keys > T)
        ties = np.flatnonzero(keys == T)
        need = k - int(kept.sum())
        kept[ties[ties.size - need:]] = True
        assert np.array_equal(np.where(kept, x, 0.0).view(np.uint64), exp.view(np.uint64)), name
