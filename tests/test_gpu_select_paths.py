"""Path-directed parity tests of the exact top-k selects (gfx950).  Every input of tests/select_cases.py is built,
from the plan of the device at hand, to drive the select down one named path (compact sample rejected, general
pick, take-all, refinement, fallback pass, re-range above the ceiling, in-bin list overflow, g-mode, x-mode, ...).
Each test runs an entry point, reads what the select recorded (codec.topk_select_stats) and asserts

1. bit-exact parity with oracle/compressors_ref.py (kept indices, values / codes, norm, tile pointers, decode);
2. a clean error word;
3. the path: the recorded sample path, fallback flag and rounds, the K-th key, the candidate count against the
   numpy model evaluated at the kernel's own floor and ceiling, and the model's g-mode / x-mode / list predicates.

A case that no longer reaches its path fails (check_expect names the plan numbers); none skips."""

import functools
import time

import numpy as np
import pytest
import torch

from oracle import compressors_ref as ref
from tests import golden_cases as gc
from tests import golden_f64 as g64
from tests import select_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, CTR, LEVELS = 7, 3, 127


def _codec():
    from fl_sim_amd import codec

    return codec


def plan_of(n, k, clients=0):
    return _codec().topk_select_plan(n, k, clients, 0)


NAMES = sc.SINGLE_NAMES + sc.STORAGE_NAMES
# (a NaN or an infinity among the kept values makes the stacked norm non-finite: case g runs the plain top-k only)
STACKED_NAMES = tuple(n for n in NAMES if not n.startswith("g_"))
DAGGER = tuple(n for n in NAMES if n[0] in "ehlop")  # the cases that also run through the delta encoder


@functools.lru_cache(maxsize=None)
def _catalogue():
    single = sc.single_cases(plan_of)[0]
    single.update(sc.storage_cases(plan_of))
    assert sorted(single) == sorted(NAMES)
    return single


@functools.lru_cache(maxsize=None)
def _built(name):
    case = _catalogue()[name]()
    return case, ref.topk_kept(case.x, case.k)


def _check_path(case, plan, st, clients=0):
    """The select's record against the case and the numpy model at the kernel's own floor and ceiling."""
    x, k, e = case.x, case.k, case.expect
    tag = f"{case.name}: n={x.size} k={k} plan={plan} stats={st}"
    keys = sc.order_key(x)
    T = sc.kth_key(x, k)
    assert st["T"] == T, tag
    assert st["strict"] == int((keys > T).sum()) and st["ties"] == int((keys == T).sum()), tag
    assert st["need"] == k - st["strict"] and st["maxkey"] == int(keys.max()), tag
    if plan["take_all"]:
        assert st["sample_path"] == 2 and st["t_lo"] == 0 and st["t_hi"] == sc.NO_CEILING, tag
    facts = sc.path_facts(x, k, plan, st["t_lo"], st["t_hi"])
    assert st["C"] == facts["C"], tag  # (also validates the mirror of keys, positions and block geometry)
    assert st["fallback"] == int(facts["fallback"]), tag
    assert (st["C"] < k) == bool(st["fallback"]), tag
    assert (st["rounds"] == 1) == facts["rounds_one"], (tag, {f: v for f, v in facts.items() if f != "pred"})
    sc.check_expect(case, plan, facts, "device")
    if "sample_path" in e:
        assert st["sample_path"] == e["sample_path"], tag
    if e.get("no_ceiling"):
        assert st["t_hi"] == sc.NO_CEILING, tag
    if "t_lo" in e:
        assert st["t_lo"] == e["t_lo"], tag
    if "band" in e:
        assert (st["t_lo"], st["t_hi"]) == e["band"], tag
    if "run" in e:  # (case f) both ranks refined: at most a second-pass bin (2^(32 - 2 hist_bits) keys) off their keys
        k_lo, k_hi = sc.sample_rank_keys(x, plan)
        fine = 1 << (32 - 2 * plan["hist_bits"])
        assert e["run"][0] <= st["t_lo"] <= k_lo and k_lo - st["t_lo"] < fine, tag
        assert k_hi < st["t_hi"] <= k_hi + fine and st["t_hi"] <= e["run"][1] + 1, tag
    return facts


def _check_tiles(tiles, exp_idx, k):
    t = tiles.cpu().numpy().astype(np.int64)
    assert t[-1] == k and np.array_equal(t[:-1], np.searchsorted(exp_idx, np.arange(len(t) - 1) * _codec().TILE))


def _check_plain(x, k, idx, val, tiles, exp):
    exp_idx, exp_val = exp
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), exp_idx), "kept index set / order differs"
    assert gc.same_bits(val.cpu().numpy(), exp_val)
    if tiles is not None:
        _check_tiles(tiles, exp_idx, k)


def _check_stacked(x, k, pkt, exp, seed, counter, decode=True):
    exp_out, exp_idx, exp_codes, pn = ref.stacked(x, k, LEVELS, lambda i: ref.philox_uniforms_at(i, seed, counter),
                                                  fast=True)
    assert np.array_equal(exp_idx, exp[0])  # (the O(n) select of the oracle agrees with its stable argsort)
    assert np.array_equal(pkt.idx.cpu().numpy().astype(np.int64), exp_idx), "kept index set / order differs"
    assert np.array_equal(pkt.codes[:k].cpu().numpy(), exp_codes)
    assert gc.same_bits(pkt.norm.cpu().numpy().reshape(1), np.array([pn], dtype=np.float32))
    _check_tiles(pkt.tiles, exp_idx, k)
    if decode:
        assert gc.same_bits(_codec().stacked_decode(pkt).cpu().numpy(), exp_out)


def _report(name, entry, case, st, t0):
    print(f"\n[select-path] {name} {entry}: n={case.x.size} k={case.k} sample_path={st['sample_path']} "
          f"fallback={st['fallback']} rounds={st['rounds']} C={st['C']} t_lo={st['t_lo']:#x} t_hi={st['t_hi']:#x} "
          f"wall={time.perf_counter() - t0:.2f}s")


@pytest.mark.parametrize("name", NAMES)
def test_select_path_topk(name):
    codec = _codec()
    t0 = time.perf_counter()
    case, exp = _built(name)
    x, k = case.x, case.k
    idx, val, tiles = codec.topk_encode(torch.from_numpy(x).to(DEV), k, with_tiles=True)
    st = codec.topk_select_stats()
    _check_plain(x, k, idx, val, tiles, exp)
    assert codec.topk_status(reset=True) == 0
    _check_path(case, plan_of(x.size, k), st)
    _report(name, "topk_encode", case, st, t0)


@pytest.mark.parametrize("name", STACKED_NAMES)
def test_select_path_stacked(name):
    codec = _codec()
    t0 = time.perf_counter()
    case, exp = _built(name)
    x, k = case.x, case.k
    pkt = codec.stacked_encode(torch.from_numpy(x).to(DEV), k, LEVELS, seed=SEED, counter=CTR)
    st = codec.topk_select_stats()
    _check_stacked(x, k, pkt, exp, SEED, CTR)
    assert codec.topk_status(reset=True) == 0
    _check_path(case, plan_of(x.size, k), st)
    _report(name, "stacked_encode", case, st, t0)


def _misaligned(t):
    """A copy of ``t`` that starts 4 bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 5, dtype=torch.float32, device=t.device)
    off = 1 + (-(buf.data_ptr() // 4) % 4)
    v = buf[off:off + t.numel()]
    assert v.data_ptr() % 16 == 4
    v.copy_(t)
    return v


@pytest.mark.parametrize("name", DAGGER)
def test_select_path_through_the_delta_encoder(name):
    """The same select behind flc_stacked_encode_delta: three tensors, the middle one misaligned; local - 0 = x."""
    codec = _codec()
    case, exp = _built(name)
    x, k = case.x, case.k
    n = x.size
    xd = torch.from_numpy(x).to(DEV)
    cuts = [0, n // 3 + 1, 2 * n // 3 + 2, n]
    local = [xd[a:b].clone() for a, b in zip(cuts, cuts[1:])]
    local[1] = _misaligned(local[1])
    glob = [torch.zeros_like(t) for t in local]
    glob[1] = _misaligned(glob[1])
    pkt = codec.stacked_encode_delta(local, glob, k, LEVELS, seed=SEED, counter=CTR)
    st = codec.topk_select_stats()
    _check_stacked(x, k, pkt, exp, SEED, CTR, decode=False)
    assert codec.topk_status(reset=True) == 0
    _check_path(case, plan_of(n, k), st)


@pytest.mark.parametrize("what", ["first", "middle", "last"])
def test_zero_ties_across_blocks(what):
    """Case n: +-0 ties of the K-th value in the first block, the ragged last block and either side of a block
    boundary, cut at their first, middle and last member; each kept zero keeps its own sign bit."""
    codec = _codec()
    x, k_above, nt, cuts = _zero_ties()
    k = dict((w, kk) for kk, w in cuts)[what]
    plan = plan_of(x.size, k)
    case = sc.Case(f"n_zero_ties_{what}", x, k, {"fallback": 0, "rerange": False, "rounds_one": True})
    exp = ref.topk_kept(x, k)
    kept_zero = exp[1][exp[1] == 0]
    assert kept_zero.size == {"first": nt, "middle": nt // 2, "last": 1}[what]
    xd = torch.from_numpy(x).to(DEV)
    idx, val, tiles = codec.topk_encode(xd, k, with_tiles=True)
    st = codec.topk_select_stats()
    _check_plain(x, k, idx, val, tiles, exp)
    assert np.array_equal(np.signbit(val.cpu().numpy()), np.signbit(exp[1]))
    _check_path(case, plan, st)
    assert st["T"] == 0x80000000 and st["ties"] == nt
    pkt = codec.stacked_encode(xd, k, LEVELS, seed=SEED, counter=CTR)
    _check_stacked(x, k, pkt, exp, SEED, CTR)
    _check_path(case, plan, codec.topk_select_stats())
    assert codec.topk_status(reset=True) == 0


@functools.lru_cache(maxsize=1)
def _zero_ties():
    return sc.zero_tie_cuts(plan_of)


def test_keys_beside_the_floor_and_the_ceiling():
    """Case k: a first run gives the kernel's own floor and ceiling; 64 copies each of the keys one ulp and one
    band-bin width either side of both are planted where the sample never looks, and each in turn is made the K-th
    largest of a select with the same k (so the same floor and ceiling)."""
    codec = _codec()
    case, _ = _built("a_fast_compact")
    x, k = case.x, case.k
    plan = plan_of(x.size, k)
    codec.topk_encode(torch.from_numpy(x).to(DEV), k)
    st0 = codec.topk_select_stats()
    t_lo, t_hi = st0["t_lo"], st0["t_hi"]
    assert t_lo > 0 and t_hi < sc.NO_CEILING, st0
    planted = sc.plant_near_band(x, k, plan, t_lo, t_hi, 5)
    assert len(planted) == 10
    for key, y in planted:
        exp = ref.topk_kept(y, k)
        yd = torch.from_numpy(y).to(DEV)
        c = sc.Case(f"k_key_{key:#x}", y, k, {"fallback": int(key < t_lo), "rerange": key >= t_hi})
        idx, val, tiles = codec.topk_encode(yd, k, with_tiles=True)
        st = codec.topk_select_stats()
        assert (st["t_lo"], st["t_hi"]) == (t_lo, t_hi), (hex(key), st, st0)
        _check_plain(y, k, idx, val, tiles, exp)
        _check_path(c, plan, st)
        assert st["T"] == key and st["ties"] == 64 and st["need"] == 32, (hex(key), st)
        assert (st["rounds"] > 1) == (key < t_lo or key >= t_hi), (hex(key), st)
        pkt = codec.stacked_encode(yd, k, LEVELS, seed=SEED, counter=CTR)
        _check_stacked(y, k, pkt, exp, SEED, CTR, decode=False)
        _check_path(c, plan, codec.topk_select_stats())
    assert codec.topk_status(reset=True) == 0


@pytest.mark.parametrize("n,k,whiches", [(70_001, 700, ("h", "l_over", "l_ctrl")), (70_001, 40, ("e", "e", "e")),
                                         (1_048_573, 10_485, ("l_over", "h")), (1_048_573, 40, ("e", "e"))])
def test_batched_select_paths(n, k, whiches):
    """The † cases a batched client's geometry can reach, one case per client, through stacked_encode_batch with
    distinct per-message counters and through topk_encode_batch; each client's own header is read."""
    codec = _codec()
    C = len(whiches)
    plan = plan_of(n, k, C)
    assert plan["chunk"] == C
    cases = [sc.batch_cases(lambda n_, k_: plan_of(n_, k_, C), n, k, w, salt=c) for c, w in enumerate(whiches)]
    exps = [ref.topk_kept(cs.x, k) for cs in cases]
    xs = [torch.from_numpy(cs.x).to(DEV) for cs in cases]
    seeds, counters = [11 + c for c in range(C)], [100 + 7 * c for c in range(C)]
    pks = codec.stacked_encode_batch(xs, k, LEVELS, seeds=seeds, counters=counters)
    stats = [codec.topk_select_stats(kind="topk_batch", client=c) for c in range(C)]
    assert codec.topk_status(reset=True) == 0
    for c in range(C):
        _check_stacked(cases[c].x, k, pks[c], exps[c], seeds[c], counters[c])
        _check_path(cases[c], plan, stats[c])
    outs = codec.topk_encode_batch(xs, k, with_tiles=True)
    stats = [codec.topk_select_stats(kind="topk_batch", client=c) for c in range(C)]
    assert codec.topk_status(reset=True) == 0
    for c in range(C):
        _check_plain(cases[c].x, k, *outs[c], exps[c])
        _check_path(cases[c], plan, stats[c])


def test_float64_select_paths():
    """Cases g, i, j, n on the float64 select: parity with the oracle, the band geometry against its numpy mirror,
    the K-th key and its ties, and whether the exact passes over x ran (fb)."""
    codec = _codec()
    n = 1 << 20
    x0 = torch.zeros(n, dtype=torch.float64, device=DEV)
    x0[::7] = 1.0
    codec.topk_dense_f64(x0, 1000)
    sample = codec.topk_stats_f64(x0, 1000)["sample"]
    for name, (x, k, fb) in sorted(sc.f64_cases(n, sample).items()):
        xd = torch.from_numpy(x).to(DEV)
        got = codec.topk_dense_f64(xd, k)
        st = codec.topk_stats_f64(xd, k)
        exp, _ = ref.topk(x, k)
        assert g64.same_bits(got.cpu().numpy(), exp), name
        S, r_lo, r_hi, on = sc.filt64(n, k, sample)
        assert (st["S"], st["r_lo"], st["r_hi"], st["on"]) == (S, r_lo, r_hi, int(on)), (name, st)
        keys = sc.order_key64(x)
        T = int(np.partition(keys, n - k)[n - k])
        assert st["err"] == 0 and st["T"] == T, (name, st)
        assert st["ties"] == int((keys == np.uint64(T)).sum()), (name, st)
        assert st["need"] == k - int((keys > np.uint64(T)).sum()), (name, st)
        assert st["fb"] == fb, (name, st)
    assert sum(codec.topk_status_all().values()) == 0


def test_error_words_are_clear_at_the_end():
    assert sum(_codec().topk_status_all().values()) == 0
