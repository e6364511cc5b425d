"""Top-k by magnitude on the device (gfx950), bit for bit against tests/topk_magnitude_ref.py (the oracle's functions on
``|x|``): the 27 path-directed select inputs with half their sign bits flipped (every path of the signed select, its
recorded diagnostics unchanged), the small shapes and edge classes, the batched encoders against one single-client call
per client, the batch key of the deferred encodes, and float64.  A clean error word after each."""

import functools

import numpy as np
import pytest
import torch

from oracle import compressors_ref as ref
from tests import golden_cases as gc
from tests import golden_f64 as g64
from tests import select_cases as sc
from tests import test_gpu_select_paths as sp
from tests import topk_magnitude_ref as mref

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, CTR, LEVELS = 7, 3, 127
FLIP = 20_260


def _codec():
    from fl_sim_amd import codec

    return codec


def MAG():
    return _codec().ORDER_MAGNITUDE


@pytest.fixture(autouse=True)
def _clean_error_word():
    yield
    assert sum(_codec().topk_status_all().values()) == 0


@functools.lru_cache(maxsize=None)
def _flipped(name):
    """(case, x' = case.x with half its sign bits flipped, the signed oracle's kept set of x = |x'|)."""
    case, exp = sp._built(name)
    assert not np.signbit(case.x).any()
    xf = mref.flip_signs(case.x, FLIP)
    assert np.array_equal(np.abs(xf).view(np.uint32), case.x.view(np.uint32))
    return case, xf, exp


def _check_plain(xf, k, idx, val, tiles, exp_idx):
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), exp_idx), "kept index set / order differs"
    assert gc.same_bits(val.cpu().numpy(), xf[exp_idx])
    if tiles is not None:
        sp._check_tiles(tiles, exp_idx, k)


def _check_stacked(xf, k, pkt, exp_idx, seed, counter, levels=LEVELS, decode=True):
    out, idx, codes, pn = mref.stacked(xf, k, levels, lambda i: ref.philox_uniforms_at(i, seed, counter), fast=True)
    assert np.array_equal(idx, exp_idx)
    assert np.array_equal(pkt.idx.cpu().numpy().astype(np.int64), idx), "kept index set / order differs"
    assert np.array_equal(pkt.codes[:k].cpu().numpy(), codes)
    assert gc.same_bits(pkt.norm.cpu().numpy().reshape(1), np.array([pn], dtype=np.float32))
    sp._check_tiles(pkt.tiles, idx, k)
    if decode:
        assert gc.same_bits(_codec().stacked_decode(pkt).cpu().numpy(), out)


# ------------------------------------------------------------------------------------------------ 4. the paths
@pytest.mark.parametrize("name", sp.NAMES)
def test_select_path_topk_by_magnitude(name):
    codec = _codec()
    case, xf, exp = _flipped(name)
    k = case.k
    idx, val, tiles = codec.topk_encode(torch.from_numpy(xf).to(DEV), k, with_tiles=True, order=MAG())
    st = codec.topk_select_stats()
    _check_plain(xf, k, idx, val, tiles, exp[0])
    assert codec.topk_status(reset=True) == 0
    sp._check_path(case, sp.plan_of(xf.size, k), st)  # the signed select's record on |x'| = x


@pytest.mark.parametrize("name", sp.STACKED_NAMES)
def test_select_path_stacked_by_magnitude(name):
    codec = _codec()
    case, xf, exp = _flipped(name)
    k = case.k
    pkt = codec.stacked_encode(torch.from_numpy(xf).to(DEV), k, LEVELS, seed=SEED, counter=CTR, order=MAG())
    st = codec.topk_select_stats()
    _check_stacked(xf, k, pkt, exp[0], SEED, CTR)
    assert codec.topk_status(reset=True) == 0
    sp._check_path(case, sp.plan_of(xf.size, k), st)


@pytest.mark.parametrize("name", sp.DAGGER)
def test_select_path_by_magnitude_through_the_delta_encoder(name):
    """Three tensors, the middle one misaligned; local - 0 = x', selected by |local - global|."""
    codec = _codec()
    case, xf, exp = _flipped(name)
    k, n = case.k, xf.size
    xd = torch.from_numpy(xf).to(DEV)
    cuts = [0, n // 3 + 1, 2 * n // 3 + 2, n]
    local = [xd[a:b].clone() for a, b in zip(cuts, cuts[1:])]
    local[1] = sp._misaligned(local[1])
    glob = [torch.zeros_like(t) for t in local]
    glob[1] = sp._misaligned(glob[1])
    pkt = codec.stacked_encode_delta(local, glob, k, LEVELS, seed=SEED, counter=CTR, order=MAG())
    st = codec.topk_select_stats()
    _check_stacked(xf, k, pkt, exp[0], SEED, CTR, decode=False)
    assert codec.topk_status(reset=True) == 0
    sp._check_path(case, sp.plan_of(n, k), st)


# ------------------------------------------------------------------------------------------------ 5. small shapes
SMALL_NS = (2, 7, 1023, 1025, 4099, 65537)
CLASSES = ("all_negative", "pm_pairs", "all_equal", "pm_zeros", "pm_inf", "pm_nan", "denormals")


def small_ks(n):
    return sorted({K for K in (1, 2, n // 2, n - 1) if 0 < K < n})


def _distinct(g, n):
    """n distinct positive magnitudes in [2^-9, 2^-8), one ulp apart, shuffled."""
    return (np.uint32(0x3B000000) + g.permutation(n).astype(np.uint32)).view(np.float32)


def small_input(cls, n, K, seed=5):
    g = np.random.default_rng(1000 * seed + 7 * n + K)
    sign = np.where(g.random(n) < 0.5, np.float32(-1), np.float32(1))
    if cls == "all_negative":  # the signed rule keeps the SMALLEST magnitudes here
        return -_distinct(g, n)
    if cls == "pm_pairs":  # the K-th and (K + 1)-th largest magnitudes are +v and -v: the higher index is kept
        m = _distinct(g, n)
        order = np.argsort(m)[::-1]
        a, b = order[K - 1], order[K]
        m[b] = m[a]
        x = m * sign
        x[min(a, b)], x[max(a, b)] = abs(x[a]), -abs(x[a])
        return x.astype(np.float32)
    if cls == "all_equal":
        return (np.float32(0.375) * sign).astype(np.float32)
    if cls == "pm_zeros":  # fewer non-zero entries than K (when K > 1): K reaches into the +-0 tie class
        x = (np.float32(0.0) * sign).astype(np.float32)
        nz = g.choice(n, size=max(0, min(K - 1, n // 3)), replace=False)
        x[nz] = (_distinct(g, n) * sign)[nz]
        return x
    if cls == "pm_inf":
        x = (_distinct(g, n) * sign).astype(np.float32)
        at = g.choice(n, size=min(n, 5), replace=False)
        x[at] = np.array([np.inf, -np.inf, -np.inf, np.inf, -np.inf], dtype=np.float32)[:at.size]
        return x
    if cls == "pm_nan":
        x = (_distinct(g, n) * sign).astype(np.float32)
        at = g.choice(n, size=min(n, 4), replace=False)
        x.view(np.uint32)[at] = np.array([0x7FC00000, 0xFFC00000, 0xFF800001, 0x7F800100], dtype=np.uint32)[:at.size]
        return x
    if cls == "denormals":
        b = g.permutation(0x7FFFFF)[:n].astype(np.uint32) + np.uint32(1)
        b |= (g.random(n) < 0.5).astype(np.uint32) << np.uint32(31)
        return b.view(np.float32)
    raise KeyError(cls)


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("n", SMALL_NS)
def test_small_shapes_and_edge_classes(n, cls):
    codec = _codec()
    for K in small_ks(n):
        x = small_input(cls, n, K)
        exp_idx, exp_val = mref.kept(x, K)
        assert np.array_equal(mref.kept(x, K, fast=True)[0], exp_idx)
        xd = torch.from_numpy(x).to(DEV)
        idx, val, tiles = codec.topk_encode(xd, K, with_tiles=True, order=MAG())
        _check_plain(x, K, idx, val, tiles, exp_idx)
        assert gc.same_bits(val.cpu().numpy(), exp_val), (cls, n, K)
        if cls == "all_negative":  # the largest magnitudes, not the signed rule's smallest
            assert np.abs(exp_val).min() >= np.sort(np.abs(x))[n - K]
            sidx = codec.topk_encode(xd, K)[0].cpu().numpy()
            assert not np.array_equal(sidx, exp_idx)
        pkt = codec.stacked_encode(xd, K, LEVELS, seed=SEED, counter=CTR + K, order=MAG())
        if cls in ("pm_inf", "pm_nan"):
            # a non-finite norm follows the existing rule: exactly what the signed encoder makes of |x| (same kept set,
            # no sign in the codes of a non-regular norm)
            ps = codec.stacked_encode(torch.from_numpy(np.abs(x)).to(DEV), K, LEVELS, seed=SEED, counter=CTR + K)
            assert np.array_equal(pkt.idx.cpu().numpy().astype(np.int64), exp_idx)
            assert torch.equal(pkt.idx, ps.idx) and torch.equal(pkt.tiles, ps.tiles)
            assert gc.same_bits(pkt.norm.cpu().numpy(), ps.norm.cpu().numpy())
            nrm = float(pkt.norm.cpu().numpy()[0])
            assert not (0 < nrm < np.inf), (cls, n, K, nrm)
            assert torch.equal(pkt.codes[:K], ps.codes[:K])
        else:
            _check_stacked(x, K, pkt, exp_idx, SEED, CTR + K)
        assert codec.topk_status(reset=True) == 0


@pytest.mark.parametrize("n", [7, 4100])
def test_compressor_by_magnitude_device_and_host_inputs(n):
    """compressVector (device tensor, host array), compressBatch and the encode-only helper honour the order; K <= 0 and
    K >= d copy x."""
    from fl_sim_amd import Compressor

    g = np.random.default_rng(n)
    x = (g.standard_normal(n) * 1e-3).astype(np.float32)
    K = max(1, n // 10)
    c = Compressor()
    c.makeTopKCompressor(K, n, magnitude=True)
    want = mref.topk(x, K)
    assert (want < 0).any()
    assert gc.same_bits(c.compressVector(torch.from_numpy(x).to(DEV)).cpu().numpy(), want)
    assert gc.same_bits(c.compressVector(x), want)
    assert c.last_need_to_send_advance == K and c.total_input_components == 2 * n
    if n % 4 == 0:  # (compressBatch decodes into the rows of one block: 16-B rows, in either order)
        X = np.stack([x, -x, x[::-1].copy()])
        got = c.compressBatch(torch.from_numpy(X).to(DEV)).cpu().numpy()
        for r in range(3):
            assert gc.same_bits(got[r], mref.topk(X[r], K)), r
    idx, val, tiles = c.encode(torch.from_numpy(x).to(DEV))
    _check_plain(x, K, idx, val, tiles, mref.kept(x, K)[0])
    assert gc.same_bits(c.decode((idx, val, tiles), n).cpu().numpy(), want)
    for Kq in (0, n, n + 3):
        q = Compressor()
        q.makeTopKCompressor(Kq, n, magnitude=True)
        assert gc.same_bits(q.compressVector(torch.from_numpy(x).to(DEV)).cpu().numpy(), x)


# ------------------------------------------------------------------------------------------------ 6. batched
def _same_packet(a, b, k):
    assert torch.equal(a.idx, b.idx) and torch.equal(a.codes[:k], b.codes[:k]) and torch.equal(a.tiles, b.tiles)
    assert gc.same_bits(a.norm.cpu().numpy().reshape(1), b.norm.cpu().numpy().reshape(1))


def test_batched_encodes_equal_the_single_client_calls():
    codec = _codec()
    n, k, C = 65_537, 655, 3
    g = np.random.default_rng(3)
    xs_h = [(g.standard_normal(n) * 10.0 ** -c).astype(np.float32) for c in range(C)]
    xs = [torch.from_numpy(x).to(DEV) for x in xs_h]
    seeds, counters = [21, 22, 23], [5, 900, 77]
    outs = codec.topk_encode_batch(xs, k, with_tiles=True, order=MAG())
    pks = codec.stacked_encode_batch(xs, k, LEVELS, seeds=seeds, counters=counters, order=MAG())
    cnt = torch.zeros(C, dtype=torch.int64, device=DEV)
    pk2 = codec.stacked_encode_batch(xs, k, LEVELS, seeds=seeds, counters=counters, counts=cnt, order=MAG())
    pk3 = codec.stacked_encode_batch(xs, k, LEVELS, seeds=seeds, counter=9, order=MAG())  # (no counters: still a round)
    assert codec.topk_status(reset=True) == 0
    for c in range(C):
        exp_idx = mref.kept(xs_h[c], k, fast=True)[0]
        assert (xs_h[c][exp_idx] < 0).any()
        one = codec.topk_encode(xs[c], k, with_tiles=True, order=MAG())
        for a, b in zip(outs[c], one):
            assert torch.equal(a, b), c
        _check_plain(xs_h[c], k, *outs[c], exp_idx)
        single = codec.stacked_encode(xs[c], k, LEVELS, seed=seeds[c], counter=counters[c], order=MAG())
        _same_packet(pks[c], single, k)
        _same_packet(pk2[c], single, k)
        _same_packet(pk3[c], codec.stacked_encode(xs[c], k, LEVELS, seed=seeds[c], counter=9, order=MAG()), k)
        _check_stacked(xs_h[c], k, pks[c], exp_idx, seeds[c], counters[c])
        assert int(cnt[c]) == int((xs_h[c][exp_idx] != 0).sum())
    # the delta form of the round encode: client c's local model, one shared global model
    cuts = [0, n // 3 + 1, 2 * n // 3 + 2, n]
    glob = [torch.from_numpy((g.standard_normal(b - a) * 0.1).astype(np.float32)).to(DEV) for a, b in zip(cuts, cuts[1:])]
    locs = [[gl + x[a:b] for gl, a, b in zip(glob, cuts, cuts[1:])] for x in xs]
    pd = codec.stacked_encode_delta_batch(locs, glob, k, LEVELS, seeds=seeds, counters=counters, order=MAG())
    for c in range(C):
        _same_packet(pd[c], codec.stacked_encode_delta(locs[c], glob, k, LEVELS, seed=seeds[c], counter=counters[c],
                                                       order=MAG()), k)
        d = torch.cat([l - gl for l, gl in zip(locs[c], glob)]).cpu().numpy()
        _check_stacked(d, k, pd[c], mref.kept(d, k, fast=True)[0], seeds[c], counters[c], decode=False)


@pytest.mark.parametrize("n,k,whiches", [(70_001, 700, ("h", "l_over", "l_ctrl")), (70_001, 40, ("e", "e", "e")),
                                         (1_048_573, 10_485, ("l_over", "h")), (1_048_573, 40, ("e", "e"))])
def test_batched_select_paths_by_magnitude(n, k, whiches):
    """The sign-flipped batch cases, one per client: each client's own header shows the signed select's path on |x'|,
    and its outputs equal one single-client call."""
    codec = _codec()
    C = len(whiches)
    plan = sp.plan_of(n, k, C)
    cases = [sc.batch_cases(lambda n_, k_: sp.plan_of(n_, k_, C), n, k, w, salt=c) for c, w in enumerate(whiches)]
    assert not any(np.signbit(cs.x).any() for cs in cases)
    xfs = [mref.flip_signs(cs.x, FLIP + c) for c, cs in enumerate(cases)]
    exps = [ref.topk_kept(cs.x, k)[0] for cs in cases]
    xs = [torch.from_numpy(x).to(DEV) for x in xfs]
    seeds, counters = [11 + c for c in range(C)], [100 + 7 * c for c in range(C)]
    pks = codec.stacked_encode_batch(xs, k, LEVELS, seeds=seeds, counters=counters, order=MAG())
    stats = [codec.topk_select_stats(kind="topk_batch", client=c) for c in range(C)]
    assert codec.topk_status(reset=True) == 0
    for c in range(C):
        _check_stacked(xfs[c], k, pks[c], exps[c], seeds[c], counters[c])
        sp._check_path(cases[c], plan, stats[c])
        _same_packet(pks[c], codec.stacked_encode(xs[c], k, LEVELS, seed=seeds[c], counter=counters[c], order=MAG()), k)
    outs = codec.topk_encode_batch(xs, k, with_tiles=True, order=MAG())
    stats = [codec.topk_select_stats(kind="topk_batch", client=c) for c in range(C)]
    assert codec.topk_status(reset=True) == 0
    for c in range(C):
        _check_plain(xfs[c], k, *outs[c], exps[c])
        sp._check_path(cases[c], plan, stats[c])


def sparse_record_fields(d):
    """The bytes of a sparse record's fields (idx, val, tiles): a record's padding is never written."""
    views = _codec().sparse_wire_views(d.record, d.n, d.k)
    return np.concatenate([v.cpu().numpy().view(np.uint8) for v in views])


def test_a_signed_and_a_magnitude_message_never_share_a_launch(monkeypatch):
    """The order is part of a deferred batch's key: two stacked and two sparse messages of one round, one of each
    order, wait in four batches; every record equals the immediate encode and the model."""
    from fl_sim_amd import Compressor, compressed
    from tests.test_gpu_round import _record_fields

    shapes = [(300, 7), (41,), (9, 3, 3)]
    n = sum(int(np.prod(s)) for s in shapes)
    K, s = n // 50, 10
    g = torch.Generator().manual_seed(8)
    cached = [torch.randn(sh, generator=g) * 0.1 for sh in shapes]
    local = [t + torch.randn(t.shape, generator=g) * 1e-2 for t in cached]
    x = torch.cat([(a - b).reshape(-1) for a, b in zip(local, cached)]).numpy()
    lc, cc = [t.cuda() for t in local], [t.cuda() for t in cached]

    def comps(mag, stacked):
        tk = Compressor(rng="philox", seed=31)
        tk.makeTopKCompressor(K, n, magnitude=mag)
        if not stacked:
            return [tk]
        sd, nc = Compressor(rng="philox", seed=31), Compressor("norm")
        nc.makeIdenticalCompressor()
        sd.makeStandardDitheringFP32(s, nc)
        return [tk, sd]

    def run(defer):
        monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
        compressed._run_pending()
        compressed.deferred_stats(reset=True)
        compressed.deferred_sparse_stats(reset=True)
        ds = [compressed.compress_delta(lc, cc, comps(mag, st), sparse=not st) for st in (True, False)
              for mag in (False, True)]
        if defer:
            assert len({id(d._batch) for d in ds}) == 4 and len(compressed._PENDING) == 4
            assert ds[0]._batch.key[:-1] == ds[1]._batch.key[:-1] and ds[2]._batch.key[:-1] == ds[3]._batch.key[:-1]
        recs = [_record_fields(ds[0]), _record_fields(ds[1])] + [sparse_record_fields(d) for d in ds[2:]]
        flats = [d.flat().cpu().numpy() for d in ds]
        return recs, flats, compressed.deferred_stats(), compressed.deferred_sparse_stats()

    ra, fa, sa, spa = run(True)
    rb, fb, sb, spb = run(False)
    assert sa == {"batches": 2, "messages": 2} and spa == {"batches": 2, "messages": 2}
    assert sb == {"batches": 0, "messages": 0} and spb == {"batches": 0, "messages": 0}
    for a, b in zip(ra, rb):
        assert np.array_equal(a, b)
    u = lambda i: ref.philox_uniforms_at(i, 31, 0)  # noqa: E731
    assert gc.same_bits(fa[0], ref.stacked(x, K, s, u, fast=True)[0])
    assert gc.same_bits(fa[1], mref.stacked(x, K, s, u, fast=True)[0])
    assert gc.same_bits(fa[2], ref.topk(x, K)[0]) and gc.same_bits(fa[3], mref.topk(x, K))
    assert not np.array_equal(fa[2], fa[3]) and (fa[3] < 0).any()


# ------------------------------------------------------------------------------------------------ 7. float64
def test_float64_select_by_magnitude():
    codec = _codec()
    n = 1 << 20
    x0 = torch.zeros(n, dtype=torch.float64, device=DEV)
    x0[::7] = 1.0
    codec.topk_dense_f64(x0, 1000)
    sample = codec.topk_stats_f64(x0, 1000)["sample"]
    for name, (x, k, fb) in sorted(sc.f64_cases(n, sample).items()):
        xf = mref.flip_signs(x, FLIP)
        xd = torch.from_numpy(xf).to(DEV)
        got = codec.topk_dense_f64(xd, k, order=MAG())
        st = codec.topk_stats_f64(xd, k)
        assert g64.same_bits(got.cpu().numpy(), mref.topk(xf, k)), name
        keys = sc.order_key64(np.abs(xf))
        T = int(np.partition(keys, n - k)[n - k])
        assert st["err"] == 0 and st["T"] == T, (name, st)
        assert st["ties"] == int((keys == np.uint64(T)).sum()), (name, st)
        assert st["need"] == k - int((keys > np.uint64(T)).sum()), (name, st)
        if np.array_equal(np.abs(xf).view(np.uint64), x.view(np.uint64)):  # |x'| == x: the signed select's path on x
            assert st["fb"] == fb, (name, st)


@pytest.mark.parametrize("n", [2, 7, 1025, 65_537, 300_001])
def test_float64_compressor_by_magnitude(n):
    from fl_sim_amd import Compressor

    codec = _codec()
    g = np.random.default_rng(n)
    x = g.standard_normal(n) * 1e-3
    x[g.random(n) < 0.05] = -0.0
    for K in small_ks(n):
        c = Compressor()
        c.makeTopKCompressor(K, n, magnitude=True)
        want = mref.topk(x, K)
        assert g64.same_bits(c.compressVector(torch.from_numpy(x).to(DEV)).cpu().numpy(), want), (n, K)
        assert g64.same_bits(c.compressVector(x), want), (n, K)
        y = -np.abs(x) - 1e-9  # all negative: the signed rule keeps the smallest magnitudes
        assert g64.same_bits(codec.topk_dense_f64(torch.from_numpy(y).to(DEV), K, order="magnitude").cpu().numpy(),
                             mref.topk(y, K)), (n, K)
    q = Compressor()
    q.makeTopKCompressor(n, n, magnitude=True)
    assert g64.same_bits(q.compressVector(torch.from_numpy(x).to(DEV)).cpu().numpy(), x)
