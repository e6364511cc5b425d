"""GPU parity of the sparse-record entry points (wire.hip's fold kernel with the fp32 entry codec, sparse.hip's gather,
feedback.hip's K-entry residual): flc_fold_sparse_wires, flc_fedopt_fold_sparse_records, flc_fold_sparse_record_groups,
flc_avg_and_gradient_sparse_records, flc_sparse_gather and flc_ef_residual_sparse_round against the chains of decodes
and dense passes they replace, bit for bit — the tile edges and both sides of the fast path, chained launches, weights,
accumulators and kept values at their edge values.  Every record here is well formed (ascending unique indices, tile
pointers from flc_tile_index or from the encoder)."""

import ctypes

import numpy as np
import pytest
import torch

from tests import golden_cases as gc

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
TILE = 1024
SIZES = [4097, 70001, 1000003]
RECORDS = [1, 3, 10, 64, 65, 70]
MAXR = max(RECORDS)
WEIGHTS = [1.0, 0.37, -1.5, 3e-39, 0.0, -0.0]
VALUE_EDGES = [-0.0, 1e-40, -3e-41, float("inf"), float("-inf"), float("nan"), 0.0]


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1)


def _fill(rec, n, k, idx, val):
    """Write (idx, val) and the tile pointers of idx (flc_tile_index) into the record."""
    from fl_sim_amd import _lib, codec

    ri, rv, rt = codec.sparse_wire_views(rec, n, k)
    ri.copy_(idx.to(torch.int32))
    rv.copy_(val)
    _lib.call("flc_tile_index", ri.data_ptr(), k, n, rt.data_ptr(), codec._stream(rec.device))


def _values(k, g, r):
    """k kept values: ordinary ones with -0, denormals, +-inf and NaN among them (a k = 1 record takes them in turn)."""
    v = torch.randn(k, generator=g, device="cuda") * 1e-2
    if k == 1:
        if r % 2:
            v[0] = VALUE_EDGES[(r // 2) % len(VALUE_EDGES)]
        return v
    for i, e in enumerate(VALUE_EDGES):
        v[i::13][: max(1, k // 40)] = e
    return v


_BLOCKS: dict = {}


def _block(n, k):
    """[MAXR, stride] sparse records of (n, k), made once: every buffer 0xAB first; uniformly random index sets (k = 1
    and k = n // 100 leave empty tiles, k = n // 3 puts ~340 entries of every client in every tile); record 1 keeps the
    last element (the last, partial tile)."""
    from fl_sim_amd import codec

    key = (n, k)
    if key not in _BLOCKS:
        stride, _ = codec.sparse_wire_layout(n, k)
        wires = torch.full((MAXR, stride), 0xAB, dtype=torch.uint8, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(7 * n + k)
        for r in range(MAXR):
            idx = torch.randperm(n, generator=g, device="cuda")[:k]
            if r == 1:
                idx[0] = n - 1 if not bool((idx == n - 1).any()) else idx[0]
            idx = idx.sort().values
            _fill(wires[r], n, k, idx, _values(k, g, r))
        torch.cuda.synchronize()
        _BLOCKS[key] = wires
    return _BLOCKS[key]


def _decode(rec, n, k, weight=None, out=None):
    """flc_sparse_decode_tiled(scale 1, weight, accumulate = 1) into out; without a weight, the plain dense decode."""
    from fl_sim_amd import codec

    if weight is None:
        return codec.sparse_record_decode(rec, n, k)
    return codec.sparse_record_decode(rec, n, k, out=out, weight=float(weight), accumulate=True)


def _seed_acc(n, seed):
    """An accumulator with -0, +-inf, NaN and denormal lanes among ordinary values."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(n, generator=g, device="cuda") * 1e-2
    for i, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"), 0.0, 1e-40, -2e-42)):
        a[i::11][: max(1, n // 50)] = v
    return a


def _check_fold(wires, slots, ws, n, k, seed, label=""):
    from fl_sim_amd import codec

    for accumulate in (0, 1):
        start = _seed_acc(n, seed)
        got = start.clone() if accumulate else torch.full((n,), float("nan"), device="cuda")
        codec.fold_sparse_wires(wires, slots, ws, n, k, out=got, accumulate=bool(accumulate))
        want = start.clone() if accumulate else torch.zeros(n, device="cuda")
        for c, s in enumerate(slots):
            _decode(wires[s], n, k, weight=ws[c], out=want)
        torch.cuda.synchronize()
        assert gc.same_bits(_bits(got), _bits(want)), (label, accumulate)


@pytest.mark.parametrize("m", RECORDS)
@pytest.mark.parametrize("kk", ["one", "percent", "third"])
@pytest.mark.parametrize("n", SIZES)
def test_fold_sparse_wires_equals_the_decode_chain(n, kk, m):
    k = {"one": 1, "percent": n // 100, "third": n // 3}[kk]
    block = _block(n, k)
    slots = list(range(m))[::-1]  # (the fold order is the slots', not the block's)
    for shift in (0, 3):  # (two weight assignments: every record meets weights of both signs, zero and denormal)
        ws = [WEIGHTS[(c + shift) % len(WEIGHTS)] for c in range(m)]
        _check_fold(block, slots, ws, n, k, 5 * n + m, (kk, shift))


def test_a_fold_from_zero_resolves_negative_zeros_as_the_chain_does():
    """The -0 rule (skip_clients): a kept -0 times a positive weight leaves -0, which a later client without an entry
    there turns into +0 when its weight's sign bit is clear — and keeps when it is set."""
    n, k = 4097, 2
    from fl_sim_amd import codec

    stride, _ = codec.sparse_wire_layout(n, k)
    wires = torch.zeros(4, stride, dtype=torch.uint8, device="cuda")
    neg0 = torch.tensor([-0.0, -0.0], device="cuda")
    _fill(wires[0], n, k, torch.tensor([5, 2000]), neg0)
    _fill(wires[1], n, k, torch.tensor([7, 3000]), torch.tensor([1.0, -1e-30], device="cuda"))
    _fill(wires[2], n, k, torch.tensor([5, 4096]), torch.tensor([-1e-30, -0.0], device="cuda"))
    _fill(wires[3], n, k, torch.tensor([9, 10]), neg0)
    for ws in ([1.0, 1.0, 1e-30, 1.0], [1.0, -1.0, 1e-30, -2.0], [1.0, -0.0, 1e-30, -0.0], [-1.0, 0.5, -1e-30, 3e-39]):
        for slots in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0], [0]):
            _check_fold(wires, slots, ws[:len(slots)], n, k, 11, (ws, slots))
    # record 2 keeps -1e-30 at element 5: times 1e-30 it underflows to -0 (a kept -0 itself gives +0 from +0)
    got = codec.fold_sparse_wires(wires, [2], [1e-30], n, k)
    assert _bits(got).view(np.uint32)[5] == 0x80000000  # (the rule has something to resolve: a -0 does appear)
    got = codec.fold_sparse_wires(wires, [2, 1], [1e-30, 1.0], n, k)
    assert _bits(got).view(np.uint32)[5] == 0  # ... the next client's +w * +0 clears it
    got = codec.fold_sparse_wires(wires, [2, 1], [1e-30, -1.0], n, k)
    assert _bits(got).view(np.uint32)[5] == 0x80000000  # ... and a weight with its sign bit set keeps it


def _counted_block(n, k, counts, seed):
    """Records whose tile t holds counts[c][t] entries of client c (-1: whatever is left of k), indices ascending."""
    from fl_sim_amd import codec

    stride, _ = codec.sparse_wire_layout(n, k)
    R = len(counts)
    wires = torch.full((R, stride), 0xAB, dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    for c, per in enumerate(counts):
        per = list(per)
        rest = k - sum(v for v in per if v >= 0)
        per = [rest if v < 0 else v for v in per]
        assert sum(per) == k and all(0 <= v <= min(TILE, n - t * TILE) for t, v in enumerate(per)), per
        idx = torch.cat([t * TILE + torch.randperm(min(TILE, n - t * TILE), generator=g, device="cuda")[:v].sort().values
                         for t, v in enumerate(per)])
        _fill(wires[c], n, k, idx, _values(k, g, c))
    torch.cuda.synchronize()
    return wires


def test_both_sides_of_the_fast_path():
    """Tile 0 holds exactly 128 entries over all clients (the single load batch), tile 1 holds 129 (the per-client
    loop), tile 2 more than 128 from each single client, tile 3 none, and the last, partial tile one entry of one
    client."""
    n, k = 4097, 286
    counts = [[43, 43, -1, 0, 0], [43, 43, -1, 0, 1], [42, 43, -1, 0, 0]]
    wires = _counted_block(n, k, counts, 3)
    from fl_sim_amd import codec

    for c, per in enumerate(counts):
        tiles = codec.sparse_wire_views(wires[c], n, k)[2].cpu().numpy().astype(np.int64)
        got = np.diff(tiles).tolist()
        assert got[:2] == per[:2] and got[2] > 128 and got[3] == 0 and got[4] == per[4]
    totals = [sum(per[t] for per in counts) for t in (0, 1)]
    assert totals == [128, 129]
    for ws in ([0.37, -1.5, 1.0], [3e-39, 0.0, -0.0], [float("inf"), 1.0, float("nan")]):
        _check_fold(wires, [0, 1, 2], ws, n, k, 17, ws)
        _check_fold(wires, [2, 0, 1], ws, n, k, 18, ws)
    # one client alone: 43 entries (fast path) next to 200 (the loop)
    _check_fold(wires, [0], [0.37], n, k, 19)
    # 64 clients of one entry per tile: 64 entries a tile, then 65 records (a chain of two launches)
    n2, k2 = 3000, 3
    w2 = _counted_block(n2, k2, [[1, 1, 1]] * 65, 5)
    _check_fold(w2, list(range(64)), [WEIGHTS[c % 6] for c in range(64)], n2, k2, 23)
    _check_fold(w2, list(range(65)), [WEIGHTS[c % 6] for c in range(65)], n2, k2, 29)


def test_the_encoders_write_records():
    """flc_topk_encode_tiled and flc_topk_encode_batch with the three pointers inside a record: the record decodes to
    the top-k compressor's vector, the batch's rows equal the single encodes."""
    from fl_sim_amd import codec

    n, k, C = 70001, 700, 5
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn(n, generator=g, device="cuda") for _ in range(C)]
    stride, _ = codec.sparse_wire_layout(n, k)
    block = torch.full((C, stride), 0xAB, dtype=torch.uint8, device="cuda")
    codec.topk_encode_records(xs, k, block)
    for c in range(C):
        rec = torch.full((stride,), 0xCD, dtype=torch.uint8, device="cuda")
        codec.topk_encode_record(xs[c], k, rec)
        idx, val, tiles = codec.topk_encode(xs[c], k, with_tiles=True)
        want = codec.sparse_decode(idx, val, n, tiles=tiles)
        for r in (rec, block[c]):
            ri, rv, rt = codec.sparse_wire_views(r, n, k)
            assert torch.equal(ri, idx) and torch.equal(rt, tiles)
            assert gc.same_bits(_bits(rv), _bits(val))
            assert gc.same_bits(_bits(codec.sparse_record_decode(r, n, k)), _bits(want))


# ------------------------------------------------------------------------------------------------ the FedOpt fold
def _cut(flat, sizes):
    ts, off = [], 0
    for m in sizes:
        ts.append(flat[off:off + m])
        off += m
    return ts


def _splits(n):
    q = n // 17
    return {"one": [n], "unaligned": [3, 1021, 1, n - 1025], "seventeen": [q] * 16 + [n - 16 * q]}


def _state(n, sizes, seed, lead):
    """theta, delta, v cut from one buffer ``lead`` elements in (lead 1: no tensor is 16-B aligned but by accident)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    span = (n + lead + 3) // 4 * 4
    base = torch.randn(3 * span, generator=g, device="cuda") * 1e-2
    base[2 * span:].abs_().add_(1e-6)
    flats = [base[i * span + lead: i * span + lead + n] for i in range(3)]
    for i, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"))):
        flats[1][7 + i::13][: max(1, n // 100)] = v  # δ: -0, +-inf and NaN lanes
    return base, flats, [_cut(f, sizes) for f in flats]


def _dense_fedopt(recs, ws, n, k, sizes, state, beta0, opt, lr, beta2, tau, step):
    """Every record decoded densely, then flc_model_fold(init_mode 0) with the step (chained beyond 16 messages)."""
    from fl_sim_amd import codec

    theta, delta, v = state
    srcs = [_cut(_decode(r, n, k), sizes) for r in recs]
    codec.model_fold(delta, srcs, ws, 0, beta0, theta=theta if step else None,
                     v=v if (step and opt != "avg") else None, opt=opt, lr=lr, beta2=beta2, tau=tau)
    torch.cuda.synchronize()


def _fused_fedopt(recs, ws, n, k, sizes, state, beta0, opt, lr, beta2, tau, step):
    from fl_sim_amd import _lib

    theta, delta, v = state
    m, T = len(recs), len(sizes)
    ptr = lambda ts: (P * T)(*[t.data_ptr() for t in ts])  # noqa: E731
    _lib.call("flc_fedopt_fold_sparse_records", (P * m)(*[r.data_ptr() for r in recs]), (ctypes.c_float * m)(*ws), m, n,
              k, ptr(delta), ptr(theta) if step else None, ptr(v) if (step and opt != "avg") else None,
              (ctypes.c_int64 * T)(*sizes), T, beta0, _lib.FLC_OPT[opt], lr, beta2, tau, None)
    torch.cuda.synchronize()


def _assert_adaptive_tail(fa, fb):
    """(theta, delta, v) of the fused fold and of decode-then-model_fold, bit for bit: both sides inline the one
    opt_step (flc_device.hpp) under -ffp-contract=off, so no tolerance applies (the tolerance of
    test_gpu_round._check_adaptive_tail is for comparisons with torch only)."""
    for name, a, b in zip(("theta", "delta", "v"), fa, fb):
        assert gc.same_bits(_bits(a), _bits(b)), name


@pytest.mark.parametrize("n,kk,R", [(4097, "third", 3), (4097, "percent", 65), (70001, "percent", 10),
                                    (70001, "third", 3), (70001, "one", 10)])
def test_fedopt_fold_sparse_records_equals_decode_then_model_fold(n, kk, R):
    """avg, adagrad, yogi, adam and theta == NULL; one tensor, a split with unaligned starts and tensor borders inside a
    tile, a 17-tensor split (a chain of two tensor launches); 65 records (a chain of two record launches); δ with
    -0 / +-inf / NaN lanes; the weights' edge values."""
    k = {"one": 1, "percent": n // 100, "third": n // 3}[kk]
    block = _block(n, k)
    recs = [block[r] for r in range(R)]
    ws = [WEIGHTS[c % len(WEIGHTS)] for c in range(R)]
    for name, sizes in _splits(n).items():
        for opt, step in (("avg", True), ("adagrad", True), ("yogi", True), ("adam", True), ("avg", False)):
            beta0, lr, beta2, tau = (0.0, 1.0, 1.0, 1.0) if opt == "avg" else (0.9, 0.01, 0.99, 1e-3)
            lead = 0 if name == "one" else 1
            base_a, fa, a = _state(n, sizes, n + R, lead)
            base_b, fb, b = _state(n, sizes, n + R, lead)
            _fused_fedopt(recs, ws, n, k, sizes, a, beta0, opt, lr, beta2, tau, step)
            _dense_fedopt(recs, ws, n, k, sizes, b, beta0, opt, lr, beta2, tau, step)
            if opt == "avg":
                assert gc.same_bits(_bits(base_a), _bits(base_b)), (name, opt, step)
            else:
                _assert_adaptive_tail(fa, fb)


@pytest.mark.parametrize("ext", [True, False])
def test_fold_records_function_takes_sparse_records(ext, monkeypatch):
    """compressed.fold_records on sparse records — through the one-C-call extension entry
    (_flcfold.fold_sparse_records) and (``ext`` False: as when the extension is not built) through ctypes."""
    from fl_sim_amd import codec
    from fl_sim_amd.compressed import CompressedDelta, fold_records, record_round, sparse_round

    if ext:
        assert codec._pysrecs() is not None, "the _flcfold extension must be built"
    else:
        monkeypatch.setattr(codec, "_PYSRECS", [None])
    n, R = 4097, 10
    k = n // 3
    block = _block(n, k)
    ds = [CompressedDelta([torch.Size([n])], block.device, n, record=block[r], k=k, sparse=True) for r in range(R)]
    assert all(d.kind == "sparse" and d.levels == 0 and d.format is None for d in ds)
    assert ds[0].nbytes == codec.sparse_wire_layout(n, k)[0]
    msgs = [{"delta_parameters": d} for d in ds]
    assert sparse_round(msgs) == ds and record_round(msgs) == ds
    sizes = _splits(n)["unaligned"]
    ws = [0.1] * R
    base_a, _, a = _state(n, sizes, 3, 1)
    base_b, _, b = _state(n, sizes, 3, 1)
    assert fold_records(ds, ws, a[1], a[0], None, 0.0, "avg", 1.0, 0.0, 0.0)
    torch.cuda.synchronize()
    _dense_fedopt([block[r] for r in range(R)], ws, n, k, sizes, b, 0.0, "avg", 1.0, 0.0, 0.0, True)
    assert gc.same_bits(_bits(base_a), _bits(base_b))
    assert all(d._flat is None for d in ds)
    assert gc.same_bits(_bits(ds[2].flat()), _bits(_decode(block[2], n, k)))  # (the message decodes itself)


def test_fold_sparse_records_extension_checks():
    """_flcfold.fold_sparse_records: fold_dense_records' check order and exception texts."""
    from fl_sim_amd import _flcfold

    n, k = 4097, 40
    block = _block(n, k)
    d = torch.zeros(n, device="cuda")
    f = _flcfold.fold_sparse_records
    with pytest.raises(TypeError, match="fold_records takes sequences"):
        f(None, [1.0], n, k, [d], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="one weight per record"):
        f([block[0]], [1.0, 2.0], n, k, [d], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError, match="needs records and server tensors"):
        f([], [], n, k, [d], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError, match="contiguous fp32 HIP tensors"):
        f([block[0]], [1.0], n, k, [d.double()], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError, match="do not hold the records' element count"):
        f([block[0]], [1.0], n, k, [d[:-1]], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="bad wire shape"):
        f([block[0]], [1.0], n, 0, [d], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    with pytest.raises(TypeError, match="records must be 16-B aligned uint8 HIP tensors"):
        f([block[0][:256]], [1.0], n, k, [d], None, None, 0.0, 0, 1.0, 0.0, 0.0)
    torch.cuda.synchronize()
    assert bool((d == 0).all())  # (nothing launched)


# ------------------------------------------------------------------------------------------------ the grouped fold
@pytest.mark.parametrize("case", ["two", "three_one_empty", "seventeen"])
@pytest.mark.parametrize("n,kk", [(4097, "third"), (70001, "percent")])
def test_fold_sparse_record_groups_equals_weighted_sums(n, kk, case):
    """Per group flc_weighted_sum(init_mode 2) on the decoded vectors: two groups; three groups with one without a
    record (never read or written, its pointers NULL) and one of 66 records (a chain of launches); 17 groups (more than
    one launch's 16); the records interleaved; -0 / +-inf / NaN / denormal accumulators; the weights' edge values."""
    from fl_sim_amd import _lib, codec

    k = {"percent": n // 100, "third": n // 3}[kk]
    block = _block(n, k)
    if case == "two":
        rec_ids, gof = list(range(7)), [0, 1, 0, 1, 1, 0, 1]
    elif case == "three_one_empty":
        rec_ids = list(range(66)) + [5, 9, 11, 2]
        gof = [2] * 66 + [0, 0, 0, 0]
    else:
        rec_ids = list(range(40))
        gof = [c % 17 for c in range(40)]
    if case != "two":
        order = np.random.RandomState(n).permutation(len(rec_ids))
        rec_ids, gof = [rec_ids[i] for i in order], [gof[i] for i in order]
    G = max(gof) + 1
    ws = [WEIGHTS[c % len(WEIGHTS)] for c in range(len(rec_ids))]
    sizes = _splits(n)["unaligned"]
    T = len(sizes)

    def dests():
        base = torch.cat([_seed_acc(n + 3, 40 + g) for g in range(G)])
        return base, [_cut(base[g * (n + 3) + 1: g * (n + 3) + 1 + n], sizes) for g in range(G)]

    base_a, a = dests()
    base_b, b = dests()
    m = len(rec_ids)
    idle = [g for g in range(G) if g not in gof]
    assert (case == "three_one_empty") == bool(idle)
    dptr = [0 if g in idle else t.data_ptr() for g in range(G) for t in a[g]]  # (an idle group's pointers may be NULL)
    _lib.call("flc_fold_sparse_record_groups", (P * m)(*[block[r].data_ptr() for r in rec_ids]),
              (ctypes.c_float * m)(*ws), (ctypes.c_int32 * m)(*gof), m, n, k, (P * (G * T))(*dptr), G,
              (ctypes.c_int64 * T)(*sizes), T, None)
    dec = {r: _cut(_decode(block[r], n, k), sizes) for r in set(rec_ids)}
    for g in range(G):
        mem = [c for c in range(m) if gof[c] == g]
        for j, t in enumerate(b[g]):
            if mem:
                codec.weighted_sum(t, [dec[rec_ids[c]][j] for c in mem], [ws[c] for c in mem], init_mode=2)
    torch.cuda.synchronize()
    assert gc.same_bits(_bits(base_a), _bits(base_b))
    fresh, _ = dests()
    for g in idle:  # untouched, bit for bit
        lo, hi = g * (n + 3), (g + 1) * (n + 3)
        assert gc.same_bits(_bits(base_a[lo:hi]), _bits(fresh[lo:hi]))


# --------------------------------------------------------------------------------- the variance-reduced servers' pass
@pytest.mark.parametrize("n,kk,m", [(4097, "third", 3), (4097, "percent", 17), (4097, "percent", 65),
                                    (70001, "percent", 10)])
def test_avg_and_gradient_sparse_records_equals_decode_then_avg_and_gradients(n, kk, m):
    """The records decoded densely, then flc_avg_and_gradients: 17 messages chain the parameter sources, 65 the records;
    unaligned tensors; the weights' edge values; and the gradients-only form (param_srcs NULL: params untouched)."""
    from fl_sim_amd import _lib

    k = {"percent": n // 100, "third": n // 3}[kk]
    block = _block(n, k)
    recs = [block[r] for r in range(m)]
    wg = [WEIGHTS[c % len(WEIGHTS)] for c in range(m)]
    wp = [0.9 / m] * m
    sizes = _splits(n)["unaligned"]
    T = len(sizes)
    g = torch.Generator(device="cuda").manual_seed(n + m)
    psrc_flat = [torch.randn(n + 1, generator=g, device="cuda")[1:] for _ in range(m)]
    psrc = [_cut(f, sizes) for f in psrc_flat]
    dec = [_cut(_decode(r, n, k), sizes) for r in recs]
    ptr = lambda ts: (P * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    fl = lambda v: (ctypes.c_float * len(v))(*v)  # noqa: E731
    sz = (ctypes.c_int64 * T)(*sizes)

    def state():
        base = torch.cat([_seed_acc(n + 3, 7), torch.full((n + 3,), float("nan"), device="cuda")])
        return base, _cut(base[1:1 + n], sizes), _cut(base[n + 4:2 * n + 4], sizes)

    for with_params in (True, False):
        base_a, pa, ga = state()
        base_b, pb, gb = state()
        _lib.call("flc_avg_and_gradient_sparse_records", ptr(pa) if with_params else None, ptr(ga),
                  ptr([t for r in psrc for t in r]) if with_params else None, ptr(recs),
                  fl(wp) if with_params else None, fl(wg), m, n, k, sz, T, 0.1, None)
        _lib.call("flc_avg_and_gradients", ptr(pb), ptr(gb), ptr([t for r in psrc for t in r]),
                  ptr([t for r in dec for t in r]), fl(wp), fl(wg), m, sz, T, 0.1, None)
        torch.cuda.synchronize()
        if with_params:
            assert gc.same_bits(_bits(base_a), _bits(base_b))
        else:
            fresh, _, _ = state()
            assert gc.same_bits(_bits(base_a[:n + 3]), _bits(fresh[:n + 3]))  # the parameters: untouched
            assert gc.same_bits(_bits(base_a[n + 3:]), _bits(base_b[n + 3:]))


# ------------------------------------------------------------------------------------------- rand-k's values
def test_sparse_gather_equals_what_randk_apply_scatters():
    from fl_sim_amd import _lib, codec

    n, k = 70001, 700
    g = torch.Generator(device="cuda").manual_seed(9)
    x = torch.randn(n, generator=g, device="cuda")
    idx = torch.randperm(n, generator=g, device="cuda")[:k].sort().values.to(torch.int32)
    for i, v in enumerate((float("nan"), -0.0, 1e-40, float("inf"), 0.0)):
        x[idx[i::5][:20].long()] = v  # kept elements that are NaN, -0, denormal, inf and +0
    scale = float(np.float32(n / k))
    want = codec.randk_apply(x, idx, scale)[idx.long()]
    got = codec.sparse_gather(x, idx, scale)
    torch.cuda.synchronize()
    assert gc.same_bits(_bits(got), _bits(want))
    assert np.isnan(_bits(got)).any() and (_bits(got).view(np.uint32) == 0x80000000).any()
    # as a record's val field: the record decodes to the rand-k compressor's vector
    stride, _ = codec.sparse_wire_layout(n, k)
    rec = torch.full((stride,), 0xAB, dtype=torch.uint8, device="cuda")
    ri, rv, rt = codec.sparse_wire_views(rec, n, k)
    ri.copy_(idx)
    _lib.call("flc_tile_index", ri.data_ptr(), k, n, rt.data_ptr(), codec._stream(rec.device))
    codec.sparse_gather(x, ri, scale, out=rv)
    assert gc.same_bits(_bits(codec.sparse_record_decode(rec, n, k)), _bits(codec.randk_apply(x, idx, scale)))
    # an index outside [0, n) writes +0 (x lies inside a larger buffer here)
    base = torch.full((n + 8,), 7.0, device="cuda")
    bad = torch.tensor([0, n - 1, n, -1, 2 ** 31 - 1, 5], dtype=torch.int32, device="cuda")
    out = torch.full((6,), float("nan"), device="cuda")
    _lib.call("flc_sparse_gather", base.data_ptr() + 16, n, bad.data_ptr(), 6, 2.0, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert _bits(out).view(np.uint32).tolist() == _bits(torch.tensor([14.0, 14.0, 0.0, 0.0, 0.0, 14.0])).view(
        np.uint32).tolist()


# ------------------------------------------------------------------------------------------- the residual
@pytest.mark.parametrize("C", [1, 33])
@pytest.mark.parametrize("n,kk", [(70001, "percent"), (4097, "third"), (4097, "one")])
def test_ef_residual_sparse_round_equals_decode_then_dense_residual(n, kk, C):
    """es[c] -= decode(record c): against flc_sparse_decode_tiled into a zeroed vector + flc_ef_residual_dense; 33
    clients chain two launches; memories with -0, +-inf, NaN and denormal lanes, which an untouched element keeps."""
    from fl_sim_amd import codec

    k = {"one": 1, "percent": n // 100, "third": n // 3}[kk]
    block = _block(n, k)
    recs = [block[c] for c in range(C)]
    got = [_seed_acc(n, 100 + c) for c in range(C)]
    want = [e.clone() for e in got]
    codec.ef_residual_sparse_round(recs, got, n, k)
    for c in range(C):
        codec.ef_residual_dense(want[c], _decode(recs[c], n, k))
    torch.cuda.synchronize()
    for c in range(C):
        a, b = _bits(got[c]), _bits(want[c])
        assert gc.same_bits(a, b), c
        start = _bits(_seed_acc(n, 100 + c))
        idx = codec.sparse_wire_views(recs[c], n, k)[0].cpu().numpy()
        rest = np.ones(n, dtype=bool)
        rest[idx] = False
        assert gc.same_bits(a[rest], start[rest])  # untouched elements keep their bits
        assert (a[rest].view(np.uint32) == 0x80000000).any()  # ... a -0 included


def test_folds_reject_bad_arguments_on_the_device():
    from fl_sim_amd import _lib, codec

    n, k = 5000, 50
    stride, _ = codec.sparse_wire_layout(n, k)
    rec = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    d = torch.ones(n, device="cuda")
    one = (ctypes.c_float * 1)(1.0)
    with pytest.raises(_lib.FlcError, match="hold"):
        _lib.call("flc_fedopt_fold_sparse_records", (P * 1)(rec.data_ptr()), one, 1, n, k, (P * 1)(d.data_ptr()), None,
                  None, (ctypes.c_int64 * 1)(n - 1), 1, 0.0, 0, 1.0, 0.0, 0.0, None)
    with pytest.raises(_lib.FlcError, match="aligned"):
        _lib.call("flc_fedopt_fold_sparse_records", (P * 1)(rec.data_ptr() + 4), one, 1, n, k, (P * 1)(d.data_ptr()),
                  None, None, (ctypes.c_int64 * 1)(n), 1, 0.0, 0, 1.0, 0.0, 0.0, None)
    with pytest.raises(_lib.FlcError, match="outside"):
        codec.fold_sparse_wires(rec.reshape(1, -1), [0], [1.0], n, n + 1, out=d, accumulate=True)
    torch.cuda.synchronize()
    assert bool((d == 1).all())  # (nothing launched)
