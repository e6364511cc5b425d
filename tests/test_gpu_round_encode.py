"""GPU parity of the round encode (flc_stacked_encode_round / flc_stacked_encode_delta_round): a round's messages in
one batched launch, each with its own Philox (seed, counter), the dithering stage's send counts made by the select
itself.  Packets against one ``codec.stacked_encode`` per client, field by field; counts against
``(~(x_c[idx_c] == 0)).sum()`` — mixed counters (one past 2^32), counts that are not k (few nonzeros, all zeros, a
NaN), the take-all, chunked, HBM-overflow (g-mode) and range re-read (x-mode) paths, the delta form, graph capture,
the torch op, and the deferred compressed round with sampled clients (one batched encode per round)."""

import ctypes

import numpy as np
import pytest
import torch

from fl_sim_amd import _lib, codec

pytestmark = pytest.mark.gpu


def _x(n, seed, kind="randn"):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, generator=g, device="cuda") * 1e-3
    if kind == "zeros":
        x[torch.rand(n, generator=g, device="cuda") < 0.3] = 0.0
    elif kind == "ties":  # few distinct values: the k-th value is tied many times
        x = torch.round(x * 4e3) / 4e3
    elif kind == "skew":
        x[: min(n, 5000)] += 1.0
    return x


def _same(a: codec.StackedPacket, b: codec.StackedPacket, what=""):
    assert torch.equal(a.idx, b.idx), f"idx differ {what}"
    assert torch.equal(a.codes[: a.idx.numel()], b.codes[: b.idx.numel()]), f"codes differ {what}"
    assert torch.equal(a.norm.view(torch.int32), b.norm.view(torch.int32)), f"norm differs {what}"  # (NaN: bits)
    if a.tiles is not None and b.tiles is not None:
        assert torch.equal(a.tiles, b.tiles), f"tiles differ {what}"


def _count(x, idx):
    return int((~(x[idx.long()] == 0)).sum().item())


def _counters(C):
    """All distinct but one equal pair (clients 0 and 1 when C > 2), one of them past 2^32."""
    ctrs = [5 + 3 * c for c in range(C)]
    if C > 2:
        ctrs[1] = ctrs[0]
    ctrs[-1] = (1 << 32) + 7
    return ctrs


def _check_round(xs, k, seeds, ctrs, what="", every=1):
    C = len(xs)
    counts = torch.full((C,), -1, dtype=torch.int64, device="cuda")
    pks = codec.stacked_encode_batch(xs, k, 127, seeds=seeds, counters=ctrs, counts=counts)
    got = counts.tolist()
    for c in range(C):
        if c % every == 0 or c == C - 1:
            _same(pks[c], codec.stacked_encode(xs[c], k, 127, seed=seeds[c], counter=ctrs[c]), f"{what} client {c}")
        assert got[c] == _count(xs[c], pks[c].idx), f"{what} count of client {c}"
    return pks, got


# ------------------------------------------------------------------------------------------------ 1. mixed counters
@pytest.mark.parametrize("n,k,C", [(70_001, 700, 3), (1_000_003, 10_000, 8), (250_000, 2_500, 17)])
def test_round_mixed_counters_equal_single_encodes(n, k, C):
    kinds = ["randn", "zeros", "ties", "skew"]
    xs = [_x(n, 100 + c, kinds[c % 4]) for c in range(C)]
    seeds = [7 + 3 * c for c in range(C)]
    ctrs = _counters(C)
    assert len(set(ctrs)) == C - 1 and max(ctrs) >= 1 << 32
    _check_round(xs, k, seeds, ctrs)
    # all counters equal: the batch entry's result, and the same counts
    counts = torch.full((C,), -1, dtype=torch.int64, device="cuda")
    a = codec.stacked_encode_batch(xs, k, 127, seeds=seeds, counters=[11] * C, counts=counts)
    b = codec.stacked_encode_batch(xs, k, 127, seeds=seeds, counter=11)
    for c in range(C):
        _same(a[c], b[c], f"equal counters, client {c}")
        assert int(counts[c]) == _count(xs[c], b[c].idx)
    assert codec.topk_status() == 0


# ------------------------------------------------------------------------------------- 2. counts that are not k
def test_round_counts_few_nonzeros_zeros_and_nan():
    n, k = 70_001, 700
    few = torch.zeros(n, device="cuda")
    few[torch.randperm(n, generator=torch.Generator().manual_seed(3))[:300].cuda()] = _x(300, 21).abs() + 1e-3  # (positive: the select keeps the largest values, so all 300)
    assert int((few != 0).sum()) == 300
    zero = torch.zeros(n, device="cuda")
    nan = _x(n, 22)
    nan[12_345] = float("nan")
    plain = _x(n, 23)
    xs = [few, zero, nan, plain]
    pks, got = _check_round(xs, k, [1, 2, 3, 4], [9, 9, 1 << 33, 2])
    assert got == [300, 0, k, k]  # (kept zeros are not sent; the all-zero client: norm 0; the NaN is kept and counted)
    assert float(pks[1].norm) == 0.0
    assert 12_345 in pks[2].idx.tolist()
    assert codec.topk_status() == 0


# --------------------------------------------------------------------------------------------------------- 3. paths
def test_round_take_all_and_repeat_calls():
    # k close to n: the sample admits everything (no sample launch: the counts are zeroed with the headers); then the
    # same workspace with other shapes, back to back
    for (n, k, C) in [(1_000, 999, 4), (300_001, 3_000, 6), (2_048, 1, 5), (70_001, 700, 2)]:
        xs = [_x(n, 7 * c + n % 97, "zeros" if c == 1 else "randn") for c in range(C)]
        _check_round(xs, k, list(range(C)), [n % 13 + c for c in range(C)], f"n={n}")
        assert codec.topk_status() == 0


def test_round_more_clients_than_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    C, n, k = cus + 44, 5_000, 50
    xs = [_x(n, c, "zeros" if c % 3 == 0 else "randn") for c in range(C)]
    _check_round(xs, k, list(range(C)), [c % 5 for c in range(C)], "chunked", every=7)  # (every count is checked)
    assert codec.topk_status() == 0


def test_round_g_mode():
    n, k = 32_000_000, 4_800_000  # (15 % kept, ~40 K candidates per block: past a block's LDS, in the HBM overflow)
    xs = [_x(n, 500), _x(n, 501, "zeros")]
    _check_round(xs, k, [3, 4], [6, 1 << 32], "g-mode")
    assert codec.topk_status() == 0


def test_round_x_mode():
    n, k = 2_000_000, 20_000  # (one block's range holds all the large values: the range re-read)
    xs = [_x(n, 510), _x(n, 511), _x(n, 512, "zeros")]
    xs[1][:30_000] += 1.0
    _check_round(xs, k, [1, 2, 3], [8, 9, 8], "x-mode")
    assert codec.topk_status() == 0


# --------------------------------------------------------------------------------------------------- 4. delta form
def test_delta_round_equals_single_delta_encodes():
    g = torch.Generator(device="cuda").manual_seed(700)
    shapes = [(16, 1, 5, 5), (16,), (32, 16, 5, 5), (32,), (2048, 123), (123,), (62, 2048), (62,)]
    glob = [torch.randn(*s, generator=g, device="cuda") for s in shapes]
    C = 6
    locs = [[t + torch.randn(*t.shape, generator=g, device="cuda") * 1e-3 for t in glob] for _ in range(C)]
    locs[2][4][:1500] = glob[4][:1500]  # (zero deltas among the kept candidates' neighbours)
    n = sum(t.numel() for t in glob)
    k = n // 100
    seeds, ctrs = [10 + c for c in range(C)], _counters(C)
    counts = torch.full((C,), -1, dtype=torch.int64, device="cuda")
    pks = codec.stacked_encode_delta_batch(locs, glob, k, 127, seeds=seeds, counters=ctrs, counts=counts)
    P = ctypes.c_void_p * len(glob)
    sizes = (ctypes.c_int64 * len(glob))(*[t.numel() for t in glob])
    for c in range(C):
        ref = codec.stacked_encode_delta(locs[c], glob, k, 127, seed=seeds[c], counter=ctrs[c])
        _same(pks[c], ref, f"client {c}")
        want = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        _lib.call("flc_delta_count_nonzero_at", P(*[t.data_ptr() for t in locs[c]]), P(*[t.data_ptr() for t in glob]),
                  sizes, len(glob), ref.idx.data_ptr(), k, want.data_ptr(), codec._stream(want.device))
        assert int(counts[c]) == int(want), f"count of client {c}"
    assert codec.topk_status() == 0


# ------------------------------------------------------------------------------------------------------ 5. capture
def test_round_capture_replays_equal_the_eager_call():
    n, k, C = 70_001, 700, 3
    xs = [_x(n, 900 + c, "zeros" if c == 1 else "randn") for c in range(C)]
    seeds, ctrs = [4, 5, 6], [2, 2, (1 << 32) + 1]
    counts = torch.full((C,), -1, dtype=torch.int64, device="cuda")
    fn = lambda cn: codec.stacked_encode_batch(xs, k, 127, seeds=seeds, counters=ctrs, counts=cn)  # noqa: E731
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm: the stream's workspace allocated outside the capture
        fn(counts)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pks = fn(counts)
    for r in range(2):
        for c, x in enumerate(xs):
            x.copy_(_x(n, 950 + 10 * r + c, "zeros" if c == r else "randn"))
        counts.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        ecounts = torch.full((C,), -1, dtype=torch.int64, device="cuda")
        eager = fn(ecounts)
        torch.cuda.synchronize()
        for c in range(C):
            _same(pks[c], eager[c], f"replay {r} client {c}")
        assert torch.equal(counts, ecounts) and counts.tolist() == [_count(xs[c], eager[c].idx) for c in range(C)]
    assert codec.topk_status(torch.device("cuda", 0)) == 0


# ----------------------------------------------------------------------------------------------------- 6. torch op
def test_round_wire_torch_op():
    import fl_sim_amd

    fl_sim_amd.load_torch_ops()
    ops = torch.ops.flcodec
    assert str(ops.stacked_encode_round_wire.default._schema) == (
        "flcodec::stacked_encode_round_wire(Tensor[] xs, int k, int levels, int[] seeds, int[] counters) -> "
        "(Tensor records, Tensor counts)")
    m_recs, m_counts = ops.stacked_encode_round_wire([torch.empty(5000, device="meta")] * 4, 50, 127, [1, 2, 3, 4],
                                                     [1, 2, 3, 4])
    n, k, C = 50_000, 500, 5
    assert m_recs.shape == (4, codec.stacked_wire_layout(5000, 50)[0]) and m_recs.dtype == torch.uint8
    assert m_counts.shape == (4,) and m_counts.dtype == torch.int64
    xs = [_x(n, 40 + c, "zeros" if c == 2 else "randn") for c in range(C)]
    seeds, ctrs = [9 + c for c in range(C)], _counters(C)
    recs, counts = ops.stacked_encode_round_wire(xs, k, 127, seeds, ctrs)
    want = torch.full((C,), -1, dtype=torch.int64, device="cuda")
    pks = codec.stacked_encode_batch(xs, k, 127, seeds=seeds, counters=ctrs, counts=want)
    assert recs.shape == (C, codec.stacked_wire_layout(n, k)[0]) and torch.equal(counts, want)
    for c in range(C):
        _same(codec.wire_packet(recs[c], n, k), pks[c], f"record {c}")
        assert int(counts[c]) == _count(xs[c], pks[c].idx)


# ---------------------------------------------------------------------------------------------------- 7. call site
def test_sampled_round_is_one_batched_encode_per_round(monkeypatch):
    """Rounds of sampled clients, each client with its own compressors (so from the second round on the sampled
    clients' Philox counters differ): deferred and immediate encodes give equal records, statistics and counters, and
    the deferred round runs one batched encode."""
    from fl_sim_amd import compressed
    from tests.test_gpu_round import _record_fields, make_compressors

    g = torch.Generator().manual_seed(13)
    shapes = [(16, 1, 5, 5), (16,), (256, 37), (10,)]
    glob = [torch.randn(sh, generator=g).cuda() for sh in shapes]
    D = sum(t.numel() for t in glob)
    n_clients, n_rounds, per_round = 12, 5, 4
    locs = [[[t + torch.randn(t.shape, generator=g).cuda() * 1e-2 for t in glob] for _ in range(per_round)]
            for _ in range(n_rounds)]

    def run(defer):
        monkeypatch.setattr(compressed, "DEFER_ENCODE", defer)
        comps = [make_compressors("stacked10", D, rng="philox", seed=100 + i) for i in range(n_clients)]
        rs = np.random.RandomState(0)
        recs, ctrs, batches = [], [], []
        for r in range(n_rounds):
            chosen = rs.choice(n_clients, per_round, replace=False)
            ctrs.append([comps[i][1].philox.counter for i in chosen])
            before = compressed.deferred_stats()
            ds = [compressed.compress_delta(locs[r][j], glob, comps[i]) for j, i in enumerate(chosen)]
            recs += [_record_fields(d) for d in ds]
            after = compressed.deferred_stats()
            batches.append((after["batches"] - before["batches"], after["messages"] - before["messages"]))
        stats = [(c[0].total_input_components, c[1].total_input_components, c[1].really_need_to_send_components,
                  c[1].last_need_to_send_advance, c[1].philox.counter) for c in comps]
        return recs, stats, ctrs, batches

    ra, sa, ca, ba = run(True)
    assert not compressed._PENDING
    rb, sb, cb, bb = run(False)
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert np.array_equal(x, y), i
    assert sa == sb and ca == cb
    for r in range(1, n_rounds):
        assert len(set(ca[r])) > 1, f"round {r}: the sampled clients' counters do not differ"
    assert ba == [(1, per_round)] * n_rounds  # one batched encode per round, all four messages in it
    assert bb == [(0, 0)] * n_rounds
    st = compressed.deferred_stats(reset=True)
    assert st["batches"] >= n_rounds and compressed.deferred_stats() == {"batches": 0, "messages": 0}
