"""flc_quant_encode_round against one flc_quant_encode_auto call with rows = 1 per message, bit for bit: the norm, every
code byte and the count, over the sizes at which either call changes its path (the group of 8, the 2048-element block
span, the 4096-element norm chunk, the 16384-element one-launch threshold of the per-message call, each +-1), every
code width and both quantizers, p = inf and 2, 1 to 65 messages (65: a chain of two tables), distinct and equal
(seed, counter) across messages; a p = 2 norm past kNormMaxParts chunks; zero, NaN, +-inf and -0 messages between
ordinary ones; counts == NULL; the records decoded against the CPU oracle; graph capture."""

import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STD, NATD = 0, 1
INF, L2 = 0, 2
FORMATS = [(STD, 127, 8), (STD, 7, 4), (STD, 1, 2), (NATD, 127, 8), (NATD, 7, 4), (NATD, 1, 2)]
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4095, 4097, 16383, 16385]
MSGS = [1, 2, 10, 64, 65]
PAD = 0xA5  # what the code buffers hold before a call: bytes past ceil(n * bits / 8) must keep it
GARBAGE = -0x0123456789ABCDEF  # what the count slots hold before the round call

P = ctypes.c_void_p
U64 = ctypes.c_uint64
vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731


def _L():
    from fl_sim_amd import _lib

    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """Per-message output buffers: [C, row] code bytes (16-B rows, >= 16 B of padding), norms and counts."""

    def __init__(self, C, n, bits, dev="cuda"):
        self.cb = (n * bits + 7) // 8
        self.row = (self.cb + 16 + 15) // 16 * 16
        self.codes = torch.full((C, self.row), PAD, dtype=torch.uint8, device=dev)
        self.norms = torch.full((C,), -7.0, dtype=torch.float32, device=dev)
        self.counts = torch.full((C,), GARBAGE, dtype=torch.int64, device=dev)

    def same(self, other, C):
        return (torch.equal(self.codes[:C], other.codes[:C])
                and torch.equal(self.norms[:C].view(torch.int32), other.norms[:C].view(torch.int32))
                and torch.equal(self.counts[:C], other.counts[:C]))


def _auto_each(X, n, fmt, pk, seeds, ctrs, out: Out, counts=True):
    """The reference: one flc_quant_encode_auto call with rows = 1 per message."""
    L = _L()
    kind, levels, bits = fmt
    ws = torch.zeros(L.size("flc_quant_workspace_size", 1, n), dtype=torch.uint8, device=X.device)
    st = _stream()
    for c in range(len(seeds)):
        L.call("flc_quant_encode_auto", X[c].data_ptr(), 1, n, kind, levels, bits, pk, seeds[c], ctrs[c],
               out.codes[c].data_ptr(), out.norms[c:c + 1].data_ptr(),
               out.counts[c:c + 1].data_ptr() if counts else None, None, ws.data_ptr(), ws.numel(), st)
    err = torch.zeros(1, dtype=torch.int64, device=X.device)
    L.call("flc_quant_status", ws.data_ptr(), err.data_ptr(), 1, st)
    assert int(err.item()) == 0


def _round(X, C, n, fmt, pk, seeds, ctrs, out: Out, counts=True, ws=None):
    L = _L()
    kind, levels, bits = fmt
    if ws is None:
        ws = torch.empty(L.size("flc_quant_encode_round_workspace_size", n, C), dtype=torch.uint8, device=X.device)
    L.call("flc_quant_encode_round", vp((P * C)(*[X[c].data_ptr() for c in range(C)])), C, n, kind, levels, bits, pk,
           vp((U64 * C)(*seeds[:C])), vp((U64 * C)(*ctrs[:C])),
           vp((P * C)(*[out.codes[c].data_ptr() for c in range(C)])),
           vp((P * C)(*[out.norms[c:c + 1].data_ptr() for c in range(C)])),
           vp((P * C)(*[out.counts[c:c + 1].data_ptr() for c in range(C)])) if counts else None,
           ws.data_ptr(), ws.numel(), _stream())
    return ws


def _inputs(C, n, seed):
    """[C, n rounded up to 4] fp32 (16-B rows): model-delta-sized values with zeros and -0 sprinkled in."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(C, (n + 3) // 4 * 4, generator=g, device="cuda") * 1e-3
    m = torch.rand(X.shape, generator=g, device="cuda")
    X[m < 0.05] = 0.0
    X[(m >= 0.05) & (m < 0.07)] = -0.0
    X[:, n:] = float("nan")  # (past the message: never read)
    return X


@pytest.mark.parametrize("pk", [INF, L2], ids=["inf", "p2"])
@pytest.mark.parametrize("n", SIZES)
def test_round_equals_per_message_auto(n, pk):
    Cmax = max(MSGS)
    X = _inputs(Cmax, n, 1000 + n)
    distinct = ([0x9E3779B97F4A7C15 * (c + 1) % (1 << 64) for c in range(Cmax)], [3 * c + 1 for c in range(Cmax)])
    equal = ([77] * Cmax, [5] * Cmax)
    for fmt in FORMATS:
        for seeds, ctrs in (distinct, equal):
            want = Out(Cmax, n, fmt[2])
            _auto_each(X, n, fmt, pk, seeds, ctrs, want)
            assert bool((want.counts >= 0).all()) and bool((want.counts <= n).all())
            for C in MSGS:
                got = Out(Cmax, n, fmt[2])
                _round(X, C, n, fmt, pk, seeds, ctrs, got)
                assert got.same(want, C), (n, pk, fmt, C, seeds is equal[0])
                # messages past C untouched, and nothing written past a message's code bytes
                assert bool((got.codes[C:] == PAD).all()) and bool((got.codes[:, got.cb:] == PAD).all())
                assert bool((got.counts[C:] == GARBAGE).all())


def test_p2_norm_past_the_partial_limit():
    """n = 4,194,305: more than kNormMaxParts chunks of kNormChunk elements, so the chunk grows (4-aligned) — the fp64
    sum keeps the per-message call's partition and its bits."""
    n, C, fmt = 4_194_305, 2, (STD, 127, 8)
    X = _inputs(C, n, 5)
    seeds, ctrs = [11, 12], [1, 2]
    want, got = Out(C, n, 8), Out(C, n, 8)
    _auto_each(X, n, fmt, L2, seeds, ctrs, want)
    _round(X, C, n, fmt, L2, seeds, ctrs, got)
    assert got.same(want, C)
    ref = torch.sqrt((X[:, :n].double() ** 2).sum(1)).float()
    assert torch.allclose(got.norms, ref, rtol=1e-6)  # (the reference itself is the bit-level check above)


@pytest.mark.parametrize("pk", [INF, L2], ids=["inf", "p2"])
@pytest.mark.parametrize("fmt", [(STD, 127, 8), (STD, 7, 4), (NATD, 7, 4), (NATD, 1, 2)], ids=str)
def test_edge_messages_between_ordinary_ones(fmt, pk):
    n, C = 4097, 7
    X = _inputs(C, n, 9)
    X[1, :n] = 0.0  # norm 0
    X[3, 1234] = float("nan")  # norm NaN
    X[5, 17] = float("inf")  # norm inf, with -inf and -0 among the elements
    X[5, 2048] = float("-inf")
    X[5, 100:200] = -0.0
    seeds, ctrs = list(range(21, 21 + C)), list(range(C))
    want, got = Out(C, n, fmt[2]), Out(C, n, fmt[2])
    _auto_each(X, n, fmt, pk, seeds, ctrs, want)
    _round(X, C, n, fmt, pk, seeds, ctrs, got)
    assert got.same(want, C)
    norms = got.norms.cpu().numpy()
    assert norms[1] == 0.0 and math.isnan(norms[3]) and math.isinf(norms[5])
    assert all(np.isfinite(norms[c]) and norms[c] > 0 for c in (0, 2, 4, 6))  # (a neighbour's NaN did not reach them)
    assert int(got.counts[1]) == 0
    # the ordinary messages alone, each at the same (seed, counter): their records do not depend on their neighbours
    for c in (0, 2, 4, 6):
        alone = Out(1, n, fmt[2])
        _round(X[c:c + 1], 1, n, fmt, pk, seeds[c:c + 1], ctrs[c:c + 1], alone)
        assert torch.equal(alone.codes[0], got.codes[c]) and torch.equal(alone.norms[0], got.norms[c])
        assert torch.equal(alone.counts[0], got.counts[c])


def test_counts_null():
    n, C, fmt = 2049, 3, (STD, 7, 4)
    X = _inputs(C, n, 13)
    seeds, ctrs = [1, 2, 3], [4, 5, 6]
    want, got = Out(C, n, 4), Out(C, n, 4)
    _auto_each(X, n, fmt, INF, seeds, ctrs, want, counts=False)
    _round(X, C, n, fmt, INF, seeds, ctrs, got, counts=False)
    assert got.same(want, C)
    assert bool((got.counts == GARBAGE).all())  # (no slot given: none written)


@pytest.mark.parametrize("kind,levels,p", [(STD, 127, math.inf), (STD, 7, 2), (NATD, 7, math.inf), (NATD, 1, 2)])
def test_records_decode_to_the_oracle(kind, levels, p):
    """The batched records, decoded, are the CPU oracle's vectors (as tests/test_gpu_codec.py pins the per-message
    encoder): p = inf exactly; p = 2 with the device norm handed to the oracle."""
    from fl_sim_amd import codec
    from oracle import compressors_ref as ref

    n, C = 3001, 3
    bits = codec.code_bits(levels)
    X = _inputs(C, n, 17)
    xs = [X[c, :n] for c in range(C)]
    seeds, ctrs = [5, 6, 7], [9, 8, 7]
    stride, _ = codec.dense_wire_layout(n, kind, bits)
    recs = torch.empty(C, stride, dtype=torch.uint8, device="cuda")
    counts = torch.full((C,), GARBAGE, dtype=torch.int64, device="cuda")
    codec.quant_encode_round(xs, kind, levels, bits, INF if math.isinf(p) else L2, seeds, ctrs, recs,
                             counts if kind == STD else None)
    fn = ref.standard_dithering if kind == STD else ref.natural_dithering
    for c in range(C):
        x = xs[c].cpu().numpy()
        norm, _ = codec.dense_wire_views(recs[c], n, kind, bits)
        got = codec.dense_record_decode(recs[c], n, kind, levels, bits).cpu().numpy()
        pn = None if math.isinf(p) else np.float32(norm.item())
        want, _, wn = fn(x, levels, p, ref.philox_stream(seeds[c], ctrs[c], n), pnorm=pn)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), c
        if math.isinf(p):
            assert np.float32(norm.item()) == np.float32(wn)
        else:
            assert abs(float(norm.item()) - float(np.linalg.norm(x.astype(np.float64)))) <= 1e-6 * float(norm.item())
        if kind == STD:
            assert int(counts[c]) == int(np.count_nonzero(x))


def test_capture_replays_with_new_inputs():
    """Captured once, replayed on changed inputs: the table went into the kernel arguments at capture, so the host
    arrays may be gone; the result equals the eager call's."""
    n, C, fmt = 4097, 5, (STD, 127, 8)
    X = _inputs(C, n, 23)
    seeds, ctrs = [31, 32, 33, 34, 35], [1, 1, 2, 3, 5]
    s = torch.cuda.Stream()
    got = Out(C, n, 8)
    with torch.cuda.stream(s):
        ws = _round(X, C, n, fmt, L2, seeds, ctrs, got)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _round(X, C, n, fmt, L2, seeds, ctrs, got, ws=ws)
    gen = torch.Generator(device="cuda").manual_seed(29)
    for r in range(2):
        X[:, :n] = torch.randn(C, n, generator=gen, device="cuda") * 10.0 ** (-r - 1)
        X[r, ::5] = 0.0  # (a zero pattern that changes with the replay)
        got.counts.fill_(GARBAGE)
        g.replay()
        torch.cuda.synchronize()
        want = Out(C, n, 8)
        _round(X, C, n, fmt, L2, seeds, ctrs, want)
        torch.cuda.synchronize()
        assert got.same(want, C), r
