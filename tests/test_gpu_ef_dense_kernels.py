"""flc_quant_encode_residual_round against the three-call chain it replaces, on copies of the same memories, bit for
bit: flc_quant_encode_round, flc_quant_decode of each record into a fresh vector, flc_ef_residual_dense.  Codes, norms,
counts and memories over the sizes at which the encode changes its path (the group of 8, the 2048-element block, the
4096-element norm chunk, each +-1, and 70,001), every code width and both quantizers, p = inf and 2, 1 to 65 messages
(65: a chain of two tables) with seeds and counters that differ; a p = 2 norm past kNormMaxParts chunks; zero, -0, NaN,
+-inf and denormal messages between ordinary ones; counts == NULL; graph capture."""

import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STD, NATD = 0, 1
INF, L2 = 0, 2
FORMATS = [(STD, 127, 8), (STD, 7, 4), (STD, 1, 2), (NATD, 127, 8), (NATD, 7, 4), (NATD, 1, 2)]
SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 4095, 4096, 4097, 70001]
MSGS = [1, 2, 64, 65]
PAD = 0xA5  # what the code buffers hold before a call: bytes past ceil(n * bits / 8) must keep it
GARBAGE = -0x0123456789ABCDEF  # what the count slots hold before a call
TAIL = 0x7FC12345  # the bits of the row elements past n (16-B rows): never read, never written

P = ctypes.c_void_p
U64 = ctypes.c_uint64
vp = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731


def _L():
    from fl_sim_amd import _lib

    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int32)


def _same(got, want):
    """Bit equality of two fp32 tensors; a mismatch reports the first differing element and both patterns."""
    g, w = _bits(got), _bits(want)
    if torch.equal(g, w):
        return True
    at = (g != w).nonzero()
    first = tuple(int(i) for i in at[0])
    raise AssertionError(f"{at.shape[0]} elements differ, first at {first}: got {int(g[first]) & 0xFFFFFFFF:#010x}, "
                         f"want {int(w[first]) & 0xFFFFFFFF:#010x}")


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
                and torch.equal(_bits(self.norms[:C]), _bits(other.norms[:C]))
                and torch.equal(self.counts[:C], other.counts[:C]))


def _tables(E, C, out: Out, seeds, ctrs, counts):
    return (vp((P * C)(*[E[c].data_ptr() for c in range(C)])), vp((U64 * C)(*seeds[:C])), vp((U64 * C)(*ctrs[:C])),
            vp((P * C)(*[out.codes[c].data_ptr() for c in range(C)])),
            vp((P * C)(*[out.norms[c:c + 1].data_ptr() for c in range(C)])),
            vp((P * C)(*[out.counts[c:c + 1].data_ptr() for c in range(C)])) if counts else None)


def _round_call(entry, E, C, n, fmt, pk, seeds, ctrs, out: Out, counts=True, ws=None):
    L = _L()
    kind, levels, bits = fmt
    if ws is None:
        ws = torch.empty(L.size("flc_quant_encode_round_workspace_size", n, C), dtype=torch.uint8, device=E.device)
    xs, sd, ct, cd, nm, cn = _tables(E, C, out, seeds, ctrs, counts)
    L.call(entry, xs, C, n, kind, levels, bits, pk, sd, ct, cd, nm, cn, ws.data_ptr(), ws.numel(), _stream())
    return ws


def _chain(E, C, n, fmt, pk, seeds, ctrs, out: Out, counts=True):
    """The reference on the memories ``E`` (in place): the round's plain encode, every record decoded into a fresh
    vector, the dense residual."""
    from fl_sim_amd import codec

    L = _L()
    kind, levels, bits = fmt
    _round_call("flc_quant_encode_round", E, C, n, fmt, pk, seeds, ctrs, out, counts)
    for c in range(C):
        dec = torch.full((n,), 12345.0, dtype=torch.float32, device=E.device)
        L.call("flc_quant_decode", out.codes[c].data_ptr(), 1, n, kind, levels, bits, out.norms[c:c + 1].data_ptr(),
               None, 0, dec.data_ptr(), _stream())
        codec.ef_residual_dense(E[c, :n], dec)


def _residual(E, C, n, fmt, pk, seeds, ctrs, out: Out, counts=True, ws=None):
    return _round_call("flc_quant_encode_residual_round", E, C, n, fmt, pk, seeds, ctrs, out, counts, ws)


def _inputs(C, n, seed):
    """[C, n rounded up to 4] fp32 (16-B rows): memory-sized values with zeros and -0 sprinkled in."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(C, (n + 3) // 4 * 4, generator=g, device="cuda") * 1e-3
    m = torch.rand(X.shape, generator=g, device="cuda")
    X[m < 0.05] = 0.0
    X[(m >= 0.05) & (m < 0.07)] = -0.0
    _bits(X)[:, n:] = TAIL
    return X


def _seeds(C):
    return [0x9E3779B97F4A7C15 * (c + 1) % (1 << 64) for c in range(C)], [3 * c + 1 for c in range(C)]


@pytest.mark.parametrize("pk", [INF, L2], ids=["inf", "p2"])
@pytest.mark.parametrize("n", SIZES)
def test_residual_round_equals_the_chain(n, pk):
    Cmax = max(MSGS)
    A = _inputs(Cmax, n, 2000 + n)
    seeds, ctrs = _seeds(Cmax)
    for fmt in FORMATS:
        want_e, want = A.clone(), Out(Cmax, n, fmt[2])
        _chain(want_e, Cmax, n, fmt, pk, seeds, ctrs, want)  # (messages are independent: its first C serve every C)
        assert not torch.equal(_bits(want_e), _bits(A))
        for C in MSGS:
            got_e, got = A.clone(), Out(Cmax, n, fmt[2])
            _residual(got_e, C, n, fmt, pk, seeds, ctrs, got)
            assert got.same(want, C), (n, pk, fmt, C)
            assert _same(got_e[:C], want_e[:C]), (n, pk, fmt, C)
            # messages past C untouched: memories, codes and counts; nothing written past a message's code bytes
            assert torch.equal(_bits(got_e[C:]), _bits(A[C:]))
            assert bool((got.codes[C:] == PAD).all()) and bool((got.codes[:, got.cb:] == PAD).all())
            assert bool((got.counts[C:] == GARBAGE).all())


def test_residual_is_input_minus_decoded_value():
    """The chain's meaning, checked once on the host: e' = fp32(a − decode(record)), zeros kept with their sign."""
    from fl_sim_amd import codec

    n, C, fmt = 2049, 2, (STD, 1, 2)
    A = _inputs(C, n, 3)
    seeds, ctrs = _seeds(C)
    E, out = A.clone(), Out(C, n, 2)
    _residual(E, C, n, fmt, INF, seeds, ctrs, out)
    for c in range(C):
        dec = torch.empty(n, dtype=torch.float32, device="cuda")
        _L().call("flc_quant_decode", out.codes[c].data_ptr(), 1, n, STD, 1, 2, out.norms[c:c + 1].data_ptr(), None, 0,
                  dec.data_ptr(), _stream())
        a, v, e = A[c, :n].cpu().numpy(), dec.cpu().numpy(), E[c, :n].cpu().numpy()
        assert np.array_equal((a - v).view(np.uint32), e.view(np.uint32))
        zero = a == 0
        assert zero.any() and np.array_equal(e[zero].view(np.uint32), a[zero].view(np.uint32))  # (-0 stays -0)
        assert float(np.abs(e).max()) <= float(out.norms[c])  # s = 1: every value within one level of its code
    assert codec.code_bits(1) == 2


def test_p2_norm_past_the_partial_limit():
    """n = 4,194,309: more than kNormMaxParts chunks of kNormChunk elements, so the chunk grows (4-aligned)."""
    n, C, fmt = 4_194_304 + 5, 2, (STD, 127, 8)
    A = _inputs(C, n, 5)
    seeds, ctrs = [11, 12], [1, 2]
    want_e, want, got_e, got = A.clone(), Out(C, n, 8), A.clone(), Out(C, n, 8)
    _chain(want_e, C, n, fmt, L2, seeds, ctrs, want)
    _residual(got_e, C, n, fmt, L2, seeds, ctrs, got)
    assert got.same(want, C) and _same(got_e, want_e)
    ref = torch.sqrt((A[:, :n].double() ** 2).sum(1)).float()
    assert torch.allclose(got.norms, ref, rtol=1e-6)  # (the chain is the bit-level check above)


@pytest.mark.parametrize("pk", [INF, L2], ids=["inf", "p2"])
@pytest.mark.parametrize("fmt", [(STD, 127, 8), (STD, 7, 4), (STD, 1, 2), (NATD, 7, 4), (NATD, 1, 2)], ids=str)
def test_edge_messages_between_ordinary_ones(fmt, pk):
    n, C = 4097, 11
    A = _inputs(C, n, 9)
    A[1, :n] = 0.0  # norm 0, every element +0
    A[3, :n] = -0.0  # norm 0, every element -0
    A[5, 1234] = float("nan")  # norm NaN
    A[7, 17] = float("inf")  # norm inf, with -inf and -0 among the elements
    A[7, 2048] = float("-inf")
    A[7, 100:200] = -0.0
    _bits(A)[9, :n] = torch.randint(0, 1 << 23, (n,), device="cuda", dtype=torch.int32)  # denormals (and a few zeros)
    _bits(A)[9, ::2] |= -(1 << 31)  # (every other one negative)
    A[9, 50:60] = 0.0
    seeds, ctrs = list(range(21, 21 + C)), list(range(C))
    want_e, want, got_e, got = A.clone(), Out(C, n, fmt[2]), A.clone(), Out(C, n, fmt[2])
    _chain(want_e, C, n, fmt, pk, seeds, ctrs, want)
    _residual(got_e, C, n, fmt, pk, seeds, ctrs, got)
    assert got.same(want, C)
    assert _same(got_e, want_e)
    norms = got.norms.cpu().numpy()
    assert norms[1] == 0.0 and norms[3] == 0.0 and math.isnan(norms[5]) and math.isinf(norms[7])
    ordinary = (0, 2, 4, 6, 8, 10)
    assert all(np.isfinite(norms[c]) and norms[c] > 0 for c in ordinary)  # (a neighbour's NaN did not reach them)
    # a norm that is not regular: a zero code leaves a as it is (the sign of a zero included), any other gives NaN
    assert torch.equal(_bits(got_e[1]), _bits(A[1])) and torch.equal(_bits(got_e[3]), _bits(A[3]))
    for c in (5, 7):
        a, e = A[c, :n], got_e[c, :n]
        zero = a == 0
        assert bool(zero.any()) and torch.equal(_bits(e[zero]), _bits(a[zero]))
        assert bool(torch.isnan(e[~zero]).all())
    assert bool(torch.isfinite(got_e[9, :n]).all())
    # the ordinary messages alone, each at the same (seed, counter): nothing of theirs depends on their neighbours
    for c in ordinary:
        alone_e, alone = A[c:c + 1].clone(), Out(1, n, fmt[2])
        _residual(alone_e, 1, n, fmt, pk, seeds[c:c + 1], ctrs[c:c + 1], alone)
        assert torch.equal(alone.codes[0], got.codes[c]) and torch.equal(alone.norms[0], got.norms[c])
        assert torch.equal(alone.counts[0], got.counts[c]) and torch.equal(_bits(alone_e[0]), _bits(got_e[c]))
        assert bool(torch.isfinite(got_e[c, :n]).all())


def test_counts_null():
    n, C, fmt = 2049, 3, (STD, 7, 4)
    A = _inputs(C, n, 13)
    seeds, ctrs = [1, 2, 3], [4, 5, 6]
    want_e, want, got_e, got = A.clone(), Out(C, n, 4), A.clone(), Out(C, n, 4)
    _chain(want_e, C, n, fmt, INF, seeds, ctrs, want, counts=False)
    _residual(got_e, C, n, fmt, INF, seeds, ctrs, got, counts=False)
    assert got.same(want, C) and _same(got_e, want_e)
    assert bool((got.counts == GARBAGE).all())  # (no slot given: none written)


def test_codec_wrapper_writes_records_and_memories():
    """codec.quant_encode_residual_round: the records of codec.quant_encode_round, the memories of the dense chain; a
    memory it would have to copy is refused, since the residual is written in place."""
    from fl_sim_amd import codec

    n, C, kind, levels = 3001, 3, STD, 7
    bits = codec.code_bits(levels)
    A = _inputs(C, n, 17)
    seeds, ctrs = [5, 6, 7], [9, 8, 7]
    stride, _ = codec.dense_wire_layout(n, kind, bits)
    want_r, got_r = (torch.zeros(C, stride, dtype=torch.uint8, device="cuda") for _ in range(2))
    want_c, got_c = (torch.full((C,), GARBAGE, dtype=torch.int64, device="cuda") for _ in range(2))
    E = A.clone()
    mems = [E[c, :n] for c in range(C)]
    codec.quant_encode_round([A[c, :n] for c in range(C)], kind, levels, bits, L2, seeds, ctrs, want_r, want_c)
    codec.quant_encode_residual_round(mems, kind, levels, bits, L2, seeds, ctrs, got_r, got_c)
    assert torch.equal(got_r, want_r) and torch.equal(got_c, want_c)
    for c in range(C):
        want_e = A[c, :n].clone()
        codec.ef_residual_dense(want_e, codec.dense_record_decode(want_r[c], n, kind, levels, bits))
        assert _same(mems[c], want_e)
    before = E.clone()
    with pytest.raises(ValueError):
        codec.quant_encode_residual_round([E[0, 1:n + 1]] + mems[1:], kind, levels, bits, L2, seeds, ctrs, got_r, got_c)
    with pytest.raises(RuntimeError):  # (FLC_EINVAL: one memory twice)
        codec.quant_encode_residual_round([mems[0], mems[1], mems[0]], kind, levels, bits, L2, seeds, ctrs, got_r, got_c)
    assert torch.equal(_bits(E), _bits(before))  # (nothing launched)


def test_capture_replays_with_new_memory_contents():
    """Captured once, replayed on changed memories: the table went into the kernel arguments at capture; the result
    equals the eager chain's."""
    n, C, fmt = 4097, 5, (STD, 127, 8)
    A = _inputs(C, n, 23)
    E = A.clone()
    seeds, ctrs = [31, 32, 33, 34, 35], [1, 1, 2, 3, 5]
    s = torch.cuda.Stream()
    got = Out(C, n, 8)
    with torch.cuda.stream(s):
        ws = _residual(E, C, n, fmt, L2, seeds, ctrs, got)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _residual(E, C, n, fmt, L2, seeds, ctrs, got, ws=ws)
    gen = torch.Generator(device="cuda").manual_seed(29)
    for r in range(2):
        A[:, :n] = torch.randn(C, n, generator=gen, device="cuda") * 10.0 ** (-r - 1)
        A[r, ::5] = 0.0  # (a zero pattern that changes with the replay)
        E.copy_(A)
        got.counts.fill_(GARBAGE)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_e, want = A.clone(), Out(C, n, 8)
        _chain(want_e, C, n, fmt, L2, seeds, ctrs, want)
        torch.cuda.synchronize()
        assert got.same(want, C) and _same(E, want_e), r
