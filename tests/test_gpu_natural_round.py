"""flc_natural_encode_round and flc_natural_encode_residual_round, bit for bit: the plain form against the per-message
flc_natural_encode with the same seeds and counters, the residual form against the chain it replaces on copies of the
same memories (plain form, flc_natural_decode of each code stream into a fresh vector, flc_ef_residual_dense).  Sizes
around the group of 8, one thread sweep of 256 x 8 and the 8192-element block; 1 to 65 messages (65: a chain of two
tables) with seeds and counters that all differ; special messages between ordinary ones; the decision edges against
the CPU oracle; graph capture."""

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import quant_cases as qc

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 2047, 2048, 2049, 8191, 8192, 8193, 16389, 70001]
MSGS = [1, 2, 64, 65]
PAD = 0xA5  # what the code rows hold before a call: bytes past 2n must keep it
TAIL = 0x7FC12345  # the bits of the row elements past n (16-B rows): never read, never written
PLAIN, RESIDUAL = "flc_natural_encode_round", "flc_natural_encode_residual_round"

P = ctypes.c_void_p
U64 = ctypes.c_uint64
vp = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731


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


def _code_rows(C, n):
    """[C, row] code bytes (16-B rows, >= 16 B of padding), pre-filled with the pad byte."""
    row = (2 * n + 16 + 15) // 16 * 16
    return torch.full((C, row), PAD, dtype=torch.uint8, device="cuda")


def _round_call(entry, E, C, n, seeds, ctrs, codes):
    _L().call(entry, vp((P * C)(*[E[c].data_ptr() for c in range(C)])), C, n, vp((U64 * C)(*seeds[:C])),
              vp((U64 * C)(*ctrs[:C])), vp((P * C)(*[codes[c].data_ptr() for c in range(C)])), _stream())


def _single(x, n, seed, ctr, codes_row):
    """The per-message encoder (philox mode, no count)."""
    _L().call("flc_natural_encode", x.data_ptr(), n, seed, ctr, None, codes_row.data_ptr(), None, None, 0, _stream())


def _chain(E, C, n, seeds, ctrs, codes):
    """The reference on the memories ``E`` (in place): the round's plain encode, every code stream decoded into a fresh
    vector, the dense residual."""
    from fl_sim_amd import codec

    _round_call(PLAIN, E, C, n, seeds, ctrs, codes)
    for c in range(C):
        dec = torch.full((n,), 12345.0, dtype=torch.float32, device=E.device)
        _L().call("flc_natural_decode", codes[c].data_ptr(), n, 1.0, 0, dec.data_ptr(), _stream())
        codec.ef_residual_dense(E[c, :n], dec)


def _inputs(C, n, seed):
    """[C, n rounded up to 4] fp32 (16-B rows): memory-sized values over many binades with zeros and -0 sprinkled in;
    the row elements past n hold the marker."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.randn(C, (n + 3) // 4 * 4, generator=g, device="cuda") * 1e-3
    X *= torch.exp2(torch.randint(-20, 20, X.shape, generator=g, device="cuda").float())
    m = torch.rand(X.shape, generator=g, device="cuda")
    X[m < 0.05] = 0.0
    X[(m >= 0.05) & (m < 0.07)] = -0.0
    _bits(X)[:, n:] = TAIL
    return X


def _seeds(C):
    return [0x9E3779B97F4A7C15 * (c + 1) % (1 << 64) for c in range(C)], [3 * c + 1 for c in range(C)]


@functools.lru_cache(maxsize=None)
def _case(n):
    """(inputs, seeds, counters, the per-message encoder's code rows) for max(MSGS) messages of n elements, computed
    once and left unchanged."""
    Cmax = max(MSGS)
    A = _inputs(Cmax, n, 2000 + n)
    seeds, ctrs = _seeds(Cmax)
    want = _code_rows(Cmax, n)
    for c in range(Cmax):
        _single(A[c], n, seeds[c], ctrs[c], want[c])
    return A, seeds, ctrs, want


@pytest.mark.parametrize("n", SIZES)
def test_plain_round_equals_the_per_message_encoder(n):
    A, seeds, ctrs, want = _case(n)
    keep = A.clone()
    assert bool((want[:, :2 * n] != PAD).any()) and bool((want[:, 2 * n:] == PAD).all())
    assert n < 2047 or not torch.equal(want[0, :2 * n], want[1, :2 * n])
    for C in MSGS:
        got = _code_rows(max(MSGS), n)
        _round_call(PLAIN, A, C, n, seeds, ctrs, got)
        assert torch.equal(got[:C], want[:C]), (n, C)  # (the codes, and the pad bytes past 2n)
        assert bool((got[C:] == PAD).all()), (n, C)
    assert torch.equal(_bits(A), _bits(keep))  # (the plain form writes no input)


@pytest.mark.parametrize("n", SIZES)
def test_residual_round_equals_the_chain(n):
    A, seeds, ctrs, plain = _case(n)
    Cmax = max(MSGS)
    want_e, want = A.clone(), _code_rows(Cmax, n)
    _chain(want_e, Cmax, n, seeds, ctrs, want)  # (messages are independent: its first C serve every C)
    assert torch.equal(want, plain)
    assert not torch.equal(_bits(want_e[:, :n]), _bits(A[:, :n]))
    assert torch.equal(_bits(want_e[:, n:]), _bits(A[:, n:]))
    for C in MSGS:
        got_e, got = A.clone(), _code_rows(Cmax, n)
        _round_call(RESIDUAL, got_e, C, n, seeds, ctrs, got)
        assert torch.equal(got[:C], plain[:C]), (n, C)  # (the plain form's codes, pad bytes past 2n kept)
        assert _same(got_e[:C], want_e[:C]), (n, C)  # (the markers past n included)
        # messages past C untouched: memories and codes
        assert torch.equal(_bits(got_e[C:]), _bits(A[C:])) and bool((got[C:] == PAD).all())


def test_residual_is_input_minus_decoded_value():
    """The chain's meaning, checked once on the host: e' = fp32(a − 2^e), zeros kept with their sign, and every
    residual smaller than the value it is left from (the code is one of the two powers of two around |a|)."""
    n, C = 2049, 2
    A = _inputs(C, n, 3)
    seeds, ctrs = _seeds(C)
    E, codes = A.clone(), _code_rows(C, n)
    _round_call(RESIDUAL, E, C, n, seeds, ctrs, codes)
    for c in range(C):
        dec = torch.empty(n, dtype=torch.float32, device="cuda")
        _L().call("flc_natural_decode", codes[c].data_ptr(), n, 1.0, 0, dec.data_ptr(), _stream())
        a, v, e = A[c, :n].cpu().numpy(), dec.cpu().numpy(), E[c, :n].cpu().numpy()
        assert np.array_equal((a - v).view(np.uint32), e.view(np.uint32))
        zero = a == 0
        assert zero.any() and np.array_equal(e[zero].view(np.uint32), a[zero].view(np.uint32))  # (-0 stays -0)
        assert np.all(np.abs(e) <= np.abs(a))  # (|a| in [2^f, 2^(f+1)], the code 2^f or 2^(f+1): |a − v| <= 2^f)


SPECIALS = ("pzero", "nzero", "nan", "inf", "subnormal", "pow2", "fltmax")


def _special_messages(n):
    """Ordinary messages at the even rows, one special message at each odd row."""
    C = 2 * len(SPECIALS) + 1
    A = _inputs(C, n, 9)
    row = {name: 2 * i + 1 for i, name in enumerate(SPECIALS)}
    A[row["pzero"], :n] = 0.0
    A[row["nzero"], :n] = -0.0
    b = _bits(A)
    b[row["nan"], 0:n:3] = 0x7FC00000  # the canonical NaN,
    b[row["nan"], 1:n:7] = 0x7F800001  # a signalling one with the smallest payload,
    b[row["nan"], 2:n:11] = -1  # 0xffffffff: negative, every payload bit set,
    b[row["nan"], 5:n:13] = -(1 << 31) | 0x7FA5A5A5  # and a negative one with a pattern
    A[row["inf"], 17] = float("inf")
    A[row["inf"], 2048] = float("-inf")
    A[row["inf"], n - 1] = float("inf")
    A[row["inf"], 100:200] = -0.0
    b[row["subnormal"], :n] = torch.randint(1, 1 << 23, (n,), device="cuda", dtype=torch.int32)
    b[row["subnormal"], 0:n:4] = 1  # the smallest subnormal
    b[row["subnormal"], 1:n:4] = 0x007FFFFF  # the largest
    b[row["subnormal"], ::2] |= -(1 << 31)  # (every other one negative)
    p2 = np.ldexp(np.float32(1), np.arange(n) % 277 - 149).astype(np.float32)  # 2^-149 .. 2^127
    p2[1::2] *= -1
    assert np.all(p2 != 0)
    A[row["pow2"], :n] = torch.from_numpy(p2).cuda()
    A[row["fltmax"], :n] = torch.finfo(torch.float32).max
    A[row["fltmax"], 1:n:2] *= -1.0
    return A, row, C


def test_special_messages_between_ordinary_ones():
    n = 8197  # (two blocks, the second a tail group of 5)
    A, row, C = _special_messages(n)
    seeds, ctrs = list(range(21, 21 + C)), list(range(C))
    want_e, want = A.clone(), _code_rows(C, n)
    _chain(want_e, C, n, seeds, ctrs, want)
    single = _code_rows(C, n)
    for c in range(C):
        _single(A[c], n, seeds[c], ctrs[c], single[c])
    plain = _code_rows(C, n)
    _round_call(PLAIN, A, C, n, seeds, ctrs, plain)
    got_e, got = A.clone(), _code_rows(C, n)
    _round_call(RESIDUAL, got_e, C, n, seeds, ctrs, got)
    assert torch.equal(plain, single) and torch.equal(got, single) and torch.equal(want, single)
    assert _same(got_e, want_e)
    cd = lambda name: got[row[name], :2 * n].view(torch.int16).int() & 0xFFFF  # noqa: E731
    a = lambda name: A[row[name], :n]  # noqa: E731
    e = lambda name: got_e[row[name], :n]  # noqa: E731
    # zeros: code 0, and a − (+0) keeps a, the sign of a zero included
    for name in ("pzero", "nzero"):
        assert bool((cd(name) == 0).all()) and torch.equal(_bits(e(name)), _bits(a(name)))
    assert int(_bits(e("nzero"))[0]) == -(1 << 31)
    # NaN: code 0x7fff whatever the sign and payload, residual NaN (its bits: the chain's, above)
    nan = torch.isnan(a("nan"))
    assert int(nan.sum()) > n // 3 and bool((cd("nan")[nan] == 0x7FFF).all()) and bool(torch.isnan(e("nan")[nan]).all())
    assert bool(torch.isfinite(e("nan")[~nan]).all())
    # +-inf: the code of 2^128 with the sign; inf − inf is NaN
    inf = torch.isinf(a("inf"))
    assert int(inf.sum()) == 3 and bool(torch.isnan(e("inf")[inf]).all()) and bool(torch.isfinite(e("inf")[~inf]).all())
    assert cd("inf")[17] == 278 and cd("inf")[2048] == (1 << 15 | 278) and cd("inf")[n - 1] == 278
    # subnormals: every code a power of two between 2^-149 and 2^-126, the residual finite
    sub = cd("subnormal") & 0x7FFF
    assert bool(((sub >= 1) & (sub <= 24)).all()) and bool(torch.isfinite(e("subnormal")).all())
    assert bool((sub[0:n:4] == 1).all())  # (2^-149 is a power of two: itself)
    # exact powers of two map to themselves: the residual is +0
    assert bool((_bits(e("pow2")) == 0).all())
    # FLT_MAX rounds up to 2^128 = inf unless u < pt = 2^-23: the residual of those is -+inf
    up = (cd("fltmax") & 0x7FFF) == 278
    assert int(up.sum()) >= n - 8 and bool(torch.isinf(e("fltmax")[up]).all())
    assert bool((torch.sign(e("fltmax")[up]) == -torch.sign(a("fltmax")[up])).all())
    # the ordinary messages alone, each at the same (seed, counter): nothing of theirs depends on their neighbours
    for c in range(0, C, 2):
        alone_e, alone = A[c:c + 1].clone(), _code_rows(1, n)
        _round_call(RESIDUAL, alone_e, 1, n, seeds[c:c + 1], ctrs[c:c + 1], alone)
        assert torch.equal(alone[0], got[c]) and torch.equal(_bits(alone_e[0]), _bits(got_e[c]))
        assert bool(torch.isfinite(got_e[c, :n]).all())


def test_decision_edges_against_the_oracle():
    """u == pt ties planted per message with that message's own (seed, counter): the round form against the CPU
    oracle's natural compressor, independently of the library's single-message encoder; the residual form leaves
    fp32(x − oracle value)."""
    from oracle import compressors_ref as ref

    n, C = 65_543, 3
    seeds, ctrs = [0x1234567, 0x89ABCDEF01, 77], [5, 1 << 33, 0]
    xs, exps = [], []
    for c in range(C):
        x, tie = qc.natural_edge_case(n, seeds[c], ctrs[c], np.random.default_rng(3 + c))
        u = ref.philox_uniforms(n, seeds[c], ctrs[c])
        with np.errstate(over="ignore"):
            exp, _, _ = ref.natural(x, lambda i: u[i])
        assert int(tie.sum()) >= 20 and np.isposinf(exp).any() and np.isneginf(exp).any()
        xs.append(x)
        exps.append(np.ascontiguousarray(exp, dtype=np.float32))
    A = torch.zeros(C, (n + 3) // 4 * 4, dtype=torch.float32, device="cuda")
    for c in range(C):
        A[c, :n] = torch.from_numpy(xs[c]).cuda()
    for entry in (PLAIN, RESIDUAL):
        E, codes = A.clone(), _code_rows(C, n)
        _round_call(entry, E, C, n, seeds, ctrs, codes)
        for c in range(C):
            dec = torch.empty(n, dtype=torch.float32, device="cuda")
            _L().call("flc_natural_decode", codes[c].data_ptr(), n, 1.0, 0, dec.data_ptr(), _stream())
            out = dec.cpu().numpy()
            bad = np.flatnonzero(out.view(np.uint32) != exps[c].view(np.uint32))
            assert bad.size == 0, (entry, c, bad.size,
                                   [(int(i), float(xs[c][i]), float(out[i]), float(exps[c][i])) for i in bad[:5]])
            if entry == RESIDUAL:
                with np.errstate(all="ignore"):
                    want = xs[c] - exps[c]
                assert not np.isnan(want).any()
                assert np.array_equal(E[c, :n].cpu().numpy().view(np.uint32), want.view(np.uint32)), c
            else:
                assert torch.equal(_bits(E), _bits(A))


def test_codec_wrappers_write_records_and_memories():
    """codec.natural_encode_round into a record block and into a list of records; codec.natural_encode_residual_round
    leaves the dense chain's memories; a memory it would have to copy is refused, since the residual is written in
    place."""
    from fl_sim_amd import _lib, codec

    n, C = 3001, 3
    fmt = _lib.FLC_WIRE_NATURAL
    A = _inputs(C, n, 17)
    seeds, ctrs = [5, 6, 7], [9, 8, 7]
    stride, _ = codec.dense_wire_layout(n, fmt, 16)
    want_r, got_r = (torch.zeros(C, stride, dtype=torch.uint8, device="cuda") for _ in range(2))
    listed = [torch.zeros(stride, dtype=torch.uint8, device="cuda") for _ in range(C)]
    E = A.clone()
    mems = [E[c, :n] for c in range(C)]
    codec.natural_encode_round([A[c, :n] for c in range(C)], seeds, ctrs, want_r)
    codec.natural_encode_round([A[c, :n] for c in range(C)], seeds, ctrs, listed)
    codec.natural_encode_residual_round(mems, seeds, ctrs, got_r)
    for c in range(C):
        single, _ = codec.natural_encode(A[c, :n].clone(), seeds[c], ctrs[c])
        codes = codec.dense_wire_views(want_r[c], n, fmt, 16)[1]
        assert torch.equal(codes.view(torch.int16), single.view(torch.int16))
        assert torch.equal(listed[c], want_r[c]) and torch.equal(got_r[c], want_r[c])
        want_e = A[c, :n].clone()
        codec.ef_residual_dense(want_e, codec.dense_record_decode(want_r[c], n, fmt, 0, 16))
        assert _same(mems[c], want_e)
    before = E.clone()
    with pytest.raises(ValueError):
        codec.natural_encode_residual_round([E[0, 1:n + 1]] + mems[1:], seeds, ctrs, got_r)
    with pytest.raises(RuntimeError):  # (FLC_EINVAL: one memory twice)
        codec.natural_encode_residual_round([mems[0], mems[1], mems[0]], seeds, ctrs, got_r)
    assert torch.equal(_bits(E), _bits(before))  # (nothing launched)


@pytest.mark.parametrize("entry", [PLAIN, RESIDUAL])
def test_capture_replays_equal_the_eager_call(entry):
    """Captured once in a linear graph and replayed on changed contents: the table went into the kernel arguments at
    capture; the result equals the eager call's."""
    n, C = 8197, 5
    A = _inputs(C, n, 23)
    E = A.clone()
    seeds, ctrs = [31, 32, 33, 34, 35], [1, 1, 2, 3, 5]
    s = torch.cuda.Stream()
    got = _code_rows(C, n)
    with torch.cuda.stream(s):
        _round_call(entry, E, C, n, seeds, ctrs, got)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        _round_call(entry, E, C, n, seeds, ctrs, got)
    gen = torch.Generator(device="cuda").manual_seed(29)
    for r in range(2):
        A[:, :n] = torch.randn(C, n, generator=gen, device="cuda") * 10.0 ** (-r - 1)
        A[r, ::5] = 0.0  # (a zero pattern that changes with the replay)
        E.copy_(A)
        got.fill_(PAD)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        want_e, want = A.clone(), _code_rows(C, n)
        _round_call(entry, want_e, C, n, seeds, ctrs, want)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and _same(E, want_e), r
        assert torch.equal(_bits(E), _bits(A)) == (entry == PLAIN)
