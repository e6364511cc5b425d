"""Bucketed dithering on the device (flc_bucket_encode / _encode_round / _decode, Compressor(bucket=B)), bit for bit:
against the existing per-row entry points on [nb, B] batches, against the numpy bucket model (tests/bucket_ref.py: the
oracle's dithering rule per slice) in philox mode over tails shorter than a group of 8 and than a quad, a partly used
last code byte and several blocks, p = inf and 2; bucket isolation under NaN, inf and a zeroed bucket; the decode with
weight and accumulate; the round form over 3 and 70 messages; given norms; and compat mode against
tests/golden/bucket_codec.npz (the reference's own compressVector on every slice)."""

import functools
import random

import numpy as np
import pytest
import torch

from oracle import compressors_ref as ref
from tests import bucket_ref as br
from tests import golden_cases as gc
from tests.golden.gen_golden_bucket import bucket_cases, bucket_key, bucket_seed

pytestmark = pytest.mark.gpu

STD, NATD = 0, 1
INF, L2 = 0, 2
FORMATS = [(2, 1), (4, 7), (8, 127)]  # (bits, levels)
SEED, CTR = 0x1234_5678_9ABC, 77
PAD = 0xA5


def _codec():
    from fl_sim_amd import codec

    return codec


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@functools.lru_cache(maxsize=None)
def _normal(n, seed=5):
    g = np.random.default_rng(seed * 1000 + n)
    x = g.standard_normal(n).astype(np.float32) * np.float32(1e-2)
    x[g.random(n) < 0.05] = 0.0
    x[3::101] = -0.0
    return x


@functools.lru_cache(maxsize=None)
def _dyadic(n):
    """m * 2^-12 with integer |m| < 2^11: every square and every sum of up to 4096 squares is exact in fp64."""
    g = np.random.default_rng(9000 + n)
    m = g.integers(-(2 ** 11) + 1, 2 ** 11, size=n)
    m[g.random(n) < 0.05] = 0
    return (m.astype(np.float64) * 2.0 ** -12).astype(np.float32)


def _encode(x, kind, levels, B, p=INF, norms=None, want_nnz=True, decode=True, seed=SEED, ctr=CTR):
    """(norms, codes bytes, nnz, out) as numpy, the record's padding checked to be untouched."""
    codec = _codec()
    n = len(x)
    bits = br.code_bits(levels)
    stride, off = codec.bucket_wire_layout(n, kind, bits, B)
    rec = torch.full((stride,), PAD, dtype=torch.uint8, device="cuda")
    _, nnz, out = codec.bucket_encode(_dev(x), kind, levels, B, p, seed, ctr, record=rec,
                                      norms=None if norms is None else _dev(norms), want_nnz=want_nnz, decode=decode)
    nv, cv = codec.bucket_wire_views(rec, n, kind, bits, B)
    r = rec.cpu().numpy()
    nb = -(-n // B)
    assert (r[4 * nb:off["codes"]] == PAD).all() and (r[off["codes"] + len(cv):] == PAD).all()
    return (nv.cpu().numpy(), cv.cpu().numpy(), None if nnz is None else int(nnz.item()),
            None if out is None else out.cpu().numpy(), rec)


# ------------------------------------------------------------------------------------- against existing code
@pytest.mark.parametrize("B,nb", [(64, 3), (512, 5), (4096, 2), (1024, 9)])
@pytest.mark.parametrize("kind", [STD, NATD])
def test_whole_buckets_equal_the_per_row_entry_points(B, nb, kind):
    codec = _codec()
    n = nb * B
    x = _normal(n)
    x2 = _dev(x).reshape(nb, B)
    for bits, levels in FORMATS:
        norms = codec.quant_norm(x2, np.inf)
        pkt = codec.quant_encode(x2, kind, levels, norms, SEED, CTR)
        pkt2, dec = codec.quant_encode_decode(x2, kind, levels, norms, SEED, CTR)
        nv, cv, nnz, out, _ = _encode(x, kind, levels, B)
        assert np.array_equal(nv.view(np.uint32), norms.cpu().numpy().view(np.uint32))
        assert np.array_equal(cv, pkt.codes.cpu().numpy()) and np.array_equal(cv, pkt2.codes.cpu().numpy())
        assert np.array_equal(out.view(np.uint32), dec.reshape(-1).cpu().numpy().view(np.uint32))
        assert nnz == int(pkt.nnz.sum().item()) == int(np.count_nonzero(x))


# ------------------------------------------------------------------------------------- against the oracle, philox
def _check_against_model(x, kind, levels, B, pnorms, got):
    nv, cv, nnz, out, _ = got
    bits = br.code_bits(levels)
    want_out, want_codes, want_nnz = br.bucket_philox(x, kind, levels, B, pnorms, SEED, CTR)
    assert np.array_equal(cv, br.pack(want_codes, bits))
    assert gc.same_bits(out, want_out)
    assert nnz == want_nnz


@pytest.mark.parametrize("n", [1, 63, 65, 4097, 12345, 70001])
@pytest.mark.parametrize("B", [64, 512, 4096])
def test_philox_p_inf_against_the_oracle(n, B):
    x = _normal(n)
    pn = np.array([np.max(np.abs(x[lo:hi])) for lo, hi in br.slices(n, B)], dtype=np.float32)  # the oracle's own max
    for kind in (STD, NATD):
        for bits, levels in FORMATS:
            got = _encode(x, kind, levels, B)
            assert np.array_equal(got[0].view(np.uint32), pn.view(np.uint32))
            _check_against_model(x, kind, levels, B, pn, got)


@pytest.mark.parametrize("n", [1, 63, 65, 4097, 12345, 70001])
@pytest.mark.parametrize("B", [64, 512, 4096])
def test_philox_p2_exact_sums(n, B):
    """Inputs whose squares sum exactly in fp64 in any order: the record's norms are float32(sqrt(sum))."""
    x = _dyadic(n)
    sq = x.astype(np.float64) ** 2
    pn = np.zeros(-(-n // B), dtype=np.float32)
    for b, (lo, hi) in enumerate(br.slices(n, B)):
        fwd = bwd = 0.0
        for v in sq[lo:hi]:
            fwd += v
        for v in sq[lo:hi][::-1]:
            bwd += v
        assert fwd == bwd == float(np.sum(sq[lo:hi]))
        pn[b] = np.float32(np.sqrt(np.float64(fwd)))
    for kind in (STD, NATD):
        for bits, levels in FORMATS:
            got = _encode(x, kind, levels, B, p=L2)
            assert np.array_equal(got[0].view(np.uint32), pn.view(np.uint32))
            _check_against_model(x, kind, levels, B, pn, got)


@pytest.mark.parametrize("n", [1, 63, 65, 4097, 12345, 70001])
@pytest.mark.parametrize("B", [64, 512, 4096])
def test_philox_p2_normal_inputs(n, B):
    """Each record norm within one fp32 ulp of the fp64 value; the codes are the oracle's under the record's norms."""
    x = _normal(n, seed=6)
    true = np.array([np.sqrt(np.sum(x[lo:hi].astype(np.float64) ** 2)) for lo, hi in br.slices(n, B)])
    first = None
    for kind in (STD, NATD):
        for bits, levels in FORMATS:
            got = _encode(x, kind, levels, B, p=L2)
            nv = got[0]
            assert np.all(np.abs(nv.astype(np.float64) - true) <= np.spacing(true.astype(np.float32)).astype(np.float64))
            first = nv if first is None else first
            assert np.array_equal(nv.view(np.uint32), first.view(np.uint32))  # (the norm does not depend on the format)
            _check_against_model(x, kind, levels, B, nv, got)


# ------------------------------------------------------------------------------------- bucket isolation
@pytest.mark.parametrize("B,n", [(64, 64 * 5 + 9), (512, 512 * 4 + 100), (4096, 4096 * 2 + 777)])
@pytest.mark.parametrize("what", ["nan", "inf", "zero"])
@pytest.mark.parametrize("p", [INF, L2])
def test_bucket_isolation(B, n, what, p):
    x = _normal(n, seed=7).copy()
    for kind, (bits, levels) in [(STD, FORMATS[2]), (NATD, FORMATS[1]), (STD, FORMATS[0])]:
        base = _encode(x, kind, levels, B, p=p)
        for b in (1, -(-n // B) - 1):  # an inner bucket and the short tail
            lo, hi = b * B, min((b + 1) * B, n)
            y = x.copy()
            if what == "zero":
                y[lo:hi] = 0.0
            else:
                y[lo + (hi - lo) // 2] = np.nan if what == "nan" else np.inf
            nv, cv, nnz, out, rec = _encode(y, kind, levels, B, p=p)
            keep = np.ones(n, dtype=bool)
            keep[lo:hi] = False
            kn = np.ones(len(nv), dtype=bool)
            kn[b] = False
            assert np.array_equal(nv[kn].view(np.uint32), base[0][kn].view(np.uint32))
            codes, codes0 = br.unpack(cv, n, bits), br.unpack(base[1], n, bits)
            assert np.array_equal(codes[keep], codes0[keep])
            assert np.array_equal(out[keep].view(np.uint32), base[3][keep].view(np.uint32))
            assert np.isnan(nv[b]) if what == "nan" else nv[b] == (np.inf if what == "inf" else 0.0)
            assert np.array_equal(codes[lo:hi], (y[lo:hi] != 0).astype(np.uint32))  # code 0 for x == 0, code 1 otherwise
            dec = _codec().bucket_decode(rec, n, kind, levels, bits, B).cpu().numpy()
            assert gc.same_bits(dec, out)
            zero = y[lo:hi] == 0
            assert np.array_equal(dec[lo:hi][zero].view(np.uint32), np.zeros(int(zero.sum()), dtype=np.uint32))
            assert np.isnan(dec[lo:hi][~zero]).all()


# ------------------------------------------------------------------------------------- decode and round forms
@pytest.mark.parametrize("n,B", [(1, 64), (65, 64), (4097, 512), (12345, 4096)])
@pytest.mark.parametrize("kind", [STD, NATD])
def test_decode_equals_the_model(n, B, kind):
    codec = _codec()
    x = _normal(n, seed=8)
    prev = _normal(n, seed=9)
    for bits, levels in FORMATS:
        nv, cv, _, out, rec = _encode(x, kind, levels, B)
        v = br.decode(br.unpack(cv, n, bits), kind, levels, B, nv)
        assert gc.same_bits(out, v)
        assert gc.same_bits(codec.bucket_decode(rec, n, kind, levels, bits, B).cpu().numpy(), v)
        w = np.float32(-0.375)
        assert gc.same_bits(codec.bucket_decode(rec, n, kind, levels, bits, B, weight=float(w)).cpu().numpy(), w * v)
        for wt in (np.float32(1.0), np.float32(0.3)):
            acc = _dev(prev).clone()
            codec.bucket_decode(rec, n, kind, levels, bits, B, out=acc, weight=float(wt), accumulate=True)
            want = (wt.astype(np.float64) * v.astype(np.float64) + prev.astype(np.float64)).astype(np.float32)  # fmaf
            assert gc.same_bits(acc.cpu().numpy(), want)


@pytest.mark.parametrize("C", [3, 70])
@pytest.mark.parametrize("n,B,kind,fmt,p", [(4097, 512, STD, FORMATS[2], INF), (1000, 64, NATD, FORMATS[1], L2),
                                             (8195, 4096, STD, FORMATS[0], L2)])
def test_round_equals_per_message_calls(C, n, B, kind, fmt, p):
    codec = _codec()
    bits, levels = fmt
    g = np.random.default_rng(C * 31 + n)
    X = (g.standard_normal((C, n)) * 1e-2).astype(np.float32)
    X[g.random((C, n)) < 0.05] = 0.0
    Xd = _dev(X)
    stride, _ = codec.bucket_wire_layout(n, kind, bits, B)
    seeds = [SEED + (c % 3) for c in range(C)]
    ctrs = [CTR + 5 * c for c in range(C)]
    recs = torch.full((C, stride), PAD, dtype=torch.uint8, device="cuda")
    counts = torch.full((C,), -12345, dtype=torch.int64, device="cuda")
    codec.bucket_encode_round([Xd[c] for c in range(C)], kind, levels, bits, B, p, seeds, ctrs,
                              [recs[c] for c in range(C)], counts=[counts[c:c + 1] for c in range(C)])
    each = torch.full((C, stride), PAD, dtype=torch.uint8, device="cuda")
    for c in range(C):
        _, nnz, _ = codec.bucket_encode(Xd[c], kind, levels, B, p, seeds[c], ctrs[c], record=each[c], want_nnz=True)
        assert int(nnz.item()) == int(counts[c].item()) == int(np.count_nonzero(X[c]))
    assert torch.equal(recs, each)
    assert not torch.equal(recs[0], recs[1])
    # counts == NULL, and slots that are not consecutive
    recs2 = torch.full((C, stride), PAD, dtype=torch.uint8, device="cuda")
    codec.bucket_encode_round([Xd[c] for c in range(C)], kind, levels, bits, B, p, seeds, ctrs,
                              [recs2[c] for c in range(C)])
    assert torch.equal(recs2, each)
    wide = torch.full((C, 2), -999, dtype=torch.int64, device="cuda")
    codec.bucket_encode_round([Xd[c] for c in range(C)], kind, levels, bits, B, p, seeds, ctrs,
                              [recs2[c] for c in range(C)], counts=[wide[c, 1:2] for c in range(C)])
    assert torch.equal(wide[:, 1], counts) and bool((wide[:, 0] == -999).all())


@pytest.mark.parametrize("n,B", [(65, 64), (4097, 512), (12345, 4096)])
def test_given_norms(n, B):
    x = _normal(n, seed=10)
    pn = np.array([np.max(np.abs(x[lo:hi])) for lo, hi in br.slices(n, B)], dtype=np.float32)
    given = (pn * np.float32(1.25)).astype(np.float32)  # (above the max: every y stays inside the level table)
    for kind in (STD, NATD):
        for bits, levels in FORMATS:
            got = _encode(x, kind, levels, B, norms=given)
            assert np.array_equal(got[0].view(np.uint32), given.view(np.uint32))
            _check_against_model(x, kind, levels, B, given, got)


def test_encode_without_optional_outputs_and_capture():
    """nnz and out are optional; the call captures into a graph and replays to the same bytes."""
    codec = _codec()
    n, B, kind, (bits, levels) = 12345, 512, STD, FORMATS[2]
    x = _dev(_normal(n))
    rec0, nnz0, out0 = codec.bucket_encode(x, kind, levels, B, np.inf, SEED, CTR, want_nnz=True, decode=True)
    rec1, nnz1, out1 = codec.bucket_encode(x, kind, levels, B, np.inf, SEED, CTR)
    assert nnz1 is None and out1 is None
    nv0, cv0 = codec.bucket_wire_views(rec0, n, kind, bits, B)
    nv1, cv1 = codec.bucket_wire_views(rec1, n, kind, bits, B)
    assert torch.equal(_bits(nv0), _bits(nv1)) and torch.equal(cv0, cv1)
    stride, _ = codec.bucket_wire_layout(n, kind, bits, B)
    rec2 = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            codec.bucket_encode(x, kind, levels, B, np.inf, SEED, CTR, record=rec2)
        g.replay()
    s.synchronize()
    nv2, cv2 = codec.bucket_wire_views(rec2, n, kind, bits, B)
    assert torch.equal(_bits(nv0), _bits(nv2)) and torch.equal(cv0, cv2)


# ------------------------------------------------------------------------------------- Compressor(bucket=B)
def _compressor(kind, s, p, B, rng="compat", seed=0):
    from fl_sim_amd import Compressor

    c = Compressor("q", rng=rng, seed=seed, bucket=B)
    nc = None
    if kind == "std":
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(s, nc, p=p)
    else:
        c.makeNaturalDitheringFP32(s, B, p=p)
    return c, nc


CASES = list(bucket_cases())


@pytest.fixture(scope="module")
def fixture():
    return np.load(f"{gc.GOLDEN}/bucket_codec.npz", allow_pickle=False)


@pytest.mark.parametrize("kind,s,p,B,n", CASES, ids=[bucket_key(*c) for c in CASES])
def test_compat_mode_reproduces_the_reference(kind, s, p, B, n, fixture):
    key = bucket_key(kind, s, p, B, n)
    x = fixture[f"x_n{n}"]
    stats = fixture[key + "|stats"]
    for device_input in (False, True):
        c, nc = _compressor(kind, s, p, B)
        random.seed(bucket_seed(kind, s, p, B, n))
        pos = c.philox.counter
        got = c.compressVector(_dev(x) if device_input else x)
        got = got.cpu().numpy() if device_input else got
        assert gc.same_bits(got, fixture[key + "|out"])
        assert c.really_need_to_send_components == stats[0] == c.last_need_to_send_advance
        assert c.total_input_components == stats[1] == n == c.last_input_advance
        if nc is not None:
            assert (nc.really_need_to_send_components, nc.total_input_components) == (stats[2], stats[3])
        assert random.random() == float(fixture[key + "|next_random"])  # the interpreter's stream position
        assert c.philox.counter == pos + 1  # one philox.next() per vector


@pytest.mark.parametrize("kind,s,p", [("std", 7, np.inf), ("natd", 8, 2)])
@pytest.mark.parametrize("B,n", [(64, 1000), (4096, 12345)])
def test_philox_mode_compressor(kind, s, p, B, n):
    import copy
    import pickle

    x = _normal(n, seed=11)
    c, nc = _compressor(kind, s, p, B, rng="philox", seed=99)
    twin = pickle.loads(pickle.dumps(c))
    assert twin.bucket == B and copy.deepcopy(c).bucket == B
    seed, ctr = twin.philox.next()
    out = c.compressVector(_dev(x)).cpu().numpy()
    k = STD if kind == "std" else NATD
    nv, _, nnz, want, _ = _encode(x, k, s, B, p=(INF if np.isinf(p) else L2), seed=seed, ctr=ctr)
    assert gc.same_bits(out, want)
    assert gc.same_bits(out, br.bucket_philox(x, k, s, B, nv, seed, ctr)[0])
    nb = -(-n // B)
    per = (1.0 + np.ceil(np.log2(s))) / 32.0
    assert c.last_input_advance == n == c.total_input_components
    assert c.really_need_to_send_components == (nb + nnz * per if kind == "std" else n * per)
    if nc is not None:
        assert nc.total_input_components == nb == nc.really_need_to_send_components


def test_bucket_zero_is_the_whole_vector_path():
    x = _normal(5000, seed=12)
    outs = []
    for kw in ({}, {"bucket": 0}):
        from fl_sim_amd import Compressor

        c = Compressor("q", **kw)
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(8, nc)
        random.seed(4)
        outs.append(c.compressVector(x))
    random.seed(4)
    want, _, _ = ref.standard_dithering(x, 8, np.inf, ref.python_random_stream())
    assert gc.same_bits(outs[0], want) and gc.same_bits(outs[1], want)


def test_bucket_errors():
    from fl_sim_amd import Compressor

    for bad in (32, 96, 8192, -64):
        with pytest.raises(ValueError, match="bucket"):
            Compressor("q", bucket=bad)
    c, _ = _compressor("std", 7, np.inf, 64)
    with pytest.raises(ValueError, match="float32"):
        c.compressVector(np.zeros(100, dtype=np.float64))
    c.bucket = 100
    with pytest.raises(ValueError, match="bucket"):
        c.compressVector(np.ones(100, dtype=np.float32))
    nat = Compressor("n")
    nat.makeNaturalCompressorFP32()
    c = Compressor("q", bucket=64)
    c.makeStandardDitheringFP32(7, nat)
    with pytest.raises(ValueError, match="identical"):
        c.compressVector(np.ones(100, dtype=np.float32))
