"""Decision-edge parity tests of the dithering and natural quantizers (gfx950).  Every input of tests/quant_cases.py
puts its elements where the per-element decision "lower level iff u < p" can go wrong: p a margin's width from the
element's own Philox uniform, y = |x| / norm a margin's width from a level, norms from a subnormal to FLT_MAX (where
fp32(s / norm) overflows or is subnormal), pt == u in the natural compressor, FLT_MAX overflowing to +-inf, non-finite
and degenerate rows, and the doubles around every power of two where log2 may round onto the integer.  Everything is
compared bit for bit (any NaN equals any NaN) with oracle/compressors_ref.py; codes and counts as integers."""

import functools
import math

import numpy as np
import pytest
import torch

from oracle import compressors_ref as ref
from tests import golden_cases as gc
from tests import golden_f64 as g64
from tests import quant_cases as qc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, CTR = 11, 5
SHAPES = ((2, 16384), (3, 16389))  # whole groups / groups straddling rows (per-element path, a norm per row)
STD, NAT = 0, 1


def _codec():
    from fl_sim_amd import codec

    return codec


def _levels(kind, s):
    return ref.standard_levels(s) if kind == STD else ref.natural_levels(s)


def _unpack(codes, n, bits):
    """Element i of the flat batch sits at bit offset i * bits of the code stream (little-endian within a byte)."""
    c = codes.cpu().numpy()
    i = np.arange(n)
    per = 8 // bits
    return (c[i // per] >> ((i % per) * bits).astype(np.uint8)) & np.uint8((1 << bits) - 1)


def _row_norms(rows, norm):
    """Shape 1: the case's norm on both rows; shape 2: the case's norm in the middle, 1.0 and 3.1e-3 outside."""
    return [norm, norm] if rows == 2 else [np.float32(1.0), norm, np.float32(3.1e-3)]


@functools.lru_cache(maxsize=None)
def _dense_case(kind, s, ni, rows, d):
    """(x [rows, d], norms [rows], expected decode, expected codes (flat, unpacked), expected nnz [rows])."""
    norm = (qc.NORMS32 if kind == STD else qc.NORMS_NAT32)[ni]
    norms = np.array(_row_norms(rows, norm), dtype=np.float32)
    g = np.random.default_rng(100_000 * kind + 1000 * s + 10 * ni + rows)
    lv = _levels(kind, s)
    bits = _codec().code_bits(s)
    x = np.empty((rows, d), dtype=np.float32)
    out = np.empty((rows, d), dtype=np.float32)
    codes = np.empty((rows, d), dtype=np.uint8)
    nnz = []
    for r in range(rows):
        at = np.arange(r * d, (r + 1) * d)
        if kind == STD:
            x[r] = qc.std_edge_case(s, norms[r], d, SEED, CTR, g, at=at)
        else:
            x[r] = qc.nat_dither_edge_case(s, norms[r], d, SEED, CTR, g, at=at)
        u = ref.philox_uniforms_at(at, SEED, CTR)
        out[r], nz, _, li = ref.dither(x[r], lv, norms[r], lambda i: u[i])
        codes[r] = np.where(x[r] != 0, li | (np.signbit(x[r]).astype(np.int64) << (bits - 1)), 0)
        nnz.append(nz)
    assert np.array_equal(np.abs(x).max(axis=1), norms)
    return x, norms, out, codes.reshape(-1), np.array(nnz, dtype=np.int64)


def _check_packet(pkt, out, case, tag, with_nnz=True):
    x, norms, exp_out, exp_codes, exp_nnz = case
    got = _unpack(pkt.codes, x.size, pkt.bits)
    bad = np.flatnonzero(got != exp_codes)
    assert bad.size == 0, (tag, "codes", bad.size, [(int(i), float(x.reshape(-1)[i]), int(got[i]), int(exp_codes[i]))
                                                   for i in bad[:5]])
    assert gc.same_bits(out.cpu().numpy(), exp_out), (tag, "decode")
    if with_nnz:
        assert np.array_equal(pkt.nnz.cpu().numpy(), exp_nnz), (tag, "nnz")


def _run_dense(kind, s, ni):
    codec = _codec()
    for rows, d in SHAPES:
        case = _dense_case(kind, s, ni, rows, d)
        x, norms = case[0], case[1]
        tag = (kind, s, float(norms[rows // 2]), rows, d)
        xd, nd = torch.from_numpy(x).to(DEV), torch.from_numpy(norms).to(DEV)
        pkt = codec.quant_encode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
        _check_packet(pkt, codec.quant_decode(pkt), case, tag + ("encode + decode",))
        pkt2, out2 = codec.quant_encode_decode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
        _check_packet(pkt2, out2, case, tag + ("encode_decode",))
        # the norm included (one launch at these shapes): x[r, 0] = +-norm makes every given norm the row's max |x|
        pkt3, out3 = codec.quant_encode_auto(xd, kind, s, math.inf, SEED, CTR, want_nnz=True)
        assert np.array_equal(pkt3.norms.cpu().numpy().view(np.uint32), norms.view(np.uint32)), tag
        _check_packet(pkt3, out3, case, tag + ("encode_auto",))
        pkt4, _ = codec.quant_encode_auto(xd, kind, s, math.inf, SEED, CTR, want_nnz=False, decode=False)
        assert torch.equal(pkt4.codes, pkt3.codes), tag
    assert codec.quant_status() == 0


@pytest.mark.parametrize("ni", range(len(qc.NORMS32)), ids=[f"{v:.8g}" for v in qc.NORMS32])
@pytest.mark.parametrize("s", qc.LEVELS_STD)
def test_standard_dithering_on_its_decision_edges(s, ni):
    """Dense standard dithering, given norms and the one-launch form, over LEVELS_STD x NORMS32 at both shapes."""
    _run_dense(STD, s, ni)


@pytest.mark.parametrize("ni", range(len(qc.NORMS_NAT32)), ids=[f"{v:.8g}" for v in qc.NORMS_NAT32])
@pytest.mark.parametrize("s", qc.LEVELS_NAT)
def test_natural_dithering_on_its_decision_edges(s, ni):
    _run_dense(NAT, s, ni)


# ------------------------------------------------------------------------------------------------- stacked encoder
N_ST, K_ST = 70_001, 7_000
NORMS_ST = tuple(np.float32(v) for v in (1.0, 3.1e-3, 3e-42, 3.7e-37, 3.8e-37, 3.4028235e38))


@functools.lru_cache(maxsize=None)
def _stacked_case(s, ni, seed, counter):
    """k edge elements at k random positions, built from the uniforms of those positions; every other element 0.
    (The select keeps the largest signed values, so the edge elements are taken positive.)"""
    g = np.random.default_rng(7000 + 10 * s + ni)
    pos = np.sort(g.choice(N_ST, K_ST, replace=False))
    x = np.zeros(N_ST, dtype=np.float32)
    x[pos] = np.abs(qc.std_edge_case(s, NORMS_ST[ni], K_ST, seed, counter, g, at=pos))
    exp = ref.stacked(x, K_ST, s, lambda i: ref.philox_uniforms_at(i, seed, counter), fast=True)
    assert exp[3] == NORMS_ST[ni]
    return x, exp


def _check_stacked(pkt, exp, tag, decode=True):
    codec = _codec()
    exp_out, exp_idx, exp_codes, pn = exp
    k = len(exp_idx)
    assert np.array_equal(pkt.idx.cpu().numpy().astype(np.int64), exp_idx), (tag, "kept index set / order")
    got = pkt.codes[:k].cpu().numpy()
    bad = np.flatnonzero(got != exp_codes)
    assert bad.size == 0, (tag, "codes", bad.size, [(int(exp_idx[i]), int(got[i]), int(exp_codes[i])) for i in bad[:5]])
    assert gc.same_bits(pkt.norm.cpu().numpy().reshape(1), np.array([pn], dtype=np.float32)), tag
    t = pkt.tiles.cpu().numpy().astype(np.int64)
    assert t[-1] == k and np.array_equal(t[:-1], np.searchsorted(exp_idx, np.arange(len(t) - 1) * codec.TILE)), tag
    if decode:
        assert gc.same_bits(codec.stacked_decode(pkt).cpu().numpy(), exp_out), (tag, "decode")


@pytest.mark.parametrize("ni", range(len(NORMS_ST)), ids=[f"{v:.8g}" for v in NORMS_ST])
@pytest.mark.parametrize("s", (1, 3, 7, 127))
def test_stacked_encode_on_the_dithering_edges(s, ni):
    codec = _codec()
    x, exp = _stacked_case(s, ni, SEED, CTR)
    pkt = codec.stacked_encode(torch.from_numpy(x).to(DEV), K_ST, s, seed=SEED, counter=CTR)
    _check_stacked(pkt, exp, (s, float(NORMS_ST[ni])))
    assert codec.topk_status(reset=True) == 0


def test_stacked_batch_and_delta_encoders_on_the_dithering_edges():
    """One batched encode of three clients with different norms, seeds and counters, and one delta encode against a
    zero global model (three tensors): each packet the oracle's."""
    codec = _codec()
    s = 127
    clients = [(0, 21, 100), (2, 22, 107), (4, 23, 114)]  # (norm index, seed, counter)
    cases = [_stacked_case(s, ni, seed, ctr) for ni, seed, ctr in clients]
    xs = [torch.from_numpy(c[0]).to(DEV) for c in cases]
    pks = codec.stacked_encode_batch(xs, K_ST, s, seeds=[c[1] for c in clients], counters=[c[2] for c in clients])
    assert codec.topk_status(reset=True) == 0
    for c, (case, cl) in enumerate(zip(cases, clients)):
        _check_stacked(pks[c], case[1], ("batch", c, float(NORMS_ST[cl[0]])))
    x, exp = _stacked_case(s, 5, SEED, CTR)
    cuts = [0, N_ST // 3 + 1, 2 * N_ST // 3 + 2, N_ST]
    local = [torch.from_numpy(x[a:b].copy()).to(DEV) for a, b in zip(cuts, cuts[1:])]
    pkt = codec.stacked_encode_delta(local, [torch.zeros_like(t) for t in local], K_ST, s, seed=SEED, counter=CTR)
    _check_stacked(pkt, exp, ("delta", float(NORMS_ST[5])), decode=False)
    assert codec.topk_status(reset=True) == 0


# --------------------------------------------------------------------------------------------- natural compressor
def test_natural_compressor_on_its_decision_edges():
    """pt = u to the last mantissa bit (pt == u exactly: the upper power), every exponent from 2^-149 to FLT_MAX,
    whose upper power is +-inf."""
    codec = _codec()
    n = 65_543
    x, tie = qc.natural_edge_case(n, SEED, CTR, np.random.default_rng(3))
    u = ref.philox_uniforms(n, SEED, CTR)
    with np.errstate(over="ignore"):
        exp, _, nz = ref.natural(x, lambda i: u[i])
    assert int(tie.sum()) >= 20 and np.isposinf(exp).any() and np.isneginf(exp).any()
    codes, nnz = codec.natural_encode(torch.from_numpy(x).to(DEV), SEED, CTR)
    out = codec.natural_decode(codes, n).cpu().numpy()
    bad = np.flatnonzero(out.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, (bad.size, [(int(i), float(x[i]), float(out[i]), float(exp[i])) for i in bad[:5]])
    assert int(nnz.item()) == nz


# --------------------------------------------------------------------------- non-finite and degenerate rows
D_ROW = 16389


@functools.lru_cache(maxsize=None)
def _odd_rows():
    g = np.random.default_rng(17)
    x = (g.standard_normal((5, D_ROW)) * 1e-3).astype(np.float32)
    x[g.random(x.shape) < 0.05] = 0
    x[:, 3] = -0.0
    x[0, 77] = np.nan
    x[1, 5] = np.inf
    x[2, D_ROW - 1] = -np.inf
    x[3, :] = 0
    x[3, 1::2] = -0.0
    return x


def _expect_row(x, lv, norm, u):
    """ref.dither with that norm.  A norm of 0 or below 0 under nonzero elements leaves compressors.py:346-354 without
    a bracket (y = inf, y < 0: the reference indexes past its table and raises, ref.dither likewise at 0); the codec's
    contract for every norm that is not a finite positive number (include/flcodec.h) is code 1 -> NaN on the nonzero
    elements, +0 on the zeros, and that is what is expected there."""
    if norm > 0 or np.isnan(norm) or not (x != 0).any():
        with np.errstate(all="ignore"):
            out, nz, _, _ = ref.dither(x, lv, np.float32(norm), lambda i: u[i])
        return out, nz
    if norm == 0:
        with pytest.raises(IndexError):
            ref.dither(x, lv, np.float32(norm), lambda i: u[i])
    out = np.where(x != 0, np.float32(np.nan), np.float32(0)).astype(np.float32)
    return out, int((x != 0).sum())


@pytest.mark.parametrize("kind,s", [(STD, 127), (STD, 3), (NAT, 8)])
def test_non_finite_and_zero_rows_against_the_oracle(kind, s):
    """Rows with one NaN, one +inf, one -inf, all zeros (of both signs) and an ordinary row, p = inf: the norm of each
    row, then ref.dither with it — zeros decode to +0, every other element of a non-finite row to NaN."""
    codec = _codec()
    x = _odd_rows()
    rows, d = x.shape
    lv = _levels(kind, s)
    with np.errstate(invalid="ignore"):
        norms = np.abs(x).max(axis=1)
    assert np.isnan(norms[0]) and np.isinf(norms[1]) and np.isinf(norms[2]) and norms[3] == 0 and norms[4] > 0
    exp, exp_nnz = np.empty_like(x), []
    for r in range(rows):
        u = ref.philox_uniforms_at(np.arange(r * d, (r + 1) * d), SEED, CTR)
        exp[r], nz = _expect_row(x[r], lv, norms[r], u)
        exp_nnz.append(nz)
    for r in range(3):
        assert np.isnan(exp[r][x[r] != 0]).all() and (exp[r][x[r] == 0].view(np.uint32) == 0).all()
    assert (exp[3].view(np.uint32) == 0).all()
    xd = torch.from_numpy(x).to(DEV)
    nd = codec.quant_norm(xd, math.inf)
    assert gc.same_bits(nd.cpu().numpy(), norms)
    pkt = codec.quant_encode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
    pkt2, out2 = codec.quant_encode_decode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
    pkt3, out3 = codec.quant_encode_auto(xd, kind, s, math.inf, SEED, CTR, want_nnz=True)
    assert gc.same_bits(pkt3.norms.cpu().numpy(), norms)
    for tag, p, o in (("encode", pkt, codec.quant_decode(pkt)), ("encode_decode", pkt2, out2), ("auto", pkt3, out3)):
        assert gc.same_bits(o.cpu().numpy(), exp), tag
        assert np.array_equal(p.nnz.cpu().numpy(), np.array(exp_nnz)), tag
    assert codec.quant_status() == 0


@pytest.mark.parametrize("norm", [0.0, float("inf"), float("nan"), -1.0])
@pytest.mark.parametrize("kind,s", [(STD, 127), (NAT, 8)])
def test_rows_with_an_irregular_norm_given(kind, s, norm):
    """A norm passed as 0, inf, NaN or -1 to the middle row of three (groups straddle the rows)."""
    codec = _codec()
    x = _odd_rows()[[4, 4, 4]].copy()
    x[1] = -x[1][::-1]
    rows, d = x.shape
    norms = np.abs(x).max(axis=1)
    norms[1] = norm
    lv = _levels(kind, s)
    exp, exp_nnz = np.empty_like(x), []
    for r in range(rows):
        u = ref.philox_uniforms_at(np.arange(r * d, (r + 1) * d), SEED, CTR)
        exp[r], nz = _expect_row(x[r], lv, norms[r], u)
        exp_nnz.append(nz)
    assert np.isnan(exp[1][x[1] != 0]).all() and (exp[1][x[1] == 0].view(np.uint32) == 0).all()
    xd, nd = torch.from_numpy(x).to(DEV), torch.from_numpy(norms).to(DEV)
    pkt = codec.quant_encode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
    pkt2, out2 = codec.quant_encode_decode(xd, kind, s, nd, SEED, CTR, None, want_nnz=True)
    for tag, p, o in (("encode", pkt, codec.quant_decode(pkt)), ("encode_decode", pkt2, out2)):
        assert gc.same_bits(o.cpu().numpy(), exp), tag
        assert np.array_equal(p.nnz.cpu().numpy(), np.array(exp_nnz)), tag


# ---------------------------------------------------------------------------------------------------- float64
N64 = 65_543


@pytest.mark.parametrize("ni", range(len(qc.NORMS64)), ids=[f"{v:.8g}" for v in qc.NORMS64])
@pytest.mark.parametrize("s", (1, 3, 10, 127))
def test_standard_dithering_f64_on_its_decision_edges(s, ni):
    from fl_sim_amd._lib import FLC_Q_STANDARD_DITHER

    codec = _codec()
    norm = np.float64(qc.NORMS64[ni])
    x = qc.std_edge_case64(s, norm, N64, SEED, CTR, np.random.default_rng(64_000 + 10 * s + ni))
    assert np.abs(x).max() == norm
    exp, nz, _, li = ref.dither64(x, ref.standard_levels(s), norm, ref.philox_stream(SEED, CTR, N64))
    exp_codes = np.where(x != 0, li | (np.signbit(x).astype(np.int64) << 7), 0).astype(np.uint8)
    xd = torch.from_numpy(x).to(DEV)
    nd = torch.tensor([norm], dtype=torch.float64, device=DEV)
    codes, out, nnz = codec.quant_f64(xd, FLC_Q_STANDARD_DITHER, s, nd, seed=SEED, counter=CTR, want_codes=True,
                                      want_nnz=True)
    got = codes.cpu().numpy()
    bad = np.flatnonzero(got != exp_codes)
    assert bad.size == 0, (bad.size, [(int(i), float(x[i]), int(got[i]), int(exp_codes[i])) for i in bad[:5]])
    assert g64.same_bits(out.cpu().numpy(), exp)
    assert g64.same_bits(codec.quant_decode_f64(codes, N64, FLC_Q_STANDARD_DITHER, s, nd).cpu().numpy(), exp)
    assert int(nnz.item()) == nz


def test_natural_compressor_f64_on_its_decision_edges():
    codec = _codec()
    x, tie = qc.natural_edge_case64(N64, SEED, CTR, np.random.default_rng(4))
    with np.errstate(all="ignore"):  # (beside DBL_MAX 2^1024 is inf, and the reference's pt inf or NaN)
        exp, _, _ = ref.natural64(x, ref.philox_stream(SEED, CTR, N64))
    assert int(tie.sum()) >= 20 and np.isinf(exp).any()
    codes, out = codec.natural_f64(torch.from_numpy(x).to(DEV), seed=SEED, counter=CTR, want_codes=True)
    got = out.cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (bad.size, [(int(i), float(x[i]).hex(), float(got[i]), float(exp[i])) for i in bad[:5]])
    assert g64.same_bits(codec.natural_decode_f64(codes, N64).cpu().numpy(), exp)


@functools.lru_cache(maxsize=None)
def _near_pow2_oracle():
    x, u = qc.near_pow2_case64()
    with np.errstate(all="ignore"):  # (above 2^1023 the upper power is inf)
        exp, _, _ = ref.natural64(x, ref.compat_stream(lambda n: u[:n]))  # (no zero: every element draws, in order)
    return x, u, exp


def test_natural_f64_beside_the_powers_of_two():
    """natural64_code's log2 branch (mantissas within (|f| + 2) 2^-48 of 1 or 2) and both sides of its switch, under
    uniforms that make the result depend on whether log2 rounded onto the integer (u = 0, delta, 1 - 2^-53)."""
    host = qc.host_log2_survey()
    if not host["decides"]:
        pytest.skip("host math.log2 does not round as a correctly rounded log2 near powers of two: no oracle here")
    codec = _codec()
    x, u, exp = _near_pow2_oracle()
    assert np.all(x != 0)
    codes, out = codec.natural_f64(torch.from_numpy(x).to(DEV), compat_u=torch.from_numpy(u).to(DEV), want_codes=True)
    got = out.cpu().numpy()
    bad = np.flatnonzero(got.view(np.uint64) != exp.view(np.uint64))
    assert bad.size == 0, (bad.size, [(float(x[i]).hex(), float(u[i]), float(got[i]).hex(), float(exp[i]).hex())
                                      for i in bad[:8]])
    assert g64.same_bits(codec.natural_decode_f64(codes, x.size).cpu().numpy(), exp)


def test_error_words_are_clear_at_the_end():
    assert sum(_codec().topk_status_all().values()) == 0
