"""The decoder model of tests/decode_cases.py against the reference's own arithmetic (the oracle's ref.dither /
ref.dither64, ref.natural / ref.natural64, ref.stacked and ref.topk): codes formed from what the oracle chose, exactly
as include/flcodec.h lays the wire out, packed, decoded by the model, and compared with the oracle's own decoded
vector bit for bit — no tolerance.  Plus the invariants of the stream builders and the coverage of the code tables that
tests/test_gpu_decode_edges.py runs the kernels on.

Norms: the oracle (like the reference) has no level bracket under a norm of 0 below nonzero elements and raises; a
negative norm cannot come out of a norm.  For both, the codec's contract (code 0 -> +0, any other code -> NaN) is the
header's, and the model states it; the norms the oracle does evaluate (inf and NaN) anchor it here."""

import numpy as np
import pytest

from oracle import compressors_ref as ref
from tests import decode_cases as dc
from tests import golden_cases as gc
from tests import golden_f64

F32, F64 = np.float32, np.float64
BITS_LEVELS = [(2, [1]), (4, list(range(1, 8))), (8, list(range(1, 128)))]


def _dither_input(s, norm, dtype, g, n=192):
    """Elements over (0, norm] of both signs with every level value times the norm, +-0, the norm itself and values so
    small that level 0 is chosen under a set sign bit among them."""
    x = (g.random(n) * 2 - 1) * norm
    lv = ref.standard_levels(s)
    x[: len(lv[:40])] = lv[:40] * norm * np.where(np.arange(len(lv[:40])) % 2, -1, 1)
    x[40:44] = [0.0, -0.0, norm, -norm]
    x[44:48] = [norm * 1e-6, -norm * 1e-6, norm * 2.0**-20, -norm * 2.0**-20]
    return x.astype(dtype)


def _wire_codes(x, lvl_idx, bits, regular):
    """sign << (bits - 1) | level; a row whose norm is not finite: code 0 for x == 0 and code 1 otherwise."""
    if not regular:
        return (x != 0).astype(np.uint8)
    return ((lvl_idx | (np.signbit(x).astype(np.int64) << (bits - 1))) * (x != 0)).astype(np.uint8)


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind", [dc.STD, dc.NAT], ids=["standard", "natural"])
@pytest.mark.parametrize("bits,levels", BITS_LEVELS, ids=["b2", "b4", "b8"])
def test_dithering_codes_decode_to_the_oracles_vector(bits, levels, kind, dtype):
    g = np.random.default_rng(100 * bits + 10 * kind + (dtype is F64))
    seen_top = set()
    for s in levels:
        lv = dc.level_table(kind, s)
        for norm in (0.37, 2.3e-3, 1.0, float("inf"), float("nan")):
            regular = np.isfinite(norm)
            x = _dither_input(s, norm if regular else 1.0, dtype, g)
            pn = dtype(np.abs(x).max()) if regular else dtype(norm)
            u = g.random(len(x))
            with np.errstate(all="ignore"):
                out, _, _, lvl_idx = (ref.dither64 if dtype is F64 else ref.dither)(x, lv, pn, lambda i: u[i])
            codes = _wire_codes(x, lvl_idx, bits, regular)
            if regular and (lvl_idx == s).any():
                seen_top.add(s)
            wire = dc.unpack(dc.pack(codes, bits), len(x), bits)
            assert np.array_equal(wire, codes)
            if dtype is F64:
                got = dc.quant_values64(wire, kind, s, pn, bits)
                assert golden_f64.same_bits(got, out), (s, norm)
            else:
                got = dc.quant_values(wire, kind, s, bits, pn)
                assert gc.same_bits(got, out), (s, norm)
            if not regular:
                assert np.isnan(got[x != 0]).all() and not got[x == 0].view(np.uint8).any()
    assert seen_top == set(levels)  # (every table's pinned top level was decoded)


def _natural_code(out, bias):
    """0 = zero, 0x7fff = NaN, else sign << 15 | (e + bias) for the power of two 2^e the oracle chose."""
    m, e = np.frexp(np.where(np.isnan(out) | (out == 0), 1.0, np.abs(out).astype(F64)))
    assert np.all(m == 0.5)
    code = (np.signbit(out).astype(np.int64) << 15) | (e - 1 + bias)
    return np.where(np.isnan(out), 0x7FFF, np.where(out == 0, 0, code)).astype(np.uint16)


def test_natural_codes_decode_to_the_oracles_vector():
    """Every binade of fp32 (denormals included) rounded down and rounded up, +-0, +-inf and NaN.  (The top binade is
    only rounded down: 2^128 is no fp32 power of two, so it has no field in 1..277.)"""
    g = np.random.default_rng(5)
    e = np.repeat(np.arange(-149, 128), 4)
    m = 1.0 + np.where(np.arange(len(e)) % 4 < 2, 0.0, g.random(len(e)))
    x = (np.ldexp(m, e) * np.where(np.arange(len(e)) % 2, -1, 1)).astype(F32)
    u = np.where(np.arange(len(e)) % 4 == 2, 0.0, 1.0 - 2.0**-53)  # (u = 0 rounds down, u just below 1 rounds up)
    u[e == 127] = 0.0
    x = np.concatenate([x, np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=F32)])
    u = np.concatenate([u, np.zeros(5)])
    with np.errstate(all="ignore"):
        out, _, _ = ref.natural(x, lambda i: u[i])
    codes = _natural_code(out, 150)
    assert gc.same_bits(dc.natural_values(codes), out)
    fields = set((codes[(codes != 0) & (codes != 0x7FFF)] & 0x7FFF).tolist())
    assert fields == set(range(1, 278)) and 0x7FFF in codes and 0 in codes
    mag = np.abs(out[np.abs(out) > 0])
    assert mag.min() == F32(2.0**-149) and mag.max() == F32(2.0**127)


def test_natural64_codes_decode_to_the_oracles_vector():
    """The float64 form over every binade of fp64.  (No inf or NaN input: the reference's math.floor raises on them.)"""
    g = np.random.default_rng(6)
    e = np.repeat(np.arange(-1074, 1024), 2)
    m = 1.0 + np.where(np.arange(len(e)) % 2 == 0, 0.0, g.random(len(e)))
    x = np.ldexp(m, e) * np.where(np.arange(len(e)) % 4 < 2, -1.0, 1.0)
    u = np.where(g.random(len(e)) < 0.5, 0.0, 1.0 - 2.0**-53)
    u[e == 1023] = 0.0
    x = np.concatenate([x, [0.0, -0.0]])
    u = np.concatenate([u, np.zeros(2)])
    with np.errstate(over="ignore"):  # (2^1024 in the top binade's pt)
        out, _, _ = ref.natural64(x, lambda i: u[i])
    codes = _natural_code(out, 1075)
    assert golden_f64.same_bits(dc.natural_values64(codes), out)
    fields = set((codes[codes != 0] & 0x7FFF).tolist())
    assert fields == set(range(1, 2099))
    assert golden_f64.same_bits(dc.natural_values64(np.array([0x7FFF, 0])), np.array([np.nan, 0.0]))


@pytest.mark.parametrize("s", dc.LEVELS)
@pytest.mark.parametrize("n,k", [(5, 2), (1025, 64), (4097, 1365)])
def test_stacked_and_topk_streams_decode_to_the_oracles_vector(n, k, s):
    g = np.random.default_rng(n + s)
    x = (g.standard_normal(n) * 1e-2).astype(F32)
    x[::7] = 0.0
    x[1::50] = -0.0
    u = g.random(n)
    out, kept, codes, pn = ref.stacked(x, k, s, lambda i: u[i])
    assert gc.same_bits(dc.stacked_dense(n, kept, codes, s, pn), out)
    xs = x.copy()
    xs[3] = np.inf  # (an infinite norm: every kept nonzero value decodes to NaN; the wire's code there is 1)
    with np.errstate(all="ignore"):
        out, kept, codes, pn = ref.stacked(xs, k, s, lambda i: u[i])
    assert np.isinf(pn)
    codes = (xs[kept] != 0).astype(np.uint8)
    assert gc.same_bits(dc.stacked_dense(n, kept, codes, s, pn), out)
    out, _ = ref.topk(x, k)
    idx, val = ref.topk_kept(x, k)
    assert gc.same_bits(dc.sparse_dense(n, idx, val), out)
    S = np.sort(g.choice(n, size=k, replace=False))
    out, _ = ref.randk(x, k, n, S)
    assert gc.same_bits(dc.sparse_dense(n, S, x[S], dc.scale_dk(n, k)), out)


# ------------------------------------------------------------------------------------------------ the builders
def test_streams_are_well_formed_and_meet_their_labels():
    seen = {}
    for n, idx, label in dc.all_streams() + [dc.large_stream()]:
        k = len(idx)
        seen.setdefault(n, set()).add(label)
        assert idx.dtype == np.int64 and (k == 0 or (idx[0] >= 0 and idx[-1] < n)), (n, label)
        assert np.all(np.diff(idx) > 0), (n, label)
        tiles = dc.tile_pointers(idx, n).astype(np.int64)
        ntiles = -(-n // dc.TILE)
        assert len(tiles) == ntiles + 1 and tiles[0] == 0 and tiles[-1] == k and np.all(np.diff(tiles) >= 0)
        for t in range(ntiles):  # (the pointers are the stream's own)
            assert np.all(idx[tiles[t]:tiles[t + 1]] // dc.TILE == t)
        per = np.diff(tiles)
        if label == "k0":
            assert k == 0
        elif label == "first":
            assert idx.tolist() == [0]
        elif label == "last":
            assert idx.tolist() == [n - 1]
        elif label == "edges":
            assert k == 2 * ((n - 1) // dc.TILE) and set((idx % dc.TILE).tolist()) == {0, dc.TILE - 1}
        elif label.startswith("tile"):
            c = int(label[4:])
            t = int(np.flatnonzero(per)[0])
            assert per[t] == c == k and idx[0] == t * dc.TILE and (c == 1 or idx[-1] == min(n, (t + 1) * dc.TILE) - 1)
        elif label == "pair":
            t = int(np.flatnonzero(per)[0])
            assert t % 2 == 0 and per[t] == per[t + 1] == dc.TILE and k == 2 * dc.TILE
        elif label == "lasttile":
            assert per[-1] == k == n - (ntiles - 1) * dc.TILE and ntiles >= 2
        elif label == "full":
            assert k == n
        elif label == "p1":
            assert k == n // 100 > 0
        elif label == "p33":
            assert k == n // 3 > 0
        else:
            raise AssertionError(label)
    assert sorted(seen) == sorted(dc.SIZES + [dc.LARGE_N])
    assert {n % 4 for n in dc.SIZES} == {0, 1, 2, 3}
    every = {"k0", "first", "last", "edges", "pair", "lasttile", "full", "p1", "p33"} | {f"tile{c}" for c in dc.TILE_COUNTS}
    for n in (2049, 3073, 4097, 5 * 1024 + 3, 70_001):
        assert seen[n] == every, n
    assert seen[1] == {"k0", "first", "last", "full"} and "tile1024" in seen[1024] and "tile1024" in seen[2048]
    assert {-(-n // dc.TILE) % 2 for n in dc.SIZES} == {0, 1}  # (odd counts: the last wave's second tile is absent)


def test_the_code_tables_cover_every_valid_code():
    table = dc.quant_codes(127, 8)
    assert sorted(table.tolist()) == list(range(256))  # (levels = 127: every byte is valid)
    for s in dc.LEVELS:
        t = dc.stacked_codes(2 * (s + 1), s, start=3)
        assert sorted(t.tolist()) == sorted(list(range(s + 1)) + [128 + i for i in range(s + 1)])
        assert 128 in t.tolist() and s in t.tolist() and (128 | s) in t.tolist()  # (sign with level 0; the top level)
    nat = dc.natural_codes()
    assert len(nat) == len(set(nat.tolist())) == 2 * 277 + 2
    v = dc.natural_values(nat)
    assert np.isnan(v).sum() == 1 and (v == 0).sum() == 1 and len(set(v[np.isfinite(v)].tolist())) == 2 * 277 + 1
    assert len(dc.natural_codes(dc.NAT_FIELDS64)) == 2 * 2098 + 2
    for s in (49, 98, 103, 107):  # (the pin is visible in fp64 and only there)
        assert s * (1.0 / s) != 1.0 and F32(s * (1.0 / s)) == F32(1.0)
        top = dc.quant_values64(np.array([s, 128 | s]), dc.STD, s, 1.0)
        assert top.tolist() == [1.0, -1.0]
        assert dc.quant_values(np.array([s, 128 | s]), dc.STD, s, 8, 1.0).tolist() == [1.0, -1.0]
    for s in range(1, 128):
        assert {s, 128 | s} <= set(dc.quant_codes(s, 8).tolist())


def test_value_edges_and_weights_are_the_listed_ones():
    v = dc.sparse_values(200, 0)
    assert np.isnan(v).any() and np.isinf(v).any() and (np.abs(v) == F32(dc.FLT_MAX)).sum() >= 2
    assert (v.view(np.uint32) == 0x80000000).any() and (v.view(np.uint32) == 0).any()
    assert ((v != 0) & (np.abs(v) < np.finfo(F32).tiny)).any()
    assert {len(dc.sparse_values(1, r)) for r in range(13)} == {1}
    assert sum(not np.isfinite(dc.sparse_values(1, r)[0]) or dc.sparse_values(1, r)[0] == 0 for r in range(13)) >= 5
    a = dc.seed_acc(4097, 3)
    assert np.isnan(a).any() and np.isinf(a).any() and (a.view(np.uint32) == 0x80000000).any()
    assert len(dc.WEIGHTS) == 8 and len(dc.NORMS) == 8 and dc.SCALES[1] != 1.0
    m, _ = np.frexp(dc.SCALES[1])
    assert m != 0.5  # (not a power of two)


def test_pack_is_little_endian_within_a_byte():
    codes = np.array([1, 2, 3, 0, 3, 1, 2], dtype=np.uint8)
    assert dc.pack(codes, 2).tolist() == [1 | 2 << 2 | 3 << 4 | 0 << 6, 3 | 1 << 2 | 2 << 4]
    assert dc.pack(np.array([0xA, 0x3, 0xF]), 4).tolist() == [0x3A, 0x0F]
    assert dc.pack(np.array([200, 7]), 8).tolist() == [200, 7]
    g = np.random.default_rng(0)
    for bits in (2, 4, 8):
        for n in (1, 7, 8, 9, 1023):
            c = g.integers(0, 1 << bits, n).astype(np.uint8)
            p = dc.pack(c, bits)
            assert len(p) == -(-n * bits // 8)
            assert np.array_equal(np.unpackbits(p, bitorder="little")[: n * bits].reshape(n, bits)
                                  @ (1 << np.arange(bits)), c)
            assert np.array_equal(dc.unpack(p, n, bits), c)


def test_the_output_rule_takes_the_unkept_positions_too():
    dense = dc.sparse_dense(5, [1, 3], [2.0, -0.0])
    assert dc.weighted(dense, 1.0, False).view(np.uint32).tolist() == dense.view(np.uint32).tolist()
    assert dc.weighted(dense, -1.5, False).view(np.uint32).tolist() == [0x80000000, 0xC0400000, 0x80000000, 0, 0x80000000]
    assert np.isnan(dc.weighted(dense, float("inf"), False)[[0, 2, 3, 4]]).all()
    acc = np.array([-0.0, 1.0, -0.0, -0.0, np.inf], dtype=F32)
    got = dc.weighted(dense, -1.0, True, acc)  # fma(-1, +0, -0) = -0 + -0 = -0; fma(-1, -0, -0) = +0 + -0 = +0
    assert got.view(np.uint32).tolist() == [0x80000000, 0xBF800000, 0x80000000, 0, 0x7F800000]
    v = np.array([[1.0, -0.0], [0.5, 2.0]], dtype=F32)
    assert dc.row_weighted(v, None, False).tolist() == v.tolist()
    assert dc.row_weighted(v, np.array([1.0, -2.0]), False).tolist() == [[1.0, -0.0], [-1.0, -4.0]]
    assert dc.row_weighted(v, None, True, np.ones((2, 2), dtype=F32)).tolist() == [[2.0, 1.0], [1.5, 3.0]]
