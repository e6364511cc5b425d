"""CPU anchors of tests/bucket_cases.py: what the bucket catalogue reaches and that its models say what the documents
say.  Every bucket of an edge message has the chosen norm as its max |x|; for every bucket size the float32 mirrors of
the two fast paths never contradict the oracle and leave elements on both sides of their margins; the p = 2 model is
exact on dyadic inputs, within one fp32 ulp of sqrt(fsum) on the general ones, does to the special buckets what
include/flcodec.h says, and tells the wave order apart on the tie bucket; a hand-built record decodes as
bucket_ref.decode says, holds every code, and keeps its padding."""

import math

import numpy as np
import pytest

from tests import bucket_cases as bc
from tests import bucket_ref as br
from tests import decode_cases as dc
from tests import golden_cases as gc
from tests import quant_cases as qc

F32, F64 = np.float32, np.float64
GROUP, LEVEL = (1e-4, 5e-5), (1e-4, 3e-5)  # shipped margins: quant.hip's group path, flc_device.hpp dither_level


# ------------------------------------------------------------------------------------------------ edge messages
@pytest.mark.parametrize("kind", [bc.STD, bc.NAT])
@pytest.mark.parametrize("B", bc.ALL_B)
def test_edge_message_shape(B, kind):
    table = bc.norms_of(kind)
    seen_tails = set()
    for i, s in enumerate(bc.levels_of(kind)):
        tail, rot = bc.rotation(kind, B, i)
        seen_tails.add(tail)
        x, norms, codes, out, nnz = bc.edge_message(kind, s, B, tail, rot)
        n = len(x)
        assert x.dtype == F32 and n >= 2 * bc.BLOCK + B and n <= 50_000 and n % B == bc.tail_len(tail, B)
        assert (tail != "six") or n % 4 == 2
        got = np.array([np.abs(x[lo:hi]).max() for lo, hi in br.slices(n, B)], dtype=F32)
        assert np.array_equal(got.view(np.uint32), norms.view(np.uint32))
        assert all(abs(x[lo]) == norms[b] for b, (lo, _) in enumerate(br.slices(n, B)))
        whole = norms[:n // B]
        assert {float(v) for v in table} == {float(v) for v in whole}  # every norm on a whole bucket
        assert nnz == int(np.count_nonzero(x)) and len(codes) == n == len(out)
        mask = (1 << (br.code_bits(s) - 1)) - 1
        assert int((codes & mask).max()) == s  # (x[lo] = +-norm sits on the top level)
    if kind == bc.STD:
        assert seen_tails == set(bc.TAILS)  # seven levels: each (B, tail) pair occurs


@pytest.mark.parametrize("B", bc.ALL_B)
def test_edge_messages_stand_on_both_sides_of_the_margins(B):
    """The claim of test_quant_cases.py for the dense catalogue, per bucket size: with the shipped margins neither
    mirror decides an element against the oracle; over the buckets where float32 leaves room (fp32(s / norm) finite
    for the group path, norm >= 2^-133 for dither_level) each decides >= 5 % of the nonzero elements itself and leaves
    >= 10 % to the exact rule; where fp32(s / norm) overflows the group path decides nothing."""
    for i, s in enumerate(qc.LEVELS_STD):
        tail, rot = bc.rotation(bc.STD, B, i)
        x, norms, codes, _, _ = bc.edge_message(bc.STD, s, B, tail, rot)
        n = len(x)
        want = (codes & ((1 << (br.code_bits(s) - 1)) - 1)).astype(np.int64)
        w = qc.words(n, bc.SEED, bc.CTR)
        u = qc.uniforms(w)
        tot = {"group": [0, 0], "level": [0, 0]}  # [decided, nonzero] over the buckets that count
        for b, (lo, hi) in enumerate(br.slices(n, B)):
            xs, nrm = x[lo:hi], norms[b]
            nz = xs != 0
            with np.errstate(all="ignore"):
                y = (np.abs(xs) / nrm).astype(F32)
                rs_finite = bool(np.isfinite(F32(s) / nrm))
            for name, (lvl, ok) in (("group", qc.fast_std_mirror(xs, nrm, s, w[lo:hi], GROUP)),
                                    ("level", qc.dither_level_mirror(y, s, u[lo:hi], LEVEL))):
                ok = ok & nz
                assert int((lvl[ok] != want[lo:hi][ok]).sum()) == 0, (B, s, b, float(nrm), name)
                if name == "group" and not rs_finite:
                    assert not ok.any(), (B, s, b)
                elif not (name == "level" and nrm < 2.0**-133) and rs_finite:
                    tot[name][0] += int(ok.sum())
                    tot[name][1] += int(nz.sum())
        for name, (decided, nonzero) in tot.items():
            print(f"[bucket-edges] B={B} s={s} {name}: fast {decided} exact {nonzero - decided}")
            assert decided >= 0.05 * nonzero and nonzero - decided >= 0.10 * nonzero, (B, s, name)


@pytest.mark.parametrize("B", bc.ALL_B)
def test_natural_edge_messages_hold_levels_and_both_decisions(B):
    for i, s in enumerate(qc.LEVELS_NAT):
        tail, rot = bc.rotation(bc.NAT, B, i)
        x, norms, codes, _, _ = bc.edge_message(bc.NAT, s, B, tail, rot)
        n = len(x)
        nrm = np.repeat(norms, B)[:n]
        lv = br.levels_of(bc.NAT, s)
        lvl = (codes & ((1 << (br.code_bits(s) - 1)) - 1)).astype(np.int64)
        with np.errstate(all="ignore"):
            y = (np.abs(x) / nrm).astype(F32).astype(F64)
        j = np.clip(np.searchsorted(lv, y, side="left"), 1, s)
        inside = (x != 0) & (y > lv[j - 1]) & (y < lv[j])
        assert (lvl[inside] == j[inside]).sum() >= n // 20 and (lvl[inside] == j[inside] - 1).sum() >= n // 20
        on = (x != 0) & np.isin(y, lv[1:])
        assert on.sum() >= n // 20 and np.array_equal(lv[lvl[on]], y[on])  # exactly on a level: that level


# ------------------------------------------------------------------------------------------------ the p = 2 model
def _dyadic(n, seed):
    """m * 2^-12 with integer |m| < 2^11: every sum of up to 4096 squares is exact in fp64 in any order."""
    g = np.random.default_rng(seed)
    m = g.integers(-(2**11) + 1, 2**11, size=n)
    m[g.random(n) < 0.05] = 0
    return (m.astype(F64) * 2.0**-12).astype(F32)


@pytest.mark.parametrize("B", bc.ALL_B)
def test_l2_model_is_exact_on_dyadic_inputs(B):
    x = _dyadic(3 * B + B // 2 + 3, B)
    want = np.array([np.sqrt(math.fsum((x[lo:hi].astype(F64) ** 2).tolist())) for lo, hi in br.slices(len(x), B)])
    assert np.array_equal(bc.l2_norm_model(x, B).view(np.uint32), want.astype(F32).view(np.uint32))
    assert np.array_equal(np.sqrt(bc.bucket_sums(x, B)), want)  # (the fp64 sum itself is the exact one)


@pytest.mark.parametrize("B", bc.ALL_B)
def test_l2_message_and_its_special_buckets(B):
    x, where = bc.l2_message(B)
    n = len(x)
    assert n >= 2 * bc.BLOCK + B and n <= 50_000 and n % B == B - 3 and set(bc.SPECIAL) <= set(where)
    model = bc.l2_norm_model(x, B)
    sums = bc.bucket_sums(x, B)
    seq_differs = 0
    for b, (lo, hi) in enumerate(br.slices(n, B)):
        sq = (x[lo:hi].astype(F64) ** 2).tolist()
        if not np.isfinite(x[lo:hi]).all():
            continue
        true = math.sqrt(math.fsum(sq))
        if true <= float(bc.FLT_MAX):  # within one fp32 ulp of the exactly summed value
            assert abs(float(model[b]) - true) <= float(np.spacing(F32(true))), (B, b)
        seq = 0.0
        for v in sq:
            seq += v
        seq_differs += seq != float(sums[b])
    assert seq_differs >= 3  # the order shows in the fp64 sum (a left-to-right chain gives other bits)
    sub = model[where["subnormal"]]
    assert 0 < sub < np.finfo(F32).tiny and float(sub) == float(F32(2.0**-149 * math.sqrt(B)))
    assert np.isposinf(model[where["overflow"]])
    below = model[where["below_max"]]
    assert np.isfinite(below) and below > F32(0.99) * bc.FLT_MAX
    assert np.isnan(model[where["nan"]]) and np.isposinf(model[where["inf"]])
    other = np.ones(len(model), dtype=bool)
    other[[where[k] for k in ("overflow", "nan", "inf")]] = False
    assert np.isfinite(model[other]).all() and (model[other] > 0).all()
    rev = bc.l2_norm_model(x, B, reverse_waves=True)
    if B >= 2048:  # the wave order decides the tie bucket's fp32 norm
        assert model[where["tie"]] == F32(1.0) and rev[where["tie"]] == F32(1.0 + 2.0**-23)
    else:  # two waves at most: a + b = b + a
        assert gc.same_bits(model, rev)


# ------------------------------------------------------------------------------------------------ hand-built records
FORMATS = [(bc.STD, 1, 2), (bc.STD, 7, 4), (bc.STD, 5, 4), (bc.STD, 127, 8), (bc.STD, 100, 8), (bc.NAT, 1, 2),
           (bc.NAT, 7, 4), (bc.NAT, 127, 8)]


@pytest.mark.parametrize("B", bc.ALL_B)
def test_handbuilt_records(B):
    seen = set()
    for f, (kind, s, bits) in enumerate(FORMATS):
        assert br.code_bits(s) == bits
        for i, name in enumerate(bc.RECORD_SIZES):
            n = bc.record_size(name, B)
            start = f + 3 * i
            rec, norms, codes, values = bc.handbuilt_record(kind, s, bits, B, n, start)
            nb = -(-n // B)
            stride, off = bc.wire_layout(n, bits, B)
            assert len(rec) == stride and stride % 256 == 0 and off % 16 == 0 and off >= 4 * nb
            nbytes = (n * bits + 7) // 8
            assert np.array_equal(rec[:4 * nb].view(F32).view(np.uint32), norms.view(np.uint32))
            assert np.array_equal(dc.unpack(rec[off:off + nbytes], n, bits), codes)
            assert (rec[4 * nb:off] == bc.PAD).all() and (rec[off + nbytes:] == bc.PAD).all()
            if (n * bits) % 8:  # the unused high bits of the last code byte are not zero
                assert rec[off + nbytes - 1] >> ((n * bits) % 8) != 0
            # bucket_ref.decode is the model of the encoder-made records; its rule for a norm that is not positive and
            # finite is the decoders' (nrm > 0 && nrm <= FLT_MAX) on every norm here, negative ones included
            assert gc.same_bits(values, br.decode(codes.astype(np.uint32), kind, s, B, norms))
            reg = np.repeat(dc.norm_regular(norms), B)[:n]
            zero = ~reg & (codes == 0)
            assert not values[zero].view(np.uint32).any() and np.isnan(values[~reg & (codes != 0)]).all()
            if n >= 2 * (s + 1):
                assert set(codes.tolist()) == set(dc.quant_codes(s, bits).tolist())
            seen |= {repr(float(v)) for v in norms}
    assert seen == {repr(float(v)) for v in bc.RECORD_NORMS}  # a one-bucket record meets every norm in turn
    r = dc.norm_regular(np.array(bc.RECORD_NORMS))
    assert int(r.sum()) == 5 and all(r[i] or r[i - 1] or r[(i + 1) % len(r)] for i in range(len(r)))


def test_fold_chain_is_the_ordered_fmaf():
    v = [np.array([1.0, 3e-39, -0.0, np.inf], dtype=F32), np.array([0.1, 1.0, 0.0, -1.0], dtype=F32)]
    got = bc.fold_chain(v, [0.37, -1.5], np.array([-0.0, 1e-40, -0.0, 2.0], dtype=F32))
    a = dc.fma_exact(F32(0.37), v[0], np.array([-0.0, 1e-40, -0.0, 2.0], dtype=F32), F32)
    assert gc.same_bits(got, dc.fma_exact(F32(-1.5), v[1], a, F32)) and np.isposinf(got[3])
