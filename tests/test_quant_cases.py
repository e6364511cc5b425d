"""CPU checks of the decision-edge quantizer inputs (tests/quant_cases.py): what the catalogue reaches.  The float32
mirrors of the two fast paths of the standard dithering never contradict the oracle with the shipped margins, both
their fast and their exact path are reached at every (levels, norm), a tenth of the u-margin is contradicted (so the
catalogue stands in the zone the margin protects), host math.log2 is correctly rounded on the near-power-of-two
catalogue (which pins the oracle of natural64_code's log2 branch), and the natural catalogue holds pt == u elements
and an overflow to +-inf."""

import functools
import math

import numpy as np
import pytest

from oracle import compressors_ref as ref
from tests import quant_cases as qc

N = 40_000
SEED, CTR = 11, 5
GROUP, LEVEL = (1e-4, 5e-5), (1e-4, 3e-5)  # shipped margins: quant.hip / topk.hip, flc_device.hpp dither_level


@functools.lru_cache(maxsize=None)
def _words():
    w = qc.words(N, SEED, CTR)
    return w, qc.uniforms(w)


@functools.lru_cache(maxsize=None)
def _survey(s, ni):
    """One (levels, norm) of the catalogue: the oracle's levels and, per mirror and margin set, (decided mask,
    wrongly decided count)."""
    norm = qc.NORMS32[ni]
    w, u = _words()
    x = qc.std_edge_case(s, norm, N, SEED, CTR, np.random.default_rng(1000 * s + ni))
    assert x.dtype == np.float32 and np.abs(x).max() == norm and abs(x[0]) == norm
    _, _, _, want = ref.dither(x, ref.standard_levels(s), norm, lambda i: u[i])
    nz = x != 0
    with np.errstate(all="ignore"):
        y = (np.abs(x) / norm).astype(np.float32)
        rs_finite = bool(np.isfinite(np.float32(s) / norm))
    out = {"nz": int(nz.sum()), "rs_finite": rs_finite}
    for name, fn, shipped in (("group", lambda m: qc.fast_std_mirror(x, norm, s, w, m), GROUP),
                              ("level", lambda m: qc.dither_level_mirror(y, s, u, m), LEVEL)):
        for tag, m in (("shipped", shipped), ("tenth", (shipped[0], shipped[1] / 10))):
            lvl, ok = fn(m)
            ok = ok & nz
            out[name, tag] = (int(ok.sum()), int((lvl[ok] != want[ok]).sum()))
    return out


def test_words_are_the_oracle_uniforms():
    w, u = _words()
    assert w.dtype == np.uint32 and np.array_equal(u, ref.philox_uniforms(N, SEED, CTR))
    at = np.array([0, 5, 70_000, 2**33 + 3], dtype=np.uint64)
    assert np.array_equal(qc.uniforms(qc.words_at(at, SEED, CTR)), ref.philox_uniforms_at(at, SEED, CTR))


@pytest.mark.parametrize("s", qc.LEVELS_STD)
def test_mirrors_agree_with_the_oracle_and_reach_both_paths(s):
    """With the shipped margins no mirror decides an element against ref.dither; each leaves >= 10 % of the nonzero
    elements to the exact rule and decides >= 5 % itself.  Two exceptions follow from float32 itself, not from the
    code: where fp32(s / norm) overflows the group path decides nothing at all (t' = inf, p' = NaN: asserted), and
    under norm = 3e-42 |x| has 2141 values, so y * s comes within 1e-4 of an integer only at 0 and at the norm and
    no offset of the catalogue can be represented (there: at least the element at the norm is left undecided)."""
    for ni, norm in enumerate(qc.NORMS32):
        r = _survey(s, ni)
        tag = (s, float(norm), r)
        for name in ("group", "level"):
            decided, wrong = r[name, "shipped"]
            print(f"[quant-edges] s={s} norm={norm:.8g} {name}: fast {decided} exact {r['nz'] - decided} wrong {wrong}")
            assert wrong == 0, tag
            if name == "group" and not r["rs_finite"]:
                assert decided == 0, tag
                continue
            if name == "level" and norm < 2.0**-133:  # fewer than 2^16 values of |x|
                assert decided < r["nz"], tag
                continue
            assert r["nz"] - decided >= 0.10 * r["nz"], tag
            assert decided >= 0.05 * r["nz"], tag


def test_a_tenth_of_the_u_margin_decides_wrongly():
    """s = 127, the four norms past the s / norm overflow taken together: with the u-margin at a tenth each mirror
    decides at least one element against the oracle."""
    norms = [np.float32(v) for v in (3.8e-37, 8.6e37, 1e38, 3.4028235e38)]
    for name in ("group", "level"):
        wrong = sum(_survey(127, qc.NORMS32.index(nv))[name, "tenth"][1] for nv in norms)
        print(f"[quant-edges] s=127 {name}: {wrong} wrong decisions at a tenth of the u-margin")
        assert wrong >= 1, name


def test_host_log2_is_correctly_rounded_near_powers_of_two():
    """The oracle's math.log2 on every element of near_pow2_case64 against log2 correctly rounded through ``decimal``:
    equal wherever either value is an integer, the same floor and ceil everywhere (what ref.natural64 takes from it),
    and never more than one ulp apart.  (Plain equality cannot be asked of every libm: glibc's log2 is faithfully, not
    correctly rounded, and under it 4 of the 845,661 elements, none beside an integer, come out one ulp off.)"""
    r = qc.host_log2_survey()
    print(f"[quant-edges] near_pow2_case64: {r}")
    assert r["n"] < 2_000_000
    assert r["decides"]
    assert r["max_ulps"] <= 1.0
    assert r["on_integer"] >= 100


def test_near_pow2_catalogue_shape():
    x, u = qc.near_pow2_case64()
    assert x.dtype == np.float64 and u.dtype == np.float64 and x.shape == u.shape
    assert (x > 0).any() and (x < 0).any() and np.all(x != 0) and np.all((u >= 0) & (u < 1))
    a = np.abs(x)
    for f in qc.NEAR_POW2_EXPONENTS:
        W = (abs(f) + 2) * 2.0**-48
        lo, hi = math.ldexp(1.0 - 4 * W, f), math.ldexp(1.0 + 4 * W, f)
        inside = a[(a >= lo) & (a <= hi)]
        assert math.ldexp(1.0, f) in inside
        if f > -1022:  # both sides of the branch switch, above and below the power
            r = inside / math.ldexp(1.0, f) - 1.0
            assert (r > W).any() and ((r > 0) & (r <= W)).any() and (r < -W).any() and ((r < 0) & (r >= -W)).any(), f


def test_natural_catalogue_holds_exact_ties_and_an_overflow():
    n = 65_543
    x, tie = qc.natural_edge_case(n, SEED, CTR, np.random.default_rng(3))
    u = ref.philox_uniforms(n, SEED, CTR)
    assert x.dtype == np.float32 and int(tie.sum()) >= 20
    with np.errstate(over="ignore"):
        out, _, _ = ref.natural(x, lambda i: u[i])
        # pt == u: the strict < sends the element to the upper power (a normal non-power: twice its binade's floor)
        up = np.ldexp(1.0, np.frexp(np.abs(x[tie]).astype(np.float64))[1]).astype(np.float32)
    assert np.array_equal(np.abs(out[tie]), up)
    assert np.isposinf(out).any() and np.isneginf(out).any()
    assert (np.abs(x) == np.float32(2.0**-149)).any() and (np.abs(x) == np.finfo(np.float32).max).any()
    x64, tie64 = qc.natural_edge_case64(n, SEED, CTR, np.random.default_rng(4))
    assert x64.dtype == np.float64 and int(tie64.sum()) >= 20
