"""tests/bucket_ref.py (the oracle's dithering rule run per slice) reproduces tests/golden/bucket_codec.npz — the
reference's own Compressor.compressVector called on every slice of B elements in order
(tests/golden/gen_golden_bucket.py) — bit for bit: outputs, send statistics and the ``random`` stream's position.
Then flc_bucket_wire_layout, a pure host function."""

import ctypes
import random

import numpy as np
import pytest

from tests import bucket_ref as br
from tests import golden_cases as gc
from tests.golden.gen_golden_bucket import BUCKET_NS, bucket_cases, bucket_input, bucket_key, bucket_seed

CASES = list(bucket_cases())


@pytest.fixture(scope="module")
def fixture():
    return np.load(f"{gc.GOLDEN}/bucket_codec.npz", allow_pickle=False)


def test_fixture_key_set_and_inputs(fixture):
    want = {f"x_n{n}" for n in BUCKET_NS}
    for c in CASES:
        want |= {bucket_key(*c) + f for f in ("|out", "|pnorm", "|stats", "|next_random")}
    assert set(fixture.files) == want
    for n in BUCKET_NS:
        x = fixture[f"x_n{n}"]
        assert gc.same_bits(x, bucket_input(n))
        assert 0.02 * n <= np.count_nonzero(x == 0) and np.count_nonzero(np.signbit(x) & (x == 0)) >= 1


@pytest.mark.parametrize("kind,s,p,B,n", CASES, ids=[bucket_key(*c) for c in CASES])
def test_oracle_reproduces_the_slice_wise_reference(kind, s, p, B, n, fixture):
    key = bucket_key(kind, s, p, B, n)
    x = fixture[f"x_n{n}"]
    pn = fixture[key + "|pnorm"]
    nb = -(-n // B)
    assert pn.shape == (nb,) and pn.dtype == np.float32
    if np.isinf(p):  # the oracle's own max per slice
        assert gc.same_bits(pn, np.array([np.max(np.abs(x[lo:hi])) for lo, hi in br.slices(n, B)], dtype=np.float32))
    random.seed(bucket_seed(kind, s, p, B, n))
    out, send, _ = br.bucket_compat(x, kind, s, B, pn)
    assert gc.same_bits(out, fixture[key + "|out"])
    stats = fixture[key + "|stats"]
    assert stats[0] == send and stats[1] == n
    assert (stats[2], stats[3]) == ((nb, nb) if kind == "std" else (0, 0))
    assert random.random() == float(fixture[key + "|next_random"])


# ----------------------------------------------------------------------------------------------- layout
c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
STD, NATD, NATURAL = 0, 1, 2


def _layout(n, fmt, bits, bucket, off=None):
    from fl_sim_amd import _lib as L

    return L.size("flc_bucket_wire_layout", n, fmt, bits, bucket, None if off is None else c(off))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("B", [64, 512, 4096])
@pytest.mark.parametrize("fmt,bits", [(STD, 2), (STD, 4), (STD, 8), (NATD, 2), (NATD, 4), (NATD, 8)])
def test_bucket_layout(n, B, fmt, bits):
    off = (ctypes.c_int64 * 2)(-1, -1)
    total = _layout(n, fmt, bits, B, off)
    nb = -(-n // B)
    code_bytes = (n * bits + 7) // 8
    assert total > 0 and total % 256 == 0
    assert off[0] % 16 == 0 and off[1] % 16 == 0
    assert off[0] + 4 * nb <= off[1] < off[0] + 4 * nb + 16  # the nb norms lie before the codes, padded to 16 B
    assert off[1] + code_bytes <= total < off[1] + code_bytes + 256
    assert (B * bits // 8) % 16 == 0  # every bucket's codes start 16-B aligned
    assert _layout(n, fmt, bits, B) == total  # (offsets are optional)
    from fl_sim_amd import codec

    assert codec.bucket_wire_layout(n, fmt, bits, B) == (total, {"norms": off[0], "codes": off[1]})


@pytest.mark.parametrize("n,fmt,bits,B", [
    (100, STD, 8, 0), (100, STD, 8, 32), (100, STD, 8, 8192), (100, STD, 8, 96), (100, STD, 8, 500), (100, STD, 8, -64),
    (100, NATURAL, 16, 64), (100, NATURAL, 8, 64), (100, 3, 8, 64), (100, -1, 8, 64),
    (100, STD, 1, 64), (100, STD, 3, 64), (100, NATD, 16, 64), (100, NATD, 0, 64),
    (0, STD, 8, 64), (-5, NATD, 4, 512), (1 << 31, STD, 8, 4096), (1 << 40, NATD, 2, 64)])
def test_bucket_layout_rejects(n, fmt, bits, B):
    assert _layout(n, fmt, bits, B) == 0


def test_bucket_layout_just_below_the_limit():
    n = (1 << 31) - 1
    assert _layout(n, STD, 8, 4096) == (1 << 19) * 4 + (1 << 31)  # 2^19 norms, then n bytes rounded up to 256


def test_bucket_symbols_exported():
    from fl_sim_amd import _lib as L

    lib = L.load()
    for name in ("flc_bucket_wire_layout", "flc_bucket_encode", "flc_bucket_encode_round", "flc_bucket_decode"):
        assert hasattr(lib, name) and name in L.SIGNATURES


def test_bucket_entry_points_validate_without_gpu():
    """The argument checks run before anything touches the device; the pointers are never dereferenced."""
    from fl_sim_amd import _lib as L

    lib = L.load()

    def enc(n=1000, kind=STD, levels=7, bits=4, bucket=64, p=0, x=0x10000, norms=0x20000, codes=0x30000, out=None):
        return lib.flc_bucket_encode(x, n, kind, levels, bits, bucket, p, 0, 1, 2, norms, codes, None, out, None)

    for kw, msg in [(dict(bucket=32), "bucket 32"), (dict(bucket=96), "bucket 96"), (dict(bucket=8192), "bucket 8192"),
                    (dict(n=0), "n must be"), (dict(n=1 << 31), "n must be"), (dict(levels=8), "levels 8"),
                    (dict(bits=3), "bits must be"), (dict(kind=2), "unknown kind"), (dict(p=1), "p must be"),
                    (dict(x=None), "null"), (dict(codes=0x30004), "16-B aligned"), (dict(out=0x40004), "16-B aligned")]:
        assert enc(**kw) == 1
        err = lib.flc_last_error().decode()
        assert msg in err  # (the quantizer's shared kind / levels / bits messages do not name the caller)
    P = ctypes.c_void_p
    U = ctypes.c_uint64

    def rnd(n_msgs=2, bucket=64, xs=(P * 2)(0x10000, 0x20000), codes=(P * 2)(0x30000, 0x40000)):
        return lib.flc_bucket_encode_round(c(xs), n_msgs, 1000, STD, 7, 4, bucket, 0, 0, c((U * 2)(1, 2)),
                                           c((U * 2)(3, 4)), c((P * 2)(0x50000, 0x60000)), c(codes), None, None)

    for kw, msg in [(dict(n_msgs=0), "n_msgs 0"), (dict(bucket=100), "bucket 100"),
                    (dict(xs=(P * 2)(0x10000, 0)), "null entry for message 1"),
                    (dict(codes=(P * 2)(0x30000, 0x40008)), "16-B aligned")]:
        assert rnd(**kw) == 1
        err = lib.flc_last_error().decode()
        assert msg in err and "flc_bucket_encode_round" in err
    assert lib.flc_bucket_decode(0x10000, 1000, STD, 7, 4, 48, 0x20000, 1.0, 0, 0x30000, None) == 1
    assert "bucket 48" in lib.flc_last_error().decode()
