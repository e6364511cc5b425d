"""flc_quant_encode_round: the symbols, the workspace size and the argument validation, which happens before anything
touches a device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
U64 = ctypes.c_uint64
EINVAL, EWORKSPACE = 1, 3
STD, NATD = 0, 1  # FLC_Q_STANDARD_DITHER, FLC_Q_NATURAL_DITHER


def _lib():
    from fl_sim_amd import _lib as L

    return L


def _args(**kw):
    a = dict(xs=(P * 3)(0x10000, 0x20000, 0x30000), n_msgs=3, n=3000, kind=STD, levels=7, bits=4, norm_p=0,
             seeds=(U64 * 3)(1, 2, 3), counters=(U64 * 3)(4, 5, 6), codes=(P * 3)(0x40010, 0x50010, 0x60010),
             norms=(P * 3)(0x40000, 0x50000, 0x60000), counts=(P * 3)(0x70000, 0x70008, 0x70010), ws=0x80000,
             ws_bytes=1 << 30)
    a.update(kw)
    tab = lambda v: None if v is None else c(v)  # noqa: E731
    return (tab(a["xs"]), a["n_msgs"], a["n"], a["kind"], a["levels"], a["bits"], a["norm_p"], tab(a["seeds"]),
            tab(a["counters"]), tab(a["codes"]), tab(a["norms"]), tab(a["counts"]), a["ws"], a["ws_bytes"], None)


def _call(**kw):
    lib = _lib().load()
    rc = lib.flc_quant_encode_round(*_args(**kw))
    return rc, lib.flc_last_error().decode(errors="replace")


def test_symbols_exported():
    L = _lib()
    lib = L.load()
    for name in ("flc_quant_encode_round", "flc_quant_encode_round_workspace_size"):
        assert hasattr(lib, name) and name in L.SIGNATURES
    assert lib.flc_abi_version() == 1
    from fl_sim_amd import codec, compressed

    assert callable(codec.quant_encode_round) and callable(compressed.deferred_dense_stats)
    assert sorted(compressed.deferred_dense_stats()) == sorted(compressed.deferred_stats()) == ["batches", "messages"]


def test_workspace_size_grows_with_messages():
    L = _lib()
    sizes = [L.size("flc_quant_encode_round_workspace_size", 417482, m) for m in (1, 2, 10, 64, 65, 200)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    # one row of norm partials per message: the size of one message's share does not depend on the batch
    assert sizes[1] - sizes[0] == (sizes[3] - sizes[2]) // 54
    assert L.size("flc_quant_encode_round_workspace_size", 1, 10) <= sizes[2]


BAD = {
    "null_xs": dict(xs=None),
    "null_seeds": dict(seeds=None),
    "null_counters": dict(counters=None),
    "null_codes": dict(codes=None),
    "null_norms": dict(norms=None),
    "null_x_entry": dict(xs=(P * 3)(0x10000, 0, 0x30000)),
    "null_codes_entry": dict(codes=(P * 3)(0x40010, 0x50010, 0)),
    "null_norm_entry": dict(norms=(P * 3)(0, 0x50000, 0x60000)),
    "null_count_entry": dict(counts=(P * 3)(0x70000, 0, 0x70010)),
    "no_messages": dict(n_msgs=0),
    "negative_messages": dict(n_msgs=-1),
    "n_zero": dict(n=0),
    "n_negative": dict(n=-7),
    "n_2_31": dict(n=1 << 31),
    "n_huge": dict(n=1 << 40),
    "levels_8_in_4_bits": dict(levels=8),
    "levels_zero": dict(levels=0),
    "levels_2_in_2_bits": dict(levels=2, bits=2),
    "levels_128": dict(levels=128, bits=8),
    "bits_3": dict(bits=3),
    "bits_16": dict(bits=16),
    "unknown_kind": dict(kind=2),
    "norm_p_1": dict(norm_p=1),
    "norm_p_3": dict(norm_p=3),
    "x_4_mod_16": dict(xs=(P * 3)(0x10000, 0x20004, 0x30000)),
    "codes_8_mod_16": dict(codes=(P * 3)(0x40010, 0x50010, 0x60018)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval_before_the_device(case):
    rc, msg = _call(**BAD[case])
    assert rc == EINVAL, (rc, msg)
    assert msg


def test_counts_table_is_optional_for_validation():
    # (counts == NULL is valid: with every other argument bad in one way the failure is that argument's)
    rc, msg = _call(counts=None, n_msgs=0)
    assert rc == EINVAL and "n_msgs" in msg


def test_short_workspace():
    L = _lib()
    need = L.size("flc_quant_encode_round_workspace_size", 3000, 3)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == EWORKSPACE and "workspace" in msg
    rc, msg = _call(ws=None)
    assert rc == EWORKSPACE
