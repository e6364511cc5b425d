"""flc_quant_encode_residual_round: the symbol, its declaration and the argument validation, which happens before
anything touches a device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
U64 = ctypes.c_uint64
EINVAL, EWORKSPACE = 1, 3
STD, NATD = 0, 1  # FLC_Q_STANDARD_DITHER, FLC_Q_NATURAL_DITHER
N = 3000


def _lib():
    from fl_sim_amd import _lib as L

    return L


def _args(**kw):
    a = dict(es=(P * 3)(0x10000, 0x20000, 0x30000), n_msgs=3, n=N, kind=STD, levels=7, bits=4, norm_p=0,
             seeds=(U64 * 3)(1, 2, 3), counters=(U64 * 3)(4, 5, 6), codes=(P * 3)(0x40010, 0x50010, 0x60010),
             norms=(P * 3)(0x40000, 0x50000, 0x60000), counts=(P * 3)(0x70000, 0x70008, 0x70010), ws=0x80000,
             ws_bytes=1 << 30)
    a.update(kw)
    tab = lambda v: None if v is None else c(v)  # noqa: E731
    return (tab(a["es"]), a["n_msgs"], a["n"], a["kind"], a["levels"], a["bits"], a["norm_p"], tab(a["seeds"]),
            tab(a["counters"]), tab(a["codes"]), tab(a["norms"]), tab(a["counts"]), a["ws"], a["ws_bytes"], None)


def _call(**kw):
    lib = _lib().load()
    rc = lib.flc_quant_encode_residual_round(*_args(**kw))
    return rc, lib.flc_last_error().decode(errors="replace")


def test_symbol_declared_and_abi_version():
    L = _lib()
    lib = L.load()
    assert hasattr(lib, "flc_quant_encode_residual_round") and "flc_quant_encode_residual_round" in L.SIGNATURES
    assert L.SIGNATURES["flc_quant_encode_residual_round"] == L.SIGNATURES["flc_quant_encode_round"]
    assert lib.flc_abi_version() == 1
    from fl_sim_amd import codec, compressed

    assert callable(codec.quant_encode_residual_round)
    assert isinstance(compressed._DEFER_EF_DENSE_MAX_N, int) and compressed._DEFER_EF_DENSE_MAX_N > 0


def test_the_switch_is_off_by_default():
    """FLC_EF_DENSE_DEFER unset: a fresh interpreter imports the package with the switch off; =1 turns it on."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from fl_sim_amd import compressed; print(int(compressed.EF_DENSE_DEFER))"
    for value, want in ((None, "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "FLC_EF_DENSE_DEFER"}
        if value is not None:
            env["FLC_EF_DENSE_DEFER"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (value, out.stdout, out.stderr)


BAD = {
    "null_es": dict(es=None),
    "null_seeds": dict(seeds=None),
    "null_counters": dict(counters=None),
    "null_codes": dict(codes=None),
    "null_norms": dict(norms=None),
    "null_memory_entry": dict(es=(P * 3)(0x10000, 0, 0x30000)),
    "null_codes_entry": dict(codes=(P * 3)(0x40010, 0x50010, 0)),
    "null_norm_entry": dict(norms=(P * 3)(0, 0x50000, 0x60000)),
    "null_count_entry": dict(counts=(P * 3)(0x70000, 0, 0x70010)),
    "same_memory_twice": dict(es=(P * 3)(0x10000, 0x20000, 0x10000)),
    "same_memory_adjacent": dict(es=(P * 3)(0x20000, 0x20000, 0x30000)),
    "memories_overlap": dict(es=(P * 3)(0x10000, 0x10000 + 4 * N - 16, 0x30000)),
    "no_messages": dict(n_msgs=0),
    "negative_messages": dict(n_msgs=-1),
    "n_zero": dict(n=0),
    "n_negative": dict(n=-7),
    "n_2_31": dict(n=1 << 31),
    "levels_8_in_4_bits": dict(levels=8),
    "levels_zero": dict(levels=0),
    "levels_2_in_2_bits": dict(levels=2, bits=2),
    "levels_128": dict(levels=128, bits=8),
    "bits_3": dict(bits=3),
    "unknown_kind": dict(kind=2),
    "norm_p_1": dict(norm_p=1),
    "norm_p_3": dict(norm_p=3),
    "memory_4_mod_16": dict(es=(P * 3)(0x10000, 0x20004, 0x30000)),
    "codes_8_mod_16": dict(codes=(P * 3)(0x40010, 0x50010, 0x60018)),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_einval_before_the_device(case):
    rc, msg = _call(**BAD[case])
    assert rc == EINVAL, (rc, msg)
    assert msg


def test_the_messages_name_the_call_and_the_fault():
    for case, word in (("same_memory_twice", "share"), ("memory_4_mod_16", "aligned"), ("null_memory_entry", "null"),
                       ("norm_p_1", "p must be"), ("no_messages", "n_msgs")):
        rc, msg = _call(**BAD[case])
        assert rc == EINVAL and "flc_quant_encode_residual_round" in msg and word in msg, (case, msg)


def test_memories_that_only_touch_are_distinct():
    # (es[1] begins where es[0]'s n elements end: valid, so the call gets as far as the workspace check)
    rc, msg = _call(es=(P * 3)(0x10000, 0x10000 + 4 * N, 0x30000), ws_bytes=0)
    assert rc == EWORKSPACE, (rc, msg)


def test_counts_table_is_optional_for_validation():
    rc, msg = _call(counts=None, n_msgs=0)
    assert rc == EINVAL and "n_msgs" in msg


def test_short_workspace():
    L = _lib()
    need = L.size("flc_quant_encode_round_workspace_size", N, 3)
    rc, msg = _call(ws_bytes=need - 1)
    assert rc == EWORKSPACE and "workspace" in msg
    rc, msg = _call(ws=None)
    assert rc == EWORKSPACE
