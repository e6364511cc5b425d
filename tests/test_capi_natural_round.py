"""flc_natural_encode_round and flc_natural_encode_residual_round: the symbols, their declarations and the argument
validation, which happens before anything touches a device, so it runs without one.  The pointers are never
dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p
U64 = ctypes.c_uint64
EINVAL = 1
N = 3000
PLAIN, RESIDUAL = "flc_natural_encode_round", "flc_natural_encode_residual_round"


def _lib():
    from fl_sim_amd import _lib as L

    return L


def _args(**kw):
    a = dict(xs=(P * 3)(0x10000, 0x20000, 0x30000), n_msgs=3, n=N, seeds=(U64 * 3)(1, 2, 3),
             counters=(U64 * 3)(4, 5, 6), codes=(P * 3)(0x40010, 0x50010, 0x60010))
    a.update(kw)
    tab = lambda v: None if v is None else c(v)  # noqa: E731
    return tab(a["xs"]), a["n_msgs"], a["n"], tab(a["seeds"]), tab(a["counters"]), tab(a["codes"]), None


def _call(entry, **kw):
    lib = _lib().load()
    rc = getattr(lib, entry)(*_args(**kw))
    return rc, lib.flc_last_error().decode(errors="replace")


def test_symbols_declared():
    L = _lib()
    lib = L.load()
    for entry in (PLAIN, RESIDUAL):
        assert hasattr(lib, entry) and entry in L.SIGNATURES
    assert L.SIGNATURES[PLAIN] == L.SIGNATURES[RESIDUAL]
    assert lib.flc_abi_version() == 1
    from fl_sim_amd import codec, compressed

    assert callable(codec.natural_encode_round) and callable(codec.natural_encode_residual_round)
    for bound in (compressed._DEFER_NATURAL_MAX_N, compressed._DEFER_EF_NATURAL_MAX_N):
        assert isinstance(bound, int) and 0 < bound <= compressed._DEFER_MAX_N


def test_the_switch_is_off_by_default():
    """FLC_NATURAL_DEFER unset: a fresh interpreter imports the package with the switch off; =1 turns it on."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "from fl_sim_amd import compressed; print(int(compressed.NATURAL_DEFER))"
    for value, want in ((None, "0"), ("1", "1")):
        env = {k: v for k, v in os.environ.items() if k != "FLC_NATURAL_DEFER"}
        if value is not None:
            env["FLC_NATURAL_DEFER"] = value
        out = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want, (value, out.stdout, out.stderr)


BAD = {
    "null_xs": dict(xs=None),
    "null_seeds": dict(seeds=None),
    "null_counters": dict(counters=None),
    "null_codes": dict(codes=None),
    "null_vector_entry": dict(xs=(P * 3)(0x10000, 0, 0x30000)),
    "null_codes_entry": dict(codes=(P * 3)(0x40010, 0x50010, 0)),
    "no_messages": dict(n_msgs=0),
    "negative_messages": dict(n_msgs=-1),
    "n_zero": dict(n=0),
    "n_negative": dict(n=-7),
    "n_2_31": dict(n=1 << 31),
    "vector_4_mod_16": dict(xs=(P * 3)(0x10000, 0x20004, 0x30000)),
    "codes_8_mod_16": dict(codes=(P * 3)(0x40010, 0x50010, 0x60018)),
}
BAD_RESIDUAL = {
    "same_memory_twice": dict(xs=(P * 3)(0x10000, 0x20000, 0x10000)),
    "same_memory_adjacent": dict(xs=(P * 3)(0x20000, 0x20000, 0x30000)),
    "memories_overlap": dict(xs=(P * 3)(0x10000, 0x10000 + 4 * N - 16, 0x30000)),
}


@pytest.mark.parametrize("entry", [PLAIN, RESIDUAL])
@pytest.mark.parametrize("case", sorted(BAD))
def test_einval_before_the_device(case, entry):
    rc, msg = _call(entry, **BAD[case])
    assert rc == EINVAL, (rc, msg)
    assert msg and entry in msg


@pytest.mark.parametrize("case", sorted(BAD_RESIDUAL))
def test_residual_form_refuses_memories_that_share_elements(case):
    rc, msg = _call(RESIDUAL, **BAD_RESIDUAL[case])
    assert rc == EINVAL and RESIDUAL in msg and "share" in msg, (rc, msg)


def test_the_messages_name_the_fault():
    for case, word in (("vector_4_mod_16", "aligned"), ("null_vector_entry", "null"), ("no_messages", "n_msgs"),
                       ("n_2_31", "2^31")):
        for entry in (PLAIN, RESIDUAL):
            rc, msg = _call(entry, **BAD[case])
            assert rc == EINVAL and word in msg, (case, entry, msg)


def test_validation_order_puts_the_tables_first():
    # (a null table with a bad n_msgs: still EINVAL, and no entry is read)
    for entry in (PLAIN, RESIDUAL):
        rc, msg = _call(entry, xs=None, n_msgs=0)
        assert rc == EINVAL and "null table" in msg
