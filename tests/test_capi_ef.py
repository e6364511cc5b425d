"""The error-feedback entry points (flc_ef_accumulate, flc_ef_residual_round, flc_ef_residual_dense): argument
validation, which happens before anything touches the device, so it runs without one.  The pointers are never
dereferenced."""

import ctypes

import pytest

c = lambda a: None if a is None else ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p


def _lib_():
    from fl_sim_amd import _lib

    return _lib, _lib.load()


# ------------------------------------------------------------------------------------------------ flc_ef_accumulate
def _acc(**kw):
    """Three tensors of 1000, 0 and 2000 elements (the empty one's pointers null) into a memory; ``kw`` replaces."""
    a = dict(local=(P * 3)(0x10000, 0, 0x20000), glob=(P * 3)(0x30000, 0, 0x40000),
             sizes=(ctypes.c_int64 * 3)(1000, 0, 2000), n_tensors=3, e=0x50000)
    a.update(kw)
    return (c(a["local"]), c(a["glob"]), c(a["sizes"]), a["n_tensors"], a["e"], None)


ACC_BAD = {
    "no_local": (dict(local=None), "bad arguments"),
    "no_sizes": (dict(sizes=None), "bad arguments"),
    "negative_count": (dict(n_tensors=-1), "bad arguments"),
    "negative_size": (dict(sizes=(ctypes.c_int64 * 3)(1000, -1, 2000)), "negative size for tensor 1"),
    "null_local": (dict(local=(P * 3)(0x10000, 0, 0)), "null pointer for tensor 2"),
    "null_global": (dict(glob=(P * 3)(0, 0, 0x40000)), "null pointer for tensor 0"),
    "null_memory": (dict(e=None), "null pointer for tensor 0"),
    # the bad tensor sits in the second launch of the chain: still nothing is launched
    "null_local_in_a_later_launch": (dict(local=(P * 60)(*([0x10000] * 59 + [0])), glob=None,
                                          sizes=(ctypes.c_int64 * 60)(*([4] * 60)), n_tensors=60),
                                     "null pointer for tensor 59"),
}


@pytest.mark.parametrize("case", list(ACC_BAD))
def test_ef_accumulate_validates_without_gpu(case):
    _, lib = _lib_()
    kw, message = ACC_BAD[case]
    assert lib.flc_ef_accumulate(*_acc(**kw)) == 1  # FLC_EINVAL
    assert "flc_ef_accumulate: " + message in lib.flc_last_error().decode()


def test_ef_accumulate_of_nothing_is_a_no_op():
    """No tensor, or empty tensors only (null pointers, a null memory): nothing launched."""
    _, lib = _lib_()
    assert lib.flc_ef_accumulate(None, None, None, 0, None, None) == 0
    assert lib.flc_ef_accumulate(*_acc(local=(P * 3)(0, 0, 0), glob=None, sizes=(ctypes.c_int64 * 3)(0, 0, 0),
                                       e=None)) == 0


# -------------------------------------------------------------------------------------------- flc_ef_residual_round
def _res(**kw):
    """Three clients' records and memories, n = 3000, k = 30, 10 levels; ``kw`` replaces."""
    a = dict(records=(P * 3)(256, 512, 768), es=(P * 3)(0x10000, 0x20000, 0x30000), n_clients=3, n=3000, k=30,
             levels=10)
    a.update(kw)
    return (c(a["records"]), c(a["es"]), a["n_clients"], a["n"], a["k"], a["levels"], None)


RES_BAD = {
    "negative_clients": (dict(n_clients=-1), "bad arguments"),
    "no_records": (dict(records=None), "bad arguments"),
    "no_memories": (dict(es=None), "bad arguments"),
    "null_record": (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "misaligned_record": (dict(records=(P * 3)(256, 512, 776)), "record 2 is null or not 16-B aligned"),
    "null_memory": (dict(es=(P * 3)(0x10000, 0, 0x30000)), "null memory for client 1"),
    "shared_memory": (dict(es=(P * 3)(0x10000, 0x20000, 0x10000)), "clients 0 and 2 share a memory"),
    "n_too_large": (dict(n=1 << 31), "n and k must be < 2^31"),
    "k_too_large": (dict(n=(1 << 31) - 1, k=1 << 31), "n and k must be < 2^31"),
    "k_above_n": (dict(k=3001), "k 3001 > n 3000"),
    "levels_zero": (dict(levels=0), "levels must be in [1, 127]"),
    "levels_128": (dict(levels=128), "levels must be in [1, 127]"),
}


@pytest.mark.parametrize("case", list(RES_BAD))
def test_ef_residual_round_validates_without_gpu(case):
    _, lib = _lib_()
    kw, message = RES_BAD[case]
    assert lib.flc_ef_residual_round(*_res(**kw)) == 1  # FLC_EINVAL
    assert "flc_ef_residual_round: " + message in lib.flc_last_error().decode()


def test_ef_residual_round_without_clients_or_entries_is_a_no_op():
    """No client, or no kept entry: nothing launched (the tables are still checked)."""
    _lib, lib = _lib_()
    assert lib.flc_ef_residual_round(*_res(n_clients=0)) == 0
    assert lib.flc_ef_residual_round(None, None, 0, 3000, 30, 10, None) == 0
    assert lib.flc_ef_residual_round(*_res(k=0)) == 0
    assert lib.flc_ef_residual_round(*_res(n_clients=0, levels=0)) == 1
    assert lib.flc_ef_residual_round(*_res(k=0, es=(P * 3)(0x10000, 0x20000, 0x20000))) == 1
    assert "clients 1 and 2 share a memory" in lib.flc_last_error().decode()
    assert lib.flc_ef_residual_round(*_res(k=0, records=(P * 3)(256, 8, 768))) == 1
    with pytest.raises(_lib.FlcError, match="levels"):
        _lib.call("flc_ef_residual_round", *_res(levels=200))


# -------------------------------------------------------------------------------------------- flc_ef_residual_dense
DENSE_BAD = {
    "same_vector": ((0x10000, 0x10000, 100), "e and c are the same vector"),
    "null_memory": ((None, 0x10000, 100), "bad arguments"),
    "null_c": ((0x10000, None, 100), "bad arguments"),
    "negative_n": ((0x10000, 0x20000, -1), "bad arguments"),
}


@pytest.mark.parametrize("case", list(DENSE_BAD))
def test_ef_residual_dense_validates_without_gpu(case):
    _, lib = _lib_()
    (e, cc, n), message = DENSE_BAD[case]
    assert lib.flc_ef_residual_dense(e, cc, n, None) == 1  # FLC_EINVAL
    assert "flc_ef_residual_dense: " + message in lib.flc_last_error().decode()


def test_ef_residual_dense_of_nothing_is_a_no_op():
    _, lib = _lib_()
    assert lib.flc_ef_residual_dense(0x10000, 0x20000, 0, None) == 0
    assert lib.flc_ef_residual_dense(None, None, 0, None) == 0


def test_abi_version_is_unchanged():
    _, lib = _lib_()
    assert lib.flc_abi_version() == 1
