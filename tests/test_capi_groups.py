"""flc_fold_record_groups (a round's records folded into several destinations in one pass): argument validation, which
happens before anything touches the device, so it runs without one.  The pointers are never dereferenced."""

import ctypes

import pytest

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731
P = ctypes.c_void_p


def _args(**kw):
    """Three records (groups 0, 2, 0) of n = 3000, k = 30, 10 levels over 3 groups x 2 tensors; ``kw`` replaces."""
    a = dict(records=(P * 3)(256, 512, 768), weights=(ctypes.c_float * 3)(0.5, 1.0, -0.25),
             group_of=(ctypes.c_int32 * 3)(0, 2, 0), n_records=3, n=3000, k=30, levels=10,
             # group 1 has no record: its destinations may be null
             dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x40000), n_groups=3,
             sizes=(ctypes.c_int64 * 2)(1000, 2000), n_tensors=2)
    a.update(kw)
    return (c(a["records"]), c(a["weights"]), c(a["group_of"]), a["n_records"], a["n"], a["k"], a["levels"],
            c(a["dsts"]), a["n_groups"], c(a["sizes"]), a["n_tensors"], None)


BAD = {
    "null_record": (dict(records=(P * 3)(256, 0, 768)), "record 1 is null or not 16-B aligned"),
    "misaligned_record": (dict(records=(P * 3)(256, 512, 776)), "record 2 is null or not 16-B aligned"),
    "group_below": (dict(group_of=(ctypes.c_int32 * 3)(0, -1, 0)), "record 1 names group -1 outside [0, 3)"),
    "group_above": (dict(group_of=(ctypes.c_int32 * 3)(0, 2, 3)), "record 2 names group 3 outside [0, 3)"),
    "sizes_sum": (dict(sizes=(ctypes.c_int64 * 2)(1000, 1999)), "the tensors hold 2999 elements, the records 3000"),
    "negative_size": (dict(sizes=(ctypes.c_int64 * 2)(3001, -1)), "negative size for tensor 1"),
    "n_too_large": (dict(n=1 << 31, sizes=(ctypes.c_int64 * 2)(1 << 30, 1 << 30)), "n and k must be < 2^31"),
    "k_too_large": (dict(k=1 << 31), "n and k must be < 2^31"),
    "levels_zero": (dict(levels=0), "levels must be in [1, 127]"),
    "levels_128": (dict(levels=128), "levels must be in [1, 127]"),
    "null_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0)), "null pointer for tensor 1 of group 2"),
    "shared_destination": (dict(dsts=(P * 6)(0x10000, 0x20000, 0, 0, 0x30000, 0x10000)),
                           "groups 0 and 2 share a destination"),
    "shared_with_idle_group": (dict(dsts=(P * 6)(0x10000, 0x20000, 0x20000, 0, 0x30000, 0x40000)),
                               "groups 0 and 1 share a destination"),
    "no_tables": (dict(records=None), "bad arguments"),
    "no_groups": (dict(n_groups=0), "bad arguments"),
    "no_tensors": (dict(n_tensors=0), "bad arguments"),
}


@pytest.mark.parametrize("case", list(BAD))
def test_fold_record_groups_validates_without_gpu(case):
    from fl_sim_amd import _lib

    lib = _lib.load()
    kw, message = BAD[case]
    if kw.get("records", 1) is None:
        args = list(_args())
        args[0] = None
        rc = lib.flc_fold_record_groups(*args)
    else:
        rc = lib.flc_fold_record_groups(*_args(**kw))
    assert rc == 1  # FLC_EINVAL
    assert message in lib.flc_last_error().decode()


def test_fold_record_groups_without_records_is_a_no_op():
    """No record: nothing to fold, nothing launched (the tables are still checked)."""
    from fl_sim_amd import _lib

    lib = _lib.load()
    assert lib.flc_fold_record_groups(*_args(n_records=0)) == 0
    assert lib.flc_fold_record_groups(*_args(n_records=0, levels=0)) == 1
    with pytest.raises(_lib.FlcError, match="levels"):
        _lib.call("flc_fold_record_groups", *_args(levels=200))
