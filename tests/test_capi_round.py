"""flc_stacked_encode_round / flc_stacked_encode_delta_round (one Philox counter per message, the send counts made by
the encode): argument validation, which happens before anything touches the device, so it runs without one."""

import ctypes

c = lambda a: ctypes.cast(a, ctypes.c_void_p)  # noqa: E731


def test_stacked_encode_round_validates_without_gpu():
    """The bad client tables flc_stacked_encode_batch rejects, a null counter table and a null count pointer."""
    from fl_sim_amd import _lib

    lib = _lib.load()
    P = ctypes.c_void_p * 2
    U = ctypes.c_uint64 * 2
    good, seeds, ctrs = P(16, 32), U(1, 2), U(3, 1 << 40)
    f = lib.flc_stacked_encode_round
    assert f(None, 2, 100, 10, 127, None, None, None, None, None, None, None, 16, 1 << 30, None) == 1
    rc = f(c(good), 0, 100, 10, 127, c(seeds), c(ctrs), c(good), c(good), c(good), None, None, 16, 1 << 30, None)
    assert rc == 1 and "bad arguments" in lib.flc_last_error().decode()
    rc = f(c(good), 2, 100, 10, 200, c(seeds), c(ctrs), c(good), c(good), c(good), None, None, 16, 1 << 30, None)
    assert rc == 1 and "levels" in lib.flc_last_error().decode()
    rc = f(c(P(16, 40)), 2, 100, 10, 127, c(seeds), c(ctrs), c(good), c(good), c(good), None, None, 16, 1 << 30,
           None)  # client 1's input not 16-B aligned
    assert rc == 1 and "aligned" in lib.flc_last_error().decode()
    rc = f(c(good), 2, 100, 100, 127, c(seeds), c(ctrs), c(good), c(good), c(good), None, None, 16, 1 << 30, None)
    assert rc == 1 and "0 < k < n" in lib.flc_last_error().decode()
    rc = f(c(good), 2, 100, 10, 127, c(seeds), c(ctrs), c(P(16, 0)), c(good), c(good), None, None, 16, 1 << 30, None)
    assert rc == 1 and "null output of client 1" in lib.flc_last_error().decode()
    # the round's own: no counters; a null count pointer inside a non-null count table
    rc = f(c(good), 2, 100, 10, 127, c(seeds), None, c(good), c(good), c(good), None, None, 16, 1 << 30, None)
    assert rc == 1 and "null counters" in lib.flc_last_error().decode()
    rc = f(c(good), 2, 100, 10, 127, c(seeds), c(ctrs), c(good), c(good), c(good), None, c(P(16, 0)), 16, 1 << 30,
           None)
    assert rc == 1 and "null count of client 1" in lib.flc_last_error().decode()


def test_stacked_encode_delta_round_validates_without_gpu():
    from fl_sim_amd import _lib

    lib = _lib.load()
    P2, P4 = ctypes.c_void_p * 2, ctypes.c_void_p * 4
    sizes, seeds = (ctypes.c_int64 * 2)(100, 100), (ctypes.c_uint64 * 2)(1, 2)
    ctrs = (ctypes.c_uint64 * 2)(5, 1 << 33)
    good2, good4 = P2(16, 32), P4(16, 32, 48, 64)
    f = lib.flc_stacked_encode_delta_round

    def args(loc, glob, k, counters=ctrs, counts=None):
        return (c(loc), c(glob), c(sizes), 2, 2, k, 127, c(seeds), None if counters is None else c(counters),
                c(good2), c(good2), c(good2), None, None if counts is None else c(counts), 16, 1 << 30, None)

    assert f(None, None, None, 2, 2, 10, 127, None, None, None, None, None, None, None, 16, 1 << 30, None) == 1
    assert f(*args(P4(16, 32, 50, 64), good2, 10)) == 1  # client 1's tensor 0
    assert "local tensor 0 of client 1" in lib.flc_last_error().decode()
    assert f(*args(good4, P2(16, 34), 10)) == 1
    assert "global tensor 1" in lib.flc_last_error().decode()
    assert f(*args(good4, good2, 200)) == 1
    assert "0 < k < n" in lib.flc_last_error().decode()
    assert f(*args(good4, good2, 10, counters=None)) == 1
    assert "null counters" in lib.flc_last_error().decode()
    assert f(*args(good4, good2, 10, counts=P2(0, 16))) == 1
    assert "null count of client 0" in lib.flc_last_error().decode()
