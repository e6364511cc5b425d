"""Shared pieces of the _flcfold contract tests (tests/test_pyfold_contract.py, tests/test_gpu_pyfold_contract.py):
calls into fl_sim_amd._flcfold (csrc/pyfold.cpp) wrapped so that every one also checks the reference counts of what
it was given — the leak and double-release check of the extension's reference handling."""

import sys

import torch

# the scalar tails of the entry points' argument lists (values that pass every check)
FOLD = (0, 0.0, None, None, 0, 1.0, 0.0, 0.0)  # model_fold: init_mode, beta, theta, v, opt, lr, beta2, tau
SRV = (1, 1, 0, 0.0, 0.0)  # server_fold: kind (FLC_SRV_FEDDYN), fold, init_mode, inertia, c
STEP = (0.0, 0, 1.0, 0.0, 0.0)  # fold_records / fold_dense_records: beta0, opt, lr, beta2, tau


def _walk(o, out, seen):
    if id(o) in seen or not isinstance(o, (list, tuple, dict, torch.Tensor)):
        return
    seen.add(id(o))
    out.append(o)
    if not isinstance(o, torch.Tensor):
        for x in (o.values() if isinstance(o, dict) else o):
            _walk(x, out, seen)


def tracked(args):
    """Every container, mapping and tensor reachable from ``args`` (numbers, strings and None are left out: the
    interpreter shares them, so their counts say nothing about the call).  Nothing here keeps a reference to them
    past the caller's own list: a leftover cycle would be freed by the collector at a time of its choosing, and move
    the counts between two readings."""
    out = []
    _walk(args, out, set())
    return out


def _counts(objs):
    return [sys.getrefcount(o) for o in objs]


def _moved(objs, before, after):
    """The arguments whose reference counts differ, for the assertion's message."""
    return [(i, type(o).__name__, b, a) for i, (o, b, a) in enumerate(zip(objs, before, after)) if a != b]


def rejected(exc, match, fn, *args):
    """``fn(*args)`` raises exactly ``exc`` with ``match`` in its text, and leaves every argument's reference count as
    it was."""
    objs = tracked(args)
    before = _counts(objs)
    try:
        fn(*args)
    except exc as e:
        assert type(e) is exc, f"{type(e).__name__} for {exc.__name__}"
        assert match in str(e), f"{match!r} not in {str(e)!r}"
    else:
        raise AssertionError(f"{fn.__name__} accepted what should raise {exc.__name__} ({match!r})")
    after = _counts(objs)
    assert after == before, (f"{fn.__name__}: reference counts moved on the {exc.__name__} path ({match!r}): "
                             f"{_moved(objs, before, after)}")


def accepted(fn, *args):
    """``fn(*args)`` returns, and leaves every argument's reference count as it was; its result."""
    objs = tracked(args)
    before = _counts(objs)
    out = fn(*args)
    after = _counts(objs)
    assert after == before, f"{fn.__name__}: reference counts moved on the success path: {_moved(objs, before, after)}"
    return out


def snapshot(*tensors):
    """Clones of ``tensors`` (lists of tensors flattened), for unchanged()."""
    flat = []
    for t in tensors:
        flat.extend(t if isinstance(t, (list, tuple)) else [t])
    return flat, [t.clone() for t in flat]


def unchanged(snap):
    """Every tensor of a snapshot() still holds, bit for bit, what it held then."""
    flat, clones = snap
    for t, c in zip(flat, clones):
        assert t.dtype == c.dtype and t.shape == c.shape
        if t.is_floating_point():
            assert torch.equal(t.contiguous().view(-1).view(torch.uint8), c.contiguous().view(-1).view(torch.uint8))
        else:
            assert torch.equal(t, c)
