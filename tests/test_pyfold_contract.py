"""The host-side contract of fl_sim_amd._flcfold (csrc/pyfold.cpp), entry by entry, without a device: which exception
each rejected input raises (TypeError is the Python callers' cue that nothing was launched and their other path is
open; anything else propagates), which error wins when two inputs are wrong, the early returns, and — through
tests/pyfold_cases.py — that no reference count of an argument moves on any of these paths.  The entries are not
consistent with each other (a count mismatch is a ValueError in model_fold and a TypeError in fold_record_groups):
that is recorded here as it is."""

import pytest
import torch

from fl_sim_amd import _flcfold as fold
from tests.pyfold_cases import FOLD, SRV, STEP, accepted, rejected, snapshot, unchanged

N, K = 8, 2  # the model below as one flat vector; (N, K) and (N, 0, 8) have nonzero wire layouts


def model():
    return [torch.zeros(5), torch.zeros(0), torch.zeros(3)]


def rec():
    return torch.zeros(256, dtype=torch.uint8)


def test_model_fold():
    d, m = model(), model()
    snap = snapshot(d, m)
    rejected(TypeError, "HIP", fold.model_fold, d, [m], None, [0.5], *FOLD)
    rejected(TypeError, "HIP", fold.model_fold, d, [{"p": m}], "p", [0.5], *FOLD)
    rejected(TypeError, "dsts must be a sequence", fold.model_fold, 5, [m], None, [0.5], *FOLD)
    rejected(TypeError, "messages must be a sequence", fold.model_fold, d, 5, None, [0.5], *FOLD)
    rejected(TypeError, "weights must be a sequence", fold.model_fold, d, [m], None, 0.5, *FOLD)
    rejected(ValueError, "one weight per message", fold.model_fold, d, [m], None, [0.5, 0.5], *FOLD)
    # two errors: the count is decided before any tensor is looked at, the model before theta
    rejected(ValueError, "one weight per message", fold.model_fold, [5], [m], None, [], *FOLD)
    rejected(TypeError, "model tensors", fold.model_fold, d, [m], None, [0.5], 0, 0.0, 5, None, 0, 1.0, 0.0, 0.0)
    # an empty model returns before the messages are looked at
    assert accepted(fold.model_fold, [], [5, m], None, [0.5, "x"], *FOLD) is None
    assert accepted(fold.model_fold, (), (), None, (), *FOLD) is None
    unchanged(snap)


def test_server_fold():
    th, aux, m = model(), model(), model()
    snap = snapshot(th, aux, m)
    rejected(TypeError, "HIP", fold.server_fold, th, aux, [m], None, [0.5], *SRV)
    rejected(TypeError, "HIP", fold.server_fold, th, aux, [{"p": m}], "p", [0.5], *SRV)
    rejected(TypeError, "theta must be a sequence", fold.server_fold, 5, aux, [m], None, [0.5], *SRV)
    rejected(TypeError, "aux must be a sequence", fold.server_fold, th, 5, [m], None, [0.5], *SRV)
    rejected(TypeError, "messages must be a sequence", fold.server_fold, th, aux, 5, None, [0.5], *SRV)
    rejected(TypeError, "weights must be a sequence", fold.server_fold, th, aux, [m], None, 0.5, *SRV)
    rejected(ValueError, "one weight per message", fold.server_fold, th, aux, [m], None, [], *SRV)
    rejected(ValueError, "one aux tensor per model tensor", fold.server_fold, th, aux[:2], [m], None, [0.5], *SRV)
    rejected(ValueError, "at most 16 messages", fold.server_fold, th, aux, [m] * 17, None, [0.5] * 17, *SRV)
    # two errors: weights before aux before the message limit; the limit before the empty model's return
    rejected(ValueError, "one weight per message", fold.server_fold, th, aux[:2], [m] * 17, None, [0.5] * 16, *SRV)
    rejected(ValueError, "one aux tensor per model tensor", fold.server_fold, th, [], [m] * 17, None, [0.5] * 17, *SRV)
    rejected(ValueError, "at most 16 messages", fold.server_fold, [], [], [m] * 17, None, [0.5] * 17, *SRV)
    assert accepted(fold.server_fold, [], [], [5], None, ["x"], *SRV) is None
    unchanged(snap)


def test_avg_and_gradients():
    p, g = model(), model()
    msg = {"parameters": model(), "gradients": model()}
    snap = snapshot(p, g, msg["parameters"], msg["gradients"])
    call = fold.avg_and_gradients
    rejected(TypeError, "HIP", call, p, g, [msg], [0.5], [0.5], 0.0)
    rejected(TypeError, "HIP", call, p, None, [msg], [0.5], [0.5], 0.0, True)
    for bad in range(5):
        args = [p, g, [msg], [0.5], [0.5]]
        args[bad] = 5
        rejected(TypeError, "avg_and_gradients takes sequences", call, *args, 0.0)
    rejected(ValueError, "one gradient buffer per parameter", call, p, g[:2], [msg], [0.5], [0.5], 0.0)
    rejected(ValueError, "one weight of each kind per message", call, p, g, [msg], [], [0.5], 0.0)
    rejected(ValueError, "one weight of each kind per message", call, p, g, [msg], [0.5], [0.5, 0.5], 0.0)
    rejected(ValueError, "at least one message", call, p, g, [], [], [], 0.0)
    # two errors: the buffers' count before the weights' before the empty round, all before the empty model's return
    rejected(ValueError, "one gradient buffer per parameter", call, p, [], [], [0.5], [], 0.0)
    rejected(ValueError, "at least one message", call, [], [], [], [], [], 0.0)
    assert accepted(call, [], [], [5], ["x"], ["y"], 0.0) is None
    assert accepted(call, [], None, [5], ["x"], ["y"], 0.0, True) is None
    unchanged(snap)


def test_stacked_delta_record():
    loc, glo, r, ws = model(), model(), rec(), rec()
    cnt = torch.zeros(1, dtype=torch.int64)
    snap = snapshot(loc, glo, r, ws, cnt)
    call = fold.stacked_delta_record
    rejected(TypeError, "HIP", call, loc, glo, K, 127, 1, 2, r, cnt, ws)
    rejected(TypeError, "local must be a sequence", call, 5, glo, K, 127, 1, 2, r, cnt, ws)
    rejected(TypeError, "global must be a sequence", call, loc, 5, K, 127, 1, 2, r, cnt, ws)
    rejected(ValueError, "one global tensor per local tensor", call, loc, glo[:2], K, 127, 1, 2, r, cnt, ws)
    rejected(ValueError, "one global tensor per local tensor", call, [], [], K, 127, 1, 2, r, cnt, ws)
    # two errors: the counts before the tensors
    rejected(ValueError, "one global tensor per local tensor", call, [5], [], K, 127, 1, 2, 5, 5, 5)
    unchanged(snap)


def test_delta_flat():
    loc, glo = model(), model()
    snap = snapshot(loc, glo)
    rejected(TypeError, "HIP", fold.delta_flat, loc, glo)
    rejected(TypeError, "local must be a sequence", fold.delta_flat, 5, glo)
    rejected(TypeError, "global must be a sequence", fold.delta_flat, loc, 5)
    rejected(ValueError, "one global tensor per local tensor", fold.delta_flat, loc, glo[:2])
    rejected(ValueError, "one global tensor per local tensor", fold.delta_flat, [], [])
    rejected(ValueError, "one global tensor per local tensor", fold.delta_flat, [5], [])
    unchanged(snap)


def test_ef_accumulate():
    loc, glo, e = model(), model(), torch.zeros(N)
    snap = snapshot(loc, glo, e)
    rejected(TypeError, "the memory must be", fold.ef_accumulate, loc, glo, e)
    rejected(TypeError, "the memory must be", fold.ef_accumulate, loc, None, e)
    rejected(TypeError, "the memory must be", fold.ef_accumulate, loc, glo, 5)
    # two errors: the memory is looked at before the lists
    rejected(TypeError, "the memory must be", fold.ef_accumulate, 5, 5, e)
    rejected(TypeError, "the memory must be", fold.ef_accumulate, [], [], e)
    unchanged(snap)


def test_stacked_records_round():
    x, r, ws = [torch.zeros(N), torch.zeros(N)], torch.zeros(2, 256, dtype=torch.uint8), rec()
    cnt = [torch.zeros(1, dtype=torch.int64) for _ in range(2)]
    snap = snapshot(x, r, ws, cnt)
    call = fold.stacked_records_round
    rejected(TypeError, "HIP", call, x, [1, 2], [3, 4], K, 127, r, cnt, ws)
    for bad in (0, 1, 6):
        args = [x, [1, 2], [3, 4], K, 127, r, cnt, ws]
        args[bad] = 5
        rejected(TypeError, "takes sequences", call, *args)
    rejected(TypeError, "takes a sequence of counters", call, x, [1, 2], 5, K, 127, r, cnt, ws)
    rejected(ValueError, "one seed and one count per client", call, x, [1], [3, 4], K, 127, r, cnt, ws)
    rejected(ValueError, "one seed and one count per client", call, x, [1, 2], [3, 4], K, 127, r, cnt[:1], ws)
    rejected(ValueError, "one seed and one count per client", call, [], [], [], K, 127, r, [], ws)
    rejected(ValueError, "one counter per client", call, x, [1, 2], [3], K, 127, r, cnt, ws)
    rejected(TypeError, "", call, x, [1, 2], [3, "x"], K, 127, r, cnt, ws)  # (a counter that is no integer)
    # two errors: the seeds' count before the counters', the counters before any tensor
    rejected(ValueError, "one seed and one count per client", call, x, [1], [3], K, 127, r, cnt, ws)
    rejected(ValueError, "one counter per client", call, [5, 5], [1, 2], [3], K, 127, 5, [5, 5], 5)
    unchanged(snap)


@pytest.mark.parametrize("dense", [False, True])
def test_fold_records(dense):
    d, th, r = model(), model(), rec()
    snap = snapshot(d, th, r)
    call = fold.fold_dense_records if dense else fold.fold_records
    name = "fold_records takes sequences"  # (both entries say fold_records)
    shape = (N, 0, 127, 8) if dense else (N, K, 127)
    rejected(TypeError, "HIP", call, [r], [0.5], *shape, d, th, None, *STEP)
    rejected(TypeError, name, call, 5, [0.5], *shape, d, None, None, *STEP)
    rejected(TypeError, name, call, [r], 0.5, *shape, d, None, None, *STEP)
    rejected(TypeError, name, call, [r], [0.5], *shape, 5, None, None, *STEP)
    rejected(ValueError, "one weight per record", call, [r], [], *shape, d, None, None, *STEP)
    rejected(TypeError, "needs records and server tensors", call, [], [], *shape, d, None, None, *STEP)
    rejected(TypeError, "needs records and server tensors", call, [r], [0.5], *shape, [], None, None, *STEP)
    # two errors: the weights' count (ValueError) before the empty lists (TypeError), those before the tensors
    rejected(ValueError, "one weight per record", call, [], [0.5], *shape, [], None, None, *STEP)
    rejected(TypeError, "needs records and server tensors", call, [], [], *shape, [5], 5, 5, *STEP)
    if dense:  # a negative format is refused before the lists are looked at
        rejected(ValueError, "bad wire shape", call, 5, 5, N, -1, 127, 8, 5, None, None, *STEP)
    unchanged(snap)


def test_fold_record_groups():
    d, r = model(), rec()
    snap = snapshot(d, r)
    call = fold.fold_record_groups
    name = "takes sequences of sequences"
    rejected(TypeError, "HIP", call, [[r]], [[0.5]], [d], N, K, 127)
    rejected(TypeError, name, call, 5, [[0.5]], [d], N, K, 127)
    rejected(TypeError, name, call, [[r]], 5, [d], N, K, 127)
    rejected(TypeError, name, call, [[r]], [[0.5]], 5, N, K, 127)
    rejected(TypeError, name, call, [[r]], [[0.5]], [5], N, K, 127)
    per_group = "one record list, weight list and tensor list per group"
    rejected(TypeError, per_group, call, [], [], [], N, K, 127)
    rejected(TypeError, per_group, call, [[r]], [[0.5]], [d, model()], N, K, 127)
    rejected(TypeError, per_group, call, [[r], []], [[0.5]], [d, model()], N, K, 127)
    rejected(ValueError, "bad wire shape", call, [[r]], [[0.5]], [d], 0, 0, 127)
    rejected(TypeError, "first group's number of tensors", call, [[r]], [[0.5]], [[]], N, K, 127)
    # two errors: the lists per group (TypeError) before the wire shape (ValueError), that before any group
    rejected(TypeError, per_group, call, [[r]], [], [d], 0, 0, 127)
    rejected(ValueError, "bad wire shape", call, [5], [5], [5], 0, 0, 127)
    unchanged(snap)


def test_avg_and_gradient_records():
    p, r = model(), rec()
    msg = {"parameters": model()}
    snap = snapshot(p, r, msg["parameters"])
    call = fold.avg_and_gradient_records
    name = "avg_and_gradient_records takes sequences"
    rejected(TypeError, "HIP", call, p, [msg], [r], [0.5], [0.5], N, K, 127, 0.0)
    rejected(TypeError, "HIP", call, p, None, [r], None, [0.5], N, K, 127, 0.0, True)
    for bad in range(5):
        args = [p, [msg], [r], [0.5], [0.5]]
        args[bad] = 5
        rejected(TypeError, name, call, *args, N, K, 127, 0.0)
    rejected(TypeError, name, call, p, None, 5, None, [0.5], N, K, 127, 0.0)
    per_msg = "one record, one message and one weight of each kind per message"
    rejected(ValueError, per_msg, call, p, [msg], [r], [0.5], [], N, K, 127, 0.0)
    rejected(ValueError, per_msg, call, p, [msg], [r], [], [0.5], N, K, 127, 0.0)
    rejected(ValueError, per_msg, call, p, [], [r], [0.5], [0.5], N, K, 127, 0.0)
    rejected(ValueError, per_msg, call, p, None, [r], None, [], N, K, 127, 0.0)
    rejected(TypeError, "needs records and model tensors", call, p, [], [], [], [], N, K, 127, 0.0)
    rejected(TypeError, "needs records and model tensors", call, [], [msg], [r], [0.5], [0.5], N, K, 127, 0.0)
    # two errors: the counts (ValueError) before the empty lists (TypeError), those before the tensors
    rejected(ValueError, per_msg, call, [], [msg], [], [0.5], [], N, K, 127, 0.0)
    rejected(TypeError, "needs records and model tensors", call, [], [5], [5], [5], [5], N, K, 127, 0.0)
    unchanged(snap)


def test_entries():
    """The entry points that exist (alias, the pinned-memory view, is not part of the table layer)."""
    names = {n for n in dir(fold) if not n.startswith("_")}
    assert {"model_fold", "server_fold", "avg_and_gradients", "fold_records", "fold_dense_records",
            "fold_record_groups", "avg_and_gradient_records", "delta_flat", "ef_accumulate", "stacked_records_round",
            "stacked_delta_record", "alias"} <= names
