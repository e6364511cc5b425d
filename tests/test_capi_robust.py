"""flc_robust_fold's argument validation, which happens before anything touches the device, so it runs without one
(the pointers are never dereferenced; FLC_EINVAL means nothing was launched), and the mixin's two switches."""

import ctypes
import types

import numpy as np
import pytest
import torch

P = ctypes.c_void_p
FN = "flc_robust_fold"


def _args(n_src=5, sizes=(1000, 2000), rule=1, trim=1, opt=3, v=True):
    tab = lambda base, k: ctypes.cast((P * k)(*[base + 0x10000 * i for i in range(k)]), P)  # noqa: E731
    return (tab(0x10000, 2), tab(0x100000, 2 * max(n_src, 1)), n_src, ctypes.cast((ctypes.c_int64 * 2)(*sizes), P), 2,
            rule, trim, 1.0, 0, 0.9, tab(0x30000, 2), tab(0x50000, 2) if v else None, opt, 0.1, 0.99, 1e-3, None)


@pytest.mark.parametrize("kw,message", [
    (dict(n_src=0, trim=0), "n_src must be"), (dict(n_src=65), "n_src must be"), (dict(n_src=4, trim=2), "trim must"),
    (dict(trim=3), "trim must"), (dict(trim=-1), "trim must"), (dict(rule=2), "unknown rule"),
    (dict(rule=-1), "unknown rule"), (dict(opt=4), "unknown opt"), (dict(v=False), "v required"),
    (dict(sizes=(1000, -1)), "negative sizes[1]")])
def test_robust_fold_validates_without_gpu(kw, message):
    from fl_sim_amd import _lib as L

    lib = L.load()
    assert FN in L.SIGNATURES and L.FLC_ROBUST == {"median": 0, "trimmed_mean": 1}
    assert getattr(lib, FN)(*_args(**kw)) == 1  # FLC_EINVAL
    err = lib.flc_last_error().decode()
    assert message in err and FN in err, err


@pytest.mark.parametrize("robust,trim,n", [("mean", 0, 10), ("trimmed_mean", 0.5, 10), ("trimmed_mean", -1, 10),
                                           ("trimmed_mean", 5, 10), ("trimmed_mean", np.int64(2), 4),
                                           ("trimmed_mean", "0.2", 10), ("median", 0, 65)])
@pytest.mark.parametrize("on_config", [False, True])
def test_mixin_switches_raise_before_anything_is_launched(robust, trim, n, on_config):
    from fl_sim_amd import ROBUST_MAX_SRC, ROBUST_RULES
    from fl_sim_amd.aggregation import FedOptUpdateMixin, robust_rule

    assert ROBUST_MAX_SRC == 64 and ROBUST_RULES == ("median", "trimmed_mean")
    assert robust_rule(None, 3, 10) is None and robust_rule("median", 3, 10) == ("median", 0)
    assert [robust_rule("trimmed_mean", t, 10)[1] for t in (0.2, np.float32(0.2), 4, np.int64(4), 0.49)] == [2, 2, 4, 4, 4]
    s = type("Server", (FedOptUpdateMixin,), {})()
    s.v_parameters, s.delta_parameters = None, [torch.zeros(3)]
    s.config = types.SimpleNamespace(optimizer="avg", lr=1, betas=(0, 1), tau=1)
    vars(s.config if on_config else s).update(robust=robust, robust_trim=trim)
    s._received_messages = [{"delta_parameters": [torch.zeros(3)]} for _ in range(n)]
    with pytest.raises(ValueError):
        s.update()
    s.robust, s.robust_trim, s.sketch_k, s._received_messages = "median", 0, 8, s._received_messages[:3]
    with pytest.raises(ValueError, match="sketch"):
        s.update()
