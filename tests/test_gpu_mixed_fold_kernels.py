"""The mixed folds at the C ABI (flc_fedopt_fold_mixed_records, flc_fold_mixed_record_groups,
flc_avg_and_gradient_mixed_records): rounds whose records differ in kind, K, levels and code width, bit for bit against
the two-step route — every record decoded by its own decoder (flc_stacked_decode_tiled, flc_sparse_decode_tiled,
flc_quant_decode, flc_natural_decode) into a vector, then the dense entry points (flc_model_fold, flc_weighted_sum,
flc_avg_and_gradients) — and, for uniform descriptor lists, against the uniform record entry points.  The records come
from the existing encoders (philox mode); the expected values never come from the new fold."""

import ctypes

import numpy as np
import pytest
import torch

from tests import golden_cases as gc

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
STACKED, SPARSE, DENSE, FLAT = 0, 1, 2, 3
SHAPES = {3077: [(1021,), (2, 1028)], 4097: [(4097,)], 70001: [(30001,), (40000,)]}
WEIGHTS = (0.37, -1.5, 3e-39, -3e-39, 0.0, 1.0)
# kinds alternate, then form runs (two 8-bit, a 4-bit natural dithering and two 4-bit standard ones — one run of one code
# width over two level tables —, four entry records of three K, two flat, two natural)
ORDER = ("stk100", "std8", "top50", "std4", "flat", "natural", "std2", "natd4", "top1", "stk10",
         "std8", "std8", "natd4", "std4", "std4", "stk100", "top50", "stk10", "top1", "flat", "flat", "natural", "natural")


def _ptrs(ts):
    return ctypes.cast((P * max(len(ts), 1))(*[t if isinstance(t, int) else t.data_ptr() for t in ts]), P)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _arr(ct, xs):
    return ctypes.cast((ct * max(len(xs), 1))(*xs), P)


class Rec:
    """One record: the tensor the fold reads, its descriptor, and its decoded vector (by the record's own decoder)."""

    def __init__(self, tensor, kind, k=0, fmt=0, levels=0, bits=0, decoded=None):
        self.t, self.kind, self.k, self.fmt, self.levels, self.bits, self.decoded = tensor, kind, k, fmt, levels, bits, decoded


def _comp(name, n, seed):
    from fl_sim_amd import Compressor

    def std(L):
        c = Compressor(rng="philox", seed=seed, extended_levels=True)  # (levels above 10)
        nc = Compressor("norm")
        nc.makeIdenticalCompressor()
        c.makeStandardDitheringFP32(L, nc, np.inf)
        return c

    def topk(k):
        c = Compressor(rng="philox", seed=seed)
        c.makeTopKCompressor(k, n)
        return c

    if name == "natural":
        c = Compressor(rng="philox", seed=seed)
        c.makeNaturalCompressorFP32()
        return [c]
    if name == "natd4":
        c = Compressor(rng="philox", seed=seed)
        c.makeNaturalDitheringFP32(7, n)
        return [c]
    return {"stk100": lambda: [topk(max(n // 100, 1)), std(10)], "stk10": lambda: [topk(n // 10), std(127)],
            "half_a": lambda: [topk(n // 2), std(127)], "half_b": lambda: [topk(n // 2), std(10)],
            "top50": lambda: [topk(n // 50)], "top1": lambda: [topk(1)],
            "std8": lambda: [std(127)], "std4": lambda: [std(7)], "std2": lambda: [std(1)]}[name]()


def _decode(d):
    from fl_sim_amd import codec

    if d.kind in ("quant", "natural"):
        return codec.dense_record_decode(d.record, d.n, d.format, d.levels, d.bits)
    if d.kind == "sparse":
        return codec.sparse_record_decode(d.record, d.n, d.k)
    return codec.stacked_decode(codec.wire_packet(d.record, d.n, d.k, d.levels))


_CACHE: dict = {}


def records(n):
    """name -> Rec for every codec of the record set at ``n`` (made once; never written afterwards)."""
    if n in _CACHE:
        return _CACHE[n]
    from fl_sim_amd import compressed

    g = torch.Generator().manual_seed(1000 + n)
    out = {}
    names = ("stk100", "stk10", "half_a", "half_b", "top50", "top1", "std8", "std4", "std2", "natd4", "natural")
    for i, name in enumerate(names):
        x = torch.randn(n, generator=g) * 1e-2
        x[torch.rand(n, generator=g) < 0.05] = 0.0  # 5 % exact zeros
        d = compressed.compress_tensors([x.cuda()], _comp(name, n, 31 + i), wire=True, sparse=True)
        want = {"stk": "stacked", "hal": "stacked", "top": "sparse", "std": "quant", "nat": "quant"}[name[:3]]
        assert d.kind == ("natural" if name == "natural" else want), (name, d.kind)
        dec = _decode(d)
        kind = {"stacked": STACKED, "sparse": SPARSE}.get(d.kind, DENSE)
        out[name] = Rec(d.record, kind, d.k, d.format or 0, d.levels, d.bits, dec)
    assert (out["std8"].bits, out["std4"].bits, out["std2"].bits, out["natd4"].bits) == (8, 4, 2, 4)
    assert (out["std4"].fmt, out["natd4"].fmt, out["natural"].fmt, out["natural"].bits) == (0, 1, 2, 16)
    assert out["stk100"].k == max(n // 100, 1) and out["top1"].k == 1 and out["half_a"].k == n // 2
    flat = out["std8"].decoded.clone()
    out["flat"] = Rec(flat, FLAT, decoded=flat)
    # one dense record with its norm field set to 0 and one to NaN (every nonzero code then decodes to NaN)
    for name, bits in (("norm0", 0), ("normnan", 0x7fc00000)):
        src = out["std4" if name == "norm0" else "std8"]
        r = src.t.clone()
        r[:4] = torch.tensor(list(int(bits).to_bytes(4, "little")), dtype=torch.uint8)
        from fl_sim_amd import codec

        out[name] = Rec(r, DENSE, 0, src.fmt, src.levels, src.bits,
                        codec.dense_record_decode(r, n, src.fmt, src.levels, src.bits))
        assert torch.isnan(out[name].decoded).any() and (out[name].decoded == 0).any()
    torch.cuda.synchronize()
    _CACHE[n] = out
    return out


def _desc(rs):
    return (_arr(ctypes.c_int32, [r.kind for r in rs]), _arr(ctypes.c_int64, [r.k for r in rs]),
            _arr(ctypes.c_int32, [r.fmt for r in rs]), _arr(ctypes.c_int32, [r.levels for r in rs]),
            _arr(ctypes.c_int32, [r.bits for r in rs]))


def _weights(m, shift=0):
    return [WEIGHTS[(i + shift) % len(WEIGHTS)] for i in range(m)]


def _state(n, seed, groups=3, minus_zero=False):
    """`groups` server tensor lists of the shapes at ``n``, cut from one misaligned flat buffer each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(groups):
        base = (torch.randn(n + 8, generator=g) * 1e-2).cuda()
        if minus_zero:
            base.fill_(-0.0)
        flat, ts, off = base[4:4 + n], [], 0
        for sh in SHAPES[n]:
            m = int(np.prod(sh))
            ts.append(flat[off:off + m].view(sh))
            off += m
        out.append(ts)
    return out


def _clone(groups):
    return [[t.clone() for t in ts] for ts in groups]


def _views(flat, n):
    ts, off = [], 0
    for sh in SHAPES[n]:
        m = int(np.prod(sh))
        ts.append(flat[off:off + m].view(sh))
        off += m
    return ts


def _same(a, b, what=""):
    for x, y in zip(a, b):
        assert gc.same_bits(x.cpu().numpy(), y.cpu().numpy()), what


def _opt_args(opt, beta0):
    return (beta0, 1.0, 1.0, 1.0) if opt == "avg" else (beta0, 0.01, 0.99, 1e-3)


def _fedopt_mixed(rs, ws, n, delta, theta, v, opt, beta0, lr, beta2, tau):
    from fl_sim_amd import _lib

    sizes = [t.numel() for t in delta]
    _lib.call("flc_fedopt_fold_mixed_records", _ptrs([r.t for r in rs]), _arr(ctypes.c_float, ws), len(rs), n,
              *_desc(rs), _ptrs(delta), _ptrs(theta) if theta is not None else None,
              _ptrs(v) if v is not None else None, _arr(ctypes.c_int64, sizes), len(sizes), beta0, _lib.FLC_OPT[opt],
              lr, beta2, tau, _st())


def _fedopt_reference(rs, ws, n, delta, theta, v, opt, beta0, lr, beta2, tau):
    from fl_sim_amd import codec

    codec.model_fold(delta, [_views(r.decoded, n) for r in rs], ws, 0, beta0, theta=theta, v=v, opt=opt, lr=lr,
                     beta2=beta2, tau=tau)


def _run_fedopt(rs, ws, n, opt, beta0, seed=5, minus_zero=False):
    theta, delta, v = _state(n, seed)
    v = [t.abs() + 1e-6 for t in v]
    if minus_zero:
        delta = _state(n, seed, 1, minus_zero=True)[0]
    a, b = _clone([theta, delta, v]), _clone([theta, delta, v])
    beta0, lr, beta2, tau = _opt_args(opt, beta0)
    _fedopt_mixed(rs, ws, n, a[1], a[0], None if opt == "avg" else a[2], opt, beta0, lr, beta2, tau)
    _fedopt_reference(rs, ws, n, b[1], b[0], None if opt == "avg" else b[2], opt, beta0, lr, beta2, tau)
    torch.cuda.synchronize()
    for x, y, what in zip(a, b, ("theta", "delta", "v")):
        _same(x, y, what)


@pytest.mark.parametrize("beta0", [0.0, 0.9])
@pytest.mark.parametrize("opt", ["avg", "adam"])
@pytest.mark.parametrize("n", list(SHAPES))
def test_fedopt_fold_of_every_kind_matches_decode_then_fold(n, opt, beta0):
    R = records(n)
    rs = [R[name] for name in ORDER]
    _run_fedopt(rs, _weights(len(rs)), n, opt, beta0)


@pytest.mark.parametrize("n", list(SHAPES))
def test_minus_zero_accumulator_and_irregular_norms(n):
    """δ pre-filled with -0 (kept by every zero product of a sign-set weight, turned to +0 by the first sign-clear
    one), a dense record whose norm is 0 and one whose norm is NaN, weights shifted so each kind meets each weight."""
    R = records(n)
    rs = [R[name] for name in ("top1", "norm0", "stk100", "normnan", "flat", "std2", "natural", "top50")]
    for shift in range(3):
        _run_fedopt(rs, _weights(len(rs), 3 + shift), n, "avg", 0.0, minus_zero=True)
    _run_fedopt([R["top1"], R["stk100"]], [-1.5, -3e-39], n, "avg", 0.9, minus_zero=True)  # (-0 survives the round)


@pytest.mark.parametrize("n", list(SHAPES))
def test_tiles_of_more_than_128_entries_take_the_per_record_loop(n):
    """Two stacked records of k = n / 2 (another levels each) beside a sparse one: every tile of the run holds ~1000
    entries."""
    R = records(n)
    rs = [R["half_a"], R["top50"], R["half_b"], R["std4"], R["half_a"]]
    _run_fedopt(rs, [0.37, -1.5, 1.0, 3e-39, -0.25], n, "adam", 0.9)


def test_seventy_records_chain_launches():
    n = 4097
    R = records(n)
    names = ("stk100", "std8", "top50", "std4", "flat", "natural", "std2", "natd4", "top1", "stk10")
    rs = [R[names[i % 10]] for i in range(70)]
    for opt in ("avg", "adam"):
        _run_fedopt(rs, _weights(70), n, opt, 0.9)


def test_more_level_tables_than_one_launch_holds():
    """Nine distinct (format, levels, bits) / stacked levels in 11 records: the launch is cut where its tables run out
    and the chain continues from the stored δ.  The extra codecs reuse the records' bytes under other levels — the
    reference decodes them under the same levels."""
    from fl_sim_amd import codec

    n = 4097
    R = records(n)
    rs = [R["stk100"], R["stk10"], R["std8"], R["std4"], R["std2"], R["natd4"]]
    for lv in (100, 50, 9):
        src = R["std8"]
        rs.append(Rec(src.t, DENSE, 0, 0, lv, 8, codec.dense_record_decode(src.t, n, 0, lv, 8)))
    rs += [R["half_b"], R["std8"]]
    _run_fedopt(rs, _weights(len(rs)), n, "adam", 0.9)


@pytest.mark.parametrize("n_groups", [2, 3])
@pytest.mark.parametrize("n", list(SHAPES))
def test_grouped_fold_matches_weighted_sums(n, n_groups):
    from fl_sim_amd import _lib, codec

    R = records(n)
    rs = [R[name] for name in ORDER[:14]]
    ws = _weights(len(rs), 1)
    gof = [i % 2 for i in range(len(rs))] if n_groups == 2 else [0 if i == 5 else 1 + i % 2 for i in range(len(rs))]
    assert n_groups == 2 or gof.count(0) == 1  # (a group with a single record)
    dsts = _state(n, 9, n_groups)
    dsts[-1] = _state(n, 9, 1, minus_zero=True)[0]  # (one group accumulates from -0)
    a, b = _clone(dsts), _clone(dsts)
    sizes = [t.numel() for t in a[0]]
    _lib.call("flc_fold_mixed_record_groups", _ptrs([r.t for r in rs]), _arr(ctypes.c_float, ws),
              _arr(ctypes.c_int32, gof), len(rs), n, *_desc(rs), _ptrs([t for ts in a for t in ts]), n_groups,
              _arr(ctypes.c_int64, sizes), len(sizes), _st())
    for g in range(n_groups):
        members = [i for i in range(len(rs)) if gof[i] == g]
        for j, dst in enumerate(b[g]):
            codec.weighted_sum(dst, [_views(rs[i].decoded, n)[j] for i in members], [ws[i] for i in members], 2)
    torch.cuda.synchronize()
    for g in range(n_groups):
        _same(a[g], b[g], f"group {g}")


@pytest.mark.parametrize("with_params", [True, False])
@pytest.mark.parametrize("n", list(SHAPES))
def test_gradient_fold_matches_avg_and_gradients(n, with_params):
    from fl_sim_amd import _lib, codec

    R = records(n)
    rs = [R[name] for name in ORDER[:10]]
    m = len(rs)
    wg, wp = _weights(m, 2), [0.75 / m] * m
    params = _state(n, 21, 1)[0]
    srcs = _state(n, 22, m)
    a_p, b_p = _clone([params])[0], _clone([params])[0]
    a_g = _views(torch.full((n,), 7.0, device="cuda"), n)  # (the gradients start from +0, whatever they held)
    b_g = _views(torch.full((n,), 9.0, device="cuda"), n)
    sizes = [t.numel() for t in a_g]
    _lib.call("flc_avg_and_gradient_mixed_records", _ptrs(a_p) if with_params else None, _ptrs(a_g),
              _ptrs([t for r in srcs for t in r]) if with_params else None, _ptrs([r.t for r in rs]),
              _arr(ctypes.c_float, wp) if with_params else None, _arr(ctypes.c_float, wg), m, n, *_desc(rs),
              _arr(ctypes.c_int64, sizes), len(sizes), 0.25, _st())
    gsrc = [_views(r.decoded, n) for r in rs]
    if with_params:
        _lib.call("flc_avg_and_gradients", _ptrs(b_p), _ptrs(b_g), _ptrs([t for r in srcs for t in r]),
                  _ptrs([t for r in gsrc for t in r]), _arr(ctypes.c_float, wp), _arr(ctypes.c_float, wg), m,
                  _arr(ctypes.c_int64, sizes), len(sizes), 0.25, _st())
    else:
        codec.model_fold(b_g, gsrc, wg, 1)
    torch.cuda.synchronize()
    _same(a_g, b_g, "gradients")
    _same(a_p, b_p, "parameters")
    if not with_params:
        _same(a_p, params, "parameters untouched")


@pytest.mark.parametrize("name", ["stk100", "top50", "std4", "natd4", "natural"])
@pytest.mark.parametrize("n", [3077, 70001])
def test_uniform_descriptor_list_matches_the_uniform_entry_point(n, name):
    from fl_sim_amd import _lib

    R = records(n)
    r = R[name]
    rs = [r, r, r, r, r]
    ws = _weights(5, 4)
    theta, delta, v = _state(n, 33)
    v = [t.abs() + 1e-6 for t in v]
    a, b = _clone([theta, delta, v]), _clone([theta, delta, v])
    beta0, lr, beta2, tau = _opt_args("adam", 0.9)
    _fedopt_mixed(rs, ws, n, a[1], a[0], a[2], "adam", beta0, lr, beta2, tau)
    sizes = [t.numel() for t in delta]
    tail = (_ptrs(b[1]), _ptrs(b[0]), _ptrs(b[2]), _arr(ctypes.c_int64, sizes), len(sizes), beta0, _lib.FLC_OPT["adam"],
            lr, beta2, tau, _st())
    head = (_ptrs([x.t for x in rs]), _arr(ctypes.c_float, ws), 5, n)
    if r.kind == STACKED:
        _lib.call("flc_fedopt_fold_records", *head, r.k, r.levels, *tail)
    elif r.kind == SPARSE:
        _lib.call("flc_fedopt_fold_sparse_records", *head, r.k, *tail)
    else:
        _lib.call("flc_fedopt_fold_dense_records", *head, r.fmt, r.levels, r.bits, *tail)
    torch.cuda.synchronize()
    for x, y, what in zip(a, b, ("theta", "delta", "v")):
        _same(x, y, what)


def test_pyfold_entry_matches_the_ctypes_call():
    """_flcfold.fold_mixed_records (one C call on the Python lists) against the ctypes call."""
    from fl_sim_amd import _flcfold, _lib

    n = 3077
    R = records(n)
    rs = [R[name] for name in ORDER[:10]]
    ws = _weights(10)
    theta, delta, v = _state(n, 44)
    v = [t.abs() + 1e-6 for t in v]
    a, b = _clone([theta, delta, v]), _clone([theta, delta, v])
    beta0, lr, beta2, tau = _opt_args("adam", 0.9)
    _flcfold.fold_mixed_records([r.t for r in rs], ws, n, [r.kind for r in rs], [r.k for r in rs],
                                [r.fmt for r in rs], [r.levels for r in rs], [r.bits for r in rs], a[1], a[0], a[2],
                                beta0, _lib.FLC_OPT["adam"], lr, beta2, tau)
    _fedopt_mixed(rs, ws, n, b[1], b[0], b[2], "adam", beta0, lr, beta2, tau)
    torch.cuda.synchronize()
    for x, y, what in zip(a, b, ("theta", "delta", "v")):
        _same(x, y, what)
    with pytest.raises(TypeError):  # a flat record that is not the n elements: nothing launched
        _flcfold.fold_mixed_records([torch.zeros(n + 1, device="cuda")], [1.0], n, [FLAT], [0], [0], [0], [0], a[1],
                                    None, None, 0.0, 0, 1.0, 0.0, 0.0)
    for x, y, what in zip(a, b, ("theta", "delta", "v")):
        _same(x, y, what)
