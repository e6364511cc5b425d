"""GPU parity of the dense-record folds (wire.hip dense_fold_records_kernel): flc_fold_dense_wires,
flc_fedopt_fold_dense_records and flc_fold_dense_record_groups against the chains of decodes and dense folds they
replace, bit for bit — every code format, the tile edges and sub-byte tails, chained launches, weights and
accumulators and norms at their edge values, records whose padding holds garbage."""

import ctypes

import numpy as np
import pytest
import torch

from tests import golden_cases as gc

pytestmark = pytest.mark.gpu
P = ctypes.c_void_p
STD, NATD, NATURAL = 0, 1, 2
# (format, bits, levels)
FORMATS = [(k, b, s) for k in (STD, NATD) for b, s in ((2, 1), (4, 4), (4, 7), (8, 8), (8, 127))] + [(NATURAL, 16, 0)]
SIZES = [1, 5, 1023, 1024, 1025, 4097, 70001]
RECORDS = [1, 3, 10, 65]
MAXR = max(RECORDS)
WEIGHTS = [0.37, -1.5, 3e-39, 0.0, 1.0]
NORM_EDGES = [0.0, float("inf"), float("nan"), 1e-40, 2.5]  # 0, +inf, NaN, a subnormal, a regular value


def _fid(f):
    return f"{('std', 'natd', 'natural')[f[0]]}{f[1]}s{f[2]}"


_BLOCKS: dict = {}


def _block(fmt, bits, s, n):
    """[MAXR, stride] records of MAXR inputs of n elements (made once per (format, n)): every buffer 0xAB before the
    encode; inputs with exact zeros, values of both signs, and small negative values that land on level 0 (code =
    sign bit alone: the -0 decode)."""
    from fl_sim_amd import _lib, codec

    key = (fmt, bits, s, n)
    if key not in _BLOCKS:
        stride, _ = codec.dense_wire_layout(n, fmt, bits)
        wires = torch.full((MAXR, stride), 0xAB, dtype=torch.uint8, device="cuda")
        g = torch.Generator(device="cuda").manual_seed(1000 * n + 10 * bits + fmt + s)
        st = codec._stream(wires.device)
        for r in range(MAXR):
            x = torch.randn(n, generator=g, device="cuda") * 1e-2
            x[torch.rand(n, generator=g, device="cuda") < 0.1] = 0.0
            tiny = torch.rand(n, generator=g, device="cuda") < 0.2
            x[tiny] = -x[tiny].abs() * 1e-4  # (far below the first level: they land on level 0 with their sign)
            if n > 3:
                x[n - 1] = 0.05  # (the norm, so the small values stay small beside it)
            norm, codes = codec.dense_wire_views(wires[r], n, fmt, bits)
            if fmt == NATURAL:
                ws = codec.workspace(x.device, codec._ws_size(x.device, "flc_natural_workspace_size", n), "natural")
                _lib.call("flc_natural_encode", x.data_ptr(), n, 7 + r, 3, None, codes.data_ptr(), None, ws.data_ptr(),
                          ws.numel(), st)
            else:
                ws = codec.workspace(x.device, codec._ws_size(x.device, "flc_quant_workspace_size", 1, n), "quant")
                _lib.call("flc_quant_norm", x.data_ptr(), 1, n, _lib.FLC_NORM_INF, norm.data_ptr(), ws.data_ptr(),
                          ws.numel(), st)
                _lib.call("flc_quant_encode", x.data_ptr(), 1, n, fmt, s, bits, norm.data_ptr(), 7 + r, 3, None,
                          codes.data_ptr(), None, ws.data_ptr(), ws.numel(), st)
        torch.cuda.synchronize()
        _BLOCKS[key] = wires
    return _BLOCKS[key]


def _with_norms(wires, fmt, bits, n, R):
    """A copy of the first R records with the norm fields of records 1.. set to the edge values, in turn (record 0
    keeps its own); the natural compressor's records get the same bytes (its fold must ignore them)."""
    w = wires[:R].clone()
    for r in range(1, R):
        w[r, 0:4].view(torch.float32)[0] = NORM_EDGES[(r - 1) % len(NORM_EDGES)]
    return w


def _decode(rec, fmt, bits, s, n, weight=None, out=None):
    """flc_quant_decode(row_weights = weight, accumulate = 1) / flc_natural_decode(weight, accumulate = 1) into out;
    without a weight, the plain dense decode."""
    from fl_sim_amd import _lib, codec

    norm, codes = codec.dense_wire_views(rec, n, fmt, bits)
    st = codec._stream(rec.device)
    acc = int(weight is not None)
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=rec.device)
    if fmt == NATURAL:
        _lib.call("flc_natural_decode", codes.data_ptr(), n, 1.0 if weight is None else float(weight), acc,
                  out.data_ptr(), st)
    else:
        rw = None if weight is None else torch.tensor([weight], dtype=torch.float32, device=rec.device)
        _lib.call("flc_quant_decode", codes.data_ptr(), 1, n, fmt, s, bits, norm.data_ptr(),
                  None if rw is None else rw.data_ptr(), acc, out.data_ptr(), st)
        torch.cuda.synchronize()  # (rw stays alive until the launch has read it)
    return out


def _seed_acc(n, seed):
    """An accumulator with -0, +-inf and NaN lanes among ordinary values."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(n, generator=g, device="cuda") * 1e-2
    for i, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"), 0.0)):
        a[i::11][: max(1, n // 50)] = v
    return a


def _bits(t):
    return t.detach().cpu().numpy().reshape(-1)


@pytest.mark.parametrize("R", RECORDS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fmt", FORMATS, ids=_fid)
def test_fold_dense_wires_equals_the_decode_chain(fmt, n, R):
    from fl_sim_amd import codec

    kind, bits, s = fmt
    block = _block(kind, bits, s, n)
    ws = [WEIGHTS[c % len(WEIGHTS)] for c in range(R)]
    slots = list(range(R))[::-1]  # (the fold order is the slots', not the block's)
    variants = {"own_norms": block[:R]}
    if R > 1:
        variants["edge_norms"] = _with_norms(block, kind, bits, n, R)
    for label, wires in variants.items():
        for accumulate in (0, 1):
            seed = _seed_acc(n, 5 * n + R)
            got = seed.clone() if accumulate else torch.full((n,), float("nan"), device="cuda")
            codec.fold_dense_wires(wires, slots, ws, n, kind, s, bits, out=got, accumulate=bool(accumulate))
            want = seed.clone() if accumulate else torch.zeros(n, device="cuda")
            for c in range(R):
                _decode(wires[slots[c]], kind, bits, s, n, weight=ws[c], out=want)
            torch.cuda.synchronize()
            assert gc.same_bits(_bits(got), _bits(want)), (label, accumulate)
    # the inputs do hold the -0 decode: a code that is the sign bit alone (natural dithering with 127 levels has its
    # first level at 2^-126 of the norm, below every input here)
    if kind != NATURAL and n >= 1023 and not (kind == NATD and s > 30):
        dec = _bits(_decode(block[0], kind, bits, s, n))
        assert (dec.view(np.uint32) == 0x80000000).any() and (dec.view(np.uint32) == 0).any()


def test_padding_bytes_do_not_matter():
    """The same records in buffers pre-filled with other bytes fold to the same vector."""
    from fl_sim_amd import codec

    for kind, bits, s in [(STD, 2, 1), (STD, 4, 7), (NATD, 8, 8), (NATURAL, 16, 0)]:
        n = 1025
        a = _block(kind, bits, s, n)[:3].contiguous()
        stride, off = codec.dense_wire_layout(n, kind, bits)
        used = off["codes"] + (2 * n if kind == NATURAL else (n * bits + 7) // 8)
        b = a.clone()
        b[:, used:] = 0x5C
        b[:, 4:16] = 0xFF
        if kind != NATURAL and (n * bits) % 8:  # the unused high bits of the last code byte
            last = used - 1
            keep = (1 << ((n * bits) % 8)) - 1
            b[:, last] = (b[:, last] & keep) | (0xFF & ~keep)
        x = codec.fold_dense_wires(a, [0, 1, 2], [0.5, -1.0, 2.0], n, kind, s, bits)
        y = codec.fold_dense_wires(b, [0, 1, 2], [0.5, -1.0, 2.0], n, kind, s, bits)
        torch.cuda.synchronize()
        assert gc.same_bits(_bits(x), _bits(y)), (kind, bits)


# ------------------------------------------------------------------------------------------------ the FedOpt fold
def _cut(flat, sizes):
    ts, off = [], 0
    for m in sizes:
        ts.append(flat[off:off + m])
        off += m
    return ts


def _splits(n):
    out = {"one": [n]}
    if n > 1025:
        out["unaligned"] = [3, 1021, 1, n - 1025]
        q = n // 17
        out["seventeen"] = [q] * 16 + [n - 16 * q]
    return out


def _state(n, sizes, seed, lead):
    """theta, delta, v cut from one buffer ``lead`` elements in (lead 1: no tensor is 16-B aligned but by accident)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    span = (n + lead + 3) // 4 * 4
    base = torch.randn(3 * span, generator=g, device="cuda") * 1e-2
    base[2 * span:].abs_().add_(1e-6)
    flats = [base[i * span + lead: i * span + lead + n] for i in range(3)]
    for i, v in enumerate((-0.0, float("inf"), float("-inf"), float("nan"))):
        flats[1][7 + i::13][: max(1, n // 100)] = v  # δ: -0, +-inf and NaN lanes
    return base, [_cut(f, sizes) for f in flats]


def _dense_fedopt(recs, ws, fmt, n, sizes, state, beta0, opt, lr, beta2, tau, step):
    """Every record decoded densely, then flc_model_fold(init_mode 0) with the step (chained beyond 16 messages)."""
    from fl_sim_amd import codec

    kind, bits, s = fmt
    theta, delta, v = state
    srcs = [_cut(_decode(r, kind, bits, s, n), sizes) for r in recs]
    codec.model_fold(delta, srcs, ws, 0, beta0, theta=theta if step else None,
                     v=v if (step and opt != "avg") else None, opt=opt, lr=lr, beta2=beta2, tau=tau)
    torch.cuda.synchronize()


def _fused_fedopt(recs, ws, fmt, n, sizes, state, beta0, opt, lr, beta2, tau, step):
    from fl_sim_amd import _lib

    kind, bits, s = fmt
    theta, delta, v = state
    m, T = len(recs), len(sizes)
    ptr = lambda ts: (P * T)(*[t.data_ptr() for t in ts])  # noqa: E731
    _lib.call("flc_fedopt_fold_dense_records", (P * m)(*[r.data_ptr() for r in recs]), (ctypes.c_float * m)(*ws), m, n,
              kind, s, bits, ptr(delta), ptr(theta) if step else None, ptr(v) if (step and opt != "avg") else None,
              (ctypes.c_int64 * T)(*sizes), T, beta0, _lib.FLC_OPT[opt], lr, beta2, tau, None)
    torch.cuda.synchronize()


FEDOPT_CASES = [(f, n, R) for f in FORMATS for n, R in ((4097, 3), (70001, 10))] + \
               [(f, 2049, 65) for f in ((STD, 4, 7), (NATD, 8, 127), (NATURAL, 16, 0))] + \
               [(f, n, 3) for f in ((STD, 2, 1), (STD, 8, 8), (NATURAL, 16, 0)) for n in (1, 5, 1023, 1024)]


@pytest.mark.parametrize("fmt,n,R", FEDOPT_CASES, ids=lambda v: _fid(v) if isinstance(v, tuple) else str(v))
def test_fedopt_fold_dense_records_equals_decode_then_model_fold(fmt, n, R):
    """All four optimisers and theta == NULL; one tensor, a split with unaligned starts and tensor borders inside a
    tile, a 17-tensor split (a chain of two tensor launches); 65 records (a chain of two record launches); δ with
    -0 / +-inf / NaN lanes; the weights' edge values; norms at their edge values."""
    kind, bits, s = fmt
    block = _with_norms(_block(kind, bits, s, n), kind, bits, n, R) if R == 10 else _block(kind, bits, s, n)[:R]
    recs = [block[r] for r in range(R)]
    ws = [WEIGHTS[c % len(WEIGHTS)] for c in range(R)]
    for name, sizes in _splits(n).items():
        for opt, step in (("avg", True), ("adagrad", True), ("yogi", True), ("adam", True), ("avg", False)):
            beta0, lr, beta2, tau = (0.0, 1.0, 1.0, 1.0) if opt == "avg" else (0.9, 0.01, 0.99, 1e-3)
            lead = 0 if name == "one" else 1
            base_a, a = _state(n, sizes, n + R, lead)
            base_b, b = _state(n, sizes, n + R, lead)
            _fused_fedopt(recs, ws, fmt, n, sizes, a, beta0, opt, lr, beta2, tau, step)
            _dense_fedopt(recs, ws, fmt, n, sizes, b, beta0, opt, lr, beta2, tau, step)
            assert gc.same_bits(_bits(base_a), _bits(base_b)), (name, opt, step)


@pytest.mark.parametrize("ext", [True, False])
@pytest.mark.parametrize("fmt", [(STD, 4, 7), (NATURAL, 16, 0)], ids=_fid)
def test_fold_records_function_takes_dense_records(fmt, ext, monkeypatch):
    """compressed.fold_records on dense records — through the one-C-call extension entry (_flcfold.fold_dense_records)
    and (``ext`` False: as when the extension is not built) through ctypes."""
    from fl_sim_amd import codec
    from fl_sim_amd.compressed import CompressedDelta, fold_records

    if ext:
        assert codec._pydrecs() is not None, "the _flcfold extension must be built"
    else:
        monkeypatch.setattr(codec, "_PYDRECS", [None])
    kind, bits, s = fmt
    n, R = 4097, 10
    block = _block(kind, bits, s, n)
    ds = [CompressedDelta([torch.Size([n])], block.device, n, record=block[r], levels=s, format=kind, bits=bits)
          for r in range(R)]
    assert all(d.kind == ("natural" if kind == NATURAL else "quant") for d in ds)
    sizes = _splits(n)["unaligned"]
    ws = [0.1] * R
    base_a, a = _state(n, sizes, 3, 1)
    base_b, b = _state(n, sizes, 3, 1)
    assert fold_records(ds, ws, a[1], a[0], a[2], 0.9, "adam", 0.01, 0.99, 1e-3)
    torch.cuda.synchronize()
    _dense_fedopt([block[r] for r in range(R)], ws, fmt, n, sizes, b, 0.9, "adam", 0.01, 0.99, 1e-3, True)
    assert gc.same_bits(_bits(base_a), _bits(base_b))
    assert all(d._flat is None for d in ds)
    assert gc.same_bits(_bits(ds[2].flat()), _bits(_decode(block[2], kind, bits, s, n)))  # (the message decodes itself)


# ------------------------------------------------------------------------------------------------ the grouped fold
@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n", [1025, 4097])
@pytest.mark.parametrize("fmt", FORMATS, ids=_fid)
def test_fold_dense_record_groups_equals_weighted_sums(fmt, n, n_groups):
    """Per group flc_weighted_sum(init_mode 2) on the decoded vectors: 1 and 3 groups with records plus one without
    (never read or written), the records interleaved; -0 / +-inf / NaN accumulators; the weights' edge values; a group
    of 66 records in the 3-group case (a chain of launches)."""
    from fl_sim_amd import _lib, codec

    kind, bits, s = fmt
    block = _with_norms(_block(kind, bits, s, n), kind, bits, n, MAXR) if n == 1025 else _block(kind, bits, s, n)
    if n_groups == 1:
        gof = [0] * 7
        rec_ids = list(range(7))
    else:  # groups 0 and 3 small, group 2 with 66 records (MAXR distinct ones, one twice); group 1 idle
        rec_ids = list(range(MAXR)) + [3] + [5, 9, 11, 2]
        gof = [2] * (MAXR + 1) + [0, 3, 0, 3]
        order = np.random.RandomState(n).permutation(len(rec_ids))
        rec_ids, gof = [rec_ids[i] for i in order], [gof[i] for i in order]
    G = max(gof) + 2  # (one idle group at the end too)
    ws = [WEIGHTS[c % len(WEIGHTS)] for c in range(len(rec_ids))]
    sizes = _splits(n)["unaligned"] if n > 1025 else [1021, 4]
    T = len(sizes)

    def dests():
        base = torch.cat([_seed_acc(n + 3, 40 + g) for g in range(G)])
        return base, [_cut(base[g * (n + 3) + 1: g * (n + 3) + 1 + n], sizes) for g in range(G)]

    base_a, a = dests()
    base_b, b = dests()
    m = len(rec_ids)
    idle = [g for g in range(G) if g not in gof]
    dptr = [0 if g in idle else t.data_ptr() for g in range(G) for t in a[g]]  # (an idle group's pointers may be NULL)
    _lib.call("flc_fold_dense_record_groups", (P * m)(*[block[r].data_ptr() for r in rec_ids]),
              (ctypes.c_float * m)(*ws), (ctypes.c_int32 * m)(*gof), m, n, kind, s, bits, (P * (G * T))(*dptr), G,
              (ctypes.c_int64 * T)(*sizes), T, None)
    for g in range(G):
        mem = [c for c in range(m) if gof[c] == g]
        if not mem:
            continue
        dec = [_cut(_decode(block[rec_ids[c]], kind, bits, s, n), sizes) for c in mem]
        for j, t in enumerate(b[g]):
            codec.weighted_sum(t, [d[j] for d in dec], [ws[c] for c in mem], init_mode=2)
    torch.cuda.synchronize()
    assert gc.same_bits(_bits(base_a), _bits(base_b))
    fresh, _ = dests()
    for g in idle:  # untouched, bit for bit
        lo, hi = g * (n + 3), (g + 1) * (n + 3)
        assert gc.same_bits(_bits(base_a[lo:hi]), _bits(fresh[lo:hi]))


def test_folds_reject_bad_arguments_on_the_device():
    from fl_sim_amd import _lib, codec

    n = 5000
    stride, _ = codec.dense_wire_layout(n, STD, 4)
    rec = torch.zeros(stride, dtype=torch.uint8, device="cuda")
    d = torch.ones(n, device="cuda")
    one = (ctypes.c_float * 1)(1.0)
    with pytest.raises(_lib.FlcError, match="hold"):
        _lib.call("flc_fedopt_fold_dense_records", (P * 1)(rec.data_ptr()), one, 1, n, STD, 7, 4,
                  (P * 1)(d.data_ptr()), None, None, (ctypes.c_int64 * 1)(n - 1), 1, 0.0, 0, 1.0, 0.0, 0.0, None)
    with pytest.raises(_lib.FlcError, match="aligned"):
        _lib.call("flc_fedopt_fold_dense_records", (P * 1)(rec.data_ptr() + 4), one, 1, n, STD, 7, 4,
                  (P * 1)(d.data_ptr()), None, None, (ctypes.c_int64 * 1)(n), 1, 0.0, 0, 1.0, 0.0, 0.0, None)
    with pytest.raises(_lib.FlcError, match="does not fit"):
        codec.fold_dense_wires(rec.reshape(1, -1), [0], [1.0], n, STD, 8, 4, out=d, accumulate=True)
    torch.cuda.synchronize()
    assert bool((d == 1).all())  # (nothing launched)
