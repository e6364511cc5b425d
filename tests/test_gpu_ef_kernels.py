"""The error-feedback kernels on the GPU, bit for bit: flc_ef_accumulate against numpy's float32 arithmetic,
flc_ef_residual_round against "dense decode of every record, then subtract", flc_ef_residual_dense against numpy."""

import numpy as np
import pytest
import torch

from tests import golden_cases as gc
from tests.golden.gen_golden import SMALL_SHAPES

pytestmark = pytest.mark.gpu

SMALL_SIZES = tuple(int(np.prod(s)) for s in SMALL_SHAPES)  # n = 4,186
ODD_SIZES = (3, 5, 4093, 1, 0, 995901)  # n = 1,000,003: misaligned slots, n % 4 tails, an empty and a tiny tensor


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _operands(sizes, seed, misalign=False):
    """(local, global, e) as device tensors and numpy arrays; ``misalign``: every operand a view at element 1."""
    g = np.random.default_rng(seed)
    mk = lambda m: (g.standard_normal(m) * 1e-2).astype(np.float32)  # noqa: E731
    ls, gs = [mk(m) for m in sizes], [mk(m) for m in sizes]
    e = mk(sum(sizes))

    def dev(a):
        if not misalign:
            return torch.from_numpy(a).cuda()
        buf = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        buf[1:].copy_(torch.from_numpy(a))
        return buf[1:]

    return ls, gs, e, [dev(a) for a in ls], [dev(a) for a in gs], torch.from_numpy(e).cuda()


@pytest.mark.parametrize("misalign", [False, True])
@pytest.mark.parametrize("sizes", [SMALL_SIZES, ODD_SIZES, (37,) * 100], ids=["small", "odd", "100x37"])
@pytest.mark.parametrize("subtract", [True, False])
def test_accumulate_matches_numpy(sizes, subtract, misalign):
    """e += local − global (and, global NULL, e += local): the 16-B and the scalar path, tails, an empty tensor, a
    tensor below 4 elements, and 100 tensors (more than one launch's pack of 48)."""
    from fl_sim_amd import codec

    ls, gs, e, dl, dg, de = _operands(sizes, 3, misalign)
    if misalign:
        assert all(t.data_ptr() % 16 == 4 for t in dl if t.numel())
    x = np.concatenate([a - b for a, b in zip(ls, gs)] if subtract else ls)
    want = e + x
    got = codec.ef_accumulate(dl, dg if subtract else None, de)
    assert got is de
    assert np.array_equal(_bits(de), want.view(np.uint32))
    for t, a in zip(dl + dg, ls + gs):  # (the operands are only read)
        assert np.array_equal(_bits(t), a.view(np.uint32))


def test_accumulate_through_the_extension_matches_the_ctypes_call():
    """_flcfold.ef_accumulate on Python lists: the same bits; TypeError (nothing written) for a tensor it does not
    take."""
    from fl_sim_amd import _flcfold, codec

    ls, gs, e, dl, dg, de = _operands(ODD_SIZES, 4)
    de2 = de.clone()
    codec.ef_accumulate(dl, dg, de)
    _flcfold.ef_accumulate(dl, dg, de2)
    assert torch.equal(de.view(torch.int32), de2.view(torch.int32))
    de3 = torch.from_numpy(e).cuda()
    _flcfold.ef_accumulate(dl, None, de3)
    assert np.array_equal(_bits(de3), (e + np.concatenate(ls)).view(np.uint32))
    before = de3.clone()
    with pytest.raises(TypeError):
        _flcfold.ef_accumulate([t.cpu() for t in dl], None, de3)
    with pytest.raises(TypeError):
        _flcfold.ef_accumulate([t.double() for t in dl], None, de3)
    with pytest.raises(ValueError):
        _flcfold.ef_accumulate(dl[:-1], None, de3)
    assert torch.equal(before.view(torch.int32), de3.view(torch.int32))


def test_accumulate_special_values():
    """±0, ±inf, NaN and denormals in every operand: IEEE float32 addition and subtraction, element by element."""
    from fl_sim_amd import codec

    f = np.float32
    vals = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1.1754942e-38, 1.0, -1.0, 3.4028235e38],
                    dtype=f)
    m = vals.size
    L, G, E = [a.reshape(-1).copy() for a in np.meshgrid(vals, vals, vals, indexing="ij")]  # every triple
    for sizes in ((m ** 3,), (5, m ** 3 - 5)):  # (the 16-B path, then misaligned slots: the scalar path)
        offs = np.cumsum((0,) + sizes)
        dl = [torch.from_numpy(L[a:b].copy()).cuda() for a, b in zip(offs[:-1], offs[1:])]
        dg = [torch.from_numpy(G[a:b].copy()).cuda() for a, b in zip(offs[:-1], offs[1:])]
        with np.errstate(all="ignore"):
            want_sub, want_add = E + (L - G), E + L
        de = torch.from_numpy(E.copy()).cuda()
        codec.ef_accumulate(dl, dg, de)
        assert gc.same_bits(de.cpu().numpy(), want_sub)
        de = torch.from_numpy(E.copy()).cuda()
        codec.ef_accumulate(dl, None, de)
        assert gc.same_bits(de.cpu().numpy(), want_add)


# ------------------------------------------------------------------------------------------------- residual, stacked
def _encode_round(n, k, levels, clients, seed, clustered=False):
    """``clients`` records made by the real encoder from seeded inputs (``clustered``: the large values sit in the
    first 2000 elements, so most tiles hold no entry) and their packets."""
    from fl_sim_amd import codec

    g = torch.Generator().manual_seed(seed)
    stride, _ = codec.stacked_wire_layout(n, k)
    recs = torch.zeros(clients, stride, dtype=torch.uint8, device="cuda")
    pks = []
    for c in range(clients):
        x = torch.randn(n, generator=g) * 1e-2
        if clustered:
            x[: min(n, 2000)] *= 100.0
        pks.append(codec.stacked_encode(x.cuda(), k, levels, seed=11 + c, counter=c, wire=recs[c]))
    return recs, pks


def _decode_then_subtract(pks, es):
    from fl_sim_amd import codec

    out = []
    for pk, e in zip(pks, es):
        c = codec.stacked_decode(pk, out=torch.zeros(pk.n, dtype=torch.float32, device="cuda"))
        out.append((e - c).cpu().numpy())
    return out


@pytest.mark.parametrize("n,k,clients,clustered", [(4097, 1, 10, False), (4097, 4096, 1, False),
                                                   (70001, 700, 70, False), (70001, 700, 10, True),
                                                   (1000003, 10000, 2, False)])
def test_residual_round_matches_decode_then_subtract(n, k, clients, clustered):
    """Real records (1, 10 and 70 clients in one call: 70 chains past a launch's 32; records with empty tiles);
    memories holding −0 at kept and at other positions."""
    from fl_sim_amd import codec

    levels = 10
    recs, pks = _encode_round(n, k, levels, clients, 21, clustered)
    g = torch.Generator().manual_seed(22)
    es = []
    for c in range(clients):
        e = torch.randn(n, generator=g) * 1e-2
        e[c % 3::3] = -0.0  # (−0 at a third of the positions: kept ones and others)
        es.append(e.cuda())
    idx0 = pks[0].idx.long()
    assert (es[0][idx0] == 0).any() or k < 3
    want = _decode_then_subtract(pks, es)
    before = [e.cpu().numpy() for e in es]
    codec.ef_residual_round(list(recs.unbind(0)), es, n, k, levels)
    for c in range(clients):
        got = es[c].cpu().numpy()
        assert gc.same_bits(got, want[c]), c
        untouched = np.ones(n, dtype=bool)
        untouched[pks[c].idx.cpu().numpy()] = False
        assert np.array_equal(got.view(np.uint32)[untouched], before[c].view(np.uint32)[untouched]), c
        assert n - k < 100 or (got.view(np.uint32)[untouched] == 0x80000000).any()


@pytest.mark.parametrize("norm", [0.0, float("inf"), float("nan"), -1.0])
def test_residual_round_with_an_irregular_norm(norm):
    """A record whose norm is 0, +inf, NaN (or negative): the entries of nonzero codes become NaN, the entries of
    zero codes and every other element stay as they are — as the dense decode gives them."""
    from fl_sim_amd import codec

    n, k, levels = 4186, 41, 10
    recs, pks = _encode_round(n, k, levels, 3, 23)
    pks[1].norm.fill_(norm)
    assert int((pks[1].codes[:k] != 0).sum()) > 0
    es = [torch.randn(n, generator=torch.Generator().manual_seed(24 + c)).cuda() for c in range(3)]
    want = _decode_then_subtract(pks, es)
    codec.ef_residual_round(list(recs.unbind(0)), es, n, k, levels)
    for c in range(3):
        assert gc.same_bits(es[c].cpu().numpy(), want[c]), c
    nz = (pks[1].codes[:k] != 0).cpu().numpy()
    assert np.isnan(es[1].cpu().numpy()[pks[1].idx.cpu().numpy()[nz]]).all()
    assert int(np.isnan(es[1].cpu().numpy()).sum()) == int(nz.sum())


def test_residual_round_skips_indices_out_of_range():
    """A record pre-filled with 0xFF (what a failed encode may leave: every index −1) and one whose indices lie at
    and past n: every memory unchanged, nothing written around it."""
    from fl_sim_amd import codec

    n, k, levels = 70001, 700, 10
    stride, off = codec.stacked_wire_layout(n, k)
    recs = torch.full((2, stride), 0xFF, dtype=torch.uint8, device="cuda")
    pk = codec.wire_packet(recs[1], n, k, levels)
    pk.idx.copy_(torch.arange(n, n + k, dtype=torch.int32))
    pk.norm.fill_(1.0)
    pk.codes.fill_(5)
    guard = torch.randn(2 * n + 4096, generator=torch.Generator().manual_seed(25)).cuda()
    es = [guard[1024:1024 + n], guard[2048 + n:2048 + 2 * n]]
    before = guard.clone()
    codec.ef_residual_round(list(recs.unbind(0)), es, n, k, levels)
    torch.cuda.synchronize()
    assert torch.equal(guard.view(torch.int32), before.view(torch.int32))


def test_residual_round_rejects_a_shared_memory():
    from fl_sim_amd import _lib, codec

    n, k, levels = 4186, 41, 10
    recs, _ = _encode_round(n, k, levels, 2, 26)
    e = torch.zeros(n, device="cuda")
    with pytest.raises(_lib.FlcError, match="clients 0 and 1 share a memory"):
        codec.ef_residual_round(list(recs.unbind(0)), [e, e], n, k, levels)
    assert not e.any()


# --------------------------------------------------------------------------------------------------- residual, dense
@pytest.mark.parametrize("n", [1, 3, 4186, 1000003])
@pytest.mark.parametrize("offset", [0, 1])
def test_residual_dense_matches_numpy(n, offset):
    """e −= c on the 16-B path and on views at element 1 (the scalar path), tails included."""
    from fl_sim_amd import codec

    g = np.random.default_rng(27)
    e = (g.standard_normal(n) * 1e-2).astype(np.float32)
    c = (g.standard_normal(n) * 1e-2).astype(np.float32)
    c[::5] = 0.0
    e[::7] = -0.0
    buf_e = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    buf_c = torch.zeros(n + 2, dtype=torch.float32, device="cuda")
    de, dc = buf_e[offset:offset + n], buf_c[offset:offset + n]
    de.copy_(torch.from_numpy(e))
    dc.copy_(torch.from_numpy(c))
    assert codec.ef_residual_dense(de, dc) is de
    assert np.array_equal(_bits(de), (e - c).view(np.uint32))
    assert np.array_equal(_bits(dc), c.view(np.uint32))
    assert float(buf_e[offset + n:].abs().sum()) == 0.0 and float(buf_e[:offset].abs().sum()) == 0.0


def test_residual_dense_rejects_the_memory_as_its_own_message():
    from fl_sim_amd import _lib, codec

    e = torch.ones(64, device="cuda")
    with pytest.raises(_lib.FlcError, match="same vector"):
        codec.ef_residual_dense(e, e)
    assert bool((e == 1).all())
