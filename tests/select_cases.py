"""Inputs that steer the exact top-k selects (fl_sim_amd/csrc/topk.hip, f64.hip) down one named path each, and a
numpy model of what the select must then report.  CPU only: no torch, no device.

Every input is built from value classes a binade or more apart, some members placed at the select's sample positions
and some at positions it never samples, so that the sample's rank-``rank_lo`` key (the floor) and rank-``rank_hi`` key
(the ceiling) land in a chosen class whatever bin arithmetic the pick uses: the floor is the floor of the bin holding
the sample's ``rank_lo``-th largest key and the ceiling the end of the bin holding its ``rank_hi``-th largest, and no
pick bin is wider than ``2^(32 - hist_bits)`` keys (a quarter binade), so

    K_lo - SLACK < t_lo <= K_lo        K_hi < t_hi <= K_hi + SLACK

and every path predicate below is monotone in t_lo / t_hi: a case whose predicate holds at both ends of the two
ranges reaches its path (``precondition``).  On the device the same predicates are evaluated from the kernel's own
t_lo / t_hi (``path_facts``).  All sizes come from the plan (``codec.topk_select_plan``), none from literals."""

from collections import namedtuple

import numpy as np

KEY_NAN = 0xFFFFFFFF
KEY_INF = 0xFF800000
NO_CEILING = 1 << 32

# value classes (float32 bit patterns of the class's first member; each class stays inside one binade)
BG = 0x3B000000     # background [2^-9, 2^-8): n distinct values one ulp apart
PAD = 0x3C800000    # [2^-6, 2^-5): a few sampled members that take the floor's sample rank
TIE = 0x3E000000    # 2^-3: the tie value, alone in its binade
U = 0x3F800000      # [1, 2): the kept class
BIG = 0x40800000    # [4, 8)

Case = namedtuple("Case", "name x k expect")


# ------------------------------------------------------------------------------------------ keys and positions
def order_key(x):
    """flc_device.hpp order_key: NaN -> 0xffffffff, -0 -> +0, then the sign fold (uint32, same order as the values)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[nan] = KEY_NAN
    return k


def key_value(key):
    """The float32 whose order key is ``key`` (0xffffffff: a NaN)."""
    key = np.asarray(key, dtype=np.uint64).astype(np.uint32)
    bits = np.where(key & np.uint32(0x80000000), key & np.uint32(0x7FFFFFFF), ~key).astype(np.uint32)
    return bits.view(np.float32)


def order_key64(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).copy()
    b[b == np.uint64(1 << 63)] = 0
    nan = (b & np.uint64((1 << 63) - 1)) > np.uint64(0x7FF0000000000000)
    k = np.where(b & np.uint64(1 << 63), ~b, b | np.uint64(1 << 63)).astype(np.uint64)
    k[nan] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def sample_positions(n, S):
    """topk.hip sample_one / f64.hip sel64_prep_kernel: position of sample key j."""
    if S == n:
        return np.arange(n, dtype=np.int64)
    pos = ((np.arange(S, dtype=np.float64) + 0.5) * float(n) / float(S)).astype(np.int64)
    return np.minimum(pos, n - 1)


def filt64(n, k, sample):
    """f64.hip filt64: (S, r_lo, r_hi, on) of the float64 select's band (``sample``: its sample size cap)."""
    if n < 65536 or k <= 0 or k >= n:
        return 0, 0, 0, False
    S = min(n, sample)
    m = float(S) * float(k) / float(n)
    sd = 4.0 * np.sqrt(m) + 16.0
    r_lo = int(np.ceil(m + sd))
    if r_lo >= S:
        return S, r_lo, 0, False
    return S, r_lo, max(0, int(np.floor(m - sd))), True


def range_shift(width, bits):
    if width <= 1:
        return 0
    ln = int(width - 1).bit_length()
    return ln - bits if ln > bits else 0


def slack(plan):
    return 1 << (32 - plan["hist_bits"])


def sample_rank_keys(x, plan):
    """(K_lo, K_hi): the sample's rank_lo-th and rank_hi-th largest keys (K_hi None without a ceiling)."""
    keys = np.sort(order_key(x[sample_positions(x.size, plan["S"])]))[::-1]
    k_lo = int(keys[plan["rank_lo"] - 1])
    k_hi = int(keys[plan["rank_hi"] - 1]) if plan["rank_hi"] > 0 else None
    return k_lo, k_hi


def clamp_band(t_lo, t_hi):
    """filter_phase's clamps of the picked floor and ceiling."""
    t_lo = min(max(int(t_lo), 0), KEY_INF)
    if t_hi is None or t_hi <= t_lo or t_hi > NO_CEILING:
        t_hi = NO_CEILING
    return t_lo, int(t_hi)


def compact_wave_max(x, plan, t_lo):
    """The most keys >= t_lo that one 64-key wave of the sample holds (more than 8: the compact sample is rejected)."""
    keys = order_key(x[sample_positions(x.size, plan["S"])])
    w = (keys >= np.uint32(t_lo)).reshape(-1, 64).sum(axis=1) if keys.size % 64 == 0 else np.zeros(1, int)
    return int(w.max())


# ------------------------------------------------------------------------------------------------- the model
def predict(x, k, plan, t_lo, t_hi, T):
    """What a select with floor ``t_lo``, ceiling ``t_hi`` (exclusive) and K-th largest key ``T`` sees in ``x``."""
    n, G, M, cap, ovf = x.size, plan["G"], plan["M"], plan["cap"], plan["ovf"]
    keys = order_key(x)
    cand = keys >= np.uint32(t_lo)
    edges = np.minimum(np.arange(G + 1, dtype=np.int64) * M, n)
    csum = np.concatenate([[0], np.cumsum(cand, dtype=np.int64)])
    C_b = csum[edges[1:]] - csum[edges[:-1]]
    mode = np.where(C_b <= cap, 0, np.where(C_b <= cap + ovf, 1, 2))  # 0 LDS only, 1 g-mode, 2 x-mode
    above = int((keys.astype(np.uint64) >= np.uint64(t_hi)).sum()) if t_hi < NO_CEILING else 0
    shift = range_shift(t_hi - t_lo, plan["hist_bits"])
    out = {"C_b": C_b, "C": int(C_b.sum()), "mode": mode, "few": int(C_b.sum()) < k, "above": above, "shift": shift,
           "bin": None, "inbin_b": np.zeros(G, np.int64), "past": 0}
    if t_lo <= T < t_hi:
        b = (T - t_lo) >> shift
        lo, hi = t_lo + (b << shift), t_lo + ((b + 1) << shift)
        k64 = keys.astype(np.uint64)
        inb = cand & (k64 >= np.uint64(lo)) & (k64 < np.uint64(min(hi, t_hi)))
        isum = np.concatenate([[0], np.cumsum(inb, dtype=np.int64)])
        out["bin"] = int(b)
        out["inbin_b"] = isum[edges[1:]] - isum[edges[:-1]]
        # keys of the bin's range that lie at or above the ceiling (counted above the band, never in the bin)
        out["past"] = int(((k64 >= np.uint64(t_hi)) & (k64 < np.uint64(hi))).sum()) if hi > t_hi else 0
    return out


def kth_key(x, k):
    keys = order_key(x)
    return int(np.partition(keys, x.size - k)[x.size - k])


def path_facts(x, k, plan, t_lo, t_hi):
    """The path a select with this floor and ceiling takes, as the kernel decides it (topk_select_kernel)."""
    T = kth_key(x, k)
    p = predict(x, k, plan, t_lo, t_hi, T)
    fallback = p["few"]
    rerange = (not fallback) and p["above"] >= k
    ov_block = bool((p["inbin_b"] > plan["list_cap"]).any())
    ov_total = int(p["inbin_b"].sum()) > plan["list_all"]
    lists = (not fallback) and (not rerange) and p["shift"] > 0  # the band narrowed to a bin: the in-bin exchange runs
    one = (not fallback) and (not rerange) and not (lists and (ov_block or ov_total))
    return {"T": T, "C": p["C"], "fallback": fallback, "rerange": rerange, "list_block_overflow": lists and ov_block,
            "list_total_overflow": lists and ov_total and not ov_block, "rounds_one": one,
            "xmode": [int(b) for b in np.flatnonzero(p["mode"] == 2)],
            "gmode": [int(b) for b in np.flatnonzero(p["mode"] == 1)], "past": p["past"], "pred": p}


def check_expect(case, plan, facts, where):
    """Assert that ``facts`` (from path_facts) show the path the case was built for; the message names the plan."""
    e = case.expect
    msg = f"{case.name} ({where}): n={case.x.size} k={case.k} plan={plan} expect={e} facts=" + str(
        {f: v for f, v in facts.items() if f != "pred"})
    assert facts["fallback"] == bool(e.get("fallback", 0)), msg
    if "rerange" in e:
        assert facts["rerange"] == e["rerange"], msg
    if "rounds_one" in e:
        assert facts["rounds_one"] == e["rounds_one"], msg
    if "list" in e:
        assert facts["list_block_overflow"] == (e["list"] == "block"), msg
        assert facts["list_total_overflow"] == (e["list"] == "total"), msg
    if "xmode" in e:
        assert facts["xmode"] == sorted(e["xmode"]), msg
    if "gmode" in e:
        assert facts["gmode"] == sorted(e["gmode"]), msg
    if e.get("past"):
        assert facts["past"] > 0, msg
    if "kth_block" in e:
        T, M = facts["T"], plan["M"]
        at = np.flatnonzero(order_key(case.x) == np.uint32(T))
        assert at.size and (at // M == e["kth_block"]).all(), msg


def precondition(case, plan):
    """The case's path holds for every floor / ceiling the pick may choose (module docstring); CPU, from the plan."""
    x, k, e = case.x, case.k, case.expect
    if plan["take_all"]:
        assert e.get("sample_path") == 2, (case.name, plan)
        check_expect(case, plan, path_facts(x, k, plan, 0, NO_CEILING), "take-all")
        return
    k_lo, k_hi = sample_rank_keys(x, plan)
    s = slack(plan)
    bands = [(lo, hi) for lo in (k_lo, k_lo - s + 1) for hi in ((None,) if k_hi is None else (k_hi + 1, k_hi + s))]
    if "band" in e:  # (case j: the general pick's floor and ceiling, multiples of 1,024 keys, are part of the case)
        assert plan["rank_lo"] > plan["fast_rank"], (case.name, plan)
        bands = [e["band"]]
        assert e["band"] == ((k_lo >> 10) << 10, ((k_hi >> 10) << 10) + 1024), (case.name, hex(k_lo), hex(k_hi))
    for lo, hi in bands:
        if True:
            t_lo, t_hi = clamp_band(lo, hi)
            if "t_lo" in e:
                assert t_lo == e["t_lo"], (case.name, hex(t_lo))
            if e.get("no_ceiling"):
                assert t_hi == NO_CEILING, (case.name, t_hi)
            check_expect(case, plan, path_facts(x, k, plan, t_lo, t_hi), f"t_lo={t_lo:#x} t_hi={t_hi:#x}")
    sp = e.get("sample_path")
    if sp == 0:  # the fast pick: the rank fits, and (single-client) no sample wave rejects the compact sample
        assert plan["rank_lo"] <= plan["fast_rank"], (case.name, plan)
        if plan["compact"]:
            assert compact_wave_max(x, plan, k_lo - s + 1) <= 8, (case.name, plan)
    elif sp == 1:
        assert plan["rank_lo"] > plan["fast_rank"] or (plan["compact"] and compact_wave_max(x, plan, k_lo) > 8), (
            case.name, plan)


# ---------------------------------------------------------------------------------------------- the builders
def distinct(rng, count, base):
    """``count`` distinct float32 of the binade starting at bit pattern ``base``, evenly spread, in random order."""
    if count == 0:
        return np.zeros(0, np.float32)
    stride = (1 << 23) // count
    assert stride >= 1, count
    off = np.arange(count, dtype=np.uint32) * np.uint32(stride) + np.uint32(stride // 2)
    rng.shuffle(off)
    return (np.uint32(base) + off).view(np.float32)


class Layout:
    """An input of n distinct background values, and its positions by kind (sampled or never sampled) and block."""

    def __init__(self, n, plan, seed, negative=False):
        assert n <= 1 << 23
        self.n, self.G, self.M, self.plan = n, plan["G"], plan["M"], plan
        self.rng = np.random.default_rng(seed)
        self.x = (np.uint32(BG) + self.rng.permutation(n).astype(np.uint32)).view(np.float32).copy()
        if negative:
            self.x = -self.x
        self.steered = not plan["take_all"] and plan["S"] < n
        self.pos = sample_positions(n, plan["S"]) if self.steered else np.zeros(0, np.int64)
        self.is_sample = np.zeros(n, bool)
        self.is_sample[self.pos] = True
        self.used = np.zeros(n, bool)

    def block(self, b):
        return b * self.M, min((b + 1) * self.M, self.n)

    def take(self, count, kind, block=None, exclude=()):
        """``count`` unused positions of ``kind`` ("sample", "free", "any"), inside ``block`` or outside ``exclude``."""
        lo, hi = (0, self.n) if block is None else self.block(block)
        ok = ~self.used[lo:hi]
        if kind != "any":
            ok &= self.is_sample[lo:hi] == (kind == "sample")
        for b in exclude:
            a, z = self.block(b)
            ok[a - lo:z - lo] = False
        cand = np.flatnonzero(ok) + lo
        assert cand.size >= count, (kind, block, count, cand.size)
        pick = np.sort(self.rng.choice(cand, count, replace=False)) if count < cand.size else cand
        self.used[pick] = True
        return pick

    def mark(self, idx):
        idx = np.asarray(idx, np.int64)
        assert not self.used[idx].any()
        self.used[idx] = True
        return idx


def _steer_floor(L, plan, upper_sampled, exclude=(), pad_base=PAD, pad_sign=1.0):
    """With ``upper_sampled`` members of higher classes already at sample positions, add higher-class members up to
    rank_lo - 10 (returned: their positions, to be filled by the caller) and 50 sampled pads below them: the
    sample's rank_lo-th key is then a pad, whatever the classes' populations are."""
    if not L.steered:
        return np.zeros(0, np.int64)
    want = plan["rank_lo"] - 10 - upper_sampled
    assert want >= 0, (plan, upper_sampled)
    more = L.take(want, "sample", exclude=exclude)
    pads = L.take(50, "sample", exclude=exclude)
    L.x[pads] = pad_sign * distinct(L.rng, 50, pad_base)
    return more


def steered(name, n, k, plan, seed, forced=None, kth_block=None, run64=None, extra=50, expect=None):
    """The workhorse: a kept class U of k + ``extra`` distinct values (the K-th largest is its (extra + 1)-th
    smallest), rank_lo - 10 of them sampled, 50 sampled pads below (the floor lands on a pad and admits U and at most
    the pads), everything else background.  ``forced``: {block: members ("all": the whole block)}; the other blocks
    share the rest in proportion to their sizes.  ``run64``: a sample wave whose 64 positions all hold U.  ``kth_block``: the block that
    holds the K-th largest."""
    L = Layout(n, plan, seed)
    forced = dict(forced or {})
    tot = k + extra
    assert tot < n
    parts = []
    for b, c in forced.items():
        lo, hi = L.block(b)
        parts.append(L.take(hi - lo if c == "all" else c, "any", block=b))
    if run64 is not None and L.steered:
        parts.append(L.mark(L.pos[64 * run64:64 * run64 + 64]))
    sampled = int(sum(L.is_sample[p].sum() for p in parts))
    parts.append(_steer_floor(L, plan, sampled, exclude=tuple(forced)))
    rest = tot - sum(p.size for p in parts)
    others = [b for b in range(L.G) if b not in forced]
    assert rest >= 0 and others
    sizes = np.array([L.block(b)[1] - L.block(b)[0] for b in others], dtype=np.int64)  # (the last block is ragged)
    share = rest * sizes // sizes.sum()
    share[:rest - int(share.sum())] += 1
    for b, c in zip(others, share):
        parts.append(L.take(int(c), "free" if L.steered else "any", block=b))
    pos = np.concatenate(parts)
    assert pos.size == tot
    vals = distinct(L.rng, tot, U)
    if kth_block is not None:  # the (extra + 1)-th smallest member into kth_block
        j = int(np.argsort(vals)[extra])
        lo, hi = L.block(kth_block)
        inb = np.flatnonzero((pos >= lo) & (pos < hi))
        i = int(inb[inb.size // 2])
        vals[[i, j]] = vals[[j, i]]
    L.x[pos] = vals
    e = {"fallback": 0, "rerange": False}
    e.update(expect or {})
    return Case(name, L.x, k, e)


def ties_case(name, n, k, plan, seed, tie_blocks, need=5, expect=None):
    """The K-th largest value is TIE: k - need members of U above it (steered as in ``steered``), and
    ``tie_blocks`` = {block: count} ties at never-sampled positions.  The band bin of TIE holds nothing else."""
    L = Layout(n, plan, seed)
    nu = k - need
    parts = [_steer_floor(L, plan, 0)]
    parts.append(L.take(nu - parts[0].size, "free" if L.steered else "any"))
    pos = np.concatenate(parts)
    L.x[pos] = distinct(L.rng, nu, U)
    for b, c in tie_blocks.items():
        L.x[L.take(c, "free" if L.steered else "any", block=b)] = np.uint32(TIE).view(np.float32)
    assert sum(tie_blocks.values()) >= need
    e = {"fallback": 0, "rerange": False}
    e.update(expect or {})
    return Case(name, L.x, k, e)


def zero_ties_case(name, n, k_above, plan, seed):
    """Case n: the tie value is zero with mixed signs (-0 == +0 in the order), members in the first block, in the
    last (ragged) block and either side of a block boundary; everything below is negative.  Returns the input, the
    number of ties, and the members above them (k = k_above + need)."""
    L = Layout(n, plan, seed, negative=True)
    G, M = L.G, L.M
    bb = min(5, G - 1)
    spots = [L.mark(np.array([bb * M - 1, bb * M])), L.take(10, "free" if L.steered else "any", block=0),
             L.take(10, "free" if L.steered else "any", block=G - 1)]
    parts = [_steer_floor(L, plan, 2, pad_base=0x35800000, pad_sign=-1.0)]  # (the boundary pair may be sampled)
    parts.append(L.take(k_above - parts[0].size, "free" if L.steered else "any"))
    L.x[np.concatenate(parts)] = distinct(L.rng, k_above, U)
    at = np.sort(np.concatenate(spots))
    z = np.zeros(at.size, np.float32)
    z[::2] = -0.0
    L.x[at] = z
    return L.x, at.size


def fallback_case(name, n, k, plan, seed, tie_blocks=None):
    """Case h: rank_lo + 30 members of U, all at sample positions, nothing else above the background: the floor lands
    inside U and admits at most those, fewer than k.  ``tie_blocks``: the K-th largest value is TIE, spread so."""
    L = Layout(n, plan, seed)
    s = plan["rank_lo"] + 30
    assert s < k and L.steered
    L.x[L.take(s, "sample")] = distinct(L.rng, s, U)
    for b, c in (tie_blocks or {}).items():
        L.x[L.take(c, "free", block=b)] = np.uint32(TIE).view(np.float32)
    if tie_blocks:
        assert s < k <= s + sum(tie_blocks.values())
    return Case(name, L.x, k, {"fallback": 1})


def low_ceiling_case(name, n, k, plan, seed):
    """Case i: k + 100 members of U, none sampled: floor and ceiling lie in the background and k keys or more lie
    at or above the ceiling, so the select re-ranges above it."""
    L = Layout(n, plan, seed)
    assert L.steered and plan["rank_hi"] > 0
    L.x[L.take(k + 100, "free")] = distinct(L.rng, k + 100, U)
    return Case(name, L.x, k, {"fallback": 0, "rerange": True, "rounds_one": False})


def refine_case(name, n, k, plan, seed, copies=64):
    """Case f: the sample holds 200 members of U and, below them, a run of 2,000 values one ulp apart that straddles
    both sample ranks (at most 5 per sample wave), so the bins of both ranks hold far more than 8 sample keys and the
    pick refines them.  Every run value is repeated ``copies`` times at never-sampled positions, which puts the K-th
    largest inside the run, between the refined floor and ceiling."""
    L = Layout(n, plan, seed)
    S = plan["S"]
    assert L.steered and S % 64 == 0 and 200 < plan["rank_hi"] < plan["rank_lo"] < 2200
    waves = S // 64
    j = np.array([(i % waves) * 64 + (i // waves) * 7 for i in range(2200)])
    at = L.mark(L.pos[j])
    L.x[at[:200]] = distinct(L.rng, 200, U)
    run = (np.uint32(TIE) + np.arange(2000, dtype=np.uint32)).view(np.float32)
    L.x[at[200:]] = run[L.rng.permutation(2000)]
    L.x[L.take(2000 * copies, "free")] = np.repeat(run, copies)[L.rng.permutation(2000 * copies)]
    return Case(name, L.x, k, {"fallback": 0, "sample_path": 0, "run": (TIE | 0x80000000, (TIE | 0x80000000) + 1999)})


def nan_floor_case(name, n, k, plan, seed):
    """Case g: 500 sampled positions (more than rank_lo) hold NaN, 600 never-sampled ones +inf: the floor lands above
    key(+inf) and is clamped to it; the admitted keys are the NaNs and the +infs, ties both."""
    L = Layout(n, plan, seed)
    s = 500
    assert L.steered and s >= plan["rank_lo"] + 30 and k < s + 600
    L.x[L.take(s, "sample")] = np.float32(np.nan)
    L.x[L.take(600, "free")] = np.float32(np.inf)
    return Case(name, L.x, k, {"fallback": 0, "t_lo": KEY_INF, "nans": s})


def top_bin_case(name, n, plan, seed):
    """Case j (general pick: t_lo and t_hi are multiples of 1,024 keys): the sample's rank_hi - 1 largest keys are
    BIG, then three B = 1.5, then fillers in (C, B), and its rank_lo-th key is C = B - 4096 * 1024 keys.  The ceiling
    is then key(B) + 1024 and the floor key(C): a band 4097 * 1024 keys wide in bins of 4,096 whose top bin starts at
    key(B) and reaches 3,072 keys past the ceiling.  Ten keys A' = B + 1024 or 1124 ulps lie in that stretch.  With 100,000
    BIG and 20 B in all, k = 100,015 makes the K-th largest a B (5 of its 20 ties kept)."""
    L = Layout(n, plan, seed)
    r_lo, r_hi = plan["rank_lo"], plan["rank_hi"]
    assert L.steered and r_lo > plan["fast_rank"] and r_hi > 1
    kb = 0xBFC00000  # key(1.5)
    n_big = 100_000
    big = np.concatenate([L.take(r_hi - 1, "sample"), L.take(n_big - (r_hi - 1), "free")])
    L.x[big] = distinct(L.rng, n_big, BIG)
    G = L.G
    L.x[L.take(3, "sample")] = key_value(kb)
    for b in range(17):  # one B per block: no block's in-bin list overflows
        L.x[L.take(1, "free", block=b % G)] = key_value(kb)
    for b in range(10):  # (half of them on the ceiling itself, the first key past the clipped bin)
        L.x[L.take(1, "free", block=(b + 20) % G)] = key_value(kb + (1024 if b % 2 else 1124))
    nf = r_lo - (r_hi - 1) - 3 - 1
    L.x[L.take(nf, "sample")] = (np.uint32(0x3F900000) + np.arange(nf, dtype=np.uint32) * np.uint32(64)).view(np.float32)
    L.x[L.take(50, "sample")] = key_value(kb - 4096 * 1024)
    return Case(name, L.x, n_big + 10 + 5, {"fallback": 0, "rerange": False, "rounds_one": True, "past": True,
                                            "sample_path": 1, "band": (kb - 4096 * 1024, kb + 1024)})


def plant_near_band(x, k, plan, t_lo, t_hi, seed):
    """Case k, second step: 64 copies each of the keys one ulp and one band-bin width either side of the kernel's own
    floor and ceiling, at never-sampled positions (the sample, hence the floor and ceiling of a select of the same k,
    stay as they were).  Returns [(planted key, input)]: in each input as many never-sampled background positions
    are raised to BIG, or never-sampled members above the planted key lowered below the background, as it takes for
    exactly k - 32 keys to lie above the planted key, which is then the K-th largest."""
    n = x.size
    free = np.ones(n, bool)
    free[sample_positions(n, plan["S"])] = False
    rng = np.random.default_rng(seed)
    bw = 1 << range_shift(t_hi - t_lo, plan["hist_bits"])
    planted = sorted({t_lo - 1, t_lo, t_lo + 1, t_hi - 1, t_hi, t_hi + 1, t_lo - bw, t_lo + bw, t_hi - bw, t_hi + bw})
    low = free & (order_key(x) < np.uint32(t_lo - (1 << 22)))  # only background values are overwritten
    at = rng.choice(np.flatnonzero(low), 64 * len(planted), replace=False)
    y = x.copy()
    for i, key in enumerate(planted):
        y[at[64 * i:64 * i + 64]] = key_value(key)
    low[at] = False
    keys = order_key(y)
    out = []
    for key in planted:
        z = y.copy()
        d = (k - 32) - int((keys > np.uint32(key)).sum())
        if d > 0:
            z[rng.choice(np.flatnonzero(low), d, replace=False)] = distinct(rng, d, BIG)
        elif d < 0:
            high = free & (keys > np.uint32(planted[-1]))  # (above every planted key)
            z[rng.choice(np.flatnonzero(high), -d, replace=False)] = distinct(rng, -d, BG - 0x00800000)
        out.append((key, z))
    return out


# ------------------------------------------------------------------------------------------------ the catalogue
SINGLE_NAMES = ("a_fast_compact", "b_compact_rejected", "c_general_5", "c_general_30", "d_all_positions_sampled",
                "d_take_all_small", "d_take_all_n_minus_1", "e_no_ceiling_k1", "e_no_ceiling_k40", "f_refinement",
                "g_nan_floor_k200", "g_nan_floor_k700", "h_fallback_unique", "h_fallback_ties", "i_ceiling_too_low",
                "j_top_bin_past_ceiling", "l_list_block_overflow", "l_list_control", "m_list_total_overflow")
STORAGE_NAMES = ("o_gmode", "o_gmode_full", "p_xmode_threshold", "p_xmode_first", "p_xmode_middle", "p_xmode_last", "p_xmode_past_overflow",
                 "q_x_g_lds_mixed")


def storage_n(plan_of):
    """The smallest size class with M > cap: two block steps per block, a ragged last block."""
    p = plan_of(1 << 20, 1)
    return 2 * p["cus"] * p["cap"] - 3


def single_cases(plan_of):
    """{name: builder} of the single-client float32 cases a-q; ``plan_of(n, k)`` returns the plan.  Builders are
    lazy: an input is made when its test runs."""
    n1 = 1_048_573
    k1 = n1 // 100
    n2 = storage_n(plan_of)
    c = {}

    def add(name, fn):
        c[name] = fn

    add("a_fast_compact", lambda: steered("a_fast_compact", n1, k1, plan_of(n1, k1), 1,
                                          expect={"sample_path": 0, "rounds_one": True}))
    add("b_compact_rejected", lambda: steered("b_compact_rejected", n1, k1, plan_of(n1, k1), 2, run64=5,
                                              expect={"sample_path": 1}))
    for pct in (5, 30):
        kk = n1 * pct // 100
        add(f"c_general_{pct}", lambda kk=kk, pct=pct: steered(f"c_general_{pct}", n1, kk, plan_of(n1, kk), 3 + pct,
                                                               expect={"sample_path": 1}))
    add("d_all_positions_sampled", lambda: steered("d_all_positions_sampled", 20_000, 10_000, plan_of(20_000, 10_000),
                                                   4, expect={"sample_path": 1}))
    add("d_take_all_small", lambda: steered("d_take_all_small", 20_000, 19_600, plan_of(20_000, 19_600), 5,
                                            expect={"sample_path": 2}))
    add("d_take_all_n_minus_1", lambda: steered("d_take_all_n_minus_1", n1, n1 - 1, plan_of(n1, n1 - 1), 6, extra=0,
                                                expect={"sample_path": 2}))
    for kk in (1, 40):
        add(f"e_no_ceiling_k{kk}", lambda kk=kk: steered(f"e_no_ceiling_k{kk}", n1, kk, plan_of(n1, kk), 7 + kk,
                                                         expect={"sample_path": 0, "no_ceiling": True}))
    add("f_refinement", lambda: refine_case("f_refinement", n1, k1, plan_of(n1, k1), 9))
    for kk in (200, 700):  # through the NaNs, then through the +inf ties
        add(f"g_nan_floor_k{kk}", lambda kk=kk: nan_floor_case(f"g_nan_floor_k{kk}", n1, kk, plan_of(n1, kk), 10))
    add("h_fallback_unique", lambda: fallback_case("h_fallback_unique", n1, k1, plan_of(n1, k1), 11))
    add("h_fallback_ties", lambda: fallback_case("h_fallback_ties", n1, k1, plan_of(n1, k1), 12,
                                                 tie_blocks={0: 5000, 1: 5000, 2: 5000}))
    add("i_ceiling_too_low", lambda: low_ceiling_case("i_ceiling_too_low", n1, k1, plan_of(n1, k1), 13))
    kj = 100_015
    add("j_top_bin_past_ceiling", lambda: top_bin_case("j_top_bin_past_ceiling", n1, plan_of(n1, kj), 14))

    def lists(name, over):
        p = plan_of(n1, k1)
        cnt = p["list_cap"] + (1 if over else 0)
        return ties_case(name, n1, k1, p, 15, {3: cnt},
                         expect={"list": "block" if over else None, "rounds_one": not over})

    add("l_list_block_overflow", lambda: lists("l_list_block_overflow", True))
    add("l_list_control", lambda: lists("l_list_control", False))

    def total():
        p = plan_of(n1, k1)
        per = p["list_all"] // p["G"] + 1
        assert per <= p["list_cap"], p
        return ties_case("m_list_total_overflow", n1, k1, p, 16, {b: per for b in range(p["G"])},
                         expect={"list": "total", "rounds_one": False})

    add("m_list_total_overflow", total)
    return c, n1, k1, n2


def storage_cases(plan_of):
    """Cases o, p, q: candidates past a block's LDS.  {name: builder}."""
    n2 = storage_n(plan_of)
    c = {}

    def gk():  # the smallest k / n in steps of 1 % whose plan keeps an overflow area
        for pct in range(1, 60):
            kk = n2 * pct // 100
            p = plan_of(n2, kk)
            if p["ovf"] > 0 and not p["take_all"]:
                return kk, p
        raise AssertionError("no k with an overflow area at this size")

    def gmode():
        kk, p = gk()
        return steered("o_gmode", n2, kk, p, 20, forced={7: p["cap"] + p["ovf"] // 2},
                       expect={"gmode": [7], "xmode": []})

    c["o_gmode"] = gmode

    def edge(name, one_more):  # the last candidate count the overflow area still holds, and the first it does not
        kk, p = gk()
        cnt = p["cap"] + p["ovf"] + (1 if one_more else 0)
        assert cnt < p["M"] and p["G"] > 10, p
        return steered(name, n2, kk, p, 24, forced={9: cnt},
                       expect={"gmode": [] if one_more else [9], "xmode": [9] if one_more else []})

    c["o_gmode_full"] = lambda: edge("o_gmode_full", False)
    c["p_xmode_threshold"] = lambda: edge("p_xmode_threshold", True)
    k1 = n2 // 100
    for which in ("first", "middle", "last"):
        def xm(which=which):
            p = plan_of(n2, k1)
            b = {"first": 0, "middle": p["G"] // 2, "last": p["G"] - 1}[which]
            assert p["M"] > p["cap"] + p["ovf"], p
            return steered(f"p_xmode_{which}", n2, k1, p, 21, forced={b: "all"},
                           expect={"xmode": [b], "gmode": []})

        c[f"p_xmode_{which}"] = xm

    def xm_ovf():
        kk, p = gk()
        assert p["M"] > p["cap"] + p["ovf"], p
        b = p["G"] - 1
        return steered("p_xmode_past_overflow", n2, kk, p, 22, forced={b: "all"},
                       expect={"xmode": [b], "gmode": []})

    c["p_xmode_past_overflow"] = xm_ovf

    def mixed():
        kk, p = gk()
        xb, gb = 3, p["G"] - 2
        return steered("q_x_g_lds_mixed", n2, kk, p, 23, forced={xb: "all", gb: p["cap"] + p["ovf"] // 2},
                       kth_block=xb, expect={"xmode": [xb], "gmode": [gb], "kth_block": xb})

    c["q_x_g_lds_mixed"] = mixed
    return c


def zero_tie_cuts(plan_of, n=1_048_573):
    """Case n: (input, [(k, what)]) with k cutting the zero ties at their first, middle and last member."""
    k_above = n // 100
    x, nt = zero_ties_case("n_zero_ties", n, k_above, plan_of(n, k_above), 17)
    return x, k_above, nt, [(k_above + nt, "first"), (k_above + nt // 2, "middle"), (k_above + 1, "last")]


def batch_cases(plan_of, n, k, which, salt=0):
    """The † cases that a batched client's geometry can reach (its blocks hold M = cap elements at these sizes, so
    no candidate ever leaves LDS: o, p, q cannot occur), built from the batched plan."""
    p = plan_of(n, k)
    if which == "e":
        return steered("e_no_ceiling", n, k, p, 31 + salt, expect={"sample_path": 0, "no_ceiling": True})
    if which == "h":
        return fallback_case("h_fallback_unique", n, k, p, 32)
    blk = min(1, p["G"] - 1)
    if which == "l_over":
        return ties_case("l_list_block_overflow", n, k, p, 33, {blk: p["list_cap"] + 1},
                         expect={"list": "block", "rounds_one": False})
    return ties_case("l_list_control", n, k, p, 34, {blk: p["list_cap"]}, expect={"list": None, "rounds_one": True})


# ------------------------------------------------------------------------------------------------ float64 cases
def f64_cases(n, sample):
    """{name: (x, k, fb)} for the float64 select (f64.hip): g, i, j, n of the float32 list, built around its own
    sample positions and ranks.  ``fb`` is 1 where the band cannot hold the K-th largest (the exact passes run)."""
    S = min(n, sample)
    pos = sample_positions(n, S)
    free = np.setdiff1d(np.arange(n), pos)
    out = {}

    def base(seed):
        g = np.random.default_rng(seed)
        return g, 2.0 ** -9 * (1.0 + g.permutation(n) / float(n))  # distinct, [2^-9, 2^-8)

    # g: more than r_lo sampled NaNs; the floor lies above +inf, so only NaNs are admitted, and they are counted
    # above the ceiling: no band bin holds the K-th largest, whether it is a NaN or a +inf
    for k in (200, 700):
        _, r_lo, _, on = filt64(n, k, sample)
        assert on
        g, x = base(40)
        x[g.choice(pos, r_lo + 30, replace=False)] = np.nan
        x[g.choice(free, 600, replace=False)] = np.inf
        out[f"g_nan_floor_k{k}"] = (x, k, 1)
    # i: k + 100 large values, none sampled: more than k keys above the ceiling
    k = n // 100
    g, x = base(41)
    x[g.choice(free, k + 100, replace=False)] = 1.0 + g.permutation(k + 100) / float(4 * k)
    out["i_ceiling_too_low"] = (x, k, 1)
    # j: tests/test_gpu_f64.py::test_f64_topk_band_top_bin_past_the_ceiling's shape, from the ranks of filt64
    k = n // 10
    _, r_lo, r_hi, on = filt64(n, k, sample)
    assert on and r_hi > 1
    g, x = base(42)
    x *= 16.0  # below 0.1
    A, B, C = 1.5 + 2.0 ** -12, 1.5, 0.75
    sp = g.permutation(pos)
    nb_s = r_lo - 8 - (r_hi - 1)
    x[sp[:r_hi - 1]] = A
    x[sp[r_hi - 1:r_hi - 1 + nb_s]] = B
    x[sp[r_hi - 1 + nb_s:r_hi - 1 + nb_s + 100]] = C
    fr = g.permutation(free)
    na, nb = 100_000 - (r_hi - 1), 10_000 - nb_s
    x[fr[:na]] = A
    x[fr[na:na + nb]] = B
    out["j_top_bin_past_ceiling"] = (x, 100_000 + 4_857, 0)
    # n: +-0 ties of the K-th value at both ends and across a chunk boundary, everything below negative
    k_above = n // 100
    g, x = base(43)
    x = -x
    _, r_lo, _, _ = filt64(n, k_above, sample)
    up = np.concatenate([g.choice(pos, r_lo - 10, replace=False), g.choice(free, k_above - (r_lo - 10), replace=False)])
    x[up] = 1.0 + g.permutation(k_above) / float(4 * k_above)
    rest = np.setdiff1d(free, up)
    at = np.sort(np.concatenate([rest[:10], rest[-10:], rest[rest.size // 2:rest.size // 2 + 2]]))
    z = np.zeros(at.size)
    z[::2] = -0.0
    x[at] = z
    for what, need in (("first", at.size), ("middle", at.size // 2), ("last", 1)):
        out[f"n_zero_ties_{what}"] = (x, k_above + need, 0)
    return out
