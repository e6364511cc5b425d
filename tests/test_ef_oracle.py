"""tests/ef_ref.py (error feedback around the oracle's compressors) reproduces tests/golden/ef_codec.npz — the same
loop around the reference's own Compressor.compressVector (tests/golden/gen_golden_ef.py) — bit for bit: every
message's decoded vector, every final memory, every send statistic and both global streams' positions."""

import random

import numpy as np
import pytest

from tests import ef_ref
from tests import golden_cases as gc
from tests.golden.gen_golden_ef import (EF_CLIENTS, EF_CODECS, EF_ROUNDS, EF_TAGS, ef_inputs, ef_key, ef_seed,
                                        flat_delta)


@pytest.fixture(scope="module")
def fixture():
    return np.load(f"{gc.GOLDEN}/ef_codec.npz", allow_pickle=False)


@pytest.fixture(scope="module")
def inputs():
    return {tag: ef_inputs(shapes) for tag, shapes in EF_TAGS.items()}


def _same(z, key, a):
    if key + "|out" in z.files and not gc.same_bits(a, z[key + "|out"]):
        return False
    return gc.sha(a) == str(z[key + "|sha"])


def test_fixture_key_set_is_complete(fixture):
    want = set()
    for tag in EF_TAGS:
        for codec in EF_CODECS:
            k = ef_key(codec, tag)
            vecs = [f"{k}|c{r}_{i}" for r in range(EF_ROUNDS) for i in range(EF_CLIENTS)]
            vecs += [f"{k}|e{i}" for i in range(EF_CLIENTS)]
            want |= {v + "|sha" for v in vecs}
            if tag == "small":
                want |= {v + "|out" for v in vecs}
            want |= {k + "|stats", k + "|next_random", k + "|next_np"}
    assert set(fixture.files) == want


@pytest.mark.parametrize("tag", list(EF_TAGS))
@pytest.mark.parametrize("codec", EF_CODECS)
def test_oracle_reproduces_the_reference_with_error_feedback(codec, tag, fixture, inputs):
    cached, locals_ = inputs[tag]
    n = sum(t.numel() for t in cached)
    key = ef_key(codec, tag)
    gc.seed_all(ef_seed(codec, tag))
    clients = [ef_ref.CompatClient(codec, n) for _ in range(EF_CLIENTS)]
    for r in range(EF_ROUNDS):
        for i, cl in enumerate(clients):
            c = cl.round(flat_delta(locals_[r][i], cached))
            assert _same(fixture, f"{key}|c{r}_{i}", c), (r, i)
    for i, cl in enumerate(clients):
        assert _same(fixture, f"{key}|e{i}", cl.e), i
    assert np.array_equal(np.array([cl.stats_row() for cl in clients], dtype=np.float64), fixture[key + "|stats"])
    assert random.random() == float(fixture[key + "|next_random"])
    assert np.random.random_sample() == float(fixture[key + "|next_np"])


def test_memory_changes_the_second_round(fixture, inputs):
    """The fixture exercises the feedback: round 2's message differs from the one the same delta gives without a
    memory (so a path that ignored the memory could not reproduce it)."""
    cached, locals_ = inputs["small"]
    n = sum(t.numel() for t in cached)
    gc.seed_all(ef_seed("topk", "small"))
    plain = ef_ref.CompatClient("topk", n).round(flat_delta(locals_[1][0], cached))
    assert not gc.same_bits(plain, fixture[ef_key("topk", "small") + "|c1_0|out"])
