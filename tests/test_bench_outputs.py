"""bench.py's options around the headline: `--steps` is checked before any GPU work, and `--dump-outputs` writes
what one step of the timed path returned (bench.dump_outputs), the same arrays for the same step."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_zero_steps_are_refused():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "0", "--warmup", "0", "--full",
                        "--dump-outputs", "unused"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2
    assert "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("sample", [1000, 1 << 20])  # a sample of the dense output; the whole output
def test_dump_outputs_writes_the_step(tmp_path, monkeypatch, sample):
    import torch

    import bench
    from fl_sim_amd import codec

    monkeypatch.setattr(bench, "DUMP_SAMPLE", sample)
    dev = torch.device("cuda", 0)
    n, k = (1 << 16) + 3, 655
    x = torch.randn(n, generator=torch.Generator(device=dev).manual_seed(5), device=dev) * 1e-3
    out = torch.empty(n, dtype=torch.float32, device=dev)
    pkt = codec.stacked_encode(x, k, bench.LEVELS, seed=0, counter=3)
    codec.stacked_decode(pkt, out=out)
    got = bench.dump_outputs(str(tmp_path / "a"), pkt, out)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(f"{name}.npy" for name in got)
    total = 0
    for name, arr in got.items():
        on_disk = np.load(tmp_path / "a" / f"{name}.npy")
        assert on_disk.dtype in (np.float32, np.float64) and on_disk.dtype == arr.dtype
        assert np.array_equal(on_disk, arr)
        total += on_disk.nbytes
    assert total <= 64_000_000
    idx = pkt.idx.cpu().numpy()
    dense = out.cpu().numpy()
    assert np.array_equal(got["wire_idx"], idx.astype(np.float64))
    assert np.array_equal(got["wire_codes"], pkt.codes[:k].cpu().numpy().astype(np.float32))
    assert np.array_equal(got["wire_norm"], pkt.norm.cpu().numpy())
    assert np.array_equal(got["wire_tiles"], pkt.tiles.cpu().numpy().astype(np.float64))
    assert np.array_equal(got["decoded_at_kept"].view(np.uint32), dense[idx].view(np.uint32))
    pos = got["decoded_sample_pos"].astype(np.int64)
    assert len(pos) == min(sample, n) and np.all(np.diff(pos) >= 0) and pos[0] >= 0 and pos[-1] < n
    assert np.array_equal(got["decoded_sample"].view(np.uint32), dense[pos].view(np.uint32))
    assert got["decoded_nnz"][0] == np.count_nonzero(dense)
    # the same step again: the same arrays, the same sample positions
    pkt2 = codec.stacked_encode(x, k, bench.LEVELS, seed=0, counter=3)
    out2 = codec.stacked_decode(pkt2)
    again = bench.dump_outputs(str(tmp_path / "b"), pkt2, out2)
    for name in got:
        assert np.array_equal(got[name], again[name]), name
    # at N > 1 every rank writes its own files
    bench.dump_outputs(str(tmp_path / "c"), pkt, out, world=2, rank=1)
    assert sorted(os.listdir(tmp_path / "c")) == sorted(f"{name}_rank1.npy" for name in got)
