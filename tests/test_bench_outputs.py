"""bench.py's plain run and --dump-outputs: the dump helper on CPU (whole arrays, the seeded
sample and block popcounts of a larger one, the 64 MB limit, the same files from the same bytes),
and one short plain run on the GPU: --steps sets the timed steps, the line carries the headline
keys and none of the --full legs, and the dumped arrays are the run's bitmap and hit mask."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY_KEYS = ("check", "host_inclusive", "cpu_baseline", "dropin_latency")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _dir_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_whole_sample_and_popcount(tmp_path, monkeypatch):
    bench = _bench_module()
    # float32 values for the budget, .npy headers and the popcounts' rounding stay under 64 MB
    assert bench.DUMP_BUDGET_BYTES + 2 ** 20 <= 64_000_000
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 2 ** 20)  # the same paths on small arrays
    rng = np.random.default_rng(7)
    small = rng.integers(0, 256, 1001, dtype=np.uint8)
    big = rng.integers(0, 256, 3 * bench.DUMP_BUDGET_BYTES // 4 + 13, dtype=np.uint8)  # 3x the whole budget
    arrays = {"big": (big.size, lambda: big), "small": (small.size, lambda: small)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    wrote = bench.dump_outputs(a, arrays, np)
    assert sorted(os.listdir(a)) == ["big_popcount.npy", "big_sample.npy", "small.npy"]
    assert _dir_bytes(a) <= bench.DUMP_BUDGET_BYTES + 3 * 128  # three .npy headers
    got = np.load(os.path.join(a, "small.npy"))
    assert got.dtype == np.float32 and np.array_equal(got, small)
    assert wrote["small"] == {"bytes": 1001, "whole": True} and wrote["big"]["whole"] is False
    # the block popcounts cover the whole array; the sample is more than half of the budget
    pc = np.load(os.path.join(a, "big_popcount.npy"))
    blk = wrote["big"]["popcount_block_bytes"]
    assert pc.dtype == np.float32 and len(pc) == -(-big.size // blk)
    assert int(pc.astype(np.int64).sum()) == int(np.unpackbits(big).sum())
    assert int(pc[-1]) == int(np.unpackbits(big[(len(pc) - 1) * blk:]).sum())
    sample = np.load(os.path.join(a, "big_sample.npy"))
    assert sample.dtype == np.float32 and sample.size == wrote["big"]["sampled"] > bench.DUMP_BUDGET_BYTES // 8
    # the same bytes give the same files; one changed byte shows in the popcounts
    bench.dump_outputs(b, arrays, np)
    for f in os.listdir(a):
        assert np.array_equal(np.load(os.path.join(a, f)), np.load(os.path.join(b, f))), f
    big[12345] ^= 0x10
    bench.dump_outputs(b, arrays, np)
    assert not np.array_equal(pc, np.load(os.path.join(b, "big_popcount.npy")))
    # a second rank's files do not collide with rank 0's
    bench.dump_outputs(a, {"small": arrays["small"]}, np, rank=1)
    assert "small_rank1.npy" in os.listdir(a)


def test_full_and_dump_options_default_off(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 3 and args.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "somewhere"


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    """`bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR`: the line has the headline keys
    and no --full leg; the hit mask (whole) says every member hits and equals the oracle's on the
    first 64k absent keys; the bitmap's block popcounts equal those of the oracle's bitmap."""
    from pebbledb_amd.keys import PackedKeys, splitmix_hex_keys
    bench = _bench_module()
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", d], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = lines[0]
    for key in HEADLINE_KEYS:
        assert key in out, key
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "Mkeys/s" and out["dtype"] == "u32"
    assert out["higher_is_better"] is True and 0 < out["ms_per_step"] < 100
    assert abs(out["value"] - 3 * 10_000_000 / out["ms_per_step"] / 1e3) <= 1e-3 * out["value"]
    for key in FULL_ONLY_KEYS:
        assert key not in out, key
    assert sorted(os.listdir(d)) == ["bitmap_popcount.npy", "bitmap_sample.npy", "hit_mask.npy"]
    assert _dir_bytes(d) <= 64_000_000
    n, nb_bytes, k, _ = bench.CONFIGS["c2"]
    hm = np.load(os.path.join(d, "hit_mask.npy"))
    assert hm.dtype == np.float32 and hm.size == 2 * n // 8
    hm = hm.astype(np.uint8)
    assert (hm[:n // 8] == 0xFF).all()  # every member hits
    # the first 64k absent keys against the oracle's filter of the same 10M members
    ns = 65_536
    want = oracle.build(nb_bytes, k, PackedKeys.fixed(splitmix_hex_keys(bench.SEED, 0, n)), omp=True)
    want_hm = oracle.probe(want, k, PackedKeys.fixed(splitmix_hex_keys(bench.SEED, n, ns)), omp=True)
    assert np.array_equal(hm[n // 8:(n + ns) // 8], want_hm)
    pc = np.load(os.path.join(d, "bitmap_popcount.npy")).astype(np.int64)
    blk = out["dumped_outputs"]["bitmap"]["popcount_block_bytes"]
    bits8 = np.unpackbits(np.arange(256, dtype=np.uint8)[:, None], axis=1).sum(axis=1).astype(np.uint8)
    want_pc = np.add.reduceat(bits8[want], np.arange(0, nb_bytes, blk), dtype=np.int64)
    assert np.array_equal(pc, want_pc)  # the whole bitmap, block by block, equals the oracle's
