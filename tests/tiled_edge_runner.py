"""Runs rows of tests/tiled_shapes.py on the GPU (test_gpu_tiled_edges.py, in-process or as the
child of one planner environment): build or probe, assert the plan that was launched, then
compare with the C oracle bit for bit."""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tiled_shapes as ts  # noqa: E402
from pebbledb_amd import BloomFilter, PackedKeys, may_contain_multi  # noqa: E402
from pebbledb_amd._native import PBF_BUILD_ATOMIC, PBF_BUILD_TILED, PBF_PROBE_TILED  # noqa: E402
from pebbledb_amd.bloom_filter import plan_tiled  # noqa: E402
from pebbledb_amd.keys import splitmix_hex_keys, varlen_keys  # noqa: E402

BLOCK = 500  # members and non-members alternate in runs of this many keys


def make_keys(layout: str, seed: int, n: int) -> PackedKeys:
    """n keys of a layout: hex16 (16 hex chars), fixN (N bytes of hex chars), var (8..64 bytes)."""
    if layout == "var":
        d, off = varlen_keys(seed, 0, n)
        return PackedKeys(d, n, offsets=off)
    kl, _ = ts.layout_args(layout)
    wide = np.concatenate([splitmix_hex_keys(seed + 7919 * j, 0, n) for j in range(-(-kl // 16))], axis=1)
    return PackedKeys.fixed(wide[:, :kl])


def take(pk: PackedKeys, idx: np.ndarray) -> PackedKeys:
    """The keys pk[idx], in that order."""
    idx = np.asarray(idx, dtype=np.int64)
    if pk.key_len > 0:
        return PackedKeys.fixed(pk.data.reshape(pk.n, pk.key_len)[idx])
    off = pk.offsets.astype(np.int64)
    lens = (off[1:] - off[:-1])[idx]
    new_off = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=new_off[1:])
    src = np.arange(new_off[-1], dtype=np.int64) - np.repeat(new_off[:-1], lens) + np.repeat(off[idx], lens)
    return PackedKeys(pk.data[src], len(idx), offsets=new_off.astype(np.uint64))


def member_index(n: int, f: int) -> np.ndarray:
    """Filter f's members among a probe stream of n keys: every (f+2)-th run of BLOCK keys (and
    key 0), so each filter of a set answers differently and hits and misses alternate all along
    the batch, on both sides of any pipeline seam."""
    i = np.arange(n)
    block = BLOCK if n >= 8 * BLOCK else max(1, n // 8)  # (small batches: shorter runs, still both kinds)
    return i[((i // block) % (f + 2) == 0) | (i == 0)]


def assert_plan(bf: BloomFilter, probe: bool, expect: dict, predicted: dict, name: str) -> dict:
    got = bf.last_tiled_plan(probe)
    for field, want in expect.items():
        assert got[field] == want, (name, field, got[field], want, got)
    # the report is the launch's own arithmetic: the host-only call says the same, field for field
    assert got == predicted, (name, {f: (got[f], predicted[f]) for f in got if got[f] != predicted[f]})
    return got


def run_row(r: ts.Row, oracle) -> None:
    pk = make_keys(r.layout, 1000 + len(r.name), r.n)
    predicted = ts.plan_of(r)
    if not r.probe:
        bf = BloomFilter(r.nb_bytes, r.k)
        want = oracle.build(r.nb_bytes, r.k, pk, omp=True)
        if r.expect.get("tiled", 1) == 0:  # the tiled build refuses this geometry: the atomic path runs
            try:
                bf.set_build_mode(PBF_BUILD_TILED)
                raise AssertionError(f"{r.name}: the tiled build was accepted")
            except ValueError:
                pass
            bf.add_many(pk)
            assert bf.last_build_mode == PBF_BUILD_ATOMIC and predicted["tiled"] == 0, r.name
            try:
                bf.last_tiled_plan(False)
                raise AssertionError(f"{r.name}: a tiled plan was reported")
            except ValueError:
                pass
        else:
            bf.set_build_mode(PBF_BUILD_TILED)
            bf.add_many(pk)
            assert bf.last_build_mode == PBF_BUILD_TILED, r.name
            assert_plan(bf, False, r.expect, predicted, r.name)
        assert bf.bitmap() == want.tobytes(), f"{r.name}: bitmap differs from the oracle"
        return
    fs, wants = [], []
    for f in range(r.nf):
        members = take(pk, member_index(r.n, f))
        bf = BloomFilter(r.nb_bytes, r.k)
        bf.add_many(members)
        bf.set_probe_mode(PBF_PROBE_TILED)
        fs.append(bf)
        wants.append(oracle.build(r.nb_bytes, r.k, members, omp=True))
    if r.nf == 1:
        got = [fs[0].may_contain_many(pk, packed=True)]
    else:
        got = may_contain_multi(fs, pk)
    for bf in fs:
        assert bf.last_probe_mode == PBF_PROBE_TILED, r.name
        assert_plan(bf, True, r.expect, predicted, r.name)
    for f in range(r.nf):
        want_hm = oracle.probe(wants[f], r.k, pk, omp=True)
        hits = int(np.unpackbits(want_hm).sum())  # hits and (one key, or 16 one-byte keys, aside) misses
        assert 0 < hits and (hits < r.n or r.n == 1 or r.layout == "fix1"), (r.name, hits)
        assert np.array_equal(np.asarray(got[f]).reshape(-1), want_hm), f"{r.name}: hit mask of filter {f} differs"


def main() -> None:
    """Child of one planner environment: every GPU row of that environment, `ok <name>` each."""
    from oracle.oracle import COracle
    env = tuple(sorted((k, v) for k, v in os.environ.items()
                       if k in ("PBF_PART", "PBF_PART_G", "PBF_GATHER_SPLIT", "PBF_PK3")))
    rows = [r for r in ts.ROWS if tuple(sorted(r.env)) == env and r.keys != "cpu_only"]
    assert rows, env
    o = COracle()
    for r in rows:
        run_row(r, o)
        print("ok", r.name, flush=True)
    print("done", len(rows), flush=True)


if __name__ == "__main__":
    main()
