"""Edge tests of the tiled Bloom build and probe, one per planner variant (tests/tiled_shapes.py).

Every test first asserts the variant it runs in (pbf_last_tiled_plan, which must also equal the
host-only pbf_plan_tiled field for field), then compares with the C oracle (oracle/bloom_oracle.c)
bit for bit: bitmaps with COracle.build, hit masks with COracle.probe over batches in which
members and non-members alternate.  Nothing is compared with the direct GPU path only, and there
is no tolerance.

Rows -> variants (the table's comments say why each shape enters its variant):
  tab2_*, tab1_whole_*, tab1_chunks_*, tab0_* (nf 1, 2, 8) ... k_tile_probe / k_tile_probe_set table modes
  tiny_*, short_last_tile_*, two_tiles_* ..................... load_tile, short tiles, nb_bytes % 4 != 0
  ring_build_*, ring_probe_*, ring_limit_1025_tiles .......... ring partition: POW2 / general m, exact / runtime k,
                                                                1024 / 512 / 256-key sub-chunks, k_gather_ring<8> with 2, 3, 8
  sort_build_*, sort_probe_* ................................. counting sort: layouts, exact k, buckets, PK3, two stage
                                                                windows, 4096 / 2048 / 1024-key probe sub-chunks
  geom_* ..................................................... n around kps, kpw and 4096; a last workgroup of one key;
                                                                n < 64; nq = 3
  mask_tail_* ................................................ n % 32 in {1, 31}, n % 8 != 0 (k_hw_to_hitmask)
  forced_*, split1_*, ring_falls_back_to_sort, two_pipelines,
  set_gather_1024_threads, cspace_* .......................... one child process per planner environment
and below: builds onto pristine / non-pristine bitmaps, alternating overflow counters, a hot tile
(overflow list, spill buffer, in-place spill; nf 1 and 3), boundary bits of a tile, empty regions
at TAB 1 chunk boundaries and in the TAB 0 search, stale region tails, misaligned device keys and
hit mask.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import tiled_edge_runner as run
import tiled_shapes as ts
from pebbledb_amd import BloomFilter, PackedKeys, _native, may_contain_multi
from pebbledb_amd._native import PBF_BUILD_TILED, PBF_PROBE_TILED
from pebbledb_amd.bloom_filter import plan_tiled
from pebbledb_amd.keys import splitmix_hex_keys

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = ts.TILE


@pytest.mark.parametrize("row", ts.gpu_rows(), ids=lambda r: r.name)
def test_row(row, oracle):
    run.run_row(row, oracle)


@pytest.mark.parametrize("env", ts.ENVS, ids=ts.env_id)
def test_rows_of_one_environment(env):
    """The planner reads PBF_PART, PBF_PART_G, PBF_GATHER_SPLIT and PBF_PK3 once per process: a
    fresh child per environment runs all of its rows."""
    rows = ts.gpu_rows(env)
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "tiled_edge_runner.py")],
                       env=dict(os.environ, **dict(env)), capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith("ok ")] == [x.name for x in rows]


def hex_keys(seed, n):
    return PackedKeys.fixed(splitmix_hex_keys(seed, 0, n))


def positions(nb_bytes, k, pk):
    """The k bit positions of every 16-byte key (pbf_hash_indices_fixed), int64[n, k].  Only used
    to choose adversarial key sets; what is built and probed is judged by the oracle."""
    bf = BloomFilter(nb_bytes, k)
    out = np.zeros(pk.n * k, dtype=np.uint64)
    _native.check(_native.lib().pbf_hash_indices_fixed(bf.handle, pk.data.ctypes.data, pk.key_len, pk.n,
                                                       out.ctypes.data, 0), "pbf_hash_indices_fixed")
    return out.reshape(pk.n, k).astype(np.int64)


def check_chosen(oracle, pk, k, m, pred, count):
    """The chosen set is large enough and (a sample, by the oracle's own hash) has the property."""
    assert pk.n >= count, (pk.n, count)
    for i in range(0, pk.n, max(1, pk.n // 50)):
        assert pred(oracle.indices(pk.key(i), k, m)), i


def tiled(nb, k):
    bf = BloomFilter(nb, k)
    bf.set_build_mode(PBF_BUILD_TILED)
    bf.set_probe_mode(PBF_PROBE_TILED)
    return bf


def expect(bf, probe, **fields):
    p = bf.last_tiled_plan(probe)
    for f, v in fields.items():
        assert p[f] == v, (f, p[f], v, p)
    return p


def test_builds_onto_pristine_and_non_pristine_bitmaps(oracle):
    """k_tile_build pristine (a new filter, after clear()) and non-pristine (a second batch, after
    from_bytes), in the packed counting sort and in the ring partition."""
    for nb, ring, pk3 in ((16 * TILE, 0, 1), (1024 * TILE, 32, 0)):
        a, b = hex_keys(71, 100_000), hex_keys(72, 60_000)
        bf = tiled(nb, 6)
        bf.add_many(a)
        expect(bf, False, ring=ring, pk3=pk3, n=a.n)
        want = oracle.build(nb, 6, a, omp=True)
        assert bf.bitmap() == want.tobytes()
        bf.add_many(b)  # onto a non-pristine bitmap
        expect(bf, False, ring=ring, pk3=pk3, n=b.n)
        oracle.build(nb, 6, b, bitmap=want, omp=True)
        assert bf.bitmap() == want.tobytes()
        again = BloomFilter.from_bytes(bf.to_bytes())
        again.set_build_mode(PBF_BUILD_TILED)
        again.add_many(hex_keys(73, 50_000))
        expect(again, False, ring=ring, pk3=pk3, n=50_000)
        assert again.bitmap() == oracle.build(nb, 6, hex_keys(73, 50_000), bitmap=want.copy(), omp=True).tobytes()
        bf.clear()
        bf.add_many(b)  # pristine again
        expect(bf, False, ring=ring, pk3=pk3)
        assert bf.bitmap() == oracle.build(nb, 6, b, omp=True).tobytes()


@pytest.mark.parametrize("nb,k,ring", [(16 * TILE, 2, 0), (128 * TILE, 1, 32)])
def test_hot_tile_builds_overflow_twice_in_a_row(oracle, nb, k, ring):
    """Every key of a batch lands in tile 3 (chosen at k = 1, or by all k positions): its regions
    (rings) overflow their capacity while every other region stays empty, so the build goes through
    the overflow list; two such builds in a row use the two overflow counters alternately, and a
    third returns to the first."""
    cand = hex_keys(81, 400_000)
    pos = positions(nb, k, cand)
    hot = np.flatnonzero(((pos >> 20) == 3).all(axis=1))
    base = run.take(cand, hot)
    check_chosen(oracle, base, k, nb * 8, lambda ix: all(i >> 20 == 3 for i in ix), 100)
    bf = tiled(nb, k)
    want = np.zeros(nb, dtype=np.uint8)
    for part in range(3):
        sel = np.resize(np.arange(part, base.n, 3), 40_000)  # 40K keys, all in tile 3
        batch = run.take(base, sel)
        bf.add_many(batch)
        p = expect(bf, False, ring=ring, n=40_000)
        assert p["kpw"] * k > p["cap"], p  # each workgroup's positions: more than its region of tile 3 holds
        oracle.build(nb, k, batch, bitmap=want, omp=True)
        assert bf.bitmap() == want.tobytes(), part


@pytest.mark.parametrize("nf", [1, 3])
def test_hot_tile_probe_spills(oracle, nf):
    """Ring probe in which every key's position lies in tile 5: first a batch whose overflow fits the
    LDS spill buffer, then one with more than spill_cap spilled entries per workgroup (the in-place
    test).  Members and non-members of the hot tile are mixed, so a dropped spill shows as a wrong
    bit in either direction."""
    nb, k = 128 * TILE, 1
    cand = hex_keys(91, 600_000)
    hot = run.take(cand, np.flatnonzero((positions(nb, k, cand)[:, 0] >> 20) == 5))
    check_chosen(oracle, hot, k, nb * 8, lambda ix: ix[0] >> 20 == 5, 3000)
    fs, wants = [], []
    for f in range(nf):
        members = run.take(hot, np.arange(f, hot.n, 2 + f))
        bf = tiled(nb, k)
        bf.add_many(members)
        fs.append(bf)
        wants.append(oracle.build(nb, k, members, omp=True))
    for n in (1500, 256 * 5120):
        # every workgroup's keys all fall into one region of `cap` entries
        batch = run.take(hot, np.resize(np.arange(hot.n), n))
        got = may_contain_multi(fs, batch) if nf > 1 else [fs[0].may_contain_many(batch, packed=True)]
        p = expect(fs[0], True, ring=32, nf=nf, n=n, kps=1024)
        over = min(n, p["kpw"]) - p["cap"]  # entries of one workgroup past its hot region
        assert over > 0 and (over > p["spill_cap"]) == (n > 1500), p
        for f in range(nf):
            want_hm = oracle.probe(wants[f], k, batch, omp=True)
            hits = int(np.unpackbits(want_hm).sum())
            assert 0 < hits < n
            assert np.array_equal(np.asarray(got[f]).reshape(-1), want_hm), (n, f)


@pytest.mark.parametrize("nb", [128, 129, 500])
def test_boundary_bits_of_a_tile(oracle, nb):
    """Keys whose only position (k = 1) is the first or the last bit of the filter's one tile; the
    last bit of a short tile for sizes that are no power of two."""
    m = nb * 8
    cand = hex_keys(101, 300_000)
    pos = positions(nb, 1, cand)[:, 0]
    edge = run.take(cand, np.flatnonzero((pos == 0) | (pos == m - 1)))
    check_chosen(oracle, edge, 1, m, lambda ix: ix[0] in (0, m - 1), 100)
    inner = run.take(cand, np.flatnonzero((pos == 1) | (pos == m - 2))[:200])
    bf = tiled(nb, 1)
    bf.add_many(edge)
    expect(bf, False, B=1, ring=0)
    want = oracle.build(nb, 1, edge)
    assert bf.bitmap() == want.tobytes()
    assert want[0] == 1 and want[-1] == 0x80 and not want[1:-1].any()
    q = PackedKeys.fixed(np.concatenate([edge.data.reshape(-1, 16), inner.data.reshape(-1, 16)]))
    got = bf.may_contain_many(q, packed=True)
    expect(bf, True, B=1, tab=2)
    assert np.array_equal(got, oracle.probe(want, 1, q))


def test_boundary_bits_across_a_tile_seam(oracle):
    """Two tiles, the second a short one of 8 bits (m = 2^20 + 8): keys whose only position (k = 1)
    is bit 0, bit 2^20 - 1 (the last of the full first tile), bit 2^20 (the first of the short last
    tile, at a non-zero tile base) or bit m - 1.  A bit takes about 2^20 candidates per hit: 16M
    keys are generated and hashed on the device and only the chosen ones come back."""
    torch = pytest.importorskip("torch")
    nb, ncand = TILE + 1, 1 << 24
    m = nb * 8
    targets = (0, (1 << 20) - 1, 1 << 20, m - 1)
    near = (1, (1 << 20) - 2, (1 << 20) + 1, m - 2)
    keys = torch.empty(ncand * 16, dtype=torch.uint8, device="cuda")
    pos = torch.empty(ncand, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    _native.check(_native.lib().pbf_gen_splitmix_hex(0, None, keys.data_ptr(), 141, 0, ncand), "gen")
    torch.cuda.synchronize()
    hasher = BloomFilter(nb, 1)
    _native.check(_native.lib().pbf_hash_indices_fixed(hasher.handle, keys.data_ptr(), 16, ncand, pos.data_ptr(), 1),
                  "pbf_hash_indices_fixed")
    hasher.sync()
    rows = keys.view(ncand, 16)

    def chosen(bits):
        sel = torch.zeros(ncand, dtype=torch.bool, device="cuda")
        for b in bits:
            hit = pos == b
            assert int(hit.sum()) >= 3, (b, int(hit.sum()))  # every target bit has its keys
            sel |= hit
        return PackedKeys.fixed(rows[sel].cpu().numpy())

    edge, inner = chosen(targets), chosen(near)
    del keys, pos, rows
    for pk, bits in ((edge, targets), (inner, near)):  # by the oracle's own hash, every chosen key
        assert {oracle.indices(pk.key(i), 1, m)[0] for i in range(pk.n)} == set(bits)
    bf = tiled(nb, 1)
    bf.add_many(edge)
    expect(bf, False, B=2, tb=20, ring=0)
    want = oracle.build(nb, 1, edge)
    assert bf.bitmap() == want.tobytes()
    assert sorted(np.flatnonzero(np.unpackbits(want, bitorder="little")).tolist()) == sorted(targets)
    q = PackedKeys.fixed(np.concatenate([edge.data.reshape(-1, 16), inner.data.reshape(-1, 16)]))
    got = bf.may_contain_many(q, packed=True)
    expect(bf, True, B=2, n=q.n)
    want_hm = oracle.probe(want, 1, q)
    assert int(np.unpackbits(want_hm).sum()) == edge.n  # the neighbours of every target bit miss
    assert np.array_equal(got, want_hm)
    # and the neighbours built on top: the words on both sides of the seam, against the oracle
    bf.add_many(inner)
    oracle.build(nb, 1, inner, bitmap=want)
    assert bf.bitmap() == want.tobytes()


@pytest.mark.parametrize("n,tab,chunked", [(140_000, 1, True), (270_000, 0, False)])
def test_empty_regions(oracle, n, tab, chunked):
    """Slices of kpw keys with disjoint tile sets: even workgroups touch tile 0 only and odd ones
    tile 1 only, so every other region of a tile is empty: empty regions inside and at the
    boundaries of the TAB 1 chunks, runs of equal prefix counts in the TAB 0 search."""
    nb, k = 2 * TILE, 8
    cand = hex_keys(111, 1_500_000)
    tile = positions(nb, k, cand) >> 20
    sets = [run.take(cand, np.flatnonzero((tile == t).all(axis=1))) for t in (0, 1)]
    for t in (0, 1):
        check_chosen(oracle, sets[t], k, nb * 8, lambda ix: all(i >> 20 == t for i in ix), 2000)
    plan = plan_tiled(nb, k, n, True)
    kpw = plan["kpw"]
    rows = []
    for g in range(-(-n // kpw)):
        s = sets[g % 2]
        rows.append(s.data.reshape(-1, 16)[np.resize(np.arange(g, s.n), kpw)])
    batch = PackedKeys.fixed(np.concatenate(rows)[:n])
    members = PackedKeys.fixed(np.concatenate([s.data.reshape(-1, 16)[::2] for s in sets]))
    bf = tiled(nb, k)
    bf.add_many(members)
    want = oracle.build(nb, k, members, omp=True)
    got = bf.may_contain_many(batch, packed=True)
    p = expect(bf, True, tab=tab, B=2, kpw=kpw)
    assert (p["tabw"] > 0) == chunked and p == plan
    want_hm = oracle.probe(want, k, batch, omp=True)
    assert 0 < int(np.unpackbits(want_hm).sum()) < n
    assert np.array_equal(got, want_hm)


def test_stale_region_tails(oracle):
    """A small probe after a larger one on the same scratch: the regions' tails still hold the
    larger batch's entries and result bits."""
    nb, k = 16 * TILE, 6
    big, small = hex_keys(121, 500_000), hex_keys(122, 3000)
    members = run.take(big, run.member_index(big.n, 0))
    bf = tiled(nb, k)
    bf.add_many(members)
    bf.add_many(run.take(small, np.arange(0, 3000, 3)))
    want = oracle.build(nb, k, members, omp=True)
    oracle.build(nb, k, run.take(small, np.arange(0, 3000, 3)), bitmap=want, omp=True)
    for pk, G in ((big, 245), (small, 2), (big, 245), (small, 2)):
        got = bf.may_contain_many(pk, packed=True)
        expect(bf, True, G=G, n=pk.n, ring=0)
        assert np.array_equal(got, oracle.probe(want, k, pk, omp=True)), pk.n


def test_misaligned_device_keys_and_hit_mask(oracle):
    """16-byte keys at a device address that is 1 mod 16 take the any-alignment key loads
    (key_mode 1), and a hit mask at an address that is 1 mod 4 cannot be the gather's word
    buffer: k_hw_to_hitmask writes it byte by byte."""
    torch = pytest.importorskip("torch")
    nb, k, n = 16 * TILE, 6, 100_000
    host = hex_keys(131, n)
    members = run.take(host, run.member_index(n, 0))
    buf = torch.zeros(n * 16 + 16, dtype=torch.uint8, device="cuda")
    buf[1:1 + n * 16] = torch.from_numpy(host.data).cuda()
    mbuf = torch.zeros(members.n * 16 + 16, dtype=torch.uint8, device="cuda")
    mbuf[1:1 + members.n * 16] = torch.from_numpy(members.data).cuda()
    hm = torch.zeros(n // 8 + 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert (buf.data_ptr() + 1) % 16 == 1 and (hm.data_ptr() + 1) % 4 == 1
    bf = tiled(nb, k)
    bf.add_device_fixed(mbuf.data_ptr() + 1, 16, members.n)
    bf.sync()
    expect(bf, False, key_mode=1, exact_k=0, pk3=0, ring=0)
    want = oracle.build(nb, k, members, omp=True)
    assert bf.bitmap() == want.tobytes()
    want_hm = oracle.probe(want, k, host, omp=True)
    for off, is_mask in ((1, 0), (0, 1)):
        hm.zero_()
        torch.cuda.synchronize()
        bf.probe_device_fixed(buf.data_ptr() + 1, 16, n, hm.data_ptr() + off)
        bf.sync()
        expect(bf, True, key_mode=1, use_hw=1, hw_is_mask=is_mask, n=n)
        got = hm.cpu().numpy()
        assert np.array_equal(got[off:off + n // 8], want_hm), off
        assert not got[:off].any() and not got[off + n // 8:].any()  # nothing written around the mask
