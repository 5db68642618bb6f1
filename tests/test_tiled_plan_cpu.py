"""The host planner of the tiled Bloom build / probe, checked without a GPU through
pbf_plan_tiled (the arithmetic the launches themselves use).

1. Invariants over a sweep of (nb_bytes, k, key layout, n, probe, nf).  Each is a limit a kernel
   relies on, taken from a comment or a check in csrc/pebblebloom.hip, tiled_kernels.hpp or
   ring_kernels.hpp; a violation is a planner bug.
2. The shape table (tests/tiled_shapes.py): every row lands in the variant it is named for, so a
   retune of the planner that moves a GPU edge test to another branch fails here, loudly.

Rows and the variants they pin (tests/test_gpu_tiled_edges.py runs the same rows on the device):
see the ROWS comments in tiled_shapes.py; `test_table_reaches_every_variant` lists the variants
and asserts that at least one row reaches each.
"""
import json
import os
import subprocess
import sys

import pytest

from pebbledb_amd.bloom_filter import plan_tiled

import tiled_shapes as ts

KIB = 1024
TILE = 2 ** 17  # bytes of one 2^20-position tile
K_RING_MAX_CAP = 8160  # ring_kernels.hpp kRingMaxCap

# the four bench configurations: (nb_bytes, k, key_len, n build, n probe, nf of the probe)
BENCH = [(2 ** 27, 6, 16, 10_000_000, 20_000_000, 1),          # c2
         (2 ** 30, 8, 0, 100_000_000, 200_000_000, 1),         # c3
         (224_649_806, 10, 16, 125_000_000, 1_000_000, 1),     # c4
         (2 ** 27, 6, 16, 10_000_000, 100_000_000, 8)]         # c5

# sizes around every tile-count threshold (1, 2, 127/128, 767/768, 1024/1025, 4096 tiles; sizes past
# 2^29 B have m > 2^32 and keep 4096), tiles below 2^20 positions, the non-power-of-two m of the
# partition tests, and the smallest m > 2^32
SIZES = [1, 3, 128, 129, 500, 4096, TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE + 5, 16 * TILE, 127 * TILE,
         128 * TILE, 767 * TILE, 768 * TILE, 768 * TILE + 4, 1024 * TILE, 1024 * TILE + 12, 1025 * TILE, 1714 * TILE,
         4096 * TILE, 8191 * TILE + 1, 8192 * TILE, 8192 * TILE + 1, 2 ** 29 + 1, 2 ** 29 + 4, 2 ** 29 + 2 ** 20]
NS = [1, 63, 64, 1023, 1024, 1025, 4095, 4096, 4097, 100_007, 135_000, 1 << 20, 3_000_000, 20_000_000, 1 << 26, 1 << 28]
LAYOUTS = [(16, True), (16, False), (7, True), (0, True)]  # (key_len, aligned): kFixed16, kFixedN, kFixedN, kVar


def check_invariants(p, k, n):
    ctx = json.dumps(p)
    assert p["pipelines"] >= 1 and p["n"] >= 1, ctx
    per, np_ = p["keys_per_pipeline"], p["pipelines"]
    # the call's keys split into `pipelines` of keys_per_pipeline, the last one described
    assert (np_ - 1) * per < n <= np_ * per and p["n"] == n - (np_ - 1) * per, ctx
    G, kpw, cap, B = p["G"], p["kpw"], p["cap"], p["B"]
    # every key belongs to exactly one partition workgroup, none is empty (PartGeom, k_part's `g * kpw`)
    assert G * kpw >= p["n"] > (G - 1) * kpw, ctx
    assert kpw == p["nsub"] * p["kps"], ctx
    assert p["nq"] == -(-kpw // 4096), ctx  # pref groups of 4096 keys
    # region capacity in whole 32-entry words; packed entries in whole 32-word units of 3 entries
    assert cap % (96 if p["pk3"] else 32) == 0 and cap > 0, ctx
    # entry offsets within a workgroup's regions are 32-bit
    assert B * cap < 2 ** 32, ctx
    assert cap < 2 ** 24, ctx  # 24-bit region addressing of the partitions
    if p["ring"]:
        # ring lim / tail are 16-bit byte counts; 32-entry rings of B tiles in LDS; KX <= 16
        assert cap <= K_RING_MAX_CAP and B <= 1024 and k <= 16, ctx
        assert p["kps"] in ((1024,) if p["probe"] else (1024, 512, 256)), ctx
        assert p["spill_cap"] >= 1, ctx
    else:
        # k_part keeps ranks and slots as 16-bit halves: kps * k + pads < 2^16
        pads = 2 * min(B, p["kps"] * k) if p["pk3"] else 0
        assert p["kps"] * k + pads < 65536, ctx
        assert p["kps"] % 1024 == 0 and p["scap"] >= 1, ctx
        if p["probe"]:
            assert p["kps"] in (1024, 2048, 4096), ctx  # sub-chunks tile the 4096-key groups
        assert p["lds_part"] <= 156 * KIB, ctx
    assert p["lds_part"] <= 160 * KIB and p["lds_tile"] <= 160 * KIB, ctx
    if not p["probe"]:
        return
    # the gather's u16 run boundaries (pref) and the u32 global region-word index
    assert cap <= 65535, ctx
    assert G * B * (cap // 32) < 2 ** 32, ctx
    # pipelines were computed from the gather's LDS (tiled_probe_batch): it fits
    assert p["lds_gather"] <= 156 * KIB, ctx
    wpr = cap // 32
    assert p["wsh"] == max(wpr - 1, 1).bit_length(), ctx
    assert p["tab"] in (0, 1, 2), ctx
    if p["tab"] == 1:  # u16 table entry = region << wsh | word, region * B + tile in 24 bits
        assert ((G - 1) << p["wsh"]) < 65536 and G * B < 2 ** 24, ctx
        assert p["tabw"] == 0 or p["tabw"] >= wpr, ctx  # a chunk holds at least one whole region
    else:
        assert p["tabw"] == 0, ctx
    if np_ > 1:  # hit masks of later pipelines start at hitmask + i0 / 8 on whole words
        assert per % 64 == 0, ctx
    assert p["gather_threads"] in (512, 1024) and 1 <= p["gsplit"] <= 64, ctx
    assert p["use_hw"] == int(p["gsplit"] > 1 or p["nf"] > 1), ctx
    assert p["hw_is_mask"] == int(p["use_hw"] and p["nf"] == 1 and p["n"] % 32 == 0), ctx
    assert 1 <= p["rounds"] <= 4 and (p["rounds"] == 1 or (p["ring"] and p["nf"] > 1)), ctx


def test_bench_configurations_keep_their_variants():
    """The variants the four bench configurations run (bench.py's numbers are measured on them)."""
    for nb, k, kl, nbuild, nprobe, nf in BENCH:
        b = plan_tiled(nb, k, nbuild, False, kl)
        q = plan_tiled(nb, k, nprobe, True, kl, nf=nf)
        check_invariants(b, k, nbuild)
        check_invariants(q, k, nprobe)
    c2b, c2p = plan_tiled(2 ** 27, 6, 10_000_000, False), plan_tiled(2 ** 27, 6, 20_000_000, True)
    assert (c2b["ring"], c2b["kps"], c2b["exact_k"], c2b["pow2"]) == (32, 1024, 1, 1)
    assert (c2p["ring"], c2p["tab"], c2p["gsplit"], c2p["hw_is_mask"], c2p["pipelines"]) == (32, 2, 8, 1, 1)
    c3b, c3p = plan_tiled(2 ** 30, 8, 100_000_000, False, 0), plan_tiled(2 ** 30, 8, 200_000_000, True, 0)
    assert (c3b["ring"], c3b["pk3"], c3b["kps"]) == (0, 1, 4096)
    assert (c3p["ring"], c3p["tab"], c3p["gsplit"], c3p["pipelines"], c3p["kps"]) == (0, 1, 32, 2, 4096)
    c4b = plan_tiled(224_649_806, 10, 125_000_000, False)
    assert (c4b["ring"], c4b["pk3"], c4b["part_kmax"], c4b["kps"]) == (0, 1, 10, 3072)
    c5p = plan_tiled(2 ** 27, 6, 100_000_000, True, nf=8)
    assert (c5p["ring"], c5p["rounds"], c5p["tab"], c5p["gather_threads"], c5p["pipelines"]) == (32, 3, 1, 1024, 1)
    assert c5p["tabw"] > 0


@pytest.mark.parametrize("probe", [False, True])
def test_planner_invariants_over_the_sweep(probe):
    """k in 1..32, n from 1 to 2^28, every size around a tile-count threshold, every key layout,
    1 / 2 / 8 filters per probe, with and without a CU spared for the resident reader."""
    seen = 0
    for nb in SIZES:
        for k in range(1, 33):
            for kl, al in LAYOUTS:
                for n in NS:
                    for nf in ((1, 2, 8) if probe and kl == 16 and al else (1,)):
                        spare = (n + k + nf) % 2 == 1
                        p = plan_tiled(nb, k, n, probe, kl, al, nf, spare)
                        if not p["tiled"]:
                            continue
                        seen += 1
                        check_invariants(p, k, n)
    assert seen > 20_000


def test_geometry_thresholds():
    """tiled_ok at 1, 2 and 4096 tiles.  Tiles hold 2^20 positions and the tile space ends at 2^32
    positions, so 4096 is the most a filter has: the planner's `more than 8192 tiles` refusal cannot
    be reached, and m > 2^32 is refused only when m % 32 != 0."""
    for nb, ok, B in ((TILE, 1, 1), (TILE + 1, 1, 2), (4096 * TILE, 1, 4096), (4096 * TILE + 1, 0, 4096),
                      (2 ** 29 + 4, 1, 4096), (2 ** 30, 1, 4096), (2 ** 34, 1, 4096)):
        p = plan_tiled(nb, 6, 100_000, False)
        assert (p["tiled_ok"], p["B"]) == (ok, B), nb
        assert p["tiled"] == ok
    assert plan_tiled(2 ** 29 + 4, 6, 1000, True)["cspace"] == 1
    assert plan_tiled(2 ** 20, 33, 1000, False)["tiled"] == 0  # k <= 32
    # tiles of 2^10 .. 2^12 positions
    assert [plan_tiled(nb, 3, 100, True)["tb"] for nb in (1, 128, 129, 256, 512, 513)] == [10, 10, 11, 11, 12, 13]


def _eval_rows(rows):
    return [ts.plan_of(r) for r in rows]


def _check_rows(rows, plans):
    for r, p in zip(rows, plans):
        for field, want in r.expect.items():
            assert p[field] == want, (r.name, field, p[field], want, p)
        if p["tiled"] and not r.env:  # (a forced workgroup count may break limits the planner keeps on its own)
            check_invariants(p, r.k, r.n)


def test_shape_table_rows_without_environment():
    rows = [r for r in ts.ROWS if not r.env]
    _check_rows(rows, _eval_rows(rows))


@pytest.mark.parametrize("env", ts.ENVS, ids=ts.env_id)
def test_shape_table_rows_with_environment(env):
    """The planner reads its environment once per process: one child per environment."""
    rows = [r for r in ts.ROWS if r.env == env]
    code = ("import json, sys; sys.path.insert(0, 'tests'); import tiled_shapes as ts; "
            "print(json.dumps([ts.plan_of(r) for r in ts.ROWS if r.env == %r]))" % (env,))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **dict(env)), capture_output=True,
                         text=True, timeout=120, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    _check_rows(rows, json.loads(out.stdout.strip().splitlines()[-1]))


def test_table_reaches_every_variant():
    """At least one row per variant of the issue's list (the `expect` of a row is asserted by the
    two tests above, so a variant counted here is a variant reached)."""
    rows = ts.ROWS

    def any_row(**want):
        return any(all(r.expect.get(f) == v for f, v in want.items()) for r in rows)

    for nf in (1, 2, 8):  # k_tile_probe / k_tile_probe_set: TAB 2, TAB 1 whole, TAB 1 chunked, TAB 0
        for tab in (2, 1, 0):
            assert any(r.expect.get("tab") == tab and r.nf == nf and r.probe for r in rows), (nf, tab)
        assert any(r.expect.get("tab") == 1 and r.expect.get("tabw", 0) > 0 and r.nf == nf for r in rows), nf
        assert any(r.expect.get("tab") == 1 and r.expect.get("tabw") == 0 and r.nf == nf for r in rows), nf
    for kps in (1024, 512, 256):  # ring build sub-chunks
        assert any(r.expect.get("ring") == 32 and r.expect.get("kps") == kps and not r.probe for r in rows), kps
    for pow2 in (0, 1):
        for exact in (0, 1):
            assert any_row(ring=32, pow2=pow2, exact_k=exact), (pow2, exact)
    for kmax in (4, 6, 8, 10, 16, 32):  # counting sort: exact k and every register bucket
        assert any_row(ring=0, part_kmax=kmax), kmax
    assert any_row(ring=0, pk3=1) and any(r.expect.get("pk3") == 0 and r.expect.get("exact_k") == 1 and not r.probe
                                          for r in rows)
    for kps in (1024, 2048, 4096):  # probe sub-chunks of the counting sort
        assert any(r.expect.get("ring") == 0 and r.expect.get("kps") == kps and r.probe for r in rows), kps
    for km in (0, 1, 2):
        assert any_row(ring=0, key_mode=km) and any_row(ring=32, key_mode=km), km
    for gs in (1, 8, 32):
        assert any_row(gsplit=gs), gs
    assert any(r.expect.get("gtq", 0) > 0 for r in rows) and any_row(gtq=0)
    assert any_row(gather_threads=512) and any_row(gather_threads=1024)
    assert {r.nf for r in rows if r.probe and r.expect.get("ring") == 32} >= {1, 2, 3, 8}
    for rounds in (2, 3, 4):
        assert any_row(rounds=rounds), rounds
    assert any_row(hw_is_mask=1) and any_row(use_hw=1, hw_is_mask=0) and any_row(use_hw=0)
    assert any(r.expect.get("pipelines", 1) > 1 and r.probe for r in rows)
    assert any(r.expect.get("nq", 0) >= 3 for r in rows)
    assert any_row(cspace=1) and any_row(tiled=0)
    for B in (1, 2, 4096):
        assert any(r.expect.get("B") == B and r.expect.get("tiled", 1) == 1 for r in rows), B
    assert any_row(ring=0, B=1024)  # the fallback from ring to sort when cap > kRingMaxCap
