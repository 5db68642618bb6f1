"""The shape table of the tiled Bloom build / probe edge tests.

Each row names one planner variant and the smallest shape found to enter it.  The CPU test
(test_tiled_plan_cpu.py) asserts with pbf_plan_tiled that the row lands in the variant; the GPU
test (test_gpu_tiled_edges.py) runs it, asserts pbf_last_tiled_plan says the same, and compares
with the C oracle bit for bit.
"""
from __future__ import annotations

from typing import NamedTuple

TILE = 2 ** 17  # bytes of one 2^20-position tile


class Row(NamedTuple):
    name: str
    nb_bytes: int
    k: int
    layout: str        # hex16 | fixN (N-byte keys) | var
    n: int
    probe: bool
    nf: int
    env: tuple         # ((name, value), ...) planner environment, () = none
    expect: dict       # pbf_tiled_plan fields the row is pinned to
    keys: str = "mix"  # "cpu_only": too large for a GPU test, the planner is pinned on the CPU alone


def layout_args(layout: str) -> tuple[int, bool]:
    """(key_len, aligned) of a layout name."""
    if layout == "hex16":
        return 16, True
    if layout == "var":
        return 0, True
    assert layout.startswith("fix"), layout
    return int(layout[3:]), True


def plan_of(r: Row) -> dict:
    from pebbledb_amd.bloom_filter import plan_tiled
    kl, al = layout_args(r.layout)
    return plan_tiled(r.nb_bytes, r.k, r.n, r.probe, kl, al, r.nf)


def env_id(env: tuple) -> str:
    return ",".join(f"{a}={b}" for a, b in env)


G1 = (("PBF_PART_G", "1"),)
G3 = (("PBF_PART_G", "3"),)
SORT = (("PBF_PART", "sort"),)
SORT_NOPK3 = (("PBF_PART", "sort"), ("PBF_PK3", "0"))
RING = (("PBF_PART", "ring"),)
SPLIT1 = (("PBF_GATHER_SPLIT", "1"),)
G512 = (("PBF_PART_G", "512"),)
G1024 = (("PBF_PART_G", "1024"),)
RING_G1024 = (("PBF_PART", "ring"), ("PBF_PART_G", "1024"))

M16, M32, M128 = 16 * TILE, 256 * TILE, 1024 * TILE  # 2 MiB (16 tiles), 32 MiB, 128 MiB (1024 tiles)
NONPOW2 = 768 * TILE                                  # 3 * 2^25 B: general m
CSPACE = 2 ** 29 + 4                                  # the smallest m > 2^32 the tiled paths take


def B(name, nb, k, n, layout="hex16", env=(), keys="mix", **expect):
    return Row(name, nb, k, layout, n, False, 1, env, expect, keys)


def P(name, nb, k, n, layout="hex16", nf=1, env=(), keys="mix", **expect):
    return Row(name, nb, k, layout, n, True, nf, env, expect, keys)


SORT_P = dict(ring=0, key_mode=0)
ROWS: list[Row] = [
    # ---- tile test (k_tile_probe, and k_tile_probe_set with 2 and 8 filters): TAB 2, TAB 1 whole,
    # TAB 1 in tabw chunks, TAB 0.  A one-tile filter makes every region as long as its workgroup's
    # positions, so the per-word table outgrows the LDS beside the tile at ~100K probes.
    *[P(f"tab2_nf{nf}", M16, 6, 100_000, nf=nf, tab=2, tabw=0, B=16, gtq=256, **SORT_P) for nf in (1, 2, 8)],
    *[P(f"tab1_whole_nf{nf}", M16, 6, 500_000, nf=nf, tab=1, tabw=0, G=245, **SORT_P) for nf in (1, 2, 8)],
    *[P(f"tab1_chunks_nf{nf}", TILE, 8, 100_000, nf=nf, tab=1, tabw=16154, B=1, G=49, **SORT_P) for nf in (1, 2, 8)],
    *[P(f"tab0_nf{nf}", TILE, 8, 135_000, nf=nf, tab=0, tabw=0, B=1, G=66, **SORT_P) for nf in (1, 2, 8)],
    # ---- tile loads: full 2^20-position tiles above take the LDS-DMA path (W % 256 == 0); tiles of
    # 2^10..2^13 positions, a short only tile, nb_bytes % 4 != 0 and a short last tile take load_tile
    *[B(f"tiny_build_{nb}", nb, 3, 1000, tb=tb, B=1, G=1) for nb, tb in ((128, 10), (129, 11), (500, 12), (513, 13))],
    *[P(f"tiny_probe_{nb}", nb, 3, 1000, tb=tb, B=1, tab=2) for nb, tb in ((128, 10), (129, 11), (500, 12), (513, 13))],
    B("short_last_tile_build", 3 * TILE + 5, 3, 1000, B=4, tb=20),
    P("short_last_tile_probe", 3 * TILE + 5, 3, 1000, B=4, tab=2),
    B("two_tiles_build", TILE + 1, 6, 50_000, B=2, ring=0, pk3=1),
    P("two_tiles_probe", TILE + 1, 6, 50_000, B=2, ring=0),
    # ---- ring partition (natural from 128 * k tiles): POW2 / general m, exact k (6, or k equal to
    # its bucket 4 / 8 / 16) and runtime k (5, 7, 12, 10, 1), sub-chunks of 1024 / 512 / 256 keys
    *[B(f"ring_build_k{k}", M128, k, 100_000, ring=32, pow2=1, exact_k=ex, kps=kps, part_kmax=km, key_mode=0)
      for k, ex, kps, km in ((4, 1, 1024, 4), (5, 0, 1024, 8), (6, 1, 1024, 8), (7, 0, 1024, 8), (8, 1, 1024, 8),
                             (10, 0, 512, 16), (16, 1, 512, 16))],
    B("ring_build_256_exact_genm", NONPOW2, 16, 100_000, ring=32, pow2=0, exact_k=1, kps=256, nsub=2),
    B("ring_build_256_runtime_pow2", 512 * TILE, 12, 100_000, ring=32, pow2=1, exact_k=0, kps=256),
    B("ring_build_genm_k6", NONPOW2, 6, 100_000, ring=32, pow2=0, exact_k=1, kps=1024),
    B("ring_build_genm_k5_var", NONPOW2, 5, 100_000, "var", ring=32, pow2=0, exact_k=0, key_mode=2),
    B("ring_build_fix7", M128, 6, 100_000, "fix7", ring=32, exact_k=0, key_mode=1),
    P("ring_probe_k6", M128, 6, 100_000, ring=32, pow2=1, exact_k=1, tab=2, gsplit=8, hw_is_mask=1, key_mode=0),
    P("ring_probe_genm", NONPOW2, 6, 100_000, ring=32, pow2=0, exact_k=1),
    P("ring_probe_k7_var", M128, 7, 100_000, "var", ring=32, exact_k=0, key_mode=2),
    P("ring_probe_fix17", M128, 6, 100_000, "fix17", ring=32, exact_k=0, key_mode=1),
    *[P(f"ring_probe_k1_nf{nf}", 128 * TILE, 1, 100_000, nf=nf, ring=32, exact_k=0, part_kmax=4, gather_nf=8,
        gather_threads=512, hw_is_mask=0, use_hw=1) for nf in (2, 3, 8)],
    # 2^27 + 12 B is 1025 tiles: past the rings' 1024, the counting sort takes it
    B("ring_limit_1025_tiles", M128 + 12, 6, 100_000, ring=0, B=1025, pk3=1),
    # ---- counting-sort partition (natural below 128 * k tiles): layouts, exact k (6, 8, 10) and every
    # register bucket, packed entries, probe sub-chunks of 4096 / 2048 / 1024 keys
    *[B(f"sort_build_k{k}", M16, k, 100_000, ring=0, part_kmax=km, exact_k=ex, pk3=ex, kps=kps, key_mode=0)
      for k, km, ex, kps in ((3, 4, 0, 4096), (5, 8, 0, 3072), (6, 6, 1, 3072), (8, 8, 1, 3072), (10, 10, 1, 3072),
                             (12, 16, 0, 2048), (20, 32, 0, 1024), (32, 32, 0, 1024))],
    *[P(f"sort_probe_k{k}", M16, k, 100_000, ring=0, part_kmax=km, exact_k=ex, kps=kps, key_mode=0, gsplit=8)
      for k, km, ex, kps in ((3, 4, 0, 4096), (5, 8, 0, 2048), (6, 6, 1, 2048), (8, 8, 1, 2048), (10, 10, 1, 2048),
                             (12, 16, 0, 2048), (20, 32, 0, 1024))],
    B("sort_build_var_k8", M16, 8, 100_000, "var", ring=0, key_mode=2, kps=4096, pk3=1, exact_k=1),
    # a 4096-key sub-chunk of k = 8 needs 32768 stage entries: placed in two windows of scap
    P("sort_probe_var_two_windows", M16, 8, 100_000, "var", ring=0, key_mode=2, kps=4096, scap=26580),
    B("sort_build_var_two_windows", 224_649_806, 8, 100_000, "var", ring=0, B=1714, kps=4096, scap=34776, pk3=1),
    *[B(f"sort_build_fix{kl}", M16, 6, 50_000, f"fix{kl}", ring=0, key_mode=1, exact_k=0, part_kmax=8, pk3=0)
      for kl in (1, 7, 15, 17, 64)],
    *[P(f"sort_probe_fix{kl}", M16, 6, 50_000, f"fix{kl}", ring=0, key_mode=1, exact_k=0, part_kmax=8)
      for kl in (1, 7, 15, 17, 64)],
    # ---- workgroup geometry: n one less than, equal to and one more than kps (= kpw here) and the
    # 4096-key pref group; a last workgroup of one key; n below 64; one key
    *[P(f"geom_probe_n{n}", M16, 6, n, ring=0, kps=2048, G=G, kpw=2048 * ns, nsub=ns, nq=1)
      for n, G, ns in ((1, 1, 1), (63, 1, 1), (2047, 1, 1), (2048, 1, 1), (2049, 2, 1), (4095, 2, 1), (4096, 2, 1),
                       (4097, 3, 1))],
    *[B(f"geom_build_n{n}", M16, 6, n, ring=0, kps=3072, G=G, kpw=3072, nsub=1)
      for n, G in ((1, 1), (63, 1), (3071, 1), (3072, 1), (3073, 2), (4097, 2))],
    *[P(f"geom_ring_probe_n{n}", M128, 6, n, ring=32, kps=1024, G=G, kpw=1024) for n, G in ((1023, 1), (1024, 1), (1025, 2))],
    P("geom_nq3_probe", M16, 6, 30_000, env=G3, G=3, kpw=10240, nsub=5, nq=3),
    B("geom_nq3_build", M16, 6, 30_000, env=G3, G=3, kpw=12288, nsub=4, nq=3),
    # n around kpw where kpw is several sub-chunks (nsub > 1): one workgroup allowed, so kpw is n
    # rounded up to kps; three allowed, with a full last workgroup, a last workgroup of one key
    # (2 * kpw + 1) and the step to the next kpw
    *[P(f"geom_g1_probe_n{n}", M16, 6, n, env=G1, G=1, kps=2048, kpw=kpw, nsub=kpw // 2048)
      for n, kpw in ((4095, 4096), (4096, 4096), (4097, 6144))],
    *[B(f"geom_g1_build_n{n}", M16, 6, n, env=G1, G=1, kps=3072, kpw=kpw, nsub=kpw // 3072)
      for n, kpw in ((6143, 6144), (6144, 6144), (6145, 9216))],
    *[P(f"geom_g3_probe_n{n}", M16, 6, n, env=G3, G=G, kps=2048, kpw=kpw, nsub=kpw // 2048)
      for n, G, kpw in ((8191, 2, 4096), (8192, 2, 4096), (8193, 3, 4096), (12287, 3, 4096), (12288, 3, 4096),
                        (12289, 3, 6144))],
    *[B(f"geom_g3_build_n{n}", M16, 6, n, env=G3, G=G, kps=3072, kpw=kpw, nsub=kpw // 3072)
      for n, G, kpw in ((12288, 2, 6144), (12289, 3, 6144), (18432, 3, 6144), (18433, 3, 9216))],
    # ---- hit-mask finish: whole words into the caller's mask (hw_is_mask) above; ragged tails here
    *[P(f"mask_tail_n{n}", M16, 6, n, use_hw=1, hw_is_mask=0) for n in (100_001, 99_999, 100_004)],
    # ---- environment: forced partitions, one workgroup, one gather split
    B("forced_sort_1024_tiles_pk3", M128, 6, 200_000, env=SORT, ring=0, B=1024, pk3=1, part_kmax=6),
    P("forced_sort_1024_tiles_probe", M128, 6, 200_000, env=SORT, ring=0, B=1024, kps=2048),
    B("forced_sort_k10_pk3", M128, 10, 200_000, env=SORT, ring=0, pk3=1, part_kmax=10),
    B("forced_sort_exact_unpacked", M128, 6, 200_000, env=SORT_NOPK3, ring=0, pk3=0, exact_k=1, part_kmax=6),
    B("forced_sort_exact_unpacked_var_k8", M16, 8, 100_000, "var", env=SORT_NOPK3, ring=0, pk3=0, exact_k=1),
    B("forced_ring_16_tiles_build", M16, 6, 200_000, env=RING, ring=32, B=16, kps=256, nsub=4),
    P("forced_ring_16_tiles_probe", M16, 6, 200_000, env=RING, ring=32, B=16, kps=1024),
    P("forced_ring_16_tiles_probe_nf3", M16, 6, 200_000, nf=3, env=RING, ring=32, B=16, gather_nf=8),
    P("split1_sort", M16, 6, 100_000, env=SPLIT1, gsplit=1, use_hw=0, hw_is_mask=0, ring=0),
    P("split1_ring", M128, 6, 100_000, env=SPLIT1, gsplit=1, use_hw=0, hw_is_mask=0, ring=32),
    P("split1_set", M16, 6, 100_000, nf=2, env=SPLIT1, gsplit=1, use_hw=1, hw_is_mask=0),
    # one workgroup of 1.5M keys: regions past kRingMaxCap, the ring plan falls back to the sort
    B("ring_falls_back_to_sort", M128, 6, 1_500_000, env=G1, ring=0, B=1024, G=1, pk3=1),
    # two pipelines in one call (the gather's key bitmap of one workgroup outgrows the LDS)
    P("two_pipelines", M128, 6, 1_300_000, env=G1, ring=32, G=1, pipelines=2, keys_per_pipeline=650_048, gtq=0,
      hw_is_mask=1),
    # 8 key bitmaps of 100K keys: the 1024-thread set gather
    P("set_gather_1024_threads", 128 * TILE, 1, 100_000, nf=8, env=G1, ring=32, G=1, gather_threads=1024, pipelines=1),
    # ---- what the kernels of a set probe's extra rounds see: 2x and 4x as many partition workgroups as
    # CUs (G = 512, 1024), with their smaller key bitmaps, k_gather_ring<8> over G x gsplit
    # workgroups and the tile test over more than 256 regions per tile.  On 1024 tiles the regions
    # stay short (TAB 2); on 16 tiles with forced rings the table of 1024 regions is walked in
    # tabw chunks.  (The planner's own `rounds` stays 1 under a forced count; rows set_rounds_* below.)
    *[P(f"set_g{g}_nf{nf}", M128, 6, 1 << 20, nf=nf, env=env, ring=32, G=g, kpw=(1 << 20) // g, tab=2, tabw=0,
        gather_threads=512, gather_nf=8, rounds=1)
      for g, env in ((512, G512), (1024, G1024)) for nf in (2, 8)],
    *[P(f"set_g1024_chunks_nf{nf}", M16, 6, 1 << 20, nf=nf, env=RING_G1024, ring=32, G=1024, kpw=1024, tab=1,
        tabw=tabw, gather_threads=512, gather_nf=8) for nf, tabw in ((2, 12254), (8, 12254))],
    # ---- m > 2^32 (the tile space is the 2^32 reachable positions; the upper tiles start at a word
    # that is 1 mod 4), with one workgroup so that the gather's splits rise to 32
    B("cspace_build", CSPACE, 6, 200_000, env=G1, cspace=1, B=4096, tiled=1, ring=0),
    P("cspace_probe_split32", CSPACE, 6, 200_000, env=G1, cspace=1, B=4096, gsplit=32, ring=0),
    B("cspace_unaligned_is_atomic", 2 ** 29 + 1, 6, 200_000, tiled=0, tiled_ok=0, B=4096),
    B("most_tiles_4096", 2 ** 29, 6, 200_000, tiled=1, B=4096, cspace=0, ring=0),
    # ---- too large for a quick GPU test (tens of millions of keys; a forced workgroup count switches
    # the extra rounds off): planner only.  The 100M-key multi-filter test of test_gpu_multi.py runs
    # rounds = 3.
    P("set_rounds_2", M128, 6, 50_000_000, nf=8, keys="cpu_only", ring=32, rounds=2, gather_threads=1024, tab=1),
    P("set_rounds_3", M128, 6, 100_000_000, nf=8, keys="cpu_only", ring=32, rounds=3, tab=1, tabw=13298),
    P("set_rounds_4", M128, 6, 130_000_000, nf=8, keys="cpu_only", ring=32, rounds=4, G=1024),
    P("bench_c3_probe", 2 ** 30, 8, 200_000_000, "var", keys="cpu_only", ring=0, gsplit=32, tab=1, tabw=0, pipelines=2,
      gtq=0, cspace=1),
]
assert len({r.name for r in ROWS}) == len(ROWS)
ENVS: list[tuple] = sorted({r.env for r in ROWS if r.env})


def gpu_rows(env: tuple = ()) -> list[Row]:
    return [r for r in ROWS if r.env == env and r.keys != "cpu_only"]
