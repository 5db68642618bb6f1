"""A numpy restatement of the device planner (pebbledb_amd/csrc/sstable_plan_kernels.hpp), step for
step: `next` by a windowed search on P[i] = ko[i] + vo[i] + 8 i, every record's exit from its chunk
and the hops to it by pointer jumping, a walk over the chunks that carries the builder position
and only goes block by block inside the chunk where the position crosses max_sstable_size, and
the expansion of the chunks crossed whole.  It exists so that the split and tail rules can be
checked against ``sstable_data.plan_blocks`` / ``plan_compaction`` without a GPU."""
from __future__ import annotations

import numpy as np

CHUNK = 8192
OPEN = 0xFFFFFFFF


class Oversize(ValueError):
    pass


def plan_next(P: np.ndarray, block_size: int) -> np.ndarray:
    """k_plan_next: nxt[s] = the largest e in [s, min(n, s + CHUNK)] with P[e] <= P[s] + block_size;
    e == n is stored as OPEN."""
    n = len(P) - 1
    s = np.arange(n, dtype=np.int64)
    lo, hi = s.copy(), np.minimum(s + CHUNK, n)
    limit = P[:n] + block_size
    for _ in range(14):
        live = lo < hi
        mid = lo + (hi - lo + 1) // 2
        ok = P[np.minimum(mid, n)] <= limit
        lo = np.where(live & ok, mid, lo)
        hi = np.where(live & ~ok, mid - 1, hi)
    if np.any(lo == s):
        raise Oversize("a record is larger than block_size")
    return np.where(lo >= n, OPEN, lo).astype(np.int64)


def plan_chunks(nxt: np.ndarray, chunk: int = CHUNK):
    """k_plan_chunks: (exit, hops) of every record, by pointer jumping chunk by chunk."""
    n = len(nxt)
    idx = np.arange(n, dtype=np.int64)
    end = np.minimum((idx // chunk + 1) * chunk, n)
    opened = nxt == OPEN
    done = opened | (nxt >= end)
    val = np.where(opened, idx, nxt)
    hops = np.where(opened, 0, 1).astype(np.int64)
    for _ in range(14):
        live = ~done
        if not live.any():
            break
        t = np.where(live, val, 0)
        val, hops, done = (np.where(live, val[t], val), np.where(live, hops + hops[t], hops),
                           np.where(live, done[t], done))
    assert done.all()
    return val, hops


def plan_device_model(ko, vo, block_size: int, max_sstable_size: int = 0, chunk: int = CHUNK):
    """(block_first, block_out, table_blocks, written) as the device planner writes them;
    max_sstable_size 0 = blocks mode."""
    ko, vo = np.asarray(ko).astype(np.int64), np.asarray(vo).astype(np.int64)
    n = len(ko) - 1
    P = ko + vo + 8 * np.arange(n + 1, dtype=np.int64)
    nxt = plan_next(P, block_size)
    ex, hp = plan_chunks(nxt, chunk)
    compaction = max_sstable_size != 0
    bf, bo, tb = {}, {}, [0]
    segs = {}  # one per chunk at most: a chunk crossed whole is left for good
    nb = out = s = pos = 0
    nb_t0 = out_t0 = s_t0 = 0
    written = n
    while s < n:
        cend = min((s // chunk + 1) * chunk, n)
        e, h = int(ex[s]), int(hp[s])
        span = int(P[e] - P[s]) + 2 * (e - s) + 2 * h
        if not compaction or pos + span < max_sstable_size:
            if h:
                assert s // chunk not in segs
                segs[s // chunk] = (nb, out, s, h)
            nb, out, pos, s = nb + h, out + span, pos + span, e
            if e < cend:
                if not compaction or pos > 0:
                    bf[nb], bo[nb] = e, out
                    out += int(P[n] - P[e]) + 2 * (n - e) + 2
                    nb += 1
                    tb.append(nb)
                else:
                    nb, out, written = nb_t0, out_t0, s_t0
                s = n
            continue
        while True:
            e1 = int(nxt[s])
            assert s < e1 < n
            bf[nb], bo[nb] = s, out
            nb += 1
            bsz = int(P[e1] - P[s]) + 2 * (e1 - s) + 2
            out, pos, s = out + bsz, pos + bsz, e1
            if pos >= max_sstable_size:
                break
        bf[nb], bo[nb] = s, out
        nb += 1
        out += int(P[s + 1] - P[s]) + 4
        tb.append(nb)
        s += 1
        pos = 0
        nb_t0, out_t0, s_t0 = nb, out, s
    bf[nb], bo[nb] = written, out
    for b0, o0, start, h in segs.values():  # k_plan_expand
        x = start
        for j in range(h):
            assert (b0 + j) not in bf
            bf[b0 + j] = x
            bo[b0 + j] = o0 + int(P[x] - P[start]) + 2 * (x - start) + 2 * j
            x = int(nxt[x])
    assert sorted(k for k in bf if k <= nb) == list(range(nb + 1)), "every entry up to nblocks is written once"
    assert max(bf) == nb, "nothing past nblocks + 1 entries"
    return (np.array([bf[i] for i in range(nb + 1)], dtype=np.uint64),
            np.array([bo[i] for i in range(nb + 1)], dtype=np.uint64), np.array(tb, dtype=np.uint64), written)
