// A memtable flush's record run from a put log (reference MemTableIterator over the red-black
// tree, src/iterators.py:24-55; MemTable.put / create_from_wal, src/memtable.py:29-72; the tree
// replaces the data of a key it already holds, src/red_black_tree.py:118-120), gfx950.
//
// The log is the puts of one memtable in put order, packed: keys ‖ u64 key_offsets[n+1], values ‖
// u64 value_offsets[n+1].  The run is every distinct key in ascending unsigned bytewise order,
// each with the value of its LAST put.  The puts are sorted by (key, put index): the order is
// strict, so no pass needs a stable variant, the result is deterministic, and the last put of a
// key is the last entry of its group of equal keys.
//
//   * k_mt_entries — one lane per put: a 16-byte entry {key_prefix, put index, klen}.
//   * k_mt_tile_sort — one workgroup sorts one tile of kMtTile entries in LDS with a bitonic
//     network (66 steps for 2048 entries); the last tile is padded with a sentinel that sorts
//     after every entry and is never written out.
//   * k_mt_merge_rank — one merge pass by rank (as k_merge_rank): runs of `run` entries in groups
//     of kMtFanIn; every entry finds its place with one lower-bound search per sibling run and
//     is written to group base + own index + the sum of the ranks in the other buffer.  A group
//     of one run (the odd run left over) has no sibling: it is copied through.
//   * k_mt_mark — one lane per sorted position: a MergeSlot {put index, klen, vlen, keep}, keep =
//     the next entry's key differs (or there is none).
//   * k_merge_tile_sums / k_merge_tile_scan / k_merge_offsets (sstable_merge_kernels.hpp) run
//     over those slots unchanged; k_mt_copy is k_merge_copy with the log as its source.
//
// The comparator decides by the 8-byte prefix; equal zero-padded prefixes do not imply equal keys
// ("a" < "a\x00"), so a tie reads both keys from the log and runs sst_key_cmp; equal keys decide
// by put index.
//
// Every loop is bounded by a count the host validated: the offsets arrays ascend from 0 and every
// key and value is shorter than 2^31 bytes (pbf_log_sort checks before any launch), a put index
// an entry carries is below n, and a binary search takes at most 33 halvings.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sstable_merge_kernels.hpp"

namespace pbf {

// The packed put log in device memory.
struct MtLog {
    const uint8_t* keys;
    const uint64_t* key_offsets;  // [n+1], from 0
    const uint8_t* values;
    const uint64_t* value_offsets;  // [n+1], from 0
    uint64_t n;
};

struct alignas(16) MtEntry {
    uint64_t prefix;  // key_prefix of the key
    uint32_t put;     // index in the log
    uint32_t klen;
};
static_assert(sizeof(MtEntry) == 16, "one 16-byte LDS slot per entry");

constexpr uint32_t kMtTile = kScanTile;      // entries per sorted tile: 2048 x 16 B = 32 KiB of LDS
constexpr uint32_t kMtSortThreads = 512;     // 2 compare-exchanges per thread and step
constexpr uint32_t kMtFanIn = 8;             // runs merged into one per pass
constexpr uint32_t kMtSentinel = 0xFFFFFFFFu;  // put index of the padding (n < 2^32 - 1)

// An entry as the one 16-byte word it is loaded and stored as (global and LDS).
typedef uint32_t MtWord __attribute__((ext_vector_type(4)));
__device__ __forceinline__ MtEntry mt_unpack(const MtWord& v) {
    return MtEntry{uint64_t(v.x) | (uint64_t(v.y) << 32), v.z, v.w};
}
__device__ __forceinline__ MtWord mt_pack(const MtEntry& e) {
    return MtWord{uint32_t(e.prefix), uint32_t(e.prefix >> 32), e.put, e.klen};
}
__device__ __forceinline__ MtEntry ld_entry(const MtEntry* p) { return mt_unpack(gld(reinterpret_cast<const MtWord*>(p))); }

__device__ __forceinline__ const uint8_t* mt_key(const MtLog& log, uint32_t put) {
    return log.keys + gld(log.key_offsets + put);
}

// The keys of two entries, neither a sentinel: <0, 0, >0.
__device__ __forceinline__ int mt_key_cmp(const MtLog& log, const MtEntry& a, const MtEntry& b) {
    if (a.prefix != b.prefix) return a.prefix < b.prefix ? -1 : 1;
    // keys of at most 8 bytes with equal padded prefixes agree up to the shorter one's end
    if (a.klen <= 8 && b.klen <= 8) return a.klen < b.klen ? -1 : (a.klen > b.klen ? 1 : 0);
    return sst_key_cmp(mt_key(log, a.put), a.klen, mt_key(log, b.put), b.klen);
}

// a before b in (key, put index) order; the sentinel after every entry.
__device__ __forceinline__ bool mt_less(const MtLog& log, const MtEntry& a, const MtEntry& b) {
    if (a.put == kMtSentinel) return false;
    if (b.put == kMtSentinel) return true;
    const int c = mt_key_cmp(log, a, b);
    return c < 0 || (c == 0 && a.put < b.put);
}

__global__ void __launch_bounds__(256) k_mt_entries(MtLog log, MtEntry* __restrict__ entries) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < log.n; i += stride) {
        const uint64_t o = gld(log.key_offsets + i);
        const uint32_t kl = uint32_t(gld(log.key_offsets + i + 1) - o);
        entries[i] = MtEntry{key_prefix(log.keys + o, kl), uint32_t(i), kl};
    }
}

// entries[tile * kMtTile, +kMtTile) ∩ [0, n) sorted in place.
__global__ void __launch_bounds__(kMtSortThreads) k_mt_tile_sort(MtLog log, MtEntry* __restrict__ entries) {
    __shared__ MtWord sh[kMtTile];  // (whole 16-byte LDS reads and writes)
    const uint64_t base = uint64_t(blockIdx.x) * kMtTile;
    MtWord* tile = reinterpret_cast<MtWord*>(entries + base);
    for (uint32_t j = threadIdx.x; j < kMtTile; j += kMtSortThreads)
        sh[j] = base + j < log.n ? gld(tile + j) : mt_pack(MtEntry{~0ull, kMtSentinel, 0});
    __syncthreads();
    for (uint32_t k = 2; k <= kMtTile; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t p = threadIdx.x; p < kMtTile / 2; p += kMtSortThreads) {
                const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const MtWord wa = sh[i], wb = sh[l];
                const MtEntry a = mt_unpack(wa), b = mt_unpack(wb);
                const bool up = (i & k) == 0;
                if (up ? mt_less(log, b, a) : mt_less(log, a, b)) {
                    sh[i] = wb;
                    sh[l] = wa;
                }
            }
            __syncthreads();
        }
    }
    // the sentinels are the tile's last entries: what lies below n is the puts
    for (uint32_t j = threadIdx.x; j < kMtTile; j += kMtSortThreads)
        if (base + j < log.n) tile[j] = sh[j];
}

// The entries of run[0, len) that sort before e.
__device__ __forceinline__ uint64_t mt_lower_bound(const MtLog& log, const MtEntry* __restrict__ run, uint64_t len,
                                                   const MtEntry& e) {
    uint64_t lo = 0, hi = len;
    for (int it = 0; it < 33 && lo < hi; ++it) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (mt_less(log, ld_entry(run + mid), e))
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// src = sorted runs of `run` entries (the last one shorter); dst = sorted runs of kMtFanIn * run.
__global__ void __launch_bounds__(256) k_mt_merge_rank(MtLog log, const MtEntry* __restrict__ src,
                                                       MtEntry* __restrict__ dst, uint64_t run) {
    const uint64_t n = log.n, stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        const MtEntry e = ld_entry(src + g);
        const uint64_t r = g / run, first = r - r % kMtFanIn;  // the lane's run, its group's first run
        uint64_t rank = g - r * run;
        for (uint32_t u = 0; u < kMtFanIn; ++u) {
            const uint64_t s = first + u, s0 = s * run;
            if (s == r || s0 >= n) continue;
            rank += mt_lower_bound(log, src + s0, min(run, n - s0), e);
        }
        const uint64_t at = first * run + rank;
        if (at < n) dst[at] = e;  // (the ranks of a group are a permutation of its extent)
    }
}

// slots[r] of the sorted entries: the last put of every key is kept.
__global__ void __launch_bounds__(256) k_mt_mark(MtLog log, const MtEntry* __restrict__ sorted,
                                                 MergeSlot* __restrict__ slots) {
    const uint64_t n = log.n, stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t r = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; r < n; r += stride) {
        const MtEntry e = ld_entry(sorted + r);
        if (e.put >= n) continue;  // (never: the slot stays zeroed, that is dropped)
        const bool keep = r + 1 == n || mt_key_cmp(log, e, ld_entry(sorted + r + 1)) != 0;
        const uint32_t vl = uint32_t(gld(log.value_offsets + e.put + 1) - gld(log.value_offsets + e.put));
        slots[r] = MergeSlot{e.put, e.klen, vl, keep ? kMergeKeep : 0u};
    }
}

// k_merge_copy with the packed log as its source: slot.rec_off is the put index.  put_out (or
// null) receives the put index of every output record.
__global__ void __launch_bounds__(256) k_mt_copy(MtLog log, const MergeSlot* __restrict__ slots,
                                                 const uint64_t* __restrict__ pos, const uint64_t* __restrict__ totals,
                                                 uint64_t* __restrict__ key_offsets,
                                                 uint64_t* __restrict__ value_offsets, uint8_t* __restrict__ keys_out,
                                                 uint8_t* __restrict__ values_out, uint32_t* __restrict__ put_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        key_offsets[totals[0]] = totals[1];
        value_offsets[totals[0]] = totals[2];
    }
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint64_t groups = uint64_t(gridDim.x) * (blockDim.x / kGatherLanes);
    for (uint64_t r = uint64_t(blockIdx.x) * (blockDim.x / kGatherLanes) + threadIdx.x / kGatherLanes; r < log.n;
         r += groups) {
        const uint4 s = gld(reinterpret_cast<const uint4*>(slots + r));
        if (!(s.w & kMergeKeep) || s.x >= log.n) continue;
        const uint64_t j = pos[r];
        if (lane == 0 && put_out) put_out[j] = s.x;
        if (s.y) merge_copy_bytes(keys_out + key_offsets[j], log.keys + gld(log.key_offsets + s.x), s.y, lane);
        if (s.z) merge_copy_bytes(values_out + value_offsets[j], log.values + gld(log.value_offsets + s.x), s.z, lane);
    }
}

}  // namespace pbf
