// The device memtable's read side (reference MemTable.get, src/memtable.py:74-79; the memtable
// stage of LsmStorage.get and LsmStorage.scan, src/lsm_storage.py:153-162 and :184-190), gfx950.
//
// A memtable owns ONE run in HBM: its records strictly ascending and de-duplicated in
// pbf_sst_merge's output layout (keys ‖ u64 key_off[n+1], values ‖ u64 val_off[n+1]) plus
// u64 prefix[n], key_prefix of every key: a search step is decided by one load wherever the
// prefixes differ.
//
//   * run_lower_bound — the index of a run's first record whose key is >= the probe, and whether
//     that key equals it.  On a prefix tie keys of at most 8 bytes order by length, longer ones run
//     sst_key_cmp on the stored key (memtable_kernels.hpp's comparator rule: equal zero-padded
//     prefixes do not imply equal keys, "a" < "a\x00").
//   * k_run_prefix — prefix[i] of a new run, one lane per record.
//   * k_mt_get — one lane per key walks the memtables in list order and stops at the first that
//     holds it; one wave ballot per 64 keys gives the miss mask's word (hit-mask layout).
//   * k_src_bounds / k_src_sizes / k_src_rank / k_src_copy — sstable_scan_kernels.hpp's bounds,
//     sizes and rank formula and the merge's copy over MIXED sources: sources [0, nm) are runs,
//     source nm + t is table t of the MergeSet.  A MergeSlot's source index says which kind its
//     bytes come from: for a run rec_off is the record's index, for a table its offset in the data
//     section.  The three scans and k_merge_offsets run over the slots unchanged.  A memtable's
//     apply is the same rank kernel with one range, full windows and two runs (new batch first).
//   * k_src_gather — k_gather_values with (base pointer, length) per source, for a batch whose
//     hits come partly from memtables (entry -2 - m) and partly from tables (entry t >= 0).
//
// Bounds: every loop is bounded by a count from a handle (a run's n, a table's validated index) or
// by a host-checked offsets array, a search by 32 halvings; a run index met in a slot is checked
// against the run's n before it is used; a rank outside its range's span is dropped, never
// written, and the slots are zeroed first; no load wider than a byte leaves a key's or value's
// extent except the 16-byte copy chunks, which stay inside the extent they copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sstable_scan_kernels.hpp"

namespace pbf {

constexpr uint32_t kMtMaxPerCall = 16;  // memtables of one call

// One memtable's run, by value in the kernel arguments.
struct RunView {
    const uint8_t* keys;
    const uint64_t* key_off;  // [n+1], from 0
    const uint8_t* vals;
    const uint64_t* val_off;  // [n+1], from 0
    const uint64_t* prefix;   // [n]
    uint64_t n;               // < 2^32 - 1
};

struct MtSet {
    RunView run[kMtMaxPerCall];
    uint32_t nm;
};

// Mixed sources of a scan or an apply: runs first, then the tables of `tab`.
struct SrcSet {
    MergeSet tab;
    RunView run[kMtMaxPerCall];
    uint32_t nm;
};
static_assert(sizeof(SrcSet) <= 3800, "the source set travels in the kernel arguments (4 KiB)");

// (base, length) of every source's value bytes: memtables [0, nm), then tables.
struct GatherSrc {
    const uint8_t* base[kMtMaxPerCall + kSstTablesPerLaunch];
    uint64_t len[kMtMaxPerCall + kSstTablesPerLaunch];
    uint32_t nm, nt;
};

// The first record of the run whose key >= the probe, in [0, n]; *eq = its key equals the probe.
__device__ __forceinline__ uint32_t run_lower_bound(const RunView& r, const uint8_t* key, uint32_t kl, uint64_t kpre,
                                                    bool* eq) {
    *eq = false;
    uint64_t lo = 0, hi = r.n;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const uint64_t p = gld(r.prefix + mid);
        int c;
        if (p != kpre) {
            c = p < kpre ? -1 : 1;
        } else {
            const uint64_t a = gld(r.key_off + mid);
            const uint32_t sl = uint32_t(gld(r.key_off + mid + 1) - a);
            if (sl <= 8 && kl <= 8)  // equal padded prefixes: the keys agree up to the shorter one's end
                c = sl < kl ? -1 : (sl > kl ? 1 : 0);
            else
                c = sst_key_cmp(r.keys + a, sl, key, kl);
        }
        if (c == 0) {  // keys ascend strictly: this is the only one
            *eq = true;
            lo = mid;
            break;
        }
        if (c < 0)
            lo = mid + 1;
        else
            hi = mid;
    }
    return uint32_t(lo);
}

__global__ void __launch_bounds__(256) k_run_prefix(const uint8_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ key_off, uint64_t n,
                                                    uint64_t* __restrict__ prefix) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t a = gld(key_off + i);
        prefix[i] = key_prefix(keys + a, uint32_t(gld(key_off + i + 1) - a));
    }
}

// MemTable.get over the memtables in list order for a batch: src[i] = the first memtable that
// holds key i or -1, val_off[i] = the value's offset in that run's value bytes, val_len[i] = its
// length, -1 if absent.  miss_mask: bit (i & 7) of byte i >> 3 = no memtable holds key i; the
// ceil(n/8) bytes are all written, pad bits zero.
template <int KM>
__global__ void __launch_bounds__(256) k_mt_get(KeySet ks, uint64_t n, MtSet set, int32_t* __restrict__ src,
                                                uint64_t* __restrict__ val_off, int32_t* __restrict__ val_len,
                                                uint8_t* __restrict__ miss_mask) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x, nbytes = (n + 7) / 8;
    const uint32_t lane = threadIdx.x & 63u;
    // (whole waves iterate together: the ballot needs every lane of a 64-key word)
    for (uint64_t i0 = uint64_t(blockIdx.x) * blockDim.x + (threadIdx.x & ~63u); i0 < n; i0 += stride) {
        const uint64_t i = i0 + lane;
        bool miss = false;
        if (i < n) {
            const uint8_t* kp;
            uint32_t kl;
            if constexpr (KM == kVar) {
                const uint64_t o0 = gld(ks.off0), a = gld(ks.offsets + i);
                kp = ks.data + (a - o0);
                kl = uint32_t(gld(ks.offsets + i + 1) - a);
            } else {
                kp = ks.data + i * uint64_t(ks.key_len);
                kl = ks.key_len;
            }
            const uint64_t kpre = key_prefix(kp, kl);
            int32_t mf = -1, vl = -1;
            uint64_t vo = 0;
            for (uint32_t m = 0; m < set.nm; ++m) {
                const RunView& r = set.run[m];
                bool eq;
                const uint32_t lb = run_lower_bound(r, kp, kl, kpre, &eq);
                if (eq) {
                    vo = gld(r.val_off + lb);
                    vl = int32_t(gld(r.val_off + lb + 1) - vo);
                    mf = int32_t(m);
                    break;
                }
            }
            src[i] = mf;
            val_off[i] = vo;
            val_len[i] = vl;
            miss = mf < 0;
        }
        const uint64_t word = __ballot(miss);  // lanes past n vote 0: the pad bits
        if (lane == 0) {
            const uint64_t b0 = i0 >> 3, nb = min(uint64_t(8), nbytes - b0);
            for (uint64_t j = 0; j < nb; ++j) miss_mask[b0 + j] = uint8_t(word >> (8 * j));
        }
    }
}

// ------------------------------------------------------------------ mixed sources
__device__ __forceinline__ uint32_t src_count(const SrcSet& set, uint32_t u) {
    if (u < set.nm) return uint32_t(set.run[u].n);
    const uint32_t t = u - set.nm;
    return gld(set.tab.rec_base[t] + set.tab.nblocks[t]);
}

__device__ __forceinline__ uint32_t src_lower_bound(const SrcSet& set, uint32_t u, const uint8_t* key, uint32_t kl,
                                                    uint64_t kpre, bool* eq) {
    if (u < set.nm) return run_lower_bound(set.run[u], key, kl, kpre, eq);
    const uint32_t t = u - set.nm;
    const SstView v{set.tab.data[t], set.tab.index[t], set.tab.last_prefix[t], set.tab.nblocks[t]};
    return sst_lower_bound(v, set.tab.rec_base[t], key, kl, kpre, eq);
}

// Record i of source u: what a MergeSlot names it by (a run: its index; a table: its offset in
// the data section), its sizes and its key.  The source holds at least one record.
__device__ __forceinline__ uint32_t src_record_at(const SrcSet& set, uint32_t u, uint32_t i, uint32_t* kl, uint32_t* vl,
                                                  const uint8_t** key) {
    if (u < set.nm) {
        const RunView& r = set.run[u];
        const uint64_t j = min(uint64_t(i), r.n - 1);  // (inside the run whatever the window holds)
        const uint64_t a = gld(r.key_off + j), b = gld(r.val_off + j);
        *kl = uint32_t(gld(r.key_off + j + 1) - a);
        *vl = uint32_t(gld(r.val_off + j + 1) - b);
        *key = r.keys + a;
        return uint32_t(j);
    }
    const uint32_t t = u - set.nm;
    const uint32_t rec_off = merge_record_at(set.tab, t, i, kl, vl);
    *key = set.tab.data[t] + rec_off + 4;
    return rec_off;
}

// k_scan_bounds over mixed sources: segment s = q * nsrc + u.
__global__ void __launch_bounds__(256) k_src_bounds(SrcSet set, ScanBounds b, uint64_t nseg,
                                                    uint32_t* __restrict__ seg_lo, uint32_t* __restrict__ seg_cnt) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint32_t nsrc = set.nm + set.tab.nt;
    const uint64_t l0 = gld(b.lower_offsets), u0 = gld(b.upper_offsets);
    for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < nseg; s += stride) {
        const uint64_t q = s / nsrc;
        const uint32_t u = uint32_t(s - q * nsrc);
        const uint64_t la = gld(b.lower_offsets + q), lb = gld(b.lower_offsets + q + 1);
        const uint8_t* lk = b.lowers + (la - l0);
        const uint32_t ll = uint32_t(lb - la);
        bool eq;
        const uint32_t lo = src_lower_bound(set, u, lk, ll, key_prefix(lk, ll), &eq);
        uint32_t hi;
        if (b.upper_open && b.upper_open[q]) {
            hi = src_count(set, u);
        } else {
            const uint64_t ua = gld(b.upper_offsets + q), ub = gld(b.upper_offsets + q + 1);
            const uint8_t* uk = b.uppers + (ua - u0);
            const uint32_t ul = uint32_t(ub - ua);
            hi = src_lower_bound(set, u, uk, ul, key_prefix(uk, ul), &eq);
            hi += eq ? 1u : 0u;
        }
        hi = max(hi, lo);  // lower > upper: nothing
        seg_lo[s] = lo;
        seg_cnt[s] = hi - lo;
    }
}

// k_scan_sizes over mixed sources.
__global__ void __launch_bounds__(kScanThreads) k_src_sizes(SrcSet set, const uint64_t* __restrict__ seg_base,
                                                            const uint32_t* __restrict__ seg_lo, uint64_t nseg,
                                                            uint64_t n, unsigned long long* __restrict__ totals) {
    __shared__ uint64_t sh[kScanThreads];
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint32_t nsrc = set.nm + set.tab.nt;
    uint64_t kb = 0, vb = 0;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint64_t s = scan_segment_of(seg_base, nseg, g);
        const uint32_t u = uint32_t(s % nsrc);
        const uint32_t i = gld(seg_lo + s) + uint32_t(g - gld(seg_base + s));
        uint32_t kl, vl;
        const uint8_t* key;
        src_record_at(set, u, i, &kl, &vl, &key);
        kb += kl;
        vb += vl;
    }
    uint64_t tk, tv;
    block_exclusive(kb, sh, &tk);
    block_exclusive(vb, sh, &tv);
    if (threadIdx.x == 0) {
        if (tk) atomicAdd(totals, static_cast<unsigned long long>(tk));
        if (tv) atomicAdd(totals + 1, static_cast<unsigned long long>(tv));
    }
}

// k_scan_rank over mixed sources (DESIGN.md "Rank inside the windows"): n = seg_base[nseg];
// slots[n] zeroed before the launch.
__global__ void __launch_bounds__(256) k_src_rank(SrcSet set, const uint64_t* __restrict__ seg_base,
                                                  const uint32_t* __restrict__ seg_lo,
                                                  const uint32_t* __restrict__ seg_cnt, uint64_t nseg, uint64_t n,
                                                  MergeSlot* __restrict__ slots) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    const uint32_t nsrc = set.nm + set.tab.nt;
    for (uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; g < n; g += stride) {
        const uint64_t s = scan_segment_of(seg_base, nseg, g);
        const uint32_t t = uint32_t(s % nsrc);
        const uint64_t s0 = s - t;  // q * nsrc
        const uint32_t j = uint32_t(g - gld(seg_base + s));
        uint32_t kl, vl;
        const uint8_t* key;
        const uint32_t rec = src_record_at(set, t, gld(seg_lo + s) + j, &kl, &vl, &key);
        const uint64_t kpre = key_prefix(key, kl);
        const uint64_t first = gld(seg_base + s0), end = gld(seg_base + s0 + nsrc);  // the range's span
        uint64_t rank = first + j;
        uint32_t keep = kMergeKeep;
        for (uint32_t u = 0; u < nsrc; ++u) {
            if (u == t || gld(seg_cnt + s0 + u) == 0) continue;  // an empty window holds nothing below the key
            bool eq;
            const uint32_t lb = src_lower_bound(set, u, key, kl, kpre, &eq);
            rank += lb - gld(seg_lo + s0 + u);
            if (u < t && eq) {  // source u's copy comes first and is the one that survives
                rank += 1;
                keep = 0;
            }
        }
        if (rank >= first && rank < end) slots[rank] = MergeSlot{rec, kl, vl, t | keep};
    }
}

// k_merge_copy over mixed sources: a run's record through its offsets (as k_mt_copy reads the
// log), a table's through its header.
__global__ void __launch_bounds__(256) k_src_copy(SrcSet set, const MergeSlot* __restrict__ slots, uint64_t n,
                                                  const uint64_t* __restrict__ pos, const uint64_t* __restrict__ totals,
                                                  uint64_t* __restrict__ key_offsets,
                                                  uint64_t* __restrict__ value_offsets, uint8_t* __restrict__ keys_out,
                                                  uint8_t* __restrict__ values_out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        key_offsets[totals[0]] = totals[1];
        value_offsets[totals[0]] = totals[2];
    }
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint32_t nsrc = set.nm + set.tab.nt;
    const uint64_t groups = uint64_t(gridDim.x) * (blockDim.x / kGatherLanes);
    for (uint64_t r = uint64_t(blockIdx.x) * (blockDim.x / kGatherLanes) + threadIdx.x / kGatherLanes; r < n;
         r += groups) {
        const uint4 s = gld(reinterpret_cast<const uint4*>(slots + r));
        if (!(s.w & kMergeKeep)) continue;
        const uint32_t u = s.w & ~kMergeKeep;
        if (u >= nsrc) continue;
        const uint64_t j = pos[r];
        const uint8_t *ksrc, *vsrc;
        if (u < set.nm) {
            const RunView& run = set.run[u];
            if (s.x >= run.n) continue;
            ksrc = run.keys + gld(run.key_off + s.x);
            vsrc = run.vals + gld(run.val_off + s.x);
        } else {
            const uint8_t* rec = set.tab.data[u - set.nm] + s.x;
            ksrc = rec + 4;
            vsrc = rec + 8 + s.y;
        }
        if (s.y) merge_copy_bytes(keys_out + key_offsets[j], ksrc, s.y, lane);
        if (s.z) merge_copy_bytes(values_out + value_offsets[j], vsrc, s.z, lane);
    }
}

// out[offs[i], offs[i+1]) = value i.  where[i] names the source: t >= 0 a table, -2 - m a
// memtable, -1 none.  An entry with a length that names no source, or that does not lie inside
// its source's bytes, is not copied and counts in *err.
__global__ void __launch_bounds__(256) k_src_gather(GatherSrc set, const int32_t* __restrict__ where,
                                                    const uint64_t* __restrict__ val_off,
                                                    const int32_t* __restrict__ val_len, uint64_t n,
                                                    const uint64_t* __restrict__ offs, uint8_t* __restrict__ out,
                                                    unsigned int* __restrict__ err) {
    const uint32_t lane = threadIdx.x % kGatherLanes;
    const uint64_t groups = uint64_t(gridDim.x) * (blockDim.x / kGatherLanes);
    for (uint64_t i = uint64_t(blockIdx.x) * (blockDim.x / kGatherLanes) + threadIdx.x / kGatherLanes; i < n;
         i += groups) {
        const int32_t len = val_len[i];
        if (len <= 0) continue;
        const int32_t w = where[i];
        uint32_t u = ~0u;
        if (w >= 0 && uint32_t(w) < set.nt) u = set.nm + uint32_t(w);
        if (w <= -2 && -2 - int64_t(w) < int64_t(set.nm)) u = uint32_t(-2 - int64_t(w));
        const uint64_t so = val_off[i];
        if (u == ~0u || so > set.len[u] || uint64_t(len) > set.len[u] - so) {
            if (lane == 0) atomicAdd(err, 1u);
            continue;
        }
        merge_copy_bytes(out + offs[i], set.base[u] + so, uint32_t(len), lane);
    }
}

}  // namespace pbf
