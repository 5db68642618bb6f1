// Device planner of the SSTable write path, gfx950: DataBlockBuilder's greedy blocks
// (src/blocks.py:78-95, sstable.py:224-244) and compaction's output split (LsmStorage._compact,
// src/lsm_storage.py:233-251) over a record run whose offsets arrays are in device memory, entry
// for entry what pbf_plan_blocks / pbf_plan_compaction return, and the blocks' first and last keys
// for the meta blocks.
//
// The prefix sum of the encoded record sizes needs no scan: P[i] = ko[i] + vo[i] + 8 i.
//   k_plan_next    one lane per record s: nxt[s] = the largest e with P[e] - P[s] <= block_size, a
//                  binary search in [s, s + 8192] (a record is >= 8 bytes and a block <= 65536);
//                  e == n (no record arrives to finish the block) is stored as kPlanOpen, and
//                  e == s (the record alone exceeds block_size) counts in *oversize.
//   k_plan_chunks  one workgroup per chunk of kPlanChunk records: every record's exit from the chunk
//                  along nxt and the hops to it, by pointer jumping in LDS (<= 13 rounds).  The
//                  exit is the first record of the orbit at or past the chunk's end, or the start
//                  of the run's open block when that lies inside the chunk (then exit < chunk end).
//   k_plan_walk    one lane: chunk by chunk from record 0, one dependent load per chunk (a block
//                  holds <= 8192 = kPlanChunk records, so an exit lies in the next chunk).  The
//                  builder position follows from the exit, the hops and P: a run of h blocks from
//                  s to e adds P[e] - P[s] + 2 (e - s) + 2 h.  Only where that crosses
//                  max_sstable_size does it walk block by block, to the split, inside that chunk.
//                  It writes the table starts, the blocks it walked itself and one segment per
//                  chunk crossed whole.
//   k_plan_expand  one workgroup per segment: the chunk's nxt in LDS, one lane follows the
//                  segment's hops there, all lanes write block_first / block_out.
// Dependent global loads in sequence: ceil(n / 8192) + per output table the blocks of one chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pbf {

constexpr uint32_t kPlanChunk = 8192;       // records per chunk = the most a block holds
constexpr uint32_t kPlanThreads = 1024;
constexpr uint32_t kPlanPer = kPlanChunk / kPlanThreads;
constexpr uint32_t kPlanOpen = 0xFFFFFFFFu;  // nxt: the block that starts here is never finished

struct PlanSeg {       // a run of `hops` blocks from record `start`, all inside one chunk
    uint64_t block;    // index of its first block
    uint64_t out;      // byte offset of its first block
    uint32_t start, hops;
};

struct PlanResult {
    unsigned long long nblocks, ntables, written, out_bytes;
    unsigned int oversize;  // records larger than block_size (k_plan_next)
    unsigned int overflow;  // the plan needs more entries than the caller provides
};

__device__ __forceinline__ uint64_t plan_P(const uint64_t* __restrict__ ko, const uint64_t* __restrict__ vo, uint64_t i) {
    return ko[i] + vo[i] + 8 * i;
}

__global__ void __launch_bounds__(256) k_plan_next(const uint64_t* __restrict__ ko, const uint64_t* __restrict__ vo,
                                                   uint64_t n, uint64_t block_size, uint32_t* __restrict__ nxt,
                                                   PlanResult* __restrict__ res) {
    const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
    for (uint64_t s = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; s < n; s += stride) {
        const uint64_t limit = plan_P(ko, vo, s) + block_size;
        // the largest e in [s, hi] with P[e] <= limit (P[s] <= limit always holds)
        uint64_t lo = s, hi = s + kPlanChunk < n ? s + kPlanChunk : n;
        for (int it = 0; it < 14 && lo < hi; ++it) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (plan_P(ko, vo, mid) <= limit) lo = mid;
            else hi = mid - 1;
        }
        if (lo == s) atomicAdd(&res->oversize, 1u);
        nxt[s] = lo >= n ? kPlanOpen : uint32_t(lo);
    }
}

// exh[s] = exit | hops << 32 (see the head of the file).
__global__ void __launch_bounds__(kPlanThreads) k_plan_chunks(const uint32_t* __restrict__ nxt, uint64_t n,
                                                              uint64_t* __restrict__ exh) {
    __shared__ uint32_t s_val[kPlanChunk];   // done: the exit; else the next record of the orbit
    __shared__ uint16_t s_hops[kPlanChunk];  // hops to s_val; bit 15 = done
    const uint64_t base = uint64_t(blockIdx.x) * kPlanChunk;
    const uint64_t end = base + kPlanChunk < n ? base + kPlanChunk : n;
    const uint32_t cnt = uint32_t(end - base), tid = threadIdx.x;
    for (uint32_t i = tid; i < cnt; i += kPlanThreads) {
        const uint32_t e = nxt[base + i];
        if (e == kPlanOpen) {  // the open block starts here
            s_val[i] = uint32_t(base + i);
            s_hops[i] = 0x8000u;
        } else if (e >= end || e <= base + i) {  // (e <= s cannot be: such a run was refused)
            s_val[i] = e;
            s_hops[i] = 0x8001u;
        } else {
            s_val[i] = e;
            s_hops[i] = 1u;
        }
    }
    __syncthreads();
    for (int round = 0; round < 14; ++round) {
        uint32_t v[kPlanPer];
        uint16_t h[kPlanPer];
        int open = 0;
#pragma unroll
        for (uint32_t j = 0; j < kPlanPer; ++j) {
            const uint32_t i = tid + j * kPlanThreads;
            v[j] = 0;
            h[j] = 0;
            if (i < cnt && !(s_hops[i] & 0x8000u)) {
                const uint32_t t = s_val[i] - uint32_t(base);  // inside the chunk, past i
                const uint16_t ht = s_hops[t];
                v[j] = s_val[t];
                h[j] = uint16_t((s_hops[i] + (ht & 0x7FFFu)) | (ht & 0x8000u));
                open |= !(ht & 0x8000u);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t j = 0; j < kPlanPer; ++j) {
            const uint32_t i = tid + j * kPlanThreads;
            if (h[j]) {
                s_val[i] = v[j];
                s_hops[i] = h[j];
            }
        }
        if (!__syncthreads_or(open)) break;
    }
    for (uint32_t i = tid; i < cnt; i += kPlanThreads)
        exh[base + i] = uint64_t(s_val[i]) | (uint64_t(s_hops[i] & 0x7FFFu) << 32);
}

// max_sstable_size == 0: blocks mode (one table, every record written).  block_first / block_out
// hold cap entries each, table_blocks too; res->overflow is set and nothing further is written
// once an entry would not fit.  segs: one per chunk, zeroed by the caller.
__global__ void k_plan_walk(const uint64_t* __restrict__ ko, const uint64_t* __restrict__ vo, uint64_t n,
                            uint64_t max_sstable_size, const uint32_t* __restrict__ nxt,
                            const uint64_t* __restrict__ exh, uint64_t* __restrict__ block_first,
                            uint64_t* __restrict__ block_out, uint64_t* __restrict__ table_blocks, uint64_t cap,
                            PlanSeg* __restrict__ segs, PlanResult* __restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const bool compaction = max_sstable_size != 0;
    uint64_t nb = 0, nt = 0, out = 0, s = 0, pos = 0;
    uint64_t nb_t0 = 0, out_t0 = 0, s_t0 = 0;  // where the open table starts
    uint64_t written = n;
    bool overflow = cap < 2;
    if (!overflow) table_blocks[0] = 0;
    // every pass either crosses a chunk or closes a table that holds >= 2 records
    for (uint64_t guard = 0; !overflow && s < n && guard <= 2 * n + 2; ++guard) {
        const uint64_t cend = (s / kPlanChunk + 1) * kPlanChunk < n ? (s / kPlanChunk + 1) * kPlanChunk : n;
        const uint64_t eh = exh[s];
        const uint64_t e = eh & 0xFFFFFFFFull, h = eh >> 32;
        const uint64_t Ps = plan_P(ko, vo, s);
        const uint64_t span = plan_P(ko, vo, e) - Ps + 2 * (e - s) + 2 * h;
        if (!compaction || pos + span < max_sstable_size) {  // no split on the way to e
            // entries: the h blocks, the open block where it is kept, and the closing one
            const bool keep_open = e < cend && (!compaction || pos + span > 0);
            if (nb + h + (keep_open ? 2 : 1) > cap) {
                overflow = true;
                break;
            }
            if (h) segs[s / kPlanChunk] = PlanSeg{nb, out, uint32_t(s), uint32_t(h)};
            nb += h;
            out += span;
            pos += span;
            s = e;
            if (e < cend) {  // the open block [e, n): no record arrives to finish it
                if (!compaction || pos > 0) {
                    block_first[nb] = e;
                    block_out[nb] = out;
                    out += plan_P(ko, vo, n) - plan_P(ko, vo, e) + 2 * (n - e) + 2;
                    ++nb;
                    if (nt + 2 > cap) {
                        overflow = true;
                        break;
                    }
                    table_blocks[++nt] = nb;
                } else {  // the last builder's position is 0: its records are not written
                    nb = nb_t0;
                    out = out_t0;
                    written = s_t0;
                }
                s = n;
            }
            continue;
        }
        // the split lies on the way to e: block by block (at most the blocks of this chunk)
        uint64_t Pcur = Ps;
        for (uint32_t j = 0; j <= kPlanChunk; ++j) {
            const uint64_t e1 = nxt[s];  // (a finished block: the crossing comes before the open one)
            if (e1 >= n || e1 <= s || nb + 3 > cap) {
                overflow = true;
                break;
            }
            const uint64_t Pe = plan_P(ko, vo, e1);
            block_first[nb] = s;
            block_out[nb] = out;
            ++nb;
            const uint64_t bsz = Pe - Pcur + 2 * (e1 - s) + 2;
            out += bsz;
            pos += bsz;
            s = e1;
            Pcur = Pe;
            if (pos >= max_sstable_size) break;
        }
        if (overflow || nt + 2 > cap) {
            overflow = true;
            break;
        }
        // build(): record s alone is the table's last block
        block_first[nb] = s;
        block_out[nb] = out;
        ++nb;
        out += plan_P(ko, vo, s + 1) - Pcur + 4;
        table_blocks[++nt] = nb;
        ++s;
        pos = 0;
        nb_t0 = nb;
        out_t0 = out;
        s_t0 = s;
    }
    if (!overflow) {
        block_first[nb] = written;
        block_out[nb] = out;
    }
    res->nblocks = nb;
    res->ntables = nt;
    res->written = written;
    res->out_bytes = out;
    res->overflow = overflow ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_plan_expand(const uint64_t* __restrict__ ko, const uint64_t* __restrict__ vo,
                                                     uint64_t n, const uint32_t* __restrict__ nxt,
                                                     const PlanSeg* __restrict__ segs,
                                                     uint64_t* __restrict__ block_first,
                                                     uint64_t* __restrict__ block_out) {
    __shared__ uint32_t s_nxt[kPlanChunk];
    __shared__ uint16_t s_list[kPlanChunk];  // the segment's block starts, relative to the chunk
    const PlanSeg sg = segs[blockIdx.x];
    if (sg.hops == 0) return;
    const uint64_t base = uint64_t(blockIdx.x) * kPlanChunk;
    const uint64_t end = base + kPlanChunk < n ? base + kPlanChunk : n;
    const uint32_t cnt = uint32_t(end - base), tid = threadIdx.x;
    for (uint32_t i = tid; i < cnt; i += blockDim.x) s_nxt[i] = nxt[base + i];
    __syncthreads();
    const uint32_t hops = sg.hops < kPlanChunk ? sg.hops : kPlanChunk;
    if (tid == 0) {
        uint32_t i = sg.start - uint32_t(base);
        for (uint32_t j = 0; j < hops; ++j) {
            if (i >= cnt) i = sg.start - uint32_t(base);  // (cannot be: the segment's blocks start inside the chunk)
            s_list[j] = uint16_t(i);
            i = s_nxt[i] - uint32_t(base);
        }
    }
    __syncthreads();
    const uint64_t P0 = plan_P(ko, vo, sg.start);
    for (uint32_t j = tid; j < hops; j += blockDim.x) {
        const uint64_t x = base + s_list[j];
        block_first[sg.block + j] = x;
        block_out[sg.block + j] = sg.out + (plan_P(ko, vo, x) - P0) + 2 * (x - sg.start) + 2 * uint64_t(j);
    }
}

// sizes[2 b] / sizes[2 b + 1] = the bytes of block b's first / last key.
__global__ void __launch_bounds__(256) k_plan_bound_sizes(const uint64_t* __restrict__ ko,
                                                          const uint64_t* __restrict__ block_first, uint64_t nblocks,
                                                          uint32_t* __restrict__ sizes) {
    const uint64_t b = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t r0 = block_first[b], r1 = block_first[b + 1];
    sizes[2 * b] = uint32_t(ko[r0 + 1] - ko[r0]);
    sizes[2 * b + 1] = r1 > r0 ? uint32_t(ko[r1] - ko[r1 - 1]) : 0u;
}

// bounds[offs[2 b], offs[2 b + 1]) = block b's first key, [offs[2 b + 1], offs[2 b + 2]) its last:
// one wave per block.
__global__ void __launch_bounds__(256) k_plan_bounds_gather(const uint8_t* __restrict__ keys,
                                                            const uint64_t* __restrict__ ko,
                                                            const uint64_t* __restrict__ block_first, uint64_t nblocks,
                                                            const uint64_t* __restrict__ offs,
                                                            uint8_t* __restrict__ bounds) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t b = (uint64_t(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    if (b >= nblocks) return;
    const uint64_t r0 = block_first[b], r1 = block_first[b + 1];
    if (r1 <= r0) return;
    const uint64_t src[2] = {ko[r0], ko[r1 - 1]};
    for (int w = 0; w < 2; ++w) {
        const uint64_t o0 = offs[2 * b + w], len = offs[2 * b + w + 1] - o0;
        for (uint64_t i = lane; i < len; i += 64) bounds[o0 + i] = keys[src[w] + i];
    }
}

}  // namespace pbf
