// pgx_slots_device.h -- where the find_mems kernels put the MEMs of a read and where the compaction finds them
// (pgx_fm_kernels.hip, pgx_pairs_kernels.hip, pgx_scan_kernels.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgx_device.h"

// MEM slots of one chunk of reads: the first PGX_FAST_SLOTS MEMs of a read live in a dense array at the start of the slot buffer, slot-major (the
// k-th MEM of read r of the chunk: entry k * chunk_reads + r) -- a read has 1.9 MEMs on average, so the compaction reads the 0.6 GB that exist of
// that 1.28 GB array, coalesced over neighbouring reads (read-major, entries 4 r .. 4 r + 3, it read every line: 0.53 -> 0.41 ms at chr22 scale) --,
// further ones in the arena or at the read's worst-case offset (slot_off) behind that array
#define PGX_FAST_SLOTS 4u
__device__ __forceinline__ uint64_t pgx_slot_index(uint64_t read_in_chunk, uint64_t chunk_reads, uint64_t slot, uint32_t nm) {
    return nm < PGX_FAST_SLOTS ? (uint64_t)nm * chunk_reads + read_in_chunk : chunk_reads * PGX_FAST_SLOTS + slot + nm;
}
// Where the fifth and later MEMs of a read go (`slot` of pgx_slot_index).  Worst-case layout (ovf_cap == 0): the read's offset in the scan of
// min(len, len - min_len + 1), 131 slots per 150-bp read -- 42 GB for 10 M reads that write 0.6 GB.  ARENA (round 3): a read reserves its extent when it
// emits its fifth MEM (2 % of the reads do) -- as many slots as it has start positions left, which bounds what it can still emit -- with one atomic,
// and records it in ovf_base[rid] for its later MEMs, the kernels that continue the read, and the compaction.  The arena is PGX_ARENA_SUBS sub-arenas,
// one per residue of the read number, each with a counter on a cache line of its own (ctr + PGX_CTR_ARENA0 + 16 sub): one counter for everybody
// serialised 48 k atomics into 0.7 ms on the x fixture (a 0.6 ms kernel).  A sub-arena that proves too small raises PGX_CTR_OVF_ABORT (the writes
// then land at its start, in bounds) and the host repeats the chunk in the worst-case layout.
__device__ __forceinline__ uint64_t pgx_slot_extent(const uint64_t *__restrict__ slot_off, uint64_t slot_base, uint32_t *__restrict__ ovf_base, uint64_t ovf_cap,
                                                    unsigned long long *__restrict__ ctr, uint64_t rid, uint32_t nm, int32_t len, int32_t x, uint64_t min_len) {
    if (!ovf_cap) return slot_off[rid] - slot_base;
    if (nm == PGX_FAST_SLOTS) {
        const int64_t ml = min_len ? (int64_t)min_len : 1;
        const int64_t left = (int64_t)len - ml - (int64_t)x + 1; // start positions from x on (x itself has just produced a MEM)
        const unsigned long long ext = left > 0 ? (unsigned long long)left : 1ull;
        // (by read id, not by workgroup: what a sub-arena is asked for then does not depend on which workgroup took which reads, so a run sized from
        //  the one before fits -- reads that need many slots come in clusters, e.g. the reads cut from an N run, and landed in a few sub-arenas)
        const uint32_t sub = (uint32_t)rid & (PGX_ARENA_SUBS - 1u);
        const uint64_t sub_cap = ovf_cap / PGX_ARENA_SUBS;
        unsigned long long at = atomicAdd(ctr + PGX_CTR_ARENA0 + 16u * sub, ext);
        if (at + ext > sub_cap) { ctr[PGX_CTR_OVF_ABORT] = 1ull; at = 0ull; }
        at += (unsigned long long)sub * sub_cap;
        ovf_base[rid] = (uint32_t)at;
        return at - PGX_FAST_SLOTS; // (pgx_slot_index adds nm)
    }
    return (uint64_t)ovf_base[rid] - PGX_FAST_SLOTS;
}
