// bk_stage.h - what each request pass over finished alignments keeps with its context between calls: its staging buffers, made by the
// pass's first call and grown when a call needs more, and its chunk knobs (bk_ctx_tune).  One struct per pass, a member of bk_ctx each;
// bytes() is what the staging holds now - the pass's read-only knob ("primer_buf_bytes" ..) - and sums the struct's own members.
// (The loci constraints keep theirs with the set, bk_constraints; only their chunk knob is the context's.)
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/biokanga_amd.h"
#include "bk_devbuf.h"

namespace bk {
// bk_snp_sites: the site list of the last call, on the device and sorted on the host
struct SnpStage {
    DevBuf<bk_snp_site> d_sites;
    std::vector<bk_snp_site> sites;
};
// bk_site_octamers: one chunk of requests and its results
struct SiteStage {
    uint64_t chunk = 8u << 20;            // requests staged at a time ("site_chunk")
    DevBuf<bk_site_req> reqs;
    DevBuf<bk_site_res> res;
    size_t bytes() const { return reqs.bytes() + res.bytes(); }
};
// bk_primer_correct: one chunk of requests and its results
struct PrimerStage {
    uint64_t chunk = 8u << 20;            // requests staged at a time ("primer_chunk")
    DevBuf<bk_primer_req> reqs;
    DevBuf<bk_primer_res> res;
    size_t bytes() const { return reqs.bytes() + res.bytes(); }
};
// bk_samtags: one chunk of requests, its reads' bases and where each starts in them, the answers
struct SamtagStage {
    uint64_t chunk = 2u << 20;            // requests staged at a time ("samtag_chunk")
    DevBuf<bk_samtag_req> reqs;
    DevBuf<uint8_t> bases, tmp;           // (tmp: the offset scan's temporary)
    DevBuf<uint64_t> gofs;
    DevBuf<uint16_t> nm;
    DevBuf<unsigned long long> len, at;
    DevBuf<char> text;
    size_t bytes() const { return reqs.bytes() + bases.bytes() + tmp.bytes() + gofs.bytes() + nm.bytes() + len.bytes() + at.bytes() + text.bytes(); }
};
// bk_coverage_*: one chunk of requests and its flag bytes, a slice's depth and tile tables, one chunk of runs and its text
struct CovStage {
    uint64_t req_chunk = 8u << 20;        // requests staged at a time ("coverage_req_chunk")
    uint64_t slice_bases = 0;             // target bases per slice ("coverage_slice_bases"; 0: the first call derives it from the free memory)
    uint64_t run_chunk = 1u << 20;        // runs per sink call ("coverage_run_chunk")
    DevBuf<bk_cov_req> reqs;
    DevBuf<uint8_t> flags, tmp;           // (tmp: the scans' temporary)
    DevBuf<int32_t> depth;                // a slice's deltas, then its depth: one per base, one more behind every sequence
    DevBuf<uint64_t> ent_ofs;             // n_ent + 1: where every sequence starts when each is followed by one position that stays 0
    DevBuf<char> names;                   // n_ent x 81 bytes, by entry index
    DevBuf<uint32_t> tile_n[2];           // run starts / run ends in every tile of a slice ..
    DevBuf<unsigned long long> tile_at[2];        // .. and their exclusive sums (+ 1: the slice's runs)
    DevBuf<unsigned long long> tot;       // covered positions, sum of depth, largest depth
    DevBuf<bk_cov_run> runs;              // one chunk of runs
    DevBuf<unsigned long long> len, at;   // the formatter: the chunk's line lengths and where each line starts
    DevBuf<char> text;
    PinBuf<uint8_t> host;                 // page-locked: a chunk of runs, or a piece of text, on its way to the sink (16 bytes per run of a chunk)
    size_t bytes() const
    {
        return reqs.bytes() + flags.bytes() + tmp.bytes() + depth.bytes() + ent_ofs.bytes() + names.bytes() + tile_n[0].bytes() + tile_n[1].bytes() + tile_at[0].bytes() +
               tile_at[1].bytes() + tot.bytes() + runs.bytes() + len.bytes() + at.bytes() + text.bytes() + host.bytes();
    }
};
// bk_mark_duplicates: all requests of a call and their answers, the grouping table, the totals
struct alignas(16) DupSlot {
    unsigned long long best;              // score << 32 | (0xFFFFFFFF - request index) of the group's keeper so far (cleared to 0)
    uint32_t owner;                       // the request that claimed the slot: its key is the slot's (cleared to 0xFFFFFFFF)
    uint32_t count;                       // templates of the group
};
struct DupStage {
    uint64_t table_slots = 0;             // "dup_table_slots": 0 - derived per call - or a power of two >= the call's requests
    DevBuf<bk_dup_req> reqs;
    DevBuf<uint8_t> out;
    DevBuf<DupSlot> table;
    DevBuf<unsigned long long> tot;       // groups, largest group, flagged, the error word
    size_t bytes() const { return reqs.bytes() + out.bytes() + table.bytes() + tot.bytes(); }
};
// bk_junctions: all requests of a call and their strands, the grouping table, the emitted junctions with their sort keys, the totals
struct alignas(16) JctSlot {
    uint32_t owner;                       // the request that claimed the slot: its key is the slot's (cleared to 0xFFFFFFFF)
    uint32_t count;                       // requests of the junction
    uint32_t overhang;                    // the largest overhang among them
    uint32_t motif;                       // motif | strand << 8, written by the owner once the grouping is done
};
struct JunctionStage {
    uint64_t table_slots = 0;             // "junction_table_slots": 0 - derived per call - or a power of two >= the call's requests
    DevBuf<bk_junction_req> reqs;
    DevBuf<uint8_t> strand, tmp;          // (tmp: the sorts' temporary)
    DevBuf<JctSlot> table;
    DevBuf<unsigned long long> tot;       // junctions, largest count, flagged, the error word, the emit counter, junctions by motif
    DevBuf<bk_junction> jct, sorted;      // as emitted; in their final order
    DevBuf<uint32_t> key_end[2], place[3];        // first sort: `end` in and out; the places in, between the sorts, out
    DevBuf<unsigned long long> key_hi[3]; // entry index << 32 | start: as emitted; second sort in and out
    size_t bytes() const
    {
        return reqs.bytes() + strand.bytes() + tmp.bytes() + table.bytes() + tot.bytes() + jct.bytes() + sorted.bytes() + key_end[0].bytes() + key_end[1].bytes() +
               place[0].bytes() + place[1].bytes() + place[2].bytes() + key_hi[0].bytes() + key_hi[1].bytes() + key_hi[2].bytes();
    }
};
}  // namespace bk
