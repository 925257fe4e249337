// test harness: the line as written (bk::RecordSet::line of biokanga_amd/csrc/host/post_filters.h over biokanga_amd/csrc/bk_line.h) on a
// built RecordSet.  tests/test_host_line.py writes the records and checks the lines against its own statement of the rule.
//   line_host <in> <out>
// in:  "<records> <reads> <with_src> <with_trims> <with_seg2>", then per record "chrom_id match_loci match_len strand trim_left trim_right read",
//      then per read "read_len seg_loci seg_len seg_flags" (the tables a run does not have are not built: the columns are read and dropped)
// out: per record "pos m c5 c3 gop m2 gap gap_written", gop as a number
#include <cstdio>
#include <vector>

#include "../../biokanga_amd/csrc/host/post_filters.h"

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned long nrec = 0, nreads = 0;
    int with_src = 0, with_trims = 0, with_seg2 = 0;
    if (fscanf(f, "%lu %lu %d %d %d", &nrec, &nreads, &with_src, &with_trims, &with_seg2) != 5) return 2;
    std::vector<bk_hit> hits(nrec);
    std::vector<bk_seg2> seg2(with_seg2 ? nreads : 0);
    std::vector<uint32_t> read_len(nreads);
    bk::RecordSet recs{hits, seg2, {}, {}, {}};
    if (with_src) recs.src.resize(nrec);
    if (with_trims) recs.ensure_trims();
    for (size_t i = 0; i < nrec; i++) {
        unsigned chrom, loci, len, tl, tr, rd;
        char strand;
        if (fscanf(f, "%u %u %u %c %u %u %u", &chrom, &loci, &len, &strand, &tl, &tr, &rd) != 7) return 2;
        bk_hit h{};
        h.chrom_id = chrom; h.match_loci = loci; h.match_len = (uint16_t)len; h.strand = (uint8_t)strand; h.nar = BK_NAR_ACCEPTED;
        hits[i] = h;
        if (with_src) recs.src[i] = rd;
        if (with_trims) { recs.trims.left[i] = (uint16_t)tl; recs.trims.right[i] = (uint16_t)tr; }
    }
    for (size_t r = 0; r < nreads; r++) {
        unsigned rl, loci, len, flags;
        if (fscanf(f, "%u %u %u %u", &rl, &loci, &len, &flags) != 4) return 2;
        read_len[r] = rl;
        if (with_seg2) { bk_seg2 g{}; g.match_loci = loci; g.match_len = (uint16_t)len; g.flags = (uint8_t)flags; seg2[r] = g; }
    }
    fclose(f);
    FILE *o = fopen(argv[2], "w");
    if (!o) return 2;
    for (size_t i = 0; i < nrec; i++) {
        const bk::Line L = recs.line(i);
        fprintf(o, "%u %u %u %u %d %u %ld %ld\n", L.pos, L.m, L.c5, L.c3, (int)L.gop, L.m2, L.gap, L.gap_written(read_len[recs.RD(i)]));
    }
    return fclose(o) ? 2 : 0;
}
