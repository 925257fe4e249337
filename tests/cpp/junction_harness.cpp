// test harness: the host half of `align --junctions` / `--splice-strand` (biokanga_amd/csrc/host/junctions.h) on a built RecordSet.
//   junction_harness <in.bin> <out.bin>
//     in.bin: uint32 0, uint32 n, then n records of 40 bytes - a bk_hit, its end trims in read orientation (uint16 left, right), the
//     bk_seg2 of its read (flags & 5: a second segment; flags & 8: a chimeric placement, whose trims are the two above), uint32 0.
//     out.bin: uint32 requests, then per request the bk_junction_req made and uint32 its record; then n bytes - RecordSet::xs after
//     junction_apply_strands with the canned answers "request t gets '+', '-', 0 for t % 3 = 0, 1, 2" - and int64 the records that carry
//     a strand; then the table text junction_line makes of every request taken as a junction of t + 1 reads, motif t % 7.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../biokanga_amd/csrc/host/junctions.h"

struct In { bk_hit hit; uint16_t tl, tr; bk_seg2 seg2; uint32_t pad; };
struct Req { bk_junction_req req; uint32_t rec; };
static_assert(sizeof(bk_hit) == 20 && sizeof(bk_seg2) == 12 && sizeof(bk_junction_req) == 16 && sizeof(bk_junction) == 20, "record layout");
static_assert(sizeof(In) == 40 && sizeof(Req) == 20, "harness layout");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t unused, n;
    if (fread(&unused, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 3;
    std::vector<In> in(n);
    if (n && fread(in.data(), sizeof(In), n, f) != n) return 3;
    fclose(f);
    std::vector<bk_hit> hits(n);
    std::vector<bk_seg2> seg2(n);
    bk::RecordSet rec{hits, seg2, {}, {}, {}};
    bool any_trim = false;
    for (uint32_t i = 0; i < n; i++) { hits[i] = in[i].hit; seg2[i] = in[i].seg2; any_trim = any_trim || in[i].tl || in[i].tr; }
    if (any_trim) {
        rec.ensure_trims();
        for (uint32_t i = 0; i < n; i++) { rec.trims.left[i] = in[i].tl; rec.trims.right[i] = in[i].tr; }
    }
    std::vector<bk_junction_req> reqs;
    std::vector<uint32_t> rec_of;
    bkcli::junction_requests(rec, reqs, rec_of);
    std::vector<uint8_t> strands(reqs.size());
    for (size_t t = 0; t < reqs.size(); t++) strands[t] = t % 3 == 0 ? '+' : (t % 3 == 1 ? '-' : 0);
    const int64_t n_tagged = bkcli::junction_apply_strands(rec, rec_of, strands);
    std::string text;
    for (size_t t = 0; t < reqs.size(); t++) {
        const uint8_t motif = (uint8_t)(t % 7);
        const bk_junction j{reqs[t].chrom_id, reqs[t].start, reqs[t].end, (uint32_t)t + 1, reqs[t].overhang, motif, (uint8_t)(motif == 0 ? '.' : (motif & 1 ? '+' : '-'))};
        const char name[3] = {'d', (char)('A' + (j.chrom_id - 1) % 26), 0};
        bkcli::junction_line(j, name, text);
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 4;
    const uint32_t nt = (uint32_t)reqs.size();
    if (fwrite(&nt, 4, 1, g) != 1) return 4;
    for (uint32_t t = 0; t < nt; t++) {
        const Req x{reqs[t], rec_of[t]};
        if (fwrite(&x, sizeof(x), 1, g) != 1) return 4;
    }
    if (n && fwrite(rec.xs.data(), 1, n, g) != n) return 4;
    if (fwrite(&n_tagged, 8, 1, g) != 1) return 4;
    if (!text.empty() && fwrite(text.data(), 1, text.size(), g) != text.size()) return 4;
    fclose(g);
    return 0;
}
