// test harness: the host half of `align --mark-duplicates` (biokanga_amd/csrc/host/duplicates.h) on a built RecordSet.
//   dup_harness <in.bin> <out.bin>
//     in.bin: uint32 paired, uint32 n, then n records of 40 bytes - a bk_hit, its end trims in read orientation (uint16 left, right), the
//     bk_seg2 of its read (flags & 5: a second segment; flags & 8: a chimeric placement, whose trims are the two above), uint32 0.
//     out.bin: uint32 templates, then per template the bk_dup_req made and uint32 its first record; then n bytes - RecordSet::dup after
//     duplicate_apply with the canned answers "template t is a duplicate iff t % 3 == 1" - and int64 the records that marked.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../biokanga_amd/csrc/host/duplicates.h"

struct In { bk_hit hit; uint16_t tl, tr; bk_seg2 seg2; uint32_t pad; };
struct Tmpl { bk_dup_req req; uint32_t first; };
static_assert(sizeof(bk_hit) == 20 && sizeof(bk_seg2) == 12 && sizeof(bk_dup_req) == 16, "record layout");
static_assert(sizeof(In) == 40 && sizeof(Tmpl) == 20, "harness layout");

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    uint32_t paired, n;
    if (fread(&paired, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1) return 3;
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
    std::vector<bk_dup_req> reqs;
    std::vector<uint32_t> first;
    bkcli::duplicate_templates(rec, paired != 0, reqs, first);
    std::vector<uint8_t> answers(reqs.size());
    for (size_t t = 0; t < reqs.size(); t++) answers[t] = t % 3 == 1 ? 1 : 0;
    const int64_t n_marked = bkcli::duplicate_apply(rec, reqs, first, answers);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 4;
    const uint32_t nt = (uint32_t)reqs.size();
    if (fwrite(&nt, 4, 1, g) != 1) return 4;
    for (uint32_t t = 0; t < nt; t++) {
        const Tmpl x{reqs[t], first[t]};
        if (fwrite(&x, sizeof(x), 1, g) != 1) return 4;
    }
    if (n && fwrite(rec.dup.data(), 1, n, g) != n) return 4;
    if (fwrite(&n_marked, 8, 1, g) != 1) return 4;
    fclose(g);
    return 0;
}
