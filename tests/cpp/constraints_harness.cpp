// test harness: the host half of the loci base constraints (biokanga_amd/csrc/host/loci_constraints.h).
//   constraints_harness load <file.csv> <entries.txt> <out.bin>
//     entries.txt: one sequence per line, "<EntryID> <length> <name>".  Success: "ok <constraints> <sequences>" on stdout and the
//     bk_constraint records, in file order, in out.bin; a refusal: the loader's message on stdout, exit status 1.
//   constraints_harness apply <in.bin> <out.bin>
//     in.bin: uint32 paired, uint32 n, uint32 m, m bytes (by chrom_id: the sequence is constrained), then n records of 64 bytes - a
//     bk_hit, its adjusted start and length, its left trim, uint32 "has a second segment", that bk_seg2, the read's offset and length, and
//     the status byte the device is taken to have answered (as uint32).  out.bin, per record: uint32 selected, int32 what
//     constraint_apply returned, the bk_constraint_req made (zeros if not selected), the bk_hit after the pass (mates marked when
//     paired); then uint64 records marked by their own answer, uint64 mates marked.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../biokanga_amd/csrc/host/loci_constraints.h"

struct In { bk_hit hit; uint32_t a_start, a_len, trim_left, has_seg2; bk_seg2 seg2; uint64_t read_ofs; uint32_t read_len, status; };
struct Out { uint32_t selected; int32_t rc; bk_constraint_req req; bk_hit hit; uint32_t pad; };
static_assert(sizeof(bk_hit) == 20 && sizeof(bk_seg2) == 12 && sizeof(bk_constraint) == 16 && sizeof(bk_constraint_seg) == 8 && sizeof(bk_constraint_req) == 32, "record layout");
static_assert(sizeof(In) == 64 && sizeof(Out) == 64, "harness layout");

static int load(const char *csv, const char *entries, const char *outp)
{
    std::vector<bk_entry_info> ents;
    FILE *f = fopen(entries, "r");
    if (!f) return 3;
    unsigned id, len;
    char name[128];
    while (fscanf(f, "%u %u %100s", &id, &len, name) == 3) {
        bk_entry_info e{};
        e.entry_id = id; e.seq_len = len;
        strncpy(e.name, name, sizeof(e.name) - 1);
        ents.push_back(e);
    }
    fclose(f);
    std::vector<bk_constraint> cons;
    size_t n_chroms = 0;
    std::string err;
    if (bk::load_loci_constraints(csv, ents, cons, n_chroms, err)) { printf("%s\n", err.c_str()); return 1; }
    FILE *g = fopen(outp, "wb");
    if (!g) return 4;
    if (!cons.empty() && fwrite(cons.data(), sizeof(bk_constraint), cons.size(), g) != cons.size()) return 4;
    fclose(g);
    printf("ok %zu %zu\n", cons.size(), n_chroms);
    return 0;
}

static int apply(const char *inp, const char *outp)
{
    FILE *f = fopen(inp, "rb");
    if (!f) return 3;
    uint32_t paired, n, m;
    if (fread(&paired, 4, 1, f) != 1 || fread(&n, 4, 1, f) != 1 || fread(&m, 4, 1, f) != 1) return 3;
    std::vector<uint8_t> constrained(m);
    if (m && fread(constrained.data(), 1, m, f) != m) return 3;
    std::vector<In> in(n);
    if (n && fread(in.data(), sizeof(In), n, f) != n) return 3;
    fclose(f);
    std::vector<Out> out(n);
    std::vector<bk_hit> hits(n);
    uint64_t n_marked = 0;
    for (uint32_t i = 0; i < n; i++) {
        Out &o = out[i];
        memset(&o, 0, sizeof(o));
        hits[i] = in[i].hit;
        o.selected = bk::constraint_selects(in[i].hit, constrained) ? 1 : 0;
        if (!o.selected) continue;
        o.req = bk::constraint_request(in[i].hit, in[i].a_start, in[i].a_len, in[i].trim_left, in[i].has_seg2 ? &in[i].seg2 : nullptr, in[i].read_ofs, in[i].read_len);
        o.rc = bk::constraint_apply((uint8_t)in[i].status, hits[i]);
        if (o.rc > 0) n_marked++;
    }
    const uint64_t n_mates = paired ? bk::constraint_mark_mates(hits) : 0;
    for (uint32_t i = 0; i < n; i++) out[i].hit = hits[i];
    FILE *g = fopen(outp, "wb");
    if (!g) return 4;
    if (n && fwrite(out.data(), sizeof(Out), n, g) != n) return 4;
    const uint64_t counts[2] = {n_marked, n_mates};
    if (fwrite(counts, 8, 2, g) != 2) return 4;
    fclose(g);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "load")) return load(argv[2], argv[3], argv[4]);
    if (argc == 4 && !strcmp(argv[1], "apply")) return apply(argv[2], argv[3]);
    return 2;
}
