// contam_loader_harness - the read store `biokanga align -H` loads (host/read_loader.cpp) with a host stand-in for the device matcher: the
// rule as plain byte compares over the entries host/contaminants.cpp makes of the file.  The store is dumped as text - one line per read:
// name, bases as letters, a 4-bit score per base as a hex digit - once for the first load and, when asked, once more for a second load
// that replays the kept cuts without a matcher (the reload of biokanga_main.cpp).  stderr: "whole <files parsed whole so far>" and
// "matched <reads>" after every load; the loaders' log lines go to stdout.
//   contam_loader_harness se|pe <threads> <reload threads | 0> <trim5> <trim3> <minlen> <maxlen> <qmode> <nth> <contaminants.fa> <dump prefix> file [file ..]
//   (pe: mates alternate a1 b1 a2 b2)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../biokanga_amd/csrc/host/contaminants.h"
#include "../../biokanga_amd/csrc/host/read_loader.h"

namespace {

struct HostMatcher : bkcli::ContamMatcher {
    std::vector<bkcli::ContamEntry> entries;
    size_t matched = 0;
    int overlap(const uint8_t *read, int n, int use, int trim) const
    {
        if (n < 20 || n > 2000) return 0;
        const bool five = use <= 2;
        int longest = 0;
        for (const auto &e : entries) if (e.use == use && (int)e.bases.size() > longest) longest = (int)e.bases.size();
        for (int L = n < longest ? n : longest; L > trim; L--)
            for (const auto &e : entries) {
                const int el = (int)e.bases.size();
                if (e.use != use || el < L) continue;
                const uint8_t *r = five ? read : read + n - L, *c = five ? e.bases.data() + el - L : e.bases.data();
                int mism = 0;
                for (int i = 0; i < L && mism < 2; i++) { const uint8_t rb = r[i] & 7; mism += rb == 4 || (c[i] != 4 && c[i] != rb); }
                if (mism < 2) return L - trim;
            }
        return 0;
    }
    int match(const uint8_t *bases, const uint32_t *lens, size_t n, bool pe2, int trim5, int trim3, uint16_t *out) override
    {
        size_t at = 0;
        for (size_t i = 0; i < n; i++) {
            out[2 * i] = (uint16_t)overlap(bases + at, (int)lens[i], pe2 ? 2 : 1, trim5);
            out[2 * i + 1] = (uint16_t)overlap(bases + at, (int)lens[i], pe2 ? 4 : 3, trim3);
            at += lens[i];
        }
        matched += n;
        return 0;
    }
};

void dump(const bkcli::ReadStore &rs, const std::string &path)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) exit(3);
    for (size_t i = 0; i < rs.size(); i++) {
        fputs(rs.name(i), f);
        fputc('\t', f);
        const uint8_t *b = rs.bases.data() + rs.offs[i];
        for (uint32_t k = 0; k < rs.lens[i]; k++) fputc("ACGTN???"[b[k] & 7], f);
        fputc('\t', f);
        for (uint32_t k = 0; k < rs.lens[i]; k++) fputc("0123456789abcdef"[b[k] >> 4], f);
        fputc('\n', f);
    }
    fclose(f);
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 13) { fprintf(stderr, "usage\n"); return 2; }
    const bool pe = !strcmp(argv[1], "pe");
    const int nt = atoi(argv[2]), nt2 = atoi(argv[3]), t5 = atoi(argv[4]), t3 = atoi(argv[5]), mn = atoi(argv[6]), mx = atoi(argv[7]);
    bkcli::g_qual_mode = atoi(argv[8]);
    bkcli::g_sample_nth = atoi(argv[9]);
    HostMatcher hm;
    if (bkcli::load_contaminants(argv[10], hm.entries)) return 4;
    const std::string prefix = argv[11];
    std::vector<std::string> f1, f2;
    for (int i = 12; i < argc; i++) (pe && ((i - 12) & 1) ? f2 : f1).push_back(argv[i]);
    bkcli::ContamTrimming ct;
    ct.matcher = &hm;
    ct.keep = nt2 > 0;
    for (int pass = 0; pass < (nt2 > 0 ? 2 : 1); pass++) {
        bkcli::ReadStore rs;
        if (pass == 1) { ct.matcher = nullptr; ct.replay_at = 0; hm.matched = 0; }
        const int threads = pass ? nt2 : nt;
        const int rc = pe ? bkcli::load_reads_pe(f1, f2, t5, t3, mn, mx, threads, rs, &ct) : bkcli::load_reads(f1, t5, t3, mn, mx, threads, rs, &ct);
        fprintf(stderr, "whole %d\nmatched %zu\n", bkcli::g_whole_file_loads, hm.matched);
        if (rc) { printf("rc %d\n", rc); return 0; }
        if (pass == 1 && ct.replay_at != ct.trims.size()) { printf("replay left %zu of %zu cuts\n", ct.trims.size() - ct.replay_at, ct.trims.size()); return 0; }
        dump(rs, prefix + (pass ? ".reload" : ".load"));
    }
    return 0;
}
