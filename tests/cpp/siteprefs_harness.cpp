// test harness: the host half of the start-site octamer preferences (biokanga_amd/csrc/host/site_prefs.h) on a recorded stream of
// visited reads - 20-byte records: a bk_site_req and the bk_site_res the gather answered for it - writes the preference CSV and,
// one int32 per visited read, the score the BED / CSV writers would print for it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../biokanga_amd/csrc/host/site_prefs.h"

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<bk_site_req> reqs;
    std::vector<bk_site_res> res;
    unsigned char rec[20];
    static_assert(sizeof(bk_site_req) == 12 && sizeof(bk_site_res) == 8, "record layout");
    while (fread(rec, sizeof(rec), 1, f) == 1) {
        bk_site_req q;
        bk_site_res r;
        memcpy(&q, rec, 12);
        memcpy(&r, rec + 12, 8);
        reqs.push_back(q);
        res.push_back(r);
    }
    fclose(f);
    std::vector<uint32_t> rec_of(reqs.size());
    for (size_t i = 0; i < rec_of.size(); i++) rec_of[i] = (uint32_t)i;
    bk::SitePrefs sp;
    bk::site_prefs_pass(reqs.data(), res.data(), rec_of.data(), reqs.size(), reqs.size(), sp);
    bk::site_prefs_scale(sp);
    std::string csv;
    bk::site_prefs_csv(sp, csv);
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(csv.data(), 1, csv.size(), g) != csv.size()) return 4;
    fclose(g);
    std::vector<int32_t> scores(reqs.size());
    for (size_t i = 0; i < scores.size(); i++) scores[i] = sp.score(reqs[i].strand, i);
    FILE *h = fopen(argv[3], "wb");
    if (!h || fwrite(scores.data(), 4, scores.size(), h) != scores.size()) return 5;
    fclose(h);
    return 0;
}
