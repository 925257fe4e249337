// contam_harness - the entries `biokanga align -H` makes of a contaminants file (host/contaminants.cpp), one per line: use, r when
// reverse complemented else f, name, bases as letters; or "rc <code>" when the file is refused (the messages go to stdout as log lines).
#include <cstdio>
#include <string>
#include <vector>

#include "../../biokanga_amd/csrc/host/contaminants.h"

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: contam_harness <contaminants.fa>\n"); return 2; }
    std::vector<bkcli::ContamEntry> entries;
    const int rc = bkcli::load_contaminants(argv[1], entries);
    if (rc) { printf("rc %d\n", rc); return 0; }
    for (const bkcli::ContamEntry &e : entries) {
        std::string s;
        for (uint8_t b : e.bases) s += "ACGTN"[b];
        printf("entry %d %c %s %s\n", e.use, e.revcpl ? 'r' : 'f', e.name.c_str(), s.c_str());
    }
    return 0;
}
