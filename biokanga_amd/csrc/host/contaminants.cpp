// contaminants.cpp - see contaminants.h
#include "contaminants.h"

#include <strings.h>

#include "cli_common.h"
#include "fasta.h"

namespace bkcli {

namespace {

constexpr int kMinLen = 4, kMaxLen = 200, kMaxEntries = 1600;      // cMinContaminantLen, cMaxContaminantLen, cMaxNumContaminants
const char *kUseTxt[5] = {"", "5' PE1", "5' PE2", "3' PE1", "3' PE2"};

}  // namespace

int load_contaminants(const std::string &path, std::vector<ContamEntry> &out)
{
    out.clear();
    bk::SeqReader rd;
    std::string err;
    int rc = rd.open(path, &err);
    if (rc) { diag("LoadContaminantsFile: Unable to open '%s' %s", path.c_str(), err.c_str()); return rc; }
    diag("LoadContaminantsFile:- Processing %s..", path.c_str());
    std::string descr;
    std::vector<uint8_t> seq;
    int seq_id = 0;
    bool vector_kind = false;                      // (kept from the record in front when a record has no name: Contaminants.cpp:255,287)
    while ((rc = rd.next(descr, seq)) > 0) {
        seq_id++;
        bool use[9] = {false};
        // the name: the descriptor's first blank-delimited token; scanned from its end while the characters are '1'..'8', down to - not
        // including - its first character; a '@' / '&' the scan stops at, with something behind it, makes what follows the codes
        size_t b = 0;
        while (b < descr.size() && isspace((unsigned char)descr[b])) b++;
        size_t e = b;
        while (e < descr.size() && !isspace((unsigned char)descr[e])) e++;
        std::string name = descr.substr(b, e - b);
        if (name.empty()) {
            name = "ContamSeq." + std::to_string(seq_id);
            use[1] = use[2] = use[5] = use[6] = true;
        } else {
            size_t p = name.size() - 1;
            for (size_t idx = name.size(); idx > 1; idx--, p--)
                if (name[p] == '@' || name[p] == '&' || !(name[p] >= '1' && name[p] <= '8')) break;
            vector_kind = name[p] == '&';
            if ((name[p] == '@' || name[p] == '&') && p + 1 < name.size()) {
                for (size_t k = p + 1; k < name.size(); k++)
                    if (name[k] >= '1' && name[k] <= '8') use[name[k] - '0'] = true;
                name.resize(p);
            } else
                use[1] = use[2] = use[5] = use[6] = true;
        }
        if (vector_kind) {
            diag("LoadContaminantsFile: '%s' is a vector contaminant ('&' codes: whole-read containment), which this build does not process - only '@' adaptor overlaps are", descr.c_str());
            return -100;
        }
        if (name.empty()) { diag("AddFlankContam: Parameter errors"); return -100; }      // (a name that is nothing but codes, :647-652)
        const int len = (int)seq.size();
        if (len < kMinLen || len > kMaxLen) {
            diag("LoadContamiantsFile: Sequence for '%s' outside of accepted length range %d..%d", name.c_str(), kMinLen, kMaxLen);
            return -73;
        }
        for (uint8_t &c : seq) {
            c &= 7;
            if (c > 4) { diag("LoadContaminantsFile: Illegal base in %s sequence, only bases A,C,G,T,N accepted", name.c_str()); return -73; }
        }
        for (int pass = 0; pass < 2; pass++) {
            if (pass == 1) {
                if (!(use[5] || use[6] || use[7] || use[8])) break;
                std::reverse(seq.begin(), seq.end());
                for (uint8_t &c : seq) if (c < 4) c = 3 - c;
                name += "xRC";
            }
            for (int u = 1; u <= 4; u++) {
                if (!use[u + 4 * pass]) continue;
                if (out.size() >= (size_t)kMaxEntries) {
                    diag("AddFlankContam: Too many flank contaminants (max allowed %d) current contaminant is '%s'", kMaxEntries, name.c_str());
                    return -100;
                }
                // (CContaminants::AddFlankContam, :747-787: within a use neither a name nor a sequence may come twice)
                for (const ContamEntry &o : out) {
                    if (o.use != u) continue;
                    const bool same_seq = o.bases == seq, same_name = !strcasecmp(o.name.c_str(), name.c_str());
                    if (same_name) {
                        diag("AddFlankContam: Contaminant name '%s' of overlap type %s duplicated with %s sequences", name.c_str(), kUseTxt[u], same_seq ? "same" : "different");
                        return -71;
                    }
                    if (same_seq) {
                        diag("AddFlankContam: Contaminant names '%s' and '%s' of overlap type %s with duplicated sequence", name.c_str(), o.name.c_str(), kUseTxt[u]);
                        return -71;
                    }
                }
                ContamEntry ce;
                ce.name = name; ce.bases = seq; ce.use = u; ce.revcpl = pass == 1;
                out.push_back(std::move(ce));
            }
        }
    }
    if (rc < 0) { diag("LoadContaminantsFile: errors whilst parsing '%s'", path.c_str()); return rc; }
    return 0;
}

}  // namespace bkcli
