// contaminants.h - the contaminants file of `biokanga align -H` (CContaminants::LoadContaminantsFile, libbiokanga/Contaminants.cpp:205-427):
// a multi-FASTA of adaptor sequences whose names say which read ends they apply to.  Parsed into the (sequence, use) entries the
// matcher is made from (bk_contam_create); records with the '&' separator - vector contaminants, whole-read containment - are refused.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace bkcli {

struct ContamEntry {
    std::string name;                   // the record's name without its codes ("xRC" appended to a reverse complemented one)
    std::vector<uint8_t> bases;         // 0..3 a,c,g,t, 4 N
    int use = 0;                        // 1 5' of SE/PE1, 2 5' of PE2, 3 3' of SE/PE1, 4 3' of PE2
    bool revcpl = false;
};

// 0 and the entries in the reference's order, or a negative teBSFrsltCodes value after the message has been logged
int load_contaminants(const std::string &path, std::vector<ContamEntry> &out);

}  // namespace bkcli
