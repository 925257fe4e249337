// loci_constraints.h - loci base constraints of `biokanga align -5 <file>`: host side of CAligner::LoadLociConstraints
// (biokanga/Aligner.cpp:1267-1439) and IdentifyConstraintViolations (:2599-2646).  "Chr1A,100,100,CT": reads aligned over Chr1A:100 are
// only accepted if they carry C or T there; "Chr1A,100,107,R": only if they match the target there.  The walk of the records' bases
// against the constraints runs on the GPU (bk_constraints_check); here: the CSV file with the reference's refusals, word for word, the
// request of one record from its adjusted loci, and what an answer does to the record and to its mate.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <strings.h>
#include <vector>

#include "../../../include/biokanga_amd.h"

namespace bk {

constexpr uint8_t kNarLociConstrained = 19;        // eNARLociConstrained, "LC"

// ---- the CSV reader: what LoadLociConstraints uses of CCSVFile (libbiokanga/CSVFile.cpp:439-771) with its defaults - fields separated
// by ',', text quoted by '"' ("" inside stands for one), '#' starts a comment line; blanks and tabs around a field go, blank lines and
// leading blanks of a line are skipped.  The line number is the reader's: the line feeds it has consumed, which is the number of the
// line just parsed
struct CsvField { std::string value; bool quoted = false; };
struct CsvLine { std::vector<CsvField> fields; int line_num = 0; };

// one field from t[pos] on -> how it ended: 0 separator, 1 end of line, 2 end of text
inline int csv_parse_field(const std::string &t, size_t &pos, CsvField &f, int &line_num)
{
    int state = 0;
    f = CsvField{};
    auto trim = [&]() { while (!f.value.empty() && (f.value.back() == ' ' || f.value.back() == '\t')) f.value.pop_back(); };
    while (pos < t.size()) {
        const char ch = t[pos++];
        switch (state) {
        case 0:                                    // not inside the field yet
            if (ch == ' ' || ch == '\t') continue;
            if (ch == '"') { f.quoted = true; state = 2; continue; }
            if (ch == '\r' || ch == '\n') { line_num += ch == '\n'; return 1; }
            if (ch == ',') return 0;
            f.value.push_back(ch);
            state = 1;
            continue;
        case 1:                                    // a plain field
            if (ch == ',' || ch == '\r' || ch == '\n') { trim(); line_num += ch == '\n'; return ch == ',' ? 0 : 1; }
            f.value.push_back(ch);
            continue;
        case 2:                                    // a quoted one
            if (ch == '"') {
                if (pos < t.size() && t[pos] == '"') pos++;
                else { state = 3; continue; }
            }
            f.value.push_back(ch);
            continue;
        default:                                   // behind the closing quote: up to the separator
            if (ch == ',') return 0;
            if (ch == '\r' || ch == '\n') { line_num += ch == '\n'; return 1; }
            continue;
        }
    }
    if (state == 1) trim();
    return 2;
}

inline std::vector<CsvLine> csv_lines(std::string t)
{
    constexpr size_t kMaxFields = 100, kMaxFieldLen = 200;      // cCSVDfltFields, cCSVDfltFieldLen
    t = t.substr(0, t.find('\0'));
    std::vector<CsvLine> out;
    size_t pos = 0;
    int line_num = 0;
    bool in_comment = false;
    while (pos < t.size()) {
        const char ch = t[pos];
        if ((unsigned char)ch < ' ' && ch != '\t' && ch != '\n' && ch != '\r') break;
        if (ch == '\r' || ch == '\n') {
            pos++;
            if (ch == '\r' && pos < t.size() && t[pos] == '\n') { line_num++; pos++; }
            else if (ch == '\n') line_num++;
            in_comment = false;
            continue;
        }
        if (in_comment || ch == ' ' || ch == '\t') { pos++; continue; }
        if (ch == '#') { in_comment = true; pos++; continue; }
        CsvLine ln;
        while (ln.fields.size() < kMaxFields) {
            CsvField f;
            const int how = csv_parse_field(t, pos, f, line_num);
            if (f.value.size() >= kMaxFieldLen) f.value.resize(kMaxFieldLen - 1);
            ln.fields.push_back(f);
            if (how) break;
        }
        ln.line_num = line_num;
        out.push_back(ln);
    }
    return out;
}

// CCSVFile::IsLikelyHeaderLine: at most two empty fields, every other one quoted or not a number
inline bool csv_likely_header(const CsvLine &ln)
{
    int n_empty = 0;
    for (const CsvField &f : ln.fields) {
        if (f.quoted) continue;
        if (f.value.empty()) { if (++n_empty > 2) return false; continue; }
        char *end = nullptr;
        (void)strtod(f.value.c_str(), &end);
        if (end && *end == '\0') return false;
    }
    return true;
}

// The file's constraints in file order (bk_constraints_create sorts them), or -1 with the reference's message in `err`.  `ents`: the
// index's sequences; names compare without case, the first match counts (CSfxArrayV3::GetIdent)
inline int load_loci_constraints(const std::string &path, const std::vector<bk_entry_info> &ents, std::vector<bk_constraint> &out, size_t &n_chroms, std::string &err)
{
    auto fail = [&](const char *fmt, const char *name, int line) {
        char msg[1024];
        snprintf(msg, sizeof(msg), fmt, name, line, path.c_str());
        err = msg;
        return -1;
    };
    out.clear();
    n_chroms = 0;
    std::string text;
    FILE *f = fopen(path.c_str(), "rb");
    if (f) {
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), f)) > 0) text.append(buf, got);
        fclose(f);
    }
    const std::vector<CsvLine> lines = csv_lines(text);
    if (!f || text.size() < 5 || lines.empty()) { err = "Unable to open '" + path + "' for processing"; return -1; }
    std::vector<uint32_t> chroms;
    for (size_t n = 0; n < lines.size(); n++) {
        const CsvLine &ln = lines[n];
        if (ln.fields.size() < 4) {
            char msg[1024];
            snprintf(msg, sizeof(msg), "Expected at least 4 fields at line %d in '%s', GetCurFields() returned '%d'", ln.line_num, path.c_str(), (int)ln.fields.size());
            err = msg;
            return -1;
        }
        if (n == 0 && csv_likely_header(ln)) continue;
        const std::string name = ln.fields[0].value.substr(0, 80);
        const int start = atoi(ln.fields[1].value.c_str()), end = atoi(ln.fields[2].value.c_str());
        const bk_entry_info *ent = nullptr;
        for (const bk_entry_info &e : ents) if (!strcasecmp(name.c_str(), e.name)) { ent = &e; break; }
        if (!ent) return fail("Unable to find matching indexed identifier for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
        if (start < 0 || start > end) return fail("Start loci must be >= 0 and <= end loci for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
        if ((uint32_t)end >= ent->seq_len) return fail("End loci must be > targeted sequence length for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
        uint8_t mask = 0;
        for (const char ch : ln.fields[3].value) {
            switch (ch) {
            case 'a': case 'A': mask |= 0x01; break;
            case 'c': case 'C': mask |= 0x02; break;
            case 'g': case 'G': mask |= 0x04; break;
            case 't': case 'T': mask |= 0x08; break;
            case 'r': case 'R': mask |= BK_CONSTRAINT_R; break;
            case ' ': case '\t': break;
            default: return fail("Illegal base specifiers for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
            }
        }
        if (!mask) return fail("Illegal base specifiers for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
        bool seen = false;
        for (const uint32_t c : chroms) seen = seen || c == ent->entry_id;
        if (!seen) {
            if (chroms.size() == BK_MAX_CONSTRAINED_SEQS)
                return fail("Number of constrained chroms would be more than max (64) allowed for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
            chroms.push_back(ent->entry_id);
        }
        if (out.size() == BK_MAX_CONSTRAINTS)
            return fail("Number of constrained loci would be more than max (6400) allowed for '%s' at line %d in '%s'", name.c_str(), ln.line_num);
        out.push_back(bk_constraint{ent->entry_id, (uint32_t)start, (uint32_t)end, mask, {0, 0, 0}});
    }
    n_chroms = chroms.size();
    return 0;
}

// by chrom_id: whether the sequence carries a constraint (AcceptLociConstraints looks nowhere else, :2552-2557)
inline std::vector<uint8_t> constrained_chroms(const std::vector<bk_constraint> &cons)
{
    std::vector<uint8_t> on;
    for (const bk_constraint &c : cons) { if (c.chrom_id >= on.size()) on.resize((size_t)c.chrom_id + 1, 0); on[c.chrom_id] = 1; }
    return on;
}

// the records the pass walks: accepted, on a constrained sequence
inline bool constraint_selects(const bk_hit &h, const std::vector<uint8_t> &constrained)
{
    return h.nar == BK_NAR_ACCEPTED && h.chrom_id < constrained.size() && constrained[h.chrom_id];
}

// The request of one record.  Seg[0]: AdjStartLoci .. AdjEndLoci with the read indexed from ReadOfs (0) + TrimLeft - the READ's left
// trim on either strand, as the reference has it (:2570-2573); `seg2` (null: one segment): Seg[1], whose trims are 0, on Seg[0]'s
// sequence.  `a_start` / `a_len`: RecordSet::a_start / a_len of the record, `trim_left`: its TL
inline bk_constraint_req constraint_request(const bk_hit &h, uint32_t a_start, uint32_t a_len, uint32_t trim_left, const bk_seg2 *seg2, uint64_t read_ofs, uint32_t read_len)
{
    bk_constraint_req q{};
    q.read_ofs = read_ofs;
    q.chrom_id = h.chrom_id;
    q.read_len = (uint16_t)read_len;
    q.strand = h.strand;
    q.n_segs = seg2 ? 2 : 1;
    q.seg[0] = bk_constraint_seg{a_start, (uint16_t)a_len, (uint16_t)trim_left};
    if (seg2) q.seg[1] = bk_constraint_seg{seg2->match_loci, seg2->match_len, seg2->read_ofs};
    return q;
}

inline void constraint_mark(bk_hit &h)            // :2617-2619
{
    h.nar = kNarLociConstrained;
    h.num_hits = 0;
    h.low_hit_instances = 0;
}

// the answer of one request: 1 the record was marked, 0 it stays, -1 the device turned the request down (never accepted silently)
inline int constraint_apply(uint8_t status, bk_hit &h)
{
    if (status == BK_CONSTRAINT_VIOLATED) { constraint_mark(h); return 1; }
    return (status == BK_CONSTRAINT_UNTOUCHED || status == BK_CONSTRAINT_TOUCHED) ? 0 : -1;
}

// -U: the ends of a pair lie side by side (PE1, PE2); a marked end takes its mate with it (:2623-2639).  -> the mates marked
inline size_t constraint_mark_mates(std::vector<bk_hit> &hits)
{
    size_t n = 0;
    for (size_t i = 0; i + 1 < hits.size(); i += 2) {
        const bool a = hits[i].nar == kNarLociConstrained, b = hits[i + 1].nar == kNarLociConstrained;
        if (a != b) { constraint_mark(hits[a ? i + 1 : i]); n++; }
    }
    return n;
}

}  // namespace bk
