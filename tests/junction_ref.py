"""Shared by the --junctions / --splice-strand tests: the rule of bk_junctions (include/biokanga_amd.h) in plain Python.

    A request is one spliced record: (chrom_id, start, end, overhang) of a line [c5 S] m M [c3 S] gap N m2 M at POS - start = POS - 1 + m,
    the first intron base, 0-based; end = start + gap, one past the last; overhang = min(m, m2).
    Motif of (sequence, start, end), from the sequence AS INDEXED (samtags_ref.Genome: a0 c1 g2 t3 n4): d = the bases at start and
    start + 1, a = the bases at end - 2 and end - 1; 1 GT..AG +, 2 CT..AC -, 3 GC..AG +, 4 CT..GC -, 5 AT..AC +, 6 GT..AT -, 0 anything else,
    any n, or end - start < 4 (no strand).  The read's own strand plays no part.
    Requests with equal (chrom_id, start, end) are one junction: reads, the largest overhang, motif, strand.  The table is sorted by
    (sequence in index order, start, end).  A request is FLAGGED - strand answer 0, counted nowhere - when its sequence does not exist,
    start == 0, end <= start, end >= the sequence's length or overhang == 0.

A dict over keys.  Also: the requests of the lines of a SAM file, and the table's text (STAR's SJ.out.tab layout)."""
import re

import numpy as np

# include/biokanga_amd.h: bk_junction_req (16 bytes), bk_junction (20 bytes)
JUNCTION_REQ_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("overhang", "<u2"), ("reserved", "<u2")])
JUNCTION_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("reads", "<u4"), ("max_overhang", "<u2"), ("motif", "u1"), ("strand", "u1")])
assert JUNCTION_REQ_DTYPE.itemsize == 16 and JUNCTION_DTYPE.itemsize == 20
PLUS, MINUS, NONE = ord("+"), ord("-"), ord(".")
# motif -> (donor pair, acceptor pair) as letters
MOTIFS = {1: ("GT", "AG"), 2: ("CT", "AC"), 3: ("GC", "AG"), 4: ("CT", "GC"), 5: ("AT", "AC"), 6: ("GT", "AT")}
_BY_CODES = {tuple("ACGT".index(c) for c in d + a): m for m, (d, a) in MOTIFS.items()}
_SPLICED = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?(\d+)N(\d+)M$")


def make_reqs(rows):
    """[(chrom_id, start, end, overhang)] -> request array"""
    out = np.zeros(len(rows), dtype=JUNCTION_REQ_DTYPE)
    for k, r in enumerate(rows):
        out[k]["chrom_id"], out[k]["start"], out[k]["end"], out[k]["overhang"] = r
    return out


def motif_of(codes, start, end):
    """codes: the sequence's base codes (0..4) -> motif 0..6"""
    if end - start < 4:
        return 0
    return _BY_CODES.get((int(codes[start]), int(codes[start + 1]), int(codes[end - 2]), int(codes[end - 1])), 0)


def strand_of(motif):
    return NONE if motif == 0 else (PLUS if motif & 1 else MINUS)


def is_flagged(q, genome):
    n = genome.length(int(q["chrom_id"]))
    return n == 0 or int(q["start"]) == 0 or int(q["end"]) <= int(q["start"]) or int(q["end"]) >= n or int(q["overhang"]) == 0


def junctions(reqs, genome):
    """genome: samtags_ref.Genome (its sequences in index order) -> (the table as JUNCTION_DTYPE, a byte per request - '+', '-' or 0 -,
    totals as bk_junction_totals has them)"""
    index_of = {cid: k for k, cid in enumerate(genome.codes)}
    reads, over = {}, {}
    strands = np.zeros(len(reqs), dtype=np.uint8)
    flagged = 0
    for i, q in enumerate(reqs):
        if is_flagged(q, genome):
            flagged += 1
            continue
        k = (int(q["chrom_id"]), int(q["start"]), int(q["end"]))
        reads[k] = reads.get(k, 0) + 1
        over[k] = max(over.get(k, 0), int(q["overhang"]))
        s = strand_of(motif_of(genome.codes[k[0]], k[1], k[2]))
        strands[i] = 0 if s == NONE else s
    table = np.zeros(len(reads), dtype=JUNCTION_DTYPE)
    by_motif = [0] * 7
    for n, k in enumerate(sorted(reads, key=lambda k: (index_of[k[0]], k[1], k[2]))):
        m = motif_of(genome.codes[k[0]], k[1], k[2])
        table[n] = (k[0], k[1], k[2], reads[k], over[k], m, strand_of(m))
        by_motif[m] += 1
    return table, strands, dict(requests=len(reqs), junctions=len(reads), flagged=flagged, max_reads=max(reads.values(), default=0), by_motif=by_motif)


def table_text(table, genome):
    """name, start + 1, end, strand 0 / 1 / 2, motif, 0, reads, 0, largest overhang - tab-separated, no header"""
    code = {NONE: 0, PLUS: 1, MINUS: 2}
    return "".join(f"{genome.names[int(j['chrom_id'])]}\t{int(j['start']) + 1}\t{int(j['end'])}\t{code[int(j['strand'])]}\t{int(j['motif'])}\t0\t{int(j['reads'])}\t0\t"
                   f"{int(j['max_overhang'])}\n" for j in table)


def request_of_line(rec, ids):
    """a record of helpers.parse_sam -> (chrom_id, start, end, overhang) when the line is accepted and its CIGAR is
    [c5 S] m M [c3 S] gap N m2 M, else None"""
    if rec["flag"] & 4:
        return None
    m = _SPLICED.match(rec["cigar"])
    if m is None:
        return None
    m1, gap, m2 = int(m.group(2)), int(m.group(4)), int(m.group(5))
    if gap <= 0:
        return None
    start = rec["pos"] - 1 + m1
    return ids[rec["rname"]], start, start + gap, min(m1, m2)


def requests_of_sam(lines, ids):
    """-> (the requests of the lines in file order, for each the index of its line)"""
    rows, line_of = [], []
    for k, r in enumerate(lines):
        q = request_of_line(r, ids)
        if q is not None:
            rows.append(q)
            line_of.append(k)
    return make_reqs(rows), line_of


def expected_xs(lines, genome):
    """-> per line None, or the '+' / '-' its XS:A must carry"""
    reqs, line_of = requests_of_sam(lines, genome.ids)
    _, strands, _ = junctions(reqs, genome)
    out = [None] * len(lines)
    for t, k in enumerate(line_of):
        if strands[t]:
            out[k] = chr(strands[t])
    return out


def log_line(tot):
    m = tot["by_motif"]
    return (f"Junctions: {tot['requests']} spliced records, {tot['junctions']} junctions ({m[1] + m[2]} GT/AG, {m[3] + m[4] + m[5] + m[6]} other canonical, "
            f"{m[0]} non-canonical), most reads at one junction {tot['max_reads']}")
