"""Shared by the --coverage tests: the rule of bk_coverage_runs / bk_coverage_text (include/biokanga_amd.h) in numpy.

    Depth at a target position = the number of accepted records whose line as written has an M base there.  A request is the M runs of
    one line, m M [gap N|I|D m2 M] from `pos` (0-based): the first run covers [pos, pos + m), the second [pos + m + gap, .. + m2) - gap
    is 0 behind an I.  A request is FLAGGED - and counts nothing - when its sequence does not exist, m is 0, gap is negative or either
    run leaves its sequence.  Output: one run per maximal stretch of equal non-zero depth, sequences by ascending id, runs by start,
    never across two sequences; as text name<TAB>start<TAB>end<TAB>depth<LF>.

np.add.at on a delta array per sequence, cumsum, run extraction.  Also: the requests of the accepted lines of a SAM file."""
import re

import numpy as np

# include/biokanga_amd.h: bk_cov_req, bk_cov_run (16 bytes each)
COV_REQ_DTYPE = np.dtype([("chrom_id", "<u4"), ("pos", "<u4"), ("m", "<u2"), ("m2", "<u2"), ("gap", "<i4")])
COV_RUN_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("depth", "<u4")])
assert COV_REQ_DTYPE.itemsize == 16 and COV_RUN_DTYPE.itemsize == 16
_SHAPE = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?(?:(\d+)([NID])(\d+)M)?$")


def make_reqs(rows):
    """[(chrom_id, pos, m[, m2, gap])] -> request array"""
    out = np.zeros(len(rows), dtype=COV_REQ_DTYPE)
    for k, r in enumerate(rows):
        out[k]["chrom_id"], out[k]["pos"], out[k]["m"] = r[0], r[1], r[2]
        if len(r) > 3:
            out[k]["m2"], out[k]["gap"] = r[3], r[4]
    return out


def flagged(reqs, lengths):
    """lengths: {chrom_id: bases} -> a bool per request"""
    ln = np.array([lengths.get(int(c), -1) for c in reqs["chrom_id"]], dtype=np.int64)
    pos, m, m2, gap = (reqs[f].astype(np.int64) for f in ("pos", "m", "m2", "gap"))
    return (ln < 0) | (m == 0) | (gap < 0) | (pos + m > ln) | ((m2 > 0) & (pos + m + gap + m2 > ln))


def depth(reqs, lengths):
    """{chrom_id: depth per base (int64)} of the requests that are not flagged"""
    ok = reqs[~flagged(reqs, lengths)]
    out = {}
    for c in sorted(lengths):
        q = ok[ok["chrom_id"] == c]
        delta = np.zeros(lengths[c] + 1, dtype=np.int64)
        pos, m, m2, gap = (q[f].astype(np.int64) for f in ("pos", "m", "m2", "gap"))
        np.add.at(delta, pos, 1)
        np.add.at(delta, pos + m, -1)
        two = m2 > 0
        np.add.at(delta, (pos + m + gap)[two], 1)
        np.add.at(delta, (pos + m + gap + m2)[two], -1)
        out[c] = np.cumsum(delta)[:-1]
        assert delta.sum() == 0
    return out


def runs_of(reqs, lengths):
    """-> (runs as COV_RUN_DTYPE in output order, totals as bk_cov_totals has them)"""
    parts, covered, dsum, dmax = [], 0, 0, 0
    for c, d in depth(reqs, lengths).items():
        prev = np.concatenate(([0], d[:-1]))
        nxt = np.concatenate((d[1:], [0]))
        starts = np.nonzero((d != 0) & (d != prev))[0]
        ends = np.nonzero((d != 0) & (d != nxt))[0] + 1
        assert len(starts) == len(ends)
        r = np.zeros(len(starts), dtype=COV_RUN_DTYPE)
        r["chrom_id"], r["start"], r["end"], r["depth"] = c, starts, ends, d[starts]
        parts.append(r)
        covered += int((d != 0).sum())
        dsum += int(d.sum())
        dmax = max(dmax, int(d.max()) if len(d) else 0)
    runs = np.concatenate(parts) if parts else np.zeros(0, dtype=COV_RUN_DTYPE)
    return runs, dict(runs=len(runs), covered=covered, depth_sum=dsum, max_depth=dmax, flagged=int(flagged(reqs, lengths).sum()))


def text_of(runs, names):
    """names: {chrom_id: name} -> the bedGraph as bytes"""
    return "".join(f"{names[int(r['chrom_id'])]}\t{int(r['start'])}\t{int(r['end'])}\t{int(r['depth'])}\n" for r in runs).encode()


def requests_of_sam(recs, ids):
    """the requests of the accepted lines (records of helpers.parse_sam) - the walk of each line's POS and CIGAR, which has the one shape
    the writers make, [c5 S] m M [c3 S] [gap N|I|D m2 M]; ids: {sequence name: chrom_id}"""
    rows = []
    for r in recs:
        if r["flag"] & 4:
            continue
        m = _SHAPE.match(r["cigar"])
        assert m is not None, r["cigar"]
        row = [ids[r["rname"]], r["pos"] - 1, int(m.group(2))]
        if m.group(5):
            row += [int(m.group(6)), 0 if m.group(5) == "I" else int(m.group(4))]
        rows.append(row)
    return make_reqs(rows)
