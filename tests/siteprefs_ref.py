"""Shared by the site-preference tests (tests/golden/siteprefs): the golden genome as base codes, a numpy restatement of the start-site
octamer gather (CAligner::ProcessSiteProbabilites, Aligner.cpp:8130-8157, in the reference's UINT32 arithmetic) and the visited reads
of a golden SAM / BED in the order the reference wrote them."""
import gzip
import json
import os

import numpy as np

import helpers
from biokanga_amd.binding import SITE_REQ_DTYPE, SITE_RES_DTYPE

DIR = os.path.join(helpers.GOLDEN, "siteprefs")
M32 = 0xffffffff
NOTHING = 0x80000000


def cases():
    with open(os.path.join(DIR, "cases.json")) as f:
        return json.load(f)


def golden(name):
    return gzip.open(os.path.join(DIR, name), "rb").read()


class Genome:
    """sequences of genome.fa.gz in file order (EntryID 1..): codes a0 c1 g2 t3 n4, one array, with each sequence's start and length"""

    def __init__(self):
        names, seqs, cur = [], [], None
        for line in gzip.open(os.path.join(DIR, "genome.fa.gz"), "rt"):
            line = line.strip()
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                cur = []
                seqs.append(cur)
            elif line:
                cur.append(line)
        lut = np.full(256, 4, dtype=np.uint8)
        for i, ch in enumerate("ACGT"):
            lut[ord(ch)] = lut[ord(ch.lower())] = i
        arrs = [lut[np.frombuffer("".join(s).encode(), dtype=np.uint8)] for s in seqs]
        self.names = names
        self.lens = np.array([0] + [len(a) for a in arrs], dtype=np.int64)            # by EntryID
        self.starts = np.concatenate([[0, 0], np.cumsum(self.lens[1:])[:-1]]).astype(np.int64)
        self.codes = np.concatenate(arrs)
        self.ids = {n: i + 1 for i, n in enumerate(names)}


def ref_octamers(g, reqs, ofs):
    """SITE_RES_DTYPE for SITE_REQ_DTYPE requests"""
    n = len(reqs)
    loci, ln = reqs["match_loci"].astype(np.int64), reqs["match_len"].astype(np.int64)
    minus = reqs["strand"] == ord("-")
    clen = g.lens[reqs["chrom_id"]]
    site = np.where(minus, loci + ln - 1 - ofs - 7, loci + ofs) & M32
    site = np.where(((site + 8) & M32) >= clen, (clen - 9) & M32, site)
    ok = site < clen
    out = np.zeros(n, dtype=SITE_RES_DTYPE)
    out["site"] = site
    at = np.where(ok, g.starts[reqs["chrom_id"]] + site, 0)
    b = g.codes[at[:, None] + np.arange(8)[None, :]].astype(np.uint32) & 7
    rc = b[:, ::-1]
    rc = np.where(rc < 4, 3 - rc, rc)
    b = np.where(minus[:, None], rc, b)
    codes = np.zeros(n, dtype=np.uint32)
    for k in range(8):
        codes |= b[:, k] << np.uint32(21 - 3 * k)
    out["codes"] = np.where(ok, codes, np.uint32(NOTHING))
    return out


def visits_from_sam(g, name):
    """the accepted single-end records of a golden SAM, in file order = the order ProcessSiteProbabilites visited them"""
    _, recs = helpers.parse_sam(os.path.join(DIR, name))
    reqs = np.zeros(len(recs), dtype=SITE_REQ_DTYPE)
    for i, r in enumerate(recs):
        assert r["cigar"] == f"{len(r['seq'])}M"
        reqs[i] = (g.ids[r["rname"]], r["pos"] - 1, len(r["seq"]), ord("-") if r["flag"] & 16 else ord("+"), 0)
    return reqs
