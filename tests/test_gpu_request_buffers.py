"""GPU tests of the staging the request passes keep with their context (run with -m gpu on an MI355X), in the manner of
test_gpu_ctx_buffers.py: one context goes through every pass over finished alignments - site octamers, primer correction, constraints
check, SAM tags with MD text, coverage runs and coverage text - three times: 300 requests in chunks of 97 (several chunks, the last one
short), 1500 requests in one chunk (the staging grows), the 300 again (the staging is larger than needed).  And bk_sam_format twice on
one context, the second call's slice needing more text than the pinned pair the first call left.  Every answer is compared bytewise with
what a fresh context gives for the same call (the answers the passes' own tests hold to their restatements).  Who frees what, and when,
is checked on the host (test_host_devbuf.py)."""
import os
import re

import numpy as np
import pytest

import helpers
from test_gpu_iv_records import _cut_reads

pytestmark = pytest.mark.gpu

ACCEPTED = 1                                          # BK_NAR_ACCEPTED
KNOBS = ("site_chunk", "primer_chunk", "constraint_chunk", "samtag_chunk", "coverage_req_chunk", "coverage_run_chunk")


def _bk():
    import biokanga_amd                               # (its __init__ imports biokanga_amd.binding, the layouts' home)
    return biokanga_amd


@pytest.fixture(scope="module")
def repeat(golden_tmp):
    path = os.path.join(golden_tmp["repeat"], "genome.sfx")
    seq, _, _ = helpers.read_sfx(path)
    return {"sfx": path, "seq": seq}


@pytest.fixture(scope="module")
def aligned(repeat):
    """2800 reads of 40 .. 100 bases with 0 .. 3 substitutions, cut from 30 000 bases of the target (so that they lie over each other),
    and their hits; the accepted ones are what the requests are made of"""
    bk = _bk()
    rng = np.random.default_rng(20)
    bases, offs, lens = _cut_reads(repeat["seq"][100000:130000], rng, rng.integers(40, 101, size=2800), max_e=3)
    with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
        hits = al.align(bases, offs, lens)
    acc = np.flatnonzero((hits["nar"] == ACCEPTED) & (hits["match_len"] == lens))
    assert len(acc) >= 1800
    return {"bases": bases, "offs": offs, "lens": lens, "hits": hits, "few": acc[1500:1800], "many": acc[:1500]}


def _requests(aligned, idx):
    """the requests of every pass for the accepted reads idx, and a constraint every fifth of them has in its middle"""
    bk = _bk()
    h, offs, lens, bases = aligned["hits"][idx], aligned["offs"][idx], aligned["lens"][idx], aligned["bases"]
    n = len(idx)
    site = np.zeros(n, dtype=bk.binding.SITE_REQ_DTYPE)
    primer = np.zeros(n, dtype=bk.binding.PRIMER_REQ_DTYPE)
    cons = np.zeros(n, dtype=bk.binding.CONSTRAINT_REQ_DTYPE)
    tags = np.zeros(n, dtype=bk.binding.SAMTAG_REQ_DTYPE)
    cov = np.zeros(n, dtype=bk.binding.COV_REQ_DTYPE)
    for r in (site, primer, cons, tags, cov):
        r["chrom_id"] = h["chrom_id"]
    for r in (site, primer, cons, tags):
        r["strand"] = h["strand"]
    for r in (site, primer):
        r["match_loci"], r["match_len"] = h["match_loci"], h["match_len"]
    first12 = np.stack([bases[int(o):int(o) + 12] & 7 for o in offs]).astype(np.uint64)
    primer["codes"] = (first12 << (3 * np.arange(11, -1, -1, dtype=np.uint64))).sum(axis=1)
    primer["low_mm"], primer["max_mms"] = h["low_mm"], 1
    for r in (cons, tags):
        r["read_ofs"], r["read_len"] = offs, lens
    cons["n_segs"] = 1
    cons["seg"]["start"][:, 0], cons["seg"]["len"][:, 0] = h["match_loci"], h["match_len"]
    tags["pos"], tags["m"] = h["match_loci"], h["match_len"]
    cov["pos"], cov["m"] = h["match_loci"], h["match_len"]
    mid = h[::5]
    table = np.zeros(len(mid), dtype=bk.binding.CONSTRAINT_DTYPE)
    table["chrom_id"], table["mask"] = mid["chrom_id"], bk.binding.CONSTRAINT_R
    table["start"] = mid["match_loci"] + mid["match_len"] // 2
    table["end"] = table["start"] + 2
    return {"site": site, "primer": primer, "cons": cons, "tags": tags, "cov": cov, "table": table}


def _every_pass(al, rq, bases, chunk):
    """the six passes on `al` with every chunk knob at `chunk`; everything they answer, as bytes where it is an array"""
    for k in KNOBS:
        al.tune(k, chunk)
    out = {"site": al.site_octamers(rq["site"], -4).tobytes(), "primer": al.primer_correct(rq["primer"])}
    with al.constraints(rq["table"]) as cs:
        out["cons"] = cs.check(rq["cons"], bases)
    nm, md = al.samtags(rq["tags"], bases)
    out["tags"] = (nm.tobytes(), md)
    out["runs"] = al.coverage_runs(rq["cov"])
    out["text"] = al.coverage_text(rq["cov"])
    return out


def _same(got, exp, what):
    bk = _bk()
    assert got["site"] == exp["site"], f"{what}: site octamers differ from a fresh context's"
    assert got["primer"].tobytes() == exp["primer"].tobytes(), f"{what}: primer correction differs"
    assert got["cons"][0].tobytes() == exp["cons"][0].tobytes() and got["cons"][1] == exp["cons"][1], f"{what}: constraint statuses differ"
    assert got["tags"] == exp["tags"], f"{what}: SAM tags differ"
    assert got["runs"][0].tobytes() == exp["runs"][0].tobytes() and got["runs"][1:] == exp["runs"][1:], f"{what}: coverage runs differ"
    assert got["text"] == exp["text"], f"{what}: coverage text differs"
    # .. and none of it is an empty answer
    assert (exp["primer"]["status"] == bk.binding.PRIMER_CORRECTED).any(), what
    assert (exp["cons"][0] != bk.binding.CONSTRAINT_UNTOUCHED).any() and exp["cons"][1][1] > 0, what
    assert any(t is not None and re.search(rb"[ACGT]", t) for t in exp["tags"][1]), what
    assert (exp["runs"][0]["depth"] > 1).any() and len(exp["text"][0]) > 0, what


def test_one_context_through_every_request_pass_three_times(repeat, aligned):
    bk = _bk()
    few, many, bases = _requests(aligned, aligned["few"]), _requests(aligned, aligned["many"]), aligned["bases"]
    steps = [("300 in chunks of 97", few, 97), ("1500 in one chunk", many, 1 << 20), ("300 again", few, 97)]
    with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
        assert al.tune("primer_buf_bytes", 0) == 0 and al.tune("samtag_buf_bytes", 0) == 0 and al.tune("coverage_buf_bytes", 0) == 0
        got, held = [], []
        for _, rq, chunk in steps:
            got.append(_every_pass(al, rq, bases, chunk))
            held.append([al.tune(k, 0) for k in ("primer_buf_bytes", "samtag_buf_bytes", "coverage_buf_bytes")])
    exp = {}
    for (what, rq, chunk), g in zip(steps, got):
        if chunk not in exp:
            with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as fresh:
                exp[chunk] = _every_pass(fresh, rq, bases, chunk)
        _same(g, exp[chunk], what)
    assert len(got[0]["runs"][2]) > 1                                     # coverage_run_chunk 97: the runs came in several sink calls
    # the staging grew for the 1500 requests and was kept, larger than needed, for the 300
    assert held[0][0] == 97 * 40 and held[1][0] == 1500 * 40 and held[2] == held[1]
    assert all(a < b for a, b in zip(held[0], held[1]))


def test_sam_format_outgrows_the_text_buffers_the_call_before_left(repeat, aligned):
    """the pinned text buffers a call leaves with its context hold its largest slice, an eighth more and 1 MiB (bk_sam.hip): the second
    call's one slice is larger than that, so it takes the pair, outgrows it and replaces it"""
    bk = _bk()
    rng = np.random.default_rng(21)
    big = _cut_reads(repeat["seq"], rng, np.full(12000, 100), max_e=3)
    small = (aligned["bases"], aligned["offs"][:50], aligned["lens"][:50])
    jobs = []
    with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
        for tag, rd in (("s", small), ("b", big)):
            n = len(rd[2])
            jobs.append(rd + ([b"%s_read_%06d_of_the_request_buffer_test" % (tag.encode(), i) for i in range(n)], al.align(*rd), np.arange(n)))
        got = [al.sam_format(*j) for j in jobs]
    exp = []
    for j in jobs:
        with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as fresh:
            exp.append(fresh.sam_format(*j))
    assert got[0] == exp[0] and got[1] == exp[1]
    assert got[0].count(b"\n") == 50 and got[1].count(b"\n") == 12000
    assert len(got[1]) > len(got[0]) + len(got[0]) // 8 + (1 << 20)
