"""GPU tests of --sam-tags (NM:i / MD:Z made on the device): the request call bk_samtags on crafted records over a small index of its
own, the formatter bk_sam_format_tags on the records of golden files (read store as bytes and as packed words), and the command line -
device formatter, host formatter, gzip'd SAM, BAM.  The reference throughout is the literal walk of tests/samtags_ref.py against the
sequence as indexed."""
import gzip
import os
import struct

import numpy as np
import pytest

import biokanga_amd as bk
from biokanga_amd.binding import BkError, HIT_DTYPE, SEG2_DTYPE, SAMTAG_NM, SAMTAG_MD, SAMTAG_NONE
import helpers
import samtags_ref as sr
from test_gpu_cli import golden_bytes, run

pytestmark = pytest.mark.gpu


# ---- 1. the request call on crafted records ---------------------------------------------------------------------
def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for name, text in seqs:
            f.write(f">{name}\n")
            for k in range(0, len(text), 70):
                f.write(text[k:k + 70] + "\n")


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    """three sequences; the first holds an N run of 20 (shorter than the 25 from which the indexer mutates a run) and two single Ns"""
    d = tmp_path_factory.mktemp("samtags")
    rng = np.random.default_rng(20261020)
    texts = ["".join("ACGT"[c] for c in rng.integers(0, 4, n)) for n in (3000, 2600, 2300)]
    a = list(texts[0])
    a[500:520] = "N" * 20
    a[100] = a[1000] = "N"
    texts[0] = "".join(a)
    fa, sfx = str(d / "g.fa"), str(d / "g.sfx")
    _write_fasta(fa, zip(("tagA", "tagB", "tagC"), texts))
    run(["index", "-i", fa, "-o", sfx, "-r", "samtags"], str(d))
    g = sr.Genome(sfx)
    assert [g.names[i] for i in (1, 2, 3)] == ["tagA", "tagB", "tagC"]
    for i in (1, 2, 3):                                   # (nothing mutated: the index holds the file's letters)
        assert "".join(sr.LETTERS[c] for c in g.codes[i]) == texts[i - 1]
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        assert al.tune("samtag_buf_bytes", 0) == 0      # no call yet: nothing allocated
        yield al, g


def craft(g, rng, chrom, pos0, m, strand="+", c5=0, c3=0, gop=None, gap=0, m2=0, mism=(), read_n=()):
    """a SAM line (record of helpers.parse_sam's kind) whose M bases copy the target except at the positions `mism` (counted over both M
    runs), where another base stands, and `read_n`, where the read has N"""
    t = g.codes[chrom]
    other = lambda c: "ACGT"[(int(c) + 1) % 4] if c < 4 else "A"
    rnd = lambda n: "".join("ACGT"[c] for c in rng.integers(0, 4, n))
    tpos = list(range(pos0, pos0 + m))
    if gop:
        t2 = pos0 + m + (gap if gop in "ND" else 0)
        tpos += list(range(t2, t2 + m2))
    letters = [sr.LETTERS[t[p]] if t[p] < 4 else "A" for p in tpos]
    for k in mism:
        letters[k] = other(t[tpos[k]])
    for k in read_n:
        letters[k] = "N"
    seq = rnd(c5) + "".join(letters[:m]) + rnd(c3) + (rnd(gap) if gop == "I" else "") + "".join(letters[m:])
    cigar = (f"{c5}S" if c5 else "") + f"{m}M" + (f"{c3}S" if c3 else "") + (f"{gap}{gop}{m2}M" if gop else "")
    return dict(flag=16 if strand == "-" else 0, rname=g.names[chrom], pos=pos0 + 1, cigar=cigar, seq=seq)


def crafted_lines(g):
    rng = np.random.default_rng(7)
    L = {i: g.length(i) for i in (1, 2, 3)}
    out = []
    for m in (1, 63, 64, 65, 127, 128, 129, 512, 2000):
        out.append(craft(g, rng, 2, 17, m))                                                   # no mismatch
        out.append(craft(g, rng, 2, 5, m, mism=sorted({0, m - 1} | {p for p in (63, 64) if p < m})))      # base 0, 63, 64 and the last
        out.append(craft(g, rng, 3, 3, m, strand="-", mism=[m // 2]))
    out.append(craft(g, rng, 2, 40, 100, mism=[10, 11, 12]))                                  # adjacent
    out.append(craft(g, rng, 2, 0, 129, mism=range(129)))                                     # every base: MD 2 m + 1 long
    out.append(craft(g, rng, 3, 100, 2000, mism=range(2000)))
    out.append(craft(g, rng, 3, 100, 2000, strand="-", mism=range(0, 2000, 2)))
    out.append(craft(g, rng, 2, 200, 1300, mism=[9, 20, 120, 221, 1222]))                     # match runs of 9, 10, 99, 100, 1000 (and 77)
    for gap in (1, 20):
        out.append(craft(g, rng, 2, 300, 70, gop="D", gap=gap, m2=66, mism=[69, 70]))         # mismatches on either side of the deletion
        out.append(craft(g, rng, 2, 300, 64, strand="-", gop="D", gap=gap, m2=64))
        out.append(craft(g, rng, 2, 300, 70, gop="I", gap=gap, m2=66, mism=[3, 100]))
        out.append(craft(g, rng, 3, 300, 64, strand="-", gop="I", gap=gap, m2=65, c5=3, c3=2))
    out.append(craft(g, rng, 2, 50, 60, gop="N", gap=900, m2=70, mism=[59, 60, 129]))
    out.append(craft(g, rng, 2, 50, 60, strand="-", gop="N", gap=900, m2=70, c5=4))
    out.append(craft(g, rng, 2, 60, 80, c5=7))                                                # clips: either end, both, both strands
    out.append(craft(g, rng, 2, 60, 80, c3=9, mism=[0]))
    out.append(craft(g, rng, 2, 60, 80, c5=5, c3=6, mism=[79]))
    out.append(craft(g, rng, 2, 60, 80, strand="-", c5=5, c3=6, mism=[1, 78]))
    for c in (1, 3):                                                                          # first / last base of a sequence, of the last sequence
        out.append(craft(g, rng, c, 0, 90, mism=[0]))
        out.append(craft(g, rng, c, L[c] - 90, 90, mism=[89]))
        out.append(craft(g, rng, c, L[c] - 150, 70, strand="-", gop="D", gap=10, m2=70))
        out.append(craft(g, rng, c, 0, L[c] if L[c] <= 2000 else 2000))
    out.append(craft(g, rng, 1, 470, 100, read_n=[5]))                                        # over the N run: target N mismatches whatever the read has;
    out.append(craft(g, rng, 1, 470, 100, strand="-", read_n=[5, 35, 36]))                    # .. a read N over a base, over a target N
    out.append(craft(g, rng, 1, 95, 10, read_n=[5]))                                          # a single target N under a read N
    out.append(craft(g, rng, 1, 995, 10))
    return out


def as_requests(lines, g):
    reqs, bases, at = [], [], 0
    for ln in lines:
        r, codes = sr.request(ln, g, at)
        reqs.append(r)
        bases.append(codes)
        at += len(codes)
    return np.array(reqs, dtype=sr.SAMTAG_REQ_DTYPE), np.concatenate(bases)


def check_answers(nm, md, exp):
    for i, e in enumerate(exp):
        if e is None:
            assert nm[i] == SAMTAG_NONE and (md is None or md[i] is None), i
        else:
            assert nm[i] == e[0], (i, int(nm[i]), e[0])
            assert md is None or md[i].decode() == e[1], (i, md[i][:80], e[1][:80])


def test_request_call_on_crafted_records(crafted):
    al, g = crafted
    lines = crafted_lines(g)
    exp = [sr.ref_tags(ln, g) for ln in lines]
    assert all(e is not None for e in exp)
    assert max(len(e[1]) for e in exp) == 2 * 2000 + 1 and any(e[0] == 0 for e in exp)
    reqs, bases = as_requests(lines, g)
    nm, md = al.samtags(reqs, bases)
    check_answers(nm, md, exp)
    assert al.tune("samtag_buf_bytes", 0) > 0
    nm1, none = al.samtags(reqs, bases, md=False)          # NM alone
    assert none is None and np.array_equal(nm1, nm)


@pytest.mark.parametrize("count,chunk", [(1, 0), (63, 0), (64, 0), (65, 0), (257, 0), (257, 100)])
def test_request_counts_and_chunks(crafted, count, chunk):
    """1, 63, 64, 65 and 257 requests - a wave's worth, one less, one more, several blocks - also through staging of 100 at a time"""
    al, g = crafted
    pool = crafted_lines(g)
    lines = [pool[(7 * k) % len(pool)] for k in range(count)]
    reqs, bases = as_requests(lines, g)
    old = al.tune("samtag_chunk", chunk) if chunk else None
    try:
        nm, md = al.samtags(reqs, bases)
    finally:
        if chunk:
            al.tune("samtag_chunk", old)
    check_answers(nm, md, [sr.ref_tags(ln, g) for ln in lines])


def test_bad_requests_answer_for_themselves_only(crafted):
    """a malformed walk, a sequence that does not exist, a read outside the bases, a walk that leaves its sequence: "no tags" for that
    request; its neighbours get theirs"""
    al, g = crafted
    rng = np.random.default_rng(3)
    lines = [craft(g, rng, 2, 10 + 3 * k, 80, mism=[k]) for k in range(70)]
    reqs, bases = as_requests(lines, g)
    exp = [sr.ref_tags(ln, g) for ln in lines]
    reqs[5]["m"] = 79                                          # does not consume exactly SEQ
    reqs[6]["chrom_id"] = 99                                   # no such sequence
    reqs[7]["read_ofs"] = len(bases) - 10                      # the read leaves the bases
    reqs[8]["pos"] = g.length(2) - 79                          # leaves its sequence
    reqs[9]["gop"], reqs[9]["gap"], reqs[9]["m2"], reqs[9]["m"] = ord("D"), -2, 40, 40     # a number <= 0
    reqs[10]["gop"], reqs[10]["gap"], reqs[10]["m2"], reqs[10]["m"] = ord("I"), 0, 40, 40
    reqs[11]["gop"], reqs[11]["gap"], reqs[11]["m2"], reqs[11]["m"] = ord("X"), 1, 40, 40    # no operation of the writers'
    reqs[64]["m"], reqs[64]["c5"] = 0, 80
    for k in (5, 6, 7, 8, 9, 10, 11, 64):
        exp[k] = None
    nm, md = al.samtags(reqs, bases)
    check_answers(nm, md, exp)


def test_text_buffer_one_byte_too_small_and_bad_arguments(crafted):
    al, g = crafted
    lines = crafted_lines(g)[:40]
    reqs, bases = as_requests(lines, g)
    need = sum(len(sr.ref_tags(ln, g)[1]) for ln in lines)
    with pytest.raises(BkError) as e:
        al.samtags(reqs, bases, md_cap=need - 1)
    assert e.value.rc == -95 and e.value.needed == need and e.value.untouched
    nm, md = al.samtags(reqs, bases, md_cap=need)              # exactly enough
    check_answers(nm, md, [sr.ref_tags(ln, g) for ln in lines])
    bad = reqs.copy()
    bad[3]["strand"] = ord("?")
    with pytest.raises(BkError) as e:
        al.samtags(bad, bases)
    assert e.value.rc == -100
    assert al.lib.bk_samtags(al.h, None, 1, bases.ctypes.data, len(bases), None, None, None, 0, None) == -100


# ---- 2. the formatter with the tags inside its lines ------------------------------------------------------------
def records_of(sam_text, names_to_id):
    """the job bk_sam_format needs to write exactly these lines (one segment or two, end trims, a record per locus): read store, names,
    hits, src, seg2, trims - taken back out of the lines themselves"""
    import re
    shape = re.compile(r"^(?:(\d+)S)?(\d+)M(?:(\d+)S)?(?:(\d+)([NID])(\d+)M)?$")
    reads, names, read_of, hits, src, seg2, tl, tr = [], [], {}, [], [], {}, [], []
    for ln in sam_text.decode().split("\n"):
        if not ln or ln.startswith("@"):
            continue
        t = ln.split("\t")
        flag, seq = int(t[1]), t[9]
        read = sr.revcomp(seq) if flag & 16 else seq
        if t[0] not in read_of:
            read_of[t[0]] = len(reads)
            reads.append(read)
            names.append(t[0].encode())
        rd = read_of[t[0]]
        assert reads[rd] == read
        h = np.zeros(1, dtype=HIT_DTYPE)[0]
        if flag & 4:
            h["strand"], h["nar"] = ord("?"), helpers.NAR_TAGS.index(t[-1][5:])
            left = right = 0
        else:
            m = shape.match(t[5])
            c5, mm, c3 = int(m.group(1) or 0), int(m.group(2)), int(m.group(3) or 0)
            left, right = (c3, c5) if flag & 16 else (c5, c3)
            h["chrom_id"], h["match_loci"], h["match_len"], h["strand"], h["nar"], h["num_hits"] = names_to_id[t[2]], int(t[3]) - 1 - c5, mm + c5 + c3, ord("-" if flag & 16 else "+"), 1, 1
            if m.group(5):
                g = np.zeros(1, dtype=SEG2_DTYPE)[0]
                gap, op = int(m.group(4)), m.group(5)
                g["match_len"], g["flags"] = int(m.group(6)), {"N": 4, "I": 3, "D": 1}[op]
                g["match_loci"] = int(h["match_loci"]) + int(h["match_len"]) + (gap if op != "I" else 0)
                assert rd not in seg2
                seg2[rd] = g
        hits.append(h)
        src.append(rd)
        tl.append(left)
        tr.append(right)
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(len(reads), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1])
    bases = np.concatenate([sr.read_codes(r) for r in reads])
    kw = dict(trim_left=np.array(tl, dtype=np.uint16), trim_right=np.array(tr, dtype=np.uint16))
    if len(hits) != len(reads):
        kw["src"] = np.array(src, dtype=np.uint32)
    if seg2:
        kw["seg2"] = np.array([seg2.get(k, np.zeros(1, dtype=SEG2_DTYPE)[0]) for k in range(len(reads))], dtype=SEG2_DTYPE)
    return (bases, offs, lens, names, np.array(hits, dtype=HIT_DTYPE), np.arange(len(hits), dtype=np.uint32)), kw


def check_body(text, plain, g, mask):
    """`text` stripped of its tags is `plain`; every aligned line carries exactly the tags of the mask, with the reference's values"""
    bare, tags = sr.strip_body(text)
    assert bare == plain
    n = 0
    for ln, (nm, md) in zip([x for x in plain.decode().split("\n") if x], tags):
        e = sr.ref_tags(ln, g)
        if int(ln.split("\t")[1]) & 4:
            assert e is None and nm is None and md is None
            continue
        assert e is not None, ln
        assert nm == (e[0] if mask & SAMTAG_NM else None) and md == (e[1] if mask & SAMTAG_MD else None), (nm, md, e, ln)
        n += 1
    for ln in text.decode().split("\n"):                  # the line form: ...QUAL\tNM:i:<n>\tMD:Z:<s>, NM first
        f = ln.split("\t")
        if ln and not int(f[1]) & 4:
            assert [x[:5] for x in f[11:]] == [k for k, b in (("NM:i:", SAMTAG_NM), ("MD:Z:", SAMTAG_MD)) if mask & b], ln
    assert n > 100


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "packed"])
@pytest.mark.parametrize("fixture,tag", [("basic", "s3"), ("indel", "a10x4"), ("splice", "A5000"), ("chimeric", "c50"), ("multi", "r5R5x4")])
def test_formatter_writes_the_tags_inside_its_lines(golden_tmp, fixture, tag, packed):
    sfx = os.path.join(golden_tmp[fixture], "genome.sfx")
    g = sr.Genome(sfx)
    golden = b"".join(ln + b"\n" for ln in golden_bytes(fixture, f"{tag}.m6.sam.gz").split(b"\n") if ln and not ln.startswith(b"@"))
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        ids = {e["name"].decode(): int(e["entry_id"]) for e in al.entries()}
        job, kw = records_of(golden, ids)
        plain = al.sam_format(*job, **kw)
        assert plain == golden                             # (the records are the file's)
        assert al.sam_format(*job, tags=0, packed=packed, **kw) == plain
        check_body(al.sam_format(*job, tags=SAMTAG_NM | SAMTAG_MD, packed=packed, **kw), plain, g, SAMTAG_NM | SAMTAG_MD)
        check_body(al.sam_format(*job, tags=SAMTAG_NM, packed=packed, **kw), plain, g, SAMTAG_NM)
        check_body(al.sam_format(*job, tags=SAMTAG_MD, packed=packed, **kw), plain, g, SAMTAG_MD)
        with pytest.raises(BkError) as e:
            al.sam_format(*job, tags=4, **kw)
        assert e.value.rc == -100


def test_formatter_reads_with_n_and_malformed_records(golden_tmp):
    """reads with N (the packed form's exception runs) on both strands, and a record whose CIGAR numbers do not add up to its read: that
    line stays as bk_sam_format writes it, the others get their tags"""
    sfx = os.path.join(golden_tmp["basic"], "genome.sfx")
    g = sr.Genome(sfx)
    t = "".join(sr.LETTERS[c] for c in g.codes[1][1000:1060])
    assert "N" not in t
    reads = [t[:10] + "N" + t[11:40] + "NNN" + t[43:], sr.revcomp(t[:59] + "N"), t, "N" * 60, t]
    names = [b"n_plus", b"n_minus", b"short_walk", b"all_n", b"left_of_its_sequence"]
    hits = np.zeros(5, dtype=HIT_DTYPE)
    hits["chrom_id"], hits["match_loci"], hits["match_len"], hits["nar"] = 1, 1000, 60, 1
    hits["strand"] = [ord(c) for c in "+-+++"]
    hits["match_len"][2] = 50                              # 50M over a read of 60: not a walk of SEQ
    hits["match_loci"][4] = g.length(1) - 30               # 60M from 30 before the end: leaves its sequence
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.zeros(5, dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1])
    bases = np.concatenate([sr.read_codes(r) for r in reads])
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        plain = al.sam_format(bases, offs, lens, names, hits, np.arange(5))
        for packed in (False, True):
            text = al.sam_format(bases, offs, lens, names, hits, np.arange(5), tags=3, packed=packed)
            got, exp = text.split(b"\n"), plain.split(b"\n")
            assert got[2] == exp[2] and got[4] == exp[4] and got[5] == exp[5] == b""
            for k in (0, 1, 3):
                bare, nm, md = sr.split_tags(got[k])
                assert bare == exp[k] and (nm, md) == sr.ref_tags(exp[k].decode(), g), got[k]
            assert sr.split_tags(got[0])[1:] == (4, "10" + t[10] + "29" + t[40] + "0" + t[41] + "0" + t[42] + "17")
            assert sr.split_tags(got[3])[1] == 60


# ---- 3. the command line ------------------------------------------------------------------------------------------
PE = ["-d200", "-D400"]
# (golden fixture, tag, genome fixture, paired reads' fixture, options)
CLI = [("basic", "s3", "basic", None, ["-s3"]), ("indel", "a10x4", "indel", None, ["-a10", "-s3", "-x4"]),
       ("pe", "U3", "basic", "pe", ["-U3", "-s5"] + PE), ("multi", "r5R5x4", "multi", None, ["-s3", "-r5", "-R5", "-x4"])]


def cli_args(golden_tmp, tmp_path, genome, pe, flags, out):
    d = golden_tmp[genome]
    if pe is None:
        inputs = ["-i", os.path.join(d, "reads.fa")]
    else:
        r1, r2 = str(tmp_path / "r1.fa"), str(tmp_path / "r2.fa")
        if not os.path.exists(r1):
            helpers.gunzip_to(os.path.join(helpers.GOLDEN, pe, "reads_1.fa.gz"), r1)
            helpers.gunzip_to(os.path.join(helpers.GOLDEN, pe, "reads_2.fa.gz"), r2)
        inputs = ["-i", r1, "-u", r2]
    return ["align"] + inputs + ["-I", os.path.join(d, "genome.sfx"), "-o", out, "-M6"] + flags


def check_file(text, golden, g):
    """the file without its tags is the golden file; every aligned line has both tags, the reference's"""
    bare, tags = sr.strip_body(text)
    assert bare == golden
    body = [ln for ln in golden.decode().split("\n") if ln and not ln.startswith("@")]
    assert len(body) == len(tags)
    n = 0
    for ln, (nm, md) in zip(body, tags):
        e = sr.ref_tags(ln, g)
        if int(ln.split("\t")[1]) & 4:
            assert (nm, md) == (None, None)
        else:
            assert e is not None and (nm, md) == e, (nm, md, e, ln)
            n += 1
    assert n > 100
    return n


@pytest.mark.parametrize("fixture,tag,genome,pe,flags", CLI, ids=[f"{c[0]}-{c[1]}" for c in CLI])
def test_cli_device_and_host_formatter_write_the_same_tagged_file(golden_tmp, tmp_path, fixture, tag, genome, pe, flags):
    g = sr.Genome(os.path.join(golden_tmp[genome], "genome.sfx"))
    dev, host = str(tmp_path / "dev.sam"), str(tmp_path / "host.sam")
    log = run(cli_args(golden_tmp, tmp_path, genome, pe, flags, dev) + ["--sam-tags", "NM,MD"], str(tmp_path), env={"BK_SAM_DEVICE_MIN": "1", "BK_TIMING": "1"})
    assert "SAM formatted on the device" in log, log[-1500:]
    log = run(cli_args(golden_tmp, tmp_path, genome, pe, flags, host) + ["--sam-tags", "NM,MD"], str(tmp_path), env={"BK_SAM_DEVICE_MIN": str(1 << 40), "BK_TIMING": "1"})
    assert "SAM formatted on the device" not in log and "SAM tags:" in log, log[-1500:]
    text = open(dev, "rb").read()
    assert text == open(host, "rb").read()
    check_file(text, golden_bytes(fixture, f"{tag}.m6.sam.gz"), g)
    if fixture == "basic":
        # one segment, untrimmed, no N on either side: NM is the mismatch count the run reports (-M0 column of the same run)
        csv = helpers.parse_m0_csv(os.path.join(helpers.GOLDEN, "basic", "s3.m0.csv.gz"))
        n = 0
        for ln in text.decode().split("\n"):
            f = ln.split("\t")
            if not ln or ln.startswith("@") or int(f[1]) & 4 or "N" in f[9] or "N" in sr.split_tags(ln)[2]:
                continue
            assert f[5] == f"{len(f[9])}M"
            assert sr.split_tags(ln)[1] == csv[f[0]]["mismatches"], ln
            n += 1
        assert n > 100


def test_cli_single_tags(golden_tmp, tmp_path):
    g = sr.Genome(os.path.join(golden_tmp["basic"], "genome.sfx"))
    golden = golden_bytes("basic", "s3.m6.sam.gz")
    for spec, env in (("NM", "1"), ("MD", str(1 << 40))):
        out = str(tmp_path / f"{spec}.sam")
        run(cli_args(golden_tmp, tmp_path, "basic", None, ["-s3"], out) + [f"--sam-tags={spec}"], str(tmp_path), env={"BK_SAM_DEVICE_MIN": env})
        bare, tags = sr.strip_body(open(out, "rb").read())
        assert bare == golden
        body = [ln for ln in golden.decode().split("\n") if ln and not ln.startswith("@")]
        for ln, (nm, md) in zip(body, tags):
            e = sr.ref_tags(ln, g)
            assert (nm, md) == ((None, None) if e is None else ((e[0], None) if spec == "NM" else (None, e[1]))), ln


def bam_records(path):
    """the uncompressed stream of a BAM -> [(record bytes without block_size)]"""
    raw = gzip.open(path, "rb").read()
    assert raw[:4] == b"BAM\1"
    l_text, = struct.unpack_from("<I", raw, 4)
    at = 8 + l_text
    n_ref, = struct.unpack_from("<I", raw, at)
    at += 4
    for _ in range(n_ref):
        l_name, = struct.unpack_from("<I", raw, at)
        at += 4 + l_name + 4
    head, recs = raw[:at], []
    while at < len(raw):
        size, = struct.unpack_from("<I", raw, at)
        recs.append(raw[at + 4:at + 4 + size])
        at += 4 + size
    assert at == len(raw)
    return head, recs


def bam_aux(aux):
    out, at = {}, 0
    while at < len(aux):
        tag, typ = aux[at:at + 2].decode(), chr(aux[at + 2])
        at += 3
        if typ == "C":
            out[tag], at = aux[at], at + 1
        elif typ == "S":
            out[tag], at = struct.unpack_from("<H", aux, at)[0], at + 2
        else:
            assert typ == "Z"
            end = aux.index(b"\0", at)
            out[tag], at = aux[at:end].decode(), end + 1
    return out


def test_cli_gzip_and_bam_carry_the_same_tags(golden_tmp, tmp_path):
    opts = ["-s3"]
    plain, gz, bam, bam0 = (str(tmp_path / n) for n in ("x.sam", "x.sam.gz", "x.bam", "x0.bam"))
    for out in (plain, gz, bam):
        run(cli_args(golden_tmp, tmp_path, "basic", None, opts, out) + ["--sam-tags", "NM,MD"], str(tmp_path), env={"BK_SAM_DEVICE_MIN": "1"})
    run(cli_args(golden_tmp, tmp_path, "basic", None, opts, bam0), str(tmp_path))
    text = open(plain, "rb").read()
    assert gzip.open(gz, "rb").read() == text
    assert open(bam0, "rb").read() == open(os.path.join(helpers.GOLDEN, "basic", "s3.m6.bam"), "rb").read()      # (without the option: the reference's file)
    _, tags = sr.strip_body(text)
    names = [ln.split(b"\t")[0] for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]
    head, recs = bam_records(bam)
    head0, recs0 = bam_records(bam0)
    assert head == head0 and len(recs) == len(recs0) == len(tags)
    n_wide = 0
    for r, r0, (nm, md), name in zip(recs, recs0, tags, names):
        assert r[:len(r0)] == r0 and r0[32:32 + r0[8]] == name + b"\0"       # bin, index fields and everything else untouched; the tags are appended
        aux = r[len(r0):]
        if nm is None:
            assert aux == b""
            continue
        assert bam_aux(aux) == {"NM": nm, "MD": md}
        assert aux[:3] == (b"NMC" if nm <= 255 else b"NMS")
        n_wide += 1
    assert n_wide > 100
