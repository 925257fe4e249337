"""GPU tests of the device SAM formatter (`bk_sam_format`) on records that are more than a plain hit: end trims (-x, -A, -c), a second
segment (-a, -A), several records of one read (-r5) - through the command line against the files the real reference wrote
(tests/golden/*), and through the C ABI against lines written out here."""
import os

import numpy as np
import pytest

import biokanga_amd as bk
from biokanga_amd.binding import BkError, HIT_DTYPE, SEG2_DTYPE
import helpers
from test_gpu_cli import golden_bytes, run

pytestmark = pytest.mark.gpu

DEVICE_ENV = {"BK_SAM_DEVICE_MIN": "1", "BK_TIMING": "1"}
PE_DFLT = ["-d200", "-D400"]

# (fixture of the golden file, its tag, -M, genome fixture, paired reads' fixture or None, options): the options are those of the host-path
# tests of the same files (tests/test_gpu_cli.py) and of the reference runs that wrote them (tests/golden/make_golden.py)
CASES = [
    # -x: flank trims
    ("basic", "s3x5", 6, "basic", None, ["-s3", "-x5"]), ("basic", "s3x5", 5, "basic", None, ["-s3", "-x5"]),
    ("basic", "s10x6", 6, "basic", None, ["-s10", "-x6"]),
    # -a: microInDels
    ("indel", "a10", 6, "indel", None, ["-a10", "-s3"]), ("indel", "a10", 5, "indel", None, ["-a10", "-s3"]),
    ("indel", "a3s5", 6, "indel", None, ["-a3", "-s5"]), ("indel", "a20Q1", 6, "indel", None, ["-a20", "-s3", "-Q1"]),
    ("indel", "a10x4", 6, "indel", None, ["-a10", "-s3", "-x4"]),
    # -A: splice junctions (switches -x on)
    ("splice", "A5000", 6, "splice", None, ["-A5000", "-s3"]), ("splice", "A5000", 5, "splice", None, ["-A5000", "-s3"]),
    ("splice", "A500s5", 6, "splice", None, ["-A500", "-s5"]), ("splice", "A5000a5", 6, "splice", None, ["-A5000", "-a5", "-s3"]),
    # -c: chimeric trims
    ("chimeric", "c50", 6, "chimeric", None, ["-c50", "-s3"]), ("chimeric", "c50", 5, "chimeric", None, ["-c50", "-s3"]),
    ("chimeric", "c60e2", 6, "chimeric", None, ["-c60", "-s3", "-e2"]), ("chimeric", "c70s5", 6, "chimeric", None, ["-c70", "-s5"]),
    # -r5: a record per locus
    ("multi", "r5R5", 6, "multi", None, ["-s3", "-r5", "-R5"]), ("multi", "r5R5", 5, "multi", None, ["-s3", "-r5", "-R5"]),
    ("multi", "r5R3X", 6, "multi", None, ["-s3", "-r5", "-R3", "-X"]), ("multi", "r5R5x4", 6, "multi", None, ["-s3", "-r5", "-R5", "-x4"]),
    ("multi", "r5R5N", 6, "multi", None, ["-s3", "-r5", "-R5", "-N"]),
    # -r with -c / -a
    ("chimml", "r5R5c50", 6, "chimml", None, ["-r5", "-R5", "-c50", "-s3", "-T1"]), ("chimml", "r3R5c50", 6, "chimml", None, ["-r3", "-R5", "-c50", "-s3", "-T4"]),
    ("chimmlindel", "r3R5c50a8", 6, "chimmlindel", None, ["-r3", "-R5", "-c50", "-a8", "-s3", "-T4"]),
    ("chimmlindel", "r3R3Xc55a10A200", 6, "chimmlindel", None, ["-r3", "-R3", "-X", "-c55", "-a10", "-A200", "-s3", "-T1"]),
    # paired ends with trims
    ("pe", "U3x4", 6, "basic", "pe", ["-U3", "-d200", "-D400", "-s5", "-x4"]),
    ("pechim", "U3c50", 6, "chimeric", "pechim", ["-U3", "-c50", "-s3"] + PE_DFLT), ("pechim", "U1c60", 6, "chimeric", "pechim", ["-U1", "-c60", "-s3"] + PE_DFLT),
    ("pechim", "U2c70s5", 6, "chimeric", "pechim", ["-U2", "-c70", "-s5"] + PE_DFLT), ("pechim", "U4c50", 6, "chimeric", "pechim", ["-U4", "-c50", "-s3"] + PE_DFLT),
    ("pechim", "U3c50wide", 6, "chimeric", "pechim", ["-U3", "-c50", "-s3", "-d150", "-D1500"]),
]


def align_args(golden_tmp, tmp_path, m, genome, pe, flags):
    d = golden_tmp[genome]
    if pe is None:
        inputs = ["-i", os.path.join(d, "reads.fa")]
    else:
        r1, r2 = str(tmp_path / "r1.fa"), str(tmp_path / "r2.fa")
        helpers.gunzip_to(os.path.join(helpers.GOLDEN, pe, "reads_1.fa.gz"), r1)
        helpers.gunzip_to(os.path.join(helpers.GOLDEN, pe, "reads_2.fa.gz"), r2)
        inputs = ["-i", r1, "-u", r2]
    return ["align"] + inputs + ["-I", os.path.join(d, "genome.sfx"), "-o", str(tmp_path / "o.sam"), f"-M{m}"] + flags


def assert_same_text(got, exp, what):
    if got != exp:
        g, e = got.split(b"\n"), exp.split(b"\n")
        k = next((i for i in range(min(len(g), len(e))) if g[i] != e[i]), min(len(g), len(e)))
        raise AssertionError(f"{what}: {len(g)} vs {len(e)} lines, first difference at line {k}:\n{g[k:k+1]}\n{e[k:k+1]}")


@pytest.mark.parametrize("fixture,tag,m,genome,pe,flags", CASES, ids=[f"{c[0]}-{c[1]}.m{c[2]}" for c in CASES])
def test_trimmed_two_segment_and_multi_loci_records_formatted_on_the_device(golden_tmp, tmp_path, fixture, tag, m, genome, pe, flags):
    """the runs whose records carry end trims, a second segment or belong several to a read get their SAM text from the device - the log
    says so, the head start (given the reads) was taken - and the file is the reference's, byte for byte"""
    log = run(align_args(golden_tmp, tmp_path, m, genome, pe, flags), str(tmp_path), env=DEVICE_ENV)
    assert "SAM formatted on the device" in log, log[-1500:]
    assert "head start taken" in log, log[-1500:]
    assert_same_text(open(tmp_path / "o.sam", "rb").read(), golden_bytes(fixture, f"{tag}.m{m}.sam.gz"), f"{fixture}/{tag}.m{m}")


def test_plain_records_unchanged(golden_tmp, tmp_path):
    """a job with none of the new fields: the plain run's bytes, as before"""
    log = run(align_args(golden_tmp, tmp_path, 6, "basic", None, ["-s3"]), str(tmp_path), env=DEVICE_ENV)
    assert "SAM formatted on the device" in log, log[-1500:]
    assert open(tmp_path / "o.sam", "rb").read() == golden_bytes("basic", "s3.m6.sam.gz")


@pytest.mark.parametrize("fixture,tag,flags", [("basic", "s3x5", ["-s3", "-x5"]), ("multi", "r5R5x4", ["-s3", "-r5", "-R5", "-x4"])])
def test_device_declines_and_the_host_formats(golden_tmp, tmp_path, fixture, tag, flags):
    """BK_SAM_DEVICE_FAIL=1: the device gives the job back after its head start; the host threads write the same file"""
    log = run(align_args(golden_tmp, tmp_path, 6, fixture, None, flags), str(tmp_path), env=dict(DEVICE_ENV, BK_SAM_DEVICE_FAIL="1"))
    assert "device SAM formatter declined" in log and "host threads format" in log, log[-1500:]
    assert "SAM formatted on the device" not in log
    assert_same_text(open(tmp_path / "o.sam", "rb").read(), golden_bytes(fixture, f"{tag}.m6.sam.gz"), tag)


# ---- the C ABI, without the command line in between ---------------------------------------------------------------
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def read_store(seqs):
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    offs = np.zeros(len(seqs), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1])
    bases = np.array([CODE[c] for s in seqs for c in s], dtype=np.uint8)
    return bases, offs, lens


def hit(chrom_id, loci, length, strand, nar=1):
    h = np.zeros(1, dtype=HIT_DTYPE)
    h["chrom_id"], h["match_loci"], h["match_len"], h["strand"], h["nar"] = chrom_id, loci, length, ord(strand), nar
    h["num_hits"] = 1 if nar == 1 else 0
    return h[0]


def seg(loci=0, length=0, flags=0):
    g = np.zeros(1, dtype=SEG2_DTYPE)
    g["match_loci"], g["match_len"], g["flags"] = loci, length, flags
    return g[0]


@pytest.fixture
def aligner(golden_tmp):
    with bk.Aligner(os.path.join(golden_tmp["basic"], "genome.sfx"), bk.AlignParams(max_subs=3)) as al:
        yield al, al.entries()[0]["name"].decode()


A20 = "AACCGGTTAAAAAAAAAAAC"
A20_RC = "GTTTTTTTTTTTAACCGGTT"
B20 = "ACGTTGCAACGGTTCCAAGT"
B20_RC = "ACTTGGAACCGTTGCAACGT"


def test_abi_hand_made_records(aligner):
    """clips on both strands, an insert, a deletion, a junction behind a clip, a read without alignment: POS = AdjStartLoci, the clips
    swap on '-', the second segment follows the 3' clip (CAligner::ReportBAMread, Aligner.cpp:5960-6033)"""
    al, chrom = aligner
    assert A20_RC == "".join("ACGT"["TGCA".index(c)] for c in reversed(A20)) and B20_RC == "".join("ACGT"["TGCA".index(c)] for c in reversed(B20))
    bases, offs, lens = read_store([B20, A20, B20, A20, B20, A20])
    names = [b"plus_clips", b"minus_clips", b"insert", b"deletion", b"junction", b"nohit"]
    hits = np.array([hit(1, 99, 20, "+"), hit(1, 199, 20, "-"), hit(1, 299, 8, "+"), hit(1, 399, 12, "-"), hit(1, 499, 10, "+"), hit(0, 0, 0, "?", nar=3)])
    left = np.array([3, 3, 0, 0, 2, 0], dtype=np.uint16)
    right = np.array([2, 2, 0, 0, 0, 0], dtype=np.uint16)
    seg2 = np.array([seg(), seg(), seg(0, 9, 3), seg(399 + 12 + 5, 8, 1), seg(499 + 10 + 1000, 10, 4), seg()])
    text = al.sam_format(bases, offs, lens, names, hits, [4, 2, 0, 5, 1, 3], seg2=seg2, trim_left=left, trim_right=right)
    exp = [f"junction\t0\t{chrom}\t502\t255\t2S8M1000N10M\t*\t0\t0\t{B20}\t*",
           f"insert\t0\t{chrom}\t300\t255\t8M3I9M\t*\t0\t0\t{B20}\t*",
           f"plus_clips\t0\t{chrom}\t103\t255\t3S15M2S\t*\t0\t0\t{B20}\t*",
           f"nohit\t4\t*\t0\t255\t20M\t*\t0\t0\t{A20}\t*\t\tYU:Z:NL",
           f"minus_clips\t16\t{chrom}\t202\t255\t2S15M3S\t*\t0\t0\t{A20_RC}\t*",
           f"deletion\t16\t{chrom}\t400\t255\t12M5D8M\t*\t0\t0\t{A20_RC}\t*"]
    assert text.decode().split("\n") == exp + [""]
    # the same records without the new arrays are plain lines
    plain = al.sam_format(bases, offs, lens, names, hits, [0, 1])
    assert plain.decode().split("\n") == [f"plus_clips\t0\t{chrom}\t100\t255\t20M\t*\t0\t0\t{B20}\t*",
                                          f"minus_clips\t16\t{chrom}\t200\t255\t20M\t*\t0\t0\t{A20_RC}\t*", ""]


def test_abi_records_of_one_read(aligner):
    """a -r5-shaped job, three records of two reads: name, bases and seg2 come from read src[i]; hit, trims and order go by record"""
    al, chrom = aligner
    bases, offs, lens = read_store([A20, B20])
    names = [b"ra", b"rb"]
    hits = np.array([hit(1, 10, 20, "+"), hit(1, 50, 8, "+"), hit(1, 70, 20, "-")])
    src = [1, 0, 1]
    seg2 = np.array([seg(0, 9, 3), seg()])                       # by read: read 0 has an insert
    left = np.array([1, 0, 0], dtype=np.uint16)                  # by record
    right = np.array([0, 0, 4], dtype=np.uint16)
    text = al.sam_format(bases, offs, lens, names, hits, [2, 0, 1], src=src, seg2=seg2, trim_left=left, trim_right=right)
    exp = [f"rb\t16\t{chrom}\t75\t255\t4S16M\t*\t0\t0\t{B20_RC}\t*",
           f"rb\t0\t{chrom}\t12\t255\t1S19M\t*\t0\t0\t{B20}\t*",
           f"ra\t0\t{chrom}\t51\t255\t8M3I9M\t*\t0\t0\t{A20}\t*"]
    assert text.decode().split("\n") == exp + [""]


def test_abi_src_with_paired_ends_is_refused(aligner):
    """the reference refuses -r with -U: BK_ERR_PARAMS; so is a record that names a read the store does not hold"""
    al, _ = aligner
    bases, offs, lens = read_store([A20, B20])
    hits = np.array([hit(1, 10, 20, "+"), hit(1, 50, 20, "+")])
    with pytest.raises(BkError) as e:
        al.sam_format(bases, offs, lens, [b"ra", b"rb"], hits, [0, 1], pe_mode=3, src=[0, 1])
    assert e.value.rc == -100
    with pytest.raises(BkError) as e:
        al.sam_format(bases, offs, lens, [b"ra", b"rb"], hits, [0, 1], src=[0, 2])
    assert e.value.rc == -100
