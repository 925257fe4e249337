"""5' primer artefact correction on the GPU (`align -6`; CAligner::PCR5PrimerCorrect): bk_primer_correct and its device form against the
plain restatement of primer_ref.py over the golden genome - random requests, every locus around both ends of every sequence, every
mismatch count against every limit, read N and target N and lower-case windows, both index images, sparse EntryIDs, bad requests - and
the command line against what the reference binary wrote, byte for byte (tests/golden/primer)."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import helpers
import primer_ref as pr

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
COUNTS = re.compile(r"Completed PCR 5' primer correction, (\d+) reads with (\d+) bases corrected, (\d+) reads with excessive substitutions rejected")
N_AT, N_LEN, LOWER = 8000, 20, (5000, 5400)          # the N run of pcB, the lower-case stretch of pcA (make_golden_primer.py)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("primer")
    return {n: helpers.gunzip_to(os.path.join(pr.DIR, n + ".gz"), str(d / n)) for n in ("genome.sfx", "reads.fa", "reads_1.fa", "reads_2.fa")}


@pytest.fixture(scope="module")
def genome():
    g = pr.Genome()
    assert "N" * N_LEN in g.text[1] and g.text[0][LOWER[0]:LOWER[1]].islower()
    return g


def make_requests(g, ids=(1, 2, 3)):
    """about 4 000 random requests - the read's window a copy of the target's with 0..6 bases changed (to N among others), or random -
    then every locus within 20 bases of both ends of every sequence on both strands, low_mm 0..12 against max_mms 0..12 on one window,
    and windows over the N run and the lower-case stretch"""
    rng = np.random.default_rng(66)
    rows = []

    def one(c, loci, ln, strand, low_mm, mms, how):
        t = pr.window(g, c, loci, ln, strand)
        if how == "random":
            r = [int(x) for x in rng.integers(0, 5, pr.KLEN)]
        else:
            r = list(t)
            for k in rng.choice(pr.KLEN, how, replace=False):
                r[k] = int((r[k] + rng.integers(1, 5)) % 5)
        rows.append((pr.pack_codes(r), c, loci, ln, ord(strand), low_mm, mms, 0))

    for _ in range(4000):
        c = ids[int(rng.integers(0, len(ids)))]
        ln = int(rng.choice([12, 13, 50, 60, 75, 100, 500]))
        loci = int(rng.integers(0, g.length(c) - ln + 1))
        one(c, loci, ln, "+-"[int(rng.integers(0, 2))], int(rng.integers(0, 13)), int(rng.integers(0, 8)),
            "random" if rng.random() < 0.2 else int(rng.integers(0, 7)))
    for c in ids:
        cl = g.length(c)
        for ln in (12, 50):
            for loci in list(range(0, 21)) + list(range(cl - ln - 20, cl - ln + 1)):
                for strand in "+-":
                    one(c, loci, ln, strand, 4, 1, 4)
    c = ids[0]
    for low_mm in range(0, 13):
        for mms in range(0, 13):
            one(c, 1234, 60, "+-"[(low_mm + mms) & 1], low_mm, mms, min(low_mm, 6))
    for d in range(-14, N_LEN + 3):                  # windows over the N run: target N into the read, N on N
        one(ids[1], N_AT + d, 60, "+", 4, 1, 4)
        one(ids[1], N_AT + d - 48, 60, "-", 4, 1, 4)
    for d in range(0, 40):                           # .. and inside the lower-case stretch: plain codes
        one(ids[0], LOWER[0] + 7 * d, 75, "+-"[d & 1], 4, 2, 3)
    reqs = np.zeros(len(rows), dtype=pr.PRIMER_REQ_DTYPE)
    for i, row in enumerate(rows):
        reqs[i] = row[:7] + ((0, 0, 0),)
    return reqs


@pytest.fixture(scope="module")
def requests(genome):
    return make_requests(genome)


@pytest.fixture(scope="module")
def expected(genome, requests):
    exp = pr.ref_primer(genome, requests)
    st = exp["status"]
    # what the requests were made to reach is there
    assert (st == pr.UNTOUCHED).sum() > 300 and (st == pr.CORRECTED).sum() > 1000 and (st == pr.REJECTED).sum() > 300 and not (st == pr.BAD).any()
    codes = np.array([pr.unpack_codes(v) for v in exp["codes"]])
    fixed = np.array([[m >> k & 1 for k in range(pr.KLEN)] for m in exp["mask"]], dtype=bool)
    assert (codes[fixed] == 4).sum() > 20                                   # a target N written into a read
    before = np.array([pr.unpack_codes(v) for v in requests["codes"]])
    assert (before[fixed] == 4).sum() > 100                                 # a read N corrected
    later = np.array([pr.window(genome, int(r["chrom_id"]), int(r["match_loci"]), int(r["match_len"]), chr(int(r["strand"]))) for r in requests])
    stays = (codes != later) & ~fixed & (st == pr.CORRECTED)[:, None]
    assert stays.any(axis=1).sum() > 100                                    # mismatches behind the one that got the count there stay
    return exp


def _bk():
    import biokanga_amd as bk
    return bk


def _aligner(path, flags=0):
    bk = _bk()
    return bk.Aligner(path, bk.AlignParams(max_subs=3), flags=flags)


def _device_call(al, reqs):
    import torch
    d_reqs = torch.from_numpy(np.ascontiguousarray(reqs).view(np.uint8).copy()).to("cuda")
    d_out = torch.full((max(len(reqs), 1) * pr.PRIMER_RES_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    al.primer_correct_device(d_reqs.data_ptr(), len(reqs), d_out.data_ptr(), sync=True)
    return d_out.cpu().numpy()[:len(reqs) * pr.PRIMER_RES_DTYPE.itemsize].view(pr.PRIMER_RES_DTYPE)


def _check(got, exp):
    for f in ("status", "mismatches", "n_corrected", "mask", "codes"):
        bad = np.flatnonzero(got[f] != exp[f])
        assert len(bad) == 0, (f, bad[:5], got[bad[:5]], exp[bad[:5]])


def test_binding_layouts_are_the_headers():
    bk = _bk()
    from biokanga_amd import binding
    assert binding.PRIMER_REQ_DTYPE == pr.PRIMER_REQ_DTYPE and binding.PRIMER_RES_DTYPE == pr.PRIMER_RES_DTYPE
    assert "bk_primer_correct" in binding.EXPORTED_SYMBOLS and "bk_primer_correct_device" in binding.EXPORTED_SYMBOLS
    assert bk.AlignParams(max_subs=4, orphan_core_subs=0).orphan_core_subs1 == 1 and bk.AlignParams(max_subs=4).orphan_core_subs1 == 0


@pytest.mark.parametrize("image", ["full", "lean"])
def test_results_equal_the_restatement(files, requests, expected, image):
    """through the host-buffer and the device-buffer entry point, on both index images: the step reads the target and the entry table only"""
    bk = _bk()
    with _aligner(files["genome.sfx"], bk.CTX_LEAN_IMAGE if image == "lean" else 0) as al:
        _check(al.primer_correct(requests), expected)
        _check(_device_call(al, requests), expected)


def test_sizes_chunks_and_no_buffer_before_the_first_call(files, requests, expected):
    """n = 0, n = 1, one more than a staging chunk, several chunks with a last partial one; the staging is made by the first call that
    has requests - a context that never corrects holds none"""
    bk = _bk()
    with _aligner(files["genome.sfx"]) as al:
        names, bases, offs, lens = helpers.read_fasta_reads(files["reads.fa"])
        al.align(bases, offs[:200], lens[:200])
        assert al.tune("primer_buf_bytes", 0) == 0
        assert len(al.primer_correct(requests[:0])) == 0
        al.primer_correct_device(0, 0, 0)
        assert al.tune("primer_buf_bytes", 0) == 0
        _check(al.primer_correct(requests[:1]), expected[:1])
        assert al.tune("primer_buf_bytes", 0) == 40
        _check(_device_call(al, requests[:1]), expected[:1])
        old = al.tune("primer_chunk", 1000)
        assert old == 8 << 20
        _check(al.primer_correct(requests[:1001]), expected[:1001])
        _check(al.primer_correct(requests), expected)
        assert al.tune("primer_buf_bytes", 0) == 1000 * 40
        al.tune("primer_chunk", old)
        _check(al.primer_correct(requests), expected)


def test_bad_requests(files, genome, requests):
    """the host entry point refuses them before anything is launched (the results stay as they were); the device entry point cannot look:
    such a request comes back flagged, nothing fetched, its neighbours served"""
    bk = _bk()
    base = requests[:8].copy()
    base["match_len"], base["match_loci"] = 60, 100
    bad = []
    for field, value in (("chrom_id", 0), ("chrom_id", 4), ("chrom_id", 0xffffffff), ("strand", ord("x")), ("strand", 0), ("match_len", 11), ("match_len", 0),
                         ("match_loci", genome.length(int(base["chrom_id"][5])) - 59), ("match_loci", 0xffffffff), ("match_loci", 0xffffffc8)):
        r = base.copy()
        r[field][5] = value
        bad.append(r)
    with _aligner(files["genome.sfx"]) as al:
        good = pr.ref_primer(genome, base)
        for r in bad:
            with pytest.raises(bk.BkError) as e:
                al.primer_correct(r)
            assert e.value.rc == -100
            assert al.tune("primer_buf_bytes", 0) == 0                       # nothing was even staged
            got, exp = _device_call(al, r), pr.ref_primer(genome, r)
            assert exp["status"][5] == pr.BAD
            _check(got, exp)
            _check(got[:5], good[:5])
        _check(al.primer_correct(base), good)
        with pytest.raises(bk.BkError):
            al.primer_correct_device(8, 1, 8)                                # misaligned result pointer


def test_sparse_entry_ids(files):
    """ids (7, 3, 12) instead of (1, 2, 3): the kernel and the host checks go through the id map"""
    import torch
    bk = _bk()
    ids = [7, 3, 12]
    g = pr.Genome(ids=ids)
    reqs = make_requests(g, ids=tuple(ids))[:3000]
    exp = pr.ref_primer(g, reqs)
    img = np.fromfile(files["genome.sfx"], dtype=np.uint8)
    blk = struct.unpack_from("<Q", img, 44)[0]
    n = struct.unpack_from("<Q", img, blk + 8)[0]
    seq = img[blk + 20: blk + 20 + n].copy()
    sa = img[blk + 20 + n: blk + 20 + 5 * n].view("<u4").copy()
    with _aligner(files["genome.sfx"]) as al:
        ents = al.entries()
    ents2 = ents.copy()
    ents2["entry_id"] = np.array([0] + ids, dtype=np.uint32)[ents["entry_id"]]
    dev = torch.device("cuda", 0)
    d_seq, d_sa = torch.from_numpy(seq).to(dev), torch.from_numpy(sa.view(np.int32)).to(dev)
    with bk.Aligner(None, bk.AlignParams(max_subs=3), d_seq=d_seq.data_ptr(), concat_len=int(n), d_sa=d_sa.data_ptr(), el_size=4, entries=ents2) as al2:
        _check(al2.primer_correct(reqs), exp)
        _check(_device_call(al2, reqs), exp)
        for unknown in (1, 2, 5, 13):
            r = reqs[:4].copy()
            r["chrom_id"][2] = unknown
            with pytest.raises(bk.BkError):
                al2.primer_correct(r)
            assert _device_call(al2, r)["status"][2] == pr.BAD


# ------------------------------------------------------------------------------------------------
# the command line

def run(args, cwd):
    r = subprocess.run(["timeout", "-k", "10", "120", BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _align(files, tmp_path, c, fmt, name, extra=()):
    out = str(tmp_path / name)
    args = ["align", "-I", files["genome.sfx"], "-o", out, fmt] + c["flags"] + list(extra)
    args += ["-i", files["reads_1.fa"], "-u", files["reads_2.fa"]] if c.get("pe") else ["-i", files["reads.fa"]]
    return out, run(args, str(tmp_path))


def _check_log(log, c):
    n = c["flags"][c["flags"].index("-6") + 1]
    assert f"correcting PCR 5' artefacts : {n}\n" in log
    assert [int(x) for x in COUNTS.search(log).groups()] == c["counts"]
    s = next(f[2:] for f in c["flags"] if f.startswith("-s"))
    assert f"Starting PCR 5' 12bp primer correction processing targeting substitution rate of {s} ..." in log


@pytest.mark.parametrize("tag", sorted(pr.cases()))
def test_cli_byte_identical(files, tmp_path, tag):
    """every run of cases.json: the -M6 SAM, and where the case lists more, BAM + BAI, the -M0 and -M3 CSV with the -O statistics, the SNP file"""
    c = pr.cases()[tag]
    if c.get("m6", True):
        out, log = _align(files, tmp_path, c, "-M6", "out.sam")
        _check_log(log, c)
        assert open(out, "rb").read() == pr.golden(f"{tag}.m6.sam.gz")
    for more in c.get("more", []):
        if more == "m5bam":
            out, log = _align(files, tmp_path, c, "-M5", "out.bam")
            assert open(out, "rb").read() == pr.golden(f"{tag}.m5.bam")
            assert open(out + ".bai", "rb").read() == pr.golden(f"{tag}.m5.bam.bai")
        elif more == "m0":
            out, log = _align(files, tmp_path, c, "-M0", "out.csv")
            assert open(out, "rb").read() == pr.golden(f"{tag}.m0.csv.gz")
        elif more == "m3stats":
            st = str(tmp_path / "stats.csv")
            out, log = _align(files, tmp_path, c, "-M3", "out3.csv", ["-O", st])
            assert open(out, "rb").read() == pr.golden(f"{tag}.m3.csv.gz")
            assert open(st, "rb").read() == pr.golden(f"{tag}.m3.stats.csv.gz")
        elif more == "snp":
            snp = str(tmp_path / "snp.csv")
            out, log = _align(files, tmp_path, c, "-M5", "out5.sam", ["-S", snp])
            assert open(out, "rb").read() == pr.golden(f"{tag}.m5.sam.gz")
            assert open(snp, "rb").read() == pr.golden(f"{tag}.snp.csv.gz")
        _check_log(log, c)


@pytest.mark.parametrize("tag", ["s2p3", "U3"])
def test_cli_device_formatter_sees_the_corrected_reads(files, tmp_path, tag):
    """the large-run machinery (the output file made ahead, SAM records formatted on the device), switched on for a small run: with -6
    the formatter is fed the corrected byte form; the rejected ends of pairs keep their paired FLAG bits there too"""
    c = pr.cases()[tag]
    out = str(tmp_path / "out.sam")
    env = dict(os.environ, BK_SAM_DEVICE_MIN="1", BK_TIMING="1")
    reads = ["-i", files["reads_1.fa"], "-u", files["reads_2.fa"]] if c.get("pe") else ["-i", files["reads.fa"]]
    r = subprocess.run(["timeout", "-k", "10", "120", BIN, "align", "-I", files["genome.sfx"], "-o", out, "-M6"] + reads + c["flags"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "SAM formatted on the device" in r.stdout, r.stdout[-3000:]
    assert open(out, "rb").read() == pr.golden(f"{tag}.m6.sam.gz")


def test_cli_without_the_option(files, tmp_path):
    """a run at the same rate without -6: the reference's output of that run, nothing said about primers and no correction launched"""
    c = {"flags": pr.spec()["bases"]["b_s5"]}
    env = dict(os.environ, BK_TIMING="1")
    out = str(tmp_path / "out.sam")
    r = subprocess.run(["timeout", "-k", "10", "120", BIN, "align", "-I", files["genome.sfx"], "-o", out, "-M6", "-i", files["reads.fa"]] + c["flags"], cwd=str(tmp_path),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == 0, r.stdout[-3000:]
    assert open(out, "rb").read() == pr.golden("b_s5.m6.sam.gz")
    assert "PCR 5'" not in r.stdout and "primer correction" not in r.stdout.lower()
