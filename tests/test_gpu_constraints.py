"""Loci base constraints on the GPU (`align -5`; CAligner::IdentifyConstraintViolations): bk_constraints_create / bk_constraints_check
against the restatement of constraints_ref.py over the golden genome - segments ending and beginning at the edges of every constraint
on both strands, second segments, trim offsets, read N and target N, nested and conflicting ranges, the first and last locus of a
sequence, both index images, every chunking, sparse EntryIDs, the limits, bad requests - and the command line against what the
reference binary wrote, byte for byte (tests/golden/constraints)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers
import constraints_ref as cr

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
CASES = cr.spec()["cases"]
NAMES, LENS = ["lcA", "lc,B", "lcC"], [28000, 18000, 10000]
DEFAULT_CHUNK = 4 << 20


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("constraints")
    return {n: helpers.gunzip_to(os.path.join(cr.DIR, n + ".gz"), str(d / n)) for n in ("genome.sfx", "many.sfx", "reads.fa", "reads_1.fa", "reads_2.fa", "main.csv")}


@pytest.fixture(scope="module")
def genome():
    return cr.Genome(os.path.join(cr.DIR, "genome.fa.gz"))


@pytest.fixture(scope="module")
def table(files):
    return cr.load_constraints(files["main.csv"], NAMES, LENS)


@pytest.fixture(scope="module")
def requests(genome, table):
    return cr.make_requests(genome, table)


@pytest.fixture(scope="module")
def expected(genome, table, requests):
    st = cr.ref_check(genome, table, *requests)
    assert (st == cr.UNTOUCHED).sum() > 500 and (st == cr.TOUCHED).sum() > 100 and (st == cr.VIOLATED).sum() > 200
    return st


def _bk():
    import biokanga_amd as bk
    return bk


def _aligner(path, flags=0):
    bk = _bk()
    return bk.Aligner(path, bk.AlignParams(max_subs=3), flags=flags)


def as_records(table):
    out = np.zeros(len(table), dtype=cr.CONSTRAINT_DTYPE)
    for i, (c, s, e, m) in enumerate(table):
        out[i] = (c, s, e, m, (0, 0, 0))
    return out


def _counts(st):
    return [int((st == k).sum()) for k in (cr.UNTOUCHED, cr.TOUCHED, cr.VIOLATED, cr.BAD)]


def _same(got, exp):
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (bad[:8], got[bad[:8]], exp[bad[:8]])


def test_binding_layouts_are_the_headers():
    from biokanga_amd import binding
    assert binding.CONSTRAINT_DTYPE == cr.CONSTRAINT_DTYPE and binding.CONSTRAINT_REQ_DTYPE == cr.CONSTRAINT_REQ_DTYPE
    assert (binding.CONSTRAINT_DTYPE.itemsize, binding.CONSTRAINT_SEG_DTYPE.itemsize, binding.CONSTRAINT_REQ_DTYPE.itemsize) == (16, 8, 32)
    hdr = open(os.path.join(helpers.ROOT, "include", "biokanga_amd.h")).read()
    for line in ("} bk_constraint;                 /* 16 bytes */", "} bk_constraint_seg;             /* 8 bytes */", "} bk_constraint_req;             /* 32 bytes */"):
        assert line in hdr
    assert (binding.MAX_CONSTRAINED_SEQS, binding.MAX_CONSTRAINTS) == (cr.MAX_CHROMS, cr.MAX_LOCI)
    assert (binding.CONSTRAINT_UNTOUCHED, binding.CONSTRAINT_TOUCHED, binding.CONSTRAINT_VIOLATED, binding.CONSTRAINT_BAD) == (cr.UNTOUCHED, cr.TOUCHED, cr.VIOLATED, cr.BAD)
    for sym in ("bk_constraints_create", "bk_constraints_destroy", "bk_constraints_check"):
        assert sym in binding.EXPORTED_SYMBOLS


@pytest.mark.parametrize("image", ["full", "lean"])
def test_statuses_equal_the_restatement(files, table, requests, expected, image):
    """on both index images - the check reads the 4-bit target and the entry table only - and in chunks of 64, 257 and the default; the
    constraints handed over in any order"""
    bk = _bk()
    reqs, bases = requests
    shuffled = as_records(table)[np.random.default_rng(1).permutation(len(table))]
    with _aligner(files["genome.sfx"], bk.CTX_LEAN_IMAGE if image == "lean" else 0) as al, al.constraints(shuffled) as cs:
        assert al.tune("constraint_chunk", 64) == DEFAULT_CHUNK
        for chunk in (64, 257, DEFAULT_CHUNK):
            al.tune("constraint_chunk", chunk)
            got, counts = cs.check(reqs, bases)
            _same(got, expected)
            assert counts == _counts(expected)


def test_sizes_and_where_the_touched_requests_lie(files, table, requests, expected):
    """n = 0; a batch nothing of which lies over a constraint and one everything of which does; a set without constraints; one touched
    request as the last of a chunk and of a wave, alone in its chunk"""
    reqs, bases = requests
    with _aligner(files["genome.sfx"]) as al, al.constraints(as_records(table)) as cs, al.constraints(as_records([])) as none:
        got, counts = cs.check(reqs[:0], bases)
        assert len(got) == 0 and counts == [0, 0, 0, 0]
        got, counts = cs.check(reqs[:0], bases[:0])
        assert counts == [0, 0, 0, 0]
        clear, over = reqs[expected == cr.UNTOUCHED], reqs[expected != cr.UNTOUCHED]
        got, counts = cs.check(clear, bases)
        assert not got.any() and counts == [len(clear), 0, 0, 0]
        got, counts = cs.check(over, bases)
        _same(got, expected[expected != cr.UNTOUCHED])
        assert counts[0] == 0 and counts[1] + counts[2] == len(over)
        got, counts = none.check(reqs, bases)
        assert not got.any() and counts == [len(reqs), 0, 0, 0]
        al.tune("constraint_chunk", 64)
        one = np.flatnonzero(expected == cr.VIOLATED)[0]
        for n, at in ((64, 63), (128, 127), (129, 128), (200, 64)):
            batch = np.concatenate([clear[:at], reqs[one:one + 1], clear[at:n - 1]])
            got, counts = cs.check(batch, bases)
            assert list(np.flatnonzero(got)) == [at] and got[at] == cr.VIOLATED and counts == [n - 1, 0, 1, 0]


def test_bad_requests(files, genome, table, requests, expected):
    """answered BAD with nothing read for them; their neighbours' answers stay"""
    reqs, bases = requests
    k = int(np.flatnonzero((expected == cr.TOUCHED) & (reqs["n_segs"] == 1))[0])
    clen = genome.length(int(reqs["chrom_id"][k]))
    edits = [("chrom_id", 0), ("chrom_id", 4), ("chrom_id", 0xffffffff), ("strand", ord("x")), ("strand", 0), ("n_segs", 0), ("n_segs", 3),
             ("start", clen - int(reqs["seg"]["len"][k, 0]) + 1), ("start", 0xffffffff), ("start", 0xfffffff0), ("read_idx", int(reqs["read_len"][k])), ("read_idx", 0xffff),
             ("len", int(reqs["read_len"][k]) + 1), ("read_ofs", len(bases)), ("read_ofs", len(bases) - int(reqs["read_len"][k]) + 1), ("read_ofs", 1 << 63), ("read_ofs", (1 << 64) - 1),
             ("seg2", None)]
    batch = np.concatenate([reqs[:100], reqs[k:k + 1]] * len(edits))
    exp = np.concatenate([expected[:100], expected[k:k + 1]] * len(edits))
    for j, (field, value) in enumerate(edits):
        at = 101 * j + 100
        if field in ("start", "len", "read_idx"):
            batch["seg"][field][at, 0] = value
        elif field == "seg2":                        # a second segment that leaves the sequence
            batch["n_segs"][at] = 2
            batch["seg"][at, 1] = (clen - 5, 6, 0)
        else:
            batch[field][at] = value
        exp[at] = cr.BAD
    assert np.array_equal(cr.ref_check(genome, table, batch, bases), exp)
    with _aligner(files["genome.sfx"]) as al, al.constraints(as_records(table)) as cs:
        for chunk in (64, DEFAULT_CHUNK):
            al.tune("constraint_chunk", chunk)
            got, counts = cs.check(batch, bases)
            _same(got, exp)
            assert counts[3] == len(edits)
        # the read of the last request ends with the bases: served
        last = reqs[k:k + 1].copy()
        last["read_ofs"] = len(bases) - int(last["read_len"][0])
        assert cs.check(last, bases)[0][0] != cr.BAD


def test_limits_and_refused_sets(files):
    """6400 constraints and 64 sequences are taken, one more of either is refused; so are constraints the loader would have refused"""
    bk = _bk()

    def refused(al, rows):
        with pytest.raises(bk.BkError) as e:
            al.constraints(as_records(rows))
        assert e.value.rc == -100

    with _aligner(files["genome.sfx"]) as al:
        al.constraints(as_records([(1, k, k + 5, 1 + k % 31) for k in range(cr.MAX_LOCI)])).close()
        refused(al, [(1, k, k + 5, 1) for k in range(cr.MAX_LOCI + 1)])
        for row in ((0, 1, 1, 1), (4, 1, 1, 1), (1, 5, 4, 1), (1, 5, 28000, 1), (2, 17999, 18000, 1), (1, 5, 5, 0), (1, 5, 5, 0x20), (0xffffffff, 1, 1, 1)):
            refused(al, [(1, 7, 7, 2), row])
        al.constraints(as_records([(1, 27999, 27999, 0x1f), (2, 0, 17999, 0x10)])).close()
    with _aligner(files["many.sfx"]) as al:
        assert al.num_entries == cr.MAX_CHROMS + 2
        with al.constraints(as_records([(k + 1, 5, 5, 1) for k in range(cr.MAX_CHROMS)] + [(3, 9, 9, 2)])) as cs:
            # .. and a full directory is searched to both of its ends
            reqs = np.zeros(4, dtype=cr.CONSTRAINT_REQ_DTYPE)
            for i, c in enumerate((1, cr.MAX_CHROMS, cr.MAX_CHROMS + 1, 3)):
                reqs[i] = (0, c, 20, ord("+"), 1, [(0, 20, 0), (0, 0, 0)])
            bases = np.full(20, 1, dtype=np.uint8)
            assert list(cs.check(reqs, bases)[0]) == [cr.VIOLATED, cr.VIOLATED, cr.UNTOUCHED, cr.VIOLATED]
            bases[9] = 0
            assert list(cs.check(reqs, bases)[0]) == [cr.VIOLATED, cr.VIOLATED, cr.UNTOUCHED, cr.VIOLATED]
            bases[5], bases[9] = 0, 1
            assert list(cs.check(reqs, bases)[0]) == [cr.TOUCHED, cr.TOUCHED, cr.UNTOUCHED, cr.TOUCHED]
        refused(al, [(k + 1, 5, 5, 1) for k in range(cr.MAX_CHROMS + 1)])


def test_a_full_table_of_nested_ranges(files, genome):
    """6400 constraints on one sequence, a few of them long ranges that keep the running maximum up over hundreds of short ones: the
    range of constraints a segment is given must hold every one that covers a locus of it"""
    rng = np.random.default_rng(64)
    rows = []
    for k in range(cr.MAX_LOCI):
        s = int(rng.integers(0, 27000))
        n = int(rng.integers(300, 900)) if k % 400 == 0 else int(rng.integers(1, 4))
        rows.append((1, s, min(27999, s + n - 1), int(rng.choice([0x10, 0x1f, 0x17, 0x1b, 0x0f, 0x1e]))))
    reqs, bases = cr.make_requests(genome, rows[::40], ids=(1,), seed=9, n_random=300)
    exp = cr.ref_check(genome, rows, reqs, bases)
    assert (exp == cr.VIOLATED).sum() > 100 and (exp == cr.TOUCHED).sum() > 100
    with _aligner(files["genome.sfx"]) as al, al.constraints(as_records(rows)) as cs:
        _same(cs.check(reqs, bases)[0], exp)


def test_sparse_entry_ids(files, table):
    """ids (7, 3, 12) instead of (1, 2, 3): the set, the kernels and the slice directory go by EntryID"""
    import torch
    bk = _bk()
    ids = [7, 3, 12]
    g = cr.Genome(os.path.join(cr.DIR, "genome.fa.gz"), ids=ids)
    tab = sorted((ids[c - 1], s, e, m) for c, s, e, m in table)
    reqs, bases = cr.make_requests(g, tab, ids=tuple(ids), n_random=800)
    exp = cr.ref_check(g, tab, reqs, bases)
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
        with al2.constraints(as_records(tab)) as cs:
            _same(cs.check(reqs, bases)[0], exp)
            for unknown in (1, 2, 5, 13):
                r = reqs[:4].copy()
                r["chrom_id"][2] = unknown
                assert cs.check(r, bases)[0][2] == cr.BAD
        with pytest.raises(bk.BkError):
            al2.constraints(as_records([(1, 5, 5, 1)]))


# ------------------------------------------------------------------------------------------------
# the command line

def run(args, cwd, env=None, rc=0):
    r = subprocess.run(["timeout", "-k", "10", "120", BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    assert r.returncode == rc, r.stdout[-3000:]
    return r.stdout


def _align(files, tmp_path, c, fmt, name, extra=(), with5=True, env=None):
    """(the constraints file is named as the generator named it: the name is in the log)"""
    if not os.path.exists(str(tmp_path / "main.csv")):
        os.symlink(files["main.csv"], str(tmp_path / "main.csv"))
    out = str(tmp_path / name)
    args = ["align", "-I", files["genome.sfx"], "-o", out, fmt] + c["flags"] + list(extra) + (["-5", "main.csv"] if with5 else [])
    args += ["-i", files["reads_1.fa"], "-u", files["reads_2.fa"]] if c.get("pe") else ["-i", files["reads.fa"]]
    return out, run(args, str(tmp_path), env=env)


def _check_log(log, c):
    kind = "PE" if c.get("pe") else "SE"
    assert "Loci base constraints file: 'main.csv'\n" in log
    assert "Loading loci base constraints from CSV file 'main.csv' ..." in log
    assert "Completed loading 20 loci base constraints for 3 target sequences from CSV file 'main.csv'" in log
    assert f"Identifying {kind} loci base constraint violations ..." in log
    assert f"Identified {c['identified']} {kind} loci base constraint violations" in log


@pytest.mark.parametrize("tag", sorted(CASES))
def test_cli_byte_identical(files, tmp_path, tag):
    """every run of cases.json: the -M6 SAM, and where the case lists more, BAM + BAI, the -M0 CSV, the -M5 SAM with the SNP file"""
    c = CASES[tag]
    if c.get("m6", True):
        out, log = _align(files, tmp_path, c, "-M6", "out.sam")
        _check_log(log, c)
        assert open(out, "rb").read() == cr.golden(f"{tag}.m6.sam.gz")
    for more in c.get("more", []):
        if more == "m5bam":
            out, log = _align(files, tmp_path, c, "-M5", "out.bam")
            assert open(out, "rb").read() == cr.golden(f"{tag}.m5.bam")
            assert open(out + ".bai", "rb").read() == cr.golden(f"{tag}.m5.bam.bai")
        elif more == "m0":
            out, log = _align(files, tmp_path, c, "-M0", "out.csv")
            assert open(out, "rb").read() == cr.golden(f"{tag}.m0.csv.gz")
        elif more == "snp":
            snp = str(tmp_path / "snp.csv")
            out, log = _align(files, tmp_path, c, "-M5", "out5.sam", ["-S", snp])
            assert open(out, "rb").read() == cr.golden(f"{tag}.m5.sam.gz")
            assert open(snp, "rb").read() == cr.golden(f"{tag}.snp.csv.gz")
        _check_log(log, c)


@pytest.mark.parametrize("tag", sorted(cr.spec()["errors"]))
def test_cli_refusals(files, tmp_path, tag):
    """every file the loader refuses: the reference's messages, its exit status, and no output file"""
    e = cr.spec()["errors"][tag]
    if tag != "e_missing":
        helpers.gunzip_to(os.path.join(cr.DIR, e["file"] + ".gz"), str(tmp_path / e["file"]))
    sfx = files["genome.sfx"] if e["index"] == "genome" else files["many.sfx"]
    log = run(["align", "-I", sfx, "-o", str(tmp_path / "out.sam"), "-M6", "-s3", "-i", files["reads.fa"], "-5", e["file"]], str(tmp_path), rc=e["exit"])
    lines = [ln.split("] ", 1)[-1] for ln in log.splitlines()]
    for m in e["messages"][-2:]:
        assert any(ln.endswith(m) for ln in lines), (m, log[-2000:])
    assert f"Exit code: {e['exit']}" in log and "Identifying" not in log


def test_cli_two_contexts_give_the_same_file(files, tmp_path):
    c = CASES["s3"]
    out, log = _align(files, tmp_path, c, "-M6", "two.sam", ["--devices", "0,0"])
    _check_log(log, c)
    assert open(out, "rb").read() == cr.golden("s3.m6.sam.gz")


@pytest.mark.parametrize("tag", ["s3", "U3"])
def test_cli_device_formatter_writes_the_marked_records(files, tmp_path, tag):
    """the large-run machinery (the output file made ahead, the formatter's head start, SAM records formatted on the device), switched on
    for a small run: -5 changes NARs behind the head start, as -k does, and the read store keeps its bases for the pass"""
    c = CASES[tag]
    env = dict(os.environ, BK_SAM_DEVICE_MIN="1", BK_TIMING="1")
    out, log = _align(files, tmp_path, c, "-M6", "out.sam", env=env)
    assert "SAM formatted on the device" in log, log[-3000:]
    assert "bk timing: loci constraints:" in log
    assert open(out, "rb").read() == cr.golden(f"{tag}.m6.sam.gz")


@pytest.mark.parametrize("tag", ["s3", "k"])
def test_cli_without_the_option(files, tmp_path, tag):
    """the run without -5: the reference's output of that run, nothing said about constraints and nothing of the pass launched"""
    out, log = _align(files, tmp_path, CASES[tag], "-M6", "out.sam", with5=False, env=dict(os.environ, BK_TIMING="1"))
    assert open(out, "rb").read() == cr.golden(f"{tag}.base.m6.sam.gz")
    for said in ("Loci base constraints file", "Loading loci base constraints", "loci base constraint violations", "bk timing: loci constraints"):
        assert said not in log
    assert "   0 (LC) Alignment violated loci base constraints" in log
