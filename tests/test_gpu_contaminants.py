"""`biokanga align -H` on the GPU: the device matcher (bk_contam_*, csrc/bk_contam.hip) against the Python statement of the rule
(contam_rule.py, itself held to the reference's runs by test_host_contaminants.py), and the command line against the reference's files
of tests/golden/contam - SAM byte for byte, NAR summary and contaminant count lines."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import biokanga_amd as bk
import contam_rule as cr
import helpers

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}


def codes(seq):
    return np.array([CODE[c] for c in cr.norm(seq)], dtype=np.uint8)


def matcher(ents):
    return bk.ContamMatcher([(codes(s), u) for u, s in ents])


def pack(reads):
    lens = np.array([len(r) for r in reads], dtype=np.uint32)
    offs = np.concatenate(([0], np.cumsum(lens[:-1], dtype=np.uint64))).astype(np.uint64)
    return np.concatenate([codes(r) for r in reads]), offs, lens


@pytest.mark.parametrize("tag", sorted(cr.cases()))
def test_device_cuts_equal_the_rule_on_the_golden_reads(tag):
    case = cr.cases()[tag]
    ents = cr.entries(os.path.join(cr.CONTAM, case["contaminants"]))
    t5, t3 = cr.flag_value(case["flags"], "-y", 0), cr.flag_value(case["flags"], "-Y", 0)
    with matcher(ents) as m:
        for e, key in enumerate(("reads", "mates")):
            if key not in case:
                continue
            p = os.path.join(cr.CONTAM, case[key] + ".gz")
            reads = [r[1] for r in (cr.read_fastq(p) if case[key].endswith(".fq") else cr.read_fasta(p))]
            bases, offs, lens = pack(reads)
            got = m.match(bases, offs, lens, all_pe2=e, trim5=t5, trim3=t3)
            exp = np.array([cr.cuts(r, ents, e == 1, t5, t3) for r in reads], dtype=np.uint16)
            assert np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0][:10]
            assert np.array_equal(m.match(bases, None, lens, all_pe2=e, trim5=t5, trim3=t3), exp)      # (reads back to back: no offsets)


@pytest.mark.parametrize("n_entries,trims", [(6, (0, 0)), (6, (2, 7)), (400, (1, 0))])
def test_device_cuts_equal_the_rule_on_random_reads(n_entries, trims):
    """lengths 15..2000, N-bearing reads, either PE2 flag per read; a set that lives in LDS and one that does not; entries with N"""
    rng = np.random.default_rng(777 + n_entries)
    ents, seen = [], set()
    while len(ents) < n_entries:
        s = "".join("ACGTN"[i] for i in rng.choice(5, int(rng.integers(4, 201)), p=[0.24, 0.24, 0.24, 0.24, 0.04]))
        u = int(rng.integers(1, 5))
        if (u, s) not in seen:
            seen.add((u, s))
            ents.append((u, s))
    reads = []
    for k in range(1500 if n_entries < 100 else 300):
        L = int(rng.integers(15, 2001)) if k % 3 else int(rng.integers(15, 120))
        r = list("ACGT"[i] for i in rng.integers(0, 4, L))
        for end in (0, 1):                          # most reads carry the end of some entry of the right kind, damaged or not
            u, s = ents[int(rng.integers(0, len(ents)))]
            k_ = min(int(rng.integers(1, len(s) + 1)), L // 2)
            part = list(s[len(s) - k_:] if u < 3 else s[:k_])
            for _ in range(int(rng.integers(0, 3))):
                part[int(rng.integers(0, k_))] = "ACGTN"[int(rng.integers(0, 5))]
            if rng.random() < 0.8:
                if u < 3:
                    r[:k_] = part
                else:
                    r[L - k_:] = part
        reads.append("".join(r))
    pe2 = rng.integers(0, 2, len(reads)).astype(np.uint8)
    bases, offs, lens = pack(reads)
    with matcher(ents) as m:
        got = m.match(bases, offs, lens, is_pe2=pe2, trim5=trims[0], trim3=trims[1])
    exp = np.array([cr.cuts(r, ents, bool(f), trims[0], trims[1]) for r, f in zip(reads, pe2)], dtype=np.uint16)
    assert np.array_equal(got, exp), np.nonzero((got != exp).any(axis=1))[0][:10]
    assert (exp > 1).any() and (exp[lens < 20] == 0).all()


def test_bad_arguments_are_parameter_errors():
    ok = [(codes("ACGTACGT"), 1)]
    for bad in ([(codes("ACG"), 1)], [(codes("A" * 201), 1)], [(codes("ACGTACGT"), 5)], [(np.array([0, 1, 2, 7], dtype=np.uint8), 1)], []):
        with pytest.raises(bk.BkError) as e:
            bk.ContamMatcher(bad)
        assert e.value.rc == -100
    with bk.ContamMatcher(ok) as m:
        bases, offs, lens = pack(["ACGT" * 10])
        for kw in (dict(trim5=-1), dict(trim3=-1), dict(all_pe2=2)):
            with pytest.raises(bk.BkError) as e:
                m.match(bases, offs, lens, **kw)
            assert e.value.rc == -100
        assert m.match(bases, offs, lens).shape == (1, 2)


def run_cli(args, cwd, ok=True, env=None):
    r = subprocess.run([BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900,
                       env=None if env is None else dict(os.environ, **env))
    assert (r.returncode == 0) == ok, r.stdout[-3000:]
    return r.stdout


def unz(name, tmp_path):
    dst = str(tmp_path / name)
    helpers.gunzip_to(os.path.join(cr.CONTAM, name + ".gz"), dst)
    return dst


@pytest.mark.parametrize("tag", sorted(cr.cases()))
@pytest.mark.parametrize("threads", ["-T1", "-T8"])
def test_align_with_contaminants_writes_the_reference_sam(golden_tmp, tmp_path, tag, threads):
    """-T1: the record-by-record loaders, -T8: the whole-file ones"""
    case = cr.cases()[tag]
    sfx = os.path.join(golden_tmp["basic"], "genome.sfx")
    out = str(tmp_path / "o.sam")
    args = ["align", "-i", unz(case["reads"], tmp_path), "-I", sfx, "-o", out, "-M6", threads, "-H", os.path.join(cr.CONTAM, case["contaminants"])]
    if "mates" in case:
        args += ["-u", unz(case["mates"], tmp_path)]
    log = run_cli(args + case["flags"], str(tmp_path))
    assert open(out, "rb").read() == gzip.open(os.path.join(cr.CONTAM, tag + ".m6.sam.gz"), "rb").read()
    for line in open(os.path.join(cr.CONTAM, tag + ".nar.txt")).read().splitlines():
        if line.strip():
            assert line.strip() in log
    msgs = [l.split("](biokanga) ", 1)[-1] for l in log.splitlines()]
    assert [m for m in msgs if "contaminate trimmed" in m or "contaminant trimmed" in m] == open(os.path.join(cr.CONTAM, tag + ".contam.txt")).read().splitlines()
    assert f"Contaminant sequences file: '{os.path.join(cr.CONTAM, case['contaminants'])}'" in log


def test_gzip_input_gives_the_golden_run(golden_tmp, tmp_path):
    """the reads from their .gz file, the option by its long name (-#2 sampling: the se13n2 case of the golden runs above)"""
    case = cr.cases()["se13"]
    out = str(tmp_path / "o.sam")
    run_cli(["align", "-i", os.path.join(cr.CONTAM, "reads.fa.gz"), "-I", os.path.join(golden_tmp["basic"], "genome.sfx"), "-o", out, "-M6", "-T8",
             "--contaminants", os.path.join(cr.CONTAM, case["contaminants"])] + case["flags"], str(tmp_path))
    assert open(out, "rb").read() == gzip.open(os.path.join(cr.CONTAM, "se13.m6.sam.gz"), "rb").read()


def test_align_without_contaminants_is_unchanged(golden_tmp, tmp_path):
    d = golden_tmp["basic"]
    out = str(tmp_path / "o.sam")
    log = run_cli(["align", "-i", os.path.join(d, "reads.fa"), "-I", os.path.join(d, "genome.sfx"), "-o", out, "-M6", "-s3"], str(tmp_path))
    assert open(out, "rb").read() == gzip.open(os.path.join(helpers.GOLDEN, "basic", "s3.m6.sam.gz"), "rb").read()
    assert "ontamina" not in log


@pytest.mark.parametrize("text", [">v&12\nACGTACGTACGTACGTACGTACGTACGT\n", ">a@1\nACG\n"])
def test_refused_contaminants_files_end_the_run(golden_tmp, tmp_path, text):
    d = golden_tmp["basic"]
    bad = str(tmp_path / "bad.fa")
    open(bad, "w").write(text)
    log = run_cli(["align", "-i", os.path.join(d, "reads.fa"), "-I", os.path.join(d, "genome.sfx"), "-o", str(tmp_path / "o.sam"), "-H", bad], str(tmp_path), ok=False)
    assert "Unable to load contaminate sequences file" in log


@pytest.mark.parametrize("paired", [False, True])
def test_whole_file_loaders_equal_the_record_loops(golden_tmp, tmp_path, paired):
    """files large enough for the all-thread parse (-T8) against the record-by-record loops (-T1): same SAM, same count lines (that -T8
    takes accept_chunks / accept_pairs on such files is asserted where the loaders' own count is visible: tests/test_host_contam_loader.py)"""
    case = cr.cases()["pe24" if paired else "se13y3Y5"]
    files = []
    for key in ("reads", "mates") if paired else ("reads",):
        text = gzip.open(os.path.join(cr.CONTAM, case[key] + ".gz"), "rb").read()
        p = str(tmp_path / case[key])
        open(p, "wb").write(text * 24)
        assert os.path.getsize(p) > (2 << 20)
        files.append(p)
    res = []
    for T in ("-T1", "-T8"):
        out = str(tmp_path / f"o{T}.sam")
        args = ["align", "-i", files[0], "-I", os.path.join(golden_tmp["basic"], "genome.sfx"), "-o", out, "-M6", T, "-H", os.path.join(cr.CONTAM, case["contaminants"])]
        log = run_cli(args + (["-u", files[1]] if paired else []) + case["flags"], str(tmp_path))
        res.append((open(out, "rb").read(), [l.split("](biokanga) ", 1)[-1] for l in log.splitlines() if "contaminate trimmed" in l or "contaminant trimmed" in l]))
    assert res[0] == res[1] and len(res[0][1]) == (4 if paired else 2)


@pytest.mark.parametrize("tag", ["se13y3Y5", "pe24", "se13n2"])
@pytest.mark.parametrize("threads", ["-T1", "-T8"])
def test_reload_after_a_declined_device_sam_pass_replays_the_cuts(golden_tmp, tmp_path, tag, threads):
    """the device takes the reads for its SAM records, the store's bases are given back, then the device declines (forced): the reads are
    loaded again with the cuts the first load kept - the reference's file, nothing matched twice (no second pair of count lines' worth of
    matcher work: the matcher is gone by then)"""
    case = cr.cases()[tag]
    out = str(tmp_path / "o.sam")
    args = ["align", "-i", unz(case["reads"], tmp_path), "-I", os.path.join(golden_tmp["basic"], "genome.sfx"), "-o", out, "-M6", threads,
            "-H", os.path.join(cr.CONTAM, case["contaminants"])]
    if "mates" in case:
        args += ["-u", unz(case["mates"], tmp_path)]
    log = run_cli(args + case["flags"], str(tmp_path), env={"BK_SAM_DEVICE_MIN": "1", "BK_SAM_EARLY_MIN": "1", "BK_SAM_DEVICE_FAIL": "1"})
    assert "loading the reads again" in log, log[-2000:]
    assert open(out, "rb").read() == gzip.open(os.path.join(cr.CONTAM, tag + ".m6.sam.gz"), "rb").read()
    msgs = [l.split("](biokanga) ", 1)[-1] for l in log.splitlines()]
    want = open(os.path.join(cr.CONTAM, tag + ".contam.txt")).read().splitlines()
    assert [m for m in msgs if "contaminate trimmed" in m or "contaminant trimmed" in m] == want + want      # (either load prints its counts)
