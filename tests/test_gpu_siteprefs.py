"""Start-site octamer preferences on the GPU (`align -8 / -9`; CAligner::ProcessSiteProbabilites): bk_site_octamers against a numpy
restatement of the reference's arithmetic over the golden genome's bases - random alignments, every locus around both ends of both
sequences, every image form - and the command line against what the reference binary wrote, byte for byte (tests/golden/siteprefs)."""
import os
import subprocess

import numpy as np
import pytest

import helpers
import siteprefs_ref as sr

pytestmark = pytest.mark.gpu
BIN = os.path.join(helpers.ROOT, "biokanga_amd", "bin", "biokanga")
OFFSETS = (-100, -4, 0, 7, 100)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("siteprefs")
    out = {}
    for n in ("genome.sfx", "reads.fa", "reads_1.fa", "reads_2.fa"):
        out[n] = helpers.gunzip_to(os.path.join(sr.DIR, n + ".gz"), str(d / n))
    return out


@pytest.fixture(scope="module")
def genome():
    return sr.Genome()


@pytest.fixture(scope="module")
def requests(genome):
    """4 096 random alignments, then every locus of the first and last 120 bases of either sequence on either strand, lengths 50 and 60"""
    rng = np.random.default_rng(8)
    n = 4096
    rnd = np.zeros(n, dtype=sr.SITE_REQ_DTYPE)
    rnd["chrom_id"] = rng.integers(1, 3, n)
    rnd["match_len"] = rng.choice([50, 60], n)
    rnd["match_loci"] = (rng.random(n) * (genome.lens[rnd["chrom_id"]] - rnd["match_len"] + 1)).astype(np.uint32)
    rnd["strand"] = rng.choice([ord("+"), ord("-")], n)
    rows = []
    for c in (1, 2):
        cl = int(genome.lens[c])
        for loci in list(range(120)) + list(range(cl - 120, cl)):
            for strand in "+-":
                for ln in (50, 60):
                    rows.append((c, loci, ln, ord(strand), 0))
    return np.concatenate([rnd, np.array(rows, dtype=sr.SITE_REQ_DTYPE)])


@pytest.fixture(scope="module")
def expected(genome, requests):
    return {ofs: sr.ref_octamers(genome, requests, ofs) for ofs in OFFSETS}


def _aligner(path):
    import biokanga_amd as bk
    return bk.Aligner(path, bk.AlignParams(max_subs=3))


def _device_call(al, reqs, ofs):
    import torch
    d_reqs = torch.from_numpy(np.ascontiguousarray(reqs).view(np.uint8).copy()).to("cuda")
    d_out = torch.full((len(reqs) * sr.SITE_RES_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
    al.site_octamers_device(d_reqs.data_ptr(), len(reqs), ofs, d_out.data_ptr(), sync=True)
    return d_out.cpu().numpy().view(sr.SITE_RES_DTYPE)


def _check(got, exp):
    assert np.array_equal(got["codes"], exp["codes"])
    assert np.array_equal(got["site"], exp["site"])


@pytest.mark.parametrize("wide", [0, 1])
def test_octamers_equal_the_restatement(files, requests, expected, wide):
    """codes, the nothing-fetched flag and the site, through the host-buffer and the device-buffer entry point; the same on a context whose
    k-mer table is forced wide: the step does not depend on the image's form"""
    with _aligner(files["genome.sfx"]) as al:
        if wide:
            al.tune("ktab_wide", 1)
        for ofs in OFFSETS:
            exp = expected[ofs]
            # a site leaves its sequence only by wrapping below 0: loci + ofs < 0 on '+', loci + len - 8 - ofs < 0 on '-'
            assert (exp["codes"] & sr.NOTHING).any() == (ofs in (-100, -4, 100))
            _check(al.site_octamers(requests, ofs), exp)
            _check(_device_call(al, requests, ofs), exp)


def test_sizes_and_chunks(files, genome, requests, expected):
    """n = 0, n = 1, one more than a chunk, several chunks with a last partial one"""
    with _aligner(files["genome.sfx"]) as al:
        assert len(al.site_octamers(requests[:0], -4)) == 0
        al.site_octamers_device(0, 0, -4, 0)
        _check(al.site_octamers(requests[:1], -4), expected[-4][:1])
        _check(_device_call(al, requests[:1], -4), expected[-4][:1])
        old = al.tune("site_chunk", 1000)
        assert old == 8 << 20
        _check(al.site_octamers(requests[:1001], 7), expected[7][:1001])
        _check(al.site_octamers(requests, -100), expected[-100])
        al.tune("site_chunk", old)
        _check(al.site_octamers(requests, 100), expected[100])


def test_many_blocks(files, genome):
    """more requests than the 2048 blocks of 256 lanes: the grid-stride loop"""
    rng = np.random.default_rng(9)
    n = 2048 * 256 + 777
    reqs = np.zeros(n, dtype=sr.SITE_REQ_DTYPE)
    reqs["chrom_id"] = rng.integers(1, 3, n)
    reqs["match_len"] = 60
    reqs["match_loci"] = (rng.random(n) * (genome.lens[reqs["chrom_id"]] - 59)).astype(np.uint32)
    reqs["strand"] = rng.choice([ord("+"), ord("-")], n)
    exp = sr.ref_octamers(genome, reqs, -4)
    with _aligner(files["genome.sfx"]) as al:
        _check(al.site_octamers(reqs, -4), exp)
        _check(_device_call(al, reqs, -4), exp)


def test_bad_parameters_are_refused(files, requests):
    import biokanga_amd as bk
    with _aligner(files["genome.sfx"]) as al:
        for ofs in (-101, 101, 1 << 20):
            with pytest.raises(bk.BkError) as e:
                al.site_octamers(requests[:8], ofs)
            assert e.value.rc == -100
            with pytest.raises(bk.BkError) as e:
                al.site_octamers_device(0, 0, ofs, 0)
            assert e.value.rc == -100
        for bad in (0, 3, 0xffffffff):
            reqs = requests[:8].copy()
            reqs["chrom_id"][5] = bad
            with pytest.raises(bk.BkError) as e:
                al.site_octamers(reqs, -4)
            assert e.value.rc == -100
            # the device entry point cannot look at the requests: such a one comes back as "nothing fetched"
            got = _device_call(al, reqs, -4)
            assert got["codes"][5] == sr.NOTHING and (got["codes"][:5] != sr.NOTHING).all()
        reqs = requests[:8].copy()
        reqs["strand"][0] = ord("x")
        with pytest.raises(bk.BkError) as e:
            al.site_octamers(reqs, -4)
        assert e.value.rc == -100


def test_index_of_5_byte_elements(files, genome, requests, expected, tmp_path):
    seq, sa, ents = helpers.read_sfx(files["genome.sfx"])
    path = str(tmp_path / "genome5.sfx")
    helpers.write_sfx(path, "siteprefs5", ents, seq, sa.astype(np.uint64), el_size=5)
    with _aligner(path) as al:
        _check(al.site_octamers(requests[:4096], -4), expected[-4][:4096])
        _check(_device_call(al, requests[:4096], 7), expected[7][:4096])


# ------------------------------------------------------------------------------------------------
# the command line

def run(args, cwd):
    r = subprocess.run([BIN] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout


def _align(files, tmp_path, c, extra=(), prefs=True):
    out, table = str(tmp_path / ("out." + c["out"])), str(tmp_path / "prefs.csv")
    args = ["align", "-I", files["genome.sfx"], "-o", out] + c["flags"] + list(extra)
    args += ["-i", files["reads_1.fa"], "-u", files["reads_2.fa"]] if c.get("pe") else ["-i", files["reads.fa"]]
    if prefs:
        args += ["-8", table]
    log = run(args, str(tmp_path))
    return open(out, "rb").read(), (open(table, "rb").read() if prefs else None), log


def _golden_out(tag, c):
    return sr.golden("dflt.sam.gz" if tag.startswith("ofs") else f"{tag}.{c['out']}.gz")


@pytest.mark.parametrize("tag", sorted(sr.cases()))
def test_cli_byte_identical(files, tmp_path, tag):
    c = sr.cases()[tag]
    out, table, log = _align(files, tmp_path, c)
    assert table == sr.golden(f"{c['prefs']}.siteprefs.csv.gz")
    assert out == _golden_out(tag, c)
    assert f"Offset read start sites when processing site octamer preferencing: {c['ofs']}\n" in log
    at = [log.index(m) for m in ("Read nonalignment reason summary", "Processing for alignment site probabilities...",
                                 "Completed alignment site probabilities", "Reporting of aligned result set started...")]
    assert at == sorted(at)


def test_cli_two_pipelines_on_one_device(files, tmp_path):
    """--devices 0,0: the gather runs on the first context, once, over the whole sorted set"""
    c = sr.cases()["ofs7"]
    out, table, _ = _align(files, tmp_path, c, extra=["--devices", "0,0"])
    assert table == sr.golden("ofs7.siteprefs.csv.gz")
    assert out == sr.golden("dflt.sam.gz")


def test_cli_output_is_the_same_without_the_option(files, tmp_path):
    c = sr.cases()["dflt"]
    out, _, log = _align(files, tmp_path, c, prefs=False)
    assert out == sr.golden("dflt.sam.gz")
    assert "site probabilities" not in log and "site octamer" not in log
    # .. and the BED score column stays 0
    out, _, _ = _align(files, tmp_path, sr.cases()["m4"], prefs=False)
    assert all(l.split("\t")[4] == "0" for l in out.decode().splitlines()[1:])
