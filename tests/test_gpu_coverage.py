"""GPU tests of --coverage (per-base depth as a bedGraph, made on the device): bk_coverage_runs / bk_coverage_text on crafted requests
over small indexes of their own, and the command line on golden fixtures.  The reference throughout is the numpy statement of the rule
in tests/coverage_ref.py: the runs must be equal, the text byte for byte."""
import os

import numpy as np
import pytest

import biokanga_amd as bk
from biokanga_amd.binding import BkError, COV_REQ_DTYPE
import coverage_ref as cr
import helpers
import samtags_ref as sr
from test_gpu_cli import golden_bytes, run

pytestmark = pytest.mark.gpu

# the constants of bk_coverage.hip the boundaries below are placed by
COV_BLOCK = 256                      # kCovBlock: threads - requests of k_cov_mark, lines of the text kernels - per block
COV_WAVE = 64                        # positions a wave of k_cov_count / k_cov_emit looks at per step
COV_TILE = 2048                      # kCovTile: positions per wave
COV_BLOCK_SPAN = 4 * COV_TILE        # .. and per block of four waves
LENS = (3000, 2600, 2300)


def _write_fasta(path, seqs):
    with open(path, "w") as f:
        for name, text in seqs:
            f.write(f">{name}\n")
            for k in range(0, len(text), 70):
                f.write(text[k:k + 70] + "\n")


def _index(d, tag, names, lens, seed):
    rng = np.random.default_rng(seed)
    fa, sfx = str(d / f"{tag}.fa"), str(d / f"{tag}.sfx")
    _write_fasta(fa, [(nm, "".join("ACGT"[c] for c in rng.integers(0, 4, n))) for nm, n in zip(names, lens)])
    run(["index", "-i", fa, "-o", sfx, "-r", tag], str(d))
    g = sr.Genome(sfx)
    assert [g.names[i + 1] for i in range(len(names))] == list(names) and [g.length(i + 1) for i in range(len(names))] == list(lens)
    return sfx, {i: g.length(i) for i in g.names}, dict(g.names)


@pytest.fixture(scope="module")
def crafted(tmp_path_factory):
    """three sequences of 3000, 2600 and 2300 bases: with the position behind each they take 7903 positions of a slice"""
    sfx, lengths, names = _index(tmp_path_factory.mktemp("coverage"), "cov3", ("covA", "covB", "covC"), LENS, 20261020)
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        assert al.tune("coverage_buf_bytes", 0) == 0          # no call yet: nothing allocated
        yield al, lengths, names


@pytest.fixture(scope="module")
def long_one(tmp_path_factory):
    """one sequence of 20000 bases: more than two blocks' worth of positions"""
    sfx, lengths, names = _index(tmp_path_factory.mktemp("coverage1"), "cov1", ("covLong",), (20000,), 7)
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        yield al, lengths, names


def check(al, lengths, names, reqs, want_runs=None):
    """both calls against the reference -> (run counts per sink call, text bytes per sink call, text)"""
    reqs = np.ascontiguousarray(reqs, dtype=COV_REQ_DTYPE)
    exp_runs, exp_tot = cr.runs_of(reqs, lengths)
    exp_text = cr.text_of(exp_runs, names)
    if want_runs is not None:
        assert [tuple(int(x) for x in r) for r in exp_runs.tolist()] == want_runs
    runs, tot, run_parts = al.coverage_runs(reqs)
    print("runs", len(runs), "expected", len(exp_runs), "totals", tot, "expected", exp_tot)
    assert tot == exp_tot
    assert runs.tolist() == exp_runs.tolist()
    text, tot2, text_parts = al.coverage_text(reqs)
    assert tot2 == exp_tot
    assert text == exp_text
    return run_parts, text_parts, text


def tuned(al, **knobs):
    class T:
        def __enter__(self):
            self.old = {k: al.tune(k, v) for k, v in knobs.items()}

        def __exit__(self, *a):
            for k, v in self.old.items():
                al.tune(k, v)
    return T()


# ---- 1. basic shapes ------------------------------------------------------------------------------------------------
def test_nothing_held_before_the_first_call_and_empty_call(crafted):
    al, lengths, names = crafted
    runs, tot, parts = al.coverage_runs(np.zeros(0, dtype=COV_REQ_DTYPE))
    assert len(runs) == 0 and parts == [] and tot == dict(runs=0, covered=0, depth_sum=0, max_depth=0, flagged=0)
    text, tot, parts = al.coverage_text(np.zeros(0, dtype=COV_REQ_DTYPE))
    assert text == b"" and parts == [] and tot["runs"] == 0
    check(al, lengths, names, cr.make_reqs([(2, 17, 1)]), want_runs=[(2, 17, 18, 1)])          # one request of m = 1
    assert al.tune("coverage_buf_bytes", 0) > 0
    with pytest.raises(BkError):
        al.tune("coverage_slice_bases", -1)
    assert al.tune("coverage_slice_bases", 0) > sum(LENS) + 3       # derived by that call: this target is one slice (and derived again by the next)


def test_bad_arguments(crafted):
    al, lengths, names = crafted
    one = cr.make_reqs([(1, 0, 5)])
    from biokanga_amd.binding import _COV_RUN_SINK, _SAM_SINK
    import ctypes
    tot = (ctypes.c_uint64 * 5)()
    ok = lambda *a: 0
    assert al.lib.bk_coverage_runs(al.h, None, 1, _COV_RUN_SINK(ok), None, ctypes.byref(tot)) == -100
    assert al.lib.bk_coverage_text(al.h, None, 1, _SAM_SINK(ok), None, ctypes.byref(tot)) == -100
    assert al.lib.bk_coverage_runs(al.h, one.ctypes.data, 1, ctypes.cast(None, _COV_RUN_SINK), None, ctypes.byref(tot)) == -100
    assert al.lib.bk_coverage_text(al.h, one.ctypes.data, 1, ctypes.cast(None, _SAM_SINK), None, ctypes.byref(tot)) == -100
    assert al.lib.bk_coverage_runs(al.h, one.ctypes.data, 1 << 31, _COV_RUN_SINK(ok), None, ctypes.byref(tot)) == -100


def test_sequence_ends_abutting_nested_and_staggered(crafted):
    al, lengths, names = crafted
    A, B, C = LENS
    check(al, lengths, names, cr.make_reqs([(1, 0, 10), (1, A - 10, 10), (3, 0, 10), (3, C - 10, 10), (1, 0, 1), (3, C - 1, 1)]),
          want_runs=[(1, 0, 1, 2), (1, 1, 10, 1), (1, A - 10, A, 1), (3, 0, 10, 1), (3, C - 10, C - 1, 1), (3, C - 1, C, 2)])
    # the last base of a sequence and the first of the next at equal depth: two runs
    check(al, lengths, names, cr.make_reqs([(1, A - 30, 30), (2, 0, 30), (2, B - 5, 5), (3, 0, 5)]),
          want_runs=[(1, A - 30, A, 1), (2, 0, 30, 1), (2, B - 5, B, 1), (3, 0, 5, 1)])
    # [a, b) and [b, c): one run
    check(al, lengths, names, cr.make_reqs([(2, 100, 50), (2, 150, 70)]), want_runs=[(2, 100, 220, 1)])
    # nested, staggered
    check(al, lengths, names, cr.make_reqs([(2, 100, 100), (2, 120, 20), (2, 125, 5), (2, 300, 50), (2, 310, 50), (2, 320, 50)]),
          want_runs=[(2, 100, 120, 1), (2, 120, 125, 2), (2, 125, 130, 3), (2, 130, 140, 2), (2, 140, 200, 1),
                     (2, 300, 310, 1), (2, 310, 320, 2), (2, 320, 350, 3), (2, 350, 360, 2), (2, 360, 370, 1)])


@pytest.mark.parametrize("m", [63, 64, 65, 2000])
def test_run_lengths(crafted, m):
    al, lengths, names = crafted
    check(al, lengths, names, cr.make_reqs([(2, 5, m), (3, 64, m)]), want_runs=[(2, 5, 5 + m, 1), (3, 64, 64 + m, 1)])


# ---- 2. two-segment requests ----------------------------------------------------------------------------------------
def test_two_segment_requests(crafted):
    al, lengths, names = crafted
    check(al, lengths, names, cr.make_reqs([(2, 50, 60, 70, 900)]), want_runs=[(2, 50, 110, 1), (2, 1010, 1080, 1)])                 # N
    check(al, lengths, names, cr.make_reqs([(2, 300, 70, 66, 1), (3, 300, 64, 64, 20)]),                                            # D: the gap is not counted
          want_runs=[(2, 300, 370, 1), (2, 371, 437, 1), (3, 300, 364, 1), (3, 384, 448, 1)])
    check(al, lengths, names, cr.make_reqs([(2, 300, 70, 66, 0)]), want_runs=[(2, 300, 436, 1)])                                    # I: one unbroken run
    check(al, lengths, names, cr.make_reqs([(2, 300, 70, 66, 0), (2, 360, 20, 30, 5), (1, 2900, 50, 50, 0)]))


# ---- 3. deep pile-ups -----------------------------------------------------------------------------------------------
def test_ten_thousand_identical_requests(crafted):
    al, lengths, names = crafted
    _, _, text = check(al, lengths, names, cr.make_reqs([(2, 100, 50)] * 10000), want_runs=[(2, 100, 150, 10000)])
    assert text == b"covB\t100\t150\t10000\n"


def test_ten_thousand_requests_staggered_by_one_base(crafted):
    al, lengths, names = crafted
    check(al, lengths, names, cr.make_reqs([(1, k % 2900, 100) for k in range(10000)]))


# ---- 4. slicing and ordering ----------------------------------------------------------------------------------------
def random_reqs(n, seed):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        c = int(rng.integers(1, 4))
        L = LENS[c - 1]
        m = int(rng.integers(1, 151))
        if rng.integers(0, 4) == 0:
            m2, gap = int(rng.integers(1, 100)), int(rng.choice([0, 1, 7, 300]))
            rows.append((c, int(rng.integers(0, L - m - gap - m2 + 1)), m, m2, gap))
        else:
            rows.append((c, int(rng.integers(0, L - m + 1)), m))
    reqs = cr.make_reqs(rows)
    return reqs[np.lexsort((reqs["pos"], reqs["chrom_id"]))]


@pytest.fixture(scope="module")
def twenty_thousand():
    return random_reqs(20000, 5)


def shuffled(reqs):
    return reqs[np.random.default_rng(9).permutation(len(reqs))]


def test_sorted_and_shuffled_requests_give_the_same_output(crafted, twenty_thousand):
    al, lengths, names = crafted
    _, _, t1 = check(al, lengths, names, twenty_thousand)
    _, _, t2 = check(al, lengths, names, shuffled(twenty_thousand))
    assert t1 == t2
    with tuned(al, coverage_req_chunk=1000):               # the requests staged twenty times
        assert check(al, lengths, names, shuffled(twenty_thousand))[2] == t1


def test_every_sequence_its_own_slice(crafted, twenty_thousand):
    al, lengths, names = crafted
    with tuned(al, coverage_slice_bases=LENS[0] + 1):
        _, _, t1 = check(al, lengths, names, twenty_thousand)
        assert check(al, lengths, names, shuffled(twenty_thousand))[2] == t1
    assert check(al, lengths, names, twenty_thousand)[2] == t1


def test_slices_below_the_longest_sequence_and_chunks_of_64_runs(crafted, twenty_thousand):
    al, lengths, names = crafted
    with tuned(al, coverage_slice_bases=1000, coverage_run_chunk=64, coverage_req_chunk=7000):
        run_parts, text_parts, text = check(al, lengths, names, shuffled(twenty_thousand))
    n_runs = sum(run_parts)
    assert n_runs > 5000 and max(run_parts) == 64 and len(run_parts) >= n_runs // 64
    assert max(text_parts) == 16 * 64 and len(text_parts) > len(run_parts)
    at, straddling = 0, 0
    for n in text_parts[:-1]:
        at += n
        straddling += text[at - 1:at] != b"\n"
    assert straddling > len(text_parts) // 4               # lines lie across sink calls


def test_runs_across_every_tile_and_block_boundary(long_one):
    """a run that ends on, starts on and lies across every multiple of a wave's step near a tile boundary, of COV_TILE and of
    COV_BLOCK_SPAN; runs whose start and end lie tiles and blocks apart; neighbours of different depth on either side of a boundary"""
    al, lengths, names = long_one
    rows = []
    for b in (COV_WAVE, 2 * COV_WAVE, COV_TILE - COV_WAVE, COV_TILE, COV_TILE + COV_WAVE, 2 * COV_TILE, 3 * COV_TILE, COV_BLOCK_SPAN, COV_BLOCK_SPAN + COV_TILE,
              2 * COV_BLOCK_SPAN):
        rows += [(1, b - 3, 3), (1, b, 2), (1, b - 1, 2), (1, b - 1, 1)]          # ends on b, starts on b, across it, its last position alone
    rows += [(1, 10, 20000 - 20), (1, COV_TILE - 5, COV_BLOCK_SPAN), (1, COV_BLOCK_SPAN - 1, COV_BLOCK_SPAN + 2)]
    check(al, lengths, names, cr.make_reqs(rows))
    with tuned(al, coverage_run_chunk=3):
        run_parts, _, _ = check(al, lengths, names, cr.make_reqs(rows))
    assert max(run_parts) == 3 and len(run_parts) == (sum(run_parts) + 2) // 3 > 10
    # a run per position over two whole blocks: every lane of every step starts and ends a run (depth 1, 2, 1, 2 ..)
    dense = [(1, p, 1) for p in range(0, 2 * COV_BLOCK_SPAN + 70)] + [(1, p, 1) for p in range(1, 2 * COV_BLOCK_SPAN + 70, 2)]
    with tuned(al, coverage_run_chunk=COV_TILE + 1):
        check(al, lengths, names, cr.make_reqs(dense))
    assert COV_BLOCK * 3 < len(dense)                      # (and several blocks of k_cov_mark and of the text kernels)


# ---- 5. bad requests ------------------------------------------------------------------------------------------------
def test_bad_requests_are_flagged_and_harm_nobody(crafted):
    al, lengths, names = crafted
    good = random_reqs(300, 3)
    bad = cr.make_reqs([(0, 10, 5), (4, 10, 5), (2, 10, 0), (2, 10, 5, 5, -3), (2, LENS[1] - 4, 5), (3, LENS[2] - 30, 10, 11, 10), (0xFFFFFFFF, 0, 1),
                        (1, 0xFFFFFFF0, 100), (1, 0, 0, 50, 0)])
    assert cr.flagged(bad, lengths).all()
    mixed = np.concatenate([good[:100], bad[:3], good[100:200], bad[3:], good[200:]])
    exp_runs, exp_tot = cr.runs_of(good, lengths)
    runs, tot, _ = al.coverage_runs(mixed)
    assert tot == dict(exp_tot, flagged=len(bad)) and runs.tolist() == exp_runs.tolist()
    check(al, lengths, names, mixed)
    check(al, lengths, names, bad)                          # nothing but bad requests: no run at all
    with tuned(al, coverage_slice_bases=1000):
        check(al, lengths, names, mixed)                    # flagged once, however many slices look at them


# ---- 6. the command line --------------------------------------------------------------------------------------------
PE = ["-d200", "-D400"]
# (name, genome fixture, paired reads' fixture, golden file of the primary output, options)
CLI = [("basic-s3", "basic", None, ("basic", "s3.m6.sam.gz"), ["-s3"]),
       ("pe-U3", "basic", "pe", ("pe", "U3.m6.sam.gz"), ["-U3", "-s5"] + PE),
       ("indel-a10", "indel", None, ("indel", "a10.m6.sam.gz"), ["-a10", "-s3"]),
       ("splice-A5000", "splice", None, ("splice", "A5000.m6.sam.gz"), ["-A5000", "-s3"]),
       ("chimeric-c50", "chimeric", None, ("chimeric", "c50.m6.sam.gz"), ["-c50", "-s3"]),
       ("multi-r5R5", "multi", None, ("multi", "r5R5.m6.sam.gz"), ["-s3", "-r5", "-R5"]),
       ("basic-s3x5", "basic", None, ("basic", "s3x5.m6.sam.gz"), ["-s3", "-x5"])]


def cli_args(golden_tmp, genome, pe, out, fmt="-M6"):
    d = golden_tmp[genome]
    if pe is None:
        inputs = ["-i", os.path.join(d, "reads.fa")]
    else:
        inputs = ["-i", os.path.join(helpers.GOLDEN, pe, "reads_1.fa.gz"), "-u", os.path.join(helpers.GOLDEN, pe, "reads_2.fa.gz")]
    return ["align"] + inputs + ["-I", os.path.join(d, "genome.sfx"), "-o", out, fmt]


def expected_bedgraph(sam_path, g):
    _, recs = helpers.parse_sam(sam_path)
    reqs = cr.requests_of_sam(recs, g.ids)
    lengths = {i: g.length(i) for i in g.names}
    assert not cr.flagged(reqs, lengths).any()
    runs, tot = cr.runs_of(reqs, lengths)
    assert tot["runs"] > 50
    return cr.text_of(runs, g.names), tot, reqs


@pytest.mark.parametrize("name,genome,pe,gold,flags", CLI, ids=[c[0] for c in CLI])
def test_cli_coverage_beside_the_unchanged_primary_output(golden_tmp, tmp_path, name, genome, pe, gold, flags):
    g = sr.Genome(os.path.join(golden_tmp[genome], "genome.sfx"))
    out, cov = str(tmp_path / "o.sam"), str(tmp_path / "o.bedgraph")
    log = run(cli_args(golden_tmp, genome, pe, out) + flags + ["--coverage", cov], str(tmp_path))
    assert open(out, "rb").read() == golden_bytes(*gold)
    exp, tot, reqs = expected_bedgraph(out, g)
    assert open(cov, "rb").read() == exp
    assert f"Coverage: {tot['covered']} bases covered, mean depth {tot['depth_sum'] / tot['covered']:.2f} over covered bases, largest depth {tot['max_depth']}, {tot['runs']} runs" in log
    if name == "pe-U3":
        assert tot["max_depth"] > 1
    if name in ("indel-a10", "splice-A5000"):
        assert (reqs["m2"] > 0).sum() > 10


def test_cli_coverage_is_the_same_for_every_output_format(golden_tmp, tmp_path):
    g = sr.Genome(os.path.join(golden_tmp["basic"], "genome.sfx"))
    covs = {}
    for tag, out, fmt, extra in (("m5", "o5.sam", "-M5", []), ("m0", "o0.csv", "-M0", []), ("bam", "o.bam", "-M6", []), ("gz", "o.sam.gz", "-M6", ["--sam-tags", "NM,MD"]),
                                 ("dev", "od.sam", "-M6", ["--devices", "0,0"])):
        cov = str(tmp_path / f"{tag}.bedgraph")
        run(cli_args(golden_tmp, "basic", None, str(tmp_path / out), fmt) + ["-s3", "--coverage", cov] + extra, str(tmp_path),
            env={"BK_SAM_DEVICE_MIN": "1"} if tag == "m5" else None)
        covs[tag] = open(cov, "rb").read()
    assert open(tmp_path / "o5.sam", "rb").read() == golden_bytes("basic", "s3.m5.sam.gz")
    assert open(tmp_path / "o0.csv", "rb").read() == golden_bytes("basic", "s3.m0.csv.gz")
    assert open(tmp_path / "o.bam", "rb").read() == open(os.path.join(helpers.GOLDEN, "basic", "s3.m6.bam"), "rb").read()
    assert open(tmp_path / "od.sam", "rb").read() == golden_bytes("basic", "s3.m6.sam.gz")
    assert covs["m5"] == expected_bedgraph(str(tmp_path / "o5.sam"), g)[0]
    assert covs["m0"] == covs["bam"] == covs["gz"] == covs["dev"] == covs["m5"]


def test_cli_without_the_option_writes_no_such_file(golden_tmp, tmp_path):
    out = str(tmp_path / "o.sam")
    log = run(cli_args(golden_tmp, "basic", None, out) + ["-s3"], str(tmp_path), env={"BK_TIMING": "1"})
    assert open(out, "rb").read() == golden_bytes("basic", "s3.m6.sam.gz")
    assert sorted(os.listdir(tmp_path)) == ["o.sam"]
    assert "overage" not in log
