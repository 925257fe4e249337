"""GPU tests of the plan table (run with -m gpu on an MI355X): the search passes, k_flat and the read preparation take a read's geometry in
a phase - core length, core step, number of cores, number of phases - from a table the host makes per (phase, read length) and keeps on
the context (biokanga_amd/csrc/bk_plan_table.h), and decode work items with reciprocals instead of divisions.  Every bk_hit field is
compared with the CPU oracle, on the synthetic two-sequence genome of tests/test_gpu_parity.py (_synth_case):
  (a) 3001 reads (no multiple of 256) of 18 .. 128 bases mixed, so the lanes of a wave read different entries, at align_strand 0, 1, 2 -
      an even and an odd number of items per read, one strand pass and two
  (b) one context, batches whose longest read is 50, then 120, then 36: the table made, made again longer, and serving a shorter batch
  (c) the same context after bk_ctx_set_params changed fields the derivation reads (max_subs; pmode -> min_core_len, slides_per100), and
      back: the table follows
  (d) reads of 129 .. 256 bases (rows in LDS, 16-word kernels), of 260 .. 500 (k_flat reads the table through the caches) and a batch with
      a few reads of 600 .. 2000 bases (the kernels that keep the direct calls; the table covers 2000 bases)
  (e) a fresh context, bk_ctx_reserve, then bk_align_batch_device_async as its first batch: reserve has made the table, the enqueue-only call
      makes none and refuses what the table does not serve."""
import numpy as np
import pytest

import helpers
from test_gpu_iv_records import _assert_records, _cut_reads
from test_gpu_parity import _synth_case

pytestmark = pytest.mark.gpu


def _bk():
    import biokanga_amd
    return biokanga_amd


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """the index file and the oracle on it, made once"""
    import torch
    bk = _bk()
    seq, ents, _reads = _synth_case(2024, 300000, 1, 100, 0, dup_len=140)
    n = len(seq)
    dev = torch.device("cuda:0")
    d_seq = torch.from_numpy(seq).to(dev)
    d_sa = torch.empty(n, dtype=torch.int32, device=dev)
    bk.build_sa_device(d_seq.data_ptr(), n, d_sa.data_ptr(), 4, 0)
    path = str(tmp_path_factory.mktemp("plan") / "synth.sfx")
    helpers.write_sfx(path, "synth", [("s1", int(ents[0]["seq_len"])), ("s2", int(ents[1]["seq_len"]))], seq, d_sa.cpu().numpy().view(np.uint32))
    o = helpers.OracleSfx(path)
    yield {"sfx": path, "seq": seq, "oracle": o}
    o.close()


def _reads(genome, seed, lens, n_with_n=0):
    return _cut_reads(genome["seq"], np.random.default_rng(seed), lens, max_e=4, n_with_n=n_with_n)


def _expect(genome, batch, **kw):
    exp, _ctr = genome["oracle"].align(*batch, helpers.make_params(**kw), nthreads=8)
    return exp


@pytest.mark.parametrize("align_strand", [0, 1, 2], ids=["both_strands", "watson", "crick"])
def test_mixed_lengths_in_one_wave(genome, align_strand):
    bk = _bk()
    rng = np.random.default_rng(31)
    batch = _reads(genome, 32, rng.integers(18, 129, size=3001), n_with_n=40)
    exp = _expect(genome, batch, max_subs=3, align_strand=align_strand)
    assert len(np.unique(exp["rslt"])) > 1 and np.count_nonzero(exp["nar"] == 1) > 500
    with bk.Aligner(genome["sfx"], bk.AlignParams(max_subs=3, align_strand=align_strand)) as al:
        for sync in (1, 0):                      # launches sized from bounds, and from counts read back
            al.tune("async_phases", sync)
            _assert_records(al.align(*batch), exp, f"3001 reads of 18..128 bases, align_strand {align_strand}, async_phases {sync}")


def test_table_reuse_regrowth_and_parameter_change(genome):
    bk = _bk()
    rng = np.random.default_rng(47)
    batches = [_reads(genome, 50 + top, np.concatenate(([top], rng.integers(20, top + 1, size=1400))), n_with_n=10) for top in (50, 120, 36)]
    with bk.Aligner(genome["sfx"], bk.AlignParams(max_subs=3)) as al:
        # (b) made for 50 bases, made again for 120, the batch of 36 served by the table for 120
        for batch in batches:
            _assert_records(al.align(*batch), _expect(genome, batch, max_subs=3), f"longest read {int(batch[2].max())}")
        # (c) fields make_plan reads change under the table, and change back
        first = _expect(genome, batches[1], max_subs=3)
        for kw in ({"max_subs": 5}, {"max_subs": 5, "pmode": 2}, {"max_subs": 3, "min_edit_dist": 2}, {"max_subs": 3}):
            al.set_params(bk.AlignParams(**kw))
            exp = _expect(genome, batches[1], **kw)
            _assert_records(al.align(*batches[1]), exp, f"after set_params({kw})")
        assert any(not np.array_equal(exp[f], _expect(genome, batches[1], max_subs=5)[f]) for f in ("low_mm", "nar", "rslt"))      # (the change mattered)
        _assert_records(al.align(*batches[1]), first, "back at the first parameters")


def test_longer_reads_and_the_kernels_that_keep_direct_calls(genome):
    bk = _bk()
    rng = np.random.default_rng(59)
    mid = _reads(genome, 60, rng.integers(129, 257, size=1300), n_with_n=10)
    long_ = _reads(genome, 61, rng.integers(260, 501, size=700), n_with_n=5)
    longest = _reads(genome, 62, np.concatenate((rng.integers(40, 200, size=300), [600, 777, 1024, 1500, 2000, 1999])), n_with_n=3)
    with bk.Aligner(genome["sfx"], bk.AlignParams(max_subs=3)) as al:
        for what, batch in (("129..256 bases", mid), ("260..500 bases", long_), ("a few reads of 600..2000 bases", longest), ("129..256 bases again", mid)):
            _assert_records(al.align(*batch), _expect(genome, batch, max_subs=3), what)


def test_reserve_makes_the_table_for_the_enqueue_only_call(genome):
    """bk_ctx_reserve makes the table with the rest of the scratch: on a fresh context the call that only enqueues is the FIRST batch and finds
    it there; what the table does not serve as it stands - a longer read than was reserved for, parameters changed since - is refused before
    anything is launched, and reserved for again it runs"""
    import torch
    bk = _bk()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(71)
    batch = _reads(genome, 72, np.concatenate(([100], rng.integers(30, 101, size=2000))), n_with_n=10)
    n = len(batch[2])
    d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in batch]
    out = torch.zeros(n * bk.HIT_DTYPE.itemsize, dtype=torch.uint8, device=dev)

    def enqueue(al, ml, stream=None):
        out.zero_()
        torch.cuda.synchronize()
        al.align_device_async(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, ml, out.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy().view(bk.HIT_DTYPE).copy()

    with bk.Aligner(genome["sfx"], bk.AlignParams(max_subs=3)) as al:
        al.reserve(n, 100)
        st = torch.cuda.Stream(device=dev)                  # (not the context's stream: the table is in HBM when reserve returns)
        _assert_records(enqueue(al, 100, st.cuda_stream), _expect(genome, batch, max_subs=3), "first batch of a fresh context, enqueue-only")
        with pytest.raises(bk.BkError):                     # reserved for 100 bases
            enqueue(al, 101)
        al.set_params(bk.AlignParams(max_subs=5))
        with pytest.raises(bk.BkError):                     # the table was made for -s3
            enqueue(al, 100)
        al.reserve(n, 100)
        _assert_records(enqueue(al, 100), _expect(genome, batch, max_subs=5), "reserved again after set_params")
