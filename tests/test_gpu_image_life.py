"""The life of an index image in HBM (bk_image.cpp): one context through every knob that rebuilds, replaces or drops a table of the image;
clones of images that are not in their default state; contexts that give all their device memory back.  Only the C ABI is used: what is
checked is that records never change and that memory neither leaks nor is shared between a clone and its source."""
import os

import numpy as np
import pytest

import helpers
from test_gpu_parity import _synth_case, assert_hits_equal, load_fixture

pytestmark = pytest.mark.gpu

GETTERS = ("ktab_packed", "ktab2_resident", "ktab2_elem", "k3_resident")


def _bk():
    import biokanga_amd
    return biokanga_amd


@pytest.fixture(scope="module")
def repeat(golden_tmp):
    """the `repeat` golden index, its s3 reads, and their records from a context in its default state"""
    bk = _bk()
    d, names, bases, offs, lens, keep = load_fixture(golden_tmp, "repeat", "s3")
    sfx = os.path.join(d, "genome.sfx")
    batch = (bases, offs[keep], lens[keep])
    with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
        ref = al.align(*batch)
    return dict(sfx=sfx, batch=batch, ref=ref)


def _sfx_of(tmp_path, name, seq, ents, el_size):
    """a .sfx of `seq` whose suffix array the device builder made"""
    import torch
    bk = _bk()
    n = len(seq)
    d_seq = torch.from_numpy(seq).to("cuda:0")
    d_sa = torch.empty(n, dtype=torch.int32, device="cuda:0")
    bk.build_sa_device(d_seq.data_ptr(), n, d_sa.data_ptr(), 4, 0)
    sa = d_sa.cpu().numpy().view(np.uint32)
    del d_seq, d_sa
    path = str(tmp_path / (name + ".sfx"))
    helpers.write_sfx(path, name, [("s1", int(ents[0]["seq_len"])), ("s2", int(ents[1]["seq_len"]))], seq, sa.astype(np.uint64) if el_size == 5 else sa,
                      el_size=el_size)
    return path


def _batch_of(reads):
    n, w = reads.shape
    return reads.reshape(-1), np.arange(n, dtype=np.uint64) * w, np.full(n, w, dtype=np.uint32)


# (knob, value, {getter: expected}) in the order they are applied; a list of knobs is one step
STEPS = [
    ([("use_ktab2", 0)], {"ktab2_resident": 0}),
    ([("use_ktab2", 2)], {"ktab2_elem": 1}),
    ([("use_ktab2", 1)], {"ktab2_resident": 1, "ktab2_elem": 0}),
    ([("ktab_wide", 1)], {"ktab_packed": 1, "ktab2_resident": 0}),
    ([("ktab_wide", 2)], {"ktab_packed": 0}),
    ([("ktab_wide", 0)], {"ktab2_resident": 1}),
    ([("use_k3", 0)], {"k3_resident": 0}),
    ([("use_k3", 1)], {"k3_resident": 1}),
    ([("use_k3", 2)], {"k3_resident": 2}),
    ([("use_k2", 0)], {"k3_resident": 0, "ktab2_resident": 0}),
    ([("use_k2", 1)], {}),
    ([("use_isa", 0)], {}),
    ([("use_isa", 1)], {}),
    ([("use_tgt2", 0)], {}),
    ([("use_tgt2", 1)], {}),
    ([("use_tgt2", 2)], {}),
    ([("kmer_bits", 6)], {}),
    ([("use_ktab", 0)], {}),
    ([("use_ktab", 1)], {}),
    ([("use_swin", 2)], {"swin_resident": 1, "swin_core_lens": "nonzero"}),
    ([("use_swin", 3)], {"swin_resident": 1, "swin_core_lens": 0}),
    ([("use_swin", 0)], {"swin_resident": 0}),
]


def test_rebuilds_on_one_context(repeat):
    """every knob that frees and makes a table of the image again, in turn on ONE context: after each step the same reads give the same
    records, and the getters say the table asked for is the one that is live"""
    bk = _bk()
    with bk.Aligner(repeat["sfx"], bk.AlignParams(max_subs=3)) as al:
        for knobs, getters in STEPS:
            for kv in knobs:
                al.tune(*kv)
            try:
                assert_hits_equal(al.align(*repeat["batch"]), repeat["ref"])
            except AssertionError as e:
                raise AssertionError(f"after {knobs}: {e}") from None
            for g, want in getters.items():
                got = al.tune(g, 0)
                assert (got != 0) if want == "nonzero" else (got == want), (knobs, g, got, want)


CLONE_STATES = {
    "default": [],
    "ktab_wide1": [("ktab_wide", 1)],
    "ktab_wide2": [("ktab_wide", 2)],
    "no_ktab2_no_k3": [("use_ktab2", 0), ("use_k3", 0)],
    "ktab2_elem": [("use_ktab2", 2)],
    "no_isa": [("use_isa", 0)],
    "tgt2_single": [("use_tgt2", 1)],
    "kmer_bits6": [("kmer_bits", 6)],
    "grown": "grown",            # a BK_CTX_GROW_IMAGE context whose worker's tables have been taken in
    "swin_resident": "swin",     # the source holds a window array (which a clone makes for itself)
    "five_byte": "five_byte",    # an index of 5-byte suffix array elements
}


@pytest.mark.parametrize("state", list(CLONE_STATES))
def test_clone_of_non_default_images(repeat, tmp_path, state):
    """bk_ctx_clone of a source whose image is not the default one: the copy has every table of the source at the source's size (the
    records and the getters agree), and it owns its memory (it goes on working when the source is gone)"""
    bk = _bk()
    sfx, batch, flags = repeat["sfx"], repeat["batch"], 0
    what = CLONE_STATES[state]
    if what == "five_byte":
        seq, ents, reads = _synth_case(777, 300000, 3000, 100, 3)
        sfx, batch = _sfx_of(tmp_path, "wide", seq, ents, 5), _batch_of(reads)
    if what == "grown":
        flags = bk.CTX_GROW_IMAGE
    src = bk.Aligner(sfx, bk.AlignParams(max_subs=3), flags=flags)
    try:
        if what == "grown":
            assert src.tune("image_wait", 0) > 0 and src.tune("grow_state", 0) == 4
        elif what == "swin":
            src.tune("use_swin", 2)
        elif what == "five_byte":
            assert src.lib.bk_sfx_el_size(src.h) == 5
        else:
            for kv in what:
                src.tune(*kv)
        ref = src.align(*batch)
        if what == "swin":
            assert src.tune("swin_resident", 0) == 1
        elif what != "five_byte":
            assert_hits_equal(ref, repeat["ref"])
        with bk.Aligner(clone_of=src, device=0) as cl:
            assert_hits_equal(cl.align(*batch), ref)
            for g in GETTERS:
                assert cl.tune(g, 0) == src.tune(g, 0), g
            src.close()
            assert_hits_equal(cl.align(*batch), ref)
    finally:
        src.close()


def _free_mb():
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info(0)[0] / 2.0**20


def test_contexts_give_their_memory_back(golden_tmp, tmp_path):
    """Contexts that are made, used, rebuilt, cloned and closed leave no device memory behind.  A 2 Mbp index of 4-byte elements: suffix
    array, inverse suffix array, keys and k-mer table are 8 MB and more each, so ONE table leaked per cycle costs 32 MB and more over
    the four cycles between the two readings; the bound is 4 MB, half the smallest of them.  Creating from a truncated .sfx, which fails,
    is held to the same bound.
    The bound is a condition, not a measurement.  The drift of the tree before the image's tables became DevBufs has NOT been measured: no
    MI355X could be had when this test was written (profiles/NOTES.md).  It belongs here once it is; both drifts are printed (-s)."""
    bk = _bk()
    seq, ents, reads = _synth_case(4321, 2_000_000, 4000, 100, 3)
    sfx, batch = _sfx_of(tmp_path, "life", seq, ents, 4), _batch_of(reads)
    free = {}
    ref = None
    for cycle in range(1, 7):
        with bk.Aligner(sfx, bk.AlignParams(max_subs=3)) as al:
            got = al.align(*batch)
            if ref is None:
                ref = got
            assert_hits_equal(got, ref)
            al.tune("use_swin", 2)
            assert_hits_equal(al.align(*batch), ref)
            al.tune("ktab_wide", 1)
            with bk.Aligner(clone_of=al, device=0) as cl:
                assert_hits_equal(cl.align(*batch), ref)
        free[cycle] = _free_mb()
    print(f"free device memory after cycle 2: {free[2]:.1f} MB, after cycle 6: {free[6]:.1f} MB, drift {free[2] - free[6]:.1f} MB")
    assert free[6] >= free[2] - 4.0, free

    img = bytearray(open(os.path.join(golden_tmp["basic"], "genome.sfx"), "rb").read())
    bad = str(tmp_path / "truncated.sfx")
    open(bad, "wb").write(img[: len(img) // 2])
    before = _free_mb()
    for _ in range(5):
        with pytest.raises(bk.BkError) as e:
            bk.Aligner(bad, bk.AlignParams(max_subs=3))
        assert e.value.rc < 0
    after = _free_mb()
    print(f"free device memory before the refused files: {before:.1f} MB, after: {after:.1f} MB, drift {before - after:.1f} MB")
    assert after >= before - 4.0, (before, after)
