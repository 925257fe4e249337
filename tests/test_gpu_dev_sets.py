"""GPU unit tests of the seen-key sets of the wave-per-read kernels (biokanga_amd/csrc/bk_dev_sets.h): the LDS set lset_*, the
epoch-tagged HBM table htab_* with its tombstones, same_key_earlier_in_round.  The helpers run under the test-only kernels of
tests/hip/devtest.hip (one wave per block, k_wave's order of look-ups and inserts); the references are a Python set and numpy,
everything is compared exactly.  Every probe loop of these helpers ends only at a free slot, so the wrappers below refuse a
load beyond the code's own caps: kLdsSetFill keys in the LDS set, half of an HBM table (tombstones counted)."""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LOOK, INSERT = 1, 2
CONTAINS, INS, FIND, FIND_RETRACT = 1, 2, 3, 4
TS = 1024                                   # the smallest table size_heavy_scratch makes
EMPTY = 0xFFFFFFFF


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.itemsize])).to("cuda")


def _host(t, dtype):
    return t.cpu().numpy().view(dtype)


def _ok(rc):
    assert rc == 0, f"hipError_t {rc}"


def lset_buckets(keys):
    import torch
    lib = helpers.devtest_lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    d_k = _dev(keys)
    d_o = torch.zeros(len(keys), dtype=torch.int32, device="cuda")
    _ok(lib.bkdt_lset_bucket(d_k.data_ptr(), len(keys), d_o.data_ptr()))
    return _host(d_o, np.uint32)


def lset_rounds(keys, flags):
    """keys, flags [R, 64] -> (look-up bit [R, 64], the Python-set model's bit, final set words, the model's set)"""
    import torch
    lib = helpers.devtest_lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 64)
    flags = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1, 64)
    assert keys.shape == flags.shape
    model, want = set(), np.zeros(keys.shape, dtype=bool)
    for r in range(len(keys)):
        for ln in range(64):
            if flags[r, ln] & LOOK:
                want[r, ln] = int(keys[r, ln]) in model
        model.update(int(k) for k in keys[r][(flags[r] & INSERT) != 0])
    assert EMPTY not in model, "the empty-slot key is never inserted (k_wave sends it to the HBM table)"
    assert len(model) <= lib.kLdsSetFill, "beyond the LDS set's cap the probe loops do not end"
    d_k, d_f = _dev(keys), _dev(flags)
    d_found = torch.zeros(keys.size, dtype=torch.uint8, device="cuda")
    d_set = torch.zeros(lib.kLdsSet, dtype=torch.int32, device="cuda")
    _ok(lib.bkdt_lset_rounds(d_k.data_ptr(), d_f.data_ptr(), len(keys), d_found.data_ptr(), d_set.data_ptr()))
    return _host(d_found, np.uint8).reshape(keys.shape) != 0, want, _host(d_set, np.uint32), model


def _check_lset(keys, flags):
    got, want, words, model = lset_rounds(keys, flags)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, [(int(r), int(ln), hex(int(np.asarray(keys).reshape(-1, 64)[r, ln])), bool(want[r, ln])) for r, ln in bad[:8]]
    held = words[words != EMPTY]
    assert sorted(int(k) for k in held) == sorted(model)            # every key once, nothing else
    return words


def _rows(keys, flag):
    """keys -> rounds of 64 lanes, the last one padded with idle lanes"""
    keys = np.asarray(keys, dtype=np.uint32)
    n = (len(keys) + 63) // 64 * 64
    k = np.zeros(n, dtype=np.uint32)
    f = np.zeros(n, dtype=np.uint8)
    k[:len(keys)] = keys
    f[:len(keys)] = flag
    return k.reshape(-1, 64), f.reshape(-1, 64)


def _random_keys(rng, n, exclude=()):
    out, seen = [], set(exclude) | {EMPTY}
    while len(out) < n:
        k = int(rng.integers(0, 1 << 32))
        if k not in seen:
            seen.add(k)
            out.append(k)
    return np.array(out, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ LDS set
def test_lset_random_keys_up_to_the_fill_cap():
    lib = helpers.devtest_lib()
    assert (lib.kLdsSet, lib.kLdsSetFill, lib.kLdsEmpty) == (2048, 1536, EMPTY)
    rng = np.random.default_rng(101)
    ins = _random_keys(rng, lib.kLdsSetFill)
    absent = _random_keys(rng, 4096 + 32 * (lib.kLdsSetFill // 64), exclude=ins.tolist())
    K, F = [], []
    for r in range(lib.kLdsSetFill // 64):
        # (a lane that inserts looks its key up first, as in k_wave)
        K.append(ins[64 * r:64 * r + 64]); F.append(np.full(64, LOOK | INSERT, dtype=np.uint8))
        look = np.concatenate([rng.choice(ins[:64 * r + 64], 32, replace=False), absent[32 * r:32 * r + 32]])
        K.append(rng.permutation(look)); F.append(np.full(64, LOOK, dtype=np.uint8))
    k2, f2 = _rows(np.concatenate([ins, absent[-4096:]]), LOOK)
    words = _check_lset(np.concatenate([np.stack(K), k2]), np.concatenate([np.stack(F), f2]))
    assert int((words != EMPTY).sum()) == lib.kLdsSetFill


@pytest.fixture(scope="module")
def bucket_keys():
    """keys by LDS bucket, from the lset_bucket export (the hash is not restated here)"""
    lib = helpers.devtest_lib()
    keys = _random_keys(np.random.default_rng(102), 1 << 17)
    b = lset_buckets(keys)
    assert int(b.max()) < lib.kLdsSet // 4
    return {int(x): keys[b == x] for x in (0, 7, 300, lib.kLdsSet // 4 - 1)}


@pytest.mark.parametrize("bucket", [7, 511])
@pytest.mark.parametrize("n", [5, 9, 64])
def test_lset_keys_of_one_bucket(bucket_keys, bucket, n):
    """more keys than a bucket's four slots: the probe goes on to the next buckets (from bucket 511 to bucket 0); all inserted in one
    round, the lanes racing for the slots"""
    lib = helpers.devtest_lib()
    nb = lib.kLdsSet // 4
    assert bucket < nb
    pool = bucket_keys[bucket]
    assert len(pool) >= n + 16
    ins, absent = pool[:n], pool[n:n + 16]
    k0, f0 = _rows(ins, LOOK | INSERT)
    k1, f1 = _rows(np.concatenate([ins, absent]), LOOK)
    words = _check_lset(np.concatenate([k0, k1]), np.concatenate([f0, f1]))
    used = np.nonzero(words != EMPTY)[0]
    assert sorted(int(u) for u in used) == sorted((4 * bucket + i) % lib.kLdsSet for i in range(n))   # the buckets fill in probe order


def test_lset_one_key_at_a_time_through_a_full_bucket(bucket_keys):
    pool = bucket_keys[300]
    K = np.zeros((20, 64), dtype=np.uint32)
    F = np.zeros((20, 64), dtype=np.uint8)
    for r in range(10):
        K[r, 0] = pool[r]; F[r, 0] = LOOK | INSERT
        K[10 + r, :12] = pool[:12]; F[10 + r, :12] = LOOK               # (the same answers every time: look-ups change nothing)
    words = _check_lset(K, F)
    assert [int(w) for w in words[1200:1210]] == [int(k) for k in pool[:10]]


def test_lset_one_key_in_every_lane_of_a_round():
    key = 0x9E3779B9
    K = np.full((2, 64), key, dtype=np.uint32)
    F = np.array([[LOOK | INSERT] * 64, [LOOK] * 64], dtype=np.uint8)
    words = _check_lset(K, F)
    assert int((words == key).sum()) == 1 and int((words != EMPTY).sum()) == 1


def test_lset_edge_keys():
    edge = np.array([0, 1, 0x80000000, 0xFFFFFFFE], dtype=np.uint32)
    K = np.zeros((3, 64), dtype=np.uint32)
    F = np.zeros((3, 64), dtype=np.uint8)
    K[0, :4] = edge; F[0, :4] = LOOK
    K[1, :4] = edge; F[1, :4] = LOOK | INSERT
    K[2, :4] = edge; F[2, :4] = LOOK
    K[2, 4:8] = [2, 0x7FFFFFFF, 0x80000001, 0xFFFFFFFD]; F[2, 4:8] = LOOK
    _check_lset(K, F)


def test_lset_never_holds_the_empty_slot_key():
    """0xFFFFFFFF - the key of a target start of 2^32 - 2 (mod 2^32) - is what a free slot holds; k_wave keeps that key in the HBM
    table and looks it up in the LDS set like every other: the answer is "not seen", whatever the set holds"""
    lib = helpers.devtest_lib()
    ins = _random_keys(np.random.default_rng(103), lib.kLdsSetFill)
    rest, frest = _rows(ins[1:], LOOK | INSERT)
    one = np.zeros((1, 64), dtype=np.uint32)
    look = np.full((1, 64), EMPTY, dtype=np.uint32)
    f_look = np.zeros((1, 64), dtype=np.uint8); f_look[0, :3] = LOOK
    f_one = np.zeros((1, 64), dtype=np.uint8); f_one[0, 0] = LOOK | INSERT
    one[0, 0] = ins[0]
    K = np.concatenate([look, one, look, rest, look])
    F = np.concatenate([f_look, f_one, f_look, frest, f_look])
    got, want, words, model = lset_rounds(K, F)
    assert len(model) == lib.kLdsSetFill
    for r in (0, 2, len(K) - 1):                                        # empty set, one key, at the fill cap
        assert not got[r, :3].any(), f"0xFFFFFFFF reads as seen in round {r}"
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ HBM table
def htab_hash(key, ts=TS):
    return (int(key) * 2654435761) % (1 << 32) & (ts - 1)               # hash_key, restated for a table of ts entries


def htab_rounds(keys, ops, epochs, ts=TS):
    """keys, ops [B, R, 64], epochs [B, R] on B zeroed table slices -> (result bit per lane, tables [B, ts]).  Refuses rounds whose
    answers depend on which lane wins a race other than "one of the lanes with a new key is told so", and loads beyond half a table."""
    import torch
    lib = helpers.devtest_lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32)
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    epochs = np.ascontiguousarray(epochs, dtype=np.uint32)
    B, R, _ = keys.shape
    assert keys.shape == ops.shape == (B, R, 64) and epochs.shape == (B, R)
    assert int(epochs.min()) >= 1 and int(epochs.max()) < lib.kTombBit
    for b in range(B):
        used = {}                                                       # epoch -> slots taken under it (tombstones stay counted)
        live, tombs = set(), set()
        for r in range(R):
            e = int(epochs[b, r])
            k, o = keys[b, r], ops[b, r]
            looked, found = set(int(x) for x in k[o == CONTAINS]), set(int(x) for x in k[(o == FIND) | (o == FIND_RETRACT)])
            assert not (looked & found), "a look-up beside a find_or_insert of the same key: the answer is a race"
            plain = looked | set(int(x) for x in k[o == INS])
            assert not (plain and e in tombs), "htab_contains / htab_insert never meet tombstones of their own epoch (k_wave: find_or_insert only, once it retracts)"
            new = set((e, x) for x in found | set(int(x) for x in k[o == INS])) - live
            used[e] = used.get(e, 0) + len(new)
            assert used[e] <= ts // 2, "beyond half a table the probe loops need not end"
            live |= new
            gone = set((e, int(x)) for x in k[o == FIND_RETRACT]) & new
            live -= gone                                                # (the slot stays counted: a key that comes again takes another)
            if gone:
                tombs.add(e)
    d_tab = torch.zeros(B * ts, dtype=torch.int64, device="cuda")
    d_k, d_o, d_e = _dev(keys), _dev(ops), _dev(epochs)
    d_out = torch.zeros(keys.size, dtype=torch.uint8, device="cuda")
    _ok(lib.bkdt_htab_rounds(d_tab.data_ptr(), ts, B, d_k.data_ptr(), d_o.data_ptr(), d_e.data_ptr(), R, d_out.data_ptr()))
    return _host(d_out, np.uint8).reshape(keys.shape) != 0, _host(d_tab, np.uint64).reshape(B, ts)


def _check_htab(keys, ops, epochs, ts=TS):
    """runs the rounds and follows them with a set per slice: contains -> membership; find_or_insert -> membership, and of the lanes
    of a round that bring one new key exactly one is told "new"; a lane that retracts takes its key out again after the round"""
    keys, ops, epochs = np.asarray(keys, dtype=np.uint32), np.asarray(ops, dtype=np.uint8), np.asarray(epochs, dtype=np.uint32)
    if keys.ndim == 2:
        keys, ops, epochs = keys[None], ops[None], epochs[None]
    got, tabs = htab_rounds(keys, ops, epochs, ts)
    B, R, _ = keys.shape
    for b in range(B):
        live = set()
        for r in range(R):
            e = int(epochs[b, r])
            first_new = {}
            for ln in range(64):
                k, o = int(keys[b, r, ln]), int(ops[b, r, ln])
                if o == CONTAINS:
                    assert bool(got[b, r, ln]) == ((e, k) in live), (b, r, ln, hex(k), "contains")
                elif o in (FIND, FIND_RETRACT):
                    if (e, k) in live:
                        assert got[b, r, ln], (b, r, ln, hex(k), "find_or_insert: a key of an earlier round reads as new")
                    elif not got[b, r, ln]:
                        assert k not in first_new, (b, r, ln, hex(k), "find_or_insert: two lanes are told that the key is new")
                        first_new[k] = o
                    else:
                        assert got[b, r, ln]                            # a lane that lost the race to another lane of this round
                else:
                    assert not got[b, r, ln]
            for ln in range(64):
                k, o = int(keys[b, r, ln]), int(ops[b, r, ln])
                if o in (FIND, FIND_RETRACT) and (e, k) not in live:
                    assert k in first_new, (b, r, hex(k), "find_or_insert: no lane is told that the key is new")
            for ln in range(64):
                if int(ops[b, r, ln]) == INS:
                    live.add((e, int(keys[b, r, ln])))
            for k, o in first_new.items():
                if o == FIND:
                    live.add((e, k))
        # the table: the live entries of the last epoch are exactly the model's
        e = int(epochs[b, -1])
        t = tabs[b]
        mine = t[(t >> np.uint64(32)) == np.uint64(e)]
        assert sorted(int(v) & 0xFFFFFFFF for v in mine) == sorted(k for (ee, k) in live if ee == e), (b, "table contents")
    return got, tabs


def _lanes(pairs):
    k = np.zeros(64, dtype=np.uint32)
    o = np.zeros(64, dtype=np.uint8)
    for i, (op, key) in enumerate(pairs):
        k[i], o[i] = key, op
    return k, o


def _rounds(rows, epoch):
    ks, os_ = zip(*(_lanes(r) for r in rows))
    ep = np.array(epoch if isinstance(epoch, (list, tuple)) else [epoch] * len(rows), dtype=np.uint32)
    return np.stack(ks), np.stack(os_), ep


def test_htab_contains_then_insert_as_k_heavy():
    rng = np.random.default_rng(201)
    new = _random_keys(rng, 448)
    absent = _random_keys(rng, 2048, exclude=new.tolist())
    rows, a = [], 0
    for r in range(14):
        fresh = new[32 * r:32 * r + 32]
        old = rng.choice(new[:32 * r], 16, replace=False) if r else absent[a:a + 16]
        look = np.concatenate([fresh, old, absent[a + 16:a + 32]])
        a += 32
        rows.append([(CONTAINS, k) for k in rng.permutation(look)])
        rows.append([(INS, k) for k in np.concatenate([fresh, fresh[:8]])])          # (a key twice in one round of inserts)
    for i in range(0, 448, 64):
        rows.append([(CONTAINS, k) for k in new[i:i + 64]])
    for i in range(1024, 2048, 64):
        rows.append([(CONTAINS, k) for k in absent[i:i + 64]])
    _check_htab(*_rounds(rows, 3))


def test_htab_find_or_insert_as_the_fused_wave_kernel():
    rng = np.random.default_rng(202)
    new = _random_keys(rng, 480)
    rows = []
    for r in range(15):
        fresh = new[32 * r:32 * r + 32]
        old = rng.choice(new[:32 * r], 24, replace=False) if r else fresh[:24]
        rows.append([(FIND, k) for k in rng.permutation(np.concatenate([fresh, old, fresh[:8]]))])
    for i in range(0, 480, 64):
        rows.append([(CONTAINS, k) for k in new[i:i + 64]])
    _check_htab(*_rounds(rows, 0x7FFFFFFF))                                          # the largest epoch there is


def test_htab_one_new_key_in_several_lanes():
    rows = [[(FIND, 0xABCDEF01)] * 64, [(FIND, 0xABCDEF01)] * 5 + [(FIND, 77)] * 7 + [(FIND, 78)], [(CONTAINS, 0xABCDEF01), (CONTAINS, 77), (CONTAINS, 78), (CONTAINS, 79)]]
    got, _ = _check_htab(*_rounds(rows, 9))
    assert int((~got[0, 0]).sum()) == 1 and int((~got[0, 1, 5:12]).sum()) == 1 and got[0, 1, :5].all() and not got[0, 1, 12]


def _colliding(h, n, rng, ts=TS):
    out = []
    while len(out) < n:
        k = int(rng.integers(0, 1 << 32))
        if htab_hash(k, ts) == h and k not in out and k != EMPTY:
            out.append(k)
    return out


def test_htab_retract():
    """a retracted key reads as not seen; its slot stays taken for the probing of others - keys that came past it are found, and are
    found (not entered a second time) by find_or_insert; the same key entered again is found"""
    rng = np.random.default_rng(203)
    h = 517
    x, a, b, c, d = _colliding(h, 5, rng)
    e = 12
    rows = [[(FIND, x)],                               # slot h
            [(FIND_RETRACT, a), (FIND, b)],            # slots h + 1, h + 2 in either order; a's becomes a tombstone
            [(FIND, c)],                               # must walk past the tombstone: slot h + 3
            [(FIND, b), (FIND, c), (FIND, x)],         # all seen: none of them may settle in the tombstone
            [(FIND, a)],                               # not seen, entered again: slot h + 4
            [(FIND, a), (FIND, b), (FIND, c)],         # all seen
            [(FIND, d)]]                               # slot h + 5
    got, tabs = _check_htab(*_rounds(rows, e))
    assert not got[0, 2, 0] and got[0, 3, :3].all() and not got[0, 4, 0] and got[0, 5, :3].all() and not got[0, 6, 0]
    t = tabs[0]
    tomb = (e | helpers.devtest_lib().kTombBit) << 32
    assert int(t[h]) == (e << 32) | x and int(t[h + 3]) == (e << 32) | c and int(t[h + 4]) == (e << 32) | a and int(t[h + 5]) == (e << 32) | d
    assert sorted([int(t[h + 1]), int(t[h + 2])]) == sorted([tomb, (e << 32) | b])
    assert int((t != 0).sum()) == 6


def test_htab_epochs():
    """the entries and the tombstones of epoch e are nothing at epoch e + 1: the keys are absent, the slots are taken again"""
    rng = np.random.default_rng(204)
    h = 90
    k0, tb, p, q = _colliding(h, 4, rng)
    many = _random_keys(rng, 500, exclude=[k0, tb, p, q])
    rows, ep = [], []
    for i in range(0, 500, 50):
        rows.append([(FIND, k) for k in many[i:i + 50]]); ep.append(7)
    rows += [[(CONTAINS, k) for k in many[:64]]]; ep.append(7)
    for i in range(0, 500, 64):
        rows.append([(CONTAINS, k) for k in many[i:i + 64]]); ep.append(8)
    for i in range(0, 500, 50):
        rows.append([(FIND, k) for k in many[i:i + 50]]); ep.append(8)          # new again, all of them
    for i in range(0, 500, 64):
        rows.append([(CONTAINS, k) for k in many[i:i + 64]]); ep.append(8)
    _check_htab(*_rounds(rows, ep))
    # a key and a tombstone of epoch 7 in slots h, h + 1; two keys of epoch 8 with the same hash take exactly these slots
    rows = [[(FIND, k0)], [(FIND_RETRACT, tb)], [(CONTAINS, k0), (CONTAINS, tb)], [(FIND, p)], [(FIND, q)], [(CONTAINS, k0), (CONTAINS, p), (CONTAINS, q)]]
    got, tabs = _check_htab(*_rounds(rows, [7, 7, 8, 8, 8, 8]))
    assert not got[0, 2, :2].any() and not got[0, 5, 0] and got[0, 5, 1:3].all()
    assert int(tabs[0][h]) == (8 << 32) | p and int(tabs[0][h + 1]) == (8 << 32) | q and int((tabs[0] != 0).sum()) == 2


def test_htab_keys_0_and_ffffffff():
    rng = np.random.default_rng(205)
    other = _random_keys(rng, 100, exclude=[0])
    for op in (INS, FIND):
        rows = [[(CONTAINS, 0), (CONTAINS, EMPTY)],
                [(op, k) for k in other[:50]],
                [(CONTAINS, 0), (CONTAINS, EMPTY)],
                [(op, 0), (op, EMPTY)] + [(op, k) for k in other[50:]],
                [(CONTAINS, 0), (CONTAINS, EMPTY), (CONTAINS, 1), (CONTAINS, 0xFFFFFFFE)],
                [(FIND, 0), (FIND, EMPTY)]]
        got, _ = _check_htab(*_rounds(rows, 1))                                       # (epoch 1: key 0 is 1 << 32, not a free slot)
        assert not got[0, 0, :2].any() and not got[0, 2, :2].any() and got[0, 4, :2].all() and not got[0, 4, 2:4].any() and got[0, 5, :2].all()


@pytest.mark.parametrize("h", [0, 1020, 1023])
def test_htab_colliding_keys_and_a_probe_sequence_that_wraps(h):
    rng = np.random.default_rng(206 + h)
    ks = _colliding(h, 9, rng)
    rows = [[(FIND, k) for k in ks[:6]], [(CONTAINS, k) for k in ks], [(INS, ks[6])], [(FIND, k) for k in ks[:8]], [(CONTAINS, k) for k in ks]]
    got, tabs = _check_htab(*_rounds(rows, 4))
    assert sorted(int(i) for i in np.nonzero(tabs[0])[0]) == sorted((h + i) % TS for i in range(8))


def test_htab_blocks_on_their_own_slices():
    """four waves at once, each on its slice of the allocation as wave_slot does, their keys drawn from one small pool: what one
    enters no other sees"""
    rng = np.random.default_rng(207)
    pool = _random_keys(rng, 600)
    B, R = 4, 20
    keys = np.zeros((B, R, 64), dtype=np.uint32)
    ops = np.zeros((B, R, 64), dtype=np.uint8)
    for b in range(B):
        for r in range(R):
            keys[b, r] = rng.choice(pool, 64, replace=False)
            ops[b, r] = (CONTAINS, FIND if b & 1 else INS)[r & 1]
    ep = np.tile(np.array([[2], [2], [5], [6]], dtype=np.uint32), (1, R))
    _, tabs = _check_htab(keys, ops, ep)
    for b in range(B):
        held = set(int(v) & 0xFFFFFFFF for v in tabs[b][tabs[b] != 0])
        assert held == set(int(k) for k in keys[b][ops[b] != CONTAINS])
    assert len(set(int(k) for k in keys[0][ops[0] != CONTAINS]) & set(int(k) for k in keys[1].ravel())) > 100


# ------------------------------------------------------------------------------------------------ same_key_earlier_in_round
def same_key(keys, cand):
    import torch
    lib = helpers.devtest_lib()
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 64)
    cand = np.ascontiguousarray(cand, dtype=np.uint8).reshape(-1, 64)
    d_k, d_c = _dev(keys), _dev(cand)
    d_o = torch.zeros(keys.size, dtype=torch.uint8, device="cuda")
    _ok(lib.bkdt_same_key(d_k.data_ptr(), d_c.data_ptr(), len(keys), d_o.data_ptr()))
    return _host(d_o, np.uint8).reshape(keys.shape) != 0


def test_same_key_earlier_in_round():
    rng = np.random.default_rng(301)
    K, C, what = [], [], []

    def add(name, keys, cand=None):
        K.append(np.asarray(keys, dtype=np.uint64).astype(np.uint32))
        C.append(np.ones(64, dtype=np.uint8) if cand is None else np.asarray(cand, dtype=np.uint8))
        what.append(name)

    same = np.full(64, 0xDEADBEEF)
    distinct = _random_keys(rng, 64)
    add("no candidate", same, np.zeros(64))
    for ln in (0, 31, 63):
        add("one candidate", same, np.arange(64) == ln)
    add("64 distinct keys", distinct)
    add("64 distinct keys, consecutive", np.arange(64) + 0xFFFFFFC0)
    for bit in range(32):
        k = distinct.copy()
        i, j = (int(x) for x in rng.choice(64, 2, replace=False))
        k[j] = k[i] ^ np.uint32(1 << bit)
        add(f"a pair that differs in bit {bit}", k)
        add(f"two lanes, bit {bit}", k, (np.arange(64) == i) | (np.arange(64) == j))
    for low in (8, 16, 24):
        k = distinct.copy()
        for _ in range(3):
            i, j = (int(x) for x in rng.choice(64, 2, replace=False))
            hi = (int(k[i]) >> low) ^ int(rng.integers(1, 1 << (32 - low)))
            k[j] = (hi << low) | (int(k[i]) & ((1 << low) - 1))
        add(f"pairs equal in the low {low} bits only", k)
    for groups in (2, 3):
        k = distinct.copy()
        lanes = rng.permutation(64)
        for g in range(groups):
            k[lanes[5 * g:5 * g + 2 + g]] = k[lanes[5 * g]]
        add(f"{groups} groups of equal keys", k)
        k = rng.integers(0, groups, 64).astype(np.uint64) * 0x01010101 + 5
        add(f"{groups} keys in 64 lanes", k)
    add("all 64 equal", same)
    add("all equal, key 0", np.zeros(64))
    add("all equal, key 0xFFFFFFFF", np.full(64, EMPTY))
    # lanes that are no candidates carry a candidate's key: they neither are duplicates nor make one
    k = distinct.copy()
    k[:32] = k[32:]
    add("non-candidates with a candidate's key, in front", k, np.arange(64) >= 32)
    add("non-candidates with a candidate's key, behind", k, np.arange(64) < 32)
    c = np.ones(64); c[10] = 0
    k = distinct.copy(); k[10] = k[3]; k[40] = k[3]
    add("a non-candidate between two equal candidates", k, c)
    for _ in range(40):
        add("random, few keys", rng.choice(distinct[:int(rng.integers(1, 40))], 64), rng.integers(0, 4, 64) != 0)
    K, C = np.stack(K), np.stack(C)
    got = same_key(K, C)
    for r in range(len(K)):
        want = np.array([bool(C[r, ln]) and bool(((K[r, :ln] == K[r, ln]) & (C[r, :ln] != 0)).any()) for ln in range(64)])
        assert np.array_equal(got[r], want), (what[r], np.nonzero(got[r] != want)[0].tolist())
    assert sum(int(g.sum()) for g in got) > 300
