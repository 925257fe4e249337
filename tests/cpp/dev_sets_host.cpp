// dev_sets_host.cpp - bk_dev_sets.h compiled for the host as it stands and run single-threaded against std::set
// (tests/test_host_devlogic.py puts an unchanged copy of the header beside a bk_dev_util.h of shims and compiles this with clang:
// the header's ext_vector_type is a clang extension).  The shims count the steps of the probe loops and give up after kMaxSteps
// between two helper calls; the loops of the LDS set that go through no shim are ended by an alarm.  A broken helper fails the
// run, it does not spin.
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "bk_dev_sets.h"

using namespace bk;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __func__, __LINE__); printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static std::vector<uint32_t> keys_of_bucket(uint32_t bucket, int n, std::mt19937_64 &rng)
{
    std::vector<uint32_t> out;
    while ((int)out.size() < n) {
        const uint32_t k = (uint32_t)rng();
        if (k != kLdsEmpty && lset_bucket(k) == bucket) out.push_back(k);
    }
    return out;
}

static int test_lset_random()
{
    std::mt19937_64 rng(11);
    std::vector<uint32_t> set(kLdsSet, kLdsEmpty);
    std::set<uint32_t> ref;
    std::vector<uint32_t> held;
    int looks = 0;
    while (ref.size() < kLdsSetFill) {
        uint32_t k = (uint32_t)rng();
        if (k == kLdsEmpty) continue;
        for (int q = 0; q < 4; q++, looks++) {
            // half of the look-ups for keys that are there
            const uint32_t l = (q & 1) && !held.empty() ? held[rng() % held.size()] : (uint32_t)rng();
            if (l == kLdsEmpty) continue;
            g_steps = 0;
            CHECK(lset_contains(set.data(), l) == (ref.count(l) != 0), "look-up %d of %08x with %zu keys held", looks, l, ref.size());
        }
        g_steps = 0;
        lset_insert(set.data(), k);
        if (rng() % 8 == 0) lset_insert(set.data(), k);         // again: nothing changes
        if (ref.insert(k).second) held.push_back(k);
    }
    CHECK(looks >= 6000, "%d look-ups", looks);
    std::multiset<uint32_t> got;
    for (uint32_t w : set) if (w != kLdsEmpty) got.insert(w);
    CHECK(got.size() == ref.size() && std::set<uint32_t>(got.begin(), got.end()) == ref, "the set holds %zu words for %zu keys", got.size(), ref.size());
    for (uint32_t k : ref) CHECK(lset_contains(set.data(), k), "key %08x of the full set is not found", k);
    for (int i = 0; i < 4096; i++) {
        const uint32_t k = (uint32_t)rng();
        if (k != kLdsEmpty) CHECK(lset_contains(set.data(), k) == (ref.count(k) != 0), "absent key %08x", k);
    }
    return 0;
}

static int test_lset_one_bucket()
{
    std::mt19937_64 rng(12);
    for (uint32_t bucket : {7u, kLdsBuckets - 1}) {
        for (int n : {5, 9, 64}) {
            std::vector<uint32_t> set(kLdsSet, kLdsEmpty);
            const std::vector<uint32_t> ks = keys_of_bucket(bucket, n + 8, rng);
            for (int i = 0; i < n; i++) {
                g_steps = 0;
                CHECK(!lset_contains(set.data(), ks[i]), "bucket %u: key %d seen before it came", bucket, i);
                lset_insert(set.data(), ks[i]);
                // one key after the other: slot i of the probe sequence, which goes on from the last bucket to bucket 0
                CHECK(set[(4 * bucket + i) % kLdsSet] == ks[i], "bucket %u: key %d is not in slot %d of the probe sequence", bucket, i, i);
            }
            for (int i = 0; i < n + 8; i++) {
                g_steps = 0;
                CHECK(lset_contains(set.data(), ks[i]) == (i < n), "bucket %u, %d keys: look-up of key %d", bucket, n, i);
            }
            uint32_t used = 0;
            for (uint32_t w : set) used += w != kLdsEmpty;
            CHECK(used == (uint32_t)n, "bucket %u: %u slots used for %d keys", bucket, used, n);
        }
    }
    return 0;
}

static int test_lset_empty_slot_key()
{
    // the key of a target start of 2^32 - 2 (mod 2^32): never inserted (k_wave keeps it in the HBM table), looked up like every other
    std::mt19937_64 rng(13);
    std::vector<uint32_t> set(kLdsSet, kLdsEmpty);
    CHECK(!lset_contains(set.data(), 0xFFFFFFFFu), "lset_contains(0xFFFFFFFF) is true on an empty set");
    uint32_t n = 0;
    while (n < kLdsSetFill) {
        const uint32_t k = (uint32_t)rng();
        if (k == kLdsEmpty || lset_contains(set.data(), k)) continue;
        lset_insert(set.data(), k);
        n++;
        if (n == 1) CHECK(!lset_contains(set.data(), 0xFFFFFFFFu), "lset_contains(0xFFFFFFFF) is true after one insert");
    }
    CHECK(!lset_contains(set.data(), 0xFFFFFFFFu), "lset_contains(0xFFFFFFFF) is true at the fill cap");
    for (uint32_t k : {0u, 1u, 0x80000000u, 0xFFFFFFFEu}) {
        std::vector<uint32_t> s2(kLdsSet, kLdsEmpty);
        CHECK(!lset_contains(s2.data(), k), "edge key %08x seen in an empty set", k);
        lset_insert(s2.data(), k);
        CHECK(lset_contains(s2.data(), k), "edge key %08x not found", k);
        CHECK(!lset_contains(s2.data(), 0xFFFFFFFFu) && !lset_contains(s2.data(), k ^ 2u), "beside edge key %08x", k);
    }
    return 0;
}

constexpr uint32_t kTs = 1024, kMask = kTs - 1;

static std::vector<uint32_t> keys_of_hash(uint32_t h, int n, std::mt19937_64 &rng)
{
    std::vector<uint32_t> out;
    while ((int)out.size() < n) {
        const uint32_t k = (uint32_t)rng();
        if (hash_key(k, kMask) == h) out.push_back(k);
    }
    return out;
}

static int test_htab_random()
{
    std::mt19937_64 rng(14);
    std::vector<unsigned long long> tab(kTs, 0);
    for (uint32_t epoch : {1u, 2u, 0x7FFFFFFFu}) {
        // contains / insert (k_heavy) in the first half, find_or_insert (k_wave) in the second; the table at most half full
        std::set<uint32_t> ref;
        std::vector<uint32_t> held;
        while (ref.size() < kTs / 2) {
            uint32_t k = rng() % 16 == 0 ? (rng() & 1 ? 0u : 0xFFFFFFFFu) : (uint32_t)rng();
            if (rng() % 3 == 0 && !held.empty()) k = held[rng() % held.size()];
            const bool was = ref.count(k) != 0;
            g_steps = 0;
            if (ref.size() < kTs / 4) {
                CHECK(htab_contains(tab.data(), kMask, epoch, k) == was, "epoch %u: contains(%08x) with %zu keys", epoch, k, ref.size());
                htab_insert(tab.data(), kMask, epoch, k);
            } else {
                uint32_t slot = 0xFFFFFFFFu;
                CHECK(htab_find_or_insert(tab.data(), kMask, epoch, k, slot) == was, "epoch %u: find_or_insert(%08x) with %zu keys", epoch, k, ref.size());
                CHECK(was || ((uint32_t)tab[slot] == k && (uint32_t)(tab[slot] >> 32) == epoch), "find_or_insert(%08x): slot %u does not hold the key", k, slot);
            }
            CHECK(htab_contains(tab.data(), kMask, epoch, k), "epoch %u: %08x is not found after it came", epoch, k);
            if (ref.insert(k).second) held.push_back(k);
        }
        CHECK(ref.count(0u) && ref.count(0xFFFFFFFFu), "keys 0 and 0xFFFFFFFF were among them");
        for (uint32_t k : ref) { g_steps = 0; CHECK(htab_contains(tab.data(), kMask, epoch, k), "epoch %u: key %08x lost", epoch, k); }
        for (int i = 0; i < 4096; i++) {
            const uint32_t k = (uint32_t)rng();
            g_steps = 0;
            CHECK(htab_contains(tab.data(), kMask, epoch, k) == (ref.count(k) != 0), "epoch %u: absent key %08x", epoch, k);
        }
        // the next epoch sees none of them (and takes their slots: three epochs of 512 keys in 1024 slots)
        const uint32_t next = epoch == 0x7FFFFFFFu ? 5u : epoch + 1;
        for (uint32_t k : ref) { g_steps = 0; CHECK(!htab_contains(tab.data(), kMask, next, k), "key %08x of epoch %u is seen at epoch %u", k, epoch, next); }
    }
    return 0;
}

static int test_htab_retract_and_epochs()
{
    std::mt19937_64 rng(15);
    for (uint32_t h : {517u, 1022u}) {                    // (from 1022 the probe sequence wraps the mask)
        std::vector<unsigned long long> tab(kTs, 0);
        const std::vector<uint32_t> k = keys_of_hash(h, 6, rng);
        const uint32_t e = 12;
        uint32_t sx = ~0u, sa = ~0u, sb = ~0u, sc = ~0u, s = ~0u;
        g_steps = 0;
        CHECK(!htab_find_or_insert(tab.data(), kMask, e, k[0], sx) && sx == h, "first key: slot %u", sx);
        CHECK(!htab_find_or_insert(tab.data(), kMask, e, k[1], sa) && sa == ((h + 1) & kMask), "second key: slot %u", sa);
        CHECK(!htab_find_or_insert(tab.data(), kMask, e, k[2], sb) && sb == ((h + 2) & kMask), "third key: slot %u", sb);
        htab_retract(tab.data(), sa, e);
        // the retracted key is not seen; its slot stays taken: the key behind it is still found, and a new one goes behind that
        CHECK(htab_find_or_insert(tab.data(), kMask, e, k[2], s), "the key that came before the retract is not found after it");
        CHECK(htab_find_or_insert(tab.data(), kMask, e, k[0], s), "the key in front of the tombstone is not found");
        CHECK(!htab_find_or_insert(tab.data(), kMask, e, k[3], sc) && sc == ((h + 3) & kMask), "a new key settles in slot %u", sc);
        CHECK(htab_find_or_insert(tab.data(), kMask, e, k[3], s), "the new key is not found");
        CHECK(!htab_find_or_insert(tab.data(), kMask, e, k[1], s) && s == ((h + 4) & kMask), "the retracted key: seen, or entered again in slot %u", s);
        CHECK(htab_find_or_insert(tab.data(), kMask, e, k[1], s), "the retracted key, entered again, is not found");
        CHECK(tab[sa] == ((unsigned long long)(e | kTombBit) << 32), "the tombstone is gone");
        // next epoch: entries and tombstone are stale, their slots are taken again in probe order
        g_steps = 0;
        for (int i = 0; i < 4; i++) CHECK(!htab_contains(tab.data(), kMask, e + 1, k[i]), "key %d of epoch %u seen at epoch %u", i, e, e + 1);
        CHECK(!htab_find_or_insert(tab.data(), kMask, e + 1, k[4], s) && s == h, "epoch %u: first key in slot %u", e + 1, s);
        CHECK(!htab_find_or_insert(tab.data(), kMask, e + 1, k[5], s) && s == sa, "epoch %u: the stale tombstone's slot is not taken (slot %u)", e + 1, s);
        htab_insert(tab.data(), kMask, e + 1, k[0]);
        CHECK((uint32_t)tab[sb] == k[0] && (uint32_t)(tab[sb] >> 32) == e + 1, "epoch %u: htab_insert does not take the third stale slot", e + 1);
        CHECK(htab_contains(tab.data(), kMask, e + 1, k[4]) && htab_contains(tab.data(), kMask, e + 1, k[5]) && htab_contains(tab.data(), kMask, e + 1, k[0])
              && !htab_contains(tab.data(), kMask, e + 1, k[1]), "epoch %u: membership", e + 1);
    }
    return 0;
}

int main()
{
    alarm(60);
    if (test_lset_random() || test_lset_one_bucket() || test_lset_empty_slot_key() || test_htab_random() || test_htab_retract_and_epochs()) return 1;
    printf("ok\n");
    return 0;
}
