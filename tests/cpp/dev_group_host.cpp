// The grouping table of the request passes (biokanga_amd/csrc/bk_dev_group.h, the file as it stands) on the host, against std::map:
// tests/test_host_dev_group.py puts the header beside a stand-in for bk_dev_util.h - one thread, the atomics as plain accesses that count
// their steps and give up after a bound - and compiles this file.  A request is its index; its key is keys[index]; the harness supplies
// the hash.  Prints "hash <a> <b> <value>" lines for the test to check against its own statement of the mix, then "ok".
#include <cinttypes>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "bk_dev_group.h"

using namespace bk;

#define CHECK(cond, ...)                                                                                                                   \
    do {                                                                                                                                   \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); exit(1); }                           \
    } while (0)

// the two layouts the passes have: owner at offset 0 (bk::JctSlot) and at offset 8 (bk::DupSlot)
struct alignas(16) Slot0 { uint32_t owner, a, b, c; };
struct alignas(16) Slot8 { unsigned long long a; uint32_t owner, c; };
static_assert(offsetof(Slot0, owner) == 0 && offsetof(Slot8, owner) == 8 && sizeof(Slot0) == 16 && sizeof(Slot8) == 16, "layouts");
template <class Slot> Slot empty_slot();
template <> Slot0 empty_slot<Slot0>() { return Slot0{kGroupEmpty, 7u, 0u, 9u}; }
template <> Slot8 empty_slot<Slot8>() { return Slot8{0x0123456789abcdefULL, kGroupEmpty, 5u}; }

template <class Slot> static std::vector<Slot> cleared(uint64_t slots)
{
    std::vector<Slot> table(slots);
    memset(table.data(), 0x5a, slots * sizeof(Slot));
    const Slot empty = empty_slot<Slot>();
    k_group_clear<Slot>(table.data(), slots, empty);                  // (the stand-in's grid is one thread: the stride loop visits every slot)
    for (uint64_t i = 0; i < slots; i++) CHECK(!memcmp(&table[i], &empty, sizeof(Slot)), "slot %" PRIu64 " is not the clear value", i);
    return table;
}

// every request claims, then every request finds again; hash_of(key) is what the caller of the header would pass.  Returns the groups.
template <class Slot, class Hash> static size_t run(const char *what, const std::vector<uint64_t> &keys, uint64_t slots, Hash hash_of)
{
    CHECK(slots && !(slots & (slots - 1)), "%s: the harness wants a power of two", what);
    const uint64_t mask = slots - 1;
    const uint32_t n = (uint32_t)keys.size();
    std::vector<Slot> table = cleared<Slot>(slots);
    struct Group { uint64_t slot; uint32_t owner; };
    std::map<uint64_t, Group> want;
    std::set<uint64_t> taken;
    for (uint32_t j = 0; j < n; j++) {
        g_steps = 0;
        const uint64_t slot = group_claim(table.data(), mask, hash_of(keys[j]), j, [&](uint32_t o) { return keys[o] == keys[j]; });
        CHECK(slot < slots, "%s: request %u got no slot", what, j);
        auto it = want.find(keys[j]);
        if (it == want.end()) {
            CHECK(taken.insert(slot).second, "%s: request %u opened a group in the slot of another", what, j);
            CHECK(table[slot].owner == j, "%s: request %u claimed slot %" PRIu64 " but does not own it", what, j, slot);
            want[keys[j]] = Group{slot, j};
        } else {
            CHECK(slot == it->second.slot, "%s: request %u joined slot %" PRIu64 ", its group has %" PRIu64, what, j, slot, it->second.slot);
            CHECK(table[slot].owner == it->second.owner, "%s: the owner of slot %" PRIu64 " changed", what, slot);
        }
    }
    uint64_t owned = 0;
    const Slot empty = empty_slot<Slot>();
    for (uint64_t i = 0; i < slots; i++) {
        if (table[i].owner != kGroupEmpty) { owned++; table[i].owner = kGroupEmpty; }
        CHECK(!memcmp(&table[i], &empty, sizeof(Slot)), "%s: a claim wrote more than the owner of slot %" PRIu64, what, i);
    }
    CHECK(owned == want.size(), "%s: %" PRIu64 " slots owned, %zu groups", what, owned, want.size());
    for (const auto &kv : want) table[kv.second.slot].owner = kv.second.owner;
    for (uint32_t j = 0; j < n; j++) {
        Slot found;
        const uint64_t slot = group_find(table.data(), mask, hash_of(keys[j]), j, [&](uint32_t o) { return keys[o] == keys[j]; }, found);
        CHECK(slot < slots && !memcmp(&found, &table[slot], sizeof(Slot)), "%s: request %u was not handed the contents of its slot", what, j);
        CHECK(slot == want[keys[j]].slot, "%s: request %u found slot %" PRIu64 ", its group has %" PRIu64, what, j, slot, want[keys[j]].slot);
    }
    // a key nobody inserted, as request n: no slot - at the first empty slot, or after `slots` steps of a full table
    const uint64_t absent = ~0ULL - 12345;
    CHECK(!want.count(absent), "%s: the harness's absent key is there", what);
    Slot unused;
    const uint64_t none = group_find(table.data(), mask, hash_of(absent), n, [&](uint32_t o) { return keys[o] == absent; }, unused);
    CHECK(none == ~0ULL, "%s: a key never inserted was found in slot %" PRIu64, what, none);
    return want.size();
}

// slots + 1 distinct keys: the last one finds every slot another group's and gives up after exactly `slots` looks
template <class Slot, class Hash> static void overfull(const char *what, uint64_t slots, Hash hash_of)
{
    const uint64_t mask = slots - 1;
    std::vector<Slot> table = cleared<Slot>(slots);
    std::vector<uint64_t> keys(slots + 1);
    for (uint64_t j = 0; j <= slots; j++) keys[j] = 1000 + 7 * j;
    for (uint32_t j = 0; j < slots; j++)
        CHECK(group_claim(table.data(), mask, hash_of(keys[j]), j, [&](uint32_t o) { return keys[o] == keys[j]; }) < slots, "%s: request %u got no slot", what, j);
    const uint32_t j = (uint32_t)slots;
    g_steps = 0; g_loads = 0;
    const uint64_t slot = group_claim(table.data(), mask, hash_of(keys[j]), j, [&](uint32_t o) { return keys[o] == keys[j]; });
    CHECK(slot == ~0ULL, "%s: request %u of %u got slot %" PRIu64 " of a full table", what, j, j, slot);
    CHECK(g_loads == slots && g_steps == slots, "%s: gave up after %llu looks (%llu atomic steps), the table has %" PRIu64 " slots", what, g_loads, g_steps, slots);
    for (uint64_t i = 0; i < slots; i++) CHECK(table[i].owner < slots, "%s: slot %" PRIu64 " lost its owner", what, i);
}

template <class Slot> static void all(const char *layout)
{
    std::mt19937_64 rng(20240611);
    char what[128];
    const auto mixed = [](uint64_t k) { return group_hash(k, k >> 7); };
    const auto one_slot = [](uint64_t) { return (uint64_t)0xfeedULL; };
    for (const uint32_t n : {1u, 2u, 63u, 64u, 257u, 1024u, 4096u}) {
        // heavy repetition: about n / 8 + 1 keys; and n distinct keys, which fill a table of exactly n slots
        std::vector<uint64_t> rep(n), dist(n);
        for (auto &k : rep) k = 17 + rng() % (n / 8 + 1);
        for (uint32_t j = 0; j < n; j++) dist[j] = (rng() << 16) | j;
        uint64_t pow2 = 1;
        while (pow2 < n) pow2 <<= 1;
        for (const uint64_t slots : {2 * pow2, pow2}) {
            if (slots < n) continue;
            snprintf(what, sizeof(what), "%s, %u requests with repeats, %" PRIu64 " slots", layout, n, slots);
            run<Slot>(what, rep, slots, mixed);
            snprintf(what, sizeof(what), "%s, %u distinct requests, %" PRIu64 " slots", layout, n, slots);
            CHECK(run<Slot>(what, dist, slots, mixed) == n, "%s: groups", what);
            if (n <= 1024) {                                          // (quadratic: every probe sequence starts at one slot)
                snprintf(what, sizeof(what), "%s, %u requests with repeats, %" PRIu64 " slots, one hash", layout, n, slots);
                run<Slot>(what, rep, slots, one_slot);
                snprintf(what, sizeof(what), "%s, %u distinct requests, %" PRIu64 " slots, one hash", layout, n, slots);
                run<Slot>(what, dist, slots, one_slot);
            }
        }
    }
    for (const uint64_t slots : {1ULL, 2ULL, 64ULL, 1024ULL}) {
        snprintf(what, sizeof(what), "%s, a table of %" PRIu64 " slots and one request more", layout, slots);
        overfull<Slot>(what, slots, mixed);
        overfull<Slot>(what, slots, one_slot);
    }
}

int main()
{
    all<Slot0>("owner at 0");
    all<Slot8>("owner at 8");
    const uint64_t pairs[][2] = {{0, 0}, {1, 0}, {0, 1}, {0x0000000100000064ULL, 0x00000005000000c8ULL}, {~0ULL, ~0ULL}, {0x123456789abcdef0ULL, 42}};
    for (const auto &p : pairs) printf("hash %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", p[0], p[1], group_hash(p[0], p[1]));
    printf("ok\n");
    return 0;
}
