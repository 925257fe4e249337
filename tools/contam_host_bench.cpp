// contam_host_bench - the contaminant rule of `align -H` (k_contam) as a plain multi-threaded host loop, timed: the figure the
// device matcher is measured against (profiles/NOTES.md).  Not part of the product.  Byte-per-base compares with an exit at the second
// mismatch, overlap lengths longest first, entries in file order - no trie, no packing.
//   c++ -O3 -std=c++17 -pthread -o contam_host_bench tools/contam_host_bench.cpp
//   contam_host_bench <reads> <read length> <threads> [adaptor length = 33]
// Synthetic input: random reads, every 10th carrying the last 12 bases of the 5' adaptor in front and the first 12 of the 3' one behind;
// two entries (one per end), trims 0.  Prints reads, seconds, reads per second and the sum of the cuts.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

static int overlap(const uint8_t *read, int n, const uint8_t *ent, int elen, bool five, int trim)
{
    if (n < 20 || n > 2000) return 0;
    for (int L = n < elen ? n : elen; L > trim; L--) {
        const uint8_t *r = five ? read : read + n - L, *c = five ? ent + elen - L : ent;
        int mism = 0;
        for (int i = 0; i < L && mism < 2; i++) {
            const uint8_t rb = r[i] & 7;
            mism += rb == 4 || (c[i] != 4 && c[i] != rb);
        }
        if (mism < 2) return L - trim;
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: contam_host_bench <reads> <read length> <threads> [adaptor length]\n"); return 2; }
    const size_t n = strtoull(argv[1], nullptr, 10);
    const int len = atoi(argv[2]), nt = atoi(argv[3]), alen = argc > 4 ? atoi(argv[4]) : 33;
    if (len < 24 || len > 2000 || nt < 1 || alen < 12 || alen > 200) return 2;
    std::vector<uint8_t> a5(alen), a3(alen), bases(n * (size_t)len);
    uint64_t x = 88172645463325252ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    for (int i = 0; i < alen; i++) { a5[i] = rnd() & 3; a3[i] = rnd() & 3; }
    for (size_t i = 0; i < bases.size(); i++) bases[i] = rnd() & 3;
    for (size_t r = 0; r < n; r += 10) {
        memcpy(&bases[r * len], &a5[alen - 12], 12);
        memcpy(&bases[r * len + len - 12], a3.data(), 12);
    }
    std::vector<uint16_t> out(2 * n);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            for (size_t r = n * t / nt; r < n * (t + 1) / nt; r++) {
                out[2 * r] = (uint16_t)overlap(&bases[r * len], len, a5.data(), alen, true, 0);
                out[2 * r + 1] = (uint16_t)overlap(&bases[r * len], len, a3.data(), alen, false, 0);
            }
        });
    for (auto &t : th) t.join();
    const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    uint64_t sum = 0;
    for (uint16_t v : out) sum += v;
    printf("reads %zu length %d threads %d adaptor %d: %.3f s, %.1f M reads/s, cuts sum %llu\n", n, len, nt, alen, s, 1e-6 * n / s, (unsigned long long)sum);
    return 0;
}
