// the interval slot arithmetic of biokanga_amd/csrc/bk_iv_slot.h on the host: slot function and decode are inverse, by position and by
// read, over the batch sizes of tests/test_gpu_prep_search0.py, both strand settings and 1 .. 16 cores per strand
#include <cstdint>
#include <algorithm>
#include <cstdio>
#include <vector>

#include "bk_iv_slot.h"

int main()
{
    const uint32_t sizes[] = {1, 63, 64, 65, 257, 1500};
    unsigned long long checked = 0;
    for (uint32_t n : sizes)
        for (int strands = 1; strands <= 2; strands++)
            for (uint32_t cores = 1; cores <= 16; cores++) {
                // an active list with holes: every third read is not on it, so that position and read number differ behind the first hole
                std::vector<uint32_t> act;
                for (uint32_t r = 0; r < n; r++)
                    if (n < 3 || r % 3 != 1) act.push_back(r);
                std::vector<uint8_t> seen((size_t)2 * cores * n, 0);
                for (uint32_t by_read = 0; by_read <= 1; by_read++) {
                    std::fill(seen.begin(), seen.end(), 0);
                    for (uint32_t a = 0; a < act.size(); a++)
                        for (int st = 2 - strands; st <= 1; st++)
                            for (int c = 0; c < (int)cores; c++) {
                                const uint32_t r = act[a];
                                const uint64_t slot = bk::iv_slot_at(cores, n, bk::iv_index(by_read, a, r), st, c);
                                if (slot >= seen.size() || slot > 0xFFFFFFFFull) { printf("slot %llu out of range (n %u cores %u)\n", (unsigned long long)slot, n, cores); return 1; }
                                if (seen[slot]++) { printf("slot %llu taken twice (n %u cores %u by_read %u)\n", (unsigned long long)slot, n, cores, by_read); return 1; }
                                uint32_t index;
                                int st2, c2;
                                bk::iv_slot_split(slot, cores, n, index, st2, c2);
                                if (st2 != st || c2 != c || index != (by_read ? r : a) || bk::iv_index_read(by_read, index, act.data()) != r) {
                                    printf("n %u cores %u by_read %u: (a %u, r %u, strand %d, core %d) -> slot %llu -> (index %u, strand %d, core %d)\n", n, cores, by_read,
                                           a, r, st, c, (unsigned long long)slot, index, st2, c2);
                                    return 1;
                                }
                                checked++;
                            }
                }
            }
    printf("%llu slots\nok\n", checked);
    return 0;
}
