// consensus_key, consensus_key_index and the serial consensus_best of mc-slam_amd/csrc/mcorb_consensus.h as a stand-alone program,
// built by tests/test_consensus_cpu.py with -fsanitize=address,undefined.  Prints "bad=<count>"; exit status 0 iff bad == 0.
//   at 10, 14 and 18 index bits   a model that is not valid is 0 and decodes to -1; a higher count wins; equal counts go to the
//                                 lower index; the round trip holds at index 0, at 2^bits - 1 and at count INT32_MAX
//   the essential family          the two-field key it had before -- (count + 1) << 18 | (16383 - h) << 4 | (15 - c), restated
//                                 here -- orders every pair of a set of slots exactly as the 18-bit key over slot = 10 h + c does
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "mcorb_consensus.h"
#include "mcorb_ess.h"

using namespace mcorb;

static int bad = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            bad++;                                                   \
            printf("line %d: %s\n", __LINE__, #x);                   \
        }                                                            \
    } while (0)

template <int kBits>
static void check_bits()
{
    const int last = (1 << kBits) - 1;
    const int32_t counts[] = {0, 1, 2, 1000, INT32_MAX - 1, INT32_MAX};
    const int indices[] = {0, 1, 2, last / 2, last - 1, last};
    CHECK(consensus_key_index<kBits>(0) == -1);
    for (int32_t c : counts)
        for (int i : indices) {
            CHECK(consensus_key<kBits>(0, c, i) == 0);
            const uint64_t k = consensus_key<kBits>(1, c, i);
            CHECK(k != 0);                                       // (a model with no inlier still beats no model)
            CHECK(consensus_key_index<kBits>(k) == i);           // the round trip
            CHECK((k >> kBits) == (uint64_t)c + 1);
            for (int32_t c2 : counts)
                for (int i2 : indices) {
                    const uint64_t k2 = consensus_key<kBits>(1, c2, i2);
                    if (c2 > c) CHECK(k2 > k);                   // a higher count wins at any index
                    if (c2 == c && i2 < i) CHECK(k2 > k);        // equal counts go to the lower index
                    if (c2 == c && i2 == i) CHECK(k2 == k);
                }
        }
    // the serial arg-max: ties to the lowest index, models that are not valid never win and are not counted
    const int32_t valid[] = {0, 1, 1, 0, 1, 1}, count[] = {9, 3, 7, 9, 7, 0};
    const ConsensusBest b = consensus_best<kBits>(6, [&](int i) { return valid[i]; }, [&](int i) { return count[i]; });
    CHECK(consensus_key_index<kBits>(b.key) == 2 && b.n_models == 4);
    const ConsensusBest none = consensus_best<kBits>(6, [&](int) { return 0; }, [&](int i) { return count[i]; });
    CHECK(none.key == 0 && none.n_models == 0 && consensus_key_index<kBits>(none.key) == -1);
    const ConsensusBest empty = consensus_best<kBits>(0, [&](int) { return 1; }, [&](int) { return 1; });
    CHECK(empty.key == 0 && empty.n_models == 0);
}

// the essential family's key as it was: the hypothesis in 14 bits above the root in 4
static uint64_t old_ess_key(int32_t valid, int32_t count, int slot)
{
    const int h = slot / kEssRoots, c = slot % kEssRoots;
    return valid ? (((uint64_t)count + 1) << 18) | ((uint64_t)(16383 - h) << 4) | (uint64_t)(15 - c) : 0;
}
static int old_ess_key_slot(uint64_t key)
{
    if (!key) return -1;
    return (16383 - (int)((key >> 4) & 16383)) * kEssRoots + (15 - (int)(key & 15));
}
static int sign(uint64_t a, uint64_t b) { return a < b ? -1 : a > b ? 1 : 0; }

static void check_ess()
{
    static_assert(kEssRoots == 10 && kEssKeyBits == 18 && MCORB_ESS_MAX_ITERATIONS == 16384, "the slots below");
    struct Slot { int h, c; };
    // the corners, and neighbours across a hypothesis boundary: (h, 9) next to (h + 1, 0)
    const Slot slots[] = {{0, 0}, {0, 1}, {0, 9}, {1, 0}, {1, 1}, {1, 9}, {2, 0}, {8191, 9}, {8192, 0}, {16382, 9}, {16383, 0}, {16383, 8}, {16383, 9}};
    const int32_t counts[] = {0, 1, 5, INT32_MAX};
    struct Entry { int32_t valid, count; int slot; };
    std::vector<Entry> entries;
    for (const Slot &s : slots)
        for (int32_t c : counts) {
            entries.push_back({1, c, s.h * kEssRoots + s.c});
            entries.push_back({0, c, s.h * kEssRoots + s.c});
        }
    for (const Entry &a : entries) {
        const uint64_t ka = consensus_key<kEssKeyBits>(a.valid, a.count, a.slot), oa = old_ess_key(a.valid, a.count, a.slot);
        CHECK(consensus_key_index<kEssKeyBits>(ka) == old_ess_key_slot(oa));
        CHECK(consensus_key_index<kEssKeyBits>(ka) == (a.valid ? a.slot : -1));
        for (const Entry &b : entries) {
            const uint64_t kb = consensus_key<kEssKeyBits>(b.valid, b.count, b.slot), ob = old_ess_key(b.valid, b.count, b.slot);
            CHECK(sign(ka, kb) == sign(oa, ob));
        }
    }
    // equal counts on either side of a hypothesis boundary: the lower hypothesis's last root wins
    CHECK(consensus_key<kEssKeyBits>(1, 5, 9) > consensus_key<kEssKeyBits>(1, 5, 10));
    CHECK(consensus_key<kEssKeyBits>(1, 5, 163829) > consensus_key<kEssKeyBits>(1, 5, 163830));
}

int main()
{
    check_bits<10>();
    check_bits<14>();
    check_bits<18>();
    static_assert(kSacKeyBits == 10 && kRelKeyBits == 14, "the families' index bits");
    check_ess();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
