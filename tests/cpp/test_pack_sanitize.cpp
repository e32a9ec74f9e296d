// The packed-input layouts of the local map's calls (mcorb_pack.h) as a stand-alone program under the sanitizers:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I mc-slam_amd/csrc tests/cpp/test_pack_sanitize.cpp
// The five blocks the library builds -- pose, RANSAC, a tracking call, the two mapping entries -- with the
// library's item types and small counts, zero-count items and a zero-size whole among them.  Every offset is a multiple of 32,
// no two items overlap, and the total covers the last item: every item is written end to end, with a value of its own, into a
// std::vector<uint8_t>(total), which the address sanitizer bounds, and read back.  Prints "bad=0".
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "mcorb_pack.h"

using namespace mcorb;

// a stack value: one counter, nothing owned
static_assert(std::is_trivially_copyable<Pack>::value && std::is_trivially_destructible<Pack>::value && sizeof(Pack) == sizeof(size_t), "Pack");

struct Item { size_t off, bytes; };

static int bad = 0;

static void expect(bool ok, const char *what, const char *name)
{
    if (!ok) { printf("%s: %s\n", name, what); bad++; }
}

// the items in the order they were added
static void check(const char *name, size_t total, const std::vector<Item> &items)
{
    std::vector<uint8_t> block(total);
    expect(total % Pack::kAlign == 0, "total is no multiple of 32", name);
    size_t end = 0;
    for (size_t i = 0; i < items.size(); i++) {
        const Item &it = items[i];
        expect(it.off % Pack::kAlign == 0, "an offset is no multiple of 32", name);
        expect(it.off >= end, "an item begins inside the one before it", name);
        if (i && items[i - 1].bytes == 0) expect(it.off == items[i - 1].off, "an item without elements takes space", name);
        end = it.off + it.bytes;
        if (it.bytes) memset(block.data() + it.off, (int)(i + 1), it.bytes);
    }
    expect(end <= total && total - end < Pack::kAlign, "total does not end with the last item", name);
    if (!items.empty() && items.back().bytes == 0) expect(total == items.back().off, "an item without elements takes space", name);
    for (size_t i = 0; i < items.size(); i++)
        for (size_t k = 0; k < items[i].bytes; k++)
            if (block[items[i].off + k] != (uint8_t)(i + 1)) { expect(false, "an item was overwritten by another", name); break; }
}

static void obs(const char *name, size_t n, bool lids, bool sac, size_t S, size_t ncams)
{
    const ObsLayout L(n, lids, sac, S, ncams);
    check(name, L.p.total,
          {{L.pose_job, sizeof(PoseJob)}, {L.sac_job, sac ? sizeof(SacJob) : 0}, {L.obs, n * sizeof(PoseObs)},
           {L.pt, n * (lids ? sizeof(int32_t) : 3 * sizeof(double))}, {L.cons, sac ? S * sizeof(int32_t) : 0},
           {L.cam_first, sac ? (ncams + 1) * sizeof(int32_t) : 0}, {L.cam_cons, sac ? S * sizeof(int32_t) : 0}, {L.is_first, sac ? n : 0}});
}

static void track(const char *name, size_t nf, size_t ncand, size_t total_kp)
{
    const TrackLayout L(nf, ncand, total_kp);
    check(name, L.p.total,
          {{L.items, nf * sizeof(TrItem)}, {L.views, nf * sizeof(mcorb_track_view)}, {L.cand, ncand * sizeof(int32_t)},
           {L.xy, total_kp * 2 * sizeof(float)}, {L.desc, total_kp * 32}});
}

static void map(const char *name, size_t nframes, size_t nF, size_t C, size_t nlevels, size_t nmi, size_t nkp, size_t nb, size_t ni, size_t nz)
{
    const MapLayout L(nframes, nF, C, nlevels, nmi, nkp, nb, ni, nz);
    check(name, L.p.total,
          {{L.frames, nframes * sizeof(MapFrameDev)}, {L.F, nF * sizeof(double)}, {L.K, C * 9 * sizeof(double)}, {L.sig, nlevels * sizeof(float)},
           {L.mi, nmi * sizeof(int32_t)}, {L.kp, nkp * sizeof(MapKp)}, {L.blocks, nb * sizeof(MapBlock)}, {L.items, ni * sizeof(MapItem)},
           {L.zlids, nz * sizeof(int32_t)}});
    std::vector<uint8_t> block(L.p.total);
    uint8_t *base = block.data();
    const MapArgs a = L.args(base, nullptr, (int)C);
    expect((const uint8_t *)a.K - base == (ptrdiff_t)L.K && (const uint8_t *)a.items - base == (ptrdiff_t)L.items, "args() and the offsets differ", name);
}

int main()
{
    Pack p;
    check("nothing", p.total, {});
    expect(p.add<double>(0) == 0 && p.total == 0, "an empty item moved the total", "nothing");
    expect(p.add<uint8_t>(1) == 0 && p.add<uint8_t>(33) == 32 && p.add<int32_t>(0) == 96 && p.total == 96, "add()", "three items");

    obs("pose, ids", 7, true, false, 0, 0);
    obs("pose, points", 5, false, false, 0, 0);
    obs("pose, one observation", 1, true, false, 0, 0);
    obs("sac, ids", 9, true, true, 4, 2);
    obs("sac, points, 16 cameras", 33, false, true, 33, 16);
    obs("sac, one camera", 3, false, true, 1, 1);
    track("track, a rig slot's frame", 1, 13, 0);
    track("track, host arrays", 1, 13, 21);
    track("track, one candidate and one keypoint", 1, 1, 1);
    track("track, one frame of a slot", 1, 3, 0);
    track("track, five frames", 5, 77, 0);
    track("track, frames without candidates", 2, 0, 0);
    track("track, 32 frames", 32, 32 * 257 + 1, 0);
    map("neighbours", 3, 2 * 2 * 2 * 9, 2, 8, 40, 55, 3, 70, 11);
    map("neighbours, none", 1, 0, 1, 1, 4, 4, 0, 0, 0);
    map("neighbours, host-only (no blocks)", 2, 9, 1, 8, 6, 9, 0, 0, 5);
    map("new", 2, 0, 2, 8, 24, 31, 2, 65, 0);
    map("new, no match needs a record", 2, 0, 3, 4, 9, 9, 0, 0, 0);
    printf("bad=%d\n", bad);
    return bad != 0;
}
