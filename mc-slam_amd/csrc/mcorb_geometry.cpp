// mcorb_geometry.cpp -- ORBextractor's constructor tables and the level / cell / tile / resize geometry: host arithmetic only.
#include <math.h>
#include <string.h>

#include "mcorb_engine.h"

namespace mcorb {

static inline int cv_round_f(float v) { return (int)lrintf(v); }
static inline int cv_round_d(double v) { return (int)lrint(v); }
static inline int cv_floor_f(float v) { int i = (int)v; return i - (i > v); }
static inline int cv_ceil_f(float v) { int i = (int)v; return i + (i < v); }

// ---------------------------------------------------------------------------
// ORBextractor::ORBextractor (ORBextractor.cpp:408-468).  scaleFactor is a
// double member initialised from a float argument (ORBextractor.h:103).
// ---------------------------------------------------------------------------
int compute_tables(const mcorb_params &p, Tables &t)
{
    if (p.nlevels < 1 || p.nlevels > kMaxLevels || p.nfeatures < 1 || !(p.scale_factor > 1.0f)) {
        set_error("bad extractor parameters");
        return MCORB_E_ARG;
    }
    const int L = p.nlevels;
    const double sf = (double)p.scale_factor;
    t.nlevels = L;
    t.scale[0] = 1.0f;
    t.sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * sf);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < L; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
        t.scaled_patch[i] = (int)(31 * t.scale[i]);   // PATCH_SIZE*mvScaleFactor[level] (:879)
    }
    const float factor = (float)(1.0 / sf);
    float desired = (float)p.nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        t.quota[l] = cv_round_f(desired);
        sum += t.quota[l];
        desired *= factor;
    }
    t.quota[L - 1] = std::max(p.nfeatures - sum, 0);
    // umax (:450-467)
    const int HP = 15;
    int v, v0;
    const int vmax = cv_floor_f(HP * sqrtf(2.f) / 2 + 1);
    const int vmin = cv_ceil_f(HP * sqrtf(2.f) / 2);
    const double hp2 = HP * HP;
    for (v = 0; v < 16; v++) t.umax[v] = 0;
    for (v = 0; v <= vmax; ++v) t.umax[v] = cv_round_d(sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return MCORB_OK;
}

// cv::resize's table loop for one axis: x clamps (sx, fx), y keeps
// the fraction and clips the row indices at use.
void build_resize_axis(int ssize, int dsize, bool is_x, std::vector<ResizeTap> &out, int pad_to)
{
    const double scale = (double)ssize / dsize;
    const size_t first = out.size();
    for (int d = 0; d < dsize; d++) {
        float f = (float)((d + 0.5) * scale - 0.5);
        int s = cv_floor_f(f);
        f -= s;
        if (is_x) {
            if (s < 0) { f = 0; s = 0; }
            if (s >= ssize - 1) { f = 0; s = ssize - 1; }
        }
        int c0 = cv_round_f((1.f - f) * 2048.f), c1 = cv_round_f(f * 2048.f);
        c0 = std::min(std::max(c0, -32768), 32767);
        c1 = std::min(std::max(c1, -32768), 32767);
        int s0 = std::min(std::max(s, 0), ssize - 1);
        int s1 = std::min(std::max(s + 1, 0), ssize - 1);
        if (is_x && s + 1 >= ssize) { c0 = 2048; c1 = 0; }   // HResizeLinear tail: S[sx]*ONE
        ResizeTap t;
        t.s0 = (uint16_t)s0; t.s1 = (uint16_t)s1; t.c0 = (int16_t)c0; t.c1 = (int16_t)c1;
        out.push_back(t);
    }
    // padding: copies of the last tap, so that a kernel reading whole groups of `pad_to` never sees an out-of-range column
    const ResizeTap last = out.size() > first ? out.back() : ResizeTap{0, 0, 0, 0};
    while ((out.size() - first) % pad_to) out.push_back(last);
}

int build_geometry(const mcorb_params &p, const Tables &t, int W, int H, Geom &g, std::vector<ResizeTap> &taps,
                   std::vector<uint16_t> *lut)
{
    memset(&g, 0, sizeof(g));
    taps.clear();
    if (lut) lut->clear();
    g.nlevels = t.nlevels;
    size_t off = 0;
    int cells = 0, tiles = 0, cellCap = 4, buckets = 0;
    for (int l = 0; l < t.nlevels; l++) {
        LevelGeom &L = g.lv[l];
        const float sc = t.inv_scale[l];
        L.w = cv_round_f((float)W * sc);   // ORBextractor.cpp:1177-1178
        L.h = cv_round_f((float)H * sc);
        L.maxBorderX = L.w - kEdge + 3;
        L.maxBorderY = L.h - kEdge + 3;
        const float width = (float)(L.maxBorderX - kMinBorder);
        const float height = (float)(L.maxBorderY - kMinBorder);
        L.nCols = (int)(width / (float)kCellW);
        L.nRows = (int)(height / (float)kCellW);
        if (L.nCols < 1 || L.nRows < 1) {
            set_error("image too small for the reference's 35-px cell grid at level " + std::to_string(l));
            return MCORB_E_SIZE;
        }
        L.wCell = (int)ceilf(width / L.nCols);
        L.hCell = (int)ceilf(height / L.nRows);
        const SelectParams sp = make_select_params(kMinBorder, L.maxBorderX, kMinBorder, L.maxBorderY, t.quota[l], 1, 1);
        if (sp.nIni < 1) {
            set_error("image too tall: DistributeOctTree would have no root node");
            return MCORB_E_SIZE;
        }
        if (sp.nIni > 16) { set_error("image too wide (more than 16 root nodes)"); return MCORB_E_SIZE; }
        L.nIni = sp.nIni;
        L.hX = sp.hX;
        L.depth = sp.depth;
        L.nBuckets = sp.nIni << (2 * sp.depth);
        L.bucket0 = buckets;
        L.quota = t.quota[l];
        buckets += L.nBuckets + 1;
        if (lut) {   // path-code tables of this level (k_compact): code(x, y) = lut[L.lutx + x] | lut[L.luty + y]
            const int W0 = L.maxBorderX - kMinBorder, H0 = L.maxBorderY - kMinBorder;
            L.lutx = (uint32_t)lut->size();
            L.luty = L.lutx + (uint32_t)W0;
            lut->resize(lut->size() + (size_t)W0 + H0);
            path_code_tables(W0, H0, L.nIni, L.hX, L.depth, lut->data() + L.lutx, lut->data() + L.luty);
            while (lut->size() & 7) lut->push_back(0);
        }
        if (L.w > 4096 || L.h > 4096) { set_error("image larger than 4096 px"); return MCORB_E_SIZE; }
        L.pitch = (int)align_up((size_t)L.w, 64);
        L.off = (uint32_t)off;
        off += align_up((size_t)L.pitch * align_up((size_t)L.h, kBlurTileRows), 256);   // whole 16x8 tiles (blurred planes)
        L.cell0 = cells;
        cells += L.nCols * L.nRows;
        L.tilesX = (L.w + kBlurTW - 1) / kBlurTW;
        L.tilesY = (L.h + kBlurTH - 1) / kBlurTH;
        L.tile0 = tiles;
        tiles += L.tilesX * L.tilesY;
        cellCap = std::max(cellCap, ((L.wCell + 1) / 2) * ((L.hCell + 1) / 2));
        if (l > 0) {
            L.xtab = (uint32_t)taps.size();
            build_resize_axis(g.lv[l - 1].w, L.w, true, taps, 4);
            L.ytab = (uint32_t)taps.size();
            build_resize_axis(g.lv[l - 1].h, L.h, false, taps, 4);
        }
    }
    g.cells = cells;
    g.tiles = tiles;
    g.bucketTotal = buckets;
    g.cellCap = (int)align_up((size_t)cellCap, 4);
    g.imgBytes = (uint32_t)(off + 256);
    g.kcap = (int)align_up((size_t)p.nfeatures + 4 * t.nlevels + 48, 64);
    if (g.kcap > 65535) { set_error("nfeatures too large (k-NN index is 16 bits)"); return MCORB_E_ARG; }
    // default: one candidate slot per 4 level-0 pixels (measured: ~1 per 28 px on the synthetic rig frames)
    // device list: worst case (every cell full: one corner per 2x2 px survives the 3x3 NMS at most), so FAST itself can
    // never overflow; host copy: one slot per 4 level-0 pixels by default (~1 per 28 px measured on the synthetic rig
    // frames) -- it is only written when the quad-tree may go below the bucketing, i.e. for sparse levels
    g.candCap = (int)align_up((size_t)g.cells * g.cellCap, 4096);
    g.hostCandCap = p.cand_cap > 0 ? p.cand_cap : (int)align_up(std::max((size_t)65536, (size_t)W * H / 4), 4096);
    if (g.hostCandCap > g.candCap) g.hostCandCap = g.candCap;
    if (g.lv[0].nCols * g.lv[0].nRows * g.cellCap > kPickOrderMask) { set_error("image too large (pick order is 23 bits)"); return MCORB_E_SIZE; }
    return MCORB_OK;
}

int resize_windows(const Geom &g, const std::vector<ResizeTap> &taps, int win[2 * kMaxLevels])
{
    for (int l = 1; l < g.nlevels; l++) {
        const LevelGeom &D = g.lv[l];
        int maxc = 16, maxr = 2;
        for (int bx0 = 0; bx0 < D.w; bx0 += 256) {
            const int bx1 = std::min(bx0 + 255, D.w - 1);
            const int a = taps[D.xtab + bx0].s0 & ~15, b = taps[D.xtab + bx1].s1;
            maxc = std::max(maxc, ((b - a) / 16 + 1) * 16);
        }
        for (int by0 = 0; by0 < D.h; by0 += kResizeTileH) {
            const int by1 = std::min(by0 + kResizeTileH - 1, D.h - 1);
            maxr = std::max(maxr, (int)taps[D.ytab + by1].s1 - (int)taps[D.ytab + by0].s0 + 1);
        }
        win[2 * l] = maxc;
        win[2 * l + 1] = maxr;
        if ((size_t)maxc * maxr > 60000) { set_error("scale factor too large for the resize window"); return MCORB_E_ARG; }
    }
    return MCORB_OK;
}

}  // namespace mcorb
