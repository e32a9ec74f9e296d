"""The stage matrix: small, odd image geometries that steer the extraction job (k_resize, k_fast_cells, k_compact, k_blur,
k_describe_fused) into each of its shape-dependent variants, the contents they are run on, and the helpers that compare one
image's stages with the oracle element by element.

Three parts:
  1. geometry(): the launch arithmetic of build_geometry / fast_cell_table / fast_layout / resize_windows / launch_pyramid /
     launch_compact restated from the formulas (mcorb_geometry.cpp, mcorb_kernels.hip).  It never loads the library: the level
     sizes and the resize tap tables come from the oracle, so the coverage claim is checked on a machine without a GPU.
  2. CONTENTS and CASES: what is run.  tags() says what a case reaches; CHECKLIST is what all cases together must reach
     (test_stage_cases_cpu.py asserts it tag by tag).
  3. oracle_stages() / diff_*(): the oracle's per-level expectation of an image and the comparisons with messages that name the
     level and the first differing element (test_gpu_stages.py, scripts/gpu_stage_check.py)."""
import math
from collections import namedtuple

import numpy as np

import oracle_lib as O

EDGE = 19            # EDGE_THRESHOLD (kEdge)
MIN_BORDER = 16      # EDGE_THRESHOLD - 3 (kMinBorder)
CELL = 35            # W of ComputeKeyPointsOctTree (kCellW)
RESIZE_ROWS = 32     # output rows per k_resize workgroup (kResizeTileH); 8 per wave
RESIZE_COLS = 256    # output columns per k_resize workgroup
RESIZE_WINDOW_MAX = 60000   # resize_windows refuses a larger LDS window (bytes)
COMPACT_COPIES = 4   # kCompactCopies
SMALL_BATCH = 8      # launch_compact: up to 8 images run 1024 threads; the engine's host-mapped results batch (kSmallBatch)
KEEP_ALL = 8000      # the budget at which the oracle keeps every candidate of the small cases
KEEP_ALL_PIXELS = 150000
MAX_PIXELS = 700000

_f32 = np.float32


def _align_up(v, a):
    return (v + a - 1) // a * a


# --------------------------------------------------------------------------------------------
# 1. the launch arithmetic
# --------------------------------------------------------------------------------------------
def _axis(size, cells_other=None):
    """one axis of a level's cell grid (build_geometry, fast_cell_table): size = the level's w or h"""
    max_border = size - EDGE + 3
    span = max_border - MIN_BORDER
    n = int(_f32(span) / _f32(CELL))
    return max_border, span, n


def _cells_1d(max_border, n, cell, skip_margin):
    """per cell of one axis: (ini, roi, evaluated, state); state = 'on', 'skipped' (the reference's `ini >= maxBorder - margin`
    rule), 'beyond' (skipped, and the start lies at or beyond maxBorder) or 'short' (not skipped, but the clamped ROI has at most
    6 pixels: FAST has nothing to evaluate)"""
    out = []
    for c in range(n):
        ini = MIN_BORDER + c * cell
        roi = min(ini + cell + 6, max_border) - ini
        ev = roi - 6
        if ini >= max_border:
            state = "beyond"
        elif ini >= max_border - skip_margin:
            state = "skipped"
        elif ev <= 0:
            state = "short"
        else:
            state = "on"
        out.append((ini, roi, ev, state))
    return out


def level_sizes(W, H, nlevels, scale_factor):
    ex = O.OracleExtractor(1000, scale_factor, nlevels)
    return [ex.level_size(l, W, H) for l in range(nlevels)]


def _taps(ssize, dsize):
    s0 = O.resize_tables(ssize, dsize)[0].astype(np.int64)
    return s0, np.minimum(s0 + 1, ssize - 1)


def geometry(W, H, nlevels, scale_factor, sizes=None, quotas=None):
    """-> dict(levels=[per-level dict], job=dict) or raises ValueError where build_geometry / resize_windows refuse"""
    sizes = sizes or level_sizes(W, H, nlevels, scale_factor)
    levels = []
    cell_cap, cells, tiles = 4, 0, 0
    tp_pitch, tile_rows = 0, 0
    for l, (w, h) in enumerate(sizes):
        mbx, spanx, ncols = _axis(w)
        mby, spany, nrows = _axis(h)
        if ncols < 1 or nrows < 1:
            raise ValueError("level %d (%dx%d) too small for the 35-px cell grid" % (l, w, h))
        wcell = int(math.ceil(_f32(spanx) / _f32(ncols)))
        hcell = int(math.ceil(_f32(spany) / _f32(nrows)))
        n_ini = int(math.floor(float(_f32(spanx) / _f32(spany)) + 0.5))   # roundf of a float quotient
        if n_ini < 1 or n_ini > 16:
            raise ValueError("level %d: nIni %d" % (l, n_ini))
        if w > 4096 or h > 4096:
            raise ValueError("level larger than 4096 px")
        xs = _cells_1d(mbx, ncols, wcell, 6)    # iniX >= maxBorderX - 6
        ys = _cells_1d(mby, nrows, hcell, 3)    # iniY >= maxBorderY - 3
        L = dict(level=l, w=w, h=h, maxBorderX=mbx, maxBorderY=mby, nCols=ncols, nRows=nrows, wCell=wcell, hCell=hcell, nIni=n_ini,
                 xs=xs, ys=ys, last_col=xs[-1], last_row=ys[-1],
                 phases=sorted({(MIN_BORDER + cj * wcell) & 3 for cj in range(ncols)}),
                 max_roi_rows=max([r for _, r, _, s in ys if s == "on"] or [0]),
                 W0=spanx, H0=spany)
        cell_cap = max(cell_cap, ((wcell + 1) // 2) * ((hcell + 1) // 2))
        cells += ncols * nrows
        tiles += ((w + 127) // 128) * ((h + 31) // 32)    # k_blur's 128 x 32 workgroup tiles
        tp_pitch = max(tp_pitch, ((3 + wcell + 6 + 15) >> 4) << 4)
        tile_rows = max(tile_rows, hcell + 6)
        if l > 0:
            sw, sh = sizes[l - 1]
            x0, x1 = _taps(sw, w)
            y0, y1 = _taps(sh, h)
            maxc, maxr = 16, 2
            for bx0 in range(0, w, RESIZE_COLS):
                bx1 = min(bx0 + RESIZE_COLS - 1, w - 1)
                a, b = int(x0[bx0]) & ~15, int(x1[bx1])
                maxc = max(maxc, ((b - a) // 16 + 1) * 16)
            for by0 in range(0, h, RESIZE_ROWS):
                by1 = min(by0 + RESIZE_ROWS - 1, h - 1)
                maxr = max(maxr, int(y1[by1]) - int(y0[by0]) + 1)
            if maxc * maxr > RESIZE_WINDOW_MAX:
                raise ValueError("level %d: resize window %dx%d too large" % (l, maxc, maxr))
            chunks = (maxc >> 4) * maxr
            nf = (chunks + 255) // 256
            L["resize"] = dict(pitch=maxc, rows=maxr, loads=nf, variant=4 if nf <= 4 else (8 if nf <= 8 else 0),
                               aligned16=all(int(x0[b]) % 16 == 0 for b in range(0, w, RESIZE_COLS)),
                               last_block_w=w - RESIZE_COLS * ((w - 1) // RESIZE_COLS),
                               last_block_h=h - RESIZE_ROWS * ((h - 1) // RESIZE_ROWS),
                               h_mod32=h % 32, h_mod8=h % 8, w_mod4=w % 4)
        levels.append(L)
    job = dict(tp=48 if tp_pitch <= 48 else (64 if tp_pitch <= 64 else 80), tile_rows=tile_rows,
               max_roi_rows=max(L["max_roi_rows"] for L in levels), min_roi_rows=min(L["max_roi_rows"] for L in levels),
               cell_cap=_align_up(cell_cap, 4), cells=cells, tiles=tiles, nlevels=len(sizes))
    if quotas is not None:
        job["compact_copies"] = compact_copies(levels, quotas)
    return dict(levels=levels, job=job)


def select_depth(n_ini, quota):
    d = 1
    while d < 5 and n_ini * (1 << (2 * d)) < quota:
        d += 1
    return d


def compact_copies(levels, quotas):
    """launch_compact: four private copies of the bucket tables where they fit 64 KiB of LDS, else one"""
    maxb = maxc = 1
    maxwh = 2
    for L, q in zip(levels, quotas):
        maxb = max(maxb, L["nIni"] << (2 * select_depth(L["nIni"], int(q))))
        maxc = max(maxc, L["nCols"] * L["nRows"])
        maxwh = max(maxwh, L["W0"] + L["H0"])
    bkt = (maxb + 1 + 3) & ~3
    cells_cap = (maxc + 8 + 7) & ~7
    tail = (cells_cap + maxwh + 8) * 2
    return COMPACT_COPIES if 2 * COMPACT_COPIES * bkt * 4 + tail <= 64 * 1024 else 1


def compact_threads(nimg):
    return 1024 if nimg <= SMALL_BATCH else 512


# --------------------------------------------------------------------------------------------
# 2. contents and cases
# --------------------------------------------------------------------------------------------
def _rng(name, W, H):
    return np.random.default_rng([sum(name.encode()), W, H])


def _noise(W, H):
    return _rng("noise", W, H).integers(0, 256, (H, W)).astype(np.uint8)


def _binary(W, H):
    return (_rng("binary", W, H).integers(0, 2, (H, W)) * 255).astype(np.uint8)


def _checker(n):
    def gen(W, H):
        y, x = np.mgrid[0:H, 0:W]
        return ((((x // n) + (y // n)) & 1) * 255).astype(np.uint8)
    return gen


def _lattice4_const(W, H):
    img = np.full((H, W), 40, np.uint8)
    img[1::4, 2::4] = 200
    return img


def _lattice4_rand(W, H):
    img = np.full((H, W), 128, np.uint8)
    d = img[2::4, 1::4]
    img[2::4, 1::4] = _rng("lattice4", W, H).integers(0, 256, d.shape)
    return img


def _lattice2_signed(W, H):
    """sites every second pixel; half of them hold a dot brighter or darker than the grey around it by a random amount (with
    every site taken, 1083x100 has more candidates than the keep-all budget), so a pixel's ring crosses other dots of either sign"""
    img = np.full((H, W), 128, np.int32)
    d = img[0::2, 1::2]
    r = _rng("lattice2", W, H)
    img[0::2, 1::2] = 128 + r.choice([-1, 1], d.shape) * r.integers(1, 128, d.shape) * r.integers(0, 2, d.shape)
    return img.astype(np.uint8)


def _ramp(W, H):
    y, x = np.mgrid[0:H, 0:W]
    return ((x * 7 + y * 13) % 256).astype(np.uint8)


def _low_contrast(W, H):
    """128 +- 14: neighbouring differences of 0 .. 28 lie below minThFAST = 7, between the two thresholds and above iniThFAST = 20"""
    return (128 + _rng("low", W, H).integers(-14, 15, (H, W))).astype(np.uint8)


def _flat(W, H):
    return np.full((H, W), 90, np.uint8)


# Order matters: the first two form the small batch (1024-thread k_compact, host-mapped results); `flat` sits between two dense
# images of the full batch, where a candidate, a count or a pixel leaking from a neighbour in the batch would show.
CONTENTS = [("noise", _noise), ("binary", _binary), ("checker1", _checker(1)), ("lattice4_rand", _lattice4_rand), ("flat", _flat),
            ("lattice2_signed", _lattice2_signed), ("lattice4_const", _lattice4_const), ("checker3", _checker(3)), ("ramp", _ramp),
            ("low_contrast", _low_contrast)]
CONTENT_NAMES = [n for n, _ in CONTENTS]
KEEP_ALL_CONTENTS = ("noise", "binary", "lattice4_rand", "lattice4_const", "lattice2_signed")
DENSE_CONTENTS = ("noise", "binary", "lattice4_rand", "lattice2_signed")


def images(case):
    return [gen(case.W, case.H) for _, gen in CONTENTS]


Case = namedtuple("Case", "name W H nlevels scale ini_th min_th")


def _case(W, H, nlevels=1, scale=1.2, ini_th=20, min_th=7):
    name = "%dx%d_l%d" % (W, H, nlevels)
    if scale != 1.2:
        name += "_s%g" % scale
    if (ini_th, min_th) != (20, 7):
        name += "_t%d_%d" % (ini_th, min_th)
    return Case(name, W, H, nlevels, scale, ini_th, min_th)


def tags(case, geo=None):
    """what the case's launches reach, as a set of CHECKLIST names"""
    g = geo or geometry(case.W, case.H, case.nlevels, case.scale)
    t = {"tp%d" % g["job"]["tp"]}
    for L in g["levels"]:
        t.add("roi_gt64" if L["max_roi_rows"] > 64 else "roi_le64")
        for axis, last in (("col", L["last_col"]), ("row", L["last_row"])):
            _, _, ev, state = last
            if state == "on" and 1 <= ev <= 3:
                t.add("%s_tail_%d" % (axis, ev))
            elif state != "on":
                t.add("%s_%s" % (axis, state))
        if any(s == "beyond" for _, _, _, s in L["xs"] + L["ys"]):
            t.add("cell_beyond")
        if len(L["phases"]) == 4:
            t.add("phases4")
        if L["nCols"] * L["nRows"] == 1:
            t.add("single_cell")
        if L["nIni"] in (1, 16):
            t.add("nIni%d" % L["nIni"])
        t.update(n for n, hit in (("blur_w_mod16", L["w"] % 16), ("blur_w_mod128", L["w"] % 128), ("blur_h_mod8", L["h"] % 8),
                                  ("blur_w_lt128", L["w"] < 128)) if hit)
        R = L.get("resize")
        if R:
            t.add("resize_le4" if R["loads"] <= 4 else ("resize_5to8" if R["loads"] <= 8 else "resize_gt8"))
            if 257 <= L["w"] <= 260:
                t.add("last_block_w%d" % R["last_block_w"])
            t.add("w_mod4_%d" % R["w_mod4"])
            if L["w"] < 256:
                t.add("level_lt256")
            if R["last_block_h"] == 1:
                t.add("last_block_h1")
            if R["h_mod8"] == 1:
                t.add("h_mod8_1")
    th = (case.ini_th, case.min_th)
    t.add("th_default" if th == (20, 7) else "th_0" if th == (0, 0) else "th_254" if th == (254, 254) else
          "th_255" if th == (255, 255) else "th_equal" if th[0] == th[1] else "th_min_above_ini" if th[1] > th[0] else "th_other")
    return t


# Sizes come from a scan of geometry() over small images; every case is the cheapest found for the tags noted beside it (the
# CPU test asserts them and fails when a case stops reaching one).  No case exceeds MAX_PIXELS.
_T = (150, 118, 2)   # the threshold cases' image: 2 x 3 + 1 x 2 cells, pitch 64, a 66-row ROI; level 1 = 125 wide (< 128, < 256)
CASES = [
    _case(99, 97),                      # one 67 x 65 cell: tile pitch 80, ROI taller than 64 rows, nIni 1, level narrower than 128
    _case(308, 116, 2),                 # level 1 = 257 x 97: last column block 1 px, last row block 1 row, h mod 8 = 1; pitch 64
    _case(1083, 100),                   # last cell column 7 px: one evaluated column
    _case(1048, 100),                   # ... two
    _case(1013, 100),                   # ... three
    _case(1118, 100),                   # last cell column skipped (iniX >= maxBorderX - 6); nIni = 16
    _case(560, 1083),                   # last cell row 7 px: one evaluated row
    _case(560, 1048),                   # ... two
    _case(560, 1013),                   # ... three
    _case(600, 1118),                   # last cell row 6 px: not skipped by iniY >= maxBorderY - 3, nothing to evaluate
    _case(1363, 120),                   # last cell column starts beyond maxBorderX
    _case(516, 140, 2, 2.0),            # level 1 = 258 wide: k_resize<8> with 8 loads per thread, last column block 2 px
    _case(388, 150, 2, 1.5),            # level 1 = 259 wide: k_resize<8> with 5 loads, last column block 3 px
    _case(436, 163, 2, 2.4),            # level 1 = 182 x 68 from a 448 x 77 window: k_resize<0> (9 loads per thread)
    _case(312, 116, 2),                 # level 1 = 260 x 97: last column block 4 px; four cell phases on level 0
    _case(*_T, ini_th=10, min_th=10),   # equal thresholds
    _case(*_T, ini_th=7, min_th=20),    # min above ini
    _case(*_T, ini_th=0, min_th=0),
    _case(*_T, ini_th=254, min_th=254),  # binary content: every corner scores exactly 254
    _case(*_T, ini_th=255, min_th=255),  # no candidates at all
]
CASE_BY_NAME = {c.name: c for c in CASES}

# what the cases together must reach (the issue's checklist); `row_skipped` is not in it: see UNREACHABLE
CHECKLIST = ["tp48", "tp64", "tp80", "roi_gt64", "roi_le64",
             "col_tail_1", "col_tail_2", "col_tail_3", "row_tail_1", "row_tail_2", "row_tail_3",
             "col_skipped", "row_short", "cell_beyond", "phases4", "single_cell", "nIni1", "nIni16",
             "resize_le4", "resize_5to8", "resize_gt8",
             "last_block_w1", "last_block_w2", "last_block_w3", "last_block_w4", "w_mod4_0", "w_mod4_1", "w_mod4_2", "w_mod4_3",
             "level_lt256", "last_block_h1", "h_mod8_1",
             "blur_w_mod16", "blur_w_mod128", "blur_h_mod8", "blur_w_lt128",
             "th_default", "th_equal", "th_min_above_ini", "th_0", "th_254", "th_255"]
# the tag that only this case carries: removing the case fails CHECKLIST on it
OWN_TAG = {"99x97_l1": "tp80", "308x116_l2": "last_block_w1", "1083x100_l1": "col_tail_1", "1048x100_l1": "col_tail_2",
           "1013x100_l1": "col_tail_3", "1118x100_l1": "col_skipped", "560x1083_l1": "row_tail_1", "560x1048_l1": "row_tail_2",
           "560x1013_l1": "row_tail_3", "600x1118_l1": "row_short", "1363x120_l1": "cell_beyond", "516x140_l2_s2": "last_block_w2",
           "388x150_l2_s1.5": "last_block_w3", "436x163_l2_s2.4": "resize_gt8", "312x116_l2": "last_block_w4",
           "150x118_l2_t10_10": "th_equal", "150x118_l2_t7_20": "th_min_above_ini", "150x118_l2_t0_0": "th_0",
           "150x118_l2_t254_254": "th_254", "150x118_l2_t255_255": "th_255"}
UNREACHABLE = {
    "row_skipped": "a last cell row skipped by `iniY >= maxBorderY - 3` needs a level of h >= 1223 (hCell = 36 with 34 rows), and "
                   "nIni >= 1 then needs w >= 628: 0.77 megapixels.  600x1118 reaches the neighbouring state instead (a 6-row ROI: "
                   "the reference calls FAST, which has no row to evaluate); k_fast_cells reads `on = 0` from the cell record in both",
}


def keep_all(case):
    return case.W * case.H <= KEEP_ALL_PIXELS


def budgets(case):
    return [KEEP_ALL, 300] if keep_all(case) else [2000]


# --------------------------------------------------------------------------------------------
# 3. the oracle's expectation and the comparisons
# --------------------------------------------------------------------------------------------
def oracle_extractor(case, nfeatures, orientation=0):
    return O.OracleExtractor(nfeatures, case.scale, case.nlevels, case.ini_th, case.min_th, orientation)


def oracle_stages(ex, img):
    """one image through the oracle -> everything the GPU job is compared with (copies: the extractor is reused)"""
    mono, kps, desc = ex(img)
    assert mono >= 0, "the oracle refuses this image (%d)" % mono
    n = ex.nlevels
    level = [ex.level(l) for l in range(n)]
    # the extractor blurs a level only when it kept a keypoint there: GaussianBlur of the level's clone (REFLECT_101 at its edges)
    blurred = [O.gaussian_blur(p) for p in level]
    for l in range(n):
        b = ex.blurred(l)
        assert b is None and len(ex.level_keypoints(l)) == 0 or np.array_equal(b, blurred[l]), "oracle: blurred level %d" % l
    return dict(mono=mono, kps=kps, desc=desc, level=level, blurred=blurred,
                cand=[tuple(a.astype(np.int32) for a in ex.candidates(l)) for l in range(n)],
                level_kps=[ex.level_keypoints(l) for l in range(n)])


def diff_plane(got, ref):
    """None, or a description of the first differing pixel (raster order) of two planes"""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape:
        return "shape %s, expected %s" % (got.shape, ref.shape)
    bad = np.argwhere(got != ref)
    if len(bad) == 0:
        return None
    y, x = (int(v) for v in bad[0])
    return "%d pixels differ, the first at x=%d y=%d: got %d, expected %d (rows %d..%d, columns %d..%d)" % (
        len(bad), x, y, got[y, x], ref[y, x], bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max())


def diff_candidates(got, ref):
    """None, or a description of the first differing (x, y, response) of two candidate lists in vToDistributeKeys order"""
    g = np.stack([np.asarray(a, np.int64) for a in got], axis=1)
    r = np.stack([np.asarray(a, np.int64) for a in ref], axis=1)
    n = min(len(g), len(r))
    bad = np.nonzero(np.any(g[:n] != r[:n], axis=1))[0]
    if len(bad) == 0 and len(g) == len(r):
        return None
    i = int(bad[0]) if len(bad) else n
    fmt = lambda a: "(x=%d, y=%d, response=%d)" % tuple(a[i]) if i < len(a) else "nothing"
    return "%d candidates, expected %d; the first difference at index %d: got %s, expected %s" % (len(g), len(r), i, fmt(g), fmt(r))


def diff_features(got, ref):
    """None, or a description of the first difference of (monoIndex, keypoints, descriptors)"""
    (m1, k1, d1), (m2, k2, d2) = got, ref
    if len(k1) != len(k2) or m1 != m2:
        return "%d keypoints (monoIndex %d), expected %d (monoIndex %d)" % (len(k1), m1, len(k2), m2)
    for f in k2.dtype.names:
        bad = np.nonzero(k1[f] != k2[f])[0]
        if len(bad):
            i = int(bad[0])
            return "keypoint %d (level %d, x=%r y=%r): field %s is %r, expected %r" % (
                i, k2["octave"][i], float(k2["x"][i]), float(k2["y"][i]), f, k1[f][i].item(), k2[f][i].item())
    bad = np.nonzero(np.any(d1 != d2, axis=1))[0]
    if len(bad):
        i = int(bad[0])
        byte = int(np.nonzero(d1[i] != d2[i])[0][0])
        return "descriptor of keypoint %d (level %d, x=%r y=%r) differs in %d bytes, the first byte %d: got 0x%02x, expected 0x%02x; %d rows differ" % (
            i, k2["octave"][i], float(k2["x"][i]), float(k2["y"][i]), int((d1[i] != d2[i]).sum()), byte, d1[i][byte], d2[i][byte], len(bad))
    return None


def diff_image(rig, m, exp, with_features=True):
    """every stage of image m of the rig's last job against oracle_stages()' expectation -> list of messages (empty: equal)"""
    out = []
    for l in range(len(exp["level"])):
        for what, got, ref in (("pyramid", rig.level(m, l), exp["level"][l]), ("blurred", rig.level(m, l, blurred=True), exp["blurred"][l])):
            d = diff_plane(got, ref)
            if d:
                out.append("%s level %d (%dx%d): %s" % (what, l, ref.shape[1], ref.shape[0], d))
        d = diff_candidates(rig.candidates(m, l), exp["cand"][l])
        if d:
            out.append("FAST candidates level %d: %s" % (l, d))
    if with_features:
        d = diff_features(rig.features(m), (exp["mono"], exp["kps"], exp["desc"]))
        if d:
            out.append("features: %s" % d)
    return out
