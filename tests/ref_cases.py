"""Inputs shared by the tests against the reference's ORBextractor (live binary, recorded fixtures, GPU): DistributeOctTree
candidate sets and the extractor parameter sets.  Every case here is one where the reference is defined: nIni >= 1 and every
candidate inside the region (the oracle answers -2 where it is not; those cases are never handed to the reference)."""
import numpy as np

# level-0 regions (minX, maxX, minY, maxY) = (16, W - 16, 16, H - 16) of an W x H image, ORBextractor.cpp:788-791
REGIONS = {
    "640x480 nIni=1": (16, 624, 16, 464),                # 608 / 448 -> 1
    "1280x720 nIni=2": (16, 1264, 16, 704),              # 1248 / 688 -> 2, hX = 624
    "1800x600 nIni=3 hX=589.33": (16, 1784, 16, 584),    # 1768 / 568 -> 3, hX not an integer
    "1241x376 nIni=4 hX=302.25": (16, 1225, 16, 360),    # 1209 / 344 -> 4, hX not an integer
    "641x479 odd": (16, 625, 16, 463),                   # odd width and height: the halves of DivideNode round up
}

PARAM_SETS = [(500, 1.2, 8, 20, 7), (3000, 1.2, 8, 20, 7), (1000, 1.5, 4, 20, 7), (1500, 1.1, 12, 20, 7), (1000, 1.2, 8, 10, 10),
              (800, 1.2, 1, 30, 5), (1000, 1.3, 6, 7, 20), (1000, 2.0, 3, 20, 7)]      # tests/test_gpu_param_sweep.py
ODD_SIZES = [(641, 479), (1000, 750), (1241, 376), (803, 601)]                          # tests/test_gpu_param_sweep.py
# Level-0 sizes L whose last 35-pixel cell starts g pixels before maxBorder = L - 16 (ORBextractor.cpp:799-818): 1119 -> 7..9 (the
# narrowest strip FAST can find a corner in; not skipped), 1118 -> 4..6 (skipped by `iniX >= maxBorderX - 6`, run with a clamped
# maxY in y), 1223 -> 1..3 (skipped by both tests), 1328 -> 0 or less (the start lies beyond the border)
SKIP_EDGE_SIZES = [(1119, 1118), (1118, 1223), (1328, 1119), (1223, 1328), (1118, 1118)]


def _uniform(rng, n, w, h):
    return rng.integers(3, w - 3, n), rng.integers(3, h - 3, n), rng.integers(7, 256, n)


def _clustered(rng, n, w, h):
    cx, cy = rng.integers(40, w - 40), rng.integers(40, h - 40)
    x = np.clip(np.rint(rng.normal(cx, 9, n)), 3, w - 4)
    y = np.clip(np.rint(rng.normal(cy, 9, n)), 3, h - 4)
    m = n // 10      # a thin background so that the other root nodes are not empty
    x[:m], y[:m] = rng.integers(3, w - 3, m), rng.integers(3, h - 3, m)
    return x, y, rng.integers(7, 256, n)


def _one_pixel(rng, n, w, h):
    """most keys on very few pixels with equal responses: the tree divides down to 1-pixel nodes that cannot separate them"""
    x, y, r = _uniform(rng, n, w, h)
    k = n * 2 // 3
    x[:k], y[:k], r[:k] = w // 3, h // 2 + 1, 40
    x[k:k + n // 10], y[k:k + n // 10], r[k:k + n // 10] = w // 3 + 1, h // 2 + 1, 40
    p = rng.permutation(n)
    return x[p], y[p], r[p]


def _lattice(rng, nx, ny, w, h, per_site=2):
    """keys on a regular lattice, per_site keys per site with equal responses: whole columns of nodes share (count, UL.x),
    so where std::sort puts equivalent elements decides which nodes are divided before the N-break"""
    xs = (np.arange(nx) * ((w - 8) // nx) + 4)
    ys = (np.arange(ny) * ((h - 8) // ny) + 4)
    X, Y = np.meshgrid(xs, ys)
    x = np.repeat(X.ravel(), per_site) + np.tile(np.arange(per_site), nx * ny)
    y = np.repeat(Y.ravel(), per_site)
    r = np.full(len(x), 50)
    p = rng.permutation(len(x))
    return x[p], y[p], r[p]


def octree_cases(small=False):
    """yields (name, x, y, response, (minX, maxX, minY, maxY), N).  small=True: the handful recorded as fixtures."""
    out = []

    def add(name, gen, region, Ns):
        x, y, r = gen
        for N in Ns:
            out.append(("%s, %s, N=%d" % (name, region, N), np.asarray(x, np.float32), np.asarray(y, np.float32),
                        np.asarray(r, np.float32), REGIONS[region], int(N)))

    rng = np.random.default_rng(2024)
    if small:
        add("uniform 600", _uniform(rng, 600, 608, 448), "640x480 nIni=1", [150])
        add("clustered 500", _clustered(rng, 500, 1768, 568), "1800x600 nIni=3 hX=589.33", [120])
        add("one pixel 300", _one_pixel(rng, 300, 1248, 688), "1280x720 nIni=2", [80])
        add("lattice 12x9 x2", _lattice(rng, 12, 9, 608, 448), "640x480 nIni=1", [70])
        add("lattice 30x20 x2", _lattice(rng, 30, 20, 1209, 344), "1241x376 nIni=4 hX=302.25", [400])
        return out
    for region, (x0, x1, y0, y1) in REGIONS.items():
        w, h = x1 - x0, y1 - y0
        n = 3000
        add("uniform %d" % n, _uniform(rng, n, w, h), region, [1, 2, 3, 37, 500, 1500, 2400, n - 1, n, n + 1, 5000])
        add("clustered 2000", _clustered(rng, 2000, w, h), region, [1, 2, 50, 300, 1000, 2500])
        add("one pixel 900", _one_pixel(rng, 900, w, h), region, [1, 2, 20, 100, 250, 300, 899, 900, 901])
        add("equal responses", (lambda g: (g[0], g[1], np.full(len(g[0]), 33)))(_uniform(rng, 1500, w, h)), region, [10, 400, 1200])
        # ties in (count, UL.x): sort vectors below std::sort's 16-element insertion threshold, above it, and thousands long
        add("lattice 4x3 x2", _lattice(rng, 4, 3, w, h), region, [5, 8, 11, 12, 13])
        add("lattice 12x9 x2", _lattice(rng, 12, 9, w, h), region, [30, 60, 70, 100, 108, 109])
        add("lattice 30x20 x3", _lattice(rng, 30, 20, w, h, 3), region, [150, 400, 590, 600, 601, 1000])
        add("lattice 75x55 x2", _lattice(rng, 75, 55, w, h), region, [1100, 2000, 3000, 4000, 4125, 5000, 8000])
        # half-pixel coordinates (FAST never makes them; the function takes any float inside the region)
        g = _uniform(rng, 800, w, h)
        add("half pixels", (g[0] + 0.5, g[1] - 0.5, g[2]), region, [100, 700])
        add("no candidate", (np.zeros(0), np.zeros(0), np.zeros(0)), region, [1, 100])
        add("one candidate", (np.array([w // 2]), np.array([h // 2]), np.array([20])), region, [1, 100])
        add("one candidate in the last column", (np.array([w - 1]), np.array([h - 1]), np.array([20])), region, [1])
        add("two candidates on one pixel", (np.array([7, 7]), np.array([9, 9]), np.array([20, 20])), region, [1, 2, 3])
    return out


def table_param_sets():
    """every parameter set of tests/test_gpu_param_sweep.py, the ranges scripts/fuzz_parity.py draws from (nfeatures 50..3499,
    its scale factors, nlevels 1..9) and nlevels 1 and 16"""
    sets = list(PARAM_SETS)
    for sf in (1.1, 1.2, 1.3, 1.5, 2.0):
        for nl in list(range(1, 10)) + [12, 16]:
            for nf in (50, 51, 333, 1000, 2000, 3499, 7000, 8000):
                sets.append((nf, sf, nl, 20, 7))
    rng = np.random.default_rng(7)
    for _ in range(300):
        sets.append((int(rng.integers(50, 3500)), float(rng.choice([1.1, 1.2, 1.3, 1.5, 2.0])), int(rng.integers(1, 10)),
                     int(rng.integers(5, 40)), int(rng.integers(3, 25))))
    return sets
