// mcorb_undistort.h on the host: undistorts the points of one camera for tests/test_undistort_cpu.py, which compares the result
// bit for bit with tests/undistort_ref.py.  Build with g++ -O2 -ffp-contract=off (the library's contraction rule).
//   test_undistort IN OUT
// IN:  K (9 float64, row-major) | ncoeffs (int32) | 12 float64 coefficients (the first ncoeffs used) | npts (int64) | npts x (u, v) float32
// OUT: status of undist_prepare (int32) | mode (int32) | npts x (x, y) float32
#include <cstdio>
#include <cstdint>
#include <vector>

#include "mcorb_undistort.h"

int main(int argc, char **argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double K[9], dist[12];
    int32_t n = 0;
    int64_t npts = 0;
    if (fread(K, 8, 9, f) != 9 || fread(&n, 4, 1, f) != 1 || fread(dist, 8, 12, f) != 12 || fread(&npts, 8, 1, f) != 1 || npts < 0) return 2;
    std::vector<float> pts((size_t)npts * 2), out((size_t)npts * 2);
    if (npts && fread(pts.data(), 4, pts.size(), f) != pts.size()) return 2;
    fclose(f);
    mcorb::UndistCam c;
    const int32_t st = mcorb::undist_prepare(K, dist, n, c);
    const int32_t mode = st == 0 ? c.mode : -1;
    if (st == 0)
        for (int64_t i = 0; i < npts; i++) mcorb::undistort_point(c, pts[2 * i], pts[2 * i + 1], out[2 * i], out[2 * i + 1]);
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(&st, 4, 1, g);
    fwrite(&mode, 4, 1, g);
    if (npts) fwrite(out.data(), 4, out.size(), g);
    fclose(g);
    return 0;
}
