// mcorb_undistort_image.h on the host, without the library: the maps of one camera and the remap of one image under them, for
// tests/test_undistort_image_cpu.py, which compares both bit for bit with tests/undistort_image_ref.py.  Build with
// g++ -O2 -ffp-contract=off (the library's contraction rule); also built with -fsanitize=address,undefined.
//   test_undistort_image IN OUT     IN:  K (9 float64, row-major) | ncoeffs (int32) | 12 float64 coefficients | w, h (int32) | w*h bytes
//                                   OUT: status of undist_image_prepare (int32) | map1 (w*h*2 int16) | map2 (w*h uint16) | w*h bytes
//   test_undistort_image            the header's own invariants; prints "bad=N"
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mcorb_undistort_image.h"

static int self_check()
{
    int bad = 0;
    // all 1024 fractional positions: non-negative weights that sum to 32768; (0, 0) weighs its pixel fully
    for (unsigned m2 = 0; m2 < 1024; m2++) {
        int w[4];
        mcorb::remap_weights(m2, w);
        bad += w[0] + w[1] + w[2] + w[3] != 32768 || w[0] < 0 || w[1] < 0 || w[2] < 0 || w[3] < 0;
    }
    int w0[4];
    mcorb::remap_weights(0, w0);
    bad += w0[0] != 32768;
    // zero distortion: the identity map, and the remap under it is the image (odd sizes: every stripe height and a short last one)
    const int sizes[][2] = {{160, 120}, {37, 29}, {4097, 3}, {1, 5}, {752, 11}};
    for (auto &s : sizes) {
        const int w = s[0], h = s[1];
        const double K[9] = {431.7, 0, 0.5 * w - 0.3, 0, 429.1, 0.5 * h + 0.2, 0, 0, 1}, d[4] = {0, 0, 0, 0};
        mcorb::UndistImageCam c;
        bad += mcorb::undist_image_prepare(K, d, 4, c) != 0;
        std::vector<int16_t> m1((size_t)w * h * 2);
        std::vector<uint16_t> m2((size_t)w * h);
        mcorb::undist_image_map(c, w, h, m1.data(), m2.data());
        std::vector<uint8_t> img((size_t)w * h), out((size_t)w * h);
        for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)(i * 2654435761u >> 24);
        for (int y = 0; y < h; y++)
            for (int x = 0; x < w; x++) {
                const size_t i = (size_t)y * w + x;
                bad += m1[2 * i] != x || m1[2 * i + 1] != y || m2[i] != 0;
            }
        mcorb::remap_u8(img.data(), w, w, h, m1.data(), m2.data(), out.data(), w);
        bad += img != out;
    }
    // a map that points far outside, and at every border: no tap is read outside the source (the sanitizers watch), zeros come back
    {
        const int w = 5, h = 4;
        std::vector<uint8_t> img((size_t)w * h, 200), out((size_t)w * h, 7);
        std::vector<int16_t> m1((size_t)w * h * 2);
        std::vector<uint16_t> m2((size_t)w * h, 1023);
        const int16_t xs[] = {-32768, -2, -1, 0, 3, 4, 5, 32767}, ys[] = {-32768, -1, 0, 2, 3, 4, 32767};
        for (int16_t sy : ys)
            for (int16_t sx : xs) {
                for (size_t i = 0; i < (size_t)w * h; i++) { m1[2 * i] = sx; m1[2 * i + 1] = sy; }
                mcorb::remap_u8(img.data(), w, w, h, m1.data(), m2.data(), out.data(), w);
                const bool all_in = sx >= 0 && sx + 1 < w && sy >= 0 && sy + 1 < h;
                const bool all_out = sx + 1 < 0 || sx >= w || sy + 1 < 0 || sy >= h;
                for (uint8_t v : out) bad += (all_in && v != 200) || (all_out && v != 0) || v > 200;
            }
    }
    // what an int cannot hold
    bad += mcorb::undist_image_round(1e300) != INT32_MIN || mcorb::undist_image_round(-1e300) != INT32_MIN;
    bad += mcorb::undist_image_round(0.5) != 0 || mcorb::undist_image_round(1.5) != 2 || mcorb::undist_image_round(-2.5) != -2;
    // counts
    {
        const double K[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, d[14] = {};
        mcorb::UndistImageCam c;
        for (int n = 0; n <= 14; n++) bad += (mcorb::undist_image_prepare(K, d, n, c) == 0) != (n == 4 || n == 5 || n == 8 || n == 12);
    }
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) { fprintf(stderr, "usage: %s [IN OUT]\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    double K[9], dist[12];
    int32_t n = 0, w = 0, h = 0;
    if (fread(K, 8, 9, f) != 9 || fread(&n, 4, 1, f) != 1 || fread(dist, 8, 12, f) != 12 || fread(&w, 4, 1, f) != 1 ||
        fread(&h, 4, 1, f) != 1 || w < 1 || h < 1)
        return 2;
    std::vector<uint8_t> img((size_t)w * h), out((size_t)w * h);
    if (fread(img.data(), 1, img.size(), f) != img.size()) return 2;
    fclose(f);
    std::vector<int16_t> m1((size_t)w * h * 2);
    std::vector<uint16_t> m2((size_t)w * h);
    mcorb::UndistImageCam c;
    const int32_t st = mcorb::undist_image_prepare(K, dist, n, c);
    if (st == 0) {
        mcorb::undist_image_map(c, w, h, m1.data(), m2.data());
        mcorb::remap_u8(img.data(), w, w, h, m1.data(), m2.data(), out.data(), w);
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(&st, 4, 1, g);
    fwrite(m1.data(), 2, m1.size(), g);
    fwrite(m2.data(), 2, m2.size(), g);
    fwrite(out.data(), 1, out.size(), g);
    fclose(g);
    return 0;
}
