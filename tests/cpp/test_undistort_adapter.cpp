// include/mcorb_adapter.hpp's UndistortKeyPoints path, driven as MC-SLAM would: setDistortion once per camera at init, then
// setData + extractFeaturesParallel.  Writes image_kps and image_kps_undist of every camera (raw mcorb_keypoint records) to
// OUTDIR/kps_<cam>.bin and OUTDIR/undist_<cam>.bin for tests/test_gpu_undistort.py to compare with its numpy restatement.
//   test_undistort_adapter C W H N FRAME OUTDIR COEFFS
// COEFFS: a file of C x (9 float64 K, int32 ncoeffs, 12 float64 coefficients)
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "mcorb_adapter.hpp"

static bool dump(const std::string &path, const std::vector<mcorb_keypoint> &k)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    if (!k.empty()) fwrite(k.data(), sizeof(mcorb_keypoint), k.size(), f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 8) { fprintf(stderr, "usage: %s C W H N FRAME OUTDIR COEFFS\n", argv[0]); return 2; }
    const int C = atoi(argv[1]), W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), frame = atoi(argv[5]);
    const std::string out = argv[6];
    try {
        mcorb_params p;
        mcorb_default_params(&p);
        p.nfeatures = N;
        mcorb::MultiCameraFrontEnd fe(C, W, H, p);
        FILE *cf = fopen(argv[7], "rb");
        if (!cf) return 2;
        for (int c = 0; c < C; c++) {
            double K[9], d[12];
            int32_t n = 0;
            if (fread(K, 8, 9, cf) != 9 || fread(&n, 4, 1, cf) != 1 || fread(d, 8, 12, cf) != 12) return 2;
            fe.setDistortion(c, K, n ? d : nullptr, n);
        }
        fclose(cf);
        std::vector<std::vector<uint8_t>> imgs(C, std::vector<uint8_t>((size_t)W * H));
        std::vector<const uint8_t *> ptrs;
        for (int c = 0; c < C; c++) {
            mcorb_synth_rig_frame(frame, C, c, W, H, imgs[c].data(), W);
            ptrs.push_back(imgs[c].data());
        }
        fe.setData(ptrs, W);
        fe.extractFeaturesParallel();
        if ((int)fe.image_kps_undist.size() != C) { fprintf(stderr, "image_kps_undist not filled\n"); return 1; }
        for (int c = 0; c < C; c++) {
            if (!dump(out + "/kps_" + std::to_string(c) + ".bin", fe.image_kps[c]) ||
                !dump(out + "/undist_" + std::to_string(c) + ".bin", fe.image_kps_undist[c]))
                return 2;
            printf("cam %d: %zu keypoints\n", c, fe.image_kps[c].size());
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
