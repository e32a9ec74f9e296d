// include/mcorb_adapter.hpp's RECTIFY path, driven as MC-SLAM would: setRectify once per camera at init, then setData (or
// setDataF32) + extractFeaturesParallel.  Writes, per camera, the raw plane the rig received, level 0 as the job read it, the
// keypoints and the descriptors to OUTDIR/{raw,level0,kps,desc}_<cam>.bin, and whether image_kps_undist stayed empty, for
// tests/test_gpu_undistort_image.py to compare with its numpy restatement and with a plain rig.
//   test_undistort_image_adapter C W H N FRAME OUTDIR COEFFS F32
// COEFFS: a file of C x (9 float64 K, int32 ncoeffs, 12 float64 coefficients); F32: 0 = setData, 1 = setDataF32 (1 channel)
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "mcorb_adapter.hpp"

static bool dump(const std::string &path, const void *p, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    if (bytes) fwrite(p, 1, bytes, f);
    fclose(f);
    return true;
}

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: %s C W H N FRAME OUTDIR COEFFS F32\n", argv[0]); return 2; }
    const int C = atoi(argv[1]), W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), frame = atoi(argv[5]), f32 = atoi(argv[8]);
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
            fe.setRectify(c, K, n ? d : nullptr, n);
            if (mcorb_rig_image_undistortion_active(fe.rig(), c) != (n ? 1 : 0)) { fprintf(stderr, "camera %d: active flag\n", c); return 1; }
        }
        fclose(cf);
        std::vector<std::vector<uint8_t>> imgs(C, std::vector<uint8_t>((size_t)W * H));
        std::vector<std::vector<float>> fimgs(C);
        std::vector<const uint8_t *> ptrs;
        std::vector<const float *> fptrs;
        for (int c = 0; c < C; c++) {
            mcorb_synth_rig_frame(frame, C, c, W, H, imgs[c].data(), W);
            ptrs.push_back(imgs[c].data());
            if (f32) {
                fimgs[c].resize(imgs[c].size());
                for (size_t i = 0; i < imgs[c].size(); i++) fimgs[c][i] = (float)imgs[c][i] / 255.f;
                fptrs.push_back(fimgs[c].data());
            }
        }
        if (f32) fe.setDataF32(fptrs, W * 4, 1);
        else fe.setData(ptrs, W);
        fe.extractFeaturesParallel();
        if (!fe.image_kps_undist.empty()) { fprintf(stderr, "image_kps_undist filled on a rectified rig\n"); return 1; }
        std::vector<uint8_t> plane((size_t)W * H);
        for (int c = 0; c < C; c++) {
            const std::string sc = std::to_string(c);
            if (mcorb_rig_get_raw_image(fe.rig(), 0, c, plane.data(), W) != MCORB_OK || !dump(out + "/raw_" + sc + ".bin", plane.data(), plane.size())) return 2;
            if (mcorb_rig_get_level(fe.rig(), 0, c, 0, plane.data(), W) != MCORB_OK || !dump(out + "/level0_" + sc + ".bin", plane.data(), plane.size())) return 2;
            if (!dump(out + "/kps_" + sc + ".bin", fe.image_kps[c].data(), fe.image_kps[c].size() * sizeof(mcorb_keypoint)) ||
                !dump(out + "/desc_" + sc + ".bin", fe.image_descriptors[c].data(), fe.image_descriptors[c].size()))
                return 2;
            printf("cam %d: %zu keypoints\n", c, fe.image_kps[c].size());
        }
    } catch (const std::exception &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
