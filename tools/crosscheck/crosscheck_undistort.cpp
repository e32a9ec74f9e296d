// crosscheck_undistort.cpp -- the sixth unpinned OpenCV primitive: cv::undistort on an 8-bit one-channel image (the RECTIFY branch of
// MultiCameraFrame::setData, MultiCameraFrame.cpp:123-136) against mcorb_undistort_image.h, the restatement k_remap_u8 and the
// engine's host-built maps come from.  Run it with crosscheck_opencv.cpp on the first machine that has OpenCV 4.x; like that file
// IT PINS NOTHING UNTIL SOMEONE RUNS IT.  No GPU and no MC-SLAM checkout needed.
//
// On mcorb_synth_rig_frame frames 0..1 at 752x480, 1280x720 and 1920x1080 (stripe heights 5, 3 and 2), for a 4-, 5-, 8- and
// 12-coefficient model and all-zero coefficients, the first differing pixel is printed.  Where a real build could differ from
// the restatement: (1) initUndistortRectifyMap's AVX2 row loop, which computes the row positions _x, _y, _w by multiplication
// instead of the scalar loop's running sum; (2) the 3x3 inverse (Ar * I).inv(DECOMP_LU), restated as cv::invert's closed form
// for n == 3; (3) remap's weight table, whose (0, 0) entry saturates at 32767 in a short where the restatement holds 32768 -- the
// same pixel for every 8-bit value, unless the table's rounding correction moves it.
//
// Build and run: tools/crosscheck/README.md.  Exit status 0 iff nothing differs.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include <opencv2/calib3d/calib3d.hpp>
#include <opencv2/core/core.hpp>

#include "mcorb.h"   // mcorb_synth_rig_frame
#include "mcorb_undistort_image.h"

int main()
{
    static const double models[5][12] = {
        {-0.2873, 0.0912, 0.00031, -0.00047},
        {0.3841, 0.1422, -0.00112, 0.00083, 0.0213},
        {0.5213, -0.1274, 0.00041, -0.00037, 0.0089, 0.8723, -0.0612, 0.0301},
        {-0.2791, 0.0833, 0.00027, -0.00061, -0.0175, 0.0213, -0.0034, 0.0011, 0.0017, -0.0008, -0.0012, 0.0004},
        {0, 0, 0, 0},
    };
    static const int counts[5] = {4, 5, 8, 12, 4}, sizes[3][2] = {{752, 480}, {1280, 720}, {1920, 1080}};
    int bad = 0;
    for (auto &sz : sizes)
        for (int frame = 0; frame < 2; frame++)
            for (int m = 0; m < 5; m++) {
                const int W = sz[0], H = sz[1], n = counts[m];
                cv::Mat img(H, W, CV_8UC1), K(3, 3, CV_64F), D(1, n, CV_64F), out;
                mcorb_synth_rig_frame((uint32_t)frame, 1, 0, W, H, img.data, (int)img.step);
                const double k[9] = {0.9 * W, 0, W / 2 + 3.3, 0, 0.9018 * W, H / 2 - 2.1, 0, 0, 1};
                for (int i = 0; i < 9; i++) K.at<double>(i / 3, i % 3) = k[i];
                for (int i = 0; i < n; i++) D.at<double>(0, i) = models[m][i];
                cv::undistort(img, out, K, D);
                mcorb::UndistImageCam c;
                std::vector<int16_t> m1((size_t)W * H * 2);
                std::vector<uint16_t> m2((size_t)W * H);
                std::vector<uint8_t> mine((size_t)W * H);
                if (mcorb::undist_image_prepare(k, models[m], n, c) != 0) return 2;
                mcorb::undist_image_map(c, W, H, m1.data(), m2.data());
                mcorb::remap_u8(img.data, (int)img.step, W, H, m1.data(), m2.data(), mine.data(), W);
                long first = -1, ndiff = 0;
                for (int y = 0; y < H; y++)
                    for (int x = 0; x < W; x++)
                        if (out.at<uint8_t>(y, x) != mine[(size_t)y * W + x]) { if (first < 0) first = (long)y * W + x; ndiff++; }
                if (first < 0) printf("  ok    cv::undistort %2d coefficients (model %d)   %4dx%-4d frame %d  (%d pixels)\n", n, m, W, H, frame, W * H);
                else {
                    bad++;
                    printf("  DIFF  cv::undistort %2d coefficients (model %d)   %4dx%-4d frame %d  %ld pixels differ, first at (%ld, %ld): OpenCV %d, restatement %d\n",
                           n, m, W, H, frame, ndiff, first % W, first / W, (int)out.at<uint8_t>((int)(first / W), (int)(first % W)), (int)mine[(size_t)first]);
                }
            }
    printf(bad ? "crosscheck_undistort: %d comparisons DIFFER\n" : "crosscheck_undistort: all equal (%d)\n", bad);
    return bad ? 1 : 0;
}
