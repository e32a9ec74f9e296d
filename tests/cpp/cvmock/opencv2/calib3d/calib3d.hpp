// Declarations only (no behaviour): lets tools/crosscheck/crosscheck_undistort.cpp be checked for well-formedness where no OpenCV
// exists.  Nothing links against this.
#pragma once
#include <opencv2/core/core.hpp>

namespace cv {
void undistort(const Mat &src, Mat &dst, const Mat &cameraMatrix, const Mat &distCoeffs);
}
