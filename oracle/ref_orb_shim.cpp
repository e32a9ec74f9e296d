/*
 * ref_orb_shim.cpp -- C interface to the reference's own MCSlam/src/ORBextractor.cpp, compiled UNCHANGED.
 *
 * TEST INFRASTRUCTURE.  The reference is reached by include path only (oracle/Makefile, target `ref`, passes
 * -I<reference>/MCSlam/include -I<reference>/MCSlam/src); no line of it is copied here.  This file holds includes and calls.
 * The cv:: names it needs come from oracle/refcv (this repository's stand-in): the reference's own logic is what becomes
 * pinned, OpenCV's primitives stay the oracle's restatements and stay unpinned -- see oracle/refcv/opencv2/core/core.hpp.
 *
 * The .cpp itself is included so that its file-static functions (IC_Angle, computeOrbDescriptor) can be called, and
 * `protected` is opened for the reference's header so that ComputePyramid, ComputeKeyPointsOctTree, DistributeOctTree and the
 * tables can be reached.
 */
#include <stdint.h>
#include <string.h>

#include <iostream>
#include <list>
#include <vector>

#include <opencv2/opencv.hpp>

#define protected public
#include <MCSlam/ORBextractor.h>
#undef protected
#include <ORBextractor.cpp>

namespace {
struct RefHandle {
    ORBextractor ex;
    std::vector<std::vector<cv::KeyPoint> > levelKeys;   // ComputeKeyPointsOctTree's output
    std::vector<cv::Mat> blurred;                        // clone + GaussianBlur of a pyramid level, as operator() makes it
    RefHandle(int nf, float sf, int nl, int ini, int mn) : ex(nf, sf, nl, ini, mn) {}
};
cv::Mat view(const void *p, int w, int h, int stride) { return cv::Mat(h, w, CV_8UC1, const_cast<void *>(p), (size_t)stride); }
void put(const cv::KeyPoint &k, orc_keypoint *o)
{
    o->x = k.pt.x; o->y = k.pt.y; o->size = k.size; o->angle = k.angle; o->response = k.response;
    o->octave = k.octave; o->class_id = k.class_id;
}
}   // namespace

extern "C" {

void *ref_create(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th)
{
    return new RefHandle(nfeatures, scale_factor, nlevels, ini_th, min_th);
}
void ref_destroy(void *h) { delete (RefHandle *)h; }

/* the getters (ORBextractor.h) and the protected tables; pattern512 receives x,y of the 512 points */
void ref_tables(void *h, float *scale, float *inv_scale, float *sigma2, float *inv_sigma2, int *quota, int *umax16, int *pattern512)
{
    ORBextractor &e = ((RefHandle *)h)->ex;
    std::vector<float> a = e.GetScaleFactors(), b = e.GetInverseScaleFactors(), c = e.GetScaleSigmaSquares(),
                       d = e.GetInverseScaleSigmaSquares();
    for (int i = 0; i < e.GetLevels(); i++) {
        scale[i] = a[i]; inv_scale[i] = b[i]; sigma2[i] = c[i]; inv_sigma2[i] = d[i];
        quota[i] = e.mnFeaturesPerLevel[i];
    }
    for (size_t i = 0; i < e.umax.size() && i < 16; i++) umax16[i] = e.umax[i];
    for (size_t i = 0; i < e.pattern.size() && i < 512; i++) { pattern512[2 * i] = e.pattern[i].x; pattern512[2 * i + 1] = e.pattern[i].y; }
}
int ref_table_sizes(void *h, int *numax, int *npattern)
{
    ORBextractor &e = ((RefHandle *)h)->ex;
    *numax = (int)e.umax.size(); *npattern = (int)e.pattern.size();
    return e.GetLevels();
}

/* ORBextractor::operator(); returns monoIndex, n_out the keypoint count, -3 when cap is too small */
int ref_extract(void *h, const uint8_t *gray, int w, int hh, int stride, int lap0, int lap1, orc_keypoint *kps, uint8_t *desc,
                int cap, int *n_out)
{
    RefHandle *H = (RefHandle *)h;
    cv::Mat img = view(gray, w, hh, stride), descriptors;
    std::vector<cv::KeyPoint> keys;
    std::vector<int> lap(2);
    lap[0] = lap0; lap[1] = lap1;
    H->blurred.clear();
    const int mono = H->ex(img, cv::Mat(), keys, descriptors, lap);
    *n_out = (int)keys.size();
    if ((int)keys.size() > cap) return -3;
    for (size_t i = 0; i < keys.size(); i++) {
        put(keys[i], kps + i);
        memcpy(desc + i * 32, descriptors.ptr((int)i), 32);
    }
    return mono;
}

/* mvImagePyramid[level] with the border ComputePyramid put around it: the view's parent matrix */
const uint8_t *ref_level_bordered(void *h, int level, int *w, int *hh, int *stride)
{
    const cv::Mat &m = ((RefHandle *)h)->ex.mvImagePyramid[level];
    cv::Size whole;
    cv::Point ofs;
    m.locateROI(whole, ofs);
    *w = whole.width; *hh = whole.height; *stride = (int)m.step;
    return m.data - (size_t)ofs.y * m.step - ofs.x;
}

/* ComputePyramid + ComputeKeyPointsOctTree; the per-level lists are read with ref_level_keypoints */
void ref_compute_keypoints(void *h, const uint8_t *gray, int w, int hh, int stride)
{
    RefHandle *H = (RefHandle *)h;
    H->blurred.clear();
    H->ex.ComputePyramid(view(gray, w, hh, stride));
    H->ex.ComputeKeyPointsOctTree(H->levelKeys);
}
int ref_level_keypoints(void *h, int level, orc_keypoint *kps, int cap)
{
    const std::vector<cv::KeyPoint> &k = ((RefHandle *)h)->levelKeys[level];
    for (int i = 0; i < (int)k.size() && i < cap; i++) put(k[i], kps + i);
    return (int)k.size();
}

/* ORBextractor::DistributeOctTree on caller-given candidates; class_id carries the input index out */
int ref_distribute(void *h, const float *x, const float *y, const float *resp, int n, int minX, int maxX, int minY, int maxY, int N,
                   int *out_idx, int cap)
{
    std::vector<cv::KeyPoint> in(n);
    for (int i = 0; i < n; i++) in[i] = cv::KeyPoint(x[i], y[i], 7.f, -1, resp[i], 0, i);
    const int level = 0;
    std::vector<cv::KeyPoint> out = ((RefHandle *)h)->ex.DistributeOctTree(in, minX, maxX, minY, maxY, N, level);
    for (int i = 0; i < (int)out.size() && i < cap; i++) out_idx[i] = out[i].class_id;
    return (int)out.size();
}

/* IC_Angle on mvImagePyramid[level] of the last ref_extract / ref_compute_keypoints call, for n points */
void ref_ic_angle(void *h, int level, const float *x, const float *y, int n, float *angle)
{
    RefHandle *H = (RefHandle *)h;
    for (int i = 0; i < n; i++) angle[i] = IC_Angle(H->ex.mvImagePyramid[level], cv::Point2f(x[i], y[i]), H->ex.umax);
}

/* the blurred level as operator() makes it (clone, GaussianBlur 7x7 sigma 2 REFLECT_101) */
static const cv::Mat &blurred_level(RefHandle *H, int level)
{
    if (H->blurred.size() != H->ex.mvImagePyramid.size()) H->blurred.assign(H->ex.mvImagePyramid.size(), cv::Mat());
    if (H->blurred[level].empty()) {
        cv::Mat workingMat = H->ex.mvImagePyramid[level].clone();
        cv::GaussianBlur(workingMat, workingMat, cv::Size(7, 7), 2, 2, cv::BORDER_REFLECT_101);
        H->blurred[level] = workingMat;
    }
    return H->blurred[level];
}
const uint8_t *ref_level_blurred(void *h, int level, int *w, int *hh, int *stride)
{
    const cv::Mat &m = blurred_level((RefHandle *)h, level);
    *w = m.cols; *hh = m.rows; *stride = (int)m.step;
    return m.data;
}
/* computeOrbDescriptor at caller-given angles on that blurred level, n keypoints, 32 bytes each */
void ref_orb_descriptor(void *h, int level, const float *x, const float *y, const float *angle, int n, uint8_t *desc)
{
    RefHandle *H = (RefHandle *)h;
    const cv::Mat &img = blurred_level(H, level);
    for (int i = 0; i < n; i++) computeOrbDescriptor(cv::KeyPoint(x[i], y[i], 31.f, angle[i]), img, &H->ex.pattern[0], desc + (size_t)i * 32);
}
int ref_descriptor_distance(void *h, const uint8_t *a, const uint8_t *b)
{
    return ((RefHandle *)h)->ex.DescriptorDistance(view(a, 32, 1, 32), view(b, 32, 1, 32));
}

/* ORBextractor::getMatches_distRatio; A and B are rows of 32 bytes, bookK accumulates as in the reference */
int ref_get_matches_dist_ratio(void *h, const uint8_t *A, int nrowsA, const uint32_t *iA, int nA, const uint8_t *B, int nrowsB,
                               const uint32_t *iB, int nB, double max_neighbor_ratio, uint32_t *mA, uint32_t *mB, int *bookK)
{
    ORBextractor &e = ((RefHandle *)h)->ex;
    std::vector<cv::Mat> vA(nrowsA), vB(nrowsB);
    for (int i = 0; i < nrowsA; i++) vA[i] = view(A + (size_t)i * 32, 32, 1, 32);
    for (int i = 0; i < nrowsB; i++) vB[i] = view(B + (size_t)i * 32, 32, 1, 32);
    std::vector<unsigned int> ia(iA, iA + nA), ib(iB, iB + nB), ma, mb;
    e.max_neighbor_ratio = max_neighbor_ratio;
    e.getMatches_distRatio(vA, ia, vB, ib, ma, mb, *bookK);
    for (size_t k = 0; k < ma.size(); k++) { mA[k] = ma[k]; mB[k] = mb[k]; }
    return (int)ma.size();
}

}   // extern "C"
