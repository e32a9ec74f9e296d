// refcv -- this repository's own, WORKING stand-in for the slice of the cv:: surface that the reference's
// MCSlam/src/ORBextractor.cpp uses, so that file can be compiled unchanged without OpenCV (oracle/Makefile, target `ref`).
//
// WHAT THIS PINS AND WHAT IT DOES NOT.  With it the reference's own program text (DistributeOctTree, DivideNode, the cell
// loop, the constructor's tables, ComputePyramid's in-place border, operator()'s assembly, IC_Angle, computeOrbDescriptor,
// DescriptorDistance, getMatches_distRatio) runs as its authors wrote it: THE REFERENCE'S OWN LOGIC BECOMES PINNED.
// The arithmetic of OpenCV's primitives is NOT taken from OpenCV: cvRound/cvFloor/cvCeil, fastAtan2, FAST, resize,
// copyMakeBorder and GaussianBlur forward to the oracle's orc_* restatements (oracle/mcorb_oracle.h), so
// OPENCV'S FIVE PRIMITIVES (FAST, resize, copyMakeBorder, GaussianBlur, fastAtan2) STAY UNPINNED -- known-answer tests
// (tests/test_oracle_primitives.py) and the torch cross-check (tests/test_oracle_vs_torch.py) are all that holds them.
//
// The container types below restate OpenCV 4.x semantics; each cites the OpenCV header it restates.  Nothing here is
// OpenCV's code.  Only CV_8UC1 storage exists.  Fresh storage is filled with 0xCD, not zero (OpenCV leaves it
// uninitialised): a read of a never-written byte then disagrees with the oracle instead of passing by luck.
// tests/cpp/cvmock (declarations for a syntax check of the adapter) is a different thing and stays what it is.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <memory>
#include <vector>

#include "mcorb_oracle.h"

typedef unsigned char uchar;   // opencv2/core/hal/interface.h

#define CV_8U 0                // opencv2/core/hal/interface.h
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795   // opencv2/core/cvdef.h
#define CV_Assert(x) do { if (!(x)) { ::abort(); } } while (0)

// opencv2/core/fast_math.hpp: cvRound is round-half-to-even (cvtss2si / cvtsd2si), with float, double and int overloads;
// cvFloor / cvCeil are `int i = (int)v; return i -/+ (i >/< v);` for both float and double.
inline int cvRound(float v) { return orc_cv_round_f(v); }
inline int cvRound(double v) { return orc_cv_round_d(v); }
inline int cvRound(int v) { return v; }
inline int cvFloor(float v) { return orc_cv_floor_f(v); }
inline int cvFloor(double v) { int i = (int)v; return i - (i > v); }
inline int cvFloor(int v) { return v; }
inline int cvCeil(float v) { return orc_cv_ceil_f(v); }
inline int cvCeil(double v) { int i = (int)v; return i + (i < v); }
inline int cvCeil(int v) { return v; }

namespace cv {

// opencv2/core/base.hpp (BorderTypes), opencv2/imgproc.hpp (InterpolationFlags)
enum { BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4, BORDER_ISOLATED = 16 };
enum { INTER_LINEAR = 1 };

// opencv2/core/types.hpp: Point_<_Tp>(_Tp _x, _Tp _y) -- the arguments ARE _Tp, so a float passed to Point2i converts by
// the C++ float->int rule (truncation toward zero), not by cvRound.  Two plain members, x first: the reference casts an
// int array to `const Point*`.
template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T _x, T _y) : x(_x), y(_y) {}
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;
// types.hpp: operator*=(Point_<_Tp>&, float) multiplies each member in float and saturate_casts back (identity for float)
template <typename T> inline Point_<T> &operator*=(Point_<T> &a, float b)
{
    a.x = (T)(a.x * b);
    a.y = (T)(a.y * b);
    return a;
}
template <typename T> inline Point_<T> &operator*=(Point_<T> &a, double b)
{
    a.x = (T)(a.x * b);
    a.y = (T)(a.y * b);
    return a;
}

// types.hpp: Size_<_Tp>, Rect_<_Tp>
struct Size {
    int width, height;
    Size() : width(0), height(0) {}
    Size(int w, int h) : width(w), height(h) {}
};
struct Rect {
    int x, y, width, height;
    Rect() : x(0), y(0), width(0), height(0) {}
    Rect(int _x, int _y, int w, int h) : x(_x), y(_y), width(w), height(h) {}
};

// types.hpp: KeyPoint() : pt(0,0), size(0), angle(-1), response(0), octave(0), class_id(-1); field order pt, size, angle,
// response, octave, class_id (28 bytes, the layout of orc_keypoint)
class KeyPoint {
public:
    Point2f pt;
    float size, angle, response;
    int octave, class_id;
    KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
    KeyPoint(float x, float y, float _size, float _angle = -1, float _response = 0, int _octave = 0, int _class_id = -1)
        : pt(x, y), size(_size), angle(_angle), response(_response), octave(_octave), class_id(_class_id) {}
};

class _InputArray;
class _OutputArray;

// opencv2/core/mat.hpp / mat.inl.hpp: a header over reference-counted storage.  Copying a Mat shares the storage; rowRange,
// colRange, row and operator()(Rect) make views into it; clone() and create() make new storage.
class Mat {
public:
    int rows, cols;
    uchar *data;
    size_t step;   // bytes per row (MatStep converts to size_t)

    Mat() : rows(0), cols(0), data(0), step(0), wrows_(0), wcols_(0), oy_(0), ox_(0) {}
    Mat(int r, int c, int type) : Mat() { create(r, c, type); }
    Mat(Size sz, int type) : Mat() { create(sz.height, sz.width, type); }
    // header over caller memory (no ownership), mat.inl.hpp Mat(int, int, int, void*, size_t)
    Mat(int r, int c, int type, void *ext, size_t _step = 0)
        : rows(r), cols(c), data((uchar *)ext), step(_step ? _step : (size_t)c), wrows_(r), wcols_(c), oy_(0), ox_(0)
    {
        CV_Assert(type == CV_8UC1);
    }

    // mat.inl.hpp Mat::create(int, int, int): `if (dims <= 2 && rows == _rows && cols == _cols && type() == _type && data)
    // return;` -- a Mat (a view too) that already has the size keeps its storage.  resize() into a view and the in-place
    // copyMakeBorder(level, temp, ...) of ComputePyramid rely on exactly this.
    void create(int r, int c, int type)
    {
        CV_Assert(type == CV_8UC1);
        if (rows == r && cols == c && data) return;
        rows = r; cols = c; step = (size_t)c;
        wrows_ = r; wcols_ = c; oy_ = ox_ = 0;
        const size_t n = (size_t)r * (size_t)c;
        buf_ = std::shared_ptr<uchar>(n ? (uchar *)malloc(n) : 0, free);
        data = buf_.get();
        if (n) memset(data, 0xCD, n);
    }
    void create(Size sz, int type) { create(sz.height, sz.width, type); }
    void release() { *this = Mat(); }
    // mat.hpp: Mat::zeros returns a MatExpr; assigning it to a Mat yields a zero-filled matrix of that size
    static Mat zeros(int r, int c, int type)
    {
        Mat m(r, c, type);
        if (m.data) memset(m.data, 0, (size_t)r * c);
        return m;
    }
    Mat clone() const
    {
        Mat m;
        if (!empty()) {
            m.create(rows, cols, CV_8UC1);
            for (int r = 0; r < rows; r++) memcpy(m.data + (size_t)r * m.step, data + (size_t)r * step, (size_t)cols);
        }
        return m;
    }
    inline void copyTo(const _OutputArray &dst) const;

    int type() const { return CV_8UC1; }
    bool empty() const { return data == 0 || rows == 0 || cols == 0; }
    size_t step1() const { return step; }   // step / elemSize1(), 1 for 8-bit
    bool isSubmatrix() const { return wrows_ != rows || wcols_ != cols; }
    // mat.hpp Mat::locateROI: size of the parent matrix and the view's offset in it
    void locateROI(Size &whole, Point &ofs) const { whole = Size(wcols_, wrows_); ofs = Point(ox_, oy_); }
    // mat.hpp Mat::adjustROI: grow (positive) or shrink the view inside its parent, clamped to the parent
    Mat &adjustROI(int dtop, int dbottom, int dleft, int dright)
    {
        int r1 = std::max(oy_ - dtop, 0), r2 = std::min(oy_ + rows + dbottom, wrows_);
        int c1 = std::max(ox_ - dleft, 0), c2 = std::min(ox_ + cols + dright, wcols_);
        data += (ptrdiff_t)(r1 - oy_) * (ptrdiff_t)step + (c1 - ox_);
        rows = r2 - r1; cols = c2 - c1; oy_ = r1; ox_ = c1;
        return *this;
    }

    Mat operator()(const Rect &r) const
    {
        CV_Assert(0 <= r.x && 0 <= r.width && r.x + r.width <= cols && 0 <= r.y && 0 <= r.height && r.y + r.height <= rows);
        Mat v(*this);
        v.data = data + (size_t)r.y * step + r.x;
        v.rows = r.height; v.cols = r.width;
        v.oy_ = oy_ + r.y; v.ox_ = ox_ + r.x;
        return v;
    }
    // int parameters: a float argument (the reference passes its float iniY/maxY/iniX/maxX) truncates toward zero
    Mat rowRange(int a, int b) const { return (*this)(Rect(0, a, cols, b - a)); }
    Mat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
    Mat row(int y) const { return (*this)(Rect(0, y, cols, 1)); }

    template <typename T> T &at(int r, int c) { return *(T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    template <typename T> const T &at(int r, int c) const { return *(const T *)(data + (size_t)r * step + (size_t)c * sizeof(T)); }
    uchar *ptr(int r = 0) { return data + (size_t)r * step; }
    const uchar *ptr(int r = 0) const { return data + (size_t)r * step; }
    template <typename T> T *ptr(int r = 0) { return (T *)(data + (size_t)r * step); }
    template <typename T> const T *ptr(int r = 0) const { return (const T *)(data + (size_t)r * step); }

private:
    std::shared_ptr<uchar> buf_;
    int wrows_, wcols_, oy_, ox_;   // parent size and this view's offset in it (what datastart/dataend encode in OpenCV)
};

// mat.hpp: proxies for function arguments.  An _OutputArray made from a temporary Mat (desc.row(i).copyTo(descriptors.row(k)))
// refers to a private copy of the header, which shares the storage.
class _InputArray {
public:
    _InputArray(const Mat &m) : m_(m) {}
    bool empty() const { return m_.empty(); }
    Mat getMat() const { return m_; }

private:
    Mat m_;
};
class _OutputArray {
public:
    _OutputArray(Mat &m) : p_(&m) {}
    _OutputArray(const Mat &m) : tmp_(m), p_(&tmp_) {}
    void release() const { p_->release(); }
    void create(int r, int c, int type) const { p_->create(r, c, type); }
    void create(Size sz, int type) const { p_->create(sz, type); }
    Mat getMat() const { return *p_; }

private:
    mutable Mat tmp_;
    Mat *p_;
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;

// copy.cpp Mat::copyTo(OutputArray): dst.create(size, type), then row-wise copy (nothing when source and destination coincide)
inline void Mat::copyTo(const _OutputArray &_dst) const
{
    if (empty()) { _dst.release(); return; }
    _dst.create(rows, cols, CV_8UC1);
    Mat dst = _dst.getMat();
    if (dst.data == data && dst.step == step) return;
    for (int r = 0; r < rows; r++) memmove(dst.data + (size_t)r * dst.step, data + (size_t)r * step, (size_t)cols);
}

// ---- the primitives: OpenCV's argument handling restated, the arithmetic forwarded to the oracle (UNPINNED) ----

// opencv2/core.hpp cv::fastAtan2
inline float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

// opencv2/features2d.hpp cv::FAST(image, keypoints, threshold, nonmaxSuppression), TYPE_9_16: clears the vector, emits
// KeyPoint((float)x, (float)y, 7.f, -1, (float)score) in raster order, coordinates relative to the passed view
inline void FAST(InputArray _img, std::vector<KeyPoint> &keypoints, int threshold, bool nonmaxSuppression = true)
{
    Mat img = _img.getMat();
    keypoints.clear();
    if (img.empty()) return;
    const int cap = img.rows * img.cols;
    std::vector<int> xs(cap), ys(cap), sc(cap);
    const int n = orc_fast_9_16(img.data, (int)img.step, img.cols, img.rows, threshold, nonmaxSuppression ? 1 : 0, xs.data(),
                                ys.data(), sc.data(), cap);
    for (int i = 0; i < n; i++) keypoints.push_back(KeyPoint((float)xs[i], (float)ys[i], 7.f, -1, (float)sc[i]));
}

// opencv2/imgproc.hpp cv::resize: dst.create(dsize) (a no-op for a view of that size), INTER_LINEAR only
inline void resize(InputArray _src, OutputArray _dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR)
{
    Mat src = _src.getMat();
    CV_Assert(interpolation == INTER_LINEAR && fx == 0 && fy == 0 && dsize.width > 0 && dsize.height > 0 && !src.empty());
    _dst.create(dsize, src.type());
    Mat dst = _dst.getMat();
    orc_resize_linear_u8(src.data, src.cols, src.rows, (int)src.step, dst.data, dsize.width, dsize.height, (int)dst.step);
}

// opencv2/core.hpp cv::copyMakeBorder (copy.cpp): without BORDER_ISOLATED a view takes as much of the border as its
// parent holds from the parent's real pixels and only the rest is extrapolated; dst.create is a no-op when dst already has
// the size, so source and destination may be one buffer.  BORDER_REFLECT_101 only.
inline void copyMakeBorder(InputArray _src, OutputArray _dst, int top, int bottom, int left, int right, int borderType)
{
    Mat src = _src.getMat();
    CV_Assert(top >= 0 && bottom >= 0 && left >= 0 && right >= 0 && !src.empty());
    if (src.isSubmatrix() && (borderType & BORDER_ISOLATED) == 0) {
        Size whole;
        Point ofs;
        src.locateROI(whole, ofs);
        int dtop = std::min(ofs.y, top), dbottom = std::min(whole.height - src.rows - ofs.y, bottom);
        int dleft = std::min(ofs.x, left), dright = std::min(whole.width - src.cols - ofs.x, right);
        src.adjustROI(dtop, dbottom, dleft, dright);
        top -= dtop; left -= dleft; bottom -= dbottom; right -= dright;
    }
    borderType &= ~BORDER_ISOLATED;
    CV_Assert(borderType == BORDER_REFLECT_101);
    _dst.create(src.rows + top + bottom, src.cols + left + right, src.type());
    Mat dst = _dst.getMat();
    if (top == bottom && left == right && top == left) {   // every call of the reference
        orc_copy_make_border_101(src.data, src.cols, src.rows, (int)src.step, dst.data, (int)dst.step, top);
        return;
    }
    // unequal borders (a view whose parent supplied part of them): not reached by the reference's own calls
    Mat s = src.clone();
    for (int y = 0; y < dst.rows; y++) {
        int sy = y - top;
        while (s.rows > 1 && (sy < 0 || sy >= s.rows)) sy = sy < 0 ? -sy : 2 * s.rows - 2 - sy;
        for (int x = 0; x < dst.cols; x++) {
            int sx = x - left;
            while (s.cols > 1 && (sx < 0 || sx >= s.cols)) sx = sx < 0 ? -sx : 2 * s.cols - 2 - sx;
            dst.at<uchar>(y, x) = s.at<uchar>(s.rows > 1 ? sy : 0, s.cols > 1 ? sx : 0);
        }
    }
}

// opencv2/imgproc.hpp cv::GaussianBlur: only the reference's call, Size(7,7), sigma 2/2, BORDER_REFLECT_101, source and
// destination the same whole matrix (a clone; a view would read its parent's pixels in OpenCV)
inline void GaussianBlur(InputArray _src, OutputArray _dst, Size ksize, double sigmaX, double sigmaY = 0, int borderType = BORDER_DEFAULT)
{
    Mat src = _src.getMat();
    CV_Assert(ksize.width == 7 && ksize.height == 7 && sigmaX == 2 && sigmaY == 2 && borderType == BORDER_REFLECT_101);
    CV_Assert(!src.empty() && !src.isSubmatrix());
    _dst.create(src.rows, src.cols, src.type());
    Mat dst = _dst.getMat();
    orc_gaussian_blur_7x7_s2(src.data, src.cols, src.rows, (int)src.step, dst.data, (int)dst.step);
}

// opencv2/features2d.hpp KeyPointsFilter::retainBest: keep the n_points strongest and everything tied with the weakest
// kept one.  Here only so that ComputeKeyPointsOld links; nothing calls it.
struct KeyPointsFilter {
    static void retainBest(std::vector<KeyPoint> &keypoints, int n_points)
    {
        if (n_points >= 0 && keypoints.size() > (size_t)n_points) {
            if (n_points == 0) { keypoints.clear(); return; }
            std::nth_element(keypoints.begin(), keypoints.begin() + n_points - 1, keypoints.end(),
                             [](const KeyPoint &a, const KeyPoint &b) { return a.response > b.response; });
            const float ambiguous = keypoints[n_points - 1].response;
            std::vector<KeyPoint>::iterator e =
                std::partition(keypoints.begin() + n_points, keypoints.end(), [ambiguous](const KeyPoint &k) { return k.response >= ambiguous; });
            keypoints.resize(e - keypoints.begin());
        }
    }
};

}  // namespace cv
