// line3D_amd.hpp -- C++ facade with the reference's public interface (class L3D::Line3D, line3D.h:61-101)
// over the C ABI of include/line3d_amd.h.  Same method names, argument order and defaults (commons.h:42-61).
// addImage / addImage_fixed_sim come in two families: (1) the reference's own signatures -- `image` (anything with .cols / .rows: cv::Mat),
// K, R, t matrix-typed (anything with K(i, j) / t(i): Eigen's) -- whose segments are detected on the device from the image's pixels when
// the image type carries them (.data / .step / .channels(), cv::Mat itself) and otherwise come from the segment cache of the data directory,
// the reference's own side door for precomputed segments (line3D.cc:143-168); (2) width, height and the segments the detector would have
// produced (std::vector<float4>, the side door of L3DSegments(list<float4>&, bool), segments.h:60), cameras as plain row-major arrays or
// matrix types.  addImageDistorted / addImage_fixed_simDistorted / undistortImage cover the drivers' undistort block in front of addImage
// (main_vsfm.cpp:243-270) without OpenCV's calib module.  Neither OpenCV nor Eigen is needed to compile this header.
#pragma once

#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <list>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "line3d_amd.h"

namespace L3D {

#ifndef L3D_AMD_HAVE_FLOAT4
struct float4 { float x, y, z, w; };      // the reference gets this type from the CUDA headers
#endif
typedef std::array<double, 3> Vec3d;

namespace detail {
template <int N> struct prio : prio<N - 1> {};      // overload ranking: prio<1> is tried before prio<0>
template <> struct prio<0> {};
}  // namespace detail

// A segment mask (include/line3d_amd.h, "A SEGMENT MASK": l3d_segment_mask) for Line3D::addImageMasked.  `mask`: width x height bytes, rows
// row_stride bytes apart (0: width), in host memory -- onDevice(): in device memory --, which has to live until the call that takes it returns.
// Without a lens the mask lies in the view's grid and has its size; withLens(): in the grid of the lens's distorted image, fx, fy, cx, cy being
// the view's camera.  The mode is one of drop (keep a segment when at least keep_permille of its samples are valid), clip (its longest valid
// stretch) and split (every valid stretch); threshold: the byte value from which a mask pixel counts as valid
class SegmentMask {
public:
    SegmentMask(const void* mask, const int width, const int height, const size_t row_stride = 0) : m_()
    {
        m_.mask = mask; m_.mask_width = width; m_.mask_height = height; m_.mask_row_stride = row_stride ? row_stride : (size_t)(width > 0 ? width : 0);
        m_.mode = L3D_SEGMASK_DROP; m_.threshold = 1; m_.keep_permille = 500;
    }
    SegmentMask& onDevice(const bool on = true) { m_.mask_on_device = on ? 1 : 0; return *this; }
    SegmentMask& withLens(const l3d_lens& lens, const double fx, const double fy, const double cx, const double cy)
    {
        lens_ = lens; has_lens_ = true;
        m_.fx = fx; m_.fy = fy; m_.cx = cx; m_.cy = cy;
        return *this;
    }
    SegmentMask& threshold(const int t) { m_.threshold = t; return *this; }
    SegmentMask& drop(const int keep_permille = 500) { m_.mode = L3D_SEGMASK_DROP; m_.keep_permille = keep_permille; return *this; }
    SegmentMask& clip(const double min_length = 0.0, const int max_gap = 0) { m_.mode = L3D_SEGMASK_CLIP; m_.min_length = min_length; m_.max_gap = max_gap; return *this; }
    SegmentMask& split(const double min_length = 0.0, const int max_gap = 0) { m_.mode = L3D_SEGMASK_SPLIT; m_.min_length = min_length; m_.max_gap = max_gap; return *this; }
    // the struct as the C ABI takes it (valid while this object lives and is not changed)
    const l3d_segment_mask* get() const { m_.lens = has_lens_ ? &lens_ : nullptr; return &m_; }
private:
    mutable l3d_segment_mask m_;
    l3d_lens lens_ = l3d_lens();
    bool has_lens_ = false;
};

// The style of Line3D::overlayView (include/line3d_amd.h, "PROJECTION AND OVERLAYS": l3d_overlay_style) with its defaults: both layers, only the
// lines observed in the view, coloured by line from the default palette, widths 1 and 2 pixels, opaque.  Change the members as needed
struct OverlayStyle : l3d_overlay_style {
    OverlayStyle() : l3d_overlay_style()
    {
        layers = L3D_LAYER_MEMBERS | L3D_LAYER_MODEL; select = L3D_SELECT_OBSERVED; by_line = 1; opacity = 255;
        width_members = 1.0; width_model = 2.0; near_z = 1e-6;
        const unsigned char green[4] = { 0, 255, 0, 255 }, red[4] = { 255, 0, 0, 255 };
        memcpy(color_members, green, 4); memcpy(color_model, red, 4);
    }
};

// commons.h:81-99
class L3DSegment2D {
public:
    L3DSegment2D() : camID_(0), segID_(0) {}
    L3DSegment2D(unsigned int camID, unsigned int segID) : camID_(camID), segID_(segID) {}
    unsigned int camID() const { return camID_; }
    unsigned int segID() const { return segID_; }
    bool operator==(const L3DSegment2D& r) const { return camID_ == r.camID_ && segID_ == r.segID_; }
    bool operator<(const L3DSegment2D& r) const { return camID_ < r.camID_ || (camID_ == r.camID_ && segID_ < r.segID_); }
    bool operator!=(const L3DSegment2D& r) const { return !(*this == r); }
private:
    unsigned int camID_, segID_;
};

// commons.h:215-238
class L3DFinalLine3D {
public:
    L3DFinalLine3D(std::list<L3DSegment2D> segments2D, std::list<std::pair<Vec3d, Vec3d> > segments3D)
        : segments3D_(std::move(segments3D)), segments2D_(std::move(segments2D)) {}
    std::list<std::pair<Vec3d, Vec3d> >* segments3D() { return &segments3D_; }
    std::list<L3DSegment2D>* segments2D() { return &segments2D_; }
private:
    std::list<std::pair<Vec3d, Vec3d> > segments3D_;
    std::list<L3DSegment2D> segments2D_;
};

// What the merging of duplicate lines did in the last compute3Dmodel (Line3D::getMerging; l3d_line3d_get_merging)
struct MergeStats {
    int linesBefore = 0, linesAfter = 0;
    int rounds = 0;                 // rounds in which the search ran (the one that found no pair included)
    int pairsFirstRound = 0;
    int groupsMerged = 0, linesReleased = 0, emptyRefits = 0;       // summed over the rounds
};

// The parameters of the junctions (Line3D::setJunctions; l3d_line3d_set_junctions): two lines meet when their axes pass within distPx pixel footprints
// of each other at an angle of at least angleMinDeg, each prolonged by at most extPx footprints and maxExtRel of its length; snap moves the ends that
// stay in a vertex or rest on another line there, along their own axes
struct JunctionParams {
    double distPx = 4.0, extPx = 12.0, angleMinDeg = 10.0, maxExtRel = 0.25;
    bool snap = false;
};

// A vertex of the wireframe: its position, its lowest staying line end (2 x line + end; end 0 = start of the first 3-D segment) and the ends it joins
struct JunctionVertex {
    double X[3] = { 0.0, 0.0, 0.0 };
    int firstNode = 0, degree = 0;
};

// What the junctions found in the last compute3Dmodel (Line3D::getJunctions; l3d_line3d_get_junctions)
struct JunctionStats {
    std::vector<JunctionVertex> vertices;
    std::vector<int> vertexP, vertexQ, attachLineP, attachLineQ;       // one per line of getResult(); -1: none
    int eligibleLines = 0, lRecords = 0, tRecords = 0, xRecords = 0, components = 0, nodesReleased = 0, nodesAttached = 0, endsMoved = 0, movesSkipped = 0;
};

// The parameters of the planes (Line3D::setPlanes; l3d_line3d_set_planes): two hypotheses -- planes spanned by pairs of lines that meet -- are grouped when
// their normals lie within angleDeg and the lines of each lie within distPx pixel footprints of the other's plane; a plane needs minLines member lines
struct PlaneParams {
    double distPx = 4.0, angleDeg = 10.0;
    int minLines = 3;
};

// A plane of the result: N . X = c, the frame (u, v) at O = c N, the rectangle (min a, max a, min b, max b) of its members' ends in that frame, the
// seed pairs it was averaged from and the lines that lie in it
struct Plane {
    double N[3] = { 0.0, 0.0, 0.0 }, c = 0.0, u[3] = { 0.0, 0.0, 0.0 }, v[3] = { 0.0, 0.0, 0.0 }, rect[4] = { 0.0, 0.0, 0.0, 0.0 };
    int hypotheses = 0;
    std::vector<int> lines;            // indices into getResult(), ascending
    std::vector<bool> seed;            // per member line: it is a line of one of the plane's seed pairs
};

// What the planes found in the last compute3Dmodel (Line3D::getPlanes; l3d_line3d_get_planes)
struct PlaneStats {
    std::vector<Plane> planes;
    std::vector<int> planesPerLine;    // one per line of getResult()
    int eligibleLines = 0, eligibleHypotheses = 0, hypothesisEdges = 0, components = 0, hypothesesReleased = 0, candidatesDropped = 0, memberRecords = 0;
};

// The parameters of the support search (Line3D::gatherSupport; l3d_support_params): a 2-D segment supports a 3-D segment's projection when both of
// its ends lie within distPx of it, the directions within angleDeg, and they overlap by at least minOverlap of the shorter one
struct SupportParams {
    double distPx = 3.0, angleDeg = 5.0, minOverlap = 0.5, nearZ = 1e-6;
    double margin = -1.0;           // pixels around the image within which a projection is kept; negative: distPx
};
// One observation of a line (l3d_line_support): segment `seg` of view `viewID` lies on 3-D segment `seg3D` (index into the flat list of getResult's 3-D
// segments) of the line
struct LineSupport {
    unsigned int viewID = 0, seg = 0;
    int seg3D = 0;
    float dist = 0.0f, overlap = 0.0f;
    bool member = false, memberElsewhere = false, best = false;
};
// What the support did in the last compute3Dmodel (Line3D::getSupport; l3d_line3d_get_support)
struct SupportStats {
    long long records = 0, membersFound = 0, membersNotFound = 0, segmentsUnclaimed = 0;
    std::vector<int> membersBefore, membersAdded, viewsBefore, viewsAfter;       // one per line of getResult()
};

class Line3D {
public:
    // line3D.h:61-66 (data_directory: where addImage keeps its segment caches, line3D.cc:143-150)
    Line3D(const std::string data_directory, const int matchingNeighbors = 10,
           const float uncertainty_t_upper_2D = 5.0f, const float uncertainty_t_lower_2D = 1.0f,
           const float sigma_p = 3.5f, const float sigma_a = 10.0f, const float min_baseline = 0.25f,
           bool useCollinearity = true, bool verbose = false, int device = 0)
        : h_(nullptr), prefix_("[L3D] "), data_directory_(data_directory), use_collinearity_(useCollinearity)
    {
        int rc = l3d_line3d_create(device, matchingNeighbors, uncertainty_t_upper_2D, uncertainty_t_lower_2D, sigma_p, sigma_a,
                                   min_baseline, useCollinearity ? 1 : 0, verbose ? 1 : 0, &h_);
        if (rc != L3D_OK) std::cerr << prefix_ << "no usable HIP device (code " << rc << "); this build has no CPU fallback" << std::endl;
    }
    // One object over several GPUs of this process (l3d_line3d_create_node): rank r on devices[r], a device may repeat (virtual ranks on one
    // GPU).  compute3Dmodel runs matchViews partitioned over the ranks and every method reads the result as above.  A driver changes only its
    // construction line, main_vsfm.cpp:116-119 e.g. to
    //     new L3D::Line3D(data_directory, neighbors, max_uncertainty, min_uncertainty, sigma_p, sigma_a, min_baseline, collinearity, verbose, devices);
    // The reference's parameters are all given here: C++ takes default arguments only at the end of a list, and `devices` has none.
    Line3D(const std::string data_directory, const int matchingNeighbors, const float uncertainty_t_upper_2D, const float uncertainty_t_lower_2D,
           const float sigma_p, const float sigma_a, const float min_baseline, bool useCollinearity, bool verbose, const std::vector<int>& devices)
        : h_(nullptr), prefix_("[L3D] "), data_directory_(data_directory), use_collinearity_(useCollinearity)
    {
        int rc = l3d_line3d_create_node(devices.empty() ? nullptr : devices.data(), (int)devices.size(), matchingNeighbors, uncertainty_t_upper_2D,
                                        uncertainty_t_lower_2D, sigma_p, sigma_a, min_baseline, useCollinearity ? 1 : 0, verbose ? 1 : 0, &h_);
        if (rc != L3D_OK) std::cerr << prefix_ << "no usable set of HIP devices (code " << rc << "); this build has no CPU fallback" << std::endl;
    }
    ~Line3D() { l3d_line3d_destroy(h_); }
    Line3D(const Line3D&) = delete;
    Line3D& operator=(const Line3D&) = delete;
    bool valid() const { return h_ != nullptr; }
    // how an object built from a device list shards matchViews (l3d_line3d_set_node_mode): 0 = the segments of every view (default), 1 = blocks of
    // views, 2 = the ranks of a device take turns on it -- a scene whose kept records do not fit the device at once, at the cost of about one
    // single-device matchViews per rank.  Without effect on a one-device object.  false: no such mode (message printed)
    bool setNodeMode(const int mode) { const int rc = l3d_line3d_set_node_mode(h_, mode); report(rc); return rc == L3D_OK; }
    // node mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover): a turn computes its own piece of the chain from the tail
    // its predecessor left instead of the whole chain.  Without effect in the other modes.  false: a one-device object (message printed)
    bool setTurnHandover(const bool on) { const int rc = l3d_line3d_set_turn_handover(h_, on ? 1 : 0); report(rc); return rc == L3D_OK; }

    // line3D.h:69-73; errors are printed and the call returns, like the reference (line3D.cc:101-127).  `image` is replaced by its size
    // and the segments the detector would have produced; maxImgWidth / loadAndStoreSegments keep their meaning: the segment cache
    // "<data_directory>/segments_<id>_<w'>x<h'>_coll<0|1>.bin" is removed, read INSTEAD of `segments`, or written (line3D.cc:128-199)
    void addImage(const unsigned int imageID, const unsigned int width, const unsigned int height,
                  const std::vector<float4>& segments, const double K[9], const double R[9], const double t[3],
                  std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        std::vector<uint32_t> wps(worldpointIDs.begin(), worldpointIDs.end());
        report(l3d_line3d_add_image_ex(h_, imageID, width, height, segments.empty() ? nullptr : &segments[0].x, (int)segments.size(),
                                       K, R, t, wps.data(), (int)wps.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0));
    }
    // addImage when "<data_directory>/segments_<id>_<w>x<h>_coll<0|1>.bin" of an earlier run exists (line3D.cc:143-168):
    // the file's segments and collinearities stand in for the image (no pixels are needed).
    // false: no such file, or it is not a segment cache (message printed)
    bool addImageFromCache(const unsigned int imageID, const unsigned int width, const unsigned int height,
                           const double K[9], const double R[9], const double t[3], std::list<unsigned int>& worldpointIDs)
    {
        char name[128];
        if (l3d_segment_cache_filename(imageID, width, height, use_collinearity_ ? 1 : 0, name, sizeof(name)) != L3D_OK) return false;
        l3d_segment_cache* cache = nullptr;
        int rc = l3d_segment_cache_read((data_directory_ + name).c_str(), &cache);
        if (rc != L3D_OK) { std::cerr << prefix_ << l3d_segment_cache_last_error(cache) << std::endl; l3d_segment_cache_free(cache); return false; }
        std::vector<uint32_t> wps(worldpointIDs.begin(), worldpointIDs.end());
        rc = l3d_line3d_add_image_cached(h_, imageID, width, height, cache, K, R, t, wps.data(), (int)wps.size());
        l3d_segment_cache_free(cache);
        report(rc);
        return rc == L3D_OK;
    }
    // line3D.h:75-79
    void addImage_fixed_sim(const unsigned int imageID, const unsigned int width, const unsigned int height,
                            const std::vector<float4>& segments, const double K[9], const double R[9], const double t[3],
                            std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        std::vector<uint32_t> ids;
        std::vector<float> sims;
        for (auto& kv : viewSimilarity) { ids.push_back(kv.first); sims.push_back(kv.second); }
        report(l3d_line3d_add_image_fixed_sim_ex(h_, imageID, width, height, segments.empty() ? nullptr : &segments[0].x, (int)segments.size(), K, R, t,
                                                 ids.data(), sims.data(), (int)ids.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0));
    }
    // Segments of the caller's behind a SEGMENT MASK (include/line3d_amd.h, "A SEGMENT MASK": l3d_line3d_add_image_masked): the segments are dropped,
    // clipped or split at the mask on the device, then added as addImage / addImage_fixed_sim add them -- without the segment cache (nothing is
    // read, written or removed).  Segments that all fall to the mask add no view.  false: refused (message printed)
    bool addImageMasked(const unsigned int imageID, const unsigned int width, const unsigned int height, const std::vector<float4>& segments,
                        const double K[9], const double R[9], const double t[3], std::list<unsigned int>& worldpointIDs, const SegmentMask& mask)
    {
        std::vector<uint32_t> wps(worldpointIDs.begin(), worldpointIDs.end());
        const int rc = l3d_line3d_add_image_masked(h_, imageID, width, height, segments.empty() ? nullptr : &segments[0].x, (int)segments.size(), K, R, t,
                                                   wps.data(), nullptr, (int)wps.size(), mask.get());
        report(rc);
        return rc == L3D_OK;
    }
    bool addImageMasked(const unsigned int imageID, const unsigned int width, const unsigned int height, const std::vector<float4>& segments,
                        const double K[9], const double R[9], const double t[3], std::map<unsigned int, float>& viewSimilarity, const SegmentMask& mask)
    {
        std::vector<uint32_t> ids;
        std::vector<float> sims;
        for (auto& kv : viewSimilarity) { ids.push_back(kv.first); sims.push_back(kv.second); }
        if (sims.empty()) sims.push_back(0.0f);             // (no links: refused by the call, as a similarity list -- not read as world points)
        const int rc = l3d_line3d_add_image_masked(h_, imageID, width, height, segments.empty() ? nullptr : &segments[0].x, (int)segments.size(), K, R, t,
                                                   ids.data(), sims.data(), (int)ids.size(), mask.get());
        report(rc);
        return rc == L3D_OK;
    }
    // The same two calls with matrix-typed cameras, as the reference's drivers pass them (Eigen::Matrix3d K, R; Eigen::Vector3d t,
    // main_vsfm.cpp:273-281): any type with K(i, j) / t(i) access -- Eigen is not a dependency of this header.
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage(const unsigned int imageID, const unsigned int width, const unsigned int height, const std::vector<float4>& segments,
                  const M3& K, const M3& R, const V3& t, std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920,
                  const bool loadAndStoreSegments = true)
    {
        double k[9], r[9], tt[3];
        flatten(K, R, t, k, r, tt);
        addImage(imageID, width, height, segments, k, r, tt, worldpointIDs, maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_sim(const unsigned int imageID, const unsigned int width, const unsigned int height, const std::vector<float4>& segments,
                            const M3& K, const M3& R, const V3& t, std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920,
                            const bool loadAndStoreSegments = true)
    {
        double k[9], r[9], tt[3];
        flatten(K, R, t, k, r, tt);
        addImage_fixed_sim(imageID, width, height, segments, k, r, tt, viewSimilarity, maxImgWidth, loadAndStoreSegments);
    }
    // The reference's OWN signatures (line3D.h:69-79): `image` as the second parameter -- cv::Mat in the reference, here any type with
    // `.cols` / `.rows` (cv::Mat itself when OpenCV is there; OpenCV is not a dependency of this header), K / R / t matrix-typed as above.
    // main_vsfm.cpp:273 / main_bundler.cpp:287 compile against these unchanged.
    //   * An image type that also has `.data` (8-bit pixels), `.step` (bytes per row) and `.channels()` (1 or 3) -- cv::Mat -- takes the
    //     reference's path (line3D.cc:143-191, l3d_line3d_add_image_pixels): the segment cache is loaded when it is there and
    //     loadAndStoreSegments is set; otherwise the segments are detected on the device from the pixels, and the cache is written, or a
    //     stale one removed.  An image without segments adds no view.
    //   * A type with only `.cols` / `.rows` gives the view its size and nothing else: the segments come from the segment cache
    //     "<data_directory>/segments_<id>_<w'>x<h'>_coll<0|1>.bin" of an earlier run (w' x h' after the maxImgWidth rule, line3D.cc:130-150).
    //     No such file: the error is printed and the call returns without a view.  loadAndStoreSegments = false removes the file like the
    //     reference does (line3D.cc:153-156) -- and then there is nothing to add.
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, std::list<unsigned int>& worldpointIDs,
                  const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_from_image(detail::prio<1>(), imageID, image, K, R, t, worldpointIDs, nullptr, maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_sim(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, std::map<unsigned int, float>& viewSimilarity,
                            const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_from_image(detail::prio<1>(), imageID, image, K, R, t, viewSimilarity, nullptr, maxImgWidth, loadAndStoreSegments);
    }
    // The drivers' per-image step in front of addImage (main_vsfm.cpp:243-273, main_bundler.cpp:256-287): the image is undistorted on the device
    // with OpenCV-convention radial coefficients k1, k2 and K's fx, fy, cx, cy (an image entry with dist, include/line3d_amd.h), then detected.  For image
    // types that carry pixels; one with a size only takes the cache path as above and the coefficients are ignored.
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageDistorted(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const double k1, const double k2,
                           std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        const double dist[2] = { k1, k2 };
        add_from_image(detail::prio<1>(), imageID, image, K, R, t, worldpointIDs, dist, maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_simDistorted(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const double k1, const double k2,
                                     std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        const double dist[2] = { k1, k2 };
        add_from_image(detail::prio<1>(), imageID, image, K, R, t, viewSimilarity, dist, maxImgWidth, loadAndStoreSegments);
    }
    // cv::initUndistortRectifyMap + cv::remap(image, image, ..., INTER_LINEAR, BORDER_CONSTANT) of the drivers, in place on image.data (staged
    // through a temporary, as remap does when source and destination coincide): undistort, then addImage -- the drivers' own structure
    template <class Img, class M3, class = decltype(static_cast<unsigned char*>(std::declval<Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels())),
              class = decltype(std::declval<const M3&>()(0, 0))>
    bool undistortImage(Img& image, const M3& K, const double k1, const double k2)
    {
        double k[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i * 3 + j] = K(i, j);
        const int w = (int)image.cols, h = (int)image.rows, ch = static_cast<int>(image.channels());
        const size_t step = static_cast<size_t>(image.step), row = (size_t)(w > 0 ? w : 0) * (size_t)(ch > 0 ? ch : 0);
        std::vector<unsigned char> tmp(row * (size_t)(h > 0 ? h : 0) + 1);
        unsigned char* px = static_cast<unsigned char*>(image.data);
        const int rc = l3d_line3d_undistort_image(h_, px, w, h, ch, step, k, k1, k2, tmp.data(), row);
        report(rc);
        if (rc != L3D_OK) return false;
        for (int i = 0; i < h; ++i) memcpy(px + (size_t)i * step, tmp.data() + (size_t)i * row, row);
        return true;
    }
    // The same with a LENS (include/line3d_amd.h, "A LENS": l3d_lens -- tangential, rational and fisheye models): the image is resampled from the
    // lens's source camera onto K, which the view keeps.  For image types that carry pixels, as addImageDistorted
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageLens(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const l3d_lens& lens, std::list<unsigned int>& worldpointIDs,
                      const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, image, K, R, t, worldpointIDs).withLens(lens), maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_simLens(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const l3d_lens& lens,
                                std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, image, K, R, t, viewSimilarity).withLens(lens), maxImgWidth, loadAndStoreSegments);
    }
    // undistortImage with a lens: in place on image.data, K the output camera
    template <class Img, class M3, class = decltype(static_cast<unsigned char*>(std::declval<Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels())),
              class = decltype(std::declval<const M3&>()(0, 0))>
    bool undistortImage(Img& image, const M3& K, const l3d_lens& lens)
    {
        double k[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i * 3 + j] = K(i, j);
        unsigned char* px = static_cast<unsigned char*>(image.data);
        const size_t step = static_cast<size_t>(image.step);
        const int rc = l3d_line3d_undistort_image_lens(h_, px, (int)image.cols, (int)image.rows, static_cast<int>(image.channels()), step, k, &lens, px, step);   // (in place: the library stages the image on the device)
        report(rc);
        return rc == L3D_OK;
    }
    // The drivers' cv::imread in front of that block, for baseline JPEG files: `bytes` are the file's contents; it is decoded on the device
    // (include/line3d_amd.h: byte-identical to libjpeg's default decoder, three channels B, G, R as cv::imread gives them) straight into the
    // detector, undistorted first in the ...Distorted forms.  The cache rules are addImage's; a cache that is present and wanted is loaded
    // without decoding the file.  A file the decoder refuses (progressive, CMYK, corrupt, ...) is reported and adds no view.
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageJPEG(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t,
                      std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, worldpointIDs), maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageJPEGDistorted(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t, const double k1,
                               const double k2, std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, worldpointIDs).distorted(k1, k2), maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_simJPEG(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t,
                                std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, viewSimilarity), maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImage_fixed_simJPEGDistorted(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t,
                                         const double k1, const double k2, std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920,
                                         const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, viewSimilarity).distorted(k1, k2), maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class Links, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageJPEGLens(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t, const l3d_lens& lens,
                          const Links& links /* world point ids, or view similarities */, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, links).withLens(lens), maxImgWidth, loadAndStoreSegments);
    }
    // With a REMAP (include/line3d_amd.h, "A REMAP": l3d_remap -- a lens, another output size, the caller's mask in the source grid, border_mask): K is
    // the OUTPUT camera, which the view keeps; the view and its segment cache file have the remap's output size, and maxImgWidth acts on it.  No
    // line segment starts where a blank or masked pixel contributed to the gradient.  links: world point ids or view similarities
    template <class Img, class M3, class V3, class Links, class = decltype(std::declval<const Img&>().cols), class = decltype(std::declval<const Img&>().rows),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageRemap(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const l3d_remap& remap, const Links& links,
                       const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, image, K, R, t, links).withRemap(remap), maxImgWidth, loadAndStoreSegments);
    }
    template <class M3, class V3, class Links, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    void addImageJPEGRemap(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t, const l3d_remap& remap,
                           const Links& links, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_one(makeEntry(imageID, bytes, n, K, R, t, links).withRemap(remap), maxImgWidth, loadAndStoreSegments);
    }
    // undistortImage with a remap: `out` (and `mask_out`, if given: one channel, 255 = valid) are images of the caller's with the remap's output size --
    // the source's when the remap names none -- and the input's channels; K the output camera.  false: refused, or an output of another size
    template <class Img, class M3, class = decltype(static_cast<unsigned char*>(std::declval<Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels())),
              class = decltype(std::declval<const M3&>()(0, 0))>
    bool undistortImage(const Img& image, const M3& K, const l3d_remap& remap, Img& out, Img* mask_out = nullptr)
    {
        double k[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i * 3 + j] = K(i, j);
        const int ow = remap.out_width > 0 ? remap.out_width : (int)image.cols, oh = remap.out_height > 0 ? remap.out_height : (int)image.rows;
        const int ch = static_cast<int>(image.channels());
        if ((int)out.cols != ow || (int)out.rows != oh || static_cast<int>(out.channels()) != ch ||
            (mask_out && ((int)mask_out->cols != ow || (int)mask_out->rows != oh || static_cast<int>(mask_out->channels()) != 1))) {
            std::cerr << prefix_ << "undistortImage: out (and mask_out) must have the remap's output size, " << ow << " x " << oh << std::endl;
            return false;
        }
        const int rc = l3d_line3d_undistort_image_remap(h_, static_cast<const unsigned char*>(image.data), (int)image.cols, (int)image.rows, ch, static_cast<size_t>(image.step), k,
                                                        &remap, static_cast<unsigned char*>(out.data), static_cast<size_t>(out.step),
                                                        mask_out ? static_cast<unsigned char*>(mask_out->data) : nullptr, mask_out ? static_cast<size_t>(mask_out->step) : 0);
        report(rc);
        return rc == L3D_OK;
    }
    // The planner of include/line3d_amd.h ("A REMAP", l3d_undistort_plan): the output camera K_out and size for a lens that carries its source camera
    // -- no device.  alpha 0: no blank pixel in the output, 1: every source pixel inside fov_max_deg is kept; out_width, out_height: the size, 0 0 for
    // the source's, -1 -1 for the size that keeps the focal length (scaled down to max_dim when that is positive).  false: refused (the cause on cerr)
    template <class M3, class = decltype(std::declval<M3&>()(0, 0) = 0.0)>
    static bool undistortPlan(const l3d_lens& lens, const int width, const int height, const double alpha, M3& K_out, int& out_width, int& out_height,
                              const int max_dim = 0, const double fov_max_deg = 120.0)
    {
        double k[9];
        int w = 0, h = 0;
        if (l3d_undistort_plan(&lens, width, height, alpha, out_width, out_height, max_dim, fov_max_deg, k, &w, &h) != L3D_OK) {
            std::cerr << "[L3D-AMD] " << l3d_undistort_plan_error() << std::endl;
            return false;
        }
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) K_out(i, j) = k[i * 3 + j];
        out_width = w; out_height = h;
        return true;
    }
    // the size and channel count (1: grey, 3: B, G, R) a JPEG file decodes to, from its headers alone -- no device; false: not a file the decoder takes
    static bool jpegSize(const unsigned char* bytes, const size_t n, unsigned int& width, unsigned int& height, unsigned int& channels)
    {
        int w = 0, h = 0, ch = 0;
        if (l3d_jpeg_info(bytes, n, &w, &h, &ch) != L3D_OK) return false;
        width = (unsigned int)w; height = (unsigned int)h; channels = (unsigned int)ch;
        return true;
    }
    // the decoded image: height rows of width x channels bytes into `pixels` (resized), B, G, R for three channels
    bool decodeJPEG(const unsigned char* bytes, const size_t n, std::vector<unsigned char>& pixels, unsigned int& width, unsigned int& height, unsigned int& channels)
    {
        if (!jpegSize(bytes, n, width, height, channels)) { std::cerr << prefix_ << l3d_jpeg_last_error() << std::endl; return false; }
        pixels.assign((size_t)width * height * channels, 0);
        const int rc = l3d_line3d_decode_jpeg(h_, bytes, n, pixels.data(), (size_t)width * channels);
        report(rc);
        return rc == L3D_OK;
    }
    // Many images in one call (l3d_line3d_add_images): what a loop over addImage / addImageDistorted / addImageJPEG[Distorted] and their _fixed_sim
    // forms adds, in entry order, with the detector run once over all images whose cache does not stand in for them.  An entry is built by makeEntry
    // from what those calls take: an image type with pixels (.cols / .rows / .data / .step / .channels(): cv::Mat) or the bytes of a baseline JPEG
    // file, matrix-typed K, R, t, and the links -- a std::list of world point ids or a std::map of view similarities.  .distorted(k1, k2) on the
    // entry gives the ...Distorted forms.  The pixels / bytes are not copied: they have to live until addImages returns.
    struct ImageEntry {
        unsigned int imageID = 0;
        const unsigned char *pixels = nullptr, *jpeg = nullptr;
        int width = 0, height = 0, channels = 0;
        size_t step = 0, jpeg_bytes = 0;
        double K[9], R[9], t[3], dist[2] = { 0.0, 0.0 };
        bool has_dist = false, fixed_sim = false, has_lens = false;
        l3d_lens lens = l3d_lens();     // in the place of dist (withLens); an entry with both is refused
        std::vector<uint32_t> link_ids;
        std::vector<float> sims;
        ImageEntry& distorted(const double k1, const double k2) { dist[0] = k1; dist[1] = k2; has_dist = true; return *this; }
        ImageEntry& withLens(const l3d_lens& l) { lens = l; has_lens = true; return *this; }
        // a remap (include/line3d_amd.h, "A REMAP") in the place of dist and lens: K is the OUTPUT camera (undistortPlan chooses one), the view has the
        // remap's output size.  The remap's lens is copied into the entry; its mask is not -- it has to live until the add call returns
        bool has_remap = false, remap_has_lens = false;
        l3d_remap remap = l3d_remap();
        ImageEntry& withRemap(const l3d_remap& r)
        {
            remap = r; has_remap = true; remap_has_lens = r.lens != nullptr;
            if (r.lens) lens = *r.lens;
            remap.lens = nullptr;           // (set where the entry is handed over: the entry may be copied in between)
            return *this;
        }
        // what the ..._remap calls take for this entry: its remap, a lens alone as a remap that asks for nothing more, or null
        const l3d_remap* remap_for_call(l3d_remap& store) const
        {
            if (has_remap) { store = remap; store.lens = remap_has_lens ? &lens : nullptr; return &store; }
            if (has_lens) { store = l3d_remap(); store.lens = &lens; return &store; }
            return nullptr;
        }
    };
    template <class Img, class M3, class V3, class Links, class = decltype(static_cast<const unsigned char*>(std::declval<const Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels())),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    static ImageEntry makeEntry(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const Links& links)
    {
        ImageEntry e;
        e.imageID = imageID;
        e.pixels = static_cast<const unsigned char*>(image.data);
        e.width = (int)image.cols; e.height = (int)image.rows; e.channels = static_cast<int>(image.channels()); e.step = static_cast<size_t>(image.step);
        flatten(K, R, t, e.K, e.R, e.t);
        set_links(e, links);
        return e;
    }
    template <class M3, class V3, class Links, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    static ImageEntry makeEntry(const unsigned int imageID, const unsigned char* bytes, const size_t n, const M3& K, const M3& R, const V3& t, const Links& links)
    {
        ImageEntry e;
        e.imageID = imageID;
        e.jpeg = bytes; e.jpeg_bytes = n;
        flatten(K, R, t, e.K, e.R, e.t);
        set_links(e, links);
        return e;
    }
    // the per-entry statuses (L3D_OK, or the code the single call would have failed with); the causes are printed, one line per failed entry
    std::vector<int> addImages(const std::vector<ImageEntry>& entries, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        std::vector<l3d_image_entry> e;
        std::vector<const l3d_lens*> lens;
        for (const ImageEntry& s : entries) { e.push_back(to_c(s)); lens.push_back(s.has_lens ? &s.lens : nullptr); }
        std::vector<int> status(entries.size(), L3D_ERR_INVALID);        // (a call refused as a whole -- no object -- leaves them)
        bool remaps = false;
        for (const ImageEntry& s : entries) remaps = remaps || s.has_remap;
        std::vector<l3d_remap> store(entries.size());
        std::vector<const l3d_remap*> remap;
        if (remaps) for (size_t i = 0; i < entries.size(); ++i) remap.push_back(entries[i].remap_for_call(store[i]));
        const int rc = remaps ? l3d_line3d_add_images_remap(h_, e.data(), remap.data(), (int)e.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0, status.data())
                              : l3d_line3d_add_images_lens(h_, e.data(), lens.data(), (int)e.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0, status.data());
        bool any = rc != L3D_OK;
        for (int st : status) any = any || st != L3D_OK;
        if (any) std::cerr << prefix_ << l3d_line3d_last_error(h_) << std::endl;
        return status;
    }
    // Images in DEVICE memory (include/line3d_amd.h, "Images in DEVICE memory"): a cv::cuda::GpuMat, a frame of a decoder, a tensor's pointer.
    // A GpuMat has cv::Mat's members (.data, .step, .cols, .rows, .channels()), so the overloads above would take its pointer for host memory:
    // the device forms have NAMES OF THEIR OWN and nothing is detected automatically.  An image type with those members is taken as 8-bit
    // interleaved pixels with `step` in bytes; every other layout and type (planar, float, 16-bit, strided, flipped) comes as an
    // l3d_device_image, filled by the caller.  `stream`: the hipStream_t the pixels were produced on (nullptr: the null stream); the library
    // waits for it before reading, and every call returns with the image consumed (an output: written).  The cache rules are addImage's: a
    // cache that is present and wanted stands in for the image, whose memory is then not touched.
    template <class Img, class = decltype(static_cast<const unsigned char*>(std::declval<const Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels()))>
    static l3d_device_image deviceImage(const Img& image, void* stream = nullptr)
    {
        l3d_device_image d;
        d.ptr = static_cast<const unsigned char*>(image.data);
        d.width = (int)image.cols; d.height = (int)image.rows; d.channels = static_cast<int>(image.channels());
        d.dtype = L3D_U8;
        d.stride_y = (long long)static_cast<size_t>(image.step); d.stride_x = d.channels; d.stride_c = 1;
        d.chan[0] = 0; d.chan[1] = 1; d.chan[2] = 2;
        d.scale = 1.0f;
        d.stream = stream;
        return d;
    }
    struct DeviceEntry {
        ImageEntry base;                // the id, the camera, dist and the links; no pixels and no file
        l3d_device_image image;
        DeviceEntry& distorted(const double k1, const double k2) { base.distorted(k1, k2); return *this; }
        DeviceEntry& withLens(const l3d_lens& l) { base.withLens(l); return *this; }
        DeviceEntry& withRemap(const l3d_remap& r) { base.withRemap(r); return *this; }
    };
    template <class M3, class V3, class Links, class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    static DeviceEntry makeDeviceEntry(const unsigned int imageID, const l3d_device_image& image, const M3& K, const M3& R, const V3& t, const Links& links)
    {
        DeviceEntry e;
        e.base.imageID = imageID;
        e.image = image;
        flatten(K, R, t, e.base.K, e.base.R, e.base.t);
        set_links(e.base, links);
        return e;
    }
    template <class Img, class M3, class V3, class Links, class = decltype(static_cast<const unsigned char*>(std::declval<const Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels())),
              class = decltype(std::declval<const M3&>()(0, 0)), class = decltype(std::declval<const V3&>()(0))>
    static DeviceEntry makeDeviceEntry(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const Links& links, void* stream = nullptr)
    {
        return makeDeviceEntry(imageID, deviceImage(image, stream), K, R, t, links);
    }
    // `image`: an l3d_device_image, or an image type with a GpuMat's members (on the null stream; another stream: makeDeviceEntry + addImagesDevice)
    template <class Img, class M3, class V3>
    void addImageDevice(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, std::list<unsigned int>& worldpointIDs,
                        const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, worldpointIDs), maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3>
    void addImageDeviceDistorted(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const double k1, const double k2,
                                 std::list<unsigned int>& worldpointIDs, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, worldpointIDs).distorted(k1, k2), maxImgWidth, loadAndStoreSegments);
    }
    // with a lens; links: world point ids or view similarities
    template <class Img, class M3, class V3, class Links>
    void addImageDeviceLens(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const l3d_lens& lens, const Links& links,
                            const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, links).withLens(lens), maxImgWidth, loadAndStoreSegments);
    }
    // with a remap (see addImageRemap); a mask in device memory: remap.mask_on_device
    template <class Img, class M3, class V3, class Links>
    void addImageDeviceRemap(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const l3d_remap& remap, const Links& links,
                             const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, links).withRemap(remap), maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3>
    void addImage_fixed_simDevice(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, std::map<unsigned int, float>& viewSimilarity,
                                  const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, viewSimilarity), maxImgWidth, loadAndStoreSegments);
    }
    template <class Img, class M3, class V3>
    void addImage_fixed_simDeviceDistorted(const unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const double k1, const double k2,
                                           std::map<unsigned int, float>& viewSimilarity, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        add_device(makeDeviceEntry(imageID, image, K, R, t, viewSimilarity).distorted(k1, k2), maxImgWidth, loadAndStoreSegments);
    }
    // addImages for device images (l3d_line3d_add_device_images): one run of the detector, one gather launch per chunk; statuses as addImages
    std::vector<int> addImagesDevice(const std::vector<DeviceEntry>& entries, const int maxImgWidth = 1920, const bool loadAndStoreSegments = true)
    {
        std::vector<l3d_device_entry> e;
        std::vector<const l3d_lens*> lens;
        for (const DeviceEntry& s : entries) { e.push_back(to_c(s)); lens.push_back(s.base.has_lens ? &s.base.lens : nullptr); }
        std::vector<int> status(entries.size(), L3D_ERR_INVALID);
        bool remaps = false;
        for (const DeviceEntry& s : entries) remaps = remaps || s.base.has_remap;
        std::vector<l3d_remap> store(entries.size());
        std::vector<const l3d_remap*> remap;
        if (remaps) for (size_t i = 0; i < entries.size(); ++i) remap.push_back(entries[i].base.remap_for_call(store[i]));
        const int rc = remaps ? l3d_line3d_add_device_images_remap(h_, e.data(), remap.data(), (int)e.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0, status.data())
                              : l3d_line3d_add_device_images_lens(h_, e.data(), lens.data(), (int)e.size(), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0, status.data());
        bool any = rc != L3D_OK;
        for (int st : status) any = any || st != L3D_OK;
        if (any) std::cerr << prefix_ << l3d_line3d_last_error(h_) << std::endl;
        return status;
    }
    // decodeJPEG into the caller's device memory: out's size and channels (1, or 3 / 4 for a colour file) must be the file's (jpegSize)
    bool decodeJPEGDevice(const unsigned char* bytes, const size_t n, const l3d_device_image& out)
    {
        const int rc = l3d_line3d_decode_jpeg_device(h_, bytes, n, &out);
        report(rc);
        return rc == L3D_OK;
    }
    // undistortImage on the device: `in` and `out` of one size and channel count; they may describe the same memory
    template <class M3, class = decltype(std::declval<const M3&>()(0, 0))>
    bool undistortImageDevice(const l3d_device_image& in, const M3& K, const double k1, const double k2, const l3d_device_image& out)
    {
        double k[9];
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) k[i * 3 + j] = K(i, j);
        const int rc = l3d_line3d_undistort_image_device(h_, &in, k, k1, k2, &out);
        report(rc);
        return rc == L3D_OK;
    }
    // line3D.h:82
    void compute3Dmodel(bool perform_diffusion = false) { report(l3d_line3d_compute3Dmodel(h_, perform_diffusion ? 1 : 0)); }
    // Refinement of the result (no counterpart in the reference; l3d_line3d_set_refinement): with it on, compute3Dmodel refines every 3-D line against the
    // 2-D segments of its cluster and replaces its 3-D segments by collinear ones -- lines, their order and their 2-D segments stay.  Off by default; reset()
    // keeps the setting.  huberPx: scale of the Huber loss in pixels, 0 = plain least squares.
    void setRefinement(bool on, int maxIterations = 20, double huberPx = 2.0) { report(l3d_line3d_set_refinement(h_, on ? 1 : 0, maxIterations, huberPx)); }
    // one entry per line of getResult(): pixel rms of the members' 2-D end points before and after, and the status (0 refined, 1 starting line kept, 2 degenerate,
    // 3 refined sweep empty: unrefined segments kept).  false (and empty vectors) when the last compute3Dmodel ran without the refinement.
    bool getRefinement(std::vector<double>& rmsBefore, std::vector<double>& rmsAfter, std::vector<int>& status)
    {
        rmsBefore.clear(); rmsAfter.clear(); status.clear();
        int nl = 0;
        if (l3d_line3d_result_sizes(h_, &nl, nullptr, nullptr) != L3D_OK) return false;
        std::vector<double> rb((size_t)nl), ra((size_t)nl);
        std::vector<int32_t> st((size_t)nl);
        if (l3d_line3d_get_refinement(h_, rb.data(), ra.data(), nullptr, st.data()) != L3D_OK) return false;
        rmsBefore = rb; rmsAfter = ra; status.assign(st.begin(), st.end());
        return true;
    }
    // Merging of duplicate lines (no counterpart in the reference; l3d_line3d_set_merging, "MERGING DUPLICATE LINES" in line3d_amd.h): with it on,
    // compute3Dmodel groups the near-copies of a 3-D line (ends within distPx pixel footprints of the longer line's axis, directions within angleDeg,
    // a gap along the axis of at most maxGap times the shorter length), refits every group from all of its 2-D segments and repeats, maxRounds times at
    // the most, before the refinement.  Off by default; reset() keeps the setting.
    void setMerging(bool on = true, double distPx = 4.0, double angleDeg = 5.0, double maxGap = 0.0, int maxRounds = 3)
    {
        report(l3d_line3d_set_merging(h_, on ? 1 : 0, distPx, angleDeg, maxGap, maxRounds));
    }
    // finalIndex (optional): one entry per line BEFORE merging, its index in getResult(); nSources (optional): one per line of getResult(), the lines it
    // was made of.  false when the last compute3Dmodel ran without the merging.
    bool getMerging(MergeStats& stats, std::vector<int>* finalIndex = nullptr, std::vector<int>* nSources = nullptr)
    {
        int32_t c[8];
        if (l3d_line3d_get_merging(h_, c, nullptr, nullptr) != L3D_OK) return false;
        stats.linesBefore = c[0]; stats.linesAfter = c[1]; stats.rounds = c[2]; stats.pairsFirstRound = c[3];
        stats.groupsMerged = c[4]; stats.linesReleased = c[5]; stats.emptyRefits = c[6];
        std::vector<int32_t> fi((size_t)c[0] + 1), ns((size_t)c[1] + 1);
        if (l3d_line3d_get_merging(h_, c, fi.data(), ns.data()) != L3D_OK) return false;
        if (finalIndex) finalIndex->assign(fi.begin(), fi.begin() + c[0]);
        if (nSources) nSources->assign(ns.begin(), ns.begin() + c[1]);
        return true;
    }
    // Support of the result's lines over ALL views (no counterpart in the reference; "SUPPORT OF 3-D LINES" in line3d_amd.h).  gatherSupport, valid behind
    // compute3Dmodel: per line of getResult() the 2-D segments of every view that lie on it, ordered by (view id, segment).  false: refused
    bool gatherSupport(std::vector<std::vector<LineSupport> >& perLine, const SupportParams& params = SupportParams())
    {
        perLine.clear();
        int nl = 0;
        if (l3d_line3d_result_sizes(h_, &nl, nullptr, nullptr) != L3D_OK) return false;
        l3d_support_params p;
        p.dist_px = params.distPx; p.cos_min = std::cos(params.angleDeg * 3.14159265358979323846 / 180.0); p.min_overlap = params.minOverlap;
        p.near_z = params.nearZ; p.margin = params.margin < 0.0 ? params.distPx : params.margin;
        l3d_line_support* rec = nullptr;
        std::vector<int64_t> start((size_t)nl + 1);
        int64_t counts[4];
        if (l3d_line3d_gather_support(h_, &p, &rec, start.data(), nullptr, counts) != L3D_OK) return false;
        perLine.resize((size_t)nl);
        for (int k = 0; k < nl; ++k)
            for (int64_t r = start[(size_t)k]; r < start[(size_t)k + 1]; ++r) {
                LineSupport o;
                o.viewID = rec[r].view_id; o.seg = rec[r].seg; o.seg3D = rec[r].seg3d; o.dist = rec[r].dist; o.overlap = rec[r].overlap;
                o.member = (rec[r].flags & L3D_SUPPORT_MEMBER) != 0; o.memberElsewhere = (rec[r].flags & L3D_SUPPORT_MEMBER_ELSEWHERE) != 0;
                o.best = (rec[r].flags & L3D_SUPPORT_BEST) != 0;
                perLine[(size_t)k].push_back(o);
            }
        l3d_free(rec);
        return true;
    }
    // With it on, compute3Dmodel ends with the gather -- after the line fit, the merging and the refinement -- and appends to every line's 2-D segments
    // the segments of all views for which it holds the best row and that are members of no line.  Off by default; reset() keeps the setting.
    void setSupport(bool on = true, double distPx = 3.0, double angleDeg = 5.0, double minOverlap = 0.5)
    {
        report(l3d_line3d_set_support(h_, on ? 1 : 0, distPx, angleDeg, minOverlap));
    }
    // false when the last compute3Dmodel ran without the support
    bool getSupport(SupportStats& stats)
    {
        int nl = 0;
        int64_t c[4];
        if (l3d_line3d_result_sizes(h_, &nl, nullptr, nullptr) != L3D_OK) return false;
        std::vector<int32_t> per((size_t)nl * 4 + 4);
        if (l3d_line3d_get_support(h_, c, per.data()) != L3D_OK) return false;
        stats.records = c[0]; stats.membersFound = c[1]; stats.membersNotFound = c[2]; stats.segmentsUnclaimed = c[3];
        stats.membersBefore.resize((size_t)nl); stats.membersAdded.resize((size_t)nl); stats.viewsBefore.resize((size_t)nl); stats.viewsAfter.resize((size_t)nl);
        for (int k = 0; k < nl; ++k) {
            stats.membersBefore[(size_t)k] = per[(size_t)k * 4]; stats.membersAdded[(size_t)k] = per[(size_t)k * 4 + 1];
            stats.viewsBefore[(size_t)k] = per[(size_t)k * 4 + 2]; stats.viewsAfter[(size_t)k] = per[(size_t)k * 4 + 3];
        }
        return true;
    }
    // Junctions of the result's lines: a wireframe (no counterpart in the reference; "JUNCTIONS OF 3-D LINES" in line3d_amd.h).  With it on, compute3Dmodel
    // finds where lines meet after the merging and the refinement and before the support: the line ends grouped into vertices, and the free ends that
    // rest on the inside of another line.  Off by default; reset() keeps the setting.
    void setJunctions(bool on = true, const JunctionParams& p = JunctionParams())
    {
        report(l3d_line3d_set_junctions(h_, on ? 1 : 0, p.distPx, p.extPx, p.angleMinDeg, p.maxExtRel, p.snap ? 1 : 0));
    }
    // false when the last compute3Dmodel ran without the junctions
    bool getJunctions(JunctionStats& stats)
    {
        int nl = 0, nv = 0;
        int32_t c[10];
        if (l3d_line3d_result_sizes(h_, &nl, nullptr, nullptr) != L3D_OK) return false;
        std::vector<int32_t> per((size_t)nl * 4 + 4);
        l3d_junction_vertex* v = nullptr;
        if (l3d_line3d_get_junctions(h_, &v, &nv, per.data(), c) != L3D_OK) return false;
        stats.vertices.resize((size_t)nv);
        for (int k = 0; k < nv; ++k) {
            JunctionVertex& o = stats.vertices[(size_t)k];
            o.X[0] = v[k].X[0]; o.X[1] = v[k].X[1]; o.X[2] = v[k].X[2]; o.firstNode = v[k].first_node; o.degree = v[k].degree;
        }
        l3d_free(v);
        stats.vertexP.resize((size_t)nl); stats.vertexQ.resize((size_t)nl); stats.attachLineP.resize((size_t)nl); stats.attachLineQ.resize((size_t)nl);
        for (int k = 0; k < nl; ++k) {
            stats.vertexP[(size_t)k] = per[(size_t)k * 4]; stats.vertexQ[(size_t)k] = per[(size_t)k * 4 + 1];
            stats.attachLineP[(size_t)k] = per[(size_t)k * 4 + 2]; stats.attachLineQ[(size_t)k] = per[(size_t)k * 4 + 3];
        }
        stats.eligibleLines = c[0]; stats.lRecords = c[1]; stats.tRecords = c[2]; stats.xRecords = c[3]; stats.components = c[4];
        stats.nodesReleased = c[6]; stats.nodesAttached = c[7]; stats.endsMoved = c[8]; stats.movesSkipped = c[9];
        return true;
    }
    // the current result as a Wavefront OBJ wireframe (l3d_line3d_save_wireframe): the vertices of the junctions, then every line as a group of its
    // own; an end that stays in a vertex uses the shared index.  Works without the junctions too: then no index is shared.  false: not written
    bool save3DLinesAsOBJ(const std::string& filename) { return l3d_line3d_save_wireframe(h_, filename.c_str()) == L3D_OK; }
    // Planes of the result's lines: faces for the wireframe (no counterpart in the reference; "PLANES OF 3-D LINES" in line3d_amd.h).  With it on,
    // compute3Dmodel finds which lines lie in one plane, after the junctions -- whose search runs for the seed pairs even when setJunctions is off -- and
    // before the support.  Off by default; reset() keeps the setting.
    void setPlanes(bool on = true, const PlaneParams& p = PlaneParams()) { report(l3d_line3d_set_planes(h_, on ? 1 : 0, p.distPx, p.angleDeg, p.minLines)); }
    // false when the last compute3Dmodel ran without the planes
    bool getPlanes(PlaneStats& stats)
    {
        int nl = 0, np = 0, nm = 0;
        int32_t c[8];
        if (l3d_line3d_result_sizes(h_, &nl, nullptr, nullptr) != L3D_OK) return false;
        std::vector<int32_t> per((size_t)nl + 1);
        l3d_plane* pl = nullptr;
        l3d_plane_member* mem = nullptr;
        if (l3d_line3d_get_planes(h_, &pl, &np, &mem, &nm, per.data(), c) != L3D_OK) return false;
        stats.planes.assign((size_t)np, Plane());
        for (int k = 0; k < np; ++k) {
            Plane& o = stats.planes[(size_t)k];
            for (int d = 0; d < 3; ++d) { o.N[d] = pl[k].N[d]; o.u[d] = pl[k].u[d]; o.v[d] = pl[k].v[d]; }
            for (int d = 0; d < 4; ++d) o.rect[d] = pl[k].rect[d];
            o.c = pl[k].c; o.hypotheses = pl[k].n_hyp;
        }
        for (int k = 0; k < nm; ++k) {
            Plane& o = stats.planes[(size_t)mem[k].plane];
            o.lines.push_back(mem[k].line);
            o.seed.push_back((mem[k].flags & L3D_PLANE_SEED) != 0);
        }
        l3d_free(pl); l3d_free(mem);
        stats.planesPerLine.assign(per.begin(), per.begin() + nl);
        stats.eligibleLines = c[0]; stats.eligibleHypotheses = c[1]; stats.hypothesisEdges = c[2]; stats.components = c[3]; stats.hypothesesReleased = c[4];
        stats.candidatesDropped = c[5]; stats.memberRecords = c[7];
        return true;
    }
    // the planes of the last compute3Dmodel as a Wavefront OBJ (l3d_line3d_save_planes): per plane a group of the four corners of its rectangle and one
    // face.  false: not written (also when the last compute3Dmodel ran without the planes)
    bool save3DPlanesAsOBJ(const std::string& filename) { return l3d_line3d_save_planes(h_, filename.c_str()) == L3D_OK; }
    // Where addImage's world point links are filed (no counterpart in the reference; l3d_line3d_set_covisibility): false, the default, on the host as every
    // view is added; true: the lists are stored and compute3Dmodel counts them on the device -- the same neighbours and the same result.  Refused while the
    // object holds views; reset() keeps the setting.
    void setDeviceCovisibility(bool on) { report(l3d_line3d_set_covisibility(h_, on ? 1 : 0)); }
    // what compute3Dmodel chose (valid behind it): the visual neighbours of a view, ascending ids
    std::vector<unsigned int> getNeighbors(const unsigned int camID)
    {
        int n = 0;
        if (l3d_line3d_get_neighbors(h_, camID, nullptr, 0, &n) != L3D_OK || n <= 0) return {};
        std::vector<uint32_t> ids((size_t)n);
        l3d_line3d_get_neighbors(h_, camID, ids.data(), n, &n);
        return std::vector<unsigned int>(ids.begin(), ids.end());
    }
    // ... and its similarities by the other view's id
    std::map<unsigned int, float> getViewSimilarities(const unsigned int camID)
    {
        std::map<unsigned int, float> out;
        int n = 0;
        if (l3d_line3d_get_view_similarities(h_, camID, nullptr, nullptr, 0, &n) != L3D_OK || n <= 0) return out;
        std::vector<uint32_t> ids((size_t)n);
        std::vector<float> sims((size_t)n);
        l3d_line3d_get_view_similarities(h_, camID, ids.data(), sims.data(), n, &n);
        for (size_t i = 0; i < ids.size(); ++i) out[ids[i]] = sims[i];
        return out;
    }
    // line3D.h:85
    void getResult(std::list<L3DFinalLine3D>& result)
    {
        result.clear();
        int nl = 0, n3 = 0, n2 = 0;
        if (l3d_line3d_result_sizes(h_, &nl, &n3, &n2) != L3D_OK || nl == 0) return;
        std::vector<int> l3((size_t)nl), l2((size_t)nl);
        std::vector<double> s3((size_t)n3 * 6);
        std::vector<uint32_t> s2((size_t)n2 * 2);
        l3d_line3d_get_result(h_, l3.data(), l2.data(), s3.data(), s2.data());
        size_t a = 0, b = 0;
        for (int k = 0; k < nl; ++k) {
            std::list<std::pair<Vec3d, Vec3d> > seg3;
            std::list<L3DSegment2D> seg2;
            for (int i = 0; i < l3[(size_t)k]; ++i, a += 6)
                seg3.push_back({ Vec3d{ s3[a], s3[a + 1], s3[a + 2] }, Vec3d{ s3[a + 3], s3[a + 4], s3[a + 5] } });
            for (int i = 0; i < l2[(size_t)k]; ++i, b += 2) seg2.push_back(L3DSegment2D(s2[b], s2[b + 1]));
            result.push_back(L3DFinalLine3D(seg2, seg3));
        }
    }
    // line3D.h:88
    float4 getSegment2D(L3DSegment2D& seg2D)
    {
        float o[4] = { 0.0f, 0.0f, 0.0f, 0.0f };   // (stays zero when the handle is null: the constructor found no HIP device)
        if (l3d_line3d_get_segment2D(h_, seg2D.camID(), seg2D.segID(), o) != L3D_OK)
            std::cerr << prefix_ << "no view with ID " << seg2D.camID() << "!" << std::endl;
        return float4{ o[0], o[1], o[2], o[3] };
    }
    // ---- the result over the views (no counterpart in the reference; include/line3d_amd.h, "PROJECTION AND OVERLAYS")
    // The result's 3-D segments projected into views: camera-major, camStart[c] .. camStart[c + 1] are view viewIDs[c]'s.  segIndex counts the 3-D
    // segments in getResult()'s order, lineIndex its lines; flags bit 0 / 1: the first / second end was moved by the near plane or the image's border.
    // select: L3D_SELECT_ALL, or L3D_SELECT_OBSERVED (only lines with a 2-D segment in the view).  The cameras are the views' own, as they were added
    struct Projection {
        std::vector<float4> segments;
        std::vector<int> segIndex, lineIndex;
        std::vector<unsigned char> flags;
        std::vector<long long> camStart;
    };
    Projection projectResult(const std::vector<unsigned int>& viewIDs, const int select = L3D_SELECT_ALL, const double nearZ = 1e-6, const double margin = 0.0)
    {
        Projection p;
        std::vector<uint32_t> ids(viewIDs.begin(), viewIDs.end());
        std::vector<int64_t> start(ids.size() + 1, 0);
        float* s = nullptr; int32_t* si = nullptr; int32_t* li = nullptr; unsigned char* fl = nullptr;
        const int rc = l3d_line3d_project_result(h_, ids.data(), (int)ids.size(), nullptr, select, nearZ, margin, &s, &si, &li, &fl, start.data());
        report(rc);
        if (rc != L3D_OK) return p;
        const size_t n = (size_t)start.back();
        for (size_t k = 0; k < n; ++k) p.segments.push_back(float4{ s[4 * k], s[4 * k + 1], s[4 * k + 2], s[4 * k + 3] });
        p.segIndex.assign(si, si + n); p.lineIndex.assign(li, li + n); p.flags.assign(fl, fl + n);
        p.camStart.assign(start.begin(), start.end());
        l3d_free(s); l3d_free(si); l3d_free(li); l3d_free(fl);
        return p;
    }
    // Overlay of a view: its 2-D segments that belong to a line, then the projected result, drawn over `image` (8 bits, the view's size) in place.
    // `image`: anything with .data, .step, .cols, .rows and .channels() (cv::Mat).  style: L3D::OverlayStyle(), changed through its members
    template <class Img, class = decltype(static_cast<unsigned char*>(std::declval<Img&>().data)), class = decltype(static_cast<int>(std::declval<const Img&>().channels()))>
    bool overlayView(const unsigned int viewID, Img& image, const l3d_overlay_style& style)
    {
        const int rc = l3d_line3d_overlay(h_, viewID, static_cast<unsigned char*>(image.data), (int)image.cols, (int)image.rows, (int)image.channels(), (size_t)image.step, &style);
        report(rc);
        return rc == L3D_OK;
    }
    // ... over an image in device memory (L3D_U8; deviceImage() fills the descriptor of a GpuMat)
    bool overlayViewDevice(const unsigned int viewID, const l3d_device_image& image, const l3d_overlay_style& style)
    {
        const int rc = l3d_line3d_overlay_device(h_, viewID, &image, &style);
        report(rc);
        return rc == L3D_OK;
    }
    // segments of the caller's (the image's grid) drawn over `image` on the object's device: segment k takes colours[k % colours.size()],
    // (c0, c1, c2, alpha) in the image's channel order
    template <class Img, class = decltype(static_cast<unsigned char*>(std::declval<Img&>().data)), class = decltype(static_cast<int>(std::declval<const Img&>().channels()))>
    bool drawSegments(Img& image, const std::vector<float4>& segments, const std::vector<std::array<unsigned char, 4> >& colours, const double widthPx = 1.0, const int opacity = 255)
    {
        std::vector<float> s;
        for (const float4& f : segments) { s.push_back(f.x); s.push_back(f.y); s.push_back(f.z); s.push_back(f.w); }
        std::vector<unsigned char> c;
        for (auto& col : colours) c.insert(c.end(), col.begin(), col.end());
        l3d_ctx* ctx = l3d_line3d_context(h_);
        const int rc = l3d_draw_segments(ctx, static_cast<unsigned char*>(image.data), (int)image.cols, (int)image.rows, (int)image.channels(), (size_t)image.step,
                                         s.data(), (int)segments.size(), c.data(), (int)colours.size(), nullptr, widthPx, opacity);
        if (rc != L3D_OK) std::cerr << prefix_ << (ctx ? l3d_last_error(ctx) : "no device context") << std::endl;
        return rc == L3D_OK;
    }
    // line3D.h:91,94 -- `result` is written as given (the caller may have filtered it); formats as in line3D.cc:384-473
    void save3DLinesAsSTL(std::list<L3DFinalLine3D>& result, std::string filename)
    {
        FILE* f = fopen(filename.c_str(), "w");
        if (!f) return;
        fprintf(f, "solid lineModel\n");
        for (L3DFinalLine3D& l : result)
            for (auto& sg : *l.segments3D()) {
                fprintf(f, " facet normal 1.0e+000 0.0e+000 0.0e+000\n  outer loop\n");
                fprintf(f, "   vertex %e %e %e\n", (double)sg.first[0], (double)sg.first[1], (double)sg.first[2]);
                fprintf(f, "   vertex %e %e %e\n", (double)sg.second[0], (double)sg.second[1], (double)sg.second[2]);
                fprintf(f, "   vertex %e %e %e\n", (double)sg.first[0], (double)sg.first[1], (double)sg.first[2]);
                fprintf(f, "  endloop\n endfacet\n");
            }
        fprintf(f, "endsolid lineModel\n");
        fclose(f);
    }
    void save3DLinesAsTXT(std::list<L3DFinalLine3D>& result, std::string filename)
    {
        FILE* f = fopen(filename.c_str(), "w");
        if (!f) return;
        for (L3DFinalLine3D& l : result) {
            if (l.segments3D()->empty()) continue;
            fprintf(f, "%zu ", l.segments3D()->size());
            for (auto& sg : *l.segments3D())
                fprintf(f, "%g %g %g %g %g %g ", (double)sg.first[0], (double)sg.first[1], (double)sg.first[2], (double)sg.second[0], (double)sg.second[1], (double)sg.second[2]);
            fprintf(f, "%zu ", l.segments2D()->size());
            for (L3DSegment2D& s2 : *l.segments2D()) {
                const float4 c = getSegment2D(s2);
                fprintf(f, "%u %u %g %g %g %g ", s2.camID(), s2.segID(), (double)c.x, (double)c.y, (double)c.z, (double)c.w);
            }
            fprintf(f, "\n");
        }
        fclose(f);
    }
    unsigned int numCameras() { return (unsigned int)l3d_line3d_num_cameras(h_); }   // line3D.h:98
    void reset() { l3d_line3d_reset(h_); }                                            // line3D.h:101
    l3d_line3d* handle() { return h_; }

private:
    template <class M3, class V3> static void flatten(const M3& K, const M3& R, const V3& t, double* k, double* r, double* tt)
    {
        for (int i = 0; i < 3; ++i) { tt[i] = t(i); for (int j = 0; j < 3; ++j) { k[i * 3 + j] = K(i, j); r[i * 3 + j] = R(i, j); } }
    }
    // the l3d_image_entry of an entry (it points into `s`)
    static l3d_image_entry to_c(const ImageEntry& s)
    {
        l3d_image_entry d;
        d.image_id = s.imageID;
        d.pixels = s.pixels; d.width = s.width; d.height = s.height; d.channels = s.channels; d.row_stride = s.step;
        d.jpeg = s.jpeg; d.jpeg_bytes = s.jpeg_bytes;
        d.K = s.K; d.R = s.R; d.t = s.t; d.dist = s.has_dist ? s.dist : nullptr;
        d.link_ids = s.link_ids.data(); d.sims = s.fixed_sim ? s.sims.data() : nullptr; d.n_links = (int)s.link_ids.size();
        return d;
    }
    static l3d_device_entry to_c(const DeviceEntry& s)
    {
        l3d_device_entry d;
        d.image_id = s.base.imageID;
        d.image = s.image;
        d.K = s.base.K; d.R = s.base.R; d.t = s.base.t; d.dist = s.base.has_dist ? s.base.dist : nullptr;
        d.link_ids = s.base.link_ids.data(); d.sims = s.base.fixed_sim ? s.base.sims.data() : nullptr; d.n_links = (int)s.base.link_ids.size();
        return d;
    }
    void add_device(const DeviceEntry& s, int maxImgWidth, bool loadAndStoreSegments)
    {
        const l3d_device_entry e = to_c(s);
        l3d_remap store;
        if (s.base.has_remap) { report(l3d_line3d_add_device_entry_remap(h_, &e, s.base.remap_for_call(store), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0)); return; }
        report(l3d_line3d_add_device_entry_lens(h_, &e, s.base.has_lens ? &s.base.lens : nullptr, data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0));
    }
    // every image and JPEG form: one entry through the library's one route (l3d_line3d_add_image_entry)
    void add_one(const ImageEntry& s, int maxImgWidth, bool loadAndStoreSegments)
    {
        const l3d_image_entry e = to_c(s);
        l3d_remap store;
        if (s.has_remap) { report(l3d_line3d_add_image_entry_remap(h_, &e, s.remap_for_call(store), data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0)); return; }
        report(l3d_line3d_add_image_entry_lens(h_, &e, s.has_lens ? &s.lens : nullptr, data_directory_.c_str(), maxImgWidth, loadAndStoreSegments ? 1 : 0));
    }
    // `image` with pixels (cv::Mat: .data, .step, .channels()): detect on the device.  links: world point ids or view similarities; dist: null or k1, k2
    template <class Img, class M3, class V3, class Links, class = decltype(static_cast<const unsigned char*>(std::declval<const Img&>().data)),
              class = decltype(static_cast<size_t>(std::declval<const Img&>().step)), class = decltype(static_cast<int>(std::declval<const Img&>().channels()))>
    void add_from_image(detail::prio<1>, unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const Links& links, const double* dist,
                        int maxImgWidth, bool loadAndStoreSegments)
    {
        ImageEntry e = makeEntry(imageID, image, K, R, t, links);
        if (dist) { add_one(e.distorted(dist[0], dist[1]), maxImgWidth, loadAndStoreSegments); return; }
        // without coefficients: the two calls named after the image, which are that entry with dist left out
        const int n = (int)e.link_ids.size(), store = loadAndStoreSegments ? 1 : 0;
        report(e.fixed_sim ? l3d_line3d_add_image_pixels_fixed_sim(h_, imageID, e.pixels, e.width, e.height, e.channels, e.step, e.K, e.R, e.t, e.link_ids.data(), e.sims.data(), n,
                                                                   data_directory_.c_str(), maxImgWidth, store)
                           : l3d_line3d_add_image_pixels(h_, imageID, e.pixels, e.width, e.height, e.channels, e.step, e.K, e.R, e.t, e.link_ids.data(), n, data_directory_.c_str(),
                                                         maxImgWidth, store));
    }
    // `image` with a size only: the segment cache or nothing
    template <class Img, class M3, class V3, class Links>
    void add_from_image(detail::prio<0>, unsigned int imageID, const Img& image, const M3& K, const M3& R, const V3& t, const Links& links, const double*,
                        int maxImgWidth, bool loadAndStoreSegments)
    {
        ImageEntry e;
        flatten(K, R, t, e.K, e.R, e.t);
        set_links(e, links);
        const unsigned int w = image.cols > 0 ? (unsigned int)image.cols : 0u, h = image.rows > 0 ? (unsigned int)image.rows : 0u;
        const int n = (int)e.link_ids.size(), store = loadAndStoreSegments ? 1 : 0;
        report(e.fixed_sim ? l3d_line3d_add_image_fixed_sim_ex(h_, imageID, w, h, nullptr, 0, e.K, e.R, e.t, e.link_ids.data(), e.sims.data(), n, data_directory_.c_str(), maxImgWidth, store)
                           : l3d_line3d_add_image_ex(h_, imageID, w, h, nullptr, 0, e.K, e.R, e.t, e.link_ids.data(), n, data_directory_.c_str(), maxImgWidth, store));
    }
    static void set_links(ImageEntry& e, const std::list<unsigned int>& worldpointIDs) { e.link_ids.assign(worldpointIDs.begin(), worldpointIDs.end()); }
    static void set_links(ImageEntry& e, const std::map<unsigned int, float>& viewSimilarity)
    {
        for (auto& kv : viewSimilarity) { e.link_ids.push_back(kv.first); e.sims.push_back(kv.second); }
        e.sims.push_back(0.0f);       // (never null: `sims` tells the two kinds of links apart)
        e.fixed_sim = true;
    }
    void report(int rc) { if (rc != L3D_OK) std::cerr << prefix_ << l3d_line3d_last_error(h_) << std::endl; }
    l3d_line3d* h_;
    std::string prefix_, data_directory_;
    bool use_collinearity_;
};

}  // namespace L3D
