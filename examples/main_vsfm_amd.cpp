// main_vsfm_amd.cpp -- the flow of the reference's VisualSfM driver (main_vsfm.cpp:34-329) over this library, with the
// segment caches of an earlier Line3D run standing in for the images, or with the images as binary PPM / PGM files or baseline JPEG files (no
// OpenCV, no tclap, no boost):
//
//   main_vsfm_amd [--merge] [--refine] [--support] [--junctions [--snap]] [--obj <file>] [--planes [--planes-obj <file>]] [--device-covisibility] [--overlays <folder>] <scene.nvm | bundle.rd.out> <data directory> [neighbors=10] [diffusion=0] [output folder=<data directory>] [image folder]
//
// --merge (anywhere on the line): the near-copies of a 3-D line -- an edge seen along a camera path longer than the matching neighbourhood comes out
// several times -- are merged on the GPU before the result is refined and written (setMerging, defaults; the counts are printed).
// --refine (anywhere on the line): the 3-D lines are refined against the 2-D segments of their clusters before they are written (setRefinement: the
// reference has no such step; its successor Line3D++ added one) -- the segments of a line in the STL / TXT files are then collinear.
// --support (anywhere on the line): as the last step of compute3Dmodel every line's 2-D segments are extended by the segments of ALL views that lie on
// its projection (setSupport, defaults: 3 px, 5 degrees, half the shorter segment) -- a line otherwise lists only the views its cluster reached through
// matches between neighbouring views; the TXT file and the overlays then show the added observations (the counts are printed).
// --junctions (anywhere on the line): after the merging and the refinement the places where lines meet are found on the GPU -- line ends grouped into
// vertices, free ends that rest on the inside of another line (setJunctions, defaults: 4 px, 12 px, 10 degrees, a quarter of the length; the counts are
// printed); with --snap those ends are moved there along their own axes.  --obj <file>: the result is also written as a Wavefront OBJ wireframe whose
// lines share the vertices' indices (save3DLinesAsOBJ; without --junctions no index is shared).
// --planes (anywhere on the line): after the junctions the lines that lie in one plane are found on the GPU -- every pair of lines that meet spans a
// hypothesis, agreeing hypotheses are averaged into a plane (setPlanes, defaults: 4 px, 10 degrees, 3 lines; a summary is printed).  --planes-obj <file>:
// the planes are also written as a Wavefront OBJ, one rectangle per plane (save3DPlanesAsOBJ).
// --device-covisibility (anywhere on the line): the cameras' world point lists are counted on the GPU when compute3Dmodel starts, instead of one
// observation at a time as the images are added (setDeviceCovisibility: the same neighbours, the same lines; it pays on models of many images).
// --overlays <folder> (anywhere on the line): after compute3Dmodel every view's image -- loaded once more and undistorted as it was added; a grey canvas
// of the view's size when the segment caches stood in for the images -- is written with the view's overlay (overlayView: its 2-D segments that belong to
// a line, and the projected 3-D lines it observes, coloured by line) as "<folder>/overlay_<camera>.ppm" (binary P6; the folder has to exist).
// With an image folder, camera i's image is "<image folder>/<camera name, extension replaced>.ppm" or ".pgm" (binary P6 / P5, maxval 255), or the
// camera's own file "<image folder>/<camera name>" when it ends in .jpg / .jpeg (baseline JPEG, decoded on the device: addImageJPEGDistorted;
// convert PNG and progressive JPEG beforehand).  The camera name is the NVM file's image name; for a bundler file it is the camera index as %08d
// ("00000000.ppm", ...: the drivers' visualize/%08d.jpg, main_bundler.cpp:208-236): it is undistorted with the scene file's coefficients and its segments are detected on the device
// (addImageDistorted: main_vsfm.cpp:243-273), and the data directory receives the segment caches.  Without one:
// For every camera of the NVM file the data directory ("<image folder>/L3D_data" of the reference, main_vsfm.cpp:108-116)
// must hold "segments_<id>_<w>x<h>_coll1.bin" (line3D.cc:143-150) -- the image size is read off the file name, K is built
// from the focal length and that size the way the driver does it (main_vsfm.cpp:232-241), addImage uses the cached segments
// and collinearities (line3D.cc:160-168), compute3Dmodel runs on the GPU, the result goes to
// "<output folder>/line3D_result__W_..." as STL and TXT (main_vsfm.cpp:289-325).
//
// Build:  g++ -std=c++17 -Iinclude examples/main_vsfm_amd.cpp -Lline3d_amd -lline3d_amd -Wl,-rpath,$PWD/line3d_amd -o main_vsfm_amd
#include <dirent.h>

#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "line3D_amd.hpp"

namespace {

// "segments_<id>_<w>x<h>_coll1.bin" of camera `id` in `dir`: the image size from the name
bool find_cache(const std::string& dir, unsigned id, unsigned& w, unsigned& h)
{
    DIR* d = opendir(dir.c_str());
    if (!d) return false;
    bool found = false;
    while (dirent* e = readdir(d)) {
        unsigned fid = 0, fw = 0, fh = 0, coll = 0;
        char tail[8] = { 0 };
        if (sscanf(e->d_name, "segments_%u_%ux%u_coll%u.%3s", &fid, &fw, &fh, &coll, tail) == 5 && fid == id && coll == 1 && strcmp(tail, "bin") == 0) {
            w = fw; h = fh; found = true;
            break;
        }
    }
    closedir(d);
    return found;
}

// a binary PGM / PPM image: what addImageDistorted needs of a cv::Mat
struct PnmImage {
    int cols = 0, rows = 0, ch = 1;
    size_t step = 0;
    unsigned char* data = nullptr;
    std::vector<unsigned char> store;
    int channels() const { return ch; }
};
// the next header number, past white space and '#' comments.  The character after the number is consumed (the header's single white space before
// the pixels); where it is a '#' ("640#c"), so is the comment it begins
bool pnm_number(FILE* f, int& v)
{
    int c = fgetc(f);
    while (c == '#' || c == ' ' || c == '\t' || c == '\n' || c == '\r') {
        if (c == '#') while (c != '\n' && c != EOF) c = fgetc(f);
        else c = fgetc(f);
    }
    if (c < '0' || c > '9') return false;
    long long n = 0;
    for (; c >= '0' && c <= '9' && n < (1ll << 31); c = fgetc(f)) n = n * 10 + (c - '0');      // (c: the single white space after the number)
    if (c == '#') while (c != '\n' && c != EOF) c = fgetc(f);
    v = (int)n;
    return n < (1ll << 31);
}
bool read_pnm(const std::string& path, PnmImage& img)
{
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    int w = 0, h = 0, maxval = 0;
    const int m0 = fgetc(f), m1 = fgetc(f);
    bool ok = m0 == 'P' && (m1 == '5' || m1 == '6') && pnm_number(f, w) && pnm_number(f, h) && pnm_number(f, maxval) && maxval == 255 && w > 0 && h > 0;
    if (ok) {
        img.cols = w; img.rows = h; img.ch = m1 == '6' ? 3 : 1;
        img.step = (size_t)w * img.ch;
        img.store.resize(img.step * h);
        ok = fread(img.store.data(), 1, img.store.size(), f) == img.store.size();
        img.data = img.store.data();
    }
    fclose(f);
    return ok;
}
// "<folder>/<name without its extension>.ppm", then ".pgm"
bool load_camera_image(const std::string& folder, const std::string& name, PnmImage& img)
{
    const size_t slash = name.find_last_of("/\\"), dot = name.find_last_of('.');
    const std::string stem = folder + "/" + (dot != std::string::npos && (slash == std::string::npos || dot > slash) ? name.substr(0, dot) : name);
    return read_pnm(stem + ".ppm", img) || read_pnm(stem + ".pgm", img);
}
// "<folder>/<name>" itself when the name ends in .jpg / .jpeg (any case): the file's bytes
bool load_camera_jpeg(const std::string& folder, const std::string& name, std::vector<unsigned char>& bytes)
{
    const size_t dot = name.find_last_of('.');
    if (dot == std::string::npos) return false;
    std::string ext = name.substr(dot + 1);
    for (char& c : ext) c = (char)tolower((unsigned char)c);
    if (ext != "jpg" && ext != "jpeg") return false;
    FILE* f = fopen((folder + "/" + name).c_str(), "rb");
    if (!f) return false;
    bytes.clear();
    unsigned char buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof(buf), f)) > 0;) bytes.insert(bytes.end(), buf, buf + got);
    fclose(f);
    return !bytes.empty();
}
// an image as three channels (a grey one repeated), written as a binary P6 file
void to_three_channels(PnmImage& img)
{
    if (img.ch == 3) return;
    std::vector<unsigned char> rgb((size_t)img.cols * img.rows * 3);
    for (int i = 0; i < img.rows; ++i)
        for (int j = 0; j < img.cols; ++j)
            for (int c = 0; c < 3; ++c) rgb[((size_t)i * img.cols + j) * 3 + c] = img.data[(size_t)i * img.step + (size_t)j * img.ch];
    img.store.swap(rgb); img.data = img.store.data(); img.ch = 3; img.step = (size_t)img.cols * 3;
}
bool write_ppm(const std::string& path, const PnmImage& img)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f) return false;
    fprintf(f, "P6\n%d %d\n255\n", img.cols, img.rows);
    bool ok = true;
    for (int i = 0; i < img.rows && ok; ++i) ok = fwrite(img.data + (size_t)i * img.step, 1, (size_t)img.cols * 3, f) == (size_t)img.cols * 3;
    return fclose(f) == 0 && ok;
}
// what --overlays needs of a camera once the model is there
struct OverlayJob { unsigned id; int w, h; double K[9], k[2]; std::string name; };

// K, R, t of the facade's matrix-typed calls over plain arrays
struct Mat3 { const double* p; double operator()(int i, int j) const { return p[i * 3 + j]; } };
struct Vec3 { const double* p; double operator()(int i) const { return p[i]; } };

}  // namespace

int main(int argc, char** argv)
{
    bool refine = false, device_covis = false, merge = false, support = false, junctions = false, snap = false, planes = false;
    std::string overlay_dir, obj_file, planes_obj_file;
    {
        int k = 1;
        for (int i = 1; i < argc; ++i) {
            if (std::string(argv[i]) == "--refine") refine = true;
            else if (std::string(argv[i]) == "--merge") merge = true;
            else if (std::string(argv[i]) == "--support") support = true;
            else if (std::string(argv[i]) == "--junctions") junctions = true;
            else if (std::string(argv[i]) == "--snap") snap = true;
            else if (std::string(argv[i]) == "--obj" && i + 1 < argc) obj_file = argv[++i];
            else if (std::string(argv[i]) == "--planes") planes = true;
            else if (std::string(argv[i]) == "--planes-obj" && i + 1 < argc) planes_obj_file = argv[++i];
            else if (std::string(argv[i]) == "--device-covisibility") device_covis = true;
            else if (std::string(argv[i]) == "--overlays" && i + 1 < argc) overlay_dir = argv[++i];
            else argv[k++] = argv[i];
        }
        argc = k;
    }
    if (argc < 3) { fprintf(stderr, "usage: %s [--merge] [--refine] [--support] [--junctions [--snap]] [--obj <file>] [--planes [--planes-obj <file>]] [--device-covisibility] [--overlays <folder>] <scene.nvm | bundle.rd.out> <data directory> [neighbors=10] [diffusion=0] [output folder] [image folder]\n", argv[0]); return 2; }
    const std::string nvm = argv[1], data_dir = argv[2];
    const int neighbors = argc > 3 ? atoi(argv[3]) : 10;
    const bool diffusion = argc > 4 && atoi(argv[4]) != 0;
    const std::string out_dir = argc > 5 ? argv[5] : data_dir;
    const std::string image_dir = argc > 6 ? argv[6] : "";

    l3d_sfm_scene* scene = nullptr;
    // a bundler file (bundle.rd.out, main_bundler.cpp:110-204) is read just as well: the rest of the two drivers is the same flow
    const bool is_nvm = nvm.size() >= 4 && nvm.compare(nvm.size() - 4, 4, ".nvm") == 0;
    if ((is_nvm ? l3d_sfm_read_nvm(nvm.c_str(), &scene) : l3d_sfm_read_bundler(nvm.c_str(), &scene)) != L3D_OK) {
        fprintf(stderr, "%s\n", l3d_sfm_last_error(scene));
        l3d_sfm_free(scene);
        return 1;
    }
    const int n = l3d_sfm_num_cameras(scene);
    // Line3D(data_directory, matchingNeighbors, ...) with the driver's defaults (main_vsfm.cpp:60-99)
    L3D::Line3D line3D(data_dir, neighbors, 5.0f, 1.0f, 3.5f, 10.0f, 0.25f, true, true);
    if (!line3D.valid()) { l3d_sfm_free(scene); return 1; }
    if (merge) line3D.setMerging(true);
    if (refine) line3D.setRefinement(true);
    if (support) line3D.setSupport(true);
    if (junctions) { L3D::JunctionParams jp; jp.snap = snap; line3D.setJunctions(true, jp); }
    if (planes) line3D.setPlanes(true);
    if (device_covis) line3D.setDeviceCovisibility(true);
    int added = 0;
    std::vector<OverlayJob> jobs;
    auto note = [&](unsigned id, int w, int h, const double* K, const double* k, const char* name) {
        OverlayJob j; j.id = id; j.w = w; j.h = h; memcpy(j.K, K, sizeof(j.K)); j.k[0] = k[0]; j.k[1] = k[1]; j.name = name ? name : "";
        jobs.push_back(j);
    };
    for (int i = 0; i < n; ++i) {
        double focal = 0, dist[2] = { 0, 0 }, R[9], t[3];
        int nwp = 0;
        l3d_sfm_camera(scene, i, &focal, dist, R, t, &nwp);
        std::vector<uint32_t> ids((size_t)nwp);
        l3d_sfm_camera_worldpoints(scene, i, ids.data());
        std::list<unsigned int> wps(ids.begin(), ids.end());
        if (!image_dir.empty()) {                   // main_vsfm.cpp:229-273: load, K from the image size, undistort, addImage
            PnmImage img;
            double K[9], k[2] = { 0, 0 };
            if (!load_camera_image(image_dir, l3d_sfm_camera_name(scene, i), img)) {
                std::vector<unsigned char> file;
                unsigned jw = 0, jh = 0, jch = 0;
                if (!load_camera_jpeg(image_dir, l3d_sfm_camera_name(scene, i), file)) { fprintf(stderr, "camera %d: no binary .ppm / .pgm image (maxval 255) and no .jpg / .jpeg file for %s in %s\n", i, l3d_sfm_camera_name(scene, i), image_dir.c_str()); continue; }
                if (!L3D::Line3D::jpegSize(file.data(), file.size(), jw, jh, jch)) { fprintf(stderr, "camera %d: %s\n", i, l3d_jpeg_last_error()); continue; }
                l3d_sfm_intrinsics(focal, jw, jh, K);
                l3d_sfm_camera_cv_distortion(scene, i, k);
                const unsigned before = line3D.numCameras();
                line3D.addImageJPEGDistorted((unsigned)i, file.data(), file.size(), Mat3{ K }, Mat3{ R }, Vec3{ t }, k[0], k[1], wps);
                if (line3D.numCameras() > before) note((unsigned)i, (int)jw, (int)jh, K, k, l3d_sfm_camera_name(scene, i));
                added += (int)(line3D.numCameras() - before);
                continue;
            }
            l3d_sfm_intrinsics(focal, (unsigned)img.cols, (unsigned)img.rows, K);
            l3d_sfm_camera_cv_distortion(scene, i, k);
            const unsigned before = line3D.numCameras();
            line3D.addImageDistorted((unsigned)i, img, Mat3{ K }, Mat3{ R }, Vec3{ t }, k[0], k[1], wps);
            if (line3D.numCameras() > before) note((unsigned)i, img.cols, img.rows, K, k, l3d_sfm_camera_name(scene, i));
            added += (int)(line3D.numCameras() - before);
            continue;
        }
        if (dist[0] != 0.0 || dist[1] != 0.0) { fprintf(stderr, "camera %d has lens distortion: the cached segments must come from undistorted images (or give an image folder)\n", i); continue; }
        unsigned w = 0, h = 0;
        if (!find_cache(data_dir, (unsigned)i, w, h)) { fprintf(stderr, "camera %d: no segment cache in %s\n", i, data_dir.c_str()); continue; }
        double K[9];
        l3d_sfm_intrinsics(focal, w, h, K);
        if (line3D.addImageFromCache((unsigned)i, w, h, K, R, t, wps)) { ++added; const double k0[2] = { 0, 0 }; note((unsigned)i, (int)w, (int)h, K, k0, nullptr); }
    }
    l3d_sfm_free(scene);
    fprintf(stderr, "[L3D] %d of %d cameras added\n", added, n);
    line3D.compute3Dmodel(diffusion);
    std::list<L3D::L3DFinalLine3D> result;
    line3D.getResult(result);
    fprintf(stderr, "[L3D] %zu 3-D lines\n", result.size());
    L3D::MergeStats ms;
    if (merge && line3D.getMerging(ms))
        fprintf(stderr, "[L3D] merging: %d -> %d lines in %d rounds (%d pairs in the first, %d groups merged, %d lines released)\n", ms.linesBefore, ms.linesAfter,
                ms.rounds, ms.pairsFirstRound, ms.groupsMerged, ms.linesReleased);
    L3D::SupportStats ss;
    if (support && line3D.getSupport(ss)) {
        long long before = 0, added_members = 0;
        for (size_t k = 0; k < ss.membersBefore.size(); ++k) { before += ss.membersBefore[k]; added_members += ss.membersAdded[k]; }
        fprintf(stderr, "[L3D] support: %lld observations of the lines in all views, %lld of %lld members found again, %lld 2-D segments added to the lines\n", ss.records,
                ss.membersFound, before, added_members);
    }
    L3D::JunctionStats js;
    if (junctions && line3D.getJunctions(js))
        fprintf(stderr, "[L3D] junctions: %zu vertices from %d corner pairs, %d line ends rest on another line, %d ends moved\n", js.vertices.size(), js.lRecords,
                js.nodesAttached, js.endsMoved);
    if (!obj_file.empty() && !line3D.save3DLinesAsOBJ(obj_file)) fprintf(stderr, "[L3D] %s could not be written\n", obj_file.c_str());
    L3D::PlaneStats ps;
    if (planes && line3D.getPlanes(ps))
        fprintf(stderr, "[L3D] planes: %zu planes from %d seed pairs in %d groups, %d member lines in all, %d pairs released\n", ps.planes.size(), ps.eligibleHypotheses,
                ps.components, ps.memberRecords, ps.hypothesesReleased);
    if (planes && !planes_obj_file.empty() && !line3D.save3DPlanesAsOBJ(planes_obj_file)) fprintf(stderr, "[L3D] %s could not be written\n", planes_obj_file.c_str());

    // the driver's output name (main_vsfm.cpp:289-313), numbers in stream-default formatting
    std::stringstream name;
    name << out_dir << "/line3D_result__W_" << -1 << "__";
    if (neighbors < 0) name << "N_ALL__"; else name << "N_" << neighbors << "__";
    name << "tL_" << 1.0f << "__tU_" << 5.0f << "__sigmaP_" << 3.5f << "__sigmaA_" << 10.0f << "__COLLIN__" << (diffusion ? "DIFFUSION" : "NO_DIFFUSION");
    line3D.save3DLinesAsSTL(result, name.str() + ".stl");                       // line3D.h:88-91
    line3D.save3DLinesAsTXT(result, name.str() + ".txt");

    // --overlays: one viewable PPM per view
    if (!overlay_dir.empty()) {
        int written = 0;
        for (const OverlayJob& j : jobs) {
            PnmImage img;
            bool have = false;
            if (!image_dir.empty() && !j.name.empty()) {
                have = load_camera_image(image_dir, j.name, img);
                if (!have) {
                    std::vector<unsigned char> file;
                    unsigned jw = 0, jh = 0, jch = 0;
                    if (load_camera_jpeg(image_dir, j.name, file) && line3D.decodeJPEG(file.data(), file.size(), img.store, jw, jh, jch)) {
                        img.cols = (int)jw; img.rows = (int)jh; img.ch = (int)jch; img.step = (size_t)jw * jch; img.data = img.store.data();
                        have = true;
                    }
                }
                if (have && (j.k[0] != 0.0 || j.k[1] != 0.0)) have = line3D.undistortImage(img, Mat3{ j.K }, j.k[0], j.k[1]);
            }
            if (!have || img.cols != j.w || img.rows != j.h) {          // no image: a grey canvas of the view's size
                img.cols = j.w; img.rows = j.h; img.ch = 3; img.step = (size_t)j.w * 3;
                img.store.assign(img.step * (size_t)j.h, 128); img.data = img.store.data();
            }
            to_three_channels(img);
            if (line3D.overlayView(j.id, img, L3D::OverlayStyle()) && write_ppm(overlay_dir + "/overlay_" + std::to_string(j.id) + ".ppm", img)) ++written;
        }
        fprintf(stderr, "[L3D] %d overlays written to %s\n", written, overlay_dir.c_str());
    }
    return result.empty() ? 3 : 0;
}
