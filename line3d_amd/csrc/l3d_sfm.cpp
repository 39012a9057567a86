// l3d_sfm.cpp -- SfM front ends of the reference's two drivers without tclap / OpenCV / boost:
// the VisualSfM NVM reader of main_vsfm.cpp:121-223 and the bundler reader of main_bundler.cpp:110-204, reduced to what
// feeds Line3D::addImage: per camera focal length, rotation, translation, distortion coefficients and the list of
// world points it observes (the similarity source of findVisualNeighbors, line3D.cc:1874-1935).  The images
// themselves go through l3d_line3d_add_image_jpeg / l3d_line3d_add_image_pixels_distorted (decoding of baseline JPEG, undistortion and the detector:
// l3d_jpeg.cpp, l3d_jpeg_device.hip, l3d_detect.hip); a camera's K is built by the caller from the
// focal length and the image size the way the drivers do it (main_vsfm.cpp:232-241): [[f,0,w/2],[0,f,h/2],[0,0,1]].
//
// A third reader has no counterpart in the drivers: COLMAP models (cameras + images, text or binary; l3d_sfm_read_colmap), whose cameras carry a
// lens model of their own -- what the ..._lens calls take (l3d_sfm_camera_lens).
//
// Parsing follows the drivers' own token order, including what they skip (header lines, the separator line before the
// point count in NVM files, colours, feature positions).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/line3d_amd.h"

struct l3d_sfm_scene {
    int n_cams = 0, n_points = 0;
    bool nvm = false;                               // read from an NVM file: one coefficient, of the opposite sign (l3d_sfm_camera_cv_distortion)
    std::vector<double> focal, dist, R, t;          // n, 2n, 9n (row-major), 3n
    std::vector<std::string> names;                 // image file names (NVM) or "%08d" of the camera index (bundler: visualize/%08d.jpg by convention)
    std::vector<std::vector<uint32_t>> wps;         // per camera: world point ids in file order
    // a COLMAP model: per image the index of its camera in the tables below (the file's camera id in cam_id), -1 on the other kinds of scene
    bool colmap = false;
    std::vector<int> cam_of, cam_id;
    struct ColmapCamera { int model = -1; unsigned long long width = 0, height = 0; std::vector<double> params; };
    std::vector<ColmapCamera> colmap_cams;
    std::string err;
};

namespace {

int fail(l3d_sfm_scene* s, const std::string& m, l3d_sfm_scene** out)
{
    // the message survives in a scene object the caller can query and must free
    s->err = m;
    s->n_cams = 0;
    *out = s;
    return L3D_ERR_INVALID;
}

}  // namespace

// ---- COLMAP models.  The camera models by id, with the number of their parameters (their order: include/line3d_amd.h)
namespace {
struct ColmapModel { const char* name; int n; };
const ColmapModel kColmapModels[] = { { "SIMPLE_PINHOLE", 3 }, { "PINHOLE", 4 }, { "SIMPLE_RADIAL", 4 }, { "RADIAL", 5 }, { "OPENCV", 8 }, { "OPENCV_FISHEYE", 8 },
                                      { "FULL_OPENCV", 12 }, { "FOV", 5 }, { "SIMPLE_RADIAL_FISHEYE", 4 }, { "RADIAL_FISHEYE", 5 }, { "THIN_PRISM_FISHEYE", 12 } };
constexpr int kColmapModelCount = (int)(sizeof(kColmapModels) / sizeof(kColmapModels[0]));

// a whole file in memory, read with bounds: a truncated file ends in a message, never in a read past the end
struct Bytes {
    std::vector<unsigned char> b;
    size_t at = 0;
    bool load(const std::string& path)
    {
        FILE* f = fopen(path.c_str(), "rb");
        if (!f) return false;
        unsigned char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
        fclose(f);
        return true;
    }
    template <class T> bool get(T& v)
    {
        if (b.size() - at < sizeof(T)) return false;
        memcpy(&v, b.data() + at, sizeof(T));
        at += sizeof(T);
        return true;
    }
    bool skip(unsigned long long n, unsigned long long each)      // n records of `each` bytes
    {
        if (each && n > (b.size() - at) / each) return false;
        at += (size_t)(n * each);
        return true;
    }
};

bool file_exists(const std::string& p) { FILE* f = fopen(p.c_str(), "rb"); if (f) fclose(f); return f != nullptr; }

// one image of the model into the scene: the quaternion (w, x, y, z; normalised, as COLMAP does on reading) to R, t as it is
void colmap_push_image(l3d_sfm_scene* s, const double q[4], const double t[3], int cam, int cam_id, const std::string& name, std::vector<uint32_t>&& wps)
{
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double w = q[0] / nq, x = q[1] / nq, y = q[2] / nq, z = q[3] / nq;
    const double R[9] = { 1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w),
                          2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w),
                          2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y) };
    s->R.insert(s->R.end(), R, R + 9);
    s->t.insert(s->t.end(), t, t + 3);
    s->cam_of.push_back(cam); s->cam_id.push_back(cam_id);
    s->names.push_back(name);
    const l3d_sfm_scene::ColmapCamera& c = s->colmap_cams[(size_t)cam];
    // focal: f, or fx; dist: what l3d_sfm_camera_cv_distortion can answer (SIMPLE_RADIAL k, RADIAL k1 k2), else zero
    s->focal.push_back(c.params[0]);
    double d[2] = { 0.0, 0.0 };
    if (c.model == 2) d[0] = c.params[3];
    if (c.model == 3) { d[0] = c.params[3]; d[1] = c.params[4]; }
    s->dist.insert(s->dist.end(), d, d + 2);
    for (uint32_t id : wps) if ((long long)id + 1 > s->n_points) s->n_points = (int)std::min<long long>((long long)id + 1, 0x7fffffff);
    s->wps.push_back(std::move(wps));
}

int colmap_read_bin(l3d_sfm_scene* s, const std::string& dir, std::map<unsigned, int>& index, l3d_sfm_scene** out)
{
    Bytes c, im;
    if (!c.load(dir + "cameras.bin")) return fail(s, "COLMAP model: cannot read " + dir + "cameras.bin", out);
    if (!im.load(dir + "images.bin")) return fail(s, "COLMAP model: cannot read " + dir + "images.bin", out);
    uint64_t nc = 0;
    if (!c.get(nc) || nc > c.b.size() / 24) return fail(s, "COLMAP model: cameras.bin is truncated (camera count)", out);
    for (uint64_t k = 0; k < nc; ++k) {
        uint32_t id = 0; int32_t model = 0; uint64_t w = 0, h = 0;
        if (!c.get(id) || !c.get(model) || !c.get(w) || !c.get(h)) return fail(s, "COLMAP model: cameras.bin is truncated (camera " + std::to_string(k) + ")", out);
        if (model < 0 || model >= kColmapModelCount) return fail(s, "COLMAP model: camera " + std::to_string(id) + " has the unknown model id " + std::to_string(model), out);
        l3d_sfm_scene::ColmapCamera cam;
        cam.model = model; cam.width = w; cam.height = h;
        cam.params.assign((size_t)kColmapModels[model].n, 0.0);
        for (double& p : cam.params) if (!c.get(p)) return fail(s, "COLMAP model: cameras.bin is truncated (parameters of camera " + std::to_string(id) + ")", out);
        index[id] = (int)s->colmap_cams.size();
        s->colmap_cams.push_back(cam);
    }
    uint64_t ni = 0;
    if (!im.get(ni) || ni > im.b.size() / 64) return fail(s, "COLMAP model: images.bin is truncated (image count)", out);
    for (uint64_t k = 0; k < ni; ++k) {
        uint32_t id = 0, cam_id = 0;
        double q[4], t[3];
        bool ok = im.get(id);
        for (double& v : q) ok = ok && im.get(v);
        for (double& v : t) ok = ok && im.get(v);
        ok = ok && im.get(cam_id);
        std::string name;
        char ch = 1;
        while (ok && (ok = im.get(ch)) && ch) name.push_back(ch);
        uint64_t np = 0;
        ok = ok && im.get(np);
        if (!ok || np > (im.b.size() - im.at) / 24) return fail(s, "COLMAP model: images.bin is truncated (image " + std::to_string(k) + ")", out);
        std::vector<uint32_t> wps;
        for (uint64_t j = 0; j < np; ++j) {
            double x, y; uint64_t p3 = 0;
            im.get(x); im.get(y); im.get(p3);                       // (the count was held against the bytes that are left)
            if (p3 == ~(uint64_t)0) continue;
            if (p3 > 0xfffffffeull) return fail(s, "COLMAP model: image " + std::to_string(id) + " observes a point id beyond 32 bits", out);
            wps.push_back((uint32_t)p3);
        }
        const auto it = index.find(cam_id);
        if (it == index.end()) return fail(s, "COLMAP model: image " + std::to_string(id) + " names camera " + std::to_string(cam_id) + ", which cameras.bin does not have", out);
        colmap_push_image(s, q, t, it->second, (int)cam_id, name, std::move(wps));
    }
    return L3D_OK;
}

// the next line that is neither empty nor a comment
bool colmap_line(std::ifstream& f, std::string& line)
{
    while (std::getline(f, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        const size_t a = line.find_first_not_of(" \t");
        if (a != std::string::npos && line[a] != '#') return true;
    }
    return false;
}

int colmap_read_txt(l3d_sfm_scene* s, const std::string& dir, std::map<unsigned, int>& index, l3d_sfm_scene** out)
{
    std::ifstream c(dir + "cameras.txt"), im(dir + "images.txt");
    if (!c.is_open()) return fail(s, "COLMAP model: neither cameras.bin + images.bin nor cameras.txt in " + dir, out);
    if (!im.is_open()) return fail(s, "COLMAP model: cannot read " + dir + "images.txt", out);
    std::string line;
    while (colmap_line(c, line)) {
        std::stringstream ss(line);
        unsigned id = 0; std::string model; unsigned long long w = 0, h = 0;
        ss >> id >> model >> w >> h;
        int m = -1;
        for (int k = 0; k < kColmapModelCount; ++k) if (model == kColmapModels[k].name) m = k;
        if (!ss || m < 0) return fail(s, "COLMAP model: cameras.txt: camera " + std::to_string(id) + " has the unknown model '" + model + "'", out);
        l3d_sfm_scene::ColmapCamera cam;
        cam.model = m; cam.width = w; cam.height = h;
        cam.params.assign((size_t)kColmapModels[m].n, 0.0);
        for (double& p : cam.params) ss >> p;
        if (!ss) return fail(s, "COLMAP model: cameras.txt: camera " + std::to_string(id) + " (" + model + ") has too few parameters", out);
        index[id] = (int)s->colmap_cams.size();
        s->colmap_cams.push_back(cam);
    }
    while (colmap_line(im, line)) {
        std::stringstream ss(line);
        unsigned id = 0, cam_id = 0;
        double q[4], t[3];
        ss >> id >> q[0] >> q[1] >> q[2] >> q[3] >> t[0] >> t[1] >> t[2] >> cam_id;
        if (!ss) return fail(s, "COLMAP model: images.txt: a malformed image line: " + line, out);
        std::string name;
        std::getline(ss, name);                                     // the rest of the line: a name may contain spaces
        const size_t a = name.find_first_not_of(" \t"), b = name.find_last_not_of(" \t");
        name = a == std::string::npos ? std::string() : name.substr(a, b - a + 1);
        std::vector<uint32_t> wps;
        if (std::getline(im, line)) {                                // the observations: X Y POINT3D_ID ...; the line may be empty
            std::stringstream ps(line);
            double x, y; long long p3;
            while (ps >> x >> y >> p3) {
                if (p3 < 0) continue;
                if (p3 > 0xfffffffell) return fail(s, "COLMAP model: image " + std::to_string(id) + " observes a point id beyond 32 bits", out);
                wps.push_back((uint32_t)p3);
            }
        }
        const auto it = index.find(cam_id);
        if (it == index.end()) return fail(s, "COLMAP model: image " + std::to_string(id) + " names camera " + std::to_string(cam_id) + ", which cameras.txt does not have", out);
        colmap_push_image(s, q, t, it->second, (int)cam_id, name, std::move(wps));
    }
    return L3D_OK;
}
}  // namespace

extern "C" {

// main_vsfm.cpp:121-223
int l3d_sfm_read_nvm(const char* path, l3d_sfm_scene** out)
{
    if (!path || !out) return L3D_ERR_INVALID;
    l3d_sfm_scene* s = new l3d_sfm_scene();
    s->nvm = true;
    std::ifstream f(path);
    if (!f.is_open()) return fail(s, std::string("NVM file ") + path + " does not exist!", out);
    std::string line;
    std::getline(f, line);                                   // header ("NVM_V3 ...")
    std::getline(f, line);                                   // empty
    std::getline(f, line);
    {
        std::stringstream ss(line);
        unsigned int n = 0;
        ss >> n;
        if (n == 0) return fail(s, "No aligned cameras in NVM file!", out);
        s->n_cams = (int)n;
    }
    const size_t n = (size_t)s->n_cams;
    s->focal.assign(n, 0.0); s->dist.assign(2 * n, 0.0); s->R.assign(9 * n, 0.0); s->t.assign(3 * n, 0.0);
    s->names.assign(n, ""); s->wps.assign(n, {});
    for (size_t i = 0; i < n; ++i) {
        std::getline(f, line);
        std::stringstream ss(line);
        std::string name;
        double fl = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0, cx = 0, cy = 0, cz = 0, d = 0;
        ss >> name >> fl >> q3 >> q0 >> q1 >> q2;            // file order: w x y z
        ss >> cx >> cy >> cz >> d;
        s->names[i] = name;
        s->focal[i] = (double)(float)fl;                     // the driver keeps focal and distortion as float
        s->dist[2 * i] = (double)(float)d;
        double* R = &s->R[9 * i];
        R[0] = 1.0 - 2.0 * q1 * q1 - 2.0 * q2 * q2; R[1] = 2.0 * q0 * q1 - 2.0 * q2 * q3; R[2] = 2.0 * q0 * q2 + 2.0 * q1 * q3;
        R[3] = 2.0 * q0 * q1 + 2.0 * q2 * q3; R[4] = 1.0 - 2.0 * q0 * q0 - 2.0 * q2 * q2; R[5] = 2.0 * q1 * q2 - 2.0 * q0 * q3;
        R[6] = 2.0 * q0 * q2 - 2.0 * q1 * q3; R[7] = 2.0 * q1 * q2 + 2.0 * q0 * q3; R[8] = 1.0 - 2.0 * q0 * q0 - 2.0 * q1 * q1;
        double* t = &s->t[3 * i];                            // t = -R C, evaluated the way Eigen evaluates -R*C: (-R) * C
        for (int r = 0; r < 3; ++r) t[r] = (-R[3 * r]) * cx + (-R[3 * r + 1]) * cy + (-R[3 * r + 2]) * cz;
    }
    std::getline(f, line);                                   // separator
    std::getline(f, line);
    {
        std::stringstream ss(line);
        unsigned int np = 0;
        ss >> np;
        s->n_points = (int)np;
    }
    for (int i = 0; i < s->n_points; ++i) {
        if (!std::getline(f, line)) break;
        std::istringstream ss(line);
        double px, py, pz, cr, cg, cb;
        ss >> px >> py >> pz >> cr >> cg >> cb;
        unsigned int nv = 0;
        ss >> nv;
        for (unsigned int j = 0; j < nv; ++j) {
            unsigned int cam = 0, sift = 0;
            float x = 0, y = 0;
            ss >> cam >> sift >> x >> y;
            if (!ss) break;
            if (cam < (unsigned int)s->n_cams) s->wps[cam].push_back((uint32_t)i);
        }
    }
    *out = s;
    return L3D_OK;
}

// main_bundler.cpp:110-204 (bundle.rd.out)
int l3d_sfm_read_bundler(const char* path, l3d_sfm_scene** out)
{
    if (!path || !out) return L3D_ERR_INVALID;
    l3d_sfm_scene* s = new l3d_sfm_scene();
    std::ifstream f(path);
    if (!f.is_open()) return fail(s, std::string("bundle file ") + path + " does not exist!", out);
    std::string line;
    std::getline(f, line);                                   // "# Bundle file v0.3"
    std::getline(f, line);
    {
        std::stringstream ss(line);
        unsigned int nc = 0, np = 0;
        ss >> nc >> np;
        if (nc == 0 || np == 0) return fail(s, "No cameras and/or points in bundle file!", out);
        s->n_cams = (int)nc; s->n_points = (int)np;
    }
    const size_t n = (size_t)s->n_cams;
    s->focal.assign(n, 0.0); s->dist.assign(2 * n, 0.0); s->R.assign(9 * n, 0.0); s->t.assign(3 * n, 0.0);
    s->names.assign(n, ""); s->wps.assign(n, {});
    for (size_t i = 0; i < n; ++i) {
        double fl = 0, d1 = 0, d2 = 0;
        std::getline(f, line);
        { std::stringstream ss(line); ss >> fl >> d1 >> d2; }
        s->focal[i] = (double)(float)fl;
        s->dist[2 * i] = (double)(float)d1; s->dist[2 * i + 1] = (double)(float)d2;
        double* R = &s->R[9 * i];
        for (int r = 0; r < 3; ++r) {
            std::getline(f, line);
            std::stringstream ss(line);
            ss >> R[3 * r] >> R[3 * r + 1] >> R[3 * r + 2];
        }
        for (int k = 3; k < 9; ++k) R[k] *= -1.0;            // bundler looks down -z: flip the 2nd and 3rd row ...
        std::getline(f, line);
        double* t = &s->t[3 * i];
        { std::stringstream ss(line); ss >> t[0] >> t[1] >> t[2]; }
        t[1] *= -1.0; t[2] *= -1.0;                          // ... and y, z of the translation
        char nm[32];
        snprintf(nm, sizeof nm, "%08u", (unsigned)i);        // visualize/%08d.{jpg,png,...}, main_bundler.cpp:208-236
        s->names[i] = nm;
    }
    for (int i = 0; i < s->n_points; ++i) {
        std::getline(f, line);                               // position
        std::getline(f, line);                               // colour
        if (!std::getline(f, line)) break;                   // view list
        std::istringstream ss(line);
        unsigned int nv = 0;
        ss >> nv;
        for (unsigned int j = 0; j < nv; ++j) {
            unsigned int cam = 0, key = 0;
            float x = 0, y = 0;
            ss >> cam >> key >> x >> y;
            if (!ss) break;
            if (cam < (unsigned int)s->n_cams) s->wps[cam].push_back((uint32_t)i);
        }
    }
    *out = s;
    return L3D_OK;
}

int l3d_sfm_read_colmap(const char* model_dir, l3d_sfm_scene** out)
{
    if (!model_dir || !out) return L3D_ERR_INVALID;
    l3d_sfm_scene* s = new l3d_sfm_scene();
    s->colmap = true;
    std::string dir(model_dir);
    if (!dir.empty() && dir.back() != '/') dir += '/';
    std::map<unsigned, int> index;                                  // the file's camera id -> place in colmap_cams
    const bool bin = file_exists(dir + "cameras.bin") && file_exists(dir + "images.bin");
    if (const int rc = bin ? colmap_read_bin(s, dir, index, out) : colmap_read_txt(s, dir, index, out)) return rc;
    s->n_cams = (int)s->names.size();
    if (s->n_cams == 0) return fail(s, "COLMAP model: no images in " + dir, out);
    *out = s;
    return L3D_OK;
}

int l3d_sfm_camera_id(const l3d_sfm_scene* s, int i) { return (s && s->colmap && i >= 0 && i < s->n_cams) ? s->cam_id[(size_t)i] : -1; }

int l3d_sfm_camera_model(const l3d_sfm_scene* s, int i, const char** name, const double** params, int* n)
{
    if (!s || !s->colmap || i < 0 || i >= s->n_cams) return L3D_ERR_INVALID;
    const l3d_sfm_scene::ColmapCamera& c = s->colmap_cams[(size_t)s->cam_of[(size_t)i]];
    if (name) *name = kColmapModels[c.model].name;
    if (params) *params = c.params.data();
    if (n) *n = (int)c.params.size();
    return L3D_OK;
}

int l3d_sfm_camera_lens(l3d_sfm_scene* s, int i, l3d_lens* lens, double K[9], int* width, int* height)
{
    if (!s || i < 0 || i >= s->n_cams || !lens) return L3D_ERR_INVALID;
    *lens = l3d_lens{};
    lens->model = L3D_LENS_BROWN;
    if (K) for (int k = 0; k < 9; ++k) K[k] = 0.0;
    if (width) *width = 0;
    if (height) *height = 0;
    if (!s->colmap) return l3d_sfm_camera_cv_distortion(s, i, lens->k);     // (k[0], k[1]; a zero source camera: the output camera)
    const l3d_sfm_scene::ColmapCamera& c = s->colmap_cams[(size_t)s->cam_of[(size_t)i]];
    const double* p = c.params.data();
    const bool one_f = c.model == 0 || c.model == 2 || c.model == 3 || c.model == 8 || c.model == 9;      // f cx cy ...; else fx fy cx cy ...
    const double* k = p + (one_f ? 3 : 4);
    switch (c.model) {
    case 0: case 1: break;
    case 2: lens->k[0] = k[0]; break;
    case 3: lens->k[0] = k[0]; lens->k[1] = k[1]; break;
    case 4: for (int j = 0; j < 4; ++j) lens->k[j] = k[j]; break;
    case 6: for (int j = 0; j < 8; ++j) lens->k[j] = k[j]; break;
    case 5: lens->model = L3D_LENS_FISHEYE; for (int j = 0; j < 4; ++j) lens->k[j] = k[j]; break;
    case 8: lens->model = L3D_LENS_FISHEYE; lens->k[0] = k[0]; break;
    case 9: lens->model = L3D_LENS_FISHEYE; lens->k[0] = k[0]; lens->k[1] = k[1]; break;
    default:
        lens->model = 0;
        s->err = std::string("camera ") + std::to_string(i) + ": the COLMAP model " + kColmapModels[c.model].name + " has no lens in this library";
        return L3D_ERR_UNSUPPORTED;
    }
    // the pixel centre: COLMAP's (0.5, 0.5) is (0, 0) here
    lens->fx = p[0]; lens->fy = one_f ? p[0] : p[1];
    lens->cx = (one_f ? p[1] : p[2]) - 0.5; lens->cy = (one_f ? p[2] : p[3]) - 0.5;
    if (K) { K[0] = lens->fx; K[4] = lens->fy; K[2] = lens->cx; K[5] = lens->cy; K[8] = 1.0; }
    if (width) *width = (int)c.width;
    if (height) *height = (int)c.height;
    return L3D_OK;
}

void l3d_sfm_free(l3d_sfm_scene* s) { delete s; }
const char* l3d_sfm_last_error(const l3d_sfm_scene* s) { return s ? s->err.c_str() : "null scene"; }
int l3d_sfm_num_cameras(const l3d_sfm_scene* s) { return s ? s->n_cams : 0; }
int l3d_sfm_num_points(const l3d_sfm_scene* s) { return s ? s->n_points : 0; }

int l3d_sfm_camera(const l3d_sfm_scene* s, int i, double* focal, double dist[2], double R[9], double t[3], int* n_worldpoints)
{
    if (!s || i < 0 || i >= s->n_cams) return L3D_ERR_INVALID;
    if (focal) *focal = s->focal[(size_t)i];
    if (dist) { dist[0] = s->dist[2 * (size_t)i]; dist[1] = s->dist[2 * (size_t)i + 1]; }
    if (R) memcpy(R, &s->R[9 * (size_t)i], 72);
    if (t) memcpy(t, &s->t[3 * (size_t)i], 24);
    if (n_worldpoints) *n_worldpoints = (int)s->wps[(size_t)i].size();
    return L3D_OK;
}
// the coefficients the drivers hand to OpenCV: NVM -d, 0 (main_vsfm.cpp:259); bundler d1, d2 (main_bundler.cpp:273-274)
int l3d_sfm_camera_cv_distortion(const l3d_sfm_scene* s, int i, double k[2])
{
    if (!s || i < 0 || i >= s->n_cams || !k) return L3D_ERR_INVALID;
    if (s->colmap) {            // the pinhole and radial models with fx == fy; the others have no (k1, k2)
        const l3d_sfm_scene::ColmapCamera& c = s->colmap_cams[(size_t)s->cam_of[(size_t)i]];
        if (c.model > 3 || (c.model == 1 && c.params[0] != c.params[1])) return L3D_ERR_UNSUPPORTED;
    }
    const double d1 = s->dist[2 * (size_t)i], d2 = s->dist[2 * (size_t)i + 1];
    k[0] = s->nvm ? -d1 : d1;
    k[1] = s->nvm ? 0.0 : d2;
    return L3D_OK;
}
const char* l3d_sfm_camera_name(const l3d_sfm_scene* s, int i) { return (s && i >= 0 && i < s->n_cams) ? s->names[(size_t)i].c_str() : ""; }
int l3d_sfm_camera_worldpoints(const l3d_sfm_scene* s, int i, uint32_t* ids)
{
    if (!s || i < 0 || i >= s->n_cams || !ids) return L3D_ERR_INVALID;
    const std::vector<uint32_t>& w = s->wps[(size_t)i];
    if (!w.empty()) memcpy(ids, w.data(), w.size() * 4);
    return L3D_OK;
}

// The drivers' camera matrix (main_vsfm.cpp:232-241, main_bundler.cpp:243-252): principal point = image size / 2 in float
void l3d_sfm_intrinsics(double focal, unsigned int width, unsigned int height, double K[9])
{
    const float px = float(width) / 2.0f, py = float(height) / 2.0f, f = (float)focal;
    for (int k = 0; k < 9; ++k) K[k] = 0.0;
    K[0] = f; K[4] = f; K[2] = px; K[5] = py; K[8] = 1.0;
}

}  // extern "C"
