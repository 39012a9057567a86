// l3d_refine.hip -- the refinement of l3d_refine.hpp on the device: one wave per cluster, four waves per workgroup (the launch shape of
// k_fit_clusters).  Lanes stride over the members; the 18 sums of an evaluation are reduced by the xor tree of the header, so every lane
// holds the same bits and the 4x4 solve and the accept / reject decision are wave-uniform -- computed redundantly by every lane, no
// atomics anywhere.  The host entry point l3d_test_refine_host runs the header's functions with the host's wave.
#include "l3d_ctx.hpp"
#include "l3d_refine.hpp"

using namespace l3d;

namespace l3d {

struct RefineArgs {
    int n_groups;
    const int* group_start;             // n_groups + 1 (members)
    const int* member_cam;              // 1 per member
    const float* member_seg;            // 4 per member
    const double* member_pts;           // 6 per member
    const refine::Cam* cams;
    int max_iterations; double huber;
    double* t; int* order;              // 2 per member          (global scratch: clusters above kRefineLds members)
    unsigned char* line_open; unsigned* cam_ids; unsigned* cam_cnt;   // 1 per member
    double* line; double* rms_before; double* rms_after; int* iterations; int* status;   // per group
    double* out;                        // 6 doubles per emitted segment, at most one per member
    int* out_cnt;                       // per group
};

constexpr int kRefineLds = 128;         // members of a cluster whose points, keys and sweep state fit the per-wave LDS arrays

struct DevWave {
    int lane;
    template <int N, class F> __device__ void sum(double* o, F f)
    {
#pragma unroll
        for (int k = 0; k < N; ++k) o[k] = 0.0;
        f(lane, o);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) o[k] = o[k] + __shfl_xor(o[k], off);
        }
    }
    template <class F> __device__ void lanes(F f) { f(lane); }
    template <class F> __device__ void first(F f) { if (lane == 0) f(); }
    __device__ void sync() { __threadfence_block(); }
};

__global__ __launch_bounds__(256) void k_refine_lines(RefineArgs a)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (g >= a.n_groups) return;
    const int m0 = a.group_start[g], members = a.group_start[g + 1] - m0, n2 = 2 * members;
    __shared__ double s_pts[4][2 * kRefineLds][3];
    __shared__ double s_t[4][2 * kRefineLds];
    __shared__ int s_order[4][2 * kRefineLds];
    __shared__ int s_cam[4][kRefineLds];
    __shared__ unsigned s_cid[4][kRefineLds], s_ccnt[4][kRefineLds];
    __shared__ unsigned char s_open[4][kRefineLds];
    const bool small = members <= kRefineLds;
    const double* gp = a.member_pts + 6 * (size_t)m0;
    if (small) {
        for (int i = lane; i < n2; i += 64) { s_pts[wv][i][0] = gp[3 * (size_t)i]; s_pts[wv][i][1] = gp[3 * (size_t)i + 1]; s_pts[wv][i][2] = gp[3 * (size_t)i + 2]; }
        for (int i = lane; i < members; i += 64) s_cam[wv][i] = a.member_cam[m0 + i];
    }
    __threadfence_block();
    refine::Group G;
    G.n = members;
    G.cam = small ? s_cam[wv] : a.member_cam + m0;
    G.seg = a.member_seg + 4 * (size_t)m0; G.pts = gp;
    G.t = small ? s_t[wv] : a.t + 2 * (size_t)m0;
    G.order = small ? s_order[wv] : a.order + 2 * (size_t)m0;
    G.open = small ? s_open[wv] : a.line_open + m0;
    G.cid = small ? s_cid[wv] : a.cam_ids + m0;
    G.ccnt = small ? s_ccnt[wv] : a.cam_cnt + m0;
    G.line = a.line + 6 * (size_t)g; G.rms_before = a.rms_before + g; G.rms_after = a.rms_after + g; G.iterations = a.iterations + g; G.status = a.status + g;
    G.out = a.out + 6 * (size_t)m0; G.out_cnt = a.out_cnt + g;
    auto get = [&](int i) { return small ? la::V3{ s_pts[wv][i][0], s_pts[wv][i][1], s_pts[wv][i][2] } : la::V3{ gp[3 * (size_t)i], gp[3 * (size_t)i + 1], gp[3 * (size_t)i + 2] }; };
    DevWave w{ lane };
    refine::refine_group(w, G, get, a.cams, a.max_iterations, a.huber);
}

}  // namespace l3d

namespace {

thread_local std::string t_refine_err;

struct RefineIn {
    const int32_t* group_start; int n_groups; const int32_t* member_cam; const float* member_seg; const double* member_pts; const double* cameras; int n_cameras;
    int max_iterations; double huber;
};

// everything that is refused, before anything is launched; msg: why
int refine_validate(const int32_t* group_start, int n_groups, const int32_t* member_cam, const float* member_seg, const double* member_pts, const double* cameras, int n_cameras,
                    const l3d_refine_params* prm, double* line, double* rms_before, double* rms_after, int32_t* iterations, int32_t* status, int32_t** seg_count, double** segs,
                    int* n_segs, RefineIn& in, std::string& msg)
{
    if (!seg_count || !segs || !n_segs || n_groups < 0 || n_cameras < 0) { msg = "bad argument"; return L3D_ERR_INVALID; }
    *seg_count = nullptr; *segs = nullptr; *n_segs = 0;
    in.max_iterations = prm ? prm->max_iterations : 20;
    in.huber = prm ? prm->huber_px : 2.0;
    if (in.max_iterations < 0) { msg = "refine: max_iterations must not be negative"; return L3D_ERR_INVALID; }
    if (!(in.huber >= 0.0) || !refine::fin(in.huber)) { msg = "refine: huber_px must be a finite number >= 0"; return L3D_ERR_INVALID; }
    if (n_groups == 0) { in.n_groups = 0; return L3D_OK; }
    if (!group_start || !line || !rms_before || !rms_after || !iterations || !status) { msg = "bad argument"; return L3D_ERR_INVALID; }
    if (group_start[0] != 0) { msg = "refine: group table must start at 0"; return L3D_ERR_INVALID; }
    for (int g = 0; g < n_groups; ++g) if (group_start[g + 1] < group_start[g]) { msg = "refine: group table must ascend"; return L3D_ERR_INVALID; }
    const int nm = group_start[n_groups];
    if (nm > 0 && (!member_cam || !member_seg || !member_pts || !cameras)) { msg = "bad argument"; return L3D_ERR_INVALID; }
    for (int i = 0; i < nm; ++i) if (member_cam[i] < 0 || member_cam[i] >= n_cameras) { msg = "refine: camera index outside the table"; return L3D_ERR_INVALID; }
    for (size_t i = 0; i < (size_t)n_cameras * 12; ++i) if (!refine::fin(cameras[i])) { msg = "refine: camera matrix is not finite"; return L3D_ERR_INVALID; }
    in.group_start = group_start; in.n_groups = n_groups; in.member_cam = member_cam; in.member_seg = member_seg; in.member_pts = member_pts; in.cameras = cameras;
    in.n_cameras = n_cameras;
    return L3D_OK;
}

// the per-group segments (6 doubles each at 6 * group_start[g]) packed back to back into callee-allocated outputs
int refine_pack(const int32_t* group_start, int n_groups, const int32_t* cnt_in, const double* out, int32_t** seg_count, double** segs, int* n_segs)
{
    size_t total = 0;
    for (int g = 0; g < n_groups; ++g) total += (size_t)cnt_in[g];
    int32_t* cnt = static_cast<int32_t*>(malloc(((size_t)n_groups + 1) * 4));
    double* packed = static_cast<double*>(malloc((total * 6 + 1) * 8));
    if (!cnt || !packed) { free(cnt); free(packed); return L3D_ERR_NOMEM; }
    size_t at = 0;
    for (int g = 0; g < n_groups; ++g) {
        cnt[g] = cnt_in[g];
        if (cnt_in[g]) memcpy(packed + 6 * at, out + 6 * (size_t)group_start[g], (size_t)cnt_in[g] * 48);
        at += (size_t)cnt_in[g];
    }
    *seg_count = cnt; *segs = packed; *n_segs = (int)total;
    return L3D_OK;
}

}  // namespace

extern "C" const char* l3d_refine_last_error(void) { return t_refine_err.c_str(); }

// the header's functions on the host: needs no device
extern "C" int l3d_test_refine_host(const int32_t* group_start, int n_groups, const int32_t* member_cam, const float* member_seg, const double* member_pts, const double* cameras,
                                    int n_cameras, const l3d_refine_params* prm, double* line, double* rms_before, double* rms_after, int32_t* iterations, int32_t* status,
                                    int32_t** seg_count, double** segs, int* n_segs)
{
    RefineIn in{};
    std::string msg;
    const int rv = refine_validate(group_start, n_groups, member_cam, member_seg, member_pts, cameras, n_cameras, prm, line, rms_before, rms_after, iterations, status, seg_count, segs,
                                   n_segs, in, msg);
    if (rv) { t_refine_err = msg; return rv; }
    if (n_groups == 0) return L3D_OK;
    const size_t nm = (size_t)group_start[n_groups];
    std::vector<refine::Cam> cams((size_t)n_cameras + 1);
    for (int c = 0; c < n_cameras; ++c) refine::make_cam(cameras + 12 * (size_t)c, cams[(size_t)c]);
    std::vector<double> t(2 * nm + 1), out(6 * nm + 1);
    std::vector<int> order(2 * nm + 1), cnt((size_t)n_groups + 1, 0);
    std::vector<unsigned char> open(nm + 1);
    std::vector<unsigned> cid(nm + 1), ccnt(nm + 1);
    for (int g = 0; g < n_groups; ++g) {
        const size_t m0 = (size_t)group_start[g];
        refine::Group G;
        G.n = group_start[g + 1] - group_start[g];
        G.cam = member_cam + m0; G.seg = member_seg + 4 * m0; G.pts = member_pts + 6 * m0;
        G.t = t.data() + 2 * m0; G.order = order.data() + 2 * m0; G.open = open.data() + m0; G.cid = cid.data() + m0; G.ccnt = ccnt.data() + m0;
        G.line = line + 6 * (size_t)g; G.rms_before = rms_before + g; G.rms_after = rms_after + g; G.iterations = iterations + g; G.status = status + g;
        G.out = out.data() + 6 * m0; G.out_cnt = cnt.data() + g;
        const double* gp = G.pts;
        auto get = [gp](int i) { return la::V3{ gp[3 * (size_t)i], gp[3 * (size_t)i + 1], gp[3 * (size_t)i + 2] }; };
        refine::HostWave w;
        refine::refine_group(w, G, get, cams.data(), in.max_iterations, in.huber);
    }
    const int rp = refine_pack(group_start, n_groups, cnt.data(), out.data(), seg_count, segs, n_segs);
    if (rp) t_refine_err = "malloc";
    return rp;
}

// Clusters as group_start (n_groups + 1) into the member tables; cameras: n_cameras 3x4 matrices.  Minv and C of every camera are computed on the
// host here, at entry (at most a few thousand cameras), and uploaded with the matrices.  Out: per group line (A, d), rms before / after, iterations,
// status; callee-allocated (l3d_free) seg_count and segs as l3d_fit_clusters.
extern "C" int l3d_refine_lines(l3d_ctx* c, const int32_t* group_start, int n_groups, const int32_t* member_cam, const float* member_seg, const double* member_pts,
                                const double* cameras, int n_cameras, const l3d_refine_params* prm, double* line, double* rms_before, double* rms_after, int32_t* iterations,
                                int32_t* status, int32_t** seg_count, double** segs, int* n_segs)
{
    if (!c) return L3D_ERR_INVALID;
    RefineIn in{};
    std::string msg;
    const int rv = refine_validate(group_start, n_groups, member_cam, member_seg, member_pts, cameras, n_cameras, prm, line, rms_before, rms_after, iterations, status, seg_count, segs,
                                   n_segs, in, msg);
    if (rv) return fail(c, rv, msg);
    if (n_groups == 0) return L3D_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t nm = (size_t)group_start[n_groups], ng = (size_t)n_groups, nc = (size_t)n_cameras;
    std::vector<refine::Cam> cams(nc + 1);
    for (size_t k = 0; k < nc; ++k) refine::make_cam(cameras + 12 * k, cams[k]);
    // inputs (g0): group table, member tables, cameras
    const size_t o_gs = 0, o_mc = al((ng + 1) * 4), o_ms = o_mc + al(nm * 4 + 4), o_mp = o_ms + al(nm * 16 + 16), o_cam = o_mp + al(nm * 48 + 48), in_bytes = o_cam + al((nc + 1) * sizeof(refine::Cam));
    HIPCHK(c, c->g0.reserve(in_bytes));
    char* ib = c->g0.as<char>();
    HIPCHK(c, hipMemcpyAsync(ib + o_gs, group_start, (ng + 1) * 4, hipMemcpyHostToDevice, st));
    if (nm) {
        HIPCHK(c, hipMemcpyAsync(ib + o_mc, member_cam, nm * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(ib + o_ms, member_seg, nm * 16, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(ib + o_mp, member_pts, nm * 48, hipMemcpyHostToDevice, st));
    }
    if (nc) HIPCHK(c, hipMemcpyAsync(ib + o_cam, cams.data(), nc * sizeof(refine::Cam), hipMemcpyHostToDevice, st));
    // scratch and outputs (g1), allocated like FitArgs's
    const size_t o_t = 0, o_ord = al(2 * nm * 8 + 8), o_open = o_ord + al(2 * nm * 4 + 4), o_ci = o_open + al(nm + 4), o_cc = o_ci + al(nm * 4 + 4), o_res = o_cc + al(nm * 4 + 4);
    // (results in one block, read back with one copy: line 6 | rms_before | rms_after doubles, then iterations | status | out_cnt ints, then the segments)
    const size_t r_line = 0, r_rb = r_line + ng * 48, r_ra = r_rb + ng * 8, r_it = r_ra + ng * 8, r_st = r_it + ng * 4, r_cnt = r_st + ng * 4, r_out = al(r_cnt + ng * 4), res_bytes = r_out + nm * 48 + 8;
    HIPCHK(c, c->g1.reserve(o_res + res_bytes));
    char* sb = c->g1.as<char>();
    RefineArgs a;
    a.n_groups = n_groups;
    a.group_start = reinterpret_cast<const int*>(ib + o_gs); a.member_cam = reinterpret_cast<const int*>(ib + o_mc); a.member_seg = reinterpret_cast<const float*>(ib + o_ms);
    a.member_pts = reinterpret_cast<const double*>(ib + o_mp); a.cams = reinterpret_cast<const refine::Cam*>(ib + o_cam);
    a.max_iterations = in.max_iterations; a.huber = in.huber;
    a.t = reinterpret_cast<double*>(sb + o_t); a.order = reinterpret_cast<int*>(sb + o_ord); a.line_open = reinterpret_cast<unsigned char*>(sb + o_open);
    a.cam_ids = reinterpret_cast<unsigned*>(sb + o_ci); a.cam_cnt = reinterpret_cast<unsigned*>(sb + o_cc);
    char* rb = sb + o_res;
    a.line = reinterpret_cast<double*>(rb + r_line); a.rms_before = reinterpret_cast<double*>(rb + r_rb); a.rms_after = reinterpret_cast<double*>(rb + r_ra);
    a.iterations = reinterpret_cast<int*>(rb + r_it); a.status = reinterpret_cast<int*>(rb + r_st); a.out_cnt = reinterpret_cast<int*>(rb + r_cnt); a.out = reinterpret_cast<double*>(rb + r_out);
    HIPCHK(c, hipMemsetAsync(rb, 0, r_out, st));
    { ProfScope p(c, "refine_lines", st); hipLaunchKernelGGL(k_refine_lines, dim3((n_groups + 3) / 4), dim3(256), 0, st, a); }
    std::vector<char> host(res_bytes);
    hipError_t e1 = hipMemcpyAsync(host.data(), rb, res_bytes, hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipStreamSynchronize(st);
    hipError_t e3 = hipGetLastError();
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
        return fail(c, L3D_ERR_HIP, std::string("refine: ") + hipGetErrorString(e1 != hipSuccess ? e1 : (e2 != hipSuccess ? e2 : e3)));
    memcpy(line, host.data() + r_line, ng * 48); memcpy(rms_before, host.data() + r_rb, ng * 8); memcpy(rms_after, host.data() + r_ra, ng * 8);
    memcpy(iterations, host.data() + r_it, ng * 4); memcpy(status, host.data() + r_st, ng * 4);
    const int rp = refine_pack(group_start, n_groups, reinterpret_cast<const int32_t*>(host.data() + r_cnt), reinterpret_cast<const double*>(host.data() + r_out), seg_count, segs, n_segs);
    return rp ? fail(c, rp, "malloc") : L3D_OK;
}

// the hypothesis table the last affinity fill left on the device (greedy selection's P1 / P2 in the normalised frame), for the pipeline's refinement
namespace l3d { int fetch_fill_hypotheses(l3d_ctx* c, int n_hyp, l3d_hypothesis* out); }
int l3d::fetch_fill_hypotheses(l3d_ctx* c, int n_hyp, l3d_hypothesis* out)
{
    if (!c || !out || n_hyp < 0) return L3D_ERR_INVALID;
    if (c->resident_hyp != n_hyp) return fail(c, L3D_ERR_INVALID, "refine: no resident hypothesis table of that size");
    if (n_hyp == 0) return L3D_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, c->aff_hyp.p, (size_t)n_hyp * sizeof(l3d_hypothesis), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return L3D_OK;
}
