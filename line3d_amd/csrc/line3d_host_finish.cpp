// line3d_host_finish.cpp -- what follows matchViews in compute3Dmodel: greedy selection, affinity fill, diffusion, clustering, line fit (line3D.cc:899-1597, clustering.cc)
// (one translation unit of the host pipeline; shared declarations: line3d_host_internal.hpp)
#include "line3d_host_internal.hpp"

namespace l3dh {

// L3DView::unprojectSegment, view.cc:302-342 (the arithmetic is shared with the device: l3d_unproject.hpp)
void unproject_segment(const View& v, uint32_t id, float d1, float d2, Hyp& o)
{
    const float* s = &v.segs[(size_t)id * 4];
    l3d::unproject_segment_f64(v.RtKinv, v.C, s[0], s[1], s[2], s[3], d1, d2, o.P1, o.P2, o.dir);
    o.depth_p1 = d1; o.depth_p2 = d2;
}

// ---- small thread helpers of the finishing stages (greedy selection .. line fit run alone on the host) ----------
unsigned finish_threads() { return l3d::host_threads(); }

// fn(begin, end, thread) over [0, n) in contiguous slices
template <class F>
void parallel_slices(size_t n, unsigned nt, F fn)
{
    nt = (unsigned)std::max<size_t>(1, std::min<size_t>(nt, n));
    if (nt == 1) { fn((size_t)0, n, 0u); return; }
    l3d::on_threads(nt, [&](unsigned t) { fn(n * t / nt, n * (t + 1) / nt, t); });
}

// Line3D::greedySelection, line3D.cc:899-965: the stored list holds one (best) match per segment.  The views are independent:
// worker threads pick the best match of every segment of their views, the hypotheses are numbered view by view afterwards
// (a prefix over the views' counts) and unprojected in parallel.
void greedy_selection(L* h)
{
    const size_t nv = h->vlist.size();
    h->best_idx.resize(nv);
    std::vector<std::vector<int>> best(nv);                  // per view: index into the store of the segment's best match, or -1
    std::vector<size_t> count(nv + 1, 0);
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(finish_threads(), nv));
    auto for_views = [&](auto fn) {
        std::atomic<size_t> next{ 0 };
        auto worker = [&]() { for (;;) { const size_t vi = next.fetch_add(1, std::memory_order_relaxed); if (vi >= nv) break; fn(vi); } };
        l3d::on_threads(nt, [&](unsigned) { worker(); });
    };
    for_views([&](size_t vi) {
        View* v = h->vlist[vi];
        const uint32_t S = (uint32_t)v->S();
        std::vector<int>& b = best[vi];
        b.assign((size_t)S, -1);
        h->best_idx[(size_t)v->index].assign((size_t)S, -1);
        if (!v->store_exists) return;
        // group by segment (ascending), first of the highest confidence
        for (size_t i = 0; i < v->store.size(); ++i) {
            const uint32_t sg = v->store[i].segID1;
            if (sg >= S) continue;
            if (b[sg] < 0 || v->store[i].confidence > v->store[(size_t)b[sg]].confidence) b[sg] = (int)i;
        }
        size_t n = 0;
        for (uint32_t sg = 0; sg < S; ++sg) n += b[sg] >= 0;
        count[vi + 1] = n;
    });
    for (size_t vi = 0; vi < nv; ++vi) count[vi + 1] += count[vi];
    h->hyps.resize(count[nv]);
    h->hyp_begin = count;                                    // the hypotheses of view index vi are [hyp_begin[vi], hyp_begin[vi + 1])
    // (the flat copies the device affinity fill takes -- hypothesis, score, dense segment id -- are written in the same pass)
    std::vector<size_t> voff(nv + 1, 0);
    for (size_t vi = 0; vi < nv; ++vi) voff[vi + 1] = voff[vi] + (size_t)h->vlist[vi]->S();
    h->aff.hyp.resize(count[nv]); h->aff.score.resize(count[nv]); h->aff.hyp_dense.resize(count[nv]); h->aff.hyp_cam.resize(count[nv]);
    for_views([&](size_t vi) {
        View* v = h->vlist[vi];
        std::vector<int>& bi = h->best_idx[(size_t)v->index];
        const std::vector<int>& b = best[vi];
        size_t k = count[vi];
        for (uint32_t sg = 0; sg < (uint32_t)b.size(); ++sg) {
            if (b[sg] < 0) continue;
            const l3d_match& mp = v->store[(size_t)b[sg]];
            Hyp hy;
            hy.src = mk(v->id, sg);
            hy.score = fminf(mp.confidence, 1.0f);
            unproject_segment(*v, sg, mp.depths[0], mp.depths[1], hy);
            bi[sg] = (int)k;
            l3d_hypothesis& o = h->aff.hyp[k];
            o.P1[0] = hy.P1.x; o.P1[1] = hy.P1.y; o.P1[2] = hy.P1.z;
            o.P2[0] = hy.P2.x; o.P2[1] = hy.P2.y; o.P2[2] = hy.P2.z;
            o.dir[0] = hy.dir.x; o.dir[1] = hy.dir.y; o.dir[2] = hy.dir.z;
            o.depth_p1 = hy.depth_p1; o.depth_p2 = hy.depth_p2;
            o.k_lower = v->k_lower; o.k_upper = v->k_upper; o.median_depth = v->median_depth; o.pad = 0;
            h->aff.score[k] = hy.score;
            h->aff.hyp_dense[k] = (int32_t)(voff[vi] + sg);
            h->aff.hyp_cam[k] = v->id;
            h->hyps[k++] = hy;
        }
    });
}

int best_of(const L* h, Key k)
{
    auto it = h->views.find(kcam(k));
    if (it == h->views.end()) return -1;
    const std::vector<int>& bi = h->best_idx[(size_t)it->second.index];
    return kseg(k) < bi.size() ? bi[kseg(k)] : -1;
}

// Felzenszwalb-Huttenlocher segmentation, clustering.cc:6-47 + universe.h:59-115, on the host: the fallback for lists the device path
// refuses and the cross-check of l3d_perform_clustering_device (L3D_HOST_CLUSTERING=1)
// presorted: edges_in already is in the stable ascending weight order (l3d_clustering_edges)
void perform_clustering(const l3d_edge* edges_in, size_t n_edges, int numNodes, float c, std::vector<int>& labels, bool presorted)
{
    // stable ascending order of the weights (clustering.cc:14: std::stable_sort over CLEdge::operator<)
    std::unique_ptr<l3d_edge[]> gathered;
    const l3d_edge* sorted = edges_in;
    if (!presorted) {
        std::vector<uint32_t> order;
        {
            const l3d_edge* e = edges_in;
            l3d::parallel_stable_order(n_edges, (size_t)65536, (size_t)65536, [e](size_t i) { return l3d::float_order_key(e[i].w) >> 16; },
                                       [e](size_t i) { return l3d::float_order_key(e[i].w) & 0xffffu; }, finish_threads(), order);
        }
        // the edges in that order, gathered by the worker threads (the merge loop below then reads them sequentially)
        gathered.reset(new l3d_edge[n_edges + 1]);
        l3d_edge* g = gathered.get();
        parallel_slices(n_edges, finish_threads(), [&](size_t k0, size_t k1, unsigned) { for (size_t k = k0; k < k1; ++k) g[k] = edges_in[order[k]]; });
        sorted = g;
    }
    std::vector<int> rank((size_t)numNodes, 0), cid((size_t)numNodes), size((size_t)numNodes, 1);
    std::vector<float> thr((size_t)numNodes, c);
    for (int i = 0; i < numNodes; ++i) cid[i] = i;
    // universe.h:81-89 compresses only the queried node's link; halving every link on the way finds the same root (unions
    // go by rank, which no compression touches) with shorter chains afterwards
    auto find = [&](int node) { int y = node; while (y != cid[y]) { cid[y] = cid[cid[y]]; y = cid[y]; } return y; };
    for (size_t q = 0; q < n_edges; ++q) {
        const l3d_edge& ed = sorted[q];
        int a = find(ed.i), b = find(ed.j);
        if (a != b && ed.w <= thr[a] && ed.w <= thr[b]) {
            if (rank[a] > rank[b]) { cid[b] = a; size[a] += size[b]; }
            else { cid[a] = b; size[b] += size[a]; if (rank[a] == rank[b]) rank[b]++; }
            a = find(a);
            thr[a] = ed.w + c / (float)size[a];
        }
        // the affinity list holds every edge in both directions, and the stable order keeps the two together: whatever the
        // first one did (merged its components, found them merged, or failed a threshold), the reversed twin right behind it
        // meets the very same state and changes nothing
        if (q + 1 < n_edges && sorted[q + 1].i == ed.j && sorted[q + 1].j == ed.i && sorted[q + 1].w == ed.w) ++q;
    }
    labels.resize((size_t)numNodes);
    for (int k = 0; k < numNodes; ++k) labels[k] = find(k);
}

// The same segmentation from the edge list grouped by connected component (l3d_clustering_edges_grouped): the merge loop never
// relates nodes of different components, so every group is walked on its own -- same unions, same ranks, same roots as the one
// sequential walk over the whole sorted list -- by the worker threads (config 2: 3240 components, the largest 1326 edges).
void perform_clustering_grouped(const l3d_edge* sorted, const int32_t* group_start, int n_groups, int numNodes, float c, std::vector<int>& labels)
{
    std::unique_ptr<int[]> rank(new int[(size_t)numNodes + 1]), cid(new int[(size_t)numNodes + 1]), size(new int[(size_t)numNodes + 1]);
    std::unique_ptr<float[]> thr(new float[(size_t)numNodes + 1]);
    labels.resize((size_t)numNodes);
    const unsigned nt = finish_threads();
    parallel_slices((size_t)numNodes, nt, [&](size_t k0, size_t k1, unsigned) { for (size_t k = k0; k < k1; ++k) { rank[k] = 0; cid[k] = (int)k; size[k] = 1; thr[k] = c; } });
    int *cidp = cid.get(), *rankp = rank.get(), *sizep = size.get();
    float* thrp = thr.get();
    auto find = [cidp](int node) { int y = node; while (y != cidp[y]) { cidp[y] = cidp[cidp[y]]; y = cidp[y]; } return y; };
    std::atomic<int> next{ 0 };
    l3d::on_threads((unsigned)std::max(1, std::min<int>((int)nt, n_groups / 16 + 1)), [&](unsigned) {
        for (;;) {
            const int g0 = next.fetch_add(32, std::memory_order_relaxed);
            if (g0 >= n_groups) break;
            for (int g = g0; g < std::min(n_groups, g0 + 32); ++g)
                for (int q = group_start[g]; q < group_start[g + 1]; ++q) {
                    const l3d_edge& ed = sorted[q];
                    int a = find(ed.i), b = find(ed.j);
                    if (a != b && ed.w <= thrp[a] && ed.w <= thrp[b]) {
                        if (rankp[a] > rankp[b]) { cidp[b] = a; sizep[a] += sizep[b]; }
                        else { cidp[a] = b; sizep[b] += sizep[a]; if (rankp[a] == rankp[b]) rankp[b]++; }
                        a = find(a);
                        thrp[a] = ed.w + c / (float)sizep[a];
                    }
                    if (q + 1 < group_start[g + 1] && sorted[q + 1].i == ed.j && sorted[q + 1].j == ed.i && sorted[q + 1].w == ed.w) ++q;   // (reversed twin)
                }
        }
    });
    // (read-only walks: several threads may look up nodes of one component)
    parallel_slices((size_t)numNodes, nt, [&](size_t k0, size_t k1, unsigned) { for (size_t k = k0; k < k1; ++k) { int y = (int)k; while (y != cidp[y]) y = cidp[y]; labels[k] = y; } });
}

// Line3D::performDiffusion, line3D.cc:1255-1303: A (read) -> diffused, symmetrised list sorted by (i,j) in `out`
int perform_diffusion(L* h, const EdgeVec& A, int n, EdgeVec& out)
{
    EdgeVec W;
    W.resize(A.size());
    int rc = l3d_replicator_dynamics_diffusion(h->ctx, A.data(), (int)A.size(), n, L3D_RDD_MAX_ITER, W.data());
    if (rc) return h->fail(rc, std::string("rdd: ") + l3d_last_error(h->ctx));
    const double t_sym = now_s();
    // symmetrise by the minimum and rebuild A sorted by (i,j) (:1275-1301).  The diffused entries come back sorted by
    // (row, column); when they are unique and the pattern is symmetric -- always the case for the affinity list built by
    // clusterSegments2D -- the reference's map arithmetic reduces to A(i,j) = A(j,i) = min(W(i,j), W(j,i)) in that same order.
    const unsigned nt = finish_threads();
    std::atomic<int> unsorted{ 0 };
    parallel_slices(W.size(), nt, [&](size_t k0, size_t k1, unsigned) {
        for (size_t k = std::max<size_t>(k0, 1); k < k1; ++k)
            if (!(W[k - 1].i < W[k].i || (W[k - 1].i == W[k].i && W[k - 1].j < W[k].j))) { unsorted.store(1, std::memory_order_relaxed); break; }
    });
    if (!unsorted.load()) {
        std::vector<int> row((size_t)n + 1, 0);
        for (const l3d_edge& e : W) ++row[(size_t)e.i + 1];
        for (int r = 0; r < n; ++r) row[(size_t)r + 1] += row[(size_t)r];
        out.resize(W.size());
        std::atomic<int> missing{ 0 };
        parallel_slices(W.size(), nt, [&](size_t k0, size_t k1, unsigned) {
            for (size_t k = k0; k < k1; ++k) {
                const l3d_edge& e = W[k];
                const l3d_edge* lo = W.data() + row[(size_t)e.j];
                const l3d_edge* hi = W.data() + row[(size_t)e.j + 1];
                const l3d_edge* t = std::lower_bound(lo, hi, e.i, [](const l3d_edge& x, int col) { return x.j < col; });
                if (t == hi || t->j != e.i) { missing.fetch_add(1, std::memory_order_relaxed); break; }
                out[k] = { e.i, e.j, e.i <= e.j ? fminf(t->w, e.w) : fminf(e.w, t->w) };     // the visit of the later entry decides
            }
        });
        if (missing.load() == 0) {
            if (hopt(h).timing) fprintf(stderr, "[l3d rdd] %-24s %8.2f ms\n", "symmetrise", (now_s() - t_sym) * 1e3);
            return L3D_OK;
        }
    }
    std::map<std::pair<int, int>, float> entries;
    for (const l3d_edge& e : W) {
        const float w12 = e.w;
        float w21 = w12;
        auto it = entries.find({ e.j, e.i });
        if (it != entries.end()) w21 = it->second;
        const float w = fminf(w12, w21);
        entries[{ e.i, e.j }] = w;
        entries[{ e.j, e.i }] = w;
    }
    out.clear();
    for (auto& kv : entries) out.push_back({ kv.first.first, kv.first.second, kv.second });
    return L3D_OK;
}

// getLineEquation3D + projectToLine, line3D.cc:1392-1597 (the arithmetic lives in l3d_linefit.hpp, shared with the device kernel)
void align_cluster(const std::vector<std::pair<Key, std::pair<V3, V3>>>& t3, std::vector<std::pair<V3, V3>>& aligned)
{
    aligned.clear();
    if (t3.empty()) return;
    const int n2 = (int)t3.size() * 2;
    auto get = [&](int i) { return (i & 1) ? t3[(size_t)(i >> 1)].second.second : t3[(size_t)(i >> 1)].second.first; };
    V3 Pc, dir, min_point;
    l3d::fit::line_of_points(get, n2, Pc, dir, min_point);
    static thread_local std::vector<float> dist;             // (per-thread buffers: a fit is a few microseconds, allocations were a third of it)
    static thread_local std::vector<int> order;
    static thread_local std::vector<unsigned char> line_open;
    static thread_local std::vector<unsigned> cam_ids, cam_cnt;
    dist.resize((size_t)n2); order.resize((size_t)n2); line_open.resize(t3.size()); cam_ids.resize(t3.size()); cam_cnt.resize(t3.size());
    for (int i = 0; i < n2; ++i) { dist[(size_t)i] = l3d::fit::point_dist(get(i), min_point); order[(size_t)i] = i; }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return dist[(size_t)a] < dist[(size_t)b]; });
    l3d::fit::sweep_line(order.data(), n2, get, [&](int member) { return kcam(t3[(size_t)member].first); }, line_open.data(), cam_ids.data(), cam_cnt.data(),
                         [&](V3 s0, V3 e0) { aligned.emplace_back(s0, e0); });
}

// segment2collinearities_ of all views as one CSR over dense ids (static per scene: kept between calls)
void pack_collinearities(L* h, const std::vector<size_t>& voff)
{
    L::AffTables& T = h->aff;
    const size_t nv = h->vlist.size(), ndense = voff.back();
    if (T.coll_valid && T.coll_start.size() == ndense + 1) return;
    T.coll_start.resize(ndense + 1);
    int64_t* coll_start = T.coll_start.data();
    coll_start[0] = 0;
    for (size_t vi = 0; vi < nv; ++vi) {
        const View& sv = *h->vlist[vi];
        for (size_t sg = 0; sg < (size_t)sv.S(); ++sg) coll_start[voff[vi] + sg + 1] = coll_start[voff[vi] + sg] + (sv.coll_start[sg + 1] - sv.coll_start[sg]);
    }
    const size_t n_coll = (size_t)coll_start[ndense];
    T.coll_other.resize(n_coll + 1); T.coll_w.resize(n_coll + 1);
    int32_t* coll_other = T.coll_other.data();
    float* coll_w = T.coll_w.data();
    std::atomic<size_t> next{ 0 };
    l3d::on_threads(std::min<unsigned>(finish_threads(), (unsigned)std::max<size_t>(1, nv)), [&](unsigned) {
        for (;;) {
            const size_t vi = next.fetch_add(1, std::memory_order_relaxed);
            if (vi >= nv) break;
            const View& sv = *h->vlist[vi];
            const size_t cb = (size_t)coll_start[voff[vi]], cn = sv.coll_other.size();
            for (size_t q = 0; q < cn; ++q) { coll_other[cb + q] = (int32_t)(voff[vi] + (size_t)sv.coll_other[q]); coll_w[cb + q] = sv.coll_w[q]; }
        }
    });
    T.coll_valid = false;           // (the caller uploads, then marks it valid)
}

// Line3D::greedySelection (line3D.cc:899-965) on the device-resident products of matchViews (l3d_products_hypotheses): the host
// keeps only what the result needs -- which 2-D segment every hypothesis belongs to
int greedy_selection_resident(L* h)
{
    const size_t nv = h->vlist.size();
    std::vector<l3d_view_geometry> geo(nv);
    for (size_t i = 0; i < nv; ++i) {
        const View& v = *h->vlist[i];
        l3d_view_geometry& g = geo[i];
        memcpy(g.RtKinv, v.RtKinv.m, 72);
        g.C[0] = v.C.x; g.C[1] = v.C.y; g.C[2] = v.C.z;
        g.k_lower = v.k_lower; g.k_upper = v.k_upper; g.median_depth = v.median_depth;
        g.n_segments = v.S(); g.segments = v.segs.data();
    }
    std::vector<int32_t> vhb(nv + 1, 0);
    int32_t* hyp_dense = nullptr; int nh = 0;
    int rc = l3d_products_hypotheses(h->ctx, geo.data(), (int)nv, vhb.data(), &hyp_dense, &nh);
    if (rc) return h->fail(rc, std::string("hypotheses: ") + l3d_last_error(h->ctx));
    h->hyp_begin.assign(nv + 1, 0);
    for (size_t i = 0; i <= nv; ++i) h->hyp_begin[i] = (size_t)vhb[i];
    h->hyps.resize((size_t)nh);
    h->aff.hyp_cam.resize((size_t)nh);
    h->best_idx.clear();
    std::vector<size_t> voff(nv + 1, 0);
    for (size_t i = 0; i < nv; ++i) voff[i + 1] = voff[i] + (size_t)h->vlist[i]->S();
    parallel_slices(nv, finish_threads(), [&](size_t v0, size_t v1, unsigned) {
        for (size_t vi = v0; vi < v1; ++vi)
            for (size_t k = h->hyp_begin[vi]; k < h->hyp_begin[vi + 1]; ++k) {
                h->hyps[k].src = mk(h->vlist[vi]->id, (uint32_t)((size_t)hyp_dense[k] - voff[vi]));
                h->aff.hyp_cam[k] = h->vlist[vi]->id;
            }
    });
    l3d_free(hyp_dense);
    return L3D_OK;
}

// the affinity list on the host (the resident fill leaves it on the device: fetched on first use)
int ensure_edges(L* h)
{
    if (h->A_on_host) return L3D_OK;
    h->A.resize(h->n_edges);
    int rc = l3d_resident_edges_get(h->ctx, h->A.data(), (int)h->n_edges);
    if (rc) { h->A.clear(); return h->fail(rc, std::string("affinity list: ") + l3d_last_error(h->ctx)); }
    h->A_on_host = true;
    return L3D_OK;
}

// the affinity fill on the resident tables (l3d_affinity_fill_resident): only the collinearity CSR comes from the host, once per scene
int fill_affinity_resident(L* h)
{
    const size_t nv = h->vlist.size();
    std::vector<size_t> voff(nv + 1, 0);
    for (size_t i = 0; i < nv; ++i) voff[i + 1] = voff[i] + (size_t)h->vlist[i]->S();
    L::AffTables& T = h->aff;
    const bool timing = hopt(h).timing != 0;
    double tl = now_s();
    auto lap = [&](const char* what) { if (timing) { const double t = now_s(); fprintf(stderr, "[l3d finish]   fill: %-22s %8.2f ms\n", what, (t - tl) * 1e3); tl = t; } };
    const bool changed = !T.coll_valid || T.coll_start.size() != voff.back() + 1;
    if (changed) pack_collinearities(h, voff);
    lap("collinearity tables");
    l3d_edge* edges = nullptr; int32_t* node_hyp = nullptr; int n_edges = 0, n_nodes = 0, n_cand = 0;
    // (the list itself stays on the device, where the clustering walks it; l3d_line3d_affinity fetches it when somebody asks)
    int rc = l3d_affinity_fill_resident(h->ctx, T.coll_start.data(), T.coll_other.data(), T.coll_w.data(), changed ? 1 : 0, h->sigma_a, nullptr, &n_edges, &node_hyp, &n_nodes, &n_cand);
    if (rc) return h->fail(rc, std::string("affinity fill: ") + l3d_last_error(h->ctx));
    lap("device");
    T.coll_valid = true;
    h->A.clear(); h->n_edges = (size_t)n_edges; h->A_on_host = n_edges == 0;
    h->local2global.resize((size_t)n_nodes);
    h->node_hyp.resize((size_t)n_nodes);
    parallel_slices((size_t)n_nodes, finish_threads(), [&](size_t k0, size_t k1, unsigned) {     // (a gather over the hypothesis table: 0.5 M nodes at 512 views)
        for (size_t k = k0; k < k1; ++k) { h->node_hyp[k] = node_hyp[k]; h->local2global[k] = h->hyps[(size_t)node_hyp[k]].src; }
    });
    l3d_free(edges); l3d_free(node_hyp);
    lap("node table");
    if (timing) fprintf(stderr, "[l3d finish] %zu hypotheses, %d candidate pairs, %zu edges (resident tables)\n", h->hyps.size(), n_cand, h->n_edges);
    return L3D_OK;
}

// the affinity fill of a job whose matchViews ran partitioned (l3d_affinity_fill_sharded): this rank's block of sources, then the global tables --
// hypothesis numbers, which segment every hypothesis belongs to -- replace the local ones of greedy_selection_resident
int fill_affinity_sharded(L* h)
{
    const size_t nv = h->vlist.size();
    std::vector<size_t> voff(nv + 1, 0);
    for (size_t i = 0; i < nv; ++i) voff[i + 1] = voff[i] + (size_t)h->vlist[i]->S();
    L::AffTables& T = h->aff;
    const bool changed = !T.coll_valid || T.coll_start.size() != voff.back() + 1;
    if (changed) pack_collinearities(h, voff);
    std::vector<int32_t> vhb(nv + 1, 0);
    int32_t *node_hyp = nullptr, *hyp_dense = nullptr;
    int n_edges = 0, n_nodes = 0, nh_all = 0;
    int64_t cand_all = 0;
    const double t0 = now_s();
    int rc = l3d_affinity_fill_sharded(h->ctx, T.coll_start.data(), T.coll_other.data(), T.coll_w.data(), changed ? 1 : 0, h->sigma_a, h->part_exchange, h->part_user,
                                       &n_edges, &node_hyp, &n_nodes, &cand_all, vhb.data(), &hyp_dense, &nh_all);
    if (rc) return h->fail(rc, std::string("affinity fill (sharded): ") + l3d_last_error(h->ctx));
    T.coll_valid = true;
    h->hyp_begin.assign(nv + 1, 0);
    for (size_t i = 0; i <= nv; ++i) h->hyp_begin[i] = (size_t)vhb[i];
    h->hyps.assign((size_t)nh_all, Hyp());
    h->aff.hyp_cam.assign((size_t)nh_all, 0u);
    parallel_slices(nv, finish_threads(), [&](size_t v0, size_t v1, unsigned) {
        for (size_t vi = v0; vi < v1; ++vi)
            for (size_t k = h->hyp_begin[vi]; k < h->hyp_begin[vi + 1]; ++k) {
                h->hyps[k].src = mk(h->vlist[vi]->id, (uint32_t)((size_t)hyp_dense[k] - voff[vi]));
                h->aff.hyp_cam[k] = h->vlist[vi]->id;
            }
    });
    h->A.clear(); h->n_edges = (size_t)n_edges; h->A_on_host = n_edges == 0;
    h->local2global.resize((size_t)n_nodes);
    h->node_hyp.resize((size_t)n_nodes);
    parallel_slices((size_t)n_nodes, finish_threads(), [&](size_t k0, size_t k1, unsigned) {
        for (size_t k = k0; k < k1; ++k) { h->node_hyp[k] = node_hyp[k]; h->local2global[k] = h->hyps[(size_t)node_hyp[k]].src; }
    });
    l3d_free(node_hyp); l3d_free(hyp_dense);
    if (hopt(h).timing) fprintf(stderr, "[l3d finish] sharded fill: %d hypotheses in the job, %lld candidate pairs, %zu edges, %.2f ms\n", nh_all, (long long)cand_all, h->n_edges, (now_s() - t0) * 1e3);
    return L3D_OK;
}

// Line3D::clusterSegments2D, line3D.cc:968-1252: the affinity fill and the edge list of the clustering on the device
// (l3d_affinity_fill / l3d_affinity_fill_resident, l3d_perform_clustering_device, l3d_fit_labelled_clusters); host union-find, symmetrisation and
// edge order remain for edge lists the device path refuses.  (The literal `used` enumeration of round 1 lives on as a test helper:
// tests/cpp/literal_used_rule.c.)
int cluster_segments_2D(L* h, bool perform_diff)
{
    const double t0 = now_s();
    const bool timing = hopt(h).timing != 0;
    double tm_last = t0;
    auto lap = [&](const char* what) { if (timing) { const double t = now_s(); fprintf(stderr, "[l3d finish] %-28s %8.2f ms\n", what, (t - tm_last) * 1e3); tm_last = t; } };
    h->A.clear(); h->n_edges = 0; h->A_on_host = true; h->local2global.clear(); h->result.clear();
    size_t nh = h->hyps.size();
    if (nh == 0 && !h->partitioned) return L3D_OK;          // (partitioned: a rank without hypotheses still takes part in the collective fill)

    // dense index of every 2-D segment of every view (for the `used` bookkeeping)
    const size_t nv = h->vlist.size();
    std::vector<size_t> voff(nv + 1, 0);
    for (size_t i = 0; i < nv; ++i) voff[i + 1] = voff[i] + (size_t)h->vlist[i]->S();
    // camera id -> view index (ascending ids; ids are small in practice, else binary search)
    std::vector<uint32_t> cam_ids(nv);
    for (size_t i = 0; i < nv; ++i) cam_ids[i] = h->vlist[i]->id;
    std::vector<int> cam_direct;
    if (nv && cam_ids.back() < (1u << 22)) { cam_direct.assign((size_t)cam_ids.back() + 1, -1); for (size_t i = 0; i < nv; ++i) cam_direct[cam_ids[i]] = (int)i; }
    auto view_of = [&](uint32_t cam) -> int {
        if (!cam_direct.empty()) return cam < cam_direct.size() ? cam_direct[cam] : -1;
        auto it = std::lower_bound(cam_ids.begin(), cam_ids.end(), cam);
        return it != cam_ids.end() && *it == cam ? (int)(it - cam_ids.begin()) : -1;
    };
    // hypotheses are in (view, segment) order: the range of each view (greedy_selection)
    const std::vector<size_t>& hyp_begin = h->hyp_begin;
    if (hyp_begin.size() != nv + 1 || hyp_begin[nv] != nh) return h->fail(L3D_ERR_INVALID, "hypothesis ranges do not match the views");

    bool resident_list = false;                     // the affinity list is still on the device (l3d_affinity_fill ran last)
    if (h->partitioned) {
        const int rc = fill_affinity_sharded(h);
        if (rc) return rc;
        resident_list = true;
        nh = h->hyps.size();                        // (global from here on)
        lap("affinity fill (sharded by source key)");
    } else if (h->resident_products) {
        const int rc = fill_affinity_resident(h);
        if (rc) return rc;
        resident_list = true;
        lap("affinity fill (resident tables)");
    } else {
        resident_list = true;
        // ---- the whole fill on the device (l3d_affinity.hip): flat tables in, edge list and node numbering out
        const unsigned nt = finish_threads();
        if (voff.back() > 0x7fffffffu || nh > 0x3fffffffu) return h->fail(L3D_ERR_INVALID, "affinity fill: too many segments");
        const size_t ndense = voff.back();
        std::vector<int32_t> seg_base(nv + 1), vhb(nv + 1);
        for (size_t i = 0; i <= nv; ++i) { seg_base[i] = (int32_t)voff[i]; vhb[i] = (int32_t)hyp_begin[i]; }
        vhb[nv] = (int32_t)nh;
        L::AffTables& T = h->aff;
        if (T.hyp.size() != nh || T.score.size() != nh || T.hyp_dense.size() != nh) return h->fail(L3D_ERR_INVALID, "hypothesis tables do not match the hypotheses");
        T.best.resize(ndense + 1);                      // (hypothesis, score, dense id: written by greedy_selection)
        l3d_hypothesis* hy = T.hyp.data();
        float* score = T.score.data();
        int32_t *hyp_dense = T.hyp_dense.data(), *best = T.best.data();
        lap("  pack: hypotheses");
        // potential correspondences and collinearities as CSR over dense ids (a view's rows are written by one thread)
        T.pot_start.resize(ndense + 1);
        int64_t* pot_start = T.pot_start.data();
        const bool pack_coll = !T.coll_valid || T.coll_start.size() != ndense + 1;
        if (pack_coll) T.coll_start.resize(ndense + 1);
        int64_t* coll_start = T.coll_start.data();
        std::vector<std::vector<int32_t>>& vt = h->aff_vt;
        vt.resize(nv);
        pot_start[0] = 0;
        if (pack_coll) coll_start[0] = 0;
        {
            std::atomic<size_t> next{ 0 };
            auto worker = [&]() {
                for (;;) {
                    const size_t vi = next.fetch_add(1, std::memory_order_relaxed);
                    if (vi >= nv) break;
                    const View& sv = *h->vlist[vi];
                    const size_t S = (size_t)sv.S();
                    for (size_t sg = 0; sg < S; ++sg) { pot_start[voff[vi] + sg + 1] = 0; best[voff[vi] + sg] = h->best_idx[vi][sg]; }
                    if (pack_coll) for (size_t sg = 0; sg < S; ++sg) coll_start[voff[vi] + sg + 1] = sv.coll_start[sg + 1] - sv.coll_start[sg];
                    std::vector<int32_t>& out = vt[vi];
                    out.clear();
                    out.reserve(h->pot[vi].size());
                    for (const auto& e : h->pot[vi]) {
                        // keys whose camera is not a view (early-return quirk) or whose segment does not exist never have a
                        // hypothesis or collinear segments: they take no part in the fill
                        const int tvi = view_of(kcam(e.second));
                        if (tvi < 0 || e.first >= S) continue;
                        const uint32_t tseg = kseg(e.second);
                        if (tseg >= (uint32_t)(voff[(size_t)tvi + 1] - voff[(size_t)tvi])) continue;
                        out.push_back((int32_t)(voff[(size_t)tvi] + tseg));
                        ++pot_start[voff[vi] + e.first + 1];
                    }
                }
            };
            l3d::on_threads(std::min<unsigned>(nt, (unsigned)nv), [&](unsigned) { worker(); });
        }
        lap("  pack: count + targets per view");
        for (size_t dd = 0; dd < ndense; ++dd) pot_start[dd + 1] += pot_start[dd];
        if (pack_coll) for (size_t dd = 0; dd < ndense; ++dd) coll_start[dd + 1] += coll_start[dd];
        const size_t n_pot = (size_t)pot_start[ndense], n_coll = (size_t)coll_start[ndense];
        T.pot_tgt.resize(n_pot + 1);
        if (pack_coll) { T.coll_other.resize(n_coll + 1); T.coll_w.resize(n_coll + 1); }
        int32_t *pot_tgt = T.pot_tgt.data(), *coll_other = T.coll_other.data();
        float* coll_w = T.coll_w.data();
        {
            std::atomic<size_t> next{ 0 };
            auto worker = [&]() {
                for (;;) {
                    const size_t vi = next.fetch_add(1, std::memory_order_relaxed);
                    if (vi >= nv) break;
                    const View& sv = *h->vlist[vi];
                    if (!vt[vi].empty()) memcpy(pot_tgt + pot_start[voff[vi]], vt[vi].data(), vt[vi].size() * 4);
                    if (!pack_coll) continue;
                    const size_t cb = (size_t)coll_start[voff[vi]], cn = sv.coll_other.size();
                    for (size_t q = 0; q < cn; ++q) { coll_other[cb + q] = (int32_t)(voff[vi] + (size_t)sv.coll_other[q]); coll_w[cb + q] = sv.coll_w[q]; }
                }
            };
            l3d::on_threads(std::min<unsigned>(nt, (unsigned)nv), [&](unsigned) { worker(); });
        }
        T.coll_valid = true;
        lap("pack tables");
        l3d_affinity_input in;
        in.n_views = (int32_t)nv; in.seg_base = seg_base.data(); in.view_hyp_begin = vhb.data();
        in.n_hyp = (int32_t)nh; in.hyp = hy; in.score = score; in.hyp_dense = hyp_dense; in.best = best;
        in.pot_start = pot_start; in.pot_tgt = pot_tgt;
        in.coll_start = coll_start; in.coll_other = coll_other; in.coll_w = coll_w;
        in.sigma_a = h->sigma_a;
        l3d_edge* edges = nullptr; int32_t* node_hyp = nullptr; int n_edges = 0, n_nodes = 0, n_cand = 0;
        int rc = l3d_affinity_fill(h->ctx, &in, &edges, &n_edges, &node_hyp, &n_nodes, &n_cand);
        if (rc) return h->fail(rc, std::string("affinity fill: ") + l3d_last_error(h->ctx));
        lap("affinity fill (device)");
        h->A.resize((size_t)n_edges);
        parallel_slices((size_t)n_edges, nt, [&](size_t k0, size_t k1, unsigned) { if (k1 > k0) memcpy(&h->A[k0], edges + k0, (k1 - k0) * sizeof(l3d_edge)); });
        h->local2global.resize((size_t)n_nodes);
        for (int k = 0; k < n_nodes; ++k) h->local2global[(size_t)k] = h->hyps[(size_t)node_hyp[k]].src;
        h->node_hyp.assign(node_hyp, node_hyp + n_nodes);
        l3d_free(edges); l3d_free(node_hyp);
        h->n_edges = h->A.size(); h->A_on_host = true;
        if (timing) fprintf(stderr, "[l3d finish] %zu hypotheses, %d candidate pairs, %zu edges, %u threads\n", nh, n_cand, h->A.size(), nt);
        lap("edge list to host");
    }
    h->t_affinity = now_s() - t0;
    if (h->n_edges == 0) return L3D_OK;                                         // :1232-1233

    const double t1 = now_s();
    const int n_nodes = (int)h->local2global.size();
    std::vector<int> labels;
    bool labels_on_device = false;
    {
        // the list clustering walks -- diffused and symmetrised when asked for, in stable ascending weight order -- comes from
        // the device, where the affinity list still is (l3d_clustering_edges); a list the device path does not take
        // (L3D_ERR_UNSUPPORTED) goes through the reference's map arithmetic on the host
        // ... and so does the merge loop itself, one wave per connected component (l3d_perform_clustering_device): only the labels
        // come back.  L3D_HOST_CLUSTERING=1 keeps the merge loop on the worker threads (the seam tests compare the two).
        const bool host_loop = hopt(h).host_clustering != 0;
        const int nnz = (int)h->n_edges, diff = perform_diff ? 1 : 0;
        int rc = L3D_ERR_UNSUPPORTED;
        if (resident_list && !host_loop) {
            // (the labels stay on the device as well: the grouping and the fits follow there, l3d_fit_labelled_clusters)
            rc = l3d_perform_clustering_device(h->ctx, nullptr, nnz, n_nodes, diff, L3D_RDD_MAX_ITER, 1.0f, nullptr, nullptr);   // :1245
            if (rc == L3D_OK) { labels_on_device = true; lap(perform_diff ? "diffusion + clustering (device)" : "clustering (device)"); }
        } else if (resident_list) {
            std::unique_ptr<l3d_edge[]> sorted(new l3d_edge[h->n_edges + 1]);
            int32_t* group_start = nullptr;
            int n_groups = 0;
            rc = l3d_clustering_edges_grouped(h->ctx, nullptr, nnz, n_nodes, diff, L3D_RDD_MAX_ITER, sorted.get(), &group_start, &n_groups);
            if (rc == L3D_OK) {
                lap(perform_diff ? "diffusion + grouped edge order (device)" : "grouped edge order (device)");
                perform_clustering_grouped(sorted.get(), group_start, n_groups, n_nodes, 1.0f, labels);   // :1245
                l3d_free(group_start);
            }
        }
        if (rc == L3D_ERR_UNSUPPORTED) {
            if (int e = ensure_edges(h)) return e;
            EdgeVec diffused;
            if (perform_diff) { rc = perform_diffusion(h, h->A, n_nodes, diffused); if (rc) return rc; lap("diffusion"); }
            const EdgeVec& edges = perform_diff ? diffused : h->A;
            perform_clustering(edges.data(), edges.size(), n_nodes, 1.0f, labels);
        } else if (rc != L3D_OK) return h->fail(rc, std::string("clustering: ") + l3d_last_error(h->ctx));
    }
    lap("clustering");

    if (labels_on_device) {
        // processClusteredSegments, line3D.cc:1306-1368, from the labels on the device: grouping (ascending label, members in key order,
        // >= 4 cameras) and the fits in one call; the host turns the answer into the result list
        int32_t *gstart = nullptr, *memb = nullptr, *cnt = nullptr; double* segs = nullptr; int n_groups = 0, n_segs = 0;
        const double tneg[3] = { h->transf_tneg.x, h->transf_tneg.y, h->transf_tneg.z };
        const int rc = l3d_fit_labelled_clusters(h->ctx, nullptr, nullptr, n_nodes, nullptr, h->aff.hyp_cam.data(), (int)h->hyps.size(), h->transf_Rinv.m, h->transf_scale_inv,
                                                 tneg, &gstart, &memb, &n_groups, &cnt, &segs, &n_segs);
        if (rc) return h->fail(rc, std::string("line fit: ") + l3d_last_error(h->ctx));
        lap("  fit: grouping + fits (device)");
        h->fit_on_device = true;
        std::vector<size_t> soff((size_t)n_groups + 1, 0);
        for (int v = 0; v < n_groups; ++v) soff[(size_t)v + 1] = soff[(size_t)v] + (size_t)cnt[v];
        std::vector<FinalLine> fitted((size_t)n_groups);
        parallel_slices((size_t)n_groups, finish_threads(), [&](size_t v0, size_t v1, unsigned) {
            for (size_t v = v0; v < v1; ++v) {
                if (cnt[v] == 0) continue;
                FinalLine& fl = fitted[v];
                for (size_t k = soff[v]; k < soff[v + 1]; ++k) {
                    const double* q = segs + 6 * k;
                    fl.segs3D.emplace_back(V3{ q[0], q[1], q[2] }, V3{ q[3], q[4], q[5] });
                }
                for (int32_t i = gstart[v]; i < gstart[v + 1]; ++i) fl.segs2D.push_back(h->hyps[(size_t)memb[(size_t)i]].src);
            }
        });
        size_t n_lines = 0;
        for (int v = 0; v < n_groups; ++v) n_lines += cnt[v] != 0;
        l3d_free(gstart); l3d_free(memb); l3d_free(cnt); l3d_free(segs);
        h->result.reserve(n_lines);
        for (FinalLine& fl : fitted) if (!fl.segs3D.empty()) h->result.push_back(std::move(fl));
        lap("line fit");
        h->t_cluster = now_s() - t1;
        return L3D_OK;
    }

    // processClusteredSegments, line3D.cc:1306-1368: clusters in ascending label order (the reference's std::map), their
    // segments in key order; clusters seen from >= 4 cameras are fitted, independently of each other, by the worker threads
    std::vector<int> lstart((size_t)n_nodes + 1, 0), lnodes((size_t)n_nodes);
    for (int lid = 0; lid < n_nodes; ++lid) ++lstart[(size_t)labels[(size_t)lid] + 1];
    for (int l = 0; l < n_nodes; ++l) lstart[(size_t)l + 1] += lstart[(size_t)l];
    {
        std::vector<int> cur(lstart.begin(), lstart.end() - 1);
        for (int lid = 0; lid < n_nodes; ++lid) lnodes[(size_t)cur[(size_t)labels[(size_t)lid]]++] = lid;
    }
    std::vector<int> groups;                                                    // labels with >= 4 members (>= 4 cameras needs that)
    for (int l = 0; l < n_nodes; ++l) if (lstart[(size_t)l + 1] - lstart[(size_t)l] >= 4) groups.push_back(l);
    std::vector<FinalLine> fitted(groups.size());
    lap("  fit: clusters by label");
    h->fit_on_device = false;
    if (resident_list && (int)h->node_hyp.size() == n_nodes) {
        // ---- the fits on the device (l3d_fit_clusters): members as hypothesis indices in key order (= ascending index)
        std::vector<int32_t> memb_tmp((size_t)n_nodes);
        std::vector<char> valid(groups.size(), 0);
        parallel_slices(groups.size(), finish_threads(), [&](size_t g0, size_t g1, unsigned) {
            for (size_t g = g0; g < g1; ++g) {
                const int l = groups[g];
                int32_t* mb = memb_tmp.data() + lstart[(size_t)l];
                const int n = lstart[(size_t)l + 1] - lstart[(size_t)l];
                for (int q = 0; q < n; ++q) mb[q] = h->node_hyp[(size_t)lnodes[(size_t)(lstart[(size_t)l] + q)]];
                std::sort(mb, mb + n);
                int ncam = 1;
                for (int q = 1; q < n; ++q) ncam += h->aff.hyp_cam[(size_t)mb[q]] != h->aff.hyp_cam[(size_t)mb[q - 1]];
                valid[g] = ncam >= 4;
            }
        });
        std::vector<int32_t> gstart(1, 0), memb;
        std::vector<size_t> gof;                                                // fitted[] slot of every cluster handed to the device
        memb.reserve((size_t)n_nodes);
        for (size_t g = 0; g < groups.size(); ++g) {
            if (!valid[g]) continue;
            const int l = groups[g];
            memb.insert(memb.end(), memb_tmp.begin() + lstart[(size_t)l], memb_tmp.begin() + lstart[(size_t)l + 1]);
            gstart.push_back((int32_t)memb.size());
            gof.push_back(g);
        }
        lap("  fit: member lists");
        int32_t* cnt = nullptr; double* segs = nullptr; int n_segs = 0;
        const double tneg[3] = { h->transf_tneg.x, h->transf_tneg.y, h->transf_tneg.z };
        // (hyp = null: the table l3d_affinity_fill uploaded in this finish is still on the device)
        const int rc = l3d_fit_clusters(h->ctx, gstart.data(), (int)gof.size(), memb.data(), nullptr, h->aff.hyp_cam.data(), (int)h->hyps.size(),
                                        h->transf_Rinv.m, h->transf_scale_inv, tneg, &cnt, &segs, &n_segs);
        if (rc) return h->fail(rc, std::string("line fit: ") + l3d_last_error(h->ctx));
        lap("  fit: device");
        h->fit_on_device = true;
        std::vector<size_t> soff(gof.size() + 1, 0);
        for (size_t v = 0; v < gof.size(); ++v) soff[v + 1] = soff[v] + (size_t)cnt[v];
        parallel_slices(gof.size(), finish_threads(), [&](size_t v0, size_t v1, unsigned) {
            for (size_t v = v0; v < v1; ++v) {
                if (cnt[v] == 0) continue;
                FinalLine& fl = fitted[gof[v]];
                for (size_t k = soff[v]; k < soff[v + 1]; ++k) {
                    const double* q = segs + 6 * k;
                    fl.segs3D.emplace_back(V3{ q[0], q[1], q[2] }, V3{ q[3], q[4], q[5] });
                }
                for (int32_t i = gstart[v]; i < gstart[v + 1]; ++i) fl.segs2D.push_back(h->hyps[(size_t)memb[(size_t)i]].src);
            }
        });
        l3d_free(cnt); l3d_free(segs);
    } else {
        std::atomic<size_t> next{ 0 };
        auto worker = [&]() {
            std::vector<Key> keys;
            std::vector<std::pair<Key, std::pair<V3, V3>>> t3;
            for (;;) {
                const size_t g0 = next.fetch_add(16, std::memory_order_relaxed);
                if (g0 >= groups.size()) break;
                for (size_t g = g0; g < std::min(groups.size(), g0 + 16); ++g) {
                    const int l = groups[g];
                    keys.clear();
                    for (int q = lstart[(size_t)l]; q < lstart[(size_t)l + 1]; ++q) keys.push_back(h->local2global[(size_t)lnodes[(size_t)q]]);
                    std::sort(keys.begin(), keys.end());
                    int ncam = 1;
                    for (size_t q = 1; q < keys.size(); ++q) ncam += kcam(keys[q]) != kcam(keys[q - 1]);
                    if (ncam < 4) continue;
                    t3.clear();
                    for (Key k : keys) {
                        const int bb = best_of(h, k);
                        if (bb < 0) continue;
                        t3.push_back({ k, { inverse_transform(h, h->hyps[(size_t)bb].P1), inverse_transform(h, h->hyps[(size_t)bb].P2) } });
                    }
                    FinalLine& fl = fitted[g];
                    align_cluster(t3, fl.segs3D);
                    if (fl.segs3D.empty()) continue;
                    for (auto& e : t3) fl.segs2D.push_back(e.first);
                }
            }
        };
        const unsigned ntf = (unsigned)std::max<size_t>(1, std::min<size_t>(finish_threads(), groups.size() / 64 + 1));
        l3d::on_threads(ntf, [&](unsigned) { worker(); });
    }
    for (FinalLine& fl : fitted) if (!fl.segs3D.empty()) h->result.push_back(std::move(fl));
    lap("line fit");
    h->t_cluster = now_s() - t1;
    return L3D_OK;
}

// The refinement of the result (l3d_refine_lines; l3d_refine.hpp), after whichever fit path built the list: members are every line's segs2D, their 2-D
// segments View::segs, cameras View::P and points the hypotheses' P1 / P2 -- all in the normalised frame transform_geometry left them in, which is better
// conditioned than the caller's; the emitted points go back through inverse_transform.  The member arrays are uploaded from the host (72 bytes per member).
int refine_input(L* h, RefineInput& in)
{
    const size_t nl = h->result.size(), nv = h->vlist.size(), nh = h->hyps.size();
    // the hypotheses' end points: on the host when greedy selection ran there, else the table the affinity fill left on the device
    std::vector<l3d_hypothesis> table;
    const bool host_points = !h->resident_products && !h->partitioned;
    if (!host_points && nl) {
        table.resize(nh + 1);
        const int rc = l3d::fetch_fill_hypotheses(h->ctx, (int)nh, table.data());
        if (rc) return h->fail(rc, std::string("refinement: ") + l3d_last_error(h->ctx));
    }
    in.cameras.assign(12 * nv + 1, 0.0);
    for (size_t i = 0; i < nv; ++i) memcpy(&in.cameras[12 * i], h->vlist[i]->P, 96);
    in.gstart.assign(nl + 1, 0);
    // (after a finish with the support on, a line's first members are those of the line fit: the ones the support added have no hypothesis)
    const bool extended = h->support_valid && h->support_per_line.size() == 4 * nl;
    auto members = [&](size_t l) { return extended ? (size_t)h->support_per_line[4 * l] : h->result[l].segs2D.size(); };
    for (size_t l = 0; l < nl; ++l) in.gstart[l + 1] = in.gstart[l] + (int32_t)members(l);
    const size_t nm = (size_t)in.gstart[nl];
    in.mcam.assign(nm + 1, 0); in.mseg.assign(4 * nm + 4, 0.0f); in.mpts.assign(6 * nm + 6, 0.0);
    std::vector<int32_t>& gstart = in.gstart; std::vector<int32_t>& mcam = in.mcam; std::vector<float>& mseg = in.mseg; std::vector<double>& mpts = in.mpts;
    std::atomic<int> bad{ 0 };
    parallel_slices(nl, finish_threads(), [&](size_t l0, size_t l1, unsigned) {
        for (size_t l = l0; l < l1; ++l) {
            size_t m = (size_t)gstart[l];
            for (size_t e = 0; e < members(l); ++e) {
                const Key k = h->result[l].segs2D[e];
                auto vt = h->views.find(kcam(k));
                // (the hypotheses are in key order: greedy selection numbers them view by view, segment by segment)
                auto hy = std::lower_bound(h->hyps.begin(), h->hyps.end(), k, [](const Hyp& a, Key b) { return a.src < b; });
                if (vt == h->views.end() || kseg(k) >= (uint32_t)vt->second.S() || hy == h->hyps.end() || hy->src != k) { bad.store(1, std::memory_order_relaxed); break; }
                mcam[m] = vt->second.index;
                memcpy(&mseg[4 * m], &vt->second.segs[(size_t)kseg(k) * 4], 16);
                double* q = &mpts[6 * m];
                if (host_points) { q[0] = hy->P1.x; q[1] = hy->P1.y; q[2] = hy->P1.z; q[3] = hy->P2.x; q[4] = hy->P2.y; q[5] = hy->P2.z; }
                else { const l3d_hypothesis& t = table[(size_t)(hy - h->hyps.begin())]; memcpy(q, t.P1, 24); memcpy(q + 3, t.P2, 24); }
                ++m;
            }
        }
    });
    if (bad.load()) return h->fail(L3D_ERR_INVALID, "refinement: a 2-D segment of the result has no view or no hypothesis");
    for (size_t i = 0; i < nv; ++i) if (h->vlist[i]->index != (int)i) return h->fail(L3D_ERR_INVALID, "refinement: views are not indexed in ascending id order");
    return L3D_OK;
}

int refine_result(L* h)
{
    h->refine_valid = false;
    h->ref_rms_before.clear(); h->ref_rms_after.clear(); h->ref_iterations.clear(); h->ref_status.clear();
    const size_t nl = h->result.size(), nv = h->vlist.size();
    const double t0 = now_s();
    if (nl == 0) { h->refine_valid = true; return L3D_OK; }
    RefineInput in;
    if (const int ri = refine_input(h, in)) return ri;
    const std::vector<int32_t>& gstart = in.gstart; const std::vector<int32_t>& mcam = in.mcam; const std::vector<float>& mseg = in.mseg; const std::vector<double>& mpts = in.mpts;
    const std::vector<double>& cameras = in.cameras;
    const size_t nm = (size_t)gstart[nl];
    l3d_refine_params prm;
    prm.max_iterations = h->refine_max_iterations; prm.pad = 0; prm.huber_px = h->refine_huber_px;
    std::vector<double> line(6 * nl);
    h->ref_rms_before.resize(nl); h->ref_rms_after.resize(nl); h->ref_iterations.resize(nl); h->ref_status.resize(nl);
    int32_t* cnt = nullptr; double* segs = nullptr; int n_segs = 0;
    const int rc = l3d_refine_lines(h->ctx, gstart.data(), (int)nl, mcam.data(), mseg.data(), mpts.data(), cameras.data(), (int)nv, &prm, line.data(), h->ref_rms_before.data(),
                                    h->ref_rms_after.data(), h->ref_iterations.data(), h->ref_status.data(), &cnt, &segs, &n_segs);
    if (rc) return h->fail(rc, std::string("refinement: ") + l3d_last_error(h->ctx));
    size_t at = 0;
    for (size_t l = 0; l < nl; ++l) {
        if (cnt[l] == 0) { if (h->ref_status[l] != 2) h->ref_status[l] = 3; continue; }      // (nothing emitted: the line keeps its unrefined segments)
        FinalLine& fl = h->result[l];
        fl.segs3D.clear();
        for (int k = 0; k < cnt[l]; ++k, ++at) {
            const double* q = segs + 6 * at;
            fl.segs3D.emplace_back(inverse_transform(h, V3{ q[0], q[1], q[2] }), inverse_transform(h, V3{ q[3], q[4], q[5] }));
        }
    }
    l3d_free(cnt); l3d_free(segs);
    h->refine_valid = true;
    if (hopt(h).timing) fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%zu lines, %zu members)\n", "refinement", (now_s() - t0) * 1e3, nl, nm);
    return L3D_OK;
}

// The support of the result's lines ("SUPPORT OF 3-D LINES" in include/line3d_amd.h, on the object): the 3-D segments of the result in
// l3d_line3d_get_result's order against every view's segments, the view's camera as it was added; one l3d_support_lines call on the owner's context.  A
// (view, segment) that several 3-D segments of one line reach is reported once, with the smallest (dist, seg3d).
int support_gather(L* owner, const l3d_support_params& prm, std::vector<l3d_line_support>& rec, std::vector<int64_t>& line_start, std::vector<int32_t>& line_views, int64_t* counts)
{
    for (int k = 0; k < 4; ++k) counts[k] = 0;
    if (!owner->result_valid) return owner->fail(L3D_ERR_INVALID, "gather_support: no result yet (compute3Dmodel first)");
    if (!owner->ctx) return owner->fail(L3D_ERR_INVALID, "gather_support: no device context");
    const size_t nl = owner->result.size(), nv = owner->views.size();
    std::vector<double> seg3d;
    std::vector<int32_t> line_of;
    for (size_t li = 0; li < nl; ++li)
        for (auto& s : owner->result[li].segs3D) {
            const double v[6] = { s.first.x, s.first.y, s.first.z, s.second.x, s.second.y, s.second.z };
            seg3d.insert(seg3d.end(), v, v + 6);
            line_of.push_back((int32_t)li);
        }
    // the views in ascending id: cameras, segments one after the other, and per segment the line it is a member of (-1: none; several: the first, and a mark)
    std::vector<l3d_camera> cams;
    std::vector<uint32_t> ids;
    std::vector<int64_t> seg_start(1, 0);
    std::vector<float> segs;
    std::map<uint32_t, size_t> cam_of;
    for (auto& kv : owner->views) {
        cam_of[kv.first] = cams.size();
        cams.push_back(camera_as_added(kv.second));
        ids.push_back(kv.first);
        segs.insert(segs.end(), kv.second.segs.begin(), kv.second.segs.end());
        seg_start.push_back((int64_t)(segs.size() / 4));
    }
    const size_t T = (size_t)seg_start[nv];
    std::vector<int32_t> member_line(T, -1);
    std::vector<unsigned char> several(T, 0);
    size_t n_members = 0;
    for (size_t li = 0; li < nl; ++li)
        for (Key key : owner->result[li].segs2D) {
            auto ct = cam_of.find(kcam(key));
            if (ct == cam_of.end() || (int64_t)kseg(key) >= seg_start[ct->second + 1] - seg_start[ct->second]) return owner->fail(L3D_ERR_INVALID, "gather_support: a 2-D segment of the result has no view");
            const size_t at = (size_t)seg_start[ct->second] + kseg(key);
            if (member_line[at] < 0) member_line[at] = (int32_t)li; else if (member_line[at] != (int32_t)li) several[at] = 1;
            ++n_members;
        }
    std::vector<int32_t> best(T + 1, -1);
    std::vector<int64_t> cam_start(nv + 1, 0);
    l3d_support_record* raw = nullptr;
    int64_t c4[4];
    const int rc = l3d_support_lines(owner->ctx, seg3d.data(), (int)line_of.size(), cams.data(), (int)nv, segs.data(), seg_start.data(), &prm, &raw, cam_start.data(), best.data(), c4);
    if (rc != L3D_OK) return owner->fail(rc, std::string("gather_support: ") + l3d_last_error(owner->ctx));
    // one entry per (line, view, segment): the smallest (dist, seg3d).  The records come camera-major and, within a camera, by ascending seg3d -- which is
    // by ascending line, the 3-D segments being numbered line after line: filing them into their lines' buckets camera after camera orders them by
    // (line, view); only a line's few records of one view are left to sort, by (segment, dist, seg3d)
    struct E { int32_t line; uint32_t cam; l3d_support_record r; };
    std::vector<size_t> bucket(nl + 1, 0);
    for (int64_t r = 0; r < cam_start[nv]; ++r) ++bucket[(size_t)line_of[(size_t)raw[r].seg3d] + 1];
    for (size_t li = 0; li < nl; ++li) bucket[li + 1] += bucket[li];
    std::vector<E> all((size_t)cam_start[nv]);
    {
        std::vector<size_t> at(bucket.begin(), bucket.end() - 1);
        for (size_t c = 0; c < nv; ++c)
            for (int64_t r = cam_start[c]; r < cam_start[c + 1]; ++r) { const int32_t li = line_of[(size_t)raw[r].seg3d]; all[at[(size_t)li]++] = E{ li, (uint32_t)c, raw[r] }; }
    }
    l3d_free(raw);
    for (size_t i = 0; i < all.size();) {
        size_t j = i + 1;
        while (j < all.size() && all[j].line == all[i].line && all[j].cam == all[i].cam) ++j;
        if (j - i > 1)
            std::sort(all.begin() + (ptrdiff_t)i, all.begin() + (ptrdiff_t)j, [](const E& a, const E& b) {
                if (a.r.seg2d != b.r.seg2d) return a.r.seg2d < b.r.seg2d;
                if (a.r.dist != b.r.dist) return a.r.dist < b.r.dist;
                return a.r.seg3d < b.r.seg3d;
            });
        i = j;
    }
    rec.clear();
    line_start.assign(nl + 1, 0);
    line_views.assign(2 * nl, 0);
    std::vector<unsigned char> on_a_line(T, 0);
    int64_t found = 0;
    int32_t prev_line = -1;
    uint32_t prev_cam = 0;
    for (size_t i = 0; i < all.size(); ++i) {
        const E& e = all[i];
        if (i && all[i - 1].line == e.line && all[i - 1].cam == e.cam && all[i - 1].r.seg2d == e.r.seg2d) continue;
        const size_t at = (size_t)seg_start[e.cam] + (size_t)e.r.seg2d;
        bool mine = member_line[at] == e.line;
        if (!mine && several[at]) { const std::vector<Key>& m = owner->result[(size_t)e.line].segs2D; mine = std::find(m.begin(), m.end(), mk(ids[e.cam], (uint32_t)e.r.seg2d)) != m.end(); }
        const bool other = member_line[at] >= 0 && (member_line[at] != e.line || several[at]);
        const bool holds_best = best[at] >= 0 && line_of[(size_t)best[at]] == e.line;
        l3d_line_support o;
        o.view_id = ids[e.cam]; o.seg = (uint32_t)e.r.seg2d; o.seg3d = e.r.seg3d; o.dist = e.r.dist; o.overlap = e.r.overlap;
        o.flags = (mine ? 1u : 0u) | (other ? 2u : 0u) | (holds_best ? 4u : 0u);
        if (e.line != prev_line || e.cam != prev_cam) ++line_views[2 * (size_t)e.line + 1];
        prev_line = e.line; prev_cam = e.cam;
        rec.push_back(o);
        ++line_start[(size_t)e.line + 1];
        found += mine ? 1 : 0;
        on_a_line[at] = 1;
    }
    for (size_t li = 0; li < nl; ++li) {
        line_start[li + 1] += line_start[li];
        std::vector<uint32_t> mv;
        for (Key key : owner->result[li].segs2D) mv.push_back(kcam(key));
        std::sort(mv.begin(), mv.end());
        line_views[2 * li] = (int32_t)(std::unique(mv.begin(), mv.end()) - mv.begin());
    }
    counts[0] = (int64_t)rec.size(); counts[1] = found; counts[2] = (int64_t)n_members - found;
    for (size_t at = 0; at < T; ++at) counts[3] += on_a_line[at] && member_line[at] < 0 ? 1 : 0;
    return L3D_OK;
}

// The gather as the last step of a finish (l3d_line3d_set_support), after the line fit, the merging and the refinement.  It EXTENDS the member lists: a
// record joins its line's segs2D iff the line holds the segment's best row (bit 2) and the segment is a member of no line (bits 0 and 1 clear), so a 2-D
// segment stays in at most one line; new members go behind the old ones in (view id, segment) order; the 3-D segments are untouched.
int support_result(L* h)
{
    h->support_valid = false;
    const double t0 = now_s();
    l3d_support_params prm;
    prm.dist_px = h->support_dist_px; prm.cos_min = std::cos(h->support_angle_deg * 3.14159265358979323846 / 180.0); prm.min_overlap = h->support_min_overlap;
    prm.near_z = 1e-6; prm.margin = h->support_dist_px;
    std::vector<l3d_line_support> rec;
    std::vector<int64_t> start;
    std::vector<int32_t> views;
    h->result_valid = true;                                            // (the gather reads the result this finish has just built)
    if (const int rc = support_gather(h, prm, rec, start, views, h->support_counts)) { h->result_valid = false; return rc; }
    const size_t nl = h->result.size();
    h->support_per_line.assign(4 * nl, 0);
    size_t added = 0;
    for (size_t li = 0; li < nl; ++li) {
        FinalLine& fl = h->result[li];
        std::vector<uint32_t> seen;
        for (Key key : fl.segs2D) seen.push_back(kcam(key));
        h->support_per_line[4 * li] = (int32_t)fl.segs2D.size();
        h->support_per_line[4 * li + 2] = views[2 * li];
        for (int64_t r = start[li]; r < start[li + 1]; ++r)
            if (rec[(size_t)r].flags == 4u) { fl.segs2D.push_back(mk(rec[(size_t)r].view_id, rec[(size_t)r].seg)); seen.push_back(rec[(size_t)r].view_id); ++added; }
        h->support_per_line[4 * li + 1] = (int32_t)fl.segs2D.size() - h->support_per_line[4 * li];
        std::sort(seen.begin(), seen.end());
        h->support_per_line[4 * li + 3] = (int32_t)(std::unique(seen.begin(), seen.end()) - seen.begin());
    }
    h->support_valid = true;
    if (hopt(h).timing) fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%zu lines, %lld records, %zu members added)\n", "support", (now_s() - t0) * 1e3, nl, (long long)h->support_counts[0], added);
    return L3D_OK;
}

// SIGMA of a line (step 1 of the merging; the junctions share it): the mean over the members, in their stored order, of z / f -- z = R[2] . M + t[2] at
// M = (P + Q) / 2, f = (|K00| + |K11|) / 2 of the member's view as it was added.  Members with z <= 0 or a term that is not finite are skipped; none
// left: 0.  missing: a member has no view
static double line_sigma(const L* h, const FinalLine& fl, bool& missing)
{
    const V3 P = fl.segs3D.front().first, Q = fl.segs3D.back().second;
    const double M[3] = { (P.x + Q.x) / 2.0, (P.y + Q.y) / 2.0, (P.z + Q.z) / 2.0 };
    double sum = 0.0;
    int cnt = 0;
    for (Key k : fl.segs2D) {
        auto vt = h->views.find(kcam(k));
        if (vt == h->views.end()) { missing = true; return 0.0; }
        const View& v = vt->second;
        const double z = ((v.R_added(2, 0) * M[0] + v.R_added(2, 1) * M[1]) + v.R_added(2, 2) * M[2]) + v.t_added.z;
        const double f = (std::fabs(v.K(0, 0)) + std::fabs(v.K(1, 1))) / 2.0;
        const double r = z / f;
        if (!(z > 0.0) || !(std::fabs(r) <= 1.7976931348623157e308)) continue;
        sum = sum + r; ++cnt;
    }
    return cnt ? sum / (double)cnt : 0.0;
}

// The duplicate lines of the result merged ("MERGING DUPLICATE LINES" in include/line3d_amd.h, on the object), after whichever fit path built the list and
// before the refinement.  Per round: a line's P is the start of its first 3-D segment, Q the end of its last, its tolerance dist_px times the mean of
// z / f over its members' views as they were added; l3d_merge_lines groups the lines; every group of two or more is refitted from the union of its
// members, in key order, by the fit path that built the result, takes the position of its lowest-index line and removes the others -- unless the
// refit emits nothing: then the group's lines stay as they were.  Rounds until one finds no pair, or max_rounds.
int merge_result(L* h)
{
    h->merge_valid = false;
    h->merge_final_index.clear(); h->merge_n_sources.clear();
    int32_t* mc = h->merge_counts;
    for (int k = 0; k < 8; ++k) mc[k] = 0;
    const double t0 = now_s();
    double t_lap = t0, t_table = 0.0, t_search = 0.0, t_members = 0.0, t_refit = 0.0, t_list = 0.0;
    const auto lap = [&t_lap](double& acc) { const double t = now_s(); acc += t - t_lap; t_lap = t; };
    const size_t n0 = h->result.size();
    mc[0] = (int32_t)n0;
    std::vector<std::vector<int32_t>> sources(n0);                              // per current line: the lines before merging it was made of
    for (size_t k = 0; k < n0; ++k) sources[k].push_back((int32_t)k);
    l3d_merge_params prm;
    prm.cos_min = std::cos(h->merge_angle_deg * 3.14159265358979323846 / 180.0);
    prm.max_gap = h->merge_max_gap;
    for (int round = 0; round < h->merge_max_rounds && !h->result.empty(); ++round) {
        const size_t n = h->result.size();
        std::vector<double> lines(6 * n), tol(n);
        std::atomic<int> bad{ 0 };
        parallel_slices(n, finish_threads(), [&](size_t l0, size_t l1, unsigned) {
            for (size_t l = l0; l < l1; ++l) {
                const FinalLine& fl = h->result[l];
                const V3 P = fl.segs3D.front().first, Q = fl.segs3D.back().second;
                double* q = &lines[6 * l];
                q[0] = P.x; q[1] = P.y; q[2] = P.z; q[3] = Q.x; q[4] = Q.y; q[5] = Q.z;
                bool missing = false;
                const double sigma = line_sigma(h, fl, missing);
                if (missing) { bad.store(1, std::memory_order_relaxed); continue; }
                tol[l] = h->merge_dist_px * sigma;
                if (!(tol[l] >= 0.0)) tol[l] = 0.0;                               // (dist_px 0 times an overflowed mean)
            }
        });
        if (bad.load()) return h->fail(L3D_ERR_INVALID, "merging: a 2-D segment of the result has no view");
        lap(t_table);
        std::vector<int32_t> group(n);
        int32_t* pairs = nullptr; int n_pairs = 0; int32_t c4[4];
        const int rc = l3d_merge_lines(h->ctx, lines.data(), tol.data(), (int)n, &prm, group.data(), &pairs, &n_pairs, c4);
        if (rc) return h->fail(rc, std::string("merging: ") + l3d_last_error(h->ctx));
        l3d_free(pairs);
        lap(t_search);
        mc[2] = round + 1;
        if (round == 0) mc[3] = n_pairs;
        mc[5] += c4[2];
        if (n_pairs == 0) break;
        // ---- the groups of two or more, in the order of their lowest index: members in key order
        std::vector<int32_t> size(n, 0), gslot(n, -1);
        for (size_t k = 0; k < n; ++k) ++size[(size_t)group[k]];
        std::vector<size_t> gof;                                                // position of every group handed to the refit
        for (size_t k = 0; k < n; ++k) if (size[k] >= 2) { gslot[k] = (int32_t)gof.size(); gof.push_back(k); }
        std::vector<std::vector<Key>> keys(gof.size());
        for (size_t k = 0; k < n; ++k) if (gslot[(size_t)group[k]] >= 0) { auto& d = keys[(size_t)gslot[(size_t)group[k]]]; d.insert(d.end(), h->result[k].segs2D.begin(), h->result[k].segs2D.end()); }
        for (auto& d : keys) std::sort(d.begin(), d.end());
        std::vector<std::vector<std::pair<V3, V3>>> fitted(gof.size());
        lap(t_members);
        if (h->fit_on_device) {
            std::vector<int32_t> gstart(1, 0), memb;
            for (auto& d : keys) {
                for (Key k : d) {
                    auto hy = std::lower_bound(h->hyps.begin(), h->hyps.end(), k, [](const Hyp& a, Key b) { return a.src < b; });
                    if (hy == h->hyps.end() || hy->src != k) return h->fail(L3D_ERR_INVALID, "merging: a 2-D segment of the result has no hypothesis");
                    memb.push_back((int32_t)(hy - h->hyps.begin()));
                }
                gstart.push_back((int32_t)memb.size());
            }
            int32_t* cnt = nullptr; double* segs = nullptr; int n_segs = 0;
            const double tneg[3] = { h->transf_tneg.x, h->transf_tneg.y, h->transf_tneg.z };
            const int rf = l3d_fit_clusters(h->ctx, gstart.data(), (int)gof.size(), memb.data(), nullptr, h->aff.hyp_cam.data(), (int)h->hyps.size(), h->transf_Rinv.m,
                                            h->transf_scale_inv, tneg, &cnt, &segs, &n_segs);
            if (rf) return h->fail(rf, std::string("merging: line fit: ") + l3d_last_error(h->ctx));
            size_t at = 0;
            for (size_t g = 0; g < gof.size(); ++g)
                for (int k = 0; k < cnt[g]; ++k, ++at) { const double* q = segs + 6 * at; fitted[g].emplace_back(V3{ q[0], q[1], q[2] }, V3{ q[3], q[4], q[5] }); }
            l3d_free(cnt); l3d_free(segs);
        } else {
            parallel_slices(gof.size(), finish_threads(), [&](size_t g0, size_t g1, unsigned) {
                std::vector<std::pair<Key, std::pair<V3, V3>>> t3;
                for (size_t g = g0; g < g1; ++g) {
                    t3.clear();
                    for (Key k : keys[g]) {
                        const int bb = best_of(h, k);
                        if (bb < 0) continue;
                        t3.push_back({ k, { inverse_transform(h, h->hyps[(size_t)bb].P1), inverse_transform(h, h->hyps[(size_t)bb].P2) } });
                    }
                    align_cluster(t3, fitted[g]);
                }
            });
        }
        lap(t_refit);
        // ---- the new list: a merged line at the position of its lowest-index line, everything else in its order
        std::vector<FinalLine> out;
        std::vector<std::vector<int32_t>> out_src;
        out.reserve(n); out_src.reserve(n);
        std::vector<char> emitted(gof.size());
        for (size_t g = 0; g < gof.size(); ++g) emitted[g] = !fitted[g].empty();
        std::vector<std::vector<int32_t>> gsrc(gof.size());                     // per group: the lines before merging of all its lines
        for (size_t k = 0; k < n; ++k) { const int32_t s = gslot[(size_t)group[k]]; if (s >= 0 && emitted[(size_t)s]) gsrc[(size_t)s].insert(gsrc[(size_t)s].end(), sources[k].begin(), sources[k].end()); }
        for (size_t k = 0; k < n; ++k) {
            const int32_t s = gslot[(size_t)group[k]];
            if (s >= 0 && emitted[(size_t)s]) {
                if ((size_t)group[k] != k) continue;                            // merged into the line at position group[k]
                FinalLine fl;
                fl.segs2D = std::move(keys[(size_t)s]);
                fl.segs3D = std::move(fitted[(size_t)s]);
                std::sort(gsrc[(size_t)s].begin(), gsrc[(size_t)s].end());
                out.push_back(std::move(fl)); out_src.push_back(std::move(gsrc[(size_t)s]));
                ++mc[4];
                continue;
            }
            if (s >= 0 && (size_t)group[k] == k) ++mc[6];                       // the refit emitted nothing: the group's lines stay as they were
            out.push_back(std::move(h->result[k])); out_src.push_back(std::move(sources[k]));
        }
        h->result.swap(out); sources.swap(out_src);
        lap(t_list);
    }
    mc[1] = (int32_t)h->result.size();
    h->merge_final_index.assign(n0, 0);
    h->merge_n_sources.resize(h->result.size());
    for (size_t k = 0; k < sources.size(); ++k) {
        h->merge_n_sources[k] = (int32_t)sources[k].size();
        for (int32_t s : sources[k]) h->merge_final_index[(size_t)s] = (int32_t)k;
    }
    h->merge_valid = true;
    if (hopt(h).timing)
        fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%d -> %d lines, %d rounds; table %.2f, search %.2f, member lists %.2f, refit %.2f, new list %.2f ms)\n", "merging",
                (now_s() - t0) * 1e3, mc[0], mc[1], mc[2], t_table * 1e3, t_search * 1e3, t_members * 1e3, t_refit * 1e3, t_list * 1e3);
    return L3D_OK;
}

// The junctions of the result ("JUNCTIONS OF 3-D LINES" in include/line3d_amd.h, on the object), after the merging and the refinement and before the
// support gather.  A line's P is the start of its first 3-D segment, Q the end of its last; tol = dist_px x sigma (line_sigma, the merging's),
// ext = min(ext_px x sigma, max_ext_rel x L) with L = sqrt((Q - P) . (Q - P)); one l3d_junction_lines call without crossings.  With snap, an end that
// stays in a vertex moves to the foot of the vertex on the line's own axis, P + ((X - P) . d) d, an attached end to its own closest point P + s d; P
// and d = (Q - P) / L are those of the table, taken before any move.  The P end is moved first, then the Q end; a move after which
// (far end - new end) . (far end - old end) > 0 no longer holds for the 3-D segment it ends -- the segment would turn round or vanish -- is skipped
void junction_geometry(const FinalLine& fl, double* q)
{
    const V3 P = fl.segs3D.front().first, Q = fl.segs3D.back().second;
    q[0] = P.x; q[1] = P.y; q[2] = P.z; q[3] = Q.x; q[4] = Q.y; q[5] = Q.z;
}

int junction_result(L* h, JunctionHandOn* hand)
{
    const bool record = h->junc_on;                        // (off: the search runs for the planes alone)
    h->junc_valid = false;
    h->junc_vertices.clear(); h->junc_per_line.clear();
    for (int k = 0; k < 10; ++k) h->junc_counts[k] = 0;
    if (hand) { hand->sigma.assign(h->result.size(), 0.0); hand->seeds.clear(); }
    const double t0 = now_s();
    const size_t n = h->result.size();
    std::vector<double> lines(6 * n + 6), tol(n + 1), ext(n + 1);
    std::atomic<int> bad{ 0 };
    parallel_slices(n, finish_threads(), [&](size_t l0, size_t l1, unsigned) {
        for (size_t l = l0; l < l1; ++l) {
            const FinalLine& fl = h->result[l];
            double* q = &lines[6 * l];
            junction_geometry(fl, q);
            bool missing = false;
            const double sigma = line_sigma(h, fl, missing);
            if (missing) { bad.store(1, std::memory_order_relaxed); continue; }
            if (hand) hand->sigma[l] = sigma;
            const double v[3] = { q[3] - q[0], q[4] - q[1], q[5] - q[2] };
            const double len = std::sqrt(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]));
            const double a = h->junc_ext_px * sigma, b = h->junc_max_ext_rel * len;
            tol[l] = h->junc_dist_px * sigma;
            ext[l] = b < a ? b : a;
            if (!(tol[l] >= 0.0)) tol[l] = 0.0;                                   // (0 times an overflowed mean)
            if (!(ext[l] >= 0.0)) ext[l] = 0.0;
        }
    });
    if (bad.load()) return h->fail(L3D_ERR_INVALID, "junctions: a 2-D segment of the result has no view");
    l3d_junction_params prm;
    prm.cos_max = std::cos(h->junc_angle_min_deg * 3.14159265358979323846 / 180.0);
    prm.crossings = 0; prm.pad = 0;
    std::vector<int32_t> node_vertex(2 * n + 2), node_attach(2 * n + 2);
    l3d_junction_record* rec = nullptr; l3d_junction_vertex* vert = nullptr; int n_rec = 0, n_vert = 0;
    int32_t counts[8];
    const int rc = l3d_junction_lines(h->ctx, lines.data(), tol.data(), ext.data(), (int)n, &prm, &rec, &n_rec, node_vertex.data(), &vert, &n_vert, node_attach.data(), counts);
    if (rc) return h->fail(rc, std::string("junctions: ") + l3d_last_error(h->ctx));
    if (hand)
        for (int k = 0; k < n_rec; ++k)
            if (rec[k].where_i != L3D_JUNCTION_INTERIOR || rec[k].where_j != L3D_JUNCTION_INTERIOR) { hand->seeds.push_back(rec[k].i); hand->seeds.push_back(rec[k].j); }
    if (!record) {                                         // the vertices are discarded: get_junctions still refuses
        l3d_free(rec); l3d_free(vert);
        if (hopt(h).timing) fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%zu lines, %d records)\n", "junction search (planes)", (now_s() - t0) * 1e3, n, n_rec);
        return L3D_OK;
    }
    for (int k = 0; k < 8; ++k) h->junc_counts[k] = counts[k];
    h->junc_vertices.assign(vert, vert + n_vert);
    h->junc_per_line.assign(4 * n, -1);
    for (size_t l = 0; l < n; ++l)
        for (int e = 0; e < 2; ++e) {
            const size_t node = 2 * l + (size_t)e;
            h->junc_per_line[4 * l + (size_t)e] = node_vertex[node];
            if (node_attach[node] >= 0) { const l3d_junction_record& r = rec[node_attach[node]]; h->junc_per_line[4 * l + 2 + (size_t)e] = (size_t)r.i == l ? r.j : r.i; }
        }
    if (h->junc_snap) {
        for (size_t l = 0; l < n; ++l) {
            const double* q = &lines[6 * l];
            const double v[3] = { q[3] - q[0], q[4] - q[1], q[5] - q[2] };
            const double len = std::sqrt(((v[0] * v[0]) + (v[1] * v[1])) + (v[2] * v[2]));
            const double d[3] = { v[0] / len, v[1] / len, v[2] / len };
            for (int e = 0; e < 2; ++e) {
                const size_t node = 2 * l + (size_t)e;
                double s;
                if (node_vertex[node] >= 0) {
                    const double* X = vert[node_vertex[node]].X;
                    const double w[3] = { X[0] - q[0], X[1] - q[1], X[2] - q[2] };
                    s = ((w[0] * d[0]) + (w[1] * d[1])) + (w[2] * d[2]);
                } else if (node_attach[node] >= 0) {
                    const l3d_junction_record& r = rec[node_attach[node]];
                    s = (size_t)r.i == l ? r.s : r.t;
                } else continue;
                const V3 to = { q[0] + (s * d[0]), q[1] + (s * d[1]), q[2] + (s * d[2]) };
                std::pair<V3, V3>& seg = e == 0 ? h->result[l].segs3D.front() : h->result[l].segs3D.back();
                const V3 far = e == 0 ? seg.second : seg.first, old = e == 0 ? seg.first : seg.second;
                const V3 a = far - to, b = far - old;
                if (!((((a.x * b.x) + (a.y * b.y)) + (a.z * b.z)) > 0.0)) { ++h->junc_counts[9]; continue; }
                (e == 0 ? seg.first : seg.second) = to;
                ++h->junc_counts[8];
            }
        }
    }
    l3d_free(rec); l3d_free(vert);
    h->junc_valid = true;
    if (hopt(h).timing)
        fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%zu lines, %d records, %d vertices, %d ends attached, %d ends moved)\n", "junctions", (now_s() - t0) * 1e3, n, n_rec, n_vert,
                h->junc_counts[7], h->junc_counts[8]);
    return L3D_OK;
}

// The planes of the result ("PLANES OF 3-D LINES" in include/line3d_amd.h, on the object), after the junctions (and their snap) and before the support
// gather.  A line's P is the start of its first 3-D segment, Q the end of its last, as the junctions left them; tol = dist_px x the sigma the junction
// search computed; cos_max is the junctions' own, cos_min = cos(angle_deg pi / 180); the seeds are the L and T records of that search, in record order
int plane_result(L* h, const JunctionHandOn& hand)
{
    h->plane_valid = false;
    h->plane_list.clear(); h->plane_members.clear(); h->plane_per_line.clear();
    for (int k = 0; k < 8; ++k) h->plane_counts[k] = 0;
    const double t0 = now_s();
    const size_t n = h->result.size();
    if (hand.sigma.size() != n) return h->fail(L3D_ERR_INVALID, "planes: the junction search did not run on this result");
    std::vector<double> lines(6 * n + 6), tol(n + 1);
    for (size_t l = 0; l < n; ++l) {
        junction_geometry(h->result[l], &lines[6 * l]);
        tol[l] = h->plane_dist_px * hand.sigma[l];
        if (!(tol[l] >= 0.0)) tol[l] = 0.0;                                       // (0 times an overflowed mean)
    }
    l3d_plane_params prm;
    prm.cos_max = std::cos(h->junc_angle_min_deg * 3.14159265358979323846 / 180.0);
    prm.cos_min = std::cos(h->plane_angle_deg * 3.14159265358979323846 / 180.0);
    prm.min_lines = h->plane_min_lines; prm.pad = 0;
    const int m = (int)(hand.seeds.size() / 2);
    std::vector<int32_t> hyp_plane((size_t)m + 1);
    l3d_plane* pl = nullptr; l3d_plane_member* mem = nullptr; int n_pl = 0, n_mem = 0;
    const int rc = l3d_plane_lines(h->ctx, lines.data(), tol.data(), (int)n, hand.seeds.data(), m, &prm, &pl, &n_pl, &mem, &n_mem, hyp_plane.data(), h->plane_counts);
    if (rc) return h->fail(rc, std::string("planes: ") + l3d_last_error(h->ctx));
    h->plane_list.assign(pl, pl + n_pl);
    h->plane_members.assign(mem, mem + n_mem);
    h->plane_per_line.assign(n, 0);
    for (int k = 0; k < n_mem; ++k) ++h->plane_per_line[(size_t)mem[k].line];
    l3d_free(pl); l3d_free(mem);
    h->plane_valid = true;
    if (hopt(h).timing)
        fprintf(stderr, "[l3d finish] %-28s %8.2f ms (%zu lines, %d seeds, %d planes, %d member records)\n", "planes", (now_s() - t0) * 1e3, n, m, n_pl, n_mem);
    return L3D_OK;
}

}  // namespace l3dh
