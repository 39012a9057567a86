/*
 * line3d_amd.h -- C ABI of the MI355X-native Line3D matching / affinity hot path.
 *
 * Drop-in boundary: these entry points are what a Line3D build binds instead of the three
 * functions of the reference's device seam (cudawrapper.h:49-75) -- plain pointers and sizes,
 * no C++ containers, no torch types.  INTEGRATION.md shows the ~80-line cudawrapper
 * replacement that forwards the reference's DataArray/std::list arguments to these calls so
 * that line3D.cc / segments.h link unchanged.
 *
 * Conventions: every function returns L3D_OK (0) or an error code; l3d_last_error(ctx) gives
 * the message (the reference prints CUDA errors and carries on, dataArray.h:153-156; here they
 * are reported).  All matrices are row-major float32 unless stated.  Output arrays marked
 * "callee-allocated" are released with l3d_free().  A context owns one GPU, one HIP stream and
 * grow-only device arenas; it is single-caller like the reference (global texture references,
 * cudawrapper.cu:5-10) but several contexts may coexist.
 */
#ifndef LINE3D_AMD_H
#define LINE3D_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L3D_OK 0
#define L3D_ERR_INVALID 1
#define L3D_ERR_HIP 2
#define L3D_ERR_NOMEM 3
#define L3D_ERR_NODEVICE 4
#define L3D_ERR_UNSUPPORTED 5

/* cudawrapper.h:35,43-46 / commons.h:42-66 */
#define L3D_RDD_MAX_ITER 10
#define L3D_DEF_COLLINEARITY_S 2.0f

typedef struct l3d_ctx l3d_ctx;

/* L3DMatchingPair, sparsematrix.h:37-65 (active_ is always true on this path and is dropped) */
typedef struct l3d_match {
    uint32_t segID1;   /* segment in the source view */
    uint32_t camID2;   /* neighbour: LOCAL index on input, GLOBAL view id on output (cudawrapper.cu:1103) */
    uint32_t segID2;   /* segment in the neighbour */
    float depths[4];   /* src p1, src p2, tgt q1, tgt q2 (cudawrapper.cu:594-601) */
    float confidence;
} l3d_match;

/* CLEdge, clustering.h:57-61 */
typedef struct l3d_edge {
    int32_t i, j;
    float w;
} l3d_edge;

/* L3DSegment3D (commons.h:69-78) + the three per-view scalars similarity_coll3D reads
 * (view.cc:353-377): one hypothesis handed to l3d_similarity_coll3D_batch */
typedef struct l3d_hypothesis {
    double P1[3], P2[3], dir[3];
    float depth_p1, depth_p2;
    float k_lower, k_upper, median_depth;
    uint32_t pad;
} l3d_hypothesis;

int l3d_ctx_create(int device, l3d_ctx** ctx);
void l3d_ctx_destroy(l3d_ctx* ctx);
const char* l3d_last_error(const l3d_ctx* ctx);
void l3d_free(void* p);

/* Replaces compute_collinearity (cudawrapper.h:49-51, K_collinearity cudawrapper.cu:476-535)
 * together with the host scan of the dense S x S relation in the L3DSegments constructor
 * (segments.h:73-98): returns the non-zero upper-triangle entries (i < j, ascending (i,j)),
 * i.e. exactly what the constructor inserts into segment2collinearities_ (both directions).
 * segments: n_segments x 4 (p1x,p1y,p2x,p2y).  Outputs callee-allocated. */
int l3d_compute_collinearity(l3d_ctx* ctx, const float* segments, int n_segments, float collin_s,
                             int32_t** out_i, int32_t** out_j, float** out_w, int* out_n);
/* The same for several segment sets at once (all views of a scene): no host round trip per set.  The triplets of set v are
 * entries [set_start[v], set_start[v+1]) of the concatenated outputs (callee-allocated; set_start: n_sets + 1, caller's). */
int l3d_compute_collinearity_batch(l3d_ctx* ctx, const float* const* segments, const int* n_segments, int n_sets, float collin_s,
                                   int32_t** out_i, int32_t** out_j, float** out_w, int* set_start);

/* Replaces compute_pairwise_matches (cudawrapper.h:54-70, cudawrapper.cu:858-1128):
 * K_pairwise_matches for every neighbour in to_be_matched, selection of pairs with four
 * positive depths, (segment, camera, target) ordering, K_verify_matches over the union with the
 * already existing (reverse) matches, best-hypothesis median depth, and the conf > 1 filter.
 *
 *   src_segs      S_src x 4            source view segments            (tex_segments)
 *   RtKinv_src    3 x 3, C_src 3       source camera                   (line3D.cc:787-803)
 *   tgt_segs      sum(S_n) x 4         all neighbours' segments        (tex_segments_f4, line3D.cc:770-784)
 *   offsets       N x (start,count)    into tgt_segs                   (line3D.cc:779)
 *   F, RtKinv     N x 3 x 3; centers N x 3; P N x 3 x 4              (line3D.cc:739-763)
 *   to_be_matched n_tbm local neighbour indices                        (line3D.cc:732-736)
 *   in_matches    existing matches, camID2 = LOCAL index               (view.cc:200-224)
 *   local2global  N global view ids                                    (line3D.cc:729)
 *   seg_begin/seg_end  source-segment range to process ([0,S_src) for the whole view); the
 *                 verification of a source segment only reads candidates of that segment, so a
 *                 range is exact -- this is what the multi-GPU sharding uses.
 * Outputs: *out_matches (callee-allocated, sorted (segID1, local camera, segID2), camID2 GLOBAL,
 * confidence already divided by 2, cudawrapper.cu:1089-1110), *out_n, *median_depth
 * (cudawrapper.cu:1066-1076; untouched when nothing is verified), and, if non-NULL,
 * *out_best_depths (callee-allocated 2*(*out_n_best) floats: the depth pairs entering the median,
 * in segment order) so that sharded callers can merge medians exactly.
 * With n_tbm == 0 the reference returns immediately (cudawrapper.cu:877-878): the output is the
 * input list unchanged (LOCAL camera ids, confidence 0) and *median_depth is left alone. */
int l3d_compute_pairwise_matches(l3d_ctx* ctx,
                                 const float* src_segs, int S_src, const float* RtKinv_src, const float* C_src,
                                 const float* tgt_segs, const int32_t* offsets, int N,
                                 const float* F, const float* RtKinv, const float* centers, const float* P,
                                 const int32_t* to_be_matched, int n_tbm,
                                 const l3d_match* in_matches, int n_in, const uint32_t* local2global,
                                 float uncertainty_k_upper, float uncertainty_k_lower,
                                 float sigma_p, float sigma_a, float spatial_k,
                                 int seg_begin, int seg_end,
                                 l3d_match** out_matches, int* out_n, float* median_depth,
                                 float** out_best_depths, int* out_n_best);

/* Replaces replicator_dynamics_diffusion (cudawrapper.h:73-74, cudawrapper.cu:1131-1191) plus the
 * SparseMatrix construction of performDiffusion (line3D.cc:1258, sparsematrix.cc:63-191):
 * A = the affinity edge list in list order, n = number of nodes; out (caller-allocated, nnz
 * entries) = the entries of the returned matrix (row-sorted) as (i,j,w).  The reference's
 * positional lock-step product (cudawrapper.cu:786-800) is reproduced, not "fixed". */
int l3d_replicator_dynamics_diffusion(l3d_ctx* ctx, const l3d_edge* A, int nnz, int n, int iters, l3d_edge* out);

/* Batched Line3D::similarity_coll3D (line3D.cc:1600-1681) for the affinity fill
 * (clusterSegments2D, line3D.cc:968-1221): sim[k] = similarity(hyp[pairs[2k]], hyp[pairs[2k+1]]). */
int l3d_similarity_coll3D_batch(l3d_ctx* ctx, const l3d_hypothesis* hyp, int n_hyp,
                                const int32_t* pairs, int n_pairs, float sigma_a, float* sim);

/* The affinity fill of Line3D::clusterSegments2D (line3D.cc:968-1221) on the device: candidate enumeration with the
 * reference's `used` bookkeeping (three edge families: potential correspondence / collinear with it / collinear with the
 * source), similarity_coll3D, the thresholds (L3D_MIN_AFFINITY 0.25 / 0.01), first-touch node numbering and the symmetric
 * edge list A -- from flat tables.  Segments are numbered densely view by view (views in ascending camera id):
 * dense id = seg_base[view] + segment.  Hypotheses (greedySelection, line3D.cc:899-965) are numbered in dense order.
 *   seg_base        n_views + 1
 *   view_hyp_begin  n_views + 1: the hypotheses of a view are [view_hyp_begin[v], view_hyp_begin[v+1])
 *   hyp, score, hyp_dense   n_hyp: 3-D hypothesis, min(confidence, 1), dense id of its segment
 *   best            per dense id: its hypothesis or -1
 *   pot_start/pot_tgt   potential_correspondences_ (line3D.cc:861-865) per dense id as CSR, targets as dense ids, ascending
 *                       (entries whose camera names no view, or whose segment does not exist, left out)
 *   coll_start/coll_other/coll_w   segment2collinearities_ (segments.h:89-93) per dense id as CSR, ascending dense ids
 * Outputs (callee-allocated, l3d_free): edges (n_edges = 2 x kept candidates, (a,b,w) then (b,a,w), in the reference's
 * order), node_hyp[node] = hypothesis (local2global), the number of enumerated candidate pairs. */
typedef struct l3d_affinity_input {
    int32_t n_views;
    const int32_t* seg_base;
    const int32_t* view_hyp_begin;
    int32_t n_hyp;
    const l3d_hypothesis* hyp;
    const float* score;
    const int32_t* hyp_dense;
    const int32_t* best;
    const int64_t* pot_start;
    const int32_t* pot_tgt;
    const int64_t* coll_start;
    const int32_t* coll_other;
    const float* coll_w;
    float sigma_a;
} l3d_affinity_input;
int l3d_affinity_fill(l3d_ctx* ctx, const l3d_affinity_input* in, l3d_edge** edges, int* n_edges, int32_t** node_hyp, int* n_nodes,
                      int* n_candidates);
/* The fill enumerates its candidates a block of source segments at a time (the reference walks them source by source, line3D.cc:996-1221), so
 * neither the transient arrays nor any count of the whole fill is bound to 31 bits; *n_candidates above saturates at INT_MAX.  The 64-bit
 * figures of the last fill on ctx: candidate pairs enumerated, candidates that passed their threshold (the list has two entries per passed
 * candidate and IS bound to 2^31 entries, like the clustering stages behind it: L3D_ERR_UNSUPPORTED beyond). */
int l3d_last_fill_counts(l3d_ctx* ctx, int64_t* n_candidates, int64_t* n_passed);

/* The edge list Line3D::performClustering walks (clustering.cc:14-40; the merge loop itself: l3d_perform_clustering_device below), prepared on
 * the device: optionally performDiffusion (line3D.cc:1255-1303: replicator_dynamics_diffusion, then A(i,j) = A(j,i) =
 * min(W(i,j), W(j,i)), rebuilt in (i,j) order), then the STABLE ascending order by weight of clustering.cc:14.
 * A == NULL: the list the last l3d_affinity_fill returned, still resident on the device (nnz must match; it is consumed).
 * L3D_ERR_UNSUPPORTED: the diffused list is not a symmetric pattern of unique entries (never the case for the list of
 * l3d_affinity_fill) -- take l3d_replicator_dynamics_diffusion and the reference's map arithmetic instead. */
int l3d_clustering_edges(l3d_ctx* ctx, const l3d_edge* A, int nnz, int n_nodes, int perform_diffusion, int iters, l3d_edge* sorted_out);
/* The same list grouped by CONNECTED COMPONENT of the (diffused) graph -- labels by hooking + pointer jumping on the device --, in
 * stable ascending weight order inside every group: the merge loop of performClustering never relates nodes of different
 * components, so the groups can be walked independently, in parallel, with the result of the sequential walk.
 * group_start (callee-allocated, l3d_free): n_groups + 1 offsets into sorted_out. */
int l3d_clustering_edges_grouped(l3d_ctx* ctx, const l3d_edge* A, int nnz, int n_nodes, int perform_diffusion, int iters, l3d_edge* sorted_out,
                                 int32_t** group_start, int* n_groups);
/* clusterSegments2D's tail in one call (line3D.cc:1239-1246 -> clustering.cc:6-47, universe.h:59-115): [performDiffusion,]
 * the grouped order above and the MERGE LOOP of performClustering on the device, one wave per connected component (the loop is
 * sequential only inside a component; each is walked in LDS with the unions, ranks and roots of the one sequential walk).
 * labels (n_nodes, caller-allocated; NULL: they only stay on the device, for l3d_fit_labelled_clusters): labels[k] =
 * CLUniverse::find(k), bit-equal to performClustering's.  c: the reference
 * passes 1.0 (line3D.cc:1245).  n_components (may be NULL): connected components that hold an edge.
 * A == NULL: the resident list of l3d_affinity_fill, as above.  L3D_ERR_UNSUPPORTED as for l3d_clustering_edges. */
int l3d_perform_clustering_device(l3d_ctx* ctx, const l3d_edge* A, int nnz, int n_nodes, int perform_diffusion, int iters, float c, int32_t* labels,
                                  int* n_components);

/* The line fit of Line3D::processClusteredSegments (line3D.cc:1306-1597: getLineEquation3D, projectToLine) for many clusters at
 * once, on the device.  A cluster = its members' hypothesis indices in key order (camera, segment):
 * group_start (n_groups + 1) into member_hyp.  hyp / hyp_cam: all hypotheses (3-D end points in the normalised scene) and their
 * camera ids; hyp == NULL: the table of the last l3d_affinity_fill, still on the device (n_hyp must match).
 * Rinv (3x3 row-major), scale_inv, tneg: Line3D::inverseTransform (line3D.cc:1782-1786), applied to every end point.
 * Outputs (callee-allocated, l3d_free): seg_count[g] = 3-D segments of cluster g (the stretches seen by at least three cameras,
 * in sweep order), segs = 6 doubles (start, end) per segment, the clusters back to back. */
int l3d_fit_clusters(l3d_ctx* ctx, const int32_t* group_start, int n_groups, const int32_t* member_hyp, const l3d_hypothesis* hyp,
                     const uint32_t* hyp_cam, int n_hyp, const double* Rinv, double scale_inv, const double* tneg,
                     int32_t** seg_count, double** segs, int* n_segs);
/* processClusteredSegments from the LABELS (line3D.cc:1306-1368): the grouping on the device too -- clusters in ascending label
 * order (the reference's std::map), members in key order, those with >= 4 members seen from >= 4 cameras are fitted as above.
 * labels / node_hyp (n_nodes each): cluster label and hypothesis index of every node of the affinity list; NULL: the arrays
 * l3d_perform_clustering_device / l3d_affinity_fill* left on the device.  Out (callee-allocated, l3d_free): the fitted
 * clusters -- group_start (n_groups + 1) into member_hyp -- and seg_count / segs as l3d_fit_clusters.
 * PRECONDITION: hyp_cam is non-decreasing in the hypothesis index (hypotheses numbered view by view, as greedySelection numbers
 * them, line3D.cc:899-965): the distinct cameras of a cluster are counted as camera changes between members in hypothesis
 * order.  Checked; L3D_ERR_INVALID otherwise. */
int l3d_fit_labelled_clusters(l3d_ctx* ctx, const int32_t* labels, const int32_t* node_hyp, int n_nodes, const l3d_hypothesis* hyp,
                              const uint32_t* hyp_cam, int n_hyp, const double* Rinv, double scale_inv, const double* tneg,
                              int32_t** group_start, int32_t** member_hyp, int* n_groups, int32_t** seg_count, double** segs, int* n_segs);

/* Refinement of 3-D lines against the 2-D segments of their clusters (no counterpart in the reference; formulas: line3d_amd/csrc/l3d_refine.hpp,
 * DESIGN.md 4g).  Every cluster gets a Levenberg-Marquardt fit of its line (4 local parameters, Huber loss on the pixel distance of the members'
 * 2-D end points to the projected line, f64), one wave per cluster, and its members' end points are taken onto the refined line by their viewing
 * rays and swept as l3d_fit_clusters sweeps them -- the emitted segments of a cluster lie on one line.
 * A cluster = its members in key order: group_start (n_groups + 1) into member_cam (index into `cameras`), member_seg (x1, y1, x2, y2) and
 * member_pts (the hypothesis' two 3-D end points); cameras: n_cameras 3x4 matrices P = [M | p4], row-major, in the frame of the points.
 * params == NULL: 20 iterations, huber_px 2.0; huber_px 0: plain least squares.
 * Outputs per cluster (caller-allocated): line (point A, unit direction d), rms_before / rms_after (pixels, unweighted), iterations (trials
 * made), status (0 refined, 1 no trial lowered the cost: the starting line, 2 degenerate -- fewer than two usable members or an input that is not
 * finite: the starting line).  seg_count / segs / n_segs: callee-allocated (l3d_free), as l3d_fit_clusters.
 * Refused with L3D_ERR_INVALID before anything is launched: a group_start that does not ascend from 0, a camera index outside the table, a negative
 * max_iterations or huber_px, a camera matrix that is not finite.  n_groups == 0: empty outputs, L3D_OK. */
typedef struct l3d_refine_params { int32_t max_iterations; int32_t pad; double huber_px; } l3d_refine_params;
int l3d_refine_lines(l3d_ctx* ctx, const int32_t* group_start, int n_groups, const int32_t* member_cam, const float* member_seg, const double* member_pts,
                     const double* cameras, int n_cameras, const l3d_refine_params* params, double* line, double* rms_before, double* rms_after,
                     int32_t* iterations, int32_t* status, int32_t** seg_count, double** segs, int* n_segs);
/* the same arithmetic on the host (the shared functions of l3d_refine.hpp with 64 lanes run one after the other): needs no device; bit-equal to
 * l3d_refine_lines.  A refusal's cause: l3d_refine_last_error (per thread). */
int l3d_test_refine_host(const int32_t* group_start, int n_groups, const int32_t* member_cam, const float* member_seg, const double* member_pts,
                         const double* cameras, int n_cameras, const l3d_refine_params* params, double* line, double* rms_before, double* rms_after,
                         int32_t* iterations, int32_t* status, int32_t** seg_count, double** segs, int* n_segs);
const char* l3d_refine_last_error(void);


/* ---- Line3D::matchViews as one device-resident chain --------------------------------------------------------
 * The schedule of matchViews (line3D.cc:620-648) is static: which neighbours a view still has to match and
 * which earlier views hand it reverse matches follows from the neighbour graph and the processing order alone.
 * The caller describes every view of the chain (same arrays as l3d_compute_pairwise_matches) plus its sources:
 * for each already-matched local camera `source_cam[i]`, the chain index `source_index[i]` (< own index) of that
 * view, whose kept matches towards this view become the existing matches (line3D.cc:806,838-872) -- on the
 * device, without touching the host.  Nothing waits for the host: stage 1 of all views is enqueued first, then
 * the per-view verification; the callback is invoked once per view, in order, as its kept list arrives, while
 * the GPU works on later views.  Results are bit-identical to calling l3d_compute_pairwise_matches per view.
 * Views with n_tbm == 0 are not computed (cudawrapper.cu:877-878): callback with verified = 0.
 * Callback arguments: kept matches (sorted, GLOBAL camera ids, confidence/2), the depth pairs entering the
 * median (cudawrapper.cu:1058-1062) and the number of candidates verified (0: the reference returns before
 * touching median_depth, cudawrapper.cu:955-956).  The buffers are only valid during the call.  Return non-zero
 * from the callback to abort. */
typedef struct l3d_chain_view {
    uint32_t view_id;
    const float* src_segs; int32_t S_src;
    const float* RtKinv_src; const float* C_src;
    const float* tgt_segs; int32_t n_tgt;
    const int32_t* offsets; int32_t N;
    const float* F; const float* RtKinv; const float* centers; const float* P;
    const int32_t* to_be_matched; int32_t n_tbm;
    const uint32_t* local2global;
    const int32_t* source_cam; const int32_t* source_index; int32_t n_sources;
    float sigma_p, sigma_a, spatial_k;
} l3d_chain_view;
/* `kept` points into pinned host memory owned by the context and stays valid until the next chain (l3d_match_chain /
 * l3d_shard_chain_open) starts on it or the context is destroyed: a callback may keep the pointer instead of copying.
 * `best_depths` is only valid during the call. */
typedef int (*l3d_chain_callback)(void* user, int index, int verified, const l3d_match* kept, int n_kept,
                                  const float* best_depths, int n_best, int n_candidates);
int l3d_match_chain(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, l3d_chain_callback cb, void* user);

/* ---- Line3D::matchViews with its products kept in HBM ------------------------------------------------------------
 * l3d_match_chain_resident runs the chain of l3d_match_chain WITHOUT handing any kept list to the host, and builds what
 * performMatching leaves behind (line3D.cc:834-884) on the device, from the kept arena that never left HBM:
 *   - potential_correspondences_ (line3D.cc:861-865): for every kept match both directions, as a CSR over DENSE segment
 *     ids -- sorted, duplicates dropped (the reference's nested std::map: set semantics, ascending iteration);
 *   - the match file of every view after its own only-best overwrite (line3D.cc:884, view.cc:165-183): per segment the
 *     first kept match with the highest confidence;
 *   - the median depth of every view (cudawrapper.cu:1058-1076).
 * Views with nothing left to match (cudawrapper.cu:877-878) hand back their existing list with LOCAL camera ids and
 * confidence 0; their entries are formed with those numbers read as view ids, as the reference does.
 * Dense ids: the segments of ALL views of the scene, view by view in ascending camera id: dense = seg_base[i] + segment.
 * summary (caller's, n_views entries): per chain view its kept / candidate counts and median depth (1.0 where the
 * reference leaves it untouched).  n_pot: entries of the CSR.  The products stay valid until the next chain runs on ctx. */
typedef struct l3d_dense_map {
    int32_t n_views;               /* all views of the scene */
    const uint32_t* view_ids;      /* ascending */
    const int32_t* seg_base;       /* n_views + 1 */
} l3d_dense_map;
typedef struct l3d_chain_summary {
    int32_t verified;              /* 0: nothing left to match (early return) */
    int32_t n_kept;                /* length of the view's list (early return: the localized existing list) */
    int64_t n_candidates;
    float median_depth;
    int32_t pad;
} l3d_chain_summary;
int l3d_match_chain_resident(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, const l3d_dense_map* map,
                             l3d_chain_summary* summary, int64_t* n_pot);
/* copies of the resident products (inspection, tests, host fallbacks).  l3d_chain_kept_list: the kept list of chain view
 * `index` as l3d_match_chain's callback would have received it (callee-allocated, l3d_free; 0 records for a view that was
 * not verified).  l3d_chain_products_get: pot_start (n_dense + 1), pot_tgt (n_pot), best_match (n_dense records; segID1 ==
 * 0xffffffff where a segment has none; camera ids as in the kept lists: GLOBAL, LOCAL for early-return views) -- any
 * pointer may be NULL. */
int l3d_chain_kept_list(l3d_ctx* ctx, int index, l3d_match** out, int* n);
/* What only matchViews and l3d_products_hypotheses read goes back to the device: the kept arena, its side words and run tables, the early pair
 * transposes, the chain's scratch.  The products stay (rows, hypotheses): affinity fill, clustering and fits run as before.  Afterwards
 * l3d_chain_kept_list, l3d_chain_records_digest, l3d_products_hypotheses and the best matches of l3d_chain_products_get return L3D_ERR_INVALID
 * with a message, until the next chain builds its products. */
int l3d_chain_release_records(l3d_ctx* ctx);
/* an order-sensitive 64-bit digest and the length of the kept list of every chain view of the resident products (n = their number of chain views;
 * 0 / 0 for a view of which this context holds nothing, and for an early-return view, whose list is rebuilt from its sources' records): what two contexts that ran the same chain with different keep sets must agree on */
int l3d_chain_records_digest(l3d_ctx* ctx, uint64_t* hash, int32_t* n_kept, int n);
int l3d_chain_products_get(l3d_ctx* ctx, int64_t* pot_start, int32_t* pot_tgt, l3d_match* best_match);

/* Line3D::greedySelection (line3D.cc:899-965) on the resident products: one 3-D hypothesis per segment that has a best
 * match (L3DView::unprojectSegment, view.cc:302-342, in double), numbered in dense order, left on the device for
 * l3d_affinity_fill_resident and l3d_fit_clusters.  geometry: one entry per view of the dense map.
 * Outputs: view_hyp_begin (caller's, n_views + 1), hyp_dense (callee-allocated, l3d_free: dense id per hypothesis). */
typedef struct l3d_view_geometry {
    double RtKinv[9];              /* R^T K^-1, row-major */
    double C[3];
    float k_lower, k_upper;        /* view.cc:90-121 */
    float median_depth;
    int32_t n_segments;
    const float* segments;         /* host pointer of the view's segments (registered: l3d_register_segments) */
} l3d_view_geometry;
int l3d_products_hypotheses(l3d_ctx* ctx, const l3d_view_geometry* geometry, int n_views, int32_t* view_hyp_begin, int32_t** hyp_dense, int* n_hyp);
/* l3d_affinity_fill on the resident tables: hypotheses of l3d_products_hypotheses, potential correspondences and best
 * matches of l3d_match_chain_resident; only the collinearity CSR (segment2collinearities_, static per scene) comes from the
 * host -- uploaded when coll_changed != 0, otherwise the copy of the previous call is used.  Outputs as l3d_affinity_fill. */
int l3d_affinity_fill_resident(l3d_ctx* ctx, const int64_t* coll_start, const int32_t* coll_other, const float* coll_w, int coll_changed,
                               float sigma_a, l3d_edge** edges, int* n_edges, int32_t** node_hyp, int* n_nodes, int* n_candidates);
/* (edges == NULL: the list is not copied to the host -- it stays resident for l3d_perform_clustering_device / l3d_clustering_edges(A
 * = NULL) and can be fetched later, also after the clustering consumed it: ) */
int l3d_resident_edges_get(l3d_ctx* ctx, l3d_edge* out, int nnz);
/* the resident hypothesis table (n_hyp entries of l3d_products_hypotheses) copied to the host */
int l3d_products_hypotheses_get(l3d_ctx* ctx, l3d_hypothesis* hyp, float* score);

/* ---- the resident chain with every view's source segments sharded over the GPUs of one node ---------------------
 * One process per GPU.  Each rank opens the chain with (rank, world) and per view k: l3d_shard_chain_enqueue writes
 * this rank's kept records for its source-segment range [S*rank/world, S*(rank+1)/world) into `send_slot`
 * (*slot_bytes bytes, device memory); the CALLER all-gathers the ranks' slots of view k into
 * gathered_base + (k*world + r)*slot_bytes (e.g. torch.distributed.all_gather_into_tensor = RCCL over xGMI, enqueued on
 * l3d_ctx_stream(ctx)), then calls l3d_shard_chain_mark.  Later views pull their reverse matches out of the gathered
 * slots on the device.  l3d_shard_chain_fetch (optional per rank, any time after mark) blocks the HOST until view k is
 * complete and calls the callback with the ranks' kept lists concatenated in rank (= segment) order -- the sorted list
 * of the unsharded run.  gathered_base must be zero-initialised (n_views*world*slot_bytes bytes) and stay valid until
 * close; the `views` array must outlive the chain. */
typedef struct l3d_shard_chain l3d_shard_chain;
void* l3d_ctx_stream(l3d_ctx* ctx);                  /* the context's hipStream_t, for framework interop */
int l3d_shard_chain_open(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, int rank, int world, int slot_records,
                         l3d_shard_chain** out, size_t* slot_bytes);
int l3d_shard_chain_enqueue(l3d_shard_chain* chain, int k, void* send_slot, const void* gathered_base);
int l3d_shard_chain_mark(l3d_shard_chain* chain, int k);
int l3d_shard_chain_fetch(l3d_shard_chain* chain, int k, l3d_chain_callback cb, void* user);
int l3d_shard_chain_close(l3d_shard_chain* chain);
/* The same protocol as ONE native call (send/gathered buffers owned by the context): the calling thread enqueues view
 * after view -- kernels, then `exchange` on the context's stream, then the completion event -- and a second host thread
 * trails behind with fetch -> cb (cb == NULL: this rank does no host bookkeeping).  `exchange` must enqueue, on `stream`,
 * the all-gather of the ranks' slots of one view: send_slot (slot_bytes) -> recv_block (world*slot_bytes, rank order);
 * non-zero return = failure.  Adapters: l3d_exchange_rccl (user = l3d_rccl_link: an RCCL communicator of the `world`
 * ranks and the address of ncclAllGather, both taken from the RCCL the process has already loaded -- this library does
 * not link against RCCL), l3d_exchange_local (world == 1), l3d_exchange_replay (user = device address of the gathered
 * blocks of a recorded run: measures one rank of a world-W job on a single GPU, scripts/emulate_rank.py). */
typedef int (*l3d_exchange_fn)(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream);
typedef struct l3d_rccl_link { void* comm; void* all_gather; } l3d_rccl_link;
int l3d_shard_chain_run(l3d_shard_chain* chain, l3d_exchange_fn exchange, void* exchange_user, l3d_chain_callback cb, void* cb_user);
int l3d_exchange_rccl(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream);
int l3d_exchange_local(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream);
int l3d_exchange_replay(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream);
const void* l3d_shard_chain_gathered(l3d_shard_chain* chain);   /* device address of the gathered blocks after l3d_shard_chain_run */
/* The fourth adapter: the ranks of ONE process, one per entry of a device list (a device may repeat: virtual ranks on one GPU), each on a host
 * thread of its own.  l3d_node_comm_create enables peer access between every pair of distinct devices (L3D_ERR_UNSUPPORTED, the pair named on
 * stderr, when a pair is refused); l3d_node_comm_bind tells it which rank's exchanges arrive on which stream (l3d_ctx_stream of the rank's
 * context; one stream per rank).  l3d_exchange_node (user = the communicator) gathers the ranks' slots with one kernel launch per rank that
 * reads the peers' slots through peer-mapped pointers; two host barriers per exchange, ordering by stream events only.
 * A broken barrier -- l3d_node_comm_abort (a rank that returns with an error calls it), a failed exchange, 600 s without the other ranks --
 * makes every pending and later exchange of every rank return non-zero: nothing hangs.  l3d_line3d_create_node owns one of these. */
typedef struct l3d_node_comm l3d_node_comm;
int l3d_node_comm_create(const int* devices, int n, l3d_node_comm** out);
void l3d_node_comm_destroy(l3d_node_comm* comm);
int l3d_node_comm_bind(l3d_node_comm* comm, int rank, void* stream);
void l3d_node_comm_abort(l3d_node_comm* comm);
int l3d_exchange_node(void* user, int view, const void* send_slot, void* recv_block, size_t slot_bytes, int world, void* stream);
/* A rank that fails inside l3d_shard_chain_run (capacity, HIP error, failing callback) keeps calling `exchange` for every
 * remaining view with a slot that says "gave up": no rank is left waiting in a collective.  Afterwards every rank reads the
 * same verdict out of the gathered slot headers: L3D_ERR_NOMEM on ALL ranks when any slot overflowed.  l3d_shard_chain_info
 * (any out pointer may be NULL): this chain's candidate capacity and slot_records, and after a run the OR of the ranks'
 * overflow bits (1 candidate capacity, 2 slot_records, 4 a rank gave up, 8 the compact arena of the ring mode) and the largest candidate / kept count one rank
 * reported for one view -- what a caller needs to reopen with more room (l3d_set_chain_capacities sets the candidate capacity
 * of the next chain); l3d_line3d_shard_run does exactly that, up to three times. */
/* matchViews' products (as l3d_match_chain_resident leaves them: potential correspondences, best matches, medians; line3D.cc:834-884)
 * built on THIS rank's device from the gathered slots of a finished l3d_shard_chain_run -- every rank holds every view's kept records,
 * so no rank has to hand lists to the host (cb == NULL on all ranks).  The context then serves l3d_chain_kept_list,
 * l3d_chain_products_get, l3d_products_hypotheses, l3d_affinity_fill_resident as after the single-GPU chain. */
int l3d_shard_chain_products(l3d_shard_chain* chain, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot);
int l3d_shard_chain_info(l3d_shard_chain* chain, size_t* cand_cap, int* slot_records, int* overflow_bits, int* max_candidates, int* max_kept);
/* Ring mode of l3d_shard_chain_run (cb == NULL; automatic when the gathered blocks of all views would exceed 8 GB -- 2048 views x 8 ranks
 * x 3.8 MB = 63 GB per rank at 4000 segments x 24 neighbours --, L3D_SLOT_RING=1 / l3d_set_option forces it, 0 forbids it): the gathered
 * buffer holds only the views later views still read (the neighbour window of the schedule + a batch); older blocks are retired into the
 * compact kept arena, in the order of the unsharded run, before they are overwritten -- what the reference does with its per-view match files
 * (view.cc:150-224).  l3d_shard_chain_gathered then returns NULL.  Overflow bit 8 = the compact arena's first guess was too small;
 * l3d_shard_chain_arena_needed: the kept matches of the whole run (records of 32 bytes), for the retry (l3d_set_chain_capacities' second
 * argument; l3d_line3d_shard_run does it). */
long long l3d_shard_chain_arena_needed(l3d_shard_chain* chain);
/* A PARTITIONED job on the segment-sharded run (call between l3d_shard_chain_open and l3d_shard_chain_run, cb == NULL there): every rank sees
 * every view's gathered slots go by, so what it KEEPS is its choice -- the views its block [own_begin, own_end) of the chain needs (2 x reach
 * either side, reach = the largest chain distance between a view and a neighbour), the sources of the early-return views and the views their
 * local camera numbers name (cudawrapper.cu:877-878, line3D.cc:861-865).  The run retires only those into this rank's arena (ring mode, forced);
 * l3d_shard_chain_products then builds this rank's share of matchViews' products -- the state l3d_match_chain_partition leaves, without any
 * speculation: exact on every scene, the chain's work split 1/world per view, the kept records and the table split by view block.
 * l3d_products_hypotheses and l3d_affinity_fill_sharded follow as there.  (l3d_line3d_shard_run: commit = 3.) */
int l3d_shard_chain_partition(l3d_shard_chain* chain, int own_begin, int own_end);
/* the keep set of l3d_shard_chain_partition as a function of the schedule alone (host logic, no context): keep[k] = 1 for the chain views a rank that
 * owns [own_begin, own_end) retires; *reach (may be NULL) = the largest chain distance between a view and one of its neighbours */
int l3d_partition_keep_views(const l3d_chain_view* views, int n_views, int own_begin, int own_end, unsigned char* keep, int* reach);
/* the schedule of a node object's turns that hand the chain over (l3d_line3d_set_turn_handover) as a function of the static schedule alone (host
 * logic, no context).  out[8 * r + 0 .. 7] of turn r of `world`, in chain positions: pre0, run0 (the views [pre0, run0) are taken over from turn
 * r - 1), run1 (the turn's chain computes [run0, run1) and holds the one chain's records of [pre0, run1)), row0, row1 (the rows of the table its share
 * builds), own0, own1 (its block), deferred (1: its share ingests something a LATER turn's block produces -- records that point at an early-return
 * view, best matches of a view an early return's local camera numbers name -- so it builds nothing in its turn and gets a second visit after the
 * last turn).  info[0 .. 3] (may be NULL) = reach, check, tail, supported (0: a scene the blocks-of-views partition refuses; its compute3Dmodel
 * runs as plain mode 2) */
int l3d_turn_handover_plan(const l3d_chain_view* views, int n_views, int world, int32_t* out, int32_t* info);

/* ---- Line3D::matchViews sharded by BLOCKS OF VIEWS over the ranks, speculatively, with exact verification ----------------------
 * (line3D.cc:620-648 is a chain over views: the kept matches of a view become candidates of its later neighbours, :806,838-872.)
 * Rank r runs the ordinary single-GPU resident chain on views [B_r - warmup_views, B_{r+1}) only (B_r = n_views * r / world), started
 * cold: nothing is known about the views in front.  The chain's memory is short -- about three neighbour windows on the synthetic
 * scenes (scripts/speculate_blocks.py) -- so by view B_r the kept lists normally ARE the one chain's.  That is checked, not assumed:
 * every rank publishes a 64-bit digest of every kept list it computed (`exchange`, an all-gather: view = -1); rank r's block is exact iff
 * rank r-1's is and the `window` views in front of B_r came out of r's warm-up exactly as r-1 computed them (from B_r on every view then
 * has the one chain's inputs).  Every rank reads the same table and reaches the same verdict.  *verdict = 0: the ranks all-gathered
 * their blocks (view = -2) and THIS context now holds matchViews' products exactly as after l3d_match_chain_resident over all views
 * (arena, potential correspondences, best matches, medians; summary / n_pot as there).  A block whose speculation did NOT hold is repaired, not
 * abandoned (round 5): every rank that missed takes over its predecessor's last `window` views -- records, best depth pairs and positions, one
 * all-gather, view = -5 -- and re-runs its block warm from them, all of them at once; the digests are exchanged again, until nobody misses (rank j
 * is exact after round j at the latest; a warm-up shorter than the window simply makes a rank take that path).  *verdict = 1 only when a block is shorter than the window
 * (it cannot vouch for its successor's sources) or option block_recover = 0 (the round-4 behaviour): nothing was committed, run l3d_shard_chain_run.
 * No per-view collective: four data exchanges per pass (digests; blocks; view = -4 the pieces of the products table, of which every rank
 * builds the rows of its own block) and three 256-byte ones of status words (view = -3; the second carries the sizes of the pieces): every step
 * only one rank can fail in (an allocation, a launch) is followed by one, so either all ranks enter the big collective behind it or all
 * return an error -- nobody is left waiting.  window = the largest distance between a view and one of its sources. */
int l3d_match_chain_blocks(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot,
                           int rank, int world, int warmup_views, int window, l3d_exchange_fn exchange, void* exchange_user, int* verdict);

/* ---- Line3D::matchViews sharded by blocks of views with NOTHING REPLICATED (the configs[4] job: 2048 views x 4000 segments x 24 neighbours keep
 * 6.4 G matches -- with the table built from them, beyond one GPU's HBM; the reference streams a view at a time
 * and spills every view's matches to a file, view.cc:150-224, line3D.cc:626-648).  Same speculation and verification as l3d_match_chain_blocks;
 * but rank r runs its chain 2 x reach views PAST its block (reach = the largest distance, in chain positions, between a view and one of its
 * neighbours) and is checked max(window, 2 x reach) views in front of it -- so it holds, computed by itself, the exact kept records of every view
 * within 2 x reach of its block.  From those it builds, locally: the rows of potential_correspondences_ of the views within `reach` of its block
 * (complete: a row needs the records of the view and of its neighbours), the best matches and medians of every view it holds.  That is all the
 * affinity fill of ITS block's sources reads (l3d_affinity_fill_sharded).  No block is gathered, no piece of the table travels; the records that
 * point at an early-return view (cudawrapper.cu:877-878: their entries are filed under LOCAL camera numbers read as view ids and can name any view
 * of the scene) are all-gathered, each source's by the rank that owns it (view = -6).  *verdict = 0: the context holds this rank's share --
 * l3d_chain_kept_list serves the views it holds (empty lists for the others), l3d_chain_products_get its rows (empty rows elsewhere; *n_pot = its
 * entries), l3d_products_hypotheses numbers the hypotheses of the views it holds from 0 (l3d_affinity_fill_sharded makes the numbers global).
 * *verdict = 1: as l3d_match_chain_blocks (only when a block is re-run more than `world` times or the schedule holds more than 64 early returns:
 * a failed speculation is repaired by re-running that block warm, see there). */
int l3d_match_chain_partition(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, l3d_chain_summary* summary, int64_t* n_pot,
                              int rank, int world, int warmup_views, int window, l3d_exchange_fn exchange, void* exchange_user, int* verdict);
/* what this rank's share covers after l3d_match_chain_partition, in views of the dense map: info = { rank, world, own block [begin, end), rows
 * [begin, end), held [begin, end), rounds of warm re-runs, blocks re-run in them (whole job; also set by l3d_match_chain_blocks) }; n_pot_all:
 * entries of the table over all ranks */
int l3d_partition_info(l3d_ctx* ctx, int info[10], int64_t* n_pot_all);
/* The fill SHARDED BY SOURCE KEY over the ranks of a job whose matchViews ran partitioned (l3d_match_chain_partition below): every
 * rank enumerates the candidates of the sources of ITS block of views -- from the rows, best matches and hypotheses it holds, nothing of another
 * rank is read -- and five small all-gathers (`exchange`, views -7 .. -10 and status words -3) make global what has to be: hypotheses per view
 * (global hypothesis numbers), the first-touch minima per hypothesis (64-bit positions: rank << 44 | position inside the rank's enumeration), the
 * candidates that passed their threshold (12 bytes each; concatenated in rank order = the reference's enumeration order, line3D.cc:996-1221) and
 * the hypothesis table (read by the line fit).  Node numbering and the edge list are then formed by every rank from the same data: afterwards the
 * context is in the state l3d_affinity_fill_resident(edges = NULL) leaves it in, with GLOBAL hypothesis numbers -- l3d_perform_clustering_device,
 * l3d_fit_labelled_clusters, l3d_resident_edges_get, l3d_products_hypotheses_get follow unchanged (replicas).  Outputs: n_edges / node_hyp / n_nodes
 * as l3d_affinity_fill_resident; n_candidates_all (may be NULL): candidate pairs enumerated by all ranks; view_hyp_begin_global (caller's,
 * n_views + 1 of the dense map), hyp_dense_global (callee-allocated, l3d_free: dense segment id per global hypothesis), n_hyp_global.
 * A rank that fails on its own still enters every collective with a mark, so all ranks return an error together. */
int l3d_affinity_fill_sharded(l3d_ctx* ctx, const int64_t* coll_start, const int32_t* coll_other, const float* coll_w, int coll_changed, float sigma_a,
                              l3d_exchange_fn exchange, void* exchange_user, int* n_edges, int32_t** node_hyp, int* n_nodes,
                              int64_t* n_candidates_all, int32_t* view_hyp_begin_global, int32_t** hyp_dense_global, int* n_hyp_global);

/* ---- residency: keep a view's segments in HBM across calls ------------------------------------
 * The reference re-uploads every neighbour's segments for every view (line3D.cc:793-800).  A
 * caller may instead register segment arrays once; l3d_compute_pairwise_matches recognises
 * host pointers that were registered (same pointer, same size) and skips the upload. */
int l3d_register_segments(l3d_ctx* ctx, const float* segments, int n_segments);
int l3d_unregister_segments(l3d_ctx* ctx, const float* segments);
/* the same for many arrays at once (all views of a scene): one device allocation, one wait */
int l3d_register_segments_batch(l3d_ctx* ctx, const float* const* arrays, const int* n_segments, int n_arrays);

/* ---- measurement ---------------------------------------------------------------------------
 * With profiling on, every kernel launch is bracketed by HIP events on the context's stream;
 * l3d_profile_get returns the launch count and summed duration for one kernel name
 * ("pair_mask", "pair_fill", "verify", ...; l3d_profile_names lists them, ';'-separated). */
/* stage-2 algorithm: 0 = depth-window search (default; segments that outgrow the kernel's LDS image use its global-scratch
 * variant; views with more than ~50 neighbours take the all-pairs kernel), 1 = all-pairs loop in the reference's formulation.
 * Results are bit-identical. */
int l3d_set_verify_mode(l3d_ctx* ctx, int mode);
/* stage-1 filters in front of the exact epipolar/overlap/triangulation sequence: bit 0 = wedge test, bit 1 = interval bounds of the two
 * overlap ratios (they reject -- and, in the chains, accept -- what they can decide; a pair with an intersection point on a segment end
 * point is always left to the exact test), bit 2 SET = the bounds do not accept; 3 = everything (default), 0 = the exact sequence
 * alone (A/B testing: results are bit-identical, candidate counts included) */
int l3d_set_pair_pretest(l3d_ctx* ctx, int mask);
/* Diagnostic / A-B switches (line3d_amd/csrc/l3d_options.hpp lists them with their meaning).  The environment (L3D_<NAME>) is
 * read ONCE, when the context is created; afterwards a switch changes only through this call.  name: "L3D_TIMING", "TIMING" or
 * "timing".  No switch selects a CPU path for the arithmetic.  L3D_ERR_INVALID for an unknown name. */
int l3d_set_option(l3d_ctx* ctx, const char* name, int value);
int l3d_get_option(l3d_ctx* ctx, const char* name, int* value);
/* testing: cap the LDS image of the depth-window kernel (bytes; 0 = device limit) so that segments take the
 * global-scratch variant; process-wide */
int l3d_set_verify_lds_budget(size_t bytes);
/* testing: initial candidate / kept-arena capacities (records) of the resident chain, 0 = the built-in estimate; small
 * values force the overflow -> grow -> restart-at-that-view path */
int l3d_set_chain_capacities(l3d_ctx* ctx, size_t cand_cap, size_t arena_cap);
/* loads the code objects of every kernel of the library now (in parallel) instead of at their first launch: takes the
 * ~10 x 3 ms of lazy loading out of the first matchViews / finish of a process */
int l3d_warm_up(l3d_ctx* ctx);
/* reserves the device arenas of the finishing stages (greedy selection, affinity fill, edge order, line fit) ahead of their
 * first use, from the size of the scene: a hint, the arenas still grow on demand */
int l3d_reserve_hint(l3d_ctx* ctx, int n_dense, int n_views, int n_neighbors);
int l3d_profile_enable(l3d_ctx* ctx, int on);
/* bracket only the named kernel with HIP events (NULL or "": all kernels) -- keeps a timed region nearly undisturbed */
int l3d_profile_only(l3d_ctx* ctx, const char* kernel);
int l3d_profile_reset(l3d_ctx* ctx);
int l3d_profile_get(l3d_ctx* ctx, const char* kernel, int64_t* launches, double* total_ms);
const char* l3d_profile_names(void);
/* counters of the last l3d_compute_pairwise_matches call:
 * [0] stage-1 pairs evaluated, [1] raw candidates (incl. existing), [2] verify inner iterations
 * (sum over segments of m^2), [3] kept matches */
int l3d_last_stats(l3d_ctx* ctx, double stats[4]);
/* the last resident chain of the context (l3d_match_chain, l3d_match_chain_resident and the ranged chains built on them): how many views were
 * enqueued collecting their reverse matches by scanning their sources' records (k_exist_count / k_place) and through their sources' run tables
 * (k_exist_count_rt + k_exist_combine / k_place_rt; options long_list, rt_g), counted where the chain decides.  A view the chain runs again
 * after an overflow counts again. */
int l3d_last_chain_routes(l3d_ctx* ctx, int* n_scanned, int* n_run_tables);
/* the lanes that share a run on the run-table route, from option rt_g and the average run of the lists seen so far (tests; host only, no
 * context): a power of two in [1, 64] whatever the option holds */
int l3d_test_rt_lanes(int opt, double avg_run);
/* the size the single-GPU chain grows its kept arena to after a view overflowed it (tests; host only, no context, no device): arena_cap records
 * overflowed with kept_base in use, the view keeps n_want, `done` of the call's `span` views are finished, free_bytes of HBM are free (UINT64_MAX:
 * not known), turn_room records are a turn's room (0: none), the chain transposes early / builds the products.  out = { new capacity, records
 * needed, records that fit, bytes counted per record, bytes kept back }; L3D_OK, or L3D_ERR_NOMEM when what fits does not do */
int l3d_test_arena_regrow(uint64_t arena_cap, uint64_t kept_base, int n_want, int done, int span, uint64_t free_bytes, uint64_t turn_room,
                          int early, int products, uint64_t out[5]);
/* the rules of matchViews sharded by blocks of views (l3d_match_chain_blocks, l3d_match_chain_partition) on a table of digests given as plain arrays
 * (tests; host only, no context, no device).  hash, n_kept: world x n_views, rank by rank -- every rank's digest of every view; comp_from[world]: the
 * first view every rank computed; verified, S_src: per view.  check, tail: how many views in front of its block a rank is checked on and how far past
 * it the chain runs (partition != 0 only).  Out: begin[world + 1] and owner[n_views], the blocks; reach_out = { reach, tail, check } as the modes derive
 * them from window and neighbour_reach; miss[world], first_diff[world] (the first view at which a rank differs from its predecessor, or -1); summary =
 * { ranks that missed, 1 when the pass is hopeless, the first rank whose table carries the failure mark or -1 }; what the predecessor of every rank
 * that missed hands over, filed under the SENDER: t_rec[world] records, t_seg[world] segments, t_first[world] (its first verified view or -1), and
 * maxima = { largest t_rec, largest t_seg } */
int l3d_test_blocks_verdict(int n_views, int world, int window, int neighbour_reach, int check, int tail, int partition, const uint64_t* hash,
                            const int32_t* n_kept, const int32_t* comp_from, const int32_t* verified, const int32_t* S_src, int32_t* begin, int32_t* owner,
                            int32_t reach_out[3], int32_t* miss, int32_t* first_diff, int32_t summary[3], int64_t* t_rec, int64_t* t_seg, int32_t* t_first,
                            int64_t maxima[2]);
/* the sizing rules of the segment-sharded run (l3d_shard_chain_open, l3d_shard_chain_run, l3d_line3d_shard_run) on plain numbers (tests; host only, no
 * context, no device).  Five sections, each skipped when its input is NULL:
 *   geom_in = { largest S_src, largest N, world, slot_records, option slot_cams_min, n_views } -> geom_out = { seg_cap, offsets of the best depth
 *     pairs, the best positions, the records, the side words (0: none), the run table (0: none), slot bytes, bytes of a staging buffer, ring, max_n }
 *   ring_in = { n_views, window, bytes of a view's gathered block, option slot_ring, partitioned, commits on the host } -> ring_out = { ring mode,
 *     view blocks in the gathered buffer, slots sent from }
 *   pairs, guess_in = { world, test cap (0: none), cap seen, option arena_guess, free bytes (-1: not known), option regrow_free_mb, partitioned, views
 *     kept, n_views, cap seen by a partitioned pass } -> guess_out = { first guess of the compact kept arena, room under regrow_free_mb (0: no limit) }
 *   verdict_in = { overflow bits (1 candidates, 2 slot, 4 gave up, 8 arena), largest candidate count, largest kept count, arena total } -> the
 *     run's return code and error text (text_cap bytes, cut if longer)
 *   retry_in = { bits, candidate capacity, largest candidate count, slot_records, largest kept count, arena needed, room, replayed exchange } ->
 *     retry_out = { retry, next candidate capacity, next slot_records, next arena capacity (0 each: as it was), refused for room } */
int l3d_test_shard_plan(const int64_t geom_in[6], int64_t geom_out[10], const int64_t ring_in[6], int32_t ring_out[3], double pairs, const int64_t guess_in[10],
                        int64_t* guess_out, const int64_t verdict_in[4], int32_t* verdict_rc, char* text, int text_cap, const int64_t retry_in[8],
                        int64_t retry_out[5]);
/* the retirement schedule of a ring-mode run as l3d_shard_chain_run drives it (tests; host only): for every view k the views retired and the views whose
 * retirement the chain has waited for when view k's exchange is enqueued (retired_at, waited_at: n_views each); every batch as four ints { first view,
 * count, the view it was enqueued at (n_views: the final flush), 1 when the chain waited for the batch before it first } (batches: 4 x max_batches);
 * summary = { ring mode, view blocks in the ring, batches, retired and waited for after the flush, 1 when a batch is still outstanding }.
 * apart: the retirement runs on a side stream (option retire_apart).  Not in ring mode nothing is scheduled: the per-view arrays stay as given */
int l3d_test_shard_retire(int n_views, int window, int slot_ring, int partition, int apart, int32_t* retired_at, int32_t* waited_at, int32_t* batches,
                          int max_batches, int32_t summary[6]);

/* contract math exported for tests (device evaluation of c_expf / c_acosf / c_acos) */
int l3d_test_contract_math(l3d_ctx* ctx, const float* x, int n, float* out_expf, float* out_acosf, double* out_acos);
/* the squared-distance gate threshold T(u) = largest float whose correctly rounded square root is <= u:
 * the ulp walk and the closed form the kernels use, evaluated on the device (tests) */
int l3d_test_sq_threshold(l3d_ctx* ctx, const float* u, int n, float* out_walk, float* out_closed);
/* the library's exclusive scan of ints on its own (tests): out[i] = in[0] + ... + in[i-1], wrapping as int32; in and out are host
 * arrays of n entries and may not overlap */
int l3d_test_exclusive_sum(l3d_ctx* ctx, const int32_t* in, int n, int32_t* out);

/* =================================================================================================
 * Host pipeline behind the reference's public operator interface, class L3D::Line3D
 * (line3D.h:61-101): the same calls, argument meaning and error behaviour, with plain arrays in
 * place of cv::Mat / Eigen / std::list.  include/line3D_amd.hpp wraps these in a C++ class named
 * L3D::Line3D.  Images are replaced by their detected segments: `segments` is what
 * detectLineSegments would have produced (line3D.cc:1789-1871); l3d_line3d_add_image_pixels (below)
 * takes the pixels and detects them on the device.
 * K, R (3x3 row-major) and t are doubles like the reference's Eigen arguments.
 * ================================================================================================= */
typedef struct l3d_line3d l3d_line3d;

/* Line3D::Line3D (line3D.cc:6-48); defaults commons.h:42-61.  Owns one l3d_ctx on `device`. */
int l3d_line3d_create(int device, int matching_neighbors, float uncertainty_t_upper_2D, float uncertainty_t_lower_2D,
                      float sigma_p, float sigma_a, float min_baseline, int use_collinearity, int verbose,
                      l3d_line3d** out);
/* ONE object over several GPUs of this process: rank r of the job on devices[r] (a device may repeat: virtual ranks on one GPU), each an
 * ordinary pipeline object with its own context, run on a host thread of its own; n_devices == 1 is l3d_line3d_create(devices[0], ...).
 * The images go to every rank; compute3Dmodel prepares all ranks (l3d_line3d_prepare: that step alone), then runs matchViews partitioned over them (l3d_line3d_set_node_mode) and
 * the collective finish (l3d_line3d_finish_sharded) through l3d_exchange_node: every rank ends with the whole result, read from rank 0
 * (result_sizes, get_result, get_segment2D, save_result, num_cameras, stats, affinity, match_path); chain_summary gives every view's entry from
 * the rank whose block of views holds it (a rank's own summary covers the views it holds only).  last_error names the first
 * failing rank ("rank r (device d): ...").  The calls that address one rank's machinery -- shard_*, match_begin / match_order /
 * view_num_to_be_matched / match_view_*, match_end, block_run, partition_run, finish_sharded, match_views, finish, view_matches,
 * products_*, set_sync_matching, l3d_line3d_context (NULL) -- are refused with L3D_ERR_INVALID.  The host-thread budget (L3D_HOST_THREADS) is
 * split among the ranks.  L3D_ERR_INVALID for NULL, n_devices <= 0 or a negative id (before any device is touched), L3D_ERR_NODEVICE without
 * a HIP device, L3D_ERR_UNSUPPORTED when two devices cannot map each other's memory. */
int l3d_line3d_create_node(const int* devices, int n_devices, int matching_neighbors, float uncertainty_t_upper_2D, float uncertainty_t_lower_2D,
                           float sigma_p, float sigma_a, float min_baseline, int use_collinearity, int verbose, l3d_line3d** out);
/* ranks of the object (1 for l3d_line3d_create) */
int l3d_line3d_num_ranks(const l3d_line3d* h);
/* how compute3Dmodel shards matchViews over the ranks of a node object: 0 (default) = the source segments of every view, partitioned
 * (l3d_line3d_shard_run, commit = 3: exact on every scene, no speculation); 1 = blocks of views, partitioned (l3d_line3d_partition_run), falling
 * back to 0 in the same call when its verdict says the speculation cannot hold (printed under verbose).  Accepted, and without effect, on a
 * single-device object.
 * 2 = the ranks that share a device TAKE TURNS on it, for a scene whose kept records do not fit one device's memory at once: rank r computes its share of
 * the W-rank job alone (the whole chain at world 1 with the keep set of block r -- l3d_partition_keep_views --, the rows of its share of the products, its
 * hypotheses), takes the digests of the views it held, releases the kept arena (l3d_chain_release_records) and hands the device's token to the next rank; ranks on
 * different devices run at the same time; turn 0 runs first and sizes every later turn exactly.  When every turn is over the 64-bit digests of the
 * views two ranks both held are compared (a mismatch is L3D_ERR_INVALID naming the view and both ranks) and the collective finish of mode 0 follows,
 * the device's token held around every rank's candidate enumeration.  Every turn computes the whole chain: matchViews costs about W single passes.
 * The result is the one-device object's, bit for bit. */
int l3d_line3d_set_node_mode(l3d_line3d* h, int mode);
/* after a compute3Dmodel in mode 2: the kept records rank `rank` retired in its turn -- the records its arena held when the chain ended (of whatever view), plus the lists of
 * the early-return views it held as chain_summary counts them (rebuilt from their sources' records: no room of their own in the arena).  For a turn
 * that kept exactly its keep set this is the sum of the one chain's chain_summary kept counts over the views l3d_partition_keep_views gives its block.  L3D_ERR_INVALID on a single-device object, a rank out of range or when the last run took no turns. */
int l3d_line3d_node_turn_records(const l3d_line3d* h, int rank, int64_t* records);
/* Mode 2 with a warm hand-over between the turns (opt-in; no effect unless the node mode is 2): turn r computes only its own piece of the chain --
 * rank 0 the views [0, own1 + tail) cold, rank r > 0 the views [own0, own1 + tail) warm from the last `check` views of turn r - 1 (records, best depth
 * pairs, best positions: a package owned by the node object) -- builds its share as l3d_match_chain_partition would, takes its digests and releases
 * its records.  What leaves a rank through exchanges there (the records that point at early-return views, the best matches of the views their local
 * camera numbers name) goes into a store of the node object.  A turn whose share needs something of a LATER turn's block (l3d_turn_handover_plan:
 * deferred) runs its piece in order, builds nothing, and is visited a second time after the last turn: the same piece from the same package, the
 * same digests or L3D_ERR_INVALID naming the rank, then the share.  The chains of all turns then compute between one and two times the views of
 * the one chain instead of W times (every visit still sets the chain up for all views and every turn builds its share: DESIGN.md section 6 has what was measured).
 * Option regrow_free_mb, where set, bounds everything a turn's arena takes: its first guess, its regrow and the slices put behind its records.  A scene the
 * partition refuses (l3d_turn_handover_plan: supported = 0) and a node object whose ranks do not all share one device run that compute3Dmodel as
 * plain mode 2.  L3D_ERR_INVALID on a single-device object and for values other than 0 / 1.  The result is the one-device object's, bit for bit. */
int l3d_line3d_set_turn_handover(l3d_line3d* h, int on);
/* after a compute3Dmodel that ran in turns: the chain views rank `rank` computed (over all its visits) and its visits.  Hand-over off, or a run that
 * fell back to plain mode 2: n_views and 1.  With the hand-over l3d_line3d_node_turn_records reports the records the rank's arena held when its share was built. */
int l3d_line3d_node_turn_views(const l3d_line3d* h, int rank, int64_t* views_computed, int* visits);
void l3d_line3d_destroy(l3d_line3d* h);
const char* l3d_line3d_last_error(const l3d_line3d* h);
l3d_ctx* l3d_line3d_context(l3d_line3d* h);
int l3d_line3d_reset(l3d_line3d* h);                                             /* line3D.cc:62-92 */
int l3d_line3d_num_cameras(const l3d_line3d* h);                                 /* line3D.h:98 */
/* Line3D::addImage (line3D.cc:95-217) and addImage_fixed_sim (line3D.cc:220-342) */
int l3d_line3d_add_image(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height,
                         const float* segments, int n_segments, const double* K, const double* R, const double* t,
                         const uint32_t* worldpoint_ids, int n_worldpoints);
int l3d_line3d_add_image_fixed_sim(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height,
                                   const float* segments, int n_segments, const double* K, const double* R, const double* t,
                                   const uint32_t* sim_ids, const float* sims, int n_sims);
/* Line3D::compute3Dmodel (line3D.cc:345-374) = prepare + match_views + finish */
int l3d_line3d_compute3Dmodel(l3d_line3d* h, int perform_diffusion);
int l3d_line3d_prepare(l3d_line3d* h);          /* findVisualNeighbors + transformGeometry; inputs become HBM-resident */
int l3d_line3d_match_views(l3d_line3d* h);      /* Line3D::matchViews, line3D.cc:620-648 (re-runnable) */
int l3d_line3d_finish(l3d_line3d* h, int perform_diffusion);   /* optimizeLocalMatches + clusterSegments2D */
/* Refinement of the result (l3d_refine_lines), off by default: with it on, finish / compute3Dmodel refine every line of the result against the 2-D
 * segments of its cluster, in the normalised frame, and replace its 3-D segments by the refined ones (status 3: the refined sweep emitted nothing, the
 * line keeps its unrefined segments); the lines, their order and their 2-D segments do not change.  reset keeps the setting.  A node object refines
 * on rank 0's context, which holds the result.  get: one entry per result line (any pointer may be NULL); L3D_ERR_INVALID after a finish without
 * the option. */
int l3d_line3d_set_refinement(l3d_line3d* h, int on, int max_iterations, double huber_px);
int l3d_line3d_get_refinement(const l3d_line3d* h, double* rms_before, double* rms_after, int32_t* iterations, int32_t* status);
/* Merging of the result's duplicate lines ("MERGING DUPLICATE LINES", l3d_merge_lines), off by default: with it on, finish / compute3Dmodel run rounds of
 * it between the line fit and the refinement.  Per round:
 *   1. a line's P is the start of its first 3-D segment, Q the end of its last; tol = dist_px x sigma, sigma the mean over the line's 2-D members in their
 *      stored order (a sequential sum, then one division) of z / f: z = R[2] . M + t[2] at M = (P + Q) / 2, f = (|K00| + |K11|) / 2, R, t, K of the
 *      member's view as it was added.  Members with z <= 0 or a term that is not finite are skipped; none left: tol = 0
 *   2. l3d_merge_lines with cos_min = cos(angle_deg pi / 180) (computed once, on the host, in double) and max_gap
 *   3. every group of two or more lines is refitted from the union of its members in key order (camera, segment) by the fit path that built the result
 *      (l3d_fit_clusters on the resident hypothesis table, or the host fit).  A refit that emits no 3-D segment leaves the group's lines as they were
 *      (counted); otherwise the merged line takes the position of its lowest-index line and the others are removed; nothing else changes its order
 *   4. rounds until one finds no pair, or max_rounds of them
 * The refinement, if on, then runs on the merged list, and l3d_line3d_get_refinement has one entry per merged line.  reset keeps the setting.  A node
 * object merges on rank 0's context; on a sharded finish every rank that has the option set runs it on the same list and ends with the same bytes.
 *   get_merging   counts[8] = lines before, lines after, rounds in which the search ran (the one that found no pair included), pairs of round 1,
 *                 groups merged, lines released by the star rule, refits that emitted nothing (the last three summed over the rounds), 0;
 *                 final_index (may be NULL): one per line BEFORE merging, its index in the result; n_sources (may be NULL): one per line of the result,
 *                 the lines before merging it was made of.  L3D_ERR_INVALID after a finish without the option.
 * REFUSED by set_merging, L3D_ERR_INVALID: dist_px or max_gap negative or not finite, angle_deg outside [0, 90], max_rounds below 1. */
int l3d_line3d_set_merging(l3d_line3d* h, int on, double dist_px, double angle_deg, double max_gap, int max_rounds);
int l3d_line3d_get_merging(const l3d_line3d* h, int32_t* counts /* 8 */, int32_t* final_index, int32_t* n_sources);
/* inspection (tests): what a refinement of the current result is fed with, in the normalised frame -- counts[3] = lines, members, cameras; then (any may be
 * NULL; sizes from a first call) group_start (lines + 1), member_cam, member_seg (4 each), member_pts (6 each), cameras (12 each, views in ascending id), and
 * Line3D::inverseTransform (line3D.cc:1782-1786) as transform[13] = Rinv (9, row-major), scale_inv, tneg (3): X = Rinv (P scale_inv + tneg). */
int l3d_line3d_refinement_input(l3d_line3d* h, int32_t* counts, int32_t* group_start, int32_t* member_cam, float* member_seg, double* member_pts, double* cameras,
                                double* transform);
/* step-wise matchViews for view sharding: begin; for each view in match_order: compute a source-segment
 * range, (all-gather), commit the merged kept list; end. */
int l3d_line3d_match_begin(l3d_line3d* h, int* n_order);
int l3d_line3d_match_order(l3d_line3d* h, uint32_t* view_ids, int* n_segments);
int l3d_line3d_view_num_to_be_matched(l3d_line3d* h, uint32_t view_id);
int l3d_line3d_match_view_compute(l3d_line3d* h, uint32_t view_id, int seg_begin, int seg_end,
                                  l3d_match** out, int* n_out, float* median, float** best_depths, int* n_best);
int l3d_line3d_match_view_commit(l3d_line3d* h, uint32_t view_id, const l3d_match* matches, int n,
                                 const float* best_depths, int n_best, float median);
int l3d_line3d_match_end(l3d_line3d* h);
/* matchViews as the resident chain sharded over ranks: the facade builds the static schedule and forwards to
 * l3d_shard_chain_* (same protocol: enqueue -> caller's all-gather -> mark; fetch = this rank's host bookkeeping) */
int l3d_line3d_shard_open(l3d_line3d* h, int rank, int world, int slot_records, int* n_views, size_t* slot_bytes);
int l3d_line3d_shard_view_verified(l3d_line3d* h, int k);
int l3d_line3d_shard_enqueue(l3d_line3d* h, int k, void* send_slot, const void* gathered_base);
int l3d_line3d_shard_mark(l3d_line3d* h, int k);
int l3d_line3d_shard_fetch(l3d_line3d* h, int k);
int l3d_line3d_shard_close(l3d_line3d* h, int committed);
/* open -> run -> close in one call (l3d_shard_chain_run); commit: 0 = this rank only computes and exchanges; 1 = it also does the
 * host bookkeeping (kept lists handed to the host view by view: the round-2 protocol, one rank of the job); 2 = it builds matchViews'
 * products on its device from the gathered slots (l3d_shard_chain_products) -- any number of ranks, no list leaves the device, the
 * rest of compute3Dmodel runs on the resident tables as after the single-GPU chain; 3 = as 2, partitioned: the rank keeps the records and
 * builds the rows of ITS block of views only (l3d_shard_chain_partition), l3d_line3d_finish_sharded follows on every rank.
 * gathered_out (optional) receives the device address of the gathered blocks (valid until the next chain) */
int l3d_line3d_shard_run(l3d_line3d* h, int rank, int world, int slot_records, l3d_exchange_fn exchange, void* exchange_user, int commit,
                         const void** gathered_out, size_t* slot_bytes_out);
/* matchViews with the VIEWS sharded over the ranks in blocks, each block started cold a few neighbour windows early, the speculation verified
 * (l3d_match_chain_blocks above; warmup_views < 0: eight windows; a block whose speculation fails all the same is re-run warm, not the pass).  *verdict = 0: this rank holds matchViews' products as after the
 * single-GPU resident chain -- compute3Dmodel goes on from there (l3d_line3d_finish); *verdict = 1 (identical on every rank): the speculation
 * did not hold, nothing was committed, run l3d_line3d_shard_run. */
int l3d_line3d_block_run(l3d_line3d* h, int rank, int world, int warmup_views, l3d_exchange_fn exchange, void* exchange_user, int* verdict);
/* matchViews sharded by blocks of views with NOTHING replicated (l3d_match_chain_partition; warmup_views < 0: eight windows), and the rest of
 * compute3Dmodel as a COLLECTIVE of the job's ranks: greedy selection on the views a rank holds, the affinity fill sharded by source key
 * (l3d_affinity_fill_sharded), then -- every rank from the same affinity list -- diffusion, clustering, line fit: every rank ends with the whole
 * result (Line3D::getResult).  l3d_line3d_finish on such an object is the same call with the exchange of the run; l3d_line3d_view_matches serves the
 * views this rank holds.  exchange == NULL in finish_sharded: the one the run was given. */
int l3d_line3d_partition_run(l3d_line3d* h, int rank, int world, int warmup_views, l3d_exchange_fn exchange, void* exchange_user, int* verdict);
int l3d_line3d_finish_sharded(l3d_line3d* h, int perform_diffusion, l3d_exchange_fn exchange, void* exchange_user);
/* performClustering (clustering.h:125, clustering.cc:6-47) on the host (fallback and cross-check of l3d_perform_clustering_device): labels[k] = CLUniverse::find(k) */
int l3d_perform_clustering(const l3d_edge* edges, int n_edges, int num_nodes, float c, int32_t* labels);
/* Line3D::getResult (line3D.cc:377-381), flattened; Line3D::getSegment2D (line3D.cc:2004-2013) */
int l3d_line3d_result_sizes(const l3d_line3d* h, int* n_lines, int* n_seg3d, int* n_seg2d);
int l3d_line3d_get_result(const l3d_line3d* h, int* line_n3d, int* line_n2d, double* seg3d, uint32_t* seg2d);
int l3d_line3d_get_segment2D(const l3d_line3d* h, uint32_t cam, uint32_t seg, float out[4]);
/* Line3D::save3DLinesAsSTL / save3DLinesAsTXT (line3D.h:91-95, line3D.cc:384-473; TXT format README.txt:177-185) for
 * the current result, with the reference's number formatting ("%e" / stream default = "%g") */
#define L3D_FORMAT_STL 0
#define L3D_FORMAT_TXT 1
int l3d_line3d_save_result(const l3d_line3d* h, const char* filename, int format);
/* inspection */
/* 1: matchViews through one l3d_compute_pairwise_matches call per view (the reference's control flow);
 * 0 (default): the device-resident chain (l3d_match_chain).  Results are identical. */
int l3d_line3d_set_sync_matching(l3d_line3d* h, int on);
int l3d_line3d_keep_view_matches(l3d_line3d* h, int on);
/* which way the last l3d_line3d_match_views took: 0 = the resident chain (products on the device), 1 = the chain with host bookkeeping, 2 = per-view
 * seam calls on request (set_sync_matching), 3 = per-view seam calls because the schedule is not static (an early-return view's local camera
 * numbers name a view that still accepts reverse matches, line3D.cc:844-845); -1 = matchViews has not run */
int l3d_line3d_match_path(const l3d_line3d* h);
int l3d_line3d_view_matches(const l3d_line3d* h, uint32_t view_id, const l3d_match** m, int* n, float* median);
int l3d_line3d_affinity(const l3d_line3d* h, const l3d_edge** A, int* nnz, int* n_nodes);
/* the device-resident products of the last matchViews (l3d_match_chain_resident) and, after finish, the hypothesis table of
 * greedySelection, copied to the host for inspection: sizes first (0 views: no resident products -- sync / host-bookkeeping /
 * sharded matching), then the arrays (any pointer may be NULL): seg_base n_views + 1, pot_start n_dense + 1, pot_tgt n_pot,
 * best n_dense (segID1 == 0xffffffff: none), hyp / score n_hyp */
int l3d_line3d_products_sizes(const l3d_line3d* h, int* n_views, int* n_dense, int64_t* n_pot, int* n_hyp);
int l3d_line3d_products_get(l3d_line3d* h, int32_t* seg_base, int64_t* pot_start, int32_t* pot_tgt, l3d_match* best, l3d_hypothesis* hyp, float* score);
/* per chain view (the index of l3d_chain_kept_list) of the last matchViews with resident products: what the builder reported (kept / candidate counts,
 * median depth; a partitioned job: the views this rank holds, zero elsewhere).  The array belongs to h and stays valid until the next matchViews;
 * *n = 0 without resident products.  Kept counts are per view: their sum -- the arena -- may exceed 2^32 */
int l3d_line3d_chain_summary(const l3d_line3d* h, const l3d_chain_summary** summary, int* n);
int l3d_line3d_stats(const l3d_line3d* h, double* stats12);

/* =================================================================================================
 * SfM front ends of the reference's drivers: VisualSfM NVM (main_vsfm.cpp:121-223) and bundler
 * bundle.rd.out (main_bundler.cpp:110-204), reduced to what feeds Line3D::addImage -- focal length, R, t, distortion
 * coefficients, observed world point ids per camera.  The images themselves: baseline JPEG files are decoded, undistorted and their line segments
 * detected on the device (l3d_line3d_add_image_jpeg, l3d_decode_jpeg, l3d_undistort_image, l3d_detect_segments below).
 * A failed read still returns a scene object carrying the message (l3d_sfm_last_error); free it with l3d_sfm_free.
 * ================================================================================================= */
typedef struct l3d_sfm_scene l3d_sfm_scene;
int l3d_sfm_read_nvm(const char* path, l3d_sfm_scene** out);
int l3d_sfm_read_bundler(const char* path, l3d_sfm_scene** out);
void l3d_sfm_free(l3d_sfm_scene* scene);
const char* l3d_sfm_last_error(const l3d_sfm_scene* scene);
int l3d_sfm_num_cameras(const l3d_sfm_scene* scene);
int l3d_sfm_num_points(const l3d_sfm_scene* scene);
int l3d_sfm_camera(const l3d_sfm_scene* scene, int i, double* focal, double dist[2], double R[9], double t[3], int* n_worldpoints);
/* the camera's radial coefficients (k1, k2) in OpenCV's convention, as the drivers hand them to initUndistortRectifyMap -- what the
 * *_distorted calls below take.  A scene read from an NVM file: k1 = -d, k2 = 0 (main_vsfm.cpp:259); from a bundler file: k1 = d1,
 * k2 = d2 (main_bundler.cpp:273-274); d, d1, d2 as l3d_sfm_camera returns them */
int l3d_sfm_camera_cv_distortion(const l3d_sfm_scene* scene, int i, double k[2]);
const char* l3d_sfm_camera_name(const l3d_sfm_scene* scene, int i);
int l3d_sfm_camera_worldpoints(const l3d_sfm_scene* scene, int i, uint32_t* ids);
/* A COLMAP model (a sparse reconstruction's folder): cameras.bin + images.bin when both are there, else cameras.txt + images.txt; points3D is not
 * needed.  A camera of the scene is one IMAGE of the model, in the file's order: R from its world-to-camera quaternion (w, x, y, z), t as it is --
 * what addImage takes --, its name, and as world point ids the POINT3D_IDs of its observations that are not -1 (l3d_sfm_num_points: the largest
 * id + 1).  The accessors above work on such a scene; focal is the model's f, or fx where it has two; l3d_sfm_camera's dist and
 * l3d_sfm_camera_cv_distortion answer for SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL and RADIAL with fx == fy ((0, 0), (k, 0), (k1, k2)) and are
 * L3D_ERR_UNSUPPORTED for the others.  The models and their parameters, in the file's order:
 *     SIMPLE_PINHOLE f cx cy | PINHOLE fx fy cx cy | SIMPLE_RADIAL f cx cy k | RADIAL f cx cy k1 k2 | OPENCV fx fy cx cy k1 k2 p1 p2 |
 *     OPENCV_FISHEYE fx fy cx cy k1 k2 k3 k4 | FULL_OPENCV fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 | FOV fx fy cx cy omega |
 *     SIMPLE_RADIAL_FISHEYE f cx cy k | RADIAL_FISHEYE f cx cy k1 k2 | THIN_PRISM_FISHEYE fx fy cx cy k1 k2 p1 p2 k3 k4 sx1 sy1
 *   l3d_sfm_camera_model   the image's camera as the file has it: the model's name, its parameters (n of them), untouched
 *   l3d_sfm_camera_lens    the l3d_lens (see A LENS, below) and K of the image's camera, and its size.  THE PIXEL CENTRE: COLMAP puts the centre of
 *                          the top-left pixel at (0.5, 0.5), the formulas here -- like remap -- at (0, 0): the lens and K carry cx - 0.5, cy - 0.5.
 *                          The pinhole and radial models give BROWN, the three fisheye models FISHEYE; FOV and THIN_PRISM_FISHEYE read fine but
 *                          have no lens here: L3D_ERR_UNSUPPORTED, the message (l3d_sfm_last_error) naming the model.  On an NVM or bundler scene:
 *                          BROWN with the l3d_sfm_camera_cv_distortion coefficients, a zero source camera ("the output camera"), K zeroed and size 0
 * Refused with a message on the scene object, L3D_ERR_INVALID: a missing or truncated file, a model id or name that is not of the list, a camera id
 * without a camera, counts that the file cannot hold. */
struct l3d_lens;
int l3d_sfm_read_colmap(const char* model_dir, l3d_sfm_scene** out);
int l3d_sfm_camera_model(const l3d_sfm_scene* scene, int i, const char** name, const double** params, int* n);
int l3d_sfm_camera_lens(l3d_sfm_scene* scene, int i, struct l3d_lens* lens, double K[9], int* width, int* height);
int l3d_sfm_camera_id(const l3d_sfm_scene* scene, int i);      /* the COLMAP camera id of image i; -1 on another kind of scene */
/* the drivers' K from a focal length and the image size (main_vsfm.cpp:232-241): [[f,0,w/2],[0,f,h/2],[0,0,1]] */
void l3d_sfm_intrinsics(double focal, unsigned int width, unsigned int height, double K[9]);

/* =================================================================================================
 * Segment cache of Line3D::addImage: "<data dir>/segments_<id>_<w>x<h>_coll<0|1>.bin" (line3D.cc:143-150),
 * a boost binary archive of one L3DSegments -- the collinearity map, then the DataArray<float>* of padded rows
 * (serialization.h:49-69, segments.h:124-131, dataArray.h:296-318) -- read and written without boost
 * (layout and its pin status: line3d_amd/csrc/l3d_segcache.cpp).  A failed read still returns an object carrying the
 * message (l3d_segment_cache_last_error); free it with l3d_segment_cache_free.
 * Collinearities are the DIRECTED entries of segment2collinearities_ (i -> j and j -> i), ascending (i, j).
 * ================================================================================================= */
typedef struct l3d_segment_cache l3d_segment_cache;
int l3d_segment_cache_filename(uint32_t image_id, unsigned int width, unsigned int height, int use_collinearity, char* out, size_t out_size);
int l3d_segment_cache_read(const char* path, l3d_segment_cache** out);
void l3d_segment_cache_free(l3d_segment_cache* cache);
const char* l3d_segment_cache_last_error(const l3d_segment_cache* cache);
int l3d_segment_cache_num_segments(const l3d_segment_cache* cache);
int l3d_segment_cache_num_collinearities(const l3d_segment_cache* cache);
int l3d_segment_cache_library_version(const l3d_segment_cache* cache);
int l3d_segment_cache_get(const l3d_segment_cache* cache, float* segments, int32_t* ci, int32_t* cj, float* cw);
int l3d_segment_cache_write(const char* path, const float* segments, int n_segments, const int32_t* ci, const int32_t* cj, const float* cw,
                            int n_collinearities, int library_version);
/* Line3D::addImage when the cache file exists (line3D.cc:160-168): the segments AND the collinearities of the file are
 * used as they are (nothing is recomputed); world points as in l3d_line3d_add_image */
int l3d_line3d_add_image_cached(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height, const l3d_segment_cache* cache,
                                const double* K, const double* R, const double* t, const uint32_t* worldpoint_ids, int n_worldpoints);

/* Line3D::addImage / addImage_fixed_sim with the reference's cache behaviour (line3D.cc:128-199, 253-324): the cache file of the
 * view is "<data_directory>/segments_<id>_<w'>x<h'>_coll<0|1>.bin" with (w', h') the image size after the max_img_width
 * down-scaling the detector would have worked at (line3D.cc:133-138; the view itself keeps the original size).
 *   file exists, load_and_store == 0   the file is removed (line3D.cc:153-156), `segments` are used
 *   file exists, load_and_store != 0   segments AND collinearities come from the file, `segments` are ignored (:159-168)
 *   otherwise                          `segments` are used; with load_and_store != 0 the cache is written (:180-182) -- at
 *                                      prepare(), when the collinearities of all new views have been computed in one batch
 * `segments` is what detectLineSegments (line3D.cc:1789-1871: LSD, length filter, longest 3000) would have produced, e.g. by
 * l3d_detect_segments; l3d_line3d_add_image_pixels does both steps.
 * links: observed world point ids (add_image_ex) or (view id, similarity) pairs (add_image_fixed_sim_ex). */
int l3d_line3d_add_image_ex(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height, const float* segments, int n_segments,
                            const double* K, const double* R, const double* t, const uint32_t* worldpoint_ids, int n_worldpoints,
                            const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_image_fixed_sim_ex(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height, const float* segments, int n_segments,
                                      const double* K, const double* R, const double* t, const uint32_t* sim_ids, const float* sims, int n_sims,
                                      const char* data_directory, int max_img_width, int load_and_store);

/* =================================================================================================
 * Line segment detection on the device (line3d_amd/csrc/l3d_detect.hip): what Line3D::detectLineSegments (line3D.cc:1789-1871)
 * does with the LSD detector (scale 0.8, sigma_scale 0.6, quant 2, ang_th 22.5 deg, log_eps 0, density_th 0.7).
 *   pixels      8-bit, `channels` = 1 or 3 interleaved, rows `row_stride` bytes apart (>= width x channels)
 *   rescale     when (new_width, new_height) differs from (width, height) (0, 0 = no rescale): bilinear, half-pixel centres, 8-bit
 *               weights.  Per axis, output index i of n_out from n_in samples: num = max((2 i + 1) n_in - n_out, 0), den = 2 n_out,
 *               i0 = num / den, a = ((num % den) 256 + den / 2) / den, and i0 = n_in - 1, a = 0 at the last sample; per channel
 *               v = ((256-a)(256-b) p00 + a (256-b) p01 + (256-a) b p10 + a b p11 + 32768) >> 16.  Output coordinates are multiplied by
 *               upscale_factor = 1 / (0.5 (new_width / width + new_height / height)) (float): they are original-image pixels
 *   grey        3 channels, the way CV_RGB2GRAY sees the buffer: (299 c0 + 587 c1 + 114 c2 + 500) / 1000 (integers).  Parity with
 *               OpenCV's fixed-point resize / convert is NOT claimed
 *   detection   Gaussian sub-sampling, 2x2 gradient, level-line angle, line-support regions, rectangle by gradient-weighted
 *               moments, density check, NFA with logNT = 5/2 (log10 X + log10 Y) + log10 11, output offset + 0.5, / scale.
 *               The reference's region growing is a sequential greedy loop; the regions here are formed in parallel, without a seed
 *               order.  The result AGREES with the reference detector (recall and precision pooled over the golden images are
 *               held to the reference's own worst single-image repeatability under redrawn noise, tests/test_gpu_detect.py);
 *               it is not identical to it.  It is deterministic: the same pixels give the same bytes
 *   selection   length > min_length, length descending (ties: smallest pixel index of the region), at most max_segments
 * Out (callee-allocated, l3d_free): 4 floats (x1, y1, x2, y2) per segment; *n = 0 when nothing is found.
 * Images below 8x8, channels other than 1 or 3, a stride below width x channels: L3D_ERR_INVALID.
 * Still outside the library: PNG and progressive JPEG decoding (baseline JPEG: l3d_decode_jpeg below), the tclap command lines of the drivers.
 * ================================================================================================= */
int l3d_detect_segments(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                        float min_length, int max_segments, float** segments, int* n);
/* Undistortion on the device (k_det_undistort, l3d_undistort.hip): what the drivers do to an image before addImage sees it
 * (main_vsfm.cpp:243-270, main_bundler.cpp:256-284): cv::initUndistortRectifyMap(K, dist, I, K) + cv::remap(INTER_LINEAR, BORDER_CONSTANT),
 * same size, same K.  fx, fy, cx, cy: the camera; k1, k2: OpenCV-convention radial coefficients (tangential terms and k3 are zero in both
 * drivers; a scene file's own numbers become k1, k2 by l3d_sfm_camera_cv_distortion).  For output pixel (column j, row i), in double:
 *     x = (j - cx) / fx            y = (i - cy) / fy
 *     r2 = x x + y y               kr = 1 + (k2 r2 + k1) r2
 *     u = fx (x kr) + cx           v = fy (y kr) + cy
 * u not in (-1, width) or v not in (-1, height) (NaN included; tested before any conversion to an integer): 0 in every channel.
 * Otherwise, per channel:
 *     iu = rint(32 u), iv = rint(32 v)           (nearest, ties to even)
 *     x0 = floor(iu / 32), a = iu - 32 x0        (a in 0..31 for negative iu as well); y0, b from iv likewise
 *     out = ((32-a)(32-b) p(y0,x0) + a (32-b) p(y0,x0+1) + (32-a) b p(y0+1,x0) + a b p(y0+1,x0+1) + 512) >> 10
 * with a tap outside the image counting as 0 (BORDER_CONSTANT, black).  This is remap's arithmetic on the 16SC2 fixed-point maps of the
 * drivers' call: 5 fractional bits per coordinate, bilinear weights in 1/32768 -- exact for these products.  Byte identity with OpenCV is
 * NOT claimed: OpenCV accumulates x incrementally along a row, so a pixel can differ where 32 u or 32 v falls within rounding of a half-integer.
 * Both |k1| and |k2| <= 1e-12 (L3D_EPS, commons.h:66, the drivers' condition): nothing is launched, the pixels pass through untouched.
 * Undistortion, rescale and grey stay three 8-bit roundings, like remap -> resize -> cvtColor.
 *   l3d_undistort_image            host in, host out (`out`: height rows of width x channels bytes, `out_row_stride` apart; may be `pixels`
 *                                  itself with the same stride).  An image below 1x1, channels other than 1 or 3, a stride below
 *                                  width x channels, fx or fy zero or not finite: L3D_ERR_INVALID
 *   l3d_detect_segments_distorted  l3d_detect_segments with the undistortion between the upload and the rescale; the segments are in
 *                                  pixels of the undistorted image */
int l3d_undistort_image(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx, double cy,
                        double k1, double k2, unsigned char* out, size_t out_row_stride);
int l3d_detect_segments_distorted(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                                  float min_length, int max_segments, double fx, double fy, double cx, double cy, double k1, double k2, float** segments, int* n);
/* A LENS: undistortion with tangential, rational and fisheye models, onto a camera matrix of the caller's choice (k_det_undistort_lens,
 * l3d_undistort.hip).  The calls above know two radial coefficients and resample onto the same camera; the ..._lens calls take an l3d_lens and an
 * OUTPUT camera (fx', fy', cx', cy') -- at context level four doubles, in the add family the entry's K, which is also the view's K.  The lens
 * carries the SOURCE camera, that of the distorted image; fx == 0 && fy == 0 there says "the output camera".  When the two differ the image is
 * resampled onto the new camera matrix, at the same size: that is what makes a fisheye usable, the caller can zoom out (fx' < fx).  Another
 * output size, cropping and choosing the new matrix automatically: A REMAP, below.
 * For output pixel (column j, row i), in double, nothing fused, in this order of operations:
 *     x = (j - cx') / fx'      y = (i - cy') / fy'      r2 = x x + y y
 *     BROWN:    num = 1 + ((k3 r2 + k2) r2 + k1) r2      den = 1 + ((k6 r2 + k5) r2 + k4) r2      kr = num / den
 *               xd = x kr + ((2 p1) x y + p2 (r2 + 2 (x x)))
 *               yd = y kr + (p1 (r2 + 2 (y y)) + (2 p2) x y)
 *     FISHEYE:  r = sqrt(r2)   th = atan(r)   t2 = th th
 *               td = th (1 + (((k4 t2 + k3) t2 + k2) t2 + k1) t2)
 *               s = r > 1e-8 ? td / r : 1      xd = x s      yd = y s
 *     u = fx xd + cx           v = fy yd + cy            (fx, fy, cx, cy: the source camera)
 * (products run left to right: (2 p1) x y is ((2 p1) x) y).  The rest is the rule above, word for word: u not in (-1, width) or v not in
 * (-1, height) (NaN included -- a rational lens whose denominator crosses zero gives inf and NaN; tested before any conversion to an integer): 0 in
 * every channel; otherwise iu = rint(32 u), iv = rint(32 v), the four taps weighted in 1/1024, black outside.  Division and square root are IEEE;
 * atan is the one operation whose bits the device does not share with a host libm (tests/lens_model.py holds its cases to a margin that a few ulp
 * cannot cross).  BROWN with p1 = p2 = k3..k6 = 0 and the source camera equal to the output camera performs exactly the operations of the rule
 * above (0 r2 + k2, num / 1 and x kr + 0 are exact): it gives the same bytes.
 * Pass-through: a BROWN lens whose eight coefficients all lie within 1e-12, with equal cameras, launches nothing.  A FISHEYE lens is always active
 * (zero coefficients are the equidistant projection, not the identity).
 * Refused before anything is launched: an unknown model, a field that is not finite, exactly one of fx, fy zero, an output fx' or fy' that is
 * zero or not finite, a non-zero k[4..7] on FISHEYE: L3D_ERR_INVALID.  Skew K[1] != 0 with an active lens (the add family and
 * l3d_line3d_undistort_image_lens, which take K): L3D_ERR_UNSUPPORTED, as with dist.  An entry that carries both dist (at context level: a camera
 * whose k1 or k2 is not zero) and a lens: L3D_ERR_INVALID.
 *   l3d_undistort_image_lens              l3d_undistort_image with a lens; in place allowed
 *   l3d_undistort_image_device_lens       l3d_undistort_image_device with a lens
 *   l3d_detect_segments_batch_lens, l3d_detect_segments_device_batch_lens
 *                                         the batch calls with, beside the entry array, an array of n lens pointers (the array or an element may be
 *                                         NULL: the entry's own camera rule).  With a lens the entry's camera must be given: its fx, fy, cx, cy are the
 *                                         output camera, its k1, k2 must be 0.  One chunk may mix models, lens-less images and k1, k2 cameras: a chunk
 *                                         in which every camera is of the k1, k2 kind (or absent) launches k_det_undistort as before, any other chunk
 *                                         launches k_det_undistort_lens once (a k1, k2 camera goes in as BROWN: the same bytes).  A single image is a
 *                                         batch of one
 *   l3d_line3d_add_image_entry_lens, l3d_line3d_add_images_lens, l3d_line3d_add_device_entry_lens, l3d_line3d_add_device_images_lens
 *                                         THE ADD FAMILY (below) with the lens in the place of dist in step 1 of the ONE ROUTE
 *   l3d_line3d_undistort_image_lens       l3d_undistort_image_lens with the object's device and K */
enum { L3D_LENS_BROWN = 1, L3D_LENS_FISHEYE = 2 };
typedef struct l3d_lens {
    int model;               /* L3D_LENS_BROWN, L3D_LENS_FISHEYE; 0 is invalid: a zeroed struct is refused */
    double fx, fy, cx, cy;   /* the SOURCE camera (of the distorted image); fx == 0 && fy == 0: the output camera */
    double k[8];             /* BROWN: k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order);  FISHEYE: k1 k2 k3 k4, the rest must be 0 */
} l3d_lens;
int l3d_undistort_image_lens(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx,
                             double cy, const l3d_lens* lens, unsigned char* out, size_t out_row_stride);
/* A REMAP: undistortion onto a PLANNED camera and ANOTHER SIZE, with a VALIDITY PLANE (l3d_remap_plan.cpp; k_det_undistort_remap, l3d_undistort.hip).
 *
 * THE PLANNER, l3d_undistort_plan: host code in double, no context and no device.  lens: a lens WITH its source camera (fx, fy > 0); model 0 means
 * a pinhole camera (the coefficients are not read).  width, height: the source image.
 *   Border points: every pixel (j, i) on the four edges of the source image, 2 (w + h) - 4 of them.  xd = (j - cx) / fx, yd = (i - cy) / fy, and
 *   the distortion is inverted:
 *     BROWN    Newton on the two forward formulas of A LENS with their analytic Jacobian, from (x, y) = (xd, yd);
 *     FISHEYE  Newton on theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8) = sqrt(xd^2 + yd^2), from theta = that value; then
 *              r = tan(theta) and (x, y) = (xd, yd) r / sqrt(xd^2 + yd^2)  (below 1e-8: (xd, yd)).
 *   An iteration ends with the first step whose components are all within 1e-12, after at most 50 steps.  A point cannot be used as it is when the
 *   iteration does not end that way or takes a step that is not finite; when the Jacobian's determinant (FISHEYE: the derivative of the left side)
 *   is not positive at the solution or at one of the 15 points that divide the segment from the optical axis to the solution into 16 equal parts
 *   -- the lens folds over, its radial function is not monotone --; when the solution lies on the other side of the axis (x xd + y yd < 0);
 *   when theta is outside [0, pi/2); or when the undistorted radius exceeds r_max = tan(fov_max_deg / 2 in radians).  Such a point is CLAMPED to radius r_max: along its own direction when only
 *   the radius is too large, along (xd, yd) otherwise.  fov_max_deg = 120 is the bindings' default: a choice (beyond it a rectilinear image spends
 *   most of its pixels on the periphery), not a measurement.
 *   Rectangles in normalised coordinates: OUTER, min and max of x and of y over all border points; INNER, max of x over the left edge, min of x over
 *   the right edge, max of y over the top edge, min of y over the bottom edge.  alpha in [0, 1] interpolates the four bounds linearly, 0 = inner
 *   (no blank pixel in the output), 1 = outer (every source pixel inside the limit is kept): l, r, t, b.
 *   The output camera: fy' = fx' (fy / fx) -- the pixel aspect is kept --, and all extents are measured between PIXEL CENTRES (an output of w'
 *   columns spans (w' - 1) / fx'), so that a camera without distortion gets its own K back at its own size:
 *     fx'(0) = max((w' - 1) / (inner r - inner l), (h' - 1) / ((fy / fx) (inner b - inner t)))     the smallest that keeps the output inside the inner rectangle
 *     fx'(1) = min((w' - 1) / (outer r - outer l), (h' - 1) / ((fy / fx) (outer b - outer t)))     the largest that keeps the outer rectangle inside the output
 *     fx' = fx'(0) + alpha (fx'(1) - fx'(0))
 *     cx' = (w' - 1) / 2 - fx' (l + r) / 2          cy' = (h' - 1) / 2 - fy' (t + b) / 2
 *   The output size: (out_width, out_height) as given; (0, 0): the source size; (-1, -1): the size at which fx' = fx (COLMAP's behaviour) --
 *   then fx' = fx, w' = floor(fx' (r - l) + 1e-6) + 1, h' = floor(fy' (b - t) + 1e-6) + 1, and when max_dim > 0 and one of them exceeds it,
 *   fx' = fx max_dim / max(w', h') and both are computed again.
 *   Refused, L3D_ERR_INVALID with the cause in l3d_undistort_plan_error() (per thread): a null argument; a lens that A LENS refuses or that has no
 *   positive source camera; alpha outside [0, 1]; fov_max_deg outside (0, 180); a negative max_dim; another combination of out_width, out_height;
 *   a degenerate rectangle (inner r <= inner l or inner b <= inner t); a source or output size below 8 in a direction, above 2^24, or of more
 *   than 2^31 bytes at three channels (the detector's limits).
 *
 * THE RESAMPLING, k_det_undistort_remap: one thread per pixel of the OUTPUT, w' x h' (32 x 8 blocks, the image in blockIdx.z), the source w x h.
 * The map, the inside test and the taps are A LENS's word for word with (j, i) running over the output and (fx', fy', cx', cy') the output camera.
 * Beside the pixel the kernel writes ONE BYTE OF VALIDITY: a pixel is valid iff the inside test passed, every tap with a non-zero weight lies
 * inside the source, and -- where the caller gave a mask in the source grid -- every such tap is non-zero in the mask.  A pixel outside is written 0
 * as before; a pixel inside is written as A LENS writes it, valid or not.  border_mask == 0 leaves the first two conditions out: only the
 * caller's mask makes a pixel invalid.
 *   l3d_remap.lens        NULL: nothing is resampled, the mask is the validity plane (out size: 0 or the source's).  model 0, or BROWN with every
 *                         coefficient within 1e-12: a pinhole camera -- with the cameras and the sizes equal nothing is launched, otherwise the
 *                         image is resampled through the same kernel
 *   out_width, out_height the output size; both 0: the source's.  A size that differs from the source's without a lens: L3D_ERR_INVALID
 *   mask                  NULL, or width x height bytes in the SOURCE grid, rows mask_row_stride bytes apart, non-zero = valid.  mask_width and
 *                         mask_height state the plane's extent: they must be the source image's (a file's: its headers'), else L3D_ERR_INVALID
 *                         before anything is read -- the library reads width x height bytes and has no other way to know.  mask_on_device: it
 *                         is device memory (checked as an l3d_device_image is: memory kind and extent, L3D_ERR_INVALID), else host memory
 *   l3d_undistort_image_remap, l3d_undistort_image_device_remap
 *                         out: out_width x out_height pixels of the input's channels.  valid: NULL, or the validity plane, one byte per output
 *                         pixel, 255 = valid and 0 = invalid (the device call: a one-channel L3D_U8 image of the output size).  The calls with a
 *                         lens and without out size, mask or validity output are l3d_undistort_image[_device]_lens.
 *
 * THE VALIDITY PLANE THROUGH THE DETECTOR (k_det_valid_grey, k_det_valid_x, k_det_valid_y, k_det_valid_apply).  One rule: A GRADIENT PIXEL IS
 * UNDEFINED IF ANY PIXEL THAT CONTRIBUTED TO ITS VALUE IS INVALID.  The plane is carried beside the pixel stages, one AND over each stage's taps:
 *     the rescale     where the detector rescales, the 2 x 2 taps of the rescale's rule whose weight ((256 - a) or a, times (256 - b) or b) is not
 *                     zero; otherwise the pixel itself
 *     the sampler     the 7 taps about the centre xc = floor(x / 0.8 + 0.5) of every output column, then the 7 about yc of every output row, an
 *                     index outside the image reflected as the sampler reflects it (symmetric boundary)
 *     the gradient    the 2 x 2 stencil (x, y), (x + 1, y), (x, y + 1), (x + 1, y + 1), clipped at the last column and row
 * and one kernel behind the gradient gives an undefined pixel what a pixel below the gradient threshold has: magnitude 0, no angle, no bucket,
 * inactive.  No line-support region starts at or grows into such a pixel; inside a candidate rectangle it counts as a point that is not aligned.
 * What the invalid pixels HOLD therefore cannot reach the segments.  The gradient kernel and everything behind it are unchanged, a call without a
 * remap launches what it launched before, and an all-valid plane gives the bytes of the call without one.
 *   l3d_detect_segments_batch_remap, l3d_detect_segments_device_batch_remap
 *                         the batch calls with, beside the entry array, an array of n remap pointers (the array or an element may be NULL: the
 *                         entry's own camera rule).  With a lens in the remap the entry's camera must be given: its fx, fy, cx, cy are the output
 *                         camera, its k1, k2 must be 0 (L3D_ERR_INVALID otherwise).  The detector sees the remap's OUTPUT: new_width, new_height,
 *                         min_length and the segments' pixel coordinates refer to it, and an output below 8 x 8 is refused as a source is.
 *                         Entries run together when their source sizes AND their output sizes (and working sizes) agree.  A chunk in which a
 *                         remap resamples an image launches k_det_undistort_remap once and neither of the other two undistortion kernels: a
 *                         plain lens and a k1, k2 camera go through it with the same bytes and an all-valid plane, an image without a camera
 *                         is copied.  A chunk whose remaps are masks alone resamples nothing: the masks are the planes.  A chunk without a remap
 *                         launches none of the new kernels.  A remap that asks for nothing (a lens alone, border_mask 0, no mask, the source's
 *                         size) is the ..._lens call.  A refused entry fails alone. */
typedef struct l3d_remap {
    const l3d_lens* lens;
    int32_t out_width, out_height;
    const void* mask;
    size_t mask_row_stride;
    int32_t mask_width, mask_height;
    int32_t mask_on_device;
    int32_t border_mask;
} l3d_remap;
int l3d_undistort_plan(const l3d_lens* lens, int width, int height, double alpha, int out_width, int out_height, int max_dim, double fov_max_deg,
                       double K_out[9], int* w_out, int* h_out);
const char* l3d_undistort_plan_error(void);
int l3d_undistort_image_remap(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, double fx, double fy, double cx,
                              double cy, const l3d_remap* remap, unsigned char* out, size_t out_row_stride, unsigned char* valid, size_t valid_row_stride);
/* (tests) host only, no context and no device: what the batch calls make of an entry with this camera (NULL, or fx, fy, cx, cy, k1, k2), lens and
 * remap (either may be NULL) for an image of width x height x channels -- the refusals above with their codes, the cause in msg (n bytes), or L3D_OK
 * with *route: 0 nothing is launched, 1 k_det_undistort, 2 k_det_undistort_lens, 3 k_det_undistort_remap; *plane: 1 when the image carries a
 * validity plane through the detector (a mask, or a remap that resamples); and the size the detector sees */
int l3d_test_undistort_route(const double* camera /* NULL or 6 */, const l3d_lens* lens, const l3d_remap* remap, int width, int height, int channels, int* route,
                             int* plane, int* out_width, int* out_height, char* msg, size_t n);
/* Line3D::addImage / addImage_fixed_sim from pixels (line3D.cc:95-217, 220-324): the image entry (THE ADD FAMILY, below) with pixels filled and no
 * dist.  The detector runs at the size the max_img_width rule gives, with min_length = 0.005 sqrt(rows^2 + cols^2) and at most 3000 segments. */
int l3d_line3d_add_image_pixels(l3d_line3d* h, uint32_t image_id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                const double* K, const double* R, const double* t, const uint32_t* worldpoint_ids, int n_worldpoints,
                                const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_image_pixels_fixed_sim(l3d_line3d* h, uint32_t image_id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                          const double* K, const double* R, const double* t, const uint32_t* sim_ids, const float* sims, int n_sims,
                                          const char* data_directory, int max_img_width, int load_and_store);
/* The same with the drivers' undistort block in front of the detector (main_vsfm.cpp:243-273): the entry with dist = (k1, k2) as above, which
 * may not be NULL here; fx, fy, cx, cy are K[0], K[4], K[2], K[5] of the full-resolution K the caller passes, which the view keeps (the drivers
 * undistort onto the same K).  l3d_line3d_undistort_image: l3d_undistort_image with the object's device and K. */
int l3d_line3d_add_image_pixels_distorted(l3d_line3d* h, uint32_t image_id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                          const double* K, const double* R, const double* t, const double dist[2], const uint32_t* worldpoint_ids, int n_worldpoints,
                                          const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_image_pixels_fixed_sim_distorted(l3d_line3d* h, uint32_t image_id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                                    const double* K, const double* R, const double* t, const double dist[2], const uint32_t* sim_ids, const float* sims,
                                                    int n_sims, const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_undistort_image(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K, double k1, double k2,
                               unsigned char* out, size_t out_row_stride);


/* =================================================================================================
 * Baseline JPEG input (line3d_amd/csrc/l3d_jpeg.cpp, l3d_jpeg_device.hip): the cv::imread in front of the drivers' undistort -> addImage block
 * (main_vsfm.cpp:229-273, main_bundler.cpp:242-287).  The host parses the file and decodes the entropy-coded data; dequantisation, inverse DCT,
 * chroma upsampling and colour conversion run on the device and write straight into the detector's pixel buffer.  The result is byte-identical
 * to the IJG / libjpeg-turbo decoder at its default settings (JDCT_ISLOW, fancy upsampling) -- the decoder behind cv::imread.
 * All arithmetic is in exact integers; >> is an arithmetic shift (a floor).
 *
 * Accepted   SOF0 and SOF1 with Huffman coding, 8-bit samples.  1 component: grey, 1 channel out.  3 components with sampling 1x1 for all, or
 *            luma 2x1 / 2x2 with chroma 1x1 (4:4:4, 4:2:2, 4:2:0).  DQT with 8- or 16-bit entries; DHT may be redefined between segments;
 *            DRI / RSTn are honoured (at each restart interval the decoder byte-aligns, checks RST m mod 8 and resets the DC predictors);
 *            fill bytes FF FF before markers; APPn / COM are skipped; anything after EOI is ignored and a missing EOI after the last MCU is
 *            accepted.  EXIF orientation is ignored: the SfM poses refer to the stored pixel grid.
 * Colour     libjpeg's rule: a JFIF APP0 means YCbCr; otherwise an Adobe APP14 decides by its transform byte (0: the components are R, G, B;
 *            1: YCbCr); otherwise component ids 'R', 'G', 'B' mean RGB; otherwise YCbCr.
 * Output     three components come out B, G, R INTERLEAVED -- what cv::imread hands the reference, whose CV_RGB2GRAY on that buffer
 *            (line3D.cc:1814) puts the weight 299 on blue; the grey formula of l3d_detect_segments on c0, c1, c2 reproduces exactly that for
 *            this buffer.  (An RGB buffer from elsewhere, e.g. a PPM, gets 299 on red, as before.)
 * Refused    L3D_ERR_UNSUPPORTED, the message naming the cause: progressive (SOF2), lossless, arithmetic coding, 12-bit; 2 or 4 components
 *            (CMYK / YCCK); any other sampling (1x2 / 4:4:0 / 4:1:1 included); more than one scan for a baseline frame.  Also a frame of more
 *            than 2^24 8x8 blocks over all components (about a gigapixel): decided from the headers, before anything is allocated.
 *            L3D_ERR_INVALID: truncated or corrupt data, a Huffman code not in the table, a coefficient index past 63, a DC predictor leaving
 *            the int16 range, a missing table, zero dimensions.  None of these reads or writes outside a buffer.
 * Coefficients  quantised, int16, de-zigzagged by the host into natural (row-major) order; per component, per block row, per block column,
 *            over whole MCUs.
 * Inverse DCT   c[k] = coef[k] q[k], then IJG's jidctint in 64-bit integers, constants at 13 bits: FIX(0.298631336) = 2446, (0.390180644) 3196,
 *            (0.541196100) 4433, (0.765366865) 6270, (0.899976223) 7373, (1.175875602) 9633, (1.501321110) 12299, (1.847759065) 15137,
 *            (1.961570560) 16069, (2.053119869) 16819, (2.562915447) 20995, (3.072711026) 25172.  A 1-D pass on v[0..7]:
 *              z1 = (v2 + v6) 4433; t2 = z1 - v6 15137; t3 = z1 + v2 6270; t0 = (v0 + v4) << 13; t1 = (v0 - v4) << 13;
 *              t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
 *              a0 = v7, a1 = v5, a2 = v3, a3 = v1; z1 = a0 + a3, z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3; z5 = (z3 + z4) 9633;
 *              a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299; z1 *= -7373; z2 *= -20995; z3 = z3 (-16069) + z5; z4 = z4 (-3196) + z5;
 *              a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4;
 *              out: t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3
 *            Pass 1 over the columns, each output (x + 1024) >> 11; pass 2 over the rows of that, each output
 *            clamp(((x + 131072) >> 18) + 128, 0, 255).  (libjpeg's range-limit table wraps where this clamps, but only for values no accepted
 *            stream produces: not part of the contract.)
 * Upsampling    the component's real size is cw = ceil(W h / hmax), chh = ceil(H v / vmax); edge samples replicate at that size, not at the
 *            padded MCU size.  2x1: out[2i] = (3 s[i] + s[i-1] + 1) >> 2, out[2i+1] = (3 s[i] + s[i+1] + 2) >> 2.  2x2: for output row 2r + k the
 *            neighbour row is nb = r - 1 (k = 0) or r + 1 (k = 1), replicated at top and bottom; t[i] = 3 s[r][i] + s[nb][i];
 *            out[2i] = (3 t[i] + t[i-1] + 8) >> 4, out[2i+1] = (3 t[i] + t[i+1] + 7) >> 4, t replicated at both row ends.
 * YCbCr -> RGB  cb' = cb - 128, cr' = cr - 128: R = y + ((91881 cr' + 32768) >> 16), B = y + ((116130 cb' + 32768) >> 16),
 *            G = y + ((-22554 cb' - 46802 cr' + 32768) >> 16), each clamped to 0..255; the output is cropped to W x H.
 *
 *   l3d_jpeg_info              headers only, no context and no device: width, height, channels (1 or 3) of the decoded image; the message of a
 *                              refusal: l3d_jpeg_last_error (of the calling thread's last context-free call)
 *   l3d_decode_jpeg            host bytes in, host pixels out (height rows of width x channels bytes, `out_row_stride` apart), any size from 1x1
 *   l3d_detect_segments_jpeg   l3d_detect_segments on the decoded image, which stays on the device; camera: NULL, or (fx, fy, cx, cy, k1, k2) of
 *                              l3d_detect_segments_distorted.  Images below 8x8 are refused as l3d_detect_segments refuses them
 *   l3d_line3d_add_image_jpeg, l3d_line3d_add_image_jpeg_fixed_sim
 *                              the image entry (THE ADD FAMILY, below) with the file in place of the pixels; dist may be NULL
 *   l3d_line3d_decode_jpeg     l3d_decode_jpeg with the object's device
 *   l3d_test_jpeg_coefficients (tests) host only: the quantised blocks as above (callee-allocated, l3d_free), qt[3][64] per component in natural
 *                              order, layout[27] = width, height, components, hmax, vmax, MCUs per row, MCU rows, restart interval, rgb, then per
 *                              component h, v, blocks per row, block rows, cw, chh
 * ================================================================================================= */
int l3d_jpeg_info(const unsigned char* bytes, size_t n, int* width, int* height, int* channels);
const char* l3d_jpeg_last_error(void);
int l3d_decode_jpeg(l3d_ctx* ctx, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride);
int l3d_detect_segments_jpeg(l3d_ctx* ctx, const unsigned char* bytes, size_t n, int new_width, int new_height, float min_length, int max_segments,
                             const double* camera, float** segments, int* n_segments);
int l3d_line3d_add_image_jpeg(l3d_line3d* h, uint32_t image_id, const unsigned char* bytes, size_t n, const double* K, const double* R, const double* t,
                              const double dist[2], const uint32_t* worldpoint_ids, int n_worldpoints, const char* data_directory, int max_img_width,
                              int load_and_store);
int l3d_line3d_add_image_jpeg_fixed_sim(l3d_line3d* h, uint32_t image_id, const unsigned char* bytes, size_t n, const double* K, const double* R, const double* t,
                                        const double dist[2], const uint32_t* sim_ids, const float* sims, int n_sims, const char* data_directory,
                                        int max_img_width, int load_and_store);
int l3d_line3d_decode_jpeg(l3d_line3d* h, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride);
int l3d_test_jpeg_coefficients(const unsigned char* bytes, size_t n, int16_t** coef, size_t* n_blocks, uint16_t* qt, int32_t* layout);

/* =================================================================================================
 * Images in batches: one pass of the detector over many images.
 *
 * l3d_detect_segments_batch   n entries, each 8-bit pixels (as l3d_detect_segments takes them) or, with pixels == NULL, a baseline JPEG file (as
 *                             l3d_detect_segments_jpeg takes it); camera: NULL, or (fx, fy, cx, cy, k1, k2) of l3d_detect_segments_distorted.
 *                             *segments (callee-allocated, l3d_free) holds the segments of all entries one after the other, those of entry i at
 *                             offsets[i] .. offsets[i + 1] (in segments of 4 floats; offsets has n + 1 places): BYTE FOR BYTE what the single call
 *                             gives for that entry alone, whatever else is in the batch and in whatever order.  Entries of the same sizes (width,
 *                             height, channels, new size) run through the detector together, in chunks: every stage is launched once per chunk
 *                             and the host waits once per look of the labelling and twice more per chunk, not per image.  A chunk holds as many
 *                             images as the option L3D_DET_BATCH_IMAGES allows (0: no limit of its own), as keep the chunk's scaled pixels within
 *                             2^30, and as fit half of the device memory that is free at the time; at most 1024.  status[i] is what the single
 *                             call would have returned for entry i: a refused entry (a progressive file, an image below 8x8, a corrupt entropy
 *                             stream ...) fails alone and has no segments, the others are not affected.  The call returns L3D_OK when the batch
 *                             was processed, else the code of a device failure (entries not finished by then carry it in their status);
 *                             l3d_last_error then holds one line per failed entry, "entry <i>: <message>".
 * l3d_line3d_add_images       THE ADD FAMILY, below
 * ================================================================================================= */
typedef struct l3d_detect_entry {
    const unsigned char* pixels; int width, height, channels; size_t row_stride;   /* or: */
    const unsigned char* jpeg; size_t jpeg_bytes;                                   /* pixels == NULL: a baseline JPEG file */
    int new_width, new_height; float min_length; int max_segments;
    const double* camera;                                                           /* NULL, or fx, fy, cx, cy, k1, k2 */
} l3d_detect_entry;
int l3d_detect_segments_batch(l3d_ctx* ctx, const l3d_detect_entry* e, int n, float** segments, int* offsets /* n + 1 */, int* status /* n */);
/* with remaps (A REMAP, above): remap NULL, or n pointers of which any may be NULL (then the entry's own camera rule) */
int l3d_detect_segments_batch_remap(l3d_ctx* ctx, const l3d_detect_entry* e, const l3d_remap* const* remap, int n, float** segments, int* offsets /* n + 1 */,
                                    int* status /* n */);
/* (tests) the defined / undefined plane of A REMAP, N x M bytes (255 = defined), that the last detector call of the context left for the first image
 * of its last chunk; *N = *M = 0 when that chunk carried no validity plane.  capacity: the bytes `defined` can take */
int l3d_test_detect_defined_plane(l3d_ctx* ctx, unsigned char* defined, size_t capacity, int* N, int* M);
/* with lenses (A LENS, above): lens NULL, or n pointers of which any may be NULL */
int l3d_detect_segments_batch_lens(l3d_ctx* ctx, const l3d_detect_entry* e, const l3d_lens* const* lens, int n, float** segments, int* offsets /* n + 1 */,
                                   int* status /* n */);

/* =================================================================================================
 * Images in DEVICE memory (line3d_amd/csrc/l3d_device_image.hip): a decoded video frame, a tensor, a GpuMat -- described where they lie and gathered
 * by one kernel (k_det_ingest, one launch per chunk of the batch detector) into the detector's pixel buffer, the place the upload of host pixels and
 * the JPEG kernels fill.  Nothing crosses the host.
 *
 * The descriptor.  Element (y, x, c) is at ptr + (y stride_y + x stride_x + c stride_c) sizeof(element); strides are in ELEMENTS and signed, 0 is
 * allowed (a broadcast channel).  One form covers H x W x C, C x H x W, cropped, strided and flipped views and one image of an N x ... batch.
 * channels is the SOURCE's: 1, 3 or 4.  A source of 1 channel gives the detector 1 channel, one of 3 or 4 gives it 3: detector channel k is read
 * from source channel chan[k] (ignored for channels == 1).  The detector applies CV_RGB2GRAY's weights to its buffer as it stands (`grey` above), so
 * an R, G, B tensor that must give the segments of the cv::imread (B, G, R) image passes chan = {2, 1, 0}.
 *
 * THE CONVERSION RULE to the detector's 8 bits, exact:
 *     L3D_U8                     copied as is (scale is ignored)
 *     L3D_U16, L3D_F16, L3D_F32  x converted to f32 (exact), y = x * scale (ONE f32 multiplication, nothing fused), r = rint(y) (ties to even),
 *                                NaN gives 0, the result is clamped to 0 .. 255
 * A tensor in [0, 1] passes scale = 255, a 16-bit image scale = 1 / 257.  The way back (k_det_egress, the ..._device output calls): U8 as is;
 * F32 (float)v * scale; F16 that f32 rounded to nearest even; U16 clamp(rint(v * scale), 0, 65535).  Output channel chan[k] receives detector
 * channel k; a fourth channel of the output is left as it is.
 *
 * Checked without a device (pure host functions):
 *   l3d_device_image_check    the fields: a size of at least 1x1 (the detector itself needs 8x8 and says so in l3d_detect_segments' words),
 *                             channels 1, 3 or 4, a dtype of the list, chan within the source's channels, scale finite (every dtype but U8).
 *                             L3D_ERR_INVALID with the cause in msg (n bytes, may be NULL)
 *   l3d_device_image_extent   *lo, *hi: the lowest and one past the highest BYTE offset from ptr the image addresses (only the channels of chan
 *                             count).  L3D_ERR_UNSUPPORTED when a product or the sum leaves 2^62 in magnitude, or width x height x 3 exceeds the
 *                             detector's 2^31; L3D_ERR_INVALID for fields l3d_device_image_check refuses
 * Checked BEFORE THE FIRST LAUNCH that reads or writes ptr (l3d_test_device_image_pointer is that routine alone: it returns the code and launches
 * nothing): hipPointerGetAttributes must say device memory of the context's device (a node object: rank 0's, where its detector runs) -- else
 * L3D_ERR_INVALID naming the kind of memory or both devices; and the extent must lie inside the allocation hipMemGetAddressRange reports for ptr --
 * else L3D_ERR_INVALID with the numbers.  Where the runtime reports no range for device memory (virtual-memory allocations) the extent check
 * is skipped.  Nothing is launched on a refusal.
 *
 * STREAM ORDER.  `stream` is the hipStream_t the pixels were produced on (NULL: the null stream).  Before the launch an event (one per context,
 * reused) is recorded on it and the context's stream waits for it: work enqueued there before the call is seen.  Every call taking a descriptor ends in
 * a synchronise of the context's stream: when it returns an input has been consumed and an output has been written -- the caller may reuse or
 * free the memory at once and read an output from any stream.
 *
 *   l3d_detect_segments_device        l3d_detect_segments on the image the descriptor gives; camera: NULL, or (fx, fy, cx, cy, k1, k2) of
 *                                     l3d_detect_segments_distorted.  The segments are byte for byte those of the host call on the converted pixels
 *   l3d_detect_segments_device_batch  l3d_detect_segments_batch's contract word for word, the entries device images: each entry's segments are
 *                                     byte for byte the single call's, the chunk's images are ingested by ONE launch, a refused entry (fields,
 *                                     memory kind, extent) fails alone, one line per failure in l3d_last_error
 *   l3d_decode_jpeg_device            l3d_decode_jpeg into the caller's device memory (`out`, written through k_det_egress); out's width, height
 *                                     and detector channel count (1 for channels == 1, else 3) must be the file's: L3D_ERR_INVALID otherwise
 *   l3d_undistort_image_device        ingest, k_det_undistort, egress: in and out of one size and detector channel count, and they may describe the
 *                                     same memory; both coefficients within 1e-12: ingest and egress only
 *   l3d_test_device_ingest            (tests) check, stream wait and the k_det_ingest launch of the product for a chunk of n images of one size and
 *                                     detector channel count; out: their slots of the pixel buffer, n x height x width x (1 or 3) bytes
 * ================================================================================================= */
#define L3D_U8 0
#define L3D_U16 1
#define L3D_F16 2
#define L3D_F32 3
typedef struct l3d_device_image {
    const void* ptr;                 /* device memory; element (y, x, c) is at ptr + (y*stride_y + x*stride_x + c*stride_c) * sizeof(element) */
    int width, height, channels;     /* channels of the SOURCE: 1, 3 or 4 */
    int dtype;                       /* L3D_U8, L3D_U16, L3D_F16, L3D_F32 */
    long long stride_y, stride_x, stride_c;   /* in ELEMENTS, signed; 0 allowed (a broadcast channel) */
    int chan[3];                     /* detector channel k is read from source channel chan[k]; ignored for channels == 1 */
    float scale;                     /* see the conversion rule; ignored for L3D_U8 */
    void* stream;                    /* the hipStream_t the pixels were produced on; NULL: the null stream */
} l3d_device_image;
typedef struct l3d_detect_device_entry {
    l3d_device_image image;
    int new_width, new_height; float min_length; int max_segments;
    const double* camera;                                                           /* NULL, or fx, fy, cx, cy, k1, k2 */
} l3d_detect_device_entry;
int l3d_device_image_check(const l3d_device_image* image, char* msg, size_t n);
int l3d_device_image_extent(const l3d_device_image* image, long long* lo, long long* hi);
int l3d_test_device_image_pointer(l3d_ctx* ctx, const l3d_device_image* image);
int l3d_test_device_ingest(l3d_ctx* ctx, const l3d_device_image* images, int n, unsigned char* out);
int l3d_detect_segments_device(l3d_ctx* ctx, const l3d_device_image* image, int new_width, int new_height, float min_length, int max_segments,
                               const double* camera /* NULL or fx, fy, cx, cy, k1, k2 */, float** segments, int* n);
int l3d_detect_segments_device_batch(l3d_ctx* ctx, const l3d_detect_device_entry* e, int n, float** segments, int* offsets /* n + 1 */, int* status /* n */);
int l3d_decode_jpeg_device(l3d_ctx* ctx, const unsigned char* bytes, size_t n, const l3d_device_image* out);
int l3d_undistort_image_device(l3d_ctx* ctx, const l3d_device_image* in, double fx, double fy, double cx, double cy, double k1, double k2,
                               const l3d_device_image* out);
/* with remaps (A REMAP, above): remap NULL, or n pointers of which any may be NULL; the entry's camera is the output camera */
int l3d_detect_segments_device_batch_remap(l3d_ctx* ctx, const l3d_detect_device_entry* e, const l3d_remap* const* remap, int n, float** segments, int* offsets,
                                           int* status);
/* with lenses (A LENS, above); fx, fy, cx, cy: the output camera */
int l3d_detect_segments_device_batch_lens(l3d_ctx* ctx, const l3d_detect_device_entry* e, const l3d_lens* const* lens, int n, float** segments,
                                          int* offsets /* n + 1 */, int* status /* n */);
int l3d_undistort_image_device_lens(l3d_ctx* ctx, const l3d_device_image* in, double fx, double fy, double cx, double cy, const l3d_lens* lens,
                                    const l3d_device_image* out);
/* A REMAP (above): out of remap's output size; valid: NULL, or a one-channel L3D_U8 image of that size */
int l3d_undistort_image_device_remap(l3d_ctx* ctx, const l3d_device_image* in, double fx, double fy, double cx, double cy, const l3d_remap* remap,
                                     const l3d_device_image* out, const l3d_device_image* valid);

/* =================================================================================================
 * THE ADD FAMILY: Line3D::addImage / addImage_fixed_sim (line3D.cc:95-342) in every form the library takes an image in.
 *
 * An image to add is an ENTRY: its id; the image -- 8-bit pixels (as l3d_detect_segments takes them) or a baseline JPEG file in memory, exactly one
 * of the two -- the camera K, R, t; dist, NULL or OpenCV-convention k1, k2 (the image is undistorted on the device with K's fx, fy, cx, cy before
 * the detector sees it; both within 1e-12: as NULL); and the links, of one of two kinds: sims == NULL: link_ids are the world point ids the view
 * observes (addImage); otherwise view ids with their similarities (addImage_fixed_sim).  The segment-taking forms (l3d_line3d_add_image[_fixed_sim],
 * ..._ex, ..._cached, above) bring segments, or an opened segment cache, where the entry has its image.
 *
 * ONE ROUTE adds an entry (line3d_amd/csrc/line3d_host.cpp: add_one), and every form below only fills an entry and takes it.  Its decisions,
 * in order -- the first that applies ends the call with its code, the message in l3d_line3d_last_error:
 *   1. the image: a JPEG file's headers give the size (a file the decoder refuses: its code and message); dist given: K NULL is
 *      L3D_ERR_INVALID, non-zero coefficients with K[1] != 0 (skew) L3D_ERR_UNSUPPORTED; a size below 1x1: "image is empty!"
 *   2. the cache decision, once: the file is "<data_directory>/segments_<id>_<w'>x<h'>_coll<0|1>.bin", (w', h') the size after the max_img_width
 *      down-scaling the detector works at (line3D.cc:133-138; the view keeps the original size).  Present and load_and_store != 0: it stands in for
 *      the image, which is neither decoded nor detected.  Present and load_and_store == 0: stale, to be removed.  Absent: to be written when
 *      load_and_store != 0
 *   3. unless the cache stands in: the detector (a JPEG file is entropy-decoded only here), on a node object once, on rank 0's device.  No
 *      segment found: L3D_OK and no view (line3D.cc:186-190); a stale cache is removed
 *   4. the guards, on every rank of a node object: "reconstruction already performed...", "imageID already in use!", "unlinked images cannot be
 *      added!" (n_links == 0), "image is empty!" (a size of 0; in the forms with a data directory also K, R or t NULL -- the forms without
 *      one, l3d_line3d_add_image[_fixed_sim] and ..._cached, answer a NULL K, R or t with "no segments" in step 5)
 *   5. the view: segments AND collinearities from the cache file (a file that cannot be read: its code and message), or the stale file removed
 *      and the detected segments, the cache noted to be written by prepare() (by rank 0 only); then the links
 * The guards come after the detector: a second image of an id in use in which nothing is detected is L3D_OK (and removes a stale cache).
 *
 * l3d_line3d_add_image_entry  the single call for an entry.  Returns the code; l3d_line3d_last_error holds the bare message.  An entry whose pixels
 *                             and jpeg are both NULL is here still the image its fields state, and is refused in the words of the call named
 *                             after it: any of width, height, channels, row_stride set: pixels ("image is empty!" for a size below 1x1); none
 *                             set: a JPEG file ("jpeg: null argument").  Both given: L3D_ERR_INVALID, as in l3d_line3d_add_images
 * l3d_line3d_add_images       n entries in one call: steps 1 and 2 per entry, ONE run of l3d_detect_segments_batch over all entries that need the
 *                             detector, then steps 3 to 5 per entry in entry order -- exactly the sequence of the single calls (but an entry with
 *                             neither or both of pixels and jpeg is L3D_ERR_INVALID, "an entry needs either ...").  status[i] (may be
 *                             NULL) is what the single call would have returned: a failed entry fails alone, an image without segments is L3D_OK and
 *                             no view.  The call returns L3D_OK when the batch was processed, else a device failure's code (entries added before
 *                             it stay added); l3d_line3d_last_error holds one line per failed entry, "image <id>: <message>"
 * The named forms are the entry with these fields filled:
 *   l3d_line3d_add_image_pixels[_fixed_sim]             pixels, dist NULL
 *   l3d_line3d_add_image_pixels[_fixed_sim]_distorted   pixels, dist -- which may not be NULL here: L3D_ERR_INVALID
 *   l3d_line3d_add_image_jpeg[_fixed_sim]               jpeg, dist or NULL
 * ================================================================================================= */
typedef struct l3d_image_entry {
    uint32_t image_id;
    const unsigned char* pixels; int width, height, channels; size_t row_stride;
    const unsigned char* jpeg; size_t jpeg_bytes;
    const double *K, *R, *t, *dist;                 /* dist: NULL or k1, k2 */
    const uint32_t* link_ids; const float* sims; int n_links;   /* sims == NULL: world point ids; else view similarities */
} l3d_image_entry;
int l3d_line3d_add_image_entry(l3d_line3d* h, const l3d_image_entry* e, const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_images(l3d_line3d* h, const l3d_image_entry* e, int n, const char* data_directory, int max_img_width, int load_and_store, int* status);
/* The entry with a lens (A LENS, above) in the place of dist: the same route, step 1 reading "a lens given: K NULL, a lens the checks refuse or an
 * entry that also carries dist is L3D_ERR_INVALID, an active lens with K[1] != 0 (skew) L3D_ERR_UNSUPPORTED".  The image is resampled from the
 * lens's source camera onto the entry's K, which the view keeps.  lens: NULL (then exactly the calls above), or one pointer per entry of which any
 * may be NULL: that entry's own dist rule */
int l3d_line3d_add_image_entry_lens(l3d_line3d* h, const l3d_image_entry* e, const l3d_lens* lens, const char* data_directory, int max_img_width, int load_and_store);
/* The entry with a remap (A REMAP, above) in the place of dist and lens -- an entry that also carries dist: L3D_ERR_INVALID.  The entry's K is the
 * OUTPUT camera and the view's K; the view's width and height are the remap's OUTPUT size, which therefore also names the segment cache file;
 * max_img_width acts on the output size; a cache that is present and wanted still stands in for the image.  Skew (K[1] != 0) with a remap that
 * resamples: L3D_ERR_UNSUPPORTED.  remap: NULL (then exactly the calls above), or one pointer per entry of which any may be NULL */
/* l3d_undistort_image_remap with the object's device and K, the output camera (a skewed K with a remap that resamples: refused) */
int l3d_line3d_undistort_image_remap(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                     const l3d_remap* remap, unsigned char* out, size_t out_row_stride, unsigned char* valid, size_t valid_row_stride);
int l3d_line3d_add_image_entry_remap(l3d_line3d* h, const l3d_image_entry* e, const l3d_remap* remap, const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_images_remap(l3d_line3d* h, const l3d_image_entry* e, const l3d_remap* const* remap, int n, const char* data_directory, int max_img_width,
                                int load_and_store, int* status);
int l3d_line3d_add_images_lens(l3d_line3d* h, const l3d_image_entry* e, const l3d_lens* const* lens, int n, const char* data_directory, int max_img_width,
                               int load_and_store, int* status);
int l3d_line3d_undistort_image_lens(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                    const l3d_lens* lens, unsigned char* out, size_t out_row_stride);

/* The add family for an image in DEVICE memory (l3d_device_image, above): the entry with a descriptor where l3d_image_entry has pixels or a file.  It
 * takes the ONE ROUTE above, with these words for its image:
 *   1. l3d_device_image_check on the descriptor (its code and message), the camera of the undistortion as above; the view's size is the
 *      descriptor's, the detector's channels 1 (channels == 1) or 3
 *   2. the cache decision, unchanged
 *   3. only where the detector runs: the pointer check, the extent check, the stream wait, k_det_ingest, the detector.  A cache that is present and
 *      wanted stands in for the image, whose memory is then never touched and never checked -- as a JPEG file's entropy data is not
 *   4., 5. unchanged; the guards come after the detector
 * l3d_line3d_add_device_entry is the single call, l3d_line3d_add_device_images the batch with l3d_line3d_add_images' contract (one run of the batch
 * detector, one k_det_ingest launch per chunk, an entry fails alone, "image <id>: <message>" per failure).  A batch that mixes host, JPEG and device
 * entries in one call is not offered.  l3d_line3d_decode_jpeg_device / l3d_line3d_undistort_image_device: the context calls on the object's device
 * (a node object: rank 0's), the latter with the object's K rule (l3d_line3d_undistort_image). */
typedef struct l3d_device_entry {
    uint32_t image_id;
    l3d_device_image image;
    const double *K, *R, *t, *dist;                 /* dist: NULL or k1, k2 */
    const uint32_t* link_ids; const float* sims; int n_links;   /* sims == NULL: world point ids; else view similarities */
} l3d_device_entry;
int l3d_line3d_add_device_entry(l3d_line3d* h, const l3d_device_entry* e, const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_device_images(l3d_line3d* h, const l3d_device_entry* e, int n, const char* data_directory, int max_img_width, int load_and_store, int* status);
int l3d_line3d_decode_jpeg_device(l3d_line3d* h, const unsigned char* bytes, size_t n, const l3d_device_image* out);
int l3d_line3d_undistort_image_device(l3d_line3d* h, const l3d_device_image* in, const double* K, double k1, double k2, const l3d_device_image* out);
/* the device entry with a lens: as l3d_line3d_add_image_entry_lens / l3d_line3d_add_images_lens */
int l3d_line3d_add_device_entry_lens(l3d_line3d* h, const l3d_device_entry* e, const l3d_lens* lens, const char* data_directory, int max_img_width, int load_and_store);
/* the device entry with a remap: as l3d_line3d_add_image_entry_remap / l3d_line3d_add_images_remap */
int l3d_line3d_add_device_entry_remap(l3d_line3d* h, const l3d_device_entry* e, const l3d_remap* remap, const char* data_directory, int max_img_width, int load_and_store);
int l3d_line3d_add_device_images_remap(l3d_line3d* h, const l3d_device_entry* e, const l3d_remap* const* remap, int n, const char* data_directory, int max_img_width,
                                       int load_and_store, int* status);
int l3d_line3d_add_device_images_lens(l3d_line3d* h, const l3d_device_entry* e, const l3d_lens* const* lens, int n, const char* data_directory, int max_img_width,
                                      int load_and_store, int* status);

/* =================================================================================================
 * A SEGMENT MASK: a mask applied to line SEGMENTS -- whole segments dropped, or segments clipped or split at the mask's edges -- on the device
 * (line3d_amd/csrc/l3d_segmask.hip, l3d_segmask.hpp).  The validity plane of A REMAP keeps masked pixels out of the detector; segments that come from
 * the caller, from a segment cache, or from a cache that stands in for the image on the pixel route never pass that plane.  This is the mask for them.
 *
 * Numeric rules: all arithmetic is f64, every product and sum rounded on its own (nothing fused); integer arithmetic is int64.
 *
 * THE SEGMENT AND ITS SAMPLES.  A segment is x1, y1, x2, y2 (f32); pixel (j, i) has its centre at (j, i).
 *     dx = x2 - x1      dy = y2 - y1      m = max(|dx|, |dy|)      n = floor(m) + 1
 *     sample k, k = 0..n (n + 1 samples):  t = k / n      px = x1 + t dx      py = y1 + t dy
 *   Without a lens the sample reads mask pixel (floor(px + 0.5), floor(py + 0.5)).  A sample outside mask_width x mask_height is invalid; otherwise
 *   it is valid when its byte is >= threshold.  threshold runs 1..255, and 0 reads as 1: this is how a weighted (soft) mask is read, any other
 *   weighting is out of scope.
 * A LENS.  With an active lens the mask lies in the lens's SOURCE grid (the distorted image) and the segments in the grid of the camera fx, fy, cx, cy
 *   given beside it: (px, py) goes through the formulas of A LENS with j = px, i = py and (fx', fy', cx', cy') = (fx, fy, cx, cy), giving (u, v), and
 *   the sample reads mask pixel (floor(u + 0.5), floor(v + 0.5)).  A u or v that is not finite is invalid.  The lens is checked as A LENS checks it,
 *   with its codes (the mask's extent in the place of the image's).  lens NULL, or a lens that is not active (BROWN, every coefficient within
 *   1e-12, equal cameras): the mask is in the segments' grid and fx, fy, cx, cy are not read.
 * ALWAYS DROPPED, in every mode: a segment with a coordinate that is not finite, with dx == dy == 0, or with m >= 65536.
 * MODE DROP.  V = the number of valid samples.  The segment is kept iff V 1000 >= keep_permille (n + 1), keep_permille in 0..1000.  A kept segment
 *   keeps its bits.
 * MODES CLIP AND SPLIT.  Bridging: a run of at most max_gap (>= 0) invalid samples strictly between two valid samples counts as valid.  A run [a, b]
 *   is a maximal run of valid samples with a < b.  Length test: with s = (b - a) / n and L2 = dx dx + dy dy the run passes iff
 *   (s s) L2 >= min_length min_length.  CLIP emits the run with the largest b - a (the first on a tie) if it passes, otherwise nothing.  SPLIT emits
 *   every passing run, in ascending a.  An emitted end point is the sample's (px, py) rounded to f32; where a == 0 the bits of x1, y1 are emitted,
 *   where b == n the bits of x2, y2: an all-valid mask returns the input byte for byte.
 * OUTPUT.  The segments in input order, the runs of one segment in order along it; an int32 src_index per output segment names the input segment it
 *   came from.  Both callee-allocated (l3d_free); *n_out may exceed n (SPLIT).
 * REFUSED, L3D_ERR_INVALID, before anything is launched or read: a NULL mask (the struct or its plane); an extent below 1 x 1; a row stride below the
 *   width; a mode, threshold (0..255), keep_permille, max_gap or min_length (finite, >= 0) out of range; what A LENS refuses; a device mask (or device
 *   segment array) whose memory kind or extent fails the check an l3d_device_image gets.  More than 2^31 - 1 output segments: L3D_ERR_UNSUPPORTED.
 *
 * THE KERNELS.  One wave per segment, four waves per workgroup; lanes stride over the samples, a ballot gives the validity of 64 samples as one word,
 * bridging and run search work on those words, uniformly across the wave.  k_segmask_count counts every segment's outputs, k_segmask_scan (one
 * workgroup, l3d_scan.hpp) turns the counts into positions, k_segmask_write writes the segments and src_index there: the order is fixed by the scan,
 * never by atomics, and the number of launches (three) does not depend on n.  Profile names segmask_count, segmask_scan, segmask_write.  A host mask is
 * uploaded once per call; a device mask and a device segment array are read in place (the caller has synchronised whatever wrote them).
 *   l3d_mask_segments              segments: n x 4 floats in host memory
 *   l3d_mask_segments_device       the same with the segments in device memory; the outputs are host memory as above
 *   l3d_test_mask_segments_host    the same arguments without the context; needs no device (mask_on_device: refused).  It runs the functions the
 *                                  kernels run, lane after lane, and is bit-equal to the device call -- but for atan in a FISHEYE lens, whose bits
 *                                  the device does not share with a host libm (A LENS).  l3d_segmask_last_error (per thread) holds its message
 *   l3d_line3d_add_image_masked    l3d_line3d_add_image (sims == NULL: link_ids are world point ids) or ..._fixed_sim with the segments filtered
 *                                  first.  mask NULL: L3D_ERR_INVALID.  Without an active lens the mask's extent must be the view's width x height,
 *                                  else L3D_ERR_INVALID.  Nothing left after the filter: L3D_OK and no view, as when the detector finds nothing.
 *                                  On a node object the filter runs once, on rank 0's device, and every rank gets the result
 *   l3d_line3d_add_image_cached_masked
 *                                  the cache's segments go through the filter; the cache's collinearities are discarded and the view computes its
 *                                  own, as it does for given segments.  No cache file is written or changed
 * On the pixel route a cache that is "present and wanted" stands in for the image (THE ADD FAMILY, step 2), so a mask that changed since the cache was
 * written has no effect there; that behaviour stays.  The masked forms are the way round it: read the cache and add it through
 * l3d_line3d_add_image_cached_masked.
 * ================================================================================================= */
enum { L3D_SEGMASK_DROP = 0, L3D_SEGMASK_CLIP = 1, L3D_SEGMASK_SPLIT = 2 };
typedef struct l3d_segment_mask {
    const void* mask;               /* mask_width x mask_height bytes, rows mask_row_stride bytes apart */
    size_t mask_row_stride;
    int32_t mask_width, mask_height;
    int32_t mask_on_device;         /* the plane is device memory */
    const l3d_lens* lens;           /* NULL: the mask is in the segments' grid */
    double fx, fy, cx, cy;          /* the segments' camera (read only with a lens) */
    int32_t mode;                   /* L3D_SEGMASK_DROP, _CLIP, _SPLIT */
    int32_t threshold;              /* 1..255; 0 reads as 1 */
    int32_t keep_permille;          /* DROP: 0..1000 */
    int32_t max_gap;                /* CLIP, SPLIT: >= 0 */
    double min_length;              /* CLIP, SPLIT: pixels, >= 0 */
} l3d_segment_mask;
int l3d_mask_segments(l3d_ctx* ctx, const float* segments, int n, const l3d_segment_mask* mask, float** out, int32_t** src_index, int* n_out);
int l3d_mask_segments_device(l3d_ctx* ctx, const float* segments, int n, const l3d_segment_mask* mask, float** out, int32_t** src_index, int* n_out);
int l3d_test_mask_segments_host(const float* segments, int n, const l3d_segment_mask* mask, float** out, int32_t** src_index, int* n_out);
const char* l3d_segmask_last_error(void);
int l3d_line3d_add_image_masked(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height, const float* segments, int n_segments, const double* K,
                                const double* R, const double* t, const uint32_t* link_ids, const float* sims, int n_links, const l3d_segment_mask* mask);
int l3d_line3d_add_image_cached_masked(l3d_line3d* h, uint32_t image_id, unsigned width, unsigned height, const l3d_segment_cache* cache, const double* K,
                                       const double* R, const double* t, const uint32_t* link_ids, const float* sims, int n_links, const l3d_segment_mask* mask);

/* =================================================================================================
 * CO-VISIBILITY.  What Line3D::processWorldpointList (line3D.cc:1874-1935) files for the world point lists of the views, counted at once.
 *   point_ids    the lists one after the other, in add order; any uint32 is an id, all 32 bits count
 *   list_start   n_lists + 1 ascending offsets into point_ids, list_start[0] == 0; list i is view index i
 * Out (callee-allocated, l3d_free): num_wps[n_lists]; the non-zero common_wps as a CSR over view indices -- row_start[n_lists + 1], col (ascending
 * within a row) and count, both row_start[n_lists] long (one spare element each); *path: 0 = the closed form on the device, 1 = the host replay.
 * THE CLOSED FORM (no list names an id twice): a point whose track has fewer than three views counts nothing; a point with L >= 3 views adds 1 to
 *   common_wps[a][b] for every ordered pair a != b of its views and 1 to num_wps of each.  The add order does not matter.
 * PATH 1.  A list that names an id twice leaves the closed form (the function counts self pairs): the device finds that out (equal neighbours in the
 *   sorted keys) and the lists are replayed through the function itself, in add order.
 * REFUSED before anything is launched: a NULL argument (point_ids may be NULL without observations), n_lists < 0, offsets that do not start at 0 or
 *   descend: L3D_ERR_INVALID.  2^31 - 1 observations or more, or 2^31 - 1 views or more: L3D_ERR_UNSUPPORTED.  So is a result of more than 2^31 - 1
 *   non-zero counts.
 * THE KERNELS.  k_covis_keys packs (point, view index) keys, one radix sort orders them (the observation's position rides along), k_covis_runs hands
 *   every observation its track (start and length in the sorted order) and flags equal neighbours.  k_covis_count: one workgroup per view and column
 *   tile walks the view's tracks of three or more views into an LDS histogram over the tile's view indices (a lane walks a short track alone, the
 *   wave shares a long one) and counts the non-zeros; k_covis_scan turns the counts into positions; k_covis_write repeats the walk and writes col and
 *   count in ascending order.  Counters are 32 bits wide.  Six launches (profile names covis_keys, covis_sort, covis_runs, covis_count, covis_scan,
 *   covis_write) whatever the number of observations; the column tiles are a dimension of the grid.  Option L3D_COVIS_TILE: columns per tile (0: 8192,
 *   the most).  No allocation grows with n_lists squared, and all device memory of the call is released before it returns.
 *   l3d_test_covisibility_host   the same arguments without the context, no device: always the replay.  l3d_covis_last_error (per thread): its message
 *   l3d_line3d_set_covisibility  0 (default): a view's links are filed on the host as it is added.  1: the add only stores the list, and prepare()
 *                                counts all lists when one arrived since the last count, replacing num_wps and common_wps; everything behind them
 *                                (findVisualNeighbors) is the same code.  Refused while the object holds views; reset keeps the setting.  A node object
 *                                counts once, on rank 0's device
 *   l3d_line3d_covisibility_path the path of the last count (0 before any)
 *   l3d_line3d_get_neighbors / l3d_line3d_get_view_similarities
 *                                after prepare, in either mode: the view's neighbours (ascending ids) / its similarities (ascending by the other
 *                                view).  *n is the number there is; at most cap are written (ids, sims may be NULL)
 * ================================================================================================= */
int l3d_covisibility(l3d_ctx* ctx, const uint32_t* point_ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col,
                     uint32_t** count, int* path);
int l3d_test_covisibility_host(const uint32_t* point_ids, const int64_t* list_start, int n_lists, uint32_t** num_wps, int32_t** row_start, int32_t** col,
                               uint32_t** count, int* path);
const char* l3d_covis_last_error(void);
int l3d_line3d_set_covisibility(l3d_line3d* h, int mode);
int l3d_line3d_covisibility_path(const l3d_line3d* h);
int l3d_line3d_get_neighbors(l3d_line3d* h, uint32_t view_id, uint32_t* ids, int cap, int* n);
int l3d_line3d_get_view_similarities(l3d_line3d* h, uint32_t view_id, uint32_t* ids, float* sims, int cap, int* n);

/* =================================================================================================
 * PROJECTION AND OVERLAYS: 3-D segments projected into cameras and clipped to their images, and 2-D segments drawn over an image, on the device
 * (line3d_amd/csrc/l3d_project.hpp, l3d_project.hip, l3d_draw.hpp, l3d_draw.hip).  The conventions the library works with, stated once:
 * x = K (R X + t); pixel (j, i) has its centre at (j, i); the image covers [-0.5, w - 0.5] x [-0.5, h - 0.5]; segments live in the grid of the image
 * as it was added (after an undistortion, before any max_img_width down-scaling).
 *
 * Numeric rules: all arithmetic is f64; every product, sum, quotient and square root is rounded on its own (nothing fused); integers are int64.
 * tests/project_model.py and tests/draw_model.py hold the same rules in numpy; the host entry points run the kernels' functions lane after lane; the
 * three agree bit for bit.
 *
 * 1. PROJECTION.  l3d_project_lines: n 3-D segments (seg3d: n x 6 f64, P then Q) into m cameras (l3d_camera: K, R, t row-major, width, height).
 *   ONE (camera, segment) PAIR:
 *   Camera frame.  For each row r of R:  c_r = ((R[r,0] X + R[r,1] Y) + R[r,2] Z) + t[r], giving (x, y, z) for P and for Q.  A pair with a camera-
 *     frame coordinate that is not finite is dropped (so is, with it, every input that is not finite).
 *   Near plane (near > 0, finite).  Both z < near: dropped.  zP < near <= zQ: s = (near - zP) / (zQ - zP) and P becomes
 *     (xP + s (xQ - xP), yP + s (yQ - yP), near).  zQ < near <= zP: the same from Q, s = (near - zQ) / (zP - zQ), Q becomes
 *     (xQ + s (xP - xQ), yQ + s (yP - yQ), near).
 *   Pixels.  xn = x / z, yn = y / z;  u = (K[0] xn + K[1] yn) + K[2];  v = (K[3] xn + K[4] yn) + K[5].  du = uQ - uP, dv = vQ - vP.  Dropped: any of
 *     uP, vP, uQ, vQ, du, dv not finite; du == dv == 0.
 *   THE RECTANGLE RULE.  [xmin, xmax] x [ymin, ymax] = [-0.5 - margin, (width - 0.5) + margin] x [-0.5 - margin, (height - 0.5) + margin], margin >= 0.
 *     Liang-Barsky on (du, dv) with t0 = 0, t1 = 1; the edges in the order left, right, top, bottom with (p, q) = (-du, uP - xmin), (du, xmax - uP),
 *     (-dv, vP - ymin), (dv, ymax - vP).  p == 0: dropped iff q < 0.  Otherwise r = q / p; p < 0: dropped iff r > t1, then t0 = max(t0, r);
 *     p > 0: dropped iff r < t0, then t1 = min(t1, r).  Kept iff t0 < t1 after the four edges.
 *   Output.  First end (uP + t0 du, vP + t0 dv), exactly (uP, vP) where t0 == 0; second end (uP + t1 du, vP + t1 dv), exactly (uQ, vQ) where
 *     t1 == 1; each rounded to f32.  flags bit 0: the P end moved (near plane, or t0 > 0); bit 1: the Q end moved (near plane, or t1 < 1).
 *   OUTPUT.  Camera-major, within a camera in input order: seg2d (4 f32 per output), src_index (int32: the input segment), flags (u8), all
 *     callee-allocated (l3d_free; one spare element each), and cam_start (m + 1 int64, the caller's): camera c's outputs are [cam_start[c], cam_start[c + 1]).
 *   REFUSED before anything is launched, L3D_ERR_INVALID: a NULL pointer (seg3d may be NULL with n == 0, cameras with m == 0); n or m < 0; a camera
 *     whose K third row is not exactly (0, 0, 1) or whose size is below 1 x 1; near not in (0, 1.7976931348623157e308]; margin not in [0, 2^30]; a
 *     device segment array whose memory kind or extent fails the check an l3d_device_image gets, or that is not aligned to 8 bytes.  n is an int: a
 *     camera cannot have more than 2^31 - 1 outputs.
 *   THE KERNELS.  Cameras are processed in chunks.  k_proj_count: one (camera, segment) pair per lane, a wave never spans two cameras; a ballot gives
 *     the wave's kept pairs as one 64-bit word.  k_proj_scan (one workgroup, l3d_scan.hpp) turns the words' bit counts into positions.  k_proj_write
 *     runs the pair function again and writes at position-of-the-word + kept lanes below: the order comes from the scan, never from atomics.  Three
 *     launches per chunk (profile names proj_count, proj_scan, proj_write) whatever n.  A chunk is L3D_PROJ_CHUNK cameras (0: 64), cut down so
 *     that its ballot words stay below 2^20 and its pairs below 2^31 (never below one camera).
 *   l3d_project_lines               seg3d in host memory
 *   l3d_project_lines_device        seg3d in device memory, read in place (the caller has synchronised whatever wrote it); outputs host memory
 *   l3d_test_project_lines_host     the same arguments without the context: the same functions, no device.  l3d_project_last_error (per thread)
 *
 * 2. DRAWING.  l3d_draw_segments draws n segments (n x 4 f32: x1, y1, x2, y2 in the image's grid) over 8-bit pixels, in place.
 *   Stroke.  W16 = rint(width_px 16); width_px in [0.5, 64], so W16 is in 8..1024.  R16 = W16 / 2.0 + 8.0.
 *   Clip.  A segment with a coordinate that is not finite is dropped.  The others go through THE RECTANGLE RULE with margin ceil(W16 / 32) + 1 (as
 *     an integer: (W16 + 31) / 32 + 1); the ends are taken as in "Output" above, in f64.  A zero-length segment inside that rectangle passes the
 *     rule (every p is 0) and gives a disc.
 *   Fixed point.  Each clipped end is quantised to sixteenths of a pixel, X = rint(x 16) (ties to even) as int64; a pixel centre is (16 j, 16 i).
 *   Distance d, in sixteenths, of a pixel centre C from the quantised segment P, Q:  a = C - P, b = Q - P, L2 = b.b, dot = a.b (int64, exact).
 *     dot <= 0: d = sqrt((double)(a.a)).  dot >= L2: d = sqrt((double)|C - Q|^2).  Otherwise d = (double)|a x b| rinv with
 *     rinv = 1.0 / sqrt((double)L2), computed once per segment.  Images are at most 32768 on a side, so every integer stays below 2^53.
 *   Coverage.  cov = clamp((R16 - d) / 16.0, 0, 1), q = (int)floor(cov 255.0 + 0.5).  Caps are round.  A 1-pixel line on an integer y gives 255 on
 *     its row and 0 beside it; on a half-integer y 128 and 128.
 *   Winner.  Among the segments with q > 0 at a pixel the one with the largest key (q << 24) | k wins, k the segment's index: on equal coverage the
 *     later segment.  The result is a function of the pixel alone: any schedule gives the same bytes.
 *   Blend (integers).  The winner's colour is colors[color_index ? color_index[k] : k % n_colors] = (c0, c1, c2, alpha) in the image's channel order.
 *     A = (alpha opacity + 127) / 255, a = (q A + 127) / 255, out = (src (255 - a) + col a + 127) / 255 for the colour components
 *     0 .. min(channels, 3) - 1; a one-channel image uses component 0; a fourth channel is left as it is.
 *   REFUSED before anything is launched, L3D_ERR_INVALID: a NULL pointer (segments may be NULL with n == 0); n < 0; a size below 1 x 1; channels not
 *     1, 3 or 4; a row stride below width x channels; n_colors < 1; a color_index entry outside [0, n_colors); width_px outside [0.5, 64]; opacity
 *     outside 0..255; for a device image what the device-image checks refuse.  L3D_ERR_UNSUPPORTED: n > 2^24; a side above 32768; a device image
 *     whose dtype is not L3D_U8; more than 2^31 - 1 pieces (below).
 *   THE KERNELS.  k_draw_pieces clips and quantises every segment and counts its pieces of 64 steps along the major axis (columns for |bx| >= |by|,
 *     else rows); k_draw_scan (one workgroup) turns the counts into positions.  k_draw_cover: one wave per piece -- a long line and ten thousand
 *     short ones keep the same number of waves busy; a lane takes one column (row) and walks the pixels across the stroke, the lanes of a wave
 *     addressing neighbouring pixels, and a no-return 32-bit atomicMax files the key in a key plane the context owns.  k_draw_resolve: one thread per
 *     pixel of the rows the pieces touch blends where the key is not 0 and writes the 0 back: the plane is zeroed when it is allocated or grown, never
 *     per call.  Four launches whatever n (profile names draw_pieces, draw_scan, draw_cover, draw_resolve).  Host pixels are uploaded and copied
 *     back; a device image is drawn where it lies: colour component k goes to source channel chan[k], any strides, and STREAM ORDER of the
 *     device-image section applies.
 *   l3d_draw_segments              pixels in host memory: height rows of width x channels bytes, row_stride bytes apart
 *   l3d_draw_segments_device       an l3d_device_image
 *   l3d_test_draw_segments_host    l3d_draw_segments without the context: the same functions, no device.  l3d_draw_last_error (per thread)
 *
 * 3. ON THE OBJECT.  The current result (l3d_line3d_get_result: world coordinates) projected into views and drawn over a view's image.
 *   l3d_line3d_project_result   the 3-D segments of the result, in l3d_line3d_get_result's order, through l3d_project_lines.  cameras NULL: each
 *                               view's own camera, K, R, t and size as the view was added (view_ids: n_views ids).  Otherwise n_views cameras of
 *                               the caller's, and view_ids may be NULL.  select L3D_SELECT_ALL: every 3-D segment.  L3D_SELECT_OBSERVED: only the
 *                               segments of lines that have a 2-D member in that view (needs view_ids): the subset of ALL, in the same order.
 *                               Out, camera-major as above: seg2d, seg_index (into l3d_line3d_get_result's seg3d array), line_index, flags
 *                               (callee-allocated, l3d_free) and cam_start (n_views + 1).  near_z, margin: as l3d_project_lines
 *   l3d_line3d_overlay          draws over 8-bit pixels of the view's size (else L3D_ERR_INVALID), layer after layer, each ONE call of
 *                               l3d_draw_segments: L3D_LAYER_MEMBERS, the view's 2-D segments that are members of a line, in line order, width
 *                               width_members; then L3D_LAYER_MODEL, l3d_line3d_project_result of the view under style->select with style->near_z
 *                               and margin 34 (above every stroke's own clip margin), width width_model.  Colours: by_line != 0:
 *                               palette[line % n_palette] for both layers (palette NULL: l3d_default_palette, 12 entries); by_line == 0: color_members
 *                               and color_model.  style NULL: both layers, OBSERVED, by line, the default palette, widths 1 and 2, opacity 255, near 1e-6
 *   l3d_line3d_overlay_device   the same over an l3d_device_image (L3D_U8)
 *   l3d_default_palette         12 x (c0, c1, c2, alpha): (230, 25, 75) (60, 180, 75) (255, 225, 25) (0, 130, 200) (245, 130, 48) (145, 30, 180)
 *                               (70, 240, 240) (240, 50, 230) (210, 245, 60) (250, 190, 212) (0, 128, 128) (170, 110, 40), alpha 255 each
 *   REFUSED, L3D_ERR_INVALID: before a finish (l3d_line3d_compute3Dmodel) has produced a result; an unknown view; a select or a layer mask out of
 *   range; OBSERVED without view ids; what the two layers refuse, with their codes.  A node object projects and draws on rank 0's context, which holds
 *   the result.
 *
 * OUT OF SCOPE: hidden-line removal and occlusion; drawing onto the distorted source image; dtypes other than U8; PNG output; a batch overlay call.
 * ================================================================================================= */
typedef struct l3d_camera {
    double K[9], R[9], t[3];        /* row-major; x = K (R X + t) */
    int32_t width, height;
} l3d_camera;
int l3d_project_lines(l3d_ctx* ctx, const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                      int32_t** src_index, unsigned char** flags, int64_t* cam_start /* m + 1 */);
int l3d_project_lines_device(l3d_ctx* ctx, const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                             int32_t** src_index, unsigned char** flags, int64_t* cam_start);
int l3d_test_project_lines_host(const double* seg3d, int n, const l3d_camera* cameras, int m, double near_z, double margin, float** seg2d,
                                int32_t** src_index, unsigned char** flags, int64_t* cam_start);
const char* l3d_project_last_error(void);
int l3d_draw_segments(l3d_ctx* ctx, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const float* segments, int n,
                      const unsigned char* colors /* n_colors x 4 */, int n_colors, const int32_t* color_index /* NULL or n */, double width_px, int opacity);
int l3d_draw_segments_device(l3d_ctx* ctx, const l3d_device_image* image, const float* segments, int n, const unsigned char* colors, int n_colors,
                             const int32_t* color_index, double width_px, int opacity);
int l3d_test_draw_segments_host(unsigned char* pixels, int width, int height, int channels, size_t row_stride, const float* segments, int n,
                                const unsigned char* colors, int n_colors, const int32_t* color_index, double width_px, int opacity);
const char* l3d_draw_last_error(void);
enum { L3D_SELECT_ALL = 0, L3D_SELECT_OBSERVED = 1 };
enum { L3D_LAYER_MEMBERS = 1, L3D_LAYER_MODEL = 2 };
typedef struct l3d_overlay_style {
    int32_t layers;                 /* L3D_LAYER_MEMBERS | L3D_LAYER_MODEL */
    int32_t select;                 /* L3D_SELECT_ALL, L3D_SELECT_OBSERVED: the model layer */
    int32_t by_line;                /* != 0: palette[line % n_palette] for both layers; 0: color_members / color_model */
    int32_t opacity;                /* 0..255 */
    double width_members, width_model, near_z;
    unsigned char color_members[4], color_model[4];     /* c0, c1, c2, alpha in the image's channel order */
    const unsigned char* palette;   /* n_palette x 4; NULL: l3d_default_palette */
    int32_t n_palette, pad;
} l3d_overlay_style;
const unsigned char* l3d_default_palette(void);
int l3d_line3d_project_result(l3d_line3d* h, const uint32_t* view_ids, int n_views, const l3d_camera* cameras, int select, double near_z, double margin,
                              float** seg2d, int32_t** seg_index, int32_t** line_index, unsigned char** flags, int64_t* cam_start /* n_views + 1 */);
int l3d_line3d_overlay(l3d_line3d* h, uint32_t view_id, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const l3d_overlay_style* style);
int l3d_line3d_overlay_device(l3d_line3d* h, uint32_t view_id, const l3d_device_image* image, const l3d_overlay_style* style);

/* =================================================================================================
 * MERGING DUPLICATE LINES (no counterpart in the reference; formulas: line3d_amd/csrc/l3d_merge.hpp, numpy model: tests/merge_model.py).  A 3-D line is a
 * cluster of 2-D segments linked through matches between NEIGHBOURING views, so an edge seen along a camera path longer than the matching neighbourhood
 * comes out as several near-copies.  l3d_merge_lines finds them: an all-pairs test on the device, the components of the pair graph, and a star rule.
 * Everything is f64; every product, sum and quotient is rounded once, in the written order; x . y = ((x0 y0) + (x1 y1)) + (x2 y2).
 *
 * A LINE OF THE TABLE   P, Q (lines[6 k ..]: 3 + 3 doubles), L = sqrt((Q - P) . (Q - P)), d = (Q - P) / L, and a tolerance tol[k] >= 0 in scene units.
 *                       ELIGIBLE iff the seven numbers and L are finite and L > 0.
 * THE PAIR TEST         for eligible i < j, a = the longer line (larger L; at equal L the lower index), b = the other.  All three must hold:
 *                       1. |d_a . d_b| >= cos_min
 *                       2. for X in {P_b, Q_b}: v = X - P_a, s = v . d_a, r = v - s d_a, e = sqrt(r . r); e_P <= max(tol_a, tol_b) and e_Q <= the same
 *                       3. min(max(s_P, s_Q), L_a) - max(min(s_P, s_Q), 0) >= -(max_gap L_b)
 * GROUPING              the connected components of the pair graph; a component's REPRESENTATIVE is its longest line (at equal L the lowest index); a
 *                       line STAYS iff it is the representative or passes the pair test against it (the star rule: no chain A ~ B ~ C with A unlike C,
 *                       so an arc of short segments never collapses into one line); every other line is RELEASED as a group of one.
 *                       group[k] = the lowest index among the staying lines of k's component, or k (released, not eligible, no pair).
 * OUTPUTS               group[n]; pairs: callee-allocated (l3d_free) int32 (i, j), ascending by (i, j) under any schedule, *n_pairs of them;
 *                       counts[4] = eligible lines, components with a pair, lines released, groups of two or more lines.
 *   l3d_merge_lines             the device: three launches find the pairs whatever n is (count, scan, write)
 *   l3d_test_merge_lines_host   the same functions in loops on the host, no device needed, bit-equal.  l3d_merge_last_error (per thread)
 * REFUSED, L3D_ERR_INVALID, before any launch: n < 0; a NULL array with n > 0 or a NULL output; cos_min outside [0, 1] or not a number; max_gap
 *   negative or not finite; a negative or NaN tol.  L3D_ERR_UNSUPPORTED: more than 2^31 - 1 pairs (no allocation is attempted), or a pair list the
 *   device cannot hold.  n == 0: empty outputs, L3D_OK.
 * ================================================================================================= */
typedef struct l3d_merge_params { double cos_min, max_gap; } l3d_merge_params;
int l3d_merge_lines(l3d_ctx* ctx, const double* lines /* 6 n: P, Q */, const double* tol /* n */, int n, const l3d_merge_params* params, int32_t* group /* n */,
                    int32_t** pairs, int* n_pairs, int32_t* counts /* 4 */);
int l3d_test_merge_lines_host(const double* lines, const double* tol, int n, const l3d_merge_params* params, int32_t* group, int32_t** pairs, int* n_pairs,
                              int32_t* counts);
const char* l3d_merge_last_error(void);

/* =================================================================================================
 * SUPPORT OF 3-D LINES (no counterpart in the reference; formulas: line3d_amd/csrc/l3d_support.hpp, numpy model: tests/support_model.py).  A 3-D line
 * knows only the 2-D segments of its cluster, and clusters are linked through matches between NEIGHBOURING views, so a line lists a small part of the
 * views that see it.  l3d_support_lines answers "which 2-D segments of which cameras lie on this 3-D segment": every 3-D segment is projected into every
 * camera and tested against every 2-D segment of that camera.  All arithmetic is f64; every product, sum, quotient and square root is rounded on its own,
 * in the written order (nothing fused); integers are int64.  max(x, y) is (x < y ? y : x) and min(x, y) is (y < x ? y : x); a comparison with a NaN
 * is false, so a condition written "must hold" fails on a NaN.
 *
 * INPUTS    seg3d: n x 6 f64, P then Q.  cameras: m l3d_camera.  seg2d: 4 f32 (x1, y1, x2, y2) per 2-D segment, the segments of camera c at
 *           [seg_start[c], seg_start[c + 1]) (seg_start: m + 1 int64, ascending from 0); j below is a segment's index WITHIN its camera.
 *           params: dist_px >= 0, cos_min in [0, 1], min_overlap in [0, 1], and near_z, margin as l3d_project_lines takes them.
 * A ROW (camera c, 3-D segment k).  ONE (camera, segment) PAIR of "PROJECTION AND OVERLAYS", 1, unchanged through THE RECTANGLE RULE, with near_z and
 *           margin; a pair dropped there has no row.  The ends stay in f64 and are not rounded to f32: A = (uP + t0 du, vP + t0 dv), exactly (uP, vP)
 *           where t0 == 0; B = (uP + t1 du, vP + t1 dv), exactly (uQ, vQ) where t1 == 1.  a = B - A, La = sqrt((ax ax) + (ay ay)); no row unless La is
 *           finite and > 0.  da = a / La (two quotients).
 * A COLUMN (2-D segment j of camera c).  U = (x1, y1), V = (x2, y2) widened to f64; b = V - U, Lb = sqrt((bx bx) + (by by)); ELIGIBLE iff the four
 *           numbers and Lb are finite and Lb > 0.  db = b / Lb.
 * THE PAIR TEST of a row and an eligible column of the same camera.  All three must hold:
 *           1. |(dax dbx) + (day dby)| >= cos_min
 *           2. for X in {U, V}: w = X - A, e = |(wx day) - (wy dax)|, s = (wx dax) + (wy day); eU <= dist_px and eV <= dist_px
 *           3. ov = min(max(sU, sV), La) - max(min(sU, sV), 0) and Lm = min(La, Lb); ov >= min_overlap Lm
 * A RECORD  l3d_support_record, 16 bytes, for every pair that passes: seg3d = k, seg2d = j, dist = (float)max(eU, eV), overlap = (float)(ov / Lm).
 * ORDER     camera-major; within a camera ascending k; within k ascending j -- under any schedule.
 * BEST ROW  best[seg_start[c] + j] = the k of the record with the smallest (dist as f32, k) among camera c's records for j; -1 where there is none.
 * OUTPUTS   records: callee-allocated (l3d_free; one spare record); cam_start (m + 1 int64, the caller's): camera c's records are
 *           [cam_start[c], cam_start[c + 1]); best (int32, seg_start[m] of them, the caller's); counts[4] (int64) = rows, eligible columns, records,
 *           columns with a best row.
 * REFUSED before anything is launched, L3D_ERR_INVALID, in this order: a NULL records, cam_start or counts; n or m < 0; a NULL seg3d with n > 0 or
 *           cameras with m > 0; with m > 0 a NULL seg_start, seg_start[0] != 0, a seg_start that descends, a camera with more than 2^31 - 1 segments,
 *           a NULL seg2d or best with seg_start[m] > 0; NULL params; dist_px negative, not finite or NaN; cos_min or min_overlap outside [0, 1] or NaN;
 *           what l3d_project_lines refuses: a camera whose K third row is not exactly (0, 0, 1) or whose size is below 1 x 1, near_z not in
 *           (0, 1.7976931348623157e308], margin not in [0, 2^30]; for l3d_support_lines_device an array whose memory kind or extent fails the check an
 *           l3d_device_image gets, a seg3d not aligned to 8 bytes or a seg2d not aligned to 4.  L3D_ERR_UNSUPPORTED: n > 2^30 (before any launch); a
 *           single camera that alone yields more than 2^31 - 1 records (decided from the count pass's 64-bit totals, before the record list is
 *           allocated), or a record list the device cannot hold.  n == 0 or m == 0: nothing is launched; no records, cam_start and counts all 0, best all -1,
 *           L3D_OK.
 * THE KERNELS.  k_sup_prepare builds the column table of all cameras once (64 bytes a column: U, V, db, Lb and the eligibility).  The search is count /
 *           scan / write over chunks of cameras: 256 threads per workgroup, a lane owns one (camera, 3-D segment) row, the camera is the grid's y
 *           dimension, so a wave never spans two cameras.  A lane projects its row, then walks the camera's columns, staged in LDS tiles of 256 (every
 *           lane reads the same entry: a broadcast).  The tiles of a camera are cut into contiguous chunks along the grid's z dimension when the rows
 *           alone cannot fill the device.  k_sup_count counts per (camera, row, column chunk) and sums every camera's records in 64 bits; k_sup_scan
 *           (one workgroup, l3d_scan.hpp) turns the counts into positions; k_sup_write runs the same functions again and files each lane's records in
 *           ascending j.  There is no floating-point atomic anywhere and the order comes from the scan.  Three launches per chunk whatever n and the
 *           segment counts are (profile names sup_count, sup_scan, sup_write); sup_prepare and sup_best run once per call.  A chunk is L3D_SUP_CHUNK
 *           cameras (0: 64), cut down so that rows x cameras x column chunks stays within 2^30 (the scan's length) and, after its count pass, to the
 *           leading cameras whose records together stay within 2^31 - 1 (the others are counted again with the next chunk); never below one camera.
 *           Sixteen guard slots behind the record list are filled before every write pass and checked after it.  The record list of the whole call
 *           stays on the device until k_sup_best has run over it: a 64-bit integer atomicMin on (bits of dist << 32) | k per column -- a non-negative
 *           float's bits order as its value -- so best does not depend on the schedule either.
 *   l3d_support_lines              seg3d and seg2d in host memory
 *   l3d_support_lines_device       both in device memory, read in place (the caller has synchronised whatever wrote them); everything else host memory
 *   l3d_test_support_lines_host    the same arguments without the context: the same functions in loops, no device.  l3d_support_last_error (per thread)
 *
 * ON THE OBJECT.  The 3-D segments of the current result (l3d_line3d_get_result's order; world coordinates) against the 2-D segments of EVERY view, each
 *           view's camera as it was added (K, R, t and size), views in ascending id; one l3d_support_lines call on the object's context (a node object:
 *           rank 0's, which holds the result).
 *   l3d_line3d_gather_support   valid after a finish, like l3d_line3d_project_result.  params NULL: 3 px, cos(5 degrees), overlap 0.5, near 1e-6, margin 3
 *                               (= dist_px).  One l3d_line_support (24 bytes) per (LINE, view, segment): view_id, seg (the segment's index in its
 *                               view), seg3d (index into l3d_line3d_get_result's seg3d array), dist, overlap, flags.  A (view, segment) that several 3-D
 *                               segments of one line reach is reported once, with the smallest (dist as f32, seg3d).  flags bit 0: the segment is a
 *                               member of this line; bit 1: it is a member of another line; bit 2: this line holds the segment's best row (BEST ROW
 *                               above, over all 3-D segments of the result).  Records are ordered by (line, view id, segment); records:
 *                               callee-allocated (l3d_free; one spare record); line_start (lines + 1 int64, the caller's) delimits each line's records;
 *                               line_views (2 per line, int32, may be NULL): the views with a member, the views with a record; counts[4] (int64):
 *                               records; members found again (records with bit 0); members not found; segments that lie on a line (have a record) and
 *                               are members of none.
 *   l3d_line3d_set_support      off by default; reset keeps the setting, like l3d_line3d_set_merging and l3d_line3d_set_refinement.  With it on, finish /
 *                               compute3Dmodel end with the gather -- after the line fit, the merging and the refinement, as the last step -- with
 *                               dist_px, cos(angle_deg pi / 180) (computed once, on the host, in double), min_overlap, near 1e-6 and margin dist_px, and
 *                               EXTEND the member lists: a record joins its line's 2-D segments iff it has bit 2 set and neither bit 0 nor bit 1, so a
 *                               2-D segment stays in at most one line.  New members are appended behind the old ones in (view id, segment) order; the 3-D
 *                               segments are untouched.  l3d_line3d_get_result, the TXT writer, L3D_SELECT_OBSERVED and the overlay's members layer then
 *                               see the added observations.  With it off nothing is launched and the result is what it was.
 *   l3d_line3d_get_support      what the last finish recorded: counts[4] as above (before the lists were extended) and per line (4 int32 each): original
 *                               members, members added, views with a member before, views with a member after.  Either may be NULL.
 *   REFUSED, L3D_ERR_INVALID: gather_support before a finish has produced a result, with a NULL records, line_start or counts, and what
 *   l3d_support_lines refuses, with its codes; set_support with dist_px negative or not finite, angle_deg outside [0, 90], min_overlap outside [0, 1];
 *   get_support when the last finish ran without the support.
 *
 * OUT OF SCOPE: refinement over the extended members (the refinement runs before the gather, over the members of the line fit); hidden-line reasoning (a segment behind a wall still supports); a spatial index over the
 * columns; a variant whose outputs stay on the device; more than one device.
 * ================================================================================================= */
typedef struct l3d_support_params { double dist_px, cos_min, min_overlap, near_z, margin; } l3d_support_params;
typedef struct l3d_support_record { int32_t seg3d, seg2d; float dist, overlap; } l3d_support_record;
int l3d_support_lines(l3d_ctx* ctx, const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start /* m + 1 */,
                      const l3d_support_params* params, l3d_support_record** records, int64_t* cam_start /* m + 1 */, int32_t* best /* seg_start[m] */,
                      int64_t* counts /* 4 */);
int l3d_support_lines_device(l3d_ctx* ctx, const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start,
                             const l3d_support_params* params, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts);
int l3d_test_support_lines_host(const double* seg3d, int n, const l3d_camera* cameras, int m, const float* seg2d, const int64_t* seg_start,
                                const l3d_support_params* params, l3d_support_record** records, int64_t* cam_start, int32_t* best, int64_t* counts);
const char* l3d_support_last_error(void);
typedef struct l3d_line_support { uint32_t view_id, seg; int32_t seg3d; float dist, overlap; uint32_t flags; } l3d_line_support;
enum { L3D_SUPPORT_MEMBER = 1, L3D_SUPPORT_MEMBER_ELSEWHERE = 2, L3D_SUPPORT_BEST = 4 };
int l3d_line3d_gather_support(l3d_line3d* h, const l3d_support_params* params, l3d_line_support** records, int64_t* line_start /* lines + 1 */,
                              int32_t* line_views /* 2 lines, or NULL */, int64_t* counts /* 4 */);
int l3d_line3d_set_support(l3d_line3d* h, int on, double dist_px, double angle_deg, double min_overlap);
int l3d_line3d_get_support(const l3d_line3d* h, int64_t* counts /* 4 */, int32_t* per_line /* 4 lines */);

/* =================================================================================================
 * JUNCTIONS OF 3-D LINES (no counterpart in the reference; formulas: line3d_amd/csrc/l3d_junction.hpp, numpy model: tests/junction_model.py).  The model is
 * a set of loose segments: nothing says which lines meet, and two edges of one corner end a little short of each other or overshoot.
 * l3d_junction_lines finds where lines meet: an all-pairs closest-approach test on the device, the line ends grouped into vertices, and the free ends
 * that rest on the inside of another line.  The arithmetic is that of MERGING DUPLICATE LINES: everything is f64; every product, sum, quotient and
 * square root is rounded on its own, in the written order (nothing fused); x . y = ((x0 y0) + (x1 y1)) + (x2 y2); max(x, y) is (x < y ? y : x) and
 * min(x, y) is (y < x ? y : x); a comparison with a NaN is false.
 *
 * A LINE OF THE TABLE   P, Q (lines[6 k ..]), L = sqrt((Q - P) . (Q - P)), d = (Q - P) / L, and two numbers in scene units: tol[k] >= 0, how far apart
 *                       two lines may pass, and ext[k] >= 0, how far line k may be prolonged beyond either end.  ELIGIBLE iff the eight numbers and L
 *                       are finite and L > 0.
 * THE PAIR TEST         for eligible i < j.  All of the following must hold:
 *                       1. b = d_i . d_j and |b| <= cos_max (near-parallel pairs belong to the merging)
 *                       2. w = P_i - P_j, p = d_i . w, q = d_j . w, den = 1 - (b b), den > 0; s = ((b q) - p) / den, t = (q - (b p)) / den: the
 *                          parameters of the closest points of the two axes
 *                       3. -ext_i <= s <= L_i + ext_i and -ext_j <= t <= L_j + ext_j
 *                       4. Ci = P_i + (s d_i), Cj = P_j + (t d_j), g = sqrt((Ci - Cj) . (Ci - Cj)), g <= max(tol_i, tol_j)
 * WHERE ON A LINE       where_i from (s, L_i, ext_i), where_j from (t, L_j, ext_j): if s + s <= L: L3D_JUNCTION_END_P (0) iff s <= ext, else
 *                       L3D_JUNCTION_INTERIOR (2); otherwise L3D_JUNCTION_END_Q (1) iff L - s <= ext, else INTERIOR.
 * KIND OF A PAIR        L (0): both at an end; T (1): exactly one at an end; X (2): both interior.  X pairs are listed only when
 *                       params.crossings != 0 (they are skipped when the records are counted and when they are written alike).
 * A RECORD              l3d_junction_record, 64 bytes, for every listed pair: i, j, where_i, where_j, s, t, gap = g, X = (Ci + Cj) 0.5 per coordinate.
 *                       Records are ordered ascending by (i, j) under any schedule.
 * VERTICES              The nodes are the line ends, 2 k + e (e = 0 for P, 1 for Q).  Every L record is an edge between its two nodes
 *                       (2 i + where_i, 2 j + where_j); a vertex candidate is a connected component of that graph.  Its REPRESENTATIVE is the node of the
 *                       longest line, at equal L the lowest node index.  A node STAYS iff it is the representative, or the pair test between its line
 *                       and the representative's line passes as an L pair at exactly these two ends (the star rule of the merging, for the same reason:
 *                       a row of short lines must not collapse into one vertex; hence at most one end of a line stays in a vertex, and the other end
 *                       of the representative's line never stays).  Every other node of a component with an edge is RELEASED.  A VERTEX is a
 *                       component's staying set when it has two or more nodes.  Its position: S = 0, then S = S + X, per coordinate, over the records
 *                       between the representative and every other staying node, in ascending order of that node's index; then S / m, m = the number of
 *                       those records as a double.  Vertices are numbered in the order of their lowest staying nodes.
 * ATTACHMENTS           for a node that is in no vertex: node_attach[node] = the index of the T record in which this node is the end, among several
 *                       the one with the smallest (gap, record index); -1 if there is none, and -1 for every node of a vertex.
 * OUTPUTS               records: callee-allocated (l3d_free; one spare record), *n_records; node_vertex[2 n]: the vertex index or -1; vertices:
 *                       callee-allocated l3d_junction_vertex (X, first_node = the lowest staying node, degree = the staying nodes), *n_vertices;
 *                       node_attach[2 n]; counts[8] = eligible lines, L records, T records, X records, components with an edge, vertices, nodes
 *                       released, nodes attached.
 * REFUSED before anything is launched, L3D_ERR_INVALID: a NULL output; n < 0; a NULL array with n > 0; NULL params; cos_max outside [0, 1) or NaN; a
 *   negative or NaN tol or ext.  L3D_ERR_UNSUPPORTED: n > 2^30 (before any launch; n = 2^30 itself has 2^31 nodes, one more than the components' int
 *   labels number, and is answered the same way by the device call); more than 2^31 - 1 records, decided from the count pass's 64-bit total with
 *   no allocation attempted; a record list the device cannot hold.  n == 0: empty outputs, L3D_OK.
 * THE KERNELS (l3d_junction.hip).  k_junc_prepare builds the table, 80 bytes a line.  The search is k_junc_count / k_junc_scan / k_junc_write: 256
 *   threads per workgroup, one row line per lane, column tiles of 256 lines staged in LDS and read as broadcasts, rows j > i only, column chunks along
 *   the grid's y dimension when rows alone cannot fill the device, positions from one scan: three launches whatever n is.  Sixteen guard records behind
 *   the list are filled before the write pass and checked after it.  The write pass also files one edge per record for the components (k_cc_init /
 *   k_cc_hook / k_cc_compress over the 2 n nodes; a record that is no L pair files an edge from node 0 to itself).  k_junc_rep (two phases: integer
 *   atomicMax on the bits of L, atomicMin on the node) names the representatives, k_junc_star decides who stays, k_junc_flag and k_junc_vscan number
 *   the vertices, k_junc_keys writes one 64-bit key (lowest staying node, node) per staying node that is not the representative, a radix sort
 *   (junc_sort) orders them, and k_junc_vertex -- one lane per vertex, walking its keys -- sums the positions in the stated order.  k_junc_attach (two
 *   phases over the records: atomicMin on the bits of gap, then on the record index) and k_junc_finish give the attachments.  No floating-point atomic
 *   anywhere.  Profile names: junc_*.
 *   l3d_junction_lines             the device
 *   l3d_test_junction_lines_host   the same arguments without the context: the same functions in loops, no device, bit-equal.
 *   l3d_junction_last_error        per thread
 *
 * ON THE OBJECT.  Per line of the result: P = the start of its first 3-D segment, Q = the end of its last; tol = dist_px x sigma, sigma exactly as
 *           step 1 of the merging defines it (the mean of z / f over the members' views); ext = min(ext_px x sigma, max_ext_rel x L);
 *           cos_max = cos(angle_min_deg pi / 180), computed once on the host in double; no crossings.  One l3d_junction_lines call on the object's
 *           context (a node object: rank 0's, which holds the result; a sharded finish: every rank that has the option set, each with the same bytes).
 *   l3d_line3d_set_junctions    off by default; reset keeps the setting.  With it on, finish / compute3Dmodel run the junctions after the merging and
 *                               the refinement and before the support gather.  snap != 0: an end that stays in a vertex moves to the foot of the
 *                               vertex position on its own axis, P + ((X - P) . d) d, and an attached end to its own closest point Ci (P + s d with the
 *                               record's parameter); P and d are the line's before any move.  The start of the first 3-D segment or the end of the
 *                               last one is replaced, the P end first; the 2-D members are untouched.  A move after which
 *                               (far end - new end) . (far end - old end) > 0 fails for that 3-D segment would reverse or annihilate it: it is
 *                               skipped and counted.  With the option off nothing is launched and the result is what it was.
 *   l3d_line3d_get_junctions    what the last finish recorded: vertices (callee-allocated, l3d_free; one spare), per line 4 int32 (vertex of the P end,
 *                               vertex of the Q end, the line the P end is attached to, the line the Q end is attached to; -1: none) and counts[10]:
 *                               the eight of l3d_junction_lines, the ends moved, the moves skipped.  Any output may be NULL.
 *   l3d_line3d_save_wireframe   the current result as a Wavefront OBJ: one "v" line per vertex of the last finish's junctions, in vertex order (none when
 *                               that finish ran without the option), then per line k "g line_<k>" and, per 3-D segment, a "v" line for each end that is
 *                               not shared and "l a b"; the start of the first and the end of the last 3-D segment of a line whose end stays in a vertex
 *                               use that vertex's index.  Coordinates are written as %.17g: the file parses back to the same doubles.
 *   REFUSED, L3D_ERR_INVALID: set_junctions with dist_px or ext_px negative or not finite, angle_min_deg outside (0, 90], max_ext_rel outside [0, 0.5];
 *   get_junctions when the last finish ran without the junctions; save_wireframe without a result or a file that cannot be written.
 *
 * OUT OF SCOPE: faces or planes from the wireframe (they have a section of their own: PLANES OF 3-D LINES, below); junctions across objects or devices; a spatial index over the columns; outputs that stay on the
 * device; refitting lines so that they pass exactly through their vertices (snapping only moves ends along their own axes); hidden-line reasoning.
 * ================================================================================================= */
enum { L3D_JUNCTION_END_P = 0, L3D_JUNCTION_END_Q = 1, L3D_JUNCTION_INTERIOR = 2 };
typedef struct l3d_junction_params { double cos_max; int32_t crossings, pad; } l3d_junction_params;
typedef struct l3d_junction_record { int32_t i, j, where_i, where_j; double s, t, gap; double X[3]; } l3d_junction_record;
typedef struct l3d_junction_vertex { double X[3]; int32_t first_node, degree; } l3d_junction_vertex;
int l3d_junction_lines(l3d_ctx* ctx, const double* lines /* 6 n: P, Q */, const double* tol /* n */, const double* ext /* n */, int n,
                       const l3d_junction_params* params, l3d_junction_record** records, int* n_records, int32_t* node_vertex /* 2 n */,
                       l3d_junction_vertex** vertices, int* n_vertices, int32_t* node_attach /* 2 n */, int32_t* counts /* 8 */);
int l3d_test_junction_lines_host(const double* lines, const double* tol, const double* ext, int n, const l3d_junction_params* params,
                                 l3d_junction_record** records, int* n_records, int32_t* node_vertex, l3d_junction_vertex** vertices, int* n_vertices,
                                 int32_t* node_attach, int32_t* counts);
const char* l3d_junction_last_error(void);
int l3d_line3d_set_junctions(l3d_line3d* h, int on, double dist_px, double ext_px, double angle_min_deg, double max_ext_rel, int snap);
int l3d_line3d_get_junctions(const l3d_line3d* h, l3d_junction_vertex** vertices, int* n_vertices, int32_t* per_line /* 4 lines */, int32_t* counts /* 10 */);
int l3d_line3d_save_wireframe(const l3d_line3d* h, const char* filename);

/* =================================================================================================
 * PLANES OF 3-D LINES (no counterpart in the reference; formulas: line3d_amd/csrc/l3d_plane.hpp, numpy model: tests/plane_model.py).  A wireframe says
 * which lines meet; l3d_plane_lines says which lines lie in one plane and where that plane is: every pair of lines that meet (a SEED) spans a plane
 * hypothesis, hypotheses that agree are grouped, the group's plane is an area-weighted average, and every line of the table that lies in it is a
 * member.  The arithmetic is that of MERGING DUPLICATE LINES and of the JUNCTIONS: everything is f64; every product, sum, quotient and square root is
 * rounded on its own, in the written order (nothing fused); x . y = ((x0 y0) + (x1 y1)) + (x2 y2);
 * a x b = ((a1 b2) - (a2 b1), (a2 b0) - (a0 b2), (a0 b1) - (a1 b0)); max(x, y) is (x < y ? y : x) and min(x, y) is (y < x ? y : x); a comparison
 * with a NaN is false.
 *
 * INPUTS                lines[6 n] (P, Q per line), tol[n] >= 0 in scene units, seeds[2 m]: int32 pairs (i, j) of lines that meet, and the parameters
 *                       cos_max, cos_min, min_lines.
 * A LINE OF THE TABLE   L = sqrt((Q - P) . (Q - P)), d = (Q - P) / L.  ELIGIBLE iff the seven numbers and L are finite and L > 0.
 * LIES IN (k; N, c)     line k lies in the plane (N, c) iff |(N . P_k) - c| <= tol_k and |(N . Q_k) - c| <= tol_k.
 * A HYPOTHESIS h        from seed h = (i, j).  ELIGIBLE iff i != j, both lines are eligible, b = d_i . d_j with |b| <= cos_max, den = 1 - (b b) > 0,
 *                       cr = d_i x d_j, mm = sqrt(cr . cr) > 0.  Then N_h = cr / mm; with w = P_i - P_j, p = d_i . w, q = d_j . w,
 *                       s = ((b q) - p) / den, t = (q - (b p)) / den, Ci = P_i + (s d_i), Cj = P_j + (t d_j): X_h = (Ci + Cj) 0.5 per coordinate,
 *                       c_h = N_h . X_h, and the weight A_h = (L_i L_j) mm (twice the area of the triangle the two lines span).  Two seeds of the
 *                       same pair are two hypotheses.
 * THE PAIR TEST         for eligible hypotheses h < g: |N_h . N_g| >= cos_min, both lines of g LIE IN (N_h, c_h) and both lines of h LIE IN
 *                       (N_g, c_g).  Every passing pair is an edge; a plane CANDIDATE is a connected component of that graph over the eligible
 *                       hypotheses, singletons included.
 * THE STAR RULE         the REPRESENTATIVE of a component is the hypothesis with the largest A, at equal A the lowest index.  A hypothesis STAYS iff
 *                       it is the representative or passes the pair test against it; the others are RELEASED (the merging's reason: a fan of slowly
 *                       turning hypotheses must not collapse into one plane).
 * PARAMETERS            over the staying hypotheses of a candidate in ascending index: sg_h = -1 if N_h . N_rep < 0, else 1;
 *                       S = S + ((A_h sg_h) N_h) per coordinate from S = 0; W = W + A_h from 0; N = S / sqrt(S . S); then T = T + (A_h (N . X_h)) from
 *                       0 and c = T / W.
 * FRAME                 with d of line i of the representative's seed: u' = d - ((d . N) N), lu = sqrt(u' . u'), u = u' / lu, v = N x u, O = c N.
 * MEMBERS               an eligible line k is a MEMBER of the candidate iff it LIES IN (N, c); flag bit 0 (L3D_PLANE_SEED) iff it is a line of one of
 *                       the candidate's staying hypotheses.  A line may be a member of several planes (a box edge lies in two).
 * KEPT                  a candidate is KEPT iff sqrt(S . S), W and lu are finite and > 0 (otherwise no line is tested against it) and its members number
 *                       at least min_lines.  Planes are the kept candidates, numbered in the order of their lowest staying hypotheses.
 * EXTENT                rect = (min a, max a, min b, max b) of a = u . (X - O), b = v . (X - O) over both ends X of all members.
 * OUTPUTS               planes: callee-allocated l3d_plane, 128 bytes (N, c, u, v, rect; rep, first_hyp = the lowest staying hypothesis, n_hyp = the
 *                       staying hypotheses, n_lines = the members), *n_planes; members: callee-allocated l3d_plane_member (plane, line, flags, pad),
 *                       ascending by (plane, line) under any schedule, *n_members; one spare record follows each list (l3d_free); hyp_plane[m]: the
 *                       plane a seed stays in, or -1; counts[8] = eligible lines, eligible hypotheses, hypothesis edges, components (candidates),
 *                       hypotheses released, candidates dropped, planes, member records.
 * REFUSED before anything is launched, L3D_ERR_INVALID: a NULL output; n or m < 0; a NULL array with n or m > 0; NULL params; cos_max outside [0, 1),
 *   cos_min outside (0, 1], min_lines < 2; a negative or NaN tol; a seed index outside [0, n).  L3D_ERR_UNSUPPORTED: n or m above 2^30 (before any
 *   launch); more than 2^31 - 1 edges or member records, decided from the count pass's 64-bit total with nothing allocated; more than 2^30 wave words
 *   in the membership pass (candidates x ceil(n / 64)); a list the device cannot hold.  n == 0 or m == 0: nothing is launched, empty outputs, counts
 *   all zero, L3D_OK.
 * THE KERNELS (l3d_plane.hip).  k_plane_prepare builds the line table (96 bytes a line), k_plane_hyp the hypothesis table, one lane per seed (160
 *   bytes a hypothesis: its plane and its two lines' ends and tolerances, plus 32 bytes for X and A).  The hypothesis search is k_plane_count /
 *   k_plane_scan / k_plane_write: 256 threads per workgroup, one row hypothesis per lane, column tiles of 256 hypotheses staged in LDS (40 KB) and
 *   read as broadcasts, rows g > h only, column chunks along the grid's y dimension when rows alone cannot fill the device, positions from one scan:
 *   three launches whatever m is; sixteen guard records behind the edge list are filled before the write pass and checked after it.  Components:
 *   k_cc_init / k_cc_hook / k_cc_compress.  k_plane_rep (two phases: integer atomicMax on the bits of A, atomicMin on the index), k_plane_star,
 *   k_plane_flag and a scan number the candidates; k_plane_keys writes a key (lowest staying hypothesis, hypothesis) per staying hypothesis, a radix
 *   sort orders them, and k_plane_param -- one lane per candidate, walking its keys -- sums in the stated order.  Membership tests every (candidate,
 *   line) pair, one pair per lane with a ballot word per wave: k_plane_mcount, then k_plane_keep (the keep flags, the 64-bit total), a scan that
 *   numbers the planes, k_plane_mmask (the words of dropped candidates count nothing), k_plane_mscan and k_plane_mwrite; k_plane_seed sets the
 *   SEED flags (integer atomicOr), k_plane_extent -- one lane per plane over its records -- the extents, k_plane_finish hyp_plane.  The number of
 *   launches does not depend on n or m beyond the components' rounds.  No floating-point atomic anywhere.  Profile names: plane_*.
 *   l3d_plane_lines             the device
 *   l3d_test_plane_lines_host   the same arguments without the context: the same functions in loops, no device, bit-equal.
 *   l3d_plane_last_error        per thread
 *
 * ON THE OBJECT.  Per line of the result: P = the start of its first 3-D segment, Q = the end of its last, as the junctions left them (after their snap);
 *           tol = dist_px x sigma, the sigma the junction search computed for the line (before any snap); cos_max = the junctions' own,
 *           cos(angle_min_deg pi / 180); cos_min = cos(angle_deg pi / 180), computed once on the host in double; the seeds are the L and T records of the
 *           junction search, in record order.  One l3d_plane_lines call on the object's context (a node object: rank 0's, which holds the result; a
 *           sharded finish follows the junctions).
 *   l3d_line3d_set_planes       off by default (4 px, 10 degrees, 3 lines); reset keeps the setting.  With it on, finish / compute3Dmodel run the planes
 *                               after the junctions and before the support gather.  With the junctions option off the junction search runs all the
 *                               same, with the junctions' stored parameters and without snap; its vertices are discarded and l3d_line3d_get_junctions
 *                               still refuses.  With the planes option off nothing is launched and every output is what it was.
 *   l3d_line3d_get_planes       what the last finish recorded: the planes and the member records (callee-allocated, l3d_free; one spare each), per line
 *                               the number of planes it lies in, and the counts[8] of l3d_plane_lines.  Any output may be NULL.
 *   l3d_line3d_save_planes      the planes of the last finish as a Wavefront OBJ: per plane k "g plane_<k>", four "v" lines -- the corners
 *                               ((c N) + (a u)) + (b v) of its rectangle for (a, b) = (rect0, rect2), (rect1, rect2), (rect1, rect3), (rect0, rect3),
 *                               written as %.17g: the file parses back to the same doubles -- and one "f" line.  l3d_line3d_save_wireframe is unchanged.
 *   REFUSED, L3D_ERR_INVALID: set_planes with dist_px negative or not finite, angle_deg outside [0, 90), min_lines < 2; get_planes and save_planes when
 *   the last finish ran without the planes; a file that cannot be written.
 *
 * OUT OF SCOPE: polygonal face boundaries or a closed mesh; a least-squares refit beyond the stated average; moving lines into their planes; seeds
 * from parallel coplanar lines; a reach limit on members; hidden-line removal; planes across objects or devices; outputs that stay on the device.
 * ================================================================================================= */
enum { L3D_PLANE_SEED = 1 };
typedef struct l3d_plane_params { double cos_max, cos_min; int32_t min_lines, pad; } l3d_plane_params;
typedef struct l3d_plane { double N[3], c, u[3], v[3], rect[4]; int32_t rep, first_hyp, n_hyp, n_lines; } l3d_plane;
typedef struct l3d_plane_member { int32_t plane, line, flags, pad; } l3d_plane_member;
int l3d_plane_lines(l3d_ctx* ctx, const double* lines /* 6 n: P, Q */, const double* tol /* n */, int n, const int32_t* seeds /* 2 m */, int m,
                    const l3d_plane_params* params, l3d_plane** planes, int* n_planes, l3d_plane_member** members, int* n_members,
                    int32_t* hyp_plane /* m */, int32_t* counts /* 8 */);
int l3d_test_plane_lines_host(const double* lines, const double* tol, int n, const int32_t* seeds, int m, const l3d_plane_params* params,
                              l3d_plane** planes, int* n_planes, l3d_plane_member** members, int* n_members, int32_t* hyp_plane, int32_t* counts);
const char* l3d_plane_last_error(void);
int l3d_line3d_set_planes(l3d_line3d* h, int on, double dist_px, double angle_deg, int min_lines);
int l3d_line3d_get_planes(const l3d_line3d* h, l3d_plane** planes, int* n_planes, l3d_plane_member** members, int* n_members, int32_t* per_line /* lines */,
                          int32_t* counts /* 8 */);
int l3d_line3d_save_planes(const l3d_line3d* h, const char* filename);

/* The detector's stages on their own, exported for tests (tests/test_gpu_detect_stages.py): the same kernels with the same launch shapes
 * as l3d_detect_segments, results copied to caller-allocated arrays.  (N, M) = (ceil(0.8 new_width), ceil(0.8 new_height)) is the scaled image.
 *   pixel stage   grey[new_width x new_height] after rescale + grey; img / mod / ang [N x M]: the Gaussian sampler's output, the 2x2 gradient's
 *                 modulus and the level-line angle (-1024 = not defined); bucket[2 N M]: per pixel the angle's bucket in partition 0 and in
 *                 partition 1 (255 = none)
 *   label         bucket as above, active[N M] (0 / 1) -> parent[2 N M]: per partition the smallest pixel index of the pixel's component
 *                 (-1 for an inactive pixel); key[N M]: the region the pixel votes for, partition x N M + root, 2 N M for none
 *   regions       the region kernel on a given labelling (key as above) with every pixel active before it: one record per region of at
 *                 least min_reg (>= 2) pixels, in ascending key order (callee-allocated, l3d_free), and the active map afterwards
 *   nfa           -log10 NFA of (n[i], k[i], p[i]) as the region kernel computes it */
typedef struct {
    uint32_t minpix;                    /* smallest pixel index among the pixels used */
    int32_t n_used, steps;              /* pixels within the last radius; shrink steps taken (0: the whole region) */
    int32_t pts, alg;                   /* points in / aligned with the final rectangle */
    int32_t scored, accepted;           /* density reached 0.7 and the rectangle was scored; it passed */
    int32_t pad;
    int32_t hist_n[8];                  /* pixels within the radius at steps 0..7 (0: step not reached) */
    double cx, cy, x1, y1, x2, y2, width, theta, density;  /* the rectangle from the moments, scaled-image coordinates (before + 0.5, / 0.8) */
    double fx1, fy1, fx2, fy2, fwidth, p, nfa;              /* the rectangle, probability and value after the retries */
} l3d_detect_region_record;
int l3d_test_detect_pixel_stage(l3d_ctx* ctx, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, int new_width, int new_height,
                                float* grey, double* img, double* mod, double* ang, unsigned char* bucket, int* N, int* M);
int l3d_test_detect_label(l3d_ctx* ctx, const unsigned char* bucket, const unsigned char* active, int N, int M, int32_t* parent, uint32_t* key);
int l3d_test_detect_regions(l3d_ctx* ctx, int N, int M, const double* mod, const double* ang, const uint32_t* key, int min_reg,
                            l3d_detect_region_record** rec, int* n_rec, unsigned char* active_out);
int l3d_test_detect_nfa(l3d_ctx* ctx, const int32_t* n, const int32_t* k, const double* p, double logNT, int count, double* out);

/* Stage 2 (K_verify_matches) on a candidate list of the caller's, exported for tests (tests/test_gpu_verify_variants.py): one source view's
 * packed candidates as stage 1 leaves them, through the product's own argument set-up and launchers, on the path `sel` names.
 *   src_segs S x 4, tgt_segs n_tgt x 4, offsets N x (start, count), P N x 3 x 4, RtKinv_src 3 x 3, C_src 3: as l3d_compute_pairwise_matches
 *   row_start     S*N + 1   row = segment * N + camera; row_start[S*N] == R
 *   cand_meta     R x (target id within its camera, camera); cand_depths R x 4 (the first two are the hypothesis' depths, positive by contract)
 * sel->path 0: the all-pairs kernel and the epilogue launch.  1: the per-view seam call's launches -- the window kernel on the segments that fit
 * the LDS image, again on a global scratch when one outgrows it, the epilogue launch.  2: the chains' single launch with the fused epilogue;
 * gb = 1 keeps the bucket starts in global memory when N > 16, split_unit > 0 (a multiple of 256) verifies the long segments in units of that
 * many hypotheses by a second launch, seg_order (NULL or a permutation of the segments; path 2 only) is the order the workgroups take them in.
 * mmax: 0 = the LDS image sized as the call site sizes it from the largest segment, else that many candidates, cut down to what the LDS budget
 * allows either way.  wide_max: launches of up to this many segments may take the 8-wave kernel (0: never).
 * Out: conf[R], kept_cnt[S] (confidence > 1), best_depths[S x 2] (the first candidate with the segment's largest confidence; (-1, -1) when
 * that is not above 0.5); sel->mmax_used, sel->kernels (L3D_VK_*: the kernels launched).
 * Checked before anything is launched, L3D_ERR_INVALID with a message otherwise: row_start ascends from 0 to R, every candidate's camera is its
 * row's, every target id is below its camera's count, the offsets stay inside n_tgt, R < 2^24, 1 <= N <= 255, the selection's ranges, and for
 * paths 1 and 2 that the window kernels take N neighbours. */
#define L3D_VK_ALL_PAIRS 1u
#define L3D_VK_SEG_POST 2u
#define L3D_VK_WINDOW_256 4u     /* k_verify_window, 4 waves */
#define L3D_VK_WINDOW_512 8u     /* k_verify_window, 8 waves */
#define L3D_VK_WINDOW_GB 16u     /* k_verify_window_gb */
#define L3D_VK_BUILD 32u         /* k_verify_window_build */
#define L3D_VK_WALK 64u          /* k_vw_walk, bucket starts in LDS */
#define L3D_VK_WALK_GB 128u      /* k_vw_walk, bucket starts in global memory */
typedef struct l3d_test_verify_path {
    int32_t path, gb, split_unit, mmax, wide_max;
    int32_t mmax_used;              /* out */
    uint32_t kernels;               /* out */
    int32_t pad;
    const int32_t* seg_order;
    const int32_t* exist_cams;      /* path 2: n_exist_cams local cameras, ascending, whose rows hold their candidates in ANY order: the window kernel */
    int32_t n_exist_cams, pad2;     /* puts each (segment, camera) run into ascending target order before it verifies, as it does with reverse matches */
    uint32_t* cand_meta_out;        /* out (NULL or R x 2, R x 4): the candidate arrays as the kernels left them */
    float* cand_depths_out;
} l3d_test_verify_path;
int l3d_test_verify_candidates(l3d_ctx* ctx, int S, int N, const float* src_segs, const float* tgt_segs, int n_tgt, const int32_t* offsets, const float* P,
                               const float* RtKinv_src, const float* C_src, const int32_t* row_start, const uint32_t* cand_meta, const float* cand_depths, int R,
                               float sigma_p, float sigma_a, float spatial_k, l3d_test_verify_path* sel, float* conf, int32_t* kept_cnt, float* best_depths);

/* Stage 1 (K_pairwise_matches and the packing of its candidates) of one source view, exported for tests (tests/test_gpu_stage1_paths.py): the
 * product's own argument set-up and launchers on the launch sequence `sel->path` names, with no existing matches.
 *   S, N, src_segs, tgt_segs (n_tgt x 4), offsets, F, RtKinv, centers, RtKinv_src, C_src, to_be_matched: as l3d_compute_pairwise_matches
 * path 0: the per-view seam call -- bit rows with the depth test inside, k_row_count, the row scan, k_pair_fill.
 * path 1: the resident chain with fused row starts (N <= 96) -- k_pair_mask counts upper bounds and their 256-row block sums, k_pair_fill forms
 *         the row starts from them, triangulates, drops the pairs without four positive depths, packs the row and writes its true count.
 * path 2: the chains with a scan launch in between -- over all rows when the range is [0, S) (resident chain, N > 96), over the range's rows
 *         otherwise (sharded chain).
 * pretest: the stage-1 filter mask 0..7 (option "pretest").  spb: 0 = the launcher's rule, else source segments per k_pair_mask workgroup
 * (option "pair_spb").  [seg_begin, seg_end): the source segments processed.  Paths 1 and 2 only: ray_tables 1 = the viewing-ray tables of
 * k_tgt_rays as the chains make them, 0 = none (k_pair_fill normalises the rays itself); cand_cap = the candidate capacity the kernels guard
 * (0: the sum of the upper bounds, i.e. exactly enough).  capacity: slots of the caller's cand_meta / cand_depths.
 * Out, rows indexed segment * N + camera:
 *   row_upper  S*N      what k_pair_mask counted: pairs that pass the overlap test (paths 1, 2); on path 0 k_row_count's result (== row_count)
 *   row_count  S*N      candidates of the row (four positive depths); with sel->overflow on paths 1 and 2: the upper bounds
 *   row_start  S*N + 1  path 0: exclusive prefix of row_count over all rows, [S*N] = their total.  Paths 1 and 2: exclusive prefix of
 *                       row_upper -- a row's candidates are packed at the front of the room of its upper bound.  Path 1 writes the rows with
 *                       row_upper > 0 only, path 2 with a partial range the rows [seg_begin * N, seg_end * N] and [S*N].
 *   cand_meta  capacity x (target id within its camera, camera); cand_depths capacity x 4
 *   sel->total, sel->largest: sum and largest per-segment sum of the counts the path scans (path 0: row_count, path 2: row_upper; path 1
 *   computes none: -1); sel->spb_used; sel->overflow (paths 1, 2: the upper bounds exceed cand_cap -- no candidate is written); sel->needed:
 *   the slots the result takes (path 0: the candidates, paths 1 and 2: the sum of the upper bounds).
 * The row starts and max(capacity, needed) candidate slots on the device are filled with 0xff bytes before the launches: what no kernel wrote
 * stays recognisable.  (The row counters are zeroed as the product zeroes them: its kernels add into them.)  capacity < needed: L3D_ERR_INVALID
 * with the number in the message and in sel->needed, row_upper / row_count / row_start filled in, no candidates.
 * Refused before any launch, L3D_ERR_INVALID with a message: a camera of to_be_matched with more than 16384 segments, to_be_matched not strictly
 * ascending or outside [0, N), offsets outside n_tgt, a range outside [0, S], path / pretest / spb out of range, path 1 with N > 96, N > 255,
 * cand_cap or ray_tables set on path 0. */
typedef struct l3d_test_pair_path {
    int32_t path, pretest, spb, seg_begin, seg_end, ray_tables, cand_cap, capacity;
    int32_t needed, total, largest, spb_used, overflow;     /* out */
    int32_t pad;
} l3d_test_pair_path;
int l3d_test_pair_candidates(l3d_ctx* ctx, int S, int N, const float* src_segs, const float* tgt_segs, int n_tgt, const int32_t* offsets, const float* F,
                             const float* RtKinv, const float* centers, const float* RtKinv_src, const float* C_src, const int32_t* to_be_matched, int n_tbm,
                             l3d_test_pair_path* sel, int32_t* row_upper, int32_t* row_count, int32_t* row_start, uint32_t* cand_meta, float* cand_depths);

/* The products of matchViews (l3d_match_chain_resident's last step: the table of potential correspondences, the best-match references, the medians,
 * the early-return quirk) built from kept lists the CALLER hands in, exported for tests (tests/test_gpu_products_paths.py): the lists go where a
 * chain leaves them (the kept arena, the best depth pairs, the best positions), then the product's own builder runs on them.  No chain runs.
 *   views, n_views   the schedule; read: view_id, S_src (<= 16384), N (<= 255), local2global, n_tbm (0 = the view returned early), source_cam,
 *                    source_index, n_sources
 *   map              the dense map (every chain view is in it, with S_src segments)
 *   kept, n_kept     the kept lists of the chain views one after the other, GLOBAL camera ids; n_kept[k] records of view k (0 for an early return)
 *   n_candidates     per chain view, the candidates its verification saw (0: the median stays 1.0)
 *   best, bestpos    per segment of every chain view, view after view (S_src entries each, those of early-return views unread): the depth pair of the
 *                    best hypothesis ((-1, -1): none) and the position of the best kept match in the view's list (-1: none; checked against n_kept)
 * sel in:  side_arrays 0 = the builder rebuilds the side words and run tables of the lists block by block; 1 = they are made here first, for every
 *          list, by the launchers the chains use for lists taken over (l3d_runtable.hpp), and handed over as the chain hands its own.  Lists those
 *          launchers find unordered get none: the builder is then called as with 0, and side_arrays_used says so.
 *          early_pairs 1 (needs side_arrays 1): the (view, camera) pairs are transposed view by view as the chain does on its side stream.
 *          [dv0, dv1) with dv1 >= 0: the rows of these dense views only, numbered from 0; held (NULL or one byte per chain view): with a row range,
 *          the rows outside it are left empty and the whole of pot_start is valid.
 * sel out: build (1 transposed, 2 sorted), refused (why the transposed build handed over to the sort: 0 it did not, 1 a view of more than 16000
 *          segments, 2 a list that is not ordered or names a camera that is no neighbour), n_blocks, max_touch (the most views a row of the transposed
 *          build touches), early_cap / early_g and, for the first block_capacity blocks of the transposed build, block_cap / block_staged / block_g
 *          (any of the three may be NULL): the LDS image of the pair transposes' two-level scatter in entries (0: direct scatter, -1: no transpose was
 *          launched for the block), whether short rows are staged by the counting pass, the lanes that share a run.
 * Afterwards l3d_chain_products_get, l3d_chain_kept_list and l3d_chain_records_digest answer as after l3d_match_chain_resident (with a row range:
 * the rows of the range, and *n_pot their entries).  Refused with L3D_ERR_INVALID before anything is uploaded: counts out of range, a best position
 * outside its list, records for an early-return view, early_pairs without side_arrays or with a view of more than 16382 segments. */
typedef struct l3d_test_products_path {
    int32_t side_arrays, early_pairs, dv0, dv1;
    const unsigned char* held;
    int32_t block_capacity;
    int32_t side_arrays_used, build, refused, n_blocks, max_touch, early_cap, early_g;     /* out */
    int32_t* block_cap; int32_t* block_staged; int32_t* block_g;                            /* out, block_capacity entries each */
} l3d_test_products_path;
int l3d_test_products(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, const l3d_dense_map* map, const l3d_match* kept, const int32_t* n_kept,
                      const int64_t* n_candidates, const float* best, const int32_t* bestpos, l3d_test_products_path* sel,
                      l3d_chain_summary* summary, int64_t* n_pot);

/* The step of the resident chain between stage 1 and the verification, on ONE view and on kept lists the caller hands in, exported for tests
 * (tests/test_gpu_collect_paths.py): the reverse matches counted out of the earlier views' lists, the row scan, stage-1 rows and reverse matches merged
 * into one candidate list in (segment, camera, target) order.  The lists go where a chain leaves them (arena, result records; side words and run tables
 * made by the launchers the chains use for lists taken over), then the chain's own code for the step runs with the chain's own rules.
 *   views, n_views   the schedule as l3d_test_products reads it: view_id, S_src (<= 16384), N (<= 255), local2global, n_tbm (0: never verified -- no list,
 *                    no run table), to_be_matched, source_cam, source_index, n_sources; k: the view under test (n_tbm > 0)
 *   kept, n_kept     the kept lists of the views [0, k) one after the other, GLOBAL camera ids, each in (segment, local camera) order; overflowed (NULL or
 *                    one byte per view): the view's result record carries overflow bit 2 and n_kept = 0, as the writer leaves it; its records stay
 *                    in the arena, unread
 *   rowA, metaA, depthsA, n_A   view k's stage-1 rows: start per row (read for the cameras to be matched; gaps allowed), n_A candidates
 *   rowcnt           S*N true stage-1 row counts (0 for cameras that are not to be matched)
 * sel in:  route 0 = records scanned (k_exist_count / k_place), 1 = run tables (k_exist_count_rt + k_exist_combine / k_place_rt); rt_g = option rt_g for
 *          this call; avg_kept = the average kept per view the chain's rules (workgroups per source, lanes per run) are fed with; cand_cap = the
 *          candidate capacity the kernels guard, also the entries of cand_meta / cand_depths; sort_apart 1 = the separate sort launch runs.
 * out:     row_start S*N + 1, cursor S*N (zeroed by the scan, advanced by the scatter), seg_order S, cand_meta cand_cap x 2 and cand_depths cand_cap x 4
 *          (0xff bytes where no kernel wrote); sel->kernels (L3D_CK_*), g, bps (workgroups per source of the route taken), blocks_move, R.
 * Refused with L3D_ERR_INVALID before anything is launched: sizes out of range, a source that is not an earlier view or whose camera is also to be
 * matched, a record whose segment is past its view's, a list that is not ordered or names a camera that is no neighbour, a stage-1 row outside n_A, a
 * stage-1 count for a camera that is not to be matched. */
#define L3D_CK_EXIST_COUNT 1u
#define L3D_CK_EXIST_COUNT_RT 2u /* k_exist_count_rt + k_exist_combine */
#define L3D_CK_SCAN 4u
#define L3D_CK_PLACE 8u
#define L3D_CK_PLACE_RT 16u
#define L3D_CK_SORT_RUNS 32u
typedef struct l3d_test_collect_path {
    int32_t route, rt_g, sort_apart, cand_cap;
    double avg_kept;
    const unsigned char* overflowed;
    uint32_t kernels;                                   /* out */
    int32_t g, bps, blocks_move, R, pad;                /* out */
} l3d_test_collect_path;
int l3d_test_collect_candidates(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, int k, const l3d_match* kept, const int32_t* n_kept,
                                const int32_t* rowA, const uint32_t* metaA, const float* depthsA, int n_A, const int32_t* rowcnt,
                                l3d_test_collect_path* sel, int32_t* row_start, uint32_t* cand_meta, float* cand_depths, int32_t* cursor, int32_t* seg_order);

/* The kept writer of the chains (k_kept_write_chain: records, side words, run table, best positions, result record) on ONE view's verified
 * candidates, handed in by the caller, and the rebuild of side words and run tables from records (the launchers the chains use for lists taken
 * over from another rank), exported for tests (tests/test_gpu_kept_write.py).  No chain runs; the product's own launchers do.
 *   row_start S*N + 1, cand_meta R x (target, local camera), cand_depths R x 4, cand_conf R: as the verification leaves them
 *   kept_cnt S            candidates of the segment with a confidence above 1 (checked on the host: the writer places a segment behind the
 *                         counts in front of it)
 *   local2global N        the view's neighbours
 * sel in:  writer 0 = the chain's writer: the view's slice starts at prev_base + prev_n_kept when has_prev is set (the result record of the view
 *          before it), at 0 otherwise; cand_cap and arena_cap are what the kernel guards (R > cand_cap: overflow bit 1; a slice that ends past
 *          arena_cap records: bit 2, n_want = the view's count, n_kept = 0; nothing is written either way).  writer 1 = the per-view seam call's
 *          writer behind the scan of kept_cnt: records only, from position 0; arena_cap must hold them.
 *          jobs, n_jobs: lists to rebuild side words and run tables of afterwards, all in one launch -- records == NULL: the list the writer just
 *          left (S, N, local2global of the call; n is filled in), else n records of the caller's with GLOBAL camera ids, any order.
 * out:     records / side (arena_cap entries each: the whole arena, 0xff bytes where no kernel wrote), rt ((N + 1) x S, rows S apart; 0xff bytes likewise),
 *          best_pos (S; 0x7f bytes where no kernel wrote, -1 being the writer's "no kept match"): what the writer left; side, rt and best_pos may be NULL with writer 1, which writes none of them.
 *          sel->kept_base, n_kept, R, overflow, n_want: the result record (device and host-mapped copy are compared by the hook; writer 1: n_kept
 *          is the scan's total, the rest 0).  Per job qt (n words) and rt ((N + 1) x S); sel->rebuild_err = the launch's error count (records whose
 *          camera is no neighbour + descents of the (segment, camera) order), sel->rebuild_blocks = workgroups per job of the pass over the records.
 * Refused with L3D_ERR_INVALID before anything is launched: N outside [1, 255], row_start not ascending from 0, a candidate whose camera is not its
 * row's or whose target id does not fit 16 bits, kept_cnt that is not the count of confidences above 1, writer 1 with arena_cap below the total. */
typedef struct l3d_test_kept_job {
    const l3d_match* records;
    const uint32_t* local2global;
    uint32_t* qt;                   /* out */
    int32_t* rt;                    /* out */
    int32_t n, S, N, pad;
} l3d_test_kept_job;
typedef struct l3d_test_kept_path {
    int32_t writer, has_prev;
    uint64_t prev_base;
    int32_t prev_n_kept, cand_cap;
    uint64_t arena_cap;
    l3d_test_kept_job* jobs;
    int32_t n_jobs;
    int32_t n_kept, R, overflow, n_want, rebuild_err, rebuild_blocks, pad;      /* out */
    uint64_t kept_base;                                                          /* out */
} l3d_test_kept_path;
int l3d_test_kept_write(l3d_ctx* ctx, int S, int N, const int32_t* row_start, const uint32_t* cand_meta, const float* cand_depths, const float* cand_conf,
                        const int32_t* kept_cnt, const uint32_t* local2global, l3d_test_kept_path* sel, l3d_match* records, uint32_t* side, int32_t* rt,
                        int32_t* best_pos);

/* The affinity fill's core (affinity_fill_core of l3d_affinity.hip, the code l3d_affinity_fill, l3d_affinity_fill_resident and every rank of
 * l3d_affinity_fill_sharded run) on host tables handed in as for l3d_affinity_fill, as ONE PART of a fill sharded by source key, exported for tests
 * (tests/test_gpu_affinity_paths.py).  No collective runs, nothing is numbered: what comes back is what a rank holds before the exchanges.
 * part in:  h0, h1: the sources (hypotheses) [h0, h1) whose candidates are enumerated; pos_base: where the part's candidates stand in the whole
 *           enumeration (the sharded fill passes rank << 44); loc2glob (n_hyp, or NULL: the numbers stay local): the global number of every local
 *           hypothesis, applied to the passed pairs; assume_symmetric != 0: every potential correspondence is taken to be recorded both ways
 *           (k_aff_sym looks nothing up).
 * out:      flags (entries of pot_tgt; may be NULL): one byte per potential correspondence as the last k_aff_groups launch left it -- bit 0 marked
 *           as a target, bit 1 expanded, bit 2 m-used; needs_prev (n_views; may be NULL); part->n_launches: launches of k_aff_groups;
 *           part->coll_sym: 1 = the collinearity table was found symmetric and the short-list path taken; part->n_candidates / n_passed: the part's
 *           candidates and those that passed their threshold; pairs (2 x n_passed hypothesis numbers) / weights (n_passed): callee-allocated,
 *           l3d_free; first (n_hyp; may be NULL): 2 * (pos_base + position among the part's candidates) + side as a minimum per LOCAL hypothesis,
 *           ~0 = never touched.
 * The table checks and their messages are those of l3d_affinity_fill; h0 > h1 or a range outside [0, n_hyp]: L3D_ERR_INVALID.  n_hyp == 0: L3D_OK,
 * everything empty. */
typedef struct l3d_test_affinity_part {
    int32_t h0, h1;
    uint64_t pos_base;
    const int32_t* loc2glob;
    int32_t assume_symmetric;
    int32_t n_launches, coll_sym, pad;                  /* out */
    int64_t n_candidates, n_passed;                     /* out */
} l3d_test_affinity_part;
int l3d_test_affinity_fill(l3d_ctx* ctx, const l3d_affinity_input* in, l3d_test_affinity_part* part, unsigned char* flags, int32_t* needs_prev,
                           int32_t** pairs, float** weights, uint64_t* first);

/* The slot kernels of the segment-sharded chain (l3d_chain_sharded.hip) on slots the caller hands in, exported for tests
 * (tests/test_gpu_shard_slots.py).  No chain is opened and no collective runs: each hook launches the product's own kernels under the product's own
 * grid rules, after everything a kernel uses as an index or a count has been checked on the host (L3D_ERR_INVALID before anything is launched).
 *   geom   the six inputs of the slot's geometry (l3d_test_shard_plan: largest S_src <= 16384, largest N in [1, 255], world in [1, 64], slot_records
 *          in [1, 2^20], option slot_cams_min, n_views <= 4096) and `ring`, the view blocks of the gathered buffer (0: n_views, as the geometry sets it;
 *          a ring-mode run sets fewer).  View j's slots lie in block j % ring, rank r's at (block * world + r) * slot_bytes. */
typedef struct l3d_test_shard_geom {
    int32_t maxS, maxN, world, slot_records, slot_cams_min, n_views, ring, pad;
} l3d_test_shard_geom;

/* k_slot_write for ONE view's verified candidates and ONE rank's range [s0, s1) of its segments.
 *   S, N, row_start, cand_meta, cand_depths, cand_conf, kept_cnt, local2global: as l3d_test_kept_write takes them (the whole view); best S x 2: the
 *   depth pair of every segment's best hypothesis; cand_cap: what the kernel guards against row_start[S*N].
 * out: slot, the slot_bytes of the geometry: 0xff bytes where the kernel did not write, 0x7f bytes in the best positions (-1 is an answer).  The hook
 *   keeps 256 guard bytes behind the slot on the device and reports a write into them as L3D_ERR_INVALID.
 * Refused before launch: N outside [1, 255], row_start not ascending from 0, a candidate whose camera is not its row's or whose target does not fit
 * 16 bits, kept_cnt that is not the count of confidences above 1, a range outside [0, S] or longer than seg_cap - 1, N > maxN, S > maxS. */
int l3d_test_shard_slot_write(l3d_ctx* ctx, int S, int N, const int32_t* row_start, const uint32_t* cand_meta, const float* cand_depths, const float* cand_conf,
                              const int32_t* kept_cnt, const uint32_t* local2global, const float* best, int s0, int s1, const l3d_test_shard_geom* geom,
                              int cand_cap, unsigned char* slot);

/* The collect step of the sharded chain for view k and one rank's range [s0, s1): k_exist_count_slots, the range scan, k_place_slots and (sort_apart)
 * the launch that orders the runs, over a gathered buffer of the caller's (ring x world x slot_bytes).
 *   views, n_views, k; rowA, metaA, depthsA, n_A, rowcnt: as l3d_test_collect_candidates reads them (every view's S_src <= maxS and N <= maxN)
 * sel in:  s0, s1; cand_cap: the candidate capacity the kernels guard, also the entries of cand_meta / cand_depths (it must hold the range's
 *          candidates: this hook does not run the overflow path); sort_apart; slot_scan_grain: option slot_scan_grain for the call.
 * out:     row_start S*N + 1, cursor S*N, seg_order S, cand_meta cand_cap x 2, cand_depths cand_cap x 4 (0xff bytes where no kernel wrote: the rows
 *          outside the range are not the rank's); sel->wps (workgroups per (source, rank) list), blocks_move, R (row_start[S*N]: the range's total).
 * Refused before launch, beside what l3d_test_collect_candidates refuses: a source whose ring block a later view in front of k has overwritten
 * (source_index + ring < k); and, in every slot of a source that lists view k as a neighbour: n_kept outside [0, slot_records] (unless the header
 * carries an overflow bit), a header range that is not 0 <= s0 <= s1 <= 65536 with s1 - s0 <= seg_cap - 1; in a slot that holds records: a record
 * whose segment is outside the header's range, whose camera is no neighbour of its view or whose target does not fit 16 bits, records out of (segment,
 * local camera) order, a side word that is not (local camera << 16 | target) of its record, a run-table entry (rows 0..N, columns 0..s1 - s0) that is
 * not the position of the first record at or behind (segment, camera).  The body of an overflowed or empty slot is not looked at: no kernel may read it. */
typedef struct l3d_test_shard_collect_path {
    int32_t s0, s1, cand_cap, sort_apart, slot_scan_grain;
    int32_t wps, blocks_move, R;                        /* out */
} l3d_test_shard_collect_path;
int l3d_test_shard_collect(l3d_ctx* ctx, const l3d_chain_view* views, int n_views, int k, const unsigned char* gathered, const l3d_test_shard_geom* geom,
                           const int32_t* rowA, const uint32_t* metaA, const float* depthsA, int n_A, const int32_t* rowcnt,
                           l3d_test_shard_collect_path* sel, int32_t* row_start, uint32_t* cand_meta, float* cand_depths, int32_t* cursor, int32_t* seg_order);

/* The consumers of the gathered blocks over ALL views' slots of the caller's (n_views x world x slot_bytes, view j's block at j):
 *   k_shard_totals and k_check_slots over the headers in front of the slots (stride slot_bytes) and over the compact 32-byte table the retire run
 *   leaves; k_pack_view per verified view; k_shard_pack_all once; k_shard_retire in the batches listed, over a ring of geom->ring blocks that the hook
 *   fills as the run's exchanges would: view j's block goes to ring block j % ring (zeros for a view that is not verified) just before the first batch
 *   enqueued at a view behind j.
 * in:  verified (n_views bytes), keep (n_views bytes or NULL), best_off (n_views: where a view's best pairs and positions go, in entries), view_sn
 *      (n_views x (S_src, N)), rt_off (n_views: where its run table starts in rt_all, in ints; read with retire_tables), batches (n_batches x (first,
 *      count, the view the batch is enqueued at -- n_views: the final flush), as l3d_test_shard_retire lists them), retire_tables (the retire kernel
 *      files side words and run tables: the geometry must have them), arena_cap (records the retire kernel guards), pack_cap (records of the pack-all
 *      arena: must hold the verified views), best_cap (entries of the best arrays), rt_cap (ints of rt_all).
 * out: stage (n_views x stage_bytes) and pack_hdr (n_views x 32 B) of k_pack_view; totals (2 x n_views x 2: stride slot_bytes, then 32) and check
 *      (2 x 3 likewise); pa_* from k_shard_pack_all and rt_* from k_shard_retire: arena (pack_cap / arena_cap records), best (best_cap x 2), bestpos
 *      (best_cap); base_dev (n_views + 2; zeros where not written, as the run starts them), hdr_all (n_views x world x 32 B), overflow (1 int), qt_arena
 *      (arena_cap), rt_all (rt_cap).  0xff bytes where no kernel wrote, 0x7f in the best positions.
 * Refused before launch: flags that are not 0 or 1; a view whose (S, N) exceeds the geometry or whose best pairs or run table end past their
 * capacity; in a verified view's slot a header with R < 0, overflow outside [0, 7], a range that is not 0 <= s0 <= s1 <= S with s1 - s0 <= seg_cap -
 * 1, or (no overflow bit) n_kept outside [0, slot_records]; verified views that keep more than pack_cap; batches that are not contiguous and ascending
 * from view 0, that retire a view not yet exchanged (first + count > at), or that read a ring block already overwritten (first + ring < at). */
typedef struct l3d_test_shard_pack_io {
    const unsigned char* verified;
    const unsigned char* keep;
    const int64_t* best_off;
    const int32_t* view_sn;
    const int64_t* rt_off;
    const int32_t* batches;
    int32_t n_batches, retire_tables;
    int64_t arena_cap, pack_cap, best_cap, rt_cap;
    unsigned char* stage;                               /* out, from here on */
    unsigned char* pack_hdr;
    int32_t* totals;
    int32_t* check;
    l3d_match* pa_arena;
    float* pa_best;
    int32_t* pa_bestpos;
    l3d_match* rt_arena;
    float* rt_best;
    int32_t* rt_bestpos;
    int64_t* base_dev;
    unsigned char* hdr_all;
    int32_t* overflow;
    uint32_t* qt_arena;
    int32_t* rt_all;
} l3d_test_shard_pack_io;
int l3d_test_shard_pack(l3d_ctx* ctx, const unsigned char* gathered, const l3d_test_shard_geom* geom, l3d_test_shard_pack_io* io);

#ifdef __cplusplus
}
#endif
#endif /* LINE3D_AMD_H */
