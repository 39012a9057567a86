// line3d_host.cpp -- the pipeline facade of the C ABI (include/line3d_amd.h: l3d_line3d_*): the reference's operator interface
// (addImage / addImage_fixed_sim / compute3Dmodel / getResult, line3D.h) over the host pipeline in line3d_host_views.cpp (views, seam path),
// line3d_host_chain.cpp (resident matchViews) and line3d_host_finish.cpp (selection, affinity, diffusion, clustering, fit).
#include "line3d_host_internal.hpp"
#include "l3d_detect.hpp"
#include "l3d_node.hpp"
#include "l3d_turns.hpp"
#include "l3d_shard_rule.hpp"

#include <hip/hip_runtime_api.h>

// ---- a node object: one ordinary object per rank, each on a host thread of its own while it computes ---------------------------------------
namespace l3dh {
struct NodeRanks {
    std::vector<int> devices;
    std::vector<L*> ranks;                  // rank r: an ordinary object with its own context on devices[r]
    l3d_node_comm* comm = nullptr;          // their all-gather (l3d_node.hip), every stream bound
    int mode = 0;                           // l3d_line3d_set_node_mode
    int threads_per_rank = 1;               // the host-thread budget split among the ranks
    std::vector<int64_t> turn_records;      // mode 2: the records every rank retired in its turn (l3d_line3d_node_turn_records)
    // mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover; l3d_turns.hpp)
    bool handover = false;
    std::vector<int64_t> turn_views;        // the chain views every rank computed over its visits, and its visits (l3d_line3d_node_turn_views)
    std::vector<int> turn_visits;
    std::vector<l3d::TurnHandover> packages;    // packages[r]: the tail turn r left for turn r + 1 -- owned here, not by a rank's context
    l3d::TurnStore store;                   // the early-return slices and alias packages of every block
};

// Mode 2 of a node object: the ranks of one device take their turns in rank order, one token per device (host condition: no device-side flag, no
// spinning).  Turn 0 runs before every other turn -- the sizes of the later ones come from it.  The same token then guards the candidate
// enumeration of the collective fill.  A rank that fails gives the token back and wakes everybody: nobody waits for a turn that will not come.
struct TurnGate {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int> devices;
    std::vector<char> done;                 // per rank: its turn is over
    std::vector<int> holder;                // per rank's device (indexed by rank, the first rank of the device keeps the word): the rank holding the token, -1: free
    bool aborted = false;
    int failed_rank = -1, failed_rc = L3D_OK;
    std::string failed_msg;
    // what the turns leave for the node layer
    std::vector<std::vector<unsigned char>> keep;      // per rank: the views it holds (l3d_partition_keep_views of its block)
    std::vector<std::vector<uint64_t>> hash;           // per rank: k_block_digest of every view it held
    std::vector<std::vector<int32_t>> n_kept;
    std::vector<size_t> arena_records;                 // per rank: its exact arena, known after turn 0
    int slot_records = 0; size_t cand_cap = 0;         // what turn 0 ended with

    explicit TurnGate(const std::vector<int>& dev) : devices(dev), done(dev.size(), 0), holder(dev.size(), -1), keep(dev.size()), hash(dev.size()), n_kept(dev.size()), arena_records(dev.size(), 0) {}
    int word(int r) const { for (int q = 0; q < r; ++q) if (devices[(size_t)q] == devices[(size_t)r]) return q; return r; }
    bool all_done() const { for (char d : done) if (!d) return false; return true; }
    // false: a rank failed, no turn starts any more
    bool begin_turn(int r)
    {
        std::unique_lock<std::mutex> lk(mu);
        const int w = word(r);
        cv.wait(lk, [&] {
            if (aborted) return true;
            if (r > 0 && !done[0]) return false;
            for (int q = 0; q < r; ++q) if (devices[(size_t)q] == devices[(size_t)r] && !done[(size_t)q]) return false;
            return holder[(size_t)w] < 0;
        });
        if (aborted) return false;
        holder[(size_t)w] = r;
        return true;
    }
    void fail_locked(int r, int rc, const std::string& msg)
    {
        if (failed_rank < 0) { failed_rank = r; failed_rc = rc; failed_msg = msg; }
        aborted = true;
    }
    // the views two ranks both held must have come out of their chains alike: the digests of the last rank to finish close the turns
    void compare_locked(const std::vector<uint32_t>& view_ids)
    {
        const int W = (int)devices.size();
        for (int a = 0; a < W; ++a)
            for (int b = a + 1; b < W; ++b) {
                const size_t n = std::min(keep[(size_t)a].size(), keep[(size_t)b].size());
                for (size_t k = 0; k < n; ++k) {
                    if (!keep[(size_t)a][k] || !keep[(size_t)b][k]) continue;
                    if (hash[(size_t)a][k] == hash[(size_t)b][k] && n_kept[(size_t)a][k] == n_kept[(size_t)b][k]) continue;
                    fail_locked(a, L3D_ERR_INVALID, "the kept list of view " + std::to_string(k < view_ids.size() ? view_ids[k] : (uint32_t)k) + " (chain index " + std::to_string(k) + ") differs between the turns of rank " +
                                                     std::to_string(a) + " (" + std::to_string(n_kept[(size_t)a][k]) + " records) and rank " + std::to_string(b) + " (" + std::to_string(n_kept[(size_t)b][k]) + " records)");
                    return;
                }
            }
    }
    void end_turn(int r, int rc, const std::string& msg, const std::vector<uint32_t>& view_ids)
    {
        std::lock_guard<std::mutex> lk(mu);
        const int w = word(r);
        if (holder[(size_t)w] == r) holder[(size_t)w] = -1;
        done[(size_t)r] = 1;
        if (rc) fail_locked(r, rc, msg);
        else if (!aborted && all_done()) compare_locked(view_ids);
        cv.notify_all();
    }
    // every turn is over (true) or a rank failed (false)
    bool wait_all()
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return aborted || all_done(); });
        return !aborted;
    }
    void abort()
    {
        std::lock_guard<std::mutex> lk(mu);
        aborted = true;
        cv.notify_all();
    }
    // the token of rank r's device around its candidate enumeration (l3d_affinity_fill_sharded); after a failure nobody is kept waiting
    void fill_token(int r, bool acquire)
    {
        std::unique_lock<std::mutex> lk(mu);
        const int w = word(r);
        if (acquire) {
            cv.wait(lk, [&] { return aborted || holder[(size_t)w] < 0; });
            if (holder[(size_t)w] < 0) holder[(size_t)w] = r;
        } else {
            if (holder[(size_t)w] == r) holder[(size_t)w] = -1;
            cv.notify_all();
        }
    }
};
struct FillGateUser { TurnGate* gate; int rank; };
static void fill_gate_fn(void* user, int acquire)
{
    FillGateUser* u = static_cast<FillGateUser*>(user);
    u->gate->fill_token(u->rank, acquire != 0);
}
}  // namespace l3dh

static std::string rank_prefix(const L* h, int r)
{
    return "rank " + std::to_string(r) + " (device " + std::to_string(h->node->devices[(size_t)r]) + "): ";
}
// the calls that address one rank's machinery: refused on a node object rather than acting on rank 0
static int node_refuse(L* h, const char* what)
{
    return h->fail(L3D_ERR_INVALID, std::string(what) + ": addresses one rank's machinery -- not on a node object (l3d_line3d_create_node), whose "
                                                        "compute3Dmodel runs every rank");
}
static L* rank0(const L* h) { return h->node->ranks[0]; }
// fn(rank object) on every rank in turn (the images, reset); stops at the first failure
template <class F>
static int node_each(L* h, F fn)
{
    for (size_t r = 0; r < h->node->ranks.size(); ++r)
        if (const int rc = fn(h->node->ranks[r])) return h->fail(rc, rank_prefix(h, (int)r) + h->node->ranks[r]->err);
    return L3D_OK;
}
// fn(r) on one host thread per rank, all at once: its device current, its share of the host threads.  A rank that returns an error breaks the
// communicator (its peers' pending and later exchanges fail instead of waiting).  The message of the rank that failed first.
static int node_run(L* h, const std::function<int(int)>& fn)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    std::vector<int> rcs((size_t)W, L3D_OK);
    std::atomic<int> first{ -1 };
    std::vector<std::thread> th;
    for (int r = 0; r < W; ++r)
        th.emplace_back([&, r]() {
            int rc = hipSetDevice(N.devices[(size_t)r]) == hipSuccess ? L3D_OK : L3D_ERR_HIP;
            if (rc) N.ranks[(size_t)r]->fail(rc, "hipSetDevice failed on the rank's thread");
            l3d::thread_host_threads() = N.threads_per_rank;
            if (!rc) rc = fn(r);
            l3d::thread_host_threads() = 0;
            if (rc) {
                int none = -1;
                first.compare_exchange_strong(none, r);
                l3d_node_comm_abort(N.comm);
            }
            rcs[(size_t)r] = rc;
        });
    for (auto& t : th) t.join();
    // the rank whose exchange broke the communicator, else the first to return an error
    int r = l3d::node_comm_culprit(N.comm);
    if (r < 0 || rcs[(size_t)r] == L3D_OK) r = first.load();
    return r < 0 ? L3D_OK : h->fail(rcs[(size_t)r], rank_prefix(h, r) + N.ranks[(size_t)r]->err);
}
// l3d_line3d_set_covisibility 1 on a node object: rank 0 holds the lists and counts them once, on its device, before the ranks prepare; every
// other rank is handed the two tables
static int node_count_covisibility(L* h)
{
    L* R0 = rank0(h);
    if (R0->covis_mode != 1 || !R0->covis_dirty) return L3D_OK;
    if (const int rc = count_covisibility(R0)) return h->fail(rc, rank_prefix(h, 0) + R0->err);
    for (size_t r = 1; r < h->node->ranks.size(); ++r) {
        L* R = h->node->ranks[r];
        R->num_wps = R0->num_wps; R->common_wps = R0->common_wps;
        R->covis_path = R0->covis_path; R->covis_dirty = false;
    }
    return L3D_OK;
}

// the per-view summary of the one chain: a rank's own lists only cover the views it holds -- view k from the rank whose block holds it
// (every mode cuts the chain's views into blocks n * r / W)
static void node_merge_summary(L* h)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    const size_t n = rank0(h)->chain_summary.size();
    h->chain_summary.assign(n, l3d_chain_summary());
    for (int r = 0; r < W; ++r) {
        const std::vector<l3d_chain_summary>& own = N.ranks[(size_t)r]->chain_summary;
        const size_t b0 = (size_t)(((long long)n * r) / W), b1 = (size_t)(((long long)n * (r + 1)) / W);
        for (size_t k = b0; k < b1 && k < own.size(); ++k) h->chain_summary[k] = own[k];
    }
}

// one rank's turn (mode 2): its share of the W-rank job computed ALONE on its device -- the whole chain at world 1 with the keep set of block r,
// the rows of its share of the products, the hypotheses (the last reader of the kept records), the digests of what it held; then the records go
static int node_turn(L* h, TurnGate& G, int r, int slot_records_1)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    L* R = N.ranks[(size_t)r];
    int rc = l3d_set_option(R->ctx, "L3D_PART_VRANK", r);
    if (!rc) rc = l3d_set_option(R->ctx, "L3D_PART_VWORLD", W);
    if (rc) return R->fail(rc, l3d_last_error(R->ctx));
    l3d::ctx_turn_share(R->ctx, 1);
    R->shard_arena_cap_hint = 0;
    if (r > 0) {        // (only turn 0 may pay a capacity re-run: the later turns start with what it ended with and with their exact arena)
        R->shard_world_seen = 1; R->shard_slot_records_seen = G.slot_records; R->shard_cand_cap_seen = G.cand_cap;
        R->shard_arena_cap_hint = G.arena_records[(size_t)r];
    }
    rc = l3d_line3d_shard_run(R, 0, 1, slot_records_1, l3d_exchange_local, nullptr, 3, nullptr, nullptr);
    R->shard_arena_cap_hint = 0;
    if (rc) return rc;
    ChainPlan* P = get_plan(R);
    if (!P) return R->fail(L3D_ERR_INVALID, "turn: no static schedule");
    const int n = (int)P->n;
    if (r == 0) {
        // every view's slot header went through turn 0's chain: every later turn's arena is known exactly
        const std::vector<int>& kept = l3d::ctx_shard_view_kept(R->ctx);
        if ((int)kept.size() != n) return R->fail(L3D_ERR_INVALID, "turn 0: the chain left no kept count per view");
        std::lock_guard<std::mutex> lk(G.mu);
        for (int q = 0; q < W; ++q) {
            G.keep[(size_t)q].assign((size_t)n, 0);
            if (const int rk = l3d_partition_keep_views(P->cv.data(), n, (int)(((long long)n * q) / W), (int)(((long long)n * (q + 1)) / W), G.keep[(size_t)q].data(), nullptr))
                return R->fail(rk, "turn 0: l3d_partition_keep_views refused the schedule");
            size_t recs = 0;
            for (int k = 0; k < n; ++k) if (G.keep[(size_t)q][(size_t)k]) recs += (size_t)kept[(size_t)k];
            G.arena_records[(size_t)q] = recs + 4096;
        }
        G.slot_records = std::max(slot_records_1, R->shard_slot_records_seen);
        G.cand_cap = R->shard_cand_cap_seen;
    }
    rc = greedy_selection_resident(R);                      // (l3d_products_hypotheses: nothing behind it reads the kept arena)
    if (rc) return rc;
    R->hyps_done = true;
    std::vector<uint64_t> hash((size_t)n, 0);
    std::vector<int32_t> nk((size_t)n, 0);
    rc = l3d_chain_records_digest(R->ctx, hash.data(), nk.data(), n);
    if (!rc) rc = l3d_chain_release_records(R->ctx);
    if (rc) return R->fail(rc, std::string("turn: ") + l3d_last_error(R->ctx));
    // what the turn retired: the records its arena really holds (the digests' lengths are the products' result records, which add up to the arena's fill:
    // l3d_shard_chain_products checks that) -- of ANY view, so a chain that kept more than its keep set shows -- plus, as the chain's summary counts them,
    // the lists of the early-return views it held (rebuilt from their sources' records, cudawrapper.cu:877-878: no room of their own in the arena)
    int64_t recs = 0;
    std::lock_guard<std::mutex> lk(G.mu);
    for (int k = 0; k < n; ++k) {
        recs += nk[(size_t)k];
        if (G.keep[(size_t)r][(size_t)k] && P->n_tbm[(size_t)k] == 0 && k < (int)R->chain_summary.size()) recs += R->chain_summary[(size_t)k].n_kept;
    }
    G.hash[(size_t)r] = std::move(hash); G.n_kept[(size_t)r] = std::move(nk);
    N.turn_records[(size_t)r] = recs;
    return L3D_OK;
}

// every rank prepares the scene without reserving the finishing stages' arenas from its size (a job sized by memory)
static int node_prepare_turns(L* h)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    std::vector<int> hint((size_t)W, 1);
    for (int r = 0; r < W; ++r) {
        (void)l3d_get_option(N.ranks[(size_t)r]->ctx, "L3D_RESERVE_HINT", &hint[(size_t)r]);
        if (const int rc = l3d_set_option(N.ranks[(size_t)r]->ctx, "L3D_RESERVE_HINT", 0)) return h->fail(rc, l3d_last_error(N.ranks[(size_t)r]->ctx));
    }
    int rc = node_count_covisibility(h);
    if (!rc) rc = node_run(h, [&](int r) { return prepare(N.ranks[(size_t)r]); });
    for (int r = 0; r < W; ++r) (void)l3d_set_option(N.ranks[(size_t)r]->ctx, "L3D_RESERVE_HINT", hint[(size_t)r]);      // (read by prepare alone: the other modes keep theirs)
    return rc;
}
// compute3Dmodel with the ranks of a device taking turns (l3d_line3d_set_node_mode 2): a scene whose kept records do not fit one device's memory at once.
// Every turn computes the WHOLE chain and keeps one block's share of it, so matchViews costs about W single passes; the collective finish is the
// one of the other modes, every share standing for its rank.
// prepared: the ranks have prepared the scene already (the hand-over variant falling back to this one)
static int node_compute_turns(L* h, int perform_diffusion, bool prepared = false)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    if (rank0(h)->views.size() < 4) return h->fail(L3D_ERR_INVALID, "not enough images! can't compute 3D model...");   // line3D.cc:347-351
    N.turn_views.clear(); N.turn_visits.clear();
    int rc = prepared ? L3D_OK : node_prepare_turns(h);
    if (rc) return rc;
    int s_max = 0;
    for (const View* v : rank0(h)->vlist) s_max = std::max(s_max, v->S());
    // kept records of one view's slot at world 1 (node_compute's first guess with one rank): grown by turn 0's capacity verdicts, then handed on
    const int slot_records_1 = (int)std::min<long long>(INT32_MAX / 2, std::max<long long>(1024, 10LL * s_max * rank0(h)->matching_neighbors + 1024));
    l3d::node_comm_rearm(N.comm);
    h->chain_summary.clear();
    N.turn_records.assign((size_t)W, 0);
    TurnGate G(N.devices);
    std::vector<FillGateUser> gate_user((size_t)W);
    std::vector<uint32_t> order_ids;
    rc = node_run(h, [&](int r) {
        L* R = N.ranks[(size_t)r];
        int rc2 = L3D_OK;
        if (!G.begin_turn(r)) rc2 = R->fail(L3D_ERR_INVALID, "another rank failed in its turn");
        else {
            rc2 = node_turn(h, G, r, slot_records_1);
            if (r == 0 && rc2 == L3D_OK) order_ids = R->order;          // (read by the last rank to finish, under the gate's lock)
            G.end_turn(r, rc2, R->err, order_ids);
        }
        // no rank enters the first collective before every turn is over: a rank waiting in an exchange gives up after its time limit, a turn may take longer
        if (rc2 == L3D_OK && !G.wait_all()) rc2 = R->fail(L3D_ERR_INVALID, "another rank failed in its turn");
        if (rc2 == L3D_OK) {
            gate_user[(size_t)r] = { &G, r };
            l3d::ctx_fill_gate(R->ctx, fill_gate_fn, &gate_user[(size_t)r]);
            l3d::ctx_fill_collective_only(R->ctx, r != 0);
            rc2 = l3d_line3d_finish_sharded(R, perform_diffusion, l3d_exchange_node, N.comm);
            if (rc2) G.abort();
        }
        // the context is an ordinary rank's again; what a rank other than 0 still holds is nobody's result
        l3d::ctx_fill_gate(R->ctx, nullptr, nullptr);
        l3d::ctx_fill_collective_only(R->ctx, 0);
        l3d::ctx_turn_share(R->ctx, 0);
        (void)l3d_set_option(R->ctx, "L3D_PART_VWORLD", 0);
        (void)l3d_set_option(R->ctx, "L3D_PART_VRANK", 0);
        R->hyps_done = false;
        if (r != 0) l3d::ctx_release_share(R->ctx);
        return rc2;
    });
    if (rc) {
        // (the rank that failed in its turn, or the pair of ranks whose digests differ -- not a rank that merely heard of it)
        if (G.failed_rank >= 0) return h->fail(G.failed_rc, rank_prefix(h, G.failed_rank) + G.failed_msg);
        return rc;
    }
    node_merge_summary(h);
    N.turn_views.assign((size_t)W, (int64_t)h->chain_summary.size());       // (every turn computed the whole chain, once)
    N.turn_visits.assign((size_t)W, 1);
    return L3D_OK;
}

// ---- mode 2 with a warm hand-over between the turns (l3d_line3d_set_turn_handover) ------------------------------------------------------------
static void node_drop_handover(NodeRanks& N)
{
    for (l3d::TurnHandover& p : N.packages) l3d::turn_handover_release(&p);
    N.packages.clear();
    l3d::turn_store_release(&N.store);
}
// one visit of rank r: its piece of the chain warm from packages[r - 1], the tail for rank r + 1 (first visit), its pieces of the store, and -- share -- its
// share of the products, the hypotheses (the last reader of the kept records); then the records go
static int node_turn_visit(L* h, int r, bool first, bool share, l3d::TurnReport& rep)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    L* R = N.ranks[(size_t)r];
    const double t0 = now_s();
    match_begin(R);
    ChainPlan* P = get_plan(R);
    if (!P) return R->fail(L3D_ERR_INVALID, "turn: no static schedule");
    std::vector<uint32_t> ids; std::vector<int32_t> base;
    dense_map(R, ids, base);
    l3d_dense_map map;
    map.n_views = (int32_t)ids.size(); map.view_ids = ids.data(); map.seg_base = base.data();
    R->chain_summary.assign(P->n, l3d_chain_summary());
    R->resident_products = false;
    const double t1 = now_s();
    int rc = l3d::match_chain_turn(R->ctx, P->cv.data(), (int)P->n, &map, R->chain_summary.data(), r, W, 0, r > 0 ? &N.packages[(size_t)r - 1] : nullptr,
                                   first ? &N.packages[(size_t)r] : nullptr, &N.store, share, &rep);
    R->t_gpu_call += now_s() - t1;
    if (rc) return R->fail(rc, std::string("match_chain_turn: ") + l3d_last_error(R->ctx));
    if (share) {
        R->resident_n_pot = rep.n_pot;
        R->partitioned = true; R->part_exchange = l3d_exchange_node; R->part_user = N.comm;
        rc = adopt_resident_products(R, *P);
        if (rc) { R->partitioned = false; return rc; }
        double st[4];
        l3d_last_stats(R->ctx, st);
        R->stat_pairs += st[0]; R->stat_raw += st[1];
        R->t_match = now_s() - t0;
        rc = greedy_selection_resident(R);                  // (l3d_products_hypotheses: nothing behind it reads the kept arena)
        if (rc) return rc;
        R->hyps_done = true;
    }
    rc = l3d_chain_release_records(R->ctx);
    if (rc) return R->fail(rc, std::string("turn: ") + l3d_last_error(R->ctx));
    return L3D_OK;
}
// a visit's report filed with the gate (the cross-check of the views two turns both held) and the node object's counters
static void node_file_visit(L* h, TurnGate& G, int r, const l3d::TurnReport& rep, bool share)
{
    NodeRanks& N = *h->node;
    L* R = N.ranks[(size_t)r];
    ChainPlan* P = get_plan(R);
    std::lock_guard<std::mutex> lk(G.mu);
    N.turn_views[(size_t)r] += rep.views_computed;
    N.turn_visits[(size_t)r] += 1;
    G.keep[(size_t)r] = rep.held; G.hash[(size_t)r] = rep.hash; G.n_kept[(size_t)r] = rep.n_kept;
    if (share) {
        // the records its arena held when the share was built, plus -- as the chain's summary counts them -- the lists of the early-return views it held
        int64_t recs = rep.arena_records;
        for (size_t k = 0; P && k < P->n && k < rep.held.size() && k < R->chain_summary.size(); ++k)
            if (rep.held[k] && P->n_tbm[k] == 0) recs += R->chain_summary[k].n_kept;
        N.turn_records[(size_t)r] = recs;
    }
}
// compute3Dmodel in turns, every turn computing its own piece of the chain: about one pass of matchViews plus the deferred turns' pieces instead of W passes
static int node_compute_turns_handover(L* h, int perform_diffusion)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    if (rank0(h)->views.size() < 4) return h->fail(L3D_ERR_INVALID, "not enough images! can't compute 3D model...");   // line3D.cc:347-351
    N.turn_views.clear(); N.turn_visits.clear();
    int rc = node_prepare_turns(h);
    if (rc) return rc;
    // the schedule is static: which turns are deferred, and whether the partition can take the scene at all, is known before the first turn
    l3d::TurnSchedule S;
    const char* why = nullptr;
    for (int r = 1; r < W; ++r) if (N.devices[(size_t)r] != N.devices[0]) why = "the ranks do not share one device";
    if (!why) {
        match_begin(rank0(h));
        ChainPlan* P = get_plan(rank0(h));
        if (!P || P->n == 0) why = "the schedule is not static";
        else if (l3d::turn_handover_schedule(P->cv.data(), (int)P->n, W, 0, &S) || !S.supported) why = "the blocks-of-views partition cannot take its early-return views";
    }
    if (why) {
        if (h->verbose) printf("[L3D] node: no hand-over between the turns on this scene (%s) -- every turn computes the whole chain (plain mode 2)\n", why);
        return node_compute_turns(h, perform_diffusion, true);
    }
    l3d::node_comm_rearm(N.comm);
    h->chain_summary.clear();
    N.turn_records.assign((size_t)W, 0);
    N.turn_views.assign((size_t)W, 0); N.turn_visits.assign((size_t)W, 0);
    node_drop_handover(N);
    N.packages.assign((size_t)W, l3d::TurnHandover());
    TurnGate G(N.devices);
    std::vector<FillGateUser> gate_user((size_t)W);
    std::vector<uint32_t> order_ids;
    std::vector<std::vector<uint64_t>> first_hash((size_t)W);
    std::vector<std::vector<int32_t>> first_kept((size_t)W);
    rc = node_run(h, [&](int r) {
        L* R = N.ranks[(size_t)r];
        int rc2 = L3D_OK;
        if (!G.begin_turn(r)) rc2 = R->fail(L3D_ERR_INVALID, "another rank failed in its turn");
        else {
            const bool deferred = S.turns[(size_t)r].deferred != 0;
            l3d::TurnReport rep;
            rc2 = node_turn_visit(h, r, true, !deferred, rep);
            if (rc2 == L3D_OK) {
                node_file_visit(h, G, r, rep, !deferred);
                first_hash[(size_t)r] = rep.hash; first_kept[(size_t)r] = rep.n_kept;
                // the package this turn started from is kept only for a second visit
                if (r > 0 && !deferred) l3d::turn_handover_release(&N.packages[(size_t)r - 1]);
            }
            if (r == 0 && rc2 == L3D_OK) order_ids = R->order;          // (read by the last rank to finish, under the gate's lock)
            // the second visits: under the same token, after the last first visit, before any rank enters a collective -- on this thread, the deferred
            // ranks' own threads wait for the turns to end
            for (int q = 0; q < W && r == W - 1 && rc2 == L3D_OK; ++q) {
                if (!S.turns[(size_t)q].deferred) continue;
                L* Q = N.ranks[(size_t)q];
                l3d::TurnReport again;
                int rcq = node_turn_visit(h, q, false, true, again);
                if (rcq == L3D_OK && (again.hash != first_hash[(size_t)q] || again.n_kept != first_kept[(size_t)q]))
                    rcq = Q->fail(L3D_ERR_INVALID, "the second visit of rank " + std::to_string(q) + " did not reproduce the kept lists of its first visit");
                if (rcq == L3D_OK) { node_file_visit(h, G, q, again, true); if (q > 0) l3d::turn_handover_release(&N.packages[(size_t)q - 1]); }
                else {
                    { std::lock_guard<std::mutex> lk(G.mu); G.fail_locked(q, rcq, Q->err); }
                    rc2 = R->fail(rcq, "the second visit of rank " + std::to_string(q) + " failed: " + Q->err);
                }
            }
            G.end_turn(r, rc2, R->err, order_ids);
        }
        // no rank enters the first collective before every turn is over
        if (rc2 == L3D_OK && !G.wait_all()) rc2 = R->fail(L3D_ERR_INVALID, "another rank failed in its turn");
        if (rc2 == L3D_OK) {
            long long n_pot_all = 0;            // (every share is built: the table's entries over all ranks, which no turn could know)
            for (int q = 0; q < W; ++q) n_pot_all += N.ranks[(size_t)q]->resident_n_pot;
            l3d::ctx_part_total(R->ctx, n_pot_all);
            gate_user[(size_t)r] = { &G, r };
            l3d::ctx_fill_gate(R->ctx, fill_gate_fn, &gate_user[(size_t)r]);
            l3d::ctx_fill_collective_only(R->ctx, r != 0);
            rc2 = l3d_line3d_finish_sharded(R, perform_diffusion, l3d_exchange_node, N.comm);
            if (rc2) G.abort();
        }
        // the context is an ordinary rank's again; what a rank other than 0 still holds is nobody's result
        l3d::ctx_fill_gate(R->ctx, nullptr, nullptr);
        l3d::ctx_fill_collective_only(R->ctx, 0);
        R->hyps_done = false;
        if (r != 0) l3d::ctx_release_share(R->ctx);
        return rc2;
    });
    node_drop_handover(N);
    if (rc) {
        N.turn_records.clear(); N.turn_views.clear(); N.turn_visits.clear();
        if (G.failed_rank >= 0) return h->fail(G.failed_rc, rank_prefix(h, G.failed_rank) + G.failed_msg);
        return rc;
    }
    node_merge_summary(h);
    return L3D_OK;
}

// Line3D::compute3Dmodel over the ranks: prepare on all of them; then matchViews partitioned (set_node_mode) and the collective finish, every
// rank through l3d_exchange_node -- every rank ends with the whole result
static int node_compute(L* h, int perform_diffusion)
{
    NodeRanks& N = *h->node;
    const int W = (int)N.ranks.size();
    if (rank0(h)->views.size() < 4) return h->fail(L3D_ERR_INVALID, "not enough images! can't compute 3D model...");   // line3D.cc:347-351
    if (N.mode == 2) return N.handover ? node_compute_turns_handover(h, perform_diffusion) : node_compute_turns(h, perform_diffusion);
    N.turn_records.clear(); N.turn_views.clear(); N.turn_visits.clear();
    int rc = node_count_covisibility(h);
    if (!rc) rc = node_run(h, [&](int r) { return prepare(N.ranks[(size_t)r]); });
    if (rc) return rc;
    int s_max = 0;
    for (const View* v : rank0(h)->vlist) s_max = std::max(s_max, v->S());
    // kept records one rank may produce for one view (distributed.default_slot_records): l3d_line3d_shard_run grows them on an overflow verdict
    const int slot_records = (int)std::min<long long>(INT32_MAX / 2, std::max<long long>(1024, (10LL * s_max * rank0(h)->matching_neighbors) / W + 1024));
    const int mode = N.mode;
    l3d::node_comm_rearm(N.comm);
    h->chain_summary.clear();
    rc = node_run(h, [&](int r) {
        L* R = N.ranks[(size_t)r];
        int rc2 = L3D_OK;
        bool matched = false;
        if (mode == 1) {
            int verdict = 1;
            rc2 = l3d_line3d_partition_run(R, r, W, -1, l3d_exchange_node, N.comm, &verdict);
            matched = rc2 == L3D_OK && verdict == 0;
            if (rc2 == L3D_OK && verdict != 0 && r == 0 && h->verbose)
                printf("[L3D] node: the blocks of views cannot vouch for one another on this scene -- matchViews runs segment-sharded (mode 0)\n");
        }
        if (rc2 == L3D_OK && !matched) rc2 = l3d_line3d_shard_run(R, r, W, slot_records, l3d_exchange_node, N.comm, 3, nullptr, nullptr);
        if (rc2 == L3D_OK) rc2 = l3d_line3d_finish_sharded(R, perform_diffusion, l3d_exchange_node, N.comm);
        return rc2;
    });
    if (rc) return rc;
    node_merge_summary(h);
    return L3D_OK;
}
static void node_destroy(L* h)
{
    node_drop_handover(*h->node);
    for (L* r : h->node->ranks) l3d_line3d_destroy(r);
    l3d_node_comm_destroy(h->node->comm);
    delete h->node;
    delete h;
}


// =================================================================================================
extern "C" {

int l3d_line3d_create(int device, int matching_neighbors, float unc_upper, float unc_lower, float sigma_p, float sigma_a,
                      float min_baseline, int use_collinearity, int verbose, l3d_line3d** out)
{
    if (!out) return L3D_ERR_INVALID;
    *out = nullptr;
    l3d_ctx* ctx = nullptr;
    int rc = l3d_ctx_create(device, &ctx);
    if (rc) return rc;
    L* h = new L();
    h->ctx = ctx;
    h->verbose = verbose != 0;
    h->matching_neighbors = matching_neighbors;
    h->unc_upper = fabsf(unc_upper);                     // line3D.cc:18-28
    h->unc_lower = fabsf(unc_lower);
    if (h->unc_lower < 1.0f) h->unc_lower = 1.0f;
    if (h->unc_upper <= h->unc_lower) h->unc_upper = h->unc_lower + 1.0f;
    h->sigma_p = sigma_p; h->sigma_a = sigma_a; h->min_baseline = min_baseline;
    h->use_collinearity = use_collinearity != 0;
    h->force_sync = l3d::ctx_options(ctx).match_sync != 0;
    h->warm_thread = std::thread([ctx]() { (void)l3d_warm_up(ctx); });
    h->host_bookkeeping = l3d::ctx_options(ctx).host_bookkeeping != 0;
    *out = h;
    return L3D_OK;
}

int l3d_line3d_create_node(const int* devices, int n, int matching_neighbors, float unc_upper, float unc_lower, float sigma_p, float sigma_a,
                           float min_baseline, int use_collinearity, int verbose, l3d_line3d** out)
{
    if (!out) return L3D_ERR_INVALID;
    *out = nullptr;
    if (!devices || n <= 0) return L3D_ERR_INVALID;
    for (int r = 0; r < n; ++r)
        if (devices[r] < 0) return L3D_ERR_INVALID;
    if (n == 1) return l3d_line3d_create(devices[0], matching_neighbors, unc_upper, unc_lower, sigma_p, sigma_a, min_baseline, use_collinearity, verbose, out);
    l3d_node_comm* comm = nullptr;
    int rc = l3d_node_comm_create(devices, n, &comm);
    if (rc) return rc;
    L* h = new L();
    h->verbose = verbose != 0;
    h->node = new NodeRanks();
    h->node->devices.assign(devices, devices + n);
    h->node->comm = comm;
    for (int r = 0; r < n && rc == L3D_OK; ++r) {
        L* R = nullptr;
        rc = l3d_line3d_create(devices[r], matching_neighbors, unc_upper, unc_lower, sigma_p, sigma_a, min_baseline, use_collinearity, r == 0 ? verbose : 0, &R);
        if (rc == L3D_OK) {
            h->node->ranks.push_back(R);
            R->covis_store = r == 0;
            rc = l3d_node_comm_bind(comm, r, l3d_ctx_stream(R->ctx));
        }
    }
    if (rc) { node_destroy(h); return rc; }
    h->node->threads_per_rank = std::max(1, (int)l3d::host_threads() / n);
    l3d::node_comm_fail_at(comm, 1, hopt(h->node->ranks[1]).node_fail_at);      // (tests)
    *out = h;
    return L3D_OK;
}
int l3d_line3d_num_ranks(const l3d_line3d* h) { return !h ? 0 : h->node ? (int)h->node->ranks.size() : 1; }
int l3d_line3d_set_node_mode(l3d_line3d* h, int mode)
{
    if (!h) return L3D_ERR_INVALID;
    if (mode < 0 || mode > 2) return h->fail(L3D_ERR_INVALID, "set_node_mode: 0 (segments of every view), 1 (blocks of views) or 2 (the ranks of a device take turns)");
    if (h->node) h->node->mode = mode;
    return L3D_OK;
}

int l3d_line3d_node_turn_records(const l3d_line3d* h, int rank, int64_t* records)
{
    if (!h || !records) return L3D_ERR_INVALID;
    *records = 0;
    if (!h->node || rank < 0 || rank >= (int)h->node->ranks.size()) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "node_turn_records: no such rank of a node object");
    if ((int)h->node->turn_records.size() != (int)h->node->ranks.size()) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "node_turn_records: the last compute3Dmodel did not run in turns (l3d_line3d_set_node_mode 2)");
    *records = h->node->turn_records[(size_t)rank];
    return L3D_OK;
}

int l3d_line3d_set_turn_handover(l3d_line3d* h, int on)
{
    if (!h) return L3D_ERR_INVALID;
    if (!h->node) return h->fail(L3D_ERR_INVALID, "set_turn_handover: the turns are those of a node object (l3d_line3d_create_node with more than one rank)");
    if (on != 0 && on != 1) return h->fail(L3D_ERR_INVALID, "set_turn_handover: 0 (every turn computes the whole chain) or 1 (a turn computes its piece, warm from its predecessor's tail)");
    h->node->handover = on == 1;
    return L3D_OK;
}

int l3d_line3d_node_turn_views(const l3d_line3d* h, int rank, int64_t* views_computed, int* visits)
{
    if (!h || !views_computed || !visits) return L3D_ERR_INVALID;
    *views_computed = 0; *visits = 0;
    if (!h->node || rank < 0 || rank >= (int)h->node->ranks.size()) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "node_turn_views: no such rank of a node object");
    if (h->node->turn_views.size() != h->node->ranks.size() || h->node->turn_visits.size() != h->node->ranks.size())
        return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "node_turn_views: the last compute3Dmodel did not run in turns (l3d_line3d_set_node_mode 2)");
    *views_computed = h->node->turn_views[(size_t)rank];
    *visits = h->node->turn_visits[(size_t)rank];
    return L3D_OK;
}

void l3d_line3d_destroy(l3d_line3d* h)
{
    if (!h) return;
    if (h->node) { node_destroy(h); return; }
    if (h->warm_thread.joinable()) h->warm_thread.join();
    destroy_finalizer(h);                                   // joins the worker threads
    drop_plan(h);
    l3d_ctx_destroy(h->ctx);
    delete h;
}

const char* l3d_line3d_last_error(const l3d_line3d* h) { return h ? h->err.c_str() : "null handle"; }
l3d_ctx* l3d_line3d_context(l3d_line3d* h)
{
    if (h && h->node) { node_refuse(h, "context"); return nullptr; }
    return h ? h->ctx : nullptr;
}

// Line3D::reset, line3D.cc:62-92
int l3d_line3d_reset(l3d_line3d* h)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) { h->chain_summary.clear(); return node_each(h, [](L* r) { return l3d_line3d_reset(r); }); }
    for (auto& kv : h->views) { l3d_unregister_segments(h->ctx, kv.second.segs.data()); l3d_unregister_segments(h->ctx, kv.second.nb_segs.data()); }
    h->views.clear(); h->vlist.clear(); h->view_similarities.clear(); h->num_wps.clear(); h->common_wps.clear();
    h->worldpoints2views.clear(); h->visual_neighbors.clear(); h->fundamentals.clear(); h->matched.clear();
    h->pot.clear(); h->pot_foreign.clear(); h->hyps.clear(); h->best_idx.clear(); h->A.clear(); h->n_edges = 0; h->A_on_host = true; h->local2global.clear(); h->result.clear();
    h->refine_valid = false;                               // (the setting itself stays)
    h->merge_valid = false;                                // (the setting itself stays)
    h->support_valid = false;                              // (the setting itself stays)
    h->junc_valid = false;                                 // (the setting itself stays)
    h->plane_valid = false;                                // (the setting itself stays)
    h->result_valid = false;
    h->covis_ids.clear(); h->covis_views.clear(); h->covis_start.assign(1, 0); h->covis_dirty = false; h->covis_path = 0;      // (covis_mode stays)
    h->computation = false; h->prepared = false;
    drop_plan(h);
    return L3D_OK;
}

// ---- the add family: every exported form fills a request, and one route adds it ---------------------------------------------------------------
// (Line3D::addImage / addImage_fixed_sim, line3D.cc:95-342.)  The order of the route's decisions, for every form:
//   1. an image (pixels or a JPEG file) only: the JPEG headers, the camera of the undistortion, "image is empty!" for a size below 1x1
//   2. the forms with a data directory: the cache decision (cache_decision), taken once and handed on
//   3. an image whose cache does not stand in for it: the detector, on rank 0's device.  Nothing found: no view, L3D_OK, a stale cache removed
//   4. per rank (add_entry): the guards, then the decision's outcome -- the view from the cache file, or the stale file removed and the view from
//      the segments, its cache noted for prepare() to write -- then the links
// An image in device memory (AddKind::Device) is an image like the other two: step 1 checks its descriptor's fields, step 3 is the only place where its
// memory is looked at (pointer and extent check, stream wait, k_det_ingest) -- a cache that stands in for it leaves the memory untouched.
// The guards (4) come AFTER the detector (3) for an image: a second image of an id in use in which nothing is detected is L3D_OK and adds nothing.
// That is the behaviour the forms had one by one (tests/golden/add_table.json records it); moving the cheap guards to the front changes it.
namespace l3dh {
enum class AddKind { Segments, Cached, Pixels, Jpeg, Device };
// the undistortion a request asks for beside its entry's dist; more than one of dist, lens and remap is refused (warp_for_add)
struct AddWarp {
    bool dist_required = false;                     // the _distorted forms: a null dist is refused (elsewhere it means no distortion)
    const l3d_lens* lens = nullptr;                 // the ..._lens forms: a lens in the place of dist
    const l3d_remap* remap = nullptr;               // the ..._remap forms ("A REMAP"): in the place of dist and lens; K is the output camera
    bool identity_camera = false;                   // the undistort calls: dist within L3D_EPS goes on as the identity camera, so that the context's
                                                    // call still makes its checks of the image before it passes the pixels through
};
// an l3d_image_entry, or in place of its image the caller's segments or an opened segment cache
struct AddRequest {
    AddKind kind = AddKind::Segments;
    l3d_image_entry e{};                            // image_id, the image, width x height, K, R, t, dist, the links
    const float* segs = nullptr; int n = 0;         // Segments
    const l3d_segment_cache* cache = nullptr;       // Cached
    const l3d_device_image* dev = nullptr;          // Device: the image in device memory (e carries its size and the detector's channel count)
    bool cache_rules = false;                       // the form has a data directory: every one but add_image, add_image_fixed_sim, add_image_cached
    AddWarp warp;                                   // what the form asks for beside e.dist
    bool image() const { return kind == AddKind::Pixels || kind == AddKind::Jpeg || kind == AddKind::Device; }
};
enum class Cache { None, Load, Stale, Write };      // no cache rules or nothing to do | read the file | remove the file | note the file for prepare()
// what steps 1 and 2 found out about a request
struct AddPlan {
    unsigned width = 0, height = 0;                 // of the view (a JPEG file: from its headers)
    int channels = 0;
    l3d::DetWarp warp;                              // as the detector takes it, which checks it (warp_for_add); a remap: width x height above are its OUTPUT
    unsigned src_w = 0, src_h = 0;                  // the image as it arrives
    Cache cache = Cache::None;
    std::string file;                               // the cache file's path
    bool detect = false;
    unsigned new_w = 0, new_h = 0;                  // the size the detector works at
    float min_length = 0.0f;
};

static AddRequest add_request(AddKind kind, uint32_t id, unsigned width, unsigned height, const double* K, const double* R, const double* t, const uint32_t* link_ids,
                              const float* sims, int n_links, bool cache_rules = true)
{
    AddRequest rq;
    rq.kind = kind; rq.cache_rules = cache_rules;
    rq.e.image_id = id; rq.e.width = (int)width; rq.e.height = (int)height;
    rq.e.K = K; rq.e.R = R; rq.e.t = t;
    rq.e.link_ids = link_ids; rq.e.sims = sims; rq.e.n_links = n_links;
    return rq;
}
static AddRequest pixels_request(uint32_t id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K, const double* R,
                                 const double* t, const double* dist, bool dist_required, const uint32_t* link_ids, const float* sims, int n_links)
{
    AddRequest rq = add_request(AddKind::Pixels, id, (unsigned)width, (unsigned)height, K, R, t, link_ids, sims, n_links);
    rq.e.pixels = pixels; rq.e.channels = channels; rq.e.row_stride = row_stride;
    rq.e.dist = dist; rq.warp.dist_required = dist_required;
    return rq;
}
static AddRequest jpeg_request(uint32_t id, const unsigned char* bytes, size_t n, const double* K, const double* R, const double* t, const double* dist,
                               const uint32_t* link_ids, const float* sims, int n_links)
{
    AddRequest rq = add_request(AddKind::Jpeg, id, 0, 0, K, R, t, link_ids, sims, n_links);
    rq.e.jpeg = bytes; rq.e.jpeg_bytes = n; rq.e.dist = dist;
    return rq;
}
// an l3d_device_entry: the image stays where it is, the request carries its size
static AddRequest device_request(const l3d_device_entry& d)
{
    AddRequest rq = add_request(AddKind::Device, d.image_id, (unsigned)std::max(0, d.image.width), (unsigned)std::max(0, d.image.height), d.K, d.R, d.t, d.link_ids, d.sims, d.n_links);
    rq.e.channels = d.image.channels == 1 ? 1 : 3;
    rq.e.dist = d.dist;
    rq.dev = &d.image;
    return rq;
}
// single: l3d_line3d_add_image_entry, where an entry without an image is still the image its fields state -- any of width, height, channels,
// row_stride set: pixels, else a JPEG file -- so that a null image is refused in the words of the call named after it
static int entry_request(L* h, const l3d_image_entry& e, AddRequest& rq, bool single)
{
    const bool none = !e.pixels && !e.jpeg;
    if ((e.pixels && e.jpeg) || (none && !single)) return h->fail(L3D_ERR_INVALID, "add_images: an entry needs either pixels or a JPEG file");
    const bool pixels = e.pixels || (none && (e.width || e.height || e.channels || e.row_stride));
    rq.kind = pixels ? AddKind::Pixels : AddKind::Jpeg;
    rq.e = e; rq.cache_rules = true;
    return L3D_OK;
}

// the guards of addImage, line3D.cc:101-127 (print-and-return in the reference; a status here), and the null checks
static int add_guards(L* h, const AddRequest& rq, const AddPlan& p)
{
    const l3d_image_entry& e = rq.e;
    if (rq.kind == AddKind::Cached && !rq.cache) return h->fail(L3D_ERR_INVALID, "null segment cache");
    if (h->computation) return h->fail(L3D_ERR_INVALID, "reconstruction already performed! cannot add more images (try reset first)");
    if (h->views.count(e.image_id)) return h->fail(L3D_ERR_INVALID, "imageID already in use!");
    if (e.n_links == 0) return h->fail(L3D_ERR_INVALID, "unlinked images cannot be added!");
    if (p.width == 0 || p.height == 0 || (rq.cache_rules && (!e.K || !e.R || !e.t))) return h->fail(L3D_ERR_INVALID, "image is empty!");
    return L3D_OK;
}

// line3D.cc:128-199: the cache file of the view -- named after the size the detector works at (:133-138) -- probed once
static int cache_decision(L* h, uint32_t id, unsigned width, unsigned height, const char* data_directory, int max_img_width, int load_and_store, AddPlan& p)
{
    p.new_w = width; p.new_h = height;
    if (max_img_width > 0 && (int)std::max(width, height) > max_img_width) {                 // :133-138
        const float scale = float(max_img_width) / fmaxf((float)height, (float)width);
        p.new_w = (unsigned)roundf(float(width) * scale);
        p.new_h = (unsigned)roundf(float(height) * scale);
    }
    char name[160];
    if (l3d_segment_cache_filename(id, p.new_w, p.new_h, (h->node ? rank0(h) : h)->use_collinearity ? 1 : 0, name, sizeof(name)) != L3D_OK) return L3D_ERR_INVALID;
    p.file = std::string(data_directory ? data_directory : "") + name;
    FILE* f = fopen(p.file.c_str(), "rb");
    if (f) fclose(f);
    p.cache = f ? (load_and_store ? Cache::Load : Cache::Stale)                              // :159-168 | :153-156
                : (load_and_store ? Cache::Write : Cache::None);                             // :180-182
    return L3D_OK;
}

// the warp of an image in the add family.  K is the camera of the undistortion -- fx, fy, cx, cy = K[0], K[4], K[2], K[5] of the full-resolution K, as
// in the drivers (main_vsfm.cpp:250-262) -- and beside a lens or a remap the OUTPUT camera.  L3D_OK with `out` as the detector takes it (dist within
// L3D_EPS: nothing given, the plain path -- or, where the request says so, the identity camera) and out_w x out_h the size of the view, or the
// refusal's code with the message in h->err: what warp_check refuses for a lens or a remap, and a skewed K where the image is resampled.  (The
// fields of a k1, k2 camera are checked where the detector runs, behind the cache decision: a cache that stands in for the image leaves them unread)
static int warp_for_add(l3d_line3d* h, const double* K, const double* dist, const AddWarp& rq, int width, int height, int channels, l3d::DetWarp& out, int& out_w, int& out_h)
{
    const char* skewed = "lens distortion with a skewed K (K[1] != 0) is not supported";
    out = l3d::DetWarp();
    out_w = width; out_h = height;
    if (rq.remap && (rq.lens || dist)) return h->fail(L3D_ERR_INVALID, "undistortion: an entry carries a remap beside dist (k1, k2) or a lens");
    if (rq.lens && dist) return h->fail(L3D_ERR_INVALID, "undistortion: an entry carries both dist (k1, k2) and a lens");
    if (!rq.remap && !rq.lens && !dist && !rq.dist_required) return L3D_OK;
    if (!K) return h->fail(L3D_ERR_INVALID, "undistortion: K is null");
    if (!rq.remap && !rq.lens) {
        if (!dist) return h->fail(L3D_ERR_INVALID, "undistortion: dist (k1, k2) is null");
        if (std::fabs(dist[0]) <= 1e-12 && std::fabs(dist[1]) <= 1e-12) { out.has_cam = rq.identity_camera; return L3D_OK; }
        if (K[1] != 0.0) return h->fail(L3D_ERR_UNSUPPORTED, skewed);
        out.has_cam = true;
        out.cam = l3d::DetCamera{ K[0], K[4], K[2], K[5], dist[0], dist[1] };
        return L3D_OK;
    }
    if (rq.remap && (width <= 0 || height <= 0)) return h->fail(L3D_ERR_INVALID, "image is empty!");
    const double camera[6] = { K[0], K[4], K[2], K[5], 0.0, 0.0 };
    out = l3d::warp_of_entry(camera, rq.lens, rq.remap);
    l3d::WarpPlan plan;
    std::string err;
    if (const int rc = l3d::warp_check(out, width, height, channels, plan, err)) return h->fail(rc, err.c_str());
    if (plan.route != l3d::WarpRoute::None && K[1] != 0.0) return h->fail(L3D_ERR_UNSUPPORTED, skewed);
    out_w = plan.out_w; out_h = plan.out_h;
    return L3D_OK;
}

// steps 1 and 2.  A JPEG file's size (cache name, max_img_width rule) comes from its headers; the entropy-coded data is touched only when the detector runs
static int add_plan(L* h, const AddRequest& rq, const char* data_directory, int max_img_width, int load_and_store, AddPlan& p)
{
    const l3d_image_entry& e = rq.e;
    int width = e.width, height = e.height;
    p.channels = e.channels;
    if (rq.kind == AddKind::Jpeg) {
        if (!e.jpeg) return h->fail(L3D_ERR_INVALID, "jpeg: null argument");
        const int rc = l3d_jpeg_info(e.jpeg, e.jpeg_bytes, &width, &height, &p.channels);
        if (rc != L3D_OK) return h->fail(rc, l3d_jpeg_last_error());
    }
    if (rq.kind == AddKind::Device) {           // the descriptor's fields; its memory is looked at only where the detector runs
        char msg[160];
        const int rc = l3d_device_image_check(rq.dev, msg, sizeof(msg));
        if (rc != L3D_OK) return h->fail(rc, msg);
    }
    p.src_w = (unsigned)std::max(0, width); p.src_h = (unsigned)std::max(0, height);
    if (rq.image()) {                           // (a remap is checked at the source size, the view is its output)
        if (const int rc = warp_for_add(h, e.K, e.dist, rq.warp, width, height, p.channels == 1 ? 1 : 3, p.warp, width, height)) return rc;
        if (width <= 0 || height <= 0) return h->fail(L3D_ERR_INVALID, "image is empty!");
    }
    p.width = (unsigned)width; p.height = (unsigned)height;
    if (!rq.cache_rules) return L3D_OK;
    if (const int rc = cache_decision(h, e.image_id, p.width, p.height, data_directory, max_img_width, load_and_store, p)) return rc;
    p.detect = rq.image() && p.cache != Cache::Load;                                         // (a cache that is present and wanted stands in for the image)
    if (!p.detect) return L3D_OK;
    if (!(h->node ? rank0(h) : h)->ctx) return h->fail(L3D_ERR_INVALID, "no device context to detect line segments with");
    p.min_length = 0.005f * sqrtf(float(height * height + width * width));                   // :176, commons.h:43
    return L3D_OK;
}

// segments and collinearities of an opened cache as the view's (line3D.cc:160-168): nothing is recomputed
static int view_from_cache(L* h, const AddRequest& rq, const AddPlan& p, const l3d_segment_cache* cache)
{
    const int n = l3d_segment_cache_num_segments(cache), nc = l3d_segment_cache_num_collinearities(cache);
    std::vector<float> segs((size_t)n * 4 + 1), cw((size_t)nc + 1);
    std::vector<int32_t> ci((size_t)nc + 1), cj((size_t)nc + 1);
    l3d_segment_cache_get(cache, segs.data(), ci.data(), cj.data(), cw.data());
    if (n <= 0 || !rq.e.K || !rq.e.R || !rq.e.t) return h->fail(L3D_ERR_INVALID, "no segments");
    return make_view(h, rq.e.image_id, p.width, p.height, segs.data(), n, rq.e.K, rq.e.R, rq.e.t, ci.data(), cj.data(), cw.data(), nc);
}

static void file_links(L* h, uint32_t id, const l3d_image_entry& e)
{
    if (!e.sims && h->covis_mode == 1) {                   // l3d_line3d_set_covisibility: the list is kept, prepare() counts
        h->covis_dirty = true;
        if (!h->covis_store) return;
        h->covis_ids.insert(h->covis_ids.end(), e.link_ids, e.link_ids + e.n_links);
        h->covis_views.push_back(id);
        h->covis_start.push_back((int64_t)h->covis_ids.size());
        return;
    }
    if (!e.sims) { process_worldpoints(h, id, e.link_ids, e.n_links); return; }
    for (int i = 0; i < e.n_links; ++i)                    // setViewSimilarity, :1938-1946
        if (e.sims[i] > 0.01f) h->view_similarities[id][e.link_ids[i]] = e.sims[i];
}

// step 4 (and the second half of 3).  detected: null, or what the detector found in the request's image
static int add_entry(L* h, const AddRequest& rq, const AddPlan& p, const std::vector<float>* detected)
{
    if (detected && detected->empty()) {                   // no view and no error (:186-190); a stale cache goes with the flag off (:153-156)
        if (p.cache == Cache::Stale) remove(p.file.c_str());
        return L3D_OK;
    }
    const uint32_t id = rq.e.image_id;
    if (h->node)        // (every rank adds the view; the cache file is written once, by rank 0)
        return node_each(h, [&](L* r) {
            const int rc = add_entry(r, rq, p, detected);
            if (rc == L3D_OK && r != rank0(h)) r->views[id].cache_to_write.clear();
            return rc;
        });
    int rc = add_guards(h, rq, p);
    if (rc) return rc;
    if (rq.kind == AddKind::Cached) rc = view_from_cache(h, rq, p, rq.cache);
    else if (p.cache == Cache::Load) {
        l3d_segment_cache* cache = nullptr;
        rc = l3d_segment_cache_read(p.file.c_str(), &cache);
        rc = rc != L3D_OK ? h->fail(rc, l3d_segment_cache_last_error(cache)) : view_from_cache(h, rq, p, cache);      // (the reference exits, serialization.h:63)
        l3d_segment_cache_free(cache);
    } else {
        if (p.cache == Cache::Stale) remove(p.file.c_str());
        const float* segs = detected ? detected->data() : rq.segs;
        const int n = detected ? (int)(detected->size() / 4) : rq.n;
        // a size-only image type of the facade brings neither segments nor pixels: nothing to add
        if (rq.cache_rules && (n <= 0 || !segs))
            return h->fail(L3D_ERR_INVALID, ("image [" + std::to_string(id) + "]: no segment cache " + p.file + " and no segments given -- line segment "
                                             "detection is not part of this library (run the reference once with loadAndStoreSegments, or pass the segments)").c_str());
        if (n <= 0 || !segs || !rq.e.K || !rq.e.R || !rq.e.t) return h->fail(L3D_ERR_INVALID, "no segments");   // detectLineSegments failed: no view, :186-190
        rc = make_view(h, id, p.width, p.height, segs, n, rq.e.K, rq.e.R, rq.e.t);
        if (rc == L3D_OK && p.cache == Cache::Write) h->views[id].cache_to_write = p.file;
    }
    if (rc) return rc;
    file_links(h, id, rq.e);
    return L3D_OK;
}

// the detector's entry for a request whose plan says detect
static void det_entry(const AddRequest& rq, const AddPlan& p, l3d::DetEntry& d)
{
    const l3d_image_entry& e = rq.e;
    d.pixels = e.pixels; d.width = (int)p.src_w; d.height = (int)p.src_h; d.channels = p.channels;
    d.row_stride = e.jpeg ? (size_t)p.src_w * p.channels : e.row_stride;
    d.jpeg = e.jpeg; d.jpeg_bytes = e.jpeg_bytes;
    d.dev = rq.dev;
    d.new_width = (int)p.new_w; d.new_height = (int)p.new_h; d.min_length = p.min_length; d.max_segments = 3000;
    d.warp = p.warp;
}

// the route for one request
static int add_one(L* h, const AddRequest& rq, const char* data_directory = nullptr, int max_img_width = 0, int load_and_store = 0)
{
    if (!h) return L3D_ERR_INVALID;
    AddPlan p;
    if (const int rc = add_plan(h, rq, data_directory, max_img_width, load_and_store, p)) return rc;
    if (!p.detect) return add_entry(h, rq, p, nullptr);
    l3d_ctx* ctx = (h->node ? rank0(h) : h)->ctx;
    // a JPEG file is decoded on the device into the detector, and a device image's memory is checked and gathered -- only here, behind the cache decision
    l3d::DetEntry d;
    det_entry(rq, p, d);
    std::vector<float> segs;
    const int rc = l3d::detect_one(ctx, d, segs);
    if (rc != L3D_OK) return h->fail(rc, l3d_last_error(ctx));
    return add_entry(h, rq, p, &segs);
}
}  // namespace l3dh

// addImage / addImage_fixed_sim with precomputed segments, line3D.cc:95-217, 220-342
int l3d_line3d_add_image(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n,
                         const double* K, const double* R, const double* t, const uint32_t* worldpoints, int n_wps)
{
    AddRequest rq = add_request(AddKind::Segments, id, width, height, K, R, t, worldpoints, nullptr, n_wps, false);
    rq.segs = segs; rq.n = n;
    return add_one(h, rq);
}
int l3d_line3d_add_image_fixed_sim(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n,
                                   const double* K, const double* R, const double* t,
                                   const uint32_t* sim_ids, const float* sims, int n_sims)
{
    AddRequest rq = add_request(AddKind::Segments, id, width, height, K, R, t, sim_ids, sims, n_sims, false);
    rq.segs = segs; rq.n = n;
    return add_one(h, rq);
}
// addImage when the segment cache exists, line3D.cc:160-168: segments and collinearities come from the file
int l3d_line3d_add_image_cached(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const l3d_segment_cache* cache,
                                const double* K, const double* R, const double* t, const uint32_t* worldpoints, int n_wps)
{
    AddRequest rq = add_request(AddKind::Cached, id, width, height, K, R, t, worldpoints, nullptr, n_wps, false);
    rq.cache = cache;
    return add_one(h, rq);
}
// ---- the segment-taking forms behind a segment mask ("A SEGMENT MASK"): the filter once, on the object's device (a node object: rank 0's), then
// the existing add with what it left.  Nothing left: no view and no error, as when the detector finds nothing (the guards come after the filter)
static int add_masked(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n, const double* K, const double* R, const double* t,
                      const uint32_t* link_ids, const float* sims, int n_links, const l3d_segment_mask* mask)
{
    if (!h) return L3D_ERR_INVALID;
    if (!mask) return h->fail(L3D_ERR_INVALID, "segment mask: the mask is null");
    L* owner = h->node ? rank0(h) : h;
    if (!owner->ctx) return h->fail(L3D_ERR_INVALID, "no device context to mask line segments with");
    // without an active lens the mask lies in the view's grid and has its extent (a lens the checks refuse: the filter says so, below)
    bool in_view_grid = true;
    if (mask->lens) {
        l3d::DetWarp w;
        w.has_lens = true;
        w.lens = l3d::make_lens(*mask->lens, mask->fx, mask->fy, mask->cx, mask->cy);
        l3d::WarpPlan plan;
        std::string err;
        in_view_grid = l3d::warp_check(w, mask->mask_width, mask->mask_height, 1, plan, err) == L3D_OK && plan.route == l3d::WarpRoute::None;
    }
    if (in_view_grid && mask->mask && mask->mask_width >= 1 && mask->mask_height >= 1 && ((unsigned)mask->mask_width != width || (unsigned)mask->mask_height != height))
        return h->fail(L3D_ERR_INVALID, ("segment mask: the mask is " + std::to_string(mask->mask_width) + " x " + std::to_string(mask->mask_height) + ", the view " +
                                         std::to_string(width) + " x " + std::to_string(height)).c_str());
    float* out = nullptr;
    int32_t* src = nullptr;
    int n_out = 0;
    const int rc = l3d_mask_segments(owner->ctx, segs, n, mask, &out, &src, &n_out);
    if (rc != L3D_OK) return h->fail(rc, l3d_last_error(owner->ctx));
    int ret = L3D_OK;
    if (n_out > 0) {
        AddRequest rq = add_request(AddKind::Segments, id, width, height, K, R, t, link_ids, sims, n_links, false);
        rq.segs = out; rq.n = n_out;
        ret = add_one(h, rq);
    }
    l3d_free(out);
    l3d_free(src);
    return ret;
}
int l3d_line3d_add_image_masked(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n, const double* K, const double* R, const double* t,
                                const uint32_t* link_ids, const float* sims, int n_links, const l3d_segment_mask* mask)
{
    return add_masked(h, id, width, height, segs, n, K, R, t, link_ids, sims, n_links, mask);
}
// the cache's segments through the filter; its collinearities are not taken over, the view computes its own.  No cache file is touched
int l3d_line3d_add_image_cached_masked(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const l3d_segment_cache* cache, const double* K, const double* R,
                                       const double* t, const uint32_t* link_ids, const float* sims, int n_links, const l3d_segment_mask* mask)
{
    if (!h) return L3D_ERR_INVALID;
    if (!cache) return h->fail(L3D_ERR_INVALID, "null segment cache");
    const int n = l3d_segment_cache_num_segments(cache), nc = l3d_segment_cache_num_collinearities(cache);
    std::vector<float> segs((size_t)std::max(n, 0) * 4 + 1), cw((size_t)std::max(nc, 0) + 1);
    std::vector<int32_t> ci((size_t)std::max(nc, 0) + 1), cj((size_t)std::max(nc, 0) + 1);
    l3d_segment_cache_get(cache, segs.data(), ci.data(), cj.data(), cw.data());
    return add_masked(h, id, width, height, segs.data(), std::max(n, 0), K, R, t, link_ids, sims, n_links, mask);
}
// the same with the cache rules, line3D.cc:128-199
int l3d_line3d_add_image_ex(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n, const double* K, const double* R,
                            const double* t, const uint32_t* worldpoints, int n_wps, const char* data_directory, int max_img_width, int load_and_store)
{
    AddRequest rq = add_request(AddKind::Segments, id, width, height, K, R, t, worldpoints, nullptr, n_wps);
    rq.segs = segs; rq.n = n;
    return add_one(h, rq, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_image_fixed_sim_ex(l3d_line3d* h, uint32_t id, unsigned width, unsigned height, const float* segs, int n, const double* K, const double* R,
                                      const double* t, const uint32_t* sim_ids, const float* sims, int n_sims, const char* data_directory, int max_img_width,
                                      int load_and_store)
{
    AddRequest rq = add_request(AddKind::Segments, id, width, height, K, R, t, sim_ids, sims, n_sims);
    rq.segs = segs; rq.n = n;
    return add_one(h, rq, data_directory, max_img_width, load_and_store);
}

// from pixels: the entry with pixels filled; _distorted: with dist, which may not be null there
int l3d_line3d_add_image_pixels(l3d_line3d* h, uint32_t id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                const double* R, const double* t, const uint32_t* worldpoints, int n_wps, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_one(h, pixels_request(id, pixels, width, height, channels, row_stride, K, R, t, nullptr, false, worldpoints, nullptr, n_wps), data_directory, max_img_width,
                   load_and_store);
}
int l3d_line3d_add_image_pixels_fixed_sim(l3d_line3d* h, uint32_t id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                          const double* R, const double* t, const uint32_t* sim_ids, const float* sims, int n_sims, const char* data_directory,
                                          int max_img_width, int load_and_store)
{
    return add_one(h, pixels_request(id, pixels, width, height, channels, row_stride, K, R, t, nullptr, false, sim_ids, sims, n_sims), data_directory, max_img_width,
                   load_and_store);
}
int l3d_line3d_add_image_pixels_distorted(l3d_line3d* h, uint32_t id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                          const double* K, const double* R, const double* t, const double dist[2], const uint32_t* worldpoints, int n_wps,
                                          const char* data_directory, int max_img_width, int load_and_store)
{
    return add_one(h, pixels_request(id, pixels, width, height, channels, row_stride, K, R, t, dist, true, worldpoints, nullptr, n_wps), data_directory, max_img_width,
                   load_and_store);
}
int l3d_line3d_add_image_pixels_fixed_sim_distorted(l3d_line3d* h, uint32_t id, const unsigned char* pixels, int width, int height, int channels, size_t row_stride,
                                                    const double* K, const double* R, const double* t, const double dist[2], const uint32_t* sim_ids, const float* sims,
                                                    int n_sims, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_one(h, pixels_request(id, pixels, width, height, channels, row_stride, K, R, t, dist, true, sim_ids, sims, n_sims), data_directory, max_img_width,
                   load_and_store);
}

// ---- the undistort calls of an object: the context's call with the object's device (a node object: rank 0's) and the add family's K rule
// (warp_for_add: K is the camera, beside a lens or a remap the output camera; a skewed K with an image that is resampled is refused)
static int undistort_with(l3d_line3d* h, bool arguments, const double* K, const double* dist, const AddWarp& rq, const l3d::WarpIo& io)
{
    if (!h) return L3D_ERR_INVALID;
    L* owner = h->node ? rank0(h) : h;
    if (!owner->ctx) return h->fail(L3D_ERR_INVALID, "no device context to undistort with");
    if (!arguments) return h->fail(L3D_ERR_INVALID, "undistort: null argument");
    const int width = io.in ? io.in->width : io.width, height = io.in ? io.in->height : io.height, channels = io.in ? io.in->channels : io.channels;
    l3d::DetWarp warp;
    int out_w = 0, out_h = 0;
    if (const int rc = warp_for_add(h, K, dist, rq, width, height, channels == 1 ? 1 : 3, warp, out_w, out_h)) return rc;
    const int rc = l3d::undistort_one(owner->ctx, io, warp);
    return rc == L3D_OK ? rc : h->fail(rc, l3d_last_error(owner->ctx));
}
// the drivers' undistort block on its own (main_vsfm.cpp:243-270)
int l3d_line3d_undistort_image(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K, double k1, double k2,
                               unsigned char* out, size_t out_row_stride)
{
    const double dist[2] = { k1, k2 };
    return undistort_with(h, true, K, dist, AddWarp{ true, nullptr, nullptr, true }, l3d::WarpIo{ pixels, width, height, channels, row_stride, out, out_row_stride });
}
int l3d_line3d_undistort_image_device(l3d_line3d* h, const l3d_device_image* in, const double* K, double k1, double k2, const l3d_device_image* out)
{
    const double dist[2] = { k1, k2 };
    l3d::WarpIo io;
    io.in = in; io.dout = out;
    return undistort_with(h, in && out, K, dist, AddWarp{ true, nullptr, nullptr, true }, io);
}
// l3d_undistort_image_lens (a lens that passes the pixels through goes on as it is: the context call copies them)
int l3d_line3d_undistort_image_lens(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                    const l3d_lens* lens, unsigned char* out, size_t out_row_stride)
{
    return undistort_with(h, lens != nullptr, K, nullptr, AddWarp{ false, lens, nullptr }, l3d::WarpIo{ pixels, width, height, channels, row_stride, out, out_row_stride });
}
// l3d_undistort_image_remap: out of the remap's output size, valid NULL or one byte per output pixel
int l3d_line3d_undistort_image_remap(l3d_line3d* h, const unsigned char* pixels, int width, int height, int channels, size_t row_stride, const double* K,
                                     const l3d_remap* remap, unsigned char* out, size_t out_row_stride, unsigned char* valid, size_t valid_row_stride)
{
    return undistort_with(h, remap && K, K, nullptr, AddWarp{ false, nullptr, remap },
                          l3d::WarpIo{ pixels, width, height, channels, row_stride, out, out_row_stride, valid, valid_row_stride });
}

// from a baseline JPEG file in memory: the entry with jpeg filled
int l3d_line3d_add_image_jpeg(l3d_line3d* h, uint32_t id, const unsigned char* bytes, size_t n, const double* K, const double* R, const double* t, const double dist[2],
                              const uint32_t* worldpoints, int n_wps, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_one(h, jpeg_request(id, bytes, n, K, R, t, dist, worldpoints, nullptr, n_wps), data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_image_jpeg_fixed_sim(l3d_line3d* h, uint32_t id, const unsigned char* bytes, size_t n, const double* K, const double* R, const double* t,
                                        const double dist[2], const uint32_t* sim_ids, const float* sims, int n_sims, const char* data_directory, int max_img_width,
                                        int load_and_store)
{
    return add_one(h, jpeg_request(id, bytes, n, K, R, t, dist, sim_ids, sims, n_sims), data_directory, max_img_width, load_and_store);
}

// Many images in one call: the route above per entry, in entry order, with the detector run once (batched, l3d_detect.hip) over all entries that
// need it.  An entry fails alone, with its single call's code and message
namespace l3dh {
// one request of a batch: what filling it said (rc, msg), the request, then its plan and its place among the detector's entries
struct AddItem { int rc = L3D_OK; std::string msg; AddRequest rq; AddPlan p; int detect_at = -1; };
// the batch body of every ..._add_images form: steps 1 and 2 per request, one run of the batch detector, steps 3 to 5 in request order
static int add_batch(L* h, std::vector<AddItem>& items, const char* data_directory, int max_img_width, int load_and_store, int* status)
{
    const int n = (int)items.size();
    std::vector<l3d::DetEntry> todo;
    todo.reserve((size_t)n);
    for (int i = 0; i < n; ++i) {
        AddItem& it = items[i];
        if (it.rc != L3D_OK) continue;          // refused when it was filled: msg says why
        it.rc = add_plan(h, it.rq, data_directory, max_img_width, load_and_store, it.p);
        if (it.rc != L3D_OK) { it.msg = h->err; continue; }
        if (!it.p.detect) continue;
        l3d::DetEntry d;
        det_entry(it.rq, it.p, d);                              // (items does not grow: the addresses hold)
        it.detect_at = (int)todo.size();
        todo.push_back(d);
    }
    std::vector<std::vector<float>> segs;
    std::vector<int> det_status;
    std::vector<std::string> det_msg;
    int rc_all = L3D_OK;
    if (!todo.empty())
        rc_all = l3d::detect_segments_batch((h->node ? rank0(h) : h)->ctx, todo.data(), (int)todo.size(), segs, det_status, det_msg);   // (one status per entry, whatever it returns)
    std::string lines;
    for (int i = 0; i < n; ++i) {
        AddItem& it = items[i];
        if (it.rc == L3D_OK && it.detect_at >= 0 && det_status[it.detect_at] != L3D_OK) { it.rc = det_status[it.detect_at]; it.msg = det_msg[it.detect_at]; }
        else if (it.rc == L3D_OK) {
            it.rc = add_entry(h, it.rq, it.p, it.detect_at >= 0 ? &segs[it.detect_at] : nullptr);
            if (it.rc != L3D_OK) it.msg = h->err;
        }
        if (status) status[i] = it.rc;
        if (it.rc != L3D_OK) lines += (lines.empty() ? "image " : "\nimage ") + std::to_string(it.rq.e.image_id) + ": " + it.msg;
    }
    h->err = lines;
    return rc_all;
}

// ---- the entry forms: an l3d_image_entry or an l3d_device_entry (an image in device memory: a descriptor where the other has pixels or a file),
// alone or n of them, each with a lens or a remap beside it or neither.  One filler per entry kind, one body for the single forms and one for the batches
static int fill_request(L* h, const l3d_image_entry& e, AddRequest& rq, bool single) { return entry_request(h, e, rq, single); }
static int fill_request(L*, const l3d_device_entry& e, AddRequest& rq, bool) { rq = device_request(e); return L3D_OK; }
static const char* form_name(const l3d_image_entry*, bool single) { return single ? "add_image_entry: null argument" : "add_images: null argument"; }
static const char* form_name(const l3d_device_entry*, bool single) { return single ? "add_device_entry: null argument" : "add_device_images: null argument"; }
static void beside(AddWarp& w, const l3d_lens* lens) { w.lens = lens; }
static void beside(AddWarp& w, const l3d_remap* remap) { w.remap = remap; }

extern "C++" {
template <class E, class X>
static int add_entry_with(L* h, const E* e, const X* x, const char* data_directory, int max_img_width, int load_and_store)
{
    if (!h) return L3D_ERR_INVALID;
    if (!e) return h->fail(L3D_ERR_INVALID, form_name(e, true));
    AddRequest rq;
    if (const int rc = fill_request(h, *e, rq, true)) return rc;
    beside(rq.warp, x);
    return add_one(h, rq, data_directory, max_img_width, load_and_store);
}
template <class E, class X>
static int add_entries_with(L* h, const E* e, const X* const* x, int n, const char* data_directory, int max_img_width, int load_and_store, int* status)
{
    if (!h) return L3D_ERR_INVALID;
    if (n < 0 || (n > 0 && !e)) return h->fail(L3D_ERR_INVALID, form_name(e, false));
    std::vector<AddItem> items((size_t)n);
    for (int i = 0; i < n; ++i) {
        items[i].rc = fill_request(h, e[i], items[i].rq, false);
        if (items[i].rc != L3D_OK) { items[i].msg = h->err; items[i].rq.e.image_id = e[i].image_id; }
        beside(items[i].rq.warp, x ? x[i] : nullptr);
    }
    return add_batch(h, items, data_directory, max_img_width, load_and_store, status);
}
}  // extern "C++"
}  // namespace l3dh

int l3d_line3d_add_image_entry_lens(l3d_line3d* h, const l3d_image_entry* e, const l3d_lens* lens, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_entry_with(h, e, lens, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_image_entry_remap(l3d_line3d* h, const l3d_image_entry* e, const l3d_remap* remap, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_entry_with(h, e, remap, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_image_entry(l3d_line3d* h, const l3d_image_entry* e, const char* data_directory, int max_img_width, int load_and_store)
{
    return l3d_line3d_add_image_entry_lens(h, e, nullptr, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_images_lens(l3d_line3d* h, const l3d_image_entry* e, const l3d_lens* const* lens, int n, const char* data_directory, int max_img_width,
                               int load_and_store, int* status)
{
    return add_entries_with(h, e, lens, n, data_directory, max_img_width, load_and_store, status);
}
int l3d_line3d_add_images_remap(l3d_line3d* h, const l3d_image_entry* e, const l3d_remap* const* remap, int n, const char* data_directory, int max_img_width,
                                int load_and_store, int* status)
{
    return add_entries_with(h, e, remap, n, data_directory, max_img_width, load_and_store, status);
}
int l3d_line3d_add_images(l3d_line3d* h, const l3d_image_entry* e, int n, const char* data_directory, int max_img_width, int load_and_store, int* status)
{
    return l3d_line3d_add_images_lens(h, e, nullptr, n, data_directory, max_img_width, load_and_store, status);
}
int l3d_line3d_add_device_entry_lens(l3d_line3d* h, const l3d_device_entry* e, const l3d_lens* lens, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_entry_with(h, e, lens, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_device_entry_remap(l3d_line3d* h, const l3d_device_entry* e, const l3d_remap* remap, const char* data_directory, int max_img_width, int load_and_store)
{
    return add_entry_with(h, e, remap, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_device_entry(l3d_line3d* h, const l3d_device_entry* e, const char* data_directory, int max_img_width, int load_and_store)
{
    return l3d_line3d_add_device_entry_lens(h, e, nullptr, data_directory, max_img_width, load_and_store);
}
int l3d_line3d_add_device_images_lens(l3d_line3d* h, const l3d_device_entry* e, const l3d_lens* const* lens, int n, const char* data_directory, int max_img_width,
                                      int load_and_store, int* status)
{
    return add_entries_with(h, e, lens, n, data_directory, max_img_width, load_and_store, status);
}
int l3d_line3d_add_device_images_remap(l3d_line3d* h, const l3d_device_entry* e, const l3d_remap* const* remap, int n, const char* data_directory, int max_img_width,
                                       int load_and_store, int* status)
{
    return add_entries_with(h, e, remap, n, data_directory, max_img_width, load_and_store, status);
}
int l3d_line3d_add_device_images(l3d_line3d* h, const l3d_device_entry* e, int n, const char* data_directory, int max_img_width, int load_and_store, int* status)
{
    return l3d_line3d_add_device_images_lens(h, e, nullptr, n, data_directory, max_img_width, load_and_store, status);
}

// l3d_decode_jpeg_device with the object's device (a node object: rank 0's)
int l3d_line3d_decode_jpeg_device(l3d_line3d* h, const unsigned char* bytes, size_t n, const l3d_device_image* out)
{
    if (!h) return L3D_ERR_INVALID;
    L* owner = h->node ? rank0(h) : h;
    if (!owner->ctx) return h->fail(L3D_ERR_INVALID, "no device context to decode with");
    const int rc = l3d_decode_jpeg_device(owner->ctx, bytes, n, out);
    return rc == L3D_OK ? rc : h->fail(rc, l3d_last_error(owner->ctx));
}
// l3d_decode_jpeg with the object's device (a node object: rank 0's)
int l3d_line3d_decode_jpeg(l3d_line3d* h, const unsigned char* bytes, size_t n, unsigned char* out, size_t out_row_stride)
{
    if (!h) return L3D_ERR_INVALID;
    L* owner = h->node ? rank0(h) : h;
    if (!owner->ctx) return h->fail(L3D_ERR_INVALID, "no device context to decode with");
    const int rc = l3d::decode_jpeg(owner->ctx, bytes, n, out, out_row_stride);
    return rc == L3D_OK ? rc : h->fail(rc, l3d_last_error(owner->ctx));
}

int l3d_line3d_num_cameras(const l3d_line3d* h) { return !h ? 0 : h->node ? l3d_line3d_num_cameras(rank0(h)) : (int)h->views.size(); }

// verbose: the counters compute_pairwise_matches prints per view (cudawrapper.cu:953,1114; line3D.cc:652), as totals of the pass -- the resident
// chain never hands a view's lists to the host
static int match_views_reported(l3d_line3d* h)
{
    const int rc = match_views(h);
    if (!rc && h->verbose)
        printf("[L3D] #raw_matches:          %.0f (all views)\n[L3D] #filtered_matches (2): %.0f (all views)\n[L3D] segment pairs tested:  %.0f\n",
               h->stat_raw, h->stat_kept, h->stat_pairs);
    return rc;
}

int l3d_line3d_prepare(l3d_line3d* h)
{
    if (h && h->node) {
        const int rc = node_count_covisibility(h);
        return rc ? rc : node_run(h, [h](int r) { return prepare(h->node->ranks[(size_t)r]); });
    }
    return h ? prepare(h) : L3D_ERR_INVALID;
}
int l3d_line3d_match_views(l3d_line3d* h)
{
    if (h && h->node) return node_refuse(h, "match_views");
    if (!h || !h->prepared) return h ? h->fail(L3D_ERR_INVALID, "prepare first") : L3D_ERR_INVALID;
    return match_views_reported(h);
}
int l3d_line3d_finish(l3d_line3d* h, int perform_diffusion)
{
    if (h && h->node) return node_refuse(h, "finish");
    if (!h || !h->prepared) return h ? h->fail(L3D_ERR_INVALID, "prepare first") : L3D_ERR_INVALID;
    const double t0 = now_s();
    if (h->partitioned && !h->part_exchange) return h->fail(L3D_ERR_INVALID, "finish: matchViews' products are partitioned over the ranks (l3d_line3d_finish_sharded)");
    if (h->hyps_done) h->hyps_done = false;                // (a turn of a node object selected before it released its records)
    else if (h->resident_products) { const int rg = greedy_selection_resident(h); if (rg) return rg; }
    else greedy_selection(h);                              // optimizeLocalMatches, :888-896
    if (hopt(h).timing) fprintf(stderr, "[l3d finish] %-28s %8.2f ms\n", "greedy selection", (now_s() - t0) * 1e3);
    h->result_valid = false;
    int rc = cluster_segments_2D(h, perform_diffusion != 0);
    h->refine_valid = false;
    h->merge_valid = false;
    if (!rc && h->merge_on) rc = merge_result(h);
    if (!rc && h->refine_on) rc = refine_result(h);
    h->junc_valid = false;
    h->plane_valid = false;
    JunctionHandOn hand;
    if (!rc && (h->junc_on || h->plane_on)) rc = junction_result(h, h->plane_on ? &hand : nullptr);
    if (!rc && h->plane_on) rc = plane_result(h, hand);
    h->support_valid = false;
    h->result_valid = rc == L3D_OK;
    if (!rc && h->support_on) { rc = support_result(h); h->result_valid = rc == L3D_OK; }
    if (hopt(h).timing) fprintf(stderr, "[l3d finish] %-28s %8.2f ms\n", "total", (now_s() - t0) * 1e3);
    if (!rc && h->verbose)      // line3D.cc:959-961, 1226-1229, 1251
        printf("[L3D] #clusterable_segments:  %zu\n[L3D] A: #num_entries = %zu\n[L3D] A: #num_rows    = %zu\n[L3D] %zu 3D lines found!\n",
               h->hyps.size(), h->n_edges, h->local2global.size(), h->result.size());
    return rc;
}
// the refinement of the result (refine_result, line3d_host_finish.cpp).  A node object refines on rank 0, which holds the result: the other ranks keep it off
int l3d_line3d_set_refinement(l3d_line3d* h, int on, int max_iterations, double huber_px)
{
    if (!h) return L3D_ERR_INVALID;
    if (max_iterations < 0 || !(huber_px >= 0.0) || huber_px - huber_px != 0.0) return h->fail(L3D_ERR_INVALID, "set_refinement: max_iterations and huber_px must not be negative");
    if (h->node) return l3d_line3d_set_refinement(rank0(h), on, max_iterations, huber_px);
    h->refine_on = on != 0; h->refine_max_iterations = max_iterations; h->refine_huber_px = huber_px;
    return L3D_OK;
}
// the merging of the result's duplicate lines (merge_result, line3d_host_finish.cpp).  A node object merges on rank 0, which holds the result
int l3d_line3d_set_merging(l3d_line3d* h, int on, double dist_px, double angle_deg, double max_gap, int max_rounds)
{
    if (!h) return L3D_ERR_INVALID;
    const auto finite_nonneg = [](double x) { return x >= 0.0 && x - x == 0.0; };
    if (!finite_nonneg(dist_px) || !finite_nonneg(max_gap) || !(angle_deg >= 0.0 && angle_deg <= 90.0) || max_rounds < 1)
        return h->fail(L3D_ERR_INVALID, "set_merging: dist_px and max_gap must be finite and not negative, angle_deg in [0, 90], max_rounds at least 1");
    if (h->node) return l3d_line3d_set_merging(rank0(h), on, dist_px, angle_deg, max_gap, max_rounds);
    h->merge_on = on != 0; h->merge_dist_px = dist_px; h->merge_angle_deg = angle_deg; h->merge_max_gap = max_gap; h->merge_max_rounds = max_rounds;
    return L3D_OK;
}
int l3d_line3d_get_merging(const l3d_line3d* h, int32_t* counts, int32_t* final_index, int32_t* n_sources)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_merging(rank0(h), counts, final_index, n_sources);
    if (!h->merge_valid || !h->result_valid || h->merge_n_sources.size() != h->result.size())
        return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "get_merging: the last finish ran without the merging");
    if (counts) memcpy(counts, h->merge_counts, sizeof(h->merge_counts));
    if (final_index && !h->merge_final_index.empty()) memcpy(final_index, h->merge_final_index.data(), h->merge_final_index.size() * 4);
    if (n_sources && !h->merge_n_sources.empty()) memcpy(n_sources, h->merge_n_sources.data(), h->merge_n_sources.size() * 4);
    return L3D_OK;
}
// the support of the result's lines over all views (support_gather / support_result, line3d_host_finish.cpp).  A node object gathers on rank 0, which holds
// the result
int l3d_line3d_set_support(l3d_line3d* h, int on, double dist_px, double angle_deg, double min_overlap)
{
    if (!h) return L3D_ERR_INVALID;
    if (!(dist_px >= 0.0 && dist_px - dist_px == 0.0) || !(angle_deg >= 0.0 && angle_deg <= 90.0) || !(min_overlap >= 0.0 && min_overlap <= 1.0))
        return h->fail(L3D_ERR_INVALID, "set_support: dist_px must be finite and not negative, angle_deg in [0, 90], min_overlap in [0, 1]");
    if (h->node) return l3d_line3d_set_support(rank0(h), on, dist_px, angle_deg, min_overlap);
    h->support_on = on != 0; h->support_dist_px = dist_px; h->support_angle_deg = angle_deg; h->support_min_overlap = min_overlap;
    return L3D_OK;
}
int l3d_line3d_get_support(const l3d_line3d* h, int64_t* counts, int32_t* per_line)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_support(rank0(h), counts, per_line);
    if (!h->support_valid || !h->result_valid || h->support_per_line.size() != 4 * h->result.size())
        return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "get_support: the last finish ran without the support");
    if (counts) memcpy(counts, h->support_counts, sizeof(h->support_counts));
    if (per_line && !h->support_per_line.empty()) memcpy(per_line, h->support_per_line.data(), h->support_per_line.size() * 4);
    return L3D_OK;
}
int l3d_line3d_gather_support(l3d_line3d* h, const l3d_support_params* params, l3d_line_support** records, int64_t* line_start, int32_t* line_views, int64_t* counts)
{
    if (!h) return L3D_ERR_INVALID;
    if (!records || !line_start || !counts) return h->fail(L3D_ERR_INVALID, "gather_support: a null output pointer");
    *records = nullptr;
    L* owner = h->node ? rank0(h) : h;
    l3d_support_params prm;
    if (params) prm = *params;
    else { prm.dist_px = 3.0; prm.cos_min = std::cos(5.0 * 3.14159265358979323846 / 180.0); prm.min_overlap = 0.5; prm.near_z = 1e-6; prm.margin = 3.0; }
    std::vector<l3d_line_support> rec;
    std::vector<int64_t> start;
    std::vector<int32_t> views;
    const int rc = support_gather(owner, prm, rec, start, views, counts);
    if (rc != L3D_OK) return owner == h ? rc : h->fail(rc, owner->err);
    l3d_line_support* o = static_cast<l3d_line_support*>(malloc((rec.size() + 1) * sizeof(l3d_line_support)));      // (one spare record)
    if (!o) return h->fail(L3D_ERR_NOMEM, "malloc");
    if (!rec.empty()) memcpy(o, rec.data(), rec.size() * sizeof(l3d_line_support));
    memcpy(line_start, start.data(), start.size() * 8);
    if (line_views && !views.empty()) memcpy(line_views, views.data(), views.size() * 4);
    *records = o;
    return L3D_OK;
}
// the junctions of the result's lines (junction_result, line3d_host_finish.cpp).  A node object runs them on rank 0, which holds the result
int l3d_line3d_set_junctions(l3d_line3d* h, int on, double dist_px, double ext_px, double angle_min_deg, double max_ext_rel, int snap)
{
    if (!h) return L3D_ERR_INVALID;
    const auto finite_nonneg = [](double x) { return x >= 0.0 && x - x == 0.0; };
    if (!finite_nonneg(dist_px) || !finite_nonneg(ext_px) || !(angle_min_deg > 0.0 && angle_min_deg <= 90.0) || !(max_ext_rel >= 0.0 && max_ext_rel <= 0.5))
        return h->fail(L3D_ERR_INVALID, "set_junctions: dist_px and ext_px must be finite and not negative, angle_min_deg in (0, 90], max_ext_rel in [0, 0.5]");
    if (h->node) return l3d_line3d_set_junctions(rank0(h), on, dist_px, ext_px, angle_min_deg, max_ext_rel, snap);
    h->junc_on = on != 0; h->junc_dist_px = dist_px; h->junc_ext_px = ext_px; h->junc_angle_min_deg = angle_min_deg; h->junc_max_ext_rel = max_ext_rel; h->junc_snap = snap != 0;
    return L3D_OK;
}
int l3d_line3d_get_junctions(const l3d_line3d* h, l3d_junction_vertex** vertices, int* n_vertices, int32_t* per_line, int32_t* counts)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_junctions(rank0(h), vertices, n_vertices, per_line, counts);
    if (vertices) *vertices = nullptr;
    if (n_vertices) *n_vertices = 0;
    if (!h->junc_valid || !h->result_valid || h->junc_per_line.size() != 4 * h->result.size())
        return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "get_junctions: the last finish ran without the junctions");
    if (vertices) {
        l3d_junction_vertex* o = static_cast<l3d_junction_vertex*>(malloc((h->junc_vertices.size() + 1) * sizeof(l3d_junction_vertex)));     // (one spare vertex)
        if (!o) return const_cast<L*>(h)->fail(L3D_ERR_NOMEM, "malloc");
        if (!h->junc_vertices.empty()) memcpy(o, h->junc_vertices.data(), h->junc_vertices.size() * sizeof(l3d_junction_vertex));
        *vertices = o;
    }
    if (n_vertices) *n_vertices = (int)h->junc_vertices.size();
    if (per_line && !h->junc_per_line.empty()) memcpy(per_line, h->junc_per_line.data(), h->junc_per_line.size() * 4);
    if (counts) memcpy(counts, h->junc_counts, sizeof(h->junc_counts));
    return L3D_OK;
}
// the result as a Wavefront OBJ wireframe: the vertices of the last finish's junctions first (none without them), then every line as a group of its own
int l3d_line3d_save_wireframe(const l3d_line3d* h, const char* filename)
{
    if (h && h->node) return l3d_line3d_save_wireframe(rank0(h), filename);
    if (!h || !filename) return L3D_ERR_INVALID;
    if (!h->result_valid) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_wireframe: no result");
    const bool shared = h->junc_valid && h->junc_per_line.size() == 4 * h->result.size();
    FILE* f = fopen(filename, "w");
    if (!f) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_wireframe: the file cannot be opened");
    long long next = 1;
    if (shared)
        for (const l3d_junction_vertex& v : h->junc_vertices) { fprintf(f, "v %.17g %.17g %.17g\n", v.X[0], v.X[1], v.X[2]); ++next; }
    for (size_t l = 0; l < h->result.size(); ++l) {
        const auto& segs = h->result[l].segs3D;
        fprintf(f, "g line_%zu\n", l);
        for (size_t k = 0; k < segs.size(); ++k) {
            long long ab[2];
            for (int e = 0; e < 2; ++e) {
                const int32_t vx = shared && ((e == 0 && k == 0) || (e == 1 && k + 1 == segs.size())) ? h->junc_per_line[4 * l + (size_t)e] : -1;
                if (vx >= 0) { ab[e] = vx + 1; continue; }
                const V3& p = e == 0 ? segs[k].first : segs[k].second;
                fprintf(f, "v %.17g %.17g %.17g\n", p.x, p.y, p.z);
                ab[e] = next++;
            }
            fprintf(f, "l %lld %lld\n", ab[0], ab[1]);
        }
    }
    const bool ok = ferror(f) == 0;
    return (fclose(f) == 0 && ok) ? L3D_OK : const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_wireframe: the file could not be written");
}
// the planes of the result's lines (plane_result, line3d_host_finish.cpp).  A node object runs them on rank 0, which holds the result
int l3d_line3d_set_planes(l3d_line3d* h, int on, double dist_px, double angle_deg, int min_lines)
{
    if (!h) return L3D_ERR_INVALID;
    if (!(dist_px >= 0.0 && dist_px - dist_px == 0.0) || !(angle_deg >= 0.0 && angle_deg < 90.0) || min_lines < 2)
        return h->fail(L3D_ERR_INVALID, "set_planes: dist_px must be finite and not negative, angle_deg in [0, 90), min_lines at least 2");
    if (h->node) return l3d_line3d_set_planes(rank0(h), on, dist_px, angle_deg, min_lines);
    h->plane_on = on != 0; h->plane_dist_px = dist_px; h->plane_angle_deg = angle_deg; h->plane_min_lines = min_lines;
    return L3D_OK;
}
int l3d_line3d_get_planes(const l3d_line3d* h, l3d_plane** planes, int* n_planes, l3d_plane_member** members, int* n_members, int32_t* per_line, int32_t* counts)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_planes(rank0(h), planes, n_planes, members, n_members, per_line, counts);
    if (planes) *planes = nullptr;
    if (n_planes) *n_planes = 0;
    if (members) *members = nullptr;
    if (n_members) *n_members = 0;
    if (!h->plane_valid || !h->result_valid || h->plane_per_line.size() != h->result.size())
        return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "get_planes: the last finish ran without the planes");
    l3d_plane* op = nullptr; l3d_plane_member* om = nullptr;
    if (planes) {
        op = static_cast<l3d_plane*>(malloc((h->plane_list.size() + 1) * sizeof(l3d_plane)));                       // (one spare record)
        if (!op) return const_cast<L*>(h)->fail(L3D_ERR_NOMEM, "malloc");
        if (!h->plane_list.empty()) memcpy(op, h->plane_list.data(), h->plane_list.size() * sizeof(l3d_plane));
    }
    if (members) {
        om = static_cast<l3d_plane_member*>(malloc((h->plane_members.size() + 1) * sizeof(l3d_plane_member)));
        if (!om) { free(op); return const_cast<L*>(h)->fail(L3D_ERR_NOMEM, "malloc"); }
        if (!h->plane_members.empty()) memcpy(om, h->plane_members.data(), h->plane_members.size() * sizeof(l3d_plane_member));
    }
    if (planes) *planes = op;
    if (members) *members = om;
    if (n_planes) *n_planes = (int)h->plane_list.size();
    if (n_members) *n_members = (int)h->plane_members.size();
    if (per_line && !h->plane_per_line.empty()) memcpy(per_line, h->plane_per_line.data(), h->plane_per_line.size() * 4);
    if (counts) memcpy(counts, h->plane_counts, sizeof(h->plane_counts));
    return L3D_OK;
}
// the planes of the last finish as a Wavefront OBJ: per plane a group of the four corners of its rectangle, O + a u + b v, and one face
int l3d_line3d_save_planes(const l3d_line3d* h, const char* filename)
{
    if (h && h->node) return l3d_line3d_save_planes(rank0(h), filename);
    if (!h || !filename) return L3D_ERR_INVALID;
    if (!h->plane_valid || !h->result_valid) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_planes: the last finish ran without the planes");
    FILE* f = fopen(filename, "w");
    if (!f) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_planes: the file cannot be opened");
    long long next = 1;
    for (size_t k = 0; k < h->plane_list.size(); ++k) {
        const l3d_plane& p = h->plane_list[k];
        fprintf(f, "g plane_%zu\n", k);
        const int ia[4] = { 0, 1, 1, 0 }, ib[4] = { 2, 2, 3, 3 };
        for (int e = 0; e < 4; ++e) {
            double X[3];
            for (int d = 0; d < 3; ++d) X[d] = ((p.c * p.N[d]) + (p.rect[ia[e]] * p.u[d])) + (p.rect[ib[e]] * p.v[d]);
            fprintf(f, "v %.17g %.17g %.17g\n", X[0], X[1], X[2]);
        }
        fprintf(f, "f %lld %lld %lld %lld\n", next, next + 1, next + 2, next + 3);
        next += 4;
    }
    const bool ok = ferror(f) == 0;
    return (fclose(f) == 0 && ok) ? L3D_OK : const_cast<L*>(h)->fail(L3D_ERR_INVALID, "save_planes: the file could not be written");
}
// where the world point links are filed ("CO-VISIBILITY"): 0 on the host as each view is added, 1 by prepare() on the device.  A node object: every rank
// takes the setting, rank 0 counts
int l3d_line3d_set_covisibility(l3d_line3d* h, int mode)
{
    if (!h) return L3D_ERR_INVALID;
    if (mode != 0 && mode != 1) return h->fail(L3D_ERR_INVALID, "set_covisibility: 0 (links filed on the host as views are added) or 1 (counted on the device by prepare)");
    if (l3d_line3d_num_cameras(h) > 0) return h->fail(L3D_ERR_INVALID, "set_covisibility: the object holds views (reset first)");
    if (h->node) return node_each(h, [mode](L* r) { return l3d_line3d_set_covisibility(r, mode); });
    h->covis_mode = mode;
    return L3D_OK;
}
int l3d_line3d_covisibility_path(const l3d_line3d* h)
{
    if (!h) return -1;
    return h->node ? rank0(h)->covis_path : h->covis_path;
}
// what prepare() chose (findVisualNeighbors): a view's neighbours, ascending, and its similarities, ascending by the other view
int l3d_line3d_get_neighbors(l3d_line3d* h, uint32_t view_id, uint32_t* ids, int cap, int* n)
{
    if (!h || !n) return L3D_ERR_INVALID;
    *n = 0;
    if (h->node) {
        const int rc = l3d_line3d_get_neighbors(rank0(h), view_id, ids, cap, n);
        return rc ? h->fail(rc, rank0(h)->err) : rc;
    }
    if (!h->prepared) return h->fail(L3D_ERR_INVALID, "get_neighbors: prepare first");
    if (!h->find_view(view_id)) return h->fail(L3D_ERR_INVALID, "get_neighbors: unknown view");
    auto it = h->visual_neighbors.find(view_id);
    if (it == h->visual_neighbors.end()) return L3D_OK;
    *n = (int)it->second.size();
    if (ids) for (int i = 0; i < *n && i < cap; ++i) ids[i] = it->second[(size_t)i];
    return L3D_OK;
}
int l3d_line3d_get_view_similarities(l3d_line3d* h, uint32_t view_id, uint32_t* ids, float* sims, int cap, int* n)
{
    if (!h || !n) return L3D_ERR_INVALID;
    *n = 0;
    if (h->node) {
        const int rc = l3d_line3d_get_view_similarities(rank0(h), view_id, ids, sims, cap, n);
        return rc ? h->fail(rc, rank0(h)->err) : rc;
    }
    if (!h->prepared) return h->fail(L3D_ERR_INVALID, "get_view_similarities: prepare first");
    if (!h->find_view(view_id)) return h->fail(L3D_ERR_INVALID, "get_view_similarities: unknown view");
    auto it = h->view_similarities.find(view_id);
    if (it == h->view_similarities.end()) return L3D_OK;
    int i = 0;
    for (auto& kv : it->second) {
        if (i < cap) { if (ids) ids[i] = kv.first; if (sims) sims[i] = kv.second; }
        ++i;
    }
    *n = i;
    return L3D_OK;
}
int l3d_line3d_get_refinement(const l3d_line3d* h, double* rms_before, double* rms_after, int32_t* iterations, int32_t* status)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_refinement(rank0(h), rms_before, rms_after, iterations, status);
    if (!h->refine_valid || h->ref_status.size() != h->result.size()) return const_cast<L*>(h)->fail(L3D_ERR_INVALID, "get_refinement: the last finish ran without the refinement");
    const size_t n = h->result.size();
    if (n && rms_before) memcpy(rms_before, h->ref_rms_before.data(), n * 8);
    if (n && rms_after) memcpy(rms_after, h->ref_rms_after.data(), n * 8);
    if (n && iterations) memcpy(iterations, h->ref_iterations.data(), n * 4);
    if (n && status) memcpy(status, h->ref_status.data(), n * 4);
    return L3D_OK;
}
// inspection (tests): what a refinement of the CURRENT result would be fed with -- counts[3] = lines, members, cameras; then (any may be NULL) group_start
// (lines + 1), member_cam, member_seg (4 each), member_pts (6 each), cameras (12 each), and Line3D::inverseTransform as transform[13] = Rinv (9), scale_inv, tneg (3)
int l3d_line3d_refinement_input(l3d_line3d* h, int32_t* counts, int32_t* group_start, int32_t* member_cam, float* member_seg, double* member_pts, double* cameras, double* transform)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_refinement_input(rank0(h), counts, group_start, member_cam, member_seg, member_pts, cameras, transform);
    RefineInput in;
    if (const int rc = refine_input(h, in)) return rc;
    const size_t nl = h->result.size(), nm = (size_t)in.gstart[nl], nv = h->vlist.size();
    if (counts) { counts[0] = (int32_t)nl; counts[1] = (int32_t)nm; counts[2] = (int32_t)nv; }
    if (group_start) memcpy(group_start, in.gstart.data(), (nl + 1) * 4);
    if (member_cam && nm) memcpy(member_cam, in.mcam.data(), nm * 4);
    if (member_seg && nm) memcpy(member_seg, in.mseg.data(), nm * 16);
    if (member_pts && nm) memcpy(member_pts, in.mpts.data(), nm * 48);
    if (cameras && nv) memcpy(cameras, in.cameras.data(), nv * 96);
    if (transform) { memcpy(transform, h->transf_Rinv.m, 72); transform[9] = h->transf_scale_inv; transform[10] = h->transf_tneg.x; transform[11] = h->transf_tneg.y; transform[12] = h->transf_tneg.z; }
    return L3D_OK;
}
// Line3D::compute3Dmodel, line3D.cc:345-374
int l3d_line3d_compute3Dmodel(l3d_line3d* h, int perform_diffusion)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_compute(h, perform_diffusion);
    int rc = prepare(h);
    if (!rc) rc = match_views_reported(h);
    if (!rc) rc = l3d_line3d_finish(h, perform_diffusion);
    return rc;
}

// ---- step-wise matching (multi-GPU: every rank computes a source-segment range of each view, the
// kept lists are all-gathered, every rank commits the same merged list) ---------------------------
int l3d_line3d_match_begin(l3d_line3d* h, int* n_order)
{
    if (h && h->node) return node_refuse(h, "match_begin");
    if (!h || !h->prepared) return h ? h->fail(L3D_ERR_INVALID, "prepare first") : L3D_ERR_INVALID;
    match_begin(h);
    if (n_order) *n_order = (int)h->order.size();
    return L3D_OK;
}
int l3d_line3d_match_order(l3d_line3d* h, uint32_t* ids, int* n_segments)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "match_order");
    for (size_t i = 0; i < h->order.size(); ++i) { if (ids) ids[i] = h->order[i]; if (n_segments) n_segments[i] = h->views[h->order[i]].S(); }
    return L3D_OK;
}
// number of neighbours still to be matched from this view (line3D.cc:732-736); 0 = the early-return case
int l3d_line3d_view_num_to_be_matched(l3d_line3d* h, uint32_t view_id)
{
    if (!h) return -1;
    if (h->node) { node_refuse(h, "view_num_to_be_matched"); return -1; }
    auto it = h->visual_neighbors.find(view_id);
    if (it == h->visual_neighbors.end()) return -1;
    int n = 0;
    for (uint32_t nb : it->second) if (!h->matched.count(((uint64_t)view_id << 32) | nb)) ++n;
    return n;
}
int l3d_line3d_match_view_compute(l3d_line3d* h, uint32_t view_id, int seg_begin, int seg_end,
                                  l3d_match** out, int* n_out, float* median, float** best, int* n_best)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "match_view_compute");
    View* v = h->find_view(view_id);
    if (!v) return h->fail(L3D_ERR_INVALID, "unknown view");
    return compute_view(h, *v, seg_begin, seg_end, out, n_out, median, best, n_best);
}
// best_depths: the merged depth pairs of all ranges (2*n_best floats); pass n_best < 0 to use `median` as is
int l3d_line3d_match_view_commit(l3d_line3d* h, uint32_t view_id, const l3d_match* matches, int n,
                                 const float* best_depths, int n_best, float median)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "match_view_commit");
    View* v = h->find_view(view_id);
    if (!v) return h->fail(L3D_ERR_INVALID, "unknown view");
    if (n_best >= 0) {
        median = -1.0f;                                    // cudawrapper.cu:1066-1073
        if (n_best > 0) {
            std::vector<float> d(best_depths, best_depths + (size_t)n_best * 2);
            std::sort(d.begin(), d.end());
            median = d[d.size() / 2];
        }
    }
    h->stat_last_tbm = l3d_line3d_view_num_to_be_matched(h, view_id);
    commit_view(h, *v, matches, n, median);
    return L3D_OK;
}
// ---- matchViews as the resident chain sharded over ranks (one process per GPU; see include/line3d_amd.h) -----------
int l3d_line3d_shard_open(l3d_line3d* h, int rank, int world, int slot_records, int* n_views, size_t* slot_bytes)
{
    if (h && h->node) return node_refuse(h, "shard_open");
    if (!h || !h->prepared) return h ? h->fail(L3D_ERR_INVALID, "prepare first") : L3D_ERR_INVALID;
    if (h->shard_plan_) return h->fail(L3D_ERR_INVALID, "a sharded chain is already open");
    match_begin(h);
    ChainPlan* P = get_plan(h);
    if (!P) return h->fail(L3D_ERR_INVALID, "schedule is not static (early-return quirk): use the per-view path");
    P->t0 = now_s();
    int rc = l3d_shard_chain_open(h->ctx, P->cv.data(), (int)P->n, rank, world, slot_records, &P->shard, slot_bytes);
    if (rc) return h->fail(rc, std::string("shard_chain_open: ") + l3d_last_error(h->ctx));
    start_finalizer(h, *P);
    h->shard_plan_ = P;
    if (n_views) *n_views = (int)P->n;
    return L3D_OK;
}
int l3d_line3d_shard_view_verified(l3d_line3d* h, int k)
{
    if (h && h->node) { node_refuse(h, "shard_view_verified"); return -1; }
    if (!h || !h->shard_plan_) return -1;
    ChainPlan* P = static_cast<ChainPlan*>(h->shard_plan_);
    if (k < 0 || (size_t)k >= P->n) return -1;
    return P->n_tbm[(size_t)k] > 0 ? 1 : 0;
}
int l3d_line3d_shard_enqueue(l3d_line3d* h, int k, void* send_slot, const void* gathered_base)
{
    if (h && h->node) return node_refuse(h, "shard_enqueue");
    if (!h || !h->shard_plan_) return L3D_ERR_INVALID;
    int rc = l3d_shard_chain_enqueue(static_cast<ChainPlan*>(h->shard_plan_)->shard, k, send_slot, gathered_base);
    return rc ? h->fail(rc, std::string("shard_chain_enqueue: ") + l3d_last_error(h->ctx)) : L3D_OK;
}
int l3d_line3d_shard_mark(l3d_line3d* h, int k)
{
    if (h && h->node) return node_refuse(h, "shard_mark");
    if (!h || !h->shard_plan_) return L3D_ERR_INVALID;
    return l3d_shard_chain_mark(static_cast<ChainPlan*>(h->shard_plan_)->shard, k);
}
// host bookkeeping of view k on this rank (optional per rank; views must be fetched in order)
int l3d_line3d_shard_fetch(l3d_line3d* h, int k)
{
    if (h && h->node) return node_refuse(h, "shard_fetch");
    if (!h || !h->shard_plan_) return L3D_ERR_INVALID;
    ChainPlan* P = static_cast<ChainPlan*>(h->shard_plan_);
    int rc = l3d_shard_chain_fetch(P->shard, k, chain_callback, &P->user);
    return rc ? h->fail(rc, std::string("shard_chain_fetch: ") + l3d_last_error(h->ctx)) : L3D_OK;
}
// committed != 0: this rank fetched every view -> its host state is finalised (finish() may follow)
int l3d_line3d_shard_close(l3d_line3d* h, int committed)
{
    if (h && h->node) return node_refuse(h, "shard_close");
    if (!h || !h->shard_plan_) return L3D_ERR_INVALID;
    ChainPlan* P = static_cast<ChainPlan*>(h->shard_plan_);
    int rc = l3d_shard_chain_close(P->shard);
    finish_chain_host(h, *P, committed != 0 && rc == L3D_OK);
    if (h->pot_check_failed && rc == L3D_OK) rc = h->fail(L3D_ERR_INVALID, "L3D_CHECK_POT: a potential-correspondence list is not in normal form");
    double st[4];
    l3d_last_stats(h->ctx, st);
    h->stat_pairs += st[0];
    h->stat_raw += st[1];
    h->t_match = now_s() - P->t0;
    P->shard = nullptr;
    h->shard_plan_ = nullptr;
    return rc;
}
int l3d_line3d_shard_run(l3d_line3d* h, int rank, int world, int slot_records, l3d_exchange_fn exchange, void* exchange_user, int commit,
                         const void** gathered_out, size_t* slot_bytes_out)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "shard_run");
    // A capacity failure is a verdict all ranks share (l3d_shard_chain_info): every rank reopens with the same, larger
    // capacities and runs again -- the bookkeeping of the failed attempt is dropped by the reopen (match_begin).
    size_t cand_cap_next = 0, arena_cap_next = h->shard_arena_cap_hint;
    int rc = L3D_OK;
    // sizes a capacity verdict of an earlier pass of this job taught us (identical on every rank: the verdict is shared)
    if (h->shard_world_seen == world) { slot_records = std::max(slot_records, h->shard_slot_records_seen); cand_cap_next = h->shard_cand_cap_seen; }
    else { h->shard_world_seen = world; h->shard_slot_records_seen = 0; h->shard_cand_cap_seen = 0; }
    for (int attempt = 0; attempt < 4; ++attempt) {
        int n_views = 0;
        size_t slot_bytes = 0;
        const double t0 = now_s();
        if (cand_cap_next) l3d_set_chain_capacities(h->ctx, cand_cap_next, 0);
        rc = l3d_line3d_shard_open(h, rank, world, slot_records, &n_views, &slot_bytes);
        if (cand_cap_next) l3d_set_chain_capacities(h->ctx, 0, 0);
        if (rc) return rc;
        const double t1 = now_s();
        ChainPlan* P = static_cast<ChainPlan*>(h->shard_plan_);
        const bool host_commit = commit == 1;
        if (commit == 3) {       // partitioned: this rank keeps what its block of views needs (l3d_shard_chain_partition), nothing else
            // (options part_vrank / part_vworld at world 1: the block another job's rank would own -- one rank's share of a job too big for one GPU, on one GPU)
            const int vw = world == 1 && hopt(h).part_vworld > 0 ? hopt(h).part_vworld : world, vr = vw != world ? std::max(0, std::min(hopt(h).part_vrank, vw - 1)) : rank;
            rc = l3d_shard_chain_partition(P->shard, (int)(((long long)n_views * vr) / vw), (int)(((long long)n_views * (vr + 1)) / vw));
            if (rc) { const std::string m = std::string("shard_chain_partition: ") + l3d_last_error(h->ctx); l3d_line3d_shard_close(h, 0); return h->fail(rc, m); }
        }
        if (arena_cap_next) l3d_set_chain_capacities(h->ctx, 0, arena_cap_next);          // (the compact arena of the slot ring: read by the run)
        rc = l3d_shard_chain_run(P->shard, exchange, exchange_user, host_commit ? chain_callback : nullptr, host_commit ? &P->user : nullptr);
        if (arena_cap_next) l3d_set_chain_capacities(h->ctx, 0, 0);
        std::string msg = rc ? std::string("shard_chain_run: ") + l3d_last_error(h->ctx) : std::string();
        if (rc == L3D_OK && (commit == 2 || commit == 3)) {
            // commit on the device: this rank builds matchViews' products from the gathered slots (every rank may), no list goes to the host
            std::vector<uint32_t> ids; std::vector<int32_t> base;
            dense_map(h, ids, base);
            l3d_dense_map map;
            map.n_views = (int32_t)ids.size(); map.view_ids = ids.data(); map.seg_base = base.data();
            h->chain_summary.assign(P->n, l3d_chain_summary());
            rc = l3d_shard_chain_products(P->shard, &map, h->chain_summary.data(), &h->resident_n_pot);
            if (rc) msg = std::string("shard_chain_products: ") + l3d_last_error(h->ctx);
            else {
                if (commit == 3) { h->partitioned = true; h->part_exchange = exchange; h->part_user = exchange_user; }      // (a share: nothing to check against a host construction)
                rc = adopt_resident_products(h, *P);
                if (rc) { msg = h->err; h->partitioned = false; }
            }
        }
        size_t cand_cap = 0; int bits = 0, max_cand = 0, max_kept = 0, recs = slot_records;
        l3d_shard_chain_info(P->shard, &cand_cap, &recs, &bits, &max_cand, &max_kept);
        const long long P_shard_arena = l3d_shard_chain_arena_needed(P->shard);
        if (gathered_out) *gathered_out = l3d_shard_chain_gathered(P->shard);
        if (slot_bytes_out) *slot_bytes_out = slot_bytes;
        const double t2 = now_s();
        const int rc2 = l3d_line3d_shard_close(h, commit == 1 && rc == L3D_OK);
        if (hopt(h).timing) fprintf(stderr, "[l3d shard_run] open (schedule, tables, arenas) %.2f  run %.2f  close (finalise host state) %.2f ms\n",
                                          (t1 - t0) * 1e3, (t2 - t1) * 1e3, (now_s() - t2) * 1e3);
        if (rc == L3D_OK) return rc2;
        h->fail(rc, msg);
        if (hopt(h).timing) fprintf(stderr, "[l3d shard_run] attempt %d failed (%d): %s\n", attempt, rc, msg.c_str());
        if (rc != L3D_ERR_NOMEM) return rc;
        // what the shared verdict asks for (shard_retry, l3d_shard_rule.hpp): nothing a retry would change, or the same, larger capacities on every rank
        const long long room = l3d::shard_room_records(hopt(h).regrow_free_mb);
        const l3d::ShardRetry next = l3d::shard_retry(bits, cand_cap, max_cand, slot_records, max_kept, P_shard_arena, room, exchange == l3d_exchange_replay);
        if (next.refuse_for_room)
            return h->fail(L3D_ERR_NOMEM, "shard_run: the compact arena of this rank needs " + std::to_string(P_shard_arena) + " records, there is room for " + std::to_string(room) + " (" +
                                          std::to_string(hopt(h).regrow_free_mb) + " MB at " + std::to_string(sizeof(l3d_match) + 4) + " B per record)");
        if (!next.retry) return rc;
        if (next.arena_cap_next) arena_cap_next = next.arena_cap_next;
        if (next.cand_cap_next) cand_cap_next = h->shard_cand_cap_seen = next.cand_cap_next;
        if (next.slot_records_next) slot_records = h->shard_slot_records_seen = next.slot_records_next;
    }
    return rc;
}
// matchViews with the VIEWS sharded over the ranks in blocks, each block started cold a few windows early and the speculation verified
// (l3d_match_chain_blocks).  *verdict = 0: this rank holds matchViews' products as after the single-GPU resident chain; 1: the speculation
// did not hold on this scene, nothing was committed -- the caller runs l3d_line3d_shard_run (every rank gets the same verdict).
// warmup_views < 0: eight neighbour windows.
static int block_run_impl(l3d_line3d* h, int rank, int world, int warmup_views, l3d_exchange_fn exchange, void* exchange_user, int* verdict, bool partition)
{
    if (!h || !verdict) return L3D_ERR_INVALID;
    *verdict = 1;
    const double t0 = now_s();
    match_begin(h);
    h->partitioned = false;
    ChainPlan* Pp = get_plan(h);
    if (!Pp) return L3D_OK;                               // (a schedule the chain cannot express: the caller's other paths handle it)
    ChainPlan& P = *Pp;
    int window = 1;
    for (size_t k = 0; k < P.n; ++k) for (int si : P.src_idx[k]) window = std::max(window, (int)k - si);
    // (round 4: eight windows -- any miss cost the pass.  Round 5: a block whose speculation fails is re-run warm, all missed blocks at once, so a
    // miss costs one more block time, not the pass.  Still eight: the chain's memory was measured at 3-7 windows (profiles/r4_speculate_*.txt), and on
    // the 512-view scene at 8 ranks a warm-up of 4 windows re-runs 7 blocks, of 6 windows 3, of 8 windows none (profiles/r5_warmup_needed_512.txt) -- what a
    // shorter warm-up saves on every rank (2 windows = 12 views) a single miss gives back five times over (a block = 64 views))
    if (warmup_views < 0) warmup_views = 8 * window;
    std::vector<uint32_t> ids; std::vector<int32_t> base;
    dense_map(h, ids, base);
    l3d_dense_map map;
    map.n_views = (int32_t)ids.size(); map.view_ids = ids.data(); map.seg_base = base.data();
    h->chain_summary.assign(P.n, l3d_chain_summary());
    h->resident_products = false;
    const double t1 = now_s();
    int rc = partition ? l3d_match_chain_partition(h->ctx, P.cv.data(), (int)P.n, &map, h->chain_summary.data(), &h->resident_n_pot, rank, world, warmup_views, window,
                                                   exchange, exchange_user, verdict)
                       : l3d_match_chain_blocks(h->ctx, P.cv.data(), (int)P.n, &map, h->chain_summary.data(), &h->resident_n_pot, rank, world, warmup_views, window,
                                                exchange, exchange_user, verdict);
    h->t_gpu_call += now_s() - t1;
    if (rc) return h->fail(rc, std::string(partition ? "match_chain_partition: " : "match_chain_blocks: ") + l3d_last_error(h->ctx));
    if (*verdict != 0) return L3D_OK;
    h->partitioned = partition;
    h->part_exchange = exchange; h->part_user = exchange_user;
    rc = adopt_resident_products(h, P);
    if (rc) return rc;
    double st[4];
    l3d_last_stats(h->ctx, st);
    h->stat_pairs += st[0];
    h->stat_raw += st[1];
    h->t_match = now_s() - t0;
    return L3D_OK;
}
int l3d_line3d_block_run(l3d_line3d* h, int rank, int world, int warmup_views, l3d_exchange_fn exchange, void* exchange_user, int* verdict)
{
    if (h && h->node) return node_refuse(h, "block_run");
    return block_run_impl(h, rank, world, warmup_views, exchange, exchange_user, verdict, false);
}
// matchViews sharded by blocks of views with NOTHING replicated (l3d_match_chain_partition): this rank holds its block's share of the kept records
// and of matchViews' products; the rest of compute3Dmodel is collective -- l3d_line3d_finish_sharded on every rank
int l3d_line3d_partition_run(l3d_line3d* h, int rank, int world, int warmup_views, l3d_exchange_fn exchange, void* exchange_user, int* verdict)
{
    if (h && h->node) return node_refuse(h, "partition_run");
    return block_run_impl(h, rank, world, warmup_views, exchange, exchange_user, verdict, true);
}
// Line3D::compute3Dmodel's tail after l3d_line3d_partition_run, on every rank of the job: greedy selection on the views this rank holds, the affinity
// fill sharded by source key (l3d_affinity_fill_sharded: five small all-gathers), then -- replicas, every rank from the same edge list -- diffusion,
// clustering, line fit.  Every rank ends with the whole result.
int l3d_line3d_finish_sharded(l3d_line3d* h, int perform_diffusion, l3d_exchange_fn exchange, void* exchange_user)
{
    if (h && h->node) return node_refuse(h, "finish_sharded");
    if (!h || !h->prepared) return h ? h->fail(L3D_ERR_INVALID, "prepare first") : L3D_ERR_INVALID;
    if (!h->partitioned || !h->resident_products) return h->fail(L3D_ERR_INVALID, "finish_sharded: matchViews did not run partitioned (l3d_line3d_partition_run)");
    if (exchange) { h->part_exchange = exchange; h->part_user = exchange_user; }
    if (!h->part_exchange) return h->fail(L3D_ERR_INVALID, "finish_sharded: no exchange");
    return l3d_line3d_finish(h, perform_diffusion);
}
// how the last l3d_line3d_match_views ran: 0 = the resident chain with its products on the device, 1 = the chain with host bookkeeping, 2 = per-view
// seam calls because the caller asked (l3d_line3d_set_sync_matching), 3 = per-view seam calls because the schedule is not static (-1: not yet)
int l3d_line3d_match_path(const l3d_line3d* h) { return !h ? -1 : h->node ? l3d_line3d_match_path(rank0(h)) : h->last_match_path; }
int l3d_line3d_match_end(l3d_line3d* h)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "match_end");
    finalize_matching(h);
    return L3D_OK;
}

// performClustering (clustering.h:125, clustering.cc:6-47) as a host entry point: labels[k] = find(k)
int l3d_perform_clustering(const l3d_edge* edges, int n_edges, int num_nodes, float c, int32_t* labels)
{
    if (n_edges < 0 || num_nodes < 0 || (n_edges > 0 && !edges) || (num_nodes > 0 && !labels)) return L3D_ERR_INVALID;
    for (int k = 0; k < n_edges; ++k)
        if (edges[k].i < 0 || edges[k].i >= num_nodes || edges[k].j < 0 || edges[k].j >= num_nodes) return L3D_ERR_INVALID;
    std::vector<int> lab;
    perform_clustering(edges, (size_t)n_edges, num_nodes, c, lab);
    for (int k = 0; k < num_nodes; ++k) labels[k] = lab[(size_t)k];
    return L3D_OK;
}

// ---- results ---------------------------------------------------------------------------------
int l3d_line3d_result_sizes(const l3d_line3d* h, int* n_lines, int* n_seg3d, int* n_seg2d)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_result_sizes(rank0(h), n_lines, n_seg3d, n_seg2d);
    int a = 0, b = 0;
    for (auto& l : h->result) { a += (int)l.segs3D.size(); b += (int)l.segs2D.size(); }
    if (n_lines) *n_lines = (int)h->result.size();
    if (n_seg3d) *n_seg3d = a;
    if (n_seg2d) *n_seg2d = b;
    return L3D_OK;
}
// per line: counts; seg3d: 6 doubles each (P1,P2); seg2d: (camID, segID) pairs  -- Line3D::getResult
int l3d_line3d_get_result(const l3d_line3d* h, int* line_n3d, int* line_n2d, double* seg3d, uint32_t* seg2d)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_result(rank0(h), line_n3d, line_n2d, seg3d, seg2d);
    size_t a = 0, b = 0, li = 0;
    for (auto& l : h->result) {
        line_n3d[li] = (int)l.segs3D.size(); line_n2d[li] = (int)l.segs2D.size(); ++li;
        for (auto& s : l.segs3D) { seg3d[a++] = s.first.x; seg3d[a++] = s.first.y; seg3d[a++] = s.first.z; seg3d[a++] = s.second.x; seg3d[a++] = s.second.y; seg3d[a++] = s.second.z; }
        for (Key k : l.segs2D) { seg2d[b++] = kcam(k); seg2d[b++] = kseg(k); }
    }
    return L3D_OK;
}
// Line3D::getSegment2D, line3D.cc:2004-2013
// Line3D::save3DLinesAsSTL / save3DLinesAsTXT (line3D.cc:384-473; TXT format: README.txt:177-185) for the current result.
// Numbers are formatted the way the reference formats them: "%e" in the STL file, the stream default (6 significant
// digits, "%g") in the TXT file; lines without 3-D segments are skipped in the TXT file only.
int l3d_line3d_save_result(const l3d_line3d* h, const char* filename, int format)
{
    if (h && h->node) return l3d_line3d_save_result(rank0(h), filename, format);
    if (!h || !filename || (format != L3D_FORMAT_STL && format != L3D_FORMAT_TXT)) return L3D_ERR_INVALID;
    FILE* f = fopen(filename, "w");
    if (!f) return L3D_ERR_INVALID;
    if (format == L3D_FORMAT_STL) {
        fprintf(f, "solid lineModel\n");
        for (auto& l : h->result)
            for (auto& sg : l.segs3D) {
                fprintf(f, " facet normal 1.0e+000 0.0e+000 0.0e+000\n  outer loop\n");
                fprintf(f, "   vertex %e %e %e\n", sg.first.x, sg.first.y, sg.first.z);
                fprintf(f, "   vertex %e %e %e\n", sg.second.x, sg.second.y, sg.second.z);
                fprintf(f, "   vertex %e %e %e\n", sg.first.x, sg.first.y, sg.first.z);
                fprintf(f, "  endloop\n endfacet\n");
            }
        fprintf(f, "endsolid lineModel\n");
    } else {
        for (auto& l : h->result) {
            if (l.segs3D.empty()) continue;
            fprintf(f, "%zu ", l.segs3D.size());
            for (auto& sg : l.segs3D) fprintf(f, "%g %g %g %g %g %g ", sg.first.x, sg.first.y, sg.first.z, sg.second.x, sg.second.y, sg.second.z);
            fprintf(f, "%zu ", l.segs2D.size());
            for (Key k : l.segs2D) {
                float c[4] = { 0, 0, 0, 0 };
                (void)l3d_line3d_get_segment2D(h, kcam(k), kseg(k), c);
                fprintf(f, "%u %u %g %g %g %g ", kcam(k), kseg(k), (double)c[0], (double)c[1], (double)c[2], (double)c[3]);
            }
            fprintf(f, "\n");
        }
    }
    return fclose(f) == 0 ? L3D_OK : L3D_ERR_INVALID;
}

int l3d_line3d_get_segment2D(const l3d_line3d* h, uint32_t cam, uint32_t seg, float out[4])
{
    if (out) out[0] = out[1] = out[2] = out[3] = 0.0f;        // zeroed before any early return
    if (!h || !out) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_get_segment2D(rank0(h), cam, seg, out);
    auto it = h->views.find(cam);
    if (it == h->views.end() || seg >= (uint32_t)it->second.S()) return L3D_ERR_INVALID;
    memcpy(out, &it->second.segs[(size_t)seg * 4], 16);
    return L3D_OK;
}

// ---- the result over the views ("PROJECTION AND OVERLAYS", 3): projected through l3d_project_lines, drawn through l3d_draw_segments, on the object's
// context (a node object: rank 0's, which holds the result)
static const unsigned char kDefaultPalette[12 * 4] = { 230, 25, 75, 255, 60, 180, 75, 255, 255, 225, 25, 255, 0, 130, 200, 255, 245, 130, 48, 255, 145, 30, 180, 255,
                                                       70, 240, 240, 255, 240, 50, 230, 255, 210, 245, 60, 255, 250, 190, 212, 255, 0, 128, 128, 255, 170, 110, 40, 255 };
const unsigned char* l3d_default_palette(void) { return kDefaultPalette; }

// owner: the object that holds the result.  The outputs are std::vectors here; the exported call packs them
static int project_result_core(L* owner, const uint32_t* view_ids, int n_views, const l3d_camera* cameras, int select, double near_z, double margin,
                               std::vector<float>& seg2d, std::vector<int32_t>& seg_index, std::vector<int32_t>& line_index, std::vector<unsigned char>& flags,
                               int64_t* cam_start)
{
    if (!owner->result_valid) return owner->fail(L3D_ERR_INVALID, "project_result: no result yet (compute3Dmodel first)");
    if (!owner->ctx) return owner->fail(L3D_ERR_INVALID, "project_result: no device context");
    if (n_views < 0 || !cam_start) return owner->fail(L3D_ERR_INVALID, "project_result: bad argument");
    if (select != L3D_SELECT_ALL && select != L3D_SELECT_OBSERVED) return owner->fail(L3D_ERR_INVALID, "project_result: select must be L3D_SELECT_ALL or L3D_SELECT_OBSERVED");
    if (n_views > 0 && !view_ids && (!cameras || select == L3D_SELECT_OBSERVED)) return owner->fail(L3D_ERR_INVALID, "project_result: view ids are needed (no cameras given, or L3D_SELECT_OBSERVED)");
    std::vector<l3d_camera> own;
    if (!cameras) {
        own.reserve((size_t)n_views);
        for (int k = 0; k < n_views; ++k) {
            const View* v = owner->find_view(view_ids[k]);
            if (!v) return owner->fail(L3D_ERR_INVALID, "project_result: unknown view " + std::to_string(view_ids[k]));
            own.push_back(camera_as_added(*v));
        }
        cameras = own.data();
    } else if (view_ids)
        for (int k = 0; k < n_views; ++k)
            if (!owner->find_view(view_ids[k])) return owner->fail(L3D_ERR_INVALID, "project_result: unknown view " + std::to_string(view_ids[k]));
    // the result's 3-D segments in l3d_line3d_get_result's order, and the line of each
    std::vector<double> seg3d;
    std::vector<int32_t> line_of;
    for (size_t li = 0; li < owner->result.size(); ++li)
        for (auto& s : owner->result[li].segs3D) {
            const double v[6] = { s.first.x, s.first.y, s.first.z, s.second.x, s.second.y, s.second.z };
            seg3d.insert(seg3d.end(), v, v + 6);
            line_of.push_back((int32_t)li);
        }
    float* o = nullptr; int32_t* src = nullptr; unsigned char* fl = nullptr;
    std::vector<int64_t> start((size_t)n_views + 1, 0);
    const int rc = l3d_project_lines(owner->ctx, seg3d.data(), (int)line_of.size(), cameras, n_views, near_z, margin, &o, &src, &fl, start.data());
    if (rc != L3D_OK) return owner->fail(rc, l3d_last_error(owner->ctx));
    seg2d.clear(); seg_index.clear(); line_index.clear(); flags.clear();
    std::vector<char> observed;
    for (int k = 0; k < n_views; ++k) {
        cam_start[k] = (int64_t)seg_index.size();
        if (select == L3D_SELECT_OBSERVED) {                // the lines with a 2-D member in this view
            observed.assign(owner->result.size(), 0);
            for (size_t li = 0; li < owner->result.size(); ++li)
                for (Key key : owner->result[li].segs2D) if (kcam(key) == view_ids[k]) { observed[li] = 1; break; }
        }
        for (int64_t i = start[(size_t)k]; i < start[(size_t)k + 1]; ++i) {
            const int32_t li = line_of[(size_t)src[i]];
            if (select == L3D_SELECT_OBSERVED && !observed[(size_t)li]) continue;
            seg2d.insert(seg2d.end(), o + 4 * i, o + 4 * i + 4);
            seg_index.push_back(src[i]); line_index.push_back(li); flags.push_back(fl[i]);
        }
    }
    cam_start[n_views] = (int64_t)seg_index.size();
    l3d_free(o); l3d_free(src); l3d_free(fl);
    return L3D_OK;
}

int l3d_line3d_project_result(l3d_line3d* h, const uint32_t* view_ids, int n_views, const l3d_camera* cameras, int select, double near_z, double margin,
                              float** seg2d, int32_t** seg_index, int32_t** line_index, unsigned char** flags, int64_t* cam_start)
{
    if (!h) return L3D_ERR_INVALID;
    if (!seg2d || !seg_index || !line_index || !flags) return h->fail(L3D_ERR_INVALID, "project_result: a null output pointer");
    *seg2d = nullptr; *seg_index = nullptr; *line_index = nullptr; *flags = nullptr;
    L* owner = h->node ? rank0(h) : h;
    std::vector<float> s2; std::vector<int32_t> si, li; std::vector<unsigned char> fl;
    const int rc = project_result_core(owner, view_ids, n_views, cameras, select, near_z, margin, s2, si, li, fl, cam_start);
    if (rc != L3D_OK) return owner == h ? rc : h->fail(rc, owner->err);
    const size_t n = si.size();                         // (one spare element each: an empty result still hands out pointers that l3d_free takes)
    float* a = static_cast<float*>(malloc((n * 4 + 1) * sizeof(float)));
    int32_t* b = static_cast<int32_t*>(malloc((n + 1) * sizeof(int32_t)));
    int32_t* c = static_cast<int32_t*>(malloc((n + 1) * sizeof(int32_t)));
    unsigned char* d = static_cast<unsigned char*>(malloc(n + 1));
    if (!a || !b || !c || !d) { free(a); free(b); free(c); free(d); return h->fail(L3D_ERR_NOMEM, "malloc"); }
    if (n) { memcpy(a, s2.data(), n * 16); memcpy(b, si.data(), n * 4); memcpy(c, li.data(), n * 4); memcpy(d, fl.data(), n); }
    *seg2d = a; *seg_index = b; *line_index = c; *flags = d;
    return L3D_OK;
}

// pixels: the host's (image == nullptr) or a device image's
static int overlay_run(l3d_line3d* h, uint32_t view_id, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const l3d_device_image* image,
                       const l3d_overlay_style* style)
{
    if (!h) return L3D_ERR_INVALID;
    L* owner = h->node ? rank0(h) : h;
    auto refuse = [&](int code, const std::string& m) { if (owner != h) owner->err = m; return h->fail(code, m); };
    if (!owner->result_valid) return refuse(L3D_ERR_INVALID, "overlay: no result yet (compute3Dmodel first)");
    if (!owner->ctx) return refuse(L3D_ERR_INVALID, "overlay: no device context");
    if (!image && !pixels) return refuse(L3D_ERR_INVALID, "overlay: a null pointer");
    const View* v = owner->find_view(view_id);
    if (!v) return refuse(L3D_ERR_INVALID, "overlay: unknown view " + std::to_string(view_id));
    if (image) { width = image->width; height = image->height; }
    if ((unsigned)width != v->width || (unsigned)height != v->height || width < 1 || height < 1)
        return refuse(L3D_ERR_INVALID, "overlay: the image is " + std::to_string(width) + " x " + std::to_string(height) + ", the view " + std::to_string(v->width) + " x " + std::to_string(v->height));
    l3d_overlay_style st;
    if (style) st = *style;
    else {
        memset(&st, 0, sizeof(st));
        st.layers = L3D_LAYER_MEMBERS | L3D_LAYER_MODEL; st.select = L3D_SELECT_OBSERVED; st.by_line = 1; st.opacity = 255;
        st.width_members = 1.0; st.width_model = 2.0; st.near_z = 1e-6;
    }
    if (st.layers < 0 || st.layers > (L3D_LAYER_MEMBERS | L3D_LAYER_MODEL)) return refuse(L3D_ERR_INVALID, "overlay: unknown layers");
    const unsigned char* palette = st.palette ? st.palette : kDefaultPalette;
    const int n_palette = st.palette ? st.n_palette : 12;
    if (st.by_line && n_palette < 1) return refuse(L3D_ERR_INVALID, "overlay: an empty palette");
    auto draw = [&](const std::vector<float>& segs, const std::vector<int32_t>& lines, const unsigned char* fixed, double width_px) {
        std::vector<int32_t> idx;
        if (st.by_line) { idx.resize(lines.size()); for (size_t k = 0; k < lines.size(); ++k) idx[k] = lines[k] % n_palette; }
        const unsigned char* colors = st.by_line ? palette : fixed;
        const int n_colors = st.by_line ? n_palette : 1, n = (int)lines.size();
        const int rc = image ? l3d_draw_segments_device(owner->ctx, image, segs.data(), n, colors, n_colors, st.by_line ? idx.data() : nullptr, width_px, st.opacity)
                             : l3d_draw_segments(owner->ctx, pixels, width, height, channels, row_stride, segs.data(), n, colors, n_colors, st.by_line ? idx.data() : nullptr, width_px, st.opacity);
        return rc == L3D_OK ? rc : refuse(rc, l3d_last_error(owner->ctx));
    };
    if (st.layers & L3D_LAYER_MEMBERS) {
        std::vector<float> segs;
        std::vector<int32_t> lines;
        for (size_t li = 0; li < owner->result.size(); ++li)
            for (Key key : owner->result[li].segs2D)
                if (kcam(key) == view_id && kseg(key) < (uint32_t)v->S()) {
                    segs.insert(segs.end(), &v->segs[(size_t)kseg(key) * 4], &v->segs[(size_t)kseg(key) * 4] + 4);
                    lines.push_back((int32_t)li);
                }
        if (int rc = draw(segs, lines, st.color_members, st.width_members)) return rc;
    }
    if (st.layers & L3D_LAYER_MODEL) {
        std::vector<float> segs; std::vector<int32_t> si, lines; std::vector<unsigned char> fl;
        int64_t start[2];
        const int rc = project_result_core(owner, &view_id, 1, nullptr, st.select, st.near_z, 34.0, segs, si, lines, fl, start);
        if (rc != L3D_OK) return owner == h ? rc : h->fail(rc, owner->err);
        if (int rd = draw(segs, lines, st.color_model, st.width_model)) return rd;
    }
    return L3D_OK;
}

int l3d_line3d_overlay(l3d_line3d* h, uint32_t view_id, unsigned char* pixels, int width, int height, int channels, size_t row_stride, const l3d_overlay_style* style)
{
    return overlay_run(h, view_id, pixels, width, height, channels, row_stride, nullptr, style);
}

int l3d_line3d_overlay_device(l3d_line3d* h, uint32_t view_id, const l3d_device_image* image, const l3d_overlay_style* style)
{
    if (!h) return L3D_ERR_INVALID;
    if (!image) return h->fail(L3D_ERR_INVALID, "overlay: a null pointer");
    return overlay_run(h, view_id, nullptr, 0, 0, 0, 0, image, style);
}

// ---- inspection for tests / bench ----------------------------------------------------------------
int l3d_line3d_set_sync_matching(l3d_line3d* h, int on)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "set_sync_matching");
    h->force_sync = on != 0;
    return L3D_OK;
}
int l3d_line3d_keep_view_matches(l3d_line3d* h, int on)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_each(h, [on](L* r) { return l3d_line3d_keep_view_matches(r, on); });
    h->keep_view_matches = on != 0;
    return L3D_OK;
}
int l3d_line3d_view_matches(const l3d_line3d* h, uint32_t view_id, const l3d_match** m, int* n, float* median)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(const_cast<L*>(h), "view_matches");
    auto it = h->view_matches.find(view_id);
    if (m) *m = it == h->view_matches.end() ? nullptr : it->second.data();
    if (n) *n = it == h->view_matches.end() ? 0 : (int)it->second.size();
    auto vt = h->views.find(view_id);
    if (median && vt != h->views.end()) *median = vt->second.median_depth;
    return L3D_OK;
}
int l3d_line3d_affinity(const l3d_line3d* h, const l3d_edge** A, int* nnz, int* n_nodes)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_affinity(rank0(h), A, nnz, n_nodes);
    if (A) { if (int rc = ensure_edges(const_cast<l3d_line3d*>(h))) return rc; *A = h->A.data(); }
    if (nnz) *nnz = (int)h->n_edges;
    if (n_nodes) *n_nodes = (int)h->local2global.size();
    return L3D_OK;
}
int l3d_line3d_products_sizes(const l3d_line3d* h, int* n_views, int* n_dense, int64_t* n_pot, int* n_hyp)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(const_cast<L*>(h), "products_sizes");
    const bool on = h->resident_products;
    int nd = 0;
    for (const View* v : h->vlist) nd += v->S();
    if (n_views) *n_views = on ? (int)h->vlist.size() : 0;
    if (n_dense) *n_dense = on ? nd : 0;
    if (n_pot) *n_pot = on ? h->resident_n_pot : 0;
    if (n_hyp) *n_hyp = on ? (int)h->hyps.size() : 0;
    return L3D_OK;
}
int l3d_line3d_chain_summary(const l3d_line3d* h, const l3d_chain_summary** summary, int* n)
{
    if (!h || !summary || !n) return L3D_ERR_INVALID;
    if (h->node) {          // (node_compute: the views of every rank's block)
        *summary = h->chain_summary.empty() ? nullptr : h->chain_summary.data();
        *n = (int)h->chain_summary.size();
        return L3D_OK;
    }
    const bool on = h->resident_products;
    *summary = on && !h->chain_summary.empty() ? h->chain_summary.data() : nullptr;
    *n = on ? (int)h->chain_summary.size() : 0;
    return L3D_OK;
}
int l3d_line3d_products_get(l3d_line3d* h, int32_t* seg_base, int64_t* pot_start, int32_t* pot_tgt, l3d_match* best, l3d_hypothesis* hyp, float* score)
{
    if (!h) return L3D_ERR_INVALID;
    if (h->node) return node_refuse(h, "products_get");
    if (!h->resident_products) return h->fail(L3D_ERR_INVALID, "no resident products");
    if (seg_base) { int b = 0; size_t i = 0; for (const View* v : h->vlist) { seg_base[i++] = b; b += v->S(); } seg_base[i] = b; }
    int rc = l3d_chain_products_get(h->ctx, pot_start, pot_tgt, best);
    if (!rc && (hyp || score) && !h->hyps.empty()) rc = l3d_products_hypotheses_get(h->ctx, hyp, score);
    return rc ? h->fail(rc, std::string("products_get: ") + l3d_last_error(h->ctx)) : L3D_OK;
}
/* stats[12]: pairs, raw candidates, kept, #hypotheses, t_match, t_gpu_call, t_commit, t_finalize, t_affinity, t_cluster, #edges, #lines */
int l3d_line3d_stats(const l3d_line3d* h, double* s)
{
    if (!h || !s) return L3D_ERR_INVALID;
    if (h->node) return l3d_line3d_stats(rank0(h), s);
    s[0] = h->stat_pairs; s[1] = h->stat_raw; s[2] = h->stat_kept; s[3] = (double)h->hyps.size();
    s[4] = h->t_match; s[5] = h->t_gpu_call; s[6] = h->t_commit; s[7] = h->t_finalize; s[8] = h->t_affinity; s[9] = h->t_cluster;
    s[10] = (double)h->n_edges; s[11] = (double)h->result.size();
    return L3D_OK;
}

}  // extern "C"
