// corr2d3d.hip -- the deterministic part of SequentialReconstructor::addNextView (SequentialReconstructor.cpp:761-813) behind
// rcn_match_lists_*, rcn_corr_2d3d*, rcn_landmark_attach and rcn_ba_session_attach (include/rcn.h).  gfx950, wave64.
//
// calc2d3dMatches (:643-695) walks, for every candidate c, every landmark and every observation (i, f) of its track in
// triangulatedFeatures order and emits (landmark, g) when featureMatches[(i, c)] maps f -> g.  Each (image, feature)
// belongs to at most one observation of the graph, so the walk can be turned round: walk the match lists of every
// (graph image, candidate) pair and find the observation of (i, f) in a table.  Ordering the hits by flattened
// observation index then gives exactly the reference's order (landmark, then track position):
//   C1 k_corr_index    obs_of[slot(i)][f] = the (smallest) flattened observation index of (i, f); obs_pt[o] = landmark;
//                      in_graph[slot] = the image has an observation
//   C2 k_corr_walk     one workgroup per (graph image slot, candidate of the batch): the list (i, c), or (c, i) read
//                      backwards under mirror; hit[cand][o] = g (dense row over the observations, one writer per
//                      entry: the list is injective), the density cell of g ORed into 32 words per candidate
//   C3 k_corr_count    hits per 4096-entry tile of every row of the batch
//   C4 k_corr_scan     one workgroup: exclusive scan of the tile counts behind the running total of earlier batches
//                      (integer sums: exact in any order); the candidates' offsets fall out of it
//   C5 k_corr_compact  rank = tile offset + thread prefix + position in the thread's 16 entries: (obs_pt[o], g) in
//                      observation order
//   C6 k_corr_final    score = popcount of the 32 words, the out-of-frame counts, the total
// Candidates go through C2-C5 in batches whose hit rows fit the workspace budget (rcn_corr_set_workspace_bytes); the
// batches share one running offset, so the output does not depend on the budget.  No atomic decides a position.
//
// Step 1 of triangulateMatchedLandmarks (:497-512), k_attach_rules / k_attach_taken: per entry (fp64, contraction off,
// camgeom.h reproj_l1) depth > 0, L1 error < max, then the first PASSING entry of every feature wins -- the smallest
// entry index by atomicMin, which is order-independent.
//
// Step 3 of triangulateMatchedLandmarks (:514-553) behind rcn_landmark_ids_* and rcn_new_view_tracks_device (DESIGN.md section
// 25): for every free feature f of the new image v the FIRST registered image reg[k], in the caller's order, whose list
// (v, reg[k]) maps f -> g with g free.  A list holds at most one g per f, so that is the minimum of (k, g) over the passing
// entries of all lists:
//   N1 k_nvt_walk      one workgroup per registered image: its list, entries with both ends free (landmark id -1 in the
//                      resident table) do a 64-bit atomicMin of (k << 32) | g into best[f] -- integer min, one value per
//                      (k, f): the result does not depend on arrival order
//   N2 k_nvt_emit      one workgroup: ordered compaction of best over f (wg_rank per 1024 features, a running count), both
//                      pixels gathered, the CSR arrays and (reg image, g, f) per track written in ascending f
//   N3 k_nvt_commit    behind the triangulation: accepted track j gets landmark first + (accepted tracks before it), written
//                      into the table for both of its features (ordered rank again; no atomic decides a position)
#include "camgeom.h"
#include "wgprim.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int CB = 256;                  // threads per workgroup (4 waves)
constexpr int CPT = 16;                  // hit-row entries per thread in C3 / C5
constexpr int CT = CB * CPT;             // entries per tile
constexpr int32_t NO_OBS = INT32_MAX;    // empty obs_of entry
constexpr int CELLS = 32;                // rankNextImages: cellSize = 1 << 5

struct SlotDev {
    const int32_t *xy;   // K x 2 pixel coordinates (rcn_coords_upload)
    int64_t oo;          // first entry of this image's row of obs_of
    int32_t K, pad;
};

__global__ __launch_bounds__(CB) void k_corr_index(const int32_t *__restrict__ pt_off, int32_t n_points, int32_t n_obs,
                                                   const int32_t *__restrict__ obs_img, const int32_t *__restrict__ obs_feat,
                                                   const int32_t *__restrict__ id2slot, int32_t id_lo, int32_t id_span,
                                                   const SlotDev *__restrict__ slots, int32_t *__restrict__ obs_of,
                                                   int32_t *__restrict__ obs_pt, int32_t *__restrict__ in_graph)
{
    const int p = blockIdx.x * CB + threadIdx.x;
    if (p >= n_points) return;
    const int o0 = max(0, min(pt_off[p], n_obs)), o1 = max(o0, min(pt_off[p + 1], n_obs));
    for (int o = o0; o < o1; ++o) {
        obs_pt[o] = p;
        const int64_t r = (int64_t)obs_img[o] - id_lo;
        if (r < 0 || r >= id_span) continue;
        const int s = id2slot[r];
        if (s < 0) continue;
        const int f = obs_feat[o];
        if (f < 0 || f >= slots[s].K) continue;
        atomicMin(obs_of + slots[s].oo + f, o);          // a repeated (image, feature): its first observation
        in_graph[s] = 1;
    }
}

struct WalkArgs {
    const int2 *ent;              // (feature of a, feature of b) per list entry
    const int64_t *list_off;      // n_lists + 1
    const int32_t *dir;           // n_slots x n_slots: (list << 1) | read backwards, -1 = no list
    const int32_t *id2slot;
    const SlotDev *slots;
    const int32_t *obs_of, *in_graph;
    const int32_t *cand, *shape;  // candidate ids, (rows, cols) per candidate
    int32_t n_slots, id_lo, id_span, c0;
    int64_t ld;                   // hit-row stride
    int32_t *hit;
    uint32_t *cells;              // 32 words per candidate
    int32_t *outside;
};

__global__ __launch_bounds__(CB) void k_corr_walk(WalkArgs a)
{
    const int i = blockIdx.x, k = blockIdx.y, c = a.c0 + k;
    const int64_t r = (int64_t)a.cand[c] - a.id_lo;
    if (r < 0 || r >= a.id_span) return;
    const int sc = a.id2slot[r];
    if (sc < 0 || sc == i || !a.in_graph[i]) return;     // imgMatches[c] never holds c
    const int d = a.dir[(size_t)i * a.n_slots + sc];
    if (d < 0) return;
    const bool back = d & 1;
    const int64_t e0 = a.list_off[d >> 1], e1 = a.list_off[(d >> 1) + 1];
    const SlotDev si = a.slots[i], sk = a.slots[sc];
    const double rows = (double)a.shape[2 * c], cols = (double)a.shape[2 * c + 1];
    int32_t *row = a.hit + (size_t)k * a.ld;
    for (int64_t e = e0 + threadIdx.x; e < e1; e += CB) {
        const int2 m = a.ent[e];
        const int f = back ? m.y : m.x, g = back ? m.x : m.y;
        if (f < 0 || f >= si.K || g < 0 || g >= sk.K) continue;
        const int o = a.obs_of[si.oo + f];
        if (o == NO_OBS) continue;
        row[o] = g;
        // rankNextImages (:726-731): (int)(cellSize * x / (double)cols); truncation toward zero puts (-1, 32) in 0 .. 31
        const double qx = (double)(CELLS * (long long)sk.xy[2 * (size_t)g]) / cols;
        const double qy = (double)(CELLS * (long long)sk.xy[2 * (size_t)g + 1]) / rows;
        if (qx > -1.0 && qx < (double)CELLS && qy > -1.0 && qy < (double)CELLS)
            atomicOr(a.cells + CELLS * (size_t)c + (int)qy, 1u << (int)qx);
        else
            atomicAdd(a.outside + c, 1);
    }
}

__device__ __forceinline__ void load_tile(const int32_t *p, int32_t (&v)[CPT])
{
    const int4 *q = reinterpret_cast<const int4 *>(p);
#pragma unroll
    for (int j = 0; j < CPT / 4; ++j) {
        const int4 w = q[j];
        v[4 * j] = w.x; v[4 * j + 1] = w.y; v[4 * j + 2] = w.z; v[4 * j + 3] = w.w;
    }
}

__global__ __launch_bounds__(CB) void k_corr_count(const int32_t *__restrict__ hit, int64_t ld, int32_t *__restrict__ blk_cnt)
{
    __shared__ int32_t red[CB / 64];
    int32_t v[CPT];
    load_tile(hit + (size_t)blockIdx.y * ld + (size_t)blockIdx.x * CT + CPT * threadIdx.x, v);
    int n = 0;
#pragma unroll
    for (int j = 0; j < CPT; ++j) n += v[j] >= 0;
    for (int s = 32; s; s >>= 1) n += __shfl_down(n, s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) blk_cnt[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// exclusive scan of the n tile counts of a batch in one workgroup, behind *base (the entries of earlier batches);
// cand_off[k] = offset of tile k * bpr (the candidate's first); *base += the batch's total
__global__ __launch_bounds__(1024) void k_corr_scan(const int32_t *__restrict__ cnt, int n, int bpr, int64_t *__restrict__ off,
                                                    int64_t *__restrict__ base, int64_t *__restrict__ cand_off)
{
    const int t = threadIdx.x;
    const int64_t end = wg_scan_array(cnt, n, off, *base);      // *base: read by every thread before the scan's barriers; written after them
    if (t == 1023) *base = end;
    __syncthreads();                                             // off was written by other threads of this workgroup
    for (int k = t; k * (int64_t)bpr < n; k += 1024) cand_off[k] = off[k * (int64_t)bpr];
}

__global__ __launch_bounds__(CB) void k_corr_compact(const int32_t *__restrict__ hit, int64_t ld, const int32_t *__restrict__ blk_cnt,
                                                     const int64_t *__restrict__ blk_off, const int32_t *__restrict__ obs_pt,
                                                     int64_t cap, int32_t *__restrict__ out_lm, int32_t *__restrict__ out_feat)
{
    __shared__ int32_t sh[CB / 64];
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    if (blk_cnt[tile] == 0) return;                 // uniform over the workgroup
    const int t = threadIdx.x;
    const size_t o0 = (size_t)blockIdx.x * CT + CPT * t;
    int32_t v[CPT];
    load_tile(hit + (size_t)blockIdx.y * ld + o0, v);
    int n = 0;
#pragma unroll
    for (int j = 0; j < CPT; ++j) n += v[j] >= 0;
    int32_t in_tile;
    int64_t pos = blk_off[tile] + wg_scan_incl<int32_t, CB>(n, sh, in_tile) - n;
#pragma unroll
    for (int j = 0; j < CPT; ++j) {
        if (v[j] < 0) continue;
        if (pos < cap) { out_lm[pos] = obs_pt[o0 + j]; out_feat[pos] = v[j]; }
        ++pos;
    }
}

__global__ void k_corr_final(const uint32_t *__restrict__ cells, const int32_t *__restrict__ outside, int n_cand,
                             const int64_t *__restrict__ base, int64_t *__restrict__ cand_off, int64_t *__restrict__ total,
                             int32_t *__restrict__ out_cells, int32_t *__restrict__ out_outside)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_cand) {
        int s = 0;
        for (int w = 0; w < CELLS; ++w) s += __popc(cells[CELLS * (size_t)c + w]);
        out_cells[c] = s;
        if (out_outside) out_outside[c] = outside[c];
    }
    if (c == 0) { cand_off[n_cand] = *base; *total = *base; }
}

// ---- attach (step 1 of triangulateMatchedLandmarks) -------------------------------------------------------------------

struct AttachArgs {
    const double *P, *K, *pts;     // [R | t] rows (12), fx fy cx cy k1 k2, n_points x 3
    const int32_t *lm, *feat, *xy;
    int32_t n_points, n, n_feat;
    double max_err;
    uint8_t *status;
    int32_t *win;                  // n_feat: smallest index of a passing entry per feature
};

__global__ __launch_bounds__(CB) void k_attach_rules(AttachArgs a)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * CB + threadIdx.x;
    if (e >= a.n) return;
    const int l = a.lm[e], f = a.feat[e];
    if (l < 0 || l >= a.n_points || f < 0 || f >= a.n_feat) { a.status[e] = 1; return; }     // the host entries reject these
    const double X[3] = {a.pts[3 * (size_t)l], a.pts[3 * (size_t)l + 1], a.pts[3 * (size_t)l + 2]};
    double depth;
    const double resid = reproj_l1(a.P, a.K, X, a.xy[2 * (size_t)e], a.xy[2 * (size_t)e + 1], &depth);
    const uint8_t st = !(depth > 0.0) ? 1 : !(resid < a.max_err) ? 2 : 0;      // :506, NaN rejected
    a.status[e] = st;
    if (st == 0) atomicMin(a.win + f, e);
}

__global__ __launch_bounds__(CB) void k_attach_taken(AttachArgs a)
{
    const int e = blockIdx.x * CB + threadIdx.x;
    if (e >= a.n || a.status[e] != 0) return;
    if (a.win[a.feat[e]] != e) a.status[e] = 3;      // an earlier entry of this feature was attached
}

size_t al256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

// Launches of the attach kernels on device arrays; ws: rcn_int_attach_ws_bytes(n_feat) bytes
size_t rcn_int_attach_ws_bytes(int32_t n_feat) { return al256(4 * (size_t)std::max(n_feat, 1)); }

int rcn_int_attach_launch(rcn_ctx *ctx, const double *P, const double *K, const double *pts, int32_t n_points, int32_t n,
                          const int32_t *lm, const int32_t *feat, const int32_t *xy, int32_t n_feat, double max_err,
                          uint8_t *status, void *ws)
{
    if (n == 0) return RCN_OK;
    hipStream_t st = ctx->stream;
    AttachArgs a{P, K, pts, lm, feat, xy, n_points, n, n_feat, max_err, status, static_cast<int32_t *>(ws)};
    RCN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(ws), INT32_MAX, (size_t)std::max(n_feat, 1), st));
    const unsigned nb = (unsigned)((n + CB - 1) / CB);
    k_attach_rules<<<nb, CB, 0, st>>>(a);
    k_attach_taken<<<nb, CB, 0, st>>>(a);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// host structure check of attach entries: landmark in range, feature >= 0; *n_feat = largest feature + 1
int rcn_int_attach_check(rcn_ctx *ctx, const char *who, int32_t n_points, int32_t n, const int32_t *lm, const int32_t *feat, int32_t *n_feat)
{
    int32_t mx = -1;
    for (int32_t e = 0; e < n; ++e) {
        if (lm[e] < 0 || lm[e] >= n_points) { ctx->set_error(std::string(who) + ": landmark index out of range"); return RCN_ERR_ARG; }
        if (feat[e] < 0) { ctx->set_error(std::string(who) + ": negative feature index"); return RCN_ERR_ARG; }
        mx = std::max(mx, feat[e]);
    }
    *n_feat = mx + 1;
    return RCN_OK;
}

namespace {

// the resident lists' slot table for the current coordinates (one small host-to-device copy, staged in the ctx)
int refresh_slots(rcn_ctx *ctx, const char *who, int64_t *sum_k)
{
    CorrLists &L = ctx->corr;
    if (ctx->corr_slots_pending) { RCN_HIP(hipEventSynchronize(ctx->corr_ev)); ctx->corr_slots_pending = false; }
    const size_t ns = L.ids.size();
    ctx->corr_slots_host.resize(std::max<size_t>(ns, 1) * sizeof(SlotDev));
    SlotDev *sd = reinterpret_cast<SlotDev *>(ctx->corr_slots_host.data());
    int64_t oo = 0;
    for (size_t s = 0; s < ns; ++s) {
        auto it = ctx->coords.find(L.ids[s]);
        if (it == ctx->coords.end()) { ctx->set_error(std::string(who) + ": coordinates of image " + std::to_string(L.ids[s]) + " are no longer resident"); return RCN_ERR_ARG; }
        sd[s].xy = it->second.first.as<int32_t>();
        sd[s].K = it->second.second;
        sd[s].oo = oo;
        sd[s].pad = 0;
        oo += it->second.second;
    }
    *sum_k = oo;
    RCN_HIP(ctx->corr_slots.reserve(std::max<size_t>(ns, 1) * sizeof(SlotDev)));
    if (ns) {
        RCN_HIP(hipMemcpyAsync(ctx->corr_slots.p, sd, ns * sizeof(SlotDev), hipMemcpyHostToDevice, ctx->stream));
        RCN_HIP(hipEventRecord(ctx->corr_ev, ctx->stream));
        ctx->corr_slots_pending = true;
    }
    return RCN_OK;
}

// everything after the argument checks, all pointers in HBM (ctx->mu held)
int corr_launch(rcn_ctx *ctx, const char *who, int32_t n_points, int32_t n_obs, const int32_t *pt_off, const int32_t *obs_img,
                const int32_t *obs_feat, int32_t n_cand, const int32_t *cand, const int32_t *shape, int64_t *cand_off,
                int32_t *out_lm, int32_t *out_feat, int64_t cap, int64_t *total, int32_t *out_cells, int32_t *out_outside)
{
    CorrLists &L = ctx->corr;
    hipStream_t st = ctx->stream;
    int64_t sum_k = 0;
    int rc = refresh_slots(ctx, who, &sum_k);
    if (rc) return rc;
    const int32_t ns = (int32_t)L.ids.size();
    const int64_t bpr = std::max<int64_t>(1, ((int64_t)n_obs + CT - 1) / CT);
    const int64_t ld = bpr * CT;
    const int64_t row_bytes = 4 * ld;
    const int64_t nbatch = std::max<int64_t>(1, std::min<int64_t>({(int64_t)std::max(n_cand, 1), ctx->corr_budget / row_bytes, 65535}));
    const size_t nc = (size_t)std::max(n_cand, 1);
    const size_t b_of = al256(4 * (size_t)std::max<int64_t>(sum_k, 1)), b_pt = al256(4 * (size_t)std::max(n_obs, 1)),
                 b_ing = al256(4 * (size_t)std::max(ns, 1)), b_cells = al256(4 * CELLS * nc), b_out = al256(4 * nc),
                 b_cnt = al256(4 * (size_t)(bpr * nbatch)), b_off = al256(8 * (size_t)(bpr * nbatch)), b_base = 256,
                 b_hit = al256((size_t)row_bytes * (size_t)nbatch);
    RCN_HIP(ctx->corr_ws.reserve(b_of + b_pt + b_ing + b_cells + b_out + b_cnt + b_off + b_base + b_hit));
    char *w = ctx->corr_ws.as<char>();
    int32_t *obs_of = reinterpret_cast<int32_t *>(w); w += b_of;
    int32_t *obs_pt = reinterpret_cast<int32_t *>(w); w += b_pt;
    int32_t *in_graph = reinterpret_cast<int32_t *>(w); w += b_ing;
    uint32_t *cells = reinterpret_cast<uint32_t *>(w); w += b_cells;
    int32_t *outside = reinterpret_cast<int32_t *>(w); w += b_out;
    int32_t *blk_cnt = reinterpret_cast<int32_t *>(w); w += b_cnt;
    int64_t *blk_off = reinterpret_cast<int64_t *>(w); w += b_off;
    int64_t *base = reinterpret_cast<int64_t *>(w); w += b_base;
    int32_t *hit = reinterpret_cast<int32_t *>(w);
    const SlotDev *slots = ctx->corr_slots.as<SlotDev>();

    RCN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(obs_of), NO_OBS, (size_t)std::max<int64_t>(sum_k, 1), st));
    RCN_HIP(hipMemsetAsync(obs_pt, 0xFF, b_pt, st));
    RCN_HIP(hipMemsetAsync(in_graph, 0, b_ing, st));
    RCN_HIP(hipMemsetAsync(cells, 0, b_cells + b_out, st));       // cells and outside are adjacent
    RCN_HIP(hipMemsetAsync(base, 0, 8, st));
    if (n_points > 0 && ns > 0)
        k_corr_index<<<(unsigned)((n_points + CB - 1) / CB), CB, 0, st>>>(pt_off, n_points, n_obs, obs_img, obs_feat, L.id2slot.as<int32_t>(),
                                                                         L.id_lo, L.id_span, slots, obs_of, obs_pt, in_graph);
    WalkArgs wa;
    wa.ent = L.ent.as<int2>(); wa.list_off = L.list_off.as<int64_t>(); wa.dir = L.dir.as<int32_t>(); wa.id2slot = L.id2slot.as<int32_t>();
    wa.slots = slots; wa.obs_of = obs_of; wa.in_graph = in_graph; wa.cand = cand; wa.shape = shape;
    wa.n_slots = ns; wa.id_lo = L.id_lo; wa.id_span = L.id_span; wa.ld = ld; wa.hit = hit; wa.cells = cells; wa.outside = outside;
    for (int64_t c0 = 0; c0 < n_cand; c0 += nbatch) {
        const int64_t nb = std::min<int64_t>(nbatch, n_cand - c0);
        RCN_HIP(hipMemsetAsync(hit, 0xFF, (size_t)row_bytes * (size_t)nb, st));
        wa.c0 = (int32_t)c0;
        if (ns > 0) k_corr_walk<<<dim3((unsigned)ns, (unsigned)nb), CB, 0, st>>>(wa);
        const dim3 tiles((unsigned)bpr, (unsigned)nb);
        k_corr_count<<<tiles, CB, 0, st>>>(hit, ld, blk_cnt);
        k_corr_scan<<<1, 1024, 0, st>>>(blk_cnt, (int)(bpr * nb), (int)bpr, blk_off, base, cand_off + c0);
        k_corr_compact<<<tiles, CB, 0, st>>>(hit, ld, blk_cnt, blk_off, obs_pt, cap, out_lm, out_feat);
    }
    k_corr_final<<<(unsigned)((n_cand + CB) / CB), CB, 0, st>>>(cells, outside, n_cand, base, cand_off, total, out_cells, out_outside);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// ---- a pair's entries in ascending query order, from the resident lists (rcn_twoview_init_device) -------------------------
//   F1 k_pair_mark     one workgroup per pair (a, b): the list (a, b), or (b, a) read backwards under mirror, scattered into
//                      a row over a's features: mark[f] = g (one writer per word: the list is injective), then the row counted
//   F2 k_pair_offsets  one thread: the pairs' offsets; a pair whose entries would pass `capacity` gets none
//   F3 k_pair_fill     one workgroup per pair: ordered compaction of the row (ballot prefix per wave, wave totals through
//                      LDS) into the pixels of both sides and, when asked, the (f, g) themselves
struct PairFill { int32_t sa, sb; int64_t woff; };      // slots of a and b, first word of the pair's row of mark

__global__ __launch_bounds__(CB) void k_pair_mark(const PairFill *__restrict__ pf, const int2 *__restrict__ ent,
                                                  const int64_t *__restrict__ list_off, const int32_t *__restrict__ dir, int32_t n_slots,
                                                  const SlotDev *__restrict__ slots, int32_t *__restrict__ mark, int32_t *__restrict__ cnt)
{
    __shared__ int32_t red[CB / 64];
    const int p = blockIdx.x, t = threadIdx.x;
    const PairFill q = pf[p];
    const int Ka = slots[q.sa].K, Kb = slots[q.sb].K;
    int32_t *row = mark + q.woff;
    const int d = dir[(size_t)q.sa * n_slots + q.sb];
    if (d >= 0) {                                        // uniform over the workgroup
        const bool back = d & 1;
        const int64_t e0 = list_off[d >> 1], e1 = list_off[(d >> 1) + 1];
        for (int64_t e = e0 + t; e < e1; e += CB) {
            const int2 m = ent[e];
            const int f = back ? m.y : m.x, g = back ? m.x : m.y;
            if (f < 0 || f >= Ka || g < 0 || g >= Kb) continue;
            row[f] = g;
        }
    }
    __syncthreads();                                     // the row is read back by this workgroup only
    int n = 0;
    for (int f = t; f < Ka; f += CB) n += row[f] >= 0;
    for (int s = 32; s; s >>= 1) n += __shfl_down(n, s);
    if ((t & 63) == 0) red[t >> 6] = n;
    __syncthreads();
    if (t == 0) cnt[p] = red[0] + red[1] + red[2] + red[3];
}

__global__ void k_pair_offsets(int32_t *__restrict__ cnt, int n_pairs, int64_t capacity, int64_t *__restrict__ off)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t s = 0;
    off[0] = 0;
    for (int p = 0; p < n_pairs; ++p) {
        int64_t c = cnt[p];
        if (s + c > capacity) { c = 0; cnt[p] = 0; }     // no room: the pair gets no entries
        s += c;
        off[p + 1] = s;
    }
}

__global__ __launch_bounds__(CB) void k_pair_fill(const PairFill *__restrict__ pf, const SlotDev *__restrict__ slots,
                                                  const int32_t *__restrict__ mark, const int32_t *__restrict__ cnt,
                                                  const int64_t *__restrict__ off, int32_t *__restrict__ xy1, int32_t *__restrict__ xy2,
                                                  int32_t *__restrict__ qt)
{
    __shared__ int32_t wtot[CB / 64];
    const int p = blockIdx.x, t = threadIdx.x;
    if (cnt[p] <= 0) return;                             // uniform
    const PairFill q = pf[p];
    const SlotDev sa = slots[q.sa], sb = slots[q.sb];
    const int32_t *row = mark + q.woff;
    int64_t run = off[p];
    const int64_t end = off[p + 1];
    for (int f0 = 0; f0 < sa.K; f0 += CB) {
        const int f = f0 + t;
        const int g = f < sa.K ? row[f] : -1;
        int chunk;
        const int64_t pos = run + wg_rank<CB>(g >= 0, wtot, chunk);
        if (g >= 0 && pos < end) {
            xy1[2 * pos] = sa.xy[2 * (size_t)f]; xy1[2 * pos + 1] = sa.xy[2 * (size_t)f + 1];
            xy2[2 * pos] = sb.xy[2 * (size_t)g]; xy2[2 * pos + 1] = sb.xy[2 * (size_t)g + 1];
            if (qt) { qt[2 * pos] = f; qt[2 * pos + 1] = g; }
        }
        run += chunk;
    }
}

}  // namespace

// rcn_twoview_init_device's front half, with ctx->mu held: the entries of n_pairs directed pairs (host array of image ids)
// in ascending order of the first image's feature, pair p at off_dev[p] .. off_dev[p + 1] of xy1_dev / xy2_dev / qt_dev
// (qt_dev may be NULL), `capacity` entries of room.  Only enqueues.  A pair without a list gets no entries.
int rcn_int_pair_fill(rcn_ctx *ctx, const char *who, int32_t n_pairs, const int32_t *pairs, int64_t capacity, int64_t *off_dev,
                      int32_t *xy1_dev, int32_t *xy2_dev, int32_t *qt_dev)
{
    CorrLists &L = ctx->corr;
    if (!L.live) { ctx->set_error(std::string(who) + ": no match lists (rcn_match_lists_upload)"); return RCN_ERR_ARG; }
    hipStream_t st = ctx->stream;
    if (n_pairs == 0) { RCN_HIP(hipMemsetAsync(off_dev, 0, 8, st)); return RCN_OK; }
    if (!ctx->tv_ev && hipEventCreateWithFlags(&ctx->tv_ev, hipEventDisableTiming) != hipSuccess) { ctx->tv_ev = nullptr; RCN_HIP(hipGetLastError()); }
    if (ctx->tv_stage_pending) { RCN_HIP(hipEventSynchronize(ctx->tv_ev)); ctx->tv_stage_pending = false; }    // the staging buffer is free again
    ctx->tv_stage_host.resize((size_t)n_pairs * sizeof(PairFill));
    PairFill *pf = reinterpret_cast<PairFill *>(ctx->tv_stage_host.data());
    int64_t sum_ka = 0;
    for (int32_t p = 0; p < n_pairs; ++p) {
        int32_t sl[2];
        for (int k = 0; k < 2; ++k) {
            const int32_t id = pairs[2 * p + k];
            auto it = std::lower_bound(L.ids.begin(), L.ids.end(), id);
            if (it == L.ids.end() || *it != id) { ctx->set_error(std::string(who) + ": image " + std::to_string(id) + " is not among the resident lists' images"); return RCN_ERR_NOT_FOUND; }
            sl[k] = (int32_t)(it - L.ids.begin());
        }
        if (sl[0] == sl[1]) { ctx->set_error(std::string(who) + ": pair (" + std::to_string(pairs[2 * p]) + ", " + std::to_string(pairs[2 * p]) + ") pairs an image with itself"); return RCN_ERR_ARG; }
        auto ca = ctx->coords.find(pairs[2 * p]);
        if (ca == ctx->coords.end()) { ctx->set_error(std::string(who) + ": coordinates of image " + std::to_string(pairs[2 * p]) + " are no longer resident"); return RCN_ERR_ARG; }
        pf[p].sa = sl[0]; pf[p].sb = sl[1]; pf[p].woff = sum_ka;
        sum_ka += ca->second.second;
    }
    int64_t sum_k = 0;
    int rc = refresh_slots(ctx, who, &sum_k);
    if (rc) return rc;
    const size_t np = (size_t)n_pairs;
    const size_t b_pf = al256(np * sizeof(PairFill)), b_cnt = al256(4 * np), b_mark = al256(4 * (size_t)std::max<int64_t>(sum_ka, 1));
    RCN_HIP(ctx->tv_fws.reserve(b_pf + b_cnt + b_mark));
    char *w = ctx->tv_fws.as<char>();
    PairFill *d_pf = reinterpret_cast<PairFill *>(w);
    int32_t *d_cnt = reinterpret_cast<int32_t *>(w + b_pf), *d_mark = reinterpret_cast<int32_t *>(w + b_pf + b_cnt);
    RCN_HIP(hipMemcpyAsync(d_pf, pf, np * sizeof(PairFill), hipMemcpyHostToDevice, st));
    RCN_HIP(hipEventRecord(ctx->tv_ev, st));
    ctx->tv_stage_pending = true;
    RCN_HIP(hipMemsetAsync(d_mark, 0xFF, b_mark, st));
    const SlotDev *slots = ctx->corr_slots.as<SlotDev>();
    k_pair_mark<<<(unsigned)n_pairs, CB, 0, st>>>(d_pf, L.ent.as<int2>(), L.list_off.as<int64_t>(), L.dir.as<int32_t>(), (int32_t)L.ids.size(), slots, d_mark, d_cnt);
    k_pair_offsets<<<1, 64, 0, st>>>(d_cnt, n_pairs, capacity, off_dev);
    k_pair_fill<<<(unsigned)n_pairs, CB, 0, st>>>(d_pf, slots, d_mark, d_cnt, off_dev, xy1_dev, xy2_dev, qt_dev);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

// ---- step 3 of triangulateMatchedLandmarks: the new view's candidate tracks -------------------------------------------------
namespace {

constexpr int NB = 1024;                                 // threads of the one workgroup of N2 / N3 (16 waves)
constexpr unsigned long long NO_BEST = ~0ull;            // best[f]: no list has a free partner for f

struct RegDev { int32_t slot, cam, img, pad; };          // registered image k: its list slot, camera row, image id

__global__ __launch_bounds__(CB) void k_nvt_walk(const RegDev *__restrict__ reg, int32_t sv, const int2 *__restrict__ ent,
                                                 const int64_t *__restrict__ list_off, const int32_t *__restrict__ dir, int32_t n_slots,
                                                 const SlotDev *__restrict__ slots, const int32_t *__restrict__ lid,
                                                 const int64_t *__restrict__ lid_off, unsigned long long *__restrict__ best)
{
    const int k = blockIdx.x, sr = reg[k].slot;
    const int d = dir[(size_t)sv * n_slots + sr];        // featureMatches[(v, reg[k])]
    if (d < 0) return;                                   // uniform over the workgroup
    const bool back = d & 1;
    const int64_t e0 = list_off[d >> 1], e1 = list_off[(d >> 1) + 1];
    const int Kv = slots[sv].K, Kr = slots[sr].K;
    const int32_t *idv = lid + lid_off[sv], *idr = lid + lid_off[sr];
    for (int64_t e = e0 + threadIdx.x; e < e1; e += CB) {
        const int2 m = ent[e];
        const int f = back ? m.y : m.x, g = back ? m.x : m.y;
        if (f < 0 || f >= Kv || g < 0 || g >= Kr) continue;
        if (idv[f] != -1 || idr[g] != -1) continue;      // :519 and :541: a taken partner does not end the search
        atomicMin(best + f, ((unsigned long long)(unsigned)k << 32) | (unsigned)g);
    }
}

__global__ __launch_bounds__(NB) void k_nvt_emit(const RegDev *__restrict__ reg, int32_t sv, int32_t cam_v,
                                                 const SlotDev *__restrict__ slots, const unsigned long long *__restrict__ best,
                                                 int32_t capacity, int32_t *__restrict__ n_tracks, int32_t *__restrict__ trk_off,
                                                 int32_t *__restrict__ obs_cam, int32_t *__restrict__ obs_xy, int32_t *__restrict__ trk_src)
{
    __shared__ int wtot[NB / 64];
    const int t = threadIdx.x;
    const SlotDev s = slots[sv];
    int run = 0;                                         // tracks of the features before this chunk (uniform)
    for (int f0 = 0; f0 < s.K; f0 += NB) {
        const int f = f0 + t;
        const unsigned long long b = f < s.K ? best[f] : NO_BEST;
        int chunk;
        const int pos = run + wg_rank<NB>(b != NO_BEST, wtot, chunk);
        if (b != NO_BEST && pos < capacity) {
            const RegDev r = reg[(int)(b >> 32)];
            const int g = (int)(unsigned)b;
            const int32_t *rxy = slots[r.slot].xy;
            const size_t p = (size_t)pos;
            obs_cam[2 * p] = r.cam; obs_cam[2 * p + 1] = cam_v;          // the registered observation first (matchedImgIdFeatId, :543-544)
            obs_xy[4 * p] = rxy[2 * (size_t)g]; obs_xy[4 * p + 1] = rxy[2 * (size_t)g + 1];
            obs_xy[4 * p + 2] = s.xy[2 * (size_t)f]; obs_xy[4 * p + 3] = s.xy[2 * (size_t)f + 1];
            trk_src[3 * p] = r.img; trk_src[3 * p + 1] = g; trk_src[3 * p + 2] = f;
        }
        run += chunk;
    }
    for (int j = t; j <= capacity; j += NB) trk_off[j] = 2 * min(j, run);
    if (t == 0) *n_tracks = run;
}

__global__ __launch_bounds__(NB) void k_nvt_commit(const int32_t *__restrict__ n_tracks, int32_t capacity, const int32_t *__restrict__ trk_src,
                                                   const uint8_t *__restrict__ status, int32_t sv, const int32_t *__restrict__ id2slot,
                                                   int32_t id_lo, int32_t id_span, int32_t *__restrict__ lid, const int64_t *__restrict__ lid_off,
                                                   int32_t first)
{
    __shared__ int wtot[NB / 64];
    const int t = threadIdx.x, n = min(*n_tracks, capacity);
    int run = 0;
    for (int j0 = 0; j0 < n; j0 += NB) {
        const int j = j0 + t;
        const bool acc = j < n && status[j] == 0;
        int chunk;
        const int id = first + run + wg_rank<NB>(acc, wtot, chunk);
        if (acc) {
            const int64_t r = (int64_t)trk_src[3 * (size_t)j] - id_lo;
            const int sr = r >= 0 && r < id_span ? id2slot[r] : -1;
            lid[lid_off[sv] + trk_src[3 * (size_t)j + 2]] = id;          // distinct tracks have distinct f, and per list distinct g
            if (sr >= 0) lid[lid_off[sr] + trk_src[3 * (size_t)j + 1]] = id;
        }
        run += chunk;
    }
}

__global__ void k_lid_scatter(const int64_t *__restrict__ at, const int32_t *__restrict__ id, int32_t n, int32_t *__restrict__ lid)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) lid[at[e]] = id[e];
}

// the landmark-id table as the current lists and coordinates need it, or an error
int lid_check(rcn_ctx *ctx, const char *who)
{
    if (!ctx->lid_live) { ctx->set_error(std::string(who) + ": no landmark-id table (rcn_landmark_ids_reset)"); return RCN_ERR_ARG; }
    if (ctx->lid_lists_gen != ctx->lists_gen || ctx->lid_coords_gen != ctx->coords_gen) {
        ctx->set_error(std::string(who) + ": the landmark-id table was invalidated by a change of the match lists or the coordinates (rcn_landmark_ids_reset)");
        return RCN_ERR_ARG;
    }
    return RCN_OK;
}

int slot_of(const CorrLists &L, int32_t id)
{
    auto it = std::lower_bound(L.ids.begin(), L.ids.end(), id);
    return it == L.ids.end() || *it != id ? -1 : (int)(it - L.ids.begin());
}

}  // namespace

int32_t rcn_int_coords_rows(rcn_ctx *ctx, int32_t img)
{
    auto it = ctx->coords.find(img);
    return it == ctx->coords.end() ? -1 : it->second.second;
}

int rcn_int_new_view_tracks(rcn_ctx *ctx, const char *who, int32_t v, int32_t n_reg, const int32_t *reg_img, int32_t cam_v,
                            const int32_t *reg_cam, int32_t capacity, int32_t *n_tracks_dev, int32_t *trk_off_dev,
                            int32_t *obs_cam_dev, int32_t *obs_xy_dev, int32_t *trk_src_dev)
{
    CorrLists &L = ctx->corr;
    if (n_reg < 0 || capacity < 0 || capacity > (1 << 30) || (n_reg > 0 && (!reg_img || !reg_cam)) || !n_tracks_dev || !trk_off_dev ||
        (capacity > 0 && (!obs_cam_dev || !obs_xy_dev || !trk_src_dev))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    if (!L.live) { ctx->set_error(std::string(who) + ": no match lists (rcn_match_lists_upload)"); return RCN_ERR_ARG; }
    int rc = lid_check(ctx, who);
    if (rc) return rc;
    const int sv = slot_of(L, v);
    if (sv < 0) { ctx->set_error(std::string(who) + ": image " + std::to_string(v) + " is not among the resident lists' images"); return RCN_ERR_NOT_FOUND; }
    if (ctx->nvt_stage_pending) { RCN_HIP(hipEventSynchronize(ctx->nvt_ev)); ctx->nvt_stage_pending = false; }     // the staging buffer is free again
    ctx->nvt_stage_host.resize((size_t)std::max(n_reg, 1) * sizeof(RegDev));
    RegDev *rd = reinterpret_cast<RegDev *>(ctx->nvt_stage_host.data());
    std::vector<uint8_t> seen(L.ids.size(), 0);
    for (int32_t k = 0; k < n_reg; ++k) {
        const int sr = slot_of(L, reg_img[k]);
        if (sr < 0) { ctx->set_error(std::string(who) + ": image " + std::to_string(reg_img[k]) + " is not among the resident lists' images"); return RCN_ERR_NOT_FOUND; }
        if (sr == sv) { ctx->set_error(std::string(who) + ": the new image " + std::to_string(v) + " is among the registered images"); return RCN_ERR_ARG; }
        if (seen[sr]) { ctx->set_error(std::string(who) + ": registered image " + std::to_string(reg_img[k]) + " is listed twice"); return RCN_ERR_ARG; }
        seen[sr] = 1;
        rd[k] = RegDev{sr, reg_cam[k], reg_img[k], 0};
    }
    int64_t sum_k = 0;
    rc = refresh_slots(ctx, who, &sum_k);
    if (rc) return rc;
    hipStream_t st = ctx->stream;
    if (!ctx->nvt_ev && hipEventCreateWithFlags(&ctx->nvt_ev, hipEventDisableTiming) != hipSuccess) { ctx->nvt_ev = nullptr; RCN_HIP(hipGetLastError()); }
    const int32_t Kv = ctx->coords.find(v)->second.second;               // refresh_slots found it
    const size_t b_reg = al256((size_t)std::max(n_reg, 1) * sizeof(RegDev)), b_best = al256(8 * (size_t)std::max(Kv, 1));
    RCN_HIP(ctx->nvt_ws.reserve(b_reg + b_best));
    RegDev *d_reg = ctx->nvt_ws.as<RegDev>();
    unsigned long long *d_best = reinterpret_cast<unsigned long long *>(ctx->nvt_ws.as<char>() + b_reg);
    if (n_reg) {
        RCN_HIP(hipMemcpyAsync(d_reg, rd, (size_t)n_reg * sizeof(RegDev), hipMemcpyHostToDevice, st));
        RCN_HIP(hipEventRecord(ctx->nvt_ev, st));
        ctx->nvt_stage_pending = true;
    }
    RCN_HIP(hipMemsetAsync(d_best, 0xFF, b_best, st));
    const SlotDev *slots = ctx->corr_slots.as<SlotDev>();
    if (n_reg)
        k_nvt_walk<<<(unsigned)n_reg, CB, 0, st>>>(d_reg, sv, L.ent.as<int2>(), L.list_off.as<int64_t>(), L.dir.as<int32_t>(), (int32_t)L.ids.size(),
                                                   slots, ctx->lid.as<int32_t>(), ctx->lid_slot_off.as<int64_t>(), d_best);
    k_nvt_emit<<<1, NB, 0, st>>>(d_reg, sv, cam_v, slots, d_best, capacity, n_tracks_dev, trk_off_dev, obs_cam_dev, obs_xy_dev, trk_src_dev);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

int rcn_int_new_view_commit(rcn_ctx *ctx, int32_t v, int32_t capacity, const int32_t *n_tracks_dev, const int32_t *trk_src_dev,
                            const uint8_t *status_dev, int32_t first_landmark)
{
    CorrLists &L = ctx->corr;
    if (capacity == 0) return RCN_OK;
    k_nvt_commit<<<1, NB, 0, ctx->stream>>>(n_tracks_dev, capacity, trk_src_dev, status_dev, slot_of(L, v), L.id2slot.as<int32_t>(), L.id_lo,
                                            L.id_span, ctx->lid.as<int32_t>(), ctx->lid_slot_off.as<int64_t>(), first_landmark);
    RCN_HIP(hipGetLastError());
    return RCN_OK;
}

extern "C" {

int rcn_landmark_ids_reset(rcn_ctx *ctx)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_landmark_ids_reset";
    std::lock_guard<std::mutex> lk(ctx->mu);
    CorrLists &L = ctx->corr;
    ctx->lid_live = false;
    if (!L.live) { ctx->set_error(std::string(who) + ": no match lists (rcn_match_lists_upload)"); return RCN_ERR_ARG; }
    if (ctx->coords.empty()) { ctx->set_error(std::string(who) + ": no coordinates (rcn_coords_upload)"); return RCN_ERR_ARG; }
    ctx->lid_rows.clear();
    int64_t total = 0;
    for (auto &kv : ctx->coords) {
        ctx->lid_rows[kv.first] = std::make_pair(total, kv.second.second);
        total += kv.second.second;
    }
    std::vector<int64_t> so(std::max<size_t>(L.ids.size(), 1), 0);
    for (size_t s = 0; s < L.ids.size(); ++s) {
        auto it = ctx->lid_rows.find(L.ids[s]);
        if (it == ctx->lid_rows.end()) { ctx->set_error(std::string(who) + ": coordinates of image " + std::to_string(L.ids[s]) + " are no longer resident"); return RCN_ERR_ARG; }
        so[s] = it->second.first;
    }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RCN_HIP(hipStreamSynchronize(st));                   // nothing queued reads the old table any more
    RCN_HIP(ctx->lid.reserve(4 * (size_t)std::max<int64_t>(total, 1)));
    RCN_HIP(ctx->lid_slot_off.reserve(8 * so.size()));
    RCN_HIP(hipMemsetAsync(ctx->lid.p, 0xFF, 4 * (size_t)std::max<int64_t>(total, 1), st));
    RCN_HIP(hipMemcpyAsync(ctx->lid_slot_off.p, so.data(), 8 * so.size(), hipMemcpyHostToDevice, st));
    RCN_HIP(hipStreamSynchronize(st));                   // so is a local
    ctx->lid_lists_gen = ctx->lists_gen;
    ctx->lid_coords_gen = ctx->coords_gen;
    ctx->lid_live = true;
    return RCN_OK;
}

int rcn_landmark_ids_set(rcn_ctx *ctx, int32_t n, const int32_t *img, const int32_t *feat, const int32_t *id)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_landmark_ids_set";
    if (n < 0 || (n > 0 && (!img || !feat || !id))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = lid_check(ctx, who);
    if (rc) return rc;
    if (n == 0) return RCN_OK;
    std::vector<int64_t> at((size_t)n);
    for (int32_t e = 0; e < n; ++e) {
        auto it = ctx->lid_rows.find(img[e]);
        if (it == ctx->lid_rows.end()) { ctx->set_error(std::string(who) + ": image " + std::to_string(img[e]) + " has no row in the table"); return RCN_ERR_NOT_FOUND; }
        if (feat[e] < 0 || feat[e] >= it->second.second) { ctx->set_error(std::string(who) + ": feature " + std::to_string(feat[e]) + " of image " + std::to_string(img[e]) + " out of range"); return RCN_ERR_ARG; }
        if (id[e] < -1) { ctx->set_error(std::string(who) + ": a landmark id is -1 (free) or >= 0"); return RCN_ERR_ARG; }
        at[e] = it->second.first + feat[e];
    }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t b_at = al256(8 * (size_t)n);
    RCN_HIP(ctx->lid_hws.reserve(b_at + al256(4 * (size_t)n)));
    int64_t *d_at = ctx->lid_hws.as<int64_t>();
    int32_t *d_id = reinterpret_cast<int32_t *>(ctx->lid_hws.as<char>() + b_at);
    RCN_HIP(hipMemcpyAsync(d_at, at.data(), 8 * (size_t)n, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_id, id, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    k_lid_scatter<<<(unsigned)((n + CB - 1) / CB), CB, 0, st>>>(d_at, d_id, n, ctx->lid.as<int32_t>());
    RCN_HIP(hipGetLastError());
    RCN_HIP(hipStreamSynchronize(st));                   // at is a local, id borrowed
    return RCN_OK;
}

int rcn_landmark_ids_read(rcn_ctx *ctx, int32_t img, int32_t *out, int32_t K)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_landmark_ids_read";
    if (K < 0 || (K > 0 && !out)) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    int rc = lid_check(ctx, who);
    if (rc) return rc;
    auto it = ctx->lid_rows.find(img);
    if (it == ctx->lid_rows.end()) { ctx->set_error(std::string(who) + ": image " + std::to_string(img) + " has no row in the table"); return RCN_ERR_NOT_FOUND; }
    if (K != it->second.second) { ctx->set_error(std::string(who) + ": image " + std::to_string(img) + " has " + std::to_string(it->second.second) + " keypoints, not " + std::to_string(K)); return RCN_ERR_ARG; }
    if (K == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipMemcpyAsync(out, ctx->lid.as<int32_t>() + it->second.first, 4 * (size_t)K, hipMemcpyDeviceToHost, ctx->stream));
    RCN_HIP(hipStreamSynchronize(ctx->stream));
    return RCN_OK;
}

int rcn_new_view_tracks_device(rcn_ctx *ctx, int32_t v, int32_t n_reg, const int32_t *reg_img_host, int32_t cam_v,
                               const int32_t *reg_cam_host, int32_t capacity, int32_t *n_tracks_dev, int32_t *trk_off_dev,
                               int32_t *obs_cam_dev, int32_t *obs_xy_dev, int32_t *trk_src_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    return rcn_int_new_view_tracks(ctx, "rcn_new_view_tracks_device", v, n_reg, reg_img_host, cam_v, reg_cam_host, capacity, n_tracks_dev,
                                   trk_off_dev, obs_cam_dev, obs_xy_dev, trk_src_dev);
}

int rcn_new_view_triangulate_device(rcn_ctx *ctx, int32_t v, int32_t n_reg, const int32_t *reg_img_host, int32_t cam_v,
                                    const int32_t *reg_cam_host, int32_t n_cams, const double *poses34_dev, const double *intrinsics_dev,
                                    double max_projection_error, double min_triangulation_angle, int32_t first_landmark, int32_t capacity,
                                    int32_t *n_tracks_dev, int32_t *trk_off_dev, int32_t *obs_cam_dev, int32_t *obs_xy_dev,
                                    int32_t *trk_src_dev, double *out_xyz_dev, uint8_t *out_status_dev, double *out_compact_dev,
                                    int32_t compact_first, int32_t *out_n_accepted_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_new_view_triangulate_device";
    if (n_cams < 1 || !poses34_dev || !intrinsics_dev || first_landmark < 0 || compact_first < 0 || !out_n_accepted_dev ||
        (capacity > 0 && (!out_xyz_dev || !out_status_dev)) || cam_v < 0 || cam_v >= n_cams) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    for (int32_t k = 0; k < n_reg && reg_cam_host; ++k)
        if (reg_cam_host[k] < 0 || reg_cam_host[k] >= n_cams) { ctx->set_error(std::string(who) + ": camera row out of range"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    int rc = rcn_int_new_view_tracks(ctx, who, v, n_reg, reg_img_host, cam_v, reg_cam_host, capacity, n_tracks_dev, trk_off_dev, obs_cam_dev,
                                     obs_xy_dev, trk_src_dev);
    if (rc) return rc;
    RCN_HIP(ctx->tri_dws.reserve(rcn_int_triangulate_ws_bytes(n_cams, capacity)));
    rcn_triangulation_problem dp{n_cams, capacity, 2 * capacity, 0, poses34_dev, intrinsics_dev, trk_off_dev, obs_cam_dev, obs_xy_dev};
    rc = rcn_int_triangulate_launch(ctx, &dp, max_projection_error, min_triangulation_angle, ctx->tri_dws.p, out_xyz_dev, out_status_dev,
                                    out_compact_dev, compact_first, out_n_accepted_dev);
    if (rc) return rc;
    return rcn_int_new_view_commit(ctx, v, capacity, n_tracks_dev, trk_src_dev, out_status_dev, first_landmark);
}

}  // extern "C"

extern "C" {

int rcn_corr_set_workspace_bytes(rcn_ctx *ctx, int64_t bytes)
{
    if (!ctx) return RCN_ERR_ARG;
    if (bytes <= 0) { ctx->set_error("rcn_corr_set_workspace_bytes: bytes must be > 0"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->corr_budget = bytes;
    return RCN_OK;
}

int rcn_match_lists_clear(rcn_ctx *ctx)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipStreamSynchronize(ctx->stream));
    ctx->corr.release();
    ++ctx->lists_gen;
    return RCN_OK;
}

int rcn_match_lists_upload(rcn_ctx *ctx, int32_t n_pairs, const int32_t *pairs, const int64_t *offsets, const int32_t *qt, int32_t mirror)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_match_lists_upload";
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !offsets))) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto fail = [&](const std::string &m) { ctx->set_error(std::string(who) + ": " + m); return RCN_ERR_ARG; };
    if (n_pairs > 0 && offsets[0] != 0) return fail("offsets[0] must be 0");
    for (int32_t p = 0; p < n_pairs; ++p)
        if (offsets[p + 1] < offsets[p]) return fail("offsets must be non-decreasing");
    const int64_t n_ent = n_pairs > 0 ? offsets[n_pairs] : 0;
    if (n_ent > 0 && !qt) return fail("qt is NULL");
    // slots: the images of the lists, ascending; every one needs resident coordinates
    std::vector<int32_t> ids;
    for (int32_t p = 0; p < 2 * n_pairs; ++p) ids.push_back(pairs[p]);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<int32_t> Ks(ids.size());
    for (size_t s = 0; s < ids.size(); ++s) {
        auto it = ctx->coords.find(ids[s]);
        if (it == ctx->coords.end()) return fail("image " + std::to_string(ids[s]) + " has no coordinates (rcn_coords_upload)");
        Ks[s] = it->second.second;
    }
    const int64_t span = ids.empty() ? 0 : (int64_t)ids.back() - ids.front() + 1;
    if (span > (1 << 24)) return fail("image ids span more than 2^24");
    if ((int64_t)ids.size() * (int64_t)ids.size() > (1ll << 28)) return fail("too many images");
    const int32_t ns = (int32_t)ids.size(), lo = ids.empty() ? 0 : ids.front();
    std::vector<int32_t> id2slot((size_t)std::max<int64_t>(span, 1), -1);
    for (int32_t s = 0; s < ns; ++s) id2slot[(size_t)((int64_t)ids[s] - lo)] = s;
    std::vector<int32_t> dir((size_t)std::max(ns, 1) * std::max(ns, 1), -1);
    std::vector<int32_t> stamp_a, stamp_b;
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t a = pairs[2 * p], b = pairs[2 * p + 1];
        if (a == b) return fail("pair (" + std::to_string(a) + ", " + std::to_string(a) + ") pairs an image with itself");
        const int32_t sa = id2slot[(size_t)((int64_t)a - lo)], sb = id2slot[(size_t)((int64_t)b - lo)];
        int32_t &d = dir[(size_t)sa * ns + sb];
        if (d >= 0) return fail("directed pair (" + std::to_string(a) + ", " + std::to_string(b) + ") given twice");
        d = p << 1;
        const int32_t Ka = Ks[sa], Kb = Ks[sb];
        stamp_a.assign((size_t)std::max(Ka, 1), -1);
        stamp_b.assign((size_t)std::max(Kb, 1), -1);
        for (int64_t e = offsets[p]; e < offsets[p + 1]; ++e) {
            const int32_t f = qt[2 * e], g = qt[2 * e + 1];
            if (f < 0 || f >= Ka || g < 0 || g >= Kb) return fail("feature out of range in pair (" + std::to_string(a) + ", " + std::to_string(b) + ")");
            if (stamp_a[f] == p || stamp_b[g] == p) return fail("list of pair (" + std::to_string(a) + ", " + std::to_string(b) + ") is not injective");
            stamp_a[f] = p; stamp_b[g] = p;
        }
    }
    if (mirror)
        for (int32_t sa = 0; sa < ns; ++sa)
            for (int32_t sb = 0; sb < ns; ++sb) {
                int32_t &d = dir[(size_t)sa * ns + sb];
                const int32_t r = dir[(size_t)sb * ns + sa];
                if (d < 0 && r >= 0 && !(r & 1)) d = r | 1;        // the reverse list, read backwards
            }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    RCN_HIP(hipStreamSynchronize(st));
    CorrLists &L = ctx->corr;
    L.release();
    ++ctx->lists_gen;
    RCN_HIP(L.ent.reserve(8 * (size_t)std::max<int64_t>(n_ent, 1)));
    RCN_HIP(L.list_off.reserve(8 * (size_t)(n_pairs + 1)));
    RCN_HIP(L.dir.reserve(4 * dir.size()));
    RCN_HIP(L.id2slot.reserve(4 * id2slot.size()));
    std::vector<int64_t> off(offsets, offsets + n_pairs + (n_pairs > 0 ? 1 : 0));
    if (off.empty()) off.push_back(0);
    if (n_ent) RCN_HIP(hipMemcpyAsync(L.ent.p, qt, 8 * (size_t)n_ent, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(L.list_off.p, off.data(), 8 * off.size(), hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(L.dir.p, dir.data(), 4 * dir.size(), hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(L.id2slot.p, id2slot.data(), 4 * id2slot.size(), hipMemcpyHostToDevice, st));
    RCN_HIP(hipStreamSynchronize(st));           // the host arrays are borrowed / local
    L.ids = std::move(ids);
    L.id_lo = lo;
    L.id_span = (int32_t)span;
    L.mirror = mirror != 0;
    L.n_pairs = n_pairs;
    L.n_ent = n_ent;
    L.coords_gen = ctx->coords_gen;
    L.live = true;
    if (!ctx->corr_ev && hipEventCreateWithFlags(&ctx->corr_ev, hipEventDisableTiming) != hipSuccess) { ctx->corr_ev = nullptr; RCN_HIP(hipGetLastError()); }
    return RCN_OK;
}

int rcn_corr_2d3d_device(rcn_ctx *ctx, int32_t n_points, int32_t n_obs, const int32_t *pt_off_dev, const int32_t *obs_img_dev,
                         const int32_t *obs_feat_dev, int32_t n_cand, const int32_t *cand_dev, const int32_t *cand_shape_dev,
                         int64_t *cand_off_dev, int32_t *out_landmark_dev, int32_t *out_feat_dev, int64_t capacity,
                         int64_t *total_dev, int32_t *out_cells_dev, int32_t *out_outside_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_corr_2d3d_device";
    if (n_points < 0 || n_obs < 0 || n_cand < 0 || capacity < 0 || (n_points > 0 && (!pt_off_dev || (n_obs > 0 && (!obs_img_dev || !obs_feat_dev)))) ||
        (n_cand > 0 && (!cand_dev || !cand_shape_dev || !out_cells_dev)) || !cand_off_dev || !total_dev ||
        (capacity > 0 && (!out_landmark_dev || !out_feat_dev))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->corr.live) { ctx->set_error(std::string(who) + ": no match lists (rcn_match_lists_upload)"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    return corr_launch(ctx, who, n_points, n_obs, pt_off_dev, obs_img_dev, obs_feat_dev, n_cand, cand_dev, cand_shape_dev,
                       cand_off_dev, out_landmark_dev, out_feat_dev, capacity, total_dev, out_cells_dev, out_outside_dev);
}

int rcn_corr_2d3d(rcn_ctx *ctx, int32_t n_points, const int32_t *pt_off, const int32_t *obs_img, const int32_t *obs_feat,
                  int32_t n_cand, const int32_t *cand, const int32_t *cand_shape, int64_t *cand_off,
                  int32_t *out_landmark, int32_t *out_feat, int64_t capacity, int64_t *total_out,
                  int32_t *out_cells, int32_t *out_outside)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_corr_2d3d";
    if (n_points < 0 || n_cand < 0 || capacity < 0 || !pt_off || (n_cand > 0 && (!cand || !cand_shape || !out_cells)) || !cand_off ||
        !total_out || (capacity > 0 && (!out_landmark || !out_feat))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto fail = [&](const std::string &m) { ctx->set_error(std::string(who) + ": " + m); return RCN_ERR_ARG; };
    if (!ctx->corr.live) return fail("no match lists (rcn_match_lists_upload)");
    if (pt_off[0] != 0) return fail("pt_off[0] must be 0");
    for (int32_t p = 0; p < n_points; ++p)
        if (pt_off[p + 1] < pt_off[p]) return fail("pt_off must be non-decreasing");
    const int32_t n_obs = pt_off[n_points];
    if (n_obs > 0 && (!obs_img || !obs_feat)) return fail("obs_img / obs_feat is NULL");
    // every (image, feature) at most once in the graph, features inside the image's coordinates
    std::map<int32_t, std::vector<uint8_t>> seen;
    for (int32_t o = 0; o < n_obs; ++o) {
        auto it = seen.find(obs_img[o]);
        if (it == seen.end()) {
            auto c = ctx->coords.find(obs_img[o]);
            if (c == ctx->coords.end()) return fail("image " + std::to_string(obs_img[o]) + " of the graph has no coordinates (rcn_coords_upload)");
            it = seen.emplace(obs_img[o], std::vector<uint8_t>((size_t)c->second.second, 0)).first;
        }
        const int32_t f = obs_feat[o];
        if (f < 0 || f >= (int32_t)it->second.size()) return fail("feature " + std::to_string(f) + " of image " + std::to_string(obs_img[o]) + " out of range");
        if (it->second[f]) return fail("(image " + std::to_string(obs_img[o]) + ", feature " + std::to_string(f) + ") observed twice in the graph");
        it->second[f] = 1;
    }
    std::vector<int32_t> sc(cand, cand + n_cand);
    std::sort(sc.begin(), sc.end());
    if (std::adjacent_find(sc.begin(), sc.end()) != sc.end()) return fail("a candidate is listed twice");
    for (int32_t k = 0; k < n_cand; ++k) {
        if (!ctx->coords.count(cand[k])) return fail("candidate " + std::to_string(cand[k]) + " has no coordinates (rcn_coords_upload)");
        if (cand_shape[2 * k] <= 0 || cand_shape[2 * k + 1] <= 0) return fail("image shape must be positive");
    }
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t np = n_points, no = n_obs, nc = n_cand;
    const size_t b_off = al256(4 * (np + 1)), b_img = al256(4 * std::max<size_t>(no, 1)), b_cand = al256(4 * std::max<size_t>(nc, 1)),
                 b_shape = al256(8 * std::max<size_t>(nc, 1)), b_coff = al256(8 * (nc + 1)), b_tot = 256;
    const size_t b_lm = al256(4 * (size_t)std::max<int64_t>(capacity, 1));
    RCN_HIP(ctx->corr_hws.reserve(b_off + 2 * b_img + b_cand + b_shape + b_coff + b_tot + 2 * b_cand + 2 * b_lm));
    char *w = ctx->corr_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += b; return q; };
    int32_t *d_off = (int32_t *)take(b_off), *d_img = (int32_t *)take(b_img), *d_feat = (int32_t *)take(b_img);
    int32_t *d_cand = (int32_t *)take(b_cand), *d_shape = (int32_t *)take(b_shape);
    int64_t *d_coff = (int64_t *)take(b_coff), *d_tot = (int64_t *)take(b_tot);
    int32_t *d_cells = (int32_t *)take(b_cand), *d_out = (int32_t *)take(b_cand);
    int32_t *d_lm = (int32_t *)take(b_lm), *d_ft = (int32_t *)take(b_lm);
    RCN_HIP(hipMemcpyAsync(d_off, pt_off, 4 * (np + 1), hipMemcpyHostToDevice, st));
    if (no) {
        RCN_HIP(hipMemcpyAsync(d_img, obs_img, 4 * no, hipMemcpyHostToDevice, st));
        RCN_HIP(hipMemcpyAsync(d_feat, obs_feat, 4 * no, hipMemcpyHostToDevice, st));
    }
    if (nc) {
        RCN_HIP(hipMemcpyAsync(d_cand, cand, 4 * nc, hipMemcpyHostToDevice, st));
        RCN_HIP(hipMemcpyAsync(d_shape, cand_shape, 8 * nc, hipMemcpyHostToDevice, st));
    }
    int rc = corr_launch(ctx, who, n_points, n_obs, d_off, d_img, d_feat, n_cand, d_cand, d_shape, d_coff, d_lm, d_ft, capacity, d_tot,
                         d_cells, d_out);
    if (rc) return rc;
    int64_t total = 0;
    RCN_HIP(hipMemcpyAsync(&total, d_tot, 8, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipMemcpyAsync(cand_off, d_coff, 8 * (nc + 1), hipMemcpyDeviceToHost, st));
    if (nc) {
        RCN_HIP(hipMemcpyAsync(out_cells, d_cells, 4 * nc, hipMemcpyDeviceToHost, st));
        if (out_outside) RCN_HIP(hipMemcpyAsync(out_outside, d_out, 4 * nc, hipMemcpyDeviceToHost, st));
    }
    RCN_HIP(hipStreamSynchronize(st));
    *total_out = total;
    if (total > capacity) return fail("capacity " + std::to_string(capacity) + " < " + std::to_string(total) + " entries (*total_out)");
    if (total) {
        RCN_HIP(hipMemcpyAsync(out_landmark, d_lm, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
        RCN_HIP(hipMemcpyAsync(out_feat, d_ft, 4 * (size_t)total, hipMemcpyDeviceToHost, st));
        RCN_HIP(hipStreamSynchronize(st));
    }
    return RCN_OK;
}

int rcn_landmark_attach(rcn_ctx *ctx, const double *pose34, const double *intr6, int32_t n_points, const double *points, int32_t n,
                        const int32_t *landmark, const int32_t *feat, const int32_t *xy, double max_projection_error,
                        uint8_t *status_out, int32_t *n_attached_out)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_landmark_attach";
    if (!pose34 || !intr6 || n_points < 0 || n < 0 || (n_points > 0 && !points) || (n > 0 && (!landmark || !feat || !xy || !status_out))) {
        ctx->set_error(std::string(who) + ": bad argument");
        return RCN_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->mu);
    int32_t n_feat = 0;
    int rc = rcn_int_attach_check(ctx, who, n_points, n, landmark, feat, &n_feat);
    if (rc) return rc;
    if (n_attached_out) *n_attached_out = 0;
    if (n == 0) return RCN_OK;
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t b_pk = 256, b_pts = al256(24 * (size_t)std::max(n_points, 1)), b_e = al256(4 * (size_t)n), b_st = al256((size_t)n);
    const size_t b_ws = rcn_int_attach_ws_bytes(n_feat);
    RCN_HIP(ctx->att_ws.reserve(b_pk + b_pts + 4 * b_e + b_st + b_ws));
    char *w = ctx->att_ws.as<char>();
    double *d_P = (double *)w, *d_K = (double *)(w + 128); w += b_pk;
    double *d_pts = (double *)w; w += b_pts;
    int32_t *d_lm = (int32_t *)w; w += b_e;
    int32_t *d_ft = (int32_t *)w; w += b_e;
    int32_t *d_xy = (int32_t *)w; w += 2 * b_e;
    uint8_t *d_st = (uint8_t *)w; w += b_st;
    RCN_HIP(hipMemcpyAsync(d_P, pose34, 96, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_K, intr6, 48, hipMemcpyHostToDevice, st));
    if (n_points) RCN_HIP(hipMemcpyAsync(d_pts, points, 24 * (size_t)n_points, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_lm, landmark, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_ft, feat, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    RCN_HIP(hipMemcpyAsync(d_xy, xy, 8 * (size_t)n, hipMemcpyHostToDevice, st));
    rc = rcn_int_attach_launch(ctx, d_P, d_K, d_pts, n_points, n, d_lm, d_ft, d_xy, n_feat, max_projection_error, d_st, w);
    if (rc) return rc;
    RCN_HIP(hipMemcpyAsync(status_out, d_st, (size_t)n, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    if (n_attached_out) *n_attached_out = (int32_t)std::count(status_out, status_out + n, (uint8_t)0);
    return RCN_OK;
}

}  // extern "C"
