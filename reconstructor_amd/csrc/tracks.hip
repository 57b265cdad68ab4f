// tracks.hip -- track building over the resident match lists behind rcn_tracks_* (include/rcn.h).  gfx950, wave64.
//
// A track is a connected component of the graph whose nodes are the (image, feature) pairs of the list images and whose edges are
// the entries of every uploaded list, after the conflict rule, the selection and the length filter (tests/tracks_ref.py is the
// contract).  Node index = node_off[slot] + feature, slots ascending by image id, so node order is (image id, feature) order.
//   T0 k_trk_pairs     the slots (a, b) of every list, read back out of the n_slots x n_slots direction table
//   T1 k_trk_init      parent[x] = x
//   T2 k_trk_hook      one lane per list entry: both roots by path halving, the larger root hooked under the smaller by atomicCAS,
//                      retried from the value the CAS returns.  parent[x] <= x always; a node that has stopped being a root never
//                      becomes one again and a halving store only writes an ancestor, so a stale read only lengthens a walk.
//                      Every parent read in this kernel is a device-scope atomic load.  No lane waits for another.
//   T3 k_trk_flatten   root[x] = the end of x's chain = the smallest node of the component, whatever the interleaving was; sizes
//   T4 k_trk_insert    (root, slot) -> count in an open-addressing table (tracks_key.h) for components of 2 .. n_slots nodes
//                      (DROP_IMAGE: of any size); a second arrival flags the component.  DROP_TRACK: a component of more nodes
//                      than slots conflicts by pigeonhole and never touches the table
//   T5 k_trk_survive   per node: conflict rule, selection; survivors counted per root, the smallest survivor by atomicMin
//   T6-T8 k_trk_scan*  the head of a kept track is its smallest survivor: track index and first observation by a two-level scan
//                      over the nodes (wg_scan_incl per 1024 nodes, wg_scan_array over the block sums); the counts, the statistics
//   T9 k_trk_scatter   survivors into their track's segment of the workspace, in arrival order
//   T10 k_trk_sort_wave / T11 k_trk_sort_wg   every segment ascending by node: one wavefront ranks a track of up to 64, one workgroup
//                      sorts a longer one in LDS (a surviving track holds at most one observation per list image: 16384 words);
//                      the sorted nodes are written out as (image, feature, camera, pixel), whole tracks only
//   T12 k_trk_tail     trk_off past the last written track repeats its end
// Integer sums, minima and maxima only: the outputs do not depend on arrival order, launch geometry or timing.
#include "rcn_internal.h"
#include "tracks_key.h"
#include "wgprim.h"

#include <algorithm>
#include <climits>

namespace {

constexpr int TB = 256;                  // threads per workgroup of the per-node and per-entry kernels (4 waves)
constexpr int SB = 1024;                 // nodes per workgroup of the scans (16 waves)
constexpr int SORT_GRID = 1024;          // workgroups of the two sort kernels (they stride over the tracks)

struct TrkSlot {                         // one list image
    const int32_t *xy;                   // K x 2 resident pixels
    int32_t K, node_off;                 // keypoints, first node
    int32_t cam;                         // camera row of a selected image (0 without a selection), -1: not selected
    int32_t img;                         // image id
};

struct TrkArgs {
    const TrkSlot *slots;
    const int2 *ent;
    const int64_t *list_off;
    const int32_t *dir;
    int2 *pslot;                         // slots (a, b) per list
    int64_t n_ent;
    int32_t ns, n_nodes, n_pairs, n_blocks;
    int32_t *parent;                     // T1-T3; from T9 on the tracks' segments
    int32_t *root, *csize;               // csize: nodes per root; from T8 on the scatter cursor of a kept track
    int32_t *nsurv, *first, *cflag, *tidx, *toff, *trk_root;
    uint8_t *alive;
    unsigned long long *keys;
    int32_t *kcnt;
    unsigned long long cells;
    int32_t *blk_trk, *blk_obs;
    int32_t *long_list;
    int32_t *scal;                       // [0] tracks longer than a wavefront, [1] written tracks, [2] their last observation's end
    unsigned long long *stat;            // the statistics as they accumulate
    int32_t min_len, max_len, policy;
    int32_t cap_tracks, cap_obs;
    int32_t *counts, *trk_off, *obs_img, *obs_feat, *obs_cam, *obs_xy, *feat_track;
    int64_t *stats_out;
};

__device__ __forceinline__ int ld_dev(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_dev(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x as far as this lane can see, halving the path on the way (parent[x] = its grandparent, then on from there)
__device__ __forceinline__ int trk_find(int32_t *parent, int x)
{
    for (;;) {
        const int p = ld_dev(parent + x);
        if (p == x) return x;
        const int g = ld_dev(parent + p);
        if (g == p) return p;
        st_dev(parent + x, g);
        x = g;
    }
}

// the slot of node x: the last one whose first node is <= x (empty slots share their first node with the next one)
__device__ __forceinline__ int trk_slot_of(const TrkSlot *slots, int ns, int x)
{
    int lo = 0, hi = ns;                 // first slot with node_off > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (slots[mid].node_off > x) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

__device__ __forceinline__ bool trk_len_ok(const TrkArgs &a, int n) { return n >= a.min_len && (a.max_len == 0 || n <= a.max_len); }

__global__ __launch_bounds__(TB) void k_trk_pairs(TrkArgs a)
{
    const int64_t c = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (c >= (int64_t)a.ns * a.ns) return;
    const int d = a.dir[c];
    if (d < 0 || (d & 1)) return;        // no list, or the reverse list read backwards (mirror): not a list of its own
    const int p = d >> 1;
    if (p < a.n_pairs) a.pslot[p] = make_int2((int)(c / a.ns), (int)(c % a.ns));
}

__global__ __launch_bounds__(TB) void k_trk_init(TrkArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (x < a.n_nodes) a.parent[x] = (int)x;
}

__global__ __launch_bounds__(TB) void k_trk_hook(TrkArgs a)
{
    const int64_t e = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (e >= a.n_ent) return;
    int lo = 0, hi = a.n_pairs - 1;      // the list of entry e: the first p with list_off[p + 1] > e
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.list_off[mid + 1] > e) hi = mid; else lo = mid + 1;
    }
    const int2 ps = a.pslot[lo];
    const int2 m = a.ent[e];
    const TrkSlot sa = a.slots[ps.x], sb = a.slots[ps.y];
    if ((unsigned)m.x >= (unsigned)sa.K || (unsigned)m.y >= (unsigned)sb.K) return;      // (the upload checked it against these row counts)
    int u = sa.node_off + m.x, v = sb.node_off + m.y;
    for (;;) {
        u = trk_find(a.parent, u);
        v = trk_find(a.parent, v);
        if (u == v) break;
        const int big = max(u, v), small = min(u, v);
        const int old = atomicCAS(a.parent + big, big, small);
        if (old == big) break;           // big was still a root: hooked
        u = old; v = small;              // somebody else hooked it first: on from where they put it
    }
}

__global__ __launch_bounds__(TB) void k_trk_flatten(TrkArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (x >= a.n_nodes) return;
    int r = (int)x, p;
    while ((p = a.parent[r]) != r) r = p;
    a.root[x] = r;
    atomicAdd(a.csize + r, 1);
}

__global__ __launch_bounds__(TB) void k_trk_insert(TrkArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (x >= a.n_nodes) return;
    const int r = a.root[x], sz = a.csize[r];
    if (sz < 2) return;
    if (a.policy == RCN_TRACKS_CONFLICT_DROP_TRACK && sz > a.ns) { a.cflag[r] = 1; return; }      // pigeonhole
    const unsigned long long key = trk_key(r, trk_slot_of(a.slots, a.ns, (int)x));
    unsigned long long c = trk_cell(key, a.cells);
    for (;;) {
        const unsigned long long old = atomicCAS(a.keys + c, TRK_EMPTY, key);
        if (old == TRK_EMPTY || old == key) break;
        c = trk_next_cell(c, a.cells);
    }
    if (atomicAdd(a.kcnt + c, 1) >= 1) a.cflag[r] = 1;      // the image's second feature in this component
}

__global__ __launch_bounds__(TB) void k_trk_survive(TrkArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    bool dropped4 = false, alive = false;
    int r = 0;
    if (x < a.n_nodes) {
        r = a.root[x];
        if (a.csize[r] >= 2) {
            const int s = trk_slot_of(a.slots, a.ns, (int)x);
            if (a.policy == RCN_TRACKS_CONFLICT_DROP_TRACK) dropped4 = a.cflag[r] != 0;
            else if (a.cflag[r]) {
                const unsigned long long key = trk_key(r, s);
                unsigned long long c = trk_cell(key, a.cells);
                for (;;) {
                    const unsigned long long k = a.keys[c];
                    if (k == key) { dropped4 = a.kcnt[c] >= 2; break; }
                    if (k == TRK_EMPTY) break;
                    c = trk_next_cell(c, a.cells);
                }
            }
            alive = !dropped4 && a.slots[s].cam >= 0;
        }
        a.alive[x] = alive ? 1 : 0;
        if (alive) { atomicAdd(a.nsurv + r, 1); atomicMin(a.first + r, (int)x); }
    }
    const unsigned long long m = __ballot(dropped4);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(a.stat + 2, (unsigned long long)__popcll(m));
}

// is node x the head (smallest survivor) of a kept track?  n = that track's observations
__device__ __forceinline__ bool trk_head(const TrkArgs &a, int64_t x, int &r, int &n)
{
    r = 0; n = 0;
    if (x >= a.n_nodes || !a.alive[x]) return false;
    r = a.root[x];
    if (a.first[r] != (int)x) return false;
    n = a.nsurv[r];
    if (!trk_len_ok(a, n)) { n = 0; return false; }
    return true;
}

__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(SB) void k_trk_scan1(TrkArgs a)
{
    __shared__ int sh[SB / 64];
    const int64_t x = (int64_t)blockIdx.x * SB + threadIdx.x;
    // the statistics, at the roots
    const bool is_root = x < a.n_nodes && a.root[x] == (int)x;
    const int sz = is_root ? a.csize[x] : 0;
    const bool comp2 = sz >= 2, cf = comp2 && a.cflag[x] != 0;
    const bool whole = cf && a.policy == RCN_TRACKS_CONFLICT_DROP_TRACK;
    const int ns = comp2 ? a.nsurv[x] : 0;
    const bool kept = comp2 && !whole && trk_len_ok(a, ns), drop6 = comp2 && !whole && !kept;
    const unsigned long long m0 = __ballot(comp2), m1 = __ballot(cf), m3 = __ballot(drop6);
    const int mx_sz = wave_max(sz), mx_len = wave_max(kept ? ns : 0);
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicAdd(a.stat + 0, (unsigned long long)__popcll(m0));
        if (m1) atomicAdd(a.stat + 1, (unsigned long long)__popcll(m1));
        if (m3) atomicAdd(a.stat + 3, (unsigned long long)__popcll(m3));
        if (mx_sz) atomicMax(a.stat + 4, (unsigned long long)mx_sz);
        if (mx_len) atomicMax(a.stat + 5, (unsigned long long)mx_len);
    }
    // the heads
    int r, n, tot_t, tot_o;
    const bool head = trk_head(a, x, r, n);
    wg_scan_incl<int, SB>(head ? 1 : 0, sh, tot_t);
    wg_scan_incl<int, SB>(n, sh, tot_o);
    if (threadIdx.x == 0) { a.blk_trk[blockIdx.x] = tot_t; a.blk_obs[blockIdx.x] = tot_o; }
}

__global__ __launch_bounds__(1024) void k_trk_scan2(TrkArgs a)
{
    const int32_t nt = wg_scan_array<int32_t, int32_t>(a.blk_trk, a.n_blocks, a.blk_trk, 0);
    const int32_t no = wg_scan_array<int32_t, int32_t>(a.blk_obs, a.n_blocks, a.blk_obs, 0);
    const int t = threadIdx.x;
    if (t == 0) { a.counts[0] = nt; a.counts[1] = no; }
    if (a.stats_out && t < 8) a.stats_out[t] = t == 6 ? a.n_ent : t == 7 ? 0 : (int64_t)a.stat[t];
}

__global__ __launch_bounds__(SB) void k_trk_scan3(TrkArgs a)
{
    __shared__ int sh[SB / 64];
    const int64_t x = (int64_t)blockIdx.x * SB + threadIdx.x;
    int r, n, tot;
    const bool head = trk_head(a, x, r, n);
    const int j = a.blk_trk[blockIdx.x] + wg_scan_incl<int, SB>(head ? 1 : 0, sh, tot) - (head ? 1 : 0);
    const int off = a.blk_obs[blockIdx.x] + wg_scan_incl<int, SB>(n, sh, tot) - n;
    if (!head) return;
    a.tidx[r] = j;
    a.toff[r] = off;
    a.trk_root[j] = r;
    a.csize[r] = 0;                      // the scatter's cursor
    if (j < a.cap_tracks && (int64_t)off + n <= a.cap_obs) {      // tracks ascend in both, so this is "tracks 0 .. j fit"
        a.trk_off[j] = off;
        atomicMax(a.scal + 1, j + 1);
        atomicMax(a.scal + 2, off + n);
    }
}

__global__ __launch_bounds__(TB) void k_trk_scatter(TrkArgs a)
{
    const int64_t x = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (x >= a.n_nodes || !a.alive[x]) return;
    const int r = a.root[x];
    if (a.tidx[r] < 0) return;
    a.parent[a.toff[r] + atomicAdd(a.csize + r, 1)] = (int)x;
}

// observation k of track j (first observation off, n in all) is node x
__device__ __forceinline__ void trk_emit(const TrkArgs &a, int j, int off, int n, int k, int x)
{
    if (j >= a.cap_tracks || (int64_t)off + n > a.cap_obs) return;
    const TrkSlot s = a.slots[trk_slot_of(a.slots, a.ns, x)];
    const int f = x - s.node_off;
    const size_t o = (size_t)off + k;
    a.obs_img[o] = s.img;
    a.obs_feat[o] = f;
    if (a.obs_cam) a.obs_cam[o] = s.cam;
    if (a.obs_xy) { a.obs_xy[2 * o] = s.xy[2 * (size_t)f]; a.obs_xy[2 * o + 1] = s.xy[2 * (size_t)f + 1]; }
    if (a.feat_track) a.feat_track[x] = j;
}

__global__ __launch_bounds__(TB) void k_trk_sort_wave(TrkArgs a)
{
    const int lane = threadIdx.x & 63;
    const int nw = gridDim.x * (TB / 64), nt = a.counts[0];
    for (int j = blockIdx.x * (TB / 64) + (threadIdx.x >> 6); j < nt; j += nw) {
        const int r = a.trk_root[j], n = a.nsurv[r], off = a.toff[r];
        if (n > 64) {
            if (lane == 0) a.long_list[atomicAdd(a.scal + 0, 1)] = j;
            continue;
        }
        const int v = lane < n ? a.parent[off + lane] : INT_MAX;
        int rank = 0;
        for (int i = 0; i < n; ++i) rank += __shfl(v, i) < v ? 1 : 0;      // the nodes of a track are distinct
        if (lane < n) trk_emit(a, j, off, n, rank, v);
    }
}

__global__ __launch_bounds__(TB) void k_trk_sort_wg(TrkArgs a)
{
    __shared__ int32_t s[TRK_MAX_SLOTS];                  // 64 KiB
    const int t = threadIdx.x, n_long = a.scal[0];
    for (int i = blockIdx.x; i < n_long; i += gridDim.x) {
        const int j = a.long_list[i], r = a.trk_root[j], n = a.nsurv[r], off = a.toff[r];
        if (n > TRK_MAX_SLOTS) continue;                  // (cannot be: one observation per list image)
        int P = 128;
        while (P < n) P <<= 1;
        for (int k = t; k < P; k += TB) s[k] = k < n ? a.parent[off + k] : INT_MAX;
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int q = k >> 1; q > 0; q >>= 1) {
                for (int e = t; e < P; e += TB) {
                    const int p = e ^ q;
                    if (p > e) {
                        const int u = s[e], v = s[p];
                        if ((u > v) == ((e & k) == 0)) { s[e] = v; s[p] = u; }
                    }
                }
                __syncthreads();
            }
        for (int k = t; k < n; k += TB) trk_emit(a, j, off, n, k, s[k]);
        __syncthreads();
    }
}

__global__ __launch_bounds__(TB) void k_trk_tail(TrkArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * TB + threadIdx.x;
    if (j <= a.cap_tracks && j >= a.scal[1]) a.trk_off[j] = a.scal[2];
}

size_t al256(size_t b) { return (b + 255) / 256 * 256; }
unsigned nblk(int64_t n, int per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

int trk_fail(rcn_ctx *ctx, const char *who, const std::string &m, int rc = RCN_ERR_ARG) { ctx->set_error(std::string(who) + ": " + m); return rc; }

// the list images' row counts as the coordinates stand, behind the check that they are the ones the lists were uploaded against
int trk_layout(rcn_ctx *ctx, const char *who, std::vector<int64_t> &node_off)
{
    const CorrLists &L = ctx->corr;
    if (!L.live) return trk_fail(ctx, who, "no match lists (rcn_match_lists_upload)");
    if (L.coords_gen != ctx->coords_gen) return trk_fail(ctx, who, "the coordinates changed since the match lists were uploaded (rcn_match_lists_upload again)");
    node_off.assign(L.ids.size() + 1, 0);
    for (size_t s = 0; s < L.ids.size(); ++s) {
        auto it = ctx->coords.find(L.ids[s]);
        if (it == ctx->coords.end()) return trk_fail(ctx, who, "coordinates of image " + std::to_string(L.ids[s]) + " are no longer resident");
        node_off[s + 1] = node_off[s] + it->second.second;
    }
    if (node_off.back() > (int64_t)INT32_MAX) return trk_fail(ctx, who, "more than 2^31 - 1 nodes");
    return RCN_OK;
}

int trk_check_options(rcn_ctx *ctx, const char *who, const rcn_tracks_options *opt, rcn_tracks_options &o)
{
    rcn_tracks_default_options(&o);
    if (opt) o = *opt;
    if (o.min_length < 2) return trk_fail(ctx, who, "min_length must be at least 2");
    if (o.max_length < 0 || (o.max_length > 0 && o.max_length < o.min_length)) return trk_fail(ctx, who, "max_length is 0 (no limit) or at least min_length");
    if (o.conflict != RCN_TRACKS_CONFLICT_DROP_TRACK && o.conflict != RCN_TRACKS_CONFLICT_DROP_IMAGE) return trk_fail(ctx, who, "unknown conflict policy");
    if (o.reserved != 0) return trk_fail(ctx, who, "the reserved option word must be 0");
    return RCN_OK;
}

// everything with ctx->mu held, all output pointers in HBM
int trk_launch(rcn_ctx *ctx, const char *who, const rcn_tracks_options *opt, int32_t n_sel, const int32_t *sel_img, const int32_t *sel_cam,
               int32_t cap_tracks, int32_t cap_obs, int32_t *counts, int32_t *trk_off, int32_t *obs_img, int32_t *obs_feat, int32_t *obs_cam,
               int32_t *obs_xy, int32_t *feat_track, int64_t *stats)
{
    CorrLists &L = ctx->corr;
    if (n_sel < 0 || cap_tracks < 0 || cap_obs < 0 || !counts || !trk_off || (n_sel > 0 && (!sel_img || !sel_cam)) ||
        (cap_obs > 0 && (!obs_img || !obs_feat)))
        return trk_fail(ctx, who, "bad argument");
    if (n_sel == 0 && obs_cam) return trk_fail(ctx, who, "camera rows without a selection (obs_cam must be NULL when n_sel is 0)");
    rcn_tracks_options o;
    int rc = trk_check_options(ctx, who, opt, o);
    if (rc) return rc;
    std::vector<int64_t> node_off;
    rc = trk_layout(ctx, who, node_off);
    if (rc) return rc;
    const int32_t ns = (int32_t)L.ids.size();
    if (ns > TRK_MAX_SLOTS) return trk_fail(ctx, who, "more than 16384 list images");
    const int64_t N = node_off.back(), n_ent = L.n_ent;

    // ---- the slot / selection table: the one staged copy
    if (ctx->trk_stage_pending) { RCN_HIP(hipEventSynchronize(ctx->trk_ev)); ctx->trk_stage_pending = false; }      // the staging buffer is free again
    ctx->trk_stage_host.resize((size_t)std::max(ns, 1) * sizeof(TrkSlot));
    TrkSlot *sd = reinterpret_cast<TrkSlot *>(ctx->trk_stage_host.data());
    for (int32_t s = 0; s < ns; ++s) {
        auto &c = ctx->coords.find(L.ids[s])->second;         // trk_layout found it
        sd[s] = TrkSlot{c.first.as<int32_t>(), c.second, (int32_t)node_off[s], n_sel == 0 ? 0 : -1, L.ids[s]};
    }
    for (int32_t k = 0; k < n_sel; ++k) {
        auto it = std::lower_bound(L.ids.begin(), L.ids.end(), sel_img[k]);
        if (it == L.ids.end() || *it != sel_img[k]) return trk_fail(ctx, who, "selected image " + std::to_string(sel_img[k]) + " is not among the resident lists' images", RCN_ERR_NOT_FOUND);
        if (sel_cam[k] < 0) return trk_fail(ctx, who, "negative camera row for image " + std::to_string(sel_img[k]));
        TrkSlot &t = sd[it - L.ids.begin()];
        if (t.cam >= 0) return trk_fail(ctx, who, "selected image " + std::to_string(sel_img[k]) + " is listed twice");
        t.cam = sel_cam[k];
    }
    hipStream_t st = ctx->stream;
    if (!ctx->trk_ev && hipEventCreateWithFlags(&ctx->trk_ev, hipEventDisableTiming) != hipSuccess) { ctx->trk_ev = nullptr; RCN_HIP(hipGetLastError()); }
    for (auto &e : ctx->trk_tev)
        if (!e && hipEventCreate(&e) != hipSuccess) { e = nullptr; RCN_HIP(hipGetLastError()); }
    RCN_HIP(ctx->trk_slots.reserve((size_t)std::max(ns, 1) * sizeof(TrkSlot)));

    // ---- workspace: 37 bytes per node, 8 per list, 12 per table cell (at most 4 min(nodes, 2 entries) cells), 8 per 1024 nodes
    const size_t n1 = (size_t)std::max<int64_t>(N, 1);
    const unsigned long long cells = trk_table_cells((unsigned long long)std::min<int64_t>(N, 2 * n_ent));
    const int32_t n_blocks = (int32_t)nblk(N, SB);
    const size_t b_node = al256(4 * n1), b_alive = al256(n1), b_pslot = al256(8 * (size_t)std::max(L.n_pairs, 1)), b_keys = al256(8 * (size_t)cells),
                 b_kcnt = al256(4 * (size_t)cells), b_blk = al256(4 * (size_t)n_blocks), b_long = al256(4 * (n1 / 64 + 1)), b_small = 256;
    RCN_HIP(ctx->trk_ws.reserve(9 * b_node + b_alive + b_pslot + b_keys + b_kcnt + 2 * b_blk + b_long + b_small));
    char *w = ctx->trk_ws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += b; return q; };
    TrkArgs a;
    a.slots = ctx->trk_slots.as<TrkSlot>();
    a.ent = L.ent.as<int2>(); a.list_off = L.list_off.as<int64_t>(); a.dir = L.dir.as<int32_t>();
    a.n_ent = n_ent; a.ns = ns; a.n_nodes = (int32_t)N; a.n_pairs = L.n_pairs; a.n_blocks = n_blocks;
    a.parent = (int32_t *)take(b_node); a.root = (int32_t *)take(b_node); a.trk_root = (int32_t *)take(b_node);
    a.toff = (int32_t *)take(b_node);
    a.csize = (int32_t *)take(b_node); a.nsurv = (int32_t *)take(b_node); a.cflag = (int32_t *)take(b_node);      // zeroed together
    a.tidx = (int32_t *)take(b_node); a.first = (int32_t *)take(b_node);
    a.alive = (uint8_t *)take(b_alive);
    a.pslot = (int2 *)take(b_pslot);
    a.keys = (unsigned long long *)take(b_keys); a.kcnt = (int32_t *)take(b_kcnt); a.cells = cells;
    a.blk_trk = (int32_t *)take(b_blk); a.blk_obs = (int32_t *)take(b_blk);
    a.long_list = (int32_t *)take(b_long);
    a.scal = (int32_t *)take(b_small);
    a.stat = reinterpret_cast<unsigned long long *>(a.scal + 16);      // 64 bytes into the same 256
    a.min_len = o.min_length; a.max_len = o.max_length; a.policy = o.conflict;
    a.cap_tracks = cap_tracks; a.cap_obs = cap_obs;
    a.counts = counts; a.trk_off = trk_off; a.obs_img = obs_img; a.obs_feat = obs_feat; a.obs_cam = obs_cam; a.obs_xy = obs_xy;
    a.feat_track = feat_track; a.stats_out = stats;

    if (ns) {
        RCN_HIP(hipMemcpyAsync(ctx->trk_slots.p, sd, (size_t)ns * sizeof(TrkSlot), hipMemcpyHostToDevice, st));
        RCN_HIP(hipEventRecord(ctx->trk_ev, st));
        ctx->trk_stage_pending = true;
    }
    RCN_HIP(hipMemsetAsync(a.csize, 0, 3 * b_node, st));
    RCN_HIP(hipMemsetAsync(a.tidx, 0xFF, b_node, st));
    RCN_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.first), INT32_MAX, n1, st));
    RCN_HIP(hipMemsetAsync(a.keys, 0xFF, b_keys, st));
    RCN_HIP(hipMemsetAsync(a.kcnt, 0, b_kcnt, st));
    RCN_HIP(hipMemsetAsync(a.scal, 0, b_small, st));
    if (feat_track && N) RCN_HIP(hipMemsetAsync(feat_track, 0xFF, 4 * (size_t)N, st));
    const unsigned nb_node = nblk(N, TB);
    if (ns && L.n_pairs) k_trk_pairs<<<nblk((int64_t)ns * ns, TB), TB, 0, st>>>(a);
    k_trk_init<<<nb_node, TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[0], st));
    if (n_ent && L.n_pairs) k_trk_hook<<<nblk(n_ent, TB), TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[1], st));
    k_trk_flatten<<<nb_node, TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[2], st));
    k_trk_insert<<<nb_node, TB, 0, st>>>(a);
    k_trk_survive<<<nb_node, TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[3], st));
    k_trk_scan1<<<(unsigned)n_blocks, SB, 0, st>>>(a);
    k_trk_scan2<<<1, 1024, 0, st>>>(a);
    k_trk_scan3<<<(unsigned)n_blocks, SB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[4], st));
    k_trk_scatter<<<nb_node, TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[5], st));
    k_trk_sort_wave<<<SORT_GRID, TB, 0, st>>>(a);
    k_trk_sort_wg<<<SORT_GRID, TB, 0, st>>>(a);
    k_trk_tail<<<nblk((int64_t)cap_tracks + 1, TB), TB, 0, st>>>(a);
    RCN_HIP(hipEventRecord(ctx->trk_tev[6], st));
    RCN_HIP(hipGetLastError());
    ctx->trk_timed = true;
    return RCN_OK;
}

}  // namespace

void rcn_int_tracks_release(rcn_ctx *ctx)
{
    ctx->trk_ws.release(); ctx->trk_slots.release(); ctx->trk_hws.release();
    if (ctx->trk_ev) (void)hipEventDestroy(ctx->trk_ev);
    for (auto &e : ctx->trk_tev)
        if (e) (void)hipEventDestroy(e);
}

extern "C" {

void rcn_tracks_default_options(rcn_tracks_options *opt)
{
    if (!opt) return;
    opt->min_length = 2;
    opt->max_length = 0;
    opt->conflict = RCN_TRACKS_CONFLICT_DROP_TRACK;
    opt->reserved = 0;
}

int rcn_tracks_layout(rcn_ctx *ctx, int32_t *img_ids_out, int64_t *node_off_out, int32_t *n_images_out)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_tracks_layout";
    if (!n_images_out) { ctx->set_error(std::string(who) + ": bad argument"); return RCN_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    std::vector<int64_t> node_off;
    int rc = trk_layout(ctx, who, node_off);
    if (rc) return rc;
    const CorrLists &L = ctx->corr;
    *n_images_out = (int32_t)L.ids.size();
    if (img_ids_out) std::copy(L.ids.begin(), L.ids.end(), img_ids_out);
    if (node_off_out) std::copy(node_off.begin(), node_off.end(), node_off_out);
    return RCN_OK;
}

int rcn_tracks_build_device(rcn_ctx *ctx, const rcn_tracks_options *opt, int32_t n_sel, const int32_t *sel_img_host,
                            const int32_t *sel_cam_host, int32_t cap_tracks, int32_t cap_obs, int32_t *counts_dev,
                            int32_t *trk_off_dev, int32_t *obs_img_dev, int32_t *obs_feat_dev, int32_t *obs_cam_dev,
                            int32_t *obs_xy_dev, int32_t *feat_track_dev, int64_t *stats_dev)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    RCN_HIP(hipSetDevice(ctx->device));
    return trk_launch(ctx, "rcn_tracks_build_device", opt, n_sel, sel_img_host, sel_cam_host, cap_tracks, cap_obs, counts_dev, trk_off_dev,
                      obs_img_dev, obs_feat_dev, obs_cam_dev, obs_xy_dev, feat_track_dev, stats_dev);
}

int rcn_tracks_build(rcn_ctx *ctx, const rcn_tracks_options *opt, int32_t n_sel, const int32_t *sel_img, const int32_t *sel_cam,
                     int32_t cap_tracks, int32_t cap_obs, int32_t *counts_out, int32_t *trk_off_out, int32_t *obs_img_out,
                     int32_t *obs_feat_out, int32_t *obs_cam_out, int32_t *obs_xy_out, int32_t *feat_track_out, int64_t *stats_out)
{
    if (!ctx) return RCN_ERR_ARG;
    const char *who = "rcn_tracks_build";
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (cap_tracks < 0 || cap_obs < 0 || !counts_out || !trk_off_out || (cap_obs > 0 && (!obs_img_out || !obs_feat_out)))
        return trk_fail(ctx, who, "bad argument");
    if (n_sel == 0 && obs_cam_out) return trk_fail(ctx, who, "camera rows without a selection (obs_cam must be NULL when n_sel is 0)");
    std::vector<int64_t> node_off;
    int rc = trk_layout(ctx, who, node_off);
    if (rc) return rc;
    RCN_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t N = (size_t)node_off.back(), ct = (size_t)cap_tracks, co = (size_t)std::max(cap_obs, 1);
    const size_t b_cnt = 256, b_off = al256(4 * (ct + 1)), b_obs = al256(4 * co), b_ft = al256(4 * std::max<size_t>(N, 1));
    RCN_HIP(ctx->trk_hws.reserve(2 * b_cnt + b_off + 5 * b_obs + b_ft));
    char *w = ctx->trk_hws.as<char>();
    auto take = [&](size_t b) { char *q = w; w += b; return q; };
    int32_t *d_cnt = (int32_t *)take(b_cnt);
    int64_t *d_stats = (int64_t *)take(b_cnt);
    int32_t *d_off = (int32_t *)take(b_off), *d_img = (int32_t *)take(b_obs), *d_feat = (int32_t *)take(b_obs), *d_cam = (int32_t *)take(b_obs);
    int32_t *d_xy = (int32_t *)take(2 * b_obs), *d_ft = (int32_t *)take(b_ft);
    rc = trk_launch(ctx, who, opt, n_sel, sel_img, sel_cam, cap_tracks, cap_obs, d_cnt, d_off, d_img, d_feat, obs_cam_out ? d_cam : nullptr,
                    obs_xy_out ? d_xy : nullptr, feat_track_out ? d_ft : nullptr, stats_out ? d_stats : nullptr);
    if (rc) return rc;
    RCN_HIP(hipMemcpyAsync(counts_out, d_cnt, 8, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    const int32_t nt = counts_out[0], no = counts_out[1];
    if (nt > cap_tracks || no > cap_obs)
        return trk_fail(ctx, who, "capacity (" + std::to_string(cap_tracks) + " tracks, " + std::to_string(cap_obs) + " observations) < the result's " +
                                      std::to_string(nt) + " tracks, " + std::to_string(no) + " observations (counts_out)");
    RCN_HIP(hipMemcpyAsync(trk_off_out, d_off, 4 * (ct + 1), hipMemcpyDeviceToHost, st));
    if (no) {
        RCN_HIP(hipMemcpyAsync(obs_img_out, d_img, 4 * (size_t)no, hipMemcpyDeviceToHost, st));
        RCN_HIP(hipMemcpyAsync(obs_feat_out, d_feat, 4 * (size_t)no, hipMemcpyDeviceToHost, st));
        if (obs_cam_out) RCN_HIP(hipMemcpyAsync(obs_cam_out, d_cam, 4 * (size_t)no, hipMemcpyDeviceToHost, st));
        if (obs_xy_out) RCN_HIP(hipMemcpyAsync(obs_xy_out, d_xy, 8 * (size_t)no, hipMemcpyDeviceToHost, st));
    }
    if (feat_track_out && N) RCN_HIP(hipMemcpyAsync(feat_track_out, d_ft, 4 * N, hipMemcpyDeviceToHost, st));
    if (stats_out) RCN_HIP(hipMemcpyAsync(stats_out, d_stats, 64, hipMemcpyDeviceToHost, st));
    RCN_HIP(hipStreamSynchronize(st));
    return RCN_OK;
}

int rcn_tracks_last_phase_ms(rcn_ctx *ctx, double *ms_out6)
{
    if (!ctx) return RCN_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ms_out6 || !ctx->trk_timed) { ctx->set_error("rcn_tracks_last_phase_ms: no build to report"); return RCN_ERR_ARG; }
    RCN_HIP(hipSetDevice(ctx->device));
    RCN_HIP(hipEventSynchronize(ctx->trk_tev[6]));
    for (int k = 0; k < 6; ++k) {
        float ms = 0.f;
        RCN_HIP(hipEventElapsedTime(&ms, ctx->trk_tev[k], ctx->trk_tev[k + 1]));
        ms_out6[k] = ms;
    }
    return RCN_OK;
}

}  // extern "C"
