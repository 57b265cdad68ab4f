// rcn_internal.h -- shared host-side state of the C ABI (include/rcn.h).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rcn.h"
#include "grid_plan.h"

#define RCN_HIP(call)                                                                    \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess) {                                                          \
            ctx->set_error(std::string(#call) + ": " + hipGetErrorString(e_));           \
            return RCN_ERR_HIP;                                                          \
        }                                                                                \
    } while (0)

// One growable device buffer; never shrinks; no allocation once large enough.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
#include "chol.h"      // CholState holds DevBufs

// Per-image device record (mirrored in a device table for the kernels).
struct ImgDev {
    const float *f32;      // [K][D]      original rows (exact re-rank reads these)
    const _Float16 *f16;   // [Kp][DP]    scaled by the global power of two, 16-B chunks XOR-swizzled; int8 path (ScaleDev::coarse_i8): int8 [Kp][256] in the
                           //             same allocation, rint(s x), same swizzle idea (256-byte rows)
    const float *hn;       // [Kp]        0.5*s^2*|t|^2 + BIAS ; padded rows = huge; int8 path: int32 rint(s^2 |t|^2 / 2) + BIAS, padded rows 2^20 - 1
    const double *nrm2;    // [K]         |x|^2 in fp64
    const unsigned long long *bigmin;   // bits of the smallest |x|^2 among this image's BIG rows (+infinity: it has none)
    int32_t K, Kp;
    const float2 *i8n;     // [Kp]        int8 path only: (|xq|, |s x - xq|) of the row, both rounded UP (k_prepare_i8)
};

struct ImgHost {
    float *f32 = nullptr;
    _Float16 *f16 = nullptr;
    float *hn = nullptr;
    double *nrm2 = nullptr;
    unsigned long long *bigmin = nullptr;
    float2 *i8n = nullptr;
    int32_t K = 0, Kp = 0;
    int32_t slot = -1;  // row in the device image table
    int32_t slab = -1;  // >= 0: buffers are views into ctx->slabs[slab] (batch upload)
    int32_t cap_rows = 0, cap_D = 0;   // capacity of the owned allocations
    bool dirty = true;  // fp16 copy / half-norms not yet built for the current scale
};

// One batch of equally shaped images (rcn_desc_upload_batch_device): one allocation per array.
struct Slab {
    int32_t first_id = 0, n = 0, K = 0, Kp = 0, D = 0;   // n = slots of the block (>= n_images)
    int32_t n_images = 0;                 // ids first_id .. first_id + n_images - 1 live in slots 0 .. n_images - 1
    int32_t conv_first = 0, conv_n = 0;   // slots this ctx converts to fp16 itself (the rest arrives by all-gather)
    const float *f32 = nullptr;   // borrowed from the caller
    const int32_t *Ks_dev = nullptr;   // borrowed: rows in use per slot when the images are ragged (NULL = K everywhere)
    float *own_f32 = nullptr;          // rcn_desc_upload_batch: the block of fp32 rows belongs to the slab (f32 points into it)
    int32_t *own_Ks = nullptr;         // ... and so do the per-slot row counts (Ks_dev points at them)
    _Float16 *f16 = nullptr;
    float *hn = nullptr;
    double *nrm2 = nullptr;
    unsigned long long *bigmin = nullptr;   // [n] one word per slot
    float2 *i8n = nullptr;                  // [n][Kp] quantised / residual norms of the int8 path
    bool live = false;
};

// ctx->counters (words): [0] max |x| bits, [2..3] max |x|^2 bits, [8..15] per-chunk list counts, [16] / [17] int8 path: fp32 bits of the largest
// residual norm / quantised norm over the rows converted at the scale in force, then the histogram of rows per octave of |x|^2
// (match.hip, k_rowstats / fix_scale)
#define RCN_I8_WORD 16
#define RCN_HIST_BINS 512
#define RCN_HIST_WORD 64
#define RCN_COUNTER_BYTES ((RCN_HIST_WORD + RCN_HIST_BINS) * 4)

// The global fp16 scale and what follows from it, kept in HBM: fixed either by the host
// (rcn_int_prepare_all, after reading the row statistics) or by k_fix_scale on the device (the sharded exchange,
// which must not wait for the host between its collectives).  Every kernel that needs a constant reads it here.
struct ScaleDev {
    double s;           // power of two
    double s2;          // s^2
    double hs2;         // s^2 / 2
    double bias;        // BIAS, accumulator units
    double c_in;        // (2u+u^2) s^2            x |q| Nmax
    double c_sub;       // 2^-14 sqrt(DP) s        x (|q| + Nmax)
    double c_acc;       // (DP+8) 2^-23
    double hn_max;      // s^2 Nmax^2 / 2 + BIAS
    double n_max;       // Nmax
    double rel_slack;   // relative slack for the fp64 evaluation of the bound itself
    double thr2;        // rows with |x|^2 >= thr2 are BIG rows (fix_scale, match.hip); +infinity: none
    float  sf;          // (float)s
    float  pad;
    // int8 coarse pass (fix_scale chooses it on the device).  When coarse_i8 is set, s is 127 / max |x| or
    // less (not a power of two), bias an integer, and the fp16 constants above (c_in, c_sub, c_acc) are unused.
    double rho;         // max |s t - tq| over the rows converted at this scale, rounded up (k_i8_commit)
    double tau;         // max |tq| over the same rows, rounded up
    int32_t coarse_i8;  // 1: the resident images hold int8 copies and integer half-norms
    int32_t pad2;
};

// fused table filter (fmat.hip): per-pair keypoint coordinate lists
struct PairXY { const int32_t *q, *t; int32_t Kq, pad; };

// 2D-3D correspondence search (corr2d3d.hip): the directed match lists of rcn_match_lists_upload, resident in HBM
struct CorrLists {
    bool live = false, mirror = false;
    std::vector<int32_t> ids;         // slot -> image id, ascending: the images of the lists
    int32_t id_lo = 0, id_span = 0;   // id2slot covers ids id_lo .. id_lo + id_span - 1
    DevBuf ent;                       // (feature of a, feature of b) per entry, pair by pair
    DevBuf list_off;                  // int64, n_pairs + 1
    DevBuf dir;                       // n_slots x n_slots int32: (list << 1) | read backwards (mirror), -1 = no list
    DevBuf id2slot;                   // int32, -1 = not in the lists
    int32_t n_pairs = 0;              // lists uploaded
    int64_t n_ent = 0;                // their entries
    uint64_t coords_gen = 0;          // ctx->coords_gen at the upload: the entries were checked against those row counts
    void release() { ent.release(); list_off.release(); dir.release(); id2slot.release(); ids.clear(); live = false; id_lo = id_span = 0; }
};

// What one Levenberg-Marquardt iteration of rcn_int_ba_solve leaves on the device, copied out at two points of that iteration
// (tools/ba_step_check.hip, tests/test_ba_step_gpu.py).  Not part of the ABI: rcn_ctx::ba_probe is null wherever
// the library creates a context, and the solve then pays a few host pointer tests per iteration.  Capture A is taken behind the Schur / finish
// launches and in front of the factorisation (which destroys the reduced system), capture B behind the candidate's evaluation (and the line
// search) and in front of the parameter-tolerance test (an accepted step overwrites the observation rows); the solve ends there.
struct BaProbe {
    int iteration = 1;                 // in: the iteration (1-based, as rcn_ba_summary counts) to capture
    int got_a = 0, got_b = 0;          // out: the captures were taken; got_b = 2: the step was invalid (no candidate was judged)
    // ---- A
    int n = 0, npad = 0, csplit = 0, offdiag_kernel = 0, diag_smb = 0, fin = -2, rhs_row = 0, fused_finish = 0, chain = 0, pair_path = 0;
    //   offdiag_kernel: 0 none, 1 k_ba_schur_mfma<4>, 2 k_ba_schur_mfma_wg; diag_smb: the SMB of k_ba_schur_diag_mfma; pair_path: 0 lists reused,
    //   1 k_pair_small, 2 count / scan / fill
    double radius = 0.0;
    std::vector<double> J, crot, Uraw, gcraw, Vraw, gpraw, sc, sp, dgc, dgp, Vinv, gps, WY, S, rhs;
    std::vector<int> flag, cam_off, cam_dim, cols, pk_off;      // flag: all 24 words (flag, reduction tickets, the factorisation's counters)
    std::vector<unsigned> tickets;                              // the per-camera ticket words (2 nc)
    std::vector<unsigned long long> pk_list;
    // ---- B
    std::vector<double> x, tobs, stc, stp, dlc, dlp, poses2, intr2, pts2, crot2, scal;      // x: the reduced solution as k_ba_backsub reads it; scal: 16 words
    std::vector<int> flag_b;           // the same words as they stand behind the step
    std::vector<unsigned> tickets_b;
    std::vector<double> trials;        // per line-search trial of the iteration: alpha, candidate cost, directional derivative (NaN: not taken), |delta|_inf (-1: not yet)
    std::vector<double> log;           // per iteration up to the captured one: scal[0 .. 14) as read behind the step, then the number of backtracks
};

struct HamState;        // hamming.hip: the resident binary rows and the workspace of the Hamming matcher

struct rcn_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err = "";
    hipDeviceProp_t prop;

    // ---- matcher state
    int32_t D = 0, DP = 0;
    std::map<int32_t, ImgHost> images;
    std::vector<Slab> slabs;
    grid::GridShape grid_shape;                       // the last grid call's pair list as table slots and row counts, and its plan (grid_plan.h):
    grid::GridPlan grid;                              // kept alive, their vectors are uploaded asynchronously
    std::vector<int32_t> all_pairs_host;              // the canonical i < j grid when the caller passes pairs == NULL
    bool prepared = false;
    double scale = 0.0;      // s, power of two (0 = nothing prepared yet)
    double bias = 0.0;       // BIAS in accumulator units
    double max_norm = 0.0;   // max |x| over resident rows
    long hist_rows = 0;      // rows counted into the norm histogram since it was last cleared / rebuilt
    double thr2 = 0.0;       // BIG-row threshold in force (part of the scale: a change reconverts everything)
    DevBuf scale_dev;        // one ScaleDev: what the kernels read
    DevBuf desc_bad;         // desc.hip: keypoints outside their descriptor map since the last rcn_desc_sample_errors
    DevBuf kp_ws;            // keypoints.hip: candidate lists, heat map / status when the caller keeps neither, scale rows
    DevBuf sg_ws, sg_scores; // superglue.hip: u, v, argmax rows, partial column sums; the scores of rcn_sg_match_device
    int64_t sg_chunk_bytes = 0;   // bytes of score matrices per chunk of pairs (rcn_sg_set_chunk_bytes; <= 0: no limit)
    DevBuf gnn_ws, gnn_mdesc; // superglue_gnn.hip: the activations of one chunk of pairs; the matching descriptors of rcn_sg_net_match_device
    int32_t gnn_chunk_pairs = 0;  // pairs per chunk of the graph network (rcn_sg_net_set_chunk_pairs; 0: as many as fit the default cap)
    DevBuf sp_ws, sp_out;     // superpoint_net.hip: the activations of one chunk of images; the logits and descriptor maps of rcn_sp_net_detect_device
    int32_t sp_chunk_images = 0;  // images per chunk of SuperPoint's network (rcn_sp_net_set_chunk_images; 0: as many as fit the default cap)
    DevBuf sift_ws, sift_pyr; // sift.hip: candidate / keypoint lists and counters of one chunk of images; the pyramids of rcn_sift_detect_and_compute_device
    int32_t sift_chunk_images = 0;  // images per chunk of the SIFT detector (rcn_sift_set_chunk_images; 0: as many as fit the default cap)
    DevBuf orb_ws, orb_pyr, orb_tab; // orb.hip: score maps, blurred levels and lists of one chunk of images; the byte pyramids of rcn_orb_detect_and_compute_device; the resize tables
    int32_t orb_chunk_images = 0;   // images per chunk of the ORB detector (rcn_orb_set_chunk_images; 0: as many as fit the default cap)
    std::vector<int64_t> orb_tab_key;   // the level sizes the tables in orb_tab were built for
    DevBuf retr_ws, retr_out; // retrieval.hip: assignments, segment sums and counts, the pair mask; global descriptors, similarities and lists of rcn_retr_image_pairs
    DevBuf img_ws;            // imgprep.hip: the resize tables of one call, 8 bytes per output column and row
    std::vector<char> img_stage_host;   // staging of those tables (uploaded asynchronously; img_ev marks the copy)
    hipEvent_t img_ev = nullptr;
    bool img_stage_pending = false;
    ScaleDev scale_host;     // staging of the host-fixed scale (uploaded asynchronously)
    bool scale_on_device = false;   // the last scale was fixed by k_fix_scale: scale / bias / max_norm above are stale until resolved
    bool want_dev_scale = false;    // shard.hip: fix the next scale on the device (no host read of the statistics)
    bool i8_allowed = false;        // what the host knows of the int8 path's preconditions held at the last prepare (D padded to 256, every image at
                                    // most 4096 padded rows, no diagnostic switch against it); the data-dependent part is fix_scale's
    int32_t coarse_i8_host = 0;     // ScaleDev::coarse_i8 of the scale in force (stale while scale_on_device)
    std::vector<ImgDev> table_host; // image table as last uploaded (unchanged tables are not uploaded again)
    DevBuf img_table, pairs_dev, groups_dev, cand, owner, fb_list, sv_list, counters, out_tmp, cnt_tmp;
    hipEvent_t f32_ready = nullptr;   // shard.hip: set while an all-gather of fp32 rows may be in flight on a side stream
    // host materialisation (store.hip): offsets, two alternating staging buffers, copy stream
    DevBuf cmp_off, cmp_qt[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t cmp_ev[2] = {nullptr, nullptr}, cmp_filled = nullptr;
    bool cmp_busy[2] = {false, false};
    int cmp_next = 0, cmp_last = -1;
    int32_t last_kq_stride = 0, last_n_pairs = 0;   // shape of the candidate table of the last grid call
    uint32_t last_idx_mask = 0;
    rcn_match_stats last_stats;
    bool profile = false;
#define RCN_EV_CHUNKS 64
    hipEvent_t ev_c[64][RCN_EV_CHUNKS][4];   // per kept call and pipeline chunk: before coarse / after coarse / after the exact stages / after uniqueness
    hipEvent_t ev_tail[64][3];               // per kept call: before the deferred pass of the middle tier / behind it / behind the uniqueness of all pairs
    bool ev_tail_on[64] = {false};
    int ev_chunks[64] = {0};                 // chunks of that call that carry events (further chunks are not timed)
    int last_chunks = 1;                     // pipeline chunks of the last grid call
    int64_t chunk_rows = 1ll << 27;          // query-row slots of the candidate table per pipeline chunk (diagnostic build: RCN_CHUNK_ROWS)
    int64_t mid_rows = 1ll << 21;            // rows per chunk the middle tier takes (diagnostic build: RCN_MID_ROWS)
    DevBuf mid_ws;                           // middle tier of the exact stages (match.hip): binned rows, thresholds, candidate lists, bins
    int mid_bins_slots = -1;                 // image slots the zeroed bins of mid_ws were laid out for
    bool ev_made = false;
    int ev_n = 0;          // recorded calls since the last stats read (<= 64)
    // Ablations / alternative device paths exist only in the diagnostic build (-DRCN_DIAG,
    // tools/librcn_diag.so), where rcn_create reads them from the environment; in the shipping
    // library they are compile-time constants and the alternative code is dead.
#ifdef RCN_DIAG
    bool coarse_w4 = false;    // RCN_COARSE_W4=1: the one-wave-per-SIMD form of K1 (k_coarse_w4, coarse_w4.h) instead of k_coarse_top2
    bool coarse_i8_off = false;   // RCN_COARSE_I8=0: never the int8 coarse pass (tools/mfma_error_model.py measures the fp16 kernel)
    int coarse_i8_shape = -1;  // RCN_COARSE_I8_S16=0/1: force the int8 kernel's MFMA shape (0: 32x32x32, 1: 16x16x64); -1: the shipping choice (16x16x64)
    int coarse_shape = -1;     // RCN_COARSE_S16=0/1: force k_coarse_top2's MFMA shape (0: 32x32x16, 1: 16x16x32) at every D; -1: the shipping choice
    int ablate = 0;            // RCN_COARSE_ABL
    bool force_exact = false;  // RCN_FORCE_EXACT=1: skip the MFMA coarse pass
    bool mid_i8_off = false;   // RCN_MID_I8=0: on the int8 path too, every row of the middle tier takes the fp32 sweep (no k_mid_eval_i8)
    bool mid_i8_dot4 = false;  // RCN_MID_I8_MFMA=0: the int8 sweep of the middle tier on v_dot4 (k_mid_eval_i8_dot4), the differential reference of the MFMA form
    int mid_i8_launched = 0;   // which form of the int8 sweep the last pass of the middle tier launched (rcn_diag_mid_sweep): 0 none, 1 MFMA, 2 dot4
    bool rerank_pass = false;  // RCN_RERANK_PASS=1: certify's verdict is ignored, every re-ranked row goes to the middle tier
    bool filter_pass = false;  // RCN_FILTER_PASS=1: k_filter certifies nothing, every row with a coarse pair goes to the re-rank
    bool no_item_order = false;   // RCN_MATCH_NO_ORDER=1: work items in pair order instead of heaviest-first per XCD
    bool ba_atomics = false;   // RCN_BA_SCHUR_ATOMICS=1: atomic Schur accumulation instead of the gather form
    bool ba_trsv_fwd = false;  // RCN_BA_TRSV_FWD=1: separate forward substitution instead of the rhs row inside the factorisation
    bool ba_pair_small = true; // RCN_PAIR_SMALL=0: the pair lists of the smallest graphs by the six general launches too
#else
    static constexpr bool coarse_w4 = false;
    static constexpr bool coarse_i8_off = false;
    static constexpr int coarse_i8_shape = -1;
    static constexpr int coarse_shape = -1;
    static constexpr int ablate = 0;
    static constexpr bool mid_i8_off = false, rerank_pass = false, filter_pass = false;
    static constexpr bool force_exact = false, no_item_order = false, ba_atomics = false, ba_trsv_fwd = false, ba_pair_small = true;
#endif

    // ---- BA state (ba.hip)
    DevBuf ba_ws[40];
    DevBuf ba_loss_ws;         // rcn_ba_loss_report's scratch: block partials, scalars, the per-observation weights
    DevBuf lm_ws;              // landmark validity sweep (validity.hip)
    DevBuf tri_ws, tri_dws;    // triangulation (triangulate.hip): host-API staging + workspace, workspace of the device entry
    DevBuf fm_ws, fm_state;    // epipolar filter (fmat.hip): host-API staging, per-pair RANSAC state
    std::vector<PairXY> fm_pairs_host;   // staging of fm_pairs (uploaded asynchronously)
    DevBuf fm_csr, fm_pairs;   // fused table filter: CSR of the matched points, per-pair coordinate pointers
    DevBuf gd_pairs, gd_ws, gd_hws, gd_F;   // guided matcher (guided.hip): per-pair pointers, owner / reverse rows of one chunk, host-API staging, the grid's models
    std::vector<char> gd_pairs_host;        // staging of gd_pairs (uploaded asynchronously)
    std::map<int32_t, std::pair<DevBuf, int32_t>> coords;   // image id -> (K x 2 int32 pixel coordinates in HBM, K)
    CorrLists corr;                     // corr2d3d.hip: resident match lists
    DevBuf corr_ws, corr_hws, corr_slots, att_ws;   // ... workspace (obs_of, hit rows, tile counts), host-API staging, slot table, attach staging
    std::vector<char> corr_slots_host;  // staging of corr_slots (uploaded asynchronously; corr_ev marks the copy)
    hipEvent_t corr_ev = nullptr;
    bool corr_slots_pending = false;
    DevBuf pnp_hws, pnp_slots;          // view registration (pnp.hip): host-API staging, image id -> resident coordinates
    std::vector<char> pnp_slots_host;   // staging of pnp_slots (uploaded asynchronously; pnp_ev marks the copy)
    hipEvent_t pnp_ev = nullptr;
    bool pnp_slots_pending = false;
    DevBuf tv_hws, tv_dws, tv_fws;      // two-view initialisation (twoview.hip): host-API staging and workspace, workspace of the device entry, of its fill (corr2d3d.hip)
    DevBuf hg_hws, hg_dws;              // homography search and two-view geometry (homography.hip): host-API staging and workspace, workspace of the device entries
    std::vector<char> tv_stage_host;   // staging of the device entry's pair table (uploaded asynchronously; tv_ev marks the copy)
    hipEvent_t tv_ev = nullptr;
    bool tv_stage_pending = false;
    int64_t corr_budget = 1ll << 30;    // bytes of hit rows per batch (rcn_corr_set_workspace_bytes)
    // landmark-id table (corr2d3d.hip, rcn_landmark_ids_*): one int32 per keypoint of every image with resident coordinates
    DevBuf lid, lid_slot_off, lid_hws;  // the table, first entry of every list slot's row (int64), staging of rcn_landmark_ids_set
    std::map<int32_t, std::pair<int64_t, int32_t>> lid_rows;   // image id -> (first entry, K) at the last reset
    bool lid_live = false;
    uint64_t coords_gen = 0, lists_gen = 0;         // bumped by every change of the resident coordinates / match lists
    uint64_t lid_coords_gen = 0, lid_lists_gen = 0; // ... as they stood at the last reset: the table is valid while both are unchanged
    DevBuf nvt_ws;                      // new-view candidates (corr2d3d.hip): registered-image table, best (position, partner) per feature
    std::vector<char> nvt_stage_host;   // staging of the registered-image table (uploaded asynchronously; nvt_ev marks the copy)
    hipEvent_t nvt_ev = nullptr;
    bool nvt_stage_pending = false;
    std::vector<int> ba_graph_cam, ba_graph_pt;     // observation graph of the last plain rcn_ba_solve (host copy): an identical graph reuses the pair lists
    int ba_graph_nc = 0, ba_graph_np = 0;
    uint64_t ba_graph_serial = 0;
    uint64_t ba_pair_token = 0;         // whose pair lists the Schur-build workspace holds (0 = nobody's)
    std::vector<int> ba_pair_camdim;    // ... and the per-camera tangent dimensions they were built for (a camera without free parameters has no pairs)
    // track building (tracks.hip): workspace, the slot / selection table and its staging (uploaded asynchronously; trk_ev marks the copy),
    // the events around the six phases of the last build
    DevBuf trk_ws, trk_slots, trk_hws;
    std::vector<char> trk_stage_host;
    hipEvent_t trk_ev = nullptr;
    bool trk_stage_pending = false;
    hipEvent_t trk_tev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool trk_timed = false;
    // plane sweep (mvs.hip): the view table of one call and its staging (uploaded asynchronously; mvs_ev marks the copy), the row
    // counts and offsets of the fusion
    DevBuf mvs_tab, mvs_ws;
    std::vector<int32_t> mvs_stage_host;
    hipEvent_t mvs_ev = nullptr;
    bool mvs_stage_pending = false;
    HamState *ham = nullptr;            // hamming.hip: created by the first rcn_bits_* / Hamming call, released by rcn_int_ham_release
    CholState chol;                     // the dense factorisation of the reduced system (chol.h, chol.hip)
    BaProbe *ba_probe = nullptr;        // tools/ba_step_check.hip only: one LM iteration copied out (above)
    double *ba_host_scal = nullptr;   // pinned mirror of the LM step's scalars (16 doubles; [15]: sequence number), written by the step's last kernel
    unsigned long long ba_host_seq = 0;
    hipEvent_t ba_pair_ev;           // the pair lists of the Schur build are there
    hipEvent_t ba_tev[6];            // phase timing of rcn_ba_solve ([4], [5]: around k_ba_eval<true>)
    bool ba_ev_made = false;

    // Host waits inside rcn_int_prepare_all.  A sharded exchange (shard.hip) installs a BOUNDED wait for the duration of
    // its call -- the ctx stream then carries collectives, and a peer that died would otherwise keep this host thread in
    // hipStreamSynchronize for ever; NULL: plain hipStreamSynchronize.
    int (*wait_hook)(void *arg, hipStream_t st) = nullptr;
    void *wait_arg = nullptr;
    // match tables owned by the ctx (out_tmp / cnt_tmp): bumped by every entry point that writes them, so that a shard can tell
    // whether the tables its rcn_shard_match left there are still the ones it is about to filter / compact
    uint64_t own_table_gen = 0;

    void set_error(const std::string &s) { err = s; }
};
// RCN_HIP-compatible wait for everything queued on ctx->stream (the hook, or hipStreamSynchronize)
inline hipError_t rcn_int_stream_wait(rcn_ctx *ctx)
{
    if (ctx->wait_hook) return ctx->wait_hook(ctx->wait_arg, ctx->stream) == RCN_OK ? hipSuccess : hipErrorUnknown;
    return hipStreamSynchronize(ctx->stream);
}

// Device-resident part of a bundle-adjustment problem (rcn_ba_session, ba_session.hip -> rcn_int_ba_solve, ba.hip)
struct BaResident {
    double *pts;                  // n_points x 3, in and out
    const double *uv;             // n_obs x 2
    const int *ocam, *opt;        // n_obs each, landmark-major
    uint64_t pair_token;          // identifies (session, graph version): pair lists built under the same token are reused
};
int rcn_int_ba_solve(rcn_ctx *ctx, const rcn_ba_problem *pb, const rcn_ba_options *opt, rcn_ba_summary *sum, const BaResident *res,
                     const rcn_ba_loss *loss = nullptr, rcn_ba_loss_report *report = nullptr, double *weights_host = nullptr,
                     const uint8_t *cam_constant = nullptr, const int32_t *cam_group = nullptr);
// ba_local.hip, ctx->mu held: the sub-problem of a local adjustment cut out of a session's resident arrays (rcn_ba_session_solve_local), the
// scatter of its solved points, and the covisibility counts (rcn_ba_session_covisible).  The workspace belongs to the session; it only grows.
struct BaLocalWs {
    DevBuf flags, ints;                              // free / selected bytes; counts, camera flags, the three scans, the sizes
    DevBuf pts, uv, ocam, opt, pt_map, cam_map;      // the compacted sub-problem and its local -> session maps
    DevBuf counts;                                   // covisibility counts
    std::vector<int32_t> h_ocam, h_opt, h_cam_map;   // the sub-problem's structure on the host (what rcn_int_ba_solve validates and counts)
    int32_t n_cams = 0, n_points = 0, n_obs = 0;     // sizes of the last extraction
    size_t last_obs = 0;                             // ... its observations, as the next extraction's guess for the copy back
    void release();
};
int rcn_int_ba_local_extract(rcn_ctx *ctx, BaLocalWs &w, int32_t nc, int32_t np, int32_t no, const double *pts, const double *uv,
                             const int32_t *ocam, const int32_t *pt_off, const uint8_t *free_host);
int rcn_int_ba_local_scatter(rcn_ctx *ctx, BaLocalWs &w, double *pts);
int rcn_int_ba_local_covisible(rcn_ctx *ctx, BaLocalWs &w, int32_t nc, int32_t np, const int32_t *ocam, const int32_t *pt_off, int32_t cam, int32_t *counts_host);
// ba.hip, ctx->mu held: the argument check of a loss (NULL: none); the loss's report at a point whose arrays are all in HBM
int rcn_int_ba_loss_check(rcn_ctx *ctx, const rcn_ba_loss *loss, const char *who, int *kind, double *a, double *b);
int rcn_int_ba_loss_report(rcn_ctx *ctx, int no, const double *poses_dev, const double *intr_dev, const double *pts_dev, const double *uv_dev,
                           const int *ocam_dev, const int *opt_dev, const rcn_ba_loss *loss, rcn_ba_loss_report *report, double *weights_host);
int rcn_match_release(rcn_ctx *ctx);
void rcn_int_ham_release(rcn_ctx *ctx);      // hamming.hip: the binary residency and its workspace (rcn_destroy)
// triangulate.hip, with ctx->mu held: the host-side structure check, the workspace size and the launches (all pointers in
// HBM; compact / n_accepted may be NULL)
int rcn_int_triangulate_check(rcn_ctx *ctx, int32_t n_cams, int32_t n_tracks, int32_t n_obs, const int32_t *trk_off, const int32_t *obs_cam);
size_t rcn_int_triangulate_ws_bytes(int32_t n_cams, int32_t n_tracks);
int rcn_int_triangulate_launch(rcn_ctx *ctx, const rcn_triangulation_problem *dp, double max_err, double min_angle, void *ws,
                               double *xyz, uint8_t *status, double *compact, int32_t compact_first, int32_t *n_accepted);
// pnp.hip: rcn_pnp_ransac with ctx->mu held; points_dev != NULL: the points are already in HBM (rcn_ba_session_pnp)
int rcn_int_pnp_host(rcn_ctx *ctx, const char *who, int32_t n_views, const int64_t *off, const int32_t *landmark, const int32_t *xy,
                     int32_t n_points, const double *points_host, const double *points_dev, const double *intr6,
                     const rcn_pnp_options *opt, double *pose34_out, double *ransac_pose34_out, uint8_t *mask_out,
                     int32_t *count_out, int32_t *iterations_out);
// twoview.hip: rcn_twoview_init with ctx->mu held (rcn_ba_session_init_pair)
int rcn_int_twoview_host(rcn_ctx *ctx, const char *who, int32_t n_pairs, const int64_t *off, const int32_t *xy1, const int32_t *xy2,
                         const double *intr6_1, const double *intr6_2, const rcn_twoview_options *opt, double *E_out,
                         double *pose34_out, uint8_t *mask_out, uint8_t *cheir_mask_out, int32_t *count_out, int32_t *iterations_out);
// twoview.hip: k_tv_pair on entries in device memory with ctx->mu held (rcn_twoview_geometry, homography.hip); n_pairs == 0 only checks opt
int rcn_int_twoview_launch(rcn_ctx *ctx, const char *who, const rcn_twoview_options *opt, int32_t n_pairs, const int64_t *off_dev,
                           const int32_t *xy1_dev, const int32_t *xy2_dev, const double *intr6_1_dev, const double *intr6_2_dev,
                           double *norm_dev, double *E_dev, double *pose34_dev, uint8_t *mask_dev, uint8_t *cheir_mask_dev,
                           int32_t *count_dev, int32_t *iterations_dev);
// corr2d3d.hip, with ctx->mu held: the entries of directed pairs from the resident lists, ascending query order (rcn_twoview_init_device)
int rcn_int_pair_fill(rcn_ctx *ctx, const char *who, int32_t n_pairs, const int32_t *pairs, int64_t capacity, int64_t *off_dev,
                      int32_t *xy1_dev, int32_t *xy2_dev, int32_t *qt_dev);
// corr2d3d.hip, with ctx->mu held: step 1 of triangulateMatchedLandmarks on device arrays (rcn_ba_session_attach)
int rcn_int_attach_check(rcn_ctx *ctx, const char *who, int32_t n_points, int32_t n, const int32_t *lm, const int32_t *feat, int32_t *n_feat);
size_t rcn_int_attach_ws_bytes(int32_t n_feat);
int rcn_int_attach_launch(rcn_ctx *ctx, const double *P, const double *K, const double *pts, int32_t n_points, int32_t n,
                          const int32_t *lm, const int32_t *feat, const int32_t *xy, int32_t n_feat, double max_err,
                          uint8_t *status, void *ws);
// corr2d3d.hip, with ctx->mu held: step 3 of triangulateMatchedLandmarks on the resident lists and the landmark-id table
// (rcn_new_view_tracks_device's body: checks, one staged copy, launches), the commit of the accepted tracks' landmark indices into
// the table, and the rows an image has in the resident coordinates (-1: none)
int rcn_int_new_view_tracks(rcn_ctx *ctx, const char *who, int32_t v, int32_t n_reg, const int32_t *reg_img, int32_t cam_v,
                            const int32_t *reg_cam, int32_t capacity, int32_t *n_tracks_dev, int32_t *trk_off_dev,
                            int32_t *obs_cam_dev, int32_t *obs_xy_dev, int32_t *trk_src_dev);
int rcn_int_new_view_commit(rcn_ctx *ctx, int32_t v, int32_t capacity, const int32_t *n_tracks_dev, const int32_t *trk_src_dev,
                            const uint8_t *status_dev, int32_t first_landmark);
int32_t rcn_int_coords_rows(rcn_ctx *ctx, int32_t img);
// store.hip: rcn_match_compact_begin / _wait with ctx->mu already held
int rcn_int_compact_begin(rcn_ctx *ctx, const int32_t *table_dev, int64_t stride, const int32_t *counts_dev,
                          int32_t n_pairs, int64_t *offsets_host, int32_t *qt_host, int64_t capacity, int64_t *total_out);
int rcn_int_compact_wait(rcn_ctx *ctx);
// store.hip: the ordered compaction kernel alone (rcn_shard_gather_lists: the lists stay in HBM)
void rcn_int_launch_cmp_fill(hipStream_t st, const int32_t *table_dev, int64_t stride, const int32_t *counts_dev, const long long *off, int32_t n_pairs, int2 *qt);
// fmat.hip: rcn_match_table_filter_device with ctx->mu already held; out_F_dev (may be NULL): the model of every pair, 9 doubles, zeros
// where there is none (rcn_match_table_filter_model_device)
int rcn_int_table_filter(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, int32_t *table_dev,
                         int64_t stride, int32_t *counts_dev, int32_t *out_status_dev, double *out_F_dev = nullptr);
// superglue.hip: rcn_sg_match_device with ctx->mu already held (rcn_sg_net_match_device, superglue_gnn.hip); check_only: the
// argument checks alone, nothing launched and the descriptor pointers not looked at
int rcn_int_sg_match(rcn_ctx *ctx, const char *who, const float *d0_dev, int64_t stride_pair0, int64_t stride_row0, int64_t stride_d0,
                     const float *d1_dev, int64_t stride_pair1, int64_t stride_row1, int64_t stride_d1,
                     const int32_t *m_dev, const int32_t *n_dev, int32_t B, int32_t M, int32_t N, int32_t D, const rcn_sg_options *opt,
                     int32_t *matches0_dev, int32_t *matches1_dev, float *mscores0_dev, float *mscores1_dev,
                     int32_t *table_dev, int64_t table_stride, int32_t *counts_dev, float *logP_out_dev, int32_t *status_dev, bool check_only);
// keypoints.hip / desc.hip: rcn_kp_detect_device and rcn_desc_sample_batch_device with ctx->mu already held
// (rcn_sp_net_detect_device, superpoint_net.hip); check_only: the argument checks alone, nothing launched
int rcn_int_kp_detect(rcn_ctx *ctx, const float *logits_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y, int64_t stride_x,
                      int32_t n, int32_t H, int32_t W, int32_t heat_mode, double conf_thresh, int32_t nms_radius, int32_t border,
                      int32_t K, int32_t *kp_xy_dev, float *conf_dev, int32_t *counts_dev, float *heat_out_dev, int32_t *rounds_dev, bool check_only);
int rcn_int_desc_sample_batch(rcn_ctx *ctx, const float *desc_maps_dev, int64_t stride_img, int64_t stride_c, int64_t stride_y,
                              int64_t stride_x, int32_t Hc, int32_t Wc, const int32_t *kp_xy_dev, const int32_t *counts_dev,
                              int32_t n, int32_t K, int32_t D, float *out_rows_dev, bool check_only);
// match.hip internals shared with shard.hip (all expect ctx->mu held)
int rcn_int_slab_attach(rcn_ctx *ctx, int32_t first_id, int32_t n_images, int32_t n_slots, const float *src,
                        int32_t K, int32_t D, int32_t conv_first, int32_t conv_n, int *slab_out,
                        const int32_t *Ks_host, const int32_t *Ks_dev);
int rcn_int_slab_rowstats(rcn_ctx *ctx, int slab, int32_t first, int32_t n);
int rcn_int_prepare_all(rcn_ctx *ctx);
int rcn_int_i8_commit(rcn_ctx *ctx);         // int8 path: the residual / quantised-norm maxima of ctx->counters into the scale record (behind the conversions,
                                             // and behind their reduction over the ranks of a sharded grid)
int rcn_int_resolve_scale(rcn_ctx *ctx);     // host copies of scale / bias / max_norm are current afterwards (may synchronise)
int rcn_int_match_grid(rcn_ctx *ctx, const int32_t *pairs_host, int32_t n_pairs, float ratio,
                       int32_t *out_dev, int64_t out_stride, int32_t *counts_dev);
void rcn_int_tracks_release(rcn_ctx *ctx);   // tracks.hip: the track builder's buffers and events (rcn_destroy)
int rcn_int_mvs_views(rcn_ctx *ctx, int32_t nc, int32_t np, const int32_t *ocam, const int32_t *pt_off, const double *pts, const double *poses34_host, int32_t S,
                      int32_t *sources_out, double *range_out, int32_t *cov_out);      // mvs.hip: rcn_ba_session_mvs_views behind the session's lock
void rcn_int_mvs_release(rcn_ctx *ctx);      // mvs.hip: the plane sweep's buffers and event (rcn_destroy)
void rcn_int_guided_release(rcn_ctx *ctx);   // guided.hip: the guided matcher's buffers (rcn_destroy)
