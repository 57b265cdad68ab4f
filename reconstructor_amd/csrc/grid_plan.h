// grid_plan.h -- everything rcn_int_match_grid (match.hip) decides before its first launch, as DATA: the groups of pairs a workgroup of
// the coarse pass sweeps, the pipeline chunks, the order of a chunk's work items, the layout of the middle tier's workspace and the
// predicates that choose the kernels.  Pure host code (no HIP), integer arithmetic on (slot, K, Kp) per pair: match.hip fills a GridShape
// in one pass over the pair list and launches what the GridPlan says, tests/cpp/grid_plan_test.cpp checks the plan's invariants on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// The constants of match.hip's kernels that the plan reads too (one definition for both sides).
#define RCN_QT 512          // query rows per workgroup (8 waves x 64)
#define RCN_GROUP 4         // consecutive pairs (same query image) swept by one workgroup
#define RCN_I8_IDX_BITS 12  // train-row bits of an int8 key
#define RCN_MIDCAP 32       // candidates kept per row of the middle tier
#define RCN_UNIQ_LDS 8192   // train rows whose owner table (K3, k_unique_pair) fits LDS
#define MI8_TR 512          // k_mid_eval_i8 (mid_i8.h): train rows per tile, 128 per wave
#define MI8_TILES ((1 << RCN_I8_IDX_BITS) / MI8_TR)   // tiles of the largest image the int8 path admits

namespace grid {

struct Group { int first, count; };      // pairs first .. first + count - 1 (the layout of int2: the kernels read it as one)
struct Chunk {
    int g0, p0, np;                      // first group, first pair, pairs
    int arr_off, arr_n;                  // the chunk's range of GridPlan::arranged (arr_n: its groups + padding)
    int items_per_xcd;                   // ceil(arr_n * tiles / 8): the coarse launch has 8 times as many workgroups
};
// Byte offsets into ctx->mid_ws: binned rows, thresholds, candidate lists, the overflow list, the call's list of deferred rows
// (k_mid_defer: as many rows as one pass of the tier takes), the integer thresholds of the int8 sweep, four words per image slot (+ 1).
struct MidLayout { size_t bins, sorted, thr, cc, cl, fb2, def, defthr, deftacc, tacc, fbtacc, end, rows_cap; };

struct PairK { int32_t kq, kt, ktp; };   // rows of the query image, rows and padded rows of the train image
struct GridShape {
    std::vector<int32_t> slots;          // per pair (query slot, train slot): the vector that is uploaded as the pair list
    std::vector<PairK> k;                // per pair
    int D = 0, DP = 0, n_slots = 0, n_cu = 0;
    int64_t chunk_rows = 0, mid_rows = 0;
    bool i8_allowed = false, force_exact = false, no_item_order = false, mid_i8_off = false;
};

struct GridPlan {
    int tiles = 1, kq_stride = RCN_QT, idx_bits = 1, owner_stride = 1, kq_max = 0, kt_max = 0, ktp_max = 0;
    uint32_t idx_mask = 1;
    int64_t rows = 0, pair_distances = 0, cap_slots = 0, cap_rows = 0;
    bool mfma = false, vec4 = false, mid = false, mid_i8 = false, uniq_lds = false, defer = false;
    std::vector<Group> groups, arranged;     // in pair order; chunk by chunk as the coarse launches walk them (uploaded)
    std::vector<Chunk> chunks;
    int mid_i8_grid_y = 1;                   // y extent of the k_mid_eval_i8 grid (x: n_slots * MI8_TILES)
    MidLayout mid_ws = {};
    std::vector<std::pair<int64_t, int>> order;   // scratch of the arrangement
};

inline void plan_grid(const GridShape &s, GridPlan &pl)
{
    const int n_pairs = (int)s.k.size();
    pl.kq_max = pl.kt_max = pl.ktp_max = 0;
    pl.rows = pl.pair_distances = 0;
    for (int p = 0; p < n_pairs; ++p) {
        pl.kq_max = std::max(pl.kq_max, s.k[p].kq);
        pl.kt_max = std::max(pl.kt_max, s.k[p].kt);
        pl.ktp_max = std::max(pl.ktp_max, s.k[p].ktp);
        pl.rows += s.k[p].kq;
        pl.pair_distances += (int64_t)s.k[p].kq * s.k[p].kt;
    }
    pl.tiles = std::max(1, (pl.kq_max + RCN_QT - 1) / RCN_QT);
    pl.kq_stride = pl.tiles * RCN_QT;
    pl.idx_bits = 1;
    while ((1 << pl.idx_bits) < pl.ktp_max) ++pl.idx_bits;
    // The packed candidate keeps the train row in its low idx_bits and the accumulator's leading 32 - idx_bits bits
    // above them: up to 16 index bits (65536 rows per image) leave sign + exponent + 7 mantissa bits, and the
    // certificates price that quantum (k_filter: upper bounds are truncated value + one quantum), so a coarser
    // value only sends more rows to the exact re-rank -- it never changes a result.
    pl.mfma = s.DP != 0 && pl.idx_bits <= 16 && !s.force_exact && pl.kq_max > 0 && pl.kt_max >= 2;
    pl.idx_mask = (1u << pl.idx_bits) - 1u;
    pl.owner_stride = std::max(1, pl.kt_max);
    pl.vec4 = (s.D % 4) == 0;
    pl.mid = pl.vec4 && pl.kt_max >= 2;               // the middle tier reads rows as float4
    pl.uniq_lds = pl.kt_max <= RCN_UNIQ_LDS;          // owner table of a pair fits LDS: one fused launch
    // the int8 form of the tier's sweep (k_mid_eval_i8): launched beside k_mid_eval wherever the int8 K1 is; like it, it returns at once unless
    // fix_scale chose the int8 path.  Its grid: (image slot x tile) x slabs of the bin's rows, the slabs so that a small grid still fills the chip
    pl.mid_i8 = pl.mid && pl.mfma && s.i8_allowed && !s.mid_i8_off;
    pl.mid_i8_grid_y = (int)std::max<int64_t>(1, std::min<int64_t>(16, (4 * (int64_t)s.n_cu) / std::max<int64_t>(1, (int64_t)s.n_slots * MI8_TILES)));

    // groups: runs of consecutive pairs that share the query image, cut at RCN_GROUP
    pl.groups.clear();
    for (int p = 0; p < n_pairs;) {
        int cnt = 1;
        while (p + cnt < n_pairs && cnt < RCN_GROUP && s.slots[2 * (size_t)(p + cnt)] == s.slots[2 * (size_t)p]) ++cnt;
        pl.groups.push_back({p, cnt});
        p += cnt;
    }
    const int n_groups = (int)pl.groups.size();
    // Pipeline chunks (round 4): the candidate table and the two row lists are sized for at most RCN_CHUNK_ROWS query-row slots
    // and REUSED by consecutive ranges of the pair list, in stream order -- coarse(c), filter(c), re-rank(c), uniqueness(c),
    // coarse(c+1), ...  Round 3 sized them for the whole grid: 16.4 GB each at cfg 3, three of them, and a 2000-image grid
    // would not have fitted the device at all.  A chunk never exceeds the budget (the lists can therefore not overflow) and
    // ends at a group boundary; a small grid is one chunk and runs exactly as before.  (The two-stream overlap of chunks that
    // the diagnostic build once had measured slower in rounds 1 and 2 and is gone.)
    pl.chunks.clear();
    pl.cap_slots = pl.cap_rows = 0;
    {
        int64_t slots_c = 0, rows_c = 0;
        pl.chunks.push_back({0, 0, 0, 0, 0, 0});
        for (int g = 0; g < n_groups; ++g) {
            int64_t gs = (int64_t)pl.groups[g].count * pl.kq_stride, gr = 0;
            for (int r = 0; r < pl.groups[g].count; ++r) gr += s.k[pl.groups[g].first + r].kq;
            if (slots_c > 0 && slots_c + gs > s.chunk_rows) {
                pl.chunks.push_back({g, pl.groups[g].first, 0, 0, 0, 0});
                pl.cap_slots = std::max(pl.cap_slots, slots_c); pl.cap_rows = std::max(pl.cap_rows, rows_c);
                slots_c = 0; rows_c = 0;
            }
            slots_c += gs; rows_c += gr;
        }
        pl.cap_slots = std::max(pl.cap_slots, slots_c); pl.cap_rows = std::max(pl.cap_rows, rows_c);
    }
    const int n_chunks = (int)pl.chunks.size();
    pl.defer = pl.mid && n_chunks > 1 && pl.uniq_lds && pl.kq_max > 0;

    // Order of the work items of a coarse launch: every XCD walks its own contiguous range of the chunk's
    // group list, heaviest groups first, so that the last items to start are the short ones (the tail
    // of a launch is one item long: 5 % of a cfg-2 grid for a four-pair group, 1 % for a one-pair group).
    // Groups are dealt to the XCD ranges round-robin in descending weight; unused slots hold empty groups.
    // (Measured and dropped in round 2: a train-block-major order -- every XCD runs the query tiles of ~8 query
    // images against the SAME four train images at a time, so that all but one of them hit in its L2 -- is 0.5-1.5 %
    // slower: the kernel is power-limited, not fabric-limited, and the order above has the shorter tail.)
    pl.arranged.clear();
    for (int c = 0; c < n_chunks; ++c) {
        Chunk &ck = pl.chunks[c];
        const int g0 = ck.g0, g1 = c + 1 < n_chunks ? pl.chunks[c + 1].g0 : n_groups, ng = g1 - g0;
        ck.np = (g1 < n_groups ? pl.groups[g1].first : n_pairs) - ck.p0;
        ck.arr_off = (int)pl.arranged.size();
        if (pl.mfma && ng >= 64 && !s.no_item_order) {
            pl.order.resize((size_t)ng);
            for (int g = 0; g < ng; ++g) {
                int64_t wgt = 0;
                for (int r = 0; r < pl.groups[g0 + g].count; ++r) wgt += s.k[pl.groups[g0 + g].first + r].kt;
                pl.order[g] = std::make_pair(-wgt, g0 + g);
            }
            std::stable_sort(pl.order.begin(), pl.order.end());
            const int gpx = (ng + 7) / 8;
            const size_t base = pl.arranged.size();
            pl.arranged.resize(base + (size_t)8 * gpx, Group{0, 0});
            for (int k = 0; k < ng; ++k) pl.arranged[base + (size_t)(k % 8) * gpx + k / 8] = pl.groups[pl.order[k].second];
            ck.arr_n = 8 * gpx;
        } else {
            pl.arranged.insert(pl.arranged.end(), pl.groups.begin() + g0, pl.groups.begin() + g1);
            ck.arr_n = ng;
        }
        ck.items_per_xcd = (int)(((int64_t)ck.arr_n * pl.tiles + 7) / 8);
    }

    // The workspace, every region on a 256-byte boundary.  The deferred regions are empty when there is one chunk.
    // (the bins come FIRST: their place must not move with the row count of the grid, they carry state -- zeros -- from call to call)
    MidLayout &m = pl.mid_ws;
    m.rows_cap = (size_t)std::min<int64_t>(std::max<int64_t>(1, pl.cap_rows), s.mid_rows);
    const size_t rc = m.rows_cap, dc = n_chunks > 1 ? rc : 0;
    size_t end = 0;
    auto take = [&end](size_t bytes) { const size_t at = end; end += (bytes + 255) / 256 * 256; return at; };
    m.bins = take(4 * 4 * ((size_t)s.n_slots + 1));
    m.sorted = take(8 * rc); m.thr = take(4 * rc); m.cc = take(4 * rc); m.cl = take(4 * rc * RCN_MIDCAP); m.fb2 = take(8 * rc);
    m.def = take(8 * dc); m.defthr = take(4 * dc); m.deftacc = take(4 * dc);
    m.tacc = take(4 * rc); m.fbtacc = take(4 * (size_t)std::max<int64_t>(1, pl.cap_rows));
    m.end = end;
}

}  // namespace grid
