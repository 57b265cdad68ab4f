// The plan of the matcher's grid call (reconstructor_amd/csrc/grid_plan.h) on the CPU: plain g++, no HIP, no librcn.so.
// Every expectation is derived HERE from the case's inputs (or stated outright); nothing is read back from the plan to judge the plan.
// One GridPlan object serves all cases, as one lives in the library's context: a case must not see what the one before left.
#include "../../reconstructor_amd/csrc/grid_plan.h"

#include <cstdio>
#include <string>

using namespace grid;

static int failures = 0;
static std::string cur;
#define CHECK(c) do { if (!(c)) { ++failures; std::printf("FAIL %s: line %d: %s\n", cur.c_str(), __LINE__, #c); } } while (0)

struct P { int q, kq, kt, ktp; };      // a pair: query slot, query rows, train rows, padded train rows

static GridShape shape(const std::vector<P> &pairs, int64_t chunk_rows = 1ll << 27, int D = 256, int n_slots = 8)
{
    GridShape s;
    for (const P &p : pairs) {
        s.slots.push_back(p.q); s.slots.push_back(1000 + p.q);      // (no decision reads the train slot)
        s.k.push_back({p.kq, p.kt, p.ktp});
    }
    s.D = D; s.DP = D <= 256 ? 256 : 0; s.n_slots = n_slots; s.n_cu = 256;
    s.chunk_rows = chunk_rows; s.mid_rows = 1ll << 21;
    s.i8_allowed = true;
    return s;
}

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

static GridPlan pl;

// plans the case and checks what must hold for every input
static void run(const std::string &name, const GridShape &s)
{
    cur = name;
    plan_grid(s, pl);
    const int n = (int)s.k.size();
    // ---- shape figures and predicates, from the inputs
    int kq_max = 0, kt_max = 0, ktp_max = 0;
    int64_t rows = 0, pd = 0;
    for (const PairK &k : s.k) {
        kq_max = std::max(kq_max, k.kq); kt_max = std::max(kt_max, k.kt); ktp_max = std::max(ktp_max, k.ktp);
        rows += k.kq; pd += (int64_t)k.kq * k.kt;
    }
    const int tiles = kq_max <= RCN_QT ? 1 : (kq_max + RCN_QT - 1) / RCN_QT, kq_stride = tiles * RCN_QT;
    int bits = 1;
    while ((1ll << bits) < ktp_max) ++bits;
    const bool mfma = s.DP != 0 && bits <= 16 && !s.force_exact && kq_max > 0 && kt_max >= 2;
    const bool vec4 = s.D % 4 == 0, mid = vec4 && kt_max >= 2, uniq_lds = kt_max <= RCN_UNIQ_LDS;
    CHECK(pl.kq_max == kq_max && pl.kt_max == kt_max && pl.ktp_max == ktp_max && pl.rows == rows && pl.pair_distances == pd);
    CHECK(pl.tiles == tiles && pl.kq_stride == kq_stride && pl.idx_bits == bits && pl.idx_mask == (uint32_t)((1ull << bits) - 1));
    CHECK(pl.owner_stride == std::max(1, kt_max));
    CHECK(pl.mfma == mfma && pl.vec4 == vec4 && pl.mid == mid && pl.uniq_lds == uniq_lds);
    CHECK(pl.mid_i8 == (mid && mfma && s.i8_allowed && !s.mid_i8_off));
    // ---- groups: every pair in exactly one, consecutive, one query slot, cut at RCN_GROUP and nowhere else
    std::vector<Group> want;
    for (int p = 0; p < n; ++p) {
        if (!want.empty() && want.back().count < RCN_GROUP && s.slots[2 * p] == s.slots[2 * want.back().first]) ++want.back().count;
        else want.push_back({p, 1});
    }
    const int ng_all = (int)want.size();
    CHECK((int)pl.groups.size() == ng_all);
    for (int g = 0; g < ng_all && g < (int)pl.groups.size(); ++g) CHECK(pl.groups[g].first == want[g].first && pl.groups[g].count == want[g].count);
    if ((int)pl.groups.size() != ng_all) return;
    // ---- chunks partition the groups in order; greedy under chunk_rows; at least one group each
    const int nc = (int)pl.chunks.size();
    CHECK(nc >= 1 && pl.chunks[0].g0 == 0);
    int64_t cap_slots = 0, cap_rows = 0;
    size_t arr_at = 0;
    for (int c = 0; c < nc; ++c) {
        const Chunk &ck = pl.chunks[c];
        const int g1 = c + 1 < nc ? pl.chunks[c + 1].g0 : ng_all, ng = g1 - ck.g0;
        CHECK(ng >= 1 && g1 <= ng_all);
        if (ng < 1 || g1 > ng_all) return;
        int np = 0;
        int64_t qrows = 0;
        for (int g = ck.g0; g < g1; ++g)
            for (int r = 0; r < want[g].count; ++r) { ++np; qrows += s.k[want[g].first + r].kq; }
        CHECK(ck.p0 == want[ck.g0].first && ck.np == np);
        const int64_t slots = (int64_t)np * kq_stride;
        CHECK(slots <= s.chunk_rows || ng == 1);
        if (g1 < ng_all) CHECK(slots + (int64_t)want[g1].count * kq_stride > s.chunk_rows);      // it ends only before the group that would not fit
        cap_slots = std::max(cap_slots, slots); cap_rows = std::max(cap_rows, qrows);
        // ---- the chunk's arranged range: each of its groups once, else padding; heaviest first per XCD range when arranged
        CHECK((size_t)ck.arr_off == arr_at);
        const bool arranged = mfma && ng >= 64 && !s.no_item_order;
        const int gpx = (ng + 7) / 8, len = arranged ? 8 * gpx : ng;
        CHECK(ck.arr_n == len && arr_at + len <= pl.arranged.size());
        CHECK(ck.items_per_xcd == (int)(((int64_t)len * tiles + 7) / 8));
        if (ck.arr_n != len || arr_at + len > pl.arranged.size()) return;
        const Group *a = pl.arranged.data() + arr_at;
        std::vector<int> seen((size_t)ng, 0);
        for (int i = 0; i < len; ++i) {
            if (a[i].count == 0) { CHECK(a[i].first == 0); continue; }
            int g = -1;
            for (int j = ck.g0; j < g1; ++j) if (want[j].first == a[i].first && want[j].count == a[i].count) g = j;
            CHECK(g >= 0);
            if (g >= 0) ++seen[g - ck.g0];
        }
        for (int g = 0; g < ng; ++g) CHECK(seen[g] == 1);
        auto weight = [&](const Group &g) { int64_t w = 0; for (int r = 0; r < g.count; ++r) w += s.k[g.first + r].kt; return w; };
        if (arranged) {
            for (int k = 0; k < len; ++k) {
                const Group &g = a[(k % 8) * gpx + k / 8];
                if (k >= ng) { CHECK(g.count == 0); continue; }
                CHECK(g.count > 0);
                if (k == 0) continue;
                const Group &prev = a[((k - 1) % 8) * gpx + (k - 1) / 8];
                CHECK(weight(prev) > weight(g) || (weight(prev) == weight(g) && prev.first < g.first));
            }
        } else {
            for (int g = 0; g < ng; ++g) CHECK(a[g].first == want[ck.g0 + g].first && a[g].count == want[ck.g0 + g].count);
        }
        arr_at += len;
    }
    CHECK(arr_at == pl.arranged.size());
    CHECK(pl.cap_slots == cap_slots && pl.cap_rows == cap_rows);
    CHECK(pl.defer == (mid && nc > 1 && uniq_lds && kq_max > 0));
    CHECK(pl.mid_i8_grid_y >= 1 && pl.mid_i8_grid_y <= 16);
    // ---- the middle tier's workspace: regions in this order, each on a 256-byte multiple and exactly as long as its content rounded up
    const MidLayout &m = pl.mid_ws;
    const size_t rc = (size_t)std::min<int64_t>(std::max<int64_t>(1, cap_rows), s.mid_rows), dc = nc > 1 ? rc : 0;
    CHECK(m.rows_cap == rc);
    const size_t at[12] = {m.bins, m.sorted, m.thr, m.cc, m.cl, m.fb2, m.def, m.defthr, m.deftacc, m.tacc, m.fbtacc, m.end};
    const size_t need[11] = {16 * ((size_t)s.n_slots + 1), 8 * rc, 4 * rc, 4 * rc, 4 * rc * RCN_MIDCAP, 8 * rc, 8 * dc, 4 * dc, 4 * dc, 4 * rc,
                             4 * (size_t)std::max<int64_t>(1, cap_rows)};
    CHECK(m.bins == 0);
    for (int i = 0; i < 11; ++i) CHECK(at[i] % 256 == 0 && at[i + 1] == at[i] + up256(need[i]));
    if (nc == 1) CHECK(m.defthr == m.def && m.deftacc == m.def && m.tacc == m.def);
}

// n one-pair groups (alternating query slots), the train rows of pair p given by kt(p)
template <class F> static std::vector<P> singles(int n, F kt)
{
    std::vector<P> v;
    for (int p = 0; p < n; ++p) v.push_back({p % 2, 512, kt(p), 1024});
    return v;
}

int main()
{
    run("one pair", shape({{0, 300, 200, 512}}));
    CHECK(pl.groups.size() == 1 && pl.chunks.size() == 1 && pl.mfma && pl.mid && !pl.defer && pl.kq_stride == 512);

    run("every query K = 0", shape({{0, 0, 200, 512}, {0, 0, 100, 512}, {1, 0, 300, 512}}));
    CHECK(pl.kq_stride == RCN_QT && !pl.mfma && pl.cap_rows == 0 && pl.mid_ws.rows_cap == 1);

    run("train K = 1", shape({{0, 300, 1, 512}, {1, 300, 1, 512}}));
    CHECK(!pl.mfma && !pl.mid);

    run("D = 130", shape({{0, 300, 200, 512}}, 1ll << 27, 130));
    CHECK(!pl.vec4 && !pl.mid && pl.mfma);

    {
        std::vector<P> same, alt;
        for (int p = 0; p < 9; ++p) { same.push_back({3, 600, 200, 512}); alt.push_back({p % 2, 600, 200, 512}); }
        run("nine pairs on one query", shape(same));
        CHECK(pl.groups.size() == 3 && pl.groups[0].count == 4 && pl.groups[1].count == 4 && pl.groups[2].count == 1 && pl.groups[2].first == 8);
        CHECK(pl.tiles == 2 && pl.kq_stride == 1024);
        run("nine pairs, alternating queries", shape(alt));
        CHECK(pl.groups.size() == 9);
    }

    run("ktp_max = 65536", shape({{0, 300, 200, 65536}}));
    CHECK(pl.idx_bits == 16 && pl.idx_mask == 0xFFFFu && pl.mfma);
    run("ktp_max = 65537", shape({{0, 300, 200, 65537}}));
    CHECK(pl.idx_bits == 17 && !pl.mfma && !pl.mid_i8);

    // two chunks (one group each), so that the owner table decides about the deferred pass too
    run("kt_max = RCN_UNIQ_LDS", shape({{0, 512, RCN_UNIQ_LDS, 8192}, {1, 512, 100, 512}}, 512));
    CHECK(pl.uniq_lds && pl.chunks.size() == 2 && pl.defer && pl.mid_ws.defthr > pl.mid_ws.def);
    run("kt_max = RCN_UNIQ_LDS + 1", shape({{0, 512, RCN_UNIQ_LDS + 1, 8704}, {1, 512, 100, 512}}, 512));
    CHECK(!pl.uniq_lds && pl.chunks.size() == 2 && !pl.defer && pl.owner_stride == RCN_UNIQ_LDS + 1);

    {
        // six groups of four pairs, 512 slots per pair: a group takes 2048 slots
        std::vector<P> v;
        for (int p = 0; p < 24; ++p) v.push_back({p / 4, 500, 200, 512});
        run("chunk_rows = two groups exactly", shape(v, 4096));
        CHECK(pl.chunks.size() == 3 && pl.chunks[1].g0 == 2 && pl.chunks[2].g0 == 4 && pl.chunks[1].p0 == 8 && pl.chunks[1].np == 8);
        CHECK(pl.cap_slots == 4096 && pl.cap_rows == 4000);
        run("chunk_rows = two groups less one", shape(v, 4095));
        CHECK(pl.chunks.size() == 6 && pl.cap_slots == 2048 && pl.cap_rows == 2000);
        run("chunk_rows below one group", shape(v, 100));
        CHECK(pl.chunks.size() == 6 && pl.chunks[5].g0 == 5 && pl.chunks[5].np == 4 && pl.cap_slots == 2048);
        run("one chunk behind several", shape(v));       // the plan object forgets the chunks and the deferred regions of the case before
        CHECK(pl.chunks.size() == 1 && !pl.defer && pl.mid_ws.tacc == pl.mid_ws.def && pl.arranged.size() == 6);
    }

    for (int n : {63, 64, 65}) {
        const int len = n < 64 ? n : 8 * ((n + 7) / 8);
        run(std::to_string(n) + " groups, distinct weights", shape(singles(n, [](int p) { return 100 + p; })));
        CHECK((int)pl.groups.size() == n && pl.chunks.size() == 1 && pl.chunks[0].arr_n == len && (int)pl.arranged.size() == len);
        if (n < 64) CHECK(pl.arranged[0].first == 0 && pl.arranged[n - 1].first == n - 1);                    // pair order
        else for (int k = 0; k < n; ++k) CHECK(pl.arranged[(k % 8) * (len / 8) + k / 8].first == n - 1 - k);  // the k-th heaviest is pair n - 1 - k
        run(std::to_string(n) + " groups, tied weights", shape(singles(n, [](int p) { return 100 + p % 3; })));
        CHECK(pl.chunks[0].arr_n == len);
        if (n >= 64) CHECK(pl.arranged[0].first == 2 && pl.arranged[len / 8].first == 5);       // weight 102: pairs 2, 5, 8, ... in list order
        int pad = 0;
        for (const Group &g : pl.arranged) pad += g.count == 0;
        CHECK(pad == len - n);                                                                  // 65 groups: 7 padding groups
    }
    {
        GridShape s = shape(singles(64, [](int p) { return 100 + p; }));
        s.no_item_order = true;
        run("64 groups, no_item_order", s);
        CHECK(pl.chunks[0].arr_n == 64 && pl.arranged[0].first == 0 && pl.arranged[63].first == 63);
        s.no_item_order = false; s.force_exact = true;
        run("64 groups, no coarse pass", s);
        CHECK(!pl.mfma && pl.arranged[63].first == 63);
        s.force_exact = false; s.mid_i8_off = true;
        run("64 groups, mid_i8_off", s);
        CHECK(pl.mfma && !pl.mid_i8);
    }
    {
        // the y extent of the k_mid_eval_i8 grid: 4 workgroups per CU over n_slots * MI8_TILES columns, within [1, 16]
        GridShape s = shape({{0, 300, 200, 512}});
        s.n_slots = 2; run("two image slots", s); CHECK(pl.mid_i8_grid_y == 16);
        s.n_slots = 32; run("32 image slots", s); CHECK(pl.mid_i8_grid_y == 4);
        const size_t bins32 = pl.mid_ws.sorted;
        s.n_slots = 2000; run("2000 image slots", s); CHECK(pl.mid_i8_grid_y == 1);
        s = shape(singles(40, [](int) { return 300; })); s.n_slots = 32;
        run("32 image slots, more rows", s); CHECK(pl.mid_ws.sorted == bins32);      // the bins' size follows the slot count only
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("grid plan: all cases pass\n");
    return 0;
}
