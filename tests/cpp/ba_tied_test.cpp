// The host side of shared intrinsics (csrc/ba_tied.h) alone: random group assignments, every invariant of the plan recomputed from the
// inputs.  Built by tests/test_ba_tied.py as an executable of its own with the address and undefined-behaviour sanitizers.
#include "../../reconstructor_amd/csrc/ba_tied.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

static int failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            ++failures;                                                          \
            std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond);          \
            std::printf(__VA_ARGS__);                                            \
            std::printf("\n");                                                   \
        }                                                                        \
    } while (0)

struct Case {
    int nc, mode;
    bool fix0, fix1;
    std::vector<uint8_t> constant;
    std::vector<int32_t> group;
    std::vector<double> intr;
};

// the expected normalisation and sizes, from the inputs alone (no code of the header)
static void check_plan(const Case &c, const char *name)
{
    ba_tied::Plan p;
    const int rc = ba_tied::build(c.nc, c.mode, c.fix0, c.fix1, c.constant.empty() ? nullptr : c.constant.data(), c.group.empty() ? nullptr : c.group.data(),
                                  (int)c.group.size(), c.intr.data(), p);
    CHECK(rc == 0, "%s: %s", name, p.error.c_str());
    if (rc) return;
    auto is_const = [&](int cam) { return !c.constant.empty() && c.constant[cam] != 0; };
    auto gid = [&](int cam) { return c.group.empty() ? -1 : c.group[cam]; };
    // expected state per camera: 0 own, 1 held, 2 live
    std::vector<int> state(c.nc, 0), first_of(c.nc, -1);
    for (int a = 0; a < c.nc; ++a) {
        if (gid(a) < 0 || c.mode != 1) continue;
        int members = 0, consts = 0, first = -1;
        for (int b = 0; b < c.nc; ++b)
            if (gid(b) == gid(a)) { ++members; consts += is_const(b); if (first < 0) first = b; }
        if (members < 2 || is_const(a)) continue;
        state[a] = consts ? 1 : 2;
        first_of[a] = first;
    }
    // live groups numbered by their smallest member
    std::vector<int> firsts;
    for (int a = 0; a < c.nc; ++a) if (state[a] == 2 && first_of[a] == a) firsts.push_back(a);
    int n = 0, n_own = 0;
    bool any = false;
    for (int a = 0; a < c.nc; ++a) {
        int pose = is_const(a) ? 0 : (a == 0 && c.fix0) ? 0 : (a == 1 && c.fix1) ? 3 : 6;
        const int own_intr = (!is_const(a) && c.mode == 1 && state[a] == 0) ? 4 : 0, member_intr = state[a] == 2 ? 4 : 0;
        CHECK(p.cam_dim[a] == pose + own_intr + member_intr, "%s: camera %d has %d columns, expected %d", name, a, p.cam_dim[a], pose + own_intr + member_intr);
        CHECK(p.cam_off[a] == n, "%s: camera %d offset", name, a);
        CHECK(p.intr_free[a] == (own_intr + member_intr > 0), "%s: camera %d intr_free", name, a);
        const int want = state[a] == 0 ? ba_tied::OWN : state[a] == 1 ? ba_tied::HELD : (int)(std::find(firsts.begin(), firsts.end(), first_of[a]) - firsts.begin());
        CHECK(p.grp[a] == want, "%s: camera %d normalised to %d, expected %d", name, a, p.grp[a], want);
        n += pose + own_intr + member_intr;
        n_own += pose + own_intr;
        any = any || state[a] != 0;
    }
    CHECK(p.tied == any, "%s: tied", name);
    CHECK(p.n == n && p.cam_off[c.nc] == n, "%s: n = %d, expected %d", name, p.n, n);
    CHECK(p.n_own == n_own && p.n_groups == (int)firsts.size(), "%s: n_own / n_groups", name);
    CHECK(p.n_tied == n_own + 4 * (int)firsts.size(), "%s: n' = %d, expected %d", name, p.n_tied, n_own + 4 * (int)firsts.size());
    // the map: a function onto 0 .. n' - 1, own columns in order, members onto their group's four
    CHECK((int)p.map.size() == n && (int)p.src.size() == n && (int)p.src_off.size() == p.n_tied + 1, "%s: sizes", name);
    std::set<int> hit;
    int next_own = 0;
    static const int icol[4] = {6, 7, 10, 11};
    for (int a = 0; a < c.nc; ++a)
        for (int k = 0; k < p.cam_dim[a]; ++k) {
            const int i = p.cam_off[a] + k, t = p.map[i];
            CHECK(t >= 0 && t < p.n_tied, "%s: map[%d] = %d", name, i, t);
            hit.insert(t);
            const bool intr_col = k >= p.cam_dim[a] - (p.intr_free[a] ? 4 : 0);
            if (intr_col) CHECK(p.cols[10 * a + k] == icol[k - (p.cam_dim[a] - 4)], "%s: camera %d column %d", name, a, k);
            else CHECK(p.cols[10 * a + k] == k, "%s: camera %d pose column %d", name, a, k);
            if (state[a] == 2 && intr_col) CHECK(t == p.n_own + 4 * p.grp[a] + (k - (p.cam_dim[a] - 4)), "%s: member column", name);
            else { CHECK(t == next_own, "%s: own column %d -> %d, expected %d", name, i, t, next_own); ++next_own; }
        }
    CHECK((int)hit.size() == p.n_tied, "%s: the map is not onto", name);
    // sources: ascending, and exactly the preimages
    CHECK(p.src_off[0] == 0 && p.src_off[p.n_tied] == n, "%s: src_off ends", name);
    for (int t = 0; t < p.n_tied; ++t) {
        CHECK(p.src_off[t + 1] > p.src_off[t], "%s: tied column %d has no source", name, t);
        for (int e = p.src_off[t]; e < p.src_off[t + 1]; ++e) {
            CHECK(p.map[p.src[e]] == t, "%s: source of %d", name, t);
            if (e > p.src_off[t]) CHECK(p.src[e] > p.src[e - 1], "%s: sources of %d not ascending", name, t);
        }
        CHECK(t >= p.n_own || p.src_off[t + 1] - p.src_off[t] == 1, "%s: own column %d with several sources", name, t);
    }
    // members CSR
    CHECK((int)p.grp_off.size() == p.n_groups + 1, "%s: grp_off", name);
    for (int g = 0; g < p.n_groups; ++g) {
        CHECK(p.grp_cam[p.grp_off[g]] == firsts[g], "%s: group %d starts at %d", name, g, p.grp_cam[p.grp_off[g]]);
        CHECK(p.grp_off[g + 1] - p.grp_off[g] >= 2, "%s: group %d has one member", name, g);
        for (int e = p.grp_off[g]; e < p.grp_off[g + 1]; ++e) {
            CHECK(p.grp[p.grp_cam[e]] == g, "%s: member list of %d", name, g);
            if (e > p.grp_off[g]) CHECK(p.grp_cam[e] > p.grp_cam[e - 1], "%s: members of %d not ascending", name, g);
        }
    }
}

static Case make(std::mt19937 &rng, int nc, int mode, bool fix0, bool fix1, int kind)
{
    Case c{nc, mode, fix0, fix1, {}, {}, std::vector<double>(6 * (size_t)nc)};
    // kind: 0 no array, 1 all -1, 2 one group of all, 3 several groups + singletons + own, 4 as 3 with constant cameras
    if (kind >= 1) c.group.assign(nc, -1);
    if (kind == 2) c.group.assign(nc, 3);
    if (kind >= 3) {
        const int ids[5] = {7, 0, 42, 3, 1000000};
        for (int a = 0; a < nc; ++a) { const int r = (int)(rng() % 7); c.group[a] = r < 5 ? ids[r] : -1; }
        if (nc > 2) c.group[nc - 1] = 99;      // a singleton
        if (nc > 3) { c.group[0] = 7; c.group[1] = 7; }      // cameras 0 and 1 inside a group
    }
    if (kind == 4) { c.constant.assign(nc, 0); for (int a = 0; a < nc; ++a) c.constant[a] = rng() % 4 == 0; }
    // intrinsics: equal within an id
    for (int a = 0; a < nc; ++a) {
        const int id = c.group.empty() || c.group[a] < 0 ? -1 - a : c.group[a];
        for (int k = 0; k < 6; ++k) c.intr[6 * a + k] = 500.0 + 0.25 * (id % 1000) + k;
    }
    return c;
}

int main()
{
    std::mt19937 rng(12345);
    int cases = 0;
    for (int nc : {1, 2, 3, 5, 12, 31, 70})
        for (int mode = 0; mode < 2; ++mode)
            for (int fix = 0; fix < 4; ++fix)
                for (int kind = 0; kind < 5; ++kind)
                    for (int rep = 0; rep < (kind >= 3 ? 6 : 1); ++rep) {
                        const Case c = make(rng, nc, mode, fix & 1, fix & 2, kind);
                        char name[96];
                        std::snprintf(name, sizeof name, "nc %d mode %d fix %d kind %d rep %d", nc, mode, fix, kind, rep);
                        check_plan(c, name);
                        ++cases;
                    }
    // n' by the formula of the design: 12 cameras, one group, default gauge: 5 * 6 + 3 + 6 * ... = 6 * 12 - 9 + 4
    {
        Case c = make(rng, 12, 1, true, true, 2);
        ba_tied::Plan p;
        CHECK(ba_tied::build(12, 1, true, true, nullptr, c.group.data(), 12, c.intr.data(), p) == 0, "one group");
        CHECK(p.n_tied == 67 && p.n == 6 * 12 - 9 + 4 * 12, "n' = %d, n = %d", p.n_tied, p.n);
    }
    // the library's own mark for a held camera
    {
        Case c = make(rng, 6, 1, false, false, 1);
        c.group = {-2, -1, 4, 4, -2, -1};
        ba_tied::Plan p;
        CHECK(ba_tied::build(6, 1, false, false, nullptr, c.group.data(), 6, c.intr.data(), p) == 1, "-2 from a caller is refused");
        c.intr.assign(36, 1.0);
        CHECK(ba_tied::build(6, 1, false, false, nullptr, c.group.data(), 6, c.intr.data(), p, true) == 0 && p.tied, "held mark");
        CHECK(p.grp[0] == ba_tied::HELD && p.grp[4] == ba_tied::HELD && p.cam_dim[0] == 6 && p.cam_dim[1] == 10 && p.n_groups == 1 && p.n_tied == 6 * 6 + 2 * 4 + 4,
              "held mark: n' = %d", p.n_tied);
    }
    // rejections
    {
        Case c = make(rng, 8, 1, true, true, 2);
        ba_tied::Plan p;
        c.intr[6 * 5 + 4] = std::nextafter(c.intr[6 * 5 + 4], 1e9);      // one bit of k1 of camera 5
        CHECK(ba_tied::build(8, 1, true, true, nullptr, c.group.data(), 8, c.intr.data(), p) == 1, "unequal members accepted");
        CHECK(p.error.find("camera 5") != std::string::npos, "message: %s", p.error.c_str());
        CHECK(ba_tied::build(8, 0, true, true, nullptr, c.group.data(), 8, c.intr.data(), p) == 1, "unequal members accepted in mode 0");
        c = make(rng, 8, 1, true, true, 2);
        c.group[3] = -2;
        CHECK(ba_tied::build(8, 1, true, true, nullptr, c.group.data(), 8, c.intr.data(), p) == 1 && p.error.find("camera 3") != std::string::npos,
              "id below -1: %s", p.error.c_str());
        c.group[3] = 3;
        CHECK(ba_tied::build(8, 1, true, true, nullptr, c.group.data(), 7, c.intr.data(), p) == 1, "wrong length accepted");
        CHECK(ba_tied::build(8, 1, true, true, nullptr, c.group.data(), 9, c.intr.data(), p) == 1, "wrong length accepted");
        CHECK(ba_tied::build(0, 1, true, true, nullptr, nullptr, 0, c.intr.data(), p) == 1, "no camera accepted");
    }
    std::printf("%d cases, %d failures\n", cases, failures);
    if (!failures) std::printf("all cases pass\n");
    return failures ? 1 : 0;
}
