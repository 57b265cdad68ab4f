// tracks_host_loop -- the loop a user of the resident match lists runs today to get tracks: a plain single-thread union-find over the
// host copy of the lists with the conflict rule and the length filter of rcn_tracks_build.  Built by
// tools/tracks_timing.py with g++ -O2 as a shared object and timed there next to the device form; it is not part of the library.
//   slot_a / slot_b   per list, the position of its two images among the list images (ascending by id)
//   node_off          first node of every list image (n_slots + 1 entries)
//   counts_out        tracks, observations
// Returns the milliseconds the loop took (steady clock), the result arrays included (trk_off, obs_slot, obs_feat as std::vector).
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <numeric>
#include <vector>

extern "C" double tracks_host_loop(int32_t n_pairs, const int32_t *slot_a, const int32_t *slot_b, const int64_t *offsets, const int32_t *qt,
                                   int32_t n_slots, const int64_t *node_off, int32_t min_length, int32_t max_length, int32_t drop_image,
                                   int64_t *counts_out)
{
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t n = (int32_t)node_off[n_slots];
    std::vector<int32_t> parent((size_t)n);
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
    for (int32_t p = 0; p < n_pairs; ++p) {
        const int32_t oa = (int32_t)node_off[slot_a[p]], ob = (int32_t)node_off[slot_b[p]];
        for (int64_t e = offsets[p]; e < offsets[p + 1]; ++e) {
            const int32_t a = find(oa + qt[2 * e]), b = find(ob + qt[2 * e + 1]);
            if (a < b) parent[b] = a; else if (b < a) parent[a] = b;
        }
    }
    // components as node lists (counting sort by root: node order inside a component is ascending)
    std::vector<int32_t> root((size_t)n), size((size_t)n + 1, 0);
    for (int32_t x = 0; x < n; ++x) { root[x] = find(x); ++size[(size_t)root[x] + 1]; }
    for (int32_t x = 0; x < n; ++x) size[(size_t)x + 1] += size[x];
    std::vector<int32_t> cursor(size.begin(), size.end() - 1), nodes((size_t)n), slot_of((size_t)n);
    for (int32_t s = 0; s < n_slots; ++s) std::fill(slot_of.begin() + node_off[s], slot_of.begin() + node_off[s + 1], s);
    for (int32_t x = 0; x < n; ++x) nodes[(size_t)cursor[root[x]]++] = x;
    std::vector<int32_t> trk_off(1, 0), obs_slot, obs_feat, seen((size_t)n_slots, -1), twice((size_t)n_slots, -1);
    for (int32_t r = 0; r < n; ++r) {
        const int32_t lo = size[r], hi = size[(size_t)r + 1];
        if (root[r] != r || hi - lo < 2) continue;
        bool conflict = false;
        for (int32_t k = lo; k < hi; ++k) {
            const int32_t s = slot_of[nodes[k]];
            if (seen[s] == r) { twice[s] = r; conflict = true; }
            seen[s] = r;
        }
        if (conflict && !drop_image) continue;
        const size_t before = obs_slot.size();
        for (int32_t k = lo; k < hi; ++k) {
            const int32_t s = slot_of[nodes[k]];
            if (twice[s] == r) continue;
            obs_slot.push_back(s);
            obs_feat.push_back(nodes[k] - (int32_t)node_off[s]);
        }
        const int64_t len = (int64_t)(obs_slot.size() - before);
        if (len < min_length || (max_length > 0 && len > max_length)) { obs_slot.resize(before); obs_feat.resize(before); continue; }
        trk_off.push_back((int32_t)obs_slot.size());
    }
    counts_out[0] = (int64_t)trk_off.size() - 1;
    counts_out[1] = (int64_t)obs_slot.size();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
