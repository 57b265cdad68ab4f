// tracks_key_test -- csrc/tracks_key.h as plain host C++ (no HIP, no GPU): reads "root slot" lines from the file named on the command
// line, inserts them one by one into the open-addressing table the header sizes for that many items (the sequential form of
// k_trk_insert, tracks.hip) and prints, per line, the key, its hash, the cell it ended in and the count there; then the table size.
// tests/test_tracks_key.py compares every number with its own restatement.  Built with the address and undefined-behaviour sanitizers.
// The program itself checks the packing round trip, that no key is the empty word, and that every probe ends within the table.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../reconstructor_amd/csrc/tracks_key.h"

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: tracks_key_test ITEMS\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<int32_t> root, slot;
    long long r, s;
    while (std::fscanf(f, "%lld %lld", &r, &s) == 2) {
        if (r < 0 || r > 2147483646ll || s < 0 || s >= TRK_MAX_SLOTS) return 2;
        root.push_back((int32_t)r);
        slot.push_back((int32_t)s);
    }
    std::fclose(f);
    const unsigned long long cells = trk_table_cells(root.size());
    if (cells < TRK_MIN_CELLS || (cells & (cells - 1)) || cells < 2 * root.size() || (cells > TRK_MIN_CELLS && cells / 2 >= 2 * root.size())) {
        std::fprintf(stderr, "table of %llu cells for %zu items\n", cells, root.size());
        return 1;
    }
    std::vector<unsigned long long> keys((size_t)cells, TRK_EMPTY);
    std::vector<int32_t> cnt((size_t)cells, 0);
    for (size_t i = 0; i < root.size(); ++i) {
        const unsigned long long key = trk_key(root[i], slot[i]);
        if (key == TRK_EMPTY || trk_key_root(key) != root[i] || trk_key_slot(key) != slot[i]) { std::fprintf(stderr, "packing of item %zu\n", i); return 1; }
        unsigned long long c = trk_cell(key, cells), probes = 0;
        while (keys[(size_t)c] != TRK_EMPTY && keys[(size_t)c] != key) {
            c = trk_next_cell(c, cells);
            if (++probes >= cells) { std::fprintf(stderr, "probe of item %zu did not end\n", i); return 1; }
        }
        keys[(size_t)c] = key;
        ++cnt[(size_t)c];
        std::printf("%llu %llu %llu %d\n", key, trk_hash(key), c, cnt[(size_t)c]);
    }
    std::printf("cells %llu\n", cells);
    return 0;
}
