// spt_nary_hostcheck.cpp -- a stand-alone, CPU-only check of the n-ary host code of the SPT path: 10^4 seeded tables of
// at most 64 rows with arbitrary integers in the link columns go through hlgs_spt_build_nary and
// hlgs_upper_tree_order_nary.  Every call must either succeed or return an error; nothing may read or write out of
// bounds, loop without end or leak.  Built with the sanitizers it exits 0 with no report:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include \
//       tools/spt_nary_hostcheck.cpp hierarchical-lod-gaussians_amd/csrc/spt_build.cpp tests/sanitize/host_shim.cpp \
//       -o spt_nary_hostcheck && ./spt_nary_hostcheck
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "../include/hlgs.h"

namespace {

// a valid random n-ary tree in breadth-first row order (child lists contiguous), leaves with first_child = id + 1
void random_tree(std::mt19937& rng, int G, std::vector<int>& nodes)
{
    nodes.assign(6 * (size_t)G, 0);
    nodes[1] = -1;
    int next = 1;
    for (int v = 0; v < G; v++) {
        int* nd = &nodes[6 * (size_t)v];
        const int room = G - next;
        const int cc = room > 0 ? (v == 0 ? 1 + (int)(rng() % room) % 5 : (int)(rng() % 4)) : 0;
        const int take = cc < room ? cc : room;
        nd[2] = take;
        nd[3] = take ? next : v + 1;
        for (int r = 0; r < take; r++) {
            int* c = &nodes[6 * (size_t)(next + r)];
            c[0] = nd[0] + 1;
            c[1] = v;
            c[4] = r + 1 < take ? next + r + 1 : 0;
        }
        next += take;
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(20240611u);
    int built = 0, rejected = 0, usable = 0, unusable = 0;
    for (int t = 0; t < 10000; t++) {
        const int G = 1 + (int)(rng() % 64);
        std::vector<int> nodes;
        random_tree(rng, G, nodes);
        // arbitrary integers in the link columns of some rows (none in one table out of eight)
        const int damage = t % 8 == 0 ? 0 : 1 + (int)(rng() % 6);
        for (int d = 0; d < damage; d++) {
            const int row = (int)(rng() % G), col = 1 + (int)(rng() % 4);
            const uint32_t r = rng();
            int v;
            switch (r % 4) {
                case 0: v = (int)(rng() % (G + 2)) - 1; break;          // near the valid range
                case 1: v = (int)rng(); break;                          // any 32-bit pattern
                case 2: v = r & 4 ? INT32_MAX : INT32_MIN; break;
                default: v = (int)(rng() % 200) - 100; break;
            }
            nodes[6 * (size_t)row + col] = v;
        }
        std::vector<float> xyz(3 * (size_t)G), sc(3 * (size_t)G);
        for (float& x : xyz) x = (float)((int)(rng() % 2001) - 1000) * 0.01f;
        for (float& x : sc) x = (float)((int)(rng() % 601) - 500) * 0.01f;
        const int root = t % 16 == 1 ? (int)(rng() % G) : 0;
        const float volume = t % 3 == 0 ? 0.f : expf((float)((int)(rng() % 12) - 9));
        hlgs_spt_result* r = nullptr;
        const int rc = hlgs_spt_build_nary(G, nodes.data(), xyz.data(), sc.data(), root, volume, 0.02f, (int)(rng() % 8),
                                           (int)(rng() % 2), &r);
        if (rc == HLGS_OK) {
            int ns = 0, ne = 0, nu = 0;
            if (!r || hlgs_spt_result_sizes(r, &ns, &ne, &nu) != HLGS_OK || nu < 1 || nu > G || ne > G || ns > G) {
                fprintf(stderr, "table %d: inconsistent sizes\n", t);
                return 1;
            }
            std::vector<int> starts(ns + 1), gidx(ne), roots(ns), up(6 * (size_t)nu);
            std::vector<float> smax(ne), smin(ne), ux(3 * (size_t)nu), us(3 * (size_t)nu), md(nu), rad(nu);
            hlgs_spt_result_copy(r, starts.data(), smax.data(), smin.data(), gidx.data(), roots.data(), up.data(),
                                 ux.data(), us.data(), md.data(), rad.data());
            if (starts[ns] != ne) {
                fprintf(stderr, "table %d: SPT starts do not end at the entry count\n", t);
                return 1;
            }
            hlgs_spt_result_free(r);
            built++;
            // the upper tree of a valid build is a tree of child lists: the order builder must be able to use it
            std::vector<char> blob(hlgs_upper_tree_order_size(nu));
            if (hlgs_upper_tree_order_nary(nu, up.data(), blob.data()) != HLGS_OK ||
                reinterpret_cast<int*>(blob.data())[2] != 1) {
                fprintf(stderr, "table %d: the upper tree of a valid build is not usable\n", t);
                return 1;
            }
        } else {
            if (r) {
                fprintf(stderr, "table %d: a result beside an error\n", t);
                return 1;
            }
            rejected++;
        }
        // the order builder takes the raw table as well (root 0)
        std::vector<char> blob(hlgs_upper_tree_order_size(G));
        if (hlgs_upper_tree_order_nary(G, nodes.data(), blob.data()) != HLGS_OK) {
            fprintf(stderr, "table %d: order builder failed\n", t);
            return 1;
        }
        (reinterpret_cast<int*>(blob.data())[2] ? usable : unusable)++;
    }
    printf("spt_nary_hostcheck: %d built, %d rejected; order blobs: %d usable, %d not\n", built, rejected, usable,
           unusable);
    return built > 500 && rejected > 500 ? 0 : 1;
}
