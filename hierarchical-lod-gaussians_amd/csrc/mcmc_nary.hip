// mcmc_nary.hip -- the selection of the MCMC relocation on an n-ary hierarchy (include/hlgs.h, "n-ary relocation").
//
// relocate_gs (scene/gaussian_model.py:1588-1698) selects on sibling pairs; a merged scene hierarchy has child lists of
// any length, and the selection over them is the one part of the relocation that scales with the scene rather than
// with the changed rows.  Two phases around one read-back, like the SPT build and emit:
//
//   count   k_select_classify   one thread per row; a row with child_count > 0 walks its own child list (at most
//                               child_count dependent steps), validates it and classifies its group.  A kept group
//                               leaves its number of freed rows m at the row of its first freed member, and marks its
//                               survivor when the survivor is promoted.
//           k_select_flags      per row: the group flag (m != 0) and the alive flag (a leaf, not flagged, not a marked
//                               survivor)
//           scan.hip x 3        group index, freed-row offset and alive position, all ascending by row
//           k_select_counts     {groups, freed rows, alive, status}
//   emit    k_select_emit       per row: an alive row writes itself; the first freed row of a kept group walks its
//                               parent's list once more and writes the group's parent, survivor, start and freed rows
//
// A group's flag sits at its first freed row, so the scans order the groups by that row: on a binary tree the ascending
// dead list of select_relocation.  Nothing depends on the launch shape: a row's words are written by one thread (its
// own, or its parent's for m and the survivor mark, which no other thread writes), the status word is an OR.
//
// The passes are memory-bound: a 24-byte node row per thread, then dependent link loads.  A list is walked by one
// thread, so a list of 3,000 children is 3,000 dependent loads in one lane; the merged scenes' longest list is 26
// (DESIGN section 5b).  Every link is checked against (sky, size) before it is used as an index, a walk takes at most
// child_count steps, and a list that ends early, runs past child_count or holds a row that names another parent sets
// the status instead of being followed.  Every store is an ordinary vector store from plain C++.
#include "hlgs_internal.h"

namespace hlgs {

struct SelectHeader {  // first words of the scratch
    int groups, freed, alive, status;
};

struct SelectScratch {
    SelectHeader* hdr;
    uint32_t* gm;      // size: m at a kept group's first freed row, else 0; then its inclusive scan
    uint8_t* surv;     // size: 1 at the survivor of a kept promote group
    uint32_t* gflag;   // size: gm != 0, then its inclusive scan
    uint32_t* aflag;   // size: alive, then its inclusive scan
    uint32_t* tmp;     // scan_scratch_elems(size)
    size_t zero_bytes; // header, gm and surv, contiguous from hdr: cleared before every count
};
static SelectScratch carve_select(void* scratch, int size, size_t* total)
{
    char* p = reinterpret_cast<char*>(align_up((size_t)scratch));
    char* const p0 = p;
    const size_t rows = align_up(sizeof(uint32_t) * (size_t)size);
    SelectScratch d;
    d.hdr = reinterpret_cast<SelectHeader*>(p);
    p += kAlign;
    d.gm = reinterpret_cast<uint32_t*>(p);
    p += rows;
    d.surv = reinterpret_cast<uint8_t*>(p);
    p += align_up((size_t)size);
    d.zero_bytes = (size_t)(p - p0);
    d.gflag = reinterpret_cast<uint32_t*>(p);
    p += rows;
    d.aflag = reinterpret_cast<uint32_t*>(p);
    p += rows;
    d.tmp = reinterpret_cast<uint32_t*>(p);
    p += align_up(sizeof(uint32_t) * scan_scratch_elems((size_t)size));
    if (total) *total = (size_t)(p - p0);
    return d;
}
size_t mcmc_select_scratch_bytes(int size)
{
    size_t t = 0;
    carve_select(nullptr, size < 0 ? 0 : size, &t);
    return t + kAlign;
}
void* mcmc_select_zero_region(void* scratch, int size, size_t* bytes)
{
    const SelectScratch d = carve_select(scratch, size, nullptr);
    *bytes = d.zero_bytes;
    return d.hdr;
}

constexpr int kDepth = 0, kParent = 1, kCount = 2, kFirst = 3, kNext = 4;  // HierarchyNode columns

// The group of parent p, from one walk of its list: the one walk of both phases.  Returns false for a list that breaks
// the contract (the caller sets the status).  first: the first freed row; surv: the promoted survivor or -1; m: freed
// rows, 0 for no kept group.  out (the emit; NULL in the count): the freed rows in their order, at most cap of them.
struct Group {
    int first, surv, m;
};
__device__ __forceinline__ bool classify_list(int p, int c_count, int size, int sky, const int* __restrict__ nodes,
                                              const uint8_t* __restrict__ dead, int* __restrict__ out, int cap,
                                              Group* g)
{
    int c = nodes[6 * (int64_t)p + kFirst];
    int k = 0, first = -1, other = -1, last = -1;
    for (int i = 0; i < c_count; i++) {
        if (c <= sky || c >= size) return false;  // out of range, the root, or a list that ends early (0 <= sky)
        const int* row = nodes + 6 * (int64_t)c;
        if (row[kParent] != p) return false;      // a member names its parent: no row sits in two lists
        if (dead[c] != 0 && row[kCount] == 0) {
            if (k == 0) first = c;
            if (out && k < cap) out[k] = c;       // the dead members land in list order
            k++;
        } else {
            other = c;
        }
        last = c;
        c = row[kNext];
    }
    if (c != 0) return false;                     // the list runs past child_count
    int a = c_count - k, surv = -1;
    if (a == 0) {                                 // every child wants to die: the last one stays, and already stands
        k--;                                      // last among the freed rows
        a = 1;
        other = last;
    } else if (a == 1 && out && k < cap) {
        out[k] = other;                           // the promoted survivor's row is freed behind the dead ones
    }
    if (a == 1) surv = other;
    const int m = k + (a == 1 ? 1 : 0);
    g->first = first;
    g->surv = surv;
    g->m = (k >= 1 && m >= 2) ? m : 0;
    return true;
}

__global__ void __launch_bounds__(256) k_select_classify(int size, int sky, const int* __restrict__ nodes,
                                                         const uint8_t* __restrict__ dead, uint32_t* __restrict__ gm,
                                                         uint8_t* __restrict__ surv, int* __restrict__ status)
{
    const int v = (int)(blockIdx.x * 256u + threadIdx.x);
    if (v < sky || v >= size) return;
    const int cc = nodes[6 * (int64_t)v + kCount];
    if (cc == 0) return;
    if (cc < 0 || cc >= size) {
        atomicOr(status, (int)HLGS_MCMC_SELECT_STATUS_LINKS);
        return;
    }
    Group g;
    if (!classify_list(v, cc, size, sky, nodes, dead, nullptr, 0, &g)) {
        atomicOr(status, (int)HLGS_MCMC_SELECT_STATUS_LINKS);
        return;
    }
    if (g.m == 0) return;
    gm[g.first] = (uint32_t)g.m;             // first and surv are members of this list: in (sky, size)
    if (g.surv >= 0) surv[g.surv] = 1;
}

__global__ void __launch_bounds__(256) k_select_flags(int size, int sky, const int* __restrict__ nodes,
                                                      const uint8_t* __restrict__ dead,
                                                      const uint32_t* __restrict__ gm,
                                                      const uint8_t* __restrict__ surv, uint32_t* __restrict__ gflag,
                                                      uint32_t* __restrict__ aflag)
{
    const int v = (int)(blockIdx.x * 256u + threadIdx.x);
    if (v >= size) return;
    gflag[v] = gm[v] != 0 ? 1u : 0u;
    aflag[v] = (v >= sky && nodes[6 * (int64_t)v + kCount] == 0 && dead[v] == 0 && surv[v] == 0) ? 1u : 0u;
}

__global__ void k_select_counts(int size, const uint32_t* __restrict__ gincl, const uint32_t* __restrict__ mincl,
                                const uint32_t* __restrict__ aincl, SelectHeader* __restrict__ hdr,
                                int* __restrict__ counts)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int status = hdr->status;
    hdr->groups = (int)gincl[size - 1];
    hdr->freed = (int)mincl[size - 1];
    hdr->alive = (int)aincl[size - 1];
    counts[0] = status ? 0 : hdr->groups;
    counts[1] = status ? 0 : hdr->freed;
    counts[2] = status ? 0 : hdr->alive;
    counts[3] = status;
}

void launch_mcmc_select_count(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch, int* counts,
                              hipStream_t s)
{
    const SelectScratch d = carve_select(scratch, size, nullptr);
    const dim3 grid((unsigned)((size + 255) / 256));
    hipLaunchKernelGGL(k_select_classify, grid, dim3(256), 0, s, size, sky, nodes, dead, d.gm, d.surv,
                       &d.hdr->status);
    hipLaunchKernelGGL(k_select_flags, grid, dim3(256), 0, s, size, sky, nodes, dead, d.gm, d.surv, d.gflag, d.aflag);
    scan_inclusive_u32(d.gflag, d.gflag, (size_t)size, d.tmp, s);
    scan_inclusive_u32(d.gm, d.gm, (size_t)size, d.tmp, s);  // the same stream: tmp is free again
    scan_inclusive_u32(d.aflag, d.aflag, (size_t)size, d.tmp, s);
    hipLaunchKernelGGL(k_select_counts, dim3(1), dim3(64), 0, s, size, d.gflag, d.gm, d.aflag, d.hdr, counts);
}

__global__ void __launch_bounds__(256) k_select_emit(int size, int sky, const int* __restrict__ nodes,
                                                     const uint8_t* __restrict__ dead,
                                                     const SelectHeader* __restrict__ hdr,
                                                     const uint32_t* __restrict__ gincl,
                                                     const uint32_t* __restrict__ mincl,
                                                     const uint32_t* __restrict__ aincl, int* __restrict__ group_parent,
                                                     int* __restrict__ group_survivor, int* __restrict__ group_start,
                                                     int* __restrict__ free_rows, int* __restrict__ alive)
{
    if (hdr->status != 0) return;
    const int v = (int)(blockIdx.x * 256u + threadIdx.x);
    if (v >= size) return;
    const uint32_t a1 = aincl[v], a0 = v ? aincl[v - 1] : 0u;
    if (a1 != a0) alive[a0] = v;                  // a0 < a1 <= hdr->alive, the length of `alive`
    const uint32_t g1 = gincl[v], g0 = v ? gincl[v - 1] : 0u;
    if (g1 == g0) return;
    // v is the first freed row of group g0 < hdr->groups; its freed rows are [start, end) of hdr->freed
    const uint32_t end = mincl[v], start = v ? mincl[v - 1] : 0u;
    const int m = (int)(end - start);
    // the count's walk again, with its checks; a table that changed after the count gives parent -1 and follows nothing
    int p = nodes[6 * (int64_t)v + kParent];
    int surv = -1;
    Group g;
    const int cc = (p >= sky && p < size) ? nodes[6 * (int64_t)p + kCount] : 0;
    if (cc > 0 && cc < size && classify_list(p, cc, size, sky, nodes, dead, free_rows + start, m, &g) && g.m == m &&
        g.first == v) {
        surv = g.surv;
    } else {
        p = -1;
    }
    group_parent[g0] = p;
    group_survivor[g0] = surv;
    group_start[g0] = (int)start;
    if ((int)g1 == hdr->groups) group_start[g1] = (int)end;
}

void launch_mcmc_select_emit(int size, int sky, const int* nodes, const uint8_t* dead, void* scratch,
                             int* group_parent, int* group_survivor, int* group_start, int* free_rows, int* alive,
                             hipStream_t s)
{
    const SelectScratch d = carve_select(scratch, size, nullptr);
    hipLaunchKernelGGL(k_select_emit, dim3((unsigned)((size + 255) / 256)), dim3(256), 0, s, size, sky, nodes, dead,
                       d.hdr, d.gflag, d.gm, d.aflag, group_parent, group_survivor, group_start, free_rows, alive);
}

}  // namespace hlgs
