// spt_build.hip -- the sequential point trees (SPTs) and the upper tree of the SPT streaming step built on the GPU:
// GaussianModel.build_hierarchical_SPT and get_min_distance (scene/gaussian_model.py:184-352), the device restatement
// of the host build in spt_build.cpp (same steps, same float32 operation order; compiled with -ffp-contract=off).
//
//   staging     k_spt_stage: one thread per row packs the strided xyz / log-scale rows (device or pinned host memory)
//               and derives exp(scale), the volume, 3 x max scale and get_min_distance once per node; the same thread
//               checks its own first_child and marks it as a first child; k_spt_check_sibling then checks the
//               next_sibling of every marked row.  Both read row i only.  An out-of-range link ends the build before
//               any walk is launched.
//   upper walk  level by level from the root: a scan of the frontier's expand flags, then k_spt_upper_step appends the
//               expanding nodes' first children in order and after them those children's next siblings in order.
//               The cut's inner nodes, which number the SPTs, are the visited list filtered by one scan at the end:
//               level by level in frontier order, as the host's cut holds them.
//   SPT walks   all candidate roots are level 0 of one forest walk.  A level is every SPT's firsts, then every SPT's
//               seconds, each in parent order; restricted to one SPT that is the SPT's own walk order (by induction
//               over the levels), so the global entry index is the tie order of the sort.
//   sort        kept entries are compacted in entry order and sorted by two stable radix sorts: max distance
//               descending, then SPT number.
//   upper tree  the upper set is a flag per node, so its sorted order and every searchsorted are one prefix sum.
//   radii       bottom-up over the links the walks followed: the second child to arrive computes its parent.  Each
//               parent is a function of its children's final values and max is exact, so the schedule does not show.
//   n-ary mode  (hlgs_spt_build_device_nary; include/hlgs.h, "the n-ary contract") the same stages over child lists of
//               child_count members in rank-major order: k_spt_validate_nary in place of the two link checks, the
//               k_spt_nary_* level step (walk_levels_nary) in place of the two step kernels, k_spt_radii_nary with
//               child_count arrivals.  The binary kernels and their launches are untouched.
// Every append is checked against the capacity G, every node may be reached once (a second visit is an error, which
// ends cycles and shared children), and no kernel follows links in an unbounded loop.
#include <string>

#include "hlgs_internal.h"

namespace hlgs {

int fail_msg(int code, const std::string& msg);  // capi.hip

namespace {

constexpr int kChildCount = 2, kFirstChild = 3, kNextSibling = 4;
constexpr uint32_t kErrLink = 1u, kErrTree = 2u, kErrBinary = 4u, kErrCount = 8u, kErrRoot = 16u;
constexpr uint32_t kSeen = 1u, kExpanded = 2u;
constexpr int kHdrInts = 64;  // [0] error bits, [1] n_spt, [2] n_entries, [3] n_upper, [4] candidate SPTs
constexpr int kHdrLevel = 8;  // n-ary walks: [8] children of the level, [9] its longest child list

template <typename T>
T* take(char*& p, size_t n)
{
    T* r = reinterpret_cast<T*>(p);
    p += align_up(n * sizeof(T));
    return r;
}

struct Bufs {
    int* hdr;
    float *xyz, *sc;          // 3 G: packed rows
    float *vol, *r3, *md;     // G: prod(exp(scale)), 3 max(exp(scale)), get_min_distance (-1e9 at leaves)
    uint32_t* isfirst;        // G: some node's first child
    uint32_t* seen;           // G: kSeen | kExpanded
    uint32_t *up, *upincl;    // G: member of the upper tree, and its inclusive scan
    int* lpar;                // G: the node whose links led here
    int* sptof;               // G: candidate number of a kept SPT root, else -1
    int* front;               // G: the upper walk's visited list
    uint32_t *fe, *fcut;      // G: per visited entry: expands / inner node of the cut
    uint32_t* se;             // G: scan output of a level (both walks)
    int* cand;                // G: candidate SPT roots
    uint32_t *cnt, *bsr;      // G: rows and bounding radius (float bits) per candidate
    uint32_t *keep, *numincl, *cntincl;  // G: kept, scan of kept, scan of the kept sizes
    int *e_node, *e_spt;      // G: forest entries
    float *e_min, *e_max;
    uint32_t *eh, *ekeep, *eincl;
    uint32_t *keys, *vals, *keys_t, *vals_t, *hist, *scan_tmp;
    float* rad;               // G
    uint32_t* arrive;         // G
};

Bufs carve(void* base, size_t G, size_t* total)
{
    char* p = static_cast<char*>(base);
    Bufs b;
    b.hdr = take<int>(p, kHdrInts);
    b.xyz = take<float>(p, 3 * G);
    b.sc = take<float>(p, 3 * G);
    b.vol = take<float>(p, G);
    b.r3 = take<float>(p, G);
    b.md = take<float>(p, G);
    b.isfirst = take<uint32_t>(p, G);
    b.seen = take<uint32_t>(p, G);
    b.up = take<uint32_t>(p, G);
    b.upincl = take<uint32_t>(p, G);
    b.lpar = take<int>(p, G);
    b.sptof = take<int>(p, G);
    b.front = take<int>(p, G);
    b.fe = take<uint32_t>(p, G);
    b.fcut = take<uint32_t>(p, G);
    b.se = take<uint32_t>(p, G);
    b.cand = take<int>(p, G);
    b.cnt = take<uint32_t>(p, G);
    b.bsr = take<uint32_t>(p, G);
    b.keep = take<uint32_t>(p, G);
    b.numincl = take<uint32_t>(p, G);
    b.cntincl = take<uint32_t>(p, G);
    b.e_node = take<int>(p, G);
    b.e_spt = take<int>(p, G);
    b.e_min = take<float>(p, G);
    b.e_max = take<float>(p, G);
    b.eh = take<uint32_t>(p, G);
    b.ekeep = take<uint32_t>(p, G);
    b.eincl = take<uint32_t>(p, G);
    b.keys = take<uint32_t>(p, G);
    b.vals = take<uint32_t>(p, G);
    b.keys_t = take<uint32_t>(p, G);
    b.vals_t = take<uint32_t>(p, G);
    const size_t nh = radix_hist_elems(G);
    b.hist = take<uint32_t>(p, nh);
    b.scan_tmp = take<uint32_t>(p, scan_scratch_elems(nh > G ? nh : G));
    b.rad = take<float>(p, G);
    b.arrive = take<uint32_t>(p, G);
    if (total) *total = (size_t)(p - static_cast<char*>(base));
    return b;
}

__device__ __forceinline__ float mx(float a, float b) { return a < b ? b : a; }  // std::max

// ------------------------------------------------------------------------------------------------ staging, validation
template <bool NARY>
__global__ void __launch_bounds__(256) k_spt_stage(int G, const int* __restrict__ nodes, const float* __restrict__ xyz,
                                                   int64_t sx, const float* __restrict__ sc, int64_t ss, float tg, Bufs b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= G) return;
    float e[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        b.xyz[3 * (size_t)i + c] = xyz[(size_t)i * sx + c];
        const float l = sc[(size_t)i * ss + c];
        b.sc[3 * (size_t)i + c] = l;
        e[c] = (float)exp((double)l);  // the correctly rounded float32 exponential
    }
    const int cc = nodes[6 * (size_t)i + kChildCount], fc = nodes[6 * (size_t)i + kFirstChild];
    b.vol[i] = e[0] * e[1] * e[2];
    b.r3[i] = mx(e[0], mx(e[1], e[2])) * 3.0f;
    b.md[i] = cc == 0 ? -1000000000.f : sqrtf(e[0] * e[1] + e[0] * e[2] + e[1] * e[2]) / tg;
    if (NARY) return;  // the child lists are checked by k_spt_validate_nary
    if (fc >= G)
        atomicOr((uint32_t*)b.hdr, kErrLink);
    else if (fc >= 0 && (cc != 0 || fc > 0))
        b.isfirst[fc] = 1u;
}

__global__ void __launch_bounds__(256) k_spt_check_sibling(int G, const int* __restrict__ nodes, Bufs b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= G) return;
    if (b.isfirst[i] && nodes[6 * (size_t)i + kNextSibling] >= G) atomicOr((uint32_t*)b.hdr, kErrLink);
}

// n-ary link validation (hlgs.h, the n-ary contract 1): the thread of a parent walks its list for exactly child_count
// members; a member must lie in [root, G) (not among the skybox rows), must not be the root, and is claimed once (isfirst, an integer exchange).  After
// it the rows reachable from the root form a tree, and every list the walks follow ends within child_count links.
__global__ void __launch_bounds__(256) k_spt_validate_nary(int G, const int* __restrict__ nodes, int root, Bufs b)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= G || v < root) return;  // rows before the root are skybox rows: their node columns are not read
    const int cc = nodes[6 * (size_t)v + kChildCount];
    if (cc < 0 || cc >= G) {
        atomicOr((uint32_t*)b.hdr, kErrCount);
        return;
    }
    int m = nodes[6 * (size_t)v + kFirstChild];
    for (int r = 0; r < cc; r++) {
        if (m < root || m >= G) {
            atomicOr((uint32_t*)b.hdr, kErrLink);
            return;
        }
        if (m == root) {
            atomicOr((uint32_t*)b.hdr, kErrRoot);
            return;
        }
        if (atomicExch(&b.isfirst[m], 1u)) {
            atomicOr((uint32_t*)b.hdr, kErrTree);
            return;
        }
        m = nodes[6 * (size_t)m + kNextSibling];
    }
}

// ------------------------------------------------------------------------------------------------ upper walk
__device__ __forceinline__ void up_classify(const int* nodes, const Bufs& b, int v, int q, float volume)
{
    const bool inner = nodes[6 * (size_t)v + kChildCount] != 0;
    const bool expand = inner && b.vol[v] > volume;
    b.fe[q] = expand ? 1u : 0u;
    b.fcut[q] = inner && !expand ? 1u : 0u;
}

__device__ __forceinline__ void up_append(int G, const int* nodes, const Bufs& b, int v, int q, int parent, float volume)
{
    if (q >= G) {
        atomicOr((uint32_t*)b.hdr, kErrTree);
        return;
    }
    b.front[q] = v;
    if (atomicExch(&b.seen[v], kSeen)) {  // reached twice: a cycle or a shared child
        atomicOr((uint32_t*)b.hdr, kErrTree);
        b.fe[q] = 0u;
        b.fcut[q] = 0u;
        return;
    }
    b.up[v] = 1u;
    b.lpar[v] = parent;
    up_classify(nodes, b, v, q, volume);
}

// a slot of the next level whose node could not be read: in range and inert (the build fails on the error word)
__device__ __forceinline__ void up_blank(int G, const Bufs& b, int q)
{
    if (q < 0 || q >= G) return;
    b.front[q] = 0;
    b.fe[q] = 0u;
    b.fcut[q] = 0u;
}

__global__ void k_spt_upper_seed(int G, const int* __restrict__ nodes, int root, float volume, Bufs b)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) up_append(G, nodes, b, root, 0, -1, volume);
}

// level [lo, lo + n): H of its entries expand (se = the inclusive scan of their flags); the next level starts at hi
__global__ void __launch_bounds__(256) k_spt_upper_step(int G, const int* __restrict__ nodes, int lo, int n, int H,
                                                        int hi, float volume, Bufs b)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = lo + t;
    if (!b.fe[i]) return;
    const int j = (int)b.se[i] - 1, p = b.front[i];
    const int f = nodes[6 * (size_t)p + kFirstChild];
    const bool okf = (unsigned)f < (unsigned)G;
    const int s = okf ? nodes[6 * (size_t)f + kNextSibling] : -1;
    const int qf = hi + j, qs = hi + H + j;
    if (!okf || (unsigned)s >= (unsigned)G || j < 0 || j >= H || qs >= G) {
        atomicOr((uint32_t*)b.hdr, !okf || (unsigned)s >= (unsigned)G ? kErrLink : kErrTree);
        up_blank(G, b, qf);
        up_blank(G, b, qs);
        return;
    }
    atomicOr(&b.seen[p], kExpanded);
    up_append(G, nodes, b, f, qf, p, volume);
    up_append(G, nodes, b, s, qs, p, volume);
}

// ------------------------------------------------------------------------------------------------ SPT forest walk
// does the SPT walk descend below v?  (first_child > 0, spt_build.cpp:129-150; a first child without a second, or the
// reverse, is the host's "needs a binary hierarchy")
__device__ __forceinline__ uint32_t spt_has_children(int G, const int* nodes, const Bufs& b, int v)
{
    const int f = nodes[6 * (size_t)v + kFirstChild];
    if (f >= G) {
        atomicOr((uint32_t*)b.hdr, kErrLink);
        return 0u;
    }
    const int s = f >= 0 ? nodes[6 * (size_t)f + kNextSibling] : 0;
    if ((f > 0) != (s > 0)) {
        atomicOr((uint32_t*)b.hdr, kErrBinary);
        return 0u;
    }
    if (s >= G) {
        atomicOr((uint32_t*)b.hdr, kErrLink);
        return 0u;
    }
    return f > 0 ? 1u : 0u;
}

// T visited entries of the upper walk, fcut scanned into se: candidate k is the k-th inner node of the cut
template <bool NARY>
__global__ void __launch_bounds__(256) k_spt_candidates(int G, const int* __restrict__ nodes, int T, Bufs b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T || !b.fcut[i]) return;
    const int k = (int)b.se[i] - 1, v = b.front[i];
    if ((unsigned)k >= (unsigned)G) return;
    b.cand[k] = v;
    b.e_node[k] = v;
    b.e_spt[k] = k;
    b.e_min[k] = b.md[v];
    b.e_max[k] = 1000000000000.f;
    b.cnt[k] = 1u;
    b.bsr[k] = __float_as_uint(b.r3[v]);
    b.eh[k] = NARY ? 1u : spt_has_children(G, nodes, b, v);  // (an inner node of the cut: child_count != 0)
}

template <bool NARY = false>
__device__ __forceinline__ void spt_append(int G, const int* nodes, const Bufs& b, int c, int q, int parent, int k,
                                           float pmin, const float* centre)
{
    uint32_t has = 0u;
    if (atomicExch(&b.seen[c], kSeen))
        atomicOr((uint32_t*)b.hdr, kErrTree);
    else
        has = NARY ? (nodes[6 * (size_t)c + kChildCount] > 0 ? 1u : 0u) : spt_has_children(G, nodes, b, c);
    b.lpar[c] = parent;
    const float d0 = b.xyz[3 * (size_t)c] - centre[0], d1 = b.xyz[3 * (size_t)c + 1] - centre[1],
                d2 = b.xyz[3 * (size_t)c + 2] - centre[2];
    const float cd = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
    const float m = b.md[c] + cd;
    b.e_node[q] = c;
    b.e_spt[q] = k;
    b.e_max[q] = pmin;
    b.e_min[q] = m < pmin ? m : pmin;
    b.eh[q] = has;
    atomicMax(&b.bsr[k], __float_as_uint(cd + b.r3[c]));  // both terms >= 0: the bit order is the float order
}

__device__ __forceinline__ void spt_blank(int G, const Bufs& b, int q, int k)
{
    if (q < 0 || q >= G) return;
    b.e_node[q] = 0;
    b.e_spt[q] = k;
    b.e_min[q] = 0.f;
    b.e_max[q] = 0.f;
    b.eh[q] = 0u;
}

__global__ void __launch_bounds__(256) k_spt_forest_step(int G, const int* __restrict__ nodes, int lo, int n, int H,
                                                         int hi, Bufs b)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = lo + t;
    if (!b.eh[i]) return;
    const int j = (int)b.se[i] - 1, p = b.e_node[i], k = b.e_spt[i];
    const int f = nodes[6 * (size_t)p + kFirstChild];
    const bool okf = f > 0 && f < G;
    const int s = okf ? nodes[6 * (size_t)f + kNextSibling] : -1;
    const int qf = hi + j, qs = hi + H + j;
    if (!okf || s <= 0 || s >= G || j < 0 || j >= H || qs >= G) {  // cannot happen after spt_has_children; stay in range
        atomicOr((uint32_t*)b.hdr, kErrTree);
        spt_blank(G, b, qf, k);
        spt_blank(G, b, qs, k);
        return;
    }
    const int cn = b.cand[k];
    const float centre[3] = {b.xyz[3 * (size_t)cn], b.xyz[3 * (size_t)cn + 1], b.xyz[3 * (size_t)cn + 2]};
    const float pmin = b.e_min[i];
    atomicOr(&b.seen[p], kExpanded);
    spt_append(G, nodes, b, f, qf, p, k, pmin, centre);
    spt_append(G, nodes, b, s, qs, p, k, pmin, centre);
    atomicAdd(&b.cnt[k], 2u);
}

// ------------------------------------------------------------------------------------------------ n-ary level step
// One level of either walk in n-ary mode.  ids = the walk's entry list (front or e_node), flags = its expand flags.
//   k_spt_nary_counts   w[i] = child_count of an expanding entry, else 0 (ekeep); the longest list (integer atomicMax)
//   (scan of w, k_spt_nary_tail: the level's children and longest list in two header words, one read-back)
//   k_spt_nary_scatter  the thread of a parent walks its list for exactly w members and writes them parent-major
//                       (eincl: child, arrive: the parent's entry), with the rank as a sort key
//   (a stable radix sort on the rank makes the order rank-major; skipped when every list has one member)
//   k_spt_nary_upper / k_spt_nary_forest  one thread per child appends it at its rank-major slot
__global__ void __launch_bounds__(256) k_spt_nary_counts(const int* __restrict__ nodes, int lo, int n,
                                                         const uint32_t* __restrict__ flags,
                                                         const int* __restrict__ ids, Bufs b)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = lo + t;
    const int w = flags[i] ? nodes[6 * (size_t)ids[i] + kChildCount] : 0;
    b.ekeep[i] = w > 0 ? (uint32_t)w : 0u;
    if (w > 0) atomicMax(&b.hdr[kHdrLevel + 1], w);
}

__global__ void k_spt_nary_tail(int last, Bufs b)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) b.hdr[kHdrLevel] = (int)b.se[last];
}

__global__ void __launch_bounds__(256) k_spt_nary_scatter(int G, const int* __restrict__ nodes, int lo, int n, int S,
                                                          const int* __restrict__ ids, int forest, Bufs b)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const int i = lo + t;
    const uint32_t w = b.ekeep[i];
    if (!w) return;
    const int64_t base = (int64_t)b.se[i] - w;
    const int p = ids[i];
    if (base < 0 || base + w > S) {
        atomicOr((uint32_t*)b.hdr, kErrTree);
        return;
    }
    int m = nodes[6 * (size_t)p + kFirstChild];
    for (uint32_t r = 0; r < w; r++) {
        const bool ok = (unsigned)m < (unsigned)G;
        if (!ok) atomicOr((uint32_t*)b.hdr, kErrLink);  // cannot happen after the validation; stay in range
        b.eincl[base + r] = ok ? (uint32_t)m : 0u;
        b.arrive[base + r] = (uint32_t)i;
        b.keys[base + r] = r;
        b.vals[base + r] = (uint32_t)(base + r);
        m = ok ? nodes[6 * (size_t)m + kNextSibling] : 0;
    }
    atomicOr(&b.seen[p], kExpanded);
    if (forest) atomicAdd(&b.cnt[b.e_spt[i]], w);
}

__global__ void __launch_bounds__(256) k_spt_nary_upper(int G, const int* __restrict__ nodes, int S, int hi,
                                                        float volume, Bufs b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= S) return;
    const uint32_t pm = b.vals[q];
    if (pm >= (uint32_t)S) {
        atomicOr((uint32_t*)b.hdr, kErrTree);
        up_blank(G, b, hi + q);
        return;
    }
    const uint32_t c = b.eincl[pm], i = b.arrive[pm];
    if (c >= (uint32_t)G || i >= (uint32_t)G) {  // a slot its parent did not write: cannot happen; stay in range
        atomicOr((uint32_t*)b.hdr, kErrTree);
        up_blank(G, b, hi + q);
        return;
    }
    up_append(G, nodes, b, (int)c, hi + q, b.front[i], volume);
}

__global__ void __launch_bounds__(256) k_spt_nary_forest(int G, const int* __restrict__ nodes, int S, int hi, Bufs b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= S || hi + q >= G) return;
    const uint32_t pm = b.vals[q];
    if (pm >= (uint32_t)S) {
        atomicOr((uint32_t*)b.hdr, kErrTree);
        spt_blank(G, b, hi + q, 0);
        return;
    }
    const uint32_t c = b.eincl[pm], iu = b.arrive[pm];
    if (c >= (uint32_t)G || iu >= (uint32_t)G || (uint32_t)b.e_spt[iu] >= (uint32_t)G) {  // cannot happen; stay in range
        atomicOr((uint32_t*)b.hdr, kErrTree);
        spt_blank(G, b, hi + q, 0);
        return;
    }
    const int i = (int)iu, k = b.e_spt[i], cn = b.cand[k];
    const float centre[3] = {b.xyz[3 * (size_t)cn], b.xyz[3 * (size_t)cn + 1], b.xyz[3 * (size_t)cn + 2]};
    spt_append<true>(G, nodes, b, (int)c, hi + q, b.e_node[i], k, b.e_min[i], centre);
}

// ------------------------------------------------------------------------------------------------ selection, sort keys
__global__ void __launch_bounds__(256) k_spt_keep(int K, int min_size, Bufs b)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    const uint32_t c = b.cnt[k];
    const bool kp = (int64_t)c > (int64_t)min_size;
    b.keep[k] = kp ? 1u : 0u;
    b.cntincl[k] = kp ? c : 0u;
    if (kp) b.sptof[b.cand[k]] = k;
}

// entries of dropped walks join the upper tree (their roots are in it already)
__global__ void __launch_bounds__(256) k_spt_entry_flags(int K, int E, Bufs b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E) return;
    const uint32_t kp = b.keep[b.e_spt[i]];
    b.ekeep[i] = kp;
    if (!kp && i >= K) b.up[b.e_node[i]] = 1u;
}

__global__ void k_spt_sizes(int G, int K, int E, Bufs b)
{
    if (threadIdx.x || blockIdx.x) return;
    b.hdr[1] = K ? (int)b.numincl[K - 1] : 0;
    b.hdr[2] = E ? (int)b.eincl[E - 1] : 0;
    b.hdr[3] = (int)b.upincl[G - 1];
    b.hdr[4] = K;
}

__device__ __forceinline__ uint32_t descending_key(float f)
{
    uint32_t u = __float_as_uint(f + 0.0f);  // -0 sorts as +0
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}

__global__ void __launch_bounds__(256) k_spt_max_keys(int E, Bufs b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= E || !b.ekeep[i]) return;
    const uint32_t q = b.eincl[i] - 1u;
    b.keys[q] = descending_key(b.e_max[i]);
    b.vals[q] = (uint32_t)i;
}

__global__ void __launch_bounds__(256) k_spt_number_keys(int n, Bufs b)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    b.keys[q] = b.numincl[b.e_spt[b.vals[q]]] - 1u;
}

// ------------------------------------------------------------------------------------------------ emit
__global__ void __launch_bounds__(256) k_spt_emit_starts(int G, int n_spt, Bufs b, int* starts, int* roots)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k == 0) starts[0] = 0;
    if (k >= G || k >= b.hdr[4] || !b.keep[k]) return;
    const int n = (int)b.numincl[k];
    if (n > n_spt) return;
    starts[n] = (int)b.cntincl[k];
    roots[n - 1] = b.cand[k];
}

__global__ void __launch_bounds__(256) k_spt_emit_entries(int G, int n, Bufs b, float* smax, float* smin, int* gidx)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n || q >= b.hdr[2]) return;
    const uint32_t i = b.vals[q];
    if (i >= (uint32_t)G) return;
    smax[q] = b.e_max[i];
    smin[q] = b.e_min[i];
    gidx[q] = b.e_node[i];
}

// torch.searchsorted(upper, v): the number of upper-tree nodes below v
__device__ __forceinline__ int lower_bound_upper(int G, int U, const Bufs& b, int v)
{
    return v < 0 ? 0 : v >= G ? U : (int)(b.upincl[v] - b.up[v]);
}

template <bool NARY>
__global__ void __launch_bounds__(256) k_spt_emit_upper(int G, int U, const int* __restrict__ nodes, Bufs b,
                                                        int* up_nodes, float* up_xyz, float* up_scaling)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= G || !b.up[v]) return;
    const int i = (int)b.upincl[v] - 1;
    if (i >= U || i >= b.hdr[3]) return;
    const int* nd = nodes + 6 * (size_t)v;
    int* o = up_nodes + 6 * (size_t)i;
    const int k = b.sptof[v];
    o[0] = nd[0];
    o[1] = i == 0 ? -1 : lower_bound_upper(G, U, b, nd[1]);
    if (k >= 0) {  // an SPT leaf
        o[2] = 0;
        o[3] = (int)b.numincl[k] - 1;
    } else {
        o[2] = nd[2];
        o[3] = (NARY ? nd[2] == 0 : nd[3] == 0) ? -1 : lower_bound_upper(G, U, b, nd[3]);
    }
    o[4] = nd[4] > 0 ? lower_bound_upper(G, U, b, nd[4]) : nd[4];
    o[5] = v;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        up_xyz[3 * (size_t)i + c] = b.xyz[3 * (size_t)v + c];
        up_scaling[3 * (size_t)i + c] = b.sc[3 * (size_t)v + c];
    }
}

__global__ void __launch_bounds__(256) k_spt_emit_min_d2(int G, int U, Bufs b, const int* __restrict__ up_nodes,
                                                         float* min_d2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= U || U != b.hdr[3]) return;
    int p = up_nodes[6 * (size_t)i + 1];
    if (p < 0) p += U;
    if (p < 0 || p >= U) p = U - 1;  // a parent column that names no upper-tree row
    const int g = up_nodes[6 * (size_t)p + 5];
    const float m = (unsigned)g < (unsigned)G ? b.md[g] : 0.f;
    min_d2[i] = i == 0 ? 1000000000000.f : m * m;
}

// bottom-up radii over the links the walks followed: a leaf of the upper tree starts with its own radius; at every
// parent the first child to arrive stops, the second one reads both children and goes on
__global__ void __launch_bounds__(256) k_spt_radii(int G, int U, const int* __restrict__ nodes, Bufs b, float* radii)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= G || !b.up[v]) return;
    const int k = b.sptof[v];
    if (k < 0 && (b.seen[v] & kExpanded)) return;
    float r = k >= 0 ? __uint_as_float(b.bsr[k]) : nodes[6 * (size_t)v + kFirstChild] == 0 ? b.r3[v] : 0.f;
    int cur = v;
    for (int it = 0; it <= U; it++) {
        __hip_atomic_store(&b.rad[cur], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int row = (int)b.upincl[cur] - 1;
        if (row >= 0 && row < U) radii[row] = r;
        const int p = b.lpar[cur];
        if (p < 0 || p >= G || !b.up[p]) return;
        if (__hip_atomic_fetch_add(&b.arrive[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0u) return;
        const int f = nodes[6 * (size_t)p + kFirstChild];
        if ((unsigned)f >= (unsigned)G) return;
        const int s = nodes[6 * (size_t)f + kNextSibling];
        if ((unsigned)s >= (unsigned)G) return;
        const float rf = __hip_atomic_load(&b.rad[f], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float rs = __hip_atomic_load(&b.rad[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float* pp = b.xyz + 3 * (size_t)p;
        const float* pf = b.xyz + 3 * (size_t)f;
        const float* ps = b.xyz + 3 * (size_t)s;
        const float a0 = pp[0] - pf[0], a1 = pp[1] - pf[1], a2 = pp[2] - pf[2];
        const float c0 = pp[0] - ps[0], c1 = pp[1] - ps[1], c2 = pp[2] - ps[2];
        r = mx(rf + sqrtf(a0 * a0 + a1 * a1 + a2 * a2), rs + sqrtf(c0 * c0 + c1 * c1 + c2 * c2));
        cur = p;
    }
}

// n-ary: the last of a parent's child_count children to arrive computes it, over the whole list (the max is exact, so
// the schedule does not show)
__global__ void __launch_bounds__(256) k_spt_radii_nary(int G, int U, const int* __restrict__ nodes, Bufs b,
                                                        float* radii)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= G || !b.up[v]) return;
    const int k = b.sptof[v];
    if (k < 0 && (b.seen[v] & kExpanded)) return;
    float r = k >= 0 ? __uint_as_float(b.bsr[k]) : nodes[6 * (size_t)v + kChildCount] == 0 ? b.r3[v] : 0.f;
    int cur = v;
    for (int it = 0; it <= U; it++) {
        __hip_atomic_store(&b.rad[cur], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int row = (int)b.upincl[cur] - 1;
        if (row >= 0 && row < U) radii[row] = r;
        const int p = b.lpar[cur];
        if (p < 0 || p >= G || !b.up[p]) return;
        const int cc = nodes[6 * (size_t)p + kChildCount];
        if (__hip_atomic_fetch_add(&b.arrive[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + 1u != (uint32_t)cc)
            return;
        const float* pp = b.xyz + 3 * (size_t)p;
        int m = nodes[6 * (size_t)p + kFirstChild];
        r = -INFINITY;
        for (int j = 0; j < cc; j++) {
            if ((unsigned)m >= (unsigned)G) return;
            const float rm = __hip_atomic_load(&b.rad[m], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float* pc = b.xyz + 3 * (size_t)m;
            const float a0 = pp[0] - pc[0], a1 = pp[1] - pc[1], a2 = pp[2] - pc[2];
            r = mx(r, rm + sqrtf(a0 * a0 + a1 * a1 + a2 * a2));
            m = nodes[6 * (size_t)m + kNextSibling];
        }
        cur = p;
    }
}

#define SPT_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess) return fail_msg(HLGS_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline dim3 grid(size_t n) { return dim3((unsigned)((n + 255) / 256)); }

int read_back(void* dst, const void* src, size_t bytes, hipStream_t s, int* syncs)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (syncs) ++*syncs;
    if (e != hipSuccess) return fail_msg(HLGS_ERR_DEVICE, std::string("SPT build read-back: ") + hipGetErrorString(e));
    return HLGS_OK;
}

int error_of(uint32_t bits)
{
    if (bits & kErrCount) return fail_msg(HLGS_ERR_ARG, "child_count out of range");
    if (bits & kErrLink) return fail_msg(HLGS_ERR_ARG, "child index out of range");
    if (bits & kErrRoot) return fail_msg(HLGS_ERR_ARG, "the root is a member of a child list");
    if (bits & kErrBinary) return fail_msg(HLGS_ERR_ARG, "SPT build needs a binary hierarchy");
    if (bits & kErrTree) return fail_msg(HLGS_ERR_ARG, "hierarchy walk does not terminate (a node is reached twice)");
    return HLGS_OK;
}

}  // namespace

size_t spt_device_scratch_bytes(int G)
{
    size_t total = 0;
    carve(nullptr, (size_t)(G > 0 ? G : 0), &total);
    return total;
}

// One level-synchronous walk over entries [0, first level) ...: scans the level's flags, reads the number of expanding
// entries back and launches `step` until a level expands nothing.  Returns the number of entries in *end.
template <typename Step>
static int walk_levels(int G, uint32_t* flags, const Bufs& b, int first, hipStream_t s, int* syncs, int* end, Step step)
{
    int lo = 0, hi = first;
    while (hi > lo) {
        const int n = hi - lo;
        scan_inclusive_u32(flags + lo, b.se + lo, (size_t)n, b.scan_tmp, s);
        uint32_t H = 0;
        if (int rc = read_back(&H, b.se + hi - 1, sizeof(H), s, syncs)) return rc;
        if (H == 0) break;
        if (H > (uint32_t)n || (size_t)hi + 2 * (size_t)H > (size_t)G)  // more rows than the table holds: not a tree
            return fail_msg(HLGS_ERR_ARG, "hierarchy walk does not terminate");
        step(lo, n, (int)H, hi);
        lo = hi;
        hi += 2 * (int)H;
        if ((size_t)hi > 4 * (size_t)G) return fail_msg(HLGS_ERR_ARG, "hierarchy walk does not terminate");
    }
    *end = hi;
    return HLGS_OK;
}

// The n-ary form of walk_levels: per level one scan of the expanding entries' list lengths and one read-back (the
// level's children and its longest list), the parent-major scatter, a stable sort on the rank unless every list has
// one member, and `append` over the children.
template <typename Append>
static int walk_levels_nary(int G, const int* nodes, uint32_t* flags, const int* ids, int forest, const Bufs& b,
                            int first, hipStream_t s, int* syncs, int* end, Append append)
{
    int lo = 0, hi = first;
    while (hi > lo) {
        const int n = hi - lo;
        if (hipMemsetAsync(b.hdr + kHdrLevel, 0, 2 * sizeof(int), s) != hipSuccess)
            return fail_msg(HLGS_ERR_DEVICE, "SPT build: memset failed");
        hipLaunchKernelGGL(k_spt_nary_counts, grid((size_t)n), dim3(256), 0, s, nodes, lo, n, flags, ids, b);
        scan_inclusive_u32(b.ekeep + lo, b.se + lo, (size_t)n, b.scan_tmp, s);
        hipLaunchKernelGGL(k_spt_nary_tail, dim3(1), dim3(64), 0, s, hi - 1, b);
        int lev[2] = {0, 0};
        if (int rc = read_back(lev, b.hdr + kHdrLevel, sizeof(lev), s, syncs)) return rc;
        const int S = lev[0];
        if (S == 0) break;
        if (S < 0 || lev[1] < 1 || (size_t)hi + (size_t)S > (size_t)G)  // more rows than the table holds: not a tree
            return fail_msg(HLGS_ERR_ARG, "hierarchy walk does not terminate");
        hipLaunchKernelGGL(k_spt_nary_scatter, grid((size_t)n), dim3(256), 0, s, G, nodes, lo, n, S, ids, forest, b);
        if (lev[1] > 1)
            radix_sort_pairs_u32((uint32_t)S, b.keys, b.vals, b.keys_t, b.vals_t, b.hist, b.scan_tmp, s);
        append(S, hi);
        lo = hi;
        hi += S;
    }
    *end = hi;
    return HLGS_OK;
}

int spt_device_build(int G, const int* nodes, const float* xyz, int64_t xyz_stride, const float* log_scales,
                     int64_t scale_stride, int root, float volume, float tg, int min_size, void* scratch, int stages,
                     int* sizes, int* syncs, bool nary, hipStream_t s)
{
    const Bufs b = carve(scratch, (size_t)G, nullptr);
    const size_t g = (size_t)G;
    uint32_t err = 0;
    if (stages & HLGS_SPT_STAGE_PACK) {
        SPT_TRY(hipMemsetAsync(b.hdr, 0, kHdrInts * sizeof(int), s));
        SPT_TRY(hipMemsetAsync(b.isfirst, 0, g * sizeof(uint32_t), s));
        if (nary) {
            hipLaunchKernelGGL(k_spt_stage<true>, grid(g), dim3(256), 0, s, G, nodes, xyz, xyz_stride, log_scales,
                               scale_stride, tg, b);
            hipLaunchKernelGGL(k_spt_validate_nary, grid(g), dim3(256), 0, s, G, nodes, root, b);
        } else {
            hipLaunchKernelGGL(k_spt_stage<false>, grid(g), dim3(256), 0, s, G, nodes, xyz, xyz_stride, log_scales,
                               scale_stride, tg, b);
            hipLaunchKernelGGL(k_spt_check_sibling, grid(g), dim3(256), 0, s, G, nodes, b);
        }
    }
    if (!(stages & HLGS_SPT_STAGE_WALK)) return HLGS_OK;
    // no link is followed before the validation has passed
    if (int rc = read_back(&err, b.hdr, sizeof(err), s, syncs)) return rc;
    if (err) return error_of(err);
    SPT_TRY(hipMemsetAsync(b.seen, 0, g * sizeof(uint32_t), s));
    SPT_TRY(hipMemsetAsync(b.up, 0, g * sizeof(uint32_t), s));
    SPT_TRY(hipMemsetAsync(b.sptof, 0xff, g * sizeof(int), s));
    // ---- upper tree and cut
    hipLaunchKernelGGL(k_spt_upper_seed, dim3(1), dim3(64), 0, s, G, nodes, root, volume, b);
    int T = 0;
    if (nary) {
        if (int rc = walk_levels_nary(G, nodes, b.fe, b.front, 0, b, 1, s, syncs, &T, [&](int S, int hi) {
                hipLaunchKernelGGL(k_spt_nary_upper, grid((size_t)S), dim3(256), 0, s, G, nodes, S, hi, volume, b);
            }))
            return rc;
    } else if (int rc = walk_levels(G, b.fe, b, 1, s, syncs, &T, [&](int lo, int n, int H, int hi) {
                   hipLaunchKernelGGL(k_spt_upper_step, grid((size_t)n), dim3(256), 0, s, G, nodes, lo, n, H, hi,
                                      volume, b);
               }))
        return rc;
    scan_inclusive_u32(b.fcut, b.se, (size_t)T, b.scan_tmp, s);
    uint32_t K = 0;
    if (int rc = read_back(&K, b.se + T - 1, sizeof(K), s, syncs)) return rc;
    if (K > (uint32_t)G) return fail_msg(HLGS_ERR_ARG, "hierarchy walk does not terminate");
    // ---- every candidate SPT at once
    int E = 0;
    if (K) {
        if (nary) {
            hipLaunchKernelGGL(k_spt_candidates<true>, grid((size_t)T), dim3(256), 0, s, G, nodes, T, b);
            if (int rc = walk_levels_nary(G, nodes, b.eh, b.e_node, 1, b, (int)K, s, syncs, &E, [&](int S, int hi) {
                    hipLaunchKernelGGL(k_spt_nary_forest, grid((size_t)S), dim3(256), 0, s, G, nodes, S, hi, b);
                }))
                return rc;
        } else {
            hipLaunchKernelGGL(k_spt_candidates<false>, grid((size_t)T), dim3(256), 0, s, G, nodes, T, b);
            if (int rc = walk_levels(G, b.eh, b, (int)K, s, syncs, &E, [&](int lo, int n, int H, int hi) {
                    hipLaunchKernelGGL(k_spt_forest_step, grid((size_t)n), dim3(256), 0, s, G, nodes, lo, n, H, hi, b);
                }))
                return rc;
        }
        hipLaunchKernelGGL(k_spt_keep, grid(K), dim3(256), 0, s, (int)K, min_size, b);
        scan_inclusive_u32(b.keep, b.numincl, K, b.scan_tmp, s);
        scan_inclusive_u32(b.cntincl, b.cntincl, K, b.scan_tmp, s);
        hipLaunchKernelGGL(k_spt_entry_flags, grid((size_t)E), dim3(256), 0, s, (int)K, E, b);
        scan_inclusive_u32(b.ekeep, b.eincl, (size_t)E, b.scan_tmp, s);
    }
    scan_inclusive_u32(b.up, b.upincl, g, b.scan_tmp, s);
    hipLaunchKernelGGL(k_spt_sizes, dim3(1), dim3(64), 0, s, G, (int)K, E, b);
    int hdr[4];
    if (int rc = read_back(hdr, b.hdr, sizeof(hdr), s, syncs)) return rc;
    if (hdr[0]) return error_of((uint32_t)hdr[0]);
    const int n_entries = hdr[2];
    if (hdr[1] < 0 || hdr[1] > (int)K || n_entries < 0 || n_entries > E || hdr[3] < 1 || hdr[3] > G)
        return fail_msg(HLGS_ERR_DEVICE, "SPT build: inconsistent sizes");
    // ---- rows of the kept SPTs: by max distance descending, then by SPT, both stable
    if (n_entries) {
        hipLaunchKernelGGL(k_spt_max_keys, grid((size_t)E), dim3(256), 0, s, E, b);
        radix_sort_pairs_u32((uint32_t)n_entries, b.keys, b.vals, b.keys_t, b.vals_t, b.hist, b.scan_tmp, s);
        hipLaunchKernelGGL(k_spt_number_keys, grid((size_t)n_entries), dim3(256), 0, s, n_entries, b);
        radix_sort_pairs_u32((uint32_t)n_entries, b.keys, b.vals, b.keys_t, b.vals_t, b.hist, b.scan_tmp, s);
    }
    sizes[0] = hdr[1];
    sizes[1] = n_entries;
    sizes[2] = hdr[3];
    return HLGS_OK;
}

int spt_device_emit(int G, const int* nodes, void* scratch, int n_spt, int n_entries, int n_upper, int* starts,
                     float* smax, float* smin, int* gidx, int* roots, int* up_nodes, float* up_xyz, float* up_scaling,
                     float* min_d2, float* radii, bool nary, hipStream_t s)
{
    const Bufs b = carve(scratch, (size_t)G, nullptr);
    hipLaunchKernelGGL(k_spt_emit_starts, grid((size_t)G), dim3(256), 0, s, G, n_spt, b, starts, roots);
    if (n_entries)
        hipLaunchKernelGGL(k_spt_emit_entries, grid((size_t)n_entries), dim3(256), 0, s, G, n_entries, b, smax, smin,
                           gidx);
    if (nary)
        hipLaunchKernelGGL(k_spt_emit_upper<true>, grid((size_t)G), dim3(256), 0, s, G, n_upper, nodes, b, up_nodes,
                           up_xyz, up_scaling);
    else
        hipLaunchKernelGGL(k_spt_emit_upper<false>, grid((size_t)G), dim3(256), 0, s, G, n_upper, nodes, b, up_nodes,
                           up_xyz, up_scaling);
    hipLaunchKernelGGL(k_spt_emit_min_d2, grid((size_t)n_upper), dim3(256), 0, s, G, n_upper, b, up_nodes, min_d2);
    if (radii) {
        SPT_TRY(hipMemsetAsync(b.arrive, 0, (size_t)G * sizeof(uint32_t), s));
        if (nary) hipLaunchKernelGGL(k_spt_radii_nary, grid((size_t)G), dim3(256), 0, s, G, n_upper, nodes, b, radii);
        else hipLaunchKernelGGL(k_spt_radii, grid((size_t)G), dim3(256), 0, s, G, n_upper, nodes, b, radii);
    }
    return HLGS_OK;
}

}  // namespace hlgs
