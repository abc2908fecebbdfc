// hier_merge.hip -- one trained chunk hierarchy (dynamic layout, rows in any order) weighted against the chunk
// centres, its weight-0 nodes dropped, the orphaned subtrees spliced onto their nearest kept ancestor and the rest
// re-linearised in pre-order under a scene root: what the reference's offline GaussianHierarchyMerger does
// (hierarchy_explicit_loader.cpp:22-150, mainHierarchyMerger.cpp:94-140, writer.cpp:99-171) with a recursion per
// chunk.  The contract is restated in include/hlgs.h (hlgs_hier_merge_*) and DESIGN.md section 5b.
//
// The tree passes are level-synchronous: the nodes are bucketed by their (validated) depth and one launch handles one
// depth, so data crosses workgroups at launch boundaries only.  Integer atomics are used where the result does not
// depend on their order (claim counts, histograms, the position of a node inside its depth bucket, which no result
// depends on); there are no float atomics.  With s(i) the kept nodes and l(i) the kept input-leaves of the input
// subtree of i (bottom-up), a parent hands each child, in list order, its first output id (base), its first leaf rank,
// its new parent, its new depth and the id at which its new parent's subtree ends (top-down); a kept node's row then
// follows in closed form.  A child list is walked by the one thread of its parent.
//
// Built with -ffp-contract=off: the weight rounds every operation on its own, as the reference's float code does.
#include <algorithm>

#include "hlgs_internal.h"

namespace hlgs {
namespace {

constexpr int kLv = kMergeLevels;
typedef uint4 __attribute__((aligned(4))) uint4_a4;  // 16-byte access at 4-byte alignment (global_load_dwordx4)

struct Scratch {
    int *hdr, *lcount, *lstart, *cursor;
    int *order, *claim, *s, *l, *cc, *base, *lbase, *npar, *ndep, *end, *src;
    float* w;
};

size_t ints(size_t n) { return align_up(n * sizeof(int)); }

Scratch carve(void* scratch, int n)
{
    char* p = static_cast<char*>(scratch);
    auto take = [&](size_t count) { int* r = reinterpret_cast<int*>(p); p += ints(count); return r; };
    Scratch sc;
    sc.hdr = take(HLGS_MERGE_HEADER_INTS + kLv);  // the read-back block: header, then the nodes per depth
    sc.lcount = sc.hdr + HLGS_MERGE_HEADER_INTS;
    sc.lstart = take(kLv + 1);
    sc.cursor = take(kLv);
    sc.claim = take(n);  // directly behind the words that are zeroed together
    sc.order = take(n);
    sc.s = take(n);
    sc.l = take(n);
    sc.cc = take(n);
    sc.base = take(n);
    sc.lbase = take(n);
    sc.npar = take(n);
    sc.ndep = take(n);
    sc.end = take(n);
    sc.src = take(n);
    sc.w = reinterpret_cast<float*>(take(n));
    return sc;
}

enum { ND_DEPTH = 0, ND_PARENT, ND_COUNT, ND_FIRST, ND_NEXT, ND_SIDE };
__device__ __forceinline__ int nd(const int* nodes, int i, int col) { return nodes[(size_t)i * 6 + col]; }

// ---------------------------------------------------------------- plan: validate, weights
// Every index a later kernel follows is checked here: ranges, parent and depth of every non-root row, and every child
// list walked for child_count members, each member claimed once.  (k_weights, one launch later, checks the claims.)
__global__ void __launch_bounds__(256) k_validate(int n, const int* __restrict__ nodes, int* claim, int* hdr)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int depth = nd(nodes, i, ND_DEPTH), par = nd(nodes, i, ND_PARENT), cnt = nd(nodes, i, ND_COUNT);
    bool bad = depth < 0 || depth > HLGS_MERGE_MAX_DEPTH || cnt < 0 || cnt >= n;
    if (i > 0 && !bad) {
        if (par < 0 || par >= n || par == i) bad = true;
        else bad = nd(nodes, par, ND_DEPTH) != depth - 1;
    }
    if (!bad) {
        int c = nd(nodes, i, ND_FIRST);
        for (int j = 0; j < cnt; j++) {
            if (c <= 0 || c >= n || nd(nodes, c, ND_PARENT) != i) { bad = true; break; }
            atomicAdd(&claim[c], 1);
            c = nd(nodes, c, ND_NEXT);
        }
    }
    if (bad) atomicOr(&hdr[0], (int)HLGS_MERGE_STATUS_LINKS);
}

// getWeight (hierarchy_explicit_loader.cpp:22-53), float32, one rounding per operation
__device__ __forceinline__ float dist3(float px, float py, float pz, const float* c)
{
    const float dx = px - c[0], dy = py - c[1], dz = pz - c[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// One LDS atomic per (wave, distinct value) instead of one per lane: the rows of a wave are mostly of one or two depths,
// and 64 lanes adding to one address serialise.  Every lane of the wave calls this; `on` lanes take part.  Returns the
// lane's rank among the wave's lanes of the same value plus the counter's value before the wave's add.
constexpr int kWeightRounds = 8;  // a block of k_weights takes 8 x 256 rows, so that zeroing and flushing its 2,048
                                  // histogram bins is spread over as many rows as there are bins
__device__ __forceinline__ int wave_count(int* counters, int value, bool on)
{
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(on);
    int rank = 0;
    while (todo) {  // uniform: todo is the same in every lane
        const int leader = __ffsll((long long)todo) - 1;
        const int v = __shfl(value, leader);
        const unsigned long long same = __ballot(on && value == v);
        int before = 0;
        if (lane == leader) before = atomicAdd(&counters[v], __popcll(same));
        before = __shfl(before, leader);
        if (on && value == v) rank = before + __popcll(same & ((1ull << lane) - 1ull));
        todo &= ~same;
    }
    return rank;
}

__global__ void __launch_bounds__(256) k_weights(int n, int k, int K, const float* __restrict__ centers,
                                                 const float* __restrict__ pos, const int* __restrict__ nodes,
                                                 const int* __restrict__ claim, float f, float* __restrict__ w,
                                                 int* hdr, int* lcount)
{
    __shared__ int hist[kLv];
    __shared__ int kept[2];
    for (int b = threadIdx.x; b < kLv; b += 256) hist[b] = 0;
    if (threadIdx.x < 2) kept[threadIdx.x] = 0;
    __syncthreads();
    int nk = 0, nl = 0;  // the wave's kept rows and kept input-leaves (the same in every lane)
    for (int r = 0; r < kWeightRounds; r++) {
        const int i = (blockIdx.x * kWeightRounds + r) * 256 + threadIdx.x;  // i < n + 2048 <= 2^30 + 2048
        int depth = -1;
        bool keep = false, leaf = false;
        if (i < n) {
            if (claim[i] != (i == 0 ? 0 : 1)) atomicOr(&hdr[0], (int)HLGS_MERGE_STATUS_LINKS);
            const float* p = i == 0 ? centers + 3 * (size_t)k : pos + 3 * (size_t)i;  // the root sits at the centre (:147)
            const float px = p[0], py = p[1], pz = p[2];
            const float dk = dist3(px, py, pz, centers + 3 * (size_t)k);
            float m = 1e12f;
            for (int j = 0; j < K; j++) {
                if (j == k) continue;
                const float d = dist3(px, py, pz, centers + 3 * (size_t)j);
                if (d < m) m = d;
            }
            float wt;
            if (dk <= (1.0f - f) * m) wt = 1.0f;
            else if (dk > (1.0f + f) * m) wt = 0.0f;
            else {
                const float a = -1.0f / ((2.0f * f) * m);
                const float b = (1.0f + f) / (2.0f * f);
                wt = a * dk + b;
            }
            w[i] = wt;
            keep = wt > 0.0f;  // false for NaN
            if (i == 0 && !keep) atomicOr(&hdr[0], (int)HLGS_MERGE_STATUS_ROOT);
            depth = nd(nodes, i, ND_DEPTH);
            leaf = nd(nodes, i, ND_COUNT) == 0;
        }
        wave_count(hist, depth, depth >= 0 && depth < kLv);
        const unsigned long long wk = __ballot(keep), wl = __ballot(keep && leaf);
        nk += __popcll(wk);
        nl += __popcll(wl);
    }
    if ((threadIdx.x & 63) == 0) {
        if (nk) atomicAdd(&kept[0], nk);
        if (nl) atomicAdd(&kept[1], nl);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < kLv; b += 256)
        if (hist[b]) atomicAdd(&lcount[b], hist[b]);
    if (threadIdx.x < 2 && kept[threadIdx.x]) atomicAdd(&hdr[1 + threadIdx.x], kept[threadIdx.x]);
}

// ---------------------------------------------------------------- emit: buckets, bottom-up, top-down, rows
// Every kernel below returns at once when the plan found a violation: nothing follows an unvalidated index.
__global__ void __launch_bounds__(1024) k_level_scan(const int* __restrict__ hdr, const int* __restrict__ lcount,
                                                     int* lstart, int* cursor)
{
    static_assert(kLv == 2048, "two depths per thread of one 1024-thread block");
    __shared__ int sm[1024];
    if (hdr[0]) return;
    const int t = threadIdx.x;
    const int a = lcount[2 * t], b = lcount[2 * t + 1];
    sm[t] = a + b;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = t >= o ? sm[t - o] : 0;
        __syncthreads();
        sm[t] += v;
        __syncthreads();
    }
    const int ex = sm[t] - (a + b);
    lstart[2 * t] = cursor[2 * t] = ex;
    lstart[2 * t + 1] = cursor[2 * t + 1] = ex + a;
    if (t == 1023) lstart[kLv] = sm[t];
}

// order[] = the node ids grouped by depth.  A block ranks its nodes per depth in LDS and takes one range per depth
// from the global cursor, so the global atomics are one per (block, depth).
__global__ void __launch_bounds__(256) k_bucket(int n, const int* __restrict__ hdr, const int* __restrict__ nodes,
                                                int* cursor, int* __restrict__ order)
{
    __shared__ int cnt[kLv];
    if (hdr[0]) return;
    for (int b = threadIdx.x; b < kLv; b += 256) cnt[b] = 0;
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int depth = i < n ? nd(nodes, i, ND_DEPTH) : -1;  // in [0, kLv): validated
    const int rank = wave_count(cnt, depth, i < n);
    __syncthreads();
    for (int b = threadIdx.x; b < kLv; b += 256)
        if (cnt[b]) cnt[b] = atomicAdd(&cursor[b], cnt[b]);
    __syncthreads();
    if (i < n) {
        const int at = cnt[depth] + rank;
        if (at < n) order[at] = i;
    }
}

__global__ void __launch_bounds__(256) k_up(int d, const int* __restrict__ hdr, const int* __restrict__ lstart,
                                            const int* __restrict__ order, const int* __restrict__ nodes,
                                            const float* __restrict__ w, int* s, int* l, int* cc)
{
    if (hdr[0]) return;
    const int at = lstart[d] + blockIdx.x * 256 + threadIdx.x;
    if (at >= lstart[d + 1]) return;
    const int i = order[at];
    const int cnt = nd(nodes, i, ND_COUNT);
    const int keep = w[i] > 0.0f ? 1 : 0;
    int S = keep, Lf = (keep && cnt == 0) ? 1 : 0, T = 0;
    int c = nd(nodes, i, ND_FIRST);
    for (int j = 0; j < cnt; j++) {
        S += s[c];
        Lf += l[c];
        T += w[c] > 0.0f ? 1 : cc[c];
        c = nd(nodes, c, ND_NEXT);
    }
    s[i] = S;
    l[i] = Lf;
    cc[i] = T;
}

struct RootSeat {
    int base, lbase, end;  // the chunk root's output id and first leaf rank, and the id its next_sibling compares to
};

__global__ void __launch_bounds__(256) k_down(int d, int n, RootSeat seat, const int* __restrict__ hdr,
                                              const int* __restrict__ lstart, const int* __restrict__ order,
                                              const int* __restrict__ nodes, const float* __restrict__ w,
                                              const int* __restrict__ s, const int* __restrict__ l, int* base,
                                              int* lbase, int* npar, int* ndep, int* end, int* __restrict__ src)
{
    if (hdr[0]) return;
    const int at = lstart[d] + blockIdx.x * 256 + threadIdx.x;
    if (at >= lstart[d + 1]) return;
    const int i = order[at];
    if (i == 0) {
        base[0] = seat.base;
        lbase[0] = seat.lbase;
        npar[0] = 0;
        ndep[0] = 1;
        end[0] = seat.end;
    }
    const int b = base[i], keep = w[i] > 0.0f ? 1 : 0;
    if (keep) {
        const int j = b - seat.base;
        if (j >= 0 && j < n) src[j] = i;
    }
    const int cnt = nd(nodes, i, ND_COUNT);
    int cb = b + keep, clb = lbase[i];
    const int cp = keep ? b : npar[i], cd = ndep[i] + keep, ce = keep ? b + s[i] : end[i];
    int c = nd(nodes, i, ND_FIRST);
    for (int j = 0; j < cnt; j++) {
        base[c] = cb;
        lbase[c] = clb;
        npar[c] = cp;
        ndep[c] = cd;
        end[c] = ce;
        cb += s[c];
        clb += l[c];
        c = nd(nodes, c, ND_NEXT);
    }
}

// The wide rows: out_t[row0 + j] = in_t[src[j]] for the kept rows j of this chunk, one table per blockIdx.y.  A lane
// owns one 16-byte aligned chunk of the destination table; where the chunk lies inside this chunk's rows and its
// source rows are consecutive, all of them (the long pre-order runs of kept rows), it is one 16-byte load at 4-byte alignment and
// one aligned store, otherwise word by word (the first and last words of the range, and the seams between runs).
struct MergeTabs {
    const uint32_t* src[4];
    uint32_t* dst[4];
    int words[4];
};

__global__ void __launch_bounds__(256) k_merge_rows(MergeTabs tabs, int n, int kept, int row0,
                                                    const int* __restrict__ hdr, const int* __restrict__ rows)
{
    if (hdr[0]) return;
    const int t = blockIdx.y;
    const int64_t words = tabs.words[t];
    const uint32_t* __restrict__ in = tabs.src[t];
    uint32_t* __restrict__ out = tabs.dst[t];
    const int64_t W0 = (int64_t)row0 * words, W1 = ((int64_t)row0 + kept) * words;
    const int64_t q1 = (W1 + 3) >> 2;
    for (int64_t q = (W0 >> 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; q < q1; q += (int64_t)gridDim.x * 256) {
        const int64_t wq = q << 2;
        const int64_t r0 = wq / words, k0 = wq - r0 * words, r1 = (wq + 3) / words;
        if (wq >= W0 && wq + 4 <= W1) {
            // every row the chunk spans (two for rows of 3 words or more, up to four for 1-word rows) must follow
            // the first one in the source as well
            const int s0 = rows[r0 - row0], s1 = rows[r1 - row0];
            bool run = (unsigned)s0 < (unsigned)n && (unsigned)s1 < (unsigned)n && (int64_t)s1 - s0 == r1 - r0;
            for (int64_t r = r0 + 1; r < r1 && run; r++) run = (int64_t)rows[r - row0] - s0 == r - r0;
            if (run) {
                *reinterpret_cast<uint4*>(out + wq) = *reinterpret_cast<const uint4_a4*>(in + (int64_t)s0 * words + k0);
                continue;
            }
        }
        int64_t r = r0, kk = k0;
        for (int e = 0; e < 4; e++) {
            const int64_t we = wq + e;
            if (we >= W0 && we < W1) {
                const int sr = rows[r - row0];
                if ((unsigned)sr < (unsigned)n) out[we] = in[(int64_t)sr * words + kk];
            }
            if (++kk == words) { kk = 0; r++; }
        }
    }
}

// The narrow part of a kept row: its node row in closed form, its opacity times the weight, and the chunk root's
// position (the centre), after k_merge_rows copied the input's.
__global__ void __launch_bounds__(256) k_finish(int n, int kept, RootSeat seat, const int* __restrict__ hdr,
                                                const int* __restrict__ src, const int* __restrict__ nodes,
                                                const float* __restrict__ alpha, const float* __restrict__ w,
                                                const int* __restrict__ s, const int* __restrict__ cc,
                                                const int* __restrict__ lbase, const int* __restrict__ npar,
                                                const int* __restrict__ ndep, const int* __restrict__ end,
                                                const float* __restrict__ center, int* __restrict__ out_nodes,
                                                float* __restrict__ out_alpha, float* __restrict__ out_pos)
{
    if (hdr[0]) return;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= kept) return;
    const int i = src[j];
    if ((unsigned)i >= (unsigned)n) return;
    const int id = seat.base + j;
    const int after = id + s[i];
    int2* row = reinterpret_cast<int2*>(out_nodes + (size_t)id * 6);
    row[0] = make_int2(ndep[i], npar[i]);
    row[1] = make_int2(cc[i], id + 1);
    row[2] = make_int2(after == end[i] ? 0 : after, nd(nodes, i, ND_COUNT) == 0 ? lbase[i] : -1);
    out_alpha[id] = alpha[i] * w[i];
    if (j == 0) {
        out_pos[(size_t)id * 3 + 0] = center[0];
        out_pos[(size_t)id * 3 + 1] = center[1];
        out_pos[(size_t)id * 3 + 2] = center[2];
    }
}

// Row 0 (decision A-40): opacity-weighted centre of the chunk roots and the mean of their SH rows, both summed in
// chunk order in float64 and rounded once; the largest root opacity; a scale no cut selects.
__global__ void __launch_bounds__(256) k_scene_root(int K, int shf, int G, const int* __restrict__ roots,
                                                    const float* __restrict__ centers, float log_scale, float* pos,
                                                    float* shs, float* alpha, float* log_scales, float* rot, int* nodes)
{
    const int t = threadIdx.x;
    auto row = [&](int k) { const int r = roots[k]; return (r > 0 && r < G) ? r : 0; };
    if (t < 3) {
        double num = 0.0, den = 0.0;
        for (int k = 0; k < K; k++) {
            const double a = (double)alpha[row(k)];
            num = num + a * (double)centers[3 * (size_t)k + t];
            den = den + a;
        }
        pos[t] = (float)(num / (den > 1e-12 ? den : 1e-12));
        log_scales[t] = log_scale;
    }
    if (t < 4) rot[t] = t == 0 ? 1.0f : 0.0f;
    if (t == 4) {
        float a = alpha[row(0)];
        for (int k = 1; k < K; k++) a = fmaxf(a, alpha[row(k)]);
        alpha[0] = a;
    }
    if (t == 5) {
        nodes[0] = 0;
        nodes[1] = -1;
        nodes[2] = K;
        nodes[3] = 1;
        nodes[4] = 0;
        nodes[5] = -1;
    }
    for (int e = t; e < shf; e += 256) {
        double acc = 0.0;
        for (int k = 0; k < K; k++) acc = acc + (double)shs[(size_t)row(k) * shf + e];
        shs[e] = (float)(acc / (double)K);
    }
}

inline unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

size_t merge_scratch_bytes(int n)
{
    const size_t N = (size_t)(n > 0 ? n : 0);
    return ints(HLGS_MERGE_HEADER_INTS + kLv) + ints(kLv + 1) + ints(kLv) + 12 * ints(N);
}

void launch_merge_plan(const MergeIn& in, int k, int K, const float* centers, float falloff, void* scratch,
                       int stages, hipStream_t s)
{
    const Scratch sc = carve(scratch, in.n);
    const unsigned g = blocks(in.n);
    if (stages & 1) {
        // header, level counts, level starts, cursors and the claims, which lie together
        const size_t zero = (size_t)(reinterpret_cast<char*>(sc.claim) - static_cast<char*>(scratch)) + ints(in.n);
        hipMemsetAsync(scratch, 0, zero, s);
        hipLaunchKernelGGL(k_validate, dim3(g), dim3(256), 0, s, in.n, in.nodes, sc.claim, sc.hdr);
    }
    if (stages & 2)
        hipLaunchKernelGGL(k_weights, dim3(blocks((in.n + kWeightRounds - 1) / kWeightRounds)), dim3(256), 0, s,
                           in.n, k, K, centers, in.pos, in.nodes, sc.claim,
                           falloff, sc.w, sc.hdr, sc.lcount);
}

void launch_merge_emit(const MergeIn& in, const HierOut& out, int k, const float* centers, const int* level_counts,
                       int kept, int out_offset, int leaf_offset, int last, void* scratch, int stages, hipStream_t s)
{
    const Scratch sc = carve(scratch, in.n);
    int lo = kLv, hi = -1;
    for (int d = 0; d < kLv; d++)
        if (level_counts[d] > 0) {
            lo = d < lo ? d : lo;
            hi = d;
        }
    const RootSeat seat = {out_offset, leaf_offset, last ? out_offset + kept : -1};
    if (stages & 1) {
        hipLaunchKernelGGL(k_level_scan, dim3(1), dim3(1024), 0, s, sc.hdr, sc.lcount, sc.lstart, sc.cursor);
        hipLaunchKernelGGL(k_bucket, dim3(blocks(in.n)), dim3(256), 0, s, in.n, sc.hdr, in.nodes, sc.cursor, sc.order);
        for (int d = hi; d >= lo; d--)
            if (level_counts[d] > 0)
                hipLaunchKernelGGL(k_up, dim3(blocks(level_counts[d])), dim3(256), 0, s, d, sc.hdr, sc.lstart,
                                   sc.order, in.nodes, sc.w, sc.s, sc.l, sc.cc);
    }
    if (stages & 2)
        for (int d = lo; d <= hi; d++)
            if (level_counts[d] > 0)
                hipLaunchKernelGGL(k_down, dim3(blocks(level_counts[d])), dim3(256), 0, s, d, in.n, seat, sc.hdr,
                                   sc.lstart, sc.order, in.nodes, sc.w, sc.s, sc.l, sc.base, sc.lbase, sc.npar,
                                   sc.ndep, sc.end, sc.src);
    if (stages & 4) {
        MergeTabs tabs;
        const float* srcs[4] = {in.pos, in.shs, in.log_scales, in.rot};
        float* dsts[4] = {out.pos, out.shs, out.log_scales, out.rot};
        const int words[4] = {3, in.shf, 3, 4};
        for (int t = 0; t < 4; t++) {
            tabs.src[t] = reinterpret_cast<const uint32_t*>(srcs[t]);
            tabs.dst[t] = reinterpret_cast<uint32_t*>(dsts[t]);
            tabs.words[t] = words[t];
        }
        const int64_t chunks = ((int64_t)kept * in.shf + 3) / 4 + 1;
        const unsigned gx = (unsigned)std::min<int64_t>((chunks + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(k_merge_rows, dim3(gx, 4), dim3(256), 0, s, tabs, in.n, kept, out_offset, sc.hdr, sc.src);
        hipLaunchKernelGGL(k_finish, dim3(blocks(kept)), dim3(256), 0, s, in.n, kept, seat, sc.hdr, sc.src, in.nodes,
                           in.alpha, sc.w, sc.s, sc.cc, sc.lbase, sc.npar, sc.ndep, sc.end, centers + 3 * (size_t)k,
                           out.nodes, out.alpha, out.pos);
    }
}

void launch_merge_root(int K, int shf, int G, const int* roots, const float* centers, float log_scale,
                       const HierOut& out, hipStream_t s)
{
    hipLaunchKernelGGL(k_scene_root, dim3(1), dim3(256), 0, s, K, shf, G, roots, centers, log_scale, out.pos, out.shs,
                       out.alpha, out.log_scales, out.rot, out.nodes);
}

}  // namespace hlgs
