// hier_build.hip -- the dynamic hierarchy of N activated Gaussians, on the device: what the reference's offline
// GaussianHierarchyCreator does between its loader and its writer (submodules/gaussianhierarchy/
// mainHierarchyCreator.cpp:87-183): filter, PointbasedKdTreeGenerator, ClusterMerger, RotationAligner,
// Writer::makeDynamicHierarchy.  The contract is restated in include/hlgs.h (hlgs_hier_build) and DESIGN.md f6.
//
// The tree's shape is a function of N alone: a node of num leaves splits into num / 2 and num - num / 2, the layout
// is pre-order, so with n_left = num / 2 a node id has its left child at id + 1 and its right child at id + 2 n_left,
// and all nodes of one depth hold floor(N / 2^d) or ceil(N / 2^d) leaves.  Every kernel finds the node it works on by
// walking down from the root (node_at / seg_of, O(log N) integer steps); the host plans all launches from N and
// reads nothing back.  Only the leaf permutation depends on the data.
//
// Stages, each a sequence of launches on the caller's stream (no waiting between workgroups, no float atomics):
//   kd, top levels   three index lists, each sorted once by (coordinate key, row) with knn.hip's stable radix passes.
//                    Per level: per-segment bounds (partial min / max, then one thread per segment picks the axis),
//                    a left / right flag per row from the segment's list of that axis, and a stable partition of
//                    the three lists by it (scan.hip), which keeps each list sorted by (key, row) inside the halves.
//   kd, in LDS       once a segment holds at most kHierCap rows one workgroup finishes its subtree: keys, radius and
//                    row index live in LDS (40 KiB: four workgroups per CU of 160 KiB, 16 of its 32 wave slots), a
//                    level ranks every row inside its segment by counting the smaller (key, row) pairs -- a full sort
//                    of the segment, which is a valid nth_element -- and permutes the rows in place.
//   leaves, table    leaf rows (normalised rotation, covariance as computeCovariance), SH rows, the node table.
//   merge            bottom-up, one launch per depth; the subtrees of at most kHierCap leaves in one launch, a
//                    workgroup each, with a barrier per level.  Moments in float32 as written (this file is built with
//                    -ffp-contract=off), the 3 x 3 eigen-decomposition by cyclic Jacobi in float64 inside the thread.
//   align            top-down, one launch per depth, the small subtrees fused the same way.
//   finish           scales -> log(scales).
// Every result is a function of the inputs alone (no atomics on data, no order-dependent reductions): two runs agree
// bit for bit.  Memory safety for any input bits: row indices come only from permutations of 0..N-1 (the rank of a
// level is taken over a strict total order of (key bits, row), so it is a permutation even for NaN coordinates), and
// every gathered index is clamped.
#include <float.h>
#include <math.h>

#include "hlgs_internal.h"

namespace hlgs {

namespace {

constexpr int kT = 256;             // threads of every workgroup here
constexpr int kPer = kHierCap / kT;  // rows per thread of the in-LDS kd kernel
constexpr int kBumpMax = 16;        // bound of the merger's diagonal-bump loop
constexpr int kMaxChunks = 64;      // partial bounds per segment
static_assert(kHierCap % kT == 0 && kHierCap >= 2, "rows per thread");

struct HierBufs {
    uint32_t* status;
    uint32_t *leafperm, *leafid;   // N: row of the p-th leaf from the left; its node id
    float* cov;                    // (2N - 1) x 6: the accumulated covariance of every node
    float2* aw;                    // 2N - 1: the merge weights (a0, a1) of interior nodes
    uint32_t* list[3][2];          // N each: per axis, rows by (key, row) inside every segment; ping-pong
    uint32_t *keys, *keys_tmp;     // N
    uint32_t *left, *incl;         // N
    uint32_t *hist, *scan_tmp;
    float* parts;                  // segments x chunks x 8
    int* axis;                     // segments
};

template <typename T>
T* take_hb(char*& p, size_t n)
{
    T* r = reinterpret_cast<T*>(p);
    p += align_up(n * sizeof(T));
    return r;
}

// depth below which no segment exceeds kHierCap rows, and the number of segments there
inline int top_depth(uint32_t N)
{
    int d = 0;
    for (uint32_t c = N; c > (uint32_t)kHierCap; c -= c / 2) d++;
    return d;
}

HierBufs carve_hb(void* base, size_t N, size_t* total)
{
    char* p = static_cast<char*>(base);
    HierBufs b = {};
    const size_t G = 2 * N - 1;
    b.status = take_hb<uint32_t>(p, 4);
    b.leafperm = take_hb<uint32_t>(p, N);
    b.leafid = take_hb<uint32_t>(p, N);
    b.cov = take_hb<float>(p, 6 * G);
    b.aw = take_hb<float2>(p, G);
    const int dS = top_depth((uint32_t)N);
    if (dS > 0) {
        for (int a = 0; a < 3; a++)
            for (int h = 0; h < 2; h++) b.list[a][h] = take_hb<uint32_t>(p, N);
        b.keys = take_hb<uint32_t>(p, N);
        b.keys_tmp = take_hb<uint32_t>(p, N);
        b.left = take_hb<uint32_t>(p, N);
        b.incl = take_hb<uint32_t>(p, N);
        const size_t nh = radix_hist_elems(N);
        b.hist = take_hb<uint32_t>(p, nh);
        b.scan_tmp = take_hb<uint32_t>(p, scan_scratch_elems(nh > N ? nh : N));
        const size_t segs = (size_t)1 << (dS - 1);
        b.parts = take_hb<float>(p, (segs > 1024 ? segs : 1024) * 8);  // bound_chunks(segs) * segs boxes
        b.axis = take_hb<int>(p, segs);
    }
    if (total) *total = (size_t)(p - static_cast<char*>(base));
    return b;
}

// ---------------------------------------------------------------- the tree in closed form
struct Node {
    uint32_t id, lo, num;  // pre-order id, first leaf (from the left), leaves
};

// node k (from the left) of depth d below a root of n leaves, ids and leaves relative to that root.  Needs every
// ancestor to be interior, which holds for d <= ceil(log2 n) - 1.
__host__ __device__ inline Node node_at(uint32_t n, int d, uint32_t k)
{
    Node v = {0u, 0u, n};
    for (int b = d - 1; b >= 0; b--) {
        const uint32_t nl = v.num >> 1;
        if ((k >> b) & 1u) {
            v.id += 2u * nl;
            v.lo += nl;
            v.num -= nl;
        } else {
            v.id += 1u;
            v.num = nl;
        }
    }
    return v;
}

// the depth-d segment holding leaf position i below a root of n leaves; k: its index from the left
__device__ inline Node seg_of(uint32_t n, int d, uint32_t i, uint32_t& k)
{
    Node v = {0u, 0u, n};
    k = 0;
    for (int t = 0; t < d; t++) {
        const uint32_t nl = v.num >> 1;
        if (i < v.lo + nl) {
            v.id += 1u;
            v.num = nl;
            k = 2u * k;
        } else {
            v.id += 2u * nl;
            v.lo += nl;
            v.num -= nl;
            k = 2u * k + 1u;
        }
    }
    return v;
}

__host__ __device__ inline int ceil_log2(uint32_t n)
{
    int d = 0;
    for (uint32_t c = n; c > 1u; c -= c / 2) d++;
    return d;
}

// ---------------------------------------------------------------- keys and bounds
// position[axis] as an unsigned key of the same order; -0.0 and +0.0 share one key (the reference compares floats)
__device__ __forceinline__ uint32_t fkey(float v)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(uint32_t k)
{
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct Box6 {
    float lo[3], hi[3];
};
__device__ __forceinline__ void box_init(Box6& b)
{
#pragma unroll
    for (int a = 0; a < 3; a++) b.lo[a] = FLT_MAX, b.hi[a] = -FLT_MAX;
}
// PointbasedKdTreeGenerator.cpp:19-32: position -+ r, r = 3 max(scale), every operation rounded on its own
__device__ __forceinline__ void box_add(Box6& b, float x, float y, float z, float r)
{
    const float p[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; a++) {
        b.lo[a] = fminf(b.lo[a], p[a] - r);
        b.hi[a] = fmaxf(b.hi[a], p[a] + r);
    }
}
// :44-54: the first axis of the strictly greatest extent, starting from (axis 0, 0)
__device__ __forceinline__ int box_axis(const Box6& b)
{
    int axis = 0;
    float greatest = 0.f;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float dist = b.hi[a] - b.lo[a];
        if (dist > greatest) greatest = dist, axis = a;
    }
    return axis;
}
__device__ __forceinline__ float wmin(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wmax(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float radius3(const float* __restrict__ scales, size_t row)
{
    return 3.0f * fmaxf(fmaxf(scales[3 * row], scales[3 * row + 1]), scales[3 * row + 2]);
}

// ---------------------------------------------------------------- validity
// strict == 0: the creator's filter (mainHierarchyCreator.cpp:87-152), mask[i] = kept.  strict == 1: what a build
// refuses (a non-finite value anywhere, or opacity 0).  A failing row sets bit 0 of *status when status is given.
__global__ void __launch_bounds__(kT) k_hb_valid(uint32_t N, int shf, const float* __restrict__ xyz,
                                                 const float* __restrict__ shs, const float* __restrict__ opacity,
                                                 const float* __restrict__ scales, const float* __restrict__ rot,
                                                 int strict, uint8_t* __restrict__ mask, uint32_t* __restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    const float o = opacity[i];
    bool nan = false, inf = false, big = false;
    for (int c = 0; c < 3; c++) {
        const float s = scales[3 * i + c], p = xyz[3 * i + c];
        nan |= isnan(s) | isnan(p);
        inf |= isinf(s) | isinf(p);
        big |= s > 10.f;
    }
    for (int c = 0; c < 4; c++) {
        nan |= isnan(rot[4 * i + c]);
        inf |= isinf(rot[4 * i + c]);
    }
    for (int c = 0; c < shf; c++) {
        const float v = shs[i * (size_t)shf + c];
        nan |= isnan(v);
        inf |= isinf(v);
    }
    bool ok = !(isinf(o) || isnan(o) || o == 0.f || nan);
    ok = strict ? (ok && !inf) : (ok && !big);
    if (mask) mask[i] = ok ? 1 : 0;
    if (status && !ok) atomicOr(status, HLGS_HIER_STATUS_INVALID);  // an integer flag: the order cannot show
}

// ---------------------------------------------------------------- kd, top levels
__global__ void __launch_bounds__(kT) k_hb_keys(uint32_t N, int axis, const float* __restrict__ xyz,
                                                uint32_t* __restrict__ keys, uint32_t* __restrict__ vals)
{
    const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
    if (i >= N) return;
    keys[i] = fkey(xyz[3 * i + axis]);
    vals[i] = (uint32_t)i;
}

// partial boxes per segment: segments x chunks <= max(1024, segments)
inline int bound_chunks(uint32_t segs)
{
    const int c = (int)(1024u / segs);
    return c < 1 ? 1 : c > kMaxChunks ? kMaxChunks : c;
}

// one workgroup per (segment, chunk): min / max of one chunk of one depth-d segment, read through list 0
__global__ void __launch_bounds__(kT) k_hb_bounds(uint32_t N, int d, uint32_t chunks, const uint32_t* __restrict__ list,
                                                  const float* __restrict__ xyz, const float* __restrict__ scales,
                                                  float* __restrict__ parts)
{
    __shared__ float red[kT / 64][6];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const Node v = node_at(N, d, blockIdx.x / chunks);
    const uint32_t chunk = (v.num + chunks - 1) / chunks;
    const uint32_t begin = min(v.num, (blockIdx.x % chunks) * chunk), end = min(v.num, begin + chunk);
    Box6 b;
    box_init(b);
    for (uint32_t j = begin + tid; j < end; j += kT) {
        const size_t row = min(list[v.lo + j], N - 1u);
        box_add(b, xyz[3 * row], xyz[3 * row + 1], xyz[3 * row + 2], radius3(scales, row));
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        b.lo[a] = wmin(b.lo[a]);
        b.hi[a] = wmax(b.hi[a]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) red[wid][a] = b.lo[a], red[wid][3 + a] = b.hi[a];
    }
    __syncthreads();
    if (tid < 6) {
        float r = red[0][tid];
        for (int w = 1; w < kT / 64; w++) r = tid < 3 ? fminf(r, red[w][tid]) : fmaxf(r, red[w][tid]);
        parts[(size_t)blockIdx.x * 8 + tid] = r;
    }
}

// one thread per segment: the segment's box from its partial boxes (min / max: the order cannot show), its axis
__global__ void __launch_bounds__(kT) k_hb_axis(uint32_t segs, int chunks, const float* __restrict__ parts,
                                                int* __restrict__ axis)
{
    const uint32_t k = blockIdx.x * kT + threadIdx.x;
    if (k >= segs) return;
    Box6 b;
    box_init(b);
    for (int c = 0; c < chunks; c++) {
        const float* p = parts + ((size_t)k * chunks + c) * 8;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            b.lo[a] = fminf(b.lo[a], p[a]);
            b.hi[a] = fmaxf(b.hi[a], p[3 + a]);
        }
    }
    axis[k] = box_axis(b);
}

// one thread per list position: the row there in the list of its segment's axis goes left iff it is among the first
// num / 2 of the segment (PointbasedKdTreeGenerator.cpp:56-63 with ties ordered by row)
__global__ void __launch_bounds__(kT) k_hb_flag(uint32_t N, int d, const int* __restrict__ axis,
                                                const uint32_t* __restrict__ l0, const uint32_t* __restrict__ l1,
                                                const uint32_t* __restrict__ l2, uint32_t* __restrict__ left)
{
    const size_t j = (size_t)blockIdx.x * kT + threadIdx.x;
    if (j >= N) return;
    uint32_t k;
    const Node v = seg_of(N, d, (uint32_t)j, k);
    const int a = axis[k];
    const uint32_t row = min((a == 0 ? l0 : a == 1 ? l1 : l2)[j], N - 1u);
    left[row] = ((uint32_t)j - v.lo) < (v.num >> 1) ? 1u : 0u;
}

__global__ void __launch_bounds__(kT) k_hb_gather(uint32_t N, const uint32_t* __restrict__ list,
                                                  const uint32_t* __restrict__ left, uint32_t* __restrict__ f)
{
    const size_t j = (size_t)blockIdx.x * kT + threadIdx.x;
    if (j < N) f[j] = left[min(list[j], N - 1u)];
}

// stable partition of every depth-d segment of one list by the flags whose inclusive scan is incl
__global__ void __launch_bounds__(kT) k_hb_partition(uint32_t N, int d, const uint32_t* __restrict__ in,
                                                     const uint32_t* __restrict__ incl, uint32_t* __restrict__ out)
{
    const size_t j = (size_t)blockIdx.x * kT + threadIdx.x;
    if (j >= N) return;
    uint32_t k;
    const Node v = seg_of(N, d, (uint32_t)j, k);
    const uint32_t base = v.lo ? incl[v.lo - 1] : 0u;
    const uint32_t f = incl[j] - (j ? incl[j - 1] : 0u);
    const uint32_t before = incl[j] - f - base;  // rows of the segment going left ahead of j
    const uint32_t dst = f ? v.lo + before : v.lo + (v.num >> 1) + ((uint32_t)j - v.lo - before);
    if (dst < N) out[dst] = in[j];  // inside the segment by the counts; the test keeps a broken invariant in range
}

// ---------------------------------------------------------------- kd, in LDS
// One workgroup per depth-dS segment (at most kHierCap rows): all remaining levels.  list == nullptr: rows in order.
__global__ void __launch_bounds__(kT) k_hb_kd_lds(uint32_t N, int dS, const uint32_t* __restrict__ list,
                                                  const float* __restrict__ xyz, const float* __restrict__ scales,
                                                  uint32_t* __restrict__ leafperm)
{
    __shared__ uint32_t key[3][kHierCap];
    __shared__ float rad[kHierCap];
    __shared__ uint32_t idx[kHierCap];
    __shared__ uint8_t s_axis[kHierCap / 2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const Node root = node_at(N, dS, blockIdx.x);
    const uint32_t n = min(root.num, (uint32_t)kHierCap);  // root.num <= kHierCap by the choice of dS
    for (uint32_t j = tid; j < n; j += kT) {
        const uint32_t row = list ? min(list[root.lo + j], N - 1u) : root.lo + j;
        idx[j] = row;
        key[0][j] = fkey(xyz[3 * (size_t)row]);
        key[1][j] = fkey(xyz[3 * (size_t)row + 1]);
        key[2][j] = fkey(xyz[3 * (size_t)row + 2]);
        rad[j] = radius3(scales, row);
    }
    __syncthreads();
    const int levels = ceil_log2(n);
    for (int ld = 0; ld < levels; ld++) {
        const uint32_t segs = 1u << ld;
        // bounds and axis of every segment: a wave per segment while they are long, then a thread per segment
        if ((n >> ld) >= 64u) {
            for (uint32_t k = wid; k < segs; k += kT / 64) {
                const Node v = node_at(n, ld, k);
                Box6 b;
                box_init(b);
                for (uint32_t j = v.lo + lane; j < v.lo + v.num; j += 64)
                    box_add(b, fkey_inv(key[0][j]), fkey_inv(key[1][j]), fkey_inv(key[2][j]), rad[j]);
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    b.lo[a] = wmin(b.lo[a]);
                    b.hi[a] = wmax(b.hi[a]);
                }
                if (lane == 0) s_axis[k] = (uint8_t)box_axis(b);
            }
        } else {
            for (uint32_t k = tid; k < segs; k += kT) {
                const Node v = node_at(n, ld, k);
                Box6 b;
                box_init(b);
                for (uint32_t j = v.lo; j < v.lo + v.num; j++)
                    box_add(b, fkey_inv(key[0][j]), fkey_inv(key[1][j]), fkey_inv(key[2][j]), rad[j]);
                s_axis[k] = (uint8_t)box_axis(b);
            }
        }
        __syncthreads();
        // rank of every row inside its segment under (key of the axis, row): a strict total order, so a permutation
        uint32_t dst[kPer], kx[kPer], ky[kPer], kz[kPer], ri[kPer];
        float rr[kPer];
#pragma unroll
        for (int e = 0; e < kPer; e++) {
            const uint32_t j = tid + e * kT;
            dst[e] = j;
            if (j >= n) continue;
            uint32_t k;
            const Node v = seg_of(n, ld, j, k);
            kx[e] = key[0][j], ky[e] = key[1][j], kz[e] = key[2][j], rr[e] = rad[j], ri[e] = idx[j];
            if (v.num < 2u) continue;
            const int a = s_axis[k] < 3 ? s_axis[k] : 0;
            const uint32_t* ka = key[a];
            const uint32_t mk = ka[j], mi = ri[e];
            uint32_t cnt = 0;
            for (uint32_t m = v.lo; m < v.lo + v.num; m++) {
                const uint32_t ok = ka[m], oi = idx[m];
                cnt += (ok < mk || (ok == mk && oi < mi)) ? 1u : 0u;
            }
            dst[e] = v.lo + cnt;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < kPer; e++) {
            const uint32_t j = tid + e * kT;
            if (j >= n || dst[e] >= n) continue;
            key[0][dst[e]] = kx[e], key[1][dst[e]] = ky[e], key[2][dst[e]] = kz[e];
            rad[dst[e]] = rr[e];
            idx[dst[e]] = ri[e];
        }
        __syncthreads();
    }
    for (uint32_t j = tid; j < n; j += kT) leafperm[root.lo + j] = idx[j];
}

// ---------------------------------------------------------------- small matrices
struct M3 {
    float m[3][3];
};

// common.h:103-117 (rot = (s, x, y, z))
__device__ __forceinline__ M3 matrix_from_quat(const float q[4])
{
    const float s = q[0], x = q[1], y = q[2], z = q[3];
    M3 R;
    R.m[0][0] = 1.f - 2.f * (y * y + z * z), R.m[0][1] = 2.f * (x * y - s * z), R.m[0][2] = 2.f * (x * z + s * y);
    R.m[1][0] = 2.f * (x * y + s * z), R.m[1][1] = 1.f - 2.f * (x * x + z * z), R.m[1][2] = 2.f * (y * z - s * x);
    R.m[2][0] = 2.f * (x * z - s * y), R.m[2][1] = 2.f * (y * z + s * x), R.m[2][2] = 1.f - 2.f * (x * x + y * y);
    return R;
}

// Eigen::Quaternionf(Matrix3f) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>), as
// (w, x, y, z)
__device__ __forceinline__ void quat_from_matrix(const M3& R, float q[4])
{
    float t = (R.m[0][0] + R.m[1][1]) + R.m[2][2];
    if (t > 0.f) {
        t = sqrtf(t + 1.0f);
        q[0] = 0.5f * t;
        t = 0.5f / t;
        q[1] = (R.m[2][1] - R.m[1][2]) * t;
        q[2] = (R.m[0][2] - R.m[2][0]) * t;
        q[3] = (R.m[1][0] - R.m[0][1]) * t;
    } else {
        int i = 0;
        if (R.m[1][1] > R.m[0][0]) i = 1;
        if (R.m[2][2] > R.m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrtf(((R.m[i][i] - R.m[j][j]) - R.m[k][k]) + 1.0f);
        q[1 + i] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (R.m[k][j] - R.m[j][k]) * t;
        q[1 + j] = (R.m[j][i] + R.m[i][j]) * t;
        q[1 + k] = (R.m[k][i] + R.m[i][k]) * t;
    }
}

// det of the columns c0, c1, c2 of R as c0.cross(c1).dot(c2)
__device__ __forceinline__ float col_det(const M3& R)
{
    const float cx = R.m[1][0] * R.m[2][1] - R.m[2][0] * R.m[1][1];
    const float cy = R.m[2][0] * R.m[0][1] - R.m[0][0] * R.m[2][1];
    const float cz = R.m[0][0] * R.m[1][1] - R.m[1][0] * R.m[0][1];
    return (cx * R.m[0][2] + cy * R.m[1][2]) + cz * R.m[2][2];
}

// common.h:119-146: T = R diag(scale), cov = T T^T, sums left to right
__device__ __forceinline__ void covariance_of(const float s[3], const float q[4], float cov[6])
{
    const M3 R = matrix_from_quat(q);
    float T[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[i][j] = R.m[i][j] * s[j];
    int o = 0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = i; j < 3; j++) cov[o++] = (T[i][0] * T[j][0] + T[i][1] * T[j][1]) + T[i][2] * T[j][2];
}

__device__ __forceinline__ float surface(const float s[3]) { return (s[0] * s[1] + s[0] * s[2]) + s[1] * s[2]; }

// eigenvalues ascending and eigenvectors (columns of V) of the symmetric matrix with the six entries c, by cyclic
// Jacobi in float64.  At most 24 sweeps; a NaN input leaves NaN eigenvalues.
__device__ void eigh3(const float c[6], double ev[3], double V[3][3])
{
    double A[3][3] = {{c[0], c[1], c[2]}, {c[1], c[3], c[4]}, {c[2], c[4], c[5]}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; sweep++) {
        const double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        const double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off == 0.0 || off <= 1e-18 * diag) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                const int r = 3 - p - q;
                const double arp = A[r][p], arq = A[r][q];
                A[p][p] -= t * apq;
                A[q][q] += t * apq;
                A[p][q] = A[q][p] = 0.0;
                A[r][p] = A[p][r] = cs * arp - sn * arq;
                A[r][q] = A[q][r] = sn * arp + cs * arq;
                for (int i = 0; i < 3; i++) {
                    const double vip = V[i][p], viq = V[i][q];
                    V[i][p] = cs * vip - sn * viq;
                    V[i][q] = sn * vip + cs * viq;
                }
            }
    }
    ev[0] = A[0][0], ev[1] = A[1][1], ev[2] = A[2][2];
    // ascending, by three compare-and-swaps of (value, column)
    const int order[3][2] = {{0, 1}, {1, 2}, {0, 1}};
    for (int s = 0; s < 3; s++) {
        const int a = order[s][0], b = order[s][1];
        if (ev[b] < ev[a]) {
            const double t = ev[a];
            ev[a] = ev[b], ev[b] = t;
            for (int i = 0; i < 3; i++) {
                const double u = V[i][a];
                V[i][a] = V[i][b], V[i][b] = u;
            }
        }
    }
}

// ---------------------------------------------------------------- leaves and the node table
struct Rows {
    float *pos, *shs, *alpha, *scale, *rot;  // 2N - 1 rows; scale holds activated scales until k_hb_finish
    float* cov;
    float2* aw;
    int shf;
};

// one thread per leaf position
__global__ void __launch_bounds__(kT) k_hb_leaves(uint32_t N, const uint32_t* __restrict__ leafperm,
                                                  const float* __restrict__ xyz, const float* __restrict__ opacity,
                                                  const float* __restrict__ scales, const float* __restrict__ rot,
                                                  Rows o, uint32_t* __restrict__ leafid)
{
    const size_t p = (size_t)blockIdx.x * kT + threadIdx.x;
    if (p >= N) return;
    const size_t row = min(leafperm[p], N - 1u);
    Node v = {0u, 0u, N};
    while (v.num > 1u) {
        const uint32_t nl = v.num >> 1;
        if (p < v.lo + nl) {
            v.id += 1u;
            v.num = nl;
        } else {
            v.id += 2u * nl;
            v.lo += nl;
            v.num -= nl;
        }
    }
    const size_t id = v.id;
    leafid[p] = v.id;
    float s[3], q[4], cov[6];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        o.pos[3 * id + c] = xyz[3 * row + c];
        s[c] = scales[3 * row + c];
        o.scale[3 * id + c] = s[c];
    }
    o.alpha[id] = opacity[row];
#pragma unroll
    for (int c = 0; c < 4; c++) q[c] = rot[4 * row + c];
    const float nrm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);  // loader.cpp:56
#pragma unroll
    for (int c = 0; c < 4; c++) {
        q[c] = q[c] / nrm;
        o.rot[4 * id + c] = q[c];
    }
    covariance_of(s, q, cov);
#pragma unroll
    for (int c = 0; c < 6; c++) o.cov[6 * id + c] = cov[c];
}

// one thread per SH value of a leaf
__global__ void __launch_bounds__(kT) k_hb_leaf_sh(uint32_t N, int shf, const uint32_t* __restrict__ leafperm,
                                                   const uint32_t* __restrict__ leafid,
                                                   const float* __restrict__ shs, float* __restrict__ out)
{
    const size_t t = (size_t)blockIdx.x * kT + threadIdx.x;
    if (t >= (size_t)N * shf) return;
    const size_t p = t / shf, c = t % shf;
    const size_t row = min(leafperm[p], N - 1u), id = min(leafid[p], 2u * N - 2u);
    out[id * shf + c] = shs[row * shf + c];
}

// one thread per node: writer.cpp:99-171 in closed form
__global__ void __launch_bounds__(kT) k_hb_nodes(uint32_t N, const uint32_t* __restrict__ leafperm,
                                                 int* __restrict__ nodes)
{
    const size_t id = (size_t)blockIdx.x * kT + threadIdx.x;
    if (id >= 2 * (size_t)N - 1) return;
    Node v = {0u, 0u, N};
    int depth = 0, parent = -1, sibling = 0;
    while (v.id != (uint32_t)id && v.num > 1u) {
        const uint32_t nl = v.num >> 1;
        parent = (int)v.id;
        if ((uint32_t)id < v.id + 2u * nl) {
            sibling = (int)(v.id + 2u * nl);
            v.id += 1u;
            v.num = nl;
        } else {
            sibling = 0;
            v.id += 2u * nl;
            v.lo += nl;
            v.num -= nl;
        }
        depth++;
    }
    int* n = nodes + 6 * id;
    n[0] = depth;
    n[1] = parent;
    n[2] = v.num > 1u ? 2 : 0;
    n[3] = (int)id + 1;
    n[4] = sibling;
    n[5] = v.num > 1u ? -1 : (int)min(leafperm[v.lo], N - 1u);
}

// ---------------------------------------------------------------- merge
// ClusterMerger.cpp:50-141 for the node id with children c0 = id + 1, c1 = id + 2 nl; without the SH row
__device__ void merge_node(const Rows& o, size_t id, uint32_t nl, uint32_t* __restrict__ status)
{
    const size_t ch[2] = {id + 1, id + 2 * (size_t)nl};
    float w[2], p[2][3];
    for (int i = 0; i < 2; i++) {
        const float s[3] = {o.scale[3 * ch[i]], o.scale[3 * ch[i] + 1], o.scale[3 * ch[i] + 2]};
        w[i] = o.alpha[ch[i]] * surface(s);
        for (int c = 0; c < 3; c++) p[i][c] = o.pos[3 * ch[i] + c];
    }
    const float W = (0.f + w[0]) + w[1];
    const float a[2] = {w[0] / W, w[1] / W};
    float pos[3], cov[6];
    for (int c = 0; c < 3; c++) pos[c] = (0.f + a[0] * p[0][c]) + a[1] * p[1][c];
    float term[2][6];
    for (int i = 0; i < 2; i++) {
        const float dx = p[i][0] - pos[0], dy = p[i][1] - pos[1], dz = p[i][2] - pos[2];
        const float* cc = o.cov + 6 * ch[i];
        term[i][0] = a[i] * (cc[0] + dx * dx);
        term[i][1] = a[i] * (cc[1] + dy * dx);
        term[i][2] = a[i] * (cc[2] + dz * dx);
        term[i][3] = a[i] * (cc[3] + dy * dy);
        term[i][4] = a[i] * (cc[4] + dz * dy);
        term[i][5] = a[i] * (cc[5] + dz * dz);
    }
    for (int c = 0; c < 6; c++) cov[c] = (0.f + term[0][c]) + term[1][c];

    float m[6] = {cov[0], cov[1], cov[2], cov[3], cov[4], cov[5]};
    double evd[3], V[3][3];
    float ev[3];
    eigh3(m, evd, V);
    for (int c = 0; c < 3; c++) ev[c] = (float)evd[c];
    uint32_t st = 0;
    if (isnan(ev[0]) || isnan(ev[1]) || isnan(ev[2])) st |= HLGS_HIER_STATUS_NAN;  // :97-101 throws
    int loops = 0;
    while (!st && (ev[0] == 0.f || ev[1] == 0.f || ev[2] == 0.f)) {  // :104-117
        if (loops++ == kBumpMax) {
            st |= HLGS_HIER_STATUS_BUMP;
            break;
        }
        m[0] += fmaxf(m[0] * 0.0001f, FLT_EPSILON);
        m[3] += fmaxf(m[3] * 0.0001f, FLT_EPSILON);
        m[5] += fmaxf(m[5] * 0.0001f, FLT_EPSILON);
        eigh3(m, evd, V);
        for (int c = 0; c < 3; c++) ev[c] = (float)evd[c];
    }
    if (st) atomicOr(status, st);
    M3 R;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R.m[i][j] = (float)V[i][j];
    if (col_det(R) < 0.f)  // :119-125
        for (int i = 0; i < 3; i++) R.m[i][2] = -R.m[i][2];
    const float s[3] = {sqrtf(fabsf(ev[0])), sqrtf(fabsf(ev[1])), sqrtf(fabsf(ev[2]))};
    float q[4];
    quat_from_matrix(R, q);
    for (int c = 0; c < 3; c++) o.pos[3 * id + c] = pos[c], o.scale[3 * id + c] = s[c];
    for (int c = 0; c < 4; c++) o.rot[4 * id + c] = q[c];
    for (int c = 0; c < 6; c++) o.cov[6 * id + c] = cov[c];
    o.alpha[id] = W / surface(s);  // may exceed 1: kept
    o.aw[id] = make_float2(a[0], a[1]);
}

__device__ __forceinline__ void merge_sh(const Rows& o, size_t id, uint32_t nl, int c)
{
    const float2 a = o.aw[id];
    const size_t shf = (size_t)o.shf;
    o.shs[id * shf + c] = (0.f + a.x * o.shs[(id + 1) * shf + c]) + a.y * o.shs[(id + 2 * (size_t)nl) * shf + c];
}

// the interior nodes of depth d, one thread each (d below the fused subtrees' roots)
__global__ void __launch_bounds__(64) k_hb_merge_level(uint32_t N, int d, Rows o, uint32_t* __restrict__ status)
{
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= (1u << d)) return;
    const Node v = node_at(N, d, k);
    if (v.num >= 2u) merge_node(o, v.id, v.num >> 1, status);
}
__global__ void __launch_bounds__(kT) k_hb_merge_sh_level(uint32_t N, int d, Rows o)
{
    const size_t t = (size_t)blockIdx.x * kT + threadIdx.x;
    if (t >= ((size_t)1 << d) * o.shf) return;
    const Node v = node_at(N, d, (uint32_t)(t / o.shf));
    if (v.num >= 2u) merge_sh(o, v.id, v.num >> 1, (int)(t % o.shf));
}

// one workgroup per depth-dS subtree, bottom-up with a barrier per level (a workgroup sees its own global writes
// after __syncthreads)
__global__ void __launch_bounds__(kT) k_hb_merge_sub(uint32_t N, int dS, Rows o, uint32_t* __restrict__ status)
{
    const Node root = node_at(N, dS, blockIdx.x);
    const int levels = ceil_log2(root.num);
    for (int ld = levels - 1; ld >= 0; ld--) {
        const uint32_t cnt = 1u << ld;
        for (uint32_t k = threadIdx.x; k < cnt; k += kT) {
            const Node v = node_at(root.num, ld, k);
            if (v.num >= 2u) merge_node(o, (size_t)root.id + v.id, v.num >> 1, status);
        }
        __syncthreads();
        for (size_t t = threadIdx.x; t < (size_t)cnt * o.shf; t += kT) {
            const Node v = node_at(root.num, ld, (uint32_t)(t / o.shf));
            if (v.num >= 2u) merge_sh(o, (size_t)root.id + v.id, v.num >> 1, (int)(t % o.shf));
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- align
// rotation_aligner.cpp:23-88: the child `ch` against its parent's rotation Rref
__device__ void align_child(const Rows& o, const M3& Rref, size_t ch)
{
    float q[4], s[3];
    for (int c = 0; c < 4; c++) q[c] = o.rot[4 * ch + c];
    for (int c = 0; c < 3; c++) s[c] = o.scale[3 * ch + c];
    const M3 Rm = matrix_from_quat(q);
    float best_score = 0.f;
    int bi = -1, bj = 0, bk = 0;
    M3 best = Rm;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            if (j == i) continue;
            const int k = 3 - i - j;
            for (int state = 0; state < 8; state++) {
                M3 test;
                const int src[3] = {i, j, k};
                for (int w = 0; w < 3; w++)
                    for (int r = 0; r < 3; r++) test.m[r][w] = (state & (1 << w)) ? -Rm.m[r][src[w]] : Rm.m[r][src[w]];
                if (col_det(test) < 0.f) continue;
                float score = 0.f;
                for (int r = 0; r < 3; r++)
                    for (int c = 0; c < 3; c++) score += test.m[r][c] * Rref.m[r][c];
                if (score > best_score) best_score = score, best = test, bi = i, bj = j, bk = k;
            }
        }
    if (bi < 0) return;  // no candidate scores above 0 (the reference reads uninitialised indices): unchanged
    quat_from_matrix(best, q);
    for (int c = 0; c < 4; c++) o.rot[4 * ch + c] = q[c];
    o.scale[3 * ch] = s[bi], o.scale[3 * ch + 1] = s[bj], o.scale[3 * ch + 2] = s[bk];
}

__device__ __forceinline__ void align_children(const Rows& o, size_t id, uint32_t nl)
{
    float q[4];
    for (int c = 0; c < 4; c++) q[c] = o.rot[4 * id + c];
    const M3 Rref = matrix_from_quat(q);
    align_child(o, Rref, id + 1);
    align_child(o, Rref, id + 2 * (size_t)nl);
}

__global__ void __launch_bounds__(64) k_hb_align_level(uint32_t N, int d, Rows o)
{
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= (1u << d)) return;
    const Node v = node_at(N, d, k);
    if (v.num >= 2u) align_children(o, v.id, v.num >> 1);
}

__global__ void __launch_bounds__(kT) k_hb_align_sub(uint32_t N, int dS, Rows o)
{
    const Node root = node_at(N, dS, blockIdx.x);
    const int levels = ceil_log2(root.num);
    for (int ld = 0; ld < levels; ld++) {
        for (uint32_t k = threadIdx.x; k < (1u << ld); k += kT) {
            const Node v = node_at(root.num, ld, k);
            if (v.num >= 2u) align_children(o, (size_t)root.id + v.id, v.num >> 1);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kT) k_hb_finish(size_t n, float* __restrict__ scale)
{
    const size_t i = (size_t)blockIdx.x * kT + threadIdx.x;
    if (i < n) scale[i] = logf(scale[i]);  // writer.cpp:119, 130
}

inline unsigned blocks_of(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

size_t hier_scratch_bytes(int N)
{
    size_t total = 0;
    carve_hb(nullptr, (size_t)(N > 0 ? N : 1), &total);
    return total;
}

void launch_hier_valid(const HierIn& in, int strict, uint8_t* mask, uint32_t* status, hipStream_t s)
{
    if (in.N <= 0) return;
    hipLaunchKernelGGL(k_hb_valid, dim3(blocks_of(in.N, kT)), dim3(kT), 0, s, (uint32_t)in.N, in.shf, in.xyz, in.shs,
                       in.opacity, in.scales, in.rotations, strict, mask, status);
}

void launch_hier_build(const HierIn& in, const HierOut& out, void* scratch, int stages, hipStream_t s)
{
    const uint32_t N = (uint32_t)in.N;
    const size_t G = 2 * (size_t)N - 1;
    const HierBufs b = carve_hb(scratch, N, nullptr);
    const int dS = top_depth(N);
    const unsigned nb = blocks_of(N, kT);
    const Rows rows = {out.pos, out.shs, out.alpha, out.log_scales, out.rot, b.cov, b.aw, in.shf};
    const uint32_t* top = nullptr;  // list 0 after the top levels

    if (stages & (1 << HB_KD_TOP)) {
        hipMemsetAsync(b.status, 0, 16, s);
        launch_hier_valid(in, 1, nullptr, b.status, s);
    }
    if (dS > 0) {
        int cur = 0;
        for (int d = 0; d < dS; d++) {
            if (!(stages & (1 << HB_KD_TOP))) {  // only where the lists end up
                cur ^= 1;
                continue;
            }
            if (d == 0)
                for (int a = 0; a < 3; a++) {
                    hipLaunchKernelGGL(k_hb_keys, dim3(nb), dim3(kT), 0, s, N, a, in.xyz, b.keys, b.list[a][0]);
                    radix_sort_pairs_u32(N, b.keys, b.list[a][0], b.keys_tmp, b.list[a][1], b.hist, b.scan_tmp, s);
                }
            const uint32_t segs = 1u << d;
            const int chunks = bound_chunks(segs);
            hipLaunchKernelGGL(k_hb_bounds, dim3(segs * chunks), dim3(kT), 0, s, N, d, (uint32_t)chunks,
                               b.list[0][cur], in.xyz, in.scales, b.parts);
            hipLaunchKernelGGL(k_hb_axis, dim3(blocks_of(segs, kT)), dim3(kT), 0, s, segs, chunks, b.parts, b.axis);
            hipLaunchKernelGGL(k_hb_flag, dim3(nb), dim3(kT), 0, s, N, d, b.axis, b.list[0][cur], b.list[1][cur],
                               b.list[2][cur], b.left);
            for (int a = 0; a < 3; a++) {
                hipLaunchKernelGGL(k_hb_gather, dim3(nb), dim3(kT), 0, s, N, b.list[a][cur], b.left, b.incl);
                scan_inclusive_u32(b.incl, b.incl, N, b.scan_tmp, s);
                hipLaunchKernelGGL(k_hb_partition, dim3(nb), dim3(kT), 0, s, N, d, b.list[a][cur], b.incl,
                                   b.list[a][cur ^ 1]);
            }
            cur ^= 1;
        }
        top = b.list[0][cur];
    }
    const unsigned subs = 1u << dS;
    if (stages & (1 << HB_KD_LDS))
        hipLaunchKernelGGL(k_hb_kd_lds, dim3(subs), dim3(kT), 0, s, N, dS, top, in.xyz, in.scales, b.leafperm);
    if (stages & (1 << HB_LEAVES)) {
        hipLaunchKernelGGL(k_hb_leaves, dim3(nb), dim3(kT), 0, s, N, b.leafperm, in.xyz, in.opacity, in.scales,
                           in.rotations, rows, b.leafid);
        hipLaunchKernelGGL(k_hb_leaf_sh, dim3(blocks_of((size_t)N * in.shf, kT)), dim3(kT), 0, s, N, in.shf,
                           b.leafperm, b.leafid, in.shs, out.shs);
        hipLaunchKernelGGL(k_hb_nodes, dim3(blocks_of(G, kT)), dim3(kT), 0, s, N, b.leafperm, out.nodes);
    }
    if (stages & (1 << HB_MERGE)) {
        hipLaunchKernelGGL(k_hb_merge_sub, dim3(subs), dim3(kT), 0, s, N, dS, rows, b.status);
        for (int d = dS - 1; d >= 0; d--) {
            hipLaunchKernelGGL(k_hb_merge_level, dim3(blocks_of((size_t)1 << d, 64)), dim3(64), 0, s, N, d, rows,
                               b.status);
            hipLaunchKernelGGL(k_hb_merge_sh_level, dim3(blocks_of(((size_t)1 << d) * in.shf, kT)), dim3(kT), 0, s, N,
                               d, rows);
        }
    }
    if (stages & (1 << HB_ALIGN)) {
        for (int d = 0; d < dS; d++)
            hipLaunchKernelGGL(k_hb_align_level, dim3(blocks_of((size_t)1 << d, 64)), dim3(64), 0, s, N, d, rows);
        hipLaunchKernelGGL(k_hb_align_sub, dim3(subs), dim3(kT), 0, s, N, dS, rows);
    }
    if (stages & (1 << HB_FINISH))
        hipLaunchKernelGGL(k_hb_finish, dim3(blocks_of(3 * G, kT)), dim3(kT), 0, s, 3 * G, out.log_scales);
}

}  // namespace hlgs
