// knn.hip -- mean squared distance to the three nearest other points (simple_knn.distCUDA2, as
// scene/gaussian_model.py:21, 848 uses it): the initial scale of every Gaussian made from an SfM point cloud.
//
// Contract: d(i, j) = (dx*dx + dy*dy) + dz*dz in float32, every operation rounded on its own (this file is built
// with -ffp-contract=off); the three smallest over all other indices j, b0 <= b1 <= b2; out[i] = ((b0 + b1) + b2) / 3.
// A missing neighbour (P < 4) counts as +inf.  The result depends only on the multiset of distances of each point,
// never on the order the candidates arrive in, so it is bitwise reproducible and equal to the all-pairs scan.
//
// Pipeline, all on the device, no host read-back:
//   1. bounding box: per-block min / max partials, reduced again by every block of the key kernel
//   2. 30-bit Morton key (10 bits per axis) per point
//   3. LSD radix sort of (key, index), four 8-bit passes: per-tile digit histograms (LDS integer atomics, whose
//      order cannot show), one scan over the digit-major (digit, tile) table (scan.hip), a one-wave scatter that
//      ranks equal digits by ballot, in lane order, so every pass is stable
//   4. sorted rows as float4 (x, y, z, index bits) and one AABB per box of kKnnBox = 64 consecutive rows;
//      one AABB per super-box of kKnnSuper = 64 consecutive boxes
//   5. search: one wave per box.  Each lane takes its 3-best from the wave's own box; the wave's reject radius R is
//      the largest b2 of its lanes.  Lanes test 64 super-boxes per step against the wave's AABB and ballot; for a
//      surviving super-box they test its 64 boxes and ballot; a surviving box is staged once in LDS and every lane
//      reads the same row (a broadcast).  R shrinks as the lanes improve.
//
// Why pruning is exact: a box is skipped only if its distance to the wave's AABB is > R (strictly), a lane sits out
// a staged box only if its own distance to the box is > its b2.  Both distances use the subtract / multiply / add
// sequence of d(i, j) on the per-axis gaps max(0, lo - p, p - hi).  For p in one box and q in the other the real
// difference |q - p| is at least the real gap; float subtraction, squaring and addition are monotone, so the float
// box distance never exceeds the float d(i, j) of any pair it stands for: a skipped box holds no candidate below
// the lane's b2.
//
// Memory safety for any input bits: row indices come only from the sort's permutation of 0..P-1; the quantised
// cell is clamped with fmaxf / fminf, which drop a NaN operand; an axis of zero (or non-finite) extent maps to
// cell 0.  Outputs of rows with non-finite coordinates are unspecified.
#include <math.h>

#include "hlgs_internal.h"

namespace hlgs {

namespace {

constexpr int kBoxParts = 256;  // most blocks of the bounding-box partial reduction
constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
constexpr int kSortRounds = kKnnSortTile / 64;

struct KnnBufs {
    uint32_t *keys_a, *keys_b, *idx_a, *idx_b;
    uint32_t* hist;      // kRadix x tiles, digit-major
    uint32_t* scan_tmp;
    float* parts;        // kBoxParts x 8: lo xyz -, hi xyz -
    float4* rows;        // P sorted rows
    float4 *blo, *bhi;   // boxes
    float4 *slo, *shi;   // super-boxes
};

inline size_t knn_tiles(size_t P) { return (P + kKnnSortTile - 1) / kKnnSortTile; }
inline size_t knn_boxes(size_t P) { return (P + kKnnBox - 1) / kKnnBox; }
inline size_t knn_supers(size_t P) { return (knn_boxes(P) + kKnnSuper - 1) / kKnnSuper; }

template <typename T>
T* take_knn(char*& p, size_t n)
{
    T* r = reinterpret_cast<T*>(p);
    p += align_up(n * sizeof(T));
    return r;
}

KnnBufs carve_knn(void* base, size_t P, size_t* total)
{
    char* p = static_cast<char*>(base);
    KnnBufs b;
    const size_t hist = (size_t)kRadix * knn_tiles(P);
    b.keys_a = take_knn<uint32_t>(p, P);
    b.keys_b = take_knn<uint32_t>(p, P);
    b.idx_a = take_knn<uint32_t>(p, P);
    b.idx_b = take_knn<uint32_t>(p, P);
    b.hist = take_knn<uint32_t>(p, hist);
    b.scan_tmp = take_knn<uint32_t>(p, scan_scratch_elems(hist));
    b.parts = take_knn<float>(p, (size_t)kBoxParts * 8);
    b.rows = take_knn<float4>(p, P);
    b.blo = take_knn<float4>(p, knn_boxes(P));
    b.bhi = take_knn<float4>(p, knn_boxes(P));
    b.slo = take_knn<float4>(p, knn_supers(P));
    b.shi = take_knn<float4>(p, knn_supers(P));
    if (total) *total = (size_t)(p - static_cast<char*>(base));
    return b;
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fminf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}

// ---------------------------------------------------------------- bounding box and keys
// 256 threads; lo / hi of the block's grid-stride share of the points (fminf / fmaxf drop NaN operands)
__global__ void __launch_bounds__(256) k_knn_bbox(uint32_t P, const float* __restrict__ xyz, float* __restrict__ parts)
{
    __shared__ float red[4][6];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < P; i += (size_t)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            const float v = xyz[3 * i + a];
            lo[a] = fminf(lo[a], v);
            hi[a] = fmaxf(hi[a], v);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = wave_min(lo[a]);
        hi[a] = wave_max(hi[a]);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            red[wid][a] = lo[a];
            red[wid][3 + a] = hi[a];
        }
    }
    __syncthreads();
    if (tid < 3) {
        parts[blockIdx.x * 8 + tid] = fminf(fminf(red[0][tid], red[1][tid]), fminf(red[2][tid], red[3][tid]));
        parts[blockIdx.x * 8 + 4 + tid] =
            fmaxf(fmaxf(red[0][3 + tid], red[1][3 + tid]), fmaxf(red[2][3 + tid], red[3][3 + tid]));
    }
}

__device__ __forceinline__ uint32_t spread10(uint32_t v)  // 10 bits -> every third bit
{
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// 256 threads, one point each.  Every block reduces the nparts (<= 256) partial boxes again: min / max do not
// depend on the order, so all blocks hold the same box.
__global__ void __launch_bounds__(256) k_knn_keys(uint32_t P, const float* __restrict__ xyz,
                                                  const float* __restrict__ parts, int nparts,
                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ idx)
{
    __shared__ float red[4][6];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    float lo[3], hi[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = wave_min(tid < nparts ? parts[tid * 8 + a] : INFINITY);
        hi[a] = wave_max(tid < nparts ? parts[tid * 8 + 4 + a] : -INFINITY);
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
            red[wid][a] = lo[a];
            red[wid][3 + a] = hi[a];
        }
    }
    __syncthreads();
    const size_t i = (size_t)blockIdx.x * 256 + tid;
    if (i >= P) return;
    uint32_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float mn = fminf(fminf(red[0][a], red[1][a]), fminf(red[2][a], red[3][a]));
        const float mx = fmaxf(fmaxf(red[0][3 + a], red[1][3 + a]), fmaxf(red[2][3 + a], red[3][3 + a]));
        const float ext = mx - mn;
        const float scale = (ext > 0.f && ext < INFINITY) ? 1023.f / ext : 0.f;  // zero / non-finite extent: cell 0
        const float t = (xyz[3 * i + a] - mn) * scale;
        const float c = fminf(fmaxf(t, 0.f), 1023.f);  // a NaN t gives 0
        key |= spread10((uint32_t)c) << a;
    }
    keys[i] = key;
    idx[i] = (uint32_t)i;
}

// ---------------------------------------------------------------- radix sort
// digit histogram of one tile of kKnnSortTile keys; hist is digit-major: hist[digit * tiles + tile]
__global__ void __launch_bounds__(256) k_knn_hist(uint32_t P, const uint32_t* __restrict__ keys, int shift,
                                                  uint32_t tiles, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[kRadix];
    const int tid = threadIdx.x;
    h[tid] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * kKnnSortTile;
#pragma unroll
    for (int r = 0; r < kKnnSortTile / 256; r++) {
        const size_t i = base + (size_t)r * 256 + tid;
        if (i < P) atomicAdd(&h[(keys[i] >> shift) & (kRadix - 1)], 1u);  // integer counts: order cannot show
    }
    __syncthreads();
    hist[(size_t)tid * tiles + blockIdx.x] = h[tid];
}

// One wave scatters one tile, 64 keys per round in tile order.  incl is the inclusive scan of hist, so the keys of
// (digit, tile) start at incl[digit * tiles + tile - 1]; within the tile equal digits keep their order (rank by
// ballot among the lanes of a round, rounds in sequence), which is what the next LSD pass relies on.
__global__ void __launch_bounds__(64) k_knn_scatter(uint32_t P, const uint32_t* __restrict__ kin,
                                                    const uint32_t* __restrict__ vin, int shift, uint32_t tiles,
                                                    const uint32_t* __restrict__ incl, uint32_t* __restrict__ kout,
                                                    uint32_t* __restrict__ vout)
{
    __shared__ uint32_t base[kRadix];
    const int lane = threadIdx.x;
    for (int d = lane; d < kRadix; d += 64) {
        const size_t e = (size_t)d * tiles + blockIdx.x;
        base[d] = e ? incl[e - 1] : 0u;
    }
    __syncthreads();
    const unsigned long long lt = (1ull << lane) - 1ull;
    const size_t tile0 = (size_t)blockIdx.x * kKnnSortTile;
    for (int r = 0; r < kSortRounds; r++) {
        const size_t i = tile0 + (size_t)r * 64 + lane;
        const bool valid = i < P;
        const uint32_t key = valid ? kin[i] : 0u;
        const uint32_t val = valid ? vin[i] : 0u;
        const uint32_t digit = (key >> shift) & (kRadix - 1);
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < kRadixBits; b++) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long v = __ballot(bit);
            same &= bit ? v : ~v;
        }
        const uint32_t rank = (uint32_t)__popcll(same & lt);
        const uint32_t pos = base[digit] + rank;
        __syncthreads();
        if (valid && rank == 0) base[digit] += (uint32_t)__popcll(same);  // one lane per digit present
        __syncthreads();
        if (valid && pos < P) {  // pos < P by the counts; the test keeps a broken invariant from writing outside
            kout[pos] = key;
            vout[pos] = val;
        }
    }
}

// ---------------------------------------------------------------- sorted rows, boxes
// one wave per box: gather the rows of the box in sorted order, reduce their AABB
__global__ void __launch_bounds__(256) k_knn_rows(uint32_t P, uint32_t nb, const float* __restrict__ xyz,
                                                  const uint32_t* __restrict__ idx, float4* __restrict__ rows,
                                                  float4* __restrict__ blo, float4* __restrict__ bhi)
{
    const int lane = threadIdx.x & 63;
    const uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (b >= nb) return;
    const size_t i = (size_t)b * kKnnBox + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < P) {
        uint32_t id = idx[i];
        if (id >= P) id = P - 1;  // a permutation of 0..P-1 by construction; never taken
        const float4 r = make_float4(xyz[3 * (size_t)id], xyz[3 * (size_t)id + 1], xyz[3 * (size_t)id + 2],
                                     __uint_as_float(id));
        rows[i] = r;
        lo[0] = hi[0] = r.x;
        lo[1] = hi[1] = r.y;
        lo[2] = hi[2] = r.z;
    }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = wave_min(lo[a]);
        hi[a] = wave_max(hi[a]);
    }
    if (lane == 0) {
        blo[b] = make_float4(lo[0], lo[1], lo[2], 0.f);
        bhi[b] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

// one wave per super-box of kKnnSuper boxes
__global__ void __launch_bounds__(256) k_knn_supers(uint32_t nb, uint32_t ns, const float4* __restrict__ blo,
                                                    const float4* __restrict__ bhi, float4* __restrict__ slo,
                                                    float4* __restrict__ shi)
{
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= ns) return;
    const size_t b = (size_t)s * kKnnSuper + lane;
    float4 lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f), hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    if (b < nb) {
        lo = blo[b];
        hi = bhi[b];
    }
    lo.x = wave_min(lo.x), lo.y = wave_min(lo.y), lo.z = wave_min(lo.z);
    hi.x = wave_max(hi.x), hi.y = wave_max(hi.y), hi.z = wave_max(hi.z);
    if (lane == 0) {
        slo[s] = lo;
        shi[s] = hi;
    }
}

// ---------------------------------------------------------------- search
// squared distance between the boxes [alo, ahi] and [blo, bhi] (a point is a box with lo = hi): the operation
// sequence of d(i, j) on the per-axis gaps
__device__ __forceinline__ float box_dist2(const float4& alo, const float4& ahi, const float4& blo, const float4& bhi)
{
    const float gx = fmaxf(0.f, fmaxf(blo.x - ahi.x, alo.x - bhi.x));
    const float gy = fmaxf(0.f, fmaxf(blo.y - ahi.y, alo.y - bhi.y));
    const float gz = fmaxf(0.f, fmaxf(blo.z - ahi.z, alo.z - bhi.z));
    return (gx * gx + gy * gy) + gz * gz;
}

struct Best3 {
    float b0, b1, b2;
};

// The kKnnBox rows staged in LDS against this lane's point; every lane reads the same row (a broadcast).  The trip
// count is fixed so that the reads of several rows are in flight at once: a box with fewer rows is padded with NaN
// rows, whose distance is no candidate.
__device__ __forceinline__ void scan_rows(const float4* __restrict__ lds, const float4& me, Best3& k)
{
    const uint32_t my = __float_as_uint(me.w);
#pragma unroll 8
    for (int j = 0; j < kKnnBox; j++) {
        const float4 q = lds[j];
        const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
        float d = (dx * dx + dy * dy) + dz * dz;
        d = fminf(d, INFINITY);                          // a NaN distance is no candidate
        d = __float_as_uint(q.w) == my ? INFINITY : d;   // other indices only
        const float n2 = fminf(k.b2, fmaxf(k.b1, d));
        const float n1 = fminf(k.b1, fmaxf(k.b0, d));
        k.b0 = fminf(k.b0, d);
        k.b1 = n1;
        k.b2 = n2;
    }
}

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ float4 uniform4(const float4& v)
{
    return make_float4(uniform(v.x), uniform(v.y), uniform(v.z), 0.f);
}

// one wave (one block) per box of 64 sorted rows
__global__ void __launch_bounds__(64) k_knn_search(uint32_t P, uint32_t nb, uint32_t ns,
                                                   const float4* __restrict__ rows, const float4* __restrict__ blo,
                                                   const float4* __restrict__ bhi, const float4* __restrict__ slo,
                                                   const float4* __restrict__ shi, float* __restrict__ out)
{
    __shared__ float4 lds[kKnnBox];                        // the staged box's rows
    __shared__ float4 lds_lo[kKnnSuper], lds_hi[kKnnSuper];  // the AABBs of the current super-box's boxes
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x;
    const size_t i = (size_t)g * kKnnBox + lane;
    const bool valid = i < P;
    const float4 pad = make_float4(NAN, NAN, NAN, __uint_as_float(0xffffffffu));  // a padding row: no index, no distance
    float4 me = pad;
    if (valid) me = rows[i];
    Best3 k = {INFINITY, INFINITY, INFINITY};

    // step 1: the wave's own box
    lds[lane] = me;
    __syncthreads();
    scan_rows(lds, me, k);
    const float4 glo = uniform4(blo[g]), ghi = uniform4(bhi[g]);
    float R = uniform(wave_max(valid ? k.b2 : 0.f));

    // steps 2 and 3: super-boxes, the wave's own first (its boxes are the likeliest to shrink R early)
    const uint32_t own = g / kKnnSuper;
    for (uint32_t pass = 0; pass < 2; pass++) {
        const uint32_t s_begin = pass == 0 ? own : 0u, s_end = pass == 0 ? own + 1u : ns;
        for (uint32_t s0 = s_begin; s0 < s_end; s0 += 64) {
            const uint32_t s = s0 + lane;
            bool hit = s < s_end && (pass == 0 || s != own);
            if (hit) hit = !(box_dist2(glo, ghi, slo[s], shi[s]) > R);
            unsigned long long sm = __ballot(hit);
            while (sm) {
                const uint32_t sb = s0 + (uint32_t)__builtin_ctzll(sm);
                sm &= sm - 1;
                if (box_dist2(glo, ghi, slo[sb], shi[sb]) > R) continue;  // R may have shrunk since the ballot
                const uint32_t b = sb * kKnnSuper + lane;
                bool bhit = b < nb && b != g;
                __syncthreads();  // the previous super-box's AABBs and rows are read
                if (bhit) {
                    const float4 lo = blo[b], hi = bhi[b];
                    lds_lo[lane] = lo;
                    lds_hi[lane] = hi;
                    bhit = !(box_dist2(glo, ghi, lo, hi) > R);
                }
                unsigned long long bm = __ballot(bhit);
                __syncthreads();
                while (bm) {
                    const int j = __builtin_ctzll(bm);
                    bm &= bm - 1;
                    // the lane sits this box out unless the box comes within its own b2
                    const bool active = valid && !(box_dist2(me, me, lds_lo[j], lds_hi[j]) > k.b2);
                    if (!__ballot(active)) continue;
                    const size_t r0 = ((size_t)sb * kKnnSuper + j) * kKnnBox;
                    __syncthreads();  // the previous box's rows are read
                    float4 row = pad;
                    if (r0 + lane < P) row = rows[r0 + lane];
                    lds[lane] = row;
                    __syncthreads();
                    if (active) scan_rows(lds, me, k);
                }
                R = uniform(wave_max(valid ? k.b2 : 0.f));
            }
        }
    }
    if (valid) {
        const uint32_t id = __float_as_uint(me.w);
        if (id < P) out[id] = ((k.b0 + k.b1) + k.b2) / 3.0f;  // id < P by construction
    }
}

}  // namespace

size_t knn_scratch_bytes(int P)
{
    size_t total = 0;
    carve_knn(nullptr, (size_t)(P > 0 ? P : 0), &total);
    return total;
}

// The sort on its own (also used by hier_build.hip): P pairs by the whole 32-bit key, stable.
size_t radix_hist_elems(size_t P) { return (size_t)kRadix * knn_tiles(P); }

void radix_sort_pairs_u32(uint32_t P, uint32_t* keys, uint32_t* vals, uint32_t* keys_tmp, uint32_t* vals_tmp,
                          uint32_t* hist, uint32_t* scan_tmp, hipStream_t s)
{
    const uint32_t tiles = (uint32_t)knn_tiles(P);
    uint32_t *kin = keys, *vin = vals, *kout = keys_tmp, *vout = vals_tmp;
    const size_t nh = (size_t)kRadix * tiles;
    for (int shift = 0; shift < 32; shift += kRadixBits) {  // four passes, ending in keys / vals
        hipLaunchKernelGGL(k_knn_hist, dim3(tiles), dim3(256), 0, s, P, kin, shift, tiles, hist);
        scan_inclusive_u32(hist, hist, nh, scan_tmp, s);
        hipLaunchKernelGGL(k_knn_scatter, dim3(tiles), dim3(64), 0, s, P, kin, vin, shift, tiles, hist, kout, vout);
        uint32_t* t = kin;
        kin = kout, kout = t;
        t = vin, vin = vout, vout = t;
    }
}

void launch_knn(int P_, const float* xyz, void* scratch, float* out, hipStream_t s)
{
    if (P_ <= 0) return;
    const uint32_t P = (uint32_t)P_;
    const KnnBufs b = carve_knn(scratch, P, nullptr);
    const uint32_t nb = (uint32_t)knn_boxes(P), ns = (uint32_t)knn_supers(P);
    const uint32_t per256 = (P + 255u) / 256u;
    const int nparts = (int)(per256 < (uint32_t)kBoxParts ? per256 : (uint32_t)kBoxParts);
    hipLaunchKernelGGL(k_knn_bbox, dim3(nparts), dim3(256), 0, s, P, xyz, b.parts);
    hipLaunchKernelGGL(k_knn_keys, dim3(per256), dim3(256), 0, s, P, xyz, b.parts, nparts, b.keys_a, b.idx_a);
    radix_sort_pairs_u32(P, b.keys_a, b.idx_a, b.keys_b, b.idx_b, b.hist, b.scan_tmp, s);  // 30 key bits
    hipLaunchKernelGGL(k_knn_rows, dim3((nb + 3u) / 4u), dim3(256), 0, s, P, nb, xyz, b.idx_a, b.rows, b.blo, b.bhi);
    hipLaunchKernelGGL(k_knn_supers, dim3((ns + 3u) / 4u), dim3(256), 0, s, nb, ns, b.blo, b.bhi, b.slo, b.shi);
    hipLaunchKernelGGL(k_knn_search, dim3(nb), dim3(64), 0, s, P, nb, ns, b.rows, b.blo, b.bhi, b.slo, b.shi, out);
}

}  // namespace hlgs
