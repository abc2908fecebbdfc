// density.hip -- the adaptive density control of chunk training (train_single.py:144-155), the stage between two
// optimizer steps that changes the number of Gaussians:
//
//   k_density_stats    add_densification_stats (train_single.py:147-148, scene/gaussian_model.py:1527-1530)
//   k_density_select   the masks of densify / densify_and_prune (:1458-1468, :1508, :1512-1514)
//   k_density_flags/_lists + scan.hip   the round's plan: the kept rows and the selected rows, ascending
//   k_density_emit     every output table of the round in one launch: _prune_optimizer (:1254-1258, :1279-1282),
//                      cat_tensors_to_optimizer (:1302-1306) and the new rows of densify_and_clone (:1420-1426),
//                      densify (:1473-1479) and densify_and_split (:1367-1376)
//   k_opacity_reset    reset_opacity (:1214-1218) with replace_tensor_to_optimizer's zeroed moments (:1237-1238)
//
// The reference's own plumbing cannot be called (add_densification_stats takes three arguments and is given two,
// densify* reads self.nodes, the prune is commented out at :1401-1402 and :1516), so the arithmetic of the cited
// lines is the contract.
//
// Order.  The reference appends the new rows and then prunes ("cat, then mask"); here the old rows are pruned and the
// new rows appended behind them.  The two are the same table: a row cannot be both selected and pruned, because
// densify_min_opacity (0.15) > prune_min_opacity (0.005), and a new row cannot be pruned in its own round, because
// its opacity is at least 0.15 / (0.8 N) (shrink; clone and split keep the parent's).  Output row d < n_kept is input
// row kept[d]; output row n_kept + copies j + k is copy k of parent selected[j], repeat_interleave's order (:1473)
// behind torch.cat's (:1306).
//
// Rounding.  A transformed value (four to seven per new row, against 708 bytes of row traffic) is computed in float64
// from the float32 inputs and rounded to float32 once, as hlgs_mcmc_noise does; the selection evaluates its rule in
// float64 as well, so a decision differs from the float64 rule only where a product sits within float64 rounding of
// its threshold.  Nothing here must be bit-equal to a float32 restatement, so the file is compiled with the default
// contraction.
//
// Deviations.  clone copies `scaling` bit for bit where the reference writes log(exp(s)) (:1421, a float32 round trip
// that moves the value by up to an ulp and means nothing).  The opacity reset writes logit(0.01) to the rows above it
// and leaves the others alone, where the reference's inverse_sigmoid(min(sigmoid(x), 0.01)) (:1215) sends every
// logit through a float32 sigmoid and back: below x = -17 that round trip loses the logit's digits and below -88 it
// returns -inf.
//
// Every store is an ordinary vector store from plain C++; the emit's 16-byte stores are non-temporal (the output
// tables are written once and not read again in the round, DESIGN section 9 "Round 7").
#include "hlgs_internal.h"
#include "hlgs_rng.h"

namespace hlgs {

// ---------------------------------------------------------------- statistics
__global__ void __launch_bounds__(256) k_density_stats(int64_t P, const float* __restrict__ g,
                                                       const int* __restrict__ radii, float* __restrict__ accum,
                                                       float* __restrict__ denom, float* __restrict__ maxr)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int r = radii[p];
    if (r <= 0) return;
    const float fr = (float)r, m = maxr[p];
    maxr[p] = (m != m || m >= fr) ? m : fr;  // torch.max: a NaN stays
    const float gx = g[3 * p], gy = g[3 * p + 1];
    const float nrm = sqrtf(gx * gx + gy * gy), a = accum[p];
    accum[p] = (a != a || a >= nrm) ? a : nrm;  // nrm NaN: a >= nrm is false, the NaN is taken, as torch.max does
    denom[p] += 1.0f;
}

void launch_density_stats(int64_t P, const float* g, const int* radii, float* accum, float* denom, float* maxr,
                          hipStream_t s)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_density_stats, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, g, radii, accum, denom,
                       maxr);
}

// ---------------------------------------------------------------- selection
__device__ __forceinline__ double sigmoid64(float x) { return 1.0 / (1.0 + exp(-(double)x)); }

__global__ void __launch_bounds__(256) k_density_select(int64_t P, const float* __restrict__ accum,
                                                        const float* __restrict__ maxr, const float* __restrict__ op,
                                                        const uint8_t* __restrict__ leaf, double thr, double dmin,
                                                        double pmin, int64_t protect, uint8_t* __restrict__ sel,
                                                        uint8_t* __restrict__ prune)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double o = sigmoid64(op[p]);
    const float a = accum[p];
    const double gr = a != a ? 0.0 : (double)a;  // grads[grads.isnan()] = 0.0 (:1508)
    const bool free_row = p >= protect;
    const bool s = gr * (double)maxr[p] * pow(o, 1.0 / 5.0) >= thr && o > dmin && (!leaf || leaf[p]) && free_row;
    sel[p] = s ? 1 : 0;
    prune[p] = (pmin >= 0.0 && o < pmin && free_row) ? 1 : 0;
}

void launch_density_select(int64_t P, const float* accum, const float* maxr, const float* op, const uint8_t* leaf,
                           double thr, double dmin, double pmin, int64_t protect, uint8_t* sel, uint8_t* prune,
                           hipStream_t s)
{
    if (P <= 0) return;
    hipLaunchKernelGGL(k_density_select, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, accum, maxr, op, leaf,
                       thr, dmin, pmin, protect, sel, prune);
}

// ---------------------------------------------------------------- plan
struct DensifyScratch {
    int* counts;        // [n_kept, n_selected]
    uint32_t* kincl;    // P: keep flags, then their inclusive scan
    uint32_t* sincl;    // P: select flags, then their inclusive scan
    int* kept;          // P
    int* selected;      // P
    uint32_t* tmp;      // scan_scratch_elems(P)
};
static DensifyScratch carve_densify(void* scratch, int64_t P, size_t* total)
{
    char* p = reinterpret_cast<char*>(align_up((size_t)scratch));
    char* const p0 = p;
    const size_t rows = align_up(sizeof(int) * (size_t)P);
    DensifyScratch d;
    d.counts = reinterpret_cast<int*>(p);
    p += kAlign;
    d.kincl = reinterpret_cast<uint32_t*>(p);
    p += rows;
    d.sincl = reinterpret_cast<uint32_t*>(p);
    p += rows;
    d.kept = reinterpret_cast<int*>(p);
    p += rows;
    d.selected = reinterpret_cast<int*>(p);
    p += rows;
    d.tmp = reinterpret_cast<uint32_t*>(p);
    p += align_up(sizeof(uint32_t) * scan_scratch_elems((size_t)P));
    if (total) *total = (size_t)(p - p0);
    return d;
}
size_t densify_scratch_bytes(int64_t P)
{
    size_t t = 0;
    carve_densify(nullptr, P < 0 ? 0 : P, &t);
    return t + kAlign;
}
const int* densify_counts(void* scratch, int64_t P) { return carve_densify(scratch, P, nullptr).counts; }

__global__ void __launch_bounds__(256) k_density_flags(int64_t P, const uint8_t* __restrict__ sel,
                                                       const uint8_t* __restrict__ prune, int drop_selected,
                                                       uint32_t* __restrict__ kflag, uint32_t* __restrict__ sflag)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const bool s = sel[p] != 0, d = prune && prune[p] != 0;
    kflag[p] = (d || (drop_selected && s)) ? 0u : 1u;
    sflag[p] = s ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_density_lists(int64_t P, const uint32_t* __restrict__ kincl,
                                                       const uint32_t* __restrict__ sincl, int* __restrict__ kept,
                                                       int* __restrict__ selected, int* __restrict__ counts)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const uint32_t k1 = kincl[p], k0 = p ? kincl[p - 1] : 0u;
    const uint32_t s1 = sincl[p], s0 = p ? sincl[p - 1] : 0u;
    if (k1 != k0) kept[k0] = (int)p;          // k0 < k1 <= P
    if (s1 != s0) selected[s0] = (int)p;
    if (p == P - 1) {
        counts[0] = (int)k1;
        counts[1] = (int)s1;
    }
}

void launch_densify_plan(int64_t P, const uint8_t* sel, const uint8_t* prune, int drop_selected, void* scratch,
                         hipStream_t s)
{
    const DensifyScratch d = carve_densify(scratch, P, nullptr);
    const dim3 grid((unsigned)((P + 255) / 256));
    hipLaunchKernelGGL(k_density_flags, grid, dim3(256), 0, s, P, sel, prune, drop_selected, d.kincl, d.sincl);
    scan_inclusive_u32(d.kincl, d.kincl, (size_t)P, d.tmp, s);
    scan_inclusive_u32(d.sincl, d.sincl, (size_t)P, d.tmp, s);  // the same stream: tmp is free again
    hipLaunchKernelGGL(k_density_lists, grid, dim3(256), 0, s, P, d.kincl, d.sincl, d.kept, d.selected, d.counts);
}

// ---------------------------------------------------------------- emit
// One 1-D grid over every table's 16-byte destination chunks, destination-major as k_rows_compact (stream.hip): block
// b writes kEmitChunks consecutive chunks of one table, a thread kEmitU of them 256 chunks apart, all of its loads
// issued ahead of its stores.  A chunk's four words lie in output rows r .. r_end:
//   all kept, and kept[r .. r_end] consecutive in the source   one 16-byte load at 4-byte alignment
//   all new, role zero                                         no load
//   all new, one row, copied                                   one 16-byte load from the parent's row
//   anything else (a kept / new boundary, a row boundary between copies, a transformed table)   word by word
// A transformed word is recomputed from the parent's float32 row in float64: only the 1- and 3-float tables are
// transformed, so the float64 work is a few values per new row.  The copy is bound by the index arithmetic in front
// of its loads, not by the loads (2.2 -> 3.3 TB/s from cheaper arithmetic alone; the store flavour and the
// order of the loads made no difference), hence one 32-bit division per thread and none for the kept rows.
constexpr int kEmitU = 4;
constexpr int kEmitChunks = 256 * kEmitU;
struct EmitTable {
    const uint32_t* src;
    uint32_t* dst;
    int words;   // per row
    int role;    // HLGS_DENSIFY_* after the mode has been applied: a role the mode does not transform is COPY here
    int dr, dk;  // 1,024 words (the distance of a thread's chunks) = dr rows and dk words
};
struct EmitArgs {
    EmitTable t[kMaxRowTables];
    int bstart[kMaxRowTables + 1];
    int T, copies, mode;
    int64_t n_kept, n_sel;
    const int* kept;
    const int* selected;
    const int* counts;
    const float* xyz;       // split: the parent's position, log-scale and quaternion
    const float* scaling;
    const float* rotation;
    const float* opacity;   // shrink
    const float* noise;
    uint64_t seed;
    uint32_t round;
    double shrink;          // 0.8 copies (shrink) or 0.7 copies (split): what the activated value is divided by
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_a4 __attribute__((aligned(4)));  // 16-byte access at 4-byte alignment (global_load_dwordx4)

// the input row behind output row d < n_kept + copies n_sel (< 2^31): kept[d], or the parent of new row d - n_kept
__device__ __forceinline__ int emit_src_row(const EmitArgs& a, int64_t d)
{
    if (d < a.n_kept) return a.kept[d];  // a branch: four waves in five lie wholly in the kept rows and skip the division
    return a.selected[(uint32_t)(d - a.n_kept) / (uint32_t)a.copies];
}

__device__ __forceinline__ uint32_t emit_new_word(const EmitArgs& a, const EmitTable& tb, int64_t rnew, int k)
{
    if (tb.role == HLGS_DENSIFY_ZERO) return 0u;
    const int64_t p = a.selected[(uint32_t)rnew / (uint32_t)a.copies];
    if (tb.role == HLGS_DENSIFY_COPY) return tb.src[p * tb.words + k];
    if (tb.role == HLGS_DENSIFY_SCALING)
        return __float_as_uint((float)log(exp((double)a.scaling[3 * p + k]) / a.shrink));
    if (tb.role == HLGS_DENSIFY_OPACITY) {
        const double y = sigmoid64(a.opacity[p]) / a.shrink;
        return __float_as_uint((float)log(y / (1.0 - y)));
    }
    // HLGS_DENSIFY_XYZ, split: R(q / |q|) (exp(s) * xi) + xyz, row k of R only
    double q0 = a.rotation[4 * p], q1 = a.rotation[4 * p + 1], q2 = a.rotation[4 * p + 2], q3 = a.rotation[4 * p + 3];
    const double d = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / d, x = q1 / d, y = q2 / d, z = q3 / d;
    double R0, R1, R2;
    if (k == 0) R0 = 1.0 - 2.0 * (y * y + z * z), R1 = 2.0 * (x * y - r * z), R2 = 2.0 * (x * z + r * y);
    else if (k == 1) R0 = 2.0 * (x * y + r * z), R1 = 1.0 - 2.0 * (x * x + z * z), R2 = 2.0 * (y * z - r * x);
    else R0 = 2.0 * (x * z - r * y), R1 = 2.0 * (y * z + r * x), R2 = 1.0 - 2.0 * (x * x + y * y);
    float n0, n1, n2;
    if (a.noise) {
        n0 = a.noise[3 * rnew], n1 = a.noise[3 * rnew + 1], n2 = a.noise[3 * rnew + 2];
    } else {
        n0 = rng_normal(a.seed, a.round, 3 * (uint64_t)rnew);
        n1 = rng_normal(a.seed, a.round, 3 * (uint64_t)rnew + 1);
        n2 = rng_normal(a.seed, a.round, 3 * (uint64_t)rnew + 2);
    }
    const double v0 = exp((double)a.scaling[3 * p]) * n0, v1 = exp((double)a.scaling[3 * p + 1]) * n1;
    const double v2 = exp((double)a.scaling[3 * p + 2]) * n2;
    return __float_as_uint((float)(R0 * v0 + R1 * v1 + R2 * v2 + (double)a.xyz[3 * p + k]));
}

__global__ void __launch_bounds__(256) k_density_emit(EmitArgs a)
{
    // the counts the tables were sized from must be the plan's (a stale scratch would index outside the inputs)
    if (a.counts[0] != (int)a.n_kept || a.counts[1] != (int)a.n_sel) return;
    int t = 0;
    for (int j = 1; j < a.T; j++) t += (int)blockIdx.x >= a.bstart[j];
    const EmitTable& tb = a.t[t];
    const int64_t words = tb.words;
    const int64_t n_out = a.n_kept + a.n_sel * a.copies;
    const int64_t total = n_out * words;
    const int64_t w0 = ((int64_t)((int)blockIdx.x - a.bstart[t]) * kEmitChunks + threadIdx.x) * 4;
    if (w0 >= total) return;
    const uint32_t* __restrict__ src = tb.src;
    uint32_t* __restrict__ dst = tb.dst;
    // (row, word) of the four chunks with one division, 32-bit whenever the table's words fit (a 64-bit division is
    // ~150 instructions; six of them per thread held the copy at 2.6 TB/s): a thread's chunks are 1,024 words apart,
    // which the host has split into tb.dr rows and tb.dk words
    int rr[kEmitU], kk[kEmitU], re[kEmitU];
    {
        int r1, k1;
        if (total <= 0xffffffffll) {
            const uint32_t q = (uint32_t)w0 / (uint32_t)tb.words;
            r1 = (int)q;
            k1 = (int)((uint32_t)w0 - q * (uint32_t)tb.words);
        } else {
            const int64_t q = w0 / words;
            r1 = (int)q;
            k1 = (int)(w0 - q * words);
        }
#pragma unroll
        for (int u = 0; u < kEmitU; u++) {
            rr[u] = r1;
            kk[u] = k1;
            int e = k1 + 3, r = r1;
            while (e >= tb.words) { e -= tb.words; r++; }  // at most three rounds: k1 < words
            re[u] = r;
            r1 += tb.dr;
            k1 += tb.dk;
            if (k1 >= tb.words) { k1 -= tb.words; r1++; }
        }
    }
    // the source rows of every chunk's first and last output row: all index loads in flight together, then all row
    // loads, then the stores (a thread's four chunks are independent; branching per chunk serialised their latencies)
    int s0[kEmitU], s1[kEmitU];
#pragma unroll
    for (int u = 0; u < kEmitU; u++) {
        const bool in = w0 + u * 1024 < total;
        s0[u] = in ? emit_src_row(a, rr[u]) : 0;
        s1[u] = in ? emit_src_row(a, re[u] < n_out ? re[u] : n_out - 1) : 0;
    }
    u32x4 v[kEmitU];
    bool slow[kEmitU];
#pragma unroll
    for (int u = 0; u < kEmitU; u++) {
        const int64_t wu = w0 + u * 1024;
        const bool whole = wu + 4 <= total, all_new = rr[u] >= a.n_kept;
        const bool fast = whole && ((re[u] < a.n_kept && s1[u] - s0[u] == re[u] - rr[u]) ||
                                    (all_new && tb.role == HLGS_DENSIFY_COPY && rr[u] == re[u]));
        slow[u] = wu < total && !fast && !(whole && all_new && tb.role == HLGS_DENSIFY_ZERO);
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (fast) v[u] = *reinterpret_cast<const u32x4_a4*>(src + (int64_t)s0[u] * words + kk[u]);
    }
#pragma unroll
    for (int u = 0; u < kEmitU; u++) {
        if (!slow[u]) continue;
        const int64_t wu = w0 + u * 1024;
        // word by word, the four words' row lookups together and then their loads (the narrow tables, whose chunks
        // span rows, come here whenever a pruned row or a copy boundary lies inside the chunk)
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        int64_t r2[4];
        int k2[4], sr[4];
        bool live[4];
        {
            int64_t r = rr[u];
            int k = (int)kk[u];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                live[q] = wu + q < total;
                r2[q] = r;
                k2[q] = k;
                if (++k == words) { k = 0; r++; }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) sr[q] = live[q] ? emit_src_row(a, r2[q]) : 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool is_new = r2[q] >= a.n_kept;
            if (live[q] && (!is_new || tb.role == HLGS_DENSIFY_COPY)) w[q] = src[(int64_t)sr[q] * words + k2[q]];
        }
        if (tb.role > HLGS_DENSIFY_ZERO) {  // a transformed table
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (live[q] && r2[q] >= a.n_kept) w[q] = emit_new_word(a, tb, r2[q] - a.n_kept, k2[q]);
        }
        v[u] = u32x4{w[0], w[1], w[2], w[3]};
    }
    const bool aligned16 = (reinterpret_cast<uintptr_t>(dst) & 15u) == 0;
#pragma unroll
    for (int u = 0; u < kEmitU; u++) {
        const int64_t wu = w0 + u * 1024;
        if (wu >= total) continue;
        if (wu + 4 <= total) {
            if (aligned16) {
                __builtin_nontemporal_store(v[u], reinterpret_cast<u32x4*>(dst + wu));
            } else {
                *reinterpret_cast<u32x4_a4*>(dst + wu) = v[u];
            }
        } else {
            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
            for (int q = 0; q < 4 && wu + q < total; q++) dst[wu + q] = w[q];
        }
    }
}

// tables: T <= kMaxRowTables entries with row_bytes > 0 (the caller has dropped the empty ones)
int launch_densify_emit(int T, const hlgs_densify_table* tables, int64_t P, int64_t n_kept, int64_t n_sel, int copies,
                        int mode, const float* rotation, const float* noise, uint64_t seed, uint32_t round,
                        void* scratch, hipStream_t s)
{
    const DensifyScratch d = carve_densify(scratch, P, nullptr);
    EmitArgs a{};
    a.T = T, a.copies = copies, a.mode = mode, a.n_kept = n_kept, a.n_sel = n_sel;
    a.kept = d.kept, a.selected = d.selected, a.counts = d.counts;
    a.rotation = rotation, a.noise = noise, a.seed = seed, a.round = round;
    a.shrink = (mode == HLGS_DENSIFY_SPLIT ? 0.7 : 0.8) * (double)copies;
    const int64_t n_out = n_kept + n_sel * copies;
    int64_t blocks = 0;
    for (int t = 0; t < T; t++) {
        int role = tables[t].role;
        if (role == HLGS_DENSIFY_XYZ) a.xyz = static_cast<const float*>(tables[t].src);
        if (role == HLGS_DENSIFY_SCALING) a.scaling = static_cast<const float*>(tables[t].src);
        if (role == HLGS_DENSIFY_OPACITY) a.opacity = static_cast<const float*>(tables[t].src);
        const bool transformed = (mode == HLGS_DENSIFY_SHRINK && (role == HLGS_DENSIFY_SCALING || role == HLGS_DENSIFY_OPACITY)) ||
                                 (mode == HLGS_DENSIFY_SPLIT && (role == HLGS_DENSIFY_SCALING || role == HLGS_DENSIFY_XYZ));
        if (role != HLGS_DENSIFY_ZERO && !transformed) role = HLGS_DENSIFY_COPY;
        a.t[t].src = static_cast<const uint32_t*>(tables[t].src);
        a.t[t].dst = static_cast<uint32_t*>(tables[t].dst);
        a.t[t].words = (int)(tables[t].row_bytes >> 2);
        a.t[t].role = role;
        a.t[t].dr = 1024 / a.t[t].words;
        a.t[t].dk = 1024 % a.t[t].words;
        a.bstart[t] = (int)blocks;
        const int64_t chunks = (n_out * a.t[t].words + 3) / 4;
        blocks += (chunks + kEmitChunks - 1) / kEmitChunks;
    }
    a.bstart[T] = (int)blocks;
    if (blocks >= (1ll << 31)) return 1;
    if (blocks > 0) hipLaunchKernelGGL(k_density_emit, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return 0;
}

// ---------------------------------------------------------------- opacity reset
__global__ void __launch_bounds__(256) k_opacity_reset(int64_t P, int64_t protect, double cap, float value,
                                                       float* __restrict__ op, float* __restrict__ m,
                                                       float* __restrict__ v)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    if (p >= protect && sigmoid64(op[p]) > cap) op[p] = value;
    if (m) m[p] = 0.0f;
    if (v) v[p] = 0.0f;
}

void launch_opacity_reset(int64_t P, int64_t protect, double cap, float* op, float* m, float* v, hipStream_t s)
{
    if (P <= 0) return;
    const float value = (float)log(cap / (1.0 - cap));
    hipLaunchKernelGGL(k_opacity_reset, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, protect, cap, value, op,
                       m, v);
}

}  // namespace hlgs
