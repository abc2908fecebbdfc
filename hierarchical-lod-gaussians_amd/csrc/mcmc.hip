// mcmc.hip -- the GPU pieces of the MCMC densification round (train_post.py:70-75, 707-789, 868-878):
//
//   hlgs_mcmc_sample   opacity-weighted sampling with replacement: GaussianModel._sample_alives
//                      (scene/gaussian_model.py:1580-1586) with the probabilities its callers build (:1614, :1714)
//   hlgs_mcmc_noise    the position noise of train_post.py:868-878 in one pass over the resident rows
//   hlgs_rng_fill      the counter-based numbers both draw from (hlgs_rng.h)
//
// The sampler.  Candidate i weighs w_i = 1 / (1 + exp(-x_i)) of its float32 logit x_i, evaluated in float64; logits
// below kMcmcZeroLogit weigh exactly 0 (float32's sigmoid underflows there: 2^-149 = e^-103.3).  C is the inclusive
// prefix sum of w in float64, associated in a fixed four-level tree that does not depend on the launch:
//   thread  8 consecutive candidates, summed in order                                v_0..v_7
//   wave    64 threads chained in lane order,        E_{t+1} = E_t + v_7(t)
//   block   4 waves chained in order,                W_{k+1} = W_k + E_64(k)          (2,048 candidates per block)
//   grid    the blocks chained in order by one wave, B_{b+1} = B_b + W_4(b)
//   C_i = B_b + (W_k + (E_t + v_j))
// Every level is a serial chain whose step is the last value of the level below, so C is non-decreasing and
// C_i == C_{i-1} exactly where w_i == 0 -- which is what keeps a zero weight from ever being drawn: draw j takes
// uniform number j of (seed, stream), u_j in [0, 1), and the smallest i with C_i > u_j C_n, found by two binary
// searches (the block totals B, then the block's 2,048 local sums).  A float32 running sum would stop growing at 2^24
// equal weights (the failure behind the reference's 16,000,000-candidate subsampling, :1611-1613, :1709-1711).  No
// floating-point atomics; the counts are integer atomics, so the result is the same bits on every run.
#include "hlgs_internal.h"
#include "hlgs_rng.h"

namespace hlgs {

constexpr float kMcmcZeroLogit = -103.0f;

struct McmcHeader {   // first words of the sampler's scratch, read by the caller after the call
    double total;     // C_n
    int status;       // 0 ok; bit 0: no candidates, or a total weight of 0 or non-finite; bit 1: a drawn row outside
    int pad;          //      [0, size)
};
static_assert(sizeof(McmcHeader) == HLGS_MCMC_HEADER_BYTES, "the header the callers read");

struct McmcScratch {
    McmcHeader* hdr;
    double* bincl;    // nb: inclusive block totals B_{b+1}
    double* local;    // n: W_k + (E_t + v_j), the prefix inside the candidate's block
};
static McmcScratch carve_mcmc(void* scratch, int64_t n, size_t* total)
{
    const size_t nb = (size_t)((n + kMcmcItems - 1) / kMcmcItems);
    char* p = reinterpret_cast<char*>(align_up((size_t)scratch));
    McmcScratch m;
    m.hdr = reinterpret_cast<McmcHeader*>(p);
    p += kAlign;
    m.bincl = reinterpret_cast<double*>(p);
    p += align_up(sizeof(double) * nb);
    m.local = reinterpret_cast<double*>(p);
    p += align_up(sizeof(double) * (size_t)n);
    if (total) *total = (size_t)(p - reinterpret_cast<char*>(align_up((size_t)scratch)));
    return m;
}
size_t mcmc_sample_scratch_bytes(int64_t n)
{
    size_t t = 0;
    carve_mcmc(nullptr, n < 0 ? 0 : n, &t);
    return t + kAlign;
}

// total of the 64 lanes' values chained in lane order; *excl = the chain's value before this lane's step
__device__ __forceinline__ double wave_chain(double v, int lane, double start, double* excl)
{
    double run = start, mine = start;
#pragma unroll
    for (int l = 0; l < 64; l++) {
        const double t = __shfl(v, l, 64);
        if (lane == l) mine = run;
        run = run + t;
    }
    *excl = mine;
    return run;
}

__global__ void __launch_bounds__(256) k_mcmc_scan_local(int64_t n, const char* __restrict__ base, int64_t stride,
                                                         const int* __restrict__ alive, double* __restrict__ local,
                                                         double* __restrict__ bsum)
{
    __shared__ double wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t first = (int64_t)blockIdx.x * kMcmcItems + (int64_t)tid * 8;
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double w = 0.0;
        if (first + i < n) {
            const int64_t row = alive ? (int64_t)alive[first + i] : first + i;
            const float x = *reinterpret_cast<const float*>(base + row * stride);
            w = x < kMcmcZeroLogit ? 0.0 : 1.0 / (1.0 + exp(-(double)x));
        }
        v[i] = w;
    }
#pragma unroll
    for (int i = 1; i < 8; i++) v[i] = v[i - 1] + v[i];
    double E;
    const double wave_total = wave_chain(v[7], lane, 0.0, &E);
    if (lane == 0) wtot[wid] = wave_total;
    __syncthreads();
    double W = 0.0, mineW = 0.0;
    for (int k = 0; k < 4; k++) {
        if (k == wid) mineW = W;
        W = W + wtot[k];
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (first + i < n) local[first + i] = mineW + (E + v[i]);
    if (tid == 0) bsum[blockIdx.x] = W;
}

// one wave: the block totals chained in block order, in place (bsum -> B_{b+1}); the header
__global__ void __launch_bounds__(64) k_mcmc_scan_blocks(int64_t n, int64_t nb, double* __restrict__ bincl,
                                                         McmcHeader* __restrict__ hdr)
{
    const int lane = threadIdx.x;
    double run = 0.0;
    for (int64_t c = 0; c < nb; c += 64) {
        const double t = c + lane < nb ? bincl[c + lane] : 0.0;
        double excl;
        run = wave_chain(t, lane, run, &excl);
        if (c + lane < nb) bincl[c + lane] = excl + t;
    }
    if (lane == 0) {
        hdr->total = run;
        hdr->status = (n > 0 && run > 0.0 && run <= 1.7976931348623157e308) ? 0 : 1;  // NaN fails both comparisons
        hdr->pad = 0;
    }
}

__global__ void __launch_bounds__(256) k_mcmc_draw(int64_t n, int64_t nb, const int* __restrict__ alive, int64_t num,
                                                   uint64_t seed, uint32_t stream_id, const double* __restrict__ bincl,
                                                   const double* __restrict__ local, McmcHeader* __restrict__ hdr,
                                                   int* __restrict__ sampled, int* __restrict__ counts, int64_t size)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= num) return;
    if (hdr->status & 1) {
        sampled[j] = -1;
        return;
    }
    const double t = rng_uniform53(seed, stream_id, (uint64_t)j) * hdr->total;  // < total: u <= 1 - 2^-53
    int64_t lo = 0, hi = nb - 1;  // smallest b with B_{b+1} > t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (bincl[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    const double B = lo > 0 ? bincl[lo - 1] : 0.0;
    const int64_t end = (lo + 1) * kMcmcItems < n ? (lo + 1) * kMcmcItems : n;
    hi = end - 1;
    lo = lo * kMcmcItems;  // smallest i of the block with B + local_i > t
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (B + local[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    const int64_t row = alive ? (int64_t)alive[lo] : lo;
    if (row < 0 || row >= size) {
        sampled[j] = -1;
        atomicOr(&hdr->status, 2);
        return;
    }
    sampled[j] = (int)row;
    atomicAdd(&counts[row], 1);
}

void launch_mcmc_sample(int64_t n, const void* opacity_base, int64_t stride_bytes, const int* alive, int64_t num,
                        uint64_t seed, uint32_t stream_id, int* sampled, int* counts, int64_t size, void* scratch,
                        hipStream_t s)
{
    const McmcScratch m = carve_mcmc(scratch, n, nullptr);
    const int64_t nb = (n + kMcmcItems - 1) / kMcmcItems;
    if (nb > 0)
        hipLaunchKernelGGL(k_mcmc_scan_local, dim3((unsigned)nb), dim3(256), 0, s, n,
                           static_cast<const char*>(opacity_base), stride_bytes, alive, m.local, m.bincl);
    hipLaunchKernelGGL(k_mcmc_scan_blocks, dim3(1), dim3(64), 0, s, n, nb, m.bincl, m.hdr);
    if (num > 0)
        hipLaunchKernelGGL(k_mcmc_draw, dim3((unsigned)((num + 255) / 256)), dim3(256), 0, s, n, nb, alive, num, seed,
                           stream_id, m.bincl, m.local, m.hdr, sampled, counts, size);
}

// ---------------------------------------------------------------- position noise (train_post.py:868-878)
// One thread per resident Gaussian.  The reference composes, in float32 torch ops,
//   L = build_scaling_rotation(exp(scales), normalize(rotations));  cov = L @ L^T
//   noise = randn_like(means3D) * op_sigmoid(1 - sigmoid(opacity)) * MCMC_Noise_LR * xyz_lr;  means3D += cov @ noise
// with op_sigmoid(x) = 1 / (1 + exp(-100 (x - 0.995))).  Here the row's arithmetic runs in float64 from the float32
// inputs (the pass is bound by its 56 bytes per row, not by the ~150 float64 operations), so the only float32 rounding
// is that of the increment: the factor 100 amplifies the rounding of a float32 1 - o into w where w sits on its
// transition (opacity near 0.005), which is exactly where the noise matters.  cov @ v is formed as R (s^2 (R^T v)).
__global__ void __launch_bounds__(256) k_mcmc_noise(int64_t P, int64_t first_row, float* __restrict__ means,
                                                    const float* __restrict__ op_raw, const float* __restrict__ sc_raw,
                                                    const float* __restrict__ rot_raw, const float* __restrict__ noise,
                                                    double scale, uint64_t seed, uint32_t step)
{
    const int64_t p = first_row + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double o = 1.0 / (1.0 + exp(-(double)op_raw[p]));
    const double s0 = exp((double)sc_raw[3 * p]), s1 = exp((double)sc_raw[3 * p + 1]), s2 = exp((double)sc_raw[3 * p + 2]);
    double q0 = rot_raw[4 * p], q1 = rot_raw[4 * p + 1], q2 = rot_raw[4 * p + 2], q3 = rot_raw[4 * p + 3];
    // rotation_activation (normalize, eps 1e-12), then build_rotation's own division by the norm
    double d = fmax(sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3), 1e-12);
    q0 /= d, q1 /= d, q2 /= d, q3 /= d;
    d = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / d, x = q1 / d, y = q2 / d, z = q3 / d;
    const double R00 = 1.0 - 2.0 * (y * y + z * z), R01 = 2.0 * (x * y - r * z), R02 = 2.0 * (x * z + r * y);
    const double R10 = 2.0 * (x * y + r * z), R11 = 1.0 - 2.0 * (x * x + z * z), R12 = 2.0 * (y * z - r * x);
    const double R20 = 2.0 * (x * z - r * y), R21 = 2.0 * (y * z + r * x), R22 = 1.0 - 2.0 * (x * x + y * y);
    const double w = 1.0 / (1.0 + exp(-100.0 * ((1.0 - o) - 0.995)));
    const double f = w * scale;
    float n0, n1, n2;
    if (noise) {
        n0 = noise[3 * p], n1 = noise[3 * p + 1], n2 = noise[3 * p + 2];
    } else {
        n0 = rng_normal(seed, step, 3 * (uint64_t)p);
        n1 = rng_normal(seed, step, 3 * (uint64_t)p + 1);
        n2 = rng_normal(seed, step, 3 * (uint64_t)p + 2);
    }
    const double v0 = n0 * f, v1 = n1 * f, v2 = n2 * f;
    const double a0 = s0 * s0 * (R00 * v0 + R10 * v1 + R20 * v2);
    const double a1 = s1 * s1 * (R01 * v0 + R11 * v1 + R21 * v2);
    const double a2 = s2 * s2 * (R02 * v0 + R12 * v1 + R22 * v2);
    means[3 * p] += (float)(R00 * a0 + R01 * a1 + R02 * a2);
    means[3 * p + 1] += (float)(R10 * a0 + R11 * a1 + R12 * a2);
    means[3 * p + 2] += (float)(R20 * a0 + R21 * a1 + R22 * a2);
}

void launch_mcmc_noise(int64_t P, int64_t first_row, float* means, const float* op_raw, const float* sc_raw,
                       const float* rot_raw, const float* noise, double scale, uint64_t seed, uint32_t step,
                       hipStream_t s)
{
    const int64_t rows = P - first_row;
    if (rows <= 0) return;
    hipLaunchKernelGGL(k_mcmc_noise, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, P, first_row, means, op_raw,
                       sc_raw, rot_raw, noise, scale, seed, step);
}

// ---------------------------------------------------------------- hlgs_rng_fill
__global__ void __launch_bounds__(256) k_rng_fill(int kind, uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n,
                                                  void* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (kind == HLGS_RNG_UNIFORM64) static_cast<double*>(out)[i] = rng_uniform53(seed, stream_id, first + (uint64_t)i);
    else static_cast<float*>(out)[i] = rng_normal(seed, stream_id, first + (uint64_t)i);
}

void launch_rng_fill(int kind, uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, void* out, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_rng_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kind, seed, stream_id, first, n,
                       out);
}

}  // namespace hlgs
