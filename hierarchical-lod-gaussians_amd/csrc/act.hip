// act.hip -- the parameter activations of the training step in one pass over the resident rows.
//
// Reference semantics (scene/gaussian_model.py:44-56, get_opacity / get_scaling / get_rotation, read by render() at
// gaussian_renderer/__init__.py and train_post.py's render_post): opacity = sigmoid(_opacity), scales =
// exp(_scaling), rotations = torch.nn.functional.normalize(_rotation) (eps 1e-12).  train_post.py applies them to
// every resident row each step, and torch runs each as its own elementwise kernel (sigmoid, exp, the norm reduction,
// clamp_min, the division) forward and again backward (sigmoid_backward, the exp product, and the division / norm
// chain).  Here one thread per Gaussian row reads its three raw rows once and writes the three activated rows; the
// backward reads the upstream gradients and writes the raw-parameter gradients in one pass as well.
//
// Operation order follows torch's kernels: sigmoid(x) = 1 / (1 + exp(-x)); its gradient (g (1 - y)) y; exp's gradient
// g y; normalize = x / max(||x||, eps), whose gradient through the division and the norm is
// g / d - x (sum_j g_j x_j) / d^2 / ||x|| (the second term only while ||x|| > eps, where clamp_min passes it).
//
// The regularised variants (k_act_reg_fwd / k_act_reg_bwd) fold the two MCMC regularisers of train_post.py:565-576 into
// the same pass: opacity_loss = sum |sigmoid(o)| / n and scaling_loss = sum |exp(s)| / n over the n rows passed in.
// The forward reduces both sums over its workgroup as loss.hip does (shuffles over the 64 lanes, then the four waves
// through LDS) into two float partials per workgroup, which k_reduce_partials (loss.hip) adds in double in index order:
// no float atomics, so the losses do not change from run to run.  The backward adds the losses' upstream gradients
// (two floats on the device, never read on the host) to the activated rows' gradients before the chain rule, the order
// in which torch accumulates them.  The plain kernels are what they were.
#include "hlgs_internal.h"

namespace hlgs {

__global__ void __launch_bounds__(256) k_act_fwd(int64_t n, const float* __restrict__ op_raw,
                                                 const float* __restrict__ sc_raw, const float4* __restrict__ rot_raw,
                                                 float* __restrict__ op, float* __restrict__ sc,
                                                 float4* __restrict__ rot)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float o = op_raw[i];
    const float s0 = sc_raw[3 * i], s1 = sc_raw[3 * i + 1], s2 = sc_raw[3 * i + 2];
    const float4 q = rot_raw[i];
    op[i] = 1.0f / (1.0f + expf(-o));
    sc[3 * i] = expf(s0);
    sc[3 * i + 1] = expf(s1);
    sc[3 * i + 2] = expf(s2);
    const float d = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
    rot[i] = make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
}

__global__ void __launch_bounds__(256) k_act_bwd(int64_t n, const float* __restrict__ op, const float* __restrict__ sc,
                                                 const float4* __restrict__ rot_raw, const float* __restrict__ g_op,
                                                 const float* __restrict__ g_sc, const float4* __restrict__ g_rot,
                                                 float* __restrict__ d_op, float* __restrict__ d_sc,
                                                 float4* __restrict__ d_rot)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (g_op) {
        const float y = op[i];
        d_op[i] = (g_op[i] * (1.0f - y)) * y;
    }
    if (g_sc) {
#pragma unroll
        for (int k = 0; k < 3; k++) d_sc[3 * i + k] = g_sc[3 * i + k] * sc[3 * i + k];
    }
    if (g_rot) {
        const float4 x = rot_raw[i], g = g_rot[i];
        const float nrm = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
        const float d = fmaxf(nrm, 1e-12f);
        float4 r = make_float4(g.x / d, g.y / d, g.z / d, g.w / d);
        if (nrm > 1e-12f) {
            const float gd = -(g.x * x.x + g.y * x.y + g.z * x.z + g.w * x.w) / (d * d);  // dL/dd
            const float c = gd / nrm;                                                        // d||x||/dx = x / ||x||
            r.x += c * x.x;
            r.y += c * x.y;
            r.z += c * x.z;
            r.w += c * x.w;
        }
        d_rot[i] = r;
    }
}

// k_act_fwd with the regularisers' sums.  sigmoid and exp are positive, so the |.| of the reference's opacity_loss and
// scaling_loss is the identity and the activated values are summed as they are.  The per-row arithmetic is k_act_fwd's
// (the three outputs are bit-identical); rows past n add 0.  partial[2 * block] = (sum of op, sum of sc) of the block.
__global__ void __launch_bounds__(256) k_act_reg_fwd(int64_t n, const float* __restrict__ op_raw,
                                                     const float* __restrict__ sc_raw,
                                                     const float4* __restrict__ rot_raw, float* __restrict__ op,
                                                     float* __restrict__ sc, float4* __restrict__ rot,
                                                     float* __restrict__ partial)
{
#pragma clang fp contract(off)
    __shared__ float red[2][4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float s_op = 0.f, s_sc = 0.f;
    if (i < n) {
        const float o = op_raw[i];
        const float s0 = sc_raw[3 * i], s1 = sc_raw[3 * i + 1], s2 = sc_raw[3 * i + 2];
        const float4 q = rot_raw[i];
        const float y = 1.0f / (1.0f + expf(-o));
        const float e0 = expf(s0), e1 = expf(s1), e2 = expf(s2);
        op[i] = y;
        sc[3 * i] = e0;
        sc[3 * i + 1] = e1;
        sc[3 * i + 2] = e2;
        const float d = fmaxf(sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w), 1e-12f);
        rot[i] = make_float4(q.x / d, q.y / d, q.z / d, q.w / d);
        s_op = y;
        s_sc = (e0 + e1) + e2;
    }
    // workgroup sums (fixed order: shuffles, then one lane per wave)
    for (int off = 32; off > 0; off >>= 1) {
        s_op += __shfl_xor(s_op, off, 64);
        s_sc += __shfl_xor(s_sc, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s_op;
        red[1][threadIdx.x >> 6] = s_sc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        partial[2 * (size_t)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// k_act_bwd with the regularisers' gradients: g_reg (device, 2 floats) holds dL/d opacity_loss and dL/d scaling_loss,
// and every activated opacity / scale receives g_reg / n beside its own upstream gradient (a NULL g_op or g_sc counts
// as 0).  The rotation is k_act_bwd's.
__global__ void __launch_bounds__(256) k_act_reg_bwd(int64_t n, const float* __restrict__ op,
                                                     const float* __restrict__ sc, const float4* __restrict__ rot_raw,
                                                     const float* __restrict__ g_op, const float* __restrict__ g_sc,
                                                     const float4* __restrict__ g_rot, const float* __restrict__ g_reg,
                                                     float* __restrict__ d_op, float* __restrict__ d_sc,
                                                     float4* __restrict__ d_rot)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float c_o = g_reg[0] / (float)n, c_s = g_reg[1] / (float)n;
    {
        const float y = op[i];
        const float g = g_op ? g_op[i] + c_o : c_o;
        d_op[i] = (g * (1.0f - y)) * y;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float g = g_sc ? g_sc[3 * i + k] + c_s : c_s;
        d_sc[3 * i + k] = g * sc[3 * i + k];
    }
    if (g_rot) {
        const float4 x = rot_raw[i], g = g_rot[i];
        const float nrm = sqrtf(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w);
        const float d = fmaxf(nrm, 1e-12f);
        float4 r = make_float4(g.x / d, g.y / d, g.z / d, g.w / d);
        if (nrm > 1e-12f) {
            const float gd = -(g.x * x.x + g.y * x.y + g.z * x.z + g.w * x.w) / (d * d);  // dL/dd
            const float c = gd / nrm;                                                        // d||x||/dx = x / ||x||
            r.x += c * x.x;
            r.y += c * x.y;
            r.z += c * x.z;
            r.w += c * x.w;
        }
        d_rot[i] = r;
    }
}

void launch_act_fwd(int64_t n, const float* op_raw, const float* sc_raw, const float* rot_raw, float* op, float* sc,
                    float* rot, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_act_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, op_raw, sc_raw,
                       reinterpret_cast<const float4*>(rot_raw), op, sc, reinterpret_cast<float4*>(rot));
}

void launch_act_bwd(int64_t n, const float* op, const float* sc, const float* rot_raw, const float* g_op,
                    const float* g_sc, const float* g_rot, float* d_op, float* d_sc, float* d_rot, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_act_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, op, sc,
                       reinterpret_cast<const float4*>(rot_raw), g_op, g_sc, reinterpret_cast<const float4*>(g_rot),
                       d_op, d_sc, reinterpret_cast<float4*>(d_rot));
}

int64_t act_reg_blocks(int64_t n) { return (n + 255) / 256; }

void launch_act_reg_fwd(int64_t n, const float* op_raw, const float* sc_raw, const float* rot_raw, float* op, float* sc,
                        float* rot, float* reg, float* partial, hipStream_t s)
{
    if (n <= 0) return;
    const int64_t nb = act_reg_blocks(n);
    hipLaunchKernelGGL(k_act_reg_fwd, dim3((unsigned)nb), dim3(256), 0, s, n, op_raw, sc_raw,
                       reinterpret_cast<const float4*>(rot_raw), op, sc, reinterpret_cast<float4*>(rot), partial);
    launch_reduce_partials((int)nb, 2, partial, 1.0 / (double)n, 1.0 / (double)n, reg, s);
}

void launch_act_reg_bwd(int64_t n, const float* op, const float* sc, const float* rot_raw, const float* g_op,
                        const float* g_sc, const float* g_rot, const float* g_reg, float* d_op, float* d_sc,
                        float* d_rot, hipStream_t s)
{
    if (n <= 0) return;
    if (!g_reg) {  // no regulariser reaches the loss: the plain backward
        launch_act_bwd(n, op, sc, rot_raw, g_op, g_sc, g_rot, d_op, d_sc, d_rot, s);
        return;
    }
    hipLaunchKernelGGL(k_act_reg_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, op, sc,
                       reinterpret_cast<const float4*>(rot_raw), g_op, g_sc, reinterpret_cast<const float4*>(g_rot),
                       g_reg, d_op, d_sc, reinterpret_cast<float4*>(d_rot));
}

}  // namespace hlgs
