// hlgs_rng.h -- the counter-based random numbers of the MCMC kernels (mcmc.hip): Philox4x32-10 (Salmon et al.,
// "Parallel random numbers: as easy as 1, 2, 3", SC'11), host and device.
//
// Number `index` of (seed, stream) is a pure function of those three 64/32-bit values: there is no state tensor, the
// launch shape does not enter, and every rank of a view-data-parallel run draws the same numbers from the same seed.
//   counter = (index & 0xffffffff, index >> 32, stream, 0)      key = (seed & 0xffffffff, seed >> 32)
// One Philox call yields four 32-bit words w0..w3:
//   uniform (sampling)   u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53, a 53-bit double in [0, 1).  (A 24-bit float
//                        uniform can select at most 2^24 distinct candidates; Max_Cap is 50M.)
//   normal  (noise)      Box-Muller on the other two words, the cosine branch only:
//                        u1 = ((w2 >> 8) + 1) * 2^-24  in (0, 1]  (so log(u1) is finite: |z| <= sqrt(2 ln 2^24) = 5.77)
//                        u2 = (w3 >> 8) * 2^-24        in [0, 1)
//                        z  = sqrtf(-2 logf(u1)) * cosf(2 pi u2)
// so uniform `index` and normal `index` of one (seed, stream) come from the same Philox block and never share a word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hlgs {

struct Philox4 {
    uint32_t w[4];
};

__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__host__ __device__ inline Philox4 rng_words(uint64_t seed, uint32_t stream, uint64_t index)
{
    return philox4x32_10((uint32_t)index, (uint32_t)(index >> 32), stream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

__host__ __device__ inline double rng_uniform53(uint64_t seed, uint32_t stream, uint64_t index)
{
    const Philox4 p = rng_words(seed, stream, index);
    const uint64_t m = ((uint64_t)(p.w[0] >> 5) << 26) | (uint64_t)(p.w[1] >> 6);
    return (double)m * (1.0 / 9007199254740992.0);
}

__host__ __device__ inline float rng_normal(uint64_t seed, uint32_t stream, uint64_t index)
{
    const Philox4 p = rng_words(seed, stream, index);
    const float u1 = (float)((p.w[2] >> 8) + 1u) * (1.0f / 16777216.0f);
    const float u2 = (float)(p.w[3] >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace hlgs
