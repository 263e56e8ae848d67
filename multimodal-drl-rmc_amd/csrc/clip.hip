// Gradient clipping (include/dqnx.h "gradient clipping"): the two launches a clipped learn step runs
// between the launch that leaves the whole gradient in DQNX_BUF_GRADS and the Adam pass that reads it.
//
//   k_grad_sumsq  workgroup b: sum of g^2 over elements [b chunk, min(P, (b + 1) chunk)) -> part[b]
//   k_clip_coef   one workgroup: part[0 .. n_part) in index order -> total_norm, the coefficient
//                 min(max_norm / (total_norm + 1e-6), 1) of torch.nn.utils.clip_grad_norm_, the info block
//
// The Adam pass (k_adam / k_adam4 mode 2, k_dw_adam16 mode 3) multiplies every gradient element by the
// one float k_clip_coef stored: the same bits for every element of the step.  The launch boundaries are
// the only synchronisation: no ticket, no flag, no atomics.
//
// Determinism: the square of an fp32 is exact in fp64 and every sum is fp64 from the first add, in a
// place fixed by the launch geometry: a lane adds its elements in index order, the 64 lanes of a wave
// fold by shuffles (a fixed tree), the 4 waves in wave order through LDS; k_clip_coef's lane t adds
// partials t, t + 256, ... in order and the workgroup folds the same way.
#include <math.h>

#include <algorithm>

#include "common.hpp"
#include "learn.hpp"

namespace dqnx {

namespace {

// the workgroup's sum in thread 0 (the other threads' return values are partial sums)
__device__ __forceinline__ double clip_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, kWave);
    const int tid = threadIdx.x;
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < kClipThreads / kWave; w++) v += sh[w];
    return v;
}

}  // namespace

__global__ __launch_bounds__(kClipThreads) void k_grad_sumsq(ClipArgs a) {
    __shared__ double sh[kClipThreads / kWave];
    const int tid = threadIdx.x;
    // chunk is a multiple of 4 and the gradient's base 16-byte aligned: b is a 16-byte boundary
    const int64_t b = (int64_t)blockIdx.x * a.chunk;
    const int64_t e = min(a.n_params, b + a.chunk);
    const int64_t v1 = max(b, e & ~(int64_t)3);   // [b, v1) 16 bytes per lane, [v1, e) scalar tail
    double s = 0.0;
#pragma unroll 4
    for (int64_t i = b + 4 * tid; i < v1; i += 4 * kClipThreads) {
        const float4 g = ld4(a.grads + i);
        s += (double)g.x * (double)g.x;
        s += (double)g.y * (double)g.y;
        s += (double)g.z * (double)g.z;
        s += (double)g.w * (double)g.w;
    }
    if (tid < (int)(e - v1)) {   // <= 3 elements, only in the last workgroup
        const float g = a.grads[v1 + tid];
        s += (double)g * (double)g;
    }
    s = clip_block_sum(s, sh);
    if (tid == 0) a.part[blockIdx.x] = s;
}

__global__ __launch_bounds__(kClipThreads) void k_clip_coef(ClipArgs a) {
    __shared__ double sh[kClipThreads / kWave];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int j = tid; j < a.n_part; j += kClipThreads) s += a.part[j];
    s = clip_block_sum(s, sh);
    if (tid != 0) return;
    const double norm = sqrt(s);
    const float nf = (float)norm;
    // clip_coef = max_norm / (total_norm + 1e-6); clamp(clip_coef, max=1.0), all in fp32: ONE correctly
    // rounded division, the formula of include/dqnx.h.  torch forms `float / tensor` as
    // tensor.reciprocal() * float (Tensor.__rdiv__), two roundings, so its coefficient may differ from
    // this one in the last bit
    const float c = a.max_norm / (nf + 1e-6f);
    const float coef = c > 1.0f ? 1.0f : c;   // (a NaN stays a NaN, as torch.clamp leaves it)
    *a.coef = coef;
    dqnx_grad_clip_info* o = a.info;
    const bool first = o->steps == 0;   // a zeroed block is the valid empty state
    o->steps += 1;
    o->clipped_steps += coef < 1.0f ? 1 : 0;
    o->norm_sum += norm;
    o->norm_max = first ? norm : fmax(o->norm_max, norm);
    o->last_norm = nf;
    o->last_coef = coef;
}

void clip_geometry(int64_t n_params, int64_t* chunk, int* n_part) {
    int64_t c = kClipMinChunk;
    while ((n_params + c - 1) / c > kClipMaxParts) c *= 2;
    *chunk = c;
    *n_part = (int)std::max<int64_t>(1, (n_params + c - 1) / c);
}

static int clip_args_ok(const ClipArgs& a) {
    if (!a.grads || !a.part || !a.coef || !a.info) return set_error(DQNX_EINVAL, "grad clip: null buffer");
    if (a.n_params < 1 || a.chunk < 4 || a.chunk % 4 || a.n_part < 1 ||
        (int64_t)a.n_part != (a.n_params + a.chunk - 1) / a.chunk)
        return set_error(DQNX_EINVAL, "grad clip: the partials do not cover the gradient");
    if (((uintptr_t)a.grads & 15) || ((uintptr_t)a.part & 7) || ((uintptr_t)a.info & 7) || ((uintptr_t)a.coef & 3))
        return set_error(DQNX_EINVAL, "grad clip: misaligned buffer");
    return DQNX_OK;
}

int launch_grad_sumsq(const ClipArgs& a, hipStream_t s) {
    const int rc = clip_args_ok(a);
    if (rc) return rc;
    DQNX_LAUNCH(k_grad_sumsq, dim3((unsigned)a.n_part), dim3(kClipThreads), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_clip_coef(const ClipArgs& a, hipStream_t s) {
    const int rc = clip_args_ok(a);
    if (rc) return rc;
    DQNX_LAUNCH(k_clip_coef, dim3(1), dim3(kClipThreads), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
