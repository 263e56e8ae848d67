// Acting path for networks whose working set does not fit a workgroup's LDS (DQNX_ACT_LARGE, engine.cpp
// act_plan_build): a conv input image over 64 KB -- the (4,84,84) variant of the two-stream net -- or a
// first dense layer too wide for the MLP acting kernel's two LDS rows (more than 8192 inputs: that
// variant's 56,462-wide dense 1, 115.6 MB of fp32 weights).
//
//   k_act_conv_band    one launch per conv: a workgroup takes one row of the call, a tile of output pixels
//                      (a band of BH output rows x TW columns) and 8 output channels; it stages the input
//                      rows the band needs, zero-padded, a slice of the input channels at a time, and keeps
//                      the 8 sums of its pixel in registers across the slices (ci ascending: fixed order)
//   k_act_dense_wide   dense 1 as a weight-streaming split-K GEMV for a chunk of up to 8 rows: grid =
//                      (tiles of 16 neurons) x (S slices of K); weights go straight to registers, 16 bytes a
//                      lane, each element loaded once and used for every row; partials to scratch [S][nr][J]
//   k_act_wide_reduce  at the kernel boundary: h1[r][j] = act(sum of the S shares in slice order + b[j])
//   k_act_large_head   nets with ONE dense layer: the head (advantage stream for dueling nets) and the
//                      first-max argmax on h1; deeper nets run layers 2..L through the MLP acting kernel
//                      (act.hip) with h1 as its input
// All sums are fp32 fmaf chains in a fixed order (no float atomics): a call repeats bitwise.
#include <algorithm>

#include "common.hpp"
#include "learn.hpp"

namespace dqnx {

namespace {

constexpr int kBandThreads = 256;
constexpr int kBandCG = 8;                    // output channels a thread accumulates
constexpr size_t kBandLds = 32 * 1024;        // staging budget: several workgroups per CU
constexpr int kWideThreads = 256;
constexpr int kWideWaves = kWideThreads / kWave;
constexpr int kWideJT = 16;                   // neurons per workgroup (4 per wave, one after the other)
constexpr int kWideLs = 1024;                 // K slice length (floats) at most
constexpr int kWideP = 4;                     // 16-byte loads of a weight row in flight per lane

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}

// KH x KW > 0: that window at compile time (taps unrolled); 0 x 0: any window
template <int ACT, int KH, int KW>
__global__ __launch_bounds__(kBandThreads) void k_act_conv_band(ActConvArgs a, ActBandPlan pl) {
    extern __shared__ float lds[];
    const int tid = threadIdx.x;
    const int kh = KH > 0 ? KH : a.kh, kw = KW > 0 ? KW : a.kw, khw = kh * kw;
    const int K = a.Ci * khw, P = a.Ho * a.Wo;
    const int tilesW = (a.Wo + pl.TW - 1) / pl.TW;
    const int tb = blockIdx.x / tilesW, tw = blockIdx.x - tb * tilesW;
    const int ho0 = tb * pl.BH, wo0 = tw * pl.TW;
    const int c0 = blockIdx.y * kBandCG, r = blockIdx.z;
    const int in_rows = (pl.BH - 1) * a.sh + kh, in_cols = (pl.TW - 1) * a.sw + kw;
    const int tile = in_rows * in_cols;
    float* x = lds;                                   // [CiC][in_rows][in_cols], zero outside the image
    float* w = lds + ((pl.CiC * tile + 3) & ~3);      // [CiC][khw][8]
    const int lr = tid / pl.TW, lc = tid - lr * pl.TW;
    const bool in_tile = lr < pl.BH;
    const bool live = in_tile && ho0 + lr < a.Ho && wo0 + lc < a.Wo;
    const int xoff = in_tile ? lr * a.sh * in_cols + lc * a.sw : 0;   // (idle threads read pixel 0, result dropped)
    const float* src = a.in + (int64_t)r * a.in_stride + a.in_off;
    const int h_base = ho0 * a.sh - a.ph, w_base = wo0 * a.sw - a.pw;
    float acc[kBandCG];
#pragma unroll
    for (int u = 0; u < kBandCG; u++) acc[u] = 0.f;
    for (int cb = 0; cb < a.Ci; cb += pl.CiC) {
        const int cn = min(pl.CiC, a.Ci - cb);
        if (cb) __syncthreads();   // the previous slice has been read
        for (int i = tid; i < cn * tile; i += kBandThreads) {
            const int ci = i / tile, t = i - ci * tile, ir = t / in_cols, ic = t - ir * in_cols;
            const int h = h_base + ir, ww = w_base + ic;
            const bool ok = h >= 0 && h < a.Hi && ww >= 0 && ww < a.Wi;
            x[i] = ok ? src[((int64_t)(cb + ci) * a.Hi + h) * a.Wi + ww] : 0.f;
        }
        const int wn = cn * khw;   // a channel's weights of this slice are contiguous in memory
        for (int i = tid; i < wn * kBandCG; i += kBandThreads) {
            const int u = i / wn, t = i - u * wn, c = c0 + u;
            w[t * kBandCG + u] = c < a.Co ? a.W[(int64_t)c * K + (int64_t)cb * khw + t] : 0.f;
        }
        __syncthreads();
        for (int ci = 0; ci < cn; ci++) {
            const float* xc = x + ci * tile + xoff;
            const float* wc = w + ci * khw * kBandCG;
            auto tap = [&](int i, int j) {
                const float xv = xc[i * in_cols + j];
                const float4 w0 = *reinterpret_cast<const float4*>(wc + (i * kw + j) * kBandCG);
                const float4 w1 = *reinterpret_cast<const float4*>(wc + (i * kw + j) * kBandCG + 4);
                acc[0] = fmaf(xv, w0.x, acc[0]); acc[1] = fmaf(xv, w0.y, acc[1]);
                acc[2] = fmaf(xv, w0.z, acc[2]); acc[3] = fmaf(xv, w0.w, acc[3]);
                acc[4] = fmaf(xv, w1.x, acc[4]); acc[5] = fmaf(xv, w1.y, acc[5]);
                acc[6] = fmaf(xv, w1.z, acc[6]); acc[7] = fmaf(xv, w1.w, acc[7]);
            };
            if constexpr (KH > 0) {
#pragma unroll
                for (int i = 0; i < KH; i++)
#pragma unroll
                    for (int j = 0; j < KW; j++) tap(i, j);
            } else {
                for (int i = 0; i < kh; i++)
                    for (int j = 0; j < kw; j++) tap(i, j);
            }
        }
    }
    if (live) {
        float* o = a.out + (int64_t)r * a.out_stride + a.out_off + (int64_t)(ho0 + lr) * a.Wo + wo0 + lc;
#pragma unroll
        for (int u = 0; u < kBandCG; u++)
            if (c0 + u < a.Co) o[(int64_t)(c0 + u) * P] = act_fwd<ACT>(acc[u] + a.b[c0 + u]);
    }
    if (a.macro && blockIdx.x == 0 && blockIdx.y == 0)   // the dense input's macro tail: F[r][Co*P ..]
        for (int i = tid; i < a.macro_len; i += kBandThreads)
            a.out[(int64_t)r * a.out_stride + a.out_off + (int64_t)a.Co * P + i] = a.macro[(int64_t)r * a.macro_stride + i];
}

// One K slice of kWideJT weight rows against the chunk's R rows (rows >= nr are zero and not stored).
// A weight row starts wherever j * K lands: each row is peeled to its own 16-byte boundary (scalar loads
// for up to 3 elements at either end of the slice), so every load stays inside the row's slice.
template <int R>
__global__ __launch_bounds__(kWideThreads) void k_act_dense_wide(ActWideArgs a) {
    extern __shared__ float xs[];   // [R][Ls]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int s = blockIdx.y, Ls = a.Ls;
    const int k0 = min(a.K, s * Ls), k1 = min(a.K, k0 + Ls), len = k1 - k0;
    for (int i = tid; i < R * Ls; i += kWideThreads) {
        const int r = i / Ls, k = i - r * Ls;
        xs[i] = (r < a.nr && k < len) ? a.x[(int64_t)r * a.x_stride + k0 + k] : 0.f;
    }
    __syncthreads();
    for (int jj = wave; jj < kWideJT; jj += kWideWaves) {
        const int j = blockIdx.x * kWideJT + jj;
        if (j >= a.J) break;   // (wave-uniform)
        const float* w = a.W + (int64_t)j * a.K + k0;
        const int pa = min(len, (int)((4 - (((uintptr_t)w >> 2) & 3)) & 3));   // elements before the boundary
        const int nv = (len - pa) >> 2, tl = len - pa - 4 * nv;                // float4s, elements after them
        float acc[R];
#pragma unroll
        for (int r = 0; r < R; r++) acc[r] = 0.f;
        {
            int k = -1;
            if (lane < pa) k = lane;
            else if (lane >= 4 && lane < 4 + tl) k = pa + 4 * nv + lane - 4;
            if (k >= 0) {
                const float wv = gld(w + k);
#pragma unroll
                for (int r = 0; r < R; r++) acc[r] = fmaf(wv, xs[r * Ls + k], acc[r]);
            }
        }
        const floatx4* wb = reinterpret_cast<const floatx4*>(w + pa);
        const float* xb = xs + pa;
        for (int v0 = lane; v0 < nv; v0 += kWideP * kWave) {
            floatx4 wv[kWideP];
#pragma unroll
            for (int p = 0; p < kWideP; p++) {
                const int v = v0 + p * kWave;
                wv[p] = v < nv ? gld(wb + v) : floatx4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int p = 0; p < kWideP; p++) {
                const int v = min(v0 + p * kWave, nv - 1);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float* xr = xb + r * Ls + 4 * v;   // (4-byte aligned only when the row was peeled)
                    acc[r] = fmaf(wv[p].x, xr[0], acc[r]);
                    acc[r] = fmaf(wv[p].y, xr[1], acc[r]);
                    acc[r] = fmaf(wv[p].z, xr[2], acc[r]);
                    acc[r] = fmaf(wv[p].w, xr[3], acc[r]);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float sum = wave_sum(acc[r]);
            if (lane == r && r < a.nr) a.part[((int64_t)s * a.nr + r) * a.J + j] = sum;
        }
    }
}

template <int ACT>
__global__ __launch_bounds__(256) void k_act_wide_reduce(ActWideArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nr * a.J) return;
    const int j = i % a.J;
    const int64_t stride = (int64_t)a.nr * a.J;
    float z = 0.f;
    constexpr int U = 8;   // shares requested together
    for (int s0 = 0; s0 < a.S; s0 += U) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) v[u] = gld(a.part + (int64_t)min(s0 + u, a.S - 1) * stride + i);
#pragma unroll
        for (int u = 0; u < U; u++)
            if (s0 + u < a.S) z += v[u];
    }
    a.h[i] = act_fwd<ACT>(z + a.b[j]);
}

// One workgroup per row: head output j on wave j % 4 (lanes stride the F inputs, butterfly sum), then the
// first-max argmax on one thread (NaN wins, like torch)
__global__ __launch_bounds__(256) void k_act_large_head(ActArgs a) {
    extern __shared__ float q[];   // [A]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int r = blockIdx.x, F = a.F, A = a.A;
    const float* H = a.params + a.head_off;
    const float* Wh = a.dueling ? H + F + 1 : H;   // advantage stream (R:dqn/network.py:110-117)
    const float* x = a.obs + (int64_t)r * F;
    for (int j = wave; j < A; j += 4) {
        const float* wr = Wh + (int64_t)j * F;
        float acc = 0.f;
        for (int k = lane; k < F; k += kWave) acc = fmaf(wr[k], x[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) q[j] = acc + Wh[(int64_t)A * F + j];
    }
    __syncthreads();
    if (tid == 0) {
        int best = 0;
        float bv = q[0];
        for (int j = 0; j < A; j++) {
            const float v = q[j];
            if (a.values) a.values[(int64_t)r * A + j] = v;
            if (v > bv || (v != v && bv == bv)) { bv = v; best = j; }
        }
        a.actions[r] = best;
    }
}

}  // namespace

bool act_band_plan(const ActConvArgs& a, ActBandPlan& p) {
    if (a.Wo < 1 || a.Ho < 1 || a.kh < 1 || a.kw < 1 || a.Ci < 1) return false;
    p.TW = std::min(a.Wo, kBandThreads);
    p.BH = std::max(1, std::min(kBandThreads / p.TW, a.Ho));
    const int khw = a.kh * a.kw;
    for (;;) {
        const int64_t tile = (int64_t)((p.BH - 1) * a.sh + a.kh) * ((p.TW - 1) * a.sw + a.kw);
        const int64_t per = tile + (int64_t)khw * kBandCG;   // floats per input channel staged
        const int64_t fit = ((int64_t)kBandLds / 4 - 4) / per;
        if (fit >= 1) {
            p.CiC = (int)std::min<int64_t>(fit, a.Ci);
            p.lds = (size_t)((((int64_t)p.CiC * tile + 3) & ~(int64_t)3) + (int64_t)p.CiC * khw * kBandCG) * 4;
            return true;
        }
        if (p.BH > 1) p.BH = (p.BH + 1) / 2;
        else if (p.TW > 1) p.TW = (p.TW + 1) / 2;
        else return false;
    }
}

int launch_act_conv_band(const ActConvArgs& a, int act, hipStream_t s) {
    if (a.n <= 0) return DQNX_OK;
    ActBandPlan p;
    if (!act_band_plan(a, p))
        return set_error(DQNX_EUNSUPPORTED, "dqnx_act: conv window %dx%d too large for the banded acting kernel", a.kh, a.kw);
    const int tiles = ((a.Wo + p.TW - 1) / p.TW) * ((a.Ho + p.BH - 1) / p.BH);
    const dim3 grid(tiles, (a.Co + kBandCG - 1) / kBandCG, a.n);
    const bool k33 = a.kh == 3 && a.kw == 3;   // (the reference's convs)
    if (act == DQNX_ACT_RELU) {
        if (k33) DQNX_LAUNCH((k_act_conv_band<DQNX_ACT_RELU, 3, 3>), grid, dim3(kBandThreads), p.lds, s, a, p);
        else DQNX_LAUNCH((k_act_conv_band<DQNX_ACT_RELU, 0, 0>), grid, dim3(kBandThreads), p.lds, s, a, p);
    } else {
        if (k33) DQNX_LAUNCH((k_act_conv_band<DQNX_ACT_ELU, 3, 3>), grid, dim3(kBandThreads), p.lds, s, a, p);
        else DQNX_LAUNCH((k_act_conv_band<DQNX_ACT_ELU, 0, 0>), grid, dim3(kBandThreads), p.lds, s, a, p);
    }
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

// S slices of at most kWideLs floats, even lengths rounded up to whole float4s (the same for every n)
void act_wide_slices(int K, int* S, int* Ls) {
    const int s = std::max(1, (K + kWideLs - 1) / kWideLs);
    *S = s;
    *Ls = ((K + s - 1) / s + 3) & ~3;
}

int launch_act_dense_wide(const ActWideArgs& a0, hipStream_t s) {
    if (a0.nr <= 0) return DQNX_OK;
    if (a0.nr > kActWideRows) return set_error(DQNX_EINVAL, "dqnx_act: more than %d rows in a chunk", kActWideRows);
    ActWideArgs a = a0;
    act_wide_slices(a.K, &a.S, &a.Ls);
    const dim3 grid((a.J + kWideJT - 1) / kWideJT, a.S);
    const int R = a.nr <= 1 ? 1 : (a.nr == 2 ? 2 : (a.nr <= 4 ? 4 : 8));
    const size_t lds = (size_t)R * a.Ls * sizeof(float);
    switch (R) {
        case 1: DQNX_LAUNCH(k_act_dense_wide<1>, grid, dim3(kWideThreads), lds, s, a); break;
        case 2: DQNX_LAUNCH(k_act_dense_wide<2>, grid, dim3(kWideThreads), lds, s, a); break;
        case 4: DQNX_LAUNCH(k_act_dense_wide<4>, grid, dim3(kWideThreads), lds, s, a); break;
        default: DQNX_LAUNCH(k_act_dense_wide<8>, grid, dim3(kWideThreads), lds, s, a); break;
    }
    DQNX_HIP_CHECK(hipGetLastError());
    const dim3 rg((a.nr * a.J + 255) / 256);
    if (a.act == DQNX_ACT_RELU) DQNX_LAUNCH(k_act_wide_reduce<DQNX_ACT_RELU>, rg, dim3(256), 0, s, a);
    else DQNX_LAUNCH(k_act_wide_reduce<DQNX_ACT_ELU>, rg, dim3(256), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_act_large_head(const ActArgs& a, hipStream_t s) {
    if (a.n <= 0) return DQNX_OK;
    DQNX_LAUNCH(k_act_large_head, dim3(a.n), dim3(256), (size_t)a.A * sizeof(float), s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
