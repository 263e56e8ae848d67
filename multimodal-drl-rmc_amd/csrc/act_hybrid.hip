// Acting path of the two-stream network (TwoStreamHybridNetwork, R:env/dqn_config.py:66-143):
// Network.actions (DuelingDeepQNetwork R:dqn/network.py:110-117: argmax of the advantage stream;
// DeepQNetwork :67-74: argmax of Q) at n_env rows, called by Agent.choose_actions
// (R:dqn/agent.py:92-99) every env step.
//
// Per row the body is 3 small convs (2 -> 32 -> 64 -> 64 channels on the 2x27x5 micro grid) and
// a 1358 -> 512 -> 256 dense stream: ~6 MFLOP and 3.5 MB of weights, so the time is set by the
// number of dependent round trips, not by FLOPs.  Two routes (engine.cpp, act_ts_plan): the whole conv
// stack as one launch (k_act_conv_stack, second half of this file), or one launch per conv, each a grid of
// (output channel x row) workgroups that stage the row's input image and the channel's weights
// in LDS and split every output pixel's K = Ci*kh*kw sum over as many threads as fit (fixed-order
// reduction); conv 3 writes its CHW output straight into the dense input F = cat(flatten(conv3),
// macro) (R:env/dqn_config.py:135-138).  The dense stream and the head are then the MLP acting
// kernel (act.hip) on F.
#include "common.hpp"
#include "learn.hpp"

namespace dqnx {

namespace {

constexpr int kConvThreads = 256;

__global__ __launch_bounds__(kConvThreads) void k_act_conv(ActConvArgs a) {
    extern __shared__ float lds[];
    const int c = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int HWi = a.Hi * a.Wi, img = a.Ci * HWi, K = a.Ci * a.kh * a.kw, P = a.Ho * a.Wo;
    float* x = lds;            // [Ci][Hi][Wi] of row r
    float* w = lds + img;      // [Ci][kh][kw] of channel c
    float* part = w + K;       // [S][P] partial sums
    const float* src = a.in + (int64_t)r * a.in_stride + a.in_off;
    for (int i = tid; i < img; i += kConvThreads) x[i] = src[i];
    const float* Wc = a.W + (int64_t)c * K;
    for (int i = tid; i < K; i += kConvThreads) w[i] = Wc[i];
    const float bias = a.b[c];
    if (a.macro && c == 0)   // the dense input's macro tail: F[r][Co*P ..] = obs[r][0 .. macro_len)
        for (int i = tid; i < a.macro_len; i += kConvThreads)
            a.out[(int64_t)r * a.out_stride + (int64_t)a.Co * P + i] = a.macro[(int64_t)r * a.macro_stride + i];
    __syncthreads();
    // output pixel p = t % P, input-channel slice s = t / P of S slices (fixed order: slice 0
    // first); within a slice the sum runs over (ci, i, j) like torch's weight row, with the
    // padding bounds hoisted out of the channel loop
    const int S = max(1, min(kConvThreads / P, a.Ci));
    const int cper = (a.Ci + S - 1) / S;
    for (int t = tid; t < S * P; t += kConvThreads) {
        const int p = t % P, s = t / P;
        const int ho = p / a.Wo, wo = p - ho * a.Wo;
        const int c0 = s * cper, c1 = min(a.Ci, c0 + cper);
        const int h0 = ho * a.sh - a.ph, w0 = wo * a.sw - a.pw;
        const int i0 = max(0, -h0), i1 = min(a.kh, a.Hi - h0), j0 = max(0, -w0), j1 = min(a.kw, a.Wi - w0);
        const int khw = a.kh * a.kw;
        float acc = 0.f;
        for (int ci = c0; ci < c1; ci++) {
            const float* xc = x + ci * HWi + h0 * a.Wi + w0;
            const float* wc = w + ci * khw;
            for (int i = i0; i < i1; i++)
                for (int j = j0; j < j1; j++) acc = fmaf(xc[i * a.Wi + j], wc[i * a.kw + j], acc);
        }
        part[s * P + p] = acc;
    }
    __syncthreads();
    for (int p = tid; p < P; p += kConvThreads) {
        float v = part[p];
        for (int s = 1; s < S; s++) v += part[s * P + p];
        a.out[(int64_t)r * a.out_stride + a.out_off + (int64_t)c * P + p] = elu_f(v + bias);
    }
}

// ---- the whole conv stack as ONE launch (NC >= 2 convs; the per-conv launches above stay for NC = 1, for
// stacks whose redundant part does not fit LDS, and for DQNX_ACT_TS=0) ----------------------------------
//
// Grid (G, n): workgroup (g, row) stages the row's micro grid and every weight it will use in ONE round
// of loads, runs convs 1 .. NC-2 redundantly in LDS (HEAD net: conv 1, 2 -> 32 channels on 27 x 5, 78 K
// FMA), then channels [g Co/G, (g+1) Co/G) of conv NC-1 (bias + ELU), and from those its share of every
// pre-activation of conv NC (split-K over conv NC's input channels: [Co_last][Ho Wo] floats, 64 x 21 for
// the HEAD net).  The last workgroup of a row group (the MLP acting kernel's R rows, and its ticket word:
// the kernel boundary orders the two users and each leaves the word at zero) sums the G shares of each
// row in workgroup order (fixed order: deterministic), adds the bias, applies ELU and writes the dense
// input F = cat(flatten(conv NC) in CHW order, macro) (R:env/dqn_config.py:135-138).
//
// The hand-off is k_act_mlp2's (act.hip): the shares go out as write-through (sc1) stores -- a relaxed
// agent-scope store lowers to `global_store ... sc1` -- every storing wave drains vmcnt before the
// workgroup barrier, ONE lane then takes the relaxed agent-scope ticket, and the workgroup whose ticket
// comes back last is the consumer: row 1 of MI355X_MICROARCH.md's measured hand-off table ("ONE lane of
// each storing workgroup, for ALL that workgroup's stores ... an agent-scope atomic add", the consumer
// "the workgroup whose add came last, told by the value its add returned", 4-byte sc1 stores and loads).
// The last arriver's agent-scope acquire is kept on top of that, as in k_act_mlp2.  No workgroup waits
// for another: all but the last arriver exit, so nothing needs the grid to be co-resident.
constexpr int kStackThreads = 1024;
constexpr int kStageU = 8;   // staged floats in flight per thread

// y[c][p] partial or whole sums of one conv on LDS operands: x [Ci][Hi][Wi], w [Cn][wK] (row c: channel
// c's [Ci][kh][kw] weights), N = Cn * Ho * Wo outputs.  N >= threads: a thread per output, the whole K sum.
// Fewer: S = min(threads / N, Ci) input-channel slices per output (slice 0 first, fixed order), summed
// through `part`.  Within a slice the sum runs (ci, i, j) like torch's weight row, padding bounds hoisted
// (k_act_conv's loop).  epi(o, sum) gets output o = c * P + p.  Block-uniform control flow.
// KH x KW > 0: that window at compile time, its taps unrolled with the padding as a per-tap predicate (a tap
// outside the image contributes fmaf(0, w, acc) = acc), so a channel's KH KW operand pairs are in flight
// together; 0 x 0: any window, k_act_conv's loops with per-thread bounds.
template <int KH, int KW, class Epi>
__device__ __forceinline__ void stack_conv_k(const ActConvGeom& q, int Ci, int Cn, const float* x, const float* w,
                                             int wK, float* part, Epi epi) {
    const int tid = threadIdx.x;
    const int P = q.Ho * q.Wo, N = Cn * P, HWi = q.Hi * q.Wi, khw = q.kh * q.kw;
    const int S = max(1, min(kStackThreads / N, Ci));
    const int cper = (Ci + S - 1) / S;
    for (int t = tid; t < S * N; t += kStackThreads) {
        const int s = t / N, o = t - s * N;
        const int c = o / P, p = o - c * P;
        const int ho = p / q.Wo, wo = p - ho * q.Wo;
        const int c0 = s * cper, c1 = min(Ci, c0 + cper);
        const int h0 = ho * q.sh - q.ph, w0 = wo * q.sw - q.pw;
        float acc = 0.f;
        if constexpr (KH > 0) {
            int off[KH * KW];   // tap's offset in a channel image (0 where the tap is padding)
            bool in[KH * KW];
#pragma unroll
            for (int i = 0; i < KH; i++)
#pragma unroll
                for (int j = 0; j < KW; j++) {
                    const bool ok = h0 + i >= 0 && h0 + i < q.Hi && w0 + j >= 0 && w0 + j < q.Wi;
                    in[i * KW + j] = ok;
                    off[i * KW + j] = ok ? (h0 + i) * q.Wi + w0 + j : 0;
                }
            const float* wc = w + c * wK + c0 * (KH * KW);
            const float* xc = x + c0 * HWi;
#pragma unroll 2
            for (int ci = c0; ci < c1; ci++, wc += KH * KW, xc += HWi) {
#pragma unroll
                for (int k = 0; k < KH * KW; k++) {
                    const float xv = xc[off[k]];
                    acc = fmaf(in[k] ? xv : 0.f, wc[k], acc);
                }
            }
        } else {
            const int i0 = max(0, -h0), i1 = min(q.kh, q.Hi - h0), j0 = max(0, -w0), j1 = min(q.kw, q.Wi - w0);
            for (int ci = c0; ci < c1; ci++) {
                const float* xc = x + ci * HWi + h0 * q.Wi + w0;
                const float* wc = w + c * wK + ci * khw;
                for (int i = i0; i < i1; i++)
                    for (int j = j0; j < j1; j++) acc = fmaf(xc[i * q.Wi + j], wc[i * q.kw + j], acc);
            }
        }
        if (S == 1) epi(o, acc);
        else part[t] = acc;
    }
    if (S > 1) {
        __syncthreads();
        for (int o = tid; o < N; o += kStackThreads) {
            float v = part[o];
            for (int s = 1; s < S; s++) v += part[s * N + o];
            epi(o, v);
        }
    }
}

template <class Epi>
__device__ __forceinline__ void stack_conv(const ActConvGeom& q, int Ci, int Cn, const float* x, const float* w, int wK,
                                           float* part, Epi epi) {
    if (q.kh == 3 && q.kw == 3) stack_conv_k<3, 3>(q, Ci, Cn, x, w, wK, part, epi);   // (the reference's convs)
    else stack_conv_k<0, 0>(q, Ci, Cn, x, w, wK, part, epi);
}

__global__ __launch_bounds__(kStackThreads) void k_act_conv_stack(ActStackArgs a) {
    extern __shared__ float lds[];
    __shared__ int s_last;
    const int tid = threadIdx.x, g = blockIdx.x, row = blockIdx.y;
    const int NC = a.NC, G = a.G;
    const ActConvGeom& gp = a.L[NC - 2];   // conv NC-1: its output channels are split over the G workgroups
    const ActConvGeom& gl = a.L[NC - 1];   // conv NC: split-K over those channels
    const int Cg = gp.Co / G, c0 = g * Cg;
    const int Kp = gp.Ci * gp.kh * gp.kw, Pp = gp.Ho * gp.Wo;
    const int khwl = gl.kh * gl.kw, Kl = gl.Ci * khwl, Pl = gl.Ho * gl.Wo, NL = gl.Co * Pl, Ks = Cg * khwl;
    const int img = a.L[0].Ci * a.L[0].Hi * a.L[0].Wi;
    // LDS: everything staged from memory first, contiguous in staging order (act_stack_plan sizes it)
    float* wred = lds;                      // convs 1 .. NC-2: [Co][K] weights + [Co] bias each
    float* wp = wred + a.wred;              // conv NC-1: [Cg][Kp] weights + [Cg] bias of this workgroup's channels
    float* wl = wp + Cg * (Kp + 1);         // conv NC: [Co_last][Ks], the K slice of this workgroup's channels
    float* buf0 = wl + gl.Co * Ks;          // the row's micro grid, then every second redundant conv's output
    float* buf1 = buf0 + a.buf0;
    float* yp = buf1 + a.buf1;              // [Cg][Pp] conv NC-1 output
    float* part = yp + Cg * Pp;             // [kStackThreads] split-K partial sums
    // (0) one round of loads: element e of the staged range comes from ...
    const int e_wp = a.wred, e_bp = e_wp + Cg * Kp, e_wl = e_bp + Cg, e_img = e_wl + gl.Co * Ks, E = e_img + img;
    const float* rowp = a.in + (int64_t)row * a.in_stride;
    auto src = [&](int e) -> const float* {
        if (e >= e_img) return rowp + a.in_off + (e - e_img);   // micro grid as (c, h, w) (R:env/dqn_config.py:126-128)
        if (e >= e_wl) {
            const int i = e - e_wl, co = i / Ks, k = i - co * Ks;
            return a.params + gl.off + (int64_t)co * Kl + c0 * khwl + k;
        }
        if (e >= e_bp) return a.params + gp.off + (int64_t)gp.Co * Kp + c0 + (e - e_bp);
        if (e >= e_wp) return a.params + gp.off + (int64_t)c0 * Kp + (e - e_wp);
        int i = e;
        for (int l = 0; l + 2 < NC; l++) {
            const int cnt = a.L[l].Co * (a.L[l].Ci * a.L[l].kh * a.L[l].kw + 1);
            if (i < cnt) return a.params + a.L[l].off + i;
            i -= cnt;
        }
        return a.params;   // (not reached: e < a.wred)
    };
    for (int e0 = tid; e0 < E; e0 += kStageU * kStackThreads) {
        float v[kStageU];
#pragma unroll
        for (int u = 0; u < kStageU; u++) {
            const int e = e0 + u * kStackThreads;
            v[u] = e < E ? *src(e) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kStageU; u++) {
            const int e = e0 + u * kStackThreads;
            if (e < E) lds[e] = v[u];
        }
    }
    __syncthreads();
    // (1) convs 1 .. NC-2, whole, in LDS
    const float* x = buf0;
    {
        const float* w = wred;
        for (int l = 0; l + 2 < NC; l++) {
            const ActConvGeom& q = a.L[l];
            const int K = q.Ci * q.kh * q.kw, P = q.Ho * q.Wo;
            float* y = (l & 1) ? buf0 : buf1;
            const float* b = w + q.Co * K;
            stack_conv(q, q.Ci, q.Co, x, w, K, part, [&](int o, float v) { y[o] = elu_f(v + b[o / P]); });
            __syncthreads();
            x = y;
            w += q.Co * (K + 1);
        }
    }
    // (2) conv NC-1, this workgroup's channels
    stack_conv(gp, gp.Ci, Cg, x, wp, Kp, part, [&](int o, float v) { yp[o] = elu_f(v + wp[Cg * Kp + o / Pp]); });
    __syncthreads();
    // (3) their share of conv NC's pre-activations, written through (sc1) to memory
    float* sh = a.shares + ((int64_t)row * G + g) * NL;
    stack_conv(gl, Cg, gl.Co, yp, wl, Ks, part,
               [&](int o, float v) { __hip_atomic_store(sh + o, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); });
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int grp = row / a.R, row0 = grp * a.R;
    const int nr = min(a.R, a.n - row0);
    const uint32_t arrivals = (uint32_t)G * (uint32_t)nr;   // workgroups of this row group
    if (arrivals > 1) {
        if (tid == 0) {
            const uint32_t t = __hip_atomic_fetch_add(a.tickets - grp, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int last = t == arrivals - 1;
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                *(a.tickets - grp) = 0;   // ready for the MLP kernel, which takes the same word next
            }
            s_last = last;
        }
        __syncthreads();
        if (!s_last) return;
    }
    // (4) last arriver of the row group: F = cat(ELU(sum of the shares in workgroup order + bias), macro)
    const float* bl = a.params + gl.off + (int64_t)gl.Co * Kl;
    // (kTailO outputs a thread, kTailW shares of each requested together: the sc1 loads are served by memory,
    // and one at a time they cost a round trip each)
    constexpr int kTailO = 4, kTailW = 16;
    const int tot = nr * NL;
    for (int i0 = tid; i0 < tot; i0 += kTailO * kStackThreads) {
        const float* p[kTailO];
        float bias[kTailO], z[kTailO];
        int fo[kTailO];
#pragma unroll
        for (int u = 0; u < kTailO; u++) {
            const int i = min(i0 + u * kStackThreads, tot - 1);   // (clamped: valid loads, result dropped)
            const int r = i / NL, o = i - r * NL;
            p[u] = a.shares + (int64_t)(row0 + r) * G * NL + o;
            bias[u] = bl[o / Pl];
            fo[u] = (row0 + r) * (int)a.F_stride + o;
            z[u] = 0.f;
        }
        for (int w0 = 0; w0 < G; w0 += kTailW) {
            float v[kTailO][kTailW];
#pragma unroll
            for (int u = 0; u < kTailO; u++)
#pragma unroll
                for (int w = 0; w < kTailW; w++)
                    v[u][w] = __hip_atomic_load(p[u] + (int64_t)min(w0 + w, G - 1) * NL, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int u = 0; u < kTailO; u++)
#pragma unroll
                for (int w = 0; w < kTailW; w++)
                    if (w0 + w < G) z[u] += v[u][w];
        }
#pragma unroll
        for (int u = 0; u < kTailO; u++)
            if (i0 + u * kStackThreads < tot) a.F[fo[u]] = elu_f(z[u] + bias[u]);
    }
    for (int i = tid; i < nr * a.macro_len; i += kStackThreads) {
        const int r = i / a.macro_len, k = i - r * a.macro_len;
        a.F[(int64_t)(row0 + r) * a.F_stride + NL + k] = a.in[(int64_t)(row0 + r) * a.in_stride + k];
    }
}

}  // namespace

size_t act_stack_plan(ActStackArgs& a) {
    a.buf0 = a.buf1 = a.wred = 0;
    if (a.NC < 2 || a.NC > DQNX_MAX_CONV || a.G < 1) return 0;
    // tensor 0 = the micro grid, tensor l = conv l's output (l <= NC-2): even ones in buf0, odd in buf1
    a.buf0 = a.L[0].Ci * a.L[0].Hi * a.L[0].Wi;
    for (int l = 0; l + 2 < a.NC; l++) {
        const ActConvGeom& q = a.L[l];
        int& b = (l & 1) ? a.buf0 : a.buf1;
        b = std::max(b, q.Co * q.Ho * q.Wo);
        a.wred += q.Co * (q.Ci * q.kh * q.kw + 1);
    }
    const ActConvGeom& gp = a.L[a.NC - 2];
    const ActConvGeom& gl = a.L[a.NC - 1];
    const int Cg = gp.Co / a.G;
    const size_t fl = (size_t)a.wred + (size_t)Cg * (gp.Ci * gp.kh * gp.kw + 1) + (size_t)gl.Co * Cg * gl.kh * gl.kw +
                      a.buf0 + a.buf1 + (size_t)Cg * gp.Ho * gp.Wo + kStackThreads;
    return fl * sizeof(float);
}

int launch_act_conv_stack(const ActStackArgs& a, hipStream_t s) {
    if (a.n <= 0) return DQNX_OK;
    ActStackArgs p = a;
    const size_t lds = act_stack_plan(p);
    if (!lds || lds > 64 * 1024 || a.L[a.NC - 2].Co % a.G || a.R < 1)
        return set_error(DQNX_EUNSUPPORTED, "dqnx_act: conv stack does not fit the one-launch kernel (%zu B LDS)", lds);
    DQNX_LAUNCH(k_act_conv_stack, dim3(a.G, a.n), dim3(kStackThreads), lds, s, p);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

size_t act_conv_lds_bytes(const ActConvArgs& a) {
    const int P = a.Ho * a.Wo, K = a.Ci * a.kh * a.kw;
    const int S = std::max(1, std::min(kConvThreads / std::max(P, 1), a.Ci));
    return (size_t)(a.Ci * a.Hi * a.Wi + K + S * P) * sizeof(float);
}

int launch_act_conv(const ActConvArgs& a, hipStream_t s) {
    if (a.n <= 0) return DQNX_OK;
    const size_t lds = act_conv_lds_bytes(a);
    if (lds > 64 * 1024 || a.Ho * a.Wo > kConvThreads * 64)
        return set_error(DQNX_EUNSUPPORTED, "dqnx_act: conv layer too large for the acting kernel (%zu B LDS)", lds);
    DQNX_LAUNCH(k_act_conv, dim3(a.Co, a.n), dim3(kConvThreads), lds, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
