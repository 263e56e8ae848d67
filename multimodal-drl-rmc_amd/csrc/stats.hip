// Training statistics of a learn step (DQNX_STEP_STATS, include/dqnx.h "training statistics"): one
// launch after the step's last compute launch that reduces the step's own buffers into the
// dqnx_learn_stats block of the arena.  It reads Q / TD / IS weights / the sampled transitions, the
// gradient, the online parameters (after Adam) and dqnx_ctrl.loss; it writes the block and its own
// workspace (the partials and the ticket), nothing else.
//
// Grid (fixed by the plan, never by scheduling): workgroups [0, n_bwg) take rows_per_bwg minibatch
// rows each; workgroups [n_bwg, n_bwg + n_chunks) take one chunk each of the flat gradient and
// parameter vectors.  Chunks are cut per tensor (StatsArgs::c0), so a tensor's sum of squares is the
// sum of whole chunk partials and no element needs a tensor lookup.
//
// Determinism: every sum is fp64 from the first add -- the square of an fp32 is exact in fp64 -- and
// every add has a fixed place: a lane adds its elements in index order, the 64 lanes of a wave fold by
// shuffles (a fixed tree), the 4 waves fold in wave order through LDS, and the workgroup's partial goes
// to the workspace.  The workgroup whose ticket comes back last folds the partials IN INDEX ORDER and
// one lane adds the step's totals into the block.  Which workgroup that is does not matter: it reads
// the same partials and adds them in the same order.  No floating-point atomics; the histograms and
// row counts are integer atomics (LDS first, then one global add per non-empty bin), which commute.
//
// Hand-off: plain partial stores, s_waitcnt, barrier, then ONE lane's agent-scope release fence and
// relaxed ticket; the last arriver's lane takes an acquire fence before the barrier that lets the
// workgroup read the partials (k_act_mlp2's form, act.hip).  The ticket is left at zero.
#include <math.h>

#include "common.hpp"
#include "learn.hpp"

namespace dqnx {

namespace {

// one batch workgroup's partial: sums first, then extrema (kept as doubles in the workspace: every
// fp32 is exact in fp64)
enum {
    S_QSA = 0, S_QSQ, S_QMAX, S_TGT, S_ATD, S_GAP, S_REW, S_ISW, N_SUM,
    X_QSA_MIN = N_SUM, X_QSA_MAX, X_QMAX_MAX, X_TGT_MIN, X_TGT_MAX, X_ATD_MAX, X_ISW_MIN, N_ALL
};
static_assert(N_ALL <= kStatsBatchDoubles, "batch partial");
// is_min[k - N_SUM]
__device__ __forceinline__ bool stat_is_min(int k) { return k == X_QSA_MIN || k == X_TGT_MIN || k == X_ISW_MIN; }

// LDS counters of a batch workgroup: three histograms, then the row counts
constexpr int H_TD = 0, H_GREEDY = 16, H_TAKEN = 32, H_HUBER = 48, H_AGREE = 49, H_DONE = 50, H_COUNT = 51;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_down(v, o, kWave);
    return v;   // lane 0
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fminf(v, __shfl_down(v, o, kWave));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmaxf(v, __shfl_down(v, o, kWave));
    return v;
}

__device__ __forceinline__ double ld_part(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// rows [r0, r1) of the minibatch; thread 0 leaves the workgroup's partial in part[0, N_ALL)
__device__ void stats_batch(const StatsArgs& a, int wg, double (*sh)[kStatsBatchDoubles], uint32_t* hist, double* part) {
    const int tid = threadIdx.x;
    if (tid < H_COUNT) hist[tid] = 0;
    __syncthreads();
    const int A = a.A;
    const bool vec = (A & 3) == 0;
    double s[N_SUM];
#pragma unroll
    for (int k = 0; k < N_SUM; k++) s[k] = 0.0;
    float qsa_min = INFINITY, qsa_max = -INFINITY, qmax_max = -INFINITY, tgt_min = INFINITY, tgt_max = -INFINITY;
    float atd_max = -INFINITY, isw_min = INFINITY;
    const int r0 = wg * a.rows_per_bwg;
    const int r1 = min(a.B, r0 + a.rows_per_bwg);
    for (int r = r0 + tid; r < r1; r += kStatsThreads) {
        const float* qr = a.q + (int64_t)r * A;
        float qv[DQNX_STATS_MAX_ACTIONS];
#pragma unroll
        for (int j = 0; j < DQNX_STATS_MAX_ACTIONS; j += 4) {
            if (j >= A) {
                qv[j] = qv[j + 1] = qv[j + 2] = qv[j + 3] = -INFINITY;
            } else if (vec) {   // rows of a multiple of 4 floats lie on 16-byte boundaries
                const float4 v = ld4(qr + j);
                qv[j] = v.x; qv[j + 1] = v.y; qv[j + 2] = v.z; qv[j + 3] = v.w;
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++) qv[j + u] = j + u < A ? qr[j + u] : -INFINITY;
            }
        }
        // first maximal index (torch.argmax) and the runner-up value
        float m1 = qv[0], m2 = -INFINITY;
        int best = 0;
#pragma unroll
        for (int j = 1; j < DQNX_STATS_MAX_ACTIONS; j++) {
            const float v = qv[j];
            if (j < A) {
                if (v > m1) { m2 = m1; m1 = v; best = j; }
                else if (v > m2) m2 = v;
            }
        }
        const float gap = A > 1 ? m1 - m2 : 0.f;
        const float y = a.td[r], qsa = a.td[(int64_t)a.B + r], ad = a.td[(int64_t)2 * a.B + r];
        int act;
        float rew, dn;
        if (a.trans) {
            const float4 t = a.trans[r];
            act = __float_as_int(t.x); rew = t.y; dn = t.z;
        } else {
            int64_t slot = a.phys[r];
            if (slot < 0 || slot >= a.capacity) slot = 0;   // (a sampler error leaves dqnx_ctrl.error set)
            act = a.ring_act[slot]; rew = a.ring_rew[slot]; dn = a.ring_done[slot];
        }
        s[S_QSA] += (double)qsa;
        s[S_QSQ] += (double)qsa * (double)qsa;
        s[S_QMAX] += (double)m1;
        s[S_TGT] += (double)y;
        s[S_ATD] += (double)ad;
        s[S_GAP] += (double)gap;
        s[S_REW] += (double)rew;
        qsa_min = fminf(qsa_min, qsa); qsa_max = fmaxf(qsa_max, qsa);
        qmax_max = fmaxf(qmax_max, m1);
        tgt_min = fminf(tgt_min, y); tgt_max = fmaxf(tgt_max, y);
        atd_max = fmaxf(atd_max, ad);
        if (a.isw) {
            const float w = a.isw[r];
            s[S_ISW] += (double)w;
            isw_min = fminf(isw_min, w);
        }
        // |delta| by its fp32 exponent (biased 0 = zero / denormal -> bin 0; 255 = inf / nan -> bin 15)
        const int e = (int)((__float_as_uint(ad) >> 23) & 0xffu) - 127;
        const int bin = min(max(e + 12, 0), DQNX_STATS_TD_BINS - 1);
        atomicAdd(&hist[H_TD + bin], 1u);
        atomicAdd(&hist[H_GREEDY + best], 1u);
        if ((unsigned)act < (unsigned)DQNX_STATS_MAX_ACTIONS) atomicAdd(&hist[H_TAKEN + act], 1u);
        if (ad >= 1.f) atomicAdd(&hist[H_HUBER], 1u);
        if (best == act) atomicAdd(&hist[H_AGREE], 1u);
        if (dn != 0.f) atomicAdd(&hist[H_DONE], 1u);
    }
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < N_SUM; k++) {
        const double v = wave_sum(s[k]);
        if (lane == 0) sh[wave][k] = v;
    }
    const float x[N_ALL - N_SUM] = {wave_min(qsa_min), wave_max(qsa_max), wave_max(qmax_max), wave_min(tgt_min),
                                    wave_max(tgt_max), wave_max(atd_max), wave_min(isw_min)};
    if (lane == 0) {
#pragma unroll
        for (int k = N_SUM; k < N_ALL; k++) sh[wave][k] = (double)x[k - N_SUM];
    }
    __syncthreads();
    if (tid < N_ALL) {   // the 4 waves, in wave order
        double v = sh[0][tid];
        for (int w = 1; w < kStatsThreads / kWave; w++) {
            const double u = sh[w][tid];
            v = tid < N_SUM ? v + u : (stat_is_min(tid) ? fmin(v, u) : fmax(v, u));
        }
        part[tid] = v;
    }
    // the counts: integer adds commute, so they go straight to the block
    if (tid < H_COUNT && hist[tid]) {
        int64_t* dst = tid < H_GREEDY  ? &a.out->td_hist[tid - H_TD]
                       : tid < H_TAKEN ? &a.out->greedy_hist[tid - H_GREEDY]
                       : tid < H_HUBER ? &a.out->taken_hist[tid - H_TAKEN]
                       : tid == H_HUBER ? &a.out->huber_linear_rows
                       : tid == H_AGREE ? &a.out->agree_rows
                                        : &a.out->done_rows;
        atomicAdd(reinterpret_cast<unsigned long long*>(dst), (unsigned long long)hist[tid]);
    }
}

// chunk c of the flat vectors: sum g^2 and sum theta^2 over its elements into part[0], part[1]
__device__ void stats_chunk(const StatsArgs& a, int c, double (*sh)[kStatsBatchDoubles], double* part) {
    const int tid = threadIdx.x;
    int t = 0;
    while (t + 1 < a.n_tensors && c >= a.c0[t + 1]) t++;
    const int64_t b = a.t_off[t] + (int64_t)(c - a.c0[t]) * a.chunk;
    const int64_t e = min(a.t_off[t + 1], b + a.chunk);
    // [b, v0) scalar head, [v0, v1) 16 bytes per lane, [v1, e) scalar tail (the vectors' bases are
    // 16-byte aligned, so an element index that is a multiple of 4 is a 16-byte boundary)
    const int64_t v0 = min(e, (b + 3) & ~(int64_t)3);
    const int64_t v1 = max(v0, e & ~(int64_t)3);
    double gs = 0.0, ps = 0.0;
#pragma unroll 4
    for (int64_t i = v0 + 4 * tid; i < v1; i += 4 * kStatsThreads) {
        const float4 g = ld4(a.grads + i), p = ld4(a.params + i);
        gs += (double)g.x * (double)g.x;
        gs += (double)g.y * (double)g.y;
        gs += (double)g.z * (double)g.z;
        gs += (double)g.w * (double)g.w;
        ps += (double)p.x * (double)p.x;
        ps += (double)p.y * (double)p.y;
        ps += (double)p.z * (double)p.z;
        ps += (double)p.w * (double)p.w;
    }
    const int nh = (int)(v0 - b), nt = (int)(e - v1);   // <= 3 each
    if (tid < nh + nt) {
        const int64_t i = tid < nh ? b + tid : v1 + (tid - nh);
        const float g = a.grads[i], p = a.params[i];
        gs += (double)g * (double)g;
        ps += (double)p * (double)p;
    }
    const int wave = tid >> 6, lane = tid & 63;
    gs = wave_sum(gs);
    ps = wave_sum(ps);
    if (lane == 0) {
        sh[wave][0] = gs;
        sh[wave][1] = ps;
    }
    __syncthreads();
    if (tid < 2) {
        double v = sh[0][tid];
        for (int w = 1; w < kStatsThreads / kWave; w++) v += sh[w][tid];
        part[tid] = v;
    }
}

}  // namespace

__global__ __launch_bounds__(kStatsThreads) void k_learn_stats(StatsArgs a) {
    __shared__ double sh[kStatsThreads / kWave][kStatsBatchDoubles];
    __shared__ uint32_t hist[64];
    __shared__ double tsum[2][DQNX_STATS_MAX_TENSORS];
    __shared__ double bsum[kStatsBatchDoubles];
    __shared__ int s_last;
    const int tid = threadIdx.x;
    const int wg = blockIdx.x;
    double* cpart = a.part + (int64_t)a.n_bwg * kStatsBatchDoubles;
    if (wg < a.n_bwg)
        stats_batch(a, wg, sh, hist, a.part + (int64_t)wg * kStatsBatchDoubles);
    else
        stats_chunk(a, wg - a.n_bwg, sh, cpart + (int64_t)2 * (wg - a.n_bwg));

    // ---- hand-off: the last workgroup to arrive folds the partials
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t tk = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = tk == gridDim.x - 1;
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // the next launch
        }
        s_last = last;
    }
    __syncthreads();
    if (!s_last) return;

    // ---- partials in index order: lane t the chunks of tensor t, one lane of another wave the batch
    if (tid < a.n_tensors) {
        double g = 0.0, p = 0.0;
        for (int c = a.c0[tid]; c < a.c0[tid + 1]; c++) {
            g += ld_part(cpart + (int64_t)2 * c);
            p += ld_part(cpart + (int64_t)2 * c + 1);
        }
        tsum[0][tid] = g;
        tsum[1][tid] = p;
    } else if (tid >= kWave && tid < kWave + N_ALL) {
        const int k = tid - kWave;
        double v = ld_part(a.part + k);
        for (int w = 1; w < a.n_bwg; w++) {
            const double u = ld_part(a.part + (int64_t)w * kStatsBatchDoubles + k);
            v = k < N_SUM ? v + u : (stat_is_min(k) ? fmin(v, u) : fmax(v, u));
        }
        bsum[k] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    dqnx_learn_stats* o = a.out;
    const bool first = o->steps == 0;   // a zeroed block: set the extrema instead of combining
    o->steps += 1;
    o->rows += a.B;
    o->q_sa_sum += bsum[S_QSA];
    o->q_sa_sq_sum += bsum[S_QSQ];
    o->q_max_sum += bsum[S_QMAX];
    o->target_sum += bsum[S_TGT];
    o->abs_td_sum += bsum[S_ATD];
    o->gap_sum += bsum[S_GAP];
    o->reward_sum += bsum[S_REW];
    o->loss_sum += (double)a.ctrl->loss;
    const float qsa_min = (float)bsum[X_QSA_MIN], qsa_max = (float)bsum[X_QSA_MAX], qmax_max = (float)bsum[X_QMAX_MAX];
    const float tgt_min = (float)bsum[X_TGT_MIN], tgt_max = (float)bsum[X_TGT_MAX], atd_max = (float)bsum[X_ATD_MAX];
    o->q_sa_min = first ? qsa_min : fminf(o->q_sa_min, qsa_min);
    o->q_sa_max = first ? qsa_max : fmaxf(o->q_sa_max, qsa_max);
    o->q_max_max = first ? qmax_max : fmaxf(o->q_max_max, qmax_max);
    o->target_min = first ? tgt_min : fminf(o->target_min, tgt_min);
    o->target_max = first ? tgt_max : fmaxf(o->target_max, tgt_max);
    o->abs_td_max = first ? atd_max : fmaxf(o->abs_td_max, atd_max);
    if (a.isw) {
        const float isw_min = (float)bsum[X_ISW_MIN];
        o->isw_sum += bsum[S_ISW];
        o->isw_min = first ? isw_min : fminf(o->isw_min, isw_min);
    }
    double total = 0.0;
    for (int t = 0; t < a.n_tensors; t++) {
        const double g = tsum[0][t];
        o->grad_sq_last[t] = g;
        o->param_sq_last[t] = tsum[1][t];
        o->grad_sq_sum[t] += g;
        total += g;
    }
    const double norm = sqrt(total);
    o->grad_norm_sum += norm;
    o->grad_norm_max = first ? norm : fmax(o->grad_norm_max, norm);
}

uint64_t stats_part_bytes(int n_bwg, int n_chunks) {
    return ((uint64_t)n_bwg * kStatsBatchDoubles + (uint64_t)n_chunks * 2) * sizeof(double);
}

int launch_learn_stats(const StatsArgs& a, hipStream_t s) {
    if (!a.out || !a.part || !a.ticket || !a.grads || !a.params || !a.q || !a.td || !a.ctrl)
        return set_error(DQNX_EINVAL, "learn stats: null buffer");
    if (!a.trans && (!a.phys || !a.ring_act || !a.ring_rew || !a.ring_done || a.capacity < 1))
        return set_error(DQNX_EINVAL, "learn stats: no source for the sampled transitions");
    if (a.n_tensors < 1 || a.n_tensors > DQNX_STATS_MAX_TENSORS || a.A < 1 || a.A > DQNX_STATS_MAX_ACTIONS)
        return set_error(DQNX_EUNSUPPORTED, "learn stats: %d tensors / %d actions (at most %d / %d)", a.n_tensors, a.A,
                         DQNX_STATS_MAX_TENSORS, DQNX_STATS_MAX_ACTIONS);
    if (a.B < 1 || a.n_bwg < 1 || a.rows_per_bwg < 1 || (int64_t)a.n_bwg * a.rows_per_bwg < a.B || a.chunk < 4)
        return set_error(DQNX_EINVAL, "learn stats: batch geometry");
    // the chunk table must cover [0, P) tensor by tensor
    if (a.c0[0] != 0 || a.t_off[0] != 0 || a.c0[a.n_tensors] != a.n_chunks)
        return set_error(DQNX_EINVAL, "learn stats: chunk table");
    for (int t = 0; t < a.n_tensors; t++) {
        const int64_t n = a.t_off[t + 1] - a.t_off[t];
        if (n < 1 || a.c0[t + 1] - a.c0[t] != (n + a.chunk - 1) / a.chunk)
            return set_error(DQNX_EINVAL, "learn stats: chunk table (tensor %d)", t);
    }
    if ((((uintptr_t)a.grads | (uintptr_t)a.params | (uintptr_t)a.q | (uintptr_t)a.trans | (uintptr_t)a.part) & 15) ||
        ((uintptr_t)a.out & 7))
        return set_error(DQNX_EINVAL, "learn stats: misaligned buffer");
    DQNX_LAUNCH(k_learn_stats, dim3((unsigned)(a.n_bwg + a.n_chunks)), dim3(kStatsThreads), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
