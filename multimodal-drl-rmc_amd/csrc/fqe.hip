// Fitted Q evaluation (include/dqnx.h "fitted Q evaluation"): the launches the two sweeps put behind the
// route's own forward launches (eval.hip's "eval_idx" before them, "eval_head" on the per-layer routes):
//
//   "policy_rows"  dqnx_policy_sweep: pi(s), pi(s') of every row of the chunk into the slot-indexed table
//   "fqe_rows"     dqnx_fqe_range: q_pi, delta_pi, Huber and the episode-start test per row, the optional
//                  per-row output, one fp64 record per workgroup
//   "fqe_fold"     one workgroup: the records in workgroup order, then into the accumulator in the scratch
//
// k_fqe_fold restates k_eval_fold for FqePartial: k_eval_fold classifies its words by kEvalSums and the
// layout of EvalPartial, so a record shape passed as a parameter would have changed its instantiation.
// No floating-point atomics anywhere; the order of every sum is fixed (eval.hip's scheme).
#include "common.hpp"
#include "learn.hpp"
#include "fqe.hpp"

namespace dqnx {

namespace {

__device__ __forceinline__ void fqe_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Q of lane hj's action slot from the raw head output r of that lane (valid for hj < A): k_eval_rows' order
__device__ __forceinline__ float fqe_qval(float r, bool duel, int hj, int A) {
    if (!duel) return r;
    const float v = __shfl(r, 0, 16);
    const float adv = __shfl(r, hj + 1 < 16 ? hj + 1 : 15, 16);
    float sum = (hj >= 1 && hj <= A) ? r : 0.f;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 16);
    return eval_dueling(v, adv, sum, A);
}

// the first maximum over the lanes hj < A (every lane of the row returns it)
__device__ __forceinline__ int fqe_argmax16(float q, int hj, int A) {
    float bv = hj < A ? q : -INFINITY;
    int bi = hj;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m, 16);
        const int oi = __shfl_xor(bi, m, 16);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    return bi;
}

// 16 rows per workgroup, 16 lanes per row, head slot j in lane j
__global__ __launch_bounds__(256) void k_policy_rows(PolicyRowsArgs a) {
    // every argument the loads read: one wait (DQNX_KERNARG, common.hpp)
    asm volatile("" ::DQNX_KERNARG(a.Bl), DQNX_KERNARG(a.A), DQNX_KERNARG(a.valid), DQNX_KERNARG(a.head_kind),
                 DQNX_KERNARG(a.slots), DQNX_KERNARG(a.raw), DQNX_KERNARG(a.phys), DQNX_KERNARG(a.table));
    const int tid = threadIdx.x, hb = tid >> 4, hj = tid & 15;
    const int b = blockIdx.x * 16 + hb;
    const int bc = b < a.Bl ? b : a.Bl - 1;
    const int A = a.A;
    // every load first
    const int64_t base = (int64_t)bc * 16 + hj;
    const float r0 = gld(a.raw + base);
    const float r1 = gld(a.raw + (int64_t)a.Bl * 16 + base);
    const int32_t slot = gld(a.phys + bc);
    const bool duel = a.head_kind == DQNX_HEAD_DUELING;
    const int p0 = fqe_argmax16(fqe_qval(r0, duel, hj, A), hj, A);
    const int p1 = fqe_argmax16(fqe_qval(r1, duel, hj, A), hj, A);
    if (hj == 0 && b < a.valid && slot >= 0 && slot < a.slots)
        *reinterpret_cast<int2*>(a.table + (int64_t)slot * 2) = make_int2(p0, p1);
}

constexpr int FQ_F = 3;   // floats per LDS row: q_pi, |delta_pi|, huber
template <bool TRANS>
__global__ __launch_bounds__(256) void k_fqe_rows(FqeRowsArgs a) {
    __shared__ float fv[16][FQ_F + 1];
    __shared__ int iv[16][2];   // real, start
    asm volatile("" ::DQNX_KERNARG(a.Bl), DQNX_KERNARG(a.A), DQNX_KERNARG(a.valid), DQNX_KERNARG(a.head_kind),
                 DQNX_KERNARG(a.n_env), DQNX_KERNARG(a.first), DQNX_KERNARG(a.capacity), DQNX_KERNARG(a.ctrl),
                 DQNX_KERNARG(a.raw), DQNX_KERNARG(a.trans), DQNX_KERNARG(a.phys), DQNX_KERNARG(a.act),
                 DQNX_KERNARG(a.rew), DQNX_KERNARG(a.done), DQNX_KERNARG(a.table));
    const int tid = threadIdx.x, hb = tid >> 4, hj = tid & 15;
    const int b0 = blockIdx.x * 16;
    const int A = a.A;
    const int b = b0 + hb;
    const int bc = b < a.Bl ? b : a.Bl - 1;
    const bool real = b < a.valid;

    // (0) every independent load first
    const int64_t rbase = (int64_t)bc * 16 + hj;
    const float r0 = gld(a.raw + rbase);
    const float r2 = gld(a.raw + (int64_t)2 * a.Bl * 16 + rbase);
    const int64_t size = gld(&a.ctrl->ring_size), wptr = gld(&a.ctrl->ring_wptr);
    int32_t slot = gld(a.phys + bc);
    int act;
    float rew, done;
    if constexpr (TRANS) {
        const float4 tr = a.trans[bc];
        act = __float_as_int(tr.x);
        rew = tr.y;
        done = tr.z;
    } else {
        const int32_t sl = (slot >= 0 && slot < a.capacity) ? slot : 0;
        act = gld(a.act + sl);
        rew = gld(a.rew + sl);
        done = gld(a.done + sl);
    }
    if (slot < 0 || slot >= a.capacity) slot = 0;
    const int2 pe = *reinterpret_cast<const int2*>(a.table + (int64_t)slot * 2);
    // the previous transition of the same environment: logical position p - n_env (nstep.hpp's convention)
    const int64_t cap = a.capacity;
    const int64_t p = a.first + (real ? b : 0);
    int64_t pp = p - a.n_env;
    const bool oldest = pp < 0;
    if (pp < 0) pp = 0;
    if (pp > size - 1) pp = size - 1;
    if (pp < 0) pp = 0;
    const int64_t rb = ((wptr - size) % cap + cap) % cap;
    const float pdone = gld(a.done + (rb + pp) % cap);
    if (act < 0 || act >= A) act = 0;
    const int ps = fqe_clamp(pe.x, A), pn = fqe_clamp(pe.y, A);

    // (1) the row: fqe.hpp's forms, 16 lanes
    const bool duel = a.head_kind == DQNX_HEAD_DUELING;
    const float q0 = fqe_qval(r0, duel, hj, A), q2 = fqe_qval(r2, duel, hj, A);
    const float qpi = __shfl(q0, ps, 16);
    const float qn = __shfl(q2, pn, 16);
    const float qa = __shfl(q0, act, 16);
    const float y = eval_target(rew, done, a.gamma, qn);
    const float delta = eval_delta(y, qa);
    const float lb = eval_huber(delta);
    const bool start = oldest || pdone != 0.f;
    if (hj == 0) {
        fv[hb][0] = qpi;
        fv[hb][1] = fabsf(delta);
        fv[hb][2] = lb;
        iv[hb][0] = real ? 1 : 0;
        iv[hb][1] = (real && start) ? 1 : 0;
        if (real && a.rows_out) *reinterpret_cast<float2*>(a.rows_out + (int64_t)b * 2) = make_float2(qpi, delta);
    }
    fqe_lds_barrier();

    // (2) the workgroup's record: one thread per 8-byte word, the 16 rows in row order
    FqePartial* out = a.part + blockIdx.x;
    if (tid == 0) {
        int64_t n = 0;
        for (int r = 0; r < 16; r++) n += iv[r][1];
        out->start_rows = n;
    } else if (tid <= kFqeSums) {
        const int w = tid - 1;   // 0 q_pi, 1 q_pi over starts, 2 |delta|, 3 huber
        const int col = w == 0 ? 0 : w - 1;
        double s = 0.0;
        for (int r = 0; r < 16; r++) {
            if (!iv[r][w == 1 ? 1 : 0]) continue;
            s += (double)fv[r][col];
        }
        out->sum[w] = s;
    } else if (tid == kFqeSums + 1) {
        double m = -INFINITY;
        for (int r = 0; r < 16; r++)
            if (iv[r][0]) m = fmax(m, (double)fv[r][0]);
        out->max_q = m;
    } else if (tid == kFqeSums + 2) {
        double m = INFINITY;
        for (int r = 0; r < 16; r++)
            if (iv[r][0]) m = fmin(m, (double)fv[r][0]);
        out->min_q = m;
    }
}

// One workgroup, one thread per 8-byte word of the record (k_eval_fold's pattern: 16 loads in flight, adds
// in record order), then the chunk into the accumulator (set by the first chunk).  The last chunk stores `rows`.
__global__ __launch_bounds__(64) void k_fqe_fold(FqeFoldArgs a) {
    const int w = threadIdx.x;
    if (w >= kFqeWords) return;
    const int kind = w == 0 ? 3 : (w <= kFqeSums ? 0 : (w == kFqeSums + 1 ? 1 : 2));   // int, sum, max, min
    int64_t* accw = reinterpret_cast<int64_t*>(a.acc) + 1 + w;
    constexpr int kFoldBatch = 16;
    int64_t si = 0;
    double s = kind == 0 ? 0.0 : (kind == 2 ? (double)INFINITY : -(double)INFINITY);
    for (int p0 = 0; p0 < a.nparts; p0 += kFoldBatch) {
        int64_t x[kFoldBatch];
#pragma unroll
        for (int u = 0; u < kFoldBatch; u++) {
            const int p = p0 + u < a.nparts ? p0 + u : a.nparts - 1;
            x[u] = gld(reinterpret_cast<const int64_t*>(a.part + p) + w);
        }
#pragma unroll
        for (int u = 0; u < kFoldBatch; u++) {
            if (p0 + u >= a.nparts) continue;
            const double xd = __longlong_as_double(x[u]);
            si += x[u];
            s = kind == 0 ? s + xd : (kind == 1 ? fmax(s, xd) : fmin(s, xd));
        }
    }
    if (kind == 3) {
        *accw = a.first ? si : *accw + si;
    } else {
        double* accd = reinterpret_cast<double*>(accw);
        if (!a.first) {
            const double o = *accd;
            s = kind == 0 ? o + s : (kind == 1 ? fmax(o, s) : fmin(o, s));
        }
        *accd = s;
    }
    if (w == 0 && a.last) a.acc->rows = a.rows;
}

}  // namespace

int launch_policy_rows(const PolicyRowsArgs& a, hipStream_t s) {
    if (!a.raw || !a.phys || !a.table) return set_error(DQNX_EINVAL, "policy rows: null buffer");
    if (a.Bl < 1 || a.valid < 1 || a.valid > a.Bl || a.A < 1 || a.A > 16 || a.slots < 1)
        return set_error(DQNX_EINVAL, "policy rows: bad shape");
    if (((uintptr_t)a.table) & 7) return set_error(DQNX_EINVAL, "policy rows: misaligned table");
    DQNX_LAUNCH(k_policy_rows, dim3((a.Bl + 15) / 16), dim3(256), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_fqe_rows(const FqeRowsArgs& a, hipStream_t s) {
    if (!a.raw || !a.part || !a.table || !a.ctrl || !a.phys || !a.done)
        return set_error(DQNX_EINVAL, "fqe rows: null buffer");
    if (!a.trans && (!a.act || !a.rew)) return set_error(DQNX_EINVAL, "fqe rows: null buffer");
    if (a.Bl < 1 || a.valid < 1 || a.valid > a.Bl || a.A < 1 || a.A > 16 || a.n_env < 1 ||
        a.capacity < 1 || a.first < 0)
        return set_error(DQNX_EINVAL, "fqe rows: bad shape");
    if ((((uintptr_t)a.rows_out | (uintptr_t)a.table) & 7) || ((uintptr_t)a.trans & 15))
        return set_error(DQNX_EINVAL, "fqe rows: misaligned buffer");
    const dim3 grid((a.Bl + 15) / 16), block(256);
    if (a.trans) DQNX_LAUNCH((k_fqe_rows<true>), grid, block, 0, s, a);
    else DQNX_LAUNCH((k_fqe_rows<false>), grid, block, 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_fqe_fold(const FqeFoldArgs& a, hipStream_t s) {
    if (!a.part || !a.acc || a.nparts < 1) return set_error(DQNX_EINVAL, "fqe fold: bad arguments");
    static_assert(kFqeWords <= 64, "k_fqe_fold: one thread per word of the record");
    DQNX_LAUNCH(k_fqe_fold, dim3(1), dim3(64), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
