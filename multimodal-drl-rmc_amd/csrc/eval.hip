// Offline evaluation (include/dqnx.h "offline evaluation"): the launches dqnx_eval_range puts around the
// route's own forward launches, per chunk of batch rows:
//
//   "eval_idx"   logical positions lo + c*B + b (clamped to hi - 1) and their ring slots into the scratch table
//   (the route's forward, reading that table; on an n-step engine "nstep_gather" first)
//   "eval_head"  per-layer routes only: the raw head outputs of every stream in the fused plan's layout
//   "eval_rows"  the per-row quantities (eval.hpp), the optional per-row output, one fp64 record per workgroup
//   "eval_fold"  one workgroup: the records in workgroup order, then into the accumulator in the scratch
//
// k_eval_fold is a launch of its own (not folded into the next chunk's k_eval_idx): the last chunk needs it
// anyway, and one shape for every chunk keeps the order of the sums in one place.
//
// No floating-point atomics anywhere: lane -> LDS row -> one thread per word sums its 16 rows in row order
// (fp64) -> k_eval_fold sums the workgroup records in workgroup order -> adds the chunk to the accumulator.
#include "common.hpp"
#include "learn.hpp"
#include "eval.hpp"

namespace dqnx {

namespace {

__device__ __forceinline__ void eval_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ __launch_bounds__(256) void k_eval_idx(EvalIdxArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const int64_t size = gld(&a.ctrl->ring_size), wptr = gld(&a.ctrl->ring_wptr);
    const int64_t cap = a.capacity;
    int64_t p = a.first + i;
    if (p > a.hi - 1) p = a.hi - 1;   // the ragged tail re-reads the range's last row: a full batch of valid rows
    if (p > size - 1) p = size - 1;   // (the host checked hi <= size against its mirror; never past the ring)
    if (p < 0) p = 0;
    const int64_t base = ((wptr - size) % cap + cap) % cap;
    a.idx[i] = (int32_t)p;
    a.phys[i] = (int32_t)((base + p) % cap);
}

// raw[st][b][o] = H_L[st][b][:] . W[o][:] + bias[o]: one wave per (16-row tile, stream), the MFMA k order of
// k_head's step (1), operands straight from global memory (K = F <= 256, 16 outputs)
__global__ __launch_bounds__(64) void k_eval_head(EvalHeadArgs a) {
    const int lane = threadIdx.x, i = lane & 15, g = lane >> 4;
    const int st = a.stream_of[blockIdx.y];
    const int b0 = blockIdx.x * 16, nb = min(16, a.Bl - b0);
    const int F = a.F;
    const float* W = st == 2 ? a.Wt : a.Wo;
    const float* hrow = a.H + ((int64_t)st * a.Bl + b0 + (i < nb ? i : nb - 1)) * F;
    const float* wrow = W + head_w_off(a.head_kind, i < a.NH ? i : 0, F);
    const bool wreal = i < a.NH;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kk = 0; kk < F; kk += 16) {
        const float4 av = ld4(hrow + kk + 4 * g);
        float bx = gld(wrow + kk + 4 * g), by = gld(wrow + kk + 4 * g + 1), bz = gld(wrow + kk + 4 * g + 2),
              bw = gld(wrow + kk + 4 * g + 3);   // (a dueling head's advantage rows are not 16-byte aligned)
        if (!wreal) bx = by = bz = bw = 0.f;
        acc = mfma16x16x4(av.x, bx, acc);
        acc = mfma16x16x4(av.y, by, acc);
        acc = mfma16x16x4(av.z, bz, acc);
        acc = mfma16x16x4(av.w, bw, acc);
    }
    const float bias = wreal ? gld(W + head_b_off(a.head_kind, i, F, a.A)) : 0.f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int b = 4 * g + r;
        if (b < nb) a.raw[((int64_t)st * a.Bl + b0 + b) * 16 + i] = acc[r] + bias;
    }
}

// 16 rows per workgroup, 16 lanes per row, head slot j in lane j: the head part of k_head_bwd without the
// weights and the dZ chain.  TRANS: the transition scalars from the forward's float4 records, else through
// the slot table.  DISC: the row's own discount (n-step engines).
constexpr int EV_F = 10;   // floats per LDS row: lb, |delta|, delta, q_a, v, gap, agap, rew, y, done
template <bool TRANS, bool DISC>
__global__ __launch_bounds__(256) void k_eval_rows(EvalRowsArgs a) {
    __shared__ float fv[16][EV_F + 1];
    __shared__ int iv[16][3];   // greedy, action, real
    // every argument the prologue loads read: one wait (DQNX_KERNARG, common.hpp)
    asm volatile("" ::DQNX_KERNARG(a.Bl), DQNX_KERNARG(a.A), DQNX_KERNARG(a.valid), DQNX_KERNARG(a.head_kind),
                 DQNX_KERNARG(a.dbl), DQNX_KERNARG(a.raw), DQNX_KERNARG(a.trans), DQNX_KERNARG(a.phys),
                 DQNX_KERNARG(a.act), DQNX_KERNARG(a.rew), DQNX_KERNARG(a.done), DQNX_KERNARG(a.disc));
    const int tid = threadIdx.x, hb = tid >> 4, hj = tid & 15;
    const int b0 = blockIdx.x * 16;
    const int A = a.A;
    const int b = b0 + hb;
    const int bc = b < a.Bl ? b : a.Bl - 1;   // (every row of the batch holds a valid row's forward)
    const bool real = b < a.valid;

    // (0) every independent load first
    const int64_t base = (int64_t)bc * 16 + hj;
    const float r0 = gld(a.raw + base);
    const float r1 = a.dbl ? gld(a.raw + (int64_t)a.Bl * 16 + base) : 0.f;
    const float r2 = gld(a.raw + (int64_t)2 * a.Bl * 16 + base);
    int act;
    float rew, done;
    if constexpr (TRANS) {
        const float4 tr = a.trans[bc];
        act = __float_as_int(tr.x);
        rew = tr.y;
        done = tr.z;
    } else {
        const int32_t slot = gld(a.phys + bc);
        act = gld(a.act + slot);
        rew = gld(a.rew + slot);
        done = gld(a.done + slot);
    }
    float gm = a.gamma;
    if constexpr (DISC) gm = gld(a.disc + bc);
    if (act < 0 || act >= A) act = 0;

    // (1) Q of this lane's action slot (valid for hj < A), k_head_bwd's order
    const bool duel = a.head_kind == DQNX_HEAD_DUELING;
    auto qval = [&](float r) {
        if (!duel) return r;
        const float v = __shfl(r, 0, 16);
        const float adv = __shfl(r, hj + 1 < 16 ? hj + 1 : 15, 16);
        float sum = (hj >= 1 && hj <= A) ? r : 0.f;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 16);
        return eval_dueling(v, adv, sum, A);
    };
    const float q0 = qval(r0), q1 = qval(r1), q2 = qval(r2);
    auto argmax16 = [&](float q, int& bi) {   // first maximum over the lanes hj < A
        float bv = hj < A ? q : -INFINITY;
        bi = hj;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, 16);
            const int oi = __shfl_xor(bi, m, 16);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        return bv;
    };
    float qn;
    if (!a.dbl) {
        float mx = hj < A ? q2 : -INFINITY;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, 16));
        qn = mx;
    } else {
        int bi;
        (void)argmax16(q1, bi);
        qn = __shfl(q2, bi, 16);
    }
    const float y = eval_target(rew, done, gm, qn);
    const float qa = __shfl(q0, act, 16);
    const float delta = eval_delta(y, qa);
    const float lb = eval_huber(delta);
    int g;
    const float v = argmax16(q0, g);
    float second = (hj < A && hj != g) ? q0 : -INFINITY;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) second = fmaxf(second, __shfl_xor(second, m, 16));
    const float ev = hj < A ? cql_exp(q0, v) : 0.f;
    float sm = ev;
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) sm += __shfl_xor(sm, m, 16);
    const float gap = cql_gap(v, sm, qa);
    const float agap = eval_action_gap(v, second, A);

    if (hj == 0) {
        fv[hb][0] = lb;
        fv[hb][1] = fabsf(delta);
        fv[hb][2] = delta;
        fv[hb][3] = qa;
        fv[hb][4] = v;
        fv[hb][5] = gap;
        fv[hb][6] = agap;
        fv[hb][7] = rew;
        fv[hb][8] = y;
        fv[hb][9] = done;
        iv[hb][0] = g;
        iv[hb][1] = act;
        iv[hb][2] = real ? 1 : 0;
        if (real && a.rows_out)
            *reinterpret_cast<float4*>(a.rows_out + (int64_t)b * 4) = make_float4((float)g, qa, v, delta);
    }
    eval_lds_barrier();

    // (2) the workgroup's record: one thread per 8-byte word, the 16 rows in row order
    EvalPartial* out = a.part + blockIdx.x;
    if (tid < kEvalSums) {
        double s = 0.0;
        for (int r = 0; r < 16; r++) {
            if (!iv[r][2]) continue;
            const double x = (double)fv[r][tid];
            s += tid == 2 ? x * x : x;   // (an fp32 x fp32 product is exact in fp64)
        }
        out->sum[tid] = s;
    } else if (tid == kEvalSums) {
        double m = 0.0;
        for (int r = 0; r < 16; r++)
            if (iv[r][2]) m = fmax(m, (double)fv[r][1]);
        out->max_abs_delta = m;
    } else if (tid == kEvalSums + 1) {
        double m = -INFINITY;
        for (int r = 0; r < 16; r++)
            if (iv[r][2]) m = fmax(m, (double)fv[r][4]);
        out->max_v = m;
    } else if (tid == kEvalSums + 2) {
        double m = INFINITY;
        for (int r = 0; r < 16; r++)
            if (iv[r][2]) m = fmin(m, (double)fv[r][4]);
        out->min_v = m;
    } else if (tid == kEvalSums + 3) {
        int64_t n = 0;
        for (int r = 0; r < 16; r++) n += (iv[r][2] && iv[r][0] == iv[r][1]) ? 1 : 0;
        out->agree_rows = n;
    } else if (tid == kEvalSums + 4) {
        int64_t n = 0;
        for (int r = 0; r < 16; r++) n += (iv[r][2] && fv[r][9] != 0.f) ? 1 : 0;
        out->done_rows = n;
    } else if (tid >= 64 && tid < 64 + 2 * DQNX_STATS_MAX_ACTIONS) {
        const int w = tid - 64, j = w & (DQNX_STATS_MAX_ACTIONS - 1), which = w >> 4;
        int64_t n = 0;
        for (int r = 0; r < 16; r++) n += (iv[r][2] && iv[r][which] == j) ? 1 : 0;
        (which ? out->taken_hist : out->greedy_hist)[j] = n;
    }
}

// One workgroup, one thread per 8-byte word of the record: the workgroup records in workgroup order, then the
// chunk into the accumulator (set by the first chunk).  The last chunk also stores `rows`.
__global__ __launch_bounds__(64) void k_eval_fold(EvalFoldArgs a) {
    const int w = threadIdx.x;
    if (w >= kEvalWords) return;
    const int kind = w < kEvalSums ? 0 : (w < kEvalSums + 2 ? 1 : (w == kEvalSums + 2 ? 2 : 3));
    int64_t* accw = reinterpret_cast<int64_t*>(a.acc) + 1 + w;
    // the records' words in batches of kFoldBatch loads in flight, added in workgroup order (one dependent
    // load per record measured 30 us for the 64 records of B = 1024: a memory round trip each)
    constexpr int kFoldBatch = 16;
    int64_t si = 0;
    double s = kind == 0 ? 0.0 : (kind == 2 ? (double)INFINITY : (w == kEvalSums ? 0.0 : -(double)INFINITY));
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

int launch_eval_idx(const EvalIdxArgs& a, hipStream_t s) {
    if (!a.ctrl || !a.idx || !a.phys) return set_error(DQNX_EINVAL, "eval idx: null buffer");
    if (a.n < 1 || a.capacity < 1 || a.lo < 0 || a.lo >= a.hi || a.first < a.lo || a.first >= a.hi)
        return set_error(DQNX_EINVAL, "eval idx: bad range");
    DQNX_LAUNCH(k_eval_idx, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_eval_head(const EvalHeadArgs& a, hipStream_t s) {
    if (!a.H || !a.Wo || !a.Wt || !a.raw) return set_error(DQNX_EINVAL, "eval head: null buffer");
    if (a.Bl < 1 || a.F < 16 || a.F % 16 || a.NH < 1 || a.NH > 16 || a.A < 1 || a.A > a.NH || a.nstreams < 2 ||
        a.nstreams > 3)
        return set_error(DQNX_EINVAL, "eval head: bad shape");
    for (int z = 0; z < a.nstreams; z++)
        if (a.stream_of[z] < 0 || a.stream_of[z] > 2) return set_error(DQNX_EINVAL, "eval head: bad stream");
    if (((uintptr_t)a.H) & 15) return set_error(DQNX_EINVAL, "eval head: misaligned buffer");
    DQNX_LAUNCH(k_eval_head, dim3((a.Bl + 15) / 16, a.nstreams), dim3(64), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_eval_rows(const EvalRowsArgs& a, hipStream_t s) {
    if (!a.raw || !a.part) return set_error(DQNX_EINVAL, "eval rows: null buffer");
    if (!a.trans && (!a.phys || !a.act || !a.rew || !a.done)) return set_error(DQNX_EINVAL, "eval rows: null buffer");
    if (a.Bl < 1 || a.valid < 1 || a.valid > a.Bl || a.A < 1 || a.A > DQNX_STATS_MAX_ACTIONS || a.NH < a.A || a.NH > 16)
        return set_error(DQNX_EINVAL, "eval rows: bad shape");
    if (((uintptr_t)a.rows_out | (uintptr_t)a.trans) & 15) return set_error(DQNX_EINVAL, "eval rows: misaligned buffer");
    const dim3 grid((a.Bl + 15) / 16), block(256);
    if (a.trans) {
        if (a.disc) DQNX_LAUNCH((k_eval_rows<true, true>), grid, block, 0, s, a);
        else DQNX_LAUNCH((k_eval_rows<true, false>), grid, block, 0, s, a);
    } else {
        if (a.disc) DQNX_LAUNCH((k_eval_rows<false, true>), grid, block, 0, s, a);
        else DQNX_LAUNCH((k_eval_rows<false, false>), grid, block, 0, s, a);
    }
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

int launch_eval_fold(const EvalFoldArgs& a, hipStream_t s) {
    if (!a.part || !a.acc || a.nparts < 1) return set_error(DQNX_EINVAL, "eval fold: bad arguments");
    static_assert(kEvalWords <= 64, "k_eval_fold: one thread per word of the record");
    DQNX_LAUNCH(k_eval_fold, dim3(1), dim3(64), 0, s, a);
    DQNX_HIP_CHECK(hipGetLastError());
    return DQNX_OK;
}

}  // namespace dqnx
