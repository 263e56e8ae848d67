// Offline evaluation (include/dqnx.h "offline evaluation"): the per-row arithmetic of the evaluation sweep,
// shared by the device kernel (eval.hip, k_eval_rows: 16 lanes per row, slot j in lane j) and the host test
// hook (dqnx_eval_row, engine.cpp: one row serially through eval_row) so that both fold the same expressions,
// and the argument structs / launchers of eval.hip.
//
// Per row, from the raw head outputs of the streams online(s), online(s') [Double], target(s'), the clamped
// replay action a, the (n-step) reward R, done d and the row's discount disc:
//
//   q_j   = raw_j                                   linear head
//         = V + (A_j - (sum_j A_j) / A)             dueling head (the kernels may sum in different orders)
//   q'    = max_j qt_j  (DQN)  |  qt_[argmax_j qn_j] (Double, first maximum)
//   y     = R + ((1 - d) * disc) * q'               the head kernels' fp32 order
//   delta = y - q_a
//   lb    = |delta| < 1 ? (0.5 |delta|) |delta| : |delta| - 0.5          Huber, beta = 1, unweighted
//   v     = max_j q_j,  g = the first j with q_j == v
//   gap   = (v + logf(sum_j expf(q_j - v))) - q_a                        cql.hpp's forms
//   agap  = v - max_{j != g} q_j                    0 when A = 1
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dqnx.h"
#include "cql.hpp"

namespace dqnx {

__host__ __device__ inline float eval_dueling(float v, float adv, float sum, int A) {
    const float mean = sum / (float)A;
    return v + (adv - mean);
}

// y = rew + ((1 - done) * disc) * q'
__host__ __device__ inline float eval_target(float rew, float done, float disc, float qn) {
    const float t1 = 1.f - done;
    const float t2 = t1 * disc;
    const float t3 = t2 * qn;
    return rew + t3;
}

__host__ __device__ inline float eval_delta(float y, float qa) { return y - qa; }

// smooth_l1(q_a, y), beta = 1, as the head kernels write it
__host__ __device__ inline float eval_huber(float delta) {
    const float z = fabsf(delta);
    return z < 1.f ? (0.5f * z) * z / 1.f : z - 0.5f;
}

__host__ __device__ inline float eval_action_gap(float v, float second, int A) { return A > 1 ? v - second : 0.f; }

struct EvalRow {
    int g, act;
    float qa, v, delta, lb, gap, agap, y;
};

// Q of one stream, serially: raw[0 .. NH) -> q[0 .. A)
__host__ __device__ inline void eval_q(const float* raw, int head_kind, int A, float* q) {
    if (head_kind == DQNX_HEAD_DUELING) {
        float sum = 0.f;
        for (int j = 0; j < A; j++) sum += raw[1 + j];
        for (int j = 0; j < A; j++) q[j] = eval_dueling(raw[0], raw[1 + j], sum, A);
    } else {
        for (int j = 0; j < A; j++) q[j] = raw[j];
    }
}

// One row, serially (A = 1 .. 16, act already clamped into [0, A); raw1 is read only when dbl)
__host__ __device__ inline EvalRow eval_row(const float* raw0, const float* raw1, const float* raw2, int head_kind, int A,
                                            bool dbl, int act, float rew, float done, float disc) {
    float q0[16], q1[16], q2[16];
    eval_q(raw0, head_kind, A, q0);
    eval_q(raw2, head_kind, A, q2);
    float qn;
    if (!dbl) {
        qn = q2[0];
        for (int j = 1; j < A; j++) qn = fmaxf(qn, q2[j]);
    } else {
        eval_q(raw1, head_kind, A, q1);
        int best = 0;
        for (int j = 1; j < A; j++)
            if (q1[j] > q1[best]) best = j;
        qn = q2[best];
    }
    EvalRow r;
    r.act = act;
    r.y = eval_target(rew, done, disc, qn);
    r.qa = q0[act];
    r.delta = eval_delta(r.y, r.qa);
    r.lb = eval_huber(r.delta);
    int g = 0;
    for (int j = 1; j < A; j++)
        if (q0[j] > q0[g]) g = j;
    r.g = g;
    r.v = q0[g];
    float second = -INFINITY, s = 0.f;
    for (int j = 0; j < A; j++) {
        if (j != g) second = fmaxf(second, q0[j]);
        s += cql_exp(q0[j], r.v);
    }
    r.gap = cql_gap(r.v, s, r.qa);
    r.agap = eval_action_gap(r.v, second, A);
    return r;
}

// ---- eval.hip ------------------------------------------------------------------------------------------
// One fp64 record per workgroup of k_eval_rows (16 rows), and the layout of the sums k_eval_fold carries:
// the words of dqnx_eval_result behind `rows`, in its order.
constexpr int kEvalSums = 9;   // lb, |delta|, delta^2, q_a, v, gap, action gap, reward, y
struct EvalPartial {
    double sum[kEvalSums];
    double max_abs_delta, max_v, min_v;
    int64_t agree_rows, done_rows;
    int64_t greedy_hist[DQNX_STATS_MAX_ACTIONS], taken_hist[DQNX_STATS_MAX_ACTIONS];
};
constexpr int kEvalWords = (int)(sizeof(EvalPartial) / 8);
static_assert(sizeof(EvalPartial) == 8 * (kEvalSums + 3 + 2 + 2 * DQNX_STATS_MAX_ACTIONS), "EvalPartial is 8-byte words");
static_assert(sizeof(dqnx_eval_result) == sizeof(EvalPartial) + 8, "dqnx_eval_result = rows + the partial's words");

struct EvalIdxArgs {
    int64_t lo, hi, first;   // first = lo + chunk * B
    int n;                   // B
    int64_t capacity;
    const dqnx_ctrl* ctrl;
    int32_t *idx, *phys;     // the scratch table
};

// the per-layer routes' head GEMM: raw[st] = H_L[st] . W_head^T + b, the fused plan's [3][Bl][16] layout
struct EvalHeadArgs {
    int Bl, F, A, NH, head_kind, nstreams;
    int stream_of[3];
    const float* H;          // [3][Bl][F]
    const float *Wo, *Wt;    // the online / target head parameter blocks
    float* raw;
};

struct EvalRowsArgs {
    int Bl, A, NH, head_kind, dbl, valid;
    float gamma;
    const float* raw;        // [3][Bl][16]
    const float4* trans;     // {act, rew, done, 0} per row (fused plan), or null: through phys
    const int32_t* phys;
    const int32_t* act;
    const float *rew, *done;
    const float* disc;       // n-step engines: fp32(gamma^m) per row, else null
    float* rows_out;         // this chunk's [valid][4] (g, q_a, v, delta), or null
    EvalPartial* part;       // [ceil(Bl / 16)]
};

struct EvalFoldArgs {
    int nparts, first, last;   // first chunk: the accumulator is set, not added to
    int64_t rows;
    const EvalPartial* part;
    dqnx_eval_result* acc;
};

int launch_eval_idx(const EvalIdxArgs& a, hipStream_t s);
int launch_eval_head(const EvalHeadArgs& a, hipStream_t s);
int launch_eval_rows(const EvalRowsArgs& a, hipStream_t s);
int launch_eval_fold(const EvalFoldArgs& a, hipStream_t s);

}  // namespace dqnx
