// Fitted Q evaluation (include/dqnx.h "fitted Q evaluation"): the per-row arithmetic of the two sweeps, shared
// by the device kernels (fqe.hip: 16 lanes per row, slot j in lane j) and the host test hook (dqnx_fqe_row,
// engine.cpp: one row serially) so that both fold the same expressions, and the argument structs / launchers
// of fqe.hip.  The Q row, target, delta and Huber forms are eval.hpp's.
//
//   pi(s)    = the first j with q_j = max_j q_j       q = the policy's Q row after the head's aggregate
//   q_pi     = Q_online(s, pi(s))
//   y        = r + ((1 - d) * gamma) * Q_target(s', pi(s'))
//   delta_pi = y - Q_online(s, a)
#pragma once
#include "eval.hpp"

namespace dqnx {

// the first maximum of q[0 .. A) (torch.argmax's tie rule; the kernels' butterflies keep the lower lane)
__host__ __device__ inline int fqe_argmax(const float* q, int A) {
    int best = 0;
    for (int j = 1; j < A; j++)
        if (q[j] > q[best]) best = j;
    return best;
}

// a table entry as the kernels read it: outside [0, A) -> 0
__host__ __device__ inline int fqe_clamp(int a, int A) { return (a < 0 || a >= A) ? 0 : a; }

struct FqeRow {
    float qpi, y, delta, lb;
};

// One row, serially: raw0 = online(s), raw2 = target(s'); act, ps, pn already inside [0, A)
__host__ __device__ inline FqeRow fqe_row(const float* raw0, const float* raw2, int head_kind, int A, int act, float rew,
                                          float done, float gamma, int ps, int pn) {
    float q0[16], q2[16];
    eval_q(raw0, head_kind, A, q0);
    eval_q(raw2, head_kind, A, q2);
    FqeRow r;
    r.qpi = q0[ps];
    r.y = eval_target(rew, done, gamma, q2[pn]);
    r.delta = eval_delta(r.y, q0[act]);
    r.lb = eval_huber(r.delta);
    return r;
}

// ---- fqe.hip -------------------------------------------------------------------------------------------
// One record per workgroup of k_fqe_rows (16 rows): the words of dqnx_fqe_result behind `rows`, in its order.
constexpr int kFqeSums = 4;   // q_pi, q_pi over start rows, |delta_pi|, huber
struct FqePartial {
    int64_t start_rows;
    double sum[kFqeSums];
    double max_q, min_q;
};
constexpr int kFqeWords = (int)(sizeof(FqePartial) / 8);
static_assert(sizeof(FqePartial) == 8 * (1 + kFqeSums + 2), "FqePartial is 8-byte words");
static_assert(sizeof(dqnx_fqe_result) == sizeof(FqePartial) + 8, "dqnx_fqe_result = rows + the partial's words");
static_assert(sizeof(FqePartial) <= sizeof(EvalPartial), "the sweeps share the evaluation scratch layout");

struct PolicyRowsArgs {
    int Bl, A, head_kind, valid;
    int64_t slots;           // table slots (= capacity): a slot outside stores nothing
    const float* raw;        // [3][Bl][16]: streams 0 (online(s)) and 1 (online(s')) are read
    const int32_t* phys;     // the chunk's ring slots
    int32_t* table;          // [slots][2]
};

struct FqeRowsArgs {
    int Bl, A, head_kind, valid, n_env;
    float gamma;
    int64_t first, capacity;   // the chunk's first logical position; ring capacity (= table slots)
    const dqnx_ctrl* ctrl;     // ring_size / ring_wptr: the predecessor's slot
    const float* raw;          // [3][Bl][16]: streams 0 and 2
    const float4* trans;       // {act, rew, done, 0} per row (fused plan), or null: through phys
    const int32_t* phys;
    const int32_t* act;
    const float *rew, *done;   // ring arrays by slot (done also for the predecessor)
    const int32_t* table;
    float* rows_out;           // this chunk's [valid][2] (q_pi, delta_pi), or null
    FqePartial* part;          // [ceil(Bl / 16)]
};

struct FqeFoldArgs {
    int nparts, first, last;   // first chunk: the accumulator is set, not added to
    int64_t rows;
    const FqePartial* part;
    dqnx_fqe_result* acc;
};

int launch_policy_rows(const PolicyRowsArgs& a, hipStream_t s);
int launch_fqe_rows(const FqeRowsArgs& a, hipStream_t s);
int launch_fqe_fold(const FqeFoldArgs& a, hipStream_t s);

}  // namespace dqnx
