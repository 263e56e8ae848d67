/*
 * dqnx.h -- C ABI of the MI355X-native DQN learn-step engine (libdqnx.so).
 *
 * Drop-in boundary for the hot path of youcefMehamlia/Multimodal-DRL-RMC
 * (R: = /root/reference/).  The reference has no FFI: its "operator API" is the
 * duck-typed Python of dqn.agent / dqn.network / dqn.replay_memory, which the
 * Python host shim (multimodal-drl-rmc_amd/dqn/) keeps, calling the entry points
 * below through ctypes.  Each entry point names the reference interface it
 * replaces.  Plain C: pointers, sizes, enums; no torch types.  Streams are
 * hipStream_t passed as void*.  All device work is enqueued on the caller's
 * stream; nothing here synchronises unless its comment says so.
 *
 * Error convention: every function returns int (0 = DQNX_OK, < 0 = invalid
 * argument/state, > 0 = DQNX_ERR_HIP + hipError_t).  dqnx_last_error() returns a
 * thread-local message for the last failure.  No C++ exception crosses the ABI.
 *
 * Memory: the engine owns no device memory.  The caller allocates ONE device arena
 * of dqnx_engine_arena_bytes() bytes and binds it; dqnx_engine_buffer() gives the
 * offset of every region inside it (parameters, Adam moments, replay ring, SumTree,
 * control block, workspace), so a host framework can view them (the Python shim
 * makes torch views so state_dict()/load_state_dict() keep working).
 */
#ifndef DQNX_H
#define DQNX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DQNX_ABI_VERSION 5

/* ---- status codes ---------------------------------------------------------------- */
#define DQNX_OK 0
#define DQNX_EINVAL (-1)      /* bad argument */
#define DQNX_ESTATE (-2)      /* call not valid in the engine's current state (e.g. unbound) */
#define DQNX_EUNSUPPORTED (-3)/* configuration outside what the engine implements */
#define DQNX_EDEVICE (-4)     /* device-side sticky error word was set (see dqnx_ctrl.error) */
#define DQNX_ERR_HIP 1000     /* DQNX_ERR_HIP + hipError_t */

/* ---- enums ------------------------------------------------------------------------- */
enum dqnx_net_kind { DQNX_NET_MLP = 0, DQNX_NET_TWO_STREAM = 1 };
enum dqnx_head_kind { DQNX_HEAD_LINEAR = 0, DQNX_HEAD_DUELING = 1 };
enum dqnx_activation { DQNX_ACT_RELU = 0, DQNX_ACT_ELU = 1 };
/* Arithmetic of the network GEMMs.  FP32 is the reference's (parity within 1e-5).  BF16
 * (BASELINE config 5): forward and dZ-chain GEMM operands rounded to bf16 (RNE), fp32
 * accumulate; bias, activations, TD target, Huber, weight gradients, Adam and the master
 * weights stay fp32.  MLP networks only. */
enum dqnx_compute_dtype { DQNX_COMPUTE_FP32 = 0, DQNX_COMPUTE_BF16 = 1 };
/* Learner algorithm = which Agent.learn() runs:
 *   DQNX_ALGO_DQN        SimpleAgent.learn          R:dqn/agent.py:166-185  (DQNAgent)
 *   DQNX_ALGO_DOUBLE     DoubleAgent.learn          R:dqn/agent.py:204-226  (DoubleDQNAgent,
 *                                                                            DuelingDoubleDQNAgent)
 *   DQNX_ALGO_PER_DOUBLE PerDoubleAgent.learn       R:dqn/agent.py:245-272  (PerDuelingDoubleDQNAgent) */
enum dqnx_algo { DQNX_ALGO_DQN = 0, DQNX_ALGO_DOUBLE = 1, DQNX_ALGO_PER_DOUBLE = 2 };

/* ---- network description (replaces nn_conf_func / network_config) ----------------
 * MLP:        R:env/custom_env/macro with lane/dqn_config.py:58-104
 *             nn.Sequential(Linear(D,h0), act, Linear(h0,h1), act, ...)
 * TWO_STREAM: TwoStreamHybridNetwork R:env/dqn_config.py:66-143 (network_config :148-193)
 * heads:      DeepQNetwork fc_out (R:dqn/network.py:50-65), DuelingDeepQNetwork
 *             fc_val/fc_adv + aggregate (R:dqn/network.py:77-96). */
#define DQNX_MAX_DENSE 6
#define DQNX_MAX_CONV 4
#define DQNX_NSTEP_MAX 16      /* largest dqnx_config.n_step */
typedef struct dqnx_net_desc {
    int32_t kind;              /* dqnx_net_kind */
    int32_t head;              /* dqnx_head_kind */
    int32_t activation;        /* dqnx_activation of the body (MLP: ReLU, hybrid: ELU) */
    int32_t obs_dim;           /* D: length of one flat observation */
    int32_t n_actions;         /* A */
    int32_t n_dense;           /* number of body Linear layers (MLP) / dense_stream layers */
    int32_t dense[DQNX_MAX_DENSE];
    /* TWO_STREAM only: obs = [macro (macro_len) | micro grid viewed as (c,h,w)] */
    int32_t macro_len;
    int32_t micro_c, micro_h, micro_w;
    int32_t n_conv;
    int32_t conv_out[DQNX_MAX_CONV], conv_kh[DQNX_MAX_CONV], conv_kw[DQNX_MAX_CONV];
    int32_t conv_sh[DQNX_MAX_CONV], conv_sw[DQNX_MAX_CONV];
} dqnx_net_desc;

/* One parameter tensor of the flat parameter vector, in torch named_parameters()
 * order (= state_dict order, = the order Adam iterates).  Names are the reference's
 * state_dict keys (e.g. "net.0.weight", "fc_adv.bias"). */
typedef struct dqnx_param_info {
    char name[48];
    int64_t offset;            /* element offset in the flat fp32 vector */
    int64_t numel;
    int32_t ndim;
    int32_t shape[4];
} dqnx_param_info;

/* Total fp32 parameter count and tensor count of a network (host only, no GPU). */
int dqnx_net_param_count(const dqnx_net_desc* net, int64_t* n_params, int32_t* n_tensors);
int dqnx_net_param_info(const dqnx_net_desc* net, int32_t index, dqnx_param_info* out);

/* ---- engine configuration (replaces the Agent constructor kwargs, R:dqn/agent.py:19-52,
 *      with the hyper-parameters of R:env/dqn_config.py:26-56) -------------------- */
typedef struct dqnx_config {
    dqnx_net_desc net;
    int32_t algo;              /* dqnx_algo */
    int32_t batch;             /* global minibatch = batch_size (k of random.sample) */
    int32_t world_size;        /* data-parallel ranks (1 = single GPU) */
    int32_t rank;              /* this rank: processes samples [rank*batch/world, (rank+1)*batch/world) */
    int32_t n_step;            /* n-step returns: 1 (dqnx_config_defaults) .. DQNX_NSTEP_MAX; fixed at create, sizes
                                  the arena, never in the state blob ("n-step returns" below).  It lies in the
                                  four bytes that were padding in front of `capacity`: the struct's size and
                                  every other field's offset are what they were, and dqnx_config_defaults
                                  (which every caller fills the struct through) has always written them */
    int64_t capacity;          /* buffer_size (deque maxlen / SumTree capacity) */
    /* hyper-parameters are doubles, like the reference's Python floats; the engine casts
     * them to fp32 exactly where torch does (tensor * Python float). */
    double gamma;              /* discount */
    double lr;                 /* Adam lr */
    double beta1, beta2, adam_eps;  /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
    double tau;                /* target_soft_update_tau */
    int32_t n_env;             /* soft update uses tau*n_env (R:dqn/agent.py:108-109) */
    int32_t local_sampling;    /* world_size > 1, uniform replay only: 0 = every rank draws the same
                                  global minibatch of `batch` (bit-exact with one GPU) and takes its
                                  shard; 1 = each rank draws its own batch/world_size positions from
                                  its own RNG stream (plain data parallelism; O(batch/world) sampling) */
    /* ReplayMemoryPrioritized constants (R:dqn/replay_memory.py:49-54) */
    double per_eps, per_alpha, per_max_priority;
    double per_beta_start, per_beta_end, per_beta_steps;   /* beta = interp(step,[0,steps],[start,end]) */
    int32_t compute_dtype;     /* dqnx_compute_dtype (ABI 2) */
    int32_t per_numpy121;      /* PER tree arithmetic of the reference's pinned numpy 1.21: 0 (default) =
                                  numpy >= 2 (NEP 50: `change` and the ancestor sums in float64, exact);
                                  1 = numpy 1.21 value-based casting: update_batch_priorities' float32
                                  `change` and float32-rounded ancestor sums, applied in update order
                                  (R:dqn/utils/sum_tree.py:18, 31-32; R:bin/environment.yml pins 1.21) */
} dqnx_config;

/* Fill cfg with the reference's HYPER_PARAMS defaults for the given network. */
void dqnx_config_defaults(dqnx_config* cfg);

/* ---- device control block (lives in the arena; layout is ABI) ------------------- */
typedef struct dqnx_ctrl {
    uint32_t py_mt[625];       /* CPython random state: random.getstate()[1] (624 words + index) */
    uint32_t np_mt[625];       /* numpy legacy RandomState: get_state()[1] keys + [2] pos */
    int64_t ring_size;         /* len(replay deque) / SumTree.size */
    int64_t ring_wptr;         /* next physical write slot (SumTree.data_pointer) */
    int64_t adam_step;         /* torch Adam state['step'] (same for every tensor) */
    int64_t agent_step;        /* agent.step * n_env handed to PER sample_transitions */
    int64_t per_max_idx;       /* SumTree.max_priority_index (tree index) */
    int64_t per_min_idx;       /* SumTree.min_priority_index (tree index) */
    float loss;                /* loss of the last learn step (global batch mean) */
    int32_t error;             /* sticky device error code, 0 = ok */
    float adam_step_size;      /* -lr / bias_correction1 of the current step (fp32) */
    float adam_bc2_sqrt;       /* sqrt(bias_correction2) of the current step (fp32) */
    double per_beta;           /* beta used by the last PER sample */
    int64_t reserved[8];
} dqnx_ctrl;

/* device error codes written to dqnx_ctrl.error */
#define DQNX_DEVERR_SAMPLE_TOO_LARGE 1   /* random.sample: k > n (ValueError) */
#define DQNX_DEVERR_EMPTY_TREE 2         /* PER sample with total priority 0 */
#define DQNX_DEVERR_PER_HANDOFF 3        /* internal: a PER update hand-off inside one launch timed out */
#define DQNX_DEVERR_FWD_PAIR_HANDOFF 4   /* internal: the paired-column forward's H_1 hand-off timed out */
/* internal: a write outside its range was skipped (bounds checks on the DP-bucket write paths) */
#define DQNX_DEVERR_BOUNDS_ADAM_WIDE 16  /*   k_adam4 wide path: a float4 outside [e0, n_params) of the launch */
#define DQNX_DEVERR_BOUNDS_ADAM_PERM 17  /*   k_adam4 wide path: a permuted conv-weight copy outside the range */
#define DQNX_DEVERR_BOUNDS_MICRO_DW 18   /*   k_micro_dw: a split-K slab tile outside its conv's slabs */
/* n-step engines: the gather launch met a ring size / write pointer / sampled slot outside the ring (the row
 * then reads a one-position window at a clamped slot: every access stays inside the ring) */
#define DQNX_DEVERR_NSTEP_STATE 19
/* fitted Q evaluation: a sampled row's entry of the target-policy table (dqnx_set_target_policy) lies outside
 * [0, n_actions); the row was computed with action 0 */
#define DQNX_DEVERR_TPOL_ACTION 20

/* ---- engine lifetime --------------------------------------------------------------- */
typedef struct dqnx_engine dqnx_engine;

int dqnx_engine_create(const dqnx_config* cfg, dqnx_engine** out);
int dqnx_engine_destroy(dqnx_engine* e);
/* Bytes of the single device arena the engine needs (host only). */
int dqnx_engine_arena_bytes(const dqnx_engine* e, uint64_t* bytes);

/* Arena regions. */
enum dqnx_buffer {
    DQNX_BUF_PARAMS = 0,       /* online network flat fp32 params (named_parameters order) */
    DQNX_BUF_TARGET_PARAMS,    /* target network flat params */
    DQNX_BUF_GRADS,            /* flat fp32 gradient of the last learn step (all-reduced under DP) */
    DQNX_BUF_ADAM_M,           /* Adam exp_avg */
    DQNX_BUF_ADAM_V,           /* Adam exp_avg_sq */
    DQNX_BUF_CTRL,             /* dqnx_ctrl */
    DQNX_BUF_RING_OBS,         /* [capacity][obs_stride] fp32 */
    DQNX_BUF_RING_NEXT_OBS,    /* [capacity][obs_stride] fp32 */
    DQNX_BUF_RING_ACT,         /* [capacity] int32 */
    DQNX_BUF_RING_REW,         /* [capacity] fp32 */
    DQNX_BUF_RING_DONE,        /* [capacity] fp32 (0/1) */
    DQNX_BUF_SUMTREE,          /* [2*capacity-1] fp64 (PER only, else 0 bytes) */
    DQNX_BUF_BATCH_IDX,        /* [2][batch] int32: sampled logical replay positions / tree leaves;
                                  slot 0 unless DQNX_STEP_PREFETCH alternates the slots */
    DQNX_BUF_Q,                /* [3][batch_local][n_actions] fp32: Q online(s), online(s'), target(s') */
    DQNX_BUF_TD,               /* [3][batch_local] fp32: targets y, q(s,a), |y - q(s,a)| */
    DQNX_BUF_IS_WEIGHTS,       /* [batch] fp32 PER importance weights */
    DQNX_BUF_WORKSPACE,        /* everything else (activations, partial slabs, scratch) */
    DQNX_BUF_PER_ABS_TD,       /* [batch] fp32 |targets - q(s,a)| of the GLOBAL minibatch (PER only):
                                  each rank's learn step writes its shard; under DP the caller
                                  all-gathers it in place before dqnx_apply_grads */
    DQNX_BUF_LEARN_STATS,      /* one dqnx_learn_stats (ABI 5): accumulated by DQNX_STEP_STATS steps; not
                                  training state (never in the state blob) */
    DQNX_BUF_GRAD_CLIP,        /* one dqnx_grad_clip_info, then the clipping launches' scratch (the step's
                                  coefficient at byte 64, the sum-of-squares partials from byte 128): written by
                                  clipped steps only; not training state (never in the state blob) */
    DQNX_BUF_COUNT
};
int dqnx_engine_buffer(const dqnx_engine* e, int32_t which, uint64_t* offset, uint64_t* bytes);
/* Row stride (in floats) of the replay observation rings (>= obs_dim, multiple of 4). */
int dqnx_engine_obs_stride(const dqnx_engine* e, int32_t* stride);
/* Bind the caller-allocated arena (device pointer, 256-byte aligned). */
int dqnx_engine_bind(dqnx_engine* e, void* arena, uint64_t bytes);
/* The caller wrote the parameters (DQNX_BUF_PARAMS / DQNX_BUF_TARGET_PARAMS) directly, e.g. a
 * checkpoint load through state_dict() views (R:dqn/network.py:37-47, R:dqn/agent.py:112-121):
 * the next learn step rebuilds the engine's derived weight layouts.  Host only, no device work.
 * (dqnx_soft_update / dqnx_hard_update / dqnx_engine_reset imply it.) */
int dqnx_params_modified(dqnx_engine* e);
/* Zero Adam moments, ring state, tree, control block (params untouched); stream-ordered. */
int dqnx_engine_reset(dqnx_engine* e, void* stream);
/* Use hipGraph capture/replay for learn steps (default OFF: measured on MI355X / ROCm 7.2, every
 * hipGraphLaunch leaves ~8.5 us between the previous graph's last kernel and its first one, while
 * back-to-back kernel launches on one stream leave ~0; eager steps are 3-4 us faster at every
 * configuration measured -- MLP B=1024 / 4096, PER, bf16 B=8192, two-stream). */
int dqnx_engine_set_graphs(dqnx_engine* e, int32_t enabled);

/* ---- replay ring: replaces ReplayMemoryNaive/Prioritized.store_transitions
 *      (R:dqn/replay_memory.py:30-36, :56-67) via Agent.store_transitions (R:dqn/agent.py:80-84).
 * Appends n transitions (evicting the oldest when full).  Pointers are host memory
 * (src_on_device = 0; up to 64 rows are copied into an engine-owned pinned block at once and sent
 * with one async copy -- the caller's arrays are free on return; larger pushes are copied with
 * hipMemcpyAsync and the call synchronises the stream) or device memory (src_on_device = 1).  obs rows are
 * obs_dim floats, contiguous.  done: 0/1 bytes.  Under PER new leaves get the current
 * max priority (1.0 when the tree is empty), exactly as the reference.
 * Row order: time-major, env-minor -- one time step is n_env consecutive rows, env 0 first (what
 * Agent.store_transitions hands over).  An n-step engine (n_step > 1) relies on it: the successor of a row
 * is the row n_env later, so there a push whose n is not a multiple of n_env returns DQNX_EINVAL (nothing
 * is written). */
int dqnx_replay_push(dqnx_engine* e, const float* obs, const int32_t* act, const float* rew,
                     const uint8_t* done, const float* next_obs, int32_t n, int32_t src_on_device,
                     void* stream);

/* ---- prioritised replay (DQNX_ALGO_PER_DOUBLE) ------------------------------------
 * The SumTree lives in DQNX_BUF_SUMTREE with the reference's layout (leaf of ring slot s
 * = tree index s + capacity - 1); its max/min priority indices in dqnx_ctrl.
 * dqnx_per_sample: ReplayMemoryPrioritized.sample_transitions(step) (R:dqn/replay_memory.py:69-92)
 *   -> ring slots into DQNX_BUF_BATCH_IDX slot 0, IS weights into DQNX_BUF_IS_WEIGHTS; consumes
 *   numpy global-state words from dqnx_ctrl.np_mt and advances dqnx_ctrl.agent_step by n_env.
 *   A PER learn step does this itself.
 * dqnx_per_update_priorities: update_batch_priorities(tree_indices, abs_td_errors)
 *   (R:dqn/replay_memory.py:94-98) for n (ring slot, |delta|) pairs in device memory, in order.
 *   A PER learn step does this itself (after the all-gather under DP: dqnx_apply_grads).
 * dqnx_set_agent_step: the `self.step * self.n_env` the next PER sample interpolates beta from
 *   (R:dqn/agent.py:247). */
int dqnx_per_sample(dqnx_engine* e, void* stream);
int dqnx_per_update_priorities(dqnx_engine* e, const int32_t* slots, const float* abs_td, int32_t n, void* stream);
int dqnx_set_agent_step(dqnx_engine* e, int64_t step_times_n_env, void* stream);

/* ---- RNG state exchange (Python random / numpy legacy global state) -------------- */
enum dqnx_rng { DQNX_RNG_PY = 0, DQNX_RNG_NP = 1 };
/* Upload 625 words (624 + index) into the control block (host pointer; stream-ordered,
 * the copy is complete when this returns). */
int dqnx_rng_set(dqnx_engine* e, int32_t which, const uint32_t* state625, void* stream);
/* Download 625 words; synchronises the stream. */
int dqnx_rng_get(dqnx_engine* e, int32_t which, uint32_t* state625, void* stream);
/* The same two copies, stream-ordered and WITHOUT a synchronisation: `state625` must be pinned
 * (page-locked) host memory that the caller keeps unchanged (set) / does not read (get) until the
 * copy has executed (e.g. an event recorded after it).  The drop-in Agent uses them to hand the
 * sampler's RNG to and from Python's global `random` / numpy state without a host round trip per
 * learn() (dqn/agent.py).  Same argument checks as dqnx_rng_set / dqnx_rng_get; refused while a
 * prefetched minibatch is pending. */
int dqnx_rng_set_async(dqnx_engine* e, int32_t which, const uint32_t* state625, void* stream);
int dqnx_rng_get_async(dqnx_engine* e, int32_t which, uint32_t* state625, void* stream);

/* The whole control block (both RNG states, ring size, loss, sticky error, ...) into PINNED host memory
 * (sizeof(dqnx_ctrl) bytes), stream-ordered and without a synchronisation: the drop-in Agent reads it
 * back after each launched learn step and checks the sticky error and its RNG mirror (below) at its
 * next synchronisation point, so a device error reaches the caller without a host round trip per step. */
int dqnx_ctrl_get_async(dqnx_engine* e, void* dst, void* stream);

/* ---- host-side RNG stream mirror (host only, no device work) -----------------------------------
 * The reference draws the minibatch inside Agent.learn() from the interpreter's global generators
 * (R:dqn/replay_memory.py:38-39 random.sample; :79-80 np.random.uniform once per sample), so the
 * caller's `random` / `np.random` have moved on when learn() returns.  The device sampler draws the
 * minibatch; these tell the host how far that draw moves the stream, so the Agent advances its global
 * generator at learn() time without waiting for the GPU (R:dqn/agent.py:204-226 stays synchronous
 * from the caller's view) and checks the device's returned state against `out625` later.
 * dqnx_rng_sample_words: the 32-bit words CPython's random.sample(population of n, k) consumes from
 *   `state625` (its _randbelow rejections and the set branch's duplicate redraws depend on the values,
 *   so the stream is walked); `out625` (may be NULL) receives the state after the draw.  k > n returns
 *   DQNX_EINVAL with random.sample's ValueError message.
 * dqnx_rng_advance: `out625` = `state625` advanced by `words` MT19937 outputs (numpy's legacy uniform
 *   takes two per draw). */
int dqnx_rng_sample_words(const uint32_t* state625, int64_t n, int32_t k, uint32_t* out625, int64_t* words);
int dqnx_rng_advance(const uint32_t* state625, int64_t words, uint32_t* out625);

/* ---- the learn step: replaces Agent.learn() (R:dqn/agent.py:166-185 / 204-226 /
 *      245-272) and, with DQNX_STEP_SOFT_UPDATE, the following
 *      Agent.update_target_network() soft update (R:dqn/agent.py:105-110; caller
 *      R:train.py:99-101).
 * Stream-ordered; returns without synchronising.  Reads ring size/RNG/step from the
 * control block, so consecutive calls need no host round trip. */
#define DQNX_STEP_SOFT_UPDATE 0x1   /* fuse the tau soft update into the Adam pass */
#define DQNX_STEP_GIVEN_INDICES 0x2 /* skip sampling: use DQNX_BUF_BATCH_IDX as written by caller */
#define DQNX_STEP_GRADS_ONLY 0x4    /* stop after writing DQNX_BUF_GRADS (DP: all-reduce, then apply) */
#define DQNX_STEP_PREFETCH 0x8      /* pure learning loops: also draw the NEXT step's minibatch,
                                       overlapped with this step's compute (fused MLP plan: by one
                                       more workgroup of the last launch; per-layer plan: on a
                                       side stream).
                                       Results are bit-identical to sequential steps; while a
                                       prefetched minibatch is pending, dqnx_replay_push and
                                       dqnx_rng_set return DQNX_ESTATE and dqnx_rng_get already
                                       reflects the prefetched draw.  A step without the flag
                                       consumes the pending minibatch. */
#define DQNX_STEP_STATS 0x10        /* (ABI 5) accumulate this step's training statistics into
                                       DQNX_BUF_LEARN_STATS: one more launch, "learn_stats", the step's
                                       last; it only reads the step's buffers, so every other result of
                                       the step is bitwise what it is without the flag.  See "training
                                       statistics" below for the fields and where the flag is refused. */
int dqnx_learn_step(dqnx_engine* e, int32_t flags, void* stream);
/* Same-stream rule for DQNX_STEP_PREFETCH: the engine remembers the stream of the step that
 * left a draw pending; dqnx_rng_get synchronises THAT stream, and a later step on another
 * stream synchronises it first.  A caller that captures prefetching steps into its own graph
 * (dqn.data_parallel.GraphedDPStep) must replay the graph on the capture's stream or call
 * dqnx_prefetch_stream() with the replay stream before dqnx_rng_get. */
int dqnx_prefetch_stream(dqnx_engine* e, void* stream);
/* Draw the first minibatch of a prefetching loop now (no-op when a draw is pending or the
 * configuration does not draw ahead), so that the next DQNX_STEP_PREFETCH step can be captured
 * into a caller's graph without its prologue (dqn.data_parallel.GraphedDPStep). */
int dqnx_prefetch_begin(dqnx_engine* e, int32_t flags, void* stream);
/* `count` (1..256) consecutive learn steps, bitwise equal to `count` dqnx_learn_step(flags) calls
 * (flags: 0 or DQNX_STEP_SOFT_UPDATE).  Replaces a loop of Agent.learn() +
 * update_target_network() with no host work in between (R:train.py:99-101 repeated, e.g. several
 * gradient steps per environment step).  Uniform replay on the fused MLP plan runs them as ONE
 * graph in which step i's last launch also draws step i+1's minibatch; other configurations
 * run the steps one by one.  Nothing is pending afterwards. */
int dqnx_learn_steps(dqnx_engine* e, int32_t flags, int32_t count, void* stream);
/* Adam (+ optional soft update) from DQNX_BUF_GRADS: second half of a GRADS_ONLY step. */
int dqnx_apply_grads(dqnx_engine* e, int32_t flags, void* stream);
/* ---- bucketed data-parallel step (conv nets) -----------------------
 * The DQNX_STEP_GRADS_ONLY step cut where a layer's weight gradient is complete, so the caller
 * can all-reduce a finished bucket (on a side stream) while the engine runs the rest of the
 * backward, and apply Adam to it before the last bucket arrives.  Bucket 0 = dense layers +
 * Q head + the loss slot (done after the dense backward), then one bucket per conv, last conv
 * first.  The fused MLP plan (up to 2048 rows per GPU): bucket 0 = every layer but layer 1 + the
 * head + the loss slot, bucket 1 = layer 1 (its weight-gradient tiles as a launch of their own); the
 * slab plan's MLP has one bucket.  Each bucket is a contiguous range of DQNX_BUF_GRADS /
 * DQNX_BUF_PARAMS.  Enqueue dqnx_learn_step_bucket for b = 0, 1, ... in order on one stream;
 * dqnx_apply_grads_bucket(b) after bucket b's all-reduce (bucket 0's also applies the PER tree
 * update).  Together they equal dqnx_learn_step(GRADS_ONLY) + dqnx_apply_grads, bit for bit.
 * Replaces the single all-reduce of dqn/data_parallel.py's unbucketed step (no reference call
 * site: the reference trains on one device). */
int dqnx_dp_bucket_count(dqnx_engine* e, int32_t* n);
int dqnx_dp_bucket_info(dqnx_engine* e, int32_t bucket, int64_t* first, int64_t* count);
int dqnx_learn_step_bucket(dqnx_engine* e, int32_t flags, int32_t bucket, void* stream);
int dqnx_apply_grads_bucket(dqnx_engine* e, int32_t flags, int32_t bucket, void* stream);
/* Agent.update_target_network (R:dqn/agent.py:101-110): soft (tau*n_env) or hard copy. */
int dqnx_soft_update(dqnx_engine* e, void* stream);
int dqnx_hard_update(dqnx_engine* e, void* stream);

/* ---- acting path: replaces Network.actions (DeepQNetwork R:dqn/network.py:67-74: argmax of Q;
 *      DuelingDeepQNetwork R:dqn/network.py:110-117: argmax of the advantage stream only), as
 *      called by Agent.choose_actions (R:dqn/agent.py:92-99) before the epsilon-greedy override.
 * Stateless: `params` is a device fp32 vector in the layout of dqnx_net_param_info (the engine's
 * DQNX_BUF_PARAMS / DQNX_BUF_TARGET_PARAMS, or any flat copy).  obs: device [n][obs_dim];
 * actions: device int32[n] (first maximal index, like torch.argmax); values: device [n][n_actions]
 * or NULL (receives the argmaxed values: Q, or the advantages for a dueling head).  scratch:
 * 16-byte aligned device buffer of scratch_bytes >= dqnx_act_scratch_bytes(net, n) bytes (a
 * multiple of 4), zero-filled before its first use; every call leaves it ready for the next, so
 * calls with any n up to its size may share it on one stream.  MLP nets: one launch.  Two-stream
 * nets (TwoStreamHybridNetwork, R:env/dqn_config.py:66-143): one launch for the whole conv stack
 * where that is the faster call (two or more convs whose first layers fit a workgroup's LDS, and
 * n <= 2 by default: DQNX_ACT_TS=2 takes it up to n = 256, DQNX_ACT_TS=0 never), else one launch
 * per conv layer; then the dense stream + head as for an MLP on cat(flatten(conv), macro).
 * dqnx_act_kernel_count reports the launches.  Stream-ordered, no sync.
 *
 * Nets that do not fit a workgroup's LDS -- a conv input image over 64 KB (the (4,84,84) variant), or
 * a first dense layer of more than 8192 inputs -- are refused (DQNX_EUNSUPPORTED) unless the
 * environment holds DQNX_ACT_LARGE, read whenever a net is planned (every entry point below, so set it
 * before the first acting call of an object that decides its path once):
 *   unset / 0  refused, as above;
 *   1          such a net takes the LARGE route; nets that fit keep their kernels and launch counts;
 *   2          every MLP and two-stream net takes the large route (for testing it at small shapes).
 * The large route works through the n rows in chunks of at most 8, each chunk one banded launch per
 * conv layer, dense 1 as a split-K weight stream, its reduce, and one launch for the rest of the net
 * (layers 2..L + head as for an MLP on dense 1's output; the head alone for a one-layer body):
 * dqnx_act_kernel_count = ceil(n / 8) * (convs + 3).  The chunks reuse the scratch in stream order, so
 * dqnx_act_scratch_bytes(net, n) is one chunk's intermediates (min(n, 8) rows) plus the MLP kernels'
 * part, and does not grow past n = 8; the scratch contract above holds unchanged.  dqnx_act_host and
 * dqnx_agent_choose on this route always stage the obs, copy the actions back and synchronise the
 * stream (no in-place pinned path, no completion word). */
uint64_t dqnx_act_scratch_bytes(const dqnx_net_desc* net, int32_t n);
int dqnx_act(const dqnx_net_desc* net, const float* params, const float* obs, int32_t n, int32_t* actions,
             float* values, void* scratch, uint64_t scratch_bytes, void* stream);
/* launches dqnx_act makes for n rows of this net (host only, no GPU);
 * DQNX_EUNSUPPORTED where dqnx_act refuses the net */
int dqnx_act_kernel_count(const dqnx_net_desc* net, int32_t n, int32_t* count);

/* ---- drop-in Agent fast path: one host call per agent method (R:train.py:88-108) ---------------
 * dqnx_agent_stage_rng: Agent.learn()'s draw source -- snapshot `state625` (the caller's
 *   random.getstate()[1], or numpy's legacy keys + pos under PER) into the engine's pinned staging
 *   block for the next dqnx_agent_launch, and return in *words the MT19937 outputs the device draw will
 *   consume (the host advances its generator by them, dqnx_rng_sample_words / dqnx_rng_advance).  The
 *   post-draw state is remembered and checked against the device's at dqnx_agent_readback.  Uniform
 *   replay with fewer stored transitions than the batch: DQNX_EINVAL with random.sample's ValueError
 *   text (R:dqn/replay_memory.py:39).  Host only.
 * dqnx_agent_launch: the staged state's upload, dqnx_learn_step(flags) (DQNX_STEP_SOFT_UPDATE allowed),
 *   then the control block into an engine-owned pinned copy with an event; stream-ordered, no wait.
 * dqnx_agent_readback: 1 when the last launch's control block has arrived (wait = 1 blocks until it
 *   has), copied to `out` (may be NULL); 0 when none is pending or (wait = 0) it has not arrived yet;
 *   DQNX_EDEVICE when it carries a sticky device error (dqnx_ctrl.error) or its RNG state differs from
 *   the host mirror (dqnx_last_error() says which).
 * dqnx_act_host: dqnx_act with HOST obs [n][obs_dim] and HOST actions [n]: the obs through pinned
 *   memory into the END of `scratch` (dqnx_act_host_scratch_bytes(net, n) bytes, zero-filled before
 *   its first use), one launch sequence, the actions back; synchronises `stream` (Network.actions,
 *   R:dqn/network.py:67-74, 110-117).  MLP nets, and two-stream nets on the one-launch conv stack
 *   with n rows in one row group (n <= 4, and where dqnx_act takes that stack): the kernels read the pinned obs and write the pinned
 *   actions in place, with no copy calls, and the call waits on a completion word instead. */
int dqnx_agent_stage_rng(dqnx_engine* e, int32_t which, const uint32_t* state625, int64_t* words);
int dqnx_agent_launch(dqnx_engine* e, int32_t flags, void* stream);
/* dqnx_agent_learn_mt: Agent.learn() on the caller's LIVE generator, uniform replay: `mt` = its 624
 *   MT19937 state words and `*pos` its output position (CPython's RandomObject holds them as
 *   `int index; uint32_t state[624]`: the drop-in passes the addresses inside random._inst after
 *   checking the layout against random.getstate()).  Staged as dqnx_agent_stage_rng(DQNX_RNG_PY)
 *   stages mt + pos, then advanced IN PLACE past the words the draw consumes (*words), i.e. the
 *   generator is left where random.sample(deque, batch_size) leaves it (R:dqn/replay_memory.py:39);
 *   with DQNX_AGENT_LAUNCH in flags, dqnx_agent_launch(flags without it) follows in the same call.
 *   One library call per learn() instead of getstate + stage + getrandbits + launch. */
#define DQNX_AGENT_LAUNCH 0x100
int dqnx_agent_learn_mt(dqnx_engine* e, uint32_t* mt, int32_t* pos, int32_t flags, void* stream, int64_t* words);
int dqnx_agent_readback(dqnx_engine* e, int32_t wait, dqnx_ctrl* out);
/* dqnx_agent_quiesce: waits for what dqnx_agent_launch / dqnx_agent_learn_mt would wait on before
 *   launching (the previous step's unread control-block readback); no state changes.  The drop-in
 *   calls it, with the GIL released, before a dqnx_agent_learn_mt (GIL held) whose previous readback
 *   is still unread, so no other Python thread is blocked for the length of a GPU wait. */
int dqnx_agent_quiesce(dqnx_engine* e);
/* dqnx_agent_choose: Agent.choose_actions(obses) (R:dqn/agent.py:92-99) in ONE call, for every net
 *   dqnx_act supports (MLP and two-stream), on the
 *   engine's online parameters: the greedy actions of the n HOST rows at obs_host (dqnx_act_host's
 *   launch: the advantage stream for dueling nets, R:dqn/network.py:110-117), and -- while the acting
 *   kernel runs -- for every env i in order: u = random.random() from the caller's LIVE MT19937 (mt =
 *   its 624 words, *pos its index, advanced in place as dqnx_agent_learn_mt does: CPython's
 *   genrand_res53, 2 words); if u <= epsilon, actions[i] = random.randint(0, n_actions - 1)
 *   (_randbelow: getrandbits(n_actions.bit_length()) redrawn while >= n_actions).  Then the wait for
 *   the kernel and the last agent step's control-block checks (as dqnx_agent_readback(wait = 1)).
 *   `scratch` as dqnx_act_host's (dqnx_act_host_scratch_bytes(&cfg.net, n)); n <= DQNX_CHOOSE_MAX_ENVS.
 *   flags & DQNX_CHOOSE_GIL_HELD: the caller holds the Python GIL (it must, for the in-place generator
 *   update); the GIL is released around the GPU wait (PyEval_SaveThread / PyEval_RestoreThread of the
 *   running interpreter). */
#define DQNX_CHOOSE_MAX_ENVS 256
#define DQNX_CHOOSE_GIL_HELD 0x1
int dqnx_agent_choose(dqnx_engine* e, const float* obs_host, int32_t n, double epsilon, uint32_t* mt, int32_t* pos,
                      int32_t* actions_out, void* scratch, uint64_t scratch_bytes, int32_t flags, void* stream);
uint64_t dqnx_act_host_scratch_bytes(const dqnx_net_desc* net, int32_t n);
int dqnx_act_host(const dqnx_net_desc* net, const float* params, const float* obs_host, int32_t n,
                  int32_t* actions_host, void* scratch, uint64_t scratch_bytes, void* stream);

/* ---- training-state snapshot (ABI 4): stop a run and continue it bit for bit -----------------
 * Everything a learn step, a push or a sample reads that an earlier one wrote, as ONE
 * self-describing little-endian blob in host memory (the reference keeps only the online weights,
 * R:dqn/agent.py:112-128; its replay deque, Adam state and target net do not survive a restart).
 *
 * Blob layout:
 *   [0, sizeof(dqnx_state_info))  the header below, as it lies in memory: magic, format version,
 *                                 the fingerprint and the section table
 *   then the sections, each at its table entry's `offset` (from the start of the blob, a multiple of
 *   DQNX_STATE_ALIGN, at or past header_bytes, in table order without overlap) with exactly `bytes`
 *   bytes.  dqnx_state_save writes them back to back in the order listed below (every size is a
 *   multiple of 4, and the fp64 SumTree, written right after the control block, lands on a multiple
 *   of 8), so total_bytes = sizeof(dqnx_state_info) + the sum of the section sizes.
 *
 * Sections (P = n_params, n = ring_size, D = net.obs_dim, C = capacity), each present exactly once:
 *   DQNX_SEC_PARAMS / TARGET_PARAMS / ADAM_M / ADAM_V   P fp32 each (dqnx_net_param_info order)
 *   DQNX_SEC_CTRL            the whole dqnx_ctrl (both MT19937 streams, ring size / write slot, Adam
 *                            step, agent_step, SumTree max / min indices, loss, PER beta)
 *   DQNX_SEC_SUMTREE         [2C-1] fp64, DQNX_ALGO_PER_DOUBLE only (absent otherwise)
 *   DQNX_SEC_RING_OBS / RING_NEXT_OBS   [n][D] fp32: ring slots 0 .. n-1 in PHYSICAL order (a ring that
 *                            has not wrapped fills slots 0 .. n-1; a full one holds all C), rows of D
 *                            floats whatever the engine's row stride
 *   DQNX_SEC_RING_ACT [n] int32, DQNX_SEC_RING_REW [n] fp32, DQNX_SEC_RING_DONE [n] fp32 (0 / 1)
 * Not state, never stored: the gradient, the minibatch indices, Q / TD buffers, IS weights and the
 * workspace (derived weight layouts, RNG block caches, bf16 ring copies, the Adam bias table: the
 * loading engine rebuilds or invalidates them).  The blob grows with the fill, not the capacity.
 *
 * A valid blob has: the magic and version below; header_bytes = sizeof(dqnx_state_info); total_bytes
 * <= the bytes given; a network dqnx_net_param_count accepts, with n_params parameters; algo,
 * compute_dtype in their enums; capacity >= 1; 0 <= ring_size <= capacity; 0 <= ring_wptr <
 * capacity, and ring_wptr = ring_size while ring_size < capacity; the sections above with the sizes
 * the fingerprint gives (computed without 64-bit overflow), inside total_bytes; and a control block
 * whose ring_size / ring_wptr equal the fingerprint's, whose MT positions are <= 624, whose SumTree
 * indices lie in [0, 2C-1), whose adam_step is >= 0 and whose sticky error is 0. */
#define DQNX_STATE_MAGIC 0x54415453584e5144ull   /* "DQNXSTAT" read as a little-endian uint64 */
#define DQNX_STATE_VERSION 1
#define DQNX_STATE_ALIGN 4
#define DQNX_STATE_MAX_SECTIONS 16
enum dqnx_state_section_id {
    DQNX_SEC_PARAMS = 1, DQNX_SEC_TARGET_PARAMS = 2, DQNX_SEC_ADAM_M = 3, DQNX_SEC_ADAM_V = 4, DQNX_SEC_CTRL = 5,
    DQNX_SEC_RING_OBS = 6, DQNX_SEC_RING_NEXT_OBS = 7, DQNX_SEC_RING_ACT = 8, DQNX_SEC_RING_REW = 9,
    DQNX_SEC_RING_DONE = 10, DQNX_SEC_SUMTREE = 11
};
typedef struct dqnx_state_section {
    uint32_t id;               /* dqnx_state_section_id */
    uint32_t reserved;         /* 0 */
    uint64_t offset;           /* from the start of the blob */
    uint64_t bytes;
} dqnx_state_section;
typedef struct dqnx_state_info {
    uint64_t magic;            /* DQNX_STATE_MAGIC */
    uint32_t version;          /* DQNX_STATE_VERSION */
    uint32_t header_bytes;     /* sizeof(dqnx_state_info) */
    uint64_t total_bytes;      /* of the whole blob */
    /* fingerprint */
    dqnx_net_desc net;
    int32_t algo;              /* dqnx_algo */
    int32_t compute_dtype;     /* dqnx_compute_dtype of the saving engine (informative: may differ at load) */
    int32_t per_numpy121;      /* of the saving engine (informative) */
    int32_t n_sections;
    int32_t reserved0;         /* 0 */
    int64_t capacity;
    int64_t n_params;
    int64_t ring_size;
    int64_t ring_wptr;
    dqnx_state_section sections[DQNX_STATE_MAX_SECTIONS];   /* [n_sections] used, the rest zero */
} dqnx_state_info;

/* Bytes dqnx_state_save would write now (host only: from the engine's mirror of the ring size). */
int dqnx_state_bytes(dqnx_engine* e, uint64_t* bytes);
/* Write the blob into dst_host (`bytes` >= dqnx_state_bytes; *written = its size).  Synchronises
 * `stream`.  DQNX_ESTATE while a prefetched minibatch is pending (as dqnx_replay_push), while an agent
 * launch's control-block readback is unread or a staged RNG state awaits its launch, or between the
 * buckets of a bucketed step; DQNX_EDEVICE when dqnx_ctrl.error is set (a faulted run is not a
 * checkpoint). */
int dqnx_state_save(dqnx_engine* e, void* dst_host, uint64_t bytes, uint64_t* written, void* stream);
/* Restore a blob.  The whole blob is validated (as dqnx_state_inspect does) and matched against the
 * engine before the first device write: the network description, the capacity and prioritised-or-not
 * must equal the engine's (uniform algorithms DQN / DOUBLE may load each other's blobs); batch, lr,
 * gamma, tau, world / rank, compute_dtype and per_numpy121 may differ.  Any mismatch: DQNX_EINVAL with
 * a message naming the field, the engine untouched.  DQNX_ESTATE under dqnx_state_save's pending
 * conditions.  Afterwards the engine behaves as if it had reached that state by itself: its ring
 * mirrors are set, the derived weight layouts are marked stale (as dqnx_params_modified), the RNG block
 * caches are invalidated, a bf16 engine's bf16 ring rows are regenerated from the restored fp32 rows,
 * the agent fast path's expectations are cleared; the Adam bias table stays the engine's own (it
 * follows ITS lr).  Cached graphs stay valid (they read the state through the arena).  Synchronises
 * `stream`; src_host is free on return. */
int dqnx_state_load(dqnx_engine* e, const void* src_host, uint64_t bytes, void* stream);
/* Validate a blob (all of the rules above) and copy its header out (host only: no engine, no GPU).
 * DQNX_EINVAL with a message naming what is wrong. */
int dqnx_state_inspect(const void* blob, uint64_t bytes, dqnx_state_info* out);

/* ---- training statistics (ABI 5): what a learn step computed, accumulated on the device ------
 * A step with DQNX_STEP_STATS ends with one more launch ("learn_stats" in dqnx_learn_kernel_info) that
 * reduces the step's own buffers -- DQNX_BUF_Q, DQNX_BUF_TD, DQNX_BUF_GRADS, DQNX_BUF_IS_WEIGHTS, the
 * online parameters after the step's Adam, dqnx_ctrl.loss, and the replay action / reward / done of the
 * rows the step sampled -- into the one dqnx_learn_stats of DQNX_BUF_LEARN_STATS.  The block accumulates
 * over steps; the host reads it once per log window (dqnx_learn_stats_get), not once per step.
 * Accepted by dqnx_learn_step, dqnx_learn_steps, dqnx_agent_launch, dqnx_agent_learn_mt,
 * dqnx_learn_step_timed, dqnx_learn_step_omit, dqnx_learn_kernel_count and dqnx_learn_kernel_info.
 * DQNX_EUNSUPPORTED (the block untouched): together with DQNX_STEP_GRADS_ONLY, in
 * dqnx_learn_step_bucket / dqnx_apply_grads / dqnx_apply_grads_bucket, on an engine with world_size > 1
 * (the batch part would need a cross-rank reduction), and for a net of more than
 * DQNX_STATS_MAX_ACTIONS actions or DQNX_STATS_MAX_TENSORS parameter tensors.
 * The micro-CNN plan does not draw a minibatch ahead in a DQNX_STEP_STATS step (DQNX_STEP_PREFETCH is
 * ignored there and dqnx_learn_steps runs the steps one by one): its in-launch draw overwrites the
 * step's indices before the statistics launch could read them.  Results are the same either way.
 *
 * Every sum is carried in fp64 from the first add (an fp32 x fp32 product is exact in fp64) and summed
 * in an order fixed by the launch geometry, never by scheduling: two runs of the same steps leave the
 * same bytes.  All fields are over the B rows of a step's minibatch and accumulate over steps, except
 * the *_last arrays (the last step only).  The first step accumulated into a zeroed block (steps == 0)
 * SETS the min / max fields, so an all-zero block is the valid empty state.
 * Not training state: zeroed by dqnx_engine_reset, dqnx_state_load and dqnx_learn_stats_reset, never
 * written to the state blob. */
#define DQNX_STATS_MAX_ACTIONS 16
#define DQNX_STATS_TD_BINS 16
#define DQNX_STATS_MAX_TENSORS 32
typedef struct dqnx_learn_stats {
    int64_t steps;             /* steps accumulated */
    int64_t rows;              /* sum of B */
    double q_sa_sum, q_sa_sq_sum;   /* Q(s,a) of the taken action (DQNX_BUF_TD[1]) */
    double q_max_sum;          /* max_a Q_online(s) (rows of DQNX_BUF_Q[0]) */
    double target_sum;         /* TD target y (DQNX_BUF_TD[0]) */
    double abs_td_sum;         /* |delta| (DQNX_BUF_TD[2]) */
    double gap_sum;            /* top-1 minus top-2 of the DQNX_BUF_Q[0] row, subtracted in fp32 (0 when A = 1) */
    double reward_sum;         /* replay reward of the sampled rows */
    double isw_sum;            /* PER importance weights (0 for uniform replay) */
    double loss_sum;           /* sum of dqnx_ctrl.loss (with dqnx_set_cql on: the total, TD + regulariser) */
    double grad_norm_sum;      /* sum over steps of sqrt(sum_t grad_sq of the step) */
    double grad_norm_max;      /* its maximum (a derived fp64 value, so kept in fp64) */
    int64_t huber_linear_rows; /* rows with |delta| >= 1 (SmoothL1's linear regime, beta = 1) */
    int64_t agree_rows;        /* rows whose greedy action is the replay action */
    int64_t done_rows;         /* sampled rows with done != 0 */
    /* |delta| by fp32 exponent: bin = clamp(e + 12, 0, 15), e the unbiased exponent; 0 and denormals in bin 0 */
    int64_t td_hist[DQNX_STATS_TD_BINS];
    int64_t greedy_hist[DQNX_STATS_MAX_ACTIONS];   /* argmax of the DQNX_BUF_Q[0] row, first maximal index */
    int64_t taken_hist[DQNX_STATS_MAX_ACTIONS];    /* replay action of each sampled row */
    /* per parameter tensor, dqnx_net_param_info order */
    double grad_sq_last[DQNX_STATS_MAX_TENSORS];   /* sum g^2 over the tensor, last step */
    double param_sq_last[DQNX_STATS_MAX_TENSORS];  /* sum theta^2 of the online params after the last step's Adam */
    double grad_sq_sum[DQNX_STATS_MAX_TENSORS];    /* grad_sq_last accumulated over steps */
    /* extrema of fp32 buffer values */
    float q_sa_min, q_sa_max, q_max_max, target_min, target_max, abs_td_max;
    float isw_min;             /* PER only (0 for uniform replay) */
    float reserved0;           /* 0 */
} dqnx_learn_stats;
/* Copy the block to host memory: synchronises `stream`, and with reset != 0 zeroes the block afterwards
 * (stream-ordered).  DQNX_ESTATE under dqnx_state_save's pending conditions (a prefetched minibatch, an
 * unread agent readback, a staged RNG state, between buckets). */
int dqnx_learn_stats_get(dqnx_engine* e, dqnx_learn_stats* out_host, int32_t reset, void* stream);
/* Zero the block; stream-ordered, no synchronisation. */
int dqnx_learn_stats_reset(dqnx_engine* e, void* stream);

/* ---- gradient clipping: the global norm of the gradient, clipped on the device before Adam ------
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) between loss.backward() and
 * optimizer.step(), where the reference's learn() leaves room for it (R:dqn/agent.py:224-226):
 *   total_norm = sqrt(sum over every parameter element of g^2)   (the loss slot grads[n_params] is not part)
 *   coef       = min(max_norm / (total_norm + 1e-6), 1.0)        (fp32: one correctly rounded division;
 *                torch evaluates float / tensor as tensor.reciprocal() * float, two roundings, so its
 *                coefficient may differ from this one by 1 ulp)
 *   g'         = g * coef        one fp32 multiply per element, also when coef == 1
 * Adam and the fused soft update consume g'.  A non-finite norm is not special-cased (torch's
 * error_if_nonfinite=False).  max_norm <= 0 means off, the default: a step then launches exactly what it
 * launches without this section.  DQNX_BUF_GRADS keeps the UNSCALED gradient, and the statistics launch
 * (grad_norm_*, grad_sq_*) and last_norm report the pre-clip norm: the number max_norm is chosen from.
 *
 * While clipping is on, a learn step is the DQNX_STEP_GRADS_ONLY step's launches, then "grad_sumsq" (one
 * fp64 partial of sum g^2 per workgroup of DQNX_BUF_GRADS[0, n_params), in an order fixed by the launch
 * geometry, no atomics), "clip_coef" (one workgroup: the partials in index order, the coefficient, the
 * info block) and dqnx_apply_grads' launch with every gradient element multiplied by the coefficient
 * (under PER the tree update dqnx_apply_grads makes); then the statistics launch, if asked for.  So a
 * clipped dqnx_learn_step equals dqnx_learn_step(DQNX_STEP_GRADS_ONLY) + dqnx_apply_grads bit for bit, and
 * with coef == 1 the unclipped step.  It applies to dqnx_learn_step, dqnx_learn_steps (the steps one by
 * one), dqnx_agent_launch / dqnx_agent_learn_mt, dqnx_apply_grads (under data parallelism the norm of the
 * all-reduced gradient: every rank computes the same coefficient from the same bytes) and to what
 * dqnx_learn_kernel_count / _info / dqnx_learn_step_timed / _omit describe (a dqnx_learn_step_omit step,
 * as without clipping, leaves the engine fit for timing only).  DQNX_EUNSUPPORTED while
 * clipping is on: dqnx_learn_step_bucket / dqnx_apply_grads_bucket (a bucket's Adam runs before the last
 * bucket's gradient exists).
 *
 * dqnx_set_grad_clip: host only; max_norm is configuration like lr (not in the state blob).  It drops the
 *   engine's cached plans and graphs (the value is a launch argument), so a caller's own captured graph of
 *   engine calls keeps the value it was captured with.  DQNX_ESTATE under dqnx_state_save's pending
 *   conditions (a prefetched minibatch, an unread agent readback, a staged RNG state, between buckets).
 * dqnx_grad_clip_info: accumulated on the device by "clip_coef", one plain read-modify-write per clipped
 *   step; read at log cadence.  Not training state: zeroed by dqnx_engine_reset and dqnx_state_load,
 *   never written to the state blob.
 * dqnx_grad_clip_info_get: copies the block to host memory, synchronises `stream`, and with reset != 0
 *   zeroes it afterwards (stream-ordered).  DQNX_ESTATE as dqnx_learn_stats_get. */
int dqnx_set_grad_clip(dqnx_engine* e, double max_norm);      /* host only; <= 0 turns it off */
int dqnx_get_grad_clip(const dqnx_engine* e, double* max_norm);
typedef struct dqnx_grad_clip_info {
    int64_t steps, clipped_steps;        /* clipped: coef < 1 */
    double norm_sum, norm_max;           /* pre-clip total_norm over steps */
    float last_norm, last_coef;
} dqnx_grad_clip_info;
int dqnx_grad_clip_info_get(dqnx_engine* e, dqnx_grad_clip_info* out_host, int32_t reset, void* stream);

/* ---- n-step returns: multi-step TD targets for every learn route, gathered on the device ----
 * dqnx_config.n_step = n in 1 .. DQNX_NSTEP_MAX (anything else: DQNX_EINVAL at create).  The replay ring
 * stays the 1-step ring the reference fills (R:dqn/replay_memory.py:30-36): a push of n_env rows is one
 * time step, so the successor of logical position p (0 = oldest) in the same environment is p + n_env, and
 * the n-step transition of a sampled start row p is assembled at sample time from the ring as it is.  With
 * size = dqnx_ctrl.ring_size, gamma = cfg.gamma (a double) and n_env = cfg.n_env:
 *
 *   g = 1.0; R = 0.0; m = 0; d = 0.0                  (fp64)
 *   for j in 0 .. n-1:
 *       q = p + j*n_env
 *       if q >= size: break                            the window reaches the newest end of the ring
 *       R += g * (double)rew[q]                        one fp64 multiply, one fp64 add, no contraction
 *       g *= gamma                                     repeated multiply, not pow
 *       m = j + 1
 *       if done[q] != 0: d = 1.0; break
 *   last = p + (m-1)*n_env
 *   row  = ( obs[p], act[p], (float)R, d, next_obs[last] ),  disc = (float)g = fp32(gamma^m)
 *   y    = R + ((1 - d) * disc) * q'                   the head's fp32 order, disc where (float)gamma stands
 *
 * m >= 1 always; n = 1 gives R = rew[p], d = done[p], last = p, disc = (float)gamma: the default step bit
 * for bit.  Sampling is unchanged (the draw and its RNG consumption stay bit-exact), a SumTree leaf still
 * means one ring slot, and PER priorities attach to the start row p (a sampled ring slot maps to its
 * logical position by (slot - (ring_wptr - ring_size)) mod capacity).  The state blob does not change: a
 * blob saved by an n-step engine loads into a 1-step engine and the other way round.
 *
 * Launches: an n-step engine's learn step gains ONE launch, "nstep_gather", its first compute launch: it
 * follows the launch that makes the step's slot table final (the sampler "sample_uniform" / "per_sample" /
 * "idx_to_phys"; in the steady state of a prefetching loop, where the previous step left the minibatch,
 * it is the step's first launch).  For each of the batch_local rows it walks the window and writes the
 * materialised minibatch: the last part of DQNX_BUF_WORKSPACE of an n-step engine (a default engine's
 * workspace has no such part: dqnx_nstep_buffer reports 0 bytes), rewritten by every learn step, never in
 * the state blob.  Its sub-arrays follow each other from the offset dqnx_nstep_buffer gives, in this order,
 * each at the next multiple of 256 bytes (Bl = batch / world_size, S = dqnx_engine_obs_stride):
 *   mb_obs [Bl][S] fp32, mb_next [Bl][S] fp32 (the row of slot `last`), mb_act [Bl] int32, mb_rew [Bl] fp32,
 *   mb_done [Bl] fp32, mb_disc [Bl] fp32, mb_phys [Bl] int32 (the identity: mb_phys[b] = b),
 *   mb_start [Bl] {int32 act, fp32 rew, fp32 done, 0} of the START rows, then (DQNX_COMPUTE_BF16 engines) the
 *   bf16 copies of mb_obs and mb_next, [Bl][S16] each, S16 = obs_dim rounded up to a multiple of 8.
 * Every other launch of the step reads these where a default engine reads the ring through its slot table;
 * no forward, backward or Adam kernel differs, and the two head kernels multiply by mb_disc[b] where they
 * multiply by (float)gamma.  dqnx_learn_kernel_count / _info / dqnx_learn_step_timed / _omit list the launch
 * (0 FLOPs; bytes = the rows and scalars moved).  An engine with n_step = 1 launches exactly what it launched
 * before this section and has the same arena size; DQNX_NSTEP_FORCE=1 in the environment at create sends it through the
 * gather too (for testing the route: bitwise the default).
 * Composition: every step flag and entry point works as before -- PER, bf16, gradient clipping,
 * DQNX_STEP_PREFETCH, dqnx_learn_steps, graphs, DQNX_STEP_GRADS_ONLY + dqnx_apply_grads (world_size > 1: each
 * rank gathers its own shard's rows), the bucketed step, the agent fast path.  The only new refusal is
 * dqnx_replay_push's row-count rule above.
 * DQNX_STEP_STATS: reward_sum, done_rows and taken_hist describe the sampled START rows (mb_start: the 1-step
 * reward and done of row p); target_*, abs_td_*, td_hist and huber_linear_rows describe the n-step target.
 *
 * dqnx_nstep_window (test hook, host only, no engine, no GPU): the window of start position p over rew /
 * done arrays indexed by logical position, by the same inline function the gather kernel calls.  DQNX_EINVAL
 * unless 0 <= p < size, 1 <= n_step <= DQNX_NSTEP_MAX and n_env >= 1.  Any output pointer may be NULL. */
/* Arena offset and size of the materialised minibatch (host only; *bytes = 0 for a default engine). */
int dqnx_nstep_buffer(const dqnx_engine* e, uint64_t* offset, uint64_t* bytes);
int dqnx_nstep_window(const float* rew, const float* done, int64_t size, int64_t p, int32_t n_step,
                      int32_t n_env, double gamma, float* R, float* d, float* disc,
                      int64_t* last, int32_t* m);

/* ---- conservative Q-learning: the CQL(H) regulariser for training from a fixed dataset ----
 * Plain (double) DQN on transitions that no longer grow over-estimates the actions the data never took.
 * CQL(H) for discrete actions adds one term to the loss,
 *
 *   L = L_TD + alpha * mean_b [ logsumexp_a Q_online(s_b, a) - Q_online(s_b, a_b) ]
 *
 * computed in the head kernels of every learn route, from the fp32 row Q_online(s_b, .) they already hold
 * (after the dueling aggregate).  Per sampled row, a = the clamped replay action, A = n_actions:
 *
 *   m    = max_j q_j
 *   e_j  = expf(q_j - m)            libm-grade expf / logf, no contraction
 *   s    = sum_j e_j                (the routes may sum in different orders)
 *   gap  = (m + logf(s)) - q_a
 *   p_j  = e_j / s
 *   dq_j = gq [j = a] + cb (p_j - [j = a]),   cb = fp32(alpha) * (1 / B_global)
 *
 * gq is the TD gradient as without this section (Huber, IS-weighted under PER).  Through the head:
 * linear d_j = dq_j; dueling d_V = sum_j dq_j, d_Aj = dq_j - (sum_j dq_j) / A.  The row's loss contribution
 * is lb + fp32(alpha) * gap, so dqnx_ctrl.loss -- and with it dqnx_learn_stats.loss_sum -- reports the TOTAL
 * loss.  Under PER the regulariser is NOT importance-weighted, and |delta|, the priorities and the SumTree
 * updates are exactly the TD error's.  The 1 / B_global factor makes data-parallel shards sum to the
 * global-batch mean like the TD term.  DQNX_BUF_TD, DQNX_BUF_Q and abs_td keep their meaning.
 *
 * It costs no launch, no device storage and no arena byte: with alpha > 0 a step launches exactly the
 * launches it launches with alpha = 0 (dqnx_learn_kernel_count / _info give the same names, FLOPs and
 * bytes); the head kernel of the step is another instantiation of the same template.  With alpha = 0 (the
 * default) the head kernels are the code of an engine that never heard of this section, bit for bit.  It
 * applies to every learn entry point and flag combination: dqnx_learn_step, dqnx_learn_steps,
 * dqnx_agent_launch / dqnx_agent_learn_mt, dqnx_learn_step_bucket, dqnx_learn_step_timed / _omit; graphs,
 * prefetch, n-step returns, gradient clipping, bf16.
 *
 * dqnx_set_cql: host only; alpha <= 0 means off.  NaN or an infinity: DQNX_EINVAL, the value kept.
 *   Configuration like lr: never in the state blob, accepted by an unbound engine.  It drops the engine's
 *   cached plans and graphs (alpha is a launch argument and picks the instantiation).  DQNX_ESTATE under
 *   dqnx_state_save's pending conditions.
 * dqnx_cql_row (test hook, host only, no engine, no GPU): gap and p_j - [j = a] of one row q[0 .. n_actions)
 *   by the inline function the head kernel calls.  1 <= n_actions <= 16 (else DQNX_EINVAL); an action outside
 *   [0, n_actions) is taken as 0, as the kernels clamp it.  q and p_minus_onehot must not overlap. */
int dqnx_set_cql(dqnx_engine* e, double alpha);
int dqnx_get_cql(const dqnx_engine* e, double* alpha);
int dqnx_cql_row(const float* q, int32_t n_actions, int32_t action, float* gap, float* p_minus_onehot);

/* ---- offline evaluation: sweep a range of the replay ring on the device, no update ----
 * What a set of weights does on a fixed set of transitions: for the logical range [lo, hi) of the engine's own
 * replay ring (0 = the oldest row, deque order) the route's forward runs over the rows IN ORDER, in chunks of
 * batch rows, and per-row quantities are reduced to dataset totals on the device.  Nothing of the engine's
 * training state changes: parameters, target parameters, Adam moments and step, RNG states, the ring, the
 * SumTree and priorities, dqnx_ctrl (loss included), the learn statistics, the (idx, phys) slots and a
 * minibatch drawn ahead (DQNX_STEP_PREFETCH: the staged minibatch and the compute slot it was copied to) are
 * all left as they were; a dqnx_state_save blob is byte-equal before and after, and learn steps interleaved
 * with evaluations are bitwise the uninterrupted steps.  Only scratch is written: the caller's scratch buffer,
 * the activations / raw head outputs of DQNX_BUF_WORKSPACE that every step's forward rewrites, on an n-step
 * engine the materialised minibatch (rewritten by every step's gather), and derived weight copies (the fused
 * plan's blocked copies, the conv plans' permuted copies) which are REBUILT from the weights when stale,
 * exactly as the next step would.  DQNX_BUF_Q and DQNX_BUF_TD are not written: they keep describing the last
 * learn step (LearnEngine.cql_gap() too).
 *
 * Row inputs: per position p in [lo, hi) the transition the engine's learn step would train on had it sampled
 * p -- the n-step window of "n-step returns" when n_step > 1 -- and the target rule of the engine's
 * algorithm (DQN: the max; Double / PER-Double: the online argmax into the target net).
 *   q_j   = Q_online(s, j) after the head's aggregate;  a = the clamped replay action
 *   y     = R + ((1 - d) * disc) * q'          the head kernels' fp32 order
 * Per-row quantities (fp32, csrc/eval.hpp):
 *   delta = y - q_a
 *   lb    = |delta| < 1 ? (0.5 |delta|) |delta| : |delta| - 0.5    Huber, beta = 1, UNWEIGHTED (no IS weights:
 *           evaluation is not sampling), no regulariser
 *   v     = max_j q_j;   g = the first j with q_j = v (torch's and the head kernels' tie rule)
 *   gap   = (v + logf(sum_j expf(q_j - v))) - q_a                  logsumexp_j q_j - q_a, csrc/cql.hpp's forms
 *   agap  = v - max_{j != g} q_j                                   the action gap; 0 when A = 1
 * Totals: dqnx_eval_result below.  Every sum is carried in fp64 from the first add (delta^2: the exact fp64
 * product) in a fixed order -- the 16 rows of a workgroup in row order, the workgroup records in workgroup
 * order, the chunks in chunk order -- with no atomics on floating-point values, so two calls on the same
 * state return the same bytes, whenever they are made.  n_actions <= DQNX_STATS_MAX_ACTIONS.
 * Optional per-row output: rows_out = a device buffer [hi - lo][4] fp32 (16-byte aligned), row p - lo =
 * (g, q_a, v, delta); NULL to skip.
 *
 * Launches per chunk c (rows lo + c*B .. , B = batch): "eval_idx" (positions and their ring slots
 * (ring_wptr - ring_size + p) mod capacity into the scratch table; positions past hi are clamped to hi - 1,
 * so the forward always runs a full batch of valid rows), on an n-step engine "nstep_gather" reading that
 * table, the route's own forward launches (fused MLP plan fp32 / bf16, per-layer plan, micro-CNN, im2col and
 * implicit-GEMM conv plans) with the table as their row source and without sampler workgroup, staged-minibatch
 * copy, Adam scalars or MT-cache work, on the per-layer routes "eval_head" (the raw head outputs in the fused
 * plan's [3][B][16] layout; the fused forward already leaves them), "eval_rows" (rows past the range's end
 * contribute nothing) and "eval_fold" (a launch of its own: one workgroup sums the workgroup records and adds
 * the chunk to the accumulator in the scratch).  Chunks accumulate on the device; the call copies the result
 * to result_out (host memory) once and synchronises `stream` once, after the last chunk.  Plans are cached per
 * engine and scratch pointer and dropped with the step plans.
 *
 * dqnx_eval_scratch_bytes: the scratch the caller allocates (device memory, 256-byte aligned): the chunk's
 *   index / slot table, one fp64 record per 16-row workgroup, the accumulator.  The arena does not change.
 * dqnx_eval_range refuses: DQNX_EINVAL for lo < 0, hi > ring size or lo >= hi (an n-step engine refuses no
 *   further row: a window is cut by the ring's newest end, m >= 1, so every position is a valid start row);
 *   DQNX_EUNSUPPORTED on a world_size > 1 engine; DQNX_ESTATE during a stream capture.
 * dqnx_eval_kernel_count / _name / dqnx_eval_chunk_timed: the launches of one chunk, and one chunk (the rows
 *   lo .. lo + B, totals discarded) run eagerly with the event pair bound to launch `kernel_index`.
 * dqnx_eval_row (test hook, host only, no engine, no GPU): one row from the raw head outputs of the three
 *   streams (n_actions entries for a linear head; V then n_actions advantages for a dueling head, n_actions
 *   <= 15 there), serially through the inline functions k_eval_rows calls.  raw_online_next may be NULL for
 *   DQNX_ALGO_DQN.  An action outside [0, n_actions) is taken as 0. */
typedef struct dqnx_eval_result {
    int64_t rows;                      /* hi - lo */
    double huber_sum;                  /* lb */
    double abs_td_sum, td_sq_sum;      /* |delta|, delta^2 */
    double q_sa_sum;                   /* q_a */
    double v_sum;                      /* max_j q_j */
    double cql_gap_sum;                /* logsumexp_j q_j - q_a */
    double action_gap_sum;             /* top-1 minus top-2 */
    double reward_sum;                 /* the (n-step) reward R */
    double target_sum;                 /* y */
    double abs_td_max, v_max, v_min;
    int64_t agree_rows;                /* g == a */
    int64_t done_rows;                 /* d != 0 */
    int64_t greedy_hist[DQNX_STATS_MAX_ACTIONS];
    int64_t taken_hist[DQNX_STATS_MAX_ACTIONS];
} dqnx_eval_result;
typedef struct dqnx_eval_row_result {
    int32_t greedy, action;            /* g; the clamped replay action */
    float q_a, v, delta, huber, gap, action_gap, y;
    float reserved0;                   /* 0 */
} dqnx_eval_row_result;
int dqnx_eval_scratch_bytes(const dqnx_engine* e, uint64_t* bytes);
int dqnx_eval_range(dqnx_engine* e, int64_t lo, int64_t hi, void* scratch, uint64_t scratch_bytes,
                    float* rows_out_or_null, dqnx_eval_result* result_out_host, void* stream);
int dqnx_eval_row(const float* raw_online, const float* raw_online_next, const float* raw_target_next,
                  int32_t head, int32_t n_actions, int32_t algo, int32_t action, float reward, float done,
                  float discount, dqnx_eval_row_result* out);
int dqnx_eval_kernel_count(dqnx_engine* e, int32_t* n);
int dqnx_eval_kernel_name(dqnx_engine* e, int32_t index, char* name, int32_t name_len);
int dqnx_eval_chunk_timed(dqnx_engine* e, int64_t lo, void* scratch, uint64_t scratch_bytes, int32_t kernel_index,
                          void* ev_start, void* ev_stop, void* stream);

/* ---- fitted Q evaluation: score a fixed policy on the logged transitions, on the device ----
 * dqnx_eval_range reports properties of a Q function; fitted Q evaluation (FQE) estimates the discounted return
 * of a POLICY pi from the logged data alone: fit a fresh Q network to
 *   y = r + ((1 - d) * gamma) * Q_target(s', pi(s'))
 * and report the mean of Q(s0, pi(s0)) over episode-start states.  pi and the dataset are fixed, so pi(s) and
 * pi(s') are computed once per ring slot and the fit needs no policy network.
 *
 * The policy-action table: a caller-allocated device buffer int32 [capacity][2] (not part of the arena),
 * indexed by PHYSICAL ring slot: [slot][0] = argmax_j Q_pi(obs[slot], j), [slot][1] = argmax_j
 * Q_pi(next_obs[slot], j), the first maximum (torch's rule) of the Q row after the head's aggregate.
 *
 * dqnx_policy_sweep: pi = the engine's ONLINE network.  Fills the table entries of the logical range
 *   [lo, hi) in chunks of batch rows: "eval_idx", the route's own forward launches over the chunk's scratch
 *   table with the Double stream set (online(s), online(s'), target(s')) whatever the engine's algorithm, on
 *   the per-layer routes "eval_head", then "policy_rows" (16 lanes per row, two first-maximum butterflies, one
 *   8-byte store per row; rows past the range's end store nothing).  Always 1-step rows: no "nstep_gather",
 *   even on an n-step engine.  Nothing of the training state changes, exactly as under dqnx_eval_range.
 *   Refusals: dqnx_eval_range's, DQNX_EINVAL for table_slots != capacity or a null / misaligned (8 bytes)
 *   table, and DQNX_EUNSUPPORTED on a DQNX_ALGO_DQN engine with conv layers: its conv workspace and split-K
 *   plans are sized for two streams, and the arena does not grow for this call.
 * dqnx_policy_scratch_bytes: the scratch of both sweeps (= dqnx_eval_scratch_bytes).
 *
 * dqnx_set_target_policy: host only, no stream.  With a table set every learn step's target is
 *     y = r + ((1 - d) * gamma) * Q_target(s', table[phys_b][1])
 *   and the step runs the DQN stream set (online(s), target(s'): no online(s') stream, even on a Double
 *   engine; DQNX_BUF_Q[1] is left unwritten, as on a DQNX_ALGO_DQN engine).  Loss, PER weighting, |delta|,
 *   priorities, SumTree updates, clipping, statistics and the soft update are what they were.  The head
 *   kernels' instantiation changes (template parameter TPOL), so the call drops the cached plans and graphs.
 *   An entry outside [0, n_actions) met by a sampled row -- or a sampled slot outside the table, for which
 *   nothing is read -- sets DQNX_DEVERR_TPOL_ACTION (sticky) and that row uses action 0.  dqnx_eval_range is not
 *   affected by a table: it keeps the engine's own target rule.  NULL restores the engine's own rule.  The table is never in the state blob; the caller
 *   keeps it alive while it is set.  Refusals: DQNX_EINVAL for table_slots != capacity; DQNX_EUNSUPPORTED
 *   together with dqnx_set_cql(alpha > 0) -- in either order of the two setters --, with n_step > 1 (an
 *   uncorrected n-step return follows the behaviour policy for n - 1 steps: it would evaluate a mixture of
 *   pi and the behaviour policy, not pi) and with world_size > 1; DQNX_ESTATE under dqnx_set_cql's pending
 *   conditions.  While a table is set dqnx_replay_push and dqnx_state_load return DQNX_ESTATE: they would
 *   make the table stale.
 *
 * dqnx_fqe_range: the number FQE exists for, over the logical range [lo, hi), same plan shape: "eval_idx",
 *   the forward (online(s), target(s')), "eval_head" where needed, "fqe_rows", "fqe_fold".  Per row p (fp32):
 *     q_pi     = Q_online(s_p, table[slot][0])
 *     delta_pi = r + ((1 - d) * gamma) * Q_target(s'_p, table[slot][1]) - Q_online(s_p, a_p)
 *     huber    = the unweighted Huber (beta = 1) of delta_pi
 *   Row p is an EPISODE START when p < n_env or done[p - n_env] != 0: p - n_env is the previous transition
 *   of the same environment ("n-step returns": rows are time-major, env-minor), read through the
 *   logical-to-physical mapping.  The oldest n_env rows therefore count as starts even if the ring cut their
 *   episode.  Table entries outside [0, n_actions) are read as 0 (no error word: nothing here is stateful).
 *   Sums in fp64 in a fixed order (rows of a workgroup, workgroup records, chunks), no floating-point atomics:
 *   two calls on the same state return the same bytes.  rows_out: device [hi - lo][2] fp32 (q_pi, delta_pi),
 *   8-byte aligned, or NULL.  Refusals as dqnx_policy_sweep (any algorithm and route is accepted).
 * dqnx_fqe_kernel_count / _name / dqnx_fqe_chunk_timed: the launches of one chunk of the policy sweep
 *   (which = 0) or of dqnx_fqe_range (which = 1), as dqnx_eval_chunk_timed.
 * dqnx_fqe_row (test hook, host only): one row through csrc/fqe.hpp's serial forms: pi_s / pi_next from the
 *   policy's raw head outputs (first maximum), then the row quantities from the raw outputs of online(s) and
 *   target(s').  Dueling: V then n_actions advantages, n_actions <= 15. */
typedef struct dqnx_fqe_result {
    int64_t rows;                      /* hi - lo */
    int64_t start_rows;                /* episode starts among them */
    double q_pi_sum;                   /* q_pi over all rows */
    double q_pi_start_sum;             /* q_pi over start rows */
    double abs_td_sum;                 /* |delta_pi| */
    double huber_sum;
    double q_pi_max, q_pi_min;
} dqnx_fqe_result;
typedef struct dqnx_fqe_row_result {
    int32_t pi_s, pi_next;
    float q_pi, delta, huber, y;
    float reserved0, reserved1;        /* 0 */
} dqnx_fqe_row_result;
int dqnx_policy_scratch_bytes(const dqnx_engine* e, uint64_t* bytes);
int dqnx_policy_sweep(dqnx_engine* e, int64_t lo, int64_t hi, void* scratch, uint64_t scratch_bytes, int32_t* table,
                      int64_t table_slots, void* stream);
int dqnx_set_target_policy(dqnx_engine* e, const int32_t* table_or_null, int64_t table_slots);
int dqnx_get_target_policy(const dqnx_engine* e, const int32_t** table, int64_t* table_slots);
int dqnx_fqe_range(dqnx_engine* e, int64_t lo, int64_t hi, void* scratch, uint64_t scratch_bytes, const int32_t* table,
                   int64_t table_slots, float* rows_out_or_null, dqnx_fqe_result* result_out_host, void* stream);
int dqnx_fqe_row(const float* raw_online, const float* raw_target_next, const float* raw_policy,
                 const float* raw_policy_next, int32_t head, int32_t n_actions, int32_t action, float reward,
                 float done, float gamma, dqnx_fqe_row_result* out);
int dqnx_fqe_kernel_count(dqnx_engine* e, int32_t which, int32_t* n);
int dqnx_fqe_kernel_name(dqnx_engine* e, int32_t which, int32_t index, char* name, int32_t name_len);
int dqnx_fqe_chunk_timed(dqnx_engine* e, int32_t which, int64_t lo, void* scratch, uint64_t scratch_bytes, int32_t* table,
                         int64_t table_slots, int32_t kernel_index, void* ev_start, void* ev_stop, void* stream);

/* ---- kernel-level timing (bench.py roofline) ---------------------------------------
 * A learn step is an ordered list of kernel launches (sample, linear_fwd_l1.., head_td_loss,
 * linear_bwd_lL..l1, adam_fused).  dqnx_learn_step_timed runs one whole step exactly like
 * dqnx_learn_step but records ev_start/ev_stop (hipEvent_t) around kernel `kernel_index`
 * on `stream` (the sub-ranges before/after it are graph-replayed separately).
 * kernel_count / kernel_info / step_omit with DQNX_STEP_PREFETCH describe the steady-state step
 * of a prefetching loop where the in-launch prefetch applies (no sampler launch; the last
 * launch, "dw_adam16+sample", also draws the next minibatch). */
int dqnx_learn_kernel_count(dqnx_engine* e, int32_t flags, int32_t* n);
int dqnx_learn_kernel_info(dqnx_engine* e, int32_t flags, int32_t index, char* name, int32_t name_len,
                           double* algorithmic_flops, double* algorithmic_bytes);
int dqnx_learn_step_timed(dqnx_engine* e, int32_t flags, int32_t kernel_index, void* ev_start, void* ev_stop,
                          void* stream);
/* Timing aid (bench.py roofline): one learn step (graph-launched when graphs are on), with kernel
 * `omit_index` (as numbered by dqnx_learn_kernel_info; -1 = none) left out.  Engine state
 * afterwards is meant for timing only. */
int dqnx_learn_step_omit(dqnx_engine* e, int32_t flags, int32_t omit_index, void* stream);

int dqnx_events_create(int32_t n, void** events);      /* hipEventCreate x n */
int dqnx_events_destroy(int32_t n, void** events);
int dqnx_event_elapsed(void* start, void* stop, float* ms);   /* synchronises `stop` */

/* ---- sampler (test hook): random.sample positions on device.
 * R:dqn/replay_memory.py:38-39.  mt625: device uint32[625] (advanced in place);
 * n: population size; k: sample size; out: device int32[k].  scratch: device buffer of
 * dqnx_sample_scratch_bytes(n, k) bytes.  err: device int32 (set to 1 if k > n).
 * BLOCKING and not capturable: it stages n into `scratch` from a host stack value and
 * synchronises `stream` before the launch.  Learn steps never call it (their samplers read the
 * ring size from the control block, stream-ordered). */
uint64_t dqnx_sample_scratch_bytes(int64_t n, int32_t k);
int dqnx_sample_uniform(uint32_t* mt625, int64_t n, int32_t k, int32_t* out, void* scratch,
                        int32_t* err, void* stream);

/* ---- misc ------------------------------------------------------------------------ */
const char* dqnx_last_error(void);
int32_t dqnx_abi_version(void);
/* Diagnostic builds only (-DDQNX_STAMPS): copy the 64 s_memtime phase stamps written by
 * block 0 of the sampler / head kernels (synchronises).  Returns DQNX_EUNSUPPORTED in
 * production builds. */
int dqnx_debug_stamps(dqnx_engine* e, int64_t* out64, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DQNX_H */
