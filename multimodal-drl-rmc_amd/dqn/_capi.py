"""ctypes binding of include/dqnx.h (libdqnx.so, the gfx950 HIP engine).

The library is built in-tree (``multimodal-drl-rmc_amd/dqn/_lib/libdqnx.so``, see the
package Makefile / ``__graft_entry__.build()``).  There is no fallback: if the library
is missing this module raises, and every engine entry point that touches the GPU
raises ``RuntimeError`` with ``dqnx_last_error()``.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DQNX_LIB may point at a diagnostic build (e.g. _lib/libdqnx_stamps.so); default: in-tree build.
LIB_PATH = os.environ.get("DQNX_LIB") or os.path.join(_HERE, "_lib", "libdqnx.so")

# ---- constants (mirror dqnx.h) --------------------------------------------------------
DQNX_OK = 0
DQNX_EINVAL, DQNX_ESTATE, DQNX_EUNSUPPORTED, DQNX_EDEVICE = -1, -2, -3, -4
DQNX_NET_MLP, DQNX_NET_TWO_STREAM = 0, 1
DQNX_HEAD_LINEAR, DQNX_HEAD_DUELING = 0, 1
DQNX_ACT_RELU, DQNX_ACT_ELU = 0, 1
DQNX_COMPUTE_FP32, DQNX_COMPUTE_BF16 = 0, 1
DQNX_ALGO_DQN, DQNX_ALGO_DOUBLE, DQNX_ALGO_PER_DOUBLE = 0, 1, 2
DQNX_MAX_DENSE, DQNX_MAX_CONV = 6, 4
(BUF_PARAMS, BUF_TARGET_PARAMS, BUF_GRADS, BUF_ADAM_M, BUF_ADAM_V, BUF_CTRL, BUF_RING_OBS,
 BUF_RING_NEXT_OBS, BUF_RING_ACT, BUF_RING_REW, BUF_RING_DONE, BUF_SUMTREE, BUF_BATCH_IDX, BUF_Q,
 BUF_TD, BUF_IS_WEIGHTS, BUF_WORKSPACE, BUF_PER_ABS_TD, BUF_LEARN_STATS, BUF_GRAD_CLIP, BUF_COUNT) = range(21)
NSTEP_MAX = 16         # largest Config.n_step (DQNX_NSTEP_MAX)
DQNX_RNG_PY, DQNX_RNG_NP = 0, 1
STEP_SOFT_UPDATE = 0x1
STEP_GIVEN_INDICES = 0x2
STEP_GRADS_ONLY = 0x4
STEP_PREFETCH = 0x8
STEP_STATS = 0x10      # accumulate the step's training statistics (dqnx_learn_stats)
AGENT_LAUNCH = 0x100   # dqnx_agent_learn_mt: launch in the same call
CHOOSE_MAX_ENVS = 256
CHOOSE_GIL_HELD = 0x1
DEVERR_SAMPLE_TOO_LARGE = 1
DEVERR_EMPTY_TREE = 2
DEVERR_PER_HANDOFF = 3
DEVERR_FWD_PAIR_HANDOFF = 4
DEVERR_NSTEP_STATE = 19
DEVERR_BOUNDS = {16: "k_adam4 wide path: a float4 outside the launch's element range",
                 17: "k_adam4 wide path: a permuted conv-weight copy outside the launch's range",
                 18: "k_micro_dw: a split-K slab tile outside its conv's slabs"}

I32 = ctypes.c_int32
I64 = ctypes.c_int64


class NetDesc(ctypes.Structure):
    _fields_ = [
        ("kind", I32), ("head", I32), ("activation", I32), ("obs_dim", I32), ("n_actions", I32),
        ("n_dense", I32), ("dense", I32 * DQNX_MAX_DENSE),
        ("macro_len", I32), ("micro_c", I32), ("micro_h", I32), ("micro_w", I32), ("n_conv", I32),
        ("conv_out", I32 * DQNX_MAX_CONV), ("conv_kh", I32 * DQNX_MAX_CONV), ("conv_kw", I32 * DQNX_MAX_CONV),
        ("conv_sh", I32 * DQNX_MAX_CONV), ("conv_sw", I32 * DQNX_MAX_CONV),
    ]


class ParamInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 48), ("offset", I64), ("numel", I64), ("ndim", I32),
                ("shape", I32 * 4)]


class Config(ctypes.Structure):
    _fields_ = [
        ("net", NetDesc), ("algo", I32), ("batch", I32), ("world_size", I32), ("rank", I32),
        ("n_step", I32),   # (in the four bytes that were padding in front of capacity)
        ("capacity", I64), ("gamma", ctypes.c_double), ("lr", ctypes.c_double), ("beta1", ctypes.c_double),
        ("beta2", ctypes.c_double), ("adam_eps", ctypes.c_double), ("tau", ctypes.c_double), ("n_env", I32),
        ("local_sampling", I32), ("per_eps", ctypes.c_double), ("per_alpha", ctypes.c_double),
        ("per_max_priority", ctypes.c_double), ("per_beta_start", ctypes.c_double),
        ("per_beta_end", ctypes.c_double), ("per_beta_steps", ctypes.c_double),
        ("compute_dtype", I32), ("per_numpy121", I32),
    ]


class Ctrl(ctypes.Structure):
    _fields_ = [
        ("py_mt", ctypes.c_uint32 * 625), ("np_mt", ctypes.c_uint32 * 625), ("ring_size", I64),
        ("ring_wptr", I64), ("adam_step", I64), ("agent_step", I64), ("per_max_idx", I64),
        ("per_min_idx", I64), ("loss", ctypes.c_float), ("error", I32), ("adam_step_size", ctypes.c_float),
        ("adam_bc2_sqrt", ctypes.c_float), ("per_beta", ctypes.c_double), ("reserved", I64 * 8),
    ]


# training statistics (dqnx.h "training statistics")
STATS_MAX_ACTIONS, STATS_TD_BINS, STATS_MAX_TENSORS = 16, 16, 32


class LearnStats(ctypes.Structure):
    _fields_ = [
        ("steps", I64), ("rows", I64), ("q_sa_sum", ctypes.c_double), ("q_sa_sq_sum", ctypes.c_double),
        ("q_max_sum", ctypes.c_double), ("target_sum", ctypes.c_double), ("abs_td_sum", ctypes.c_double),
        ("gap_sum", ctypes.c_double), ("reward_sum", ctypes.c_double), ("isw_sum", ctypes.c_double),
        ("loss_sum", ctypes.c_double), ("grad_norm_sum", ctypes.c_double), ("grad_norm_max", ctypes.c_double),
        ("huber_linear_rows", I64), ("agree_rows", I64), ("done_rows", I64),
        ("td_hist", I64 * STATS_TD_BINS), ("greedy_hist", I64 * STATS_MAX_ACTIONS),
        ("taken_hist", I64 * STATS_MAX_ACTIONS),
        ("grad_sq_last", ctypes.c_double * STATS_MAX_TENSORS), ("param_sq_last", ctypes.c_double * STATS_MAX_TENSORS),
        ("grad_sq_sum", ctypes.c_double * STATS_MAX_TENSORS),
        ("q_sa_min", ctypes.c_float), ("q_sa_max", ctypes.c_float), ("q_max_max", ctypes.c_float),
        ("target_min", ctypes.c_float), ("target_max", ctypes.c_float), ("abs_td_max", ctypes.c_float),
        ("isw_min", ctypes.c_float), ("reserved0", ctypes.c_float),
    ]


# gradient clipping (dqnx.h "gradient clipping")
class GradClipInfo(ctypes.Structure):
    _fields_ = [("steps", I64), ("clipped_steps", I64), ("norm_sum", ctypes.c_double), ("norm_max", ctypes.c_double),
                ("last_norm", ctypes.c_float), ("last_coef", ctypes.c_float)]


# offline evaluation (dqnx.h "offline evaluation")
class EvalResult(ctypes.Structure):
    _fields_ = [
        ("rows", I64), ("huber_sum", ctypes.c_double), ("abs_td_sum", ctypes.c_double), ("td_sq_sum", ctypes.c_double),
        ("q_sa_sum", ctypes.c_double), ("v_sum", ctypes.c_double), ("cql_gap_sum", ctypes.c_double),
        ("action_gap_sum", ctypes.c_double), ("reward_sum", ctypes.c_double), ("target_sum", ctypes.c_double),
        ("abs_td_max", ctypes.c_double), ("v_max", ctypes.c_double), ("v_min", ctypes.c_double),
        ("agree_rows", I64), ("done_rows", I64),
        ("greedy_hist", I64 * STATS_MAX_ACTIONS), ("taken_hist", I64 * STATS_MAX_ACTIONS),
    ]


class EvalRowResult(ctypes.Structure):
    _fields_ = [("greedy", I32), ("action", I32), ("q_a", ctypes.c_float), ("v", ctypes.c_float),
                ("delta", ctypes.c_float), ("huber", ctypes.c_float), ("gap", ctypes.c_float),
                ("action_gap", ctypes.c_float), ("y", ctypes.c_float), ("reserved0", ctypes.c_float)]


# fitted Q evaluation (dqnx.h "fitted Q evaluation")
DEVERR_TPOL_ACTION = 20


class FqeResult(ctypes.Structure):
    _fields_ = [("rows", I64), ("start_rows", I64), ("q_pi_sum", ctypes.c_double), ("q_pi_start_sum", ctypes.c_double),
                ("abs_td_sum", ctypes.c_double), ("huber_sum", ctypes.c_double), ("q_pi_max", ctypes.c_double),
                ("q_pi_min", ctypes.c_double)]


class FqeRowResult(ctypes.Structure):
    _fields_ = [("pi_s", I32), ("pi_next", I32), ("q_pi", ctypes.c_float), ("delta", ctypes.c_float),
                ("huber", ctypes.c_float), ("y", ctypes.c_float), ("reserved0", ctypes.c_float),
                ("reserved1", ctypes.c_float)]


# training-state snapshot (dqnx.h "training-state snapshot")
STATE_MAGIC = 0x54415453584E5144   # b"DQNXSTAT" little-endian
STATE_VERSION = 1
STATE_ALIGN = 4
STATE_MAX_SECTIONS = 16
(SEC_PARAMS, SEC_TARGET_PARAMS, SEC_ADAM_M, SEC_ADAM_V, SEC_CTRL, SEC_RING_OBS, SEC_RING_NEXT_OBS, SEC_RING_ACT,
 SEC_RING_REW, SEC_RING_DONE, SEC_SUMTREE) = range(1, 12)
SEC_NAMES = {SEC_PARAMS: "params", SEC_TARGET_PARAMS: "target_params", SEC_ADAM_M: "adam_m", SEC_ADAM_V: "adam_v",
             SEC_CTRL: "ctrl", SEC_RING_OBS: "ring_obs", SEC_RING_NEXT_OBS: "ring_next_obs", SEC_RING_ACT: "ring_act",
             SEC_RING_REW: "ring_rew", SEC_RING_DONE: "ring_done", SEC_SUMTREE: "sumtree"}


class StateSection(ctypes.Structure):
    _fields_ = [("id", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("offset", ctypes.c_uint64),
                ("bytes", ctypes.c_uint64)]


class StateInfo(ctypes.Structure):
    _fields_ = [
        ("magic", ctypes.c_uint64), ("version", ctypes.c_uint32), ("header_bytes", ctypes.c_uint32),
        ("total_bytes", ctypes.c_uint64), ("net", NetDesc), ("algo", I32), ("compute_dtype", I32),
        ("per_numpy121", I32), ("n_sections", I32), ("reserved0", I32), ("capacity", I64), ("n_params", I64),
        ("ring_size", I64), ("ring_wptr", I64), ("sections", StateSection * STATE_MAX_SECTIONS),
    ]


# every symbol the header declares (checked by tests/test_capi.py)
EXPORTS = [
    "dqnx_net_param_count", "dqnx_net_param_info", "dqnx_config_defaults", "dqnx_engine_create",
    "dqnx_engine_destroy", "dqnx_engine_arena_bytes", "dqnx_engine_buffer", "dqnx_engine_obs_stride",
    "dqnx_engine_bind", "dqnx_engine_reset", "dqnx_engine_set_graphs", "dqnx_replay_push", "dqnx_rng_set",
    "dqnx_rng_get", "dqnx_rng_set_async", "dqnx_rng_get_async", "dqnx_learn_step", "dqnx_learn_steps", "dqnx_prefetch_begin", "dqnx_prefetch_stream", "dqnx_apply_grads", "dqnx_soft_update", "dqnx_hard_update",
    "dqnx_sample_scratch_bytes", "dqnx_sample_uniform", "dqnx_last_error", "dqnx_abi_version",
    "dqnx_learn_kernel_count", "dqnx_learn_kernel_info", "dqnx_learn_step_timed", "dqnx_learn_step_omit", "dqnx_events_create",
    "dqnx_events_destroy", "dqnx_event_elapsed", "dqnx_debug_stamps",
    "dqnx_per_sample", "dqnx_per_update_priorities", "dqnx_set_agent_step", "dqnx_act", "dqnx_act_scratch_bytes",
    "dqnx_params_modified", "dqnx_dp_bucket_count", "dqnx_dp_bucket_info", "dqnx_learn_step_bucket",
    "dqnx_apply_grads_bucket", "dqnx_ctrl_get_async", "dqnx_rng_sample_words", "dqnx_rng_advance",
    "dqnx_agent_stage_rng", "dqnx_agent_launch", "dqnx_agent_readback", "dqnx_act_host_scratch_bytes",
    "dqnx_act_host", "dqnx_agent_learn_mt", "dqnx_agent_quiesce", "dqnx_agent_choose", "dqnx_act_kernel_count",
    "dqnx_state_bytes", "dqnx_state_save", "dqnx_state_load", "dqnx_state_inspect",
    "dqnx_learn_stats_get", "dqnx_learn_stats_reset",
    "dqnx_set_grad_clip", "dqnx_get_grad_clip", "dqnx_grad_clip_info_get",
    "dqnx_nstep_window", "dqnx_nstep_buffer",
    "dqnx_set_cql", "dqnx_get_cql", "dqnx_cql_row",
    "dqnx_eval_scratch_bytes", "dqnx_eval_range", "dqnx_eval_row", "dqnx_eval_kernel_count",
    "dqnx_eval_kernel_name", "dqnx_eval_chunk_timed",
    "dqnx_policy_scratch_bytes", "dqnx_policy_sweep", "dqnx_set_target_policy", "dqnx_get_target_policy",
    "dqnx_fqe_range", "dqnx_fqe_row", "dqnx_fqe_kernel_count", "dqnx_fqe_kernel_name", "dqnx_fqe_chunk_timed",
]

GIL_HELD = ("dqnx_agent_learn_mt", "dqnx_agent_choose")   # entry points called with the GIL held (see lib())

_lib = None


class DqnxError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"libdqnx.so not built ({LIB_PATH}); run `make -C multimodal-drl-rmc_amd` or "
            "__graft_entry__.build().  There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    P = ctypes.POINTER
    sig = {
        "dqnx_net_param_count": ([P(NetDesc), P(I64), P(I32)], ctypes.c_int),
        "dqnx_net_param_info": ([P(NetDesc), I32, P(ParamInfo)], ctypes.c_int),
        "dqnx_config_defaults": ([P(Config)], None),
        "dqnx_engine_create": ([P(Config), P(vp)], ctypes.c_int),
        "dqnx_engine_destroy": ([vp], ctypes.c_int),
        "dqnx_engine_arena_bytes": ([vp, P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_engine_buffer": ([vp, I32, P(ctypes.c_uint64), P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_engine_obs_stride": ([vp, P(I32)], ctypes.c_int),
        "dqnx_engine_bind": ([vp, vp, ctypes.c_uint64], ctypes.c_int),
        "dqnx_engine_reset": ([vp, vp], ctypes.c_int),
        "dqnx_params_modified": ([vp], ctypes.c_int),
        "dqnx_engine_set_graphs": ([vp, I32], ctypes.c_int),
        "dqnx_replay_push": ([vp, vp, vp, vp, vp, vp, I32, I32, vp], ctypes.c_int),
        "dqnx_rng_set": ([vp, I32, P(ctypes.c_uint32), vp], ctypes.c_int),
        "dqnx_rng_get": ([vp, I32, P(ctypes.c_uint32), vp], ctypes.c_int),
        "dqnx_rng_set_async": ([vp, I32, vp, vp], ctypes.c_int),
        "dqnx_rng_get_async": ([vp, I32, vp, vp], ctypes.c_int),
        "dqnx_learn_step": ([vp, I32, vp], ctypes.c_int),
        "dqnx_learn_steps": ([vp, I32, I32, vp], ctypes.c_int),
        "dqnx_prefetch_begin": ([vp, I32, vp], ctypes.c_int),
        "dqnx_prefetch_stream": ([vp, vp], ctypes.c_int),
        "dqnx_apply_grads": ([vp, I32, vp], ctypes.c_int),
        "dqnx_dp_bucket_count": ([vp, P(I32)], ctypes.c_int),
        "dqnx_dp_bucket_info": ([vp, I32, P(I64), P(I64)], ctypes.c_int),
        "dqnx_learn_step_bucket": ([vp, I32, I32, vp], ctypes.c_int),
        "dqnx_apply_grads_bucket": ([vp, I32, I32, vp], ctypes.c_int),
        "dqnx_soft_update": ([vp, vp], ctypes.c_int),
        "dqnx_hard_update": ([vp, vp], ctypes.c_int),
        "dqnx_sample_scratch_bytes": ([I64, I32], ctypes.c_uint64),
        "dqnx_sample_uniform": ([vp, I64, I32, vp, vp, vp, vp], ctypes.c_int),
        "dqnx_last_error": ([], ctypes.c_char_p),
        "dqnx_learn_kernel_count": ([vp, I32, P(I32)], ctypes.c_int),
        "dqnx_learn_kernel_info": ([vp, I32, I32, ctypes.c_char_p, I32, P(ctypes.c_double), P(ctypes.c_double)],
                                   ctypes.c_int),
        "dqnx_learn_step_timed": ([vp, I32, I32, vp, vp, vp], ctypes.c_int),
        "dqnx_learn_step_omit": ([vp, I32, I32, vp], ctypes.c_int),
        "dqnx_events_create": ([I32, P(vp)], ctypes.c_int),
        "dqnx_events_destroy": ([I32, P(vp)], ctypes.c_int),
        "dqnx_event_elapsed": ([vp, vp, P(ctypes.c_float)], ctypes.c_int),
        "dqnx_abi_version": ([], I32),
        "dqnx_debug_stamps": ([vp, P(I64), vp], ctypes.c_int),
        "dqnx_per_sample": ([vp, vp], ctypes.c_int),
        "dqnx_per_update_priorities": ([vp, vp, vp, I32, vp], ctypes.c_int),
        "dqnx_set_agent_step": ([vp, I64, vp], ctypes.c_int),
        "dqnx_act": ([P(NetDesc), vp, vp, I32, vp, vp, vp, ctypes.c_uint64, vp], ctypes.c_int),
        "dqnx_act_scratch_bytes": ([P(NetDesc), I32], ctypes.c_uint64),
        "dqnx_act_kernel_count": ([P(NetDesc), I32, P(I32)], ctypes.c_int),
        "dqnx_ctrl_get_async": ([vp, vp, vp], ctypes.c_int),
        "dqnx_rng_sample_words": ([vp, I64, I32, vp, P(I64)], ctypes.c_int),
        "dqnx_rng_advance": ([vp, I64, vp], ctypes.c_int),
        "dqnx_agent_stage_rng": ([vp, I32, vp, P(I64)], ctypes.c_int),
        "dqnx_agent_launch": ([vp, I32, vp], ctypes.c_int),
        "dqnx_agent_learn_mt": ([vp, vp, vp, I32, vp, P(I64)], ctypes.c_int),
        "dqnx_agent_readback": ([vp, I32, vp], ctypes.c_int),
        "dqnx_agent_quiesce": ([vp], ctypes.c_int),
        "dqnx_agent_choose": ([vp, vp, I32, ctypes.c_double, vp, vp, vp, vp, ctypes.c_uint64, I32, vp], ctypes.c_int),
        "dqnx_act_host_scratch_bytes": ([P(NetDesc), I32], ctypes.c_uint64),
        "dqnx_act_host": ([P(NetDesc), vp, vp, I32, vp, vp, ctypes.c_uint64, vp], ctypes.c_int),
        "dqnx_state_bytes": ([vp, P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_state_save": ([vp, vp, ctypes.c_uint64, P(ctypes.c_uint64), vp], ctypes.c_int),
        "dqnx_state_load": ([vp, vp, ctypes.c_uint64, vp], ctypes.c_int),
        "dqnx_state_inspect": ([vp, ctypes.c_uint64, P(StateInfo)], ctypes.c_int),
        "dqnx_learn_stats_get": ([vp, P(LearnStats), I32, vp], ctypes.c_int),
        "dqnx_learn_stats_reset": ([vp, vp], ctypes.c_int),
        "dqnx_set_grad_clip": ([vp, ctypes.c_double], ctypes.c_int),
        "dqnx_get_grad_clip": ([vp, P(ctypes.c_double)], ctypes.c_int),
        "dqnx_grad_clip_info_get": ([vp, P(GradClipInfo), I32, vp], ctypes.c_int),
        "dqnx_nstep_buffer": ([vp, P(ctypes.c_uint64), P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_set_cql": ([vp, ctypes.c_double], ctypes.c_int),
        "dqnx_get_cql": ([vp, P(ctypes.c_double)], ctypes.c_int),
        "dqnx_cql_row": ([P(ctypes.c_float), I32, I32, P(ctypes.c_float), P(ctypes.c_float)], ctypes.c_int),
        "dqnx_eval_scratch_bytes": ([vp, P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_eval_range": ([vp, I64, I64, vp, ctypes.c_uint64, vp, P(EvalResult), vp], ctypes.c_int),
        "dqnx_eval_row": ([P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float), I32, I32, I32, I32,
                           ctypes.c_float, ctypes.c_float, ctypes.c_float, P(EvalRowResult)], ctypes.c_int),
        "dqnx_eval_kernel_count": ([vp, P(I32)], ctypes.c_int),
        "dqnx_eval_kernel_name": ([vp, I32, ctypes.c_char_p, I32], ctypes.c_int),
        "dqnx_eval_chunk_timed": ([vp, I64, vp, ctypes.c_uint64, I32, vp, vp, vp], ctypes.c_int),
        "dqnx_policy_scratch_bytes": ([vp, P(ctypes.c_uint64)], ctypes.c_int),
        "dqnx_policy_sweep": ([vp, I64, I64, vp, ctypes.c_uint64, vp, I64, vp], ctypes.c_int),
        "dqnx_set_target_policy": ([vp, vp, I64], ctypes.c_int),
        "dqnx_get_target_policy": ([vp, P(vp), P(I64)], ctypes.c_int),
        "dqnx_fqe_range": ([vp, I64, I64, vp, ctypes.c_uint64, vp, I64, vp, P(FqeResult), vp], ctypes.c_int),
        "dqnx_fqe_row": ([P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float), P(ctypes.c_float), I32, I32, I32,
                          ctypes.c_float, ctypes.c_float, ctypes.c_float, P(FqeRowResult)], ctypes.c_int),
        "dqnx_fqe_kernel_count": ([vp, I32, P(I32)], ctypes.c_int),
        "dqnx_fqe_kernel_name": ([vp, I32, I32, ctypes.c_char_p, I32], ctypes.c_int),
        "dqnx_fqe_chunk_timed": ([vp, I32, I64, vp, ctypes.c_uint64, vp, I64, I32, vp, vp, vp], ctypes.c_int),
        "dqnx_nstep_window": ([vp, vp, I64, I64, I32, I32, ctypes.c_double, P(ctypes.c_float), P(ctypes.c_float),
                               P(ctypes.c_float), P(I64), P(I32)], ctypes.c_int),
    }
    # dqnx_agent_learn_mt reads and writes random._inst's MT words in place: call it through a PyDLL
    # handle, which keeps the GIL for the call (a CDLL call releases it, and another thread's `random`
    # use could then see a torn generator state; the reference's random.sample holds the GIL throughout)
    L_gil = ctypes.PyDLL(LIB_PATH)
    for name, (args, res) in sig.items():
        f = getattr(L_gil if name in GIL_HELD else L, name)
        f.argtypes = args
        f.restype = res
        if name in GIL_HELD:
            setattr(L, name, f)
    _lib = L
    return L


def check(rc: int, what: str = ""):
    if rc != DQNX_OK:
        msg = lib().dqnx_last_error().decode(errors="replace")
        err = DqnxError(f"{what}: dqnx error {rc}: {msg}")
        err.code = rc   # the DQNX_E* status, for callers that tell refusals apart
        raise err
    return rc
