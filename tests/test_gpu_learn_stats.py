"""GPU: on-device training statistics of the learn step (DQNX_STEP_STATS, dqnx_learn_stats_get,
LearnEngine.learn_stats, Agent.log with DQNX_LEARN_STATS=1).

The reference for every value is numpy in float64 over the engine's OWN buffers, read back after each
step (q, td, grads, params, is_weights, the minibatch indices and the ring columns, ctrl().loss): the
other GPU tests hold those buffers to the oracle, this file holds the statistics to the buffers.

Tolerances follow from the arithmetic.  Counts, histograms and extrema are compared with ==.  The
kernel adds exact fp64 terms in another order than numpy: reordering n <= 2^20 non-negative fp64 terms
moves a sum by at most n * 2^-53 ~ 1.2e-10 relative, so sums of squares and the gradient norms get
1e-9 relative, and signed sums |err| <= 1e-9 * sum |x|.  The (4,84,84) net, a case this file adds, has one
tensor of 2^24.8 elements: its sum of squares alone is held to n * 2^-53 ~ 3.2e-9, the same argument."""
import ctypes
import functools
import math
import random

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from oracle import ref as O
from refnets import agent_kwargs

pytestmark = pytest.mark.gpu

REL = 1e-9
SUMS = ("q_sa_sum", "q_max_sum", "target_sum", "abs_td_sum", "gap_sum", "reward_sum", "isw_sum", "loss_sum")
EXACT = ("steps", "rows", "huber_linear_rows", "agree_rows", "done_rows", "q_sa_min", "q_sa_max", "q_max_max",
         "target_min", "target_max", "abs_td_max", "isw_min")
HISTS = ("td_hist", "greedy_hist", "taken_hist")


# ---- data and engines --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transitions(n, obs_dim, n_actions, seed):
    """Synthetic rows in which every action occurs, a quarter of the rows are terminal and half of the
    rewards are small (so |delta| spreads over several exponent bins)."""
    obs, act, rew, done, nobs = O.synth_transitions(n, obs_dim, n_actions, seed=seed)
    rng = np.random.default_rng(seed + 1)
    act = rng.permutation(np.arange(n, dtype=np.int64) % n_actions)
    done = rng.random(n) < 0.25
    rew = (rew * np.where(rng.random(n) < 0.5, 0.02, 1.0)).astype(np.float32)
    assert set(act.tolist()) == set(range(n_actions)), "every action must occur"
    assert done.any() and not done.all(), "done and not-done rows must both occur"
    return obs, act, rew, done, nobs


CASES = {
    # name: (net, n_actions, head, algo, batch, capacity, rows pushed, engine kwargs, steps)
    "mlp14": (14, 8, "dueling", "DuelingDoubleDQNAgent", 32, 200, 150, {}, 3),
    "mlp14_wrapped": (14, 8, "dueling", "DuelingDoubleDQNAgent", 32, 200, 260, {}, 3),   # the ring has wrapped
    "linear_a3_b100": (14, 3, "linear", "DQNAgent", 100, 200, 150, {}, 3),
    "mlp14_b300": (14, 8, "dueling", "DuelingDoubleDQNAgent", 300, 400, 350, {}, 3),   # two batch workgroups
    "per_b64": (14, 8, "dueling", "PerDuelingDoubleDQNAgent", 64, 256, 200, {}, 3),
    "per_b64_wrapped": (14, 8, "dueling", "PerDuelingDoubleDQNAgent", 64, 256, 300, {}, 3),
    "mlp284_bf16": (284, 8, "dueling", "DuelingDoubleDQNAgent", 64, 200, 150, {"compute_dtype": "bf16"}, 3),
    "head": ("hybrid", 8, "dueling", "DuelingDoubleDQNAgent", 32, 200, 150, {}, 3),
    "head_per": ("hybrid", 8, "dueling", "PerDuelingDoubleDQNAgent", 32, 200, 150, {}, 3),
    "hybrid84": ("hybrid84", 8, "dueling", "DuelingDoubleDQNAgent", 32, 100, 60, {}, 2),
}
# routes selected through the environment when the engine plans its step
ROUTE_ENV = {"mlp14_per_layer": ("mlp14", {"DQNX_BWD_PLAN": "0"}),
             "mlp14_slab": ("mlp14", {"DQNX_DW_ADAM16": "0", "DQNX_ADAM_BLK": "1"})}


def make(case, seed=3, **over):
    net, A, head, algo, batch, cap, n_push, kw, _ = CASES[case]
    if net == "hybrid":
        spec, ospec = E.hybrid_spec(A, head), O.hybrid_spec(A, head)
    elif net == "hybrid84":
        spec, ospec = E.hybrid_spec(A, head, micro_chw=(4, 84, 84)), O.hybrid_spec(A, head, micro_chw=(4, 84, 84))
    else:
        spec, ospec = E.mlp_spec(net, A, head), O.mlp_spec(net, A, head)
    eng = E.LearnEngine(spec, algo, batch, cap, **{**kw, **over})
    eng.load_params(O.reference_init(ospec, seed))
    eng.push(*transitions(n_push, spec.obs_dim, A, seed + 100))
    random.seed(seed + 7)
    np.random.seed(seed + 7)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    eng.set_rng(C.DQNX_RNG_NP, O.np_state_to_array())
    return eng


def is_per(eng):
    return eng.cfg.algo == C.DQNX_ALGO_PER_DOUBLE


def block_bytes(eng):
    torch.cuda.synchronize()
    return eng.learn_stats_view.cpu().numpy().tobytes()


def raw_block(eng):
    return C.LearnStats.from_buffer_copy(block_bytes(eng))


# ---- the numpy reference -------------------------------------------------------------------------
def step_reference(eng, slot=0):
    """One step's statistics from the engine's buffers, in float64."""
    torch.cuda.synchronize()
    f8 = np.float64
    P, cap = eng.n_params, eng.capacity
    q = eng.q[0].cpu().numpy()
    y, qsa, ad = eng.td.cpu().numpy()
    idx = eng.batch_idx_slots[slot].cpu().numpy().astype(np.int64)
    # uniform replay stores logical positions, PER ring slots
    phys = idx if is_per(eng) else (eng.ring_wptr - eng.ring_size + idx) % cap
    act = eng.ring_act.cpu().numpy()[phys].astype(np.int64)
    rew = eng.ring_rew.cpu().numpy()[phys]
    done = eng.ring_done.cpu().numpy()[phys]
    g = eng.grads[:P].cpu().numpy().astype(f8)
    p = eng.params.cpu().numpy().astype(f8)
    A = q.shape[1]
    greedy = q.argmax(axis=1)
    srt = np.sort(q, axis=1)[:, ::-1]
    gap = (srt[:, 0] - srt[:, 1]) if A > 1 else np.zeros(len(q), np.float32)
    assert gap.dtype == np.float32
    e = np.where(ad == 0, -127, np.frexp(ad)[1] - 1)   # unbiased exponent (frexp's mantissa is in [0.5, 1))
    bins = np.clip(e + 12, 0, 15)
    qmax = q.max(axis=1)
    r = {"steps": 1, "rows": len(q)}
    terms = {"q_sa_sum": qsa, "q_max_sum": qmax, "target_sum": y, "abs_td_sum": ad, "gap_sum": gap, "reward_sum": rew,
             "isw_sum": eng.is_weights.cpu().numpy() if is_per(eng) else np.zeros(1, np.float32),
             "loss_sum": np.array([eng.ctrl().loss], np.float32)}
    for k, x in terms.items():
        r[k] = x.astype(f8).sum()
        r[k + "_abs"] = np.abs(x.astype(f8)).sum()
    r["q_sa_sq_sum"] = (qsa.astype(f8) ** 2).sum()
    r.update(q_sa_min=qsa.min(), q_sa_max=qsa.max(), q_max_max=qmax.max(), target_min=y.min(), target_max=y.max(),
             abs_td_max=ad.max(), isw_min=eng.is_weights.cpu().numpy().min() if is_per(eng) else np.float32(0))
    r.update(huber_linear_rows=int((ad >= 1).sum()), agree_rows=int((greedy == act).sum()), done_rows=int((done != 0).sum()))
    r["td_hist"] = np.bincount(bins, minlength=16)
    r["greedy_hist"] = np.bincount(greedy, minlength=16)
    r["taken_hist"] = np.bincount(act, minlength=16)
    lay = eng.param_layout
    ends = [off for _, off, _ in lay[1:]] + [P]
    r["grad_sq"] = np.array([(g[off:end] ** 2).sum() for (_, off, _), end in zip(lay, ends)])
    r["param_sq"] = np.array([(p[off:end] ** 2).sum() for (_, off, _), end in zip(lay, ends)])
    r["numel"] = np.array([end - off for (_, off, _), end in zip(lay, ends)])
    return r


def accumulate(refs):
    """The block after the steps of `refs`, starting from a zeroed one."""
    out = {}
    for k in ("steps", "rows", "huber_linear_rows", "agree_rows", "done_rows", "q_sa_sq_sum") + SUMS + HISTS \
            + tuple(s + "_abs" for s in SUMS):
        out[k] = sum(r[k] for r in refs)
    for k in ("q_sa_min", "target_min", "isw_min"):
        out[k] = min(r[k] for r in refs)
    for k in ("q_sa_max", "q_max_max", "target_max", "abs_td_max"):
        out[k] = max(r[k] for r in refs)
    norms = [math.sqrt(r["grad_sq"].sum()) for r in refs]
    out.update(grad_sq_last=refs[-1]["grad_sq"], param_sq_last=refs[-1]["param_sq"], numel=refs[-1]["numel"],
               grad_sq_sum=sum(r["grad_sq"] for r in refs), grad_norm_sum=sum(norms), grad_norm_max=max(norms))
    return out


def check_block(st, want, what=""):
    """st: C.LearnStats read from the device; want: accumulate(...)."""
    for k in EXACT:
        print(what, k, getattr(st, k), want[k])
        assert getattr(st, k) == want[k], (what, k, getattr(st, k), want[k])
    for k in HISTS:
        got = np.array(getattr(st, k)[:], dtype=np.int64)
        print(what, k, got.tolist())
        assert np.array_equal(got, want[k]), (what, k, got, want[k])
    for k in SUMS:
        err, bound = abs(getattr(st, k) - want[k]), REL * want[k + "_abs"]
        print(what, k, getattr(st, k), want[k], "err", err, "bound", bound)
        assert err <= bound, (what, k, getattr(st, k), want[k], err, bound)
    nt = len(want["numel"])
    # sums of squares: relative 1e-9 (n * 2^-53 of the reordering for n <= 2^20; larger tensors n * 2^-53)
    rel = np.maximum(REL, want["numel"] * 2.0 ** -53)
    for k in ("grad_sq_last", "param_sq_last", "grad_sq_sum"):
        got = np.array(getattr(st, k)[:], dtype=np.float64)
        err = np.abs(got[:nt] - want[k])
        print(what, k, "max rel err", float((err / np.maximum(want[k], 1e-300)).max()))
        assert (err <= rel * want[k]).all(), (what, k, got[:nt], want[k])
        assert not got[nt:].any(), (what, k, "entries past the net's tensors must stay zero")
    for k in ("q_sa_sq_sum", "grad_norm_sum", "grad_norm_max"):
        err = abs(getattr(st, k) - want[k])
        print(what, k, getattr(st, k), want[k], "rel err", err / want[k])
        assert err <= REL * want[k], (what, k, getattr(st, k), want[k])


# ---- value parity ---------------------------------------------------------------------------------
def run_parity(case):
    eng = make(case)
    refs = []
    for step in range(CASES[case][8]):
        eng.learn_step(soft_update=True, stats=True)
        eng.check_device_error()
        refs.append(step_reference(eng))
        check_block(raw_block(eng), accumulate(refs), f"{case} step {step}")
    # the histograms are not trivially one bin
    want = accumulate(refs)
    assert (want["taken_hist"] > 0).sum() >= min(3, eng.spec.n_actions) and (want["td_hist"] > 0).sum() >= 2
    assert 0 < want["done_rows"] < want["rows"]
    return eng, refs


@pytest.mark.parametrize("case", list(CASES))
def test_gpu_learn_stats_match_numpy_after_every_step(case):
    """The block after step k equals the numpy accumulation of the k per-step references (so this is
    the accumulate check too)."""
    eng, refs = run_parity(case)
    if is_per(eng):
        assert raw_block(eng).isw_sum > 0 and raw_block(eng).isw_min > 0
    else:
        assert raw_block(eng).isw_sum == 0 and raw_block(eng).isw_min == 0


@pytest.mark.parametrize("route", list(ROUTE_ENV))
def test_gpu_learn_stats_other_mlp_plans(monkeypatch, route):
    """The per-layer plan (ring rows through the step's physical slots) and the slab plan's Adam pass."""
    case, env = ROUTE_ENV[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_parity(case)


# ---- read-only, determinism -----------------------------------------------------------------------
def end_state(eng):
    torch.cuda.synchronize()
    return {"params": eng.params.cpu().clone(), "target": eng.target_params.cpu().clone(), "m": eng.adam_m.cpu().clone(),
            "v": eng.adam_v.cpu().clone(), "tree": eng.sumtree.cpu().clone(), "q": eng.q.cpu().clone(),
            "td": eng.td.cpu().clone(), "grads": eng.grads.cpu().clone(), "loss": np.float32(eng.ctrl().loss),
            "py": eng.get_rng(C.DQNX_RNG_PY), "np": eng.get_rng(C.DQNX_RNG_NP)}


def assert_state_equal(a, b):
    for k in ("params", "target", "m", "v", "tree", "q", "td", "grads"):
        assert torch.equal(a[k], b[k]), k
    assert a["loss"].tobytes() == b["loss"].tobytes()
    assert np.array_equal(a["py"], b["py"]) and np.array_equal(a["np"], b["np"])


@pytest.mark.parametrize("case", ["mlp14", "per_b64", "head"])
def test_gpu_learn_stats_launch_is_read_only(case):
    """Four steps with and without the flag: parameters, target, Adam moments, loss, both RNG streams
    and the SumTree are bitwise equal, and so are the two state blobs (the block is not state)."""
    with_stats, without = make(case), make(case)
    for _ in range(4):
        with_stats.learn_step(soft_update=True, stats=True)
        without.learn_step(soft_update=True)
    assert_state_equal(end_state(with_stats), end_state(without))
    assert raw_block(with_stats).steps == 4 and not any(block_bytes(without))
    assert with_stats.state_blob().tobytes() == without.state_blob().tobytes()


@pytest.mark.parametrize("case", ["mlp14_b300", "per_b64", "head"])
def test_gpu_learn_stats_deterministic(case):
    a, b = make(case), make(case)
    for _ in range(4):
        a.learn_step(soft_update=True, stats=True)
        b.learn_step(soft_update=True, stats=True)
    assert block_bytes(a) == block_bytes(b)
    assert raw_block(a).steps == 4


# ---- every route to the launch --------------------------------------------------------------------
def run_route(case, route):
    eng = make(case, graphs=(route == "graphed"))
    if route == "learn_steps":
        eng.learn_steps(4, soft_update=True, stats=True)
    else:
        for _ in range(4):
            eng.learn_step(soft_update=True, stats=True, prefetch=(route == "prefetch"))
    eng.check_device_error()
    return block_bytes(eng), end_state(eng)["params"]


@pytest.mark.parametrize("case", ["mlp14", "per_b64", "head"])
def test_gpu_learn_stats_every_route_agrees(case):
    """eager, graph-captured, the one-call learn_steps loop and prefetching steps (the step's own
    indices are overwritten by the draw-ahead before the statistics launch runs) leave the same bytes."""
    eager, p0 = run_route(case, "eager")
    assert C.LearnStats.from_buffer_copy(eager).steps == 4
    for route in ("graphed", "learn_steps", "prefetch"):
        got, p = run_route(case, route)
        assert torch.equal(p, p0), route
        assert got == eager, route


def test_gpu_learn_stats_side_stream_prefetch_reads_the_steps_own_slot(monkeypatch):
    """The per-layer plan's prefetch pipeline alternates the two (idx, phys) slots: step t computes on
    slot t % 2 while the side stream draws step t + 1 into the other.  The statistics of step t must
    come through slot t % 2 (here: held to numpy over that slot after every step)."""
    monkeypatch.setenv("DQNX_BWD_PLAN", "0")
    eng = make("mlp14_wrapped")
    refs = []
    for step in range(4):
        eng.learn_step(soft_update=True, stats=True, prefetch=True)
        refs.append(step_reference(eng, slot=step % 2))
        check_block(raw_block(eng), accumulate(refs), f"side-stream prefetch step {step}")
    eng.check_device_error()
    assert not torch.equal(eng.batch_idx_slots[0], eng.batch_idx_slots[1])
    assert refs[2]["taken_hist"].tolist() != refs[3]["taken_hist"].tolist() or refs[2]["reward_sum"] != refs[3]["reward_sum"]


# ---- accumulate / reset ---------------------------------------------------------------------------
def test_gpu_learn_stats_read_and_reset():
    eng, refs = run_parity("mlp14")
    want = accumulate(refs)
    d = eng.learn_stats(reset=True)
    assert d["steps"] == 3 and d["rows"] == 96
    for k in SUMS:
        assert abs(d[k] - want[k]) <= REL * want[k + "_abs"], k
    assert np.array_equal(d["greedy_hist"], want["greedy_hist"][:8]) and d["q_sa_max"] == want["q_sa_max"]
    assert abs(d["q_sa_mean"] - want["q_sa_sum"] / 96) <= REL * want["q_sa_sum_abs"] / 96
    assert d["huber_linear_frac"] == want["huber_linear_rows"] / 96 and d["done_frac"] == want["done_rows"] / 96
    names = [n for n, _, _ in eng.param_layout]
    assert list(d["grad_norm_last"]) == names == list(d["param_norm_last"])
    for n, g in zip(names, want["grad_sq_last"]):
        assert abs(d["grad_norm_last"][n] - math.sqrt(g)) <= REL * math.sqrt(g), n
    assert not any(block_bytes(eng)), "reset=True leaves zeros"
    assert eng.learn_stats()["steps"] == 0
    # the next step's extrema are that step's alone
    eng.learn_step(soft_update=True, stats=True)
    check_block(raw_block(eng), accumulate([step_reference(eng)]), "after reset")
    # a step without the flag leaves the block alone
    before = block_bytes(eng)
    eng.learn_step(soft_update=True)
    assert block_bytes(eng) == before
    # engine reset and a state load zero it; the stream-ordered reset call too
    blob = eng.state_blob().copy()
    eng.learn_step(stats=True)
    eng.load_state_blob(blob)
    assert not any(block_bytes(eng))
    eng.learn_step(stats=True)
    assert raw_block(eng).steps == 1
    eng.learn_stats_reset()
    assert not any(block_bytes(eng))
    eng.learn_step(stats=True)
    eng.reset()
    assert not any(block_bytes(eng))


# ---- kernel table ---------------------------------------------------------------------------------
def kernel_table(eng, flags):
    n = C.I32()
    C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
    out = []
    for i in range(n.value):
        name, fl, by = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_double()
        C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, ctypes.byref(fl), ctypes.byref(by)), "kernel_info")
        out.append((name.value.decode(), fl.value, by.value))
    return out


@pytest.mark.parametrize("case,flag_sets,today", [
    ("mlp14", (0, C.STEP_SOFT_UPDATE, C.STEP_PREFETCH), ["sample_uniform", "mlp_fwd", "head_bwd", "dw_adam16"]),
    # (the micro-CNN plan draws nothing ahead in a statistics step, so PREFETCH is not compared there)
    ("head", (0, C.STEP_SOFT_UPDATE), ["sample_uniform", "conv_perm", "micro_fwd", "linear_fwd_l1", "linear_fwd_l1_reduce",
                                       "linear_fwd_l2", "head_td_loss", "linear_bwd_l2", "linear_bwd_l1", "micro_dx",
                                       "micro_dw", "adam_fused"]),
])
def test_gpu_learn_stats_kernel_table(case, flag_sets, today):
    eng = make(case)
    eng.learn_step()
    assert [k[0] for k in kernel_table(eng, 0)] == today
    for flags in flag_sets:
        off, on = kernel_table(eng, flags), kernel_table(eng, flags | C.STEP_STATS)
        assert len(on) == len(off) + 1
        assert on[:-1] == off
        name, flops, nbytes = on[-1]
        assert name == "learn_stats" and flops == 0 and nbytes >= 8 * eng.n_params
    # the timed step runs the launch under its own index
    on = kernel_table(eng, C.STEP_STATS)
    ev = (ctypes.c_void_p * 2)()
    C.check(eng.L.dqnx_events_create(2, ev), "events")
    C.check(eng.L.dqnx_learn_step_timed(eng.h, C.STEP_STATS, len(on) - 1, ev[0], ev[1], eng.stream()), "timed")
    ms = ctypes.c_float()
    C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
    eng.L.dqnx_events_destroy(2, ev)
    assert ms.value > 0 and raw_block(eng).steps == 1


# ---- refusals -------------------------------------------------------------------------------------
def test_gpu_learn_stats_refusals_leave_the_block_untouched():
    eng = make("mlp14")
    eng.learn_step(stats=True)
    before = block_bytes(eng)
    with pytest.raises(C.DqnxError) as ei:
        eng.learn_step(grads_only=True, stats=True)
    assert ei.value.code == C.DQNX_EUNSUPPORTED and "GRADS_ONLY" in str(ei.value)
    assert eng.L.dqnx_learn_step_bucket(eng.h, C.STEP_STATS, 0, eng.stream()) == C.DQNX_EUNSUPPORTED
    assert b"out of scope" in eng.L.dqnx_last_error()
    assert eng.L.dqnx_apply_grads(eng.h, C.STEP_STATS, eng.stream()) == C.DQNX_EUNSUPPORTED
    assert eng.L.dqnx_apply_grads_bucket(eng.h, C.STEP_STATS, 0, eng.stream()) == C.DQNX_EUNSUPPORTED
    assert block_bytes(eng) == before
    eng.learn_step(stats=True)   # and the engine goes on
    assert raw_block(eng).steps == 2

    dp = E.LearnEngine(E.mlp_spec(14, 8, "dueling"), "DuelingDoubleDQNAgent", 64, 200, world_size=2, rank=0)
    dp.push(*transitions(150, 14, 8, 103))
    with pytest.raises(C.DqnxError) as ei:
        dp.learn_step(stats=True)
    assert ei.value.code == C.DQNX_EUNSUPPORTED and "world_size" in str(ei.value)
    n = C.I32()
    assert dp.L.dqnx_learn_kernel_count(dp.h, C.STEP_STATS, ctypes.byref(n)) == C.DQNX_EUNSUPPORTED
    assert not any(block_bytes(dp))


# ---- the drop-in Agent ----------------------------------------------------------------------------
TODAY_TAGS = {"AvgRew", "AvgEpLen", "Episodes", "Loss", "LearnTransitionsPerSec"}
STATS_TAGS = {"QMean", "QMaxMean", "TargetMean", "TDAbsMean", "TDAbsMax", "HuberLinearFrac", "ActionGap",
              "GreedyActionEntropy", "GradNorm"}


def agent_window(tmp_path, algo, property_on=False):
    """3 learn() calls and the log() that closes their window -> (tags, q(s,a) of the window, losses)"""
    agent = getattr(Agents, algo)(**agent_kwargs(algo, 14, 32, 500, tmp_path, log_frequency=2))
    if property_on:
        agent.collect_learn_stats = True
    obs, act, rew, done, nobs = transitions(100, 14, 8, 1)
    for i in range(100):
        agent.store_transitions(obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1], None)
    seen = {}
    agent.summary_writer.add_scalar = lambda tag, v, global_step=None: seen.__setitem__(tag, v)
    qsa, losses = [], []
    for t in range(3):
        agent.step = t
        agent.learn()
        agent.update_target_network()
        agent.flush()
        qsa.append(agent.engine.td[1].cpu().numpy().astype(np.float64))
        losses.append(float(agent.engine.loss()))
        agent.log()
    return agent, seen, np.concatenate(qsa), losses


@pytest.mark.parametrize("algo,defer,how", [("DuelingDoubleDQNAgent", "0", "env"), ("DuelingDoubleDQNAgent", "1", "env"),
                                            ("DuelingDoubleDQNAgent", "0", "property"),
                                            ("PerDuelingDoubleDQNAgent", "0", "env")])
def test_gpu_agent_logs_learn_stats(tmp_path, monkeypatch, algo, defer, how):
    """DQNX_LEARN_STATS=1 (or agent.collect_learn_stats = True): the one-call learn path
    (dqnx_agent_learn_mt), the deferred path (DQNX_AGENT_DEFER=1) and the staged PER path all
    accumulate, and log() writes the window's scalars."""
    monkeypatch.setenv("DQNX_AGENT_DEFER", defer)
    if how == "env":
        monkeypatch.setenv("DQNX_LEARN_STATS", "1")
    else:
        monkeypatch.delenv("DQNX_LEARN_STATS", raising=False)
    agent, seen, qsa, losses = agent_window(tmp_path, algo, property_on=(how == "property"))
    per = algo.startswith("Per")
    names = [n for n, _, _ in agent.engine.param_layout]
    want = TODAY_TAGS | STATS_TAGS | {"GradNorm/" + n for n in names} | ({"ISWeightMean"} if per else set())
    assert set(seen) == want
    assert all(math.isfinite(float(v)) for v in seen.values())
    assert len(qsa) == 96   # three steps in the window
    assert abs(seen["QMean"] - qsa.mean()) <= REL * np.abs(qsa).sum() / len(qsa)
    assert abs(seen["Loss"] - sum(losses) / 3) <= REL * sum(abs(x) for x in losses) / 3 + 1e-12   # the window mean
    assert seen["GradNorm"] > 0 and 0 <= seen["GreedyActionEntropy"] <= math.log(8) + 1e-12
    assert agent.engine.learn_stats()["steps"] == 0   # log() read with reset


def test_gpu_agent_log_without_learn_stats_is_todays(tmp_path, monkeypatch):
    monkeypatch.delenv("DQNX_LEARN_STATS", raising=False)
    agent, seen, _, losses = agent_window(tmp_path, "DuelingDoubleDQNAgent")
    assert set(seen) == TODAY_TAGS
    assert seen["Loss"] == losses[-1]   # the last step's loss, as before
    assert not agent.collect_learn_stats and not any(block_bytes(agent.engine))
