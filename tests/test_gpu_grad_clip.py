"""GPU: global-norm gradient clipping on the device (dqnx_set_grad_clip, LearnEngine(grad_clip=),
Agent.set_grad_clip, DQNX_GRAD_CLIP).

The parity reference is the unchanged oracle with torch's own clipping between its two halves:
    rec = oracle.learn(shard=(0, B))        # the full-batch gradient, not applied
    torch.nn.utils.clip_grad_norm_(...)     # on CPU, on rec.grads
    oracle.apply_grads(clipped)             # under PER with rec.abs_td and rec.positions
    oracle.update_target_network()
Adam is nearly invariant to the gradient's scale: at lr 1e-4 a clipped step moves the weights by a few
1e-6 less than an unclipped one, under the 1e-5 bar.  So the assertions that tell a clipped step from an
unclipped one are those on the Adam moments m and v and on the reported norm and coefficient.

max_norm is the median of the oracle's own unclipped norms over the test's steps (checked on the oracle
alone: a step with coef < 1, a step with coef == 1, no norm within 0.1 % of max_norm)."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from oracle import ref as O
from parity import assert_grad_close
from refnets import agent_kwargs
import test_gpu_engine as GE
import test_gpu_hybrid as GH
import test_gpu_learn_stats as GS
import test_gpu_per as GP

pytestmark = pytest.mark.gpu

SEED, FILL, CAP, STEPS = 11, 400, 500, 4


# ---- the oracle's clipped step ------------------------------------------------------------------
def torch_clip(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_ on copies of `grads` -> (clipped grads, total_norm, coef as torch forms it)"""
    ps = []
    for g in grads.values():
        p = torch.zeros_like(g, requires_grad=True)
        p.grad = g.clone()
        ps.append(p)
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2)
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return type(grads)(zip(grads.keys(), [p.grad for p in ps])), float(total), float(coef)


def oracle_step(oracle, max_norm):
    """One R:train.py:99-101 unit with clipping between backward and optimizer.step -> (rec, norm, coef)"""
    rec = oracle.learn(shard=(0, oracle.batch_size))
    clipped, norm, coef = torch_clip(rec.grads, max_norm) if max_norm else (rec.grads, None, 1.0)
    if oracle.per:
        oracle.apply_grads(clipped, rec.abs_td, rec.positions)
    else:
        oracle.apply_grads(clipped)
    oracle.update_target_network()
    oracle.step += 1
    return rec, norm, coef


def make_pair(case):
    if case == "per284":
        return GP.make_per_pair(284, 64, CAP, FILL, SEED, graphs=False)
    if case == "head":
        return GH.make_hybrid_pair("DuelingDoubleDQNAgent", 32, CAP, FILL, SEED)
    algo = "DQNAgent" if case == "linear14" else "DuelingDoubleDQNAgent"
    return GE.make_pair(algo, 14, 32, CAP, FILL, SEED, graphs=False)


def drop(eng):
    del eng
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def median_norm(case):
    """The median of the oracle's unclipped global norms over STEPS steps, with the conditions that make
    it a max_norm worth testing, checked on the clipped oracle run alone.  Computed once per case."""
    oracle, eng = make_pair(case)
    drop(eng)
    norms = []
    for _ in range(STEPS):
        rec, _, _ = oracle_step(oracle, None)
        norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for g in rec.grads.values()))))
    max_norm = float(np.median(norms))
    oracle, eng = make_pair(case)
    drop(eng)
    seen = [oracle_step(oracle, max_norm)[1:] for _ in range(STEPS)]
    assert any(c < 1.0 for _, c in seen) and any(c == 1.0 for _, c in seen), seen
    assert all(abs(n - max_norm) > 1e-3 * max_norm for n, _ in seen), (seen, max_norm)
    return max_norm


CASE_OF = {"mlp14": "mlp14", "linear14": "linear14", "per284": "per284", "mlp14_slab": "mlp14",
           "mlp14_per_layer": "mlp14", "head": "head"}
ENV_OF = {"mlp14_slab": {"DQNX_DW_ADAM16": "0"}, "mlp14_per_layer": {"DQNX_BWD_PLAN": "0"}}


# ---- 1. parity with torch's clipping ----------------------------------------------------------------
@pytest.mark.parametrize("route", ["mlp14", "linear14", "per284", "mlp14_slab", "mlp14_per_layer", "head"])
def test_gpu_clipped_steps_match_torch_clipping(monkeypatch, route):
    """4 clipped steps with the soft update against the oracle + clip_grad_norm_, after every step."""
    case = CASE_OF[route]
    max_norm = median_norm(case)
    for k, v in ENV_OF.get(route, {}).items():
        monkeypatch.setenv(k, v)
    oracle, eng = make_pair(case)
    eng.set_grad_clip(max_norm)
    per = case == "per284"
    clipped, loose = 0, {}
    for step in range(STEPS):
        rec, norm, coef = oracle_step(oracle, max_norm)
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        idx = eng.batch_idx.cpu().numpy().astype(np.int64) + (CAP - 1 if per else 0)
        assert np.array_equal(idx, rec.positions), f"step {step}: sampled indices differ"
        info = eng.grad_clip_info()
        print(f"{route} step {step}: loss {eng.loss()} vs {rec.loss}; norm {info['last_norm']} vs {norm}; "
              f"coef {info['last_coef']} vs {coef}")
        assert abs(eng.loss() - rec.loss) <= 1e-5
        assert abs(info["last_norm"] - norm) <= 1e-5 * norm
        assert abs(info["last_coef"] - coef) <= 1e-5
        clipped += coef < 1.0
        assert info["steps"] == step + 1 and info["clipped_steps"] == clipped
        # DQNX_BUF_GRADS keeps the unscaled gradient
        g = eng.param_views(eng.grads[:-1])
        for k, ref in rec.grads.items():
            gk = g[k].cpu()
            if case == "head":
                np.testing.assert_allclose(gk.numpy(), ref.numpy(), atol=5e-6, rtol=1e-3, err_msg=k)
            else:
                assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
            loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
        worst = GE.compare_state(oracle, eng, loose=loose)   # weights 1e-5 (2 lr rule), m 1e-6, v 1e-7
        print(f"{route} step {step}: worst {worst}")
        if per:
            same = np.array_equal(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1).astype(np.float32))
            GP.assert_tree_equal(eng, oracle.replay.replay_buffer, exact=same)
        GE.sync_oracle(oracle, eng)
    assert 0 < clipped < STEPS
    assert np.array_equal(eng.get_rng(1 if per else 0), oracle.np_state if per else oracle.py_state)


# ---- engines without an oracle ------------------------------------------------------------------------
def engine(case, env=None, **over):
    """test_gpu_learn_stats' engines (seeded weights, replay and RNG streams); `env` routes the plan"""
    mp = pytest.MonkeyPatch()
    try:
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        return GS.make(case, **over)
    finally:
        mp.undo()


def snapshot(eng, per=None):
    """every result of the steps so far, as bytes"""
    torch.cuda.synchronize()
    eng.check_device_error()
    per = GS.is_per(eng) if per is None else per
    out = {"params": eng.params.cpu().numpy().tobytes(), "target": eng.target_params.cpu().numpy().tobytes(),
           "m": eng.adam_m.cpu().numpy().tobytes(), "v": eng.adam_v.cpu().numpy().tobytes(),
           "loss": np.float32(eng.loss()).tobytes(), "rng_py": eng.get_rng(0).tobytes(), "rng_np": eng.get_rng(1).tobytes()}
    if per:
        out["tree"] = eng.sumtree.cpu().numpy().tobytes()
        out["tree_idx"] = (int(eng.ctrl().per_max_idx), int(eng.ctrl().per_min_idx))
    return out


def assert_same(a, b, what=""):
    for k in a:
        assert a[k] == b[k], (what, k)


ROUTES = {   # name: (test_gpu_learn_stats case, routing environment, engine kwargs)
    "fused": ("mlp14", {}, {}),
    "slab": ("mlp14", {"DQNX_DW_ADAM16": "0"}, {}),
    "per_layer": ("mlp14", {"DQNX_BWD_PLAN": "0"}, {}),
    "bf16": ("mlp284_bf16", {}, {}),
    "mlp284": ("mlp284_bf16", {}, {"compute_dtype": "fp32"}),   # MLP-284, B = 64
    "head": ("head", {}, {}),
    "per": ("per_b64", {}, {}),
    "conv_ig": ("hybrid84", {}, {}),   # the (4,84,84) net: implicit-GEMM convs, side-stream pipeline
}


def route_engine(route, **over):
    case, env, kw = ROUTES[route]
    return engine(case, env, **{**kw, **over}), env


def run_steps(eng, env, n, **kw):
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for _ in range(n):
            eng.learn_step(soft_update=True, **kw)
    finally:
        mp.undo()


@functools.lru_cache(maxsize=None)
def engine_median_norm(route):
    """the median pre-clip norm of the route's first STEPS unclipped steps (max_norm = 1e30: coef == 1)"""
    eng, env = route_engine(route, grad_clip=1e30)
    norms = []
    for _ in range(STEPS):
        run_steps(eng, env, 1)
        norms.append(eng.grad_clip_info()["last_norm"])
    assert eng.grad_clip_info()["clipped_steps"] == 0
    return float(np.median(norms))


# ---- 2. the norm is the norm of what Adam consumed -----------------------------------------------------
@pytest.mark.parametrize("route", ["mlp284", "bf16", "fused", "head"])
def test_gpu_clip_norm_and_first_moment(route):
    probe, env = route_engine(route, grad_clip=1e30)
    run_steps(probe, env, 1)
    max_norm = 0.5 * probe.grad_clip_info()["last_norm"]
    eng, env = route_engine(route, grad_clip=max_norm)
    assert not eng.adam_m.any() and not eng.adam_v.any()
    run_steps(eng, env, 1)
    torch.cuda.synchronize()
    eng.check_device_error()
    info = eng.grad_clip_info()
    P = eng.n_params
    g = eng.grads.cpu().numpy()
    assert g.shape == (P + 1,) and g[P] == np.float32(eng.loss()) and g[P] != 0   # the loss slot
    norm = np.sqrt((g[:P].astype(np.float64) ** 2).sum())
    assert abs(info["last_norm"] - norm) <= 1e-6 * norm   # an fp64 sum stored as fp32
    with_loss = np.sqrt((g.astype(np.float64) ** 2).sum())
    assert with_loss > norm and abs(info["last_norm"] - norm) < abs(info["last_norm"] - with_loss)   # not part of it
    assert info["steps"] == 1 and info["clipped_steps"] == 1 and info["norm_max"] == info["norm_sum"]
    assert abs(info["norm_sum"] - norm) <= 1e-9 * norm
    coef = np.float32(info["last_coef"])
    assert coef == np.float32(max_norm) / (np.float32(info["last_norm"]) + np.float32(1e-6)) and 0.49 < coef < 0.51
    # m = lerp(0, g', 0.1) from zero moments: one multiply by the fp32 weight (1 - beta1)
    gp = g[:P] * coef
    want = np.float32(0.1) * gp
    m = eng.adam_m.cpu().numpy()
    assert np.all(np.abs(m - want) <= np.spacing(np.abs(want)))
    v = eng.adam_v.cpu().numpy()
    want_v = (np.float32(1.0 - 0.999) * gp) * gp
    assert np.all(np.abs(v - want_v) <= np.spacing(np.abs(want_v)))


# ---- 3. coef == 1 is bitwise the unclipped step ------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "slab", "bf16", "head", "per", "per_layer"])
def test_gpu_clip_coef_one_is_bitwise_unclipped(route):
    e0, env = route_engine(route)
    e1, _ = route_engine(route, grad_clip=1e30)
    assert e0.grad_clip == 0.0 and e1.grad_clip == 1e30
    run_steps(e0, env, STEPS)
    run_steps(e1, env, STEPS)
    assert_same(snapshot(e0), snapshot(e1), route)
    info = e1.grad_clip_info()
    assert info["steps"] == STEPS and info["clipped_steps"] == 0 and info["last_coef"] == 1.0
    assert e0.grad_clip_info()["steps"] == 0   # clipping off: the block is never written


# ---- 4. step forms agree bitwise with clipping on -----------------------------------------------------------
def clipped_reference(route, max_norm, **over):
    eng, env = route_engine(route, grad_clip=max_norm, **over)
    run_steps(eng, env, STEPS)
    snap = snapshot(eng)
    info = eng.grad_clip_info()
    assert 0 < info["clipped_steps"] < STEPS, info   # both kinds of step occur
    return snap, info


@pytest.mark.parametrize("route", ["fused", "slab", "head", "per"])
def test_gpu_clip_learn_steps_equal_single_steps(route):
    max_norm = engine_median_norm(route)
    ref, info = clipped_reference(route, max_norm)
    eng, env = route_engine(route, grad_clip=max_norm)
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        eng.learn_steps(STEPS, soft_update=True)
    finally:
        mp.undo()
    assert_same(ref, snapshot(eng), route)
    assert eng.grad_clip_info() == info
    eng.push(*O.synth_transitions(4, eng.spec.obs_dim, 8, seed=3))   # nothing is pending afterwards


@pytest.mark.parametrize("route", ["fused", "slab", "per_layer", "head", "bf16"])
def test_gpu_clip_prefetch_loop_equals_sequential_steps(route):
    """the in-launch draw (fused, head), no draw ahead (slab) and the side-stream pipeline (per-layer)"""
    max_norm = engine_median_norm(route)
    ref, info = clipped_reference(route, max_norm)
    eng, env = route_engine(route, grad_clip=max_norm)
    run_steps(eng, env, STEPS - 1, prefetch=True)
    run_steps(eng, env, 1)   # consumes the pending minibatch
    assert_same(ref, snapshot(eng), route)
    assert eng.grad_clip_info() == info


@pytest.mark.parametrize("route", ["fused", "slab", "per_layer", "bf16", "head", "per"])
def test_gpu_clip_grads_only_plus_apply_equals_the_step(route):
    max_norm = engine_median_norm(route)
    ref, info = clipped_reference(route, max_norm)
    eng, env = route_engine(route, grad_clip=max_norm)
    mp = pytest.MonkeyPatch()
    try:
        for k, v in env.items():
            mp.setenv(k, v)
        for i in range(STEPS):
            eng.learn_step(grads_only=True)
            assert eng.grad_clip_info()["steps"] == i   # the gradient-only half does not clip
            eng.apply_grads(soft_update=True)
    finally:
        mp.undo()
    assert_same(ref, snapshot(eng), route)
    assert eng.grad_clip_info() == info


@pytest.mark.parametrize("route", ["fused", "slab", "head", "per"])
def test_gpu_clip_graphs_on_equals_off(route):
    max_norm = engine_median_norm(route)
    ref, info = clipped_reference(route, max_norm)
    eng, env = route_engine(route, grad_clip=max_norm, graphs=True)
    run_steps(eng, env, STEPS)
    assert_same(ref, snapshot(eng), route)
    assert eng.grad_clip_info() == info
    # a new max_norm reaches the replayed graphs: the cached plans are dropped
    eng.set_grad_clip(1e30)
    run_steps(eng, env, 1)
    assert eng.grad_clip_info()["last_coef"] == 1.0


# ---- 5. the statistics are independent ---------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "slab", "per_layer", "head", "per"])
def test_gpu_clip_with_stats(route):
    max_norm = engine_median_norm(route)
    ref, info = clipped_reference(route, max_norm)
    eng, env = route_engine(route, grad_clip=max_norm)
    for step in range(STEPS):
        run_steps(eng, env, 1, stats=True)
        st = eng.learn_stats()
        ci = eng.grad_clip_info()
        norm = float(np.sqrt(st["grad_sq_last"].sum()))
        assert abs(norm - ci["last_norm"]) <= 1e-6 * norm   # both report the pre-clip norm
        assert st["steps"] == ci["steps"] == step + 1
    assert abs(st["grad_norm_sum"] - ci["norm_sum"]) <= 1e-9 * ci["norm_sum"]
    assert_same(ref, snapshot(eng), route)
    assert eng.grad_clip_info() == info


@pytest.mark.parametrize("route,steps", [("per_layer", 12), ("conv_ig", 6), ("fused", 12), ("head", 12)])
def test_gpu_clip_stats_in_a_prefetching_loop(route, steps):
    """stats=True and prefetch=True together, clipping on, with no host wait between the steps: the
    statistics launch ends the clipped tail, behind the point where the gradient-only half is done with
    the minibatch, and on the side-stream pipeline (per-layer plan, implicit-GEMM convs) a later draw
    reuses the step's (idx, phys) pair.  The statistics block, the clip block and every result equal
    those of sequential steps, byte for byte."""
    max_norm = engine_median_norm(route)
    seq, env = route_engine(route, grad_clip=max_norm)
    run_steps(seq, env, steps, stats=True)
    eng, _ = route_engine(route, grad_clip=max_norm)
    run_steps(eng, env, steps - 1, stats=True, prefetch=True)
    run_steps(eng, env, 1, stats=True)   # consumes the pending minibatch
    assert_same(snapshot(seq), snapshot(eng), route)
    assert GS.block_bytes(seq) == GS.block_bytes(eng)
    assert GS.raw_block(eng).steps == steps
    assert eng.grad_clip_info() == seq.grad_clip_info()


# ---- 6. the drop-in Agent -----------------------------------------------------------------------------------
@pytest.mark.parametrize("how,defer", [("env", "0"), ("method", "0"), ("env", "1")])
def test_gpu_agent_clipped_loop_matches_oracle(tmp_path, monkeypatch, how, defer):
    algo, obs_dim, batch, seed, steps = "DuelingDoubleDQNAgent", 14, 32, SEED, 3
    max_norm = median_norm("mlp14")
    monkeypatch.setenv("DQNX_AGENT_DEFER", defer)
    if how == "env":
        monkeypatch.setenv("DQNX_GRAD_CLIP", repr(max_norm))
    else:
        monkeypatch.delenv("DQNX_GRAD_CLIP", raising=False)
    torch.manual_seed(seed)
    agent = getattr(Agents, algo)(**agent_kwargs(algo, obs_dim, batch, CAP, tmp_path, log_frequency=3))
    if how == "method":
        assert agent.engine.grad_clip == 0.0
        agent.set_grad_clip(max_norm)
    assert agent.engine.grad_clip == max_norm
    spec = O.mlp_spec(obs_dim, 8, "dueling")
    init = O.reference_init(spec, seed)
    oracle = O.OracleLearner(spec, algo, batch, CAP, seed=seed, params=init)
    obs, act, rew, done, nobs = O.synth_transitions(FILL, obs_dim, 8, seed=seed + 100)
    for i in range(FILL):
        rows = (obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1])
        agent.store_transitions(*rows, None)
        oracle.store_transitions(*rows)
    seen = {}
    agent.summary_writer.add_scalar = lambda tag, v, global_step=None: seen.__setitem__(tag, v)
    random.seed(seed + 7)
    norms, clipped = [], 0
    for t in range(steps):
        agent.step = t + 1
        oracle.py_state = O.py_state_to_array()
        agent.learn()
        agent.update_target_network()
        rec, norm, coef = oracle_step(oracle, max_norm)
        # learn() leaves the global generator where the reference's draw leaves it
        assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.uint32), oracle.py_state)
        agent.flush()
        assert abs(agent.engine.loss() - rec.loss) <= 1e-5
        norms.append(norm)
        clipped += coef < 1.0
        GE.compare_state(oracle, agent.engine)   # m within 1e-6, v within 1e-7, weights within 1e-5
        GE.sync_oracle(oracle, agent.engine)
    info = agent.engine.grad_clip_info()
    assert info["steps"] == steps and info["clipped_steps"] == clipped and 0 < clipped < steps
    agent.log()   # step 3 closes the window
    assert {"GradNorm", "GradClipFrac"} <= set(seen) and "QMean" not in seen
    assert abs(seen["GradNorm"] - np.mean(norms)) <= 1e-5 * np.mean(norms)
    assert seen["GradClipFrac"] == clipped / steps
    assert agent.engine.grad_clip_info()["steps"] == 0   # log() read with reset


def test_gpu_agent_log_without_clipping_is_todays(tmp_path, monkeypatch):
    monkeypatch.delenv("DQNX_GRAD_CLIP", raising=False)
    monkeypatch.delenv("DQNX_LEARN_STATS", raising=False)
    agent, seen, _, _ = GS.agent_window(tmp_path, "DuelingDoubleDQNAgent")
    assert set(seen) == GS.TODAY_TAGS and agent.engine.grad_clip == 0.0
    assert agent.engine.grad_clip_info()["steps"] == 0


def test_gpu_clip_state_blob_carries_no_clipping():
    """max_norm is configuration and the info block a log window's: a blob saved with clipping on loads
    into an engine with clipping off, which continues unclipped (and the other way round)."""
    max_norm = engine_median_norm("fused")
    a, env = route_engine("fused", grad_clip=max_norm)
    run_steps(a, env, 2)
    blob = a.state_blob()
    b, _ = route_engine("fused")
    c, _ = route_engine("fused", grad_clip=max_norm)
    run_steps(c, env, 1)
    for e in (b, c):
        e.load_state_blob(blob)
        assert e.grad_clip_info()["steps"] == 0   # zeroed by the load, never in the blob
    assert b.grad_clip == 0.0 and c.grad_clip == max_norm
    # the unclipped continuation equals an engine that was never clipped, started from the same state
    d, _ = route_engine("fused")
    d.load_state_blob(blob)
    for e in (a, b, c, d):
        run_steps(e, env, 2)
    assert_same(snapshot(a), snapshot(c), "clipped continuation")
    assert_same(snapshot(b), snapshot(d), "unclipped continuation")
    assert snapshot(a)["m"] != snapshot(b)["m"]
    assert b.grad_clip_info()["steps"] == 0 and c.grad_clip_info()["steps"] == 2


# ---- 7. refusals and bookkeeping ------------------------------------------------------------------------------
def test_gpu_clip_refusals_and_bookkeeping():
    eng, env = route_engine("fused", grad_clip=1.0)
    L, h = eng.L, eng.h
    # a draw is pending: the setting may not change under it, and the block is not read
    eng.learn_step(soft_update=True, prefetch=True)
    assert L.dqnx_set_grad_clip(h, ctypes.c_double(2.0)) == C.DQNX_ESTATE
    assert b"prefetched" in L.dqnx_last_error()
    assert L.dqnx_grad_clip_info_get(h, ctypes.byref(C.GradClipInfo()), 0, eng.stream()) == C.DQNX_ESTATE
    eng.learn_step(soft_update=True)   # consumes it
    eng.set_grad_clip(2.0)
    assert eng.grad_clip == 2.0
    # both bucket entry points, and the engine goes on
    for call in (lambda: eng.learn_step_bucket(0), lambda: eng.apply_grads_bucket(0)):
        with pytest.raises(C.DqnxError) as ei:
            call()
        assert ei.value.code == C.DQNX_EUNSUPPORTED and "gradient clipping" in str(ei.value)
    eng.learn_step(soft_update=True)
    info = eng.grad_clip_info(reset=True)
    assert info["steps"] == 3 and info["norm_max"] >= info["norm_sum"] / 3 > 0
    zero = {"steps": 0, "clipped_steps": 0, "norm_sum": 0.0, "norm_max": 0.0, "last_norm": 0.0, "last_coef": 0.0,
            "norm_mean": 0.0, "clipped_frac": 0.0}
    assert eng.grad_clip_info() == zero   # info(reset=True) zeroed the block
    eng.push(*O.synth_transitions(4, 14, 8, seed=3))
    eng.learn_step()
    assert eng.grad_clip_info()["steps"] == 1
    eng.reset()   # dqnx_engine_reset zeroes it too; max_norm stays (configuration)
    assert eng.grad_clip_info() == zero and eng.grad_clip == 2.0
    # with clipping turned off again the bucketed step runs as before
    e2, _ = route_engine("fused", grad_clip=1.0)
    e2.set_grad_clip(None)
    assert e2.grad_clip == 0.0
    for b in range(len(e2.dp_buckets())):
        e2.learn_step_bucket(b)
        e2.apply_grads_bucket(b)
    torch.cuda.synchronize()
    e2.check_device_error()
    assert e2.grad_clip_info() == zero


def test_gpu_clip_timed_step_runs_the_listed_launches():
    """dqnx_learn_kernel_info / dqnx_learn_step_timed with clipping on: the listed launches are the step"""
    max_norm = engine_median_norm("fused")
    ref, _ = route_engine("fused", grad_clip=max_norm)
    run_steps(ref, {}, 1)
    eng, _ = route_engine("fused", grad_clip=max_norm)
    n = C.I32()
    C.check(eng.L.dqnx_learn_kernel_count(eng.h, C.STEP_SOFT_UPDATE, ctypes.byref(n)), "count")
    names = []
    for i in range(n.value):
        name = ctypes.create_string_buffer(64)
        C.check(eng.L.dqnx_learn_kernel_info(eng.h, C.STEP_SOFT_UPDATE, i, name, 64, None, None), "info")
        names.append(name.value.decode())
    assert names[-3:] == ["grad_sumsq", "clip_coef", "adam_clipped"]
    ev = (ctypes.c_void_p * 2)()
    C.check(eng.L.dqnx_events_create(2, ev), "events")
    C.check(eng.L.dqnx_learn_step_timed(eng.h, C.STEP_SOFT_UPDATE, n.value - 3, ev[0], ev[1], eng.stream()), "timed")
    ms = ctypes.c_float()
    C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
    eng.L.dqnx_events_destroy(2, ev)
    assert 0 < ms.value < 50
    assert_same(snapshot(ref), snapshot(eng), "timed step")
    assert eng.grad_clip_info() == ref.grad_clip_info()
