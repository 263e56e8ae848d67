"""GPU: n-step returns (include/dqnx.h "n-step returns"; LearnEngine(n_step=), DQNX_N_STEP).

Three references, none of them the code under test:
  * an n_step = 1 engine forced through the gather (DQNX_NSTEP_FORCE=1) must be bitwise the default engine;
  * the unchanged oracle, its replay's sample_transitions wrapped to hand back the rows the numpy loop of
    tests/nstep_ref.py aggregates and its gamma set to the [B, 1] fp32 tensor of the rows' discounts, so
    `(1 - dones_t) * gamma * sel` is the same arithmetic: indices ==, Q / targets / loss 1e-5, weights and
    moments with the bars of test_gpu_engine (parity.assert_grad_close, compare_state);
  * the materialised minibatch itself against the numpy loop and the ring, with ==.
Rings carry a done rate of 1/6; every parity case asserts, on the oracle side alone, which kinds of window
its steps met.  n_env = 3 pushes whole time steps: 399 rows where one environment pushes 400 (249 for
250 into the wrapping ring)."""
import contextlib
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from oracle import ref as O
from parity import assert_grad_close
from refnets import agent_kwargs
import conv_geoms as G
import nstep_ref as NR
import test_gpu_engine as GE
import test_gpu_grad_clip as GC
import test_gpu_per as GP

pytestmark = pytest.mark.gpu

SEED, CAP, FILL, STEPS, GAMMA = 11, 500, 400, 4, 0.99
DDQN, PER = "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"
IG = G.BY_NAME[G.IMPLICIT[0]]   # the smallest implicit-GEMM row of tests/conv_geoms.py


# ---- nets, data, engines ---------------------------------------------------------------------------------
def specs(net):
    """(engine spec, oracle spec, batch, (capacity, fill))"""
    if net == "mlp14":
        return E.mlp_spec(14, 8, "dueling"), O.mlp_spec(14, 8, "dueling"), 32, (CAP, FILL)
    if net == "mlp284":
        return E.mlp_spec(284, 8, "dueling"), O.mlp_spec(284, 8, "dueling"), 64, (CAP, FILL)
    if net == "head":
        return E.hybrid_spec(8, "dueling"), O.hybrid_spec(8, "dueling"), 32, (CAP, FILL)
    assert net == "ig"
    return G.engine_spec(E, IG, "dueling"), G.oracle_spec(O, IG, "dueling"), G.base_batch(IG), G.replay_sizes(IG)


ROUTES = {   # name: (net, algorithm, routing environment, engine kwargs)
    "fused": ("mlp14", DDQN, {}, {}),
    "slab": ("mlp14", DDQN, {"DQNX_DW_ADAM16": "0"}, {}),
    "per_layer": ("mlp14", DDQN, {"DQNX_BWD_PLAN": "0"}, {}),
    "mlp284": ("mlp284", DDQN, {}, {}),
    "bf16": ("mlp284", DDQN, {}, {"compute_dtype": "bf16"}),
    "per": ("mlp284", PER, {}, {}),
    "head": ("head", DDQN, {}, {}),                            # the micro-CNN plan
    "im2col": ("head", DDQN, {"DQNX_MICRO_CNN": "0"}, {}),     # the explicit conv route
    "conv_ig": ("ig", DDQN, {}, {}),                           # implicit-GEMM convs, side-stream pipeline
}


@functools.lru_cache(maxsize=None)
def transitions(count, obs_dim, macro_len, seed):
    """the synthetic env's rows with a done rate of 1/6"""
    obs, act, rew, _, nobs = O.synth_transitions(count, obs_dim, 8, seed=seed, macro_len=macro_len)
    done = np.random.default_rng(seed + 1).random(count) < 1.0 / 6.0
    assert 0.12 < done.mean() < 0.22
    return obs, act, rew, done, nobs


@contextlib.contextmanager
def routed(env, force=False):
    mp = pytest.MonkeyPatch()
    try:
        mp.delenv("DQNX_NSTEP_FORCE", raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        if force:
            mp.setenv("DQNX_NSTEP_FORCE", "1")
        yield
    finally:
        mp.undo()


def push_steps(eng, data, n_env, lo=0, hi=None):
    """whole time steps of n_env rows, in one call (the ring takes any multiple of n_env)"""
    hi = len(data[1]) if hi is None else hi
    hi -= (hi - lo) % n_env
    eng.push(*(x[lo:hi] for x in data))
    return hi


def make_engine(route, n_step=1, n_env=1, force=False, sizes=None, seed=SEED, **over):
    net, algo, env, kw = ROUTES[route]
    spec, ospec, batch, (cap, fill) = specs(net)
    cap, fill = sizes or (cap, fill)
    with routed(env, force):
        eng = E.LearnEngine(spec, algo, batch, cap, n_env=n_env, n_step=n_step, **{**kw, **over})
    eng.load_params(O.reference_init(ospec, seed))
    push_steps(eng, transitions(fill, spec.obs_dim, ospec.macro_len or 14, seed + 100), n_env)
    random.seed(seed + 7)
    np.random.seed(seed + 11)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    eng.set_rng(C.DQNX_RNG_NP, O.np_state_to_array())
    eng.route_env = env
    return eng


def run(eng, n, **kw):
    with routed(eng.route_env):
        for _ in range(n):
            eng.learn_step(soft_update=True, **kw)


def kernel_names(eng, flags=C.STEP_SOFT_UPDATE):
    n = C.I32()
    with routed(eng.route_env):
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "count")
        out = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(64)
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, None, None), "info")
            out.append(name.value.decode())
    return out


# ---- 1. the forced route is bitwise the default ---------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "slab", "per_layer", "bf16", "per", "head", "im2col", "conv_ig"])
def test_gpu_forced_gather_is_bitwise_the_default(route):
    plain = make_engine(route)
    forced = make_engine(route, force=True)
    names = kernel_names(forced)
    assert names.count("nstep_gather") == 1 and [n for n in names if n != "nstep_gather"] == kernel_names(plain)
    assert plain.nstep_views() is None and forced.nstep_views() is not None
    run(plain, STEPS)
    run(forced, STEPS)
    GC.assert_same(GC.snapshot(plain), GC.snapshot(forced), route)
    for a, b in ((plain.q, forced.q), (plain.td, forced.td), (plain.grads, forced.grads)):
        assert torch.equal(a, b)
    mb = forced.nstep_views()
    assert torch.all(mb["mb_disc"] == np.float32(GAMMA))   # n = 1: the discount the default engine multiplies by


# ---- 2. parity with the oracle -----------------------------------------------------------------------------------
def wrap_oracle(oracle, n, n_env, seen, forced):
    """The oracle's replay hands back n-step rows: the numpy loop over its own stored transitions, in
    logical order.  `seen` collects the kind of every window; `forced` (a one-element list) holds the
    positions of a given-indices step, which draws nothing."""
    rep, gamma0, cap = oracle.replay, oracle.gamma, oracle.buffer_size
    orig = rep.sample_transitions

    def logical_rows():
        if not oracle.per:
            return list(rep.replay_buffer)
        t = rep.replay_buffer
        base = (t.data_pointer - t.size) % cap
        return [t.data[(base + i) % cap] for i in range(t.size)]

    def aggregate(ps):
        rows = logical_rows()
        size = len(rows)
        rew = np.asarray([r[2] for r in rows], np.float32)
        done = np.asarray([float(r[3]) for r in rows], np.float32)
        out, disc = [], []
        for p in ps:
            R, d, g, last, m = NR.window(rew, done, size, p, n, n_env, gamma0)
            seen.add(NR.kind(rew, done, size, p, n, n_env))
            out.append((rows[p][0], rows[p][1], R, d, rows[last][4]))
            disc.append(g)
        oracle.gamma = torch.tensor(np.asarray(disc, np.float32)).view(-1, 1)
        oracle.last_windows = (np.asarray(ps), out, np.asarray(disc, np.float32))
        return out

    if oracle.per:
        def sample(step, np_state):
            is_w, leaves, _ = orig(step, np_state)
            t = rep.replay_buffer
            base = (t.data_pointer - t.size) % cap
            return is_w, leaves, aggregate([((leaf - (cap - 1)) - base) % cap for leaf in leaves])
    else:
        def sample(mt_state):
            if forced[0] is not None:
                pos, forced[0] = forced[0], None
                return aggregate([int(p) for p in pos]), pos
            _, pos = orig(mt_state)
            return aggregate([int(p) for p in pos]), pos
    rep.sample_transitions = sample


def make_pair(route, n, n_env, sizes=None, pushes=None, seed=SEED):
    net, algo, env, kw = ROUTES[route]
    spec, ospec, batch, (cap, fill) = specs(net)
    cap, fill = sizes or (cap, fill)
    pushes = pushes or fill
    init = O.reference_init(ospec, seed)
    oracle = O.OracleLearner(ospec, algo, batch, cap, seed=seed, params=init, per_pow="cr", n_env=n_env, gamma=GAMMA)
    with routed(env):
        eng = E.LearnEngine(spec, algo, batch, cap, n_env=n_env, n_step=n, gamma=GAMMA, **kw)
    eng.load_params(init)
    data = transitions(pushes, spec.obs_dim, ospec.macro_len or 14, seed + 100)
    hi = push_steps(eng, data, n_env)
    for i in range(0, hi, n_env):
        oracle.store_transitions(data[0][i:i + n_env], [int(a) for a in data[1][i:i + n_env]],
                                 [float(r) for r in data[2][i:i + n_env]], [bool(d) for d in data[3][i:i + n_env]],
                                 data[4][i:i + n_env])
    random.seed(seed + 7)
    np.random.seed(seed + 11)
    oracle.py_state, oracle.np_state = O.py_state_to_array(), O.np_state_to_array()
    eng.set_rng(C.DQNX_RNG_PY, oracle.py_state.copy())
    eng.set_rng(C.DQNX_RNG_NP, oracle.np_state.copy())
    eng.route_env = env
    seen, forced = set(), [None]
    wrap_oracle(oracle, n, n_env, seen, forced)
    return oracle, eng, seen, forced


def check_step(oracle, eng, rec, step, loose, head):
    """one step's results against the oracle's record, then the oracle continues from the engine's state"""
    torch.cuda.synchronize()
    eng.check_device_error()
    per, cap = oracle.per, eng.capacity
    idx = eng.batch_idx.cpu().numpy().astype(np.int64) + (cap - 1 if per else 0)
    assert np.array_equal(idx, rec.positions), f"step {step}: sampled indices differ"
    q = eng.q.cpu()
    np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(q[2].numpy(), rec.q_target_next.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(q[1].numpy(), rec.q_online_next.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.td[0].cpu().numpy(), rec.targets.view(-1).numpy(), atol=1e-5, rtol=0)
    assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss)), (step, eng.loss(), rec.loss)
    g = eng.param_views(eng.grads[:-1])
    for k, ref in rec.grads.items():
        gk = g[k].cpu()
        assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
        loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
    # ELU nets have no mask to flip: no entry is exempted there (test_gpu_conv_geoms)
    GE.compare_state(oracle, eng, loose=None if head else loose)
    if per:
        # the trees are equal bit for bit as long as every |delta| written into them agreed in fp32 (two
        # devices: ~1e-6 apart now and then); a leaf one ulp apart stays so until it is sampled again
        same = np.array_equal(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1).astype(np.float32))
        oracle.tree_exact = getattr(oracle, "tree_exact", True) and same
        GP.assert_tree_equal(eng, oracle.replay.replay_buffer, exact=oracle.tree_exact)
    # the minibatch the step trained on is the oracle's
    ps, rows, disc = oracle.last_windows
    mb = eng.nstep_views()
    assert np.array_equal(mb["mb_rew"].cpu().numpy(), np.asarray([r[2] for r in rows], np.float32))
    assert np.array_equal(mb["mb_done"].cpu().numpy(), np.asarray([r[3] for r in rows], np.float32))
    assert np.array_equal(mb["mb_disc"].cpu().numpy(), disc)
    GE.sync_oracle(oracle, eng)


def given_positions(eng, n, n_env, rng, extra=()):
    """a minibatch that contains the newest (n - 1) * n_env positions and `extra`, the rest drawn without repeats"""
    size, B = eng.ring_size, eng.batch
    must = list(dict.fromkeys(list(range(size - (n - 1) * n_env, size)) + [int(p) for p in extra]))
    rest = [int(p) for p in rng.permutation(size) if int(p) not in set(must)]
    pos = np.asarray(must + rest[:B - len(must)], np.int64)
    assert len(pos) == B
    rng.shuffle(pos)
    return pos


PARITY = [(r, n, e) for r in ("fused", "per", "head") for n, e in ((3, 1), (5, 3), (3, 3), (5, 1))]


@pytest.mark.parametrize("route,n,n_env", PARITY)
def test_gpu_nstep_steps_match_oracle(route, n, n_env):
    oracle, eng, seen, forced = make_pair(route, n, n_env)
    assert kernel_names(eng).count("nstep_gather") == 1
    loose, head = {}, route == "head"
    for step in range(STEPS):
        oracle.step = step
        rec = oracle.train_step()
        run(eng, 1)
        check_step(oracle, eng, rec, step, loose, head)
    assert np.array_equal(eng.get_rng(1 if oracle.per else 0), oracle.np_state if oracle.per else oracle.py_state)
    want = {("full",)} | {("done", j) for j in range(n)}
    if not oracle.per:   # one more step on given indices: the windows the newest end of the ring cuts
        pos = given_positions(eng, n, n_env, np.random.default_rng(SEED))
        forced[0] = pos
        eng.batch_idx.copy_(torch.from_numpy(pos.astype(np.int32)))
        rec = oracle.train_step()
        run(eng, 1, given_indices=True)
        check_step(oracle, eng, rec, STEPS, loose, head)
        want |= {("end", m) for m in range(1, n)}
    assert want <= seen, sorted(want - seen)   # (on the oracle side alone)


@pytest.mark.parametrize("route,n,n_env", [("fused", 3, 1), ("fused", 5, 3), ("per", 3, 3), ("head", 5, 1)])
def test_gpu_nstep_wrapped_ring_matches_oracle(route, n, n_env):
    """capacity 100 with 250 rows pushed (249 for n_env = 3, and 100 is no multiple of 3): logical position
    0 is a slot in the middle of the ring, and windows cross the physical end of the arrays"""
    oracle, eng, seen, forced = make_pair(route, n, n_env, sizes=(100, 100), pushes=250)
    assert eng.ring_size == 100 and eng.ring_wptr == (250 - 250 % n_env) % 100 != 0
    loose, head = {}, route == "head"
    for step in range(STEPS):
        oracle.step = step
        rec = oracle.train_step()
        run(eng, 1)
        check_step(oracle, eng, rec, step, loose, head)
    base = (eng.ring_wptr - eng.ring_size) % 100
    want = {("full",)} | {("done", j) for j in range(n)}
    if not oracle.per:
        # the newest positions, and the start rows in the last slots of the arrays: their windows go on at slot 0
        cross = [(99 - base - j) % 100 for j in range((n - 1) * n_env)]
        pos = given_positions(eng, n, n_env, np.random.default_rng(SEED + 1), extra=cross)
        forced[0] = pos
        eng.batch_idx.copy_(torch.from_numpy(pos.astype(np.int32)))
        rec = oracle.train_step()
        run(eng, 1, given_indices=True)
        check_step(oracle, eng, rec, STEPS, loose, head)
        want |= {("end", m) for m in range(1, n)}
    assert want <= seen, sorted(want - seen)


# ---- 3. the materialised minibatch itself ---------------------------------------------------------------------
@pytest.mark.parametrize("route,n,n_env,sizes,pushes", [
    ("fused", 3, 1, None, None), ("mlp284", 5, 3, None, None), ("bf16", 3, 3, None, None), ("per", 16, 1, None, None),
    ("head", 5, 3, (100, 100), 250), ("per_layer", 2, 1, (100, 100), 250), ("conv_ig", 3, 1, None, None)])
def test_gpu_materialised_minibatch_equals_numpy_loop(route, n, n_env, sizes, pushes):
    eng = make_engine(route, n_step=n, n_env=n_env, sizes=sizes and (sizes[0], pushes))
    run(eng, 1)
    torch.cuda.synchronize()
    eng.check_device_error()
    cap, size, per = eng.capacity, eng.ring_size, GC.GS.is_per(eng)
    base = (eng.ring_wptr - size) % cap
    idx = eng.batch_idx.cpu().numpy().astype(np.int64)
    ps = (idx - base) % cap if per else idx          # PER stores ring slots, uniform replay logical positions
    slot = lambda p: (base + p) % cap                # noqa: E731
    rew = eng.ring_rew.cpu().numpy()[slot(np.arange(size))]
    done = eng.ring_done.cpu().numpy()[slot(np.arange(size))]
    R, d, disc, last, m = NR.windows(rew, done, size, ps, n, n_env, GAMMA)
    mb = {k: v.cpu() for k, v in eng.nstep_views().items()}
    assert np.array_equal(mb["mb_rew"].numpy(), R) and np.array_equal(mb["mb_done"].numpy(), d)
    assert np.array_equal(mb["mb_disc"].numpy(), disc)
    assert np.array_equal(mb["mb_act"].numpy(), eng.ring_act.cpu().numpy()[slot(ps)])
    assert np.array_equal(mb["mb_phys"].numpy(), np.arange(eng.batch_local))
    assert torch.equal(mb["mb_obs"], eng.ring_obs.cpu()[slot(ps)])
    assert torch.equal(mb["mb_next"], eng.ring_next_obs.cpu()[slot(last)])
    start = mb["mb_start"].numpy()
    assert np.array_equal(start[:, 0].view(np.int32), mb["mb_act"].numpy())
    assert np.array_equal(start[:, 1], rew[ps]) and np.array_equal(start[:, 2], done[ps]) and not start[:, 3].any()
    if "mb_obs16" in mb:   # the bf16 copies are the rows rounded as the push rounds them
        D = eng.spec.obs_dim
        assert torch.equal(mb["mb_obs16"][:, :D], mb["mb_obs"][:, :D].to(torch.bfloat16))
        assert torch.equal(mb["mb_next16"][:, :D], mb["mb_next"][:, :D].to(torch.bfloat16))
    assert m.max() > 1 or n == 1


# ---- 4. compositions: bitwise the sequential n-step steps ------------------------------------------------------
COMPOSE = [("fused", 3, 1), ("slab", 3, 3), ("per_layer", 5, 1), ("bf16", 3, 1), ("per", 3, 3), ("head", 5, 3),
           ("im2col", 3, 1), ("conv_ig", 3, 1)]


@functools.lru_cache(maxsize=None)
def sequential(route, n, n_env):
    eng = make_engine(route, n_step=n, n_env=n_env)
    run(eng, STEPS)
    return GC.snapshot(eng)


@pytest.mark.parametrize("route,n,n_env", COMPOSE)
def test_gpu_nstep_prefetch_loop_equals_sequential_steps(route, n, n_env):
    eng = make_engine(route, n_step=n, n_env=n_env)
    run(eng, STEPS - 1, prefetch=True)
    run(eng, 1)   # consumes the pending minibatch
    GC.assert_same(sequential(route, n, n_env), GC.snapshot(eng), route)


@pytest.mark.parametrize("route,n,n_env", COMPOSE)
def test_gpu_nstep_learn_steps_equal_single_steps(route, n, n_env):
    eng = make_engine(route, n_step=n, n_env=n_env)
    with routed(eng.route_env):
        eng.learn_steps(STEPS, soft_update=True)
    GC.assert_same(sequential(route, n, n_env), GC.snapshot(eng), route)


@pytest.mark.parametrize("route,n,n_env", [c for c in COMPOSE if c[0] != "conv_ig"])
def test_gpu_nstep_graphs_on_equals_off(route, n, n_env):
    eng = make_engine(route, n_step=n, n_env=n_env, graphs=True)
    run(eng, STEPS)
    GC.assert_same(sequential(route, n, n_env), GC.snapshot(eng), route)


@pytest.mark.parametrize("route,n,n_env", COMPOSE)
def test_gpu_nstep_grads_only_plus_apply_equals_the_step(route, n, n_env):
    eng = make_engine(route, n_step=n, n_env=n_env)
    with routed(eng.route_env):
        for _ in range(STEPS):
            eng.learn_step(grads_only=True)
            eng.apply_grads(soft_update=True)
    GC.assert_same(sequential(route, n, n_env), GC.snapshot(eng), route)


@pytest.mark.parametrize("route,n,n_env", COMPOSE)
def test_gpu_nstep_with_stats_changes_nothing_else(route, n, n_env):
    """and the statistics describe the sampled START rows (reward, done, action) and the n-step target"""
    eng = make_engine(route, n_step=n, n_env=n_env)
    rew_sum, done_rows, taken = 0.0, 0, np.zeros(C.STATS_MAX_ACTIONS, np.int64)
    tgt_sum = 0.0
    for _ in range(STEPS):
        run(eng, 1, stats=True)
        torch.cuda.synchronize()
        start = eng.nstep_views()["mb_start"].cpu().numpy()
        rew_sum += float(start[:, 1].astype(np.float64).sum())
        done_rows += int((start[:, 2] != 0).sum())
        taken += np.bincount(start[:, 0].view(np.int32), minlength=C.STATS_MAX_ACTIONS)
        tgt_sum += float(eng.td[0].cpu().numpy().astype(np.float64).sum())
    GC.assert_same(sequential(route, n, n_env), GC.snapshot(eng), route)
    st = eng.learn_stats()
    assert st["steps"] == STEPS and st["done_rows"] == done_rows
    hist = np.asarray(st["taken_hist"])   # (learn_stats() cuts the histogram at the net's actions)
    assert np.array_equal(hist, taken[:len(hist)]) and not taken[len(hist):].any()
    assert abs(st["reward_sum"] - rew_sum) <= 1e-9 * STEPS * eng.batch * 24.0
    assert abs(st["target_sum"] - tgt_sum) <= 1e-9 * max(1.0, abs(tgt_sum)) + 1e-9 * STEPS * eng.batch * 100.0


@pytest.mark.parametrize("route,n,n_env", [("fused", 3, 1), ("per", 3, 3), ("head", 5, 1)])
def test_gpu_nstep_clipped_steps_match_the_clipped_oracle(route, n, n_env):
    """grad_clip on top of n-step against the oracle's step with torch's clip_grad_norm_ between its halves"""
    probe, _, _, _ = make_pair(route, n, n_env)
    norms = []
    for step in range(STEPS):
        probe.step = step
        rec, _, _ = GC.oracle_step(probe, None)
        norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for g in rec.grads.values()))))
    max_norm = float(np.median(norms))
    oracle, eng, _, _ = make_pair(route, n, n_env)
    eng.set_grad_clip(max_norm)
    clipped, loose = 0, {}
    for step in range(STEPS):
        oracle.step = step
        rec, norm, coef = GC.oracle_step(oracle, max_norm)
        run(eng, 1)
        torch.cuda.synchronize()
        eng.check_device_error()
        info = eng.grad_clip_info()
        assert abs(eng.loss() - rec.loss) <= 1e-5
        assert abs(info["last_norm"] - norm) <= 1e-5 * norm and abs(info["last_coef"] - coef) <= 1e-5
        clipped += coef < 1.0
        g = eng.param_views(eng.grads[:-1])
        for k, ref in rec.grads.items():
            loose[k] = (g[k].cpu() - ref).abs() > 1e-3 * ref.abs() + 1e-9
        GE.compare_state(oracle, eng, loose=None if route == "head" else loose)
        GE.sync_oracle(oracle, eng)
    assert 0 < clipped < STEPS and eng.grad_clip_info()["clipped_steps"] == clipped


# ---- 5. the state blob is the 1-step ring's --------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fused", "per", "head"])
def test_gpu_nstep_state_blob_loads_across_n_step(route):
    a3 = make_engine(route, n_step=3)
    a1 = make_engine(route, n_step=1)
    run(a3, 2)
    run(a1, 2)
    blob3, blob1 = a3.state_blob(), a1.state_blob()
    assert len(blob3) == len(blob1)   # n_step is configuration: nothing of it in the blob
    for blob, src in ((blob3, "from n_step 3"), (blob1, "from n_step 1")):
        into1, own1 = make_engine(route, n_step=1), make_engine(route, n_step=1)
        into3, own3 = make_engine(route, n_step=3), make_engine(route, n_step=3)
        run(into1, 1)   # (a receiving engine with steps behind it)
        run(into3, 1)
        for e in (into1, own1, into3, own3):
            e.load_state_blob(blob)
            run(e, 2)
        GC.assert_same(GC.snapshot(into1), GC.snapshot(own1), src)
        GC.assert_same(GC.snapshot(into3), GC.snapshot(own3), src)
        assert GC.snapshot(into1)["params"] != GC.snapshot(into3)["params"]   # each continues with its own n_step
    # and the n_step = 1 continuation of the n-step blob is what a default engine makes of that state
    assert a3.n_step == 3 and a1.n_step == 1


# ---- 6. the push rule ---------------------------------------------------------------------------------------
def test_gpu_nstep_push_of_a_partial_time_step_is_refused():
    eng = make_engine("fused", n_step=3, n_env=3)
    size, wptr = eng.ring_size, eng.ring_wptr
    before = eng.ring_rew.clone()
    with pytest.raises(C.DqnxError) as ei:
        eng.push(*O.synth_transitions(4, 14, 8, seed=3))
    assert ei.value.code == C.DQNX_EINVAL and "n_env" in str(ei.value)
    torch.cuda.synchronize()
    assert eng.ctrl().ring_size == size and eng.ctrl().ring_wptr == wptr and torch.equal(before, eng.ring_rew)
    eng.push(*O.synth_transitions(6, 14, 8, seed=3))   # two whole time steps: the engine goes on
    run(eng, 2)
    torch.cuda.synchronize()
    eng.check_device_error()
    assert eng.ctrl().ring_size == size + 6
    # a default engine takes any row count, as before
    e1 = make_engine("fused", n_step=1, n_env=3)
    e1.push(*O.synth_transitions(4, 14, 8, seed=3))
    run(e1, 1)
    e1.check_device_error()


# ---- 7. the drop-in Agent ------------------------------------------------------------------------------------
def test_gpu_agent_loop_with_n_step_from_the_environment(tmp_path, monkeypatch):
    """DQNX_N_STEP=3, n_env = 2: the train.py loop of test_gpu_agent_train_loop_matches_oracle against the
    wrapped oracle; actions and RNG ==, weights within 1e-5"""
    monkeypatch.setenv("DQNX_N_STEP", "3")
    algo, obs_dim, batch, buffer, n_fill, n_env, seed, steps = DDQN, 14, 32, 500, 300, 2, 17, 4
    torch.manual_seed(seed)
    agent = getattr(Agents, algo)(**agent_kwargs(algo, obs_dim, batch, buffer, tmp_path, n_env=n_env))
    assert agent.engine.n_step == 3 and agent.engine.cfg.n_step == 3
    spec = O.mlp_spec(obs_dim, 8, "dueling")
    init = O.reference_init(spec, seed)
    oracle = O.OracleLearner(spec, algo, batch, buffer, seed=seed, params=init, per_pow="cr", n_env=n_env)
    seen, forced = set(), [None]
    wrap_oracle(oracle, 3, n_env, seen, forced)
    obs, act, rew, _, nobs = O.synth_transitions(n_fill + steps * n_env, obs_dim, 8, seed=seed)
    done = np.random.default_rng(seed + 1).random(len(act)) < 1.0 / 6.0
    for i in range(0, n_fill, n_env):
        rows = (obs[i:i + n_env], [int(a) for a in act[i:i + n_env]], [float(r) for r in rew[i:i + n_env]],
                [bool(d) for d in done[i:i + n_env]], nobs[i:i + n_env])
        agent.store_transitions(*rows, None)
        oracle.store_transitions(*rows)
    random.seed(seed)
    np.random.seed(seed)
    for t in range(steps):
        agent.step = t
        agent.epsilon_start = 0.5
        lo, hi = n_fill + t * n_env, n_fill + (t + 1) * n_env
        x = obs[lo:hi]
        s0 = random.getstate()
        actions = agent.choose_actions(x)
        s1 = random.getstate()
        random.setstate(s0)
        ref_actions = O.greedy_actions(spec, oracle.online, x)
        for i in range(len(ref_actions)):
            if random.random() <= agent.epsilon():
                ref_actions[i] = random.randint(0, 7)
        assert random.getstate() == s1 and actions == ref_actions
        rows = (x, list(actions), [float(r) for r in rew[lo:hi]], [bool(d) for d in done[lo:hi]], nobs[lo:hi])
        agent.store_transitions(*rows, None)
        oracle.store_transitions(*rows)
        oracle.py_state = O.py_state_to_array()
        oracle.np_state = O.np_state_to_array()
        oracle.step = t
        agent.learn()
        agent.update_target_network()
        rec = oracle.learn()
        oracle.update_target_network()
        assert np.array_equal(np.asarray(random.getstate()[1], dtype=np.uint32), oracle.py_state)
        assert abs(agent.engine.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss))
        on, tg = agent.online_network.state_dict(), agent.target_network.state_dict()
        for k in init:
            np.testing.assert_allclose(on[k].cpu().numpy(), oracle.online[k].numpy(), atol=1e-5, rtol=0, err_msg=k)
            np.testing.assert_allclose(tg[k].cpu().numpy(), oracle.target[k].numpy(), atol=1e-5, rtol=0, err_msg=k)
    assert ("full",) in seen and any(k[0] == "done" for k in seen)
