"""GPU: offline evaluation (include/dqnx.h "offline evaluation"; LearnEngine.evaluate, dqn.offline.evaluate /
split / fit(validate=), Agent.evaluate_replay).

  1. parity with the oracle: the ring holds O.synth_transitions rows (capacity 100, 130 pushed: wrapped,
     wptr = 30), the parameters are O.reference_init's (online and target from different seeds), and the expected
     per-row values come from O.q_forward over the oracle-side copy of the rows, reduced in float64 with numpy.
     n_step = 3 uses the numpy window of tests/nstep_ref.py; bf16 the oracle's bf16 emulation and the bars
     tests/test_gpu_bf16.py states.
  2. nothing moves: state blobs byte-equal around evaluate, learn statistics untouched, and learn steps with an
     evaluation between every two bitwise the uninterrupted steps.
  3. determinism and additivity.  4. consistency with a given-indices learn step.  5. the Python layer."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from dqn import offline
from oracle import ref as O
from refnets import agent_kwargs
import nstep_ref as NR
import test_gpu_bf16 as BF
import test_gpu_grad_clip as GC
import test_gpu_nstep as NS

pytestmark = pytest.mark.gpu

CAP, PUSHED, GAMMA, SEED = 100, 130, 0.99, 11
DQN, DDQN, PER = "DQNAgent", "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"
RANGES = [(0, 100), (7, 44), (99, 100)]   # 32 + 32 + 32 + 4 (ragged tail, clamp) | unaligned at both ends | the newest row
BAND = 1e-4        # rows whose oracle top-two gap is inside it are left out of the greedy comparisons ...
BAND_FRAC = 0.02   # ... and may be at most this share of a range
TOL = 1e-5         # the project's bar for fp32 values against the oracle

ROUTES = {   # name: (net, algorithm, routing environment, engine kwargs, batch, n_step)
    "mlp14_dqn": ("mlp14", DQN, {}, {}, 32, 1),
    "mlp284": ("mlp284", DDQN, {}, {}, 32, 1),
    "slab": ("mlp14", DDQN, {"DQNX_DW_ADAM16": "0"}, {}, 32, 1),
    "per_layer": ("mlp14", DDQN, {"DQNX_BWD_PLAN": "0"}, {}, 32, 1),
    "head": ("head", DDQN, {}, {}, 16, 1),
    "im2col": ("head", DDQN, {"DQNX_MICRO_CNN": "0"}, {}, 16, 1),
    "per": ("mlp284", PER, {}, {}, 32, 1),
    "nstep3": ("mlp14", DDQN, {}, {}, 32, 3),
    "nstep3_per_layer": ("mlp14", DDQN, {"DQNX_BWD_PLAN": "0"}, {}, 32, 3),
    "bf16": ("mlp284", DDQN, {}, {"compute_dtype": "bf16"}, 32, 1),
}


# seeds per net, picked on the CPU so that the oracle alone meets BAND_FRAC (assert_oracle_not_vacuous asserts it)
NET_SEED = {"mlp14": SEED, "mlp284": SEED, "head": 18}


def _specs(net):
    spec, ospec, _, _ = NS.specs(net)
    return spec, ospec


def _data(net):
    spec, ospec = _specs(net)
    return NS.transitions(PUSHED, spec.obs_dim, ospec.macro_len or 14, NET_SEED[net] + 100)


def make_engine(route, cap=CAP, pushed=PUSHED, **over):
    net, algo, env, kw, batch, n_step = ROUTES[route]
    spec, ospec = _specs(net)
    with NS.routed(env):
        eng = E.LearnEngine(spec, algo, batch, cap, n_step=n_step, gamma=GAMMA, **{**kw, **over})
    seed = NET_SEED[net]
    eng.load_params(O.reference_init(ospec, seed), target=O.reference_init(ospec, seed + 1))
    data = NS.transitions(pushed, spec.obs_dim, ospec.macro_len or 14, seed + 100)
    half = pushed // 2
    eng.push(*(x[:half] for x in data))
    eng.push(*(x[half:] for x in data))
    random.seed(SEED + 7)
    np.random.seed(SEED + 11)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    eng.set_rng(C.DQNX_RNG_NP, O.np_state_to_array())
    eng.route_env = env
    return eng


def evaluate(eng, lo=0, hi=None, rows=False):
    with NS.routed(eng.route_env):
        return eng.evaluate(lo, hi, rows=rows)


@functools.lru_cache(maxsize=None)
def expected(route):
    """per-row expected values for logical positions 0 .. CAP-1 of the wrapped ring (float64 / int arrays),
    from the oracle's forward over its own copy of the rows; computed once per route and never modified"""
    net, algo, _, kw, _, n_step = ROUTES[route]
    _, ospec = _specs(net)
    bf = kw.get("compute_dtype") == "bf16"
    obs, act, rew, done, nobs = (x[PUSHED - CAP:] for x in _data(net))   # deque order: the newest CAP rows
    online, target = O.reference_init(ospec, NET_SEED[net]), O.reference_init(ospec, NET_SEED[net] + 1)
    R, d, disc, last, _ = NR.windows(rew, done, CAP, np.arange(CAP), n_step, 1, GAMMA)
    if n_step == 1:
        assert np.array_equal(R, rew) and np.array_equal(d, done.astype(np.float32)) and np.array_equal(last, np.arange(CAP))
    with torch.no_grad():
        x, xn = torch.from_numpy(obs), torch.from_numpy(nobs[last])
        q0 = O.q_forward(ospec, online, x, bf).double().numpy()
        q2 = O.q_forward(ospec, target, xn, bf).double().numpy()
        if algo == DQN:
            sel = q2.max(1)
        else:
            q1 = O.q_forward(ospec, online, xn, bf)
            sel = q2[np.arange(CAP), q1.argmax(1).numpy()]
    a = np.where((act < 0) | (act >= q0.shape[1]), 0, act).astype(np.int64)
    y = R.astype(np.float64) + (1.0 - d.astype(np.float64)) * disc.astype(np.float64) * sel
    qa = q0[np.arange(CAP), a]
    delta = y - qa
    z = np.abs(delta)
    srt = np.sort(q0, 1)
    v = srt[:, -1]
    out = {"act": a, "g": q0.argmax(1), "qa": qa, "v": v, "delta": delta, "y": y, "rew": R.astype(np.float64),
           "done": d != 0, "lb": np.where(z < 1.0, 0.5 * z * z, z - 0.5),
           "gap": v + np.log(np.exp(q0 - v[:, None]).sum(1)) - qa, "agap": srt[:, -1] - srt[:, -2]}
    for x in out.values():
        x.setflags(write=False)
    return out


def assert_oracle_not_vacuous(route):
    """on the oracle side alone: every range keeps at least 98 % of its rows in the greedy comparison (the newest
    row, a range of its own, is outside the band), both greedy outcomes occur, and dones occur"""
    ex = expected(route)
    clear = ex["agap"] > BAND
    for lo, hi in RANGES:
        assert (~clear[lo:hi]).mean() <= BAND_FRAC, (route, lo, hi)
    assert clear[CAP - 1]
    agree = ex["g"] == ex["act"]
    assert agree.any() and (~agree).any() and ex["done"].any() and not ex["done"].all()
    assert np.unique(ex["g"]).size >= 2
    return clear


def _bars(route):
    """(per-value bar, share of values that may exceed the tight bar): fp32 -- the project's 1e-5, none beyond;
    bf16 -- tests/test_gpu_bf16.py's Q_ATOL with at most Q_FLIP_FRAC of the values beyond Q_TIGHT"""
    if ROUTES[route][3].get("compute_dtype") == "bf16":
        return BF.Q_ATOL, BF.Q_TIGHT, BF.Q_FLIP_FRAC
    return TOL, TOL, 0.0


def _close(got, want, bar, tight, frac, what, scale=1.0):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    over = float((d > tight * scale).mean())
    print(f"{what}: max |d| {float(d.max()):.3e}, beyond {tight * scale:.1e}: {over:.3f}")
    # one 2 % of a 1-row range is no row: the flip share is over the values compared, at least one allowed where any are
    assert d.max() <= bar * scale and over <= max(frac, (1.0 / d.size) if frac else 0.0), (what, float(d.max()), over)


# ---- 1. parity with the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", list(ROUTES))
def test_gpu_eval_matches_oracle(route):
    clear = assert_oracle_not_vacuous(route)
    ex = expected(route)
    eng = make_engine(route)
    assert eng.ring_size == CAP and eng.ring_wptr == PUSHED - CAP != 0
    bar, tight, frac = _bars(route)
    A = eng.spec.n_actions
    for lo, hi in RANGES:
        res, rows = evaluate(eng, lo, hi, rows=True)
        eng.check_device_error()
        rows = rows.cpu().numpy()
        n = hi - lo
        sl = slice(lo, hi)
        assert rows.shape == (n, 4) and np.isfinite(rows).all()
        what = f"{route} [{lo}, {hi})"
        _close(rows[:, 1], ex["qa"][sl], bar, tight, frac, what + " q_a")
        _close(rows[:, 2], ex["v"][sl], bar, tight, frac, what + " v")
        _close(rows[:, 3], ex["delta"][sl], bar, tight, frac, what + " delta", scale=2.0 if frac else 1.0)
        # exact integers
        assert res["rows"] == n
        assert res["done_rows"] == int(ex["done"][sl].sum())
        assert res["taken_hist"] == np.bincount(ex["act"][sl], minlength=A).tolist()
        # greedy action, on every row whose oracle top-two gap is outside the band
        c = clear[sl]
        g = rows[:, 0].astype(np.int64)
        assert np.array_equal(rows[:, 0], g) and np.array_equal(g[c], ex["g"][sl][c]), what
        unclear = int((~c).sum())
        assert abs(res["agree_rows"] - int((ex["g"][sl] == ex["act"][sl])[c].sum())) <= unclear
        assert sum(res["greedy_hist"]) == n
        assert np.abs(np.asarray(res["greedy_hist"]) - np.bincount(ex["g"][sl][c], minlength=A)).sum() <= unclear
        if unclear == 0:
            assert res["agree_rows"] == int((ex["g"][sl] == ex["act"][sl]).sum())
            assert res["greedy_hist"] == np.bincount(ex["g"][sl], minlength=A).tolist()
        assert res["agree_rows"] == int((g == ex["act"][sl]).sum())       # the totals are the per-row output's
        assert res["greedy_hist"] == np.bincount(g, minlength=A).tolist()
        # means: the same bar
        for key, col in (("loss", "lb"), ("abs_td_mean", None), ("q_sa_mean", "qa"), ("v_mean", "v"), ("cql_gap", "gap"),
                         ("action_gap_mean", "agap"), ("reward_mean", "rew"), ("target_mean", "y")):
            want = np.abs(ex["delta"][sl]).mean() if col is None else ex[col][sl].mean()
            mbar = bar * (2.0 if frac and key in ("loss", "abs_td_mean") else 1.0)
            print(f"{what} {key}: {res[key]:.9g} vs {want:.9g}")
            assert abs(res[key] - want) <= mbar * max(1.0, abs(want)), (what, key, res[key], want)
        assert abs(res["td_rms"] - np.sqrt((ex["delta"][sl] ** 2).mean())) <= 2 * bar * max(1.0, res["td_rms"])
        assert abs(res["abs_td_max"] - np.abs(ex["delta"][sl]).max()) <= 2 * bar
        assert abs(res["v_max"] - ex["v"][sl].max()) <= bar and abs(res["v_min"] - ex["v"][sl].min()) <= bar
        # the totals are the per-row output's own, reduced in float64
        assert res["q_sa_mean"] == pytest.approx(rows[:, 1].astype(np.float64).mean(), rel=1e-12, abs=1e-12)
        assert res["v_max"] == float(rows[:, 2].max()) and res["v_min"] == float(rows[:, 2].min())
        assert res["abs_td_max"] == float(np.abs(rows[:, 3]).max())


def test_gpu_eval_nstep_newest_rows_are_cut_windows():
    """n_step = 3: the two newest rows are windows cut by the ring's end (m = 1 and 2); they are valid rows."""
    ex = expected("nstep3")
    rew, done = (x[PUSHED - CAP:] for x in _data("mlp14")[2:4])
    kinds = [NR.kind(rew, done, CAP, p, 3, 1) for p in (CAP - 1, CAP - 2)]
    assert kinds[0] in {("end", 1), ("done", 0)} and kinds[1] in {("end", 2), ("done", 0), ("done", 1)}
    assert NR.every_kind(3) <= NR.census(rew, done, CAP, range(CAP), 3, 1)
    eng = make_engine("nstep3")
    res, rows = evaluate(eng, CAP - 2, CAP, rows=True)
    eng.check_device_error()
    assert res["rows"] == 2
    assert np.abs(rows[:, 3].cpu().numpy() - ex["delta"][CAP - 2:]).max() <= TOL
    assert abs(res["reward_mean"] - ex["rew"][CAP - 2:].mean()) <= TOL


def test_gpu_eval_refusals():
    eng = make_engine("mlp14_dqn")
    for lo, hi in ((-1, 5), (0, CAP + 1), (5, 5), (9, 3)):
        with pytest.raises(C.DqnxError) as ei:
            eng.evaluate(lo, hi)
        assert ei.value.code == C.DQNX_EINVAL
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        eng.eval_scratch()
        torch.cuda.synchronize()
        g.capture_begin()
        try:
            with pytest.raises(C.DqnxError) as ei:
                eng.evaluate(0, 10)
            assert ei.value.code == C.DQNX_ESTATE
        finally:
            g.capture_end()
    assert eng.evaluate(0, 10)["rows"] == 10


# ---- 2. nothing moves --------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["mlp284", "per", "head"])
def test_gpu_eval_leaves_the_state_blob_and_statistics(route):
    eng = make_engine(route)
    with NS.routed(eng.route_env):
        for _ in range(2):
            eng.learn_step(soft_update=True, stats=True)
    blob = eng.state_blob().tobytes()
    stats = bytes(eng.learn_stats_raw())
    q, td = eng.q.clone(), eng.td.clone()
    for lo, hi in RANGES:
        evaluate(eng, lo, hi, rows=True)
    assert eng.state_blob().tobytes() == blob
    assert bytes(eng.learn_stats_raw()) == stats
    assert torch.equal(eng.q, q) and torch.equal(eng.td, td)   # DQNX_BUF_Q / DQNX_BUF_TD still the last step's
    eng.check_device_error()


def _loop(route, mode, with_eval, **over):
    eng = make_engine(route, cap=500, pushed=400, **over)
    losses = []
    with NS.routed(eng.route_env):
        if mode == "learn_steps":
            if with_eval:
                eng.learn_steps(4, soft_update=True)
                eng.evaluate(3, 390)
                eng.learn_steps(4, soft_update=True)
            else:
                eng.learn_steps(8, soft_update=True)
        else:
            for i in range(8):
                eng.learn_step(soft_update=True, prefetch=(mode == "prefetch" and i < 7))
                losses.append(eng.loss() if mode != "prefetch" else 0.0)
                if with_eval and i % 2 == 1 and i < 7:
                    eng.evaluate(3, 390)
    snap = GC.snapshot(eng)
    snap["losses"] = losses
    snap["q"], snap["td"] = eng.q.cpu().numpy().tobytes(), eng.td.cpu().numpy().tobytes()
    return snap


@pytest.mark.parametrize("route,mode,over", [
    ("mlp284", "prefetch", {}), ("head", "prefetch", {}), ("per_layer", "prefetch", {}),
    ("mlp284", "learn_steps", {}), ("mlp284", "steps", {"graphs": True}), ("mlp284", "steps", {"cql_alpha": 1.0}),
    ("per", "steps", {}), ("nstep3", "prefetch", {}), ("slab", "steps", {}), ("bf16", "steps", {})])
def test_gpu_eval_between_learn_steps_is_bitwise_invisible(route, mode, over):
    """eight learn steps with an evaluation between every two are bitwise eight uninterrupted steps: parameters,
    target, Adam moments, RNG states, loss (PER: the SumTree too), and the last step's q / td buffers"""
    a, b = _loop(route, mode, False, **over), _loop(route, mode, True, **over)
    GC.assert_same(a, b, (route, mode))


# ---- 3. determinism and additivity ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["mlp284", "head", "nstep3"])
def test_gpu_eval_is_deterministic_and_additive(route):
    eng = make_engine(route)
    with NS.routed(eng.route_env):
        r1 = eng.evaluate_raw(0, CAP)
        full = torch.empty((CAP, 4), device=eng.device)
        r2 = eng.evaluate_raw(0, CAP, full)
        ra, rb = eng.evaluate_raw(0, 50), eng.evaluate_raw(50, CAP)
        sub = torch.empty((37, 4), device=eng.device)
        eng.evaluate_raw(7, 44, sub)
        r3 = eng.evaluate_raw(0, CAP)
    assert bytes(r1) == bytes(r2) == bytes(r3)
    assert torch.equal(sub, full[7:44])   # a sub-range's rows are the full range's, bit for bit
    for name, t in C.EvalResult._fields_:
        x, xa, xb = getattr(r1, name), getattr(ra, name), getattr(rb, name)
        if name in ("greedy_hist", "taken_hist"):
            assert [p + q for p, q in zip(xa, xb)] == list(x), name
        elif t is C.I64:
            assert xa + xb == x, name
        elif name in ("abs_td_max", "v_max"):
            assert max(xa, xb) == x, name
        elif name == "v_min":
            assert min(xa, xb) == x
        else:
            assert abs((xa + xb) - x) <= 1e-12 * max(abs(x), 1e-300), (name, xa + xb, x)
    assert r1.rows == CAP and ra.rows == 50 and rb.rows == 50


# ---- 4. consistency with the learn step ----------------------------------------------------------------------
@pytest.mark.parametrize("route,lo", [("mlp284", 0), ("mlp284", 61), ("mlp14_dqn", 68), ("nstep3", 68), ("per_layer", 40),
                                      ("head", 84)])
def test_gpu_eval_agrees_with_a_given_indices_step(route, lo):
    eng = make_engine(route)
    B = eng.batch
    res, rows = evaluate(eng, lo, lo + B, rows=True)
    eng.batch_idx[:B].copy_(torch.arange(lo, lo + B, dtype=torch.int32))
    with NS.routed(eng.route_env):
        eng.learn_step(given_indices=True, grads_only=True)
    torch.cuda.synchronize()
    eng.check_device_error()
    y, qa = eng.td[0], eng.td[1]
    fused_fp32 = eng.route_env == {}  and route != "head"
    if fused_fp32:   # the row arithmetic is the same code over the same forward: bitwise
        assert torch.equal(rows[:, 1], qa) and torch.equal(rows[:, 3], y - qa)
        assert torch.equal(rows[:, 2], eng.q[0].max(1).values)
        assert torch.equal(rows[:, 0], eng.q[0].argmax(1).float())
    else:            # the per-layer head kernel forms Q in another order: the project's bar
        assert (rows[:, 1] - qa).abs().max() <= TOL and (rows[:, 3] - (y - qa)).abs().max() <= TOL
    assert abs(eng.loss() - res["loss"]) <= 1e-6 * max(abs(res["loss"]), 1e-30)
    gap = float((torch.logsumexp(eng.q[0].double(), 1) - qa.double()).mean())
    assert abs(res["cql_gap"] - gap) <= TOL


# ---- 5. the Python layer -------------------------------------------------------------------------------------
def test_gpu_offline_split_evaluate_and_fit(tmp_path):
    src = NS.make_engine("fused")   # capacity 500, 400 rows
    NS.run(src, 3)
    path = str(tmp_path / "run.dqnx")
    src.save_state(path)
    rows = offline.ring_rows(src)
    train, val = offline.split(path, 100, batch=32, cql_alpha=0.5)
    assert train.ring_size == 300 and val.ring_size == 100 and train.cql_alpha == val.cql_alpha == 0.5
    for eng, lo, hi in ((train, 0, 300), (val, 300, 400)):
        got = offline.ring_rows(eng)
        for g, w in zip(got, rows):
            assert np.array_equal(g, w[lo:hi])
        assert torch.equal(eng.params, src.params) and torch.equal(eng.target_params, src.target_params)
        assert np.array_equal(eng.get_rng(0), src.get_rng(0))
    with pytest.raises(ValueError):
        offline.split(path, 400, batch=32)
    # fit with the defaults: the list a direct loop gives, as before
    direct = offline.engine_from_state(train.state_blob(), batch=32, cql_alpha=0.5)
    log = offline.fit(train, steps=6, log_every=2)
    want = []
    for i in range(6):
        direct.learn_step(soft_update=True)
        if i % 2 == 1:
            want.append({"step": i + 1, "loss": direct.loss(), "cql_gap": direct.cql_gap(),
                         "q_sa_mean": float(direct.td[1].mean())})
    assert log == want and all(sorted(r) == ["cql_gap", "loss", "q_sa_mean", "step"] for r in log)
    GC.assert_same(GC.snapshot(direct), GC.snapshot(train), "offline.fit defaults")
    assert offline.fit(train, steps=1) == []
    direct.learn_step(soft_update=True)
    # evaluate(train, data=val) is val.evaluate() after copying the parameters by hand
    before = GC.snapshot(train)
    got = offline.evaluate(train, data=val)
    hand = offline.engine_from_state(val.state_blob(), batch=32)
    hand.params.copy_(train.params)
    hand.target_params.copy_(train.target_params)
    hand.params_modified()
    assert got == hand.evaluate() and got["rows"] == 100
    assert offline.evaluate(train) == train.evaluate() and train.evaluate()["rows"] == 300
    GC.assert_same(before, GC.snapshot(train), "evaluate")
    # validation inside fit: val_* at the boundaries, the learn steps bitwise those without validation
    log = offline.fit(train, steps=5, log_every=2, validate=val, validate_every=2)
    for _ in range(5):
        direct.learn_step(soft_update=True)
    GC.assert_same(GC.snapshot(direct), GC.snapshot(train), "offline.fit validate")
    assert [r["step"] for r in log] == [2, 4, 5]
    for r in log:
        assert {"loss", "cql_gap", "q_sa_mean", "val_loss", "val_cql_gap", "val_agree"} <= set(r)
        assert np.isfinite([r["val_loss"], r["val_cql_gap"]]).all() and 0.0 <= r["val_agree"] <= 1.0
    assert log[-1]["val_loss"] == offline.evaluate(train, data=val)["loss"]
    only_val = offline.fit(train, steps=2, validate_every=2)   # no log_every: the record is the validation's
    assert [sorted(r) for r in only_val] == [sorted(["step", "val_loss", "val_cql_gap", "val_agree", "val_q_sa_mean",
                                                     "val_v_mean", "val_abs_td_mean"])]


def test_gpu_agent_evaluate_replay(tmp_path):
    agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs(DDQN, 14, 32, 500, tmp_path))
    obs, act, rew, done, nobs = O.synth_transitions(100, 14, 8, seed=1)
    for i in range(100):
        agent.store_transitions(obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1], None)
    for t in range(3):
        agent.step = t
        agent.learn()
        agent.update_target_network()
    res = agent.evaluate_replay()
    assert res["rows"] == 100 and res["taken_hist"] == np.bincount(act, minlength=8).tolist()
    assert res["done_rows"] == int(done.sum()) and np.isfinite(res["loss"])
    part = agent.evaluate_replay(10, 40)
    assert part["rows"] == 30 and part["taken_hist"] == np.bincount(act[10:40], minlength=8).tolist()
    agent.learn()   # the loop goes on
    agent.flush()
