"""GPU: fitted Q evaluation (include/dqnx.h "fitted Q evaluation"; LearnEngine.policy_actions / set_target_policy /
fqe_value, dqn.offline.fqe).

  1. the policy sweep against the oracle's argmax by ring slot (wrapped ring, ragged ranges, every route family);
  2. learn steps with a target-policy table against FqeOracle: oracle.ref.OracleLearner with learn() restated and
     sel = gather(tq, pi_next).  The tables of these tests are built FROM THE ORACLE (its argmax over the ring rows),
     not by the sweep, so 2. does not lean on 1.;
  3. off is off; the step forms are bitwise the sequential steps; clipping on top; the device check;
  4. fqe_value against a float64 restatement; nothing of the training state moves;  5. dqn.offline.fqe."""
import copy
import functools
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dqn import _capi as C
from dqn import engine as E
from dqn import offline
from oracle import ref as O
from parity import assert_grad_close
import test_gpu_bf16 as GB
import test_gpu_cql as GQ
import test_gpu_engine as GE
import test_gpu_eval as GV
import test_gpu_grad_clip as GC
import test_gpu_hybrid as GH
import test_gpu_nstep as GN
import test_gpu_per as GP

pytestmark = pytest.mark.gpu

SEED, FILL, CAP, STEPS = 11, 400, 500, 4
DQN, DDQN, PER = "DQNAgent", "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"
POLICY_SEED = 31        # the policy: a second oracle's parameters from another seed; picked on the CPU so that the
                        # oracle alone keeps every sweep range under BAND_FRAC (the sweep test asserts it)
BAND, BAND_FRAC = 1e-4, 0.02


# ---- 1. the policy sweep -----------------------------------------------------------------------------------------
SWEEP = {   # test_gpu_eval's routes (capacity 100, 130 pushed: wrapped, wptr = 30)
    "fused": "mlp284", "per_layer": "per_layer", "head": "head", "dqn": "mlp14_dqn", "nstep3": "nstep3"}


@functools.lru_cache(maxsize=None)
def sweep_expected(route):
    """(table by ring slot int64 [CAP, 2], top-two gaps [CAP, 2]) from the oracle's forward with the policy's
    parameters over its own copy of the rows; computed once per route and never modified"""
    net = GV.ROUTES[route][0]
    _, ospec = GV._specs(net)
    obs, _, _, _, nobs = (x[GV.PUSHED - GV.CAP:] for x in GV._data(net))    # logical order: the newest CAP rows
    pol = O.reference_init(ospec, POLICY_SEED)
    slot = (np.arange(GV.CAP) + GV.PUSHED) % GV.CAP                           # logical p -> slot (wptr = 30, full)
    table, gaps = np.zeros((GV.CAP, 2), np.int64), np.zeros((GV.CAP, 2))
    with torch.no_grad():
        for k, x in enumerate((obs, nobs)):
            q = O.q_forward(ospec, pol, torch.from_numpy(x)).double().numpy()
            srt = np.sort(q, 1)
            table[slot, k] = q.argmax(1)
            gaps[slot, k] = srt[:, -1] - srt[:, -2]
    table.setflags(write=False)
    gaps.setflags(write=False)
    return table, gaps, slot


@pytest.mark.parametrize("route", list(SWEEP))
def test_gpu_policy_sweep_matches_the_oracle_argmax(route):
    r = SWEEP[route]
    want, gaps, slot = sweep_expected(r)
    clear = gaps >= BAND
    # on the oracle alone: the seed keeps the skipped rows of every range under the cap; the policy is no constant
    for lo, hi in GV.RANGES:
        assert (~clear[slot[lo:hi]]).any(1).mean() <= BAND_FRAC, (route, lo, hi)
    assert np.unique(want).size >= 2
    eng = GV.make_engine(r)
    _, ospec = GV._specs(GV.ROUTES[r][0])
    eng.load_params(O.reference_init(ospec, POLICY_SEED), target=O.reference_init(ospec, GV.NET_SEED[GV.ROUTES[r][0]] + 1))
    blob = eng.state_blob().tobytes()
    for lo, hi in GV.RANGES:
        with GN.routed(eng.route_env):
            table = eng.policy_actions(lo, hi)
        torch.cuda.synchronize()
        eng.check_device_error()
        got = table.cpu().numpy()
        touched = np.zeros(GV.CAP, bool)
        touched[slot[lo:hi]] = True
        assert (got[~touched] == -1).all(), (route, lo, hi)               # untouched slots keep their sentinel
        for k in (0, 1):
            m = touched & clear[:, k]
            assert np.array_equal(got[m, k], want[m, k]), (route, lo, hi, k, np.flatnonzero(m & (got[:, k] != want[:, k])))
        assert ((got[touched] >= 0) & (got[touched] < ospec.n_actions)).all()
    # out=: the ranges accumulate into one table; the call touched nothing of the training state
    table = eng.policy_actions(0, 50)
    with GN.routed(eng.route_env):
        assert eng.policy_actions(50, 100, out=table) is table
    assert (table.cpu().numpy() >= 0).all()
    assert eng.state_blob().tobytes() == blob


def test_gpu_policy_sweep_refusals():
    eng = GV.make_engine("mlp14_dqn")
    with pytest.raises(RuntimeError):
        eng.policy_actions(0, 101)
    with pytest.raises(RuntimeError):
        eng.policy_actions(5, 5)
    with pytest.raises(RuntimeError):
        eng.policy_actions(0, 10, out=torch.zeros((99, 2), dtype=torch.int32, device=eng.device))
    with pytest.raises(RuntimeError):
        eng.fqe_value(torch.zeros((101, 2), dtype=torch.int32, device=eng.device))


# ---- 2. learn parity with the FQE oracle --------------------------------------------------------------------------
class FqeOracle(O.OracleLearner):
    """OracleLearner whose target is r + (1 - d) * gamma * Q_target(s', pi(s')) with pi(s') read from a table by
    logical position (self.pi_next).  learn() restates the parent's with sel = gather(tq, pi_next)."""
    pi_next = None

    def learn(self, shard=None):
        rec = O.StepRecord()
        B = self.batch_size
        if self.per:
            is_w, idxs, transitions = self.replay.sample_transitions(self.step * self.n_env, self.np_state)
            rec.positions = np.asarray(idxs, dtype=np.int64)
            rec.is_weights = np.asarray(is_w, dtype=np.float64)
            is_weights_t = torch.as_tensor(np.asarray(is_w), dtype=torch.float32).unsqueeze(-1)
            pos = rec.positions - (self.pi_next.shape[0] - 1)      # tree leaves -> slots
        else:
            transitions, pos = self.replay.sample_transitions(self.py_state)
            rec.positions = pos
        obses_t, actions_t, rews_t, dones_t, new_obses_t = O.transitions_to_tensor(transitions)
        with torch.no_grad():
            best = torch.as_tensor(self.pi_next[np.asarray(pos, dtype=np.int64)], dtype=torch.int64).unsqueeze(-1)
            tq = self._q(self.target, new_obses_t)
            rec.q_target_next = tq
            sel = torch.gather(input=tq, dim=1, index=best)
            targets = rews_t + (1 - dones_t) * self.gamma * sel
        rec.targets = targets
        params = OrderedDict((k, v.detach().clone().requires_grad_(True)) for k, v in self.online.items())
        q = self._q(params, obses_t)
        rec.q_online = q.detach()
        qa = torch.gather(input=q, dim=1, index=actions_t)
        if self.per:
            with torch.no_grad():
                abs_td = torch.abs(targets - qa).detach().cpu().numpy()
                rec.abs_td = abs_td
                if shard is None:
                    self.replay.update_batch_priorities(rec.positions.tolist(), abs_td)
            per_sample = is_weights_t * F.smooth_l1_loss(qa, targets, reduction="none")
            loss = torch.mean(per_sample) if shard is None else per_sample[shard[0]:shard[1]].sum() / B
        elif shard is None:
            loss = F.smooth_l1_loss(qa, targets, reduction="mean")
        else:
            loss = F.smooth_l1_loss(qa[shard[0]:shard[1]], targets[shard[0]:shard[1]], reduction="sum") / B
        rec.loss = float(loss.item())
        grads = torch.autograd.grad(loss, list(params.values()))
        rec.grads = OrderedDict(zip(params.keys(), [g.detach() for g in grads]))
        if shard is None:
            self.apply_grads(rec.grads)
        return rec


def oracle_table(oracle, eng, seed=POLICY_SEED):
    """int32 [capacity, 2] by ring slot from the ORACLE's forward of a policy (the oracle's network from another
    seed) over the ring's rows; unfilled slots -1.  The rings of these pairs are not wrapped: slot = position."""
    assert eng.ring_size == eng.ring_wptr < eng.capacity
    pol = O.reference_init(oracle.spec, seed)
    n, D = eng.ring_size, eng.spec.obs_dim
    table = np.full((eng.capacity, 2), -1, np.int32)
    with torch.no_grad():
        for k, ring in enumerate((eng.ring_obs, eng.ring_next_obs)):
            table[:n, k] = oracle._q(pol, ring[:n, :D].cpu()).argmax(1).numpy()
    return table


def to_fqe(oracle, table):
    oracle.__class__ = FqeOracle
    oracle.pi_next = np.asarray(table[:, 1], dtype=np.int64)
    return oracle


def assert_not_vacuous(oracle, plain_cls):
    """On the oracles alone, from the pair's state, step 0: the FQE loss differs from the engine's own rule's by
    more than 1e-3 and some tensor's gradient by more than 10 x assert_grad_close's tolerance."""
    o1, o0 = copy.deepcopy(oracle), copy.deepcopy(oracle)
    o0.__class__ = plain_cls
    r1, r0 = o1.learn(), o0.learn()
    assert abs(r1.loss - r0.loss) > 1e-3, (r1.loss, r0.loss)
    over = {k: float((np.abs(r1.grads[k].numpy() - r0.grads[k].numpy()) / GQ.grad_tol(r0.grads[k].numpy())).max())
            for k in r0.grads}
    print("fqe vs own rule: loss", r1.loss, r0.loss, "max |dg| / tol", over)
    assert max(over.values()) > 10.0, over


def set_table(eng, table):
    t = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).to(eng.device)
    eng.set_target_policy(t)
    return t


def check_step(oracle, eng, rec, step, loose):
    torch.cuda.synchronize()
    eng.check_device_error()
    per, cap = oracle.per, eng.capacity
    idx = eng.batch_idx.cpu().numpy().astype(np.int64) + (cap - 1 if per else 0)
    assert np.array_equal(idx, rec.positions), f"step {step}: sampled positions differ"
    q = eng.q.cpu()
    np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(q[2].numpy(), rec.q_target_next.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.td[0].cpu().numpy(), rec.targets.view(-1).numpy(), atol=1e-5, rtol=0)
    print(f"step {step}: loss {eng.loss()} vs {rec.loss}")
    assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss)), (step, eng.loss(), rec.loss)
    g = eng.param_views(eng.grads[:-1])
    for k, ref in rec.grads.items():
        gk = g[k].cpu()
        assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
        loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
    GE.compare_state(oracle, eng, loose=loose)
    if per:
        np.testing.assert_allclose(eng.is_weights.cpu().numpy(), rec.is_weights.astype(np.float32),
                                   rtol=2e-7 if step == 0 else 1e-5)
        np.testing.assert_allclose(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1), atol=1e-5, rtol=0)
        same = np.array_equal(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1).astype(np.float32))
        oracle.tree_exact = getattr(oracle, "tree_exact", True) and same
        GP.assert_tree_equal(eng, oracle.replay.replay_buffer, exact=oracle.tree_exact)
    GE.sync_oracle(oracle, eng)


@pytest.mark.parametrize("route", list(GQ.PARITY))
def test_gpu_fqe_steps_match_the_fqe_oracle(monkeypatch, route):
    build, env = GQ.PARITY[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    oracle, eng = build()
    plain = oracle.__class__
    table = oracle_table(oracle, eng)
    to_fqe(oracle, table)
    assert_not_vacuous(oracle, plain)
    keep = set_table(eng, table)
    q1 = eng.q[1].clone()
    loose = {}
    for step in range(STEPS):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        check_step(oracle, eng, rec, step, loose)
    assert torch.equal(eng.q[1], q1)     # DQNX_BUF_Q[1] is left unwritten: no online(s') stream
    assert np.array_equal(eng.get_rng(1 if oracle.per else 0), oracle.np_state if oracle.per else oracle.py_state)
    del keep


@pytest.mark.parametrize("head,A", [("dueling", 15), ("linear", 16), ("linear", 1)])
def test_gpu_fqe_head_widths_match_the_fqe_oracle(head, A):
    oracle, eng = GQ.width_pair(head, A)
    eng.set_cql_alpha(0)
    oracle.__class__ = O.OracleLearner
    table = oracle_table(oracle, eng)
    to_fqe(oracle, table)
    if A > 1:
        assert_not_vacuous(oracle, O.OracleLearner)
    keep = set_table(eng, table)
    loose = {}
    for step in range(2):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        check_step(oracle, eng, rec, step, loose)
    del keep


def test_gpu_fqe_bf16_matches_the_bf16_fqe_oracle():
    emu, _, eng = GB.make_bf16_pair(DDQN, 284, 64, CAP, FILL, SEED, graphs=False)
    plain = emu.__class__
    table = oracle_table(emu, eng)
    to_fqe(emu, table)
    assert_not_vacuous(emu, plain)
    keep = set_table(eng, table)
    for step in range(STEPS):
        rec = emu.train_step()
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        GB._check_step(eng, rec, None, step)
        GB._compare_weights(emu, eng)
        GE.sync_oracle(emu, eng)
    assert np.array_equal(eng.get_rng(0), emu.py_state)
    del keep


# ---- 3. off is off; the step forms ---------------------------------------------------------------------------------
COMPOSE = ["fused", "per_layer", "head", "per"]   # k_head_bwd, k_head (ReLU), k_head (ELU), PER


def fqe_engine(route, **over):
    """test_gpu_nstep's engine of the route with the table of another seed's policy set (by the engine's sweep)"""
    eng = GN.make_engine(route, **over)
    own = eng.params.clone(), eng.target_params.clone()
    _, ospec, _, _ = GN.specs(GN.ROUTES[route][0])
    eng.load_params(O.reference_init(ospec, POLICY_SEED))
    with GN.routed(eng.route_env):
        eng.fqe_table = eng.policy_actions()
    eng.params.copy_(own[0])
    eng.target_params.copy_(own[1])
    eng.params_modified()
    eng.set_target_policy(eng.fqe_table)
    return eng


@functools.lru_cache(maxsize=None)
def sequential(route, steps=STEPS):
    eng = fqe_engine(route)
    GN.run(eng, steps)
    snap = GC.snapshot(eng)
    if steps == STEPS:   # the table is in these steps: another trajectory than the engine's own rule
        off = GN.make_engine(route)
        GN.run(off, steps)
        assert GC.snapshot(off)["params"] != snap["params"]
    return snap


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_off_is_bitwise_the_default_step(route):
    e1 = fqe_engine(route)
    e1.set_target_policy(None)
    e0 = GN.make_engine(route)
    GN.run(e0, 8)
    GN.run(e1, 8)
    GC.assert_same(GC.snapshot(e0), GC.snapshot(e1), route)
    assert torch.equal(e0.q, e1.q) and torch.equal(e0.td, e1.td) and torch.equal(e0.grads, e1.grads)
    assert GN.kernel_names(e0) == GN.kernel_names(e1)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_learn_steps_equal_single_steps(route):
    eng = fqe_engine(route)
    with GN.routed(eng.route_env):
        eng.learn_steps(8, soft_update=True)
    GC.assert_same(sequential(route, 8), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_prefetch_loop_equals_sequential_steps(route):
    eng = fqe_engine(route)
    GN.run(eng, STEPS - 1, prefetch=True)
    GN.run(eng, 1)   # consumes the pending minibatch
    GC.assert_same(sequential(route), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_graphs_on_equals_off(route):
    eng = fqe_engine(route, graphs=True)
    GN.run(eng, STEPS)
    GC.assert_same(sequential(route), GC.snapshot(eng), route)
    # clearing the table reaches the replayed graphs: the cached plans are dropped
    eng.set_target_policy(None)
    off = GN.make_engine(route, graphs=True)
    off.load_state_blob(eng.state_blob())
    GN.run(eng, 1)
    GN.run(off, 1)
    GC.assert_same(GC.snapshot(off), GC.snapshot(eng), route + " after clearing the table")


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_grads_only_plus_apply_equals_the_step(route):
    eng = fqe_engine(route)
    with GN.routed(eng.route_env):
        for _ in range(STEPS):
            eng.learn_step(grads_only=True)
            eng.apply_grads(soft_update=True)
    GC.assert_same(sequential(route), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_with_stats_changes_nothing_else(route):
    eng = fqe_engine(route)
    for _ in range(STEPS):
        GN.run(eng, 1, stats=True)
    GC.assert_same(sequential(route), GC.snapshot(eng), route)
    assert eng.learn_stats()["steps"] == STEPS


@pytest.mark.parametrize("case", ["mlp14", "head"])
def test_gpu_fqe_clipped_steps_match_the_clipped_fqe_oracle(case):
    def pair():
        oracle, eng = GC.make_pair(case)
        table = oracle_table(oracle, eng)
        return to_fqe(oracle, table), eng, table

    oracle, eng, _ = pair()
    GC.drop(eng)
    norms = []
    for _ in range(STEPS):
        rec, _, _ = GC.oracle_step(oracle, None)
        norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for g in rec.grads.values()))))
    max_norm = float(np.median(norms))
    oracle, eng, table = pair()
    keep = set_table(eng, table)
    eng.set_grad_clip(max_norm)
    clipped, loose = 0, {}
    for step in range(STEPS):
        rec, norm, coef = GC.oracle_step(oracle, max_norm)
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        info = eng.grad_clip_info()
        print(f"{case} step {step}: loss {eng.loss()} vs {rec.loss}; norm {info['last_norm']} vs {norm}; coef {info['last_coef']} vs {coef}")
        assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss))
        assert abs(info["last_norm"] - norm) <= 1e-5 * norm and abs(info["last_coef"] - coef) <= 1e-5
        clipped += coef < 1.0
        g = eng.param_views(eng.grads[:-1])   # DQNX_BUF_GRADS keeps the unscaled gradient
        for k, ref in rec.grads.items():
            gk = g[k].cpu()
            assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
            loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
        GE.compare_state(oracle, eng, loose=loose)
        GE.sync_oracle(oracle, eng)
    assert 0 < clipped <= STEPS
    del keep


@pytest.mark.parametrize("route", ["fused", "per_layer"])
def test_gpu_fqe_out_of_range_entry_sets_the_error_word(route):
    """An error word, not a fault: the entry is only ever used as a lane / LDS index after the range check."""
    eng = fqe_engine(route)
    bad = 123
    eng.fqe_table[bad, 1] = 8                      # n_actions = 8: one past the last action
    B = eng.batch
    ok = torch.arange(B, dtype=torch.int32, device=eng.device)
    for _ in range(2):
        eng.batch_idx.copy_(ok)
        GN.run(eng, 1, given_indices=True)
        torch.cuda.synchronize()
        eng.check_device_error()                   # the bad slot was not sampled: nothing is raised
    ref = fqe_engine(route)
    ref.fqe_table[bad, 1] = 0                      # "that row is computed with action 0"
    for _ in range(2):
        ref.batch_idx.copy_(ok)
        GN.run(ref, 1, given_indices=True)
    hit = ok.clone()
    hit[5] = bad
    for e in (eng, ref):
        e.batch_idx.copy_(hit)
        GN.run(e, 1, given_indices=True)
    torch.cuda.synchronize()
    assert int(eng.ctrl().error) == C.DEVERR_TPOL_ACTION
    with pytest.raises(RuntimeError, match="target-policy table"):
        eng.check_device_error()
    ref.check_device_error()
    assert torch.equal(eng.params, ref.params) and torch.equal(eng.td, ref.td)


@pytest.mark.parametrize("route", ["fused", "per_layer", "per"])
def test_gpu_evaluate_is_the_engines_own_rule_with_a_table_set(route):
    """evaluate() reports the engine's Double rule whether or not a table is set: the same bytes, and the per-row
    output too (the learn step's stream set changes with the table, the evaluation's does not)"""
    eng = fqe_engine(route)
    with GN.routed(eng.route_env):
        with_table = bytes(eng.evaluate_raw())
        _, rows1 = eng.evaluate(3, 77, rows=True)
        eng.set_target_policy(None)
        cleared = bytes(eng.evaluate_raw())
        _, rows0 = eng.evaluate(3, 77, rows=True)
    assert with_table == cleared and torch.equal(rows1, rows0)
    plain = GN.make_engine(route)
    with GN.routed(plain.route_env):
        assert bytes(plain.evaluate_raw()) == cleared


@pytest.mark.parametrize("route", ["fused", "per_layer"])
def test_gpu_fqe_unswept_slot_sets_the_error_word(route):
    """a sampled row whose slot the sweep never wrote holds policy_actions()'s sentinel -1: outside [0, A), so the
    error word is raised and nothing is indexed with it"""
    eng = GN.make_engine(route)
    table = eng.policy_actions(0, 200)             # slots 200 .. keep the sentinel -1
    eng.set_target_policy(table)
    pos = torch.arange(eng.batch, dtype=torch.int32, device=eng.device)
    pos[3] = 250
    eng.batch_idx.copy_(pos)
    GN.run(eng, 1, given_indices=True)
    torch.cuda.synchronize()
    assert int(eng.ctrl().error) == C.DEVERR_TPOL_ACTION
    with pytest.raises(RuntimeError, match="target-policy table"):
        eng.check_device_error()


def test_gpu_fqe_setter_refusals_on_live_engines():
    eng = GN.make_engine("fused")
    table = eng.policy_actions()
    eng.set_target_policy(table)
    with pytest.raises(RuntimeError):
        eng.set_cql_alpha(1.0)
    with pytest.raises(RuntimeError):
        eng.push(*(x[:4] for x in GN.transitions(GN.FILL, 14, 14, SEED + 100)))
    with pytest.raises(RuntimeError):
        eng.load_state_blob(eng.state_blob())
    eng.set_target_policy(None)
    eng.set_cql_alpha(1.0)
    with pytest.raises(RuntimeError):
        eng.set_target_policy(table)
    n3 = GN.make_engine("fused", n_step=3)
    with pytest.raises(RuntimeError):
        n3.set_target_policy(n3.policy_actions())


# ---- 4. fqe_value ----------------------------------------------------------------------------------------------------
def value_engine(n_env, route="mlp284"):
    """capacity 100, 130 pushed (wrapped); dones re-placed so that start rows exist on both sides of the wrap:
    logical rows 0 .. n_env-1 are starts by position, and the rows behind a done of their environment"""
    net, algo, env, kw, batch, _ = GV.ROUTES[route]
    spec, ospec = GV._specs(net)
    with GN.routed(env):
        eng = E.LearnEngine(spec, algo, batch, GV.CAP, n_env=n_env, gamma=GV.GAMMA, **kw)
    seed = GV.NET_SEED[net]
    eng.load_params(O.reference_init(ospec, seed), target=O.reference_init(ospec, seed + 1))
    obs, act, rew, done, nobs = (x.copy() for x in GV._data(net))
    done[:] = False
    # slots 99 and 0 are logical 69 and 70 (wptr = 30): a done on the last slot of the array makes slot 0 / 1 a start
    for p in (GV.PUSHED - GV.CAP + k for k in (3, 10, 11, 40, 69, 70 - n_env, 98, 99)):
        done[p] = True
    half = GV.PUSHED // 2 // n_env * n_env
    eng.push(obs[:half], act[:half], rew[:half], done[:half], nobs[:half])
    eng.push(obs[half:], act[half:], rew[half:], done[half:], nobs[half:])
    random.seed(SEED + 7)
    np.random.seed(SEED + 11)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    eng.set_rng(C.DQNX_RNG_NP, O.np_state_to_array())
    eng.route_env = env
    rows = tuple(x[GV.PUSHED - GV.CAP:] for x in (obs, act, rew, done, nobs))
    return eng, ospec, rows


@pytest.mark.parametrize("n_env", [1, 2])
@pytest.mark.parametrize("route", ["mlp284", "per_layer"])
def test_gpu_fqe_value_matches_float64(route, n_env):
    eng, ospec, (obs, act, rew, done, nobs) = value_engine(n_env, route)
    n = GV.CAP
    seed = GV.NET_SEED[GV.ROUTES[route][0]]
    online, target = O.reference_init(ospec, seed), O.reference_init(ospec, seed + 1)
    slot = (np.arange(n) + GV.PUSHED) % n
    # the table: any fixed one serves; a random one by slot
    rng = np.random.default_rng(SEED)
    tab = rng.integers(0, ospec.n_actions, size=(n, 2)).astype(np.int32)
    table = torch.from_numpy(tab).to(eng.device)
    with torch.no_grad():
        q0 = O.q_forward(ospec, online, torch.from_numpy(obs)).double().numpy()
        q2 = O.q_forward(ospec, target, torch.from_numpy(nobs)).double().numpy()
    ar = np.arange(n)
    qpi = q0[ar, tab[slot, 0]]
    y = rew.astype(np.float64) + (1.0 - done.astype(np.float64)) * float(np.float32(GV.GAMMA)) * q2[ar, tab[slot, 1]]
    delta = y - q0[ar, act]
    z = np.abs(delta)
    lb = np.where(z < 1.0, 0.5 * z * z, z - 0.5)
    start = np.array([p < n_env or bool(done[p - n_env]) for p in range(n)])
    assert start[:n_env].all() and start[70] and 1 < start.sum() < n // 2      # starts on both sides of the wrap
    blob = eng.state_blob().tobytes()
    for lo, hi in GV.RANGES + [(60, 80)]:
        with GN.routed(eng.route_env):
            d, rows = eng.fqe_value(table, lo, hi, rows=True)
            raw1 = bytes(eng.fqe_value_raw(table, lo, hi))
            raw2 = bytes(eng.fqe_value_raw(table, lo, hi))
        assert raw1 == raw2                                                     # the same bytes on a second call
        m = hi - lo
        s = start[lo:hi]
        assert d["rows"] == m and d["start_rows"] == int(s.sum())
        got = rows.cpu().numpy().astype(np.float64)
        assert np.abs(got[:, 0] - qpi[lo:hi]).max() <= 1e-5 and np.abs(got[:, 1] - delta[lo:hi]).max() <= 1e-5
        tol = m * 1e-5
        assert abs(d["q_pi_mean"] * m - qpi[lo:hi].sum()) <= tol
        assert abs(d["abs_td_mean"] * m - z[lo:hi].sum()) <= tol
        assert abs(d["loss"] * m - lb[lo:hi].sum()) <= tol
        if s.any():
            assert abs(d["value"] * s.sum() - qpi[lo:hi][s].sum()) <= tol
        else:
            assert d["value"] is None
        assert abs(d["q_pi_max"] - qpi[lo:hi].max()) <= 1e-5 and abs(d["q_pi_min"] - qpi[lo:hi].min()) <= 1e-5
    assert eng.state_blob().tobytes() == blob


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_fqe_sweeps_touch_nothing_of_the_training_state(route):
    """state blob, statistics, q / td byte-equal around both sweeps; 8 steps with sweeps in between are bitwise
    the uninterrupted ones"""
    plain = GN.make_engine(route)
    GN.run(plain, 8, stats=True)
    eng = GN.make_engine(route)
    table = None
    for step in range(8):
        GN.run(eng, 1, stats=True)
        if step % 2 == 0:
            before = (eng.state_blob().tobytes(), eng.learn_stats_view.clone(), eng.q.clone(), eng.td.clone())
            with GN.routed(eng.route_env):
                table = eng.policy_actions(out=table)
                eng.fqe_value(table, 3, eng.ring_size - 1)
            assert eng.state_blob().tobytes() == before[0] and torch.equal(eng.learn_stats_view, before[1])
            assert torch.equal(eng.q, before[2]) and torch.equal(eng.td, before[3])
    GC.assert_same(GC.snapshot(plain), GC.snapshot(eng), route)
    assert bytes(plain.learn_stats_view.cpu().numpy()) == bytes(eng.learn_stats_view.cpu().numpy())


# ---- 5. dqn.offline.fqe ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["blob", "engine"])
def test_gpu_offline_fqe_equals_the_primitive_calls(how):
    src = GN.make_engine("fused")
    GN.run(src, 2)
    _, ospec, _, _ = GN.specs("mlp14")
    policy = O.reference_init(ospec, POLICY_SEED)
    blob = src.state_blob()
    before = blob.tobytes()
    out = offline.fqe(policy, blob if how == "blob" else src, 6, seed=3, log_every=3, batch=32, lr=1e-3)
    assert src.state_blob().tobytes() == before                                 # the data engine is not changed
    # the direct sequence
    eng = offline.engine_from_state(blob, batch=32, lr=1e-3)
    eng.load_params(policy)
    table = eng.policy_actions()
    offline.fresh_fit_state(eng, 3)
    eng.set_target_policy(table)
    for _ in range(6):
        eng.learn_step(soft_update=True)
    torch.cuda.synchronize()
    eng.check_device_error()
    want = eng.fqe_value(table)
    assert set(out) == set(want) | {"log", "steps"} and out["steps"] == 6
    for k, v in want.items():
        assert out[k] == v, k                                                   # bitwise: the same floats
    assert [r["step"] for r in out["log"]] == [3, 6] and out["log"][-1]["loss"] == eng.loss()
    assert out["start_rows"] >= 1 and np.isfinite(out["value"])
    # an engine as the policy: its online network
    pe = GN.make_engine("fused", seed=POLICY_SEED)
    pe.load_params(policy)
    out2 = offline.fqe(pe, blob, 6, seed=3, batch=32, lr=1e-3)
    assert out2["log"] == [] and all(out2[k] == want[k] for k in want)
