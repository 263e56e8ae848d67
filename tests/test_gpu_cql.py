"""The CQL(H) regulariser of the head kernels (include/dqnx.h "conservative Q-learning") on the GPU: off is the
step of an engine that never set it; on, every learn route matches an oracle whose loss carries
alpha * mean(logsumexp_a Q(s, a) - Q(s, a_b)); the step forms, clipping, n-step returns, shards, the state
blob, dqn.offline and the drop-in Agent compose with it.

The parity reference is CqlOracle below: oracle.ref.OracleLearner with learn() restated and the one term added.
The pairs come from the existing tests' builders; their oracle is re-classed in place (to_cql)."""
import copy
import functools
import random
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from dqn import offline
from oracle import ref as O
from parity import assert_grad_close
from refnets import agent_kwargs
import test_gpu_bf16 as GB
import test_gpu_engine as GE
import test_gpu_grad_clip as GC
import test_gpu_hybrid as GH
import test_gpu_nstep as GN
import test_gpu_per as GP

pytestmark = pytest.mark.gpu

ALPHA, SEED, FILL, CAP, STEPS = 1.0, 11, 400, 500, 4
DDQN, PER = "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"


# ---- the oracle -------------------------------------------------------------------------------------------
class CqlOracle(O.OracleLearner):
    """OracleLearner whose loss is L_TD + alpha * mean_b(logsumexp_a Q(s_b, a) - Q(s_b, a_b)); under PER the
    term is not importance-weighted and the priorities stay the TD error's; under shard= the slice's sum
    is divided by B.  learn() restates the parent's; rec.gap is the batch mean of the bracket."""
    alpha = ALPHA

    def learn(self, shard=None):
        rec = O.StepRecord()
        B = self.batch_size
        if self.per:
            is_w, idxs, transitions = self.replay.sample_transitions(self.step * self.n_env, self.np_state)
            rec.positions = np.asarray(idxs, dtype=np.int64)
            rec.is_weights = np.asarray(is_w, dtype=np.float64)
            is_weights_t = torch.as_tensor(np.asarray(is_w), dtype=torch.float32).unsqueeze(-1)
        else:
            transitions, pos = self.replay.sample_transitions(self.py_state)
            rec.positions = pos
        obses_t, actions_t, rews_t, dones_t, new_obses_t = O.transitions_to_tensor(transitions)
        with torch.no_grad():
            if self.algo == "DQNAgent":
                tq = self._q(self.target, new_obses_t)
                rec.q_target_next = tq
                sel = tq.max(dim=1, keepdim=True)[0]
            else:
                oq = self._q(self.online, new_obses_t)
                rec.q_online_next = oq
                best = oq.argmax(dim=1, keepdim=True)
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
        gap = torch.logsumexp(q, 1, keepdim=True) - qa
        if shard is None:
            loss = loss + self.alpha * gap.mean()
        else:
            loss = loss + self.alpha * (gap[shard[0]:shard[1]].sum() / B)
        rec.gap = float(gap.detach().mean())
        rec.loss = float(loss.item())
        grads = torch.autograd.grad(loss, list(params.values()))
        rec.grads = OrderedDict(zip(params.keys(), [g.detach() for g in grads]))
        if shard is None:
            self.apply_grads(rec.grads)
        return rec


def to_cql(oracle, alpha=ALPHA):
    oracle.__class__ = CqlOracle
    oracle.alpha = alpha
    return oracle


def grad_tol(ref):
    """assert_grad_close's bound (tests/parity.py), per element"""
    ref = np.asarray(ref, np.float64)
    return 2e-6 + 1e-4 * np.abs(ref) + 5e-4 * (float(np.abs(ref).max()) if ref.size else 0.0)


def assert_not_vacuous(oracle):
    """On the two oracles alone, from the pair's state, step 0: the alpha = 1 loss differs from the alpha = 0
    loss by more than 1e-3 and some tensor's gradient by more than 10 x assert_grad_close's tolerance
    (not every tensor: fc_val's is unchanged under the dueling head, sum_j (p_j - onehot) = 0)."""
    o1, o0 = copy.deepcopy(oracle), to_cql(copy.deepcopy(oracle), 0.0)
    r1, r0 = o1.learn(), o0.learn()
    assert abs(r1.loss - r0.loss) > 1e-3, (r1.loss, r0.loss)
    over = {k: float((np.abs(r1.grads[k].numpy() - r0.grads[k].numpy()) / grad_tol(r0.grads[k].numpy())).max())
            for k in r0.grads}
    print("alpha 1 vs 0: loss", r1.loss, r0.loss, "max |dg| / tol", over)
    assert max(over.values()) > 10.0, over


def check_step(oracle, eng, rec, step, loose):
    """one step against the CQL oracle's record (test_gpu_engine._check_learn's assertions, the PER test's
    tree assertions, cql_gap), then the oracle continues from the engine's state"""
    torch.cuda.synchronize()
    eng.check_device_error()
    per, cap = oracle.per, eng.capacity
    idx = eng.batch_idx.cpu().numpy().astype(np.int64) + (cap - 1 if per else 0)
    assert np.array_equal(idx, rec.positions), f"step {step}: sampled positions differ"
    q = eng.q.cpu()
    np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(q[2].numpy(), rec.q_target_next.numpy(), atol=1e-5, rtol=0)
    if rec.q_online_next is not None:
        np.testing.assert_allclose(q[1].numpy(), rec.q_online_next.numpy(), atol=1e-5, rtol=0)
    np.testing.assert_allclose(eng.td[0].cpu().numpy(), rec.targets.view(-1).numpy(), atol=1e-5, rtol=0)
    gap = eng.cql_gap()
    print(f"step {step}: loss {eng.loss()} vs {rec.loss}; gap {gap} vs {rec.gap}")
    assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss)), (step, eng.loss(), rec.loss)
    assert abs(gap - rec.gap) <= 1e-5, (step, gap, rec.gap)
    g = eng.param_views(eng.grads[:-1])
    for k, ref in rec.grads.items():
        gk = g[k].cpu()
        assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
        loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
    GE.compare_state(oracle, eng, loose=loose)
    if per:   # the regulariser left the priorities alone: the tree is the TD error's, as the PER test asserts it
        np.testing.assert_allclose(eng.is_weights.cpu().numpy(), rec.is_weights.astype(np.float32),
                                   rtol=2e-7 if step == 0 else 1e-5)
        np.testing.assert_allclose(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1), atol=1e-5, rtol=0)
        same = np.array_equal(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1).astype(np.float32))
        oracle.tree_exact = getattr(oracle, "tree_exact", True) and same
        GP.assert_tree_equal(eng, oracle.replay.replay_buffer, exact=oracle.tree_exact)
    GE.sync_oracle(oracle, eng)


# ---- 1. off is the parent's step ---------------------------------------------------------------------------
def test_gpu_cql_off_is_bitwise_the_default_step():
    e1 = GN.make_engine("fused", cql_alpha=ALPHA)
    assert e1.cql_alpha == ALPHA and e1.cql_gap() is None
    e1.set_cql_alpha(0)
    e0 = GN.make_engine("fused")
    assert e0.cql_alpha == 0.0 == e1.cql_alpha
    for step in range(3):
        GN.run(e0, 1)
        GN.run(e1, 1)
        torch.cuda.synchronize()
        for a, b in ((e0.params, e1.params), (e0.target_params, e1.target_params), (e0.adam_m, e1.adam_m),
                     (e0.adam_v, e1.adam_v), (e0.grads, e1.grads), (e0.q, e1.q), (e0.td, e1.td)):
            assert torch.equal(a, b), step
        assert np.float32(e0.loss()).tobytes() == np.float32(e1.loss()).tobytes()
        assert np.array_equal(e0.get_rng(0), e1.get_rng(0)) and np.array_equal(e0.get_rng(1), e1.get_rng(1))
    e0.check_device_error()
    e1.check_device_error()
    assert GN.kernel_names(e0) == GN.kernel_names(GN.make_engine("fused", cql_alpha=ALPHA))   # and on: the same launches


# ---- 2. parity with the CQL oracle --------------------------------------------------------------------------
PARITY = {   # name: (pair builder, routing environment)
    "mlp14": (lambda: GE.make_pair(DDQN, 14, 32, CAP, FILL, SEED, graphs=False), {}),
    "mlp14_b40": (lambda: GE.make_pair(DDQN, 14, 40, CAP, FILL, SEED, graphs=False), {}),   # last tile: 8 real rows
    "linear14": (lambda: GE.make_pair("DQNAgent", 14, 32, CAP, FILL, SEED, graphs=False), {}),
    "mlp14_slab": (lambda: GE.make_pair(DDQN, 14, 32, CAP, FILL, SEED, graphs=False), {"DQNX_DW_ADAM16": "0"}),
    "mlp14_per_layer": (lambda: GE.make_pair(DDQN, 14, 32, CAP, FILL, SEED, graphs=False), {"DQNX_BWD_PLAN": "0"}),   # k_head
    "head": (lambda: GH.make_hybrid_pair(DDQN, 32, CAP, FILL, SEED), {}),                                             # k_head, ELU
    "per284": (lambda: GP.make_per_pair(284, 64, CAP, FILL, SEED, graphs=False), {}),
}


@pytest.mark.parametrize("route", list(PARITY))
def test_gpu_cql_steps_match_the_cql_oracle(monkeypatch, route):
    build, env = PARITY[route]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    oracle, eng = build()
    to_cql(oracle)
    assert_not_vacuous(oracle)
    eng.set_cql_alpha(ALPHA)
    loose = {}
    for step in range(STEPS):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        check_step(oracle, eng, rec, step, loose)
    assert np.array_equal(eng.get_rng(1 if oracle.per else 0), oracle.np_state if oracle.per else oracle.py_state)


def width_pair(head, A):
    """obs 14, default hidden widths, A actions"""
    algo = DDQN if head == "dueling" else "DQNAgent"
    ospec = O.mlp_spec(14, A, head)
    init = O.reference_init(ospec, SEED)
    oracle = to_cql(O.OracleLearner(ospec, algo, 32, CAP, seed=SEED, params=init))
    data = O.synth_transitions(FILL, 14, A, seed=SEED + 100)
    assert int(np.max(data[1])) == A - 1 and int(np.min(data[1])) == 0
    O.fill_replay(oracle, *data)
    eng = E.LearnEngine(E.mlp_spec(14, A, head), algo, 32, CAP, cql_alpha=ALPHA)
    eng.load_params(init)
    eng.push(*data)
    random.seed(SEED + 7)
    st = O.py_state_to_array()
    oracle.py_state = st.copy()
    eng.set_rng(0, st)
    return oracle, eng


@pytest.mark.parametrize("head,A", [("dueling", 15), ("linear", 16), ("linear", 1)])
def test_gpu_cql_head_widths_match_the_cql_oracle(head, A):
    """dueling A = 15 fills all 16 head slots, linear A = 16 too; A = 1: logsumexp is the only Q, the term vanishes"""
    oracle, eng = width_pair(head, A)
    if A > 1:
        assert_not_vacuous(oracle)
    else:
        r0 = to_cql(copy.deepcopy(oracle), 0.0).learn()
    rec = oracle.train_step()
    eng.learn_step(soft_update=True)
    check_step(oracle, eng, rec, 0, {})
    if A == 1:
        assert abs(rec.gap) <= 1e-6 and eng.cql_gap() == 0.0
        g = eng.param_views(eng.grads[:-1])
        for k, ref in r0.grads.items():
            assert_grad_close(g[k].cpu().numpy(), ref.numpy(), f"{k} against the alpha = 0 step")


def test_gpu_cql_bf16_matches_the_bf16_cql_oracle():
    """mlp284, B = 64, against the oracle's bf16 emulation with test_gpu_bf16's tolerances.  cql_gap: logsumexp
    and the gather are both 1-Lipschitz in max |dQ|, so the batch mean moves by at most 2 Q_ATOL."""
    emu, _, eng = GB.make_bf16_pair(DDQN, 284, 64, CAP, FILL, SEED, graphs=False)
    to_cql(emu)
    assert_not_vacuous(emu)
    eng.set_cql_alpha(ALPHA)
    for step in range(STEPS):
        rec = emu.train_step()
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        GB._check_step(eng, rec, None, step)
        GB._compare_weights(emu, eng)
        print(f"step {step}: gap {eng.cql_gap()} vs {rec.gap}")
        assert abs(eng.cql_gap() - rec.gap) <= 2 * GB.Q_ATOL
        GE.sync_oracle(emu, eng)
    assert np.array_equal(eng.get_rng(0), emu.py_state)


# ---- 3. compositions with CQL on: bitwise the sequential steps ---------------------------------------------------
COMPOSE = ["fused", "per_layer", "head", "per"]   # k_head_bwd, k_head (ReLU), k_head (ELU), PER


@functools.lru_cache(maxsize=None)
def sequential(route, steps=STEPS):
    eng = GN.make_engine(route, cql_alpha=ALPHA)
    GN.run(eng, steps)
    snap = GC.snapshot(eng)
    if steps == STEPS:   # the regulariser is in these steps: another trajectory than alpha = 0
        off = GN.make_engine(route)
        GN.run(off, steps)
        assert GC.snapshot(off)["params"] != snap["params"]
    return snap


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_cql_learn_steps_equal_single_steps(route):
    eng = GN.make_engine(route, cql_alpha=ALPHA)
    with GN.routed(eng.route_env):
        eng.learn_steps(8, soft_update=True)
    GC.assert_same(sequential(route, 8), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_cql_prefetch_loop_equals_sequential_steps(route):
    eng = GN.make_engine(route, cql_alpha=ALPHA)
    GN.run(eng, STEPS - 1, prefetch=True)
    GN.run(eng, 1)   # consumes the pending minibatch
    GC.assert_same(sequential(route), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_cql_graphs_on_equals_off(route):
    eng = GN.make_engine(route, cql_alpha=ALPHA, graphs=True)
    GN.run(eng, STEPS)
    GC.assert_same(sequential(route), GC.snapshot(eng), route)
    # a new alpha reaches the replayed graphs: the cached plans are dropped
    eng.set_cql_alpha(0)
    off = GN.make_engine(route, graphs=True)
    off.load_state_blob(eng.state_blob())
    GN.run(eng, 1)
    GN.run(off, 1)
    GC.assert_same(GC.snapshot(off), GC.snapshot(eng), route + " after alpha = 0")


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_cql_grads_only_plus_apply_equals_the_step(route):
    eng = GN.make_engine(route, cql_alpha=ALPHA)
    with GN.routed(eng.route_env):
        for _ in range(STEPS):
            eng.learn_step(grads_only=True)
            eng.apply_grads(soft_update=True)
    GC.assert_same(sequential(route), GC.snapshot(eng), route)


@pytest.mark.parametrize("route", COMPOSE)
def test_gpu_cql_with_stats_changes_nothing_else(route):
    """and loss_sum is the sum of the TOTAL losses (dqnx_ctrl.loss reports the total)"""
    eng = GN.make_engine(route, cql_alpha=ALPHA)
    total = 0.0
    for _ in range(STEPS):
        GN.run(eng, 1, stats=True)
        total += float(np.float32(eng.loss()))
    GC.assert_same(sequential(route), GC.snapshot(eng), route)
    st = eng.learn_stats()
    assert st["steps"] == STEPS and abs(st["loss_sum"] - total) <= 1e-9 * max(1.0, abs(total))
    assert total > STEPS * 1.0   # ~ln 8 per step from the regulariser alone at these weights


@functools.lru_cache(maxsize=None)
def cql_median_norm(case):
    """test_gpu_grad_clip.median_norm with the CQL oracle: the median of its unclipped global norms over
    STEPS steps, with the same conditions on the clipped oracle run"""
    oracle, eng = GC.make_pair(case)
    GC.drop(eng)
    to_cql(oracle)
    norms = []
    for _ in range(STEPS):
        rec, _, _ = GC.oracle_step(oracle, None)
        norms.append(float(torch.sqrt(sum((g.double() ** 2).sum() for g in rec.grads.values()))))
    max_norm = float(np.median(norms))
    oracle, eng = GC.make_pair(case)
    GC.drop(eng)
    to_cql(oracle)
    seen = [GC.oracle_step(oracle, max_norm)[1:] for _ in range(STEPS)]
    assert any(c < 1.0 for _, c in seen) and any(c == 1.0 for _, c in seen), seen
    assert all(abs(n - max_norm) > 1e-3 * max_norm for n, _ in seen), (seen, max_norm)
    return max_norm


@pytest.mark.parametrize("case", ["mlp14", "head"])
def test_gpu_cql_clipped_steps_match_the_clipped_cql_oracle(case):
    max_norm = cql_median_norm(case)
    oracle, eng = GC.make_pair(case)
    to_cql(oracle)
    eng.set_cql_alpha(ALPHA)
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
        assert abs(eng.cql_gap() - rec.gap) <= 1e-5
        clipped += coef < 1.0
        g = eng.param_views(eng.grads[:-1])   # DQNX_BUF_GRADS keeps the unscaled gradient
        for k, ref in rec.grads.items():
            gk = g[k].cpu()
            assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
            loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
        GE.compare_state(oracle, eng, loose=loose)
        GE.sync_oracle(oracle, eng)
    assert 0 < clipped < STEPS and eng.grad_clip_info()["clipped_steps"] == clipped


def test_gpu_cql_on_top_of_n_step_matches_the_wrapped_cql_oracle():
    oracle, eng, seen, _ = GN.make_pair("fused", 3, 1)
    to_cql(oracle)
    eng.set_cql_alpha(ALPHA)
    loose = {}
    for step in range(STEPS):
        oracle.step = step
        rec = oracle.train_step()
        GN.run(eng, 1)
        torch.cuda.synchronize()
        assert abs(eng.cql_gap() - rec.gap) <= 1e-5
        GN.check_step(oracle, eng, rec, step, loose, False)
    assert ("full",) in seen and any(k[0] == "done" for k in seen)


# ---- 4. shards -----------------------------------------------------------------------------------------------
def test_gpu_cql_shards_sum_to_the_global_batch():
    ospec = O.mlp_spec(14, 8, "dueling")
    init = O.reference_init(ospec, SEED)
    data = O.synth_transitions(FILL, 14, 8, seed=SEED + 100)
    pos = torch.from_numpy(np.random.default_rng(SEED).permutation(FILL)[:32].astype(np.int32))

    def step(world, rank, alpha=ALPHA):
        eng = E.LearnEngine(E.mlp_spec(14, 8, "dueling"), DDQN, 32, CAP, world_size=world, rank=rank, cql_alpha=alpha)
        eng.load_params(init)
        eng.push(*data)
        eng.batch_idx.copy_(pos)
        eng.learn_step(given_indices=True, grads_only=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        return eng.grads.cpu().numpy().astype(np.float64), eng

    whole, e1 = step(1, 0)
    parts = [step(2, r)[0] for r in (0, 1)]
    both = parts[0] + parts[1]
    P = e1.n_params
    views = lambda flat: {k: flat[o:o + int(np.prod(s))] for k, o, s in e1.param_layout}   # noqa: E731
    got, want = views(both[:P]), views(whole[:P])
    for k in want:
        assert_grad_close(got[k], want[k], k)
    assert abs(both[P] - whole[P]) <= 1e-5, (parts[0][P], parts[1][P], whole[P])   # the loss slot: two shares
    assert min(parts[0][P], parts[1][P]) > 0.5   # each carries its half of ~ln 8
    plain, _ = step(1, 0, alpha=None)
    assert abs(whole[P] - plain[P]) > 1e-3       # (the term is in these steps)


# ---- 5. state ------------------------------------------------------------------------------------------------
def test_gpu_cql_alpha_is_not_state():
    a = GN.make_engine("fused", cql_alpha=ALPHA)
    GN.run(a, 2)
    blob1 = a.state_blob().tobytes()
    a.set_cql_alpha(0)
    blob0 = a.state_blob().tobytes()
    assert blob1 == blob0
    a.set_cql_alpha(ALPHA)
    b = GN.make_engine("fused", seed=SEED + 1)   # a fresh engine with other weights and streams
    b.set_cql_alpha(ALPHA)
    b.load_state_blob(blob1)
    assert b.cql_alpha == ALPHA                  # the load leaves configuration alone
    GN.run(a, 3)
    GN.run(b, 3)
    GC.assert_same(GC.snapshot(a), GC.snapshot(b), "continuation")
    assert torch.equal(a.q, b.q) and torch.equal(a.td, b.td) and a.cql_gap() == b.cql_gap()


# ---- 6. the offline module -------------------------------------------------------------------------------------
def test_gpu_offline_fit_equals_the_direct_loop(tmp_path):
    a = GN.make_engine("fused")
    GN.run(a, 3)
    path = str(tmp_path / "run.dqnx")
    a.save_state(path)
    eng = offline.engine_from_state(path, batch=32)
    assert eng.spec == a.spec and eng.capacity == CAP and eng.batch == 32 and eng.cql_alpha == 0.0
    eng.set_cql_alpha(ALPHA)
    log = offline.fit(eng, steps=6, log_every=2)
    direct = E.LearnEngine(E.mlp_spec(14, 8, "dueling"), DDQN, 32, CAP)
    direct.load_state(path)
    direct.set_cql_alpha(ALPHA)
    for _ in range(6):
        direct.learn_step(soft_update=True)
    GC.assert_same(GC.snapshot(direct), GC.snapshot(eng), "offline.fit")
    assert torch.equal(direct.q, eng.q) and torch.equal(direct.td, eng.td)
    assert [r["step"] for r in log] == [2, 4, 6]
    for r in log:
        assert set(r) == {"step", "loss", "cql_gap", "q_sa_mean"}
        assert np.isfinite(r["loss"]) and np.isfinite(r["q_sa_mean"]) and np.isfinite(r["cql_gap"]) and r["cql_gap"] >= 0
    assert log[-1]["loss"] == direct.loss() and log[-1]["cql_gap"] == direct.cql_gap()
    assert offline.fit(eng, steps=1) == []       # log_every = 0: no record, no read
    # a prioritised blob gives a prioritised engine
    p = GN.make_engine("per")
    GN.run(p, 1)
    pe = offline.engine_from_state(p.state_blob(), batch=64, cql_alpha=0.5)
    assert pe.cfg.algo == C.DQNX_ALGO_PER_DOUBLE and pe.cql_alpha == 0.5 and pe.spec == p.spec
    assert torch.equal(pe.sumtree, p.sumtree)


# ---- 7. the drop-in Agent --------------------------------------------------------------------------------------
def _agent_run(tmp_path, how):
    tmp_path.mkdir(parents=True, exist_ok=True)
    torch.manual_seed(SEED)
    agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs(DDQN, 14, 32, CAP, tmp_path, log_frequency=2))
    if how == "method":
        assert agent.engine.cql_alpha == 0.0
        agent.set_cql_alpha(ALPHA)
    obs, act, rew, done, nobs = O.synth_transitions(100, 14, 8, seed=SEED + 100)
    for i in range(100):
        agent.store_transitions(obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1], None)
    seen = {}
    agent.summary_writer.add_scalar = lambda tag, v, global_step=None: seen.__setitem__(tag, v)
    random.seed(SEED + 7)
    np.random.seed(SEED + 7)
    for t in range(3):
        agent.step = t
        agent.learn()
        agent.update_target_network()
        agent.flush()
        agent.log()
    torch.cuda.synchronize()
    eng = agent.engine
    snap = {"params": eng.params.cpu().numpy().tobytes(), "target": eng.target_params.cpu().numpy().tobytes(),
            "m": eng.adam_m.cpu().numpy().tobytes(), "v": eng.adam_v.cpu().numpy().tobytes(),
            "loss": np.float32(eng.loss()).tobytes(), "rng": random.getstate()}
    return agent, seen, snap


def test_gpu_agent_cql_from_the_environment_equals_the_method(tmp_path, monkeypatch):
    monkeypatch.setenv("DQNX_CQL_ALPHA", "1")
    a_env, seen_env, s_env = _agent_run(tmp_path / "env", "env")
    assert a_env.engine.cql_alpha == 1.0
    monkeypatch.delenv("DQNX_CQL_ALPHA")
    a_m, seen_m, s_m = _agent_run(tmp_path / "method", "method")
    assert s_env == s_m
    for seen, agent in ((seen_env, a_env), (seen_m, a_m)):
        assert set(seen) == GC.GS.TODAY_TAGS | {"CQLGap"}
        assert seen["CQLGap"] > 0 and np.isfinite(seen["CQLGap"])
    a_off, seen_off, s_off = _agent_run(tmp_path / "off", "env")   # the variable is gone: today's agent
    assert a_off.engine.cql_alpha == 0.0 and set(seen_off) == GC.GS.TODAY_TAGS
    assert s_off["params"] != s_env["params"]
