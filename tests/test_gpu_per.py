"""GPU parity of prioritised replay (PerDuelingDoubleDQNAgent): device SumTree pushes,
ordered priority updates (incl. max/min rescans), stratified sampling + IS weights, and the
full PER learn step, through the C ABI, against the oracle (R:dqn/replay_memory.py:43-98,
R:dqn/utils/sum_tree.py, R:dqn/agent.py:245-272).

The oracle runs with pow_mode="cr" (correctly rounded float32 power, as libdqnx and glibc
powf compute it); the golden fixture was made by the reference under this host's numpy
(SVML power, within 1 ulp), so that comparison carries a tolerance on the tree."""
import os
import random

import numpy as np
import pytest
import torch

from golden_io import load_fixture
from oracle import ref as O
from parity import assert_grad_close

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALGO = "PerDuelingDoubleDQNAgent"


def _E():
    from dqn import engine as E
    return E


def tree_state(eng):
    c = eng.ctrl()
    return eng.sumtree.cpu().numpy(), int(c.per_max_idx), int(c.per_min_idx)


def assert_tree_equal(eng, st: O.SumTree, exact=True):
    tree, mx, mn = tree_state(eng)
    if exact:
        bad = np.nonzero(tree != st.tree)[0]
        assert bad.size == 0, f"{bad.size} tree nodes differ, first {bad[:5]}: {tree[bad[:5]]} vs {st.tree[bad[:5]]}"
    else:   # priorities from |delta| that agree to ~1e-6: d(p)/d|delta| <= 0.6 * 1e-4^-0.4 = 24
        np.testing.assert_allclose(tree, st.tree, rtol=1e-6, atol=1e-4)
    assert mx == st.max_priority_index and mn == st.min_priority_index, (mx, mn, st.max_priority_index,
                                                                         st.min_priority_index)


def per_engine(obs_dim, batch, cap, graphs=True, numpy121=False):
    E = _E()
    return E.LearnEngine(E.mlp_spec(obs_dim, 8, "dueling"), ALGO, batch, cap, graphs=graphs, per_numpy121=numpy121)


def test_gpu_per_push_matches_sumtree_add():
    cap = 500
    eng = per_engine(14, 32, cap)
    rep = O.PerReplay(cap, 32, 2e6, "cr")
    obs, act, rew, done, new_obs = O.synth_transitions(1300, 14, 8, seed=5)
    o = 0
    for n in (1, 37, 300, 362, 1, 599):   # wraps the ring twice
        sl = slice(o, o + n)
        eng.push(obs[sl], act[sl], rew[sl], done[sl], new_obs[sl])
        list(rep.store_transitions(obs[sl], act[sl], rew[sl], done[sl], new_obs[sl]))
        o += n
        torch.cuda.synchronize()
        assert_tree_equal(eng, rep.replay_buffer)
        assert eng.ctrl().ring_size == rep.replay_buffer.size


@pytest.mark.parametrize("cap,fill,n,rounds", [(500, 300, 64, 40), (20000, 20000, 5000, 3), (20000, 20000, 8192, 2),
                                               (30000, 30000, 12000, 2)])
def test_gpu_per_priority_updates_match_sequential_semantics(cap, fill, n, rounds):
    """Batches with duplicate leaves, the max leaf lowered and the min leaf raised (the
    argmax / argmin rescans), and more updates than one launch takes."""
    eng = per_engine(14, 32, cap)
    rep = O.PerReplay(cap, 32, 2e6, "cr")
    data = O.synth_transitions(fill, 14, 8, seed=6)
    eng.push(*data)
    list(rep.store_transitions(*data))
    rng = np.random.default_rng(7)
    st = rep.replay_buffer
    for r in range(rounds):
        slots = rng.integers(0, fill, size=n).astype(np.int32)
        slots[rng.integers(0, n, size=n // 8)] = slots[0]                   # duplicates
        absd = (rng.random(n).astype(np.float32) * np.float32(3.0)) ** 3
        absd[rng.random(n) < 0.1] = np.float32(0.0)
        k = rng.integers(0, n, size=3)
        slots[k[0]] = st.max_priority_index - (cap - 1)                     # lower the max leaf
        absd[k[0]] = np.float32(1e-3)
        slots[k[1]] = st.min_priority_index - (cap - 1)                     # raise the min leaf
        absd[k[1]] = np.float32(5.0)
        eng.per_update_priorities(torch.from_numpy(slots), torch.from_numpy(absd))
        rep.update_batch_priorities((slots.astype(np.int64) + cap - 1).tolist(), absd.reshape(-1, 1))
        torch.cuda.synchronize()
        assert_tree_equal(eng, st)


@pytest.mark.parametrize("cap,fill,B", [(3000, 2500, 256), (100000, 90000, 8192), (200000, 150000, 5000)])
def test_gpu_per_sample_matches_oracle(cap, fill, B):
    """One sampling workgroup (B <= 1024) and several (each walks the MT twists, the last to
    arrive writes the state back); trees deeper than the LDS-cached top 13 levels."""
    eng = per_engine(14, B, cap)
    rep = O.PerReplay(cap, B, 2e6, "cr")
    data = O.synth_transitions(fill, 14, 8, seed=8)
    eng.push(*data)
    list(rep.store_transitions(*data))
    rng = np.random.default_rng(9)
    nu = min(fill, 20000)
    slots = rng.integers(0, fill, size=nu).astype(np.int32)
    absd = rng.random(nu).astype(np.float32) * np.float32(2.0)
    eng.per_update_priorities(torch.from_numpy(slots), torch.from_numpy(absd))
    rep.update_batch_priorities((slots.astype(np.int64) + cap - 1).tolist(), absd.reshape(-1, 1))
    np.random.seed(10)
    nps = O.np_state_to_array()
    eng.set_rng(1, nps)
    for step in (0, 12345, 3_000_000):
        eng.set_agent_step(step)
        eng.per_sample()
        isw, leaves, _ = rep.sample_transitions(step, nps)
        torch.cuda.synchronize()
        eng.check_device_error()
        got = eng.batch_idx.cpu().numpy().astype(np.int64) + cap - 1
        assert np.array_equal(got, np.asarray(leaves)), f"step {step}: leaves differ"
        np.testing.assert_allclose(eng.is_weights.cpu().numpy(), np.asarray(isw, dtype=np.float32), rtol=2e-7, atol=0)
        assert np.array_equal(eng.get_rng(1), nps)
        assert abs(eng.ctrl().per_beta - rep.beta(step)) == 0.0
        assert eng.ctrl().agent_step == step + 1


def make_per_pair(obs_dim, batch, cap, n_fill, seed, graphs=True):
    E = _E()
    ospec = O.mlp_spec(obs_dim, 8, "dueling")
    init = O.reference_init(ospec, seed)
    oracle = O.OracleLearner(ospec, ALGO, batch, cap, seed=seed, params=init, per_pow="cr")
    data = O.synth_transitions(n_fill, obs_dim, 8, seed=seed + 100)
    O.fill_replay(oracle, *data)
    eng = E.LearnEngine(E.mlp_spec(obs_dim, 8, "dueling"), ALGO, batch, cap, graphs=graphs)
    eng.load_params(init)
    eng.push(*data)
    np.random.seed(seed + 11)
    nps = O.np_state_to_array()
    oracle.np_state = nps.copy()
    eng.set_rng(1, nps)
    return oracle, eng


@pytest.mark.parametrize("obs_dim,batch,cap,n_fill,seed", [
    (14, 32, 500, 300, 3),
    (284, 256, 5000, 3000, 4),
    (284, 1024, 20000, 20000, 5),
])
def test_gpu_per_learn_matches_oracle(obs_dim, batch, cap, n_fill, seed):
    oracle, eng = make_per_pair(obs_dim, batch, cap, n_fill, seed)
    for step in range(3):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        leaves = eng.batch_idx.cpu().numpy().astype(np.int64) + cap - 1
        assert np.array_equal(leaves, rec.positions), f"step {step}: sampled leaves differ"
        # IS weights depend on leaf priorities from earlier steps' |delta| (two devices, ~1e-6)
        np.testing.assert_allclose(eng.is_weights.cpu().numpy(), rec.is_weights.astype(np.float32),
                                   rtol=2e-7 if step == 0 else 1e-5)
        np.testing.assert_allclose(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1), atol=1e-5, rtol=0)
        q = eng.q.cpu()
        np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=0)
        assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss))
        g = eng.param_views(eng.grads[:-1])
        for k, ref in rec.grads.items():
            assert_grad_close(g[k].cpu().numpy(), ref.numpy(), k)
        # the tree follows |delta| computed on two devices: equal when the fp32 |delta| agree
        same = np.array_equal(eng.per_abs_td.cpu().numpy(), rec.abs_td.reshape(-1).astype(np.float32))
        assert_tree_equal(eng, oracle.replay.replay_buffer, exact=same)
        from test_gpu_engine import compare_state
        compare_state(oracle, eng)
    assert np.array_equal(eng.get_rng(1), oracle.np_state)


def test_gpu_per_learn_golden():
    """Against the reference's own PER steps (tests/golden, made by make_golden.py)."""
    z = load_fixture(os.path.join(GOLDEN, "learn_mlp284_PerDuelingDoubleDQNAgent.npz"))
    obs_dim, batch, cap = int(z["obs_dim"]), int(z["batch"]), int(z["buffer"])
    init = O.reference_init(O.mlp_spec(obs_dim, 8, "dueling"), int(z["seed"]))
    eng = per_engine(obs_dim, batch, cap)
    eng.load_params(init)
    eng.push(*O.synth_transitions(int(z["n_fill"]), obs_dim, 8, seed=int(z["seed"]) + 100))
    eng.set_rng(1, z["np_state_in"])
    for s in range(int(z["steps"])):
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        assert np.array_equal(eng.batch_idx.cpu().numpy().astype(np.int64) + cap - 1, z["pos"][s])
        np.testing.assert_allclose(eng.is_weights.cpu().numpy(), z["isw"][s].astype(np.float32), rtol=1e-6)
        assert abs(eng.loss() - z["loss"][s]) <= 1e-5 * max(1.0, abs(z["loss"][s]))
    assert np.array_equal(eng.get_rng(1), z["np_state_out"])
    tree, mx, mn = tree_state(eng)
    np.testing.assert_allclose(tree, z["tree"], rtol=1e-6, atol=1e-4)   # SVML powf (1 ulp) + |delta| 1e-6
    assert mx == int(z["tree_max_idx"]) and mn == int(z["tree_min_idx"])
    keys = [str(k) for k in z["keys"]]
    on = eng.param_views(eng.params)
    for i, k in enumerate(keys):
        np.testing.assert_allclose(on[k].cpu().numpy().reshape(-1), z[f"online_{i}"], atol=1e-5, rtol=0)


def test_gpu_per_graph_and_eager_identical():
    o1, e1 = make_per_pair(284, 256, 3000, 3000, 31, graphs=True)
    o2, e2 = make_per_pair(284, 256, 3000, 3000, 31, graphs=False)
    for _ in range(4):
        e1.learn_step(soft_update=True)
        e2.learn_step(soft_update=True)
    torch.cuda.synchronize()
    assert torch.equal(e1.params, e2.params)
    assert torch.equal(e1.sumtree, e2.sumtree)


@pytest.mark.parametrize("cap,fill,n,rounds", [(500, 300, 64, 40), (20000, 20000, 5000, 3), (30000, 30000, 12000, 2)])
def test_gpu_per_numpy121_updates_match_float32_semantics(cap, fill, n, rounds):
    """per_numpy121: update_batch_priorities with the reference's pinned numpy 1.21 arithmetic
    (float32 `change`, float32-rounded ancestor sums, in update order; oracle SumTree(numpy121))
    -- duplicates, rescans, pushes between rounds (float64 under both versions), chunked
    launches; the tree compared with ==.  The numpy >= 2 tree differs from it (checked), so the
    mode is not a no-op."""
    eng = per_engine(14, 32, cap, numpy121=True)
    rep = O.PerReplay(cap, 32, 2e6, "cr", numpy121=True)
    ref2 = O.PerReplay(cap, 32, 2e6, "cr")
    data = O.synth_transitions(fill, 14, 8, seed=16)
    eng.push(*data)
    list(rep.store_transitions(*data))
    list(ref2.store_transitions(*data))
    rng = np.random.default_rng(17)
    st = rep.replay_buffer
    for r in range(rounds):
        slots = rng.integers(0, fill, size=n).astype(np.int32)
        slots[rng.integers(0, n, size=n // 8)] = slots[0]                   # duplicates
        absd = (rng.random(n).astype(np.float32) * np.float32(3.0)) ** 3
        k = rng.integers(0, n, size=2)
        slots[k[0]] = st.max_priority_index - (cap - 1)                     # lower the max leaf
        absd[k[0]] = np.float32(1e-3)
        slots[k[1]] = st.min_priority_index - (cap - 1)                     # raise the min leaf
        absd[k[1]] = np.float32(5.0)
        eng.per_update_priorities(torch.from_numpy(slots), torch.from_numpy(absd))
        idx = (slots.astype(np.int64) + cap - 1).tolist()
        rep.update_batch_priorities(idx, absd.reshape(-1, 1))
        ref2.update_batch_priorities(idx, absd.reshape(-1, 1))
        torch.cuda.synchronize()
        assert_tree_equal(eng, st)
        if r == 0:
            extra = O.synth_transitions(17, 14, 8, seed=100 + r)               # a push between rounds
            eng.push(*extra)
            list(rep.store_transitions(*extra))
            list(ref2.store_transitions(*extra))
            torch.cuda.synchronize()
            assert_tree_equal(eng, st)
    assert not np.array_equal(st.tree, ref2.replay_buffer.tree)


def test_gpu_per_numpy121_learn_steps_match_oracle():
    """PerDuelingDoubleDQNAgent learn steps in numpy 1.21 mode against the oracle in the same
    mode: sampled leaves (the descent reads the float32-rounded sums), IS weights through the
    loss, the tree after every step's priority update."""
    E = _E()
    cap, fill, batch, seed = 3000, 2500, 256, 23
    spec = O.mlp_spec(14, 8, "dueling")
    init = O.reference_init(spec, seed)
    oracle = O.OracleLearner(spec, ALGO, batch, cap, seed=seed, params=init, per_pow="cr", per_numpy121=True)
    data = O.synth_transitions(fill, 14, 8, seed=seed + 100)
    O.fill_replay(oracle, *data)
    eng = E.LearnEngine(E.mlp_spec(14, 8, "dueling"), ALGO, batch, cap, per_numpy121=True)
    eng.load_params(init)
    eng.push(*data)
    import random
    random.seed(seed + 7)
    st = O.py_state_to_array()
    oracle.py_state = st.copy()
    eng.set_rng(0, st)
    np.random.seed(seed + 11)
    nps = O.np_state_to_array()
    oracle.np_state = nps.copy()
    eng.set_rng(1, nps)
    for step in range(4):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        assert np.array_equal(eng.batch_idx.cpu().numpy().astype(np.int64) + cap - 1, rec.positions), step
        assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss))
        assert_tree_equal(eng, oracle.replay.replay_buffer, exact=False)


@pytest.mark.parametrize("batch,cap", [(256, 5000), (1024, 20000), (8192, 40000)])
def test_gpu_per_np_cache_bit_identical(monkeypatch, batch, cap):
    """The numpy MT block cache (the next PER sample's blocks twisted ahead by one workgroup of the
    forward launch) gives the same leaves, IS weights, RNG state, tree and weights as twisting in
    the sampler (DQNX_NO_NP_CACHE=1), across learn steps and after the host replaces the state."""
    monkeypatch.setenv("DQNX_NO_NP_CACHE", "1")
    _, e1 = make_per_pair(284, batch, cap, cap, 91)
    monkeypatch.delenv("DQNX_NO_NP_CACHE")
    _, e2 = make_per_pair(284, batch, cap, cap, 91)
    for rnd in range(2):
        for _ in range(4):
            e1.learn_step(soft_update=True)
            e2.learn_step(soft_update=True)
        torch.cuda.synchronize()
        e1.check_device_error()
        e2.check_device_error()
        assert torch.equal(e1.batch_idx, e2.batch_idx), rnd
        assert torch.equal(e1.is_weights, e2.is_weights), rnd
        assert np.array_equal(e1.get_rng(1), e2.get_rng(1)), rnd
        assert torch.equal(e1.sumtree, e2.sumtree), rnd
        assert torch.equal(e1.params, e2.params) and torch.equal(e1.target_params, e2.target_params), rnd
        np.random.seed(500 + rnd)   # a new state from the host: the cache no longer matches
        st = O.np_state_to_array()
        if rnd == 0:
            st[624] = 624            # ... and one whose next word needs a twist
        e1.set_rng(1, st)
        e2.set_rng(1, st)


@pytest.mark.parametrize("batch,compute,cap,world,dw16", [
    (1024, "fp32", 20000, 1, None), (8192, "bf16", 40000, 1, None), (300, "fp32", 2000, 1, None),
    (2048, "fp32", 9000, 1, None), (2048, "fp32", 2500, 1, None), (512, "bf16", 1500, 1, None),
    (4096, "fp32", 6000, 1, "1"), (8192, "bf16", 40000, 8, None), (1024, "fp32", 20000, 2, None)])
def test_gpu_per_fused_update_bit_identical(monkeypatch, batch, compute, cap, world, dw16):
    """The single-GPU PER step with the SumTree update spread over the launches that run anyway (the
    head kernel does k_per_prep's work per sample, the gradient launch runs k_per_prop's workgroups
    beside its tiles; the default) against the three update launches (DQNX_PER_FUSED=0): the same
    leaves, tree, tracked max / min indices, IS weights, sampled indices and weights, bitwise, over
    several steps (each step samples from the tree the previous one updated).  world > 1: rank 0's
    GRADS_ONLY step + dqnx_apply_grads, whose Adam launch runs k_per_prop's workgroups.  Three
    modes: the three launches, prep / prop fused with the tracking launch kept
    (DQNX_PER_TRACK_INLAUNCH=0), and the default with the tracking workgroup in the gradient launch
    (k_dw_adam16: its prop workgroups wait for it in the same launch; k_dw_bf16: the Adam launch
    runs the prop).  Small trees against large batches (cap 2500 / 1500) resample the tracked max /
    min leaves, so the rescans run; B=4096 on k_dw_adam16 (DQNX_DW_ADAM16=1) and B=8192 on k_dw_bf16
    take the tracking in several super-chunks."""
    E = _E()
    ospec = O.mlp_spec(284, 8, "dueling")
    init = O.reference_init(ospec, 63)
    data = O.synth_transitions(cap, 284, 8, seed=163)
    if dw16:
        monkeypatch.setenv("DQNX_DW_ADAM16", dw16)
    runs = []
    for fused, track in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("DQNX_PER_FUSED", fused)
        monkeypatch.setenv("DQNX_PER_TRACK_INLAUNCH", track)
        eng = E.LearnEngine(E.mlp_spec(284, 8, "dueling"), ALGO, batch, cap, compute_dtype=compute,
                            world_size=world, rank=0)
        eng.load_params(init)
        eng.push(*data)
        np.random.seed(64)
        eng.set_rng(1, O.np_state_to_array())
        for t in range(4):
            eng.set_agent_step(t)
            if world > 1:
                eng.learn_step(grads_only=True)
                eng.apply_grads(soft_update=True)
            else:
                eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        runs.append((eng, tree_state(eng)))
    e0, (t0, mx0, mn0) = runs[0]
    for mode, (e1, (t1, mx1, mn1)) in enumerate(runs[1:], 1):
        assert np.array_equal(t0, t1) and mx0 == mx1 and mn0 == mn1, mode
        assert torch.equal(e0.batch_idx, e1.batch_idx) and torch.equal(e0.is_weights, e1.is_weights), mode
        assert torch.equal(e0.params, e1.params) and torch.equal(e0.target_params, e1.target_params), mode


PER_LONG = ["learn_mlp284long1024_PerDuelingDoubleDQNAgent", "learn_mlp284long8192_PerDuelingDoubleDQNAgent"]


@pytest.mark.parametrize("golden", PER_LONG)
def test_gpu_per_long_golden(golden):
    """The reference's own 8-step prioritised runs (tests/golden, make_golden.py mlp284long1024 /
    mlp284long8192: B = 1024 and configs[4]'s B = 8192, fp32, full SumTree kept): every step's sampled
    leaves compared with ==, the numpy RNG state after the run with ==, the final tree's max / min leaf
    indices with ==.  The tree VALUES are compared to 1e-4 (leaves: 2e-6 absolute): libdqnx's |delta| comes from its own
    fp32 forward (summation order differs from torch CPU by ~1e-7 relative), so the float32 priorities
    it writes may differ by an ulp from the reference's, and the IS weights fed back through the
    training carry that on (the oracle with the correctly rounded power drifts as far from the same
    run: tests/test_oracle.py::test_oracle_per_long_tree_and_cr_pow).  R:dqn/replay_memory.py:69-98."""
    from dqn import engine as E
    z = np.load(os.path.join(GOLDEN, golden + ".npz"))
    assert bool(z["tree_full"])
    batch, cap, seed = int(z["batch"]), int(z["buffer"]), int(z["seed"])
    spec = O.mlp_spec(int(z["obs_dim"]), 8, "dueling")
    eng = E.LearnEngine(E.mlp_spec(int(z["obs_dim"]), 8, "dueling"), ALGO, batch, cap)
    eng.load_params(O.reference_init(spec, seed))
    eng.push(*O.synth_transitions(int(z["n_fill"]), int(z["obs_dim"]), 8, seed=seed + 100))
    eng.set_rng(0, z["py_state_in"])
    eng.set_rng(1, z["np_state_in"])
    moved, dloss, disw = [], [], []
    for s in range(int(z["steps"])):
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        got = eng.batch_idx.cpu().numpy().astype(np.int64) + cap - 1
        moved.append(int((got != z["pos"][s]).sum()))
        dloss.append(abs(eng.loss() - z["loss"][s]) / max(1.0, abs(z["loss"][s])))
        disw.append(float(np.max(np.abs(eng.is_weights.cpu().numpy() / z["isw"][s].astype(np.float32) - 1))))
    assert moved == [0] * int(z["steps"]), f"sampled leaves differing from the reference run, per step: {moved}"
    # the IS-weighted loss and the IS weights share the factor (size * p_min / total)^beta, and p_min comes
    # from the smallest |delta| of the run, whose fp32 forward noise dp/d|delta| (<= 24) amplifies: after
    # several steps they agree to ~1e-4 (the correctly rounded power alone moves them by <= 2e-7 against
    # this run, tests/test_oracle.py); step 0 (the pushed max priorities) is held to 1e-5
    assert dloss[0] <= 1e-5 and max(dloss) <= 2e-4, f"relative loss differences per step: {dloss}"
    assert disw[0] <= 1e-6 and max(disw) <= 2e-4, f"IS weight differences per step: {disw}"
    assert np.array_equal(eng.get_rng(1), z["np_state_out"])
    tree, mx, mn = tree_state(eng)
    assert (mx, mn) == (int(z["tree_max_idx"]), int(z["tree_min_idx"]))
    # a leaf's priority (|delta| + 1e-4)^0.6 <= 1 moves with its |delta|, which agrees with the reference's
    # to the forward's fp32 noise (~1e-6 absolute): leaves within 2e-6 absolute, the sums within 1e-4
    np.testing.assert_allclose(tree, z["tree"], rtol=1e-4, atol=2e-6)
