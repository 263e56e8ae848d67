"""GPU: save and restore of the whole training state (dqnx_state_save / dqnx_state_load,
LearnEngine.save_state / load_state, Agent.save_training_state / load_training_state).

Every comparison is bitwise.  Pattern of the round trips: engine A runs, saves, runs on and records
every step; engine B is built fresh with other weights, other rows and another RNG stream, takes a
step of its own so that every region holds something else, loads A's blob and runs the same tail:
everything recorded must be equal."""
import functools
import io
import os
import random

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from oracle import ref as O
from refnets import agent_kwargs, hybrid_network_config

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def rows(obs_dim, n, seed):
    return O.synth_transitions(n, obs_dim, 8, seed=seed)


def push(eng, data, a, b):
    obs, act, rew, done, nobs = data
    if b > a:
        eng.push(obs[a:b], act[a:b], rew[a:b], done[a:b], nobs[a:b])


def seed_rng(eng, seed):
    random.seed(seed)
    np.random.seed(seed)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    eng.set_rng(C.DQNX_RNG_NP, O.np_state_to_array())


def make(net, algo, batch, cap, init_seed, **kw):
    head = O.algo_spec_head(algo)
    if net == "hybrid":
        spec, ospec = E.hybrid_spec(8, head), O.hybrid_spec(8, head)
    else:
        spec, ospec = E.mlp_spec(net, 8, head), O.mlp_spec(net, 8, head)
    eng = E.LearnEngine(spec, algo, batch, cap, **kw)
    eng.load_params(O.reference_init(ospec, init_seed))
    return eng


def step_record(eng, soft):
    eng.learn_step(soft_update=soft)
    torch.cuda.synchronize()
    return {"idx": eng.batch_idx.cpu().clone(), "loss": eng.loss(), "q": eng.q.cpu().clone(), "td": eng.td.cpu().clone()}


def final_record(eng):
    torch.cuda.synchronize()
    return {"params": eng.params.cpu().clone(), "target": eng.target_params.cpu().clone(), "m": eng.adam_m.cpu().clone(),
            "v": eng.adam_v.cpu().clone(), "ctrl": eng.ctrl_bytes.cpu().clone(), "tree": eng.sumtree.cpu().clone(),
            "np": eng.get_rng(C.DQNX_RNG_NP), "py": eng.get_rng(C.DQNX_RNG_PY),
            "mirrors": (eng.ring_size, eng.ring_wptr, eng.agent_step)}


def tail(eng, data, at, n_steps=3):
    """push 30, n_steps soft-updating steps, recorded; then the end state"""
    push(eng, data, at, at + 30)
    recs = [step_record(eng, True) for _ in range(n_steps)]
    eng.check_device_error()
    return recs, final_record(eng)


def assert_same(a, b):
    (ra, fa), (rb, fb) = a, b
    assert len(ra) == len(rb)
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert torch.equal(x["idx"], y["idx"]), f"step {i}: sampled positions differ"
        assert x["loss"] == y["loss"], (i, x["loss"], y["loss"])
        assert torch.equal(x["q"], y["q"]) and torch.equal(x["td"], y["td"]), f"step {i}: q / td differ"
    for k in ("params", "target", "m", "v", "ctrl", "tree"):
        assert torch.equal(fa[k], fb[k]), k
    assert np.array_equal(fa["np"], fb["np"]) and np.array_equal(fa["py"], fb["py"])
    assert fa["mirrors"] == fb["mirrors"]


def run_a(mk, data, fill, wrap):
    """engine A up to the save: fill, 2 steps, wrap, 2 steps -> (engine, blob)"""
    a = mk(1)
    push(a, data, 0, fill)
    seed_rng(a, 11)
    for _ in range(2):
        a.learn_step()
    push(a, data, fill, fill + wrap)
    for _ in range(2):
        a.learn_step(soft_update=True)
    blob = a.state_blob().copy()
    return a, blob


def dirty_b(mk, obs_dim, n_other):
    """engine B before the load: other weights, other rows, another stream, one step of its own"""
    b = mk(2)
    push(b, rows(obs_dim, n_other, 77), 0, n_other)
    seed_rng(b, 99)
    b.learn_step(soft_update=True)
    return b


def round_trip(mk, obs_dim, cap, fill, wrap, n_other=200):
    data = rows(obs_dim, fill + wrap + 30, 5)
    a, blob = run_a(mk, data, fill, wrap)
    info = E.inspect_state_blob(blob)
    n = min(fill + wrap, cap)
    assert (info["ring_size"], info["ring_wptr"], info["capacity"]) == (n, (fill + wrap) % cap, cap)
    assert len(blob) == a.state_bytes() == info["total_bytes"]
    at_save = (a.ring_size, a.ring_wptr, a.agent_step)
    ta = tail(a, data, fill + wrap)
    b = dirty_b(mk, obs_dim, n_other)
    b.load_state_blob(blob)
    assert (b.ring_size, b.ring_wptr, b.agent_step) == at_save
    tb = tail(b, data, fill + wrap)
    assert_same(ta, tb)
    return blob


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("algo", ["DQNAgent", "DoubleDQNAgent", "DuelingDoubleDQNAgent"])
def test_gpu_state_round_trip_mlp14(algo, graphs):
    round_trip(lambda s: make(14, algo, 32, 500, s, graphs=graphs), 14, 500, 450, 100)


@pytest.mark.parametrize("env", [{"DQNX_BWD_PLAN": "0"}, {"DQNX_BWD_PLAN": "1"},
                                 {"DQNX_DW_ADAM16": "0", "DQNX_ADAM_BLK": "1"}],
                         ids=["per_layer_plan", "bwd_plan_1", "slab_adam_blk"])
def test_gpu_state_round_trip_other_weight_copy_routes(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    round_trip(lambda s: make(14, "DuelingDoubleDQNAgent", 32, 500, s), 14, 500, 450, 100)


@pytest.mark.parametrize("numpy121", [False, True])
def test_gpu_state_round_trip_per(numpy121):
    """capacity 500 is no power of two; the tree, per_max_idx / per_min_idx, per_beta, agent_step (all
    in the control block) and the numpy stream are compared by assert_same"""
    mk = lambda s: make(14, "PerDuelingDoubleDQNAgent", 32, 500, s, per_numpy121=numpy121)   # noqa: E731
    blob = round_trip(mk, 14, 500, 450, 100)
    info = E.inspect_state_blob(blob)
    assert info["sections"]["sumtree"][1] == (2 * 500 - 1) * 8 and info["per_numpy121"] == int(numpy121)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_gpu_state_round_trip_mlp284_fused(dtype):
    round_trip(lambda s: make(284, "DuelingDoubleDQNAgent", 128, 1000, s, compute_dtype=dtype), 284, 1000, 900, 200)


def test_gpu_state_fp32_blob_into_bf16_engine_rebuilds_bf16_rows():
    """A bf16 engine gathers bf16 copies of the ring rows, which only a push writes: after loading an
    fp32 engine's blob it must step like a bf16 engine that got the same rows by the same pushes and
    the parameters, moments and control block through its views."""
    data = rows(284, 900 + 200 + 30, 5)
    a, blob = run_a(lambda s: make(284, "DuelingDoubleDQNAgent", 128, 1000, s), data, 900, 200)
    c = make(284, "DuelingDoubleDQNAgent", 128, 1000, 3, compute_dtype="bf16")
    push(c, data, 0, 900)
    push(c, data, 900, 1100)
    for dst, src in ((c.params, a.params), (c.target_params, a.target_params), (c.adam_m, a.adam_m),
                     (c.adam_v, a.adam_v), (c.ctrl_bytes, a.ctrl_bytes)):
        dst.copy_(src)
    c.params_modified()
    tc = tail(c, data, 1100)
    b = dirty_b(lambda s: make(284, "DuelingDoubleDQNAgent", 128, 1000, s, compute_dtype="bf16"), 284, 200)
    b.load_state_blob(blob)
    tb = tail(b, data, 1100)
    assert_same(tc, tb)


def test_gpu_state_round_trip_head_net():
    """hybrid_spec(): the permuted conv weight copies are derived state"""
    round_trip(lambda s: make("hybrid", "DuelingDoubleDQNAgent", 32, 300, s), 284, 300, 280, 50)


def test_gpu_state_partly_filled_ring():
    mk = lambda s: make(14, "DuelingDoubleDQNAgent", 32, 500, s)   # noqa: E731
    blob = round_trip(mk, 14, 500, 120, 0)
    full = mk(1)
    push(full, rows(14, 500, 5), 0, 500)
    # the layout: obs + next_obs rows of 14 floats, act, rew, done of 4 bytes, nothing else depends on the fill
    assert len(blob) == full.state_bytes() - (500 - 120) * (2 * 14 * 4 + 3 * 4)


def test_gpu_state_file_objects_and_paths(tmp_path):
    data = rows(14, 200, 5)
    a = make(14, "DuelingDoubleDQNAgent", 32, 500, 1)
    push(a, data, 0, 150)
    seed_rng(a, 11)
    a.learn_step()
    p = str(tmp_path / "engine.state")
    n = a.save_state(p)
    f = io.BytesIO()
    assert a.save_state(f) == n == os.path.getsize(p) and f.getvalue() == open(p, "rb").read()
    assert E.inspect_state(p)["ring_size"] == 150
    ta = tail(a, data, 150)
    b1, b2 = dirty_b(lambda s: make(14, "DuelingDoubleDQNAgent", 32, 500, s), 14, 60), make(14, "DuelingDoubleDQNAgent", 32, 500, 4)
    b1.load_state(p)
    f.seek(0)
    b2.load_state(f)
    assert_same(ta, tail(b1, data, 150))
    assert_same(ta, tail(b2, data, 150))


def _refused(fn, code):
    with pytest.raises(C.DqnxError) as ei:
        fn()
    assert ei.value.code == code, str(ei.value)
    return str(ei.value)


def test_gpu_state_refused_while_a_prefetched_minibatch_is_pending():
    data = rows(14, 200, 5)
    a = make(14, "DuelingDoubleDQNAgent", 32, 500, 1)
    push(a, data, 0, 150)
    seed_rng(a, 11)
    a.learn_step()
    blob = a.state_blob().copy()
    a.learn_step(prefetch=True)
    assert "prefetched" in _refused(a.state_blob, C.DQNX_ESTATE)
    assert "prefetched" in _refused(lambda: a.load_state_blob(blob), C.DQNX_ESTATE)
    a.learn_step()           # consumes the pending minibatch
    a.state_blob()
    a.load_state_blob(blob)


def test_gpu_state_save_refuses_a_faulted_run():
    """dqnx_ctrl.error set (here: the word written through the control-block view) is DQNX_EDEVICE"""
    a = make(14, "DuelingDoubleDQNAgent", 32, 500, 1)
    push(a, rows(14, 200, 5), 0, 150)
    seed_rng(a, 11)
    a.learn_step()
    err = a.ctrl_bytes[C.Ctrl.error.offset:C.Ctrl.error.offset + 4].view(torch.int32)
    err.fill_(C.DEVERR_EMPTY_TREE)
    assert "device error" in _refused(a.state_blob, C.DQNX_EDEVICE)
    err.zero_()
    a.state_blob()


def test_gpu_state_refused_while_an_agent_readback_is_unread(tmp_path):
    agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs("DuelingDoubleDQNAgent", 14, 32, 500, tmp_path))
    obs, act, rew, done, nobs = rows(14, 200, 5)
    for i in range(0, 40):
        agent.store_transitions(obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1], None)
    random.seed(5)
    agent.learn()            # launched; its control block comes back unread
    assert "readback" in _refused(agent.engine.state_blob, C.DQNX_ESTATE)
    agent.flush()
    blob = agent.engine.state_blob().copy()
    agent.learn()
    assert "readback" in _refused(lambda: agent.engine.load_state_blob(blob), C.DQNX_ESTATE)
    agent.flush()
    agent.engine.load_state_blob(blob)


@pytest.mark.parametrize("what,field", [("capacity", "capacity"), ("net", "obs_dim"), ("per", "algo")])
def test_gpu_state_mismatch_is_refused_and_leaves_the_engine_untouched(what, field):
    a = make(14, "DuelingDoubleDQNAgent", 32, 500, 1)
    push(a, rows(14, 200, 5), 0, 150)
    seed_rng(a, 11)
    a.learn_step()
    blob = a.state_blob().copy()
    obs_dim = 284 if what == "net" else 14
    mk = lambda: make(obs_dim, "PerDuelingDoubleDQNAgent" if what == "per" else "DuelingDoubleDQNAgent", 32,   # noqa: E731
                      512 if what == "capacity" else 500, 2)
    data = rows(obs_dim, 200, 77)
    out = []
    for loads in (True, False):   # the refusing engine and a twin that never saw the blob
        e = mk()
        push(e, data, 0, 100)
        seed_rng(e, 99)
        e.learn_step(soft_update=True)
        if loads:
            assert field in _refused(lambda: e.load_state_blob(blob), C.DQNX_EINVAL)
        out.append(tail(e, data, 100, n_steps=2))
    assert_same(out[0], out[1])


# ---- agent level ------------------------------------------------------------------------------------
def _agent_loop(agent, data, first, last, save_at=None, save=None):
    obs, act, rew, done, nobs = data
    n_env, chosen = agent.n_env, []
    for t in range(first, last + 1):
        agent.step = t
        lo = 40 + (t - 1) * n_env
        x = obs[lo:lo + n_env]
        actions = agent.choose_actions(x)
        chosen.append(list(actions))
        agent.store_transitions(x, list(actions), [float(r) for r in rew[lo:lo + n_env]],
                                [bool(d) for d in done[lo:lo + n_env]], nobs[lo:lo + n_env],
                                [{'r': float(rew[i]), 'l': i} for i in range(lo, lo + n_env)])
        agent.learn()
        agent.update_target_network()
        if t == save_at:
            save(agent)
    return chosen


def _new_agent(algo, tmp_path, torch_seed, **over):
    torch.manual_seed(torch_seed)
    agent = getattr(Agents, algo)(**agent_kwargs(algo, 14, 32, 500, tmp_path, n_env=2, save_frequency=6, **over))
    agent.epsilon_start = 0.5   # greedy and random actions
    return agent


def _agent_end(agent):
    agent.flush()
    return ({k: v.cpu().clone() for k, v in agent.online_network.state_dict().items()},
            {k: v.cpu().clone() for k, v in agent.target_network.state_dict().items()},
            random.getstate(), np.random.get_state(), agent.episode_count, list(agent.ep_info_buffer))


def _prefill(agent, data):
    obs, act, rew, done, nobs = data
    for i in range(0, 40, 2):
        agent.store_transitions(obs[i:i + 2], [int(a) for a in act[i:i + 2]], [float(r) for r in rew[i:i + 2]],
                                [bool(d) for d in done[i:i + 2]], nobs[i:i + 2], None)


@pytest.mark.parametrize("via", ["training_state", "save_model"])
@pytest.mark.parametrize("algo", ["DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"])
def test_gpu_agent_resumes_bit_exact(tmp_path, monkeypatch, algo, via):
    if via == "save_model":
        monkeypatch.setenv("DQNX_TRAIN_STATE", "1")
    data = rows(14, 40 + 12 * 2, 9)
    path = str(tmp_path / "agent.state")
    a1 = _new_agent(algo, tmp_path, 17)
    _prefill(a1, data)
    random.seed(5)
    np.random.seed(5)
    save = (lambda ag: ag.save_training_state(path)) if via == "training_state" else (lambda ag: ag.save_model())
    chosen1 = _agent_loop(a1, data, 1, 12, save_at=6, save=save)
    end1 = _agent_end(a1)

    random.seed(77)
    np.random.seed(77)
    a2 = _new_agent(algo, tmp_path, 23, load=via == "save_model")
    if via == "training_state":
        a2.load_training_state(path)
    else:
        assert os.path.exists(a1.save_path + ".state") and not os.path.exists(a1.save_path + ".state.tmp")
        a2.load_model()
        assert a2.resume_step == 6
    assert a2.step == 6 and len(a2.replay_memory_buffer.replay_buffer) == 40 + 6 * 2
    chosen2 = _agent_loop(a2, data, 7, 12)
    end2 = _agent_end(a2)
    assert chosen1[6:] == chosen2
    for d1, d2 in ((end1[0], end2[0]), (end1[1], end2[1])):
        for k in d1:
            assert torch.equal(d1[k], d2[k]), k
    assert end1[2] == end2[2]
    assert end1[3][0] == end2[3][0] and np.array_equal(end1[3][1], end2[3][1]) and end1[3][2:] == end2[3][2:]
    assert end1[4:] == end2[4:]


def test_gpu_agent_restore_rng_false_keeps_the_host_generators(tmp_path):
    data = rows(14, 40 + 12 * 2, 9)
    a1 = _new_agent("DuelingDoubleDQNAgent", tmp_path, 17)
    _prefill(a1, data)
    random.seed(5)
    np.random.seed(5)
    path = str(tmp_path / "agent.state")
    _agent_loop(a1, data, 1, 3, save_at=3, save=lambda ag: ag.save_training_state(path))
    random.seed(123)
    np.random.seed(123)
    s0, n0 = random.getstate(), np.random.get_state()
    a1.load_training_state(path, restore_rng=False)
    assert random.getstate() == s0 and np.array_equal(np.random.get_state()[1], n0[1])


def test_gpu_agent_save_model_without_the_variable_is_the_reference_checkpoint(tmp_path, monkeypatch):
    monkeypatch.delenv("DQNX_TRAIN_STATE", raising=False)
    data = rows(14, 40 + 12 * 2, 9)
    a1 = _new_agent("DuelingDoubleDQNAgent", tmp_path, 17)
    _prefill(a1, data)
    random.seed(5)
    _agent_loop(a1, data, 1, 6, save_at=6, save=lambda ag: ag.save_model())
    assert os.path.exists(a1.save_path) and not os.path.exists(a1.save_path + ".state")
    saved = {k: v.cpu().clone() for k, v in a1.online_network.state_dict().items()}
    a2 = _new_agent("DuelingDoubleDQNAgent", tmp_path, 23, load=True)
    a2.load_model()
    on, tg = a2.online_network.state_dict(), a2.target_network.state_dict()
    for k in saved:   # the weights, and the forced hard update
        assert torch.equal(on[k].cpu(), saved[k]) and torch.equal(tg[k].cpu(), saved[k]), k
    assert a2.step == a2.resume_step == 6
    assert not a2.engine.adam_m.any() and not a2.engine.adam_v.any() and a2.engine.ring_size == 0
    assert int(a2.engine.ctrl().adam_step) == 0
