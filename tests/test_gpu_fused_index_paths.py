"""GPU: the index paths of the fused MLP step (k_mlp_fwd's gather and tile mapping, k_head_bwd's
tile mapping, k_dw_adam16's tile -> layer mapping) at the smallest shapes where they can go wrong:
batches of 16, 17 and 1020 rows (one tile, a ragged second tile, a ragged last tile of many with
the XCD-aligned mapping), rows of 14 and 284 columns (4 and 72 gather pieces a row), 3 and 8
actions, dueling and linear heads, one to three dense layers.

Every case is checked against the oracle at the suite's tolerances (tests/parity.py,
test_gpu_engine.compare_state), with and without the soft update, and bit for bit across routes
the engine already offers: 16 x 16 against 32 x 16 weight-gradient tiles (DQNX_DW16_R=1),
xcd_remap's order against the XCD-aligned row tiles (DQNX_XCD_ROWS=0), eager against graph
launches, each with and without the in-launch prefetch; and the gradient-only step + apply_grads
against the one-call step, with and without clipping."""
import random

import numpy as np
import pytest
import torch

from oracle import ref as O
from parity import assert_grad_close
import test_gpu_engine as GE

pytestmark = pytest.mark.gpu

# (algo -> head, obs_dim, actions, hidden, batch)
CASES = [
    ("DoubleDQNAgent", 14, 3, (64,), 16),
    ("DuelingDoubleDQNAgent", 284, 8, (256, 128), 17),
    ("DuelingDoubleDQNAgent", 284, 3, (256, 128, 64), 1020),
    ("DQNAgent", 14, 8, (128, 64), 1020),
    ("DoubleDQNAgent", 284, 8, (64,), 17),
    ("DuelingDoubleDQNAgent", 14, 3, (256, 128, 64), 16),
]
IDS = [f"{c[0][:-5]}-o{c[1]}-a{c[2]}-l{len(c[3])}-b{c[4]}" for c in CASES]
STATE = ("q", "td", "grads", "params", "target_params", "adam_m", "adam_v")


def make_pair(case, seed, graphs=False, oracle=True):
    algo, obs_dim, A, hidden, batch = case
    E = GE._engine_mod()
    head = O.algo_spec_head(algo)
    ospec = O.mlp_spec(obs_dim, A, head, hidden)
    init = O.reference_init(ospec, seed)
    n_fill = capacity = 2048
    orc = O.OracleLearner(ospec, algo, batch, capacity, seed=seed, params=init) if oracle else None
    data = O.synth_transitions(n_fill, obs_dim, A, seed=seed + 100)
    if orc is not None:
        O.fill_replay(orc, *data)
    eng = E.LearnEngine(E.mlp_spec(obs_dim, A, head, hidden), algo, batch, capacity, graphs=graphs)
    eng.load_params(init)
    eng.push(*data)
    random.seed(seed + 7)
    st = O.py_state_to_array()
    if orc is not None:
        orc.py_state = st.copy()
    eng.set_rng(0, st)
    return orc, eng


@pytest.mark.parametrize("soft", [True, False], ids=["soft", "nosoft"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_index_paths_match_oracle(case, soft):
    oracle, eng = make_pair(case, 31)
    loose = {}
    for step in range(2):
        rec = oracle.learn()
        if soft:
            oracle.update_target_network()
        oracle.step += 1
        eng.learn_step(soft_update=soft)
        torch.cuda.synchronize()
        eng.check_device_error()
        assert np.array_equal(eng.batch_idx.cpu().numpy().astype(np.int64), rec.positions)
        q = eng.q.cpu()
        np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=0)
        np.testing.assert_allclose(q[2].numpy(), rec.q_target_next.numpy(), atol=1e-5, rtol=0)
        if rec.q_online_next is not None:
            np.testing.assert_allclose(q[1].numpy(), rec.q_online_next.numpy(), atol=1e-5, rtol=0)
        np.testing.assert_allclose(eng.td[0].cpu().numpy(), rec.targets.view(-1).numpy(), atol=1e-5, rtol=0)
        assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss))
        g = eng.param_views(eng.grads[:-1])
        for k, ref in rec.grads.items():
            gk = g[k].cpu()
            assert_grad_close(gk.numpy(), ref.numpy(), f"{k} step {step}")
            loose[k] = (gk - ref).abs() > 1e-3 * ref.abs() + 1e-9
        GE.compare_state(oracle, eng, loose=loose)
        GE.sync_oracle(oracle, eng)
    assert np.array_equal(eng.get_rng(0), oracle.py_state)


def _run(case, prefetch, graphs=False):
    _, eng = make_pair(case, 47, graphs=graphs, oracle=False)
    for i in range(3):
        eng.learn_step(soft_update=True, prefetch=prefetch and i < 2)
    torch.cuda.synchronize()
    eng.check_device_error()
    return {k: getattr(eng, k).clone() for k in STATE}


@pytest.mark.parametrize("prefetch", [False, True], ids=["noprefetch", "prefetch"])
@pytest.mark.parametrize("route", ["DQNX_DW16_R=1", "DQNX_XCD_ROWS=0", "graph"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_index_paths_routes_bit_identical(monkeypatch, case, route, prefetch):
    if route == "graph":
        other = _run(case, prefetch, graphs=True)
    else:
        monkeypatch.setenv(*route.split("="))
        other = _run(case, prefetch)
        monkeypatch.delenv(route.split("=")[0])
    base = _run(case, prefetch)
    for k in STATE:
        assert torch.equal(base[k], other[k]), k


@pytest.mark.parametrize("clip", [None, 0.05], ids=["noclip", "clip"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gpu_index_paths_grads_then_apply_equals_step(case, clip):
    out = []
    for split in (False, True):
        _, eng = make_pair(case, 53, oracle=False)
        if clip is not None:
            eng.set_grad_clip(clip)
        for _ in range(2):
            if split:
                eng.learn_step(grads_only=True)
                eng.apply_grads(soft_update=True)
            else:
                eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        out.append({k: getattr(eng, k).clone() for k in STATE if k != "grads"})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k
