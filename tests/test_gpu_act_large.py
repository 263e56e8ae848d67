"""GPU: the acting path's large route (DQNX_ACT_LARGE; csrc/act_large.hip: banded convs, dense 1 as a
split-K weight stream, its reduce, then the rest of the net) against the oracle's torch-CPU forward.

The comparison is tests/test_gpu_act.py's: values within 1e-5 (scaled by max(1, |ref|max)); actions equal
the oracle's argmax wherever the top-two gap exceeds 4x that; at least 90 % of rows that clear."""
import ctypes
import functools
import random
import time

import numpy as np
import pytest
import torch

from dqn import _capi as C
from dqn import engine as E
from dqn.network import DeepQNetwork, DuelingDeepQNetwork
from oracle import ref as O
from refnets import Box, agent_kwargs, hybrid_network_config

pytestmark = pytest.mark.gpu
TOL = 1e-5
BIG = (4, 84, 84)
ODD = (2, 45, 19)   # heights 45 -> 23 -> 12, widths 19 -> 19 -> 10; with macro_len 13 the dense input is 7,693 wide


def _flat(espec, params):
    n, layout = espec.param_infos()
    flat = torch.empty(n, dtype=torch.float32)
    for name, off, shape in layout:
        flat[off:off + int(np.prod(shape))] = params[name].reshape(-1)
    return flat.cuda()


def _check(vals, ref, acts):
    np.testing.assert_allclose(vals, ref, atol=TOL * max(1.0, float(np.abs(ref).max())), rtol=0)
    srt = np.sort(ref, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 4 * TOL * max(1.0, float(np.abs(ref).max()))
    assert np.array_equal(acts[clear], ref.argmax(axis=1)[clear])
    assert clear.mean() > 0.9


@functools.lru_cache(maxsize=None)
def _net(kind, head, dense=None):
    """(oracle spec, engine spec, oracle parameters, flat parameters on the GPU), built once per module."""
    if kind == "big":
        ospec, espec = O.hybrid_spec(8, head, micro_chw=BIG), E.hybrid_spec(8, head, micro_chw=BIG)
    elif kind == "odd":
        dn = dense or (512, 256)
        ospec = O.hybrid_spec(8, head, micro_chw=ODD, macro_len=13, dense=dn)
        espec = E.hybrid_spec(8, head, micro_chw=ODD, macro_len=13, dense=dn)
    elif kind == "head":
        ospec, espec = O.hybrid_spec(8, head), E.hybrid_spec(8, head)
    else:
        ospec, espec = O.mlp_spec(int(kind), 8, head), E.mlp_spec(int(kind), 8, head)
    params = O.reference_init(ospec, 7)
    return ospec, espec, params, _flat(espec, params)


@functools.lru_cache(maxsize=None)
def _rows(kind, head, dense, n):
    ospec, _, params, _ = _net(kind, head, dense)
    x = torch.from_numpy(O.synth_transitions(n, ospec.obs_dim, 8, seed=n)[0])
    with torch.no_grad():
        ref = (O.advantages(ospec, params, x) if head == "dueling" else O.q_forward(ospec, params, x)).numpy()
    return x, ref


def _act(espec, flat, x, scratch=None):
    n = x.shape[0]
    vals = torch.empty(n, 8, dtype=torch.float32, device="cuda")
    acts = E.act(espec, flat, x.cuda(), vals, scratch=scratch)
    torch.cuda.synchronize()
    return vals.cpu().numpy(), acts.cpu().numpy()


def _against_oracle(kind, head, n, dense=None):
    _, espec, _, flat = _net(kind, head, dense)
    x, ref = _rows(kind, head, dense, n)
    vals, acts = _act(espec, flat, x)
    _check(vals, ref, acts)
    return vals


@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("n", [1, 3])
def test_gpu_act_large_84(monkeypatch, head, n):
    """The (4,84,84) net: 56,462-wide dense 1, conv images of up to 903 KB a row."""
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _against_oracle("big", head, n)


@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("n", [1, 2, 5, 9])
def test_gpu_act_large_odd_grid(monkeypatch, head, n):
    """The smallest net refused for its conv input: odd image sizes under stride 2, a band count that does
    not divide Ho, an odd K (weight rows 4-byte aligned, each peeled on its own), a micro grid 13 floats
    into the row; 9 rows cross the 8-row chunk."""
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _against_oracle("odd", head, n)


@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("n", [1, 5])
def test_gpu_act_large_one_dense_layer(monkeypatch, head, n):
    """L = 1: the head runs straight on the reduced dense 1."""
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _against_oracle("odd", head, n, dense=(256,))


@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_gpu_act_large_wide_mlp(monkeypatch, head, n):
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _against_oracle("9001", head, n)


@pytest.mark.parametrize("kind,n", [("head", 1), ("head", 2), ("head", 3), ("head", 8), ("head", 37),
                                    ("284", 1), ("284", 3)])
@pytest.mark.parametrize("head", ["dueling", "linear"])
def test_gpu_act_large_forced_on_nets_that_fit(monkeypatch, kind, head, n):
    """DQNX_ACT_LARGE=2 on the HEAD net (K = 1,358: 8-byte aligned rows) and MLP-284: the oracle, and the
    LDS-resident route's values on the same rows (both within 1e-5 of the oracle: 2e-5 apart at most)."""
    monkeypatch.delenv("DQNX_ACT_LARGE", raising=False)
    _, espec, _, flat = _net(kind, head)
    x, ref = _rows(kind, head, None, n)
    base, _ = _act(espec, flat, x)
    monkeypatch.setenv("DQNX_ACT_LARGE", "2")
    vals = _against_oracle(kind, head, n)
    np.testing.assert_allclose(vals, base, atol=2 * TOL * max(1.0, float(np.abs(ref).max())), rtol=0)


def test_gpu_act_large_shared_scratch_and_determinism(monkeypatch):
    """One scratch sized for 16 rows serves calls of 16, 1, 3, 16, 2 rows; a repeated call is bitwise equal."""
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _, espec, _, flat = _net("odd", "dueling")
    scratch = E.act_scratch(espec, 16, "cuda")
    for n in (16, 1, 3, 16, 2):
        x, ref = _rows("odd", "dueling", None, n)
        vals, acts = _act(espec, flat, x, scratch=scratch)
        _check(vals, ref, acts)
        again, acts2 = _act(espec, flat, x, scratch=scratch)
        assert np.array_equal(vals.view(np.uint32), again.view(np.uint32))
        assert np.array_equal(acts, acts2)


@pytest.mark.parametrize("n", [1, 3, 9])
def test_gpu_act_large_host_call(monkeypatch, n):
    """dqnx_act_host on the large route: staged obs, launches, actions copied back, one stream
    synchronisation -- no poll for a completion word the route never stores."""
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    _, espec, _, flat = _net("odd", "dueling")
    desc = espec.to_c()
    L = C.lib()
    nb = int(L.dqnx_act_host_scratch_bytes(ctypes.byref(desc), n))
    assert nb > 0
    scratch = torch.zeros((nb + 15) // 16 * 4, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    xt, _ = _rows("odd", "dueling", None, n)
    x = np.ascontiguousarray(xt.numpy())
    out = np.full(n, -1, dtype=np.int32)
    args = (ctypes.byref(desc), flat.data_ptr(), x.ctypes.data, n, out.ctypes.data, scratch.data_ptr(),
            scratch.numel() * 4, stream)
    C.check(L.dqnx_act_host(*args), "act_host")
    _, acts = _act(espec, flat, xt)
    assert np.array_equal(out, acts), (out, acts)
    t0 = time.perf_counter()
    for _ in range(20):
        C.check(L.dqnx_act_host(*args), "act_host")
    assert time.perf_counter() - t0 < 0.4, "act_host waited for a completion word its launch never stores"
    assert np.array_equal(out, acts)


@pytest.mark.parametrize("cls", [DeepQNetwork, DuelingDeepQNetwork])
def test_gpu_act_large_standalone_network(monkeypatch, cls):
    conf = functools.partial(hybrid_network_config, micro_chw=BIG)
    obs_dim = 14 + 4 * 84 * 84
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    torch.manual_seed(5)
    net = cls("cuda:0", 1e-4, conf, Box(obs_dim), 8)
    x = O.synth_transitions(3, obs_dim, 8, seed=2)[0]
    xt = torch.from_numpy(x).cuda()
    assert net._native_act() is not None
    with torch.no_grad():
        q = (net.advantages(xt) if cls is DuelingDeepQNetwork else net(xt)).cpu().numpy()
    got = net.actions(x)
    srt = np.sort(q, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 1e-4
    assert clear.any()
    assert np.array_equal(np.asarray(got)[clear], q.argmax(1)[clear])
    del net
    monkeypatch.delenv("DQNX_ACT_LARGE")
    torch.manual_seed(5)
    fresh = cls("cuda:0", 1e-4, conf, Box(obs_dim), 8)
    assert fresh._native_act() is None


def test_gpu_act_large_agent(monkeypatch, tmp_path):
    """choose_actions of an agent on the (4,84,84) net is one dqnx_agent_choose call on the large route:
    the torch forward's argmax at epsilon 0, two MT words per env, and the post-step weights after learn()."""
    from dqn import agent as Agents
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    obs_dim, batch, seed = 14 + 4 * 84 * 84, 32, 17
    conf = functools.partial(hybrid_network_config, micro_chw=BIG)
    torch.manual_seed(seed)
    agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs("DuelingDoubleDQNAgent", obs_dim, batch, 64, tmp_path,
                                                        nn_conf_func=conf, epsilon_start=0.0, epsilon_min=0.0))
    obs, act, rew, done, nobs = O.synth_transitions(48, obs_dim, 8, seed=seed)
    for i in range(40):
        agent.store_transitions(obs[i:i + 1], [int(act[i])], [float(rew[i])], [bool(done[i])], nobs[i:i + 1], None)
    random.seed(seed)
    np.random.seed(seed)

    def greedy(x):
        with torch.no_grad():
            q = agent.online_network.advantages(torch.from_numpy(x).cuda()).cpu().numpy()
        srt = np.sort(q, axis=1)
        return q.argmax(1), (srt[:, -1] - srt[:, -2]) > 1e-4

    def choose_and_check(x):
        twin = random.Random()
        twin.setstate(random.getstate())
        got = np.asarray(agent.choose_actions(x))
        assert agent._choose_cache is not None   # (the one-call path, not the method-by-method one)
        for _ in range(len(x)):
            twin.random()
        assert random.getstate() == twin.getstate()
        want, clear = greedy(x)
        assert clear.any()
        assert np.array_equal(got[clear], want[clear])

    choose_and_check(obs[40:41])
    choose_and_check(obs[41:43])
    agent.learn()
    choose_and_check(obs[43:44])
