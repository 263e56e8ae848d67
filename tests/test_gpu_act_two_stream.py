"""GPU: the two-stream (HEAD) network's acting path with the conv stack as ONE launch (k_act_conv_stack,
csrc/act_hybrid.hip) followed by the MLP acting kernel, against the oracle's torch-CPU forward
(R:env/dqn_config.py:66-143 body, R:dqn/network.py:67-74 / 110-117 argmax) and against the per-conv
launches (DQNX_ACT_TS=0); dqnx_act_host's in-place pinned path with its completion word; and
Agent.choose_actions as one dqnx_agent_choose call for a HEAD-net agent.

Geometries (micro_chw / macro_len -> dense input width): the reference's (1358, width % 4 = 2), an odd
height under stride 2 (9 -> 5 -> 3; 390), an aligned width (272: the float4 branches of the MLP kernel),
and the smallest grid that survives both strides (last conv 1 x 2 pixels: every padding bound active).
Row counts: one row; R = 2; a partial group of R = 4; two groups with the second partial (no completion
word); many groups.

Tolerance: the project's TOL = 1e-5 scaled by max(1, |ref|max) (tests/test_gpu_act.py).  With these
parameters (reference_init seed 31) and observations (synth_transitions seed 200 + n) every row's
top-two gap in the oracle exceeds 4 TOL max(1, |ref|max) for all four geometries, both heads and n in
{1, 2, 3, 5, 8, 37, 64} (smallest: 4.6e-5 at (2,3,3) linear n = 64, threshold 4e-5), so the tests assert
that all rows are clear and compare every action."""
import ctypes
import functools
import random
import time

import numpy as np
import pytest
import torch

from dqn import Agents
from dqn import _capi as C
from dqn import engine as E
from oracle import ref as O
from refnets import agent_kwargs, hybrid_network_config

pytestmark = pytest.mark.gpu
TOL = 1e-5
GEOMS = [((2, 27, 5), 14), ((2, 9, 4), 6), ((2, 8, 4), 16), ((2, 3, 3), 2)]
GEOM_IDS = ["2x27x5+14", "2x9x4+6", "2x8x4+16", "2x3x3+2"]
ROWS = [1, 2, 3, 5, 8, 37]


@functools.lru_cache(maxsize=None)
def _net(geom, head):
    chw, ml = geom
    ospec = O.hybrid_spec(8, head, micro_chw=chw, macro_len=ml)
    espec = E.hybrid_spec(8, head, micro_chw=chw, macro_len=ml)
    params = O.reference_init(ospec, 31)
    n, layout = espec.param_infos()
    flat = torch.empty(n, dtype=torch.float32)
    for name, off, shape in layout:
        flat[off:off + int(np.prod(shape))] = params[name].reshape(-1)
    return ospec, espec, params, flat.cuda()


@functools.lru_cache(maxsize=None)
def _case(geom, head, n, shift=0.0):
    """(obs, oracle values, scale) of one case: computed once, shared by the tests, never modified."""
    ospec, _, params, _ = _net(geom, head)
    x = O.synth_transitions(n, ospec.obs_dim, 8, seed=200 + n, macro_len=geom[1])[0]
    x = np.ascontiguousarray(x, dtype=np.float32) + np.float32(shift)
    with torch.no_grad():
        xt = torch.from_numpy(x)
        ref = (O.advantages(ospec, params, xt) if head == "dueling" else O.q_forward(ospec, params, xt)).numpy()
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref, max(1.0, float(np.abs(ref).max()))


def _all_clear(ref, scale):
    srt = np.sort(ref, axis=1)
    return bool(((srt[:, -1] - srt[:, -2]) > 4 * TOL * scale).all())


def _act(espec, flat, x, scratch=None):
    n = x.shape[0]
    vals = torch.empty(n, 8, dtype=torch.float32, device="cuda")
    acts = E.act(espec, flat, torch.from_numpy(np.array(x)).cuda(), vals, scratch=scratch)
    torch.cuda.synchronize()
    return acts.cpu().numpy(), vals.cpu().numpy()


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_gpu_act_two_stream_stack_matches_oracle(monkeypatch, geom, head, n):
    monkeypatch.setenv("DQNX_ACT_TS", "2")   # the stack at every n (the default takes it where it measured faster)
    _, espec, _, flat = _net(geom, head)
    x, ref, scale = _case(geom, head, n)
    k = C.I32(0)
    C.check(C.lib().dqnx_act_kernel_count(ctypes.byref(espec.to_c()), n, ctypes.byref(k)), "act_kernel_count")
    assert k.value == 2   # the route under test: conv stack + MLP kernel
    acts, vals = _act(espec, flat, x)
    print(f"max |values - oracle| = {np.abs(vals - ref).max():.3e} (bound {TOL * scale:.3e})")
    np.testing.assert_allclose(vals, ref, atol=TOL * scale, rtol=0)
    assert _all_clear(ref, scale)
    assert np.array_equal(acts, ref.argmax(axis=1))


@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("head", ["dueling", "linear"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_gpu_act_two_stream_both_routes(monkeypatch, geom, head, n):
    """The per-conv launches (DQNX_ACT_TS=0) and the one-launch stack: equal actions, values within 2 TOL
    (each is within TOL of the oracle); the stack's values are bitwise reproducible, also after calls with
    other row counts on the same scratch (fixed summation order, tickets back at zero)."""
    _, espec, _, flat = _net(geom, head)
    x, ref, scale = _case(geom, head, n)
    scratch = E.act_scratch(espec, 64, "cuda")
    monkeypatch.setenv("DQNX_ACT_TS", "0")
    acts0, vals0 = _act(espec, flat, x, scratch)
    monkeypatch.setenv("DQNX_ACT_TS", "2")
    acts1, vals1 = _act(espec, flat, x, scratch)
    print(f"max |stack - per-conv| = {np.abs(vals1 - vals0).max():.3e} (bound {2 * TOL * scale:.3e})")
    assert np.array_equal(acts0, acts1)
    np.testing.assert_allclose(vals1, vals0, atol=2 * TOL * scale, rtol=0)
    acts2, vals2 = _act(espec, flat, x, scratch)
    assert np.array_equal(vals1, vals2) and np.array_equal(acts1, acts2)
    for m in (64, 3 if n != 3 else 2):
        xm, refm, scm = _case(geom, head, m)
        am, _ = _act(espec, flat, xm, scratch)
        assert _all_clear(refm, scm) and np.array_equal(am, refm.argmax(axis=1)), m
    acts3, vals3 = _act(espec, flat, x, scratch)
    assert np.array_equal(vals1, vals3) and np.array_equal(acts1, acts3)


@pytest.mark.parametrize("n", [1, 5])
def test_gpu_act_two_stream_stack_other_windows(monkeypatch, n):
    """Windows other than the reference's 3 x 3 (1 x 3, 5 x 3, 3 x 1: the stack kernel's run-time-window
    loops) against torch's conv2d / linear on the same flat parameters.  Values within TOL max(1, |ref|max);
    actions where the reference's top-two gap is clear of 4 TOL (random parameters: ties are possible)."""
    import torch.nn.functional as F
    monkeypatch.setenv("DQNX_ACT_TS", "2")
    conv = ((8, (1, 3), (1, 1)), (16, (5, 3), (2, 1)), (16, (3, 1), (2, 2)))
    chw, ml = (2, 9, 4), 6
    espec = E.hybrid_spec(8, "linear", micro_chw=chw, macro_len=ml, conv=conv, dense=(64, 32))
    k = C.I32(0)
    C.check(C.lib().dqnx_act_kernel_count(ctypes.byref(espec.to_c()), n, ctypes.byref(k)), "act_kernel_count")
    assert k.value == 2
    n_params, layout = espec.param_infos()
    g = torch.Generator().manual_seed(11)
    flat = torch.randn(n_params, generator=g) * 0.1
    it = iter([flat[off:off + int(np.prod(s))].view(*s) for _, off, s in layout])
    x = torch.rand(n, espec.obs_dim, generator=g)
    with torch.no_grad():
        h = x[:, ml:].reshape(n, *chw)
        for f, (kh, kw), (sh, sw) in conv:
            W, b = next(it), next(it)
            assert W.shape == (f, h.shape[1], kh, kw)
            h = F.elu(F.conv2d(h, W, b, stride=(sh, sw), padding=(kh // 2, kw // 2)))
        h = torch.cat([h.flatten(1), x[:, :ml]], dim=1)
        for _ in range(2):
            W, b = next(it), next(it)
            h = F.elu(F.linear(h, W, b))
        W, b = next(it), next(it)
        ref = F.linear(h, W, b).numpy()
    acts, vals = _act(espec, flat.cuda(), x.numpy())
    scale = max(1.0, float(np.abs(ref).max()))
    np.testing.assert_allclose(vals, ref, atol=TOL * scale, rtol=0)
    srt = np.sort(ref, axis=1)
    clear = (srt[:, -1] - srt[:, -2]) > 4 * TOL * scale
    assert np.array_equal(acts[clear], ref.argmax(axis=1)[clear])


def _act_host(desc, flat, x, scratch):
    out = np.full(x.shape[0], -1, dtype=np.int32)
    x = np.array(x)
    C.check(C.lib().dqnx_act_host(ctypes.byref(desc), flat.data_ptr(), x.ctypes.data, x.shape[0], out.ctypes.data,
                                  scratch.data_ptr(), scratch.numel() * 4, torch.cuda.current_stream().cuda_stream),
            "act_host")
    return out


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("geom", [GEOMS[1], GEOMS[0]], ids=[GEOM_IDS[1], GEOM_IDS[0]])
def test_gpu_act_host_two_stream_shared_scratch_across_row_counts(monkeypatch, geom, mode):
    """dqnx_act_host with one scratch sized for 64 rows and n up and down: the shares and F sit at the start,
    the tickets (shared by the conv stack and the MLP kernel) at the end whatever n; n <= 4 takes the
    in-place pinned path with the completion word, larger n the copies.  Obs shifted by +0.25 so that no
    obs word is near zero.  Actions equal dqnx_act's on the same rows, and the oracle's on every row (its
    top-two gaps on these inputs are all clear of 4 TOL).  mode: DQNX_ACT_TS, 1 = the default routing (the
    stack where it measured faster, the per-conv launches elsewhere), 2 = the stack for every n."""
    monkeypatch.setenv("DQNX_ACT_TS", mode)
    ospec, espec, params, flat = _net(geom, "dueling")
    desc = espec.to_c()
    nb = int(C.lib().dqnx_act_host_scratch_bytes(ctypes.byref(desc), 64))
    scratch = torch.zeros((nb + 15) // 16 * 4, dtype=torch.float32, device="cuda")
    for n in (64, 8, 1, 64, 3, 2, 5, 8):
        x, ref, scale = _case(geom, "dueling", n, 0.25)
        out = _act_host(desc, flat, x, scratch)
        acts, vals = _act(espec, flat, x)
        assert np.array_equal(out, acts), (n, out, acts)
        np.testing.assert_allclose(vals, ref, atol=TOL * scale, rtol=0)
        assert _all_clear(ref, scale)   # (smallest oracle gap of these inputs: 1.5e-4 at 2x27x5, n = 64)
        assert np.array_equal(out, ref.argmax(axis=1)), n


@pytest.mark.parametrize("mode", ["1", "2"])
def test_gpu_act_host_two_stream_no_poll_without_word(monkeypatch, mode):
    """HEAD net, n = 5: two row groups, so the launch stores no completion word and the call must not
    poll for one (the poll's fall-back is 500 ms: 20 calls inside 0.4 s, the bound of the MLP test).
    mode: DQNX_ACT_TS (1 = default routing, 2 = the conv stack for every n)."""
    monkeypatch.setenv("DQNX_ACT_TS", mode)
    geom = GEOMS[0]
    _, espec, _, flat = _net(geom, "dueling")
    desc = espec.to_c()
    x, ref, scale = _case(geom, "dueling", 5)
    nb = int(C.lib().dqnx_act_host_scratch_bytes(ctypes.byref(desc), 5))
    scratch = torch.zeros((nb + 15) // 16 * 4, dtype=torch.float32, device="cuda")
    out = _act_host(desc, flat, x, scratch)
    assert _all_clear(ref, scale) and np.array_equal(out, ref.argmax(axis=1))
    t0 = time.perf_counter()
    for _ in range(20):
        out = _act_host(desc, flat, x, scratch)
    dt = time.perf_counter() - t0
    assert dt < 0.4, f"act_host waited for a completion word its launch never stores ({dt:.3f} s)"
    assert np.array_equal(out, ref.argmax(axis=1))


@pytest.mark.parametrize("n_env", [1, 2])
def test_gpu_agent_choose_actions_one_call_two_stream(tmp_path, n_env):
    """A HEAD-net agent's choose_actions is ONE dqnx_agent_choose call (Network.actions is never entered):
    the oracle's greedy actions with the reference's epsilon draws (R:dqn/agent.py:92-99) on the live
    `random` generator, on post-step weights (learn() and update_target_network() between the steps)."""
    algo, obs_dim, batch, buffer, n_fill, seed = "DuelingDoubleDQNAgent", 284, 32, 500, 300, 23
    torch.manual_seed(seed)
    agent = getattr(Agents, algo)(**agent_kwargs(algo, obs_dim, batch, buffer, tmp_path, n_env=n_env,
                                                 nn_conf_func=hybrid_network_config))

    def no_fallback(*a, **k):
        raise AssertionError("choose_actions fell back to Network.actions")
    agent.online_network.actions = no_fallback
    spec = O.hybrid_spec(8, O.algo_spec_head(algo))
    init = O.reference_init(spec, seed)
    oracle = O.OracleLearner(spec, algo, batch, buffer, seed=seed, params=init, per_pow="cr", n_env=n_env)
    steps = 3
    obs, act, rew, done, nobs = O.synth_transitions(n_fill + steps * n_env, obs_dim, 8, seed=seed)
    for i in range(0, n_fill, n_env):
        j = min(i + n_env, n_fill)
        rows = (obs[i:j], [int(a) for a in act[i:j]], [float(r) for r in rew[i:j]], [bool(d) for d in done[i:j]],
                nobs[i:j])
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
        if n_env > 1:
            rows = (x, list(actions), [float(r) for r in rew[lo:hi]], [bool(d) for d in done[lo:hi]], nobs[lo:hi])
            agent.store_transitions(*rows, None)
            oracle.store_transitions(*rows)
        oracle.py_state = O.py_state_to_array()
        oracle.np_state = O.np_state_to_array()
        oracle.step = t
        agent.learn()
        agent.update_target_network()
        oracle.learn()
        oracle.update_target_network()
