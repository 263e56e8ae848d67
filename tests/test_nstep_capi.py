"""CPU checks of n-step returns (include/dqnx.h "n-step returns" <-> libdqnx.so <-> dqn/_capi.py): the
window arithmetic of dqnx_nstep_window -- the inline function the gather kernel calls -- against the
numpy loop of the header, on data that contains every kind of window; what create refuses; the launch
list of an n-step engine.  No GPU calls."""
import ctypes
import functools

import numpy as np
import pytest

from dqn import _capi as C
from dqn import engine as E
import nstep_ref as NR

SIZE, GAMMA = 200, 0.99
N_STEPS, N_ENVS = (1, 2, 3, 5, 16), (1, 3)


@functools.lru_cache(maxsize=None)
def ring(n, n_env):
    """200 random rewards and done flags (rate 1/6): the first seed whose ring holds every window kind
    for (n, n_env) -- with one environment the newest n - 1 rows must all be not-done for the ring end
    to cut a window at every length, which one seed in a few gives"""
    ps = range(SIZE)
    for seed in range(2000):
        rew, done = NR.ring_scalars(SIZE, 7000 + seed)
        if NR.census(rew, done, SIZE, ps, n, n_env) == NR.every_kind(n):
            return rew, done
    raise AssertionError(f"no seed gives every window kind for n = {n}, n_env = {n_env}")


@pytest.mark.parametrize("n_env", N_ENVS)
@pytest.mark.parametrize("n", N_STEPS)
def test_data_contains_every_window_kind(n, n_env):
    """on the numpy side alone: a full window, a window cut by done at each j < n, a window cut by the
    ring end at each m < n; done rate about 1/6"""
    rew, done = ring(n, n_env)
    kinds = NR.census(rew, done, SIZE, range(SIZE), n, n_env)
    assert ("full",) in kinds
    for j in range(n):
        assert ("done", j) in kinds, j
    for m in range(1, n):
        assert ("end", m) in kinds, m
    assert 0.10 < done.mean() < 0.24, done.mean()
    # and the reference itself: m >= 1, last inside the ring, n = 1 is the row itself
    R, d, disc, last, m = NR.windows(rew, done, SIZE, range(SIZE), n, n_env, GAMMA)
    assert m.min() >= 1 and m.max() == n and last.max() < SIZE
    if n == 1:
        assert np.array_equal(R, rew) and np.array_equal(d, done.astype(np.float32))
        assert np.array_equal(last, np.arange(SIZE)) and np.all(disc == np.float32(GAMMA))


@pytest.mark.parametrize("n_env", N_ENVS)
@pytest.mark.parametrize("n", N_STEPS)
def test_nstep_window_matches_numpy_loop(n, n_env):
    """every p of the ring: R, d and disc with ==, last and m exactly"""
    L = C.lib()
    rew, done = ring(n, n_env)
    donef = done.astype(np.float32)
    want = NR.windows(rew, donef, SIZE, range(SIZE), n, n_env, GAMMA)
    R, d, disc = ctypes.c_float(), ctypes.c_float(), ctypes.c_float()
    last, m = C.I64(), C.I32()
    for p in range(SIZE):
        rc = L.dqnx_nstep_window(rew.ctypes.data, donef.ctypes.data, SIZE, p, n, n_env, GAMMA, ctypes.byref(R),
                                 ctypes.byref(d), ctypes.byref(disc), ctypes.byref(last), ctypes.byref(m))
        assert rc == C.DQNX_OK
        got = (np.float32(R.value), np.float32(d.value), np.float32(disc.value), last.value, m.value)
        exp = tuple(col[p] for col in want)
        assert got == exp, (p, got, exp)
    # the discount is a repeated fp64 multiply rounded once: fp32(gamma^m)
    g = np.float64(1.0)
    for k in range(1, n + 1):
        g = g * np.float64(GAMMA)
        assert np.all(want[2][want[4] == k] == np.float32(g))


def test_nstep_window_other_gamma_and_argument_checks():
    L = C.lib()
    rew, done = ring(5, 3)
    donef = done.astype(np.float32)
    R, disc, m = ctypes.c_float(), ctypes.c_float(), C.I32()
    for gamma in (0.5, 0.999, 1.0):
        want = NR.windows(rew, donef, SIZE, range(SIZE), 5, 3, gamma)
        for p in range(SIZE):
            assert L.dqnx_nstep_window(rew.ctypes.data, donef.ctypes.data, SIZE, p, 5, 3, gamma, ctypes.byref(R),
                                       None, ctypes.byref(disc), None, ctypes.byref(m)) == C.DQNX_OK
            assert (np.float32(R.value), np.float32(disc.value), m.value) == (want[0][p], want[2][p], want[4][p])
    bad = [dict(p=-1), dict(p=SIZE), dict(n=0), dict(n=C.NSTEP_MAX + 1), dict(n_env=0), dict(size=0)]
    for kw in bad:
        a = dict(size=SIZE, p=0, n=3, n_env=1)
        a.update(kw)
        assert L.dqnx_nstep_window(rew.ctypes.data, donef.ctypes.data, a["size"], a["p"], a["n"], a["n_env"], GAMMA,
                                   None, None, None, None, None) == C.DQNX_EINVAL, kw
    assert L.dqnx_nstep_window(None, donef.ctypes.data, SIZE, 0, 3, 1, GAMMA, None, None, None, None, None) == C.DQNX_EINVAL


# ---- configuration and create -------------------------------------------------------------------------
def _config(spec, n_step, batch=32, cap=500, algo=C.DQNX_ALGO_DOUBLE, n_env=1):
    cfg = C.Config()
    cfg.net = spec.to_c()
    C.lib().dqnx_config_defaults(ctypes.byref(cfg))
    assert cfg.n_step == 1   # the default
    cfg.batch, cfg.capacity, cfg.algo, cfg.n_env = batch, cap, algo, n_env
    if n_step is not None:
        cfg.n_step = n_step
    return cfg


def _create(cfg):
    h = ctypes.c_void_p()
    rc = C.lib().dqnx_engine_create(ctypes.byref(cfg), ctypes.byref(h))
    return rc, h


def test_n_step_fills_the_config_structs_padding():
    """dqnx_config keeps its size and every other field its offset (tests/test_grad_clip_capi.py pins 288 bytes
    and the ABI version): n_step lies in the four bytes that were padding between rank and capacity, which
    dqnx_config_defaults has always written.  test_capi's generic check holds the offsets to the header."""
    assert ctypes.sizeof(C.Config) == 288
    assert C.Config.rank.offset + 4 == C.Config.n_step.offset == C.Config.capacity.offset - 4 == 164
    assert C.NSTEP_MAX == 16
    cfg = C.Config()
    ctypes.memset(ctypes.byref(cfg), 0xff, ctypes.sizeof(cfg))
    C.lib().dqnx_config_defaults(ctypes.byref(cfg))
    assert cfg.n_step == 1


@pytest.mark.parametrize("n_step", [0, 17, -1])
def test_create_refuses_n_step_out_of_range(n_step):
    rc, _ = _create(_config(E.mlp_spec(14, 8, "dueling"), n_step))
    assert rc == C.DQNX_EINVAL and b"n_step" in C.lib().dqnx_last_error()


def _unbound(cfg):
    """an engine with a host arena bound: the plan tables are host work (tests/test_plan_tables.py)"""
    rc, h = _create(cfg)
    assert rc == C.DQNX_OK, C.lib().dqnx_last_error()
    nbytes = ctypes.c_uint64()
    C.check(C.lib().dqnx_engine_arena_bytes(h, ctypes.byref(nbytes)), "arena_bytes")
    arena = np.zeros(int(nbytes.value) + 256, np.uint8)
    base = (arena.ctypes.data + 255) // 256 * 256
    C.check(C.lib().dqnx_engine_bind(h, ctypes.c_void_p(base), nbytes.value), "bind")
    return h, arena, int(nbytes.value)


def _kernels(h, flags=0):
    L = C.lib()
    n = C.I32()
    C.check(L.dqnx_learn_kernel_count(h, flags, ctypes.byref(n)), "count")
    out = []
    for i in range(n.value):
        name = ctypes.create_string_buffer(64)
        fl, by = ctypes.c_double(), ctypes.c_double()
        C.check(L.dqnx_learn_kernel_info(h, flags, i, name, 64, ctypes.byref(fl), ctypes.byref(by)), "info")
        out.append((name.value.decode(), fl.value, by.value))
    return out


def _region(h, which):
    o, b = ctypes.c_uint64(), ctypes.c_uint64()
    C.check(C.lib().dqnx_engine_buffer(h, which, ctypes.byref(o), ctypes.byref(b)), "buffer")
    return int(o.value), int(b.value)


def _minibatch(h):
    o, b = ctypes.c_uint64(), ctypes.c_uint64()
    C.check(C.lib().dqnx_nstep_buffer(h, ctypes.byref(o), ctypes.byref(b)), "nstep_buffer")
    return int(o.value), int(b.value)


SAMPLERS = ("sample_uniform", "per_sample", "idx_to_phys")


@pytest.mark.parametrize("net", ["mlp", "head"])
@pytest.mark.parametrize("flags", [0, C.STEP_SOFT_UPDATE, C.STEP_GIVEN_INDICES, C.STEP_PREFETCH, C.STEP_GRADS_ONLY])
def test_kernel_list_gains_exactly_one_leading_nstep_gather(monkeypatch, net, flags):
    """n_step = 3: the default engine's launches plus "nstep_gather", the first launch behind the one that
    makes the slot table final (the step's first launch where no sampler launch is listed); 0 FLOPs and
    the bytes of the rows and scalars moved.  n_step = 1: unchanged, the same arena, an empty region."""
    monkeypatch.delenv("DQNX_NSTEP_FORCE", raising=False)
    spec = E.mlp_spec(14, 8, "dueling") if net == "mlp" else E.hybrid_spec(8, "dueling")
    h1, a1, bytes1 = _unbound(_config(spec, None))
    h3, a3, bytes3 = _unbound(_config(spec, 3))
    try:
        k1, k3 = _kernels(h1, flags), _kernels(h3, flags)
        names3 = [k[0] for k in k3]
        assert names3.count("nstep_gather") == 1 and "nstep_gather" not in [k[0] for k in k1]
        at = names3.index("nstep_gather")
        assert [k for k in k3 if k[0] != "nstep_gather"] == k1   # names, FLOPs and bytes of every other launch
        assert at == (1 if k1[0][0] in SAMPLERS else 0), names3
        assert all(nm not in SAMPLERS for nm in names3[at + 1:])
        _, fl, by = k3[at]
        S = (spec.obs_dim + 3) // 4 * 4
        assert fl == 0 and by == 32 * (4 * 4 * S + 4 + 8 * 3 + 4 + 20 + 16)
        assert _minibatch(h1)[1] == 0
        o3, b3 = _minibatch(h3)
        assert b3 >= 32 * (2 * 4 * S + 5 * 4 + 16) and o3 % 256 == 0
        # the workspace's last part: every region up to the workspace where it was, the workspace longer by it
        w1, w3 = _region(h1, C.BUF_WORKSPACE), _region(h3, C.BUF_WORKSPACE)
        assert w3[0] == w1[0] and w3[0] + w3[1] == (o3 + b3 + 255) // 256 * 256 and o3 >= w1[0] + w1[1]
        for which in range(C.BUF_WORKSPACE):
            assert _region(h1, which) == _region(h3, which), which
        assert bytes3 > bytes1
    finally:
        C.lib().dqnx_engine_destroy(h1)
        C.lib().dqnx_engine_destroy(h3)


def test_force_variable_sends_a_default_engine_through_the_gather(monkeypatch):
    spec = E.mlp_spec(14, 8, "dueling")
    monkeypatch.delenv("DQNX_NSTEP_FORCE", raising=False)
    h0, a0, _ = _unbound(_config(spec, 1))
    monkeypatch.setenv("DQNX_NSTEP_FORCE", "1")   # read at create
    h1, a1, _ = _unbound(_config(spec, 1))
    monkeypatch.delenv("DQNX_NSTEP_FORCE")
    try:
        n0, n1 = [k[0] for k in _kernels(h0)], [k[0] for k in _kernels(h1)]
        assert n1 == n0[:1] + ["nstep_gather"] + n0[1:]
        assert _minibatch(h0)[1] == 0 < _minibatch(h1)[1]
    finally:
        C.lib().dqnx_engine_destroy(h0)
        C.lib().dqnx_engine_destroy(h1)
