"""CPU checks of the conservative Q-learning ABI (include/dqnx.h "conservative Q-learning" <-> libdqnx.so <->
dqn/_capi.py): the new exports with every pinned layout unchanged, the set / get round trip, the planned
kernel tables and arena with the regulariser on (what they are with it off) and the row arithmetic of
csrc/cql.hpp against a float64 restatement.  No GPU calls: planning binds an address that is never
dereferenced."""
import ctypes
import math
import re

import numpy as np
import pytest

from dqn import _capi as C
from dqn import engine as E
import test_grad_clip_capi as GC

LS = GC.LS
NEW = ("dqnx_set_cql", "dqnx_get_cql", "dqnx_cql_row")
FP = ctypes.POINTER(ctypes.c_float)


def test_cql_symbols_abi_and_layouts(tmp_path):
    L = C.lib()
    src = re.sub(r"/\*.*?\*/", "", open(LS.HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in C.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    sizes = {"dqnx_config": C.Config, "dqnx_ctrl": C.Ctrl, "dqnx_net_desc": C.NetDesc, "dqnx_state_info": C.StateInfo,
             "dqnx_learn_stats": C.LearnStats, "dqnx_grad_clip_info": C.GradClipInfo}
    got = LS._gcc_values(tmp_path, {"abi": "DQNX_ABI_VERSION", "clip": "DQNX_BUF_GRAD_CLIP", "stats": "DQNX_BUF_LEARN_STATS",
                                    "count": "DQNX_BUF_COUNT", **{n: "DQNX_BUF_" + n for n in LS.ABI4_BUFFERS},
                                    **{k: f"sizeof({k})" for k in sizes}})
    assert got["abi"] == 5 == L.dqnx_abi_version()   # new symbols only: the version stays
    for i, n in enumerate(LS.ABI4_BUFFERS):
        assert got[n] == i
    assert got["stats"] == C.BUF_LEARN_STATS == len(LS.ABI4_BUFFERS)
    assert got["clip"] == C.BUF_GRAD_CLIP == got["stats"] + 1 and got["count"] == C.BUF_COUNT == got["clip"] + 1 == 20
    assert {k: got[k] for k in sizes} == {"dqnx_config": 288, "dqnx_ctrl": 5136, "dqnx_net_desc": 148,
                                          "dqnx_state_info": 608, "dqnx_learn_stats": 1312, "dqnx_grad_clip_info": 40}
    for k, t in sizes.items():
        assert ctypes.sizeof(t) == got[k], k


def test_cql_set_get_round_trip():
    L = C.lib()
    h = LS._unbound(E.mlp_spec(14, 8, "dueling"), C.DQNX_ALGO_DOUBLE, 32, 200)   # host only: an unbound engine takes it
    try:
        v = ctypes.c_double(-1.0)
        assert L.dqnx_get_cql(h, ctypes.byref(v)) == 0 and v.value == 0.0   # off is the default
        for given, want in ((1.0, 1.0), (0.25, 0.25), (0.0, 0.0), (-3.0, 0.0), (0.25, 0.25)):
            assert L.dqnx_set_cql(h, ctypes.c_double(given)) == 0
            assert L.dqnx_get_cql(h, ctypes.byref(v)) == 0 and v.value == want
        for bad in (math.nan, math.inf, -math.inf):
            assert L.dqnx_set_cql(h, ctypes.c_double(bad)) == C.DQNX_EINVAL
            assert L.dqnx_get_cql(h, ctypes.byref(v)) == 0 and v.value == 0.25   # the value is kept
        assert L.dqnx_set_cql(None, ctypes.c_double(1.0)) == C.DQNX_EINVAL
        assert L.dqnx_get_cql(h, None) == C.DQNX_EINVAL
        assert L.dqnx_get_cql(None, ctypes.byref(v)) == C.DQNX_EINVAL
    finally:
        L.dqnx_engine_destroy(h)


def _arena(h):
    total = ctypes.c_uint64()
    assert C.lib().dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
    return total.value


@pytest.mark.parametrize("net,algo,env", [
    ("mlp14", C.DQNX_ALGO_DOUBLE, {}), ("mlp14", C.DQNX_ALGO_DQN, {}), ("mlp284", C.DQNX_ALGO_PER_DOUBLE, {}),
    ("mlp14", C.DQNX_ALGO_DOUBLE, {"DQNX_DW_ADAM16": "0"}), ("mlp14", C.DQNX_ALGO_DOUBLE, {"DQNX_BWD_PLAN": "0"}),
    ("head", C.DQNX_ALGO_DOUBLE, {}), ("head", C.DQNX_ALGO_PER_DOUBLE, {}), ("hybrid84", C.DQNX_ALGO_DOUBLE, {})])
def test_cql_planned_kernel_tables(monkeypatch, net, algo, env):
    """The regulariser costs no launch, FLOP, byte or arena byte that a plan table shows: with alpha = 1 every
    table (names, FLOPs, bytes) and the arena size are those of an engine that never set it, with clipping
    off and on."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = C.lib()
    spec = {"mlp14": E.mlp_spec(14, 8, "dueling" if algo != C.DQNX_ALGO_DQN else "linear"),
            "mlp284": E.mlp_spec(284, 8, "dueling"), "head": E.hybrid_spec(8, "dueling"),
            "hybrid84": E.hybrid_spec(8, "dueling", micro_chw=(4, 84, 84))}[net]
    per = algo == C.DQNX_ALGO_PER_DOUBLE
    queried = [f for f in GC.QUERIED if not (per and f & C.STEP_GIVEN_INDICES)]
    h0, h1 = GC._bound(spec, algo), GC._bound(spec, algo)
    try:
        assert L.dqnx_set_cql(h1, ctypes.c_double(1.0)) == 0
        assert _arena(h0) == _arena(h1)
        for f in queried:
            assert LS._kernel_names(h1, f) == LS._kernel_names(h0, f), f
        for h in (h0, h1):
            assert L.dqnx_set_grad_clip(h, ctypes.c_double(10.0)) == 0
        assert _arena(h0) == _arena(h1)
        for f in queried:
            t = LS._kernel_names(h1, f)
            assert t == LS._kernel_names(h0, f), f
            if not f & C.STEP_GRADS_ONLY:
                assert "clip_coef" in [n for n, _, _ in t]
    finally:
        L.dqnx_engine_destroy(h0)
        L.dqnx_engine_destroy(h1)


# ---- dqnx_cql_row against float64 ------------------------------------------------------------------------
def _row(q, a):
    L = C.lib()
    q = np.ascontiguousarray(q, dtype=np.float32)
    gap = ctypes.c_float(np.nan)
    pm = np.full(q.size, np.nan, dtype=np.float32)
    assert L.dqnx_cql_row(q.ctypes.data_as(FP), q.size, a, ctypes.byref(gap), pm.ctypes.data_as(FP)) == 0
    return np.float32(gap.value), pm


def _ref(q, a):
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    m = q.max()
    e = np.exp(q - m)
    lse = m + np.log(e.sum())
    onehot = np.zeros(q.size)
    onehot[a] = 1.0
    return lse - q[a], e / e.sum() - onehot, lse


def _rows(A):
    rng = np.random.default_rng(1000 + A)
    rows = [np.full(A, 0.75), np.full(A, -3.0)]
    for k in {0, A // 2, A - 1}:   # one dominant entry 200 above the rest: the others' e_j are exactly 0
        r = rng.normal(size=A)
        r[k] += 200.0
        rows.append(r)
    rows += [1e4 + rng.normal(size=A), -1e4 + rng.normal(size=A)]   # the max subtraction keeps everything finite
    rows += [rng.normal(size=A) * s for s in (0.1, 1.0, 10.0) for _ in range(4)]
    return rows


@pytest.mark.parametrize("A", [1, 2, 3, 8, 15, 16])
def test_cql_row_matches_float64(A):
    for q in _rows(A):
        for a in {0, A - 1}:
            gap, pm = _row(q, a)
            rgap, rpm, lse = _ref(q, a)
            assert np.isfinite(gap) and np.isfinite(pm).all()
            # a sum of up to 16 fp32 terms and two libm calls stays under 16 * 2^-23 relative
            assert abs(float(gap) - rgap) <= 4e-6 * max(1.0, abs(lse)), (A, a, q, gap, rgap)
            assert np.abs(pm.astype(np.float64) - rpm).max() <= 4e-6, (A, a, q, pm, rpm)
            assert gap >= -4e-6
            if A == 1:
                assert gap == 0.0 and pm[0] == 0.0


def test_cql_row_dominant_entry_is_exact():
    q = np.zeros(8, dtype=np.float32)
    q[5] = 200.0
    gap, pm = _row(q, 5)
    assert gap == 0.0 and (pm == 0.0).all()        # e_j == 0 exactly for the others, p_5 == 1
    gap, pm = _row(q, 2)
    assert gap == 200.0 and pm[5] == 1.0 and pm[2] == -1.0 and (np.delete(pm, [2, 5]) == 0.0).all()


def test_cql_row_clamps_the_action_and_refuses_bad_arguments():
    L = C.lib()
    q = np.array([0.3, -1.0, 2.0], dtype=np.float32)
    g0, p0 = _row(q, 0)
    for a in (-1, 3, 99):   # outside [0, A): action 0, as the head kernels clamp it
        g, p = _row(q, a)
        assert g == g0 and np.array_equal(p, p0)
    gap = ctypes.c_float()
    pm = np.zeros(17, dtype=np.float32)
    q17 = np.zeros(17, dtype=np.float32)
    for n in (0, -1, 17):
        assert L.dqnx_cql_row(q17.ctypes.data_as(FP), n, 0, ctypes.byref(gap), pm.ctypes.data_as(FP)) == C.DQNX_EINVAL
    assert L.dqnx_cql_row(None, 3, 0, ctypes.byref(gap), pm.ctypes.data_as(FP)) == C.DQNX_EINVAL
    assert L.dqnx_cql_row(q.ctypes.data_as(FP), 3, 0, None, pm.ctypes.data_as(FP)) == C.DQNX_EINVAL
    assert L.dqnx_cql_row(q.ctypes.data_as(FP), 3, 0, ctypes.byref(gap), None) == C.DQNX_EINVAL
