"""CPU checks of the offline-evaluation ABI (include/dqnx.h "offline evaluation" <-> libdqnx.so <-> dqn/_capi.py):
the new exports with every pinned layout and the ABI version unchanged, dqnx_eval_result's layout against gcc,
the row arithmetic of csrc/eval.hpp (dqnx_eval_row) against a float64 restatement, the refusals that need no GPU,
and the arena and planned kernel tables of default, n-step and CQL engines, which the feature must not move.  No
GPU calls: planning binds an address that is never dereferenced."""
import ctypes
import re

import numpy as np
import pytest

from dqn import _capi as C
from dqn import engine as E
import test_grad_clip_capi as GC

LS = GC.LS
NEW = ("dqnx_eval_scratch_bytes", "dqnx_eval_range", "dqnx_eval_row", "dqnx_eval_kernel_count", "dqnx_eval_kernel_name",
       "dqnx_eval_chunk_timed")
FP = ctypes.POINTER(ctypes.c_float)


def test_eval_symbols_abi_and_layouts(tmp_path):
    L = C.lib()
    src = re.sub(r"/\*.*?\*/", "", open(LS.HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in C.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    sizes = {"dqnx_config": C.Config, "dqnx_ctrl": C.Ctrl, "dqnx_net_desc": C.NetDesc, "dqnx_state_info": C.StateInfo,
             "dqnx_learn_stats": C.LearnStats, "dqnx_grad_clip_info": C.GradClipInfo}
    got = LS._gcc_values(tmp_path, {"abi": "DQNX_ABI_VERSION", "count": "DQNX_BUF_COUNT",
                                    **{k: f"sizeof({k})" for k in sizes}})
    assert got["abi"] == 5 == L.dqnx_abi_version()   # new symbols only: the version stays
    assert got["count"] == C.BUF_COUNT == 20
    assert {k: got[k] for k in sizes} == {"dqnx_config": 288, "dqnx_ctrl": 5136, "dqnx_net_desc": 148,
                                          "dqnx_state_info": 608, "dqnx_learn_stats": 1312, "dqnx_grad_clip_info": 40}


@pytest.mark.parametrize("cname,py,size", [("dqnx_eval_result", C.EvalResult, 376),
                                           ("dqnx_eval_row_result", C.EvalRowResult, 40)])
def test_eval_struct_layouts_match_gcc(tmp_path, cname, py, size):
    exprs = {"sizeof": f"sizeof({cname})"}
    for fname, _ in py._fields_:
        exprs[fname] = f"offsetof({cname}, {fname})"
    got = LS._gcc_values(tmp_path, exprs)
    assert ctypes.sizeof(py) == got["sizeof"] == size
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[fname], fname
    assert sum(ctypes.sizeof(t) for _, t in py._fields_) == got["sizeof"]   # no padding
    if py is C.EvalResult:
        assert [f for f, _ in py._fields_] == [
            "rows", "huber_sum", "abs_td_sum", "td_sq_sum", "q_sa_sum", "v_sum", "cql_gap_sum", "action_gap_sum",
            "reward_sum", "target_sum", "abs_td_max", "v_max", "v_min", "agree_rows", "done_rows", "greedy_hist",
            "taken_hist"]
        assert C.EvalResult.greedy_hist.size == C.EvalResult.taken_hist.size == 8 * C.STATS_MAX_ACTIONS


# ---- dqnx_eval_row against float64 -----------------------------------------------------------------------
def _row(raw0, raw1, raw2, head, A, algo, act, rew, done, disc):
    L = C.lib()
    arrs = [None if r is None else np.ascontiguousarray(r, dtype=np.float32) for r in (raw0, raw1, raw2)]
    ptrs = [None if a is None else a.ctypes.data_as(FP) for a in arrs]
    out = C.EvalRowResult()
    rc = L.dqnx_eval_row(ptrs[0], ptrs[1], ptrs[2], head, A, algo, act, ctypes.c_float(rew), ctypes.c_float(done),
                         ctypes.c_float(disc), ctypes.byref(out))
    return rc, out


def _q64(raw, head, A):
    raw = np.asarray(raw, dtype=np.float32).astype(np.float64)
    if head == C.DQNX_HEAD_DUELING:
        return raw[0] + (raw[1:1 + A] - raw[1:1 + A].mean())
    return raw[:A].copy()


def _ref(raw0, raw1, raw2, head, A, algo, act, rew, done, disc):
    """float64 restatement over the fp32 inputs.  The greedy / Double argmax are taken from the fp32 rows the
    library forms (passed back in), so a float64 tie-break can never disagree with an fp32 one."""
    q0, q2 = _q64(raw0, head, A), _q64(raw2, head, A)
    f = lambda x: float(np.float32(x))
    if algo == C.DQNX_ALGO_DQN:
        qn = q2.max()
    else:
        q1 = _q64(raw1, head, A)
        qn = q2[int(np.argmax(q1))]
    y = f(rew) + (1.0 - f(done)) * f(disc) * qn
    delta = y - q0[act]
    z = abs(delta)
    lb = 0.5 * z * z if z < 1.0 else z - 0.5
    v = q0.max()
    lse = v + np.log(np.exp(q0 - v).sum())
    srt = np.sort(q0)
    return {"q": q0, "qn": qn, "y": y, "delta": delta, "lb": lb, "v": v, "gap": lse - q0[act], "lse": lse,
            "agap": (srt[-1] - srt[-2]) if A > 1 else 0.0}


def _raws(NH, seed):
    rng = np.random.default_rng(seed)
    rows = [np.full(NH, 0.75), np.full(NH, -3.0)]                      # all-equal: first-maximum tie rule
    for k in {0, NH // 2, NH - 1}:                                      # one dominant entry
        r = rng.normal(size=NH)
        r[k] += 200.0
        rows.append(r)
    rows += [1e4 + rng.normal(size=NH), -1e4 + rng.normal(size=NH)]     # entries +-1e4
    rows += [rng.normal(size=NH) * s for s in (0.1, 1.0, 10.0) for _ in range(3)]
    return rows


@pytest.mark.parametrize("head", [C.DQNX_HEAD_LINEAR, C.DQNX_HEAD_DUELING])
@pytest.mark.parametrize("A", [1, 2, 3, 8, 15, 16])
def test_eval_row_matches_float64(A, head):
    if head == C.DQNX_HEAD_DUELING and A == 16:
        # a dueling head has V + A advantages in the 16 head slots: 15 actions at most; the hook says so
        rc, _ = _row(np.zeros(17), np.zeros(17), np.zeros(17), head, 16, C.DQNX_ALGO_DOUBLE, 0, 0.0, 0.0, 0.99)
        assert rc == C.DQNX_EINVAL
        return
    NH = A + 1 if head == C.DQNX_HEAD_DUELING else A
    raws = _raws(NH, 2000 + 17 * A + head)
    rng = np.random.default_rng(77 + A)
    n_checked = 0
    for i, raw0 in enumerate(raws):
        raw1, raw2 = raws[(i + 3) % len(raws)], raws[(i + 5) % len(raws)]
        for algo in (C.DQNX_ALGO_DQN, C.DQNX_ALGO_DOUBLE):
            for act in {0, A - 1}:
                rew, done, disc = float(rng.normal()), float(i % 3 == 0), 0.99 ** (1 + i % 3)
                rc, out = _row(raw0, raw1, raw2, head, A, algo, act, rew, done, disc)
                assert rc == 0
                r = _ref(raw0, raw1, raw2, head, A, algo, act, rew, done, disc)
                q32 = r["q"].astype(np.float32)
                scale = max(1.0, np.abs(np.asarray(raw0)).max(), abs(r["y"]), abs(r["qn"]))
                tol = 4e-6 * scale   # the bound tests/test_cql_capi.py uses for the same forms, at the row's magnitude
                # integers: exact.  The greedy action is the FIRST maximum of the fp32 row; where float64 sees a
                # near-tie the fp32 row decides (the all-equal rows pin the tie rule itself)
                assert out.action == act
                if np.unique(q32).size == A or np.all(q32 == q32[0]):
                    assert out.greedy == int(np.argmax(q32)), (A, head, raw0)
                if np.all(np.asarray(raw0) == np.asarray(raw0)[0]):
                    assert out.greedy == 0 and out.action_gap == 0.0
                assert abs(out.q_a - r["q"][act]) <= tol
                assert abs(out.v - r["v"]) <= tol
                assert abs(out.y - r["y"]) <= tol, (out.y, r["y"])
                assert abs(out.delta - r["delta"]) <= 2 * tol
                assert abs(out.huber - r["lb"]) <= 2 * tol
                assert abs(out.gap - r["gap"]) <= 4e-6 * max(1.0, abs(r["lse"]), scale)
                assert abs(out.action_gap - r["agap"]) <= 2 * tol
                assert out.gap >= -4e-6 * scale and out.action_gap >= 0.0 and out.reserved0 == 0.0
                if A == 1:
                    assert out.greedy == 0 and out.action_gap == 0.0 and out.gap == 0.0
                n_checked += 1
    assert n_checked >= 28


def test_eval_row_tie_rule_and_exact_cases():
    # first maximum, as torch.argmax and the head kernels take it
    rc, out = _row([1.0, 5.0, 5.0, 2.0], None, [0.0, 1.0, 2.0, 3.0], C.DQNX_HEAD_LINEAR, 4, C.DQNX_ALGO_DQN, 3, 1.0, 0.0, 0.5)
    assert rc == 0 and out.greedy == 1 and out.v == 5.0 and out.action_gap == 0.0
    assert out.y == 1.0 + 0.5 * 3.0 and out.q_a == 2.0 and out.delta == 0.5 and out.huber == 0.125
    # Double: the online(s') argmax (first maximum: slot 0) picks the target net's entry; done cuts the bootstrap
    rc, out = _row([0.0, 4.0], [7.0, 7.0], [10.0, 20.0], C.DQNX_HEAD_LINEAR, 2, C.DQNX_ALGO_DOUBLE, 1, 2.0, 0.0, 1.0)
    assert rc == 0 and out.y == 12.0 and out.delta == 8.0 and out.huber == 7.5 and out.action_gap == 4.0
    rc, out = _row([0.0, 4.0], [7.0, 7.0], [10.0, 20.0], C.DQNX_HEAD_LINEAR, 2, C.DQNX_ALGO_DOUBLE, 1, 2.0, 1.0, 1.0)
    assert rc == 0 and out.y == 2.0 and out.delta == -2.0 and out.huber == 1.5
    # dueling aggregate: V + (A_j - mean A)
    rc, out = _row([1.0, 2.0, 4.0], None, [0.0, 0.0, 0.0], C.DQNX_HEAD_DUELING, 2, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)
    assert rc == 0 and out.q_a == 0.0 and out.v == 2.0 and out.greedy == 1 and out.action_gap == 2.0
    # an action outside [0, A) is taken as 0
    a = _row([0.3, -1.0, 2.0], None, [0.1, 0.2, 0.3], C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DQN, 0, 0.5, 0.0, 0.9)[1]
    for bad in (-1, 3, 99):
        b = _row([0.3, -1.0, 2.0], None, [0.1, 0.2, 0.3], C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DQN, bad, 0.5, 0.0, 0.9)[1]
        assert bytes(a) == bytes(b)


def test_eval_row_refuses_bad_arguments():
    z = np.zeros(17, dtype=np.float32)
    for A in (0, -1, 17):
        assert _row(z, z, z, C.DQNX_HEAD_LINEAR, A, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(None, z, z, C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(z, z, None, C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(z, None, z, C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DOUBLE, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(z, None, z, C.DQNX_HEAD_LINEAR, 3, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)[0] == 0
    assert _row(z, z, z, 7, 3, C.DQNX_ALGO_DQN, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(z, z, z, C.DQNX_HEAD_LINEAR, 3, 9, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    L = C.lib()
    assert L.dqnx_eval_row(z.ctypes.data_as(FP), None, z.ctypes.data_as(FP), 0, 3, 0, 0, ctypes.c_float(0), ctypes.c_float(0),
                           ctypes.c_float(0.9), None) == C.DQNX_EINVAL


# ---- refusals that need no GPU ---------------------------------------------------------------------------
def _scratch_bytes(h):
    n = ctypes.c_uint64()
    assert C.lib().dqnx_eval_scratch_bytes(h, ctypes.byref(n)) == 0
    return n.value


def _eval(h, lo, hi, scratch=0x7e0000000000, nbytes=None, rows=None):
    out = C.EvalResult()
    nb = _scratch_bytes(h) if nbytes is None else nbytes
    return C.lib().dqnx_eval_range(h, lo, hi, ctypes.c_void_p(scratch), nb, rows, ctypes.byref(out), None)


def test_eval_range_refusals_without_gpu():
    L = C.lib()
    spec = E.mlp_spec(14, 8, "dueling")
    h = GC._bound(spec, C.DQNX_ALGO_DOUBLE)
    try:
        need = _scratch_bytes(h)
        assert need > 0 and need % 256 == 0
        # the ring is empty: every range is outside it, and so are the malformed ones
        for lo, hi in ((-1, 1), (0, 0), (5, 5), (3, 2), (0, 1), (0, 201)):
            assert _eval(h, lo, hi) == C.DQNX_EINVAL, (lo, hi)
        assert _eval(h, 0, 1, scratch=0) == C.DQNX_EINVAL                      # no scratch
        assert _eval(h, 0, 1, scratch=0x7e0000000010) == C.DQNX_EINVAL         # misaligned
        assert _eval(h, 0, 1, nbytes=need - 1) == C.DQNX_EINVAL                # too small
        assert _eval(h, 0, 1, rows=ctypes.c_void_p(0x7e0000100004)) == C.DQNX_EINVAL   # misaligned per-row output
        assert L.dqnx_eval_range(h, 0, 1, ctypes.c_void_p(0x7e0000000000), need, None, None, None) == C.DQNX_EINVAL
        assert L.dqnx_eval_range(None, 0, 1, ctypes.c_void_p(0x7e0000000000), need, None, ctypes.byref(C.EvalResult()),
                                 None) == C.DQNX_EINVAL
        assert L.dqnx_eval_scratch_bytes(None, ctypes.byref(ctypes.c_uint64())) == C.DQNX_EINVAL
        assert L.dqnx_eval_scratch_bytes(h, None) == C.DQNX_EINVAL
    finally:
        L.dqnx_engine_destroy(h)
    # not bound: DQNX_ESTATE like every launch
    h = LS._unbound(spec, C.DQNX_ALGO_DOUBLE, 32, 200)
    try:
        assert _eval(h, 0, 1) == C.DQNX_ESTATE
    finally:
        L.dqnx_engine_destroy(h)
    # a data-parallel engine: DQNX_EUNSUPPORTED, whatever the range
    cfg = C.Config()
    cfg.net = spec.to_c()
    L.dqnx_config_defaults(ctypes.byref(cfg))
    cfg.algo, cfg.batch, cfg.capacity, cfg.world_size, cfg.rank = C.DQNX_ALGO_DOUBLE, 32, 200, 2, 0
    h = ctypes.c_void_p()
    assert L.dqnx_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    try:
        total = ctypes.c_uint64()
        assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
        assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
        assert _eval(h, 0, 1) == C.DQNX_EUNSUPPORTED
    finally:
        L.dqnx_engine_destroy(h)


# ---- nothing that exists moves ---------------------------------------------------------------------------
def _eval_names(h):
    L = C.lib()
    n = C.I32()
    assert L.dqnx_eval_kernel_count(h, ctypes.byref(n)) == 0
    out = []
    for i in range(n.value):
        name = ctypes.create_string_buffer(64)
        assert L.dqnx_eval_kernel_name(h, i, name, 64) == 0
        out.append(name.value.decode())
    return out


def _make(spec, algo, n_step=1, cql=0.0):
    L = C.lib()
    cfg = C.Config()
    cfg.net = spec.to_c()
    L.dqnx_config_defaults(ctypes.byref(cfg))
    cfg.algo, cfg.batch, cfg.capacity, cfg.n_step = algo, 32, 200, n_step
    h = ctypes.c_void_p()
    assert L.dqnx_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    total = ctypes.c_uint64()
    assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
    assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
    if cql:
        assert L.dqnx_set_cql(h, ctypes.c_double(cql)) == 0
    return h


@pytest.mark.parametrize("net,algo,n_step,cql,env,fwd", [
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, ["mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DQN, 1, 0.0, {}, ["mlp_fwd"]),
    ("mlp284", C.DQNX_ALGO_PER_DOUBLE, 1, 0.0, {}, None),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 3, 0.0, {}, ["nstep_gather", "mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 1.0, {}, ["mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 0.0, {"DQNX_DW_ADAM16": "0"}, ["mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 0.0, {"DQNX_BWD_PLAN": "0"}, ["linear_fwd_l1", "linear_fwd_l2", "eval_head"]),
    ("head", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, None),
    ("head", C.DQNX_ALGO_DOUBLE, 3, 1.0, {}, None),
    ("hybrid84", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, None)])
def test_eval_plan_moves_nothing_that_exists(monkeypatch, net, algo, n_step, cql, env, fwd):
    """The arena size, every buffer region and every planned kernel table (names, FLOPs, bytes) of an engine are
    what they are on an engine that never planned an evaluation; the evaluation's own launch list is eval_idx,
    the route's forward launches (a prefix of the learn step's compute launches), eval_rows, eval_fold."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = C.lib()
    spec = {"mlp14": E.mlp_spec(14, 8, "dueling" if algo != C.DQNX_ALGO_DQN else "linear"),
            "mlp284": E.mlp_spec(284, 8, "dueling"), "head": E.hybrid_spec(8, "dueling"),
            "hybrid84": E.hybrid_spec(8, "dueling", micro_chw=(4, 84, 84))}[net]
    per = algo == C.DQNX_ALGO_PER_DOUBLE
    queried = [f for f in GC.QUERIED if not (per and f & C.STEP_GIVEN_INDICES)]
    h0, h1 = _make(spec, algo, n_step, cql), _make(spec, algo, n_step, cql)
    try:
        before = {f: LS._kernel_names(h1, f) for f in queried}
        regions = LS._regions(h1)
        names = _eval_names(h1)          # plans the evaluation
        assert _scratch_bytes(h1) > 0
        assert LS._regions(h1) == regions == LS._regions(h0)
        for f in queried:
            assert LS._kernel_names(h1, f) == before[f] == LS._kernel_names(h0, f), f
        assert names[0] == "eval_idx" and names[-2:] == ["eval_rows", "eval_fold"]
        mid = names[1:-2]
        if fwd is not None:
            assert mid == fwd, names
        # the forward launches are the learn step's own, in its order, cut before the head kernel
        step = [n for n, _, _ in before[0]][1:]   # (behind the sampler launch)
        core = [n for n in mid if n != "eval_head"]
        assert core == step[:len(core)], (names, step)
        assert step[len(core)] in ("head_bwd", "head_td_loss"), step
        assert ("eval_head" in mid) == (step[len(core)] == "head_td_loss")
        assert not any("sample" in n for n in names)
    finally:
        L.dqnx_engine_destroy(h0)
        L.dqnx_engine_destroy(h1)
