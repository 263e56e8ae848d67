"""CPU checks of the fitted-Q-evaluation ABI (include/dqnx.h "fitted Q evaluation" <-> libdqnx.so <-> dqn/_capi.py):
the new exports with every pinned layout and the ABI version unchanged, dqnx_fqe_result's layout against gcc, the
row arithmetic of csrc/fqe.hpp (dqnx_fqe_row) against a float64 restatement, every refusal that needs no GPU, and
the arena and planned kernel tables, which planning the sweeps must not move and which a target-policy table
turns into the DQN stream set's.  No GPU calls: planning binds an address that is never dereferenced."""
import ctypes
import re

import numpy as np
import pytest

from dqn import _capi as C
from dqn import engine as E
import test_grad_clip_capi as GC

LS = GC.LS
NEW = ("dqnx_policy_scratch_bytes", "dqnx_policy_sweep", "dqnx_set_target_policy", "dqnx_get_target_policy",
       "dqnx_fqe_range", "dqnx_fqe_row", "dqnx_fqe_kernel_count", "dqnx_fqe_kernel_name", "dqnx_fqe_chunk_timed")
FP = ctypes.POINTER(ctypes.c_float)
SCRATCH, TABLE = 0x7e0000000000, 0x7d0000000000   # addresses that are never dereferenced


def test_fqe_symbols_abi_and_layouts(tmp_path):
    L = C.lib()
    src = re.sub(r"/\*.*?\*/", "", open(LS.HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in C.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    sizes = {"dqnx_config": C.Config, "dqnx_ctrl": C.Ctrl, "dqnx_net_desc": C.NetDesc, "dqnx_state_info": C.StateInfo,
             "dqnx_learn_stats": C.LearnStats, "dqnx_grad_clip_info": C.GradClipInfo, "dqnx_eval_result": C.EvalResult,
             "dqnx_eval_row_result": C.EvalRowResult}
    got = LS._gcc_values(tmp_path, {"abi": "DQNX_ABI_VERSION", "count": "DQNX_BUF_COUNT", "deverr": "DQNX_DEVERR_TPOL_ACTION",
                                    **{k: f"sizeof({k})" for k in sizes}})
    assert got["abi"] == 5 == L.dqnx_abi_version()   # new symbols only: the version stays
    assert got["count"] == C.BUF_COUNT == 20
    assert got["deverr"] == C.DEVERR_TPOL_ACTION == 20
    assert {k: got[k] for k in sizes} == {"dqnx_config": 288, "dqnx_ctrl": 5136, "dqnx_net_desc": 148,
                                          "dqnx_state_info": 608, "dqnx_learn_stats": 1312, "dqnx_grad_clip_info": 40,
                                          "dqnx_eval_result": 376, "dqnx_eval_row_result": 40}
    for k, py in sizes.items():
        assert ctypes.sizeof(py) == got[k], k


@pytest.mark.parametrize("cname,py,size", [("dqnx_fqe_result", C.FqeResult, 64), ("dqnx_fqe_row_result", C.FqeRowResult, 32)])
def test_fqe_struct_layouts_match_gcc(tmp_path, cname, py, size):
    exprs = {"sizeof": f"sizeof({cname})"}
    for fname, _ in py._fields_:
        exprs[fname] = f"offsetof({cname}, {fname})"
    got = LS._gcc_values(tmp_path, exprs)
    assert ctypes.sizeof(py) == got["sizeof"] == size
    for fname, _ in py._fields_:
        assert getattr(py, fname).offset == got[fname], fname
    assert sum(ctypes.sizeof(t) for _, t in py._fields_) == got["sizeof"]   # no padding
    if py is C.FqeResult:
        assert [f for f, _ in py._fields_] == ["rows", "start_rows", "q_pi_sum", "q_pi_start_sum", "abs_td_sum",
                                               "huber_sum", "q_pi_max", "q_pi_min"]


# ---- dqnx_fqe_row against float64 ------------------------------------------------------------------------
def _row(raw0, raw2, rawp, rawpn, head, A, act, rew, done, gamma):
    arrs = [None if r is None else np.ascontiguousarray(r, dtype=np.float32) for r in (raw0, raw2, rawp, rawpn)]
    ptrs = [None if a is None else a.ctypes.data_as(FP) for a in arrs]
    out = C.FqeRowResult()
    rc = C.lib().dqnx_fqe_row(ptrs[0], ptrs[1], ptrs[2], ptrs[3], head, A, act, ctypes.c_float(rew), ctypes.c_float(done),
                              ctypes.c_float(gamma), ctypes.byref(out))
    return rc, out


def _q64(raw, head, A):
    raw = np.asarray(raw, dtype=np.float32).astype(np.float64)
    if head == C.DQNX_HEAD_DUELING:
        return raw[0] + (raw[1:1 + A] - raw[1:1 + A].mean())
    return raw[:A].copy()


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
def test_fqe_row_matches_float64(A, head):
    if head == C.DQNX_HEAD_DUELING and A == 16:
        # a dueling head has V + A advantages in the 16 head slots: 15 actions at most; the hook says so
        z = np.zeros(17)
        assert _row(z, z, z, z, head, 16, 0, 0.0, 0.0, 0.99)[0] == C.DQNX_EINVAL
        return
    NH = A + 1 if head == C.DQNX_HEAD_DUELING else A
    raws = _raws(NH, 3000 + 17 * A + head)
    rng = np.random.default_rng(91 + A)
    f = lambda x: float(np.float32(x))
    n_checked = 0
    for i, raw0 in enumerate(raws):
        raw2, rawp, rawpn = raws[(i + 5) % len(raws)], raws[(i + 2) % len(raws)], raws[(i + 7) % len(raws)]
        for act in {0, A - 1}:
            rew, done, gamma = float(rng.normal()), float(i % 3 == 0), 0.99
            rc, out = _row(raw0, raw2, rawp, rawpn, head, A, act, rew, done, gamma)
            assert rc == 0
            q0, q2, qp, qpn = (_q64(r, head, A) for r in (raw0, raw2, rawp, rawpn))
            # integers: exact.  pi is the FIRST maximum of the fp32 row the library forms; where the fp32 row has
            # distinct entries (or is all-equal: the tie rule itself) float64 -> fp32 rounding cannot reorder it
            for got, q in ((out.pi_s, qp), (out.pi_next, qpn)):
                q32 = q.astype(np.float32)
                if np.unique(q32).size == A or np.all(q32 == q32[0]):
                    assert got == int(np.argmax(q32)), (A, head, q32)
                assert 0 <= got < A
            for raw, got in ((rawp, out.pi_s), (rawpn, out.pi_next)):
                if np.all(np.asarray(raw) == np.asarray(raw)[0]):
                    assert got == 0
            # floats: against float64 at the library's own pi (checked above), 4e-6 at the row's magnitude
            qn = q2[out.pi_next]
            y = f(rew) + (1.0 - f(done)) * f(gamma) * qn
            delta = y - q0[act]
            z = abs(delta)
            lb = 0.5 * z * z if z < 1.0 else z - 0.5
            scale = max(1.0, np.abs(np.asarray(raw0)).max(), abs(y), abs(qn))
            tol = 4e-6 * scale
            assert abs(out.q_pi - q0[out.pi_s]) <= tol
            assert abs(out.y - y) <= tol
            assert abs(out.delta - delta) <= 2 * tol
            assert abs(out.huber - lb) <= 2 * tol
            assert out.reserved0 == 0.0 and out.reserved1 == 0.0
            n_checked += 1
    assert n_checked >= 14


def test_fqe_row_exact_cases_and_refusals():
    lin = C.DQNX_HEAD_LINEAR
    # pi(s) = 1 (first of the two maxima), pi(s') = 0 (all equal): y = 1 + 0.5 * 10, delta = y - q0[act]
    rc, out = _row([1.0, 5.0, 2.0], [10.0, 20.0, 30.0], [0.0, 7.0, 7.0], [3.0, 3.0, 3.0], lin, 3, 2, 1.0, 0.0, 0.5)
    assert rc == 0 and (out.pi_s, out.pi_next) == (1, 0)
    assert out.q_pi == 5.0 and out.y == 6.0 and out.delta == 4.0 and out.huber == 3.5
    # done cuts the bootstrap; a small delta takes the quadratic branch
    rc, out = _row([1.0, 5.0, 2.0], [10.0, 20.0, 30.0], [0.0, 7.0, 7.0], [3.0, 3.0, 9.0], lin, 3, 0, 1.5, 1.0, 0.5)
    assert rc == 0 and out.pi_next == 2 and out.y == 1.5 and out.delta == 0.5 and out.huber == 0.125
    # dueling: V + (A_j - mean A); the policy's V does not move its argmax
    rc, out = _row([1.0, 2.0, 4.0], [0.0, 1.0, 3.0], [100.0, 0.0, 1.0], [-100.0, 2.0, 1.0], C.DQNX_HEAD_DUELING, 2, 0,
                   0.0, 0.0, 1.0)
    assert rc == 0 and (out.pi_s, out.pi_next) == (1, 0) and out.q_pi == 2.0 and out.y == -1.0 and out.delta == -1.0
    # an action outside [0, A) is taken as 0
    a = _row([0.3, -1.0, 2.0], [0.1, 0.2, 0.3], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], lin, 3, 0, 0.5, 0.0, 0.9)[1]
    for bad in (-1, 3, 99):
        b = _row([0.3, -1.0, 2.0], [0.1, 0.2, 0.3], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], lin, 3, bad, 0.5, 0.0, 0.9)[1]
        assert bytes(a) == bytes(b)
    z = np.zeros(17, dtype=np.float32)
    for A in (0, -1, 17):
        assert _row(z, z, z, z, lin, A, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    for k in range(4):
        args = [z, z, z, z]
        args[k] = None
        assert _row(*args, lin, 3, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    assert _row(z, z, z, z, 7, 3, 0, 0.0, 0.0, 0.9)[0] == C.DQNX_EINVAL
    p = z.ctypes.data_as(FP)
    assert C.lib().dqnx_fqe_row(p, p, p, p, 0, 3, 0, ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0.9),
                                None) == C.DQNX_EINVAL


# ---- refusals that need no GPU ---------------------------------------------------------------------------
def _make(spec, algo, n_step=1, cql=0.0, world=1, batch=32, cap=200, bind=True):
    L = C.lib()
    cfg = C.Config()
    cfg.net = spec.to_c()
    L.dqnx_config_defaults(ctypes.byref(cfg))
    cfg.algo, cfg.batch, cfg.capacity, cfg.n_step, cfg.world_size, cfg.rank = algo, batch, cap, n_step, world, 0
    h = ctypes.c_void_p()
    assert L.dqnx_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    if bind:
        total = ctypes.c_uint64()
        assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
        assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
    if cql:
        assert L.dqnx_set_cql(h, ctypes.c_double(cql)) == 0
    return h


def _last_error():
    L = C.lib()
    L.dqnx_last_error.restype = ctypes.c_char_p
    return L.dqnx_last_error().decode()


def _set(h, table=TABLE, slots=200):
    return C.lib().dqnx_set_target_policy(h, ctypes.c_void_p(table) if table else None, slots)


def _get(h):
    t, n = ctypes.c_void_p(), C.I64()
    assert C.lib().dqnx_get_target_policy(h, ctypes.byref(t), ctypes.byref(n)) == 0
    return t.value, n.value


def test_set_target_policy_refusals_without_gpu():
    L = C.lib()
    spec = E.mlp_spec(14, 8, "dueling")
    dbl = C.DQNX_ALGO_DOUBLE
    # CQL, in both orders of the two setters
    h = _make(spec, dbl, cql=1.0)
    try:
        assert _set(h) == C.DQNX_EUNSUPPORTED and "CQL" in _last_error()
        assert _get(h) == (None, 0)
        assert L.dqnx_set_cql(h, ctypes.c_double(0.0)) == 0
        assert _set(h) == 0 and _get(h) == (TABLE, 200)
        assert L.dqnx_set_cql(h, ctypes.c_double(0.5)) == C.DQNX_EUNSUPPORTED and "target-policy" in _last_error()
        alpha = ctypes.c_double(-1)
        assert L.dqnx_get_cql(h, ctypes.byref(alpha)) == 0 and alpha.value == 0.0
        assert L.dqnx_set_cql(h, ctypes.c_double(0.0)) == 0       # off stays allowed
        assert _set(h, None, 0) == 0 and _get(h) == (None, 0)
        assert L.dqnx_set_cql(h, ctypes.c_double(0.5)) == 0
    finally:
        L.dqnx_engine_destroy(h)
    # n_step = 3
    h = _make(spec, dbl, n_step=3)
    try:
        assert _set(h) == C.DQNX_EUNSUPPORTED and "n-step" in _last_error() and "behaviour policy" in _last_error()
        assert _get(h) == (None, 0)
        assert _set(h, None, 0) == 0
    finally:
        L.dqnx_engine_destroy(h)
    # world 2: the setter and both sweeps
    h = _make(spec, dbl, world=2)
    try:
        assert _set(h) == C.DQNX_EUNSUPPORTED and "world_size" in _last_error()
        assert L.dqnx_policy_sweep(h, 0, 1, ctypes.c_void_p(SCRATCH), 1 << 20, ctypes.c_void_p(TABLE), 200,
                                   None) == C.DQNX_EUNSUPPORTED
        assert L.dqnx_fqe_range(h, 0, 1, ctypes.c_void_p(SCRATCH), 1 << 20, ctypes.c_void_p(TABLE), 200, None,
                                ctypes.byref(C.FqeResult()), None) == C.DQNX_EUNSUPPORTED
    finally:
        L.dqnx_engine_destroy(h)
    # table_slots != capacity, a misaligned table, a null engine; an unbound engine takes the setting (like lr)
    h = _make(spec, dbl, bind=False)
    try:
        for slots in (0, 199, 201, -1):
            assert _set(h, TABLE, slots) == C.DQNX_EINVAL and "capacity" in _last_error()
        assert _set(h, TABLE + 4, 200) == C.DQNX_EINVAL
        assert _set(None) == C.DQNX_EINVAL
        assert _get(h) == (None, 0)
        assert _set(h) == 0 and _get(h) == (TABLE, 200)
        assert _set(h) == 0                                       # the same table again: nothing to do
    finally:
        L.dqnx_engine_destroy(h)


def test_push_and_state_load_refused_while_a_table_is_set():
    L = C.lib()
    spec = E.mlp_spec(14, 8, "dueling")
    h = _make(spec, C.DQNX_ALGO_DOUBLE)
    try:
        obs = np.zeros((2, 14), dtype=np.float32)
        act = np.zeros(2, dtype=np.int32)
        rew = np.zeros(2, dtype=np.float32)
        done = np.zeros(2, dtype=np.uint8)
        push = lambda: L.dqnx_replay_push(h, ctypes.c_void_p(obs.ctypes.data), ctypes.c_void_p(act.ctypes.data),
                                          ctypes.c_void_p(rew.ctypes.data), ctypes.c_void_p(done.ctypes.data),
                                          ctypes.c_void_p(obs.ctypes.data), 2, 0, None)
        assert _set(h) == 0
        assert push() == C.DQNX_ESTATE and "target-policy table" in _last_error()
        blob = np.zeros(64, dtype=np.uint8)
        assert L.dqnx_state_load(h, ctypes.c_void_p(blob.ctypes.data), blob.nbytes, None) == C.DQNX_ESTATE
        assert "target-policy table" in _last_error()
        assert _set(h, None, 0) == 0
        # (cleared: the blob is now looked at -- and refused for what it is, not for the table)
        rc = L.dqnx_state_load(h, ctypes.c_void_p(blob.ctypes.data), blob.nbytes, None)
        assert rc != 0 and "target-policy table" not in _last_error()
    finally:
        L.dqnx_engine_destroy(h)


def _sweep(h, which, lo, hi, scratch=SCRATCH, nbytes=None, table=TABLE, slots=200, rows=None):
    L = C.lib()
    if nbytes is None:
        n = ctypes.c_uint64()
        assert L.dqnx_policy_scratch_bytes(h, ctypes.byref(n)) == 0
        nbytes = n.value
    t = ctypes.c_void_p(table) if table else None
    if which == 0:
        return L.dqnx_policy_sweep(h, lo, hi, ctypes.c_void_p(scratch), nbytes, t, slots, None)
    return L.dqnx_fqe_range(h, lo, hi, ctypes.c_void_p(scratch), nbytes, t, slots, rows, ctypes.byref(C.FqeResult()), None)


@pytest.mark.parametrize("which", [0, 1])
def test_sweep_refusals_without_gpu(which):
    """dqnx_eval_range's refusals, plus DQNX_EINVAL for table_slots != capacity."""
    L = C.lib()
    spec = E.mlp_spec(14, 8, "dueling")
    h = _make(spec, C.DQNX_ALGO_DOUBLE)
    try:
        need, need_eval = ctypes.c_uint64(), ctypes.c_uint64()
        assert L.dqnx_policy_scratch_bytes(h, ctypes.byref(need)) == 0
        assert L.dqnx_eval_scratch_bytes(h, ctypes.byref(need_eval)) == 0
        assert need.value == need_eval.value > 0
        for lo, hi in ((-1, 1), (0, 0), (3, 2), (0, 1), (0, 201)):   # the ring is empty: every range is outside it
            assert _sweep(h, which, lo, hi) == C.DQNX_EINVAL, (lo, hi)
        for slots in (0, 199, 201):
            assert _sweep(h, which, 0, 1, slots=slots) == C.DQNX_EINVAL and "capacity" in _last_error()
        assert _sweep(h, which, 0, 1, table=0) == C.DQNX_EINVAL
        assert _sweep(h, which, 0, 1, table=TABLE + 4) == C.DQNX_EINVAL
        assert _sweep(h, which, 0, 1, scratch=0) == C.DQNX_EINVAL
        assert _sweep(h, which, 0, 1, scratch=SCRATCH + 16) == C.DQNX_EINVAL
        assert _sweep(h, which, 0, 1, nbytes=need.value - 1) == C.DQNX_EINVAL
        if which == 1:
            assert _sweep(h, 1, 0, 1, rows=ctypes.c_void_p(0x7e0000100004)) == C.DQNX_EINVAL
            assert L.dqnx_fqe_range(h, 0, 1, ctypes.c_void_p(SCRATCH), need.value, ctypes.c_void_p(TABLE), 200, None, None,
                                    None) == C.DQNX_EINVAL
    finally:
        L.dqnx_engine_destroy(h)
    h = _make(spec, C.DQNX_ALGO_DOUBLE, bind=False)   # not bound: DQNX_ESTATE like every launch
    try:
        assert _sweep(h, which, 0, 1) == C.DQNX_ESTATE
    finally:
        L.dqnx_engine_destroy(h)


def test_policy_sweep_refused_on_a_two_stream_conv_engine():
    """The sweep runs the Double stream set; a DQNAgent conv engine's split-K plans are sized for two streams and the
    arena does not grow for it.  The value sweep (two streams) is not refused for that."""
    L = C.lib()
    h = _make(E.hybrid_spec(8, "linear"), C.DQNX_ALGO_DQN)
    try:
        assert _sweep(h, 0, 0, 1) == C.DQNX_EUNSUPPORTED and "two streams" in _last_error()
        assert _sweep(h, 1, 0, 1) == C.DQNX_EINVAL        # (the empty ring)
        n = C.I32()
        assert L.dqnx_fqe_kernel_count(h, 0, ctypes.byref(n)) == C.DQNX_EUNSUPPORTED
        assert L.dqnx_fqe_kernel_count(h, 1, ctypes.byref(n)) == 0 and n.value > 3
    finally:
        L.dqnx_engine_destroy(h)


# ---- nothing that exists moves; a table turns the step into the DQN stream set's -------------------------
def _fqe_names(h, which):
    L = C.lib()
    n = C.I32()
    assert L.dqnx_fqe_kernel_count(h, which, ctypes.byref(n)) == 0
    out = []
    for i in range(n.value):
        name = ctypes.create_string_buffer(64)
        assert L.dqnx_fqe_kernel_name(h, which, i, name, 64) == 0
        out.append(name.value.decode())
    return out


SPECS = {"mlp14": lambda algo: E.mlp_spec(14, 8, "dueling" if algo != C.DQNX_ALGO_DQN else "linear"),
         "mlp284": lambda algo: E.mlp_spec(284, 8, "dueling"), "head": lambda algo: E.hybrid_spec(8, "dueling"),
         "hybrid84": lambda algo: E.hybrid_spec(8, "dueling", micro_chw=(4, 84, 84))}


@pytest.mark.parametrize("net,algo,n_step,cql,env,fwd", [
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, ["mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DQN, 1, 0.0, {}, ["mlp_fwd"]),
    ("mlp284", C.DQNX_ALGO_PER_DOUBLE, 1, 0.0, {}, None),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 3, 0.0, {}, ["mlp_fwd"]),          # 1-step rows: no nstep_gather
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 1.0, {}, ["mlp_fwd"]),
    ("mlp14", C.DQNX_ALGO_DOUBLE, 1, 0.0, {"DQNX_BWD_PLAN": "0"}, ["linear_fwd_l1", "linear_fwd_l2", "eval_head"]),
    ("head", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, None),
    ("hybrid84", C.DQNX_ALGO_DOUBLE, 1, 0.0, {}, None)])
def test_sweep_plans_move_nothing_that_exists(monkeypatch, net, algo, n_step, cql, env, fwd):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = C.lib()
    spec = SPECS[net](algo)
    per = algo == C.DQNX_ALGO_PER_DOUBLE
    queried = [f for f in GC.QUERIED if not (per and f & C.STEP_GIVEN_INDICES)]
    h0, h1 = _make(spec, algo, n_step, cql), _make(spec, algo, n_step, cql)
    try:
        before = {f: LS._kernel_names(h1, f) for f in queried}
        regions = LS._regions(h1)
        pol, val = _fqe_names(h1, 0), _fqe_names(h1, 1)     # plans both sweeps
        assert LS._regions(h1) == regions == LS._regions(h0)
        for f in queried:
            assert LS._kernel_names(h1, f) == before[f] == LS._kernel_names(h0, f), f
        assert pol[0] == val[0] == "eval_idx" and pol[-1] == "policy_rows" and val[-2:] == ["fqe_rows", "fqe_fold"]
        assert pol[1:-1] == val[1:-2]                       # the same forward launches, another stream set
        assert "nstep_gather" not in pol and not any("sample" in n for n in pol + val)
        if fwd is not None:
            assert pol[1:-1] == fwd, pol
    finally:
        L.dqnx_engine_destroy(h0)
        L.dqnx_engine_destroy(h1)


@pytest.mark.parametrize("net,env", [("mlp14", {}), ("mlp284", {}), ("mlp14", {"DQNX_BWD_PLAN": "0"})])
def test_table_turns_the_forward_into_the_dqn_engines(monkeypatch, net, env):
    """With a table set on a DuelingDoubleDQNAgent engine the plan's forward entries have the stream count (FLOPs)
    and bytes of the DQNAgent engine's of the same network; every other launch keeps its name; clearing the table
    restores the Double plan."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = C.lib()
    spec = E.mlp_spec(14 if net == "mlp14" else 284, 8, "dueling")
    hd, hq = _make(spec, C.DQNX_ALGO_DOUBLE), _make(spec, C.DQNX_ALGO_DQN)
    try:
        for f in (0, C.STEP_SOFT_UPDATE, C.STEP_PREFETCH, C.STEP_GIVEN_INDICES):
            double, dqn = LS._kernel_names(hd, f), LS._kernel_names(hq, f)
            assert _set(hd) == 0
            tpol = LS._kernel_names(hd, f)
            assert _set(hd, None, 0) == 0
            assert LS._kernel_names(hd, f) == double, f
            assert [n for n, _, _ in tpol] == [n for n, _, _ in double] == [n for n, _, _ in dqn]
            moved = 0
            for t, d, q in zip(tpol, double, dqn):
                if "fwd" in t[0]:
                    assert t == q, (t, q)                       # the DQN engine's entry: name, FLOPs, bytes
                    assert t[1] * 3 == pytest.approx(d[1] * 2)   # two streams' FLOPs of the Double plan's three
                    moved += 1
                elif t[0] == "head_td_loss":
                    assert t == q and t != d                     # (its table counts the streams' H_L rows)
                else:
                    assert t == d, (t, d)
            assert moved >= 1
    finally:
        L.dqnx_engine_destroy(hd)
        L.dqnx_engine_destroy(hq)
