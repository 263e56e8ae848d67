"""CPU checks of the training-statistics ABI (include/dqnx.h "training statistics" <-> libdqnx.so <->
dqn/_capi.py): the dqnx_learn_stats layout against gcc, the new exports, the arena region of an unbound
engine, and the buffer ids that existed before it.  No GPU calls."""
import ctypes
import os
import re
import subprocess

from dqn import _capi as C
from dqn import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dqnx.h")

# enum dqnx_buffer as it stood at ABI 4: these ids are in callers' binaries
ABI4_BUFFERS = ["PARAMS", "TARGET_PARAMS", "GRADS", "ADAM_M", "ADAM_V", "CTRL", "RING_OBS", "RING_NEXT_OBS",
                "RING_ACT", "RING_REW", "RING_DONE", "SUMTREE", "BATCH_IDX", "Q", "TD", "IS_WEIGHTS", "WORKSPACE",
                "PER_ABS_TD"]


def _gcc_values(tmp_path, exprs):
    """name -> value of integer C expressions over the header, as gcc evaluates them"""
    prog = tmp_path / "stats_abi.c"
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {"]
    for name, ex in exprs.items():
        lines.append(f'printf("{name} %lld\\n", (long long)({ex}));')
    lines += ["return 0;", "}"]
    prog.write_text("\n".join(lines))
    exe = tmp_path / "stats_abi"
    subprocess.check_call(["gcc", "-std=c11", "-o", str(exe), str(prog)])
    out = subprocess.check_output([str(exe)]).decode().split("\n")
    return {ln.split()[0]: int(ln.split()[1]) for ln in out if ln}


def test_learn_stats_layout_matches_gcc(tmp_path):
    exprs = {"sizeof": "sizeof(dqnx_learn_stats)"}
    for fname, _ in C.LearnStats._fields_:
        exprs[fname] = f"offsetof(dqnx_learn_stats, {fname})"
    got = _gcc_values(tmp_path, exprs)
    assert ctypes.sizeof(C.LearnStats) == got["sizeof"]
    for fname, _ in C.LearnStats._fields_:
        assert getattr(C.LearnStats, fname).offset == got[fname], fname
    # every byte of the struct is a declared field (no padding a memset-to-zero reader could trip on)
    assert sum(ctypes.sizeof(t) for _, t in C.LearnStats._fields_) == got["sizeof"]


def test_learn_stats_constants_match_header(tmp_path):
    got = _gcc_values(tmp_path, {"abi": "DQNX_ABI_VERSION", "flag": "DQNX_STEP_STATS", "acts": "DQNX_STATS_MAX_ACTIONS",
                                 "bins": "DQNX_STATS_TD_BINS", "tensors": "DQNX_STATS_MAX_TENSORS",
                                 "buf": "DQNX_BUF_LEARN_STATS", "count": "DQNX_BUF_COUNT"})
    assert got["abi"] == 5 == C.lib().dqnx_abi_version()
    assert got["flag"] == 0x10 == C.STEP_STATS
    assert (got["acts"], got["bins"], got["tensors"]) == (C.STATS_MAX_ACTIONS, C.STATS_TD_BINS, C.STATS_MAX_TENSORS) \
        == (16, 16, 32)
    assert got["buf"] == C.BUF_LEARN_STATS and got["count"] == C.BUF_COUNT
    # the flag is a bit of its own among the step flags
    assert C.STEP_STATS & (C.STEP_SOFT_UPDATE | C.STEP_GIVEN_INDICES | C.STEP_GRADS_ONLY | C.STEP_PREFETCH
                           | C.AGENT_LAUNCH) == 0


def test_learn_stats_symbols_exported():
    L = C.lib()
    for name in ("dqnx_learn_stats_get", "dqnx_learn_stats_reset"):
        assert hasattr(L, name), name
        assert name in C.EXPORTS
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+dqnx_learn_stats_get\s*\(", src) and re.search(r"\bint\s+dqnx_learn_stats_reset\s*\(", src)


def test_earlier_buffer_ids_unchanged(tmp_path):
    got = _gcc_values(tmp_path, {n: "DQNX_BUF_" + n for n in ABI4_BUFFERS + ["LEARN_STATS"]})
    for i, n in enumerate(ABI4_BUFFERS):
        assert got[n] == i == getattr(C, "BUF_" + n), n
    assert got["LEARN_STATS"] == len(ABI4_BUFFERS)   # appended after DQNX_BUF_PER_ABS_TD


def _unbound(spec, algo, batch, cap):
    cfg = C.Config()
    cfg.net = spec.to_c()
    C.lib().dqnx_config_defaults(ctypes.byref(cfg))
    cfg.algo, cfg.batch, cfg.capacity = algo, batch, cap
    h = ctypes.c_void_p()
    assert C.lib().dqnx_engine_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    return h


def _regions(h):
    out = {}
    for b in range(C.BUF_COUNT):
        o, n = ctypes.c_uint64(), ctypes.c_uint64()
        assert C.lib().dqnx_engine_buffer(h, b, ctypes.byref(o), ctypes.byref(n)) == 0
        out[b] = (o.value, n.value)
    return out


def test_learn_stats_region_in_an_unbound_engines_plan():
    L = C.lib()
    for spec, algo in ((E.mlp_spec(284, 8, "dueling"), C.DQNX_ALGO_DOUBLE), (E.mlp_spec(14, 3, "linear"), C.DQNX_ALGO_DQN),
                       (E.mlp_spec(284, 8, "dueling"), C.DQNX_ALGO_PER_DOUBLE), (E.hybrid_spec(8, "dueling"), C.DQNX_ALGO_DOUBLE)):
        h = _unbound(spec, algo, 64, 1000)
        try:
            reg = _regions(h)
            total = ctypes.c_uint64()
            assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
            off, n = reg[C.BUF_LEARN_STATS]
            assert n == ctypes.sizeof(C.LearnStats)
            assert off % 256 == 0 and off + n <= total.value
            # disjoint from every other region
            for b, (o, m) in reg.items():
                if b != C.BUF_LEARN_STATS and m:
                    assert o + m <= off or off + n <= o, b
            # the new entry points refuse an unbound engine like the other device calls
            st = C.LearnStats()
            assert L.dqnx_learn_stats_get(h, ctypes.byref(st), 0, None) == C.DQNX_ESTATE
            assert L.dqnx_learn_stats_reset(h, None) == C.DQNX_ESTATE
        finally:
            L.dqnx_engine_destroy(h)


def _kernel_names(h, flags):
    L = C.lib()
    n = C.I32()
    rc = L.dqnx_learn_kernel_count(h, flags, ctypes.byref(n))
    if rc:
        return rc
    out = []
    for i in range(n.value):
        name, fl, by = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_double()
        assert L.dqnx_learn_kernel_info(h, flags, i, name, 64, ctypes.byref(fl), ctypes.byref(by)) == 0
        out.append((name.value.decode(), fl.value, by.value))
    return out


def test_learn_stats_launch_in_the_planned_kernel_table():
    """Planning needs no GPU: bound to an address that is never dereferenced, the step's kernel table
    gains exactly one entry, the last, under DQNX_STEP_STATS, and is unchanged without it."""
    L = C.lib()
    for spec, flag_sets in ((E.mlp_spec(14, 8, "dueling"), (0, C.STEP_SOFT_UPDATE, C.STEP_PREFETCH)),
                            (E.hybrid_spec(8, "dueling"), (0, C.STEP_SOFT_UPDATE))):
        h = _unbound(spec, C.DQNX_ALGO_DOUBLE, 32, 200)
        try:
            total = ctypes.c_uint64()
            assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
            assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
            n_params, _ = spec.param_infos()
            for flags in flag_sets:
                off, on = _kernel_names(h, flags), _kernel_names(h, flags | C.STEP_STATS)
                assert on[:-1] == off
                name, flops, nbytes = on[-1]
                assert name == "learn_stats" and flops == 0 and nbytes >= 8 * n_params
            assert _kernel_names(h, C.STEP_STATS | C.STEP_GRADS_ONLY) == C.DQNX_EUNSUPPORTED
            assert b"GRADS_ONLY" in L.dqnx_last_error()
        finally:
            L.dqnx_engine_destroy(h)
