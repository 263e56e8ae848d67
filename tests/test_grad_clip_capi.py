"""CPU checks of the gradient-clipping ABI (include/dqnx.h "gradient clipping" <-> libdqnx.so <->
dqn/_capi.py): the dqnx_grad_clip_info layout against gcc, the new exports, the arena region, the
set / get round trip, the refusals that need no device, and the planned kernel tables with clipping
off (unchanged) and on (the launches that run).  No GPU calls: planning binds an address that is never
dereferenced."""
import ctypes
import math
import re

import pytest

from dqn import _capi as C
from dqn import engine as E
import test_learn_stats_capi as LS

NEW = ("dqnx_set_grad_clip", "dqnx_get_grad_clip", "dqnx_grad_clip_info_get")
TAIL = ["grad_sumsq", "clip_coef", "adam_clipped"]
PER_TAIL = ["grad_sumsq", "clip_coef", "per_update", "adam_clipped"]


def test_grad_clip_info_layout_matches_gcc(tmp_path):
    exprs = {"sizeof": "sizeof(dqnx_grad_clip_info)"}
    for fname, _ in C.GradClipInfo._fields_:
        exprs[fname] = f"offsetof(dqnx_grad_clip_info, {fname})"
    got = LS._gcc_values(tmp_path, exprs)
    assert ctypes.sizeof(C.GradClipInfo) == got["sizeof"] == 40
    for fname, _ in C.GradClipInfo._fields_:
        assert getattr(C.GradClipInfo, fname).offset == got[fname], fname
    assert sum(ctypes.sizeof(t) for _, t in C.GradClipInfo._fields_) == got["sizeof"]   # no padding
    assert [f for f, _ in C.GradClipInfo._fields_] == ["steps", "clipped_steps", "norm_sum", "norm_max", "last_norm",
                                                       "last_coef"]


def test_grad_clip_symbols_abi_and_buffer_ids(tmp_path):
    L = C.lib()
    src = re.sub(r"/\*.*?\*/", "", open(LS.HEADER).read(), flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert name in C.EXPORTS
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
    got = LS._gcc_values(tmp_path, {"abi": "DQNX_ABI_VERSION", "clip": "DQNX_BUF_GRAD_CLIP", "stats": "DQNX_BUF_LEARN_STATS",
                                    "count": "DQNX_BUF_COUNT",
                                    **{n: "DQNX_BUF_" + n for n in LS.ABI4_BUFFERS}})
    assert got["abi"] == 5 == L.dqnx_abi_version()   # new symbols only: the version stays
    for i, n in enumerate(LS.ABI4_BUFFERS):
        assert got[n] == i
    assert got["stats"] == C.BUF_LEARN_STATS == len(LS.ABI4_BUFFERS)
    assert got["clip"] == C.BUF_GRAD_CLIP == got["stats"] + 1 and got["count"] == C.BUF_COUNT == got["clip"] + 1


def test_existing_struct_sizes_unchanged(tmp_path):
    """dqnx_config, dqnx_ctrl, dqnx_net_desc, dqnx_state_info and dqnx_learn_stats keep their layout."""
    pairs = {"dqnx_config": C.Config, "dqnx_ctrl": C.Ctrl, "dqnx_net_desc": C.NetDesc, "dqnx_state_info": C.StateInfo,
             "dqnx_learn_stats": C.LearnStats}
    got = LS._gcc_values(tmp_path, {k: f"sizeof({k})" for k in pairs})
    assert got == {"dqnx_config": 288, "dqnx_ctrl": 5136, "dqnx_net_desc": 148, "dqnx_state_info": 608,
                   "dqnx_learn_stats": 1312}   # as gcc sizes them in the header before this section existed
    for k, t in pairs.items():
        assert ctypes.sizeof(t) == got[k], k


def test_grad_clip_set_get_round_trip():
    L = C.lib()
    h = LS._unbound(E.mlp_spec(14, 8, "dueling"), C.DQNX_ALGO_DOUBLE, 32, 200)
    try:
        v = ctypes.c_double(-1.0)
        assert L.dqnx_get_grad_clip(h, ctypes.byref(v)) == 0 and v.value == 0.0   # off is the default
        for given, want in ((10.0, 10.0), (0.37, 0.37), (0.0, 0.0), (1e30, 1e30), (-3.0, 0.0), (2.5, 2.5)):
            assert L.dqnx_set_grad_clip(h, ctypes.c_double(given)) == 0   # host only: an unbound engine takes it
            assert L.dqnx_get_grad_clip(h, ctypes.byref(v)) == 0 and v.value == want
        assert L.dqnx_set_grad_clip(h, ctypes.c_double(math.nan)) == C.DQNX_EINVAL
        assert L.dqnx_get_grad_clip(h, ctypes.byref(v)) == 0 and v.value == 2.5
        assert L.dqnx_set_grad_clip(None, ctypes.c_double(1.0)) == C.DQNX_EINVAL
        assert L.dqnx_get_grad_clip(h, None) == C.DQNX_EINVAL
        # the device read refuses an unbound engine like the other device calls
        assert L.dqnx_grad_clip_info_get(h, ctypes.byref(C.GradClipInfo()), 0, None) == C.DQNX_ESTATE
    finally:
        L.dqnx_engine_destroy(h)


def test_grad_clip_region_lies_after_the_existing_ones():
    L = C.lib()
    for spec, algo in ((E.mlp_spec(284, 8, "dueling"), C.DQNX_ALGO_DOUBLE), (E.mlp_spec(14, 3, "linear"), C.DQNX_ALGO_DQN),
                       (E.mlp_spec(284, 8, "dueling"), C.DQNX_ALGO_PER_DOUBLE), (E.hybrid_spec(8, "dueling"), C.DQNX_ALGO_DOUBLE),
                       (E.hybrid_spec(8, "dueling", micro_chw=(4, 84, 84)), C.DQNX_ALGO_DOUBLE)):
        h = LS._unbound(spec, algo, 64, 1000)
        try:
            reg = LS._regions(h)
            total = ctypes.c_uint64()
            assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
            off, n = reg[C.BUF_GRAD_CLIP]
            n_params, _ = spec.param_infos()
            # the info block, the coefficient at byte 64, one fp64 partial per 4096-element chunk from byte
            # 128 (the chunk doubled until at most 512 partials)
            chunk = 4096
            while -(-n_params // chunk) > 512:
                chunk *= 2
            assert n == 128 + 8 * -(-n_params // chunk)
            assert ctypes.sizeof(C.GradClipInfo) <= 64
            assert off % 256 == 0 and off + n <= total.value
            for b, (o, m) in reg.items():   # behind every other region: their offsets are the parent's
                if b != C.BUF_GRAD_CLIP and m:
                    assert o + m <= off, b
        finally:
            L.dqnx_engine_destroy(h)


def _bound(spec, algo, batch=32, cap=200):
    L = C.lib()
    h = LS._unbound(spec, algo, batch, cap)
    total = ctypes.c_uint64()
    assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
    assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
    return h


def _names(h, flags):
    t = LS._kernel_names(h, flags)
    return t if isinstance(t, int) else [n for n, _, _ in t]


# every flag combination the existing tests hand to dqnx_learn_kernel_count / _info
QUERIED = (0, C.STEP_SOFT_UPDATE, C.STEP_PREFETCH, C.STEP_GRADS_ONLY, C.STEP_STATS, C.STEP_SOFT_UPDATE | C.STEP_STATS,
           C.STEP_PREFETCH | C.STEP_STATS, C.STEP_SOFT_UPDATE | C.STEP_PREFETCH, C.STEP_GIVEN_INDICES,
           C.STEP_GRADS_ONLY | C.STEP_PREFETCH)


@pytest.mark.parametrize("net,algo,env", [
    ("mlp14", C.DQNX_ALGO_DOUBLE, {}), ("mlp14", C.DQNX_ALGO_DQN, {}), ("mlp284", C.DQNX_ALGO_PER_DOUBLE, {}),
    ("mlp14", C.DQNX_ALGO_DOUBLE, {"DQNX_DW_ADAM16": "0"}), ("mlp14", C.DQNX_ALGO_DOUBLE, {"DQNX_BWD_PLAN": "0"}),
    ("head", C.DQNX_ALGO_DOUBLE, {}), ("head", C.DQNX_ALGO_PER_DOUBLE, {}), ("hybrid84", C.DQNX_ALGO_DOUBLE, {})])
def test_grad_clip_planned_kernel_tables(monkeypatch, net, algo, env):
    """Clipping off: every table is what it was before clipping was ever set.  Clipping on: a step is the
    gradient-only step's launches, grad_sumsq, clip_coef, (PER: per_update,) adam_clipped, then the
    statistics launch if asked for; a DQNX_STEP_GRADS_ONLY step is unchanged."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    L = C.lib()
    spec = {"mlp14": E.mlp_spec(14, 8, "dueling" if algo != C.DQNX_ALGO_DQN else "linear"),
            "mlp284": E.mlp_spec(284, 8, "dueling"), "head": E.hybrid_spec(8, "dueling"),
            "hybrid84": E.hybrid_spec(8, "dueling", micro_chw=(4, 84, 84))}[net]
    per = algo == C.DQNX_ALGO_PER_DOUBLE
    queried = [f for f in QUERIED if not (per and f & C.STEP_GIVEN_INDICES)]
    h = _bound(spec, algo)
    try:
        off0 = {f: LS._kernel_names(h, f) for f in queried}
        assert L.dqnx_set_grad_clip(h, ctypes.c_double(10.0)) == 0
        tail = PER_TAIL if per else TAIL
        for f in queried:
            on = _names(h, f)
            if f & C.STEP_GRADS_ONLY:
                assert LS._kernel_names(h, f) == off0[f]
                continue
            stats = ["learn_stats"] if f & C.STEP_STATS else []
            # the gradient-only step with the same way of drawing the minibatch (the micro-CNN plan draws
            # nothing ahead in a statistics step)
            pf = f & C.STEP_PREFETCH if not (net == "head" and f & C.STEP_STATS) else 0
            grads = _names(h, C.STEP_GRADS_ONLY | pf | (f & C.STEP_GIVEN_INDICES))
            assert on == grads + tail + stats, (f, on)
        # the tail's entries say what they move: the gradient once for the sum, seven vectors for Adam
        n_params, _ = spec.param_infos()
        t = {n: (fl, by) for n, fl, by in LS._kernel_names(h, 0)}
        assert t["grad_sumsq"][1] >= 4 * n_params and t["adam_clipped"][1] == 4 * 7 * n_params
        assert L.dqnx_set_grad_clip(h, ctypes.c_double(0.0)) == 0
        for f in queried:
            assert LS._kernel_names(h, f) == off0[f], f
    finally:
        L.dqnx_engine_destroy(h)


def test_grad_clip_refuses_the_bucketed_entry_points():
    L = C.lib()
    for spec in (E.mlp_spec(14, 8, "dueling"), E.hybrid_spec(8, "dueling")):
        h = _bound(spec, C.DQNX_ALGO_DOUBLE)
        try:
            assert L.dqnx_set_grad_clip(h, ctypes.c_double(5.0)) == 0
            assert L.dqnx_learn_step_bucket(h, 0, 0, None) == C.DQNX_EUNSUPPORTED
            assert b"gradient clipping" in L.dqnx_last_error() and b"dqnx_learn_step_bucket" in L.dqnx_last_error()
            assert L.dqnx_apply_grads_bucket(h, 0, 0, None) == C.DQNX_EUNSUPPORTED
            assert b"gradient clipping" in L.dqnx_last_error() and b"dqnx_apply_grads_bucket" in L.dqnx_last_error()
            n = C.I32()
            assert L.dqnx_dp_bucket_count(h, ctypes.byref(n)) == 0 and n.value >= 1   # planning still answers
        finally:
            L.dqnx_engine_destroy(h)
