"""CPU: the conv route engine creation plans for every row of tests/conv_geoms.py, at every batch and
algorithm tests/test_gpu_conv_geoms.py runs it with.  Planning needs no GPU: the engine is bound to an
address that is never dereferenced and its planned kernel list (dqnx_learn_kernel_count / _info) is
read: micro_fwd present = the micro-CNN plan (csrc/micro.hip), im2col_c1 present = the explicit plan
(csrc/conv.hip), neither = the implicit-GEMM plan (csrc/conv_ig.hip).  An edit to a planner that moves
a row to another route fails here, so the GPU sweep cannot silently exercise a different kernel."""
import ctypes

import pytest

import conv_geoms as G
import test_learn_stats_capi as LS
from dqn import _capi as C
from dqn import engine as E

ALGO = {"DQNAgent": C.DQNX_ALGO_DQN, "DuelingDoubleDQNAgent": C.DQNX_ALGO_DOUBLE,
        "PerDuelingDoubleDQNAgent": C.DQNX_ALGO_PER_DOUBLE}


def planned_names(g, algo, batch):
    L = C.lib()
    head = "linear" if algo == "DQNAgent" else "dueling"
    h = LS._unbound(G.engine_spec(E, g, head), ALGO[algo], batch, G.replay_sizes(g)[0])
    try:
        total = ctypes.c_uint64()
        assert L.dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
        assert L.dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
        out = {}
        for flags in (C.STEP_SOFT_UPDATE, C.STEP_SOFT_UPDATE | C.STEP_PREFETCH):
            t = LS._kernel_names(h, flags)
            assert not isinstance(t, int), (g.name, algo, batch, flags, t)
            out[flags] = [n for n, _, _ in t]
        return out
    finally:
        L.dqnx_engine_destroy(h)


def routes(g):
    """The route of every (algorithm, batch) the GPU tests create an engine at."""
    got = set()
    for algo in G.ALGOS:
        for batch in G.gpu_batches(g):
            for names in planned_names(g, algo, batch).values():
                got.add(G.route_of(names))
    return got


def test_table_is_what_the_sweep_was_planned_with():
    assert len(G.GEOMS) == 18 and len({g.name for g in G.GEOMS}) == 18
    assert G.MICRO == ("odd9x4", "even8x4", "tiny3x3", "two_c1s2", "ci7", "alls1", "big144")
    assert G.IMPLICIT == ("ig37x29", "ig33x32", "ig_2conv")
    for g in G.GEOMS:
        assert G.base_batch(g) == (21 if g.name.startswith("ig") else 37)
        cap, fill = G.replay_sizes(g)
        assert max(G.gpu_batches(g)) <= fill <= cap
    # the dense input widths cover every F % 4 (the HEAD net's 1358 is 2)
    from oracle import ref as O
    widths = {}
    for g in G.GEOMS:
        f, h, w = O.conv_out_hw(G.oracle_spec(O, g, "dueling"))[-1]
        widths[g.name] = f * h * w + g.macro_len
    assert {widths[n] % 4 for n in G.MICRO} == {0, 1, 2, 3}, widths


@pytest.mark.parametrize("name", [g.name for g in G.GEOMS])
def test_conv_route_of_every_row(name):
    g = G.BY_NAME[name]
    assert routes(g) == {g.route}


@pytest.mark.parametrize("name", G.MICRO)
def test_micro_rows_fall_to_the_explicit_route_without_the_micro_plan(monkeypatch, name):
    monkeypatch.setenv("DQNX_MICRO_CNN", "0")
    assert routes(G.BY_NAME[name]) == {"explicit"}


@pytest.mark.parametrize("name", G.IMPLICIT)
def test_implicit_rows_fall_to_the_explicit_route_without_the_implicit_plan(monkeypatch, name):
    monkeypatch.setenv("DQNX_CONV_IG", "0")
    assert routes(G.BY_NAME[name]) == {"explicit"}


def test_dense1_reduce_is_planned_only_behind_more_than_one_slab():
    """Dense 1 of a conv net: split-K slabs, then an ordered reduce.  With a single slab (F < 256, or
    more 64 x 64 tiles than compute units) the slab kernel's epilogue writes the activations
    and the reduce, which would overwrite them from slabs nobody filled, must not be planned."""
    def dense1(names):
        return [n for n in names if n.startswith("linear_fwd_l1")]
    for name, batch, reduce in (("tiny3x3", 37, False), ("k5", 37, False), ("s3", 37, False),   # F = 130, 102, 243
                                ("even8x4", 37, True), ("odd9x4", 37, True), ("ig37x29", 21, True)):
        names = planned_names(G.BY_NAME[name], "DuelingDoubleDQNAgent", batch)[C.STEP_SOFT_UPDATE]
        assert dense1(names) == ["linear_fwd_l1"] + (["linear_fwd_l1_reduce"] if reduce else []), (name, dense1(names))
    # the reference's net: 8 column tiles x ceil(B / 64) row tiles x 3 streams > 256 from B = 641
    for batch, reduce in ((256, True), (640, True), (641, False), (720, False)):
        h = LS._unbound(E.hybrid_spec(8, "dueling"), C.DQNX_ALGO_DOUBLE, batch, 1000)
        try:
            total = ctypes.c_uint64()
            assert C.lib().dqnx_engine_arena_bytes(h, ctypes.byref(total)) == 0
            assert C.lib().dqnx_engine_bind(h, ctypes.c_void_p(0x7f0000000000), total.value) == 0
            names = [n for n, _, _ in LS._kernel_names(h, C.STEP_SOFT_UPDATE)]
        finally:
            C.lib().dqnx_engine_destroy(h)
        assert ("linear_fwd_l1_reduce" in names) == reduce, (batch, dense1(names))


def test_big_explicit_row_plans_the_big_conv_kernels():
    """ig_c2 (Ci = 2 keeps it off the implicit route) is in the table for the explicit route's big
    variants: conv 2's data gradient in a launch of its own (conv_dx_c2: k_conv_dx_big's 128x64 tiles),
    which the small explicit rows keep inside conv_bwd_c2.  The big weight-gradient tiles have no entry
    of their own in the kernel list; their threshold (65,536 output pixels per step, K >= 127) is met by
    conv 2 at BIG_DW_BATCH."""
    g = G.BY_NAME[G.BIG_DW_ROW]
    for batch in (21, G.BIG_DW_BATCH):
        assert "conv_dx_c2" in planned_names(g, "DuelingDoubleDQNAgent", batch)[C.STEP_SOFT_UPDATE]
    assert "conv_dx_c2" not in planned_names(G.BY_NAME["big13x12"], "DuelingDoubleDQNAgent", 37)[C.STEP_SOFT_UPDATE]
    from oracle import ref as O
    (_, h1, w1), (_, h2, w2), _ = O.conv_out_hw(G.oracle_spec(O, g, "dueling"))
    assert G.BIG_DW_BATCH * h2 * w2 >= 65536 > (G.BIG_DW_BATCH - 1) * h2 * w2 and 9 * g.conv[0][0] >= 127
    assert G.BIG_DW_BATCH <= G.replay_sizes(g)[1]
