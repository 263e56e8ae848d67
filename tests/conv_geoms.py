"""The conv geometries of the learn-step sweep (tests/test_conv_routes.py on the CPU,
tests/test_gpu_conv_geoms.py on the GPU, tests/sanitize/plan_check.cpp under the sanitizers; DESIGN.md
§4 "conv geometry sweep").  One row = one TwoStreamHybridNetwork: the micro grid, the number of macro
features, the conv stack, the dense widths and the conv route engine creation is expected to plan:

  micro     csrc/micro.hip    (micro_fwd / micro_dx / micro_dw in the planned kernel list)
  explicit  csrc/conv.hip     (im2col_c1 ...)
  implicit  csrc/conv_ig.hip  (neither of the two)

plan_check.cpp carries the same rows (C++ cannot import this table); test_sanitize.py checks the two
lists against each other."""
from collections import namedtuple

Geom = namedtuple("Geom", "name micro_chw macro_len conv dense route")

K33 = (3, 3)
REF = ((32, K33, (1, 1)), (64, K33, (2, 1)), (64, K33, (2, 2)))   # the reference's stack (R:env/dqn_config.py:163-167)

GEOMS = (
    # -- micro route: 3x3 windows, strides 1-2, Co % 16 == 0, Ci * 9 <= 64, conv-1 output <= 144 pixels
    Geom("odd9x4", (2, 9, 4), 6, REF, (512, 256), "micro"),        # F = 64*3*1 + 6 = 198 (% 4 = 2), odd height
    Geom("even8x4", (2, 8, 4), 16, REF, (512, 256), "micro"),      # even heights under stride 2: unequal phases
    Geom("tiny3x3", (2, 3, 3), 2, REF, (512, 256), "micro"),       # last conv of 1x2 pixels: every tap pads somewhere
    Geom("two_c1s2", (1, 12, 12), 1, ((16, K33, (2, 2)), (32, K33, (1, 2))), (128, 64), "micro"),   # Ci = 1, strided conv 1, stride (1,2)
    Geom("ci7", (7, 5, 4), 3, ((32, K33, (1, 1)), (16, K33, (2, 2)), (64, K33, (1, 1))), (128, 64), "micro"),   # K = 63, narrow middle conv
    Geom("alls1", (3, 6, 7), 5, ((64, K33, (1, 1)), (64, K33, (1, 1)), (32, K33, (1, 1))), (128, 64), "micro"),
    Geom("big144", (2, 12, 12), 2, REF, (128, 64), "micro"),       # conv-1 output of exactly 144 pixels
    # -- explicit route: everything else
    Geom("big13x12", (2, 13, 12), 2, REF, (128, 64), "explicit"),  # one row past the micro limit
    Geom("w1", (2, 16, 1), 4, REF, (128, 64), "explicit"),
    Geom("co48", (2, 6, 6), 2, ((48, K33, (1, 1)), (64, K33, (2, 2))), (128, 64), "explicit"),
    Geom("k5", (2, 9, 4), 6, ((8, (5, 3), (1, 1)), (16, (1, 3), (2, 1)), (16, (3, 1), (2, 2))), (128, 64), "explicit"),
    Geom("even_k2", (2, 9, 4), 6, ((8, (2, 2), (1, 1)), (16, (4, 2), (2, 1))), (128, 64), "explicit"),   # padding k//2: output larger than input
    Geom("s3", (2, 10, 7), 3, ((12, K33, (3, 3)), (20, K33, (1, 1))), (72, 64), "explicit"),
    Geom("oneconv", (2, 9, 4), 6, ((32, K33, (2, 2)),), (128, 64), "explicit"),
    # -- implicit-GEMM route: micro grids of >= 1024 pixels, Ci = 4 first, Co in {32, 64}
    Geom("ig37x29", (4, 37, 29), 3, REF, (128, 64), "implicit"),
    Geom("ig33x32", (4, 33, 32), 14, REF, (128, 64), "implicit"),
    Geom("ig_2conv", (4, 40, 30), 2, ((32, K33, (2, 2)), (64, K33, (2, 2))), (128, 64), "implicit"),
    Geom("ig_c2", (2, 40, 30), 2, REF, (128, 64), "explicit"),     # Ci = 2: the explicit route's big kernels
)
BY_NAME = {g.name: g for g in GEOMS}
MICRO = tuple(g.name for g in GEOMS if g.route == "micro")
IMPLICIT = tuple(g.name for g in GEOMS if g.route == "implicit")

N_ACTIONS = 8
ALGOS = ("DQNAgent", "DuelingDoubleDQNAgent", "PerDuelingDoubleDQNAgent")


def is_big(g):
    """The 1024-pixel rows: smaller replay (capacity 200, 150 pushed) and B = 21 in place of 37."""
    return g.micro_chw[1] * g.micro_chw[2] >= 1024


def base_batch(g):
    return 21 if is_big(g) else 37


def replay_sizes(g):
    return (200, 150) if is_big(g) else (500, 400)


# Batches at which the forward packs more than one sample into a workgroup (micro_plan's S with the
# 256 compute units of an MI355X; plan_check.cpp pins every value): three streams 37 -> 1, 101 -> 2,
# 173 -> 3; DQNAgent's two streams 37 -> 1, 173 -> 2, 259 -> 3.  {streams: {batch: S}}
S_ROWS = ("odd9x4", "tiny3x3", "two_c1s2", "ci7")
S_BATCHES = {3: {37: 1, 101: 2, 173: 3}, 2: {37: 1, 173: 2, 259: 3}}
S_DQN_ROW = "two_c1s2"

# The explicit route's big variants on ig_c2 (engine.cpp): at B = 21 conv 2's data gradient runs on the
# 128x64 tiles of k_conv_dx_big (planned as conv_dx_c2); the 64x128 weight-gradient tiles of
# k_conv_dw_big need 65,536 output pixels per step and K >= 127: conv 2 (20x30 pixels, K = 288) from B = 110.
BIG_DW_ROW, BIG_DW_BATCH = "ig_c2", 110


def gpu_batches(g):
    """Every batch the GPU tests create an engine of this row at."""
    bs = {base_batch(g)}
    if g.name == BIG_DW_ROW:
        bs.add(BIG_DW_BATCH)
    if g.name in S_ROWS:
        bs |= set(S_BATCHES[3]) | (set(S_BATCHES[2]) if g.name == S_DQN_ROW else set())
    return sorted(bs)


def engine_spec(E, g, head):
    return E.hybrid_spec(N_ACTIONS, head, micro_chw=g.micro_chw, macro_len=g.macro_len, conv=g.conv, dense=g.dense)


def oracle_spec(O, g, head):
    return O.hybrid_spec(N_ACTIONS, head, micro_chw=g.micro_chw, macro_len=g.macro_len, conv=g.conv, dense=g.dense)


def route_of(names):
    """The conv route of a planned kernel list (dqnx_learn_kernel_info names)."""
    if any(n.startswith("micro_fwd") for n in names):
        return "micro"
    if any(n.startswith("im2col_c1") for n in names):
        return "explicit"
    return "implicit"
