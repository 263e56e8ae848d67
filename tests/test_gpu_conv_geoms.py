"""GPU parity of the two-stream learn step across conv geometries and conv routes (tests/conv_geoms.py;
DESIGN.md §4 "conv geometry sweep"): every row against the fp32 oracle on each route that can run it --
the micro-CNN plan (csrc/micro.hip), the implicit-GEMM plan (csrc/conv_ig.hip), the explicit plan
(csrc/conv.hip) -- at batches that put one, two and three samples into a forward workgroup, and the
launch variants bitwise against each other.

Tolerances are the project's own: Q, loss and weights at the 1e-5 of BASELINE.json (weights atol=1e-5,
rtol=0, no entry exempted: these are ELU nets, no ReLU mask can flip, and the fp32 oracle stays within
3.5e-6 of an fp64 forward / backward on every row), gradients by parity.assert_grad_close, Adam's m / v
within 1e-6 / 1e-7.  tests/test_conv_routes.py (CPU) pins the route of every (row, algorithm, batch)
used here."""
import numpy as np
import pytest
import torch

import conv_geoms as G
from parity import assert_grad_close
from test_gpu_hybrid import make_hybrid_pair

pytestmark = pytest.mark.gpu

DDQN, DQN, PER = "DuelingDoubleDQNAgent", "DQNAgent", "PerDuelingDoubleDQNAgent"


def _grad_margin(got, ref):
    """Largest |got - ref| of a gradient tensor, absolute and as a fraction of assert_grad_close's bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = np.abs(got - ref)
    tol = 2e-6 + 1e-4 * np.abs(ref) + 5e-4 * float(np.abs(ref).max())
    return float(d.max()), float((d / tol).max())


def check_against_oracle(name, algo, batch, seed, steps=3, route=None):
    """`steps` train steps of the engine against the oracle's train_step on one table row: sampled
    indices bit-exact, q[0] / q[2], the loss, every gradient tensor, online and target weights each step;
    Adam's moments and the RNG state after the last."""
    g = G.BY_NAME[name] if name != "head" else None   # "head": the reference's net on its (2,27,5) grid
    cap, fill = G.replay_sizes(g) if g else (1000, 800)
    oracle, eng = make_hybrid_pair(algo, batch, cap, fill, seed, geom=g)
    per = algo.startswith("Per")
    worst = {"q": 0.0, "grad": 0.0, "grad/tol": 0.0, "w": 0.0}
    for step in range(steps):
        rec = oracle.train_step()
        eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        eng.check_device_error()
        idx = eng.batch_idx.cpu().numpy().astype(np.int64) + (cap - 1 if per else 0)
        assert np.array_equal(idx, rec.positions), f"step {step}: sampled indices differ"
        q = eng.q.cpu()
        worst["q"] = max(worst["q"], float((q[0] - rec.q_online).abs().max()), float((q[2] - rec.q_target_next).abs().max()))
        np.testing.assert_allclose(q[0].numpy(), rec.q_online.numpy(), atol=1e-5, rtol=1e-5, err_msg=f"step {step} q")
        np.testing.assert_allclose(q[2].numpy(), rec.q_target_next.numpy(), atol=1e-5, rtol=1e-5, err_msg=f"step {step} q'")
        assert abs(eng.loss() - rec.loss) <= 1e-5 * max(1.0, abs(rec.loss)), (step, eng.loss(), rec.loss)
        gv = eng.param_views(eng.grads[:-1])
        for k, ref in rec.grads.items():
            got = gv[k].cpu()
            d, r = _grad_margin(got, ref)
            worst["grad"], worst["grad/tol"] = max(worst["grad"], d), max(worst["grad/tol"], r)
            assert_grad_close(got, ref, f"step {step} {k}")
        on = eng.param_views(eng.params)
        tg = eng.param_views(eng.target_params)
        for k in oracle.online:
            a, b = on[k].cpu(), tg[k].cpu()
            worst["w"] = max(worst["w"], float((a - oracle.online[k]).abs().max()), float((b - oracle.target[k]).abs().max()))
            np.testing.assert_allclose(a.numpy(), oracle.online[k].numpy(), atol=1e-5, rtol=0, err_msg=f"step {step} {k}")
            np.testing.assert_allclose(b.numpy(), oracle.target[k].numpy(), atol=1e-5, rtol=0, err_msg=f"step {step} target {k}")
    m, v = eng.param_views(eng.adam_m), eng.param_views(eng.adam_v)
    for k in oracle.online:
        np.testing.assert_allclose(m[k].cpu().numpy(), oracle.m[k].numpy(), atol=1e-6, rtol=0, err_msg=f"m {k}")
        np.testing.assert_allclose(v[k].cpu().numpy(), oracle.v[k].numpy(), atol=1e-7, rtol=0, err_msg=f"v {k}")
    assert np.array_equal(eng.get_rng(1 if per else 0), oracle.np_state if per else oracle.py_state)
    print(f"conv_geom {name} [{route or (g.route if g else 'micro')}] {algo} B={batch}: worst |dw| {worst['w']:.2e}  |dq| {worst['q']:.2e}  "
          f"|dgrad| {worst['grad']:.2e} ({worst['grad/tol']:.3f} of its bound)")
    return worst


LEARN_CASES = ([(g.name, DDQN, G.base_batch(g)) for g in G.GEOMS] +
               [(n, DQN, 37) for n in G.MICRO + ("k5", "even_k2", "s3")] +
               [(n, PER, G.base_batch(G.BY_NAME[n])) for n in ("tiny3x3", "two_c1s2", "ig37x29")] +
               [(G.BIG_DW_ROW, DDQN, G.BIG_DW_BATCH)])


@pytest.mark.parametrize("name,algo,batch", LEARN_CASES)
def test_gpu_conv_geom_learn_matches_oracle(name, algo, batch):
    """Every table row on its default route, 3 steps: DuelingDouble at B = 37 (a multiple of nothing;
    the 1024-pixel rows at B = 21), the micro rows and three explicit rows also with DQNAgent's two
    streams and linear head, two micro rows and one implicit row also under PER; ig_c2 also at the
    batch from which its conv 2 takes the explicit route's big weight-gradient tiles."""
    check_against_oracle(name, algo, batch, seed=100 + LEARN_CASES.index((name, algo, batch)))


S_CASES = ([(n, DDQN, b) for n in G.S_ROWS for b in (101, 173)] +
           [(G.S_DQN_ROW, DQN, b) for b, s in sorted(G.S_BATCHES[2].items()) if s > 1])


@pytest.mark.parametrize("name,algo,batch", S_CASES)
def test_gpu_conv_geom_multi_sample_workgroups(name, algo, batch):
    """k_micro_fwd with more than one sample per workgroup (LDS image offsets per sample, pixel tiles
    that straddle two samples, the ragged last workgroup).  micro_plan picks S from the batch, the
    number of forward streams and the device's compute units; with the 256 of an MI355X, three streams:
    B = 101 is S = 2 with a one-sample last workgroup, B = 173 is S = 3 with two samples in the last;
    DQNAgent's two streams: B = 173 is S = 2, B = 259 is S = 3, each with one sample in the last.
    This test cannot observe S: tests/sanitize/plan_check.cpp (run by tests/test_sanitize.py on the
    CPU) calls micro_plan with 256 compute units and pins S for exactly these rows and batches; that
    check is what ties the batch sizes here to the code path."""
    assert G.S_BATCHES[2 if algo == DQN else 3][batch] > 1
    check_against_oracle(name, algo, batch, seed=200 + S_CASES.index((name, algo, batch)))


@pytest.mark.parametrize("name,knob", [(n, "DQNX_MICRO_CNN") for n in G.MICRO] +
                         [(n, "DQNX_CONV_IG") for n in ("ig37x29", "ig_2conv")])
def test_gpu_conv_geom_routes_agree(monkeypatch, name, knob):
    """The explicit kernels on geometries a second implementation also runs: every micro row with
    DQNX_MICRO_CNN=0, two implicit rows with DQNX_CONV_IG=0, through the same oracle comparison."""
    monkeypatch.setenv(knob, "0")
    g = G.BY_NAME[name]
    check_against_oracle(name, DDQN, G.base_batch(g), seed=300, route=f"{g.route} row on the explicit route")


def test_gpu_conv_geom_dense1_single_slab_at_large_batch():
    """Dense 1 of a conv net runs as split-K slabs plus an ordered reduce; with one slab the kernel's
    epilogue writes the activations itself and no reduce may follow (it once did, and overwrote them
    with act(bias): every sample got the same Q).  One slab is planned where F < 256 (tiny3x3, k5 and
    s3 above) and where the 64 x 64 tiles alone exceed one per compute unit: the reference's net
    (512 columns, three streams) from B = 641; tests/test_conv_routes.py pins that plan."""
    check_against_oracle("head", DDQN, 720, seed=400, steps=2)


def _state(eng):
    torch.cuda.synchronize()
    eng.check_device_error()
    return {"q": eng.q.cpu().clone(), "grads": eng.grads.cpu().clone(), "params": eng.params.cpu().clone(),
            "target": eng.target_params.cpu().clone(), "batch_idx": eng.batch_idx.cpu().clone(),
            "rng": torch.from_numpy(eng.get_rng(0).astype(np.int64))}


def _assert_identical(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differ"


def _engine(name, batch, seed, graphs=False):
    g = G.BY_NAME[name]
    cap, fill = G.replay_sizes(g)
    return make_hybrid_pair(DDQN, batch, cap, fill, seed, graphs=graphs, geom=g)[1]


VARIANTS = ([(n, 37, v) for n in ("two_c1s2", "ci7", "even8x4") for v in ("mdx_waves", "pixpad")] +
            [(n, b, v) for n, b in (("tiny3x3", 101), ("two_c1s2", 37)) for v in ("graphs", "prefetch")])


@pytest.mark.parametrize("name,batch,variant", VARIANTS)
def test_gpu_conv_geom_variants_bit_identical(monkeypatch, name, batch, variant):
    """Bitwise equal q, gradients, weights, targets, sampled indices and RNG state between
      mdx_waves  8 vs 4 data-gradient waves per workgroup (DQNX_MDX_WAVES), 4 steps,
      pixpad     LDS pixel stride Co + 4 vs Co + 8 (DQNX_MICRO_PIXPAD), 4 steps
                 (both change which wave computes an output or where it lies, never the order of a sum),
      graphs     graph replay vs eager launches over 5 steps with a hard update in the middle (eager
                 steps skip conv_perm while the Adam-written conv weight copies are current; the hard
                 update stales them),
      prefetch   DQNX_STEP_PREFETCH (k_micro_fwd's block 0 draws the next minibatch) vs sequential
                 steps; at B = 101 the sampler block runs beside S = 2 compute workgroups."""
    if variant in ("mdx_waves", "pixpad"):
        knob, vals = {"mdx_waves": ("DQNX_MDX_WAVES", ("8", "4")), "pixpad": ("DQNX_MICRO_PIXPAD", ("4", "8"))}[variant]
        out = []
        for val in vals:
            monkeypatch.setenv(knob, val)
            eng = _engine(name, batch, 41)
            for _ in range(4):
                eng.learn_step(soft_update=True)
            out.append(_state(eng))
            del eng
        _assert_identical(out[0], out[1], f"{name} {knob}={vals[0]} vs {vals[1]}")
        return
    e1, e2 = _engine(name, batch, 51), _engine(name, batch, 51, graphs=variant == "graphs")
    for i in range(5):
        e1.learn_step(soft_update=True)
        e2.learn_step(soft_update=True, prefetch=variant == "prefetch" and i < 4)
        if variant == "graphs" and i == 2:
            e1.hard_update()
            e2.hard_update()
    _assert_identical(_state(e1), _state(e2), f"{name} B={batch} {variant}")
