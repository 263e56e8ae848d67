"""Cost of the offline evaluation sweep (LearnEngine.evaluate, include/dqnx.h "offline evaluation"): in one
process, on one engine,
  sweep   evaluate() over the whole ring (one host read per call): time per chunk of `batch` rows and rows/s,
          medians of --reps calls,
  step    the engine's own learn step at the same batch from windows of --steps steps (the yardstick: a chunk
          runs the step's forward and omits the dZ chain, the weight gradients and Adam),
  launch  the own time of every launch of one chunk from dqnx_eval_chunk_timed (the timed-launch facility: the
          event pair bound to the launch's dispatch), medians of 50.
One JSON line.

  python tools/eval_cost.py --config mlp284|head [--steps N] [--reps R] [--rows N]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, "..")
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-drl-rmc_amd")]

CONFIGS = {   # name: (spec builder, batch, learn steps per timed window)
    "mlp284": (lambda E: E.mlp_spec(284, 8, "dueling"), 1024, 4000),
    "head": (lambda E: E.hybrid_spec(8, "dueling"), 256, 1500),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="mlp284")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=0, help="ring rows swept (default 200 chunks)")
    args = ap.parse_args()
    import torch

    from dqn import _capi as C
    from dqn import engine as E
    from oracle import ref as O

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to measure without one"
    build, batch, steps = CONFIGS[args.config]
    steps = args.steps or steps
    spec = build(E)
    fill = args.rows or 200 * batch
    data = O.synth_transitions(fill, spec.obs_dim, 8, seed=5)
    eng = E.LearnEngine(spec, "DuelingDoubleDQNAgent", batch, fill)
    for a in range(0, fill, 16384):
        eng.push(*(x[a:a + 16384] for x in data))
    random.seed(11)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    for _ in range(200):   # plans built and every shape warm
        eng.learn_step(soft_update=True)
    eng.evaluate()
    torch.cuda.synchronize()

    def summary(v):
        return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "samples": len(v)}

    chunks = (fill + batch - 1) // batch
    sweeps, step_us = [], []
    for _ in range(args.reps):   # sweep, learn window, sweep, ...
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.evaluate()          # (ends with its one read of the result)
        sweeps.append((time.perf_counter() - t0) * 1e6)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            eng.learn_step(soft_update=True)
        e1.record()
        e1.synchronize()
        step_us.append(e0.elapsed_time(e1) * 1000.0 / steps)
    assert res["rows"] == fill
    per_chunk = [t / chunks for t in sweeps]
    out = {"config": args.config, "batch": batch, "rows": fill, "chunks": chunks, "abi": int(C.lib().dqnx_abi_version()),
           "sweep": summary(sweeps), "chunk": summary(per_chunk),
           "rows_per_s": round(fill / (statistics.median(sweeps) * 1e-6), 1),
           "learn_step": summary(step_us), "learn_steps_per_window": steps}
    # every launch of one chunk, by the dispatch's own begin / end timestamps
    n = C.I32()
    C.check(eng.L.dqnx_eval_kernel_count(eng.h, ctypes.byref(n)), "eval_kernel_count")
    ev = (ctypes.c_void_p * 2)()
    C.check(C.lib().dqnx_events_create(2, ev), "events_create")
    sc = eng.eval_scratch()
    launches, total = [], 0.0
    for i in range(n.value):
        name = ctypes.create_string_buffer(64)
        C.check(eng.L.dqnx_eval_kernel_name(eng.h, i, name, 64), "eval_kernel_name")
        ks, skipped = [], False
        for r in range(60):
            rc = eng.L.dqnx_eval_chunk_timed(eng.h, 0, ctypes.c_void_p(sc.data_ptr()), sc.numel(), i, ev[0], ev[1], eng.stream())
            if rc == C.DQNX_EUNSUPPORTED:   # a launch the plan skips while its outputs are current (conv_perm)
                skipped = True
                break
            C.check(rc, "eval_chunk_timed")
            ms = ctypes.c_float()
            C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
            if r >= 10:
                ks.append(ms.value * 1000.0)
        if skipped:
            launches.append({"name": name.value.decode(), "skipped": True})
            continue
        s = summary(ks)
        total += s["median_us"]
        launches.append({"name": name.value.decode(), **s})
    C.lib().dqnx_events_destroy(2, ev)
    out["launches"] = launches
    out["launch_sum_us"] = round(total, 3)
    out["loss"] = res["loss"]
    eng.check_device_error()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
