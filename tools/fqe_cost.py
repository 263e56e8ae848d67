"""Cost of fitted Q evaluation (include/dqnx.h "fitted Q evaluation"): in one process, at one batch,
  step    the learn step of a DuelingDoubleDQNAgent engine with a target-policy table set (the FQE step: the DQN
          stream set), the SAME engine's own Double step (table cleared), and a DQNAgent engine's step on the same
          network and ring, from alternating windows of --steps steps, medians of --reps windows,
  sweep   policy_actions() and fqe_value() over the whole ring against evaluate() on the same engine: time per
          chunk of `batch` rows, medians of --reps calls,
  launch  the own time of every launch of one chunk of the two sweeps from dqnx_fqe_chunk_timed (the timed-launch
          facility: the event pair bound to the launch's dispatch), medians of 50.
One JSON line.

  python tools/fqe_cost.py --config mlp284|head [--steps N] [--reps R] [--rows N]"""
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
    ap.add_argument("--rows", type=int, default=0, help="ring rows (default 200 chunks)")
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

    def engine(algo):
        eng = E.LearnEngine(spec, algo, batch, fill)
        for a in range(0, fill, 16384):
            eng.push(*(x[a:a + 16384] for x in data))
        random.seed(11)
        eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
        return eng

    ddqn, dqn = engine("DuelingDoubleDQNAgent"), engine("DQNAgent")
    table = ddqn.policy_actions()
    for eng in (ddqn, dqn):   # plans built and every shape warm, with and without the table
        for _ in range(200):
            eng.learn_step(soft_update=True)
    ddqn.set_target_policy(table)
    for _ in range(200):
        ddqn.learn_step(soft_update=True)
    ddqn.evaluate()
    ddqn.fqe_value(table)
    torch.cuda.synchronize()

    def summary(v):
        return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "samples": len(v)}

    def window(eng):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            eng.learn_step(soft_update=True)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    chunks = (fill + batch - 1) // batch
    t_fqe, t_double, t_dqn, s_pol, s_val, s_eval = [], [], [], [], [], []
    for _ in range(args.reps):   # FQE window, Double window, DQN window, the three sweeps, ...
        ddqn.set_target_policy(table)
        ddqn.learn_step(soft_update=True)   # (the plan rebuild is not in the window)
        t_fqe.append(window(ddqn))
        ddqn.set_target_policy(None)
        ddqn.learn_step(soft_update=True)
        t_double.append(window(ddqn))
        t_dqn.append(window(dqn))
        s_pol.append(timed(lambda: ddqn.policy_actions(out=table)) / chunks)
        s_val.append(timed(lambda: ddqn.fqe_value(table)) / chunks)
        s_eval.append(timed(lambda: ddqn.evaluate()) / chunks)
    res = ddqn.fqe_value(table)
    assert res["rows"] == fill
    out = {"config": args.config, "batch": batch, "rows": fill, "chunks": chunks, "abi": int(C.lib().dqnx_abi_version()),
           "fqe_step": summary(t_fqe), "double_step_same_engine": summary(t_double), "dqn_engine_step": summary(t_dqn),
           "learn_steps_per_window": steps,
           "policy_sweep_chunk": summary(s_pol), "fqe_value_chunk": summary(s_val), "evaluate_chunk": summary(s_eval)}
    # every launch of one chunk of both sweeps, by the dispatch's own begin / end timestamps
    ev = (ctypes.c_void_p * 2)()
    C.check(C.lib().dqnx_events_create(2, ev), "events_create")
    sc = ddqn.eval_scratch()
    for which, key in ((0, "policy_sweep_launches"), (1, "fqe_value_launches")):
        n = C.I32()
        C.check(ddqn.L.dqnx_fqe_kernel_count(ddqn.h, which, ctypes.byref(n)), "fqe_kernel_count")
        launches, total = [], 0.0
        for i in range(n.value):
            name = ctypes.create_string_buffer(64)
            C.check(ddqn.L.dqnx_fqe_kernel_name(ddqn.h, which, i, name, 64), "fqe_kernel_name")
            ks, skipped = [], False
            for r in range(60):
                rc = ddqn.L.dqnx_fqe_chunk_timed(ddqn.h, which, 0, ctypes.c_void_p(sc.data_ptr()), sc.numel(),
                                                 ctypes.c_void_p(table.data_ptr()), int(table.shape[0]), i, ev[0], ev[1],
                                                 ddqn.stream())
                if rc == C.DQNX_EUNSUPPORTED:   # a launch the plan skips while its outputs are current (conv_perm)
                    skipped = True
                    break
                C.check(rc, "fqe_chunk_timed")
                ms = ctypes.c_float()
                C.check(ddqn.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
                if r >= 10:
                    ks.append(ms.value * 1000.0)
            if skipped:
                launches.append({"name": name.value.decode(), "skipped": True})
                continue
            s = summary(ks)
            total += s["median_us"]
            launches.append({"name": name.value.decode(), **s})
        out[key] = launches
        out[key.replace("launches", "launch_sum_us")] = round(total, 3)
    # every launch of the three learn steps (dqnx_learn_step_timed: one whole step per sample)
    flags = C.STEP_SOFT_UPDATE

    def step_launches(eng):
        n = C.I32()
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
        rows = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(64)
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, None, None), "kernel_info")
            ks, skipped = [], False
            for r in range(40):
                rc = eng.L.dqnx_learn_step_timed(eng.h, flags, i, ev[0], ev[1], eng.stream())
                if rc == C.DQNX_EUNSUPPORTED:   # a launch the plan skips while its outputs are current (conv_perm)
                    skipped = True
                    break
                C.check(rc, "learn_step_timed")
                ms = ctypes.c_float()
                C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
                if r >= 10:
                    ks.append(ms.value * 1000.0)
            rows.append({"name": name.value.decode(), "skipped": True} if skipped else {"name": name.value.decode(), **summary(ks)})
        return rows

    ddqn.set_target_policy(table)
    out["fqe_step_launches"] = step_launches(ddqn)
    ddqn.set_target_policy(None)
    out["double_step_launches"] = step_launches(ddqn)
    out["dqn_engine_step_launches"] = step_launches(dqn)
    C.lib().dqnx_events_destroy(2, ev)
    out["value"] = res["value"]
    ddqn.check_device_error()
    dqn.check_device_error()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
