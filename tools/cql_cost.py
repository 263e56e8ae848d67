"""Cost of the CQL(H) regulariser (LearnEngine(cql_alpha=)): in one process, on engines of the same net and
batch,
  a0  alpha = 0 (the default: the head kernel's CQL = false instantiation),
  a1  alpha = 1 (CQL = true: three more 16-lane reductions, one expf and one logf per action slot),
whole learn-step times from interleaved windows (medians of --reps), and the own time of the head launch
("head_bwd" on the fused MLP plan, "head_td_loss" elsewhere) from dqnx_learn_step_timed.  The launch tables
of the two engines must be equal: the regulariser adds no launch.  One JSON line.

  python tools/cql_cost.py --config mlp284|head [--steps N] [--reps R] [--alpha A]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, "..")
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-drl-rmc_amd")]

CONFIGS = {   # name: (spec builder, batch, steps per timed window)
    "mlp284": (lambda E: E.mlp_spec(284, 8, "dueling"), 1024, 4000),
    "head": (lambda E: E.hybrid_spec(8, "dueling"), 256, 1500),
}
HEAD_LAUNCHES = ("head_bwd", "head_td_loss")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="mlp284")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=1.0)
    args = ap.parse_args()
    import torch

    from dqn import _capi as C
    from dqn import engine as E
    from oracle import ref as O

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to measure without one"
    build, batch, steps = CONFIGS[args.config]
    steps = args.steps or steps
    spec = build(E)
    cap, fill = 20000, 10000
    data = O.synth_transitions(fill, spec.obs_dim, 8, seed=5)

    def engine(alpha):
        eng = E.LearnEngine(spec, "DuelingDoubleDQNAgent", batch, cap, cql_alpha=alpha)
        eng.push(*data)
        random.seed(11)
        eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
        for _ in range(200):   # plans built and every shape warm
            eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        return eng

    engines = {"a0": engine(None), "a1": engine(args.alpha)}

    def window(eng):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            eng.learn_step(soft_update=True)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps   # us per step

    times = {k: [] for k in engines}
    for _ in range(args.reps):   # a0, a1, a0, ...
        for k, eng in engines.items():
            times[k].append(window(eng))

    def summary(v):
        return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "windows": len(v)}

    out = {"config": args.config, "batch": batch, "alpha": args.alpha, "steps_per_window": steps,
           "abi": int(C.lib().dqnx_abi_version())}
    ev = (ctypes.c_void_p * 2)()
    C.check(C.lib().dqnx_events_create(2, ev), "events_create")
    flags = C.STEP_SOFT_UPDATE
    tables = {}
    for k, eng in engines.items():
        out["step_" + k] = summary(times[k])
        n = C.I32()
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
        table = []
        for i in range(n.value):
            name, fl, by = ctypes.create_string_buffer(64), ctypes.c_double(), ctypes.c_double()
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, ctypes.byref(fl), ctypes.byref(by)), "kernel_info")
            table.append((name.value.decode(), fl.value, by.value))
        tables[k] = table
        names = [t[0] for t in table]
        idx = [i for i, nm in enumerate(names) if nm in HEAD_LAUNCHES]
        assert len(idx) == 1, names
        ks = []
        for i in range(60):
            C.check(eng.L.dqnx_learn_step_timed(eng.h, flags, idx[0], ev[0], ev[1], eng.stream()), "learn_step_timed")
            ms = ctypes.c_float()
            C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
            if i >= 10:
                ks.append(ms.value * 1000.0)
        out["kernel_%s_%s" % (names[idx[0]], k)] = summary(ks)
        out["cql_gap_" + k] = eng.cql_gap()
        out["loss_" + k] = eng.loss()
        eng.check_device_error()
    C.lib().dqnx_events_destroy(2, ev)
    assert tables["a0"] == tables["a1"], "the regulariser changed the launch table"
    out["launches"] = [t[0] for t in tables["a0"]]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
