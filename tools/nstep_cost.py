"""Cost of n-step returns (LearnEngine(n_step=)): in one process, on engines of the same net and batch,
  n1       the default engine (n_step = 1: no gather launch),
  n3       n_step = 3, the gather's workgroups placed on the forward's XCDs (the default),
  n3_flat  n_step = 3 with DQNX_NSTEP_XCD=0 (workgroups in launch order; fused MLP plan only),
  n3_off4  n_step = 3 with DQNX_NSTEP_XCD=2 (every tile written four XCDs away from the forward that reads it),
whole learn-step times from interleaved windows, and the own times of "nstep_gather" and of the forward
launch that reads its rows (dqnx_learn_step_timed), with the gather's algorithmic bytes.  One JSON line.

  python tools/nstep_cost.py --config mlp284|head [--steps N] [--reps R] [--n-step K]"""
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

CONFIGS = {   # name: (spec builder, batch, steps per timed window, the forward launch's name)
    "mlp284": (lambda E: E.mlp_spec(284, 8, "dueling"), 1024, 4000, "mlp_fwd"),
    "head": (lambda E: E.hybrid_spec(8, "dueling"), 256, 1500, "micro_fwd"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="mlp284")
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n-step", type=int, default=3)
    args = ap.parse_args()
    import torch

    from dqn import _capi as C
    from dqn import engine as E
    from oracle import ref as O

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to measure without one"
    build, batch, steps, fwd_name = CONFIGS[args.config]
    steps = args.steps or steps
    spec = build(E)
    cap, fill = 20000, 10000
    data = O.synth_transitions(fill, spec.obs_dim, 8, seed=5)

    def engine(n_step, xcd):
        if xcd is not None:
            os.environ["DQNX_NSTEP_XCD"] = xcd
        eng = E.LearnEngine(spec, "DuelingDoubleDQNAgent", batch, cap, n_step=n_step)
        eng.push(*data)
        random.seed(11)
        eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
        for _ in range(200):   # plans built (the placement knob is read then) and every shape warm
            eng.learn_step(soft_update=True)
        torch.cuda.synchronize()
        os.environ.pop("DQNX_NSTEP_XCD", None)
        return eng

    engines = {"n1": engine(1, None), "n%d" % args.n_step: engine(args.n_step, None)}
    if args.config == "mlp284":
        engines["n%d_flat" % args.n_step] = engine(args.n_step, "0")
        engines["n%d_off4" % args.n_step] = engine(args.n_step, "2")

    def window(eng):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            eng.learn_step(soft_update=True)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps   # us per step

    times = {k: [] for k in engines}
    for _ in range(args.reps):   # n1, n3, n3_flat, n1, ...
        for k, eng in engines.items():
            times[k].append(window(eng))

    def summary(v):
        return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "windows": len(v)}

    out = {"config": args.config, "batch": batch, "n_step": args.n_step, "steps_per_window": steps,
           "abi": int(C.lib().dqnx_abi_version())}
    ev = (ctypes.c_void_p * 2)()
    C.check(C.lib().dqnx_events_create(2, ev), "events_create")
    flags = C.STEP_SOFT_UPDATE
    for k, eng in engines.items():
        out["step_" + k] = summary(times[k])
        n = C.I32()
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
        names, nbytes = [], []
        for i in range(n.value):
            name, by = ctypes.create_string_buffer(64), ctypes.c_double()
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, None, ctypes.byref(by)), "kernel_info")
            names.append(name.value.decode())
            nbytes.append(by.value)
        out["launches_" + k] = names
        for kname in ("nstep_gather", fwd_name):
            if kname not in names:
                continue
            idx = names.index(kname)
            ks = []
            for i in range(60):
                C.check(eng.L.dqnx_learn_step_timed(eng.h, flags, idx, ev[0], ev[1], eng.stream()), "learn_step_timed")
                ms = ctypes.c_float()
                C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
                if i >= 10:
                    ks.append(ms.value * 1000.0)
            out["kernel_%s_%s" % (kname, k)] = dict(summary(ks), algorithmic_bytes=nbytes[idx])
        eng.check_device_error()
    C.lib().dqnx_events_destroy(2, ev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
