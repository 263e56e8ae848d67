"""Cost of on-device gradient clipping (dqnx_set_grad_clip): whole learn-step times, interleaved in one
process, of
  off    the step with clipping off (the launches of a build without clipping),
  split  the world-1 data-parallel form, learn_step(grads_only) + apply_grads, clipping off: a clipped
         step is this path plus the norm reduction, so it is the yardstick for what clipping adds,
  on     the step with clipping on,
and the clipping launches' own times (dqnx_learn_step_timed on grad_sumsq / clip_coef / adam_clipped).
One JSON line.

  python tools/grad_clip_cost.py --config mlp284|head [--pkg DIR] [--steps N] [--reps R] [--max-norm X]

--pkg: the directory that holds the `dqn` package to measure (default: this tree's).  A package from
before clipping existed is measured in the off and split forms only, so the same script times a parent
build beside this one in alternating processes (DESIGN.md "Gradient clipping")."""
import argparse
import ctypes
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.join(HERE, "..")

CONFIGS = {   # name: (spec builder, batch, default steps per timed window)
    "mlp284": (lambda E: E.mlp_spec(284, 8, "dueling"), 1024, 4000),
    "head": (lambda E: E.hybrid_spec(8, "dueling"), 256, 1500),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="mlp284")
    ap.add_argument("--pkg", default=os.path.join(REPO, "multimodal-drl-rmc_amd"))
    ap.add_argument("--steps", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-norm", type=float, default=1.0)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path[:0] = [REPO, os.path.abspath(args.pkg)]
    import random

    import torch

    from dqn import _capi as C
    from dqn import engine as E
    from oracle import ref as O

    assert torch.cuda.is_available(), "needs a GPU: there is nothing to measure without one"
    build, batch, steps = CONFIGS[args.config]
    steps = args.steps or steps
    spec = build(E)
    cap, fill = 20000, 10000
    eng = E.LearnEngine(spec, "DuelingDoubleDQNAgent", batch, cap)
    eng.push(*O.synth_transitions(fill, spec.obs_dim, 8, seed=5))
    random.seed(11)
    eng.set_rng(C.DQNX_RNG_PY, O.py_state_to_array())
    has_clip = hasattr(eng, "set_grad_clip")

    def run(mode, n):
        if has_clip:
            eng.set_grad_clip(args.max_norm if mode == "on" else None)
        if mode == "split":
            for _ in range(n):
                eng.learn_step(grads_only=True)
                eng.apply_grads(soft_update=True)
        else:
            for _ in range(n):
                eng.learn_step(soft_update=True)

    def window(mode):
        run(mode, 20)   # the mode's plans are built (set_grad_clip drops them) before the clock starts
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(mode, steps)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / steps   # us per step

    modes = ["off", "split", "on"] if has_clip else ["off", "split"]
    for m in modes:   # warm every shape the timed windows use
        run(m, 200)
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for _ in range(args.reps):   # off, split, on, off, split, on, ...
        for m in modes:
            times[m].append(window(m))
    eng.check_device_error()

    def summary(v):
        return {"median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "max_us": round(max(v), 3),
                "windows": len(v)}

    out = {"label": args.label, "config": args.config, "batch": batch, "n_params": eng.n_params, "steps_per_window": steps,
           "abi": int(C.lib().dqnx_abi_version()), "has_clip": has_clip}
    for m in modes:
        out["step_" + m] = summary(times[m])
    if has_clip:
        eng.set_grad_clip(args.max_norm)
        flags = C.STEP_SOFT_UPDATE
        n = C.I32()
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
        names = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(64)
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, None, None), "kernel_info")
            names.append(name.value.decode())
        out["launches_on"] = names
        ev = (ctypes.c_void_p * 2)()
        C.check(eng.L.dqnx_events_create(2, ev), "events_create")
        for kname in ("grad_sumsq", "clip_coef", "adam_clipped"):
            idx = names.index(kname)
            ks = []
            for i in range(60):
                C.check(eng.L.dqnx_learn_step_timed(eng.h, flags, idx, ev[0], ev[1], eng.stream()), "learn_step_timed")
                ms = ctypes.c_float()
                C.check(eng.L.dqnx_event_elapsed(ev[0], ev[1], ctypes.byref(ms)), "event_elapsed")
                if i >= 10:
                    ks.append(ms.value * 1000.0)
            out["kernel_" + kname] = summary(ks)
        eng.L.dqnx_events_destroy(2, ev)
        info = eng.grad_clip_info()
        out["clip_window"] = {"steps": info["steps"], "clipped_frac": round(info["clipped_frac"], 4),
                              "norm_mean": info["norm_mean"]}
        eng.set_grad_clip(None)
        C.check(eng.L.dqnx_learn_kernel_count(eng.h, flags, ctypes.byref(n)), "kernel_count")
        names = []
        for i in range(n.value):
            name = ctypes.create_string_buffer(64)
            C.check(eng.L.dqnx_learn_kernel_info(eng.h, flags, i, name, 64, None, None), "kernel_info")
            names.append(name.value.decode())
        out["launches_off"] = names
    eng.check_device_error()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
