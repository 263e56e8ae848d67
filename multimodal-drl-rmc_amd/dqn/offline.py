"""Offline training: fit a Q-network to transitions that already exist.

A replay ring saved with LearnEngine.save_state (or filled from logged baseline controllers and saved) is
loaded into a fresh engine whose batch, learning rate, discount, loss and seeds may differ, and trained with
learn_steps: no simulator, no host work between steps.  On a fixed dataset plain (double) DQN over-estimates
the actions the data never took; set_cql_alpha turns on the CQL(H) regulariser that keeps it conservative
(include/dqnx.h "conservative Q-learning").

    eng = offline.engine_from_state("run.dqnx", batch=1024, lr=3e-4, cql_alpha=1.0)
    log = offline.fit(eng, 20000, log_every=1000)

A validation signal without a simulator: evaluate() sweeps a range of a ring with the current weights on the
device and touches nothing of the training state (include/dqnx.h "offline evaluation"); split() makes a
training and a held-out engine from one saved ring, and fit(validate=...) reports val_* at its boundaries.

    train, val = offline.split("run.dqnx", holdout=20000, batch=1024, cql_alpha=1.0)
    log = offline.fit(train, 20000, log_every=1000, validate=val, validate_every=1000)

What evaluate() reports are properties of the Q function.  fqe() estimates the discounted return of a candidate
POLICY from the logged transitions alone (fitted Q evaluation, include/dqnx.h "fitted Q evaluation"): the
policy's actions are computed once per ring slot, a fresh network is fitted to r + gamma * Q_target(s', pi(s')),
and the mean of Q(s0, pi(s0)) over episode-start states is the estimate.

    est = offline.fqe(candidate_engine, "run.dqnx", 5000, batch=1024, lr=3e-4)["value"]
"""
import ctypes
from typing import List, Optional

import numpy as np
import torch

from . import _capi as C
from .engine import LearnEngine, NetSpec, inspect_state_blob

FIT_CHUNK = 256   # learn steps per dqnx_learn_steps call

# the algorithm an engine is created with when the caller names none: the blob records only the id
_ALGO_NAMES = {C.DQNX_ALGO_DQN: "DQNAgent", C.DQNX_ALGO_DOUBLE: "DoubleDQNAgent",
               C.DQNX_ALGO_PER_DOUBLE: "PerDuelingDoubleDQNAgent"}


def _read_blob(path_or_blob):
    if isinstance(path_or_blob, (bytes, bytearray, memoryview)) or hasattr(path_or_blob, "__array_interface__"):
        return path_or_blob
    if hasattr(path_or_blob, "read"):
        return path_or_blob.read()
    with open(path_or_blob, "rb") as f:
        return f.read()


def engine_from_state(path_or_blob, algo: Optional[str] = None, batch: Optional[int] = None,
                      **engine_kwargs) -> LearnEngine:
    """A LearnEngine built for a training-state blob (a path, a binary file object, bytes or a uint8 array),
    with the blob loaded: the network of the blob's header, the blob's capacity and its prioritised-or-not
    kind.  algo: a LearnEngine algorithm name (default: the one of the blob's algorithm id; a prioritised
    blob needs a prioritised algorithm and the other way round).  batch: default 32.  engine_kwargs go to
    LearnEngine (lr, gamma, tau, cql_alpha, compute_dtype, ...)."""
    blob = _read_blob(path_or_blob)
    info = inspect_state_blob(blob)
    a = np.frombuffer(blob, dtype=np.uint8) if not isinstance(blob, np.ndarray) else np.ascontiguousarray(blob).view(np.uint8)
    head = C.StateInfo()
    C.check(C.lib().dqnx_state_inspect(ctypes.c_void_p(a.ctypes.data), a.nbytes, ctypes.byref(head)), "state_inspect")
    spec = NetSpec.from_c(head.net)   # the header's dqnx_net_desc
    if algo is None:
        algo = _ALGO_NAMES[info["algo"]]
    eng = LearnEngine(spec, algo, 32 if batch is None else int(batch), info["capacity"], **engine_kwargs)
    eng.load_state_blob(blob)
    return eng


def ring_rows(engine: LearnEngine):
    """The engine's replay rows in logical order (0 = oldest) as host arrays (obs, act, rew, done, next_obs),
    read through the ring buffer views."""
    engine.launch_recorded()
    n, cap = engine.ring_size, engine.capacity
    slots = (torch.arange(n, device=engine.device) + (engine.ring_wptr - n)) % cap
    D = engine.spec.obs_dim
    return (engine.ring_obs[slots, :D].cpu().numpy(), engine.ring_act[slots].cpu().numpy(),
            engine.ring_rew[slots].cpu().numpy(), engine.ring_done[slots].cpu().numpy() != 0,
            engine.ring_next_obs[slots, :D].cpu().numpy())


def _refill(engine: LearnEngine, rows, lo: int, hi: int) -> None:
    """The engine's ring := rows [lo, hi): the parameters and both RNG states stay, the ring, the Adam state
    and (prioritised engines) the priorities start fresh, as dqnx_engine_reset leaves them."""
    rng = [engine.get_rng(w) for w in (C.DQNX_RNG_PY, C.DQNX_RNG_NP)]
    engine.reset()
    for w, st in zip((C.DQNX_RNG_PY, C.DQNX_RNG_NP), rng):
        engine.set_rng(w, st)
    step = max(engine.cfg.n_env, 1) * max(1, 4096 // max(engine.cfg.n_env, 1))   # whole time steps per push
    for a in range(lo, hi, step):
        b = min(a + step, hi)
        engine.push(*[r[a:b] for r in rows])


def split(path_or_blob, holdout: int, **kw):
    """(train, val): two engines from one saved ring.  The validation ring is the newest `holdout` rows,
    rounded down to whole time steps (n_env rows, kw's n_env or 1), the training ring the rows before them,
    both in the saved order.  Both engines are engine_from_state(path_or_blob, **kw) -- the blob's parameters
    and RNG states -- refilled through the ring buffer views and replay_push; their Adam state (and a
    prioritised engine's priorities) start fresh."""
    blob = _read_blob(path_or_blob)
    train = engine_from_state(blob, **kw)
    val = engine_from_state(blob, **kw)
    n_env = max(int(kw.get("n_env", 1)), 1)
    n = train.ring_size
    hold = int(holdout) // n_env * n_env
    if hold < 1 or hold >= n:
        raise ValueError(f"holdout of {holdout} rows (whole time steps: {hold}) leaves no split of {n} rows")
    rows = ring_rows(train)
    _refill(train, rows, 0, n - hold)
    _refill(val, rows, n - hold, n)
    return train, val


def evaluate(engine: LearnEngine, data: Optional[LearnEngine] = None, lo: int = 0, hi: Optional[int] = None) -> dict:
    """engine's weights on replay rows [lo, hi): LearnEngine.evaluate on the engine's own ring, or (data: another
    engine of the same network whose ring holds the validation transitions) on data's ring after copying the
    online and target parameters into it.  Nothing of `engine` changes; of `data` only its parameters."""
    if data is None or data is engine:
        return engine.evaluate(lo, hi)
    engine.launch_recorded()
    data.launch_recorded()
    data.params.copy_(engine.params)
    data.target_params.copy_(engine.target_params)
    data.params_modified()
    return data.evaluate(lo, hi)


def fit(engine: LearnEngine, steps: int, soft_update: bool = True, log_every: int = 0,
        validate: Optional[LearnEngine] = None, validate_every: int = 0) -> List[dict]:
    """`steps` learn steps on the engine's ring, in learn_steps calls of at most FIT_CHUNK (cut at the log
    boundaries), bitwise the same as that many learn_step(soft_update) calls.  log_every > 0: after every
    log_every-th step (and after the last) one record {"step", "loss", "cql_gap", "q_sa_mean"} of that
    step is read from the device (step counts from 1 within this call; cql_gap is the mean logsumexp_a
    Q(s, a) - Q(s, a_b) whether or not the regulariser is on).  No other host work.
    validate_every > 0: after every validate_every-th step (and after the last) the weights are evaluated on
    `validate`'s ring (None: the engine's own) with evaluate(); the record of that boundary -- a new one if
    log_every made none -- gains val_loss, val_cql_gap, val_agree, val_q_sa_mean, val_v_mean and val_abs_td_mean.
    The learn steps are bitwise what they are without validation."""
    out: List[dict] = []
    done, steps = 0, int(steps)
    validate_every = int(validate_every)
    while done < steps:
        n = min(FIT_CHUNK, steps - done)
        if log_every > 0:
            n = min(n, log_every - done % log_every)
        if validate_every > 0:
            n = min(n, validate_every - done % validate_every)
        engine.learn_steps(n, soft_update=soft_update)
        done += n
        logged = log_every > 0 and (done % log_every == 0 or done == steps)
        if logged:
            torch.cuda.synchronize(engine.device)
            engine.check_device_error()
            out.append({"step": done, "loss": engine.loss(), "cql_gap": engine.cql_gap(),
                        "q_sa_mean": float(engine.td[1].mean())})
        if validate_every > 0 and (done % validate_every == 0 or done == steps):
            if not logged:
                out.append({"step": done})
            ev = evaluate(engine, validate)
            engine.check_device_error()
            out[-1].update({"val_loss": ev["loss"], "val_cql_gap": ev["cql_gap"], "val_agree": ev["agree"],
                            "val_q_sa_mean": ev["q_sa_mean"], "val_v_mean": ev["v_mean"],
                            "val_abs_td_mean": ev["abs_td_mean"]})
    return out


def fresh_params(engine: LearnEngine, seed: int) -> dict:
    """name -> tensor: a fresh parameter set for the engine's network from `seed`, by torch's default rule for
    Linear / Conv2d (weights and biases uniform in +-1 / sqrt(fan_in)), drawn from a CPU generator in
    state_dict order."""
    g = torch.Generator(device="cpu")
    g.manual_seed(int(seed))
    out, fan_in = {}, 1
    for name, _, shape in engine.param_layout:
        if len(shape) >= 2:
            fan_in = int(np.prod(shape[1:]))
        bound = 1.0 / float(max(fan_in, 1)) ** 0.5
        out[name] = (torch.rand(tuple(shape), generator=g, dtype=torch.float32) * 2.0 - 1.0) * bound
    return out


def fresh_fit_state(engine: LearnEngine, seed: int) -> None:
    """Both networks := fresh_params(engine, seed); the Adam moments and step count start from zero.  The ring,
    the RNG states and (prioritised engines) the priorities stay."""
    engine.launch_recorded()
    engine.load_params(fresh_params(engine, seed))
    engine.adam_m.zero_()
    engine.adam_v.zero_()
    off = C.Ctrl.adam_step.offset
    engine.ctrl_bytes[off:off + 8].zero_()


def fqe(policy, data, steps: int, soft_update: bool = True, seed: int = 0, log_every: int = 0, **engine_kw) -> dict:
    """Fitted Q evaluation of `policy` on the transitions of `data`.
    policy: a LearnEngine (its online network) or a state_dict-like name -> tensor of the data's network.
    data: a training-state blob (a path, a file object, bytes, a uint8 array) or a LearnEngine (its state_blob()).
    A data engine is built with engine_from_state(data, **engine_kw) (batch, lr, gamma, tau, algo, ...); the policy
    goes into its online parameters and policy_actions() sweeps the whole ring once; then both networks are
    re-initialised from `seed` (fresh_fit_state), the table is set as the target policy and fit() runs `steps`
    learn steps.  Returns fqe_value()'s dict over the whole ring -- "value" is the estimate of the policy's
    discounted return from the episode starts -- plus "log" (fit's records) and "steps".  `policy` and a `data`
    engine are not changed.
    A prioritised blob gives a prioritised engine by default: the fit then samples by the blob's priorities
    (updated by the fit's own |delta|), which weights the regression towards high-priority rows and changes what
    "value" estimates.  A prioritised blob needs a prioritised algorithm (engine_from_state), so for the estimate
    under uniform sampling push ring_rows() of the prioritised engine into a uniform LearnEngine and pass that
    engine as `data`."""
    blob = data.state_blob() if isinstance(data, LearnEngine) else _read_blob(data)
    eng = engine_from_state(blob, **engine_kw)
    if isinstance(policy, LearnEngine):
        policy.launch_recorded()
        eng.params.copy_(policy.params)
        eng.params_modified()
    else:
        eng.load_params(policy)
    table = eng.policy_actions()
    fresh_fit_state(eng, seed)
    eng.set_target_policy(table)
    try:
        log = fit(eng, steps, soft_update=soft_update, log_every=log_every)
        torch.cuda.synchronize(eng.device)
        eng.check_device_error()
        out = eng.fqe_value(table)
    finally:
        eng.set_target_policy(None)
    out["log"] = log
    out["steps"] = int(steps)
    return out
