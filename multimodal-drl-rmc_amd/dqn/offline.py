"""Offline training: fit a Q-network to transitions that already exist.

A replay ring saved with LearnEngine.save_state (or filled from logged baseline controllers and saved) is
loaded into a fresh engine whose batch, learning rate, discount, loss and seeds may differ, and trained with
learn_steps: no simulator, no host work between steps.  On a fixed dataset plain (double) DQN over-estimates
the actions the data never took; set_cql_alpha turns on the CQL(H) regulariser that keeps it conservative
(include/dqnx.h "conservative Q-learning").

    eng = offline.engine_from_state("run.dqnx", batch=1024, lr=3e-4, cql_alpha=1.0)
    log = offline.fit(eng, 20000, log_every=1000)
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


def fit(engine: LearnEngine, steps: int, soft_update: bool = True, log_every: int = 0) -> List[dict]:
    """`steps` learn steps on the engine's ring, in learn_steps calls of at most FIT_CHUNK (cut at the log
    boundaries), bitwise the same as that many learn_step(soft_update) calls.  log_every > 0: after every
    log_every-th step (and after the last) one record {"step", "loss", "cql_gap", "q_sa_mean"} of that
    step is read from the device (step counts from 1 within this call; cql_gap is the mean logsumexp_a
    Q(s, a) - Q(s, a_b) whether or not the regulariser is on).  No other host work."""
    out: List[dict] = []
    done, steps = 0, int(steps)
    while done < steps:
        n = min(FIT_CHUNK, steps - done)
        if log_every > 0:
            n = min(n, log_every - done % log_every)
        engine.learn_steps(n, soft_update=soft_update)
        done += n
        if log_every > 0 and (done % log_every == 0 or done == steps):
            torch.cuda.synchronize(engine.device)
            engine.check_device_error()
            out.append({"step": done, "loss": engine.loss(), "cql_gap": engine.cql_gap(),
                        "q_sa_mean": float(engine.td[1].mean())})
    return out
