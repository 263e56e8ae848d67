"""Idle Agent.choose_actions latency on the GPU: a drop-in DuelingDoubleDQNAgent on the MLP-284
body and on the two-stream HEAD body, n_env = 1 and 2, nothing else in flight (after flush()).

Prints one JSON line: per-call host wall time of choose_actions(obs) with host numpy observations, as
R:train.py:88-108 calls it -- the median, 10th and 90th percentile over the timed calls.

`--net two_stream84`: the (4,84,84) variant at n_env = 1 instead (a 64-transition ring), the large acting
route with DQNX_ACT_LARGE=1 in the environment, the torch forward without it; also the first call after a
learn step (the step's 1.4 GB of traffic has pushed dense 1's weights out of the Infinity Cache)."""
import functools
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-drl-rmc_amd"), os.path.join(REPO, "tests")]
from dqn import Agents  # noqa: E402
from refnets import agent_kwargs, hybrid_network_config, mlp_network_config  # noqa: E402

CALLS, WARMUP = 2000, 200


def measure(conf, n_env, obs_dim=284, batch=64, buffer=1000, calls=CALLS, warmup=WARMUP, after_learn=0):
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as d:
        agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs("DuelingDoubleDQNAgent", obs_dim, batch, buffer, d,
                                                            n_env=n_env, nn_conf_func=conf))
        agent.epsilon_start = 0.5   # greedy and random actions mixed
        x = np.random.default_rng(n_env).random((n_env, obs_dim), dtype=np.float32)
        for _ in range(warmup):
            agent.choose_actions(x)
        agent.flush()
        torch.cuda.synchronize()
        ts = np.empty(calls)
        for i in range(calls):
            t0 = time.perf_counter()
            agent.choose_actions(x)
            ts[i] = time.perf_counter() - t0
        ts *= 1e6
        out = {"median_us": float(np.median(ts)), "p10_us": float(np.percentile(ts, 10)),
               "p90_us": float(np.percentile(ts, 90)), "calls": calls}
        if after_learn:   # the first choose_actions after a learn step that has completed
            for i in range(batch):
                agent.store_transitions(x[:1], [i % 8], [0.5], [False], x[:1], None)
            ts = np.empty(after_learn)
            for i in range(after_learn):
                agent.learn()
                agent.flush()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                agent.choose_actions(x)
                ts[i] = (time.perf_counter() - t0) * 1e6
            out["after_learn_us"] = {"median": float(np.median(ts)), "min": float(ts.min()), "max": float(ts.max()),
                                     "calls": after_learn}
        return out


def main():
    out = {}
    if "two_stream84" in sys.argv[1:]:
        conf = functools.partial(hybrid_network_config, micro_chw=(4, 84, 84))
        out["DQNX_ACT_LARGE"] = os.environ.get("DQNX_ACT_LARGE")
        out["two_stream84"] = {"n_env1": measure(conf, 1, 14 + 4 * 84 * 84, 32, 64, 500, 50, after_learn=10)}
        print(json.dumps(out))
        return
    for tag, conf in (("mlp284", mlp_network_config), ("two_stream", hybrid_network_config)):
        out[tag] = {f"n_env{n}": measure(conf, n) for n in (1, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
