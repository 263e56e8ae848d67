"""Idle Agent.choose_actions latency on the GPU: a drop-in DuelingDoubleDQNAgent on the MLP-284
body and on the two-stream HEAD body, n_env = 1 and 2, nothing else in flight (after flush()).

Prints one JSON line: per-call host wall time of choose_actions(obs) with host numpy observations, as
R:train.py:88-108 calls it -- the median, 10th and 90th percentile over the timed calls."""
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


def measure(conf, n_env):
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as d:
        agent = Agents.DuelingDoubleDQNAgent(**agent_kwargs("DuelingDoubleDQNAgent", 284, 64, 1000, d, n_env=n_env,
                                                            nn_conf_func=conf))
        agent.epsilon_start = 0.5   # greedy and random actions mixed
        x = np.random.default_rng(n_env).random((n_env, 284), dtype=np.float32)
        for _ in range(WARMUP):
            agent.choose_actions(x)
        agent.flush()
        torch.cuda.synchronize()
        ts = np.empty(CALLS)
        for i in range(CALLS):
            t0 = time.perf_counter()
            agent.choose_actions(x)
            ts[i] = time.perf_counter() - t0
        ts *= 1e6
        return {"median_us": float(np.median(ts)), "p10_us": float(np.percentile(ts, 10)),
                "p90_us": float(np.percentile(ts, 90)), "calls": CALLS}


def main():
    out = {}
    for tag, conf in (("mlp284", mlp_network_config), ("two_stream", hybrid_network_config)):
        out[tag] = {f"n_env{n}": measure(conf, n) for n in (1, 2)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
