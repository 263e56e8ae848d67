"""The n-step window of include/dqnx.h "n-step returns", restated in numpy, and what the n-step tests
share: rings that contain every kind of window, and the census that proves it.  No GPU, no library."""
import numpy as np


def window(rew, done, size, p, n, n_env, gamma):
    """(R fp32, d fp32, disc fp32, last, m) of start position p: fp64 accumulation, one multiply and one
    add per position, the discount by repeated multiplication."""
    g, R, m, d = np.float64(1.0), np.float64(0.0), 0, np.float32(0.0)
    gamma = np.float64(gamma)
    for j in range(n):
        q = p + j * n_env
        if q >= size:
            break                       # the window reaches the newest end of the ring
        R = R + g * np.float64(rew[q])
        g = g * gamma
        m = j + 1
        if done[q] != 0:
            d = np.float32(1.0)
            break
    return np.float32(R), d, np.float32(g), p + (m - 1) * n_env, m


def windows(rew, done, size, ps, n, n_env, gamma):
    """column arrays (R, d, disc, last, m) for the start positions ps"""
    rows = [window(rew, done, size, int(p), n, n_env, gamma) for p in ps]
    R, d, disc, last, m = zip(*rows)
    return (np.asarray(R, np.float32), np.asarray(d, np.float32), np.asarray(disc, np.float32),
            np.asarray(last, np.int64), np.asarray(m, np.int64))


def kind(rew, done, size, p, n, n_env):
    """("full",) | ("done", j) with j < n the position that ended the window | ("end", m) with m < n
    positions before the newest end of the ring"""
    for j in range(n):
        q = p + j * n_env
        if q >= size:
            return ("end", j)
        if done[q] != 0:
            # a done at the last position of a full window cuts nothing off, but d = 1: its own kind
            return ("done", j)
    return ("full",)


def census(rew, done, size, ps, n, n_env):
    return {kind(rew, done, size, int(p), n, n_env) for p in ps}


def every_kind(n):
    """the kinds a test's data must contain for n_step = n: a full window, a window cut by done at each
    j < n, a window cut by the ring end at each m in 1 .. n-1"""
    return {("full",)} | {("done", j) for j in range(n)} | {("end", m) for m in range(1, n)}


def ring_scalars(count, seed, done_rate=1.0 / 6.0):
    """rewards (fp32, the synthetic env's range) and done flags at the given rate"""
    rng = np.random.default_rng(seed)
    rew = (rng.random(count) * 27.0 - 24.0).astype(np.float32)
    done = rng.random(count) < done_rate
    return rew, done
