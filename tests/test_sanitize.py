"""CPU: the host engine (csrc/engine.cpp and the host side of every .hip launcher) under
AddressSanitizer + UndefinedBehaviorSanitizer (SURVEY.md §5 "race detection / sanitizers").

`make -C multimodal-drl-rmc_amd sanitize` builds host-only objects (no device code) with
-fsanitize=address,undefined and links tests/sanitize/plan_check.cpp, which plans ~730 engine
configurations without a GPU: every network family, algorithm, dtype, batch and data-parallel
split, every row of the conv geometry sweep (tests/conv_geoms.py), their arena layouts, learn-step
launch lists for every flag set, DP bucket cuts, acting / sampler scratch sizes and the refusal
paths.  Any sanitizer report aborts the program.
(It found two reads of the engine's config after `delete e` on create's error paths.)"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "multimodal-drl-rmc_amd")


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None,
                    reason="needs hipcc (host-only compile)")
def test_host_engine_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", PKG, "-j8", "sanitize"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(PKG, "build", "plan_check")], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert ", 0 failures" in r.stdout, out[-2000:]
    _check_conv_geometry_sweep(r.stdout)


def _check_conv_geometry_sweep(stdout):
    """plan_check planned every row of tests/conv_geoms.py (its "geom" lines are that table: the C++
    program cannot import it) on the expected route, and micro_plan -- called with the 256 compute units
    of an MI355X -- gave the forward S = 1, 2 and 3 samples per workgroup at the batches
    tests/test_gpu_conv_geoms.py runs.  The GPU tests cannot observe S (the engine takes the compute
    unit count from the device); these lines are what ties their batch sizes to the code path."""
    import conv_geoms as G
    geoms, S = [], {}
    for line in stdout.splitlines():
        f = line.split()
        if f[:1] == ["geom"]:
            geoms.append(line)
        elif f[:1] == ["S"]:
            S[(f[1], int(f[2]), int(f[3]))] = int(f[4])
    want = []
    for g in G.GEOMS:
        convs = " ".join(f"{co},{kh},{kw},{sh},{sw}" for co, (kh, kw), (sh, sw) in g.conv)
        want.append(f"geom {g.name} {g.micro_chw[0]} {g.micro_chw[1]} {g.micro_chw[2]} {g.macro_len} {convs} "
                    f"dense {g.dense[0]},{g.dense[1]} {g.route}")
    assert geoms == want
    for name in G.S_ROWS:
        for nst, pins in G.S_BATCHES.items():
            assert sorted(pins.values()) == [1, 2, 3]
            for batch, s in pins.items():
                assert S[(name, nst, batch)] == s, (name, nst, batch, S[(name, nst, batch)])
    for name in G.MICRO:   # every micro row has a forward plan at every batch the GPU tests use
        for nst in (2, 3):
            for batch in G.gpu_batches(G.BY_NAME[name]):
                assert 1 <= S[(name, nst, batch)] <= 3, (name, nst, batch)
