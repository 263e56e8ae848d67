"""CPU: the training-state blob parser (include/dqnx.h "training-state snapshot") without a GPU.

The Python part builds a small valid blob by hand from the documented layout (struct.pack, no
library help: MLP-14, capacity 8, fill 3) and checks dqnx_state_inspect on it, on every truncation
and on a list of corruptions.  The sanitizer part builds tests/sanitize/state_check.cpp against the
host-only AddressSanitizer + UndefinedBehaviorSanitizer objects (`make sanitize-state`) and runs it
as an ordinary executable: the same walk in C++ on exactly-sized heap copies, plus
dqnx_state_bytes on engines created without a GPU."""
import ctypes
import os
import shutil
import struct
import subprocess

import pytest

from dqn import _capi as C
from dqn import engine as E

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "multimodal-drl-rmc_amd")

HDR = 608            # sizeof(dqnx_state_info): 24 + 148 (net) + 20 + 32 + 16 * 24
NET_OFF = 24
ALGO_OFF = 172       # algo, compute_dtype, per_numpy121, n_sections, reserved0
CAP_OFF = 192        # capacity, n_params, ring_size, ring_wptr
SEC_OFF = 224
CTRL_BYTES = 5136    # sizeof(dqnx_ctrl): 2 * 625 * 4 + 6 * 8 + 4 * 4 + 8 + 8 * 8
CTRL_RING_SIZE = 5000


def make_blob(obs_dim=14, hidden=(256, 128), n_actions=8, cap=8, fill=3, wptr=3, per=False):
    """The documented layout, by hand (dueling MLP, ReLU)."""
    P = 0
    d = obs_dim
    for w in hidden:
        P += d * w + w
        d = w
    P += d * 1 + 1 + d * n_actions + n_actions          # fc_val, fc_adv
    net = [C.DQNX_NET_MLP, C.DQNX_HEAD_DUELING, C.DQNX_ACT_RELU, obs_dim, n_actions, len(hidden)]
    net += list(hidden) + [0] * (6 - len(hidden)) + [0] * (5 + 20)
    assert len(net) == 37
    # (id, bytes) back to back in file order: the fp64 tree right after the control block
    secs = [(C.SEC_PARAMS, P * 4), (C.SEC_TARGET_PARAMS, P * 4), (C.SEC_ADAM_M, P * 4), (C.SEC_ADAM_V, P * 4),
            (C.SEC_CTRL, CTRL_BYTES)] + ([(C.SEC_SUMTREE, (2 * cap - 1) * 8)] if per else []) + \
           [(C.SEC_RING_OBS, fill * obs_dim * 4), (C.SEC_RING_NEXT_OBS, fill * obs_dim * 4), (C.SEC_RING_ACT, fill * 4),
            (C.SEC_RING_REW, fill * 4), (C.SEC_RING_DONE, fill * 4)]
    table, cur = [], HDR
    for sid, n in secs:
        table.append((sid, 0, cur, n))
        cur += n
    total = cur
    h = struct.pack("<QIIQ", C.STATE_MAGIC, C.STATE_VERSION, HDR, total)
    h += struct.pack("<37i", *net)
    h += struct.pack("<5i", C.DQNX_ALGO_PER_DOUBLE if per else C.DQNX_ALGO_DOUBLE, 0, 0, len(table), 0)
    h += struct.pack("<4q", cap, P, fill, wptr)
    for t in table:
        h += struct.pack("<IIQQ", *t)
    h += b"\0" * (24 * (16 - len(table)))
    assert len(h) == HDR
    b = bytearray(total)
    b[:HDR] = h
    ctrl = bytearray(CTRL_BYTES)
    struct.pack_into("<I", ctrl, 624 * 4, 624)                 # py_mt position
    struct.pack_into("<I", ctrl, 625 * 4 + 624 * 4, 624)       # np_mt position
    struct.pack_into("<6q", ctrl, CTRL_RING_SIZE, fill, wptr, 0, 0, cap - 1, cap - 1)
    off = table[4][2]
    b[off:off + CTRL_BYTES] = ctrl
    return b, {"P": P, "table": table, "ctrl_off": off}


def inspect_rc(blob):
    buf = (ctypes.c_ubyte * max(len(blob), 1)).from_buffer_copy(bytes(blob) or b"\0")
    info = C.StateInfo()
    rc = C.lib().dqnx_state_inspect(buf, len(blob), ctypes.byref(info))
    return rc, info, C.lib().dqnx_last_error().decode(errors="replace")


def test_layout_constants_match_the_header():
    assert ctypes.sizeof(C.StateInfo) == HDR and ctypes.sizeof(C.StateSection) == 24
    assert ctypes.sizeof(C.Ctrl) == CTRL_BYTES and C.Ctrl.ring_size.offset == CTRL_RING_SIZE
    assert C.StateInfo.net.offset == NET_OFF and C.StateInfo.algo.offset == ALGO_OFF
    assert C.StateInfo.capacity.offset == CAP_OFF and C.StateInfo.sections.offset == SEC_OFF
    assert struct.pack("<Q", C.STATE_MAGIC) == b"DQNXSTAT"
    prog = r'''#include <stdio.h>
#include <stddef.h>
#include "%s"
int main(void) { printf("%%zu %%zu %%zu %%zu %%zu\n", sizeof(dqnx_state_info), offsetof(dqnx_state_info, net),
  offsetof(dqnx_state_info, algo), offsetof(dqnx_state_info, capacity), offsetof(dqnx_state_info, sections)); return 0; }
''' % os.path.join(REPO, "include", "dqnx.h")
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        src, exe = os.path.join(td, "l.c"), os.path.join(td, "l")
        open(src, "w").write(prog)
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    assert got == [HDR, NET_OFF, ALGO_OFF, CAP_OFF, SEC_OFF]


@pytest.mark.parametrize("per", [False, True])
def test_inspect_returns_the_fingerprint(per):
    blob, meta = make_blob(per=per, fill=8 if per else 3, wptr=5 if per else 3)
    rc, info, msg = inspect_rc(blob)
    assert rc == C.DQNX_OK, msg
    assert (info.net.obs_dim, info.net.n_actions, info.net.n_dense, tuple(info.net.dense[:2])) == (14, 8, 2, (256, 128))
    assert info.algo == (C.DQNX_ALGO_PER_DOUBLE if per else C.DQNX_ALGO_DOUBLE)
    assert (info.capacity, info.n_params, info.ring_size, info.ring_wptr) == (8, meta["P"], 8 if per else 3, 5 if per else 3)
    assert [(s.id, s.reserved, s.offset, s.bytes) for s in info.sections[:info.n_sections]] == meta["table"]
    d = E.inspect_state_blob(bytes(blob))
    assert d["capacity"] == 8 and d["ring_size"] == info.ring_size and d["net"]["dense"] == (256, 128)
    assert d["sections"]["ctrl"] == (meta["ctrl_off"], CTRL_BYTES) and ("sumtree" in d["sections"]) == per
    # the parameter count the hand layout uses is the library's
    n, _ = E.mlp_spec(14, 8, "dueling").param_infos()
    assert n == meta["P"]


def test_every_truncation_is_refused():
    blob, _ = make_blob()
    buf = (ctypes.c_ubyte * len(blob)).from_buffer(blob)   # one buffer, every length (state_check.cpp walks
    info, f = C.StateInfo(), C.lib().dqnx_state_inspect     # exactly-sized copies under the sanitizers)
    bad = [n for n in range(len(blob)) if f(buf, n, ctypes.byref(info)) != C.DQNX_EINVAL]
    assert not bad, bad[:10]


def _poke(fmt, off, *v):
    return lambda b, m: struct.pack_into(fmt, b, off, *v)


def _overflow(b, m):   # ring_size = capacity = 2^62 rows of 56 bytes: the section size overflows 64 bits
    struct.pack_into("<q", b, CAP_OFF, 1 << 62)
    struct.pack_into("<2q", b, CAP_OFF + 16, 1 << 62, 0)
    struct.pack_into("<2q", b, m["ctrl_off"] + CTRL_RING_SIZE, 1 << 62, 0)


CORRUPTIONS = {
    "bad magic": _poke("<B", 0, 0x45),
    "future version": _poke("<I", 8, C.STATE_VERSION + 1),
    "version 0": _poke("<I", 8, 0),
    "section offset past the end": lambda b, m: struct.pack_into("<Q", b, SEC_OFF + 24 * 5 + 8, len(b) + 64),
    "section offset + size wraps": _poke("<Q", SEC_OFF + 24 * 5 + 8, (1 << 64) - 64),
    "section size product overflows": _overflow,
    "ring_size > capacity": _poke("<q", CAP_OFF + 16, 9),
    "negative wptr": _poke("<q", CAP_OFF + 24, -1),
    "wptr of an unwrapped ring": _poke("<q", CAP_OFF + 24, 5),
    "section size": lambda b, m: struct.pack_into("<Q", b, SEC_OFF + 24 * 7 + 16, 16),
    "n_params": lambda b, m: struct.pack_into("<q", b, CAP_OFF + 8, m["P"] + 1),
    "unknown section id": _poke("<I", SEC_OFF + 24 * 3, 12),
    "control block ring_size": lambda b, m: struct.pack_into("<q", b, m["ctrl_off"] + CTRL_RING_SIZE, 2),
    "MT position": lambda b, m: struct.pack_into("<I", b, m["ctrl_off"] + 624 * 4, 625),
    "SumTree index": lambda b, m: struct.pack_into("<q", b, m["ctrl_off"] + CTRL_RING_SIZE + 32, 15),
    "device error set": lambda b, m: struct.pack_into("<i", b, m["ctrl_off"] + CTRL_RING_SIZE + 52, 2),
}


@pytest.mark.parametrize("name", sorted(CORRUPTIONS))
def test_corrupt_blob_is_refused(name):
    blob, meta = make_blob()
    CORRUPTIONS[name](blob, meta)
    rc, _, msg = inspect_rc(blob)
    assert rc == C.DQNX_EINVAL and msg, (name, rc, msg)
    with pytest.raises(C.DqnxError) as ei:
        E.inspect_state_blob(bytes(blob))
    assert ei.value.code == C.DQNX_EINVAL


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("hipcc") is None,
                    reason="needs hipcc (host-only compile)")
def test_state_check_under_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", PKG, "-j8", "sanitize-state"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    # a sanitized process never opens a GPU: with no device visible, engine creation keeps its planning
    # defaults (the "engine without a GPU" this program is about) wherever the test runs
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([os.path.join(PKG, "build", "state_check")], capture_output=True, text=True, timeout=120, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
    assert ", 0 failures" in r.stdout, out[-2000:]
