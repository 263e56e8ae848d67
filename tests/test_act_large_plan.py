"""Host only: the acting path's large route (DQNX_ACT_LARGE; csrc/act_large.hip) as the plan reports it --
`dqnx_act_kernel_count`, `dqnx_act_scratch_bytes`, `E.act_supported` -- for nets whose conv images or
first dense layer do not fit a workgroup's LDS.  No GPU."""
import ctypes

import pytest

from dqn import _capi as C
from dqn import engine as E

CHUNK = 8   # rows per chunk of the large route (kActWideRows)


def _large_nets():
    return [E.hybrid_spec(micro_chw=(4, 84, 84)),
            E.hybrid_spec(micro_chw=(2, 45, 19), macro_len=13),
            E.mlp_spec(9001, 8, "dueling")]


def _count(spec, n):
    d = spec.to_c()
    k = C.I32(-1)
    rc = C.lib().dqnx_act_kernel_count(ctypes.byref(d), n, ctypes.byref(k))
    return rc, k.value


def _bytes(spec, n):
    return int(C.lib().dqnx_act_scratch_bytes(ctypes.byref(spec.to_c()), n))


@pytest.fixture(autouse=True)
def _no_route_knobs(monkeypatch):
    for k in ("DQNX_ACT_LARGE", "DQNX_ACT_TS", "DQNX_ACT_TS_ROWS"):
        monkeypatch.delenv(k, raising=False)


def test_act_large_accepts_nets_that_do_not_fit_lds(monkeypatch):
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    for spec in _large_nets():
        rc, k = _count(spec, 1)
        assert rc == C.DQNX_OK and k > 0, (spec, rc, k)
        assert _bytes(spec, 1) > 0
        assert E.act_supported(spec)


def test_act_large_knob_is_part_of_the_plan_cache(monkeypatch):
    """The plans made under the knob do not answer for the same nets once it is gone (one process, one
    thread: the plan cache is keyed on the knob)."""
    head = E.hybrid_spec()
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    for spec in _large_nets():
        assert _count(spec, 1)[0] == C.DQNX_OK
    assert _count(head, 1) == (C.DQNX_OK, 2)
    monkeypatch.delenv("DQNX_ACT_LARGE")
    for spec in _large_nets():
        assert _count(spec, 1)[0] == C.DQNX_EUNSUPPORTED, spec
        assert _bytes(spec, 1) == 0
        assert not E.act_supported(spec)
    assert _count(head, 1) == (C.DQNX_OK, 2)
    assert _count(head, 8) == (C.DQNX_OK, len(head.conv) + 1)
    monkeypatch.setenv("DQNX_ACT_LARGE", "0")
    for spec in _large_nets():
        assert _count(spec, 1)[0] == C.DQNX_EUNSUPPORTED, spec


def test_act_large_leaves_nets_that_fit_alone(monkeypatch):
    head, mlp = E.hybrid_spec(), E.mlp_spec(284)
    rows = (1, 2, 8, 37)
    off = [(_count(s, n), _bytes(s, n)) for s in (head, mlp) for n in rows]
    assert all(rc == C.DQNX_OK for (rc, _), _ in off)
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    assert [(_count(s, n), _bytes(s, n)) for s in (head, mlp) for n in rows] == off
    monkeypatch.setenv("DQNX_ACT_LARGE", "2")   # forced: a launch per conv, dense 1, its reduce, the rest
    forced = [_count(s, n) for s in (head, mlp) for n in rows]
    want = [(C.DQNX_OK, (len(s.conv) + 3) * ((n + CHUNK - 1) // CHUNK)) for s in (head, mlp) for n in rows]
    assert forced == want
    assert all(f[1] != o[0][1] for f, o in zip(forced, off))


def test_act_large_scratch_is_chunked(monkeypatch):
    monkeypatch.setenv("DQNX_ACT_LARGE", "1")
    for spec in _large_nets():
        sizes = [_bytes(spec, n) for n in range(1, 300)]
        assert sizes[0] > 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        # rows beyond a chunk reuse the chunk's intermediates: nothing grows from 64 to 256 rows (the MLP
        # acting kernel's part is sized for a chunk as well)
        assert _bytes(spec, 256) == _bytes(spec, 64) == _bytes(spec, CHUNK)
    big = E.hybrid_spec(micro_chw=(4, 84, 84))
    one_row = 2 * 903168 + 4 * 56462   # two conv intermediates and the dense input of one row
    assert _bytes(big, 256) < 2 * CHUNK * (one_row + 57 * 512 * 4)
