"""Host only: `dqnx_act_kernel_count`, the acting path's plan introspection (the counterpart of
dqnx_learn_kernel_count): how many launches dqnx_act makes for n rows of a net, without a GPU."""
import ctypes

from dqn import _capi as C
from dqn import engine as E


def _count(spec, n):
    d = spec.to_c()
    k = C.I32(-1)
    rc = C.lib().dqnx_act_kernel_count(ctypes.byref(d), n, ctypes.byref(k))
    return rc, k.value


def test_act_kernel_count_per_net(monkeypatch):
    monkeypatch.delenv("DQNX_ACT_TS", raising=False)
    monkeypatch.delenv("DQNX_ACT_TS_ROWS", raising=False)
    assert _count(E.mlp_spec(284), 1) == (C.DQNX_OK, 1)
    head = E.hybrid_spec()   # the reference's HEAD net: the conv stack as one launch, then the MLP kernel
    assert _count(head, 1) == (C.DQNX_OK, 2)
    # the count is what runs: by default the stack is taken only where it measured faster than the
    # per-conv launches (one row); DQNX_ACT_TS=2 takes it for every n it applies to
    assert _count(head, 37) == (C.DQNX_OK, 4)
    monkeypatch.setenv("DQNX_ACT_TS", "2")
    assert _count(head, 1) == (C.DQNX_OK, 2)
    assert _count(head, 37) == (C.DQNX_OK, 2)
    assert _count(head, 257) == (C.DQNX_OK, 4)   # (the stack's row cap)
    # a single conv has no layer to split over workgroups: one conv launch plus the MLP kernel
    one = E.hybrid_spec(conv=E.HYBRID_CONV[:1])
    assert _count(one, 1) == (C.DQNX_OK, 2)
    monkeypatch.setenv("DQNX_ACT_TS", "0")   # the per-conv launches for every net
    assert _count(head, 1) == (C.DQNX_OK, 4)
    assert _count(head, 37) == (C.DQNX_OK, 4)
    assert _count(one, 1) == (C.DQNX_OK, 2)
    assert _count(E.mlp_spec(284), 1) == (C.DQNX_OK, 1)


def test_act_kernel_count_refusals():
    big = E.hybrid_spec(micro_chw=(4, 84, 84))   # stays on the torch forward (tests/test_gpu_act.py)
    rc, _ = _count(big, 1)
    assert rc == C.DQNX_EUNSUPPORTED
    assert not E.act_supported(big)
    assert E.act_supported(E.hybrid_spec())
    L = C.lib()
    d = E.hybrid_spec().to_c()
    k = C.I32(0)
    assert L.dqnx_act_kernel_count(ctypes.byref(d), 1, None) == C.DQNX_EINVAL
    assert L.dqnx_act_kernel_count(ctypes.byref(d), -1, ctypes.byref(k)) == C.DQNX_EINVAL


def test_act_scratch_serves_smaller_row_counts_two_stream():
    """One scratch sized for N rows serves every n <= N on either conv route: the bytes never decrease
    with n, and stay positive for every geometry the acting kernels take."""
    L = C.lib()
    for chw, ml in (((2, 27, 5), 14), ((2, 9, 4), 6), ((2, 8, 4), 16), ((2, 3, 3), 2)):
        d = E.hybrid_spec(micro_chw=chw, macro_len=ml).to_c()
        sizes = [L.dqnx_act_scratch_bytes(ctypes.byref(d), n) for n in range(1, 300)]
        assert sizes[0] > 0
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
