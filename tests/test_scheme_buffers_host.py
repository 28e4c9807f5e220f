"""Who frees BatchScheme's device temporaries, checked without a device: every public method that allocates device memory, and
the six staged host-face methods of Context, run against a stand-in context that keeps a ledger of malloc and free
(tests/_scheme_buffers.py; the hostpipe calls are the real host C code).  A clean run must leave nothing allocated but what it
returned; then EVERY interaction with the stand-in in turn -- allocations, copies, launches, synchronize -- is made to raise, once
a FusionHipError and, where it is an allocation, once a MemoryError, and the same must hold when the exception reaches the
caller.  FZ_E_UNSUPPORTED from the device challenge pipeline and the device sampler is no failure: the host fallback is walked
the same way."""
import pytest

from _scheme_buffers import SECPAR, cases, context_cases, host_inputs, no_finalizers, scheme_on, stand_in_context

FALLBACKS = ("challenge_msgs_dev", "sample_secret_polys_dev")


@pytest.fixture(scope="module")
def params():
    import fusion.fusion as F
    return F.fusion_setup(SECPAR, 1)


@pytest.fixture(autouse=True)
def _leaks_stay_visible(monkeypatch):
    no_finalizers(monkeypatch)


def _run(params, name, fail_at=None, kind=None, unsupported=()):
    """one call of case `name` on a fresh stand-in -> (context, complaints of the ledger, the exception that reached the caller)"""
    from fusion_hip import FusionHipError
    from fusion_hip.context import DeviceArray
    ctx = stand_in_context(params)
    if name.startswith("Context."):
        call, args, bs = context_cases(params)[name], (ctx,), None
    else:
        bs, a = scheme_on(ctx, params), host_inputs(params)
        if name.endswith("[device]"):
            a = {k: DeviceArray.from_numpy(ctx, v) for k, v in a.items()}
        call, args = cases()[name], (bs, a)
    before = set(ctx.ledger.live)
    ctx.unsupported = unsupported
    del ctx.names[:], ctx.calls[:]
    ctx.arm(fail_at, kind)
    result = raised = None
    try:
        result = call(*args)
    except (FusionHipError, MemoryError) as e:
        raised = e
    finally:
        if bs is not None and bs._pool is not None:
            bs._pool.shutdown(wait=True)
    return ctx, ctx.ledger.settle(before, result), raised


def _all_names():
    import types
    return list(cases()) + list(context_cases(types.SimpleNamespace(degree=64)))


def test_the_ledger_sees_a_leak_and_a_second_free(params):
    from fusion_hip.context import DeviceArray
    ctx = stand_in_context(params)
    kept = DeviceArray(ctx, (4,))
    assert ctx.ledger.settle(set(), None) == ["1 buffer(s) of [16] bytes left allocated"]
    ptr = kept.ptr
    kept.free()
    assert ctx.ledger.settle(set(), None) == []
    ctx.free(ptr)
    assert "freed before" in ctx.ledger.settle(set(), None)[0]


@pytest.mark.parametrize("name", _all_names())
def test_every_temporary_is_freed_once_whatever_raises(params, name):
    clean, wrong, raised = _run(params, name)
    assert raised is None and not wrong, (name, raised, wrong)
    assert len(clean.names) >= 2, (name, clean.names)
    walks = [((), clean.names)]
    if any(n in FALLBACKS for n in clean.names):                        # the host fallbacks: no failure, and they balance too
        fb, wrong, raised = _run(params, name, unsupported=FALLBACKS)
        assert raised is None and not wrong, (name, "fallback", raised, wrong)
        walks.append((FALLBACKS, fb.names))
    for unsupported, names in walks:
        for k, interaction in enumerate(names, 1):
            for kind in ("error", "memory") if interaction == "malloc" else ("error",):
                _, wrong, raised = _run(params, name, k, kind, unsupported)
                what = (name, unsupported, k, interaction, kind, raised, wrong)
                assert raised is not None and f"injected at interaction {k} " in str(raised), what
                assert isinstance(raised, MemoryError) == (kind == "memory"), what
                assert not wrong, what
