"""Who frees BatchScheme's device temporaries, on the device: the calls of tests/test_scheme_buffers_host.py on a private-context
BatchScheme whose context is wrapped by a recorder that forwards everything and keeps the ledger of malloc and free
(tests/_scheme_buffers.py), with real keys, signatures and records the scheme made itself.  Per call: the ledger balances, the
result equals the same call on an unwrapped scheme; then the recorder raises -- a Python exception, before it forwards the last
launch of the call; nothing is done to the device -- and the ledger must balance again and the next call on the same scheme
give the right result."""
import numpy as np
import pytest

from _scheme_buffers import MESSAGES, SECPAR, SIZES, Ledger, cases, no_finalizers

pytestmark = pytest.mark.gpu


class Recorder:
    """forwards every call to the context, keeps the ledger, and raises instead of forwarding call number `fail_at`"""

    def __init__(self, ctx):
        self._ctx, self.ledger, self.names, self.fail_at = ctx, Ledger(), [], None

    def malloc(self, nbytes):
        ptr = self._ctx.malloc(nbytes)
        self.ledger.malloc(ptr, nbytes)
        return ptr

    def free(self, ptr):
        self.ledger.free(ptr)
        self._ctx.free(ptr)

    def __getattr__(self, name):
        attr = getattr(self._ctx, name)
        if not callable(attr):
            return attr

        def call(*args, **kwargs):
            from fusion_hip._lib import FZ_E_HIP, FusionHipError
            self.names.append(name)
            self.ledger.use(name, args)
            if len(self.names) == self.fail_at:
                raise FusionHipError(FZ_E_HIP, f"injected before {name}")
            return attr(*args, **kwargs)
        return call


def _host(x):
    """a result with its DeviceArrays downloaded, for comparing"""
    from fusion_hip.context import DeviceArray
    if isinstance(x, DeviceArray):
        return x.numpy()
    return [_host(y) for y in x] if isinstance(x, (tuple, list)) else x


def _same(a, b):
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b)
    return type(a) is type(b) and a == b


@pytest.fixture(scope="module")
def world():
    """-> (the recorded scheme, its recorder, host inputs, the device copies of them on the recorded context, the expected
    result of every case from an unwrapped scheme)"""
    import fusion.fusion as F
    from fusion_hip.context import DeviceArray
    from fusion_hip.scheme import BatchScheme
    params = F.fusion_setup(SECPAR, 7)
    ref = BatchScheme(params)
    sk, vk = ref.keygen_batch([11, 12, 13])
    sig = ref.sign_batch(sk, vk, MESSAGES)
    agg, aggs = ref.aggregate(vk, MESSAGES, sig), ref.aggregate_many(vk, MESSAGES, sig, SIZES)
    a = dict(vk=vk, sk=sk, sig=sig, agg=agg, aggs=aggs, recs=ref.encode("signature", sig)[0],
             aggrec=ref.encode("aggregate", agg)[0], aggrecs=ref.encode("aggregate", aggs)[0])
    assert ref.verify(vk, MESSAGES, agg) == (True, "") and not ref.verify_signatures(vk, MESSAGES, sig).any()
    want = {}
    for name, call in cases().items():
        if not name.endswith("[device]"):
            want[name] = _host(_call(ref, call, a))
    ref.close()
    bs = BatchScheme(params, private_context=True)
    bs._A_dev()
    real = bs.ctx
    rec = bs.ctx = Recorder(real)
    dev = {k: DeviceArray.from_numpy(rec, v) for k, v in a.items()}
    yield bs, rec, a, dev, want
    for x in dev.values():
        x.free()
    bs.ctx = real
    bs.close()


def _call(bs, call, a):
    params = bs.params                                   # one case lowers the capacity of the scheme it runs on
    try:
        return call(bs, a)
    finally:
        bs.params = params


def _recorded(bs, rec, call, a, fail_at=None):
    """-> (result with its device buffers downloaded or None, the ledger's complaints, the exception)"""
    from fusion_hip import FusionHipError
    before = set(rec.ledger.live)
    del rec.names[:], rec.ledger.errors[:]
    rec.fail_at = fail_at
    result = got = raised = None
    try:
        result = _call(bs, call, a)
        got = _host(result)
    except FusionHipError as e:
        raised = e
    finally:
        rec.fail_at = None
    return got, rec.ledger.settle(before, result), raised


@pytest.mark.parametrize("name", list(cases()))
def test_device_temporaries_balance_and_results_hold(world, monkeypatch, name):
    no_finalizers(monkeypatch)
    bs, rec, host, dev, want = world
    call, a = cases()[name], (dev if name.endswith("[device]") else host)
    expected = want[name[:-len("[device]")] if name.endswith("[device]") else name]
    got, wrong, raised = _recorded(bs, rec, call, a)
    assert raised is None and not wrong, (name, raised, wrong)
    assert _same(got, expected), name
    launches = [k for k, n in enumerate(rec.names, 1) if n.endswith("_dev")]
    assert launches, (name, rec.names)
    got, wrong, raised = _recorded(bs, rec, call, a, fail_at=launches[-1])
    assert got is None and raised is not None and "injected before" in str(raised), (name, raised)
    assert not wrong, (name, wrong)
    got, wrong, raised = _recorded(bs, rec, call, a)
    assert raised is None and not wrong and _same(got, expected), (name, raised, wrong)
