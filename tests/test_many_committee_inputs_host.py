"""The many-committee calls of BatchScheme (aggregate_many, verify_many, aggregate_many_encoded, aggregate_verify_many_encoded,
verify_many_encoded, hash_ag_many_dev) hold their inputs in one type (fusion_hip.scheme._Committees), checked without a GPU on the
stand-in context of tests/_scheme_buffers.py.

* tests/golden/many_committee_calls.json holds, for the cells that tests/golden/vk_order_host_calls.json does not cover, every
  device call with its arguments (ctx.calls) and every interaction, allocations included (ctx.names), as the code made them BEFORE
  the type existed: the device form with the device sort, both fall-backs on a first and a second call of one object, the valid
  mask of hash_ag_many_dev, the bytes-out forms.  Every cell must reproduce both lists exactly.  record() below wrote the file; it
  is run by hand, and only when the calls are meant to change.
* _hash_ag_form decides once per call, and not at all where a call returns before it touches a device.
* Every interaction of every call in turn is made to raise (tests/test_scheme_buffers_host.py's sweep): nothing stays allocated.
* The key_sort comparison is written in one function."""
import ast
import inspect
import json
import os

import pytest

import test_scheme_buffers_host as sweep
from _scheme_buffers import MESSAGES, SIZES, host_inputs, no_finalizers, scheme_on, stand_in_context
from test_vk_order_host import MANY

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "many_committee_calls.json")
UNSUPPORTED = {"hash_ag": ("hash_ag_ragged_dev", "hash_ag_ragged_sorted_dev"), "challenge": ("challenge_msgs_dev", "challenge_msgs_keep_dev")}
MASK = [True, False, True]
EXTRA = {
    "hash_ag_many_dev[valid]": lambda bs, a, M, S: bs.hash_ag_many_dev(a["vk"], M, S, valid=MASK),
    "aggregate_many_encoded[encoded]": lambda bs, a, M, S: bs.aggregate_many_encoded(a["vk"], M, a["recs"], S, encoded=True),
    "aggregate_verify_many_encoded[encoded]": lambda bs, a, M, S: bs.aggregate_verify_many_encoded(a["vk"], M, a["recs"], S, encoded=True),
}


@pytest.fixture(scope="module")
def params():
    import fusion.fusion as F
    return F.fusion_setup(128, 1)


@pytest.fixture(autouse=True)
def _leaks_stay_visible(monkeypatch):
    no_finalizers(monkeypatch)


def cells():
    """-> [(id, call, key_sort, keys, the calls that answer FZ_E_UNSUPPORTED, how many calls on the one object)], all under
    hash_ag="device\""""
    out = []
    for keys in ("host", "device"):
        for name in sorted(MANY):
            out.append((f"{name}|key_sort=device|keys={keys}", MANY[name], "device", keys, (), 1))
        for key_sort in ("host", "device"):
            for what in sorted(UNSUPPORTED):
                for name in sorted(MANY):
                    out.append((f"{name}|key_sort={key_sort}|keys={keys}|unsupported={what}", MANY[name], key_sort, keys, UNSUPPORTED[what], 2))
            out.append((f"hash_ag_many_dev[valid]|key_sort={key_sort}|keys={keys}", EXTRA["hash_ag_many_dev[valid]"], key_sort, keys, (), 1))
        for name in ("aggregate_many_encoded[encoded]", "aggregate_verify_many_encoded[encoded]"):
            out.append((f"{name}|key_sort=device|keys={keys}", EXTRA[name], "device", keys, (), 1))
    return out


def run_cell(params, call, key_sort, keys, unsupported, times, wrap=None):
    """the cell on a fresh stand-in -> one {"calls", "names"} per call on the one object, with "error" where the call raised"""
    from fusion_hip._lib import FusionHipError
    from fusion_hip.context import DeviceArray
    ctx = stand_in_context(params)
    bs, a = scheme_on(ctx, params), host_inputs(params)
    bs.hash_ag, bs.key_sort = "device", key_sort
    if wrap is not None:
        wrap(bs)
    if keys == "device":
        a["vk"] = DeviceArray.from_numpy(ctx, a["vk"])
    ctx.unsupported = unsupported
    before, out = dict(ctx.ledger.live), []
    for _ in range(times):
        del ctx.calls[:], ctx.names[:]
        result = error = None
        try:
            result = call(bs, a, MESSAGES, SIZES)
        except FusionHipError as e:
            error = str(e)
        assert ctx.ledger.settle(before, result) == []
        out.append(dict(calls=json.loads(json.dumps(ctx.calls)), names=list(ctx.names), **({} if error is None else {"error": error})))
    return out


def record():
    """writes tests/golden/many_committee_calls.json from the code as it stands.  Not a test and not run by one: call it by hand
    (python -c "import test_many_committee_inputs_host as t; t.record()" with tests/ on the path) when the device work of the
    many-committee calls is changed on purpose, and say so where the change is described."""
    import fusion.fusion as F
    from fusion_hip.context import DeviceBuffer
    DeviceBuffer.__del__ = lambda self: None
    params = F.fusion_setup(128, 1)
    golden = {cell[0]: run_cell(params, *cell[1:]) for cell in cells()}
    with open(GOLDEN, "w") as fh:
        json.dump(golden, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    return golden


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_the_cells(golden):
    assert sorted(golden) == sorted(c[0] for c in cells())
    refused = [k for k, v in golden.items() if any("error" in r for r in v)]
    assert sorted(refused) == sorted(f"hash_ag_many_dev|key_sort={s}|keys={k}|unsupported=hash_ag" for s in ("host", "device") for k in ("host", "device"))


@pytest.mark.parametrize("cell", cells(), ids=lambda c: c[0])
def test_cell_makes_the_recorded_calls_and_decides_its_form_once(params, golden, cell):
    count = []

    def wrap(bs):
        form = bs._hash_ag_form
        bs._hash_ag_form = lambda sizes: (count.append(1), form(sizes))[1]
    got = run_cell(params, *cell[1:], wrap=wrap)
    want = golden[cell[0]]
    assert len(got) == len(want) == cell[5]
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["names"] == w["names"], (cell[0], k)
        assert g["calls"] == w["calls"], (cell[0], k)
        assert g.get("error") == w.get("error"), (cell[0], k)
    assert len(count) == cell[5], f"_hash_ag_form ran {len(count)} times in {cell[5]} call(s)"


def test_form_is_not_decided_where_no_device_is_touched(params):
    import numpy as np
    from fusion_hip._lib import FusionHipError
    ctx = stand_in_context(params)
    bs, a = scheme_on(ctx, params), host_inputs(params)
    bs.hash_ag = bs.key_sort = "device"
    bs._hash_ag_form = lambda sizes: pytest.fail("_hash_ag_form ran")
    del ctx.names[:]
    none, empty = a["vk"][:0], np.zeros(0, dtype=np.uint8)
    for encoded in (False, True):
        assert bs.aggregate_many_encoded(none, [], empty, [], encoded=encoded)[1].shape == (0,)
        assert bs.aggregate_verify_many_encoded(none, [], empty, [], encoded=encoded)[-1] == []
    assert bs.verify_many_encoded(none, [], empty, []) == []
    for name in sorted(MANY):
        for sizes in ([1, 1], [3, 0], [1, 2, 1]):                       # not the keys' number, an empty committee, not the messages'
            with pytest.raises(FusionHipError):
                MANY[name](bs, a, MESSAGES + ["4"] * (sum(sizes) - 3), sizes)
    with pytest.raises(FusionHipError):
        bs.aggregate_many_encoded(a["vk"], MESSAGES, a["recs"][:2], SIZES)
    with pytest.raises(FusionHipError):
        bs.verify_many_encoded(a["vk"], MESSAGES, a["aggrecs"][:1], SIZES)
    assert ctx.names == []


@pytest.mark.parametrize("inputs", ["", "[device]"])
@pytest.mark.parametrize("key_sort", ["host", "device"])
@pytest.mark.parametrize("name", sorted(MANY))
def test_every_temporary_is_freed_once_whatever_raises(params, name, key_sort, inputs, monkeypatch):
    """the sweep of tests/test_scheme_buffers_host.py, its own helper on the seven calls: "error" at every interaction and "memory"
    besides at every allocation, under hash_ag="device" with either sort, the arguments host arrays or ([device]) DeviceArrays"""
    from fusion_hip.scheme import BatchScheme
    monkeypatch.setattr(BatchScheme, "hash_ag", "device")               # (scheme_on makes its object without __init__)
    monkeypatch.setattr(BatchScheme, "key_sort", key_sort)
    call, name = MANY[name], name + inputs
    monkeypatch.setattr(sweep, "cases", lambda: {name: lambda bs, a: call(bs, a, MESSAGES, SIZES)})
    clean, wrong, raised = sweep._run(params, name)
    assert raised is None and not wrong, (name, raised, wrong)
    entry = "hash_ag_ragged_sorted_dev" if key_sort == "device" else "hash_ag_ragged_dev"
    assert entry in clean.names and len(clean.names) >= 2, clean.names
    for k, interaction in enumerate(clean.names, 1):
        for kind in ("error", "memory") if interaction == "malloc" else ("error",):
            _, wrong, raised = sweep._run(params, name, k, kind)
            what = (name, key_sort, k, interaction, kind, raised, wrong)
            assert raised is not None and f"injected at interaction {k} " in str(raised), what
            assert isinstance(raised, MemoryError) == (kind == "memory"), what
            assert not wrong, what


def test_key_sort_is_compared_in_one_function():
    """where the sort runs is ONE predicate of the call's inputs; only the constructor's validation names the option besides"""
    from fusion_hip import scheme
    where = set()
    for fn in ast.walk(ast.parse(inspect.getsource(scheme))):
        if isinstance(fn, (ast.FunctionDef, ast.Lambda)):
            for node in ast.walk(fn):
                if isinstance(node, ast.Compare) and isinstance(node.ops[0], (ast.Eq, ast.NotEq)) and \
                        "key_sort" in ast.dump(node) and "'device'" in ast.dump(node):
                    where.add((getattr(fn, "name", "lambda"), fn.lineno))
    assert len(where) == 1, sorted(where)
