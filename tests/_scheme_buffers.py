"""What tests/test_scheme_buffers_host.py and tests/test_gpu_scheme_buffers.py share: a ledger of device allocations, a stand-in
context that keeps one without a device, and the table of BatchScheme / Context calls both tests walk.

The ledger's rule: when a call comes back -- with a result or with an exception -- every address it allocated has been freed
exactly once, except the buffers it returned; what the caller held before (its DeviceArrays, the scheme's resident public
challenge) is still allocated; and nothing was handed an address after its free.  DeviceBuffer.__del__ is switched off while a
test runs (no_finalizers), so a buffer left to the garbage collector shows up as a leak instead of being tidied away at a time
of the collector's choosing."""
import copy
import zlib

import numpy as np

SECPAR, N, SIZES = 128, 3, [1, 2]
MESSAGES = ["first", "second message", "3"]
HOST_FACE = ("keygen_core", "keygen_core_bcast", "sign_core", "sign_encoded", "aggregate_core", "verify_core")
_BASE, _STEP = 0x7F0000000000, 0x1000000                # the stand-in's addresses: no argument that is a count gets this large


class Ledger:
    def __init__(self):
        self.live, self.freed, self.errors, self.sizes = {}, set(), [], []

    def malloc(self, ptr, nbytes):
        if ptr in self.live:
            self.errors.append(f"malloc returned {ptr:#x}, which is still allocated")
        self.live[ptr] = nbytes
        self.freed.discard(ptr)                          # a real allocator hands freed addresses out again
        self.sizes.append(nbytes)

    def free(self, ptr):
        if ptr not in self.live:
            self.errors.append(f"free of {ptr:#x}, which is not allocated" + (" (freed before)" if ptr in self.freed else ""))
            return
        del self.live[ptr]
        self.freed.add(ptr)

    def use(self, name, args):
        for a in args:
            if isinstance(a, int) and not isinstance(a, bool) and a in self.freed:
                self.errors.append(f"{name} was given {a:#x} after its free")

    def settle(self, before, result):
        """-> what is wrong after a call that started with the addresses `before` allocated and returned `result` (None after an
        exception); the buffers it returned are freed here"""
        from fusion_hip.context import DeviceArray
        returned = [x for x in (result if isinstance(result, (tuple, list)) else [result]) if isinstance(x, DeviceArray)]
        out = list(self.errors)
        out += [f"the caller's {p:#x} was freed" for p in before if p not in self.live]
        out += [f"a returned buffer ({x.ptr:#x}) is not allocated" for x in returned if x.ptr not in self.live]
        left = set(self.live) - set(before) - {x.ptr for x in returned}
        out += [f"{len(left)} buffer(s) of {sorted(self.live[p] for p in left)} bytes left allocated"] if left else []
        for x in returned:
            x.free()
        return out


def no_finalizers(monkeypatch):
    from fusion_hip.context import DeviceBuffer
    monkeypatch.setattr(DeviceBuffer, "__del__", lambda self: None)


def _plain(a):
    """an argument as the record of the device work keeps it: pointers, which differ from run to run, by their kind alone"""
    if isinstance(a, (bool, str, type(None))):
        return a
    if isinstance(a, (int, np.integer)):
        return "ptr" if int(a) >= _BASE else int(a)
    if isinstance(a, np.ndarray):
        return (str(a.dtype), a.shape, zlib.crc32(np.ascontiguousarray(a).tobytes()))
    if isinstance(a, (bytes, bytearray)):
        return ("bytes", len(a), zlib.crc32(bytes(a)))
    if isinstance(a, (list, tuple)):
        return tuple(_plain(x) for x in a)
    return type(a).__name__


def stand_in_context(params):
    """A Context without a library or a device: malloc hands out distinct fake addresses, free / malloc keep the ledger, h2d does
    nothing, d2h zero-fills, every other device call is counted and returns what lets the caller go on (verdict 0, zero digests,
    the input of ntt_forward).  The six staged host-face methods are Context's own code.  arm(k, kind) makes interaction k
    (malloc included, free not: a failing free has no owner left to tidy up after it) raise; `unsupported` names the calls that
    answer FZ_E_UNSUPPORTED, which is no failure: the caller falls back to the host."""
    from fusion_hip._lib import FZ_E_HIP, FZ_E_UNSUPPORTED, FusionHipError
    from fusion_hip.context import Context

    class StandIn(Context):
        def __init__(self):
            self.modulus, self.degree = params.modulus, params.degree
            self.ledger, self.calls, self.names, self.fail_at, self.kind, self.unsupported = Ledger(), [], [], None, None, ()
            self._next = _BASE

        def close(self):
            pass

        def arm(self, k, kind):
            self.fail_at, self.kind = k, kind

        def _hit(self, name, args):
            self.names.append(name)
            self.ledger.use(name, args)
            if name != "malloc":
                self.calls.append((name,) + tuple(_plain(a) for a in args))
            if len(self.names) == self.fail_at:
                if self.kind == "memory":
                    raise MemoryError(f"injected at interaction {self.fail_at} ({name})")
                raise FusionHipError(FZ_E_HIP, f"injected at interaction {self.fail_at} ({name})")
            if name in self.unsupported:
                raise FusionHipError(FZ_E_UNSUPPORTED, f"{name}: not for this parameter set")

        def malloc(self, nbytes):
            self._hit("malloc", (nbytes,))
            self._next += _STEP
            self.ledger.malloc(self._next, nbytes)
            return self._next

        def free(self, ptr):
            self.ledger.free(ptr)

        def h2d(self, dptr, arr):
            self._hit("h2d", (dptr, np.ascontiguousarray(arr)))

        def d2h(self, arr, dptr):
            self._hit("d2h", (dptr, str(arr.dtype), arr.shape))
            arr[...] = 0
            return arr

        def ntt_forward(self, x):
            self._hit("ntt_forward", (np.asarray(x),))
            return np.ascontiguousarray(x, dtype=np.int32)

        def challenge_msgs_dev(self, P, d_vk, blob, offsets, n, d_out, want_prehash=False):
            self._hit("challenge_msgs_dev", (d_vk, blob, np.asarray(offsets), n, d_out, want_prehash))
            return np.zeros((n, 32), dtype=np.uint8) if want_prehash else None

    def counted(name):
        def call(self, *args, **kwargs):
            self._hit(name, args + tuple(kwargs.values()))
            return 0 if name.startswith("verify_") else None
        return call
    for name in dir(Context):
        if not name.startswith("_") and name not in HOST_FACE and name not in StandIn.__dict__ and callable(getattr(Context, name)):
            setattr(StandIn, name, counted(name))
    return StandIn()


def scheme_on(ctx, params):
    """a BatchScheme on `ctx` without BatchScheme.__init__ (which opens a device), its public challenge already resident"""
    from fusion_hip import hostpipe
    from fusion_hip.scheme import BatchScheme
    bs = BatchScheme.__new__(BatchScheme)
    bs.params, bs.P, bs.ctx = params, hostpipe.scheme_params(params), ctx
    bs.d, bs.l, bs.q = params.degree, params.num_rows_sk, params.modulus
    bs.threads, bs._pool, bs._private = 2, None, False
    bs.device_hash = bs.device_sampler = True
    bs.A, bs._dA = np.zeros((bs.l, bs.d), dtype=np.int32), None
    bs._A_dev()
    return bs


def host_inputs(params, rng=None):
    """the arguments of every case as host arrays; values do not matter to the ledger (the GPU test replaces them by real keys,
    signatures and records)"""
    from fusion_hip.scheme import encoded_size
    rng = rng or np.random.default_rng(SECPAR)
    d, l, g = params.degree, params.num_rows_sk, len(SIZES)
    small = lambda *shape: rng.integers(-3, 4, size=shape).astype(np.int32)      # noqa: E731
    return dict(vk=small(N, 2, d), sk=small(N, 2, l, d), sig=small(N, l, d), agg=small(l, d), aggs=small(g, l, d),
                recs=np.zeros((N, encoded_size(params, "signature")), dtype=np.uint8),
                aggrec=np.zeros((1, encoded_size(params, "aggregate")), dtype=np.uint8),
                aggrecs=np.zeros((g, encoded_size(params, "aggregate")), dtype=np.uint8))


def cases():
    """name -> call(bs, a): every public BatchScheme method that allocates device memory, in each output mode and -- the name
    ends in [device] -- with DeviceArray arguments, where `a` maps the names of host_inputs to them"""
    out = {}
    for device in (False, True):
        for keep in (False, True):
            tag = f"[device={device},keep_vk={keep}]"
            out["keygen_batch" + tag] = lambda bs, a, dv=device, k=keep: bs.keygen_batch([5, 6, 7], device=dv, keep_vk=k)
            out["keygen_batch(negative seed)" + tag] = lambda bs, a, dv=device, k=keep: bs.keygen_batch([-5, 6, 7], device=dv, keep_vk=k)
        out[f"sign_batch[device={device}]"] = lambda bs, a, dv=device: bs.sign_batch(a["sk"], a["vk"], MESSAGES, device=dv)
        out[f"sign_batch_encoded[device={device}]"] = lambda bs, a, dv=device: bs.sign_batch_encoded(a["sk"], a["vk"], MESSAGES, device=dv)
        out[f"decode[device={device}]"] = lambda bs, a, dv=device: bs.decode("signature", a["recs"], device=dv)
    out.update({
        "challenges": lambda bs, a: bs.challenges(a["vk"], MESSAGES),
        "aggregate": lambda bs, a: bs.aggregate(a["vk"], MESSAGES, a["sig"]),
        "verify": lambda bs, a: bs.verify(a["vk"], MESSAGES, a["agg"]),
        "verify_signatures": lambda bs, a: bs.verify_signatures(a["vk"], MESSAGES, a["sig"]),
        "aggregate_screened": lambda bs, a: bs.aggregate_screened(a["vk"], MESSAGES, a["sig"]),
        "encode": lambda bs, a: bs.encode("signature", a["sig"]),
        "aggregate_encoded": lambda bs, a: bs.aggregate_encoded(a["vk"], MESSAGES, a["recs"]),
        "verify_signatures_encoded": lambda bs, a: bs.verify_signatures_encoded(a["vk"], MESSAGES, a["recs"]),
        "aggregate_encoded_screened": lambda bs, a: bs.aggregate_encoded_screened(a["vk"], MESSAGES, a["recs"]),
        "verify_encoded": lambda bs, a: bs.verify_encoded(a["vk"], MESSAGES, a["aggrec"]),
        "aggregate_many": lambda bs, a: bs.aggregate_many(a["vk"], MESSAGES, a["sig"], SIZES),
        "verify_many": lambda bs, a: bs.verify_many(a["vk"], MESSAGES, a["aggs"], SIZES),
        "verify_many(one group over capacity)": lambda bs, a: _capacity_one(bs).verify_many(a["vk"], MESSAGES, a["aggs"], SIZES),
        "verify_many_encoded": lambda bs, a: bs.verify_many_encoded(a["vk"], MESSAGES, a["aggrecs"], SIZES),
    })
    for screened in (False, True):
        for encoded in (False, True):
            out[f"aggregate_many_encoded[screened={screened},encoded={encoded}]"] = lambda bs, a, s=screened, e=encoded: \
                bs.aggregate_many_encoded(a["vk"], MESSAGES, a["recs"], SIZES, screened=s, encoded=e)
    plain = [k for k in out if "[" not in k or k.startswith("aggregate_many_encoded")]
    for k in plain + ["sign_batch[device=False]", "sign_batch_encoded[device=False]", "decode[device=False]"]:
        out[k + "[device]"] = out[k]
    return out


def _capacity_one(bs):
    """the same scheme with room for one signer per aggregate: of the groups [1, 2] the second is over capacity"""
    bs.params = copy.copy(bs.params)
    bs.params.capacity = 1
    return bs


def context_cases(params):
    """name -> call(ctx): the six staged host-face methods of Context"""
    rng = np.random.default_rng(1)
    d, l = params.degree, 2
    r = lambda *shape: rng.integers(-3, 4, size=shape).astype(np.int32)          # noqa: E731
    A, sk, c, sig, vk, coef, polys = r(l, d), r(N, 2, l, d), r(N, d), r(N, l, d), r(N, 2, d), r(N, 2, l, d), r(N, 2, d)
    return {
        "Context.keygen_core": lambda ctx: ctx.keygen_core(A, coef),
        "Context.keygen_core_bcast": lambda ctx: ctx.keygen_core_bcast(A, polys),
        "Context.sign_core": lambda ctx: ctx.sign_core(sk, c),
        "Context.sign_encoded": lambda ctx: ctx.sign_encoded(sk, c, 4264),
        "Context.aggregate_core": lambda ctx: ctx.aggregate_core(sig, c),
        "Context.verify_core": lambda ctx: ctx.verify_core(A, sig[0, :l], vk[:, 0], vk[:, 1], c, c, 1000, d),
    }
