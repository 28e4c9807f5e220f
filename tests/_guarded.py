"""A guarded arena for the entries that read and write int32 / int64 rows: every operand of a call lives inside one allocation
laid out as [lead guard | interior | trail guard], and after the call every word is accounted for.

- Each guard is GUARD_BYTES = 16 KiB: twice the largest tile any of these kernels owns (1024 coefficients of int64, 8 KiB), so a
  lane that stores one tile past either end still lands in the guard, never outside the allocation.
- The interior begins 16-byte aligned, or at 16 k + 4 bytes with `offset=4` (int32 operands only): the launchers then take their
  scalar routes.
- The interior may be rows of `row` elements `stride` apart (stride > row); the words between two rows belong to the guard.
- A case runs once per fill (FILLS: 0x5a5a5a5a and 0x80000000, as 64-bit patterns in int64 operands).  The fill goes into the
  guards of every operand and into the previous contents of the outputs.  After each run: (1) every output interior equals its
  expectation bit for bit, (2) every guard word of every operand still holds the fill, (3) every input interior equals what was
  uploaded; and after both: (4) both runs left the same outputs -- a read past an input's end, or a dependence on what the output
  held before, shows there (an operand that is read AND written, `inout`, carries its previous contents as data instead).

The checks (`Arena`, `check_run`, `check_same`) work on flat numpy images; the transport is a backend: `DeviceBackend` (DeviceBuffer /
ctx.h2d) or `HostBackend` (plain numpy arrays, the operand handed to a fake entry as a view), so tests/test_guarded_host.py shows
without a GPU that each kind of fault is reported with the operand's name and the index."""
import numpy as np

GUARD_BYTES = 16384
FILLS = (0x5a5a5a5a, 0x80000000)


class GuardError(AssertionError):
    pass


def fill_value(dtype, fill):
    """the fill as one element of dtype: the 32-bit pattern, twice over in a 64-bit element"""
    dtype = np.dtype(dtype)
    word = np.array([fill], dtype=np.uint32)
    if dtype.itemsize == 8:
        word = np.array([(fill << 32) | fill], dtype=np.uint64)
    return word.view(dtype)[0]


class Operand:
    """what a test says about one operand: `role` in | out | inout, rows x row elements `stride` apart, the data of an input (or
    an inout's previous contents), the expected contents of an output, offset = 0 | 4 bytes past 16-byte alignment"""

    def __init__(self, name, role, rows=None, row=None, dtype=np.int32, stride=None, data=None, expect=None, offset=0, canon=None):
        assert role in ("in", "out", "inout")
        self.name, self.role, self.dtype, self.offset = name, role, np.dtype(dtype), offset
        # canon: the int64 partial sums are specified modulo q only ("the same sum WITHOUT the final reduction"): their interiors
        # are compared after canon (the centred residue), with the expectation and between the fills
        self.canon = canon
        ref = data if data is not None else expect
        if rows is None:
            ref = np.asarray(ref)
            rows, row = (1, ref.size) if ref.ndim < 2 else (int(np.prod(ref.shape[:-1])), ref.shape[-1])
        self.rows, self.row = int(rows), int(row)
        self.stride = self.row if stride is None else int(stride)
        assert self.stride >= self.row and offset in (0, 4) and (offset == 0 or self.dtype.itemsize == 4)
        self.data = None if data is None else np.ascontiguousarray(data, dtype=self.dtype).reshape(self.rows, self.row)
        self.expect = None if expect is None else np.ascontiguousarray(expect, dtype=self.dtype).reshape(self.rows, self.row)
        assert (self.data is not None) == (role != "out") and (self.expect is not None) == (role != "in")


def inp(name, data, **kw):
    return Operand(name, "in", data=data, dtype=np.asarray(data).dtype, **kw)


def out(name, expect, **kw):
    expect = np.asarray(expect)
    return Operand(name, "out", expect=expect, dtype=kw.pop("dtype", expect.dtype), **kw)


def inout(name, data, expect, **kw):
    return Operand(name, "inout", data=data, expect=expect, dtype=np.asarray(data).dtype, **kw)


class Arena:
    """the flat image of one operand's allocation: where the interior lies, how to name any index of it"""

    def __init__(self, op):
        self.op = op
        size = op.dtype.itemsize
        self.lead = (GUARD_BYTES + op.offset) // size                   # first interior element
        self.span = (op.rows - 1) * op.stride + op.row if op.rows else 0
        self.total = self.lead + self.span + GUARD_BYTES // size
        self.byte_offset = GUARD_BYTES + op.offset
        idx = np.arange(self.span)
        self.interior = np.zeros(self.total, dtype=bool)
        self.interior[self.lead:self.lead + self.span] = (idx % op.stride) < op.row if op.rows else False

    def image(self, fill, with_data=True):
        a = np.full(self.total, fill_value(self.op.dtype, fill), dtype=self.op.dtype)
        if with_data and self.op.data is not None:
            a[self.interior] = self.op.data.reshape(-1)
        return a

    def where(self, flat):
        """a flat index of the allocation, in the operand's own terms"""
        flat = int(flat)
        rel = flat - self.lead
        if rel < 0:
            return f"lead guard, {-rel} element(s) before the interior (index {rel})"
        if rel >= self.span:
            return f"trail guard, {rel - self.span} element(s) after the interior (index {rel})"
        r, c = divmod(rel, self.op.stride)
        if c >= self.op.row:
            return f"stride gap after row {r}, gap word {c - self.op.row} (index {rel})"
        return f"row {r}, column {c} (index {rel})"


def _first(mask):
    return int(np.flatnonzero(mask)[0])


def _hex(v):
    return hex(int(np.array([v]).view(np.uint64 if np.asarray(v).dtype.itemsize == 8 else np.uint32)[0]))


def check_run(arenas, before, after, fill):
    """checks 1-3 of one run -> list of messages; before / after: name -> flat image"""
    bad = []
    for name, ar in arenas.items():
        op, b, a = ar.op, before[name], after[name]
        guard = ~ar.interior
        hit = guard & (a != b)
        if hit.any():
            i = _first(hit)
            bad.append(f"{name}: guard word written: {ar.where(i)}: {_hex(a[i])}, fill {_hex(b[i])}; {int(hit.sum())} guard word(s) in all")
        if op.role == "in":
            hit = ar.interior & (a != b)
            if hit.any():
                i = _first(hit)
                bad.append(f"{name}: input changed: {ar.where(i)}: {_hex(a[i])}, uploaded {_hex(b[i])}; {int(hit.sum())} word(s) in all")
        else:
            want = b.copy()
            want[ar.interior] = op.expect.reshape(-1)
            if op.canon is not None:
                a = a.copy()
                a[ar.interior] = op.canon(a[ar.interior])
            hit = ar.interior & (a != want)
            if hit.any():
                i = _first(hit)
                stale = " (still the previous contents)" if a[i] == b[i] else ""
                bad.append(f"{name}: output differs from the expectation: {ar.where(i)}: got {int(a[i])}{stale}, expected {int(want[i])}; "
                           f"{int(hit.sum())} word(s) in all")
    return [f"[fill {fill:#x}] {m}" for m in bad]


def check_same(arenas, afters):
    """check 4: the output interiors of the runs agree -> list of messages"""
    bad = []
    for name, ar in arenas.items():
        if ar.op.role == "in":
            continue
        x, y = afters[0][name], afters[1][name]
        if ar.op.canon is not None:
            x, y = x.copy(), y.copy()
            x[ar.interior], y[ar.interior] = ar.op.canon(x[ar.interior]), ar.op.canon(y[ar.interior])
        hit = ar.interior & (x != y)
        if hit.any():
            i = _first(hit)
            bad.append(f"{name}: output depends on the fill: {ar.where(i)}: {int(x[i])} under {FILLS[0]:#x}, {int(y[i])} under {FILLS[1]:#x}")
    return bad


class Placed:
    """one operand in place for a call: .ptr is what the entry takes (a device address, or a numpy view from the interior's first
    element to the end of the allocation on the host backend), .handle the backend's allocation"""

    def __init__(self, op, ptr, handle):
        self.op, self.ptr, self.handle = op, ptr, handle


class HostBackend:
    def alloc(self, arena, image):
        a = image.copy()
        return Placed(arena.op, a[arena.lead:], a)

    def read(self, arena, placed):
        return placed.handle.copy()

    def free(self, placed):
        pass


class DeviceBackend:
    def __init__(self, ctx):
        self.ctx = ctx

    def alloc(self, arena, image):
        import fusion_hip
        buf = fusion_hip.DeviceBuffer.from_numpy(self.ctx, image)
        assert buf.ptr % 256 == 0, "allocations are expected 256-byte aligned"
        return Placed(arena.op, buf.ptr + arena.byte_offset, buf)

    def read(self, arena, placed):
        self.ctx.synchronize()
        return placed.handle.to_numpy(arena.op.dtype, (arena.total,))

    def free(self, placed):
        placed.handle.free()


def run_case(backend, operands, call, fills=FILLS):
    """call(p) with p[name] = Placed once per fill -> the list of call's return values (the caller compares them with what it
    expects); raises GuardError with every finding of checks 1-4"""
    arenas = {op.name: Arena(op) for op in operands}
    assert len(arenas) == len(operands), "operand names must differ"
    bad, afters, rets = [], [], []
    for fill in fills:
        before = {n: ar.image(fill) for n, ar in arenas.items()}
        placed = {}
        try:
            for n, ar in arenas.items():
                placed[n] = backend.alloc(ar, before[n])
            rets.append(call(placed))
            after = {n: backend.read(ar, placed[n]) for n, ar in arenas.items()}
        finally:
            for p in placed.values():
                backend.free(p)
        bad += check_run(arenas, before, after, fill)
        afters.append(after)
    if len(afters) == 2:
        bad += check_same(arenas, afters)
    if bad:
        raise GuardError("\n".join(bad))
    return rets


def run_refusal(backend, operands, call, code, fill=FILLS[0]):
    """a call the entry must refuse with `code`: every arena, interiors included, is all fill before and must be after"""
    arenas = {op.name: Arena(op) for op in operands}
    before = {n: ar.image(fill, with_data=False) for n, ar in arenas.items()}
    placed, got = {}, None
    try:
        for n, ar in arenas.items():
            placed[n] = backend.alloc(ar, before[n])
        try:
            call(placed)
        except Exception as e:                                          # FusionHipError carries .code
            got = getattr(e, "code", e)
        after = {n: backend.read(ar, placed[n]) for n, ar in arenas.items()}
    finally:
        for p in placed.values():
            backend.free(p)
    assert got == code, f"expected refusal code {code}, got {got!r}"
    bad = []
    for n, ar in arenas.items():
        hit = after[n] != before[n]
        if hit.any():
            i = _first(hit)
            bad.append(f"{n}: written by a refused call: {ar.where(i)}: {_hex(after[n][i])}")
    if bad:
        raise GuardError("\n".join(bad))


def any_int32(rng, shape):
    """the full int32 range with -2^31, 2^31 - 1, 0 and +-1 planted (first and last elements and ~5 % of the rest)"""
    x = rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64)
    edge = np.array([-2 ** 31, 2 ** 31 - 1, 0, -1, 1], dtype=np.int64)
    f = x.reshape(-1)
    hit = rng.random(f.size) < 0.05
    f[hit] = edge[rng.integers(0, 5, size=int(hit.sum()))]
    f[0] = -2 ** 31
    f[-1] = 2 ** 31 - 1 if f.size > 1 else f[-1]
    return x.astype(np.int32)


# ---- what the GPU files share: contexts per (ring, knobs), rings, the device's size ----------------------------------------------
def root_pair(q, d):
    """(root, inverse) of order 2 d mod q"""
    for g in range(2, 5000):
        r = pow(g, (q - 1) // (2 * d), q)
        if pow(r, d, q) == q - 1:
            return r, pow(r, q - 2, q)
    raise AssertionError(f"no root of order {2 * d} mod {q}")


def scheme_ring(d):
    """(q, d, root, inverse root) of the scheme's parameter set of degree 64 or 256"""
    from oracle import oracle as O
    P = O.PARAMS[{64: 128, 256: 256}[d]]
    return P["q"], d, P["root"], P["inv_root"]


def num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


class Contexts:
    """one context per (ring, knobs), created with the knobs in the environment (they are read at creation) and closed together"""

    def __init__(self):
        self._made = {}

    def get(self, ring, env=None):
        import os

        import fusion_hip
        env = dict(env or {})
        key = (tuple(ring), tuple(sorted(env.items())))
        if key not in self._made:
            for k, v in env.items():
                os.environ[k] = v
            try:
                self._made[key] = fusion_hip.Context(*ring)
            finally:
                for k in env:
                    os.environ.pop(k, None)
        return self._made[key]

    def close(self):
        for c in self._made.values():
            c.close()
        self._made = {}


def on_device(ctx, operands, call):
    return run_case(DeviceBackend(ctx), operands, call)


def refused(ctx, operands, call, code):
    return run_refusal(DeviceBackend(ctx), operands, call, code)


def cent_mod(q):
    """canon= of an int64 partial sum: its centred residue"""
    def canon(a):
        r = np.asarray(a, dtype=np.int64) % q
        return np.where(r > q // 2, r - q, r)
    return canon
