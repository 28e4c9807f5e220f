"""ISA-level checks of the 16-per-lane transform loops (CPU only: hipcc cross-compiles gfx950 without a GPU).

The loops of ntt_fwd16 / ntt_inv16 / ntt_jobs16 / ntt_jobs16_keep take a wave's next chunk straight into LDS (chunk_load_lds,
fz_ntt_dev.h): the chunk holds no register while in flight and is not written to LDS by the wave.  What that buys rests on the
generated code, pinned here: the register count the freed sixteen leave, no scratch, the workgroup's LDS unchanged, the direct
load inside every transform loop and no 16-byte LDS write between a loop's header and its first conversion (the staging copy the
register path needed)."""
import re

import pytest

from _isa import asm, family, metadata

FAMILIES = ("ntt_fwd16", "ntt_inv16", "ntt_jobs16", "ntt_jobs16_keep")
MAX_VGPRS = 108                                     # 121 before, minus the chunk's sixteen, with slack


def lds16_bytes(logd):
    """lds16_doubles<LOGD>() * 8: a transpose region per wave + the per-lane twiddle table"""
    d = 1 << logd
    lanes, sb = d // 16, logd - 4
    ne = 16 - (16 >> sb)
    return 8 * (4 * (64 // lanes) * (d + 2 * (d // 16)) + 2 * ne * lanes)


def degree_log(name):
    return int(re.search(r"ILi(\d)E", name).group(1))


def checked(name):
    f = family(name)
    return f in FAMILIES and (degree_log(name) == 8 or (degree_log(name) == 6 and f in ("ntt_fwd16", "ntt_inv16")))


def loops(text, name):
    """[instructions] of every loop of the kernel: from a block label to the last backward branch to it (the kernel's text ends at
    its .Lfunc_end label: an early return is an s_endpgm in the middle)"""
    body = re.search(r"^" + re.escape(name) + r":.*?$(.*?)^\.Lfunc_end", text, re.S | re.M).group(1).splitlines()
    labels = {m.group(1): i for i, ln in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    spans = {}
    for i, ln in enumerate(body):
        m = re.match(r"\s+s_c?branch\S*\s+(\.LBB\d+_\d+)", ln)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            spans[m.group(1)] = i
    return [[ln.strip() for ln in body[labels[lb]:end + 1] if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
            for lb, end in spans.items()]


@pytest.fixture(scope="module")
def text():
    return asm("fz_transforms")


@pytest.fixture(scope="module")
def kernels(text):
    names = [n for n in metadata(text) if checked(n)]
    # degree 256: 2 + 2 one-job kernels, 6 + 12 multi-job ones; degree 64: 2 + 2
    assert len(names) == 26, sorted(names)
    return names


def test_registers_scratch_and_lds(text, kernels):
    meta = metadata(text)
    for name in kernels:
        f = meta[name]
        assert f["vgpr_count"] <= MAX_VGPRS, (name, f)
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0, (name, f)
        assert f["lds"] == lds16_bytes(degree_log(name)), (name, f)


def test_every_transform_loop_lands_its_next_chunk_in_lds(text, kernels):
    for name in kernels:
        # the loops of ONE iteration's body: sixteen conversions (a backward branch that spans several bodies is layout, not a loop)
        transform = [ins for ins in loops(text, name) if sum(s.startswith("v_cvt_f64_i32") for s in ins) == 16]
        assert len(transform) == (1 if family(name) in ("ntt_fwd16", "ntt_inv16") else 2), (name, len(transform))
        for ins in transform:
            assert sum(s.startswith("global_load_lds_dwordx4") for s in ins) == 4, name
            # the chunk reaches the lanes' registers without a staging copy by the wave
            first = next(i for i, s in enumerate(ins) if s.startswith("v_cvt_f64_i32"))
            assert not any(s.startswith("ds_write_b128") for s in ins[:first]), (name, ins[:first])
            # ... and no register load of a chunk is left in the loop
            assert not any(s.startswith("global_load_dwordx4") for s in ins), name
            # the wait for it leaves the iteration's four stores outstanding
            stores = [i for i, s in enumerate(ins) if s.startswith("global_store_dwordx4")]
            assert len(stores) == 4 and stores[-1] > max(i for i, s in enumerate(ins) if s.startswith("global_load_lds")), name
            assert ins[stores[-1] + 1].startswith("s_waitcnt vmcnt(4)"), (name, ins[stores[-1]:stores[-1] + 3])
            assert not any(re.match(r"s_waitcnt vmcnt\([0-3]\)", s) for s in ins), name
