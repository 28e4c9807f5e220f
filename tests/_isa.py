"""gfx950 assembly of the library's translation units for the CPU-side ISA checks (hipcc cross-compiles without a GPU): one
compile per unit and session, with the build's code-generation flags, and the parsers the checks share."""
import functools
import os
import re
import subprocess
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from isa_diff import family, metadata  # noqa: E402,F401  (the metadata parser and the family name: one copy, the tool's)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fusion-cryptography_amd", "csrc")
# the units the transform kernels and what is built on them are compiled in: 232 kernels (test_isa_checks.py pins them per family)
TRANSFORM_UNITS = ("fz_transforms", "fz_records")
# the units of the streaming kernels: 37 kernels (test_isa_checks.py pins them per family, aggregation's in its own unit)
STREAM_UNITS = ("fz_pointwise", "fz_aggregate")


@functools.lru_cache(maxsize=None)
def asm(unit):
    """the device assembly of csrc/<unit>.hip as text"""
    import __graft_entry__ as G
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    flags = [f for f in G.HIPCC_FLAGS if f.startswith(("--offload-arch", "-O", "-std", "-ff"))]      # what decides the code, not the linking
    with tempfile.TemporaryDirectory(prefix="isa_") as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.check_call([hipcc] + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, unit + ".hip"), "-o", out],
                              stderr=subprocess.DEVNULL)
        with open(out) as fh:
            return fh.read()


def assert_fits_transforms(kernels, logd_re, lds_of):
    """what every unit built on the transforms' LDS is held to, for `kernels` = {mangled name: metadata}: no spill, no scratch,
    and for a kernel whose name gives its degree (group 1 of `logd_re`) no more LDS than the largest kernel of
    fz_transforms matching `lds_of` at that degree"""
    lds = {k: v["lds"] for k, v in metadata(asm("fz_transforms"), lds_of).items()}
    for name, f in kernels.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        logd = re.search(logd_re, name)
        if logd:
            same = [v for k, v in lds.items() if f"16ILi{logd.group(1)}E" in k]
            assert same and f["lds"] <= max(same), (name, f["lds"], same)


def bodies(text, needle):
    """{mangled name: [instructions]} of every kernel whose name contains `needle`"""
    out = {}
    for m in re.finditer(r"^(_ZN\S*" + needle + r"\S*):\s*;.*?$(.*?)s_endpgm", text, re.S | re.M):
        ins = [ln.strip() for ln in m.group(2).splitlines() if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
        out[m.group(1)] = ins
    return out
