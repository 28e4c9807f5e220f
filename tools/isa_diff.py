#!/usr/bin/env python3
"""Compare two builds' gfx950 assembly kernel by kernel: is the generated code of a kernel the same in both?

    python tools/isa_diff.py --a old/fz_ntt.s --b new/fz_transforms.s new/fz_records.s

Each side is a set of `.s` files (hipcc -S --cuda-device-only with the build's flags); a kernel is looked up by its mangled name
in whichever file of a side holds it.  Compared per kernel: the instruction list (block labels `.LBB<n>_<m>` normalised: their
function index depends on what else the file holds) and the resource figures of the metadata: vgpr_count, sgpr_count, LDS,
scratch, spills.  Reported: equal / different per kernel with the sizes (and whether the difference is only the order of source operands,
instruction by instruction), a summary per kernel family, and the kernels only one side has."""
import argparse
import collections
import re

FIELDS = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def metadata(text, pattern=""):
    """{mangled name: {register, spill, scratch counts, "lds"}} of every kernel whose name matches `pattern`"""
    meta = {}
    for entry in text[text.index("amdhsa.kernels:"):].split("\n  - ")[1:]:          # one metadata entry per kernel
        name = re.search(r"\.name:\s+(\S+)", entry)                              # (amdhsa.version's list has none)
        if not name or not re.search(pattern, name.group(1)):
            continue
        found = dict(re.findall(r"\.(%s):\s+(\d+)" % "|".join(FIELDS), entry))
        meta[name.group(1)] = {"lds" if k == "group_segment_fixed_size" else k: int(found[k]) for k in FIELDS}
    return meta


def kernels(paths):
    """{mangled name: (instructions, metadata)} over the files of one side"""
    out = {}
    for path in paths:
        text = open(path).read()
        meta = metadata(text)
        for m in re.finditer(r"^(\S+):\s*;\s*@\1\s*$(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
            if m.group(1) not in meta:
                continue
            ins = [re.sub(r"\.LBB\d+_", ".LBB_", ln.strip()) for ln in m.group(2).splitlines()
                   if ln.startswith("\t") and not ln.strip().startswith((".", ";"))]
            out[m.group(1)] = (ins, meta[m.group(1)])
    return out


COMMUTATIVE = re.compile(r"^[sv]_(add_f\d+|mul_f\d+|mul_lo_u32|mul_hi_u32|mul_i32|add_u32|add_i32|and_b\d+|or_b\d+|xor_b\d+|max_[fiu]\d+|min_[fiu]\d+)(_e32|_e64)?$")


def exchanged_only(ia, ib):
    """do the two instruction lists differ in nothing but the order of the two source operands of commutative instructions,
    instruction by instruction?"""
    def same(x, y):
        if x == y:
            return True
        (ox, _, rx), (oy, _, ry) = x.partition(" "), y.partition(" ")
        ax, ay = rx.split(", "), ry.split(", ")
        return ox == oy and bool(COMMUTATIVE.match(ox)) and len(ax) == 3 and ax[0] == ay[0] and ax[1:] == ay[:0:-1]
    return len(ia) == len(ib) and all(same(x, y) for x, y in zip(ia, ib))


def family(name):
    """the kernel's own name out of its mangled one (an anonymous namespace in front or not)"""
    m = re.match(r"_ZN?(?:12_GLOBAL__N_1)?(\d+)", name)
    return name[m.end():m.end() + int(m.group(1))] if m else name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--a", nargs="+", required=True, help="assembly files of the first build")
    ap.add_argument("--b", nargs="+", required=True, help="assembly files of the second build")
    args = ap.parse_args()
    A, B = kernels(args.a), kernels(args.b)
    fam = collections.defaultdict(lambda: [0, 0])
    for name in sorted(set(A) & set(B), key=lambda n: (family(n), n)):
        (ia, ma), (ib, mb) = A[name], B[name]
        same = ia == ib and ma == mb
        fam[family(name)][0 if same else 1] += 1
        if not same:
            what = " ".join(f"{k} {ma[k]}->{mb[k]}" for k in ma if ma[k] != mb[k])
            swaps = sum(x != y for x, y in zip(ia, ib)) if ma == mb and exchanged_only(ia, ib) else 0
            note = f"; the two source operands of {swaps} commutative instructions exchanged, nothing else" if swaps else ""
            print(f"DIFFERENT {name}: {len(ia)} -> {len(ib)} instructions{'; ' + what if what else ''}{note}")
    for side, only in (("first", sorted(set(A) - set(B))), ("second", sorted(set(B) - set(A)))):
        for name in only:
            print(f"ONLY IN THE {side.upper()} BUILD {name}")
    print(f"{'family':<24}{'equal':>8}{'different':>11}")
    for f in sorted(fam):
        print(f"{f:<24}{fam[f][0]:>8}{fam[f][1]:>11}")
    print(f"{'all':<24}{sum(v[0] for v in fam.values()):>8}{sum(v[1] for v in fam.values()):>11}    ({len(A)} kernels in the first build, {len(B)} in the second)")


if __name__ == "__main__":
    main()
