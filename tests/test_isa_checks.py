"""ISA-level checks of the cross-workgroup protocols (CPU only: hipcc cross-compiles gfx950 without a GPU).

The fused verification kernel combines its workgroups through agent-scope atomics with RELAXED ordering (a device-scope
fence is an L2 write-back on this multi-XCD part; ADVICE round 1 called the resulting reliance on hardware behaviour
fragile).  What the correctness argument needs from the generated code is pinned here, so that a compiler change that
breaks it fails the CPU suite instead of producing a rare wrong verdict:
  * the adds into the shared accumulator are RETURNING atomics (`sc0`: the old value comes back = the add was performed),
  * between the last of them and the workgroup barrier the wave executes `s_waitcnt vmcnt(0)`,
  * the arrival counter is bumped only after that barrier,
  * the default build contains no `buffer_wbl2` / `buffer_inv` (the fence-free form is what is being measured), the
    FZ_VERIFY_ORDERED instantiation contains both."""
import collections
import re

from _isa import STREAM_UNITS, TRANSFORM_UNITS, asm, bodies, family, metadata

# kernels per family: the host dispatch instantiates one for every (degree, multiply form, shape) it can launch and no other
KERNELS = {"ntt_fwd16": 8, "ntt_inv16": 8, "ntt_fwd4": 20, "ntt_inv4": 20, "ntt_jobs4": 60, "ntt_jobs16": 12, "ntt_jobs16_keep": 24,
           "ntt_small": 8, "ntt_big": 2, "polymul_fused": 4, "polymul16": 8, "records_encode": 5, "records_decode": 5,
           "records_zero_failed": 1, "keygen_fused": 8, "keygen_bcast_fused": 4, "verify_fused": 32, "diag_*": 3}


def test_the_units_hold_the_kernels_of_every_family_and_no_other():
    got = collections.Counter()
    for unit in TRANSFORM_UNITS:
        for name in metadata(asm(unit)):
            f = family(name)
            got["diag_*" if f.startswith("diag_") else f] += 1
    assert dict(got) == KERNELS
    assert sum(got.values()) == 232


# the two units of streaming kernels: what the launchers of fz_pointwise.hip and fz_aggregate.hip can launch and no other
STREAM_KERNELS = {"pw_kernel": 5, "matvec_sliced_kernel": 5, "aggregate_onepass": 9, "aggregate_direct": 4, "pw_bcast_kernel": 1,
                  "matvec_kernel": 1, "matvec_split_kernel": 1, "matvec_scalar_kernel": 1, "sign_kernel": 1, "sign_scalar_kernel": 1,
                  "aggregate_generic_kernel": 1, "target_kernel": 1, "zero_i64_kernel": 1, "reduce_i64_kernel": 1,
                  "norm_weight_kernel": 1, "verdict_kernel": 1, "bcast_rows_kernel": 1, "fill_synthetic_kernel": 1}


def test_the_streaming_units_hold_the_kernels_of_every_family_and_aggregation_has_its_own():
    got = {unit: collections.Counter(family(name) for name in metadata(asm(unit))) for unit in STREAM_UNITS}
    assert dict(got["fz_pointwise"] + got["fz_aggregate"]) == STREAM_KERNELS
    assert sum(STREAM_KERNELS.values()) == 37
    assert set(got["fz_aggregate"]) == {f for f in STREAM_KERNELS if f.startswith("aggregate_")}
    assert not set(got["fz_pointwise"]) & set(got["fz_aggregate"])


def test_verify_fused_orders_its_adds_before_the_arrival():
    ks = bodies(asm("fz_transforms"), "verify_fused")
    # degree 64 / 256 x general / pseudo-Mersenne multiply x int32 / int64 rows x ordered / not x integer / fp64 accumulation of
    # A * sigma (round 3 also carried one / two row groups per iteration x twiddles as pairs / w alone: 128 instantiations)
    assert len(ks) == 32, sorted(ks)
    for name, ins in ks.items():
        ordered = re.search(r"verify_fusedILi\dELb\dE[il]Lb(\d)ELb\dE", name).group(1) == "1"     # fourth template argument
        adds = [i for i, s in enumerate(ins) if s.startswith("global_atomic_add_f64")]
        assert adds, name
        assert all(" sc0" in ins[i] for i in adds), (name, [ins[i] for i in adds])      # returning form
        after = ins[adds[-1] + 1:]
        bar = next(i for i, s in enumerate(after) if s.startswith("s_barrier"))
        assert any(s.startswith("s_waitcnt vmcnt(0)") for s in after[:bar]), (name, after[:bar])
        arrive = [i for i, s in enumerate(ins) if s.startswith("global_atomic_add ") or s.startswith("global_atomic_add_u32")]
        assert arrive and arrive[0] > adds[-1] + 1 + bar, name
        fences = [s for s in ins if s.startswith(("buffer_wbl2", "buffer_inv"))]
        assert bool(fences) == ordered, (name, fences)


def test_aggregate_onepass_instantiations_do_not_spill_and_add_with_returning_atomics():
    """aggregate_onepass<8, RAG, SIGN, AR>: the nine instantiations the launcher can pick (rows per column block 4 / 3 / 2 x plain /
    ragged / fused signing) keep their state in registers -- no scratch (a spill in the signer loop would double the launch) --
    and every cross-workgroup sum is added with a RETURNING 64-bit atomic (the arrival count travels in the word the add returns),
    paired with the one non-returning add that re-arms the word"""
    text = asm("fz_aggregate")
    meta = metadata(text, "aggregate_onepass")
    assert len(meta) == 9, sorted(meta)
    for name, f in meta.items():
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0, (name, f)
        assert f["vgpr_count"] <= 256, (name, f)                 # two waves per SIMD: one 8-wave workgroup per CU
    ks = bodies(text, "aggregate_onepass")
    assert len(ks) == 9
    for name, ins in ks.items():
        adds = [s for s in ins if s.startswith("global_atomic_add_x2")]
        returning = [s for s in adds if " sc0" in s]           # the sum's add: its return value says who arrived last
        rearm = [s for s in adds if " sc0" not in s]           # the last arrival's subtraction that re-arms the word: result unused
        assert returning and len(returning) == len(rearm), (name, adds)
