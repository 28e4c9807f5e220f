"""CPU half of the far-offset tests (tests/_far.py, tests/test_gpu_far_offsets.py).

Part one: the helper itself.  The indexable stream equals oracle.splitmix_centered on runs below and above index 2^32; every
case's operand is the smallest that crosses its thresholds, with a ragged remainder; every fault model that applies to a case
changes a SAMPLED row (so the sampled-row check alone sees it; the whole-buffer comparison sees every changed row); the alias rows
a wrapped store would overwrite are sampled; the pieces of the whole-buffer comparison are out of every model's reach.

Part two: the size refusals of the entry points, on both sides of their limit, without a GPU.  csrc/fz_capi.hip and csrc/fz_records_capi.hip are compiled
for the host with the REAL host launchers of fz_ntt.hip, fz_pointwise.hip, fz_wide.hip and fz_verify_encoded.hip (their kernel
launches end in a recording hipLaunchKernel of the stub runtime: kernel name, grid, and the count arguments) and recording
stand-ins for the other fz_launch_* (they store the counts they were handed), linked with a driver into a stand-alone program
under AddressSanitizer and UBSan.  At the limit the call reaches the launcher with its counts unchanged; at limit + 1 it
returns the documented code and logs no runtime call.  No buffer is ever touched: every pointer is a dummy (the wide path's
entries copy host arrays: for them the stub's copies touch nothing and its large allocations are backed by one byte)."""
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

import _far as F
from _hip_stub import CSRC, STUB, build_driver, fatbin_definitions


# ---- part one: the helper -----------------------------------------------------------------------------------------------------------
def test_prime_and_constants_match_the_sources():
    assert F.PRIME == O.PRIME
    dev = open(os.path.join(CSRC, "fz_ntt_dev.h")).read()
    assert "constexpr int kChunk = %d;" % F.CHUNK in dev and "constexpr int kWavesPerBlock = %d;" % F.WAVES_PER_BLOCK in dev
    assert F.PIECE_BYTES < 1 << 31 and all(k * F.PIECE_BYTES not in (1 << 32, 1 << 33, 1 << 34) for k in range(1, 16))


@pytest.mark.parametrize("first", [0, 12345, (1 << 32) - 1000, (1 << 32) - 1, 1 << 32, (1 << 32) + 777, (1 << 33) + 5])
def test_stream_at_equals_the_oracle_stream_below_and_above_2_32(first):
    for seed in (5, 0xFFFFFFFFFFFFFFF1):
        want = O.splitmix_centered(F.shifted_seed(seed, first), 3000)
        assert np.array_equal(F.stream_run(seed, first, 3000), want)
        idx = np.array([first + 2999, first, first + 17, first + 17], dtype=np.uint64)      # any order, repeats
        assert np.array_equal(F.stream_at(seed, idx), want[[2999, 0, 17, 17]])
    assert np.array_equal(F.stream_run(9, first, 64, q=12289), O.splitmix_centered(F.shifted_seed(9, first), 64, q=12289))


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_operand_is_the_smallest_that_crosses_with_a_ragged_remainder(case):
    crossed = F.crossed(case)
    assert crossed, "the operand crosses nothing"
    top = max(crossed.values())
    # the smallest: three rows fewer (or 1027 values at one value per row) and the highest threshold is not crossed
    spare = 1027 if case.unit == 1 else 3
    part = 1 if top % case.unit else 0                      # (a record that straddles the threshold)
    assert 0 < F.elems(case) - top <= max(spare, (3 + part) * case.unit) and (case.rows - spare - part) * case.unit <= top
    assert F.excess(case)[max(crossed, key=crossed.get)] == F.elems(case) - top
    if case.unit == 1:
        assert case.rows % 4 != 0 and case.rows % case.degree != 0
    if case.chunked:
        assert F.elems(case) % F.CHUNK != 0, "no partial last chunk"
        tasks = -(-F.elems(case) // F.CHUNK)
        assert tasks % F.WAVES_PER_BLOCK != 0, "the last workgroup has no idle wave"
    assert case.count * case.per_count == F.elems(case)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_sample_set_holds_ends_thresholds_and_aliases(case):
    rows = set(F.sampled_rows(case).tolist())
    win = F.windows(case)
    assert all(n > 0 and lo >= 0 and lo + n <= case.rows for lo, n in win)
    assert all(a[0] + a[1] < b[0] for a, b in zip(win, win[1:])), "windows overlap or touch"
    assert {0, 1, case.rows - 1, case.rows - 2} <= rows
    for e in F.crossed(case).values():
        r = e // case.unit
        assert {r - 1, r, r + 1} <= rows, "both sides of a threshold"
        for shift in (F.T1_BYTES // case.esize, F.T2_ELEMS, F.T3_ELEMS):
            a = (r * case.unit - shift) // case.unit
            if a >= 1:
                assert {a, a + 1} <= rows, "alias of a threshold row"
    last = case.rows - 1
    for shift in (F.T1_BYTES // case.esize, F.T2_ELEMS, F.T3_ELEMS):
        if last * case.unit >= shift:
            assert -(-(last * case.unit - shift) // case.unit) in rows, "alias of the last row"
    assert len(rows) * case.unit <= 64 * F.WINDOW_ELEMS, "the sample set stays small"
    pieces = F.pieces(case)
    assert sum(n for _, n in pieces) == case.rows and all(n * case.unit * case.esize <= F.PIECE_BYTES for _, n in pieces)
    for lo, _ in pieces[1:]:
        assert all(lo * case.unit != e for e in F.crossed(case).values()), "a piece boundary on a threshold"


STREAM_PAIRS = [(c, m) for c in F.CASES if c.kind == "stream" for m in F.MODELS if F.applies(m, c)]


@pytest.mark.parametrize("case,model", STREAM_PAIRS, ids=lambda x: x if isinstance(x, str) else x.name)
def test_every_applicable_fault_model_changes_a_sampled_row(case, model):
    rows = F.sampled_rows(case)
    bad_load = F.wrong_rows(model, case, rows, "load")
    assert bad_load.size, "a narrowed load index changes no sampled row"
    f = F.row_map(model, case, bad_load)
    assert (f != bad_load).all()
    bad_store = set(F.wrong_rows(model, case, rows, "store").tolist())
    assert set(bad_load.tolist()) <= bad_store, "a row whose store went elsewhere keeps its poison"
    if model != "count_u32":
        # the rows a wrapped store lands on are in the sample set: they must hold their own result, and the check reads them
        landed = {int(x) for x in f if x >= 0}
        assert landed & bad_store and landed & set(rows.tolist()), "no sampled alias row receives a foreign result"
    # the whole-buffer comparison sees it as well: inside a piece, at its shifted base, no index is large enough for the model to
    # change it (so the piecewise reference is right where the whole call is wrong)
    for lo, n in F.pieces(case):
        piece = case._replace(rows=n, count=n * case.unit // case.per_count)
        assert not F.applies(model, piece)
        ends = np.array([0, n - 1], dtype=np.int64)
        assert np.array_equal(F.row_map(model, piece, ends), ends)


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c.name)
def test_models_that_do_not_apply_change_nothing(case):
    rows = F.sampled_rows(case)
    for m in F.MODELS:
        if not F.applies(m, case):
            assert np.array_equal(F.row_map(m, case, rows), rows)
    assert F.applies("u32_bytes", case), "every case crosses T1"


@pytest.mark.parametrize("name", [c.name for c in F.CASES if c.kind == "accumulate"][:1])
def test_a_narrowed_signer_offset_changes_the_sampled_aggregate_columns(name):
    case = F.CASE[name]
    for k, j in ((0, 0), (3, 255)):
        honest = F.accumulate_column(case, 1, 2, k, j, 4)
        assert honest == F.accumulate_column(case, 1, 2, k, j, 4, model="u32_elems")         # (does not apply: nothing changes)
        assert honest != F.accumulate_column(case, 1, 2, k, j, 4, model="u32_bytes")
    # the column sum is the oracle's on a short prefix (the same arithmetic, all signers)
    short = case._replace(rows=37)
    sig = O.splitmix_centered(1, 37 * 4 * 256).reshape(37, 4, 256)
    alpha = O.splitmix_centered(2, 37 * 256).reshape(37, 256)
    ref = O.COracle().aggregate_core(sig, alpha, F.PRIME)
    assert all(F.accumulate_column(short, 1, 2, k, j, 4) == ref[k, j] for k, j in ((0, 0), (1, 7), (3, 255)))


def test_table_keys_are_unique_and_three_threshold_cases_meet_every_model():
    """a consistency check of the table, not a proof that its cases are independent: no two cases state the same (entry, operand,
    degree, route, thresholds crossed); each three-threshold case has its quick T1 half; the models each must meet"""
    keys = [(c.entry, c.operand, c.degree, tuple(sorted(c.route.items())), tuple(sorted(F.crossed(c)))) for c in F.CASES]
    assert len(set(keys)) == len(keys)
    for c in F.CASES:
        if c.esize == 4 and len(F.crossed(c)) == 3:
            want = set(F.MODELS) if c.per_count == 1 else set(F.MODELS) - {"count_u32"}
            assert {m for m in F.MODELS if F.applies(m, c)} == want, c.name
            quick = F.CASE[c.name + "_t1"]
            assert (quick.entry, quick.operand, quick.degree, quick.route, quick.unit) == (c.entry, c.operand, c.degree, c.route, c.unit)
            assert sorted(F.crossed(quick)) == ["T1"]
    assert set(F.QUICK.values()) == {c.name for c in F.CASES if c.esize == 4 and len(F.crossed(c)) == 3}
    assert all(len(u) == 3 and all(u) for u in F.UNREACHABLE)


def test_every_case_has_a_gpu_test():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_far_offsets.py")).read()
    for c in F.CASES:
        assert '"%s"' % c.name in text, c.name


# ---- part two: the size refusals ------------------------------------------------------------------------------------------------------
UNITS = ("fz_capi", "fz_records_capi", "fz_context", "fz_diag", "fz_ntt", "fz_pointwise", "fz_wide", "fz_verify_encoded")
MARK = "// what fz_context.hip and fz_diag.hip take from the kernel units"
assert MARK in STUB
RUNTIME = STUB.split(MARK)[0]           # (the stand-ins behind the mark are per unit: the driver has its own, for the units not linked here)

DRIVER = RUNTIME + r'''
#include <map>
#include <hip/hip_ext.h>
#include "fusion_hip_generic.h"
// ---- kernel launches end here: name (from the registration), grid, block, the count arguments of the kernels the tests look at ----
struct Launch { std::string name; dim3 grid, block; std::vector<unsigned long long> v; };
static std::vector<Launch> g_launches;
static std::map<const void *, std::string> &kernel_names() { static std::map<const void *, std::string> m; return m; }
static bool has(const std::string &s, const char *t) { return s.find(t) != std::string::npos; }
template <int N> static void table_rows(void **args, std::vector<unsigned long long> &v) {
    FzJobsN<N> S;
    memcpy(&S, args[0], sizeof(S));
    for (int j = 0; j < N; ++j) if (S.in[j]) v.push_back(S.rows[j]);
}
static hipError_t launched(const void *f, dim3 grid, dim3 block, void **args, hipStream_t st) {
    Launch L{kernel_names().count(f) ? kernel_names()[f] : std::string("?"), grid, block, {}};
    auto size_at = [&](int k) { size_t x; memcpy(&x, args[k], sizeof(x)); L.v.push_back(x); };
    auto int_at = [&](int k) { int x; memcpy(&x, args[k], sizeof(x)); L.v.push_back((unsigned long long)x); };
    const std::string &n = L.name;
    if (has(n, "ntt_jobs")) {
        if (has(n, "FzJobsNILi4E")) table_rows<4>(args, L.v);
        else if (has(n, "FzJobsNILi8E")) table_rows<8>(args, L.v);
        else table_rows<32>(args, L.v);
    }
    else if (has(n, "ntt_fwd") || has(n, "ntt_inv")) size_at(2);                  // (in, out, batch, ...)
    else if (has(n, "matvec_sliced_kernel") || has(n, "matvec_kernel")) size_at(3);   // (A, S, out, batch, ...)
    else if (has(n, "verify_encoded") && !has(n, "finish")) int_at(4);            // (bytes, A, rv, rb, l, ...)
    else if (has(n, "fill_synthetic_kernel")) size_at(1);                         // (out, count, ...)
    else if (has(n, "wide_ntt_kernel")) size_at(2);                               // (in, out, batch, ...)
    else if (has(n, "wide_norm_weight_kernel")) size_at(1);                       // (rows, batch, ...)
    else if (has(n, "target_kernel")) size_at(6);                                 // (vkL, vkR, c, alpha, partial, pstride, N, ...)
    g_launches.push_back(L);
    rec("hipLaunchKernel", f, 0, st);
    return hipSuccess;
}
static thread_local struct { dim3 grid, block; size_t shmem; hipStream_t st; } g_cfg;
extern "C" {
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t st) { g_cfg = {grid, block, shmem, st}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *st) { *grid = g_cfg.grid; *block = g_cfg.block; *shmem = g_cfg.shmem; *st = g_cfg.st; return hipSuccess; }
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *device, unsigned, void *, void *, void *, void *, int *) { kernel_names()[host] = device; }
hipError_t hipLaunchKernel(const void *f, dim3 grid, dim3 block, void **args, size_t, hipStream_t st) { return launched(f, grid, block, args, st); }
hipError_t hipExtLaunchKernel(const void *f, dim3 grid, dim3 block, void **args, size_t, hipStream_t st, hipEvent_t, hipEvent_t, int) { return launched(f, grid, block, args, st); }
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *n, const void *, int, size_t) { *n = 2; return hipSuccess; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) { *v = 65535; return hipSuccess; }
}
// ---- recording stand-ins for the launchers of the units that are not linked: the counts they were handed ----
struct Rec { std::string fn; std::vector<unsigned long long> v; };
static std::vector<Rec> g_recs;
static int recd(const char *fn, std::initializer_list<unsigned long long> v) { g_recs.push_back({fn, v}); return FZ_OK; }
#define U(x) (unsigned long long)(x)
int fz_launch_aggregate(fz_ctx *, const int32_t *, const int32_t *, int64_t *, size_t, int32_t *, size_t groups, size_t N, int l, const int32_t *,
                        const int32_t *, const int32_t *, int64_t *, size_t, const size_t *h_off, const int32_t *, int32_t *) {
    return recd("aggregate", {U(groups), U(N), U(l), U(h_off ? h_off[groups] : 0)});
}
int fz_launch_keygen_fused(fz_ctx *, const int32_t *, const int32_t *, int32_t *, int32_t *, size_t segs, int l, bool) { return recd("keygen_fused", {U(segs), U(l)}); }
int fz_launch_records(fz_ctx *, bool, const void *, void *, size_t n, int rows, bool, int, int64_t, int *) { return recd("records", {U(n), U(rows)}); }
int fz_launch_check_records(fz_ctx *, const uint8_t *, size_t n, int rows, int, int64_t, int *) { return recd("check_records", {U(n), U(rows)}); }
int fz_launch_sign_encoded(fz_ctx *, const int32_t *, const int32_t *, size_t N, int l, int, int64_t, uint8_t *, int *) { return recd("sign_encoded", {U(N), U(l)}); }
int fz_launch_sign_records(fz_ctx *, const uint8_t *, int, int64_t, const int32_t *, size_t N, int l, int, int64_t, uint8_t *, int *) { return recd("sign_records", {U(N), U(l)}); }
int fz_launch_keygen_records(fz_ctx *, const int32_t *, const int32_t *, bool, size_t n, int l, int, int64_t, uint8_t *, int32_t *, int *) { return recd("keygen_records", {U(n), U(l)}); }
int fz_launch_aggregate_encoded(fz_ctx *, const uint8_t *, const int32_t *, const int *, size_t N, int l, int, int64_t, int64_t *, int32_t *) { return recd("aggregate_encoded", {U(N), U(l)}); }
int fz_launch_aggregate_encoded_ragged(fz_ctx *, const uint8_t *, const int32_t *, const int *, const size_t *off, size_t groups, int l, int, int64_t, int64_t *,
                                       size_t, int32_t *) { return recd("aggregate_encoded_ragged", {U(groups), U(off[groups]), U(l)}); }
int fz_launch_verify_fused(fz_ctx *, const int32_t *, const int32_t *, const int32_t *, size_t groups, int l, int64_t, int64_t, int *) { return recd("verify_fused", {U(groups), U(l)}); }
int fz_launch_verify_fused_i64(fz_ctx *, const int32_t *, const int64_t *, size_t, const int64_t *, size_t, size_t groups, int l, int64_t, int64_t, int *) {
    return recd("verify_fused_i64", {U(groups), U(l)});
}
int fz_launch_verify_signatures(fz_ctx *, const int32_t *, const int32_t *, const int32_t *, const int32_t *, size_t N, int l, int64_t, int64_t, int *) { return recd("verify_signatures", {U(N), U(l)}); }
int fz_launch_polymul_fused(fz_ctx *, const int32_t *, const int32_t *, int32_t *, size_t batch) { return recd("polymul_fused", {U(batch)}); }
bool fz_polymul16_ok(const fz_ctx *, const int32_t *, const int32_t *, const int32_t *, size_t) { return false; }
// the setup of each unit that is not linked
int fz_records_query_grid(fz_ctx *) { return FZ_OK; }
int fz_aggregate_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_sign_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_aggregate_many_encoded_query_grid(fz_ctx *) { return FZ_OK; }
int fz_sign_records_query_grid(fz_ctx *) { return FZ_OK; }
int fz_keygen_records_query_grid(fz_ctx *) { return FZ_OK; }

// ---- the checks ----
static int g_fail = 0;
static const char *g_label = "";
static int g_mark = 0;                                   // g_fail when the block that prints its own "ok" began
#define CHECK(c) do { if (!(c)) { printf("FAIL %s: %s (line %d; last error: %s)\n", g_label, #c, __LINE__, fz_last_error()); ++g_fail; } } while (0)
struct Snap { size_t log, launches, recs; };
static Snap snap() { return {stub_mark(), g_launches.size(), g_recs.size()}; }
// the call was refused with `code`, and nothing reached the runtime or a launcher
static void refused(const char *label, int rc, int code, Snap s) {
    g_label = label;
    const int f0 = g_fail;
    CHECK(rc == code);
    CHECK(stub_mark() == s.log && g_launches.size() == s.launches && g_recs.size() == s.recs);
    if (g_fail == f0) printf("ok %s\n", label);
}
// the call went through: the stand-in `fn` was reached once with exactly these counts
static void reached(const char *label, int rc, Snap s, const char *fn, std::vector<unsigned long long> want) {
    g_label = label;
    const int f0 = g_fail;
    CHECK(rc == FZ_OK);
    CHECK(g_recs.size() == s.recs + 1 && g_recs.back().fn == fn && g_recs.back().v == want);
    if (g_fail == f0) printf("ok %s\n", label);
}
// the call went through to a kernel launch whose name holds `kernel`, with these count arguments
static void launched_as(const char *label, int rc, Snap s, const char *kernel, std::vector<unsigned long long> want) {
    g_label = label;
    const int f0 = g_fail;
    CHECK(rc == FZ_OK);
    bool found = false;
    for (size_t k = s.launches; k < g_launches.size(); ++k) found |= has(g_launches[k].name, kernel) && g_launches[k].v == want;
    CHECK(found);
    if (g_fail == f0) printf("ok %s\n", label);
}
static fz_ctx *make_ctx(int degree) {
    fz_ctx *c = nullptr;
    const int rc = degree == 256 ? fz_ctx_create(0, 2147465729u, 256, 3337519u, 1978410468u, &c) : fz_ctx_create(0, 2147465729u, 64, 23584283u, 540632852u, &c);
    if (rc != FZ_OK) { printf("FAIL context: %s\n", fz_last_error()); exit(2); }
    return c;
}

int main() {
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers: address on\n");
#else
    printf("sanitizers: address off\n");
#endif
#endif
    alignas(16) static char dummy[1024];
    const int32_t *I = (const int32_t *)dummy;
    int32_t *O32 = (int32_t *)dummy;
    int64_t *O64 = (int64_t *)dummy;
    const uint8_t *B = (const uint8_t *)dummy;
    uint8_t *BO = (uint8_t *)dummy;
    int *ST = (int *)dummy;
    const size_t G = 65535, N21 = ((size_t)1 << 21) - 1, N22 = ((size_t)1 << 22) - 1;
    fz_ctx *c = make_ctx(256);
    const size_t ld = 4 * 256;
    Snap s;

    // ---- groups <= 65535 (FZ_E_BADARG) ----
    s = snap(); reached("groups aggregate_partial_batch at 65535", fz_aggregate_partial_batch(c, I, I, O64, ld, G, 3, 4), s, "aggregate", {G, 3, 4, 0});
    s = snap(); refused("groups aggregate_partial_batch at 65536", fz_aggregate_partial_batch(c, I, I, O64, ld, G + 1, 3, 4), FZ_E_BADARG, s);
    s = snap(); reached("groups aggregate_target_partial_batch at 65535", fz_aggregate_target_partial_batch(c, I, I, I, I, I, O64, ld, O64, 256, G, 3, 4), s, "aggregate", {G, 3, 4, 0});
    s = snap(); refused("groups aggregate_target_partial_batch at 65536", fz_aggregate_target_partial_batch(c, I, I, I, I, I, O64, ld, O64, 256, G + 1, 3, 4), FZ_E_BADARG, s);
    s = snap(); reached("groups sign_aggregate_target_partial_batch at 65535", fz_sign_aggregate_target_partial_batch(c, I, I, I, I, I, O32, O64, ld, O64, 256, G, 3, 4), s, "aggregate", {G, 3, 4, 0});
    s = snap(); refused("groups sign_aggregate_target_partial_batch at 65536", fz_sign_aggregate_target_partial_batch(c, I, I, I, I, I, O32, O64, ld, O64, 256, G + 1, 3, 4), FZ_E_BADARG, s);
    s = snap();
    { const int rc = fz_target_partial_batch(c, I, I, I, I, O64, 256, G, 3);
      launched_as("groups target_partial_batch at 65535", rc, s, "target_kernel", {3});
      g_label = "groups target_partial_batch at 65535"; CHECK(g_launches.back().grid.z == G); }
    s = snap(); refused("groups target_partial_batch at 65536", fz_target_partial_batch(c, I, I, I, I, O64, 256, G + 1, 3), FZ_E_BADARG, s);
    s = snap(); reached("groups verify_with_target_batch_async at 65535", fz_verify_with_target_batch_async(c, I, I, I, G, 4, 1, 1, ST), s, "verify_fused", {G, 4});
    s = snap(); refused("groups verify_with_target_batch_async at 65536", fz_verify_with_target_batch_async(c, I, I, I, G + 1, 4, 1, 1, ST), FZ_E_BADARG, s);
    s = snap(); reached("groups verify_partials_batch_async at 65535", fz_verify_partials_batch_async(c, I, O64, ld, O64, 256, G, 4, 1, 1, ST), s, "verify_fused_i64", {G, 4});
    s = snap(); refused("groups verify_partials_batch_async at 65536", fz_verify_partials_batch_async(c, I, O64, ld, O64, 256, G + 1, 4, 1, 1, ST), FZ_E_BADARG, s);
    { int v[1]; s = snap(); refused("groups verify_with_target_batch at 65536", fz_verify_with_target_batch(c, I, I, I, G + 1, 4, 1, 1, v), FZ_E_BADARG, s); }

    // ---- N < 2^21 on the int32-row aggregates (FZ_E_BADARG), the ragged form's per-group and total limits ----
    s = snap(); reached("N aggregate_core at 2^21 - 1", fz_aggregate_core(c, I, I, O32, N21, 4), s, "aggregate", {1, N21, 4, 0});
    s = snap(); refused("N aggregate_core at 2^21", fz_aggregate_core(c, I, I, O32, N21 + 1, 4), FZ_E_BADARG, s);
    s = snap(); reached("N aggregate_partial at 2^21 - 1", fz_aggregate_partial(c, I, I, O64, N21, 4), s, "aggregate", {1, N21, 4, 0});
    s = snap(); refused("N aggregate_partial at 2^21", fz_aggregate_partial(c, I, I, O64, N21 + 1, 4), FZ_E_BADARG, s);
    s = snap(); refused("N aggregate_target_partial_batch at 2^21", fz_aggregate_target_partial_batch(c, I, I, I, I, I, O64, ld, O64, 256, 1, N21 + 1, 4), FZ_E_BADARG, s);
    s = snap(); refused("N sign_aggregate_target_partial_batch at 2^21", fz_sign_aggregate_target_partial_batch(c, I, I, I, I, I, O32, O64, ld, O64, 256, 1, N21 + 1, 4), FZ_E_BADARG, s);
    s = snap(); refused("N target_partial_batch at 2^21", fz_target_partial_batch(c, I, I, I, I, O64, 256, 1, N21 + 1), FZ_E_BADARG, s);
    { size_t off[3] = {0, N21, 2 * N21};
      s = snap(); reached("N aggregate_core_ragged group at 2^21 - 1", fz_aggregate_core_ragged(c, I, I, off, 2, 4, O32), s, "aggregate", {2, N21, 4, 2 * N21});
      off[2] = 2 * N21 + 1;
      s = snap(); refused("N aggregate_core_ragged group at 2^21", fz_aggregate_core_ragged(c, I, I, off, 2, 4, O32), FZ_E_BADARG, s); }
    { std::vector<size_t> off(2050);                                        // 2049 groups: the total reaches 0xfffffffe / 0xffffffff
      const size_t per = 0xfffffffeull / 2049;
      for (size_t g = 0; g <= 2049; ++g) off[g] = g * per;
      off[2049] = 0xfffffffeull;
      g_label = "ragged total"; CHECK(off[2049] - off[2048] < ((size_t)1 << 21));
      s = snap();
      { const int rc = fz_aggregate_core_ragged(c, I, I, off.data(), 2049, 4, O32);
        g_label = "total aggregate_core_ragged at 0xfffffffe"; g_mark = g_fail; CHECK(rc == FZ_OK && g_recs.size() == s.recs + 33 && g_recs.back().v[3] == 0xfffffffeull);
        if (g_fail == g_mark) printf("ok %s\n", g_label); }
      off[2049] = 0xffffffffull;
      s = snap(); refused("total aggregate_core_ragged at 0xffffffff", fz_aggregate_core_ragged(c, I, I, off.data(), 2049, 4, O32), FZ_E_BADARG, s); }

    // ---- the compact-bytes entries: rows * degree <= 0x7fffffff, the records product, N < 2^22 (FZ_E_UNSUPPORTED), l < 2^22 ----
    const int R = 0x7fffffff / 256;                                          // 8388607 rows of degree 256
    s = snap(); reached("rows*degree encode_records at 0x7fffff00", fz_encode_records_async(c, I, 2, R, 0, 1, BO, ST), s, "records", {2, U(R)});
    s = snap(); refused("rows*degree encode_records past 0x7fffffff", fz_encode_records_async(c, I, 2, R + 1, 0, 1, BO, ST), FZ_E_BADARG, s);
    s = snap(); reached("rows*degree decode_records at 0x7fffff00", fz_decode_records_async(c, B, 2, R, 0, 1, O32, ST), s, "records", {2, U(R)});
    s = snap(); refused("rows*degree decode_records past 0x7fffffff", fz_decode_records_async(c, B, 2, R + 1, 0, 1, O32, ST), FZ_E_BADARG, s);
    s = snap(); reached("rows*degree check_records at 0x7fffff00", fz_check_records_async(c, B, 2, R, 1, ST), s, "check_records", {2, U(R)});
    s = snap(); refused("rows*degree check_records past 0x7fffffff", fz_check_records_async(c, B, 2, R + 1, 1, ST), FZ_E_BADARG, s);
    s = snap(); reached("rows*degree sign_encoded at 0x7fffff00", fz_sign_encoded_async(c, I, I, 2, R, 1, BO, ST), s, "sign_encoded", {2, U(R)});
    s = snap(); refused("rows*degree sign_encoded past 0x7fffffff", fz_sign_encoded_async(c, I, I, 2, R + 1, 1, BO, ST), FZ_E_BADARG, s);
    const size_t NP = ((size_t)-1 >> 3) / 256;                               // the most records of one row
    s = snap(); reached("records product encode_records at the most", fz_encode_records_async(c, I, NP, 1, 0, 1, BO, ST), s, "records", {NP, 1});
    s = snap(); refused("records product encode_records one more", fz_encode_records_async(c, I, NP + 1, 1, 0, 1, BO, ST), FZ_E_BADARG, s);
    s = snap(); reached("N aggregate_encoded at 2^22 - 1", fz_aggregate_encoded_async(c, B, I, nullptr, N22, 4, 1, O64, O32), s, "aggregate_encoded", {N22, 4});
    s = snap(); refused("N aggregate_encoded at 2^22", fz_aggregate_encoded_async(c, B, I, nullptr, N22 + 1, 4, 1, O64, O32), FZ_E_UNSUPPORTED, s);
    { size_t off[3] = {0, N22, 2 * N22};
      s = snap(); reached("N aggregate_encoded_ragged group at 2^22 - 1", fz_aggregate_encoded_ragged_async(c, B, I, nullptr, off, 2, 4, 1, O64, ld, O32), s, "aggregate_encoded_ragged", {2, 2 * N22, 4});
      off[2] = 2 * N22 + 1;
      s = snap(); refused("N aggregate_encoded_ragged group at 2^22", fz_aggregate_encoded_ragged_async(c, B, I, nullptr, off, 2, 4, 1, O64, ld, O32), FZ_E_UNSUPPORTED, s); }
    { std::vector<size_t> off(1026);
      for (size_t g = 0; g <= 1025; ++g) off[g] = g * N22;
      off[1025] = 0xffffffbfull;
      g_label = "encoded ragged total"; CHECK(off[1025] - off[1024] < ((size_t)1 << 22) && off[1025] > off[1024]);
      s = snap(); reached("total aggregate_encoded_ragged at 0xffffffbf", fz_aggregate_encoded_ragged_async(c, B, I, nullptr, off.data(), 1025, 4, 1, O64, ld, O32), s, "aggregate_encoded_ragged", {1025, 0xffffffbfull, 4});
      off[1025] = 0xffffffc0ull;
      s = snap(); refused("total aggregate_encoded_ragged at 0xffffffc0", fz_aggregate_encoded_ragged_async(c, B, I, nullptr, off.data(), 1025, 4, 1, O64, ld, O32), FZ_E_UNSUPPORTED, s); }
    // fz_keygen_records_async: records of 2 l rows, and a workgroup per (key, half) in one grid: N <= 0x3fffffff (FZ_E_BADARG)
    const int LK = 0x7fffffff / 512;                                         // 4194303: 2 l rows of degree 256
    s = snap(); reached("rows*degree keygen_records at 0x7ffffe00", fz_keygen_records_async(c, I, I, 1, 2, LK, 1, BO, O32, ST), s, "keygen_records", {2, U(LK)});
    s = snap(); refused("rows*degree keygen_records past 0x7fffffff", fz_keygen_records_async(c, I, I, 1, 2, LK + 1, 1, BO, O32, ST), FZ_E_BADARG, s);
    s = snap(); refused("rows*degree keygen_records l at 2^30", fz_keygen_records_async(c, I, I, 1, 2, 1 << 30, 1, BO, O32, ST), FZ_E_BADARG, s);
    g_label = "rows*degree keygen_records l at 2^30"; CHECK(strstr(fz_last_error(), "too many") != nullptr);      // (2 l is taken in 64 bits: the size's refusal, not the rows')
    s = snap(); refused("rows*degree keygen_records l at 2^31 - 1", fz_keygen_records_async(c, I, I, 1, 2, 0x7fffffff, 1, BO, O32, ST), FZ_E_BADARG, s);
    s = snap(); reached("N keygen_records at 0x3fffffff", fz_keygen_records_async(c, I, I, 1, 0x3fffffff, 4, 1, BO, O32, ST), s, "keygen_records", {0x3fffffffull, 4});
    s = snap(); refused("N keygen_records at 0x40000000", fz_keygen_records_async(c, I, I, 1, 0x40000000, 4, 1, BO, O32, ST), FZ_E_BADARG, s);
    // fz_verify_encoded_async: l < 2^22 in the real launcher (512 records: one workgroup per record, no shared area)
    s = snap(); launched_as("l verify_encoded at 2^22 - 1", fz_verify_encoded_async(c, I, B, 512, (int)N22, 1, I, nullptr, nullptr, ST), s, "verify_encoded", {N22});
    s = snap(); refused("l verify_encoded at 2^22", fz_verify_encoded_async(c, I, B, 512, (int)N22 + 1, 1, I, nullptr, nullptr, ST), FZ_E_UNSUPPORTED, s);

    // ---- keygen: batch * 2 <= 0x7fffffff takes the fused launch, one more the two-launch form (not a refusal: both sides run) ----
    s = snap(); reached("batch*2 keygen_core at 0x7ffffffe", fz_keygen_core(c, I, I, O32, O32, 0x3fffffff, 4), s, "keygen_fused", {0x7ffffffeull, 4});
    s = snap();
    { const int rc = fz_keygen_core(c, I, I, O32, O32, 0x40000000, 4);
      launched_as("batch*2 keygen_core at 0x80000000: transform", rc, s, "ntt_fwd", {0x80000000ull * 4});
      launched_as("batch*2 keygen_core at 0x80000000: products", rc, s, "matvec", {0x80000000ull});
      g_label = "batch*2 keygen_core at 0x80000000"; CHECK(g_recs.size() == s.recs); }
    s = snap(); reached("batch*2 keygen_core_bcast at 0x7ffffffe", fz_keygen_core_bcast(c, I, I, O32, O32, 0x3fffffff, 4), s, "keygen_fused", {0x7ffffffeull, 4});
    s = snap();
    { const int rc = fz_keygen_core_bcast(c, I, I, O32, O32, 0x40000000, 4);
      launched_as("batch*2 keygen_core_bcast at 0x80000000: transform", rc, s, "ntt_fwd", {0x80000000ull * 4});
      launched_as("batch*2 keygen_core_bcast at 0x80000000: products", rc, s, "matvec", {0x80000000ull}); }

    // ---- matvec: the sliced kernel's grid, blocks <= 0x7fffffff (FZ_E_UNSUPPORTED); 64 columns per product, 256 per workgroup ----
    const size_t MB = (size_t)0x7fffffff * 4;
    s = snap(); launched_as("blocks matvec at 0x7fffffff", fz_matvec(c, I, I, O32, MB, 8), s, "matvec_sliced_kernel", {MB});
    g_label = "blocks matvec at 0x7fffffff"; CHECK(g_launches.back().grid.x == 0x7fffffffu);
    s = snap(); refused("blocks matvec at 0x80000000", fz_matvec(c, I, I, O32, MB + 1, 8), FZ_E_UNSUPPORTED, s);

    // ---- the flat grid of the streaming kernels: gridDim.x * blockDim.x stays below 2^32 (the runtime refuses exactly 2^32 threads),
    // the count reaches the kernel unchanged and its grid-stride loop walks the rest ----
    for (size_t count : {((size_t)1 << 32) - 256, (size_t)1 << 32, ((size_t)1 << 32) + 1027}) {
        s = snap();
        launched_as(count < ((size_t)1 << 32) ? "threads fill_synthetic below 2^32" : count == ((size_t)1 << 32) ? "threads fill_synthetic at 2^32" : "threads fill_synthetic past 2^32",
                    fz_fill_synthetic(c, O32, count, 1), s, "fill_synthetic_kernel", {count});
        const Launch &L = g_launches.back();
        g_label = "threads fill_synthetic"; CHECK((unsigned long long)L.grid.x * L.block.x < (1ull << 32) && (unsigned long long)L.grid.x * L.block.x >= (1ull << 32) - 256);
    }

    // ---- fz_ntt_multi: rows < 2^31 per job, a flush at a full table and one at total + tasks > 0x7fffffff ----
    { fz_ntt_job jobs[33];
      for (int j = 0; j < 33; ++j) jobs[j] = {I + 4 * j, O32 + 4 * j, (size_t)(100 + j), j & 1};
      s = snap();
      const int rc = fz_ntt_multi(c, jobs, 33);
      g_label = "multi flush at a full table"; g_mark = g_fail;
      CHECK(rc == FZ_OK && g_launches.size() == s.launches + 2);
      if (g_launches.size() == s.launches + 2) {
          std::vector<unsigned long long> all = g_launches[s.launches].v, second = g_launches[s.launches + 1].v, want;
          CHECK(all.size() == 32 && second.size() == 1);
          all.insert(all.end(), second.begin(), second.end());
          for (int j = 0; j < 33; ++j) want.push_back((unsigned long long)(100 + j) | ((j & 1) ? 0x80000000ull : 0));
          std::sort(all.begin(), all.end()); std::sort(want.begin(), want.end());
          CHECK(all == want);                                               // every job launched exactly once
      }
      if (g_fail == g_mark) printf("ok %s\n", g_label);
      fz_ntt_job big[3] = {{I, O32, 0x40000000, 0}, {I + 4, O32 + 4, 0x3fffffff, 1}, {I + 8, O32 + 8, 1, 0}};
      s = snap();
      const int rc2 = fz_ntt_multi(c, big, 3);
      g_label = "multi flush at total + tasks > 0x7fffffff"; g_mark = g_fail;
      CHECK(rc2 == FZ_OK && g_launches.size() == s.launches + 2);
      if (g_launches.size() == s.launches + 2) {
          std::vector<unsigned long long> a = g_launches[s.launches].v, b = g_launches[s.launches + 1].v;
          std::sort(a.begin(), a.end());
          CHECK((a == std::vector<unsigned long long>{0x40000000ull, 0xbfffffffull}));   // 0x40000000 + 0x3fffffff tasks fill a launch exactly
          CHECK((b == std::vector<unsigned long long>{1}));
      }
      if (g_fail == g_mark) printf("ok %s\n", g_label);
      fz_ntt_job one[2] = {{I, O32, 0x7fffffff, 1}, {I + 4, O32 + 4, 5, 0}};
      s = snap();
      const int rc3 = fz_ntt_multi(c, one, 2);
      g_label = "multi rows at 2^31 - 1"; g_mark = g_fail;
      CHECK(rc3 == FZ_OK && g_launches.size() == s.launches + 2 && g_launches[s.launches].v == std::vector<unsigned long long>{0xffffffffull});
      if (g_fail == g_mark) printf("ok %s\n", g_label);
      one[0].rows = 0x80000000ull;
      s = snap(); refused("multi rows at 2^31", fz_ntt_multi(c, one, 2), FZ_E_BADARG, s); }
    fz_ctx_destroy(c);

    // ---- the radix-4 schedule's waves1 cap (FZ_E_UNSUPPORTED): one row group per wave is 1 row at degree 256, 4 at degree 64 ----
    setenv("FZ_NTT_KERNEL", "4", 1);
    c = make_ctx(256);
    s = snap(); launched_as("waves1 ntt_forward degree 256 at 0x7fffffff", fz_ntt_forward(c, I, O32, 0x7fffffff), s, "ntt_fwd4", {0x7fffffffull});
    s = snap(); refused("waves1 ntt_forward degree 256 at 0x80000000", fz_ntt_forward(c, I, O32, 0x80000000ull), FZ_E_UNSUPPORTED, s);
    s = snap(); launched_as("waves1 ntt_inverse degree 256 at 0x7fffffff", fz_ntt_inverse(c, I, O32, 0x7fffffff), s, "ntt_inv4", {0x7fffffffull});
    s = snap(); refused("waves1 ntt_inverse degree 256 at 0x80000000", fz_ntt_inverse(c, I, O32, 0x80000000ull), FZ_E_UNSUPPORTED, s);
    fz_ctx_destroy(c);
    c = make_ctx(64);
    s = snap(); launched_as("waves1 ntt_forward degree 64 at 4 * 0x7fffffff", fz_ntt_forward(c, I, O32, MB), s, "ntt_fwd4", {MB});
    s = snap(); refused("waves1 ntt_forward degree 64 one more", fz_ntt_forward(c, I, O32, MB + 1), FZ_E_UNSUPPORTED, s);
    fz_ctx_destroy(c);
    unsetenv("FZ_NTT_KERNEL");

    // ---- the wide path: at most 2^31 - 1 rows per call (FZ_E_BADARG).  Its entries take HOST arrays and copy them: with the stub's
    // copies touching nothing and its large allocations backed by one byte, a call at the limit reaches the launch with dummies.
    // fz_wide_pw_host and fz_wide_matvec_host state no count limit: there is nothing to pin for them ----
    { uint64_t tab[2] = {1, 1}; int64_t x[2] = {0, 0}; uint64_t mx[1]; int32_t wt[1];
      g_copy_nothing = true; g_fake_above = (size_t)1 << 30;
      s = snap(); launched_as("wide_ntt rows at 2^31 - 1", fz_wide_ntt_host(0, 12289, 2, tab, 1, 0, x, x, 0x7fffffffull), s, "wide_ntt_kernel", {0x7fffffffull});
      g_label = "wide_ntt rows at 2^31 - 1"; CHECK(g_launches.back().grid.x == (1u << 20));
      s = snap(); launched_as("wide_norm_weight rows at 2^31 - 1", fz_wide_norm_weight_host(0, x, 0x7fffffffull, 2, mx, wt), s, "wide_norm_weight_kernel", {0x7fffffffull});
      g_label = "wide_norm_weight rows at 2^31 - 1"; CHECK(g_launches.back().grid.x == (1u << 20));
      g_copy_nothing = false; g_fake_above = 0;
      s = snap(); refused("wide_ntt rows at 2^31", fz_wide_ntt_host(0, 12289, 2, tab, 1, 0, x, x, 0x80000000ull), FZ_E_BADARG, s);
      s = snap(); refused("wide_norm_weight rows at 2^31", fz_wide_norm_weight_host(0, x, 0x80000000ull, 2, mx, wt), FZ_E_BADARG, s); }

    long a = 0, e = 0, st = 0;
    stub_live(&a, &e, &st);
    g_label = "nothing left allocated"; CHECK(a == 0 && e == 0 && st == 0);
    printf(g_fail ? "FAILED %d\n" : "ALL OK\n", g_fail);
    return g_fail ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def refusals(tmp_path_factory):
    """the driver's output: one "ok <label>" line per pinned side of a limit"""
    tmp = tmp_path_factory.mktemp("far_refusals")
    san = "-fsanitize=address,undefined"                                    # (as tests/test_context_host.py: no build without them)
    exe = build_driver(tmp, UNITS, DRIVER, san, name="far_refusals", sources=[os.path.join(CSRC, "fz_host.cpp")],
                       flags=["-fno-sanitize-recover=all"], late_text=fatbin_definitions)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=dict(os.environ, FZ_POOL_MB="0"))
    return r


LIMITS = [
    "groups aggregate_partial_batch", "groups aggregate_target_partial_batch", "groups sign_aggregate_target_partial_batch",
    "groups target_partial_batch", "groups verify_with_target_batch_async", "groups verify_partials_batch_async",
    "N aggregate_core", "N aggregate_partial", "N aggregate_core_ragged group", "total aggregate_core_ragged",
    "rows*degree encode_records", "rows*degree decode_records", "rows*degree check_records", "rows*degree sign_encoded",
    "records product encode_records", "N aggregate_encoded", "N aggregate_encoded_ragged group", "total aggregate_encoded_ragged",
    "rows*degree keygen_records", "N keygen_records", "l verify_encoded", "batch*2 keygen_core", "batch*2 keygen_core_bcast", "blocks matvec", "multi rows",
    "waves1 ntt_forward degree 256", "waves1 ntt_inverse degree 256", "waves1 ntt_forward degree 64",
    "wide_ntt rows", "wide_norm_weight rows", "threads fill_synthetic",
]


def test_refusal_driver_runs_clean(refusals):
    assert refusals.returncode == 0 and "ALL OK" in refusals.stdout, refusals.stdout[-4000:] + refusals.stderr[-4000:]
    assert "sanitizers: address on" in refusals.stdout.splitlines()
    assert "FAIL" not in refusals.stdout


@pytest.mark.parametrize("limit", LIMITS)
def test_limit_is_pinned_on_both_sides(limit, refusals):
    sides = [ln for ln in refusals.stdout.splitlines() if ln.startswith("ok " + limit + " ")]
    assert len(sides) >= 2, "%s: %s" % (limit, sides)


@pytest.mark.parametrize("label", ["multi flush at a full table", "multi flush at total + tasks > 0x7fffffff",
                                   "groups verify_with_target_batch at 65536"])
def test_flushes_and_one_sided_refusals(label, refusals):
    assert "ok " + label in refusals.stdout.splitlines()
