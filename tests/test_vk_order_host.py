"""The device key sort of hash_ag for many committees (csrc/fz_vk_order.hip, its entries csrc/fz_vk_order_capi.hip and
fz_challenge_hat_msgs_keep_dev of csrc/fz_staged_capi.hip; BatchScheme(key_sort=...)) without a GPU.

* The comparator.  csrc/fz_vk_order_key.h is host-callable: a stand-alone driver links the entries against the stub HIP runtime of
  tests/_hip_stub.py, and its stand-in for the sort's launcher runs the kernel's algorithm -- rank by counting with fz_vk_text_key
  and fz_vk_text_cmp, reading the staged group table and mask -- on the host.  Its order is checked against Python's
  sorted(key=str) of the keys' text on the trap list: values whose decimals are prefixes of each other inside a row and at a
  row's end, negative values, both ends of int32, differences at several positions of either row, identical keys.
* The three entries' argument rules in their order, and that a refused call reaches neither the runtime nor a launcher.
* The kernel's resources: no spill, no scratch, no LDS, no atomic.
* BatchScheme on the stand-in context of tests/_scheme_buffers.py: key_sort="device" calls no host sort, downloads neither keys nor
  digests and uploads no digests in any many-committee method; key_sort="host" makes, call for call, the calls recorded from the
  code before the option existed (tests/golden/vk_order_host_calls.json)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from _hip_stub import CSRC, STUB, build_driver

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vk_order_host_calls.json")
Q = 2147465729
TRAPS = [0, 1, 10, 12, 123, -1, -12, -123, 9, -9, 2147483647, -2147483648, (Q - 1) // 2, -(Q - 1) // 2]

DRIVER_BODY = r'''
#include "fz_vk_order_key.h"
#include <cstdarg>
static int g_sort = 0, g_hash = 0, g_ntt = 0, g_chal = 0;
static std::string g_last;
static bool g_wave_ok = true;
static const uint8_t *g_pre_arg = nullptr;              // the caller's digest buffer: how the stand-ins name a pointer into it
static std::string pre_name(const uint8_t *p) {
    if (!p) return "0";
    if (g_pre_arg && p >= g_pre_arg && p < g_pre_arg + (1 << 20)) return "arg+" + std::to_string((size_t)(p - g_pre_arg));
    return "other";
}
bool fz_challenge_wave_ok(const fz_scheme_params *P) { return g_wave_ok && P->omega_ch <= 64 && P->degree <= 256 && P->degree >= 4; }
void fz_challenge_weight_table(int, int degree, uint32_t *t) { memset(t, 0, (size_t)(degree + 1) * 16 * 4); }
void fz_mt_init_table(uint32_t *tab) { memset(tab, 0, 624 * 4); }
int fz_launch_mt_sample(fz_ctx *, const unsigned long long *, size_t, int, uint32_t, int, const uint32_t *, int32_t *, int *, uint32_t *) { return FZ_OK; }
int fz_launch_ntt(fz_ctx *, const int32_t *, int32_t *, size_t, bool) { ++g_ntt; return FZ_OK; }
int fz_launch_vk_halves(fz_ctx *, const int32_t *, size_t, int, int32_t *, int32_t *) { return FZ_OK; }
int fz_launch_challenge_wave(fz_ctx *, const fz_scheme_params *, const int32_t *, const uint8_t *pre, const uint8_t *, const unsigned long long *, uint8_t *pre_out,
                             size_t N, size_t, int, const uint32_t *, int32_t *) {
    ++g_chal;
    g_last += " wave(pre=" + pre_name(pre) + " pre_out=" + pre_name(pre_out) + " N=" + std::to_string(N) + ")";
    return FZ_OK;
}
int fz_launch_prehash(fz_ctx *, const fz_scheme_params *, const uint8_t *, const unsigned long long *, size_t N, uint8_t *pre, uint32_t *) {
    ++g_chal;
    g_last += " prehash(pre=" + pre_name(pre) + " N=" + std::to_string(N) + ")";
    return FZ_OK;
}
int fz_launch_challenge(fz_ctx *, const fz_scheme_params *, const int32_t *, const uint8_t *pre, const uint32_t *, size_t N, uint8_t *, size_t, int *, uint32_t *,
                        size_t, int, const uint32_t *, int32_t *) {
    ++g_chal;
    g_last += " challenge(pre=" + pre_name(pre) + " N=" + std::to_string(N) + ")";
    return FZ_OK;
}
// the sort kernel's algorithm on the host: rank = rows of the committee that compare less + equal rows with a smaller index
int fz_launch_vk_order(fz_ctx *, const int32_t *vk, int d, const void *grp, size_t G, const uint8_t *valid, uint32_t *order) {
    ++g_sort;
    const uint32_t *g = (const uint32_t *)grp;
    g_last += " sort:";
    for (size_t k = 0; k < G; ++k) {
        const uint32_t first = g[4 * k], n = g[4 * k + 1], at = g[4 * k + 2];
        g_last += " (" + std::to_string(first) + "+" + std::to_string(n) + "@" + std::to_string(at) + ")";
        const int32_t *base = vk + (size_t)first * 2 * d;
        for (uint32_t i = 0; i < n; ++i) {
            if (valid && !valid[first + i]) continue;
            uint32_t rank = 0;
            const uint64_t ki = fz_vk_text_key(base[(size_t)i * 2 * d], false);
            for (uint32_t j = 0; j < n; ++j) {
                if (valid && !valid[first + j]) continue;
                const uint64_t kj = fz_vk_text_key(base[(size_t)j * 2 * d], false);
                if (kj < ki) ++rank;
                else if (kj == ki && j != i) {
                    const int c = fz_vk_text_cmp(base + (size_t)j * 2 * d, base + (size_t)i * 2 * d, d);
                    rank += (c < 0 || (c == 0 && j < i)) ? 1u : 0u;
                }
            }
            order[at + rank] = first + i;
        }
    }
    return FZ_OK;
}
int fz_launch_hash_ag(fz_ctx *, const fz_scheme_params *, const int32_t *, const uint8_t *, const int32_t *, const uint32_t *ord, const void *grp,
                      size_t G, const uint32_t *, int32_t *) {
    ++g_hash;
    const uint32_t *g = (const uint32_t *)grp;
    g_last += " hash:";
    for (size_t k = 0; k < G; ++k) {
        g_last += " (" + std::to_string(g[2 * k]) + "+" + std::to_string(g[2 * k + 1]) + ":";
        for (uint32_t i = 0; i < g[2 * k + 1]; ++i) g_last += " " + std::to_string(ord[g[2 * k] + i]);
        g_last += ")";
    }
    return FZ_OK;
}

static fz_scheme_params params(int secpar, int degree, int64_t root, int64_t inv_root, int w_ch, int w_ag) {
    fz_scheme_params P;
    memset(&P, 0, sizeof(P));
    P.modulus = 2147465729; P.root = root; P.inv_root = inv_root; P.degree = degree; P.root_order = 2 * degree; P.secpar = secpar;
    P.omega_ch = w_ch; P.omega_ag = w_ag; P.beta_ch = 1; P.beta_ag = 1;
    P.agg_xof_dst[0] = '3'; P.agg_xof_dst[1] = '2';
    P.sign_pre_hash_dst[0] = '0'; P.sign_pre_hash_dst[1] = '0'; P.sign_hash_dst[0] = '0'; P.sign_hash_dst[1] = '1';
    return P;
}
static int g_fail = 0;
static void report(const char *what, int rc, int want_rc, size_t mark, int s0, int h0, int n0, int c0) {
    size_t enq = 0, syncs = 0, d2h = 0;
    for (const Call &k : stub_log(mark)) {
        enq += k.fn != "hipSetDevice" && k.fn != "hipStreamIsCapturing";
        syncs += k.fn == "hipStreamSynchronize";
        d2h += k.kind == (int)hipMemcpyDeviceToHost;
    }
    printf("[%s] -> rc=%d", what, rc);
    if (rc != FZ_OK) printf(" \"%s\"", fz_last_error());
    printf(" sorts=%d hashes=%d transforms=%d challenge=%d syncs=%zu d2h=%zu%s\n", g_sort - s0, g_hash - h0, g_ntt - n0, g_chal - c0, syncs, d2h, g_last.c_str());
    if (rc != want_rc) { printf("FAIL: code %d expected\n", want_rc); ++g_fail; }
    if (rc != FZ_OK && (enq || g_sort != s0 || g_hash != h0 || g_ntt != n0 || g_chal != c0)) { printf("FAIL: a refused call reached the runtime or a launcher\n"); ++g_fail; }
}
#define RUN(what, want, call) do { const size_t mark_ = stub_mark(); const int s0 = g_sort, h0 = g_hash, n0 = g_ntt, c0 = g_chal; g_last.clear(); \
                                   const int rc_ = (call); report(what, rc_, want, mark_, s0, h0, n0, c0); } while (0)

struct Args {
    fz_ctx *ctx; fz_scheme_params P; bool noP;
    int32_t *vk; uint8_t *pre; int32_t *c, *al; uint32_t *ord;
    size_t N, G;
    std::vector<size_t> off; std::vector<uint8_t> valid;
    bool no_off;
};
static int sort_of(const Args &a) {
    return fz_sort_by_vk_string_ragged_dev(a.ctx, a.noP ? nullptr : &a.P, a.vk, a.N, a.no_off ? nullptr : a.off.data(), a.G,
                                           a.valid.empty() ? nullptr : a.valid.data(), a.ord);
}
static int sorted_of(const Args &a) {
    return fz_hash_ag_ragged_sorted_dev(a.ctx, a.noP ? nullptr : &a.P, a.vk, a.pre, a.c, a.N, a.no_off ? nullptr : a.off.data(), a.G,
                                        a.valid.empty() ? nullptr : a.valid.data(), a.al);
}

static int rules() {
    const uint32_t Q = 2147465729u;
    fz_ctx *c = nullptr, *ring = nullptr;
    if (fz_ctx_create(0, Q, 256, 3337519u, 1978410468u, &c) != FZ_OK) { printf("FAIL context: %s\n", fz_last_error()); return 2; }
    if (fz_ctx_create(0, Q, 256, 0, 0, &ring) != FZ_OK) { printf("FAIL ring context: %s\n", fz_last_error()); return 2; }
    alignas(64) static int32_t vk[6 * 2 * 256], chat[6 * 256], alpha[6 * 256];
    alignas(64) static uint8_t pre[1 << 20];
    alignas(64) static uint32_t ord[16];
    for (int i = 0; i < 6; ++i) vk[i * 512] = 5 - i;             // row i's first coefficient: rows sort in reverse
    vk[3 * 512] = vk[4 * 512];                                   // ... rows 3 and 4 are one key: they keep their order
    g_pre_arg = pre;
    Args good{c, params(256, 256, 3337519, 1978410468, 60, 60), false, vk, pre, chat, alpha, ord, 6, 3, {0, 2, 3, 6}, {}, false};
    // ---- fz_sort_by_vk_string_ragged_dev ----
    RUN("sort good", FZ_OK, sort_of(good));
    printf("[sort good order] -> %u %u %u %u %u %u\n", ord[0], ord[1], ord[2], ord[3], ord[4], ord[5]);
    { Args a = good; a.valid = {1, 0, 0, 1, 0, 1}; for (auto &x : ord) x = 99; RUN("sort masked", FZ_OK, sort_of(a));
      printf("[sort masked order] -> %u %u %u %u\n", ord[0], ord[1], ord[2], ord[3]); }
    { Args a = good; a.off = {0, 2, 2, 6}; RUN("sort empty group", FZ_OK, sort_of(a)); }
    { Args a = good; a.ctx = nullptr; RUN("sort ctx", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.noP = true; RUN("sort params", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.vk = nullptr; RUN("sort null vk", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.ord = nullptr; RUN("sort null order", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.no_off = true; RUN("sort null off", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.P.degree = 64; RUN("sort foreign params", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.vk += 2; RUN("sort misaligned vk", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.ord = (uint32_t *)((char *)a.ord + 2); RUN("sort misaligned order", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; c->capturing = 1; RUN("sort capture", FZ_E_BADARG, sort_of(a)); c->capturing = 0; }
    { Args a = good; a.N = (size_t)1 << 31; RUN("sort N 2^31", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.off = {1, 2, 3, 6}; RUN("sort off from 1", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.off = {0, 3, 2, 6}; RUN("sort off decreasing", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.off = {0, 2, 3, 5}; RUN("sort off short", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.vk += 2; a.off = {1, 2, 3, 6}; RUN("sort misaligned before offsets", FZ_E_BADARG, sort_of(a)); }
    { Args a = good; a.G = 0; a.no_off = true; RUN("sort G = 0", FZ_OK, sort_of(a)); }
    { Args a = good; a.N = 0; a.G = 0; a.vk = nullptr; a.ord = nullptr; a.no_off = true; RUN("sort N = 0", FZ_OK, sort_of(a)); }
    // ---- fz_hash_ag_ragged_sorted_dev ----
    RUN("sorted good", FZ_OK, sorted_of(good));
    { Args a = good; a.off = {0, 1, 2, 6}; RUN("sorted longest first", FZ_OK, sorted_of(a)); }
    { Args a = good; a.valid = {1, 0, 0, 1, 0, 1}; RUN("sorted masked", FZ_OK, sorted_of(a)); }
    { Args a = good; a.valid = {0, 0, 0, 0, 0, 0}; RUN("sorted none valid", FZ_OK, sorted_of(a)); }
    { Args a = good; a.off = {0, 2, 3, 5}; RUN("sorted fewer than N", FZ_OK, sorted_of(a)); }
    { Args a = good; a.ctx = nullptr; RUN("sorted ctx", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.noP = true; RUN("sorted params", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.vk = nullptr; RUN("sorted null vk", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.pre = nullptr; RUN("sorted null pre", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.c = nullptr; RUN("sorted null c_hat", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.al = nullptr; RUN("sorted null alpha", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.no_off = true; RUN("sorted null off", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.P.degree = 64; RUN("sorted foreign params", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.vk += 2; RUN("sorted misaligned vk", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.pre += 2; RUN("sorted misaligned pre", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; c->capturing = 1; RUN("sorted capture", FZ_E_BADARG, sorted_of(a)); c->capturing = 0; }
    { Args a = good; a.off = {1, 2, 3, 6}; RUN("sorted off from 1", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.off = {0, 3, 2, 6}; RUN("sorted off decreasing", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.off = {0, 2, 2, 6}; RUN("sorted empty group", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.N = 4; RUN("sorted more rows than N", FZ_E_BADARG, sorted_of(a)); }
    { Args a = good; a.vk += 2; c->capturing = 1; RUN("sorted misaligned before capture", FZ_E_BADARG, sorted_of(a)); c->capturing = 0; }
    { Args a = good; a.P.beta_ag = 2; RUN("sorted beta_ag 2", FZ_E_UNSUPPORTED, sorted_of(a)); }
    { Args a = good; a.P.omega_ag = 65; RUN("sorted omega_ag 65", FZ_E_UNSUPPORTED, sorted_of(a)); }
    { Args a = good; a.ctx = ring; RUN("sorted ring-only context", FZ_E_UNSUPPORTED, sorted_of(a)); }
    { Args a = good; a.G = 0; a.no_off = true; RUN("sorted G = 0", FZ_OK, sorted_of(a)); }
    { Args a = good; a.N = 0; a.G = 0; a.vk = nullptr; a.pre = nullptr; a.c = a.al = nullptr; a.no_off = true; RUN("sorted N = 0", FZ_OK, sorted_of(a)); }
    // ---- fz_challenge_hat_msgs_keep_dev ----
    const char msgs[] = "abcde";
    std::vector<size_t> moff = {0, 1, 2, 3, 4, 5};
    const fz_scheme_params P = good.P;
    RUN("keep good", FZ_OK, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, moff.data(), 5, chat, pre));
    RUN("keep three kernels by the rule", FZ_OK, (g_wave_ok = false, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, moff.data(), 5, chat, pre)));
    g_wave_ok = true;
    {
        std::vector<size_t> many(4610, 0);                       // 4609 empty messages: beyond the wave form's batch
        g_copy_nothing = true;
        g_fake_above = (size_t)1 << 20;
        RUN("keep 4609", FZ_OK, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, many.data(), 4609, chat, pre));
        RUN("keep 4609 again", FZ_OK, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, many.data(), 4609, chat, pre));
        g_copy_nothing = false;
        g_fake_above = 0;
    }
    RUN("keep null digests", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, moff.data(), 5, chat, nullptr));
    RUN("keep null offsets", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, nullptr, 5, chat, pre));
    RUN("keep misaligned digests", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, moff.data(), 5, chat, pre + 8));
    RUN("keep null ctx", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(nullptr, &P, vk, msgs, moff.data(), 5, chat, pre));
    RUN("keep null vk", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(c, &P, nullptr, msgs, moff.data(), 5, chat, pre));
    { c->capturing = 1; RUN("keep capture", FZ_E_BADARG, fz_challenge_hat_msgs_keep_dev(c, &P, vk, msgs, moff.data(), 5, chat, pre)); c->capturing = 0; }
    RUN("keep N = 0", FZ_OK, fz_challenge_hat_msgs_keep_dev(c, &P, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    RUN("digests to the host still wait", FZ_OK, fz_challenge_hat_msgs_dev(c, &P, vk, msgs, moff.data(), 5, chat, pre));
    fz_ctx_destroy(c);
    fz_ctx_destroy(ring);
    fz_ctx *odd = nullptr;                                       // a degree the sort does not take
    if (fz_ctx_create(0, Q, 12, 0, 0, &odd) == FZ_OK) {
        Args a = good; a.ctx = odd; a.P.degree = 12; a.P.root_order = 24;
        RUN("sort degree 12", FZ_E_UNSUPPORTED, sort_of(a));
        fz_ctx_destroy(odd);
    } else { printf("FAIL context of degree 12: %s\n", fz_last_error()); ++g_fail; }
    long al = 0, ev = 0, st = 0;
    stub_live(&al, &ev, &st);
    if (al || ev || st) { printf("FAIL: something is left allocated (%ld %ld %ld)\n", al, ev, st); ++g_fail; }
    return g_fail;
}

// argv[2]: a file of int64 d, N, G, masked; G + 1 int64 offsets; N mask bytes when masked; N * 2 * d int32 values.  The order the
// entry leaves, through the stand-in sort above, goes to stdout; entries behind the last valid row must keep their sentinel.
static int sort_file(const char *path) {
    FILE *fh = fopen(path, "rb");
    if (!fh) return 2;
    long long head[4];
    if (fread(head, 8, 4, fh) != 4) return 2;
    const int d = (int)head[0];
    const size_t N = (size_t)head[1], G = (size_t)head[2];
    std::vector<long long> off64(G + 1);
    if (fread(off64.data(), 8, G + 1, fh) != G + 1) return 2;
    std::vector<size_t> off(off64.begin(), off64.end());
    std::vector<uint8_t> valid(head[3] ? N : 0);
    if (head[3] && fread(valid.data(), 1, N, fh) != N) return 2;
    std::vector<int32_t> raw(N * 2 * d + 16);
    int32_t *vk = (int32_t *)(((uintptr_t)raw.data() + 63) & ~(uintptr_t)63);
    if (fread(vk, 4, N * 2 * d, fh) != N * 2 * d) return 2;
    fclose(fh);
    fz_ctx *c = nullptr;
    if (fz_ctx_create(0, 2147465729u, d, 0, 0, &c) != FZ_OK) { printf("FAIL context: %s\n", fz_last_error()); return 2; }
    fz_scheme_params P = params(128, d, 0, 0, d < 60 ? d : 60, d < 60 ? d : 60);
    std::vector<uint32_t> ord(N + 4, 0xfffffff0u);
    const int rc = fz_sort_by_vk_string_ragged_dev(c, &P, vk, N, off.data(), G, head[3] ? valid.data() : nullptr, ord.data());
    if (rc != FZ_OK) { printf("FAIL sort: %s\n", fz_last_error()); return 1; }
    size_t M = N;
    if (head[3]) { M = 0; for (uint8_t v : valid) M += v != 0; }
    printf("order:");
    for (size_t i = 0; i < M; ++i) printf(" %u", ord[i]);
    printf("\n");
    for (size_t i = M; i < ord.size(); ++i)
        if (ord[i] != 0xfffffff0u) { printf("FAIL: entry %zu behind the last valid row was written\n", i); ++g_fail; }
    fz_ctx_destroy(c);
    return g_fail;
}

int main(int argc, char **argv) {
    const int bad = argc > 2 ? sort_file(argv[2]) : rules();
    printf(bad ? "FAILED %d\n" : "ALL OK\n", bad);
    return bad ? 1 : 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("vk_order_entry")
    exe = build_driver(tmp, ("fz_vk_order_capi", "fz_hash_ag_capi", "fz_staged_capi", "fz_context", "fz_diag"), STUB + DRIVER_BODY,
                       "-fsanitize=address,undefined", name="vk_order_entry", sources=[os.path.join(CSRC, "fz_host.cpp")],
                       flags=["-fno-sanitize-recover=all"])
    return tmp, exe


def _run(exe, *args):
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=dict(os.environ, FZ_POOL_MB="0"))
    assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.fixture(scope="module")
def lines(driver):
    out = _run(driver[1], "rules")
    return {ln[1:ln.index("]")]: ln[ln.index("]") + 5:] for ln in out.splitlines() if ln.startswith("[")}


# ---- the comparator, against sorted(key=str) -----------------------------------------------------------------------------------------
def text_of(row):
    """what decides the order of str(vk): the two rows' values as the text prints them, fixed text between them"""
    return "values=%s)]])" % list(map(int, row[0])) + ", right_vk_hat=values=%s)" % list(map(int, row[1]))


def trap_keys(d, rng):
    """one committee per position (left row's 0, 1, 7, 8, d - 2, d - 1; right row's 0, d - 1): keys equal everywhere but there, where
    they take every trap value; then committees with 2, 3 and 5 identical keys among distinct ones"""
    groups = []
    base = rng.integers(-50, 50, size=(2, d)).astype(np.int64)
    for half, pos in [(0, 0), (0, 1), (0, min(7, d - 1)), (0, min(8, d - 1)), (0, d - 2), (0, d - 1), (1, 0), (1, d - 1)]:
        rows = np.repeat(base[None], len(TRAPS), axis=0)
        rows[:, half, pos] = TRAPS
        groups.append(rows[rng.permutation(len(TRAPS))])
    for same in (2, 3, 5):
        rows = np.repeat(base[None], same + 4, axis=0)
        rows[same:, 0, 0] = [12, 123, -12, 1]
        groups.append(rows[rng.permutation(same + 4)])
    return groups


def _write(path, d, groups, valid=None):
    vk = np.concatenate(groups).astype(np.int32)
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int64)
    with open(path, "wb") as fh:
        fh.write(struct.pack("<4q", d, vk.shape[0], len(groups), 0 if valid is None else 1))
        fh.write(off.tobytes())
        if valid is not None:
            fh.write(np.asarray(valid, dtype=np.uint8).tobytes())
        fh.write(np.ascontiguousarray(vk).tobytes())
    return vk, off


def _want(vk, off, valid=None):
    out = []
    for a, b in zip(off[:-1], off[1:]):
        rows = [i for i in range(a, b) if valid is None or valid[i]]
        out += sorted(rows, key=lambda i: text_of(vk[i]))
    return out


@pytest.mark.parametrize("d", [4, 64, 256])
def test_comparator_is_the_text_order_on_the_trap_list(driver, d):
    tmp, exe = driver
    rng = np.random.default_rng(d)
    groups = trap_keys(d, rng)
    groups.append(rng.integers(-2 ** 31, 2 ** 31, size=(130, 2, d)))          # a committee of three tiles, decided on coefficient 0
    vk, off = _write(tmp / f"traps{d}.bin", d, groups)
    got = [int(x) for x in _run(exe, "sort", tmp / f"traps{d}.bin").split("order:")[1].split("\n")[0].split()]
    assert got == _want(vk, off)
    # the rule the text states: inside a row "12" sorts before "123", at a row's end after it; "-" before every digit
    for g, flipped in ((0, False), (5, True), (7, True)):
        rows = got[off[g]:off[g + 1]]
        half, pos = (0, 0) if g == 0 else ((0, d - 1) if g == 5 else (1, d - 1))
        vals = [int(vk[i, half, pos]) for i in rows]
        assert (vals.index(123) < vals.index(12)) == flipped and vals.index(-1) < vals.index(0), (g, vals)


def test_mask_compacts_every_group_and_writes_nothing_behind(driver):
    tmp, exe = driver
    rng = np.random.default_rng(7)
    groups = trap_keys(64, rng)[:4] + [rng.integers(-9, 9, size=(70, 2, 64))]
    n = sum(len(g) for g in groups)
    valid = rng.integers(0, 2, size=n).astype(np.uint8)
    a, b, c = len(groups[0]), len(groups[0]) + len(groups[1]), len(groups[0]) + len(groups[1]) + len(groups[2])
    valid[:a] = 0                                                            # a group with no valid row
    valid[a:b] = 0
    valid[b - 1] = 1                                                         # only its last row
    valid[b:c] = 1                                                           # every row
    vk, off = _write(tmp / "masked.bin", 64, groups, valid)
    got = [int(x) for x in _run(exe, "sort", tmp / "masked.bin").split("order:")[1].split("\n")[0].split()]
    assert got == _want(vk, off, valid)


def test_key_is_monotone_in_the_text(driver):
    """fz_vk_text_key through the driver: a committee whose keys differ at coefficient 0 alone sorts like the decimals with ", "
    behind them, for every pair of trap values and their neighbours"""
    tmp, exe = driver
    vals = sorted({v + e for v in TRAPS for e in (-1, 0, 1) if -2 ** 31 <= v + e < 2 ** 31} | {99, 100, 101, 999999999, 1000000000, -1000000000})
    rows = np.zeros((len(vals), 2, 4), dtype=np.int64)
    rows[:, 0, 0] = vals
    vk, off = _write(tmp / "mono.bin", 4, [rows])
    got = [int(x) for x in _run(exe, "sort", tmp / "mono.bin").split("order:")[1].split("\n")[0].split()]
    assert [vals[i] for i in got] == sorted(vals, key=lambda v: str(v) + ", ")


# ---- the entries' rules ---------------------------------------------------------------------------------------------------------------
def test_sort_entry_stages_the_groups_and_sorts(lines):
    assert lines["sort good"] == "rc=0 sorts=1 hashes=0 transforms=0 challenge=0 syncs=0 d2h=0 sort: (0+2@0) (2+1@2) (3+3@3)"
    assert lines["sort good order"] == "1 0 2 5 3 4"                        # rows 3 and 4 hold one key: the callers' order
    assert lines["sort masked"].endswith("sort: (0+2@0) (3+3@1)")           # the group without a valid row is not handed out
    assert lines["sort masked order"] == "0 5 3 99"
    assert lines["sort empty group"].endswith("sort: (0+2@0) (2+4@2)")


def test_sort_entry_refusals_in_their_order(lines):
    none = " sorts=0 hashes=0 transforms=0 challenge=0 syncs=0 d2h=0"
    for what in ("sort ctx", "sort params", "sort null vk", "sort null order", "sort null off"):
        assert lines[what] == 'rc=-1 "NULL argument"' + none, what
    assert "do not belong to this context" in lines["sort foreign params"]
    assert lines["sort misaligned vk"] == 'rc=-1 "misaligned device pointer"' + none == lines["sort misaligned order"]
    assert "not during graph capture" in lines["sort capture"]
    assert "fewer than 2^31 each" in lines["sort N 2^31"]
    assert 'rc=-1 "offsets must start at 0 (got 1)"' in lines["sort off from 1"]
    assert 'rc=-1 "offsets must not decrease (group 1)"' in lines["sort off decreasing"]
    assert 'rc=-1 "offsets end at 5 for 6 rows"' in lines["sort off short"]
    assert "misaligned" in lines["sort misaligned before offsets"]
    assert lines["sort degree 12"].startswith('rc=-2 "device key sort: degree 4..256, a power of two, only')
    assert lines["sort G = 0"] == "rc=0" + none == lines["sort N = 0"]
    for what, ln in lines.items():
        if not ln.startswith("rc=0") and not what.endswith("order"):
            assert ln.endswith(none), what


def test_sorted_entry_sorts_then_hashes_that_order(lines):
    # (a context's first call allocates the decoder's table and the order list's scratch, draining the stream for each; no later one waits)
    assert lines["sorted good"] == ("rc=0 sorts=1 hashes=1 transforms=1 challenge=0 syncs=2 d2h=0 sort: (0+2@0) (2+1@2) (3+3@3)"
                                    " hash: (3+3: 5 3 4) (0+2: 1 0) (2+1: 2)")
    assert lines["sorted longest first"] == ("rc=0 sorts=1 hashes=1 transforms=1 challenge=0 syncs=0 d2h=0 sort: (0+1@0) (1+1@1) (2+4@2)"
                                             " hash: (2+4: 5 3 4 2) (0+1: 0) (1+1: 1)")
    assert lines["sorted masked"].endswith("sort: (0+2@0) (3+3@1) hash: (1+2: 5 3) (0+1: 0)")
    assert lines["sorted none valid"] == "rc=0 sorts=0 hashes=0 transforms=0 challenge=0 syncs=0 d2h=0"
    assert lines["sorted fewer than N"].endswith("hash: (0+2: 1 0) (3+2: 3 4) (2+1: 2)")


def test_sorted_entry_refusals_are_the_hash_entrys(lines):
    none = " sorts=0 hashes=0 transforms=0 challenge=0 syncs=0 d2h=0"
    for what in ("ctx", "params", "null vk", "null pre", "null c_hat", "null alpha", "null off"):
        assert lines["sorted " + what] == 'rc=-1 "NULL argument"' + none, what
    assert "do not belong to this context" in lines["sorted foreign params"]
    assert lines["sorted misaligned vk"] == 'rc=-1 "misaligned device pointer"' + none == lines["sorted misaligned pre"]
    assert "not during graph capture" in lines["sorted capture"] and "misaligned" in lines["sorted misaligned before capture"]
    assert 'rc=-1 "offsets must start at 0 (got 1)"' in lines["sorted off from 1"]
    assert 'rc=-1 "offsets must not decrease (group 1)"' in lines["sorted off decreasing"]
    assert 'rc=-1 "group 1 is empty"' in lines["sorted empty group"]
    assert 'rc=-1 "offsets end at 6 for 4 rows"' in lines["sorted more rows than N"]
    assert lines["sorted beta_ag 2"].startswith('rc=-2 "device hash_ag: ternary aggregation coefficients (norm bound 1) only')
    assert lines["sorted omega_ag 65"].startswith('rc=-2 "device hash_ag: weight <= min(64, degree)')
    assert lines["sorted ring-only context"].startswith('rc=-2 "ring-only context')
    assert lines["sorted G = 0"] == "rc=0" + none                           # (N zero rows: the clear alone)
    assert lines["sorted N = 0"] == "rc=0" + none


def test_keep_entry_leaves_the_digests_on_the_device_and_waits_for_nothing(lines):
    assert lines["keep good"] == "rc=0 sorts=0 hashes=0 transforms=1 challenge=1 syncs=0 d2h=0 wave(pre=0 pre_out=arg+0 N=5)"
    # the three-kernel path writes them there as well, and reads them from there: one synchronisation (the upload: the caller's
    # messages have been consumed) and no download; a call that grows the scratch drains the stream for that once more
    for what, n, syncs in (("keep three kernels by the rule", 5, 2), ("keep 4609", 4609, 2), ("keep 4609 again", 4609, 1)):
        assert lines[what] == (f"rc=0 sorts=0 hashes=0 transforms=1 challenge=2 syncs={syncs} d2h=0 prehash(pre=arg+0 N={n})"
                               f" challenge(pre=arg+0 N={n})"), what
    assert lines["digests to the host still wait"] == "rc=0 sorts=0 hashes=0 transforms=1 challenge=1 syncs=1 d2h=0 wave(pre=0 pre_out=other N=5)"
    none = " sorts=0 hashes=0 transforms=0 challenge=0 syncs=0 d2h=0"
    for what in ("keep null digests", "keep null offsets", "keep null ctx", "keep null vk"):
        assert lines[what] == 'rc=-1 "NULL argument"' + none, what
    assert lines["keep misaligned digests"] == 'rc=-1 "misaligned device pointer"' + none
    assert "not during graph capture" in lines["keep capture"]
    assert lines["keep N = 0"] == "rc=0" + none


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
def test_kernel_compiles_without_spills_scratch_lds_or_atomics():
    import __graft_entry__ as GE
    from _isa import asm, bodies, metadata
    assert "fz_vk_order.hip" in GE.SOURCES and "fz_vk_order_capi.hip" in GE.SOURCES
    kernels = metadata(asm("fz_vk_order"), "vk_order_wave_kernel")
    assert len(kernels) == 1, sorted(kernels)
    for name, f in list(kernels.items()) + list(metadata(asm("fz_vk_order"), "vk_halves_kernel").items()):
        assert f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0 and f["private_segment_fixed_size"] == 0 and f["lds"] == 0, (name, f)
    for name, ins in bodies(asm("fz_vk_order"), "vk_order_wave_kernel").items():
        assert not [i for i in ins if "atomic" in i or i.startswith(("scratch_", "ds_"))], name
        assert [i for i in ins if i.startswith("v_readlane_b32")], "the tile's keys no longer reach the lanes as scalars"
        assert [i for i in ins if i.startswith("global_load_dwordx4")], "the walk past coefficient 0 no longer loads four values at a time"


def test_hash_and_challenge_kernels_are_untouched():
    for unit in ("fz_hash_ag.hip", "fz_challenge.hip"):
        assert "fz_vk_order" not in open(os.path.join(CSRC, unit)).read()


# ---- BatchScheme(key_sort=...) on the stand-in context ------------------------------------------------------------------------------------
MANY = {
    "aggregate_many": lambda bs, a, M, S: bs.aggregate_many(a["vk"], M, a["sig"], S),
    "verify_many": lambda bs, a, M, S: bs.verify_many(a["vk"], M, a["aggs"], S),
    "verify_many_encoded": lambda bs, a, M, S: bs.verify_many_encoded(a["vk"], M, a["aggrecs"], S),
    "aggregate_many_encoded": lambda bs, a, M, S: bs.aggregate_many_encoded(a["vk"], M, a["recs"], S),
    "aggregate_many_encoded[screened]": lambda bs, a, M, S: bs.aggregate_many_encoded(a["vk"], M, a["recs"], S, screened=True),
    "aggregate_verify_many_encoded": lambda bs, a, M, S: bs.aggregate_verify_many_encoded(a["vk"], M, a["recs"], S),
    "hash_ag_many_dev": lambda bs, a, M, S: bs.hash_ag_many_dev(a["vk"], M, S),
}


def _stand_in(monkeypatch, hash_ag, key_sort, keys):
    import fusion.fusion as F
    from _scheme_buffers import host_inputs, no_finalizers, scheme_on, stand_in_context
    from fusion_hip.context import DeviceArray
    params = F.fusion_setup(128, 1)
    no_finalizers(monkeypatch)
    ctx = stand_in_context(params)
    bs = scheme_on(ctx, params)
    bs.hash_ag = hash_ag
    if key_sort is not None:
        bs.key_sort = key_sort
    a = host_inputs(params)
    if keys == "device":
        a["vk"] = DeviceArray.from_numpy(ctx, a["vk"])
    del ctx.calls[:]
    return params, ctx, bs, a


def test_option_is_validated_and_defaults_to_host():
    import inspect
    import fusion.fusion as F
    from fusion_hip import scheme
    from fusion_hip._lib import FZ_E_BADARG, FusionHipError
    assert inspect.signature(scheme.BatchScheme.__init__).parameters["key_sort"].default == "host"
    assert scheme.BatchScheme.key_sort == "host"
    for bad in ("gpu", "auto", None):
        with pytest.raises(FusionHipError) as e:
            scheme.BatchScheme(F.fusion_setup(128, 1), hash_ag="device", key_sort=bad)
        assert e.value.code == FZ_E_BADARG and "key_sort" in str(e.value)
    for fn in (F.aggregate_many_from_bytes, F.verify_many_from_bytes, F.aggregate_verify_many_from_bytes):
        assert inspect.signature(fn).parameters["key_sort"].default == "host"


@pytest.mark.parametrize("keys", ["host", "device"])
@pytest.mark.parametrize("name", sorted(MANY))
def test_device_sort_downloads_no_keys_and_no_digests(name, keys, monkeypatch):
    from _scheme_buffers import MESSAGES, N, SIZES
    from fusion_hip import hostpipe
    params, ctx, bs, a = _stand_in(monkeypatch, "device", "device", keys)
    for fn in ("sort_by_vk_string", "sort_by_vk_string_ragged", "aggregation_coefficients"):
        monkeypatch.setattr(hostpipe, fn, lambda *x, _fn=fn, **k: pytest.fail(f"hostpipe.{_fn} ran"))
    before = dict(ctx.ledger.live)
    result = MANY[name](bs, a, MESSAGES, SIZES)
    assert ctx.ledger.settle(before, result) == []
    d = params.degree
    entry = [c for c in ctx.calls if c[0] == "hash_ag_ragged_sorted_dev"]
    assert len(entry) == 1 and entry[0][5] == N and not [c for c in ctx.calls if c[0] == "hash_ag_ragged_dev"], ctx.calls
    assert len([c for c in ctx.calls if c[0] == "challenge_msgs_keep_dev"]) == 1 and not [c for c in ctx.calls if c[0] == "challenge_msgs_dev"]
    down = [c[2:] for c in ctx.calls if c[0] == "d2h"]
    assert ("int32", (N, 2, d)) not in down, "the keys were downloaded"
    assert ("uint8", (N, 32)) not in down, "the digests were downloaded"
    assert ("int32", (N, d)) not in down, "c_hat was downloaded"
    up = [c[2][:2] for c in ctx.calls if c[0] == "h2d"]
    assert ("uint8", (N, 32)) not in up, "the digests were uploaded"
    assert ("int32", (N, 2, d)) in up if keys == "host" else ("int32", (N, 2, d)) not in up
    if keys == "device":
        assert ("int32", (N, d)) not in up, "a half of the keys was uploaded from a host copy"
        if name.startswith("verify_many"):
            assert len([c for c in ctx.calls if c[0] == "vk_halves_dev"]) == 1


@pytest.mark.parametrize("name", sorted(k for k in MANY if k != "hash_ag_many_dev"))
def test_device_sort_changes_nothing_under_the_host_form(name, monkeypatch):
    """key_sort="device" has effect where hash_ag takes its device form only (hash_ag_many_dev always takes it)"""
    from _scheme_buffers import MESSAGES, SIZES
    _, plain, bs, a = _stand_in(monkeypatch, "host", None, "device")
    MANY[name](bs, a, MESSAGES, SIZES)
    _, ctx, bs, a = _stand_in(monkeypatch, "host", "device", "device")
    MANY[name](bs, a, MESSAGES, SIZES)
    assert ctx.calls == plain.calls


def test_host_sort_makes_the_calls_it_made_before_the_option(monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    seen = 0
    for form in ("host", "device"):
        for keys in ("host", "device"):
            for name in sorted(MANY):
                for key_sort in (None, "host"):
                    _, ctx, bs, a = _stand_in(monkeypatch, form, key_sort, keys)
                    MANY[name](bs, a, MESSAGES, SIZES)
                    assert json.loads(json.dumps(ctx.calls)) == golden[f"{name}|hash_ag={form}|keys={keys}"], (name, form, keys, key_sort)
                    seen += 1
    assert seen == 2 * len(golden)


@pytest.mark.parametrize("name", sorted(k for k in MANY if k != "hash_ag_many_dev"))
def test_unsupported_falls_back_to_the_host_once_and_stays_there(name, monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES
    params, ctx, bs, a = _stand_in(monkeypatch, "device", "device", "device")
    ctx.unsupported = ("hash_ag_ragged_sorted_dev",)
    before = dict(ctx.ledger.live)
    assert ctx.ledger.settle(before, MANY[name](bs, a, MESSAGES, SIZES)) == []
    assert bs.device_hash_ag is False and sum(c[0] == "hash_ag_ragged_sorted_dev" for c in ctx.calls) == 1
    assert [c for c in ctx.calls if c[0] == "ntt_forward_dev"], "the host form did not finish the call"
    del ctx.calls[:]
    assert ctx.ledger.settle(before, MANY[name](bs, a, MESSAGES, SIZES)) == []
    assert not [c for c in ctx.calls if c[0] in ("hash_ag_ragged_sorted_dev", "challenge_msgs_keep_dev")]


@pytest.mark.parametrize("name", sorted(MANY))
def test_device_sort_frees_every_buffer_when_an_entry_raises(name, monkeypatch):
    from _scheme_buffers import MESSAGES, SIZES
    from fusion_hip._lib import FZ_E_HIP, FusionHipError
    for victim in ("hash_ag_ragged_sorted_dev", "challenge_msgs_keep_dev"):
        params, ctx, bs, a = _stand_in(monkeypatch, "device", "device", "host")

        def boom(*x, **k):
            raise FusionHipError(FZ_E_HIP, "injected")
        setattr(ctx, victim, boom)
        before = dict(ctx.ledger.live)
        with pytest.raises(FusionHipError):
            MANY[name](bs, a, MESSAGES, SIZES)
        assert ctx.ledger.settle(before, None) == []


def test_sort_keys_many_dev_hands_back_the_valid_rows_only(monkeypatch):
    from _scheme_buffers import N, SIZES
    params, ctx, bs, a = _stand_in(monkeypatch, "device", "device", "host")
    before = dict(ctx.ledger.live)
    out = bs.sort_keys_many_dev(a["vk"], SIZES, valid=[True, False, True])
    assert out.shape == (2,) and out.dtype == np.int64 and ctx.ledger.settle(before, None) == []
    call = [c for c in ctx.calls if c[0] == "sort_by_vk_string_ragged_dev"]
    assert len(call) == 1 and call[0][3] == N
    assert bs.sort_keys_many_dev(a["vk"], SIZES, valid=[False] * N).shape == (0,)
    from fusion_hip._lib import FusionHipError
    with pytest.raises(FusionHipError):
        bs.sort_keys_many_dev(a["vk"], [1, 1])
