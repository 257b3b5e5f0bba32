"""The owners of GPU resources (csrc/trx_mem.h) and two of the objects built on them, under AddressSanitizer +
UndefinedBehaviorSanitizer with LeakSanitizer on.  Each case is a stand-alone program with its own main that does NOT link the
HIP runtime: it defines the handful of runtime calls itself, over malloc and counted dummies, with a counter `fail_at` that makes
the k-th allocation or event creation fail.  So every allocation-failure path of create, submit and render runs, and a block or
an event that is lost, freed twice, destroyed while recorded and not waited for, or used after its free shows."""
import os
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "osmo_trx_amd", "csrc")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]

# the runtime calls the host code under test makes, as the runtime declares them
STUBS = r'''
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
static long live_blocks = 0, live_events = 0;     /* allocated and not freed */
static long n_alloc = 0, n_free = 0, n_sync = 0;   /* block allocations, block frees, event waits */
static long n_counted = 0, fail_at = -1;          /* the fail_at-th counted call (from 0) fails */
static bool fired = false;
static long bad = 0;                              /* an event destroyed while recorded and not waited for */
struct stub_event { bool recorded; };
static bool fail_now()
{
    if (n_counted++ != fail_at) return false;
    fired = true;
    return true;
}
static hipError_t stub_alloc(void **p, size_t bytes)
{
    if (fail_now()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    if (!*p) abort();
    memset(*p, 0xa5, bytes);
    live_blocks++; n_alloc++;
    return hipSuccess;
}
static hipError_t stub_free(void *p)
{
    if (p) { free(p); live_blocks--; n_free++; }
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return stub_alloc(p, bytes); }
hipError_t hipFree(void *p) { return stub_free(p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return stub_alloc(p, bytes); }
hipError_t hipHostFree(void *p) { return stub_free(p); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    if (fail_now()) return hipErrorOutOfMemory;
    *e = reinterpret_cast<hipEvent_t>(new stub_event{false});
    live_events++;
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e)
{
    stub_event *s = reinterpret_cast<stub_event *>(e);
    if (s->recorded) bad++;
    delete s;
    live_events--;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t) { reinterpret_cast<stub_event *>(e)->recorded = true; return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t e) { reinterpret_cast<stub_event *>(e)->recorded = false; n_sync++; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpy2DAsync(void *d, size_t dp, const void *s, size_t sp, size_t w, size_t h, hipMemcpyKind, hipStream_t)
{
    for (size_t r = 0; r < h; r++) memcpy(static_cast<char *>(d) + r * dp, static_cast<const char *>(s) + r * sp, w);
    return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) { memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t) { memset(d, v, n); return hipSuccess; }
}
#define CHECK(c) do { if (!(c)) { printf("line %d: %s (fail_at %ld)\n", __LINE__, #c, fail_at); return 1; } } while (0)
'''

# what trx_ms_tx.cpp and trx_tx_sched.cpp call besides the runtime, and a context filled in by hand
OBJECT_STUBS = r'''
#include "trx_ctx.h"
#include "trx_launch.h"
#include "trx_ms_tx.h"
#include "trx_tx_sched.h"
extern "C" {
int trx_tx_tables_generate(trx_tx_tables *t) { memset(t, 0, sizeof(*t)); return 0; }
int trx_launch_tx_render(const uint32_t *, size_t, int, int, int, const uint8_t *, const trx_tx_fill *, const float *, const trx_tx_tables *,
                         float *, int16_t *, const float *, size_t, hipStream_t) { return 0; }
int trx_launch_tx_fill_update(const trx_tx_fill_update *, size_t, const uint8_t *, trx_tx_fill *, hipStream_t) { return 0; }
int trx_launch_ms_tx_render(const trx_mstx_seg *, size_t, const trx_mstx_row *, const trx_tx_tables *, int16_t *, hipStream_t) { return 0; }
int trx_launch_ms_tx_stage(const trx_mstx_row *, const uint32_t *, size_t, trx_mstx_row *, size_t, hipStream_t) { return 0; }
int trx_launch_ms_tx_render_group(const trx_mstx_gmember *, uint32_t, uint32_t, const trx_mstx_row *, const trx_tx_tables *, int16_t *,
                                  hipStream_t) { return 0; }
int trx_launch_ms_tx_render_nco(const trx_mstx_seg *, size_t, const trx_mstx_row *, const trx_tx_tables *, int16_t *, trxhip_ms_nco_row,
                                const float *, hipStream_t) { return 0; }
int trx_launch_ms_tx_render_group_nco(const trx_mstx_gmember *, uint32_t, uint32_t, const trx_mstx_row *, const trx_tx_tables *, int16_t *,
                                      const float *, hipStream_t) { return 0; }
int trx_tx_frontend_geometry(const trxhip_tx_frontend *, int *, int *, size_t *) { return TRXHIP_EINVAL; }
int trxhip_tx_frontend_push(trxhip_tx_frontend *, const float *, size_t, size_t, float *, int16_t *, float, void *) { return TRXHIP_EINVAL; }
}
/* the two tables the objects ask the context for; with the owners of trx_mem.h the context frees them itself */
struct hand_ctx {
    trxhip_ctx ctx;
    hand_ctx()
    {
#ifdef TRX_MEM_H
        if (ctx.d_tx_tables.alloc(1) != TRXHIP_OK || ctx.d_nco_tab.alloc(4096) != TRXHIP_OK) abort();
#else
        if (hipMalloc((void **)&ctx.d_tx_tables, sizeof(trx_tx_tables)) != hipSuccess ||
            hipMalloc((void **)&ctx.d_nco_tab, 4096 * sizeof(float)) != hipSuccess) abort();
#endif
    }
    ~hand_ctx()
    {
#ifndef TRX_MEM_H
        hipFree(ctx.d_tx_tables);
        hipFree(ctx.d_nco_tab);
#endif
    }
};
/* a call's result under the one failure of a run: OK, or, when the failure fell into this call, what the site reports */
static bool result_ok(int rc, bool fired_before)
{
    return (fired && !fired_before) ? (rc == TRXHIP_ENOMEM || rc == TRXHIP_EIO) : rc == TRXHIP_OK;
}
'''

HEADER_MAIN = r'''
#include "trx_mem.h"
#include <utility>
template <typename B> static int block_case()
{
    {
        B a;
        CHECK(a.p == nullptr && a.cap == 0 && a.get() == nullptr);
        CHECK(a.alloc(100) == TRXHIP_OK && a.p && a.cap == 100 && a.get() == a.p && live_blocks == 1);
        a.p[99] = a.p[0];
        auto *p0 = a.p;
        const long na = n_alloc, nf = n_free;
        CHECK(a.reserve(50) == TRXHIP_OK && a.reserve(100) == TRXHIP_OK && a.p == p0 && a.cap == 100 && n_alloc == na && n_free == nf);
        CHECK(a.reserve(101) == TRXHIP_OK && a.cap == 101 && n_alloc == na + 1 && n_free == nf + 1 && live_blocks == 1);
        a.p[100] = a.p[0];
        /* growth whose allocation fails: out of memory, empty, nothing live */
        fail_at = n_counted;
        CHECK(a.reserve(1000) == TRXHIP_ENOMEM && a.p == nullptr && a.cap == 0 && live_blocks == 0);
        fail_at = n_counted;
        CHECK(a.alloc(10) == TRXHIP_ENOMEM && a.p == nullptr && a.cap == 0 && live_blocks == 0);
        fail_at = -1;
        CHECK(a.reserve(7) == TRXHIP_OK && a.cap == 7 && live_blocks == 1);
        /* move construction, move assignment over a non-empty target, onto itself */
        B b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.cap == 7 && b.p && live_blocks == 1);
        B c;
        CHECK(c.alloc(3) == TRXHIP_OK && live_blocks == 2);
        auto *pb = b.p;
        c = std::move(b);
        CHECK(c.p == pb && c.cap == 7 && b.p == nullptr && b.cap == 0 && live_blocks == 1);
        B &same = c;
        c = std::move(same);
        CHECK(c.p == pb && c.cap == 7 && live_blocks == 1);
        CHECK(c.reset() == TRXHIP_OK && c.p == nullptr && c.cap == 0 && live_blocks == 0 && c.reset() == TRXHIP_OK);
        CHECK(c.alloc(5) == TRXHIP_OK && live_blocks == 1);
    }
    CHECK(live_blocks == 0);                     /* the destructor freed the last one */
    return 0;
}
static int event_case()
{
    {
        trx_event never, e;
        CHECK(!e.pending() && e.wait() == TRXHIP_OK && n_sync == 0);       /* nothing made yet: nothing to wait for */
        fail_at = n_counted;
        CHECK(e.create() == TRXHIP_ENOMEM && e.ev == nullptr && live_events == 0);
        fail_at = -1;
        CHECK(e.create() == TRXHIP_OK && live_events == 1 && e.create() == TRXHIP_OK && live_events == 1);   /* idempotent */
        CHECK(never.create() == TRXHIP_OK && live_events == 2);
        CHECK(e.record(nullptr) == TRXHIP_OK && e.pending() && n_sync == 0);
        CHECK(e.wait() == TRXHIP_OK && !e.pending() && n_sync == 1);
        CHECK(e.wait() == TRXHIP_OK && n_sync == 1);                       /* waited for once */
        CHECK(e.record(nullptr) == TRXHIP_OK && e.pending());
        trx_event f(std::move(e));
        CHECK(f.pending() && !e.pending() && e.ev == nullptr && live_events == 2);
        trx_event g;
        CHECK(g.create() == TRXHIP_OK && g.record(nullptr) == TRXHIP_OK && live_events == 3);
        g = std::move(f);                        /* what g held is waited for, then destroyed */
        CHECK(n_sync == 2 && live_events == 2 && g.pending() && !f.pending() && bad == 0);
    }
    /* g was recorded: waited for exactly once before it went; `never` was not waited for */
    CHECK(n_sync == 3 && live_events == 0 && bad == 0);
    return 0;
}
int main()
{
    if (block_case<trx_dev<float>>() || block_case<trx_pin<double>>() || event_case()) return 1;
    trx_pin<char> mapped(hipHostMallocMapped);
    CHECK(mapped.flags == hipHostMallocMapped && mapped.alloc(16) == TRXHIP_OK);
    CHECK(mapped.reset() == TRXHIP_OK && live_blocks == 0 && live_events == 0);
    puts("owners ok");
    return 0;
}
'''

MS_TX_MAIN = r'''
static const size_t WIN[3] = { 8 * 625, 64 * 625, 512 * 625 };    /* 512 slots: past the buffers' floor of 4096 bytes */
static int16_t *out;
/* submit, then the three windows; *grew: counted calls during the last window */
template <typename Submit, typename Render> static int drive(Submit submit, Render render, long *grew)
{
    bool before = fired;
    CHECK(result_ok(submit(), before));
    int64_t first = 0;
    for (int w = 0; w < 3; w++) {
        before = fired;
        const long c0 = n_counted;
        const int rc = render(first, WIN[w]);
        CHECK(result_ok(rc, before));
        if (rc == TRXHIP_OK) first += (int64_t)WIN[w];     /* a refused window has not moved */
        *grew = n_counted - c0;
    }
    return 0;
}
static int run(trxhip_ctx *ctx, bool group, long *counted, long *grew)
{
    n_counted = 0;
    fired = false;
    const uint32_t n_mem = group ? 3 : 1, per = 200;
    std::vector<trxhip_ms_tx_req> reqs(n_mem * per);
    std::vector<uint32_t> member(reqs.size());
    for (size_t i = 0; i < reqs.size(); i++) {             /* one burst per slot from frame 110 on, per member */
        memset(&reqs[i], 0, sizeof(reqs[i]));
        reqs[i].fn = 110 + (uint32_t)(i / n_mem / 8);
        reqs[i].tn = (uint8_t)(i / n_mem % 8);
        reqs[i].bits[i % 148] = 1;
        member[i] = (uint32_t)(i % n_mem);
    }
    int rc;
    if (group) {
        const trxhip_ms_tx_group_cfg cfg = { n_mem, 2047, -60, 256 };
        trxhip_ms_tx_group *g = nullptr;
        rc = trxhip_ms_tx_group_create(ctx, &cfg, &g);
        CHECK(result_ok(rc, false) && (rc == TRXHIP_OK) == (g != nullptr));
        if (g) {
            const trxhip_ms_tx_clock now[3] = { { 100, 0, 0 }, { 100, 0, 0 }, { 100, 0, 0 } };
            std::vector<trxhip_ms_tx_plan> plan(reqs.size());
            /* one burst each first (the issue's sequence), then the rest: the staging buffer grows */
            bool before = fired;
            CHECK(result_ok(trxhip_ms_tx_group_submit(g, member.data(), reqs.data(), n_mem, now, plan.data(), nullptr, nullptr), before));
            if (drive([&] { return trxhip_ms_tx_group_submit(g, member.data() + n_mem, reqs.data() + n_mem, reqs.size() - n_mem, now,
                                                             plan.data(), nullptr, nullptr); },
                      [&](int64_t first, size_t n) {
                          const int64_t ts[3] = { first, first, first };
                          const size_t ns[3] = { n, n, n };
                          return trxhip_ms_tx_group_render_s16(g, out, WIN[2], ts, ns, nullptr, nullptr, nullptr);
                      }, grew))
                return 1;
            trxhip_ms_tx_status st;
            CHECK(trxhip_ms_tx_group_state(g, 2, &st) == TRXHIP_OK && (fired || st.queued == per));
            trxhip_ms_tx_group_destroy(g);
        }
    } else {
        const trxhip_ms_tx_cfg cfg = { 2047, -60, 256, 0 };
        trxhip_ms_tx *s = nullptr;
        rc = trxhip_ms_tx_create(ctx, &cfg, &s);
        CHECK(result_ok(rc, false) && (rc == TRXHIP_OK) == (s != nullptr));
        if (s) {
            bool before = fired;
            CHECK(result_ok(trxhip_ms_tx_submit(s, reqs.data(), 1, 100, 0, 0, nullptr, nullptr), before));
            if (drive([&] { return trxhip_ms_tx_submit(s, reqs.data() + 1, reqs.size() - 1, 100, 0, 0, nullptr, nullptr); },
                      [&](int64_t first, size_t n) { return trxhip_ms_tx_render_s16(s, out, n, first, nullptr, nullptr); }, grew))
                return 1;
            trxhip_ms_tx_status st;
            CHECK(trxhip_ms_tx_state(s, &st) == TRXHIP_OK && (fired || st.queued == per));
            trxhip_ms_tx_destroy(s);
        }
    }
    *counted = n_counted;
    return 0;
}
int main()
{
    out = static_cast<int16_t *>(malloc(3 * WIN[2] * 2 * sizeof(int16_t)));
    {
        hand_ctx h;
        const long base = live_blocks;
        for (int group = 0; group < 2; group++) {
            long counted = 0, grew = 0, c2, g2;
            fail_at = -1;
            if (run(&h.ctx, group, &counted, &grew)) return 1;
            CHECK(!fired && counted > 0 && grew > 0);      /* the last window made its tables grow */
            CHECK(live_blocks == base && live_events == 0 && bad == 0);
            for (long k = 0; k < counted; k++) {
                fail_at = k;
                if (run(&h.ctx, group, &c2, &g2)) return 1;
                CHECK(fired && live_blocks == base && live_events == 0 && bad == 0);
            }
            printf("%s: %ld counted calls\n", group ? "group" : "single", counted);
        }
        fail_at = -1;
    }
    free(out);
    CHECK(live_blocks == 0 && live_events == 0);
    puts("ms_tx ok");
    return 0;
}
'''

TX_SCHED_MAIN = r'''
static int run(trxhip_ctx *ctx, float *out, long *counted)
{
    n_counted = 0;
    fired = false;
    const trxhip_tx_sched_cfg cfg = { 2, 4, TRXHIP_FILLER_DUMMY, 4, 16, 1.0 };
    trxhip_tx_sched *s = nullptr;
    const int rc = trxhip_tx_sched_create(ctx, &cfg, &s);
    CHECK(result_ok(rc, false) && (rc == TRXHIP_OK) == (s != nullptr));
    if (s) {
        CHECK(trxhip_tx_sched_set_clock(s, 10, 0) == TRXHIP_OK && trxhip_tx_sched_set_slot(s, 0, 2, 1) == TRXHIP_OK);
        uint8_t dgram[6 + 148] = { 2, 0, 0, 0, 10, 0 };       /* version 0, TN 2, FN 10, no attenuation */
        int64_t id = -1;
        bool before = fired;
        CHECK(result_ok(trxhip_tx_sched_submit(s, 0, dgram, sizeof(dgram), &id), before) && id == 0);
        before = fired;
        CHECK(result_ok(trxhip_tx_sched_render(s, 8, out, 8 * 625, nullptr, nullptr, nullptr), before));
        trxhip_tx_plan plan[8];
        CHECK(trxhip_tx_sched_plan(s, 0, plan, 8) == TRXHIP_OK && plan[2].src == TRXHIP_TXS_SRC_BURST && plan[2].id == 0);
        trxhip_tx_sched_destroy(s);
    }
    *counted = n_counted;
    return 0;
}
int main()
{
    float *out = static_cast<float *>(malloc(2 * 8 * 625 * 2 * sizeof(float)));
    {
        hand_ctx h;
        const long base = live_blocks;
        long counted = 0, c2;
        fail_at = -1;
        if (run(&h.ctx, out, &counted)) return 1;
        CHECK(!fired && counted > 0 && live_blocks == base && live_events == 0 && bad == 0);
        for (long k = 0; k < counted; k++) {
            fail_at = k;
            if (run(&h.ctx, out, &c2)) return 1;
            CHECK(fired && live_blocks == base && live_events == 0 && bad == 0);
        }
        printf("tx_sched: %ld counted calls\n", counted);
        fail_at = -1;
    }
    free(out);
    CHECK(live_blocks == 0 && live_events == 0);
    puts("tx_sched ok");
    return 0;
}
'''


def run(cmd, **kw):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, **kw)


def build_and_run(tmp_path, text, sources, expect):
    if not os.path.exists(os.path.join(ROCM, "include", "hip", "hip_runtime.h")):
        pytest.fail("the HIP headers are needed (ROCM_PATH)")
    src = tmp_path / "main.cpp"
    src.write_text(textwrap.dedent(text))
    exe = tmp_path / "main"
    r = run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-Wall", "-Wno-unused-result"] + SAN +
            ["-I", os.path.join(ROCM, "include"), "-I", CSRC, "-I", os.path.join(ROOT, "include"), str(src)] +
            [os.path.join(CSRC, s) for s in sources] + ["-o", str(exe)])
    assert r.returncode == 0, r.stdout
    r = run([str(exe)])
    assert r.returncode == 0 and expect in r.stdout, r.stdout
    return r.stdout


def test_owners_alone(tmp_path):
    build_and_run(tmp_path, STUBS + HEADER_MAIN, [], "owners ok")


def test_ms_tx_every_allocation_failure(tmp_path):
    """The single object and a group of three: submit, windows of 8, 64 and 512 slots, destroy; then the same with each counted
    call failing in turn."""
    build_and_run(tmp_path, STUBS + "#include <vector>\n" + OBJECT_STUBS + MS_TX_MAIN, ["trx_ms_tx.cpp"], "ms_tx ok")


def test_tx_sched_every_allocation_failure(tmp_path):
    build_and_run(tmp_path, STUBS + OBJECT_STUBS + TX_SCHED_MAIN, ["trx_tx_sched.cpp"], "tx_sched ok")
