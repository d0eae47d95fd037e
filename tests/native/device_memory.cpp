// CPU test of csrc/nmi_mem.h (tests/test_device_memory.py builds it with g++ under ASan / UBSan): the owners of device memory
// against a HIP runtime defined right here -- malloc / free behind every allocation and handle, so that the sanitizer sees a
// leak, a double free or a use after free; a log of the calls; and a switch that makes the Nth call fail.  A failed free or
// destroy still releases (the runtime reports a broken device there): what the test looks for is a SECOND release.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "nmi_mem.h"

using namespace nmi_mem;

namespace {

struct Call {
    std::string name;
    const void *what;  // the buffer, event or stream it was about
};
std::vector<Call> g_log;
std::set<void *> g_device, g_host, g_events, g_streams;
long g_calls = 0, g_fail_at = 0;  // g_fail_at: the call (counted from 1) that fails; 0 = none

bool enter(const char *name, const void *what)
{
    g_log.push_back({name, what});
    return ++g_calls != g_fail_at;
}

void fresh_runtime(long fail_at = 0)
{
    g_log.clear();
    g_calls = 0;
    g_fail_at = fail_at;
}

size_t live() { return g_device.size() + g_host.size() + g_events.size() + g_streams.size(); }

hipError_t make(std::set<void *> &where, void **out, size_t bytes, bool ok)
{
    if (!ok) return hipErrorOutOfMemory;
    *out = malloc(bytes ? bytes : 1);
    where.insert(*out);
    return hipSuccess;
}

hipError_t drop(std::set<void *> &where, void *p, bool ok)
{
    if (!where.erase(p)) {
        printf("FAIL: release of %p, which is not live (%s)\n", p, g_log.back().name.c_str());
        exit(1);
    }
    free(p);
    return ok ? hipSuccess : hipErrorUnknown;
}

void must_be_live(const std::set<void *> &where, const void *p)
{
    if (!where.count(const_cast<void *>(p))) {
        printf("FAIL: %s on %p, which is not live\n", g_log.back().name.c_str(), p);
        exit(1);
    }
}

}  // namespace

extern "C" {

hipError_t hipMalloc(void **p, size_t bytes) { return make(g_device, p, bytes, enter("malloc", nullptr)); }
hipError_t hipFree(void *p) { return drop(g_device, p, enter("free", p)); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned) { return make(g_host, p, bytes, enter("host_malloc", nullptr)); }
hipError_t hipHostFree(void *p) { return drop(g_host, p, enter("host_free", p)); }
hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned)
{
    const bool ok = enter("device_pointer", host);
    must_be_live(g_host, host);
    *dev = host;
    return ok ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipMemsetAsync(void *dst, int value, size_t bytes, hipStream_t stream)
{
    const bool ok = enter("memset", dst);
    must_be_live(g_device, dst);
    if (stream) must_be_live(g_streams, stream);
    if (ok) memset(dst, value, bytes);
    return ok ? hipSuccess : hipErrorUnknown;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t stream)
{
    const bool ok = enter("memcpy", dst);
    must_be_live(g_device, dst);
    must_be_live(g_host, src);
    must_be_live(g_streams, stream);
    if (ok) memcpy(dst, src, bytes);
    return ok ? hipSuccess : hipErrorUnknown;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    const bool ok = enter("wait", s);
    must_be_live(g_streams, s);
    return ok ? hipSuccess : hipErrorUnknown;
}
hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) { return make(g_streams, (void **)s, 1, enter("stream_create", nullptr)); }
hipError_t hipStreamDestroy(hipStream_t s) { return drop(g_streams, s, enter("stream_destroy", s)); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return make(g_events, (void **)e, 1, enter("event_create", nullptr)); }
hipError_t hipEventDestroy(hipEvent_t e) { return drop(g_events, e, enter("event_destroy", e)); }
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    const bool ok = enter("event_record", e);
    must_be_live(g_events, e);
    must_be_live(g_streams, s);
    return ok ? hipSuccess : hipErrorUnknown;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    const bool ok = enter("event_wait", e);
    must_be_live(g_events, e);
    return ok ? hipSuccess : hipErrorUnknown;
}

}  // extern "C"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++g_failures;                                             \
        }                                                             \
    } while (0)

std::string names()
{
    std::string s;
    for (const Call &c : g_log) s += (s.empty() ? "" : " ") + c.name;
    return s;
}

void test_grow_rule()
{
    fresh_runtime();
    Stream st;
    CHECK(st.create(0) == hipSuccess);
    {
        DeviceBuffer b;
        fresh_runtime();
        CHECK(b.grow(64, st) == hipSuccess);  // empty: nothing to wait for
        CHECK(names() == "malloc");
        CHECK(b && b.size() == 64);
        void *first = b.as<>();
        fresh_runtime();
        CHECK(b.grow(64, st) == hipSuccess && b.grow(1, st, true) == hipSuccess && b.grow(0) == hipSuccess);
        CHECK(g_calls == 0 && b.as<>() == first);  // a request that fits: no runtime call
        fresh_runtime();
        CHECK(b.grow(65, st, /*zero=*/true) == hipSuccess);
        CHECK(names() == "wait free malloc memset");
        CHECK(g_log[1].what == first && g_log[3].what == b.as<>() && b.size() == 65);
        for (size_t i = 0; i < 65; ++i) CHECK(b.as<unsigned char>()[i] == 0);
        fresh_runtime();
        CHECK(b.grow(200) == hipSuccess);  // no stream given: never a wait
        CHECK(names() == "free malloc" && b.size() == 200);
        fresh_runtime();
        CHECK(b.grow(300, st) == hipSuccess);
        CHECK(names() == "wait free malloc");
        fresh_runtime();
    }
    CHECK(names() == "free");  // the destructor's, once
    {
        PinnedBuffer p;
        fresh_runtime();
        CHECK(p.grow(32, kPosted, st) == hipSuccess);
        CHECK(names() == "host_malloc device_pointer" && p.device<>() == p.as<>() && p.size() == 32);
        fresh_runtime();
        CHECK(p.grow(32, kPosted, st) == hipSuccess && g_calls == 0);
        CHECK(p.grow(33, kPinned, st) == hipSuccess);
        CHECK(names() == "wait host_free host_malloc" && p.device<>() == nullptr);
        fresh_runtime();
        CHECK(p.grow(64, kPinned) == hipSuccess);
        CHECK(names() == "host_free host_malloc");
    }
    CHECK(live() == 1);  // the stream
}

void test_failures_leave_it_empty()
{
    Stream st;
    CHECK(st.create(0) == hipSuccess);
    // a failed allocation (the 3rd call of wait, free, malloc)
    {
        DeviceBuffer b;
        CHECK(b.alloc(16) == hipSuccess);
        fresh_runtime(3);
        CHECK(b.grow(32, st) == hipErrorOutOfMemory);
        CHECK(!b && b.size() == 0 && b.as<>() == nullptr);
        fresh_runtime();
    }
    CHECK(g_calls == 0);  // destruction of the empty object frees nothing
    // a failed free, a failed wait, a failed memset
    for (long nth = 1; nth <= 4; ++nth) {
        {
            DeviceBuffer b;
            CHECK(b.alloc(16) == hipSuccess);
            fresh_runtime(nth);
            CHECK(b.grow(32, st, true) != hipSuccess);
            CHECK(!b && b.size() == 0);
            if (nth <= 2) CHECK(names() == "wait free");  // nothing is allocated after a failed wait or free
            fresh_runtime();
        }
        CHECK(g_calls == 0);
    }
    // pinned: a failed allocation, a failed free, a failed device-pointer lookup
    for (long nth = 1; nth <= 3; ++nth) {
        {
            PinnedBuffer p;
            CHECK(p.alloc(16, kPosted) == hipSuccess);
            fresh_runtime(nth);
            CHECK(p.grow(32, kPosted) != hipSuccess);
            CHECK(!p && p.size() == 0 && p.device<>() == nullptr);
            fresh_runtime();
        }
        CHECK(g_calls == 0);
    }
    fresh_runtime(1);
    Event ev;
    CHECK(ev.create(0) != hipSuccess && (hipEvent_t)ev == nullptr);
    fresh_runtime();
}

void test_moves()
{
    fresh_runtime();
    {
        DeviceBuffer a;
        CHECK(a.alloc(8) == hipSuccess);
        void *p = a.as<>();
        DeviceBuffer b(std::move(a));
        CHECK(!a && a.size() == 0 && b.as<>() == p && b.size() == 8);
        DeviceBuffer c;
        CHECK(c.alloc(4) == hipSuccess);
        c = std::move(b);  // releases its own, takes b's
        CHECK(!b && c.as<>() == p);
        PinnedBuffer h;
        CHECK(h.alloc(8, kPosted) == hipSuccess);
        PinnedBuffer h2(std::move(h));
        CHECK(!h && h.device<>() == nullptr && h2 && h2.device<>() == h2.as<>());
        Event e;
        CHECK(e.create(0) == hipSuccess);
        Event e2(std::move(e));
        CHECK((hipEvent_t)e == nullptr && (hipEvent_t)e2 != nullptr);
        Stream s, s2;
        CHECK(s.create(0) == hipSuccess);
        s2 = std::move(s);
        CHECK((hipStream_t)s == nullptr && (hipStream_t)s2 != nullptr);
        fresh_runtime();
    }
    CHECK(names() == "stream_destroy event_destroy host_free free");  // one release each: the moved-from objects release nothing
    CHECK(live() == 0);
}

void test_ring()
{
    Stream st;
    CHECK(st.create(0) == hipSuccess);
    {
        UploadRing ring;
        UploadRing::Slot slots[UploadRing::kSlots + 1];
        fresh_runtime();
        CHECK(ring.acquire(9, st, &slots[0]) == hipSuccess);
        // first use: no wait for the stream, every slot allocated, then the slot's own event
        CHECK(names() == "malloc host_malloc event_create malloc host_malloc event_create malloc host_malloc event_create malloc host_malloc event_create event_wait");
        for (int i = 0; i < 9; ++i) slots[0].h[i] = (float)i;
        CHECK(UploadRing::upload(slots[0], st) == hipSuccess && UploadRing::release(slots[0], st) == hipSuccess);
        CHECK(slots[0].d[8] == 8.0f && slots[0].n == 9);
        for (int k = 1; k <= UploadRing::kSlots; ++k) {
            fresh_runtime();
            CHECK(ring.acquire(9, st, &slots[k]) == hipSuccess);
            CHECK(names() == "event_wait" && g_log[0].what == slots[k].consumed);  // nothing but the wait for that slot's event
            CHECK(UploadRing::upload(slots[k], st) == hipSuccess && UploadRing::release(slots[k], st) == hipSuccess);
            CHECK(g_log[1].what == slots[k].d && g_log[2].what == slots[k].consumed);
        }
        for (int k = 1; k < UploadRing::kSlots; ++k) CHECK(slots[k].d != slots[0].d && slots[k].consumed != slots[0].consumed);
        // the fifth use is the first slot again -- handed out after the wait for the event its release recorded
        CHECK(slots[UploadRing::kSlots].d == slots[0].d && slots[UploadRing::kSlots].h == slots[0].h &&
              slots[UploadRing::kSlots].consumed == slots[0].consumed);
        // growth: one wait for the stream, all four slots freed and allocated together, the events kept
        UploadRing::Slot big;
        fresh_runtime();
        CHECK(ring.acquire(18, st, &big) == hipSuccess);
        CHECK(names() == "wait free host_free free host_free free host_free free host_free malloc host_malloc malloc host_malloc malloc host_malloc "
                         "malloc host_malloc event_wait");
        CHECK(big.n == 18 && big.consumed == slots[1].consumed);
        big.h[17] = 1.0f;
        CHECK(UploadRing::upload(big, st) == hipSuccess && big.d[17] == 1.0f);
        fresh_runtime();
        CHECK(ring.acquire(10, st, &big) == hipSuccess && names() == "event_wait");  // smaller again: fits
        fresh_runtime();
    }
    CHECK(g_calls == 3 * UploadRing::kSlots && live() == 1);
}

// Buffers, pinned buffers, a ring, events and a stream, each grown twice; whatever fails, the scenario goes on with what it
// still may use, as a caller that returned the error and was called again would.
void scenario()
{
    Stream st;
    Event ev;
    DeviceBuffer a, b;
    PinnedBuffer p, q;
    UploadRing ring;
    if (st.create(0) != hipSuccess) return;  // (every other call takes the stream)
    const bool have_ev = ev.create(0) == hipSuccess;
    for (size_t bytes : {64, 128, 512}) {
        if (a.grow(bytes, st, /*zero=*/true) != hipSuccess) CHECK(!a && a.size() == 0);
        if (b.grow(bytes / 2) != hipSuccess) CHECK(!b && b.size() == 0);
        if (p.grow(bytes, kPosted, st) != hipSuccess) CHECK(!p && p.device<>() == nullptr);
        if (q.grow(bytes, kPinned) != hipSuccess) CHECK(!q);
        if (a) a.as<char>()[bytes - 1] = 1;
        if (p) p.as<char>()[bytes - 1] = 1;
        for (int use = 0; use < 5; ++use) {
            UploadRing::Slot s;
            if (ring.acquire(bytes / 16, st, &s) != hipSuccess) continue;
            s.h[bytes / 16 - 1] = 2.0f;
            if (UploadRing::upload(s, st) == hipSuccess) (void)UploadRing::release(s, st);
        }
        if (have_ev) (void)hipEventRecord(ev, st);
    }
    DeviceBuffer moved(std::move(a));
    b = std::move(moved);
}

void test_every_failure_point()
{
    fresh_runtime();
    scenario();
    const long total = g_calls;
    CHECK(total > 100 && live() == 0);
    for (long nth = 1; nth <= total; ++nth) {
        fresh_runtime(nth);
        scenario();
        if (live() != 0) {
            printf("FAIL: call %ld of %ld failing leaves %zu allocations or handles alive\n", nth, total, live());
            ++g_failures;
        }
    }
    fresh_runtime();
    printf("every failure point: %ld runtime calls, each failed once\n", total);
}

}  // namespace

int main()
{
    test_grow_rule();
    test_failures_leave_it_empty();
    test_moves();
    test_ring();
    test_every_failure_point();
    if (g_failures || live() != 0) {
        printf("device memory: %d failures, %zu live\n", g_failures, live());
        return 1;
    }
    printf("device memory ok\n");
    return 0;
}
