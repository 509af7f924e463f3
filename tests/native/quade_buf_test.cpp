// Host-only test of quade_amd/csrc/quade_buf.h: the owner's growth and ownership logic over a counting source that backs every
// allocation with malloc.  No HIP call is linked: the header reaches HIP only through a source, and the HIP sources are not used here.
// Built and run by tests/test_host_buf.py, plain and under AddressSanitizer + UBSan (which also sees a leak and a double free).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../quade_amd/csrc/quade_buf.h"

namespace {

int g_failed = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                    \
        }                                                                  \
    } while (0)

// The counting source: every get is a malloc of exactly `want` bytes and is recorded; the k-th get from now can be told to fail.
struct Fake {
    static std::map<void*, size_t> live;  // block -> size
    static std::vector<size_t> gets;      // sizes asked for, successful or not
    static std::vector<void*> puts;       // blocks given back, in order
    static int double_puts, foreign_puts, wrong_cap_puts, drains, copies;
    static int fail_in;  // > 0: the fail_in-th get from now fails

    static void reset() {
        gets.clear();
        puts.clear();
        double_puts = foreign_puts = wrong_cap_puts = drains = copies = 0;
        fail_in = 0;
    }
    static hipError_t get(size_t want, void** p, size_t* cap) {
        gets.push_back(want);
        if (fail_in > 0 && --fail_in == 0) return hipErrorOutOfMemory;
        *p = malloc(want ? want : 1);
        *cap = want;
        live[*p] = want;
        return hipSuccess;
    }
    static void put(void* p, size_t cap) {
        auto it = live.find(p);
        if (it == live.end()) {
            bool before = false;
            for (void* q : puts) before |= q == p;
            ++(before ? double_puts : foreign_puts);
            return;
        }
        if (it->second != cap) ++wrong_cap_puts;
        live.erase(it);
        puts.push_back(p);
        free(p);
    }
    static hipError_t drain() {
        ++drains;
        return hipSuccess;
    }
    static hipError_t copy(void* dst, const void* src, size_t n, hipStream_t) {
        ++copies;
        memcpy(dst, src, n);
        return hipSuccess;
    }
    static bool clean() { return double_puts == 0 && foreign_puts == 0 && wrong_cap_puts == 0; }
};
std::map<void*, size_t> Fake::live;
std::vector<size_t> Fake::gets;
std::vector<void*> Fake::puts;
int Fake::double_puts, Fake::foreign_puts, Fake::wrong_cap_puts, Fake::drains, Fake::copies, Fake::fail_in;

using Buf = qbuf::Buf<Fake>;

void test_need_below_capacity_does_nothing() {
    Fake::reset();
    Buf b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.need(1000, 1500) == hipSuccess);
    uint8_t* const p = b.p;
    CHECK(p && b.cap == 1500 && Fake::gets.size() == 1);
    for (size_t n : {(size_t)0, (size_t)1, (size_t)1000, (size_t)1500}) {
        CHECK(b.need(n, n + 7777) == hipSuccess);
        CHECK(b.need(n, n + 7777, n / 2, nullptr) == hipSuccess);
    }
    CHECK(b.p == p && b.cap == 1500 && Fake::gets.size() == 1 && Fake::puts.empty() && Fake::drains == 0 && Fake::copies == 0);
}

// every rule the call sites use: a growth asks the source for exactly the rule's bytes, and the old block goes back exactly once
void test_growth_requests_the_site_rule() {
    for (size_t n : {(size_t)1, (size_t)3, (size_t)4096, (size_t)65537, (size_t)1000003}) {
        // the pipeline's device buffers and the gzip inflater's: n + n/4 + 64 KiB
        // the page-locked ones: n + n/4 + 4096
        // exact
        const size_t want[3] = {qbuf::quarter(n, 65536), qbuf::quarter(n, 4096), n};
        const size_t expect[3] = {n + n / 4 + 65536, n + n / 4 + 4096, n};
        for (int r = 0; r < 3; ++r) {
            Fake::reset();
            {
                Buf b;
                CHECK(b.need(8, 8) == hipSuccess);  // something to give back
                uint8_t* const old = b.p;
                CHECK(b.need(n + 8, want[r] + 8) == hipSuccess);
                CHECK(Fake::gets.size() == 2 && Fake::gets[1] == expect[r] + 8 && b.cap == expect[r] + 8);
                CHECK(Fake::puts.size() == 1 && Fake::puts[0] == old);
                CHECK(Fake::live.size() == 1);
            }
            CHECK(Fake::puts.size() == 2 && Fake::live.empty() && Fake::clean());
        }
        // elements: the stand-alone coders' pairs (n + n/4 + 4096 elements) and their scratch (n + n/4 + 16 elements)
        {
            Fake::reset();
            qbuf::Pair<uint32_t, Fake, Fake> pr;
            CHECK(pr.need(n, qbuf::quarter(n, 4096)) == hipSuccess);
            CHECK(Fake::gets.size() == 2 && Fake::gets[0] == (n + n / 4 + 4096) * 4 && Fake::gets[1] == (n + n / 4 + 4096) * 4);
            CHECK(pr.cap() == n + n / 4 + 4096);
            CHECK(pr.need(pr.cap(), 1) == hipSuccess && Fake::gets.size() == 2);  // one capacity, in elements
            Buf b;
            const size_t per = 24;
            CHECK(b.need(n * per, qbuf::quarter(n, 16) * per) == hipSuccess);
            CHECK(Fake::gets.back() == (n + n / 4 + 16) * per);
            CHECK(b.need((n + n / 4 + 16) * per, 1) == hipSuccess && Fake::gets.size() == 3);
        }
        CHECK(Fake::live.empty() && Fake::clean());
    }
    // doubling (the per-stream scratch): twice what it held, at least what is needed; the site keeps the units and allocates exactly
    CHECK(qbuf::twice(10, 0) == 10 && qbuf::twice(10, 4) == 10 && qbuf::twice(10, 5) == 10 && qbuf::twice(10, 6) == 12 && qbuf::twice(1, 1000) == 2000);
    Fake::reset();
    {
        Buf b;
        size_t units = 0;
        auto bytes_for = [](size_t u) { return (2 * u + 4) * 4; };
        for (size_t ask : {(size_t)100, (size_t)150, (size_t)201, (size_t)1000}) {
            if (b.p && units >= ask) continue;
            const size_t grown = qbuf::twice(ask, units);
            CHECK(b.alloc(bytes_for(grown)) == hipSuccess);
            units = grown;
        }
        CHECK(Fake::gets.size() == 4 && Fake::gets[0] == bytes_for(100) && Fake::gets[1] == bytes_for(200) && Fake::gets[2] == bytes_for(400) &&
              Fake::gets[3] == bytes_for(1000));
        CHECK(Fake::puts.size() == 3 && Fake::live.size() == 1);
    }
    CHECK(Fake::live.empty() && Fake::clean());
}

void test_need_keeps_a_prefix() {
    for (size_t keep : {(size_t)0, (size_t)1, (size_t)777, (size_t)1000}) {
        Fake::reset();
        {
            Buf b;
            CHECK(b.need(1000, 1000, keep, nullptr) == hipSuccess);  // a first allocation: nothing to keep, nothing to drain
            CHECK(Fake::drains == 0 && Fake::copies == 0);
            for (size_t i = 0; i < 1000; ++i) b.p[i] = (uint8_t)(i * 7 + 3);
            uint8_t* const old = b.p;
            CHECK(b.need(5000, 6000, keep, nullptr) == hipSuccess);
            CHECK(b.p != old && b.cap == 6000 && Fake::gets.size() == 2 && Fake::gets[1] == 6000);
            CHECK(Fake::drains == 1 && Fake::copies == (keep ? 1 : 0));
            CHECK(Fake::puts.size() == 1 && Fake::puts[0] == old);
            bool same = true;
            for (size_t i = 0; i < keep; ++i) same &= b.p[i] == (uint8_t)(i * 7 + 3);
            CHECK(same);
            // a failed get behind a growth with a prefix to keep leaves the old block in place, and the next call grows it
            Fake::fail_in = 1;
            uint8_t* const cur = b.p;
            CHECK(b.need(7000, 8000, keep, nullptr) == hipErrorOutOfMemory);
            CHECK(b.p == cur && b.cap == 6000 && Fake::puts.size() == 1);
            CHECK(b.need(7000, 8000, keep, nullptr) == hipSuccess && b.cap == 8000 && Fake::puts.size() == 2);
        }
        CHECK(Fake::live.empty() && Fake::clean());
    }
}

void test_a_failed_get_leaves_the_buffer_empty() {
    Fake::reset();
    {
        Buf b;
        Fake::fail_in = 1;
        CHECK(b.need(100, 200) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);
        CHECK(b.need(100, 200) == hipSuccess && b.p && b.cap == 200);
        Fake::fail_in = 1;
        CHECK(b.need(300, 400) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);  // the old block went back before the get
        CHECK(Fake::puts.size() == 1);
        CHECK(b.need(10, 20) == hipSuccess && b.p && b.cap == 20);  // allocates again, even for less than it once held
        Fake::fail_in = 1;
        CHECK(b.alloc(50) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0);
        b.release();
        CHECK(Fake::puts.size() == 2);
    }
    CHECK(Fake::puts.size() == 2 && Fake::live.empty() && Fake::clean());
}

void test_moves() {
    Fake::reset();
    {
        Buf a;
        CHECK(a.alloc(64) == hipSuccess);
        uint8_t* const pa = a.p;
        Buf b(std::move(a));  // move construction: the source is empty, nothing is put
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 64 && Fake::puts.empty());
        Buf c;
        CHECK(c.alloc(32) == hipSuccess);
        uint8_t* const pc = c.p;
        c = std::move(b);  // move assignment: the overwritten block is put, the source is empty
        CHECK(b.p == nullptr && b.cap == 0 && c.p == pa && c.cap == 64);
        CHECK(Fake::puts.size() == 1 && Fake::puts[0] == pc);
        Buf& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.cap == 64 && Fake::puts.size() == 1);
        // owners inside a growing vector (the per-stream scratch, the staging chunks)
        std::vector<Buf> v;
        for (int i = 0; i < 9; ++i) {
            v.emplace_back();
            CHECK(v.back().alloc(16 + (size_t)i) == hipSuccess);
        }
        CHECK(Fake::live.size() == 10 && Fake::puts.size() == 1);
        static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "an owner is not copied");
    }
    CHECK(Fake::puts.size() == 11 && Fake::live.empty() && Fake::clean());
}

void test_release_then_destructor_puts_once() {
    Fake::reset();
    {
        Buf b;
        CHECK(b.alloc(128) == hipSuccess);
        b.release();
        CHECK(b.p == nullptr && b.cap == 0 && Fake::puts.size() == 1);
        b.release();
        CHECK(Fake::puts.size() == 1);
    }
    CHECK(Fake::puts.size() == 1 && Fake::live.empty() && Fake::clean());
    {
        qbuf::Arr<uint32_t, Fake> a;  // the typed view converts to its pointer
        CHECK(!a);
        CHECK(a.alloc(40) == hipSuccess);
        uint32_t* q = a;
        CHECK(q == a.as<uint32_t>() && (void*)q == (void*)a.p);
        q[9] = 5;
        CHECK(a[9] == 5);
    }
    CHECK(Fake::live.empty() && Fake::clean());
}

void test_pair() {
    Fake::reset();
    {
        qbuf::Pair<uint64_t, Fake, Fake> pr;
        CHECK(pr.need(10, 20) == hipSuccess && pr.cap() == 20 && pr.h && pr.d && pr.h.cap == 160 && pr.d.cap == 160);
        CHECK(pr.need(20, 99) == hipSuccess && Fake::gets.size() == 2);
        // the second half fails: both halves are empty, the first half's new block and both old blocks went back once each
        Fake::fail_in = 2;
        CHECK(pr.need(21, 30) == hipErrorOutOfMemory);
        CHECK(!pr.h && !pr.d && pr.cap() == 0 && pr.h.cap == 0 && pr.d.cap == 0);
        CHECK(Fake::gets.size() == 4 && Fake::puts.size() == 3 && Fake::live.empty());
        // the first half fails: the second is not asked for
        Fake::fail_in = 1;
        CHECK(pr.need(21, 30) == hipErrorOutOfMemory && Fake::gets.size() == 5 && pr.cap() == 0);
        // and the next call recovers
        CHECK(pr.need(21, 30) == hipSuccess && pr.cap() == 30 && pr.h && pr.d && Fake::live.size() == 2);
    }
    CHECK(Fake::live.empty() && Fake::clean());
}

}  // namespace

int main() {
    test_need_below_capacity_does_nothing();
    test_growth_requests_the_site_rule();
    test_need_keeps_a_prefix();
    test_a_failed_get_leaves_the_buffer_empty();
    test_moves();
    test_release_then_destructor_puts_once();
    test_pair();
    CHECK(Fake::live.empty());
    if (g_failed) {
        printf("%d checks failed\n", g_failed);
        return 1;
    }
    printf("ok\n");
    return 0;
}
