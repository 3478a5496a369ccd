// gd::DevMem (gpudrive_lab_amd/csrc/dev_mem.hpp) on the host: the two allocator hooks over malloc, with a record of the live
// blocks, a count of frees of blocks that are not live, and a countdown that makes the n-th allocation throw.  Prints one
// line per failed check and exits with their number (tests/test_dev_mem.py).
#include <cstdio>
#include <cstdlib>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "../gpudrive_lab_amd/csrc/dev_mem.hpp"

namespace {
std::set<void *> g_live;
int g_unknown_frees = 0;
int g_fail_in = 0;  // n > 0: the n-th allocation from now throws
int g_failed = 0;

void check(bool ok, const char *what) {
    if (ok) return;
    std::printf("FAILED: %s\n", what);
    g_failed++;
}
}  // namespace

void *gd::dev_alloc(size_t bytes) {
    if (g_fail_in > 0 && --g_fail_in == 0) throw std::runtime_error("out of device memory");
    void *p = std::malloc(bytes);
    g_live.insert(p);
    return p;
}

void gd::dev_free(void *p) noexcept {
    if (g_live.erase(p) == 0) {
        g_unknown_frees++;
        return;
    }
    std::free(p);
}

int main() {
    using gd::DevMem;
    {  // a move leaves the source empty
        DevMem a(64);
        void *p = a.get();
        check(p && a.bytes() == 64 && g_live.count(p) == 1, "constructor allocates");
        DevMem b(std::move(a));
        check(a.get() == nullptr && a.bytes() == 0, "move construction empties the source");
        check(b.get() == p && b.bytes() == 64, "move construction hands the block over");
        DevMem c(32);
        void *q = c.get();
        c = std::move(b);
        check(b.get() == nullptr && b.bytes() == 0, "move assignment empties the source");
        check(c.get() == p && c.bytes() == 64 && g_live.count(q) == 0 && g_live.size() == 1, "move assignment frees the target's block");
        c = std::move(c);
        check(c.get() == p && g_live.size() == 1, "self move keeps the block");
    }
    check(g_live.empty(), "destructors free");
    {  // a reserve within capacity keeps the pointer; one beyond it frees exactly the old block first
        DevMem a;
        check(!a.reserve(0, 100) && a.get() == nullptr, "nothing needed, nothing allocated");
        check(a.reserve(10, 100) && a.bytes() == 100, "first reserve allocates grow_to bytes");
        void *p = a.get();
        check(!a.reserve(100, 500) && a.get() == p && a.bytes() == 100, "reserve within capacity keeps the block");
        check(a.reserve(101, 500) && a.bytes() == 500, "reserve beyond capacity reports the reallocation");
        check(g_live.count(p) == 0 && g_live.size() == 1 && g_live.count(a.get()) == 1, "exactly the old block was freed");
    }
    check(g_live.empty(), "destructor frees the grown block");
    {  // a failed reserve leaves the owner empty, with the old block returned before the request
        DevMem a(16);
        g_fail_in = 1;
        bool threw = false;
        try {
            a.reserve(17, 64);
        } catch (const std::runtime_error &) {
            threw = true;
        }
        check(threw, "the failed allocation throws");
        check(a.get() == nullptr && a.bytes() == 0 && g_live.empty(), "a failed reserve leaves the owner empty");
        check(a.reserve(17, 64) && a.get() && a.bytes() == 64, "a later reserve works");
    }
    check(g_live.empty(), "destructor after a failed and a successful reserve");
    {
        DevMem a(16);
        g_fail_in = 1;
        try {
            a.reserve(17, 64);
        } catch (const std::runtime_error &) {
        }
    }  // destructor of the empty owner
    check(g_live.empty() && g_unknown_frees == 0, "destructor after a failed reserve frees nothing twice");
    {  // the rank buffers' pattern: local owners unwind after a failure in the middle, the published list is untouched
        std::vector<DevMem> published;
        published.emplace_back(8);
        bool threw = false;
        try {
            std::vector<DevMem> mine;
            g_fail_in = 4;
            for (int k = 0; k < 8; k++) mine.emplace_back(static_cast<size_t>(32 + k));
            for (DevMem &m : mine) published.push_back(std::move(m));
        } catch (const std::runtime_error &) {
            threw = true;
        }
        check(threw && published.size() == 1 && g_live.size() == 1, "a vector of owners unwinds after a failure in the middle");
        std::vector<DevMem> mine;  // and the same without a failure: everything is handed over
        for (int k = 0; k < 8; k++) mine.emplace_back(static_cast<size_t>(32 + k));
        for (DevMem &m : mine) published.push_back(std::move(m));
        mine.clear();
        check(published.size() == 9 && g_live.size() == 9, "published owners keep their blocks");
    }
    check(g_live.empty(), "no live blocks at exit");
    check(g_unknown_frees == 0, "no frees of unknown blocks");
    if (!g_failed) std::printf("ok\n");
    return g_failed;
}
