// dev_mem_demo.cpp — DevMem (relearn_amd/csrc/dev_mem.hpp) over malloc: the ownership rules the handles of the C ABI rely
// on, checked on the host under the sanitizers (tests/test_device_memory_cpu.py).  The four allocator functions are this
// program's own: they count what is live and can be told to fail the k-th allocation.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>

#include "relearn_amd/csrc/dev_mem.hpp"

static uint64_t g_bytes = 0, g_allocs = 0, g_host_allocs = 0;
static int64_t g_fail_in = 0;  // > 0: that many allocations from now, one throws

static void *counted_alloc(uint64_t bytes, uint64_t &count) {
  if (g_fail_in > 0 && --g_fail_in == 0) throw std::runtime_error("injected allocation failure");
  void *p = std::malloc(bytes);
  if (!p) throw std::bad_alloc();
  count += 1;
  return p;
}
void *rl_device_alloc(uint64_t bytes) {
  void *p = counted_alloc(bytes, g_allocs);
  g_bytes += bytes;
  return p;
}
void rl_device_free(void *p, uint64_t bytes) {
  std::free(p);
  g_bytes -= bytes;
  g_allocs -= 1;
}
void *rl_host_alloc(uint64_t bytes, bool) { return counted_alloc(bytes, g_host_allocs); }
void rl_host_free(void *p) {
  std::free(p);
  g_host_allocs -= 1;
}

static int g_failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "%s:%d: FAILED %s\n", __FILE__, __LINE__, #cond); \
      g_failures += 1;                                                  \
    }                                                                   \
  } while (0)
static bool nothing_live() { return g_bytes == 0 && g_allocs == 0 && g_host_allocs == 0; }

// a handle in the shape of the library's: an owner and plain pointers beside it
struct Handle {
  DevMem mem;
  float *a = nullptr, *b = nullptr;
  double *c = nullptr;
  uint32_t *pinned = nullptr;
  float *view = nullptr;  // into the middle of `a`
};
constexpr int CREATE_ALLOCATIONS = 4;
static void create(Handle &h) {
  h.a = h.mem.alloc<float>(100);
  h.view = h.a + 50;
  h.b = h.mem.alloc<float>(0);  // (a count of 0 becomes 1)
  h.c = h.mem.alloc<double>(7);
  h.pinned = h.mem.alloc_host<uint32_t>(16, true);
}

int main() {
  {  // the destructor frees everything; views are not its business
    Handle h;
    create(h);
    CHECK(g_allocs == 3 && g_host_allocs == 1 && g_bytes == 100 * 4 + 4 + 7 * 8);
    CHECK(h.mem.count_of(h.a) == 100 && h.mem.count_of(h.b) == 1 && h.mem.count_of(h.c) == 7);
    CHECK(h.mem.count_of(h.view) == 0 && h.mem.count_of((float *)nullptr) == 0);
    h.a[99] = 1.0f;
    h.view[49] = 2.0f;
    h.pinned[15] = 3u;
  }
  CHECK(nothing_live());

  {  // ensure: nothing at or below what is held, a new allocation above it
    DevMem m;
    float *p = nullptr;
    CHECK(!m.ensure(p, 0) && p == nullptr && g_allocs == 0);  // (a null pointer holds 0 elements)
    CHECK(m.ensure(p, 10) && p != nullptr && m.count_of(p) == 10 && g_allocs == 1);
    float *first = p;
    CHECK(!m.ensure(p, 10) && p == first);
    CHECK(!m.ensure(p, 3) && p == first && m.count_of(p) == 10);
    CHECK(m.ensure(p, 11) && m.count_of(p) == 11 && g_allocs == 1 && g_bytes == 44);
    p[10] = 1.0f;
    // a throwing ensure: null, no record, and the next one succeeds
    g_fail_in = 1;
    bool threw = false;
    try {
      m.ensure(p, 1000);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    CHECK(threw && p == nullptr && g_allocs == 0 && g_bytes == 0);
    CHECK(m.ensure(p, 1000) && p != nullptr && m.count_of(p) == 1000 && g_allocs == 1);
    p[999] = 1.0f;
    // a view handed to ensure is replaced, never freed
    float *view = p + 500;
    CHECK(m.ensure(view, 5) && view != p + 500 && m.count_of(view) == 5 && m.count_of(p) == 1000 && g_allocs == 2);
  }
  CHECK(nothing_live());

  // a create that throws on its k-th allocation: nothing is left once the owner is gone (first, middle, last)
  for (int k : {1, 2, CREATE_ALLOCATIONS}) {
    bool threw = false;
    try {
      Handle h;
      g_fail_in = k;
      create(h);
    } catch (const std::runtime_error &) {
      threw = true;
    }
    CHECK(threw);
    CHECK(nothing_live());
    g_fail_in = 0;
  }

  {  // release: nulls, frees once; releasing a view or a null pointer frees nothing
    Handle h;
    create(h);
    float *view = h.view;
    h.mem.release(view);
    CHECK(view == nullptr && g_allocs == 3);
    h.mem.release(h.a);
    CHECK(h.a == nullptr && g_allocs == 2 && g_bytes == 4 + 7 * 8);
    h.mem.release(h.a);
    CHECK(h.a == nullptr && g_allocs == 2);
    h.mem.release(h.pinned);
    CHECK(h.pinned == nullptr && g_host_allocs == 0);
  }
  CHECK(nothing_live());

  {  // a moved-from owner frees nothing; the new owner frees it all
    Handle h;
    create(h);
    {
      DevMem taken(std::move(h.mem));
      CHECK(taken.count_of(h.a) == 100 && h.mem.count_of(h.a) == 0);
      DevMem other;
      float *q = other.alloc<float>(3);
      other = std::move(taken);  // (what `other` held is freed by the assignment)
      CHECK(other.count_of(q) == 0 && other.count_of(h.a) == 100 && g_allocs == 3);
      h.mem = DevMem();  // the moved-from owner, destroyed in effect: nothing to free
      CHECK(g_allocs == 3 && g_host_allocs == 1);
      h.a[0] = 1.0f;  // still alive
    }
    CHECK(nothing_live());
  }
  CHECK(nothing_live());

  if (g_failures == 0) std::printf("dev_mem ok\n");
  return g_failures == 0 ? 0 : 1;
}
