// res_owner.cpp -- the owning types of the engine's device resources
// (drb_res.hpp: Buf, Handle) on a counting fake allocator.
//
// The fake allocates with malloc, keeps the live count and the totals of
// allocations and frees, and fails the N-th allocation on request; the fake
// handle is a non-zero int whose destroy call is counted.  Checks that
//   - reserve at or below the capacity does not allocate;
//   - growth frees exactly one allocation and makes exactly one;
//   - over a sequence of mixed reserves on several buffers, failing the
//     N-th allocation (every N) leaves that buffer {nullptr, 0}, the others
//     as they were, and as many live allocations as non-null buffers;
//   - move construction and move assignment hand the allocation over, leave
//     the source empty and free once;
//   - a struct of several Buf and Handle members built behind a unique_ptr
//     and abandoned at each construction step leaves nothing live (what a
//     lazily built engine state relies on to be published only complete);
//   - a Handle destroys once, and never a null handle.
//
// Built by tests/test_res_owner.py with -fsanitize=address,undefined and run
// with leak detection.  Prints "ok <checks>" and exits 0, or the first
// mismatch and 1.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <utility>

#include "../../dragonboat_amd/csrc/drb_res.hpp"

static long g_live = 0, g_allocs = 0, g_frees = 0;
static long g_fail_at = 0;  // fail the allocation that makes g_allocs this
static long g_hlive = 0, g_hdestroyed = 0, g_hnext = 0;
static unsigned long long g_checked = 0;

#define CHECK(c)                                              \
  do {                                                        \
    ++g_checked;                                              \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      exit(1);                                                \
    }                                                         \
  } while (0)

struct Fake {
  static int alloc(void **p, size_t n) {
    if (++g_allocs == g_fail_at) {
      *p = (void *)0x1;  // (a failing allocator may scribble on *p)
      return 7;
    }
    *p = malloc(n ? n : 1);
    ++g_live;
    return 0;
  }
  static void free(void *p) {
    ::free(p);
    --g_live;
    ++g_frees;
  }
};
struct FakeDestroy {
  static bool null(int h) { return h == 0; }
  static void destroy(int h) {
    if (h == 0) {
      printf("FAIL: a null handle destroyed\n");
      exit(1);
    }
    --g_hlive;
    ++g_hdestroyed;
  }
};
using B = drb::Buf<Fake>;
using H = drb::Handle<int, FakeDestroy>;

static int hcreate(H &h, bool ok = true) {
  int *o = h.out();
  if (!ok) return 1;
  *o = (int)++g_hnext;
  ++g_hlive;
  return 0;
}

static void reset_counts() {
  CHECK(g_live == 0 && g_hlive == 0);
  g_allocs = g_frees = g_fail_at = 0;
  g_hdestroyed = 0;
}

static void test_reserve() {
  reset_counts();
  {
    B b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(0) == 0 && g_allocs == 0 && b.p == nullptr);
    CHECK(b.reserve(100) == 0 && b.p && b.cap == 100);
    CHECK(g_allocs == 1 && g_frees == 0 && g_live == 1);
    void *p = b.p;
    CHECK(b.reserve(100) == 0 && b.reserve(1) == 0 && b.reserve(0) == 0);
    CHECK(b.p == p && b.cap == 100 && g_allocs == 1 && g_frees == 0);
    CHECK(b.as<uint32_t>() == (uint32_t *)p);
    b.as<uint8_t>()[99] = 1;  // (the capacity is real: ASan watches)
    CHECK(b.reserve(101) == 0 && b.cap == 101);
    CHECK(g_allocs == 2 && g_frees == 1 && g_live == 1);
    b.as<uint8_t>()[100] = 1;
    g_fail_at = 3;
    CHECK(b.reserve(1000) == 7);
    CHECK(b.p == nullptr && b.cap == 0 && g_live == 0 && g_frees == 2);
    CHECK(b.reserve(10) == 0 && b.cap == 10 && g_live == 1);  // and recovers
  }
  CHECK(g_live == 0 && g_allocs == g_frees + 1);  // (one failed)
}

// mixed reserves over three buffers; the N-th allocation fails, every N
static void test_fail_every_n() {
  static const struct {
    int b;
    size_t need;
  } seq[] = {{0, 16}, {1, 64}, {0, 8},   {2, 1},   {0, 32}, {1, 64},
             {1, 65}, {2, 4096}, {0, 32}, {2, 100}, {0, 33}, {1, 1 << 16}};
  const int n = sizeof(seq) / sizeof(seq[0]);
  long total = 0;
  for (long fail = 0;; ++fail) {  // 0: none fails (counts the allocations)
    reset_counts();
    g_fail_at = fail;
    bool failed = false;
    {
      B b[3];
      for (int i = 0; i < n; ++i) {
        void *p[3] = {b[0].p, b[1].p, b[2].p};
        size_t cap[3] = {b[0].cap, b[1].cap, b[2].cap};
        const long before = g_allocs;
        const int rc = b[seq[i].b].reserve(seq[i].need);
        const bool grew = g_allocs != before;
        CHECK(grew == (seq[i].need > cap[seq[i].b]));
        CHECK(g_allocs - before <= 1);
        for (int k = 0; k < 3; ++k)
          if (k != seq[i].b) CHECK(b[k].p == p[k] && b[k].cap == cap[k]);
        B &x = b[seq[i].b];
        if (grew && g_allocs == fail) {
          failed = true;
          CHECK(rc != 0 && x.p == nullptr && x.cap == 0);
        } else {
          CHECK(rc == 0 && x.p && x.cap >= seq[i].need);
          if (grew) CHECK(x.cap == seq[i].need);
          x.as<uint8_t>()[x.cap - 1] = 1;
        }
        CHECK(g_live == (b[0].p != 0) + (b[1].p != 0) + (b[2].p != 0));
        for (int k = 0; k < 3; ++k) CHECK((b[k].p == nullptr) == (b[k].cap == 0));
      }
      if (fail == 0) total = g_allocs;
    }
    CHECK(g_live == 0);
    CHECK(failed == (fail >= 1 && fail <= total));
    // (a failure makes the next reserve of that buffer grow again, so a
    // failing run may allocate more often than the clean one)
    if (fail > total) break;
  }
  CHECK(total >= 8);
}

static void test_moves() {
  reset_counts();
  {
    B a;
    CHECK(a.reserve(40) == 0);
    void *p = a.p;
    B b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == p && b.cap == 40);
    CHECK(g_live == 1 && g_frees == 0);
    B c;
    CHECK(c.reserve(8) == 0 && g_live == 2);
    c = std::move(b);  // frees c's own, takes b's
    CHECK(b.p == nullptr && b.cap == 0 && c.p == p && c.cap == 40);
    CHECK(g_live == 1 && g_frees == 1);
    B &self = c;
    c = std::move(self);
    CHECK(c.p == p && c.cap == 40 && g_live == 1);
    CHECK(a.reserve(4) == 0 && g_live == 2);  // a moved-from buffer is usable
  }
  CHECK(g_live == 0 && g_allocs == g_frees);
  {
    H a;
    CHECK(!a && (int)a == 0);
    CHECK(hcreate(a) == 0 && a && g_hlive == 1);
    const int v = a;
    H b(std::move(a));
    CHECK(!a && (int)b == v && g_hlive == 1 && g_hdestroyed == 0);
    H c;
    CHECK(hcreate(c) == 0 && g_hlive == 2);
    c = std::move(b);
    CHECK(!b && (int)c == v && g_hlive == 1 && g_hdestroyed == 1);
    CHECK(hcreate(c) == 0 && g_hlive == 1 && g_hdestroyed == 2);  // replaced
  }
  CHECK(g_hlive == 0 && g_hdestroyed == 3);
  {
    H never;  // null from start to end: FakeDestroy exits on a null destroy
    H failed;
    CHECK(hcreate(failed, false) != 0 && !failed);
  }
  CHECK(g_hlive == 0 && g_hdestroyed == 3);
}

// a lazily built state as the engine's: built behind a unique_ptr, handed
// over (release) only when every step succeeded
struct State {
  H stream;
  B a, b;
  H ev[2];
  B out;
};
static State *g_published = nullptr;
static int state_init(int stop_at) {
  int step = 0;
  auto fails = [&]() { return ++step == stop_at; };
  std::unique_ptr<State> s(new State());
  if (fails() || hcreate(s->stream)) return 1;
  if (fails() || s->a.reserve(24)) return 1;
  if (fails() || s->b.reserve(48)) return 1;
  for (H &e : s->ev)
    if (fails() || hcreate(e)) return 1;
  if (fails() || s->out.reserve(1 << 12)) return 1;
  g_published = s.release();
  return 0;
}
static void test_abandoned_state() {
  const int steps = 6;
  for (int stop = 1; stop <= steps; ++stop) {
    reset_counts();
    g_published = nullptr;
    CHECK(state_init(stop) != 0);
    CHECK(g_published == nullptr && g_live == 0 && g_hlive == 0);
    CHECK(g_allocs == g_frees);
  }
  // and by the allocator's own failure at each of its three allocations
  for (long fail = 1; fail <= 3; ++fail) {
    reset_counts();
    g_fail_at = fail;
    CHECK(state_init(0) != 0 && g_published == nullptr);
    CHECK(g_live == 0 && g_hlive == 0);
  }
  reset_counts();
  CHECK(state_init(0) == 0 && g_published);
  CHECK(g_live == 3 && g_hlive == 3);
  delete g_published;
  CHECK(g_live == 0 && g_hlive == 0 && g_hdestroyed == 3 && g_frees == 3);
}

int main() {
  test_reserve();
  test_fail_every_n();
  test_moves();
  test_abandoned_state();
  printf("ok %llu\n", g_checked);
  return 0;
}
