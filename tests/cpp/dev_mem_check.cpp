// The scoped handles of uvio_amd/csrc/dev_mem.h on a host with no HIP device visible: empty handles, moves, swap,
// reset, and the failed allocation.  Built with the address and undefined-behaviour sanitizers and run directly
// (tests/test_host_structs.py), so a double release or a stranded allocation ends the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <utility>

#include "dev_mem.h"

using namespace uvhp;

// The handles own no host memory, so a leak report can only come from this program's own code or from the HIP / HSA
// runtime's start-up on a machine whose devices are hidden; the runtime's own allocations are not this test's.
extern "C" const char *__lsan_default_suppressions() { return "leak:libhsa-runtime64\nleak:libamdhip64\n"; }

#define CHECK(c)                                                       \
  do {                                                                 \
    if (!(c)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                    \
    }                                                                  \
  } while (0)

// No allocation can succeed here, so the moves get something to move by hand: the handle's two words (pointer,
// element count) are written in place and taken out again before the handle dies, so no HIP call sees the address.
template <class B>
static void plant(B &b, void *p, size_t n) {
  struct Words {
    void *p;
    size_t n;
  } w{p, n};
  static_assert(sizeof(B) == sizeof(Words), "handle: a pointer and a size");
  std::memcpy((void *)&b, &w, sizeof(w));
}

template <class B>
static void empty_semantics() {
  {
    B a;  // destructor of an empty handle: no call
    CHECK(a.get() == nullptr && a.size() == 0 && !a);
    a.reset();  // harmless
    a.reset();
    CHECK(a.get() == nullptr && a.size() == 0);
    B b(std::move(a));
    CHECK(!a && !b && a.size() == 0 && b.size() == 0);
    a = std::move(b);
    CHECK(!a && !b);
    std::swap(a, b);
    CHECK(!a && !b);
    a = std::move(a);  // self-assignment keeps the (empty) state
    CHECK(!a);
  }
}

template <class B>
static void move_semantics() {
  static double slab[8];
  B a;
  plant(a, slab, 8);
  CHECK(a.get() == slab && a.size() == 8);
  B c(std::move(a));  // move construction empties the source
  CHECK(!a && a.size() == 0 && c.get() == slab && c.size() == 8);
  B d;
  d = std::move(c);  // move assignment empties the source
  CHECK(!c && c.size() == 0 && d.get() == slab && d.size() == 8);
  B e;
  std::swap(d, e);  // swap: the content changes sides
  CHECK(!d && d.size() == 0 && e.get() == slab && e.size() == 8);
  double *raw = e;  // the implicit conversion, and pointer arithmetic and indexing through it
  CHECK(raw == slab && e + 2 == slab + 2 && &e[3] == slab + 3);
  plant(e, nullptr, 0);  // taken out: nothing reaches hipFree / hipHostFree
  CHECK(!e);
}

template <class B>
static void failed_allocation() {
  bool thrown = false;
  try {
    B a(1000);
    CHECK(false && "an allocation succeeded with no device visible");
  } catch (const HpError &e) {
    thrown = true;
    CHECK(e.code == UVIO_HP_E_DEVICE);
  }
  CHECK(thrown);
  // the same into an existing handle: it stays empty
  B b;
  try {
    b = B(0);
  } catch (const HpError &e) {
    CHECK(e.code == UVIO_HP_E_DEVICE);
  }
  CHECK(!b && b.size() == 0);
}

template <class H>
static void handle_semantics() {
  H a;
  CHECK(!a && a.get() == nullptr);
  a.reset();
  H b(std::move(a));
  a = std::move(b);
  std::swap(a, b);
  CHECK(!a && !b);
  bool thrown = false;
  try {
    a = H::create();
  } catch (const HpError &e) {
    thrown = true;
    CHECK(e.code == UVIO_HP_E_DEVICE);
  }
  CHECK(thrown && !a);
}

int main() {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    std::fprintf(stderr, "dev_mem_check: run with the devices hidden (HIP_VISIBLE_DEVICES=-1)\n");
    return 2;
  }
  static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value,
                "DevBuf is move-only");
  static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_constructible<Event>::value,
                "Stream / Event are move-only");
  static_assert(std::is_nothrow_move_constructible<DevBuf<double>>::value &&
                    std::is_nothrow_move_assignable<PinBuf<int>>::value,
                "moves do not throw");
  empty_semantics<DevBuf<double>>();
  empty_semantics<PinBuf<double>>();
  move_semantics<DevBuf<double>>();
  move_semantics<PinBuf<double>>();
  failed_allocation<DevBuf<double>>();
  failed_allocation<PinBuf<double>>();
  handle_semantics<Stream>();
  handle_semantics<Event>();
  std::printf("dev_mem_check: ok\n");
  return 0;
}
