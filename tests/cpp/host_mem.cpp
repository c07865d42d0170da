// host_mem.cpp -- the owner template of aither_amd/csrc/agx_mem.hpp over a counting backend
// (malloc / free): every allocation is freed exactly once, whatever moves, failures and
// growing vectors come between.  Built with the address and undefined-behaviour sanitizers;
// exits non-zero unless every property holds.
#include "../../aither_amd/csrc/agx_mem.hpp"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

namespace {
struct Counting {
  using error = int;
  static constexpr error ok = 0;
  static std::set<void*> live;
  static long allocs, frees, bad_frees;   // bad: double or foreign
  static bool fail_next;
  static error alloc(void** p, size_t bytes) {
    if (fail_next) { fail_next = false; *p = nullptr; return 7; }
    *p = malloc(bytes ? bytes : 1);
    live.insert(*p);
    ++allocs;
    return ok;
  }
  static void free(void* p) {
    if (live.erase(p) != 1) { ++bad_frees; return; }
    ++frees;
    ::free(p);
  }
  static error copy_in(void* dst, const void* src, size_t bytes) {
    memcpy(dst, src, bytes);
    return ok;
  }
};
std::set<void*> Counting::live;
long Counting::allocs = 0, Counting::frees = 0, Counting::bad_frees = 0;
bool Counting::fail_next = false;

using B = agx::Buf<double, Counting>;
struct Holder { int tag = 0; B a; agx::Buf<long, Counting> b; };

int failures = 0;
#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) { printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)
long live() { return (long)Counting::live.size(); }
}  // namespace

int main() {
  static_assert(noexcept(B(std::declval<B&&>())), "move construction is noexcept");
  static_assert(noexcept(std::declval<B&>() = std::declval<B&&>()), "move assignment is noexcept");
  static_assert(!std::is_copy_constructible<B>::value && !std::is_copy_assignable<B>::value,
                "an owner is not copied");
  {   // an empty owner frees nothing
    B e;
    CHECK(!e && e.get() == nullptr && e.size() == 0);
    e.reset();
  }
  CHECK(Counting::allocs == 0 && Counting::frees == 0 && Counting::bad_frees == 0);
  {   // alloc, out of scope: one free
    B x;
    CHECK(x.alloc(10) == 0 && x && x.size() == 10 && live() == 1);
    x.get()[9] = 1.0;
  }
  CHECK(Counting::allocs == 1 && Counting::frees == 1 && live() == 0);
  {   // alloc twice: the first allocation is freed exactly once
    B x;
    CHECK(x.alloc(4) == 0);
    CHECK(x.alloc(8) == 0 && x.size() == 8);
    CHECK(Counting::allocs == 3 && Counting::frees == 2 && live() == 1);
  }
  CHECK(Counting::frees == 3 && live() == 0);
  {   // a failing alloc leaves the owner empty; a later one works
    B x;
    CHECK(x.alloc(4) == 0);
    Counting::fail_next = true;
    CHECK(x.alloc(16) == 7);
    CHECK(!x && x.get() == nullptr && x.size() == 0 && live() == 0);
    CHECK(x.alloc(16) == 0 && x && x.size() == 16 && live() == 1);
    Counting::fail_next = true;
    bool grew = false;
    CHECK(x.reserve(32, &grew) == 7 && grew && !x && x.size() == 0 && live() == 0);
    Counting::fail_next = true;
    const std::vector<double> v(3, 1.0);
    CHECK(x.upload(v) == 7 && !x && live() == 0);
  }
  CHECK(live() == 0 && Counting::bad_frees == 0);
  {   // moves neither leak nor free twice
    B x;
    CHECK(x.alloc(5) == 0);
    double* const p = x.get();
    B y(std::move(x));
    CHECK(!x && x.size() == 0 && y.get() == p && y.size() == 5 && live() == 1);
    B z;
    CHECK(z.alloc(6) == 0 && live() == 2);
    z = std::move(y);                      // (frees z's own)
    CHECK(!y && z.get() == p && z.size() == 5 && live() == 1);
    B& zr = z;
    z = std::move(zr);                     // self-move-assignment
    CHECK(z.get() == p && z.size() == 5 && live() == 1);
    z.get()[4] = 2.0;
  }
  CHECK(live() == 0 && Counting::bad_frees == 0 && Counting::allocs == Counting::frees);
  {   // a vector of structs holding owners, grown past its capacity several times
    std::vector<Holder> v;
    size_t regrown = 0, cap = v.capacity();
    for (int n = 0; n < 100; ++n) {
      v.emplace_back();
      v.back().tag = n;
      CHECK(v.back().a.alloc(n + 1) == 0);
      if (n % 3 == 0) CHECK(v.back().b.alloc(2) == 0);
      v.back().a.get()[n] = n;
      if (v.capacity() != cap) { ++regrown; cap = v.capacity(); }
    }
    CHECK(regrown >= 3);
    CHECK(live() == 100 + 34);
    for (int n = 0; n < 100; ++n)
      CHECK(v[n].tag == n && v[n].a.size() == (size_t)n + 1 && v[n].a.get()[n] == n);
    v.clear();
    CHECK(live() == 0);
  }
  CHECK(Counting::bad_frees == 0 && Counting::allocs == Counting::frees);
  {   // reserve grows only, and says when it reallocated
    B x;
    bool grew = true;
    CHECK(x.reserve(0, &grew) == 0 && !grew && !x);
    CHECK(x.reserve(8, &grew) == 0 && grew && x.size() == 8);
    double* const p = x.get();
    CHECK(x.reserve(8, &grew) == 0 && !grew && x.get() == p && x.size() == 8);
    CHECK(x.reserve(3, &grew) == 0 && !grew && x.get() == p && x.size() == 8);
    const long before = Counting::frees;
    CHECK(x.reserve(9, &grew) == 0 && grew && x.size() == 9 && Counting::frees == before + 1);
    CHECK(live() == 1);
  }
  {   // upload: an empty vector leaves the owner empty with success, a full one is held
    agx::Buf<long, Counting> x;
    CHECK(x.upload(std::vector<long>()) == 0 && !x && x.size() == 0 && live() == 0);
    const std::vector<long> v = {3, 1, 4, 1, 5, 9, 2, 6};
    CHECK(x.upload(v) == 0 && x.size() == v.size() && live() == 1);
    for (size_t n = 0; n < v.size(); ++n) CHECK(x.get()[n] == v[n]);
    CHECK(x.upload(v.data(), 3) == 0 && x.size() == 3 && x.get()[2] == 4 && live() == 1);
    CHECK(x.upload(std::vector<long>()) == 0 && !x && live() == 0);   // (and frees what was held)
  }
  CHECK(live() == 0);
  CHECK(Counting::bad_frees == 0);
  CHECK(Counting::allocs == Counting::frees);
  if (failures) { printf("host_mem: %d checks failed\n", failures); return 1; }
  printf("host_mem OK: %ld allocations, %ld frees\n", Counting::allocs, Counting::frees);
  return 0;
}
